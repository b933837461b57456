// Per-pair flag bits of a diff pass and the wave-level helpers its kernels share (kernels.hip K2-K6,
// smallpass.hip K20).  Device code for gfx950 (wave64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gpudiff.h"

namespace gd {

// per-pair flag byte written by K2: bits 0-2 are the public GPUDIFF_* result
// bits; bits 3-6 are internal hints for K4/K6 (masked off on the host)
constexpr uint32_t F_SPEC = 1u, F_STATUS = 2u, F_ERR = 4u;
constexpr uint32_t F_SENT = 8u;    // status-absent-in-new sentinel path
constexpr uint32_t F_JSPEC = 16u;  // spec region needs the merge-join
constexpr uint32_t F_JSTAT = 32u;  // status region needs the merge-join
constexpr uint32_t F_SEED = 64u;   // pair path-hash seed != 0
constexpr uint32_t F_DEFER = 128u; // paths not produced by K2 (wave arena full): K4 joins it
constexpr uint32_t ARENA_BIT = 0x80000000u;  // scratch_off[d]: paths live in the K2 wave arenas

// K4 merge-path slices (k_join_slices below)
constexpr uint32_t kJoinSlice = 1024;  // merged keys per slice (<= 16 windows of 64 + 64)
constexpr uint32_t kDeepJoin = 2048;   // K2 defers a dirty pair whose join covers more keys
constexpr uint32_t kTailJoinMax = 1024;  // K2's largest-first rounds: joins over this many keys go to K4's slices

// Scratch entries of a deferred pair.  need = the merged keys of each joined region + the status-absent
// sentinel (when the pair has one) bounds its paths.  A pair with need <= kJoinSlice -- one K2 deferred
// only because its wave arena was full -- is a *whole* deferral: exactly need entries, joined by one
// wave in K3 (k_compact).  A larger one is *sliced*: each region's merged keys in kJoinSlice-key slices,
// every slice writing at its own kJoinSlice-entry offset, so the cap is a whole number of slices (and at
// least need, for the sentinel after the packed paths); a sliced cap is therefore >= 2 * kJoinSlice and
// cap <= kJoinSlice tells the two kinds apart.
constexpr uint32_t kNoOwner = 0xFFFFFFFFu;  // slot_owner of a slot inside a whole deferral's entries
__device__ __forceinline__ uint32_t defer_cap(uint32_t spec_l_a, uint32_t spec_l_b, uint32_t stat_l_a,
                                              uint32_t stat_l_b, uint32_t f) {
    const uint32_t Ls = (f & F_JSPEC) ? spec_l_a + spec_l_b : 0u;
    const uint32_t Lt = (f & F_JSTAT) ? stat_l_a + stat_l_b : 0u;
    const uint32_t need = Ls + Lt + ((f & F_SENT) ? 1u : 0u);
    if (need <= kJoinSlice) return need;
    const uint32_t slices = (Ls + kJoinSlice - 1u) / kJoinSlice + (Lt + kJoinSlice - 1u) / kJoinSlice;
    return max(slices, (need + kJoinSlice - 1u) / kJoinSlice) * kJoinSlice;
}
__device__ __forceinline__ uint32_t sat_add(uint32_t a, uint32_t b) {
    const uint32_t s = a + b;
    return s < a ? 0xFFFFFFFFu : s;
}


// ---------------------------------------------------------------- wave helpers
__device__ __forceinline__ uint32_t lane_id() { return __lane_id(); }

__device__ __forceinline__ uint32_t shfl32(uint32_t v, uint32_t src) {
    return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src << 2), (int)v);
}
__device__ __forceinline__ uint64_t shfl64(uint64_t v, uint32_t src) {
    uint32_t lo = shfl32((uint32_t)v, src), hi = shfl32((uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t ballot(bool p) { return __ballot(p); }
__device__ __forceinline__ uint32_t popc64(uint64_t m) { return (uint32_t)__popcll(m); }
__device__ __forceinline__ uint64_t mask_lt(uint32_t n) { return n >= 64 ? ~0ULL : ((1ULL << n) - 1ULL); }

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
    const uint32_t lane = lane_id();
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        uint32_t o = shfl32(v, lane >= d ? lane - d : lane);
        if (lane >= d) v += o;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (uint32_t d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, (int)d);
    return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (uint32_t d = 32; d >= 1; d >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, (int)d));
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (uint32_t d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, (int)d));
    return v;
}
__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// must equal gpudiff_seg_bytes / gpudiff_meta_is_long / gpudiff_meta_arena (gpudiff_format.h); why restated: DESIGN.md §4j
__device__ __forceinline__ uint64_t seg_bytes(uint32_t l, uint32_t arena) { return (uint64_t)l * 16u + arena; }
__device__ __forceinline__ bool meta_long(uint32_t m) { return (m & 7u) == GPUDIFF_TAG_STR && (m >> 3) > 8u; }
// arena bytes of a leaf's value: a long string's tail past its first 8 bytes (which sit in vals), at a
// 4-byte aligned offset (include/gpudiff_format.h)
__device__ __forceinline__ uint32_t meta_arena(uint32_t m) { return meta_long(m) ? (((m >> 3) - 8u + 3u) & ~3u) : 0u; }

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool neq16(const u32x4& a, const u32x4& b) {
    const u32x4 x = a ^ b;
    return (x.x | x.y | x.z | x.w) != 0u;
}

}  // namespace gd
