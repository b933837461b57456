// Changed leaves' old and new values as JSON text (gfx950, wave64): GPUDIFF_OPT_PATH_VALUES renders, for every
// (path hash, kind) a diffed batch reports, A's and B's leaf from the segments the blobs carry in HBM
// (include/gpudiff_format.h), with the routine of valstr.h -- the same one the host entry point runs.
//
//   K21 k_value_len    wave per dirty pair, lanes striding over the pair's changed-path entries, once per side:
//                      the leaf by binary search of keys[], its tag, the arena offsets of the side's long changed
//                      leaves in one forward sweep over metas[] (64 leaves a step, wave scan, running base), the
//                      text's length -- a lane's own work for short values, the whole wave's (lane per byte) for
//                      long strings; (leaf, arena offset) cached per entry and side; a counter of unresolved values
//   scan               exclusive u64 scan of the 2 * n_paths lengths (scan64.h: sums and total, then the offsets)
//   K22 k_value_write  the same mapping; each text into its slot, packed back to back, no terminator; long strings
//                      by the whole wave with a scan per 64 bytes, the rest a lane per value
//
// K21 chases dependent loads (the searches): latency-bound, one pair's lanes on one pair's segments.  No LDS
// beyond what a wave's own scans use, no spin-waits, no atomics other than the unresolved counter.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gpudiff.h"
#include "scan64.h"
#include "tokdev.h"
#include "values.h"
#include "valstr.h"

namespace gd {

namespace {

// Go's shortest float64 text on the device (tokdev.h; the canonical value holds no negative zero)
struct DevFloat {
    __device__ __forceinline__ uint64_t operator()(uint64_t bits, uint8_t* o) const {
        return go_float_put(bits, false, o);
    }
};

// the region's segment of one side (0 = A, 1 = B) of row r; l = 0 when it does not lie inside the space
__device__ __forceinline__ ValSeg entry_seg(const ValueJob& j, const gpudiff_pair_row& r, uint32_t side, bool status) {
    const uint64_t off = side ? r.off_b : r.off_a;
    if (off > j.space_bytes) return val_seg(j.space, 0, 0, 0, 0, 0, false);
    return side ? val_seg(j.space + off, j.space_bytes - off, r.spec_l_b, r.spec_ar_b, r.stat_l_b, r.stat_ar_b, status)
                : val_seg(j.space + off, j.space_bytes - off, r.spec_l_a, r.spec_ar_a, r.stat_l_a, r.stat_ar_a, status);
}

// seg[reg] for a per-lane reg, field by field (a dynamically indexed private array would live in scratch)
__device__ __forceinline__ ValSeg seg_of(const ValSeg (&seg)[2], uint32_t reg) {
    ValSeg s;
    s.vals = reg ? seg[1].vals : seg[0].vals;
    s.keys = reg ? seg[1].keys : seg[0].keys;
    s.metas = reg ? seg[1].metas : seg[0].metas;
    s.arena = reg ? seg[1].arena : seg[0].arena;
    s.l = reg ? seg[1].l : seg[0].l;
    s.ar = reg ? seg[1].ar : seg[0].ar;
    s.ok = reg ? seg[1].ok : seg[0].ok;
    return s;
}

// entry kind k has a value on this side: CHANGED both, ADDED new only, REMOVED old only, the sentinel neither
__device__ __forceinline__ bool side_present(uint32_t k, uint32_t side) {
    const uint32_t kind = k & 3u;
    return kind == GPUDIFF_PATH_CHANGED || kind == (side ? GPUDIFF_PATH_ADDED : GPUDIFF_PATH_REMOVED);
}

// inclusive wave scan of values below 2^32 whose sum may pass it: two 32-bit DPP scans, of the low 24 bits and
// of the rest (64 lanes of 2^24 and of 2^8 both stay below 2^32)
__device__ __forceinline__ uint64_t wave_incl_scan_wide(uint32_t v) {
    const uint32_t lo = wave_incl_scan(v & 0xFFFFFFu), hi = wave_incl_scan(v >> 24);
    return ((uint64_t)hi << 24) + lo;
}

// lane l's leaf in every lane (a long string: head, tail and length are all that is read)
__device__ __forceinline__ ValLeaf leaf_of_lane(const ValLeaf& v, uint32_t l) {
    ValLeaf b;
    b.head = rdlane64(v.head, l);
    b.tail = (const uint8_t*)rdlane64((uint64_t)v.tail, l);
    b.tag = GPUDIFF_TAG_STR;
    b.len = rdlane(v.len, l);
    b.ok = true;
    return b;
}

__global__ __launch_bounds__(256) void k_value_len(const ValueJob j, uint8_t* __restrict__ tags,
                                                   uint64_t* __restrict__ lens, ValueSlot* __restrict__ slots,
                                                   unsigned long long* __restrict__ unresolved) {
    const uint32_t lane = __lane_id();
    const uint32_t d = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (d >= j.n_dirty) return;
    const uint32_t e0 = j.path_off[d], e1 = min(j.path_off[d + 1], j.n_paths);
    if (e0 >= e1) return;
    const gpudiff_pair_row r = j.rows[j.dirty_idx[d]];
    uint32_t bad = 0;
    for (uint32_t side = 0; side < 2; side++) {
        const ValSeg seg[2] = {entry_seg(j, r, side, false), entry_seg(j, r, side, true)};
        // the sweep over each region's metas: leaves [0, pos) sum to base arena bytes (wave-uniform)
        uint32_t pos[2] = {0, 0};
        uint64_t base[2] = {0, 0};
        for (uint32_t c0 = e0; c0 < e1; c0 += 64) {  // every lane runs every step: the scans need the whole wave
            const uint32_t e = c0 + lane;
            const bool act = e < e1;
            const uint32_t k = act ? j.out_k[e] : GPUDIFF_PATH_STATUS_ABSENT;
            const uint64_t h = act ? j.out_h[e] : 0;
            const uint32_t reg = k >> 7;
            const bool present = act && side_present(k, side);
            const ValSeg sg = seg_of(seg, reg);
            uint32_t idx = kValNoLeaf, m = 0;
            if (present && !(h & ~j.mask)) {
                idx = val_find(sg, h);
                if (idx != kValNoLeaf) m = val_meta(sg, idx);
            }
            const bool is_long = idx != kValNoLeaf && gpudiff_meta_is_long(m);
            uint64_t aoff = 0;
#pragma unroll
            for (uint32_t g = 0; g < 2; g++) {
                const bool need = is_long && reg == g;
                if (!ballot(need)) continue;
                if (ballot(need && idx < pos[g])) {  // not ascending (no list the engine wrote): sweep again
                    pos[g] = 0;
                    base[g] = 0;
                }
                const uint32_t last = wave_max(need ? idx : 0u);
                for (;;) {
                    const uint32_t li = pos[g] + lane;
                    const uint32_t a = li < seg[g].l ? gpudiff_meta_arena(val_meta(seg[g], li)) : 0u;
                    const uint64_t inc = wave_incl_scan_wide(a);
                    const uint64_t excl = inc - a;
                    const uint32_t src = (idx - pos[g]) & 63u;
                    const uint64_t mine =
                        ((uint64_t)shfl32((uint32_t)(excl >> 32), src) << 32) | shfl32((uint32_t)excl, src);
                    if (need && idx >= pos[g] && idx - pos[g] < 64u) aoff = base[g] + mine;
                    if (last - pos[g] < 64u) break;  // the sweep rests on the step that holds the last leaf asked for
                    base[g] += rdlane64(inc, 63);
                    pos[g] += 64;
                }
            }
            ValLeaf v = val_leaf(sg, idx, aoff);  // idx = kValNoLeaf: not ok
            if (is_long && aoff > 0xFFFFFFFFull) v.ok = false;
            uint64_t len = 0;
            if (present && v.ok && !is_long) len = val_text_len(v, DevFloat());
            // long strings: the whole wave sizes each, a lane per decoded byte
            for (uint64_t todo = ballot(present && v.ok && is_long); todo; todo &= todo - 1) {
                const uint32_t l = (uint32_t)__builtin_ctzll(todo);
                const ValLeaf b = leaf_of_lane(v, l);
                uint32_t acc = 0;
                for (uint32_t i = lane; i < b.len; i += 64) acc += val_esc_unit(b, b.len, i);
                const uint32_t sum = wave_sum(acc);  // len < 2^29: at most 6 * len + 2 < 2^32
                if (lane == l) len = (uint64_t)sum + 2u;
            }
            if (act) {
                const bool ok = present && v.ok;
                if (present && !ok) bad++;
                tags[2ull * e + side] = ok ? (uint8_t)v.tag : (uint8_t)GPUDIFF_VALUE_ABSENT;
                lens[2ull * e + side] = ok ? len : 0;
                slots[2ull * e + side] = ValueSlot{ok ? idx : kValNoLeaf, (uint32_t)aoff};
            }
        }
    }
    if (bad) atomicAdd(unresolved, (unsigned long long)bad);
}

__global__ __launch_bounds__(256) void k_value_write(const ValueJob j, const uint8_t* __restrict__ tags,
                                                     const ValueSlot* __restrict__ slots,
                                                     const uint64_t* __restrict__ offsets, uint8_t* __restrict__ bytes,
                                                     uint64_t bytes_cap, unsigned long long* __restrict__ unresolved) {
    const uint32_t lane = __lane_id();
    const uint32_t d = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (d >= j.n_dirty) return;
    const uint32_t e0 = j.path_off[d], e1 = min(j.path_off[d + 1], j.n_paths);
    if (e0 >= e1) return;
    const gpudiff_pair_row r = j.rows[j.dirty_idx[d]];
    uint32_t bad = 0;
    for (uint32_t side = 0; side < 2; side++) {
        const ValSeg seg[2] = {entry_seg(j, r, side, false), entry_seg(j, r, side, true)};
        for (uint32_t c0 = e0; c0 < e1; c0 += 64) {
            const uint32_t e = c0 + lane;
            const bool act = e < e1;
            const uint64_t t = 2ull * e + side;
            bool present = act && tags[t] != GPUDIFF_VALUE_ABSENT;
            uint64_t o0 = 0, len = 0;
            if (present) {
                o0 = offsets[t];
                const uint64_t o1 = offsets[t + 1];
                if (o1 < o0 || o1 > bytes_cap) {  // the slot does not lie inside the buffer: nothing is written
                    bad++;
                    present = false;
                } else {
                    len = o1 - o0;
                }
            }
            ValLeaf v = val_leaf(seg[0], kValNoLeaf, 0);
            if (present) {
                const ValueSlot sl = slots[t];
                v = val_leaf(seg_of(seg, (uint32_t)j.out_k[e] >> 7), sl.leaf, sl.arena);
            }
            uint8_t* dst = bytes + o0;
            const bool is_long = present && v.ok && v.tag == GPUDIFF_TAG_STR && v.len > GPUDIFF_INLINE_MAX;
            bool fail = present && !is_long && !val_text_write(v, dst, len, DevFloat());
            // long strings: the whole wave writes each, a scan per 64 decoded bytes; no store outside [o0, o0 + len)
            for (uint64_t todo = ballot(is_long); todo; todo &= todo - 1) {
                const uint32_t l = (uint32_t)__builtin_ctzll(todo);
                const ValLeaf b = leaf_of_lane(v, l);
                uint8_t* o = (uint8_t*)rdlane64((uint64_t)dst, l);
                const uint64_t n = rdlane64(len, l);
                uint64_t run = 1;  // behind the opening quote
                for (uint32_t b0 = 0; b0 < b.len; b0 += 64) {
                    const uint32_t i = b0 + lane;
                    const uint32_t u = i < b.len ? val_esc_unit(b, b.len, i) : 0u;
                    const uint32_t inc = wave_incl_scan(u);
                    const uint64_t p = run + inc - u;
                    if (u && n >= 2 && p + u <= n - 1) val_esc_emit(b, i, u, o + p);
                    run += rdlane(inc, 63);
                }
                const bool fits = n >= 2 && run == n - 1;
                if (lane == 0 && fits) {
                    o[0] = '"';
                    o[n - 1] = '"';
                }
                if (lane == l && !fits) fail = true;
            }
            if (fail) {
                for (uint64_t q = 0; q < len; q++) dst[q] = 0;
                bad++;
            }
        }
    }
    if (bad) atomicAdd(unresolved, (unsigned long long)bad);
}

}  // namespace

hipError_t launch_value_len(hipStream_t s, const ValueJob& j, uint8_t* tags, uint64_t* lens, ValueSlot* slots,
                            uint64_t* tile_sums, unsigned long long* total, unsigned long long* unresolved) {
    hipError_t e = hipMemsetAsync(total, 0, 8, s);
    if (e != hipSuccess || (e = hipMemsetAsync(unresolved, 0, 8, s)) != hipSuccess || !j.n_paths) return e;
    // an entry no dirty pair's range covers (none, by K6's CSR) would otherwise scan an unwritten length
    if ((e = hipMemsetAsync(lens, 0, 16ull * j.n_paths, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(tags, GPUDIFF_VALUE_ABSENT, 2ull * j.n_paths, s)) != hipSuccess) return e;
    k_value_len<<<(j.n_dirty + 3) / 4, 256, 0, s>>>(j, tags, lens, slots, unresolved);
    return launch_scan64_sums(s, lens, 2u * j.n_paths, tile_sums, (uint64_t*)total);
}

hipError_t launch_value_write(hipStream_t s, const ValueJob& j, const uint8_t* tags, const uint64_t* lens,
                              const ValueSlot* slots, const uint64_t* tile_sums, uint64_t* offsets, uint8_t* bytes,
                              uint64_t bytes_cap, unsigned long long* unresolved) {
    if (!j.n_paths) return hipMemsetAsync(offsets, 0, 8, s);
    const hipError_t e = launch_scan64_offsets(s, lens, 2u * j.n_paths, tile_sums, offsets);
    if (e != hipSuccess) return e;
    k_value_write<<<(j.n_dirty + 3) / 4, 256, 0, s>>>(j, tags, slots, offsets, bytes, bytes_cap, unresolved);
    return hipGetLastError();
}

}  // namespace gd
