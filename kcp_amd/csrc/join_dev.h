// The merge-join of one pair's changed paths (K4's core), shared by every kernel that joins: K2's in-place
// joins, K3's whole deferrals and K4's slices (kernels.hip) and the fused small pass K20 (smallpass.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gpudiff.h"
#include "wave_dev.h"
#include "xxh64.h"

namespace gd {

struct RegionView {
    const uint32_t* keys;
    const uint64_t* vals;
    const uint32_t* metas;
    const uint8_t* arena;
    uint32_t L;
};

__device__ __forceinline__ RegionView region_view(const uint8_t* pool, uint64_t off, uint32_t sl, uint32_t sar,
                                                  bool status, uint32_t L) {
    const uint8_t* seg = pool + off + (status ? seg_bytes(sl, sar) : 0);
    RegionView v;
    v.vals = (const uint64_t*)seg;  // vals u64 | keys u32 | metas u32 | arena (include/gpudiff_format.h)
    v.keys = (const uint32_t*)(seg + 8ull * L);
    v.metas = (const uint32_t*)(seg + 12ull * L);
    v.arena = seg + 16ull * L;
    v.L = L;
    return v;
}

// number of tile keys (lanes < nt, ascending) strictly less than x
__device__ __forceinline__ uint32_t tile_lower_bound(uint32_t x, uint32_t tile, uint32_t nt) {
    uint32_t j = 0;
#pragma unroll
    for (uint32_t s = 64; s >= 1; s >>= 1) {
        const uint32_t cand = j + s;
        const uint32_t t = shfl32(tile, min(cand, 64u) - 1u);
        if (cand <= nt && t < x) j = cand;
    }
    return j;
}

// Byte-exact confirmation of every lane's pending long value at once (same
// length, same first 8 bytes): the tails of len bytes in the two arenas.  The
// lanes' tails are flattened into one index space of dwords (prefix sum of
// dword counts: tails sit at 4-byte aligned arena offsets, zero padded to 4, so
// two equal-length tails are equal iff their padded dwords are); each pass the
// wave compares 64 x CV_U dwords (consecutive dwords of a tail are consecutive
// addresses), finding a dword's owner lane by a cross-lane binary search over
// the prefix sums.  No load reaches past a tail's padded end.  Returns true in
// the lanes whose tail differs.
__device__ bool confirm_values(bool need, const uint8_t* arena_a, uint32_t off_a, const uint8_t* arena_b,
                               uint32_t off_b, uint32_t len, uint32_t lane) {
    const uint32_t n4 = need ? (len + 3u) >> 2 : 0u;
    const uint32_t incl = wave_incl_scan(n4);
    const uint32_t total = shfl32(incl, 63);
    uint64_t bad = 0;  // lanes whose value differs (wave-uniform)
    constexpr int CV_U = 4;  // dword pairs in flight per lane
    for (uint32_t base = 0; base < total; base += 64 * CV_U) {
        uint32_t xa[CV_U], xb[CV_U];
        uint32_t own[CV_U];
        bool act[CV_U];
#pragma unroll
        for (int u = 0; u < CV_U; u++) {
            const uint32_t g = base + u * 64 + lane;
            act[u] = g < total;
            // owner = number of lanes whose inclusive dword prefix is <= g
            uint32_t o = 0;
#pragma unroll
            for (uint32_t s = 64; s >= 1; s >>= 1) {
                const uint32_t cand = o + s;
                const uint32_t t = shfl32(incl, min(cand, 64u) - 1u);
                if (cand <= 64u && t <= g) o = cand;
            }
            own[u] = min(o, 63u);
            const uint32_t oa = shfl32(off_a, own[u]), ob = shfl32(off_b, own[u]);
            const uint32_t first = shfl32(incl - n4, own[u]);
            if (act[u]) {
                const uint32_t k = g - first;
                xa[u] = *(const uint32_t*)(arena_a + oa + 4u * k);
                xb[u] = *(const uint32_t*)(arena_b + ob + 4u * k);
            }
        }
#pragma unroll
        for (int u = 0; u < CV_U; u++) {
            uint64_t m = ballot(act[u] && xa[u] != xb[u]);
            while (m) {  // values that differ only past their first 8 bytes
                const uint32_t j = (uint32_t)__builtin_ctzll(m);
                m &= m - 1;
                bad |= 1ull << shfl32(own[u], j);
            }
        }
    }
    return (bad >> lane) & 1ull;
}

// A changed leaf whose two values Go's json.Marshal writes as the same text
// and the API server decodes back to the same int64 (the write-path no-op rule,
// DESIGN.md §4g): an int64 v on one side, a float64 f == v on the other,
// |v| <= 2^53 (canonical values: int64 / float64 bits, -0.0 stored as +0.0).
__device__ __forceinline__ bool wire_equal_number(uint32_t ma, uint64_t xa, uint32_t mb, uint64_t xb) {
    const uint32_t ta = ma & 7u, tb = mb & 7u;
    if (!((ta == GPUDIFF_TAG_INT && tb == GPUDIFF_TAG_FLOAT) || (ta == GPUDIFF_TAG_FLOAT && tb == GPUDIFF_TAG_INT)))
        return false;
    const int64_t v = (int64_t)(ta == GPUDIFF_TAG_INT ? xa : xb);
    const double f = __longlong_as_double((long long)(ta == GPUDIFF_TAG_INT ? xb : xa));
    const int64_t lim = 1ll << 53;
    return v >= -lim && v <= lim && (double)v == f;
}

// Merge-join of one region; returns the number of paths emitted.  Emission
// order = ascending key (the union of both sorted key lists).  *weq_all: every
// emitted path is a CHANGED leaf with wire_equal_number values (wave-uniform).
template <bool EMIT>
__device__ uint32_t join_region(const RegionView& A, const RegionView& B, uint8_t region_bit,
                                uint64_t* __restrict__ out_h, uint8_t* __restrict__ out_k, uint32_t out_base,
                                uint32_t lane, bool* weq_all) {
    uint32_t ia = 0, ib = 0, arA = 0, arB = 0, outpos = 0;
    bool weq = true;
    const uint64_t lt = mask_lt(lane);
    while (ia < A.L || ib < B.L) {
        const uint32_t na = min(64u, A.L - ia), nb = min(64u, B.L - ib);
        const bool va = lane < na, vb = lane < nb;
        const uint32_t ka = va ? A.keys[ia + lane] : 0u;
        const uint32_t kb = vb ? B.keys[ib + lane] : 0u;
        const uint32_t ma = va ? A.metas[ia + lane] : 0u;
        const uint32_t mb = vb ? B.metas[ib + lane] : 0u;
        const uint64_t xa = va ? A.vals[ia + lane] : 0ull;
        const uint64_t xb = vb ? B.vals[ib + lane] : 0ull;
        const bool endA = ia + na == A.L, endB = ib + nb == B.L;
        const uint32_t lastA = na ? shfl32(ka, na - 1) : 0u;
        const uint32_t lastB = nb ? shfl32(kb, nb - 1) : 0u;
        // everything <= bound is resolvable in this window
        bool inf = true;
        uint32_t bound = 0;
        if (!endA) { bound = lastA; inf = false; }
        if (!endB) { bound = inf ? lastB : min(bound, lastB); inf = false; }
        const bool inA = va && (inf || ka <= bound);
        const bool inB = vb && (inf || kb <= bound);
        // arena offsets of this window's long values
        const uint32_t asA = meta_arena(ma), asB = meta_arena(mb);
        const uint32_t incA = wave_incl_scan(asA), incB = wave_incl_scan(asB);
        const uint32_t offA = arA + incA - asA, offB = arB + incB - asB;
        // resolve A keys against the B window
        const uint32_t jA = tile_lower_bound(ka, kb, nb);
        const uint32_t kbj = shfl32(kb, min(jA, 63u));
        const uint32_t mbj = shfl32(mb, min(jA, 63u));
        const uint64_t xbj = shfl64(xb, min(jA, 63u));
        const uint32_t obj = shfl32(offB, min(jA, 63u));
        const bool matchA = inA && jA < nb && kbj == ka;
        bool differ = matchA && (ma != mbj || xa != xbj);
        // equal head (the first 8 bytes, in vals) and length: confirm the tails in the arenas
        differ |= confirm_values(matchA && !differ && meta_long(ma), A.arena, offA, B.arena, obj, (ma >> 3) - 8u, lane);
        // resolve B keys against the A window
        const uint32_t iB = tile_lower_bound(kb, ka, na);
        const uint32_t kai = shfl32(ka, min(iB, 63u));
        const bool matchB = inB && iB < na && kai == kb;
        const bool emitA = inA && (!matchA || differ);
        const bool emitB = inB && !matchB;
        const uint64_t balA = ballot(emitA), balB = ballot(emitB);
        if (ballot((emitA && !(matchA && wire_equal_number(ma, xa, mbj, xbj))) || emitB)) weq = false;
        if (EMIT) {
            if (emitA) {
                const uint32_t pos = popc64(balA & lt) + popc64(balB & mask_lt(jA));
                out_h[out_base + outpos + pos] = ka;
                out_k[out_base + outpos + pos] = region_bit | (matchA ? GPUDIFF_PATH_CHANGED : GPUDIFF_PATH_REMOVED);
            }
            if (emitB) {
                const uint32_t pos = popc64(balB & lt) + popc64(balA & mask_lt(iB));
                out_h[out_base + outpos + pos] = kb;
                out_k[out_base + outpos + pos] = region_bit | GPUDIFF_PATH_ADDED;
            }
        }
        outpos += popc64(balA) + popc64(balB);
        const uint32_t ca = popc64(ballot(inA)), cb = popc64(ballot(inB));
        arA += ca ? shfl32(incA, ca - 1) : 0u;
        arB += cb ? shfl32(incB, cb - 1) : 0u;
        ia += ca;
        ib += cb;
    }
    *weq_all = weq;
    return outpos;
}

__device__ uint64_t status_sentinel_hash(uint32_t seed, uint64_t mask) {
    // XXH64 of the 11 path bytes 01 06 00 00 00 's' 't' 'a' 't' 'u' 's'
    // bytes: [0]=01 [1]=06 [2..4]=00 [5]='s' [6]='t' [7]='a' | [8]='t' [9]='u' [10]='s'
    uint64_t w[4] = {0, 0, 0, 0};
    w[0] = 0x01ull | (0x06ull << 8) | ((uint64_t)'s' << 40) | ((uint64_t)'t' << 48) | ((uint64_t)'a' << 56);
    w[1] = (uint64_t)'t' | ((uint64_t)'u' << 8) | ((uint64_t)'s' << 16);
    uint64_t h = (uint64_t)seed + XP5 + 11u;
    h = xxh64_tail(h, w, 11);
    return xavalanche(h) & mask;
}

// The write-path no-op bits of a dirty pair: bit 0 = the spec
// write (A's body over B) changes nothing deepEqualApartFromStatus compares
// (every changed spec leaf is a wire_equal_number change); bit 1 = the status
// write (B's status into A) changes nothing (every changed status leaf is one,
// and when B has no status key, A has none either).
constexpr uint32_t NOOP_SPEC = 1u, NOOP_STATUS = 2u;
__device__ __forceinline__ uint32_t sentinel_noop_bits(uint32_t flags_a) {
    return (flags_a & GPUDIFF_OBJ_HAS_STATUS) ? 0u : NOOP_STATUS;
}

template <bool EMIT>
__device__ uint32_t join_pair(const gpudiff_pair_row& r, uint32_t f, const uint8_t* pool, uint64_t mask,
                              uint64_t* out_h, uint8_t* out_k, uint32_t base, uint32_t lane, uint32_t* noop) {
    uint32_t n = 0;
    bool spec_weq = true, stat_weq = true;
    if (f & F_JSPEC) {
        RegionView A = region_view(pool, r.off_a, r.spec_l_a, r.spec_ar_a, false, r.spec_l_a);
        RegionView B = region_view(pool, r.off_b, r.spec_l_b, r.spec_ar_b, false, r.spec_l_b);
        n += join_region<EMIT>(A, B, 0, out_h, out_k, base + n, lane, &spec_weq);
    }
    if (f & F_JSTAT) {
        RegionView A = region_view(pool, r.off_a, r.spec_l_a, r.spec_ar_a, true, r.stat_l_a);
        RegionView B = region_view(pool, r.off_b, r.spec_l_b, r.spec_ar_b, true, r.stat_l_b);
        n += join_region<EMIT>(A, B, GPUDIFF_PATH_REGION_STATUS, out_h, out_k, base + n, lane, &stat_weq);
    }
    const bool stat_ok = stat_weq && (!(f & F_SENT) || !(r.flags_a & GPUDIFF_OBJ_HAS_STATUS));
    *noop = (((f & F_SPEC) && spec_weq) ? NOOP_SPEC : 0u) | (((f & F_STATUS) && stat_ok) ? NOOP_STATUS : 0u);
    if (f & F_SENT) {
        if (EMIT && lane == 0) {
            out_h[base + n] = status_sentinel_hash((r.flags_a >> GPUDIFF_OBJ_SEED_SHIFT) & 0xFFu, mask);
            out_k[base + n] = GPUDIFF_PATH_REGION_STATUS | GPUDIFF_PATH_STATUS_ABSENT;
        }
        n += 1;
    }
    return n;
}

}  // namespace gd
