// The result image of a fused small pass (GPUDIFF_OPT_SMALL_PASS, kernel K20 in smallpass.hip): where its
// sections lie, how many bytes the first read-back round copies, and the host's unpacker.  The layout functions are
// pure arithmetic for both sides (GPUDIFF_HD, like include/gpudiff_format.h); the unpacker is host code over plain
// memory, no HIP runtime call.
//
//   header (16 u32) | flags[n_pairs] u8 | spec_ids[n_spec] u32 | status_ids[n_status] u32 | dirty_ids[n_dirty] u32
//   | dirty_idx[n_dirty] u32 | path_off[n_dirty + 1] u32 | noop_d[n_dirty] u8 | out_k[n_paths] u8 | out_h[n_paths] u64
//
// Sections are packed by the actual counts, each aligned to its element size.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/gpudiff.h"

namespace gd {

constexpr uint32_t kSmallMagic = 0x30324B47u;  // "GK20"
constexpr uint32_t kSmallHeaderWords = 16;
// header words
constexpr uint32_t SH_MAGIC = 0, SH_FINAL = 1, SH_REASON = 2, SH_PAIRS = 3, SH_SPEC = 4, SH_STATUS = 5, SH_DIRTY = 6,
                   SH_PATHS = 7, SH_BYTES = 8;
// why K20 declined to finish a pass (header word SH_REASON, a bit each)
constexpr uint32_t kSmallArena = 1u;  // a dirty pair's paths did not fit the batch's path arena
constexpr uint32_t kSmallDeep = 2u;   // a join over more keys than one wave takes (kDeepJoin)
constexpr uint32_t kSmallPaths = 4u;  // more than GPUDIFF_SMALL_PASS_MAX_PATHS changed paths

struct SmallLayout {  // byte offsets into the image
    uint64_t flags, spec_ids, status_ids, dirty_ids, dirty_idx, path_off, noop_d, out_k, out_h, total;
};

GPUDIFF_HD inline uint64_t small_align(uint64_t x, uint64_t a) { return (x + a - 1u) / a * a; }

GPUDIFF_HD inline SmallLayout small_layout(uint32_t n_pairs, uint32_t n_spec, uint32_t n_status, uint32_t n_dirty,
                                           uint32_t n_paths) {
    SmallLayout l;
    uint64_t o = 4ull * kSmallHeaderWords;
    l.flags = o;
    o = small_align(o + n_pairs, 4);
    l.spec_ids = o;
    o += 4ull * n_spec;
    l.status_ids = o;
    o += 4ull * n_status;
    l.dirty_ids = o;
    o += 4ull * n_dirty;
    l.dirty_idx = o;
    o += 4ull * n_dirty;
    l.path_off = o;
    o += 4ull * ((uint64_t)n_dirty + 1u);
    l.noop_d = o;
    o += n_dirty;
    l.out_k = o;
    o = small_align(o + n_paths, 8);
    l.out_h = o;
    o += 8ull * n_paths;
    l.total = o;
    return l;
}

// the largest image: what a batch's image buffer and the context's pinned read-back buffer are sized to
GPUDIFF_HD inline uint64_t small_image_capacity() {
    return small_layout(GPUDIFF_SMALL_PASS_MAX_PAIRS, GPUDIFF_SMALL_PASS_MAX_PAIRS, GPUDIFF_SMALL_PASS_MAX_PAIRS,
                        GPUDIFF_SMALL_PASS_MAX_PAIRS, GPUDIFF_SMALL_PASS_MAX_PATHS)
        .total;
}

// paths the first read-back round allows for: 4 per pair (about 8x config3's 0.48 per pair), at least 64
GPUDIFF_HD inline uint32_t small_first_round_paths(uint32_t n_pairs) {
    const uint64_t want = 4ull * n_pairs < 64u ? 64u : 4ull * n_pairs;
    return (uint32_t)(want < GPUDIFF_SMALL_PASS_MAX_PATHS ? want : GPUDIFF_SMALL_PASS_MAX_PATHS);
}

// bytes of the first read-back round: they hold any result of n_pairs pairs with at most
// small_first_round_paths(n_pairs) paths (the layout grows with every count)
GPUDIFF_HD inline uint64_t small_first_round_bytes(uint32_t n_pairs) {
    return small_layout(n_pairs, n_pairs, n_pairs, n_pairs, small_first_round_paths(n_pairs)).total;
}

// ---------------------------------------------------------------- host: unpacking
enum SmallUnpack : int {
    SMALL_OK = 0,        // the result arrays are filled
    SMALL_MORE = 1,      // the prefix is short: *need bytes hold the whole image
    SMALL_DECLINED = 2,  // K20 did not finish the pass (*reason): the image holds a header only
    SMALL_BAD = -1,      // not an image of at most `capacity` bytes
};

// Unpacks the image prefix img[0, len) into rs (.flags .spec .status .dirty .off .hashes .kinds: vectors, as
// engine.h's ResultStore) and the dirty pairs' rows and no-op bits (idx, noop).  Every offset and count is checked
// against len and capacity before it is used; nothing past img + len is read.  The vectors may throw bad_alloc.
template <class RS, class VecU32, class VecU8>
inline SmallUnpack small_unpack(const uint8_t* img, uint64_t len, uint64_t capacity, RS& rs, VecU32& idx, VecU8& noop,
                                uint64_t* need, uint32_t* reason) {
    *need = 4ull * kSmallHeaderWords;
    *reason = 0;
    if (len < 4ull * kSmallHeaderWords) return SMALL_MORE;
    uint32_t h[kSmallHeaderWords];
    memcpy(h, img, sizeof(h));
    if (h[SH_MAGIC] != kSmallMagic || h[SH_FINAL] > 1u) return SMALL_BAD;
    const uint32_t n = h[SH_PAIRS], ns = h[SH_SPEC], nt = h[SH_STATUS], nd = h[SH_DIRTY], np = h[SH_PATHS];
    if (n == 0 || n > GPUDIFF_SMALL_PASS_MAX_PAIRS || ns > n || nt > n || nd > n) return SMALL_BAD;
    if (!h[SH_FINAL]) {
        if (!h[SH_REASON] || (h[SH_REASON] & ~(kSmallArena | kSmallDeep | kSmallPaths))) return SMALL_BAD;
        *reason = h[SH_REASON];
        return SMALL_DECLINED;
    }
    if (np > GPUDIFF_SMALL_PASS_MAX_PATHS) return SMALL_BAD;
    const SmallLayout l = small_layout(n, ns, nt, nd, np);
    if (h[SH_BYTES] < l.total || h[SH_BYTES] > capacity) return SMALL_BAD;
    *need = h[SH_BYTES];
    if (len < h[SH_BYTES]) return SMALL_MORE;
    rs.flags.resize(n);
    rs.spec.resize(ns);
    rs.status.resize(nt);
    rs.dirty.resize(nd);
    rs.off.resize((size_t)nd + 1);
    rs.hashes.resize(np);
    rs.kinds.resize(np);
    idx.resize(nd);
    noop.resize(nd);
    auto take = [&](void* dst, uint64_t off, uint64_t bytes) {
        if (bytes) memcpy(dst, img + off, bytes);
    };
    take(rs.flags.data(), l.flags, n);
    take(rs.spec.data(), l.spec_ids, 4ull * ns);
    take(rs.status.data(), l.status_ids, 4ull * nt);
    take(rs.dirty.data(), l.dirty_ids, 4ull * nd);
    take(idx.data(), l.dirty_idx, 4ull * nd);
    take(rs.off.data(), l.path_off, 4ull * nd + 4u);
    take(noop.data(), l.noop_d, nd);
    take(rs.kinds.data(), l.out_k, np);
    take(rs.hashes.data(), l.out_h, 8ull * np);
    // the lists index each other: a dirty pair's row, its slice of the paths
    if (rs.off[0] != 0u || rs.off[nd] != np) return SMALL_BAD;
    for (uint32_t k = 0; k < nd; k++)
        if (idx[k] >= n || rs.off[k] > rs.off[k + 1]) return SMALL_BAD;
    return SMALL_OK;
}

}  // namespace gd
