// Changed paths of a size-matched dirty region straight from K2's stream: which leaf a
// mismatching 16-B chunk of the compare stream belongs to, and when those leaves alone are the region's
// changed paths, so that the merge-join (and its second read of the pair) is not needed.  Plain inline
// arithmetic over the segment layout, shared by the kernel and the host test: no HIP runtime call.
//
// A segment is  vals[L] u64 | keys[L] u32 | metas[L] u32 | arena  (include/gpudiff_format.h); both sides of a
// size-matched region have the same L and the same arena size, so byte b of the one is byte b of the other.
//
// The rule.  Let S be the leaves hit by a differing dword: a val or meta dword hits its leaf, an arena dword
// the leaf whose tail [off(i), off(i) + meta_arena(m_i)) holds it (off = the prefix sum of meta_arena over side
// A's metas).  The region qualifies when no key dword differs, every differing dword is placed, |S| <=
// kSpMaxLeaves and meta_arena(ma_i) == meta_arena(mb_i) for every leaf of S.  Its changed paths are then exactly
// the keys of S, all CHANGED: with equal L and equal (unique, ascending) keys the merge-join pairs leaf i with
// leaf i and emits it iff its meta, val or tail differs; the leaves outside S have equal metas and those inside
// equal padded tail lengths, so both sides' tails sit at equal offsets and a tail differs iff a differing arena
// dword lies inside it.  Anything else -- a key dword, an arena dword no tail owns (the arena's final padding, the
// stream's line padding), a tail whose padded length changed (every later tail shifts) -- goes to the join.
#pragma once
#include <stdint.h>

#include "../../include/gpudiff_format.h"

#if defined(__HIPCC__)
#define GD_SP_HD __host__ __device__
#else
#define GD_SP_HD
#endif

namespace gd {

constexpr uint32_t kSpLogCap = 4;        // mismatching chunks K2 logs per pair and region; one more: the join
constexpr uint32_t kSpMaxLeaves = 64;    // |S| the emission handles (a lane per leaf)
constexpr uint32_t kSpRefuse = 0xFFFFFFFFu;

// a log entry: the chunk's index within its region and which of its four dwords differ
GD_SP_HD inline uint32_t sp_entry(uint32_t chunk, uint32_t dwords) { return (chunk << 4) | (dwords & 15u); }
GD_SP_HD inline uint32_t sp_entry_dwords(uint32_t e) { return e & 15u; }
GD_SP_HD inline uint64_t sp_entry_byte(uint32_t e, uint32_t d) { return 16ull * (e >> 4) + 4u * d; }

// A pair's key or shape hole (gpudiff_keys_hole, gpudiff_shape_hole: hs, hl in 16-B chunks, both multiples of 8 -- whole
// lines; a descriptor's L is below 2^19, so both halves fit) as the one word K2
// keeps per lane and per pair of the log: hs / 8 | hl / 8 << 16; 0: no hole.  Streamed spec chunk k of the pair is
// chunk k + (k >= hs ? hl : 0) of the segment (gpudiff_hole_chunk): the stream adds sp_hole_bytes to the address, and a
// logged entry goes back through sp_entry_unhole before sp_entry_byte, so the rule above sees segment bytes.  A shape
// hole may end at the arena's first byte (16 L a multiple of 128) or at the streamed span's end (no arena, no status):
// the chunk behind it is then an arena chunk, or there is none.  The rule reads the metas it needs (the owners of arena
// dwords, the padded tail lengths of S) from memory, never from the stream: the metas inside a hole are the equal ones.
static_assert(GPUDIFF_KEYS_HOLE_UNIT % 128u == 0u, "sp_hole_word keeps the hole in 128-B lines");
GD_SP_HD inline uint32_t sp_hole_word(uint32_t hs, uint32_t hl) { return (hs >> 3) | ((hl >> 3) << 16); }
GD_SP_HD inline uint32_t sp_hole_start(uint32_t w) { return (w & 0xFFFFu) << 3; }   // chunks; only read when hl != 0
GD_SP_HD inline uint32_t sp_hole_chunks(uint32_t w) { return (w >> 16) << 3; }
GD_SP_HD inline uint32_t sp_hole_bytes(uint32_t w) { return (w >> 16) << 7; }
// the entry of streamed chunk k as the entry of the segment's chunk
GD_SP_HD inline uint32_t sp_entry_unhole(uint32_t e, uint32_t w) {
    return e + ((e >> 4) >= sp_hole_start(w) ? sp_entry(sp_hole_chunks(w), 0u) : 0u);
}

// A pair streamed from the batch's compare image (gpudiff_format.h: gpudiff_pair_image_parts) has no hole to step over:
// its log slot carries kSpHoleImage instead, which no sp_hole_word equals (hs and hl are below 2^19 chunks together).
// A region whose keys and metas the image drops is written packed (sp_packed_rule, at the end) into a slot that keeps the
// size of the chunk compaction described next -- the slot's accounting (gpudiff_pair_image_parts) and
// tests/test_image_rule.py hold it: the region as  vals[L] zero padded to 16 | arena : nv = ceil(L / 2) chunks of
// values, then the arena's.  Image chunk k is segment chunk k below nv and chunk k + (L - nv) from there on -- the
// chunks of [8 L, 16 L) that hold no value byte are the ones left out.  With L odd, chunk nv - 1 holds the last value
// and 8 bytes of zeros in the image, the last value and keys[0], keys[1] in the segment: its dwords 2 and 3 are zero on
// both image sides, so a logged entry never names them and the rule above never sees a key of an imaged region.  A chunk
// past the image part's end (the line padding) lands at or past the segment's end, where the rule refuses as before.
constexpr uint32_t kSpHoleImage = 0xFFFFFFFFu;
GD_SP_HD inline uint32_t sp_image_vals(uint32_t L) { return (L + 1u) >> 1; }
GD_SP_HD inline uint32_t sp_image_chunk(uint32_t k, uint32_t L) { return k + (k >= sp_image_vals(L) ? L - sp_image_vals(L) : 0u); }
// the compaction itself: the image chunk that holds segment chunk c of such a region, kSpRefuse for a chunk left out
GD_SP_HD inline uint32_t sp_image_of_chunk(uint32_t c, uint32_t L) {
    return c < sp_image_vals(L) ? c : c >= L ? c - (L - sp_image_vals(L)) : kSpRefuse;
}
// the entry of image chunk k as the entry of the segment's chunk
GD_SP_HD inline uint32_t sp_entry_unimage(uint32_t e, uint32_t L) {
    return e + ((e >> 4) >= sp_image_vals(L) ? sp_entry(L - sp_image_vals(L), 0u) : 0u);
}

// arena bytes of a leaf's value: a long string's tail past its first 8 bytes, zero padded to 4; must equal
// gpudiff_meta_arena (include/gpudiff_format.h), restated here because K2 compiles it
GD_SP_HD inline uint32_t sp_meta_arena(uint32_t m) {
    return ((m & 7u) == GPUDIFF_TAG_STR && (m >> 3) > GPUDIFF_INLINE_MAX) ? (((m >> 3) - GPUDIFF_INLINE_MAX + 3u) & ~3u)
                                                                          : 0u;
}

// packed bytes of a leaf's value in an image region (a string's length padded to 4, a number's 8 bytes, nothing for a
// tag-only leaf); must equal gpudiff_meta_packed (include/gpudiff_format.h), restated like sp_meta_arena because K2
// compiles it (tests/test_packed_rule.py ties the two together over every tag and length)
GD_SP_HD inline uint32_t sp_pk(uint32_t m) {
    const uint32_t tag = m & 7u;
    return tag == GPUDIFF_TAG_STR ? (((m >> 3) + 3u) & ~3u) : (tag == GPUDIFF_TAG_INT || tag == GPUDIFF_TAG_FLOAT) ? 8u : 0u;
}

enum SpClass : uint32_t { SP_VAL = 0, SP_KEY = 1, SP_META = 2, SP_ARENA = 3 };
struct SpWhere {
    uint32_t cls;
    uint32_t idx;  // SP_VAL / SP_KEY / SP_META: the leaf; SP_ARENA: the byte's offset in the arena
};
// where the dword at byte b (a multiple of 4) of a region of L leaves lies.  L may be odd, so the boundaries
// fall inside 16-B chunks: per dword, never per chunk
GD_SP_HD inline SpWhere sp_classify(uint64_t b, uint32_t L) {
    const uint64_t l = L;
    if (b < 8u * l) return SpWhere{SP_VAL, (uint32_t)(b >> 3)};
    if (b < 12u * l) return SpWhere{SP_KEY, (uint32_t)((b - 8u * l) >> 2)};
    if (b < 16u * l) return SpWhere{SP_META, (uint32_t)((b - 12u * l) >> 2)};
    return SpWhere{SP_ARENA, (uint32_t)(b - 16u * l)};
}

// the leaf whose tail holds arena byte ao; L when none does
GD_SP_HD inline uint32_t sp_arena_owner(const uint32_t* metas, uint32_t L, uint32_t ao) {
    uint32_t off = 0;
    for (uint32_t i = 0; i < L; i++) {
        const uint32_t n = sp_meta_arena(metas[i]);
        if (ao - off < n) return i;  // off <= ao here
        off += n;
    }
    return L;
}

// The whole rule, one region, serially (the kernel does the same a lane per differing dword): entries[n] are
// the region's mismatching chunks, seg_a / seg_b its two sides of seg_bytes each.  Returns |S| with the leaves
// ascending in leaves[], or kSpRefuse.
GD_SP_HD inline uint32_t sp_region_rule(const uint8_t* seg_a, const uint8_t* seg_b, uint32_t L, uint64_t seg_bytes,
                                        const uint32_t* entries, uint32_t n, uint32_t leaves[kSpMaxLeaves]) {
    const uint32_t* ma = (const uint32_t*)(seg_a + 12ull * L);
    const uint32_t* mb = (const uint32_t*)(seg_b + 12ull * L);
    uint32_t ns = 0;
    for (uint32_t q = 0; q < n; q++)
        for (uint32_t d = 0; d < 4; d++) {
            if (!((sp_entry_dwords(entries[q]) >> d) & 1u)) continue;
            const uint64_t b = sp_entry_byte(entries[q], d);
            if (b >= seg_bytes) return kSpRefuse;
            const SpWhere w = sp_classify(b, L);
            if (w.cls == SP_KEY) return kSpRefuse;
            const uint32_t leaf = w.cls == SP_ARENA ? sp_arena_owner(ma, L, w.idx) : w.idx;
            if (leaf >= L) return kSpRefuse;
            uint32_t at = 0;  // sorted insert, once
            while (at < ns && leaves[at] < leaf) at++;
            if (at < ns && leaves[at] == leaf) continue;
            if (ns == kSpMaxLeaves) return kSpRefuse;
            for (uint32_t k = ns; k > at; k--) leaves[k] = leaves[k - 1];
            leaves[at] = leaf;
            ns++;
        }
    for (uint32_t k = 0; k < ns; k++)
        if (sp_meta_arena(ma[leaves[k]]) != sp_meta_arena(mb[leaves[k]])) return kSpRefuse;
    return ns;
}

// ---- A packed region of the compare image (gpudiff_format.h: gpudiff_meta_packed) is not mapped back to its segment:
// it holds value bytes alone, leaf i at [P_i, P_{i+1}) with P the exclusive prefix of sp_pk over side A's metas (the
// pool's: the image has none), so the differing dword at packed byte p is leaf i's, and a byte at or past P_L is the
// region's final padding.  No key dword, no meta dword and no shifted tail can occur: both sides were packed by A's
// metas.  The region's changed paths are the keys of the set S of owners when the log did not overflow and |S| <=
// kSpMaxLeaves; the padded tail lengths of S are compared as above (they are equal unless a meta was changed behind the
// encoder's back, which the join then sees as before).
// the leaf that owns packed byte p; L when none does
GD_SP_HD inline uint32_t sp_packed_owner(const uint32_t* metas, uint32_t L, uint32_t p) {
    uint32_t off = 0;
    for (uint32_t i = 0; i < L; i++) {
        const uint32_t n = sp_pk(metas[i]);
        if (p - off < n) return i;  // off <= p here
        off += n;
    }
    return L;
}
// The rule, one packed region, serially: entries[n] its mismatching chunks (chunk indices in the packed region), ma / mb
// the two sides' metas[L] in the pool.  Returns |S| with the leaves ascending in leaves[], or kSpRefuse.
GD_SP_HD inline uint32_t sp_packed_rule(const uint32_t* ma, const uint32_t* mb, uint32_t L, const uint32_t* entries,
                                        uint32_t n, uint32_t leaves[kSpMaxLeaves]) {
    uint32_t ns = 0;
    for (uint32_t q = 0; q < n; q++)
        for (uint32_t d = 0; d < 4; d++) {
            if (!((sp_entry_dwords(entries[q]) >> d) & 1u)) continue;
            const uint32_t leaf = sp_packed_owner(ma, L, (uint32_t)sp_entry_byte(entries[q], d));
            if (leaf >= L) return kSpRefuse;
            uint32_t at = 0;
            while (at < ns && leaves[at] < leaf) at++;
            if (at < ns && leaves[at] == leaf) continue;
            if (ns == kSpMaxLeaves) return kSpRefuse;
            for (uint32_t k = ns; k > at; k--) leaves[k] = leaves[k - 1];
            leaves[at] = leaf;
            ns++;
        }
    for (uint32_t k = 0; k < ns; k++)
        if (sp_meta_arena(ma[leaves[k]]) != sp_meta_arena(mb[leaves[k]])) return kSpRefuse;
    return ns;
}

}  // namespace gd
