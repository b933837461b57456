/*
 * gpudiff_format.h -- canonical encoding shared by the host encoder and the
 * HIP kernels (DESIGN.md "Canonical encoding").  Plain C layout, no HIP types.
 *
 * One object = one blob in a pool, its start and its segments' end aligned to
 * GPUDIFF_BLOB_ALIGN (128 B, the HBM line) with zeros:
 *
 *   [ spec segment ][ status segment ][ zero pad to 128 ]
 *
 * The decision kernel streams whole lines: a stream that starts or ends inside
 * a line costs a partial-line request per blob edge (measured on MI355X: 16-B
 * aligned blobs of ~3.2 KB read at 6.1 TB/s, line-aligned ones at 6.8 TB/s).
 *
 *   segment(L, arena) = vals[L] u64 | keys[L] u32 | metas[L] u32
 *                       | arena: the tails of the long string values in key
 *                         order, each at a 4-byte aligned offset (zero padded
 *                         to 4), the whole zero padded to a multiple of 16
 *
 *   keys   = pathHash: the chained XXH64 path hash under the pair seed, cut
 *            to GPUDIFF_PATH_HASH_BITS (32) bits, ascending, unique
 *   vals   = the value's first 8 bytes: the whole value when it fits (inline:
 *            <= 8 bytes, zero padded), else the head of a long string, whose
 *            remaining len - 8 bytes (its tail) sit in the arena
 *   metas  = (len << 3) | tag
 *
 * Every byte of a value is stored exactly once: the leaf record carries the
 * first 8, the arena the rest.  (Until ABI 4 a long string's vals slot held an
 * XXH64 digest and the arena the whole value: the decision kernel compares
 * arena bytes anyway, so the digest was 8 redundant bytes per long value in
 * every pass -- 9.6% of config3's compared bytes.)
 *
 * Two objects' compared regions are equal under the reference predicates
 * (pkg/syncer/specsyncer.go:17-41, statussyncer.go:15-27) iff their segments
 * are byte-identical, because the encoding is a deterministic function of the
 * leaf set and the path hash is verified injective over each pair's path
 * union: by the encoder over both path sets (it re-seeds the pair on a
 * collision), or, in the object store, against the resident version's path
 * table (below).
 */
#ifndef GPUDIFF_FORMAT_H
#define GPUDIFF_FORMAT_H

#include <stdint.h>

/* The functions below are the format's arithmetic, written down once: the
 * host, the oracle and the HIP kernels call them.  In a HIP translation unit
 * they compile for both sides; in C and plain C++ the qualifier is empty. */
#ifdef __HIPCC__
#define GPUDIFF_HD __host__ __device__
#else
#define GPUDIFF_HD
#endif

#define GPUDIFF_TAG_NULL 0u
#define GPUDIFF_TAG_FALSE 1u
#define GPUDIFF_TAG_TRUE 2u
#define GPUDIFF_TAG_INT 3u
#define GPUDIFF_TAG_FLOAT 4u
#define GPUDIFF_TAG_STR 5u
#define GPUDIFF_TAG_EOBJ 6u
#define GPUDIFF_TAG_EARR 7u

#define GPUDIFF_INLINE_MAX 8u
/* width of the path hashes kept in segments and reported in changed-path
 * lists: 32 bits (16 B per leaf record).  Exactness never rests on the width:
 * the hash is verified injective over each pair's path union (re-seeded on a
 * collision) and the object store's path tables agree at any width. */
#define GPUDIFF_PATH_HASH_BITS 32u

/* object flags (PairRow.flags_a / flags_b) */
#define GPUDIFF_OBJ_HAS_STATUS 0x1u   /* top-level "status" key present (even null) */
#define GPUDIFF_OBJ_DECODE_ERR 0x2u   /* JSON failed the Go decode rules */
#define GPUDIFF_OBJ_FRESH 0x4u        /* object store: blob uploaded with this batch (informational) */
/* flags_b only: spec_l_a == spec_l_b and A's and B's spec keys[] are element for element equal -- with the
 * injectivity the encoder has just verified, the same paths.  A structural fact like the sizes, stated by the
 * producer that sorted both key lists (PairEncoder::encode_flat), never on a decode-error row; K2 trusts it
 * exactly as it trusts the sizes and leaves the whole lines that hold only spec keys out of its stream
 * (gpudiff_keys_hole).  Additive: a producer that leaves it 0 (the object stores, an older encoder) gets the keys
 * streamed as before. */
#define GPUDIFF_OBJ_SPEC_KEYS_EQ 0x8u
/* flags_b only, and only beside GPUDIFF_OBJ_SPEC_KEYS_EQ: A's and B's spec metas[] (each leaf's type tag and byte
 * length) are element for element equal as well, so the two spec regions have the same shape -- the same paths, types
 * and lengths -- and spec_ar_a == spec_ar_b follows.  Stated by the same loop of PairEncoder::encode_flat, never on a
 * decode-error row.  K2 then also leaves out the whole lines that hold only spec metas (gpudiff_shape_hole): of such a
 * pair it compares every value and tail byte on every pass, and trusts the keys and metas inside whole lines as it
 * trusts the sizes.  Additive like the bit above: the object stores, K0 and an older encoder leave it 0. */
#define GPUDIFF_OBJ_SPEC_SHAPE_EQ 0x10u
/* flags_b only: the same fact about the status region -- stat_l_a == stat_l_b > 0, both sides have a status key, and
 * the two status keys[] and the two status metas[] are element for element equal (so stat_ar_a == stat_ar_b).  Stated
 * by PairEncoder::encode_flat, which holds both sides' status leaves sorted by hash, never on a decode-error row.  It
 * is read only where a batch's compare image is built (gpudiff_pair_image_parts): the image of such a pair keeps the
 * status vals[] and arena alone.  Additive: every other producer of rows leaves it 0. */
#define GPUDIFF_OBJ_STAT_SHAPE_EQ 0x20u
/* object store: the path table kept after a resident blob's segments (the
 * "trailer"), which makes the store's old-vs-new path check exact.  Its n
 * entries are the region leaves and all their ancestors except the root,
 * ascending by (masked) path hash:
 *
 *   hs[n] u64 | phs[n] u64 | cs[n] u64 | key bytes | pad (the whole a multiple of 128),
 *   at the blob's body end (gpudiff_blob_body)
 *
 *   hs    = the node's path hash; unique, and none equals the root's (the seed)
 *   phs   = its parent's path hash (depth-1 nodes: the seed)
 *   cs    = its last component: GPUDIFF_TAB_INDEX | index, or
 *           (key length << 32) | offset of the key bytes in the key area
 *
 * Two tables agree when every hash both hold has the same parent hash and the
 * same component in each.  By induction on depth (the root is the same in
 * both; a node's parent hash names exactly one node of each table), agreeing
 * tables give every shared hash the same path in both objects: an equal key in
 * two segments is then an equal path, whatever the hash width. */
#define GPUDIFF_TAB_INDEX 0x8000000000000000ull
/* entry count of a blob stored without a valid table (its node hashes are not
 * unique under the pair's seed): nothing agrees with it, so the next event on
 * its slot is re-encoded from old_json */
#define GPUDIFF_TAB_NONE 0xFFFFFFFFu
GPUDIFF_HD static inline uint64_t gpudiff_tab_bytes(uint32_t n, uint64_t key_bytes) {
    return (24ull * n + key_bytes + 127u) & ~(uint64_t)127u;  /* blobs stay GPUDIFF_BLOB_ALIGN multiples */
}

/* bits 8..15 of flags_a: per-pair path-hash seed */
#define GPUDIFF_OBJ_SEED_SHIFT 8u

#ifdef __cplusplus
extern "C" {
#endif

/* One pair descriptor, 64 bytes, device resident.  Offsets are byte offsets
 * into the pool the row lives with. */
typedef struct gpudiff_pair_row {
    uint64_t off_a;          /* blob of A (old / upstream) */
    uint64_t off_b;          /* blob of B (new / downstream) */
    uint32_t spec_l_a, spec_l_b;       /* spec-region leaves */
    uint32_t spec_ar_a, spec_ar_b;     /* spec arena bytes (multiple of 16) */
    uint32_t stat_l_a, stat_l_b;       /* status-region leaves */
    uint32_t stat_ar_a, stat_ar_b;     /* status arena bytes (multiple of 16) */
    uint32_t flags_a, flags_b;
    uint32_t pair_id, cluster_id;
} gpudiff_pair_row;

/* segment bytes: 16 B per leaf record (a multiple of 16) + the arena */
GPUDIFF_HD static inline uint64_t gpudiff_seg_bytes(uint32_t l, uint32_t arena) {
    return (uint64_t)l * 16u + (uint64_t)arena;
}

#define GPUDIFF_BLOB_ALIGN 128u
/* a blob's body: both segments, zero padded to GPUDIFF_BLOB_ALIGN -- the span the
 * decision kernel reads; a device-store blob's path table starts here */
GPUDIFF_HD static inline uint64_t gpudiff_blob_body(uint32_t sl, uint32_t sar, uint32_t tl, uint32_t tar) {
    return (gpudiff_seg_bytes(sl, sar) + gpudiff_seg_bytes(tl, tar) + (GPUDIFF_BLOB_ALIGN - 1u)) &
           ~(uint64_t)(GPUDIFF_BLOB_ALIGN - 1u);
}

/* ---- key holes: the part of a segment's keys[L] that K2 may skip when the row says the two sides' keys are equal
 * (GPUDIFF_OBJ_SPEC_KEYS_EQ).  keys[] occupies bytes [8 L, 12 L) of the segment; the hole is the whole
 * GPUDIFF_KEYS_HOLE_UNIT-byte units inside it, so with the segment at the blob's (line-aligned) start it is whole
 * lines of memory.  The partial units at both ends -- the last values, the first metas and a few keys -- are still
 * streamed.  *hs: the hole's first 16-B chunk, *hl: its chunks (0: no hole).  L = 32 is the first with a hole
 * (one line), L = 33..42 have none, L = 184 skips 640 B a side. */
#ifndef GPUDIFF_KEYS_HOLE_UNIT
#define GPUDIFF_KEYS_HOLE_UNIT 128u
#endif
GPUDIFF_HD static inline void gpudiff_keys_hole(uint32_t l, uint32_t* hs, uint32_t* hl) {
    const uint64_t u = GPUDIFF_KEYS_HOLE_UNIT;
    const uint64_t lo = (8ull * l + (u - 1u)) / u * u, hi = 12ull * l / u * u;
    *hs = hi > lo ? (uint32_t)(lo >> 4) : 0u;
    *hl = hi > lo ? (uint32_t)((hi - lo) >> 4) : 0u;
}
/* ---- shape holes: keys[] and metas[] together occupy bytes [8 L, 16 L); a row that carries GPUDIFF_OBJ_SPEC_SHAPE_EQ
 * beside GPUDIFF_OBJ_SPEC_KEYS_EQ lets K2 skip the whole units inside that span.  Twice the key span with the same two
 * partial units at its ends: L = 16 is the first with a hole (one line), L = 17..23 have none, L = 24..31 one line,
 * L = 28 skips 128 B a side, L = 184 1408 B.  The hole ends at the arena's first byte when 16 L is a multiple of the
 * unit.  Contains gpudiff_keys_hole(L) whenever that is not empty. */
GPUDIFF_HD static inline void gpudiff_shape_hole(uint32_t l, uint32_t* hs, uint32_t* hl) {
    const uint64_t u = GPUDIFF_KEYS_HOLE_UNIT;
    const uint64_t lo = (8ull * l + (u - 1u)) / u * u, hi = 16ull * l / u * u;
    *hs = hi > lo ? (uint32_t)(lo >> 4) : 0u;
    *hl = hi > lo ? (uint32_t)((hi - lo) >> 4) : 0u;
}
/* streamed spec chunk k of a pair with the hole (hs, hl) is chunk k + (k >= hs ? hl : 0) of the segment */
GPUDIFF_HD static inline uint32_t gpudiff_hole_chunk(uint32_t k, uint32_t hs, uint32_t hl) {
    return k + (k >= hs ? hl : 0u);
}

/* B_pair: the bytes the decision kernel (K2) reads for one pair -- the 64-B row, the flag byte and, per
 * object, the compared 16-B chunks: the whole body (segments + zero pad) when both regions' sizes match
 * and B has status; the spec segment when only the spec sizes match (padded to the line too when neither
 * side has status leaves); the status segment when only the status sizes match; nothing else (a size
 * mismatch decides the region without reading it).  The roofline's format bytes and the shard weight. */
GPUDIFF_HD static inline uint64_t gpudiff_pair_compare_bytes(const gpudiff_pair_row* r) {
    const uint64_t al = GPUDIFF_BLOB_ALIGN - 1u;
    uint64_t per = 0;
    if ((r->flags_a | r->flags_b) & GPUDIFF_OBJ_DECODE_ERR) return sizeof(gpudiff_pair_row) + 1u;
    {
        const int spec_sz = r->spec_l_a == r->spec_l_b && r->spec_ar_a == r->spec_ar_b;
        const int stat_sz = (r->flags_b & GPUDIFF_OBJ_HAS_STATUS) && r->stat_l_a == r->stat_l_b &&
                            r->stat_ar_a == r->stat_ar_b;
        const uint64_t seg_s = gpudiff_seg_bytes(r->spec_l_a, r->spec_ar_a);
        const uint64_t seg_t = gpudiff_seg_bytes(r->stat_l_a, r->stat_ar_a);
        if (spec_sz && stat_sz) per = (seg_s + seg_t + al) & ~al;
        else if (spec_sz) per = (r->stat_l_a | r->stat_l_b | r->stat_ar_a | r->stat_ar_b) ? seg_s : (seg_s + al) & ~al;
        else if (stat_sz) per = seg_t;
    }
    return sizeof(gpudiff_pair_row) + 1u + 2u * per;
}

/* ---- the pair descriptor: 16 bytes that stand for a row in the decision kernel's stream (DESIGN.md §5
 * "Pair descriptors").  Written beside the rows when a batch is appended; K2 reads it instead of the 64-B row and
 * goes back to the row only for what the descriptor leaves out (the leaf counts, the seed's value, the IDs).
 *
 *   word 0, 1   off_a >> 7, off_b >> 7                  (blobs are GPUDIFF_BLOB_ALIGN aligned)
 *   bits  0-18  spec segment bytes of A, in 16-B units  (word 2 | word 3 << 32)
 *   bits 19-37  spec segment bytes of B, in 16-B units; under SPEC_EQ (B's equal A's) the skip L instead: the spec
 *               leaf count when the row carries GPUDIFF_OBJ_SPEC_KEYS_EQ, no error and a non-empty key hole, else 0.
 *               A skip L never exceeds A's field (16 L <= the segment), so with A's field below GPUDIFF_PD_SHAPE_L
 *               (a spec segment under 4 MiB) a value of GPUDIFF_PD_SHAPE_L or more is free: L | GPUDIFF_PD_SHAPE_L
 *               says that the row carries GPUDIFF_OBJ_SPEC_SHAPE_EQ too and its shape hole is not empty.  A shape
 *               row of 4 MiB or more keeps the key hole's code (no real object is that large).
 *   bits 38-56  status segment bytes of A, in 16-B units
 *   bits 57-63  GPUDIFF_PD_* >> 0
 *
 * Two of the bits cannot be derived from the sizes: SPEC_EQ and STAT_EQ mean that the leaf counts and the arenas
 * are both equal, which equal segment bytes do not imply (16 L + arena coincides for other L).
 *
 * A row whose offsets or sizes do not fit, or are not multiples of the units, or whose status leaf counts
 * contradict its NO_STAT bit (never an encoder's row), is packed as the escape: all ones.  No packed row equals it
 * -- it would carry NO_STAT with a non-zero status segment -- and word 3 alone tells. */
#define GPUDIFF_PD_ERR 0x01u       /* either side failed to decode */
#define GPUDIFF_PD_SPEC_EQ 0x02u   /* spec_l and spec_ar equal on both sides */
#define GPUDIFF_PD_STAT_EQ 0x04u   /* stat_l and stat_ar equal on both sides */
#define GPUDIFF_PD_HAS_ST_B 0x08u  /* flags_b & GPUDIFF_OBJ_HAS_STATUS */
#define GPUDIFF_PD_HAS_ST_A 0x10u  /* flags_a & GPUDIFF_OBJ_HAS_STATUS */
#define GPUDIFF_PD_SEED 0x20u      /* the pair's path-hash seed != 0 */
#define GPUDIFF_PD_NO_STAT 0x40u   /* stat_l and stat_ar zero on both sides */
#define GPUDIFF_PD_SIZE_BITS 19u
#define GPUDIFF_PD_SIZE_MAX 0x7FFFFu  /* 16-B units: segments below 8 MiB */
#define GPUDIFF_PD_ESCAPE 0xFFFFFFFFu
#define GPUDIFF_PD_SHAPE_L 0x40000u   /* in the skip L field: the hole is the shape hole, L the low 18 bits */
/* The image form (gpudiff_pair_desc_pack_image): the descriptor of a fictitious row whose two blobs are the pair's
 * sides in the batch's compare image -- words 0, 1 in 128-B units from the image's base, A's field the image's spec
 * part, the status field its status part, the seven bits the real row's.  Its mark is the skip L field all ones under
 * SPEC_EQ with A's field below GPUDIFF_PD_IMAGE_SPEC_MAX.  gpudiff_pair_desc_pack writes all ones there in two corners
 * only -- a key hole's L = 0x7FFFF (then A's field is 0x7FFFF too: 16 L <= the segment) and a shape hole's
 * L | GPUDIFF_PD_SHAPE_L with L = 0x3FFFF (then A's field is 0x3FFFF) -- so the bound on A's field keeps the two
 * forms apart; a pair whose image spec part is that large is not imaged.  gpudiff_pair_desc_unpack reports the mark as
 * GPUDIFF_PD_IMAGE in gpudiff_pair_geom::bits (no descriptor bit: the seven above fill the field). */
#define GPUDIFF_PD_IMAGE 0x80u
#define GPUDIFF_PD_IMAGE_SPEC_MAX 0x3FFFFu

typedef struct gpudiff_pair_desc {
    uint32_t w[4];
} gpudiff_pair_desc;

/* what K2's stream needs of a pair: n1 streamed spec chunks -- chunk k at off + 16 gpudiff_hole_chunk(k, hs, hl) --
 * n2 status chunks from off + 16 n1 + adj (per side), and the GPUDIFF_PD_* bits its decisions read */
typedef struct gpudiff_pair_geom {
    uint64_t off_a, off_b;
    uint32_t n1, n2, adj_a, adj_b;
    uint32_t bits;
    uint32_t hs, hl; /* the key or shape hole left out of the n1 spec chunks (16-B chunks; hl 0: none) */
} gpudiff_pair_geom;

/* the stream's chunk counts from the segment bytes and the bits: K2's rule (gpudiff_pair_compare_bytes counts the
 * same chunks, the hole included).  skip_l: the spec leaf count of a pair whose spec keys need no compare, else 0;
 * shape: its metas need none either (the hole is gpudiff_shape_hole).  A count whose keys (and metas) would not lie
 * inside the streamed spec span (never a packer's) is taken as 0 */
GPUDIFF_HD static inline gpudiff_pair_geom gpudiff_pair_geom_of(uint64_t off_a, uint64_t off_b, uint32_t seg_a,
                                                                uint32_t seg_b, uint32_t seg_t, uint32_t bits,
                                                                uint32_t skip_l, int shape) {
    gpudiff_pair_geom g;
    const int ok = !(bits & GPUDIFF_PD_ERR);
    const int spec_sz = (bits & GPUDIFF_PD_SPEC_EQ) != 0u;
    const int stat_sz = (bits & GPUDIFF_PD_HAS_ST_B) && (bits & GPUDIFF_PD_STAT_EQ);
    const uint32_t r128 = (seg_a + seg_t + 127u) & ~127u;
    g.off_a = off_a;
    g.off_b = off_b;
    g.n1 = (ok && spec_sz) ? ((!stat_sz && (bits & GPUDIFF_PD_NO_STAT)) ? ((seg_a + 127u) & ~127u) : seg_a) >> 4 : 0u;
    g.n2 = (ok && stat_sz) ? (spec_sz ? r128 - seg_a : seg_t) >> 4 : 0u;
    g.hs = g.hl = 0u;
    if (skip_l && (uint64_t)skip_l * (shape ? 16u : 12u) <= 16ull * g.n1) {
        if (shape) gpudiff_shape_hole(skip_l, &g.hs, &g.hl);
        else gpudiff_keys_hole(skip_l, &g.hs, &g.hl);
        g.n1 -= g.hl;
    }
    g.adj_a = seg_a - 16u * g.n1;
    g.adj_b = seg_b - 16u * g.n1;
    g.bits = bits;
    return g;
}

GPUDIFF_HD static inline uint32_t gpudiff_pair_row_bits(const gpudiff_pair_row* r) {
    return (((r->flags_a | r->flags_b) & GPUDIFF_OBJ_DECODE_ERR) ? GPUDIFF_PD_ERR : 0u) |
           ((r->spec_l_a == r->spec_l_b && r->spec_ar_a == r->spec_ar_b) ? GPUDIFF_PD_SPEC_EQ : 0u) |
           ((r->stat_l_a == r->stat_l_b && r->stat_ar_a == r->stat_ar_b) ? GPUDIFF_PD_STAT_EQ : 0u) |
           ((r->flags_b & GPUDIFF_OBJ_HAS_STATUS) ? GPUDIFF_PD_HAS_ST_B : 0u) |
           ((r->flags_a & GPUDIFF_OBJ_HAS_STATUS) ? GPUDIFF_PD_HAS_ST_A : 0u) |
           (((r->flags_a >> GPUDIFF_OBJ_SEED_SHIFT) & 0xFFu) ? GPUDIFF_PD_SEED : 0u) |
           ((r->stat_l_a | r->stat_l_b | r->stat_ar_a | r->stat_ar_b) == 0u ? GPUDIFF_PD_NO_STAT : 0u);
}

/* the same from the row itself (an escape's lane in K2, the row-path kernels): never a hole */
GPUDIFF_HD static inline gpudiff_pair_geom gpudiff_pair_row_geom(const gpudiff_pair_row* r) {
    return gpudiff_pair_geom_of(r->off_a, r->off_b, (uint32_t)gpudiff_seg_bytes(r->spec_l_a, r->spec_ar_a),
                                (uint32_t)gpudiff_seg_bytes(r->spec_l_b, r->spec_ar_b),
                                (uint32_t)gpudiff_seg_bytes(r->stat_l_a, r->stat_ar_a), gpudiff_pair_row_bits(r), 0u, 0);
}

GPUDIFF_HD static inline gpudiff_pair_desc gpudiff_pair_desc_pack(const gpudiff_pair_row* r) {
    gpudiff_pair_desc d;
    const uint64_t sa = gpudiff_seg_bytes(r->spec_l_a, r->spec_ar_a), sb = gpudiff_seg_bytes(r->spec_l_b, r->spec_ar_b);
    const uint64_t st = gpudiff_seg_bytes(r->stat_l_a, r->stat_ar_a);
    const uint32_t bits = gpudiff_pair_row_bits(r);
    const uint64_t size_max = (uint64_t)GPUDIFF_PD_SIZE_MAX << 4;
    const int fits = ((r->off_a | r->off_b) & (GPUDIFF_BLOB_ALIGN - 1u)) == 0u && (r->off_a >> 7) <= 0xFFFFFFFFull &&
                     (r->off_b >> 7) <= 0xFFFFFFFFull && ((sa | sb | st) & 15u) == 0u && sa <= size_max &&
                     sb <= size_max && st <= size_max &&
                     /* K2 joins the status region when stat_l_a + stat_l_b != 0 (u32): the NO_STAT bit must say so */
                     ((uint32_t)(r->stat_l_a + r->stat_l_b) == 0u) == ((bits & GPUDIFF_PD_NO_STAT) != 0u);
    if (!fits) {
        d.w[0] = d.w[1] = d.w[2] = d.w[3] = GPUDIFF_PD_ESCAPE;
        return d;
    }
    {
        /* under SPEC_EQ sb == sa: the field carries the skip L (16 L <= sa, so it fits) */
        uint64_t f1 = sb >> 4;
        if (bits & GPUDIFF_PD_SPEC_EQ) {
            uint32_t hs = 0, hl = 0;
            const int keys = (r->flags_b & GPUDIFF_OBJ_SPEC_KEYS_EQ) && !(bits & GPUDIFF_PD_ERR);
            f1 = 0u;
            if (keys && (r->flags_b & GPUDIFF_OBJ_SPEC_SHAPE_EQ) && (sa >> 4) < GPUDIFF_PD_SHAPE_L) {
                gpudiff_shape_hole(r->spec_l_a, &hs, &hl);
                if (hl) f1 = r->spec_l_a | GPUDIFF_PD_SHAPE_L;
            }
            if (keys && !f1) { /* (an empty shape hole: the key hole inside it is empty too) */
                gpudiff_keys_hole(r->spec_l_a, &hs, &hl);
                f1 = hl ? r->spec_l_a : 0u;
            }
        }
        const uint64_t zw = (sa >> 4) | (f1 << GPUDIFF_PD_SIZE_BITS) | ((st >> 4) << (2u * GPUDIFF_PD_SIZE_BITS)) |
                            ((uint64_t)bits << (3u * GPUDIFF_PD_SIZE_BITS));
        d.w[0] = (uint32_t)(r->off_a >> 7);
        d.w[1] = (uint32_t)(r->off_b >> 7);
        d.w[2] = (uint32_t)zw;
        d.w[3] = (uint32_t)(zw >> 32);
    }
    return d;
}

GPUDIFF_HD static inline int gpudiff_pair_desc_is_escape(uint32_t w3) { return w3 == GPUDIFF_PD_ESCAPE; }

/* of a descriptor that is not the escape */
GPUDIFF_HD static inline gpudiff_pair_geom gpudiff_pair_desc_unpack(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
    const uint64_t zw = ((uint64_t)w3 << 32) | w2;
    const uint32_t bits = w3 >> (3u * GPUDIFF_PD_SIZE_BITS - 32u);
    const uint32_t seg_a = (w2 & GPUDIFF_PD_SIZE_MAX) << 4;
    const uint32_t f1 = (uint32_t)(zw >> GPUDIFF_PD_SIZE_BITS) & GPUDIFF_PD_SIZE_MAX;
    const int eq = (bits & GPUDIFF_PD_SPEC_EQ) != 0u;
    /* L <= A's field: below GPUDIFF_PD_SHAPE_L there, a skip field at or above it is L | GPUDIFF_PD_SHAPE_L */
    const int shape = eq && f1 >= GPUDIFF_PD_SHAPE_L && (w2 & GPUDIFF_PD_SIZE_MAX) < GPUDIFF_PD_SHAPE_L;
    /* the image form: offsets from the image's base, no hole (the image holds no key and no meta to step over) */
    const int image = eq && f1 == GPUDIFF_PD_SIZE_MAX && (w2 & GPUDIFF_PD_SIZE_MAX) < GPUDIFF_PD_IMAGE_SPEC_MAX;
    gpudiff_pair_geom g =
        gpudiff_pair_geom_of((uint64_t)w0 << 7, (uint64_t)w1 << 7, seg_a, eq ? seg_a : f1 << 4,
                             ((w3 >> (2u * GPUDIFF_PD_SIZE_BITS - 32u)) & GPUDIFF_PD_SIZE_MAX) << 4, bits,
                             (eq && !image) ? (shape ? f1 & (GPUDIFF_PD_SHAPE_L - 1u) : f1) : 0u, shape && !image);
    if (image) g.bits |= GPUDIFF_PD_IMAGE;
    return g;
}

/* the bytes the descriptor kernel reads for one pair: its 16-B descriptor and both sides' streamed chunks, key and
 * shape holes left out (an escape's pair streams from its row: no hole).  gpudiff_pair_compare_bytes stays the
 * format's bytes. */
GPUDIFF_HD static inline uint64_t gpudiff_pair_stream_bytes(const gpudiff_pair_row* r) {
    const gpudiff_pair_desc d = gpudiff_pair_desc_pack(r);
    const gpudiff_pair_geom g = gpudiff_pair_desc_is_escape(d.w[3]) ? gpudiff_pair_row_geom(r)
                                                                   : gpudiff_pair_desc_unpack(d.w[0], d.w[1], d.w[2], d.w[3]);
    return sizeof(gpudiff_pair_desc) + 32ull * ((uint64_t)g.n1 + g.n2);
}

/* ---- the compare image (DESIGN.md §5 "Compare image"): for a row with no decode error, equal spec sizes and both
 * GPUDIFF_OBJ_SPEC_KEYS_EQ and GPUDIFF_OBJ_SPEC_SHAPE_EQ, gpudiff_dbatch_append also writes a compacted copy of what K2
 * must compare into a second allocation.  Per side a 128-B aligned slot, A's then B's, sized for
 *
 *   spec vals[L] (zero padded to 16) | spec arena
 *   | the status region, when its sizes are equal and B has a status key: vals[Lt] (zero padded to 16) | status arena
 *     under GPUDIFF_OBJ_STAT_SHAPE_EQ, the whole status segment otherwise
 *   | zeros to 128
 *
 * A part whose keys and metas are dropped is written packed to its values' true lengths (gpudiff_meta_packed, below) at
 * the slot's front, the next part and the zeros to the line right behind it: the slot keeps the size above, the bytes
 * behind a packed side are neither written nor streamed, and the pair's descriptor carries the packed parts' sizes.
 *
 * *spec, *stat: the two parts' slot bytes (multiples of 16); returns 0 for a row that is not imaged (its ordinary descriptor
 * is the escape, or its image spec part would not leave the mark free).  (stream_paths.h's sp_image_vals /
 * sp_image_chunk / sp_entry_unimage -- chunk k of a compacted part as chunk k of the segment below ceil(L / 2), chunk
 * k + L - ceil(L / 2) from there on -- are the slot-size arithmetic of this layout and nothing else now: a packed part's
 * chunks are not mapped back to the segment, and only tests/test_image_rule.py calls them.) */
GPUDIFF_HD static inline int gpudiff_pair_image_parts(const gpudiff_pair_row* r, uint32_t* spec, uint32_t* stat) {
    const uint32_t need = GPUDIFF_OBJ_SPEC_KEYS_EQ | GPUDIFF_OBJ_SPEC_SHAPE_EQ;
    *spec = *stat = 0u;
    if ((r->flags_a | r->flags_b) & GPUDIFF_OBJ_DECODE_ERR) return 0;
    if (r->spec_l_a != r->spec_l_b || r->spec_ar_a != r->spec_ar_b || (r->flags_b & need) != need) return 0;
    {
        const gpudiff_pair_desc d = gpudiff_pair_desc_pack(r);
        const uint64_t s = 16ull * (((uint64_t)r->spec_l_a + 1u) >> 1) + r->spec_ar_a;
        const int stat_sz = (r->flags_b & GPUDIFF_OBJ_HAS_STATUS) && r->stat_l_a == r->stat_l_b &&
                            r->stat_ar_a == r->stat_ar_b;
        if (gpudiff_pair_desc_is_escape(d.w[3]) || (s >> 4) >= GPUDIFF_PD_IMAGE_SPEC_MAX) return 0;
        *spec = (uint32_t)s;
        if (stat_sz)
            *stat = (r->flags_b & GPUDIFF_OBJ_STAT_SHAPE_EQ)
                        ? (uint32_t)(16ull * (((uint64_t)r->stat_l_a + 1u) >> 1) + r->stat_ar_a)
                        : (uint32_t)gpudiff_seg_bytes(r->stat_l_a, r->stat_ar_a);
    }
    return 1;
}
/* the image bytes of one side of the pair (a multiple of GPUDIFF_BLOB_ALIGN; B's side follows A's); 0: not imaged */
GPUDIFF_HD static inline uint64_t gpudiff_pair_image_side(const gpudiff_pair_row* r) {
    uint32_t s, t;
    if (!gpudiff_pair_image_parts(r, &s, &t)) return 0u;
    return ((uint64_t)s + t + (GPUDIFF_BLOB_ALIGN - 1u)) & ~(uint64_t)(GPUDIFF_BLOB_ALIGN - 1u);
}
/* the image form of the row's descriptor, its sides at bytes img_a and img_b of the image, with the two parts' bytes as
 * streamed given (multiples of 16, at most gpudiff_pair_image_parts': a packed part, below, is shorter than its slot);
 * the escape (K2 then reads the row and the pool) when the row is not imaged or an offset does not fit */
GPUDIFF_HD static inline gpudiff_pair_desc gpudiff_pair_desc_pack_image_parts(const gpudiff_pair_row* r, uint32_t spec,
                                                                              uint32_t stat, uint64_t img_a,
                                                                              uint64_t img_b) {
    gpudiff_pair_desc d;
    uint32_t s, t;
    if (!gpudiff_pair_image_parts(r, &s, &t) || spec > s || stat > t || ((spec | stat) & 15u) != 0u ||
        ((img_a | img_b) & (GPUDIFF_BLOB_ALIGN - 1u)) != 0u || (img_a >> 7) > 0xFFFFFFFFull ||
        (img_b >> 7) > 0xFFFFFFFFull) {
        d.w[0] = d.w[1] = d.w[2] = d.w[3] = GPUDIFF_PD_ESCAPE;
        return d;
    }
    {
        const uint64_t zw = (uint64_t)(spec >> 4) | ((uint64_t)GPUDIFF_PD_SIZE_MAX << GPUDIFF_PD_SIZE_BITS) |
                            ((uint64_t)(stat >> 4) << (2u * GPUDIFF_PD_SIZE_BITS)) |
                            ((uint64_t)gpudiff_pair_row_bits(r) << (3u * GPUDIFF_PD_SIZE_BITS));
        d.w[0] = (uint32_t)(img_a >> 7);
        d.w[1] = (uint32_t)(img_b >> 7);
        d.w[2] = (uint32_t)zw;
        d.w[3] = (uint32_t)(zw >> 32);
    }
    return d;
}
/* ... with the parts at their slots' sizes (gpudiff_pair_image_parts): the row's own arithmetic, no meta read */
GPUDIFF_HD static inline gpudiff_pair_desc gpudiff_pair_desc_pack_image(const gpudiff_pair_row* r, uint64_t img_a,
                                                                        uint64_t img_b) {
    uint32_t s = 0, t = 0;
    (void)gpudiff_pair_image_parts(r, &s, &t); /* (not imaged: the variant finds out again and escapes) */
    return gpudiff_pair_desc_pack_image_parts(r, s, t, img_a, img_b);
}
/* an upper bound on the bytes the descriptor kernel reads for one pair of a batch that images every row it can: the
 * descriptor and both image sides' chunks at the slots' sizes (packed parts are shorter, but their sizes take the metas
 * and a row has none: gpudiff_rows_image_streamed_bytes, gpudiff.h); gpudiff_pair_stream_bytes for a row that is not
 * imaged */
GPUDIFF_HD static inline uint64_t gpudiff_pair_image_bytes(const gpudiff_pair_row* r) {
    const gpudiff_pair_desc d = gpudiff_pair_desc_pack_image(r, 0u, 0u);
    if (gpudiff_pair_desc_is_escape(d.w[3])) return gpudiff_pair_stream_bytes(r);
    {
        const gpudiff_pair_geom g = gpudiff_pair_desc_unpack(d.w[0], d.w[1], d.w[2], d.w[3]);
        return sizeof(gpudiff_pair_desc) + 32ull * ((uint64_t)g.n1 + g.n2);
    }
}

GPUDIFF_HD static inline uint32_t gpudiff_meta(uint32_t tag, uint32_t len) { return (len << 3) | tag; }
GPUDIFF_HD static inline uint32_t gpudiff_meta_tag(uint32_t m) { return m & 7u; }
GPUDIFF_HD static inline uint32_t gpudiff_meta_len(uint32_t m) { return m >> 3; }
GPUDIFF_HD static inline int gpudiff_meta_is_long(uint32_t m) {
    return gpudiff_meta_tag(m) == GPUDIFF_TAG_STR && gpudiff_meta_len(m) > GPUDIFF_INLINE_MAX;
}
/* arena bytes of one leaf's value (long strings: the tail past the 8 bytes in
 * vals, its length rounded up to 4) */
GPUDIFF_HD static inline uint32_t gpudiff_meta_arena(uint32_t m) {
    return gpudiff_meta_is_long(m) ? ((gpudiff_meta_len(m) - GPUDIFF_INLINE_MAX + 3u) & ~3u) : 0u;
}
/* a segment's arena size (the row's *_ar fields): the sum of its leaves'
 * gpudiff_meta_arena, rounded up to 16 */
GPUDIFF_HD static inline uint32_t gpudiff_arena_bytes(uint32_t sum) { return (sum + 15u) & ~15u; }

/* ---- the packed region (DESIGN.md §5 "Compare image"): what the image keeps of a region whose keys and metas it drops
 * -- the spec region of every imaged pair, the status region under GPUDIFF_OBJ_STAT_SHAPE_EQ.  The leaves in key order,
 * leaf i taking gpudiff_meta_packed(m_i) bytes, then zeros to a multiple of 16:
 *
 *   string          its length rounded up to 4: the first min(len, 8) bytes from vals[i], the rest its arena tail (which
 *                   is zero padded to 4 already; a string of at most 8 bytes takes pad4(len) bytes of its vals slot)
 *   int64, float64  the 8 bytes of vals[i]
 *   null, false, true, {}, []   nothing: the meta is the value, and vals[i] is 8 zero bytes by the format
 *
 * Under equal metas leaf i lies at the same packed offset on both sides and the packed bytes hold every byte of its
 * value, so two packed regions are equal iff the regions' values are.  Never longer than vals[L] padded to 16 plus the
 * arena: a leaf takes at most its 8 bytes of vals and its tail. */
GPUDIFF_HD static inline uint32_t gpudiff_meta_packed(uint32_t m) {
    const uint32_t tag = gpudiff_meta_tag(m);
    if (tag == GPUDIFF_TAG_STR) return (gpudiff_meta_len(m) + 3u) & ~3u;
    return (tag == GPUDIFF_TAG_INT || tag == GPUDIFF_TAG_FLOAT) ? 8u : 0u;
}
/* a packed region's bytes: the sum of its leaves' gpudiff_meta_packed, rounded up to 16 */
GPUDIFF_HD static inline uint32_t gpudiff_packed_bytes(uint32_t sum) { return (sum + 15u) & ~15u; }
/* the same from a region's metas[L] */
GPUDIFF_HD static inline uint32_t gpudiff_region_packed_bytes(const uint32_t* metas, uint32_t l) {
    uint32_t sum = 0, i;
    for (i = 0; i < l; i++) sum += gpudiff_meta_packed(metas[i]);
    return gpudiff_packed_bytes(sum);
}
/* the packing itself, serially (the builder kernel does the same a wave per pair): seg the region's segment on the
 * side to pack, metas the metas that say how (A's, for both sides), dst gpudiff_region_packed_bytes(metas, l) bytes */
GPUDIFF_HD static inline uint32_t gpudiff_region_pack(const uint8_t* seg, const uint32_t* metas, uint32_t l, uint8_t* dst) {
    const uint8_t* arena = seg + 16ull * l;
    uint32_t p = 0, t = 0, i, k;
    for (i = 0; i < l; i++) {
        const uint32_t n = gpudiff_meta_packed(metas[i]), ar = gpudiff_meta_arena(metas[i]);
        for (k = 0; k < n; k++) dst[p + k] = k < 8u ? seg[8ull * i + k] : arena[t + (k - 8u)];
        p += n;
        t += ar;
    }
    for (; p & 15u; p++) dst[p] = 0u;
    return p;
}

#ifdef __cplusplus
}
#endif
#endif
