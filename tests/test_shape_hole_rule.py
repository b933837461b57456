"""include/gpudiff_format.h: the shape hole.  A row whose flags_b carries GPUDIFF_OBJ_SPEC_SHAPE_EQ beside
GPUDIFF_OBJ_SPEC_KEYS_EQ lets K2 leave the whole 128-byte lines that hold only spec keys and metas -- inside bytes
[8 L, 16 L) of the segment -- out of its stream; the descriptor says so with bit 18 of the skip L field, a value no row
below 4 MiB of spec could carry before.  Checked here: the rule at its edges, unpack(pack(row)) against a geometry
restated below, that rows without the bit pack to the four words of a restated copy of the earlier packer, that the
escape set does not depend on the bit, the bytes the stream's chunks touch against the compared span minus the hole,
the log's chunk-index mapping (kcp_amd/csrc/stream_paths.h) and the byte sum.  Plain arithmetic, so it is a
stand-alone program built with the address and undefined-behaviour sanitizers; no GPU, nothing loaded into Python."""
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include "gpudiff_format.h"
#include "stream_paths.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

static std::string g_case;
#define CHECK(x) do { if (!(x)) { std::printf("%s:%d: %s failed (case %s)\n", __FILE__, __LINE__, #x, g_case.c_str()); std::exit(1); } } while (0)

static const uint32_t kKeys = 0x8u, kShape = 0x10u;  // the two flags_b bits, written out

// the holes of L leaves, written out here: the whole 128-byte lines inside [8 L, 12 L) and inside [8 L, 16 L), in bytes
static void keys_hole_bytes(uint64_t L, uint64_t* lo, uint64_t* hi) {
    *lo = (8 * L + 127) / 128 * 128;
    *hi = 12 * L / 128 * 128;
    if (*hi <= *lo) *lo = *hi = 0;
}
static void shape_hole_bytes(uint64_t L, uint64_t* lo, uint64_t* hi) {
    *lo = (8 * L + 127) / 128 * 128;
    *hi = 16 * L / 128 * 128;
    if (*hi <= *lo) *lo = *hi = 0;
}

static void check_hole(uint32_t L) {
    g_case = "shape hole of L = " + std::to_string(L);
    uint32_t hs = 12345, hl = 12345;
    gpudiff_shape_hole(L, &hs, &hl);
    const uint64_t b0 = 16ull * hs, b1 = 16ull * (hs + (uint64_t)hl);
    if (hl) {
        CHECK(b0 >= 8ull * L && b1 <= 16ull * L);            // inside keys[] | metas[]
        CHECK(b0 % 128 == 0 && b1 % 128 == 0);                // whole lines
        CHECK(b0 < 8ull * L + 128 && b1 + 128 > 16ull * L);  // maximal
    } else {
        CHECK(hs == 0);
        CHECK((8ull * L + 127) / 128 * 128 + 128 > 16ull * L);
    }
    uint64_t lo, hi, klo, khi;
    shape_hole_bytes(L, &lo, &hi);
    CHECK(b0 == lo && b1 == hi);
    keys_hole_bytes(L, &klo, &khi);  // the key hole lies inside it, from the same first line
    if (khi > klo) CHECK(klo == lo && khi <= hi);
    if (L >= 0x40000u) return;  // the packed word K2 keeps per lane: any L a shape descriptor can carry
    const uint32_t w = gd::sp_hole_word(hs, hl);
    CHECK(gd::sp_hole_chunks(w) == hl && gd::sp_hole_bytes(w) == 16u * hl);
    if (hl) CHECK(gd::sp_hole_start(w) == hs);
    else CHECK(w == 0);
}

// the packer before the bit existed, restated word for word
static const uint64_t kOffMax = 0xFFFFFFFFull << 7, kSegMax = 0x7FFFFull << 4;
static bool must_escape(const gpudiff_pair_row& r) {
    const uint64_t sa = (uint64_t)r.spec_l_a * 16u + r.spec_ar_a, sb = (uint64_t)r.spec_l_b * 16u + r.spec_ar_b;
    const uint64_t st = (uint64_t)r.stat_l_a * 16u + r.stat_ar_a;
    if ((r.off_a & 127u) || (r.off_b & 127u) || r.off_a > kOffMax || r.off_b > kOffMax) return true;
    if ((sa & 15u) || (sb & 15u) || (st & 15u) || sa > kSegMax || sb > kSegMax || st > kSegMax) return true;
    const bool no_stat = (r.stat_l_a | r.stat_l_b | r.stat_ar_a | r.stat_ar_b) == 0u;
    return ((uint32_t)(r.stat_l_a + r.stat_l_b) != 0u) == no_stat;
}
static void old_pack(const gpudiff_pair_row& r, uint32_t w[4]) {
    if (must_escape(r)) {
        w[0] = w[1] = w[2] = w[3] = 0xFFFFFFFFu;
        return;
    }
    const uint64_t sa = (uint64_t)r.spec_l_a * 16u + r.spec_ar_a, sb = (uint64_t)r.spec_l_b * 16u + r.spec_ar_b;
    const uint64_t st = (uint64_t)r.stat_l_a * 16u + r.stat_ar_a;
    const bool err = ((r.flags_a | r.flags_b) & 0x2u) != 0u;
    const bool spec_eq = r.spec_l_a == r.spec_l_b && r.spec_ar_a == r.spec_ar_b;
    const uint32_t bits = (err ? 0x01u : 0u) | (spec_eq ? 0x02u : 0u) |
                          ((r.stat_l_a == r.stat_l_b && r.stat_ar_a == r.stat_ar_b) ? 0x04u : 0u) |
                          ((r.flags_b & 0x1u) ? 0x08u : 0u) | ((r.flags_a & 0x1u) ? 0x10u : 0u) |
                          (((r.flags_a >> 8) & 0xFFu) ? 0x20u : 0u) |
                          ((r.stat_l_a | r.stat_l_b | r.stat_ar_a | r.stat_ar_b) == 0u ? 0x40u : 0u);
    uint64_t f1 = sb >> 4;
    if (spec_eq) {
        uint64_t lo = 0, hi = 0;
        if ((r.flags_b & kKeys) && !err) keys_hole_bytes(r.spec_l_a, &lo, &hi);
        f1 = hi > lo ? r.spec_l_a : 0u;
    }
    const uint64_t zw = (sa >> 4) | (f1 << 19) | ((st >> 4) << 38) | ((uint64_t)bits << 57);
    w[0] = (uint32_t)(r.off_a >> 7);
    w[1] = (uint32_t)(r.off_b >> 7);
    w[2] = (uint32_t)zw;
    w[3] = (uint32_t)(zw >> 32);
}

// the geometry: what k_compare_flat computes from a row's four 16-B words (its row path), and the hole by the rule:
// mode 0 none (the row path), 1 the key hole alone (the bit masked), 2 the whole rule
struct Want {
    uint64_t off_a, off_b;
    uint32_t n1, n2, adj_a, adj_b;
    uint32_t seg_a, seg_b;
    uint32_t hs, hl;
    uint64_t lo, hi;  // the hole's bytes
    int kind;         // 0 no hole, 1 the key hole, 2 the shape hole
    bool err, spec_sz, stat_sz, has_st_b, no_stat, fallback;
};
static Want from_row(const gpudiff_pair_row& r, int mode) {
    Want w;
    const uint32_t v1x = r.spec_l_a, v1y = r.spec_l_b, v1z = r.spec_ar_a, v1w = r.spec_ar_b;
    const uint32_t v2x = r.stat_l_a, v2y = r.stat_l_b, v2z = r.stat_ar_a, v2w = r.stat_ar_b;
    const uint32_t v3x = r.flags_a, v3y = r.flags_b;
    w.off_a = r.off_a;
    w.off_b = r.off_b;
    w.err = ((v3x | v3y) & GPUDIFF_OBJ_DECODE_ERR) != 0u;
    const bool ok = !w.err;
    w.spec_sz = v1x == v1y && v1z == v1w;
    w.has_st_b = (v3y & GPUDIFF_OBJ_HAS_STATUS) != 0u;
    w.stat_sz = w.has_st_b && v2x == v2y && v2z == v2w;
    const uint32_t seg_a = (uint32_t)((uint64_t)v1x * 16u + v1z), seg_b = (uint32_t)((uint64_t)v1y * 16u + v1w);
    const uint32_t seg_t = (uint32_t)((uint64_t)v2x * 16u + v2z);
    const uint32_t r128 = ((seg_a + seg_t + 127u) & ~127u);
    w.no_stat = (v2x | v2y | v2z | v2w) == 0u;
    w.n1 = (ok && w.spec_sz) ? ((!w.stat_sz && w.no_stat) ? ((seg_a + 127u) & ~127u) : seg_a) >> 4 : 0u;
    w.n2 = (ok && w.stat_sz) ? (w.spec_sz ? r128 - seg_a : seg_t) >> 4 : 0u;
    w.hs = w.hl = 0;
    w.lo = w.hi = 0;
    w.kind = 0;
    w.fallback = false;
    if (mode >= 1 && (v3y & kKeys) && ok && w.spec_sz) {
        const bool shape_bit = mode >= 2 && (v3y & kShape);
        // a shape row of 4 MiB of spec or more keeps the key hole
        w.fallback = shape_bit && (uint64_t)v1x * 16u + v1z >= (1ull << 22);
        if (shape_bit && !w.fallback) {
            shape_hole_bytes(v1x, &w.lo, &w.hi);
            if (w.hi > w.lo) w.kind = 2;
        } else {
            keys_hole_bytes(v1x, &w.lo, &w.hi);
            if (w.hi > w.lo) w.kind = 1;
        }
        if (w.kind) {
            w.hs = (uint32_t)(w.lo / 16);
            w.hl = (uint32_t)((w.hi - w.lo) / 16);
            w.n1 -= w.hl;
        }
    }
    w.adj_a = seg_a - 16u * w.n1;
    w.adj_b = seg_b - 16u * w.n1;
    w.seg_a = seg_a;
    w.seg_b = seg_b;
    return w;
}

static void same(const gpudiff_pair_geom& g, const Want& w) {
    CHECK(g.off_a == w.off_a && g.off_b == w.off_b);
    CHECK(g.n1 == w.n1 && g.n2 == w.n2);
    CHECK(g.adj_a == w.adj_a && g.adj_b == w.adj_b);
    CHECK(g.hl == w.hl);
    if (w.hl) CHECK(g.hs == w.hs);
    CHECK(((g.bits & GPUDIFF_PD_ERR) != 0u) == w.err);
    CHECK(((g.bits & GPUDIFF_PD_SPEC_EQ) != 0u) == w.spec_sz);
    CHECK(((g.bits & GPUDIFF_PD_HAS_ST_B) && (g.bits & GPUDIFF_PD_STAT_EQ)) == w.stat_sz);
    CHECK(((g.bits & GPUDIFF_PD_NO_STAT) != 0u) == w.no_stat);
    CHECK((g.bits & ~0x7Fu) == 0u);
}

// Whether the 16-B chunks 0 .. n1 + n2 of one side, as the stream addresses them (byte offsets relative to the blob),
// are the compared span of that side -- old.n1 spec chunks from 0, old.n2 status chunks from the segment's end --
// minus the hole's bytes [lo, hi), in ascending order
static bool stream_is_span_minus_hole(const gpudiff_pair_geom& g, uint32_t adj, const Want& old, uint32_t seg,
                                      uint64_t lo, uint64_t hi) {
    uint32_t j = 0;
    auto next_is = [&](uint64_t byte) {
        if (j >= g.n1 + g.n2) return false;
        const uint64_t at = j < g.n1 ? 16ull * gpudiff_hole_chunk(j, g.hs, g.hl) : 16ull * j + adj;
        j++;
        return at == byte;
    };
    for (uint32_t k = 0; k < old.n1; k++)
        if (!(16ull * k >= lo && 16ull * k < hi) && !next_is(16ull * k)) return false;
    for (uint32_t k = 0; k < old.n2; k++)
        if (!next_is((uint64_t)seg + 16ull * k)) return false;
    return j == g.n1 + g.n2;
}

static uint64_t n_escaped = 0, n_packed = 0, n_shape = 0, n_keys = 0, n_none = 0, n_fallback = 0, n_spans = 0,
                n_same_words = 0, n_shape_no_keys = 0, n_hole_to_arena = 0, n_hole_to_end = 0;
static void check(const std::string& name, const gpudiff_pair_row& r) {
    g_case = name;
    const Want w = from_row(r, 2), keys_only = from_row(r, 1), old = from_row(r, 0);
    same(gpudiff_pair_row_geom(&r), old);  // an escape's lane, the row-path kernels: never a hole
    const gpudiff_pair_desc d = gpudiff_pair_desc_pack(&r);
    const bool esc = gpudiff_pair_desc_is_escape(d.w[3]) != 0;
    CHECK(esc == must_escape(r));  // the escape set: as before ...
    for (uint32_t flip : {kShape, kKeys, kShape | kKeys}) {  // ... and neither bit moves a row into or out of it
        gpudiff_pair_row q = r;
        q.flags_b ^= flip;
        CHECK((gpudiff_pair_desc_is_escape(gpudiff_pair_desc_pack(&q).w[3]) != 0) == esc);
    }
    {   // without the bit: the earlier packer's four words, and with it too wherever the rule gives no shape hole
        gpudiff_pair_row q = r;
        q.flags_b &= ~kShape;
        uint32_t ow[4];
        old_pack(q, ow);
        const gpudiff_pair_desc dq = gpudiff_pair_desc_pack(&q);
        CHECK(dq.w[0] == ow[0] && dq.w[1] == ow[1] && dq.w[2] == ow[2] && dq.w[3] == ow[3]);
        if (w.kind != 2) CHECK(d.w[0] == ow[0] && d.w[1] == ow[1] && d.w[2] == ow[2] && d.w[3] == ow[3]);
        n_same_words++;
        if (!esc) same(gpudiff_pair_desc_unpack(dq.w[0], dq.w[1], dq.w[2], dq.w[3]), keys_only);
        CHECK(gpudiff_pair_stream_bytes(&q) == 16u + 32ull * ((uint64_t)(esc ? old.n1 : keys_only.n1) + old.n2));
    }
    if (esc) {
        CHECK(d.w[0] == 0xFFFFFFFFu && d.w[1] == 0xFFFFFFFFu && d.w[2] == 0xFFFFFFFFu && d.w[3] == 0xFFFFFFFFu);
        CHECK(gpudiff_pair_stream_bytes(&r) == 16u + 32ull * ((uint64_t)old.n1 + old.n2));
        n_escaped++;
        return;
    }
    n_packed++;
    const gpudiff_pair_geom g = gpudiff_pair_desc_unpack(d.w[0], d.w[1], d.w[2], d.w[3]);
    same(g, w);
    if (!(r.flags_b & kShape)) same(g, keys_only);
    if (!(r.flags_b & kKeys)) same(g, old);  // the shape bit alone (never an encoder's row) states nothing
    if (!w.spec_sz) CHECK(g.adj_b == w.seg_b && g.n1 == 0 && g.hl == 0);
    if (w.err) CHECK(g.n1 == 0 && g.n2 == 0 && g.hl == 0);
    // the byte sum: the descriptor and both sides' streamed chunks; against the format's bytes, the hole's less
    CHECK(gpudiff_pair_stream_bytes(&r) == 16u + 32ull * ((uint64_t)g.n1 + g.n2));
    CHECK(gpudiff_pair_stream_bytes(&r) + 2u * (w.hi - w.lo) + 65u == gpudiff_pair_compare_bytes(&r) + 16u);
    n_shape += w.kind == 2;
    n_keys += w.kind == 1;
    n_none += w.kind == 0;
    n_fallback += w.fallback && w.kind == 1;
    n_shape_no_keys += (r.flags_b & (kShape | kKeys)) == kShape && w.spec_sz && !w.err;
    n_hole_to_arena += w.kind == 2 && w.hi == 16ull * r.spec_l_a;
    if (w.kind) {  // the hole holds keys and metas only, and lies in the streamed spec span
        CHECK(w.lo >= 8ull * r.spec_l_a && w.hi <= (w.kind == 2 ? 16ull : 12ull) * r.spec_l_a);
        CHECK(16ull * r.spec_l_a <= w.seg_a && w.hi <= 16ull * old.n1);
    }
    if ((uint64_t)old.n1 + old.n2 <= 8192u) {
        CHECK(stream_is_span_minus_hole(g, g.adj_a, old, w.seg_a, w.lo, w.hi));
        CHECK(stream_is_span_minus_hole(g, g.adj_b, old, w.seg_b, w.lo, w.hi));
        n_spans++;
    }
    // the log's mapping: streamed chunk k's entry back to the segment's chunk, any differing dwords
    {
        const uint32_t hw = gd::sp_hole_word(g.hs, g.hl);
        // every chunk of the small directed rows; of a random or a huge row the first ones and those around the hole's start
        const bool all = name[0] != 'r' && g.n1 <= 8192u;
        for (uint32_t k = 0; k < g.n1; k++) {
            if (!all && k >= 16u && k + 16u < g.hs) k = g.hs - 16u;
            if (!all && k >= g.hs + 16u) break;
            const uint32_t dw = 1u + k % 15u;
            const uint32_t e = gd::sp_entry_unhole(gd::sp_entry(k, dw), hw);
            CHECK(e == gd::sp_entry(gpudiff_hole_chunk(k, g.hs, g.hl), dw));
            const uint64_t b = gd::sp_entry_byte(e, 0);
            CHECK(b < w.lo || b >= w.hi || !w.kind);  // never a byte of the hole
        }
        if (g.n1) {  // the last streamed chunk is the span's last, or the one before a hole that runs to the span's end
            const uint32_t e = gd::sp_entry_unhole(gd::sp_entry(g.n1 - 1u, 15u), hw);
            const bool to_end = w.kind && w.hi == 16ull * old.n1;  // (L = 16 without an arena: metas[] end the span)
            CHECK(to_end == (w.kind && g.n1 == g.hs));
            CHECK(gd::sp_entry_byte(e, 0) == (to_end ? w.lo - 16u : 16ull * (old.n1 - 1u)));
            n_hole_to_end += to_end;
        }
        if (w.kind == 2 && g.hs + 0u < g.n1) {  // the first chunk behind the hole: the last metas or the arena's start
            const uint32_t e = gd::sp_entry_unhole(gd::sp_entry(g.hs, 1u), hw);
            CHECK(gd::sp_entry_byte(e, 0) == w.hi);
            const gd::SpWhere at = gd::sp_classify(w.hi, r.spec_l_a);
            if (w.hi == 16ull * r.spec_l_a) CHECK(at.cls == gd::SP_ARENA && at.idx == 0);
            else CHECK(at.cls == gd::SP_META);
        }
    }
}

static gpudiff_pair_row zero_row() {
    gpudiff_pair_row r;
    std::memset(&r, 0, sizeof r);
    return r;
}

// xorshift64*: the random rows are the same on every run
static uint64_t g_rng = 0xD1B54A32D192ED03ull;
static uint64_t rnd() {
    g_rng ^= g_rng >> 12;
    g_rng ^= g_rng << 25;
    g_rng ^= g_rng >> 27;
    return g_rng * 0x2545F4914F6CDD1Dull;
}
static uint32_t rnd_leaves() {
    switch (rnd() % 9) {
        case 0: return 0;
        case 1: return (uint32_t)(rnd() % 4);
        case 2: return 0x7FFFFu - (uint32_t)(rnd() % 3);  // at the size field's limit when the arena is empty
        case 3: return 0x80000u + (uint32_t)(rnd() % 3);  // past it
        case 4: return (uint32_t)rnd();                    // 16 L past 32 bits
        case 5: return 12u + (uint32_t)(rnd() % 40);       // around the first holes
        case 6: return 0x40000u - 2u + (uint32_t)(rnd() % 4);  // around the shape code's limit
        default: return (uint32_t)(rnd() % 400);
    }
}
static uint32_t rnd_arena() {
    switch (rnd() % 8) {
        case 0: case 1: return 0;
        case 2: return (uint32_t)(rnd() % 64);                      // not always a multiple of 16
        case 3: return 0x7FFFF0u - 16u * (uint32_t)(rnd() % 400);  // near the limit
        case 4: return (uint32_t)rnd() & ~15u;
        default: return 16u * (uint32_t)(rnd() % 300);
    }
}
static uint64_t rnd_off() {
    switch (rnd() % 8) {
        case 0: return 0;
        case 1: return kOffMax - 128u * (rnd() % 3);
        case 2: return kOffMax + 128u * (1 + rnd() % 3);
        case 3: return (rnd() % (1ull << 40));  // mostly misaligned
        default: return 128u * (rnd() % (1ull << 29));
    }
}

struct Edge { uint32_t L; uint64_t lo, hi; };

int main() {
    // ---- the hole rule
    for (uint32_t L = 0; L <= 4096; L++) check_hole(L);
    for (uint32_t L = 0x40000u - 200u; L <= 0x40000u + 8u; L++) check_hole(L);
    for (uint32_t L : {0x7FFFFu, 0x80000u, 0xFFFFFFFFu, 0x80000000u, 0x10000000u, 0x0FFFFFFFu}) check_hole(L);  // no wrap
    // the rule's edges, each hole written out in bytes (0, 0: none)
    const Edge edges[] = {{0, 0, 0}, {15, 0, 0}, {16, 128, 256}, {17, 0, 0}, {23, 0, 0}, {24, 256, 384}, {25, 256, 384},
                          {31, 256, 384}, {32, 256, 512}, {33, 384, 512}, {47, 384, 640}, {48, 384, 768},
                          {49, 512, 768}, {184, 1536, 2944}, {0x3FFFFu, 2097152, 4194176},
                          {0x40000u, 2097152, 3145728}};  // 2^18 leaves are 4 MiB: the key hole, [8 L, 12 L) exactly
    for (const Edge& e : edges)
        for (uint32_t ar : {0u, 16u, 48u, 1008u})
            for (uint32_t shape = 0; shape < 6; shape++)
                for (uint32_t bits = 0; bits < 4; bits++) {
                    gpudiff_pair_row r = zero_row();
                    r.off_a = 128u * 7u, r.off_b = 128u * 1000u;
                    r.spec_l_a = r.spec_l_b = e.L;
                    r.spec_ar_a = r.spec_ar_b = ar;
                    r.flags_b = ((bits & 1u) ? kKeys : 0u) | ((bits & 2u) ? kShape : 0u);
                    if (shape == 1) r.stat_l_a = r.stat_l_b = 17, r.flags_a = GPUDIFF_OBJ_HAS_STATUS, r.flags_b |= GPUDIFF_OBJ_HAS_STATUS;
                    if (shape == 2) r.stat_l_a = 17, r.stat_l_b = 18, r.flags_b |= GPUDIFF_OBJ_HAS_STATUS;  // spec only
                    if (shape == 3) r.stat_l_a = r.stat_l_b = 5, r.stat_ar_a = r.stat_ar_b = 32;  // B without the key
                    if (shape == 4) r.spec_ar_b = ar + 16u, r.stat_l_a = r.stat_l_b = 3, r.flags_b |= GPUDIFF_OBJ_HAS_STATUS;
                    if (shape == 5) r.flags_a = GPUDIFF_OBJ_DECODE_ERR;  // never an encoder's row with the bits
                    check("L " + std::to_string(e.L) + " arena " + std::to_string(ar) + " shape " +
                              std::to_string(shape) + " bits " + std::to_string(bits), r);
                    if (bits == 3 && shape <= 3) {
                        const gpudiff_pair_desc d = gpudiff_pair_desc_pack(&r);
                        CHECK(!gpudiff_pair_desc_is_escape(d.w[3]));
                        const gpudiff_pair_geom g = gpudiff_pair_desc_unpack(d.w[0], d.w[1], d.w[2], d.w[3]);
                        // 2^18 - 1 leaves with an arena are 4 MiB or more as well: the key hole [8 L rounded up, 12 L rounded down)
                        uint64_t lo = e.lo, hi = e.hi;
                        if (e.L == 0x3FFFFu && ar) keys_hole_bytes(e.L, &lo, &hi);
                        CHECK(16ull * g.hl == hi - lo);
                        if (g.hl) CHECK(16ull * g.hs == lo);
                    }
                }
    // ---- random rows, as tests/test_keys_hole_rule.py draws them: the key bit on three quarters, the shape bit on half
    for (uint32_t i = 0; i < 1000000u; i++) {
        gpudiff_pair_row r = zero_row();
        r.off_a = rnd_off();
        r.off_b = rnd_off();
        r.spec_l_a = rnd_leaves(), r.spec_ar_a = rnd_arena();
        r.spec_l_b = rnd_leaves(), r.spec_ar_b = rnd_arena();
        r.stat_l_a = rnd_leaves(), r.stat_ar_a = rnd_arena();
        r.stat_l_b = rnd_leaves(), r.stat_ar_b = rnd_arena();
        if (rnd() % 4) r.spec_l_b = r.spec_l_a;
        if (rnd() % 4) r.spec_ar_b = r.spec_ar_a;
        if (rnd() & 1u) r.stat_l_b = r.stat_l_a;
        if (rnd() & 1u) r.stat_ar_b = r.stat_ar_a;
        if (rnd() % 4 == 0) r.stat_l_a = r.stat_l_b = r.stat_ar_a = r.stat_ar_b = 0;
        const uint64_t kind = rnd() % 4;
        if (kind <= 1) {  // a row as the encoder makes them: aligned, small, arenas in 16-B units
            r.off_a &= ~127ull, r.off_b &= ~127ull;
            r.off_a %= 1ull << 38, r.off_b %= 1ull << 38;
            const bool eq = r.spec_l_a == r.spec_l_b;
            r.spec_l_a %= 500u, r.spec_l_b = eq ? r.spec_l_a : r.spec_l_b % 500u;
            r.stat_l_a %= 100u, r.stat_l_b %= 100u;
            const bool eqa = r.spec_ar_a == r.spec_ar_b;
            r.spec_ar_a = (r.spec_ar_a % 4096u) & ~15u, r.spec_ar_b = eqa ? r.spec_ar_a : (r.spec_ar_b % 4096u) & ~15u;
            r.stat_ar_a = r.stat_l_a ? (r.stat_ar_a % 1024u) & ~15u : 0u;
            r.stat_ar_b = r.stat_l_b ? (r.stat_ar_b % 1024u) & ~15u : 0u;
        } else if (kind == 2) {  // aligned and with a status that fits, the spec sizes as drawn: the large rows that pack
            r.off_a = (r.off_a & ~127ull) % (1ull << 38), r.off_b = (r.off_b & ~127ull) % (1ull << 38);
            r.stat_l_a = r.stat_l_b = 1u + r.stat_l_a % 50u;
            r.stat_ar_a = r.stat_ar_b = 0u;
        }
        const uint64_t f = rnd();
        r.flags_a = ((f & 1u) ? GPUDIFF_OBJ_HAS_STATUS : 0u) | ((f & 0x70u) == 0u ? GPUDIFF_OBJ_DECODE_ERR : 0u) |
                    ((f & 0x100u) ? (uint32_t)((f >> 16) & 0xFFu) << GPUDIFF_OBJ_SEED_SHIFT : 0u) | ((f & 0x200u) ? GPUDIFF_OBJ_FRESH : 0u);
        r.flags_b = ((f & 2u) ? GPUDIFF_OBJ_HAS_STATUS : 0u) | ((f & 0x7000u) == 0u ? GPUDIFF_OBJ_DECODE_ERR : 0u) |
                    ((f & 0x30000000u) ? kKeys : 0u) | ((f & 0x40000000u) ? kShape : 0u);
        r.pair_id = (uint32_t)rnd();
        r.cluster_id = (uint32_t)rnd();
        check("random row " + std::to_string(i), r);
    }
    std::printf("packed %llu escaped %llu shape %llu keys %llu none %llu fallback %llu spans %llu same words %llu "
                "shape bit alone %llu hole to the arena %llu hole to the span's end %llu\n",
                (unsigned long long)n_packed, (unsigned long long)n_escaped, (unsigned long long)n_shape,
                (unsigned long long)n_keys, (unsigned long long)n_none, (unsigned long long)n_fallback,
                (unsigned long long)n_spans, (unsigned long long)n_same_words, (unsigned long long)n_shape_no_keys,
                (unsigned long long)n_hole_to_arena, (unsigned long long)n_hole_to_end);
    // the rows must have exercised every outcome in numbers
    CHECK(n_packed > 100000 && n_escaped > 100000 && n_shape > 20000 && n_keys > 10000 && n_none > 100000);
    CHECK(n_fallback > 200 && n_spans > 100000 && n_same_words > 1000000 && n_shape_no_keys > 10000);
    CHECK(n_hole_to_arena > 1000 && n_hole_to_end > 500);
    std::printf("ok\n");
    return 0;
}
'''


def test_shape_hole_rule():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/bin/hipcc"
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        exe = os.path.join(d, "t")
        with open(src, "w") as f:
            f.write(SRC)
        subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "kcp_amd", "csrc"), src, "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
        print(r.stdout)
        assert r.stdout.strip().endswith("ok")
