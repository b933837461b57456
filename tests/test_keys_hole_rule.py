"""include/gpudiff_format.h: the key hole.  A row whose flags_b carries GPUDIFF_OBJ_SPEC_KEYS_EQ lets K2 leave the
whole 128-byte lines that hold only spec keys out of its stream; the descriptor carries the spec leaf count where it
carried B's (redundant) spec size.  Checked here: the hole rule itself, unpack(pack(row)) against a geometry restated
below, the bytes the stream's chunks touch against today's compared span minus the hole, that rows without the bit
and rows with unequal spec sizes unpack as before, that the escape set has not moved, and that the log's chunk-index
mapping (kcp_amd/csrc/stream_paths.h) is the inverse of the stream's.  Plain arithmetic, so it is a stand-alone
program built with the address and undefined-behaviour sanitizers; no GPU, nothing loaded into Python."""
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

// the hole of L leaves, written out here: the whole 128-byte units inside [8 L, 12 L), in bytes
static void hole_bytes(uint64_t L, uint64_t* lo, uint64_t* hi) {
    *lo = (8 * L + 127) / 128 * 128;
    *hi = 12 * L / 128 * 128;
    if (*hi <= *lo) *lo = *hi = 0;
}

static void check_hole(uint32_t L) {
    g_case = "hole of L = " + std::to_string(L);
    uint32_t hs = 12345, hl = 12345;
    gpudiff_keys_hole(L, &hs, &hl);
    const uint64_t b0 = 16ull * hs, b1 = 16ull * (hs + (uint64_t)hl);
    if (hl) {
        CHECK(b0 >= 8ull * L && b1 <= 12ull * L);       // inside keys[]
        CHECK(b0 % 128 == 0 && b1 % 128 == 0);           // whole units
        CHECK(b0 < 8ull * L + 128 && b1 + 128 > 12ull * L);  // maximal: no unit more fits at either end
    } else {
        CHECK(hs == 0);
        CHECK((8ull * L + 127) / 128 * 128 + 128 > 12ull * L);  // no aligned unit lies inside keys[]
    }
    uint64_t lo, hi;
    hole_bytes(L, &lo, &hi);
    CHECK(b0 == lo && b1 == hi);
    // the packed word K2 keeps per lane: any L a descriptor can carry
    if (L > 0x7FFFFu) return;
    const uint32_t w = gd::sp_hole_word(hs, hl);
    CHECK(gd::sp_hole_chunks(w) == hl && gd::sp_hole_bytes(w) == 16u * hl);
    if (hl) CHECK(gd::sp_hole_start(w) == hs);
    else CHECK(w == 0);
}

// today's geometry: what k_compare_flat computes from a row's four 16-B words (its row path, for a valid lane)
struct Want {
    uint64_t off_a, off_b;
    uint32_t n1, n2, adj_a, adj_b;
    uint32_t seg_a, seg_b;
    uint32_t hs, hl;
    bool err, spec_sz, stat_sz, has_st_b, no_stat, has_st_a, seeded;
};
static Want from_row(const gpudiff_pair_row& r, bool with_hole) {
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
    // the hole: the bit, equal spec sizes, no error
    if (with_hole && (v3y & 0x8u) && ok && w.spec_sz) {
        uint64_t lo, hi;
        hole_bytes(v1x, &lo, &hi);
        if (hi > lo) {
            w.hs = (uint32_t)(lo / 16);
            w.hl = (uint32_t)((hi - lo) / 16);
            w.n1 -= w.hl;  // the streamed spec chunks
        }
    }
    w.adj_a = seg_a - 16u * w.n1;
    w.adj_b = seg_b - 16u * w.n1;
    w.seg_a = seg_a;
    w.seg_b = seg_b;
    w.has_st_a = (v3x & GPUDIFF_OBJ_HAS_STATUS) != 0u;
    w.seeded = ((v3x >> GPUDIFF_OBJ_SEED_SHIFT) & 0xFFu) != 0u;
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
    CHECK(((g.bits & GPUDIFF_PD_HAS_ST_B) != 0u) == w.has_st_b);
    CHECK(((g.bits & GPUDIFF_PD_HAS_ST_B) && (g.bits & GPUDIFF_PD_STAT_EQ)) == w.stat_sz);
    CHECK(((g.bits & GPUDIFF_PD_NO_STAT) != 0u) == w.no_stat);
    CHECK(((g.bits & GPUDIFF_PD_HAS_ST_A) != 0u) == w.has_st_a);
    CHECK(((g.bits & GPUDIFF_PD_SEED) != 0u) == w.seeded);
    CHECK((g.bits & ~0x7Fu) == 0u);
}

// the fields' limits, written out here and not taken from the header's macros
static const uint64_t kOffMax = 0xFFFFFFFFull << 7, kSegMax = 0x7FFFFull << 4;
static bool must_escape(const gpudiff_pair_row& r) {
    const uint64_t sa = (uint64_t)r.spec_l_a * 16u + r.spec_ar_a, sb = (uint64_t)r.spec_l_b * 16u + r.spec_ar_b;
    const uint64_t st = (uint64_t)r.stat_l_a * 16u + r.stat_ar_a;
    if ((r.off_a & 127u) || (r.off_b & 127u) || r.off_a > kOffMax || r.off_b > kOffMax) return true;
    if ((sa & 15u) || (sb & 15u) || (st & 15u) || sa > kSegMax || sb > kSegMax || st > kSegMax) return true;
    const bool no_stat = (r.stat_l_a | r.stat_l_b | r.stat_ar_a | r.stat_ar_b) == 0u;
    return ((uint32_t)(r.stat_l_a + r.stat_l_b) != 0u) == no_stat;
}

// Whether the 16-B chunks 0 .. n1 + n2 of one side, as the stream addresses them (byte offsets relative to the blob),
// are today's compared span of that side -- old.n1 spec chunks from 0, old.n2 status chunks from the segment's end --
// minus the hole's bytes [lo, hi), in ascending order
static bool stream_is_span_minus_hole(const gpudiff_pair_geom& g, uint32_t adj, const Want& old, uint32_t seg,
                                      uint64_t lo, uint64_t hi) {
    uint32_t j = 0;  // the stream's next chunk
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

static uint64_t n_escaped = 0, n_packed = 0, n_holes = 0, n_spans = 0;
static void check(const std::string& name, const gpudiff_pair_row& r) {
    g_case = name;
    const Want w = from_row(r, true), old = from_row(r, false);
    same(gpudiff_pair_row_geom(&r), old);  // an escape's lane, the row-path kernels: never a hole
    const gpudiff_pair_desc d = gpudiff_pair_desc_pack(&r);
    const bool esc = gpudiff_pair_desc_is_escape(d.w[3]) != 0;
    CHECK(esc == must_escape(r));  // the escape set: as before, whatever the bit says
    {   // ... and the bit alone never moves a row into or out of it
        gpudiff_pair_row q = r;
        q.flags_b ^= GPUDIFF_OBJ_SPEC_KEYS_EQ;
        CHECK((gpudiff_pair_desc_is_escape(gpudiff_pair_desc_pack(&q).w[3]) != 0) == esc);
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
    if (!(r.flags_b & GPUDIFF_OBJ_SPEC_KEYS_EQ)) same(g, old);  // without the bit: today's geometry
    if (!w.spec_sz) CHECK(g.adj_b == w.seg_b && g.n1 == 0 && g.hl == 0);  // SPEC_EQ clear: B's own size is kept
    if (w.err) CHECK(g.n1 == 0 && g.n2 == 0 && g.hl == 0);
    CHECK(gpudiff_pair_stream_bytes(&r) == 16u + 32ull * ((uint64_t)w.n1 + w.n2));
    CHECK(gpudiff_pair_stream_bytes(&r) + 32ull * w.hl + 65u == gpudiff_pair_compare_bytes(&r) + 16u);
    n_holes += w.hl != 0;
    // the bytes the chunks touch, both sides: today's span minus the hole (small pairs: a chunk at a time)
    if ((uint64_t)old.n1 + old.n2 <= 8192u) {
        uint64_t lo = 0, hi = 0;
        if (w.hl) hole_bytes(r.spec_l_a, &lo, &hi);
        if (w.hl) CHECK(hi <= 12ull * r.spec_l_a && 12ull * r.spec_l_a <= w.seg_a && lo >= 8ull * r.spec_l_a);
        CHECK(stream_is_span_minus_hole(g, g.adj_a, old, w.seg_a, lo, hi));
        CHECK(stream_is_span_minus_hole(g, g.adj_b, old, w.seg_b, lo, hi));
        n_spans++;
    }
    // the log's mapping: streamed chunk k's entry back to the segment's chunk, any differing dwords
    {
        const uint32_t hw = gd::sp_hole_word(g.hs, g.hl);
        // (every chunk of the directed rows; of a random row the first ones and those around the hole's start)
        const bool all = name[0] != 'r';
        for (uint32_t k = 0; k < g.n1; k++) {
            if (!all && k >= 16u && k + 16u < g.hs) k = g.hs - 16u;
            if (!all && k >= g.hs + 16u) break;
            const uint32_t dw = 1u + k % 15u;
            CHECK(gd::sp_entry_unhole(gd::sp_entry(k, dw), hw) == gd::sp_entry(gpudiff_hole_chunk(k, g.hs, g.hl), dw));
        }
        if (g.n1) {  // ... and the last streamed chunk is the span's last
            const uint32_t e = gd::sp_entry_unhole(gd::sp_entry(g.n1 - 1u, 15u), hw);
            CHECK(gd::sp_entry_byte(e, 0) == 16ull * (old.n1 - 1u));
        }
    }
}

static gpudiff_pair_row zero_row() {
    gpudiff_pair_row r;
    std::memset(&r, 0, sizeof r);
    return r;
}

// xorshift64*: the random rows are the same on every run
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    g_rng ^= g_rng >> 12;
    g_rng ^= g_rng << 25;
    g_rng ^= g_rng >> 27;
    return g_rng * 0x2545F4914F6CDD1Dull;
}
static uint32_t rnd_leaves() {
    switch (rnd() % 8) {
        case 0: return 0;
        case 1: return (uint32_t)(rnd() % 4);
        case 2: return 0x7FFFFu - (uint32_t)(rnd() % 3);  // at the field's limit when the arena is empty
        case 3: return 0x80000u + (uint32_t)(rnd() % 3);  // past it
        case 4: return (uint32_t)rnd();                    // 16 L past 32 bits
        case 5: return 28u + (uint32_t)(rnd() % 24);       // around the first holes
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

int main() {
    // ---- the hole rule
    for (uint32_t L = 0; L <= 4096; L++) check_hole(L);
    for (uint32_t L = 0x7FFFFu - 200u; L <= 0x7FFFFu; L++) check_hole(L);  // the descriptor's size field: 16 L fits
    for (uint32_t L : {0x80000u, 0xFFFFFFFFu, 0x80000000u, 0x15555555u, 0x15555556u}) check_hole(L);  // no wrap
    {
        uint32_t hs, hl;
        g_case = "the first holes";
        for (uint32_t L = 0; L < 32; L++) { gpudiff_keys_hole(L, &hs, &hl); CHECK(hl == 0); }
        gpudiff_keys_hole(32, &hs, &hl);
        CHECK(hs == 16 && hl == 8);  // keys[32] is bytes [256, 384): one line
        for (uint32_t L = 33; L <= 42; L++) { gpudiff_keys_hole(L, &hs, &hl); CHECK(hl == 0); }
        for (uint32_t L = 43; L <= 48; L++) {  // keys[43] is bytes [344, 516): the line [384, 512)
            gpudiff_keys_hole(L, &hs, &hl);
            CHECK(hs == 24 && hl == 8);
        }
        for (uint32_t L = 49; L <= 53; L++) { gpudiff_keys_hole(L, &hs, &hl); CHECK(hl == 0); }  // [392, 588) .. [424, 636)
        gpudiff_keys_hole(184, &hs, &hl);
        CHECK(16u * hl == 640u && 16u * hs == 1536u);
    }
    // ---- directed rows
    for (uint32_t L : {0u, 1u, 31u, 32u, 33u, 42u, 43u, 46u, 47u, 48u, 64u, 184u, 185u, 1000u})
        for (uint32_t ar : {0u, 16u, 48u, 1008u})
            for (uint32_t shape = 0; shape < 6; shape++)
                for (uint32_t bit = 0; bit < 2; bit++) {
                    gpudiff_pair_row r = zero_row();
                    r.off_a = 128u * 7u, r.off_b = 128u * 1000u;
                    r.spec_l_a = r.spec_l_b = L;
                    r.spec_ar_a = r.spec_ar_b = ar;
                    r.flags_b = bit ? GPUDIFF_OBJ_SPEC_KEYS_EQ : 0u;
                    if (shape == 1) r.stat_l_a = r.stat_l_b = 17, r.flags_a = GPUDIFF_OBJ_HAS_STATUS, r.flags_b |= GPUDIFF_OBJ_HAS_STATUS;
                    if (shape == 2) r.stat_l_a = 17, r.stat_l_b = 18, r.flags_b |= GPUDIFF_OBJ_HAS_STATUS;  // spec only
                    if (shape == 3) r.stat_l_a = r.stat_l_b = 5, r.stat_ar_a = r.stat_ar_b = 32;  // B without the key
                    if (shape == 4) r.spec_ar_b = ar + 16u, r.stat_l_a = r.stat_l_b = 3, r.flags_b |= GPUDIFF_OBJ_HAS_STATUS;
                    if (shape == 5) r.flags_a = GPUDIFF_OBJ_DECODE_ERR;  // never an encoder's row with the bit
                    check("L " + std::to_string(L) + " arena " + std::to_string(ar) + " shape " + std::to_string(shape) +
                              " bit " + std::to_string(bit), r);
                    if (bit && shape <= 3) {
                        const gpudiff_pair_desc d = gpudiff_pair_desc_pack(&r);
                        const gpudiff_pair_geom g = gpudiff_pair_desc_unpack(d.w[0], d.w[1], d.w[2], d.w[3]);
                        CHECK((g.hl != 0) == (L == 32 || L >= 43));
                    }
                }
    {   // the size field's limit: the largest L a descriptor can carry, with the bit
        gpudiff_pair_row r = zero_row();
        r.spec_l_a = r.spec_l_b = 0x7FFFFu;
        r.flags_b = GPUDIFF_OBJ_SPEC_KEYS_EQ;
        check("L at the size field's limit", r);
        const gpudiff_pair_desc d = gpudiff_pair_desc_pack(&r);
        CHECK(!gpudiff_pair_desc_is_escape(d.w[3]));
        uint64_t lo, hi;
        hole_bytes(0x7FFFFu, &lo, &hi);
        CHECK(hi > lo && gpudiff_pair_desc_unpack(d.w[0], d.w[1], d.w[2], d.w[3]).hl == (hi - lo) / 16);
        r.spec_l_a = r.spec_l_b = 0x80000u;
        check("L past the size field's limit", r);
        r.spec_l_a = r.spec_l_b = 0x40000u;
        r.spec_ar_a = r.spec_ar_b = (uint32_t)kSegMax - 16u * 0x40000u;
        check("L and the arena at the limit", r);
    }
    // ---- random rows, as tests/test_pair_desc_rule.py draws them, the bit on half of them
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
        if (rnd() % 2 == 0) {  // a row as the encoder makes them: aligned, small, arenas in 16-B units
            r.off_a &= ~127ull, r.off_b &= ~127ull;
            r.off_a %= 1ull << 38, r.off_b %= 1ull << 38;
            const bool eq = r.spec_l_a == r.spec_l_b;
            r.spec_l_a %= 500u, r.spec_l_b = eq ? r.spec_l_a : r.spec_l_b % 500u;
            r.stat_l_a %= 100u, r.stat_l_b %= 100u;
            const bool eqa = r.spec_ar_a == r.spec_ar_b;
            r.spec_ar_a = (r.spec_ar_a % 4096u) & ~15u, r.spec_ar_b = eqa ? r.spec_ar_a : (r.spec_ar_b % 4096u) & ~15u;
            r.stat_ar_a = r.stat_l_a ? (r.stat_ar_a % 1024u) & ~15u : 0u;
            r.stat_ar_b = r.stat_l_b ? (r.stat_ar_b % 1024u) & ~15u : 0u;
        }
        const uint64_t f = rnd();
        r.flags_a = ((f & 1u) ? GPUDIFF_OBJ_HAS_STATUS : 0u) | ((f & 0x70u) == 0u ? GPUDIFF_OBJ_DECODE_ERR : 0u) |
                    ((f & 0x100u) ? (uint32_t)((f >> 16) & 0xFFu) << GPUDIFF_OBJ_SEED_SHIFT : 0u) | ((f & 0x200u) ? GPUDIFF_OBJ_FRESH : 0u);
        r.flags_b = ((f & 2u) ? GPUDIFF_OBJ_HAS_STATUS : 0u) | ((f & 0x7000u) == 0u ? GPUDIFF_OBJ_DECODE_ERR : 0u) |
                    ((f & 0x10000000u) ? GPUDIFF_OBJ_SPEC_KEYS_EQ : 0u);
        r.pair_id = (uint32_t)rnd();
        r.cluster_id = (uint32_t)rnd();
        check("random row " + std::to_string(i), r);
    }
    // the random rows must have exercised every outcome in numbers
    CHECK(n_packed > 100000 && n_escaped > 100000 && n_holes > 20000 && n_spans > 100000);
    std::printf("ok\n");
    return 0;
}
'''


def test_keys_hole_rule():
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
        assert r.stdout.strip() == "ok"
