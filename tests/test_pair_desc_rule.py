"""include/gpudiff_format.h: the 16-byte pair descriptor K2 streams from in place of the 64-byte row.  What K2 takes
from unpack(pack(row)) must be what it computes from the row itself -- the formulas of k_compare_flat's row path,
restated below -- and a row takes the escape exactly when a field does not fit.  Plain arithmetic, so it is checked
in a stand-alone program built with the address and undefined-behaviour sanitizers; no GPU, nothing loaded into
Python."""
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include "gpudiff_format.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

static std::string g_case;
#define CHECK(x) do { if (!(x)) { std::printf("%s:%d: %s failed (case %s)\n", __FILE__, __LINE__, #x, g_case.c_str()); std::exit(1); } } while (0)

// what k_compare_flat computes from a row's four 16-B words (its row path, for a valid lane)
struct Want {
    uint64_t off_a, off_b;
    uint32_t n1, n2, adj_a, adj_b;
    bool err, spec_sz, stat_sz, has_st_b, no_stat, has_st_a, seeded;
};
static Want from_row(const gpudiff_pair_row& r) {
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
    w.adj_a = seg_a - 16u * w.n1;
    w.adj_b = seg_b - 16u * w.n1;
    w.has_st_a = (v3x & GPUDIFF_OBJ_HAS_STATUS) != 0u;
    w.seeded = ((v3x >> GPUDIFF_OBJ_SEED_SHIFT) & 0xFFu) != 0u;
    return w;
}

static void same(const gpudiff_pair_geom& g, const Want& w) {
    CHECK(g.off_a == w.off_a && g.off_b == w.off_b);
    CHECK(g.n1 == w.n1 && g.n2 == w.n2);
    CHECK(g.adj_a == w.adj_a && g.adj_b == w.adj_b);
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
    // K2 joins the status region when stat_l_a + stat_l_b != 0: without the row that is "not NO_STAT"
    const bool no_stat = (r.stat_l_a | r.stat_l_b | r.stat_ar_a | r.stat_ar_b) == 0u;
    return ((uint32_t)(r.stat_l_a + r.stat_l_b) != 0u) == no_stat;
}

static uint64_t n_escaped = 0, n_packed = 0;
static void check(const std::string& name, const gpudiff_pair_row& r, int want_escape /* -1: by must_escape */) {
    g_case = name;
    const Want w = from_row(r);
    same(gpudiff_pair_row_geom(&r), w);  // an escape's lane in K2
    const gpudiff_pair_desc d = gpudiff_pair_desc_pack(&r);
    const bool esc = gpudiff_pair_desc_is_escape(d.w[3]) != 0;
    CHECK(esc == must_escape(r));
    if (want_escape >= 0) CHECK(esc == (want_escape != 0));
    if (esc) {
        CHECK(d.w[0] == 0xFFFFFFFFu && d.w[1] == 0xFFFFFFFFu && d.w[2] == 0xFFFFFFFFu && d.w[3] == 0xFFFFFFFFu);
        n_escaped++;
        return;
    }
    n_packed++;
    same(gpudiff_pair_desc_unpack(d.w[0], d.w[1], d.w[2], d.w[3]), w);
    // what K2 relies on where it has no row: a status join exactly when not NO_STAT
    CHECK(((uint32_t)(r.stat_l_a + r.stat_l_b) != 0u) == !w.no_stat);
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
        case 4: return rnd() & ~127ull;
        default: return 128u * (rnd() % (1ull << 29));
    }
}

int main() {
    {
        gpudiff_pair_row r = zero_row();
        check("every field 0", r, 0);
        r.flags_b = GPUDIFF_OBJ_HAS_STATUS;
        check("every field 0, B has status", r, 0);
    }
    // every field at its maximum, the segment bytes made of leaves alone, of one leaf and the arena, and of both
    for (int shape = 0; shape < 3; shape++)
        for (uint32_t fl = 0; fl < 32; fl++) {
            gpudiff_pair_row r = zero_row();
            r.off_a = r.off_b = kOffMax;
            const uint32_t l = shape == 0 ? 0x7FFFFu : shape == 1 ? 1u : 0x40000u;
            const uint32_t ar = (uint32_t)kSegMax - 16u * l;
            r.spec_l_a = r.spec_l_b = r.stat_l_a = l;
            r.spec_ar_a = r.spec_ar_b = r.stat_ar_a = ar;
            r.stat_l_b = (fl & 1u) ? l : l - 1u;  // status sizes equal or not
            r.stat_ar_b = ar;
            r.flags_a = ((fl & 2u) ? GPUDIFF_OBJ_HAS_STATUS : 0u) | ((fl & 4u) ? 0xFFu << GPUDIFF_OBJ_SEED_SHIFT : 0u);
            r.flags_b = ((fl & 8u) ? GPUDIFF_OBJ_HAS_STATUS | GPUDIFF_OBJ_FRESH : 0u) | ((fl & 16u) ? GPUDIFF_OBJ_DECODE_ERR : 0u);
            r.pair_id = r.cluster_id = 0xFFFFFFFFu;
            check("every field at its maximum, shape " + std::to_string(shape) + " flags " + std::to_string(fl), r, 0);
            for (int f = 0; f < 5; f++) {  // ... and each one step past it
                gpudiff_pair_row q = r;
                if (f == 0) q.off_a += 128u;
                if (f == 1) q.off_b += 128u;
                if (f == 2) q.spec_ar_a += 16u;
                if (f == 3) q.spec_ar_b += 16u;
                if (f == 4) q.stat_ar_a += 16u;
                check("maximum + 1, field " + std::to_string(f) + " shape " + std::to_string(shape), q, 1);
                gpudiff_pair_row p = r;  // one leaf more is 16 bytes more
                if (f == 2) p.spec_l_a += 1u;
                if (f == 3) p.spec_l_b += 1u;
                if (f == 4) p.stat_l_a += 1u;
                if (f >= 2) check("maximum + 1 leaf, field " + std::to_string(f) + " shape " + std::to_string(shape), p, 1);
            }
        }
    {   // status B is not in the descriptor: any size of it fits
        gpudiff_pair_row r = zero_row();
        r.stat_l_a = 1;
        r.stat_l_b = 0x7FFFFFFFu;
        r.stat_ar_b = 0xFFFFFFF0u;
        r.flags_b = GPUDIFF_OBJ_HAS_STATUS;
        check("status B beyond every field", r, 0);
    }
    {   // 16 L + arena: equal segment bytes with different L are not equal sizes
        gpudiff_pair_row r = zero_row();
        r.off_b = 1024;
        r.spec_l_a = 2, r.spec_ar_a = 16;
        r.spec_l_b = 1, r.spec_ar_b = 32;
        r.stat_l_a = r.stat_l_b = 3;
        r.flags_a = r.flags_b = GPUDIFF_OBJ_HAS_STATUS;
        check("spec: equal bytes, different L", r, 0);
        CHECK(from_row(r).n1 == 0 && from_row(r).n2 == 3);
        gpudiff_pair_row q = zero_row();
        q.off_b = 1024;
        q.spec_l_a = q.spec_l_b = 5;
        q.stat_l_a = 4, q.stat_ar_a = 0;
        q.stat_l_b = 1, q.stat_ar_b = 48;
        q.flags_a = q.flags_b = GPUDIFF_OBJ_HAS_STATUS;
        check("status: equal bytes, different L", q, 0);
        CHECK(from_row(q).n1 == 5 && from_row(q).n2 == 0);
        q.stat_l_b = 4, q.stat_ar_b = 0;
        check("status: equal sizes", q, 0);
        CHECK(from_row(q).n2 == 16 - 5);  // to the body's end: 9 x 16 = 144 -> 256 bytes
    }
    for (uint32_t side = 0; side < 2; side++) {  // a decode error, on either side
        gpudiff_pair_row r = zero_row();
        r.off_a = 128, r.off_b = 256;
        r.spec_l_a = r.spec_l_b = 7;
        (side ? r.flags_b : r.flags_a) = GPUDIFF_OBJ_DECODE_ERR;
        check("decode error, side " + std::to_string(side), r, 0);
        CHECK(from_row(r).n1 == 0 && from_row(r).n2 == 0 && from_row(r).err);
    }
    {   // what is no multiple of the units
        gpudiff_pair_row r = zero_row();
        r.off_a = 64;
        check("offset inside a line", r, 1);
        r = zero_row();
        r.spec_ar_b = 8;
        check("arena of 8 bytes", r, 1);
        r = zero_row();
        r.stat_l_a = r.stat_l_b = 0x80000000u;  // their u32 sum is 0
        check("status leaf counts that sum to 0", r, 1);
    }
    for (uint32_t i = 0; i < 1000000u; i++) {
        gpudiff_pair_row r = zero_row();
        r.off_a = rnd_off();
        r.off_b = rnd_off();
        r.spec_l_a = rnd_leaves(), r.spec_ar_a = rnd_arena();
        r.spec_l_b = rnd_leaves(), r.spec_ar_b = rnd_arena();
        r.stat_l_a = rnd_leaves(), r.stat_ar_a = rnd_arena();
        r.stat_l_b = rnd_leaves(), r.stat_ar_b = rnd_arena();
        // sizes equal on both sides, and whole regions empty, as often as not
        if (rnd() & 1u) r.spec_l_b = r.spec_l_a;
        if (rnd() & 1u) r.spec_ar_b = r.spec_ar_a;
        if (rnd() & 1u) r.stat_l_b = r.stat_l_a;
        if (rnd() & 1u) r.stat_ar_b = r.stat_ar_a;
        if (rnd() % 4 == 0) r.stat_l_a = r.stat_l_b = r.stat_ar_a = r.stat_ar_b = 0;
        if (rnd() % 4 == 0) {  // a row as the encoder makes them: aligned, small, arenas in 16-B units
            r.off_a &= ~127ull, r.off_b &= ~127ull;
            r.off_a %= 1ull << 38, r.off_b %= 1ull << 38;
            r.spec_l_a %= 500u, r.spec_l_b %= 500u, r.stat_l_a %= 100u, r.stat_l_b %= 100u;
            r.spec_ar_a = (r.spec_ar_a % 4096u) & ~15u, r.spec_ar_b = (r.spec_ar_b % 4096u) & ~15u;
            r.stat_ar_a = r.stat_l_a ? (r.stat_ar_a % 1024u) & ~15u : 0u;
            r.stat_ar_b = r.stat_l_b ? (r.stat_ar_b % 1024u) & ~15u : 0u;
        }
        const uint64_t f = rnd();
        r.flags_a = ((f & 1u) ? GPUDIFF_OBJ_HAS_STATUS : 0u) | ((f & 0x70u) == 0u ? GPUDIFF_OBJ_DECODE_ERR : 0u) |
                    ((f & 0x100u) ? (uint32_t)((f >> 16) & 0xFFu) << GPUDIFF_OBJ_SEED_SHIFT : 0u) | ((f & 0x200u) ? GPUDIFF_OBJ_FRESH : 0u);
        r.flags_b = ((f & 2u) ? GPUDIFF_OBJ_HAS_STATUS : 0u) | ((f & 0x7000u) == 0u ? GPUDIFF_OBJ_DECODE_ERR : 0u);
        r.pair_id = (uint32_t)rnd();
        r.cluster_id = (uint32_t)rnd();
        check("random row " + std::to_string(i), r, -1);
    }
    // the random rows must have exercised both outcomes in numbers
    CHECK(n_packed > 100000 && n_escaped > 100000);
    std::printf("ok\n");
    return 0;
}
'''


def test_pair_desc_rule():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/bin/hipcc"
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        exe = os.path.join(d, "t")
        with open(src, "w") as f:
            f.write(SRC)
        subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), src, "-o", exe],
                       check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
        assert r.stdout.strip() == "ok"
