"""include/gpudiff_format.h, kcp_amd/csrc/stream_paths.h: the compare image.  A row with no decode error, equal spec
sizes and both GPUDIFF_OBJ_SPEC_KEYS_EQ and GPUDIFF_OBJ_SPEC_SHAPE_EQ is streamed by K2 from a compacted copy --
per side  spec vals[L] padded to 16 | spec arena | status (vals[Lt] padded to 16 | arena under
GPUDIFF_OBJ_STAT_SHAPE_EQ, the whole segment otherwise) | zeros to 128  -- through the descriptor of a fictitious
row whose blobs are the image sides, marked by the skip L field all ones.  Checked here, on directed rows and 10^6
random ones: the image part sizes against a formula restated below; unpack(image pack) against gpudiff_pair_geom_of
of the fictitious row; that the mark collides with no output of gpudiff_pair_desc_pack (the skip L field alone does,
in two corners, which is why the mark also bounds A's field) and not with the escape; that the image -> segment chunk
mapping is the inverse of the compaction, by building both from bytes; and that the byte sum is the per-pair sum.
Plain arithmetic, so it is a stand-alone program built with the address and undefined-behaviour sanitizers; no GPU,
nothing loaded into Python."""
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
#include <vector>

static std::string g_case;
#define CHECK(x) do { if (!(x)) { std::printf("%s:%d: %s failed (case %s)\n", __FILE__, __LINE__, #x, g_case.c_str()); std::exit(1); } } while (0)

// the flags_b bits and the descriptor's fields, written out
static const uint32_t kHasStatus = 0x1u, kErr = 0x2u, kKeys = 0x8u, kShape = 0x10u, kStatShape = 0x20u;
static const uint32_t kFieldMax = 0x7FFFFu, kImageBit = 0x80u;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    g_rng ^= g_rng >> 12;
    g_rng ^= g_rng << 25;
    g_rng ^= g_rng >> 27;
    return g_rng * 0x2545F4914F6CDD1Dull;
}

static gpudiff_pair_row zero_row() {
    gpudiff_pair_row r;
    std::memset(&r, 0, sizeof(r));
    return r;
}
static std::string show(const gpudiff_pair_row& r) {
    char b[256];
    std::snprintf(b, sizeof(b), "off %llx %llx spec %u %u / %u %u stat %u %u / %u %u flags %x %x",
                  (unsigned long long)r.off_a, (unsigned long long)r.off_b, r.spec_l_a, r.spec_l_b, r.spec_ar_a,
                  r.spec_ar_b, r.stat_l_a, r.stat_l_b, r.stat_ar_a, r.stat_ar_b, r.flags_a, r.flags_b);
    return b;
}

// ---- the image's parts, restated: which rows are imaged and how many bytes each part takes
static bool escapes(const gpudiff_pair_row& r) {
    const uint64_t sa = 16ull * r.spec_l_a + r.spec_ar_a, sb = 16ull * r.spec_l_b + r.spec_ar_b;
    const uint64_t st = 16ull * r.stat_l_a + r.stat_ar_a, seg_max = (uint64_t)kFieldMax << 4;
    if ((r.off_a & 127u) || (r.off_b & 127u) || (r.off_a >> 7) > 0xFFFFFFFFull || (r.off_b >> 7) > 0xFFFFFFFFull) return true;
    if (((sa | sb | st) & 15u) || sa > seg_max || sb > seg_max || st > seg_max) return true;
    const bool no_stat = (r.stat_l_a | r.stat_l_b | r.stat_ar_a | r.stat_ar_b) == 0u;
    return ((uint32_t)(r.stat_l_a + r.stat_l_b) == 0u) != no_stat;
}
static bool want_parts(const gpudiff_pair_row& r, uint64_t* s, uint64_t* t) {
    *s = *t = 0;
    if ((r.flags_a | r.flags_b) & kErr) return false;
    if (r.spec_l_a != r.spec_l_b || r.spec_ar_a != r.spec_ar_b) return false;
    if (!(r.flags_b & kKeys) || !(r.flags_b & kShape)) return false;
    if (escapes(r)) return false;
    const uint64_t spec = 16ull * ((r.spec_l_a + 1ull) / 2) + r.spec_ar_a;  // vals[L] padded to 16 | arena
    if (spec / 16 >= 0x3FFFFull) return false;                            // the mark's bound on A's field
    *s = spec;
    if ((r.flags_b & kHasStatus) && r.stat_l_a == r.stat_l_b && r.stat_ar_a == r.stat_ar_b)
        *t = (r.flags_b & kStatShape) ? 16ull * ((r.stat_l_a + 1ull) / 2) + r.stat_ar_a : 16ull * r.stat_l_a + r.stat_ar_a;
    return true;
}

static void same_geom(const gpudiff_pair_geom& a, const gpudiff_pair_geom& b) {
    CHECK(a.off_a == b.off_a && a.off_b == b.off_b && a.n1 == b.n1 && a.n2 == b.n2 && a.adj_a == b.adj_a &&
          a.adj_b == b.adj_b && a.bits == b.bits && a.hs == b.hs && a.hl == b.hl);
}

static uint64_t g_imaged = 0, g_sum = 0;

static void check_row(const gpudiff_pair_row& r) {
    g_case = show(r);
    uint64_t ws, wt;
    const bool want = want_parts(r, &ws, &wt);
    uint32_t s = 77, t = 77;
    const int got = gpudiff_pair_image_parts(&r, &s, &t);
    CHECK((got != 0) == want && s == ws && t == wt);
    const uint64_t side = (ws + wt + 127) / 128 * 128;
    CHECK(gpudiff_pair_image_side(&r) == (want ? side : 0u));
    // the ordinary packer is what it was whatever the new bit says, and never carries the mark
    const gpudiff_pair_desc od = gpudiff_pair_desc_pack(&r);
    {
        gpudiff_pair_row q = r;
        q.flags_b ^= kStatShape;
        const gpudiff_pair_desc qd = gpudiff_pair_desc_pack(&q);
        CHECK(std::memcmp(&od, &qd, sizeof(od)) == 0);
    }
    if (!gpudiff_pair_desc_is_escape(od.w[3])) {
        const gpudiff_pair_geom og = gpudiff_pair_desc_unpack(od.w[0], od.w[1], od.w[2], od.w[3]);
        CHECK(!(og.bits & kImageBit));
        CHECK(og.bits == gpudiff_pair_row_bits(&r));
    }
    const uint64_t ia = (rnd() & 0xFFFFFFFFull) << 7, ib = ia + side;
    const gpudiff_pair_desc d = gpudiff_pair_desc_pack_image(&r, ia, ib);
    if (!want || (ib >> 7) > 0xFFFFFFFFull) {
        CHECK(d.w[0] == 0xFFFFFFFFu && d.w[1] == 0xFFFFFFFFu && d.w[2] == 0xFFFFFFFFu && d.w[3] == 0xFFFFFFFFu);
        CHECK(gpudiff_pair_image_bytes(&r) == gpudiff_pair_stream_bytes(&r) || want);
        g_sum += gpudiff_pair_image_bytes(&r);
        return;
    }
    g_imaged++;
    CHECK(!gpudiff_pair_desc_is_escape(d.w[3]));
    CHECK(std::memcmp(&d, &od, sizeof(d)) != 0);
    // a misaligned image offset is refused
    {
        const gpudiff_pair_desc bad = gpudiff_pair_desc_pack_image(&r, ia + 16, ib);
        CHECK(gpudiff_pair_desc_is_escape(bad.w[3]));
    }
    // unpack(image pack) == the geometry of the fictitious row: blobs at the image sides, spec segment s (no leaves to
    // skip), status segment t, the real row's seven bits -- plus the mark
    const uint32_t bits = gpudiff_pair_row_bits(&r);
    gpudiff_pair_geom want_g = gpudiff_pair_geom_of(ia, ib, (uint32_t)ws, (uint32_t)ws, (uint32_t)wt, bits, 0u, 0);
    want_g.bits |= kImageBit;
    const gpudiff_pair_geom g = gpudiff_pair_desc_unpack(d.w[0], d.w[1], d.w[2], d.w[3]);
    same_geom(g, want_g);
    CHECK(g.hl == 0);
    if (g.n2) CHECK(g.adj_a == 0 && g.adj_b == 0);  // one contiguous run per side: status chunks follow the spec part
    // the chunks it streams lie inside the side, and are all of it exactly where the pool's stream pads its span
    CHECK(16ull * (g.n1 + (uint64_t)g.n2) <= side);
    const bool stat_sz = wt != 0 || ((r.flags_b & kHasStatus) && r.stat_l_a == r.stat_l_b && r.stat_ar_a == r.stat_ar_b);
    const bool no_stat = (r.stat_l_a | r.stat_l_b | r.stat_ar_a | r.stat_ar_b) == 0u;
    if (stat_sz || no_stat) CHECK(16ull * (g.n1 + (uint64_t)g.n2) == side);
    else CHECK(16ull * g.n1 == ws && g.n2 == 0);
    // never more than the pool's stream
    const uint64_t ibytes = gpudiff_pair_image_bytes(&r);
    CHECK(ibytes == 16u + 32ull * (g.n1 + (uint64_t)g.n2));
    CHECK(ibytes <= gpudiff_pair_stream_bytes(&r));
    g_sum += ibytes;
}

// ---- the mark against every word the ordinary packer can write: over all (A's field, L) the packer's skip L field is
// all ones in two corners only, and there A's field is at or above the mark's bound
static void check_mark() {
    g_case = "mark";
    uint64_t corners = 0;
    const uint32_t ls[] = {0x3FFFEu, 0x3FFFFu, 0x40000u, 0x7FFFEu, 0x7FFFFu};
    for (uint32_t L : ls)
        for (uint32_t extra = 0; extra < 3; extra++)
            for (uint32_t fl = 0; fl < 4; fl++) {
                gpudiff_pair_row r = zero_row();
                r.spec_l_a = r.spec_l_b = L;
                r.spec_ar_a = r.spec_ar_b = 16u * extra;
                r.flags_b = (fl & 1u ? kKeys : 0u) | (fl & 2u ? kShape : 0u);
                const gpudiff_pair_desc d = gpudiff_pair_desc_pack(&r);
                if (gpudiff_pair_desc_is_escape(d.w[3])) continue;
                const uint64_t zw = ((uint64_t)d.w[3] << 32) | d.w[2];
                const uint32_t fa = (uint32_t)zw & kFieldMax, f1 = (uint32_t)(zw >> 19) & kFieldMax;
                if (f1 == kFieldMax) {
                    corners++;
                    CHECK(fa >= GPUDIFF_PD_IMAGE_SPEC_MAX);
                    CHECK((fa == 0x7FFFFu && L == 0x7FFFFu) || (fa == 0x3FFFFu && L == 0x3FFFFu));
                }
                const gpudiff_pair_geom g = gpudiff_pair_desc_unpack(d.w[0], d.w[1], d.w[2], d.w[3]);
                CHECK(!(g.bits & kImageBit));
            }
    CHECK(corners >= 2);  // so the skip L field alone would not do
}

// ---- the chunk mapping against the compaction done on bytes
static void check_mapping(uint32_t L, uint32_t arena_chunks) {
    g_case = "mapping L = " + std::to_string(L) + " arena chunks " + std::to_string(arena_chunks);
    const uint32_t segc = L + arena_chunks;  // the segment's 16-B chunks
    std::vector<uint8_t> seg(16ull * segc + 16);
    for (size_t i = 0; i < seg.size(); i++) seg[i] = (uint8_t)(rnd() | 1u);  // no zero byte: zeros are padding
    seg.resize(16ull * segc);
    // the compaction: vals[L], zero padded to 16, then the arena
    const uint32_t nv = (L + 1) / 2;
    std::vector<uint8_t> img(16ull * (nv + arena_chunks), 0);
    if (L) std::memcpy(img.data(), seg.data(), 8ull * L);
    if (arena_chunks) std::memcpy(img.data() + 16ull * nv, seg.data() + 16ull * L, 16ull * arena_chunks);
    CHECK(gd::sp_image_vals(L) == nv);
    // every image chunk: its non-padding bytes are the mapped segment chunk's, dword for dword
    for (uint32_t k = 0; k < nv + arena_chunks; k++) {
        const uint32_t c = gd::sp_image_chunk(k, L);
        CHECK(c < segc);
        CHECK(gd::sp_image_of_chunk(c, L) == k);  // the inverse
        for (uint32_t d = 0; d < 4; d++) {
            const uint8_t* ib = img.data() + 16ull * k + 4 * d;
            const bool pad = (L & 1u) && k == nv - 1 && d >= 2;
            if (pad) CHECK(ib[0] == 0 && ib[1] == 0 && ib[2] == 0 && ib[3] == 0);
            else CHECK(std::memcmp(ib, seg.data() + 16ull * c + 4 * d, 4) == 0);
            // a dword the image holds is a value or an arena dword of the segment, never a key or a meta
            if (!pad) {
                const gd::SpWhere w = gd::sp_classify(16ull * c + 4 * d, L);
                CHECK(w.cls == gd::SP_VAL || w.cls == gd::SP_ARENA);
                CHECK((w.cls == gd::SP_VAL) == (k < nv));
            }
        }
        // the log entry's form of the same
        for (uint32_t dw = 1; dw < 16; dw++) {
            const uint32_t e = gd::sp_entry_unimage(gd::sp_entry(k, dw), L);
            CHECK((e >> 4) == c && gd::sp_entry_dwords(e) == dw);
        }
    }
    // every segment chunk: kept iff it holds a value or arena byte
    uint32_t kept = 0;
    for (uint32_t c = 0; c < segc; c++) {
        const uint32_t k = gd::sp_image_of_chunk(c, L);
        const bool holds = 16ull * c < 8ull * L || c >= L;
        CHECK((k != gd::kSpRefuse) == holds);
        if (holds) {
            kept++;
            CHECK(gd::sp_image_chunk(k, L) == c);
        }
    }
    CHECK(kept == nv + arena_chunks);
    // a chunk past the part's end (the line padding) lands at or past the segment's end
    for (uint32_t k = nv + arena_chunks; k < nv + arena_chunks + 8; k++) CHECK(gd::sp_image_chunk(k, L) >= segc);
}

int main() {
    check_mark();
    // the marker's hole word: the stream steps over nothing below 2^19 - 8 spec chunks, and an image pair has fewer
    // than GPUDIFF_PD_IMAGE_SPEC_MAX + 8 (its spec part, padded to the line)
    CHECK(gd::sp_hole_start(gd::kSpHoleImage) > GPUDIFF_PD_IMAGE_SPEC_MAX + 8u);
    for (uint32_t L = 0; L < 0x40000u; L += (L < 4096 ? 1 : 4093)) {
        uint32_t hs, hl;
        gpudiff_shape_hole(L, &hs, &hl);
        CHECK(gd::sp_hole_word(hs, hl) != gd::kSpHoleImage);
        gpudiff_keys_hole(L, &hs, &hl);
        CHECK(gd::sp_hole_word(hs, hl) != gd::kSpHoleImage);
    }
    const uint32_t dl[] = {0, 1, 2, 3, 4, 15, 16, 17, 31, 32, 33, 63, 64, 65, 184, 185, 1000, 1001};
    for (uint32_t L : dl)
        for (uint32_t ar = 0; ar < 10; ar++) check_mapping(L, ar);
    // directed rows: L, Lt in {0, 1, 2, ...}, every flag combination, the status forms
    const uint32_t ls[] = {0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 184, 0x3FFFEu, 0x3FFFFu, 0x40000u, 0x7FFFEu, 0x7FFFFu};
    const uint32_t lts[] = {0, 1, 2, 17, 18};
    for (uint32_t L : ls)
        for (uint32_t ar : {0u, 16u, 48u, 112u})
            for (uint32_t Lt : lts)
                for (uint32_t tar : {0u, 16u, 96u})
                    for (uint32_t fb = 0; fb < 64; fb++)
                        for (uint32_t form = 0; form < 4; form++) {
                            gpudiff_pair_row r = zero_row();
                            r.off_a = 128ull * (rnd() % 1000);
                            r.off_b = r.off_a + 128ull * (1 + rnd() % 1000);
                            r.spec_l_a = r.spec_l_b = L;
                            r.spec_ar_a = r.spec_ar_b = ar;
                            r.stat_l_a = r.stat_l_b = Lt;
                            r.stat_ar_a = r.stat_ar_b = tar;
                            if (form == 1) r.stat_l_b += 1;
                            if (form == 2) r.stat_ar_b += 16;
                            if (form == 3) r.spec_ar_b += 16;
                            r.flags_b = fb;
                            r.flags_a = (fb & 4u) ? kHasStatus : 0u;
                            check_row(r);
                        }
    // random rows
    for (uint32_t i = 0; i < 1000000u; i++) {
        gpudiff_pair_row r = zero_row();
        const uint64_t x = rnd();
        const uint32_t big = (x & 63u) == 0u;
        r.off_a = ((rnd() & 0xFFFFFFFFull) << 7) | ((x >> 6 & 255u) == 0u ? 16u : 0u);
        r.off_b = (rnd() & 0xFFFFFFFFull) << 7;
        r.spec_l_a = (uint32_t)(rnd() % (big ? 0x80010u : 300u));
        r.spec_l_b = (x >> 14 & 7u) ? r.spec_l_a : (uint32_t)(rnd() % 300u);
        r.spec_ar_a = 16u * (uint32_t)(rnd() % (big ? 0x1000u : 64u));
        r.spec_ar_b = (x >> 17 & 7u) ? r.spec_ar_a : 16u * (uint32_t)(rnd() % 64u);
        r.stat_l_a = (x >> 20 & 3u) ? (uint32_t)(rnd() % 40u) : 0u;
        r.stat_l_b = (x >> 22 & 7u) ? r.stat_l_a : (uint32_t)(rnd() % 40u);
        r.stat_ar_a = (x >> 25 & 1u) ? 16u * (uint32_t)(rnd() % 16u) : 0u;
        r.stat_ar_b = (x >> 26 & 7u) ? r.stat_ar_a : 16u * (uint32_t)(rnd() % 16u);
        r.flags_a = (uint32_t)(x >> 29 & 1u) | ((x >> 30 & 15u) == 0u ? kErr : 0u) | ((uint32_t)(x >> 34 & 1u) << 8);
        r.flags_b = (uint32_t)(x >> 35 & 1u) | ((x >> 36 & 7u) ? kKeys | kShape : (uint32_t)(x >> 39 & 3u) << 3) |
                    ((x >> 41 & 1u) ? kStatShape : 0u);
        check_row(r);
    }
    CHECK(g_imaged > 300000u);
    std::printf("imaged %llu rows\n", (unsigned long long)g_imaged);
    // the byte sum is the per-pair sum (restated over a small batch)
    {
        std::vector<gpudiff_pair_row> rows;
        uint64_t sum = 0;
        for (uint32_t i = 0; i < 1000; i++) {
            gpudiff_pair_row r = zero_row();
            r.off_a = 128ull * i * 64;
            r.off_b = r.off_a + 128ull * 32;
            r.spec_l_a = r.spec_l_b = (uint32_t)(rnd() % 200u);
            r.spec_ar_a = r.spec_ar_b = 16u * (uint32_t)(rnd() % 32u);
            r.stat_l_a = r.stat_l_b = (uint32_t)(rnd() % 20u);
            r.flags_a = r.flags_b = kHasStatus;
            r.flags_b |= (i % 3 ? kKeys | kShape : 0u) | (i % 5 && r.stat_l_a ? kStatShape : 0u);
            rows.push_back(r);
            uint64_t s, t;
            if (want_parts(r, &s, &t)) sum += 16u + 2u * ((s + t + 127) / 128 * 128);
            else sum += gpudiff_pair_stream_bytes(&r);
        }
        uint64_t got = 0;
        for (const gpudiff_pair_row& r : rows) got += gpudiff_pair_image_bytes(&r);
        g_case = "byte sum";
        CHECK(got == sum);
    }
    std::printf("ok\n");
    return 0;
}
'''


def test_image_rule():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or "/opt/rocm/bin/hipcc"
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


def test_rows_image_read_bytes_is_the_sum():
    """gpudiff_rows_image_read_bytes (the library's export) over encoded rows: never above gpudiff_rows_read_bytes,
    equal to it once the shape bits are masked, and additive over a split of the rows."""
    import numpy as np
    from kcp_amd import gpudiff as G
    from tests.workload import make_pairs
    e = G.Engine(device=G.DEVICE_NONE)
    hb = e.encode(make_pairs(300, seed=5, mutate_frac=0.5)[0])
    rows = hb.rows().copy()
    hb.free()
    e.close()
    total = G.image_read_bytes(rows)
    assert total == G.image_read_bytes(rows[:117]) + G.image_read_bytes(rows[117:])
    assert total <= G.read_bytes(rows)
    plain = rows.copy()
    plain["flags_b"] &= ~np.uint32(G.OBJ_SPEC_SHAPE_EQ)
    assert G.image_read_bytes(plain) == G.read_bytes(plain)
    assert ((rows["flags_b"] & G.OBJ_SPEC_SHAPE_EQ) != 0).any() and total < G.read_bytes(rows)
