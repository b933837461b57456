"""include/gpudiff_format.h, kcp_amd/csrc/stream_paths.h: the packed region of the compare image.  A region whose keys
and metas the image drops is written as its leaves' value bytes alone -- a string's length padded to 4 (head from vals,
the rest its arena tail), a number's 8 bytes, nothing for null, false, true, {} and [] -- then zeros to 16.  Checked
here: gpudiff_meta_packed and K2's restatement sp_pk against the definition for every tag and every string length
0..20, and the region's size; gpudiff_region_pack against a packing done value byte by value byte, for leaf counts
around the builder's rounds of 64; the owner of every dword of a packed region against brute force; and on 10^5 random
shape-equal region pairs with random value edits, that whenever neither log overflows the packed rule names exactly the
leaves stream_paths.h's rule names on the segments.  A stand-alone program built with the address and
undefined-behaviour sanitizers; no GPU, nothing loaded into Python.  The library's host byte sum is then checked
against the formula restated in numpy."""
import os
import shutil
import subprocess
import tempfile

import numpy as np

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

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    g_rng ^= g_rng >> 12;
    g_rng ^= g_rng << 25;
    g_rng ^= g_rng >> 27;
    return g_rng * 0x2545F4914F6CDD1Dull;
}

// the definition, written out: bytes of a leaf's value in a packed region
static uint32_t want_pk(uint32_t tag, uint32_t len) {
    switch (tag) {
        case 5: return (len + 3) / 4 * 4;   // string
        case 3: case 4: return 8;           // int64, float64
        default: return 0;                  // null, false, true, {}, []
    }
}

// a leaf's value: tag and, for the tags that have any, its bytes
struct Leaf {
    uint32_t tag;
    std::vector<uint8_t> v;
};
static Leaf random_leaf(uint32_t max_len) {
    Leaf l;
    const uint32_t pick = (uint32_t)(rnd() % 16);  // half strings, a quarter numbers, a quarter tag-only leaves
    l.tag = pick < 8 ? 5u : pick < 10 ? 3u : pick < 12 ? 4u : pick == 12 ? 0u : pick == 13 ? 1u : pick == 14 ? 6u : 7u;
    if (pick == 15 && (rnd() & 1u)) l.tag = 2u;
    uint32_t len = 0;
    if (l.tag == 5) len = (uint32_t)(rnd() % (max_len + 1));
    if (l.tag == 3 || l.tag == 4) len = 8;
    for (uint32_t i = 0; i < len; i++) l.v.push_back((uint8_t)(1 + rnd() % 255));
    return l;
}
// the segment of the leaves by the format: vals | keys | metas | arena (tails 4-padded, the whole 16-padded)
static std::vector<uint8_t> segment(const std::vector<Leaf>& ls) {
    const uint32_t L = (uint32_t)ls.size();
    std::vector<uint8_t> tails;
    std::vector<uint8_t> s(16ull * L, 0);
    for (uint32_t i = 0; i < L; i++) {
        const uint32_t len = (uint32_t)ls[i].v.size();
        for (uint32_t k = 0; k < len && k < 8; k++) s[8ull * i + k] = ls[i].v[k];
        const uint32_t key = 16u * i + 5u;  // ascending, unique
        const uint32_t meta = (len << 3) | ls[i].tag;
        std::memcpy(&s[8ull * L + 4ull * i], &key, 4);
        std::memcpy(&s[12ull * L + 4ull * i], &meta, 4);
        for (uint32_t k = 8; k < len; k++) tails.push_back(ls[i].v[k]);
        while (tails.size() & 3u) tails.push_back(0);
    }
    while (tails.size() & 15u) tails.push_back(0);
    s.insert(s.end(), tails.begin(), tails.end());
    return s;
}
// the packing, value byte by value byte, and the owner of each of its dwords (L: the final padding)
static std::vector<uint8_t> pack_bytes(const std::vector<Leaf>& ls, std::vector<uint32_t>* owner) {
    std::vector<uint8_t> p;
    owner->clear();
    for (uint32_t i = 0; i < ls.size(); i++) {
        if (ls[i].tag != 3 && ls[i].tag != 4 && ls[i].tag != 5) continue;
        for (uint8_t b : ls[i].v) p.push_back(b);
        while (p.size() & 3u) p.push_back(0);
        while (owner->size() < p.size() / 4) owner->push_back(i);
    }
    while (p.size() & 15u) p.push_back(0);
    while (owner->size() < p.size() / 4) owner->push_back((uint32_t)ls.size());
    return p;
}
static const uint32_t* metas_of(const std::vector<uint8_t>& seg, uint32_t L) {
    return (const uint32_t*)(seg.data() + 12ull * L);
}
// the mismatching 16-B chunks of two equally long spans as K2 logs them: the first kSpLogCap entries, and the count
static uint32_t log_of(const std::vector<uint8_t>& a, const std::vector<uint8_t>& b, uint32_t ent[gd::kSpLogCap]) {
    uint32_t n = 0;
    for (size_t c = 0; c < a.size() / 16; c++) {
        uint32_t dw = 0;
        for (uint32_t d = 0; d < 4; d++)
            if (std::memcmp(&a[16 * c + 4 * d], &b[16 * c + 4 * d], 4)) dw |= 1u << d;
        if (!dw) continue;
        if (n < gd::kSpLogCap) ent[n] = gd::sp_entry((uint32_t)c, dw);
        n++;
    }
    return n;
}

int main() {
    // 1. pk for every tag and every string length 0..20 (and two long ones), three ways; the region's size
    for (uint32_t tag = 0; tag < 8; tag++)
        for (uint32_t len : {0u, 1u, 2u, 3u, 4u, 5u, 6u, 7u, 8u, 9u, 10u, 11u, 12u, 13u, 14u, 15u, 16u, 17u, 18u, 19u, 20u, 4095u, (1u << 29) - 1u}) {
            g_case = "pk tag " + std::to_string(tag) + " len " + std::to_string(len);
            const uint32_t m = gpudiff_meta(tag, len);
            CHECK(gpudiff_meta_packed(m) == want_pk(tag, len));
            CHECK(gd::sp_pk(m) == want_pk(tag, len));
            CHECK(gd::sp_meta_arena(m) == gpudiff_meta_arena(m));
            // a leaf never takes more than its 8 bytes of vals and its tail
            CHECK(gpudiff_meta_packed(m) <= 8u + gpudiff_meta_arena(m));
            if (tag == 5 && len > 8) CHECK(gpudiff_meta_packed(m) == 8u + gpudiff_meta_arena(m));
        }
    for (uint32_t sum = 0; sum < 100; sum++) CHECK(gpudiff_packed_bytes(sum) == (sum + 15) / 16 * 16);

    // 2., 3. the packed bytes and every dword's owner, around the builder's rounds of 64 leaves
    for (uint32_t L : {0u, 1u, 2u, 3u, 33u, 64u, 65u, 130u})
        for (uint32_t rep = 0; rep < 200; rep++) {
            g_case = "pack L " + std::to_string(L) + " rep " + std::to_string(rep);
            std::vector<Leaf> ls;
            for (uint32_t i = 0; i < L; i++) ls.push_back(random_leaf(rep % 3 == 0 ? 8 : 40));
            if (rep == 1) for (Leaf& l : ls) l = Leaf{(uint32_t)(rnd() % 3), {}};  // tag-only leaves alone
            const std::vector<uint8_t> seg = segment(ls);
            std::vector<uint32_t> owner;
            const std::vector<uint8_t> want = pack_bytes(ls, &owner);
            const uint32_t* ms = metas_of(seg, L);
            CHECK(gpudiff_region_packed_bytes(ms, L) == want.size());
            CHECK(want.size() <= 16ull * ((L + 1) / 2) + (seg.size() - 16ull * L));  // fits the slot's part
            std::vector<uint8_t> got(want.size() + 1, 0xEE);
            CHECK(gpudiff_region_pack(seg.data(), ms, L, got.data()) == want.size());
            CHECK(got[want.size()] == 0xEE);
            CHECK(want.empty() || std::memcmp(got.data(), want.data(), want.size()) == 0);
            for (uint32_t w = 0; w < owner.size(); w++) CHECK(gd::sp_packed_owner(ms, L, 4 * w) == owner[w]);
            CHECK(gd::sp_packed_owner(ms, L, (uint32_t)want.size()) == L);
            CHECK(gd::sp_packed_owner(ms, L, (uint32_t)want.size() + 4096u) == L);
        }

    // 4. random shape-equal region pairs, random value edits: the packed rule against the segments' rule
    uint64_t both = 0, over = 0, clean = 0;
    for (uint32_t it = 0; it < 160000; it++) {
        g_case = "rule " + std::to_string(it);
        const uint32_t L = 1 + (uint32_t)(rnd() % (it % 7 == 0 ? 130 : 12));
        std::vector<Leaf> a;
        for (uint32_t i = 0; i < L; i++) a.push_back(random_leaf(it % 2 ? 40 : 13));
        std::vector<Leaf> b = a;
        const uint32_t edits = (uint32_t)(rnd() % 8);
        for (uint32_t e = 0; e < edits; e++) {
            uint32_t at_leaf = (uint32_t)(rnd() % L);
            for (uint32_t tries = 0; tries < 4 && b[at_leaf].v.empty(); tries++) at_leaf = (uint32_t)(rnd() % L);
            Leaf& l = b[at_leaf];
            if (l.v.empty()) continue;  // a tag-only leaf or an empty string: no value byte to change
            const uint32_t at = rnd() % 3 == 0 ? (uint32_t)l.v.size() - 1 : (uint32_t)(rnd() % l.v.size());
            l.v[at] = (uint8_t)(1 + (l.v[at] + rnd() % 254) % 255);  // another non-zero byte
        }
        const std::vector<uint8_t> sa = segment(a), sb = segment(b);
        CHECK(sa.size() == sb.size());
        const uint32_t *ma = metas_of(sa, L), *mb = metas_of(sb, L);
        CHECK(std::memcmp(ma, mb, 4ull * L) == 0);
        std::vector<uint8_t> pa(gpudiff_region_packed_bytes(ma, L)), pb(pa.size());
        gpudiff_region_pack(sa.data(), ma, L, pa.data());
        gpudiff_region_pack(sb.data(), ma, L, pb.data());  // (A's metas for both sides, as the builder does)
        CHECK((pa == pb) == (sa == sb));  // equal packed regions iff equal values
        uint32_t es[gd::kSpLogCap], ep[gd::kSpLogCap];
        const uint32_t ns = log_of(sa, sb, es), np = log_of(pa, pb, ep);
        CHECK((ns == 0) == (np == 0));
        if (!ns) { clean++; continue; }
        if (ns > gd::kSpLogCap || np > gd::kSpLogCap) { over++; continue; }
        uint32_t ls[gd::kSpMaxLeaves], lp[gd::kSpMaxLeaves];
        const uint32_t ks = gd::sp_region_rule(sa.data(), sb.data(), L, sa.size(), es, ns, ls);
        const uint32_t kp = gd::sp_packed_rule(ma, mb, L, ep, np, lp);
        CHECK(ks != gd::kSpRefuse && kp == ks);
        CHECK(std::memcmp(ls, lp, 4ull * ks) == 0);
        for (uint32_t k = 0; k < ks; k++) CHECK(a[ls[k]].v != b[ls[k]].v);
        both++;
    }
    std::printf("rule: %llu pairs compared, %llu overflowed a log, %llu clean\n", (unsigned long long)both,
                (unsigned long long)over, (unsigned long long)clean);
    g_case = "counts";
    CHECK(both + over + clean == 160000 && both >= 100000 && over >= 1000 && clean >= 1000);
    std::printf("ok\n");
    return 0;
}
'''


def test_packed_rule():
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


def pk_of(metas):
    """gpudiff_meta_packed over an array of metas, restated."""
    tag, ln = metas & 7, (metas >> 3).astype(np.int64)
    return np.where(tag == 5, (ln + 3) // 4 * 4, np.where((tag == 3) | (tag == 4), 8, 0))


def streamed_bytes_of(rows, pool):
    """What K2 streams of the imaged pairs among the rows, restated: the descriptor and, per side, the packed spec part,
    then the packed (GPUDIFF_OBJ_STAT_SHAPE_EQ) or whole status part -- to the line when the status sizes match or no
    side has a status leaf, as K2 pads every stream."""
    from kcp_amd import gpudiff as G
    total = n = 0
    both = G.OBJ_SPEC_KEYS_EQ | G.OBJ_SPEC_SHAPE_EQ
    for r in rows:
        fa, fb = int(r["flags_a"]), int(r["flags_b"])
        L, ar, Lt, tar = int(r["spec_l_a"]), int(r["spec_ar_a"]), int(r["stat_l_a"]), int(r["stat_ar_a"])
        if (fa | fb) & G.OBJ_DECODE_ERR or L != r["spec_l_b"] or ar != r["spec_ar_b"] or fb & both != both:
            continue
        oa = int(r["off_a"])
        sp = (int(pk_of(pool[oa + 12 * L:oa + 16 * L].view("<u4")).sum()) + 15) // 16 * 16
        stat_sz = bool(fb & G.OBJ_HAS_STATUS) and Lt == r["stat_l_b"] and tar == r["stat_ar_b"]
        tp = 0
        if stat_sz:
            seg = oa + 16 * L + ar
            tp = 16 * Lt + tar
            if fb & G.OBJ_STAT_SHAPE_EQ:
                tp = (int(pk_of(pool[seg + 12 * Lt:seg + 16 * Lt].view("<u4")).sum()) + 15) // 16 * 16
        no_stat = not (Lt or tar or int(r["stat_l_b"]) or int(r["stat_ar_b"]))
        side = (sp + tp + 127) // 128 * 128 if stat_sz or no_stat else sp
        total += 16 + 2 * side
        n += 1
    return total, n


def test_rows_image_streamed_bytes_is_the_formula():
    """gpudiff_rows_image_streamed_bytes (the library's export) over an encoded batch against the formula restated
    above; additive over a split; never above the slots' bound (gpudiff_rows_image_read_bytes of the imaged rows)."""
    from kcp_amd import gpudiff as G
    from tests.workload import make_pairs
    e = G.Engine(device=G.DEVICE_NONE)
    hb = e.encode(make_pairs(300, seed=5, mutate_frac=0.5)[0])
    rows, pool = hb.rows().copy(), np.array(hb.pool_view(), dtype=np.uint8)
    hb.free()
    e.close()
    want, n = streamed_bytes_of(rows, pool)
    got = G.image_streamed_bytes(rows, pool)
    print("%d of %d rows imaged: %d B streamed packed, %d B by the slots" % (n, rows.size, got, G.image_read_bytes(rows)))
    assert n > 100 and got == want
    assert got == G.image_streamed_bytes(rows[:117], pool) + G.image_streamed_bytes(rows[117:], pool)
    fb = rows["flags_b"]
    both = G.OBJ_SPEC_KEYS_EQ | G.OBJ_SPEC_SHAPE_EQ
    imaged = rows[(fb & both) == both]
    assert got < G.image_read_bytes(imaged)
    plain = rows.copy()
    plain["flags_b"] &= ~np.uint32(G.OBJ_SPEC_SHAPE_EQ)
    assert G.image_streamed_bytes(plain, pool) == 0
