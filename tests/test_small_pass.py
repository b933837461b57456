"""GPUDIFF_OPT_SMALL_PASS without a GPU: the option bit, its constants and gpudiff_pass_stats_get on a host-only
context, and kcp_amd/csrc/small_pass.h -- the result image's layout and the host unpacker -- checked by a stand-alone
host program (its own main, built with AddressSanitizer and UBSan and run directly; nothing is loaded into Python)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_define(name):
    src = open(os.path.join(ROOT, "include", "gpudiff.h")).read()
    return int(re.search(r"#define %s (0x[0-9a-fA-F]+|\d+)u\b" % name, src).group(1), 0)


def test_option_and_constants_equal_the_header():
    from kcp_amd import gpudiff as G
    assert G.OPT_SMALL_PASS == _header_define("GPUDIFF_OPT_SMALL_PASS") == 0x20000000
    assert G.SMALL_PASS_MAX_PAIRS == _header_define("GPUDIFF_SMALL_PASS_MAX_PAIRS")
    assert G.SMALL_PASS_MAX_PATHS == _header_define("GPUDIFF_SMALL_PASS_MAX_PATHS")
    assert G.SMALL_PASS_MAX_PAIRS == 64 * 64  # the finishing block scans 64 chunks with one lane each


def test_host_only_context_takes_the_option_and_has_no_pass_stats():
    from kcp_amd import gpudiff as G
    e = G.Engine(device=G.DEVICE_NONE, flags=G.OPT_SMALL_PASS)
    with pytest.raises(G.GpuDiffError) as ei:
        e.pass_stats()
    assert ei.value.code == G.E_NODEVICE
    e.close()
    e = G.Engine(device=G.DEVICE_NONE, small_pass=True)
    with pytest.raises(G.GpuDiffError) as ei:
        e.submit([(b"{}", b"{}")])
    assert ei.value.code == G.E_NODEVICE
    e.close()


MAIN = r'''
#include "small_pass.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace gd;

struct RS {
    std::vector<uint8_t> flags;
    std::vector<uint32_t> spec, status, dirty, off;
    std::vector<uint64_t> hashes;
    std::vector<uint8_t> kinds;
};

static int bad = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("line %d: %s\n", __LINE__, #c);               \
            bad++;                                                    \
        }                                                             \
    } while (0)

static void check_layout(uint32_t n, uint32_t ns, uint32_t nt, uint32_t nd, uint32_t np) {
    const SmallLayout l = small_layout(n, ns, nt, nd, np);
    // ascending and disjoint: each section ends at or before the next one's start
    CHECK(l.flags == 64);
    CHECK(l.flags + n <= l.spec_ids);
    CHECK(l.spec_ids + 4ull * ns <= l.status_ids);
    CHECK(l.status_ids + 4ull * nt <= l.dirty_ids);
    CHECK(l.dirty_ids + 4ull * nd <= l.dirty_idx);
    CHECK(l.dirty_idx + 4ull * nd <= l.path_off);
    CHECK(l.path_off + 4ull * (nd + 1ull) <= l.noop_d);
    CHECK(l.noop_d + nd <= l.out_k);
    CHECK(l.out_k + np <= l.out_h);
    CHECK(l.out_h + 8ull * np == l.total);
    // aligned to the element size
    CHECK(l.spec_ids % 4 == 0 && l.status_ids % 4 == 0 && l.dirty_ids % 4 == 0 && l.dirty_idx % 4 == 0 &&
          l.path_off % 4 == 0);
    CHECK(l.out_h % 8 == 0);
    // packed: no more than the alignment's padding
    CHECK(l.total <= 64ull + n + 3 + 4ull * ns + 4ull * nt + 8ull * nd + 4ull * (nd + 1ull) + nd + np + 7 + 8ull * np);
    CHECK(l.total <= small_image_capacity());
    if (np <= small_first_round_paths(n)) CHECK(l.total <= small_first_round_bytes(n));
}

// a hand-built image of the given counts; section contents are functions of the index
static std::vector<uint8_t> build(uint32_t n, uint32_t ns, uint32_t nt, uint32_t nd, uint32_t np) {
    const SmallLayout l = small_layout(n, ns, nt, nd, np);
    std::vector<uint8_t> img(l.total, 0xEE);
    uint32_t h[kSmallHeaderWords] = {0};
    h[SH_MAGIC] = kSmallMagic;
    h[SH_FINAL] = 1;
    h[SH_PAIRS] = n;
    h[SH_SPEC] = ns;
    h[SH_STATUS] = nt;
    h[SH_DIRTY] = nd;
    h[SH_PATHS] = np;
    h[SH_BYTES] = (uint32_t)l.total;
    memcpy(img.data(), h, sizeof(h));
    for (uint32_t i = 0; i < n; i++) img[l.flags + i] = (uint8_t)(i % 8);
    auto put32 = [&](uint64_t off, uint32_t i, uint32_t v) { memcpy(img.data() + off + 4ull * i, &v, 4); };
    for (uint32_t i = 0; i < ns; i++) put32(l.spec_ids, i, 1000u + 3u * i);
    for (uint32_t i = 0; i < nt; i++) put32(l.status_ids, i, 2000u + 5u * i);
    for (uint32_t i = 0; i < nd; i++) put32(l.dirty_ids, i, 3000u + 7u * i);
    for (uint32_t i = 0; i < nd; i++) put32(l.dirty_idx, i, (uint32_t)((uint64_t)i * n / (nd ? nd : 1)));
    for (uint32_t i = 0; i <= nd; i++) put32(l.path_off, i, nd ? (uint32_t)((uint64_t)i * np / nd) : np);
    for (uint32_t i = 0; i < nd; i++) img[l.noop_d + i] = (uint8_t)(i % 4);
    for (uint32_t i = 0; i < np; i++) img[l.out_k + i] = (uint8_t)(0x80u | (i % 4));
    for (uint32_t i = 0; i < np; i++) {
        const uint64_t v = 0x0123456789ABCDEFull * (i + 1u);
        memcpy(img.data() + l.out_h + 8ull * i, &v, 8);
    }
    return img;
}

// unpacks exactly len bytes held in a heap block of that size (ASan sees any read past the prefix)
static SmallUnpack unpack_prefix(const std::vector<uint8_t>& img, uint64_t len, RS& rs, std::vector<uint32_t>& idx,
                                 std::vector<uint8_t>& noop, uint64_t* need, uint32_t* reason) {
    uint8_t* p = (uint8_t*)std::malloc(len ? len : 1);
    if (len) memcpy(p, img.data(), len);
    const SmallUnpack u = small_unpack(p, len, small_image_capacity(), rs, idx, noop, need, reason);
    std::free(p);
    return u;
}

static void check_round_trip(uint32_t n, uint32_t ns, uint32_t nt, uint32_t nd, uint32_t np) {
    if (nd == 0 && np != 0) return;  // no such result: paths belong to dirty pairs
    const std::vector<uint8_t> img = build(n, ns, nt, nd, np);
    const SmallLayout l = small_layout(n, ns, nt, nd, np);
    RS rs;
    std::vector<uint32_t> idx;
    std::vector<uint8_t> noop;
    uint64_t need = 0;
    uint32_t reason = 0;
    CHECK(unpack_prefix(img, img.size(), rs, idx, noop, &need, &reason) == SMALL_OK);
    CHECK(need == l.total);
    CHECK(rs.flags.size() == n && rs.spec.size() == ns && rs.status.size() == nt && rs.dirty.size() == nd);
    CHECK(rs.off.size() == nd + 1ull && rs.hashes.size() == np && rs.kinds.size() == np && idx.size() == nd &&
          noop.size() == nd);
    bool same = true;
    for (uint32_t i = 0; i < n; i++) same &= rs.flags[i] == (uint8_t)(i % 8);
    for (uint32_t i = 0; i < ns; i++) same &= rs.spec[i] == 1000u + 3u * i;
    for (uint32_t i = 0; i < nt; i++) same &= rs.status[i] == 2000u + 5u * i;
    for (uint32_t i = 0; i < nd; i++) same &= rs.dirty[i] == 3000u + 7u * i && noop[i] == (uint8_t)(i % 4);
    for (uint32_t i = 0; i < np; i++)
        same &= rs.hashes[i] == 0x0123456789ABCDEFull * (i + 1u) && rs.kinds[i] == (uint8_t)(0x80u | (i % 4));
    CHECK(same);
    CHECK(rs.off[nd] == np);
    // short prefixes ask for more, and for exactly the image's bytes once the header is there
    const uint64_t lens[] = {0, 1, 63, 64, l.total / 2, l.total - 1};
    for (uint64_t len : lens) {
        if (len >= l.total) continue;
        RS r2;
        CHECK(unpack_prefix(img, len, r2, idx, noop, &need, &reason) == SMALL_MORE);
        CHECK(need == (len < 64 ? 64 : l.total));
    }
    // the first round's bytes hold it iff its paths are within the budget
    if (small_first_round_bytes(n) < l.total) CHECK(np > small_first_round_paths(n));
}

static SmallUnpack unpack_with(std::vector<uint8_t> img, uint32_t word, uint32_t value, uint32_t* reason) {
    memcpy(img.data() + 4ull * word, &value, 4);
    RS rs;
    std::vector<uint32_t> idx;
    std::vector<uint8_t> noop;
    uint64_t need = 0;
    return unpack_prefix(img, img.size(), rs, idx, noop, &need, reason);
}

int main() {
    const uint32_t ns_[] = {1, 64, 65, GPUDIFF_SMALL_PASS_MAX_PAIRS};
    for (uint32_t n : ns_) {
        const uint32_t budget = small_first_round_paths(n);
        CHECK(budget == (4 * n < 64 ? 64 : 4 * n) || budget == GPUDIFF_SMALL_PASS_MAX_PATHS);
        const uint32_t nps[] = {0, 1, budget - 1, budget, budget + 1, GPUDIFF_SMALL_PASS_MAX_PATHS};
        const uint32_t nds[] = {0, n};
        for (uint32_t nd : nds)
            for (uint32_t np : nps) {
                if (np > GPUDIFF_SMALL_PASS_MAX_PATHS) continue;
                const uint32_t halves[] = {0, nd};
                for (uint32_t nspec : halves)
                    for (uint32_t nstat : halves) {
                        check_layout(n, nspec, nstat, nd, np);
                        check_round_trip(n, nspec, nstat, nd, np);
                    }
            }
        CHECK(small_first_round_bytes(n) <= small_image_capacity());
    }
    CHECK(small_layout(GPUDIFF_SMALL_PASS_MAX_PAIRS, GPUDIFF_SMALL_PASS_MAX_PAIRS, GPUDIFF_SMALL_PASS_MAX_PAIRS,
                       GPUDIFF_SMALL_PASS_MAX_PAIRS, GPUDIFF_SMALL_PASS_MAX_PATHS).total == small_image_capacity());
    CHECK(small_image_capacity() < (1ull << 32));  // the header's byte count is a u32

    // rejections, from one good image of 65 pairs, 10 dirty, 23 paths
    const std::vector<uint8_t> good = build(65, 7, 5, 10, 23);
    const SmallLayout gl = small_layout(65, 7, 5, 10, 23);
    uint32_t reason = 0;
    CHECK(unpack_with(good, SH_REASON, 0, &reason) == SMALL_OK);
    CHECK(unpack_with(good, SH_MAGIC, kSmallMagic ^ 1u, &reason) == SMALL_BAD);
    CHECK(unpack_with(good, SH_FINAL, 2, &reason) == SMALL_BAD);
    CHECK(unpack_with(good, SH_PAIRS, 0, &reason) == SMALL_BAD);
    CHECK(unpack_with(good, SH_PAIRS, GPUDIFF_SMALL_PASS_MAX_PAIRS + 1, &reason) == SMALL_BAD);
    CHECK(unpack_with(good, SH_SPEC, 66, &reason) == SMALL_BAD);
    CHECK(unpack_with(good, SH_STATUS, 66, &reason) == SMALL_BAD);
    CHECK(unpack_with(good, SH_DIRTY, 66, &reason) == SMALL_BAD);
    CHECK(unpack_with(good, SH_PATHS, GPUDIFF_SMALL_PASS_MAX_PATHS + 1, &reason) == SMALL_BAD);
    CHECK(unpack_with(good, SH_BYTES, (uint32_t)gl.total - 1, &reason) == SMALL_BAD);  // smaller than its sections
    CHECK(unpack_with(good, SH_BYTES, 0, &reason) == SMALL_BAD);
    CHECK(unpack_with(good, SH_BYTES, (uint32_t)small_image_capacity() + 1, &reason) == SMALL_BAD);
    CHECK(unpack_with(good, SH_PATHS, 24, &reason) == SMALL_BAD);  // counts that outgrow total_bytes
    {   // the lists must index each other
        std::vector<uint8_t> img = good;
        const uint32_t v = 65;
        memcpy(img.data() + gl.dirty_idx + 4 * 3, &v, 4);  // a dirty pair's row past the batch
        CHECK(unpack_with(img, SH_REASON, 0, &reason) == SMALL_BAD);
        img = good;
        const uint32_t w = 24;
        memcpy(img.data() + gl.path_off + 4 * 4, &w, 4);  // offsets that run backwards
        CHECK(unpack_with(img, SH_REASON, 0, &reason) == SMALL_BAD);
        img = good;
        memcpy(img.data() + gl.path_off + 4 * 10, &w, 4);  // the last offset is not the path count
        CHECK(unpack_with(img, SH_REASON, 0, &reason) == SMALL_BAD);
    }
    {   // a declined pass is a header only
        std::vector<uint8_t> img(good.begin(), good.begin() + 64);
        uint32_t zero = 0, why = kSmallDeep | kSmallPaths, len = 64;
        memcpy(img.data() + 4 * SH_FINAL, &zero, 4);
        memcpy(img.data() + 4 * SH_REASON, &why, 4);
        memcpy(img.data() + 4 * SH_BYTES, &len, 4);
        RS rs;
        std::vector<uint32_t> idx;
        std::vector<uint8_t> noop;
        uint64_t need = 0;
        CHECK(unpack_prefix(img, 64, rs, idx, noop, &need, &reason) == SMALL_DECLINED);
        CHECK(reason == why);
        CHECK(unpack_with(img, SH_REASON, 0, &reason) == SMALL_BAD);
        CHECK(unpack_with(img, SH_REASON, 8, &reason) == SMALL_BAD);
    }
    if (!bad) std::printf("ok\n");
    return bad ? 1 : 0;
}
'''

SAN = ["-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _sanitizers_link(d):
    probe = os.path.join(d, "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17"] + SAN + [probe, "-o", os.path.join(d, "probe")], capture_output=True)
    return r.returncode == 0


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("small_pass"))
    if not _sanitizers_link(d):
        pytest.skip("g++ cannot link -fsanitize=address,undefined here: the small_pass.h host program was not run")
    src = os.path.join(d, "main.cpp")
    with open(src, "w") as f:
        f.write(MAIN)
    subprocess.run(["g++", "-std=c++17"] + SAN + ["-I", os.path.join(ROOT, "kcp_amd", "csrc"), src, "-o",
                                                   os.path.join(d, "t")], check=True)
    return os.path.join(d, "t")


def test_image_layout_and_unpacker(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert MAIN.count("CHECK(") >= 40  # the program still holds its checks
