"""kcp_amd/csrc/stream_paths.h: the rule by which K2 turns the mismatching chunks of a size-matched region's compare
stream into its changed paths without the merge-join.  Plain arithmetic over the segment layout, so it is checked on
hand-made segments against a brute-force index-aligned compare -- in a stand-alone program built with the address
and undefined-behaviour sanitizers; no GPU, nothing loaded into Python."""
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include "stream_paths.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
using namespace gd;

static std::string g_case;
#define CHECK(x) do { if (!(x)) { std::printf("%s:%d: %s failed (case %s)\n", __FILE__, __LINE__, #x, g_case.c_str()); std::exit(1); } } while (0)

struct Leaf {
    uint32_t key, tag;
    std::string v;  // the value's bytes (ints: 8 bytes; true / false / null: none)
};
static Leaf int_leaf(uint32_t key, uint64_t x) { return Leaf{key, GPUDIFF_TAG_INT, std::string((const char*)&x, 8)}; }
static Leaf float_leaf(uint32_t key, uint64_t bits) { return Leaf{key, GPUDIFF_TAG_FLOAT, std::string((const char*)&bits, 8)}; }
static Leaf str_leaf(uint32_t key, const std::string& s) { return Leaf{key, GPUDIFF_TAG_STR, s}; }
static Leaf bool_leaf(uint32_t key, bool b) { return Leaf{key, b ? GPUDIFF_TAG_TRUE : GPUDIFF_TAG_FALSE, ""}; }

// vals[L] u64 | keys[L] u32 | metas[L] u32 | arena (tails at 4-byte aligned offsets, the whole padded to 16)
static std::vector<uint8_t> segment(const std::vector<Leaf>& ls) {
    const uint32_t L = (uint32_t)ls.size();
    std::vector<uint8_t> arena;
    std::vector<uint8_t> seg(16u * L, 0);
    for (uint32_t i = 0; i < L; i++) {
        const std::string& v = ls[i].v;
        uint64_t head = 0;
        std::memcpy(&head, v.data(), v.size() < 8 ? v.size() : 8);
        const uint32_t meta = gpudiff_meta(ls[i].tag, (uint32_t)v.size());
        std::memcpy(&seg[8u * i], &head, 8);
        std::memcpy(&seg[8u * L + 4u * i], &ls[i].key, 4);
        std::memcpy(&seg[12u * L + 4u * i], &meta, 4);
        if (gpudiff_meta_is_long(meta)) {
            arena.insert(arena.end(), v.begin() + 8, v.end());
            while (arena.size() & 3u) arena.push_back(0);
        }
    }
    while (arena.size() & 15u) arena.push_back(0);
    seg.insert(seg.end(), arena.begin(), arena.end());
    return seg;
}

// every mismatching 16-B chunk of two equally long segments, as the stream logs them (no cap here)
static std::vector<uint32_t> mismatches(const std::vector<uint8_t>& a, const std::vector<uint8_t>& b) {
    std::vector<uint32_t> e;
    CHECK(a.size() == b.size() && a.size() % 16 == 0);
    for (size_t c = 0; c < a.size() / 16; c++) {
        uint32_t dw = 0;
        for (uint32_t d = 0; d < 4; d++)
            if (std::memcmp(&a[16 * c + 4 * d], &b[16 * c + 4 * d], 4)) dw |= 1u << d;
        if (dw) e.push_back(sp_entry((uint32_t)c, dw));
    }
    return e;
}

// the index-aligned compare the merge-join makes when both key lists are equal: leaf i changed iff its meta, its
// val or its tail differs, each side's tail at that side's own offset
static std::vector<uint32_t> brute(const std::vector<Leaf>& A, const std::vector<Leaf>& B) {
    std::vector<uint32_t> out;
    for (size_t i = 0; i < A.size(); i++)
        if (A[i].tag != B[i].tag || A[i].v != B[i].v) out.push_back((uint32_t)i);
    return out;
}

enum Want { ACCEPT, REFUSE };
static void run(const std::string& name, const std::vector<Leaf>& A, const std::vector<Leaf>& B, Want want,
                const std::vector<uint8_t>* b_override = nullptr) {
    g_case = name;
    CHECK(A.size() == B.size());
    const std::vector<uint8_t> sa = segment(A);
    const std::vector<uint8_t> sb = b_override ? *b_override : segment(B);
    CHECK(sa.size() == sb.size());  // the rule is for size-matched regions only
    const std::vector<uint32_t> e = mismatches(sa, sb);
    CHECK(!e.empty());
    // exact-size heap copies: a read past a segment's end is the sanitizer's to find
    std::vector<uint8_t> ha(sa), hb(sb);
    uint32_t leaves[kSpMaxLeaves];
    const uint32_t n = sp_region_rule(ha.data(), hb.data(), (uint32_t)A.size(), ha.size(), e.data(), (uint32_t)e.size(),
                                      leaves);
    if (want == REFUSE) {
        CHECK(n == kSpRefuse);
        return;
    }
    CHECK(n != kSpRefuse);
    bool keys_equal = true;
    for (size_t i = 0; i < A.size(); i++) keys_equal = keys_equal && A[i].key == B[i].key;
    CHECK(keys_equal);
    const std::vector<uint32_t> want_s = brute(A, B);
    CHECK(n == want_s.size());
    for (uint32_t k = 0; k < n; k++) CHECK(leaves[k] == want_s[k]);
}

// L leaves with long strings, ints and booleans around position p, whose leaf the case replaces
static std::vector<Leaf> base(uint32_t L, uint32_t p, const Leaf& at_p) {
    std::vector<Leaf> ls;
    for (uint32_t i = 0; i < L; i++) {
        const uint32_t key = 100u + 10u * i;
        if (i == p) { Leaf l = at_p; l.key = key; ls.push_back(l); }
        else if (i % 3 == 0) ls.push_back(str_leaf(key, std::string(9 + i, (char)('a' + i))));
        else if (i % 3 == 1) ls.push_back(int_leaf(key, 1000 + i));
        else ls.push_back(bool_leaf(key, true));
    }
    return ls;
}
static void pair_case(const char* what, uint32_t L, uint32_t p, const Leaf& a, const Leaf& b, Want want) {
    run(std::string(what) + " L=" + std::to_string(L) + " p=" + std::to_string(p), base(L, p, a), base(L, p, b), want);
}

int main() {
    // where a dword lies: the boundaries of vals | keys | metas | arena for odd and even L
    for (uint32_t L = 1; L <= 9; L++)
        for (uint64_t b = 0; b < 16u * L + 32u; b += 4) {
            const SpWhere w = sp_classify(b, L);
            if (b < 8u * L) CHECK(w.cls == SP_VAL && w.idx == b / 8);
            else if (b < 12u * L) CHECK(w.cls == SP_KEY && w.idx == (b - 8u * L) / 4);
            else if (b < 16u * L) CHECK(w.cls == SP_META && w.idx == (b - 12u * L) / 4);
            else CHECK(w.cls == SP_ARENA && w.idx == b - 16u * L);
        }
    const uint64_t one = 0x3FF0000000000000ull;  // 1.0
    for (uint32_t L = 1; L <= 9; L++)
        for (uint32_t p = 0; p < L; p++) {
            pair_case("inline val", L, p, int_leaf(0, 7), int_leaf(0, 8), ACCEPT);
            pair_case("tag only", L, p, bool_leaf(0, true), bool_leaf(0, false), ACCEPT);
            pair_case("tag only int-float", L, p, int_leaf(0, one), float_leaf(0, one), ACCEPT);
            pair_case("inline length", L, p, str_leaf(0, "abc"), str_leaf(0, "abcd"), ACCEPT);
            pair_case("inline to 8", L, p, str_leaf(0, "abcdefg"), str_leaf(0, "abcdefgh"), ACCEPT);
            {   // long, equal length, one byte of the tail: first, middle and last tail byte
                const std::string s(29, 'q');
                for (size_t at : {(size_t)8, (size_t)17, (size_t)28}) {
                    std::string t = s;
                    t[at] = 'r';
                    pair_case("long tail", L, p, str_leaf(0, s), str_leaf(0, t), ACCEPT);
                }
                std::string h = s;  // ... and of the head alone (the val)
                h[3] = 'r';
                pair_case("long head", L, p, str_leaf(0, s), str_leaf(0, h), ACCEPT);
            }
            // the length changes within the padding (tails of 1 and 2 bytes, both padded to 4), either way
            pair_case("long within padding", L, p, str_leaf(0, "123456789"), str_leaf(0, "1234567890"), ACCEPT);
            pair_case("long within padding back", L, p, str_leaf(0, "1234567890"), str_leaf(0, "123456789"), ACCEPT);
            pair_case("long within padding 3-4", L, p, str_leaf(0, "12345678abc"), str_leaf(0, "12345678abcd"), ACCEPT);
            // ... and across it (tails of 4 and 5 bytes: 4 and 8 padded) while the arena's 16-B size stays: every later
            // tail shifts
            {
                const std::vector<Leaf> A = base(L, p, str_leaf(0, "12345678abcd")), B = base(L, p, str_leaf(0, "12345678abcde"));
                if (segment(A).size() == segment(B).size()) {
                    run("long across padding L=" + std::to_string(L) + " p=" + std::to_string(p), A, B, REFUSE);
                    // shrinking: every differing arena dword lies in a tail of side A, only the lengths tell
                    run("long across padding back L=" + std::to_string(L) + " p=" + std::to_string(p), B, A, REFUSE);
                }
                const std::vector<Leaf> A2 = base(L, p, str_leaf(0, "12345678")), B2 = base(L, p, str_leaf(0, "123456789"));
                if (segment(A2).size() == segment(B2).size()) run("inline to long L=" + std::to_string(L) + " p=" + std::to_string(p), A2, B2, REFUSE);
            }
            {   // one key renamed (still ascending), the value kept
                std::vector<Leaf> A = base(L, p, int_leaf(0, 5)), B = A;
                B[p].key += 3;
                run("key L=" + std::to_string(L) + " p=" + std::to_string(p), A, B, REFUSE);
                B[p].v = int_leaf(0, 6).v;  // ... and with the value changed too
                run("key and val L=" + std::to_string(L) + " p=" + std::to_string(p), A, B, REFUSE);
            }
            {   // two changed leaves: p and the last one
                std::vector<Leaf> A = base(L, p, int_leaf(0, 5)), B = base(L, p, int_leaf(0, 6));
                if (p + 1 < L) {
                    B[L - 1] = (L - 1) % 3 == 0 ? str_leaf(B[L - 1].key, std::string(9 + L - 1, 'Z')) : int_leaf(B[L - 1].key, 77);
                    if (segment(A).size() == segment(B).size()) run("two leaves L=" + std::to_string(L) + " p=" + std::to_string(p), A, B, ACCEPT);
                }
            }
        }
    // the across-padding case must have run where it matters: one long value grown under an equal 16-B arena size
    {
        const std::vector<Leaf> A = base(5, 1, str_leaf(0, "12345678abcd")), B = base(5, 1, str_leaf(0, "12345678abcde"));
        CHECK(segment(A).size() == segment(B).size());
        run("long across padding, a later tail shifts", A, B, REFUSE);
        run("long across padding back, a later tail shifts", B, A, REFUSE);
    }
    {   // a differing dword in the arena's final 16-B padding: no leaf owns it
        for (uint32_t L = 1; L <= 9; L++) {
            const std::vector<Leaf> A = base(L, 0, str_leaf(0, "123456789"));
            std::vector<uint8_t> sb = segment(A);
            uint32_t used = 0;
            for (const Leaf& l : A) used += sp_meta_arena(gpudiff_meta(l.tag, (uint32_t)l.v.size()));
            if (16u * L + used == sb.size()) continue;  // no padding at this L
            sb[sb.size() - 1] = 1;
            run("arena padding L=" + std::to_string(L), A, A, REFUSE, &sb);
        }
        const std::vector<Leaf> A = base(1, 0, str_leaf(0, "123456789"));
        std::vector<uint8_t> sb = segment(A);
        CHECK(sb.size() == 32);
        sb[16 + 4] = 1;  // the first padding dword, right behind the one tail
        run("arena padding, first dword", A, A, REFUSE, &sb);
    }
    {   // a chunk past the segment (the stream's line padding) cannot be placed
        g_case = "past the segment";
        const std::vector<uint8_t> sa = segment(base(3, 0, int_leaf(0, 1)));
        const uint32_t e = sp_entry((uint32_t)(sa.size() / 16), 1u);
        uint32_t leaves[kSpMaxLeaves];
        CHECK(sp_region_rule(sa.data(), sa.data(), 3, sa.size(), &e, 1, leaves) == kSpRefuse);
    }
    for (uint32_t changed : {64u, 65u}) {  // |S| = 64 is the most
        std::vector<Leaf> A, B;
        for (uint32_t i = 0; i < 70; i++) {
            A.push_back(int_leaf(10 + i, i));
            B.push_back(int_leaf(10 + i, i < changed ? i + 1000 : i));
        }
        run(std::to_string(changed) + " changed leaves", A, B, changed <= kSpMaxLeaves ? ACCEPT : REFUSE);
    }
    {   // many leaves, long values on both sides of the changed one: the arena owner past the first 64 leaves
        std::vector<Leaf> A;
        for (uint32_t i = 0; i < 150; i++) A.push_back(str_leaf(10 + i, std::string(9 + i % 23, (char)('a' + i % 26))));
        for (uint32_t p : {0u, 63u, 64u, 65u, 127u, 128u, 149u}) {
            std::vector<Leaf> B = A;
            B[p].v[B[p].v.size() - 1] ^= 1;
            run("150 long values p=" + std::to_string(p), A, B, ACCEPT);
        }
    }
    std::printf("ok\n");
    return 0;
}
'''


def test_stream_paths_rule():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/bin/hipcc"
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        exe = os.path.join(d, "t")
        with open(src, "w") as f:
            f.write(SRC)
        subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "kcp_amd", "csrc"), src, "-o", exe],
                       check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
        assert r.stdout.strip() == "ok"
