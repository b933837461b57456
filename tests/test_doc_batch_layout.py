"""kcp_amd/csrc/doc_batch.h (lay_out_docs): the document table of a K10 / K11 / K13 batch.  Pure host arithmetic,
so it is checked on lengths alone -- no JSON and no GPU -- against a literal restatement of the loop the three
batch types each carried before they shared it, field by field, under the address and undefined-behaviour
sanitizers (a stand-alone program, run directly)."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include "doc_batch.h"
#include <cstdio>
#include <cstdlib>
using namespace gd;

#define CHECK(x) do { if (!(x)) { std::printf("%s:%d: %s failed (case %s)\n", __FILE__, __LINE__, #x, g_case); std::exit(1); } } while (0)
static const char* g_case = "";

enum Mode { kRoll, kMarshal, kPairs };
static const uint64_t kAbsent = ~0ull;  // kPairs: an old side that is not there (a null pointer in the API)

// The loop as rollup.cpp had it (upsert.cpp's with the marshal offsets, negotiate.cpp's over interleaved pairs):
// the reference.  lens: kRoll / kMarshal one per document; kPairs old, new, old, new, ... and kinds one per pair.
struct Ref {
    std::vector<TokDoc> docs;
    uint64_t jb = 0, sb = 0, ob = 0;
};
static Ref reference(Mode m, const std::vector<uint64_t>& lens, const std::vector<uint8_t>& kinds) {
    Ref R;
    const size_t n = lens.size();
    R.docs.resize(n);
    uint64_t jb = 0, sb = 0, ob = 0;
    for (size_t i = 0; i < n; i++) {
        size_t raw = (size_t)lens[i];
        if (m == kPairs && (i & 1) == 0 && lens[i] == kAbsent) raw = 0;
        const uint32_t l = raw > kTokMaxLen ? kTokMaxLen + 1 : (uint32_t)raw;
        TokDoc& t = R.docs[i];
        memset(&t, 0, sizeof(t));
        t.json_off = jb;
        t.json_len = l;
        t.scratch_off = sb;
        if (m == kMarshal) tokdoc_set_marshal_off(t, ob);
        if (m == kPairs) tokdoc_set_neg_kind(t, kinds[i / 2]);
        if (l <= kTokMaxLen) {
            jb = (jb + l + kTokSlack + 15) & ~15ull;
            sb += m == kMarshal ? marshal_scratch_bytes(l) : rollup_scratch_bytes(l);
            if (m == kMarshal) ob += marshal_out_cap(l);
        }
    }
    jb += kTokSlack;
    R.jb = jb;
    R.sb = sb;
    R.ob = ob;
    return R;
}

// lay_out_docs as the three callers use it; a sentinel behind the table must stay untouched
static std::vector<TokDoc> run(const char* name, Mode m, const std::vector<uint64_t>& lens,
                               const std::vector<uint8_t>& kinds = {}) {
    g_case = name;
    const size_t n = lens.size();
    std::vector<TokDoc> docs(n + 1);
    memset(docs.data(), 0xEE, (n + 1) * sizeof(TokDoc));
    DocTableBytes B;
    if (m == kRoll)
        B = lay_out_docs(docs.data(), n, [&](size_t i) { return (size_t)lens[i]; }, rollup_scratch_bytes, nullptr,
                         [](size_t, TokDoc&, uint64_t) {});
    else if (m == kMarshal)
        B = lay_out_docs(docs.data(), n, [&](size_t i) { return (size_t)lens[i]; }, marshal_scratch_bytes,
                         marshal_out_cap, [](size_t, TokDoc& t, uint64_t off) { tokdoc_set_marshal_off(t, off); });
    else
        B = lay_out_docs(docs.data(), n,
                         [&](size_t i) { return (i & 1) ? (size_t)lens[i] : (lens[i] == kAbsent ? 0 : (size_t)lens[i]); },
                         rollup_scratch_bytes, nullptr,
                         [&](size_t i, TokDoc& t, uint64_t) { tokdoc_set_neg_kind(t, kinds[i / 2]); });
    // equal to the reference, field by field (and byte by byte: the padding too)
    const Ref R = reference(m, lens, kinds);
    CHECK(B.json_bytes == R.jb && B.scratch_bytes == R.sb && B.out_bytes == R.ob);
    for (size_t i = 0; i < n; i++) {
        CHECK(docs[i].json_off == R.docs[i].json_off);
        CHECK(docs[i].json_len == R.docs[i].json_len);
        CHECK(docs[i].scratch_off == R.docs[i].scratch_off);
        CHECK(docs[i].seed == 0 && docs[i].pad[0] == R.docs[i].pad[0] && docs[i].pad[1] == R.docs[i].pad[1]);
        CHECK(memcmp(&docs[i], &R.docs[i], sizeof(TokDoc)) == 0);
    }
    for (size_t k = 0; k < sizeof(TokDoc); k++) CHECK(((const uint8_t*)&docs[n])[k] == 0xEE);
    // the properties, for any table
    uint64_t spans = 0, sb = 0, ob = 0;
    bool have_prev = false;
    uint64_t prev_off = 0;
    for (size_t i = 0; i < n; i++) {
        const TokDoc& t = docs[i];
        const uint64_t raw = m == kPairs && !(i & 1) && lens[i] == kAbsent ? 0 : lens[i];
        CHECK(t.json_len == (raw > kTokMaxLen ? kTokMaxLen + 1 : raw));  // clamped, never wrapped
        CHECK(t.json_off == spans && t.json_off % 16 == 0);
        CHECK(t.scratch_off == sb);  // running sums
        if (m == kMarshal) CHECK(tokdoc_marshal_off(t) == ob);
        if (m == kPairs) CHECK(tokdoc_neg_kind(t) == kinds[i / 2]);
        if (t.json_len > kTokMaxLen) continue;  // no span, no scratch, no room
        if (have_prev) CHECK(t.json_off > prev_off);  // strictly increasing over the documents that are staged
        have_prev = true;
        prev_off = t.json_off;
        CHECK(t.json_off + t.json_len + kTokSlack <= B.json_bytes);  // the slack is readable
        spans += tok_staged_span(t.json_len);
        sb += m == kMarshal ? marshal_scratch_bytes(t.json_len) : rollup_scratch_bytes(t.json_len);
        if (m == kMarshal) ob += marshal_out_cap(t.json_len);
    }
    CHECK(B.json_bytes == spans + kTokSlack && B.scratch_bytes == sb && B.out_bytes == ob);
    docs.resize(n);
    return docs;
}

int main() {
    const uint64_t M = kTokMaxLen;
    const std::vector<uint64_t> every = {0, 1, 15, 16, 17, M - 1, M, M + 1, (1ull << 32) + 5};
    CHECK(sizeof(size_t) == 8);  // 2^32 + 5 is a length the API can be given
    for (Mode m : {kRoll, kMarshal}) {
        run("empty table", m, {});
        for (uint64_t l : every) {
            std::vector<TokDoc> d = run("one document", m, {l});
            CHECK(d[0].json_off == 0 && d[0].scratch_off == 0 && d[0].json_len == (l > M ? M + 1 : l));
        }
        run("every length", m, every);
        run("every length, reversed", m, std::vector<uint64_t>(every.rbegin(), every.rend()));
        {   // a table whose only document is oversize: the slack alone is staged
            g_case = "only oversize";
            TokDoc t;
            const DocTableBytes B = lay_out_docs(&t, 1, [&](size_t) { return (size_t)(M + 1); },
                                                 m == kMarshal ? marshal_scratch_bytes : rollup_scratch_bytes,
                                                 m == kMarshal ? marshal_out_cap : nullptr,
                                                 [](size_t, TokDoc&, uint64_t) {});
            CHECK(B.json_bytes == kTokSlack && B.scratch_bytes == 0 && B.out_bytes == 0 && t.json_len == M + 1);
        }
        for (uint64_t big : {M + 1, (uint64_t)(1ull << 32) + 5}) {
            // an oversize document between two small ones: the neighbours lie exactly where they do without it,
            // and it carries the offsets the document behind it gets
            std::vector<TokDoc> with = run("oversize between", m, {17, big, 33});
            std::vector<TokDoc> without = run("without it", m, {17, 33});
            CHECK(memcmp(&with[0], &without[0], sizeof(TokDoc)) == 0);
            CHECK(memcmp(&with[2], &without[1], sizeof(TokDoc)) == 0);
            CHECK(with[1].json_off == with[2].json_off && with[1].scratch_off == with[2].scratch_off);
            CHECK(with[1].pad[0] == with[2].pad[0] && with[1].pad[1] == with[2].pad[1]);
            CHECK(with[1].json_len == M + 1);
        }
    }
    {   // the marshal variant's output offsets: the room of the documents before
        std::vector<TokDoc> d = run("marshal offsets", kMarshal, {100, 0, 7});
        CHECK(tokdoc_marshal_off(d[0]) == 0 && tokdoc_marshal_off(d[1]) == marshal_out_cap(100));
        CHECK(tokdoc_marshal_off(d[2]) == marshal_out_cap(100) + marshal_out_cap(0));
    }
    {   // interleaved pairs: an absent old is an empty document whatever length came with it, kinds per pair
        run("no pairs", kPairs, {}, {});
        std::vector<TokDoc> d = run("pairs", kPairs, {40, 41, kAbsent, 50, 0, 17, M + 1, 9, 12, (1ull << 32) + 5},
                                    {0, 1, 0, 1, 1});
        CHECK(d[2].json_len == 0 && d[3].json_off == d[2].json_off + tok_staged_span(0));
        CHECK(tokdoc_neg_kind(d[2]) == 1 && tokdoc_neg_kind(d[3]) == 1 && tokdoc_neg_kind(d[4]) == 0);
        CHECK(d[6].json_len == M + 1 && d[7].json_off == d[6].json_off);
        CHECK(d[9].json_len == M + 1);
        for (uint64_t l : every) run("pair of one length", kPairs, {l, l}, {1});
    }
    std::printf("ok\n");
    return 0;
}
'''


def test_lay_out_docs():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        exe = os.path.join(d, "t")
        with open(src, "w") as f:
            f.write(SRC)
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-host-only", "-O1", "-std=c++17", "-Wall", "-Xarch_host",
                        "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "kcp_amd", "csrc"), "-I", os.path.join(ROOT, "include"), src,
                        "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
        assert r.stdout.strip() == "ok"
