"""kcp_amd/csrc/dstore_plan.h (plan_upload): how a device-encoded batch is cut into upload chunks and K0 launches.
Pure host arithmetic over the document table, so it is checked on hand-made TokDoc arrays -- lengths and offsets
only, no JSON and no GPU."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include "dstore_plan.h"
#include <cstdio>
#include <cstdlib>
using namespace gd;

#define CHECK(x) do { if (!(x)) { std::printf("%s:%d: %s failed (case %s)\n", __FILE__, __LINE__, #x, g_case); std::exit(1); } } while (0)
static const char* g_case = "";

// documents of the given lengths, laid out as dstore.cpp stages them; returns jbytes (the trailing slack included)
static uint64_t lay_out(std::vector<TokDoc>& docs, const std::vector<uint32_t>& lens) {
    docs.assign(lens.size() + 1, TokDoc{});  // + a sentinel behind the table: plan_upload must not touch it
    uint64_t at = 0;
    for (size_t i = 0; i < lens.size(); i++) {
        docs[i].json_off = at;
        docs[i].json_len = lens[i];
        docs[i].scratch_off = ~0ull;
        at += tok_staged_span(lens[i]);
    }
    docs[lens.size()].scratch_off = 0x5EED;
    return at + kTokSlack;
}

// every property a plan must have, for any table
static void check_plan(const UploadPlan& P, const std::vector<TokDoc>& docs, uint32_t nd, uint64_t jbytes,
                       uint64_t cap) {
    CHECK(P.C >= 1 && P.C <= kMaxUpChunks);
    // chunks partition [0, nd) on document boundaries, and their bytes partition [0, jbytes)
    CHECK(P.cdoc[0] == 0 && P.cdoc[P.C] == nd);
    CHECK(P.cbyte(0) == (nd ? 0 : jbytes) && P.cbyte(P.C) == jbytes);  // a chunk without documents: empty, at the end
    for (uint32_t q = 0; q < P.C; q++) {
        CHECK(P.cdoc[q] <= P.cdoc[q + 1]);
        CHECK(P.cbyte(q) <= P.cbyte(q + 1));
        if (P.cdoc[q] < nd) CHECK(P.cbyte(q) == docs[P.cdoc[q]].json_off);
    }
    // launches partition each chunk in order and never straddle one
    CHECK(P.launches.size() == P.chunk_of_launch.size());
    uint32_t at = 0;
    uint64_t max_sb = 0;
    for (size_t l = 0; l < P.launches.size(); l++) {
        const uint32_t a = P.launches[l].first, b = P.launches[l].second, q = P.chunk_of_launch[l];
        CHECK(a == at && b > a);
        CHECK(q < P.C && a >= P.cdoc[q] && b <= P.cdoc[q + 1]);
        if (l) CHECK(P.chunk_of_launch[l - 1] <= q);
        uint64_t sb = 0;  // scratch_off: the running sum within the launch
        for (uint32_t k = a; k < b; k++) {
            CHECK(docs[k].scratch_off == sb);
            sb += tok_scratch_bytes(docs[k].json_len);
        }
        CHECK(sb <= cap || b == a + 1);  // under the cap unless one document alone exceeds it
        max_sb = sb > max_sb ? sb : max_sb;
        at = b;
    }
    CHECK(at == nd);
    CHECK(P.max_sb == max_sb);
    CHECK(docs[nd].scratch_off == 0x5EED);
    // first_doc: the first document starting at or after a byte
    CHECK(P.first_doc(0) == 0 && P.first_doc(jbytes) == nd);
    if (nd > 1) CHECK(P.first_doc(1) == 1 && P.first_doc(docs[1].json_off) == 1);
}

static UploadPlan run(const char* name, std::vector<TokDoc>& docs, const std::vector<uint32_t>& lens,
                      uint64_t cap = kScratchCap) {
    g_case = name;
    const uint64_t jbytes = lay_out(docs, lens);
    UploadPlan P = cap == kScratchCap ? plan_upload(docs.data(), (uint32_t)lens.size(), jbytes)
                                      : plan_upload(docs.data(), (uint32_t)lens.size(), jbytes, cap);
    check_plan(P, docs, (uint32_t)lens.size(), jbytes, cap);
    return P;
}

int main() {
    std::vector<TokDoc> docs;
    {   // zero documents: jbytes is the slack alone, in one chunk with nothing to launch (and, as no document
        // starts in it, nothing to upload: its byte range is empty at jbytes)
        UploadPlan P = run("empty", docs, {});
        CHECK(P.jbytes == kTokSlack);
        CHECK(P.C == 1 && P.cdoc[0] == 0 && P.cdoc[1] == 0 && P.launches.empty() && P.max_sb == 0);
        CHECK(P.cbyte(0) == kTokSlack && P.cbyte(1) == kTokSlack);
    }
    {
        UploadPlan P = run("one", docs, {700});
        CHECK(P.C == 1 && P.launches.size() == 1 && P.max_sb == tok_scratch_bytes(700));
    }
    {   // many documents but few bytes
        UploadPlan P = run("small bytes", docs, std::vector<uint32_t>(3 * kMinChunkDocs, 100));
        CHECK(3 * kMinChunkDocs * tok_staged_span(100) < kUpChunkBytes);
        CHECK(P.C == 1 && P.launches.size() == 1);
    }
    {   // many bytes but few documents
        UploadPlan P = run("few docs", docs, std::vector<uint32_t>(kMinChunkDocs - 1, 4096));
        CHECK((kMinChunkDocs - 1) * 4096 >= 2 * kUpChunkBytes);
        CHECK(P.C == 1);
    }
    {   // 2 x kMinChunkDocs documents and >= 2 x kUpChunkBytes: two chunks, split at the documents' middle byte
        std::vector<uint32_t> lens(2 * kMinChunkDocs + 1);
        for (size_t i = 0; i < lens.size(); i++) lens[i] = 1024 + (uint32_t)(i % 7) * 16 + (uint32_t)(i % 3);  // odd sizes
        UploadPlan P = run("two chunks", docs, lens);
        CHECK(P.jbytes >= 2 * kUpChunkBytes);
        CHECK(P.C == 2 && P.launches.size() == 2);
        CHECK(P.cdoc[1] > 0 && P.cdoc[1] < lens.size());
        CHECK(docs[P.cdoc[1]].json_off >= P.jbytes / 2 && docs[P.cdoc[1] - 1].json_off < P.jbytes / 2);
        CHECK(docs[P.cdoc[1]].scratch_off == 0);  // a chunk starts a launch
    }
    {   // enough for more than kMaxUpChunks chunks by both rules: capped
        UploadPlan P = run("capped", docs, std::vector<uint32_t>(20 * kMinChunkDocs, 1008));
        CHECK(20 * kMinChunkDocs * tok_staged_span(1008) >= 20 * kUpChunkBytes);
        CHECK(P.C == kMaxUpChunks && P.launches.size() == kMaxUpChunks);
    }
    {   // a small scratch cap: several launches inside the one chunk, one document alone above the cap
        std::vector<uint32_t> lens(41, 300);
        lens[17] = 9000;
        const uint64_t cap = 3 * tok_scratch_bytes(300) + 1;
        CHECK(tok_scratch_bytes(9000) > cap);
        UploadPlan P = run("scratch cap", docs, lens, cap);
        CHECK(P.C == 1);
        // 17 documents in launches of 3 (6 launches), the large one alone, 23 more (8 launches)
        CHECK(P.launches.size() == 6 + 1 + 8);
        CHECK(P.launches[6].first == 17 && P.launches[6].second == 18);
        CHECK(P.max_sb == tok_scratch_bytes(9000));
    }
    {   // the cap splits launches within each of two chunks, never across the boundary
        std::vector<uint32_t> lens(2 * kMinChunkDocs, 1024);
        const uint64_t cap = 5000 * tok_scratch_bytes(1024);
        UploadPlan P = run("cap and chunks", docs, lens, cap);
        CHECK(P.C == 2 && P.cdoc[1] == kMinChunkDocs + 1);  // the middle byte (slack included) lies inside document 16384
        CHECK(P.launches.size() == 2 * 4);  // 16385 = 3 x 5000 + 1385, 16383 = 3 x 5000 + 1383
        CHECK(P.max_sb == cap);
    }
    std::printf("ok\n");
    return 0;
}
'''


def test_plan_upload():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        exe = os.path.join(d, "t")
        with open(src, "w") as f:
            f.write(SRC)
        subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "kcp_amd", "csrc"),
                        "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
        assert r.stdout.strip() == "ok"
