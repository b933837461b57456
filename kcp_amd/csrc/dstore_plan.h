// How a device-encoded batch's staged JSON is cut into upload chunks and K0 launches (dstore.cpp's plan_upload
// phase).  Host arithmetic over the document table only: no HIP runtime call.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

#include "tokenize.h"

namespace gd {

constexpr uint64_t kScratchCap = 2ull << 30;  // K0 working area, reused across launches
// a device-encoded batch's JSON is staged, uploaded and encoded in up to kMaxUpChunks chunks of at least
// kUpChunkBytes (whole documents): the smaller the chunks, the sooner the first upload starts and the shorter
// the last chunk's K0 after the copy stream is done.  Compile-time constants: nothing overrides them at run time.
constexpr uint32_t kMaxUpChunks = 16;
constexpr uint64_t kUpChunkBytes = 16ull << 20;
// ... and of at least kMinChunkDocs documents: each chunk's K0 launch (a wave per document) should fill the
// chip's ~8k resident waves twice over (r04m: 12 chunks of 5.4k documents made config5's K0 6.4 ms, from 4.1)
constexpr uint64_t kMinChunkDocs = 16384;

struct UploadPlan {
    const TokDoc* docs = nullptr;
    uint32_t nd = 0;
    uint64_t jbytes = 0;                // the staged JSON, the trailing kTokSlack included
    uint32_t C = 1;                     // chunks
    uint32_t cdoc[kMaxUpChunks + 1] = {};  // chunk q holds documents [cdoc[q], cdoc[q + 1])
    std::vector<std::pair<uint32_t, uint32_t>> launches;  // K0 over [first, last), in order, never across a chunk
    std::vector<uint32_t> chunk_of_launch;
    uint64_t max_sb = 0;  // the largest launch's scratch: one such area per K0 stream

    uint32_t first_doc(uint64_t b) const {  // first document starting at or after byte b
        uint32_t lo = 0, hi = nd;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) / 2;
            if (docs[mid].json_off < b) lo = mid + 1;
            else hi = mid;
        }
        return lo;
    }
    uint64_t cbyte(uint32_t q) const {  // chunk q's first byte (q == C: the end)
        return q == C || cdoc[q] >= nd ? jbytes : docs[cdoc[q]].json_off;
    }
};

// Chunks of the batch's JSON (by bytes, whole documents): the host copies chunk c into pinned staging while chunk
// c - 1 is uploading, and K0 starts on a chunk as soon as it has landed, so copy, upload and encode of one batch
// overlap instead of running back to back.  Sets each docs[k].scratch_off: per-document areas within launches of
// at most scratch_cap (a single larger document gets a launch of its own).
inline UploadPlan plan_upload(TokDoc* docs, uint32_t nd, uint64_t jbytes, uint64_t scratch_cap = kScratchCap) {
    UploadPlan P;
    P.docs = docs;
    P.nd = nd;
    P.jbytes = jbytes;
    P.C = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(kMaxUpChunks, std::max<uint64_t>(1, nd / kMinChunkDocs)),
                                       std::max<uint64_t>(1, jbytes / kUpChunkBytes));
    for (uint32_t q = 0; q <= P.C; q++) P.cdoc[q] = q == P.C ? nd : P.first_doc(jbytes * q / P.C);
    for (uint32_t q = 0; q < P.C; q++) {
        uint64_t sb = 0;
        uint32_t first = P.cdoc[q];
        for (uint32_t k = P.cdoc[q]; k < P.cdoc[q + 1]; k++) {
            const uint64_t need = tok_scratch_bytes(docs[k].json_len);
            if (sb && sb + need > std::max(scratch_cap, need)) {
                P.launches.emplace_back(first, k);
                P.chunk_of_launch.push_back(q);
                first = k;
                sb = 0;
            }
            docs[k].scratch_off = sb;
            sb += need;
            P.max_sb = std::max(P.max_sb, sb);
        }
        if (P.cdoc[q + 1] > first) {
            P.launches.emplace_back(first, P.cdoc[q + 1]);
            P.chunk_of_launch.push_back(q);
        }
    }
    return P;
}

}  // namespace gd
