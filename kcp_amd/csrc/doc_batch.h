// A resident batch of caller-supplied JSON documents for the wave-per-document kernels K10, K11 and K13
// (upsert.cpp, rollup.cpp, negotiate.cpp): how its document table is laid out, and the device side the three
// batch types share (DESIGN.md §4f').  The layout is host arithmetic only and this header makes no HIP runtime
// call; DocBatch's members that do are in doc_batch.cpp.  HIP's types (hipError_t, hipEvent_t) come with tokenize.h.
#pragma once
#include <string.h>

#include <vector>

#include "tokenize.h"

struct gpudiff_ctx;

namespace gd {

using DocBytesFn = uint64_t (*)(uint32_t json_len);

struct DocTableBytes {
    uint64_t json_bytes = 0;     // the staged JSON, the trailing kTokSlack included
    uint64_t scratch_bytes = 0;  // the documents' working areas
    uint64_t out_bytes = 0;      // their output room (0 without an out_of)
};

// Fills docs[0, n): document i has raw_len(i) bytes (clamped to kTokMaxLen + 1, never wrapped), a 16-B aligned
// staged span of tok_staged_span, scratch_of(len) bytes of working area at a running offset and, with an out_of,
// out_of(len) bytes of output room at the running offset each(i, doc, out_off) is told.  A document beyond
// kTokMaxLen keeps its TokDoc (the kernel reports GPUDIFF_TOK_SIZE) with the offsets it would have had, and takes
// no span, no scratch and no room.  each() writes the mode word (TokDoc.pad), which is zero before it.
template <class RawLen, class Each>
inline DocTableBytes lay_out_docs(TokDoc* docs, size_t n, RawLen raw_len, DocBytesFn scratch_of, DocBytesFn out_of,
                                  Each each) {
    DocTableBytes B;
    for (size_t i = 0; i < n; i++) {
        const uint64_t raw = raw_len(i);
        TokDoc& t = docs[i];
        memset(&t, 0, sizeof(t));
        t.json_off = B.json_bytes;
        t.json_len = raw > kTokMaxLen ? kTokMaxLen + 1 : (uint32_t)raw;
        t.scratch_off = B.scratch_bytes;
        each(i, t, B.out_bytes);
        if (t.json_len <= kTokMaxLen) {
            B.json_bytes += tok_staged_span(t.json_len);
            B.scratch_bytes += scratch_of(t.json_len);
            if (out_of) B.out_bytes += out_of(t.json_len);
        }
    }
    B.json_bytes += kTokSlack;
    return B;
}

// HIP's answer as the C-ABI's, the error text kept for gpudiff_strerror as HIPCHK keeps it: out of memory is
// GPUDIFF_E_CAPACITY, any other failure GPUDIFF_E_DEVICE
int doc_batch_rc(hipError_t e);
// what every *_free does first: the context's device current and its stream drained, so no kernel reads the batch
void doc_batch_quiesce(gpudiff_ctx* c);

// a host buffer that goes up with a batch's documents (DocBatch::upload)
struct HostCopy {
    void* dst = nullptr;
    const void* src = nullptr;
    size_t bytes = 0;
};

// The device side of a resident document batch.  gpudiff_wbatch, gpudiff_rbatch and gpudiff_nbatch derive from it
// and add their mode's buffers (through alloc(), so that release() frees them too) and launches.
struct DocBatch {
    std::vector<TokDoc> docs;
    uint64_t json_bytes = 0, scratch_bytes = 0;
    void *d_json = nullptr, *d_scratch = nullptr, *d_docs = nullptr;
    // GPUDIFF_OPT_TIMING: n_ev events around the run's launches, interval k between events k and k + 1
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    uint32_t n_ev = 0;
    bool pending_timing = false;  // the last run's events are recorded and not folded in yet
    uint64_t runs = 0;
    double ms_sum[2] = {0, 0};

    DocBatch() = default;
    DocBatch(const DocBatch&) = delete;
    DocBatch& operator=(const DocBatch&) = delete;
    ~DocBatch() { release(); }

    // a device buffer of `bytes` that release() frees
    int alloc(void** p, uint64_t bytes);
    // d_json / d_scratch / d_docs for the laid-out table, the documents' bytes (src_of(i): document i's, or null)
    // up through one zeroed pinned buffer with the table and, behind them on the same stream, the mode's `also`;
    // the stream synchronised (whatever was enqueued, so no host buffer is left in flight); then, on a timing
    // context, n_events events.  Whatever fails, the batch's destructor releases what was made.
    template <class SrcOf>
    int upload(gpudiff_ctx* c, const DocTableBytes& B, SrcOf src_of, uint32_t n_events, HostCopy also = {}) {
        uint8_t* stage = nullptr;
        const int rc = upload_begin(B, &stage);
        if (rc) return rc;
        for (size_t i = 0; i < docs.size(); i++) {
            const TokDoc& t = docs[i];
            const uint8_t* src = src_of(i);
            if (src && t.json_len && t.json_len <= kTokMaxLen) memcpy(stage + t.json_off, src, t.json_len);
        }
        return upload_end(c, stage, n_events, also);
    }
    // event k into the context's stream (nothing without events); the last one leaves a timing pending
    int record(gpudiff_ctx* c, uint32_t k);
    // the pending timing (if any) into runs / ms_sum; an interval HIP cannot give drops that run's timing only.
    // fold_timing: the caller has synchronised the stream (a fetch).  await_timing: waits for the last event first
    // (a run folds the run before it), and fails only if that wait does.
    void fold_timing();
    int await_timing();
    double mean_ms(uint32_t k) const { return runs ? ms_sum[k] / (double)runs : 0.0; }
    void release();

   private:
    std::vector<void*> owned_;
    int upload_begin(const DocTableBytes& B, uint8_t** stage);
    int upload_end(gpudiff_ctx* c, uint8_t* stage, uint32_t n_events, HostCopy also);
};

}  // namespace gd
