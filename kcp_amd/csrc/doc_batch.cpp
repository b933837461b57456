// DocBatch (doc_batch.h): the device buffers, the upload and the timing events of a resident document batch.
#include "doc_batch.h"

#include "engine.h"

namespace gd {

int doc_batch_rc(hipError_t e) {
    if (e == hipSuccess) return GPUDIFF_OK;
    g_last_hip_error = hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? GPUDIFF_E_CAPACITY : GPUDIFF_E_DEVICE;
}

void doc_batch_quiesce(gpudiff_ctx* c) {
    if (!c || !c->has_device) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
}

int DocBatch::alloc(void** p, uint64_t bytes) {
    *p = nullptr;
    const int rc = doc_batch_rc(hipMalloc(p, bytes));
    if (!rc) owned_.push_back(*p);
    return rc;
}

int DocBatch::upload_begin(const DocTableBytes& B, uint8_t** stage) {
    json_bytes = B.json_bytes;
    scratch_bytes = B.scratch_bytes;
    int rc;
    if ((rc = alloc(&d_json, json_bytes))) return rc;
    if ((rc = alloc(&d_scratch, std::max<uint64_t>(scratch_bytes, 256)))) return rc;
    if ((rc = alloc(&d_docs, std::max<size_t>(docs.size(), 1) * sizeof(TokDoc)))) return rc;
    if ((rc = doc_batch_rc(hipHostMalloc((void**)stage, json_bytes, hipHostMallocDefault)))) return rc;
    memset(*stage, 0, json_bytes);
    return GPUDIFF_OK;
}

int DocBatch::upload_end(gpudiff_ctx* c, uint8_t* stage, uint32_t n_events, HostCopy also) {
    hipError_t e = hipMemcpyAsync(d_json, stage, json_bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && !docs.empty())
        e = hipMemcpyAsync(d_docs, docs.data(), docs.size() * sizeof(TokDoc), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && also.bytes)
        e = hipMemcpyAsync(also.dst, also.src, also.bytes, hipMemcpyHostToDevice, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);  // also after a failure: nothing reads `stage` or `also` later
    if (e == hipSuccess) e = es;
    (void)hipHostFree(stage);
    if (e == hipSuccess && (c->flags & GPUDIFF_OPT_TIMING))
        while (n_ev < n_events && (e = hipEventCreate(&ev[n_ev])) == hipSuccess) n_ev++;
    return doc_batch_rc(e);
}

int DocBatch::record(gpudiff_ctx* c, uint32_t k) {
    if (k >= n_ev) return GPUDIFF_OK;
    HIPCHK(hipEventRecord(ev[k], c->stream));
    if (k + 1 == n_ev) pending_timing = true;
    return GPUDIFF_OK;
}

int DocBatch::await_timing() {
    if (pending_timing) HIPCHK(hipEventSynchronize(ev[n_ev - 1]));
    fold_timing();
    return GPUDIFF_OK;
}

void DocBatch::fold_timing() {
    if (!pending_timing) return;
    float ms[2] = {0, 0};
    bool ok = true;
    for (uint32_t k = 0; k + 1 < n_ev && ok; k++) ok = hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]) == hipSuccess;
    if (ok) {
        ms_sum[0] += ms[0];
        ms_sum[1] += ms[1];
        runs++;
    }
    pending_timing = false;
}

void DocBatch::release() {
    for (void* p : owned_) (void)hipFree(p);
    owned_.clear();
    d_json = d_scratch = d_docs = nullptr;
    for (; n_ev; n_ev--) (void)hipEventDestroy(ev[n_ev - 1]);
    pending_timing = false;
}

}  // namespace gd
