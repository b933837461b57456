// Device-encode mode of the object store (dstore.cpp); internal.
#pragma once
#include "engine.h"
#include "tokenize.h"

#include <vector>

struct DStore;

DStore* dstore_create(gpudiff_ctx* c, uint32_t max_slots, uint64_t space_bytes, uint32_t max_events, int* rc);
int dstore_submit(gpudiff_ctx* c, DStore* s, const gpudiff_event* ev, size_t n, gpudiff_ticket* ticket);
int dstore_forget(gpudiff_ctx* c, DStore* s, uint32_t slot);
// gpudiff_submit with GPUDIFF_OPT_DEVICE_ENCODE: pairs through K0 (c->pair_store);
// GPUDIFF_E_CAPACITY = take the host-encode path for this batch
int dstore_submit_pairs(gpudiff_ctx* c, const gpudiff_json_pair* pairs, size_t n, gpudiff_ticket* ticket);
int dstore_stats(const DStore* s, gpudiff_store_stats* out);
void dstore_timing_reset(DStore* s);  // gpudiff_timing_reset: the submit path's phase sums too
void dstore_free(gpudiff_ctx* c, DStore* s);
void dstore_host_bufs_release(gpudiff_ctx* c);  // gpudiff_close: the context's remaining gpudiff_host_alloc buffers

// The staged JSON of a waited pair-mode batch (gpudiff_submit with GPUDIFF_OPT_DEVICE_ENCODE): pair i's
// old object is document 2i, its new one 2i + 1; hdocs[] holds their offsets into djson (HBM); flags = the
// batch's final result flags (host-deferred pairs resolved).  Valid until the ring slot is reused by the
// submit after the next one.  There is no host copy to offer: a zero-copy batch was uploaded from the
// caller's buffer (reusable once gpudiff_wait returned), so host work on a staged document reads it back
// from djson.
struct StagedPairs {
    const gd::TokDoc* hdocs = nullptr;
    const uint8_t* djson = nullptr;
    uint32_t n = 0;
    const std::vector<uint8_t>* flags = nullptr;
    const std::vector<gpudiff_event>* events = nullptr;
};
int dstore_staged_pairs(gpudiff_ctx* c, gpudiff_ticket t, StagedPairs* out);
// work launched on the context stream now reads the batch's device JSON: the ring slot's next upload waits
int dstore_staged_mark_read(gpudiff_ctx* c, gpudiff_ticket t);

// ------------------------------------------------------------------ the store's write plan
// gpudiff_store_write_plan_get's device side for a waited batch of a device-encode store: the write list and the
// bodies K10 rendered, as they came back from the device in one allocation, and the JSON of the documents K10 left to
// the host (gathered on the device, one copy back).  upsert.cpp has go_marshal.cpp marshal those and wraps the result.
struct StorePlan {
    size_t n = 0;                  // writes
    // offsets[n + 1] | pair_index[n] | src_doc[n] | k10[n] | tgt[n] (16 B each, only when asked for) | kind[n] |
    // noop[n] | pad | bytes; k10[] comes back as
    // K10's verdict words (store_plan.h plan_k10_word) and is unpacked in place, the splice points into rv_*_v
    std::vector<uint64_t> words;
    const uint64_t* offsets = nullptr;    // dense: body w = bytes[offsets[w], offsets[w + 1]); empty unless K10 rendered it
    const uint32_t* pair_index = nullptr;
    const uint32_t* src_doc = nullptr;
    const int32_t* k10 = nullptr;         // GPUDIFF_TOK_*; not OK: the host renders the body
    const uint8_t* kind = nullptr;
    const uint8_t* noop = nullptr;
    const uint32_t* rv_off = nullptr;     // K10's resourceVersion splice point per write (GPUDIFF_RV_*; a write
    const uint8_t* rv_form = nullptr;     // without a device body: 0 / GPUDIFF_RV_NONE)
    const gd::TargetWords* tgt = nullptr; // K10's request target per write (all zero without a device body); null
                                          // unless the plan was asked for targets
    const uint8_t* bytes = nullptr;
    std::vector<uint32_t> rv_off_v;
    std::vector<uint8_t> rv_form_v;
    std::vector<uint32_t> def;    // the writes whose document K10 left to the host, ascending
    std::vector<uint8_t> hjson;    // their documents' JSON: write def[k]'s at hjson[hoff[k]], hlen[k] bytes
    std::vector<uint64_t> hoff;
    std::vector<uint32_t> hlen;
};
// kinds: GPUDIFF_PLAN_SPEC | GPUDIFF_PLAN_STATUS; targets: GPUDIFF_PLAN_TARGETS was asked for.  GPUDIFF_E_STATE: not a waited ticket of this store whose ring slot
// still holds the batch, or the store is broken; GPUDIFF_E_CAPACITY: no device memory for the plan's buffers
int dstore_write_plan(gpudiff_ctx* c, DStore* s, gpudiff_ticket t, uint32_t kinds, bool targets, StorePlan* out);
int dstore_plan_stats(const DStore* s, gpudiff_store_plan_stats* out);
// store.cpp: the device-encode store behind a gpudiff_store, null for a host-encode one
DStore* gpudiff_store_dstore(gpudiff_store* s);
