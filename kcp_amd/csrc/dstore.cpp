// Device-encode mode of the object store (gpudiff_store_create_ex with
// GPUDIFF_STORE_DEVICE_ENCODE; include/gpudiff.h): the informer's events go
// up as raw JSON and the GPU does the rest.
//
// submit (host work is a memcpy into pinned staging plus O(1) per event):
//   1. documents: each event's new object, plus its old object when the slot
//      has never been seen (the first sighting diffs against it); per slot a
//      chain of the batch's documents (prev/next) so events on one slot apply
//      in order;
//   2. one H2D of the JSON and the document table;
//   3. K0 (tokenize.hip) encodes every document into the current space; K0c
//      checks each event against its old side for path-hash collisions; K0x
//      walks the chains, writes the (old, new) rows and the slots' new resident
//      blobs; then the ordinary diff pass (K2..K6).
// Everything K0 does not take (a Go decode error, a float beyond its exact
// conversion, an escaped key, a duplicate key or a collision, ...) is
// deferred: its row is conservative in the device pass, the slot is marked
// pending, and gpudiff_wait re-does those events on the host with the
// Go-exact encoder (PairEncoder::store_decide, the one ladder store.cpp takes
// its decisions from too), places the blobs, diffs them and patches the
// results -- so every result equals the host store's, and later batches defer
// events of pending slots until then.
//
// dstore_submit drives these phases, in order: refuse_if_strings_need_compaction, claim_ring_slot,
// build_tables_pairs | build_tables_store, plan_upload (dstore_plan.h), grow_batch_buffers, stage_and_encode,
// link_and_diff; the ticket's finisher is finish_batch (render_text: the changed paths and values as text).  resolve
// (from finish_batch, when K0 deferred events):
// encode_deferred_pair | encode_deferred_store per event, slot_updates, place_conservative | place_and_diff,
// merge_results.
//
// Contract of this mode: event buffers stay valid until gpudiff_wait on the
// ticket returns (deferred events are re-read), and batches are waited in
// submit order, at most two in flight.
#include "dstore.h"
#include "dstore_plan.h"
#include "pathstr.h"
#include "plan.h"
#include "scan64.h"
#include "store_plan.h"
#include "values.h"

#include <emmintrin.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <mutex>
#include <new>
#include <thread>
#include <unordered_map>
#include <vector>

using namespace gd;

namespace {

// GPUDIFF_OPT_PATH_VALUES: K21 / K22's device buffers for one batch (a ring slot's, or the resolution batch's),
// cached and grown on demand, never allocated per batch
struct ValBufs {
    uint64_t* len = nullptr;     // K21: the texts' lengths [2n]
    uint64_t* tiles = nullptr;   // the scan's tile sums
    ValueSlot* slots = nullptr;  // K21's (leaf index, arena offset) per entry and side
    uint8_t* tags = nullptr;     // K21's tags [2n] (copied into out once it is sized)
    uint8_t* out = nullptr;      // offsets[2n + 1] | tags[2n], padded to 8 | bytes: one D2H
    uint64_t len_cap = 0, tiles_cap = 0, slots_cap = 0, tags_cap = 0, out_cap = 0;
    unsigned long long* ctr = nullptr;  // the resolution batch's own: total bytes, unresolved values
    hipEvent_t ev[4] = {};       // GPUDIFF_OPT_TIMING: K21 + scan begin/end, offsets + K22 begin/end
    void free_all() {
        for (void* p : {(void*)len, (void*)tiles, (void*)slots, (void*)tags, (void*)out, (void*)ctr})
            if (p) (void)hipFree(p);
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

struct Ring {
    gpudiff_dbatch* d = nullptr;  // rows, pair_ids, results; pool = the store's current space
    uint8_t* hjson = nullptr;     // pinned staging
    uint64_t hjson_cap = 0;
    uint8_t* hmeta = nullptr;     // pinned: TokDoc[] | DocLink[] | heads[]
    uint64_t hmeta_cap = 0;
    uint8_t* djson = nullptr;
    uint64_t djson_cap = 0;
    uint8_t* dmeta = nullptr;
    uint64_t dmeta_cap = 0;
    TokOut* douts = nullptr;
    uint8_t* dcoll = nullptr;
    uint8_t* ddef = nullptr;
    uint64_t docs_cap = 0, coll_cap = 0, def_cap = 0;
    uint32_t* dcnt = nullptr;     // deferred events of the batch
    hipEvent_t staged = nullptr;  // its H2D copies finished (pinned buffers reusable)
    hipEvent_t k0_done = nullptr;  // its K0..K0x finished reading the device JSON / document table
    bool k0_recorded = false;
    hipEvent_t pass_done = nullptr;  // pair mode: its diff pass finished reading its space (K0 may refill it)
    bool pass_recorded = false;
    hipEvent_t t_ev[5] = {};      // GPUDIFF_OPT_TIMING: H2D begin/end (copy stream), K0 begin/end, K0c+K0x end
    hipEvent_t chunk_ev[kMaxUpChunks] = {};  // each JSON chunk's H2D done: its K0 launches may start
    std::vector<gpudiff_event> events;
    std::vector<uint8_t> final_flags;  // the waited batch's result flags (deferred events resolved)
    bool waited = false;
    uint32_t batch = 0, nev = 0;
    uint64_t bound = 0;
    gpudiff_ticket ticket = 0;
    bool outstanding = false;
    // GPUDIFF_OPT_PATH_STRINGS (render_text): cached here and grown on demand, never allocated per batch
    bool strs = false;            // this batch was submitted with the option on
    uint32_t space_idx = 0;       // the space its blobs were written to
    uint32_t* dntab = nullptr;    // K0x: per row, the path-table entry counts of its old and new blob
    uint64_t ntab_cap = 0;
    uint64_t* ps_len = nullptr;   // K15: the strings' lengths
    uint64_t* ps_tiles = nullptr;  // the scan's tile sums
    // the renderers' counters, one block so both totals come back in one 16-byte copy: the values' bytes, the
    // strings' bytes, the strings' unresolved entries (K15 / K16 own [1..2]), the values' unresolved
    unsigned long long* tx_ctr = nullptr;
    uint8_t* ps_out = nullptr;    // offsets[n + 1] | bytes: one D2H
    uint64_t ps_len_cap = 0, ps_tiles_cap = 0, ps_out_cap = 0;
    hipEvent_t ps_ev[4] = {};     // GPUDIFF_OPT_TIMING: K15 + scan begin/end, offsets + K16 begin/end
    bool vals = false;            // GPUDIFF_OPT_PATH_VALUES: this batch was submitted with the option on
    ValBufs vb;
    // gpudiff_store_write_plan_get (dstore_write_plan): what submit and wait keep for it -- the tables' extent and
    // the host-resolved rows' final flags, nothing per event -- and its device buffers, cached and grown on demand
    uint32_t nd = 0;              // staged documents of the batch (TokDoc[nd] at dmeta, DocLink[nd] at links_off)
    uint64_t links_off = 0;
    std::vector<PlanPatch> plan_patch;
    uint8_t* pl_flags = nullptr;  // [nev] final flags
    PlanPatch* pl_patch = nullptr;
    uint8_t* pl_words = nullptr;  // [nd] K17's plan words
    uint64_t* pl_tiles = nullptr;
    uint64_t* pl_rec = nullptr;   // [16]: K17's totals, [8] the bodies' bytes
    uint8_t* pl_head = nullptr;   // offsets | pair_index | src_doc | k10 | kind | noop: the write list as it goes back
    uint32_t* pl_wdoc = nullptr;
    uint64_t* pl_lens = nullptr;
    TokDoc* pl_tdocs = nullptr;   // K10's table, its scratch, arena and results
    TokOut* pl_touts = nullptr;
    uint8_t* pl_scratch = nullptr;
    uint8_t* pl_arena = nullptr;
    uint8_t* pl_bytes = nullptr;  // K19's dense bodies
    BlobMove* pl_mv = nullptr;    // K10's deferrals: the gather list and the gathered JSON
    uint8_t* pl_gather = nullptr;
    uint64_t pl_flags_cap = 0, pl_patch_cap = 0, pl_words_cap = 0, pl_tiles_cap = 0, pl_head_cap = 0, pl_wdoc_cap = 0,
             pl_lens_cap = 0, pl_tdocs_cap = 0, pl_touts_cap = 0, pl_scratch_cap = 0, pl_arena_cap = 0,
             pl_bytes_cap = 0, pl_mv_cap = 0, pl_gather_cap = 0;
    hipEvent_t pl_ev[6] = {};     // GPUDIFF_OPT_TIMING: fold, K10, pack begin/end
};

// gpudiff_host_alloc's pinned buffers: a gpudiff_submit batch laid out in one of them (gpudiff.h) is uploaded
// straight from it, without the staging copy
struct HostBuf {
    gpudiff_ctx* c;
    uint8_t* p;
    uint64_t n;
};
std::mutex g_hb_mu;
std::vector<HostBuf> g_hb;

bool find_host_buf(gpudiff_ctx* c, const void* q, uint8_t** base, uint64_t* size) {
    std::lock_guard<std::mutex> lk(g_hb_mu);
    for (const HostBuf& h : g_hb)
        if (h.c == c && (const uint8_t*)q >= h.p && (const uint8_t*)q < h.p + h.n) {
            *base = h.p;
            *size = h.n;
            return true;
        }
    return false;
}

}  // namespace

struct DStore {
    gpudiff_ctx* c = nullptr;
    uint32_t max_slots = 0, max_events = 0;
    uint64_t space_bytes = 0;
    uint8_t* space[2] = {nullptr, nullptr};
    uint32_t cur = 0;
    unsigned long long* used_dev = nullptr;  // the current space's append point (one of used_base[0..1])
    unsigned long long* used_base = nullptr;
    uint64_t used_ub = 0;  // host upper bound of *used_dev
    // gpudiff_submit's pair mode: ring slot r's batches own space[r] and used_base[r] (each batch starts it
    // empty: the batch two submits back is dropped), so neither a compaction nor its host sync is ever needed
    DSlot* slots = nullptr;
    uint32_t* ctr = nullptr;  // kCtrLive, kCtrLiveBytes
    hipStream_t cs = nullptr;  // H2D of the next batch overlaps K0 of the current one
    // K0 of odd chunks runs on a second stream (its own half of the scratch), so one chunk's launch tail
    // overlaps the next chunk's start instead of idling the CUs between back-to-back launches on one stream
    // (interleaved A/B, profiles/r04ze: one K0 stream 7.44-7.51M pairs/s vs 7.90-8.37M)
    hipStream_t ks = nullptr;
    hipEvent_t ks_ev = nullptr;
    // pair mode with two K0 streams: the whole K0 stage (slot reset, K0 of even chunks, K0c, K0x) runs on ks0 and
    // waits only for what it reuses -- the previous batch's K0x (the shared slot table) and this ring slot's
    // previous diff pass (its space) -- so a batch's K0 overlaps the previous batch's diff pass on the kernel stream
    hipStream_t ks0 = nullptr;
    int last_ring = -1;  // the ring slot of the previous submit
    uint64_t* sizes = nullptr;
    uint64_t* tile_sums = nullptr;
    uint8_t* scratch = nullptr;
    uint64_t scratch_cap = 0;
    Ring ring[2];
    uint32_t ring_next = 0;
    uint32_t batch_seq = 0;
    uint32_t next_wait = 1;  // batches are waited in submit order
    // per slot, one cache line fetch per event: the batch that last staged a document of the slot,
    // that document, and whether the slot was submitted before (its resident version may exist)
    struct SlotState {
        uint32_t stamp;
        int32_t last;
    };
    std::vector<SlotState> sstate;
    std::vector<uint8_t> seen;
    std::unordered_map<uint32_t, uint32_t> forgotten;  // slot -> batch_seq at forget
    // resolution
    std::unique_ptr<PairEncoder> enc;
    gpudiff_dbatch* res_d = nullptr;
    uint8_t* res_stage = nullptr;
    uint64_t res_stage_cap = 0;
    ValBufs res_vb;  // GPUDIFF_OPT_PATH_VALUES: the resolution batch's values
    SlotUpdate* res_ups = nullptr;
    uint64_t res_ups_cap = 0;
    uint32_t* res_err = nullptr;
    bool broken = false;
    bool pair_mode = false;  // gpudiff_submit with GPUDIFF_OPT_DEVICE_ENCODE: slot i = pair i, no state kept
    gpudiff_store_stats st{};
    uint64_t deferred_total = 0;
    gpudiff_store_plan_stats plan_st{};  // the last dstore_write_plan
    // GPUDIFF_OPT_TIMING: per-batch sums (ms) of host submit, H2D, K0, K0c+K0x
    double t_sum[4] = {0, 0, 0, 0};
    double t_sub[5] = {0, 0, 0, 0, 0};  // submit: slot wait, tables, copy, enqueue; finisher
    uint64_t t_n = 0;
};

namespace {

// one staged document: its bytes, then zeros up to `span` (a multiple of 16; dst 16-B aligned), with
// non-temporal 16-B stores -- the pinned staging is only read by the DMA engine, so the stores skip
// the read-for-ownership and do not evict the workers' caches
void stream_doc(uint8_t* dst, const uint8_t* src, size_t len, size_t span) {
    size_t i = 0;
    for (; i + 16 <= len; i += 16)
        _mm_stream_si128((__m128i*)(dst + i), _mm_loadu_si128((const __m128i*)(src + i)));
    if (i < len) {
        alignas(16) uint8_t t[16] = {0};
        memcpy(t, src + i, len - i);
        _mm_stream_si128((__m128i*)(dst + i), _mm_load_si128((const __m128i*)t));
        i += 16;
    }
    const __m128i z = _mm_setzero_si128();
    for (; i < span; i += 16) _mm_stream_si128((__m128i*)(dst + i), z);
}

int grow_pinned(uint8_t** p, uint64_t* cap, uint64_t need) {
    if (need <= *cap) return GPUDIFF_OK;
    if (*p) (void)hipHostFree(*p);
    *p = nullptr;
    *cap = 0;
    const uint64_t n = std::max<uint64_t>(need + need / 4, 1 << 16);
    HIPCHK(hipHostMalloc((void**)p, n, hipHostMallocDefault));
    *cap = n;
    return GPUDIFF_OK;
}

template <class T>
int grow_dev(T** p, uint64_t* cap, uint64_t need) {
    if (need <= *cap) return GPUDIFF_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    const uint64_t n = std::max<uint64_t>(need + need / 4, 256);
    int rc = dalloc(p, n);
    if (rc) return rc;
    *cap = n;
    return GPUDIFF_OK;
}

// packs the live blobs into the other space (stream-ordered), then reads the
// exact append point back
int compact(DStore* s) {
    gpudiff_ctx* c = s->c;
    // GPUDIFF_OPT_PATH_STRINGS / _VALUES: a batch in flight renders its text from the space it was written to; packing
    // into that space would overwrite its superseded blobs first (dstore_submit refuses such a submit before it gets
    // here)
    for (const Ring& R : s->ring)
        if (R.outstanding && (R.strs || R.vals) && R.space_idx == 1 - s->cur) return GPUDIFF_E_STATE;
    HIPCHK(launch_compact_store(c->stream, s->slots, s->max_slots, s->space[s->cur], s->space[1 - s->cur], s->sizes,
                                s->tile_sums, s->used_dev));
    s->cur = 1 - s->cur;
    uint64_t used = 0;
    HIPCHK(hipMemcpyAsync(&used, s->used_dev, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    s->used_ub = used;
    s->st.compactions++;
    return GPUDIFF_OK;
}

// compacts when `want` bytes may not fit; fails only when not even `need` bytes fit after it
int ensure_space(DStore* s, uint64_t want, uint64_t need) {
    if (s->used_ub + want <= s->space_bytes) return GPUDIFF_OK;
    if (s->pair_mode)  // the other space is the other ring slot's batch: no compaction into it
        return s->used_ub + need <= s->space_bytes ? GPUDIFF_OK : GPUDIFF_E_CAPACITY;
    int rc = compact(s);
    if (rc) return rc;
    return s->used_ub + need <= s->space_bytes ? GPUDIFF_OK : GPUDIFF_E_CAPACITY;
}

// ------------------------------------------------------------------ changed paths and values as text
// GPUDIFF_OPT_PATH_STRINGS: K15 + scan + K16 (paths.hip), GPUDIFF_OPT_PATH_VALUES: K21 + scan + K22 (values.hip), over
// a waited batch's changed-path lists, on the readback stream (never behind the next batch's work).  Runs in the
// finisher between collect_results (the counts; the diff pass is done) and resolve(): until then the batch's rows, its
// changed-path lists and both sides' blobs are as the diff pass read them, in the space the batch was written to
// (R.d->pool) -- DESIGN.md "Changed paths as text", "Changed values as text".
//
// Each renderer is two enqueues around one sizing read-back: lengths + the scan's sums, then (the total known, the
// output grown) the offsets + the write and the copy home.  With both options on the two length passes run first and
// both totals come back in one 16-byte copy and one synchronisation.
int paths_len(gpudiff_ctx* c, Ring& R, const PathJob& j, hipStream_t st, bool timing) {
    int rc;
    if ((rc = grow_dev(&R.ps_len, &R.ps_len_cap, j.n_paths)) ||
        (rc = grow_dev(&R.ps_tiles, &R.ps_tiles_cap, scan64_tiles(j.n_paths) + 1)))
        return rc;
    if (timing && !R.ps_ev[0])
        for (auto& e : R.ps_ev) HIPCHK(hipEventCreate(&e));
    if (timing) HIPCHK(hipEventRecord(R.ps_ev[0], st));
    HIPCHK(launch_path_len(st, j, R.ps_len, R.ps_tiles, R.tx_ctr + 1));
    if (timing) HIPCHK(hipEventRecord(R.ps_ev[1], st));
    return GPUDIFF_OK;
}

int paths_write(Ring& R, const PathJob& j, uint64_t total, hipStream_t st, bool timing, PathStrs& ps) {
    int rc;
    const uint64_t head = 8ull * ((uint64_t)j.n_paths + 1);
    if ((rc = grow_dev(&R.ps_out, &R.ps_out_cap, head + total + 8))) return rc;
    if (timing) HIPCHK(hipEventRecord(R.ps_ev[2], st));
    HIPCHK(launch_path_write(st, j, R.ps_len, R.ps_tiles, (uint64_t*)R.ps_out, R.ps_out + head, total, R.tx_ctr + 1));
    if (timing) HIPCHK(hipEventRecord(R.ps_ev[3], st));
    try {
        ps.words.assign((size_t)j.n_paths + 1 + (size_t)((total + 7) / 8), 0);
    } catch (const std::bad_alloc&) {
        return GPUDIFF_E_NOMEM;
    }
    HIPCHK(hipMemcpyAsync(ps.words.data(), R.ps_out, head + total, hipMemcpyDeviceToHost, st));
    return GPUDIFF_OK;
}

// kernel time of one renderer's two event pairs into its stats
int add_kernel_ms(const hipEvent_t* ev, gpudiff_path_stats& st) {
    float a = 0, b = 0;
    HIPCHK(hipEventElapsedTime(&a, ev[0], ev[1]));
    HIPCHK(hipEventElapsedTime(&b, ev[2], ev[3]));
    st.kernel_ms += (double)a + b;
    return GPUDIFF_OK;
}

// the values' buffers: out of device memory is GPUDIFF_E_CAPACITY
template <class T>
int grow_val(T** p, uint64_t* cap, uint64_t need) {
    if (grow_dev(p, cap, need) == GPUDIFF_OK) return GPUDIFF_OK;
    (void)hipGetLastError();
    return GPUDIFF_E_CAPACITY;
}

int values_len(ValBufs& B, const ValueJob& j, hipStream_t st, bool timing, unsigned long long* total,
               unsigned long long* unresolved) {
    int rc;
    const uint64_t n2 = 2ull * j.n_paths;
    if ((rc = grow_val(&B.len, &B.len_cap, n2)) ||
        (rc = grow_val(&B.tiles, &B.tiles_cap, scan64_tiles((uint32_t)n2) + 1)) ||
        (rc = grow_val(&B.slots, &B.slots_cap, n2)) || (rc = grow_val(&B.tags, &B.tags_cap, n2)))
        return rc;
    if (timing && !B.ev[0])
        for (auto& e : B.ev) HIPCHK(hipEventCreate(&e));
    if (timing) HIPCHK(hipEventRecord(B.ev[0], st));
    HIPCHK(launch_value_len(st, j, B.tags, B.len, B.slots, B.tiles, total, unresolved));
    if (timing) HIPCHK(hipEventRecord(B.ev[1], st));
    return GPUDIFF_OK;
}

int values_write(ValBufs& B, const ValueJob& j, uint64_t total, hipStream_t st, bool timing,
                 unsigned long long* unresolved, PathVals& pv) {
    int rc;
    const uint64_t n2 = 2ull * j.n_paths, head = 8ull * (n2 + 1 + PathVals::tag_words(j.n_paths));
    if ((rc = grow_val(&B.out, &B.out_cap, head + total + 8))) return rc;
    if (timing) HIPCHK(hipEventRecord(B.ev[2], st));
    HIPCHK(hipMemsetAsync(B.out + 8ull * (n2 + 1), 0, 8ull * PathVals::tag_words(j.n_paths), st));
    HIPCHK(hipMemcpyAsync(B.out + 8ull * (n2 + 1), B.tags, n2, hipMemcpyDeviceToDevice, st));
    HIPCHK(launch_value_write(st, j, B.tags, B.len, B.slots, B.tiles, (uint64_t*)B.out, B.out + head, total,
                              unresolved));
    if (timing) HIPCHK(hipEventRecord(B.ev[3], st));
    try {
        pv.words.assign((size_t)(head / 8) + (size_t)((total + 7) / 8), 0);
    } catch (const std::bad_alloc&) {
        return GPUDIFF_E_NOMEM;
    }
    HIPCHK(hipMemcpyAsync(pv.words.data(), B.out, head + total, hipMemcpyDeviceToHost, st));
    return GPUDIFF_OK;
}

ValueJob value_job(const gpudiff_ctx* c, const gpudiff_dbatch* d, size_t n_dirty, uint32_t n) {
    return ValueJob{d->rows, d->dirty_idx, d->path_off, d->out_h, d->out_k, d->pool, d->pool_cap, c->hash_mask,
                    (uint32_t)n_dirty, n};
}

int render_text(DStore* s, Ring& R, ResultStore& rs) {
    gpudiff_ctx* c = s->c;
    gpudiff_dbatch* d = R.d;
    PathStrs& ps = rs.ps;
    PathVals& pv = rs.pv;
    const size_t np = rs.hashes.size();
    if (R.strs) {
        ps.on = true;
        ps.n = np;
        ps.words.assign(1, 0);
        c->path_stats.batches++;
    }
    if (R.vals) {
        pv.on = true;
        pv.n = np;
        pv.words.assign(1, 0);
        c->value_stats.batches++;
    }
    if (!np) return GPUDIFF_OK;
    if (np > 0x7FFFFFFFull) return GPUDIFF_E_CAPACITY;
    int rc;
    const uint32_t n = (uint32_t)np;
    if (!R.tx_ctr && (rc = dalloc(&R.tx_ctr, 4))) return rc;
    const bool timing = (c->flags & GPUDIFF_OPT_TIMING) != 0;
    const PathJob j{d->rows,     R.dntab,      d->dirty_idx,  d->path_off,           d->out_h, d->out_k,
                    d->pool,     d->pool_cap,  c->hash_mask,  (uint32_t)rs.dirty.size(), n};
    const ValueJob vj = value_job(c, d, rs.dirty.size(), n);
    hipStream_t st = c->rb;
    unsigned long long ctr[4] = {0, 0, 0, 0};
    if (R.strs && (rc = paths_len(c, R, j, st, timing))) return rc;
    if (R.vals && (rc = values_len(R.vb, vj, st, timing, R.tx_ctr, R.tx_ctr + 3))) return rc;
    HIPCHK(hipMemcpyAsync(ctr, R.tx_ctr, 16, hipMemcpyDeviceToHost, st));  // the bytes to make room for, both kinds
    HIPCHK(hipStreamSynchronize(st));
    c->render_syncs++;
    const uint64_t vtotal = R.vals ? ctr[0] : 0, ptotal = R.strs ? ctr[1] : 0;
    if (R.strs && (rc = paths_write(R, j, ptotal, st, timing, ps))) return rc;
    if (R.vals && (rc = values_write(R.vb, vj, vtotal, st, timing, R.tx_ctr + 3, pv))) return rc;
    HIPCHK(hipMemcpyAsync(ctr, R.tx_ctr, 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    c->render_syncs++;
    if (R.strs) {
        ps.n_unresolved = (size_t)ctr[2];
        if (ps.words[n] != ptotal) return GPUDIFF_E_DEVICE;  // the offsets the strings were written by
        if (timing) {
            if ((rc = add_kernel_ms(R.ps_ev, c->path_stats))) return rc;
            c->path_stats.timed_batches++;
        }
    }
    if (R.vals) {
        pv.n_unresolved = (size_t)ctr[3];
        if (pv.words[2 * (size_t)n] != vtotal) return GPUDIFF_E_DEVICE;
        if (timing) {
            if ((rc = add_kernel_ms(R.vb.ev, c->value_stats))) return rc;
            c->value_stats.timed_batches++;
        }
    }
    return GPUDIFF_OK;
}

// The resolution batch's values (place_and_diff): the same two kernels over s->res_d, whose blobs -- host-written,
// or a slot's resident one -- are all in HBM.
int render_values_resolved(DStore* s, const ResultStore& r2, PathVals& pv) {
    gpudiff_ctx* c = s->c;
    ValBufs& B = s->res_vb;
    const size_t np = r2.hashes.size();
    pv.on = true;
    pv.n = np;
    pv.words.assign(1, 0);
    if (!np) return GPUDIFF_OK;
    if (np > 0x7FFFFFFFull) return GPUDIFF_E_CAPACITY;
    int rc;
    if (!B.ctr && (rc = dalloc(&B.ctr, 2))) return rc;
    const bool timing = (c->flags & GPUDIFF_OPT_TIMING) != 0;
    const ValueJob vj = value_job(c, s->res_d, r2.dirty.size(), (uint32_t)np);
    hipStream_t st = c->rb;
    unsigned long long ctr[2] = {0, 0};
    if ((rc = values_len(B, vj, st, timing, B.ctr, B.ctr + 1))) return rc;
    HIPCHK(hipMemcpyAsync(ctr, B.ctr, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    c->render_syncs++;
    const uint64_t total = ctr[0];
    if ((rc = values_write(B, vj, total, st, timing, B.ctr + 1, pv))) return rc;
    HIPCHK(hipMemcpyAsync(ctr, B.ctr, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    c->render_syncs++;
    pv.n_unresolved = (size_t)ctr[1];
    if (pv.words[2 * np] != total) return GPUDIFF_E_DEVICE;
    if (timing && (rc = add_kernel_ms(B.ev, c->value_stats))) return rc;
    return GPUDIFF_OK;
}

// The host resolution's side of it: what renders a deferred event's changed paths once its diff is known -- per
// side, the flattened object's leaves (hash -> path bytes, as hashed under the pair's final seed) or, for a
// resident old side, its path table.
struct HostSide {
    struct Leaf {
        uint64_t h;
        uint32_t off, len;
    };
    std::vector<Leaf> spec, stat;  // ascending by h
    std::string paths;
    PathTable tab;  // a resident blob's (load_tab), walked by pathstr.h
    uint32_t seed = 0;
    bool flat = false, table = false;
    void of_flat(const FlatObject& o) {
        flat = true;
        table = false;
        paths = o.paths;
        spec.clear();
        stat.clear();
        for (const LeafRec& r : o.spec) spec.push_back(Leaf{r.h, r.path_off, r.path_len});
        for (const LeafRec& r : o.stat) stat.push_back(Leaf{r.h, r.path_off, r.path_len});
    }
    void of_table(const PathTable& t, uint32_t sd) {
        flat = false;
        table = true;
        tab = t;
        seed = sd;
    }
    bool render(uint64_t h, bool status, uint64_t mask, std::string& out) const {
        out.clear();
        if (flat) {
            const std::vector<Leaf>& v = status ? stat : spec;
            auto it = std::lower_bound(v.begin(), v.end(), h, [](const Leaf& l, uint64_t x) { return l.h < x; });
            if (it == v.end() || it->h != h) return false;
            out = render_path(paths.data() + it->off, it->len);
            return true;
        }
        if (!table || tab.n == GPUDIFF_TAB_NONE) return false;
        const PathTab t = path_tab(tab.data.data(), tab.n, tab.data.size());
        const uint64_t root = (uint64_t)seed & mask, len = path_text_len(t, root, h);
        if (len == kPathUnresolved) return false;
        out.resize(len);
        return path_text_write(t, root, h, (uint8_t*)&out[0], len);
    }
};
struct HostPaths {
    HostSide a, b;
};

// entry q of `r`'s changed paths (a deferred event's, diffed from host-encoded blobs) as text
void host_path(const HostPaths& hp, const ResultStore& r, uint32_t q, uint64_t mask, PathStrs& out) {
    const uint8_t k = r.kinds[q];
    std::string s;
    bool ok = true;
    if ((k & 3u) == GPUDIFF_PATH_STATUS_ABSENT) s = "status";
    else ok = ((k & 3u) == GPUDIFF_PATH_REMOVED ? hp.a : hp.b).render(r.hashes[q], (k & GPUDIFF_PATH_REGION_STATUS) != 0,
                                                                     mask, s);
    if (!ok) {
        s.clear();
        out.n_unresolved++;
    }
    out.push(s.data(), s.size());
    out.n_host++;
}

// ------------------------------------------------------------------ host resolution
// a slot as the resolution sees it: the device's entry as fetched, then as the batch's deferred events leave it
// (d.off: absolute, or kRelTag | offset in the resolution pool), and its path table once a decision has read it
struct HostSlot {
    DStore* s = nullptr;  // set once fetched
    DSlot d{};
    bool tab_loaded = false;
    PathTable tab;
    bool live() const { return d.flags & DS_LIVE; }
    uint32_t seed() const { return (d.flags >> 8) & 0xFF; }
    void empty() {
        d.flags &= ~DS_LIVE;
        tab_loaded = false;
    }
};

int fetch_slot(DStore* s, uint32_t slot, HostSlot& H) {
    HIPCHK(hipMemcpy(&H.d, s->slots + slot, sizeof(DSlot), hipMemcpyDeviceToHost));
    H.s = s;
    H.tab_loaded = false;
    return GPUDIFF_OK;
}

// the path table of a device-resident blob, its trailer, fetched when store_decide first reads it (ResidentTabFn)
int load_tab(void* slot, const PathTable** out) {
    HostSlot& H = *(HostSlot*)slot;
    *out = &H.tab;
    if (H.tab_loaded) return GPUDIFF_OK;
    const uint64_t segs = gpudiff_blob_body(H.d.spec_l, H.d.spec_ar, H.d.stat_l, H.d.stat_ar);  // the table follows
    H.tab.n = H.d.n_tab;
    H.tab.data.resize(H.d.bytes - segs);
    if (!H.tab.data.empty())
        HIPCHK(hipMemcpy(H.tab.data.data(), H.s->space[H.s->cur] + H.d.off + segs, H.tab.data.size(),
                         hipMemcpyDeviceToHost));
    H.tab_loaded = true;
    return GPUDIFF_OK;
}

// The working set of one batch's host resolution: its deferred events, their re-encoded blobs and rows, and the
// slots they touch.
struct Deferred {
    std::vector<uint8_t> def;     // per event of the batch: K0 deferred it
    std::vector<uint32_t> drows;  // the deferred events, ascending
    std::vector<uint8_t> pool;    // their blobs, placed behind the append point
    std::vector<gpudiff_pair_row> rows;  // [drows.size()]
    // GPUDIFF_OPT_PATH_STRINGS: these events' strings come from the objects flattened here (their blobs carry no
    // table in pair mode, the re-encoded old side none in store mode)
    bool strs = false;
    bool vals = false;  // GPUDIFF_OPT_PATH_VALUES: place_and_diff renders the resolution batch's values
    std::vector<HostPaths> hp;  // [drows.size()], or empty
    std::unordered_map<uint32_t, HostSlot> hs;
    std::vector<uint32_t> touched;  // hs's slots in first-touch order
    Arena arena_new, arena_old;
    FlatObject fn, fo;
};

gpudiff_pair_row& deferred_row(Deferred& W, size_t k, const gpudiff_event& e) {
    gpudiff_pair_row& r = W.rows[k];
    memset(&r, 0, sizeof(r));
    r.pair_id = e.pair_id;
    r.cluster_id = e.cluster_id;
    return r;
}

// pair mode: gpudiff_encode_pairs' decisions on (old_json, new_json)
void encode_deferred_pair(PairEncoder& enc, const gpudiff_event& e, Deferred& W, size_t k) {
    gpudiff_pair_row& r = deferred_row(W, k, e);
    uint32_t seed = 0;
    if (!(e.old_json && enc.flatten_json(e.old_json, e.old_len, W.arena_old, W.fo) &&
          enc.flatten_json(e.new_json, e.new_len, W.arena_new, W.fn) && enc.pair_seed(W.fo, W.fn, &seed))) {
        r.flags_a = r.flags_b = GPUDIFF_OBJ_DECODE_ERR;
        return;
    }
    uint64_t oa, ob;
    enc.write_object(W.fo, W.pool, &oa, &r.spec_l_a, &r.spec_ar_a, &r.stat_l_a, &r.stat_ar_a);
    enc.write_object(W.fn, W.pool, &ob, &r.spec_l_b, &r.spec_ar_b, &r.stat_l_b, &r.stat_ar_b);
    r.off_a = kRelTag | oa;
    r.off_b = kRelTag | ob;
    r.flags_a = (W.fo.flags & GPUDIFF_OBJ_HAS_STATUS) | (seed << GPUDIFF_OBJ_SEED_SHIFT);
    r.flags_b = (W.fn.flags & GPUDIFF_OBJ_HAS_STATUS) | (seed << GPUDIFF_OBJ_SEED_SHIFT);
    if (W.strs) {
        W.hp[k].a.of_flat(W.fo);
        W.hp[k].b.of_flat(W.fn);
    }
}

// store mode: the host store's decision for the event (store_decide), its blobs into W.pool with offsets relative
// to the placement, and the slot's state after it
int encode_deferred_store(DStore* s, const gpudiff_event& e, Deferred& W, size_t k) {
    PairEncoder& enc = *s->enc;
    HostSlot& S = W.hs[e.slot];
    if (!S.s) {
        if (int rc = fetch_slot(s, e.slot, S)) return rc;
        W.touched.push_back(e.slot);
    }
    gpudiff_pair_row& r = deferred_row(W, k, e);
    const StoreDecision D = enc.store_decide(S.live(), S.seed(), load_tab, &S, e.old_json, e.old_len, e.new_json,
                                             e.new_len, W.arena_old, W.arena_new, W.fo, W.fn);
    if (D.rc) return D.rc;
    s->st.old_encoded += D.old_encoded;
    s->st.reseeded += D.reseeded;
    s->st.collisions_unresolved += D.unresolved;
    const bool pair_error = D.rung == StoreRung::kPairError;
    if (pair_error) r.flags_a = r.flags_b = GPUDIFF_OBJ_DECODE_ERR;  // conservative
    if (!D.store_ok) {
        S.empty();
        return GPUDIFF_OK;
    }
    if (D.rung == StoreRung::kResidentSeed0 || D.rung == StoreRung::kResidentSlotSeed) {
        // the slot's blob as it is when k_place runs (a compaction may move it)
        r.off_a = (S.d.off & kRelTag) ? S.d.off : (kSlotTag | e.slot);
        r.spec_l_a = S.d.spec_l;
        r.spec_ar_a = S.d.spec_ar;
        r.stat_l_a = S.d.stat_l;
        r.stat_ar_a = S.d.stat_ar;
        r.flags_a = ((S.d.flags & DS_HAS_STATUS) ? GPUDIFF_OBJ_HAS_STATUS : 0u) | (D.seed << GPUDIFF_OBJ_SEED_SHIFT);
        if (W.strs) W.hp[k].a.of_table(S.tab, S.seed());  // the table load_tab fetched (or the previous event's)
    } else if (D.rung == StoreRung::kReencodedOld) {
        uint64_t off;
        enc.write_object(W.fo, W.pool, &off, &r.spec_l_a, &r.spec_ar_a, &r.stat_l_a, &r.stat_ar_a);
        r.off_a = kRelTag | off;
        r.flags_a = (W.fo.flags & GPUDIFF_OBJ_HAS_STATUS) | (D.seed << GPUDIFF_OBJ_SEED_SHIFT);
        if (W.strs) W.hp[k].a.of_flat(W.fo);
    } else if (!pair_error) {  // first sighting: no old side
        r.flags_a = D.seed << GPUDIFF_OBJ_SEED_SHIFT;
    }
    uint64_t off;
    uint32_t sl, sar, tl, tar, bytes;
    enc.write_object_tab(W.fn, W.pool, &off, &sl, &sar, &tl, &tar, &bytes);
    if (!pair_error) {
        if (W.strs) W.hp[k].b.of_flat(W.fn);
        r.off_b = kRelTag | off;
        r.spec_l_b = sl;
        r.spec_ar_b = sar;
        r.stat_l_b = tl;
        r.stat_ar_b = tar;
        r.flags_b = (W.fn.flags & GPUDIFF_OBJ_HAS_STATUS) | (D.seed << GPUDIFF_OBJ_SEED_SHIFT);
    }
    const uint32_t has_status = (W.fn.flags & GPUDIFF_OBJ_HAS_STATUS) ? DS_HAS_STATUS : 0u;
    S.d = DSlot{kRelTag | off, sl, sar, tl, tar, bytes, DS_LIVE | has_status | (D.seed << 8), 0, W.fn.tab.n};
    S.tab = W.fn.tab;
    S.tab_loaded = true;
    return GPUDIFF_OK;
}

// the touched slots' states for k_place (forgotten-since slots keep their forget)
std::vector<SlotUpdate> slot_updates(DStore* s, const Ring& R, const Deferred& W) {
    std::vector<SlotUpdate> ups;
    for (uint32_t slot : W.touched) {
        auto f = s->forgotten.find(slot);
        if (f != s->forgotten.end() && f->second >= R.batch) continue;
        const HostSlot& S = W.hs.at(slot);
        SlotUpdate u{};
        u.slot = slot;
        u.batch = R.batch;
        if (S.live()) u.entry = S.d;  // as its last deferred event wrote it
        else s->seen[slot] = 0;       // the next event stages its old object again
        ups.push_back(u);
    }
    return ups;
}

// the slot states on the device, and k_place's error word cleared: what both placements start with
int upload_slot_updates(DStore* s, const std::vector<SlotUpdate>& ups) {
    if (int rc = grow_dev(&s->res_ups, &s->res_ups_cap, std::max<size_t>(ups.size(), 1))) return rc;
    if (!ups.empty()) HIPCHK(hipMemcpy(s->res_ups, ups.data(), ups.size() * sizeof(SlotUpdate), hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(s->res_err, 0, 4, s->c->stream));
    return GPUDIFF_OK;
}

// The space cannot take the re-encoded blobs even after a compaction (K0 deferred these events for lack of space,
// and the host's blobs do not fit either).  The store stays usable: the events are reported dirty with
// GPUDIFF_DECODE_ERROR (the reference's conservative rule, specsyncer.go:20-22: never "equal") and their slots are
// emptied, so each slot's next event stages its old object again.
int place_conservative(DStore* s, std::vector<SlotUpdate>& ups, size_t n_deferred) {
    for (SlotUpdate& u : ups) {
        memset(&u.entry, 0, sizeof(u.entry));
        s->seen[u.slot] = 0;
    }
    if (int rc = upload_slot_updates(s, ups)) return rc;
    HIPCHK(launch_place(s->c->stream, nullptr, 0, s->space[s->cur], s->used_dev, s->space_bytes, nullptr, nullptr, 0,
                        s->res_ups, (uint32_t)ups.size(), s->slots, s->ctr, s->res_err));
    HIPCHK(hipStreamSynchronize(s->c->stream));
    s->st.space_conservative += n_deferred;
    return GPUDIFF_OK;
}

// place: blobs behind the append point, rows, slot states; then the diff pass over the placed rows into r2
int place_and_diff(DStore* s, const Deferred& W, const std::vector<SlotUpdate>& ups, ResultStore& r2) {
    gpudiff_ctx* c = s->c;
    const uint64_t pbytes = W.pool.size();
    const size_t nr = W.rows.size();
    int rc;
    if ((rc = grow_dev(&s->res_stage, &s->res_stage_cap, std::max<uint64_t>(pbytes, 16)))) return rc;
    gpudiff_dbatch* d = s->res_d;
    if (d->max_pairs < nr) {
        gpudiff_dbatch_free(c, d);
        s->res_d = nullptr;
        if ((rc = gpudiff_dbatch_create(c, 16, nr + nr / 2, &s->res_d))) return rc;
        d = s->res_d;
        (void)hipFree(d->pool);
        d->pool = nullptr;
        d->pool_borrowed = true;
    }
    if (pbytes) HIPCHK(hipMemcpy(s->res_stage, W.pool.data(), pbytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d->rows, W.rows.data(), nr * sizeof(gpudiff_pair_row), hipMemcpyHostToDevice));
    if ((rc = upload_slot_updates(s, ups))) return rc;
    HIPCHK(launch_place(c->stream, s->res_stage, pbytes, s->space[s->cur], s->used_dev, s->space_bytes, d->rows,
                        d->pair_ids, (uint32_t)nr, s->res_ups, (uint32_t)ups.size(), s->slots, s->ctr, s->res_err));
    s->used_ub += pbytes;
    d->pool = s->space[s->cur];
    d->pool_cap = s->space_bytes;
    d->n_pairs = nr;
    d->rows_gen++;
    gpudiff_ticket t2;
    if ((rc = gpudiff_diff(c, d, &t2))) return rc;
    if ((rc = collect_results(c, d, r2))) return rc;
    c->tickets.erase(t2);
    d->ticket = 0;
    // the values of these events' changed leaves: the rows k_place wrote name blobs that are all in HBM
    if (W.vals && (rc = render_values_resolved(s, r2, r2.pv))) return rc;
    uint32_t err = 0;
    HIPCHK(hipMemcpy(&err, s->res_err, 4, hipMemcpyDeviceToHost));
    return err ? GPUDIFF_E_CAPACITY : GPUDIFF_OK;
}

// patch: deferred events take r2's results (r2 null, the conservative exit: each is dirty in both regions with
// GPUDIFF_DECODE_ERROR and no paths), the rest keep rs's
void merge_results(const Ring& R, const Deferred& W, ResultStore& rs, const ResultStore* r2, uint64_t mask) {
    constexpr uint8_t kDirty = GPUDIFF_SPEC_DIRTY | GPUDIFF_STATUS_DIRTY;
    ResultStore out;
    out.flags.resize(R.nev);
    out.off.push_back(0);
    if (W.strs) {
        out.ps.on = true;
        out.ps.n_unresolved = rs.ps.n_unresolved;
        out.ps.begin();
    }
    if (W.vals) {
        out.pv.on = true;
        out.pv.n_unresolved = rs.pv.n_unresolved + (r2 ? r2->pv.n_unresolved : 0);
        out.pv.begin();
    }
    size_t jr = 0, j2 = 0, k = 0;
    for (uint32_t i = 0; i < R.nev; i++) {
        uint8_t f = rs.flags[i];
        uint32_t lo = 0, hi = 0;
        const ResultStore* src = &rs;
        if (f & kDirty) {
            lo = rs.off[jr];
            hi = rs.off[jr + 1];
            jr++;
        }
        const size_t kd = k;  // the deferred event's index (rows, hp)
        if (W.def[i]) {
            k++;
            lo = hi = 0;
            f = r2 ? r2->flags[kd] : (uint8_t)(kDirty | GPUDIFF_DECODE_ERROR);
            if (r2 && (f & kDirty)) {
                src = r2;
                lo = r2->off[j2];
                hi = r2->off[j2 + 1];
                j2++;
            }
        }
        out.flags[i] = f;
        const uint32_t pid = R.events[i].pair_id;
        if (f & GPUDIFF_SPEC_DIRTY) out.spec.push_back(pid);
        if (f & GPUDIFF_STATUS_DIRTY) out.status.push_back(pid);
        if (!(f & kDirty)) continue;
        out.dirty.push_back(pid);
        for (uint32_t q = lo; q < hi; q++) {
            out.hashes.push_back(src->hashes[q]);
            out.kinds.push_back(src->kinds[q]);
            if (W.vals) {  // both branches carry what the device rendered: the batch's pass, or the resolution's
                const PathVals& v = src->pv;
                for (size_t t = 2 * (size_t)q; t < 2 * (size_t)q + 2; t++)
                    out.pv.push(v.tags()[t], v.bytes() + v.offsets()[t], v.offsets()[t + 1] - v.offsets()[t]);
                if (src == r2) out.pv.n_host++;
            }
            if (!W.strs) continue;
            if (src == r2) host_path(W.hp[kd], *r2, q, mask, out.ps);
            else out.ps.push(rs.ps.bytes() + rs.ps.offsets()[q], rs.ps.offsets()[q + 1] - rs.ps.offsets()[q]);
        }
        out.off.push_back((uint32_t)out.hashes.size());
    }
    if (W.strs) out.ps.finish();
    if (W.vals) out.pv.finish();
    rs = std::move(out);
}

// Re-does the batch's deferred events on the host, diffs them on the device and patches rs.
int resolve(DStore* s, Ring& R, ResultStore& rs) {
    gpudiff_ctx* c = s->c;
    HIPCHK(hipStreamSynchronize(c->stream));
    Deferred W;
    W.def.resize(R.nev);
    if (R.nev) HIPCHK(hipMemcpy(W.def.data(), R.ddef, R.nev, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < R.nev; i++)
        if (W.def[i]) W.drows.push_back(i);
    if (W.drows.empty()) return GPUDIFF_OK;
    s->deferred_total += W.drows.size();
    W.rows.resize(W.drows.size());
    W.strs = rs.ps.on;
    W.vals = rs.pv.on;
    W.hp.resize(W.strs ? W.drows.size() : 0);
    int rc;
    for (size_t k = 0; k < W.drows.size(); k++) {
        const gpudiff_event& e = R.events[W.drows[k]];
        if (s->pair_mode) encode_deferred_pair(*s->enc, e, W, k);
        else if ((rc = encode_deferred_store(s, e, W, k))) return rc;
    }
    std::vector<SlotUpdate> ups = slot_updates(s, R, W);
    const uint64_t pbytes = (W.pool.size() + GPUDIFF_BLOB_ALIGN - 1) & ~(uint64_t)(GPUDIFF_BLOB_ALIGN - 1);
    W.pool.resize(pbytes, 0);
    ResultStore r2;
    const bool fits = !(rc = ensure_space(s, pbytes, pbytes));
    if (!fits && rc != GPUDIFF_E_CAPACITY) return rc;
    if ((rc = fits ? place_and_diff(s, W, ups, r2) : place_conservative(s, ups, W.drows.size()))) return rc;
    merge_results(R, W, rs, fits ? &r2 : nullptr, c->hash_mask);
    // the write plan reads the batch's flags in HBM, where these rows are still the conservative ones K0x wrote
    for (uint32_t row : W.drows) R.plan_patch.push_back(PlanPatch{row, rs.flags[row]});
    return GPUDIFF_OK;
}

}  // namespace

// ------------------------------------------------------------------ API
DStore* dstore_create(gpudiff_ctx* c, uint32_t max_slots, uint64_t space_bytes, uint32_t max_events, int* rc_out) {
    std::unique_ptr<DStore> s(new (std::nothrow) DStore());
    int rc = GPUDIFF_E_NOMEM;
    if (!s) {
        *rc_out = rc;
        return nullptr;
    }
    s->c = c;
    s->max_slots = max_slots;
    s->max_events = max_events;
    s->space_bytes = (space_bytes + 15) & ~15ull;
    auto fail = [&](int e) {
        dstore_free(c, s.release());
        *rc_out = e;
        return (DStore*)nullptr;
    };
    try {
        s->sstate.assign(max_slots, DStore::SlotState{0u, -1});
        s->seen.assign(max_slots, 0);
    } catch (const std::bad_alloc&) {
        return fail(GPUDIFF_E_NOMEM);
    }
    EncodeConfig cfg = c->ecfg;
    s->enc.reset(new (std::nothrow) PairEncoder(cfg));
    if (!s->enc) return fail(GPUDIFF_E_NOMEM);
    for (auto& sp : s->space)
        if ((rc = dalloc(&sp, s->space_bytes))) return fail(rc);
    if ((rc = dalloc(&s->used_base, 2)) || (rc = dalloc(&s->slots, max_slots)) || (rc = dalloc(&s->ctr, 4)) ||
        (rc = dalloc(&s->sizes, max_slots)) || (rc = dalloc(&s->tile_sums, scan64_tiles(max_slots) + 1)) ||
        (rc = dalloc(&s->res_err, 1)))
        return fail(rc);
    s->used_dev = s->used_base;
    if (hipMemset(s->used_base, 0, 16) != hipSuccess || hipMemset(s->slots, 0, sizeof(DSlot) * (size_t)max_slots) ||
        hipMemset(s->ctr, 0, 16) != hipSuccess)
        return fail(GPUDIFF_E_DEVICE);
    for (Ring& R : s->ring) {
        if ((rc = gpudiff_dbatch_create(c, 16, max_events, &R.d))) return fail(rc);
        (void)hipFree(R.d->pool);
        R.d->pool = nullptr;
        R.d->pool_borrowed = true;
        R.d->host_resolves = true;
        if ((rc = dalloc(&R.dcnt, 1))) return fail(rc);
        if (hipEventCreateWithFlags(&R.staged, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&R.k0_done, hipEventDisableTiming) != hipSuccess)
            return fail(GPUDIFF_E_DEVICE);
    }
    if (hipStreamCreateWithFlags(&s->cs, hipStreamNonBlocking) != hipSuccess) return fail(GPUDIFF_E_DEVICE);
    // the pair-mode K0 stage on its own stream (interleaved A/B, profiles/r04zf: on the kernel stream 7.71-7.79M
    // pairs/s staged vs 7.90-8.37M)
    if (hipStreamCreateWithFlags(&s->ks, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&s->ks_ev, hipEventDisableTiming) != hipSuccess ||
        hipStreamCreateWithFlags(&s->ks0, hipStreamNonBlocking) != hipSuccess)
        return fail(GPUDIFF_E_DEVICE);
    for (Ring& R : s->ring)
        if (hipEventCreateWithFlags(&R.pass_done, hipEventDisableTiming) != hipSuccess) return fail(GPUDIFF_E_DEVICE);
    if ((rc = gpudiff_dbatch_create(c, 16, 1024, &s->res_d))) return fail(rc);
    (void)hipFree(s->res_d->pool);
    s->res_d->pool = nullptr;
    s->res_d->pool_borrowed = true;
    s->st.max_slots = max_slots;
    s->st.space_bytes = s->space_bytes;
    *rc_out = GPUDIFF_OK;
    return s.release();
}

// ------------------------------------------------------------------ submit
namespace {

// GPUDIFF_OPT_TIMING: the submit's host phases, t_sub[k] += the time since the previous lap
struct Lap {
    bool on;
    double* t_sub;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void operator()(int k) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        t_sub[k] += std::chrono::duration<double, std::milli>(now - t).count();
        t = now;
    }
};

// The host-side description of one batch: the document table, the slot chains and their heads (in R.hmeta, laid
// out for 2n documents), where each document's bytes are, and the sums the later phases size things by.
struct BatchTables {
    TokDoc* docs = nullptr;
    DocLink* links = nullptr;
    uint32_t* heads = nullptr;
    uint64_t max_docs = 0, meta_bytes = 0;
    std::vector<const uint8_t*> src;  // per document, the caller's bytes
    uint32_t nd = 0, nh = 0;
    uint64_t jbytes = 0;              // the staged JSON (build_tables adds the trailing kTokSlack last)
    uint64_t bound = 0, floor = 0;    // the blobs' estimate that triggers compaction, and the least they take
    uint64_t new_json_bytes = 0;
    const uint8_t* zsrc = nullptr;    // zero copy: the caller's pinned buffer holds the staged layout (offset 0 here)
    uint64_t links_off() const { return max_docs * sizeof(TokDoc); }
    uint64_t heads_off() const { return max_docs * (sizeof(TokDoc) + sizeof(DocLink)); }
};

// GPUDIFF_OPT_PATH_STRINGS in store mode: the batch in flight renders its paths, at its gpudiff_wait, from the
// space it was written to.  If a compaction has since left it behind in the other space, the next compaction packs
// into that space: a submit that may need one is refused before it changes anything (wait on the outstanding
// ticket first).
bool refuse_if_strings_need_compaction(const DStore* s, const gpudiff_event* ev, size_t n) {
    if (s->pair_mode || !(s->c->flags & (GPUDIFF_OPT_PATH_STRINGS | GPUDIFF_OPT_PATH_VALUES))) return false;
    const Ring& O = s->ring[s->ring_next ^ 1u];
    if (!(O.outstanding && (O.strs || O.vals) && O.space_idx != s->cur)) return false;
    uint64_t pre = 0;  // >= the bound ensure_space is asked for
    for (size_t i = 0; i < n; i++)
        pre += (5 * ((uint64_t)ev[i].new_len + (ev[i].old_json ? ev[i].old_len : 0))) / 2 + 768;
    return s->used_ub + pre > s->space_bytes;
}

// The ring slot this submit takes, with its pinned buffers reusable.  dec: the K0 stage runs on its own streams
// (it resets the space's append point there).
int claim_ring_slot(DStore* s, bool dec, Ring** out) {
    gpudiff_ctx* c = s->c;
    Ring& R = s->ring[s->ring_next];
    if (R.outstanding) {
        if (!s->pair_mode) return GPUDIFF_E_STATE;  // wait on the batch two submits back first
        // pair mode keeps gpudiff_submit's ring rule: the ticket two submits back is dropped
        c->finishers.erase(R.ticket);
        R.outstanding = false;
    }
    if (R.staged) HIPCHK(hipEventSynchronize(R.staged));
    if (s->pair_mode) {  // this ring slot's space, emptied behind its previous batch (stream order)
        s->cur = s->ring_next;
        s->used_dev = s->used_base + s->ring_next;
        s->used_ub = 0;
        if (!dec) HIPCHK(hipMemsetAsync(s->used_dev, 0, 8, c->stream));  // (dec: on ks0, in stage_and_encode)
    }
    *out = &R;
    return GPUDIFF_OK;
}

int map_tables(Ring& R, size_t n, BatchTables& B) {
    B.max_docs = 2 * (uint64_t)n;
    B.meta_bytes = B.max_docs * (sizeof(TokDoc) + sizeof(DocLink)) + 4 * (uint64_t)n + 64;
    if (int rc = grow_pinned(&R.hmeta, &R.hmeta_cap, B.meta_bytes)) return rc;
    B.docs = (TokDoc*)R.hmeta;
    B.links = (DocLink*)(R.hmeta + B.links_off());
    B.heads = (uint32_t*)(R.hmeta + B.heads_off());
    B.src.reserve(B.max_docs);
    return GPUDIFF_OK;
}

// gpudiff_submit's pairs: event i is slot i with documents 2i (old) and 2i + 1 (new), so the tables are filled by
// the workers -- a per-thread byte sum, then each thread writes its range from its offset.  Same tables as
// build_tables_store builds (that is the order-dependent path for store events).
int build_tables_pairs(DStore* s, const gpudiff_event* ev, size_t n, uint32_t batch, BatchTables& B) {
    gpudiff_ctx* c = s->c;
    static const uint8_t kNone[1] = {0};  // an absent old object: decode error
    const uint32_t T = (uint32_t)std::min<size_t>(std::max(1u, c->threads), std::max<size_t>(1, n / 4096));
    std::vector<uint64_t> part(4 * (size_t)T + 4, 0);  // per thread: JSON bytes, bound, floor, new bytes
    std::atomic<int> bad{0};
    B.src.resize(2 * n);
    // Zero copy: every document in one gpudiff_host_alloc buffer, 16-B aligned, in pair order, each followed
    // by its staged span before the next -- then the buffer's range is the staged layout itself
    uint8_t* zb = nullptr;
    uint64_t zn = 0;
    bool zc = ev[0].old_json && find_host_buf(c, ev[0].old_json, &zb, &zn);
    std::atomic<int> zc_bad{0};
    const uint8_t* zend = zb + zn - kTokSlack;  // the upload runs kTokSlack past the last document's span
    const uint32_t max_slots = s->max_slots;
    workers(c).run(T, [&part, &bad, &zc_bad, ev, n, T, zc, zb, zend, max_slots](uint32_t t) {
        uint64_t jb = 0, bd = 0, fl = 0, nj = 0;
        for (size_t i = n * t / T, i1 = n * (t + 1) / T; i < i1; i++) {
            const gpudiff_event& e = ev[i];
            if (e.slot != i || e.slot >= max_slots || !e.new_json || e.new_len > kTokMaxLen || e.old_len > kTokMaxLen)
                bad.store(1, std::memory_order_relaxed);
            if (zc) {
                const uint8_t* next = i + 1 < n ? ev[i + 1].old_json : zend;
                if (!e.old_json || e.old_json < zb || (((uintptr_t)e.old_json | (uintptr_t)e.new_json) & 15u) ||
                    e.new_json < e.old_json + tok_staged_span(e.old_len) || !next ||
                    next < e.new_json + tok_staged_span(e.new_len) || next > zend)
                    zc_bad.store(1, std::memory_order_relaxed);
            }
            const size_t lo = e.old_json ? e.old_len : 0;
            jb += tok_staged_span(lo) + tok_staged_span(e.new_len);
            bd += (5 * (uint64_t)lo) / 2 + (5 * (uint64_t)e.new_len) / 2 + 768;
            fl += lo + e.new_len;
            nj += e.new_len;
        }
        uint64_t* q = &part[4 * (size_t)(t + 1)];
        q[0] = jb, q[1] = bd, q[2] = fl, q[3] = nj;
    });
    if (bad.load()) return GPUDIFF_E_INVAL;
    zc = zc && !zc_bad.load();
    const uint8_t* zlo = ev[0].old_json;
    for (uint32_t t = 1; t <= T; t++)
        for (int k = 0; k < 4; k++) part[4 * (size_t)t + k] += part[4 * (size_t)(t - 1) + k];
    workers(c).run(T, [&part, &B, s, ev, n, T, zc, zlo, batch](uint32_t t) {
        uint64_t off = part[4 * (size_t)t];
        for (size_t i = n * t / T, i1 = n * (t + 1) / T; i < i1; i++) {
            const gpudiff_event& e = ev[i];
            const uint8_t* pj[2] = {e.old_json ? e.old_json : kNone, e.new_json};
            const size_t len[2] = {e.old_json ? e.old_len : 0, e.new_len};
            for (uint32_t h = 0; h < 2; h++) {
                const size_t k = 2 * i + h;
                TokDoc& D = B.docs[k];
                memset(&D, 0, sizeof(D));
                D.json_off = zc ? (uint64_t)(pj[h] - zlo) : off;
                D.json_len = (uint32_t)len[h];
                off += tok_staged_span(len[h]);
                if (zc)  // the staged span's padding, as the staging copy writes it (gpudiff.h: engine-owned)
                    memset((uint8_t*)pj[h] + len[h], 0, tok_staged_span(len[h]) - len[h]);
                DocLink& L = B.links[k];
                memset(&L, 0, sizeof(L));
                L.slot = e.slot;
                L.row = h ? (uint32_t)i : kNoRow;
                L.pair_id = e.pair_id;
                L.cluster_id = e.cluster_id;
                L.prev = h ? (int32_t)(2 * i) : -1;
                L.next = h ? -1 : (int32_t)(2 * i + 1);
                B.src[k] = pj[h];
            }
            B.heads[i] = (uint32_t)(2 * i);
            s->sstate[e.slot] = DStore::SlotState{batch, (int32_t)(2 * i + 1)};
        }
    });
    const uint64_t* tot = &part[4 * (size_t)T];
    B.nd = (uint32_t)(2 * n);
    B.nh = (uint32_t)n;
    B.jbytes = tot[0], B.bound = tot[1], B.floor = tot[2], B.new_json_bytes = tot[3];
    if (zc) {
        B.zsrc = zlo;
        B.jbytes = (uint64_t)(ev[n - 1].new_json + tok_staged_span(ev[n - 1].new_len) - zlo);
        s->st.zero_copy_batches++;
    }
    B.jbytes += kTokSlack;
    return GPUDIFF_OK;
}

// one staged document of a store batch, chained behind its slot's previous document of the batch
void add_doc(DStore* s, BatchTables& B, uint32_t batch, const uint8_t* p, size_t len, uint32_t row,
             const gpudiff_event& e) {
    const uint32_t nd = B.nd++;
    TokDoc& D = B.docs[nd];
    memset(&D, 0, sizeof(D));
    D.json_off = B.jbytes;
    D.json_len = (uint32_t)len;
    B.jbytes += tok_staged_span(len);
    // blob + path table: typically < 2.5x the JSON (the append estimate that triggers compaction);
    // K0 defers a document that does not fit (SPACE) to the host
    B.bound += (5 * (uint64_t)len) / 2 + 384;  // + the body's and the table's pads to 128 B
    B.floor += len;
    DocLink& L = B.links[nd];
    memset(&L, 0, sizeof(L));
    L.slot = e.slot;
    L.row = row;
    L.pair_id = e.pair_id;
    L.cluster_id = e.cluster_id;
    L.next = -1;
    DStore::SlotState& ss = s->sstate[e.slot];
    if (ss.stamp == batch) {
        L.prev = ss.last;
        B.links[L.prev].next = (int32_t)nd;
    } else {
        L.prev = -1;
        ss.stamp = batch;
        B.heads[B.nh++] = nd;
    }
    ss.last = (int32_t)nd;
    B.src.push_back(p);
}

// Store-mode zero copy: the documents this submit encodes -- per event, its old object on a slot's first sighting,
// then its new one -- lie in one gpudiff_host_alloc buffer in that order, each 16-B aligned and followed by its
// staged span, so the buffer's range is the staged layout (gaps between the documents, e.g. old objects the store
// does not encode, are uploaded but never read).  No staging copy.
void store_zero_copy(DStore* s, BatchTables& B) {
    uint8_t* zb = nullptr;
    uint64_t zn = 0;
    if (!find_host_buf(s->c, B.src[0], &zb, &zn) || zn <= kTokSlack) return;
    const uint8_t* zend = zb + zn - kTokSlack;  // the upload runs kTokSlack past the last document's span
    const uint8_t* at = B.src[0];
    for (uint32_t k = 0; k < B.nd; k++) {
        const uint8_t* p = B.src[k];
        if (!(p >= at && !((uintptr_t)p & 15u) && p + tok_staged_span(B.docs[k].json_len) <= zend)) return;
        at = p + tok_staged_span(B.docs[k].json_len);
    }
    B.zsrc = B.src[0];
    for (uint32_t k = 0; k < B.nd; k++) {
        B.docs[k].json_off = (uint64_t)(B.src[k] - B.zsrc);
        // the staged span's padding, as the staging copy writes it (gpudiff.h: engine-owned)
        memset((uint8_t*)B.src[k] + B.docs[k].json_len, 0, tok_staged_span(B.docs[k].json_len) - B.docs[k].json_len);
    }
    B.jbytes = (uint64_t)(at - B.zsrc);
    s->st.zero_copy_batches++;
}

// store events, in order: per event its new object, behind its old object on the slot's first sighting
int build_tables_store(DStore* s, const gpudiff_event* ev, size_t n, uint32_t batch, BatchTables& B) {
    for (size_t i = 0; i < n; i++) {
        const gpudiff_event& e = ev[i];
        if (i + 16 < n && ev[i + 16].slot < s->max_slots) {  // the slot state 16 events ahead
            __builtin_prefetch(&s->sstate[ev[i + 16].slot], 1);
            __builtin_prefetch(&s->seen[ev[i + 16].slot], 1);
        }
        if (e.slot >= s->max_slots || !e.new_json || e.new_len > kTokMaxLen || e.old_len > kTokMaxLen)
            return GPUDIFF_E_INVAL;
        if (!s->seen[e.slot] && e.old_json) {  // first sighting: its old object is the old side
            add_doc(s, B, batch, e.old_json, e.old_len, kNoRow, e);
            s->st.old_encoded++;
        }
        s->seen[e.slot] = 1;
        add_doc(s, B, batch, e.new_json, e.new_len, (uint32_t)i, e);
        B.new_json_bytes += e.new_len;
    }
    if (B.nd) store_zero_copy(s, B);
    B.jbytes += kTokSlack;
    return GPUDIFF_OK;
}

// the batch's device buffers and events
int grow_batch_buffers(DStore* s, Ring& R, const BatchTables& B, size_t n, bool strs, bool timing) {
    int rc;
    if ((rc = grow_dev(&R.djson, &R.djson_cap, B.jbytes)) || (rc = grow_dev(&R.dmeta, &R.dmeta_cap, B.meta_bytes)) ||
        (rc = grow_dev(&R.douts, &R.docs_cap, B.nd + 1)) || (rc = grow_dev(&R.dcoll, &R.coll_cap, B.nd + 1)) ||
        (rc = grow_dev(&R.ddef, &R.def_cap, n + 1)))
        return rc;
    if (strs && (rc = grow_dev(&R.dntab, &R.ntab_cap, 2 * (uint64_t)n + 2))) return rc;
    if (timing && !R.t_ev[0])
        for (auto& e : R.t_ev) HIPCHK(hipEventCreate(&e));
    if (!R.chunk_ev[0])
        for (auto& e : R.chunk_ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return GPUDIFF_OK;
}

// One chunk's way to the device: its H2D on the copy stream, then its K0 launches behind the copy's event -- on
// the kernel stream as soon as the upload is enqueued, so K0 of chunk q runs while chunk q + 1 is on the link,
// not after the host has staged them all.  Called in chunk order from one thread.
struct ChunkUploader {
    DStore* s;
    Ring& R;
    const UploadPlan& P;
    const uint8_t* hsrc;    // the staged layout: R.hjson, or the caller's buffer (zero copy)
    bool zero_copy;
    hipStream_t cs, k0s;    // the copy stream; the K0 stage's stream (even chunks, K0c, K0x)
    uint64_t scratch_half;  // each K0 stream's part of the scratch
    const TokDoc* ddocs;
    const DocLink* dlinks;
    bool timing;
    size_t li = 0;  // next K0 launch
    std::atomic<int> err{0};

    void upload(uint32_t q) {
        const uint64_t b0 = P.cbyte(q), b1 = P.cbyte(q + 1);
        if (!zero_copy && q + 1 == P.C && P.cdoc[q] >= P.nd) memset(R.hjson + b0, 0, b1 - b0);  // the slack only
        hipStream_t qs = cs;  // one DMA queue saturates the link (two measured slower, profiles/r04z)
        const bool odd = (q & 1u) != 0u;
        hipStream_t kq = odd ? s->ks : k0s;  // this chunk's K0 stream, and its half of the scratch
        uint8_t* scr = s->scratch + (odd ? scratch_half : 0);
        if (hipMemcpyAsync(R.djson + b0, hsrc + b0, b1 - b0, hipMemcpyHostToDevice, qs) != hipSuccess ||
            hipEventRecord(R.chunk_ev[q], qs) != hipSuccess || hipStreamWaitEvent(kq, R.chunk_ev[q], 0) != hipSuccess ||
            (q == 0 && timing && hipEventRecord(R.t_ev[2], k0s) != hipSuccess)) {
            err.store(1);
            return;
        }
        for (; li < P.launches.size() && P.chunk_of_launch[li] == q; li++) {
            const auto& L = P.launches[li];
            if (launch_encode_docs(kq, ddocs + L.first, L.second - L.first, R.djson, scr, s->space[s->cur],
                                   s->space_bytes, s->used_dev, s->c->hash_mask, R.douts + L.first, s->slots,
                                   dlinks + L.first) != hipSuccess) {
                err.store(1);
                return;
            }
        }
    }
};

// The stream ordering of the batch's upload and K0 stage, the three table copies, the staging copy by the workers
// with each chunk uploaded (and its K0 launched) as soon as it is staged, and R.staged behind the last copy.
int stage_and_encode(DStore* s, Ring& R, const BatchTables& B, const UploadPlan& P, size_t n, bool dec,
                     uint64_t scratch_half, bool timing, Lap& lap) {
    gpudiff_ctx* c = s->c;
    hipStream_t cs = s->cs;
    hipStream_t k0s = dec ? s->ks0 : c->stream;
    // the upload runs on the copy stream, behind this ring slot's previous K0 (which read the
    // same device buffers), so it overlaps the other batch's K0 / diff pass
    if (R.k0_recorded) HIPCHK(hipStreamWaitEvent(cs, R.k0_done, 0));
    if (timing) HIPCHK(hipEventRecord(R.t_ev[0], cs));
    // the tables' used parts only (their device offsets are sized for 2n documents)
    HIPCHK(hipMemcpyAsync(R.dmeta, R.hmeta, (uint64_t)B.nd * sizeof(TokDoc), hipMemcpyHostToDevice, cs));
    HIPCHK(hipMemcpyAsync(R.dmeta + B.links_off(), R.hmeta + B.links_off(), (uint64_t)B.nd * sizeof(DocLink),
                          hipMemcpyHostToDevice, cs));
    HIPCHK(hipMemcpyAsync(R.dmeta + B.heads_off(), R.hmeta + B.heads_off(), 4ull * B.nh + 4, hipMemcpyHostToDevice,
                          cs));
    if (dec) {  // what this batch's K0 stage reuses: the slot table (the previous batch's K0x read it) and this
                // ring slot's space, douts and rows (its previous batch's diff pass read them)
        if (s->last_ring >= 0 && s->ring[s->last_ring].k0_recorded)
            HIPCHK(hipStreamWaitEvent(k0s, s->ring[s->last_ring].k0_done, 0));
        if (R.pass_recorded) HIPCHK(hipStreamWaitEvent(k0s, R.pass_done, 0));
        HIPCHK(hipMemsetAsync(s->used_dev, 0, 8, k0s));
    }
    if (s->pair_mode) HIPCHK(hipMemsetAsync(s->slots, 0, sizeof(DSlot) * n, k0s));  // every pair starts empty
    if (s->ks) {  // the second K0 stream starts behind everything before this batch's K0 on the K0 stage's stream
        HIPCHK(hipEventRecord(s->ks_ev, k0s));
        HIPCHK(hipStreamWaitEvent(s->ks, s->ks_ev, 0));
    }
    ChunkUploader up{s, R, P, B.zsrc ? B.zsrc : R.hjson, B.zsrc != nullptr, cs, k0s, scratch_half,
                     (const TokDoc*)R.dmeta, (const DocLink*)(R.dmeta + B.links_off()), timing};
    uint32_t uploaded = 0;
    if (B.zsrc) {  // nothing to stage: every chunk's upload (and its K0 launches) goes out at once
        while (uploaded < P.C) up.upload(uploaded++);
    } else {
        // One run of the workers over all chunks: worker t copies its share of chunk 0, then of chunk
        // 1, ... and counts each chunk done; the calling thread (worker 0) enqueues a chunk's upload as
        // soon as every worker has counted it, then goes on with its own share of the next chunk.
        const uint32_t T =
            (uint32_t)std::min<uint64_t>(std::max(1u, c->threads), std::max<uint64_t>(1, B.jbytes >> 20));
        std::atomic<uint32_t> chunk_done[kMaxUpChunks];
        for (auto& x : chunk_done) x.store(0, std::memory_order_relaxed);
        uint8_t* hjson = R.hjson;
        workers(c).run(T, [&up, &P, &B, &chunk_done, &uploaded, hjson, T](uint32_t t) {
            for (uint32_t q = 0; q < P.C; q++) {
                const uint64_t b0 = P.cbyte(q), b1 = P.cbyte(q + 1);
                const uint32_t k0 = std::max(P.cdoc[q], P.first_doc(b0 + (b1 - b0) * t / T));
                const uint32_t k1 = std::min(P.cdoc[q + 1], P.first_doc(b0 + (b1 - b0) * (t + 1) / T));
                for (uint32_t k = k0; k < k1; k++) {
                    const uint64_t o = B.docs[k].json_off;
                    const uint64_t end = k + 1 < B.nd ? B.docs[k + 1].json_off : B.jbytes;
                    stream_doc(hjson + o, B.src[k], B.docs[k].json_len, end - o);
                }
                _mm_sfence();  // the streaming stores are visible before the chunk counts as done
                chunk_done[q].fetch_add(1, std::memory_order_release);
                if (t == 0)  // upload every chunk all workers have finished, in order, without waiting
                    while (uploaded <= q && chunk_done[uploaded].load(std::memory_order_acquire) >= T)
                        up.upload(uploaded++);
            }
            if (t == 0)
                while (uploaded < P.C) {
                    if (chunk_done[uploaded].load(std::memory_order_acquire) < T) {
                        std::this_thread::yield();
                        continue;
                    }
                    up.upload(uploaded++);
                }
        });
    }
    if (up.err.load()) return GPUDIFF_E_DEVICE;
    lap(2);
    HIPCHK(hipEventRecord(R.staged, cs));
    if (timing) HIPCHK(hipEventRecord(R.t_ev[1], cs));
    if (up.li != P.launches.size()) return GPUDIFF_E_STATE;  // every launch belongs to an uploaded chunk
    return GPUDIFF_OK;
}

// K0c and K0x behind every chunk's K0, then the ordinary diff pass over the batch's rows
int link_and_diff(DStore* s, Ring& R, const BatchTables& B, size_t n, uint32_t batch, bool dec, bool strs, bool timing,
                  gpudiff_ticket* ticket) {
    gpudiff_ctx* c = s->c;
    hipStream_t st = c->stream;
    hipStream_t k0s = dec ? s->ks0 : st;
    const DocLink* dlinks = (const DocLink*)(R.dmeta + B.links_off());
    const uint32_t* dheads = (const uint32_t*)(R.dmeta + B.heads_off());
    uint8_t* space = s->space[s->cur];
    if (s->ks) {  // K0c waits for the odd chunks' K0 too
        HIPCHK(hipEventRecord(s->ks_ev, s->ks));
        HIPCHK(hipStreamWaitEvent(k0s, s->ks_ev, 0));
    }
    HIPCHK(hipStreamWaitEvent(k0s, R.staged, 0));  // every chunk (and the tables) landed
    if (timing) HIPCHK(hipEventRecord(R.t_ev[3], k0s));
    HIPCHK(launch_collide(k0s, dlinks, R.douts, s->slots, B.nd, space, R.dcoll));
    HIPCHK(hipMemsetAsync(R.dcnt, 0, 4, k0s));
    gpudiff_dbatch* d = R.d;
    HIPCHK(launch_link(k0s, dheads, B.nh, dlinks, R.douts, R.dcoll, s->slots, d->rows, d->pair_ids, R.ddef, batch,
                       R.dcnt, s->ctr, strs ? R.dntab : nullptr));
    HIPCHK(hipEventRecord(R.k0_done, k0s));
    R.k0_recorded = true;
    if (timing) HIPCHK(hipEventRecord(R.t_ev[4], k0s));
    if (dec) HIPCHK(hipStreamWaitEvent(st, R.k0_done, 0));  // the diff pass reads the rows K0x wrote
    s->used_ub += B.bound;
    d->pool = space;
    d->pool_cap = s->space_bytes;
    d->pool_used = s->used_ub;
    d->n_pairs = n;
    d->rows_gen++;
    d->leaves = 0;
    d->compare_bytes = d->value_bytes = 0;
    d->size_hint_bytes = 2 * B.new_json_bytes;  // k2_sub_shift's size class (engine.h)
    if (int rc = gpudiff_diff(c, d, ticket)) {
        s->broken = true;
        return rc;
    }
    if (dec) {  // this ring slot's next K0 stage may refill its space once this pass has read it
        HIPCHK(hipEventRecord(R.pass_done, st));
        R.pass_recorded = true;
    }
    return GPUDIFF_OK;
}

// gpudiff_wait on the batch's ticket, after collect_results: the exact append point, the phase timings, the
// changed paths as text, the host resolution of what K0 deferred
int finish_batch(DStore* s, Ring& R, ResultStore& rs) {
    const auto t_fin0 = std::chrono::steady_clock::now();
    gpudiff_ctx* c = s->c;
    const uint32_t ri = (uint32_t)(&R - s->ring);
    R.outstanding = false;
    if (!s->pair_mode) {
        if (R.batch != s->next_wait) return GPUDIFF_E_STATE;  // waits follow submit order
        s->next_wait++;
    }
    uint32_t ndef = 0;
    uint64_t used = 0;
    if (s->pair_mode) {  // resolution appends to this batch's own space
        s->cur = ri;
        s->used_dev = s->used_base + s->cur;
    }
    HIPCHK(hipMemcpyAsync(&ndef, R.dcnt, 4, hipMemcpyDeviceToHost, c->rb));  // behind K0x: d->done waited
    HIPCHK(hipMemcpyAsync(&used, s->used_dev, 8, hipMemcpyDeviceToHost, c->rb));
    HIPCHK(hipStreamSynchronize(c->rb));
    // exact append point + what the other batch in flight may still add
    const Ring& other = s->ring[ri ^ 1u];
    s->used_ub = s->pair_mode ? used : std::max<uint64_t>(used, used + (other.outstanding ? other.bound : 0));
    if (R.t_ev[0] && (c->flags & GPUDIFF_OPT_TIMING)) {
        float ms[3];
        HIPCHK(hipEventElapsedTime(&ms[0], R.t_ev[0], R.t_ev[1]));  // H2D
        HIPCHK(hipEventElapsedTime(&ms[1], R.t_ev[2], R.t_ev[3]));  // K0
        HIPCHK(hipEventElapsedTime(&ms[2], R.t_ev[3], R.t_ev[4]));  // K0c + K0x
        for (int k = 0; k < 3; k++) s->t_sum[1 + k] += ms[k];
        s->t_n++;
    }
    // the strings before resolve(): its compaction may pack into the space this batch's superseded blobs are in
    int rc = (R.strs || R.vals) ? render_text(s, R, rs) : GPUDIFF_OK;
    R.d->final_patch = nullptr;
    R.plan_patch.clear();
    if (!rc && ndef) rc = resolve(s, R, rs);
    if (!rc && R.strs) {
        c->path_stats.paths += rs.ps.n;
        c->path_stats.bytes += rs.ps.offsets()[rs.ps.n];
        c->path_stats.host_paths += rs.ps.n_host;
    }
    if (!rc && R.vals) {
        c->value_stats.paths += rs.pv.n;
        c->value_stats.bytes += rs.pv.offsets()[2 * rs.pv.n];
        c->value_stats.host_paths += rs.pv.n_host;
    }
    if (rc) s->broken = true;
    if (!rc && s->pair_mode)  // kept for gpudiff_write_plan_get
        R.final_flags.assign(rs.flags.begin(), rs.flags.end());
    if (!rc) R.waited = true;  // the ring slot holds a waited batch until its next submit (the write plans' window)
    if (!rc) R.d->final_patch = &R.plan_patch;  // and gpudiff_cluster_index_get_final's: the resolved rows' final flags
    // forgets older than every outstanding batch are settled
    for (auto it = s->forgotten.begin(); it != s->forgotten.end();)
        it = it->second < s->next_wait ? s->forgotten.erase(it) : std::next(it);
    s->t_sub[4] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_fin0).count();
    return rc;
}

}  // namespace

int dstore_submit(gpudiff_ctx* c, DStore* s, const gpudiff_event* ev, size_t n, gpudiff_ticket* ticket) {
    if (s->broken) return GPUDIFF_E_STATE;
    if (n > s->max_events) return GPUDIFF_E_INVAL;
    if (refuse_if_strings_need_compaction(s, ev, n)) return GPUDIFF_E_STATE;
    const auto t_host0 = std::chrono::steady_clock::now();
    const bool timing = (c->flags & GPUDIFF_OPT_TIMING) != 0;
    const bool strs = (c->flags & GPUDIFF_OPT_PATH_STRINGS) != 0;
    // pair mode runs the K0 stage on its own streams (ks0 / ks), decoupled from the kernel stream
    const bool dec = s->pair_mode && s->ks0;
    int rc;
    Ring* Rp = nullptr;
    if ((rc = claim_ring_slot(s, dec, &Rp))) return rc;
    Ring& R = *Rp;
    R.waited = false;  // its tables are rewritten from here on: the previous batch's write plan is gone
    R.d->final_patch = nullptr;
    Lap lap{timing, s->t_sub};
    lap(0);
    const uint32_t batch = ++s->batch_seq;

    // 1. documents and slot chains
    BatchTables B;
    if ((rc = map_tables(R, n, B))) return rc;
    if ((rc = (s->pair_mode ? build_tables_pairs : build_tables_store)(s, ev, n, batch, B))) return rc;
    if (!B.zsrc && (rc = grow_pinned(&R.hjson, &R.hjson_cap, B.jbytes))) return rc;
    lap(1);
    const UploadPlan P = plan_upload(B.docs, B.nd, B.jbytes);
    const uint64_t scratch_half = (P.max_sb + 255u) & ~255ull;
    if ((rc = grow_dev(&s->scratch, &s->scratch_cap, s->ks ? 2 * scratch_half : scratch_half))) return rc;
    // 2. capacity (compaction is stream-ordered after every earlier batch)
    if ((rc = ensure_space(s, B.bound, B.floor))) return rc;
    // 3. upload + kernels
    if ((rc = grow_batch_buffers(s, R, B, n, strs, timing))) return rc;
    if ((rc = stage_and_encode(s, R, B, P, n, dec, scratch_half, timing, lap))) return rc;
    // 4. the links, and the diff pass over the batch's rows
    if ((rc = link_and_diff(s, R, B, n, batch, dec, strs, timing, ticket))) return rc;

    s->last_ring = (int)(&R - s->ring);
    R.events.assign(ev, ev + n);
    R.waited = false;
    R.batch = batch;
    R.nev = (uint32_t)n;
    R.nd = B.nd;
    R.links_off = B.links_off();
    R.bound = B.bound;
    R.strs = strs;
    R.vals = (c->flags & GPUDIFF_OPT_PATH_VALUES) != 0;
    R.space_idx = s->cur;
    R.ticket = *ticket;
    R.outstanding = true;
    c->finishers[*ticket] = [s, Rp](ResultStore& rs) -> int { return finish_batch(s, *Rp, rs); };
    s->ring_next ^= 1u;
    lap(3);
    if (timing)
        s->t_sum[0] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count();
    s->st.events += n;
    s->st.last_batch_bytes = B.jbytes;
    return GPUDIFF_OK;
}


int dstore_submit_pairs(gpudiff_ctx* c, const gpudiff_json_pair* pairs, size_t n, gpudiff_ticket* ticket) {
    DStore*& s = c->pair_store;
    uint64_t json = 0;
    for (size_t i = 0; i < n; i++) json += pairs[i].old_len + pairs[i].new_len;
    // one space per ring slot, each taking a whole batch: dstore_submit's bound (5/2 of the JSON + 384 B a
    // document), with half again as headroom so a growing batch does not recreate the store every time
    const uint64_t need = (5 * json) / 2 + 768 * (uint64_t)n + (1ull << 20);
    const uint64_t space = std::max<uint64_t>(512ull << 20, need + need / 2);
    if (!s || s->max_events < n || s->space_bytes < need) {
        if (s && (s->ring[0].outstanding || s->ring[1].outstanding))
            return GPUDIFF_E_CAPACITY;  // grows only between batches: gpudiff_submit encodes this one on the host
        if (s) dstore_free(c, s);
        s = nullptr;
        const uint32_t cap = (uint32_t)std::max<size_t>(65536, n + n / 2);
        int rc;
        s = dstore_create(c, cap, space, cap, &rc);
        if (!s) return rc;
        s->pair_mode = true;
    }
    std::vector<gpudiff_event> ev(n);
    for (size_t i = 0; i < n; i++) {
        const gpudiff_json_pair& p = pairs[i];
        ev[i] = gpudiff_event{(uint32_t)i, p.pair_id, p.cluster_id, 0, p.new_json, p.new_len, p.old_json, p.old_len};
        if (!p.new_json) {  // as gpudiff_encode_pairs: an absent object is a decode error
            static const uint8_t kNone[1] = {0};
            ev[i].new_json = kNone;
            ev[i].new_len = 0;
        }
    }
    return dstore_submit(c, s, ev.data(), n, ticket);
}

void dstore_timing_reset(DStore* s) {
    for (double& x : s->t_sum) x = 0;
    for (double& x : s->t_sub) x = 0;
    s->t_n = 0;
}

extern "C" int gpudiff_submit_stats_get(gpudiff_ctx* c, gpudiff_store_stats* out) {
    if (!c || !out) return GPUDIFF_E_INVAL;
    if (!c->pair_store) return GPUDIFF_E_STATE;
    return dstore_stats(c->pair_store, out);
}

extern "C" int gpudiff_host_alloc(gpudiff_ctx* c, size_t bytes, void** out) {
    if (!c || !out || !bytes) return GPUDIFF_E_INVAL;
    if (!c->has_device) return GPUDIFF_E_NODEVICE;
    HIPCHK(hipSetDevice(c->device));
    uint8_t* p = nullptr;
    if (hipHostMalloc((void**)&p, bytes, hipHostMallocDefault) != hipSuccess) return GPUDIFF_E_NOMEM;
    {
        std::lock_guard<std::mutex> lk(g_hb_mu);
        g_hb.push_back(HostBuf{c, p, (uint64_t)bytes});
    }
    *out = p;
    return GPUDIFF_OK;
}

extern "C" int gpudiff_host_free(gpudiff_ctx* c, void* p) {
    if (!c || !p) return GPUDIFF_E_INVAL;
    {
        std::lock_guard<std::mutex> lk(g_hb_mu);
        auto it = std::find_if(g_hb.begin(), g_hb.end(), [&](const HostBuf& h) { return h.c == c && h.p == p; });
        if (it == g_hb.end()) return GPUDIFF_E_INVAL;
        g_hb.erase(it);
    }
    if (c->has_device) (void)hipSetDevice(c->device);
    return hipHostFree(p) == hipSuccess ? GPUDIFF_OK : GPUDIFF_E_DEVICE;
}

void dstore_host_bufs_release(gpudiff_ctx* c) {
    std::lock_guard<std::mutex> lk(g_hb_mu);
    for (auto it = g_hb.begin(); it != g_hb.end();)
        if (it->c == c) {
            (void)hipHostFree(it->p);
            it = g_hb.erase(it);
        } else {
            ++it;
        }
}

int dstore_forget(gpudiff_ctx* c, DStore* s, uint32_t slot) {
    HIPCHK(launch_forget(c->stream, s->slots, slot, s->ctr));
    s->seen[slot] = 0;
    s->forgotten[slot] = s->batch_seq;
    return GPUDIFF_OK;
}

int dstore_stats(const DStore* s, gpudiff_store_stats* out) {
    *out = s->st;
    uint32_t ctr[4] = {0, 0, 0, 0};
    uint64_t used = 0;
    HIPCHK(hipSetDevice(s->c->device));
    HIPCHK(hipStreamSynchronize(s->c->stream));
    HIPCHK(hipMemcpy(ctr, s->ctr, 16, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&used, s->used_dev, 8, hipMemcpyDeviceToHost));
    out->live_slots = ctr[kCtrLive];
    uint64_t lb;
    memcpy(&lb, ctr + kCtrLiveBytes, 8);
    out->live_bytes = lb;
    out->used_bytes = used;
    out->deferred = s->deferred_total;
    if (s->t_n) {
        out->host_submit_ms = (float)(s->t_sum[0] / s->t_n);
        out->h2d_ms = (float)(s->t_sum[1] / s->t_n);
        out->encode_ms = (float)(s->t_sum[2] / s->t_n);
        out->link_ms = (float)(s->t_sum[3] / s->t_n);
        float* sub[5] = {&out->submit_wait_ms, &out->submit_docs_ms, &out->submit_copy_ms, &out->submit_enqueue_ms,
                         &out->finish_ms};
        for (int k = 0; k < 5; k++) *sub[k] = (float)(s->t_sub[k] / s->t_n);
        out->timing_batches = (uint32_t)s->t_n;
    }
    return GPUDIFF_OK;
}

void dstore_free(gpudiff_ctx* c, DStore* s) {
    if (!s) return;
    if (c && c->has_device) {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        if (s->cs) (void)hipStreamSynchronize(s->cs);
    }
    for (Ring& R : s->ring) {
        if (R.d) gpudiff_dbatch_free(c, R.d);
        if (R.ticket) c->finishers.erase(R.ticket);
        for (void* p : {(void*)R.djson, (void*)R.dmeta, (void*)R.douts, (void*)R.dcoll, (void*)R.ddef, (void*)R.dcnt,
                        (void*)R.dntab, (void*)R.ps_len, (void*)R.ps_tiles, (void*)R.tx_ctr, (void*)R.ps_out,
                        (void*)R.pl_flags, (void*)R.pl_patch, (void*)R.pl_words, (void*)R.pl_tiles, (void*)R.pl_rec,
                        (void*)R.pl_head, (void*)R.pl_wdoc, (void*)R.pl_lens, (void*)R.pl_tdocs, (void*)R.pl_touts,
                        (void*)R.pl_scratch, (void*)R.pl_arena, (void*)R.pl_bytes, (void*)R.pl_mv,
                        (void*)R.pl_gather})
            if (p) (void)hipFree(p);
        for (auto& e : R.ps_ev)
            if (e) (void)hipEventDestroy(e);
        R.vb.free_all();
        for (auto& e : R.pl_ev)
            if (e) (void)hipEventDestroy(e);
        for (void* p : {(void*)R.hjson, (void*)R.hmeta})
            if (p) (void)hipHostFree(p);
        if (R.staged) (void)hipEventDestroy(R.staged);
        if (R.k0_done) (void)hipEventDestroy(R.k0_done);
        for (auto& e : R.t_ev)
            if (e) (void)hipEventDestroy(e);
        for (auto& e : R.chunk_ev)
            if (e) (void)hipEventDestroy(e);
    }
    if (s->res_d) gpudiff_dbatch_free(c, s->res_d);
    s->res_vb.free_all();
    for (hipStream_t* k : {&s->ks, &s->ks0})
        if (*k) {
            (void)hipStreamSynchronize(*k);
            (void)hipStreamDestroy(*k);
        }
    for (Ring& R : s->ring)
        if (R.pass_done) (void)hipEventDestroy(R.pass_done);
    if (s->ks_ev) (void)hipEventDestroy(s->ks_ev);
    if (s->cs) {
        (void)hipStreamSynchronize(s->cs);
        (void)hipStreamDestroy(s->cs);
    }
    for (void* p : {(void*)s->space[0], (void*)s->space[1], (void*)s->used_base, (void*)s->slots, (void*)s->ctr,
                    (void*)s->sizes, (void*)s->tile_sums, (void*)s->scratch, (void*)s->res_stage, (void*)s->res_ups,
                    (void*)s->res_err})
        if (p) (void)hipFree(p);
    delete s;
}

// ------------------------------------------------------------------ the store's write plan
namespace {

// a plan buffer on the ring slot: kept across calls, grown (never per call) -- out of memory is the caller's
// GPUDIFF_E_CAPACITY, not a device error
template <class T>
int grow_plan(T** p, uint64_t* cap, uint64_t need) {
    if (need <= *cap) return GPUDIFF_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    const uint64_t n = std::max<uint64_t>(need + need / 4, 64);
    const hipError_t e = hipMalloc((void**)p, (size_t)n * sizeof(T));
    if (e != hipSuccess) {
        *p = nullptr;
        (void)hipGetLastError();
        gd::g_last_hip_error = hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? GPUDIFF_E_CAPACITY : GPUDIFF_E_DEVICE;
    }
    *cap = n;
    return GPUDIFF_OK;
}

// the write list as K18 / K19 write it and one copy brings it back: 8-B words, then 4-B, then bytes
// (the targets, when asked for, among the 4-B words)
struct PlanHead {
    uint64_t off_pair, off_src, off_k10, off_tgt, off_kind, off_noop, bytes;
    PlanHead(uint64_t nw, bool targets) {
        off_pair = 8 * (nw + 1);
        off_src = off_pair + 4 * nw;
        off_k10 = off_src + 4 * nw;
        off_tgt = off_k10 + 4 * nw;
        off_kind = off_tgt + (targets ? sizeof(TargetWords) * nw : 0);
        off_noop = off_kind + nw;
        bytes = (off_noop + nw + 7) & ~7ull;
    }
};

}  // namespace

// The plan reads only what the waited batch left on its ring slot -- dmeta (documents, chains), djson, the diff
// pass's flags on R.d -- and writes only the slot's pl_* buffers, so it runs on the readback stream: never behind
// the other batch in flight on the kernel stream.  Its last read of djson / dmeta is marked in R.k0_done, which
// the slot's next upload waits for (lifetimes).
int dstore_write_plan(gpudiff_ctx* c, DStore* s, gpudiff_ticket t, uint32_t kinds, bool targets, StorePlan* out) {
    if (!s || s->broken || s->pair_mode || !t) return GPUDIFF_E_STATE;
    Ring* Rp = nullptr;
    for (Ring& Q : s->ring)
        if (Q.ticket == t) Rp = &Q;
    if (!Rp || !Rp->waited || Rp->outstanding) return GPUDIFF_E_STATE;  // unknown, not waited yet, or reused
    Ring& R = *Rp;
    hipStream_t st = c->rb;
    const bool timing = (c->flags & GPUDIFF_OPT_TIMING) != 0;
    if (timing && !R.pl_ev[0])
        for (auto& e : R.pl_ev) HIPCHK(hipEventCreate(&e));
    gpudiff_store_plan_stats S{};
    S.calls = s->plan_st.calls + 1;
    S.events = R.nev;
    S.docs = R.nd;
    int rc;
    const uint32_t nev = R.nev, nd = R.nd, np = (uint32_t)R.plan_patch.size();
    const uint32_t nt = scan64_tiles(nd);
    if ((rc = grow_plan(&R.pl_flags, &R.pl_flags_cap, nev)) || (rc = grow_plan(&R.pl_patch, &R.pl_patch_cap, np)) ||
        (rc = grow_plan(&R.pl_words, &R.pl_words_cap, nd)) ||
        (rc = grow_plan(&R.pl_tiles, &R.pl_tiles_cap, (uint64_t)kPlanCols * nt + 8)))
        return rc;
    if (!R.pl_rec) {
        uint64_t cap = 0;
        if ((rc = grow_plan(&R.pl_rec, &cap, 16))) return rc;
    }
    // 1. final flags, K17, the scan's top: the counts and byte totals
    if (np) {
        HIPCHK(hipMemcpyAsync(R.pl_patch, R.plan_patch.data(), np * sizeof(PlanPatch), hipMemcpyHostToDevice, st));
        S.h2d_bytes += np * sizeof(PlanPatch);
    }
    if (timing) HIPCHK(hipEventRecord(R.pl_ev[0], st));
    const gpudiff_dbatch* d = R.d;
    HIPCHK(launch_plan_flags(st, d->flags, d->summary, d->dirty_idx, d->noop_d, R.pl_patch, np, nev, R.pl_flags));
    const PlanIn in{(const TokDoc*)R.dmeta, (const DocLink*)(R.dmeta + R.links_off), nd, R.pl_flags, nev, kinds};
    HIPCHK(launch_plan_tails(st, in, R.pl_words, R.pl_tiles, R.pl_rec));
    uint64_t rec[kPlanCols] = {};
    HIPCHK(hipMemcpyAsync(rec, R.pl_rec, sizeof(rec), hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(R.k0_done, st));  // dmeta's read marker (no write: nothing after this reads it or djson)
    R.k0_recorded = true;
    HIPCHK(hipStreamSynchronize(st));
    S.d2h_bytes += sizeof(rec);
    const uint64_t nw = rec[kColSpecWrites] + rec[kColStatusWrites], n_sd = rec[kColSpecDocs],
                   n_td = rec[kColStatusDocs], ndocs = n_sd + n_td;
    if (nw > 2ull * nd || ndocs > nw) return GPUDIFF_E_DEVICE;  // not a scan of this table
    out->n = (size_t)nw;
    const PlanHead H(nw, targets);
    auto map_words = [&]() {
        const uint8_t* b = (const uint8_t*)out->words.data();
        out->offsets = out->words.data();
        out->pair_index = (const uint32_t*)(b + H.off_pair);
        out->src_doc = (const uint32_t*)(b + H.off_src);
        out->k10 = (const int32_t*)(b + H.off_k10);
        out->tgt = targets ? (const TargetWords*)(b + H.off_tgt) : nullptr;
        out->kind = b + H.off_kind;
        out->noop = b + H.off_noop;
        out->bytes = b + H.bytes;
    };
    if (!nw) {  // nothing to write: nothing more is launched
        out->words.assign(1, 0);
        map_words();
        s->plan_st = S;
        return GPUDIFF_OK;
    }
    // 2. K18 into the write list and K10's table, K10 once per kind, the bodies' lengths scanned
    const uint64_t scratch_bytes = std::max(rec[kColSpecScratch], rec[kColStatusScratch]);
    const uint64_t arena_bytes = rec[kColSpecCap] + rec[kColStatusCap];
    if ((rc = grow_plan(&R.pl_head, &R.pl_head_cap, H.bytes)) || (rc = grow_plan(&R.pl_wdoc, &R.pl_wdoc_cap, nw)) ||
        (rc = grow_plan(&R.pl_lens, &R.pl_lens_cap, nw)) || (rc = grow_plan(&R.pl_tdocs, &R.pl_tdocs_cap, ndocs)) ||
        (rc = grow_plan(&R.pl_touts, &R.pl_touts_cap, ndocs)) ||
        (rc = grow_plan(&R.pl_scratch, &R.pl_scratch_cap, scratch_bytes)) ||
        (rc = grow_plan(&R.pl_arena, &R.pl_arena_cap, arena_bytes + 16)))  // K19 reads whole dwords
        return rc;
    const PlanLists L{(uint32_t*)(R.pl_head + H.off_pair), (uint32_t*)(R.pl_head + H.off_src), R.pl_wdoc,
                      R.pl_head + H.off_kind, R.pl_head + H.off_noop, R.pl_tdocs, (uint32_t)nw, (uint32_t)ndocs};
    HIPCHK(launch_plan_docs(st, in, R.pl_words, R.pl_tiles, R.pl_rec, L));
    if (timing) HIPCHK(hipEventRecord(R.pl_ev[1], st));
    if (timing) HIPCHK(hipEventRecord(R.pl_ev[2], st));
    HIPCHK(launch_marshal_docs(st, R.pl_tdocs, (uint32_t)n_sd, R.djson, R.pl_scratch, R.pl_arena, GPUDIFF_UPSERT_SPEC,
                               R.pl_touts));
    HIPCHK(launch_marshal_docs(st, R.pl_tdocs + n_sd, (uint32_t)n_td, R.djson, R.pl_scratch, R.pl_arena,
                               GPUDIFF_UPSERT_STATUS, R.pl_touts + n_sd));
    HIPCHK(hipEventRecord(R.k0_done, st));  // the staged JSON's read marker, behind K10
    if (timing) HIPCHK(hipEventRecord(R.pl_ev[3], st));
    if (timing) HIPCHK(hipEventRecord(R.pl_ev[4], st));
    HIPCHK(launch_body_lens(st, R.pl_wdoc, R.pl_touts, (uint32_t)nw, (uint32_t)ndocs, R.pl_lens,
                            (uint32_t*)(R.pl_head + H.off_k10),
                            targets ? (TargetWords*)(R.pl_head + H.off_tgt) : nullptr, R.pl_tiles, R.pl_rec + 8));
    uint64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, R.pl_rec + 8, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    S.d2h_bytes += 8;
    if (total > arena_bytes) return GPUDIFF_E_DEVICE;
    // 3. K19: the bodies packed to their dense offsets; offsets | write list | bytes come back
    if ((rc = grow_plan(&R.pl_bytes, &R.pl_bytes_cap, total + 8))) return rc;
    HIPCHK(launch_pack_bodies(st, R.pl_wdoc, R.pl_touts, (uint32_t)nw, (uint32_t)ndocs, R.pl_lens, R.pl_tiles,
                              (uint64_t*)R.pl_head, R.pl_arena, arena_bytes, R.pl_bytes, total));
    if (timing) HIPCHK(hipEventRecord(R.pl_ev[5], st));
    try {
        out->words.assign((size_t)(H.bytes / 8 + (total + 7) / 8), 0);
    } catch (const std::bad_alloc&) {
        return GPUDIFF_E_NOMEM;
    }
    map_words();
    HIPCHK(hipMemcpyAsync(out->words.data(), R.pl_head, H.bytes, hipMemcpyDeviceToHost, st));
    if (total) HIPCHK(hipMemcpyAsync((uint8_t*)out->words.data() + H.bytes, R.pl_bytes, total, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    S.d2h_bytes += H.bytes + total;
    if (out->offsets[nw] != total) return GPUDIFF_E_DEVICE;  // the offsets the bodies were packed by
    // K10's verdict words, in place: the statuses where they came back, the splice points beside them
    try {
        out->rv_off_v.resize(nw);
        out->rv_form_v.resize(nw);
    } catch (const std::bad_alloc&) {
        return GPUDIFF_E_NOMEM;
    }
    int32_t* const k10 = (int32_t*)((uint8_t*)out->words.data() + H.off_k10);
    for (uint64_t w = 0; w < nw; w++) {
        uint32_t ro, rf;
        plan_k10_unpack((uint32_t)k10[w], &k10[w], &ro, &rf);
        out->rv_off_v[w] = ro;
        out->rv_form_v[w] = (uint8_t)rf;
    }
    out->rv_off = out->rv_off_v.data();
    out->rv_form = out->rv_form_v.data();
    // 4. K10's deferrals: their JSON gathered from djson on the device, one copy back (the caller's event buffers
    //    are not read: they are only valid until gpudiff_wait)
    const TokDoc* hdocs = (const TokDoc*)R.hmeta;
    for (uint64_t w = 0; w < nw; w++) {
        if (out->noop[w]) S.noops++;
        else if (out->k10[w] != GPUDIFF_TOK_OK) out->def.push_back((uint32_t)w);
    }
    if (!out->def.empty()) {
        const size_t n_def = out->def.size();
        std::vector<BlobMove> mv(n_def);
        out->hoff.resize(n_def);
        out->hlen.resize(n_def);
        uint64_t gb = 0;
        for (size_t k = 0; k < n_def; k++) {
            const uint32_t sd = out->src_doc[out->def[k]];
            if (sd >= nd) return GPUDIFF_E_DEVICE;
            // K7's 16-B copies: a staged document starts 16-B aligned and its span runs >= 16 B past its end
            mv[k] = BlobMove{hdocs[sd].json_off, gb, ((uint64_t)hdocs[sd].json_len + 15u) & ~15ull};
            out->hoff[k] = gb;
            out->hlen[k] = hdocs[sd].json_len;
            gb += mv[k].bytes;
        }
        if ((rc = grow_plan(&R.pl_mv, &R.pl_mv_cap, n_def)) || (rc = grow_plan(&R.pl_gather, &R.pl_gather_cap, gb + 16)))
            return rc;
        out->hjson.resize(gb);
        HIPCHK(hipMemcpyAsync(R.pl_mv, mv.data(), n_def * sizeof(BlobMove), hipMemcpyHostToDevice, st));
        HIPCHK(launch_move_blobs(st, R.djson, R.pl_gather, R.pl_mv, (uint32_t)n_def));
        HIPCHK(hipEventRecord(R.k0_done, st));  // the read marker again, behind the last read of djson
        if (gb) HIPCHK(hipMemcpyAsync(out->hjson.data(), R.pl_gather, gb, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        S.h2d_bytes += n_def * sizeof(BlobMove);
        S.d2h_bytes += gb;
    }
    S.writes = nw;
    S.bodies = ndocs;
    S.host_bodies = out->def.size();
    S.body_bytes = total;
    S.arena_bytes = arena_bytes;
    if (timing) {
        float ms[3] = {0, 0, 0};
        for (int k = 0; k < 3; k++) HIPCHK(hipEventElapsedTime(&ms[k], R.pl_ev[2 * k], R.pl_ev[2 * k + 1]));
        S.fold_ms = ms[0];
        S.k10_ms = ms[1];
        S.pack_ms = ms[2];
    }
    s->plan_st = S;
    return GPUDIFF_OK;
}

int dstore_plan_stats(const DStore* s, gpudiff_store_plan_stats* out) {
    *out = s->plan_st;
    return GPUDIFF_OK;
}

int dstore_staged_pairs(gpudiff_ctx* c, gpudiff_ticket t, StagedPairs* out) {
    DStore* s = c->pair_store;
    if (!s || !t) return GPUDIFF_E_STATE;
    for (Ring& R : s->ring) {
        if (R.ticket != t) continue;
        if (!R.waited || R.outstanding) return GPUDIFF_E_STATE;  // gpudiff_wait first
        out->hdocs = (const TokDoc*)R.hmeta;
        out->djson = R.djson;
        out->n = R.nev;
        out->flags = &R.final_flags;
        out->events = &R.events;
        return GPUDIFF_OK;
    }
    return GPUDIFF_E_STATE;  // not a device-encoded batch, or its staging was reused
}

int dstore_staged_mark_read(gpudiff_ctx* c, gpudiff_ticket t) {
    DStore* s = c->pair_store;
    if (!s) return GPUDIFF_E_STATE;
    for (Ring& R : s->ring)
        if (R.ticket == t) {
            HIPCHK(hipEventRecord(R.k0_done, c->stream));
            R.k0_recorded = true;
            return GPUDIFF_OK;
        }
    return GPUDIFF_E_STATE;
}
