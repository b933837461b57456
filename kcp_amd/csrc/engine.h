// Internal engine state shared by the C-ABI translation units (api.cpp,
// store.cpp).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <functional>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/gpudiff.h"
#include "encoder.h"
#include "pool.h"
#include "kernels.h"

using gd::PairEncoder;
using gd::EncodeConfig;

namespace gd {
extern thread_local std::string g_last_hip_error;
}

#define HIPCHK(x)                                             \
    do {                                                      \
        hipError_t e_ = (x);                                  \
        if (e_ != hipSuccess) {                               \
            gd::g_last_hip_error = hipGetErrorString(e_);     \
            return GPUDIFF_E_DEVICE;                          \
        }                                                     \
    } while (0)

namespace gd {
struct Part {
    std::vector<uint8_t> pool;
    std::vector<gpudiff_pair_row> rows;
    uint64_t leaves = 0, errors = 0, reseeded = 0;
};
}  // namespace gd

// changed-path arena entries per K2 wave (a pair whose worst case does not
// fit the wave's remaining arena is deferred to K4)
inline constexpr uint32_t kArenaPerWave = 16384;

struct gpudiff_hbatch {
    uint8_t* pool = nullptr;
    gpudiff_pair_row* rows = nullptr;
    size_t n = 0;
    uint64_t pool_bytes = 0;
    uint64_t leaves = 0, errors = 0, reseeded = 0;
    uint64_t pool_cap = 0;
    size_t rows_cap = 0;
    bool pinned = false;
    hipEvent_t used = nullptr;  // last async copy that reads this batch
};

// gpudiff_cluster_index_get (fanout.cpp): the one mark gpudiff_wait leaves on a batch -- the ticket whose results it
// returned and their counts -- and the index's device buffers, which live on the batch and grow on demand
struct WaitedMark {
    gpudiff_ticket ticket = 0;
    uint32_t n_spec = 0, n_status = 0, n_dirty = 0;
    // gpudiff_cluster_index_get_final: the length of the device pass's own dirty list (dirty_idx / dirty_ids), read
    // before the ticket's finisher ran; n_dirty above counts what is left after the host resolved the deferred rows
    uint32_t n_dev_dirty = 0;
};
namespace gd {
struct PlanPatch;  // plan.h
}
struct FanBuffers;
void fan_buffers_release(FanBuffers* f);
struct FanCtx;
void fan_ctx_release(FanCtx* f);

struct gpudiff_dbatch {
    uint64_t pool_cap = 0, pool_used = 0;
    uint64_t max_pairs = 0, n_pairs = 0;
    uint64_t leaves = 0, compare_bytes = 0, value_bytes = 0;
    // K0-encoded batches (the device-encode store / submit): the rows are built on the device, so
    // compare_bytes is unknown on the host; this is the batch's JSON bytes per pair side x 2 (config3
    // objects: 0.85 compare bytes per JSON byte), the size class K2's item split goes by (k2_sub_shift)
    uint64_t size_hint_bytes = 0;
    uint8_t* pool = nullptr;
    bool pool_borrowed = false;  // pool owned by a gpudiff_store (its current space)
    gpudiff_pair_row* rows = nullptr;
    uint32_t* pair_ids = nullptr;
    uint8_t* flags = nullptr;
    uint32_t* caps = nullptr;
    void* chunk_counts = nullptr;
    uint32_t* summary = nullptr;
    uint32_t* spec_ids = nullptr;
    uint32_t* status_ids = nullptr;
    uint32_t* dirty_ids = nullptr;
    uint32_t* dirty_idx = nullptr;
    uint32_t* scratch_off = nullptr;
    uint32_t* path_count = nullptr;
    uint32_t* path_off = nullptr;
    uint32_t* tile_sums = nullptr;
    uint32_t* path_src = nullptr;
    uint32_t* path_cnt = nullptr;
    uint8_t* nbits = nullptr;   // per pair: no-op bits of K2's joins
    uint8_t* noop_d = nullptr;  // per dirty pair: no-op bits
    uint64_t arena_cap = 0;
    uint64_t* arena_h = nullptr;
    uint8_t* arena_k = nullptr;
    uint64_t scratch_cap = 0;
    uint64_t* scratch_h = nullptr;
    uint8_t* scratch_k = nullptr;
    uint32_t* slot_owner = nullptr;  // K4 slices (kernels.h DiffBuffers)
    uint32_t* slice_cnt = nullptr;
    uint8_t* slice_weq = nullptr;
    uint64_t* out_h = nullptr;
    uint8_t* out_k = nullptr;
    hipEvent_t done = nullptr;
    gpudiff_ticket ticket = 0;
    uint32_t* gather_send = nullptr;  // gpudiff_dbatch_bind_gather
    uint32_t gather_cap_spec = 0, gather_cap_status = 0;
    // gpudiff_dbatch_result_slot: the spec / status lists and the summary (counts) of the other slot
    // (spec_ids / status_ids / summary are always the current slot's; switching swaps them), allocated on
    // first use -- all three or none
    uint32_t* ids_alt[2] = {nullptr, nullptr};
    uint32_t* summary_alt = nullptr;
    uint32_t res_slot = 0;
    // gpudiff_dbatch_create_view: this batch diffs `base`'s resident pairs (pool, rows, pair IDs borrowed,
    // refreshed at every diff) into its own outputs, so two passes over one population can be in flight
    const gpudiff_dbatch* base = nullptr;
    // a base's live views (gpudiff_dbatch_create_view registers, gpudiff_dbatch_free removes): the passes of one
    // population that can be in flight together -- K2 launches half its grid while another of them is running
    mutable std::vector<gpudiff_dbatch*> views;
    int device = -1;
    uint32_t* tail_perm = nullptr;  // K2's largest-first final round (kernels.h DiffBuffers)
    gd::TailPermKey tail_perm_key;
    uint64_t rows_gen = 0;  // bumped whenever the rows change (appends, resets, store batches): K2's cached order
    // K2's 16-B pair descriptors (gpudiff_format.h), parallel to rows; a view borrows its base's.  Written by
    // gpudiff_dbatch_append's rebase kernel only: desc_gen == rows_gen says every resident row's descriptor is
    // current, and K2 gets the array only then -- any other producer of rows bumps rows_gen alone and K2 reads rows
    uint4* desc = nullptr;
    uint64_t desc_gen = ~0ull;
    // The compare image (gpudiff_format.h: gpudiff_pair_image_parts): one allocation made by the first
    // append, image_cap bytes (gpudiff_dbatch_set_image_capacity, default the pool's capacity), filled by the appends'
    // builder kernel and reached only through image-form descriptors -- so desc_gen covers its staleness too.  A view
    // borrows it.  image_cursor: the image bytes of every imaged-if-it-fits pair appended so far (the next append's
    // base; past image_cap once the image is full), image_used / image_pairs: what is in it.  image_off: no image
    // (capacity 0, or its allocation failed).  image_scan: the builder's scratch for a chunk of image_scan_n rows.
    uint8_t* image = nullptr;
    uint64_t image_cap = 0, image_cap_req = ~0ull, image_cursor = 0, image_used = 0, image_pairs = 0;
    bool image_off = false;
    uint64_t* image_scan = nullptr;
    uint64_t image_scan_n = 0;
    // what K2 streams of the imaged pairs (their descriptors and packed chunks), summed by the builder on the device:
    // one u64 allocated with the image, read back by gpudiff_dbatch_image_streamed_bytes
    uint64_t* image_streamed = nullptr;
    hipEvent_t image_built = nullptr;  // recorded behind each append's builder kernel: the sum's reader waits for it
    // GPUDIFF_OPT_SMALL_PASS: the result image K20 packs (small_pass.h; allocated by the batch's first small pass),
    // and whether the pass `done` stands for was a small one (collect_results reads the image then)
    uint8_t* small_image = nullptr;
    bool small_pending = false;
    WaitedMark waited;          // set by gpudiff_wait alone; waited.ticket == ticket: the device arrays are final
    FanBuffers* fan = nullptr;  // allocated by the batch's first gpudiff_cluster_index_get / _get_final
    // a device-encode store's ring batch (store or pair mode): the host resolves its deferred rows.  final_patch is
    // those rows' final flags of the waited batch (Ring::plan_patch), set by the batch's finisher and null again from
    // the ring slot's next submit on -- gpudiff_cluster_index_get_final's window, as the write plan's
    bool host_resolves = false;
    const std::vector<gd::PlanPatch>* final_patch = nullptr;
};

struct DStore;

// GPUDIFF_OPT_PATH_STRINGS: the changed paths as text, entry i for hashes[i] / kinds[i].  One allocation, as it
// comes back from the device in one copy: offsets[n + 1], then the strings' bytes
struct PathStrs {
    bool on = false;
    size_t n = 0;
    std::vector<uint64_t> words;  // [n + 1] offsets | bytes (rounded up to 8)
    size_t n_host = 0, n_unresolved = 0;
    const uint64_t* offsets() const { return words.data(); }
    const char* bytes() const { return (const char*)(words.data() + n + 1); }
    // built entry by entry (the host resolution's merge)
    void begin() {
        words.assign(1, 0);
        tail.clear();
        n = 0;
    }
    void push(const char* p, size_t len) {
        tail.append(p, len);
        words.push_back(tail.size());
        n++;
    }
    void finish() {
        const size_t w = (tail.size() + 7) / 8;
        words.resize(n + 1 + w, 0);
        if (!tail.empty()) memcpy(words.data() + n + 1, tail.data(), tail.size());
        tail.clear();
        tail.shrink_to_fit();
    }
    std::string tail;
};

// GPUDIFF_OPT_PATH_VALUES: the changed leaves' old and new values as JSON text, texts 2i / 2i + 1 for hashes[i] /
// kinds[i].  One allocation, as it comes back from the device in one copy: offsets[2n + 1], the tags[2n] (padded to
// 8), then the texts' bytes
struct PathVals {
    bool on = false;
    size_t n = 0;  // entries (two texts each)
    std::vector<uint64_t> words;
    size_t n_host = 0, n_unresolved = 0;
    static size_t tag_words(size_t n) { return (2 * n + 7) / 8; }
    const uint64_t* offsets() const { return words.data(); }
    const uint8_t* tags() const { return (const uint8_t*)(words.data() + 2 * n + 1); }
    const char* bytes() const { return (const char*)(words.data() + 2 * n + 1 + tag_words(n)); }
    // built entry by entry (the host resolution's merge)
    void begin() {
        offs.assign(1, 0);
        tg.clear();
        tail.clear();
        n = 0;
    }
    void push(uint8_t tag, const char* p, size_t len) {  // one text; two of them make an entry
        tail.append(p, len);
        offs.push_back(tail.size());
        tg.push_back(tag);
    }
    void finish() {
        n = tg.size() / 2;
        words.assign(2 * n + 1 + tag_words(n) + (tail.size() + 7) / 8, 0);
        memcpy(words.data(), offs.data(), offs.size() * 8);
        if (!tg.empty()) memcpy(words.data() + 2 * n + 1, tg.data(), tg.size());
        if (!tail.empty()) memcpy(words.data() + 2 * n + 1 + tag_words(n), tail.data(), tail.size());
        offs = {};
        tg = {};
        tail = {};
    }
    std::vector<uint64_t> offs;
    std::vector<uint8_t> tg;
    std::string tail;
};

struct ResultStore {
    std::vector<uint8_t> flags;
    std::vector<uint32_t> spec, status, dirty, off;
    std::vector<uint64_t> hashes;
    std::vector<uint8_t> kinds;
    PathStrs ps;
    PathVals pv;
};

struct gpudiff_ctx {
    int device = GPUDIFF_DEVICE_NONE;
    bool has_device = false;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    uint32_t threads = 1;
    uint32_t flags = 0;
    bool k2_timeline = false;  // gpudiff_k2_profile installed a buffer: the timeline build of K2 runs
    EncodeConfig ecfg;
    uint64_t hash_mask = ~0ULL;
    std::vector<std::unique_ptr<PairEncoder>> encoders;
    std::vector<gd::Part> parts;
    gpudiff_ticket next_ticket = 1;
    std::unordered_map<gpudiff_ticket, gpudiff_dbatch*> tickets;
    std::vector<std::array<hipEvent_t, 5>> pass_ev;
    size_t n_pass = 0;
    hipStream_t rb = nullptr;     // result readback (never behind work queued after the batch)
    gpudiff_pass_stats pass_stats{};  // gpudiff_pass_stats_get
    uint8_t* small_rb = nullptr;  // GPUDIFF_OPT_SMALL_PASS: pinned read-back buffer of one result image (first use)
    // per-ticket completion hooks run by gpudiff_wait before results are
    // published (the device-encode store resolves its host-deferred events)
    std::unordered_map<gpudiff_ticket, std::function<int(ResultStore&)>> finishers;
    // GPUDIFF_OPT_DEVICE_ENCODE: gpudiff_submit's pairs go through K0 (dstore.cpp, pair mode)
    DStore* pair_store = nullptr;
    gpudiff_path_stats path_stats{};  // GPUDIFF_OPT_PATH_STRINGS: what the finishers rendered
    gpudiff_path_stats value_stats{};  // GPUDIFF_OPT_PATH_VALUES: the same, counted for the values
    uint64_t render_syncs = 0;  // stream synchronisations of the finishers' text rendering (gpudiff_render_syncs_get)
    FanCtx* fan = nullptr;  // gpudiff_cluster_index_get: statistics, the pinned read-back buffer, events (first use)
    // submit ring
    gpudiff_dbatch* ring[2] = {nullptr, nullptr};
    gpudiff_hbatch* ring_hb[2] = {nullptr, nullptr};
    uint32_t ring_next = 0;
    // persistent host workers (c->threads of them, the calling thread included), made on first use
    std::unique_ptr<gd::WorkerPool> pool;
};

// ------------------------------------------------------------------ helpers
inline gd::WorkerPool& workers(gpudiff_ctx* c) {
    if (!c->pool) c->pool.reset(new gd::WorkerPool(c->threads));
    return *c->pool;
}

// the host path of the n_def documents a kernel deferred: fn(k) for k in [0, n_def), strided over one of the
// context's threads per 64 of them
template <class F>
inline void for_deferred(gpudiff_ctx* c, size_t n_def, F&& fn) {
    if (!n_def) return;
    const uint32_t T = std::max<uint32_t>(1, std::min<uint32_t>(c->threads, (uint32_t)((n_def + 63) / 64)));
    workers(c).run(T, [&](uint32_t t) {
        for (size_t k = t; k < n_def; k += T) fn(k);
    });
}

inline int set_device(gpudiff_ctx* c) {
    if (!c->has_device) return GPUDIFF_E_NODEVICE;
    HIPCHK(hipSetDevice(c->device));
    return GPUDIFF_OK;
}

template <class T>
inline int dalloc(T** p, uint64_t count) {
    *p = nullptr;
    size_t bytes = (size_t)std::max<uint64_t>(count, 1) * sizeof(T);
    HIPCHK(hipMalloc((void**)p, bytes));
    return GPUDIFF_OK;
}

inline void dfree_all(gpudiff_dbatch* d) {
    if (d->pool && !d->pool_borrowed) (void)hipFree(d->pool);
    if (d->base) d->rows = nullptr, d->pair_ids = nullptr, d->desc = nullptr, d->image = nullptr;  // a view's inputs are its base's
    if (d->image) (void)hipFree(d->image);
    if (d->image_scan) (void)hipFree(d->image_scan);
    if (d->image_streamed) (void)hipFree(d->image_streamed);
    if (d->image_built) (void)hipEventDestroy(d->image_built);
    d->image_built = nullptr;
    d->image = nullptr, d->image_scan = nullptr, d->image_streamed = nullptr;
    void* ps[] = {d->rows, d->pair_ids, d->desc, d->flags, d->caps, d->chunk_counts, d->summary, d->spec_ids,
                  d->status_ids, d->dirty_ids, d->dirty_idx, d->scratch_off, d->path_count, d->path_off,
                  d->tile_sums, d->path_src, d->path_cnt, d->arena_h, d->arena_k,
                  d->scratch_h, d->scratch_k, d->out_h, d->out_k, d->nbits, d->noop_d, d->slot_owner,
                  d->slice_cnt, d->slice_weq, d->ids_alt[0], d->ids_alt[1], d->summary_alt, d->tail_perm,
                  d->small_image};
    for (void* p : ps)
        if (p) (void)hipFree(p);
    if (d->done) (void)hipEventDestroy(d->done);
    if (d->fan) fan_buffers_release(d->fan);
}

// copies a finished diff pass's results to host memory (gpudiff_wait's body)
int collect_results(gpudiff_ctx* c, gpudiff_dbatch* d, ResultStore& rs);

// canonical bytes of one object's long string values (V of SURVEY §8(d)); blob at pool + off
inline uint64_t blob_value_bytes(const uint8_t* blob, uint32_t spec_l, uint32_t spec_ar, uint32_t stat_l) {
    uint64_t v = 0;
    const uint32_t* m = (const uint32_t*)(blob + 12ull * spec_l);
    for (uint32_t i = 0; i < spec_l; i++)
        if (gpudiff_meta_is_long(m[i])) v += gpudiff_meta_len(m[i]);
    m = (const uint32_t*)(blob + gpudiff_seg_bytes(spec_l, spec_ar) + 12ull * stat_l);
    for (uint32_t i = 0; i < stat_l; i++)
        if (gpudiff_meta_is_long(m[i])) v += gpudiff_meta_len(m[i]);
    return v;
}

// bytes the decision kernel must read for this pair (DESIGN.md "Roofline"; the same rule as
// k_compare_flat's streamed chunks): gpudiff_format.h gpudiff_pair_compare_bytes
inline uint64_t pair_compare_bytes(const gpudiff_pair_row& r) { return gpudiff_pair_compare_bytes(&r); }
