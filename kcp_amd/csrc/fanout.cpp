// gpudiff_cluster_index_* (include/gpudiff.h): the per-cluster index of a waited pass's dirty IDs,
// built on demand from what the pass left in HBM (kernels K23 - K25, fanout.hip; K26 - K28, fanout_live.hip, for a
// batch whose deferred rows the host resolved), and the same function on the host.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <new>
#include <vector>

#include "../../include/gpudiff.h"
#include "engine.h"
#include "fanout.h"
#include "fanout_dev.h"
#include "scan64.h"

using namespace gd;
using gd::g_last_hip_error;

// The index's device buffers: they live on the batch, grow on demand and are freed with it -- no hipMalloc or hipFree
// per call.  The alternates and the sort's temporary storage exist only once a call has had to sort.
struct FanBuffers {
    uint64_t cap = 0;  // entries: keys at kv[0, cap), vals at kv[cap, 2 cap) (cap is a multiple of 4: 16-byte loads)
    uint32_t* kv = nullptr;
    uint64_t alt_cap = 0;  // the sort's outputs, laid out the same way
    uint32_t* kv_alt = nullptr;
    size_t temp_cap = 0;
    uint8_t* temp = nullptr;
    uint64_t tiles_cap = 0;  // tiles of kFanCols u64
    uint64_t* tiles = nullptr;
    uint64_t* ctl = nullptr;  // [0..2] the totals, [3] K23's control word (its low u32)
    uint64_t block_cap = 0;   // u32 words
    uint32_t* block = nullptr;
    // gpudiff_cluster_index_get_final on a batch with host-resolved rows (K26 - K28), first use
    uint64_t fin_cap = 0;  // bytes: the rows' final flags
    uint8_t* fin = nullptr;
    uint64_t patch_cap = 0;  // the host-resolved rows' final flags as uploaded
    PlanPatch* patch = nullptr;
    uint64_t live_cap = 0;  // entries: live_idx at live[0, live_cap), live_ids at live[live_cap, 2 live_cap)
    uint32_t* live = nullptr;
    uint64_t live_tiles_cap = 0;  // K27's tile sums, one column
    uint64_t* live_tiles = nullptr;
    uint64_t* live_ctl = nullptr;  // [0] the live entries, [1] K26's control word (its low u32): one 16-byte read-back
};

void fan_buffers_release(FanBuffers* f) {
    if (!f) return;
    void* ps[] = {f->kv,  f->kv_alt, f->temp, f->tiles,      f->ctl,     f->block,
                  f->fin, f->patch,  f->live, f->live_tiles, f->live_ctl};
    for (void* p : ps)
        if (p) (void)hipFree(p);
    delete f;
}

// The context's side: statistics, one cached pinned read-back buffer (an index holds it until its release hands it
// back) and the timing events
struct FanCtx {
    gpudiff_cluster_index_stats st{};
    void* pin = nullptr;
    size_t pin_cap = 0;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    gpudiff_cluster_index_final_stats fst{};  // gpudiff_cluster_index_get_final's own
    hipEvent_t evl[4] = {nullptr, nullptr, nullptr, nullptr};  // around K26 + K27 + scan, around K28
};

void fan_ctx_release(FanCtx* f) {
    if (!f) return;
    if (f->pin) (void)hipHostFree(f->pin);
    for (hipEvent_t e : f->ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : f->evl)
        if (e) (void)hipEventDestroy(e);
    delete f;
}

// what gpudiff_cluster_index.internal points at: the arrays' owner
struct FanResult {
    void* pin = nullptr;  // a device-built index: the pinned block
    size_t pin_cap = 0;
    std::vector<uint32_t> host;  // a host-built (or empty) index
};

static int fan_alloc_rc(hipError_t e) {
    if (e == hipSuccess) return GPUDIFF_OK;
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        return GPUDIFF_E_CAPACITY;
    }
    g_last_hip_error = hipGetErrorString(e);
    return GPUDIFF_E_DEVICE;
}

// *p holds at least `need` elements of `elem` bytes afterwards (one eighth of headroom when it has to grow; the
// capacity is a multiple of 4)
template <class T, class N>
static int fan_grow(T** p, N* cap, uint64_t need, size_t elem = sizeof(T)) {
    if (*p && *cap >= need) return GPUDIFF_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    const uint64_t want = (need + need / 8 + 3) & ~3ull;
    int rc = fan_alloc_rc(hipMalloc((void**)p, (size_t)std::max<uint64_t>(want, 1) * elem));
    if (rc) return rc;
    *cap = (N)want;
    return GPUDIFF_OK;
}

static void fill_out(gpudiff_cluster_index* out, const uint32_t* w, const FanLayout& l, uint64_t nc, uint64_t ns,
                     uint64_t nt, uint32_t sorted, FanResult* own) {
    out->n_clusters = (size_t)nc;
    out->cluster_ids = w + l.cluster_ids;
    out->spec_off = w + l.spec_off;
    out->status_off = w + l.status_off;
    out->n_spec = (size_t)ns;
    out->n_status = (size_t)nt;
    out->spec_ids = w + l.spec_ids;
    out->status_ids = w + l.status_ids;
    out->sorted_on_device = sorted;
    out->internal = own;
}

// the index of no dirty row: the two closing offsets, nothing launched, nothing copied
static int fan_empty(gpudiff_cluster_index* out) {
    std::unique_ptr<FanResult> res(new (std::nothrow) FanResult());
    if (!res) return GPUDIFF_E_NOMEM;
    try {
        res->host.assign(2, 0u);
    } catch (const std::bad_alloc&) {
        return GPUDIFF_E_NOMEM;
    }
    fill_out(out, res->host.data(), fan_layout(0, 0, 0), 0, 0, 0, 0, res.get());
    res.release();
    return GPUDIFF_OK;
}

// the batch whose waited results `ticket` stands for
static int fan_waited_batch(gpudiff_ctx* c, gpudiff_ticket ticket, gpudiff_dbatch** out) {
    auto it = c->tickets.find(ticket);
    if (it == c->tickets.end()) return GPUDIFF_E_STATE;  // unknown, or superseded by a later diff of its batch
    gpudiff_dbatch* d = it->second;
    if (d->ticket != ticket || d->waited.ticket != ticket) return GPUDIFF_E_STATE;  // not waited yet
    *out = d;
    return GPUDIFF_OK;
}

static int fan_ctx(gpudiff_ctx* c) {
    if (!c->fan) c->fan = new (std::nothrow) FanCtx();
    return c->fan ? GPUDIFF_OK : GPUDIFF_E_NOMEM;
}

// what one run of fan_build cost, for its caller's statistics (the synchronisations are counted as they happen)
struct FanTally {
    uint64_t* syncs;
    bool sorted = false;
    size_t d2h_bytes = 0;
    bool timed = false;
    double kernel_ms = 0;
};

// Both entry points' tail: K23, the sort when the list does not ascend by cluster, K24, K25, the three read-backs and
// the pinned block, over n > 0 dirty entries k of batch d -- row idx[k], pair id ids[k], final flags flags[idx[k]] --
// on the context stream.  The totals are held to exp_spec / exp_status.
static int fan_build(gpudiff_ctx* c, gpudiff_dbatch* d, const uint32_t* idx, const uint32_t* ids, const uint8_t* flags,
                     uint32_t n, uint32_t exp_spec, uint32_t exp_status, gpudiff_cluster_index* out, FanTally* tally) {
    int rc;
    FanCtx* fc = c->fan;
    std::unique_ptr<FanResult> res(new (std::nothrow) FanResult());
    if (!res) return GPUDIFF_E_NOMEM;
    if (n > 0x7FFFFFFFu || n > d->n_pairs) return GPUDIFF_E_CAPACITY;
    if (!d->fan) {
        d->fan = new (std::nothrow) FanBuffers();
        if (!d->fan) return GPUDIFF_E_NOMEM;
    }
    FanBuffers* fb = d->fan;
    const uint32_t n_tiles = scan64_tiles(n);
    const uint32_t n_pairs = (uint32_t)d->n_pairs;
    if ((rc = fan_grow(&fb->kv, &fb->cap, n, 2 * sizeof(uint32_t)))) return rc;
    if ((rc = fan_grow(&fb->tiles, &fb->tiles_cap, n_tiles, kFanCols * sizeof(uint64_t)))) return rc;
    if (!fb->ctl && (rc = fan_alloc_rc(hipMalloc((void**)&fb->ctl, 4 * sizeof(uint64_t))))) return rc;
    const bool timing = (c->flags & GPUDIFF_OPT_TIMING) != 0;
    if (timing)
        for (hipEvent_t& e : fc->ev)
            if (!e) HIPCHK(hipEventCreate(&e));
    hipStream_t s = c->stream;
    uint32_t *key_in = fb->kv, *val_in = fb->kv + fb->cap;
    uint32_t* ctl_word = (uint32_t*)(fb->ctl + 3);

    // K23, then the first read-back: does the dirty list ascend by cluster?
    if (timing) HIPCHK(hipEventRecord(fc->ev[0], s));
    HIPCHK(launch_fan_keys(s, d->rows, n_pairs, idx, n, key_in, val_in, ctl_word));
    if (timing) HIPCHK(hipEventRecord(fc->ev[1], s));
    uint32_t ctl = 0;
    HIPCHK(hipMemcpyAsync(&ctl, ctl_word, sizeof(ctl), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    ++*tally->syncs;
    if (ctl & kFanBadRow) {
        g_last_hip_error = "cluster index: a dirty entry names no row of the batch";
        return GPUDIFF_E_DEVICE;
    }
    const bool sort = (ctl & kFanUnsorted) != 0;
    const uint32_t *key = key_in, *val = val_in;
    if (sort) {
        if ((rc = fan_grow(&fb->kv_alt, &fb->alt_cap, n, 2 * sizeof(uint32_t)))) return rc;
        if ((rc = fan_grow(&fb->temp, &fb->temp_cap, fan_sort_temp_bytes(n)))) return rc;
    }
    // the sort if needed, K24 and the scan of its tile sums, then the second read-back: the three totals
    if (timing) HIPCHK(hipEventRecord(fc->ev[2], s));
    if (sort) {
        HIPCHK(launch_fan_sort(s, fb->temp, fb->temp_cap, key_in, fb->kv_alt, val_in, fb->kv_alt + fb->alt_cap, n));
        key = fb->kv_alt, val = fb->kv_alt + fb->alt_cap;
    }
    HIPCHK(launch_fan_marks(s, key, val, idx, flags, n_pairs, n, fb->tiles, fb->ctl));
    if (timing) HIPCHK(hipEventRecord(fc->ev[3], s));
    uint64_t tot[kFanCols] = {0, 0, 0};
    HIPCHK(hipMemcpyAsync(tot, fb->ctl, sizeof(tot), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    ++*tally->syncs;
    if (tot[0] == 0 || tot[0] > n || tot[1] != exp_spec || tot[2] != exp_status) {
        g_last_hip_error = "cluster index: the counts disagree with the pass's own";
        return GPUDIFF_E_DEVICE;
    }
    const uint32_t nc = (uint32_t)tot[0], ns = (uint32_t)tot[1], nt = (uint32_t)tot[2];
    const FanLayout l = fan_layout(nc, ns, nt);
    const size_t bytes = (size_t)l.words * sizeof(uint32_t);
    if ((rc = fan_grow(&fb->block, &fb->block_cap, l.words))) return rc;
    // the pinned block the index will own: the context's cached one when it is large enough
    if (fc->pin && fc->pin_cap >= bytes) {
        res->pin = fc->pin, res->pin_cap = fc->pin_cap;
        fc->pin = nullptr, fc->pin_cap = 0;
    } else {
        const size_t want = bytes + bytes / 8;
        if ((rc = fan_alloc_rc(hipHostMalloc(&res->pin, want, hipHostMallocDefault)))) {
            res->pin = nullptr;
            return rc == GPUDIFF_E_CAPACITY ? GPUDIFF_E_NOMEM : rc;
        }
        res->pin_cap = want;
    }
    auto give_back = [&]() {  // an error below: the pinned block returns to the cache or is freed
        gpudiff_cluster_index tmp{};
        tmp.internal = res.release();
        gpudiff_cluster_index_release(c, &tmp);
    };
    // K25 and the one copy of its block: the third synchronisation
    hipError_t e = hipSuccess;
    if (timing) e = hipEventRecord(fc->ev[4], s);
    if (e == hipSuccess) e = launch_fan_emit(s, key, val, idx, ids, flags, n_pairs, n, fb->tiles, nc, ns, nt, fb->block);
    if (e == hipSuccess && timing) e = hipEventRecord(fc->ev[5], s);
    if (e == hipSuccess) e = hipMemcpyAsync(res->pin, fb->block, bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        g_last_hip_error = hipGetErrorString(e);
        give_back();
        return GPUDIFF_E_DEVICE;
    }
    ++*tally->syncs;
    if (timing) {
        float a = 0, b = 0, k = 0;
        if (hipEventElapsedTime(&a, fc->ev[0], fc->ev[1]) == hipSuccess &&
            hipEventElapsedTime(&b, fc->ev[2], fc->ev[3]) == hipSuccess &&
            hipEventElapsedTime(&k, fc->ev[4], fc->ev[5]) == hipSuccess) {
            tally->kernel_ms = (double)a + b + k;
            tally->timed = true;
        }
    }
    tally->sorted = sort;
    tally->d2h_bytes = bytes;
    fill_out(out, (const uint32_t*)res->pin, l, nc, ns, nt, sort ? 1u : 0u, res.get());
    res.release();
    return GPUDIFF_OK;
}

extern "C" {

int gpudiff_cluster_index_host(const uint8_t* flags, const uint32_t* pair_ids, const uint32_t* cluster_ids, size_t n,
                               gpudiff_cluster_index* out) {
    if (!out) return GPUDIFF_E_INVAL;
    memset(out, 0, sizeof(*out));
    if (n > 0xFFFFFFFFull || (n && (!flags || !pair_ids || !cluster_ids))) return GPUDIFF_E_INVAL;
    std::unique_ptr<FanResult> r(new (std::nothrow) FanResult());
    if (!r) return GPUDIFF_E_NOMEM;
    uint64_t nc, ns, nt;
    FanLayout l;
    try {
        l = fan_index_host(flags, pair_ids, cluster_ids, n, r->host, &nc, &ns, &nt);
    } catch (const std::bad_alloc&) {
        return GPUDIFF_E_NOMEM;
    }
    fill_out(out, r->host.data(), l, nc, ns, nt, 0, r.get());
    r.release();
    return GPUDIFF_OK;
}

void gpudiff_cluster_index_release(gpudiff_ctx* c, gpudiff_cluster_index* idx) {
    if (!idx) return;
    FanResult* r = (FanResult*)idx->internal;
    if (r) {
        if (r->pin) {
            FanCtx* f = (c && c->has_device) ? c->fan : nullptr;
            if (f) (void)hipSetDevice(c->device);
            if (f && !f->pin) {  // back into the context's cache for the next call
                f->pin = r->pin;
                f->pin_cap = r->pin_cap;
            } else {
                (void)hipHostFree(r->pin);
            }
        }
        delete r;
    }
    memset(idx, 0, sizeof(*idx));
}

int gpudiff_cluster_index_stats_get(gpudiff_ctx* c, gpudiff_cluster_index_stats* out) {
    if (!c || !out) return GPUDIFF_E_INVAL;
    memset(out, 0, sizeof(*out));
    if (!c->has_device) return GPUDIFF_E_NODEVICE;
    if (c->fan) *out = c->fan->st;
    return GPUDIFF_OK;
}

int gpudiff_cluster_index_get(gpudiff_ctx* c, gpudiff_ticket ticket, gpudiff_cluster_index* out) {
    if (!c || !out) return GPUDIFF_E_INVAL;
    memset(out, 0, sizeof(*out));
    int rc = set_device(c);
    if (rc) return rc;
    gpudiff_dbatch* d = nullptr;
    if ((rc = fan_waited_batch(c, ticket, &d))) return rc;
    // a store's or a device-encoded submit's batch (its pool is the store's space): the host resolved its deferred
    // rows, so their final flags are not the ones in HBM (gpudiff_cluster_index_get_final serves these)
    if (d->pool_borrowed && !d->base) return GPUDIFF_E_STATE;
    if ((rc = fan_ctx(c))) return rc;
    FanCtx* fc = c->fan;
    const uint32_t n = d->waited.n_dirty;
    if (n == 0) {  // nothing launched, nothing copied
        if ((rc = fan_empty(out))) return rc;
        fc->st.calls++;
        return GPUDIFF_OK;
    }
    FanTally t{&fc->st.syncs};
    if ((rc = fan_build(c, d, d->dirty_idx, d->dirty_ids, d->flags, n, d->waited.n_spec, d->waited.n_status, out, &t)))
        return rc;
    if (t.timed) {
        fc->st.kernel_ms += t.kernel_ms;
        fc->st.timed_calls++;
    }
    fc->st.calls++;
    fc->st.sorted_calls += t.sorted ? 1u : 0u;
    fc->st.entries += n;
    fc->st.d2h_bytes += t.d2h_bytes;
    return GPUDIFF_OK;
}

int gpudiff_cluster_index_final_stats_get(gpudiff_ctx* c, gpudiff_cluster_index_final_stats* out) {
    if (!c || !out) return GPUDIFF_E_INVAL;
    memset(out, 0, sizeof(*out));
    if (!c->has_device) return GPUDIFF_E_NODEVICE;
    if (c->fan) *out = c->fan->fst;
    return GPUDIFF_OK;
}

// The index under the batch's final flags.  Without host-resolved rows the pass's own arrays are final and the tail
// runs over them as it does for gpudiff_cluster_index_get.  With them: K26 makes the per-row final flags, K27 counts
// the entries of the pass's dirty list that are still dirty (held to the host's final count), K28 compacts the list
// when some are not, and the tail runs over that.
int gpudiff_cluster_index_get_final(gpudiff_ctx* c, gpudiff_ticket ticket, gpudiff_cluster_index* out) {
    if (!c || !out) return GPUDIFF_E_INVAL;
    memset(out, 0, sizeof(*out));
    int rc = set_device(c);
    if (rc) return rc;
    gpudiff_dbatch* d = nullptr;
    if ((rc = fan_waited_batch(c, ticket, &d))) return rc;
    // a device-encode store's batch between its ring slot's next submit and that submit's diff, or one whose wait
    // failed: its resolved rows' flags are gone
    if (d->host_resolves && !d->final_patch) return GPUDIFF_E_STATE;
    if ((rc = fan_ctx(c))) return rc;
    FanCtx* fc = c->fan;
    gpudiff_cluster_index_final_stats& st = fc->fst;
    const std::vector<PlanPatch>* patch = d->host_resolves ? d->final_patch : nullptr;
    const uint32_t np = patch ? (uint32_t)patch->size() : 0u;
    const uint32_t n_fin = d->waited.n_dirty, n_dev = d->waited.n_dev_dirty;
    const uint32_t n_pairs = (uint32_t)d->n_pairs;
    FanTally t{&st.syncs};
    const uint32_t *idx = d->dirty_idx, *ids = d->dirty_ids;
    const uint8_t* flags = d->flags;
    uint32_t n = n_dev;
    bool compacted = false;
    double live_ms = 0;
    bool live_timed = false;
    if (np == 0) {
        if (n_dev != n_fin) {  // no row was resolved, so the pass's list is the final one
            g_last_hip_error = "cluster index: the final dirty count differs from the pass's without a resolved row";
            return GPUDIFF_E_DEVICE;
        }
        if (n == 0) rc = fan_empty(out);
        else rc = fan_build(c, d, idx, ids, flags, n, d->waited.n_spec, d->waited.n_status, out, &t);
        if (rc) return rc;
    } else if (n_fin == 0) {
        if ((rc = fan_empty(out))) return rc;  // the host resolved every dirty row clean: nothing is launched
        n = 0;
    } else {
        if (n_fin > n_dev) {  // the final dirty set is a subset of the pass's list
            g_last_hip_error = "cluster index: more final dirty rows than entries of the pass's dirty list";
            return GPUDIFF_E_DEVICE;
        }
        if (n_dev > 0x7FFFFFFFu || n_dev > n_pairs) return GPUDIFF_E_CAPACITY;
        if (!d->fan) {
            d->fan = new (std::nothrow) FanBuffers();
            if (!d->fan) return GPUDIFF_E_NOMEM;
        }
        FanBuffers* fb = d->fan;
        if ((rc = fan_grow(&fb->fin, &fb->fin_cap, n_pairs))) return rc;
        if ((rc = fan_grow(&fb->patch, &fb->patch_cap, np))) return rc;
        if ((rc = fan_grow(&fb->live_tiles, &fb->live_tiles_cap, scan64_tiles(n_dev)))) return rc;
        if (!fb->live_ctl && (rc = fan_alloc_rc(hipMalloc((void**)&fb->live_ctl, 2 * sizeof(uint64_t))))) return rc;
        const bool timing = (c->flags & GPUDIFF_OPT_TIMING) != 0;
        if (timing)
            for (hipEvent_t& e : fc->evl)
                if (!e) HIPCHK(hipEventCreate(&e));
        hipStream_t s = c->stream;
        // K26, K27 and the scan of its tile sums, then the one read-back this path adds: the live count and K26's
        // control word
        HIPCHK(hipMemcpyAsync(fb->patch, patch->data(), (size_t)np * sizeof(PlanPatch), hipMemcpyHostToDevice, s));
        if (timing) HIPCHK(hipEventRecord(fc->evl[0], s));
        HIPCHK(launch_fan_patch(s, d->flags, n_pairs, fb->patch, np, fb->fin, (uint32_t*)(fb->live_ctl + 1)));
        HIPCHK(launch_fan_live_marks(s, d->dirty_idx, n_dev, fb->fin, n_pairs, fb->live_tiles, fb->live_ctl));
        if (timing) HIPCHK(hipEventRecord(fc->evl[1], s));
        uint64_t lc[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(lc, fb->live_ctl, sizeof(lc), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        st.syncs++;
        if ((uint32_t)lc[1] & kFanBadRow) {
            g_last_hip_error = "cluster index: a host-resolved row is no row of the batch";
            return GPUDIFF_E_DEVICE;
        }
        if (lc[0] != n_fin) {  // also a final-dirty row that the pass's list does not hold
            g_last_hip_error = "cluster index: the live entries disagree with the final dirty count";
            return GPUDIFF_E_DEVICE;
        }
        flags = fb->fin;
        if (n_fin < n_dev) {  // K28: the live entries alone
            if ((rc = fan_grow(&fb->live, &fb->live_cap, n_fin, 2 * sizeof(uint32_t)))) return rc;
            uint32_t *live_idx = fb->live, *live_ids = fb->live + fb->live_cap;
            if (timing) HIPCHK(hipEventRecord(fc->evl[2], s));
            HIPCHK(launch_fan_live_emit(s, d->dirty_idx, d->dirty_ids, n_dev, fb->fin, n_pairs, fb->live_tiles, n_fin,
                                        live_idx, live_ids));
            if (timing) HIPCHK(hipEventRecord(fc->evl[3], s));
            idx = live_idx, ids = live_ids, n = n_fin;
            compacted = true;
        }
        if ((rc = fan_build(c, d, idx, ids, flags, n, d->waited.n_spec, d->waited.n_status, out, &t))) return rc;
        if (timing) {  // the events have completed: fan_build synchronised behind them
            float a = 0, b = 0;
            if (hipEventElapsedTime(&a, fc->evl[0], fc->evl[1]) == hipSuccess &&
                (!compacted || hipEventElapsedTime(&b, fc->evl[2], fc->evl[3]) == hipSuccess)) {
                live_ms = (double)a + b;
                live_timed = true;
            }
        }
        st.h2d_bytes += (uint64_t)np * sizeof(PlanPatch);
    }
    if (t.timed && (np == 0 || n_fin == 0 || live_timed)) {
        st.kernel_ms += t.kernel_ms + live_ms;
        st.timed_calls++;
    }
    st.calls++;
    st.patched_calls += np ? 1u : 0u;
    st.compacted_calls += compacted ? 1u : 0u;
    st.sorted_calls += t.sorted ? 1u : 0u;
    st.entries_in += n_dev;
    st.entries_live += n_fin;
    st.patch_rows += np;
    st.d2h_bytes += t.d2h_bytes;
    return GPUDIFF_OK;
}

}  // extern "C"
