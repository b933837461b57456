// gpudiff_cluster_index_* (include/gpudiff.h): the per-cluster index of a waited pass's dirty IDs,
// built on demand from what the pass left in HBM (kernels K23 - K25, fanout.hip), and the same function on the host.
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
};

void fan_buffers_release(FanBuffers* f) {
    if (!f) return;
    void* ps[] = {f->kv, f->kv_alt, f->temp, f->tiles, f->ctl, f->block};
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
};

void fan_ctx_release(FanCtx* f) {
    if (!f) return;
    if (f->pin) (void)hipHostFree(f->pin);
    for (hipEvent_t e : f->ev)
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
    auto it = c->tickets.find(ticket);
    if (it == c->tickets.end()) return GPUDIFF_E_STATE;  // unknown, or superseded by a later diff of its batch
    gpudiff_dbatch* d = it->second;
    if (d->ticket != ticket || d->waited.ticket != ticket) return GPUDIFF_E_STATE;  // not waited yet
    // a store's or a device-encoded submit's batch (its pool is the store's space): the host resolved its deferred
    // rows, so their final flags are not the ones in HBM
    if (d->pool_borrowed && !d->base) return GPUDIFF_E_STATE;
    if (!c->fan) {
        c->fan = new (std::nothrow) FanCtx();
        if (!c->fan) return GPUDIFF_E_NOMEM;
    }
    FanCtx* fc = c->fan;
    std::unique_ptr<FanResult> res(new (std::nothrow) FanResult());
    if (!res) return GPUDIFF_E_NOMEM;
    const uint32_t n = d->waited.n_dirty;
    if (n == 0) {  // nothing launched, nothing copied
        try {
            res->host.assign(2, 0u);  // the two closing offsets
        } catch (const std::bad_alloc&) {
            return GPUDIFF_E_NOMEM;
        }
        fill_out(out, res->host.data(), fan_layout(0, 0, 0), 0, 0, 0, 0, res.get());
        res.release();
        fc->st.calls++;
        return GPUDIFF_OK;
    }
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
    HIPCHK(launch_fan_keys(s, d->rows, n_pairs, d->dirty_idx, n, key_in, val_in, ctl_word));
    if (timing) HIPCHK(hipEventRecord(fc->ev[1], s));
    uint32_t ctl = 0;
    HIPCHK(hipMemcpyAsync(&ctl, ctl_word, sizeof(ctl), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    fc->st.syncs++;
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
    HIPCHK(launch_fan_marks(s, key, val, d->dirty_idx, d->flags, n_pairs, n, fb->tiles, fb->ctl));
    if (timing) HIPCHK(hipEventRecord(fc->ev[3], s));
    uint64_t tot[kFanCols] = {0, 0, 0};
    HIPCHK(hipMemcpyAsync(tot, fb->ctl, sizeof(tot), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    fc->st.syncs++;
    if (tot[0] == 0 || tot[0] > n || tot[1] != d->waited.n_spec || tot[2] != d->waited.n_status) {
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
    if (e == hipSuccess)
        e = launch_fan_emit(s, key, val, d->dirty_idx, d->dirty_ids, d->flags, n_pairs, n, fb->tiles, nc, ns, nt,
                            fb->block);
    if (e == hipSuccess && timing) e = hipEventRecord(fc->ev[5], s);
    if (e == hipSuccess) e = hipMemcpyAsync(res->pin, fb->block, bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        g_last_hip_error = hipGetErrorString(e);
        give_back();
        return GPUDIFF_E_DEVICE;
    }
    fc->st.syncs++;
    if (timing) {
        float a = 0, b = 0, k = 0;
        if (hipEventElapsedTime(&a, fc->ev[0], fc->ev[1]) == hipSuccess &&
            hipEventElapsedTime(&b, fc->ev[2], fc->ev[3]) == hipSuccess &&
            hipEventElapsedTime(&k, fc->ev[4], fc->ev[5]) == hipSuccess) {
            fc->st.kernel_ms += (double)a + b + k;
            fc->st.timed_calls++;
        }
    }
    fc->st.calls++;
    fc->st.sorted_calls += sort ? 1u : 0u;
    fc->st.entries += n;
    fc->st.d2h_bytes += bytes;
    fill_out(out, (const uint32_t*)res->pin, l, nc, ns, nt, sort ? 1u : 0u, res.get());
    res.release();
    return GPUDIFF_OK;
}

}  // extern "C"
