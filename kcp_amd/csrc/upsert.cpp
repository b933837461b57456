// Write path: the request body the syncer sends for a
// dirty object, on the device (kernel K10, marshal mode of k_encode_docs) with
// the host completing the documents K10 leaves (floats, duplicate keys, Go
// decode errors, ...).
//
// This file is the C-ABI that touches the device and the assembly of a set of bodies from K10's and the host's.
// The host path itself, the Go-exact restatement, is go_marshal.cpp.
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "doc_batch.h"
#include "dstore.h"
#include "engine.h"
#include "go_marshal.h"
#include "tokenize.h"

using namespace gd;

struct gpudiff_wbatch : DocBatch {
    uint32_t n = 0, mode = 0;
    std::vector<const uint8_t*> src;
    std::vector<size_t> lens;
    uint64_t out_bytes = 0, body_bytes = 0;
    void *d_out = nullptr, *d_res = nullptr;
};

namespace {

struct BodiesStore {
    std::vector<uint64_t> offsets;
    std::vector<uint8_t> bytes;
    std::vector<int32_t> status, k10;
    std::vector<uint8_t> source;
    // per body, where its resourceVersion member goes (gpudiff_bodies_rv_splice), and who computed it
    std::vector<uint32_t> rv_off;
    std::vector<uint8_t> rv_form;
    size_t rv_device = 0, rv_host = 0;
    // per body, its request target (gpudiff_bodies_targets): off / len hold [2w] name, [2w + 1] namespace.  Not
    // there (has_tgt false) for a store plan that was not asked for them
    std::vector<uint32_t> tgt_off, tgt_len;
    std::vector<uint8_t> tgt_flags;
    bool has_tgt = false;
    void set_targets(size_t w, const Targets& t) {
        for (int k = 0; k < 2; k++) {
            tgt_off[2 * w + k] = t.off[k];
            tgt_len[2 * w + k] = t.len[k];
        }
        tgt_flags[w] = (uint8_t)t.flags;
    }
    void clear_targets(size_t nw) {
        tgt_off.assign(2 * nw, 0);
        tgt_len.assign(2 * nw, 0);
        tgt_flags.assign(nw, 0);
        has_tgt = true;
    }
};

struct PlanStore {
    std::vector<uint32_t> pair_index;
    std::vector<uint8_t> kind, noop;
};

// K10's target words (tokenize.h TargetWords: a TokOut's, or a store plan write's)
Targets targets_of(const TargetWords& g) {
    Targets t;
    t.off[0] = target_name_off(g);
    t.len[0] = target_name_len(g);
    t.off[1] = target_ns_off(g);
    t.len[1] = target_ns_len(g);
    t.flags = target_flags(g);
    return t;
}

// the finished bodies to the caller, who owns them from here (gpudiff_bodies_release)
void publish(std::unique_ptr<BodiesStore> bs, gpudiff_bodies* out, size_t n, size_t n_host) {
    out->n = n;
    out->offsets = bs->offsets.data();
    out->bytes = bs->bytes.data();
    out->status = bs->status.data();
    out->source = bs->source.data();
    out->k10_status = bs->k10.data();
    out->n_host = n_host;
    out->internal = bs.release();
}

// a plan's writes and their finished bodies to the caller (gpudiff_write_plan_release)
int finish_plan(std::unique_ptr<BodiesStore> bs, std::unique_ptr<PlanStore> ps, size_t n_host,
                gpudiff_write_plan* out) {
    const size_t nw = ps->pair_index.size();
    publish(std::move(bs), &out->bodies, nw, n_host);
    out->n = nw;
    out->pair_index = ps->pair_index.data();
    out->kind = ps->kind.data();
    out->noop = ps->noop.data();
    out->internal = ps.release();
    return GPUDIFF_OK;
}

// One write's body, as assemble_bodies takes it: the device's bytes, the host's, a Go decode error on the host
// path, or none at all (a no-op write)
struct Body {
    enum Kind { kNone, kDevice, kHost, kDecodeError } kind;
    const uint8_t* p;
    size_t n;
    RvSplice rv;  // of a kDevice / kHost body: K10's (TokOut) or the host marshaller's
    Targets tgt;  // likewise
};
const Body kNoBody{Body::kNone, nullptr, 0, RvSplice{}, Targets{}};

// offsets / bytes / status / source of bs for nw writes.  body_of(w) is called exactly once per write, for
// w = 0, 1, ..., nw - 1 in that order: the callers' lambdas count deferred writes and fill bs->k10 as they go
// targets: the bodies carry their request targets (always, but for a store plan that was not asked for them)
template <class F>
void assemble_bodies(BodiesStore* bs, size_t nw, F&& body_of, bool targets = true) {
    bs->offsets.resize(nw + 1);
    bs->status.assign(nw, 0);
    bs->source.assign(nw, GPUDIFF_BODY_DEVICE);
    bs->rv_off.assign(nw, 0);
    bs->rv_form.assign(nw, GPUDIFF_RV_NONE);
    if (targets) bs->clear_targets(nw);
    for (size_t w = 0; w < nw; w++) {
        bs->offsets[w] = bs->bytes.size();
        const Body b = body_of(w);
        if (b.kind == Body::kHost || b.kind == Body::kDecodeError) bs->source[w] = GPUDIFF_BODY_HOST;
        if (b.kind == Body::kDecodeError) bs->status[w] = GPUDIFF_E_DECODE;
        else if (b.kind != Body::kNone) bs->bytes.insert(bs->bytes.end(), b.p, b.p + b.n);
        if (b.kind == Body::kDevice || b.kind == Body::kHost) {
            bs->rv_off[w] = b.rv.off;
            bs->rv_form[w] = (uint8_t)b.rv.form;
            (b.kind == Body::kDevice ? bs->rv_device : bs->rv_host)++;
            if (targets) bs->set_targets(w, b.tgt);
        }
    }
    bs->offsets[nw] = bs->bytes.size();
}

// one document K10 left to the host
struct HostDoc {
    const uint8_t* p;
    size_t n;
    uint32_t mode;
};

// The host path's answers for the n documents K10 deferred: doc_of(k) is deferred document k, marshalled
// (go_marshal.h host_body) on the context's encode threads
struct HostBodies {
    template <class DocOf>
    HostBodies(gpudiff_ctx* c, size_t n, DocOf&& doc_of) : text(n), ok(n, 0), desc(n) {
        for_deferred(c, n, [&](size_t k) {
            const HostDoc d = doc_of(k);
            ok[k] = host_body(d.p, d.n, d.mode, text[k], &desc[k]) ? 1 : 0;
        });
    }
    Body at(size_t k) const {
        return ok[k] ? Body{Body::kHost, (const uint8_t*)text[k].data(), text[k].size(), desc[k].rv, desc[k].tgt}
                      : Body{Body::kDecodeError, nullptr, 0, RvSplice{}, Targets{}};
    }
    std::vector<std::string> text;
    std::vector<uint8_t> ok;
    std::vector<HostDesc> desc;
};

// K10's answer for one write: the body's bytes in `raw` and the descriptors in its TokOut
Body device_body_of(const uint8_t* raw, const TokOut& t) {
    return Body{Body::kDevice, raw + t.off, t.bytes, RvSplice{tokout_rv_off(t), tokout_rv_form(t)},
                targets_of(tokout_targets(t))};
}

}  // namespace

extern "C" {

int gpudiff_bodies_targets(gpudiff_ctx*, const gpudiff_bodies* b, gpudiff_targets* out) {
    if (!b || !out || !b->internal) return GPUDIFF_E_INVAL;
    const BodiesStore* bs = (const BodiesStore*)b->internal;
    if (!bs->has_tgt || bs->tgt_flags.size() != b->n) return GPUDIFF_E_STATE;
    out->n = b->n;
    out->off = bs->tgt_off.data();
    out->len = bs->tgt_len.data();
    out->flags = bs->tgt_flags.data();
    out->n_device = bs->rv_device;  // the same bodies carry both descriptors
    out->n_host = bs->rv_host;
    return GPUDIFF_OK;
}

int gpudiff_bodies_rv_splice(gpudiff_ctx*, const gpudiff_bodies* b, gpudiff_rv_splice* out) {
    if (!b || !out || !b->internal) return GPUDIFF_E_INVAL;
    const BodiesStore* bs = (const BodiesStore*)b->internal;
    if (bs->rv_off.size() != b->n || bs->rv_form.size() != b->n) return GPUDIFF_E_STATE;
    out->n = b->n;
    out->off = bs->rv_off.data();
    out->form = bs->rv_form.data();
    out->n_device = bs->rv_device;
    out->n_host = bs->rv_host;
    return GPUDIFF_OK;
}

int gpudiff_wbatch_create(gpudiff_ctx* c, const uint8_t* const* docs, const size_t* lens, size_t n, uint32_t mode,
                          gpudiff_wbatch** out) {
    if (!c || !out || (n && (!docs || !lens)) || n > 0xFFFFFFFFu || mode > GPUDIFF_UPSERT_STATUS)
        return GPUDIFF_E_INVAL;
    *out = nullptr;
    int rc = set_device(c);
    if (rc) return rc;
    std::unique_ptr<gpudiff_wbatch> wb(new (std::nothrow) gpudiff_wbatch());
    if (!wb) return GPUDIFF_E_NOMEM;
    wb->n = (uint32_t)n;
    wb->mode = mode;
    wb->docs.resize(n);
    wb->src.assign(docs, docs + n);
    wb->lens.assign(lens, lens + n);
    const DocTableBytes B = lay_out_docs(
        wb->docs.data(), n, [&](size_t i) { return lens[i]; }, marshal_scratch_bytes, marshal_out_cap,
        [](size_t, TokDoc& t, uint64_t out_off) { tokdoc_set_marshal_off(t, out_off); });
    wb->out_bytes = B.out_bytes;
    if ((rc = wb->alloc(&wb->d_out, std::max<uint64_t>(B.out_bytes, 256)))) return rc;
    if ((rc = wb->alloc(&wb->d_res, std::max<size_t>(n, 1) * sizeof(TokOut)))) return rc;
    if ((rc = wb->upload(c, B, [&](size_t i) { return docs[i]; }, 2))) return rc;
    *out = wb.release();
    return GPUDIFF_OK;
}

int gpudiff_wbatch_run(gpudiff_ctx* c, gpudiff_wbatch* wb) {
    if (!c || !wb) return GPUDIFF_E_INVAL;
    int rc = set_device(c);
    if (rc) return rc;
    if ((rc = wb->await_timing())) return rc;  // the previous run's duration
    if ((rc = wb->record(c, 0))) return rc;
    HIPCHK(launch_marshal_docs(c->stream, (const TokDoc*)wb->d_docs, wb->n, (const uint8_t*)wb->d_json,
                               (uint8_t*)wb->d_scratch, (uint8_t*)wb->d_out, wb->mode, (TokOut*)wb->d_res));
    return wb->record(c, 1);
}

int gpudiff_wbatch_fetch(gpudiff_ctx* c, gpudiff_wbatch* wb, gpudiff_bodies* out) {
    if (!c || !wb || !out) return GPUDIFF_E_INVAL;
    memset(out, 0, sizeof(*out));
    int rc = set_device(c);
    if (rc) return rc;
    const size_t n = wb->n;
    std::vector<TokOut> to(n);
    std::vector<uint8_t> raw(wb->out_bytes);
    if (n) HIPCHK(hipMemcpyAsync(to.data(), wb->d_res, n * sizeof(TokOut), hipMemcpyDeviceToHost, c->stream));
    if (wb->out_bytes) HIPCHK(hipMemcpyAsync(raw.data(), wb->d_out, wb->out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    wb->fold_timing();
    std::unique_ptr<BodiesStore> bs(new (std::nothrow) BodiesStore());
    if (!bs) return GPUDIFF_E_NOMEM;
    std::vector<uint32_t> def;  // the documents K10 left
    for (size_t i = 0; i < n; i++)
        if (to[i].status != GPUDIFF_TOK_OK) def.push_back((uint32_t)i);
    const HostBodies host(c, def.size(), [&](size_t k) { return HostDoc{wb->src[def[k]], wb->lens[def[k]], wb->mode}; });
    bs->k10.resize(n);
    uint64_t dev_bytes = 0;
    size_t k = 0;
    assemble_bodies(bs.get(), n, [&](size_t i) {
        bs->k10[i] = (int32_t)to[i].status;
        if (to[i].status != GPUDIFF_TOK_OK) return host.at(k++);
        dev_bytes += to[i].bytes;
        return device_body_of(raw.data(), to[i]);
    });
    wb->body_bytes = dev_bytes;
    publish(std::move(bs), out, n, def.size());
    return GPUDIFF_OK;
}

int gpudiff_wbatch_stats_get(const gpudiff_wbatch* wb, gpudiff_wbatch_stats* st) {
    if (!wb || !st) return GPUDIFF_E_INVAL;
    memset(st, 0, sizeof(*st));
    st->n_docs = wb->n;
    for (size_t l : wb->lens) st->json_bytes += l;
    st->body_bytes = wb->body_bytes;
    st->scratch_bytes = wb->scratch_bytes;
    st->out_cap_bytes = wb->out_bytes;
    st->runs = wb->runs;
    st->k10_ms = wb->mean_ms(0);
    return GPUDIFF_OK;
}

void gpudiff_wbatch_free(gpudiff_ctx* c, gpudiff_wbatch* wb) {
    if (!wb) return;
    doc_batch_quiesce(c);
    delete wb;
}

int gpudiff_upsert_bodies(gpudiff_ctx* c, const uint8_t* const* docs, const size_t* lens, size_t n, uint32_t mode,
                          gpudiff_bodies* out) {
    if (!out) return GPUDIFF_E_INVAL;
    memset(out, 0, sizeof(*out));
    gpudiff_wbatch* wb = nullptr;
    int rc = gpudiff_wbatch_create(c, docs, lens, n, mode, &wb);
    if (rc) return rc;
    rc = gpudiff_wbatch_run(c, wb);
    if (!rc) rc = gpudiff_wbatch_fetch(c, wb, out);
    gpudiff_wbatch_free(c, wb);
    return rc;
}

void gpudiff_bodies_release(gpudiff_ctx*, gpudiff_bodies* b) {
    if (!b) return;
    delete (BodiesStore*)b->internal;
    memset(b, 0, sizeof(*b));
}

// ------------------------------------------------------------------ gate -> write on the device
int gpudiff_write_plan_get(gpudiff_ctx* c, gpudiff_ticket ticket, gpudiff_write_plan* out) {
    return gpudiff_write_plan_get_ex(c, ticket, GPUDIFF_PLAN_INFORMER, out);
}

int gpudiff_write_plan_get_ex(gpudiff_ctx* c, gpudiff_ticket ticket, uint32_t mode, gpudiff_write_plan* out) {
    if (!c || !out) return GPUDIFF_E_INVAL;
    if (mode & ~(GPUDIFF_PLAN_SPEC | GPUDIFF_PLAN_STATUS | GPUDIFF_PLAN_UPSTREAM_DOWNSTREAM | GPUDIFF_PLAN_TARGETS))
        return GPUDIFF_E_INVAL;
    mode &= ~GPUDIFF_PLAN_TARGETS;  // the TokOuts come back whole here: the bodies always carry their targets
    const uint32_t kinds = (mode & (GPUDIFF_PLAN_SPEC | GPUDIFF_PLAN_STATUS)) ? mode : (GPUDIFF_PLAN_SPEC | GPUDIFF_PLAN_STATUS);
    // informer pairs (old, new): UpdateFunc enqueues newObj and the worker writes it (specsyncer.go:47-50 ->
    // :86-132, statussyncer.go:32-35 -> :41-63), so both kinds render document 2i+1; (A, B) pairs: the spec
    // write is A's (2i), the status write B's (2i+1)
    const uint32_t spec_side = (mode & GPUDIFF_PLAN_UPSTREAM_DOWNSTREAM) ? 0u : 1u;
    memset(out, 0, sizeof(*out));
    int rc = set_device(c);
    if (rc) return rc;
    StagedPairs sp;
    if ((rc = dstore_staged_pairs(c, ticket, &sp))) return rc;
    const std::vector<uint8_t>& fl = *sp.flags;
    std::unique_ptr<PlanStore> ps(new (std::nothrow) PlanStore());
    if (!ps) return GPUDIFF_E_NOMEM;
    // the writes: spec-dirty pairs, then status-dirty pairs
    for (uint32_t kind = GPUDIFF_UPSERT_SPEC; kind <= GPUDIFF_UPSERT_STATUS; kind++) {
        if (!(kinds & (kind == GPUDIFF_UPSERT_SPEC ? GPUDIFF_PLAN_SPEC : GPUDIFF_PLAN_STATUS))) continue;
        const uint8_t dirty = kind == GPUDIFF_UPSERT_SPEC ? GPUDIFF_SPEC_DIRTY : GPUDIFF_STATUS_DIRTY;
        const uint8_t noop = kind == GPUDIFF_UPSERT_SPEC ? GPUDIFF_SPEC_NOOP : GPUDIFF_STATUS_NOOP;
        for (uint32_t p = 0; p < sp.n; p++)
            if (fl[p] & dirty) {
                ps->pair_index.push_back(p);
                ps->kind.push_back((uint8_t)kind);
                ps->noop.push_back((fl[p] & noop) ? 1 : 0);
            }
    }
    const size_t nw = ps->pair_index.size();
    // K10 documents: the staged document of every write that is not a no-op, read where K0 read it (HBM)
    std::vector<TokDoc> docs;
    std::vector<uint32_t> wdoc(nw, UINT32_MAX);
    uint32_t n_spec_docs = 0;
    uint64_t sb = 0, ob = 0;
    // not lay_out_docs: a document here is a copy of its staged TokDoc and keeps that one's json_off and length
    for (size_t w = 0; w < nw; w++) {
        if (ps->noop[w]) continue;
        const uint32_t di = 2 * ps->pair_index[w] + (ps->kind[w] == GPUDIFF_UPSERT_SPEC ? spec_side : 1u);
        TokDoc t = sp.hdocs[di];
        t.seed = 0;
        t.scratch_off = sb;
        tokdoc_set_marshal_off(t, ob);
        sb += marshal_scratch_bytes(t.json_len);
        ob += marshal_out_cap(t.json_len);
        wdoc[w] = (uint32_t)docs.size();
        docs.push_back(t);
        if (ps->kind[w] == GPUDIFF_UPSERT_SPEC) n_spec_docs++;
    }
    const size_t nd = docs.size();
    std::vector<TokOut> to(nd);
    std::vector<uint8_t> raw(ob);
    if (nd) {
        DocBatch dev;  // owns the device buffers: freed where this block ends or returns, before `to` and `raw` go
        void *d_docs = nullptr, *d_scratch = nullptr, *d_out = nullptr, *d_res = nullptr;
        if ((rc = dev.alloc(&d_docs, nd * sizeof(TokDoc))) || (rc = dev.alloc(&d_scratch, std::max<uint64_t>(sb, 256))) ||
            (rc = dev.alloc(&d_out, std::max<uint64_t>(ob, 256))) || (rc = dev.alloc(&d_res, nd * sizeof(TokOut))))
            return rc;
        HIPCHK(hipMemcpyAsync(d_docs, docs.data(), nd * sizeof(TokDoc), hipMemcpyHostToDevice, c->stream));
        if (n_spec_docs)
            HIPCHK(launch_marshal_docs(c->stream, (const TokDoc*)d_docs, n_spec_docs, sp.djson, (uint8_t*)d_scratch,
                                       (uint8_t*)d_out, GPUDIFF_UPSERT_SPEC, (TokOut*)d_res));
        if (nd > n_spec_docs)
            HIPCHK(launch_marshal_docs(c->stream, (const TokDoc*)d_docs + n_spec_docs, (uint32_t)(nd - n_spec_docs),
                                       sp.djson, (uint8_t*)d_scratch, (uint8_t*)d_out, GPUDIFF_UPSERT_STATUS,
                                       (TokOut*)d_res + n_spec_docs));
        if ((rc = dstore_staged_mark_read(c, ticket))) return rc;
        HIPCHK(hipMemcpyAsync(to.data(), d_res, nd * sizeof(TokOut), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(raw.data(), d_out, ob, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    // K10's deferrals: the host path over the same staged JSON, read back from HBM (the batch may have been
    // uploaded zero-copy from a caller's buffer that is reusable since gpudiff_wait returned, and a staging
    // copy in the ring slot may belong to another batch)
    std::vector<uint32_t> def;
    for (size_t k = 0; k < nd; k++)
        if (to[k].status != GPUDIFF_TOK_OK) def.push_back((uint32_t)k);
    std::vector<uint64_t> hoff(def.size());
    std::vector<uint8_t> hjson;
    if (!def.empty()) {
        // one gather on the device (K7's 16-B copies: staged documents start 16-B aligned and their spans run at
        // least 16 bytes past their ends), then ONE copy back -- not a pageable round trip per document
        std::vector<BlobMove> mv(def.size());
        uint64_t gb = 0;
        for (size_t k = 0; k < def.size(); k++) {
            const TokDoc& d = docs[def[k]];
            mv[k] = BlobMove{d.json_off, gb, ((uint64_t)d.json_len + 15u) & ~15ull};
            hoff[k] = gb;
            gb += mv[k].bytes;
        }
        hjson.resize(gb);
        DocBatch dev;
        void *d_mv = nullptr, *d_gather = nullptr;
        if ((rc = dev.alloc(&d_mv, mv.size() * sizeof(BlobMove))) || (rc = dev.alloc(&d_gather, std::max<uint64_t>(gb, 16))))
            return rc;
        HIPCHK(hipMemcpyAsync(d_mv, mv.data(), mv.size() * sizeof(BlobMove), hipMemcpyHostToDevice, c->stream));
        HIPCHK(launch_move_blobs(c->stream, sp.djson, (uint8_t*)d_gather, (const BlobMove*)d_mv, (uint32_t)mv.size()));
        // the staged JSON's read marker again, behind the last read of it (k0_done covers every read)
        if ((rc = dstore_staged_mark_read(c, ticket))) return rc;
        HIPCHK(hipMemcpyAsync(hjson.data(), d_gather, gb, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    const HostBodies host(c, def.size(), [&](size_t k) {
        return HostDoc{hjson.data() + hoff[k], docs[def[k]].json_len,
                       def[k] < n_spec_docs ? (uint32_t)GPUDIFF_UPSERT_SPEC : (uint32_t)GPUDIFF_UPSERT_STATUS};
    });
    std::unique_ptr<BodiesStore> bs(new (std::nothrow) BodiesStore());
    if (!bs) return GPUDIFF_E_NOMEM;
    bs->k10.assign(nw, GPUDIFF_TOK_OK);
    size_t h = 0;  // the writes' documents ascend with w, so the deferred ones come in def's order
    assemble_bodies(bs.get(), nw, [&](size_t w) {
        if (wdoc[w] == UINT32_MAX) return kNoBody;  // no-op: no body
        const uint32_t k = wdoc[w];
        bs->k10[w] = (int32_t)to[k].status;
        if (to[k].status != GPUDIFF_TOK_OK) return host.at(h++);
        return device_body_of(raw.data(), to[k]);
    });
    return finish_plan(std::move(bs), std::move(ps), def.size(), out);
}

// The store's plan: the device lists the writes and renders the bodies (dstore_write_plan); what is
// left here is the host path for the documents K10 deferred and wrapping the result.
int gpudiff_store_write_plan_get(gpudiff_ctx* c, gpudiff_store* st, gpudiff_ticket ticket, uint32_t mode,
                                 gpudiff_write_plan* out) {
    if (!c || !st || !out) return GPUDIFF_E_INVAL;
    // store events are informer events: there is no (A, B) reading of them
    if (mode & ~(GPUDIFF_PLAN_SPEC | GPUDIFF_PLAN_STATUS | GPUDIFF_PLAN_TARGETS)) return GPUDIFF_E_INVAL;
    const bool targets = (mode & GPUDIFF_PLAN_TARGETS) != 0;
    mode &= ~GPUDIFF_PLAN_TARGETS;
    const uint32_t kinds = mode ? mode : (GPUDIFF_PLAN_SPEC | GPUDIFF_PLAN_STATUS);
    memset(out, 0, sizeof(*out));
    int rc = set_device(c);
    if (rc) return rc;
    DStore* ds = gpudiff_store_dstore(st);
    if (!ds) return GPUDIFF_E_STATE;  // a host-encode store: its JSON never reaches HBM
    StorePlan sp;
    if ((rc = dstore_write_plan(c, ds, ticket, kinds, targets, &sp))) return rc;
    const size_t nw = sp.n, n_def = sp.def.size();
    const HostBodies host(c, n_def, [&](size_t k) {
        return HostDoc{sp.hjson.data() + sp.hoff[k], sp.hlen[k], sp.kind[sp.def[k]]};
    });
    std::unique_ptr<PlanStore> ps(new (std::nothrow) PlanStore());
    std::unique_ptr<BodiesStore> bs(new (std::nothrow) BodiesStore());
    if (!ps || !bs) return GPUDIFF_E_NOMEM;
    ps->pair_index.assign(sp.pair_index, sp.pair_index + nw);
    ps->kind.assign(sp.kind, sp.kind + nw);
    ps->noop.assign(sp.noop, sp.noop + nw);
    bs->k10.assign(sp.k10, sp.k10 + nw);
    if (!n_def) {  // the device's dense bodies are the result as they are
        bs->status.assign(nw, 0);
        bs->source.assign(nw, GPUDIFF_BODY_DEVICE);
        bs->offsets.assign(sp.offsets, sp.offsets + nw + 1);
        bs->bytes.assign(sp.bytes, sp.bytes + sp.offsets[nw]);
        bs->rv_off.assign(sp.rv_off, sp.rv_off + nw);  // K19 left a no-op write's descriptor GPUDIFF_RV_NONE
        bs->rv_form.assign(sp.rv_form, sp.rv_form + nw);
        for (size_t w = 0; w < nw; w++) bs->rv_device += sp.noop[w] ? 0 : 1;
        if (targets) {
            bs->clear_targets(nw);
            for (size_t w = 0; w < nw; w++) bs->set_targets(w, targets_of(sp.tgt[w]));  // a no-op write's: zero
        }
    } else {  // the host's bodies go in between
        size_t k = 0;
        assemble_bodies(bs.get(), nw, [&](size_t w) {
            if (k < n_def && sp.def[k] == w) return host.at(k++);
            if (sp.noop[w]) return kNoBody;
            return Body{Body::kDevice, sp.bytes + sp.offsets[w], (size_t)(sp.offsets[w + 1] - sp.offsets[w]),
                        RvSplice{sp.rv_off[w], sp.rv_form[w]}, targets ? targets_of(sp.tgt[w]) : Targets{}};
        }, targets);
    }
    return finish_plan(std::move(bs), std::move(ps), n_def, out);
}

int gpudiff_store_plan_stats_get(const gpudiff_store* st, gpudiff_store_plan_stats* out) {
    if (!st || !out) return GPUDIFF_E_INVAL;
    memset(out, 0, sizeof(*out));
    DStore* ds = gpudiff_store_dstore(const_cast<gpudiff_store*>(st));
    return ds ? dstore_plan_stats(ds, out) : GPUDIFF_E_STATE;
}

void gpudiff_write_plan_release(gpudiff_ctx* c, gpudiff_write_plan* p) {
    if (!p) return;
    gpudiff_bodies_release(c, &p->bodies);
    delete (PlanStore*)p->internal;
    memset(p, 0, sizeof(*p));
}

}  // extern "C"
