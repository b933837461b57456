// Write path: the request body the syncer sends for a
// dirty object, on the device (kernel K10, marshal mode of k_encode_docs) with
// the host completing the documents K10 leaves (floats, duplicate keys, Go
// decode errors, ...).
//
// The host path here is the Go-exact restatement:
//   * decode with the informer's rules (json.cpp: k8s util/json over Go
//     1.16 encoding/json, duplicate keys last-wins, U+FFFD repair);
//   * transform as upsertIntoDownstream (pkg/syncer/specsyncer.go:94-108:
//     SetUID(""), SetResourceVersion(""), owner references named by the
//     kcp.dev/owned-by label dropped, SetOwnerReferences) or
//     updateStatusInUpstream (pkg/syncer/statussyncer.go:44-48: SetUID(""),
//     SetResourceVersion(""));
//   * marshal as the dynamic client's body, json.NewEncoder(w).Encode(obj):
//     map keys sorted by bytes, encodeState.string with escapeHTML, floats via
//     strconv.AppendFloat(f, 'f' | 'e', -1, 64) with the 1e-6 / 1e21 switch and
//     the e-09 -> e-9 clean-up, trailing '\n'.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <charconv>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "doc_batch.h"
#include "dstore.h"
#include "engine.h"
#include "json.h"
#include "tokenize.h"

using namespace gd;

namespace gd {
// a body's resourceVersion splice point (include/gpudiff.h GPUDIFF_RV_*)
struct RvSplice {
    uint32_t off = 0;
    uint32_t form = GPUDIFF_RV_NONE;
};
// a body's request target (include/gpudiff.h GPUDIFF_TGT_*): [0] metadata.name, [1] metadata.namespace
struct Targets {
    uint32_t off[2] = {0, 0};
    uint32_t len[2] = {0, 0};
    uint32_t flags = 0;
};
}  // namespace gd

namespace {

const char kHex[] = "0123456789abcdef";

void put_str(std::string& o, const char* s, size_t n) {
    o.push_back('"');
    for (size_t i = 0; i < n; i++) {
        const uint8_t c = (uint8_t)s[i];
        if (c < 0x80) {
            if (c == '"' || c == '\\') {
                o.push_back('\\');
                o.push_back((char)c);
            } else if (c == '\n') {
                o += "\\n";
            } else if (c == '\r') {
                o += "\\r";
            } else if (c == '\t') {
                o += "\\t";
            } else if (c < 0x20 || c == '<' || c == '>' || c == '&') {
                o += "\\u00";
                o.push_back(kHex[c >> 4]);
                o.push_back(kHex[c & 15]);
            } else {
                o.push_back((char)c);
            }
        } else if (c == 0xE2 && i + 2 < n && (uint8_t)s[i + 1] == 0x80 &&
                   ((uint8_t)s[i + 2] == 0xA8 || (uint8_t)s[i + 2] == 0xA9)) {
            o += "\\u202";
            o.push_back((uint8_t)s[i + 2] == 0xA8 ? '8' : '9');
            i += 2;
        } else {
            o.push_back((char)c);  // decoded strings are valid UTF-8 (json.cpp repairs)
        }
    }
    o.push_back('"');
}

// floatEncoder(64): strconv.AppendFloat(f, 'f' | 'e', -1, 64).  Go formats the
// shortest round-trip digit string (closest on ties) in the chosen layout, so
// 'f' pads with zeros (2^63 -> "9223372036854776000"); std::to_chars' fixed
// form would print the exact integer instead, so the digits come from its
// scientific form and are laid out here.
void put_float(std::string& o, double f) {
    char b[64];
    auto r = std::to_chars(b, b + sizeof(b) - 1, f, std::chars_format::scientific);
    size_t n = (size_t)(r.ptr - b);
    b[n] = 0;
    const double a = f < 0 ? -f : f;
    if (a != 0 && (a < 1e-6 || a >= 1e21)) {
        if (n >= 4 && b[n - 4] == 'e' && b[n - 3] == '-' && b[n - 2] == '0') {  // e-07 -> e-7
            b[n - 2] = b[n - 1];
            n--;
        }
        o.append(b, n);
        return;
    }
    size_t i = 0;
    if (b[0] == '-') {
        o.push_back('-');
        i = 1;
    }
    std::string dig;
    for (; i < n && b[i] != 'e'; i++)
        if (b[i] != '.') dig.push_back(b[i]);
    const int x = atoi(b + i + 1);  // decimal exponent of the first digit
    const int nd = (int)dig.size();
    if (x >= nd - 1) {
        o += dig;
        o.append((size_t)(x - (nd - 1)), '0');
    } else if (x >= 0) {
        o.append(dig, 0, (size_t)x + 1);
        o.push_back('.');
        o.append(dig, (size_t)x + 1, std::string::npos);
    } else {
        o += "0.";
        o.append((size_t)(-x - 1), '0');
        o += dig;
    }
}

}  // namespace

// put_float for the value renderer (valstr.h's host formatter, devenc.cpp): Go's text of `f` into out (32 bytes
// hold any float64: 24 digits and zeros, sign, "0."), its length returned
namespace gd {
uint32_t go_float_text(double f, char* out) {
    std::string s;
    put_float(s, f);
    memcpy(out, s.data(), std::min<size_t>(s.size(), 32));
    return (uint32_t)s.size();
}
}  // namespace gd

namespace {

const Member* find(const Node& obj, const char* k) {
    const size_t kl = strlen(k);
    for (uint32_t i = 0; i < obj.n; i++)
        if (obj.u.mem[i].klen == kl && memcmp(obj.u.mem[i].k, k, kl) == 0) return &obj.u.mem[i];
    return nullptr;
}

std::vector<const Member*> sorted_members(const Node& obj) {
    std::vector<const Member*> m(obj.n);
    for (uint32_t i = 0; i < obj.n; i++) m[i] = &obj.u.mem[i];
    std::sort(m.begin(), m.end(), [](const Member* a, const Member* b) {
        const int c = memcmp(a->k, b->k, std::min(a->klen, b->klen));
        return c != 0 ? c < 0 : a->klen < b->klen;
    });
    return m;
}

void put_value(std::string& o, const Node& v);

void put_object(std::string& o, const Node& v) {
    o.push_back('{');
    bool first = true;
    for (const Member* m : sorted_members(v)) {
        if (!first) o.push_back(',');
        first = false;
        put_str(o, m->k, m->klen);
        o.push_back(':');
        put_value(o, m->v);
    }
    o.push_back('}');
}

void put_value(std::string& o, const Node& v) {
    switch (v.t) {
        case J_NULL: o += "null"; break;
        case J_FALSE: o += "false"; break;
        case J_TRUE: o += "true"; break;
        case J_INT: {
            char b[24];
            auto r = std::to_chars(b, b + sizeof(b), (long long)v.u.i);
            o.append(b, (size_t)(r.ptr - b));
            break;
        }
        case J_FLOAT: put_float(o, v.u.d); break;
        case J_STR: put_str(o, v.u.s, v.n); break;
        case J_ARR:
            o.push_back('[');
            for (uint32_t i = 0; i < v.n; i++) {
                if (i) o.push_back(',');
                put_value(o, v.u.items[i]);
            }
            o.push_back(']');
            break;
        default: put_object(o, v); break;
    }
}

// Unstructured.GetOwnerReferences -> filter -> SetOwnerReferences, written as
// ToUnstructured(&OwnerReference) maps (apiVersion, blockOwnerDeletion?,
// controller?, kind, name, uid).  Returns false when the field is removed
// (no reference kept: the Go slice stays nil, specsyncer.go:101-108).
bool put_owner_refs(std::string& o, const Node& refs, const char* owned, size_t owned_len) {
    if (refs.t != J_ARR || refs.n == 0) return false;
    for (uint32_t i = 0; i < refs.n; i++)
        if (refs.u.items[i].t != J_OBJ) return false;  // GetOwnerReferences: nil
    size_t kept = 0;
    std::string tmp;
    for (uint32_t i = 0; i < refs.n; i++) {
        const Node& e = refs.u.items[i];
        auto sval = [&](const char* k, const char** p, size_t* n) {
            const Member* m = find(e, k);
            if (m && m->v.t == J_STR) {
                *p = m->v.u.s;
                *n = m->v.n;
            } else {
                *p = "";
                *n = 0;
            }
        };
        const char* np;
        size_t nl;
        sval("name", &np, &nl);
        if (nl == owned_len && memcmp(np, owned, nl) == 0) continue;  // reference.Name == ownedByLabel
        if (kept++) tmp.push_back(',');
        const char* p;
        size_t n;
        tmp += "{\"apiVersion\":";
        sval("apiVersion", &p, &n);
        put_str(tmp, p, n);
        const Member* b = find(e, "blockOwnerDeletion");
        if (b && (b->v.t == J_TRUE || b->v.t == J_FALSE)) tmp += b->v.t == J_TRUE ? ",\"blockOwnerDeletion\":true" : ",\"blockOwnerDeletion\":false";
        const Member* c = find(e, "controller");
        if (c && (c->v.t == J_TRUE || c->v.t == J_FALSE)) tmp += c->v.t == J_TRUE ? ",\"controller\":true" : ",\"controller\":false";
        tmp += ",\"kind\":";
        sval("kind", &p, &n);
        put_str(tmp, p, n);
        tmp += ",\"name\":";
        put_str(tmp, np, nl);
        tmp += ",\"uid\":";
        sval("uid", &p, &n);
        put_str(tmp, p, n);
        tmp.push_back('}');
    }
    if (!kept) return false;
    o.push_back('[');
    o += tmp;
    o.push_back(']');
    return true;
}

}  // namespace

namespace {

// Go string order of a member's key against a literal
int key_cmp(const Member* m, const char* lit) {
    const size_t ll = strlen(lit);
    const int c = memcmp(m->k, lit, std::min<size_t>(m->klen, ll));
    return c != 0 ? c : m->klen < ll ? -1 : m->klen > ll ? 1 : 0;
}

// the kcp.dev/owned-by label of a metadata map: GetLabels() is NestedStringMap (nil unless every value is a string)
void owned_by(const Node& md, const char** owned, size_t* owned_len) {
    *owned = "";
    *owned_len = 0;
    const Member* lb = find(md, "labels");
    if (!lb || lb->v.t != J_OBJ) return;
    for (uint32_t i = 0; i < lb->v.n; i++)
        if (lb->v.u.mem[i].v.t != J_STR) return;
    if (const Member* ob = find(lb->v, "kcp.dev/owned-by")) {
        *owned = ob->v.u.s;
        *owned_len = ob->v.n;
    }
}

// Where a member with a given key goes in the object being written (include/gpudiff.h GPUDIFF_RV_*): fed each
// emitted member in key order, it keeps the end of the last one that sorts before the key.
struct SplicePoint {
    size_t open = 0;  // just past the container's '{'
    size_t before_end = 0;
    bool before = false, after = false;
    void member(int cmp, size_t end) {
        if (cmp < 0) {
            before = true;
            before_end = end;
        } else {
            after = true;
        }
    }
    RvSplice done(uint32_t extra) const {
        RvSplice s;
        s.form = GPUDIFF_RV_INSERT | extra;
        if (before) {
            s.off = (uint32_t)before_end;
            s.form |= GPUDIFF_RV_LEAD;
        } else {
            s.off = (uint32_t)open;
            if (after) s.form |= GPUDIFF_RV_TRAIL;
        }
        return s;
    }
};

// encodeState.string(s, escapeHTML = true) of Go 1.16 over arbitrary bytes: what put_str writes for valid UTF-8,
// and "\ufffd" for every byte utf8.DecodeRuneInString rejects (RuneError, width 1)
void put_go_str(std::string& o, const uint8_t* s, size_t n) {
    o.push_back('"');
    for (size_t i = 0; i < n;) {
        const uint8_t c = s[i];
        if (c < 0x80) {  // put_str's ASCII rules, without its quotes
            const char one = (char)c;
            std::string t;
            put_str(t, &one, 1);
            o.append(t, 1, t.size() - 2);
            i++;
            continue;
        }
        // utf8.DecodeRune's acceptance: the lead byte's length and the second byte's range
        size_t need = 0;
        uint8_t lo = 0x80, hi = 0xBF;
        if (c >= 0xC2 && c <= 0xDF) need = 1;
        else if (c >= 0xE0 && c <= 0xEF) {
            need = 2;
            if (c == 0xE0) lo = 0xA0;
            if (c == 0xED) hi = 0x9F;
        } else if (c >= 0xF0 && c <= 0xF4) {
            need = 3;
            if (c == 0xF0) lo = 0x90;
            if (c == 0xF4) hi = 0x8F;
        }
        bool ok = need != 0 && need < n - i;  // the whole sequence lies inside the string
        if (ok) {
            if (s[i + 1] < lo || s[i + 1] > hi) ok = false;
            for (size_t k = 2; ok && k <= need; k++)
                if (s[i + k] < 0x80 || s[i + k] > 0xBF) ok = false;
        }
        if (!ok) {
            o += "\\ufffd";
            i++;
        } else if (c == 0xE2 && s[i + 1] == 0x80 && (s[i + 2] == 0xA8 || s[i + 2] == 0xA9)) {
            o += "\\u202";
            o.push_back(s[i + 2] == 0xA8 ? '8' : '9');
            i += 3;
        } else {
            o.append((const char*)s + i, need + 1);
            i += need + 1;
        }
    }
    o.push_back('"');
}

}  // namespace

namespace gd {

// The body for one decoded object (root: a J_OBJ); *sp (optional) = where its resourceVersion member would go, *tg
// (optional) = where metadata.name's and metadata.namespace's values stand in it.
void upsert_body(const Node& root, uint32_t mode, std::string& o, RvSplice* sp, Targets* tg) {
    o.clear();
    const Member* md = find(root, "metadata");
    const bool md_map = md && md->v.t == J_OBJ;
    // RemoveNestedField / SetNestedField are no-ops without a metadata map
    const char* owned = "";
    size_t owned_len = 0;
    if (md_map && mode == GPUDIFF_UPSERT_SPEC) owned_by(md->v, &owned, &owned_len);
    SplicePoint root_pt, meta_pt;
    Targets tgt;
    o.push_back('{');
    root_pt.open = o.size();
    bool first = true;
    for (const Member* m : sorted_members(root)) {
        if (!first) o.push_back(',');
        first = false;
        put_str(o, m->k, m->klen);
        o.push_back(':');
        if (m != md || !md_map) {
            put_value(o, m->v);
            root_pt.member(key_cmp(m, "metadata"), o.size());
            continue;
        }
        o.push_back('{');
        meta_pt.open = o.size();
        bool f2 = true;
        for (const Member* x : sorted_members(md->v)) {
            auto is = [&](const char* k) { return x->klen == strlen(k) && memcmp(x->k, k, x->klen) == 0; };
            if (is("uid") || is("resourceVersion")) continue;
            std::string item;
            if (!f2) item.push_back(',');
            put_str(item, x->k, x->klen);
            item.push_back(':');
            if (mode == GPUDIFF_UPSERT_SPEC && is("ownerReferences")) {
                if (!put_owner_refs(item, x->v, owned, owned_len)) continue;
            } else {
                // NestedString(obj, "metadata", field): the decoded key byte for byte (the parser kept the last of
                // duplicates), a string value
                const int k = x->v.t != J_STR ? -1 : is("name") ? 0 : is("namespace") ? 1 : -1;
                const size_t vs = item.size();
                put_value(item, x->v);
                if (k >= 0) {
                    tgt.off[k] = (uint32_t)(o.size() + vs + 1);
                    tgt.len[k] = (uint32_t)(item.size() - vs - 2);
                    const bool esc = memchr(item.data() + vs + 1, '\\', tgt.len[k]) != nullptr;
                    tgt.flags |= (GPUDIFF_TGT_NAME | (esc ? GPUDIFF_TGT_NAME_ESC : 0u)) << (2 * k);
                }
            }
            o += item;
            f2 = false;
            meta_pt.member(key_cmp(x, "resourceVersion"), o.size());
        }
        o.push_back('}');
    }
    o.push_back('}');
    o.push_back('\n');
    if (sp) *sp = md_map ? meta_pt.done(0) : md ? RvSplice{} : root_pt.done(GPUDIFF_RV_WRAP);
    if (tg) *tg = tgt;
}

// Unstructured.GetName() / GetNamespace(): NestedString(obj, "metadata", field) on the decoded object, "" unless the
// whole path is there and ends in a string
void target_strings(const Node& root, const char** p, size_t* n) {
    static const char* const kField[2] = {"name", "namespace"};
    const Member* md = find(root, "metadata");
    for (int k = 0; k < 2; k++) {
        p[k] = "";
        n[k] = 0;
        if (!md || md->v.t != J_OBJ) continue;
        const Member* f = find(md->v, kField[k]);
        if (!f || f->v.t != J_STR) continue;
        p[k] = f->v.u.s;
        n[k] = f->v.n;
    }
}

// The Update body for one decoded object: the transform of `mode`, then SetResourceVersion(rv) =
// SetNestedField(obj, rv, "metadata", "resourceVersion"), then the marshal -- written as that: the members of the
// map the field is set in are rendered one by one, the new member joins them, and they are written in key order.
void update_body(const Node& root, uint32_t mode, const uint8_t* rv, size_t rv_len, std::string& o) {
    const Member* md = find(root, "metadata");
    if (!rv_len || (md && md->v.t != J_OBJ)) {  // RemoveNestedField; SetNestedField's error, dropped
        upsert_body(root, mode, o, nullptr, nullptr);
        return;
    }
    struct Item {
        std::string key, text;
    };
    auto put_items = [](std::string& out, std::vector<Item>& items) {
        std::sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.key < b.key; });
        out.push_back('{');
        for (size_t i = 0; i < items.size(); i++) {
            if (i) out.push_back(',');
            put_str(out, items[i].key.data(), items[i].key.size());
            out.push_back(':');
            out += items[i].text;
        }
        out.push_back('}');
    };
    std::vector<Item> meta;
    if (md) {
        const char* owned = "";
        size_t owned_len = 0;
        if (mode == GPUDIFF_UPSERT_SPEC) owned_by(md->v, &owned, &owned_len);
        for (uint32_t i = 0; i < md->v.n; i++) {
            const Member& x = md->v.u.mem[i];
            Item it{std::string(x.k, x.klen), std::string()};
            if (it.key == "uid" || it.key == "resourceVersion") continue;
            if (mode == GPUDIFF_UPSERT_SPEC && it.key == "ownerReferences") {
                if (!put_owner_refs(it.text, x.v, owned, owned_len)) continue;
            } else {
                put_value(it.text, x.v);
            }
            meta.push_back(std::move(it));
        }
    }
    meta.push_back(Item{"resourceVersion", std::string()});
    put_go_str(meta.back().text, rv, rv_len);
    std::vector<Item> top;
    for (uint32_t i = 0; i < root.n; i++) {
        const Member& m = root.u.mem[i];
        if (&m == md) continue;
        top.push_back(Item{std::string(m.k, m.klen), std::string()});
        put_value(top.back().text, m.v);
    }
    top.push_back(Item{"metadata", std::string()});
    put_items(top.back().text, meta);
    o.clear();
    put_items(o, top);
    o.push_back('\n');
}

}  // namespace gd

// ------------------------------------------------------------------ C-ABI
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

void publish(BodiesStore* bs, gpudiff_bodies* out, size_t n, size_t n_host) {
    out->n = n;
    out->offsets = bs->offsets.data();
    out->bytes = bs->bytes.data();
    out->status = bs->status.data();
    out->source = bs->source.data();
    out->k10_status = bs->k10.data();
    out->n_host = n_host;
    out->internal = bs;
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

// the host path's answer for one deferred write
struct HostDesc {
    RvSplice rv;
    Targets tgt;
};
Body host_body_of(const std::string& body, bool ok, const HostDesc& d) {
    return ok ? Body{Body::kHost, (const uint8_t*)body.data(), body.size(), d.rv, d.tgt}
              : Body{Body::kDecodeError, nullptr, 0, RvSplice{}, Targets{}};
}

// K10's answer for one write: the body's bytes in `raw` and the descriptors in its TokOut
Body device_body_of(const uint8_t* raw, const TokOut& t) {
    return Body{Body::kDevice, raw + t.off, t.bytes, RvSplice{tokout_rv_off(t), tokout_rv_form(t)},
                targets_of(tokout_targets(t))};
}

// host marshal of one document into o, its descriptors into *d; false = Go decode error
bool host_body(const uint8_t* doc, size_t len, uint32_t mode, std::string& o, HostDesc* d) {
    JsonParser jp;
    Arena arena;
    Node root;
    if (!jp.parse_object(doc, len, arena, &root)) return false;
    upsert_body(root, mode, o, &d->rv, &d->tgt);
    return true;
}

// a host-only entry point's result into the caller's buffer
int give(const std::string& o, uint8_t* out, size_t cap, size_t* out_len) {
    *out_len = o.size();
    if (o.size() > cap || (!out && o.size())) return GPUDIFF_E_CAPACITY;
    if (o.size()) memcpy(out, o.data(), o.size());
    return GPUDIFF_OK;
}

}  // namespace

extern "C" {

int gpudiff_upsert_body_host(const uint8_t* doc, size_t len, uint32_t mode, uint8_t* out, size_t cap,
                             size_t* out_len) {
    uint32_t off, form;
    return gpudiff_upsert_body_host_rv(doc, len, mode, out, cap, out_len, &off, &form);
}

int gpudiff_upsert_body_host_targets(const uint8_t* doc, size_t len, uint32_t mode, uint8_t* out, size_t cap,
                                     size_t* out_len, uint32_t* off, uint32_t* tlen, uint32_t* flags) {
    if ((!doc && len) || !out_len || !off || !tlen || !flags || mode > GPUDIFF_UPSERT_STATUS) return GPUDIFF_E_INVAL;
    std::string o;
    HostDesc d;
    off[0] = off[1] = tlen[0] = tlen[1] = *flags = 0;
    if (!host_body(doc ? doc : (const uint8_t*)"", len, mode, o, &d)) {
        *out_len = 0;
        return GPUDIFF_E_DECODE;
    }
    for (int k = 0; k < 2; k++) {
        off[k] = d.tgt.off[k];
        tlen[k] = d.tgt.len[k];
    }
    *flags = d.tgt.flags;
    return give(o, out, cap, out_len);
}

int gpudiff_target_host(const uint8_t* doc, size_t len, uint8_t* name_out, size_t name_cap, size_t* name_len,
                        uint8_t* ns_out, size_t ns_cap, size_t* ns_len) {
    if ((!doc && len) || !name_len || !ns_len) return GPUDIFF_E_INVAL;
    *name_len = *ns_len = 0;
    JsonParser jp;
    Arena arena;
    Node root;
    if (!jp.parse_object(doc ? doc : (const uint8_t*)"", len, arena, &root)) return GPUDIFF_E_DECODE;
    const char* p[2];
    size_t n[2];
    target_strings(root, p, n);
    *name_len = n[0];
    *ns_len = n[1];
    if (n[0] > name_cap || n[1] > ns_cap || (!name_out && n[0]) || (!ns_out && n[1])) return GPUDIFF_E_CAPACITY;
    if (n[0]) memcpy(name_out, p[0], n[0]);
    if (n[1]) memcpy(ns_out, p[1], n[1]);
    return GPUDIFF_OK;
}

int gpudiff_target_decode(const uint8_t* body, size_t body_len, uint32_t off, uint32_t len, uint8_t* out, size_t cap,
                          size_t* out_len) {
    if ((!body && body_len) || !out_len) return GPUDIFF_E_INVAL;
    *out_len = 0;
    if ((uint64_t)off + len > body_len) return GPUDIFF_E_INVAL;
    const uint8_t* const s = body + off;
    auto hex4 = [&](size_t i, uint32_t* v) {  // s[i, i + 4) as a code unit
        if (i + 4 > len) return false;
        *v = 0;
        for (size_t k = 0; k < 4; k++) {
            const uint8_t c = s[i + k];
            const uint32_t d = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10u
                               : c >= 'A' && c <= 'F' ? c - 'A' + 10u : 16u;
            if (d > 15u) return false;
            *v = *v << 4 | d;
        }
        return true;
    };
    size_t w = 0;
    auto put = [&](uint8_t c) {
        if (out && w < cap) out[w] = c;
        w++;
    };
    for (size_t i = 0; i < len;) {
        const uint8_t c = s[i++];
        if (c != '\\') {
            put(c);
            continue;
        }
        if (i >= len) return GPUDIFF_E_INVAL;
        const uint8_t e = s[i++];
        switch (e) {
            case '"': put('"'); break;
            case '\\': put('\\'); break;
            case 'n': put('\n'); break;
            case 'r': put('\r'); break;
            case 't': put('\t'); break;
            case 'b': put('\b'); break;
            case 'f': put('\f'); break;
            case 'u': {
                uint32_t r, lo;
                if (!hex4(i, &r)) return GPUDIFF_E_INVAL;
                i += 4;
                if (r >= 0xD800u && r < 0xDC00u && i + 6 <= len && s[i] == '\\' && s[i + 1] == 'u' && hex4(i + 2, &lo) &&
                    lo >= 0xDC00u && lo < 0xE000u) {
                    r = 0x10000u + ((r - 0xD800u) << 10) + (lo - 0xDC00u);
                    i += 6;
                } else if (r >= 0xD800u && r < 0xE000u) {
                    r = 0xFFFDu;  // a lone surrogate, as Go's decoder reads it
                }
                if (r < 0x80u) {
                    put((uint8_t)r);
                } else if (r < 0x800u) {
                    put((uint8_t)(0xC0u | r >> 6));
                    put((uint8_t)(0x80u | (r & 63u)));
                } else if (r < 0x10000u) {
                    put((uint8_t)(0xE0u | r >> 12));
                    put((uint8_t)(0x80u | ((r >> 6) & 63u)));
                    put((uint8_t)(0x80u | (r & 63u)));
                } else {
                    put((uint8_t)(0xF0u | r >> 18));
                    put((uint8_t)(0x80u | ((r >> 12) & 63u)));
                    put((uint8_t)(0x80u | ((r >> 6) & 63u)));
                    put((uint8_t)(0x80u | (r & 63u)));
                }
                break;
            }
            default: return GPUDIFF_E_INVAL;
        }
    }
    *out_len = w;
    return (w > cap || (!out && w)) ? GPUDIFF_E_CAPACITY : GPUDIFF_OK;
}

int gpudiff_targets_namespaces(const gpudiff_bodies* b, const gpudiff_targets* t, const uint32_t* cluster_ids,
                               const uint8_t* skip, uint32_t* group_of, uint32_t* first, size_t* n_groups) {
    if (!b || !t || !n_groups || t->n != b->n || b->n > 0xFFFFFFFEull) return GPUDIFF_E_INVAL;
    const size_t n = b->n;
    *n_groups = 0;
    if (n && (!group_of || !first || !b->offsets || !b->status || !t->off || !t->len)) return GPUDIFF_E_INVAL;
    std::unordered_map<std::string, uint32_t> groups;
    std::string key;
    try {
        for (size_t w = 0; w < n; w++) {
            group_of[w] = 0xFFFFFFFFu;
            const uint64_t bo = b->offsets[w], bl = b->offsets[w + 1] - bo;
            if ((skip && skip[w]) || b->status[w] != 0 || bl == 0) continue;
            const uint32_t off = t->off[2 * w + 1], len = t->len[2 * w + 1];
            if ((uint64_t)off + len > bl) return GPUDIFF_E_INVAL;
            const uint32_t cl = cluster_ids ? cluster_ids[w] : 0u;
            key.assign((const char*)&cl, sizeof(cl));  // absent and "": both an empty span
            key.append((const char*)b->bytes + bo + off, len);
            const auto it = groups.emplace(key, (uint32_t)groups.size());
            if (it.second) first[it.first->second] = (uint32_t)w;
            group_of[w] = it.first->second;
        }
    } catch (const std::bad_alloc&) {
        return GPUDIFF_E_NOMEM;
    }
    *n_groups = groups.size();
    return GPUDIFF_OK;
}

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

int gpudiff_upsert_body_host_rv(const uint8_t* doc, size_t len, uint32_t mode, uint8_t* out, size_t cap,
                                size_t* out_len, uint32_t* off, uint32_t* form) {
    if ((!doc && len) || !out_len || !off || !form || mode > GPUDIFF_UPSERT_STATUS) return GPUDIFF_E_INVAL;
    std::string o;
    HostDesc d;
    *off = 0;
    *form = GPUDIFF_RV_NONE;
    if (!host_body(doc ? doc : (const uint8_t*)"", len, mode, o, &d)) {
        *out_len = 0;
        return GPUDIFF_E_DECODE;
    }
    *off = d.rv.off;
    *form = d.rv.form;
    return give(o, out, cap, out_len);
}

int gpudiff_update_body_host(const uint8_t* doc, size_t len, uint32_t mode, const uint8_t* rv, size_t rv_len,
                             uint8_t* out, size_t cap, size_t* out_len) {
    if ((!doc && len) || (!rv && rv_len) || !out_len || mode > GPUDIFF_UPSERT_STATUS) return GPUDIFF_E_INVAL;
    JsonParser jp;
    Arena arena;
    Node root;
    if (!jp.parse_object(doc ? doc : (const uint8_t*)"", len, arena, &root)) {
        *out_len = 0;
        return GPUDIFF_E_DECODE;
    }
    std::string o;
    update_body(root, mode, rv, rv_len, o);
    return give(o, out, cap, out_len);
}

int gpudiff_splice_resource_version(const uint8_t* body, size_t len, uint32_t off, uint32_t form, const uint8_t* rv,
                                    size_t rv_len, uint8_t* out, size_t cap, size_t* out_len) {
    constexpr uint32_t kKnown = GPUDIFF_RV_INSERT | GPUDIFF_RV_LEAD | GPUDIFF_RV_TRAIL | GPUDIFF_RV_WRAP;
    if ((!body && len) || (!rv && rv_len) || !out_len) return GPUDIFF_E_INVAL;
    if ((form & ~kKnown) || (form != GPUDIFF_RV_NONE && !(form & GPUDIFF_RV_INSERT)) || off > len)
        return GPUDIFF_E_INVAL;
    const bool insert = form != GPUDIFF_RV_NONE && rv_len != 0;
    if (form != GPUDIFF_RV_NONE && (off == 0 || off >= len)) return GPUDIFF_E_INVAL;  // inside the outer braces
    std::string text;
    if (insert) {
        if (form & GPUDIFF_RV_LEAD) text.push_back(',');
        text += (form & GPUDIFF_RV_WRAP) ? "\"metadata\":{\"resourceVersion\":" : "\"resourceVersion\":";
        put_go_str(text, rv, rv_len);
        if (form & GPUDIFF_RV_WRAP) text.push_back('}');
        if (form & GPUDIFF_RV_TRAIL) text.push_back(',');
    }
    *out_len = len + text.size();
    if (*out_len > cap || (!out && *out_len)) return GPUDIFF_E_CAPACITY;
    const size_t at = insert ? off : len;
    if (at) memcpy(out, body, at);
    if (!text.empty()) memcpy(out + at, text.data(), text.size());
    if (len > at) memcpy(out + at + text.size(), body + at, len - at);
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
    BodiesStore* bs = new (std::nothrow) BodiesStore();
    if (!bs) return GPUDIFF_E_NOMEM;
    // documents K10 left: the host path, on the context's encode threads
    std::vector<uint32_t> def;
    for (size_t i = 0; i < n; i++)
        if (to[i].status != GPUDIFF_TOK_OK) def.push_back((uint32_t)i);
    std::vector<std::string> hb(def.size());
    std::vector<uint8_t> hok(def.size(), 0);
    std::vector<HostDesc> hrv(def.size());
    for_deferred(c, def.size(), [&](size_t k) {
        hok[k] = host_body(wb->src[def[k]], wb->lens[def[k]], wb->mode, hb[k], &hrv[k]) ? 1 : 0;
    });
    bs->k10.resize(n);
    uint64_t dev_bytes = 0;
    size_t k = 0;
    assemble_bodies(bs, n, [&](size_t i) {
        bs->k10[i] = (int32_t)to[i].status;
        if (to[i].status != GPUDIFF_TOK_OK) {
            const size_t h = k++;
            return host_body_of(hb[h], hok[h], hrv[h]);
        }
        dev_bytes += to[i].bytes;
        return device_body_of(raw.data(), to[i]);
    });
    wb->body_bytes = dev_bytes;
    publish(bs, out, n, def.size());
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
struct PlanStore {
    std::vector<uint32_t> pair_index;
    std::vector<uint8_t> kind, noop;
};

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
    void *d_docs = nullptr, *d_scratch = nullptr, *d_out = nullptr, *d_res = nullptr;
    auto cleanup = [&]() {
        for (void* p : {d_docs, d_scratch, d_out, d_res})
            if (p) (void)hipFree(p);
    };
    std::vector<TokOut> to(nd);
    std::vector<uint8_t> raw(ob);
    if (nd) {
        hipError_t e;
        if ((e = hipMalloc(&d_docs, nd * sizeof(TokDoc))) != hipSuccess ||
            (e = hipMalloc(&d_scratch, std::max<uint64_t>(sb, 256))) != hipSuccess ||
            (e = hipMalloc(&d_out, std::max<uint64_t>(ob, 256))) != hipSuccess ||
            (e = hipMalloc(&d_res, nd * sizeof(TokOut))) != hipSuccess) {
            cleanup();
            return e == hipErrorOutOfMemory ? GPUDIFF_E_CAPACITY : GPUDIFF_E_DEVICE;
        }
        hipError_t le = hipMemcpyAsync(d_docs, docs.data(), nd * sizeof(TokDoc), hipMemcpyHostToDevice, c->stream);
        if (le == hipSuccess && n_spec_docs)
            le = launch_marshal_docs(c->stream, (const TokDoc*)d_docs, n_spec_docs, sp.djson, (uint8_t*)d_scratch,
                                     (uint8_t*)d_out, GPUDIFF_UPSERT_SPEC, (TokOut*)d_res);
        if (le == hipSuccess && nd > n_spec_docs)
            le = launch_marshal_docs(c->stream, (const TokDoc*)d_docs + n_spec_docs, (uint32_t)(nd - n_spec_docs),
                                     sp.djson, (uint8_t*)d_scratch, (uint8_t*)d_out, GPUDIFF_UPSERT_STATUS,
                                     (TokOut*)d_res + n_spec_docs);
        if (le == hipSuccess && (rc = dstore_staged_mark_read(c, ticket))) le = hipErrorUnknown;
        if (le == hipSuccess) le = hipMemcpyAsync(to.data(), d_res, nd * sizeof(TokOut), hipMemcpyDeviceToHost, c->stream);
        if (le == hipSuccess) le = hipMemcpyAsync(raw.data(), d_out, ob, hipMemcpyDeviceToHost, c->stream);
        if (le == hipSuccess) le = hipStreamSynchronize(c->stream);
        cleanup();
        if (le != hipSuccess) {
            gd::g_last_hip_error = hipGetErrorString(le);
            return GPUDIFF_E_DEVICE;
        }
    }
    // K10's deferrals: the host path over the same staged JSON, read back from HBM (the batch may have been
    // uploaded zero-copy from a caller's buffer that is reusable since gpudiff_wait returned, and a staging
    // copy in the ring slot may belong to another batch)
    std::vector<uint32_t> def;
    for (size_t k = 0; k < nd; k++)
        if (to[k].status != GPUDIFF_TOK_OK) def.push_back((uint32_t)k);
    std::vector<uint64_t> hoff(def.size() + 1, 0);
    for (size_t k = 0; k < def.size(); k++) hoff[k + 1] = hoff[k] + docs[def[k]].json_len;
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
        void *d_mv = nullptr, *d_gather = nullptr;
        hipError_t e = hipMalloc(&d_mv, mv.size() * sizeof(BlobMove));
        if (e == hipSuccess) e = hipMalloc(&d_gather, std::max<uint64_t>(gb, 16));
        if (e == hipSuccess)
            e = hipMemcpyAsync(d_mv, mv.data(), mv.size() * sizeof(BlobMove), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess)
            e = launch_move_blobs(c->stream, sp.djson, (uint8_t*)d_gather, (const BlobMove*)d_mv, (uint32_t)mv.size());
        // the staged JSON's read marker again, behind the last read of it (k0_done covers every read)
        if (e == hipSuccess && dstore_staged_mark_read(c, ticket)) e = hipErrorUnknown;
        if (e == hipSuccess) e = hipMemcpyAsync(hjson.data(), d_gather, gb, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        for (void* q : {d_mv, d_gather})
            if (q) (void)hipFree(q);
        if (e != hipSuccess) {
            gd::g_last_hip_error = hipGetErrorString(e);
            return GPUDIFF_E_DEVICE;
        }
    }
    std::vector<std::string> hb(def.size());
    std::vector<uint8_t> hok(def.size(), 0);
    std::vector<HostDesc> hrv(def.size());
    const uint32_t mode_split = n_spec_docs;
    for_deferred(c, def.size(), [&](size_t k) {
        hok[k] = host_body(hjson.data() + hoff[k], docs[def[k]].json_len,
                           def[k] < mode_split ? GPUDIFF_UPSERT_SPEC : GPUDIFF_UPSERT_STATUS, hb[k], &hrv[k])
                     ? 1
                     : 0;
    });
    std::vector<int32_t> hidx(nd, -1);
    for (size_t k = 0; k < def.size(); k++) hidx[def[k]] = (int32_t)k;
    BodiesStore* bs = new (std::nothrow) BodiesStore();
    if (!bs) return GPUDIFF_E_NOMEM;
    bs->k10.assign(nw, GPUDIFF_TOK_OK);
    assemble_bodies(bs, nw, [&](size_t w) {
        if (wdoc[w] == UINT32_MAX) return Body{Body::kNone, nullptr, 0, RvSplice{}, Targets{}};  // no-op: no body
        const uint32_t k = wdoc[w];
        bs->k10[w] = (int32_t)to[k].status;
        if (to[k].status != GPUDIFF_TOK_OK) return host_body_of(hb[hidx[k]], hok[hidx[k]], hrv[hidx[k]]);
        return device_body_of(raw.data(), to[k]);
    });
    publish(bs, &out->bodies, nw, def.size());
    out->n = nw;
    out->pair_index = ps->pair_index.data();
    out->kind = ps->kind.data();
    out->noop = ps->noop.data();
    out->internal = ps.release();
    return GPUDIFF_OK;
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
    std::vector<std::string> hb(n_def);
    std::vector<uint8_t> hok(n_def, 0);
    std::vector<HostDesc> hrv(n_def);
    for_deferred(c, n_def, [&](size_t k) {
        hok[k] = host_body(sp.hjson.data() + sp.hoff[k], sp.hlen[k], sp.kind[sp.def[k]], hb[k], &hrv[k]) ? 1 : 0;
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
            if (k < n_def && sp.def[k] == w) {
                const size_t h = k++;
                return host_body_of(hb[h], hok[h], hrv[h]);
            }
            if (sp.noop[w]) return Body{Body::kNone, nullptr, 0, RvSplice{}, Targets{}};
            return Body{Body::kDevice, sp.bytes + sp.offsets[w], (size_t)(sp.offsets[w + 1] - sp.offsets[w]),
                        RvSplice{sp.rv_off[w], sp.rv_form[w]}, targets ? targets_of(sp.tgt[w]) : Targets{}};
        }, targets);
    }
    publish(bs.release(), &out->bodies, nw, n_def);
    out->n = nw;
    out->pair_index = ps->pair_index.data();
    out->kind = ps->kind.data();
    out->noop = ps->noop.data();
    out->internal = ps.release();
    return GPUDIFF_OK;
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
