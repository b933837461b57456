// Write path, the host's side: the request body the syncer sends for a dirty object, as Go
// writes it.  Kernel K10 renders the same bytes on the device and leaves some documents (floats, duplicate keys, Go
// decode errors, ...) to this path (upsert.cpp).
//
// The Go-exact restatement:
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
#include "go_marshal.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <charconv>
#include <new>
#include <unordered_map>
#include <vector>

using namespace gd;

namespace {

const char kHex[] = "0123456789abcdef";

// encodeState.string(s, escapeHTML = true) of Go 1.16.  kAnyBytes false: s is a decoded string, valid UTF-8 (json.cpp
// repairs), and its non-ASCII bytes are copied; true: s is arbitrary bytes, and every byte utf8.DecodeRuneInString
// rejects (RuneError, width 1) is written as "\ufffd".  One function, so that the escapes are stated once -- and in
// the loop: as a helper of two writers the ASCII rules made a marshalled body about a quarter slower (measured).
template <bool kAnyBytes>
void put_string(std::string& o, const uint8_t* s, size_t n) {
    o.push_back('"');
    for (size_t i = 0; i < n; i++) {
        const uint8_t c = s[i];
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
        } else if (c == 0xE2 && i + 2 < n && s[i + 1] == 0x80 && (s[i + 2] == 0xA8 || s[i + 2] == 0xA9)) {
            o += "\\u202";
            o.push_back(s[i + 2] == 0xA8 ? '8' : '9');
            i += 2;
        } else if (!kAnyBytes) {
            o.push_back((char)c);
        } else {
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
            } else {
                o.append((const char*)s + i, need + 1);
                i += need;
            }
        }
    }
    o.push_back('"');
}
void put_str(std::string& o, const char* s, size_t n) { put_string<false>(o, (const uint8_t*)s, n); }
void put_go_str(std::string& o, const uint8_t* s, size_t n) { put_string<true>(o, s, n); }

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

bool key_is(const Member& m, const char* k) { return m.klen == strlen(k) && memcmp(m.k, k, m.klen) == 0; }

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

// a string value of the decoded object, or "" where Go's accessor finds none
struct Str {
    const char* p = "";
    size_t n = 0;
};
Str str_member(const Node& obj, const char* k) {
    const Member* m = find(obj, k);
    return m && m->v.t == J_STR ? Str{m->v.u.s, m->v.n} : Str{};
}

// the kcp.dev/owned-by label of a metadata map, which only the spec mode reads: GetLabels() is NestedStringMap (nil
// unless every value is a string)
Str owned_by(const Node& md, uint32_t mode) {
    const Member* lb = mode == GPUDIFF_UPSERT_SPEC ? find(md, "labels") : nullptr;
    if (!lb || lb->v.t != J_OBJ) return Str{};
    for (uint32_t i = 0; i < lb->v.n; i++)
        if (lb->v.u.mem[i].v.t != J_STR) return Str{};
    return str_member(lb->v, "kcp.dev/owned-by");
}

// Unstructured.GetOwnerReferences -> filter -> SetOwnerReferences, written as
// ToUnstructured(&OwnerReference) maps (apiVersion, blockOwnerDeletion?,
// controller?, kind, name, uid).  Returns false when the field is removed
// (no reference kept: the Go slice stays nil, specsyncer.go:101-108).
bool put_owner_refs(std::string& o, const Node& refs, const Str& owned) {
    if (refs.t != J_ARR || refs.n == 0) return false;
    for (uint32_t i = 0; i < refs.n; i++)
        if (refs.u.items[i].t != J_OBJ) return false;  // GetOwnerReferences: nil
    size_t kept = 0;
    std::string tmp;
    for (uint32_t i = 0; i < refs.n; i++) {
        const Node& e = refs.u.items[i];
        const Str name = str_member(e, "name");
        if (name.n == owned.n && memcmp(name.p, owned.p, name.n) == 0) continue;  // reference.Name == ownedByLabel
        if (kept++) tmp.push_back(',');
        const Str api = str_member(e, "apiVersion");
        tmp += "{\"apiVersion\":";
        put_str(tmp, api.p, api.n);
        const Member* b = find(e, "blockOwnerDeletion");
        if (b && (b->v.t == J_TRUE || b->v.t == J_FALSE)) tmp += b->v.t == J_TRUE ? ",\"blockOwnerDeletion\":true" : ",\"blockOwnerDeletion\":false";
        const Member* c = find(e, "controller");
        if (c && (c->v.t == J_TRUE || c->v.t == J_FALSE)) tmp += c->v.t == J_TRUE ? ",\"controller\":true" : ",\"controller\":false";
        for (const char* k : {"kind", "name", "uid"}) {
            const Str v = str_member(e, k);
            tmp.append(",\"").append(k).append("\":");
            put_str(tmp, v.p, v.n);
        }
        tmp.push_back('}');
    }
    if (!kept) return false;
    o.push_back('[');
    o += tmp;
    o.push_back(']');
    return true;
}

// The transform of `mode` (upsertIntoDownstream / updateStatusInUpstream, above) over one member of a metadata map
// whose owned-by label is `owned`: false = the member is dropped (uid and resourceVersion; in the spec mode,
// ownerReferences with no reference kept), otherwise its value's text is appended to o.
bool put_meta_member(std::string& o, const Member& x, uint32_t mode, const Str& owned) {
    if (key_is(x, "uid") || key_is(x, "resourceVersion")) return false;
    if (mode == GPUDIFF_UPSERT_SPEC && key_is(x, "ownerReferences")) return put_owner_refs(o, x.v, owned);
    put_value(o, x.v);
    return true;
}

// Go string order of a member's key against a literal
int key_cmp(const Member* m, const char* lit) {
    const size_t ll = strlen(lit);
    const int c = memcmp(m->k, lit, std::min<size_t>(m->klen, ll));
    return c != 0 ? c : m->klen < ll ? -1 : m->klen > ll ? 1 : 0;
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

// a host-only entry point's result into the caller's buffer
int give(const std::string& o, uint8_t* out, size_t cap, size_t* out_len) {
    *out_len = o.size();
    if (o.size() > cap || (!out && o.size())) return GPUDIFF_E_CAPACITY;
    if (o.size()) memcpy(out, o.data(), o.size());
    return GPUDIFF_OK;
}

// a document's body into the caller's buffer and its descriptors into *d, which a Go decode error leaves all zero
int host_body_out(const uint8_t* doc, size_t len, uint32_t mode, uint8_t* out, size_t cap, size_t* out_len,
                  HostDesc* d) {
    if ((!doc && len) || !out_len || mode > GPUDIFF_UPSERT_STATUS) return GPUDIFF_E_INVAL;
    std::string o;
    if (host_body(doc ? doc : (const uint8_t*)"", len, mode, o, d)) return give(o, out, cap, out_len);
    *out_len = 0;
    return GPUDIFF_E_DECODE;
}

}  // namespace

namespace gd {

uint32_t go_float_text(double f, char* out) {
    std::string s;
    put_float(s, f);
    memcpy(out, s.data(), std::min<size_t>(s.size(), 32));
    return (uint32_t)s.size();
}

void upsert_body(const Node& root, uint32_t mode, std::string& o, HostDesc* d) {
    o.clear();
    const Member* md = find(root, "metadata");
    const bool md_map = md && md->v.t == J_OBJ;
    // RemoveNestedField / SetNestedField are no-ops without a metadata map
    const Str owned = md_map ? owned_by(md->v, mode) : Str{};
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
        std::string val;
        for (const Member* x : sorted_members(md->v)) {
            val.clear();
            if (!put_meta_member(val, *x, mode, owned)) continue;
            if (!f2) o.push_back(',');
            f2 = false;
            put_str(o, x->k, x->klen);
            o.push_back(':');
            // NestedString(obj, "metadata", field): the decoded key byte for byte (the parser kept the last of
            // duplicates), a string value
            const int k = x->v.t != J_STR ? -1 : key_is(*x, "name") ? 0 : key_is(*x, "namespace") ? 1 : -1;
            if (k >= 0) {  // between val's quotes
                tgt.off[k] = (uint32_t)(o.size() + 1);
                tgt.len[k] = (uint32_t)(val.size() - 2);
                const bool esc = memchr(val.data() + 1, '\\', tgt.len[k]) != nullptr;
                tgt.flags |= (GPUDIFF_TGT_NAME | (esc ? GPUDIFF_TGT_NAME_ESC : 0u)) << (2 * k);
            }
            o += val;
            meta_pt.member(key_cmp(x, "resourceVersion"), o.size());
        }
        o.push_back('}');
    }
    o.push_back('}');
    o.push_back('\n');
    if (d) *d = HostDesc{md_map ? meta_pt.done(0) : md ? RvSplice{} : root_pt.done(GPUDIFF_RV_WRAP), tgt};
}

void target_strings(const Node& root, const char** p, size_t* n) {
    static const char* const kField[2] = {"name", "namespace"};
    const Member* md = find(root, "metadata");
    for (int k = 0; k < 2; k++) {  // NestedString(obj, "metadata", field): "" unless the whole path is there
        const Str v = md && md->v.t == J_OBJ ? str_member(md->v, kField[k]) : Str{};
        p[k] = v.p;
        n[k] = v.n;
    }
}

// SetResourceVersion(rv) = SetNestedField(obj, rv, "metadata", "resourceVersion") -- written as that: the members of
// the map the field is set in are rendered one by one, the new member joins them, and they are written in key order.
void update_body(const Node& root, uint32_t mode, const uint8_t* rv, size_t rv_len, std::string& o) {
    const Member* md = find(root, "metadata");
    if (!rv_len || (md && md->v.t != J_OBJ)) {  // RemoveNestedField; SetNestedField's error, dropped
        upsert_body(root, mode, o, nullptr);
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
        const Str owned = owned_by(md->v, mode);
        for (uint32_t i = 0; i < md->v.n; i++) {
            const Member& x = md->v.u.mem[i];
            Item it{std::string(x.k, x.klen), std::string()};
            if (put_meta_member(it.text, x, mode, owned)) meta.push_back(std::move(it));
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

bool host_body(const uint8_t* doc, size_t len, uint32_t mode, std::string& o, HostDesc* d) {
    JsonParser jp;
    Arena arena;
    Node root;
    if (!jp.parse_object(doc, len, arena, &root)) return false;
    upsert_body(root, mode, o, d);
    return true;
}

}  // namespace gd

// ------------------------------------------------------------------ C-ABI: the entry points with no device work
extern "C" {

int gpudiff_upsert_body_host(const uint8_t* doc, size_t len, uint32_t mode, uint8_t* out, size_t cap,
                             size_t* out_len) {
    HostDesc d;
    return host_body_out(doc, len, mode, out, cap, out_len, &d);
}

int gpudiff_upsert_body_host_rv(const uint8_t* doc, size_t len, uint32_t mode, uint8_t* out, size_t cap,
                                size_t* out_len, uint32_t* off, uint32_t* form) {
    if (!off || !form) return GPUDIFF_E_INVAL;
    HostDesc d;
    const int rc = host_body_out(doc, len, mode, out, cap, out_len, &d);
    if (rc != GPUDIFF_E_INVAL) *off = d.rv.off, *form = d.rv.form;
    return rc;
}

int gpudiff_upsert_body_host_targets(const uint8_t* doc, size_t len, uint32_t mode, uint8_t* out, size_t cap,
                                     size_t* out_len, uint32_t* off, uint32_t* tlen, uint32_t* flags) {
    if (!off || !tlen || !flags) return GPUDIFF_E_INVAL;
    HostDesc d;
    const int rc = host_body_out(doc, len, mode, out, cap, out_len, &d);
    if (rc == GPUDIFF_E_INVAL) return rc;
    for (int k = 0; k < 2; k++) {
        off[k] = d.tgt.off[k];
        tlen[k] = d.tgt.len[k];
    }
    *flags = d.tgt.flags;
    return rc;
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

}  // extern "C"
