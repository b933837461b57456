// K10 -- the write path's request bodies: what
// k_encode_docs<MINW, kModeMarshal> runs after phases 1-2 (structural scan, tree).
//
// For one informer object the syncer writes (specsyncer.go:86-110
// upsertIntoDownstream: SetUID(""), SetResourceVersion(""), drop the owner
// references named by the kcp.dev/owned-by label, SetOwnerReferences;
// statussyncer.go:41-48 updateStatusInUpstream: SetUID(""),
// SetResourceVersion("")), this emits the exact bytes the dynamic client
// sends: json.NewEncoder(w).Encode(obj.Object) of Go 1.16 -- map keys sorted
// by bytes, HTML-safe string escaping, no whitespace, trailing newline.
//
// Lane-parallel over the tree's nodes (pre-order ids from phase 2):
//   M1 own text size per node (escaped strings, int64 digits, literals,
//      floats in Go's shortest form via Ryu), escaped key size
//   M2 transform marks (uid / resourceVersion hidden, the ownerReferences
//      and owned-by nodes found), child counts
//   M3 child lists (exclusive scan of the counts + one atomic per child)
//   M4 owner references: each kept element becomes a custom node whose text
//      is the normalized OwnerReference (ToUnstructured: apiVersion,
//      [blockOwnerDeletion], [controller], kind, name, uid)
//   M5 sibling ranks: key byte order for object members (a duplicate key
//      goes to the host: Go's last-wins), array index for elements
//   M6 subtree text sizes bottom-up by depth
//   M7 sibling prefix sums: item sizes laid out by (parent's child base +
//      rank) and one exclusive scan over all of them, so a member's offset
//      in its container is a difference of two prefix values
//   M8 value offsets top-down by depth, visibility
//   M8b the byte offset at which the Update body's `"resourceVersion":"<rv>"` goes, and its commas (marks from M2,
//      ends gathered by M9, settled after it)
//   M8c the request target: where metadata.name's and metadata.namespace's values stand in the body (nodes from M2)
//   M9 emit: every visible node writes its comma, key and value text
// Anything outside this subset keeps a nonzero status and the host marshals
// the document (go_marshal.cpp, the Go-exact path).
#pragma once
#include "tokdev.h"

namespace gd {

namespace {

// K10's per-node words in the document's working area (tokenize.h MarshalLayout)
struct MarshalScratch {
    uint32_t *vsz, *ksz, *sz, *fl, *nch, *base, *kids, *pre, *rank, *vst, *order;
    uint64_t* val;  // an integer's value; a string's len << 32 | in-scratch bit | offset
};
__device__ __forceinline__ MarshalScratch bind_marshal_scratch(uint8_t* work, uint32_t len) {
    const MarshalLayout ML = marshal_layout(len);
    MarshalScratch M;
    M.vsz = (uint32_t*)(work + ML.vsz);
    M.ksz = (uint32_t*)(work + ML.ksz);
    M.sz = (uint32_t*)(work + ML.sz);
    M.fl = (uint32_t*)(work + ML.fl);
    M.nch = (uint32_t*)(work + ML.nch);
    M.base = (uint32_t*)(work + ML.base);
    M.kids = (uint32_t*)(work + ML.kids);
    M.pre = (uint32_t*)(work + ML.pre);
    M.rank = (uint32_t*)(work + ML.rank);
    M.vst = (uint32_t*)(work + ML.vst);
    M.order = (uint32_t*)(work + ML.order);
    M.val = (uint64_t*)(work + ML.val);
    return M;
}

// a string node's decoded bytes (M.val: len << 32 | in-scratch bit | offset)
__device__ __forceinline__ const uint8_t* sptr(const DocTree& T, uint64_t v) {
    const uint32_t off = (uint32_t)v & 0x7FFFFFFFu;
    return ((uint32_t)v & 0x80000000u) ? (T.S.str + off) : (T.d + off);
}
__device__ __forceinline__ uint32_t key_of(const DocTree& T, uint32_t comp, const uint8_t** kp) {
    const uint32_t kt = comp & ~KEYBIT;
    const uint32_t op = T.S.tok[kt] & POS_MASK, cp = T.S.tok[kt + 1] & POS_MASK;
    *kp = T.d + op + 1;
    return cp - op - 1;
}
// a key's first 32 bytes in registers (ld32u reads no word past the document's slack): the names below are
// matched by word compares (field_fold == 1: exact) instead of byte loops, a dependent load per matching byte
__device__ __forceinline__ KeyWin key_win(const DocTree& T, uint32_t comp) {
    const uint8_t* kp;
    const uint32_t kl = key_of(T, comp, &kp);
    return key_window(kp, kl, T.d + T.len + kTokSlack);
}
__device__ __forceinline__ bool is_obj(const DocTree& T, uint32_t i) {  // non-empty object (the root included)
    const uint4 r = T.S.rec[i];
    return !(r.w & NI_LEAF) && (T.S.tok[r.z] >> 24) == '{';
}

// ---------------------------------------------------------- M1 own sizes
// Strings (values and keys, any length) are measured by two flattened wave passes per 64-node window
// (wave_esc_extra: 8-byte units laid end to end, a SWAR test per unit, owner by binary search), so a window costs
// sum(len) / 512 passes; a string whose escaped form equals its bytes is marked clean (MF_VCLEAN /
// MF_KCLEAN) and M9 copies it the same flattened way.
// Returns whether any node is a float (sized by marshal_m1_floats).
__device__ __forceinline__ bool marshal_m1_sizes(const DocTree& T, const MarshalScratch& M, uint32_t& status) {
    const uint8_t* const d = T.d;
    const uint32_t len = T.len, lane = T.lane, nn = T.nn;
    const Scratch& S = T.S;
    bool any_float = false;
    if (status == GPUDIFF_TOK_OK) {
        uint32_t err = GPUDIFF_TOK_OK;
        bool any_float_lane = false;
        for (uint32_t i0 = 0; i0 < nn; i0 += 64) {
            const uint32_t i = i0 + lane;
            bool is_str = false, has_key = false, slow = false;
            uint64_t v = 0;
            uint32_t vsz = 2, fl0 = 0, kl = 0, s_op = 0, s_cp = 0;
            const uint8_t* kp = d;
            if (i < nn) {
                const uint4 r = S.rec[i];
                if (r.w & NI_LEAF) {
                    if (r.w & NI_STR) {
                        const uint32_t op = S.tok[r.z] & POS_MASK, cp = S.tok[r.z + 1] & POS_MASK;
                        v = ((uint64_t)(cp - op - 1) << 32) | (op + 1);
                        is_str = true;
                        slow = (r.w & NI_SLOW) != 0u;  // decoded below, by the whole wave
                        s_op = op;
                        s_cp = cp;
                    } else if (r.w & NI_ATOM) {
                        uint32_t tag = 0;
                        const uint32_t e = parse_atom_quick(d + (S.tok[r.z] & POS_MASK), d + len, &tag, &v);
                        if (e) err = e;
                        else if (tag == GPUDIFF_TAG_FLOAT) {
                            // sized by the float pass below; the canonical value drops -0's sign:
                            // restore it (Go keeps -0.0 and writes "-0")
                            if (v == 0 && d[S.tok[r.z] & POS_MASK] == '-') v = 1ull << 63;
                            fl0 = MF_FLOAT;
                        } else {
                            vsz = tag == GPUDIFF_TAG_INT ? i64_len((int64_t)v) : tag == GPUDIFF_TAG_FALSE ? 5u : 4u;
                        }
                    }
                }
                if (r.y & KEYBIT) {
                    kl = key_of(T, r.y, &kp);
                    has_key = true;
                }
                any_float_lane |= fl0 != 0;
                M.nch[i] = 0;
                M.rank[i] = 0;
            }
            // strings that need decoding: one at a time by the whole wave into S.str at the same offset (a lane's
            // byte-by-byte loop paid a dependent load and store per byte); the owner keeps the decoded length
            const uint64_t sm = ballot(slow);
            for (uint64_t m = sm; m; m &= m - 1) {
                const uint32_t src = (uint32_t)__builtin_ctzll(m);
                const uint32_t sop = rdlane(s_op, src), scp = rdlane(s_cp, src);
                const int dl = wave_decode_string<true>(d + sop + 1, scp - sop - 1, d + len, S.str + sop + 1, lane);
                if (lane == src) {
                    if (dl < 0) err = GPUDIFF_TOK_STRING;
                    else v = ((uint64_t)(uint32_t)dl << 32) | (uint64_t)(sop + 1) | 0x80000000ull;
                }
            }
            if (sm) wave_sync();  // the decoded bytes, read by other lanes below
            if (i < nn) M.val[i] = v;
            // the window's strings, flattened (uniform: every lane takes part)
            const uint32_t vl = (uint32_t)(v >> 32);
            const uint32_t xv = wave_esc_extra(is_str && err == GPUDIFF_TOK_OK, sptr(T, v), vl);
            const uint32_t xk = wave_esc_extra(has_key, kp, kl);
            if (i < nn) {
                if (is_str) {
                    vsz = 2 + vl + xv;
                    if (xv == 0) fl0 |= MF_VCLEAN;
                }
                if (has_key && xk == 0) fl0 |= MF_KCLEAN;
                M.vsz[i] = vsz;
                M.sz[i] = vsz;
                M.ksz[i] = has_key ? 3 + kl + xk : 0u;
                M.fl[i] = fl0;
            }
        }
        const uint32_t e = wave_max_v(err);
        if (e) status = e;
        any_float = ballot(any_float_lane) != 0;
    }
    wave_sync();
    return any_float;
}

// floats (Go's shortest text, Ryu) in a pass of their own: it keeps the
// 64-bit digit arithmetic out of the register budget of the other phases
__device__ __forceinline__ void marshal_m1_floats(const DocTree& T, const MarshalScratch& M) {
    const uint32_t lane = T.lane, nn = T.nn;
    for (uint32_t i0 = 0; i0 < nn; i0 += 64) {
        const uint32_t i = i0 + lane;
        if (i < nn && (M.fl[i] & MF_FLOAT)) {
            const uint64_t fv = M.val[i];
            const uint32_t fs = go_float_put(fv, false, nullptr);
            M.vsz[i] = fs;
            M.sz[i] = fs;
        }
    }
    wave_sync();
}

// ---------------------------------------------------------- M2-M4 transform marks, child lists, owner references
// mmode: GPUDIFF_UPSERT_* (owner references are normalized in spec mode only)
// Returns whether the root has a "metadata" member that is no object (the Update body then takes no splice).
// name_node / ns_node: metadata's "name" / "namespace" member when its value is a string, else NONE (M8c).
__device__ __forceinline__ bool marshal_m2_m4_children(const DocTree& T, const MarshalScratch& M, uint32_t mmode,
                                                       uint32_t& status, uint32_t& name_node, uint32_t& ns_node) {
    const uint8_t* const d = T.d;
    const uint32_t lane = T.lane, nn = T.nn, meta_node = T.meta_node, labels_node = T.labels_node;
    const bool labels_ok = T.labels_ok;
    const Scratch& S = T.S;
    // ---------------------------------------------------------- M2 transform marks, child counts
    uint32_t orf = NONE, owned = NONE;
    bool meta_other = false;
    name_node = NONE;
    ns_node = NONE;
    if (status == GPUDIFF_TOK_OK) {
        uint32_t my_orf = NONE, my_owned = NONE, my_name = NONE, my_ns = NONE;
        bool my_meta_other = false;
        for (uint32_t i0 = 1; i0 < nn; i0 += 64) {
            const uint32_t i = i0 + lane;
            if (i >= nn) break;
            const uint4 r = S.rec[i];
            atomicAdd(&M.nch[r.x], 1u);
            if (r.x == meta_node && meta_node != NONE) {
                const KeyWin K = key_win(T, r.y);
                if (field_fold(K, "uid", 3) == 1u || field_fold(K, "resourceVersion", 15) == 1u) {
                    M.fl[i] = MF_HIDDEN;
                } else {
                    if (mmode == GPUDIFF_UPSERT_SPEC && field_fold(K, "ownerReferences", 15) == 1u) my_orf = i;
                    if (key_win_cmp(K, "resourceVersion", 15) < 0) M.fl[i] |= MF_RVPRE;  // for M9's splice point
                    if (r.w & NI_STR) {  // NestedString: a string value, the key byte for byte
                        if (field_fold(K, "name", 4) == 1u) my_name = i;
                        else if (field_fold(K, "namespace", 9) == 1u) my_ns = i;
                    }
                }
            } else if (meta_node == NONE && r.x == 0u) {
                // no metadata object: the splice wraps the member into a "metadata" member of the root -- unless
                // the root has that key with another kind of value (SetNestedField fails, nothing is set)
                const int c = key_win_cmp(key_win(T, r.y), "metadata", 8);
                if (c < 0) M.fl[i] |= MF_RVPRE;
                my_meta_other |= c == 0;
            }
            if (r.x == labels_node && labels_node != NONE && labels_ok && (r.w & NI_STR)) {
                if (field_fold(key_win(T, r.y), "kcp.dev/owned-by", 16) == 1u) my_owned = i;
            }
        }
        // duplicate keys are resolved (deferred) by M5 before anything is emitted
        orf = wave_min_v(my_orf);
        owned = wave_min_v(my_owned);
        name_node = wave_min_v(my_name);
        ns_node = wave_min_v(my_ns);
        if (meta_node == NONE) meta_other = ballot(my_meta_other) != 0;
    }
    wave_sync();

    // ---------------------------------------------------------- M3 child lists
    if (status == GPUDIFF_TOK_OK) {
        uint32_t run = 0, wide = 0;
        for (uint32_t i0 = 0; i0 < nn; i0 += 64) {
            const uint32_t i = i0 + lane;
            const uint32_t c = i < nn ? M.nch[i] : 0u;
            if (c > kMarshalMaxMembers && i < nn && is_obj(T, i)) wide = 1;
            const uint32_t inc = wave_incl_scan(c);
            if (i < nn) M.base[i] = run + inc - c;
            run += rdlane(inc, 63);
        }
        if (ballot(wide)) status = GPUDIFF_TOK_WIDE;
        wave_sync();
        if (status == GPUDIFF_TOK_OK) {
            for (uint32_t i0 = 1; i0 < nn; i0 += 64) {
                const uint32_t i = i0 + lane;
                if (i >= nn) break;
                const uint32_t p = S.rec[i].x;
                const uint32_t slot = atomicAdd(&M.rank[p], 1u);  // M.rank: a cursor until M5
                M.kids[M.base[p] + slot] = i;
            }
        }
    }
    wave_sync();

    // ---------------------------------------------------------- M4 owner references (spec mode)
    if (status == GPUDIFF_TOK_OK && orf != NONE) {
        const uint4 ro = S.rec[orf];
        bool drop = (ro.w & NI_LEAF) || (S.tok[ro.z] >> 24) != '[';  // [] or not a list: removed
        uint32_t kept = 0;
        if (!drop) {
            // the owned-by label value ("" when absent / labels not a string map)
            const uint8_t* own_p = d;
            uint32_t own_l = 0;
            if (owned != NONE) {
                const uint64_t ov = M.val[owned];
                own_p = sptr(T, ov);
                own_l = (uint32_t)(ov >> 32);
            }
            const uint32_t ne = M.nch[orf], eb = M.base[orf];
            bool bad = false;
            for (uint32_t j0 = 0; j0 < ne; j0 += 64) {
                const uint32_t j = j0 + lane;
                if (j >= ne) break;
                const uint32_t e = M.kids[eb + j];
                const uint4 re = S.rec[e];
                const bool eobj = (re.w & NI_LEAF) ? ((re.w & NI_TAG) == GPUDIFF_TAG_EOBJ) : (S.tok[re.z] >> 24) == '{';
                if (!eobj) {
                    bad = true;
                    continue;
                }
                // extractOwnerReference: the four strings ("" unless a string) and two bools (set only if bool)
                uint32_t role[6] = {NONE, NONE, NONE, NONE, NONE, NONE};  // apiVersion bOD controller kind name uid
                if (!(re.w & NI_LEAF)) {
                    const uint32_t nk = M.nch[e], kb = M.base[e];
                    for (uint32_t q = 0; q < nk; q++) {
                        const uint32_t c = M.kids[kb + q];
                        const uint4 rc = S.rec[c];
                        const KeyWin K = key_win(T, rc.y);
                        const bool s = (rc.w & NI_STR) != 0;
                        const uint32_t c0 = d[S.tok[rc.z] & POS_MASK];
                        const bool b = (rc.w & NI_ATOM) && (c0 == 't' || c0 == 'f');
                        if (s && field_fold(K, "apiVersion", 10) == 1u) role[0] = c;
                        else if (b && field_fold(K, "blockOwnerDeletion", 18) == 1u) role[1] = c;
                        else if (b && field_fold(K, "controller", 10) == 1u) role[2] = c;
                        else if (s && field_fold(K, "kind", 4) == 1u) role[3] = c;
                        else if (s && field_fold(K, "name", 4) == 1u) role[4] = c;
                        else if (s && field_fold(K, "uid", 3) == 1u) role[5] = c;
                    }
                }
                const uint8_t* np = d;
                uint32_t nl = 0;
                if (role[4] != NONE) {
                    const uint64_t nv = M.val[role[4]];
                    np = sptr(T, nv);
                    nl = (uint32_t)(nv >> 32);
                }
                uint32_t f = MF_CUSTOM;
                if (bytes_eq(np, nl, own_p, own_l)) {
                    f |= MF_HIDDEN;  // reference.Name == ownedByLabel: skipped (specsyncer.go:102-104)
                } else {
                    kept++;
                    auto sv = [&](uint32_t c) -> uint32_t { return c == NONE ? 2u : M.vsz[c]; };
                    uint32_t size = 2 + 13 + sv(role[0]) + 1 + 7 + sv(role[3]) + 1 + 7 + sv(role[4]) + 1 + 6 + sv(role[5]);
                    if (role[1] != NONE) size += 1 + 21 + M.vsz[role[1]];
                    if (role[2] != NONE) size += 1 + 13 + M.vsz[role[2]];
                    M.sz[e] = size;
                    // M9 re-finds the string roles; the two optional bools ride in the element's value word
                    M.val[e] = ((uint64_t)role[1] << 32) | role[2];  // the two optional bools
                }
                M.fl[e] = f;
            }
            if (ballot(bad)) drop = true;
            kept = wave_sum_v(kept);
            if (!kept) drop = true;
        }
        if (drop && lane == 0) M.fl[orf] = MF_HIDDEN;
    }
    wave_sync();
    return meta_other;
}

// ---------------------------------------------------------- M5 sibling ranks
// A member's rank among its siblings in key byte order. Each key's first 8 bytes, big-endian and
// zero padded, are laid out first (M.pre / M.vst are free until M7 / M8): keys reaching K10 hold no
// escapes (the tree defers those) hence no 0 byte, so the prefixes order the keys exactly unless
// two are equal, and only such ties compare the key bytes.
__device__ __forceinline__ void marshal_m5_ranks(const DocTree& T, const MarshalScratch& M, uint32_t& status) {
    const uint32_t lane = T.lane, nn = T.nn;
    const Scratch& S = T.S;
    if (status == GPUDIFF_TOK_OK) {
        bool dup = false;
        for (uint32_t i0 = 1; i0 < nn; i0 += 64) {
            const uint32_t i = i0 + lane;
            if (i >= nn) break;
            const uint32_t y = S.rec[i].y;
            uint64_t pre = 0;
            uint32_t kl = 0;
            if (y & KEYBIT) {
                const uint8_t* kp;
                kl = key_of(T, y, &kp);
                if (kl) {
                    const uint64_t w = ld8u(kp);
                    pre = __builtin_bswap64(kl >= 8u ? w : (w & ((1ull << (8u * kl)) - 1ull)));
                }
            }
            M.pre[i] = (uint32_t)(pre >> 32);
            M.vst[i] = (uint32_t)pre;
            M.order[i] = kl;  // the key length, for ties
        }
        wave_sync();
        for (uint32_t i0 = 1; i0 < nn; i0 += 64) {
            const uint32_t i = i0 + lane;
            if (i >= nn) break;
            const uint4 r = S.rec[i];
            uint32_t rank = r.y;
            if (r.y & KEYBIT) {
                const uint64_t pre = ((uint64_t)M.pre[i] << 32) | M.vst[i];
                const uint32_t kl = M.order[i];
                const uint32_t nk = M.nch[r.x], kb = M.base[r.x];
                rank = 0;
                // siblings four at a time: their ids, then their prefixes, issued together (one sibling a
                // turn waited for two dependent loads per sibling)
                for (uint32_t q0 = 0; q0 < nk; q0 += 4) {
                uint32_t sv[4];
                uint64_t pv[4];
#pragma unroll
                for (uint32_t u = 0; u < 4; u++) sv[u] = q0 + u < nk ? M.kids[kb + q0 + u] : i;
#pragma unroll
                for (uint32_t u = 0; u < 4; u++) pv[u] = ((uint64_t)M.pre[sv[u]] << 32) | M.vst[sv[u]];
#pragma unroll
                for (uint32_t u = 0; u < 4; u++) {
                    const uint32_t s = sv[u];
                    if (s == i) continue;  // itself, or past the list's end
                    const uint64_t sp = pv[u];
                    if (sp < pre) {
                        rank++;
                    } else if (sp == pre) {
                        const uint32_t sl = M.order[s];
                        if (kl <= 8u && sl <= 8u) {
                            if (sl < kl) rank++;
                            else if (sl == kl) dup = true;
                        } else {
                            const uint8_t *kp, *sq;
                            key_of(T, r.y, &kp);
                            key_of(T, S.rec[s].y, &sq);
                            const int c = bytes_cmp(sq, sl, kp, kl);
                            if (c < 0) rank++;
                            else if (c == 0) dup = true;
                        }
                    }
                }
                }
            }
            M.rank[i] = rank;  // (M3's cursors are no longer read; M.order holds key lengths other lanes read)
        }
        if (ballot(dup)) status = GPUDIFF_TOK_HASH;
    }
    wave_sync();
}

// ---------------------------------------------------------- M6-M8 the layout of the text
// lds: the wave's LDS area (the depth sort's histogram and cursors); ocap: the room at the body's place.
// Returns the body's size without its newline.
__device__ __forceinline__ uint32_t marshal_m6_m8_layout(const DocTree& T, const MarshalScratch& M, uint8_t* lds,
                                                         uint64_t ocap, uint32_t& status) {
    const uint32_t lane = T.lane, nn = T.nn, max_depth = T.max_depth;
    const Scratch& S = T.S;
    uint32_t* const hist = (uint32_t*)(lds + kLdsHist.off);
    uint32_t* const cur = (uint32_t*)(lds + kLdsCursor.off);
    // ---------------------------------------------------------- depth order (counting sort)
    if (status == GPUDIFF_TOK_OK && nn > 1) {
        for (uint32_t i = lane; i <= kMaxDepth; i += 64) hist[i] = 0;
        wave_sync();
        for (uint32_t i0 = 1; i0 < nn; i0 += 64) {
            const uint32_t i = i0 + lane;
            if (i < nn) atomicAdd(&hist[(S.rec[i].w >> NI_DEPTH_SHIFT) & 0xFFu], 1u);
        }
        wave_sync();
        uint32_t run = 0;
        for (uint32_t d0 = 0; d0 <= kMaxDepth; d0 += 64) {
            const uint32_t dd = d0 + lane;
            const uint32_t cnt = dd <= kMaxDepth ? hist[dd] : 0u;
            const uint32_t inc = wave_incl_scan(cnt);
            if (dd <= kMaxDepth) cur[dd] = run + inc - cnt;
            run += rdlane(inc, 63);
        }
        wave_sync();
        for (uint32_t i0 = 1; i0 < nn; i0 += 64) {
            const uint32_t i = i0 + lane;
            if (i < nn) {
                const uint32_t dep = (S.rec[i].w >> NI_DEPTH_SHIFT) & 0xFFu;
                M.order[atomicAdd(&cur[dep], 1u)] = i;
            }
        }
        wave_sync();
        // cur[dep] now = end of depth dep's range; hist[dep] = its count
    }

    // ---------------------------------------------------------- M6 subtree sizes, bottom-up
    if (status == GPUDIFF_TOK_OK && nn > 1) {
        for (uint32_t dep = max_depth; dep >= 1; dep--) {
            const uint32_t cnt = hist[dep], end = cur[dep], beg = end - cnt;
            for (uint32_t j0 = beg; j0 < end; j0 += 64) {
                const uint32_t j = j0 + lane;
                if (j >= end) break;
                const uint32_t c = M.order[j];
                const uint4 r = S.rec[c];
                uint32_t fl = M.fl[c];
                uint32_t sz = M.sz[c];
                if (!(r.w & NI_LEAF) && !(fl & MF_CUSTOM) && (fl & MF_HASVIS)) {
                    sz -= 1;  // n members carry n - 1 commas
                    M.sz[c] = sz;
                }
                if (!(fl & MF_HIDDEN) && !(M.fl[r.x] & MF_CUSTOM)) {
                    atomicAdd(&M.sz[r.x], 1u + M.ksz[c] + sz);
                    atomicOr(&M.fl[r.x], MF_HASVIS);
                }
            }
            wave_sync();
        }
    }
    uint32_t sz0 = 2;
    if (status == GPUDIFF_TOK_OK) {
        sz0 = M.sz[0] - ((M.fl[0] & MF_HASVIS) ? 1u : 0u);
        if ((uint64_t)sz0 + 1u > ocap) status = GPUDIFF_TOK_SPACE;
    }

    // ---------------------------------------------------------- M7 sibling prefix sums
    if (status == GPUDIFF_TOK_OK && nn > 1) {
        for (uint32_t i0 = 1; i0 < nn; i0 += 64) {
            const uint32_t i = i0 + lane;
            if (i >= nn) break;
            const uint4 r = S.rec[i];
            const uint32_t item = (M.fl[i] & MF_HIDDEN) ? 0u : 1u + M.ksz[i] + M.sz[i];
            M.pre[M.base[r.x] + M.rank[i]] = item;
        }
        wave_sync();
        const uint32_t ns = nn - 1;  // child slots
        uint32_t run = 0;
        for (uint32_t j0 = 0; j0 < ns; j0 += 64) {
            const uint32_t j = j0 + lane;
            const uint32_t v = j < ns ? M.pre[j] : 0u;
            const uint32_t inc = wave_incl_scan(v);
            if (j < ns) M.pre[j] = run + inc - v;
            run += rdlane(inc, 63);
        }
        wave_sync();
    }

    // ---------------------------------------------------------- M8 value offsets, top-down
    if (status == GPUDIFF_TOK_OK) {
        if (lane == 0) {
            M.vst[0] = 0;
            M.fl[0] |= MF_VIS;
        }
        wave_sync();
        uint32_t beg = 0;
        for (uint32_t dep = 1; dep <= max_depth && nn > 1; dep++) {
            const uint32_t cnt = hist[dep];
            for (uint32_t j0 = 0; j0 < cnt; j0 += 64) {
                if (j0 + lane >= cnt) break;
                const uint32_t c = M.order[beg + j0 + lane];
                const uint4 r = S.rec[c];
                const uint32_t fp = M.fl[r.x];
                const uint32_t fc = M.fl[c];
                if ((fp & MF_VIS) && !(fp & MF_CUSTOM) && !(fc & MF_HIDDEN)) {
                    const uint32_t b = M.base[r.x];
                    const uint32_t e = M.pre[b + M.rank[c]] - M.pre[b];
                    M.vst[c] = M.vst[r.x] + 1u + e + M.ksz[c];
                    M.fl[c] = fc | MF_VIS;
                }
            }
            beg += cnt;
            wave_sync();
        }
    }
    return sz0;
}

// ---------------------------------------------------------- M8b the resourceVersion splice point
// Where `"resourceVersion":"<rv>"` goes in the body M9 writes (include/gpudiff.h GPUDIFF_RV_*): the Update body is
// then two copies around that member, with no second marshal.  The member belongs in metadata (an object:
// T.meta_node, `{}` included), or -- when the root has no "metadata" key -- inside a new `"metadata":{...}` member
// of the root; a metadata that is present and not an object takes no splice (meta_other, from M2).
//
// Either way the place is the end of the last visible member of the container whose key sorts before the literal,
// else just past the container's `{`.  M2 marked those members (MF_RVPRE: it holds their keys in registers anyway,
// KeyWin, and compares the first 16 bytes as two big-endian words); M9, which visits every visible node with its
// value's start in hand, keeps the largest end among the marked ones (rv_end: the layout grows with the rank, so
// the last one is the maximum).  Hidden members (uid, resourceVersion, removed owner references) are never
// visited, so they do not count.  What is left here is a wave maximum and two words of the container.
__device__ __forceinline__ void marshal_m8b_rv_splice(const DocTree& T, const MarshalScratch& M, bool meta_other,
                                                      uint32_t rv_end, uint32_t& off, uint32_t& form) {
    const bool wrap = T.meta_node == NONE;
    const uint32_t cont = wrap ? 0u : T.meta_node;  // the container the member text goes into
    const uint32_t open = M.vst[cont], cfl = M.fl[cont];
    const uint32_t end = wave_max_v(rv_end);
    off = 0;
    form = GPUDIFF_RV_NONE;
    if (meta_other) return;
    form = GPUDIFF_RV_INSERT | (wrap ? GPUDIFF_RV_WRAP : 0u);
    if (end) {
        off = end;
        form |= GPUDIFF_RV_LEAD;
    } else {
        off = open + 1u;
        if (cfl & MF_HASVIS) form |= GPUDIFF_RV_TRAIL;
    }
}

// ---------------------------------------------------------- M8c the request target
// Where the values of metadata.name and metadata.namespace stand in the body (include/gpudiff.h GPUDIFF_TGT_*): M2
// found the two members among metadata's (the key window it compares anyway; a duplicate key defers the document in
// M5), M1 knows whether each string renders as its own bytes, M8 placed the value.  A string's text is its quotes
// around the rendered bytes, so the span is [vst + 1, vst + sz - 1).  Three words of each node, read once.
static_assert(GPUDIFF_TGT_NS == GPUDIFF_TGT_NAME << 2 && GPUDIFF_TGT_NS_ESC == GPUDIFF_TGT_NAME_ESC << 2,
              "the namespace's flags are the name's, two bits up");
__device__ __forceinline__ void marshal_m8c_targets(const MarshalScratch& M, uint32_t name_node, uint32_t ns_node,
                                                    TokOut& o) {
    uint32_t off[2] = {0, 0}, len[2] = {0, 0}, flags = 0;
    const uint32_t node[2] = {name_node, ns_node};
#pragma unroll
    for (uint32_t k = 0; k < 2; k++) {
        if (node[k] == NONE) continue;
        off[k] = M.vst[node[k]] + 1u;
        len[k] = M.sz[node[k]] - 2u;
        flags |= (GPUDIFF_TGT_NAME | ((M.fl[node[k]] & MF_VCLEAN) ? 0u : GPUDIFF_TGT_NAME_ESC)) << (2u * k);
    }
    tokout_set_targets(o, off[0], len[0], off[1], len[1], flags);
}

// ---------------------------------------------------------- M9 emit
// dst: the body's place; sz0, any_float: from M6-M8 and M1.  Returns this lane's part of M8b: the largest end of a
// visible MF_RVPRE member's value it wrote (0: none).
__device__ __forceinline__ uint32_t marshal_m9_emit(const DocTree& T, const MarshalScratch& M, uint8_t* dst,
                                                    uint32_t sz0, bool any_float) {
    const uint8_t* const d = T.d;
    const uint32_t lane = T.lane, nn = T.nn;
    const Scratch& S = T.S;
    uint32_t rv_end = 0;
    if (lane == 0) {
        dst[0] = '{';
        dst[sz0 - 1] = '}';
        dst[sz0] = '\n';
    }
    for (uint32_t i0 = 1; i0 < nn; i0 += 64) {
        const uint32_t i = i0 + lane;
        const uint32_t fl = i < nn ? M.fl[i] : 0u;
        bool long_str = false;
        uint32_t lvs = 0;
        // clean keys / string values are copied by the flattened passes after this block
        bool ck = false, cv = false;
        const uint8_t* ckp = d;
        uint32_t ckl = 0, ckd = 0, cvd = 0;
        uint64_t cvv = 0;
        if (fl & MF_VIS) {
        const uint4 r = S.rec[i];
        const uint32_t vs = M.vst[i], ksz = M.ksz[i];
        const uint32_t kpos = vs - ksz;
        if (kpos != M.vst[r.x] + 1u) dst[kpos - 1] = ',';
        if (fl & MF_RVPRE) rv_end = max(rv_end, vs + M.sz[i]);
        if (ksz) {
            const uint8_t* kp;
            const uint32_t kl = key_of(T, r.y, &kp);
            uint8_t* q = dst + kpos;
            q[0] = '"';
            q[ksz - 2] = '"';
            q[ksz - 1] = ':';
            if (fl & MF_KCLEAN) {
                ck = true;
                ckp = kp;
                ckl = kl;
                ckd = kpos + 1;
            } else {
                go_esc_put(q + 1, kp, kl);
            }
        }
        uint8_t* q = dst + vs;
        if (fl & MF_CUSTOM) {
            // normalized OwnerReference, keys in Go's sorted order
            uint32_t role[6] = {NONE, (uint32_t)(M.val[i] >> 32), (uint32_t)M.val[i], NONE, NONE, NONE};
            if (!(r.w & NI_LEAF)) {
                const uint32_t nk = M.nch[i], kb = M.base[i];
                for (uint32_t qq = 0; qq < nk; qq++) {
                    const uint32_t c = M.kids[kb + qq];
                    const uint4 rc = S.rec[c];
                    if (!(rc.w & NI_STR)) continue;
                    const KeyWin K = key_win(T, rc.y);
                    if (field_fold(K, "apiVersion", 10) == 1u) role[0] = c;
                    else if (field_fold(K, "kind", 4) == 1u) role[3] = c;
                    else if (field_fold(K, "name", 4) == 1u) role[4] = c;
                    else if (field_fold(K, "uid", 3) == 1u) role[5] = c;
                }
            }
            auto put_lit = [&](const char* s, uint32_t n) {
                for (uint32_t k = 0; k < n; k++) *q++ = (uint8_t)s[k];
            };
            auto put_sv = [&](uint32_t c) {
                *q++ = '"';
                if (c != NONE) {
                    const uint64_t v = M.val[c];
                    q = go_esc_put(q, sptr(T, v), (uint32_t)(v >> 32));
                }
                *q++ = '"';
            };
            auto put_bool = [&](uint32_t c) {
                if (d[S.tok[S.rec[c].z] & POS_MASK] == 't') put_lit("true", 4);
                else put_lit("false", 5);
            };
            put_lit("{\"apiVersion\":", 14);
            put_sv(role[0]);
            if (role[1] != NONE) {
                put_lit(",\"blockOwnerDeletion\":", 22);
                put_bool(role[1]);
            }
            if (role[2] != NONE) {
                put_lit(",\"controller\":", 14);
                put_bool(role[2]);
            }
            put_lit(",\"kind\":", 8);
            put_sv(role[3]);
            put_lit(",\"name\":", 8);
            put_sv(role[4]);
            put_lit(",\"uid\":", 7);
            put_sv(role[5]);
            *q = '}';
        } else if (!(r.w & NI_LEAF)) {
            const bool ob = (S.tok[r.z] >> 24) == '{';
            q[0] = ob ? '{' : '[';
            q[M.sz[i] - 1] = ob ? '}' : ']';
        } else if (r.w & NI_STR) {
            const uint64_t v = M.val[i];
            const uint32_t sl = (uint32_t)(v >> 32);
            q[0] = '"';
            q[M.sz[i] - 1] = '"';
            if (fl & MF_VCLEAN) {
                cv = true;
                cvv = v;
                cvd = vs + 1;
            } else if (sl > kLongString) {
                long_str = true;
                lvs = vs + 1;
            } else {
                go_esc_put(q + 1, sptr(T, v), sl);
            }
        } else if (r.w & NI_ATOM) {
            const uint32_t c0 = d[S.tok[r.z] & POS_MASK];
            if (c0 == 't') { q[0] = 't'; q[1] = 'r'; q[2] = 'u'; q[3] = 'e'; }
            else if (c0 == 'f') { q[0] = 'f'; q[1] = 'a'; q[2] = 'l'; q[3] = 's'; q[4] = 'e'; }
            else if (c0 == 'n') { q[0] = 'n'; q[1] = 'u'; q[2] = 'l'; q[3] = 'l'; }
            else if (!(fl & MF_FLOAT)) i64_put(q, (int64_t)M.val[i], M.vsz[i]);  // floats: below
        } else {
            const bool ob = (r.w & NI_TAG) == GPUDIFF_TAG_EOBJ;
            q[0] = ob ? '{' : '[';
            q[1] = ob ? '}' : ']';
        }
        }
        wave_copy_flat(ck, ckp, ckl, dst + ckd);
        wave_copy_flat(cv, sptr(T, cvv), (uint32_t)(cvv >> 32), dst + cvd);
        for (uint64_t bl = ballot(long_str); bl; bl &= bl - 1) {  // long strings that need escaping
            const uint32_t src = (uint32_t)__builtin_ctzll(bl);
            const uint64_t sv = rdlane64(M.val[i < nn ? i : 0], src);
            wave_esc_put(dst + rdlane(lvs, src), sptr(T, sv), (uint32_t)(sv >> 32));
        }
    }
    if (any_float) {
        for (uint32_t i0 = 1; i0 < nn; i0 += 64) {
            const uint32_t i = i0 + lane;
            if (i < nn && (M.fl[i] & (MF_FLOAT | MF_VIS)) == (MF_FLOAT | MF_VIS)) {
                const uint64_t fv = M.val[i];
                go_float_put(fv, false, dst + M.vst[i]);
            }
        }
    }
    return rv_end;
}

// T: the document's tree; work: the document's working area (marshal_layout); mmode: GPUDIFF_UPSERT_*; bodies +
// obase: the body's place; out: the document's result; lds: the wave's LDS area
__device__ __forceinline__ void marshal_doc(const DocTree& T, uint8_t* work, uint32_t mmode, uint8_t* bodies,
                                            uint64_t obase, TokOut* out, uint8_t* lds, PhaseClock& mark) {
    mark(PS_TREE);  // the tree (phase 2) ends here in marshal mode
    const MarshalScratch M = bind_marshal_scratch(work, T.len);
    uint32_t status = T.status;
    TokOut o{};
    o.off = obase;
    const bool any_float = marshal_m1_sizes(T, M, status);
    mark(PM_M1);
    if (status == GPUDIFF_TOK_OK && any_float) marshal_m1_floats(T, M);
    mark(PM_M1_FLOATS);
    uint32_t name_node, ns_node;
    const bool meta_other = marshal_m2_m4_children(T, M, mmode, status, name_node, ns_node);
    mark(PM_M2_M4);
    marshal_m5_ranks(T, M, status);
    mark(PM_M5);
    const uint32_t sz0 = marshal_m6_m8_layout(T, M, lds, marshal_out_cap(T.len), status);
    mark(PM_M6_M8);
    if (status == GPUDIFF_TOK_OK) {
        const uint32_t rv_end = marshal_m9_emit(T, M, bodies + obase, sz0, any_float);
        o.bytes = sz0 + 1u;
        uint32_t rv_off, rv_form;
        marshal_m8b_rv_splice(T, M, meta_other, rv_end, rv_off, rv_form);
        tokout_set_rv_splice(o, rv_off, rv_form);
        marshal_m8c_targets(M, name_node, ns_node, o);
    }
    o.n_nodes = T.nn;
    o.status = status;
    if (T.lane == 0) *out = o;
    mark(PM_M9);
}

}  // namespace

}  // namespace gd
