// K11 -- the Deployment splitter's status roll-up fields:
// what k_encode_docs<MINW, kModeRollup> runs after phases 1-2 (structural scan,
// tree).
//
// pkg/reconciler/deployment/deployment.go:41-91 reads, per cached Deployment,
// the kcp.dev/owned-by label (the selector at :44-51) and the five int32
// counters of .status (:79-85).  The objects are typed appsv1.Deployments
// decoded by encoding/json, so the device takes a document only where that
// decode is certain:
//   R0 the rest of Go's scanner: every literal / number and every escaped
//      string valid (phases 1-2 check the structure)
//   R1 root members: "metadata" / "status" matched exactly, at most once each;
//      a key equal to either under ASCII case folding (Go's field lookup) but
//      not exactly -> host
//   R2 "labels" under metadata, the five counters under status: same rules;
//      a counter must be null (a no-op) or an integer literal in int32 range
//   R3 the owned-by member of labels (map key: exact), a string without
//      escapes; every label value must be a string
// Anything else (a duplicate, a fold-only match, a type mismatch the host must
// judge as a Go decode error, a float or out-of-range counter) keeps
// GPUDIFF_TOK_FIELD and the host path (rollup.cpp) decides the document.
//
// R0-R3 are one sweep over the nodes, a lane per node: each chunk of 64 loads its records, their tokens, then the
// value's and the key's bytes into registers (one dependent chain a chunk), and every rule is decided from those.
// Nodes are in pre-order, so a parent precedes its members: within a chunk the root members are found first
// (metadata / status ids by ballot), then the members of those (labels), then the members of labels.  (Separate
// passes paid the record -> token -> bytes chain once per pass and per looked-up node kind.)  The first R0 error a
// lane meets stays its code; any R1-R3 failure is GPUDIFF_TOK_FIELD, applied in that order.
#pragma once
#include "tokdev.h"

namespace gd {

namespace {

// T: the document's tree; out: the document's result
__device__ __forceinline__ void rollup_doc(const DocTree& T, RollOut* out, PhaseClock& mark) {
    const uint8_t* const d = T.d;
    const uint32_t len = T.len, lane = T.lane, nn = T.nn;
    const Scratch& S = T.S;
    uint32_t status = T.status;
    mark(PS_TREE);
    RollOut R{};
    if (status == GPUDIFF_TOK_OK) {
        uint32_t err0 = 0;     // R0, per lane
        bool bad = false;      // R1-R3, per lane
        uint32_t meta_id = NONE, stat_id = NONE, lab_id = NONE, mk = 0, sk = 0, lk = 0;
        uint32_t n_meta = 0, n_stat = 0, n_lab = 0, n_own = 0;
        uint32_t n_f[5] = {0, 0, 0, 0, 0};
        const uint8_t* const lim = d + len + kTokSlack;
        for (uint32_t i0 = 1; i0 < nn; i0 += 64) {
            const uint32_t i = i0 + lane;
            const bool live = i < nn;
            const uint4 r = S.rec[live ? i : 0u];
            const bool leaf = live && (r.w & NI_LEAF), atom = leaf && (r.w & NI_ATOM), str = leaf && (r.w & NI_STR);
            const bool keyed = live && (r.y & KEYBIT);
            // the value's tokens and the key's, then the bytes at both (every lane loads: selects, not branches)
            const uint32_t tz = live ? r.z : 0u, kt = keyed ? r.y & ~KEYBIT : 0u;
            const uint32_t t0 = S.tok[tz], t1 = S.tok[tz + 1u], k0 = S.tok[kt], k1 = S.tok[kt + 1u];
            const uint32_t vop = t0 & POS_MASK, kop = k0 & POS_MASK;
            uint64_t w0, w1;
            ld16u(d + vop, &w0, &w1);
            KeyWin K = key_window(d + kop + 1u, (k1 & POS_MASK) - kop - 1u, lim);
            if (!keyed) K.kl = NONE;  // matches no name
            // R0: the atom (from the window; memory for what it does not decide)
            uint32_t t = GPUDIFF_TAG_NULL, e = GPUDIFF_TOK_OK;
            uint64_t v = 0;
            if (atom) {
                if (parse_atom_fast(w0, w1, (uint64_t)(len - vop), &t, &v) != 0u) e = parse_atom_mem(d + vop, d + len, &t, &v);
                if (e) err0 = e;
            }
            // obj_kind: 0 null, 1 empty object, 2 object with members, 3 anything else
            const uint32_t kind = !leaf ? ((t0 >> 24) == '{' ? 2u : 3u)
                                  : atom ? ((e == GPUDIFF_TOK_OK && t == GPUDIFF_TAG_NULL) ? 0u : 3u)
                                         : ((r.w & NI_TAG) == GPUDIFF_TAG_EOBJ ? 1u : 3u);
            // R1: root members
            const bool root = live && r.x == 0u;
            const uint32_t fm = field_fold(K, "metadata", 8), fs = field_fold(K, "status", 6);
            if (root && (fm == 2u || fs == 2u)) bad = true;
            const uint64_t bm = ballot(root && fm == 1u), bs = ballot(root && fs == 1u);
            n_meta += popc64(bm);
            n_stat += popc64(bs);
            if (bm) {
                const uint32_t src = 63u - (uint32_t)__builtin_clzll(bm);
                meta_id = i0 + src;
                mk = rdlane(kind, src);
            }
            if (bs) {
                const uint32_t src = 63u - (uint32_t)__builtin_clzll(bs);
                stat_id = i0 + src;
                sk = rdlane(kind, src);
            }
            // R2: labels under metadata, the counters under status
            const bool in_meta = live && mk == 2u && r.x == meta_id, in_stat = live && sk == 2u && r.x == stat_id;
            const uint32_t fl = field_fold(K, "labels", 6);
            if (in_meta && fl == 2u) bad = true;
            uint32_t f = NONE;
#pragma unroll
            for (uint32_t k = 0; k < 5; k++) {
                const uint32_t ff = field_fold(K, roll_field(k), roll_field_len(k));
                if (in_stat && ff == 2u) bad = true;
                if (in_stat && ff == 1u) f = k;
            }
            if (f != NONE && (!atom || e != GPUDIFF_TOK_OK ||
                              !(t == GPUDIFF_TAG_NULL ||
                                (t == GPUDIFF_TAG_INT && (int64_t)v >= INT32_MIN && (int64_t)v <= INT32_MAX))))
                bad = true;
            const uint64_t bl = ballot(in_meta && fl == 1u);
            n_lab += popc64(bl);
            if (bl) {
                const uint32_t src = 63u - (uint32_t)__builtin_clzll(bl);
                lab_id = i0 + src;
                lk = rdlane(kind, src);
            }
#pragma unroll
            for (uint32_t k = 0; k < 5; k++) {
                const uint64_t bf = ballot(f == k);
                n_f[k] += popc64(bf);
                if (bf) R.v[k] = (int32_t)rdlane((uint32_t)v, (uint32_t)__builtin_ctzll(bf));  // null: 0, a no-op
            }
            // R3: the members of labels
            const bool in_lab = live && lk == 2u && r.x == lab_id;
            if (in_lab && !str) bad = true;  // map[string]string: a type error
            const bool ho = in_lab && field_fold(K, "kcp.dev/owned-by", 16u) == 1u;  // exact: a map key
            if (ho && (r.w & NI_SLOW)) bad = true;                              // escapes: the host decodes
            const uint64_t bo = ballot(ho);
            n_own += popc64(bo);
            if (bo) {
                const uint32_t src = (uint32_t)__builtin_ctzll(bo);
                R.label_off = rdlane(vop + 1u, src);
                R.label_len = rdlane((t1 & POS_MASK) - vop - 1u, src);
            }
            // R0: escaped strings, one at a time by the whole wave, the error kept by the lane whose node it is
            const bool ss = str && (r.w & NI_SLOW);
            for (uint64_t m = ballot(ss); m; m &= m - 1) {
                const uint32_t src = (uint32_t)__builtin_ctzll(m);
                const uint32_t sop = rdlane(vop, src), scp = rdlane(t1 & POS_MASK, src);
                if (!wave_string_ok(d + sop + 1, scp - sop - 1, d + len, S.str + sop + 1, lane) && lane == src)
                    err0 = GPUDIFF_TOK_STRING;
            }
        }
        err0 = wave_max_v(err0);
        const bool any_bad = ballot(bad) != 0ull;
        bool fail = n_meta > 1 || n_stat > 1 || mk == 3u || sk == 3u || n_lab > 1 || lk == 3u || n_own > 1;
#pragma unroll
        for (uint32_t k = 0; k < 5; k++) fail |= n_f[k] > 1;
        if (err0) status = err0;
        else if (any_bad || fail) status = GPUDIFF_TOK_FIELD;
        else if (n_own == 1) R.flags = kRollHasLabel;
    }
    R.status = status;
    if (lane == 0) *out = R;
    mark(PR_SWEEP);
}

}  // namespace

}  // namespace gd
