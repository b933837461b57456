// K13 -- the API-negotiation update classifier's fields:
// what k_encode_docs<MINW, kModeNegotiate> runs after phases 1-2 (structural
// scan, tree).
//
// pkg/reconciler/apiresource/controller.go:253-283 reads, per typed
// APIResourceImport / NegotiatedAPIResource, metadata.{resourceVersion,
// generation, labels, annotations} and .status ({conditions: [...]}).  The
// device takes a document only where Go 1.16's typed decode is certain:
//   N1 root "metadata" / "status": exact names, at most once, null / object
//   N2 the four metadata fields and status.conditions: same rules;
//      resourceVersion a string without escapes (or null), generation an int64
//      literal (or null), labels / annotations objects (or null), conditions an
//      array (or null)
//   N3 label / annotation entries: string values without escapes, at most
//      kNegMaxMembers, no repeated key; condition elements: objects, at most
//      kNegMaxConds
//   N4 condition fields: exact names at most once each, strings without
//      escapes (or null), lastTransitionTime in neg_parse_time's strict shape
// For a CustomResourceDefinition (tokdoc_neg_kind() == GPUDIFF_NEG_KIND_CRD,
// controller.go:186-199) the status also holds acceptedNames and
// storedVersions:
//   N2 status.acceptedNames (null / object) and storedVersions (null / array)
//      under the same name rules
//   N3 acceptedNames fields (exact, at most once): plural / singular / kind /
//      listKind strings without escapes (or null), shortNames / categories
//      arrays (or null); storedVersions elements: strings without escapes, at
//      most kNegMaxList
//   N3b shortNames / categories elements: the same
// Anything else (fold-only names, repeats that Go merges, null elements, other
// time shapes, type errors Go reports) keeps GPUDIFF_TOK_FIELD and the host
// path (negotiate.cpp) classifies every pair holding the document.
//
// N0-N4 are one sweep over the nodes, a lane per node, as K11's R0-R3: each chunk of 64 loads its records, their
// value and key tokens, then the bytes at both into registers (one dependent chain a chunk), and every rule is
// decided from those.  A parent precedes its members in pre-order, so within a chunk the levels are resolved in
// order -- root members, their fields, map entries / condition elements / CRD name fields, CRD list elements,
// condition fields -- each level's parent ids (and kinds) taken by ballot before the next level looks at the chunk.
// The first N0 error a lane meets stays its code; any N1-N4 failure is GPUDIFF_TOK_FIELD.
#pragma once
#include "tokdev.h"

namespace gd {

namespace {

// T: the document's tree; neg_kind: GPUDIFF_NEG_KIND_* (which typed status to read); O: the document's result; lds:
// the wave's LDS area
__device__ __forceinline__ void negotiate_doc(const DocTree& T, uint32_t neg_kind, NegOut* O, uint8_t* lds,
                                              PhaseClock& mark) {
    const uint8_t* const d = T.d;
    const uint32_t len = T.len, lane = T.lane, nn = T.nn;
    const Scratch& S = T.S;
    uint32_t status = T.status;
    mark(PS_TREE);
    // LDS (the phase 1-2 areas are free now): label / annotation tables, the
    // condition table, condition element node ids, per (condition, field) counts
    NegMember* const t_lab = (NegMember*)(lds + kLdsNegLab.off);
    NegMember* const t_ann = (NegMember*)(lds + kLdsNegAnn.off);
    NegCond* const t_cond = (NegCond*)(lds + kLdsNegCond.off);
    uint32_t* const t_eid = (uint32_t*)(lds + kLdsNegEid.off);
    uint32_t* const t_cnt = (uint32_t*)(lds + kLdsNegCnt.off);
    NegSpan* const t_short = (NegSpan*)(lds + kLdsNegShort.off);  // CRD lists: 3 x kNegMaxList spans
    NegSpan* const t_cat = (NegSpan*)(lds + kLdsNegCat.off);
    NegSpan* const t_stored = (NegSpan*)(lds + kLdsNegStored.off);
    const bool crd = neg_kind == GPUDIFF_NEG_KIND_CRD;
    // LDS tables start empty (N4 fills condition fields as the sweep meets them)
    if (lane < kNegMaxConds) {
        NegCond z{};
        z.sec = kZeroTimeSec;
        t_cond[lane] = z;
    }
    for (uint32_t q = lane; q < kNegMaxConds * 5u; q += 64) t_cnt[q] = 0u;
    wave_sync();
    uint32_t rv_off = 0, rv_len = 0, n_lab = 0, n_ann = 0, n_cond = 0, n_stored = 0, n_short = 0, n_cat = 0;
    int64_t gen = 0;
    NegSpan names[4] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
    if (status == GPUDIFF_TOK_OK) {
        uint32_t err0 = 0;  // N0, per lane
        bool bad = false;   // N1-N4, per lane
        uint32_t meta_id = NONE, stat_id = NONE, mk = 0, sk = 0, n_meta = 0, n_stat = 0;
        // fid[0..3] resourceVersion, generation, labels, annotations; fid[4] conditions; CRD: fid[5] acceptedNames,
        // fid[6] storedVersions -- each with its kind (0 null, 1 {}, 2 object, 3 [], 4 array, 5 string without
        // escapes, 6 anything else)
        uint32_t fid[7] = {NONE, NONE, NONE, NONE, NONE, NONE, NONE}, fk[7] = {0, 0, 0, 0, 0, 0, 0};
        uint32_t n_f[7] = {0, 0, 0, 0, 0, 0, 0};
        bool g_bad = false;
        uint32_t g_tag = GPUDIFF_TAG_NULL;
        uint64_t g_val = 0;
        // CRD acceptedNames: nid[0..5] plural, singular, shortNames, kind, listKind, categories
        uint32_t nid[6] = {NONE, NONE, NONE, NONE, NONE, NONE}, nkd[6] = {0, 0, 0, 0, 0, 0};
        uint32_t n_nf[6] = {0, 0, 0, 0, 0, 0};
        NegSpan nsp[4] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};  // plural, singular, kind, listKind
        const uint8_t* const lim = d + len + kTokSlack;
        const uint64_t below = mask_lt(lane);
        for (uint32_t i0 = 1; i0 < nn; i0 += 64) {
            const uint32_t i = i0 + lane;
            const bool live = i < nn;
            const uint4 r = S.rec[live ? i : 0u];
            const bool leaf = live && (r.w & NI_LEAF), atom = leaf && (r.w & NI_ATOM), str = leaf && (r.w & NI_STR);
            const bool slow = str && (r.w & NI_SLOW), keyed = live && (r.y & KEYBIT);
            // the value's tokens and the key's, then the bytes at both (every lane loads: selects, not branches)
            const uint32_t tz = live ? r.z : 0u, kt = keyed ? r.y & ~KEYBIT : 0u;
            const uint32_t t0 = S.tok[tz], t1 = S.tok[tz + 1u], k0 = S.tok[kt], k1 = S.tok[kt + 1u];
            const uint32_t vop = t0 & POS_MASK, vcp = t1 & POS_MASK, kop = k0 & POS_MASK;
            uint64_t w0, w1;
            ld16u(d + vop, &w0, &w1);
            KeyWin K = key_window(d + kop + 1u, (k1 & POS_MASK) - kop - 1u, lim);
            if (!keyed) K.kl = NONE;  // matches no name
            // N0: the atom (from the window; memory for what it does not decide)
            uint32_t t = GPUDIFF_TAG_NULL, e = GPUDIFF_TOK_OK;
            uint64_t v = 0;
            if (atom) {
                if (parse_atom_fast(w0, w1, (uint64_t)(len - vop), &t, &v) != 0u) e = parse_atom_mem(d + vop, d + len, &t, &v);
                if (e) err0 = e;
            }
            const uint32_t tag = r.w & NI_TAG;
            const uint32_t kind = !leaf ? ((t0 >> 24) == '{' ? 2u : 4u)
                                  : atom ? ((e == GPUDIFF_TOK_OK && t == GPUDIFF_TAG_NULL) ? 0u : 6u)
                                  : str  ? (slow ? 6u : 5u)
                                         : (tag == GPUDIFF_TAG_EOBJ ? 1u : tag == GPUDIFF_TAG_EARR ? 3u : 6u);
            const uint32_t soff = vop + 1u, slen = vcp - vop - 1u;  // a string's span
            // N1: root members
            const bool root = live && r.x == 0u;
            const uint32_t fm = field_fold(K, "metadata", 8), fs = field_fold(K, "status", 6);
            if (root && (fm == 2u || fs == 2u)) bad = true;
            const uint64_t bm = ballot(root && fm == 1u), bs = ballot(root && fs == 1u);
            n_meta += popc64(bm);
            n_stat += popc64(bs);
            if (bm) {
                const uint32_t src = (uint32_t)__builtin_ctzll(bm);
                meta_id = i0 + src;
                mk = rdlane(kind, src);
            }
            if (bs) {
                const uint32_t src = (uint32_t)__builtin_ctzll(bs);
                stat_id = i0 + src;
                sk = rdlane(kind, src);
            }
            // N2: the metadata fields, status.conditions (CRD: acceptedNames, storedVersions)
            const bool in_meta = live && mk == 2u && r.x == meta_id, in_stat = live && sk == 2u && r.x == stat_id;
            uint32_t f = NONE;
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                const uint32_t ff = field_fold(K, neg_meta_field(k), neg_meta_field_len(k));
                if (in_meta && ff == 2u) bad = true;
                if (in_meta && ff == 1u) f = k;
            }
            {
                const uint32_t ff = field_fold(K, "conditions", 10);
                if (in_stat && ff == 2u) bad = true;
                if (in_stat && ff == 1u) f = 4u;
            }
            if (crd) {
                const uint32_t fa = field_fold(K, "acceptedNames", 13), fv = field_fold(K, "storedVersions", 14);
                if (in_stat && (fa == 2u || fv == 2u)) bad = true;
                if (in_stat && fa == 1u) f = 5u;
                if (in_stat && fv == 1u) f = 6u;
            }
            const bool gb = !atom || e != GPUDIFF_TOK_OK || !(t == GPUDIFF_TAG_NULL || t == GPUDIFF_TAG_INT);
#pragma unroll
            for (uint32_t k = 0; k < 7; k++) {
                const uint64_t bf = ballot(f == k);
                n_f[k] += popc64(bf);
                if (bf) {
                    const uint32_t src = (uint32_t)__builtin_ctzll(bf);
                    fid[k] = i0 + src;
                    fk[k] = rdlane(kind, src);
                    if (k == 0u) {
                        rv_off = rdlane(soff, src);
                        rv_len = rdlane(slen, src);
                    }
                    if (k == 1u) {  // generation: an int64 literal or null
                        g_bad = ballot(gb && lane == src) != 0ull;
                        g_tag = rdlane(t, src);
                        g_val = ((uint64_t)rdlane((uint32_t)(v >> 32), src) << 32) | rdlane((uint32_t)v, src);
                    }
                }
            }
            // N3: label / annotation entries, condition elements, CRD name fields, storedVersions elements
            const bool in_lab = live && fk[2] == 2u && r.x == fid[2], in_ann = live && fk[3] == 2u && r.x == fid[3];
            const bool hc = live && fk[4] == 4u && r.x == fid[4], in_names = live && fk[5] == 2u && r.x == fid[5];
            const bool hv = live && fk[6] == 4u && r.x == fid[6];
            if ((in_lab || in_ann || hv) && kind != 5u) bad = true;  // null value / element, escapes, a type error
            if (hc && kind != 1u && kind != 2u) bad = true;
            uint32_t nf = NONE;
#pragma unroll
            for (uint32_t k = 0; k < 6; k++) {
                const uint32_t ff = field_fold(K, neg_crd_names_field(k), neg_crd_names_field_len(k));
                if (in_names && ff == 2u) bad = true;
                if (in_names && ff == 1u) nf = k;
            }
            const uint64_t bl = ballot(in_lab), ba = ballot(in_ann), bc = ballot(hc), bv = ballot(hv);
            if (in_lab | in_ann) {
                const uint32_t p = (in_lab ? n_lab + popc64(bl & below) : n_ann + popc64(ba & below));
                if (p < kNegMaxMembers) (in_lab ? t_lab : t_ann)[p] = NegMember{kop + 1u, K.kl, soff, slen};
            }
            if (hc) {
                const uint32_t p = n_cond + popc64(bc & below);
                if (p < kNegMaxConds) t_eid[p] = i;
            }
            if (hv) {
                const uint32_t p = n_stored + popc64(bv & below);
                if (p < kNegMaxList) t_stored[p] = NegSpan{soff, slen};
            }
            n_lab += popc64(bl);
            n_ann += popc64(ba);
            n_cond += popc64(bc);
            n_stored += popc64(bv);
            if (fk[5] == 2u) {
#pragma unroll
                for (uint32_t k = 0; k < 6; k++) {
                    const uint64_t bf = ballot(nf == k);
                    n_nf[k] += popc64(bf);
                    if (bf) {
                        const uint32_t src = (uint32_t)__builtin_ctzll(bf);
                        nid[k] = i0 + src;
                        nkd[k] = rdlane(kind, src);
                        const uint32_t q = k == 0u ? 0u : k == 1u ? 1u : k == 3u ? 2u : 3u;
                        if (k != 2u && k != 5u) nsp[q] = NegSpan{rdlane(soff, src), rdlane(slen, src)};
                    }
                }
                // N3b: shortNames / categories elements
                const bool hs = live && nkd[2] == 4u && r.x == nid[2], hk = live && nkd[5] == 4u && r.x == nid[5];
                if ((hs || hk) && kind != 5u) bad = true;
                const uint64_t bsn = ballot(hs), bk = ballot(hk);
                if (hs) {
                    const uint32_t p = n_short + popc64(bsn & below);
                    if (p < kNegMaxList) t_short[p] = NegSpan{soff, slen};
                }
                if (hk) {
                    const uint32_t p = n_cat + popc64(bk & below);
                    if (p < kNegMaxList) t_cat[p] = NegSpan{soff, slen};
                }
                n_short += popc64(bsn);
                n_cat += popc64(bk);
            }
            // N4: condition fields (their element's id in t_eid, written above when in this chunk)
            if (n_cond) {
                lds_order();
                const uint32_t nc = min(n_cond, kNegMaxConds);
                uint32_t ci = NONE;
                for (uint32_t c = 0; c < nc; c++)
                    if (t_eid[c] == r.x) ci = c;
                const bool in_cf = live && ci != NONE;
                uint32_t cf = NONE;
#pragma unroll
                for (uint32_t k = 0; k < 5; k++) {
                    const uint32_t ff = field_fold(K, neg_cond_field(k), neg_cond_field_len(k));
                    if (in_cf && ff == 2u) bad = true;
                    if (in_cf && ff == 1u) cf = k;
                }
                if (cf != NONE) {  // (an unknown field: ignored by the typed decode)
                    atomicAdd(&t_cnt[ci * 5u + cf], 1u);
                    if (kind != 0u) {  // null: no-op for a string, the zero Time for lastTransitionTime
                        if (kind != 5u) {
                            bad = true;
                        } else if (cf < 4u) {
                            t_cond[ci].off[cf] = soff;
                            t_cond[ci].len[cf] = slen;
                        } else {
                            int64_t sec;
                            int32_t ns;
                            if (!neg_parse_time(d + soff, slen, &sec, &ns)) {
                                bad = true;
                            } else {
                                t_cond[ci].sec = sec;
                                t_cond[ci].nsec = ns;
                            }
                        }
                    }
                }
            }
            // N0: escaped strings, one at a time by the whole wave, the error kept by the lane whose node it is
            for (uint64_t m = ballot(slow); m; m &= m - 1) {
                const uint32_t src = (uint32_t)__builtin_ctzll(m);
                const uint32_t sop = rdlane(vop, src), scp = rdlane(vcp, src);
                if (!wave_string_ok(d + sop + 1, scp - sop - 1, d + len, S.str + sop + 1, lane) && lane == src)
                    err0 = GPUDIFF_TOK_STRING;
            }
        }
        wave_sync();
        err0 = wave_max_v(err0);
        bool fail = ballot(bad) != 0ull || n_meta > 1 || n_stat > 1 || mk > 2u || sk > 2u;
#pragma unroll
        for (uint32_t k = 0; k < 7; k++) fail |= n_f[k] > 1;
        if (fid[0] == NONE || fk[0] != 5u) {
            rv_off = 0;
            rv_len = 0;
            if (fid[0] != NONE && fk[0] != 0u) fail = true;
        }
        if (fid[1] != NONE) {
            if (g_bad) fail = true;
            else if (g_tag == GPUDIFF_TAG_INT) gen = (int64_t)g_val;
        }
        const uint32_t lk = fk[2], ak = fk[3], ck = fk[4], nk = fk[5], vk = fk[6];
        if (lk > 2u || ak > 2u || (ck != 0u && ck != 3u && ck != 4u)) fail = true;
        if (nk > 2u || (vk != 0u && vk != 3u && vk != 4u)) fail = true;
#pragma unroll
        for (uint32_t k = 0; k < 6; k++) fail |= n_nf[k] > 1;  // a repeated field: Go decodes it again (merges)
        if (n_lab > kNegMaxMembers || n_ann > kNegMaxMembers || n_cond > kNegMaxConds || n_stored > kNegMaxList)
            fail = true;
        if (nk == 2u) {
            const uint32_t sidx[4] = {0u, 1u, 3u, 4u};  // plural, singular, kind, listKind
#pragma unroll
            for (uint32_t q = 0; q < 4; q++) {
                if (nid[sidx[q]] == NONE) continue;
                if (nkd[sidx[q]] == 5u) names[q] = nsp[q];
                else if (nkd[sidx[q]] != 0u) fail = true;  // null: no-op on the zero string
            }
            const uint32_t shk = nkd[2], cak = nkd[5];
            if ((shk != 0u && shk != 3u && shk != 4u) || (cak != 0u && cak != 3u && cak != 4u)) fail = true;
            if (n_short > kNegMaxList || n_cat > kNegMaxList) fail = true;
        }
        {  // a repeated condition field: Go decodes it again, the host decides
            bool rep = false;
            for (uint32_t q = lane; q < min(n_cond, kNegMaxConds) * 5u; q += 64)
                if (t_cnt[q] > 1u) rep = true;
            if (ballot(rep)) fail = true;
        }
        if (err0) status = err0;
        else if (fail) status = GPUDIFF_TOK_FIELD;
        if (status == GPUDIFF_TOK_OK) {  // a repeated map key: Go keeps the last, the host decides
            bool dup = false;
            for (uint32_t q = lane; q < 2u * kNegMaxMembers * kNegMaxMembers; q += 64) {
                const uint32_t which = q / (kNegMaxMembers * kNegMaxMembers);
                const uint32_t a = (q / kNegMaxMembers) % kNegMaxMembers, b = q % kNegMaxMembers;
                const uint32_t nm = which ? n_ann : n_lab;
                const NegMember* tt = which ? t_ann : t_lab;
                if (a < b && b < nm && bytes_eq(d + tt[a].koff, tt[a].klen, d + tt[b].koff, tt[b].klen)) dup = true;
            }
            if (ballot(dup)) status = GPUDIFF_TOK_FIELD;
        }
    }
    // ---------------------------------------------------------- out
    if (status == GPUDIFF_TOK_OK) {
        const uint4* src = (const uint4*)t_lab;
        uint4* dst = (uint4*)O->lab;
        for (uint32_t q = lane; q < n_lab; q += 64) dst[q] = src[q];
        src = (const uint4*)t_ann;
        dst = (uint4*)O->ann;
        for (uint32_t q = lane; q < n_ann; q += 64) dst[q] = src[q];
        src = (const uint4*)t_cond;
        dst = (uint4*)O->cond;
        for (uint32_t q = lane; q < 3u * n_cond; q += 64) dst[q] = src[q];
        if (crd) {
            wave_sync();
            if (lane < n_short) O->shortn[lane] = t_short[lane];
            if (lane < n_cat) O->cat[lane] = t_cat[lane];
            if (lane < n_stored) O->stored[lane] = t_stored[lane];
        }
    }
    if (lane == 0) {
        O->status = status;
        O->n_lab = n_lab;
        O->n_ann = n_ann;
        O->n_cond = n_cond;
        O->rv_off = rv_off;
        O->rv_len = rv_len;
        O->gen = gen;
        O->n_short = n_short;
        O->n_cat = n_cat;
        O->n_stored = n_stored;
        if (crd)
#pragma unroll
            for (uint32_t q = 0; q < 4; q++) O->names[q] = names[q];
    }
    mark(PN_SWEEP);
}

}  // namespace

}  // namespace gd
