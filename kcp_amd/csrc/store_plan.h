// The write plan of a device-encode store batch (plan.hip, gpudiff_store_write_plan_get): the rules the kernels
// and the CPU test both run.  No HIP runtime call; the functions are __host__ __device__.
//
// One write per dirty slot, rendering the slot's last version of the batch.  A slot's events of one
// batch are a DocLink chain (prev / next) in the batch's document table; its tail is the last event's new document.
// For kind K (spec, status), over the chain's documents that have a result row:
//   dirty_K = OR of the events' GPUDIFF_SPEC_DIRTY / GPUDIFF_STATUS_DIRTY
//   noop_K  = dirty_K and every event carrying the dirty bit of K also carries GPUDIFF_SPEC_NOOP / GPUDIFF_STATUS_NOOP
// A first sighting's old_json document (row == kNoRow) has no row and contributes nothing.
#pragma once
#include <stdint.h>

#include "../../include/gpudiff.h"
#include "tokenize.h"

namespace gd {

// per staged document (nonzero on chain tails only): the writes its event gets
constexpr uint32_t kPlanSpecWrite = 1u, kPlanStatusWrite = 2u, kPlanSpecNoop = 4u, kPlanStatusNoop = 8u;

// Folds the chain that ends in document `tail` (walking prev to the head) over the batch's final flags.
// links[nd], flags[nev].  A link or row outside the tables ends the walk / is skipped, and the walk takes at most
// nd steps, so a damaged table cannot run it out of bounds or forever.
__host__ __device__ inline uint32_t plan_fold_chain(const DocLink* links, uint32_t nd, const uint8_t* flags,
                                                    uint32_t nev, uint32_t tail) {
    uint32_t dirty = 0, real = 0;
    int64_t doc = tail;
    for (uint32_t step = 0; step < nd && doc >= 0 && doc < (int64_t)nd; step++) {
        const uint32_t row = links[doc].row;
        if (row != kNoRow && row < nev) {
            const uint32_t f = flags[row];
            dirty |= f & (GPUDIFF_SPEC_DIRTY | GPUDIFF_STATUS_DIRTY);
            if ((f & GPUDIFF_SPEC_DIRTY) && !(f & GPUDIFF_SPEC_NOOP)) real |= GPUDIFF_SPEC_DIRTY;
            if ((f & GPUDIFF_STATUS_DIRTY) && !(f & GPUDIFF_STATUS_NOOP)) real |= GPUDIFF_STATUS_DIRTY;
        }
        doc = links[doc].prev;
    }
    uint32_t w = 0;
    if (dirty & GPUDIFF_SPEC_DIRTY) w |= kPlanSpecWrite | ((real & GPUDIFF_SPEC_DIRTY) ? 0u : kPlanSpecNoop);
    if (dirty & GPUDIFF_STATUS_DIRTY) w |= kPlanStatusWrite | ((real & GPUDIFF_STATUS_DIRTY) ? 0u : kPlanStatusNoop);
    return w;
}

// The plan word of document i: zero unless it is a chain tail with a row; `kinds` = GPUDIFF_PLAN_SPEC |
// GPUDIFF_PLAN_STATUS bits of the writes to list.
__host__ __device__ inline uint32_t plan_word(const DocLink* links, uint32_t nd, const uint8_t* flags, uint32_t nev,
                                              uint32_t i, uint32_t kinds) {
    if (links[i].next != -1 || links[i].row == kNoRow) return 0;
    uint32_t w = plan_fold_chain(links, nd, flags, nev, i);
    if (!(kinds & GPUDIFF_PLAN_SPEC)) w &= ~(kPlanSpecWrite | kPlanSpecNoop);
    if (!(kinds & GPUDIFF_PLAN_STATUS)) w &= ~(kPlanStatusWrite | kPlanStatusNoop);
    return w;
}

// a row's final flags from what the diff pass left in HBM (api.cpp collect_results does the same on the host):
// the no-op bits count only for a region that is dirty, and never beside a decode error
__host__ __device__ inline uint8_t plan_final_flags(uint8_t pass_flags, uint8_t noop_bits) {
    uint8_t f = pass_flags & (uint8_t)(GPUDIFF_SPEC_DIRTY | GPUDIFF_STATUS_DIRTY | GPUDIFF_DECODE_ERROR);
    if (f & GPUDIFF_DECODE_ERROR) return f;
    if ((noop_bits & 1u) && (f & GPUDIFF_SPEC_DIRTY)) f |= GPUDIFF_SPEC_NOOP;
    if ((noop_bits & 2u) && (f & GPUDIFF_STATUS_DIRTY)) f |= GPUDIFF_STATUS_NOOP;
    return f;
}

// K10's verdict per write, one word in the write list that comes back (k_body_lens packs, dstore_write_plan unpacks):
// a status other than GPUDIFF_TOK_OK as it is -- the host renders that body and works out its own descriptor -- else
// bit 31 with the body's resourceVersion splice point (include/gpudiff.h GPUDIFF_RV_*): the form in bits 26-29, the
// body-relative offset in bits 0-25.  The word the status alone used to take, so the list stays 22 B a write.
constexpr uint32_t kPlanRvBit = 1u << 31, kPlanRvFormShift = 26, kPlanRvOffMask = (1u << kPlanRvFormShift) - 1u;
static_assert(2ull * kTokMaxLen + 512u + 15u <= kPlanRvOffMask, "an offset inside marshal_out_cap(len) fits 26 bits");
static_assert(((GPUDIFF_RV_INSERT | GPUDIFF_RV_LEAD | GPUDIFF_RV_TRAIL | GPUDIFF_RV_WRAP) << kPlanRvFormShift) <
                  kPlanRvBit, "the form fits below bit 31");
static_assert(kTgtFlagShift == kPlanRvFormShift, "a target offset (tokenize.h TargetWords) fits the same 26 bits");
__host__ __device__ inline uint32_t plan_k10_word(uint32_t status, uint32_t rv_off, uint32_t rv_form) {
    return status != GPUDIFF_TOK_OK ? status & ~kPlanRvBit
                                    : kPlanRvBit | (rv_form << kPlanRvFormShift) | (rv_off & kPlanRvOffMask);
}
__host__ __device__ inline void plan_k10_unpack(uint32_t word, int32_t* status, uint32_t* rv_off, uint32_t* rv_form) {
    const bool ok = (word & kPlanRvBit) != 0u || word == GPUDIFF_TOK_OK;
    *status = ok ? (int32_t)GPUDIFF_TOK_OK : (int32_t)word;
    *rv_off = ok ? word & kPlanRvOffMask : 0u;
    *rv_form = ok ? (word & ~kPlanRvBit) >> kPlanRvFormShift : (uint32_t)GPUDIFF_RV_NONE;
}

// K19's copy of one body, this lane's share (lane of 64): n bytes from src to dst, both of any alignment.
// Dword granularity: the bytes up to dst's first 4-B boundary and behind its last one go as single bytes, every
// dword between is one aligned 4-B store built from the one or two aligned source dwords that hold its bytes.
// Writes only [dst, dst + n).  Reads whole aligned dwords around src's bytes: up to 3 bytes before src and 3
// behind src + n lie in the same aligned dwords as bytes of the body, so the source needs 4-B-aligned bounds
// (K10's arena slots are 16-B multiples).
__host__ __device__ inline void plan_copy_body(uint8_t* dst, const uint8_t* src, uint64_t n, uint32_t lane) {
    uint64_t head = (4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u;
    if (head > n) head = n;
    if (lane < head) dst[lane] = src[lane];
    const uint64_t nw = (n - head) >> 2;
    const uintptr_t a0 = (uintptr_t)(src + head);
    const uint32_t sh = (uint32_t)(a0 & 3u) * 8u;
    const uint32_t* s4 = (const uint32_t*)(a0 & ~(uintptr_t)3u);
    uint32_t* d4 = (uint32_t*)(dst + head);
    for (uint64_t k = lane; k < nw; k += 64) {
        const uint32_t lo = s4[k];
        d4[k] = sh ? (lo >> sh) | (s4[k + 1] << (32u - sh)) : lo;
    }
    const uint64_t done = head + 4u * nw, tail = n - done;
    if (lane < tail) dst[done + lane] = src[done + lane];
}

}  // namespace gd
