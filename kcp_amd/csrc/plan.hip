// The write plan of a device-encode store batch (gfx950, wave64): gpudiff_store_write_plan_get lists one write per
// dirty slot of a waited watch-replay batch and renders the slot's last version of the batch with K10, all from what
// the batch left on its ring slot in HBM -- the document table and its slot chains, the staged JSON, the diff pass's
// flags (the rules are store_plan.h's, which the CPU test runs too).
//
//   k_plan_flags / k_plan_noop / k_plan_patch   the batch's final flags: the diff pass's flags, its no-op bits per
//                        dirty pair scattered to their rows, the host-resolved events' flags written over them
//   K17 k_plan_tails     lane per staged document: a chain tail walks prev to the head and folds the flags into its
//                        event's plan word (which writes, which of them no-ops); per 64-document wave a ballot /
//                        popcount of the writes by kind and of the ones with a body, per 1024-document tile their
//                        sums and the sums of K10's scratch and arena room (u64)
//   scan64 top           one block: the tile sums' exclusive scans, column by column, and the totals into the
//                        record the host reads (scan64.h launch_scan64_top over kPlanCols columns)
//   K18 k_plan_docs      the same tile prefix again, plus the tile's base: each write into the write list, each body
//                        into K10's TokDoc table -- document order is event order, so each kind comes out ascending
//   k_body_lens          K10's output sizes per write, then scanned (scan64.h: sums, top, offsets); with them K10's
//                        status and resourceVersion splice point, through the same wdoc indirection -- and, for a
//                        plan with GPUDIFF_PLAN_TARGETS, the body's request target (four words of the same TokOut)
//   K19 k_pack_bodies    wave per body: from its arena slot (2 x len + 512 B apart) to its byte-exact dense offset
//
// K19's copy works at dword granularity (store_plan.h plan_copy_body): a dense offset has any alignment, so each
// lane builds one dst-aligned dword from the two aligned source dwords holding its bytes (one shift pair) and
// stores 4 B; the few bytes before dst's first and behind its last 4-B boundary go as single bytes.  Chosen over
// aligned 16-B loads with realigned 16-B stores: a body is ~1 KiB, i.e. four dwords a lane, the kernel is bound by
// launch and first-touch latency rather than by issue rate, and the 16-B form needs eight loaded dwords and a
// four-way select per store for the same bytes.  Either way nothing outside [offset_w, offset_w+1) is written.
//
// All of these are latency-bound and tiny next to K10.  No atomics: every count comes out of a scan.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gpudiff.h"
#include "plan.h"
#include "scan64.h"
#include "store_plan.h"

namespace gd {

namespace {

// ---------------------------------------------------------------- final flags
__global__ __launch_bounds__(256) void k_plan_flags(const uint8_t* __restrict__ pass_flags, uint32_t nev,
                                                    uint8_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nev) flags[i] = plan_final_flags(pass_flags[i], 0);
}

__global__ __launch_bounds__(256) void k_plan_noop(const uint32_t* __restrict__ summary,
                                                   const uint32_t* __restrict__ dirty_idx,
                                                   const uint8_t* __restrict__ noop_d,
                                                   const uint8_t* __restrict__ pass_flags, uint32_t nev,
                                                   uint8_t* __restrict__ flags) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nev || k >= summary[2]) return;  // summary[2]: the pass's dirty pairs (each row at most once)
    const uint32_t row = dirty_idx[k];
    if (row < nev) flags[row] = plan_final_flags(pass_flags[row], noop_d[k]);
}

__global__ __launch_bounds__(256) void k_plan_patch(const PlanPatch* __restrict__ patch, uint32_t n, uint32_t nev,
                                                    uint8_t* __restrict__ flags) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const PlanPatch p = patch[k];
    if (p.row < nev) flags[p.row] = (uint8_t)p.flags;
}

// ---------------------------------------------------------------- the tile's prefix
// One tile of kPlanTile documents, a lane each (block of 1024 = 16 waves): this document's exclusive prefix inside
// the tile and the tile's total, per column.  The four counts by ballot / popcount per wave and a sum over the
// waves before it; the four byte sums by the block scan.
__device__ void tile_prefix(uint32_t w, uint32_t json_len, uint64_t pre[kPlanCols], uint64_t tot[kPlanCols],
                            uint64_t* tmp, uint32_t (*wave_cnt)[4]) {
    const uint32_t wave = threadIdx.x >> 6;
    const bool bit[4] = {(w & kPlanSpecWrite) != 0, (w & kPlanStatusWrite) != 0,
                         (w & kPlanSpecWrite) && !(w & kPlanSpecNoop), (w & kPlanStatusWrite) && !(w & kPlanStatusNoop)};
    uint32_t before[4];
    for (uint32_t c = 0; c < 4; c++) {
        const uint64_t m = __ballot(bit[c]);
        before[c] = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (__lane_id() == 0) wave_cnt[wave][c] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    const uint32_t waves = blockDim.x >> 6;
    for (uint32_t c = 0; c < 4; c++) {
        uint32_t base = 0, total = 0;
        for (uint32_t v = 0; v < waves; v++) {
            const uint32_t x = wave_cnt[v][c];
            base += v < wave ? x : 0u;
            total += x;
        }
        pre[c] = base + before[c];
        tot[c] = total;
    }
    const uint64_t scr = marshal_scratch_bytes(json_len), cap = marshal_out_cap(json_len);
    const uint64_t v[4] = {bit[2] ? scr : 0ull, bit[2] ? cap : 0ull, bit[3] ? scr : 0ull, bit[3] ? cap : 0ull};
    for (uint32_t c = 0; c < 4; c++) pre[4 + c] = block_excl_scan_u64(v[c], tmp, &tot[4 + c]);
}

// ---------------------------------------------------------------- K17
__global__ __launch_bounds__(kPlanTile) void k_plan_tails(const PlanIn in, uint8_t* __restrict__ words,
                                                          uint64_t* __restrict__ tiles) {
    __shared__ uint64_t tmp[kPlanTile];
    __shared__ uint32_t wave_cnt[kPlanTile / 64][4];
    const uint32_t i = blockIdx.x * kPlanTile + threadIdx.x;
    uint32_t w = 0, len = 0;
    if (i < in.nd) {
        w = plan_word(in.links, in.nd, in.flags, in.nev, i, in.kinds);
        words[i] = (uint8_t)w;
        if (w) len = in.docs[i].json_len;
    }
    uint64_t pre[kPlanCols], tot[kPlanCols];
    tile_prefix(w, len, pre, tot, tmp, wave_cnt);
    if (threadIdx.x == 0)
        for (uint32_t c = 0; c < kPlanCols; c++) tiles[(uint64_t)blockIdx.x * kPlanCols + c] = tot[c];
}

// ---------------------------------------------------------------- K18
__global__ __launch_bounds__(kPlanTile) void k_plan_docs(const PlanIn in, const uint8_t* __restrict__ words,
                                                         const uint64_t* __restrict__ tiles,
                                                         const uint64_t* __restrict__ rec, const PlanLists out) {
    __shared__ uint64_t tmp[kPlanTile];
    __shared__ uint32_t wave_cnt[kPlanTile / 64][4];
    const uint32_t i = blockIdx.x * kPlanTile + threadIdx.x;
    uint32_t w = 0;
    TokDoc src{};
    if (i < in.nd) {
        w = words[i];
        if (w) src = in.docs[i];
    }
    uint64_t pre[kPlanCols], tot[kPlanCols];
    tile_prefix(w, src.json_len, pre, tot, tmp, wave_cnt);
    if (!w) return;
    for (uint32_t c = 0; c < kPlanCols; c++) pre[c] += tiles[(uint64_t)blockIdx.x * kPlanCols + c];
    const uint32_t row = in.links[i].row;
    // spec writes, then status writes; K10's documents likewise, and each kind's launch has the scratch to itself
    const uint64_t write_base[2] = {0, rec[kColSpecWrites]}, doc_base[2] = {0, rec[kColSpecDocs]};
    const uint64_t cap_base[2] = {0, rec[kColSpecCap]};
    for (uint32_t k = 0; k < 2; k++) {
        if (!(w & (k ? kPlanStatusWrite : kPlanSpecWrite))) continue;
        const bool noop = (w & (k ? kPlanStatusNoop : kPlanSpecNoop)) != 0;
        const uint64_t wi = write_base[k] + pre[kColSpecWrites + k], di = doc_base[k] + pre[kColSpecDocs + k];
        if (wi < out.n_writes) {
            out.pair_index[wi] = row;
            out.src_doc[wi] = i;
            out.kind[wi] = (uint8_t)(k ? GPUDIFF_UPSERT_STATUS : GPUDIFF_UPSERT_SPEC);
            out.noop[wi] = noop ? 1 : 0;
            out.wdoc[wi] = noop ? kPlanNoDoc : (uint32_t)di;
        }
        if (noop || di >= out.n_docs) continue;
        TokDoc t{};
        t.json_off = src.json_off;
        t.json_len = src.json_len;
        t.seed = 0;
        t.scratch_off = pre[kColSpecScratch + 2 * k];
        tokdoc_set_marshal_off(t, cap_base[k] + pre[kColSpecCap + 2 * k]);
        out.tdocs[di] = t;
    }
}

// ---------------------------------------------------------------- K19
__global__ __launch_bounds__(256) void k_body_lens(const uint32_t* __restrict__ wdoc, const TokOut* __restrict__ touts,
                                                   uint32_t n_writes, uint32_t n_docs, uint64_t* __restrict__ lens,
                                                   uint32_t* __restrict__ k10, TargetWords* __restrict__ tgt) {
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_writes) return;
    const uint32_t d = wdoc[w];
    uint64_t len = 0;
    uint32_t st = GPUDIFF_TOK_OK, ro = 0, rf = GPUDIFF_RV_NONE;
    TargetWords tw{};  // a no-op write, a body left to the host: all zero
    if (d < n_docs) {  // kPlanNoDoc: a no-op write
        const TokOut t = touts[d];
        st = t.status;
        if (st == GPUDIFF_TOK_OK) {
            len = t.bytes;
            ro = tokout_rv_off(t);
            rf = tokout_rv_form(t);
            tw = tokout_targets(t);
        }
    }
    lens[w] = len;
    if (tgt) tgt[w] = tw;
    k10[w] = plan_k10_word(st, ro, rf);
}

__global__ __launch_bounds__(256) void k_pack_bodies(const uint32_t* __restrict__ wdoc,
                                                     const TokOut* __restrict__ touts, uint32_t n_writes,
                                                     uint32_t n_docs, const uint64_t* __restrict__ offsets,
                                                     const uint8_t* __restrict__ arena, uint64_t arena_bytes,
                                                     uint8_t* __restrict__ bytes, uint64_t bytes_cap) {
    const uint32_t lane = __lane_id();
    const uint32_t w = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (w >= n_writes) return;
    const uint64_t o0 = offsets[w], o1 = offsets[w + 1];
    if (o1 <= o0 || o1 > bytes_cap) return;  // no body, or a slot that does not lie inside the buffer
    const uint32_t d = wdoc[w];
    if (d >= n_docs) return;
    const uint64_t src = touts[d].off, len = o1 - o0;
    // the arena is allocated 4-B aligned with 16 B of slack behind arena_bytes (the copy reads whole dwords)
    if (src > arena_bytes || len > arena_bytes - src) return;
    plan_copy_body(bytes + o0, arena + src, len, lane);
}

}  // namespace

// ---------------------------------------------------------------- launchers
hipError_t launch_plan_flags(hipStream_t s, const uint8_t* pass_flags, const uint32_t* summary,
                             const uint32_t* dirty_idx, const uint8_t* noop_d, const PlanPatch* patch,
                             uint32_t n_patch, uint32_t nev, uint8_t* flags) {
    if (!nev) return hipSuccess;
    const uint32_t blocks = (nev + 255) / 256;
    k_plan_flags<<<blocks, 256, 0, s>>>(pass_flags, nev, flags);
    k_plan_noop<<<blocks, 256, 0, s>>>(summary, dirty_idx, noop_d, pass_flags, nev, flags);
    if (n_patch) k_plan_patch<<<(n_patch + 255) / 256, 256, 0, s>>>(patch, n_patch, nev, flags);
    return hipGetLastError();
}

hipError_t launch_plan_tails(hipStream_t s, const PlanIn& in, uint8_t* words, uint64_t* tiles, uint64_t* rec) {
    if (!in.nd) return hipMemsetAsync(rec, 0, 8ull * kPlanCols, s);
    const uint32_t nt = scan64_tiles(in.nd);
    k_plan_tails<<<nt, kPlanTile, 0, s>>>(in, words, tiles);
    return launch_scan64_top(s, tiles, nt, kPlanCols, rec);
}

hipError_t launch_plan_docs(hipStream_t s, const PlanIn& in, const uint8_t* words, const uint64_t* tiles,
                            const uint64_t* rec, const PlanLists& out) {
    if (!in.nd || !out.n_writes) return hipSuccess;
    k_plan_docs<<<scan64_tiles(in.nd), kPlanTile, 0, s>>>(in, words, tiles, rec, out);
    return hipGetLastError();
}

hipError_t launch_body_lens(hipStream_t s, const uint32_t* wdoc, const TokOut* touts, uint32_t n_writes,
                            uint32_t n_docs, uint64_t* lens, uint32_t* k10, TargetWords* tgt, uint64_t* tiles,
                            uint64_t* rec) {
    if (!n_writes) return hipMemsetAsync(rec, 0, 8, s);
    k_body_lens<<<(n_writes + 255) / 256, 256, 0, s>>>(wdoc, touts, n_writes, n_docs, lens, k10, tgt);
    return launch_scan64_sums(s, lens, n_writes, tiles, rec);
}

hipError_t launch_pack_bodies(hipStream_t s, const uint32_t* wdoc, const TokOut* touts, uint32_t n_writes,
                              uint32_t n_docs, const uint64_t* lens, const uint64_t* tiles, uint64_t* offsets,
                              const uint8_t* arena, uint64_t arena_bytes, uint8_t* bytes, uint64_t bytes_cap) {
    if (!n_writes) return hipMemsetAsync(offsets, 0, 8, s);
    const hipError_t e = launch_scan64_offsets(s, lens, n_writes, tiles, offsets);
    if (e != hipSuccess) return e;
    k_pack_bodies<<<(n_writes + 3) / 4, 256, 0, s>>>(wdoc, touts, n_writes, n_docs, offsets, arena, arena_bytes, bytes,
                                                     bytes_cap);
    return hipGetLastError();
}

}  // namespace gd
