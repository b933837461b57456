// The device side of gpudiff_store_write_plan_get (plan.hip): launchers and the tables they share with
// dstore.cpp.  Internal, not part of the ABI.  The rules themselves are in store_plan.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan64.h"
#include "tokenize.h"

namespace gd {

// one waited device-encode store batch, as it lies on its ring slot in HBM
struct PlanIn {
    const TokDoc* docs;     // [nd] the staged documents (json_off / json_len into the staged JSON)
    const DocLink* links;   // [nd] their slot chains
    uint32_t nd;
    const uint8_t* flags;   // [nev] the batch's final result flags (launch_plan_flags)
    uint32_t nev;
    uint32_t kinds;         // GPUDIFF_PLAN_SPEC | GPUDIFF_PLAN_STATUS
};

// a host-resolved event's final flags, written over the diff pass's
struct PlanPatch {
    uint32_t row, flags;
};

constexpr uint32_t kPlanTile = 1024;  // K17 / K18's block: a lane per document, one scan tile per block
static_assert(kPlanTile == kScanTile, "K17 / K18 write one row of tile sums per block");
// the record the host sizes the buffers by (u64 each), and the columns of K17's tile sums
enum PlanCol : uint32_t {
    kColSpecWrites = 0, kColStatusWrites, kColSpecDocs, kColStatusDocs,
    kColSpecScratch, kColSpecCap, kColStatusScratch, kColStatusCap, kPlanCols
};

// the compacted plan: the write list (spec writes first, each kind ascending by event) and K10's documents (spec
// documents first)
struct PlanLists {
    uint32_t* pair_index;  // [n_writes] the event's index in the submitted array
    uint32_t* src_doc;     // [n_writes] the staged document the write renders
    uint32_t* wdoc;        // [n_writes] its K10 document, kPlanNoDoc for a no-op write
    uint8_t* kind;         // [n_writes] GPUDIFF_UPSERT_SPEC / GPUDIFF_UPSERT_STATUS
    uint8_t* noop;         // [n_writes]
    TokDoc* tdocs;         // [n_docs]
    uint32_t n_writes, n_docs;  // the room: nothing is written at or past these
};
constexpr uint32_t kPlanNoDoc = 0xFFFFFFFFu;

// flags[nev] = the diff pass's flags with its no-op bits (per dirty pair: dirty_idx / noop_d, summary[2] of them)
// merged as gpudiff_wait merges them, then the n_patch host-resolved rows written over them
hipError_t launch_plan_flags(hipStream_t s, const uint8_t* pass_flags, const uint32_t* summary,
                             const uint32_t* dirty_idx, const uint8_t* noop_d, const PlanPatch* patch,
                             uint32_t n_patch, uint32_t nev, uint8_t* flags);
// K17 + the scan's first two steps: words[nd] (store_plan.h plan_word), tiles[scan64_tiles(nd) * kPlanCols]
// (exclusive, per column), rec[kPlanCols] = the totals
hipError_t launch_plan_tails(hipStream_t s, const PlanIn& in, uint8_t* words, uint64_t* tiles, uint64_t* rec);
// K18: the scan's last step and the compaction into `out`
hipError_t launch_plan_docs(hipStream_t s, const PlanIn& in, const uint8_t* words, const uint64_t* tiles,
                            const uint64_t* rec, const PlanLists& out);
// per write, the bytes K10 rendered for it (0: a no-op write, or a document K10 left to the host) and K10's verdict
// word (store_plan.h plan_k10_word: a status that leaves the body to the host, else the body's resourceVersion splice
// point -- body-relative, so packing keeps it); tile sums of the lengths; rec[0] = their total.  tgt (or null:
// not asked for): per write, the body's request target words (tokenize.h TargetWords), body-relative too
hipError_t launch_body_lens(hipStream_t s, const uint32_t* wdoc, const TokOut* touts, uint32_t n_writes,
                            uint32_t n_docs, uint64_t* lens, uint32_t* k10, TargetWords* tgt, uint64_t* tiles,
                            uint64_t* rec);
// offsets[n_writes + 1] (dense, byte-exact) + K19: body w from its arena slot to bytes[offsets[w], offsets[w + 1])
hipError_t launch_pack_bodies(hipStream_t s, const uint32_t* wdoc, const TokOut* touts, uint32_t n_writes,
                              uint32_t n_docs, const uint64_t* lens, const uint64_t* tiles, uint64_t* offsets,
                              const uint8_t* arena, uint64_t arena_bytes, uint8_t* bytes, uint64_t bytes_cap);

}  // namespace gd
