// Launches of the cluster index's kernels K23 - K25 (fanout.hip), of the stable sort between them, and of K26 - K28
// (fanout_live.hip).  Every dependency between the steps is a kernel boundary on stream s.  Internal, not part of the
// ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gpudiff.h"
#include "fanout.h"
#include "plan.h"

namespace gd {

constexpr uint32_t kFanCols = 3;  // the tile sums' columns: heads, spec-dirty, status-dirty
// bits of K23's control word (zeroed before the launch)
constexpr uint32_t kFanUnsorted = 1u;  // some entry's cluster is smaller than its predecessor's
constexpr uint32_t kFanBadRow = 2u;    // a dirty_idx entry names no row of the batch

// K23: key[k] = rows[dirty_idx[k]].cluster_id, val[k] = k for k < n_dirty; *ctl |= kFanUnsorted / kFanBadRow.
// *ctl is zeroed on s first.  n_dirty > 0.
hipError_t launch_fan_keys(hipStream_t s, const gpudiff_pair_row* rows, uint32_t n_pairs, const uint32_t* dirty_idx,
                           uint32_t n_dirty, uint32_t* key, uint32_t* val, uint32_t* ctl);
// bytes of temporary storage launch_fan_sort needs for n entries
size_t fan_sort_temp_bytes(uint32_t n);
// (key, val) -> (key_out, val_out) ascending by key, stable (radix sort over all 32 bits)
hipError_t launch_fan_sort(hipStream_t s, void* temp, size_t temp_bytes, const uint32_t* key, uint32_t* key_out,
                           const uint32_t* val, uint32_t* val_out, uint32_t n);
// K24 + the scan of its tile sums: tiles[scan64_tiles(n) * kFanCols] becomes each tile's exclusive base per column,
// totals[kFanCols] = (n_clusters, n_spec, n_status)
hipError_t launch_fan_marks(hipStream_t s, const uint32_t* key, const uint32_t* val, const uint32_t* dirty_idx,
                            const uint8_t* flags, uint32_t n_pairs, uint32_t n, uint64_t* tiles, uint64_t* totals);
// K25: the packed block (fanout.h FanLayout l of the counts nc / ns / nt that launch_fan_marks' totals gave)
hipError_t launch_fan_emit(hipStream_t s, const uint32_t* key, const uint32_t* val, const uint32_t* dirty_idx,
                           const uint32_t* dirty_ids, const uint8_t* flags, uint32_t n_pairs, uint32_t n,
                           const uint64_t* tiles, uint32_t nc, uint32_t ns, uint32_t nt, uint32_t* block);

// ---- fanout_live.hip: the dirty list of a batch whose deferred rows the host resolved, under their final flags
// K26: *ctl is zeroed on s, fin[n_pairs] = flags[n_pairs] (device to device), then fin[patch[k].row] = patch[k].flags
// for k < n_patch; a row >= n_pairs writes nothing and sets kFanBadRow in *ctl
hipError_t launch_fan_patch(hipStream_t s, const uint8_t* flags, uint32_t n_pairs, const PlanPatch* patch,
                            uint32_t n_patch, uint8_t* fin, uint32_t* ctl);
// K27 + the scan of its tile sums: tiles[scan64_tiles(n)] becomes each tile's exclusive base, *total = the entries k <
// n of dirty_idx with fin[dirty_idx[k]] dirty in some kind.  n > 0.
hipError_t launch_fan_live_marks(hipStream_t s, const uint32_t* dirty_idx, uint32_t n, const uint8_t* fin,
                                 uint32_t n_pairs, uint64_t* tiles, uint64_t* total);
// K28: those entries' rows and pair ids, in list order, into live_idx / live_ids[n_live] (n_live = K27's total)
hipError_t launch_fan_live_emit(hipStream_t s, const uint32_t* dirty_idx, const uint32_t* dirty_ids, uint32_t n,
                                const uint8_t* fin, uint32_t n_pairs, const uint64_t* tiles, uint32_t n_live,
                                uint32_t* live_idx, uint32_t* live_ids);

}  // namespace gd
