// Changed leaves' old and new values as JSON text (values.hip): the launchers of K21 / K22.
// Internal, not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gpudiff_format.h"

namespace gd {

// One diffed batch whose blobs are in HBM: its rows, the diff pass's changed-path lists (dirty_idx -> row,
// path_off CSR, out_h / out_k) and the space the blobs live in.  PathJob's arrays without ntab: the values come
// from the segments, so host-written and table-less blobs serve too.
struct ValueJob {
    const gpudiff_pair_row* rows;
    const uint32_t* dirty_idx;  // [n_dirty]
    const uint32_t* path_off;   // [n_dirty + 1]
    const uint64_t* out_h;      // [n_paths]
    const uint8_t* out_k;       // [n_paths]
    const uint8_t* space;
    uint64_t space_bytes;
    uint64_t mask;              // the context's path-hash mask: a hash with a bit outside it names no leaf
    uint32_t n_dirty, n_paths;
};

// what K21 found per entry and side (2 * entry + side; side 0 = old / A, 1 = new / B), so K22 searches nothing again
struct ValueSlot {
    uint32_t leaf;   // index in its region's segment, or 0xFFFFFFFF
    uint32_t arena;  // arena offset of a long string's tail
};

// K21 k_value_len + the scan's first two steps (scan64.h) over the 2 * n_paths texts: tags[2n], lens[2n],
// slots[2n], tile_sums[scan64_tiles(2n)] (exclusive), *total = the texts' bytes; *unresolved is zeroed here
hipError_t launch_value_len(hipStream_t s, const ValueJob& j, uint8_t* tags, uint64_t* lens, ValueSlot* slots,
                            uint64_t* tile_sums, unsigned long long* total, unsigned long long* unresolved);
// the scan's last step (offsets[2n + 1]) + K22 k_value_write: text t at bytes[offsets[t], offsets[t + 1])
hipError_t launch_value_write(hipStream_t s, const ValueJob& j, const uint8_t* tags, const uint64_t* lens,
                              const ValueSlot* slots, const uint64_t* tile_sums, uint64_t* offsets, uint8_t* bytes,
                              uint64_t bytes_cap, unsigned long long* unresolved);

}  // namespace gd
