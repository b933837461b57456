// The cluster index of a batch whose deferred rows the host resolved (gfx950, wave64; include/gpudiff.h
// gpudiff_cluster_index_get_final, DESIGN.md §4m "Final flags").  The pass's flags in HBM are the conservative ones
// K0x wrote for those rows; their final flags live on the host (Ring::plan_patch).  The final dirty set is a subset of
// the pass's dirty list, so the list is filtered, never rebuilt:
//
//   K26 k_fan_patch       fin[n_pairs] starts as a device-to-device copy of the pass's flags; a lane per host-resolved
//                         row writes fin[row] = its final flags.  A row at or beyond n_pairs writes nothing and ORs
//                         kFanBadRow into the control word (one atomic per wave that has something to report)
//   K27 k_fan_live_marks  block per tile of kScanTile entries of the pass's dirty list, 4 a thread (16-byte loads):
//                         live = fin[dirty_idx[k]] & (SPEC | STATUS); the tile's count into one column, scanned by
//                         launch_scan64_top -- the total is the number of live entries
//   K28 k_fan_live_emit   same tiling: the tile's prefixes again, then every live entry k writes live_idx[j] =
//                         dirty_idx[k], live_ids[j] = dirty_ids[k] at its rank j.  Only when entries were dropped
//
// K23 - K25 (fanout.hip) then run unchanged over (rows, live_idx, live_ids, fin, n_live).  Every dependency between
// the steps is a kernel boundary; plain stores; no LDS beyond the block scans.
#include <hip/hip_runtime.h>

#include "fanout_dev.h"
#include "scan64.h"

namespace gd {

namespace {

__global__ __launch_bounds__(256) void k_fan_patch(const PlanPatch* __restrict__ patch, uint32_t n_patch,
                                                   uint32_t n_pairs, uint8_t* __restrict__ fin,
                                                   uint32_t* __restrict__ ctl) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    int bad = 0;
    if (k < n_patch) {
        const PlanPatch p = patch[k];
        if (p.row < n_pairs) fin[p.row] = (uint8_t)p.flags;
        else bad = 1;  // nothing written; the host refuses the index
    }
    // every lane arrives here
    if (__any(bad) && (threadIdx.x & 63u) == 0) atomicOr(ctl, kFanBadRow);
}

// The thread's 4 consecutive entries of the pass's dirty list: their rows, and bit i of the result set when entry
// base + i is live.  An entry behind the end, or one that names no row of the batch, is not live: the total then
// misses the host's count and the host refuses the index.
__device__ inline uint32_t fan_live4(const uint32_t* __restrict__ dirty_idx, uint32_t n,
                                     const uint8_t* __restrict__ fin, uint32_t n_pairs, uint64_t base, uint32_t r[4]) {
    if (base + 3 < n) {  // base is a multiple of 4: a 16-byte load
        const uint4 rr = *(const uint4*)(dirty_idx + base);
        r[0] = rr.x, r[1] = rr.y, r[2] = rr.z, r[3] = rr.w;
    } else {
        for (uint32_t i = 0; i < 4; i++) r[i] = base + i < n ? dirty_idx[base + i] : n_pairs;
    }
    uint32_t live = 0;
    for (uint32_t i = 0; i < 4; i++)
        if (base + i < n && r[i] < n_pairs && (fin[r[i]] & (GPUDIFF_SPEC_DIRTY | GPUDIFF_STATUS_DIRTY))) live |= 1u << i;
    return live;
}

__global__ __launch_bounds__(256) void k_fan_live_marks(const uint32_t* __restrict__ dirty_idx, uint32_t n,
                                                        const uint8_t* __restrict__ fin, uint32_t n_pairs,
                                                        uint64_t* __restrict__ tiles) {
    __shared__ uint64_t tmp[256];
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + threadIdx.x * 4u;
    uint32_t r[4];
    const uint32_t live = fan_live4(dirty_idx, n, fin, n_pairs, base, r);
    uint64_t total;
    (void)block_excl_scan_u64((uint64_t)__popc(live), tmp, &total);
    if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_fan_live_emit(const uint32_t* __restrict__ dirty_idx,
                                                       const uint32_t* __restrict__ dirty_ids, uint32_t n,
                                                       const uint8_t* __restrict__ fin, uint32_t n_pairs,
                                                       const uint64_t* __restrict__ tiles, uint32_t n_live,
                                                       uint32_t* __restrict__ live_idx,
                                                       uint32_t* __restrict__ live_ids) {
    __shared__ uint64_t tmp[256];
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + threadIdx.x * 4u;
    uint32_t r[4];
    const uint32_t live = fan_live4(dirty_idx, n, fin, n_pairs, base, r);
    uint64_t total;
    // the rank of this thread's first live entry; every index below is checked against the count the lists were
    // sized by
    uint64_t j = tiles[blockIdx.x] + block_excl_scan_u64((uint64_t)__popc(live), tmp, &total);
    for (uint32_t i = 0; i < 4; i++) {
        if (!(live & (1u << i))) continue;  // live entries have base + i < n
        if (j < n_live) {
            live_idx[j] = r[i];
            live_ids[j] = dirty_ids[base + i];
        }
        j++;
    }
}

}  // namespace

hipError_t launch_fan_patch(hipStream_t s, const uint8_t* flags, uint32_t n_pairs, const PlanPatch* patch,
                            uint32_t n_patch, uint8_t* fin, uint32_t* ctl) {
    hipError_t e = hipMemsetAsync(ctl, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(fin, flags, n_pairs, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess || !n_patch) return e;
    k_fan_patch<<<(n_patch + 255u) / 256u, 256, 0, s>>>(patch, n_patch, n_pairs, fin, ctl);
    return hipGetLastError();
}

hipError_t launch_fan_live_marks(hipStream_t s, const uint32_t* dirty_idx, uint32_t n, const uint8_t* fin,
                                 uint32_t n_pairs, uint64_t* tiles, uint64_t* total) {
    const uint32_t n_tiles = scan64_tiles(n);
    k_fan_live_marks<<<n_tiles, 256, 0, s>>>(dirty_idx, n, fin, n_pairs, tiles);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_scan64_top(s, tiles, n_tiles, 1, total);
}

hipError_t launch_fan_live_emit(hipStream_t s, const uint32_t* dirty_idx, const uint32_t* dirty_ids, uint32_t n,
                                const uint8_t* fin, uint32_t n_pairs, const uint64_t* tiles, uint32_t n_live,
                                uint32_t* live_idx, uint32_t* live_ids) {
    k_fan_live_emit<<<scan64_tiles(n), 256, 0, s>>>(dirty_idx, dirty_ids, n, fin, n_pairs, tiles, n_live, live_idx,
                                                    live_ids);
    return hipGetLastError();
}

}  // namespace gd
