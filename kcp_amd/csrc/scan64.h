// The one device-wide exclusive u64 scan (scan64.hip): the store's compaction (K8, dstore.hip), the path strings'
// offsets (K15 / K16, paths.hip) and the write plan's counts and body offsets (K17 - K19, plan.hip) all size their
// outputs by it.  Tiles of kScanTile values: per-tile sums, a one-block exclusive scan of the sums (which also gives
// the grand total the host sizes a buffer by), then each tile rescans its values on top of its base -- in
// launch_scan64_offsets, or inside a kernel of the caller's that needs the tile's prefix anyway (k_pack_slots,
// K17 / K18's tile_prefix), with the block scan below.  Internal, not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gd {

constexpr uint32_t kScanTile = 1024;  // values per tile: 256 threads x 4 in the kernels of scan64.hip
inline uint32_t scan64_tiles(uint32_t n) { return (n + kScanTile - 1) / kScanTile; }

// tile_sums[scan64_tiles(n)] = the exclusive scan of the sums of in[n]'s tiles, *total = the sum of in[n].  n > 0.
hipError_t launch_scan64_sums(hipStream_t s, const uint64_t* in, uint32_t n, uint64_t* tile_sums, uint64_t* total);
// The second step alone, one block, over `cols` interleaved columns: tiles[t * cols + c] becomes the exclusive scan
// down column c, totals[c] the column's sum.  n_tiles > 0.
hipError_t launch_scan64_top(hipStream_t s, uint64_t* tiles, uint32_t n_tiles, uint32_t cols, uint64_t* totals);
// offsets[i] = the exclusive prefix of in[i] for i < n and offsets[n] = the end, from launch_scan64_sums' tile_sums.
// n > 0.
hipError_t launch_scan64_offsets(hipStream_t s, const uint64_t* in, uint32_t n, const uint64_t* tile_sums,
                                 uint64_t* offsets);

#ifdef __HIPCC__
// Exclusive scan of v over the block (Hillis-Steele in LDS, any blockDim.x), every thread calling it: returns the sum
// of the lower threads' v, *total = the block's sum.  tmp: blockDim.x u64 of LDS, free again on return.
__device__ inline uint64_t block_excl_scan_u64(uint64_t v, uint64_t* tmp, uint64_t* total) {
    const uint32_t t = threadIdx.x;
    tmp[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < blockDim.x; d <<= 1) {
        const uint64_t o = t >= d ? tmp[t - d] : 0ull;
        __syncthreads();
        tmp[t] += o;
        __syncthreads();
    }
    const uint64_t incl = tmp[t];
    *total = tmp[blockDim.x - 1];
    __syncthreads();
    return incl - v;
}
#endif

}  // namespace gd
