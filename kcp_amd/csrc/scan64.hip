// The device-wide exclusive u64 scan of scan64.h (gfx950, wave64), three small kernels of 256 threads:
//
//   k_scan64_tiles     block per tile of kScanTile values, 4 a thread: the tile's sum
//   k_scan64_top       one block: the tile sums' exclusive scan in place, 256 tiles a trip with a running total,
//                      column by column; each column's total
//   k_scan64_offsets   block per tile: the values' exclusive scan on top of the tile's base, and the end behind the
//                      last value
//
// All three are bound by launch latency: their callers scan a few thousand values between two host round trips.
#include "scan64.h"

namespace gd {

namespace {

__global__ __launch_bounds__(256) void k_scan64_tiles(const uint64_t* __restrict__ in, uint32_t n,
                                                      uint64_t* __restrict__ tile_sums) {
    __shared__ uint64_t tmp[256];
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + threadIdx.x * 4u;
    uint64_t s = 0;
    for (uint32_t k = 0; k < 4; k++)
        if (base + k < n) s += in[base + k];
    uint64_t total;
    (void)block_excl_scan_u64(s, tmp, &total);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_scan64_top(uint64_t* __restrict__ tiles, uint32_t n_tiles, uint32_t cols,
                                                    uint64_t* __restrict__ totals) {
    __shared__ uint64_t tmp[256];
    for (uint32_t c = 0; c < cols; c++) {
        uint64_t run = 0;
        for (uint32_t b = 0; b < n_tiles; b += 256) {
            const uint32_t t = b + threadIdx.x;
            const uint64_t v = t < n_tiles ? tiles[(uint64_t)t * cols + c] : 0ull;
            uint64_t total;
            const uint64_t ex = block_excl_scan_u64(v, tmp, &total);
            if (t < n_tiles) tiles[(uint64_t)t * cols + c] = run + ex;
            run += total;
        }
        if (threadIdx.x == 0) totals[c] = run;
    }
}

__global__ __launch_bounds__(256) void k_scan64_offsets(const uint64_t* __restrict__ in, uint32_t n,
                                                        const uint64_t* __restrict__ tile_sums,
                                                        uint64_t* __restrict__ offsets) {
    __shared__ uint64_t tmp[256];
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + threadIdx.x * 4u;
    uint64_t v[4], s = 0;
    for (uint32_t k = 0; k < 4; k++) {
        v[k] = base + k < n ? in[base + k] : 0ull;
        s += v[k];
    }
    uint64_t total;
    uint64_t ex = block_excl_scan_u64(s, tmp, &total) + tile_sums[blockIdx.x];
    for (uint32_t k = 0; k < 4; k++) {
        if (base + k < n) offsets[base + k] = ex;
        ex += v[k];
        if (base + k + 1 == n) offsets[n] = ex;  // the end of the last value
    }
}

}  // namespace

hipError_t launch_scan64_sums(hipStream_t s, const uint64_t* in, uint32_t n, uint64_t* tile_sums, uint64_t* total) {
    const uint32_t tiles = scan64_tiles(n);
    k_scan64_tiles<<<tiles, 256, 0, s>>>(in, n, tile_sums);
    return launch_scan64_top(s, tile_sums, tiles, 1, total);
}

hipError_t launch_scan64_top(hipStream_t s, uint64_t* tiles, uint32_t n_tiles, uint32_t cols, uint64_t* totals) {
    k_scan64_top<<<1, 256, 0, s>>>(tiles, n_tiles, cols, totals);
    return hipGetLastError();
}

hipError_t launch_scan64_offsets(hipStream_t s, const uint64_t* in, uint32_t n, const uint64_t* tile_sums,
                                 uint64_t* offsets) {
    k_scan64_offsets<<<scan64_tiles(n), 256, 0, s>>>(in, n, tile_sums, offsets);
    return hipGetLastError();
}

}  // namespace gd
