// Changed paths as text (gfx950, wave64): GPUDIFF_OPT_PATH_STRINGS renders every (path hash, kind) a diffed
// device-encoded batch reports from the path tables its blobs carry in HBM (include/gpudiff_format.h), with
// the walk of pathstr.h -- the same routine the host entry point runs.
//
//   K15 k_path_len    wave per dirty pair, lanes striding over the pair's changed-path entries: the table
//                     by kind (CHANGED / ADDED: B's, REMOVED: A's; STATUS_ABSENT: the literal "status"), the
//                     string's length, a counter of unresolved entries
//   scan              exclusive u64 scan of the lengths (scan64.h: sums and total, then the offsets)
//   K16 k_path_write  the same mapping; each string into its slot, packed back to back, no terminator
//
// Both kernels chase dependent loads (a binary search per step up the tree): latency-bound.  One pair's
// lanes stay on one pair's tables, so their searches share the tables' top cache lines.  No LDS staging.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gpudiff.h"
#include "pathstr.h"
#include "scan64.h"
#include "tokenize.h"

namespace gd {

namespace {

// the table (and the root's hash) that renders entry kind `k` of row r; n = 0 when the side has none
// or it does not lie inside the space
__device__ __forceinline__ PathTab entry_tab(const PathJob& j, const gpudiff_pair_row& r, uint32_t row, uint32_t k) {
    const bool a = (k & 3u) == GPUDIFF_PATH_REMOVED;
    const uint64_t off = a ? r.off_a : r.off_b;
    const uint64_t body = a ? gpudiff_blob_body(r.spec_l_a, r.spec_ar_a, r.stat_l_a, r.stat_ar_a)
                            : gpudiff_blob_body(r.spec_l_b, r.spec_ar_b, r.stat_l_b, r.stat_ar_b);
    const uint32_t n = j.ntab[2ull * row + (a ? 0u : 1u)];
    if (off > j.space_bytes || body > j.space_bytes - off) return path_tab(j.space, 0, 0);
    return path_tab(j.space + off + body, n, j.space_bytes - off - body);
}

constexpr uint32_t kStatusLen = 6;  // "status": the sentinel's text

__global__ __launch_bounds__(256) void k_path_len(const PathJob j, uint64_t* __restrict__ lens,
                                                  unsigned long long* __restrict__ ctr) {
    const uint32_t lane = __lane_id();
    const uint32_t d = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (d >= j.n_dirty) return;
    const uint32_t e0 = j.path_off[d], e1 = min(j.path_off[d + 1], j.n_paths);
    if (e0 >= e1) return;
    const uint32_t row = j.dirty_idx[d];
    const gpudiff_pair_row r = j.rows[row];
    const uint64_t root = (uint64_t)((r.flags_b >> GPUDIFF_OBJ_SEED_SHIFT) & 0xFFu) & j.mask;
    uint32_t bad = 0;
    for (uint32_t e = e0 + lane; e < e1; e += 64) {
        const uint32_t k = j.out_k[e];
        uint64_t len = kStatusLen;
        if ((k & 3u) != GPUDIFF_PATH_STATUS_ABSENT) {
            len = path_text_len(entry_tab(j, r, row, k), root, j.out_h[e]);
            if (len == kPathUnresolved) {
                len = 0;
                bad++;
            }
        }
        lens[e] = len;
    }
    if (bad) atomicAdd(&ctr[1], (unsigned long long)bad);
}

__global__ __launch_bounds__(256) void k_path_write(const PathJob j, const uint64_t* __restrict__ offsets,
                                                    uint8_t* __restrict__ bytes, uint64_t bytes_cap,
                                                    unsigned long long* __restrict__ ctr) {
    const uint32_t lane = __lane_id();
    const uint32_t d = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (d >= j.n_dirty) return;
    const uint32_t e0 = j.path_off[d], e1 = min(j.path_off[d + 1], j.n_paths);
    if (e0 >= e1) return;
    const uint32_t row = j.dirty_idx[d];
    const gpudiff_pair_row r = j.rows[row];
    const uint64_t root = (uint64_t)((r.flags_b >> GPUDIFF_OBJ_SEED_SHIFT) & 0xFFu) & j.mask;
    uint32_t bad = 0;
    for (uint32_t e = e0 + lane; e < e1; e += 64) {
        const uint64_t o0 = offsets[e], o1 = offsets[e + 1];
        if (o1 < o0 || o1 > bytes_cap) {  // the slot does not lie inside the buffer: nothing is written
            bad++;
            continue;
        }
        const uint64_t len = o1 - o0;
        if (!len) continue;
        uint8_t* dst = bytes + o0;
        const uint32_t k = j.out_k[e];
        if ((k & 3u) == GPUDIFF_PATH_STATUS_ABSENT) {
            const char* s = "status";
            for (uint32_t q = 0; q < kStatusLen && q < len; q++) dst[q] = (uint8_t)s[q];
        } else if (!path_text_write(entry_tab(j, r, row, k), root, j.out_h[e], dst, len)) {
            for (uint64_t q = 0; q < len; q++) dst[q] = 0;
            bad++;
        }
    }
    if (bad) atomicAdd(&ctr[1], (unsigned long long)bad);
}

}  // namespace

hipError_t launch_path_len(hipStream_t s, const PathJob& j, uint64_t* lens, uint64_t* tile_sums,
                           unsigned long long* ctr) {
    hipError_t e = hipMemsetAsync(ctr, 0, 16, s);
    if (e != hipSuccess || !j.n_paths) return e;
    // an entry no dirty pair's range covers (none, by K6's CSR) would otherwise scan an unwritten length
    if ((e = hipMemsetAsync(lens, 0, 8ull * j.n_paths, s)) != hipSuccess) return e;
    k_path_len<<<(j.n_dirty + 3) / 4, 256, 0, s>>>(j, lens, ctr);
    return launch_scan64_sums(s, lens, j.n_paths, tile_sums, (uint64_t*)ctr);  // ctr[0] = the total
}

hipError_t launch_path_write(hipStream_t s, const PathJob& j, const uint64_t* lens, const uint64_t* tile_sums,
                             uint64_t* offsets, uint8_t* bytes, uint64_t bytes_cap, unsigned long long* ctr) {
    if (!j.n_paths) return hipMemsetAsync(offsets, 0, 8, s);
    const hipError_t e = launch_scan64_offsets(s, lens, j.n_paths, tile_sums, offsets);
    if (e != hipSuccess) return e;
    k_path_write<<<(j.n_dirty + 3) / 4, 256, 0, s>>>(j, offsets, bytes, bytes_cap, ctr);
    return hipGetLastError();
}

}  // namespace gd
