// The per-cluster index of a pass's dirty IDs on the device (gfx950, wave64; include/gpudiff.h
// gpudiff_cluster_index).  Over the pass's n_dirty dirty entries, never over all pairs:
//
//   K23 k_fan_keys    lane per dirty entry k: key[k] = its row's cluster id (a 4-byte gather from the 64-B rows),
//                     val[k] = k; a wave that sees a key below its predecessor's ORs kFanUnsorted into the control
//                     word with one atomic
//   sort              only when that word came back set: hipCUB's radix sort of (key, val) over all 32 bits.  It is
//                     stable and val ascends in batch order, which is the whole ordering rule
//   K24 k_fan_marks   block per tile of kScanTile entries of the (sorted) order, 4 a thread: heads (an entry whose key
//                     differs from its predecessor's, read across tile edges), spec and status bits of the entry's
//                     flags; the tile's three sums into interleaved columns, scanned by launch_scan64_top
//   K25 k_fan_emit    same tiling: the tile's prefixes again (block_excl_scan_u64 over the three counts packed into
//                     one word), then every head writes its cluster id and both offsets, every set bit its pair id,
//                     and the last entry the closing offsets, into one packed block (fanout.h FanLayout)
//
// Every dependency between the steps is a kernel boundary; plain stores; no LDS beyond the block scans.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "fanout_dev.h"
#include "scan64.h"

namespace gd {

namespace {

constexpr uint32_t kFanHead = 1u, kFanS = 2u, kFanT = 4u;  // an entry's marks
// the three counts of up to kScanTile entries in one u64, so one block scan serves all three
constexpr uint32_t kFanField = 20, kFanMask = (1u << kFanField) - 1u;
static_assert(kScanTile <= kFanMask, "a tile's count fits its field");

__global__ __launch_bounds__(256) void k_fan_keys(const gpudiff_pair_row* __restrict__ rows, uint32_t n_pairs,
                                                  const uint32_t* __restrict__ dirty_idx, uint32_t n,
                                                  uint32_t* __restrict__ key, uint32_t* __restrict__ val,
                                                  uint32_t* __restrict__ ctl) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    uint32_t bad = 0;
    if (k < n) {
        uint32_t r = dirty_idx[k];
        if (r >= n_pairs) bad |= kFanBadRow, r = 0;  // never read past the rows; the host refuses the index
        const uint32_t c = rows[r].cluster_id;
        key[k] = c;
        val[k] = k;
        if (k > 0) {
            uint32_t rp = dirty_idx[k - 1];
            if (rp >= n_pairs) rp = 0;  // its own lane reports it
            if (rows[rp].cluster_id > c) bad |= kFanUnsorted;
        }
    }
    // every lane arrives here: one atomic per wave that has something to report
    const uint32_t w = (__any((int)(bad & kFanUnsorted)) ? kFanUnsorted : 0u) | (__any((int)(bad & kFanBadRow)) ? kFanBadRow : 0u);
    if (w && (threadIdx.x & 63u) == 0) atomicOr(ctl, w);
}

// The thread's 4 consecutive entries of the order: keys, vals and marks (0 behind the end), and the packed counts
__device__ inline uint64_t fan_load4(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val,
                                     const uint32_t* __restrict__ dirty_idx, const uint8_t* __restrict__ flags,
                                     uint32_t n_pairs, uint32_t n, uint64_t base, uint32_t k[4], uint32_t v[4],
                                     uint32_t m[4]) {
    if (base + 3 < n) {  // base is a multiple of 4: 16-byte loads
        const uint4 kk = *(const uint4*)(key + base);
        const uint4 vv = *(const uint4*)(val + base);
        k[0] = kk.x, k[1] = kk.y, k[2] = kk.z, k[3] = kk.w;
        v[0] = vv.x, v[1] = vv.y, v[2] = vv.z, v[3] = vv.w;
    } else {
        for (uint32_t i = 0; i < 4; i++) {
            k[i] = base + i < n ? key[base + i] : 0u;
            v[i] = base + i < n ? val[base + i] : 0u;
        }
    }
    uint32_t prev = (base > 0 && base < n) ? key[base - 1] : 0u;  // across the tile's and the block's edge
    uint64_t cnt = 0;
    for (uint32_t i = 0; i < 4; i++) {
        m[i] = 0;
        if (base + i < n) {
            if (base + i == 0 || k[i] != prev) m[i] |= kFanHead;
            // a val or a row out of range leaves the entry unmarked: the totals then miss the pass's own counts
            const uint32_t r = v[i] < n ? dirty_idx[v[i]] : n_pairs;
            const uint32_t f = r < n_pairs ? flags[r] : 0u;
            if (f & GPUDIFF_SPEC_DIRTY) m[i] |= kFanS;
            if (f & GPUDIFF_STATUS_DIRTY) m[i] |= kFanT;
            prev = k[i];
        }
        cnt += (uint64_t)(m[i] & kFanHead) + ((uint64_t)((m[i] >> 1) & 1u) << kFanField) +
               ((uint64_t)((m[i] >> 2) & 1u) << (2 * kFanField));
    }
    return cnt;
}

__global__ __launch_bounds__(256) void k_fan_marks(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val,
                                                   const uint32_t* __restrict__ dirty_idx,
                                                   const uint8_t* __restrict__ flags, uint32_t n_pairs, uint32_t n,
                                                   uint64_t* __restrict__ tiles) {
    __shared__ uint64_t tmp[256];
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + threadIdx.x * 4u;
    uint32_t k[4], v[4], m[4];
    const uint64_t cnt = fan_load4(key, val, dirty_idx, flags, n_pairs, n, base, k, v, m);
    uint64_t total;
    (void)block_excl_scan_u64(cnt, tmp, &total);
    if (threadIdx.x == 0) {
        uint64_t* t = tiles + (uint64_t)blockIdx.x * kFanCols;
        t[0] = total & kFanMask;
        t[1] = (total >> kFanField) & kFanMask;
        t[2] = total >> (2 * kFanField);
    }
}

__global__ __launch_bounds__(256) void k_fan_emit(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val,
                                                  const uint32_t* __restrict__ dirty_idx,
                                                  const uint32_t* __restrict__ dirty_ids,
                                                  const uint8_t* __restrict__ flags, uint32_t n_pairs, uint32_t n,
                                                  const uint64_t* __restrict__ tiles, uint32_t nc, uint32_t ns,
                                                  uint32_t nt, FanLayout l, uint32_t* __restrict__ block) {
    __shared__ uint64_t tmp[256];
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + threadIdx.x * 4u;
    uint32_t k[4], v[4], m[4];
    const uint64_t cnt = fan_load4(key, val, dirty_idx, flags, n_pairs, n, base, k, v, m);
    uint64_t total;
    const uint64_t ex = block_excl_scan_u64(cnt, tmp, &total);
    const uint64_t* tb = tiles + (uint64_t)blockIdx.x * kFanCols;
    // ranks before this thread's first entry; every index below is checked against the counts the block was sized by
    uint64_t h = tb[0] + (ex & kFanMask);
    uint64_t s = tb[1] + ((ex >> kFanField) & kFanMask);
    uint64_t t = tb[2] + (ex >> (2 * kFanField));
    for (uint32_t i = 0; i < 4; i++) {
        if (base + i >= n) break;
        if (m[i] & kFanHead) {
            if (h < nc) {
                block[l.cluster_ids + h] = k[i];
                block[l.spec_off + h] = (uint32_t)s;
                block[l.status_off + h] = (uint32_t)t;
            }
            h++;
        }
        if (m[i] & (kFanS | kFanT)) {  // marked entries have v[i] < n
            const uint32_t id = dirty_ids[v[i]];
            if (m[i] & kFanS) {
                if (s < ns) block[l.spec_ids + s] = id;
                s++;
            }
            if (m[i] & kFanT) {
                if (t < nt) block[l.status_ids + t] = id;
                t++;
            }
        }
        if (base + i + 1 == n) {  // the closing offsets
            block[l.spec_off + nc] = (uint32_t)s;
            block[l.status_off + nc] = (uint32_t)t;
        }
    }
}

}  // namespace

hipError_t launch_fan_keys(hipStream_t s, const gpudiff_pair_row* rows, uint32_t n_pairs, const uint32_t* dirty_idx,
                           uint32_t n_dirty, uint32_t* key, uint32_t* val, uint32_t* ctl) {
    hipError_t e = hipMemsetAsync(ctl, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    k_fan_keys<<<(n_dirty + 255u) / 256u, 256, 0, s>>>(rows, n_pairs, dirty_idx, n_dirty, key, val, ctl);
    return hipGetLastError();
}

size_t fan_sort_temp_bytes(uint32_t n) {
    size_t b = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                             (const uint32_t*)nullptr, (uint32_t*)nullptr, n, 0, 32, (hipStream_t)0);
    return b;
}

hipError_t launch_fan_sort(hipStream_t s, void* temp, size_t temp_bytes, const uint32_t* key, uint32_t* key_out,
                           const uint32_t* val, uint32_t* val_out, uint32_t n) {
    return hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, key, key_out, val, val_out, n, 0, 32, s);
}

hipError_t launch_fan_marks(hipStream_t s, const uint32_t* key, const uint32_t* val, const uint32_t* dirty_idx,
                            const uint8_t* flags, uint32_t n_pairs, uint32_t n, uint64_t* tiles, uint64_t* totals) {
    const uint32_t n_tiles = scan64_tiles(n);
    k_fan_marks<<<n_tiles, 256, 0, s>>>(key, val, dirty_idx, flags, n_pairs, n, tiles);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_scan64_top(s, tiles, n_tiles, kFanCols, totals);
}

hipError_t launch_fan_emit(hipStream_t s, const uint32_t* key, const uint32_t* val, const uint32_t* dirty_idx,
                           const uint32_t* dirty_ids, const uint8_t* flags, uint32_t n_pairs, uint32_t n,
                           const uint64_t* tiles, uint32_t nc, uint32_t ns, uint32_t nt, uint32_t* block) {
    k_fan_emit<<<scan64_tiles(n), 256, 0, s>>>(key, val, dirty_idx, dirty_ids, flags, n_pairs, n, tiles, nc, ns, nt,
                                               fan_layout(nc, ns, nt), block);
    return hipGetLastError();
}

}  // namespace gd
