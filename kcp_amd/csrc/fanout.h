// The per-cluster index of a pass's dirty IDs (include/gpudiff.h gpudiff_cluster_index): the packed
// block K25 writes and the host reads in one copy, and the same function on the host (gpudiff_cluster_index_host:
// host-only callers, the tests' second implementation, the measurements' baseline).  Plain C++, no HIP: the tests
// compile this header into a stand-alone program under the sanitizers.  Internal, not part of the ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace gd {

// One block of u32 words: cluster_ids[nc] | spec_off[nc + 1] | status_off[nc + 1] | spec_ids[ns] | status_ids[nt]
struct FanLayout {
    uint64_t cluster_ids, spec_off, status_off, spec_ids, status_ids, words;  // word offsets; words = the block's size
};

inline FanLayout fan_layout(uint64_t nc, uint64_t ns, uint64_t nt) {
    FanLayout l;
    l.cluster_ids = 0;
    l.spec_off = nc;
    l.status_off = l.spec_off + nc + 1;
    l.spec_ids = l.status_off + nc + 1;
    l.status_ids = l.spec_ids + ns;
    l.words = l.status_ids + nt;
    return l;
}

constexpr uint8_t kFanSpec = 0x1u, kFanStatus = 0x2u;  // GPUDIFF_SPEC_DIRTY / GPUDIFF_STATUS_DIRTY

// The index of n rows in batch order into `block` (laid out by the FanLayout returned); *nc / *ns / *nt its counts.
// The dirty positions ordered by (cluster, position): already so when the clusters ascend along them, otherwise one
// sort of (cluster << 32 | position) keys, which is that order.  n <= 0xFFFFFFFF.  Throws std::bad_alloc.
inline FanLayout fan_index_host(const uint8_t* flags, const uint32_t* pair_ids, const uint32_t* cluster_ids, size_t n,
                                std::vector<uint32_t>& block, uint64_t* nc, uint64_t* ns, uint64_t* nt) {
    std::vector<uint64_t> ord;  // cluster << 32 | position, of the dirty rows
    bool ascending = true;
    uint64_t n_spec = 0, n_status = 0;
    for (size_t i = 0; i < n; i++) {
        const uint8_t f = flags[i];
        if (!(f & (kFanSpec | kFanStatus))) continue;
        n_spec += (f & kFanSpec) ? 1u : 0u;
        n_status += (f & kFanStatus) ? 1u : 0u;
        const uint64_t k = ((uint64_t)cluster_ids[i] << 32) | (uint64_t)i;
        if (!ord.empty() && k < ord.back()) ascending = false;
        ord.push_back(k);
    }
    if (!ascending) std::sort(ord.begin(), ord.end());
    uint64_t n_cl = 0;
    for (size_t j = 0; j < ord.size(); j++)
        if (j == 0 || (ord[j] >> 32) != (ord[j - 1] >> 32)) n_cl++;
    const FanLayout l = fan_layout(n_cl, n_spec, n_status);
    block.assign(l.words, 0u);
    uint32_t* w = block.data();
    uint64_t h = 0, s = 0, t = 0;
    for (size_t j = 0; j < ord.size(); j++) {
        const uint32_t c = (uint32_t)(ord[j] >> 32), i = (uint32_t)ord[j];
        if (j == 0 || c != (uint32_t)(ord[j - 1] >> 32)) {
            w[l.cluster_ids + h] = c;
            w[l.spec_off + h] = (uint32_t)s;
            w[l.status_off + h] = (uint32_t)t;
            h++;
        }
        if (flags[i] & kFanSpec) w[l.spec_ids + s++] = pair_ids[i];
        if (flags[i] & kFanStatus) w[l.status_ids + t++] = pair_ids[i];
    }
    w[l.spec_off + n_cl] = (uint32_t)s;  // the closing offsets (an empty index has them too)
    w[l.status_off + n_cl] = (uint32_t)t;
    *nc = n_cl, *ns = n_spec, *nt = n_status;
    return l;
}

}  // namespace gd
