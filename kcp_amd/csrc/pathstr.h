// Rendering a path hash as text ("spec.containers[0].image") from one blob's
// path table (include/gpudiff_format.h): the one routine the host entry point
// (gpudiff_render_path_from_blob), the store's host resolution and kernels
// K15 / K16 (paths.hip) share.  Internal, not part of the ABI.
//
// The text is render_path's (encoder.cpp): a key is its raw decoded bytes,
// preceded by '.' only when the text rendered so far is non-empty; an index is
// "[%u]".  The walk goes from the node up to the root (the pair's seed), so the
// length pass counts the dots without knowing the prefixes -- a key gets its
// dot iff some component above it renders non-empty -- and the write pass
// fills the string right to left from its known end: after a key, the '.' goes
// in exactly when the cursor is still past the string's start.
//
// Nothing here trusts the table: a hash or a parent that is not found, a key
// outside the key area, a chain of more than kPathMaxSteps nodes (a parent
// cycle ends there) all end as "unresolved", which renders empty.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gpudiff_format.h"

namespace gd {

struct PathTab {
    const uint64_t* hs;   // [n] ascending, unique
    const uint64_t* phs;  // [n]
    const uint64_t* cs;   // [n]
    const uint8_t* keys;
    uint32_t n;
    uint64_t key_bytes;   // readable bytes at keys
};

constexpr uint32_t kPathMaxSteps = 256;
constexpr uint64_t kPathUnresolved = ~0ull;

// a table at `trailer` (a blob's body end) with `room` readable bytes; n = 0 when it does not fit
__host__ __device__ inline PathTab path_tab(const uint8_t* trailer, uint32_t n, uint64_t room) {
    PathTab t;
    if (n == GPUDIFF_TAB_NONE || 24ull * n > room) n = 0;
    t.hs = (const uint64_t*)trailer;
    t.phs = t.hs + n;
    t.cs = t.phs + n;
    t.keys = trailer + 24ull * n;
    t.n = n;
    t.key_bytes = n ? room - 24ull * n : 0;
    return t;
}

// index of h in hs[0, n), or n
__host__ __device__ inline uint32_t path_find(const uint64_t* hs, uint32_t n, uint64_t h) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (hs[mid] < h) lo = mid + 1;
        else hi = mid;
    }
    return (lo < n && hs[lo] == h) ? lo : n;
}

__host__ __device__ inline uint32_t path_digits(uint32_t v) {
    uint32_t d = 1;
    while (v >= 10u) {
        v /= 10u;
        d++;
    }
    return d;
}

// length of the path of `h` as text, or kPathUnresolved
__host__ __device__ inline uint64_t path_text_len(const PathTab& t, uint64_t root, uint64_t h) {
    uint32_t i = path_find(t.hs, t.n, h);
    uint64_t len = 0;
    uint32_t open = 0;  // keys below that wait for a non-empty component above them
    for (uint32_t step = 0; step < kPathMaxSteps; step++) {
        if (i >= t.n) return kPathUnresolved;
        const uint64_t c = t.cs[i];
        if (c & GPUDIFF_TAB_INDEX) {
            len += 2u + path_digits((uint32_t)c) + open;
            open = 0;
        } else {
            const uint32_t kl = (uint32_t)(c >> 32);
            if ((uint64_t)(uint32_t)c + kl > t.key_bytes) return kPathUnresolved;
            if (kl) {
                len += (uint64_t)kl + open;
                open = 0;
            }
            open++;
        }
        const uint64_t ph = t.phs[i];
        if (ph == root) return len;
        i = path_find(t.hs, t.n, ph);
    }
    return kPathUnresolved;
}

// writes the text into dst[0, len), len = path_text_len's answer for the same table.  Whatever len is,
// nothing outside dst[0, len) is touched; false (dst's contents undefined) when the walk fails or the
// text is longer than len or ends short of it -- a len that is too long can still pass with dots a
// correct length would not place, so the length must come from path_text_len
__host__ __device__ inline bool path_text_write(const PathTab& t, uint64_t root, uint64_t h, uint8_t* dst,
                                                uint64_t len) {
    uint32_t i = path_find(t.hs, t.n, h);
    uint64_t cur = len;
    for (uint32_t step = 0; step < kPathMaxSteps; step++) {
        if (i >= t.n) return false;
        const uint64_t c = t.cs[i];
        if (c & GPUDIFF_TAB_INDEX) {
            uint32_t v = (uint32_t)c;
            if (cur < 2ull + path_digits(v)) return false;
            dst[--cur] = ']';
            do {
                dst[--cur] = (uint8_t)('0' + v % 10u);
                v /= 10u;
            } while (v);
            dst[--cur] = '[';
        } else {
            const uint32_t kl = (uint32_t)(c >> 32);
            if ((uint64_t)(uint32_t)c + kl > t.key_bytes || kl > cur) return false;
            const uint8_t* k = t.keys + (uint32_t)c;
            cur -= kl;
            for (uint32_t q = 0; q < kl; q++) dst[cur + q] = k[q];
            if (cur) dst[--cur] = '.';
        }
        const uint64_t ph = t.phs[i];
        if (ph == root) return cur == 0;
        i = path_find(t.hs, t.n, ph);
    }
    return false;
}

}  // namespace gd
