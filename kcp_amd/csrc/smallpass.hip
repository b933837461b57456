// K20 k_small_pass: a whole diff pass of at most GPUDIFF_SMALL_PASS_MAX_PAIRS pairs in one launch
// (GPUDIFF_OPT_SMALL_PASS), written for gfx950 (CDNA4, wave64).
//
//   phase A   one wave per pair: the pair's row and geometry as K2's decision block derives them, both objects'
//             compared chunks streamed against each other (16-B non-temporal loads, lane-strided), K2's flag byte,
//             and a dirty pair's changed paths merge-joined (join_pair, join_dev.h) into `cap` entries of the
//             batch's path arena, taken with one atomicAdd on a cursor
//   hand-off  every block releases its stores and adds to an arrival counter; the block that arrives last
//             acquires and finishes the pass.  Nobody polls: every other block has exited, so no wait can hang
//   phase B   the last block, 4 waves: per-chunk counts, a wave scan over the (at most 64) chunks, K3's compaction,
//             the path offsets, K6's path copy -- into the batch's device arrays as the ordinary pass leaves them,
//             and packed into the result image (small_pass.h) the host reads back in one copy
//
// The kernel declines to finish (image header: finalised = 0 and the reasons) when a dirty pair's paths do not fit
// the arena, a join covers more than kDeepJoin keys, or the pass has more than GPUDIFF_SMALL_PASS_MAX_PATHS paths;
// the host then runs the ordinary pass.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gpudiff.h"
#include "join_dev.h"
#include "kernels.h"
#include "small_pass.h"
#include "wave_dev.h"

namespace gd {

// words of the pass's summary block K20 uses for itself (zeroed with the block before every launch; the ordinary
// pass keeps its K2 item counters there)
constexpr uint32_t kSmCursor = 8, kSmArrive = 9, kSmGiveUp = 10;
static_assert(kSmGiveUp < kSummaryWords, "K20's words lie inside the zeroed summary block");
static_assert(GPUDIFF_SMALL_PASS_MAX_PAIRS == 64u * 64u, "the finishing block scans the chunks with one lane each");

struct SmallArgs {
    const gpudiff_pair_row* rows;
    const uint8_t* pool;
    const uint32_t* pair_ids;
    uint32_t n;
    uint32_t arena_cap;  // usable entries of arena_h / arena_k
    uint64_t mask;
    // written per pair by phase A, read by the finishing block: never through the scalar cache (no const
    // __restrict__ on anything another block wrote in this launch)
    uint8_t* flags;
    uint32_t* caps;
    uint32_t* path_src;
    uint32_t* path_cnt;
    uint8_t* nbits;
    uint64_t* arena_h;
    uint8_t* arena_k;
    uint32_t* summary;
    // written by the finishing block only
    uint32_t* spec_ids;
    uint32_t* status_ids;
    uint32_t* dirty_ids;
    uint32_t* dirty_idx;
    uint32_t* scratch_off;
    uint32_t* path_count;
    uint32_t* path_off;
    uint8_t* noop_d;
    uint64_t* out_h;
    uint8_t* out_k;
    uint8_t* image;
};

constexpr int kSmU = 4;  // 16-B chunk pairs in flight per lane

// Phase A for pair p.  The geometry and the flag rules must equal k_compare_flat's decision block (kernels.hip:
// "rows: lane k holds pair p0 + k" and "decisions"), the arena entries join_pair<true>'s.
__device__ __forceinline__ void small_pair(const SmallArgs& a, uint32_t p, uint32_t lane) {
    const gpudiff_pair_row r = a.rows[p];
    const bool err = ((r.flags_a | r.flags_b) & GPUDIFF_OBJ_DECODE_ERR) != 0u;
    const bool spec_sz = r.spec_l_a == r.spec_l_b && r.spec_ar_a == r.spec_ar_b;
    const bool has_st_b = (r.flags_b & GPUDIFF_OBJ_HAS_STATUS) != 0u;
    const bool stat_sz = has_st_b && r.stat_l_a == r.stat_l_b && r.stat_ar_a == r.stat_ar_b;
    const uint32_t seg_a = (uint32_t)seg_bytes(r.spec_l_a, r.spec_ar_a), seg_b = (uint32_t)seg_bytes(r.spec_l_b, r.spec_ar_b);
    const uint32_t seg_t = (uint32_t)seg_bytes(r.stat_l_a, r.stat_ar_a);
    // whole 128-B lines wherever both sides' spans are equal (K2's rule)
    const uint32_t r128 = (seg_a + seg_t + 127u) & ~127u;
    const bool no_stat = (r.stat_l_a | r.stat_l_b | r.stat_ar_a | r.stat_ar_b) == 0u;
    const uint32_t n1 = (!err && spec_sz) ? ((!stat_sz && no_stat) ? ((seg_a + 127u) & ~127u) : seg_a) >> 4 : 0u;
    const uint32_t n2 = (!err && stat_sz) ? (spec_sz ? r128 - seg_a : seg_t) >> 4 : 0u;
    const uint32_t tot = n1 + n2;
    // chunk k: spec chunk at off + 16k (k < n1), status chunk at off + seg + 16 (k - n1)
    const uint32_t adj_a = seg_a - 16u * n1, adj_b = seg_b - 16u * n1;
    bool mis_s = false, mis_t = false;  // a differing spec / status chunk (wave-uniform)
    for (uint32_t base = 0; base < tot; base += 64u * kSmU) {
        u32x4 va[kSmU], vb[kSmU];
        bool act[kSmU], st[kSmU];
#pragma unroll
        for (int u = 0; u < kSmU; u++) {
            const uint32_t g = base + (uint32_t)u * 64u + lane;
            act[u] = g < tot;
            st[u] = g >= n1;
            const uint64_t rel = 16ull * g;
            if (act[u]) {
                va[u] = __builtin_nontemporal_load((const u32x4*)(a.pool + r.off_a + rel + (st[u] ? adj_a : 0u)));
                vb[u] = __builtin_nontemporal_load((const u32x4*)(a.pool + r.off_b + rel + (st[u] ? adj_b : 0u)));
            }
        }
#pragma unroll
        for (int u = 0; u < kSmU; u++) {
            const bool ne = act[u] && neq16(va[u], vb[u]);
            if (ballot(ne && !st[u])) mis_s = true;
            if (ballot(ne && st[u])) mis_t = true;
        }
    }
    uint32_t f = 0, cap = 0;
    if (err) {
        f = F_SPEC | F_STATUS | F_ERR;
    } else {
        const bool spec_dirty = !spec_sz || mis_s;
        const bool stat_dirty = !stat_sz || mis_t;
        const bool stat_join = stat_dirty && (r.stat_l_a + r.stat_l_b) != 0u;
        f = (spec_dirty ? F_SPEC | F_JSPEC : 0u) | (stat_dirty ? F_STATUS : 0u) | (stat_join ? F_JSTAT : 0u) |
            (stat_dirty && !has_st_b ? F_SENT : 0u) | (((r.flags_a >> GPUDIFF_OBJ_SEED_SHIFT) & 0xFFu) ? F_SEED : 0u);
        cap = (spec_dirty ? r.spec_l_a + r.spec_l_b : 0u) +
              (stat_dirty ? r.stat_l_a + r.stat_l_b + (has_st_b ? 0u : 1u) : 0u);  // K2's mycap: an upper bound
    }
    const bool dirty = (f & (F_SPEC | F_STATUS)) != 0u;
    uint32_t src = 0, cnt = 0, nb = 0;
    if (dirty && !err) {
        uint32_t why = 0;
        if (cap > kDeepJoin) {
            why = kSmallDeep;  // the ordinary pass slices such a join over many waves
        } else {
            uint32_t base = 0;
            if (lane == 0)
                base = __hip_atomic_fetch_add(a.summary + kSmCursor, cap, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            base = uni(base);
            if (base > a.arena_cap || cap > a.arena_cap - base) {
                why = kSmallArena;
            } else {
                src = base;
                cnt = join_pair<true>(r, f, a.pool, a.mask, a.arena_h, a.arena_k, src, lane, &nb);
            }
        }
        if (why && lane == 0)
            __hip_atomic_fetch_or(a.summary + kSmGiveUp, why, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (lane == 0) {
        a.flags[p] = (uint8_t)f;
        if (dirty) {
            a.caps[p] = 0u;  // no K4 scratch slot
            a.path_src[p] = src;
            a.path_cnt[p] = cnt;
            a.nbits[p] = (uint8_t)nb;
        }
    }
}

// LDS words of the kernel's one __shared__ array
constexpr uint32_t kLdsLast = 0, kLdsReason = 1, kLdsTotals = 4, kLdsCnt = 8, kLdsBase = kLdsCnt + 4u * 64u,
                   kLdsWords = kLdsBase + 4u * 64u;

// Phase B: the whole block; every load of another block's bytes is a vector load behind the hand-off's acquire.
__device__ __forceinline__ void small_finish(const SmallArgs& a, uint32_t* lds) {
    const uint32_t lane = lane_id();
    const uint32_t wib = uni(threadIdx.x >> 6);
    const uint32_t n = a.n, nch = (n + 63u) >> 6;
    const uint64_t lt = mask_lt(lane);
    // per chunk: spec / status / dirty pairs and paths, recounted from the flags
    for (uint32_t c = wib; c < nch; c += 4u) {
        const uint32_t p = (c << 6) + lane;
        const uint32_t f = p < n ? (uint32_t)a.flags[p] : 0u;
        const bool dirty = (f & (F_SPEC | F_STATUS)) != 0u;
        const uint32_t pc = wave_sum(dirty ? a.path_cnt[p] : 0u);
        const uint32_t ns = popc64(ballot(f & F_SPEC)), nt = popc64(ballot(f & F_STATUS)), nd = popc64(ballot(dirty));
        if (lane == 0) {
            lds[kLdsCnt + 4u * c + 0u] = ns;
            lds[kLdsCnt + 4u * c + 1u] = nt;
            lds[kLdsCnt + 4u * c + 2u] = nd;
            lds[kLdsCnt + 4u * c + 3u] = pc;
        }
    }
    __syncthreads();
    if (wib == 0) {  // one lane per chunk: the chunk bases
        uint32_t v[4], inc[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            v[k] = lane < nch ? lds[kLdsCnt + 4u * lane + k] : 0u;
            inc[k] = wave_incl_scan(v[k]);
            lds[kLdsBase + 4u * lane + k] = inc[k] - v[k];
        }
        if (lane == 63) {
            const uint32_t gave = __hip_atomic_load(a.summary + kSmGiveUp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) lds[kLdsTotals + k] = inc[k];
            lds[kLdsReason] = gave | (inc[3] > GPUDIFF_SMALL_PASS_MAX_PATHS ? kSmallPaths : 0u);
        }
    }
    __syncthreads();
    const uint32_t n_spec = lds[kLdsTotals + 0u], n_status = lds[kLdsTotals + 1u], n_dirty = lds[kLdsTotals + 2u],
                   n_paths = lds[kLdsTotals + 3u], reason = lds[kLdsReason];
    const SmallLayout l = small_layout(n, n_spec, n_status, n_dirty, n_paths);
    if (threadIdx.x < kSmallHeaderWords) {
        const uint32_t t = threadIdx.x;
        const uint32_t h = t == SH_MAGIC    ? kSmallMagic
                           : t == SH_FINAL  ? (reason ? 0u : 1u)
                           : t == SH_REASON ? reason
                           : t == SH_PAIRS  ? n
                           : t == SH_SPEC   ? n_spec
                           : t == SH_STATUS ? n_status
                           : t == SH_DIRTY  ? n_dirty
                           : t == SH_PATHS  ? n_paths
                           : t == SH_BYTES  ? (reason ? 4u * kSmallHeaderWords : (uint32_t)l.total)
                                            : 0u;
        ((uint32_t*)a.image)[t] = h;
    }
    if (reason) return;  // the host runs the ordinary pass
    uint8_t* const i_flags = a.image + l.flags;
    uint32_t* const i_spec = (uint32_t*)(a.image + l.spec_ids);
    uint32_t* const i_status = (uint32_t*)(a.image + l.status_ids);
    uint32_t* const i_dirty = (uint32_t*)(a.image + l.dirty_ids);
    uint32_t* const i_idx = (uint32_t*)(a.image + l.dirty_idx);
    uint32_t* const i_off = (uint32_t*)(a.image + l.path_off);
    uint8_t* const i_noop = a.image + l.noop_d;
    uint8_t* const i_k = a.image + l.out_k;
    uint64_t* const i_h = (uint64_t*)(a.image + l.out_h);
    // K3's compaction (k_compact) chunk by chunk, the path offsets, K6's copy (k_copy_paths)
    for (uint32_t c = wib; c < nch; c += 4u) {
        const uint32_t p = (c << 6) + lane;
        const bool valid = p < n;
        const uint32_t f = valid ? (uint32_t)a.flags[p] : 0u;
        if (valid) i_flags[p] = (uint8_t)(f & (F_SPEC | F_STATUS | F_ERR));
        const uint64_t bs = ballot(f & F_SPEC), bt = ballot(f & F_STATUS), bd = ballot(f & (F_SPEC | F_STATUS));
        if (bd == 0) continue;
        const uint32_t b_spec = lds[kLdsBase + 4u * c + 0u], b_status = lds[kLdsBase + 4u * c + 1u],
                       b_dirty = lds[kLdsBase + 4u * c + 2u], b_paths = lds[kLdsBase + 4u * c + 3u];
        const bool dirty = (f & (F_SPEC | F_STATUS)) != 0u;
        const uint32_t id = dirty ? a.pair_ids[p] : 0u;
        if (f & F_SPEC) {
            const uint32_t q = b_spec + popc64(bs & lt);
            a.spec_ids[q] = id;
            i_spec[q] = id;
        }
        if (f & F_STATUS) {
            const uint32_t q = b_status + popc64(bt & lt);
            a.status_ids[q] = id;
            i_status[q] = id;
        }
        const uint32_t so = dirty ? a.path_src[p] : 0u;
        const uint32_t cnt = dirty ? a.path_cnt[p] : 0u;
        const uint32_t po = b_paths + wave_incl_scan(cnt) - cnt;
        if (dirty) {
            const uint32_t d = b_dirty + popc64(bd & lt);
            const uint8_t nb = a.nbits[p];
            a.dirty_ids[d] = id;
            a.dirty_idx[d] = p;
            a.scratch_off[d] = so | ARENA_BIT;
            a.path_count[d] = cnt;
            a.noop_d[d] = nb;
            a.path_off[d] = po;
            i_dirty[d] = id;
            i_idx[d] = p;
            i_noop[d] = nb;
            i_off[d] = po;
        }
        // lane per dirty pair for a few paths, the whole wave for many
        const bool big = cnt > 16u;
        if (!big)
            for (uint32_t i = 0; i < cnt; i++) {
                const uint64_t h = a.arena_h[so + i];
                const uint8_t k = a.arena_k[so + i];
                a.out_h[po + i] = h;
                a.out_k[po + i] = k;
                i_h[po + i] = h;
                i_k[po + i] = k;
            }
        for (uint64_t m = ballot(big); m; m &= m - 1) {
            const uint32_t k = (uint32_t)__builtin_ctzll(m);
            const uint32_t sok = uni(shfl32(so, k)), pok = uni(shfl32(po, k)), ck = uni(shfl32(cnt, k));
            for (uint32_t i = lane; i < ck; i += 64u) {
                const uint64_t h = a.arena_h[sok + i];
                const uint8_t kk = a.arena_k[sok + i];
                a.out_h[pok + i] = h;
                a.out_k[pok + i] = kk;
                i_h[pok + i] = h;
                i_k[pok + i] = kk;
            }
        }
    }
    if (threadIdx.x == 0) {
        a.path_off[n_dirty] = n_paths;
        i_off[n_dirty] = n_paths;
        a.summary[0] = n_spec;
        a.summary[1] = n_status;
        a.summary[2] = n_dirty;
        a.summary[5] = n_paths;
    }
}

__global__ __launch_bounds__(256) void k_small_pass(const SmallArgs a) {
    __shared__ uint32_t lds[kLdsWords];
    const uint32_t lane = lane_id();
    const uint32_t p = blockIdx.x * 4u + uni(threadIdx.x >> 6);
    if (p < a.n) small_pair(a, p, lane);
    // the hand-off, counter form: every wave drains its stores, the block meets, one lane releases at agent scope,
    // waits again, then adds to the arrival counter (this order: the fence before the add, the wait between them)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t t =
            __hip_atomic_fetch_add(a.summary + kSmArrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = t == gridDim.x - 1u;
        if (last) {  // every other block's stores are released: acquire once for the whole block
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        lds[kLdsLast] = last ? 1u : 0u;
    }
    __syncthreads();
    if (lds[kLdsLast] == 0u) return;  // nobody waits for anybody
    small_finish(a, lds);
}

hipError_t launch_small_pass(hipStream_t s, const DiffBuffers& b, uint64_t arena_cap, uint8_t* image) {
    if (b.n_pairs == 0 || b.n_pairs > GPUDIFF_SMALL_PASS_MAX_PAIRS || !image) return hipErrorInvalidValue;
    // the summary block (the counts, K20's cursor, arrival counter and give-up word) zeroed before every launch
    hipError_t e = hipMemsetAsync(b.summary, 0, kSummaryWords * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    SmallArgs a;
    a.rows = b.rows;
    a.pool = b.pool;
    a.pair_ids = b.pair_ids;
    a.n = b.n_pairs;
    a.arena_cap = (uint32_t)(arena_cap < 0xFFFFFFFFull ? arena_cap : 0xFFFFFFFFull);
    a.mask = b.hash_mask;
    a.flags = b.flags;
    a.caps = b.caps;
    a.path_src = b.path_src;
    a.path_cnt = b.path_cnt;
    a.nbits = b.nbits;
    a.arena_h = b.arena_h;
    a.arena_k = b.arena_k;
    a.summary = b.summary;
    a.spec_ids = b.spec_ids;
    a.status_ids = b.status_ids;
    a.dirty_ids = b.dirty_ids;
    a.dirty_idx = b.dirty_idx;
    a.scratch_off = b.scratch_off;
    a.path_count = b.path_count;
    a.path_off = b.path_off;
    a.noop_d = b.noop_d;
    a.out_h = b.out_h;
    a.out_k = b.out_k;
    a.image = image;
    k_small_pass<<<(b.n_pairs + 3u) / 4u, 256, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace gd
