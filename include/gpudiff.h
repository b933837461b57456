/*
 * gpudiff.h -- C ABI of the MI355X batched reconciliation-diff engine.
 *
 * Drop-in boundary for kcp's syncer change detection.  Each entry point names
 * the reference interface (paths relative to the sttts/kcp tree) it replaces;
 * INTEGRATION.md shows the cgo binding a maintainer adds to pkg/syncer.
 *
 *   reference seam                                   replaced by
 *   ------------------------------------------------ ---------------------------
 *   deepEqualApartFromStatus  specsyncer.go:17-41    gpudiff_spec_equal (1 pair),
 *                                                    spec bits of gpudiff_wait
 *   deepEqualStatus           statussyncer.go:15-27  gpudiff_status_equal (1 pair),
 *                                                    status bits of gpudiff_wait
 *   UpdateFunc gates          specsyncer.go:47-51,   gpudiff_submit/gpudiff_wait:
 *                             statussyncer.go:32-36  dirty IDs -> AddToQueue
 *   Controller.AddToQueue     syncer.go:222-224      consumer of dirty_ids
 *
 * Conventions: 0 = OK, negative = error (gpudiff_strerror).  No exceptions or
 * longjmp cross the ABI.  The caller owns inputs until the call that reads
 * them returns (gpudiff_encode_pairs copies everything it needs).  The library
 * owns result buffers until gpudiff_result_release.  A context is not
 * reentrant: one submitting thread per context (the Go shim's batcher
 * goroutine).  Errors are conservative, as in the reference
 * (specsyncer.go:20-22): a pair that cannot be decoded is reported dirty in
 * both regions with GPUDIFF_DECODE_ERROR set, never "equal".
 *
 * There is no CPU fallback for the diff: device entry points on a context
 * without a GPU return GPUDIFF_E_NODEVICE.
 */
#ifndef GPUDIFF_H
#define GPUDIFF_H

#include <stddef.h>
#include <stdint.h>

#include "gpudiff_format.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPUDIFF_ABI_VERSION 6  /* 6: bit 0x100 (the K2 timeline build) retired: gpudiff_k2_profile selects that build;
                                   5: the tuning option bits removed (GPUDIFF_OPT_KNOWN); result slots own their counts */

enum {
    GPUDIFF_OK = 0,
    GPUDIFF_E_INVAL = -1,     /* bad argument */
    GPUDIFF_E_NOMEM = -2,     /* host allocation failed */
    GPUDIFF_E_DEVICE = -3,    /* HIP runtime error */
    GPUDIFF_E_NODEVICE = -4,  /* context has no GPU */
    GPUDIFF_E_CAPACITY = -5,  /* device batch capacity exceeded */
    GPUDIFF_E_STATE = -6,     /* call order violated (e.g. wait on unknown ticket) */
    GPUDIFF_E_DECODE = -7,    /* single-pair helpers: an input failed to decode */
    GPUDIFF_E_NOTFOUND = -8,  /* gpudiff_resolve_path: hash not in either object */
};

/* per-pair result flags */
#define GPUDIFF_SPEC_DIRTY 0x1u
#define GPUDIFF_STATUS_DIRTY 0x2u
#define GPUDIFF_DECODE_ERROR 0x4u
/* write-path hints, set only on dirty pairs: the write the
 * syncer issues for the decision would not change what the predicate compares, so the API call can
 * be skipped.  GPUDIFF_SPEC_NOOP: every changed spec leaf is an int64 v on one side and a float64
 * == v (|v| <= 2^53) on the other -- Go's json.Marshal writes both as the same digits and the API
 * server decodes them back to int64 v, so the two documents' bodies agree on the wire in that
 * region (gpudiff_write_plan_get_ex says what that means for informer and for (A, B) pairs).
 * GPUDIFF_STATUS_NOOP: the same for the status leaves, and when B has no status key, A has none
 * either (UpdateStatus would write nothing). */
#define GPUDIFF_SPEC_NOOP 0x8u
#define GPUDIFF_STATUS_NOOP 0x10u

/* device encoder (K0) per-object status: 0 = encoded on the device; otherwise
 * the reason the object was handed to the host encoder (the Go-exact path) */
#define GPUDIFF_TOK_OK 0
#define GPUDIFF_TOK_SYNTAX 1  /* not in the device's JSON subset: the host decides (usually a Go decode error) */
#define GPUDIFF_TOK_NUMBER 2  /* number outside the exact fast path (float needing full strtod, int64 overflow) */
#define GPUDIFF_TOK_KEY 3     /* object key that needs unescaping or UTF-8 repair */
#define GPUDIFF_TOK_STRING 4  /* control character or invalid escape in a string */
#define GPUDIFF_TOK_HASH 5    /* equal path hashes: duplicate key, or a collision under the seed */
#define GPUDIFF_TOK_DEPTH 6   /* nesting deeper than 255 */
#define GPUDIFF_TOK_SIZE 7    /* document larger than 16 MiB */
#define GPUDIFF_TOK_SPACE 8   /* output space exhausted */
#define GPUDIFF_TOK_FLOAT 9   /* K10 (write path): a float64 value (Go's shortest formatting is done on the host) */
#define GPUDIFF_TOK_WIDE 10   /* K10: an object with more than 2048 members (quadratic key ranking) */
#define GPUDIFF_TOK_FIELD 11  /* K11 (roll-up): a field the typed decode must judge on the host (duplicate,
                                 case-folded key, type mismatch, counter not an int32 literal, escaped label) */
#define GPUDIFF_TOK_LIST 12   /* K0: a top-level key the informer decoder's list probe matches ("items" under
                                 Go's case folding): the host decides (the object is an UnstructuredList, the
                                 pair is dirty -- specsyncer.go:18-22) */

/* changed-path kinds (low 2 bits); bit 7 = status region */
#define GPUDIFF_PATH_CHANGED 0u        /* present in both, value differs */
#define GPUDIFF_PATH_ADDED 1u          /* only in new (B) */
#define GPUDIFF_PATH_REMOVED 2u        /* only in old (A) */
#define GPUDIFF_PATH_STATUS_ABSENT 3u  /* new has no "status" key (statussyncer.go:22-26) */
#define GPUDIFF_PATH_REGION_STATUS 0x80u

/* context option flags (any other bit: gpudiff_open returns GPUDIFF_E_INVAL).  Round 5 removed the A/B tuning
 * bits of earlier rounds whose measurements rejected them (DESIGN.md §5-§6 keep the numbers):
 * 0x2 two upload streams, 0x4 index-order final round, 0x8 pipelined K4 join, 0x10-0x80 tail shapes (0x40 has a new meaning below), bits 9-20
 * kernel variants / blocks per CU / segmented passes, bits 26-31 K0 occupancy, items per wave, deep-join bounds.
 * ABI 6 retired 0x100 (ABI 5's K2 timeline bit, ABI 4's K2 variant bit): refused like the rest, so no caller of
 * either meaning gets the other; the timeline build is selected by gpudiff_k2_profile. */
#define GPUDIFF_OPT_TIMING 0x1u          /* record per-kernel HIP event times (gpudiff_last_timings) */
#define GPUDIFF_OPT_K2_ROWS 0x40u        /* diagnostic (the A/B, the tests): K2 reads the 64-B rows although the
                                            batch's 16-B pair descriptors are current; results do not change */
#define GPUDIFF_OPT_NO_IMAGE 0x20u       /* honoured at gpudiff_dbatch_append: the appended pairs get no compare image
                                            (below) and their ordinary descriptors; results do not change.  The
                                            in-build A/B reference beside GPUDIFF_OPT_K2_ROWS */
#define GPUDIFF_OPT_ARENA_SHIFT 21u      /* 4 bits, test hook: shrink the per-wave path arena 2^k-fold (forces
                                            pairs through the deferred K4 path) */
#define GPUDIFF_OPT_DEVICE_ENCODE 0x2000000u /* gpudiff_submit / single-pair helpers: raw JSON up, kernel K0
                                                encodes (as GPUDIFF_STORE_DEVICE_ENCODE does for the store) */
#define GPUDIFF_OPT_PATH_STRINGS 0x8000000u  /* device-encoded batches (gpudiff_submit with GPUDIFF_OPT_DEVICE_ENCODE,
                                                gpudiff_store_submit on a GPUDIFF_STORE_DEVICE_ENCODE store): kernels
                                                K15 / K16 render every changed path as text inside gpudiff_wait
                                                (gpudiff_result_path_strings) */
#define GPUDIFF_OPT_SMALL_PASS 0x20000000u   /* a diff pass of 1..GPUDIFF_SMALL_PASS_MAX_PAIRS pairs runs as ONE kernel
                                                (K20: decision, joins, compaction and path copy fused) and comes back
                                                in one read-back; results are those of the ordinary pass, byte for
                                                byte (gpudiff_pass_stats_get) */
#define GPUDIFF_OPT_PATH_VALUES 0x80000000u   /* the scope of GPUDIFF_OPT_PATH_STRINGS, and independent of it: kernels
                                                K21 / K22 render every changed leaf's old and new value as JSON text
                                                inside gpudiff_wait (gpudiff_result_path_values) */
#define GPUDIFF_OPT_KNOWN                                                                                         \
    (GPUDIFF_OPT_TIMING | (0xFu << GPUDIFF_OPT_ARENA_SHIFT) | GPUDIFF_OPT_DEVICE_ENCODE | GPUDIFF_OPT_PATH_STRINGS | \
     GPUDIFF_OPT_SMALL_PASS | GPUDIFF_OPT_PATH_VALUES | GPUDIFF_OPT_K2_ROWS | GPUDIFF_OPT_NO_IMAGE)

/* GPUDIFF_OPT_SMALL_PASS: the largest pass the fused kernel takes (64 chunks of 64 pairs: its finishing block scans
 * the chunks with one lane each), and the most changed paths it finishes itself -- a pass with more is run again as
 * the ordinary pass inside gpudiff_wait (gpudiff_pass_stats.redo_paths) */
#define GPUDIFF_SMALL_PASS_MAX_PAIRS 4096u
#define GPUDIFF_SMALL_PASS_MAX_PATHS 32768u

#define GPUDIFF_DEVICE_CURRENT (-1)
#define GPUDIFF_DEVICE_NONE (-2)   /* host-only context: encoding only */

typedef struct gpudiff_opts {
    int32_t device;          /* HIP ordinal, GPUDIFF_DEVICE_CURRENT or GPUDIFF_DEVICE_NONE */
    uint32_t encode_threads; /* 0 = all host cores */
    void* stream;            /* hipStream_t to launch on; NULL = context-owned stream */
    uint32_t flags;          /* GPUDIFF_OPT_* */
    uint32_t path_hash_bits; /* 0 (or >= 32): GPUDIFF_PATH_HASH_BITS = 32; 8..31 only to force collisions in tests */
} gpudiff_opts;

typedef struct gpudiff_json_pair {
    const uint8_t* old_json;  /* A: upstream (kcp) copy / old version */
    size_t old_len;
    const uint8_t* new_json;  /* B: downstream copy / new version */
    size_t new_len;
    uint32_t pair_id;         /* echoed in results */
    uint32_t cluster_id;      /* logical cluster (shard key, syncer.go:106-108) */
} gpudiff_json_pair;

typedef struct gpudiff_ctx gpudiff_ctx;
typedef struct gpudiff_hbatch gpudiff_hbatch;  /* encoded pairs in host memory */
typedef struct gpudiff_dbatch gpudiff_dbatch;  /* encoded pairs resident in HBM */
typedef uint64_t gpudiff_ticket;

typedef struct gpudiff_hbatch_info {
    size_t n_pairs;
    const gpudiff_pair_row* rows;   /* offsets relative to pool */
    const uint8_t* pool;
    uint64_t pool_bytes;
    uint64_t total_leaves;          /* over both objects of every pair */
    uint64_t n_decode_errors;
    uint64_t n_reseeded;            /* pairs whose path hash needed seed > 0 */
} gpudiff_hbatch_info;

typedef struct gpudiff_result {
    size_t n_pairs;
    const uint8_t* pair_flags;          /* [n_pairs], batch order, GPUDIFF_*_DIRTY */
    size_t n_spec_dirty;
    const uint32_t* spec_dirty_ids;     /* pair_id, batch order */
    size_t n_status_dirty;
    const uint32_t* status_dirty_ids;
    size_t n_dirty;                     /* spec or status dirty */
    const uint32_t* dirty_ids;
    const uint32_t* path_offsets;       /* [n_dirty + 1] into the path arrays */
    size_t n_paths;
    const uint64_t* path_hashes;        /* per dirty pair: spec asc, status asc, sentinel */
    const uint8_t* path_kinds;
    void* internal_;
} gpudiff_result;

/* ---- changed paths as text (GPUDIFF_OPT_PATH_STRINGS) ----
 * The batch's changed paths rendered from the path tables its blobs carry in HBM (gpudiff_format.h): string i
 * belongs to path_hashes[i] / path_kinds[i].  A key is its raw decoded bytes (any byte, NUL included), preceded by
 * '.' only when the text before it is non-empty; an index is "[%u]"; the GPUDIFF_PATH_STATUS_ABSENT sentinel is
 * "status" -- the text gpudiff_resolve_path gives, without decoding a document again.  Pairs the host resolved
 * (K0's deferrals) get their strings from the host encoder's flattened objects: n_host counts those entries.
 * n_unresolved counts entries whose table walk failed (rendered empty): always 0 for tables the engine wrote.
 * The arrays belong to the result (valid until gpudiff_result_release).
 * GPUDIFF_E_STATE: the option was off, the batch was encoded on the host (gpudiff_submit without
 * GPUDIFF_OPT_DEVICE_ENCODE or after its GPUDIFF_E_CAPACITY fallback: gpudiff_resolve_path serves those), or the
 * store is not a GPUDIFF_STORE_DEVICE_ENCODE one. */
typedef struct gpudiff_path_strings {
    size_t n_paths;            /* == result.n_paths, same order as path_hashes / path_kinds */
    const uint64_t* offsets;   /* n_paths + 1 */
    const char* bytes;         /* string i = bytes[offsets[i], offsets[i+1]) -- raw key bytes, no terminator */
    size_t n_host;             /* entries rendered by the host path */
    size_t n_unresolved;       /* must be 0; such entries are empty */
} gpudiff_path_strings;
int gpudiff_result_path_strings(gpudiff_ctx* ctx, const gpudiff_result* res, gpudiff_path_strings* out);
/* what the context has rendered so far; kernel_ms needs GPUDIFF_OPT_TIMING (HIP events around K15 + scan and
 * around the offsets + K16, summed over timed_batches) */
typedef struct gpudiff_path_stats {
    uint64_t batches;        /* waited batches with the option on */
    uint64_t paths;          /* strings, the host-rendered ones included */
    uint64_t bytes;
    uint64_t host_paths;
    double kernel_ms;
    uint64_t timed_batches;
} gpudiff_path_stats;
int gpudiff_path_strings_stats_get(gpudiff_ctx* ctx, gpudiff_path_stats* out);

/* ---- changed leaves' values as text (GPUDIFF_OPT_PATH_VALUES) ----
 * For entry i of the batch's changed paths (path_hashes[i] / path_kinds[i]) two values, old (A's leaf) and new (B's
 * leaf), rendered from the segments the blobs carry in HBM (gpudiff_format.h):
 *
 *   GPUDIFF_PATH_CHANGED         old = A's leaf   new = B's leaf
 *   GPUDIFF_PATH_ADDED           old absent       new = B's leaf
 *   GPUDIFF_PATH_REMOVED         old = A's leaf   new absent
 *   GPUDIFF_PATH_STATUS_ABSENT   both absent
 *
 * A present value is a type tag (GPUDIFF_TAG_*, gpudiff_format.h) and a text, never empty: the bytes the write
 * path's encoder (json.NewEncoder(w).Encode) puts on the wire for the leaf, rendered from the canonical value the
 * blob stores -- null / false / true / {} / [], int64 digits, Go's shortest float64 form (a negative zero is stored
 * as +0 and renders "0"), a string as '"' + HTML-safe escaping + '"'.  3 -> 3.0 is a CHANGED entry whose two texts
 * are both "3" and whose tags differ (INT, FLOAT).  An absent value has tag GPUDIFF_VALUE_ABSENT and an empty text.
 * Pairs the host resolved (K0's deferrals) get their values from the resolution batch's blobs, by the same kernels:
 * n_host counts those entries.  n_unresolved counts values whose leaf was not found or whose segment did not check
 * out (rendered ABSENT / empty): always 0 for blobs the engine wrote.
 * The arrays belong to the result (valid until gpudiff_result_release).
 * GPUDIFF_E_STATE: exactly the cases of gpudiff_result_path_strings. */
#define GPUDIFF_VALUE_ABSENT 0xFFu
typedef struct gpudiff_path_values {
    size_t n_paths;            /* == result.n_paths */
    const uint64_t* offsets;   /* 2 * n_paths + 1: text 2i = old of entry i, 2i + 1 = new */
    const char* bytes;         /* packed, no terminators */
    const uint8_t* tags;       /* 2 * n_paths: GPUDIFF_TAG_* or GPUDIFF_VALUE_ABSENT */
    size_t n_host;             /* entries whose pair the host resolved */
    size_t n_unresolved;       /* must be 0; such values are ABSENT / empty */
} gpudiff_path_values;
int gpudiff_result_path_values(gpudiff_ctx* ctx, const gpudiff_result* res, gpudiff_path_values* out);
/* gpudiff_path_stats counted for the values: paths = entries, bytes = the texts' bytes, host_paths = n_host summed;
 * kernel_ms (GPUDIFF_OPT_TIMING): HIP events around K21 + scan and around the offsets + K22 */
int gpudiff_path_values_stats_get(gpudiff_ctx* ctx, gpudiff_path_stats* out);
/* stream synchronisations the context's finishers spent on rendering text (strings and values together): with both
 * options on, one batch's two sizing read-backs are one 16-byte copy and one synchronisation */
int gpudiff_render_syncs_get(gpudiff_ctx* ctx, uint64_t* out);

/* device-side view of a diffed batch (for RCCL gathers; pointers are HBM).  The pointers belong to the batch's
 * current result slot: after gpudiff_dbatch_result_slot switches slots, fetch the view again (counts included --
 * a slot owns its counts since ABI 5). */
typedef struct gpudiff_device_view {
    const uint8_t* pair_flags;
    const uint32_t* spec_dirty_ids;
    const uint32_t* status_dirty_ids;
    const uint32_t* dirty_ids;
    const uint32_t* counts;   /* [0]=n_spec [1]=n_status [2]=n_dirty [3]=n_paths [4]=overflow */
} gpudiff_device_view;

typedef struct gpudiff_batch_stats {
    uint64_t n_pairs;
    uint64_t pool_bytes;       /* bytes of object blobs resident */
    uint64_t total_leaves;
    uint64_t compare_bytes;    /* format bytes one diff pass reads */
    uint64_t value_bytes;      /* canonical bytes of the long (non-inline) string values of every object:
                                  V of SURVEY.md §8(d)'s B_pair = sum over A, B of (24 L + V + 8) + O */
} gpudiff_batch_stats;

typedef struct gpudiff_timings {
    float compare_ms;     /* K2: all k2_launches launches of a pass (back to back on the stream) */
    float compact_ms;     /* K3 (scan + compaction); 0 when overlapped with K2 (segmented pass) */
    float join_ms;        /* K4 merge-join; segmented pass: the part not hidden behind K2 */
    float emit_ms;        /* K5 + K6 path scan and copy */
    float total_ms;       /* first to last event of gpudiff_diff */
    uint32_t n_passes;    /* diff passes averaged (since gpudiff_timing_reset) */
    uint32_t k2_launches; /* K2 launches per pass (batch segments) */
} gpudiff_timings;

/* ---- library ---- */
const char* gpudiff_strerror(int err);
int gpudiff_abi_version(void);
/* 16 hex digits: SHA-256 over the contents of every source, header, map and build script the library was
 * compiled from (kcp_amd/buildinfo.py).  A binding that ships the sources recomputes it and refuses a
 * library built from anything else; the bench line carries it as `build_id`. */
const char* gpudiff_build_id(void);
int gpudiff_device_count(int* n);

/* ---- context ---- */
int gpudiff_open(const gpudiff_opts* opts, gpudiff_ctx** out);
void gpudiff_close(gpudiff_ctx* ctx);

/* ---- host encoding (canonical CSR, no GPU needed) ---- */
int gpudiff_encode_pairs(gpudiff_ctx* ctx, const gpudiff_json_pair* pairs, size_t n,
                         gpudiff_hbatch** out);
int gpudiff_hbatch_info_get(const gpudiff_hbatch* hb, gpudiff_hbatch_info* info);
/* empty host batch (pinned on a GPU context) for pairs encoded elsewhere in the
 * canonical format (pre-encoded replays, synthetic populations); the caller
 * fills *pool and *rows (row offsets relative to *pool) before appending.
 * The decision kernel trusts a row's structural fields as it always trusted the sizes: a row whose flags_b carries
 * GPUDIFF_OBJ_SPEC_KEYS_EQ (gpudiff_format.h) states that both sides' spec keys[] are equal, and the whole 128-byte
 * lines holding only those keys are then not read or compared; with GPUDIFF_OBJ_SPEC_SHAPE_EQ beside it the row states
 * the same of both sides' spec metas[], and the lines holding only keys and metas are not read.  A caller that cannot
 * vouch for a bit leaves it 0.  A row that carries both bits (and no decode error) is streamed from the batch's compare
 * image (gpudiff_dbatch_set_image_capacity), which holds none of its spec keys or metas; with
 * GPUDIFF_OBJ_STAT_SHAPE_EQ beside them none of its status keys or metas either. */
int gpudiff_hbatch_create(gpudiff_ctx* ctx, uint64_t pool_bytes, size_t n_pairs, uint64_t total_leaves,
                          gpudiff_hbatch** out, uint8_t** pool, gpudiff_pair_row** rows);
/* reuses a host batch (staging ring): waits for its last H2D copy, grows the
 * buffers only when needed, and returns them for refilling */
int gpudiff_hbatch_resize(gpudiff_ctx* ctx, gpudiff_hbatch* hb, uint64_t pool_bytes, size_t n_pairs,
                          uint64_t total_leaves, uint8_t** pool, gpudiff_pair_row** rows);
void gpudiff_hbatch_free(gpudiff_ctx* ctx, gpudiff_hbatch* hb);

/* ---- device batches ---- */
int gpudiff_dbatch_create(gpudiff_ctx* ctx, uint64_t pool_bytes, uint64_t max_pairs,
                          gpudiff_dbatch** out);
/* A view of `base`: a batch with its own per-pass outputs (flags, lists, path arenas, scratch, counts) over
 * base's resident pairs (pool, rows and pair IDs are base's; appends to base are seen by later diffs of
 * the view; append / reset on a view are GPUDIFF_E_INVAL).  With a second context (its own stream) it lets
 * two diff passes over one population be in flight at once -- pass s + 1's decision kernel fills the CUs
 * pass s's tail frees, and pass s's compaction, joins and collective run beside it.  Same device as base;
 * the caller orders base's appends before the view's diffs (e.g. gpudiff_sync on base's context).  Free
 * views before their base. */
int gpudiff_dbatch_create_view(gpudiff_ctx* ctx, const gpudiff_dbatch* base, gpudiff_dbatch** out);
/* async H2D of hb into the batch (rows rebased onto the batch's pool) */
int gpudiff_dbatch_append(gpudiff_ctx* ctx, gpudiff_dbatch* db, const gpudiff_hbatch* hb);
int gpudiff_dbatch_reset(gpudiff_ctx* ctx, gpudiff_dbatch* db);
/* The compare image: a second device allocation per batch, made by its first append, into which every append also
 * writes a compacted copy of what the decision kernel must compare of each shape-equal pair (gpudiff_format.h,
 * gpudiff_pair_image_parts): the values and the string tails, without the keys and metas the encoder has proved
 * equal.  The decision kernel streams such a pair from the image; everything else (joins, exports, the pool, the
 * rows) is unchanged.  Its capacity defaults to the pool's (an image is never larger than its blobs); when it is
 * full, or cannot be allocated, the remaining pairs are streamed from the pool as before -- an append never fails
 * for the image.  gpudiff_dbatch_set_image_capacity sets the capacity in bytes before the batch's first append
 * (GPUDIFF_E_STATE after it, GPUDIFF_E_INVAL on a view); 0: no image.  The ring batches behind gpudiff_submit are
 * diffed once and have none. */
int gpudiff_dbatch_set_image_capacity(gpudiff_dbatch* db, uint64_t bytes);
typedef struct gpudiff_image_stats {
    uint64_t bytes_used; /* image bytes written (both sides of every imaged pair) */
    uint64_t capacity;   /* bytes allocated; 0: no image (none wanted, not yet appended, or the allocation failed) */
    uint64_t pairs;      /* resident pairs streamed from the image */
} gpudiff_image_stats;
int gpudiff_dbatch_image_stats(const gpudiff_dbatch* db, gpudiff_image_stats* st);
/* *out = the bytes the decision kernel streams for the batch's imaged pairs in one pass: each one's 16-B descriptor and
 * both sides' chunks of its packed parts, padded to the line as streamed.  Summed on the device by the appends' builder
 * kernel; the call waits for the last append's builder kernel, whichever context is given (a view's will do), and reads
 * the sum back.  0 with no image. */
int gpudiff_dbatch_image_streamed_bytes(gpudiff_ctx* ctx, const gpudiff_dbatch* db, uint64_t* out);
int gpudiff_dbatch_stats_get(const gpudiff_dbatch* db, gpudiff_batch_stats* st);
int gpudiff_dbatch_device_view(const gpudiff_dbatch* db, gpudiff_device_view* v);
/* async device-to-device copy of a diffed batch's results into caller memory
 * (e.g. a tensor handed to an RCCL all-gather), ordered on the context
 * stream; copies min(count, max_elems) elements of `what` */
#define GPUDIFF_EXPORT_COUNTS 0u      /* 8 x u32: n_spec, n_status, n_dirty, K4 scratch entries (saturating),
                                         overflow, n_paths, any join deferred to K3/K4, regions whose changed
                                         paths K2 emitted from its compare stream without the merge-join */
#define GPUDIFF_EXPORT_SPEC_IDS 1u    /* u32 */
#define GPUDIFF_EXPORT_STATUS_IDS 2u  /* u32 */
#define GPUDIFF_EXPORT_DIRTY_IDS 3u   /* u32 */
#define GPUDIFF_EXPORT_FLAGS 4u       /* u8 per pair */
int gpudiff_dbatch_export(gpudiff_ctx* ctx, const gpudiff_dbatch* db, uint32_t what, void* dst_device,
                          uint64_t max_elems, uint64_t known_count);
/* Gather binding: while bound, every diff of this batch also writes -- from its K3 compaction, no extra
 * launch or copy -- the buffer a per-step all-gather sends (kcp_amd/shard.py DirtyGather): u32
 * [8 counts | cap_spec spec-dirty IDs | cap_status status-dirty IDs], counts = (n_spec, n_status, n_dirty,
 * K4 scratch entries, 0, 0, 0, 0).  The counts are the batch totals even past a capacity; IDs past it are
 * not written (the caller grows its buffers and exports them with gpudiff_dbatch_export, whose lists are
 * always complete).  Words 4..7 are zeroed here, on the context stream, when the buffer differs from the
 * one bound (rebinding the same buffer is free).  send_dev = NULL unbinds. */
int gpudiff_dbatch_bind_gather(gpudiff_ctx* ctx, gpudiff_dbatch* db, void* send_dev, uint32_t cap_spec,
                               uint32_t cap_status);
/* Result slots: the spec / status dirty-ID lists and the counts (GPUDIFF_EXPORT_COUNTS) come in two slots
 * (0 by default; slot 1 allocated on first use).  Later diffs write, and exports / gpudiff_wait read, the
 * selected slot; the other keeps the lists and counts of the last diff made under it.  A per-step collective that checks step s's gathered counts only after
 * step s + 1's diff is enqueued alternates slots by step, so a capacity regrow can still export step s's
 * complete lists (kcp_amd/shard.py DirtyGather, lookahead).  Host-only state: ordered like every call. */
int gpudiff_dbatch_result_slot(gpudiff_ctx* ctx, gpudiff_dbatch* db, uint32_t slot);
/* synchronous D2H copy of resident pool bytes (inspection / tests) */
int gpudiff_dbatch_read_pool(gpudiff_ctx* ctx, const gpudiff_dbatch* db, uint64_t off, void* dst,
                             uint64_t bytes);
void gpudiff_dbatch_free(gpudiff_ctx* ctx, gpudiff_dbatch* db);

/* ---- sharding by logical cluster ----
 * The reference runs one syncer per logical cluster (pkg/reconciler/cluster/cluster.go:125-138), so a
 * node shards pairs by whole cluster with no data-path exchange.  A rank's step time is its decision
 * kernel's byte stream, so clusters are balanced by Σ B_pair, not by pair count (object sizes differ by
 * tenant).  Host-only; no GPU needed.
 * gpudiff_cluster_bytes adds each row's B_pair -- the bytes K2 streams for it: the 64-B row, the flag
 * and both objects' compared 16-B chunks (gpudiff_pair_compare_bytes, gpudiff_format.h) -- into
 * out[row.cluster_id] (out has n_clusters entries; a row with cluster_id >= n_clusters is
 * GPUDIFF_E_INVAL).  Weights can come from the previous step's encoded rows of each cluster.
 * gpudiff_shard_lpt: greedy LPT -- clusters by descending weight (ties: lower cluster id) each onto the
 * least-loaded rank (ties: lower rank); owner[c] = its rank.  The heaviest rank's load is at most
 * 4/3 of the optimum (Graham's bound) and within one cluster's weight of the mean. */
int gpudiff_cluster_bytes(const gpudiff_pair_row* rows, size_t n, uint32_t n_clusters, uint64_t* out);
int gpudiff_shard_lpt(const uint64_t* weights, uint32_t n_clusters, uint32_t world, int32_t* owner);
/* *out = the sum of gpudiff_pair_stream_bytes (gpudiff_format.h) over the rows with GPUDIFF_OBJ_SPEC_SHAPE_EQ masked:
 * the format's bytes less the 64-B rows and the key holes alone -- DESIGN.md §6n's measure, what the decision kernel
 * read before it honoured shape holes.  For measurements: the shard weight stays gpudiff_cluster_bytes. */
int gpudiff_rows_stream_bytes(const gpudiff_pair_row* rows, size_t n, uint64_t* out);
/* *out = the same sum with every bit honoured: what the decision kernel really reads for the rows from their
 * descriptors, key and shape holes left out (16 B + 32 B per streamed chunk, a pair) */
int gpudiff_rows_read_bytes(const gpudiff_pair_row* rows, size_t n, uint64_t* out);
/* *out = the sum of gpudiff_pair_image_bytes: what the decision kernel reads at most for the rows when every pair that
 * can be is streamed from the compare image, each image part at its slot's size (gpudiff_rows_read_bytes where none
 * is) */
int gpudiff_rows_image_read_bytes(const gpudiff_pair_row* rows, size_t n, uint64_t* out);
/* The sum above is an upper bound: an imaged pair's regions are packed to their values' true lengths
 * (gpudiff_format.h: gpudiff_meta_packed), which takes the metas, and a row has none.  *out = what the decision kernel
 * streams for the imaged rows alone -- 16 B + 32 B per streamed chunk of the packed parts, a pair; rows that are not
 * imaged add nothing -- with the parts packed by A's metas in pool, the host batch's pool the rows' offsets count
 * from.  The same sum as gpudiff_dbatch_image_streamed_bytes gives for a batch whose image held every such pair. */
int gpudiff_rows_image_streamed_bytes(const gpudiff_pair_row* rows, size_t n, const uint8_t* pool, uint64_t* out);

/* ---- diff (the hot path) ---- */
/* enqueue K2..K6 on the context stream; returns immediately */
int gpudiff_diff(gpudiff_ctx* ctx, gpudiff_dbatch* db, gpudiff_ticket* ticket);
/* block until the ticket's diff finished and copy results to host */
int gpudiff_wait(gpudiff_ctx* ctx, gpudiff_ticket ticket, gpudiff_result* res);
void gpudiff_result_release(gpudiff_ctx* ctx, gpudiff_result* res);
/* mean per-kernel times over the passes recorded since the last reset
 * (GPUDIFF_OPT_TIMING); synchronizes the context stream */
int gpudiff_last_timings(gpudiff_ctx* ctx, gpudiff_timings* t);
int gpudiff_timing_reset(gpudiff_ctx* ctx);
int gpudiff_sync(gpudiff_ctx* ctx);
/* What the context's diff passes cost since gpudiff_open (GPUDIFF_OPT_SMALL_PASS).  A pass takes the fused kernel
 * iff the option is set, 1 <= n_pairs <= GPUDIFF_SMALL_PASS_MAX_PAIRS, no gather send buffer is bound
 * (gpudiff_dbatch_bind_gather) and no gpudiff_k2_profile buffer is installed; every other pass is the ordinary one.
 * The kernel declines to finish a pass whose paths do not fit the batch's path arena (redo_arena), that holds a join
 * over more keys than one wave takes (redo_deep: the ordinary pass slices those over many waves) or that has more
 * than GPUDIFF_SMALL_PASS_MAX_PATHS changed paths (redo_paths); gpudiff_wait then runs the ordinary pass over the
 * batch.  GPUDIFF_E_NODEVICE on a host-only context. */
typedef struct gpudiff_pass_stats {
    uint64_t passes;          /* diff passes enqueued */
    uint64_t small_passes;    /* fused small passes launched */
    uint64_t small_redone;    /* of those: declined by the kernel, run again as the ordinary pass in gpudiff_wait */
    uint64_t redo_arena, redo_deep, redo_paths; /* small_redone by reason (a pass can count under several) */
    uint64_t readback_rounds; /* host synchronisations spent reading results back, over all passes */
} gpudiff_pass_stats;
int gpudiff_pass_stats_get(gpudiff_ctx* ctx, gpudiff_pass_stats* out);

/* encode + upload into a context-owned batch + diff (the syncer batcher's call) */
int gpudiff_submit(gpudiff_ctx* ctx, const gpudiff_json_pair* pairs, size_t n,
                   gpudiff_ticket* ticket);

/* ---- per-cluster index of a pass's dirty IDs ----
 * The reference runs one syncer per logical cluster (pkg/reconciler/cluster/cluster.go:125-138), each with its own
 * work queue fed by AddToQueue (pkg/syncer/syncer.go:222-224).  The index says whose queue a dirty pair belongs to:
 * a pure function of the waited pass's rows i = 0..n-1 in batch order (pair_id[i], cluster_id[i], final flags[i]):
 *   cluster_ids  the distinct cluster ids with at least one pair carrying GPUDIFF_SPEC_DIRTY or GPUDIFF_STATUS_DIRTY,
 *                ascending as unsigned 32-bit values (any u32 is a legal id, 0 and 0xFFFFFFFF included);
 *   spec_ids     the pair_id of every spec-dirty pair, ordered by (cluster_id ascending, batch position ascending);
 *   status_ids   the same for the status-dirty pairs;
 *   spec_off / status_off  cluster_ids[j] owns spec_ids[spec_off[j], spec_off[j + 1]) and the like slice of
 *                status_ids (a listed cluster may have an empty slice of one kind).
 * A decode-error pair is dirty in both kinds, as its flags say; the no-op bits play no part.  When the batch's dirty
 * pairs already lie in non-decreasing cluster order (a resident batch laid out by cluster), spec_ids and status_ids
 * equal the result's spec_dirty_ids and status_dirty_ids element for element and no sort runs.
 *
 * gpudiff_cluster_index_get builds it on the device (kernels K23 - K25, a radix sort between them only when the dirty
 * list does not ascend by cluster) from what the pass left in HBM, for tickets of gpudiff_diff (on a batch or on a
 * view, which reads its base's rows) and of gpudiff_submit batches the host encoded.  Valid after gpudiff_wait on the
 * ticket has returned and until that batch is diffed or submitted again.  On demand: a caller that never makes the
 * call launches and allocates nothing.  At most three host synchronisations per call, none when nothing is dirty.
 * GPUDIFF_E_STATE: an unknown, unwaited or superseded ticket, and a ticket whose flags the host may still patch
 * (device-encoded gpudiff_submit batches, every gpudiff_store_submit ticket: their deferred rows' final flags live on
 * the host); GPUDIFF_E_NODEVICE: a host-only context; GPUDIFF_E_CAPACITY: out of device memory; GPUDIFF_E_DEVICE
 * also when the index's counts disagree with the pass's own (never a silently wrong index).
 * The arrays belong to the index until gpudiff_cluster_index_release (ctx may be NULL for a host-built index). */
typedef struct gpudiff_cluster_index {
    size_t n_clusters;
    const uint32_t* cluster_ids;   /* [n_clusters] ascending, distinct */
    const uint32_t* spec_off;      /* [n_clusters + 1] */
    const uint32_t* status_off;    /* [n_clusters + 1] */
    size_t n_spec, n_status;       /* == the result's n_spec_dirty / n_status_dirty */
    const uint32_t* spec_ids;
    const uint32_t* status_ids;
    uint32_t sorted_on_device;     /* 0: the dirty list was already in cluster order, no sort ran */
    void* internal;
} gpudiff_cluster_index;
int gpudiff_cluster_index_get(gpudiff_ctx* ctx, gpudiff_ticket ticket, gpudiff_cluster_index* out);
void gpudiff_cluster_index_release(gpudiff_ctx* ctx, gpudiff_cluster_index* idx);
/* The same function on the host, one thread, no GPU needed (host-only callers, the tests' second implementation, the
 * measurements' baseline): flags / pair_ids / cluster_ids of n rows in batch order.  sorted_on_device is 0.
 * GPUDIFF_E_INVAL: n > 0xFFFFFFFF or a missing array. */
int gpudiff_cluster_index_host(const uint8_t* flags, const uint32_t* pair_ids, const uint32_t* cluster_ids, size_t n,
                               gpudiff_cluster_index* out);
/* what the context's gpudiff_cluster_index_get calls cost since gpudiff_open; kernel_ms needs GPUDIFF_OPT_TIMING (HIP
 * events around K23, around the sort + K24 + scan, and around K25, summed over timed_calls).  GPUDIFF_E_NODEVICE on a
 * host-only context. */
typedef struct gpudiff_cluster_index_stats {
    uint64_t calls;         /* calls that returned an index */
    uint64_t sorted_calls;  /* of those: the radix sort ran */
    uint64_t syncs;         /* host synchronisations: at most 3 a call, 0 for a pass with nothing dirty */
    uint64_t entries;       /* dirty entries indexed */
    uint64_t d2h_bytes;     /* the packed blocks copied back */
    double kernel_ms;
    uint64_t timed_calls;
} gpudiff_cluster_index_stats;
int gpudiff_cluster_index_stats_get(gpudiff_ctx* ctx, gpudiff_cluster_index_stats* out);
/* The index of ANY waited ticket, under the batch's final flags -- the ones gpudiff_wait returned in pair_flags:
 * the same function, the same gpudiff_cluster_index (released with gpudiff_cluster_index_release), also for the
 * tickets gpudiff_cluster_index_get refuses: device-encoded gpudiff_submit batches and every gpudiff_store_submit
 * ticket, whose deferred rows the host resolved.  Such a row found clean is not in the index (a cluster whose only
 * dirty row it was is not listed); one found dirty in one kind is in that kind's slice only; a conservative exit or
 * an undecodable pair stays dirty in both.  A ticket gpudiff_cluster_index_get serves gets an identical index.
 * On the device: the final dirty set is a subset of the pass's dirty list, so with host-resolved rows K26 writes
 * their final flags over a copy of the pass's, K27 counts the list's entries that are still dirty (held to
 * gpudiff_wait's n_dirty) and K28 compacts the list when some are not; K23 - K25 then run as they do for
 * gpudiff_cluster_index_get.  At most four host synchronisations a call, three without host-resolved rows, none
 * when nothing is dirty.  Runs on the context stream.
 * Valid after gpudiff_wait on the ticket has returned and until that batch is diffed or submitted again (a store
 * ticket: until its ring slot's next gpudiff_store_submit, the write plan's window).  GPUDIFF_E_STATE: anything
 * else; GPUDIFF_E_NODEVICE: a host-only context; GPUDIFF_E_CAPACITY: out of device memory; GPUDIFF_E_DEVICE also when
 * the device's counts disagree with the final ones (never a silently wrong index). */
int gpudiff_cluster_index_get_final(gpudiff_ctx* ctx, gpudiff_ticket ticket, gpudiff_cluster_index* out);
/* what the context's gpudiff_cluster_index_get_final calls cost since gpudiff_open (gpudiff_cluster_index_stats is
 * not moved by them); kernel_ms needs GPUDIFF_OPT_TIMING (HIP events around K26 + K27 + scan and around K28, added to
 * the three spans of gpudiff_cluster_index_stats).  GPUDIFF_E_NODEVICE on a host-only context. */
typedef struct gpudiff_cluster_index_final_stats {
    uint64_t calls;            /* calls that returned an index */
    uint64_t patched_calls;    /* of those: the batch had host-resolved rows */
    uint64_t compacted_calls;  /* of those: some entry of the pass's dirty list was dropped and K28 ran */
    uint64_t sorted_calls;     /* the radix sort ran */
    uint64_t syncs;            /* host synchronisations: at most 4 a call, 3 without host-resolved rows */
    uint64_t entries_in;       /* entries of the passes' dirty lists */
    uint64_t entries_live;     /* of those: still dirty under the final flags, indexed */
    uint64_t patch_rows;       /* host-resolved rows whose final flags were uploaded (or, all clean, just counted) */
    uint64_t h2d_bytes;        /* those uploads */
    uint64_t d2h_bytes;        /* the packed blocks copied back */
    double kernel_ms;
    uint64_t timed_calls;
} gpudiff_cluster_index_final_stats;
int gpudiff_cluster_index_final_stats_get(gpudiff_ctx* ctx, gpudiff_cluster_index_final_stats* out);

/* ---- device-resident object store (watch replay) ----
 * The informer cache's "old" objects stay resident in HBM, one per caller
 * slot (the shim maps (cluster, gvr, namespace, name) to a slot, as the
 * indexer at pkg/syncer/syncer.go:318 keys its cache).  An Update event
 * uploads only its new version: the engine diffs it against the slot's
 * resident version -- UpdateFunc(old, new), specsyncer.go:47-51 and
 * statussyncer.go:32-36 -- and the new version becomes the resident one.
 * Events of one batch apply in order, so two events on one slot chain.
 * Exactness: every resident blob carries a path table (one entry per region
 * leaf and ancestor: its hash, its parent's hash, its last component;
 * include/gpudiff_format.h); a new version's table must agree
 * with the resident one, which makes every shared path hash name the same path
 * in both.  A disagreement (a path-hash collision between versions, or within
 * the new one) re-encodes the pair with the smallest valid seed from old_json
 * (dirty with GPUDIFF_DECODE_ERROR when old_json is absent).  Blobs are
 * appended to the current space and the live ones are packed into the other
 * space (K7 k_move_blobs) when it fills. */
typedef struct gpudiff_store gpudiff_store;

typedef struct gpudiff_event {
    uint32_t slot;            /* < max_slots */
    uint32_t pair_id;         /* echoed in the result id lists */
    uint32_t cluster_id;      /* logical cluster */
    uint32_t reserved;        /* 0 */
    const uint8_t* new_json;  /* the event's object (required) */
    size_t new_len;
    /* optional: the informer's old object, read only when the slot is empty
     * (a first sighting diffs against it) or a collision forces a re-seed.
     * An empty slot without old_json diffs against the empty object {};
     * a collision without old_json reports the event dirty with
     * GPUDIFF_DECODE_ERROR (conservative) and stores the new version. */
    const uint8_t* old_json;
    size_t old_len;
} gpudiff_event;

typedef struct gpudiff_store_stats {
    uint64_t max_slots, live_slots;
    uint64_t space_bytes;      /* per space (two are allocated) */
    uint64_t used_bytes;       /* appended to the current space */
    uint64_t live_bytes;       /* resident blobs */
    uint64_t compactions;
    uint64_t events, old_encoded, reseeded, collisions_unresolved;
    uint64_t last_batch_bytes; /* bytes uploaded by the last submit (blobs; device-encode: JSON) */
    uint64_t deferred;         /* device-encode: events K0 handed to the host encoder */
    /* device-encode with GPUDIFF_OPT_TIMING: per-batch means (ms) of the host side of submit,
     * the H2D copy, K0 and K0c+K0x */
    float host_submit_ms, h2d_ms, encode_ms, link_ms;
    /* the host side of submit split: waiting for the ring slot's previous upload,
     * the document / slot-chain tables, the JSON copy into pinned staging, the
     * enqueue of copies and kernels; and the store's part of gpudiff_wait */
    float submit_wait_ms, submit_docs_ms, submit_copy_ms, submit_enqueue_ms, finish_ms;
    uint32_t timing_batches; /* batches the means are over */
    uint32_t zero_copy_batches; /* batches uploaded straight from a gpudiff_host_alloc buffer (gpudiff_submit's
                                    device-encode pairs, or this store's device-encode events) */
    uint64_t space_conservative; /* device-encode: deferred events reported dirty (GPUDIFF_DECODE_ERROR, slot
                                    emptied) because the space could not take their re-encoded blobs */
} gpudiff_store_stats;

int gpudiff_store_create(gpudiff_ctx* ctx, uint32_t max_slots, uint64_t space_bytes, uint32_t max_events,
                         gpudiff_store** out);
/* GPUDIFF_STORE_DEVICE_ENCODE: events go up as raw JSON; kernel K0 encodes
 * them in HBM, K0c checks collisions against the resident versions, K0x
 * chains events per slot, and the host encoder only re-does the events K0
 * defers (GPUDIFF_TOK_*), inside gpudiff_wait, with identical results.  In
 * this mode event buffers must stay valid until gpudiff_wait on the ticket
 * returns, and tickets are waited in submit order (at most two in flight). */
#define GPUDIFF_STORE_DEVICE_ENCODE 0x1u
int gpudiff_store_create_ex(gpudiff_ctx* ctx, uint32_t max_slots, uint64_t space_bytes, uint32_t max_events,
                            uint32_t flags, gpudiff_store** out);
/* encode (host threads), H2D into the current space,
 * K2..K6 over the batch's (resident, new) pairs; results via gpudiff_wait.
 * Two submits may be in flight (the next batch encodes while the GPU diffs
 * the previous one); wait on a ticket before its slot in the ring is reused. */
int gpudiff_store_submit(gpudiff_ctx* ctx, gpudiff_store* st, const gpudiff_event* events, size_t n,
                         gpudiff_ticket* ticket);
/* Delete event: the slot is empty again */
int gpudiff_store_forget(gpudiff_ctx* ctx, gpudiff_store* st, uint32_t slot);
int gpudiff_store_stats_get(const gpudiff_store* st, gpudiff_store_stats* out);
/* The same statistics for gpudiff_submit's device-encode path (GPUDIFF_OPT_DEVICE_ENCODE: the context's
 * pair-mode store), e.g. the per-phase times of JSON-in with GPUDIFF_OPT_TIMING; GPUDIFF_E_STATE before the
 * context's first device-encoded submit. */
int gpudiff_submit_stats_get(gpudiff_ctx* ctx, gpudiff_store_stats* out);
void gpudiff_store_free(gpudiff_ctx* ctx, gpudiff_store* st);
/* Pinned host memory for gpudiff_submit's JSON on a device-encode context (no reference counterpart: the syncer
 * batcher renders each flush's objects into it).  A batch whose documents all lie in ONE such
 * buffer, in pair order (old_0, new_0, old_1, new_1, ...), each at a 16-B aligned address and followed by at
 * least its staged span -- len + 32 bytes rounded up to 16 -- before the next document (the last one's span and
 * 32 more bytes inside the buffer) is uploaded straight from it: no staging copy.  The engine zeroes each
 * document's padding up to that span (those bytes are its to write).  The same holds for gpudiff_store_submit on
 * a GPUDIFF_STORE_DEVICE_ENCODE store (the watch stream's events rendered straight into engine-pinned memory):
 * the documents the store encodes -- per event, in submit order, its old object when the slot is seen for the
 * first time, then its new object -- lie in ONE such buffer in that order, 16-B aligned, each followed by its
 * staged span before the next (gaps allowed; old objects the store does not encode may lie anywhere).  Any
 * other layout takes the staging copy; results are identical either way
 * (gpudiff_store_stats.zero_copy_batches counts the zero-copy ones).  The buffer must stay untouched until
 * gpudiff_wait on the ticket returns; gpudiff_close frees what is left. */
int gpudiff_host_alloc(gpudiff_ctx* ctx, size_t bytes, void** out);
int gpudiff_host_free(gpudiff_ctx* ctx, void* p);

/* ---- object encoding in the device-store format (inspection / parity) ----
 * An object's blob followed by its path table (gpudiff_format.h: the node
 * hashes, parent hashes and last components of the region leaves and their
 * ancestors, which the store checks old-vs-new paths with exactly).
 * gpudiff_encode_objects
 * runs kernel K0 (the device JSON tokenizer + encoder) over n documents;
 * gpudiff_encode_object_host runs the host encoder (the Go-exact path) over
 * one.  Where K0 reports GPUDIFF_TOK_OK the two are byte-identical. */
typedef struct gpudiff_obj_info {
    int32_t status;          /* GPUDIFF_TOK_*: 0 = encoded */
    uint32_t oflags;         /* GPUDIFF_OBJ_HAS_STATUS */
    uint32_t spec_l, spec_ar, stat_l, stat_ar;
    uint64_t off;            /* blob offset in out */
    uint64_t bytes;          /* blob + path-table bytes */
    uint32_t n_tab;          /* path-table entries */
    uint32_t reserved;
} gpudiff_obj_info;

int gpudiff_encode_objects(gpudiff_ctx* ctx, const uint8_t* const* docs, const size_t* lens, const uint32_t* seeds,
                           size_t n, uint8_t* out, uint64_t out_cap, gpudiff_obj_info* info);
int gpudiff_encode_object_host(const uint8_t* doc, size_t len, uint32_t seed, uint32_t path_hash_bits, uint8_t* out,
                               uint64_t out_cap, gpudiff_obj_info* info);
/* Renders the path of `path_hash` (masked, as reported in gpudiff_result.path_hashes) from one object's blob in
 * the device-store format: `blob` points at the blob itself (out + info->off of gpudiff_encode_objects, out of
 * gpudiff_encode_object_host), `seed` is the seed it was encoded under.  No GPU needed: the walk kernels K15 / K16
 * do, on the host.  Writes *out_len bytes into buf, raw key bytes, no terminator.
 * GPUDIFF_E_NOTFOUND: the hash is not in the table (or its chain of parents does not reach the root within 256
 * nodes); GPUDIFF_E_STATE: the blob has no valid table (n_tab == GPUDIFF_TAB_NONE) or was not encoded;
 * GPUDIFF_E_CAPACITY: the text is longer than cap, *out_len is still set. */
int gpudiff_render_path_from_blob(const uint8_t* blob, const gpudiff_obj_info* info, uint32_t seed,
                                  uint64_t path_hash, char* buf, size_t cap, size_t* out_len);
/* The value twin of gpudiff_render_path_from_blob: the leaf whose key is `path_hash` in the blob's spec
 * (status_region == 0) or status segment, as *tag and the text gpudiff_result_path_values gives, *out_len bytes into
 * buf, no terminator.  No GPU needed: the routine kernels K21 / K22 run, on the host.
 * GPUDIFF_E_NOTFOUND: the hash is not in that region's keys, or the leaf's record does not check out;
 * GPUDIFF_E_CAPACITY: the text is longer than cap, *out_len is still set; GPUDIFF_E_STATE: the object was not encoded. */
int gpudiff_render_value_from_blob(const uint8_t* blob, const gpudiff_obj_info* info, uint32_t status_region,
                                   uint64_t path_hash, uint8_t* tag, char* buf, size_t cap, size_t* out_len);
/* profiling hook: K0 per-phase wall-clock ticks (100 MHz, summed over waves) since the
 * previous call (scan, tree, values, hashes, sort, blob, -, -); enable != 0
 * keeps recording */
int gpudiff_k0_profile(gpudiff_ctx* ctx, int enable, uint64_t* ticks8);
/* profiling hook: the decision kernel's per-wave timeline.  While a buffer is installed (dev_buf != NULL) this
 * context's passes run the timeline build of the decision kernel (the same kernel plus timestamps), writing 12
 * u64 per wave (start, end of the first
 * item, items, start of the last item, end, streaming ticks, join ticks, hardware CU id, then ticks
 * spent per item on its rows, between its rows and its first pass, after its joins, and from one
 * item's end to the next one's start; 100 MHz) into device memory dev_buf of cap_waves records;
 * dev_buf NULL stops recording and returns the context to the default build */
int gpudiff_k2_profile(gpudiff_ctx* ctx, uint64_t* dev_buf, uint32_t cap_waves);

/* ---- write path: the request body for a dirty object ----
 * GPUDIFF_UPSERT_SPEC: what upsertIntoDownstream hands to client.Create
 *   (pkg/syncer/specsyncer.go:86-110): the object with metadata.uid and
 *   metadata.resourceVersion removed and every owner reference whose name equals
 *   the kcp.dev/owned-by label dropped (the rest normalized as
 *   Unstructured.SetOwnerReferences writes them; the field removed when none
 *   remain).
 * GPUDIFF_UPSERT_STATUS: updateStatusInUpstream's object (statussyncer.go:41-48)
 *   before the live resourceVersion is set: uid and resourceVersion removed.
 * Bytes are exactly json.NewEncoder(w).Encode(obj.Object) of Go 1.16 -- what the
 * dynamic client sends (UnstructuredJSONScheme): keys sorted, HTML-safe string
 * escaping, shortest floats, trailing newline.  Kernel K10 emits the bodies in
 * HBM; documents outside its subset (floats, duplicate keys, undecodable input,
 * ...) are marshalled by the host path, with identical bytes. */
#define GPUDIFF_UPSERT_SPEC 0u
#define GPUDIFF_UPSERT_STATUS 1u

typedef struct gpudiff_bodies {
    size_t n;
    const uint64_t* offsets;  /* n + 1: body i = bytes[offsets[i], offsets[i + 1]) */
    const uint8_t* bytes;
    const int32_t* status;    /* 0 = body; GPUDIFF_E_DECODE = Go could not decode the object (empty body) */
    const uint8_t* source;    /* GPUDIFF_BODY_DEVICE / GPUDIFF_BODY_HOST per document */
    const int32_t* k10_status; /* K10's GPUDIFF_TOK_* per document (why the host took it over) */
    size_t n_host;            /* documents the host marshalled */
    void* internal;
} gpudiff_bodies;
#define GPUDIFF_BODY_DEVICE 0u
#define GPUDIFF_BODY_HOST 1u

/* n documents (JSON objects) -> n bodies; synchronous.  Release with
 * gpudiff_bodies_release. */
int gpudiff_upsert_bodies(gpudiff_ctx* ctx, const uint8_t* const* docs, const size_t* lens, size_t n, uint32_t mode,
                          gpudiff_bodies* out);
void gpudiff_bodies_release(gpudiff_ctx* ctx, gpudiff_bodies* b);

/* Gate -> write on the device.  For a
 * batch submitted with GPUDIFF_OPT_DEVICE_ENCODE and waited (gpudiff_wait), the
 * writes the syncer issues for its decisions, rendered by K10 from the pairs'
 * JSON still staged in HBM -- no re-upload.  Which document a write renders
 * depends on what the submitted pairs are (`mode` of gpudiff_write_plan_get_ex):
 *   GPUDIFF_PLAN_INFORMER (default): each pair is an informer Update event
 *     (old, new).  UpdateFunc enqueues newObj (specsyncer.go:47-50,
 *     statussyncer.go:32-35) and the worker writes that object, so both kinds
 *     render the NEW document: a spec-dirty pair gets upsertIntoDownstream's
 *     body of new (GPUDIFF_UPSERT_SPEC, specsyncer.go:86-132), a status-dirty
 *     pair updateStatusInUpstream's body of new (GPUDIFF_UPSERT_STATUS,
 *     statussyncer.go:41-63).
 *   GPUDIFF_PLAN_UPSTREAM_DOWNSTREAM: each pair is (A = upstream/kcp copy,
 *     B = downstream copy): a spec-dirty pair gets the spec body
 *     of A (written over B), a status-dirty pair the status body of B (written
 *     into A).
 * GPUDIFF_PLAN_SPEC / GPUDIFF_PLAN_STATUS select which kinds are listed (an
 * upstream informer's batch wants spec writes only, a downstream informer's
 * status writes only); neither bit = both.
 * A write whose pair carries GPUDIFF_SPEC_NOOP / GPUDIFF_STATUS_NOOP is listed
 * with noop = 1 and no body: what the write carries in that region is, on the
 * wire, exactly what the write of the other document of the pair carries (Go
 * marshals int64 v and float64 v the same way).  For informer pairs that means
 * the call repeats the write already issued for `old`; for (A, B) pairs it
 * leaves B's compared content as it is.  Call after gpudiff_wait on the ticket
 * and before the submit after the next one (the staging is reused then);
 * GPUDIFF_E_STATE otherwise, or for a batch the context encoded on the host.
 * Release with gpudiff_write_plan_release. */
#define GPUDIFF_PLAN_INFORMER 0x0u
#define GPUDIFF_PLAN_SPEC 0x1u
#define GPUDIFF_PLAN_STATUS 0x2u
#define GPUDIFF_PLAN_UPSTREAM_DOWNSTREAM 0x4u
/* gpudiff_store_write_plan_get: also bring back each body's request target (gpudiff_bodies_targets), 16 B more per
 * write in the list that comes back.  gpudiff_write_plan_get_ex accepts and ignores it: its bodies always carry
 * their targets. */
#define GPUDIFF_PLAN_TARGETS 0x8u
typedef struct gpudiff_write_plan {
    size_t n;                    /* writes: the spec-dirty pairs (ascending index), then the status-dirty ones */
    const uint32_t* pair_index;  /* the pair's index in the submitted batch */
    const uint8_t* kind;         /* GPUDIFF_UPSERT_SPEC / GPUDIFF_UPSERT_STATUS */
    const uint8_t* noop;         /* 1 = skip the call (no body) */
    gpudiff_bodies bodies;       /* n bodies (empty for no-op writes; status GPUDIFF_E_DECODE = undecodable) */
    void* internal;
} gpudiff_write_plan;
/* gpudiff_write_plan_get = _ex(..., GPUDIFF_PLAN_INFORMER, ...).  ABI 3 rendered a spec write from the
 * pair's FIRST document (the upstream/downstream reading); since ABI 4 the default is the informer
 * reading (the NEW document).  Bindings must check gpudiff_abi_version() == GPUDIFF_ABI_VERSION at load
 * (the Go binding and kcp_amd/gpudiff.py refuse a mismatched library) and pass
 * GPUDIFF_PLAN_UPSTREAM_DOWNSTREAM to _ex for (A, B) pairs. */
int gpudiff_write_plan_get(gpudiff_ctx* ctx, gpudiff_ticket ticket, gpudiff_write_plan* out);
int gpudiff_write_plan_get_ex(gpudiff_ctx* ctx, gpudiff_ticket ticket, uint32_t mode, gpudiff_write_plan* out);
void gpudiff_write_plan_release(gpudiff_ctx* ctx, gpudiff_write_plan* p);

/* The write plan of a watch-replay batch: for a waited batch of a GPUDIFF_STORE_DEVICE_ENCODE
 * store, ONE write per dirty slot, rendering the slot's LAST version of the batch -- the worker re-reads the
 * latest object from the indexer and writes that (pkg/syncer/syncer.go:318), and the store is that indexer.  For
 * every slot with at least one event in the batch and each kind K (spec, status):
 *   dirty_K = OR over the slot's events in the batch of GPUDIFF_SPEC_DIRTY / GPUDIFF_STATUS_DIRTY (the final flags
 *             gpudiff_wait returned, host-resolved events included);
 *   if dirty_K, one write of kind K: the new_json of the slot's last event in the batch rendered as
 *             GPUDIFF_UPSERT_SPEC / GPUDIFF_UPSERT_STATUS, pair_index = that event's index in the submitted array;
 *   noop_K  = dirty_K and every event of the slot carrying the dirty bit of K also carries GPUDIFF_SPEC_NOOP /
 *             GPUDIFF_STATUS_NOOP (a clean event leaves the region's wire bytes as they were, a no-op dirty event
 *             too, so the last version's write carries what the write before the batch carried): no body.
 * Spec writes ascending by pair_index, then status writes ascending.  An undecodable last version is listed with
 * body status GPUDIFF_E_DECODE.  Several dirty events of one slot coalesce into one write (the reference would
 * issue the same write once per event).  The plan of batch b is a function of batch b's events and flags alone: it
 * does not look at batch b + 1, and it does not look at gpudiff_store_forget.
 * mode: GPUDIFF_PLAN_SPEC / GPUDIFF_PLAN_STATUS select the kinds (neither = both);
 * GPUDIFF_PLAN_UPSTREAM_DOWNSTREAM is GPUDIFF_E_INVAL (store events are informer events); GPUDIFF_PLAN_TARGETS adds
 * each body's request target to the list that comes back (16 B a write; without it the plan's bodies answer
 * gpudiff_bodies_targets with GPUDIFF_E_STATE and the copy back is what it was).
 * The bodies come from the batch's JSON still staged in HBM: nothing is uploaded again, and only the bodies' bytes
 * come back.  Call after gpudiff_wait on the ticket and before the submit after the next one (which reuses the ring
 * slot); GPUDIFF_E_STATE otherwise, for an unknown or unwaited ticket, for a host-encode store (its JSON never
 * reaches HBM) and for a store marked broken; GPUDIFF_E_CAPACITY when the plan's device buffers cannot be
 * allocated.  Fills a gpudiff_write_plan; release with gpudiff_write_plan_release. */
int gpudiff_store_write_plan_get(gpudiff_ctx* ctx, gpudiff_store* st, gpudiff_ticket ticket, uint32_t mode,
                                 gpudiff_write_plan* out);
/* What the store's last gpudiff_store_write_plan_get did (times with GPUDIFF_OPT_TIMING only, HIP events). */
typedef struct gpudiff_store_plan_stats {
    uint64_t calls;        /* plans built since the store was created */
    uint64_t events, docs; /* the batch: events, staged documents */
    uint64_t writes, noops, bodies, host_bodies;
    uint64_t body_bytes;   /* bytes of the bodies K10 rendered */
    uint64_t h2d_bytes;    /* uploaded: the host-resolved rows' flags, the deferred documents' gather list */
    uint64_t d2h_bytes;    /* copied back: the two records, the write list, the bodies, the deferred documents' JSON */
    uint64_t arena_bytes;  /* K10's output arena in HBM (never copied back) */
    double fold_ms;        /* final flags + K17 + scans + K18 */
    double k10_ms;
    double pack_ms;        /* the lengths' scan + K19 */
} gpudiff_store_plan_stats;
int gpudiff_store_plan_stats_get(const gpudiff_store* st, gpudiff_store_plan_stats* out);

/* The staged form: documents uploaded once into HBM (gpudiff_wbatch_create),
 * K10 launched on the context's stream (gpudiff_wbatch_run, asynchronous; with
 * GPUDIFF_OPT_TIMING each launch is bracketed by HIP events and
 * gpudiff_wbatch_stats.k10_ms is the mean), bodies read back and host-completed
 * (gpudiff_wbatch_fetch). */
typedef struct gpudiff_wbatch gpudiff_wbatch;
typedef struct gpudiff_wbatch_stats {
    uint64_t n_docs, json_bytes, body_bytes;  /* body_bytes: K10's output (valid after a fetch) */
    uint64_t scratch_bytes, out_cap_bytes;
    double k10_ms;                            /* mean K10 duration over the timed runs */
    uint64_t runs;                            /* timed runs (GPUDIFF_OPT_TIMING) */
} gpudiff_wbatch_stats;
int gpudiff_wbatch_create(gpudiff_ctx* ctx, const uint8_t* const* docs, const size_t* lens, size_t n, uint32_t mode,
                          gpudiff_wbatch** out);
int gpudiff_wbatch_run(gpudiff_ctx* ctx, gpudiff_wbatch* wb);
int gpudiff_wbatch_fetch(gpudiff_ctx* ctx, gpudiff_wbatch* wb, gpudiff_bodies* out);
int gpudiff_wbatch_stats_get(const gpudiff_wbatch* wb, gpudiff_wbatch_stats* st);
void gpudiff_wbatch_free(gpudiff_ctx* ctx, gpudiff_wbatch* wb);

/* The host path (Go-exact restatement; also what completes K10's deferrals):
 * one body into out[0, cap).  *out_len = the body length (also when it does not
 * fit: then GPUDIFF_E_CAPACITY).  GPUDIFF_E_DECODE if Go cannot decode doc. */
int gpudiff_upsert_body_host(const uint8_t* doc, size_t len, uint32_t mode, uint8_t* out, size_t cap,
                             size_t* out_len);

/* ---- the Update body: where the live resourceVersion goes ----
 * Every steady-state write sets the live object's resourceVersion on the body it sends: updateStatusInUpstream
 * always (Get -> SetResourceVersion(existing.GetResourceVersion()) -> UpdateStatus, pkg/syncer/statussyncer.go:50-57),
 * upsertIntoDownstream on every AlreadyExists (specsyncer.go:116-124).  SetResourceVersion(rv) with rv != "" is
 * SetNestedField(obj, rv, "metadata", "resourceVersion"): the member is set when metadata is a map, a new map
 * {"resourceVersion": rv} is created when the metadata key is absent, and nothing changes when metadata is present
 * and not a map (the accessor drops SetNestedField's error); rv == "" removes the field, which the body above has
 * done already.  The bytes stay json.NewEncoder(w).Encode(obj.Object): keys sorted, rv escaped as any Go string.
 *
 * With each body the engine reports where that member goes, so the Update body is two copies around a short string
 * once the Get has returned -- no decode, no second marshal.  One descriptor per body: `off`, a byte offset from the
 * body's first byte, and `form`:
 *   GPUDIFF_RV_NONE    no splice: the Update body is the body (metadata present and not a map; a write without a
 *                      body -- a no-op or a decode error)
 *   GPUDIFF_RV_INSERT  insert the member text at off
 *   GPUDIFF_RV_LEAD    the inserted text starts with ','
 *   GPUDIFF_RV_TRAIL   the inserted text ends with ','
 *   GPUDIFF_RV_WRAP    the member text is "metadata":{"resourceVersion":"<rv>"} instead of "resourceVersion":"<rv>"
 *                      (no metadata key at the root)
 * The choice is canonical, so that descriptors compare byte for byte: a visible member precedes in the container:
 * LEAD, off just past that member's value (where its ',' or the closing '}' stands); none precedes and one follows:
 * TRAIL, off just past the container's '{'; neither: no comma, off just past '{'.  Visible = emitted in the body
 * (not uid, not an ownerReferences member the spec transform removed).  Kernel K10 computes the descriptor for the
 * bodies it renders, the host path for the ones it marshals. */
#define GPUDIFF_RV_NONE 0u
#define GPUDIFF_RV_INSERT 0x1u
#define GPUDIFF_RV_LEAD 0x2u
#define GPUDIFF_RV_TRAIL 0x4u
#define GPUDIFF_RV_WRAP 0x8u
typedef struct gpudiff_rv_splice {
    size_t n;             /* = the bodies' n */
    const uint32_t* off;  /* n */
    const uint8_t* form;  /* n: GPUDIFF_RV_* */
    size_t n_device;      /* descriptors K10 computed (the bodies it rendered) */
    size_t n_host;        /* descriptors the host path computed (the bodies it marshalled; not decode errors) */
} gpudiff_rv_splice;
/* The descriptors of `b` (of gpudiff_upsert_bodies / gpudiff_wbatch_fetch, or &plan.bodies of either write plan).
 * The arrays live as long as the bodies do (gpudiff_bodies_release / gpudiff_write_plan_release). */
int gpudiff_bodies_rv_splice(gpudiff_ctx* ctx, const gpudiff_bodies* b, gpudiff_rv_splice* out);
/* body[0, len) with the resourceVersion member spliced in as (off, form) say, into out[0, cap); host only, no
 * context.  rv is escaped as Go escapes any string (HTML-safe, each invalid UTF-8 byte written as the escape of U+FFFD).  rv_len == 0 or
 * GPUDIFF_RV_NONE copies the body.  *out_len = the result's length, also when it does not fit (then
 * GPUDIFF_E_CAPACITY).  GPUDIFF_E_INVAL: an unknown form bit, form bits without GPUDIFF_RV_INSERT, or an off that
 * is not inside the body (0 < off < len when inserting). */
int gpudiff_splice_resource_version(const uint8_t* body, size_t len, uint32_t off, uint32_t form, const uint8_t* rv,
                                    size_t rv_len, uint8_t* out, size_t cap, size_t* out_len);
/* gpudiff_upsert_body_host plus the body's descriptor (*off, *form), as the host path records it while it writes
 * the body. */
int gpudiff_upsert_body_host_rv(const uint8_t* doc, size_t len, uint32_t mode, uint8_t* out, size_t cap,
                                size_t* out_len, uint32_t* off, uint32_t* form);
/* The Update body marshalled directly: decode, the transform of `mode`, SetResourceVersion(rv), marshal -- no
 * splicing.  The independent second implementation the splice is tested against, and what a caller without the
 * descriptor has to do per write.  Results as gpudiff_upsert_body_host. */
int gpudiff_update_body_host(const uint8_t* doc, size_t len, uint32_t mode, const uint8_t* rv, size_t rv_len,
                             uint8_t* out, size_t cap, size_t* out_len);

/* ---- the request target: the object's namespace and name ----
 * Controller.process reads meta.GetNamespace(), meta.GetName() first (pkg/syncer/syncer.go:310) and takes from them
 * the in-syncer-namespace skip (:311, :352-363), ensureNamespaceExists (specsyncer.go:87), getClient(gvr, namespace)
 * (syncer.go:344-350), the Get(name) before every Update (specsyncer.go:116, statussyncer.go:50) and Delete(name)
 * (specsyncer.go:83).  With each body the engine reports where those two strings stand in it, so a consumer that
 * holds only the plan sends the body without decoding it again.
 *
 * Two fields per body, GetName() / GetNamespace() = NestedString(obj, "metadata", field).  A field is PRESENT when
 * the root has a "metadata" member whose value is a JSON object ({} counts; null, a string, a number, a list do
 * not), that object has a member whose decoded key is exactly the field's name, and that member's value is a JSON
 * string; otherwise it is absent and its value is "".  The last of duplicate keys wins, as everywhere in Go's decode.
 *
 * Canonical, so that two implementations compare byte for byte: an absent field has offset 0, length 0 and no flag;
 * a present field has its flag, also when the value is "" (length 0, the offset just behind the opening quote);
 * _ESC is set exactly when the rendered span holds a backslash, i.e. Go's encoder escaped something in it -- without
 * _ESC the span is the value itself; a write without a body (a no-op, a Go decode error) has all fields zero. */
#define GPUDIFF_TGT_NAME 0x1u
#define GPUDIFF_TGT_NAME_ESC 0x2u
#define GPUDIFF_TGT_NS 0x4u
#define GPUDIFF_TGT_NS_ESC 0x8u
typedef struct gpudiff_targets {
    size_t n;             /* = the bodies' n */
    const uint32_t* off;  /* 2n: [2i] name, [2i+1] namespace; offset from the body's first byte of the first byte
                             after the value's opening quote */
    const uint32_t* len;  /* 2n: rendered bytes up to the closing quote */
    const uint8_t* flags; /* n: GPUDIFF_TGT_* */
    size_t n_device;      /* descriptors K10 computed (the bodies it rendered) */
    size_t n_host;        /* descriptors the host path computed (the bodies it marshalled; not decode errors) */
} gpudiff_targets;
/* The descriptors of `b` (of gpudiff_upsert_bodies / gpudiff_wbatch_fetch, or &plan.bodies of either write plan).
 * The arrays live as long as the bodies do.  GPUDIFF_E_STATE for the bodies of a gpudiff_store_write_plan_get
 * without GPUDIFF_PLAN_TARGETS. */
int gpudiff_bodies_targets(gpudiff_ctx* ctx, const gpudiff_bodies* b, gpudiff_targets* out);
/* body[off, off + len) with JSON escaping undone (what Go's encoder emits: \" \\ \n \r \t \b \f \uXXXX), into
 * out[0, cap); host only, no context.  *out_len = the result's length, also when it does not fit (then
 * GPUDIFF_E_CAPACITY).  GPUDIFF_E_INVAL: a span outside the body or a malformed escape. */
int gpudiff_target_decode(const uint8_t* body, size_t body_len, uint32_t off, uint32_t len, uint8_t* out, size_t cap,
                          size_t* out_len);
/* One document decoded and its two NestedString values returned directly: the independent second implementation the
 * descriptors are tested against, what a Delete event uses (it has no body), and what a caller without the
 * descriptor has to do per write.  *name_len / *ns_len are set also when a value does not fit (then
 * GPUDIFF_E_CAPACITY).  GPUDIFF_E_DECODE as gpudiff_upsert_body_host. */
int gpudiff_target_host(const uint8_t* doc, size_t len, uint8_t* name_out, size_t name_cap, size_t* name_len,
                        uint8_t* ns_out, size_t ns_cap, size_t* ns_len);
/* The distinct (cluster_id, namespace) pairs among the writes that have a body (status 0, not empty) and are not
 * skipped (skip[w] != 0), in order of first appearance: group_of[w] = the write's group, 0xFFFFFFFF for a write that
 * is not grouped; first[g] = the group's first write; *n_groups = their number.  ensureNamespaceExists then runs once
 * per namespace and downstream cluster instead of once per write.  cluster_ids (n, may be NULL: one cluster) and
 * skip (n, may be NULL) are the caller's; group_of and first hold n each.  Keys are compared as rendered bytes --
 * exact, because Go's encoding of a string is canonical; an absent namespace and "" fall into the same group. */
int gpudiff_targets_namespaces(const gpudiff_bodies* bodies, const gpudiff_targets* targets,
                               const uint32_t* cluster_ids, const uint8_t* skip, uint32_t* group_of, uint32_t* first,
                               size_t* n_groups);
/* gpudiff_upsert_body_host plus the body's target descriptor as the host path records it while it writes the body:
 * off[2], len[2] ([0] name, [1] namespace) and *flags. */
int gpudiff_upsert_body_host_targets(const uint8_t* doc, size_t len, uint32_t mode, uint8_t* out, size_t cap,
                                     size_t* out_len, uint32_t* off, uint32_t* tlen, uint32_t* flags);

/* ---- Deployment splitter status roll-up ----
 * pkg/reconciler/deployment/deployment.go:41-91: when a leaf Deployment
 * changes, the splitter lists every cached Deployment labelled
 * kcp.dev/owned-by=<root> (:44-51; all namespaces, all logical clusters), sums
 * their status.{replicas, updatedReplicas, readyReplicas, availableReplicas,
 * unavailableReplicas} into the root's status (:74-85, int32: Go wrap-around)
 * and copies others[0].status.conditions (:89-91).  Batch form: n cached
 * Deployments (JSON) -> one group per distinct owned-by value, ordered by first
 * appearance; others[0] is the member with the lowest index (the lister's order
 * is unspecified).  The objects are typed appsv1.Deployments: Go 1.16
 * encoding/json rules apply to the fields read (case-insensitive field names,
 * repeated keys merge, null is a no-op, counters must be int32 literals); a
 * document Go cannot decode gets GPUDIFF_ROLLUP_DECODE.  Kernel K11 extracts
 * the fields (roll-up mode of k_encode_docs), K12 groups by label on the device;
 * documents outside K11's subset (GPUDIFF_TOK_*) are decided by the host path
 * (gpudiff_rollup_doc_host), which then regroups the batch with identical
 * results. */
typedef struct gpudiff_rollup_group {
    uint32_t first_doc;  /* others[0]: its status.conditions become the root's */
    uint32_t n_members;
    int32_t sums[5];     /* replicas, updatedReplicas, readyReplicas, availableReplicas, unavailableReplicas */
    uint32_t reserved;
} gpudiff_rollup_group;
#define GPUDIFF_ROLLUP_NONE (-1)    /* no kcp.dev/owned-by label: not a leaf */
#define GPUDIFF_ROLLUP_DECODE (-2)  /* Go cannot decode the document into an appsv1.Deployment */

typedef struct gpudiff_rollup {
    size_t n_docs;
    const int32_t* doc_group;              /* [n_docs]: group index or GPUDIFF_ROLLUP_* */
    size_t n_groups;
    const gpudiff_rollup_group* groups;    /* ascending first_doc */
    const int32_t* k11_status;             /* [n_docs]: K11's GPUDIFF_TOK_* (why the host took it) */
    size_t n_host;                         /* documents the host path decided */
    uint32_t host_grouped;                 /* 1: the host regrouped (deferrals or a label-hash collision) */
    void* internal;
} gpudiff_rollup;

typedef struct gpudiff_rbatch gpudiff_rbatch;
typedef struct gpudiff_rbatch_stats {
    uint64_t n_docs, json_bytes, scratch_bytes;
    double k11_ms, k12_ms;  /* mean durations over the timed runs (GPUDIFF_OPT_TIMING) */
    uint64_t runs;
} gpudiff_rbatch_stats;
/* documents uploaded once into HBM; run = K11 + K12 on the context stream
 * (asynchronous); fetch = results to the host, host path for deferrals.  The
 * caller's document buffers must stay valid until gpudiff_rbatch_free (the
 * host path and regrouping read them). */
int gpudiff_rbatch_create(gpudiff_ctx* ctx, const uint8_t* const* docs, const size_t* lens, size_t n,
                          gpudiff_rbatch** out);
int gpudiff_rbatch_run(gpudiff_ctx* ctx, gpudiff_rbatch* rb);
int gpudiff_rbatch_fetch(gpudiff_ctx* ctx, gpudiff_rbatch* rb, gpudiff_rollup* out);
int gpudiff_rbatch_stats_get(const gpudiff_rbatch* rb, gpudiff_rbatch_stats* st);
void gpudiff_rbatch_free(gpudiff_ctx* ctx, gpudiff_rbatch* rb);
/* create + run + fetch + free */
int gpudiff_rollup_status(gpudiff_ctx* ctx, const uint8_t* const* docs, const size_t* lens, size_t n,
                          gpudiff_rollup* out);
void gpudiff_rollup_release(gpudiff_ctx* ctx, gpudiff_rollup* r);
/* the host path for one document (Go-exact typed decode of the fields read):
 * counters into v[5]; the owned-by value into label[0, cap) with *label_len
 * its length, or SIZE_MAX when the label is absent (GPUDIFF_E_CAPACITY when it
 * does not fit); GPUDIFF_E_DECODE when Go rejects the document. */
int gpudiff_rollup_doc_host(const uint8_t* doc, size_t len, int32_t* v, uint8_t* label, size_t cap,
                            size_t* label_len);

/* ---- API-negotiation update classifier (second half) ----
 * Replaces the "Update" branch of Controller.enqueue,
 * pkg/reconciler/apiresource/controller.go:253-283, for the three kinds its
 * toQueueElementType (:185-236) types: APIResourceImport and
 * NegotiatedAPIResource (GPUDIFF_NEG_KIND_API; both have status {conditions:
 * [{type, status, lastTransitionTime, reason, message}]}) and
 * CustomResourceDefinition (GPUDIFF_NEG_KIND_CRD, :186-199; apiextensions/v1
 * status {conditions (same five fields), acceptedNames {plural, singular,
 * shortNames[], kind, listKind, categories[]}, storedVersions[]}).  Per
 * (old, new) pair: no old object
 * -> CREATED; equal resourceVersion -> IGNORE; different generation -> SPEC;
 * status not Semantic.DeepEqual (nil == empty, metav1.Time by instant) ->
 * STATUS; annotations differ OR labels EQUAL (the reference's missing `!` at
 * :278, reproduced) -> META; else IGNORE.  Objects are decoded with Go 1.16
 * encoding/json typed rules; DECODE when a side is not valid JSON, is not an
 * object, or a field the classifier reads (metadata.resourceVersion /
 * generation / labels / annotations, the typed status's fields and their
 * elements) fails Go's typed decode.  Type errors in fields the classifier does not read
 * (spec, metadata.name, ...) are not checked: such an object cannot reach the
 * reference's informer at all, so no reference outcome exists for it.
 * Kernel K13 (negotiation mode of k_encode_docs) extracts each document's
 * fields, K14 classifies each pair on the device; pairs with a document outside
 * K13's subset are classified by the host path (gpudiff_negotiate_pair_host). */
#define GPUDIFF_NEG_IGNORE 0
#define GPUDIFF_NEG_SPEC 1     /* SpecChanged */
#define GPUDIFF_NEG_STATUS 2   /* StatusOnlyChanged */
#define GPUDIFF_NEG_META 3     /* AnnotationOrLabelsOnlyChanged */
#define GPUDIFF_NEG_CREATED 4  /* no old object */
#define GPUDIFF_NEG_DECODE (-1)
#define GPUDIFF_NEG_KIND_API 0 /* APIResourceImport / NegotiatedAPIResource */
#define GPUDIFF_NEG_KIND_CRD 1 /* CustomResourceDefinition */

typedef struct gpudiff_nbatch gpudiff_nbatch;
typedef struct gpudiff_nbatch_stats {
    uint64_t n_pairs, json_bytes, scratch_bytes, n_host;
    double k13_ms, k14_ms;  /* mean durations over the timed runs (GPUDIFF_OPT_TIMING) */
    uint64_t runs;
} gpudiff_nbatch_stats;
/* olds[i] == NULL: no old object.  The documents are uploaded once into HBM;
 * run = K13 + K14 on the context stream (asynchronous); fetch = actions[n] to
 * the host, host path for the deferred pairs (GPUDIFF_E_STATE before the first
 * run).  The caller's buffers must stay
 * valid until gpudiff_nbatch_free. */
int gpudiff_nbatch_create(gpudiff_ctx* ctx, const uint8_t* const* olds, const size_t* old_lens,
                          const uint8_t* const* news, const size_t* new_lens, size_t n, gpudiff_nbatch** out);
/* kinds[i]: GPUDIFF_NEG_KIND_* of pair i (NULL: all GPUDIFF_NEG_KIND_API --
 * what the *_kinds-less entry points use); other values: GPUDIFF_E_INVAL */
int gpudiff_nbatch_create_kinds(gpudiff_ctx* ctx, const uint8_t* kinds, const uint8_t* const* olds,
                                const size_t* old_lens, const uint8_t* const* news, const size_t* new_lens, size_t n,
                                gpudiff_nbatch** out);
int gpudiff_nbatch_run(gpudiff_ctx* ctx, gpudiff_nbatch* nb);
int gpudiff_nbatch_fetch(gpudiff_ctx* ctx, gpudiff_nbatch* nb, int32_t* actions);
int gpudiff_nbatch_stats_get(const gpudiff_nbatch* nb, gpudiff_nbatch_stats* st);
void gpudiff_nbatch_free(gpudiff_ctx* ctx, gpudiff_nbatch* nb);
/* The host path (Go-exact typed decode + classification) over n pairs on
 * `threads` host threads -- no device needed; what the batch falls back to for
 * K13's deferrals, exposed for CPU baselines and callers without a GPU. */
int gpudiff_classify_updates_host(const uint8_t* const* olds, const size_t* old_lens, const uint8_t* const* news,
                                  const size_t* new_lens, size_t n, uint32_t threads, int32_t* actions);
int gpudiff_classify_updates_host_kinds(const uint8_t* kinds, const uint8_t* const* olds, const size_t* old_lens,
                                        const uint8_t* const* news, const size_t* new_lens, size_t n, uint32_t threads,
                                        int32_t* actions);
/* create + run + fetch + free */
int gpudiff_classify_updates(gpudiff_ctx* ctx, const uint8_t* const* olds, const size_t* old_lens,
                             const uint8_t* const* news, const size_t* new_lens, size_t n, int32_t* actions);
int gpudiff_classify_updates_kinds(gpudiff_ctx* ctx, const uint8_t* kinds, const uint8_t* const* olds,
                                   const size_t* old_lens, const uint8_t* const* news, const size_t* new_lens, size_t n,
                                   int32_t* actions);
/* the host path for one pair (old == NULL: no old object) */
int gpudiff_negotiate_pair_host(const uint8_t* old_json, size_t old_len, const uint8_t* new_json, size_t new_len,
                                int32_t* action);
int gpudiff_negotiate_pair_host_kind(uint32_t kind, const uint8_t* old_json, size_t old_len, const uint8_t* new_json,
                                     size_t new_len, int32_t* action);

/* ---- single-pair drop-ins (same semantics as the Go predicates) ---- */
int gpudiff_spec_equal(gpudiff_ctx* ctx, const uint8_t* old_json, size_t old_len,
                       const uint8_t* new_json, size_t new_len, int* equal);
int gpudiff_status_equal(gpudiff_ctx* ctx, const uint8_t* old_json, size_t old_len,
                         const uint8_t* new_json, size_t new_len, int* equal);

/* ---- host helper: render a changed path ("spec.containers[0].image") ----
 * path_kind is the kind byte reported with the hash (selects the region). */
int gpudiff_resolve_path(const uint8_t* old_json, size_t old_len, const uint8_t* new_json,
                         size_t new_len, uint64_t path_hash, uint8_t path_kind,
                         uint32_t path_hash_bits, char* buf, size_t cap, size_t* out_len);

#ifdef __cplusplus
}
#endif
#endif
