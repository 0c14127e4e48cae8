/*
 * lsdsort.h -- C-ABI of the MI355X-native LSD radix sort (liblsdsort.so).
 *
 * Plain pointers and sizes only; no C++ or torch types.  Every entry returns 0
 * (LSDSORT_OK) or a negative lsdsort_status; nothing here aborts the process (the reference
 * crashes on any error: CUDA_CALL, LSDRadixSort/CudaUtils.h:7-8; MYASSERT, Utils.h:6-15).
 *
 * What each entry replaces in the reference (paths relative to /root/reference/, ".cu" =
 * LSDRadixSort/LSDRadixSort.cu) is cited at its declaration.  The reference has no
 * sort(uint32_t*, size_t) symbol; lsdsort_u32 is defined as "what
 * TestGPULSDRadixSort does between .cu:1001 and .cu:1005, minus RNG and checking".
 *
 * There is NO CPU fallback behind this ABI: without a usable gfx950 device every compute
 * entry returns LSDSORT_ERR_NO_DEVICE.  The CPU legs of the reference (std::sort .cu:97,
 * CPU LSD .cu:25-69) live in oracle/ as test infrastructure only.
 */
#ifndef LSDSORT_H
#define LSDSORT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(LSDSORT_BUILD)
#define LSDSORT_API __attribute__((visibility("default")))
#else
#define LSDSORT_API
#endif

typedef enum lsdsort_status {
    LSDSORT_OK = 0,
    LSDSORT_ERR_INVALID_ARG = -1,  /* null pointer with n > 0, bad radix_bits, bad enum          */
    LSDSORT_ERR_NO_DEVICE = -2,    /* no HIP device / not gfx950; also num_gpus == 0 (no CPU path) */
    LSDSORT_ERR_HIP = -3,          /* a HIP runtime call failed; see lsdsort_last_hip_error()    */
    LSDSORT_ERR_WORKSPACE = -4,    /* workspace null, misaligned or smaller than required        */
    LSDSORT_ERR_TOO_LARGE = -5,    /* n above LSDSORT_MAX_KEYS (a local argument check, never collective) */
    LSDSORT_ERR_UNSUPPORTED = -6,  /* valid request that cannot be served here (e.g. no librccl) */
    LSDSORT_ERR_DEVICE_FAULT = -7, /* a kernel gave up a bounded wait, or refused destinations outside  */
                                   /* the output because the counts do not describe the keys (see below) */
    LSDSORT_ERR_COMM = -8,         /* a collective failed or a peer left it; lsdsort_last_comm_error() */
    LSDSORT_ERR_CAPACITY = -9      /* sharded step: some rank's out_capacity is too small; EVERY rank  */
                                   /* returns this before anything is exchanged (retry with *n_out)    */
} lsdsort_status;

/* Largest n any entry accepts: the chained tile prefix keeps 30 value bits per word.  The
 * reference stops at int count < 2^31 (.cu:839) and in practice at 2^30 (.cu:1033-1042). */
#define LSDSORT_MAX_KEYS ((size_t)0x3fffffffu)

/* Which pass structure runs on the device. */
typedef enum lsdsort_algorithm {
    /* default: one read of all keys for every digit histogram, one scan of the digit counts,
     * then per pass ONE rank-and-scatter kernel whose per-tile bases come from a chained
     * (decoupled look-back) scan over tiles.  4*(2P+1) bytes per key. */
    LSDSORT_ALGO_ONESWEEP = 0,
    /* the reference's own stage structure (GPULSDRadixSort, .cu:839-910): per pass
     * BuildHistogram -> local/global offsets -> rank-and-scatter as separate kernels with
     * the [tile][digit] tables in memory.  12 bytes per key per pass.  Same results. */
    LSDSORT_ALGO_STAGED = 1
} lsdsort_algorithm;

/* ---- host-pointer entries ------------------------------------------------------------- */

/* sort(uint32_t* keys, size_t n) of BASELINE.json's north_star: host pointer, in place,
 * ascending.  Replaces the alloc / H2D / GPULSDRadixSort / D2H sequence of
 * TestGPULSDRadixSort, .cu:966-1005.  Blocking.  radix 8, current HIP device.
 * The input crosses PCIe in 64 MiB chunks with the upfront histogram of each chunk running behind it; the
 * device buffers and workspace are kept per device between calls (the reference allocates and frees around
 * every sort) -- lsdsort_release_host_cache() frees them; calls on one device take turns. */
LSDSORT_API int lsdsort_u32(uint32_t* keys, size_t n);
LSDSORT_API int lsdsort_release_host_cache(void);

/* Same with the radix width (1, 2, 4 or 8 -- the reference's sweep `rs`, .cu:1055-1062) and
 * a GPU count: num_gpus in {1, 2, 4, 8}.  0 (the "CPU path") returns
 * LSDSORT_ERR_NO_DEVICE.  More than one GPU: this one process drives devices 0 .. num_gpus-1 (one host
 * thread per device, one RCCL communicator made with ncclCommInitAll and kept for later calls): the array
 * is cut into num_gpus shards, each device runs lsdsort_sharded_u32_device (below) on its shard, and the
 * slices come back in rank order.  LSDSORT_ERR_NO_DEVICE if fewer gfx950 devices are visible,
 * LSDSORT_ERR_UNSUPPORTED if librccl cannot be loaded.  Every device first sets itself up (buffers for its share plus a
 * quarter, upload); the ranks then AGREE on a status before the first collective, so a device that fails there takes the call
 * down with an error instead of leaving its peers in an all-gather; skewed keys repeat the step once with exact sizes.
 * Calls with num_gpus > 1 take turns (one set of communicators per device count).  NOT YET RUN ON MORE THAN ONE DEVICE:
 * the same code is exercised with virtual ranks on one GPU (lsdsort_u32_loopback).  The one-process-per-GPU form (bench.py, a
 * torch.distributed or MPI launcher) uses the lsdsort_comm_* entries directly. */
LSDSORT_API int lsdsort_u32_ex(uint32_t* keys, size_t n, int radix_bits, int num_gpus);
/* The num_gpus > 1 code of lsdsort_u32_ex with `virtual_gpus` (1, 2, 4, 8) VIRTUAL ranks on the current device (loopback
 * transport, lsdsort_comm_create_loopback below): threads, set-up agreement, capacity retry, the step and the copy back run
 * as they would on a multi-GPU node.  A rehearsal entry for one-GPU machines; the result is the sorted array all the same. */
LSDSORT_API int lsdsort_u32_loopback(uint32_t* keys, size_t n, int radix_bits, int virtual_gpus);

/* Key/value form, stable by key (BASELINE.json configs[4]); no reference counterpart. */
LSDSORT_API int lsdsort_pairs_u32(uint32_t* keys, uint32_t* vals, size_t n);

/* ---- device-resident entries (the timed path) ---------------------------------------- */
/* Threads: every call keeps its state in the workspace it is given, so calls with different workspaces may run
 * concurrently from different host threads and on different streams; two calls sharing a workspace must be
 * ordered by the caller (same stream, or an event).  The tuning setters (lsdsort_set_*) are process-wide. */

/* Bytes of device workspace the device entries need for (n, radix_bits, pairs, algorithm); `pairs` = the number of 32-bit
 * payload arrays that travel with the keys: 0 keys only, 1 key/value pairs, 2 or 3 for lsdsort_multi_u32_device.
 * Replaces the reference's d_b + d_h + d_block_sums sizing, .cu:919-930 and
 * GetGPUPrefixSumBlockSumsCount .cu:265-276.  Returns 0 for invalid arguments.  The figure is
 * monotonic in n and covers every tile shape the library may pick for up to n keys: a workspace
 * made for n serves every smaller sort with the same (radix_bits, pairs, algorithm). */
LSDSORT_API size_t lsdsort_workspace_bytes(size_t n, int radix_bits, int pairs);
LSDSORT_API size_t lsdsort_workspace_bytes_ex(size_t n, int radix_bits, int pairs, int algorithm);
/* The workspace of a keys-only sort (default algorithm) with room for the hybrid form's HALF variant (lsdsort_set_half_hop):
 * lsdsort_workspace_bytes(n, radix_bits, 0), and where the variant can be attempted -- 8-bit digits, about 1.58e8 .. 3.3e8 keys
 * (the sizes sorted in 2^15 buckets), the default tile -- behind it 2 n bytes for the low halves of the keys (256-byte aligned),
 * 65536 words for the counts and 32768 words of bucket splits.  Everywhere else it equals lsdsort_workspace_bytes(n,
 * radix_bits, 0).  A sort given at least this much runs the variant where the device takes it; given less (the plain size
 * included) it runs exactly what it ran without.  The entries that take keys of other types, payloads, or a shard
 * (lsdsort_u32_device_prefixed) never run it. */
LSDSORT_API size_t lsdsort_workspace_bytes_roomy(size_t n, int radix_bits);

/* Replaces GPULSDRadixSort(a, b, h, block_sums, d, grid, block, ...), .cu:839-910: device
 * pointers, result in d_keys (the reference's `a`; the pass count is even), stream-ordered
 * on hip_stream (a hipStream_t; NULL = the null stream), does not synchronise.  The
 * workspace (256-byte aligned) holds the ping-pong buffer (`b`) and every table (`h`,
 * `block_sums`); nothing is allocated or freed inside, so the call can be graph-captured. */
LSDSORT_API int lsdsort_u32_device(uint32_t* d_keys, void* d_workspace, size_t workspace_bytes,
                                   size_t n, int radix_bits, void* hip_stream);
LSDSORT_API int lsdsort_pairs_u32_device(uint32_t* d_keys, uint32_t* d_vals, void* d_workspace,
                                         size_t workspace_bytes, size_t n, int radix_bits,
                                         void* hip_stream);
/* Keys with up to THREE 32-bit payload arrays (d_vals[0 .. num_vals-1], num_vals 1..3), each permuted exactly like the
 * keys, stable: the building block of the record sorts below (a 64-bit payload = two arrays; the other word of a 64-bit
 * key = one more).  The key/value kernel sends the arrays through the same LDS slots one after the other: 8 + 8 num_vals
 * bytes per key per pass.  Workspace: lsdsort_workspace_bytes(n, radix_bits, num_vals).  No reference counterpart (.cu:62). */
LSDSORT_API int lsdsort_multi_u32_device(uint32_t* d_keys, uint32_t* const* d_vals, int num_vals, void* d_workspace,
                                         size_t workspace_bytes, size_t n, int radix_bits, void* hip_stream);
/* Same with the pass structure chosen explicitly; d_vals may be NULL (keys only). */
LSDSORT_API int lsdsort_u32_device_ex(uint32_t* d_keys, uint32_t* d_vals, void* d_workspace,
                                      size_t workspace_bytes, size_t n, int radix_bits,
                                      int algorithm, void* hip_stream);

/* Keys of another 32-bit type or order (no reference counterpart: it sorts ascending uint32 only,
 * .cu:62).  The keys are mapped to order-preserving uint32 where they are first read
 * (upfront histogram, first pass) and mapped back where the last pass stores them: same passes, same
 * traffic as lsdsort_u32_device.  float32 sorts in IEEE total order (-NaN < -inf < ... < -0 < +0 < ... <
 * +inf < +NaN).  Descending = ascending on the complemented key; with payloads it is stable (equal keys
 * keep their input order).  d_vals may be NULL.  Chained algorithm, radix_bits 4 or 8. */
typedef enum lsdsort_key_type {
    LSDSORT_KEY_U32 = 0, LSDSORT_KEY_I32 = 1, LSDSORT_KEY_F32 = 2,
    /* 64-bit keys: lsdsort_keys64_device only; every 32-bit entry answers them with LSDSORT_ERR_INVALID_ARG */
    LSDSORT_KEY_U64 = 3, LSDSORT_KEY_I64 = 4, LSDSORT_KEY_F64 = 5
} lsdsort_key_type;
LSDSORT_API int lsdsort_keys_device(void* d_keys, uint32_t* d_vals, void* d_workspace, size_t workspace_bytes,
                                    size_t n, int radix_bits, int key_type, int descending, void* hip_stream);

/* 64-bit keys and 64-bit payloads (no reference counterpart, .cu:62), built on the 32-bit
 * pass kernels: an LSD sort on a 64-bit key is an LSD sort on its low word followed by a stable one on its
 * high word (lsdradixsort_amd/csrc/wide.hip).  Device pointers, in place, stream-ordered, nothing allocated.
 *   lsdsort_u64_device     : uint64 keys only.  Split into words, two key/value sorts (each word once the key,
 *                            once the payload), merge: 8 passes at radix 8, 16 B/key/pass.
 *   lsdsort_records_device : keys of key_bits (32 | 64) with payloads of val_bits (32 | 64; 32/32 is
 *                            lsdsort_pairs_u32_device), stable by key: every word that is not the key word being sorted on
 *                            rides through the passes as a payload array of its own (lsdsort_multi_u32_device); no gather.
 *                            A NULL d_vals is LSDSORT_ERR_INVALID_ARG and is reported BEFORE a bad workspace (the order of
 *                            lsdsort_keys64_device below and of the segmented and top-k entries; it used to come after).
 * lsdsort_wide_workspace_bytes(n, radix_bits, key_bits, val_bits) sizes the workspace (val_bits 0 = keys only);
 * lsdsort_wide_check_device reads the fault word of the sorts inside it (like lsdsort_check_device). */
LSDSORT_API size_t lsdsort_wide_workspace_bytes(size_t n, int radix_bits, int key_bits, int val_bits);
LSDSORT_API int lsdsort_u64_device(uint64_t* d_keys, void* d_workspace, size_t workspace_bytes, size_t n,
                                   int radix_bits, void* hip_stream);
LSDSORT_API int lsdsort_records_device(void* d_keys, void* d_vals, int key_bits, int val_bits, void* d_workspace,
                                       size_t workspace_bytes, size_t n, int radix_bits, void* hip_stream);
LSDSORT_API int lsdsort_wide_check_device(void* d_workspace, size_t n, int radix_bits, int key_bits, int val_bits,
                                          void* hip_stream);
/* 64-bit keys of another type or order, alone (val_bits 0, d_vals NULL) or with 32- or 64-bit payloads: key_type LSDSORT_KEY_U64,
 * _I64 or _F64 (a 32-bit key type is LSDSORT_ERR_INVALID_ARG), descending != 0 for the largest key first.  The keys are mapped to
 * the uint64 whose unsigned order is the requested one where they are split into words, and mapped back where the sorted words
 * are merged into d_keys -- the two kernels that touch every key once in any case: same passes, same traffic as
 * lsdsort_u64_device, and the sorts in between are plain uint32 sorts (pass skipping and the hybrid form included).  uint64: t = k;
 * int64: t = k ^ 2^63; float64: t = ~k for a negative key (ALL 64 bits), k ^ 2^63 otherwise -- IEEE total order, -NaN < -inf < ...
 * < -0 < +0 < ... < +inf < +NaN; descending: t = ~t afterwards, i.e. ascending on the complemented key, so it is stable as
 * well: equal keys keep their input order (what torch.sort(stable=True, descending=True) does).  Payloads are never mapped.
 * Workspace: lsdsort_wide_workspace_bytes(n, radix_bits, 64, val_bits); fault word: lsdsort_wide_check_device(ws, n, radix_bits,
 * 64, val_bits, stream).  d_keys 8-byte aligned (16-byte accesses are used where it is 16-byte aligned).  Stream-ordered, nothing
 * allocated, capturable in a graph (lsdsort_prepare_device first).  Checks, in order: key_type and val_bits (INVALID_ARG), n above
 * LSDSORT_MAX_KEYS (TOO_LARGE), radix_bits (INVALID_ARG), n == 0 (OK, nothing launched), a NULL d_keys, or a NULL d_vals with
 * val_bits != 0 (INVALID_ARG), the workspace (WORKSPACE), the device (NO_DEVICE).  lsdsort_u64_device and lsdsort_records_device
 * with key_bits 64 are this entry with (LSDSORT_KEY_U64, ascending).  NOT served: typed 32-bit keys with 64-bit payloads --
 * lsdsort_records_device(32, 64) stays uint32 ascending (the multi-payload pass kernel has no typed instantiation). */
LSDSORT_API int lsdsort_keys64_device(void* d_keys, void* d_vals, int val_bits /* 0 | 32 | 64 */, void* d_workspace,
                                      size_t workspace_bytes, size_t n, int radix_bits, int key_type, int descending,
                                      void* hip_stream);

/* 16-bit keys: uint16, int16, float16, bfloat16 (no reference counterpart, .cu:62; lsdradixsort_amd/csrc/keys16.hip).  In place,
 * stream-ordered, nothing allocated, no host synchronisation, every launch sized from n alone: capturable in a graph
 * (lsdsort_prepare_device first).  The sortable 16-bit value t of key k: uint16 t = k; int16 t = k ^ 0x8000; float16 and bfloat16
 * (one map: both are sign-magnitude; the two enumerators are kept apart so that callers say what they have) t = ~k where the sign
 * bit is set, k ^ 0x8000 otherwise -- IEEE total order, -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN; descending: t = ~t
 * afterwards.  The map is applied where a key is read; the raw key is what is stored.
 *   d_vals == NULL : keys only.  A 16-bit key has 65536 values, so from a measured size on (the automatic rule) the sort is a
 *                    COUNT of the values into 65536 counters, a scan of the counters and a FILL of d_keys with runs: one read of
 *                    the keys per half of the value range and one write, no key is moved (equal 16-bit keys are the same bits).
 *                    Smaller sorts take the widen route below.
 *   d_vals given   : the 32-bit payloads are permuted with the keys, stable in either direction (equal keys keep their input
 *                    order).  WIDEN route: the keys are mapped to uint32 with t in the low half-word, lsdsort_pairs_u32_device
 *                    (keys only: lsdsort_u32_device) runs on them inside this call's workspace -- its pass skipping drops the two
 *                    dead high passes on the device, the payloads are sorted where they lie -- and one kernel narrows and un-maps.
 * d_keys needs 2-byte alignment only: 16-byte accesses are used from the first 16-byte line on, the keys in front of it and behind
 * the last whole line go one by one.  Checks, in order, each before a device is touched: key_type (INVALID_ARG), n above
 * LSDSORT_MAX_KEYS (TOO_LARGE), n == 0 (OK, nothing launched), a NULL (or odd) d_keys (INVALID_ARG), the workspace (WORKSPACE: NULL,
 * not 256-byte aligned, or below lsdsort_keys16_workspace_bytes(n, d_vals != NULL)), the device (NO_DEVICE).
 * lsdsort_keys16_workspace_bytes is a multiple of 256, monotonic in n, covers BOTH routes (a workspace serves whichever the library
 * picks) and is 0 for pairs outside {0, 1} or n above the limit.
 * lsdsort_set_keys16_route: -1 the automatic rule (default), 0 always widen, 1 count wherever it applies (keys only); process-wide
 * like the other setters, anything else is INVALID_ARG.  It exists so that both routes can be tested at small sizes.
 * lsdsort_keys16_check_device reads the call's fault word -- set by the fill kernel where the scanned total is not n, or taken over
 * from the sort inside the widen route -- and synchronises the stream. */
typedef enum lsdsort_key16_type {
    LSDSORT_KEY16_U16 = 0, LSDSORT_KEY16_I16 = 1, LSDSORT_KEY16_F16 = 2, LSDSORT_KEY16_BF16 = 3
} lsdsort_key16_type;
LSDSORT_API size_t lsdsort_keys16_workspace_bytes(size_t n, int pairs /* 0 | 1 */);
LSDSORT_API int lsdsort_keys16_device(void* d_keys, uint32_t* d_vals, void* d_workspace, size_t workspace_bytes, size_t n,
                                      int key_type, int descending, void* hip_stream);
LSDSORT_API int lsdsort_keys16_check_device(void* d_workspace, size_t n, int pairs, void* hip_stream);
LSDSORT_API int lsdsort_set_keys16_route(int route);   /* -1 auto (default), 0 widen, 1 count */

/* Segmented sort (no reference counterpart; the counterpart of DeviceSegmentedRadixSort and of torch.sort(x, dim=-1) on rows).
 * Segment s = keys[d_offsets[s] .. d_offsets[s+1]) for s < num_segments; each segment is sorted in place,
 * independently, stable; d_vals (may be NULL) is permuted with the keys.  d_offsets: num_segments + 1 ascending
 * uint32 device words, d_offsets[num_segments] <= n; keys outside [d_offsets[0], d_offsets[num_segments]) are
 * not touched.  key_type / descending as lsdsort_keys_device (0 uint32, 1 int32, 2 float32 IEEE total order).
 * Stream-ordered, no host synchronisation, capturable in a graph: every launch is sized from (n, num_segments).
 * A planner kernel sorts the segments into three size classes on the device: up to 1024 keys one wavefront each, up to
 * 16384 one workgroup's LDS each (both skip every 8-bit digit that is the same in all keys of the segment), larger ones
 * four staged passes over tiles that never cross a segment (lsdradixsort_amd/csrc/segmented.hip).  Where the returning-add
 * rank form is not in force (lsdsort_set_rank_method) every segment takes the staged passes: same result, slower.
 * Offsets are checked on the device: a segment whose end is below its start or beyond n is left untouched, the call still
 * returns LSDSORT_OK, and lsdsort_check_device(d_workspace, stream) then returns LSDSORT_ERR_DEVICE_FAULT.  Nothing outside
 * [0, n) is ever read or written.  Segments that overlap one another (possible only around such a pair) come out in an
 * unspecified order.  Checks, in order: key_type (INVALID_ARG), n or num_segments above LSDSORT_MAX_KEYS (TOO_LARGE), a NULL
 * d_keys or d_offsets with n > 0 or num_segments > 0 (INVALID_ARG), n == 0 or num_segments == 0 (OK, nothing launched), the
 * workspace (WORKSPACE: NULL, not 256-byte aligned, or below lsdsort_segmented_workspace_bytes), the device (NO_DEVICE).
 * lsdsort_segmented_workspace_bytes is monotonic in n and num_segments and returns 0 above LSDSORT_MAX_KEYS. */
LSDSORT_API size_t lsdsort_segmented_workspace_bytes(size_t n, size_t num_segments, int pairs);
LSDSORT_API int lsdsort_segmented_device(void* d_keys, uint32_t* d_vals, const uint32_t* d_offsets,
                                         size_t num_segments, size_t n, int key_type, int descending,
                                         void* d_workspace, size_t workspace_bytes, void* hip_stream);

/* Top-k selection (no reference counterpart; the counterpart of torch.topk(x, k, dim=-1, sorted=True) and of a radix-select
 * entry).  d_keys: rows x cols 32-bit keys, row-major, READ ONLY.  Row r's result is the first k items of the STABLE sort of
 * the row in the requested order (key_type as lsdsort_keys_device: 0 uint32, 1 int32, 2 float32 IEEE total order; largest != 0 =
 * descending = ascending on the complemented key): d_out_keys[r * k + j], j < k, best first, in the caller's key type, and
 * d_out_idx[r * k + j] its position within the row (d_out_idx may be NULL: values only).  Equal keys come out in position order,
 * and of the duplicates of the k-th value those at the lowest positions are selected: the result equals the row's full stable
 * sort cut to k columns, bit for bit, on every run.  rows = 1 is the whole-array case.
 * The row is not sorted: a most-significant-digit-first radix select counts digits (rows of up to 1024 keys in one wavefront,
 * up to 16384 in one workgroup's LDS, longer ones by many workgroups with at most five reads of the row and no write but the
 * winners), the winners are written in position order and only those rows x k items are sorted (lsdradixsort_amd/csrc/topk.hip).
 * Where k is above three quarters of cols the rows are copied into the workspace and sorted whole instead: same result.
 * Stream-ordered, no host synchronisation, nothing allocated; every launch is sized from (rows, cols, k): capturable in a graph.
 * lsdsort_check_device(d_workspace, stream) reports the call's fault word (never expected to be set).
 * Checks, in order: key_type (INVALID_ARG), rows * cols or rows above LSDSORT_MAX_KEYS (TOO_LARGE), k > cols (INVALID_ARG),
 * rows == 0, cols == 0 or k == 0 (OK, nothing launched), a NULL d_keys or d_out_keys (INVALID_ARG), the workspace (WORKSPACE:
 * NULL, not 256-byte aligned, or below lsdsort_topk_workspace_bytes), the device (NO_DEVICE).
 * lsdsort_topk_workspace_bytes is a multiple of 256, monotonic in each argument and 0 above the limits (rows * cols, rows * k or
 * any argument above LSDSORT_MAX_KEYS).  It is O(rows * k) -- the winners' sort, and the sort route's copy, which only a call with
 * cols < 4 k / 3 can take -- plus 16 B per row, and for rows above 16384 keys 8 KiB of counters per row and 8 B per 16384 keys. */
LSDSORT_API size_t lsdsort_topk_workspace_bytes(size_t rows, size_t cols, size_t k);
LSDSORT_API int lsdsort_topk_device(const void* d_keys, size_t rows, size_t cols, size_t k, int key_type, int largest,
                                    void* d_out_keys, uint32_t* d_out_idx, void* d_workspace, size_t workspace_bytes,
                                    void* hip_stream);

/* Top-k selection for 16-bit keys (lsdradixsort_amd/csrc/topk16.hip): lsdsort_topk_device's contract, word for word, with the key
 * types of lsdsort_keys16_device (lsdsort_key16_type; float16 and bfloat16 in IEEE total order; largest != 0 = ascending on the
 * complemented sortable value).  d_keys: rows x cols 16-bit keys, row-major, READ ONLY.  Row r's result is the first k items of the
 * STABLE sort of the row in the requested order: d_out_keys[r * k + j], j < k, best first, 16-bit words in the caller's key type,
 * and d_out_idx[r * k + j] its position within the row (d_out_idx may be NULL: values only, and no position is written anywhere
 * the caller can see).  Equal keys come out in position order, and of the duplicates of the k-th value those at the lowest
 * positions are selected; the result is identical on every run and under graph replay.
 * d_keys and d_out_keys need 2-byte alignment only and cols may be odd: every row is read by 16-byte loads of eight keys from ITS
 * first 16-byte line on, the keys in front of that line and behind the row's last whole line one by one.
 * The row is not sorted: a counting radix select of at most TWO digit levels (rows of up to 1024 keys in one wavefront, up to 16384
 * in one workgroup, two rounds of 8-bit digits; longer rows by many workgroups, 11 bits then 5, at most four reads of the row --
 * 8 B/key -- and nothing written but the winners), an ordered write of the winners into the workspace, a segmented sort of those
 * rows x k items alone (none for k = 1), and one kernel that narrows them into the outputs.  Where k is above three quarters of
 * cols the rows are widened into the workspace and sorted whole instead: same result (the 3/4 is the 32-bit entry's, not tuned for
 * 2-byte keys).  Stream-ordered, no host synchronisation, nothing allocated; every launch is sized from (rows, cols, k):
 * capturable in a graph after lsdsort_prepare_device.  The fault word is the first word of the workspace:
 * lsdsort_check_device(d_workspace, stream) reports it (never expected to be set).
 * Checks, in order, each before a device is touched: key_type (INVALID_ARG), rows or rows * cols above LSDSORT_MAX_KEYS
 * (TOO_LARGE), k > cols (INVALID_ARG), rows == 0, cols == 0 or k == 0 (OK, nothing launched), a NULL or odd d_keys or d_out_keys
 * (INVALID_ARG), the workspace (WORKSPACE: NULL, not 256-byte aligned, or below lsdsort_topk16_workspace_bytes), the device
 * (NO_DEVICE).  lsdsort_topk16_workspace_bytes is a multiple of 256, monotonic in each argument, 0 above the limits (rows * cols,
 * rows * k or any argument above LSDSORT_MAX_KEYS), sized for the call with indices, and covers both routes. */
LSDSORT_API size_t lsdsort_topk16_workspace_bytes(size_t rows, size_t cols, size_t k);
LSDSORT_API int lsdsort_topk16_device(const void* d_keys, size_t rows, size_t cols, size_t k, int key_type /* lsdsort_key16_type */,
                                      int largest, void* d_out_keys /* [rows][k] 16-bit, caller's type */,
                                      uint32_t* d_out_idx /* [rows][k] or NULL */, void* d_workspace, size_t workspace_bytes,
                                      void* hip_stream);

/* Stable sort of every row of 16-bit keys, with positions (lsdradixsort_amd/csrc/rows16.hip; the counterpart of
 * torch.sort(x, dim=-1, stable=True) on [batch x vocab] float16 / bfloat16 logits).  d_keys: rows x cols 16-bit keys, row-major.
 * Row r of d_out_keys is the STABLE sort of row r of d_keys in the requested order (key types and key map of
 * lsdsort_keys16_device: lsdsort_key16_type, float16 and bfloat16 in IEEE total order; descending != 0 = ascending on the
 * complemented sortable value), and d_out_idx[r * cols + j] the position within the row of the key now at column j (d_out_idx may
 * be NULL: keys only, and no position is written anywhere the caller can see).  Equal keys come out in position order, in either
 * direction; the result is identical on every run and under graph replay.
 * d_out_keys may be d_keys itself (in place); any other overlap is the caller's error and is not checked; d_keys is otherwise only
 * read.  d_keys and d_out_keys need 2-byte alignment only and cols may be odd: rows are read and written by 16-byte accesses of
 * eight keys from a 16-byte line on, the keys in front of it and behind the last whole group one by one.
 * The host chooses the route by cols.  Rows of up to 1024 keys are sorted by one wavefront each, up to 16384 by one workgroup each:
 * the row is read once into LDS as words of (sortable key << 16 | position), sorted there by at most two 8-bit digit passes (a byte
 * that is the same in every key of the row is no pass) and stored -- no key is widened through memory.  Rows of up to
 * LSDSORT_ROWS16_NATIVE_MAX_COLS keys take two global passes (low byte, high byte) over tiles of 8192 row positions: per pass a
 * histogram kernel, a scan per row and a scatter kernel; pass 1 leaves a uint32 key and a uint32 position per item in the workspace.
 * Longer rows, and every row where the returning-add rank form is not in force (lsdsort_set_rank_method), take the WIDEN route: the
 * keys go to the workspace as sortable uint32 words with their positions, lsdsort_segmented_device sorts the pairs with the rows as
 * segments, one kernel un-maps and narrows.  Same result on every route.
 * Stream-ordered, no host synchronisation, nothing allocated; every launch is sized from (rows, cols): capturable in a graph after
 * lsdsort_prepare_device.  Phases are ordered by kernel boundaries.  The fault word is the first word of the workspace:
 * lsdsort_check_device(d_workspace, stream) reports it (never expected to be set); every store into the outputs is guarded
 * against its row.
 * Checks, in order, each before a device is touched: key_type (INVALID_ARG), rows or rows * cols above LSDSORT_MAX_KEYS
 * (TOO_LARGE), rows == 0 or cols == 0 (OK, nothing launched), a NULL or odd d_keys or d_out_keys (INVALID_ARG), the workspace
 * (WORKSPACE: NULL, not 256-byte aligned, or below lsdsort_rows16_workspace_bytes), the device (NO_DEVICE).
 * lsdsort_rows16_workspace_bytes is a multiple of 256, monotonic in each argument, 0 above the limits (rows, cols or rows * cols
 * above LSDSORT_MAX_KEYS), sized for the call with indices, and covers BOTH routes whatever the route setting says.
 * lsdsort_set_rows16_route: -1 by size (default), 0 always the widen route, 1 native wherever it exists; process-wide like the other
 * setters, anything else is INVALID_ARG. */
#define LSDSORT_ROWS16_NATIVE_MAX_COLS 262144   /* rows longer than this take the widen route */
LSDSORT_API size_t lsdsort_rows16_workspace_bytes(size_t rows, size_t cols);
LSDSORT_API int lsdsort_rows16_device(const void* d_keys, size_t rows, size_t cols, int key_type /* lsdsort_key16_type */,
                                      int descending, void* d_out_keys /* [rows][cols] 16-bit; may be d_keys itself */,
                                      uint32_t* d_out_idx /* [rows][cols] or NULL */, void* d_workspace, size_t workspace_bytes,
                                      void* hip_stream);
LSDSORT_API int lsdsort_set_rows16_route(int route);   /* -1 by size (default), 0 always the widen route, 1 native wherever it exists */

/* K-th value selection: ONE order statistic per row, no sort (lsdradixsort_amd/csrc/kth.hip; the counterpart of
 * torch.kthvalue(x, k, dim=-1), torch.median(x, dim=-1) and the `lower` / `higher` / `nearest` forms of torch.quantile).
 * d_keys: rows x cols 32-bit keys, row-major, READ ONLY; it needs 4-byte alignment only and cols may be anything: every row is read
 * by 16-byte loads of four keys from ITS first 16-byte line on, the keys in front of that line and behind the row's last whole
 * group one by one.  Let S_r be the STABLE sort of row r in the requested order (key_type as lsdsort_keys_device: 0 uint32, 1 int32,
 * 2 float32 IEEE total order; largest != 0 = descending = ascending on the complemented key, so equal keys keep their position order
 * in either direction).  d_out_keys[r] = S_r[rank] (rank is 0-based), in the caller's key type, and d_out_idx[r] the position within
 * the row of that same item -- among the duplicates of the value the one the stable sort puts at `rank`, not "some occurrence"
 * (d_out_idx may be NULL: values only).  The result equals column `rank` of lsdsort_topk_device(.., k = rank + 1, ..), bit for bit,
 * values and positions; it is identical on every run and under graph replay.  rows = 1 is the whole-array case.
 * The row is not sorted and no winner is written: a most-significant-digit-first radix select counts digits until ONE key is left
 * under the prefix or all 32 bits are fixed (rows of up to 1024 keys in one wavefront, up to 16384 in one workgroup: one read of the
 * row; longer ones by many workgroups, digits of 11, 11 and 10 bits), then the wanted key is located among the keys of that value in
 * position order (long rows: one count pass, then ONE chunk is read again): at most four reads of a long row plus one chunk, and
 * nothing written but counters and 8 B per row.
 * Stream-ordered, no host synchronisation, nothing allocated; every launch is sized from (rows, cols) alone: capturable in a graph
 * after lsdsort_prepare_device.  Counters and row states are zeroed by a kernel of the call; phases are ordered by kernel boundaries.
 * The fault word is the first word of the workspace: lsdsort_check_device(d_workspace, stream) reports it -- set where a row's digit
 * counts do not reach the rank or no key is located (neither is expected).  The result does not depend on lsdsort_set_rank_method.
 * Checks, in order, each before a device is touched: key_type outside U32 / I32 / F32 (INVALID_ARG), rows or rows * cols above
 * LSDSORT_MAX_KEYS (TOO_LARGE), rows == 0 or cols == 0 (OK, nothing launched -- before the rank: an empty row has no valid rank),
 * rank >= cols (INVALID_ARG), a NULL d_keys or d_out_keys or either not 4-byte aligned (INVALID_ARG), the workspace (WORKSPACE:
 * NULL, not 256-byte aligned, or below lsdsort_kth_workspace_bytes), the device (NO_DEVICE).
 * lsdsort_kth_workspace_bytes is a multiple of 256, monotonic in each argument, 0 where rows, cols or rows * cols is above
 * LSDSORT_MAX_KEYS, and does not depend on the rank.  It is O(rows), never O(rows * cols): the control block, 16 B per row, and for
 * rows above 16384 keys 8 KiB of counters per row and 4 B per 16384 keys. */
LSDSORT_API size_t lsdsort_kth_workspace_bytes(size_t rows, size_t cols);
LSDSORT_API int lsdsort_kth_device(const void* d_keys, size_t rows, size_t cols, size_t rank /* 0-based */,
                                   int key_type /* lsdsort_key_type: U32, I32, F32 */, int largest,
                                   void* d_out_keys /* [rows], caller's type */, uint32_t* d_out_idx /* [rows] or NULL */,
                                   void* d_workspace, size_t workspace_bytes, void* hip_stream);

/* Multi-rank k-th value selection: SEVERAL order statistics of every row in one call (lsdradixsort_amd/csrc/kth_multi.hip) --
 * quartiles, a set of percentiles, the two clipping thresholds of a row, and the two adjacent order statistics floor(q (n - 1)) and
 * ceil(q (n - 1)) that an interpolating quantile (torch.quantile's `linear` and `midpoint`) is made of.
 * `ranks` is a HOST array of num_ranks (at most LSDSORT_KTH_MAX_RANKS) 0-based ranks, each below cols, in any order, repeats
 * allowed; it is copied into the launches (as the splitters of lsdsort_splitter_partition_u32_device are), so it is fixed in a
 * captured graph.  d_out_keys[r * num_ranks + j] and d_out_idx[r * num_ranks + j] are exactly what
 * lsdsort_kth_device(.., rank = ranks[j], ..) stores for row r -- item ranks[j] of the row's STABLE sort in the requested order and
 * the position of that very item, values and positions bit for bit; slot j is defined by ranks[j] alone.  d_out_idx may be NULL:
 * values only, and no position is written anywhere the caller can see.  Everything else is lsdsort_kth_device's contract: d_keys is
 * READ ONLY and needs 4-byte alignment only, cols may be anything, key_type U32 / I32 / F32 (IEEE total order), largest != 0 =
 * ascending on the complemented key; the result is identical on every run and under graph replay.
 * The reads of the row are shared by the ranks.  Rows of up to 1024 keys (one wavefront) and up to 16384 (one workgroup) are loaded
 * into registers once and every rank selects and locates there: one read of the row, one launch.  Longer rows: the first digit level
 * is ONE histogram per row that every rank walks; at the two later levels each key is tested against the prefixes of the ranks still
 * open, and ranks that share a prefix are counted once; one count pass serves every rank; then each rank reads its ONE chunk again.
 * At most four reads of a long row plus num_ranks chunks, in the ten launches of the single-rank call.
 * Stream-ordered, no host synchronisation, nothing allocated; every launch is sized from (rows, cols, num_ranks) alone: capturable
 * in a graph after lsdsort_prepare_device.  Control block, counters and states are zeroed by a kernel of the call; phases are
 * ordered by kernel boundaries.  The fault word is the first word of the workspace: lsdsort_check_device(d_workspace, stream)
 * reports it -- bit 1024 where a row's digit counts do not reach a rank, bit 2048 where no key is located (neither is expected).
 * The result does not depend on lsdsort_set_rank_method.
 * Checks, in order, each before a device is touched: key_type outside U32 / I32 / F32 (INVALID_ARG), num_ranks above
 * LSDSORT_KTH_MAX_RANKS (INVALID_ARG), rows, rows * cols or rows * num_ranks above LSDSORT_MAX_KEYS (TOO_LARGE), rows == 0,
 * cols == 0 or num_ranks == 0 (OK, nothing launched), a NULL `ranks` or any ranks[j] >= cols (INVALID_ARG), a NULL d_keys or
 * d_out_keys or either not 4-byte aligned (INVALID_ARG), the workspace (WORKSPACE: NULL, not 256-byte aligned, or below
 * lsdsort_kth_multi_workspace_bytes), the device (NO_DEVICE).
 * lsdsort_kth_multi_workspace_bytes is a multiple of 256, monotonic in each argument, 0 above the limits and for num_ranks above
 * LSDSORT_KTH_MAX_RANKS, and depends neither on the rank values nor on d_out_idx.  It is O(rows * num_ranks), never O(rows * cols):
 * the control block, 16 B per row and rank, and for rows above 16384 keys 8 KiB of counters per row and rank and 4 B per 16384 keys
 * and rank. */
#define LSDSORT_KTH_MAX_RANKS 8
LSDSORT_API size_t lsdsort_kth_multi_workspace_bytes(size_t rows, size_t cols, size_t num_ranks);
LSDSORT_API int lsdsort_kth_multi_device(const void* d_keys, size_t rows, size_t cols,
                                         const size_t* ranks /* HOST array, num_ranks entries, 0-based */, size_t num_ranks,
                                         int key_type /* lsdsort_key_type: U32, I32, F32 */, int largest,
                                         void* d_out_keys /* [rows][num_ranks], caller's type */,
                                         uint32_t* d_out_idx /* [rows][num_ranks] or NULL */, void* d_workspace,
                                         size_t workspace_bytes, void* hip_stream);

/* K-th value selection for 16-bit keys (lsdradixsort_amd/csrc/kth16.hip; the median, a percentile or a clipping threshold of
 * float16 / bfloat16 rows without a conversion to float32): lsdsort_kth_device's contract, word for word, with the key types of
 * lsdsort_keys16_device (lsdsort_key16_type; float16 and bfloat16 in IEEE total order; largest != 0 = ascending on the complemented
 * sortable value).  d_keys: rows x cols 16-bit keys, row-major, READ ONLY.  Let S_r be the STABLE sort of row r in the requested
 * order.  d_out_keys[r] = S_r[rank] (rank is 0-based), a 16-bit word in the caller's key type, and d_out_idx[r] the position within
 * the row of that same item -- among the duplicates of the value the one the stable sort puts at `rank` (d_out_idx may be NULL:
 * values only, and no position is written anywhere the caller can see).  The result equals column `rank` of
 * lsdsort_topk16_device(.., k = rank + 1, ..), bit for bit, values and positions; it is identical on every run and under graph
 * replay.  rows = 1 is the whole-array case.
 * d_keys and d_out_keys need 2-byte alignment only and cols may be odd: every row is read by 16-byte loads of eight keys from ITS
 * first 16-byte line on, the keys in front of that line and behind the row's last whole group one by one.
 * The row is not sorted and no winner is written: a counting radix select of at most TWO digit levels stops where ONE key is left
 * under the prefix or all 16 bits are fixed (rows of up to 1024 keys in one wavefront, up to 16384 in one workgroup, two rounds of
 * 8-bit digits: one read of the row; longer ones by many workgroups, 11 bits then 5), then the wanted key is located among the keys
 * of that value in position order (long rows: one count pass, then ONE chunk is read again): at most three reads of a long row plus
 * one chunk -- 6 B/key by byte accounting, not measured -- and nothing written but counters and 6 B per row.  With d_out_idx == NULL a long row needs no locate: both
 * levels run, the prefix is the value and one small kernel stores it -- two reads of the row.
 * Stream-ordered, no host synchronisation, nothing allocated; every launch is sized from (rows, cols) and from whether d_out_idx
 * was given: capturable in a graph after lsdsort_prepare_device.  Counters and row states are zeroed by a kernel of the call; phases
 * are ordered by kernel boundaries.  The fault word is the first word of the workspace: lsdsort_check_device(d_workspace, stream)
 * reports it -- set where a row's digit counts do not reach the rank or no key is located (neither is expected).  The result does
 * not depend on lsdsort_set_rank_method.
 * Checks, in order, each before a device is touched: key_type outside lsdsort_key16_type (INVALID_ARG), rows or rows * cols above
 * LSDSORT_MAX_KEYS (TOO_LARGE), rows == 0 or cols == 0 (OK, nothing launched -- before the rank: an empty row has no valid rank),
 * rank >= cols (INVALID_ARG), a NULL or odd d_keys or d_out_keys (INVALID_ARG), the workspace (WORKSPACE: NULL, not 256-byte
 * aligned, or below lsdsort_kth16_workspace_bytes), the device (NO_DEVICE).
 * lsdsort_kth16_workspace_bytes is a multiple of 256, monotonic in each argument, 0 where rows, cols or rows * cols is above
 * LSDSORT_MAX_KEYS, and depends neither on the rank nor on d_out_idx.  It is O(rows), never O(rows * cols): the control block, 16 B
 * per row, and for rows above 16384 keys 8 KiB of counters per row and 4 B per 16384 keys. */
LSDSORT_API size_t lsdsort_kth16_workspace_bytes(size_t rows, size_t cols);
LSDSORT_API int lsdsort_kth16_device(const void* d_keys, size_t rows, size_t cols, size_t rank /* 0-based */,
                                     int key_type /* lsdsort_key16_type */, int largest,
                                     void* d_out_keys /* [rows] 16-bit, caller's type */, uint32_t* d_out_idx /* [rows] or NULL */,
                                     void* d_workspace, size_t workspace_bytes, void* hip_stream);

/* Multi-rank k-th value selection for 16-bit keys: SEVERAL order statistics of every row in one call
 * (lsdradixsort_amd/csrc/kth16_multi.hip) -- the quartiles, a set of percentiles or the clipping thresholds of float16 / bfloat16
 * rows, and the two adjacent order statistics an interpolating quantile is made of, without a conversion to float32.  It is to
 * lsdsort_kth16_device what lsdsort_kth_multi_device is to lsdsort_kth_device.
 * `ranks` is a HOST array of num_ranks (at most LSDSORT_KTH_MAX_RANKS) 0-based ranks, each below cols, in any order, repeats
 * allowed; it is copied into the launches, so it is fixed in a captured graph.  d_out_keys[r * num_ranks + j] and
 * d_out_idx[r * num_ranks + j] are exactly what lsdsort_kth16_device(.., rank = ranks[j], ..) stores for row r -- item ranks[j] of
 * the row's STABLE sort in the requested order and the position of that very item, values and positions bit for bit; slot j is
 * defined by ranks[j] alone.  d_out_idx may be NULL: values only, and no position is written anywhere the caller can see.
 * Everything else is lsdsort_kth16_device's contract: d_keys is READ ONLY; d_keys and d_out_keys need 2-byte alignment only and cols
 * may be odd; the key types are lsdsort_key16_type (float16 and bfloat16 in IEEE total order; largest != 0 = ascending on the
 * complemented sortable value); the result is identical on every run and under graph replay.
 * The reads of the row are shared by the ranks.  Rows of up to 1024 keys (one wavefront) and up to 16384 (one workgroup) are loaded
 * into registers once and every rank selects and locates there: one read of the row, one launch after the clear.  Longer rows: the
 * first digit level (11 bits) is ONE histogram per row in which every rank finds its bin; at the second (5 bits) each key is tested
 * against the prefixes of the ranks still open, and ranks that share a prefix share 32 counters; one count pass serves every rank;
 * then each rank reads its ONE chunk again: at most three reads of a long row plus num_ranks chunks, in eight launches.  With
 * d_out_idx == NULL a long row needs no locate: both levels run for every rank, the prefix is the value and one small kernel stores
 * it -- two reads of the row (4 B/key by byte accounting) in six launches, whatever num_ranks.
 * Stream-ordered, no host synchronisation, nothing allocated; every launch is sized from (rows, cols, num_ranks) and from whether
 * d_out_idx was given: capturable in a graph after lsdsort_prepare_device.  Control block, counters and states are zeroed by a
 * kernel of the call; phases are ordered by kernel boundaries.  The fault word is the first word of the workspace:
 * lsdsort_check_device(d_workspace, stream) reports it -- bit 1024 where a row's digit counts do not reach a rank, bit 2048 where
 * nothing is located or a values-only state is not a whole value (neither is expected).  The result does not depend on
 * lsdsort_set_rank_method.
 * Checks, in order, each before a device is touched: key_type outside lsdsort_key16_type (INVALID_ARG), num_ranks above
 * LSDSORT_KTH_MAX_RANKS (INVALID_ARG), rows, rows * cols or rows * num_ranks above LSDSORT_MAX_KEYS (TOO_LARGE), rows == 0,
 * cols == 0 or num_ranks == 0 (OK, nothing launched), a NULL `ranks` or any ranks[j] >= cols (INVALID_ARG), a NULL or odd d_keys or
 * d_out_keys (INVALID_ARG), the workspace (WORKSPACE: NULL, not 256-byte aligned, or below lsdsort_kth16_multi_workspace_bytes), the
 * device (NO_DEVICE).
 * lsdsort_kth16_multi_workspace_bytes is a multiple of 256, monotonic in each argument, 0 above the limits and for num_ranks above
 * LSDSORT_KTH_MAX_RANKS, and depends neither on the rank values nor on d_out_idx.  It is O(rows * num_ranks), never O(rows * cols):
 * the control block, 16 B per row and rank, and for rows above 16384 keys 8 KiB of counters per ROW, 128 B of counters per row and
 * rank and 4 B per 16384 keys and rank.  It need not equal lsdsort_kth16_workspace_bytes at num_ranks = 1. */
LSDSORT_API size_t lsdsort_kth16_multi_workspace_bytes(size_t rows, size_t cols, size_t num_ranks);
LSDSORT_API int lsdsort_kth16_multi_device(const void* d_keys, size_t rows, size_t cols,
                                           const size_t* ranks /* HOST array, num_ranks entries, 0-based */, size_t num_ranks,
                                           int key_type /* lsdsort_key16_type */, int largest,
                                           void* d_out_keys /* [rows][num_ranks] 16-bit, caller's type */,
                                           uint32_t* d_out_idx /* [rows][num_ranks] or NULL */, void* d_workspace,
                                           size_t workspace_bytes, void* hip_stream);

/* K-th value selection for 16-bit keys with a rank of its own for EVERY row, read from device memory
 * (lsdradixsort_amd/csrc/kth16_rowk.hip): lsdsort_kth16_device's contract, word for word, with one change -- row r uses
 * d_ranks[r], a DEVICE array of `rows` 0-based ranks (4-byte aligned) that a kernel of the call reads.  For every row with
 * d_ranks[r] < cols, d_out_keys[r] and d_out_idx[r] are exactly what lsdsort_kth16_device(.., rank = d_ranks[r], ..) stores for that
 * row, bit for bit: item d_ranks[r] of the row's STABLE sort in the requested order and the position of that very item, the float
 * types in IEEE total order, largest != 0 = ascending on the complemented sortable value.  d_keys is READ ONLY; d_keys and d_out_keys
 * need 2-byte alignment only and cols may be odd; d_out_idx may be NULL (values only).
 * The host never reads d_ranks and NO value in it sizes a launch: every launch is sized from (rows, cols) and from whether d_out_idx
 * was given.  Changing the contents of d_ranks between replays of a captured graph changes the result accordingly -- a batch of
 * requests with mixed ranks is one call, and a decode loop that replays a graph follows a changed rank without a recapture (the
 * host ranks of lsdsort_kth16_device and of the multi-rank entries are fixed in a captured graph).
 * A rank outside its row cannot be refused by the host (as the offsets of lsdsort_segmented_device cannot): a row with
 * d_ranks[r] >= cols has NOTHING stored for it in either output, the call still returns LSDSORT_OK, bit 4096 -- and only that bit --
 * is set in the fault word (the first word of the workspace), lsdsort_check_device(d_workspace, stream) then reports
 * LSDSORT_ERR_DEVICE_FAULT, and every other row of the call is correct.  A flag in a software word; nothing faults.  Bits 1024 (a
 * row's digit counts do not reach the rank) and 2048 (no key is located) are lsdsort_kth16_device's and never expected.
 * Kernels: lsdsort_kth16_device's three size classes (rows of up to 1024 keys one wavefront, up to 16384 one workgroup: one read of
 * the row; longer ones by many workgroups: at most three reads plus one chunk, two reads without d_out_idx).  Stream-ordered, no host
 * synchronisation, nothing allocated; capturable after lsdsort_prepare_device; phases are ordered by kernel boundaries.  The result
 * does not depend on lsdsort_set_rank_method.
 * Checks, in order, each before a device is touched: key_type outside lsdsort_key16_type (INVALID_ARG), rows or rows * cols above
 * LSDSORT_MAX_KEYS (TOO_LARGE), rows == 0 or cols == 0 (OK, nothing launched), a NULL or odd d_keys or d_out_keys (INVALID_ARG), a
 * NULL d_ranks or one that is not 4-byte aligned (INVALID_ARG), the workspace (WORKSPACE: NULL, not 256-byte aligned, or below
 * lsdsort_kth16_perrow_workspace_bytes), the device (NO_DEVICE).
 * lsdsort_kth16_perrow_workspace_bytes is a multiple of 256, monotonic in each argument, 0 where rows, cols or rows * cols is above
 * LSDSORT_MAX_KEYS, and depends neither on the ranks nor on d_out_idx.  It is O(rows), never O(rows * cols): the control block, 16 B
 * per row, and for rows above 16384 keys 8 KiB of counters per row and 4 B per 16384 keys. */
LSDSORT_API size_t lsdsort_kth16_perrow_workspace_bytes(size_t rows, size_t cols);
LSDSORT_API int lsdsort_kth16_perrow_device(const void* d_keys, size_t rows, size_t cols,
                                            const uint32_t* d_ranks /* DEVICE, [rows], 0-based */,
                                            int key_type /* lsdsort_key16_type */, int largest,
                                            void* d_out_keys /* [rows] 16-bit, caller's type */, uint32_t* d_out_idx /* [rows] or NULL */,
                                            void* d_workspace, size_t workspace_bytes, void* hip_stream);

/* Top-k FILTER for 16-bit rows with a k of its own for every row, read from device memory (lsdradixsort_amd/csrc/kth16_rowk.hip):
 * the last step of top-k sampling over [batch x vocab] float16 / bfloat16 logits, "keep the k_r best logits of request r, set the
 * rest to -inf" -- logits.masked_fill_(logits < kth, -inf) with the k-th value selected and applied in one call.
 * d_k is a DEVICE array of `rows` uint32 (4-byte aligned); let k_r = d_k[r].  If k_r == 0 or k_r >= cols the filter is OFF for the
 * row: row r of d_out is row r of d_keys (the serving convention; an int32 -1 reads as 0xFFFFFFFF, which is also off).  Otherwise let
 * T_r be item k_r - 1 of the row's STABLE sort in the requested order (largest != 0: the k_r-th largest): d_out[r][p] = d_keys[r][p]
 * where the key is at least as good as T_r -- sortable(key) <= sortable(T_r) under the map of the 16-bit entries -- and fill_bits
 * elsewhere.  EVERY duplicate of the threshold value is kept, so a row keeps at least k_r keys; kept keys are copied bit for bit.
 * The comparison is the library's total order, not IEEE's `<`: -0.0 ranks below +0.0 (with largest, a threshold of +0.0 fills the
 * -0.0s), and NaNs sort by sign at the two ends (+NaN above +inf, -NaN below -inf) instead of comparing false.
 * d_out may be d_keys itself (in place); any other overlap is the caller's error and is not checked.  d_keys and d_out need 2-byte
 * alignment only, their alignments may differ from each other, and cols may be odd.  There is no bad-argument flag: every value of
 * d_k means something.  The host never reads d_k and no value in it sizes a launch: capturable after lsdsort_prepare_device, and d_k
 * is read again on every replay.
 * Kernels: rows of up to 1024 keys (one wavefront) and up to 16384 (one workgroup) are loaded into registers once, selected there,
 * and the same registers are compared and stored: one read and one write of the row (4 B/key by byte accounting).  Longer rows: the
 * values-only select of lsdsort_kth16_device (two reads), then one kernel reads every tile again, compares and stores: 8 B/key.  Rows
 * whose filter is off skip the select; they are copied, or not touched at all in place.  Stores are 16-byte groups where a row of
 * d_out has the 16-byte phase of its row of d_keys (always in place), key by key otherwise.
 * Stream-ordered, no host synchronisation, nothing allocated; phases are ordered by kernel boundaries; every store stays within its
 * row.  The fault word is the first word of the workspace: bit 1024 where a row's digit counts do not reach k_r (never expected;
 * nothing is stored for the row).  The result does not depend on lsdsort_set_rank_method.
 * Checks, in order, each before a device is touched: key_type outside lsdsort_key16_type (INVALID_ARG), rows or rows * cols above
 * LSDSORT_MAX_KEYS (TOO_LARGE), rows == 0 or cols == 0 (OK, nothing launched), a NULL or odd d_keys or d_out, a NULL d_k or one that
 * is not 4-byte aligned (INVALID_ARG), the workspace (WORKSPACE: NULL, not 256-byte aligned, or below
 * lsdsort_topk16_filter_workspace_bytes), the device (NO_DEVICE).
 * lsdsort_topk16_filter_workspace_bytes is a multiple of 256, monotonic in each argument, 0 above the limits, independent of d_k,
 * and O(rows): the control block, 16 B per row, and for rows above 16384 keys 8 KiB of counters per row. */
LSDSORT_API size_t lsdsort_topk16_filter_workspace_bytes(size_t rows, size_t cols);
LSDSORT_API int lsdsort_topk16_filter_device(const void* d_keys, size_t rows, size_t cols, const uint32_t* d_k /* DEVICE, [rows] */,
                                             int key_type /* lsdsort_key16_type */, int largest, uint16_t fill_bits,
                                             void* d_out /* [rows][cols] 16-bit; may be d_keys itself */, void* d_workspace,
                                             size_t workspace_bytes, void* hip_stream);

/* Top-p (nucleus) FILTER for float16 / bfloat16 rows with a p of its own for every row, read from device memory
 * (lsdradixsort_amd/csrc/topp16.hip): "keep the smallest set of best logits whose softmax mass reaches p_r, set the rest to -inf",
 * without a sort.  key_type is LSDSORT_KEY16_F16 or LSDSORT_KEY16_BF16; the order is always "largest is best" in the library's total
 * order: -0.0 below +0.0, +NaN above +inf, -NaN below -inf.
 * d_p is a DEVICE array of `rows` float32 (4-byte aligned); let p = d_p[r].  If !(p < 1) -- p >= 1 or a NaN -- the filter is OFF for
 * the row: row r of d_out is row r of d_keys (left alone in place).  Otherwise, in exact arithmetic: m is the largest non-NaN key of
 * the row by value; w(x) is 0 for a NaN, 1 where x == m (which also defines rows whose maximum is an infinity) and exp(x - m)
 * elsewhere; Z is the sum of w over the row; A(x) the sum of w over the keys strictly better than x in the library's order.  Key x
 * is KEPT iff A(x) < p * Z or x is the best value of the row.  So p <= 0 keeps the best value and its duplicates alone, a row always
 * keeps at least one key, every duplicate of a kept value is kept.  Kept keys are copied bit for bit, the others become fill_bits.
 * The kept set is "every key at least as good as a threshold value T_r".  The device works in float32 and truncated fixed point
 * (w by v_exp_f32, masses floor(w * 2^32) summed as 64-bit integers), so T_r is specified to a mass tolerance: it is consistent with
 * p_r +- 2^-12 for |logit| <= 64 and cols <= 2^17; given T_r the output is exact.  The result is DETERMINISTIC: integer sums do not
 * depend on the order of the adds, so the same row and p give the same bits on every call, whatever the other rows and `rows`.
 * Composition: w(-inf) = 0, so lsdsort_topk16_filter_device(fill_bits = -inf) followed by this entry, both in place, is "top-k,
 * then top-p over the renormalised survivors".
 * d_out may be d_keys itself (in place); any other overlap is the caller's error and is not checked.  d_keys and d_out need 2-byte
 * alignment only, their alignments may differ from each other, and cols may be odd.  There is no bad-argument flag: every value of
 * d_p means something.  The host never reads d_p and no value in it sizes a launch: capturable after lsdsort_prepare_device, and d_p
 * is read again on every replay, so a captured decode graph follows a changed top_p.
 * Kernels: rows of up to 1024 keys (one wavefront) and up to 16384 (one workgroup) are loaded into registers once, the threshold is
 * found there by a 16-step bisection over the masses, and the same registers are compared and stored: one read and one write of the
 * row (4 B/key by byte accounting).  Longer rows: the best key, a 2048-bin mass histogram and a 32-bin count histogram (three
 * reads), then one kernel reads every tile again, compares and stores: 10 B/key.  Rows whose filter is off skip the select.
 * Stream-ordered, no host synchronisation, nothing allocated; phases are ordered by kernel boundaries; every store stays within its
 * row.  The fault word is the first word of the workspace: bit 1024 where nothing was selected for a row (never expected; nothing
 * is stored for the row).  The result does not depend on lsdsort_set_rank_method.
 * Checks, in order, each before a device is touched: key_type other than float16 / bfloat16 (INVALID_ARG), rows or rows * cols above
 * LSDSORT_MAX_KEYS (TOO_LARGE), rows == 0 or cols == 0 (OK, nothing launched), a NULL or odd d_keys or d_out, a NULL d_p or one that
 * is not 4-byte aligned (INVALID_ARG), the workspace (WORKSPACE: NULL, not 256-byte aligned, or below
 * lsdsort_topp16_filter_workspace_bytes), the device (NO_DEVICE).
 * lsdsort_topp16_filter_workspace_bytes is a multiple of 256, monotonic in each argument, 0 above the limits, independent of d_p,
 * and O(rows): lsdsort_topk16_filter_workspace_bytes, and for rows above 16384 keys 16 KiB of mass bins per row on top of it. */
LSDSORT_API size_t lsdsort_topp16_filter_workspace_bytes(size_t rows, size_t cols);
LSDSORT_API int lsdsort_topp16_filter_device(const void* d_keys, size_t rows, size_t cols, const float* d_p /* DEVICE, [rows] */,
                                             int key_type /* float16 or bfloat16 */, uint16_t fill_bits,
                                             void* d_out /* [rows][cols] 16-bit; may be d_keys itself */, void* d_workspace,
                                             size_t workspace_bytes, void* hip_stream);

/* The top-p filter with a TEMPERATURE and a MIN-P of its own for every row (the same kernels of topp16.hip; DESIGN.md section
 * 6.16).  d_p, d_min_p and d_temperature are DEVICE arrays of `rows` float32 (4-byte aligned) and each of them may be NULL.
 * Temperature T = d_temperature[r]; NULL: 1 for every row.  The weights of lsdsort_topp16_filter_device become w(x) = 0 for a NaN, 1
 * where x == m, exp((x - m) / T) elsewhere: the device takes exp2((x - m) * c) with c = log2(e) / T computed in float64 and rounded
 * to float32.  T above 2^64 (+inf) acts as 2^64, so a -inf under a finite maximum has no mass at ANY temperature.  !(T > 0) -- zero,
 * a negative T, a NaN -- and a T so small that c overflows mean GREEDY: the maximum's duplicates alone have mass, and a select that
 * is on (p < 1) keeps the best value alone.  T = 1 gives the literal log2(e) of the entry above: a NULL d_temperature, an array of
 * ones and lsdsort_topp16_filter_device give the SAME BITS.  Every value of T means something.
 * Top-p, p = d_p[r] as above under these weights; a NULL d_p, like !(p < 1), is OFF.
 * Min-p, mp = d_min_p[r]: NULL or !(mp > 0) -- zero, a negative mp, a NaN -- is OFF.  Otherwise theta = value(m) + T ln(mp), for a
 * greedy row theta = value(m), and the min-p threshold is the worst value of the library's order that is a number with
 * value >= theta, never worse than m: "keep the keys whose probability is at least mp times the best key's".  So mp >= 1 keeps the
 * best number's duplicates (and the +NaNs above them: as in the top-p filter every key at least as good as the threshold is kept),
 * -0.0 is kept when theta == 0, and a row without a number keeps its best key value alone.  theta is float32: logf, then one fused
 * multiply-add, within B = 2^-22 * (|value(m)| + |T ln mp|) of the exact value; given theta the output is exact.
 * A key is KEPT iff it is at least as good as the STRICTER of the two thresholds.  The ratio to the maximum does not change under
 * renormalisation, so this is "top-p, then min-p over the survivors" and equally the other order.  A row where both are off is
 * copied (left alone in place); a row with top-p off and min-p on skips the mass select and needs its best number only.
 * Tolerance of the top-p threshold: the mass tolerance 2^-12 above, for |logit| <= 64, cols <= 2^17 and T greedy or >= 2^-10.
 * Alignment, in place, capture, determinism, the fault word and the kernels are those of lsdsort_topp16_filter_device: the host
 * reads none of the three arrays, no launch is sized from them, and all three are read again on every replay of a captured graph.
 * Long rows without d_p: the kernel that clears the row states reads 4 * rows bytes of d_keys in d_p's place and ignores them.
 * Checks, in order, each before a device is touched: key_type (INVALID_ARG), rows or rows * cols above LSDSORT_MAX_KEYS (TOO_LARGE),
 * rows == 0 or cols == 0 (OK, nothing launched), a NULL or odd d_keys or d_out, then a d_p, d_min_p or d_temperature that is not
 * 4-byte aligned (INVALID_ARG), the workspace (WORKSPACE; lsdsort_topp16_filter_workspace_bytes), the device (NO_DEVICE). */
LSDSORT_API int lsdsort_topp16_filter_ex_device(const void* d_keys, size_t rows, size_t cols, const float* d_p /* DEVICE, [rows], or NULL: off */,
                                                const float* d_min_p /* DEVICE, [rows], or NULL: off */,
                                                const float* d_temperature /* DEVICE, [rows], or NULL: 1 */,
                                                int key_type /* float16 or bfloat16 */, uint16_t fill_bits,
                                                void* d_out /* [rows][cols] 16-bit; may be d_keys itself */, void* d_workspace,
                                                size_t workspace_bytes, void* hip_stream);

/* The DRAW of a sampling step for float16 / bfloat16 rows, one token per row, with a uniform u of its own for every row read from
 * device memory (lsdradixsort_amd/csrc/sample16.hip): the inverse CDF of the row's softmax in POSITION order, without a select, a
 * sort or a float32 copy of the row.  key_type is LSDSORT_KEY16_F16 or LSDSORT_KEY16_BF16.
 * Weights, those of lsdsort_topp16_filter_device: m is the largest non-NaN key of the row by value; w(x) is 0 for a NaN, 1 where
 * x == m (which also defines rows whose maximum is an infinity) and exp(x - m) elsewhere; Z is the sum of w over the row; C_i the sum
 * of w over the positions j < i.  d_u is a DEVICE array of `rows` float32 (4-byte aligned); with u = d_u[r], row r stores into
 * d_index[r] the position i with C_i <= u * Z < C_i + w_i.  A key of zero mass is never drawn: a NaN, and a -inf under a finite
 * maximum -- what the filters write.  Composition: lsdsort_topk16_filter_device and lsdsort_topp16_filter_device (fill_bits = -inf,
 * in place) followed by this entry are "top-k, top-p, sample over the renormalised survivors" with no further code.  A row of -inf
 * alone draws uniformly from its keys (x == m).  A row that holds no number (Z == 0) stores index -1 and logprob NaN and raises no
 * flag: that is data, not a fault.
 * Arithmetic actually used: q(x) = floor(w(x) * 2^32) as uint64 with w in float32 by v_exp_f32 -- the SAME device functions as the
 * top-p filter, so a value has one mass in the filter and in the draw --, Z and C integer sums of q (Z < 2^62).  G = 0 where
 * !(u > 0) (zero, a negative u, a NaN), else G = min(Z - 1, (uint64)floor((double)u * (double)Z)), so u >= 1 draws the last key of
 * non-zero q; the result is the i with C_i <= G < C_i + q_i.  Tolerance, for |logit| <= 64 and cols <= 2^17: the drawn index is
 * consistent with u +- 2^-12 of the row's mass (the top-p filter's budget: the masses are the same and the float64 product adds
 * nothing visible).  The result is DETERMINISTIC: integer sums do not depend on the chunking, on the order of the atomics or on the
 * other rows, so the same (row, u) gives the same index on every call, in any batch, at any `rows`, in every size class.
 * d_logprob (optional, NULL: none) receives (x_i - m) - ln(Z * 2^-32) in float32, the log-probability of the drawn key under the
 * row's softmax -- only this entry knows Z --, within 2^-11 absolute of float64 under the conditions above.
 * The host never reads d_u and no value in it sizes a launch: capturable after lsdsort_prepare_device, and d_u and the keys are read
 * again on every replay, so a captured decode graph follows changed u and changed keys.
 * d_keys is READ ONLY, needs 2-byte alignment only, and cols may be odd.  Stores go to d_index[r] and d_logprob[r], r < rows, only.
 * Kernels: rows of up to 1024 keys (one wavefront) and up to 16384 (one workgroup) are loaded into registers once: the maximum by an
 * integer reduction, q per register, a 64-bit exclusive scan in position order, and the one lane whose range holds G stores: one read
 * of the row (2 B/key by byte accounting).  Longer rows: the best number per chunk (integer atomicMin), the sum of q per chunk (one
 * plain 64-bit store per chunk, every chunk on every call), Z, G and the chunk that holds G per row, then one workgroup per row reads
 * that one chunk up to the crossing: two reads plus one chunk, about 4 B/key.
 * Stream-ordered, no host synchronisation, nothing allocated; phases are ordered by kernel boundaries.  The fault word is the first
 * word of the workspace: bit 1024 where no key was located for a row that has mass (never expected; nothing is stored for the row).
 * The result does not depend on lsdsort_set_rank_method.
 * Checks, in order, each before a device is touched: key_type other than float16 / bfloat16 (INVALID_ARG), rows or rows * cols above
 * LSDSORT_MAX_KEYS (TOO_LARGE), rows == 0 or cols == 0 (OK, nothing launched), a NULL or odd d_keys (INVALID_ARG), a NULL d_u or
 * d_index or one that is not 4-byte aligned (INVALID_ARG), a non-NULL d_logprob that is not 4-byte aligned (INVALID_ARG), the
 * workspace (WORKSPACE: NULL, not 256-byte aligned, or below lsdsort_sample16_workspace_bytes), the device (NO_DEVICE).
 * lsdsort_sample16_workspace_bytes is a multiple of 256, monotonic in each argument, 0 above the limits, independent of d_u and
 * d_logprob, and O(rows): the control block, 16 B per row, and for rows above 16384 keys 8 B per 16384 keys of a row. */
LSDSORT_API size_t lsdsort_sample16_workspace_bytes(size_t rows, size_t cols);
LSDSORT_API int lsdsort_sample16_device(const void* d_keys, size_t rows, size_t cols, const float* d_u /* DEVICE, [rows] */,
                                        int key_type /* float16 or bfloat16 */, int32_t* d_index /* [rows] */,
                                        float* d_logprob /* [rows], or NULL */, void* d_workspace, size_t workspace_bytes,
                                        void* hip_stream);

/* The draw with a TEMPERATURE of its own for every row (the same kernels of sample16.hip): d_temperature is
 * a DEVICE array of `rows` float32 (4-byte aligned), or NULL for T = 1 in every row, with the meaning and the arithmetic of
 * lsdsort_topp16_filter_ex_device -- the same device function gives a key its mass in the filter and in the draw.  A greedy row --
 * !(T > 0), or a T so small that log2(e) / T overflows -- draws the argmax, uniformly over its duplicates by u: the j-th of `ties`
 * duplicates in position order with j = floor(u * ties).  A -inf under a finite maximum has no mass at any T, so what the filters
 * write is never drawn.  d_logprob receives the log-probability under the TEMPERED softmax, (x_i - m) * c * ln 2 - ln(Z * 2^-32)
 * with 0 for the first term where x_i == m, within 2^-11 + 2^-22 * |(x_i - m) / T| of float64; for T = 1 the factor c * ln 2 is taken
 * as 1.  A NULL d_temperature, an array of ones and lsdsort_sample16_device give the SAME BITS in d_index and d_logprob.  Index
 * tolerance: 2^-12 of the row's mass for |logit| <= 64, cols <= 2^17 and T greedy or >= 2^-10.  Everything else -- u, alignment,
 * capture (d_temperature is read again on every replay), determinism, kernels, the fault word, the workspace figure -- is
 * lsdsort_sample16_device's.  Checks, in order: those of lsdsort_sample16_device, a d_temperature that is not 4-byte aligned
 * (INVALID_ARG) together with d_logprob's. */
LSDSORT_API int lsdsort_sample16_ex_device(const void* d_keys, size_t rows, size_t cols, const float* d_u /* DEVICE, [rows] */,
                                           const float* d_temperature /* DEVICE, [rows], or NULL: 1 */,
                                           int key_type /* float16 or bfloat16 */, int32_t* d_index /* [rows] */,
                                           float* d_logprob /* [rows], or NULL */, void* d_workspace, size_t workspace_bytes,
                                           void* hip_stream);

/* LOG-PROBABILITIES and RANKS of GIVEN tokens of float16 / bfloat16 logit rows (lsdradixsort_amd/csrc/logprob16.hip; DESIGN.md
 * section 6.17): what a server returns next to the token -- `logprobs` / `top_logprobs`, the rank of the sampled token, prompt
 * log-probabilities, the forward of a cross-entropy loss -- without a float32 copy of the row.  d_ids is a DEVICE array of
 * rows * slots int32 (4-byte aligned), 1 <= slots <= LSDSORT_LOGPROB_MAX_SLOTS; slot s of row r asks for key i = d_ids[r * slots + s]
 * of row r, with value x.  key_type is LSDSORT_KEY16_F16 or LSDSORT_KEY16_BF16.
 * Masses: m, c = log2(e) / T_r, w, q = floor(w * 2^32) and the integer sum Z are exactly those of lsdsort_sample16_ex_device, from the
 * same device functions; d_temperature as there (NULL: 1 in every row; !(T > 0) or a T so small that c overflows: GREEDY).
 * d_logprob[r * slots + s] = (x == m ? 0 : (x - m) * c * ln 2) - ln(Z * 2^-32) in float32, the factor taken as 1 for T = 1: the
 * expression the draw stores, in its order.  Called on the index the draw returned, with the same keys and temperature, this entry
 * gives THE BITS of the draw's d_logprob, in every size class.  A -inf under a finite maximum gives exactly -inf; a greedy row gives
 * -ln(ties) on the maximum's duplicates and -inf elsewhere; a NaN key gives NaN; a row without a number (Z == 0) gives NaN in every
 * slot.  Tolerance, for |logit| <= 64, cols <= 2^17 and T greedy or >= 2^-10: within 2^-11 + 2^-22 * |(x - m) / T| of float64.
 * d_rank (optional, NULL: none): d_rank[r * slots + s] is the number of keys of row r that are numbers and strictly greater than x BY
 * VALUE, (row.float() > x).sum(): NaNs count for nothing, -0.0 and +0.0 are equal, the maximum and all its ties have rank 0.  -1 where
 * x is a NaN.  Exact, and independent of the temperature.
 * d_lse (optional, NULL: none): d_lse[r] = value(m) * c * ln 2 + ln(Z * 2^-32), the log-sum-exp of the tempered row, within
 * 2^-11 + 2^-22 * |m / T| of float64 under the conditions above; NaN for a greedy row and for a row without a number, +inf / -inf
 * where m is an infinity.
 * An id below 0 or at or above cols is PADDING: its slot stores logprob NaN and rank -1 and raises no flag -- data, not a fault; a
 * ragged top-n is padded with -1.  Every word of the three outputs is written on every call.  This entry sets no fault bit: it clears
 * the control block, so lsdsort_check_device answers OK.
 * The host reads neither d_ids nor d_temperature and no launch is sized from them: capturable after lsdsort_prepare_device, and ids,
 * temperatures and keys are read again on every replay of a captured graph.  d_keys is READ ONLY, needs 2-byte alignment only, and
 * cols may be odd.  Stores go to the three outputs under r < rows only.  The result is DETERMINISTIC: integer sums and counts do not depend on the chunking, on
 * the order of the atomics or on the other rows; the same row, ids and T give the same bits in any batch and any size class.
 * Kernels: rows of up to 1024 keys (one wavefront) and up to 16384 (one workgroup) are loaded into registers once, behind the loads of
 * the row's ids and of the keys they name: the maximum by an integer reduction, Z by an integer sum, per slot the queried key broadcast
 * and the better keys counted by ballot and popcount; lane s stores slot s: one read of the row (2 B/key by byte accounting).  Longer
 * rows, launches sized from (rows, cols, slots, whether d_rank was given): the best number per chunk (integer atomicMin), the sum of q
 * per chunk (one plain 64-bit store per chunk, every chunk on every call) with the per-slot counts (integer atomicAdd), and one
 * wavefront per row that finishes: two reads, 4 B/key.  Stream-ordered, no host synchronisation, nothing allocated; phases are ordered
 * by kernel boundaries.  The result does not depend on lsdsort_set_rank_method.
 * Checks, in order, each before a device is touched: key_type other than float16 / bfloat16 (INVALID_ARG), slots 0 or above
 * LSDSORT_LOGPROB_MAX_SLOTS (INVALID_ARG), rows or rows * cols above LSDSORT_MAX_KEYS (TOO_LARGE), rows == 0 or cols == 0 (OK, nothing
 * launched), a NULL or odd d_keys (INVALID_ARG), a NULL d_ids or d_logprob or one that is not 4-byte aligned (INVALID_ARG), a non-NULL
 * d_rank, d_lse or d_temperature that is not 4-byte aligned (INVALID_ARG), the workspace (WORKSPACE: NULL, not 256-byte aligned, or
 * below lsdsort_logprob16_workspace_bytes), the device (NO_DEVICE).
 * lsdsort_logprob16_workspace_bytes is a multiple of 256, monotonic in each argument, 0 above the limits and for a bad `slots`,
 * independent of which optional outputs are given, and O(rows * slots): the control block, 4 B per row, and for rows above 16384 keys
 * 8 B per 16384 keys of a row and 4 B per slot. */
#define LSDSORT_LOGPROB_MAX_SLOTS 32
LSDSORT_API size_t lsdsort_logprob16_workspace_bytes(size_t rows, size_t cols, size_t slots);
LSDSORT_API int lsdsort_logprob16_device(const void* d_keys, size_t rows, size_t cols, const int32_t* d_ids /* DEVICE, [rows][slots] */,
                                         size_t slots, const float* d_temperature /* DEVICE, [rows], or NULL: 1 */,
                                         int key_type /* float16 or bfloat16 */, float* d_logprob /* [rows][slots] */,
                                         int32_t* d_rank /* [rows][slots], or NULL */, float* d_lse /* [rows], or NULL */,
                                         void* d_workspace, size_t workspace_bytes, void* hip_stream);

/* Run-length encode and unique for 32- and 64-bit keys (no reference counterpart, .cu:62; lsdradixsort_amd/csrc/unique.hip, DESIGN.md
 * section 6.18): the distinct keys of an array and how often each occurs -- torch.unique_consecutive, torch.unique(sorted=True),
 * np.unique(return_index / return_inverse / return_counts), group-by, deduplication of ids.  Both entries are device-resident and
 * stream-ordered, allocate nothing and never synchronise with the host; EVERY LAUNCH IS SIZED FROM n ALONE -- the number of runs is
 * known on the device only and sizes nothing.  GRAPH CAPTURE: both entries launch kernels only and clear or rewrite every word of
 * state they read on every call; either can be captured after lsdsort_prepare_device and replayed any number of times on changed
 * keys, in the same workspace.  No workgroup of the run-length phases waits for another: they are ordered by kernel boundaries.
 * EQUALITY IS EQUALITY OF BIT PATTERNS, which matches the sorts' total order: -0.0 and +0.0 are two values and every NaN payload is a
 * value of its own.  torch.unique and torch.unique_consecutive compare floats by value (they merge -0.0 with +0.0 and keep every NaN
 * apart); on integer keys, and on floats that hold no -0.0 next to a +0.0 and no NaN, the results are the same.
 *
 * lsdsort_rle_device: run-length encode of d_keys AS IT LIES, sorted or not: torch.unique_consecutive(return_counts=True).  Run j is a
 * maximal stretch of equal adjacent words of key_bits (32 | 64); d_out_keys[j] is its word, d_out_starts[j] the position of its first
 * element, d_out_counts[j] its length, *d_num_runs (a DEVICE word) the number of runs.  d_out_counts and d_out_starts may each be
 * NULL.  Words at index >= *d_num_runs of every output are NOT WRITTEN.  d_keys is READ ONLY and needs the alignment of its word only
 * (16-byte loads where it starts on a 16-byte line).  d_out_keys == d_keys is INVALID_ARG; any other overlap is the caller's error.
 * Kernels: count the run heads of every tile of 4096 keys (head(i) = i == 0 || key[i] != key[i-1]) | one workgroup scans the tile
 * counts, carries the last head forward and stores the total | every tile ranks its heads and stores word and start of each run at
 * its rank, and every head stores the length of the run before it (the last run's comes from the scan): no array of starts is
 * written and read again for the counts.  Two reads of the keys.  The fault word, the first word of the workspace
 * (lsdsort_check_device), is set where the scanned total is 0 or above n -- never expected; nothing is stored then.
 *
 * lsdsort_unique_device: the distinct keys of d_keys in the library's order for key_type (all six of lsdsort_key_type: ascending, or
 * the largest first with descending != 0), d_out_counts[j] how often value j occurs, d_out_first[j] the LOWEST input position that
 * holds it, d_out_inverse[i] the j with d_out_keys[j] == d_keys[i], *d_num_unique (a DEVICE word) their number; the three arrays may
 * each be NULL.  The entry copies the keys into the workspace -- after that copy d_keys is no longer read, so d_out_keys MAY BE d_keys
 * itself -- writes the positions 0..n-1 beside the copy where d_out_first or d_out_inverse is given (`with_positions` of the
 * workspace figure and of the check), sorts the copy with lsdsort_keys_device / lsdsort_keys64_device (8-bit digits, the positions as
 * a 32-bit payload) inside a sub-range of its workspace, and runs the run-length kernels over the sorted copy.  The sorts are stable,
 * so the head of every run carries the lowest input position; inverse[pos[i]] = (run heads at sorted positions <= i) - 1, every
 * position written exactly once: the same bits on every call.  Words at index >= *d_num_unique of keys, counts and first are not
 * written.  Workspace: control block (fault word first) | key copy | positions | the sort's workspace | per-tile head counts | per-tile last heads,
 * each 256-byte aligned.  lsdsort_unique_check_device synchronises the stream and answers LSDSORT_ERR_DEVICE_FAULT where the unit's
 * own word is set or the check of the sort inside (lsdsort_check_device / lsdsort_wide_check_device on its sub-range) reports one.
 *
 * Checks of both entries, in order, each before a device is touched: key_bits / key_type (INVALID_ARG), n above LSDSORT_MAX_KEYS
 * (TOO_LARGE), n == 0 (OK: *d_num_* receives 0 by one stream-ordered 4-byte store where the pointer is given -- the one thing an empty
 * call does, and the one that needs the device -- and nothing else happens), a NULL d_keys, d_out_keys or d_num_*, keys or output keys
 * not aligned to their word, a 32-bit output that is not 4-byte aligned (INVALID_ARG), the workspace (WORKSPACE: NULL, not 256-byte
 * aligned, or below the figure), the device (NO_DEVICE).  The workspace functions return a multiple of 256, are monotonic in n, cover
 * every combination of optional outputs (with_positions: d_out_first or d_out_inverse is given; never smaller than without) and
 * return 0 above the limit or for a bad key_bits / key_type. */
LSDSORT_API size_t lsdsort_rle_workspace_bytes(size_t n, int key_bits);
LSDSORT_API int lsdsort_rle_device(const void* d_keys, size_t n, int key_bits /* 32 | 64 */,
                                   void* d_out_keys /* [n] words of key_bits */, uint32_t* d_out_counts /* [n] or NULL */,
                                   uint32_t* d_out_starts /* [n] or NULL */, uint32_t* d_num_runs /* DEVICE, one word */,
                                   void* d_workspace, size_t workspace_bytes, void* hip_stream);
LSDSORT_API size_t lsdsort_unique_workspace_bytes(size_t n, int key_type, int with_positions);
LSDSORT_API int lsdsort_unique_device(const void* d_keys, size_t n, int key_type /* lsdsort_key_type, all six */, int descending,
                                      void* d_out_keys /* [n], caller's type; may be d_keys itself */,
                                      uint32_t* d_out_counts /* [n] or NULL */,
                                      uint32_t* d_out_first /* [n] or NULL: lowest input position holding value j */,
                                      uint32_t* d_out_inverse /* [n] or NULL: d_out_keys[d_out_inverse[i]] == d_keys[i] */,
                                      uint32_t* d_num_unique /* DEVICE, one word */, void* d_workspace, size_t workspace_bytes,
                                      void* hip_stream);
LSDSORT_API int lsdsort_unique_check_device(void* d_workspace, size_t n, int key_type, int with_positions, void* hip_stream);

/* Reduce by key: the sum, minimum or maximum of a 32-bit value array per run and per distinct key, for 32- and 64-bit keys (no reference
 * counterpart, .cu:62; lsdradixsort_amd/csrc/reduce_by_key.hip) -- thrust::reduce_by_key, segment sums of
 * gradients per embedding id, the best score per document id; what index_add_ / scatter_reduce_ on unique's inverse map do with
 * atomics.  Both entries are device-resident and stream-ordered, allocate nothing and never synchronise with the host; EVERY LAUNCH IS
 * SIZED FROM n ALONE.  GRAPH CAPTURE: both entries launch kernels only (no memset) and clear or rewrite every word of state they read
 * on every call; either can be captured after lsdsort_prepare_device and replayed any number of times on changed keys and values, in
 * the same workspace.  No workgroup of the three phases waits for another: they are ordered by kernel boundaries.  Keys are equal
 * where their BIT PATTERNS are, as in lsdsort_rle_device.
 *
 * VALUES AND OPERATIONS.  val_type says how the 32-bit value words are read (lsdsort_val_type), op what is taken over a run
 * (lsdsort_reduce_op).  SUM of U32 / I32 is arithmetic mod 2^32.  MIN / MAX of U32 / I32 are unsigned / signed.  MIN / MAX of F32 are
 * taken in the library's float TOTAL ORDER, the map lsdsort_keys_device sorts float32 by: -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf
 * < +NaN; the result is always the bits of one of the run's values, and equals amin / amax wherever the run holds no NaN.  SUM of F32
 * is IEEE float32 addition in an order FIXED BY THE POSITIONS ALONE: the same input gives the same bits on every call, eager or
 * replayed.  A run of one element returns that element's bits, -0.0 and NaN payloads included: no identity element is ever added to a
 * value.  The order is not the sequential one -- a run is summed as a tree over (16-byte group, wavefront, lane, word) of its tiles of
 * 4096 keys, tile after tile -- so the result differs from a left-to-right sum by rounding: for a run of L values
 * |result - exact| <= g * sum|v| with g = (L-1)u / (1 - (L-1)u), u = 2^-24, the bound of every summation order.
 *
 * lsdsort_reduce_runs_device: the runs of d_keys AS IT LIES, sorted or not (torch.unique_consecutive plus a segment reduce).  Run j is
 * a maximal stretch of equal adjacent words of key_bits (32 | 64); d_out_keys[j] is its word, d_out_vals[j] the aggregate of its
 * values, d_out_counts[j] (may be NULL) its length, *d_num_runs (a DEVICE word) the number of runs.  Words at index >= *d_num_runs of
 * every output are NOT WRITTEN.  d_keys and d_vals are READ ONLY and need the alignment of their word only (16-byte loads where an
 * array starts on a 16-byte line).  d_out_keys == d_keys or d_out_vals == d_vals is INVALID_ARG: the inputs are read while the runs
 * are stored; any other overlap is the caller's error.  Kernels: every tile of 4096 keys counts its run heads and folds its values
 * from its last head on | one workgroup scans the tile counts and carries the open run's aggregate and head from tile to tile, and
 * stores the last run's aggregate and length | every tile ranks its heads and folds its values in position order; every head stores
 * the aggregate and the length of the run before it.  Two reads of keys and values.  The fault word, the first word of the workspace
 * (lsdsort_check_device), is set where the scanned total or last head is 0 or above n -- never expected; nothing is stored then.
 *
 * lsdsort_reduce_by_key_device: the same per DISTINCT key of unsorted input, in the library's order for key_type (all six of
 * lsdsort_key_type: ascending, or the largest first with descending != 0); *d_num_groups (a DEVICE word) their number.  The entry
 * copies keys and values into the workspace -- after that copy the inputs are no longer read, so d_out_keys MAY BE d_keys and
 * d_out_vals MAY BE d_vals -- sorts the copies with lsdsort_keys_device / lsdsort_keys64_device (8-bit digits, the value bits as the
 * 32-bit payload) inside a sub-range of its workspace, and runs the three phases over the sorted copies.  The sort is stable, so the
 * values of a group meet the reduction IN INPUT ORDER.  Workspace: control block (fault word first) | key copy | value copy | the
 * sort's workspace | per-tile head counts | per-tile open-run heads | per-tile open-run aggregates, each 256-byte aligned.
 * lsdsort_reduce_by_key_check_device synchronises the stream and answers LSDSORT_ERR_DEVICE_FAULT where the unit's own word is set or
 * the check of the sort inside (lsdsort_check_device / lsdsort_wide_check_device on its sub-range) reports one.
 *
 * Checks of both entries, in order, each before a device is touched: key_bits / key_type, val_type, op (INVALID_ARG), n above
 * LSDSORT_MAX_KEYS (TOO_LARGE), n == 0 (OK: *d_num_* receives 0 by one stream-ordered 4-byte store where the pointer is given, and
 * nothing else happens), a NULL d_keys, d_vals, d_out_keys, d_out_vals or d_num_*, an array not aligned to its word (INVALID_ARG), the
 * forbidden aliases of the runs entry (INVALID_ARG), the workspace (WORKSPACE: NULL, not 256-byte aligned, or below the figure), the
 * device (NO_DEVICE).  The workspace functions return a multiple of 256, are monotonic in n and return 0 above the limit or for a bad
 * key_bits / key_type. */
typedef enum lsdsort_reduce_op { LSDSORT_REDUCE_SUM = 0, LSDSORT_REDUCE_MIN = 1, LSDSORT_REDUCE_MAX = 2 } lsdsort_reduce_op;
typedef enum lsdsort_val_type { LSDSORT_VAL_U32 = 0, LSDSORT_VAL_I32 = 1, LSDSORT_VAL_F32 = 2 } lsdsort_val_type;
LSDSORT_API size_t lsdsort_reduce_runs_workspace_bytes(size_t n, int key_bits);
LSDSORT_API int lsdsort_reduce_runs_device(const void* d_keys, const void* d_vals /* [n], 32-bit */, size_t n, int key_bits /* 32 | 64 */,
                                           int val_type /* lsdsort_val_type */, int op /* lsdsort_reduce_op */,
                                           void* d_out_keys /* [n] words of key_bits */, void* d_out_vals /* [n], 32-bit */,
                                           uint32_t* d_out_counts /* [n] or NULL */, uint32_t* d_num_runs /* DEVICE, one word */,
                                           void* d_workspace, size_t workspace_bytes, void* hip_stream);
LSDSORT_API size_t lsdsort_reduce_by_key_workspace_bytes(size_t n, int key_type);
LSDSORT_API int lsdsort_reduce_by_key_device(const void* d_keys, const void* d_vals /* [n], 32-bit */, size_t n,
                                             int key_type /* lsdsort_key_type, all six */, int descending, int val_type, int op,
                                             void* d_out_keys /* [n], caller's type; may be d_keys itself */,
                                             void* d_out_vals /* [n], 32-bit; may be d_vals itself */,
                                             uint32_t* d_out_counts /* [n] or NULL */, uint32_t* d_num_groups /* DEVICE, one word */,
                                             void* d_workspace, size_t workspace_bytes, void* hip_stream);
LSDSORT_API int lsdsort_reduce_by_key_check_device(void* d_workspace, size_t n, int key_type, void* hip_stream);

/* After the stream has drained: LSDSORT_OK, or LSDSORT_ERR_DEVICE_FAULT if a kernel of the
 * last sort on this workspace gave up a bounded spin or refused destinations outside the output
 * (never expected; the output is then undefined).  Synchronises hip_stream.  With LSDSORT_REPROBE=1
 * in the environment (always in the diagnostic build) the device probe behind the default rank form
 * (lsdsort_set_rank_method) is run again here; a failure is reported as LSDSORT_ERR_DEVICE_FAULT and
 * the library uses the mask forms from then on. */
LSDSORT_API int lsdsort_check_device(void* d_workspace, void* hip_stream);

/* Per-kernel device times of one sort, by hipEvent on hip_stream (the reference times only
 * the whole sort, .cu:1002-1004).  Blocking.  Stages beyond `passes` are zero. */
#define LSDSORT_MAX_PASSES 32
typedef struct lsdsort_timing {
    float total_ms;       /* first kernel start to last kernel end                         */
    float clear_ms;       /* workspace control words + tile-status memset                   */
    float histogram_ms;   /* stage 1 (onesweep: all digits in one read; staged: summed)     */
    float scan_ms;        /* stage 2 (digit-count scan / tile offset tables)                */
    float scatter_ms[LSDSORT_MAX_PASSES]; /* stage 3, one entry per pass (chained form: the  */
                                          /* kernel's own begin/end, hipExtLaunchKernel)    */
    int passes;           /* global passes that ran (hybrid form: 2)                          */
    int tile_keys;        /* keys per rank-and-scatter tile                                 */
    int tiles;
    int hybrid;           /* 1: the hybrid form ran (two global passes + the local stage)    */
    float local_ms;       /* hybrid form: the local stage (every bucket finished in LDS)     */
} lsdsort_timing;
LSDSORT_API int lsdsort_u32_device_timed(uint32_t* d_keys, uint32_t* d_vals, void* d_workspace,
                                         size_t workspace_bytes, size_t n, int radix_bits,
                                         int algorithm, void* hip_stream, lsdsort_timing* out);

/* ---- stage entries (device pointers, stream-ordered) ---------------------------------- */
/* The three stages of a pass as separate calls, for stage-level parity and the histogram /
 * scan micro-benchmarks (counterparts of TestBuildHistogram .cu:704 and TestGPUPrefixSum
 * .cu:304).  Tables are block-major [tiles][2^radix_bits] exactly like the reference's `h`. */

/* Keys per tile of the stage entries for this radix (the reference's `block`).  Whole sorts may
 * use a larger tile for large n (lsdsort_timing.tile_keys reports it); the stage entries and the
 * staged algorithm always use this one. */
LSDSORT_API size_t lsdsort_tile_keys(int radix_bits);

/* Replaces BuildHistogramsKernel, .cu:660-702 (launch .cu:850): d_hist[t][d] = number of
 * keys of tile t whose digit `bit_group` equals d. */
LSDSORT_API int lsdsort_tile_histograms_u32_device(const uint32_t* d_keys, size_t n, int radix_bits,
                                                   int bit_group, uint32_t* d_hist, void* hip_stream);

/* Replaces .cu:862-895 (D2D copy, BlockPrefixSumKernel as local scan, two transposes,
 * GPUPrefixSum + AddBlockSumsKernel): from the counts in d_hist writes d_local (per-tile
 * exclusive scan) and d_global (digit-major exclusive scan, stored block-major).
 * d_scratch holds lsdsort_tile_offsets_scratch_bytes(tiles, radix_bits) bytes. */
LSDSORT_API size_t lsdsort_tile_offsets_scratch_bytes(size_t tiles, int radix_bits);
LSDSORT_API int lsdsort_tile_offsets_u32_device(const uint32_t* d_hist, uint32_t* d_local,
                                                uint32_t* d_global, size_t tiles, int radix_bits,
                                                void* d_scratch, void* hip_stream);

/* Replaces LSDRadixSortKernel, .cu:795-837 (launch .cu:902): stable rank inside each tile,
 * dst = rank - local[d] + global[d] (.cu:833), scatter.  d_vals_in/out may be NULL. */
LSDSORT_API int lsdsort_rank_scatter_u32_device(const uint32_t* d_in, uint32_t* d_out,
                                                const uint32_t* d_vals_in, uint32_t* d_vals_out,
                                                const uint32_t* d_global, size_t n, int radix_bits,
                                                int bit_group, void* hip_stream);

/* The hybrid form's local stage on its own (lsdradixsort_amd/csrc/local_sort.hip): bucket b = d_keys[d_bases[b] .. d_bases[b + 1])
 * (num_buckets + 1 ascending device words) is sorted IN PLACE by its keys' low `low_bits` bits (1..27; stable LSD passes of at
 * most nine bits each, run from LDS to LDS by one workgroup per bucket); d_vals (may be NULL) holds a payload word per key that
 * is permuted with it.  Buckets of more than 16384 keys are left as they are (inside a whole sort the planner has ruled them
 * out).  Needs the returning-LDS-add rank form (LSDSORT_ERR_UNSUPPORTED where the device probe failed). */
LSDSORT_API int lsdsort_local_sort_u32_device(uint32_t* d_keys, uint32_t* d_vals, const uint32_t* d_bases, size_t num_buckets,
                                              int low_bits, void* hip_stream);
/* The same stage reading HALVES, as the hybrid form's half variant runs it (lsdsort_set_half_hop): position q of bucket b is read
 * as the 16-bit word d_halves[d_bases[b] + q] and rebuilt as
 *     key = high | ((2 b + (q >= d_first[b])) >> t) << 16 | half
 * with the three device words d_words = { t (0 .. 7), high (the t top bits every key shares, in place; 0 for t = 0), low_bits
 * (17 - t in a whole sort) }; the bucket is sorted by its keys' low `low_bits` bits (nine bits, then the rest; a digit that is
 * the same for every key of a bucket is no pass) and the full keys are stored to d_keys_out[d_bases[b] ..], which is never
 * read.  d_first: num_buckets words.  The 10240-key kernel: a larger bucket raises bit 3 of *d_fault (may be NULL) and its range
 * of d_keys_out is left as it was.  num_buckets at most 65536.  UNSUPPORTED where the device probe failed. */
LSDSORT_API int lsdsort_local_sort_halves_u32_device(uint32_t* d_keys_out, const uint16_t* d_halves, const uint32_t* d_bases,
                                                     const uint32_t* d_first, size_t num_buckets, const uint32_t* d_words,
                                                     uint32_t* d_fault, void* hip_stream);

/* One read of all keys -> all 32/radix_bits digit histograms, d_hist[g][d] (uint32). */
LSDSORT_API int lsdsort_digit_histograms_u32_device(const uint32_t* d_keys, size_t n, int radix_bits,
                                                    uint32_t* d_hist, void* hip_stream);

/* ---- multi-GPU building block (one process per GPU) ----------------------------------- */
/* Stable partition of this rank's shard by the top msb_bits bits (0..4): d_out holds bucket
 * 0, bucket 1, ... contiguously, d_counts[b] (uint64, 2^msb_bits entries) their sizes.  The
 * caller exchanges buckets with its RCCL communicator (all-to-all over xGMI) and then runs
 * lsdsort_u32_device on what it received.  New work; the reference is single-GPU.
 * n == 0 is NOT a no-op here (nor in the two forms below): d_counts is written (all
 * zero) and the workspace's control block cleared, so d_counts and a workspace of
 * lsdsort_msb_partition_workspace_bytes(0, msb_bits) are needed; d_in / d_out may be NULL. */
LSDSORT_API size_t lsdsort_msb_partition_workspace_bytes(size_t n, int msb_bits);
LSDSORT_API int lsdsort_msb_partition_u32_device(const uint32_t* d_in, uint32_t* d_out, size_t n,
                                                 int msb_bits, uint64_t* d_counts, void* d_workspace,
                                                 size_t workspace_bytes, void* hip_stream);
/* The same partition by value instead of by bit field, for keys that fixed MSB buckets would not
 * balance: `splitters` is a HOST array of 2^log2_buckets - 1 ascending values (copied into the launch),
 * bucket(key) = number of splitters <= key, so bucket b holds splitters[b-1] <= key < splitters[b].
 * Stable; same workspace size as the MSB form (lsdsort_msb_partition_workspace_bytes(n, log2_buckets)).
 * lsdradixsort_amd/dist.py picks the splitters from a gathered sample. */
LSDSORT_API int lsdsort_splitter_partition_u32_device(const uint32_t* d_in, uint32_t* d_out, size_t n,
                                                      int log2_buckets, const uint32_t* splitters,
                                                      uint64_t* d_counts, void* d_workspace,
                                                      size_t workspace_bytes, void* hip_stream);
/* The same with 64-bit thresholds (HOST array, 2^log2_buckets - 1 ascending values in [0, 2^32]):
 * bucket(key) = number of thresholds <= key, and 2^32 stands for "above every key", which a 32-bit splitter
 * cannot say.  The form the sharded step's splitter rule uses (lsdsort_sharded_thresholds). */
LSDSORT_API int lsdsort_threshold_partition_u32_device(const uint32_t* d_in, uint32_t* d_out, size_t n,
                                                       int log2_buckets, const uint64_t* thresholds,
                                                       uint64_t* d_counts, void* d_workspace,
                                                       size_t workspace_bytes, void* hip_stream);

/* ---- multi-GPU sort over RCCL / xGMI (BASELINE.json configs[3]) ------------------------ */
/* New work: the reference is single-GPU.  Rank b of `world` (1, 2, 4 or 8) ends up
 * owning every key whose top log2(world) bits equal b; the sorted array is the concatenation of the ranks'
 * outputs in rank order.  One step per call, on the caller's stream:
 *   1. histogram of the local keys' top bits                                    (one read)
 *   2. stable partition of the shard by those bits  ||  on a side stream: ncclAllGather of the bucket
 *      counts and capacities, count matrix to pinned host memory               (the only host wait)
 *   3. ONE grouped ncclSend/ncclRecv exchange, every peer at once (all xGMI links busy; no ring),
 *      the own bucket by a device copy
 *   4. lsdsort_u32_device on what arrived.
 * librccl is loaded on first use (dlopen); the rest of the library does not depend on it. */
typedef struct lsdsort_comm lsdsort_comm;
#define LSDSORT_COMM_ID_BYTES 128
/* One-process-per-GPU bootstrap: rank 0 makes an id (ncclGetUniqueId), the launcher's own channel
 * (torch.distributed, MPI, a file) carries its 128 bytes to every rank, every rank calls create with the HIP
 * device it will sort on current.  Collective over the `world` ranks. */
LSDSORT_API int lsdsort_comm_unique_id(void* id_out);
LSDSORT_API int lsdsort_comm_create(const void* id, int world, int rank, lsdsort_comm** out);
/* LOOPBACK: `world` (1, 2, 4 or 8) VIRTUAL ranks in this process on the CURRENT device -- out[0 .. world-1] receive their
 * communicators.  Same step, same code; the all-gathers and the grouped exchange are device copies ordered by events
 * instead of RCCL calls.  For machines with one GPU (the step's offsets, ordering, capacities and error paths can then be
 * run with world > 1: tests/test_sharded_loopback.py) and for rehearsing a launcher.  Each virtual rank must be driven by
 * its OWN host thread (the step is collective and waits for the others) and should be given its own stream.  A rank that
 * fails inside a step marks the world aborted: its peers return LSDSORT_ERR_COMM instead of waiting, and the communicators
 * are then only good for lsdsort_comm_destroy. */
LSDSORT_API int lsdsort_comm_create_loopback(int world, lsdsort_comm** out);
LSDSORT_API int lsdsort_comm_destroy(lsdsort_comm* comm);
/* Sub-buckets (1, 2 or 4; world x sub_buckets <= 16, and <= 8 under the splitter rule): the step cuts every rank's key range
 * into that many consecutive sub-ranges, exchanges them one grouped exchange after the other and sorts sub-bucket j on an
 * internal stream while sub-bucket j + 1 is still on the links -- the exchange hides under the local sort instead of in front
 * of it.  Collective setting: every rank of the world must use the same value.  Default 1. */
LSDSORT_API int lsdsort_comm_set_sub_buckets(lsdsort_comm* comm, int sub_buckets);
LSDSORT_API int lsdsort_comm_world(const lsdsort_comm* comm);
LSDSORT_API int lsdsort_comm_rank(const lsdsort_comm* comm);
/* Device workspace for a rank that contributes up to n_local_max keys and may receive up to out_capacity. */
LSDSORT_API size_t lsdsort_sharded_workspace_bytes(size_t n_local_max, size_t out_capacity, int world, int radix_bits);
/* The step.  d_keys_in (n_local keys, left untouched) and d_out (room for out_capacity keys) are device
 * pointers on the communicator's device; on return *n_out keys of d_out are this rank's slice, *global_offset
 * is the index of its first key in the global order, counts_matrix (may be NULL; world*world entries,
 * [src][dst]) says who sent what.  Collective; blocks the host only for the count matrix (the exchange and
 * the local sort stay queued on hip_stream).  If ANY rank would receive more than its out_capacity every rank
 * returns LSDSORT_ERR_CAPACITY before the exchange (capacities travel with the counts; *n_out then holds what this rank
 * would have received), so nobody hangs and the caller can repeat the step with exact sizes.  Every OTHER error is this
 * rank's alone (its peers may be inside a collective): the loopback transport then releases them with LSDSORT_ERR_COMM; over
 * RCCL the launcher has to tear the job down, as with any failed rank of an RCCL job. */
LSDSORT_API int lsdsort_sharded_u32_device(lsdsort_comm* comm, const uint32_t* d_keys_in, size_t n_local,
                                           uint32_t* d_out, size_t out_capacity, size_t* n_out,
                                           uint64_t* global_offset, uint64_t* counts_matrix,
                                           void* d_workspace, size_t workspace_bytes, int radix_bits,
                                           void* hip_stream);
/* The same step with the rule that decides which rank owns a key:
 *   LSDSORT_PARTITION_MSB        the top log2(world) key bits, as above: no extra work, balanced for uniform keys;
 *   LSDSORT_PARTITION_SPLITTERS  sampled splitters, for keys fixed MSB buckets would not balance.  Step 0 is added:
 *      every rank samples LSDSORT_SPLITTER_SAMPLES of its keys at a regular stride, one ncclAllGather hands every
 *      sample to every rank (a second, earlier host wait), and the sorted sample of (key, source rank) pairs is cut into
 *      `world` equal parts (lsdsort_sharded_thresholds).  A splitter is such a PAIR: keys equal to a splitter's value go
 *      below it from ranks before the splitter's rank and above it from the others, so a run of one value longer than a
 *      bucket is still cut (between source ranks) and the exchange stays stable.  Rank b then owns the pairs between
 *      splitters b-1 and b; the concatenation of the ranks' outputs is the sorted array as before (an MSB-style
 *      "which rank owns key k" question has no single answer for a value that sits on a splitter). */
#define LSDSORT_PARTITION_MSB 0
#define LSDSORT_PARTITION_SPLITTERS 1
#define LSDSORT_SPLITTER_SAMPLES 512
LSDSORT_API int lsdsort_sharded_u32_device_ex(lsdsort_comm* comm, const uint32_t* d_keys_in, size_t n_local,
                                              uint32_t* d_out, size_t out_capacity, size_t* n_out,
                                              uint64_t* global_offset, uint64_t* counts_matrix,
                                              void* d_workspace, size_t workspace_bytes, int radix_bits,
                                              int partition, void* hip_stream);
/* Host-side arithmetic of step 0, exported so that it can be checked without a GPU.  `gathered` is
 * [world][1 + samples_per_rank] uint32: per source rank the number of valid samples, then the samples.
 * thresholds[b-1] (b = 1 .. world-1, ascending, values in [0, 2^32]) is the smallest key of rank `rank` that goes to
 * bucket b or higher: bucket(key) = number of thresholds <= key; 2^32 = no key of this rank does. */
LSDSORT_API int lsdsort_sharded_thresholds(const uint32_t* gathered, int world, int samples_per_rank, int rank,
                                           uint64_t* thresholds);
/* The same cut into `parts` (1..8) parts instead of `world`: parts = world x sub-buckets; thresholds[parts - 1]. */
LSDSORT_API int lsdsort_sharded_thresholds_parts(const uint32_t* gathered, int world, int samples_per_rank, int rank,
                                                 int parts, uint64_t* thresholds);
/* After the stream has drained: the fault words of the step's two chained kernels sequences (partition pass, local
 * sort) in a workspace last used with these sizes; LSDSORT_OK or LSDSORT_ERR_DEVICE_FAULT.  Synchronises hip_stream. */
LSDSORT_API int lsdsort_sharded_check_device(void* d_workspace, size_t n_local, size_t out_capacity, int world,
                                             int radix_bits, void* hip_stream);
/* Text of the most recent failed RCCL call on this thread ("" if none). */
LSDSORT_API const char* lsdsort_last_comm_error(void);
/* Host-side arithmetic of step 3, exported so that it can be checked without a GPU: from the world x world
 * count matrix ([src][dst]) the element offsets of rank `rank`'s sends in its partitioned shard, of its
 * receives in its output (source-rank order keeps the exchange stable), its output size and global offset.
 * Returns LSDSORT_ERR_INVALID_ARG for a bad world / rank. */
LSDSORT_API int lsdsort_sharded_plan(const uint64_t* counts_matrix, int world, int rank, uint64_t* send_offsets,
                                     uint64_t* recv_offsets, uint64_t* n_out, uint64_t* global_offset);
/* The same with `sub` sub-buckets per rank: bucket_counts is [src][world * sub] (bucket b belongs to rank b / sub, its
 * sub-bucket b % sub); send_offsets[world * sub] by bucket, recv_offsets[sub * world] by (sub-bucket, source) -- a rank's
 * output holds sub-bucket 0 from source 0, 1, .. then sub-bucket 1 .. --, sub_sizes[sub]. */
LSDSORT_API int lsdsort_sharded_plan_sub(const uint64_t* bucket_counts, int world, int sub, int rank, uint64_t* send_offsets,
                                         uint64_t* recv_offsets, uint64_t* sub_sizes, uint64_t* n_out, uint64_t* global_offset);

/* ---- misc ----------------------------------------------------------------------------- */
LSDSORT_API const char* lsdsort_strerror(int status);
/* hipError_t of the most recent failed HIP call on this thread (0 if none) and its text. */
LSDSORT_API int lsdsort_last_hip_error(void);
LSDSORT_API const char* lsdsort_last_hip_error_string(void);
/* "lsdsort <version> gfx950 hip <runtime>" */
LSDSORT_API const char* lsdsort_version(void);
/* Number of usable devices (gfx950) visible to this process; 0 if none.  Never fails. */
LSDSORT_API int lsdsort_device_count(void);
/* One-time per-device set-up (architecture check + the LDS-atomic probe below); implicit in
 * the first compute call, explicit here so that it can be kept out of a graph capture. */
LSDSORT_API int lsdsort_prepare_device(void);
/* How the rank-and-scatter kernel ranks a key among the same-digit keys of its wavefront:
 *   0  peer masks (wave ballots for digits <= 4 bits, a wave-private LDS OR for 8 bits):
 *      correct on any hardware;
 *   2  one returning LDS add per key, which needs the LDS to serve the colliding lanes of one
 *      wave instruction in lane order; the library verifies that on the device (a probe
 *      kernel at set-up, in the workgroup sizes and LDS footprints of the sort's own kernels) and silently
 *      uses form 0 if it does not hold;
 *  -1  (default) form 2 for 4- and 8-bit digits when the probe passes, form 0 otherwise.
 * lsdsort_rank_method reports the form a sort with this radix will use on the current device. */
LSDSORT_API int lsdsort_set_rank_method(int method);
LSDSORT_API int lsdsort_rank_method(int radix_bits);
/* XCD affinity of the rank-and-scatter kernel: C consecutive tiles are claimed by workgroups of
 * one XCD so that neighbouring runs merge in one L2; 0 disables, default 16,
 * at most 64.  Speed only: results and forward progress never depend on it. */
LSDSORT_API int lsdsort_set_xcd_chunk(int chunk);
/* Dead passes.  A pass whose digit is the same for every key (small key ranges, dead high bits, constant input) is the
 * identity; the device sees that in the digit counts of the upfront read and skips it (its workgroups leave at once), and
 * one copy brings the keys back into the caller's buffer if an odd number of passes ran.  No host round trip, graph-
 * capturable, results identical.  On by default for the uint32 sorts (keys and pairs, default algorithm); the typed
 * sorts and 1-bit digits always run every pass.  0 switches it off (every pass runs, as the reference's do). */
LSDSORT_API int lsdsort_set_pass_skipping(int on);
/* The hybrid form (lsdradixsort_amd/csrc/hybrid.hip, local_sort.hip; no reference counterpart -- its every pass goes through
 * global memory, .cu:844-905).  Sorts of 3.8e7 (pairs 2.2e7, 4-bit digits 2^24) .. 9.6e8 keys or key/value pairs (uint32, int32, float32, either order) with 8- or
 * 4-bit digits: bits 16-31 are sorted first by ordinary global passes (LSD order; two passes at 8-bit digits, four at 4-bit),
 * which leaves the array sorted by its top 16 bits; every bucket of equal top-15-bit value (top 14 bits while uniform keys still fit the local stage: up to about 2^27 items; top 16
 * from 4.8e8) is
 * then finished inside one CU's LDS (bits 0-8, then 9-16) and stored once: at 8-bit digits 4 + 8 + 8 + 8 = 28 bytes per key of
 * memory traffic instead of 4 + 4 x 8 = 36 (pairs: 52 instead of 68), at 4-bit digits 44 instead of 68.  Valid only if every
 * bucket fits the local stage (16384 keys), which depends on the keys: the upfront read counts the buckets exactly and the
 * DEVICE decides before a key is moved; otherwise the ordinary passes run (after their own upfront read: such keys pay about
 * 10 % for the attempt, 1 % where a 65536-key sample already shows it).  Same result either way.  On by default; 0 = always
 * the ordinary passes, the reference's structure. */
LSDSORT_API int lsdsort_set_hybrid(int on);
/* The hybrid form's HALF variant (lsdradixsort_amd/csrc/half_hop.hip): after the second global pass the array is sorted by the 16
 * bits below the key prefix, so those bits of a key follow from its position and the exact counts of the 2^16 groups of equal
 * such bits.  The second pass then writes, and the local stage reads, only the low 16 bits of every key: 4 + 8 + 6 + 6 = 24
 * bytes per key instead of 28.  Attempted for uint32 keys without payloads at 8-bit digits in 2^15 buckets, in a workspace of
 * at least lsdsort_workspace_bytes_roomy(n, 8); the device runs it iff it runs the hybrid form and every bucket fits the
 * 10240-key local kernel, otherwise the full-key launches run, as without it.  Same result either way.  On by default
 * (LSDSORT_HALF_HOP=0 in the environment starts it off); 0 = never attempted. */
LSDSORT_API int lsdsort_set_half_hop(int on);
/* Sorts of up to 16384 keys or pairs (uint32, default algorithm and rank form) are ONE launch: one workgroup sorts them inside
 * its LDS in four 8-bit digit passes (lsdradixsort_amd/csrc/local_sort.hip) instead of clear + stage 1 + stage 2 + 32 / r passes,
 * whose own latencies are all there is at this size (12 us instead of 39).  Same result.  On by default; 0 = the chained form at
 * every size (the reference's stage structure). */
LSDSORT_API int lsdsort_set_small_sort(int on);
/* Which form the last sort queued on `hip_stream` in this workspace ran: *hybrid = 1 the hybrid form, 0 the ordinary passes (also
 * where the hybrid form was not tried).  Reads the device's verdict back: synchronises the stream. */
LSDSORT_API int lsdsort_workspace_form(const void* d_workspace, void* hip_stream, int* hybrid);
/* ... and whether it ran the half variant of it: *half = 1 if so (lsdsort_workspace_form then says 1 as well), else 0.
 * Synchronises the stream. */
LSDSORT_API int lsdsort_workspace_half(const void* d_workspace, void* hip_stream, int* half);
/* lsdsort_u32_device for a SHARD of a range-partitioned array: every key is expected to agree with the others on its top
 * `common_prefix_bits` bits (0 .. 8) -- what a rank holds after the MSB-bucket exchange of the multi-GPU sort (north_star;
 * csrc/sharded.hip calls this).  The hybrid form takes its buckets BELOW a key prefix (with the prefix inside them a shard's 2^15
 * buckets would be 2^(15 - prefix) non-empty ones, each 2^prefix times too large for the local stage, and the form would be
 * refused).  Since the device finds the prefix itself -- from its 65536-key sample, for every sort (keys below 2^31, non-negative
 * int32 keys, shards ...), checked against every key by the upfront read, 0 .. 7 bits -- the argument is only validated; the entry
 * is kept for callers that say what they know.  The result is the sorted array whatever the keys are. */
LSDSORT_API int lsdsort_u32_device_prefixed(uint32_t* d_keys, void* d_workspace, size_t workspace_bytes, size_t n, int radix_bits,
                                            int common_prefix_bits, void* hip_stream);
/* Runtime tuning knob for experiments: selects among the compiled tile shapes (see
 * DESIGN.md); -1 restores the default.  Returns LSDSORT_ERR_INVALID_ARG if unknown. */
LSDSORT_API int lsdsort_set_tile_config(int radix_bits, int config_id);

#ifdef __cplusplus
}
#endif
#endif /* LSDSORT_H */
