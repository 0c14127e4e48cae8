// keys16.hip -- 16-bit keys: uint16, int16, float16, bfloat16.
//
// No reference counterpart: the reference sorts ascending uint32 keys only (LSDRadixSort.cu:62).  A 16-bit key has 65536 values,
// so a keys-only sort needs no pass at all:
//
//   count route (keys only): count | scan | fill.  The COUNT kernel reads the keys once per half of the value range: 65536 32-bit
//       counters are 256 KiB and a CU has 160 KiB of LDS, so every slice of the keys is read by two workgroups and each counts the
//       keys whose sortable top bit is its own into 32768 LDS counters (128 KiB, one workgroup per CU), then adds its non-zero
//       counters to a global uint32[65536] table.  The SCAN kernel (one workgroup) turns the table into exclusive offsets and the
//       total.  The FILL kernel writes the output as runs of the inverse-mapped value, one workgroup per output tile, into the
//       caller's own array -- no key is ever moved, so there is no scatter, no second buffer and no stability question (equal
//       16-bit keys are the same bits).  2 x 2 B read + 2 B written per key.
//   widen route (payloads, and keys-only sorts too small for the count route's fixed costs): one kernel maps the keys to uint32
//       with the sortable value in the low half-word, the ordinary uint32 sort runs on them (its pass skipping drops the two dead
//       high passes on the device; payloads are sorted where they lie), one kernel narrows and un-maps.
//
// The caller's keys need 2-byte alignment only: every kernel peels the keys in front of the first 16-byte line and behind the last
// whole one (Span) and uses 16-byte accesses in between.  Stream-ordered, nothing allocated, every launch sized from n.
#define LSDSORT_BUILD 1
#include "../../include/lsdsort.h"

#include <atomic>

#include "keys16_map.hpp"
#include "lsd_host.hpp"

namespace {

constexpr uint32_t kValues = 65536;          // values of a 16-bit key
constexpr uint32_t kHalfValues = 32768;      // counters of one count workgroup: 128 KiB of LDS
constexpr int kCountThreads = 1024;
constexpr int kCountUnroll = 4;              // 16-byte loads in flight per thread
constexpr uint32_t kMaxSlices = 128;         // x 2 halves = 256 workgroups: one per CU
constexpr uint32_t kMinSliceGroups = 4096;   // a slice is worth its 128 KiB of zeroing and flushing from 32768 keys on
constexpr int kScanThreads = 1024;
constexpr int kFillThreads = 256;
constexpr uint32_t kFillTileGroups = kFillThreads * 4;   // an output tile: 8192 keys
constexpr int kMapThreads = 256;

// Keys-only sorts of at least this many keys take the count route under the automatic rule (lsdsort_set_keys16_route(-1)): the
// smallest measured size at which the count route is ahead of the widen route, 93 against 116 us at 2^23 uniform keys; at 2^22
// it is still behind, 90 against 87 us.  Below that its time is its fixed costs.
constexpr size_t kKeys16CountMinKeys = (size_t)1 << 23;

std::atomic<int> g_route{-1};   // lsdsort_set_keys16_route: -1 auto, 0 widen, 1 count

// The key map (Key16Map, to_sortable16, from_sortable16, key16_map) and the head / 16-byte groups / tail split (Span, span_of,
// body_of, first_tail_key) are keys16_map.hpp's: the 16-bit top-k (topk16.hip) reads keys the same way.

// ------------------------------------------------------------------------------------------------ both routes: clear
// The fault word (widen route: quads = 1) and with it the table (count route) start at zero: `quads` 16-byte stores, one per
// thread.  A kernel rather than a memset, as in segmented.hip: a captured hipMemsetAsync of the table left counts behind when
// its graph was replayed, and the fault word is cleared the same way so that one rule holds here.
__global__ void __launch_bounds__(kMapThreads) keys16_clear_kernel(uint4* __restrict__ words, uint32_t quads)
{
    const uint32_t i = blockIdx.x * kMapThreads + threadIdx.x;
    if (i < quads) words[i] = make_uint4(0, 0, 0, 0);
}

// ------------------------------------------------------------------------------------------------ count route: count
// Workgroup b counts slice b % slices of the 16-byte groups, and of those keys the ones whose sortable value lies in half
// b / slices.  (The two workgroups of a slice are `slices` apart: with 128 slices they run on the same XCD.)
__global__ void __launch_bounds__(kCountThreads) keys16_count_kernel(const uint16_t* __restrict__ keys, Span sp, uint32_t slices,
                                                                    uint32_t slice_groups, Key16Map m, uint32_t* __restrict__ table)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t counters[];   // [kHalfValues]
    const uint32_t tid = threadIdx.x;
    const uint32_t slice = blockIdx.x % slices, half = blockIdx.x / slices;
    for (uint32_t i = tid; i < kHalfValues / 4; i += kCountThreads) reinterpret_cast<uint4*>(counters)[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();

    auto count_key = [&](uint32_t k) {
        const uint32_t t = to_sortable16(k, m);
        if ((t >> 15) == half) atomicAdd(&counters[t & (kHalfValues - 1)], 1u);
    };
    // one 16-byte group per lane.  Where every key of the wavefront's groups is one value (a constant array, a long run) its lanes
    // would serialise on one LDS word: the first active lane adds their number once instead.
    auto count_group = [&](const uint4& v) {
        const uint32_t k0 = v.x & 0xFFFFu;
        const bool one_value = v.x == (k0 | k0 << 16) && v.y == v.x && v.z == v.x && v.w == v.x &&
                               v.x == (uint32_t)__builtin_amdgcn_readfirstlane((int)v.x);
        if (__all(one_value)) {
            const unsigned long long active = __ballot(1);
            const uint32_t t = to_sortable16(k0, m);
            if ((t >> 15) == half && (int)__lane_id() == __ffsll((long long)active) - 1)
                atomicAdd(&counters[t & (kHalfValues - 1)], kGroupKeys * (uint32_t)__popcll(active));
        } else {
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                count_key(w[i] & 0xFFFFu);
                count_key(w[i] >> 16);
            }
        }
    };

    const uint4* body = body_of(keys, sp);
    const uint32_t first = slice * slice_groups;
    const uint32_t end = sp.groups - first < slice_groups ? sp.groups : first + slice_groups;   // first <= groups: the host's slices
    for (uint32_t g = first + tid; g < end; g += kCountUnroll * kCountThreads) {
        uint4 v[kCountUnroll];
#pragma unroll
        for (int j = 0; j < kCountUnroll; j++)
            if (g + j * kCountThreads < end) v[j] = body[g + j * kCountThreads];
#pragma unroll
        for (int j = 0; j < kCountUnroll; j++)
            if (g + j * kCountThreads < end) count_group(v[j]);
    }
    if (slice == 0) {   // the keys outside the 16-byte groups
        if (tid < sp.head) count_key(keys[tid]);
        if (tid < sp.tail) count_key(keys[first_tail_key(sp) + tid]);
    }
    __syncthreads();
    uint32_t* mine = table + half * kHalfValues;
    for (uint32_t i = tid; i < kHalfValues; i += kCountThreads) {
        const uint32_t c = counters[i];
        if (c) atomicAdd(&mine[i], c);   // exact and order-free
    }
}

// ------------------------------------------------------------------------------------------------ count route: scan
// table[v] = number of keys of sortable value v  ->  table[v] = number of keys below v, table[65536] = the total.  One workgroup,
// in place: 16 rounds of 1024 threads x 4 counters, the running total carried from round to round.
__global__ void __launch_bounds__(kScanThreads) keys16_scan_kernel(uint32_t* __restrict__ table)
{
    __shared__ uint32_t wave_total[kScanThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint4* table4 = reinterpret_cast<uint4*>(table);
    uint32_t carry = 0;
    for (uint32_t round = 0; round < kValues / (4 * kScanThreads); round++) {
        const uint4 v = table4[round * kScanThreads + tid];
        const uint32_t sum = v.x + v.y + v.z + v.w;
        uint32_t incl = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if ((int)lane >= d) incl += up;
        }
        if (lane == 63) wave_total[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < kScanThreads / 64; w++) {
            const uint32_t t = wave_total[w];
            if (w < wave) before += t;
            all += t;
        }
        const uint32_t excl = carry + before + incl - sum;
        table4[round * kScanThreads + tid] = make_uint4(excl, excl + v.x, excl + v.x + v.y, excl + v.x + v.y + v.z);
        carry += all;
        __syncthreads();   // wave_total is rewritten by the next round
    }
    if (tid == 0) table[kValues] = carry;
}

// ------------------------------------------------------------------------------------------------ count route: fill
// The largest v in [lo, hi) with offsets[v] <= p; the caller knows offsets[lo] <= p.  Reads offsets[lo + 1 .. hi - 1] only.
__device__ __forceinline__ uint32_t value_at(const uint32_t* __restrict__ offsets, uint32_t p, uint32_t lo, uint32_t hi)
{
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (offsets[mid] <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Output position p holds the key of the sortable value v with offsets[v] <= p < offsets[v + 1].  One workgroup per tile of
// kFillTileGroups 16-byte groups: the tile's first and last value by binary search over all offsets, then every group its first
// value by a search between those two, and on from there.  Every store is inside the tile and inside [0, n).  Where the scanned
// total is not n (never expected: the counts then do not describe the keys) the fault word is set; the stores stay inside.
__global__ void __launch_bounds__(kFillThreads) keys16_fill_kernel(uint16_t* __restrict__ keys, Span sp, uint32_t n,
                                                                  const uint32_t* __restrict__ offsets, Key16Map m,
                                                                  uint32_t* __restrict__ fault)
{
    const uint32_t tid = threadIdx.x;
    if (blockIdx.x == 0) {
        if (tid == 0 && offsets[kValues] != n) atomicOr(fault, 1u);
        if (tid < sp.head) keys[tid] = (uint16_t)from_sortable16(value_at(offsets, tid, 0, kValues), m);
        if (tid < sp.tail) {
            const uint32_t p = first_tail_key(sp) + tid;   // < n
            keys[p] = (uint16_t)from_sortable16(value_at(offsets, p, 0, kValues), m);
        }
    }
    const uint32_t first = blockIdx.x * kFillTileGroups;
    if (first >= sp.groups) return;
    const uint32_t end = sp.groups - first < kFillTileGroups ? sp.groups : first + kFillTileGroups;
    const uint32_t v_first = value_at(offsets, sp.head + first * kGroupKeys, 0, kValues);
    const uint32_t v_last = value_at(offsets, sp.head + end * kGroupKeys - 1, v_first, kValues);
    uint4* body = reinterpret_cast<uint4*>(keys + sp.head);
    for (uint32_t g = first + tid; g < end; g += kFillThreads) {
        const uint32_t p = sp.head + g * kGroupKeys;
        uint32_t v = value_at(offsets, p, v_first, v_last + 1);
        uint32_t next = offsets[v + 1];   // v <= 65535: the total at most
        uint32_t key = from_sortable16(v, m);
        uint32_t w[4];
#pragma unroll
        for (uint32_t i = 0; i < kGroupKeys; i++) {
            if (p + i >= next && v < v_last) {   // the run ends inside the group: the next non-empty value
                v = value_at(offsets, p + i, v, v_last + 1);
                next = offsets[v + 1];
                key = from_sortable16(v, m);
            }
            if (i & 1) w[i >> 1] |= key << 16;
            else w[i >> 1] = key;
        }
        body[g] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// ------------------------------------------------------------------------------------------------ widen route
// wide[i] = sortable value of key i, as a uint32.  `wide` is 256-byte aligned, so the eight words of group g lie on 16-byte lines
// where the head is a multiple of four keys (wide_vec); otherwise they go word by word.
__global__ void __launch_bounds__(kMapThreads) keys16_widen_kernel(const uint16_t* __restrict__ keys, Span sp, uint32_t wide_vec,
                                                                  Key16Map m, uint32_t* __restrict__ wide)
{
    const uint32_t tid = threadIdx.x;
    if (blockIdx.x == 0) {
        if (tid < sp.head) wide[tid] = to_sortable16(keys[tid], m);
        if (tid < sp.tail) wide[first_tail_key(sp) + tid] = to_sortable16(keys[first_tail_key(sp) + tid], m);
    }
    const uint4* body = body_of(keys, sp);
    for (uint32_t g = blockIdx.x * kMapThreads + tid; g < sp.groups; g += gridDim.x * kMapThreads) {
        const uint4 v = body[g];
        const uint32_t in[4] = {v.x, v.y, v.z, v.w};
        uint32_t t[kGroupKeys];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            t[2 * i] = to_sortable16(in[i] & 0xFFFFu, m);
            t[2 * i + 1] = to_sortable16(in[i] >> 16, m);
        }
        uint32_t* out = wide + sp.head + g * kGroupKeys;
        if (wide_vec) {
            reinterpret_cast<uint4*>(out)[0] = make_uint4(t[0], t[1], t[2], t[3]);
            reinterpret_cast<uint4*>(out)[1] = make_uint4(t[4], t[5], t[6], t[7]);
        } else {
#pragma unroll
            for (uint32_t i = 0; i < kGroupKeys; i++) out[i] = t[i];
        }
    }
}

// key i = the key of the sortable value wide[i]
__global__ void __launch_bounds__(kMapThreads) keys16_narrow_kernel(const uint32_t* __restrict__ wide, Span sp, uint32_t wide_vec,
                                                                   Key16Map m, uint16_t* __restrict__ keys)
{
    const uint32_t tid = threadIdx.x;
    if (blockIdx.x == 0) {
        if (tid < sp.head) keys[tid] = (uint16_t)from_sortable16(wide[tid] & 0xFFFFu, m);
        if (tid < sp.tail) keys[first_tail_key(sp) + tid] = (uint16_t)from_sortable16(wide[first_tail_key(sp) + tid] & 0xFFFFu, m);
    }
    uint4* body = reinterpret_cast<uint4*>(keys + sp.head);
    for (uint32_t g = blockIdx.x * kMapThreads + tid; g < sp.groups; g += gridDim.x * kMapThreads) {
        const uint32_t* in = wide + sp.head + g * kGroupKeys;
        uint32_t t[kGroupKeys];
        if (wide_vec) {
            const uint4 lo = reinterpret_cast<const uint4*>(in)[0], hi = reinterpret_cast<const uint4*>(in)[1];
            t[0] = lo.x; t[1] = lo.y; t[2] = lo.z; t[3] = lo.w;
            t[4] = hi.x; t[5] = hi.y; t[6] = hi.z; t[7] = hi.w;
        } else {
#pragma unroll
            for (uint32_t i = 0; i < kGroupKeys; i++) t[i] = in[i];
        }
        uint32_t w[4];
#pragma unroll
        for (int i = 0; i < 4; i++)
            w[i] = from_sortable16(t[2 * i] & 0xFFFFu, m) | from_sortable16(t[2 * i + 1] & 0xFFFFu, m) << 16;
        body[g] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// ------------------------------------------------------------------------------------------------ host side
// One carve-up for both routes: a workspace serves whichever the library picks.
struct Keys16Layout {
    size_t control = 0;        // u32: the call's fault word (the fill kernel's, and the inner sort's kept from its own workspace)
    size_t table = 0;          // count route: uint32[65537], counts, then offsets and the total
    size_t wide = 0;           // widen route: uint32[n]
    size_t sort_ws = 0;        // widen route: the inner sort's workspace
    size_t sort_ws_bytes = 0;
    size_t total = 0;
};

Keys16Layout make_keys16_layout(size_t n, int pairs)
{
    Keys16Layout L;
    size_t off = 0;
    L.control = off; off += lsd::kAlign;
    L.table = off; off += lsd::align_up((kValues + 1) * sizeof(uint32_t));
    L.wide = off; off += lsd::align_up(n * sizeof(uint32_t));
    L.sort_ws = off;
    L.sort_ws_bytes = lsdsort_workspace_bytes(n, 8, pairs);
    off += lsd::align_up(L.sort_ws_bytes);
    L.total = off;
    return L;
}

int count_route(uint16_t* keys, const Span& sp, size_t n, const Key16Map& m, char* ws, const Keys16Layout& L, hipStream_t s)
{
    uint32_t* fault = reinterpret_cast<uint32_t*>(ws + L.control);
    uint32_t* table = reinterpret_cast<uint32_t*>(ws + L.table);
    const uint32_t quads = (uint32_t)((L.wide - L.control) / sizeof(uint4));   // the fault word and the table, which lie together
    hipLaunchKernelGGL(keys16_clear_kernel, dim3(lsd::grid_for(quads, kMapThreads, (size_t)1 << 31)), dim3(kMapThreads), 0, s,
                       reinterpret_cast<uint4*>(ws + L.control), quads);
    LSD_HIP(hipGetLastError());
    const uint32_t slices = lsd::grid_for(sp.groups, kMinSliceGroups, kMaxSlices);
    const uint32_t slice_groups = (sp.groups + slices - 1) / slices;   // every slice starts at or before the end: (slices - 1)^2 <= groups
    LSD_HIP((lsd::launch_dynamic_lds<keys16_count_kernel>(dim3(2 * slices), dim3(kCountThreads), kHalfValues * sizeof(uint32_t), s,
                                                          static_cast<const uint16_t*>(keys), sp, slices, slice_groups, m, table)));
    hipLaunchKernelGGL(keys16_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, table);
    LSD_HIP(hipGetLastError());
    const uint32_t tiles = lsd::grid_for(sp.groups, kFillTileGroups, (size_t)1 << 31);
    hipLaunchKernelGGL(keys16_fill_kernel, dim3(tiles), dim3(kFillThreads), 0, s, keys, sp, (uint32_t)n, static_cast<const uint32_t*>(table), m,
                       fault);
    LSD_HIP(hipGetLastError());
    return LSDSORT_OK;
}

int widen_route(uint16_t* keys, uint32_t* vals, const Span& sp, size_t n, const Key16Map& m, char* ws, const Keys16Layout& L, hipStream_t s)
{
    uint32_t* fault = reinterpret_cast<uint32_t*>(ws + L.control);
    uint32_t* wide = reinterpret_cast<uint32_t*>(ws + L.wide);
    hipLaunchKernelGGL(keys16_clear_kernel, dim3(1), dim3(kMapThreads), 0, s, reinterpret_cast<uint4*>(fault), 1u);   // the control block's first 16 bytes
    LSD_HIP(hipGetLastError());
    const uint32_t grid = lsd::grid_for(sp.groups, kMapThreads, 2048);
    const uint32_t wide_vec = (sp.head & 3u) == 0 ? 1u : 0u;
    hipLaunchKernelGGL(keys16_widen_kernel, dim3(grid), dim3(kMapThreads), 0, s, static_cast<const uint16_t*>(keys), sp, wide_vec, m, wide);
    LSD_HIP(hipGetLastError());
    // the high half-words are zero: the sort's upfront read sees two dead digits and its last two passes leave at once
    if (vals) LSD_TRY(lsdsort_pairs_u32_device(wide, vals, ws + L.sort_ws, L.sort_ws_bytes, n, 8, s));
    else LSD_TRY(lsdsort_u32_device(wide, ws + L.sort_ws, L.sort_ws_bytes, n, 8, s));
    LSD_HIP(lsd::launch_keep_fault(fault, reinterpret_cast<const uint32_t*>(ws + L.sort_ws), s));
    hipLaunchKernelGGL(keys16_narrow_kernel, dim3(grid), dim3(kMapThreads), 0, s, static_cast<const uint32_t*>(wide), sp, wide_vec, m, keys);
    LSD_HIP(hipGetLastError());
    return LSDSORT_OK;
}

}  // namespace

extern "C" {

size_t lsdsort_keys16_workspace_bytes(size_t n, int pairs)
{
    if ((pairs != 0 && pairs != 1) || n > LSDSORT_MAX_KEYS) return 0;
    return make_keys16_layout(n, pairs).total;
}

int lsdsort_set_keys16_route(int route)
{
    if (route < -1 || route > 1) return LSDSORT_ERR_INVALID_ARG;
    g_route.store(route, std::memory_order_relaxed);
    return LSDSORT_OK;
}

int lsdsort_keys16_device(void* d_keys, uint32_t* d_vals, void* d_workspace, size_t workspace_bytes, size_t n, int key_type,
                          int descending, void* hip_stream)
{
    Key16Map m;
    LSD_TRY(key16_map(key_type, descending, &m));
    if (n > LSDSORT_MAX_KEYS) return LSDSORT_ERR_TOO_LARGE;
    if (n == 0) return LSDSORT_OK;
    if (!d_keys || ((uintptr_t)d_keys & 1)) return LSDSORT_ERR_INVALID_ARG;
    const Keys16Layout L = make_keys16_layout(n, d_vals ? 1 : 0);
    if (!lsd::workspace_ok(d_workspace, workspace_bytes, L.total)) return LSDSORT_ERR_WORKSPACE;
    LSD_TRY(lsdsort_prepare_device());
    const int route = g_route.load(std::memory_order_relaxed);
    const bool count = !d_vals && (route == 1 || (route == -1 && n >= kKeys16CountMinKeys));
    const Span sp = span_of(d_keys, n);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    char* ws = static_cast<char*>(d_workspace);
    uint16_t* keys = static_cast<uint16_t*>(d_keys);
    return count ? count_route(keys, sp, n, m, ws, L, s) : widen_route(keys, d_vals, sp, n, m, ws, L, s);
}

int lsdsort_keys16_check_device(void* d_workspace, size_t n, int pairs, void* hip_stream)
{
    if (!d_workspace) return LSDSORT_ERR_WORKSPACE;
    if (pairs != 0 && pairs != 1) return LSDSORT_ERR_INVALID_ARG;
    if (n > LSDSORT_MAX_KEYS) return LSDSORT_ERR_TOO_LARGE;
    if (n == 0) return LSDSORT_OK;   // an empty call touches nothing
    // the control word holds the fill kernel's verdict or the inner sort's fault word, whichever route ran
    return lsdsort_check_device(static_cast<char*>(d_workspace) + make_keys16_layout(n, pairs).control, hip_stream);
}

}  // extern "C"
