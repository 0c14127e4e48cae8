// wide.hip -- 64-bit keys and 64-bit payloads over the 32-bit pass kernels.
//
// No reference counterpart: the reference sorts ascending uint32 keys only (LSDRadixSort.cu:62).  An LSD sort on a
// 64-bit key is an LSD sort on its low word followed by a stable LSD sort on its high word, so nothing new is needed
// in the pass kernels: the key/value kernel (the other word, or an index, rides as the payload) does all of it.
//
//   uint64 keys only            : split (lo[], hi[]) | pairs sort by lo carrying hi | pairs sort by hi carrying lo | merge.
//                                 8 passes at 8-bit digits, 16 B/key/pass -- what a native 64-bit-key pass would move --
//                                 plus the split and the merge (16 B/key each) and the two upfront histogram reads.
//   uint64 keys + 32/64-bit payloads, uint32 keys + 64-bit payloads (records): every word that is not the key word being
//                                 sorted on rides through the passes as a payload array of its own (the key/value kernel
//                                 carries up to three: lsdsort_multi_u32_device) -- 64/64: by lo carrying (hi, vlo, vhi), then by
//                                 hi carrying (lo, vlo, vhi).  No gather: round 2 sorted an index and gathered the records at
//                                 random at the end, which cost more than the passes (13.5 ms of a 64/64 sort of 2^27 records).
//   int64 / float64 keys, descending order (lsdsort_keys64_device): the order-preserving map to uint64 is applied where the key
//                                 is split into words and undone where the sorted words are merged -- the two kernels that touch
//                                 every key once anyway -- so it costs no pass and no byte; the sorts in between are plain uint32
//                                 sorts of the mapped words and keep pass skipping and the hybrid form.  Payloads are never mapped.
// Everything is stream-ordered on the caller's stream and allocates nothing (workspace), like the 32-bit entries.
#define LSDSORT_BUILD 1
#include "../../include/lsdsort.h"

#include "lsd_host.hpp"

namespace {

constexpr int kThreads = 256;
uint32_t grid_for(size_t n, size_t per_thread = 4)
{
    const size_t blocks = (n + kThreads * per_thread - 1) / (kThreads * per_thread);
    return (uint32_t)(blocks < 1 ? 1 : (blocks > 65536 ? 65536 : blocks));
}

__global__ void __launch_bounds__(kThreads) split_u64_kernel(const uint2* __restrict__ in, uint32_t* __restrict__ lo,
                                                            uint32_t* __restrict__ hi, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
        const uint2 k = in[i];   // little-endian: x = low word
        lo[i] = k.x;
        if (hi) hi[i] = k.y;
    }
}

__global__ void __launch_bounds__(kThreads) merge_u64_kernel(const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi,
                                                            uint2* __restrict__ out, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads)
        out[i] = make_uint2(lo[i], hi[i]);
}

// The caller's 64-bit key type and order as the map the key kernels below apply: t = k ^ ((sign(k) & a) | b) ^ c, sign(k) = k's top
// bit in all 64 positions.  uint64 (0, 0), int64 (0, 2^63), float64 (~0, 2^63): a negative double is complemented in ALL 64 bits, a
// non-negative one gets its sign bit flipped (IEEE total order); c = ~0 for descending.  The 64-bit form of KeyTransform.
struct Key64Transform {
    uint64_t a = 0, b = 0, c = 0;
    bool on() const { return (a | b | c) != 0; }
};

template <bool XF>
__device__ __forceinline__ uint64_t key64_to_ordered(uint64_t k, const Key64Transform& xf)
{
    if (!XF) return k;
    const uint64_t sign = (uint64_t)((int64_t)k >> 63);
    return k ^ ((sign & xf.a) | xf.b) ^ xf.c;
}

// the inverse: u = t ^ c has its top bit SET where the key was not negative (or the type has no sign map)
template <bool XF>
__device__ __forceinline__ uint64_t key64_from_ordered(uint64_t t, const Key64Transform& xf)
{
    if (!XF) return t;
    const uint64_t u = t ^ xf.c;
    const uint64_t was_negative = (uint64_t)((int64_t)~u >> 63);
    return u ^ ((was_negative & xf.a) | xf.b);
}

constexpr size_t kKeysPerThread = 4;   // of the key kernels' vector part: two 16-byte loads, one 16-byte store per word array

// Keys: the split with the map in it.  `groups` = groups of four keys handled with 16-byte accesses (n / 4 where the caller's array
// is 16-byte aligned, else 0: the word arrays are workspace, 256-byte aligned); keys from 4 * groups on go one by one.
template <bool XF>
__global__ void __launch_bounds__(kThreads) split_keys64_kernel(const uint64_t* __restrict__ in, uint32_t* __restrict__ lo,
                                                               uint32_t* __restrict__ hi, size_t n, size_t groups, Key64Transform xf)
{
    const size_t first = (size_t)blockIdx.x * kThreads + threadIdx.x, stride = (size_t)gridDim.x * kThreads;
    const ulonglong2* in2 = reinterpret_cast<const ulonglong2*>(in);
    for (size_t g = first; g < groups; g += stride) {
        const ulonglong2 p = in2[2 * g], q = in2[2 * g + 1];
        const uint64_t t0 = key64_to_ordered<XF>(p.x, xf), t1 = key64_to_ordered<XF>(p.y, xf);
        const uint64_t t2 = key64_to_ordered<XF>(q.x, xf), t3 = key64_to_ordered<XF>(q.y, xf);
        reinterpret_cast<uint4*>(lo)[g] = make_uint4((uint32_t)t0, (uint32_t)t1, (uint32_t)t2, (uint32_t)t3);
        reinterpret_cast<uint4*>(hi)[g] = make_uint4((uint32_t)(t0 >> 32), (uint32_t)(t1 >> 32), (uint32_t)(t2 >> 32), (uint32_t)(t3 >> 32));
    }
    for (size_t i = groups * kKeysPerThread + first; i < n; i += stride) {
        const uint64_t t = key64_to_ordered<XF>(in[i], xf);
        lo[i] = (uint32_t)t;
        hi[i] = (uint32_t)(t >> 32);
    }
}

// Keys: the merge with the inverse map in it; `groups` as above.
template <bool XF>
__global__ void __launch_bounds__(kThreads) merge_keys64_kernel(const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi,
                                                               uint64_t* __restrict__ out, size_t n, size_t groups, Key64Transform xf)
{
    const size_t first = (size_t)blockIdx.x * kThreads + threadIdx.x, stride = (size_t)gridDim.x * kThreads;
    ulonglong2* out2 = reinterpret_cast<ulonglong2*>(out);
    for (size_t g = first; g < groups; g += stride) {
        const uint4 l = reinterpret_cast<const uint4*>(lo)[g], h = reinterpret_cast<const uint4*>(hi)[g];
        ulonglong2 p, q;
        p.x = key64_from_ordered<XF>((uint64_t)h.x << 32 | l.x, xf);
        p.y = key64_from_ordered<XF>((uint64_t)h.y << 32 | l.y, xf);
        q.x = key64_from_ordered<XF>((uint64_t)h.z << 32 | l.z, xf);
        q.y = key64_from_ordered<XF>((uint64_t)h.w << 32 | l.w, xf);
        out2[2 * g] = p;
        out2[2 * g + 1] = q;
    }
    for (size_t i = groups * kKeysPerThread + first; i < n; i += stride)
        out[i] = key64_from_ordered<XF>((uint64_t)hi[i] << 32 | lo[i], xf);
}

// key_type (LSDSORT_KEY_U64 | I64 | F64) and direction as that map; a 32-bit key type is no key of these entries
int key64_transform(int key_type, int descending, Key64Transform* xf)
{
    *xf = Key64Transform{};
    switch (key_type) {
        case LSDSORT_KEY_U64: break;
        case LSDSORT_KEY_I64: xf->b = 1ull << 63; break;
        case LSDSORT_KEY_F64: xf->a = ~0ull; xf->b = 1ull << 63; break;
        default: return LSDSORT_ERR_INVALID_ARG;
    }
    if (descending) xf->c = ~0ull;
    return LSDSORT_OK;
}

struct WideLayout {
    size_t sticky = 0;              // u32: fault words of every sort inside the call, ORed together (each sort's opening
                                    // clear takes the shared sort workspace's own word, so the first sort's would be lost)
    size_t a = 0, b = 0;            // uint32[n]: low / high key words (64-bit keys)
    size_t c = 0, d = 0;            // uint32[n]: low / high payload words (64-bit payloads)
    size_t sort_ws = 0;             // workspace of the sorts inside
    size_t sort_ws_bytes = 0;
    int payloads = 1;               // payload arrays the sorts inside carry
    size_t total = 0;
};

// key_bits 32 | 64, val_bits 0 | 32 | 64 (32/32 and 32/0 are the ordinary entries, not served here)
WideLayout make_wide_layout(size_t n, int radix_bits, int key_bits, int val_bits)
{
    WideLayout L;
    size_t off = 0;
    L.sticky = off; off += lsd::kAlign;
    const size_t words = lsd::align_up(n * sizeof(uint32_t));
    if (key_bits == 64) {
        L.a = off; off += words;
        L.b = off; off += words;
    }
    if (val_bits == 64) {
        L.c = off; off += words;
        L.d = off; off += words;
    }
    // what rides with the key word: the other key word (64-bit keys) and the payload's words
    L.payloads = (key_bits == 64 ? 1 : 0) + val_bits / 32;
    L.sort_ws = off;
    L.sort_ws_bytes = lsdsort_workspace_bytes(n, radix_bits, L.payloads);
    off += lsd::align_up(L.sort_ws_bytes);
    L.total = off;
    return L;
}

bool wide_combo(int key_bits, int val_bits)
{
    return (key_bits == 64 && (val_bits == 0 || val_bits == 32 || val_bits == 64)) || (key_bits == 32 && val_bits == 64);
}

int check_common(const void* d_keys, const void* d_vals, int val_bits, void* ws, size_t ws_bytes, size_t n, int radix_bits,
                 const WideLayout& L)
{
    if (n > LSDSORT_MAX_KEYS) return LSDSORT_ERR_TOO_LARGE;
    if (lsdsort_workspace_bytes(1, radix_bits, 1) == 0) return LSDSORT_ERR_INVALID_ARG;
    if (n == 0) return LSDSORT_OK;
    if (!d_keys || (val_bits && !d_vals)) return LSDSORT_ERR_INVALID_ARG;
    if (!lsd::workspace_ok(ws, ws_bytes, L.total)) return LSDSORT_ERR_WORKSPACE;
    return LSDSORT_OK;
}

}  // namespace

extern "C" {

size_t lsdsort_wide_workspace_bytes(size_t n, int radix_bits, int key_bits, int val_bits)
{
    if (!wide_combo(key_bits, val_bits) || n > LSDSORT_MAX_KEYS || lsdsort_workspace_bytes(1, radix_bits, 1) == 0) return 0;
    return make_wide_layout(n, radix_bits, key_bits, val_bits).total;
}

// Any of the wide combinations (key_bits 32 | 64, val_bits 0 | 32 | 64); stable by key.  xf: how 64-bit keys compare (32-bit keys
// are uint32 ascending: the multi-payload pass kernel has no typed instantiation).
static int sort_wide(void* d_keys, void* d_vals, int key_bits, int val_bits, void* d_workspace, size_t workspace_bytes, size_t n,
                     int radix_bits, const Key64Transform& xf, void* hip_stream)
{
    const WideLayout L = make_wide_layout(n, radix_bits, key_bits, val_bits);
    LSD_TRY(check_common(d_keys, d_vals, val_bits, d_workspace, workspace_bytes, n, radix_bits, L));
    if (n == 0) return LSDSORT_OK;
    LSD_TRY(lsdsort_prepare_device());
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    char* ws = static_cast<char*>(d_workspace);
    const uint32_t g = grid_for(n);
    uint32_t* sticky = reinterpret_cast<uint32_t*>(ws + L.sticky);
    const uint32_t* fault = reinterpret_cast<const uint32_t*>(ws + L.sort_ws);   // the sorts' fault word: first word of their workspace
    LSD_HIP(lsd::launch_clear(sticky, sizeof(uint32_t), s));
    // the words of the records as arrays of their own: 32-bit members are used where they lie
    uint32_t* klo = key_bits == 64 ? reinterpret_cast<uint32_t*>(ws + L.a) : static_cast<uint32_t*>(d_keys);
    uint32_t* khi = key_bits == 64 ? reinterpret_cast<uint32_t*>(ws + L.b) : nullptr;
    uint32_t* vlo = val_bits == 64 ? reinterpret_cast<uint32_t*>(ws + L.c) : static_cast<uint32_t*>(d_vals);   // null: keys only
    uint32_t* vhi = val_bits == 64 ? reinterpret_cast<uint32_t*>(ws + L.d) : nullptr;
    // 16-byte accesses on the caller's keys where they allow it (the ABI asks for 8-byte alignment only)
    const size_t groups = ((uintptr_t)d_keys & 15) == 0 ? n / kKeysPerThread : 0;
    if (key_bits == 64) {
        if (xf.on())
            hipLaunchKernelGGL(split_keys64_kernel<true>, dim3(g), dim3(kThreads), 0, s, static_cast<const uint64_t*>(d_keys), klo, khi, n,
                               groups, xf);
        else
            hipLaunchKernelGGL(split_keys64_kernel<false>, dim3(g), dim3(kThreads), 0, s, static_cast<const uint64_t*>(d_keys), klo, khi, n,
                               groups, xf);
        LSD_HIP(hipGetLastError());
    }
    if (val_bits == 64) {
        hipLaunchKernelGGL(split_u64_kernel, dim3(g), dim3(kThreads), 0, s, static_cast<const uint2*>(d_vals), vlo, vhi, n);
        LSD_HIP(hipGetLastError());
    }
    // LSD over the key's words, low word first, then a stable sort on the high word: sorted by (hi, lo) -- the LSD argument, one
    // word at a time; everything else rides as payload arrays (stable: ties keep their order)
    {
        uint32_t* pay[3];
        int np = 0;
        if (khi) pay[np++] = khi;
        if (vlo) pay[np++] = vlo;
        if (vhi) pay[np++] = vhi;
        LSD_TRY(lsdsort_multi_u32_device(klo, pay, np, ws + L.sort_ws, L.sort_ws_bytes, n, radix_bits, s));
        LSD_HIP(lsd::launch_keep_fault(sticky, fault, s));   // the next sort's opening clear takes that word
    }
    if (khi) {
        uint32_t* pay[3];
        int np = 0;
        pay[np++] = klo;
        if (vlo) pay[np++] = vlo;
        if (vhi) pay[np++] = vhi;
        LSD_TRY(lsdsort_multi_u32_device(khi, pay, np, ws + L.sort_ws, L.sort_ws_bytes, n, radix_bits, s));
        LSD_HIP(lsd::launch_keep_fault(sticky, fault, s));
        if (xf.on())
            hipLaunchKernelGGL(merge_keys64_kernel<true>, dim3(g), dim3(kThreads), 0, s, klo, khi, static_cast<uint64_t*>(d_keys), n, groups,
                               xf);
        else
            hipLaunchKernelGGL(merge_keys64_kernel<false>, dim3(g), dim3(kThreads), 0, s, klo, khi, static_cast<uint64_t*>(d_keys), n, groups,
                               xf);
        LSD_HIP(hipGetLastError());
    }
    if (vhi) {
        hipLaunchKernelGGL(merge_u64_kernel, dim3(g), dim3(kThreads), 0, s, vlo, vhi, static_cast<uint2*>(d_vals), n);
        LSD_HIP(hipGetLastError());
    }
    return LSDSORT_OK;
}

int lsdsort_u64_device(uint64_t* d_keys, void* d_workspace, size_t workspace_bytes, size_t n, int radix_bits, void* hip_stream)
{
    return lsdsort_keys64_device(d_keys, nullptr, 0, d_workspace, workspace_bytes, n, radix_bits, LSDSORT_KEY_U64, 0, hip_stream);
}

// 64-bit keys of another type or order, alone or with 32- or 64-bit payloads; stable by key (descending too).
int lsdsort_keys64_device(void* d_keys, void* d_vals, int val_bits, void* d_workspace, size_t workspace_bytes, size_t n, int radix_bits,
                          int key_type, int descending, void* hip_stream)
{
    Key64Transform xf;
    LSD_TRY(key64_transform(key_type, descending, &xf));
    if (!wide_combo(64, val_bits)) return LSDSORT_ERR_INVALID_ARG;
    return sort_wide(d_keys, d_vals, 64, val_bits, d_workspace, workspace_bytes, n, radix_bits, xf, hip_stream);
}

// Records: keys of key_bits (32 | 64) with payloads of val_bits (32 | 64, not both 32); stable by key.
int lsdsort_records_device(void* d_keys, void* d_vals, int key_bits, int val_bits, void* d_workspace, size_t workspace_bytes,
                           size_t n, int radix_bits, void* hip_stream)
{
    if (!wide_combo(key_bits, val_bits) || val_bits == 0) return LSDSORT_ERR_INVALID_ARG;
    if (key_bits == 64)
        return lsdsort_keys64_device(d_keys, d_vals, val_bits, d_workspace, workspace_bytes, n, radix_bits, LSDSORT_KEY_U64, 0, hip_stream);
    return sort_wide(d_keys, d_vals, key_bits, val_bits, d_workspace, workspace_bytes, n, radix_bits, Key64Transform{}, hip_stream);
}

int lsdsort_wide_check_device(void* d_workspace, size_t n, int radix_bits, int key_bits, int val_bits, void* hip_stream)
{
    if (!d_workspace) return LSDSORT_ERR_WORKSPACE;
    if (!wide_combo(key_bits, val_bits) || lsdsort_workspace_bytes(1, radix_bits, 1) == 0) return LSDSORT_ERR_INVALID_ARG;
    const WideLayout L = make_wide_layout(n, radix_bits, key_bits, val_bits);
    if (n == 0) return LSDSORT_OK;   // an empty call touches nothing
    // the sticky word holds every inner sort's fault word (lsdsort_check_device reads the first word of what it is given)
    return lsdsort_check_device(static_cast<char*>(d_workspace) + L.sticky, hip_stream);
}

}  // extern "C"
