// histograms.hip -- stage 1: the digit counts every later stage works from.
//
// Stands in for BuildHistogramsKernel (.cu:660-702).  Four kernels: all digit histograms of an array in one read
// (digit_histograms_kernel), the bucket counts of the splitter partition (bucket_histogram_kernel), the joint (digit, region)
// counts of every pass in one read (joint_histograms_kernel: what the chained form runs) and the per-tile counts of the staged
// form (tile_histograms_kernel).
#include "lsd_device.hpp"
#include "lsd_kernels.hpp"
#include "stage1_stream.hpp"

namespace lsd {

// ------------------------------------------------------------------------------------------
// Stage 1 (onesweep): every digit histogram of the array in ONE read.
//
// A pass permutes keys and never changes them, so the counts LSDRadixSortPass builds at
// .cu:30-35 for each pass can all be taken from the unsorted input.  Each workgroup keeps
// G x 2^R counters in LDS (replicated for narrow digits so 64 lanes do not serialise on two
// or sixteen words), streams keys with 16-byte loads, and flushes once with global atomics.
// ------------------------------------------------------------------------------------------
constexpr int kHistThreads = 256;
constexpr int kHistVecPerThread = 4;   // uint4 loads in flight per thread per iteration

// Grid cap of the stage-1 kernels, in waves: enough to cover HBM latency (256 CUs x 8 workgroups of 256 threads, or 512
// workgroups of 1024).
constexpr uint32_t kHistGridWaves = 2048 * 4;
constexpr uint32_t hist_grid_cap(uint32_t threads) { return kHistGridWaves * 64 / threads; }

template <int R, int G>
__global__ void __launch_bounds__(kHistThreads) digit_histograms_kernel(const uint32_t* __restrict__ keys, uint32_t n,
                                                                       uint32_t shift0, uint32_t* __restrict__ hist,
                                                                       uint32_t vec_chunks)
{
    constexpr int H = 1 << R;
    constexpr int C = hist_copies<R>();
    __shared__ uint32_t s_hist[G * H * C];
    const uint32_t tid = threadIdx.x;
    const uint32_t copy = tid & (C - 1);
    for (uint32_t j = tid; j < (uint32_t)(G * H * C); j += kHistThreads) s_hist[j] = 0;
    __syncthreads();

    auto count_key = [&](uint32_t k) {
#pragma unroll
        for (int g = 0; g < G; g++) {
            const uint32_t d = digit_at<R>(k, shift0 + g * R);
            uint32_t* slot = &s_hist[(g * H + d) * C + copy];
            if (R >= 6) {
                // Low-entropy digits (sorted / constant input) would serialise 64 lanes on
                // one LDS word; when the whole wave agrees, one lane adds 64.
                const uint32_t d0 = __builtin_amdgcn_readfirstlane(d);
                if (__builtin_amdgcn_read_exec() == ~0ull && __all(d == d0)) {
                    if ((tid & 63u) == 0) atomicAdd(&s_hist[(g * H + d0) * C], 64u);
                    continue;
                }
            }
            atomicAdd(slot, 1u);
        }
    };

    // body: whole uint4 chunks, grid-strided; each chunk is kHistThreads*4 keys
    const uint4* __restrict__ keys4 = reinterpret_cast<const uint4*>(keys);
    for (uint32_t c = blockIdx.x * kHistVecPerThread; c < vec_chunks; c += gridDim.x * kHistVecPerThread) {
        uint4 v[kHistVecPerThread];
#pragma unroll
        for (int u = 0; u < kHistVecPerThread; u++) {
            const uint32_t cc = c + u;
            v[u] = cc < vec_chunks ? keys4[(size_t)cc * kHistThreads + tid] : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < kHistVecPerThread; u++) {
            if (c + u < vec_chunks) {
                count_key(v[u].x);
                count_key(v[u].y);
                count_key(v[u].z);
                count_key(v[u].w);
            }
        }
    }
    // tail: the last (n mod chunk) keys -- or, for a base that is not 16-byte aligned (vec_chunks == 0: a
    // slice of a larger buffer), every key -- one per thread per step, strided over the whole grid
    {
        const uint32_t tail_begin = vec_chunks * (kHistThreads * 4);
        for (size_t i = (size_t)tail_begin + (size_t)blockIdx.x * kHistThreads + tid; i < n; i += (size_t)gridDim.x * kHistThreads) {
            const uint32_t k = keys[i];
#pragma unroll
            for (int g = 0; g < G; g++) atomicAdd(&s_hist[(g * H + digit_at<R>(k, shift0 + g * R)) * C + copy], 1u);
        }
    }
    __syncthreads();
    for (uint32_t j = tid; j < (uint32_t)(G * H); j += kHistThreads) {
        uint32_t sum = 0;
#pragma unroll
        for (int c = 0; c < C; c++) sum += s_hist[j * C + c];
        if (sum) atomicAdd(&hist[j], sum);
    }
}

template <int R, int G>
static hipError_t launch_digit_histograms_inst(uint32_t shift0, const uint32_t* keys, uint32_t n, uint32_t* hist,
                                               hipStream_t stream)
{
    const StreamGrid g = stream_grid(keys, n, kHistThreads, kHistVecPerThread, hist_grid_cap(kHistThreads));
    hipLaunchKernelGGL((digit_histograms_kernel<R, G>), dim3(g.blocks), dim3(kHistThreads), 0, stream, keys, n, shift0,
                       hist, g.vec_chunks);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Bucket counts for the splitter partition (multi-GPU step 1 on skewed keys): bucket of a key = the
// number of (ascending) splitters <= key.  Same structure as the digit histogram above, eight
// replicated LDS counters per bucket.
// ------------------------------------------------------------------------------------------
struct SplitterSet {
    uint32_t count;   // buckets - 1
    uint32_t live;    // splitters compared (the rest lie above every key)
    uint32_t value[7];
};

__global__ void __launch_bounds__(kHistThreads) bucket_histogram_kernel(const uint32_t* __restrict__ keys, uint32_t n,
                                                                       SplitterSet sp, uint32_t* __restrict__ hist,
                                                                       uint32_t vec_chunks)
{
    constexpr int C = 8;
    __shared__ uint32_t s_hist[8 * C];
    const uint32_t tid = threadIdx.x;
    if (tid < 8 * C) s_hist[tid] = 0;
    __syncthreads();
    auto count_key = [&](uint32_t k) {
        uint32_t b = 0;
#pragma unroll
        for (int i = 0; i < 7; i++) b += (i < (int)sp.live && k >= sp.value[i]) ? 1u : 0u;
        atomicAdd(&s_hist[b * C + (tid & (C - 1))], 1u);
    };
    const uint4* __restrict__ keys4 = reinterpret_cast<const uint4*>(keys);
    for (uint32_t c = blockIdx.x; c < vec_chunks; c += gridDim.x) {
        const uint4 v = keys4[(size_t)c * kHistThreads + tid];
        count_key(v.x);
        count_key(v.y);
        count_key(v.z);
        count_key(v.w);
    }
    for (size_t i = (size_t)vec_chunks * (kHistThreads * 4) + (size_t)blockIdx.x * kHistThreads + tid; i < n;
         i += (size_t)gridDim.x * kHistThreads)
        count_key(keys[i]);   // tail, or everything when the base is not 16-byte aligned
    __syncthreads();
    if (tid <= sp.count) {
        uint32_t sum = 0;
#pragma unroll
        for (int c = 0; c < C; c++) sum += s_hist[tid * C + c];
        if (sum) atomicAdd(&hist[tid], sum);
    }
}

hipError_t launch_bucket_histogram(int bits, const uint32_t* splitters_host, int live, const uint32_t* keys, uint32_t n,
                                   uint32_t* hist, hipStream_t stream)
{
    if (bits < 1 || bits > 3 || !splitters_host || live < 0 || live > (1 << bits) - 1) return hipErrorInvalidValue;
    SplitterSet sp{};
    sp.count = (1u << bits) - 1u;
    sp.live = (uint32_t)live;
    for (uint32_t i = 0; i < sp.live; i++) sp.value[i] = splitters_host[i];
    const StreamGrid g = stream_grid(keys, n, kHistThreads, 1, hist_grid_cap(kHistThreads));
    hipLaunchKernelGGL(bucket_histogram_kernel, dim3(g.blocks), dim3(kHistThreads), 0, stream, keys, n, sp, hist, g.vec_chunks);
    return hipGetLastError();
}

hipError_t launch_digit_histograms(int radix_bits, int groups, uint32_t shift0, const uint32_t* keys, uint32_t n,
                                   uint32_t* hist, hipStream_t stream)
{
    if (groups == 1) {
        switch (radix_bits) {
            case 1: return launch_digit_histograms_inst<1, 1>(shift0, keys, n, hist, stream);
            case 2: return launch_digit_histograms_inst<2, 1>(shift0, keys, n, hist, stream);
            case 3: return launch_digit_histograms_inst<3, 1>(shift0, keys, n, hist, stream);
            case 4: return launch_digit_histograms_inst<4, 1>(shift0, keys, n, hist, stream);
            case 8: return launch_digit_histograms_inst<8, 1>(shift0, keys, n, hist, stream);
            default: return hipErrorInvalidValue;
        }
    }
    if (groups * radix_bits != 32) return hipErrorInvalidValue;
    switch (radix_bits) {
        case 1: return launch_digit_histograms_inst<1, 32>(shift0, keys, n, hist, stream);
        case 2: return launch_digit_histograms_inst<2, 16>(shift0, keys, n, hist, stream);
        case 4: return launch_digit_histograms_inst<4, 8>(shift0, keys, n, hist, stream);
        case 8: return launch_digit_histograms_inst<8, 4>(shift0, keys, n, hist, stream);
        default: return hipErrorInvalidValue;
    }
}

// ------------------------------------------------------------------------------------------
// Stage 1 (onesweep with regions): joint counts for every pass in ONE read.
//
// For pass p the rank-and-scatter kernel wants, per region x of that pass's input, the histogram
// of digit p (lsd_kernels.hpp, "Regions").  Region membership is a key field too -- the top three
// bits of digit p-1 -- so (digit p, region) is one (R+3)-bit field of the key, bits
// [R*p - 3, R*p + R), and counting it is one v_bfe_u32 and one LDS atomic per key per pass, the
// same work as a plain digit histogram with a table 8x as large.  Pass 0 has no previous digit:
// its regions are by position, uniform for a whole 1024-key chunk.
// ------------------------------------------------------------------------------------------
// Copies of every counter, chosen by lane (tid & (C-1)): small tables are replicated so that 64 lanes do not
// pile onto a few hundred words.
// 8-bit digits, 8 regions: FOUR copies of the 32 KiB of counters, chosen by lane % 4, in 1024-thread workgroups (128 KiB
// of LDS, one workgroup per CU).  LDS atomics of a wave instruction that meet on one word are served a lane per clock
// (tools/ceiling/lds_atomic.hip), so what the copies buy is not speed on uniform keys (1, 2 and 4 copies measure within
// 3 % of each other) but a bound on what a heavy value costs: with c copies at most 16/c lanes of a 16-lane group share a
// word.  2 -> 4 copies: stage 1 on keys that are half zeros 1.02 -> 0.63 ms, on 90 % one value 1.66 -> 0.86 ms, before
// the heavy values are counted by hand (count_vectors below).
constexpr int kR8HistCopies = 4;
constexpr int joint_copies(int radix_bits, bool wide, int counters_per_table)
{
    if (counters_per_table < 1024) return 4;
    if (radix_bits == 8 && !wide && counters_per_table <= 2048) return kR8HistCopies;   // 128 KiB of LDS at most
    return 1;
}

// WIDE (4-bit digits, B = 4): one LDS atomic serves TWO passes.  The field of pass p is key bits
// [4p - 4, 4p + 4); the 12-bit field W_j = bits [8j - 4, 8j + 8) contains the fields of passes 2j (its low
// 8 bits) and 2j + 1 (its high 8 bits), so counting W_0..W_3 (W_0: position region | byte 0) and summing
// 16 counters per output at flush time gives all eight tables from four atomics per key instead of eight:
// the kernel is LDS-atomic-bound, so that is what its time follows (0.49 -> 0.30 ms at 2^28 keys).
// The keys come in by 16-byte loads into registers.  (An LDS-DMA form -- global_load_lds_dwordx4 into a per-wave ring of
// three groups, fetched with ds_read_b128 -- measured 0.32 ms against 0.27 ms in round 3, although a read-only stream of
// LDS-DMA nt loads runs at 6.9-7.0 TB/s where plain 16-byte loads reach 5.2-5.4 and nt ones 5.7-5.9 (tools/ceiling/ceiling2.hip,
// profiles/r3_ceilings.txt): the kernel is bound by the LDS pipe, and the DMA's LDS writes and the ds_read_b128 fetches are 10 %
// more work for it.)
template <int R, int THREADS, bool WIDE = false>
__global__ void __launch_bounds__(THREADS) joint_histograms_kernel(const uint32_t* __restrict__ keys, uint32_t n,
                                                                  uint32_t region0_keys, uint32_t* __restrict__ joint,
                                                                  uint32_t vec_chunks, const KeyTransform xf,
                                                                  uint32_t first_key, const uint32_t* __restrict__ skip)
{
    if (skip && *skip != 0u) return;   // uniform: the hybrid form took the sort (hybrid.hip)
    // `keys` may be a slice [first_key, first_key + n) of the array being sorted (the host entry counts each chunk as
    // it arrives over PCIe): pass-0 regions are by position in the WHOLE array; first_key is a multiple of the chunk.
    const uint32_t chunk_base = first_key / (uint32_t)(THREADS * 4);
    static_assert(!WIDE || R == 4, "wide fields are laid out for 4-bit digits with 4 region bits");
    constexpr int P = 32 / R;
    constexpr int B = region_bits_for_radix(R);
    constexpr int F = (1 << R) << B;          // fields per pass: (digit, region)
    constexpr int NF = WIDE ? P / 2 : P;      // LDS tables
    constexpr int FW = WIDE ? 4096 : F;       // counters per LDS table
    // Narrow digits put 64 lanes on a few hundred words per pass: replicate the table so that
    // neighbouring lanes use different words (and banks); wide digits spread by themselves.
    constexpr int C = joint_copies(R, WIDE, FW);
    static_assert(!WIDE || C == 1, "the wide flush reads one copy per counter");
    extern __shared__ __attribute__((aligned(16))) uint32_t s_joint[];   // [NF][FW][C]
    const uint32_t tid = threadIdx.x;
    const uint32_t copy = tid & (C - 1);
    for (uint32_t j = tid; j < (uint32_t)(NF * FW * C); j += THREADS) s_joint[j] = 0;
    __syncthreads();
    // Counter of a field value, bank-swizzled: the low five index bits (the LDS bank) are XORed with the
    // next five.  Few-valued digits (16 values per byte: text, small alphabets) give field values that
    // are multiples of 8 -- four banks for the whole wave without this (0.81 ms instead of 0.27).
    auto word = [&](uint32_t slot) -> uint32_t& { return s_joint[(slot ^ ((slot >> 5) & 31u)) * C]; };

    // Low-entropy fields (constant or sorted input, dead high digits) would serialise all 64 lanes
    // of a wave on one LDS word; when the whole wave agrees on a field, one lane adds 64 instead.
    // The agreement test is only paid by groups of keys whose FIRST key already shows it in some
    // digit (uniform random input takes the plain path with P tests per 16 keys).
    auto add_field_checked = [&](uint32_t slot) {
        const uint32_t s0 = __builtin_amdgcn_readfirstlane(slot);
        if (__builtin_amdgcn_read_exec() == ~0ull && __all(slot == s0)) {
            if ((tid & 63u) == 0) atomicAdd(&word(s0), 64u);
        } else {
            atomicAdd(&word(slot) + copy, 1u);
        }
    };
    auto count_key_checked = [&](uint32_t k, uint32_t region0) {
        if (WIDE) {
            add_field_checked((region0 << 8) | (k & 0xFFu));
#pragma unroll
            for (int j = 1; j < NF; j++) add_field_checked(j * FW + digit_at<12>(k, (uint32_t)(8 * j - 4)));
            return;
        }
        add_field_checked((region0 << R) | digit_at<R>(k, 0));   // pass 0: region-major in LDS (see flush)
#pragma unroll
        for (int p = 1; p < P; p++) add_field_checked(p * F + digit_at<R + B>(k, (uint32_t)(R * p - B)));
    };
    auto count_key_plain = [&](uint32_t k, uint32_t region0) {
        if (WIDE) {
            atomicAdd(&word((region0 << 8) | (k & 0xFFu)), 1u);
#pragma unroll
            for (int j = 1; j < NF; j++) atomicAdd(&word(j * FW + digit_at<12>(k, (uint32_t)(8 * j - 4))), 1u);
            return;
        }
        atomicAdd(&word((region0 << R) | digit_at<R>(k, 0)) + copy, 1u);
#pragma unroll
        for (int p = 1; p < P; p++)
            atomicAdd(&word(p * F + digit_at<R + B>(k, (uint32_t)(R * p - B))) + copy, 1u);
    };
    // Field f of a key as a table slot (the tables follow each other in LDS).
    auto slot_of = [&](int f, uint32_t k, uint32_t region0) -> uint32_t {
        if (WIDE) return f == 0 ? ((region0 << 8) | (k & 0xFFu)) : (uint32_t)(f * FW) + digit_at<12>(k, (uint32_t)(8 * f - 4));
        return f == 0 ? ((region0 << R) | digit_at<R>(k, 0)) : (uint32_t)(f * F) + digit_at<R + B>(k, (uint32_t)(R * f - B));
    };
    // HEAVY field values.  LDS atomics of one wave instruction that meet on one word are served a lane per clock
    // (tools/ceiling/lds_atomic.hip: 63 clocks for a whole 16-lane group on one word against 7 for random words), so a value
    // that a quarter, half or all of the keys carry -- zeros, a default value, constant or sorted input, dead digits -- would
    // cost stage 1 several times its uniform-key time even with the copies.  A group of VPT vectors whose first keys show
    // such a value in some field (lane 0's value, held by at least kHeavyLanes lanes) takes the careful path below: keys
    // that hold a candidate value are counted in scalar registers (a compare and a population count per wave row, no LDS
    // operation), everybody else adds for itself.  A group without one takes the plain path; both paths count every key
    // exactly, the choice is speed only.
    constexpr uint32_t kNoCandidate = 0xFFFFFFFFu;   // never a slot
    // Software-pipelined with TWO register buffers that swap roles (the loop is unrolled by two): while one group of
    // 16-byte loads goes through the LDS atomics the next is in flight, and the wait in front of a group is a COUNTED one
    // (`vmcnt(VPT)`: everything but the loads just issued).  For the compiler to count, the loads and the group they overtake
    // must sit in ONE straight line: its wait-count pass merges paths conservatively, so a load behind a branch of its own
    // (an `if (chunk < end)` per load, an `if (more) load_group()` per group -- rounds 1 and 2 had both) turned the wait into
    // `vmcnt(0)`, i.e. into waiting for the loads just issued, with nothing in flight while a wave counted.  So the loop takes
    // FULL groups only and always loads: past its last group a workgroup reloads the group it already holds (an L2 hit)
    // and does not count it.  Chunks beyond the last full group go with the tail below.
    constexpr int VPT = kHistVecPerThread;
    const uint32_t full_chunks = full_group_chunks<VPT>(vec_chunks);
    auto load_group = [&](uint32_t c, uint4 (&v)[VPT]) {
        // non-temporal loads: a read-only stream of them runs 8 % faster than plain ones (profiles/r3_ceilings.txt:
        // 5.67-5.88 against 5.24-5.40 TB/s), and the keys are not read again before 2 GiB of other traffic has
        // gone by; stage 1 0.267-0.274 -> 0.249 ms at 2^28 keys (tools/ab_bench.sh)
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        const u32x4* __restrict__ k4 = reinterpret_cast<const u32x4*>(keys);
#pragma unroll
        for (int u = 0; u < VPT; u++) {
            const u32x4 t = __builtin_nontemporal_load(k4 + (size_t)(c + u) * THREADS + tid);
            v[u] = make_uint4(t.x, t.y, t.z, t.w);
        }
    };
    uint32_t key1 = 0, key2 = 0;        // heavy-key candidates of this wave (uniform; kept from group to group)
    bool have1 = false, have2 = false;
    // region_of(u): pass-0 region of vector u of the group (a vector's 4 keys, and the 256 keys of the wave's row, share it)
    auto count_vectors = [&](auto region_of, uint4 (&v)[VPT]) {
        if (xf.on) {   // typed sorts count the "sortable" form of the keys (uniform branch); applied where the keys are used
#pragma unroll
            for (int u = 0; u < VPT; u++)
                v[u] = make_uint4(to_sortable(v[u].x, xf), to_sortable(v[u].y, xf), to_sortable(v[u].z, xf), to_sortable(v[u].w, xf));
        }
        // region0_keys is a multiple of the chunk (THREADS*4 keys), so a chunk is in one region
        const uint32_t region_first = region_of(0);
        // Heavy KEYS first (zeros, a default value, two-valued keys): a key equal to a candidate is counted for ALL its fields
        // by one compare, ballot and population count -- against NF times that in the per-field form below, which such keys
        // used to take (round 2: stage 1 at 4-bit digits 1.05 ms on half-zero keys against 0.25 ms on uniform ones).  The
        // candidates are sticky across groups (a global default value stays one): the group's first keys are compared with
        // them, and only if they do not describe the group (fewer than 16 lanes) is lane 0's key, then lane 32's, tried.
        {
            const uint32_t k0 = v[0].x;
            uint32_t n1 = (uint32_t)__builtin_popcountll(__ballot(k0 == key1));
            if (!have1 || n1 < kHeavyLanes) {
                have1 = have2 = false;
                const uint32_t a = __builtin_amdgcn_readfirstlane(k0);
                unsigned long long m = __ballot(k0 == a);
                if ((uint32_t)__builtin_popcountll(m) >= kHeavyLanes) {
                    key1 = a;
                    have1 = true;
                } else {
                    const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)k0, 32);
                    m = __ballot(k0 == b);
                    if ((uint32_t)__builtin_popcountll(m) >= kHeavyLanes) {
                        key1 = b;
                        have1 = true;
                    }
                }
                if (have1 && ~m != 0ull) {   // a second one: the first value that differs, if eight lanes hold it
                    const uint32_t other = (uint32_t)__builtin_amdgcn_readlane((int)k0, (int)__builtin_ctzll(~m));
                    if ((uint32_t)__builtin_popcountll(__ballot(k0 == other)) >= kHeavySecondLanes) {
                        key2 = other;
                        have2 = true;
                    }
                }
            }
        }
        if (have1) {
            const uint32_t lane = tid & 63u;
            uint32_t total1 = 0, total2 = 0;   // uniform: scalar registers
#pragma unroll
            for (int u = 0; u < VPT; u++) {
                const uint32_t region0 = region_of(u);
                const uint32_t k4[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
                uint32_t n1 = 0, n2 = 0;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const bool h1 = k4[q] == key1, h2 = have2 && k4[q] == key2;
                    n1 += (uint32_t)__builtin_popcountll(__ballot(h1));
                    n2 += (uint32_t)__builtin_popcountll(__ballot(h2));
                    if (!(h1 || h2)) count_key_plain(k4[q], region0);
                }
                // field 0 carries the position region of the vector; the other fields are the key's alone
                if (lane == 0) {
                    if (n1) atomicAdd(&word(slot_of(0, key1, region0)), n1);
                    if (n2) atomicAdd(&word(slot_of(0, key2, region0)), n2);
                }
                total1 += n1;
                total2 += n2;
            }
            if (lane == 0) {
#pragma unroll
                for (int f = 1; f < NF; f++) {
                    if (total1) atomicAdd(&word(slot_of(f, key1, 0u)), total1);
                    if (total2) atomicAdd(&word(slot_of(f, key2, 0u)), total2);
                }
            }
            return;
        }
        bool any = false;
#pragma unroll
        for (int f = 0; f < NF; f++) {
            const uint32_t s0 = slot_of(f, v[0].x, region_first);
            any = any || (uint32_t)__builtin_popcountll(__ballot(s0 == __builtin_amdgcn_readfirstlane(s0))) >= kHeavyLanes;
        }
        if (!any) {
#pragma unroll
            for (int u = 0; u < VPT; u++) {
                const uint32_t region0 = region_of(u);
                count_key_plain(v[u].x, region0);
                count_key_plain(v[u].y, region0);
                count_key_plain(v[u].z, region0);
                count_key_plain(v[u].w, region0);
            }
            return;
        }
        // Per field: up to two candidate values c1, c2 whose holders are counted in scalar registers and added by one lane
        // when the candidates change or the group ends.  The candidates are kept while they describe the vector at hand (16
        // lanes or more of its first keys hold one of them: global heavy values never change) and are picked again from
        // the vector's own first keys otherwise (sorted input: every vector has its own leading value and, where a digit
        // boundary falls inside the wave's 256 keys, a trailing one = the first value that differs).
        const uint32_t lane = tid & 63u;
#pragma unroll
        for (int f = 0; f < NF; f++) {
            uint32_t c1 = kNoCandidate, c2 = kNoCandidate, held1 = 0, held2 = 0;   // uniform: scalar registers; picked at the first vector
            auto flush = [&]() {
                if (lane == 0) {
                    if (held1) atomicAdd(&word(c1), held1);
                    if (held2) atomicAdd(&word(c2), held2);
                }
                held1 = held2 = 0;
            };
#pragma unroll
            for (int u = 0; u < VPT; u++) {
                const uint32_t region0 = region_of(u);
                const uint32_t s4[4] = {slot_of(f, v[u].x, region0), slot_of(f, v[u].y, region0), slot_of(f, v[u].z, region0),
                                        slot_of(f, v[u].w, region0)};
                const uint32_t a = s4[0];
                if ((uint32_t)__builtin_popcountll(__ballot(a == c1 || a == c2)) < kHeavyLanes) {
                    flush();
                    const uint32_t first = __builtin_amdgcn_readfirstlane(a);
                    const unsigned long long mf = __ballot(a == first);
                    c1 = c2 = kNoCandidate;
                    if ((uint32_t)__builtin_popcountll(mf) >= kHeavyLanes) {
                        c1 = first;
                        const unsigned long long rest = ~mf;
                        if (rest) {
                            const uint32_t other = (uint32_t)__builtin_amdgcn_readlane((int)a, (int)__builtin_ctzll(rest));
                            if ((uint32_t)__builtin_popcountll(__ballot(a == other)) >= kHeavySecondLanes) c2 = other;
                        }
                    }
                }
                if (c1 == kNoCandidate) {
                    atomicAdd(&word(s4[0]) + copy, 1u);
                    atomicAdd(&word(s4[1]) + copy, 1u);
                    atomicAdd(&word(s4[2]) + copy, 1u);
                    atomicAdd(&word(s4[3]) + copy, 1u);
                    continue;
                }
                const bool all4 = (s4[0] == c1) & (s4[1] == c1) & (s4[2] == c1) & (s4[3] == c1);
                if (__all(all4)) {   // the wave's 256 keys agree (constant or sorted input, dead digits)
                    held1 += 256u;
                    continue;
                }
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const bool h1 = s4[q] == c1, h2 = s4[q] == c2;
                    held1 += (uint32_t)__builtin_popcountll(__ballot(h1));
                    held2 += (uint32_t)__builtin_popcountll(__ballot(h2));
                    if (!(h1 || h2)) atomicAdd(&word(s4[q]) + copy, 1u);
                }
            }
            flush();
        }
    };
    {
        auto count_group = [&](uint32_t c, uint4 (&v)[VPT]) {
            count_vectors([&](int u) { return ((chunk_base + c + (uint32_t)u) * (uint32_t)(THREADS * 4)) / region0_keys; }, v);
        };
        const uint32_t stride = gridDim.x * VPT;
        uint32_t c = blockIdx.x * VPT;
        if (c < full_chunks) {
            uint4 buf_a[VPT], buf_b[VPT];
            load_group(c, buf_a);
            for (;;) {
                const uint32_t c1 = c + stride;
                const bool more1 = c1 < full_chunks;
                load_group(more1 ? c1 : c, buf_b);
                count_group(c, buf_a);
                if (!more1) break;
                const uint32_t c2 = c1 + stride;
                const bool more2 = c2 < full_chunks;
                load_group(more2 ? c2 : c1, buf_a);
                count_group(c1, buf_b);
                if (!more2) break;
                c = c2;
            }
        }
    }
    const uint32_t tail_begin = full_chunks * (THREADS * 4);   // first key the loop above leaves to the tail
    {
        // tail: the chunks past the last full group and the keys past the last chunk -- or every key when the base is not
        // 16-byte aligned (vec_chunks == 0) -- strided over the grid; a step's keys are consecutive, so a wave stays inside
        // one pass-0 region except at a boundary
        for (size_t i = (size_t)tail_begin + (size_t)blockIdx.x * THREADS + tid; i < n; i += (size_t)gridDim.x * THREADS)
            count_key_checked(xf.on ? to_sortable(keys[i], xf) : keys[i], (uint32_t)((first_key + i) / region0_keys));
    }
    __syncthreads();
    // Flush.  Pass 0's fields sit region-major in LDS: all 64 lanes of a wave share their position
    // region, so with the region in the low index bits they would share four LDS banks; the global
    // table is digit-major for every pass.
    for (uint32_t j = tid; j < (uint32_t)(P * F); j += THREADS) {
        uint32_t cnt = 0;
        if (WIDE) {
            // global entry j = pass p, digit d, region x (digit-major); sum the 16 wide counters that agree
            const uint32_t p = j / (uint32_t)F, d = (j >> B) & 15u, x = j & 15u;
#pragma unroll
            for (uint32_t o = 0; o < 16; o++) {
                uint32_t slot;
                if (p == 0) slot = (x << 8) | (o << 4) | d;            // W_0 = region0 | digit 1 | digit 0: sum over digit 1
                else if (p == 1) slot = (o << 8) | (d << 4) | x;       // region = digit 0: sum over the position region
                else if ((p & 1) == 0) slot = (o << 8) | (d << 4) | x; // W_j = digit 2j+1 | digit 2j | digit 2j-1: sum over the top
                else slot = (d << 8) | (x << 4) | o;                   // pass 2j+1: region = digit 2j: sum over the bottom
                cnt += word((p / 2) * FW + slot);
            }
        } else {
            uint32_t src = j;
            if (j < (uint32_t)F) src = ((j & (uint32_t)((1 << B) - 1)) << R) | (j >> B);
#pragma unroll
            for (int q = 0; q < C; q++) cnt += (&word(src))[q];
        }
        if (cnt) atomicAdd(&joint[j], cnt);
    }
}

// Workgroup sizes.  8-bit digits: 1024 threads around the 128 KiB of counters (four copies, one workgroup per CU); 4-bit
// digits: 512 threads around the wide form's 64 KiB.  (A 512-thread workgroup at 8-bit digits with four region bits, and the
// narrow 256-thread form at 4-bit digits -- eight atomics per key instead of four -- were the alternatives.)
constexpr int kR8HistThreads = 1024;
constexpr int kR4HistThreads = 512;

template <int R, int THREADS, bool WIDE = false>
static hipError_t launch_joint_inst(const uint32_t* keys, uint32_t n, uint32_t region0_keys, uint32_t* joint,
                                    hipStream_t stream, const KeyTransform& xf, uint32_t first_key, const uint32_t* skip)
{
    constexpr int P = 32 / R;
    constexpr int F = (1 << R) << region_bits_for_radix(R);
    constexpr int NF = WIDE ? P / 2 : P;
    constexpr int FW = WIDE ? 4096 : F;
    constexpr int C = joint_copies(R, WIDE, FW);
    constexpr size_t lds_bytes = (size_t)NF * FW * C * sizeof(uint32_t);
    static_assert(lds_bytes <= 160 * 1024, "the counters must fit one CU's LDS");
    if (region0_keys == 0 || region0_keys % (THREADS * 4) != 0 || first_key % (THREADS * 4) != 0) return hipErrorInvalidValue;
    const StreamGrid g = stream_grid(keys, n, THREADS, kHistVecPerThread, hist_grid_cap(THREADS));
    return launch_dynamic_lds<joint_histograms_kernel<R, THREADS, WIDE>>(dim3(g.blocks), dim3(THREADS), lds_bytes, stream, keys, n, region0_keys,
                                                                         joint, g.vec_chunks, xf, first_key, skip);
}

hipError_t launch_joint_histograms(int radix_bits, const uint32_t* keys, uint32_t n, uint32_t region0_keys,
                                   uint32_t* joint, hipStream_t stream, const KeyTransform& xf, uint32_t first_key, const uint32_t* skip)
{
    switch (radix_bits) {
        case 4: return launch_joint_inst<4, kR4HistThreads, true>(keys, n, region0_keys, joint, stream, xf, first_key, skip);   // 64 KiB of counters per workgroup
        case 8: return launch_joint_inst<8, kR8HistThreads>(keys, n, region0_keys, joint, stream, xf, first_key, skip);         // 128 KiB
        default: return hipErrorInvalidValue;
    }
}

// ------------------------------------------------------------------------------------------
// Stage 1 (staged): per-tile digit counts h[tile][digit], BuildHistogramsKernel .cu:660-702.
// One workgroup per tile; counters in LDS, one coalesced row written per tile.
// ------------------------------------------------------------------------------------------
template <int R, int T>
__global__ void __launch_bounds__(T) tile_histograms_kernel(const uint32_t* __restrict__ keys, uint32_t n,
                                                           uint32_t shift, uint32_t tile_keys,
                                                           uint32_t* __restrict__ hist)
{
    constexpr int H = 1 << R;
    constexpr int C = hist_copies<R>();
    __shared__ uint32_t s_hist[H * C];
    const uint32_t tid = threadIdx.x;
    const uint32_t copy = tid & (C - 1);
    for (uint32_t j = tid; j < (uint32_t)(H * C); j += T) s_hist[j] = 0;
    __syncthreads();
    const uint32_t begin = blockIdx.x * tile_keys;
    const uint32_t end = (n - begin < tile_keys) ? n : begin + tile_keys;
    // 16-byte loads over the tile's body when the tile starts on a 16-byte boundary (tile sizes are multiples of four keys,
    // so it does whenever the array does); the few keys behind the last whole vector, or everything otherwise, one by one
    uint32_t scalar_from = begin;
    if ((reinterpret_cast<uintptr_t>(keys + begin) & 15u) == 0) {
        const uint4* __restrict__ v4 = reinterpret_cast<const uint4*>(keys + begin);
        const uint32_t vecs = (end - begin) / 4u;
        for (uint32_t v = tid; v < vecs; v += T) {
            const uint4 k = v4[v];
            atomicAdd(&s_hist[digit_at<R>(k.x, shift) * C + copy], 1u);
            atomicAdd(&s_hist[digit_at<R>(k.y, shift) * C + copy], 1u);
            atomicAdd(&s_hist[digit_at<R>(k.z, shift) * C + copy], 1u);
            atomicAdd(&s_hist[digit_at<R>(k.w, shift) * C + copy], 1u);
        }
        scalar_from = begin + vecs * 4u;
    }
    for (uint32_t i = scalar_from + tid; i < end; i += T) atomicAdd(&s_hist[digit_at<R>(keys[i], shift) * C + copy], 1u);
    __syncthreads();
    for (uint32_t d = tid; d < (uint32_t)H; d += T) {
        uint32_t sum = 0;
#pragma unroll
        for (int c = 0; c < C; c++) sum += s_hist[d * C + c];
        hist[(size_t)blockIdx.x * H + d] = sum;
    }
}

hipError_t launch_tile_histograms(int radix_bits, const TileShape& shape, const uint32_t* keys, uint32_t n,
                                  uint32_t shift, uint32_t* hist, hipStream_t stream)
{
    const uint32_t tile_keys = (uint32_t)shape.tile();
    const uint32_t tiles = (n + tile_keys - 1) / tile_keys;
    if (tiles == 0) return hipSuccess;
    switch (radix_bits) {
#define LSD_CASE(RB)                                                                                              \
    case RB:                                                                                                      \
        hipLaunchKernelGGL((tile_histograms_kernel<RB, 256>), dim3(tiles), dim3(256), 0, stream, keys, n, shift, \
                           tile_keys, hist);                                                                      \
        break;
        LSD_CASE(1) LSD_CASE(2) LSD_CASE(3) LSD_CASE(4) LSD_CASE(8)
#undef LSD_CASE
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace lsd
