// local_sort.hip -- the last stage of the hybrid form: buckets that fit the LDS, one workgroup each.
//
// No counterpart in the reference (its every pass goes through global memory, LSDRadixSort.cu:839-910).  After the hybrid form's two
// global passes on the key's two high bytes the array is sorted by its top 16 bits, i.e. cut into 2^15 buckets of equal top-15-bit
// value whose sizes the upfront read has counted exactly (hybrid.hip).  A bucket of at most kLocalCap keys is then finished
// where it lies: one 512-thread workgroup loads it, runs the remaining digit passes -- the same stable rank (one returning LDS add
// per key against wave-private counters) and the same LDS reorder as a global pass, but from LDS to LDS -- and stores it back
// in place.  8 B/key of HBM traffic for the low 17 bits instead of 16 B/key for two more global passes, and no chained scan:
// buckets are independent.
//
// Buckets are the top 15 or the top 14 bits (lsd_kernels.hpp hybrid_bucket_bits), below a key prefix where the caller has named one;
// 4-bit-digit sorts come here after four global passes instead of two.
//
// Per workgroup (T = 512 threads, up to K = 32 keys each, two workgroups per CU):
//   load, wave-striped: wave w owns positions [w * rows * 64, (w + 1) * rows * 64) of the bucket, lane l's i-th register holds
//                       position w * rows * 64 + i * 64 + l, rows = ceil(size / T); positions past the bucket hold 0xFFFFFFFF
//                       (the highest digit in every pass and the highest positions: they would stay at the end and are never
//                       stored) and are neither ranked nor scattered (LocalGroup::live, ::inside)
//   per digit pass    : zero the wave's counters | rank = returning add | barrier | one thread per counter word (two digits): wave
//                       bases + exclusive scan over digits | barrier | keys -> LDS at (base + rank) | barrier | read back in
//                       position order
//   store             : from LDS, linear.
// Counters are 16 bits wide, two to a word (a wave holds at most 2048 keys): 8 waves x 512 digits in 8 KiB, so that two
// workgroups share a CU (72 KiB each) and one's loads and barriers hide under the other's LDS work.
//
// The pass is written once (LocalGroup and the steps that follow it); sort_bucket, sort_bucket_multi and sort_segment are what is
// particular to each: how keys are loaded, which digits run, and what leaves.
#include "lsd_device.hpp"
#include "lsd_kernels.hpp"

namespace lsd {

typedef __attribute__((address_space(3))) uint16_t lds_u16;

constexpr int kLocalThreads = 512;
constexpr int kLocalWaves = kLocalThreads / kWave;
constexpr int kLocalMaxBins = 512;
static_assert(kLocalThreads * 32 == kLocalSortCap, "the capacity the planner checks buckets against");
static_assert(kLocalThreads * 20 == kLocalSortCapSmall && kLocalThreads * 16 == kLocalSortCapSmallPairs, "the capacities of the three-per-CU variants");
template <int K>
constexpr size_t local_lds_words() { return (size_t)kLocalThreads * K + kLocalWaves * (kLocalMaxBins / 2) + 64; }

// ---- the workgroup's LDS, one bucket's place in it, and the steps of a digit pass ---------------------------------------------
// K registers per thread and array: key[i], rank[i], val[i] belong to position wbase + 64 i, rows of them in use.
template <int K>
struct LocalGroup {
    lds_u32* s_keys;              // [T * K]: keys (then payloads) in their new order
    volatile lds_u32* s_cnt;      // [W][256] words = [W][512] 16-bit counters, then bases
    volatile lds_u16* s_cnt16;
    lds_u32* s_misc;              // 64 words: the scan's partials [0, W), the callers' reductions over waves from 32
    uint32_t tid, lane, wave;
    uint32_t size, rows, wbase;   // rows = ceil(size / T), uniform, 1 .. K
    // Padding: the wave's rows from `live` on (0 .. rows, uniform per wave) lie wholly past the bucket's end and take no part in a
    // pass; in the one partial row, lane l holds a key in row i iff 64 i < inside.  Ranked like keys, the padding of a wave would
    // all add to the highest digit's counter, which the LDS serves a lane per clock (about 64 clocks a row against 8 for random
    // digits), on the last wave's way to the barrier.  It was the last of the highest digit and was never stored, so every key
    // keeps its slot.
    // INVARIANT: s_keys[size, rows * T) belongs to the padding lanes of the partial rows, each lane to its own position wbase + 64 i.
    // No key's slot lies there (slots are ranks below size), store_linear stops at size, and only the owner reads or writes a
    // position.  Such a lane is not switched off -- an exec mask around the adds costs more than the padding did --
    // but made harmless: its add is of 0 to word [wave][lane] of the wave's own counters (lane < 64 <= kLocalMaxBins / 2), its
    // scatter goes to its own position, its slot (KEEP) is that position, so read_rows, write_slots and the composition of two
    // passes' slots find there what the lane itself put there.
    uint32_t live, inside;
};
// SKIP_PADDING false: every row and lane takes part, as if the bucket filled its rows (the segmented sort's kernels: with the two
// words more they spill -- 88 B of scratch per lane without payloads, a wave per SIMD less with: tools/isa_diff.py --resources,
// recorded in profiles/half_hop/compare.txt; tests/test_kernel_resources.py fails on both if sort_segment asks for true)
template <int K, bool SKIP_PADDING = true>
__device__ __forceinline__ LocalGroup<K> local_group(uint32_t size)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    LocalGroup<K> g;
    g.s_keys = (lds_u32*)smem;
    g.s_cnt = (volatile lds_u32*)(g.s_keys + kLocalThreads * K);
    g.s_cnt16 = (volatile lds_u16*)g.s_cnt;
    g.s_misc = (lds_u32*)(g.s_cnt + kLocalWaves * (kLocalMaxBins / 2));
    g.tid = threadIdx.x;
    g.lane = g.tid & 63u;
    g.wave = g.tid >> 6;
    g.size = size;
    g.rows = (size + (uint32_t)kLocalThreads - 1u) / (uint32_t)kLocalThreads;
    g.wbase = g.wave * g.rows * 64u + g.lane;
    g.live = g.rows;
    g.inside = 0xFFFFFFFFu;
    if (SKIP_PADDING) {
        const uint32_t wfirst = (uint32_t)__builtin_amdgcn_readfirstlane((int)(g.wave * g.rows * 64u));
        const uint32_t left = size > wfirst ? (size - wfirst + 63u) / 64u : 0u;
        g.live = left < g.rows ? left : g.rows;
        g.inside = size > g.wbase ? size - g.wbase : 0u;
    }
    return g;
}
// does lane l's position in row i hold a key?  (one compare against a constant: all of a row but in the partial one)
template <int K>
__device__ __forceinline__ bool holds_key(const LocalGroup<K>& g, int i) { return (uint32_t)i * 64u < g.inside; }

__device__ __forceinline__ void raise_fault(uint32_t* fault, uint32_t bit)
{
    if (threadIdx.x == 0 && fault) atomicOr(fault, bit);
}

// r[i] = src[position of register i], 0xFFFFFFFF past the end and in the rows past the last (the paired scatter looks at one)
template <int K>
__device__ __forceinline__ void load_rows(const LocalGroup<K>& g, const uint32_t* src, uint32_t (&r)[K])
{
#pragma unroll
    for (int i = 0; i < K; i++) {
        r[i] = 0xFFFFFFFFu;
        if ((uint32_t)i < g.rows) {
            const uint32_t pos = g.wbase + (uint32_t)i * 64u;
            if (pos < g.size) r[i] = src[pos];
        }
    }
}
// LDS -> registers in position order; registers -> LDS at slot[i]; LDS -> global memory, linear (x: the key transform to undo).
// The live rows only: the registers of the others keep what the load gave them (0xFFFFFFFF), and a padding lane of the partial
// row finds in its own position what scatter_keys parked there (its own register again); its slot[i] is that position.
template <int K>
__device__ __forceinline__ void read_rows(const LocalGroup<K>& g, uint32_t (&r)[K])
{
#pragma unroll
    for (int i = 0; i < K; i++)
        if ((uint32_t)i < g.live) r[i] = g.s_keys[g.wbase + (uint32_t)i * 64u];
}
template <int K>
__device__ __forceinline__ void write_slots(const LocalGroup<K>& g, const uint32_t (&slot)[K], const uint32_t (&r)[K])
{
#pragma unroll
    for (int i = 0; i < K; i++)
        if ((uint32_t)i < g.live) g.s_keys[slot[i]] = r[i];
}
template <int K>
__device__ __forceinline__ void store_linear(const LocalGroup<K>& g, uint32_t* dst, const KeyTransform* x = nullptr)
{
    for (uint32_t q = g.tid; q < g.size; q += (uint32_t)kLocalThreads) dst[q] = x ? from_sortable(g.s_keys[q], *x) : g.s_keys[q];
}

// Count and rank: rank[i] = the keys of this wave with key[i]'s digit that stand before it, by one returning add per key.
template <int K>
__device__ __forceinline__ void count_and_rank(const LocalGroup<K>& g, const uint32_t (&key)[K], uint32_t (&rank)[K], uint32_t shift,
                                               uint32_t mask)
{
    constexpr int HW = kLocalMaxBins / 2;   // counter words per wave
    // this wave's counters start at zero (its own words only: LDS operations of a wave are served in order, and nobody
    // else reads them before the barrier below)
#pragma unroll
    for (int j = 0; j < HW / kWave; j++) g.s_cnt[g.wave * HW + j * kWave + g.lane] = 0;
#pragma unroll
    for (int i = 0; i < K; i++) {
        if ((uint32_t)i < g.live) {
            // a padding lane of the partial row adds nothing, to a word of its own (no exec mask: the adds of all rows stay in
            // one chain of uniform branches, issued back to back)
            const bool on = holds_key(g, i);
            const uint32_t d = (key[i] >> shift) & mask;
            const uint32_t sh = (d & 1u) * 16u;
            const uint32_t old = __hip_atomic_fetch_add((lds_u32*)&g.s_cnt[g.wave * HW + (on ? d >> 1 : g.lane)], on ? 1u << sh : 0u,
                                                        __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            rank[i] = (old >> sh) & 0xFFFFu;
        }
    }
    __syncthreads();
}
// Exclusive scan of v over the first `threads` threads of the workgroup (uniform, at most 256; v = 0 in the others).  The form of
// group_exclusive_scan (lsd_device.hpp) for a scan that few waves take part in: one wave needs no partials and no barrier; with
// more, only the waves that hold such threads write a partial or read them (four words: at most three waves precede one).
template <int K>
__device__ __forceinline__ uint32_t live_exclusive_scan(const LocalGroup<K>& g, uint32_t v, uint32_t threads)
{
    const uint32_t incl = wave_inclusive_scan(v);
    uint32_t before = 0;
    if (threads > (uint32_t)kWave) {   // uniform
        const bool live_wave = g.tid - g.lane < threads;
        if (live_wave && g.lane == 63u) g.s_misc[g.wave] = incl;
        __syncthreads();
        if (live_wave) {
#pragma unroll
            for (int w = 0; w < 4; w++) {   // a partial at or past this wave's own may be stale: never added
                const uint32_t t = g.s_misc[w];
                before += (uint32_t)w < g.wave ? t : 0u;
            }
        }
    }
    return before + incl - v;
}
// Counts to bases, one thread per counter WORD (digits 2j and 2j + 1; bins / 2 threads): the waves' counts become their bases inside
// the digit's range, the digits' totals an exclusive scan.  The running sum over the waves stays packed, both halves in one add,
// and so does what is written back: run + (off | (off + low) << 16), off = the keys of the digits below 2j.  Every half is a
// number of keys of one bucket, at most kLocalSortCap = 16384, so no carry leaves a low half (tests/test_local_bases_cpu.py).
// Half the LDS instructions of one thread per 16-bit counter, between two barriers where the workgroup's other waves wait.
template <int K>
__device__ __forceinline__ void counts_to_bases(const LocalGroup<K>& g, uint32_t bins)
{
    constexpr int W = kLocalWaves, HW = kLocalMaxBins / 2;
    const uint32_t threads = bins >> 1;   // bins is even: a digit has at least one bit
    const bool mine = g.tid < threads;
    uint32_t total = 0;
    uint32_t wave_excl[W];
    if (mine) {
#pragma unroll
        for (int w = 0; w < W; w++) {
            wave_excl[w] = total;
            total += g.s_cnt[w * HW + g.tid];
        }
    }
    const uint32_t low = total & 0xFFFFu;
    const uint32_t off = live_exclusive_scan(g, low + (total >> 16), threads);   // total = 0 past the last word
    if (mine) {
        const uint32_t add = off | ((off + low) << 16);
#pragma unroll
        for (int w = 0; w < W; w++) g.s_cnt[w * HW + g.tid] = wave_excl[w] + add;
    }
    __syncthreads();
}
// Scatter: key[i] to LDS slot base + rank.  KEEP: rank[i] becomes that slot (a payload follows its key there).
template <int K, bool KEEP>
__device__ __forceinline__ void scatter_keys(const LocalGroup<K>& g, const uint32_t (&key)[K], uint32_t (&rank)[K], uint32_t shift,
                                             uint32_t mask)
{
    // two rows per uniform branch: both base reads are in flight before the first write waits for its own (0.590 -> 0.584 ms per
    // 2^28 keys).  A row past the wave's last live one reads a counter it never uses -- its key register holds whatever it holds,
    // masked into the table.  A padding lane of the partial row parks its register (0xFFFFFFFF) at its own position: past the
    // bucket's end, where no key goes and nothing is stored from.
    static_assert(K % 2 == 0, "rows are scattered in pairs");
#pragma unroll
    for (int i = 0; i < K; i += 2) {
        if ((uint32_t)i < g.live) {
            const uint32_t b0 = g.s_cnt16[g.wave * kLocalMaxBins + ((key[i] >> shift) & mask)];
            const uint32_t b1 = g.s_cnt16[g.wave * kLocalMaxBins + ((key[i + 1] >> shift) & mask)];
            const uint32_t pos0 = holds_key(g, i) ? b0 + rank[i] : g.wbase + (uint32_t)i * 64u;
            if (KEEP) rank[i] = pos0;
            g.s_keys[pos0] = key[i];
            if ((uint32_t)(i + 1) < g.live) {
                const uint32_t pos1 = holds_key(g, i + 1) ? b1 + rank[i + 1] : g.wbase + (uint32_t)(i + 1) * 64u;
                if (KEEP) rank[i + 1] = pos1;
                g.s_keys[pos1] = key[i + 1];
            }
        }
    }
    __syncthreads();
}
// One digit pass over key[] (position order): afterwards the keys lie in LDS in their new order, and with KEEP rank[i] says
// where key[i] went.
template <int K, bool KEEP>
__device__ __forceinline__ void digit_pass(const LocalGroup<K>& g, const uint32_t (&key)[K], uint32_t (&rank)[K], uint32_t shift,
                                           uint32_t width)
{
    const uint32_t bins = 1u << width, mask = bins - 1u;
    count_and_rank(g, key, rank, shift, mask);
    counts_to_bases(g, bins);
    scatter_keys<K, KEEP>(g, key, rank, shift, mask);
}
// After a pass the keys are in LDS in their new order.  `last`: they leave for global memory (linear store, `x` undone); otherwise
// they come back into registers in position order (the next pass's first barrier keeps its LDS writes behind these reads).  With
// payloads: the same for them, through the same slots, once the keys have been taken out -- two more barriers per pass.
template <int K, bool PAIRS>
__device__ __forceinline__ void take_out(const LocalGroup<K>& g, bool last, uint32_t (&key)[K], const uint32_t (&slot)[K],
                                         uint32_t (&val)[K], uint32_t* keys_out, const KeyTransform* x, uint32_t* vals_out)
{
    if (last) store_linear(g, keys_out, x);
    else read_rows(g, key);
    if (PAIRS) {
        __syncthreads();   // every key has been taken out
        write_slots(g, slot, val);
        __syncthreads();
        if (last) store_linear(g, vals_out);
        else read_rows(g, val);
    }
}

// The size of bucket [lo, hi), or 0 where this workgroup has nothing to do: an empty bucket, or one above the capacity -- the
// small variant leaves larger buckets to the listed launch; above the large capacity the planner promised otherwise: say so,
// touch nothing.
template <int K>
__device__ __forceinline__ uint32_t bucket_size(const LocalSortParams& p, uint32_t lo, uint32_t hi)
{
    if (hi < lo) return 0u;
    if (hi - lo > (uint32_t)(kLocalThreads * K)) {
        if (!p.larger_elsewhere) raise_fault(p.fault, 8u);
        return 0u;
    }
    return hi - lo;
}

// K = 32: buckets of up to 16384 keys, 72 KiB of LDS, two workgroups per CU.  K = 20: up to 10240 keys, 48 KiB, THREE per CU
// (and at most 80 registers): the stage is bound by LDS work that one workgroup's barriers and loads leave idle, so the third
// resident workgroup is worth about a fifth of its time.  The planner knows the largest bucket and picks (LocalSortParams::skip
// of the other launch); uniform keys at 2^28 have buckets of 8192 +- 300.
// PAIRS: a payload word follows each key (LocalSortParams::vals).  It takes the key's LDS slot in a second round of every pass, as
// in the global pass kernel: keys to LDS, keys back, payloads to the same slots, payloads back (take_out).
// XOUT: a typed sort's keys leave as what they were (int32, float32, descending order).  A kernel of its own: the five
// instructions per key cost the uint32 sort 0.025 ms of 0.59 when they sat in the one store loop.
// WHOLE: the bucket is the whole array [0, p.num_buckets) and a fourth digit pass may follow (launch_small_sort)
template <int K, bool PAIRS, bool XOUT, bool WHOLE = false>
__device__ __forceinline__ void sort_bucket(const LocalSortParams& p, const uint32_t b)
{
    const uint32_t lo = WHOLE ? 0u : p.bases[b];
    const uint32_t size = bucket_size<K>(p, lo, WHOLE ? p.num_buckets : p.bases[b + 1]);
    if (size == 0u) return;
    const LocalGroup<K> g = local_group<K>(size);
    uint32_t* const bucket = p.keys + lo;
    uint32_t* const bucket_vals = PAIRS ? p.vals + lo : nullptr;
    uint32_t key[K], rank[K], val[K];   // val: PAIRS only
    // The half form (LocalSortParams::halves; this one kernel only, every other instantiation keeps its code): the bucket arrives
    // as 16-bit halves and each key is rebuilt from its position -- the bits above the half are those of group 2 b for the first
    // first[b] positions and of group 2 b + 1 behind them, below the prefix every key shares.  For a prefix t >= 1 the group's
    // lowest t bits lie inside the half and the two words are equal.  `bucket` is then only written.
    constexpr bool kMayReadHalves = K == 20 && !PAIRS && !XOUT && !WHOLE;
    bool from_halves = false;   // uniform
    uint32_t ref = 0u;          // the key at position 0: the dead-digit test's reference
    if constexpr (kMayReadHalves) from_halves = p.halves != nullptr && (!p.half_on || *p.half_on != 0u);
    if (from_halves) {
        if constexpr (kMayReadHalves) {
            const uint16_t* const half = p.halves + lo;
            const uint32_t t = *p.prefix_word, high = *p.high_word, first = p.first[b];
            const uint32_t upper0 = high | (((2u * b) >> t) << 16), upper1 = high | (((2u * b + 1u) >> t) << 16);
            ref = (first ? upper0 : upper1) | half[0];
            // the loads first, all of them in flight, and the upper bits in a loop of its own: ORed in where the half is loaded,
            // each row's region ends waiting for its own load -- twenty round trips in a row (local stage 0.55 -> 0.86 ms)
#pragma unroll
            for (int i = 0; i < K; i++) {
                key[i] = 0xFFFFFFFFu;
                if ((uint32_t)i < g.rows) {
                    const uint32_t pos = g.wbase + (uint32_t)i * 64u;
                    if (pos < size) key[i] = half[pos];
                }
            }
#pragma unroll
            for (int i = 0; i < K; i++) key[i] |= g.wbase + (uint32_t)i * 64u < first ? upper0 : upper1;   // padding stays 0xFFFFFFFF
        }
    } else {
        // keys and payloads in one loop, written out here: through load_rows, or one array after the other, the pairs kernels take ten
        // registers more (K = 16 spills, the K = 32 list kernel loses a wave per SIMD)
#pragma unroll
        for (int i = 0; i < K; i++) {
            key[i] = 0xFFFFFFFFu;   // rows past the bucket's last are never ranked or stored; the paired scatter looks at one
            if ((uint32_t)i < g.rows) {
                const uint32_t pos = g.wbase + (uint32_t)i * 64u;
                if (pos < size) key[i] = bucket[pos];
                if (PAIRS) val[i] = pos < size ? bucket_vals[pos] : 0u;
            }
        }
    }
    auto pass = [&](uint32_t shift, uint32_t width, bool last) {
        digit_pass<K, PAIRS>(g, key, rank, shift, width);
        take_out<K, PAIRS>(g, last, key, rank, val, bucket, XOUT ? &p.xout : nullptr, bucket_vals);
    };

    // the digits: as given, or (the hybrid form, planned on the device) bits [0, low) in one or two passes: nine bits, then the rest
    uint32_t sh0 = p.shift[0], wd0 = p.width[0], sh1 = p.shift[1], wd1 = p.width[1], wd2 = p.width[2];
    if (p.low_bits_word) {
        const uint32_t low = *p.low_bits_word;   // uniform
        sh0 = 0u; wd0 = low < 9u ? low : 9u;
        sh1 = wd0; wd1 = low - wd0;
        wd2 = 0u;
    }
    bool dead0 = false, dead1 = false;
    if (p.low_bits_word && wd1) {
        // Two digits (the hybrid form).  A digit that is the same for every key of the bucket -- dead low bits: keys that are
        // multiples of 512 -- is no pass at all, and as a pass it is the worst one: every lane on one counter, which the LDS
        // serves a lane per clock (2.47 instead of 1.85 ms per 2^28 such keys).  One OR over the bucket says so: key ^ first key,
        // per thread, per wave, then across the waves through LDS.  One of the two passes always runs.
        if (!from_halves) ref = bucket[0];   // (the half form: bucket[0] is a stale word; ref is the rebuilt key)
        uint32_t diff = 0;
#pragma unroll
        for (int i = 0; i < K; i++)
            if ((uint32_t)i < g.rows) diff |= g.wbase + (uint32_t)i * 64u < size ? key[i] ^ ref : 0u;
        diff = wave_or(diff);
        if (g.lane == 0u) g.s_misc[32 + g.wave] = diff;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < kLocalWaves; w++) diff |= g.s_misc[32 + w];
        dead0 = ((diff >> sh0) & ((1u << wd0) - 1u)) == 0u;                  // uniform
        dead1 = !dead0 && ((diff >> sh1) & ((1u << wd1) - 1u)) == 0u;
    }
    if (!dead0) pass(sh0, wd0, wd1 == 0u || dead1);
    if (wd1 && !dead1) pass(sh1, wd1, wd2 == 0u);
    if (wd2) pass(p.shift[2], wd2, !WHOLE || p.width[3] == 0u);
    if (WHOLE && wd2 && p.width[3]) pass(p.shift[3], p.width[3], true);
}

// Several payload arrays (records: lsdsort_multi_u32_device): carrying each of them through every digit pass, as PAIRS does with
// its one, would cost two LDS round trips per array and pass and a register array each.  Instead the KEYS are sorted first (as in
// the keys-only kernel, remembering each element's slot after the first pass), the second pass's slots are left in LDS indexed by
// position, and one random LDS read per element composes the two: final[i] = slot2[slot1[i]].  Each payload array then takes ONE
// trip: loaded in position order, written to its elements' final slots, stored linearly -- in place, the bucket being this
// workgroup's alone (every load of an array is in registers before the barrier that precedes its first store).  At most two
// digit passes (the hybrid form's local stage has two).
template <int K>
__device__ __forceinline__ void sort_bucket_multi(const LocalSortParams& p, const uint32_t b)
{
    const uint32_t lo = p.bases[b];
    const uint32_t size = bucket_size<K>(p, lo, p.bases[b + 1]);
    if (size == 0u) return;
    const LocalGroup<K> g = local_group<K>(size);
    uint32_t* const bucket = p.keys + lo;
    uint32_t key[K], slot[K], first_slot[K];
    load_rows(g, bucket, key);
    uint32_t sh0 = p.shift[0], wd0 = p.width[0], sh1 = p.shift[1], wd1 = p.width[1];
    if (p.low_bits_word) {   // the hybrid form: bits [0, low), nine first (see sort_bucket)
        const uint32_t low = *p.low_bits_word;
        sh0 = 0u; wd0 = low < 9u ? low : 9u;
        sh1 = wd0; wd1 = low - wd0;
    }
    digit_pass<K, true>(g, key, slot, sh0, wd0);
    if (wd1) {
#pragma unroll
        for (int i = 0; i < K; i++) first_slot[i] = slot[i];
        read_rows(g, key);
        digit_pass<K, true>(g, key, slot, sh1, wd1);
    }
    store_linear(g, bucket);   // the keys are done
    if (wd1) {
        __syncthreads();   // the keys have left the LDS: it now holds the second pass's slots by position ...
#pragma unroll
        for (int i = 0; i < K; i++)
            if ((uint32_t)i < g.live) g.s_keys[g.wbase + (uint32_t)i * 64u] = slot[i];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < K; i++)   // ... and the element that started at position wbase + 64 i ends in slot2[slot1]
            if ((uint32_t)i < g.live) slot[i] = g.s_keys[first_slot[i]];   // (a padding lane: its own position both times)
    }
    for (uint32_t e = 0; e < p.num_payloads; e++) {
        uint32_t* const pay = (e == 0 ? p.vals : p.more[e - 1]) + lo;
        __syncthreads();   // the LDS is free again (slots read, or the previous array stored)
        load_rows(g, pay, key);
        write_slots(g, slot, key);
        __syncthreads();
        store_linear(g, pay);
    }
}

template <int K>
__global__ void __launch_bounds__(kLocalThreads, (K <= 16 ? 6 : 2)) local_sort_multi_kernel(const LocalSortParams p)
{
    if (p.skip && *p.skip != 0u) return;
    sort_bucket_multi<K>(p, blockIdx.x);
}

// the planner's list, walked by a small grid (a kernel of its own: with both uses in one kernel the body is inlined twice and spills)
template <int K>
__global__ void __launch_bounds__(kLocalThreads, (K <= 16 ? 6 : 2)) local_sort_multi_list_kernel(const LocalSortParams p)
{
    if (p.skip && *p.skip != 0u) return;
    const uint32_t listed = *p.list_count;
    for (uint32_t item = blockIdx.x; item < listed; item += gridDim.x) {
        sort_bucket_multi<K>(p, p.list[item]);
        __syncthreads();
    }
}

// registers: three workgroups per CU need 80 or fewer (keys K <= 20; pairs K <= 16), two 128; the 16384-pair variant keeps three
// arrays of 32 and gets 256 (one workgroup per CU: it only ever sees the planner's list of outsized buckets)
template <int K, bool PAIRS>
constexpr int local_waves_per_simd() { return K <= 10 ? 8 : (PAIRS ? K <= 16 : K <= 20) ? 6 : (PAIRS ? 2 : 4); }

// one bucket per workgroup
template <int K, bool PAIRS, bool XOUT>
__global__ void __launch_bounds__(kLocalThreads, (local_waves_per_simd<K, PAIRS>())) local_sort_kernel(const LocalSortParams p)
{
    if (p.skip && *p.skip != 0u) return;   // uniform: the plan took the other form
    sort_bucket<K, PAIRS, XOUT>(p, blockIdx.x);
}

// The buckets of the planner's list (those above the small variant's capacity), dealt over a small grid: uniform keys leave
// the list empty, and a launch of 32768 workgroups that each find nothing to do costs 17 us.
template <int K, bool PAIRS, bool XOUT>
__global__ void __launch_bounds__(kLocalThreads, (local_waves_per_simd<K, PAIRS>())) local_sort_list_kernel(const LocalSortParams p)
{
    if (p.skip && *p.skip != 0u) return;
    const uint32_t listed = *p.list_count;
    for (uint32_t item = blockIdx.x; item < listed; item += gridDim.x) {
        sort_bucket<K, PAIRS, XOUT>(p, p.list[item]);
        __syncthreads();   // the next bucket reuses the LDS
    }
}

// One workgroup per bucket, or (the list is the large variant's: K = 32) a small grid that walks the planner's list: 512
// workgroups, two per CU; 256 with several payload arrays (three register arrays of 32: one workgroup per CU, as the pairs').
template <int K>
static hipError_t launch_local_multi(const LocalSortParams& p, hipStream_t stream)
{
    constexpr size_t lds_bytes = local_lds_words<K>() * sizeof(uint32_t);
    const dim3 block(kLocalThreads);
    if (!p.list) return launch_dynamic_lds<local_sort_multi_kernel<K>>(dim3(p.num_buckets), block, lds_bytes, stream, p);
    if constexpr (K == 32) return launch_dynamic_lds<local_sort_multi_list_kernel<K>>(dim3(256), block, lds_bytes, stream, p);
    return hipErrorInvalidValue;
}
template <int K, bool PAIRS, bool XOUT>
static hipError_t launch_local_inst_x(const LocalSortParams& p, hipStream_t stream)
{
    constexpr size_t lds_bytes = local_lds_words<K>() * sizeof(uint32_t);
    const dim3 block(kLocalThreads);
    if (!p.list) return launch_dynamic_lds<local_sort_kernel<K, PAIRS, XOUT>>(dim3(p.num_buckets), block, lds_bytes, stream, p);
    if constexpr (K == 32) return launch_dynamic_lds<local_sort_list_kernel<K, PAIRS, XOUT>>(dim3(512), block, lds_bytes, stream, p);
    return hipErrorInvalidValue;
}
template <int K, bool PAIRS>
static hipError_t launch_local_inst(const LocalSortParams& p, hipStream_t stream)
{
    return p.xout.on ? launch_local_inst_x<K, PAIRS, true>(p, stream) : launch_local_inst_x<K, PAIRS, false>(p, stream);
}

// A sort of up to 16384 items is one workgroup's work: one launch instead of the eight of the chained form (whose kernels are
// all latency at this size: 39 us for 2^14 keys).
template <bool PAIRS>
__global__ void __launch_bounds__(kLocalThreads, (PAIRS ? 2 : 4)) small_sort_kernel(const LocalSortParams p, uint32_t* clear0, uint32_t* clear1)
{
    if (threadIdx.x == 0) {
        if (clear0) *clear0 = 0u;
        if (clear1) *clear1 = 0u;
    }
    sort_bucket<32, PAIRS, false, true>(p, 0u);
}

hipError_t launch_small_sort(uint32_t* keys, uint32_t* vals, uint32_t n, uint32_t* clear0, uint32_t* clear1, hipStream_t stream)
{
    if (!keys || n == 0 || n > (uint32_t)kLocalSortCap) return hipErrorInvalidValue;
    LocalSortParams p{};
    p.keys = keys;
    p.vals = vals;
    p.num_buckets = n;                                  // WHOLE: the array's length
    for (int i = 0; i < 4; i++) {
        p.shift[i] = 8u * (uint32_t)i;
        p.width[i] = 8u;
    }
    constexpr size_t lds_bytes = local_lds_words<32>() * sizeof(uint32_t);
    const dim3 block(kLocalThreads);
    if (vals) return launch_dynamic_lds<small_sort_kernel<true>>(dim3(1), block, lds_bytes, stream, p, clear0, clear1);
    return launch_dynamic_lds<small_sort_kernel<false>>(dim3(1), block, lds_bytes, stream, p, clear0, clear1);
}

hipError_t launch_local_sort(const LocalSortParams& p, hipStream_t stream)
{
    if (p.num_buckets == 0) return hipSuccess;
    if (!p.keys || !p.bases || (p.width[0] == 0 && !p.low_bits_word)) return hipErrorInvalidValue;
    for (int i = 0; i < 3; i++)
        if (p.width[i] > 9 || (p.width[i] && p.shift[i] + p.width[i] > 32)) return hipErrorInvalidValue;
    if (p.width[3]) return hipErrorInvalidValue;   // a fourth pass is launch_small_sort's
    if ((p.list == nullptr) != (p.list_count == nullptr)) return hipErrorInvalidValue;
    if (p.small_variant && p.list) return hipErrorInvalidValue;   // the list is the large variant's
    if (p.num_payloads > 3 || (p.num_payloads > 0 && !p.vals)) return hipErrorInvalidValue;
    // halves are read by the 10240-key keys-only kernel alone, in its device-planned form
    if (p.halves && (p.small_variant != 1 || p.vals || p.xout.on || p.list || !p.low_bits_word || !p.first || !p.high_word || !p.prefix_word))
        return hipErrorInvalidValue;
    if (p.num_payloads > 1) {   // records: several payload arrays
        if (p.width[2] || p.xout.on || !p.more[0] || (p.num_payloads > 2 && !p.more[1])) return hipErrorInvalidValue;
        return p.small_variant ? launch_local_multi<16>(p, stream) : launch_local_multi<32>(p, stream);
    }
    if (p.small_variant == 2) {
        if (p.vals) return launch_local_inst<kLocalSortCapTiny / kLocalThreads, true>(p, stream);
        return launch_local_inst<kLocalSortCapTiny / kLocalThreads, false>(p, stream);
    }
    if (p.vals) {
        if (p.small_variant) return launch_local_inst<kLocalSortCapSmallPairs / kLocalThreads, true>(p, stream);
        return launch_local_inst<32, true>(p, stream);
    }
    if (p.small_variant) return launch_local_inst<kLocalSortCapSmall / kLocalThreads, false>(p, stream);
    return launch_local_inst<32, false>(p, stream);
}


// ---- the segmented sort's workgroup tier (segmented.hip plans it) -------------------------------------------------------------
// Segment s = keys [offsets[s], offsets[s + 1]), kWaveSegCap < size <= kLocalSortCap, listed by the planner.  The digit pass above
// (16384-key variant) over the four bytes of the key, plus what a segment needs that a bucket of the hybrid form does not: the
// key transform on load as well as on store, and no pass for a byte that is the same in every key of the segment (AND and OR of
// the keys agree on it: small key ranges, one value per segment).
template <bool PAIRS>
__device__ __forceinline__ void sort_segment(const SegSortParams& p, const uint32_t s)
{
    constexpr int K = 32;
    if (s >= p.num_segments) return raise_fault(p.fault, 128u);   // never listed: say so, touch nothing
    const uint32_t lo = p.offsets[s], hi = p.offsets[s + 1];
    if (hi < lo || hi > p.n || hi - lo > (uint32_t)(kLocalThreads * K)) return raise_fault(p.fault, 128u);
    const LocalGroup<K> g = local_group<K, false>(hi - lo);
    uint32_t* const seg = p.keys + lo;
    uint32_t* const seg_vals = PAIRS ? p.vals + lo : nullptr;

    uint32_t key[K], rank[K], val[K];   // val: PAIRS only
    uint32_t any = 0u, all = ~0u;
#pragma unroll
    for (int i = 0; i < K; i++) {
        key[i] = 0xFFFFFFFFu;   // past the segment: the highest digit in every pass, stays last, never stored
        if ((uint32_t)i < g.rows) {
            const uint32_t pos = g.wbase + (uint32_t)i * 64u;
            if (pos < g.size) {
                uint32_t k = seg[pos];
                if (p.xin.on) k = to_sortable(k, p.xin);
                key[i] = k;
                any |= k;
                all &= k;
            }
            if (PAIRS) val[i] = pos < g.size ? seg_vals[pos] : 0u;
        }
    }
    any = wave_or(any);
    all = wave_and(all);
    if (g.lane == 0u) {
        g.s_misc[32 + g.wave] = any;
        g.s_misc[40 + g.wave] = all;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kLocalWaves; w++) {
        any |= g.s_misc[32 + w];
        all &= g.s_misc[40 + w];
    }
    uint32_t todo = 0;   // bit b: byte b differs somewhere in the segment (uniform)
#pragma unroll
    for (int b = 0; b < 4; b++) todo |= (((any ^ all) >> (8 * b)) & 0xFFu) ? 1u << b : 0u;

    while (todo) {
        const uint32_t shift = 8u * (uint32_t)__builtin_ctz(todo);
        todo &= todo - 1u;
        digit_pass<K, PAIRS>(g, key, rank, shift, 8u);
        take_out<K, PAIRS>(g, todo == 0u, key, rank, val, seg, p.xout.on ? &p.xout : nullptr, seg_vals);
    }
}

template <bool PAIRS>
__global__ void __launch_bounds__(kLocalThreads, (local_waves_per_simd<32, PAIRS>())) segment_sort_kernel(const SegSortParams p)
{
    const uint32_t listed = *p.list_count < p.list_cap ? (uint32_t)*p.list_count : p.list_cap;
    for (uint32_t item = blockIdx.x; item < listed; item += gridDim.x) {
        sort_segment<PAIRS>(p, p.list[item]);
        __syncthreads();   // the next segment reuses the LDS
    }
}

hipError_t launch_segment_sort(const SegSortParams& p, uint32_t grid, hipStream_t stream)
{
    constexpr size_t lds_bytes = local_lds_words<32>() * sizeof(uint32_t);
    if (!p.keys || !p.offsets || !p.list || !p.list_count || grid == 0) return hipErrorInvalidValue;
    const dim3 block(kLocalThreads);
    if (p.vals) return launch_dynamic_lds<segment_sort_kernel<true>>(dim3(grid), block, lds_bytes, stream, p);
    return launch_dynamic_lds<segment_sort_kernel<false>>(dim3(grid), block, lds_bytes, stream, p);
}

}  // namespace lsd
