// topk16.hip -- the k best 16-bit keys of every row of a [rows x cols] array, with their positions (lsdsort_topk16_device;
// DESIGN.md section 6.6).  The 16-bit sibling of topk.hip: same contract, same three steps, same size classes.
//
// No counterpart in the reference (it sorts one whole array of uint32, LSDRadixSort.cu:839-910).  Row r's result is the first k
// items of the stable sort of the row in the requested order.  "Best" is always "smallest sortable value": the map of
// keys16_map.hpp (to_sortable16, with the complement for largest) is applied where a key is read.
//
//   select   as in topk.hip, on 16 bits: state per row (prefix, shift, need); key t wins if (t >> shift) < prefix, or if
//            (t >> shift) == prefix and fewer than `need` such keys stand before it in the row.  At most TWO digit levels.
//   compact  the winners go to the WORKSPACE in position order, as uint32 words (the sortable value in the low half-word, the high
//            half-word zero) with their positions beside them: slot = winners before it in the row.
//   sort     those rows x k words are sorted by the segmented sort as uint32 ascending, rows as segments, positions as payload:
//            stable, and its tiers of up to 16384 keys skip the two dead high digits on their own.  k = 1 needs no sort.
//   finish   one small kernel un-maps, narrows into d_out_keys and copies the positions into d_out_idx.
//
// Key reads.  A row starts 2 r cols bytes past d_keys, at any even offset within a 16-byte line.  Every kernel therefore splits
// EACH ROW by address (Row): `head` keys in front of the row's first 16-byte line (0..7), read one by one, and the `body` from that
// line on, read as 16-byte groups of eight keys; the last group of a row (or chunk) that is not whole is read one by one too.
// A lane holds two groups of a tile of its wave: register 8 j + e is body position q0 + 8 (64 j + lane) + e.  A key that does not
// exist is kNoKey, which no (prefix, shift) of a select matches.
// Size classes (those of topk.hip, by cols):
//   cols <= kWaveSegCap (1024)      one wavefront per row: the row in its registers, two rounds of 8-bit digits in its LDS slice
//   cols <= kLocalSortCap (16384)   one workgroup per row: the same with 16 wavefronts
//   longer                          many workgroups per row (chunks of body positions): digits of 11 then 5 bits counted in LDS,
//                                   flushed into [row][2048] by global atomics, one workgroup per row walks the bins between the
//                                   reads; then per-chunk counts of "better" and "equal" and the ordered write.  At most four
//                                   reads of the row (8 B/key), one fewer where the select stops after the first level.  A chunk
//                                   without winners is not read by the write pass.  Chunk 0 also owns the row's head.
//   k above kLargeKNum / kLargeKDen of cols: the rows are widened into the workspace with their positions, sorted whole by the
//                                   segmented sort, and the first k of each are taken.  The 3/4 is topk.hip's, NOT tuned for
//                                   2-byte keys.
// Every launch is sized from (rows, cols, k); phases are ordered by kernel boundaries; every store of a winner is guarded by
// slot < k (counts that do not describe the keys raise a fault bit instead -- never expected).
#define LSDSORT_BUILD 1
#include "../../include/lsdsort.h"

#include "keys16_map.hpp"
#include "lsd_device.hpp"
#include "lsd_host.hpp"

namespace lsd {
namespace {

constexpr size_t kLargeKNum = 3, kLargeKDen = 4;   // topk.hip's threshold of the sort route, inherited

constexpr uint32_t kTopkFaultCount = 1024u;   // fault word: the digit counts of a row do not reach k (never expected)
constexpr uint32_t kTopkFaultDest = 2048u;    // fault word: a winner's slot is not below k (never expected; not stored)
constexpr size_t kCtlBytes = 256;
constexpr int kRegs = 16;                     // keys per lane of a tile: two groups of eight
constexpr uint32_t kWaveTile = 64u * kRegs;   // body positions of one wave's tile
constexpr uint32_t kNoKey = 0xFFFFFFFFu;      // a sortable value is below 65536
constexpr uint32_t kBins = 2048;              // long rows: counters per row (the 11-bit level)
constexpr uint32_t kLowBits = 5;              // long rows: the second level
constexpr uint32_t kLongThreads = 256, kLongWaves = kLongThreads / kWave, kLongTile = kLongThreads * kRegs;
constexpr uint32_t kMinChunk = 16384, kMaxChunks = 2048;
constexpr int kPlainThreads = 256;

size_t max_sz(size_t a, size_t b) { return a > b ? a : b; }

template <int WAVES>
__device__ __forceinline__ void group_sync()
{
    if (WAVES == 1) wave_sync();
    else __syncthreads();
}

// One row by address: key p of the row is keys[p]; keys [0, head) lie in front of the row's first 16-byte line, the `body` keys
// from there on are keys[head + q], q < body, and q = 8 g is the start of a 16-byte line.
struct Row {
    const uint16_t* keys;
    uint32_t head, body;
};
__device__ __forceinline__ Row row_of(const uint16_t* keys, uint32_t row, uint32_t cols)
{
    Row r;
    r.keys = keys + (size_t)row * cols;
    const uint32_t to_line = ((16u - ((uint32_t)(uintptr_t)r.keys & 15u)) & 15u) / (uint32_t)sizeof(uint16_t);
    r.head = to_line < cols ? to_line : cols;
    r.body = cols - r.head;
    return r;
}

// The wave's tile from body position q0 on, valid below `end`: a whole group by one 16-byte load, the others key by key.
__device__ __forceinline__ void load_tile(const Row& r, uint32_t q0, uint32_t end, uint32_t lane, const Key16Map& m, uint32_t (&t)[kRegs])
{
#pragma unroll
    for (int j = 0; j < kRegs / 8; j++) {
        const uint32_t q = q0 + ((uint32_t)j * 64u + lane) * kGroupKeys;
        if (q < end && end - q >= kGroupKeys) {
            const uint4 v = *reinterpret_cast<const uint4*>(r.keys + r.head + q);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                t[8 * j + 2 * i] = to_sortable16(w[i] & 0xFFFFu, m);
                t[8 * j + 2 * i + 1] = to_sortable16(w[i] >> 16, m);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; e++) {
                t[8 * j + e] = kNoKey;
                if (q + (uint32_t)e < end) t[8 * j + e] = to_sortable16(r.keys[r.head + q + (uint32_t)e], m);
            }
        }
    }
}
// head key `lane` of the row, for the one wave that owns the head
__device__ __forceinline__ uint32_t load_head(const Row& r, uint32_t lane, const Key16Map& m)
{
    return lane < r.head ? to_sortable16(r.keys[lane], m) : kNoKey;
}

struct Winners {
    uint32_t* keys;       // [rows][k] in the workspace: sortable values as uint32
    uint32_t* pos;        // [rows][k] positions, null where the caller wants none
    uint32_t rows, k;
    uint32_t* fault;
};

// Ordered write of one tile held in registers (load_tile at q0), and with `has_head` (uniform; the first tile of wave 0 of the
// row) of the head keys `h` in front of it.  base_b / base_e: the better / equal keys of the row before this tile; both move on
// past it.  s_wc: 2 WAVES words.  A lane's counts travel packed: better in the low half-word, equal in the high one.
template <int WAVES>
__device__ __forceinline__ void compact_tile(const uint32_t (&t)[kRegs], uint32_t h, bool has_head, uint32_t q0, const Row& r,
                                             uint32_t prefix, uint32_t shift, uint32_t need, uint32_t& base_b, uint32_t& base_e,
                                             volatile lds_u32* s_wc, uint32_t wave, uint32_t lane, uint32_t row, const Winners& o)
{
    auto packed = [&](uint32_t key) {
        const uint32_t top = key >> shift;
        return (top < prefix ? 1u : 0u) | (top == prefix ? 0x10000u : 0u);
    };
    uint32_t c[kRegs / 8];
    const uint32_t ch = has_head ? packed(h) : 0u;
    uint32_t sum = ch;
#pragma unroll
    for (int j = 0; j < kRegs / 8; j++) {
        c[j] = 0u;
#pragma unroll
        for (int e = 0; e < 8; e++) c[j] += packed(t[8 * j + e]);
        sum += c[j];
    }
    sum = wave_sum(sum);
    const uint32_t nb = sum & 0xFFFFu, ne = sum >> 16;
    uint32_t my_b = base_b, my_e = base_e, all_b = nb, all_e = ne;
    if (WAVES > 1) {
        if (lane == 0u) {
            s_wc[2u * wave] = nb;
            s_wc[2u * wave + 1u] = ne;
        }
        __syncthreads();
        all_b = 0u;
        all_e = 0u;
        for (uint32_t w = 0; w < (uint32_t)WAVES; w++) {
            const uint32_t b = s_wc[2u * w], e = s_wc[2u * w + 1u];
            if (w < wave) {
                my_b += b;
                my_e += e;
            }
            all_b += b;
            all_e += e;
        }
        __syncthreads();   // the next tile writes s_wc again
    }
    // (uniform) a tile without winners writes nothing
    if (all_b != 0u || (all_e != 0u && base_e < need)) {
        auto emit = [&](uint32_t key, uint32_t pos, uint32_t& b_before, uint32_t& e_before) {
            const uint32_t top = key >> shift;
            const bool better = top < prefix, equal = top == prefix;
            if (better || (equal && e_before < need)) {
                const uint32_t slot = b_before + (e_before < need ? e_before : need);
                if (slot < o.k && row < o.rows) {
                    const size_t at = (size_t)row * o.k + slot;
                    o.keys[at] = key;
                    if (o.pos) o.pos[at] = pos;
                } else {
                    atomicOr(o.fault, kTopkFaultDest);
                }
            }
            b_before += better ? 1u : 0u;
            e_before += equal ? 1u : 0u;
        };
        if (has_head) {   // uniform
            const uint32_t incl = wave_inclusive_scan(ch), excl = incl - ch;
            uint32_t b_before = my_b + (excl & 0xFFFFu), e_before = my_e + (excl >> 16);
            emit(h, lane, b_before, e_before);
            const uint32_t all = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            my_b += all & 0xFFFFu;
            my_e += all >> 16;
        }
#pragma unroll
        for (int j = 0; j < kRegs / 8; j++) {
            const uint32_t incl = wave_inclusive_scan(c[j]), excl = incl - c[j];
            uint32_t b_before = my_b + (excl & 0xFFFFu), e_before = my_e + (excl >> 16);
            const uint32_t pos = r.head + q0 + ((uint32_t)j * 64u + lane) * kGroupKeys;
#pragma unroll
            for (int e = 0; e < 8; e++) emit(t[8 * j + e], pos + (uint32_t)e, b_before, e_before);
            const uint32_t all = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            my_b += all & 0xFFFFu;
            my_e += all >> 16;
        }
    }
    base_b += all_b;
    base_e += all_e;
}

// ---- short rows: one wavefront (WAVES = 1, eight rows per workgroup) or one workgroup (WAVES = 16) per row ----------------------
struct ShortParams {
    const uint16_t* keys;
    uint32_t cols;
    Key16Map map;
    Winners out;
};

template <int WAVES>
__global__ void __launch_bounds__(WAVES == 1 ? 512 : 1024) topk16_short_kernel(const ShortParams p)
{
    constexpr int kGroups = WAVES == 1 ? 8 : 1;          // rows in flight per workgroup
    constexpr int kSlice = 256 + 8 + 2 * WAVES;          // per row: digit counters, the found bin, per-wave counts
    __shared__ uint32_t smem[kGroups * kSlice];
    const uint32_t lane = threadIdx.x & 63u, wave_of_block = threadIdx.x >> 6;
    const uint32_t group = WAVES == 1 ? wave_of_block : 0u, wave = WAVES == 1 ? 0u : wave_of_block;
    volatile lds_u32* const s_cnt = (volatile lds_u32*)((lds_u32*)smem + group * kSlice);
    volatile lds_u32* const s_found = s_cnt + 256;
    volatile lds_u32* const s_wc = s_cnt + 264;
    // `row` is the same for every thread of a group (a wave, or the whole workgroup): its barriers are reached together
    for (uint32_t row = blockIdx.x * kGroups + group; row < p.out.rows; row += gridDim.x * kGroups) {
        const Row r = row_of(p.keys, row, p.cols);
        const uint32_t q0 = wave * kWaveTile;
        uint32_t t[kRegs];
        load_tile(r, q0, r.body, lane, p.map, t);
        const uint32_t h = wave == 0u ? load_head(r, lane, p.map) : kNoKey;
        uint32_t prefix = 0u, shift = 8u, need = p.out.k;
#pragma unroll 1
        for (int round = 0; round < 2; round++) {
            shift = 8u - 8u * (uint32_t)round;
            if (wave == 0u) {
#pragma unroll
                for (int j = 0; j < 4; j++) s_cnt[j * 64 + lane] = 0u;
                if (lane == 0u) s_found[0] = 0xFFFFFFFFu;
            }
            group_sync<WAVES>();
            // round 0: every key there is; round 1: those whose top byte is the prefix (kNoKey never is)
            auto count = [&](uint32_t key) {
                const bool match = round == 0 ? key != kNoKey : (key >> 8) == prefix;
                if (match)
                    __hip_atomic_fetch_add((lds_u32*)&s_cnt[(key >> shift) & 0xFFu], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            };
#pragma unroll
            for (int i = 0; i < kRegs; i++) count(t[i]);
            count(h);
            group_sync<WAVES>();
            if (wave == 0u) {   // four bins per lane, from the best end
                uint32_t c[4], sum = 0u;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    c[j] = s_cnt[lane * 4u + j];
                    sum += c[j];
                }
                uint32_t run = wave_inclusive_scan(sum) - sum;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    if (run < need && need - run <= c[j]) {   // at most one bin of the row
                        s_found[0] = lane * 4u + j;
                        s_found[1] = run;
                        s_found[2] = c[j];
                    }
                    run += c[j];
                }
            }
            group_sync<WAVES>();
            const uint32_t bin = s_found[0], before = s_found[1], count_in_bin = s_found[2];
            group_sync<WAVES>();   // the next round writes s_found again
            if (bin > 0xFFu) {     // (uniform) the counts do not reach k: nothing is selected
                if (wave == 0u && lane == 0u) atomicOr(p.out.fault, kTopkFaultCount);
                prefix = 0u;
                shift = 0u;
                need = 0u;
                break;
            }
            prefix = (prefix << 8) | bin;
            need -= before;
            if (count_in_bin == need) break;   // (uniform) the remainder is decided: every key under the prefix wins
        }
        uint32_t base_b = 0u, base_e = 0u;
        compact_tile<WAVES>(t, h, wave == 0u, q0, r, prefix, shift, need, base_b, base_e, s_wc, wave, lane, row, p.out);
        group_sync<WAVES>();
    }
}

// ---- long rows ------------------------------------------------------------------------------------------------------------------
// Row state in the workspace (uint4): x prefix, y shift (16: no level has run), z need, w done (the select stopped).
struct LongParams {
    const uint16_t* keys;
    uint32_t cols;
    uint32_t chunk, chunks;       // body positions per chunk (a multiple of kLongTile), chunks per row
    uint32_t chunk_cap;           // row stride of `counts`
    uint4* state;
    uint32_t* hist;               // [rows][kBins], zero on entry to every level
    uint2* counts;                // [rows][chunk_cap]: better, equal per chunk
    Key16Map map;
    Winners out;
};

// Chunk c of a row is body positions [lo, hi) -- in EVERY kernel below -- and chunk 0 owns the head keys as well.  A row whose
// head is not empty may leave its last chunk empty (lo == hi): the chunks are counted from cols.
struct ChunkRange {
    uint32_t lo, hi;
};
__device__ __forceinline__ ChunkRange chunk_of(const Row& r, const LongParams& p, uint32_t c)
{
    ChunkRange g;
    g.lo = c * p.chunk < r.body ? c * p.chunk : r.body;
    g.hi = r.body - g.lo < p.chunk ? r.body : g.lo + p.chunk;
    return g;
}

// control block, counters and row states of a call (a kernel rather than memsets: one kind of node in a captured graph)
__global__ void __launch_bounds__(kPlainThreads) topk16_clear_kernel(uint32_t* ctl, uint32_t* hist, uint32_t hist_words, uint4* state,
                                                                    uint32_t rows, uint32_t k)
{
    const uint32_t at = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
    if (at < (uint32_t)(kCtlBytes / 4)) ctl[at] = 0u;
    for (uint32_t q = at; q < hist_words; q += step) hist[q] = 0u;
    if (state)
        for (uint32_t r = at; r < rows; r += step) state[r] = make_uint4(0u, 16u, k, 0u);
}

// One register of every lane into the LDS counters.  A wave whose matching keys all carry one digit (a shared prefix, few values,
// all equal -- 16-bit rows are full of runs) adds their number once instead of piling 64 adds onto one word.
__device__ __forceinline__ void count_digit(uint32_t* s_hist, bool match, uint32_t bin, uint32_t lane)
{
    const uint64_t m = __ballot(match);
    if (m == 0ull) return;   // uniform
    const uint32_t leader = (uint32_t)__builtin_ctzll(m);
    const uint32_t lead_bin = (uint32_t)__builtin_amdgcn_readlane((int)bin, (int)leader);
    if (__ballot(match && bin != lead_bin) == 0ull) {
        if (lane == leader) atomicAdd(&s_hist[lead_bin], popc64(m));
    } else if (match) {
        atomicAdd(&s_hist[bin], 1u);
    }
}

// One chunk of one row per workgroup: the digit of every key under the row's prefix, counted in LDS.  LEVEL 0: the top 11 bits
// of every key; LEVEL 1: the low 5 bits of the keys whose top 11 are the prefix.
template <int LEVEL>
__global__ void __launch_bounds__(kLongThreads) topk16_hist_kernel(const LongParams p)
{
    __shared__ uint32_t s_hist[kBins];
    const uint32_t row = blockIdx.x / p.chunks, c = blockIdx.x % p.chunks;
    if (row >= p.out.rows) return;
    const uint4 st = p.state[row];
    if (st.w != 0u) return;   // uniform
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t b = tid; b < kBins; b += kLongThreads) s_hist[b] = 0u;
    __syncthreads();
    const Row r = row_of(p.keys, row, p.cols);
    const ChunkRange g = chunk_of(r, p, c);
    auto count = [&](uint32_t key) {
        const bool match = LEVEL == 0 ? key != kNoKey : (key >> kLowBits) == st.x;
        const uint32_t bin = LEVEL == 0 ? (key >> kLowBits) & (kBins - 1u) : key & ((1u << kLowBits) - 1u);
        count_digit(s_hist, match, bin, lane);
    };
    if (c == 0u && wave == 0u) count(load_head(r, lane, p.map));   // uniform
    for (uint32_t tile = g.lo; tile < g.hi; tile += kLongTile) {   // uniform
        uint32_t t[kRegs];
        load_tile(r, tile + wave * kWaveTile, g.hi, lane, p.map, t);
#pragma unroll
        for (int i = 0; i < kRegs; i++) count(t[i]);
    }
    __syncthreads();
    uint32_t* const out = p.hist + (size_t)row * kBins;
    for (uint32_t b = tid; b < kBins; b += kLongThreads) {
        const uint32_t v = s_hist[b];
        if (v != 0u) atomicAdd(out + b, v);
    }
}

// One workgroup per row: walk the bins from the best end to the one that holds the k-th key; the counters go back to zero.
template <int LEVEL>
__global__ void __launch_bounds__(256) topk16_scan_kernel(const LongParams p)
{
    __shared__ uint32_t s_part[4];
    __shared__ uint32_t s_found[3];
    const uint32_t row = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (row >= p.out.rows) return;
    const uint4 st = p.state[row];
    if (st.w != 0u) return;   // uniform
    uint32_t* const h = p.hist + (size_t)row * kBins;
    constexpr uint32_t E = kBins / 256u;
    uint32_t c[E], sum = 0u;
#pragma unroll
    for (uint32_t e = 0; e < E; e++) {
        c[e] = h[tid * E + e];
        h[tid * E + e] = 0u;
        sum += c[e];
    }
    if (tid == 0u) s_found[0] = 0xFFFFFFFFu;
    uint32_t run = group_exclusive_scan<4>(sum, lane, wave, s_part);
    const uint32_t need = st.z;
#pragma unroll
    for (uint32_t e = 0; e < E; e++) {
        if (run < need && need - run <= c[e]) {   // at most one bin of the row
            s_found[0] = tid * E + e;
            s_found[1] = run;
            s_found[2] = c[e];
        }
        run += c[e];
    }
    __syncthreads();
    if (tid != 0u) return;
    const uint32_t bin = s_found[0], before = s_found[1], count = s_found[2];
    if (bin >= (LEVEL == 0 ? kBins : 1u << kLowBits)) {   // the counts do not reach k: nothing is selected
        atomicOr(p.out.fault, kTopkFaultCount);
        p.state[row] = make_uint4(0u, 0u, 0u, 1u);
        return;
    }
    const uint32_t prefix = LEVEL == 0 ? bin : ((st.x << kLowBits) | bin);
    const uint32_t left = need - before;
    p.state[row] = make_uint4(prefix, LEVEL == 0 ? kLowBits : 0u, left, (LEVEL == 1 || count == left) ? 1u : 0u);
}

// better / equal keys of every chunk
__global__ void __launch_bounds__(kLongThreads) topk16_count_kernel(const LongParams p)
{
    __shared__ uint32_t s_part[2 * kLongWaves];
    const uint32_t row = blockIdx.x / p.chunks, c = blockIdx.x % p.chunks;
    if (row >= p.out.rows) return;
    const uint4 st = p.state[row];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const Row r = row_of(p.keys, row, p.cols);
    const ChunkRange g = chunk_of(r, p, c);
    uint32_t nb = 0u, ne = 0u;
    if (st.y < 16u) {
        auto count = [&](uint32_t key) {
            const uint32_t top = key >> st.y;
            nb += top < st.x ? 1u : 0u;
            ne += top == st.x ? 1u : 0u;
        };
        if (c == 0u && wave == 0u) count(load_head(r, lane, p.map));   // uniform
        for (uint32_t tile = g.lo; tile < g.hi; tile += kLongTile) {   // uniform
            uint32_t t[kRegs];
            load_tile(r, tile + wave * kWaveTile, g.hi, lane, p.map, t);
#pragma unroll
            for (int i = 0; i < kRegs; i++) count(t[i]);
        }
    }
    nb = wave_sum(nb);
    ne = wave_sum(ne);
    if (lane == 0u) {
        s_part[2u * wave] = nb;
        s_part[2u * wave + 1u] = ne;
    }
    __syncthreads();
    if (tid == 0u) {
        uint32_t b = 0u, e = 0u;
        for (uint32_t w = 0; w < kLongWaves; w++) {
            b += s_part[2u * w];
            e += s_part[2u * w + 1u];
        }
        p.counts[(size_t)row * p.chunk_cap + c] = make_uint2(b, e);
    }
}

// the ordered write: the chunk's winners go to slots that follow those of the chunks before it
__global__ void __launch_bounds__(kLongThreads) topk16_write_kernel(const LongParams p)
{
    __shared__ uint32_t s_part[2 * kLongWaves];
    __shared__ uint32_t s_wc_raw[2 * kLongWaves];
    const uint32_t row = blockIdx.x / p.chunks, c = blockIdx.x % p.chunks;
    if (row >= p.out.rows) return;
    const uint4 st = p.state[row];
    if (st.y >= 16u) return;   // (uniform) a row no scan has visited: never
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint2* const counts = p.counts + (size_t)row * p.chunk_cap;
    uint32_t base_b = 0u, base_e = 0u;
    for (uint32_t q = tid; q < c; q += kLongThreads) {
        const uint2 v = counts[q];
        base_b += v.x;
        base_e += v.y;
    }
    base_b = wave_sum(base_b);
    base_e = wave_sum(base_e);
    if (lane == 0u) {
        s_part[2u * wave] = base_b;
        s_part[2u * wave + 1u] = base_e;
    }
    __syncthreads();
    base_b = 0u;
    base_e = 0u;
    for (uint32_t w = 0; w < kLongWaves; w++) {
        base_b += s_part[2u * w];
        base_e += s_part[2u * w + 1u];
    }
    const uint2 mine = counts[c];
    if (mine.x == 0u && (mine.y == 0u || base_e >= st.z)) return;   // (uniform) no winner in this chunk: it is not read again
    const Row r = row_of(p.keys, row, p.cols);
    const ChunkRange g = chunk_of(r, p, c);
    volatile lds_u32* const s_wc = (volatile lds_u32*)(lds_u32*)s_wc_raw;
    // chunk 0 has at least one tile (a long row's body is longer than its head), and its first tile carries the head
    for (uint32_t tile = g.lo; tile < g.hi; tile += kLongTile) {   // uniform
        const uint32_t q0 = tile + wave * kWaveTile;
        const bool has_head = c == 0u && tile == g.lo && wave == 0u;
        uint32_t t[kRegs];
        load_tile(r, q0, g.hi, lane, p.map, t);
        const uint32_t h = has_head ? load_head(r, lane, p.map) : kNoKey;
        compact_tile<(int)kLongWaves>(t, h, has_head, q0, r, st.x, st.y, st.z, base_b, base_e, s_wc, wave, lane, row, p.out);
    }
}

// ---- plumbing -------------------------------------------------------------------------------------------------------------------
// off[r] = r * stride, r <= rows: the rows as segments
__global__ void __launch_bounds__(kPlainThreads) topk16_offsets_kernel(uint32_t* off, uint32_t rows, uint32_t stride)
{
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r <= rows; r += gridDim.x * blockDim.x) off[r] = r * stride;
}

// The sort route: every key of the array widened to its sortable value, with its position in its row beside it.  The array as a
// whole is one Span here (the rows lie back to back); `wide` and `idx` are 256-byte aligned, so the eight words of a group lie on
// 16-byte lines where the head is a multiple of four keys (wide_vec).
__global__ void __launch_bounds__(kPlainThreads) topk16_widen_kernel(const uint16_t* __restrict__ keys, Span sp, uint32_t wide_vec, uint32_t cols,
                                                                    Key16Map m, uint32_t* __restrict__ wide, uint32_t* __restrict__ idx)
{
    const uint32_t tid = threadIdx.x;
    auto one = [&](uint32_t q) {
        wide[q] = to_sortable16(keys[q], m);
        if (idx) idx[q] = q % cols;
    };
    if (blockIdx.x == 0) {
        if (tid < sp.head) one(tid);
        if (tid < sp.tail) one(first_tail_key(sp) + tid);
    }
    const uint4* body = body_of(keys, sp);
    for (uint32_t g = blockIdx.x * kPlainThreads + tid; g < sp.groups; g += gridDim.x * kPlainThreads) {
        const uint4 v = body[g];
        const uint32_t in[4] = {v.x, v.y, v.z, v.w};
        uint32_t t[kGroupKeys], at[kGroupKeys];
        const uint32_t q = sp.head + g * kGroupKeys;
        uint32_t col = q % cols;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            t[2 * i] = to_sortable16(in[i] & 0xFFFFu, m);
            t[2 * i + 1] = to_sortable16(in[i] >> 16, m);
        }
#pragma unroll
        for (uint32_t i = 0; i < kGroupKeys; i++) {
            at[i] = col;
            col = col + 1u == cols ? 0u : col + 1u;
        }
        if (wide_vec) {
            reinterpret_cast<uint4*>(wide + q)[0] = make_uint4(t[0], t[1], t[2], t[3]);
            reinterpret_cast<uint4*>(wide + q)[1] = make_uint4(t[4], t[5], t[6], t[7]);
            if (idx) {
                reinterpret_cast<uint4*>(idx + q)[0] = make_uint4(at[0], at[1], at[2], at[3]);
                reinterpret_cast<uint4*>(idx + q)[1] = make_uint4(at[4], at[5], at[6], at[7]);
            }
        } else {
#pragma unroll
            for (uint32_t i = 0; i < kGroupKeys; i++) {
                wide[q + i] = t[i];
                if (idx) idx[q + i] = at[i];
            }
        }
    }
}

// Both routes end here: slot j of row r is word r * stride + j of `sorted` (stride k: the sorted winners; stride cols: the
// sorted rows).  Un-map, narrow, and the positions where the caller wants them.
__global__ void __launch_bounds__(kPlainThreads) topk16_finish_kernel(const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ pos,
                                                                     uint32_t stride, Key16Map m, uint16_t* __restrict__ out_keys,
                                                                     uint32_t* __restrict__ out_idx, uint32_t rows, uint32_t k)
{
    const uint32_t total = rows * k;
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < total; q += gridDim.x * blockDim.x) {
        const uint32_t row = q / k, slot = q - row * k;
        const size_t from = (size_t)row * stride + slot;
        out_keys[q] = (uint16_t)from_sortable16(sorted[from] & 0xFFFFu, m);
        if (out_idx) out_idx[q] = pos[from];
    }
}

bool sort_route(size_t cols, size_t k) { return k * kLargeKDen > cols * kLargeKNum; }

// Long rows are cut into chunks of a multiple of kLongTile keys, about kMaxChunks of them over the whole array.
struct Chunks {
    uint32_t chunk, per_row;
};
Chunks chunks_for(size_t rows, size_t cols)
{
    const size_t n = rows * cols;
    size_t chunk = max_sz(kMinChunk, (n + kMaxChunks - 1) / kMaxChunks);
    chunk = (chunk + kLongTile - 1) / kLongTile * kLongTile;
    return Chunks{(uint32_t)chunk, (uint32_t)((cols + chunk - 1) / chunk)};
}
size_t chunk_cap_for(size_t cols) { return min_sz(kMaxChunks, (cols + kMinChunk - 1) / kMinChunk); }

// Workspace.  Select route: control | row states | offsets | counters [rows][2048] | chunk counts | the winners as uint32 | their
// positions | segmented sort of rows x k pairs.  Sort route: control | offsets | the widened keys | their positions | segmented
// sort of rows x cols pairs.  The size is the larger of the two, the sort route's taken at the most keys a sort-route call with
// this (rows, k) can have: monotonic in each argument.  Sized for the call with indices.
struct Topk16Layout {
    size_t state, offsets, hist, counts, win, win_pos, seg, seg_bytes, total;   // select route
    size_t s_offsets, s_keys, s_idx, s_seg, s_seg_bytes, s_total;               // sort route, for `sort_keys` keys
};
Topk16Layout topk16_layout(size_t rows, size_t cols, size_t k, size_t sort_keys)
{
    Topk16Layout L{};
    const bool is_long = cols > (size_t)kLocalSortCap;
    const size_t winners = min_sz(rows * k, LSDSORT_MAX_KEYS);
    size_t off = kCtlBytes;
    L.state = off;    off = align_up(off + rows * 16);
    L.offsets = off;  off = align_up(off + (rows + 1) * 4);
    L.hist = off;     off = align_up(off + (is_long ? rows * kBins * 4 : 0));
    L.counts = off;   off = align_up(off + (is_long ? rows * chunk_cap_for(cols) * 8 : 0));
    L.win = off;      off = align_up(off + winners * 4);
    L.win_pos = off;  off = align_up(off + winners * 4);
    L.seg = off;
    L.seg_bytes = lsdsort_segmented_workspace_bytes(winners, rows, 1);
    L.total = align_up(off + L.seg_bytes);
    off = kCtlBytes;
    L.s_offsets = off;  off = align_up(off + (rows + 1) * 4);
    L.s_keys = off;     off = align_up(off + sort_keys * 4);
    L.s_idx = off;      off = align_up(off + sort_keys * 4);
    L.s_seg = off;
    L.s_seg_bytes = lsdsort_segmented_workspace_bytes(sort_keys, rows, 1);
    L.s_total = align_up(off + L.s_seg_bytes);
    return L;
}
size_t sort_route_keys(size_t rows, size_t cols, size_t k)
{
    // a call takes the sort route only if cols < 4 k / 3
    return min_sz(min_sz(rows * cols, rows * ((k * kLargeKDen + kLargeKNum - 1) / kLargeKNum)), LSDSORT_MAX_KEYS);
}

int run_topk16(const uint16_t* keys, size_t rows, size_t cols, size_t k, const Key16Map& map, uint16_t* out_keys, uint32_t* out_idx,
               char* ws, const Topk16Layout& L, hipStream_t stream)
{
    uint32_t* const ctl = reinterpret_cast<uint32_t*>(ws);
    const size_t n = rows * cols;
    const uint32_t finish_grid = grid_for(rows * k, 1024, 8192);

    if (sort_route(cols, k)) {
        uint32_t* const offsets = reinterpret_cast<uint32_t*>(ws + L.s_offsets);
        uint32_t* const wide = reinterpret_cast<uint32_t*>(ws + L.s_keys);
        uint32_t* const idx = out_idx ? reinterpret_cast<uint32_t*>(ws + L.s_idx) : nullptr;
        const Span sp = span_of(keys, n);
        hipLaunchKernelGGL(topk16_clear_kernel, dim3(1), dim3(kPlainThreads), 0, stream, ctl, (uint32_t*)nullptr, 0u, (uint4*)nullptr, 0u, 0u);
        hipLaunchKernelGGL(topk16_offsets_kernel, dim3(grid_for(rows + 1, 256, 1024)), dim3(kPlainThreads), 0, stream, offsets,
                           (uint32_t)rows, (uint32_t)cols);
        hipLaunchKernelGGL(topk16_widen_kernel, dim3(grid_for(sp.groups, kPlainThreads, 2048)), dim3(kPlainThreads), 0, stream, keys, sp,
                           (sp.head & 3u) == 0 ? 1u : 0u, (uint32_t)cols, map, wide, idx);
        LSD_HIP(hipGetLastError());
        LSD_TRY(lsdsort_segmented_device(wide, idx, offsets, rows, n, LSDSORT_KEY_U32, 0, ws + L.s_seg, L.s_seg_bytes, stream));
        hipLaunchKernelGGL(topk16_finish_kernel, dim3(finish_grid), dim3(kPlainThreads), 0, stream, static_cast<const uint32_t*>(wide),
                           static_cast<const uint32_t*>(idx), (uint32_t)cols, map, out_keys, out_idx, (uint32_t)rows, (uint32_t)k);
        LSD_HIP(hipGetLastError());
        LSD_HIP(launch_keep_fault(ctl, reinterpret_cast<const uint32_t*>(ws + L.s_seg), stream));
        return LSDSORT_OK;
    }

    uint32_t* const offsets = reinterpret_cast<uint32_t*>(ws + L.offsets);
    uint32_t* const win = reinterpret_cast<uint32_t*>(ws + L.win);
    uint32_t* const win_pos = out_idx ? reinterpret_cast<uint32_t*>(ws + L.win_pos) : nullptr;
    const Winners out{win, win_pos, (uint32_t)rows, (uint32_t)k, ctl};
    if (cols <= (size_t)kLocalSortCap) {
        ShortParams sp{keys, (uint32_t)cols, map, out};
        hipLaunchKernelGGL(topk16_clear_kernel, dim3(1), dim3(kPlainThreads), 0, stream, ctl, (uint32_t*)nullptr, 0u, (uint4*)nullptr, 0u, 0u);
        if (cols <= (size_t)kWaveSegCap)
            hipLaunchKernelGGL(topk16_short_kernel<1>, dim3(grid_for(rows, 8, 16384)), dim3(512), 0, stream, sp);
        else
            hipLaunchKernelGGL(topk16_short_kernel<16>, dim3(grid_for(rows, 1, 4096)), dim3(1024), 0, stream, sp);
        LSD_HIP(hipGetLastError());
    } else {
        const Chunks ch = chunks_for(rows, cols);
        LongParams lp{};
        lp.keys = keys;
        lp.cols = (uint32_t)cols;
        lp.chunk = ch.chunk;
        lp.chunks = ch.per_row;
        lp.chunk_cap = (uint32_t)chunk_cap_for(cols);
        lp.state = reinterpret_cast<uint4*>(ws + L.state);
        lp.hist = reinterpret_cast<uint32_t*>(ws + L.hist);
        lp.counts = reinterpret_cast<uint2*>(ws + L.counts);
        lp.map = map;
        lp.out = out;
        if (lp.chunks > lp.chunk_cap) return LSDSORT_ERR_INVALID_ARG;   // never: chunks are at least kMinChunk keys
        const uint32_t grid = (uint32_t)(rows * lp.chunks), row_grid = (uint32_t)rows;
        hipLaunchKernelGGL(topk16_clear_kernel, dim3(grid_for(rows * kBins, 1024, 4096)), dim3(kPlainThreads), 0, stream, ctl, lp.hist,
                           (uint32_t)(rows * kBins), lp.state, (uint32_t)rows, (uint32_t)k);
        hipLaunchKernelGGL(topk16_hist_kernel<0>, dim3(grid), dim3(kLongThreads), 0, stream, lp);
        hipLaunchKernelGGL(topk16_scan_kernel<0>, dim3(row_grid), dim3(256), 0, stream, lp);
        hipLaunchKernelGGL(topk16_hist_kernel<1>, dim3(grid), dim3(kLongThreads), 0, stream, lp);
        hipLaunchKernelGGL(topk16_scan_kernel<1>, dim3(row_grid), dim3(256), 0, stream, lp);
        LSD_HIP(hipGetLastError());
        hipLaunchKernelGGL(topk16_count_kernel, dim3(grid), dim3(kLongThreads), 0, stream, lp);
        hipLaunchKernelGGL(topk16_write_kernel, dim3(grid), dim3(kLongThreads), 0, stream, lp);
        LSD_HIP(hipGetLastError());
    }
    if (k >= 2) {   // one winner per row is in order as it stands
        hipLaunchKernelGGL(topk16_offsets_kernel, dim3(grid_for(rows + 1, 256, 1024)), dim3(kPlainThreads), 0, stream, offsets, (uint32_t)rows,
                           (uint32_t)k);
        LSD_HIP(hipGetLastError());
        LSD_TRY(lsdsort_segmented_device(win, win_pos, offsets, rows, rows * k, LSDSORT_KEY_U32, 0, ws + L.seg, L.seg_bytes, stream));
    }
    hipLaunchKernelGGL(topk16_finish_kernel, dim3(finish_grid), dim3(kPlainThreads), 0, stream, static_cast<const uint32_t*>(win),
                       static_cast<const uint32_t*>(win_pos), (uint32_t)k, map, out_keys, out_idx, (uint32_t)rows, (uint32_t)k);
    LSD_HIP(hipGetLastError());
    if (k >= 2) LSD_HIP(launch_keep_fault(ctl, reinterpret_cast<const uint32_t*>(ws + L.seg), stream));
    return LSDSORT_OK;
}

}  // namespace
}  // namespace lsd

extern "C" {

size_t lsdsort_topk16_workspace_bytes(size_t rows, size_t cols, size_t k)
{
    if (rows > LSDSORT_MAX_KEYS || cols > LSDSORT_MAX_KEYS || k > LSDSORT_MAX_KEYS) return 0;
    if (rows != 0 && cols > LSDSORT_MAX_KEYS / rows) return 0;
    if (rows != 0 && k > LSDSORT_MAX_KEYS / rows) return 0;
    const lsd::Topk16Layout L = lsd::topk16_layout(rows, cols, k, lsd::sort_route_keys(rows, cols, k));
    return L.total > L.s_total ? L.total : L.s_total;
}

int lsdsort_topk16_device(const void* d_keys, size_t rows, size_t cols, size_t k, int key_type, int largest, void* d_out_keys,
                          uint32_t* d_out_idx, void* d_workspace, size_t workspace_bytes, void* hip_stream)
{
    Key16Map map;
    LSD_TRY(key16_map(key_type, largest, &map));
    if (rows > LSDSORT_MAX_KEYS || (rows != 0 && cols > LSDSORT_MAX_KEYS / rows)) return LSDSORT_ERR_TOO_LARGE;
    if (k > cols) return LSDSORT_ERR_INVALID_ARG;
    if (rows == 0 || cols == 0 || k == 0) return LSDSORT_OK;
    if (!d_keys || !d_out_keys || (((uintptr_t)d_keys | (uintptr_t)d_out_keys) & 1)) return LSDSORT_ERR_INVALID_ARG;
    const lsd::Topk16Layout L = lsd::topk16_layout(rows, cols, k, lsd::sort_route_keys(rows, cols, k));
    const size_t need = L.total > L.s_total ? L.total : L.s_total;
    if (!lsd::workspace_ok(d_workspace, workspace_bytes, need)) return LSDSORT_ERR_WORKSPACE;
    int rank_method = 0;
    LSD_TRY(lsd::device_rank_method(8, &rank_method));
    return lsd::run_topk16(static_cast<const uint16_t*>(d_keys), rows, cols, k, map, static_cast<uint16_t*>(d_out_keys), d_out_idx,
                           static_cast<char*>(d_workspace), L, static_cast<hipStream_t>(hip_stream));
}

}  // extern "C"
