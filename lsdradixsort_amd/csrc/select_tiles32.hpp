// select_tiles32.hpp -- the tile helpers of the 32-bit k-th value units, once: what kth.hip and kth_multi.hip do with one wave's
// tile of a Row<uint32_t>.  The 32-bit sibling of select_tiles16.hpp, and as there a unit calls these
// helpers DIRECTLY from its kernels.  topk.hip's load_tile has another shape (a plain pointer, one key per load, no validity mask)
// and stays in that unit.
//
// Key reads.  A row starts 4 r cols bytes past the keys, at any multiple of 4 within a 16-byte line.  Every kernel therefore splits
// EACH ROW by address (Row): `head` keys in front of the row's first 16-byte line (0..3), read one by one, and the `body` from that
// line on, read as 16-byte groups of four keys; the last group of a row (or chunk) that is not whole is read one by one too.  A
// lane holds four groups of its wave's tile: register 4 j + e is body position q0 + 4 (64 j + lane) + e.
// A key that does not exist.  Every 32-bit pattern is a real key, so no padding value can stand for "no key" (the 16-bit select's
// 0xFFFFFFFF does not carry over).  Instead every tile comes with a per-lane VALIDITY MASK (bit i: register i holds a key of the
// row; bit 16: the head register does), made from the positions alone where the tile is loaded, and every count and every match
// is the AND of that bit with the comparison: a register without a key matches no (prefix, shift) whatever it holds.
#pragma once

#include "lsd_device.hpp"
#include "radix_select.hpp"

namespace lsd {
namespace {

constexpr uint32_t kGroup = 4;                // keys of one 16-byte load
constexpr uint32_t kHeadBit = 1u << kRegs;    // validity mask: the head register
using Row32 = Row<uint32_t>;   // a lane holds four 16-byte groups of four keys of its wave's tile

// The wave's tile from body position q0 (a multiple of four) on, valid below `end`: a whole group by one 16-byte load, the others
// key by key.  Returns the validity mask of the sixteen registers; a register without a key holds zero and its bit is clear.
__device__ __forceinline__ uint32_t load_tile(const Row32& r, uint32_t q0, uint32_t end, uint32_t lane, const KeyTransform& xf,
                                              uint32_t (&t)[kRegs])
{
    uint32_t vm = 0u;
#pragma unroll
    for (int j = 0; j < kRegs / 4; j++) {
        const uint32_t q = q0 + ((uint32_t)j * 64u + lane) * kGroup;
        if (q < end && end - q >= kGroup) {
            const uint4 v = *reinterpret_cast<const uint4*>(r.keys + r.head + q);
            t[4 * j] = to_sortable(v.x, xf);
            t[4 * j + 1] = to_sortable(v.y, xf);
            t[4 * j + 2] = to_sortable(v.z, xf);
            t[4 * j + 3] = to_sortable(v.w, xf);
            vm |= 0xFu << (4 * j);
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                t[4 * j + e] = 0u;
                if (q < end && q + (uint32_t)e < end) {
                    t[4 * j + e] = to_sortable(r.keys[r.head + q + (uint32_t)e], xf);
                    vm |= 1u << (4 * j + e);
                }
            }
        }
    }
    return vm;
}
// head key `lane` of the row, for the one wave that owns the head: its validity bit, and the key into h
__device__ __forceinline__ uint32_t load_head(const Row32& r, uint32_t lane, const KeyTransform& xf, uint32_t& h)
{
    h = 0u;
    if (lane >= r.head) return 0u;
    h = to_sortable(r.keys[lane], xf);
    return kHeadBit;
}

// Locate within one tile held in registers (load_tile at q0, validity mask vm; with kHeadBit in vm of some lanes: the head keys h
// in front of it).  `base`: the keys under the prefix before this tile in the row; it moves on past the tile.  If the `need`-th
// (1-based) such key of the row lies in this tile, the lane that holds it stores it, un-mapped, and its position at o.at(row, slot)
// of o.keys and o.idx (may be null): `row` in kth.hip, row * slots + slot in kth_multi.hip.  Returns whether it did (uniform over
// the group).  s_wc: WAVES words.  The store stays a lambda inside `if (here)` with the index computed in it (select_tiles16.hpp).
template <int WAVES, class Out>
__device__ __forceinline__ bool locate_tile(const uint32_t (&t)[kRegs], uint32_t h, uint32_t vm, uint32_t q0, const Row32& r, uint32_t prefix,
                                            uint32_t shift, uint32_t need, uint32_t& base, volatile lds_u32* s_wc, uint32_t wave,
                                            uint32_t lane, uint32_t row, uint32_t slot, const Out& o, const KeyTransform& xf)
{
    uint32_t em = ((vm & kHeadBit) != 0u && (h >> shift) == prefix) ? kHeadBit : 0u;   // the keys under the prefix
#pragma unroll
    for (int i = 0; i < kRegs; i++) em |= (((vm >> i) & 1u) != 0u && (t[i] >> shift) == prefix) ? 1u << i : 0u;
    const uint32_t mine = wave_sum((uint32_t)__builtin_popcount(em));
    uint32_t before = base, all = mine;
    if (WAVES > 1) {
        if (lane == 0u) s_wc[wave] = mine;
        __syncthreads();
        all = 0u;
        for (uint32_t w = 0; w < (uint32_t)WAVES; w++) {
            const uint32_t c = s_wc[w];
            if (w < wave) before += c;
            all += c;
        }
        __syncthreads();   // the next tile writes s_wc again
    }
    const bool here = base < need && need - base <= all;   // uniform
    if (here) {
        auto store = [&](uint32_t key, uint32_t pos) {
            if (row < o.rows) {
                const size_t at = o.at(row, slot);
                o.keys[at] = from_sortable(key, xf);
                if (o.idx) o.idx[at] = pos;
            }
        };
        // position order: the head keys by lane, then group j of lane 0, 1, .. 63, j = 0 .. 3
        const uint32_t ch = em >> kRegs;
        const uint32_t hi = wave_inclusive_scan(ch);
        if (ch != 0u && before + hi == need) store(h, lane);
        before += (uint32_t)__builtin_amdgcn_readlane((int)hi, 63);
#pragma unroll
        for (int j = 0; j < kRegs / 4; j++) {
            const uint32_t g = (em >> (4 * j)) & 0xFu, c = (uint32_t)__builtin_popcount(g);
            const uint32_t incl = wave_inclusive_scan(c), lo = before + incl - c;
            if (lo < need && need - lo <= c) {
                uint32_t left = need - lo;   // 1 .. c: which of this group's matching keys
                const uint32_t pos = r.head + q0 + ((uint32_t)j * 64u + lane) * kGroup;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    if (((g >> e) & 1u) != 0u && --left == 0u) store(t[4 * j + e], pos + (uint32_t)e);
                }
            }
            before += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        }
    }
    base += all;
    return here;
}

}  // namespace
}  // namespace lsd
