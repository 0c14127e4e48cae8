// phase_stats.hpp -- in-kernel phase stamps of the rank-and-scatter kernel.
//
// Diagnostic build only (make stats -> liblsdsort_stats.so, never the product): wave 0 of every
// tile stamps s_memrealtime (100 MHz) at phase boundaries and adds the differences to
// a per-tile record p.stats[tile][0..6]; [7] look-back refills, [8] empty polls (thread 0's digit).
// tools/phase_stats.py reads the records.  In the product the context is empty and every macro expands to
// nothing (its arguments are not evaluated).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace lsd {

constexpr int kStatsStride = 16;   // [0..6] phases, [7] refills, [8] empty polls, [9] start, [10] rows walked,
                                   // [11] t(prefix stored), [12] t(prefix met), [13] chain pos it was met at, [14] t(walk start), [15] t(first step consumed)

#ifdef LSD_PHASE_STATS
// What a stamp needs to know, handed to every phase that stamps or counts.
struct PhaseStats {
    unsigned long long* table;   // PassParams::stats (null: nothing is recorded)
    unsigned long long stamp;    // time of the previous stamp
    uint32_t row;                // status row of the tile being stamped
    bool lead;                   // thread 0 writes the stamps
};
#define LSD_STATS_BEGIN(st, p, tid) lsd::PhaseStats st = {(p).stats, __builtin_amdgcn_s_memrealtime(), 0u, (tid) == 0}
#define LSD_SET(st, idx, v)                                                                             \
    do {                                                                                                \
        if ((st).table) (st).table[(size_t)(st).row * lsd::kStatsStride + (idx)] = (unsigned long long)(v); \
    } while (0)
#define LSD_STAMP(st, idx)                                                                              \
    do {                                                                                                \
        const unsigned long long now__ = __builtin_amdgcn_s_memrealtime();                              \
        if ((st).lead && (st).table) (st).table[(size_t)(st).row * lsd::kStatsStride + (idx)] = now__ - (st).stamp; \
        (st).stamp = now__;                                                                             \
    } while (0)
#define LSD_COUNT(st, idx, v)                                                                           \
    do {                                                                                                \
        if ((st).table) (st).table[(size_t)(st).row * lsd::kStatsStride + (idx)] += (unsigned long long)(v); \
    } while (0)
// The tile is known: its row, the kernel's start time, and the per-pass counters back to zero (the rows are reused by every
// pass of a sort); then the first stamp, the ticket.
#define LSD_STATS_TILE(st, tile)                                                                        \
    do {                                                                                                \
        (st).row = (tile);                                                                              \
        if ((st).lead) {                                                                                \
            LSD_SET(st, 9, (st).stamp);                                                                 \
            LSD_SET(st, 7, 0);                                                                          \
            LSD_SET(st, 8, 0);                                                                          \
            LSD_SET(st, 10, 0);                                                                         \
        }                                                                                               \
        LSD_STAMP(st, 0);                                                                               \
    } while (0)
// a stamp that first waits for the wave's outstanding global loads and stores
#define LSD_STAMP_DRAINED(st, idx)                                                                      \
    do {                                                                                                \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                \
        LSD_STAMP(st, idx);                                                                             \
    } while (0)
#else
struct PhaseStats { };
#define LSD_STATS_BEGIN(st, p, tid) [[maybe_unused]] lsd::PhaseStats st
#define LSD_STAMP(st, idx) do { } while (0)
#define LSD_COUNT(st, idx, v) do { } while (0)
#define LSD_SET(st, idx, v) do { } while (0)
#define LSD_STATS_TILE(st, tile) do { } while (0)
#define LSD_STAMP_DRAINED(st, idx) do { } while (0)
#endif

}  // namespace lsd
