// lsd_host.hpp -- what the host side of every translation unit shares: error propagation, workspace alignment, the typed
// entries' key transform, grid sizing, the on/off environment knobs, and the functions one unit defines for another.
// Included by the file that defines each of those functions as well as by its users, so the compiler checks the signatures.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdlib>
#include "../../include/lsdsort.h"
#include "lsd_kernels.hpp"

namespace lsd {
// lsdsort_api.hip
void set_last_hip_error(hipError_t e);                      // what lsdsort_last_hip_error reports (per host thread)
int device_rank_method(int radix_bits, int* rank_method);   // the current device set up (probe included), and the rank form in force there
// the MSB partition with its bucket counts published (and `counts_ready` recorded) BEFORE the partition pass
int partition_with_event(const uint32_t* d_in, uint32_t* d_out, size_t n, int msb_bits, uint64_t* d_counts,
                         void* d_workspace, size_t workspace_bytes, hipStream_t stream, hipEvent_t counts_ready);
// the same by thresholds: bucket of a key = number of thresholds <= key; ascending values in [0, 2^32], 2^32 = above every key
int threshold_partition_with_event(const uint32_t* d_in, uint32_t* d_out, size_t n, int log2_buckets, const uint64_t* thresholds,
                                   uint64_t* d_counts, void* d_workspace, size_t workspace_bytes, hipStream_t stream,
                                   hipEvent_t counts_ready);
// sharded.hip: one host thread per device (or per virtual device: loopback), RCCL between them
int sort_host_multi(uint32_t* keys, size_t n, int radix_bits, int num_gpus, bool loopback);

// A failed HIP call is recorded for lsdsort_last_hip_error, HIP's sticky error is cleared (or the next unrelated HIP call of
// the process would report it again), and the caller returns LSDSORT_ERR_HIP.
#define LSD_HIP(expr)                         \
    do {                                      \
        hipError_t e__ = (expr);              \
        if (e__ != hipSuccess) {              \
            lsd::set_last_hip_error(e__);     \
            (void)hipGetLastError();          \
            return LSDSORT_ERR_HIP;           \
        }                                     \
    } while (0)

#define LSD_TRY(expr)                      \
    do {                                   \
        int s__ = (expr);                  \
        if (s__ != LSDSORT_OK) return s__; \
    } while (0)

constexpr size_t kAlign = 256;   // every workspace, and every array inside one
constexpr size_t kCtlBytes = 256;   // the control block at the front of a workspace whose first word is the entry's fault word
inline size_t align_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }
inline size_t min_sz(size_t a, size_t b) { return a < b ? a : b; }
inline size_t max_sz(size_t a, size_t b) { return a > b ? a : b; }
inline bool workspace_ok(const void* ws, size_t bytes, size_t need) { return ws && !((uintptr_t)ws & (kAlign - 1)) && bytes >= need; }

// key_type (LSDSORT_KEY_*) and direction as the transform the kernels apply (lsd_kernels.hpp, KeyTransform)
inline int key_transform(int key_type, int descending, KeyTransform* xf)
{
    *xf = KeyTransform{};
    switch (key_type) {
        case LSDSORT_KEY_U32: break;
        case LSDSORT_KEY_I32: xf->b = 0x80000000u; break;
        case LSDSORT_KEY_F32: xf->a = 0x80000000u; xf->b = 0x80000000u; break;
        default: return LSDSORT_ERR_INVALID_ARG;
    }
    if (descending) xf->c = 0xFFFFFFFFu;
    xf->on = (xf->a | xf->b | xf->c) != 0u;
    return LSDSORT_OK;
}

// workgroups for `items` at `per_workgroup` each: at least one, at most `cap`
inline uint32_t grid_for(size_t items, size_t per_workgroup, size_t cap)
{
    const size_t g = (items + per_workgroup - 1) / per_workgroup;
    return (uint32_t)(g < 1 ? 1 : (g > cap ? cap : g));
}

// An on/off environment knob: a knob that is on by default goes off with a leading '0', one that is off goes on with a leading '1'.
inline bool env_flag(const char* name, bool on_by_default)
{
    const char* e = getenv(name);
    return !e ? on_by_default : on_by_default ? e[0] != '0' : e[0] == '1';
}
}  // namespace lsd
