// lsdsort.hpp -- C++ face of liblsdsort.so: namespace lsd { sort(...) }.
//
// `lsd::sort(uint32_t* keys, size_t n)` is the host-side entry point BASELINE.json's north_star
// names.  The reference has no such symbol; it is defined as the body of
// TestGPULSDRadixSort between LSDRadixSort/LSDRadixSort.cu:1001 and :1005 (H2D, GPULSDRadixSort,
// D2H).  Header-only wrappers over include/lsdsort.h; a non-zero status becomes an exception (the
// reference crashes instead: MYCRASH, Utils.h:6-15).
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "lsdsort.h"

namespace lsd {

class sort_error : public std::runtime_error {
public:
    sort_error(int status, const char* where)
        : std::runtime_error(std::string(where) + ": " + lsdsort_strerror(status)), status_(status) {}
    int status() const noexcept { return status_; }

private:
    int status_;
};

inline void check(int status, const char* where)
{
    if (status != LSDSORT_OK) throw sort_error(status, where);
}

// Host array, in place, ascending.  Blocking.
inline void sort(uint32_t* keys, size_t n) { check(lsdsort_u32(keys, n), "lsdsort_u32"); }
inline void sort(uint32_t* keys, size_t n, int radix_bits) { check(lsdsort_u32_ex(keys, n, radix_bits, 1), "lsdsort_u32_ex"); }

// Host array over several GPUs of this node (one process; RCCL over xGMI; BASELINE.json configs[3]).
inline void sort(uint32_t* keys, size_t n, int radix_bits, int num_gpus) { check(lsdsort_u32_ex(keys, n, radix_bits, num_gpus), "lsdsort_u32_ex"); }

// Host key/value arrays, stable by key.
inline void sort_pairs(uint32_t* keys, uint32_t* vals, size_t n) { check(lsdsort_pairs_u32(keys, vals, n), "lsdsort_pairs_u32"); }

// Device-resident sort, stream-ordered: the counterpart of GPULSDRadixSort(a, b, h, ...), .cu:839.
inline size_t workspace_bytes(size_t n, int radix_bits = 8, bool pairs = false) { return lsdsort_workspace_bytes(n, radix_bits, pairs ? 1 : 0); }
inline void sort_device(uint32_t* d_keys, void* d_workspace, size_t workspace_bytes_, size_t n, int radix_bits = 8,
                        void* hip_stream = nullptr)
{
    check(lsdsort_u32_device(d_keys, d_workspace, workspace_bytes_, n, radix_bits, hip_stream), "lsdsort_u32_device");
}
inline void sort_pairs_device(uint32_t* d_keys, uint32_t* d_vals, void* d_workspace, size_t workspace_bytes_, size_t n,
                              int radix_bits = 8, void* hip_stream = nullptr)
{
    check(lsdsort_pairs_u32_device(d_keys, d_vals, d_workspace, workspace_bytes_, n, radix_bits, hip_stream),
          "lsdsort_pairs_u32_device");
}

// Other 32-bit key types and orders (no reference counterpart): the overload picks the key type.
inline void sort_device(int32_t* d_keys, void* d_workspace, size_t workspace_bytes_, size_t n, bool descending = false,
                        uint32_t* d_vals = nullptr, int radix_bits = 8, void* hip_stream = nullptr)
{
    check(lsdsort_keys_device(d_keys, d_vals, d_workspace, workspace_bytes_, n, radix_bits, LSDSORT_KEY_I32, descending ? 1 : 0,
                              hip_stream), "lsdsort_keys_device");
}
inline void sort_device(float* d_keys, void* d_workspace, size_t workspace_bytes_, size_t n, bool descending = false,
                        uint32_t* d_vals = nullptr, int radix_bits = 8, void* hip_stream = nullptr)
{
    check(lsdsort_keys_device(d_keys, d_vals, d_workspace, workspace_bytes_, n, radix_bits, LSDSORT_KEY_F32, descending ? 1 : 0,
                              hip_stream), "lsdsort_keys_device");
}
inline void sort_device_descending(uint32_t* d_keys, void* d_workspace, size_t workspace_bytes_, size_t n,
                                   uint32_t* d_vals = nullptr, int radix_bits = 8, void* hip_stream = nullptr)
{
    check(lsdsort_keys_device(d_keys, d_vals, d_workspace, workspace_bytes_, n, radix_bits, LSDSORT_KEY_U32, 1, hip_stream),
          "lsdsort_keys_device");
}

// 64-bit keys (lsdsort_keys64_device): the overload picks the key type; workspace of wide_workspace_bytes(n, radix_bits, val_bits).
// float64 sorts in IEEE total order; descending is stable too.  sort_records_device: the same with a 32- or 64-bit payload per key.
inline size_t wide_workspace_bytes(size_t n, int radix_bits = 8, int val_bits = 0) { return lsdsort_wide_workspace_bytes(n, radix_bits, 64, val_bits); }
inline void sort_device(uint64_t* d_keys, void* d_workspace, size_t workspace_bytes_, size_t n, bool descending = false,
                        int radix_bits = 8, void* hip_stream = nullptr)
{
    check(lsdsort_keys64_device(d_keys, nullptr, 0, d_workspace, workspace_bytes_, n, radix_bits, LSDSORT_KEY_U64, descending ? 1 : 0,
                                hip_stream), "lsdsort_keys64_device");
}
inline void sort_device(int64_t* d_keys, void* d_workspace, size_t workspace_bytes_, size_t n, bool descending = false,
                        int radix_bits = 8, void* hip_stream = nullptr)
{
    check(lsdsort_keys64_device(d_keys, nullptr, 0, d_workspace, workspace_bytes_, n, radix_bits, LSDSORT_KEY_I64, descending ? 1 : 0,
                                hip_stream), "lsdsort_keys64_device");
}
inline void sort_device(double* d_keys, void* d_workspace, size_t workspace_bytes_, size_t n, bool descending = false,
                        int radix_bits = 8, void* hip_stream = nullptr)
{
    check(lsdsort_keys64_device(d_keys, nullptr, 0, d_workspace, workspace_bytes_, n, radix_bits, LSDSORT_KEY_F64, descending ? 1 : 0,
                                hip_stream), "lsdsort_keys64_device");
}
namespace detail {
inline lsdsort_key_type key64_type(const uint64_t*) { return LSDSORT_KEY_U64; }
inline lsdsort_key_type key64_type(const int64_t*) { return LSDSORT_KEY_I64; }
inline lsdsort_key_type key64_type(const double*) { return LSDSORT_KEY_F64; }
}  // namespace detail
// Key = uint64_t, int64_t or double; Val = a 32- or 64-bit type (its bits travel untouched)
template <class Key, class Val>
inline void sort_records_device(Key* d_keys, Val* d_vals, void* d_workspace, size_t workspace_bytes_, size_t n, bool descending = false,
                                int radix_bits = 8, void* hip_stream = nullptr)
{
    static_assert(sizeof(Val) == 4 || sizeof(Val) == 8, "payloads of 32 or 64 bits");
    check(lsdsort_keys64_device(d_keys, d_vals, (int)sizeof(Val) * 8, d_workspace, workspace_bytes_, n, radix_bits,
                                detail::key64_type(d_keys), descending ? 1 : 0, hip_stream), "lsdsort_keys64_device");
}

// 16-bit keys (lsdsort_keys16_device): uint16_t or int16_t by overload; float16 and bfloat16 have no standard C++ type, so their
// bits are passed as uint16_t with the key type named.  Workspace of keys16_workspace_bytes(n, pairs).  Keys only: large sorts
// count the 65536 values instead of moving keys.  With d_vals: stable, descending too.
inline size_t keys16_workspace_bytes(size_t n, bool pairs = false) { return lsdsort_keys16_workspace_bytes(n, pairs ? 1 : 0); }
inline void sort16_device(uint16_t* d_keys, void* d_workspace, size_t workspace_bytes_, size_t n, bool descending = false,
                          uint32_t* d_vals = nullptr, lsdsort_key16_type key_type = LSDSORT_KEY16_U16, void* hip_stream = nullptr)
{
    check(lsdsort_keys16_device(d_keys, d_vals, d_workspace, workspace_bytes_, n, key_type, descending ? 1 : 0, hip_stream),
          "lsdsort_keys16_device");
}
inline void sort16_device(int16_t* d_keys, void* d_workspace, size_t workspace_bytes_, size_t n, bool descending = false,
                          uint32_t* d_vals = nullptr, void* hip_stream = nullptr)
{
    check(lsdsort_keys16_device(d_keys, d_vals, d_workspace, workspace_bytes_, n, LSDSORT_KEY16_I16, descending ? 1 : 0, hip_stream),
          "lsdsort_keys16_device");
}

// Many independent segments of one array, each sorted in place and stable (lsdsort_segmented_device): segment s =
// d_keys[d_offsets[s] .. d_offsets[s + 1]), d_offsets on the device.  Malformed offsets: lsdsort_check_device afterwards.
inline size_t segmented_workspace_bytes(size_t n, size_t num_segments, bool pairs = false)
{
    return lsdsort_segmented_workspace_bytes(n, num_segments, pairs ? 1 : 0);
}
inline void sort_segments(void* d_keys, const uint32_t* d_offsets, size_t num_segments, size_t n, void* d_workspace,
                          size_t workspace_bytes_, lsdsort_key_type key_type = LSDSORT_KEY_U32, bool descending = false,
                          uint32_t* d_vals = nullptr, void* hip_stream = nullptr)
{
    check(lsdsort_segmented_device(d_keys, d_vals, d_offsets, num_segments, n, key_type, descending ? 1 : 0, d_workspace,
                                   workspace_bytes_, hip_stream), "lsdsort_segmented_device");
}

// The k best keys of every row of a row-major [rows x cols] array and their positions in the row, best first, without sorting the
// rows (lsdsort_topk_device): exactly the first k columns of the rows' stable sort.  d_keys is only read; d_out_idx may be null.
inline size_t topk_workspace_bytes(size_t rows, size_t cols, size_t k) { return lsdsort_topk_workspace_bytes(rows, cols, k); }
inline void topk(const void* d_keys, size_t rows, size_t cols, size_t k, void* d_out_keys, uint32_t* d_out_idx, void* d_workspace,
                 size_t workspace_bytes_, lsdsort_key_type key_type = LSDSORT_KEY_U32, bool largest = true, void* hip_stream = nullptr)
{
    check(lsdsort_topk_device(d_keys, rows, cols, k, key_type, largest ? 1 : 0, d_out_keys, d_out_idx, d_workspace, workspace_bytes_,
                              hip_stream), "lsdsort_topk_device");
}

// The same for 16-bit keys (lsdsort_topk16_device): uint16_t or int16_t by overload; float16 and bfloat16 bits are passed as
// uint16_t with the key type named, as in sort16_device.  Workspace of topk16_workspace_bytes(rows, cols, k).
inline size_t topk16_workspace_bytes(size_t rows, size_t cols, size_t k) { return lsdsort_topk16_workspace_bytes(rows, cols, k); }
inline void topk16_device(const uint16_t* d_keys, size_t rows, size_t cols, size_t k, uint16_t* d_out_keys, uint32_t* d_out_idx,
                          void* d_workspace, size_t workspace_bytes_, bool largest = true,
                          lsdsort_key16_type key_type = LSDSORT_KEY16_U16, void* hip_stream = nullptr)
{
    check(lsdsort_topk16_device(d_keys, rows, cols, k, key_type, largest ? 1 : 0, d_out_keys, d_out_idx, d_workspace, workspace_bytes_,
                                hip_stream), "lsdsort_topk16_device");
}
inline void topk16_device(const int16_t* d_keys, size_t rows, size_t cols, size_t k, int16_t* d_out_keys, uint32_t* d_out_idx,
                          void* d_workspace, size_t workspace_bytes_, bool largest = true, void* hip_stream = nullptr)
{
    check(lsdsort_topk16_device(d_keys, rows, cols, k, LSDSORT_KEY16_I16, largest ? 1 : 0, d_out_keys, d_out_idx, d_workspace,
                                workspace_bytes_, hip_stream), "lsdsort_topk16_device");
}

// The key at 0-based `rank` of every row's stable sort and its position in the row, without sorting the rows or writing any winner
// (lsdsort_kth_device): column `rank` of topk(.., k = rank + 1, ..).  uint32_t, int32_t or float by overload; d_keys is only read;
// d_out_idx may be null.  Workspace of kth_workspace_bytes(rows, cols).
inline size_t kth_workspace_bytes(size_t rows, size_t cols) { return lsdsort_kth_workspace_bytes(rows, cols); }
inline void kth_device(const uint32_t* d_keys, size_t rows, size_t cols, size_t rank, uint32_t* d_out_keys, uint32_t* d_out_idx,
                       void* d_workspace, size_t workspace_bytes_, bool largest = false, void* hip_stream = nullptr)
{
    check(lsdsort_kth_device(d_keys, rows, cols, rank, LSDSORT_KEY_U32, largest ? 1 : 0, d_out_keys, d_out_idx, d_workspace,
                             workspace_bytes_, hip_stream), "lsdsort_kth_device");
}
inline void kth_device(const int32_t* d_keys, size_t rows, size_t cols, size_t rank, int32_t* d_out_keys, uint32_t* d_out_idx,
                       void* d_workspace, size_t workspace_bytes_, bool largest = false, void* hip_stream = nullptr)
{
    check(lsdsort_kth_device(d_keys, rows, cols, rank, LSDSORT_KEY_I32, largest ? 1 : 0, d_out_keys, d_out_idx, d_workspace,
                             workspace_bytes_, hip_stream), "lsdsort_kth_device");
}
inline void kth_device(const float* d_keys, size_t rows, size_t cols, size_t rank, float* d_out_keys, uint32_t* d_out_idx,
                       void* d_workspace, size_t workspace_bytes_, bool largest = false, void* hip_stream = nullptr)
{
    check(lsdsort_kth_device(d_keys, rows, cols, rank, LSDSORT_KEY_F32, largest ? 1 : 0, d_out_keys, d_out_idx, d_workspace,
                             workspace_bytes_, hip_stream), "lsdsort_kth_device");
}

// The same for 16-bit keys (lsdsort_kth16_device): column `rank` of topk16(.., k = rank + 1, ..).  uint16_t or int16_t by overload;
// float16 and bfloat16 bits are passed as uint16_t with the key type named, as in topk16_device.  d_keys is only read; d_out_idx may
// be null (long rows then need no locate).  Workspace of kth16_workspace_bytes(rows, cols).
inline size_t kth16_workspace_bytes(size_t rows, size_t cols) { return lsdsort_kth16_workspace_bytes(rows, cols); }
inline void kth16_device(const uint16_t* d_keys, size_t rows, size_t cols, size_t rank, uint16_t* d_out_keys, uint32_t* d_out_idx,
                         void* d_workspace, size_t workspace_bytes_, bool largest = false,
                         lsdsort_key16_type key_type = LSDSORT_KEY16_U16, void* hip_stream = nullptr)
{
    check(lsdsort_kth16_device(d_keys, rows, cols, rank, key_type, largest ? 1 : 0, d_out_keys, d_out_idx, d_workspace, workspace_bytes_,
                               hip_stream), "lsdsort_kth16_device");
}
inline void kth16_device(const int16_t* d_keys, size_t rows, size_t cols, size_t rank, int16_t* d_out_keys, uint32_t* d_out_idx,
                         void* d_workspace, size_t workspace_bytes_, bool largest = false, void* hip_stream = nullptr)
{
    check(lsdsort_kth16_device(d_keys, rows, cols, rank, LSDSORT_KEY16_I16, largest ? 1 : 0, d_out_keys, d_out_idx, d_workspace,
                               workspace_bytes_, hip_stream), "lsdsort_kth16_device");
}

// The stable sort of every row of a row-major [rows x cols] array of 16-bit keys with each key's position in its row
// (lsdsort_rows16_device): uint16_t or int16_t by overload; float16 and bfloat16 bits are passed as uint16_t with the key type named.
// d_out_keys may be d_keys (in place); d_out_idx may be null.  Workspace of rows16_workspace_bytes(rows, cols).
inline size_t rows16_workspace_bytes(size_t rows, size_t cols) { return lsdsort_rows16_workspace_bytes(rows, cols); }
inline void sort_rows16_device(const uint16_t* d_keys, size_t rows, size_t cols, uint16_t* d_out_keys, uint32_t* d_out_idx, void* d_workspace,
                               size_t workspace_bytes_, bool descending = false, lsdsort_key16_type key_type = LSDSORT_KEY16_U16,
                               void* hip_stream = nullptr)
{
    check(lsdsort_rows16_device(d_keys, rows, cols, key_type, descending ? 1 : 0, d_out_keys, d_out_idx, d_workspace, workspace_bytes_,
                                hip_stream), "lsdsort_rows16_device");
}
inline void sort_rows16_device(const int16_t* d_keys, size_t rows, size_t cols, int16_t* d_out_keys, uint32_t* d_out_idx, void* d_workspace,
                               size_t workspace_bytes_, bool descending = false, void* hip_stream = nullptr)
{
    check(lsdsort_rows16_device(d_keys, rows, cols, LSDSORT_KEY16_I16, descending ? 1 : 0, d_out_keys, d_out_idx, d_workspace,
                                workspace_bytes_, hip_stream), "lsdsort_rows16_device");
}

// A shard of a range-partitioned array: keys expected to share their top `common_prefix_bits` bits (a hint; the device checks)
inline void sort_shard_device(uint32_t* d_keys, void* d_workspace, size_t workspace_bytes_, size_t n, int common_prefix_bits,
                              int radix_bits = 8, void* hip_stream = nullptr)
{
    check(lsdsort_u32_device_prefixed(d_keys, d_workspace, workspace_bytes_, n, radix_bits, common_prefix_bits, hip_stream),
          "lsdsort_u32_device_prefixed");
}
// Did the last sort queued in this workspace run the hybrid form (lsdsort_set_hybrid)?  Synchronises the stream.
inline bool ran_hybrid_form(const void* d_workspace, void* hip_stream = nullptr)
{
    int hybrid = 0;
    check(lsdsort_workspace_form(d_workspace, hip_stream, &hybrid), "lsdsort_workspace_form");
    return hybrid != 0;
}

// One rank of a multi-GPU sort (one process per GPU): RAII over lsdsort_comm_*.  Rank 0 calls unique_id() and ships
// the 128 bytes to the other ranks over the launcher's own channel (MPI_Bcast, a file, torch.distributed).
struct comm_id {
    unsigned char bytes[LSDSORT_COMM_ID_BYTES];
};
inline comm_id unique_id()
{
    comm_id id;
    check(lsdsort_comm_unique_id(id.bytes), "lsdsort_comm_unique_id");
    return id;
}
class communicator {
public:
    communicator(const comm_id& id, int world, int rank) { check(lsdsort_comm_create(id.bytes, world, rank, &c_), "lsdsort_comm_create"); }
    // `world` VIRTUAL ranks on the current device (lsdsort_comm_create_loopback): element r is rank r's communicator; each is to
    // be driven by its own host thread.  For one-GPU machines: the step then runs with world > 1 (tests/cpp/test_sharded.cpp).
    static std::vector<std::unique_ptr<communicator>> loopback(int world)
    {
        std::vector<lsdsort_comm*> raw((size_t)(world > 0 ? world : 1), nullptr);
        check(lsdsort_comm_create_loopback(world, raw.data()), "lsdsort_comm_create_loopback");
        std::vector<std::unique_ptr<communicator>> out;
        for (lsdsort_comm* c : raw) out.emplace_back(new communicator(c));
        return out;
    }
    ~communicator() { lsdsort_comm_destroy(c_); }
    communicator(const communicator&) = delete;
    communicator& operator=(const communicator&) = delete;
    int world() const { return lsdsort_comm_world(c_); }
    int rank() const { return lsdsort_comm_rank(c_); }
    size_t workspace_bytes(size_t n_local_max, size_t out_capacity, int radix_bits = 8) const
    {
        return lsdsort_sharded_workspace_bytes(n_local_max, out_capacity, world(), radix_bits);
    }
    struct slice {
        size_t n;                 // keys of d_out that are this rank's part of the result
        uint64_t global_offset;   // index of the first of them in the global order
    };
    // Collective.  d_keys_in is left untouched; the exchange and the local sort stay queued on hip_stream.
    // partition: LSDSORT_PARTITION_MSB (top key bits; uniform keys) or LSDSORT_PARTITION_SPLITTERS (sampled; any keys).
    slice sort_device(const uint32_t* d_keys_in, size_t n_local, uint32_t* d_out, size_t out_capacity, void* d_workspace,
                      size_t workspace_bytes_, int radix_bits = 8, void* hip_stream = nullptr, uint64_t* counts_matrix = nullptr,
                      int partition = LSDSORT_PARTITION_MSB)
    {
        slice s{0, 0};
        check(lsdsort_sharded_u32_device_ex(c_, d_keys_in, n_local, d_out, out_capacity, &s.n, &s.global_offset, counts_matrix,
                                            d_workspace, workspace_bytes_, radix_bits, partition, hip_stream),
              "lsdsort_sharded_u32_device_ex");
        return s;
    }

private:
    explicit communicator(lsdsort_comm* adopted) : c_(adopted) {}
    lsdsort_comm* c_ = nullptr;
};

}  // namespace lsd
