// The device face of include/lsdsort.hpp: every lsd:: wrapper that test_lsd_sort.cpp and test_sharded.cpp do not reach, called
// once with every argument observable and compared bit for bit with a reference made here from the standard library alone.
//
// A wrapper's body has one job -- each argument into the right slot of a C entry with ten positional parameters, many of one type
// (rows, cols, k; key_type, largest; n, radix_bits), in an order that deliberately differs from the C++ one.  A transposition
// compiles clean.  So in at least one call of each wrapper every parameter has a value that differs from its default and from
// every other parameter of its type in that call, and the expected output depends on it: rows, cols, k and rank pairwise
// different; both orders; keys with the top bit set, so that the unsigned, signed and float orders of the same bits differ.
// Parameters that cannot change a result are checked through the error they cause: radix_bits = 7 must throw INVALID_ARG, a
// workspace one byte short must throw WORKSPACE and leave every output word as it was.
//
// References: std::stable_sort on (sortable key, position).  The sortable value t of key k is the project's documented map
// (lsdsort.h): unsigned t = k; signed t = k ^ top bit; float (16, 32, 64 bits alike: sign-magnitude) t = ~k where the sign bit is
// set, k ^ top bit otherwise -- IEEE total order; descending t = ~t afterwards, which is stable as well.  top-k = the first k
// columns of each row's stable sort, k-th = column `rank`, with positions.  float16 and bfloat16 share one map and cannot be told
// apart by output: each is named in one call at least.
//
// LIMIT: hip_stream is a created, non-default stream in every call, and that is the only check on it.  A wrapper that dropped
// the stream would still produce right results most of the time; nothing here asserts an ordering that could only be racy.
//
// Shapes are the smallest at which the plumbing shows (a few thousand keys; the kernels' tiers are the GPU suite's business).
// The row entries get one shape of the one-wavefront class and one above the one-workgroup capacity (16384 keys) with three
// rows, so that a rows / cols swap also changes the size class.  The one large input is the hybrid-form call of
// sort_shard_device (the smallest size and radix at which the form is taken).
//
//   test_device_face              needs a gfx950 device
//   test_device_face --no-device  any machine: the *_workspace_bytes wrappers against the C functions, and the argument checks the
//                                 C entries make before they look for a device.  Every call of this mode fails such a check (or
//                                 has n = 0): none can reach a device, whether there is one or not.
//
// On a mismatch: the wrapper, the call's arguments, the first differing index, both values; exit 1 at once, nothing further is
// launched.  Every HIP call is checked the same way.  Built with hipcc (host code only) and run by tests/test_cpp_device_face.py.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <numeric>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "lsdsort.hpp"

namespace {

[[noreturn]] void fail(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    std::fprintf(stderr, "FAILED: ");
    std::vfprintf(stderr, fmt, ap);
    std::fprintf(stderr, "\n");
    va_end(ap);
    std::fflush(nullptr);
    std::_Exit(1);   // at once: no destructor launches or frees anything
}

std::string text(const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return buf;
}

#define HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) fail("%s (line %d): %s", #x, __LINE__, hipGetErrorString(e_)); } while (0)

void* g_stream = nullptr;   // the created stream every call is given

void drain() { HIP(hipStreamSynchronize(static_cast<hipStream_t>(g_stream))); }

template <class T>
struct Dev {
    T* p = nullptr;
    size_t n = 0;
    explicit Dev(size_t count) : n(count) { HIP(hipMalloc(reinterpret_cast<void**>(&p), (count ? count : 1) * sizeof(T))); }
    explicit Dev(const std::vector<T>& h) : Dev(h.size()) { up(h); }
    Dev(const Dev&) = delete;
    Dev& operator=(const Dev&) = delete;
    ~Dev() { (void)hipFree(p); }
    void up(const std::vector<T>& h) { HIP(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice)); }
    std::vector<T> down() const
    {
        std::vector<T> h(n);
        HIP(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
        return h;
    }
};

// ---- the references ------------------------------------------------------------------------------------------------------

enum Order { kUnsigned, kSigned, kFloat };
const char* order_name(Order o) { return o == kUnsigned ? "unsigned" : o == kSigned ? "signed" : "float"; }
Order order_of(lsdsort_key_type t) { return t == LSDSORT_KEY_U32 ? kUnsigned : t == LSDSORT_KEY_I32 ? kSigned : kFloat; }
Order order_of(lsdsort_key16_type t) { return t == LSDSORT_KEY16_U16 ? kUnsigned : t == LSDSORT_KEY16_I16 ? kSigned : kFloat; }

template <class U>
U sortable(U k, Order o, bool descending)
{
    const U top = (U)((U)1 << (sizeof(U) * 8 - 1));
    const U t = o == kUnsigned ? k : o == kSigned ? (U)(k ^ top) : (k & top) ? (U)~k : (U)(k ^ top);
    return descending ? (U)~t : t;
}

// positions of keys[0 .. n) in their stable sort
template <class U>
std::vector<uint32_t> stable_order(const U* keys, size_t n, Order o, bool descending)
{
    std::vector<U> t(n);
    for (size_t i = 0; i < n; i++) t[i] = sortable(keys[i], o, descending);
    std::vector<uint32_t> idx(n);
    std::iota(idx.begin(), idx.end(), 0u);
    std::stable_sort(idx.begin(), idx.end(), [&t](uint32_t a, uint32_t b) { return t[a] < t[b]; });
    return idx;
}

// Keys whose three orders differ and whose duplicates make stability visible: a quarter from a pool of special and repeated
// values (both zeros, all ones = -NaN / -1, the largest positive pattern = +NaN / max, random ones), the rest random bits.
template <class U>
std::vector<U> make_keys(size_t n, uint64_t seed)
{
    std::mt19937_64 gen(seed * 0x9E3779B97F4A7C15ull + 12345);
    const U top = (U)((U)1 << (sizeof(U) * 8 - 1));
    std::vector<U> pool = {(U)0, top, (U)~(U)0, (U)(top - 1), (U)(top | 1), (U)1};
    for (int i = 0; i < 26; i++) pool.push_back((U)gen());
    std::vector<U> keys(n);
    for (auto& k : keys) k = (gen() & 3) == 0 ? pool[gen() % pool.size()] : (U)gen();
    return keys;
}

template <class V>
std::vector<V> make_payloads(size_t n, uint64_t seed)
{
    std::vector<V> v(n);   // distinct, every bit in use, not the positions
    for (size_t i = 0; i < n; i++) v[i] = (V)(((uint64_t)(i + 1 + seed) * 0x9E3779B97F4A7C15ull) >> (64 - sizeof(V) * 8));
    return v;
}

template <class U>
void expect_equal(const std::string& call, const char* what, const std::vector<U>& got, const std::vector<U>& want)
{
    if (got.size() != want.size()) fail("%s: %s: %zu words, expected %zu", call.c_str(), what, got.size(), want.size());
    for (size_t i = 0; i < want.size(); i++)
        if (got[i] != want[i])
            fail("%s: %s differ at %zu: got 0x%llx, expected 0x%llx", call.c_str(), what, i, (unsigned long long)got[i],
                 (unsigned long long)want[i]);
}

template <class F>
void expect_status(const std::string& call, int want, F&& f)
{
    int got = LSDSORT_OK;
    std::string msg;
    try {
        f();
    } catch (const lsd::sort_error& e) {
        got = e.status();
        msg = e.what();
    }
    if (got != want)
        fail("%s: status %d (%s)%s%s, expected %d (%s)", call.c_str(), got, lsdsort_strerror(got), msg.empty() ? "" : " from ", msg.c_str(), want,
             lsdsort_strerror(want));
}

struct Group {
    const char* name;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    explicit Group(const char* n) : name(n) {}
    ~Group()
    {
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::printf("  %-22s %8.1f ms\n", name, ms);
        std::fflush(stdout);
    }
};

void same_figure(const char* wrapper, size_t got, size_t c_figure, std::initializer_list<size_t> swapped);

template <class U> constexpr U sentinel() { return (U)0xA5C3A5C3A5C3A5C3ull; }

// ---- whole-array sorts -----------------------------------------------------------------------------------------------------
// One sort wrapper, one call: `skew` elements in front of the keys (an off-line base address) and `tail` behind them are not part
// of the sort and must come back unchanged -- `n` is observable.  radix = 0: the wrapper takes no radix.
template <class U, class V>
void sort_case(const std::string& call, Order o, bool descending, bool with_vals, size_t n, size_t skew, size_t wb, int radix,
               const std::function<void(U* d_keys, V* d_vals, void* d_ws, size_t wsb, int radix_bits)>& run)
{
    static uint64_t seed = 100;
    const size_t tail = 37;
    const std::string what = text("%s [%s %s n=%zu skew=%zu radix_bits=%d vals=%d workspace=%zu]", call.c_str(), order_name(o),
                                  descending ? "descending" : "ascending", n, skew, radix, (int)with_vals, wb);
    const std::vector<U> all = make_keys<U>(skew + n + tail, ++seed);
    const std::vector<V> vals = make_payloads<V>(n + tail, seed);
    if (wb == 0) fail("%s: a workspace figure of 0", what.c_str());
    Dev<U> dk(all);
    Dev<V> dv(vals);
    Dev<unsigned char> ws(wb);
    V* pv = with_vals ? dv.p : nullptr;
    if (radix) {
        expect_status(what + " with radix_bits = 7", LSDSORT_ERR_INVALID_ARG, [&] { run(dk.p + skew, pv, ws.p, wb, 7); });
        drain();
    }
    expect_status(what + " with a workspace one byte short", LSDSORT_ERR_WORKSPACE, [&] { run(dk.p + skew, pv, ws.p, wb - 1, radix); });
    drain();
    expect_equal(what, "keys after a refused call", dk.down(), all);
    expect_equal(what, "payloads after a refused call", dv.down(), vals);

    expect_status(what, LSDSORT_OK, [&] { run(dk.p + skew, pv, ws.p, wb, radix); });
    drain();
    const std::vector<uint32_t> ord = stable_order(all.data() + skew, n, o, descending);
    std::vector<U> want = all;
    std::vector<V> want_vals = vals;
    for (size_t i = 0; i < n; i++) {
        want[skew + i] = all[skew + ord[i]];
        if (with_vals) want_vals[i] = vals[ord[i]];
    }
    expect_equal(what, "keys (with the words around them)", dk.down(), want);
    expect_equal(what, with_vals ? "payloads (stable argsort)" : "the payload buffer that was not passed", dv.down(), want_vals);
}

void group_sorts32()
{
    Group g("32-bit sorts");
    const size_t n = 3001;
    const int r = 4;
    using Run = std::function<void(uint32_t*, uint32_t*, void*, size_t, int)>;
    const size_t wb = lsd::workspace_bytes(n, r), wbp = lsd::workspace_bytes(n, r, true);
    sort_case<uint32_t, uint32_t>("sort_device(uint32_t*)", kUnsigned, false, false, n, 0, wb, r,
                                  Run([&](uint32_t* k, uint32_t*, void* ws, size_t b, int rb) { lsd::sort_device(k, ws, b, n, rb, g_stream); }));
    sort_case<uint32_t, uint32_t>("sort_pairs_device", kUnsigned, false, true, n, 0, wbp, r,
                                  Run([&](uint32_t* k, uint32_t* v, void* ws, size_t b, int rb) { lsd::sort_pairs_device(k, v, ws, b, n, rb, g_stream); }));
    for (int desc = 0; desc < 2; desc++) {   // payloads with one order, none with the other
        const bool d = desc != 0;
        sort_case<uint32_t, uint32_t>("sort_device(int32_t*)", kSigned, d, d, n, 0, d ? wbp : wb, r,
                                      Run([&](uint32_t* k, uint32_t* v, void* ws, size_t b, int rb) {
                                          lsd::sort_device(reinterpret_cast<int32_t*>(k), ws, b, n, d, v, rb, g_stream);
                                      }));
        sort_case<uint32_t, uint32_t>("sort_device(float*)", kFloat, d, !d, n, 0, !d ? wbp : wb, r,
                                      Run([&](uint32_t* k, uint32_t* v, void* ws, size_t b, int rb) {
                                          lsd::sort_device(reinterpret_cast<float*>(k), ws, b, n, d, v, rb, g_stream);
                                      }));
        sort_case<uint32_t, uint32_t>("sort_device_descending", kUnsigned, true, d, n, 0, d ? wbp : wb, r,
                                      Run([&](uint32_t* k, uint32_t* v, void* ws, size_t b, int rb) {
                                          lsd::sort_device_descending(k, ws, b, n, v, rb, g_stream);
                                      }));
    }
}

template <class Key>
void sorts64_of(const char* name, Order o)
{
    const size_t n = 2999;
    const int r = 4;
    const size_t wb = lsd::wide_workspace_bytes(n, r);
    using Run = std::function<void(uint64_t*, uint32_t*, void*, size_t, int)>;
    for (int desc = 0; desc < 2; desc++)
        sort_case<uint64_t, uint32_t>(name, o, desc != 0, false, n, 0, wb, r, Run([&](uint64_t* k, uint32_t*, void* ws, size_t b, int rb) {
                                          lsd::sort_device(reinterpret_cast<Key*>(k), ws, b, n, desc != 0, rb, g_stream);
                                      }));
}

void group_sorts64()
{
    Group g("64-bit sorts");
    sorts64_of<uint64_t>("sort_device(uint64_t*)", kUnsigned);
    sorts64_of<int64_t>("sort_device(int64_t*)", kSigned);
    sorts64_of<double>("sort_device(double*)", kFloat);
}

// Val: the wrapper's payload type; VBits: the unsigned type of its width (the bits travel untouched)
template <class Key, class Val, class VBits>
void records_of(const char* name, Order o, bool descending)
{
    static_assert(sizeof(Val) == sizeof(VBits), "payload bits");
    const size_t n = 3003;
    const int r = 4;
    const size_t wb = lsd::wide_workspace_bytes(n, r, (int)sizeof(Val) * 8);
    sort_case<uint64_t, VBits>(name, o, descending, true, n, 0, wb, r,
                               std::function<void(uint64_t*, VBits*, void*, size_t, int)>([&](uint64_t* k, VBits* v, void* ws, size_t b, int rb) {
                                   lsd::sort_records_device(reinterpret_cast<Key*>(k), reinterpret_cast<Val*>(v), ws, b, n, descending, rb, g_stream);
                               }));
}

void group_records()
{
    Group g("64-bit records");
    records_of<uint64_t, float, uint32_t>("sort_records_device<uint64_t, float>", kUnsigned, true);
    records_of<uint64_t, uint64_t, uint64_t>("sort_records_device<uint64_t, uint64_t>", kUnsigned, false);
    records_of<int64_t, uint32_t, uint32_t>("sort_records_device<int64_t, uint32_t>", kSigned, false);
    records_of<int64_t, double, uint64_t>("sort_records_device<int64_t, double>", kSigned, true);
    records_of<double, int32_t, uint32_t>("sort_records_device<double, int32_t>", kFloat, true);
    records_of<double, int64_t, uint64_t>("sort_records_device<double, int64_t>", kFloat, false);
}

void group_sort16()
{
    Group g("16-bit sorts");
    const size_t n = 3005;
    using Run = std::function<void(uint16_t*, uint32_t*, void*, size_t, int)>;
    struct Case { lsdsort_key16_type type; bool descending, vals; size_t skew; };
    // float16 and bfloat16 share one sortable map: no output tells them apart, each is named once
    const Case cases[] = {{LSDSORT_KEY16_F16, true, true, 1}, {LSDSORT_KEY16_BF16, false, false, 0}, {LSDSORT_KEY16_I16, false, true, 0},
                          {LSDSORT_KEY16_U16, true, false, 0}};
    for (const Case& c : cases)
        sort_case<uint16_t, uint32_t>(text("sort16_device(uint16_t*, key_type=%d)", (int)c.type), order_of(c.type), c.descending, c.vals, n, c.skew,
                                      lsd::keys16_workspace_bytes(n, c.vals), 0, Run([&](uint16_t* k, uint32_t* v, void* ws, size_t b, int) {
                                          lsd::sort16_device(k, ws, b, n, c.descending, v, c.type, g_stream);
                                      }));
    for (int desc = 0; desc < 2; desc++)
        sort_case<uint16_t, uint32_t>("sort16_device(int16_t*)", kSigned, desc != 0, desc != 0, n, (size_t)desc, lsd::keys16_workspace_bytes(n, desc != 0), 0,
                                      Run([&](uint16_t* k, uint32_t* v, void* ws, size_t b, int) {
                                          lsd::sort16_device(reinterpret_cast<int16_t*>(k), ws, b, n, desc != 0, v, g_stream);
                                      }));
}

void group_segments()
{
    Group g("segmented sort");
    const size_t n = 4001;
    const std::vector<uint32_t> off = {13, 200, 200, 1500, 1501, 3000, 3500, 3987};   // an empty segment, one of one key; 13 and 14 words outside
    const size_t segs = off.size() - 1;
    Dev<uint32_t> doff(off);
    struct Case { lsdsort_key_type type; bool descending, vals; };
    const Case cases[] = {{LSDSORT_KEY_I32, true, true}, {LSDSORT_KEY_F32, false, false}, {LSDSORT_KEY_U32, true, true}, {LSDSORT_KEY_F32, true, true}};
    uint64_t seed = 300;
    for (const Case& c : cases) {
        const size_t wb = lsd::segmented_workspace_bytes(n, segs, c.vals);
        const std::string what = text("sort_segments [key_type=%d %s num_segments=%zu n=%zu vals=%d workspace=%zu]", (int)c.type,
                                      c.descending ? "descending" : "ascending", segs, n, (int)c.vals, wb);
        const std::vector<uint32_t> keys = make_keys<uint32_t>(n, ++seed), vals = make_payloads<uint32_t>(n, seed);
        Dev<uint32_t> dk(keys), dv(vals);
        Dev<unsigned char> ws(wb);
        uint32_t* pv = c.vals ? dv.p : nullptr;
        expect_status(what + " with a workspace one byte short", LSDSORT_ERR_WORKSPACE,
                      [&] { lsd::sort_segments(dk.p, doff.p, segs, n, ws.p, wb - 1, c.type, c.descending, pv, g_stream); });
        drain();
        expect_equal(what, "keys after a refused call", dk.down(), keys);
        expect_status(what, LSDSORT_OK, [&] { lsd::sort_segments(dk.p, doff.p, segs, n, ws.p, wb, c.type, c.descending, pv, g_stream); });
        drain();
        std::vector<uint32_t> want = keys, want_vals = vals;
        for (size_t s = 0; s < segs; s++) {
            const size_t b = off[s], len = off[s + 1] - off[s];
            const std::vector<uint32_t> ord = stable_order(keys.data() + b, len, order_of(c.type), c.descending);
            for (size_t i = 0; i < len; i++) {
                want[b + i] = keys[b + ord[i]];
                if (c.vals) want_vals[b + i] = vals[b + ord[i]];
            }
        }
        expect_equal(what, "keys (segments sorted, the words outside them unchanged)", dk.down(), want);
        expect_equal(what, c.vals ? "payloads (stable argsort per segment)" : "the payload buffer that was not passed", dv.down(), want_vals);
    }
}

// ---- the row entries -------------------------------------------------------------------------------------------------------
// Columns [from, from + take) of every row's stable sort and their positions: top-k (0, k), k-th (rank, 1), the row sort (0, cols).
// The outputs are pre-filled with a sentinel and carry 19 more words than the result, which must stay; `skew` puts the input and the
// key output one element off their line.  in_place: the key output is the input (the row sort only).
template <class U>
void rows_case(const std::string& call, Order o, bool descending, size_t rows, size_t cols, size_t from, size_t take, bool with_idx, bool in_place,
               size_t skew, size_t wb, const std::function<void(const U* d_keys, U* d_out, uint32_t* d_idx, void* d_ws, size_t wsb)>& run)
{
    static uint64_t seed = 500;
    const size_t pad = 19, out_n = rows * take;
    const std::string what = text("%s [%s %s rows=%zu cols=%zu from=%zu take=%zu idx=%d in_place=%d skew=%zu workspace=%zu]", call.c_str(),
                                  order_name(o), descending ? "descending" : "ascending", rows, cols, from, take, (int)with_idx, (int)in_place, skew, wb);
    if (wb == 0) fail("%s: a workspace figure of 0", what.c_str());
    const std::vector<U> keys = make_keys<U>(skew + rows * cols + pad, ++seed);
    const std::vector<U> blank_keys(skew + out_n + pad, sentinel<U>());
    const std::vector<uint32_t> blank_idx(out_n + pad, sentinel<uint32_t>());
    Dev<U> dk(keys), dout(blank_keys);
    Dev<uint32_t> didx(blank_idx);
    Dev<unsigned char> ws(wb);
    U* out = in_place ? dk.p + skew : dout.p + skew;
    uint32_t* idx = with_idx ? didx.p : nullptr;
    expect_status(what + " with a workspace one byte short", LSDSORT_ERR_WORKSPACE, [&] { run(dk.p + skew, out, idx, ws.p, wb - 1); });
    drain();
    expect_equal(what, "the input after a refused call", dk.down(), keys);
    expect_equal(what, "the key output after a refused call", dout.down(), blank_keys);
    expect_equal(what, "the positions after a refused call", didx.down(), blank_idx);

    expect_status(what, LSDSORT_OK, [&] { run(dk.p + skew, out, idx, ws.p, wb); });
    drain();
    std::vector<U> want_keys = in_place ? keys : blank_keys;
    std::vector<uint32_t> want_idx = blank_idx;
    for (size_t r = 0; r < rows; r++) {
        const U* row = keys.data() + skew + r * cols;
        const std::vector<uint32_t> ord = stable_order(row, cols, o, descending);
        for (size_t j = 0; j < take; j++) {
            want_keys[skew + r * take + j] = row[ord[from + j]];
            if (with_idx) want_idx[r * take + j] = ord[from + j];
        }
    }
    expect_equal(what, "keys (with the words around them)", (in_place ? dk : dout).down(), want_keys);
    expect_equal(what, with_idx ? "positions" : "the position buffer that was not passed", didx.down(), want_idx);
    if (!in_place) expect_equal(what, "the input, which is only read", dk.down(), keys);
}

// one shape of the one-wavefront class, one above the one-workgroup capacity: rows, cols, k and rank pairwise different
struct Shape { size_t rows, cols, k, rank; };
const Shape kShapes[2] = {{5, 333, 17, 41}, {3, 17001, 29, 123}};

void group_topk()
{
    Group g("top-k");
    using Run = std::function<void(const uint32_t*, uint32_t*, uint32_t*, void*, size_t)>;
    struct Case { lsdsort_key_type type; bool largest, idx; int shape; };
    const Case cases[] = {{LSDSORT_KEY_I32, false, true, 0}, {LSDSORT_KEY_F32, true, true, 1}, {LSDSORT_KEY_U32, false, false, 1}, {LSDSORT_KEY_F32, false, true, 0}};
    for (const Case& c : cases) {
        const Shape s = kShapes[c.shape];
        rows_case<uint32_t>(text("topk(key_type=%d, largest=%d, k=%zu)", (int)c.type, (int)c.largest, s.k), order_of(c.type), c.largest, s.rows, s.cols, 0, s.k,
                            c.idx, false, 0, lsd::topk_workspace_bytes(s.rows, s.cols, s.k),
                            Run([&](const uint32_t* k, uint32_t* out, uint32_t* idx, void* ws, size_t b) {
                                lsd::topk(k, s.rows, s.cols, s.k, out, idx, ws, b, c.type, c.largest, g_stream);
                            }));
    }
}

void group_topk16()
{
    Group g("top-k, 16-bit");
    using Run = std::function<void(const uint16_t*, uint16_t*, uint32_t*, void*, size_t)>;
    struct Case { lsdsort_key16_type type; bool largest, idx; int shape; size_t skew; };
    // bfloat16 and float16: one map, each named once
    const Case cases[] = {{LSDSORT_KEY16_BF16, false, true, 0, 1}, {LSDSORT_KEY16_F16, true, true, 1, 0}, {LSDSORT_KEY16_U16, false, false, 1, 0},
                          {LSDSORT_KEY16_I16, true, true, 0, 0}};
    for (const Case& c : cases) {
        const Shape s = kShapes[c.shape];
        rows_case<uint16_t>(text("topk16_device(uint16_t*, largest=%d, key_type=%d, k=%zu)", (int)c.largest, (int)c.type, s.k), order_of(c.type), c.largest,
                            s.rows, s.cols, 0, s.k, c.idx, false, c.skew, lsd::topk16_workspace_bytes(s.rows, s.cols, s.k),
                            Run([&](const uint16_t* k, uint16_t* out, uint32_t* idx, void* ws, size_t b) {
                                lsd::topk16_device(k, s.rows, s.cols, s.k, out, idx, ws, b, c.largest, c.type, g_stream);
                            }));
    }
    for (int i = 0; i < 2; i++) {
        const Shape s = kShapes[i];
        const bool largest = i == 0;
        rows_case<uint16_t>(text("topk16_device(int16_t*, largest=%d, k=%zu)", (int)largest, s.k), kSigned, largest, s.rows, s.cols, 0, s.k, true, false,
                            (size_t)i, lsd::topk16_workspace_bytes(s.rows, s.cols, s.k),
                            Run([&](const uint16_t* k, uint16_t* out, uint32_t* idx, void* ws, size_t b) {
                                lsd::topk16_device(reinterpret_cast<const int16_t*>(k), s.rows, s.cols, s.k, reinterpret_cast<int16_t*>(out), idx, ws, b,
                                                   largest, g_stream);
                            }));
    }
}

template <class Key>
void kth_of(const char* name, Order o)
{
    using Run = std::function<void(const uint32_t*, uint32_t*, uint32_t*, void*, size_t)>;
    for (int i = 0; i < 2; i++) {
        const Shape s = kShapes[i];
        const bool largest = (i == 0) == (o != kSigned);   // each order at each shape, over the three overloads
        rows_case<uint32_t>(text("%s rank=%zu largest=%d", name, s.rank, (int)largest), o, largest, s.rows, s.cols, s.rank, 1, !(i == 1 && o == kFloat), false,
                            0, lsd::kth_workspace_bytes(s.rows, s.cols), Run([&](const uint32_t* k, uint32_t* out, uint32_t* idx, void* ws, size_t b) {
                                lsd::kth_device(reinterpret_cast<const Key*>(k), s.rows, s.cols, s.rank, reinterpret_cast<Key*>(out), idx, ws, b, largest,
                                                g_stream);
                            }));
    }
}

void group_kth()
{
    Group g("k-th value");
    kth_of<uint32_t>("kth_device(uint32_t*)", kUnsigned);
    kth_of<int32_t>("kth_device(int32_t*)", kSigned);
    kth_of<float>("kth_device(float*)", kFloat);
}

void group_kth16()
{
    Group g("k-th value, 16-bit");
    using Run = std::function<void(const uint16_t*, uint16_t*, uint32_t*, void*, size_t)>;
    struct Case { lsdsort_key16_type type; bool largest, idx; int shape; size_t skew; };
    const Case cases[] = {{LSDSORT_KEY16_F16, true, true, 0, 1}, {LSDSORT_KEY16_BF16, false, true, 1, 0}, {LSDSORT_KEY16_I16, true, false, 1, 0},
                          {LSDSORT_KEY16_U16, true, true, 1, 1}};
    for (const Case& c : cases) {
        const Shape s = kShapes[c.shape];
        rows_case<uint16_t>(text("kth16_device(uint16_t*, rank=%zu, largest=%d, key_type=%d)", s.rank, (int)c.largest, (int)c.type), order_of(c.type),
                            c.largest, s.rows, s.cols, s.rank, 1, c.idx, false, c.skew, lsd::kth16_workspace_bytes(s.rows, s.cols),
                            Run([&](const uint16_t* k, uint16_t* out, uint32_t* idx, void* ws, size_t b) {
                                lsd::kth16_device(k, s.rows, s.cols, s.rank, out, idx, ws, b, c.largest, c.type, g_stream);
                            }));
    }
    for (int i = 0; i < 2; i++) {
        const Shape s = kShapes[i];
        const bool largest = i == 1;
        rows_case<uint16_t>(text("kth16_device(int16_t*, rank=%zu, largest=%d)", s.rank, (int)largest), kSigned, largest, s.rows, s.cols, s.rank, 1, true, false,
                            (size_t)(1 - i), lsd::kth16_workspace_bytes(s.rows, s.cols),
                            Run([&](const uint16_t* k, uint16_t* out, uint32_t* idx, void* ws, size_t b) {
                                lsd::kth16_device(reinterpret_cast<const int16_t*>(k), s.rows, s.cols, s.rank, reinterpret_cast<int16_t*>(out), idx, ws, b,
                                                  largest, g_stream);
                            }));
    }
}

void group_rows16()
{
    Group g("row sort, 16-bit");
    using Run = std::function<void(const uint16_t*, uint16_t*, uint32_t*, void*, size_t)>;
    struct Case { lsdsort_key16_type type; bool descending, idx, in_place; int shape; size_t skew; };
    const Case cases[] = {{LSDSORT_KEY16_BF16, true, true, false, 0, 1},    // into a second buffer, off the line
                          {LSDSORT_KEY16_F16, false, true, true, 1, 0},     // in place
                          {LSDSORT_KEY16_U16, true, false, false, 0, 0},    // no positions
                          {LSDSORT_KEY16_I16, false, true, false, 1, 1}};
    for (const Case& c : cases) {
        const Shape s = kShapes[c.shape];
        rows_case<uint16_t>(text("sort_rows16_device(uint16_t*, descending=%d, key_type=%d)", (int)c.descending, (int)c.type), order_of(c.type), c.descending,
                            s.rows, s.cols, 0, s.cols, c.idx, c.in_place, c.skew, lsd::rows16_workspace_bytes(s.rows, s.cols),
                            Run([&](const uint16_t* k, uint16_t* out, uint32_t* idx, void* ws, size_t b) {
                                lsd::sort_rows16_device(k, s.rows, s.cols, out, idx, ws, b, c.descending, c.type, g_stream);
                            }));
    }
    for (int i = 0; i < 2; i++) {
        const Shape s = kShapes[i];
        const bool descending = i == 1;
        rows_case<uint16_t>(text("sort_rows16_device(int16_t*, descending=%d)", (int)descending), kSigned, descending, s.rows, s.cols, 0, s.cols, true, i == 0,
                            (size_t)i, lsd::rows16_workspace_bytes(s.rows, s.cols), Run([&](const uint16_t* k, uint16_t* out, uint32_t* idx, void* ws, size_t b) {
                                lsd::sort_rows16_device(reinterpret_cast<const int16_t*>(k), s.rows, s.cols, reinterpret_cast<int16_t*>(out), idx, ws, b,
                                                        descending, g_stream);
                            }));
    }
}

// ---- a shard, and which form sorted it --------------------------------------------------------------------------------------
void shard_case(size_t n, int radix, int prefix, bool hybrid)
{
    const std::string what = text("sort_shard_device [n=%zu common_prefix_bits=%d radix_bits=%d]", n, prefix, radix);
    std::mt19937 gen((uint32_t)n);
    std::vector<uint32_t> keys(n + 5);   // five words behind the shard stay
    const uint32_t top = (0xA5u >> (8 - prefix)) << (32 - prefix);   // a prefix value with its top bit set
    for (auto& k : keys) k = ((uint32_t)gen() >> prefix) | top;
    const size_t wb = lsd::workspace_bytes(n, radix);
    Dev<uint32_t> dk(keys);
    Dev<unsigned char> ws(wb);
    expect_status(what + " with radix_bits = 7", LSDSORT_ERR_INVALID_ARG, [&] { lsd::sort_shard_device(dk.p, ws.p, wb, n, prefix, 7, g_stream); });
    expect_status(what + " with common_prefix_bits = 9", LSDSORT_ERR_INVALID_ARG, [&] { lsd::sort_shard_device(dk.p, ws.p, wb, n, 9, radix, g_stream); });
    // workspace_bytes(n, ..) is the need of a sort of n keys only in the smallest size class; above it the figure also covers the
    // smaller classes' tile shapes and one byte less is still enough for this n -- the short workspace is the small call's check
    if (!hybrid) expect_status(what + " with a workspace one byte short", LSDSORT_ERR_WORKSPACE, [&] { lsd::sort_shard_device(dk.p, ws.p, wb - 1, n, prefix, radix, g_stream); });
    drain();
    expect_equal(what, "keys after a refused call", dk.down(), keys);
    expect_status(what, LSDSORT_OK, [&] { lsd::sort_shard_device(dk.p, ws.p, wb, n, prefix, radix, g_stream); });
    bool form = !hybrid;
    expect_status("ran_hybrid_form after " + what, LSDSORT_OK, [&] { form = lsd::ran_hybrid_form(ws.p, g_stream); });
    if (form != hybrid) fail("ran_hybrid_form after %s: %d, expected %d", what.c_str(), (int)form, (int)hybrid);
    std::vector<uint32_t> want = keys;
    std::sort(want.begin(), want.begin() + (ptrdiff_t)n);
    expect_equal(what, "keys against std::sort (with the words behind them)", dk.down(), want);
}

void group_shard()
{
    {
        Group g("shard, small");
        shard_case(5000, 4, 3, false);
    }
    Group g("shard, hybrid form");
    shard_case(((size_t)1 << 24) + 99, 4, 3, true);   // the smallest size and radix at which the hybrid form is taken
}

// ---- two virtual ranks -------------------------------------------------------------------------------------------------------
// Everything a rank needs is allocated before its thread starts, so that a thread can only fail inside the collective call, where
// the library releases the peer (LSDSORT_ERR_COMM) instead of leaving it waiting.
struct Rank {
    std::vector<uint32_t> keys;
    size_t cap = 0, wb = 0;
    Dev<uint32_t>*in = nullptr, *out = nullptr;
    Dev<unsigned char>* ws = nullptr;
    hipStream_t stream = nullptr;
    uint64_t matrix[4] = {~0ull, ~0ull, ~0ull, ~0ull};
    lsd::communicator::slice slice{0, 0};
    int status = LSDSORT_OK, hip = 0;
};

void run_world(std::vector<std::unique_ptr<lsd::communicator>>& comms, Rank* ranks, int device, int radix, int partition, const size_t* wsb)
{
    std::vector<std::thread> threads;
    for (int r = 0; r < 2; r++)
        threads.emplace_back([&, r] {
            Rank& k = ranks[r];
            if (hipSetDevice(device) != hipSuccess) { k.hip = 1; k.status = LSDSORT_ERR_HIP; return; }
            try {
                k.slice = comms[(size_t)r]->sort_device(k.in->p, k.keys.size(), k.out->p, k.cap, k.ws->p, wsb[r], radix, k.stream, k.matrix, partition);
            } catch (const lsd::sort_error& e) {
                k.status = e.status();
            }
            if (hipStreamSynchronize(k.stream) != hipSuccess) k.hip = 1;
        });
    for (auto& t : threads) t.join();
    for (int r = 0; r < 2; r++)
        if (ranks[r].hip) fail("communicator::sort_device, rank %d: a HIP call failed: %s", r, hipGetErrorString(hipGetLastError()));
}

void group_loopback()
{
    Group g("loopback(2)");
    int device = 0;
    HIP(hipGetDevice(&device));
    const int radix = 4;
    const size_t n_local[2] = {3001, 4100}, caps[2] = {7200, 7300};
    std::mt19937 gen(77);
    Rank ranks[2];
    std::vector<uint32_t> all;
    for (int r = 0; r < 2; r++) {
        Rank& k = ranks[r];
        k.keys.resize(n_local[r]);
        for (auto& x : k.keys) x = (uint32_t)gen();
        all.insert(all.end(), k.keys.begin(), k.keys.end());
        k.cap = caps[r];
        k.in = new Dev<uint32_t>(k.keys);
        k.out = new Dev<uint32_t>(std::vector<uint32_t>(k.cap, sentinel<uint32_t>()));
        HIP(hipStreamCreateWithFlags(&k.stream, hipStreamNonBlocking));
    }
    std::sort(all.begin(), all.end());

    expect_status("communicator::loopback(3)", LSDSORT_ERR_INVALID_ARG, [] { (void)lsd::communicator::loopback(3); });
    std::vector<std::unique_ptr<lsd::communicator>> comms;
    expect_status("communicator::loopback(2)", LSDSORT_OK, [&] { comms = lsd::communicator::loopback(2); });
    if (comms.size() != 2) fail("communicator::loopback(2): %zu communicators", comms.size());
    size_t wsb[2];
    for (int r = 0; r < 2; r++) {
        if (comms[(size_t)r]->world() != 2 || comms[(size_t)r]->rank() != r)
            fail("communicator::loopback(2): element %d says world %d rank %d", r, comms[(size_t)r]->world(), comms[(size_t)r]->rank());
        Rank& k = ranks[r];
        k.wb = wsb[r] = comms[(size_t)r]->workspace_bytes(n_local[r], k.cap, radix);
        const size_t c_figure = lsdsort_sharded_workspace_bytes(n_local[r], k.cap, 2, radix);
        if (k.wb == 0 || k.wb != c_figure)
            fail("communicator::workspace_bytes(%zu, %zu, %d): %zu, the C function says %zu", n_local[r], k.cap, radix, k.wb, c_figure);
        k.ws = new Dev<unsigned char>(k.wb);
    }
    // at the shards' own sizes the figure is the same with n_local_max and out_capacity swapped; at these it is not
    same_figure("communicator::workspace_bytes(100003, 300001, 4)", comms[0]->workspace_bytes(100003, 300001, 4), lsdsort_sharded_workspace_bytes(100003, 300001, 2, 4),
                {lsdsort_sharded_workspace_bytes(300001, 100003, 2, 4), lsdsort_sharded_workspace_bytes(100003, 300001, 4, 2),
                 lsdsort_sharded_workspace_bytes(100003, 300001, 2, 8)});
    for (int partition : {LSDSORT_PARTITION_MSB, LSDSORT_PARTITION_SPLITTERS}) {
        const std::string what = text("communicator::sort_device [loopback(2) n_local=%zu,%zu out_capacity=%zu,%zu radix_bits=%d partition=%d]", n_local[0],
                                      n_local[1], caps[0], caps[1], radix, partition);
        for (Rank& k : ranks) {
            k.status = LSDSORT_OK;
            std::fill(k.matrix, k.matrix + 4, ~0ull);
        }
        run_world(comms, ranks, device, radix, partition, wsb);
        std::vector<uint32_t> joined;
        uint64_t offset = 0;
        for (int r = 0; r < 2; r++) {
            const Rank& k = ranks[r];
            if (k.status != LSDSORT_OK) fail("%s: rank %d: status %d (%s)", what.c_str(), r, k.status, lsdsort_strerror(k.status));
            if (k.slice.global_offset != offset || k.slice.n > k.cap)
                fail("%s: rank %d: slice of %zu at %llu, expected at %llu", what.c_str(), r, k.slice.n, (unsigned long long)k.slice.global_offset,
                     (unsigned long long)offset);
            const std::vector<uint32_t> got = k.out->down();
            joined.insert(joined.end(), got.begin(), got.begin() + (ptrdiff_t)k.slice.n);
            offset += k.slice.n;
            expect_equal(what, "the input shard, which is left untouched", k.in->down(), k.keys);
            for (int i = 0; i < 4; i++)
                if (k.matrix[i] != ranks[0].matrix[i]) fail("%s: counts_matrix[%d] is %llu on rank %d and %llu on rank 0", what.c_str(), i,
                                                            (unsigned long long)k.matrix[i], r, (unsigned long long)ranks[0].matrix[i]);
        }
        expect_equal(what, "the slices in global_offset order against std::sort of the union", joined, all);
        const uint64_t* m = ranks[0].matrix;   // [src][dst]
        for (int r = 0; r < 2; r++) {
            if (m[r * 2] + m[r * 2 + 1] != n_local[r])
                fail("%s: counts_matrix row %d sums to %llu, rank %d sent %zu", what.c_str(), r, (unsigned long long)(m[r * 2] + m[r * 2 + 1]), r, n_local[r]);
            if (m[r] + m[2 + r] != ranks[r].slice.n)
                fail("%s: counts_matrix column %d sums to %llu, rank %d received %zu", what.c_str(), r, (unsigned long long)(m[r] + m[2 + r]), r, ranks[r].slice.n);
        }
        if (partition == LSDSORT_PARTITION_MSB && !(joined[ranks[0].slice.n - 1] < 0x80000000u && joined[ranks[0].slice.n] >= 0x80000000u))
            fail("%s: rank 0 does not own exactly the keys below 2^31", what.c_str());
    }
    // the errors: a world of its own each, since a rank that fails alone aborts its world for good
    for (int which = 0; which < 2; which++) {
        std::vector<std::unique_ptr<lsd::communicator>> world;
        expect_status("communicator::loopback(2)", LSDSORT_OK, [&] { world = lsd::communicator::loopback(2); });
        for (Rank& k : ranks) {
            k.status = LSDSORT_OK;
            k.out->up(std::vector<uint32_t>(k.cap, sentinel<uint32_t>()));
        }
        const size_t short_ws[2] = {wsb[0] - 1, wsb[1]};
        run_world(world, ranks, device, which == 0 ? 7 : radix, LSDSORT_PARTITION_MSB, which == 0 ? wsb : short_ws);
        const int want0 = which == 0 ? LSDSORT_ERR_INVALID_ARG : LSDSORT_ERR_WORKSPACE, want1 = which == 0 ? LSDSORT_ERR_INVALID_ARG : LSDSORT_ERR_COMM;
        if (ranks[0].status != want0 || ranks[1].status != want1)
            fail("communicator::sort_device with %s: statuses %d and %d, expected %d and %d", which == 0 ? "radix_bits = 7" : "rank 0's workspace one byte short",
                 ranks[0].status, ranks[1].status, want0, want1);
        expect_equal(std::string("communicator::sort_device, refused"), "rank 0's output", ranks[0].out->down(), std::vector<uint32_t>(ranks[0].cap, sentinel<uint32_t>()));
    }
    for (Rank& k : ranks) {
        HIP(hipStreamDestroy(k.stream));
        delete k.in;
        delete k.out;
        delete k.ws;
    }
}

// ---- --no-device -------------------------------------------------------------------------------------------------------------
void same_figure(const char* wrapper, size_t got, size_t c_figure, std::initializer_list<size_t> swapped)
{
    if (got == 0 || got != c_figure) fail("%s: %zu, the C function says %zu", wrapper, got, c_figure);
    for (size_t s : swapped)
        if (s == got) fail("%s: these arguments do not tell a swap apart (the C function gives %zu either way): choose others", wrapper, got);
}

void workspace_figures()
{
    const size_t n = 100003, segs = 37, rows = 7, cols = 40000, k = 33;
    same_figure("workspace_bytes(n, 4, true)", lsd::workspace_bytes(n, 4, true), lsdsort_workspace_bytes(n, 4, 1),
                {lsdsort_workspace_bytes(n, 1, 4), lsdsort_workspace_bytes(4, (int)n, 1), lsdsort_workspace_bytes(n, 4, 0), lsdsort_workspace_bytes(n, 8, 1)});
    same_figure("workspace_bytes(n)", lsd::workspace_bytes(n), lsdsort_workspace_bytes(n, 8, 0), {});
    same_figure("wide_workspace_bytes(n, 4, 32)", lsd::wide_workspace_bytes(n, 4, 32), lsdsort_wide_workspace_bytes(n, 4, 64, 32),
                {lsdsort_wide_workspace_bytes(n, 32, 64, 4), lsdsort_wide_workspace_bytes(n, 64, 4, 32),   // (the wrapper's constant 64 and 32 swapped: the same three words)
                 lsdsort_wide_workspace_bytes(n, 4, 64, 0), lsdsort_wide_workspace_bytes(n, 4, 64, 64), lsdsort_wide_workspace_bytes(n, 8, 64, 32)});
    same_figure("wide_workspace_bytes(n)", lsd::wide_workspace_bytes(n), lsdsort_wide_workspace_bytes(n, 8, 64, 0), {});
    same_figure("keys16_workspace_bytes(n, true)", lsd::keys16_workspace_bytes(n, true), lsdsort_keys16_workspace_bytes(n, 1),
                {lsdsort_keys16_workspace_bytes(1, (int)n), lsdsort_keys16_workspace_bytes(n, 0)});
    same_figure("keys16_workspace_bytes(n)", lsd::keys16_workspace_bytes(n), lsdsort_keys16_workspace_bytes(n, 0), {});
    same_figure("segmented_workspace_bytes(n, num_segments, true)", lsd::segmented_workspace_bytes(n, segs, true), lsdsort_segmented_workspace_bytes(n, segs, 1),
                {lsdsort_segmented_workspace_bytes(segs, n, 1), lsdsort_segmented_workspace_bytes(n, segs, 0), lsdsort_segmented_workspace_bytes(n, 1, (int)segs),
                 lsdsort_segmented_workspace_bytes(1, segs, (int)n)});
    same_figure("segmented_workspace_bytes(n, num_segments)", lsd::segmented_workspace_bytes(n, segs), lsdsort_segmented_workspace_bytes(n, segs, 0), {});
    same_figure("topk_workspace_bytes(rows, cols, k)", lsd::topk_workspace_bytes(rows, cols, k), lsdsort_topk_workspace_bytes(rows, cols, k),
                {lsdsort_topk_workspace_bytes(cols, rows, k), lsdsort_topk_workspace_bytes(rows, k, cols), lsdsort_topk_workspace_bytes(k, cols, rows)});
    same_figure("topk16_workspace_bytes(rows, cols, k)", lsd::topk16_workspace_bytes(rows, cols, k), lsdsort_topk16_workspace_bytes(rows, cols, k),
                {lsdsort_topk16_workspace_bytes(cols, rows, k), lsdsort_topk16_workspace_bytes(rows, k, cols), lsdsort_topk16_workspace_bytes(k, cols, rows)});
    same_figure("kth_workspace_bytes(rows, cols)", lsd::kth_workspace_bytes(rows, cols), lsdsort_kth_workspace_bytes(rows, cols),
                {lsdsort_kth_workspace_bytes(cols, rows)});
    same_figure("kth16_workspace_bytes(rows, cols)", lsd::kth16_workspace_bytes(rows, cols), lsdsort_kth16_workspace_bytes(rows, cols),
                {lsdsort_kth16_workspace_bytes(cols, rows)});
    same_figure("rows16_workspace_bytes(rows, cols)", lsd::rows16_workspace_bytes(rows, cols), lsdsort_rows16_workspace_bytes(rows, cols),
                {lsdsort_rows16_workspace_bytes(cols, rows)});
}

// The checks each C entry makes before it looks for a device (read off the entries: the 32-bit sorts check only radix_bits that
// early; every other entry checks all its arguments and its workspace first).  Pointers are made up and never followed: each call
// fails a check, or has n = 0.  An "invalid" call gets no workspace at all, so that a wrapper which made it valid by swapping two
// arguments is stopped by the workspace check, with another status; a call with a workspace one byte short has no other fault.
void argument_checks()
{
    const int kInvalid = LSDSORT_ERR_INVALID_ARG, kWorkspace = LSDSORT_ERR_WORKSPACE;
    char* const base = reinterpret_cast<char*>((uintptr_t)1 << 20);   // 256-byte aligned, never followed
    void* const ws = base;
    uint32_t* const a32 = reinterpret_cast<uint32_t*>(base + 4096);
    uint32_t* const b32 = reinterpret_cast<uint32_t*>(base + 8192);
    uint32_t* const c32 = reinterpret_cast<uint32_t*>(base + 12288);
    uint16_t* const a16 = reinterpret_cast<uint16_t*>(a32);
    uint16_t* const b16 = reinterpret_cast<uint16_t*>(b32);
    uint16_t* const odd16 = reinterpret_cast<uint16_t*>(base + 8193);
    uint64_t* const a64 = reinterpret_cast<uint64_t*>(a32);
    void* const s = nullptr;
    const size_t n = 1000;

    // radix_bits, with n = 0 (a valid radix then returns LSDSORT_OK before anything else is looked at)
    expect_status("sort_device(uint32_t*, n=0, radix_bits=7)", kInvalid, [&] { lsd::sort_device(a32, ws, 0, 0, 7, s); });
    expect_status("sort_device(uint32_t*, n=0, radix_bits=2)", LSDSORT_OK, [&] { lsd::sort_device(a32, ws, 0, 0, 2, s); });
    expect_status("sort_pairs_device(n=0, radix_bits=7)", kInvalid, [&] { lsd::sort_pairs_device(a32, b32, ws, 0, 0, 7, s); });
    expect_status("sort_device(int32_t*, n=0, descending, radix_bits=7)", kInvalid, [&] { lsd::sort_device(reinterpret_cast<int32_t*>(a32), ws, 0, 0, true, b32, 7, s); });
    expect_status("sort_device(float*, n=0, descending, radix_bits=7)", kInvalid, [&] { lsd::sort_device(reinterpret_cast<float*>(a32), ws, 0, 0, true, b32, 7, s); });
    expect_status("sort_device_descending(n=0, radix_bits=7)", kInvalid, [&] { lsd::sort_device_descending(a32, ws, 0, 0, b32, 7, s); });
    expect_status("sort_device(uint64_t*, n=0, descending, radix_bits=7)", kInvalid, [&] { lsd::sort_device(a64, ws, 0, 0, true, 7, s); });
    expect_status("sort_device(int64_t*, n=0, descending, radix_bits=7)", kInvalid, [&] { lsd::sort_device(reinterpret_cast<int64_t*>(a64), ws, 0, 0, true, 7, s); });
    expect_status("sort_device(double*, n=0, descending, radix_bits=7)", kInvalid, [&] { lsd::sort_device(reinterpret_cast<double*>(a64), ws, 0, 0, true, 7, s); });
    expect_status("sort_device(int64_t*, n=0, ascending, radix_bits=2)", LSDSORT_OK, [&] { lsd::sort_device(reinterpret_cast<int64_t*>(a64), ws, 0, 0, false, 2, s); });
    expect_status("sort_records_device<uint64_t, float>(n=0, descending, radix_bits=7)", kInvalid,
                  [&] { lsd::sort_records_device(a64, reinterpret_cast<float*>(b32), ws, 0, 0, true, 7, s); });
    expect_status("sort_shard_device(n=0, common_prefix_bits=2, radix_bits=7)", kInvalid, [&] { lsd::sort_shard_device(a32, ws, 0, 0, 2, 7, s); });
    expect_status("sort_shard_device(n=0, common_prefix_bits=9, radix_bits=8)", kInvalid, [&] { lsd::sort_shard_device(a32, ws, 0, 0, 9, 8, s); });
    expect_status("sort_shard_device(n=0, common_prefix_bits=8, radix_bits=2)", LSDSORT_OK, [&] { lsd::sort_shard_device(a32, ws, 0, 0, 8, 2, s); });

    // 64-bit keys and records: a null array, then the workspace
    expect_status("sort_device(uint64_t*, null keys)", kInvalid, [&] { lsd::sort_device(static_cast<uint64_t*>(nullptr), nullptr, 0, n, true, 4, s); });
    expect_status("sort_device(uint64_t*, workspace one byte short)", kWorkspace, [&] { lsd::sort_device(a64, ws, lsd::wide_workspace_bytes(n, 4) - 1, n, true, 4, s); });
    expect_status("sort_device(int64_t*, workspace one byte short)", kWorkspace,
                  [&] { lsd::sort_device(reinterpret_cast<int64_t*>(a64), ws, lsd::wide_workspace_bytes(n, 4) - 1, n, true, 4, s); });
    expect_status("sort_device(double*, workspace one byte short)", kWorkspace,
                  [&] { lsd::sort_device(reinterpret_cast<double*>(a64), ws, lsd::wide_workspace_bytes(n, 4) - 1, n, true, 4, s); });
    expect_status("sort_records_device<int64_t, uint32_t>(null payloads)", kInvalid,
                  [&] { lsd::sort_records_device(reinterpret_cast<int64_t*>(a64), static_cast<uint32_t*>(nullptr), nullptr, 0, n, true, 4, s); });
    expect_status("sort_records_device<int64_t, uint32_t>(workspace one byte short)", kWorkspace,
                  [&] { lsd::sort_records_device(reinterpret_cast<int64_t*>(a64), b32, ws, lsd::wide_workspace_bytes(n, 4, 32) - 1, n, true, 4, s); });
    expect_status("sort_records_device<double, uint64_t>(workspace one byte short)", kWorkspace,
                  [&] { lsd::sort_records_device(reinterpret_cast<double*>(a64), reinterpret_cast<uint64_t*>(b32), ws, lsd::wide_workspace_bytes(n, 4, 64) - 1, n, true, 4, s); });

    // 16-bit sorts
    const lsdsort_key16_type bad16 = static_cast<lsdsort_key16_type>(9);
    expect_status("sort16_device(uint16_t*, key_type=9)", kInvalid, [&] { lsd::sort16_device(a16, nullptr, 0, n, false, nullptr, bad16, s); });
    expect_status("sort16_device(uint16_t*, odd keys)", kInvalid, [&] { lsd::sort16_device(odd16, nullptr, 0, n, true, b32, LSDSORT_KEY16_F16, s); });
    expect_status("sort16_device(uint16_t*, workspace one byte short)", kWorkspace,
                  [&] { lsd::sort16_device(a16, ws, lsd::keys16_workspace_bytes(n, true) - 1, n, true, b32, LSDSORT_KEY16_F16, s); });
    expect_status("sort16_device(int16_t*, odd keys)", kInvalid, [&] { lsd::sort16_device(reinterpret_cast<int16_t*>(odd16), nullptr, 0, n, true, b32, s); });
    expect_status("sort16_device(int16_t*, workspace one byte short)", kWorkspace,
                  [&] { lsd::sort16_device(reinterpret_cast<int16_t*>(a16), ws, lsd::keys16_workspace_bytes(n, true) - 1, n, true, b32, s); });

    // segments: 37 of them in 1000 keys
    expect_status("sort_segments(key_type=LSDSORT_KEY_U64)", kInvalid, [&] { lsd::sort_segments(a32, b32, 37, n, nullptr, 0, LSDSORT_KEY_U64, false, nullptr, s); });
    expect_status("sort_segments(null offsets)", kInvalid, [&] { lsd::sort_segments(a32, nullptr, 37, n, nullptr, 0, LSDSORT_KEY_F32, true, c32, s); });
    expect_status("sort_segments(null keys)", kInvalid, [&] { lsd::sort_segments(nullptr, b32, 37, n, nullptr, 0, LSDSORT_KEY_F32, true, c32, s); });
    expect_status("sort_segments(num_segments=0)", LSDSORT_OK, [&] { lsd::sort_segments(a32, b32, 0, n, nullptr, 0, LSDSORT_KEY_F32, true, c32, s); });
    expect_status("sort_segments(workspace one byte short)", kWorkspace,
                  [&] { lsd::sort_segments(a32, b32, 37, n, ws, lsd::segmented_workspace_bytes(n, 37, true) - 1, LSDSORT_KEY_F32, true, c32, s); });

    // the row entries.  rows = 5, cols = 3 with k = 4 or rank = 4 is invalid; with rows and cols swapped, or cols and k, it would not be
    const lsdsort_key_type bad32 = static_cast<lsdsort_key_type>(9);
    expect_status("topk(rows=5, cols=3, k=4)", kInvalid, [&] { lsd::topk(a32, 5, 3, 4, b32, c32, nullptr, 0, LSDSORT_KEY_I32, false, s); });
    expect_status("topk(rows=0, cols=3, k=4)", kInvalid, [&] { lsd::topk(a32, 0, 3, 4, b32, c32, nullptr, 0, LSDSORT_KEY_I32, false, s); });
    expect_status("topk(rows=5, cols=3, k=0)", LSDSORT_OK, [&] { lsd::topk(a32, 5, 3, 0, b32, c32, nullptr, 0, LSDSORT_KEY_I32, false, s); });
    expect_status("topk(key_type=9, largest=false)", kInvalid, [&] { lsd::topk(a32, 5, 33, 4, b32, c32, nullptr, 0, bad32, false, s); });
    expect_status("topk(null keys)", kInvalid, [&] { lsd::topk(nullptr, 5, 33, 4, b32, c32, nullptr, 0, LSDSORT_KEY_I32, false, s); });
    expect_status("topk(null output)", kInvalid, [&] { lsd::topk(a32, 5, 33, 4, nullptr, c32, nullptr, 0, LSDSORT_KEY_I32, false, s); });
    expect_status("topk(workspace one byte short)", kWorkspace,
                  [&] { lsd::topk(a32, 5, 33, 4, b32, c32, ws, lsd::topk_workspace_bytes(5, 33, 4) - 1, LSDSORT_KEY_I32, false, s); });

    expect_status("topk16_device(uint16_t*, rows=5, cols=3, k=4)", kInvalid, [&] { lsd::topk16_device(a16, 5, 3, 4, b16, c32, nullptr, 0, false, LSDSORT_KEY16_BF16, s); });
    expect_status("topk16_device(uint16_t*, largest=false, key_type=9)", kInvalid, [&] { lsd::topk16_device(a16, 5, 33, 4, b16, c32, nullptr, 0, false, bad16, s); });
    expect_status("topk16_device(uint16_t*, odd output)", kInvalid, [&] { lsd::topk16_device(a16, 5, 33, 4, odd16, c32, nullptr, 0, false, LSDSORT_KEY16_BF16, s); });
    expect_status("topk16_device(uint16_t*, null keys)", kInvalid, [&] { lsd::topk16_device(static_cast<const uint16_t*>(nullptr), 5, 33, 4, b16, c32, nullptr, 0, false, LSDSORT_KEY16_BF16, s); });
    expect_status("topk16_device(uint16_t*, workspace one byte short)", kWorkspace,
                  [&] { lsd::topk16_device(a16, 5, 33, 4, b16, c32, ws, lsd::topk16_workspace_bytes(5, 33, 4) - 1, false, LSDSORT_KEY16_BF16, s); });
    expect_status("topk16_device(int16_t*, rows=5, cols=3, k=4)", kInvalid,
                  [&] { lsd::topk16_device(reinterpret_cast<const int16_t*>(a16), 5, 3, 4, reinterpret_cast<int16_t*>(b16), c32, nullptr, 0, false, s); });
    expect_status("topk16_device(int16_t*, workspace one byte short)", kWorkspace, [&] {
        lsd::topk16_device(reinterpret_cast<const int16_t*>(a16), 5, 33, 4, reinterpret_cast<int16_t*>(b16), c32, ws, lsd::topk16_workspace_bytes(5, 33, 4) - 1, false, s);
    });

    expect_status("kth_device(uint32_t*, rows=5, cols=3, rank=4)", kInvalid, [&] { lsd::kth_device(a32, 5, 3, 4, b32, c32, nullptr, 0, true, s); });
    expect_status("kth_device(int32_t*, rows=5, cols=3, rank=4)", kInvalid,
                  [&] { lsd::kth_device(reinterpret_cast<const int32_t*>(a32), 5, 3, 4, reinterpret_cast<int32_t*>(b32), c32, nullptr, 0, true, s); });
    expect_status("kth_device(float*, rows=5, cols=3, rank=4)", kInvalid,
                  [&] { lsd::kth_device(reinterpret_cast<const float*>(a32), 5, 3, 4, reinterpret_cast<float*>(b32), c32, nullptr, 0, true, s); });
    expect_status("kth_device(uint32_t*, rows=5, cols=0, rank=4)", LSDSORT_OK, [&] { lsd::kth_device(a32, 5, 0, 4, b32, c32, nullptr, 0, true, s); });
    expect_status("kth_device(uint32_t*, output not 4-byte aligned)", kInvalid,
                  [&] { lsd::kth_device(a32, 5, 33, 4, reinterpret_cast<uint32_t*>(base + 8194), c32, nullptr, 0, true, s); });
    expect_status("kth_device(uint32_t*, workspace one byte short)", kWorkspace, [&] { lsd::kth_device(a32, 5, 33, 4, b32, c32, ws, lsd::kth_workspace_bytes(5, 33) - 1, true, s); });
    expect_status("kth_device(int32_t*, workspace one byte short)", kWorkspace, [&] {
        lsd::kth_device(reinterpret_cast<const int32_t*>(a32), 5, 33, 4, reinterpret_cast<int32_t*>(b32), c32, ws, lsd::kth_workspace_bytes(5, 33) - 1, true, s);
    });
    expect_status("kth_device(float*, workspace one byte short)", kWorkspace, [&] {
        lsd::kth_device(reinterpret_cast<const float*>(a32), 5, 33, 4, reinterpret_cast<float*>(b32), c32, ws, lsd::kth_workspace_bytes(5, 33) - 1, true, s);
    });

    expect_status("kth16_device(uint16_t*, rows=5, cols=3, rank=4)", kInvalid, [&] { lsd::kth16_device(a16, 5, 3, 4, b16, c32, nullptr, 0, true, LSDSORT_KEY16_F16, s); });
    expect_status("kth16_device(uint16_t*, largest=false, key_type=9)", kInvalid, [&] { lsd::kth16_device(a16, 5, 33, 4, b16, c32, nullptr, 0, false, bad16, s); });
    expect_status("kth16_device(uint16_t*, odd keys)", kInvalid, [&] { lsd::kth16_device(odd16, 5, 33, 4, b16, c32, nullptr, 0, true, LSDSORT_KEY16_F16, s); });
    expect_status("kth16_device(uint16_t*, workspace one byte short)", kWorkspace,
                  [&] { lsd::kth16_device(a16, 5, 33, 4, b16, c32, ws, lsd::kth16_workspace_bytes(5, 33) - 1, true, LSDSORT_KEY16_F16, s); });
    expect_status("kth16_device(int16_t*, rows=5, cols=3, rank=4)", kInvalid,
                  [&] { lsd::kth16_device(reinterpret_cast<const int16_t*>(a16), 5, 3, 4, reinterpret_cast<int16_t*>(b16), c32, nullptr, 0, true, s); });
    expect_status("kth16_device(int16_t*, workspace one byte short)", kWorkspace, [&] {
        lsd::kth16_device(reinterpret_cast<const int16_t*>(a16), 5, 33, 4, reinterpret_cast<int16_t*>(b16), c32, ws, lsd::kth16_workspace_bytes(5, 33) - 1, true, s);
    });

    expect_status("sort_rows16_device(uint16_t*, descending=false, key_type=9)", kInvalid, [&] { lsd::sort_rows16_device(a16, 5, 33, b16, c32, nullptr, 0, false, bad16, s); });
    expect_status("sort_rows16_device(uint16_t*, odd output)", kInvalid, [&] { lsd::sort_rows16_device(a16, 5, 33, odd16, c32, nullptr, 0, true, LSDSORT_KEY16_BF16, s); });
    expect_status("sort_rows16_device(uint16_t*, null keys)", kInvalid,
                  [&] { lsd::sort_rows16_device(static_cast<const uint16_t*>(nullptr), 5, 33, b16, c32, nullptr, 0, true, LSDSORT_KEY16_BF16, s); });
    expect_status("sort_rows16_device(uint16_t*, cols=0)", LSDSORT_OK, [&] { lsd::sort_rows16_device(a16, 5, 0, b16, c32, nullptr, 0, true, LSDSORT_KEY16_BF16, s); });
    expect_status("sort_rows16_device(uint16_t*, workspace one byte short)", kWorkspace,
                  [&] { lsd::sort_rows16_device(a16, 5, 33, b16, c32, ws, lsd::rows16_workspace_bytes(5, 33) - 1, true, LSDSORT_KEY16_BF16, s); });
    expect_status("sort_rows16_device(int16_t*, odd output)", kInvalid,
                  [&] { lsd::sort_rows16_device(reinterpret_cast<const int16_t*>(a16), 5, 33, reinterpret_cast<int16_t*>(odd16), c32, nullptr, 0, true, s); });
    expect_status("sort_rows16_device(int16_t*, workspace one byte short)", kWorkspace, [&] {
        lsd::sort_rows16_device(reinterpret_cast<const int16_t*>(a16), 5, 33, reinterpret_cast<int16_t*>(b16), c32, ws, lsd::rows16_workspace_bytes(5, 33) - 1, true, s);
    });

    expect_status("ran_hybrid_form(null workspace)", kInvalid, [&] { (void)lsd::ran_hybrid_form(nullptr, s); });
    expect_status("communicator::loopback(3)", kInvalid, [] { (void)lsd::communicator::loopback(3); });
}

}  // namespace

int main(int argc, char** argv)
{
    const bool no_device = argc > 1 && std::strcmp(argv[1], "--no-device") == 0;
    if (argc > 1 && !no_device) {
        std::fprintf(stderr, "usage: %s [--no-device]\n", argv[0]);
        return 2;
    }
    try {
        workspace_figures();
        argument_checks();
        if (no_device) {
            std::printf("device face test ok (--no-device)\n");
            return 0;
        }
        const auto t0 = std::chrono::steady_clock::now();
        hipStream_t stream = nullptr;
        HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        g_stream = stream;
        group_sorts32();
        group_sorts64();
        group_records();
        group_sort16();
        group_segments();
        group_topk();
        group_topk16();
        group_kth();
        group_kth16();
        group_rows16();
        group_shard();
        group_loopback();
        HIP(hipStreamDestroy(stream));
        std::printf("  %-22s %8.1f ms\n", "all groups", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    } catch (const std::exception& e) {
        fail("exception outside a checked call: %s", e.what());
    }
    std::printf("device face test ok\n");
    return 0;
}
