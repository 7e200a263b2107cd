// pw_hip_host.h -- host-side plumbing shared by the three seed indexes (pw_seeds.hip, pw_mseeds.hip and pw_qseeds.hip, through
// pw_seed_host.h and pw_seed_kernels.h), overlap band selection (pw_overlap.hip), the k-mer table (pw_kmers.hip), the complement
// table of the stranded paths (pw_complement.h) and the batch API (pwlib_api.cpp): checked HIP calls, device memory and an event
// that free themselves, the checked copy of a host array into a device array (upload), the grid of one thread per row
// (rows_grid, kBlock256), rocPRIM's two-phase calls in one, the width of a sort-key field (bits_for).  Device code: the two
// binary searches of the seed joins.  Device memory is a DeviceArray<T>; DeviceBuffer only in the cases listed at its definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <utility>

// Return -1 from the enclosing function when `call` fails, after handing "<call>: <hip error string>" to `sink` (each
// C API keeps its own error channel).
#define PW_HIP_CHECK(sink, call)                                                                   \
  do {                                                                                             \
    const hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess) { sink(std::string(#call) + ": " + hipGetErrorString(e_)); return -1; }  \
  } while (0)

// Device memory that grows on demand and is freed with its owner, without an element type: `cap` bytes at `p`.  ensure()
// keeps nothing of the old contents: it frees the old block before it allocates the new one (hipFree waits for the device).
// A successful call always leaves a usable pointer: a zero-byte request allocates 16 bytes.
// Only for memory that has no single static element type (as<T>() names the type at the use):
//   - rocPRIM's scratch (`tmp`);
//   - key arrays whose width, uint32_t or uint64_t (WordSpace::key32), is chosen at run time: keys_in, keys_s, keys_t, keys,
//     rkeys of the three seed indexes and of encode_sort;
//   - staging that is deliberately reused for two types (none at present: the `kin` that graph_finish borrows as `wide`
//     holds uint64_t both times and is a DeviceArray);
//   - the batch's memory in its score type, int32_t or double: pw_batch::d_hdump, d_subst and d_state.
// Everything else is a DeviceArray<T>.
struct DeviceBuffer {
  void* p = nullptr;
  size_t cap = 0;
  DeviceBuffer() = default;
  DeviceBuffer(DeviceBuffer&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
  ~DeviceBuffer() { if (p) (void)hipFree(p); }
  hipError_t ensure(size_t bytes) {
    if (p && bytes <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    const hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
    if (e != hipSuccess) { p = nullptr; return e; }
    cap = bytes ? bytes : 16;
    return hipSuccess;
  }
  template <class T> T* as() const { return static_cast<T*>(p); }
};

// DeviceBuffer's contract with an element type: `p` points at T, ensure() counts elements (grow-only, the old block freed
// first, old contents not kept, a zero count allocates 16 bytes), bytes(count) is what `count` elements take in a copy or a
// memset.  T is exactly the pointee type the kernels and rocPRIM take: it is part of rocPRIM's instantiations.  (Hidden, as
// upload() below: plumbing of each unit, not symbols the library exports.)
template <class T>
struct __attribute__((visibility("hidden"))) DeviceArray {
  T* p = nullptr;
  size_t cap = 0;                                      // elements
  DeviceArray() = default;
  DeviceArray(DeviceArray&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  DeviceArray& operator=(DeviceArray&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
  ~DeviceArray() { if (p) (void)hipFree(p); }
  static constexpr size_t bytes(size_t count) { return count * sizeof(T); }
  hipError_t ensure(size_t count) {
    if (p && count <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, count ? bytes(count) : 16);
    if (e != hipSuccess) return e;
    p = static_cast<T*>(q);
    cap = count ? count : 16 / sizeof(T);
    return hipSuccess;
  }
  const T* cp() const { return p; }                    // read-only: a rocPRIM input's pointer type is part of the instantiation
  // the same memory as a type that splits no element: uint64_t for counts written as unsigned long long, int32_t for rows of int2
  template <class U> U* as() const {
    static_assert(sizeof(T) % sizeof(U) == 0, "as<U>() splits no element");
    return reinterpret_cast<U*>(p);
  }
};

struct DeviceEvent {
  hipEvent_t e = nullptr;
  DeviceEvent() = default;
  DeviceEvent(DeviceEvent&& o) noexcept : e(std::exchange(o.e, nullptr)) {}
  DeviceEvent& operator=(DeviceEvent&& o) noexcept { std::swap(e, o.e); return *this; }
  ~DeviceEvent() { if (e) (void)hipEventDestroy(e); }
  hipError_t create() { return hipEventCreate(&e); }
};

// `arr` grown to `count` elements and filled from the host, 0 or -1 with the HIP error in `sink` (as PW_HIP_CHECK's).  Without
// a stream the copy is hipMemcpy; with one, null included, hipMemcpyAsync on it.  Nothing is copied when count is 0.
template <class Sink, class T>
__attribute__((visibility("hidden"))) int upload(Sink&& sink, DeviceArray<T>& arr, const T* host, size_t count) {
  PW_HIP_CHECK(sink, arr.ensure(count));
  if (count) PW_HIP_CHECK(sink, hipMemcpy(arr.p, host, arr.bytes(count), hipMemcpyHostToDevice));
  return 0;
}
template <class Sink, class T>
__attribute__((visibility("hidden"))) int upload(Sink&& sink, DeviceArray<T>& arr, const T* host, size_t count, hipStream_t st) {
  PW_HIP_CHECK(sink, arr.ensure(count));
  if (count) PW_HIP_CHECK(sink, hipMemcpyAsync(arr.p, host, arr.bytes(count), hipMemcpyHostToDevice, st));
  return 0;
}

// one thread per row in workgroups of 256: the launch shape of nearly every kernel of the seed, overlap and k-mer paths
const dim3 kBlock256(256);
inline dim3 rows_grid(uint64_t n) { return dim3((unsigned)((n + 255) / 256)); }

// A rocPRIM algorithm in one call: f(tmp, bytes) with tmp = nullptr asks for the scratch size, `scratch` grows to it,
// then f runs in it.  (A null scratch pointer would make rocPRIM answer the size query again and do nothing.)
template <typename F>
hipError_t rocprim_run(DeviceBuffer& scratch, F&& f) {
  size_t bytes = 0;
  hipError_t e = f(nullptr, bytes);
  if (e == hipSuccess) e = scratch.ensure(bytes);
  return e == hipSuccess ? f(scratch.p, bytes) : e;
}

// the width of a sort-key field that holds 0 .. maxval
inline int bits_for(uint64_t maxval) { int b = 1; while ((maxval >> b) != 0) b++; return b; }

// First index of the ascending a[0, n) whose element is >= key (lower) / > key (upper).
template <typename K>
__device__ __forceinline__ int64_t lower_bound_dev(const K* __restrict__ a, int64_t n, K key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (a[mid] < key) lo = mid + 1; else hi = mid; }
  return lo;
}
template <typename K>
__device__ __forceinline__ int64_t upper_bound_dev(const K* __restrict__ a, int64_t n, K key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (a[mid] <= key) lo = mid + 1; else hi = mid; }
  return lo;
}
