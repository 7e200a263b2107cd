// pw_hip_host.h -- host-side plumbing shared by the three seed indexes (pw_seeds.hip, pw_mseeds.hip and pw_qseeds.hip, through
// pw_seed_host.h and pw_seed_kernels.h), overlap band selection (pw_overlap.hip), the complement table of the stranded paths
// (pw_complement.h) and the batch API (pwlib_api.cpp): checked HIP calls, a device buffer and an event that free themselves, rocPRIM's
// two-phase calls in one, the width of a sort-key field (bits_for).  Device code: the two binary searches of the seed joins.
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

// Device memory that grows on demand and is freed with its owner.  ensure() keeps nothing of the old contents: it frees
// the old block before it allocates the new one (hipFree waits for the device).  A successful call always leaves a
// usable pointer: a zero-byte request allocates 16 bytes.
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
};

struct DeviceEvent {
  hipEvent_t e = nullptr;
  DeviceEvent() = default;
  DeviceEvent(DeviceEvent&& o) noexcept : e(std::exchange(o.e, nullptr)) {}
  DeviceEvent& operator=(DeviceEvent&& o) noexcept { std::swap(e, o.e); return *this; }
  ~DeviceEvent() { if (e) (void)hipEventDestroy(e); }
  hipError_t create() { return hipEventCreate(&e); }
};

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
