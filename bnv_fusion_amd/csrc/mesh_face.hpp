// What the mesh operators share (meshpost.hip, meshcomp.hip, meshcolor.hip): the error bits, the per-face step (corner
// indices with their range check, float64 cross product and area, the area as an integer and its exact total), which
// decides which meshes every entry refuses, the union-find, the face step of the operators that merge vertices
// (meshpost.hip, meshsimplify.hip), and the rocPRIM temporary-storage helpers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "bnv_common.hpp"
#include "workspace.hpp"

namespace bnv {

enum : int32_t { kErrNonFinite = 1, kErrFaceIndex = 2, kErrExtent = 4, kErrArea = 8 };   // bits of a header's error word
constexpr double kAreaScale = 1125899906842624.0;   // 2^50: areas are summed as integers in units of 2^-50
constexpr double kAreaLimit = 4096.0;               // total area below 2^12: the integer sums stay below 2^62
constexpr uint64_t kPadKey = ~0ull;                 // sorts behind every live key
inline bool mesh_sizes_ok(int64_t V, int64_t T) { return V >= 0 && T >= 0 && V <= INT32_MAX - 1 && T <= INT32_MAX - 1; }

// ---- one face ---------------------------------------------------------------------------------------------------------
// the corner indices of face t; false when one lies outside [0, V)
__device__ __forceinline__ bool load_face(const int64_t* __restrict__ fin, int64_t t, int64_t V, int64_t c[3]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    c[k] = fin[t * 3 + k];
    ok &= c[k] >= 0 && c[k] < V;
  }
  return ok;
}

// n = (b - a) x (c - a) of the face with corners c (in range) -> its area, in float64 from the float32 coordinates, one
// rounding per operation in the order written (mesh._face_cross64)
__device__ __forceinline__ double face_cross(const float* __restrict__ vin, const int64_t c[3], double n[3]) {
  double p[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int a = 0; a < 3; ++a) p[k][a] = (double)vin[c[k] * 3 + a];
  const double e1x = __dsub_rn(p[1][0], p[0][0]), e1y = __dsub_rn(p[1][1], p[0][1]), e1z = __dsub_rn(p[1][2], p[0][2]);
  const double e2x = __dsub_rn(p[2][0], p[0][0]), e2y = __dsub_rn(p[2][1], p[0][1]), e2z = __dsub_rn(p[2][2], p[0][2]);
  n[0] = __dsub_rn(__dmul_rn(e1y, e2z), __dmul_rn(e1z, e2y));
  n[1] = __dsub_rn(__dmul_rn(e1z, e2x), __dmul_rn(e1x, e2z));
  n[2] = __dsub_rn(__dmul_rn(e1x, e2y), __dmul_rn(e1y, e2x));
  return __dmul_rn(
      0.5, __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(n[0], n[0]), __dmul_rn(n[1], n[1])), __dmul_rn(n[2], n[2]))));
}

// q = rint(area * 2^50); false (q untouched) when the face alone reaches the limit (non-finite corners fail the test)
__device__ __forceinline__ bool area_units(double area, int64_t& q) {
  const bool ok = area < kAreaLimit;
  if (ok) q = (int64_t)rint(__dmul_rn(area, kAreaScale));
  return ok;
}

// The exact total of the q's: sums of q >> 31 (hi) and of q & (2^31 - 1) (lo), here over the 64 lanes of a wave, into
// every lane; how a kernel publishes them is its own business.  The area reaches 2^12 when hi * 2^31 + lo >= 2^62.
__device__ __forceinline__ void wave_area_total(int64_t q, unsigned long long& hi, unsigned long long& lo) {
  hi = (unsigned long long)q >> 31;
  lo = (unsigned long long)q & 0x7fffffffull;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    hi += __shfl_xor(hi, d, 64);
    lo += __shfl_xor(lo, d, 64);
  }
}
__device__ __forceinline__ bool total_reaches_limit(unsigned long long hi, unsigned long long lo) {
  return hi + (lo >> 31) >= (1ull << 31);
}

// ---- union-find ---------------------------------------------------------------------------------------------------------
// Over parent[] (parent[x] <= x).  The weld walks plainly.  HALVE (the components: the whole room is one
// component of millions of faces) halves the path as it walks: a node's parent is only ever replaced by an ancestor
// further up (atomic min), so parent[x] <= x holds, every walk descends strictly, and the root found -- the
// component's smallest member -- does not depend on what other threads do meanwhile.
template <bool HALVE>
__device__ __forceinline__ int32_t uf_find(int32_t* parent, int32_t x) {
  while (true) {
    const int32_t p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == x) return x;
    if constexpr (HALVE) {
      const int32_t g = __hip_atomic_load(&parent[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (g == p) return p;
      __hip_atomic_fetch_min(&parent[x], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      x = g;
    } else {
      x = p;
    }
  }
}

// a root is only ever linked below a SMALLER root, so every component ends rooted at its smallest member
template <bool HALVE>
__device__ __forceinline__ void uf_union(int32_t* parent, int32_t a, int32_t b) {
  while (true) {
    a = uf_find<HALVE>(parent, a);
    b = uf_find<HALVE>(parent, b);
    if (a == b) return;
    if (a > b) {
      const int32_t t = a;
      a = b;
      b = t;
    }
    if (atomicCAS(&parent[b], b, a) == b) return;
  }
}

__device__ __forceinline__ int64_t lower_bound_u64(const uint64_t* __restrict__ s, int64_t n, uint64_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (s[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// ---- the face step: corners -> clusters, collapsed faces dropped, cyclic duplicates keep the first ---------------------
// (meshpost.hip and meshsimplify.hip).  A face's corners go vertex -> [unique point ->] cluster; a face with two equal
// clusters is dropped; a face rotated so its smallest cluster comes first (cyclic order kept) is a duplicate of an
// earlier face with the same rotation, and the smallest face index of every such key is kept through an integer
// atomic-min, so the answer does not depend on the order threads arrive in.  The pieces live in the caller's workspace.
struct FaceStep {
  const int32_t* inv;   // [V] vertex -> unique point, or null: the vertex itself
  const int32_t* cl;    // [V] unique point -> cluster
  int32_t* canon;       // [T, 3] face corners as cluster labels, rotated (canon[3t] = -1: dropped)
  int32_t* slot_of;     // [T] hash slot of every kept face
  int32_t* keep;        // [T]
  int32_t* fscan;       // [T] inclusive scan of keep
  int32_t* slots;       // [H] first face claiming a slot (-1 empty)
  uint32_t* minf;       // [H] smallest face index with the slot's key
  int32_t* flag;        // [V] 1 for every cluster a kept face references
  int32_t* error;       // the header's error word
  uint64_t H;
};

inline uint64_t face_hash_slots(int64_t T) {
  uint64_t h = 64;
  while (h < 2 * (uint64_t)T) h <<= 1;
  return h;
}

__device__ __forceinline__ bool face_clusters(const int64_t* __restrict__ fin, int64_t t, int64_t V,
                                              const FaceStep& w, int32_t c[3]) {
  int64_t v[3];
  if (!load_face(fin, t, V, v)) return false;
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = w.cl[w.inv ? w.inv[v[k]] : (int32_t)v[k]];
  return true;
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_face_canon(const int64_t* __restrict__ fin, int64_t T, int64_t V,
                                                        FaceStep w) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  int32_t c[3];
  int32_t* out = w.canon + t * 3;
  if (!face_clusters(fin, t, V, w, c)) {
    atomicOr(w.error, (int32_t)kErrFaceIndex);
    out[0] = -1;
    return;
  }
  if (c[0] == c[1] || c[1] == c[2] || c[0] == c[2]) {
    out[0] = -1;
    return;
  }
  const int lo = (c[1] < c[0]) ? ((c[2] < c[1]) ? 2 : 1) : ((c[2] < c[0]) ? 2 : 0);
  out[0] = c[lo];
  out[1] = c[(lo + 1) % 3];
  out[2] = c[(lo + 2) % 3];
}

__device__ __forceinline__ uint64_t face_hash(int32_t a, int32_t b, int32_t c) {
  uint64_t h = ((uint64_t)(uint32_t)a << 32 | (uint32_t)b) * 0x9E3779B97F4A7C15ull;
  h ^= (uint64_t)(uint32_t)c * 0xC2B2AE3D27D4EB4Full;
  h ^= h >> 29;
  h *= 0xBF58476D1CE4E5B9ull;
  h ^= h >> 32;
  return h;
}

// canon[] was written by the previous launch, so every thread reads every face's key coherently
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_face_insert(int64_t T, FaceStep w) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  const int32_t* f = w.canon + t * 3;
  if (f[0] < 0) return;
  const uint64_t mask = w.H - 1;
  for (uint64_t h = face_hash(f[0], f[1], f[2]) & mask;; h = (h + 1) & mask) {
    const int32_t owner = atomicCAS(&w.slots[h], -1, (int32_t)t);
    const int32_t* g = w.canon + (int64_t)(owner < 0 ? t : owner) * 3;
    if (owner < 0 || (g[0] == f[0] && g[1] == f[1] && g[2] == f[2])) {
      atomicMin(&w.minf[h], (uint32_t)t);
      w.slot_of[t] = (int32_t)h;
      return;
    }
  }
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_face_keep(int64_t T, FaceStep w) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  const int32_t* f = w.canon + t * 3;
  const int32_t keep = f[0] >= 0 && w.minf[w.slot_of[t]] == (uint32_t)t;
  w.keep[t] = keep;
  if (keep) {
    w.flag[f[0]] = 1;   // referenced cluster
    w.flag[f[1]] = 1;
    w.flag[f[2]] = 1;
  }
}

// ---- rocPRIM temporary storage: the bytes of a radix sort of n keys K (with int32 values, or alone), of an int32 scan --
template <class K>
inline size_t prim_sort_bytes(int64_t n, bool pairs = true) {
  size_t s = 0;
  const size_t m = (size_t)std::max<int64_t>(n, 1);
  K* k = nullptr;
  int32_t* v = nullptr;
  if (pairs) (void)rocprim::radix_sort_pairs(nullptr, s, k, k, v, v, m);
  else (void)rocprim::radix_sort_keys(nullptr, s, k, k, m);
  return s;
}
inline size_t prim_scan_bytes(int64_t n) {
  size_t s = 0;
  int32_t* v = nullptr;
  (void)rocprim::inclusive_scan(nullptr, s, v, v, (size_t)std::max<int64_t>(n, 1), rocprim::plus<int32_t>());
  return s;
}

// rocPRIM takes the temporary storage size by reference: every call is handed the whole block (`w.tmp_bytes` into `tb`)
#define BNV_PRIM_CHECK(expr) do { tb = w.tmp_bytes; BNV_HIP_CHECK(expr); } while (0)

// The face step's launches (T > 0): keep[] and its scan fscan[], flag[] (cleared here over n_flags entries).
inline int run_face_step(const int64_t* faces, int64_t T, int64_t V, const FaceStep& f, int64_t n_flags, void* tmp,
                         size_t tmp_bytes, hipStream_t s) {
  constexpr int kThreads = 256;
  BNV_HIP_CHECK(hipMemsetAsync(f.slots, 0xff, (size_t)f.H * 4, s));
  BNV_HIP_CHECK(hipMemsetAsync(f.minf, 0xff, (size_t)f.H * 4, s));
  BNV_HIP_CHECK(hipMemsetAsync(f.flag, 0, (size_t)n_flags * 4, s));
  k_face_canon<kThreads><<<blocks_for(T, kThreads), kThreads, 0, s>>>(faces, T, V, f);
  k_face_insert<kThreads><<<blocks_for(T, kThreads), kThreads, 0, s>>>(T, f);
  k_face_keep<kThreads><<<blocks_for(T, kThreads), kThreads, 0, s>>>(T, f);
  BNV_HIP_CHECK(rocprim::inclusive_scan(tmp, tmp_bytes, f.keep, f.fscan, (size_t)T, rocprim::plus<int32_t>(), s));
  return BNV_OK;
}

}  // namespace bnv
