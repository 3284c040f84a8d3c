// Mesh components on the device (include/bnv_fusion.h, "Mesh components"): connected components of the faces over
// shared edges, their face counts and areas, and the filter that drops the small ones -- mesh.connected_components /
// mesh.remove_small_components bit for bit.  Order-free throughout: the union-find's roots are the smallest members
// whatever order the unions arrive in, areas are integers (rint(area * 2^50)) summed with integer atomics, and the
// ranking is a stable sort.  Sorts and prefix sums are rocPRIM's device primitives.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "../../include/bnv_fusion.h"
#include "mesh_face.hpp"

namespace bnv {
namespace {

constexpr int kCompThreads = 256;

struct CompHdr {
  unsigned long long tot_hi, tot_lo;   // sums of q >> 31 and q & (2^31 - 1) over all faces: the exact total
  int32_t n_comp, error, pad[2];
};

struct CompWs {
  CompHdr* hdr;
  uint64_t* ekey;      // [3T] undirected edges (min << 32 | max), pad kPadKey
  uint64_t* ekey_s;    // [3T] sorted
  int32_t* eface;      // [3T] face of every edge
  int32_t* eface_s;    // [3T]
  int64_t* q;          // [T] rint(area * 2^50)
  int32_t* parent;     // [T] union-find over faces (parent[t] <= t; paths halved, not flattened: readers still walk)
  int32_t* flag;       // [T] roots; later: kept faces
  int32_t* scan;       // [T] inclusive scans of flag
  unsigned long long* sum;   // [T] per component: sum of q
  // the filter only
  int32_t* labels;     // [T]
  long long* cnt;      // [T] faces per component
  double* area;        // [T]
  uint64_t* rkey;      // [T] ~bits(area) (pad: kPadKey): ascending = largest area first
  uint64_t* rkey_s;    // [T]
  int32_t* rval;       // [T] component labels
  int32_t* rval_s;     // [T]
  int32_t* keepc;      // [T] component kept
  int32_t* vflag;      // [V] vertex referenced by a kept face
  int32_t* vscan;      // [V]
  void* tmp;
  size_t tmp_bytes;
};

static size_t comp_ws_layout(int64_t V, int64_t T, char* base, CompWs* w) {
  Carver c(base);
  CompWs l{};
  l.hdr = c.take<CompHdr>(1);
  l.ekey = c.take<uint64_t>(3 * T);
  l.ekey_s = c.take<uint64_t>(3 * T);
  l.eface = c.take<int32_t>(3 * T);
  l.eface_s = c.take<int32_t>(3 * T);
  l.q = c.take<int64_t>(T);
  l.parent = c.take<int32_t>(T);
  l.flag = c.take<int32_t>(T);
  l.scan = c.take<int32_t>(T);
  l.sum = c.take<unsigned long long>(T);
  l.labels = c.take<int32_t>(T);
  l.cnt = c.take<long long>(T);
  l.area = c.take<double>(T);
  l.rkey = c.take<uint64_t>(T);
  l.rkey_s = c.take<uint64_t>(T);
  l.rval = c.take<int32_t>(T);
  l.rval_s = c.take<int32_t>(T);
  l.keepc = c.take<int32_t>(T);
  l.vflag = c.take<int32_t>(V);
  l.vscan = c.take<int32_t>(V);
  l.tmp_bytes = std::max(prim_sort_bytes<uint64_t>(3 * std::max<int64_t>(T, 1)), prim_scan_bytes(std::max(V, T)));
  l.tmp = c.take<char>(l.tmp_bytes);
  if (w) *w = l;
  return c.bytes();
}

__global__ __launch_bounds__(kCompThreads) void k_mc_vcheck(const float* __restrict__ vin, int64_t n, int32_t* err) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && !isfinite(vin[i])) atomicOr(err, (int32_t)kErrNonFinite);
}

// one thread per face: its three undirected edges, its area as an integer, the exact total (one atomic pair per block)
__global__ __launch_bounds__(kCompThreads) void k_mc_faces(const float* __restrict__ vin, int64_t V,
                                                           const int64_t* __restrict__ fin, int64_t T, CompWs w) {
  __shared__ unsigned long long s_hi[kCompThreads / 64], s_lo[kCompThreads / 64];
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t q = 0;
  if (t < T) {
    int64_t c[3];
    const bool ok = load_face(fin, t, V, c);
    int32_t err = ok ? 0 : (int32_t)kErrFaceIndex;
    uint64_t e[3] = {kPadKey, kPadKey, kPadKey};
    if (ok) {
      double n[3];
      if (!area_units(face_cross(vin, c, n), q)) err |= kErrArea;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const uint64_t a = (uint64_t)c[k], b = (uint64_t)c[(k + 1) % 3];
        if (a != b) e[k] = a < b ? (a << 32 | b) : (b << 32 | a);
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      w.ekey[t * 3 + k] = e[k];
      w.eface[t * 3 + k] = (int32_t)t;
    }
    w.q[t] = q;
    w.parent[t] = (int32_t)t;
    if (err) atomicOr(&w.hdr->error, err);
  }
  unsigned long long hi, lo;
  wave_area_total(q, hi, lo);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    s_hi[wave] = hi;
    s_lo[wave] = lo;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    hi = lo = 0;
#pragma unroll
    for (int k = 0; k < kCompThreads / 64; ++k) {
      hi += s_hi[k];
      lo += s_lo[k];
    }
    if (hi | lo) {
      atomicAdd(&w.hdr->tot_hi, hi);
      atomicAdd(&w.hdr->tot_lo, lo);
    }
  }
}

// neighbours in the sorted edge array with equal keys: faces on one edge
__global__ __launch_bounds__(kCompThreads) void k_mc_union(int64_t E, CompWs w) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < 1 || k >= E) return;
  const uint64_t e = w.ekey_s[k];
  if (e == kPadKey || e != w.ekey_s[k - 1]) return;
  uf_union<true>(w.parent, w.eface_s[k - 1], w.eface_s[k]);
}

__global__ __launch_bounds__(kCompThreads) void k_mc_roots(int64_t T, CompWs w) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  w.flag[t] = uf_find<true>(w.parent, (int32_t)t) == (int32_t)t;
}

// components numbered in ascending order of their smallest face; per component the face count and the integer area,
// pre-reduced over the runs of equal labels inside every block (one atomic pair per run per block: integer adds are
// associative, so any grouping gives the same sum).  Runs are found per wave; a run that reaches its wave's last lane
// and goes on in the next wave is handed to that wave through LDS.
__global__ __launch_bounds__(kCompThreads) void k_mc_labels(int64_t T, CompWs w, int32_t* __restrict__ labels,
                                                            long long* __restrict__ cnt) {
  constexpr int kWaves = kCompThreads / 64;
  __shared__ int32_t s_first[kWaves], s_last[kWaves], s_whole[kWaves];   // per wave: first / last label, one run only
  __shared__ unsigned long long s_sum[kWaves];                           // its last run's sums
  __shared__ long long s_cnt[kWaves];
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int32_t lab = -1;
  unsigned long long s = 0;
  long long n = 0;
  if (t < T) {
    lab = w.scan[uf_find<false>(w.parent, (int32_t)t)] - 1;
    labels[t] = lab;
    s = (unsigned long long)w.q[t];
    n = 1;
    if (t == T - 1) w.hdr->n_comp = w.scan[t];
  }
  const int32_t prev = __shfl_up(lab, 1, 64);
  const unsigned long long heads = __ballot(lane == 0 || prev != lab);
  const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));   // first lane of this lane's run
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long os = __shfl_up(s, d, 64);
    const long long on = __shfl_up(n, d, 64);
    if (lane - d >= start) {
      s += os;
      n += on;
    }
  }
  const int wave = threadIdx.x >> 6;
  if (lane == 0) s_first[wave] = lab;
  if (lane == 63) {
    s_last[wave] = lab;
    s_sum[wave] = s;
    s_cnt[wave] = n;
    s_whole[wave] = start == 0;
  }
  __syncthreads();
  const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
  if (!tail || lab < 0) return;
  if (lane == 63 && wave + 1 < kWaves && s_first[wave + 1] == lab) return;   // goes on in the next wave: left to it
  if (start == 0) {   // began at the wave's first lane: takes what the waves before left, as far as the run reaches back
    for (int j = wave - 1; j >= 0 && s_last[j] == lab; --j) {
      s += s_sum[j];
      n += s_cnt[j];
      if (!s_whole[j]) break;
    }
  }
  atomicAdd(&w.sum[lab], s);
  atomicAdd((unsigned long long*)&cnt[lab], (unsigned long long)n);
}

__global__ __launch_bounds__(kCompThreads) void k_mc_areas(int64_t T, CompWs w, double* __restrict__ area) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c == 0 && total_reaches_limit(w.hdr->tot_hi, w.hdr->tot_lo)) atomicOr(&w.hdr->error, (int32_t)kErrArea);
  if (c >= T || c >= w.hdr->n_comp) return;
  area[c] = __dmul_rn((double)(long long)w.sum[c], 1.0 / kAreaScale);
}

__global__ void k_mc_count(CompWs w, int64_t* count) { *count = w.hdr->error ? -1 : w.hdr->n_comp; }

// ---- the filter -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCompThreads) void k_mc_keepc(int64_t T, double min_area, int64_t min_faces, CompWs w) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= T) return;
  const bool live = c < w.hdr->n_comp;
  w.keepc[c] = live && w.area[c] >= min_area && w.cnt[c] >= min_faces;
  // non-negative doubles order as their bits; the complement puts the largest area first
  w.rkey[c] = live ? ~__builtin_bit_cast(uint64_t, w.area[c]) : kPadKey;
  w.rval[c] = (int32_t)c;
}

// after the stable sort: position = rank by (area descending, label ascending)
__global__ __launch_bounds__(kCompThreads) void k_mc_rank(int64_t T, int64_t keep_largest, CompWs w) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T || i < keep_largest) return;
  w.keepc[w.rval_s[i]] = 0;
}

__global__ __launch_bounds__(kCompThreads) void k_mc_fkeep(const int64_t* __restrict__ fin, int64_t T, int64_t V,
                                                           CompWs w) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  int64_t c[3];
  const int32_t keep = load_face(fin, t, V, c) && w.keepc[w.labels[t]];
  w.flag[t] = keep;
  if (keep) {
#pragma unroll
    for (int k = 0; k < 3; ++k) w.vflag[c[k]] = 1;
  }
}

__global__ __launch_bounds__(kCompThreads) void k_mc_vwrite(const float* __restrict__ vin, int64_t V, CompWs w,
                                                            float* __restrict__ vout) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V || !w.vflag[i]) return;
  const int64_t o = w.vscan[i] - 1;
#pragma unroll
  for (int a = 0; a < 3; ++a) vout[o * 3 + a] = vin[i * 3 + a];
}

__global__ __launch_bounds__(kCompThreads) void k_mc_fwrite(const int64_t* __restrict__ fin, int64_t T, CompWs w,
                                                            int64_t* __restrict__ fout) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T || !w.flag[t]) return;   // (a kept face's corners are in range: k_mc_fkeep)
  const int64_t o = w.scan[t] - 1;
#pragma unroll
  for (int k = 0; k < 3; ++k) fout[o * 3 + k] = (int64_t)(w.vscan[fin[t * 3 + k]] - 1);
}

__global__ void k_mc_fcounts(int64_t V, int64_t T, CompWs w, int64_t* counts) {
  const bool bad = w.hdr->error != 0;
  counts[0] = bad ? -1 : (V && T ? w.vscan[V - 1] : 0);
  counts[1] = bad ? -1 : (V && T ? w.scan[T - 1] : 0);
}

// the stages both entries share: labels, per-component face counts and areas, hdr->n_comp, hdr->error (T >= 1)
static int mesh_components_run(const float* vertices, int64_t V, const int64_t* faces, int64_t T, CompWs& w,
                               int32_t* labels, long long* cnt, double* area, hipStream_t s) {
  const int64_t E = 3 * T;
  size_t tb = w.tmp_bytes;
  BNV_HIP_CHECK(hipMemsetAsync(w.sum, 0, (size_t)T * 8, s));
  BNV_HIP_CHECK(hipMemsetAsync(cnt, 0, (size_t)T * 8, s));
  k_mc_faces<<<blocks_for(T, kCompThreads), kCompThreads, 0, s>>>(vertices, V, faces, T, w);
  BNV_PRIM_CHECK(rocprim::radix_sort_pairs(w.tmp, tb, w.ekey, w.ekey_s, w.eface, w.eface_s, (size_t)E, 0, 64, s));
  k_mc_union<<<blocks_for(E, kCompThreads), kCompThreads, 0, s>>>(E, w);
  k_mc_roots<<<blocks_for(T, kCompThreads), kCompThreads, 0, s>>>(T, w);
  BNV_PRIM_CHECK(rocprim::inclusive_scan(w.tmp, tb, w.flag, w.scan, (size_t)T, rocprim::plus<int32_t>(), s));
  k_mc_labels<<<blocks_for(T, kCompThreads), kCompThreads, 0, s>>>(T, w, labels, cnt);
  k_mc_areas<<<blocks_for(T, kCompThreads), kCompThreads, 0, s>>>(T, w, area);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

}  // namespace
}  // namespace bnv

using namespace bnv;

extern "C" {

int bnv_mesh_components_workspace_bytes(int64_t n_vertices, int64_t n_faces, int64_t* bytes) {
  if (!bytes || !mesh_sizes_ok(n_vertices, n_faces)) return BNV_ERR_INVALID_ARGUMENT;
  *bytes = (int64_t)comp_ws_layout(n_vertices, n_faces, nullptr, nullptr);
  return BNV_OK;
}

int bnv_mesh_components(const float* vertices, int64_t n_vertices, const int64_t* faces, int64_t n_faces,
                        void* workspace, int64_t ws_bytes, int32_t* labels, int64_t* n_faces_out, double* areas_out,
                        int64_t* count, bnv_stream_t stream) {
  const int64_t V = n_vertices, T = n_faces;
  if (!count || !mesh_sizes_ok(V, T)) return BNV_ERR_INVALID_ARGUMENT;
  if ((V && !vertices) || (T && (!faces || !labels || !n_faces_out || !areas_out))) return BNV_ERR_INVALID_ARGUMENT;
  CompWs w;
  if (!workspace || ws_bytes < (int64_t)comp_ws_layout(V, T, (char*)workspace, &w)) return BNV_ERR_WORKSPACE_TOO_SMALL;
  hipStream_t s = (hipStream_t)stream;
  BNV_HIP_CHECK(hipMemsetAsync(w.hdr, 0, sizeof(CompHdr), s));
  if (V) k_mc_vcheck<<<blocks_for(3 * V, kCompThreads), kCompThreads, 0, s>>>(vertices, 3 * V, &w.hdr->error);
  if (T) {
    const int rc = mesh_components_run(vertices, V, faces, T, w, labels, (long long*)n_faces_out, areas_out, s);
    if (rc != BNV_OK) return rc;
  }
  k_mc_count<<<1, 1, 0, s>>>(w, count);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

int bnv_mesh_filter_components(const float* vertices, int64_t n_vertices, const int64_t* faces, int64_t n_faces,
                               double min_area, int64_t min_faces, int64_t keep_largest, void* workspace,
                               int64_t ws_bytes, float* vertices_out, int64_t* faces_out, int64_t* counts,
                               bnv_stream_t stream) {
  const int64_t V = n_vertices, T = n_faces;
  if (!counts || !mesh_sizes_ok(V, T)) return BNV_ERR_INVALID_ARGUMENT;
  if (!(min_area >= 0.0) || !std::isfinite(min_area) || min_faces < 0 || keep_largest < 0)
    return BNV_ERR_INVALID_ARGUMENT;
  if ((V && (!vertices || !vertices_out)) || (T && (!faces || !faces_out))) return BNV_ERR_INVALID_ARGUMENT;
  CompWs w;
  if (!workspace || ws_bytes < (int64_t)comp_ws_layout(V, T, (char*)workspace, &w)) return BNV_ERR_WORKSPACE_TOO_SMALL;
  hipStream_t s = (hipStream_t)stream;
  BNV_HIP_CHECK(hipMemsetAsync(w.hdr, 0, sizeof(CompHdr), s));
  if (V) k_mc_vcheck<<<blocks_for(3 * V, kCompThreads), kCompThreads, 0, s>>>(vertices, 3 * V, &w.hdr->error);
  if (T) {
    const int rc = mesh_components_run(vertices, V, faces, T, w, w.labels, w.cnt, w.area, s);
    if (rc != BNV_OK) return rc;
    size_t tb = w.tmp_bytes;
    k_mc_keepc<<<blocks_for(T, kCompThreads), kCompThreads, 0, s>>>(T, min_area, min_faces, w);
    // The ranking sorts all T slots although only C are live: C is known on the device only, and reading it back would
    // be a host read.  Dead slots carry kPadKey.  A live component of area 0 has the same key (~bits(0.0) == kPadKey);
    // it still ranks before every dead slot because its index is smaller (live labels are 0..C-1) and the sort is
    // stable, and among live equals the smaller label comes first for the same reason.
    if (keep_largest > 0 && keep_largest < T) {   // (at most T components: a larger k keeps them all)
      BNV_PRIM_CHECK(rocprim::radix_sort_pairs(w.tmp, tb, w.rkey, w.rkey_s, w.rval, w.rval_s, (size_t)T, 0, 64, s));
      k_mc_rank<<<blocks_for(T, kCompThreads), kCompThreads, 0, s>>>(T, keep_largest, w);
    }
    if (V) {
      BNV_HIP_CHECK(hipMemsetAsync(w.vflag, 0, (size_t)V * 4, s));
      k_mc_fkeep<<<blocks_for(T, kCompThreads), kCompThreads, 0, s>>>(faces, T, V, w);
      BNV_PRIM_CHECK(rocprim::inclusive_scan(w.tmp, tb, w.flag, w.scan, (size_t)T, rocprim::plus<int32_t>(), s));
      BNV_PRIM_CHECK(rocprim::inclusive_scan(w.tmp, tb, w.vflag, w.vscan, (size_t)V, rocprim::plus<int32_t>(), s));
      k_mc_vwrite<<<blocks_for(V, kCompThreads), kCompThreads, 0, s>>>(vertices, V, w, vertices_out);
      k_mc_fwrite<<<blocks_for(T, kCompThreads), kCompThreads, 0, s>>>(faces, T, w, faces_out);
    }
  }
  k_mc_fcounts<<<1, 1, 0, s>>>(V, T, w, counts);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

}  // extern "C"
