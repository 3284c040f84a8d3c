// Mesh simplification on the device: vertex clustering on a uniform grid with quadric placement -- mesh.simplify_mesh
// with the same output bit for bit.  The specification is in include/bnv_fusion.h ("Mesh simplification") and, as code,
// in tests/mesh_simplify_restatement.py; the kernels below mirror it operation by operation.  All arithmetic is float64
// with one rounding per operation in the order written; every sum runs in a stated order inside ONE thread (a cluster's
// vertices in ascending index, its corners in ascending corner id), which a stable radix sort of the cluster numbers
// provides.  No float atomics, so two runs give the same bits.  The face step and its compaction are mesh_face.hpp's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "../../include/bnv_fusion.h"
#include "mesh_face.hpp"

namespace bnv {
namespace {

constexpr int kSimpThreads = 256;       // four waves of 64
constexpr uint32_t kPadCluster = ~0u;   // corners of faces with an index out of range: behind every cluster
constexpr uint32_t kNoCorner = ~0u;
constexpr double kCellExtent = 1048576.0;   // 2^20: |x| / h below it, so every axis index + 2^20 fits 21 bits
constexpr int64_t kMaxFaces = (int64_t)1 << 30;   // corner ids 3 t + k fit 32 bits

inline bool simplify_sizes_ok(int64_t V, int64_t T) { return V >= 0 && T >= 0 && V <= INT32_MAX - 1 && T <= kMaxFaces; }

struct SimpHdr {
  int32_t n_clusters, error, pad[6];
};

struct SimpWs {
  SimpHdr* hdr;
  uint64_t* key;      // [V] cell keys
  uint64_t* key_s;    // [V] sorted
  int32_t* pa;        // [V] vertex indices
  int32_t* pb;        // [V] vertex indices in key order (ties in ascending index)
  int32_t* flag;      // [V] heads of the sorted keys; later: referenced clusters
  int32_t* scan;      // [V] inclusive scans of flag
  int32_t* cl;        // [V] vertex -> cluster
  int32_t* vstart;    // [V] first sorted vertex of every cluster
  uint32_t* qstart;   // [V] first sorted corner of every cluster (kNoCorner: none; 3 T can pass 2^31)
  float* pos;         // [V, 3] cluster positions
  uint32_t* ck;       // [3T] cluster of every corner (kPadCluster: the face has an index out of range)
  uint32_t* ck_s;     // [3T] sorted
  int32_t* ca;        // [3T] corner ids (the bits of a uint32)
  int32_t* cb;        // [3T] corner ids in cluster order (ties in ascending id)
  int32_t* canon;     // the face step's pieces (mesh_face.hpp)
  int32_t* slot_of;
  int32_t* keep;
  int32_t* fscan;
  int32_t* slots;
  uint32_t* minf;
  void* tmp;          // rocPRIM temporary storage
  size_t tmp_bytes;
  uint64_t H;
};

static size_t simp_ws_layout(int64_t V, int64_t T, char* base, SimpWs* w) {
  Carver c(base);
  SimpWs l{};
  l.H = face_hash_slots(T);
  l.hdr = c.take<SimpHdr>(1);
  l.key = c.take<uint64_t>(V);
  l.key_s = c.take<uint64_t>(V);
  l.pa = c.take<int32_t>(V);
  l.pb = c.take<int32_t>(V);
  l.flag = c.take<int32_t>(V);
  l.scan = c.take<int32_t>(V);
  l.cl = c.take<int32_t>(V);
  l.vstart = c.take<int32_t>(V);
  l.qstart = c.take<uint32_t>(V);
  l.pos = c.take<float>(3 * V);
  l.ck = c.take<uint32_t>(3 * T);
  l.ck_s = c.take<uint32_t>(3 * T);
  l.ca = c.take<int32_t>(3 * T);
  l.cb = c.take<int32_t>(3 * T);
  l.canon = c.take<int32_t>(3 * T);
  l.slot_of = c.take<int32_t>(T);
  l.keep = c.take<int32_t>(T);
  l.fscan = c.take<int32_t>(T);
  l.slots = c.take<int32_t>(l.H);
  l.minf = c.take<uint32_t>(l.H);
  l.tmp_bytes = std::max({prim_sort_bytes<uint64_t>(V), prim_sort_bytes<uint32_t>(3 * T), prim_scan_bytes(std::max(V, T))});
  l.tmp = c.take<char>(l.tmp_bytes);
  if (w) *w = l;
  return c.bytes();
}

static FaceStep face_step(const SimpWs& w) {
  return FaceStep{nullptr, w.cl, w.canon, w.slot_of, w.keep, w.fscan, w.slots, w.minf, w.flag, &w.hdr->error, w.H};
}

// ---- 1. cells: i_a = floor(x_a / h), key = (ix + 2^20) << 42 | (iy + 2^20) << 21 | (iz + 2^20) --------------------------
__global__ __launch_bounds__(kSimpThreads) void k_ms_keys(const float* __restrict__ vin, int64_t V, double h, SimpWs w) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V) return;
  int32_t err = 0;
  uint64_t key = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float x = vin[i * 3 + a];
    int64_t c = 0;
    if (!isfinite(x)) {
      err |= kErrNonFinite;
    } else {
      const double q = __ddiv_rn((double)x, h);
      if (fabs(q) < kCellExtent) c = (int64_t)floor(q);
      else err |= kErrExtent;
    }
    key = key << 21 | (uint64_t)(c + 1048576);
  }
  w.key[i] = key;
  w.pa[i] = (int32_t)i;
  if (err) atomicOr(&w.hdr->error, err);
}

__global__ __launch_bounds__(kSimpThreads) void k_ms_heads(int64_t V, SimpWs w) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= V) return;
  w.flag[k] = k == 0 || w.key_s[k] != w.key_s[k - 1];
}

// clusters = the distinct keys in ascending order
__global__ __launch_bounds__(kSimpThreads) void k_ms_clusters(int64_t V, SimpWs w) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= V) return;
  const int32_t c = w.scan[k] - 1;
  w.cl[w.pb[k]] = c;
  w.qstart[k] = kNoCorner;
  if (w.flag[k]) w.vstart[c] = (int32_t)k;
  if (k == V - 1) w.hdr->n_clusters = c + 1;
}

// ---- 2. corners: id 3 t + k -> the cluster of its vertex -------------------------------------------------------------
__global__ __launch_bounds__(kSimpThreads) void k_ms_corners(const int64_t* __restrict__ fin, int64_t T, int64_t V,
                                                            SimpWs w) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  int64_t v[3];
  const bool ok = load_face(fin, t, V, v);   // (the face step reports the index error)
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    w.ck[t * 3 + k] = ok ? (uint32_t)w.cl[v[k]] : kPadCluster;
    w.ca[t * 3 + k] = (int32_t)(uint32_t)(t * 3 + k);
  }
}

__global__ __launch_bounds__(kSimpThreads) void k_ms_qstart(int64_t Q, SimpWs w) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= Q) return;
  const uint32_t c = w.ck_s[k];
  if (c != kPadCluster && (k == 0 || w.ck_s[k - 1] != c)) w.qstart[c] = (uint32_t)k;
}

// ---- 3. placement: one thread per cluster, both sums in their stated order ----------------------------------------------
__global__ __launch_bounds__(kSimpThreads) void k_ms_place(const float* __restrict__ vin, const int64_t* __restrict__ fin,
                                                          int64_t V, int64_t Q, double h, int quadric, double min_det,
                                                          SimpWs w) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= w.hdr->n_clusters) return;
  // mean: the float64 coordinates of the cluster's vertices in ascending index, / their number
  const int64_t k0 = w.vstart[c];
  const uint64_t key = w.key_s[k0];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  int64_t cnt = 0;
  for (int64_t k = k0; k < V && w.key_s[k] == key; ++k, ++cnt) {
    const int64_t m = w.pb[k];
    s0 = __dadd_rn(s0, (double)vin[m * 3]);
    s1 = __dadd_rn(s1, (double)vin[m * 3 + 1]);
    s2 = __dadd_rn(s2, (double)vin[m * 3 + 2]);
  }
  const double dc = (double)cnt;
  float o0 = (float)__ddiv_rn(s0, dc), o1 = (float)__ddiv_rn(s1, dc), o2 = (float)__ddiv_rn(s2, dc);
  const uint32_t qs = w.qstart[c];
  if (quadric && qs != kNoCorner) {
    // cell centre (i_a + 0.5) * h
    const double cx = __dmul_rn((double)((int64_t)(key >> 42) - 1048576) + 0.5, h);
    const double cy = __dmul_rn((double)((int64_t)((key >> 21) & 0x1fffff) - 1048576) + 0.5, h);
    const double cz = __dmul_rn((double)((int64_t)(key & 0x1fffff) - 1048576) + 0.5, h);
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    for (int64_t k = qs; k < Q && w.ck_s[k] == (uint32_t)c; ++k) {
      const int64_t t = (int64_t)((uint32_t)w.cb[k] / 3u);
      const int64_t i0 = fin[t * 3], i1 = fin[t * 3 + 1], i2 = fin[t * 3 + 2];   // in range: the corner has a cluster
      if (i0 == i1 || i1 == i2 || i0 == i2) continue;
      const double p0x = __dsub_rn((double)vin[i0 * 3], cx), p0y = __dsub_rn((double)vin[i0 * 3 + 1], cy),
                   p0z = __dsub_rn((double)vin[i0 * 3 + 2], cz);
      const double e1x = __dsub_rn(__dsub_rn((double)vin[i1 * 3], cx), p0x),
                   e1y = __dsub_rn(__dsub_rn((double)vin[i1 * 3 + 1], cy), p0y),
                   e1z = __dsub_rn(__dsub_rn((double)vin[i1 * 3 + 2], cz), p0z);
      const double e2x = __dsub_rn(__dsub_rn((double)vin[i2 * 3], cx), p0x),
                   e2y = __dsub_rn(__dsub_rn((double)vin[i2 * 3 + 1], cy), p0y),
                   e2z = __dsub_rn(__dsub_rn((double)vin[i2 * 3 + 2], cz), p0z);
      const double n0 = __dsub_rn(__dmul_rn(e1y, e2z), __dmul_rn(e1z, e2y));
      const double n1 = __dsub_rn(__dmul_rn(e1z, e2x), __dmul_rn(e1x, e2z));
      const double n2 = __dsub_rn(__dmul_rn(e1x, e2y), __dmul_rn(e1y, e2x));
      const double L = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(n0, n0), __dmul_rn(n1, n1)), __dmul_rn(n2, n2)));
      if (L == 0.0) continue;
      const double u0 = __ddiv_rn(n0, L), u1 = __ddiv_rn(n1, L), u2 = __ddiv_rn(n2, L);
      const double wt = __dmul_rn(0.5, L);
      const double d = -__dadd_rn(__dadd_rn(__dmul_rn(u0, p0x), __dmul_rn(u1, p0y)), __dmul_rn(u2, p0z));
      const double wu0 = __dmul_rn(wt, u0), wu1 = __dmul_rn(wt, u1), wu2 = __dmul_rn(wt, u2), wd = __dmul_rn(wt, d);
      a00 = __dadd_rn(a00, __dmul_rn(wu0, u0));
      a01 = __dadd_rn(a01, __dmul_rn(wu0, u1));
      a02 = __dadd_rn(a02, __dmul_rn(wu0, u2));
      a11 = __dadd_rn(a11, __dmul_rn(wu1, u1));
      a12 = __dadd_rn(a12, __dmul_rn(wu1, u2));
      a22 = __dadd_rn(a22, __dmul_rn(wu2, u2));
      b0 = __dadd_rn(b0, __dmul_rn(wd, u0));
      b1 = __dadd_rn(b1, __dmul_rn(wd, u1));
      b2 = __dadd_rn(b2, __dmul_rn(wd, u2));
    }
    // x = adj(A) (-b) / det, det by the cofactors of the first row
    const double c00 = __dsub_rn(__dmul_rn(a11, a22), __dmul_rn(a12, a12));
    const double c01 = __dsub_rn(__dmul_rn(a02, a12), __dmul_rn(a01, a22));
    const double c02 = __dsub_rn(__dmul_rn(a01, a12), __dmul_rn(a02, a11));
    const double c11 = __dsub_rn(__dmul_rn(a00, a22), __dmul_rn(a02, a02));
    const double c12 = __dsub_rn(__dmul_rn(a01, a02), __dmul_rn(a00, a12));
    const double c22 = __dsub_rn(__dmul_rn(a00, a11), __dmul_rn(a01, a01));
    const double det = __dadd_rn(__dadd_rn(__dmul_rn(a00, c00), __dmul_rn(a01, c01)), __dmul_rn(a02, c02));
    const double tr = __dadd_rn(__dadd_rn(a00, a11), a22);
    const double r0 = -b0, r1 = -b1, r2 = -b2;
    const double x0 = __ddiv_rn(__dadd_rn(__dadd_rn(__dmul_rn(c00, r0), __dmul_rn(c01, r1)), __dmul_rn(c02, r2)), det);
    const double x1 = __ddiv_rn(__dadd_rn(__dadd_rn(__dmul_rn(c01, r0), __dmul_rn(c11, r1)), __dmul_rn(c12, r2)), det);
    const double x2 = __ddiv_rn(__dadd_rn(__dadd_rn(__dmul_rn(c02, r0), __dmul_rn(c12, r1)), __dmul_rn(c22, r2)), det);
    const double m = __ddiv_rn(tr, 3.0);
    const double thr = __dmul_rn(min_det, __dmul_rn(__dmul_rn(m, m), m));
    // (det = 0 leaves x infinite or NaN: both fail the last test)
    if (tr > 0.0 && fabs(det) >= thr && fabs(x0) <= h && fabs(x1) <= h && fabs(x2) <= h) {
      o0 = (float)__dadd_rn(cx, x0);
      o1 = (float)__dadd_rn(cy, x1);
      o2 = (float)__dadd_rn(cz, x2);
    }
  }
  w.pos[c * 3] = o0;
  w.pos[c * 3 + 1] = o1;
  w.pos[c * 3 + 2] = o2;
}

// ---- 4. referenced clusters only, in key order; faces renumbered, in input order ------------------------------------------
__global__ __launch_bounds__(kSimpThreads) void k_ms_vert_write(int64_t V, int64_t T, SimpWs w, float* __restrict__ vout,
                                                               int64_t* __restrict__ counts) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c == 0) {
    const bool bad = w.hdr->error != 0;
    counts[0] = bad ? -1 : w.scan[V - 1];
    counts[1] = bad ? -1 : w.fscan[T - 1];
  }
  if (c >= w.hdr->n_clusters || !w.flag[c]) return;
  const int64_t o = w.scan[c] - 1;
#pragma unroll
  for (int a = 0; a < 3; ++a) vout[o * 3 + a] = w.pos[c * 3 + a];
}

__global__ __launch_bounds__(kSimpThreads) void k_ms_face_write(const int64_t* __restrict__ fin, int64_t T, int64_t V,
                                                               SimpWs w, FaceStep fs, int64_t* __restrict__ fout) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  int32_t c[3];
  if (!w.keep[t] || !face_clusters(fin, t, V, fs, c)) return;
  const int64_t o = w.fscan[t] - 1;
#pragma unroll
  for (int k = 0; k < 3; ++k) fout[o * 3 + k] = (int64_t)(w.scan[c[k]] - 1);   // original corner order
}

// no vertices or no faces: an empty mesh (a face of a mesh without vertices has an index out of range)
__global__ __launch_bounds__(kSimpThreads) void k_ms_empty(const float* __restrict__ vin, int64_t V, int64_t T, double h,
                                                          int64_t* __restrict__ counts, int32_t* __restrict__ err) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) counts[0] = counts[1] = (T && !V) ? -1 : 0;
  if (i >= 3 * V) return;
  const float x = vin[i];
  if (!isfinite(x) || !(fabs(__ddiv_rn((double)x, h)) < kCellExtent)) atomicOr(err, 1);
}
__global__ void k_ms_empty_counts(const int32_t* err, int64_t* counts) {
  if (*err) counts[0] = counts[1] = -1;
}

}  // namespace
}  // namespace bnv

using namespace bnv;

extern "C" {

int bnv_mesh_simplify_bytes(int64_t n_vertices, int64_t n_faces, int64_t* bytes) {
  if (!bytes || !simplify_sizes_ok(n_vertices, n_faces)) return BNV_ERR_INVALID_ARGUMENT;
  *bytes = (int64_t)simp_ws_layout(n_vertices, n_faces, nullptr, nullptr);
  return BNV_OK;
}

int bnv_mesh_simplify(const float* vertices, int64_t n_vertices, const int64_t* faces, int64_t n_faces, double cell,
                      int32_t placement, double min_det, void* workspace, int64_t ws_bytes, float* vertices_out,
                      int64_t* faces_out, int64_t* counts, bnv_stream_t stream) {
  const int64_t V = n_vertices, T = n_faces, Q = 3 * n_faces;
  if (!counts || !simplify_sizes_ok(V, T)) return BNV_ERR_INVALID_ARGUMENT;
  if (!std::isfinite(cell) || !(cell > 0.0) || !std::isfinite(min_det) || !(min_det >= 0.0)) return BNV_ERR_INVALID_ARGUMENT;
  if (placement != BNV_SIMPLIFY_QUADRIC && placement != BNV_SIMPLIFY_MEAN) return BNV_ERR_INVALID_ARGUMENT;
  if ((V && (!vertices || !vertices_out)) || (T && (!faces || !faces_out))) return BNV_ERR_INVALID_ARGUMENT;
  SimpWs w;
  if (!workspace || ws_bytes < (int64_t)simp_ws_layout(V, T, (char*)workspace, &w)) return BNV_ERR_WORKSPACE_TOO_SMALL;
  hipStream_t s = (hipStream_t)stream;
  BNV_HIP_CHECK(hipMemsetAsync(w.hdr, 0, sizeof(SimpHdr), s));
  if (V == 0 || T == 0) {
    k_ms_empty<<<std::max(1u, blocks_for(3 * V, kSimpThreads)), kSimpThreads, 0, s>>>(vertices, V, T, cell, counts,
                                                                                     &w.hdr->error);
    k_ms_empty_counts<<<1, 1, 0, s>>>(&w.hdr->error, counts);
    BNV_LAUNCH_CHECK();
    return BNV_OK;
  }
  const size_t v = (size_t)V;
  size_t tb = w.tmp_bytes;
  // 1. cells and clusters (a stable sort: a cluster's vertices in ascending index)
  k_ms_keys<<<blocks_for(V, kSimpThreads), kSimpThreads, 0, s>>>(vertices, V, cell, w);
  BNV_PRIM_CHECK(rocprim::radix_sort_pairs(w.tmp, tb, w.key, w.key_s, w.pa, w.pb, v, 0, 63, s));
  k_ms_heads<<<blocks_for(V, kSimpThreads), kSimpThreads, 0, s>>>(V, w);
  BNV_PRIM_CHECK(rocprim::inclusive_scan(w.tmp, tb, w.flag, w.scan, v, rocprim::plus<int32_t>(), s));
  k_ms_clusters<<<blocks_for(V, kSimpThreads), kSimpThreads, 0, s>>>(V, w);
  // 2. corners by cluster (stable: ascending corner id)
  if (placement == BNV_SIMPLIFY_QUADRIC) {
    k_ms_corners<<<blocks_for(T, kSimpThreads), kSimpThreads, 0, s>>>(faces, T, V, w);
    BNV_PRIM_CHECK(rocprim::radix_sort_pairs(w.tmp, tb, w.ck, w.ck_s, w.ca, w.cb, (size_t)Q, 0, 32, s));
    k_ms_qstart<<<blocks_for(Q, kSimpThreads), kSimpThreads, 0, s>>>(Q, w);
  }
  // 3. positions
  k_ms_place<<<blocks_for(V, kSimpThreads), kSimpThreads, 0, s>>>(vertices, faces, V, Q, cell,
                                                                 placement == BNV_SIMPLIFY_QUADRIC, min_det, w);
  // 4. faces, referenced clusters, output
  const FaceStep fs = face_step(w);
  BNV_TRY(run_face_step(faces, T, V, fs, V, w.tmp, w.tmp_bytes, s));
  BNV_PRIM_CHECK(rocprim::inclusive_scan(w.tmp, tb, w.flag, w.scan, v, rocprim::plus<int32_t>(), s));
  k_ms_vert_write<<<blocks_for(V, kSimpThreads), kSimpThreads, 0, s>>>(V, T, w, vertices_out, counts);
  k_ms_face_write<<<blocks_for(T, kSimpThreads), kSimpThreads, 0, s>>>(faces, T, V, w, fs, faces_out);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

}  // extern "C"
