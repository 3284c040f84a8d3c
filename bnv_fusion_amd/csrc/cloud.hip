// Normals for point clouds that come without a pixel grid (LiDAR scans, exported clouds, PLY files): the k nearest
// neighbours of every point among the points themselves (exact, on the index of nn_index.hpp), a plane through them
// (float64 covariance, cyclic Jacobi), and the sign from a known sensor position -- the [N, 6] rows the encoder takes.
// The specification is include/bnv_fusion.h, "Point-cloud normals"; tests/cloud_restatement.py restates it in numpy
// and the kernel matches it bit for bit: every float operation below is written once, in that order, one rounding each
// (-ffp-contract=off).  No float atomic feeds a result and the neighbour order is (d2, index), so the order the index
// build's integer atomics give the points inside a cell changes nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bnv_fusion.h"
#include "bnv_common.hpp"
#include "cell_grid.hpp"
#include "nn_index.hpp"
#include "scan.hpp"
#include "workspace.hpp"

namespace bnv {

// Cell target.  The k nearest neighbours of a surface sample lie in a disc of radius r_k with pi r_k^2 rho = k (rho
// points per area); a cell of edge h holds rho h^2 points.  After ring 1 the visited box reaches at least h beyond the
// query on every side, so the search ends there when r_k <= h, i.e. rho h^2 >= k / pi: with k / 3 points per cell a
// query of a uniformly sampled surface reads ring 0 and ring 1 -- 9 occupied cells, ~3 k candidates -- and stops.
// A smaller cell reads fewer candidates per ring but needs ring 2 (25 columns of cell runs) for most queries.
constexpr double kCellPerK = 1.0 / 3.0;
constexpr int kJacobiSweeps = BNV_CLOUD_JACOBI_SWEEPS;   // cyclic sweeps over (0,1), (0,2), (1,2); fixed, so the result is one expression
constexpr double kPlaneRatio = 1e-6;    // a plane needs lambda_mid > kPlaneRatio * lambda_max (width / length > 1e-3)
constexpr int32_t kEmpty = INT32_MAX;   // index of an unused list entry: above every point index

struct CloudWs {
  NnIndex ix;
};

static size_t cloud_ws_layout(int64_t n, char* base, CloudWs* w) {
  const int64_t n_bins = nn_bins(n), tiles = nn_scan_tiles(n);
  Carver c(base);
  CloudWs t;
  t.ix.P = c.take<NnParams>(2);
  t.ix.ref_count = c.take<uint32_t>(n_bins);
  t.ix.ref_start = c.take<uint32_t>(n_bins);
  t.ix.ref_cell = c.take<uint32_t>(n);
  t.ix.ref_slot = c.take<uint32_t>(n);
  t.ix.ref_sorted = c.take<float4>(n);
  t.ix.rc_count = c.take<uint32_t>(n_bins);
  t.ix.rc_start = c.take<uint32_t>(n_bins);
  t.ix.rc_cell = c.take<uint32_t>(n);
  t.ix.rc_slot = c.take<uint32_t>(n);
  t.ix.rc_sorted = c.take<float4>(n);
  t.ix.scan_state = c.take<uint64_t>(tiles * 2);
  if (w) *w = t;
  return c.bytes();
}

struct CloudArgs {
  const float* points;          // [n, 3]
  int64_t n;
  int32_t k, min_neighbors;
  float r2;                     // fp32 max_radius^2, +inf without a radius
  const float* origins;         // [n_origins, 3]
  int64_t n_origins;
  const int32_t* origin_index;  // [n] or null: origin 0
  float* out;                   // [n, 6]
  float* variation;             // [n] or null
  int32_t* n_neighbors;         // [n] or null
  int32_t* status;              // [0] rejected rows, [1] bad origin indices
};

__device__ __forceinline__ bool origin_ok(const CloudArgs& a, int64_t i, int32_t& o) {
  o = a.origin_index ? a.origin_index[i] : 0;
  return o >= 0 && (int64_t)o < a.n_origins;
}

__device__ __forceinline__ void write_rejected(const CloudArgs& a, int64_t i, int32_t m) {
  const float nan = __builtin_nanf("");
#pragma unroll
  for (int c = 0; c < 6; ++c) a.out[i * 6 + c] = nan;
  if (a.variation) a.variation[i] = nan;
  if (a.n_neighbors) a.n_neighbors[i] = m;
}

// one integer atomic per wave
__device__ __forceinline__ void count_lanes(bool flag, int32_t* counter) {
  const unsigned long long mask = __ballot(flag);
  if (mask != 0ull && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)mask) - 1)) atomicAdd(counter, __popcll(mask));
}

// Rows the index does not hold (a NaN / Inf coordinate): neither queries nor neighbours.  Every row's origin index is
// checked here, so a bad one is counted once whether the row is finite or not.
__global__ __launch_bounds__(256) void k_cloud_rows(CloudArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool nonfinite = false, bad = false;
  if (i < a.n) {
    int32_t o;
    bad = !origin_ok(a, i, o);
    nonfinite = !finite3(a.points[i * 3], a.points[i * 3 + 1], a.points[i * 3 + 2]);
    if (nonfinite) write_rejected(a, i, 0);
  }
  count_lanes(nonfinite, a.status);
  count_lanes(bad, a.status + 1);
}

// ---- the k best of a query: a sorted list in registers --------------------------------------------------------------
// K is a compile-time size and every loop over the list is fully unrolled, so d[] and i[] are 2 K VGPRs; an index
// that depends on data would send them to scratch.
template <int K>
struct KBest {
  float d[K];
  int32_t i[K];
};

// (d2, index) lexicographic: the lowest index wins a tie
__device__ __forceinline__ bool kb_less(float d, int32_t i, float ld, int32_t li) { return d < ld || (d == ld && i < li); }

// compare-and-swap insertion: the candidate takes the first slot it beats and pushes the rest down one slot
template <int K>
__device__ __forceinline__ void kb_insert(KBest<K>& b, float d, int32_t i) {
  if (!kb_less(d, i, b.d[K - 1], b.i[K - 1])) return;
#pragma unroll
  for (int s = 0; s < K; ++s) {
    const bool lt = kb_less(d, i, b.d[s], b.i[s]);
    const float td = b.d[s];
    const int32_t ti = b.i[s];
    b.d[s] = lt ? d : td;
    b.i[s] = lt ? i : ti;
    d = lt ? td : d;
    i = lt ? ti : i;
  }
}

// Ring search of one query on one grid from ring 0 up to ring `rmax`, or until the stop test proves the first k list
// entries final (-> true): nn_can_stop with the k-th best in place of the best (+inf while fewer than k are known: not
// full, continue), capped by the radius, beyond which nothing counts.
template <int K>
__device__ __forceinline__ bool cloud_rings(const NnParams& P, const uint32_t* __restrict__ rstart,
                                            const float4* __restrict__ Rs, const float4 qv, const double q[3], int rmax,
                                            int k, float r2, KBest<K>& b) {
  const int c[3] = {cell_axis(qv.x, P.lo[0], P.inv_h, P.dims[0]), cell_axis(qv.y, P.lo[1], P.inv_h, P.dims[1]),
                    cell_axis(qv.z, P.lo[2], P.inv_h, P.dims[2])};
  for (int r = 0; r <= rmax; ++r) {
    grid_ring(c, r, P.dims, rstart, [&](uint32_t k0, uint32_t k1) {
      for (uint32_t e = k0; e < k1; ++e) {
        const float4 rv = Rs[e];
        const float d2 = nn_d2(qv.x, qv.y, qv.z, rv);
        if (d2 <= r2) kb_insert(b, d2, __builtin_bit_cast(int32_t, rv.w));
      }
    });
    float kth = INFINITY;
#pragma unroll
    for (int s = 0; s < K; ++s) kth = s == k - 1 ? b.d[s] : kth;
    if (nn_can_stop(P, c, r, q, fminf(kth, r2))) return true;
  }
  return false;
}

// ---- the plane fit ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ double pick3(int i, double a, double b, double c) { return i == 0 ? a : (i == 1 ? b : c); }

// One Jacobi rotation that zeroes a_pq; r is the third index.  Skipped when a_pq is exactly zero.
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq,
                                              double& v0p, double& v0q, double& v1p, double& v1q, double& v2p,
                                              double& v2q) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0);
  const double s = t * c;
  const double h = t * apq;
  app = app - h;
  aqq = aqq + h;
  apq = 0.0;
  const double rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
  double p, q;
  p = v0p, q = v0q, v0p = c * p - s * q, v0q = s * p + c * q;
  p = v1p, q = v1q, v1p = c * p - s * q, v1q = s * p + c * q;
  p = v2p, q = v2q, v2p = c * p - s * q, v2q = s * p + c * q;
}

template <int K>
__device__ __forceinline__ void cloud_fit(const CloudArgs& a, const float4 qv, int32_t qi, const KBest<K>& b) {
  int32_t m = 0;
#pragma unroll
  for (int s = 0; s < K; ++s) m += (s < a.k && b.i[s] != kEmpty) ? 1 : 0;
  int32_t o;
  const bool o_ok = origin_ok(a, qi, o);
  bool rejected = m < a.min_neighbors || !o_ok;
  if (!rejected) {
    const double dm = (double)m;
    // mean: the ordered sum / m
    double sx = 0.0, sy = 0.0, sz = 0.0;
#pragma unroll
    for (int s = 0; s < K; ++s)
      if (s < m) {
        const float* p = a.points + (int64_t)b.i[s] * 3;
        sx += (double)p[0];
        sy += (double)p[1];
        sz += (double)p[2];
      }
    const double mx = sx / dm, my = sy / dm, mz = sz / dm;
    // centred second moments: ordered sums / m
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0;
#pragma unroll
    for (int s = 0; s < K; ++s)
      if (s < m) {
        const float* p = a.points + (int64_t)b.i[s] * 3;
        const double dx = (double)p[0] - mx, dy = (double)p[1] - my, dz = (double)p[2] - mz;
        a00 += dx * dx;
        a01 += dx * dy;
        a02 += dx * dz;
        a11 += dy * dy;
        a12 += dy * dz;
        a22 += dz * dz;
      }
    a00 = a00 / dm, a01 = a01 / dm, a02 = a02 / dm, a11 = a11 / dm, a12 = a12 / dm, a22 = a22 / dm;
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
      jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);   // (0, 1), r = 2
      jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);   // (0, 2), r = 1
      jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);   // (1, 2), r = 0
    }
    // smallest: the first index among equals; largest: the last index among equals; the third is the middle one
    int i0 = 0;
    if (a11 < pick3(i0, a00, a11, a22)) i0 = 1;
    if (a22 < pick3(i0, a00, a11, a22)) i0 = 2;
    int i2 = 2;
    if (a11 > pick3(i2, a00, a11, a22)) i2 = 1;
    if (a00 > pick3(i2, a00, a11, a22)) i2 = 0;
    const int i1 = 3 - i0 - i2;
    const double l0 = pick3(i0, a00, a11, a22), l1 = pick3(i1, a00, a11, a22), l2 = pick3(i2, a00, a11, a22);
    rejected = !(l1 > kPlaneRatio * l2);
    if (!rejected) {
      double n0 = pick3(i0, v00, v01, v02), n1 = pick3(i0, v10, v11, v12), n2 = pick3(i0, v20, v21, v22);
      // away from the sensor, as the depth front end's normals point
      const float* og = a.origins + (int64_t)o * 3;
      const double dot = (n0 * ((double)qv.x - (double)og[0]) + n1 * ((double)qv.y - (double)og[1])) +
                         n2 * ((double)qv.z - (double)og[2]);
      if (dot < 0.0) n0 = -n0, n1 = -n1, n2 = -n2;
      float* out = a.out + (int64_t)qi * 6;
      out[0] = qv.x, out[1] = qv.y, out[2] = qv.z;
      out[3] = (float)n0, out[4] = (float)n1, out[5] = (float)n2;
      if (a.variation) a.variation[qi] = (float)((l0 < 0.0 ? 0.0 : l0) / ((l0 + l1) + l2));
      if (a.n_neighbors) a.n_neighbors[qi] = m;
    }
  }
  if (rejected) write_rejected(a, qi, m);
  count_lanes(rejected, a.status);
}

// One query per thread, in the fine grid's cell order: the self-join's queries are the cell-ordered reference copy, so
// neighbouring threads walk the same cells and no query sort is needed.  The two-grid scheme is bnv_nn_query's: a
// query the first kFineRings rings of the fine grid do not settle (its k-th neighbour lies many cells away: an
// outlier, a sparse cluster) starts again on the coarse grid, whose search is exact on its own -- from an empty list,
// since a list carried over would meet its own entries a second time.
template <int K>
__global__ __launch_bounds__(256) void k_cloud_normals(CloudArgs a, const NnParams* __restrict__ Pp,
                                                       const float4* __restrict__ Rs, const uint32_t* __restrict__ rstart,
                                                       const float4* __restrict__ Rc, const uint32_t* __restrict__ cstart) {
  const int64_t item = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n_finite = Pp[0].n_cells > 0 ? (int64_t)rstart[Pp[0].n_cells] : 0;
  if (item >= n_finite) return;   // (whole waves leave together except in the last one; count_lanes masks the rest)
  const float4 qv = Rs[item];
  const int32_t qi = __builtin_bit_cast(int32_t, qv.w);
  const double q[3] = {(double)qv.x, (double)qv.y, (double)qv.z};
  KBest<K> b;
#pragma unroll
  for (int s = 0; s < K; ++s) b.d[s] = INFINITY, b.i[s] = kEmpty;
  if (!cloud_rings<K>(Pp[0], rstart, Rs, qv, q, kFineRings, a.k, a.r2, b)) {
#pragma unroll
    for (int s = 0; s < K; ++s) b.d[s] = INFINITY, b.i[s] = kEmpty;
    const NnParams& G = Pp[1];
    cloud_rings<K>(G, cstart, Rc, qv, q, max(G.dims[0], max(G.dims[1], G.dims[2])), a.k, a.r2, b);
  }
  cloud_fit<K>(a, qv, qi, b);
}

}  // namespace bnv

using namespace bnv;

extern "C" {

int bnv_cloud_normals_bytes(int64_t n_points, int64_t* bytes) {
  if (!bytes || n_points <= 0 || n_points > INT32_MAX - 2) return BNV_ERR_INVALID_ARGUMENT;
  *bytes = (int64_t)cloud_ws_layout(n_points, nullptr, nullptr);
  return BNV_OK;
}

int bnv_cloud_normals(const float* points, int64_t n_points, int32_t k, float max_radius, int32_t min_neighbors,
                      const float* origins, int64_t n_origins, const int32_t* origin_index, void* workspace,
                      int64_t ws_bytes, float* input_pts_out, float* variation_out, int32_t* n_neighbors_out,
                      int32_t* status_out, bnv_stream_t stream) {
  if (!points || !origins || !workspace || !input_pts_out || !status_out) return BNV_ERR_INVALID_ARGUMENT;
  if (n_points <= 0 || n_points > INT32_MAX - 2 || n_origins <= 0 || n_origins > INT32_MAX)
    return BNV_ERR_INVALID_ARGUMENT;
  if (k < BNV_CLOUD_MIN_K || k > BNV_CLOUD_MAX_K || min_neighbors < 3 || min_neighbors > k)
    return BNV_ERR_INVALID_ARGUMENT;
  if (!(max_radius >= 0.0f) || !(max_radius <= 3.4028234663852886e38f)) return BNV_ERR_INVALID_ARGUMENT;
  CloudWs w;
  if (ws_bytes < (int64_t)cloud_ws_layout(n_points, (char*)workspace, &w)) return BNV_ERR_WORKSPACE_TOO_SMALL;
  hipStream_t s = (hipStream_t)stream;
  CloudArgs a;
  a.points = points;
  a.n = n_points;
  a.k = k;
  a.min_neighbors = min_neighbors;
  a.r2 = max_radius > 0.0f ? max_radius * max_radius : INFINITY;   // one fp32 product; an overflow means no radius
  a.origins = origins;
  a.n_origins = n_origins;
  a.origin_index = origin_index;
  a.out = input_pts_out;
  a.variation = variation_out;
  a.n_neighbors = n_neighbors_out;
  a.status = status_out;
  BNV_HIP_CHECK(hipMemsetAsync(status_out, 0, 4 * sizeof(int32_t), s));
  if (const int e = nn_build_index(points, n_points, w.ix, kCellPerK * (double)k, s)) return e;
  const dim3 blocks(blocks_for(n_points, 256));
  hipLaunchKernelGGL(k_cloud_rows, blocks, dim3(256), 0, s, a);
  BNV_LAUNCH_CHECK();
  const NnIndex& x = w.ix;
  if (k <= 8)
    hipLaunchKernelGGL(k_cloud_normals<8>, blocks, dim3(256), 0, s, a, x.P, x.ref_sorted, x.ref_start, x.rc_sorted,
                       x.rc_start);
  else if (k <= 16)
    hipLaunchKernelGGL(k_cloud_normals<16>, blocks, dim3(256), 0, s, a, x.P, x.ref_sorted, x.ref_start, x.rc_sorted,
                       x.rc_start);
  else
    hipLaunchKernelGGL(k_cloud_normals<32>, blocks, dim3(256), 0, s, a, x.P, x.ref_sorted, x.ref_start, x.rc_sorted,
                       x.rc_start);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

}  // extern "C"
