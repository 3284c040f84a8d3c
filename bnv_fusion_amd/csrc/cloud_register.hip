// Cloud-to-cloud registration: point-to-plane ICP of a point cloud against another point cloud with normals, and the
// persistent index of that target.  Semantics: include/bnv_fusion.h, "Cloud registration"; restated in float64 numpy
// by tests/cloud_register_restatement.py.
//
// The kernel that joins what the tree already has: the two-level uniform-grid point index and its 1-NN ring walk
// (nn_index.hpp, the search of bnv_nn_query) and the aligners' 29 float64 sums, their fixed-order reduction and the
// on-device solve (icp_solve.hpp).
//   bnv_cloud_index_build    one workspace = the index: a header, an fp32 copy of the positions (a rejected row all
//                            NaN, which the grid build leaves out: it is nobody's neighbour), the unit normals, and the
//                            NnIndex over the position copy.  No host read; the header is written by a kernel.
//   bnv_cloud_index_nearest  the plain 1-NN query, one thread per query in the order given.
//   k_cloud_reg_accumulate   a fixed grid of kBlocks x 256 threads; thread g takes the level's sampled points g, g + G,
//                            ...: transforms the point (float64, rounded to fp32 once), walks the rings from the gate
//                            as the initial bound -- a point beyond the gate of everything stops after a ring or two
//                            instead of walking the grid --, forms the row with the target's normal and adds it to the
//                            thread's 29 float64 registers; then icp_block_reduce.  No float atomics.
//   k_icp_solve              (icp_solve.hpp) with `clamp`, as csrc/register.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/bnv_fusion.h"
#include "bnv_common.hpp"
#include "cell_grid.hpp"
#include "icp_solve.hpp"
#include "nn_index.hpp"
#include "workspace.hpp"

namespace bnv {
namespace {

constexpr uint64_t kCloudMagic = 0x58444e49444c4342ull;   // "BCLDINDX"
constexpr uint32_t kCloudVersion = 1;                     // of the layout below
constexpr double kMinNormal = 1e-12;                      // a shorter normal has no direction: the row is rejected

struct CloudHeader {
  uint64_t magic;
  int64_t n;
  uint32_t version;
  uint32_t pad;
};

struct CloudIx {
  CloudHeader* H;
  float* pos;   // [n, 3]: the positions, a rejected row all NaN
  float* nrm;   // [n, 3]: unit normals (NaN for a rejected row)
  NnIndex ix;   // over pos
};

// the layout is a function of n alone: the host carves it to build, a kernel re-derives it from the header
__host__ __device__ inline size_t cloud_ix_layout(int64_t n, const void* base, CloudIx* w) {
  const int64_t n_bins = n + 2, tiles = (n_bins + kScanTile - 1) / kScanTile;   // nn_bins, nn_scan_tiles
  Carver c(base);
  CloudIx t;
  t.H = c.take<CloudHeader>(1);
  t.pos = c.take<float>(n * 3);
  t.nrm = c.take<float>(n * 3);
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

// does `bytes` of memory behind H hold an index this code built?  (An index that does not answers nothing.)
__device__ __forceinline__ bool cloud_ix_usable(const CloudHeader& H, int64_t bytes) {
  return H.magic == kCloudMagic && H.version == kCloudVersion && H.n >= 1 && H.n <= INT32_MAX - 2 &&
         (int64_t)cloud_ix_layout(H.n, nullptr, nullptr) <= bytes;
}

// [n, 6] rows -> the position copy and the unit normals; thread 0 writes the header
__global__ __launch_bounds__(256) void k_cloud_index_rows(const float* __restrict__ X, int64_t n, CloudIx w) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    w.H->magic = kCloudMagic;
    w.H->n = n;
    w.H->version = kCloudVersion;
    w.H->pad = 0;
  }
  if (i >= n) return;
  const float x = X[i * 6], y = X[i * 6 + 1], z = X[i * 6 + 2];
  const double nx = (double)X[i * 6 + 3], ny = (double)X[i * 6 + 4], nz = (double)X[i * 6 + 5];
  const double len = sqrt((nx * nx + ny * ny) + nz * nz);
  const bool ok = finite3(x, y, z) && isfinite(len) && len >= kMinNormal;   // (a NaN / Inf normal: len is not finite)
  const float nan = __builtin_nanf("");
  w.pos[i * 3] = ok ? x : nan;
  w.pos[i * 3 + 1] = ok ? y : nan;
  w.pos[i * 3 + 2] = ok ? z : nan;
  w.nrm[i * 3] = ok ? (float)(nx / len) : nan;
  w.nrm[i * 3 + 1] = ok ? (float)(ny / len) : nan;
  w.nrm[i * 3 + 2] = ok ? (float)(nz / len) : nan;
}

// one thread per query, in the order given (bnv_nn_query sorts its queries by cell first; the answers are the same)
__global__ __launch_bounds__(256) void k_cloud_nearest(const char* __restrict__ index, int64_t index_bytes,
                                                       const float* __restrict__ Q, int64_t n_query,
                                                       float* __restrict__ d2_out, int32_t* __restrict__ idx_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_query) return;
  const CloudHeader& H = *(const CloudHeader*)index;
  float best = INFINITY;
  int32_t bi = -1;
  if (cloud_ix_usable(H, index_bytes)) {
    CloudIx W;
    cloud_ix_layout(H.n, index, &W);
    const float4 qv = make_float4(Q[i * 3], Q[i * 3 + 1], Q[i * 3 + 2], 0.0f);
    if (W.ix.P[0].n_cells > 0 && finite3(qv.x, qv.y, qv.z))
      nn_search(W.ix.P, W.ix.ref_sorted, W.ix.ref_start, W.ix.rc_sorted, W.ix.rc_start, qv, best, bi);
  }
  d2_out[i] = best;
  idx_out[i] = bi;
}

struct CregArgs {   // what does not change over the call
  const char* index;   // the target index (only read)
  int64_t index_bytes;
  const float* points;
  const float* normals;   // source normals or null: no normal gate
  int64_t n_points;
  double min_cos;
  int oriented;
  float* q_out;         // the dumps, [n_points ..] or null
  int32_t* index_out;
};

__global__ __launch_bounds__(kThreads) void k_cloud_reg_accumulate(CregArgs f, int64_t stride, int64_t n_samples,
                                                                   float bound, const double* __restrict__ pose,
                                                                   const int32_t* __restrict__ status,
                                                                   double* __restrict__ partials) {
  if (*status != BNV_ICP_OK) return;
  double T[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) T[i] = pose[i];
  const CloudHeader& H = *(const CloudHeader*)f.index;
  CloudIx W = {};
  bool searchable = cloud_ix_usable(H, f.index_bytes);
  if (searchable) {
    cloud_ix_layout(H.n, f.index, &W);
    searchable = W.ix.P[0].n_cells > 0;
  }
  double S[kSums];
#pragma unroll
  for (int i = 0; i < kSums; ++i) S[i] = 0.0;
  for (int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x; k < n_samples; k += (int64_t)kBlocks * kThreads) {
    const int64_t i = k * stride;
    const double p[3] = {(double)f.points[i * 3], (double)f.points[i * 3 + 1], (double)f.points[i * 3 + 2]};
    float qf[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
      qf[a] = (float)(((T[a * 4] * p[0] + T[a * 4 + 1] * p[1]) + T[a * 4 + 2] * p[2]) + T[a * 4 + 3]);
    // the nearest indexed point with d2 < bound = the first float above the gate: d2 <= gate^2, the lowest index
    float best = bound;
    int32_t bi = -1;
    if (searchable && finite3(qf[0], qf[1], qf[2]))
      nn_search(W.ix.P, W.ix.ref_sorted, W.ix.ref_start, W.ix.rc_sorted, W.ix.rc_start,
                make_float4(qf[0], qf[1], qf[2], 0.0f), best, bi);
    if (f.q_out) {
      f.q_out[k * 3] = qf[0];
      f.q_out[k * 3 + 1] = qf[1];
      f.q_out[k * 3 + 2] = qf[2];
    }
    if (f.index_out) f.index_out[k] = bi;
    if (bi < 0) continue;
    const double n[3] = {(double)W.nrm[(int64_t)bi * 3], (double)W.nrm[(int64_t)bi * 3 + 1],
                         (double)W.nrm[(int64_t)bi * 3 + 2]};
    if (f.normals) {
      const float s0 = f.normals[i * 3], s1 = f.normals[i * 3 + 1], s2 = f.normals[i * 3 + 2];
      if (!finite3(s0, s1, s2)) continue;
      const double s[3] = {(double)s0, (double)s1, (double)s2};
      double m[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) m[a] = (T[a * 4] * s[0] + T[a * 4 + 1] * s[1]) + T[a * 4 + 2] * s[2];
      const double c = (m[0] * n[0] + m[1] * n[1]) + m[2] * n[2];
      if (!((f.oriented ? c : fabs(c)) >= f.min_cos)) continue;
    }
    const double q[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
    const double e[3] = {(double)W.pos[(int64_t)bi * 3] - q[0], (double)W.pos[(int64_t)bi * 3 + 1] - q[1],
                         (double)W.pos[(int64_t)bi * 3 + 2] - q[2]};
    S[28] += 1.0;
    const double r = (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2];
    const double J[6] = {q[1] * n[2] - q[2] * n[1], q[2] * n[0] - q[0] * n[2], q[0] * n[1] - q[1] * n[0],
                         n[0], n[1], n[2]};
    icp_add_row(S, J, r);
  }
  icp_block_reduce(S, partials);
}

}  // namespace
}  // namespace bnv

using namespace bnv;

extern "C" {

int bnv_cloud_index_bytes(int64_t n_points, int64_t* bytes) {
  if (!bytes || n_points <= 0 || n_points > INT32_MAX - 2) return BNV_ERR_INVALID_ARGUMENT;
  *bytes = (int64_t)cloud_ix_layout(n_points, nullptr, nullptr);
  return BNV_OK;
}

int bnv_cloud_index_build(const float* input_pts, int64_t n_points, void* workspace, int64_t ws_bytes,
                          bnv_stream_t stream) {
  if (!input_pts || !workspace) return BNV_ERR_INVALID_ARGUMENT;
  if (n_points <= 0 || n_points > INT32_MAX - 2) return BNV_ERR_INVALID_ARGUMENT;
  CloudIx w;
  if (ws_bytes < (int64_t)cloud_ix_layout(n_points, workspace, &w)) return BNV_ERR_WORKSPACE_TOO_SMALL;
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_cloud_index_rows, dim3(blocks_for(n_points, 256)), dim3(256), 0, s, input_pts, n_points, w);
  BNV_LAUNCH_CHECK();
  return nn_build_index(w.pos, n_points, w.ix, kNnCellTarget, s);
}

int bnv_cloud_index_nearest(const void* cloud_index, int64_t index_bytes, const float* query, int64_t n_query,
                            float* d2_out, int32_t* idx_out, bnv_stream_t stream) {
  if (!cloud_index || !query || !d2_out || !idx_out) return BNV_ERR_INVALID_ARGUMENT;
  if (n_query <= 0 || n_query > INT32_MAX) return BNV_ERR_INVALID_ARGUMENT;
  if (index_bytes < (int64_t)cloud_ix_layout(1, nullptr, nullptr)) return BNV_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_cloud_nearest, dim3(blocks_for(n_query, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const char*)cloud_index, index_bytes, query, n_query, d2_out, idx_out);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

size_t bnv_cloud_register_bytes(int32_t n_levels, const int32_t* levels_host) {
  const int64_t n_iter = schedule_iterations(n_levels, levels_host, 1);
  if (n_iter < 0) return 0;
  return icp_workspace_bytes(n_iter);
}

int bnv_cloud_register(const void* cloud_index, int64_t index_bytes, const float* points, int64_t n_points,
                       const float* source_normals, const double T_guess_host[16], int32_t n_levels,
                       const int32_t* levels_host, const double* dist_host, double min_normal_cos, int32_t oriented,
                       double min_pair_share, double min_spread, double max_rotation, double max_translation,
                       void* workspace, size_t ws_bytes, double* pose_out, double* poses_out, double* stats_out,
                       int32_t* status_out, float* q_out, int32_t* index_out, bnv_stream_t stream) {
  if (!cloud_index || !points || !T_guess_host || !levels_host || !dist_host || !workspace || !pose_out ||
      !stats_out || !status_out)
    return BNV_ERR_INVALID_ARGUMENT;
  if (n_points <= 0 || n_points > INT32_MAX) return BNV_ERR_INVALID_ARGUMENT;
  if (index_bytes < (int64_t)cloud_ix_layout(1, nullptr, nullptr)) return BNV_ERR_INVALID_ARGUMENT;
  const int64_t n_iter = schedule_iterations(n_levels, levels_host, 1);
  if (n_iter < 0) return BNV_ERR_INVALID_ARGUMENT;
  for (int l = 0; l < n_levels; ++l)
    if (!(dist_host[l] > 0.0) || !std::isfinite(dist_host[l])) return BNV_ERR_INVALID_ARGUMENT;
  if (!all_finite(T_guess_host, 16)) return BNV_ERR_INVALID_ARGUMENT;
  if (source_normals && !(min_normal_cos >= -1.0 && min_normal_cos <= 1.0)) return BNV_ERR_INVALID_ARGUMENT;
  if (!(min_pair_share >= 0.0) || !(min_spread >= 0.0) || !(max_rotation > 0.0) || !(max_translation > 0.0) ||
      !std::isfinite(min_pair_share) || !std::isfinite(min_spread) || !std::isfinite(max_rotation) ||
      !std::isfinite(max_translation))
    return BNV_ERR_INVALID_ARGUMENT;
  if (ws_bytes < icp_workspace_bytes(n_iter)) return BNV_ERR_WORKSPACE_TOO_SMALL;

  CregArgs f;
  f.index = (const char*)cloud_index;
  f.index_bytes = index_bytes;
  f.points = points;
  f.normals = source_normals;
  f.n_points = n_points;
  f.min_cos = min_normal_cos;
  f.oriented = oriented != 0;
  f.q_out = q_out;
  f.index_out = index_out;
  double* partials = (double*)workspace;
  double* records = partials + (size_t)kBlocks * kSums;
  const hipStream_t s = (hipStream_t)stream;

  IcpInit init;
  for (int i = 0; i < 16; ++i) init.T0[i] = T_guess_host[i];
  init.n_iter = (int)n_iter;
  hipLaunchKernelGGL(k_icp_init, dim3(1), dim3(64), 0, s, init, pose_out, poses_out, stats_out, records, status_out);
  BNV_LAUNCH_CHECK();
  IcpSolve sol;
  for (int i = 0; i < 16; ++i) sol.T0[i] = T_guess_host[i];
  sol.min_spread = min_spread;
  sol.max_w = max_rotation;
  sol.max_v = max_translation;
  sol.clamp = 1;
  sol.n_iter = (int)n_iter;
  int iter = 0;
  for (int l = 0; l < n_levels; ++l) {
    const int64_t stride = levels_host[l * 2];
    const int64_t n_samples = (n_points + stride - 1) / stride;
    // g2 = the gate squared in float64, rounded to fp32 once; the walk starts from the first float above it
    const float bound = nextafterf((float)(dist_host[l] * dist_host[l]), INFINITY);
    sol.min_pairs = min_pair_share * (double)n_samples;
    for (int k = 0; k < levels_host[l * 2 + 1]; ++k, ++iter) {
      hipLaunchKernelGGL(k_cloud_reg_accumulate, dim3(kBlocks), dim3(kThreads), 0, s, f, stride, n_samples, bound,
                         (const double*)pose_out, (const int32_t*)status_out, partials);
      BNV_LAUNCH_CHECK();
      sol.iter = iter;
      hipLaunchKernelGGL(k_icp_solve, dim3(1), dim3(64), 0, s, sol, (const double*)partials, pose_out, poses_out,
                         stats_out, records, status_out);
      BNV_LAUNCH_CHECK();
    }
  }
  return BNV_OK;
}

}  // extern "C"
