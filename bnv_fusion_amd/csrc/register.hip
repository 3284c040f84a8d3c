// Point-to-mesh registration: ICP of a point cloud against a triangle mesh, with no camera in between.
// Semantics: include/bnv_fusion.h, "Registration"; restated in float64 numpy by tests/register_restatement.py.
//
// The kernel that joins the two things the tree already has: the exact closest point of a mesh (meshsdf_query.hpp, the
// search of bnv_mesh_sdf_query over the index bnv_mesh_sdf_build makes) and the aligners' 29 float64 sums, their
// fixed-order reduction and the on-device solve (icp_solve.hpp).  Every iteration is two launches on the caller's
// stream and nothing is read by the host in between:
//   k_reg_accumulate  a fixed grid of kBlocks x 256 threads; thread g takes the level's sampled points g, g + G, ...:
//                     transforms the point (float64, rounded to fp32 once), searches the mesh with it -- one thread per
//                     point, as the query does: cells hold a handful of triangles --, and only when the search has
//                     finished into (q, closest, feature) forms the point-to-plane row and adds it to the thread's 29
//                     float64 registers; then icp_block_reduce.  No float atomics: the same inputs give the same bits.
//   k_icp_solve       (icp_solve.hpp) with `clamp`: a step beyond the limits is scaled onto them, not refused.
// The pose, the status word and the outputs live in device memory; a status other than BNV_ICP_OK is sticky.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/bnv_fusion.h"
#include "bnv_common.hpp"
#include "icp_solve.hpp"
#include "meshsdf.hpp"
#include "meshsdf_query.hpp"

namespace bnv {
namespace {

struct RegCloud {   // what does not change over the call
  char* index;      // the mesh index (only read)
  int64_t index_bytes;
  const float* points;
  int64_t n_points;
  int reject_boundary;
  float* q_out;          // the dumps, [n_points ..] or null
  float* closest_out;
  int32_t* face_out;
  uint8_t* feature_out;
};

// What the search makes of sampled point k (source point k * stride) at pose T: the transformed point qf, the closest
// point c and the feature; false: no candidate (a non-finite q, an unusable index).
__device__ __forceinline__ bool reg_closest(const RegCloud& f, const Header& H, const Ws& W, bool usable,
                                            const double* __restrict__ T, int64_t k, int64_t stride, float (&qf)[3],
                                            float (&c)[3], uint32_t& feature) {
  const int64_t i = k * stride;
  const double p[3] = {(double)f.points[i * 3], (double)f.points[i * 3 + 1], (double)f.points[i * 3 + 2]};
#pragma unroll
  for (int a = 0; a < 3; ++a)
    qf[a] = (float)(((T[a * 4] * p[0] + T[a * 4 + 1] * p[1]) + T[a * 4 + 2] * p[2]) + T[a * 4 + 3]);
  const float nan = __builtin_nanf("");
  int32_t face = -1;
  feature = 0;
  c[0] = c[1] = c[2] = nan;
  bool found = false;
  if (usable && finite3(qf[0], qf[1], qf[2])) {
    const double q[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
    Best best;
    uint32_t tests = 0;
    msdf_search(H, W, qf, q, best, tests);
    if (best.face != INT32_MAX) {
      if (best.code != 0) {
        const int32_t vi0 = __builtin_bit_cast(int32_t, W.tri[(int64_t)best.face * 3].w),
                      vi1 = __builtin_bit_cast(int32_t, W.tri[(int64_t)best.face * 3 + 1].w),
                      vi2 = __builtin_bit_cast(int32_t, W.tri[(int64_t)best.face * 3 + 2].w);
        const long long* acc;
        feature = msdf_feature(W, best, vi0, vi1, vi2, acc);
      }
      face = best.face;
      c[0] = best.c[0];
      c[1] = best.c[1];
      c[2] = best.c[2];
      found = true;
    }
  }
  if (f.q_out) {
    f.q_out[k * 3] = qf[0];
    f.q_out[k * 3 + 1] = qf[1];
    f.q_out[k * 3 + 2] = qf[2];
  }
  if (f.closest_out) {
    f.closest_out[k * 3] = c[0];
    f.closest_out[k * 3 + 1] = c[1];
    f.closest_out[k * 3 + 2] = c[2];
  }
  if (f.face_out) f.face_out[k] = face;
  if (f.feature_out) f.feature_out[k] = (uint8_t)feature;
  return found;
}

__global__ __launch_bounds__(kThreads) void k_reg_accumulate(RegCloud f, int64_t stride, int64_t n_samples, double dist2,
                                                             const double* __restrict__ pose,
                                                             const int32_t* __restrict__ status,
                                                             double* __restrict__ partials) {
  if (*status != BNV_ICP_OK) return;
  double T[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) T[i] = pose[i];
  const Header& H = *(const Header*)f.index;
  const bool usable = msdf_usable(H, f.index_bytes);
  Ws W;
  if (usable) msdf_layout(H.n_vertices, H.n_faces, f.index, &W);
  double S[kSums];
#pragma unroll
  for (int i = 0; i < kSums; ++i) S[i] = 0.0;
  for (int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x; k < n_samples; k += (int64_t)kBlocks * kThreads) {
    float qf[3], c[3];
    uint32_t feature;
    if (!reg_closest(f, H, W, usable, T, k, stride, qf, c, feature)) continue;
    const double q[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
    const double u[3] = {q[0] - (double)c[0], q[1] - (double)c[1], q[2] - (double)c[2]};
    const double d2 = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2];
    const double d = sqrt(d2);
    if (!(d2 <= dist2)) continue;
    if (f.reject_boundary && (feature & 0x10u)) continue;
    S[28] += 1.0;
    if (d == 0.0) continue;   // on the mesh: a pair without a direction
    const double n[3] = {u[0] / d, u[1] / d, u[2] / d};
    const double e[3] = {-u[0], -u[1], -u[2]};
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

size_t bnv_mesh_register_bytes(int32_t n_levels, const int32_t* levels_host) {
  const int64_t n_iter = schedule_iterations(n_levels, levels_host, 1);
  if (n_iter < 0) return 0;
  return icp_workspace_bytes(n_iter);
}

int bnv_mesh_register(const void* mesh_index, int64_t index_bytes, const float* points, int64_t n_points,
                      const double T_guess_host[16], int32_t n_levels, const int32_t* levels_host,
                      const double* dist_host, int32_t reject_boundary, double min_pair_share, double min_spread,
                      double max_rotation, double max_translation, void* workspace, size_t ws_bytes,
                      double* pose_out, double* poses_out, double* stats_out, int32_t* status_out, float* q_out,
                      float* closest_out, int32_t* face_out, uint8_t* feature_out, bnv_stream_t stream) {
  if (!mesh_index || !points || !T_guess_host || !levels_host || !dist_host || !workspace || !pose_out || !stats_out ||
      !status_out)
    return BNV_ERR_INVALID_ARGUMENT;
  if (n_points <= 0 || n_points > INT32_MAX) return BNV_ERR_INVALID_ARGUMENT;
  if (index_bytes < (int64_t)msdf_layout(1, 1, nullptr, nullptr)) return BNV_ERR_INVALID_ARGUMENT;
  const int64_t n_iter = schedule_iterations(n_levels, levels_host, 1);
  if (n_iter < 0) return BNV_ERR_INVALID_ARGUMENT;
  for (int l = 0; l < n_levels; ++l)
    if (!(dist_host[l] > 0.0) || !std::isfinite(dist_host[l])) return BNV_ERR_INVALID_ARGUMENT;
  if (!all_finite(T_guess_host, 16)) return BNV_ERR_INVALID_ARGUMENT;
  if (!(min_pair_share >= 0.0) || !(min_spread >= 0.0) || !(max_rotation > 0.0) || !(max_translation > 0.0) ||
      !std::isfinite(min_pair_share) || !std::isfinite(min_spread) || !std::isfinite(max_rotation) ||
      !std::isfinite(max_translation))
    return BNV_ERR_INVALID_ARGUMENT;
  if (ws_bytes < icp_workspace_bytes(n_iter)) return BNV_ERR_WORKSPACE_TOO_SMALL;

  RegCloud f;
  f.index = (char*)mesh_index;
  f.index_bytes = index_bytes;
  f.points = points;
  f.n_points = n_points;
  f.reject_boundary = reject_boundary != 0;
  f.q_out = q_out;
  f.closest_out = closest_out;
  f.face_out = face_out;
  f.feature_out = feature_out;
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
    const double dist2 = dist_host[l] * dist_host[l];
    sol.min_pairs = min_pair_share * (double)n_samples;
    for (int k = 0; k < levels_host[l * 2 + 1]; ++k, ++iter) {
      hipLaunchKernelGGL(k_reg_accumulate, dim3(kBlocks), dim3(kThreads), 0, s, f, stride, n_samples, dist2,
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
