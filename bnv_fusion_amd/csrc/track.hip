// Frame-to-model tracking: projective point-to-plane ICP of a depth frame against a rendered view of the map
// (depth + world normals, as bnv_render_depth / bnv_tsdf_render_depth / bnv_mesh_render_depth write them).
// Semantics: include/bnv_fusion.h, "Tracking"; restated in float64 numpy by tests/track_restatement.py.
//
// Every iteration is two launches on the caller's stream and nothing is read by the host in between:
//   k_icp_accumulate  a fixed grid of kBlocks x 256 threads; thread g takes the level's sampled pixels g, g + G, ...
//                     in that order into 29 float64 registers (upper triangle of J^T J, J^T r, sum r^2, pairs), then
//                     icp_block_reduce: one partial row per block.  No float atomics: the same inputs give the same bits.
//   k_icp_solve       (icp_solve.hpp, shared with odometry.hip) sums the partial rows, decides the status, solves and
//                     applies exp(xi^) to the pose in device memory.
// The pose, the status word and the outputs live in device memory; a status other than BNV_ICP_OK is sticky: every
// later launch of the call reads it first and returns.  float64 throughout, one rounding per operation
// (-ffp-contract=off).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/bnv_fusion.h"
#include "bnv_common.hpp"
#include "icp_solve.hpp"

namespace bnv {
namespace {

struct IcpFrame {   // what does not change over the call
  const void* depth;
  int dtype;        // 0: uint16 millimetres, 1: float32 metres (frontend.hpp: depth_at)
  int H, W;
  double fx, fy, cx, cy, max_depth;
  const float* model_depth;
  const float* model_normals;
  int Hm, Wm;
  double fxm, fym, cxm, cym;
  double Tm[12];    // rows 0..2 of the model view's camera-to-world pose
  double Tmi[12];   // rows 0..2 of its inverse
  double dist2;     // dist * dist
};

__device__ __forceinline__ double frame_depth(const IcpFrame& f, int64_t i) {
  return f.dtype == 0 ? (double)((const uint16_t*)f.depth)[i] / 1000.0 : (double)((const float*)f.depth)[i];
}

// One frame pixel at pose T (rows of [R | t]): J[6] and r of its pair, or false.
__device__ __forceinline__ bool icp_pair(const IcpFrame& f, const double* __restrict__ T, int u, int v, double (&J)[6],
                                         double& r) {
  const double d = frame_depth(f, (int64_t)v * f.W + u);
  if (!(d > 0.0 && d <= f.max_depth)) return false;
  const double x = ((double)u - f.cx) / f.fx, y = ((double)v - f.cy) / f.fy;
  const double pc[3] = {x * d, y * d, d};
  double pw[3], pm[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) pw[a] = ((T[a * 4] * pc[0] + T[a * 4 + 1] * pc[1]) + T[a * 4 + 2] * pc[2]) + T[a * 4 + 3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
    pm[a] = ((f.Tmi[a * 4] * pw[0] + f.Tmi[a * 4 + 1] * pw[1]) + f.Tmi[a * 4 + 2] * pw[2]) + f.Tmi[a * 4 + 3];
  if (!(pm[2] > 0.0)) return false;
  const double um = rint(f.fxm * pm[0] / pm[2] + f.cxm), vm = rint(f.fym * pm[1] / pm[2] + f.cym);
  if (!(um >= 0.0 && um <= (double)(f.Wm - 1) && vm >= 0.0 && vm <= (double)(f.Hm - 1))) return false;   // (NaN too)
  const int64_t at = (int64_t)vm * f.Wm + (int64_t)um;
  const double dm = (double)f.model_depth[at];
  if (!(dm > 0.0)) return false;
  const double n[3] = {(double)f.model_normals[at * 3], (double)f.model_normals[at * 3 + 1],
                       (double)f.model_normals[at * 3 + 2]};
  if (!((n[0] != 0.0 || n[1] != 0.0 || n[2] != 0.0) && isfinite(dm))) return false;
  const double xm = (um - f.cxm) / f.fxm, ym = (vm - f.cym) / f.fym;
  const double qc[3] = {xm * dm, ym * dm, dm};
  double e[3], tq[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double q = ((f.Tm[a * 4] * qc[0] + f.Tm[a * 4 + 1] * qc[1]) + f.Tm[a * 4 + 2] * qc[2]) + f.Tm[a * 4 + 3];
    e[a] = q - pw[a];
    tq[a] = T[a * 4 + 3] - q;
  }
  if (!((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] <= f.dist2)) return false;
  if (!((n[0] * tq[0] + n[1] * tq[1]) + n[2] * tq[2] > 0.0)) return false;
  r = (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2];
  J[0] = pw[1] * n[2] - pw[2] * n[1];
  J[1] = pw[2] * n[0] - pw[0] * n[2];
  J[2] = pw[0] * n[1] - pw[1] * n[0];
  J[3] = n[0];
  J[4] = n[1];
  J[5] = n[2];
  return isfinite(r);
}

__global__ __launch_bounds__(kThreads) void k_icp_accumulate(IcpFrame f, int stride, int Ws, int64_t n_samples,
                                                             const double* __restrict__ pose,
                                                             const int32_t* __restrict__ status,
                                                             double* __restrict__ partials) {
  if (*status != BNV_ICP_OK) return;
  double T[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) T[i] = pose[i];
  double S[kSums];
#pragma unroll
  for (int i = 0; i < kSums; ++i) S[i] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_samples; i += (int64_t)kBlocks * kThreads) {
    const int v = (int)(i / Ws) * stride, u = (int)(i % Ws) * stride;
    double J[6], r;
    if (!icp_pair(f, T, u, v, J, r)) continue;
    icp_add_row(S, J, r);
    S[28] += 1.0;
  }
  icp_block_reduce(S, partials);
}

}  // namespace
}  // namespace bnv

using namespace bnv;

extern "C" {

size_t bnv_icp_workspace_bytes(int32_t n_levels, const int32_t* levels_host) {
  const int64_t n_iter = schedule_iterations(n_levels, levels_host, 1);
  if (n_iter < 0) return 0;
  return icp_workspace_bytes(n_iter);
}

int bnv_icp_align(const void* depth, int depth_dtype, int32_t H, int32_t W, const double K_host[9], double max_depth,
                  const float* model_depth, const float* model_normals, int32_t H_m, int32_t W_m,
                  const double K_m_host[9], const double T_m_host[16], const double T_m_inv_host[16],
                  const double T_guess_host[16], int32_t n_levels, const int32_t* levels_host, double dist,
                  double min_pair_share, double min_spread, void* workspace, size_t ws_bytes, double* pose_out,
                  double* poses_out, double* stats_out, int32_t* status_out, bnv_stream_t stream) {
  if (!depth || !K_host || !model_depth || !model_normals || !K_m_host || !T_m_host || !T_m_inv_host ||
      !T_guess_host || !levels_host || !workspace || !pose_out || !stats_out || !status_out)
    return BNV_ERR_INVALID_ARGUMENT;
  if (depth_dtype != 0 && depth_dtype != 1) return BNV_ERR_INVALID_ARGUMENT;
  if (H < 1 || W < 1 || H_m < 1 || W_m < 1 || H > 32768 || W > 32768 || H_m > 32768 || W_m > 32768)
    return BNV_ERR_INVALID_ARGUMENT;
  const int64_t n_iter = schedule_iterations(n_levels, levels_host, 1);
  if (n_iter < 0) return BNV_ERR_INVALID_ARGUMENT;
  if (!all_finite(K_host, 9) || !all_finite(K_m_host, 9) || !all_finite(T_m_host, 16) ||
      !all_finite(T_m_inv_host, 16) || !all_finite(T_guess_host, 16))
    return BNV_ERR_INVALID_ARGUMENT;
  if (K_host[0] == 0.0 || K_host[4] == 0.0 || K_m_host[0] == 0.0 || K_m_host[4] == 0.0) return BNV_ERR_INVALID_ARGUMENT;
  if (!(max_depth > 0.0) || !(dist > 0.0) || !(min_pair_share >= 0.0) || !(min_spread >= 0.0) ||
      !std::isfinite(max_depth) || !std::isfinite(dist) || !std::isfinite(min_pair_share) || !std::isfinite(min_spread))
    return BNV_ERR_INVALID_ARGUMENT;
  if (ws_bytes < bnv_icp_workspace_bytes(n_levels, levels_host)) return BNV_ERR_WORKSPACE_TOO_SMALL;

  IcpFrame f;
  f.depth = depth;
  f.dtype = depth_dtype;
  f.H = H;
  f.W = W;
  f.fx = K_host[0];
  f.fy = K_host[4];
  f.cx = K_host[2];
  f.cy = K_host[5];
  f.max_depth = max_depth;
  f.model_depth = model_depth;
  f.model_normals = model_normals;
  f.Hm = H_m;
  f.Wm = W_m;
  f.fxm = K_m_host[0];
  f.fym = K_m_host[4];
  f.cxm = K_m_host[2];
  f.cym = K_m_host[5];
  for (int i = 0; i < 12; ++i) {
    f.Tm[i] = T_m_host[i];
    f.Tmi[i] = T_m_inv_host[i];
  }
  f.dist2 = dist * dist;
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
  sol.max_w = BNV_ICP_MAX_ROTATION;
  sol.max_v = BNV_ICP_MAX_TRANSLATION;
  sol.clamp = 0;
  sol.n_iter = (int)n_iter;
  int iter = 0;
  for (int l = 0; l < n_levels; ++l) {
    const int stride = levels_host[l * 2];
    const int Ws = (W + stride - 1) / stride, Hs = (H + stride - 1) / stride;
    const int64_t n_samples = (int64_t)Ws * Hs;
    sol.min_pairs = min_pair_share * (double)n_samples;
    for (int k = 0; k < levels_host[l * 2 + 1]; ++k, ++iter) {
      hipLaunchKernelGGL(k_icp_accumulate, dim3(kBlocks), dim3(kThreads), 0, s, f, stride, Ws, n_samples,
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
