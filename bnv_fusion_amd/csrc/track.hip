// Frame-to-model tracking: projective point-to-plane ICP of a depth frame against a rendered view of the map
// (depth + world normals, as bnv_render_depth / bnv_tsdf_render_depth / bnv_mesh_render_depth write them).
// Semantics: include/bnv_fusion.h, "Tracking"; restated in float64 numpy by tests/track_restatement.py.
//
// Every iteration is two launches on the caller's stream and nothing is read by the host in between:
//   k_icp_accumulate  a fixed grid of kBlocks x 256 threads; thread g takes the level's sampled pixels g, g + G, ...
//                     in that order into 29 float64 registers (upper triangle of J^T J, J^T r, sum r^2, pairs), a
//                     fixed __shfl_down tree per wave, LDS across the block's four waves in wave order, one partial
//                     row per block.  No float atomics: the same inputs give the same bits.
//   k_icp_solve       one wave: sums the partial rows in ascending block order, decides the status, solves the 6 x 6
//                     system by LDL^T, applies exp(xi^) to the pose in device memory.
// The pose, the status word and the outputs live in device memory; a status other than BNV_ICP_OK is sticky: every
// later launch of the call reads it first and returns.  float64 throughout, one rounding per operation
// (-ffp-contract=off).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/bnv_fusion.h"
#include "bnv_common.hpp"

namespace bnv {
namespace {

constexpr int kBlocks = BNV_ICP_BLOCKS;
constexpr int kThreads = 256;
constexpr int kSums = BNV_ICP_SUMS;              // 21 + 6 + 1 + 1
constexpr int kRecord = BNV_ICP_RECORD_DOUBLES;  // per iteration: the 29 sums, xi[6], one pad
constexpr int kMaxLevels = BNV_ICP_MAX_LEVELS;
constexpr int kMaxIters = 4096;                  // over all levels

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

struct IcpInit {
  double T0[16];
  int n_iter;
};

struct IcpSolve {
  double T0[16];
  double min_pairs;   // min_pair_share * (sampled pixels of the level)
  double min_spread;
  int iter, n_iter;
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

__global__ __launch_bounds__(64) void k_icp_init(IcpInit a, double* __restrict__ pose, double* __restrict__ poses,
                                                 double* __restrict__ stats, double* __restrict__ records,
                                                 int32_t* __restrict__ status) {
  const int t = threadIdx.x;
  if (t < 16) pose[t] = a.T0[t];
  if (t == 0) *status = BNV_ICP_OK;
  if (poses)
    for (int i = t; i < (a.n_iter + 1) * 16; i += 64) poses[i] = a.T0[i & 15];
  for (int i = t; i < a.n_iter * 5; i += 64) stats[i] = 0.0;
  for (int i = t; i < a.n_iter * kRecord; i += 64) records[i] = 0.0;
}

__global__ __launch_bounds__(kThreads) void k_icp_accumulate(IcpFrame f, int stride, int Ws, int64_t n_samples,
                                                             const double* __restrict__ pose,
                                                             const int32_t* __restrict__ status,
                                                             double* __restrict__ partials) {
  if (*status != BNV_ICP_OK) return;
  __shared__ double lds[kThreads / 64][kSums];
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
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = a; b < 6; ++b) S[k++] += J[a] * J[b];
#pragma unroll
    for (int a = 0; a < 6; ++a) S[21 + a] += J[a] * r;
    S[27] += r * r;
    S[28] += 1.0;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < kSums; ++i) {
    double s = S[i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) lds[wave][i] = s;
  }
  __syncthreads();
  if (threadIdx.x < kSums) {
    double s = lds[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) s += lds[w][threadIdx.x];
    partials[(int64_t)blockIdx.x * kSums + threadIdx.x] = s;
  }
}

// smallest eigenvalue of the symmetric 3 x 3 matrix M: six sweeps of cyclic Jacobi over (0,1), (0,2), (1,2).
// Every loop of the solve has constant bounds and is unrolled: the matrices stay in registers.
__device__ __forceinline__ void jacobi_rotate(double (&M)[3][3], const int p, const int q) {
  const double apq = M[p][q];
  if (apq == 0.0) return;
  const double theta = (M[q][q] - M[p][p]) / (2.0 * apq);
  const double tt = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double t = theta < 0.0 ? -tt : tt;
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
  for (int k = 0; k < 3; ++k) {   // M <- M G
    const double mkp = M[k][p], mkq = M[k][q];
    M[k][p] = c * mkp - s * mkq;
    M[k][q] = s * mkp + c * mkq;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {   // M <- G^T M
    const double mpk = M[p][k], mqk = M[q][k];
    M[p][k] = c * mpk - s * mqk;
    M[q][k] = s * mpk + c * mqk;
  }
}

__device__ __forceinline__ double min_eig3(double (&M)[3][3]) {
#pragma unroll 1
  for (int sweep = 0; sweep < 6; ++sweep) {
    jacobi_rotate(M, 0, 1);
    jacobi_rotate(M, 0, 2);
    jacobi_rotate(M, 1, 2);
  }
  return fmin(fmin(M[0][0], M[1][1]), M[2][2]);
}

__global__ __launch_bounds__(64) void k_icp_solve(IcpSolve a, const double* __restrict__ partials,
                                                  double* __restrict__ pose, double* __restrict__ poses,
                                                  double* __restrict__ stats, double* __restrict__ records,
                                                  int32_t* __restrict__ status) {
  if (*status != BNV_ICP_OK) return;
  __shared__ double sums[kSums];
  if (threadIdx.x < kSums) {
    double s = partials[threadIdx.x];
#pragma unroll 16   // sixteen loads in flight; the adds stay in block order
    for (int b = 1; b < kBlocks; ++b) s += partials[b * kSums + threadIdx.x];
    sums[threadIdx.x] = s;
    records[(int64_t)a.iter * kRecord + threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double A[6][6], b[6], T[16];
  {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) A[i][j] = A[j][i] = sums[k++];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) b[i] = sums[21 + i];
#pragma unroll
  for (int i = 0; i < 16; ++i) T[i] = pose[i];
  const double rr = sums[27], pairs = sums[28];
  double* st = stats + (int64_t)a.iter * 5;
  double* xi_out = records + (int64_t)a.iter * kRecord + kSums;
  if (poses)
#pragma unroll
    for (int i = 0; i < 16; ++i) poses[(int64_t)a.iter * 16 + i] = T[i];
  int code = BNV_ICP_OK;
  double spread = 0.0, wn = 0.0, vn = 0.0, xi[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const double rmse = pairs > 0.0 ? sqrt(rr / pairs) : 0.0;
  if (!(pairs > 0.0) || pairs < a.min_pairs) code = BNV_ICP_LOST;
  if (code == BNV_ICP_OK) {
    double M[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) M[i][j] = A[3 + i][3 + j] / pairs;
    spread = min_eig3(M);
    if (!(spread >= a.min_spread)) code = BNV_ICP_DEGENERATE;
  }
  if (code == BNV_ICP_OK) {
    // LDL^T without pivoting, column by column; L is unit lower triangular.  A pivot <= 0 is remembered and the
    // (meaningless) rest still computed: no branch depends on data inside the unrolled loops.
    double L[6][6], D[6];
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double dj = A[j][j];
#pragma unroll
      for (int k = 0; k < j; ++k) dj = dj - (L[j][k] * L[j][k]) * D[k];
      bad = bad || !(dj > 0.0);
      D[j] = dj;
#pragma unroll
      for (int i = j + 1; i < 6; ++i) {
        double l = A[i][j];
#pragma unroll
        for (int k = 0; k < j; ++k) l = l - (L[i][k] * L[j][k]) * D[k];
        L[i][j] = l / dj;
      }
    }
    if (bad) code = BNV_ICP_DEGENERATE;
    if (code == BNV_ICP_OK) {
      double z[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) {      // L z = b
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s = s - L[i][k] * z[k];
        z[i] = s;
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) z[i] = z[i] / D[i];
#pragma unroll
      for (int i = 5; i >= 0; --i) {     // L^T xi = z
        double s = z[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * xi[k];
        xi[i] = s;
      }
      wn = sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]);
      vn = sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5]);
      if (!(wn <= BNV_ICP_MAX_ROTATION && vn <= BNV_ICP_MAX_TRANSLATION)) code = BNV_ICP_JUMP;   // (NaN too)
    }
  }
  st[0] = pairs;
  st[1] = rmse;
  st[2] = wn;
  st[3] = vn;
  st[4] = spread;
#pragma unroll
  for (int i = 0; i < 6; ++i) xi_out[i] = xi[i];
  if (code != BNV_ICP_OK) {
    *status = code;
#pragma unroll
    for (int i = 0; i < 16; ++i) pose[i] = a.T0[i];
    return;
  }
  // exp(xi^): R = I + A K + B K^2, V = I + B K + C K^2 with K = [w]x
  const double th2 = (xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2];
  double ca, cb, cc;
  if (wn < 1e-8) {
    ca = 1.0 - th2 / 6.0;
    cb = 0.5 - th2 / 24.0;
    cc = 1.0 / 6.0 - th2 / 120.0;
  } else {
    const double sn = sin(wn), cs = cos(wn);
    ca = sn / wn;
    cb = (1.0 - cs) / th2;
    cc = (wn - sn) / (th2 * wn);
  }
  const double K[3][3] = {{0.0, -xi[2], xi[1]}, {xi[2], 0.0, -xi[0]}, {-xi[1], xi[0], 0.0}};
  double K2[3][3], E[3][3], V[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) K2[i][j] = (K[i][0] * K[0][j] + K[i][1] * K[1][j]) + K[i][2] * K[2][j];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double id = i == j ? 1.0 : 0.0;
      E[i][j] = (id + ca * K[i][j]) + cb * K2[i][j];
      V[i][j] = (id + cb * K[i][j]) + cc * K2[i][j];
    }
  double Tn[16];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) Tn[i * 4 + j] = (E[i][0] * T[j] + E[i][1] * T[4 + j]) + E[i][2] * T[8 + j];
    const double tv = (V[i][0] * xi[3] + V[i][1] * xi[4]) + V[i][2] * xi[5];
    Tn[i * 4 + 3] = ((E[i][0] * T[3] + E[i][1] * T[7]) + E[i][2] * T[11]) + tv;
  }
  Tn[12] = Tn[13] = Tn[14] = 0.0;
  Tn[15] = 1.0;
#pragma unroll
  for (int i = 0; i < 16; ++i) pose[i] = Tn[i];
  if (poses && a.iter + 1 == a.n_iter)
#pragma unroll
    for (int i = 0; i < 16; ++i) poses[(int64_t)a.n_iter * 16 + i] = Tn[i];
}

// total iterations of a schedule, or -1 when it is not one
int64_t schedule_iterations(int32_t n_levels, const int32_t* levels) {
  if (!levels || n_levels < 1 || n_levels > kMaxLevels) return -1;
  int64_t n = 0;
  for (int l = 0; l < n_levels; ++l) {
    if (levels[l * 2] < 1 || levels[l * 2 + 1] < 0) return -1;
    n += levels[l * 2 + 1];
  }
  return n >= 1 && n <= kMaxIters ? n : -1;
}

}  // namespace
}  // namespace bnv

using namespace bnv;

extern "C" {

size_t bnv_icp_workspace_bytes(int32_t n_levels, const int32_t* levels_host) {
  const int64_t n_iter = schedule_iterations(n_levels, levels_host);
  if (n_iter < 0) return 0;
  // (packed, not carved: the records follow the partial rows directly, as include/bnv_fusion.h documents them)
  return ((size_t)kBlocks * kSums + (size_t)n_iter * kRecord) * sizeof(double);
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
  const int64_t n_iter = schedule_iterations(n_levels, levels_host);
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
