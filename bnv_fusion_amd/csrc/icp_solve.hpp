// What the three aligners share (track.hip: frame-to-model ICP; odometry.hip: frame-to-frame RGB-D odometry;
// register.hip: point-to-mesh registration): the 29 float64 sums of an iteration, their reduction inside a block, and
// the launches around them.
//   k_icp_init        writes the guess, the status word and the zeroed outputs.
//   icp_block_reduce  a thread's 29 sums -> one partial row per block: a fixed __shfl_down tree per wave, LDS across the
//                     block's four waves in wave order.
//   k_icp_solve       one wave: sums the partial rows in ascending block order, decides the status, solves the 6 x 6
//                     system by LDL^T, applies exp(xi^) to the pose in device memory.  A step beyond IcpSolve's
//                     limits is refused (the trackers) or, with `clamp`, scaled onto them (registration).
// Semantics: include/bnv_fusion.h, "Tracking" (Sums, Solve); restated in float64 numpy by tests/track_restatement.py.
// float64 throughout, one rounding per operation (-ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/bnv_fusion.h"

namespace bnv {
namespace {

constexpr int kBlocks = BNV_ICP_BLOCKS;
constexpr int kThreads = 256;
constexpr int kSums = BNV_ICP_SUMS;              // 21 + 6 + 1 + 1
constexpr int kRecord = BNV_ICP_RECORD_DOUBLES;  // per iteration: the 29 sums, xi[6], one pad
constexpr int kMaxLevels = BNV_ICP_MAX_LEVELS;
constexpr int kMaxIters = 4096;                  // over all levels

struct IcpInit {
  double T0[16];
  int n_iter;
};

struct IcpSolve {
  double T0[16];
  double min_pairs;   // min_pair_share * (sampled pixels of the level)
  double min_spread;
  double max_w, max_v;   // limits of one step: radians, metres
  int clamp;             // 0: a step beyond the limits is BNV_ICP_JUMP; 1: it is scaled onto them (register.hip)
  int iter, n_iter;
};

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

// adds one row J[6], r to a thread's sums (pairs, S[28], is the caller's: a pixel may add more than one row)
__device__ __forceinline__ void icp_add_row(double (&S)[kSums], const double (&J)[6], const double r) {
  int k = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = a; b < 6; ++b) S[k++] += J[a] * J[b];
#pragma unroll
  for (int a = 0; a < 6; ++a) S[21 + a] += J[a] * r;
  S[27] += r * r;
}

// the block's kThreads x 29 sums -> partials[blockIdx.x]; every thread of the block calls it
__device__ __forceinline__ void icp_block_reduce(const double (&S)[kSums], double* __restrict__ partials) {
  __shared__ double lds[kThreads / 64][kSums];
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
      if (a.clamp) {
        // a step beyond the limits is scaled onto them, all six components by one factor; the norms are those of the
        // step that is applied.  Only a non-finite step is refused.
        if (!(isfinite(wn) && isfinite(vn))) {
          code = BNV_ICP_JUMP;
        } else {
          const double s = fmin(1.0, fmin(a.max_w / wn, a.max_v / vn));
          if (s < 1.0) {
#pragma unroll
            for (int i = 0; i < 6; ++i) xi[i] = xi[i] * s;
            wn = sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]);
            vn = sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5]);
          }
        }
      } else if (!(wn <= a.max_w && vn <= a.max_v)) {
        code = BNV_ICP_JUMP;   // (NaN too)
      }
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

// total iterations of a schedule [(first, iterations)], first >= min_first, or -1 when it is not one
inline int64_t schedule_iterations(int32_t n_levels, const int32_t* levels, int32_t min_first) {
  if (!levels || n_levels < 1 || n_levels > kMaxLevels) return -1;
  int64_t n = 0;
  for (int l = 0; l < n_levels; ++l) {
    if (levels[l * 2] < min_first || levels[l * 2 + 1] < 0) return -1;
    n += levels[l * 2 + 1];
  }
  return n >= 1 && n <= kMaxIters ? n : -1;
}

// the workspace both aligners use (packed, not carved: the records follow the partial rows directly, as
// include/bnv_fusion.h documents them)
inline size_t icp_workspace_bytes(int64_t n_iter) {
  return ((size_t)kBlocks * kSums + (size_t)n_iter * kRecord) * sizeof(double);
}

}  // namespace
}  // namespace bnv
