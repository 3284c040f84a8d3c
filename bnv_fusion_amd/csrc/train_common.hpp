// What the two embedding trainers share (train.hip: the fp32 Conv / BatchNorm / Linear networks; train_tcnn.hip: the
// tiny-cuda-nn networks): the constants of the reference's step, Adam, the ordered row sums around the per-patch
// feature, the tail of the loss reduction and the argument checks.
//
// This is the only place these are written.  A trainer brings what differs on purpose: its networks, what it feeds the
// loss reduction and writes to loss[0], the scaling of d feats, and where the bias corrections are formed (fp32: on
// the host; tcnn: on the device, after the step count advanced).  Every sum below runs in one fixed order.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace bnv {
namespace {

constexpr int kMaxN = 64, kF = 8;                   // input points per patch at most; feature width
constexpr float kW_L1 = 1.0f, kW_Reg = 0.001f;      // fusion_pointnet_model.yaml:36-38
constexpr int kLossThreads = 1024;                  // the one workgroup of a loss kernel

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- argument checks of the entry points ----
// (the fp32 trainer adds B n >= 2: its batch statistics need two rows)
inline bool train_shape_ok(int64_t B, int64_t n, int64_t M) {
  return B >= 1 && n >= 1 && n <= kMaxN && M >= 1 && B <= (1LL << 24) && M <= (1LL << 24) && B * M <= (1LL << 24);
}
inline bool adam_args_ok(float lr, float beta1, float beta2, float eps) {
  return lr >= 0.0f && beta1 >= 0.0f && beta1 < 1.0f && beta2 >= 0.0f && beta2 < 1.0f && eps >= 0.0f;
}

// ---- Adam, torch's single-tensor form ----
// m.lerp_(g, 1 - b1); v = v b2 + (1 - b2) g g; p -= step_size m / (sqrt(v) / bc2_sqrt + eps)
__device__ __forceinline__ void adam_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                            float* __restrict__ v, int64_t i, float beta1, float beta2, float eps,
                                            float step_size, float bc2_sqrt) {
  const float gi = g[i];
  const float mi = m[i] + (1.0f - beta1) * (gi - m[i]);
  const float vi = v[i] * beta2 + (1.0f - beta2) * (gi * gi);
  m[i] = mi;
  v[i] = vi;
  const float denom = sqrtf(vi) / bc2_sqrt + eps;
  p[i] = p[i] + (-step_size) * (mi / denom);
}
// step_size = lr / (1 - beta1^step) and bc2_sqrt = sqrt(1 - beta2^step) in double, like torch's python-float
// step_size / bias_correction2 ** 0.5.  Host and device pow need not agree in the last place: a trainer calls this on
// one side and stays there.
__host__ __device__ inline void adam_bias_corrections(float lr, float beta1, float beta2, int64_t step,
                                                      float* step_size, float* bc2_sqrt) {
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  *step_size = (float)((double)lr / bc1);
  *bc2_sqrt = (float)sqrt(bc2);
}

// ---- ordered sums ----
// out[i] = scale * sum over s ascending of P[s * count + i]   (scale 1: the plain sum, bit for bit)
__global__ void k_sum_partials(const float* __restrict__ P, int64_t S, int64_t count, float scale,
                               float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  float s = 0.0f;
  for (int64_t z = 0; z < S; ++z) s += P[z * count + i];
  out[i] = s * scale;
}

// feats[b, c] = mean over the n rows of patch b of Y [B * n, 8], summed in row order; ROUND_F16: rounded to f16
template <bool ROUND_F16>
__global__ void k_patch_mean(const float* __restrict__ Y, int64_t B, int n, float* __restrict__ feats) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * kF) return;
  const int64_t b = i / kF;
  const int c = (int)(i % kF);
  float s = 0.0f;
  for (int j = 0; j < n; ++j) s += Y[(b * n + j) * kF + c];
  const float mean = s / (float)n;
  feats[i] = ROUND_F16 ? (float)(_Float16)mean : mean;
}

// |feats_b|_2: the eight squares summed k ascending
__device__ __forceinline__ float feat_norm(const float* __restrict__ feats, int64_t b) {
  float ss = 0.0f;
  for (int k = 0; k < kF; ++k) ss += feats[b * kF + k] * feats[b * kF + k];
  return sqrtf(ss);
}
// column c of dfrows [B * M, 8] summed over patch b's M rows, m ascending
__device__ __forceinline__ float dfrows_patch_sum(const float* __restrict__ dfrows, int64_t b, int64_t M, int c) {
  float s = 0.0f;
  for (int64_t m = 0; m < M; ++m) s += dfrows[(b * M + m) * kF + c];
  return s;
}

// ---- the tail of a loss kernel (one workgroup of kLossThreads) ----
// thread t's share of sum_b |feats_b|_2: patches t, t + kLossThreads, ...
__device__ __forceinline__ float loss_feat_norms(const float* __restrict__ feats, int64_t B, int t) {
  float q = 0.0f;
  for (int64_t b = t; b < B; b += kLossThreads) q += feat_norm(feats, b);
  return q;
}
// s1[0], s2[0] = the tree sums of the two LDS arrays.  On entry every thread has stored its s1[t] and s2[t] and the
// workgroup has passed a barrier; on return a barrier has been passed, too.
__device__ __forceinline__ void loss_tree_sums(float* s1, float* s2, int t) {
  for (int w = kLossThreads / 2; w > 0; w >>= 1) {
    if (t < w) {
      s1[t] += s1[t + w];
      s2[t] += s2[t + w];
    }
    __syncthreads();
  }
}

}  // namespace
}  // namespace bnv
