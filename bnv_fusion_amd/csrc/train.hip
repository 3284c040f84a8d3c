// Training of the local shape embedding (point encoder + SDF decoder) on gfx950: the reference's
// LitFusionPointNet.training_step with training_global=False (local_point_fusion.py:381-460), in exact fp32.
//
// One step is a fixed sequence of launches on the caller's stream, no host synchronisation:
//   encoder forward (train-mode BatchNorm: batch statistics, running-stat update) -> per-patch mean -> decoder input
//   -> decoder forward -> loss -> decoder backward -> d feats -> encoder backward -> Adam.
// Every GEMM is one tiled VALU kernel (fmaf, k ascending).  Every sum over rows -- dW, db, BatchNorm statistics,
// d feats -- is formed as per-workgroup partials over fixed row chunks, then a second pass adds the partials in
// chunk order.  No float atomics: a run is bit-reproducible for a given shape.
//
// Parameters live in one flat fp32 buffer in state_dict order (bnv_fusion.h); running statistics in a second one.
#include <math.h>

#include "bnv_common.hpp"
#include "train_common.hpp"
#include "workspace.hpp"

namespace bnv {
namespace train {

constexpr int kNin = 6, kC = 128, kDin = 17, kH = 256;
constexpr float kBnEps = 1e-5f, kBnMomentum = 0.1f;

// ---- flat parameter layout (state_dict order, running stats and num_batches_tracked excluded) ----
struct Layout {
  int64_t conv_w[4], conv_b[4], bn_w[4], bn_b[4], geo_w[4], geo_b[4], alpha_w, alpha_b, total;
};
static Layout make_layout() {
  Layout L;
  int64_t o = 0;
  const int cin[4] = {kNin, kC, kC, kC}, cout[4] = {kC, kC, kC, kF};
  for (int l = 0; l < 4; ++l) {
    L.conv_w[l] = o; o += (int64_t)cout[l] * cin[l];
    L.conv_b[l] = o; o += cout[l];
  }
  for (int l = 0; l < 4; ++l) {
    L.bn_w[l] = o; o += cout[l];
    L.bn_b[l] = o; o += cout[l];
  }
  const int din[4] = {kDin, kH, kH, kH};
  for (int l = 0; l < 4; ++l) {
    L.geo_w[l] = o; o += (int64_t)kH * din[l];
    L.geo_b[l] = o; o += kH;
  }
  L.alpha_w = o; o += kH;
  L.alpha_b = o; o += 1;
  L.total = o;
  return L;
}
// running stats: per BN layer l, running_mean [C_l] then running_var [C_l]
static int64_t running_off(int l) { return (int64_t)2 * kC * (l < 3 ? l : 3); }
constexpr int64_t kRunningFloats = 2 * (3 * kC + kF);

// ---- the GEMM: C(m, n) = sum_k A(m, k) B(k, n) over strided operands ----
constexpr int TM = 64, TN = 64, TK = 16, kGemmThreads = 256;
struct GemmArgs {
  const float* A; int64_t sam, sak;
  const float* B; int64_t sbk, sbn;
  float* C; int64_t ldc;
  int64_t M, N, K, kchunk;   // gridDim.z = ceil(K / kchunk); z > 1: partials at C + z * M * ldc, plain sums
  const float* bias;         // [N] or null (single-chunk launches only)
  const float* mask; int64_t ldmask;   // out *= (mask(m, n) > 0), or null
  int relu;
};

__global__ void __launch_bounds__(kGemmThreads) k_gemm(GemmArgs g) {
  __shared__ float As[TK][TM];
  __shared__ float Bs[TK][TN];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int64_t m0 = (int64_t)blockIdx.x * TM, n0 = (int64_t)blockIdx.y * TN;
  const int64_t k_begin = (int64_t)blockIdx.z * g.kchunk;
  const int64_t k_end = k_begin + g.kchunk < g.K ? k_begin + g.kchunk : g.K;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
  const bool a_k_fast = g.sak == 1, b_n_fast = g.sbn == 1;
  for (int64_t k0 = k_begin; k0 < k_end; k0 += TK) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + i * kGemmThreads;
      const int mm = a_k_fast ? e / TK : e % TM, kk = a_k_fast ? e % TK : e / TM;
      const int64_t m = m0 + mm, k = k0 + kk;
      As[kk][mm] = (m < g.M && k < k_end) ? g.A[m * g.sam + k * g.sak] : 0.0f;
      const int nn = b_n_fast ? e % TN : e / TK, kb = b_n_fast ? e / TN : e % TK;
      const int64_t n = n0 + nn, kq = k0 + kb;
      Bs[kb][nn] = (n < g.N && kq < k_end) ? g.B[kq * g.sbk + n * g.sbn] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < TK; ++kk) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(&As[kk][ty * 4]);
      const f32x4 b = *reinterpret_cast<const f32x4*>(&Bs[kk][tx * 4]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_fmaf(a[i], b[j], acc[i][j]);
    }
    __syncthreads();
  }
  float* C = g.C + (int64_t)blockIdx.z * g.M * g.ldc;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t m = m0 + ty * 4 + i;
    if (m >= g.M) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t n = n0 + tx * 4 + j;
      if (n >= g.N) continue;
      float v = acc[i][j];
      if (g.bias) v = v + g.bias[n];
      if (g.relu) v = relu_bits(v);
      if (g.mask && !(g.mask[m * g.ldmask + n] > 0.0f)) v = 0.0f;
      C[m * g.ldc + n] = v;
    }
  }
}

// Column partials of X [R, C] (row stride ldx) over row chunk blockIdx.x:
//   mode 0: sum x;  mode 1: sum (x - mean[c])^2;  mode 2: sum dy (P) and sum dy * xhat (P2), X = dy, Y = xhat.
__global__ void k_col_partials(const float* __restrict__ X, const float* __restrict__ Y, int64_t R, int C,
                               int64_t ldx, int64_t rows, const float* __restrict__ mean, int mode,
                               float* __restrict__ P, float* __restrict__ P2) {
  const int64_t r0 = (int64_t)blockIdx.x * rows;
  const int64_t r1 = r0 + rows < R ? r0 + rows : R;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float s = 0.0f, s2 = 0.0f;
    const float mu = mode == 1 ? mean[c] : 0.0f;
    for (int64_t r = r0; r < r1; ++r) {
      const float x = X[r * ldx + c];
      if (mode == 1) {
        const float d = x - mu;
        s += d * d;
      } else {
        s += x;
        if (mode == 2) s2 += x * Y[r * ldx + c];
      }
    }
    P[(int64_t)blockIdx.x * C + c] = s;
    if (mode == 2) P2[(int64_t)blockIdx.x * C + c] = s2;
  }
}

// BatchNorm statistics: phase 0 turns the column sums into the mean; phase 1 the centred sums into the biased
// variance, rstd = 1 / sqrt(var + eps), and (update) the running stats with the unbiased variance.  eval: mean and
// rstd from the running stats.
__global__ void k_bn_stats(int phase, int eval, int update, int C, int64_t R, float* __restrict__ mean,
                           float* __restrict__ rstd, float* __restrict__ run_mean, float* __restrict__ run_var) {
  const int c = threadIdx.x;
  if (c >= C) return;
  if (eval) {
    mean[c] = run_mean[c];
    rstd[c] = 1.0f / sqrtf(run_var[c] + kBnEps);
    return;
  }
  const float r = (float)R;
  if (phase == 0) {
    mean[c] = mean[c] / r;      // mean[] holds the column sum on entry
    return;
  }
  const float var = rstd[c] / r;   // rstd[] holds the centred sum of squares on entry
  const float mu = mean[c];
  rstd[c] = 1.0f / sqrtf(var + kBnEps);
  if (update) {
    const float unbiased = var * (r / (r - 1.0f));   // R >= 2 (shape_ok)
    run_mean[c] = (1.0f - kBnMomentum) * run_mean[c] + kBnMomentum * mu;
    run_var[c] = (1.0f - kBnMomentum) * run_var[c] + kBnMomentum * unbiased;
  }
}

// xhat = (z - mean) * rstd in place; y = gamma * xhat + beta; out = relu(y) (relu) or y
__global__ void k_bn_apply(float* __restrict__ Z, int64_t R, int C, const float* __restrict__ mean,
                           const float* __restrict__ rstd, const float* __restrict__ gamma,
                           const float* __restrict__ beta, int relu, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= R * C) return;
  const int c = (int)(i % C);
  const float xh = (Z[i] - mean[c]) * rstd[c];
  Z[i] = xh;
  const float y = gamma[c] * xh + beta[c];
  out[i] = relu ? relu_bits(y) : y;
}

// encoder input rows: X0[b * n + j] = input_pts[b, j, :6]
__global__ void k_gather_input(const float* __restrict__ pts, int64_t B, int n, float* __restrict__ X0) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * n * kNin) return;
  const int64_t r = i / kNin, b = r / n;
  const int j = (int)(r % n), c = (int)(i % kNin);
  X0[i] = pts[(b * kMaxN + j) * kNin + c];
}

// decoder input rows [xyz, sin xyz, cos xyz, feat] (modules.py:923-971, one encoding frequency)
__global__ void k_decoder_input(const float* __restrict__ xyz, const float* __restrict__ feats, int64_t B, int64_t M,
                                float* __restrict__ D0) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= B * M) return;
  const int64_t b = r / M;
  float* d = D0 + r * kDin;
  for (int a = 0; a < 3; ++a) {
    const float x = xyz[r * 3 + a];
    d[a] = x;
    d[3 + a] = sinf(x);
    d[6 + a] = cosf(x);
  }
  for (int c = 0; c < kF; ++c) d[9 + c] = feats[b * kF + c];
}

// Loss (one workgroup, fixed reduction order): l1 = mean |pred - gt|, reg = mean_b |feats_b|_2,
// loss = {w_l1 l1 + w_reg reg, l1, reg}; dpred = w_l1 sign(pred - gt) / (B M) (train: with_grad)
__global__ void __launch_bounds__(kLossThreads) k_loss(const float* __restrict__ pred, const float* __restrict__ gt,
                                                       int64_t R, const float* __restrict__ feats, int64_t B,
                                                       int with_grad, float* __restrict__ dpred,
                                                       float* __restrict__ loss) {
  __shared__ float s1[kLossThreads], s2[kLossThreads];
  const int t = threadIdx.x;
  const float g = kW_L1 / (float)R;
  float a = 0.0f;
  for (int64_t r = t; r < R; r += kLossThreads) {
    const float d = pred[r] - gt[r];
    a += fabsf(d);
    if (with_grad) dpred[r] = d > 0.0f ? g : (d < 0.0f ? -g : 0.0f);
  }
  s1[t] = a;
  s2[t] = loss_feat_norms(feats, B, t);
  __syncthreads();
  loss_tree_sums(s1, s2, t);
  if (t == 0) {
    const float l1 = s1[0] / (float)R, reg = s2[0] / (float)B;
    loss[0] = with_grad ? kW_L1 * l1 + kW_Reg * reg : l1;
    loss[1] = l1;
    loss[2] = reg;
  }
}

// d feats[b, c] = sum over patch b's M rows of dfrows [B * M, 8] + w_reg / B * feats_b / |feats_b| (0 at |feats_b| = 0)
__global__ void k_dfeats(const float* __restrict__ dfrows, const float* __restrict__ feats, int64_t B, int64_t M,
                         float* __restrict__ dfeats) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * kF) return;
  const int64_t b = i / kF;
  const float s = dfrows_patch_sum(dfrows, b, M, (int)(i % kF));
  const float nrm = feat_norm(feats, b);
  const float reg = nrm > 0.0f ? (kW_Reg / (float)B) * (feats[i] / nrm) : 0.0f;
  dfeats[i] = s + reg;
}

// d y4 [B * n, 8] = d feats / n (backward of the per-patch mean)
__global__ void k_mean_backward(const float* __restrict__ dfeats, int64_t B, int n, float* __restrict__ dy) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * n * kF) return;
  const int64_t b = i / ((int64_t)n * kF);
  dy[i] = dfeats[b * kF + (int)(i % kF)] / (float)n;
}

// train-mode BatchNorm backward: dz = (dy - sum_dy / R - xhat * sum_dyxh / R) * (rstd * gamma)
__global__ void k_bn_backward(const float* __restrict__ dy, const float* __restrict__ xh, int64_t R, int C,
                              const float* __restrict__ sum_dy, const float* __restrict__ sum_dyxh,
                              const float* __restrict__ rstd, const float* __restrict__ gamma,
                              float* __restrict__ dz) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= R * C) return;
  const int c = (int)(i % C);
  const float r = (float)R;
  dz[i] = (dy[i] - sum_dy[c] / r - xh[i] * (sum_dyxh[c] / r)) * (rstd[c] * gamma[c]);
}

// Adam (train_common.hpp: adam_update) with the host's step size and bias correction
__global__ void k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                       float* __restrict__ v, int64_t P, float beta1, float beta2, float eps, float step_size,
                       float bc2_sqrt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  adam_update(p, g, m, v, i, beta1, beta2, eps, step_size, bc2_sqrt);
}

// ---- host side ----
constexpr int64_t kMaxSplits = 64;
constexpr int64_t kMinChunkRows = 256;
constexpr int64_t kColChunkRows = 128;   // rows per workgroup of the column sums

// row chunks of a reduction over R rows: a multiple of TK, at most kMaxSplits chunks
static int64_t chunk_rows(int64_t R) {
  int64_t c = cdiv(R, kMaxSplits);
  if (c < kMinChunkRows) c = kMinChunkRows;
  return cdiv(c, TK) * TK;
}

struct Ws {
  float *X0, *Z[4], *A[3], *Y4, *stats, *feats, *D0, *Hd[4], *pred, *dpred, *dH[2], *dfrows, *dfeats, *dE[2], *part,
      *loss_tmp;
  size_t bytes;
};
static int64_t partial_floats(int64_t Re, int64_t Rd) {
  const int64_t se = cdiv(Re, chunk_rows(Re)), sd = cdiv(Rd, chunk_rows(Rd));
  int64_t p = sd * kH * kH;
  p = p > se * kC * kC ? p : se * kC * kC;
  p = p > 2 * sd * kH ? p : 2 * sd * kH;   // column partials (two sets for the BatchNorm backward)
  p = p > 2 * se * kC ? p : 2 * se * kC;
  const int64_t ce = cdiv(Re, kColChunkRows), cd = cdiv(Rd, kColChunkRows);
  p = p > 2 * ce * kC ? p : 2 * ce * kC;
  p = p > cd * kH ? p : cd * kH;
  return p;
}
static size_t layout_ws(int64_t B, int n, int64_t M, char* base, Ws* w) {
  const int64_t Re = B * n, Rd = B * M;
  Carver c(base);
  Ws t;
  t.X0 = c.take<float>(Re * kNin);
  for (int l = 0; l < 4; ++l) t.Z[l] = c.take<float>(Re * (l < 3 ? kC : kF));
  for (int l = 0; l < 3; ++l) t.A[l] = c.take<float>(Re * kC);
  t.Y4 = c.take<float>(Re * kF);
  t.stats = c.take<float>(8 * kC);       // per layer: mean [C], rstd [C]
  t.feats = c.take<float>(B * kF);
  t.D0 = c.take<float>(Rd * kDin);
  for (int l = 0; l < 4; ++l) t.Hd[l] = c.take<float>(Rd * kH);
  t.pred = c.take<float>(Rd);
  t.dpred = c.take<float>(Rd);
  t.dH[0] = c.take<float>(Rd * kH);
  t.dH[1] = c.take<float>(Rd * kH);
  t.dfrows = c.take<float>(Rd * kF);
  t.dfeats = c.take<float>(B * kF);
  t.dE[0] = c.take<float>(Re * kC);
  t.dE[1] = c.take<float>(Re * kC);
  t.part = c.take<float>(partial_floats(Re, Rd));
  t.loss_tmp = c.take<float>(4);
  t.bytes = c.bytes();
  if (w) *w = t;
  return c.bytes();
}

static bool shape_ok(int64_t B, int64_t n, int64_t M) {
  return train_shape_ok(B, n, M) && B * n >= 2;   // train-mode BatchNorm: the batch statistics need two rows
}

// C(m, n) over operands A, B (see GemmArgs); a reduction over K is split in row chunks and summed in order
static int gemm(hipStream_t s, const float* A, int64_t sam, int64_t sak, const float* Bm, int64_t sbk, int64_t sbn,
                float* C, int64_t ldc, int64_t M, int64_t N, int64_t K, const float* bias, int relu,
                const float* mask, int64_t ldmask) {
  GemmArgs g{A, sam, sak, Bm, sbk, sbn, C, ldc, M, N, K, K, bias, mask, ldmask, relu};
  dim3 grid((unsigned)cdiv(M, TM), (unsigned)cdiv(N, TN), 1);
  k_gemm<<<grid, kGemmThreads, 0, s>>>(g);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}
// dW [N_out, K_in] = sum_r dZ[r, o] X[r, i], in row chunks summed in order into out
static int gemm_dw(hipStream_t s, const float* dZ, int64_t N_out, const float* X, int64_t K_in, int64_t R,
                   float* part, float* out) {
  const int64_t rows = chunk_rows(R), S = cdiv(R, rows);
  GemmArgs g{dZ, 1, N_out, X, K_in, 1, part, K_in, N_out, K_in, R, rows, nullptr, nullptr, 0, 0};
  dim3 grid((unsigned)cdiv(N_out, TM), (unsigned)cdiv(K_in, TN), (unsigned)S);
  k_gemm<<<grid, kGemmThreads, 0, s>>>(g);
  k_sum_partials<<<blocks_for(N_out * K_in, 256), 256, 0, s>>>(part, S, N_out * K_in, 1.0f, out);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}
// column sums of X [R, C] in row chunks summed in order (mode 0 / 1 of k_col_partials); mode 2: out and out2
static int colsum(hipStream_t s, const float* X, const float* Y, int64_t R, int C, const float* mean, int mode,
                  float* part, float* out, float* out2 = nullptr) {
  const int64_t rows = kColChunkRows, S = cdiv(R, rows);
  float* p2 = part + S * C;
  k_col_partials<<<(unsigned)S, 256, 0, s>>>(X, Y, R, C, C, rows, mean, mode, part, p2);
  k_sum_partials<<<blocks_for(C, 256), 256, 0, s>>>(part, S, C, 1.0f, out);
  if (mode == 2) k_sum_partials<<<blocks_for(C, 256), 256, 0, s>>>(p2, S, C, 1.0f, out2);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

// forward through encoder and decoder; loss into loss_out; train: batch statistics (+ running update), dpred
static int forward(hipStream_t s, const Layout& L, const float* params, float* running, const float* input_pts,
                   const float* training_pts, const float* gt, int64_t B, int n, int64_t M, int train, Ws& w,
                   float* loss_out) {
  const int64_t Re = B * n, Rd = B * M;
  k_gather_input<<<blocks_for(Re * kNin, 256), 256, 0, s>>>(input_pts, B, n, w.X0);
  const int cin[4] = {kNin, kC, kC, kC}, cout[4] = {kC, kC, kC, kF};
  const float* X = w.X0;
  for (int l = 0; l < 4; ++l) {
    const int C = cout[l];
    float* mean = w.stats + 2 * kC * l;
    float* rstd = mean + kC;
    float* rm = running + running_off(l);
    float* rv = rm + C;
    BNV_TRY(gemm(s, X, cin[l], 1, params + L.conv_w[l], 1, cin[l], w.Z[l], C, Re, C, cin[l], params + L.conv_b[l], 0,
                 nullptr, 0));
    if (train) {
      BNV_TRY(colsum(s, w.Z[l], nullptr, Re, C, nullptr, 0, w.part, mean, nullptr));
      k_bn_stats<<<1, kC, 0, s>>>(0, 0, 0, C, Re, mean, rstd, rm, rv);
      BNV_TRY(colsum(s, w.Z[l], nullptr, Re, C, mean, 1, w.part, rstd, nullptr));
      k_bn_stats<<<1, kC, 0, s>>>(1, 0, 1, C, Re, mean, rstd, rm, rv);
    } else {
      k_bn_stats<<<1, kC, 0, s>>>(0, 1, 0, C, Re, mean, rstd, rm, rv);
    }
    float* out = l < 3 ? w.A[l] : w.Y4;
    k_bn_apply<<<blocks_for(Re * C, 256), 256, 0, s>>>(w.Z[l], Re, C, mean, rstd, params + L.bn_w[l], params + L.bn_b[l],
                                                 l < 3, out);
    X = out;
  }
  k_patch_mean<false><<<blocks_for(B * kF, 256), 256, 0, s>>>(w.Y4, B, n, w.feats);
  k_decoder_input<<<blocks_for(Rd, 256), 256, 0, s>>>(training_pts, w.feats, B, M, w.D0);
  const float* H = w.D0;
  int64_t din = kDin;
  for (int l = 0; l < 4; ++l) {
    BNV_TRY(gemm(s, H, din, 1, params + L.geo_w[l], 1, din, w.Hd[l], kH, Rd, kH, din, params + L.geo_b[l], 1, nullptr,
                 0));
    H = w.Hd[l];
    din = kH;
  }
  BNV_TRY(gemm(s, H, kH, 1, params + L.alpha_w, 1, kH, w.pred, 1, Rd, 1, kH, params + L.alpha_b, 0, nullptr, 0));
  k_loss<<<1, kLossThreads, 0, s>>>(w.pred, gt, Rd, w.feats, B, train, w.dpred, loss_out);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

static int backward(hipStream_t s, const Layout& L, const float* params, float* grads, int64_t B, int n, int64_t M,
                    Ws& w) {
  const int64_t Re = B * n, Rd = B * M;
  // decoder: fc_alpha, then geo_layer3 .. geo_layer0
  BNV_TRY(gemm_dw(s, w.dpred, 1, w.Hd[3], kH, Rd, w.part, grads + L.alpha_w));
  BNV_TRY(colsum(s, w.dpred, nullptr, Rd, 1, nullptr, 0, w.part, grads + L.alpha_b, nullptr));
  BNV_TRY(gemm(s, w.dpred, 1, 1, params + L.alpha_w, kH, 1, w.dH[0], kH, Rd, kH, 1, nullptr, 0, w.Hd[3], kH));
  int cur = 0;
  for (int l = 3; l >= 0; --l) {
    const float* in = l > 0 ? w.Hd[l - 1] : w.D0;
    const int64_t din = l > 0 ? kH : kDin;
    float* dG = w.dH[cur];
    BNV_TRY(gemm_dw(s, dG, kH, in, din, Rd, w.part, grads + L.geo_w[l]));
    BNV_TRY(colsum(s, dG, nullptr, Rd, kH, nullptr, 0, w.part, grads + L.geo_b[l], nullptr));
    if (l > 0) {
      BNV_TRY(gemm(s, dG, kH, 1, params + L.geo_w[l], kH, 1, w.dH[cur ^ 1], kH, Rd, kH, kH, nullptr, 0, w.Hd[l - 1],
                   kH));
      cur ^= 1;
    } else {   // only the 8 feature columns of geo_layer0's input carry a gradient back
      BNV_TRY(gemm(s, dG, kH, 1, params + L.geo_w[0] + 9, kDin, 1, w.dfrows, kF, Rd, kF, kH, nullptr, 0, nullptr, 0));
    }
  }
  k_dfeats<<<blocks_for(B * kF, 256), 256, 0, s>>>(w.dfrows, w.feats, B, M, w.dfeats);
  // encoder: mean, then (BatchNorm, conv) for layers 4 .. 1
  k_mean_backward<<<blocks_for(Re * kF, 256), 256, 0, s>>>(w.dfeats, B, n, w.dE[0]);
  const int cin[4] = {kNin, kC, kC, kC}, cout[4] = {kC, kC, kC, kF};
  cur = 0;
  for (int l = 3; l >= 0; --l) {
    const int C = cout[l];
    const float* rstd = w.stats + 2 * kC * l + kC;
    float* dY = w.dE[cur];
    float* dZ = w.dE[cur ^ 1];
    BNV_TRY(colsum(s, dY, w.Z[l], Re, C, nullptr, 2, w.part, grads + L.bn_b[l], grads + L.bn_w[l]));
    k_bn_backward<<<blocks_for(Re * C, 256), 256, 0, s>>>(dY, w.Z[l], Re, C, grads + L.bn_b[l], grads + L.bn_w[l], rstd,
                                                    params + L.bn_w[l], dZ);
    // conv bias: sum_r dz = (rstd gamma) (sum_dy - R mean_dy - sum_xhat mean_dyxh) = 0 exactly, since the batch mean
    // centres xhat.  Written as the exact 0: summing the rounded dz leaves ~1e-6 of the weight gradient, which Adam
    // would turn into +-lr moves of a bias that does not affect the output.
    BNV_HIP_CHECK(hipMemsetAsync(grads + L.conv_b[l], 0, sizeof(float) * C, s));
    const float* X = l > 0 ? w.A[l - 1] : w.X0;
    BNV_TRY(gemm_dw(s, dZ, C, X, cin[l], Re, w.part, grads + L.conv_w[l]));
    if (l > 0) {   // d A_{l-1} = dZ W, through the ReLU: the next dY lands where dY was
      BNV_TRY(gemm(s, dZ, C, 1, params + L.conv_w[l], cin[l], 1, dY, cin[l], Re, cin[l], C, nullptr, 0, w.A[l - 1],
                   cin[l]));
    }
  }
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

}  // namespace train
}  // namespace bnv

using namespace bnv;
using namespace bnv::train;

extern "C" {

int64_t bnv_train_param_floats(void) { return make_layout().total; }
int64_t bnv_train_running_floats(void) { return kRunningFloats; }

size_t bnv_train_workspace_bytes(int64_t B, int32_t n, int64_t M) {
  if (!shape_ok(B, n, M)) return 0;
  return layout_ws(B, n, M, nullptr, nullptr);
}

int bnv_train_step(float* params, float* grads, float* adam_m, float* adam_v, float* running, const float* input_pts,
                   const float* training_pts, const float* gt, int64_t B, int32_t n, int64_t M, float lr, float beta1,
                   float beta2, float eps, int64_t adam_step, float* loss_out, void* workspace, size_t ws_bytes,
                   bnv_stream_t stream) {
  if (!shape_ok(B, n, M) || adam_step < 1 || !adam_args_ok(lr, beta1, beta2, eps)) return BNV_ERR_INVALID_ARGUMENT;
  if (!params || !grads || !adam_m || !adam_v || !running || !input_pts || !training_pts || !gt || !loss_out)
    return BNV_ERR_INVALID_ARGUMENT;
  Ws w;
  if (!workspace || ws_bytes < layout_ws(B, n, M, (char*)workspace, &w)) return BNV_ERR_WORKSPACE_TOO_SMALL;
  if (g_num_cus <= 0) return BNV_ERR_NOT_INITIALISED;
  hipStream_t s = (hipStream_t)stream;
  const Layout L = make_layout();
  BNV_TRY(forward(s, L, params, running, input_pts, training_pts, gt, B, n, M, 1, w, loss_out));
  BNV_TRY(backward(s, L, params, grads, B, n, M, w));
  float step_size, bc2_sqrt;   // formed on the host
  adam_bias_corrections(lr, beta1, beta2, adam_step, &step_size, &bc2_sqrt);
  k_adam<<<blocks_for(L.total, 256), 256, 0, s>>>(params, grads, adam_m, adam_v, L.total, beta1, beta2, eps, step_size,
                                                  bc2_sqrt);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

int bnv_train_eval_loss(const float* params, const float* running, const float* input_pts, const float* training_pts,
                        const float* gt, int64_t B, int32_t n, int64_t M, float* loss_out, void* workspace,
                        size_t ws_bytes, bnv_stream_t stream) {
  if (!shape_ok(B, n, M)) return BNV_ERR_INVALID_ARGUMENT;
  if (!params || !running || !input_pts || !training_pts || !gt || !loss_out) return BNV_ERR_INVALID_ARGUMENT;
  Ws w;
  if (!workspace || ws_bytes < layout_ws(B, n, M, (char*)workspace, &w)) return BNV_ERR_WORKSPACE_TOO_SMALL;
  if (g_num_cus <= 0) return BNV_ERR_NOT_INITIALISED;
  return forward((hipStream_t)stream, make_layout(), params, const_cast<float*>(running), input_pts, training_pts, gt,
                 B, n, M, 0, w, loss_out);
}

}  // extern "C"
