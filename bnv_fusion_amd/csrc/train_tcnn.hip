// Training of the tiny-cuda-nn local shape embedding on gfx950: the reference's default networks
// (tcnnPointNetEncoder, pointnet_utils.py:269-294; tcnnNeRFModel, modules.py:136-285; tiny_cuda: True in
// fusion_pointnet_model.yaml) under LitFusionPointNet.training_step with training_global=False
// (local_point_fusion.py:381-460).
//
// Networks: FullyFusedMLP, 64 wide, 3 hidden layers, ReLU, no bias, one flat fp32 master vector each, row-major
// [out, in] matrices in layer order:  encoder 16 | 64 | 64 | 64 | 16 (10,240 weights), decoder 32 | 64 | 64 | 64 | 16
// (11,264).  The input is padded with 1.0 to 16 / 32 columns (the pad columns act as biases).
//
// Forward = the mode-2 arithmetic of the inference kernels (encode_tcnn.hip k_pointnet_scatter_tb, sdf_mlp.hpp
// sdf_mlp_tile_t), from the same code (tcnn_mlp.hpp): inputs and weights rounded to f16, every layer an f16 MFMA with
// fp32 accumulation, ReLU after the hidden layers, every layer output rounded to f16.
//
// Backward: every f16 rounding counts as the identity (straight-through).  The activations and weights are exact
// f16 values; the incoming gradient of each layer is split into hi + lo f16 parts (hi = rn16(g), lo = rn16(g - hi)),
// so each product dX = W^T dZ and dW = sum_rows dZ X runs as two f16 MFMAs with fp32 accumulation: near fp32 (the
// split keeps ~22 significant bits; a lo part below 2^-14 loses bits as an f16 subnormal, at most 2^-25 absolute).
// Declared end-to-end precision: every gradient within 5e-3 of its tensor's largest |gradient| of the float64
// restatement, the f16 forward's rounding decisions included (a value one ulp off flips sign(pred - gt) or a ReLU
// downstream; the fp32 restatement flips at other places).  To keep the parts out of the subnormal range the decoder back-propagates sign(pred - gt) and the
// encoder (dfeat / n) B n, both of order 1; the weight gradients are scaled by 1 / (B M) and 1 / (B n) at the end.
//
// One step is a fixed chain of launches on the caller's stream, with no allocation, synchronisation or host read:
//   k_tcnn_pack (f16 MFMA fragment images of W and W^T, both networks)
//   -> k_tcnn_tile<enc, fwd> (point outputs) -> k_patch_mean<f16> (feats, f16)
//   -> k_tcnn_tile<dec, train> (forward, |pred - gt| per tile, backward to the input; activation and gradient
//      images for the weight gradients) -> k_tcnn_dw + k_sum_partials (decoder dW)
//   -> k_tcnn_dfeats (d feats: sum over M, + the reg term)
//   -> k_tcnn_tile<enc, train> (forward RECOMPUTED, backward) -> k_tcnn_dw + k_sum_partials (encoder dW)
//   -> k_tcnn_loss (loss terms, finite check, device-side Adam step count) -> k_tcnn_adam.
// k_patch_mean, k_sum_partials, Adam's update and the tail of the loss reduction are the fp32 trainer's, too
// (train_common.hpp).
// One wave runs all layers of a 32-row tile with the activations in registers (32x32x16 f16 MFMA; the layer output
// tile feeds the next MFMA as its B operand with no data movement, tcnn_mlp.hpp).  Weight fragments
// are read from the f16 images in global memory (45 KB per network, cache-resident), as the inference decoder does.
// Every sum over rows -- weight gradients (per-chunk partials summed in chunk order), patch means, d feats over M,
// the loss -- runs in a fixed order with no float atomics: a run is bit-reproducible for a given shape.
//
// A step whose loss or any gradient is not finite (an f16 overflow in the forward) leaves params, moments and the
// step count untouched and reports loss_out[3] = 1, like the reference's AMP gradient scaler skipping the step.
#include <math.h>

#include "bnv_common.hpp"
#include "train_common.hpp"
#include "workspace.hpp"
#include "tcnn_mlp.hpp"

namespace bnv {
namespace train_tcnn {

constexpr int kW = 64;
constexpr int64_t kEncParams = 16 * 64 + 64 * 64 * 2 + 64 * 16;   // 10,240
constexpr int64_t kDecParams = 32 * 64 + 64 * 64 * 2 + 64 * 16;   // 11,264
constexpr int64_t kParams = kEncParams + kDecParams;
constexpr int kMaxChunks = 64;                                  // row chunks of the weight-gradient partials

// fragment images (halves): forward = the inference pack (tcnn_mlp.hpp: TcnnPack), transposed the same with the roles
// swapped
__host__ __device__ constexpr int fwd_halves(int nk0) { return 128 * 8 * nk0 + 1280 * 8; }
static_assert(fwd_halves(1) == TcnnPack<1>::TOTAL && fwd_halves(2) == TcnnPack<2>::TOTAL,
              "the forward image is the inference pack");
constexpr int kBwdHalves = 1408 * 8;   // W3^T [2][1] | W2^T [2][4] | W1^T [2][4] | W0^T [1][4]

__device__ __forceinline__ int layer_in(int l, int nin0) { return l == 0 ? nin0 : kW; }
__device__ __forceinline__ int layer_out(int l) { return l == 3 ? 16 : kW; }
__device__ __forceinline__ int64_t layer_poff(int l, int nin0) { return l == 0 ? 0 : (int64_t)kW * nin0 + (l - 1) * kW * kW; }

// Fragment images of both networks from the fp32 masters.  Entry e of a network: forward part, then transposed part.
__global__ void k_tcnn_pack(const float* __restrict__ params, _Float16* __restrict__ img_e,
                            _Float16* __restrict__ img_d) {
  const int64_t e_all = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int tot_e = fwd_halves(1) + kBwdHalves, tot_d = fwd_halves(2) + kBwdHalves;
  if (e_all >= tot_e + tot_d) return;
  const bool dec = e_all >= tot_e;
  int e = (int)(dec ? e_all - tot_e : e_all);
  const int nin0 = dec ? 32 : 16, nk0 = nin0 / 16;
  const float* W = params + (dec ? kEncParams : 0);
  _Float16* out = dec ? img_d : img_e;
  const int idx = e;
  const int fwd = fwd_halves(nk0);
  int l, ng, base;
  bool transposed = e >= fwd;
  if (!transposed) {
    const int s0 = 128 * 8 * nk0;
    if (e < s0) { l = 0; ng = nk0; base = 0; }
    else if (e < s0 + 4096) { l = 1; ng = 4; base = s0; }
    else if (e < s0 + 8192) { l = 2; ng = 4; base = s0 + 4096; }
    else { l = 3; ng = 4; base = s0 + 8192; }
  } else {
    e -= fwd;
    if (e < 1024) { l = 3; ng = 1; base = 0; }
    else if (e < 5120) { l = 2; ng = 4; base = 1024; }
    else if (e < 9216) { l = 1; ng = 4; base = 5120; }
    else { l = 0; ng = 4; base = 9216; }
  }
  const int q = e - base, jj = q & 7, lane = (q >> 3) & 63, rest = q >> 9;
  const int g = rest % ng, mb = rest / ng, r = lane & 31, h = lane >> 5;
  const int I = layer_in(l, nin0), O = layer_out(l);
  // forward: A[o = 32 mb + r][k = 16 g + slot feature];  transposed: A[i = 32 mb + r][k = o = 16 g + slot feature]
  const int o = transposed ? 16 * g + tcnn_slot_feature(jj, h) : 32 * mb + r;
  const int i = transposed ? 32 * mb + r : 16 * g + tcnn_slot_feature(jj, h);
  const float v = (o < O && i < I) ? W[layer_poff(l, nin0) + (int64_t)o * I + i] : 0.0f;
  out[idx] = (_Float16)v;
}

struct TileArgs {
  const _Float16* wf;        // forward fragment image
  const _Float16* wt;        // transposed fragment image
  int64_t R, T;              // rows, 32-row tiles
  const float* input_pts;    // encoder: [B, 64, 6], rows b n + j read from patch b's row j
  int n;
  const float* xyz;          // decoder: [B M, 3]
  const float* feats;        // decoder: [B, 8] (f16 values)
  const float* gt;           // decoder: [B M] or null
  int64_t M;
  float* Y;                  // encoder forward: [R, 8] point outputs (f16 values)
  float* pred;               // decoder: [R] or null
  float* ltile;              // decoder: [T] sum of |pred - gt| over the tile, or null
  float* dfrows;             // decoder train: [R, 8] d input columns 9..16 (unscaled: sign(pred - gt) back-propagated)
  const float* egrad;        // encoder train: [B, 8] (d feats / n) B n
  _Float16* X[4];            // train: layer inputs   [T][I_l][32]
  _Float16* Zh[4];           // train: d layer outputs, hi part [T][O_l][32]
  _Float16* Zl[4];           //                          lo part
};

__device__ __forceinline__ half8 frag(const _Float16* img, int idx8) {
  return *reinterpret_cast<const half8*>(img + (int64_t)idx8 * 8);
}
// The trainer's one departure from the inference tile (tcnn_mlp.hpp: relu_half8, which drops a NaN whose sign bit is
// set): the same bits for every number, but NaN stays NaN, so that a forward that overflowed f16 (inf - inf in the
// next layer) reaches the loss and the step is skipped.
__device__ __forceinline__ half8 relu_half8_keep_nan(const f32x16& v, int base) {
  half8 r;
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = (_Float16)(!(v[base + e] <= 0.0f) ? v[base + e] : 0.0f);
  return r;
}
__device__ __forceinline__ void split_half8(const f32x16& v, int base, half8& hi, half8& lo) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const _Float16 t = (_Float16)v[base + e];
    hi[e] = t;
    lo[e] = (_Float16)(v[base + e] - (float)t);
  }
}
__device__ __forceinline__ void apply_mask(f32x16 (&d)[2], uint32_t m) {
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int r = 0; r < 16; ++r) d[mb][r] = ((m >> (mb * 16 + r)) & 1u) ? d[mb][r] : 0.0f;
}
// image [tile][F][32]: feature 16 g + tcnn_slot_feature(jj, h) of row j
__device__ __forceinline__ void store_frag(_Float16* img, int64_t tile, int F, int g, int j, int h, half8 v) {
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) img[((tile * F) + 16 * g + tcnn_slot_feature(jj, h)) * 32 + j] = v[jj];
}

// NET 0: encoder, 1: decoder.  TRAIN 0: forward (encoder: point outputs; decoder: pred / loss partials), 1: forward
// and backward with the images for the weight gradients.  One wave per 32-row tile, four waves per workgroup.
template <int NET, int TRAIN>
__global__ __launch_bounds__(256) void k_tcnn_tile(TileArgs a) {
  constexpr int NK0 = NET ? 2 : 1, NIN = 16 * NK0;
  const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
  const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= a.T) return;                   // uniform per wave
  const int64_t row = tile * 32 + j;
  const bool valid = row < a.R;
  int64_t b = 0;
  float in[NIN];
#pragma unroll
  for (int f = 0; f < NIN; ++f) in[f] = valid ? 1.0f : 0.0f;   // rows past R: all zero, so they add nothing
  if (valid) {
    if constexpr (NET == 0) {
      b = row / a.n;
      const float* src = a.input_pts + (b * kMaxN + (row - b * a.n)) * 6;
#pragma unroll
      for (int c = 0; c < 6; ++c) in[c] = src[c];
    } else {
      // the encoding NeuralMap's mode-2 decode stages (sdf_mlp.hpp: stage_input_t)
      b = row / a.M;
      const float* p = a.xyz + row * 3;
      const float loc[3] = {p[0], p[1], p[2]};
      float feat[kF];
#pragma unroll
      for (int c = 0; c < kF; ++c) feat[c] = a.feats[b * kF + c];
      tcnn_sdf_inputs(loc, feat, in);
    }
  }
  half8 xin[NK0];
#pragma unroll
  for (int ks = 0; ks < NK0; ++ks) xin[ks] = tcnn_input_frag(in, ks, h);

  // ---- forward: the layers of tcnn_mlp.hpp; between them the ReLU masks and (TRAIN) the layer inputs are kept ----
  typedef TcnnPack<NK0> P;
  f32x16 acc[2];
  tcnn_first_layer<NK0>(a.wf + P::W0, lane, xin, acc);
  if (TRAIN) {
#pragma unroll
    for (int ks = 0; ks < NK0; ++ks) store_frag(a.X[0], tile, NIN, ks, j, h, xin[ks]);
  }
  uint32_t mask[3];
  half8 s[4];
#pragma unroll
  for (int l = 1; l <= 3; ++l) {
    mask[l - 1] = positive_bits32(acc);
#pragma unroll
    for (int g = 0; g < 4; ++g) s[g] = relu_half8_keep_nan(acc[g >> 1], 8 * (g & 1));
    if (TRAIN) {
#pragma unroll
      for (int g = 0; g < 4; ++g) store_frag(a.X[l], tile, kW, g, j, h, s[g]);
    }
    if (l < 3) tcnn_hidden_layer(a.wf + (l == 1 ? P::W1 : P::W2), lane, s, acc);
  }
  const f32x16 o = tcnn_output_layer(a.wf + P::W3, lane, s);
  // output rows 4 h + r (r < 4) and 8 + 4 h + r (r = 4 .. 7) of row j; the networks return f16
  float sg = 0.0f;
  if (NET == 0) {
    if (!TRAIN && valid) {
#pragma unroll
      for (int r = 0; r < 4; ++r) a.Y[row * kF + 4 * h + r] = (float)(_Float16)o[r];
    }
  } else {
    const float pred = (float)(_Float16)o[0];   // output 0 = register 0 of the lanes with h == 0
    float ad = 0.0f;
    if (h == 0 && valid) {
      if (a.pred) a.pred[row] = pred;
      if (a.gt) {
        const float d = pred - a.gt[row];
        ad = fabsf(d);
        sg = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
      }
    }
    if (a.ltile) {
#pragma unroll
      for (int w = 32; w >= 1; w >>= 1) ad += __shfl_xor(ad, w);   // fixed butterfly: same bits every run
      if (lane == 0) a.ltile[tile] = ad;
    }
  }
  if (!TRAIN) return;

  // ---- backward ----
  // d output (16 rows, K-step 0): decoder row 0 = sign(pred - gt); encoder rows 0..7 = egrad of the row's patch
  half8 dh, dl;
  {
    f32x16 t = zero16();
    if (NET == 1) {
      t[0] = h == 0 ? sg : 0.0f;
    } else if (valid) {
#pragma unroll
      for (int r = 0; r < 4; ++r) t[r] = a.egrad[b * kF + 4 * h + r];
    }
    split_half8(t, 0, dh, dl);
    store_frag(a.Zh[3], tile, 16, 0, j, h, dh);
    store_frag(a.Zl[3], tile, 16, 0, j, h, dl);
  }
  constexpr int T2 = 128, T1 = 640, T0 = 1152;   // transposed image offsets, in fragments
  f32x16 d[2];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb) {
    const half8 w = frag(a.wt, mb * 64 + lane);
    d[mb] = mfma_f16(w, dl, zero16());
    d[mb] = mfma_f16(w, dh, d[mb]);
  }
  apply_mask(d, mask[2]);
#pragma unroll
  for (int l = 2; l >= 0; --l) {
    half8 zh[4], zl[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      split_half8(d[g >> 1], 8 * (g & 1), zh[g], zl[g]);
      store_frag(a.Zh[l], tile, kW, g, j, h, zh[g]);
      store_frag(a.Zl[l], tile, kW, g, j, h, zl[g]);
    }
    if (l > 0) {
      const int off = l == 2 ? T2 : T1;
#pragma unroll
      for (int mb = 0; mb < 2; ++mb) {
        d[mb] = zero16();
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const half8 w = frag(a.wt, off + (mb * 4 + g) * 64 + lane);
          d[mb] = mfma_f16(w, zl[g], d[mb]);
          d[mb] = mfma_f16(w, zh[g], d[mb]);
        }
      }
      apply_mask(d, mask[l - 1]);
    } else if (NET == 1) {
      // d input columns 9..16 (the feature): rows (r & 3) + 8 (r >> 2) + 4 h of W0^T dZ0
      f32x16 x = zero16();
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const half8 w = frag(a.wt, T0 + g * 64 + lane);
        x = mfma_f16(w, zl[g], x);
        x = mfma_f16(w, zh[g], x);
      }
      if (valid) {
        float* dst = a.dfrows + row * kF;
        if (h == 0) {
          dst[0] = x[5]; dst[1] = x[6]; dst[2] = x[7]; dst[7] = x[8];
        } else {
          dst[3] = x[4]; dst[4] = x[5]; dst[5] = x[6]; dst[6] = x[7];
        }
      }
    }
  }
}

// egrad[b, c] = (sum over patch b's M rows of dfrows) / M + w_reg feats_b / |feats_b|  (= d feats_b * B; the encoder
// row gradient d feats_b / n scaled by B n)
__global__ void k_tcnn_dfeats(const float* __restrict__ dfrows, const float* __restrict__ feats, int64_t B, int64_t M,
                              float* __restrict__ egrad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * kF) return;
  const int64_t b = i / kF;
  const float s = dfrows_patch_sum(dfrows, b, M, (int)(i % kF));
  const float nrm = feat_norm(feats, b);
  egrad[i] = s / (float)M + (nrm > 0.0f ? kW_Reg * (feats[i] / nrm) : 0.0f);
}

// Weight-gradient partials: one wave per (32 x 32 block of one layer's dW, chunk of tiles).
// dW[o, i] = sum over the chunk's rows of dZ[row, o] X[row, i], as (lo, hi) f16 MFMA pairs in tile order.
struct DwArgs {
  const _Float16* X[4];
  const _Float16* Zh[4];
  const _Float16* Zl[4];
  int I[4], O[4];
  int64_t poff[4];
  int blk_l[12], blk_o[12], blk_i[12];
  int64_t T, tpc;             // tiles, tiles per chunk
  float* part;                // [chunk][P]
  int64_t P;
};
__global__ __launch_bounds__(64) void k_tcnn_dw(DwArgs a) {
  const int blk = blockIdx.x;
  const int64_t chunk = blockIdx.y;
  const int l = a.blk_l[blk], I = a.I[l], O = a.O[l];
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int o = 32 * a.blk_o[blk] + r, i = 32 * a.blk_i[blk] + r;
  const bool ok_o = o < O, ok_i = i < I;
  const _Float16* zh = a.Zh[l];
  const _Float16* zl = a.Zl[l];
  const _Float16* x = a.X[l];
  half8 zero;
#pragma unroll
  for (int e = 0; e < 8; ++e) zero[e] = (_Float16)0.0f;
  f32x16 acc = zero16();
  const int64_t t0 = chunk * a.tpc, t1 = t0 + a.tpc < a.T ? t0 + a.tpc : a.T;
  for (int64_t t = t0; t < t1; ++t) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int64_t ko = 16 * ks + 8 * h;
      const half8 ah = ok_o ? *reinterpret_cast<const half8*>(zh + (t * O + o) * 32 + ko) : zero;
      const half8 al = ok_o ? *reinterpret_cast<const half8*>(zl + (t * O + o) * 32 + ko) : zero;
      const half8 bx = ok_i ? *reinterpret_cast<const half8*>(x + (t * I + i) * 32 + ko) : zero;
      acc = mfma_f16(al, bx, acc);
      acc = mfma_f16(ah, bx, acc);
    }
  }
  float* dst = a.part + chunk * a.P + a.poff[l];
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int oo = 32 * a.blk_o[blk] + (reg & 3) + 8 * (reg >> 2) + 4 * h;
    if (oo < O && ok_i) dst[(int64_t)oo * I + i] = acc[reg];
  }
}

// Loss (one workgroup, fixed order): l1 = sum of the tile partials / (B M), reg = mean_b |feats_b|;
// loss_out = {l1 + w_reg reg, l1, reg} (+ [3] = skipped, train).  Train: a non-finite loss or gradient marks the step
// skipped; otherwise the device step count advances and Adam's step size and bias correction are formed for it.
__global__ __launch_bounds__(kLossThreads) void k_tcnn_loss(const float* __restrict__ ltile, int64_t T, int64_t R,
                                                            const float* __restrict__ feats, int64_t B,
                                                            const float* __restrict__ grads, int train, float lr,
                                                            float beta1, float beta2, int64_t* __restrict__ adam_step,
                                                            float* __restrict__ st, float* __restrict__ loss) {
  __shared__ float s1[kLossThreads], s2[kLossThreads];
  __shared__ int bad_any;
  const int t = threadIdx.x;
  if (t == 0) bad_any = 0;
  float a = 0.0f;
  for (int64_t i = t; i < T; i += kLossThreads) a += ltile[i];
  bool bad = false;
  if (train)
    for (int64_t i = t; i < kParams; i += kLossThreads) bad = bad || !isfinite(grads[i]);
  s1[t] = a;
  s2[t] = loss_feat_norms(feats, B, t);
  __syncthreads();
  if (bad) bad_any = 1;   // every writer stores the same value; the barriers of the tree order it before the read
  loss_tree_sums(s1, s2, t);
  if (t == 0) {
    const float l1 = s1[0] / (float)R, reg = s2[0] / (float)B;
    const float total = kW_L1 * l1 + kW_Reg * reg;
    loss[0] = total;
    loss[1] = l1;
    loss[2] = reg;
    if (train) {
      const bool skip = bad_any || !isfinite(total);
      loss[3] = skip ? 1.0f : 0.0f;
      st[0] = skip ? 1.0f : 0.0f;
      if (!skip) {
        const int64_t step = *adam_step + 1;
        *adam_step = step;
        adam_bias_corrections(lr, beta1, beta2, step, &st[1], &st[2]);   // formed on the device
      }
    }
  }
}

// Adam (train_common.hpp: adam_update) with k_tcnn_loss's step size and bias correction, unless the step is marked
// skipped
__global__ void k_tcnn_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, int64_t P, float beta1, float beta2, float eps,
                            const float* __restrict__ st) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P || st[0] != 0.0f) return;
  adam_update(p, g, m, v, i, beta1, beta2, eps, st[1], st[2]);
}

// ---- host side ----

// per network: feature widths of the layer inputs (X) and outputs (dZ)
struct Net {
  int I[4], O[4];
  int64_t poff[4];
  int64_t P;
};
static Net make_net(int nin0) {
  Net t;
  const int I[4] = {nin0, kW, kW, kW}, O[4] = {kW, kW, kW, 16};
  int64_t o = 0;
  for (int l = 0; l < 4; ++l) {
    t.I[l] = I[l];
    t.O[l] = O[l];
    t.poff[l] = o;
    o += (int64_t)I[l] * O[l];
  }
  t.P = o;
  return t;
}
static int64_t tiles_per_chunk(int64_t T) {
  const int64_t c = cdiv(T, kMaxChunks);
  return c < 4 ? 4 : c;
}

struct Ws {
  _Float16 *img_e, *img_d;
  float *Y, *feats, *egrad, *dfrows, *ltile, *part, *st;
  _Float16 *act;     // X, Zh, Zl images of one network at a time
  size_t bytes;
};
static int64_t image_halves(const Net& N, int64_t T) {
  int64_t f = 0;
  for (int l = 0; l < 4; ++l) f += N.I[l] + 2 * N.O[l];
  return f * T * 32;
}
static size_t layout_ws(int64_t B, int n, int64_t M, char* base, Ws* w) {
  const int64_t Re = B * n, Rd = B * M, Te = cdiv(Re, 32), Td = cdiv(Rd, 32);
  const Net E = make_net(16), D = make_net(32);
  Carver c(base);
  Ws t;
  t.img_e = c.take<_Float16>(fwd_halves(1) + kBwdHalves);
  t.img_d = c.take<_Float16>(fwd_halves(2) + kBwdHalves);
  t.Y = c.take<float>(Re * kF);
  t.feats = c.take<float>(B * kF);
  t.egrad = c.take<float>(B * kF);
  t.dfrows = c.take<float>(Rd * kF);
  t.ltile = c.take<float>(Td);
  const int64_t ie = image_halves(E, Te), id = image_halves(D, Td);
  t.act = c.take<_Float16>(ie > id ? ie : id);
  t.part = c.take<float>(kMaxChunks * (E.P > D.P ? E.P : D.P));   // cdiv(T, tiles_per_chunk(T)) <= kMaxChunks
  t.st = c.take<float>(4);
  t.bytes = c.bytes();
  if (w) *w = t;
  return c.bytes();
}

// image pointers of one network inside the act region
static void set_images(const Net& N, int64_t T, _Float16* act, _Float16* X[4], _Float16* Zh[4], _Float16* Zl[4]) {
  int64_t o = 0;
  for (int l = 0; l < 4; ++l) {
    X[l] = act + o; o += (int64_t)N.I[l] * T * 32;
    Zh[l] = act + o; o += (int64_t)N.O[l] * T * 32;
    Zl[l] = act + o; o += (int64_t)N.O[l] * T * 32;
  }
}

static TileArgs tile_args(const Ws& w, int net, int64_t R, const float* input_pts, int n, const float* xyz,
                          const float* gt, int64_t M) {
  TileArgs a{};
  a.wf = net ? w.img_d : w.img_e;
  a.wt = a.wf + fwd_halves(net ? 2 : 1);
  a.R = R;
  a.T = cdiv(R, 32);
  a.input_pts = input_pts;
  a.n = n;
  a.xyz = xyz;
  a.feats = w.feats;
  a.gt = gt;
  a.M = M;
  a.Y = w.Y;
  a.egrad = w.egrad;
  a.dfrows = w.dfrows;
  set_images(make_net(net ? 32 : 16), a.T, w.act, a.X, a.Zh, a.Zl);
  return a;
}

// dW of one network from its images into grads (scaled), through per-chunk partials summed in chunk order
static int weight_grads(hipStream_t s, const Ws& w, int nin0, int64_t T, float scale, float* grads) {
  const Net N = make_net(nin0);
  DwArgs d{};
  set_images(N, T, w.act, const_cast<_Float16**>(d.X), const_cast<_Float16**>(d.Zh), const_cast<_Float16**>(d.Zl));
  int nb = 0;
  for (int l = 0; l < 4; ++l) {
    d.I[l] = N.I[l];
    d.O[l] = N.O[l];
    d.poff[l] = N.poff[l];
    for (int bo = 0; bo < (int)cdiv(N.O[l], 32); ++bo)
      for (int bi = 0; bi < (int)cdiv(N.I[l], 32); ++bi) {
        d.blk_l[nb] = l;
        d.blk_o[nb] = bo;
        d.blk_i[nb] = bi;
        ++nb;
      }
  }
  d.T = T;
  d.tpc = tiles_per_chunk(T);
  d.part = w.part;
  d.P = N.P;
  const int64_t S = cdiv(T, d.tpc);
  k_tcnn_dw<<<dim3((unsigned)nb, (unsigned)S), 64, 0, s>>>(d);
  k_sum_partials<<<blocks_for(N.P, 256), 256, 0, s>>>(w.part, S, N.P, scale, grads);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

// pack, encoder forward, patch means
static int encode(hipStream_t s, const float* params, const float* input_pts, int64_t B, int n, const Ws& w) {
  const int64_t tot = fwd_halves(1) + fwd_halves(2) + 2 * kBwdHalves;
  k_tcnn_pack<<<blocks_for(tot, 256), 256, 0, s>>>(params, w.img_e, w.img_d);
  const TileArgs a = tile_args(w, 0, B * n, input_pts, n, nullptr, nullptr, 0);
  k_tcnn_tile<0, 0><<<blocks_for(a.T, 4), 256, 0, s>>>(a);
  k_patch_mean<true><<<blocks_for(B * kF, 256), 256, 0, s>>>(w.Y, B, n, w.feats);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

}  // namespace train_tcnn
}  // namespace bnv

using namespace bnv;
using namespace bnv::train_tcnn;

extern "C" {

int64_t bnv_train_tcnn_param_floats(void) { return kParams; }

size_t bnv_train_tcnn_workspace_bytes(int64_t B, int32_t n, int64_t M) {
  if (!train_shape_ok(B, n, M)) return 0;
  return layout_ws(B, n, M, nullptr, nullptr);
}

int bnv_train_tcnn_step(float* params, float* grads, float* adam_m, float* adam_v, int64_t* adam_step,
                        const float* input_pts, const float* training_pts, const float* gt, int64_t B, int32_t n,
                        int64_t M, float lr, float beta1, float beta2, float eps, float* loss_out, void* workspace,
                        size_t ws_bytes, bnv_stream_t stream) {
  if (!train_shape_ok(B, n, M) || !adam_args_ok(lr, beta1, beta2, eps)) return BNV_ERR_INVALID_ARGUMENT;
  if (!params || !grads || !adam_m || !adam_v || !adam_step || !input_pts || !training_pts || !gt || !loss_out)
    return BNV_ERR_INVALID_ARGUMENT;
  Ws w;
  if (!workspace || ws_bytes < layout_ws(B, n, M, (char*)workspace, &w)) return BNV_ERR_WORKSPACE_TOO_SMALL;
  if (bnv::g_num_cus <= 0) return BNV_ERR_NOT_INITIALISED;
  hipStream_t s = (hipStream_t)stream;
  const int64_t Re = B * n, Rd = B * M;
  BNV_TRY(encode(s, params, input_pts, B, n, w));
  // decoder: forward, loss partials, backward to the feature columns; its weight gradients
  TileArgs d = tile_args(w, 1, Rd, nullptr, n, training_pts, gt, M);
  d.ltile = w.ltile;
  k_tcnn_tile<1, 1><<<bnv::blocks_for(d.T, 4), 256, 0, s>>>(d);
  BNV_LAUNCH_CHECK();
  BNV_TRY(weight_grads(s, w, 32, d.T, 1.0f / (float)Rd, grads + kEncParams));
  // encoder: d feats, then forward again and backward; its weight gradients
  k_tcnn_dfeats<<<bnv::blocks_for(B * kF, 256), 256, 0, s>>>(w.dfrows, w.feats, B, M, w.egrad);
  const TileArgs e = tile_args(w, 0, Re, input_pts, n, nullptr, nullptr, 0);
  k_tcnn_tile<0, 1><<<bnv::blocks_for(e.T, 4), 256, 0, s>>>(e);
  BNV_LAUNCH_CHECK();
  BNV_TRY(weight_grads(s, w, 16, e.T, 1.0f / (float)Re, grads));
  k_tcnn_loss<<<1, kLossThreads, 0, s>>>(w.ltile, d.T, Rd, w.feats, B, grads, 1, lr, beta1, beta2, adam_step, w.st,
                                         loss_out);
  k_tcnn_adam<<<bnv::blocks_for(kParams, 256), 256, 0, s>>>(params, grads, adam_m, adam_v, kParams, beta1, beta2, eps, w.st);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

int bnv_train_tcnn_eval_loss(const float* params, const float* input_pts, const float* training_pts, const float* gt,
                             int64_t B, int32_t n, int64_t M, float* loss_out, void* workspace, size_t ws_bytes,
                             bnv_stream_t stream) {
  if (!train_shape_ok(B, n, M)) return BNV_ERR_INVALID_ARGUMENT;
  if (!params || !input_pts || !training_pts || !gt || !loss_out) return BNV_ERR_INVALID_ARGUMENT;
  Ws w;
  if (!workspace || ws_bytes < layout_ws(B, n, M, (char*)workspace, &w)) return BNV_ERR_WORKSPACE_TOO_SMALL;
  if (bnv::g_num_cus <= 0) return BNV_ERR_NOT_INITIALISED;
  hipStream_t s = (hipStream_t)stream;
  BNV_TRY(encode(s, params, input_pts, B, n, w));
  TileArgs d = tile_args(w, 1, B * M, nullptr, n, training_pts, gt, M);
  d.ltile = w.ltile;
  k_tcnn_tile<1, 0><<<bnv::blocks_for(d.T, 4), 256, 0, s>>>(d);
  k_tcnn_loss<<<1, kLossThreads, 0, s>>>(w.ltile, d.T, B * M, w.feats, B, nullptr, 0, 0.0f, 0.0f, 0.0f, nullptr,
                                         nullptr, loss_out);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

int bnv_train_tcnn_forward(const float* params, const float* input_pts, const float* training_pts, int64_t B,
                           int32_t n, int64_t M, float* feats, float* pred, void* workspace, size_t ws_bytes,
                           bnv_stream_t stream) {
  if (!train_shape_ok(B, n, M)) return BNV_ERR_INVALID_ARGUMENT;
  if (!params || !input_pts || !training_pts || !feats || !pred) return BNV_ERR_INVALID_ARGUMENT;
  Ws w;
  if (!workspace || ws_bytes < layout_ws(B, n, M, (char*)workspace, &w)) return BNV_ERR_WORKSPACE_TOO_SMALL;
  if (bnv::g_num_cus <= 0) return BNV_ERR_NOT_INITIALISED;
  hipStream_t s = (hipStream_t)stream;
  BNV_TRY(encode(s, params, input_pts, B, n, w));
  TileArgs d = tile_args(w, 1, B * M, nullptr, n, training_pts, nullptr, M);
  d.pred = pred;
  k_tcnn_tile<1, 0><<<bnv::blocks_for(d.T, 4), 256, 0, s>>>(d);
  BNV_HIP_CHECK(hipMemcpyAsync(feats, w.feats, sizeof(float) * B * kF, hipMemcpyDeviceToDevice, s));
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

}  // extern "C"
