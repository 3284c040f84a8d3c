// The tiny-cuda-nn networks of the reference's default checkpoint (pointnet_tcnn: FullyFusedMLP, 64 wide, three
// hidden layers, ReLU, no bias, fp16 weights and activations) as ONE wave tile: 32 evaluations per wave on
// v_mfma_f32_32x32x16_f16, fp32 accumulation, activations in registers, rounded to f16 between layers as the CUDA
// kernel stores them.  Encoder 16 | 64 | 64 | 64 | 16 (NK0 = 1 input K-step), SDF decoder 32 | 64 | 64 | 64 | 16
// (NK0 = 2); inputs are padded with 1.0 (the pad columns act as biases).
//
// This is the only place the tile is written.  Every kernel that runs these networks (sdf_mlp.hpp: sdf_mlp_tile_t;
// decode_pts.hip: k_decode_pts_bwd_t; decode.hip: k_lattice_table_t; encode_tcnn.hip: k_pointnet_scatter_t, k_pointnet_scatter_tb; train_tcnn.hip:
// k_tcnn_tile) brings its own inputs and takes the outputs where it needs them; the operands and the MFMA order
// per accumulator (mb outer, K-step inner, accumulate in place) are the ones below, so the kernels agree bit for bit.
//
// Lane (j = lane & 31, h = lane >> 5) holds evaluation j.  Operand slot jj of lane half h holds feature
// 8 (jj >> 2) + 4 h + (jj & 3) of a 16-deep K-step: the row order of a 32x32 MFMA result's registers, so a layer's
// output tile feeds the next MFMA as its B operand with no data movement (weights.py: _slot_feature).
#pragma once
#include "bnv_common.hpp"

namespace bnv {

// Weight pack of a network (halves): fragments of 8 halves, fragment (mb * NK + ks) * 64 + lane of a layer with NK
// K-steps.  W0 [2 mb][NK0 ks][64 lane][8] | W1, W2 [2 mb][4 ks][64][8] | W3 [4 ks][64][8] (rows >= 16 zero).
// weights.py: pack_pointnet_tcnn (NK0 = 1), pack_sdf_tcnn (NK0 = 2); train_tcnn.hip: k_tcnn_pack.
template <int NK0>
struct TcnnPack {
  static constexpr int W0 = 0;
  static constexpr int W1 = W0 + 2 * NK0 * 64 * 8;
  static constexpr int W2 = W1 + 2 * 4 * 64 * 8;
  static constexpr int W3 = W2 + 2 * 4 * 64 * 8;
  static constexpr int TOTAL = W3 + 4 * 64 * 8;
};
static_assert(TcnnPack<1>::TOTAL == 11264, "tcnn encoder pack size (weights.py: pack_pointnet_tcnn)");
static_assert(TcnnPack<2>::TOTAL == 12288, "tcnn SDF pack size (weights.py: pack_sdf_tcnn)");

__host__ __device__ constexpr int tcnn_slot_feature(int jj, int h) { return 8 * (jj >> 2) + 4 * h + (jj & 3); }

__device__ __forceinline__ f32x16 zero16() {
  f32x16 v;
#pragma unroll
  for (int r = 0; r < 16; ++r) v[r] = 0.f;
  return v;
}
__device__ __forceinline__ f32x16 mfma_f16(half8 a, half8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}
// fragment `frag` of a layer (or of any image of 64-lane fragments); w in global memory or in LDS
__device__ __forceinline__ half8 tcnn_wfrag(const _Float16* w, int frag, int lane) {
  return *(const half8*)&w[(frag * 64 + lane) * 8];
}

// ReLU + f16 of registers base .. base + 7 of an accumulator
__device__ __forceinline__ half8 relu_half8(const f32x16& v, int base) {
  half8 r;
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = (_Float16)relu_bits(v[base + e]);
  return r;
}
// the accumulator pair of a 64-wide layer as the four B fragments of the next: K-step g = registers 8 (g & 1) .. of
// accumulator g >> 1
__device__ __forceinline__ void tcnn_relu_round(const f32x16 (&a)[2], half8 (&s)[4]) {
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
    s[nb * 2] = relu_half8(a[nb], 0);
    s[nb * 2 + 1] = relu_half8(a[nb], 8);
  }
}
// bit 16 mb + r: a[mb][r] > 0 (where the ReLU passes a gradient)
__device__ __forceinline__ uint32_t positive_bits32(const f32x16 (&a)[2]) {
  uint32_t m = 0u;
#pragma unroll
  for (int mb = 1; mb >= 0; --mb) {
#pragma unroll
    for (int r = 15; r >= 0; --r) m = (m << 1) | (uint32_t)(a[mb][r] > 0.f);
  }
  return m;
}

// ---- layers: w points at the layer's fragments -------------------------------------------------------------------
template <int NK0>
__device__ __forceinline__ void tcnn_first_layer(const _Float16* w, int lane, const half8 (&x)[NK0], f32x16 (&out)[2]) {
#pragma unroll
  for (int mb = 0; mb < 2; ++mb) {
    out[mb] = zero16();
#pragma unroll
    for (int ks = 0; ks < NK0; ++ks) out[mb] = mfma_f16(tcnn_wfrag(w, mb * NK0 + ks, lane), x[ks], out[mb]);
  }
}
// 64 -> 64.  Also the shape of the transposed hidden layers of the backward passes.
__device__ __forceinline__ void tcnn_hidden_layer(const _Float16* w, int lane, const half8 (&s)[4], f32x16 (&out)[2]) {
#pragma unroll
  for (int mb = 0; mb < 2; ++mb) {
    out[mb] = zero16();
#pragma unroll
    for (int g = 0; g < 4; ++g) out[mb] = mfma_f16(tcnn_wfrag(w, mb * 4 + g, lane), s[g], out[mb]);
  }
}
// 64 -> 16 (one row block; rows >= 16 of the fragments are zero): lane (j, h) holds outputs 4 h + r of evaluation j in
// registers r < 4 (and outputs 8 + 4 h .. in registers 4 .. 7), so output 0 = row 0 of the tile = register 0 of the
// lanes with h == 0.  fp32 here: the network returns fp16, the caller rounds the registers it uses.
__device__ __forceinline__ f32x16 tcnn_output_layer(const _Float16* w, int lane, const half8 (&s)[4]) {
  f32x16 o = zero16();
#pragma unroll
  for (int g = 0; g < 4; ++g) o = mfma_f16(tcnn_wfrag(w, g, lane), s[g], o);
  return o;
}

// the whole network on the input fragments x of this lane; w: the network's pack
template <int NK0>
__device__ __forceinline__ f32x16 tcnn_forward(const _Float16* w, int lane, const half8 (&x)[NK0]) {
  typedef TcnnPack<NK0> P;
  f32x16 a0[2], a1[2];
  half8 s[4];
  tcnn_first_layer<NK0>(w + P::W0, lane, x, a0);
  tcnn_relu_round(a0, s);
  tcnn_hidden_layer(w + P::W1, lane, s, a1);
  tcnn_relu_round(a1, s);
  tcnn_hidden_layer(w + P::W2, lane, s, a0);
  tcnn_relu_round(a0, s);
  return tcnn_output_layer(w + P::W3, lane, s);
}

// ---- inputs --------------------------------------------------------------------------------------------------------
// B fragment of K-step ks for lane half h from the evaluation's NIN padded inputs
template <int NIN>
__device__ __forceinline__ half8 tcnn_input_frag(const float (&in)[NIN], int ks, int h) {
  half8 v;
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) {
    // both values first: a select between the two ELEMENTS would be an index that depends on the lane
    const float lo = in[16 * ks + tcnn_slot_feature(jj, 0)], hi = in[16 * ks + tcnn_slot_feature(jj, 1)];
    v[jj] = (_Float16)(h ? hi : lo);
  }
  return v;
}
// inputs of the SDF decoder (tcnnNeRFModel, modules.py:136-253): [p, sin p, cos p, feat], 17 values padded to 32
// with 1.0
__device__ __forceinline__ void tcnn_sdf_inputs(const float (&loc)[3], const float (&feat)[8], float (&in)[32]) {
#pragma unroll
  for (int f = 17; f < 32; ++f) in[f] = 1.0f;
  in[0] = loc[0]; in[1] = loc[1]; in[2] = loc[2];
  in[3] = sinf(loc[0]); in[4] = sinf(loc[1]); in[5] = sinf(loc[2]);
  in[6] = cosf(loc[0]); in[7] = cosf(loc[1]); in[8] = cosf(loc[2]);
#pragma unroll
  for (int f = 0; f < 8; ++f) in[9 + f] = feat[f];
}

}  // namespace bnv
