// sdf_mlp.hpp -- the SDF-decoder MLP tile (reference modules.py:81-123,657-662) on gfx950, in its four arithmetic modes.
// Only constants, typedefs, structs and __device__ __forceinline__ functions: the kernels that run the tile are in
// decode.hip (tables, dense grids) and decode_pts.hip (arbitrary points and their gradient).
//
// One MLP core, 17 -> 256 -> 256 -> 256 -> 256 -> 1 in exact fp32 on v_mfma_f32_32x32x2_f32:
//   * a workgroup (8 waves) evaluates a tile of 128 inputs; wave w owns output features
//     [32w, 32w+32) of every layer for all 128 inputs (4 MFMA column tiles of 32);
//   * activations live in LDS as HL[kb][h][j][4] (feature 8kb+4h+i of input j): a wave reads its
//     B operands with conflict-free ds_read_b128 and writes its D registers back with
//     ds_write_b128 -- D register 4q+i of lane (j,h) IS feature 32w+8q+4h+i, the same layout;
//   * weights stream from L2 (0.8 MB, resident in every XCD's 4 MB L2) as one coalesced
//     dwordx4 per lane per 8-deep K block, pre-permuted on the host (weights.py: pack_sdf_mlp).
#pragma once
#include "bnv_common.hpp"
#include "tcnn_mlp.hpp"

namespace bnv {

constexpr int DM = 128;  // MLP inputs per tile

// packed SDF-MLP weights (floats)
constexpr int SD_W0 = 0;                      // [8 w][3 kb][64 lane][4]
constexpr int SD_W1 = SD_W0 + 8 * 3 * 256;    // [8 w][32 kb][64 lane][4]
constexpr int SD_W2 = SD_W1 + 65536;
constexpr int SD_W3 = SD_W2 + 65536;
constexpr int SD_B0 = SD_W3 + 65536;          // [256] x 4
constexpr int SD_WA = SD_B0 + 4 * 256;        // fc_alpha weight [256]
constexpr int SD_BA = SD_WA + 256;            // fc_alpha bias, padded to 4; [1] = certified |feature| bound (below)
constexpr int SD_TOTAL = SD_BA + 4;
// split-operand variant, appended to the same pack (units: 16-bit halves from float offset SD_TOTAL)
constexpr int SH_W0 = 0;                          // [8 w][2 ks][2 hi/lo][64 lane][8]
constexpr int SH_W1 = SH_W0 + 8 * 2 * 2 * 64 * 8; // [8 w][16 ks][2 hi/lo][64 lane][8]
constexpr int SH_W2 = SH_W1 + 8 * 16 * 2 * 64 * 8;
constexpr int SH_W3 = SH_W2 + 8 * 16 * 2 * 64 * 8;
constexpr int SH_TOTAL = SH_W3 + 8 * 16 * 2 * 64 * 8;   // 409,600 halves
constexpr int SD_PACK_FLOATS = SD_TOTAL + SH_TOTAL / 2;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// weight fragment fetch through a buffer descriptor: wave-uniform base (SGPRs) + one shared per-lane
// byte offset + a scalar offset per load -- no 64-bit address VGPR per load (with flat loads the compiler
// hoists dozens of lane-constant addresses out of the tile loop and spills them)
__device__ __forceinline__ half8 load_frag(__amdgpu_buffer_rsrc_t rs, int voff, int soff) {
  const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0);
  return __builtin_bit_cast(half8, v);
}

// LDS (floats)
constexpr int L_HL = 0;                       // [32 kb][2 h][128 j][4]
constexpr int L_PART = L_HL + 32 * 2 * DM * 4;  // [8 w][2 h][128]
constexpr int L_ALPHA = L_PART + 16 * DM;     // [128]
constexpr int L_WTRI = L_ALPHA + DM;          // [128] trilinear weight of the evaluation
constexpr int L_WVOL = L_WTRI + DM;           // [128] volume weight (or dense count) of its corner
constexpr int L_DELTA = L_WVOL + DM;          // [128] sdf_delta sample of its corner
constexpr int L_TOTAL = L_DELTA + DM;         // 35,328 floats = 141,312 B

// MODE_PTS runs k_decode_pts, the others k_decode.  MODE_DENSE1: the two one-evaluation-per-query branches of
// decode_feature_grid_w_pts (DecodeArgs::variant).
enum { MODE_PTS = 0, MODE_LATTICE = 1, MODE_DENSE = 2, MODE_DENSE1 = 3 };

// Phase timing of the decode tile loop (development builds only: -DBNV_PHASE_PROF, tools/phase_prof.py).
// Thread 0 of every workgroup accumulates shader-clock deltas per phase in LDS; the kernels of decode.hip add them
// to g_phase_cycles at their end.
#ifdef BNV_PHASE_PROF
constexpr int L_PROF = L_TOTAL;  // [8 waves][32] x u64 behind the regular LDS layout
#define BNV_PH(i)                                                                 \
  do {                                                                            \
    if ((threadIdx.x & 63) == 0) {                                                \
      unsigned long long* _p = (unsigned long long*)(lds + L_PROF) + (threadIdx.x >> 6) * 32; \
      const unsigned long long _t = clock64();                                    \
      _p[i] += _t - _p[31];                                                       \
      _p[31] = _t;                                                                \
    }                                                                             \
  } while (0)
#else
#define BNV_PH(i)
#endif

struct DecodeArgs {
  bnv_volume_t vol;
  bnv_grid_t grid;
  const float* features;
  const float* weights;
  int64_t row_limit;
  const float* pack;
  const float* coords;
  int64_t n;
  int is_coords;
  bnv_sdf_delta_t delta;
  float* out;
  // LATTICE: work list of rows (27 evaluations each) or, if `entries` is set, of (row << 5 | l) entries
  const int32_t* list;
  const int32_t* n_list;
  float* table;
  const int32_t* entries;
  uint32_t* need_mask;
  // DENSE
  const float* feat_grid;
  const float* pts_weight;
  int32_t dims[3];
  // DENSE1: 0 = nearest voxel (interpolate_decode=False), 1 = global coordinates (trilinear features)
  int32_t variant;
  float* nf_out;     // optional [n, 8]: the features the evaluation used
  int32_t* status;   // optional: [1] = 5 when a feature leaves the certified range of the split arithmetic
  int32_t half_tail; // k_lattice_table_x: hand the last partial round out as 64-evaluation tiles
  // PTS, several ray splits of an optimiser step in ONE call (bnv_optim_step, bnv_decode_pts with a split_mask): query q belongs
  // to split q / split_samples; bit s of split_mask[row] = split s touches the row (bnv_volume_count_optim_splits).
  // The weight the mask decision of a split-s query sees is weights[row] + 1 for every split <= s that touches the
  // row -- count_optim (sparse_volume.py:602-622) called split by split, render_utils.py:491-497.  Null: plain weights.
  const uint32_t* split_mask;
  int64_t split_samples;
};

__device__ __forceinline__ f32x16 frag256(const float* __restrict__ b, int w, int h) {
  f32x16 v;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x4 t = *(const f32x4*)&b[w * 32 + 8 * q + 4 * h];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[4 * q + i] = t[i];
  }
  return v;
}

template <int NKB>
__device__ __forceinline__ void mlp_layer(const float* __restrict__ wp, const float* __restrict__ bias,
                                          const float* __restrict__ hl, f32x16 (&acc)[4], int w, int lane,
                                          int j, int h) {
  const f32x16 b0 = frag256(bias, w, h);
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) acc[pt] = b0;
  const float* wl = wp + (size_t)w * NKB * 256 + lane * 4;
  const float* hb = hl + (h * DM + j) * 4;
#pragma unroll 4
  for (int kb = 0; kb < NKB; ++kb) {
    const f32x4 a = *(const f32x4*)(wl + kb * 256);
    f32x4 b[4];
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) b[pt] = *(const f32x4*)(hb + (kb * 2 * DM + pt * 32) * 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int pt = 0; pt < 4; ++pt)
        acc[pt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[pt][i], acc[pt], 0, 0, 0);
    }
  }
}

__device__ __forceinline__ void store_relu(float* __restrict__ hl, const f32x16 (&acc)[4], int w, int j, int h) {
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f32x4 v;
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = relu_bits(acc[pt][4 * q + i]);
      *(f32x4*)&hl[(((4 * w + q) * 2 + h) * DM + pt * 32 + j) * 4] = v;
    }
  }
}

// Runs the MLP on the 128 inputs staged in HL[kb 0..2]; leaves alpha[128] (raw network output).
__device__ __forceinline__ void sdf_mlp_tile(float* __restrict__ lds, const float* __restrict__ pack) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 31, h = lane >> 5;
  float* hl = lds + L_HL;
  f32x16 acc[4];
  mlp_layer<3>(pack + SD_W0, pack + SD_B0, hl, acc, w, lane, j, h);
  __syncthreads();
  store_relu(hl, acc, w, j, h);
  __syncthreads();
  mlp_layer<32>(pack + SD_W1, pack + SD_B0 + 256, hl, acc, w, lane, j, h);
  __syncthreads();
  store_relu(hl, acc, w, j, h);
  __syncthreads();
  mlp_layer<32>(pack + SD_W2, pack + SD_B0 + 512, hl, acc, w, lane, j, h);
  __syncthreads();
  store_relu(hl, acc, w, j, h);
  __syncthreads();
  mlp_layer<32>(pack + SD_W3, pack + SD_B0 + 768, hl, acc, w, lane, j, h);
  // fc_alpha: 256 -> 1.  Each lane reduces its 16 features, partials are summed in a fixed order.
  const f32x16 wa = frag256(pack + SD_WA, w, h);
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) s = fmaf(wa[r], relu_bits(acc[pt][r]), s);
    lds[L_PART + (w * 2 + h) * DM + pt * 32 + j] = s;
  }
  __syncthreads();
  if (threadIdx.x < DM) {
    float s = pack[SD_BA];
#pragma unroll
    for (int p = 0; p < 16; ++p) s += lds[L_PART + p * DM + threadIdx.x];
    lds[L_ALPHA + threadIdx.x] = s;
  }
  __syncthreads();
}

// writes the 17 network inputs [local(3), sin(3), cos(3), feat(8)] of evaluation j into HL
__device__ __forceinline__ void stage_input(float* __restrict__ hl, int j, const float (&loc)[3],
                                            const float (&feat)[8]) {
  const float s0 = sinf(loc[0]), s1 = sinf(loc[1]), s2 = sinf(loc[2]);
  const float c0 = cosf(loc[0]), c1 = cosf(loc[1]), c2 = cosf(loc[2]);
  const f32x4 v0 = {loc[0], loc[1], loc[2], s0};
  const f32x4 v1 = {s1, s2, c0, c1};
  const f32x4 v2 = {c2, feat[0], feat[1], feat[2]};
  const f32x4 v3 = {feat[3], feat[4], feat[5], feat[6]};
  const f32x4 v4 = {feat[7], 0.f, 0.f, 0.f};
  const f32x4 v5 = {0.f, 0.f, 0.f, 0.f};
  *(f32x4*)&hl[((0 * 2 + 0) * DM + j) * 4] = v0;
  *(f32x4*)&hl[((0 * 2 + 1) * DM + j) * 4] = v1;
  *(f32x4*)&hl[((1 * 2 + 0) * DM + j) * 4] = v2;
  *(f32x4*)&hl[((1 * 2 + 1) * DM + j) * 4] = v3;
  *(f32x4*)&hl[((2 * 2 + 0) * DM + j) * 4] = v4;
  *(f32x4*)&hl[((2 * 2 + 1) * DM + j) * 4] = v5;
}

// ---- split-operand MLP core: x = hi + lo (f16), a.b ~ ah.bh + ah.bl + al.bh on the f16 MFMA ----
// LDS: HH[ks][h][j][8 halves] (hi) at L_HL, HLo (lo) 64 KB behind it; slot jj of lane half h in
// K-step ks is feature 16 ks + 8 (jj >> 2) + 4 h + (jj & 3), which makes D registers 8 ksl .. 8 ksl+7
// of wave w exactly the 8 slots of K-step 2 w + ksl.
constexpr int L_HLO = L_HL + 16 * 2 * DM * 4;  // float offset of the lo plane

__device__ __forceinline__ float relu1(float x) { return relu_bits(x); }

#ifndef BNV_A_AHEAD
#define BNV_A_AHEAD 2
#endif
// NPROD = 3: split operands (al.bh + ah.bl + ah.bh); NPROD = 1: f16 operands (ah.bh only; MLP mode 3)
template <int NKS, bool BIAS = true, int NPROD = 3>
__device__ __forceinline__ void mlp_layer_h(const _Float16* __restrict__ wp, const float* __restrict__ bias,
                                            const float* __restrict__ lds, f32x16 (&acc)[4], int w, int lane,
                                            int j, int h) {
  f32x16 b0;
  if constexpr (BIAS) {
    b0 = frag256(bias, w, h);
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) b0[r] = 0.f;
  }
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) acc[pt] = b0;
  const _Float16* wl = wp + (size_t)w * NKS * 2 * 64 * 8 + lane * 8;
  const float* hh = lds + L_HL + (h * DM + j) * 4;
  const float* hl = lds + L_HLO + (h * DM + j) * 4;
  // software pipeline over the K-steps (fully unrolled, all indices static): weight fragments come
  // from L2 kAhead steps ahead (register ring), activation fragments from LDS one step ahead
  constexpr int kAhead = BNV_A_AHEAD, kRing = kAhead + 1;
  half8 ah[kRing], al[kRing], bh[2][4], bl[2][4];
#define BNV_LOAD_A(ks)                                                                  \
  {                                                                                     \
    ah[(ks) % kRing] = *(const half8*)(wl + ((ks) * 2) * 64 * 8);                       \
    if (NPROD == 3) al[(ks) % kRing] = *(const half8*)(wl + ((ks) * 2 + 1) * 64 * 8);   \
  }
#define BNV_LOAD_B(ks)                                                                    \
  {                                                                                       \
    _Pragma("unroll") for (int pt = 0; pt < 4; ++pt) {                                    \
      bh[(ks) & 1][pt] = *(const half8*)(hh + ((ks) * 2 * DM + pt * 32) * 4);             \
      if (NPROD == 3) bl[(ks) & 1][pt] = *(const half8*)(hl + ((ks) * 2 * DM + pt * 32) * 4); \
    }                                                                                     \
  }
#pragma unroll
  for (int p = 0; p < kAhead; ++p)
    if (p < NKS) BNV_LOAD_A(p);
  BNV_LOAD_B(0);
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    if (ks + kAhead < NKS) BNV_LOAD_A(ks + kAhead);
    if (ks + 1 < NKS) BNV_LOAD_B(ks + 1);
    const half8 a_hi = ah[ks % kRing];
    if constexpr (NPROD == 3) {
      const half8 a_lo = al[ks % kRing];
#pragma unroll
      for (int pt = 0; pt < 4; ++pt)
        acc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo, bh[ks & 1][pt], acc[pt], 0, 0, 0);
#pragma unroll
      for (int pt = 0; pt < 4; ++pt)
        acc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, bl[ks & 1][pt], acc[pt], 0, 0, 0);
    }
#pragma unroll
    for (int pt = 0; pt < 4; ++pt)
      acc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, bh[ks & 1][pt], acc[pt], 0, 0, 0);
    // Issue order inside the step: every prefetch goes into the shadow of an MFMA (one memory instruction
    // behind each MFMA).  A wave then keeps the MFMA pipe busy on its own; with all the loads clustered at
    // the top of the step a lone wave reached only 55-70 % (tools/phase_prof.py).
    constexpr int kDs = NPROD == 3 ? 8 : 4, kVm = NPROD == 3 ? 2 : 1;
    if (ks + 1 < NKS) {
#pragma unroll
      for (int g = 0; g < (NPROD == 3 ? kDs : kDs - 1); ++g) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // 1 DS read
      }
      if (NPROD == 1) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    }
    if (ks + kAhead < NKS) {
#pragma unroll
      for (int g = 0; g < kVm; ++g) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // 1 VMEM read
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
#undef BNV_LOAD_A
#undef BNV_LOAD_B
}

template <int NPROD = 3>
__device__ __forceinline__ void store_relu_h(float* __restrict__ lds, const f32x16 (&acc)[4], int w, int j, int h) {
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
#pragma unroll
    for (int ksl = 0; ksl < 2; ++ksl) {
      half8 hi, lo;
      if (NPROD == 3) {
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = relu1(acc[pt][8 * ksl + e]);
        split8_f16(x, hi, lo);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) hi[e] = (_Float16)relu1(acc[pt][8 * ksl + e]);
      }
      const int o = (((2 * w + ksl) * 2 + h) * DM + pt * 32 + j) * 4;
      *(half8*)&lds[L_HL + o] = hi;
      if (NPROD == 3) *(half8*)&lds[L_HLO + o] = lo;
    }
  }
}

template <int NPROD = 3>
__device__ __forceinline__ void sdf_mlp_tile_h(float* __restrict__ lds, const float* __restrict__ pack) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 31, h = lane >> 5;
  const _Float16* ph = (const _Float16*)(pack + SD_TOTAL);
  f32x16 acc[4];
  mlp_layer_h<2, true, NPROD>(ph + SH_W0, pack + SD_B0, lds, acc, w, lane, j, h);
  BNV_PH(1);
  __syncthreads();
  BNV_PH(2);
  store_relu_h<NPROD>(lds, acc, w, j, h);
  BNV_PH(3);
  __syncthreads();
  BNV_PH(4);
  mlp_layer_h<16, true, NPROD>(ph + SH_W1, pack + SD_B0 + 256, lds, acc, w, lane, j, h);
  BNV_PH(5);
  __syncthreads();
  BNV_PH(6);
  store_relu_h<NPROD>(lds, acc, w, j, h);
  BNV_PH(7);
  __syncthreads();
  BNV_PH(8);
  mlp_layer_h<16, true, NPROD>(ph + SH_W2, pack + SD_B0 + 512, lds, acc, w, lane, j, h);
  BNV_PH(9);
  __syncthreads();
  BNV_PH(10);
  store_relu_h<NPROD>(lds, acc, w, j, h);
  BNV_PH(11);
  __syncthreads();
  BNV_PH(12);
  mlp_layer_h<16, true, NPROD>(ph + SH_W3, pack + SD_B0 + 768, lds, acc, w, lane, j, h);
  BNV_PH(13);
  const f32x16 wa = frag256(pack + SD_WA, w, h);
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) s = fmaf(wa[r], relu_bits(acc[pt][r]), s);
    lds[L_PART + (w * 2 + h) * DM + pt * 32 + j] = s;
  }
  BNV_PH(14);
  __syncthreads();
  BNV_PH(15);
  if (threadIdx.x < DM) {
    float s = pack[SD_BA];
#pragma unroll
    for (int p = 0; p < 16; ++p) s += lds[L_PART + p * DM + threadIdx.x];
    lds[L_ALPHA + threadIdx.x] = s;
  }
  __syncthreads();
  BNV_PH(16);
}

// Range certificate of the f16-split arithmetic (MLP modes 1 and 3; weights.py: certified_input_bound): with the
// local coordinates and their sin / cos in [-1, 1] and |feature| <= pack[SD_BA + 1], no value of any layer can
// reach the f16 overflow threshold (65,520), where fp32 -- the reference's arithmetic -- would still be fine.  A
// feature row beyond the bound (or NaN) sets the volume's sticky error word to 5 instead of silently producing
// inf / NaN: the caller then switches to exact fp32 (bnv_set_mlp_mode(0)).  8 compares per EVALUATION, not per
// activation: free.
__device__ __forceinline__ void check_feature_range(const float (&feat)[8], float bound, int32_t* __restrict__ status) {
  float m = fmaxf(fabsf(feat[0]), fabsf(feat[1]));
#pragma unroll
  for (int f = 2; f < 8; ++f) m = fmaxf(m, fabsf(feat[f]));
  bool bad = !(m <= bound);
#pragma unroll
  for (int f = 0; f < 8; ++f) bad = bad || (feat[f] != feat[f]);   // fmaxf drops NaNs
  if (bad && status) status[1] = 5;
}

// inputs of evaluation j in the split layout: features 0..16 (+15 zero) over K-steps 0, 1
template <int NPROD = 3>
__device__ __forceinline__ void stage_input_h(float* __restrict__ lds, int j, const float (&loc)[3],
                                              const float (&feat)[8]) {
  float in[32];
#pragma unroll
  for (int f = 0; f < 32; ++f) in[f] = 0.f;
  in[0] = loc[0]; in[1] = loc[1]; in[2] = loc[2];
  in[3] = sinf(loc[0]); in[4] = sinf(loc[1]); in[5] = sinf(loc[2]);
  in[6] = cosf(loc[0]); in[7] = cosf(loc[1]); in[8] = cosf(loc[2]);
#pragma unroll
  for (int f = 0; f < 8; ++f) in[9 + f] = feat[f];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      half8 hi, lo;
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const float x = in[16 * ks + 8 * (jj >> 2) + 4 * hh + (jj & 3)];
        const _Float16 t = (_Float16)x;
        hi[jj] = t;
        if (NPROD == 3) lo[jj] = (_Float16)(x - (float)t);
      }
      const int o = ((ks * 2 + hh) * DM + j) * 4;
      *(half8*)&lds[L_HL + o] = hi;
      if (NPROD == 3) *(half8*)&lds[L_HLO + o] = lo;
    }
  }
}

// ---- tiny-cuda-nn SDF decoder (reference default checkpoint; tcnnNeRFModel, modules.py:136-253):
// 17 inputs padded to 32 with 1.0 -> 64 -> 64 -> 64 -> 16 (output 0 used), ReLU, no bias, fp16.
// The network is small enough that ONE wave runs all layers for 32 evaluations in registers (no
// barriers between layers); waves 0..3 of the workgroup cover the tile's 128 evaluations.
// Network, pack layout and wave tile: tcnn_mlp.hpp (NK0 = 2).
typedef TcnnPack<2> SdfPack;

__device__ __forceinline__ void sdf_mlp_tile_t(float* __restrict__ lds, const float* __restrict__ pack) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 31, h = lane >> 5;
  if (w < 4) {
    const int col = w * 32 + j;
    half8 x[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) x[ks] = *(const half8*)&lds[L_HL + ((ks * 2 + h) * DM + col) * 4];
    const f32x16 o = tcnn_forward<2>((const _Float16*)pack, lane, x);
    // output 0 = register 0 of the lanes with h == 0; the network returns fp16
    if (h == 0) lds[L_ALPHA + col] = (float)(_Float16)o[0];
  }
  __syncthreads();
}

// inputs of evaluation j for the tcnn decoder: 17 features, padded to 32 with 1.0, f16
__device__ __forceinline__ void stage_input_t(float* __restrict__ lds, int j, const float (&loc)[3],
                                              const float (&feat)[8]) {
  float in[32];
  tcnn_sdf_inputs(loc, feat, in);
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) *(half8*)&lds[L_HL + ((ks * 2 + hh) * DM + j) * 4] = tcnn_input_frag(in, ks, hh);
  }
}

// F.grid_sample(mode="nearest", padding_mode="zeros", align_corners=True) of the TSDF prior at a
// corner given in voxel units (sparse_volume.py:820-829): coordinate a -> index along dims[a].
__device__ __forceinline__ float sample_delta(const bnv_sdf_delta_t& d, const bnv_grid_t& g, const float (&c)[3]) {
  int idx[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float t = __fdiv_rn(c[a], (float)(g.n_xyz[a] - 1));
    t = __fsub_rn(__fmul_rn(t, 2.f), 1.f);
    t = __fmul_rn(__fdiv_rn(__fadd_rn(t, 1.f), 2.f), (float)(d.dims[a] - 1));
    const float r = nearbyintf(t);
    if (!(r >= 0.f) || !(r <= (float)(d.dims[a] - 1))) return 0.f;
    idx[a] = (int)r;
  }
  return d.data[((size_t)idx[0] * d.dims[1] + idx[1]) * d.dims[2] + idx[2]];
}

}  // namespace bnv
