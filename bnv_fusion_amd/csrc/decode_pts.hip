// decode_pts.hip -- SparseVolume.decode_pts at arbitrary points (8 corner evaluations per point, reference
// sparse_volume.py:768-833) and its gradient with respect to the volume's features, on the MLP tile of sdf_mlp.hpp:
// k_decode_pts<PREC>, k_decode_pts_bwd, k_optim_step, k_decode_pts_bwd_t.
#include "decode_host.hpp"
#include "sdf_mlp.hpp"
#include "volume_keys.hpp"

namespace bnv {

// ---------------------------------------------------------------------------------------------------
// Arbitrary query points (SparseVolume.decode_pts, sparse_volume.py:768-833) with LIVE-QUERY COMPACTION.
// A query whose 8 corners are not all observed decodes to the constant voxel_size (:809, :818) without ever
// reading its MLP outputs; the ray samples of the global optimiser are ~90 % such free-space points, but
// spread so that nearly every run of 16 consecutive queries contains a live one.  The workgroup therefore
// first CLASSIFIES a chunk of 128 queries (1,024 corner look-ups by all 512 threads; masked queries are
// finished right there), compacts the live ones into an LDS list, and runs the MLP on tiles of 16 LIVE
// queries.  Shared by the forward kernel and the two backward kernels.
// ---------------------------------------------------------------------------------------------------
constexpr int PC_Q = 128;                         // queries per chunk
constexpr int C_ROW = L_TOTAL;                    // [1024] int   row of every (query, corner) or -1
constexpr int C_WN = C_ROW + PC_Q * 8;            // [1024] float trilinear weight / sum over the 8 corners
constexpr int C_DLT = C_WN + PC_Q * 8;            // [1024] float sdf_delta sample of the corner
constexpr int C_LIST = C_DLT + PC_Q * 8;          // [128]  int   chunk-local indices of the live queries
constexpr int C_CNT = C_LIST + PC_Q;              // [4]    int   number of live queries
constexpr int C_TOTAL = C_CNT + 4;                // 38,532 floats = 154,128 B

// corner k of query point c (voxel units): corner coordinates, local offset, trilinear weight
__device__ __forceinline__ float pts_corner(const DecodeArgs& A, int64_t q, int k, float (&corner)[3], float (&loc)[3]) {
  const int cb = kCornerCeilBits[k];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float c = A.coords[q * 3 + a];
    if (!A.is_coords) c = __fdiv_rn(__fsub_rn(c, A.grid.bound_min[a]), A.grid.voxel_size);  // (:793)
    corner[a] = ((cb >> a) & 1) ? ceilf(c) : floorf(c);
    loc[a] = __fsub_rn(c, corner[a]);
  }
  return __fmul_rn(__fmul_rn(1.f - fabsf(loc[0]), 1.f - fabsf(loc[1])), 1.f - fabsf(loc[2]));
}

// Classifies chunk `chunk`; returns the number of live queries (uniform).  Masked queries are finished here:
// masked(q, value) gets their final value (forward: written to A.out; fused optimiser step: their loss term); live
// ones are listed in C_LIST in ascending order.
template <class MaskedFn>
__device__ __forceinline__ int pts_classify_chunk_fn(const DecodeArgs& A, int64_t chunk, float* __restrict__ lds,
                                                     MaskedFn masked) {
  int* c_row = (int*)(lds + C_ROW);
  int* c_list = (int*)(lds + C_LIST);
  int* c_cnt = (int*)(lds + C_CNT);
  const float voxel = A.grid.voxel_size;
  if (threadIdx.x == 0) *c_cnt = 0;
  __syncthreads();
  unsigned live_bits = 0;  // lanes with k == 0: bit i set when this thread's i-th query is live
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int ce = it * 512 + threadIdx.x;  // (query, corner) index within the chunk
    const int64_t q = chunk * PC_Q + (ce >> 3);
    const int k = ce & 7;
    float wtri = 0.f, wvol = 0.f, dlt = 0.f;
    int row = -1;
    if (q < A.n) {
      float corner[3], loc[3];
      wtri = pts_corner(A, q, k, corner, loc);
      uint64_t key;
      if (pack_key((int64_t)corner[0], (int64_t)corner[1], (int64_t)corner[2], &key))
        row = volume_find(A.vol.slot_keys, A.vol.slot_rows, (uint32_t)(A.vol.n_slots - 1), key);
      if (row >= A.row_limit) row = -1;
      if (row >= 0) {
        wvol = A.weights[row];
        if (A.split_mask) {   // count_optim of the splits up to and including this query's, one exact +1 each
          uint32_t m = A.split_mask[row] & ((2u << (uint32_t)(q / A.split_samples)) - 1u);
          while (m) {
            wvol = __fadd_rn(wvol, 1.0f);
            m &= m - 1u;
          }
        }
      }
      if (A.delta.data) dlt = sample_delta(A.delta, A.grid, corner);
    }
    // the 8 corners of a query sit in 8 consecutive lanes: sums in corner order, like the reference's dim-1 sum
    float norm = 0.f, wmin = 3.4e38f;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      norm = __fadd_rn(norm, __shfl(wtri, (threadIdx.x & 56) + kk));
      wmin = fminf(wmin, __shfl(wvol, (threadIdx.x & 56) + kk));
    }
    const float wn = __fdiv_rn(wtri, norm);
    float dacc = 0.f;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) dacc = __fadd_rn(dacc, __shfl(__fmul_rn(dlt, wn), (threadIdx.x & 56) + kk));
    c_row[ce] = row;
    lds[C_WN + ce] = wn;
    lds[C_DLT + ce] = dlt;
    const bool live = q < A.n && wmin >= (float)A.grid.min_pts_in_grid;
    if (k == 0 && q < A.n) {
      if (live) {
        live_bits |= 1u << it;
      } else {
        float o = voxel;
        if (A.delta.data) o = __fadd_rn(o, dacc);
        masked(q, o);
      }
    }
  }
  // ordered compaction of the live queries (chunk-local index = ce >> 3): ballot per wave, wave offsets via LDS
  __shared__ int wave_cnt[2][8];
  const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
  unsigned long long b0 = __ballot(live_bits & 1u), b1 = __ballot(live_bits & 2u);
  if (ln == 0) {
    wave_cnt[0][wv] = __popcll(b0);
    wave_cnt[1][wv] = __popcll(b1);
  }
  __syncthreads();
  int base0 = 0, base1 = 0, tot0 = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (i < wv) {
      base0 += wave_cnt[0][i];
      base1 += wave_cnt[1][i];
    }
    tot0 += wave_cnt[0][i];
  }
  if (live_bits & 1u) c_list[base0 + __popcll(b0 & ((1ull << ln) - 1ull))] = threadIdx.x >> 3;
  if (live_bits & 2u) c_list[tot0 + base1 + __popcll(b1 & ((1ull << ln) - 1ull))] = 64 + (threadIdx.x >> 3);
  if (threadIdx.x == 511) {
    int t1 = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) t1 += wave_cnt[1][i];
    *c_cnt = tot0 + t1;
  }
  __syncthreads();
  return *c_cnt;
}

template <bool WRITE_MASKED>
__device__ __forceinline__ int pts_classify_chunk(const DecodeArgs& A, int64_t chunk, float* __restrict__ lds) {
  return pts_classify_chunk_fn(A, chunk, lds, [&](int64_t q, float o) {
    if (WRITE_MASKED) A.out[q] = o;
  });
}

// front end of one tile of 16 live queries: thread e < 128 = (live query e >> 3, corner e & 7)
template <int PREC>
__device__ __forceinline__ void pts_stage_tile(const DecodeArgs& A, int64_t chunk, int tile, int n_live,
                                               float* __restrict__ lds, int* __restrict__ row_out) {
  const int e = threadIdx.x;
  const int* c_row = (const int*)(lds + C_ROW);
  const int* c_list = (const int*)(lds + C_LIST);
  float loc[3] = {0.f, 0.f, 0.f};
  float feat[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float wn = 0.f, dlt = 0.f;
  int row = -1;
  const int li = tile * 16 + (e >> 3);
  if (li < n_live) {
    const int ql = c_list[li];
    const int ce = ql * 8 + (e & 7);
    float corner[3];
    pts_corner(A, chunk * PC_Q + ql, e & 7, corner, loc);
    row = c_row[ce];
    wn = lds[C_WN + ce];
    dlt = lds[C_DLT + ce];
    if (row >= 0) {
      const f32x4 f0 = *(const f32x4*)&A.features[(size_t)row * 8];
      const f32x4 f1 = *(const f32x4*)&A.features[(size_t)row * 8 + 4];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        feat[f] = f0[f];
        feat[4 + f] = f1[f];
      }
    }
  }
  if constexpr (PREC == 1 || PREC == 3) check_feature_range(feat, A.pack[SD_BA + 1], A.vol.n_rows);
  if constexpr (PREC == 2) stage_input_t(lds, e, loc, feat);
  else if constexpr (PREC == 1) stage_input_h<3>(lds, e, loc, feat);
  else if constexpr (PREC == 3) stage_input_h<1>(lds, e, loc, feat);
  else stage_input(lds + L_HL, e, loc, feat);
  lds[L_WTRI + e] = wn;
  lds[L_DELTA + e] = dlt;
  if (row_out) row_out[e] = row;
}

template <int PREC>
__global__ __launch_bounds__(512, 2) void k_decode_pts(DecodeArgs A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const float voxel = A.grid.voxel_size;
  const int64_t n_chunks = (A.n + PC_Q - 1) / PC_Q;
  for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
    const int n_live = pts_classify_chunk<true>(A, chunk, lds);
    for (int tile = 0; tile * 16 < n_live; ++tile) {
      if (threadIdx.x < DM) pts_stage_tile<PREC>(A, chunk, tile, n_live, lds, nullptr);
      __syncthreads();
      if constexpr (PREC == 2) sdf_mlp_tile_t(lds, A.pack);
      else if constexpr (PREC == 1) sdf_mlp_tile_h<3>(lds, A.pack);
      else if constexpr (PREC == 3) sdf_mlp_tile_h<1>(lds, A.pack);
      else sdf_mlp_tile(lds, A.pack);
      if (threadIdx.x < 16 && tile * 16 + threadIdx.x < n_live) {
        const int b = threadIdx.x * 8;
        float acc = 0.f, dacc = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float wk = lds[L_WTRI + b + k];
          float a = __fmul_rn(lds[L_ALPHA + b + k], voxel);
          if constexpr (PREC == 2) a = (float)(_Float16)a;  // half tensor * python float stays half (:813)
          acc = __fadd_rn(acc, __fmul_rn(a, wk));
          dacc = __fadd_rn(dacc, __fmul_rn(lds[L_DELTA + b + k], wk));
        }
        if (A.delta.data) acc = __fadd_rn(acc, dacc);
        A.out[chunk * PC_Q + ((const int*)(lds + C_LIST))[tile * 16 + threadIdx.x]] = acc;
      }
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// k_decode_pts_bwd: d(loss)/d(volume features) of k_decode<PTS> -- what the global optimiser needs
// (run_e2e.py:111-162 makes volume.features an nn.Parameter and back-propagates the ray loss of
// render_utils.py:461-560 through SparseVolume.decode_pts, sparse_volume.py:768-833).
// Only the features carry gradient (the decoder is frozen, the query points are data).
//
// Per 128-evaluation tile: the forward MLP is recomputed in split-f16 arithmetic keeping ONE BIT per
// pre-activation (z > 0) in registers -- the lane that owns z_l[feature][evaluation] in the forward D
// layout owns the same position of W_{l+1}^T delta_{l+1} in the backward pass, so the ReLU masks never
// leave the lane.  The backward pass is the same transposed-chaining MLP run on the transposed weight
// packs: delta_3 = wa * [z3 > 0]; delta_l = (W_{l+1}^T delta_{l+1}) * [z_l > 0]; g_in = W_0^T delta_0.
// It propagates d(alpha)/d(input) with a unit seed per evaluation, so its operands stay O(1) whatever the
// scale of the loss (an f16 split of 1e-7-sized loss gradients would underflow); the evaluation's
// incoming gradient go = grad_sdf[q] * voxel * w_k / sum(w) * [mask_q] multiplies the 8 feature rows of
// g_in in fp32 at the very end, followed by float atomics into grad_features[row].  Tiles whose 16
// queries are all masked (free space: most ray samples) skip the MLP altogether.
// ---------------------------------------------------------------------------------------------------
// mlp_layer_h with the weight fragments fetched by buffer loads (used where several layers' worth of
// hoisted flat addresses would not fit the register file)
template <int NKS, bool BIAS>
__device__ __forceinline__ void mlp_layer_hb(const _Float16* __restrict__ wp, const float* __restrict__ bias,
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
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)wp, 0, 8 * NKS * 2 * 64 * 8 * 2, 0x00020000);
  const int voff = lane * 16;
  const int sbase = w * NKS * 2 * 1024;
  const float* hh = lds + L_HL + (h * DM + j) * 4;
  const float* hl = lds + L_HLO + (h * DM + j) * 4;
  half8 ah[3], al[3], bh[2][4], bl[2][4];
#define BNV_LOAD_A(ks)                                                  \
  {                                                                     \
    ah[(ks) % 3] = load_frag(rs, voff, sbase + ((ks) * 2) * 1024);      \
    al[(ks) % 3] = load_frag(rs, voff, sbase + ((ks) * 2 + 1) * 1024);  \
  }
#define BNV_LOAD_B(ks)                                                                    \
  {                                                                                       \
    _Pragma("unroll") for (int pt = 0; pt < 4; ++pt) {                                    \
      bh[(ks) & 1][pt] = *(const half8*)(hh + ((ks) * 2 * DM + pt * 32) * 4);             \
      bl[(ks) & 1][pt] = *(const half8*)(hl + ((ks) * 2 * DM + pt * 32) * 4);             \
    }                                                                                     \
  }
  BNV_LOAD_A(0);
  if (NKS > 1) BNV_LOAD_A(1);
  BNV_LOAD_B(0);
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    if (ks + 2 < NKS) BNV_LOAD_A(ks + 2);
    if (ks + 1 < NKS) BNV_LOAD_B(ks + 1);
    __builtin_amdgcn_sched_barrier(0);
    const half8 a_hi = ah[ks % 3], a_lo = al[ks % 3];
#pragma unroll
    for (int pt = 0; pt < 4; ++pt)
      acc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo, bh[ks & 1][pt], acc[pt], 0, 0, 0);
#pragma unroll
    for (int pt = 0; pt < 4; ++pt)
      acc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, bl[ks & 1][pt], acc[pt], 0, 0, 0);
#pragma unroll
    for (int pt = 0; pt < 4; ++pt)
      acc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, bh[ks & 1][pt], acc[pt], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
#undef BNV_LOAD_A
#undef BNV_LOAD_B
}

constexpr int SB_W3T = 0;                          // [8 w][16 ks][2 hi/lo][64 lane][8]: W3^T
constexpr int SB_W2T = SB_W3T + 8 * 16 * 2 * 64 * 8;
constexpr int SB_W1T = SB_W2T + 8 * 16 * 2 * 64 * 8;
constexpr int SB_W0T = SB_W1T + 8 * 16 * 2 * 64 * 8;  // [16 ks][2][64][8]: W0^T, 17 rows padded to 32
constexpr int SB_TOTAL = SB_W0T + 16 * 2 * 64 * 8;    // 409,600 halves
constexpr int SB_PACK_FLOATS = SB_TOTAL / 2;

struct DecodeBwdArgs {
  DecodeArgs d;
  const float* bwd_pack;
  const float* grad_out;
  float* grad_features;
};

// bit (pt * 16 + r) = [acc[pt][r] > 0].  Built as a shift-or chain: with independent (cmp << k) terms the
// compiler keeps all 64 selected constants live and spills them.
__device__ __forceinline__ uint64_t positive_bits(const f32x16 (&acc)[4]) {
  uint32_t m[2] = {0u, 0u};
#pragma unroll
  for (int pt = 3; pt >= 0; --pt) {
#pragma unroll
    for (int r = 15; r >= 0; --r) m[pt >> 1] = (m[pt >> 1] << 1) | (uint32_t)(acc[pt][r] > 0.f);
  }
  return ((uint64_t)m[1] << 32) | m[0];
}

// acc <- acc where the bit is set, else 0, then split + store as the next layer's B operand
__device__ __forceinline__ void store_masked_h(float* __restrict__ lds, const f32x16 (&acc)[4], uint64_t m, int w,
                                               int j, int h) {
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
#pragma unroll
    for (int ksl = 0; ksl < 2; ++ksl) {
      half8 hi, lo;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float x = ((m >> (pt * 16 + 8 * ksl + e)) & 1) ? acc[pt][8 * ksl + e] : 0.f;
        const _Float16 t = (_Float16)x;
        hi[e] = t;
        lo[e] = (_Float16)(x - (float)t);
      }
      const int o = (((2 * w + ksl) * 2 + h) * DM + pt * 32 + j) * 4;
      *(half8*)&lds[L_HL + o] = hi;
      *(half8*)&lds[L_HLO + o] = lo;
    }
  }
}

// incoming gradient of evaluation e = threadIdx.x < 128 of a staged tile, into L_ALPHA:
// d out_q / d alpha_k = voxel * w_k / sum(w)
__device__ __forceinline__ void seed_grad(const DecodeBwdArgs& B, int64_t chunk, int tile, int n_live,
                                          float* __restrict__ lds) {
  const int li = tile * 16 + (threadIdx.x >> 3);
  float go = 0.f;
  if (li < n_live)
    go = B.grad_out[chunk * PC_Q + ((const int*)(lds + C_LIST))[li]] * B.d.grid.voxel_size * lds[L_WTRI + threadIdx.x];
  lds[L_ALPHA + threadIdx.x] = go;
}

// g_in = W0^T delta_0: 32 (17 used) x 128; wave w < 4 takes column block w
__device__ __forceinline__ f32x16 input_grad(const _Float16* __restrict__ pb, const float* __restrict__ lds, int w,
                                             int lane, int j, int h) {
  f32x16 g;
#pragma unroll
  for (int r = 0; r < 16; ++r) g[r] = 0.f;
  const _Float16* wl = pb + SB_W0T + lane * 8;
  const float* hh = lds + L_HL + (h * DM + w * 32 + j) * 4;
  const float* hl = lds + L_HLO + (h * DM + w * 32 + j) * 4;
#pragma unroll 4
  for (int ks = 0; ks < 16; ++ks) {
    const half8 a_hi = *(const half8*)(wl + (ks * 2) * 64 * 8);
    const half8 a_lo = *(const half8*)(wl + (ks * 2 + 1) * 64 * 8);
    const half8 b_hi = *(const half8*)(hh + ks * 2 * DM * 4);
    const half8 b_lo = *(const half8*)(hl + ks * 2 * DM * 4);
    g = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo, b_hi, g, 0, 0, 0);
    g = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_lo, g, 0, 0, 0);
    g = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_hi, g, 0, 0, 0);
  }
  return g;
}

// gf[f] += g_in[9 + f] * s for the 8 features of one evaluation.  D row (r&3) + 8 (r>>2) + 4 h is network input 9 + f
// for feature f: h = 0 holds f = 0, 1, 2 (r = 5, 6, 7) and f = 7 (r = 8); h = 1 holds f = 3..6 (r = 4..7)
__device__ __forceinline__ void scatter_feature_grad(float* __restrict__ gf, const f32x16& g, float s, int h) {
  if (h == 0) {
    unsafeAtomicAdd(gf + 0, g[5] * s);
    unsafeAtomicAdd(gf + 1, g[6] * s);
    unsafeAtomicAdd(gf + 2, g[7] * s);
    unsafeAtomicAdd(gf + 7, g[8] * s);
  } else {
    unsafeAtomicAdd(gf + 3, g[4] * s);
    unsafeAtomicAdd(gf + 4, g[5] * s);
    unsafeAtomicAdd(gf + 5, g[6] * s);
    unsafeAtomicAdd(gf + 6, g[7] * s);
  }
}

__global__ __launch_bounds__(512, 2) void k_decode_pts_bwd(DecodeBwdArgs B) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const DecodeArgs& A = B.d;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 31, h = lane >> 5;
  int* l_row = (int*)(lds + L_WVOL);
  const int64_t n_chunks = (A.n + PC_Q - 1) / PC_Q;
  for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
   const int n_live = pts_classify_chunk<false>(A, chunk, lds);
   for (int tile = 0; tile * 16 < n_live; ++tile) {
    // front end: 16 LIVE queries of the chunk; masked queries carry no gradient and were dropped above
    if (threadIdx.x < DM) {
      pts_stage_tile<1>(A, chunk, tile, n_live, lds, l_row);
      seed_grad(B, chunk, tile, n_live, lds);
    }
    __syncthreads();
    // launder the weight pointers once per tile: otherwise the bias / fc_alpha fragments (80 VGPRs) are
    // hoisted out of the tile loop as loop invariants and the MLP spills
    const float* pack = A.pack;
    const float* bpack = B.bwd_pack;
    asm volatile("" : "+s"(pack), "+s"(bpack));
    const _Float16* ph = (const _Float16*)(pack + SD_TOTAL);
    const _Float16* pb = (const _Float16*)bpack;
    // ---------------- forward, keeping the sign bits of the pre-activations ---------------------------
    f32x16 acc[4];
    mlp_layer_hb<2, true>(ph + SH_W0, pack + SD_B0, lds, acc, w, lane, j, h);
    const uint64_t m0 = positive_bits(acc);
    __syncthreads();
    store_relu_h(lds, acc, w, j, h);
    __syncthreads();
    mlp_layer_hb<16, true>(ph + SH_W1, pack + SD_B0 + 256, lds, acc, w, lane, j, h);
    const uint64_t m1 = positive_bits(acc);
    __syncthreads();
    store_relu_h(lds, acc, w, j, h);
    __syncthreads();
    mlp_layer_hb<16, true>(ph + SH_W2, pack + SD_B0 + 512, lds, acc, w, lane, j, h);
    const uint64_t m2 = positive_bits(acc);
    __syncthreads();
    store_relu_h(lds, acc, w, j, h);
    __syncthreads();
    mlp_layer_hb<16, true>(ph + SH_W3, pack + SD_B0 + 768, lds, acc, w, lane, j, h);
    // ---------------- backward with a unit seed: delta_3 = wa * [z3 > 0] ------------------------------
    {
      const uint64_t m3 = positive_bits(acc);
      const f32x16 wa = frag256(pack + SD_WA, w, h);
#pragma unroll
      for (int pt = 0; pt < 4; ++pt) acc[pt] = wa;
      __syncthreads();
      store_masked_h(lds, acc, m3, w, j, h);
    }
    __syncthreads();
    mlp_layer_hb<16, false>(pb + SB_W3T, nullptr, lds, acc, w, lane, j, h);
    __syncthreads();
    store_masked_h(lds, acc, m2, w, j, h);
    __syncthreads();
    mlp_layer_hb<16, false>(pb + SB_W2T, nullptr, lds, acc, w, lane, j, h);
    __syncthreads();
    store_masked_h(lds, acc, m1, w, j, h);
    __syncthreads();
    mlp_layer_hb<16, false>(pb + SB_W1T, nullptr, lds, acc, w, lane, j, h);
    __syncthreads();
    store_masked_h(lds, acc, m0, w, j, h);
    __syncthreads();
    if (w < 4) {
      const f32x16 g = input_grad(pb, lds, w, lane, j, h);
      const int col = w * 32 + j;
      const float s = lds[L_ALPHA + col];
      const int row = l_row[col];
      if (s != 0.f && row >= 0) scatter_feature_grad(B.grad_features + (size_t)row * 8, g, s, h);
    }
    __syncthreads();
   }
  }
}

// ---------------------------------------------------------------------------------------------------
// k_optim_step (round 6): ONE launch for what an optimiser step of the reference spends five forward and five
// backward decode_pts calls on (run_e2e.py:127-153: 5,000 rays in splits of 1,000; render_utils.py:461-590).
// The L1 ray loss is elementwise -- d loss / d pred_q = sign(pred_q - target_q) * weight_q / n_valid(split) -- so the
// gradient a query sends back is known as soon as ITS forward value is: the forward (which k_decode_pts_bwd
// recomputes anyway for the ReLU masks) yields pred, the loss term and the seed of the backward in the same tile,
// and the separate forward kernel, the loss kernel and the round trip of pred / grad through memory all go.  All
// splits of a step ride in one launch: the weight a mask decision sees is reconstructed per split from
// split_mask (DecodeArgs), so every decision is the one the split-by-split sequence takes; chunks of 128 queries
// are handed out dynamically (a ray split has < 1 tile of live queries per workgroup: five launches of each kernel
// left 3/4 of every launch's time to launch latency and one-tile rounds).  Arithmetic: the split-f16 forward /
// backward of k_decode_pts_bwd (fp32 checkpoints; SDF within 1e-8 of the exact-fp32 forward, gradients to 1e-6).
// ---------------------------------------------------------------------------------------------------
struct OptimArgs {
  DecodeBwdArgs b;          // b.d: the queries (coords = the step's samples, split_mask / split_samples); b.grad_features
  const float* target;      // [n]  L1 target of every sample (bnv_ray_samples)
  const float* wgt;         // [n]  valid x ray mask
  const float* n_valid;     // [n_splits]  sum of the split's ray masks + 1e-4 (render_utils.py:553)
  float* loss;              // [0] += sum over the splits of their losses; [1]: int32 chunk counter (zeroed by the caller)
  float* pred;              // optional [n]: the decoded SDF (tests, diagnostics)
};

__global__ __launch_bounds__(512) void k_optim_step(OptimArgs O) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const DecodeBwdArgs& B = O.b;
  const DecodeArgs& A = B.d;
  const float voxel = A.grid.voxel_size;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 31, h = lane >> 5;
  int* l_row = (int*)(lds + L_WVOL);
  __shared__ int s_chunk;
  __shared__ float s_red[8];
  const int64_t n_chunks = (A.n + PC_Q - 1) / PC_Q;
  float loss_acc = 0.f;
  auto loss_term = [&](int64_t q, float pred) -> float {      // -> d loss / d pred_q
    const float inv = 1.f / O.n_valid[A.split_samples > 0 ? q / A.split_samples : 0];
    const float wq = O.wgt[q] * inv;
    const float d = pred - O.target[q];
    loss_acc += fabsf(d) * wq;
    if (O.pred) O.pred[q] = pred;
    return d > 0.f ? wq : (d < 0.f ? -wq : 0.f);               // d|x|/dx with torch's sign(0) = 0
  };
  for (;;) {
    __syncthreads();                                           // (s_chunk of the round before has been read)
    if (threadIdx.x == 0) s_chunk = atomicAdd((int*)(O.loss + 1), 1);
    __syncthreads();
    const int64_t chunk = s_chunk;
    if (chunk >= n_chunks) break;
    const int n_live = pts_classify_chunk_fn(A, chunk, lds, [&](int64_t q, float o) { (void)loss_term(q, o); });
#if defined(BNV_OPTIM_PHASES) && BNV_OPTIM_PHASES == 1      // development probe (tools/optim_phases.sh): classification only
    continue;
#endif
    for (int tile = 0; tile * 16 < n_live; ++tile) {
      if (threadIdx.x < DM) pts_stage_tile<1>(A, chunk, tile, n_live, lds, l_row);
      __syncthreads();
      const float* pack = A.pack;
      const float* bpack = B.bwd_pack;
      asm volatile("" : "+s"(pack), "+s"(bpack));
      const _Float16* ph = (const _Float16*)(pack + SD_TOTAL);
      const _Float16* pb = (const _Float16*)bpack;
      // ---------------- forward, keeping the sign bits of the pre-activations ---------------------------
      // (the 256-wide layers are LOOPS, not three copies of the tile code each way: unrolled, the kernel's body is ~90 KB of
      // instructions against a 64 KB instruction cache, and every tile streamed all of it through the cache)
      constexpr int LAYER_HALVES = 8 * 16 * 2 * 64 * 8;
      static_assert(SH_W2 - SH_W1 == LAYER_HALVES && SH_W3 - SH_W2 == LAYER_HALVES, "forward layers are equally spaced");
      static_assert(SB_W2T - SB_W3T == LAYER_HALVES && SB_W1T - SB_W2T == LAYER_HALVES, "backward layers too");
      f32x16 acc[4];
      mlp_layer_hb<2, true>(ph + SH_W0, pack + SD_B0, lds, acc, w, lane, j, h);
      const uint64_t m0 = positive_bits(acc);
      uint64_t m1 = 0, m2 = 0;
      __syncthreads();
      store_relu_h(lds, acc, w, j, h);
      __syncthreads();
#pragma unroll 1
      for (int l = 1;; ++l) {
        mlp_layer_hb<16, true>(ph + SH_W1 + (l - 1) * LAYER_HALVES, pack + SD_B0 + 256 * l, lds, acc, w, lane, j, h);
        if (l == 3) break;
        const uint64_t m = positive_bits(acc);
        if (l == 1) m1 = m; else m2 = m;
        __syncthreads();
        store_relu_h(lds, acc, w, j, h);
        __syncthreads();
      }
      {
        // fc_alpha (the forward's last layer) and the backward's seed delta_3 = wa * [z3 > 0] from the same fragment
        const uint64_t m3 = positive_bits(acc);
        const f32x16 wa = frag256(pack + SD_WA, w, h);
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) {
          float sp = 0.f;
#pragma unroll
          for (int r = 0; r < 16; ++r) sp = fmaf(wa[r], relu_bits(acc[pt][r]), sp);
          lds[L_PART + (w * 2 + h) * DM + pt * 32 + j] = sp;
          acc[pt] = wa;
        }
        __syncthreads();                      // layer 3 has read its operands; the partial sums are in place
        store_masked_h(lds, acc, m3, w, j, h);
      }
      if (threadIdx.x < DM) {
        // evaluation e = (live query e >> 3, corner e & 7): alpha -> the query's SDF (sums in corner order, like the
        // forward kernel) -> its loss term -> the gradient every one of its 8 evaluations starts from
        const int e = threadIdx.x;
        float al = pack[SD_BA];
#pragma unroll
        for (int p = 0; p < 16; ++p) al += lds[L_PART + p * DM + e];
        const float wk = lds[L_WTRI + e];
        const float ak = __fmul_rn(__fmul_rn(al, voxel), wk);
        const float dk = __fmul_rn(lds[L_DELTA + e], wk);
        float sum = 0.f, dsum = 0.f;
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
          sum = __fadd_rn(sum, __shfl(ak, (e & 56) + kk));
          dsum = __fadd_rn(dsum, __shfl(dk, (e & 56) + kk));
        }
        if (A.delta.data) sum = __fadd_rn(sum, dsum);
        const int li = tile * 16 + (e >> 3);
        float go = 0.f;
        if (li < n_live) {
          const int64_t q = chunk * PC_Q + ((const int*)(lds + C_LIST))[li];
          float g = 0.f;
          if ((e & 7) == 0) g = loss_term(q, sum);
          g = __shfl(g, e & 56);
          go = g * voxel * wk;
        }
        lds[L_ALPHA + e] = go;
      }
      __syncthreads();
#if defined(BNV_OPTIM_PHASES) && BNV_OPTIM_PHASES == 2      // development probe: classification + forward + loss only
      continue;
#endif
      // ---------------- backward with a unit seed (as k_decode_pts_bwd) ---------------------------------
#pragma unroll 1
      for (int l = 0; l < 3; ++l) {
        mlp_layer_hb<16, false>(pb + SB_W3T + l * LAYER_HALVES, nullptr, lds, acc, w, lane, j, h);
        const uint64_t m = l == 0 ? m2 : (l == 1 ? m1 : m0);
        __syncthreads();
        store_masked_h(lds, acc, m, w, j, h);
        __syncthreads();
      }
#if defined(BNV_OPTIM_PHASES) && BNV_OPTIM_PHASES == 3      // development probe: ... + the three 256-wide backward layers
      continue;
#endif
      if (w < 4) {
        const f32x16 g = input_grad(pb, lds, w, lane, j, h);
        const int col = w * 32 + j;
        const float sg = lds[L_ALPHA + col];
        const int row = l_row[col];
#if defined(BNV_OPTIM_PHASES) && BNV_OPTIM_PHASES == 4      // development probe: everything but the gradient's atomics
        if (sg == 12345.f && row >= 0)
#else
        if (sg != 0.f && row >= 0)
#endif
          scatter_feature_grad(B.grad_features + (size_t)row * 8, g, sg, h);
      }
      __syncthreads();
    }
  }
  // the workgroup's share of the loss: one atomic
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) loss_acc += __shfl_xor(loss_acc, o);
  if (lane == 0) s_red[w] = loss_acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) t += s_red[i];
    if (t != 0.f) unsafeAtomicAdd(O.loss, t);
  }
}

// ---------------------------------------------------------------------------------------------------
// k_decode_pts_bwd_t: the same backward for the tiny-cuda-nn decoder (MLP mode 2; the reference's default
// checkpoint).  32 | 64 | 64 | 64 | 16, no bias, f16 operands, fp32 accumulate: one wave carries 32
// evaluations forward and backward in registers (waves 0..3 of the workgroup; no barriers inside).
// PARITY UNPINNED like the forward (tcnn's CUDA arithmetic cannot run here).  tcnn back-propagates in fp16
// with a loss scale; here the Jacobian d(alpha)/d(input) is propagated with a unit seed (f16 operands O(1),
// fp32 accumulation) and multiplied by the incoming gradient in fp32, which cannot underflow.
// Pack (halves): W2^T [2 mb][4 g][64][8] | W1^T [2 mb][4 g][64][8] | W0^T [4 g][64][8] | 128 halves holding
// row 0 of the output layer as 64 floats.
// ---------------------------------------------------------------------------------------------------
constexpr int TB_W2T = 0;
constexpr int TB_W1T = TB_W2T + 2 * 4 * 64 * 8;
constexpr int TB_W0T = TB_W1T + 2 * 4 * 64 * 8;
constexpr int TB_W3R = TB_W0T + 4 * 64 * 8;   // 64 floats
constexpr int TB_TOTAL = TB_W3R + 128;        // 10,368 halves = 5,184 floats

__global__ __launch_bounds__(512, 2) void k_decode_pts_bwd_t(DecodeBwdArgs B) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const DecodeArgs& A = B.d;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 31, h = lane >> 5;
  int* l_row = (int*)(lds + L_WVOL);
  const int64_t n_chunks = (A.n + PC_Q - 1) / PC_Q;
  for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
   const int n_live = pts_classify_chunk<false>(A, chunk, lds);
   for (int tile = 0; tile * 16 < n_live; ++tile) {
    // front end: 16 LIVE queries of the chunk; masked queries carry no gradient and were dropped above
    if (threadIdx.x < DM) {
      pts_stage_tile<2>(A, chunk, tile, n_live, lds, l_row);
      seed_grad(B, chunk, tile, n_live, lds);
    }
    __syncthreads();
    if (w < 4) {
      const _Float16* ph = (const _Float16*)A.pack;
      const _Float16* pb = (const _Float16*)B.bwd_pack;
      const int col = w * 32 + j;
      // ---- forward, keeping the sign bits of the three hidden pre-activations -------------------------
      half8 x[2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) x[ks] = *(const half8*)&lds[L_HL + ((ks * 2 + h) * DM + col) * 4];
      f32x16 a0[2], a1[2];
      half8 s[4];
      tcnn_first_layer<2>(ph + SdfPack::W0, lane, x, a0);
      const uint32_t m0 = positive_bits32(a0);
      tcnn_relu_round(a0, s);
      tcnn_hidden_layer(ph + SdfPack::W1, lane, s, a1);
      const uint32_t m1 = positive_bits32(a1);
      tcnn_relu_round(a1, s);
      tcnn_hidden_layer(ph + SdfPack::W2, lane, s, a0);
      const uint32_t m2 = positive_bits32(a0);
      // ---- backward with a unit seed: delta_2 = W3[0, :] * [z2 > 0] ------------------------------------
      {
        const float* w3r = (const float*)(pb + TB_W3R);
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
#pragma unroll
          for (int qd = 0; qd < 4; ++qd) {
            const f32x4 t = *(const f32x4*)&w3r[mb * 32 + 8 * qd + 4 * h];
#pragma unroll
            for (int i = 0; i < 4; ++i) a0[mb][4 * qd + i] = t[i];
          }
        }
      }
      auto fill_masked = [&](const f32x16 (&in)[2], uint32_t m) {
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
#pragma unroll
          for (int ksl = 0; ksl < 2; ++ksl) {
#pragma unroll
            for (int e = 0; e < 8; ++e)
              s[nb * 2 + ksl][e] = (_Float16)(((m >> (nb * 16 + ksl * 8 + e)) & 1u) ? in[nb][ksl * 8 + e] : 0.f);
          }
        }
      };
      fill_masked(a0, m2);
      tcnn_hidden_layer(pb + TB_W2T, lane, s, a1);
      fill_masked(a1, m1);
      tcnn_hidden_layer(pb + TB_W1T, lane, s, a0);
      fill_masked(a0, m0);
      const f32x16 g = tcnn_output_layer(pb + TB_W0T, lane, s);
      const float sc = lds[L_ALPHA + col];
      const int row = l_row[col];
      if (sc != 0.f && row >= 0) scatter_feature_grad(B.grad_features + (size_t)row * 8, g, sc, h);
    }
    __syncthreads();
   }
  }
}

int decode_pts_init() {
  int rc = BNV_OK;
  opt_in_lds(rc, (const void*)k_decode_pts_bwd, C_TOTAL * 4);
  opt_in_lds(rc, (const void*)k_decode_pts_bwd_t, C_TOTAL * 4);
  opt_in_lds(rc, (const void*)k_optim_step, C_TOTAL * 4);
  for (int mlp = 0; mlp < 4; ++mlp)
    dispatch_prec(mlp, [&](auto p) { opt_in_lds(rc, (const void*)k_decode_pts<decltype(p)::value>, C_TOTAL * 4); });
  return rc;
}

// the DecodeArgs of a call on query points (delta may be null; split_mask null: one split, plain weights)
static DecodeArgs pts_args(const bnv_volume_t* vol, const bnv_grid_t* grid, const float* features, const float* weights,
                           int64_t row_limit, const float* sdfmlp_pack, const float* coords, int64_t n, int is_coords,
                           const bnv_sdf_delta_t* delta, const uint32_t* split_mask, int64_t split_samples) {
  DecodeArgs a = {};
  a.split_mask = split_mask;
  a.split_samples = split_mask ? split_samples : 0;
  a.vol = *vol;
  a.grid = *grid;
  a.features = features;
  a.weights = weights;
  a.row_limit = row_limit;
  a.pack = sdfmlp_pack;
  a.coords = coords;
  a.n = n;
  a.is_coords = is_coords;
  if (delta) a.delta = *delta;
  return a;
}

// workgroups of a kernel that walks chunks of PC_Q queries: one per chunk, at most `cus`
static unsigned pts_grid(int64_t n, int64_t cus) {
  int64_t g = (n + PC_Q - 1) / PC_Q;
  if (g > cus) g = cus;
  return (unsigned)(g < 1 ? 1 : g);
}

}  // namespace bnv

using namespace bnv;

extern "C" {

// split_mask == NULL: one split (plain weights); else split_samples > 0 queries per split, at most 31 splits
static bool splits_ok(const uint32_t* split_mask, int64_t split_samples, int64_t n) {
  if (!split_mask) return true;
  return split_samples > 0 && (n + split_samples - 1) / split_samples <= 31;
}

int bnv_decode_pts(const bnv_volume_t* vol, const bnv_grid_t* grid, const float* features, const float* weights,
                   int64_t row_limit, const float* sdfmlp_pack, const float* coords, int64_t n, int is_coords,
                   const bnv_sdf_delta_t* delta, const uint32_t* split_mask, int64_t split_samples, float* out_sdf,
                   bnv_stream_t stream) {
  if (g_num_cus <= 0) return BNV_ERR_NOT_INITIALISED;
  if (!vol_ok_ro(vol) || !grid || !features || !weights || !sdfmlp_pack || n < 0) return BNV_ERR_INVALID_ARGUMENT;
  if (!mlp_mode_field_ok(grid->mlp_mode) || !splits_ok(split_mask, split_samples, n)) return BNV_ERR_INVALID_ARGUMENT;
  if (n == 0) return BNV_OK;
  if (!coords || !out_sdf) return BNV_ERR_INVALID_ARGUMENT;
  DecodeArgs a = pts_args(vol, grid, features, weights, row_limit, sdfmlp_pack, coords, n, is_coords, delta, split_mask,
                          split_samples);
  a.out = out_sdf;
  ProfScope prof(PROF_DECODE_PTS, (hipStream_t)stream);
  dispatch_prec(mlp_mode_of(grid->mlp_mode), [&](auto p) {
    hipLaunchKernelGGL((k_decode_pts<decltype(p)::value>), dim3(pts_grid(n, g_num_cus)), dim3(512), C_TOTAL * 4,
                       (hipStream_t)stream, a);
  });
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

size_t bnv_sdfmlp_bwd_pack_floats(void) { return SB_PACK_FLOATS; }
size_t bnv_sdfmlp_tcnn_bwd_pack_floats(void) { return TB_TOTAL / 2; }

int bnv_decode_pts_backward(const bnv_volume_t* vol, const bnv_grid_t* grid, const float* features,
                            const float* weights, int64_t row_limit, const float* sdfmlp_pack,
                            const float* sdfmlp_bwd_pack, const float* coords, int64_t n, int is_coords,
                            const uint32_t* split_mask, int64_t split_samples, const float* grad_sdf,
                            float* grad_features, bnv_stream_t stream) {
  if (g_num_cus <= 0) return BNV_ERR_NOT_INITIALISED;
  if (!vol_ok_ro(vol) || !grid || !features || !weights || !sdfmlp_pack || !sdfmlp_bwd_pack || n < 0 ||
      !mlp_mode_field_ok(grid->mlp_mode) || !splits_ok(split_mask, split_samples, n))
    return BNV_ERR_INVALID_ARGUMENT;
  if (n == 0) return BNV_OK;
  if (!coords || !grad_sdf || !grad_features) return BNV_ERR_INVALID_ARGUMENT;
  DecodeBwdArgs b = {};
  b.d = pts_args(vol, grid, features, weights, row_limit, sdfmlp_pack, coords, n, is_coords, nullptr, split_mask,
                 split_samples);
  b.bwd_pack = sdfmlp_bwd_pack;
  b.grad_out = grad_sdf;
  b.grad_features = grad_features;
  const dim3 nblk(pts_grid(n, g_num_cus));
  ProfScope prof(PROF_DECODE_PTS, (hipStream_t)stream);
  if (mlp_mode_of(grid->mlp_mode) == 2)
    hipLaunchKernelGGL(k_decode_pts_bwd_t, nblk, dim3(512), C_TOTAL * 4, (hipStream_t)stream, b);
  else
    hipLaunchKernelGGL(k_decode_pts_bwd, nblk, dim3(512), C_TOTAL * 4, (hipStream_t)stream, b);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

int bnv_optim_step(const bnv_volume_t* vol, const bnv_grid_t* grid, const float* features, const float* weights,
                   int64_t row_limit, const float* sdfmlp_pack, const float* sdfmlp_bwd_pack, const float* pts,
                   int64_t n, int is_coords, const bnv_sdf_delta_t* delta, const uint32_t* split_mask,
                   int64_t split_samples, const float* target, const float* sample_weight, const float* n_valid,
                   float* loss_and_counter, float* pred, float* grad_features, bnv_stream_t stream) {
  if (g_num_cus <= 0) return BNV_ERR_NOT_INITIALISED;
  if (!vol_ok_ro(vol) || !grid || !features || !weights || !sdfmlp_pack || !sdfmlp_bwd_pack || n < 0 ||
      !mlp_mode_field_ok(grid->mlp_mode) || !splits_ok(split_mask, split_samples, n))
    return BNV_ERR_INVALID_ARGUMENT;
  // the fused kernel is the split-f16 forward + backward of the fp32 decoder (modes 1 / 3 / 0 share it as
  // bnv_decode_pts_backward does); the tiny-cuda-nn decoder keeps its separate kernels
  if (mlp_mode_of(grid->mlp_mode) == 2) return BNV_ERR_INVALID_ARGUMENT;
  if (n == 0) return BNV_OK;
  if (!pts || !target || !sample_weight || !n_valid || !loss_and_counter || !grad_features) return BNV_ERR_INVALID_ARGUMENT;
  OptimArgs o = {};
  o.b.d = pts_args(vol, grid, features, weights, row_limit, sdfmlp_pack, pts, n, is_coords, delta, split_mask,
                   split_samples);
  o.b.bwd_pack = sdfmlp_bwd_pack;
  o.b.grad_features = grad_features;
  o.target = target;
  o.wgt = sample_weight;
  o.n_valid = n_valid;
  o.loss = loss_and_counter;
  o.pred = pred;
  const dim3 nblk(pts_grid(n, g_num_cus - g_reserve_cus.load(std::memory_order_relaxed)));
  ProfScope prof(PROF_DECODE_PTS, (hipStream_t)stream);
  hipLaunchKernelGGL(k_optim_step, nblk, dim3(512), C_TOTAL * 4, (hipStream_t)stream, o);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

}  // extern "C"
