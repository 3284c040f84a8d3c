// decode.hip -- SDF decode (reference sparse_volume.py:768-833, local_point_fusion.py:265-379,
// modules.py:81-123,657-662) on gfx950: the TABLE kernels.  The MLP tile they run is sdf_mlp.hpp.
//   LATTICE  per-voxel table g[row][27] = MLP(enc(l), feat[row]) * voxel, l in {-.5,0,.5}^3 --
//            on the 3x3x3 meshing lattice every (point, corner) input is one of those 27 per
//            corner voxel, so the MLP runs 27x per corner voxel instead of 216x per voxel
//            (k_decode<LATTICE>, k_lattice_table_x, k_lattice_table_t; the bookkeeping around them: lattice.hip);
//   DENSE    decode_feature_grid_w_pts on dense grids (k_decode<DENSE / DENSE1>).
// Decode at arbitrary points (PTS) and its gradient: decode_pts.hip.
#include <string.h>

#include "decode_host.hpp"
#include "sdf_mlp.hpp"

namespace bnv {

#ifdef BNV_PHASE_PROF
__device__ unsigned long long g_phase_cycles[8 * 32];   // BNV_PH / BNV_PHX, read by bnv_dev_phase_read
#endif

template <int MODE, int PREC>
__global__ __launch_bounds__(512, 2) void k_decode(DecodeArgs A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* hl = lds + L_HL;
  const float voxel = A.grid.voxel_size;
  int64_t n_tiles;
  int64_t n_evals = 0;
  if constexpr (MODE == MODE_LATTICE) {
    n_evals = A.entries ? (int64_t)A.n_list[1] : (int64_t)(*A.n_list) * 27;
    n_tiles = (n_evals + DM - 1) / DM;
  } else if constexpr (MODE == MODE_DENSE1) {
    n_tiles = (A.n + DM - 1) / DM;
  } else {
    n_tiles = (A.n + 15) / 16;
  }
#ifdef BNV_PHASE_PROF
  if (threadIdx.x < 256) ((unsigned long long*)(lds + L_PROF))[threadIdx.x] = 0;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) ((unsigned long long*)(lds + L_PROF))[(threadIdx.x >> 6) * 32 + 31] = clock64();
#endif
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    // ---------------- front end: one thread per MLP input ---------------------------------
    if (threadIdx.x < DM) {
      const int j = threadIdx.x;
      float loc[3] = {0.f, 0.f, 0.f};
      float feat[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      float wtri = 0.f, wvol = 0.f, dlt = 0.f;
      if constexpr (MODE == MODE_LATTICE) {
        const int64_t e = tile * DM + j;
        if (e < n_evals) {
          int row, l;
          if (A.entries) {
            const int ent = A.entries[e];
            row = ent >> 5;
            l = ent & 31;
          } else {
            const int64_t ci = e / 27;
            l = (int)(e - ci * 27);
            row = A.list[ci];
          }
          loc[0] = (float)(l / 9 - 1) * 0.5f;
          loc[1] = (float)((l / 3) % 3 - 1) * 0.5f;
          loc[2] = (float)(l % 3 - 1) * 0.5f;
          const f32x4 f0 = *(const f32x4*)&A.features[(size_t)row * 8];
          const f32x4 f1 = *(const f32x4*)&A.features[(size_t)row * 8 + 4];
#pragma unroll
          for (int f = 0; f < 4; ++f) {
            feat[f] = f0[f];
            feat[4 + f] = f1[f];
          }
        }
      } else if constexpr (MODE == MODE_DENSE1) {
        const int64_t q = tile * DM + j;
        if (q < A.n) {
          const size_t plane = (size_t)A.dims[0] * A.dims[1] * A.dims[2];
          float c[3];
#pragma unroll
          for (int a = 0; a < 3; ++a) c[a] = A.coords[q * 3 + a];
          if (A.variant == 0) {
            // nearest voxel, one evaluation (local_point_fusion.py:288-292, 331-343): torch.round = half to even
            int v[3];
            bool in = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
              const float r = rintf(c[a]);
              // relative_xyz = rel * voxel; decode_implicit divides it by voxel again (:335,:374)
              loc[a] = __fdiv_rn(__fmul_rn(__fsub_rn(c[a], r), voxel), voxel);
              in = in && r >= 0.f && r <= (float)(A.dims[a] - 1);
              v[a] = (int)r;
            }
            if (in) {
              const size_t o = ((size_t)v[0] * A.dims[1] + v[1]) * A.dims[2] + v[2];
#pragma unroll
              for (int f = 0; f < 8; ++f) feat[f] = A.feat_grid[f * plane + o];
              wvol = A.pts_weight[o];
            }
          } else {
            // global coordinates (:345-367): features by trilinear grid_sample (align_corners, zero padding: the
            // order of torch's grid_sampler_3d, x = last axis), weight by nearest; the MLP sees coords / (res - 1)
            float u[3], fl[3];
            bool near_in = true;
            int nr[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
              const float t = __fdiv_rn(c[a], (float)(A.dims[a] - 1));
              loc[a] = t;
              const float gs = __fsub_rn(__fmul_rn(t, 2.f), 1.f);
              u[a] = __fmul_rn(__fdiv_rn(__fadd_rn(gs, 1.f), 2.f), (float)(A.dims[a] - 1));
              fl[a] = floorf(u[a]);
              const float r = nearbyintf(u[a]);
              near_in = near_in && r >= 0.f && r <= (float)(A.dims[a] - 1);
              nr[a] = (int)r;
            }
            if (near_in) wvol = A.pts_weight[((size_t)nr[0] * A.dims[1] + nr[1]) * A.dims[2] + nr[2]];
#pragma unroll
            for (int k = 0; k < 8; ++k) {   // tnw, tne, tsw, tse, bnw, bne, bsw, bse: bit 0 = x (axis 2), 1 = y, 2 = z (axis 0)
              const int d0 = (k >> 2) & 1, d1 = (k >> 1) & 1, d2 = k & 1;
              const float p0 = fl[0] + (float)d0, p1 = fl[1] + (float)d1, p2 = fl[2] + (float)d2;
              // weight of a corner = product over axes of (opposite corner - u) or (u - opposite corner)
              const float w2 = d2 ? __fsub_rn(u[2], fl[2]) : __fsub_rn(fl[2] + 1.f, u[2]);
              const float w1 = d1 ? __fsub_rn(u[1], fl[1]) : __fsub_rn(fl[1] + 1.f, u[1]);
              const float w0 = d0 ? __fsub_rn(u[0], fl[0]) : __fsub_rn(fl[0] + 1.f, u[0]);
              const float wk = __fmul_rn(__fmul_rn(w2, w1), w0);
              if (p0 >= 0.f && p1 >= 0.f && p2 >= 0.f && p0 <= (float)(A.dims[0] - 1) &&
                  p1 <= (float)(A.dims[1] - 1) && p2 <= (float)(A.dims[2] - 1)) {
                const size_t o = ((size_t)(int)p0 * A.dims[1] + (int)p1) * A.dims[2] + (int)p2;
#pragma unroll
                for (int f = 0; f < 8; ++f) feat[f] = __fadd_rn(feat[f], __fmul_rn(A.feat_grid[f * plane + o], wk));
              }
            }
          }
          if (A.nf_out) {
#pragma unroll
            for (int f = 0; f < 8; ++f) A.nf_out[q * 8 + f] = feat[f];
          }
        }
      } else {
        const int64_t q = tile * 16 + (j >> 3);
        const int cb = kCornerCeilBits[j & 7];
        if (q < A.n) {
          float c[3], corner[3];
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            c[a] = A.coords[q * 3 + a];
            corner[a] = ((cb >> a) & 1) ? ceilf(c[a]) : floorf(c[a]);
            loc[a] = __fsub_rn(c[a], corner[a]);
          }
          wtri = __fmul_rn(__fmul_rn(1.f - fabsf(loc[0]), 1.f - fabsf(loc[1])), 1.f - fabsf(loc[2]));
          {  // MODE_DENSE: nearest gather == direct index, zero outside (:296-310)
            const int x = (int)corner[0], y = (int)corner[1], z = (int)corner[2];
            if (x >= 0 && y >= 0 && z >= 0 && x < A.dims[0] && y < A.dims[1] && z < A.dims[2]) {
              const size_t plane = (size_t)A.dims[0] * A.dims[1] * A.dims[2];
              const size_t o = ((size_t)x * A.dims[1] + y) * A.dims[2] + z;
#pragma unroll
              for (int f = 0; f < 8; ++f) feat[f] = A.feat_grid[f * plane + o];
              wvol = A.pts_weight[o];
            }
            // relative_xyz = rel * voxel; decode_implicit divides it by voxel again (:321,:374)
#pragma unroll
            for (int a = 0; a < 3; ++a) loc[a] = __fdiv_rn(__fmul_rn(loc[a], voxel), voxel);
          }
        }
      }
      if constexpr (PREC == 1 || PREC == 3)
        check_feature_range(feat, A.pack[SD_BA + 1], (MODE == MODE_DENSE || MODE == MODE_DENSE1) ? A.status : A.vol.n_rows);
      if constexpr (PREC == 2) stage_input_t(lds, j, loc, feat);
      else if constexpr (PREC == 1) stage_input_h<3>(lds, j, loc, feat);
      else if constexpr (PREC == 3) stage_input_h<1>(lds, j, loc, feat);
      else stage_input(hl, j, loc, feat);
      lds[L_WTRI + j] = wtri;
      lds[L_WVOL + j] = wvol;
      lds[L_DELTA + j] = dlt;
    }
    // ---------------- MLP -----------------------------------------------------------------
    BNV_PH(0);
    __syncthreads();
    BNV_PH(18);
    if constexpr (PREC == 2) sdf_mlp_tile_t(lds, A.pack);
    else if constexpr (PREC == 1) sdf_mlp_tile_h<3>(lds, A.pack);
    else if constexpr (PREC == 3) sdf_mlp_tile_h<1>(lds, A.pack);
    else sdf_mlp_tile(lds, A.pack);
    // ---------------- back end ------------------------------------------------------------
    if constexpr (MODE == MODE_LATTICE) {
      if (threadIdx.x < DM) {
        const int64_t e = tile * DM + threadIdx.x;
        if (e < n_evals) {
          int row, l;
          if (A.entries) {
            const int ent = A.entries[e];
            row = ent >> 5;
            l = ent & 31;
            if (A.need_mask) A.need_mask[row] = 0u;  // leave the per-row masks clean for the next call
          } else {
            const int64_t ci = e / 27;
            l = (int)(e - ci * 27);
            row = A.list[ci];
          }
          float av = __fmul_rn(lds[L_ALPHA + threadIdx.x], voxel);
          if constexpr (PREC == 2) av = (float)(_Float16)av;  // half tensor * python float stays half (sparse_volume.py:813)
          A.table[(size_t)row * 27 + l] = av;
        }
      }
    } else if constexpr (MODE == MODE_DENSE1) {
      if (threadIdx.x < DM) {
        const int64_t q = tile * DM + threadIdx.x;
        if (q < A.n) {
          const float wv = lds[L_WVOL + threadIdx.x];
          const bool ok = wv >= (float)A.grid.min_pts_in_grid;
          float a = lds[L_ALPHA + threadIdx.x];
          // nearest: decode_implicit(normalize=True) scales by voxel; global: normalize=False, the raw prediction
          if (A.variant == 0) {
            a = __fmul_rn(a, voxel);
            if constexpr (PREC == 2) a = (float)(_Float16)a;
          }
          A.out[q] = ok ? a : voxel;   // forward_with_mask zero + valid_mask (:340-343) / valid_mask (:365-366)
        }
      }
    } else {
      if (threadIdx.x < 16) {
        const int64_t q = tile * 16 + threadIdx.x;
        if (q < A.n) {
          const int b = threadIdx.x * 8;
          float norm = 0.f;
#pragma unroll
          for (int k = 0; k < 8; ++k) norm = __fadd_rn(norm, lds[L_WTRI + b + k]);
          float acc = 0.f, dacc = 0.f, wmin = 3.4e38f, wsum = 0.f;
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const float wk = __fdiv_rn(lds[L_WTRI + b + k], norm);
            const float wv = lds[L_WVOL + b + k];
            float a = __fmul_rn(lds[L_ALPHA + b + k], voxel);
            if constexpr (PREC == 2) a = (float)(_Float16)a;
            if constexpr (MODE == MODE_DENSE) {
              const bool ok = wv >= (float)A.grid.min_pts_in_grid;  // forward_with_mask (modules.py:774-783)
              a = ok ? a : 0.f;
              wsum = __fadd_rn(wsum, ok ? wv : 0.f);
            }
            acc = __fadd_rn(acc, __fmul_rn(a, wk));
            dacc = __fadd_rn(dacc, __fmul_rn(lds[L_DELTA + b + k], wk));
            wmin = fminf(wmin, wv);
          }
          (void)dacc;
          (void)wmin;
          A.out[q] = (wsum > 0.f) ? acc : voxel;  // MODE_DENSE: any corner valid (:328-329)
        }
      }
    }
    BNV_PH(17);
    __syncthreads();
    BNV_PH(19);
  }
#ifdef BNV_PHASE_PROF
  __syncthreads();
  if (threadIdx.x < 256 && (threadIdx.x & 31) != 31)
    atomicAdd(&g_phase_cycles[threadIdx.x], ((unsigned long long*)(lds + L_PROF))[threadIdx.x]);
  if (threadIdx.x == 0) atomicAdd(&g_phase_cycles[31], 1ull);
#endif
}

// ---------------------------------------------------------------------------------------------------
// The lattice-table kernel of the split-operand modes (k_lattice_table_x below) is software-pipelined ACROSS
// tiles and layers.  Same arithmetic as k_decode<LATTICE, 1>, in another summation grouping (tables equal to
// ~1e-8); what changes is when things are fetched:
//  * the work-list entry of tile t+2 and the features of tile t+1 are loaded while tile t runs its MLP;
//    the inputs of tile t+1 are split and staged into a separate LDS buffer (PARK) in the shadow of layer
//    0's store phase, and layer 0 reads its B operands from PARK -- no gather on the critical path;
//  * the weight-fragment ring runs continuously through the 50 units of a tile and on into the next
//    tile: the first fragments of layer L+1 are requested during the last units of layer L, so they
//    arrive during the convert/store phase and its barriers;
//  * sin / cos of the lattice offsets {-.5, 0, .5} are two constants; the final reduction writes the table
//    directly; 7 barriers per tile.
// (Round 1's and 2's version of this kernel on v_mfma_f32_32x32x16_f16, k_lattice_table_h, is in the git history
// up to commit c19da39: bit-identical to k_decode<LATTICE, 1>, 5 % slower than the 16x16x32 form.)
// ---------------------------------------------------------------------------------------------------
constexpr int T_PARK_HI = L_PART + 16 * DM;            // [4 octets][128 evaluations][8 halves] = 8 KB
constexpr int T_PARK_LO = T_PARK_HI + 2 * 2 * DM * 4;  // lo plane
constexpr int T_TOTAL = T_PARK_LO + 2 * 2 * DM * 4;    // 38,912 floats = 155,648 B
constexpr int kTRing = 5, kTAhead = 3;                 // 50 units per tile: 50 % 5 == 0 keeps the ring phase

struct ARing {
  half8 hi[kTRing], lo[kTRing];
};

// (row, l) of evaluation e of the work list, or row = -1 beyond its end
__device__ __forceinline__ int lattice_entry(const DecodeArgs& A, int64_t e, int64_t n_evals) {
  if (e >= n_evals) return -1;
  if (A.entries) return A.entries[e];
  const int64_t ci = e / 27;
  return (A.list[ci] << 5) | (int)(e - ci * 27);
}

// ---------------------------------------------------------------------------------------------------
// k_lattice_table_x: the same tables on v_mfma_f32_16x16x32_f16.
// Both MLP kernels run at the package power limit (tools/power_probe.py), and under that limit the 16x16x32 form
// delivers ~14 % more FLOP/s than the 32x32x16 form (tools/probe_shapes.hip: 1.88 against 1.65 PFLOP/s with random
// f16 operands, MFMA-only streams): half the accumulator traffic per FLOP.  Same tile (128 evaluations), same
// split arithmetic (three products, fp32 accumulation), same bytes from L2 and LDS; what changes is the shape of
// a wave's work and therefore every layout:
//  * wave w still owns output features [32 w, 32 w + 32) of every layer for all 128 evaluations: 2 row blocks
//    (rb) of 16 features x 8 column blocks (cb) of 16 evaluations = 16 accumulators of 4 registers.  Lane
//    (n = l & 15, g = l >> 4), register i of acc[rb][cb] is feature 32 w + 16 rb + 4 g + i of evaluation 16 cb + n;
//  * a K-step is 32 deep: operand slot jj of a lane of K-group g is K index 8 g + jj.  The activations live in LDS
//    as OCTETS [32 octets][128 evaluations][8 halves] (hi plane, lo plane 64 KB behind): octet 4 s + g of K-step
//    s.  A lane's 8 registers {acc[0][cb][0..3], acc[1][cb][0..3]} are exactly one octet (4 w + g) of the next
//    layer's input, so the epilogue is again one ds_write_b128 per plane and column block, and K-step s of the
//    next layer consumes what wave s produced: slot jj <-> feature 32 s + 16 (jj >> 2) + 4 g + (jj & 3).  The weight
//    fragments are packed to that order on the host (weights.py: _pack_split16; SX_* below);
//  * one UNIT = half a K-step = 24 MFMAs of 16 cycles = the 384 cycles of a 32x32x16 K-step, so the weight ring
//    (5 units of one hi + one lo fragment, 3 ahead, 50 units per tile) and the activation double buffer carry
//    over unchanged (chain_layer_x).
// ---------------------------------------------------------------------------------------------------
constexpr int SX_W0 = 0;                              // [8 w][2 units][2 hi/lo][64 lane][8]
constexpr int SX_W1 = SX_W0 + 8 * 2 * 2 * 64 * 8;     // [8 w][16 units][2 hi/lo][64 lane][8]
constexpr int SX_W2 = SX_W1 + 8 * 16 * 2 * 64 * 8;
constexpr int SX_W3 = SX_W2 + 8 * 16 * 2 * 64 * 8;
constexpr int SX_TOTAL = SX_W3 + 8 * 16 * 2 * 64 * 8;  // 409,600 halves, behind the SH_* pack
static_assert(SX_TOTAL == SH_TOTAL, "16x16x32 pack size");
constexpr int SD_PACK_FLOATS_X = SD_PACK_FLOATS + SX_TOTAL / 2;

typedef __attribute__((address_space(3))) const half8 lds_half8_t;
typedef __attribute__((address_space(3))) half8 lds_half8_w_t;

// One layer.  NU = units of this layer (2 for layer 0, 16 for the others), BASE = units before it within the tile
// (ring phase).  A WEIGHT unit is (K-step s, row block rb), index 2 s + rb: one hi + one lo fragment; a COMPUTE unit
// is (K-step s, column half ch), index 2 s + ch: both row blocks x 4 column blocks x 3 products = 24 MFMAs, reading
// both weight units of its K-step and 4 + 4 activation fragments.  The ring holds weight units 0 .. kTAhead-1 on
// entry; compute unit u requests weight unit u + kTAhead (the last ones those of the NEXT layer) and the activation
// fragments of compute unit u + 1 (double buffer) -- per unit 24 MFMAs, 8 LDS reads, 2 L2 reads, like a K-step of
// the 32x32x16 kernel.  b_hi / b_lo: this lane's LDS byte address of octet g, evaluation n in the source planes.
// HALF: a 64-evaluation tile (the tail of a launch, k_lattice_table_x): only the compute units of column half 0 run;
// the weight ring keeps its schedule (every weight unit is still needed), the activation fragments of K-step s + 1
// are requested during K-step s.
template <int NU, int BASE, int NEXT_NU, int NPROD, bool HALF = false>
__device__ __forceinline__ void chain_layer_x(__amdgpu_buffer_rsrc_t rs, int voff, int off, int off_next,
                                              const float* __restrict__ bias, uint32_t b_hi, uint32_t b_lo,
                                              ARing& ring, f32x4 (&acc)[2][8], int w, int g) {
  const f32x4 bias0 = *(const f32x4*)&bias[32 * w + 4 * g];
  const f32x4 bias1 = *(const f32x4*)&bias[32 * w + 16 + 4 * g];
#pragma unroll
  for (int cb = 0; cb < 8; ++cb) {
    acc[0][cb] = bias0;
    acc[1][cb] = bias1;
  }
  const int sl = off + w * NU * 2048;
  const int sn = off_next + w * NEXT_NU * 2048;
  half8 bh[2][4], bl[2][4];
#define BNV_LOAD_B(u)                                                                                         \
  {                                                                                                           \
    _Pragma("unroll") for (int c = 0; c < 4; ++c) {                                                           \
      const uint32_t o = (uint32_t)(((u) >> 1) * 8192 + (((u) & 1) * 4 + c) * 256);                           \
      bh[(u) & 1][c] = *(lds_half8_t*)(b_hi + o);                                                             \
      if (NPROD == 3) bl[(u) & 1][c] = *(lds_half8_t*)(b_lo + o);                                             \
    }                                                                                                         \
  }
#define BNV_LOAD_BH(s_)                                                                                       \
  {                                                                                                           \
    _Pragma("unroll") for (int c = 0; c < 4; ++c) {                                                           \
      const uint32_t o = (uint32_t)((s_) * 8192 + c * 256);                                                   \
      bh[(s_) & 1][c] = *(lds_half8_t*)(b_hi + o);                                                            \
      if (NPROD == 3) bl[(s_) & 1][c] = *(lds_half8_t*)(b_lo + o);                                            \
    }                                                                                                         \
  }
  if constexpr (HALF) {
    BNV_LOAD_BH(0);
  } else {
    BNV_LOAD_B(0);
  }
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int s = u >> 1, ch = u & 1;
    const int nx = u + kTAhead;   // the weight unit requested during this compute unit
    bool loads_a = false;
    if (nx < NU) {
      ring.hi[(BASE + nx) % kTRing] = load_frag(rs, voff, sl + nx * 2048);
      if (NPROD == 3) ring.lo[(BASE + nx) % kTRing] = load_frag(rs, voff, sl + nx * 2048 + 1024);
      loads_a = true;
    } else if (nx - NU < NEXT_NU && nx - NU < kTAhead) {
      ring.hi[(BASE + nx) % kTRing] = load_frag(rs, voff, sn + (nx - NU) * 2048);
      if (NPROD == 3) ring.lo[(BASE + nx) % kTRing] = load_frag(rs, voff, sn + (nx - NU) * 2048 + 1024);
      loads_a = true;
    }
    if constexpr (HALF) {
      if (ch == 1) {   // nothing to compute in this unit of a half tile; its weight request stays
        __builtin_amdgcn_sched_barrier(0);
        continue;
      }
      if (2 * (s + 1) < NU) BNV_LOAD_BH(s + 1);
    } else {
      if (u + 1 < NU) BNV_LOAD_B(u + 1);
    }
    const int bb = HALF ? (s & 1) : (u & 1);
    if constexpr (NPROD == 3) {
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int c = 0; c < 4; ++c)
          acc[rb][4 * ch + c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ring.hi[(BASE + 2 * s + rb) % kTRing], bl[bb][c],
                                                                       acc[rb][4 * ch + c], 0, 0, 0);
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int c = 0; c < 4; ++c)
          acc[rb][4 * ch + c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ring.lo[(BASE + 2 * s + rb) % kTRing], bh[bb][c],
                                                                       acc[rb][4 * ch + c], 0, 0, 0);
    }
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int c = 0; c < 4; ++c)
        acc[rb][4 * ch + c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ring.hi[(BASE + 2 * s + rb) % kTRing], bh[bb][c],
                                                                     acc[rb][4 * ch + c], 0, 0, 0);
    // issue order: every prefetch in the shadow of an MFMA (one memory instruction behind each)
    if (HALF ? (2 * (s + 1) < NU) : (u + 1 < NU)) {
#pragma unroll
      for (int q = 0; q < (NPROD == 3 ? 8 : 4); ++q) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // 1 DS read
      }
    }
    if (loads_a) {
#pragma unroll
      for (int q = 0; q < (NPROD == 3 ? 2 : 1); ++q) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // 1 VMEM read
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
#undef BNV_LOAD_BH
#undef BNV_LOAD_B
}

// ReLU + hi/lo split of a wave's 32 features x 128 evaluations into octet 4 w + g of the activation planes, one
// column block at a time (conversion and ds_write_b128 interleaved), BEHIND the barrier that frees the planes.
// (Converting before that barrier -- the older wave of a SIMD wins MFMA arbitration and leaves the K-loop ~6,000
// cycles early, tools/phase_prof.py -- was measured: its VALU stream then takes issue slots from the younger
// wave's MFMAs and the tile gets 2.6 % longer; converting all blocks before the first store: +1.7 %.)
template <int NPROD, bool HALF = false>
__device__ __forceinline__ void store_relu_x(uint32_t st_hi, uint32_t st_lo, const f32x4 (&acc)[2][8]) {
#pragma unroll
  for (int cb = 0; cb < (HALF ? 4 : 8); ++cb) {
    half8 hi, lo;
    float x[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = relu1(acc[e >> 2][cb][e & 3]);
    if (NPROD == 3) {
      split8_f16(x, hi, lo);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) hi[e] = (_Float16)x[e];
    }
    *(lds_half8_w_t*)(st_hi + (uint32_t)(cb * 256)) = hi;
    if (NPROD == 3) *(lds_half8_w_t*)(st_lo + (uint32_t)(cb * 256)) = lo;
  }
}

#ifdef BNV_PHASE_PROF
#define BNV_PHX(i)                                                                 \
  do {                                                                             \
    if ((threadIdx.x & 63) == 0) {                                                 \
      unsigned long long* _p = (unsigned long long*)(lds + T_TOTAL) + (threadIdx.x >> 6) * 32; \
      const unsigned long long _t = clock64();                                     \
      _p[i] += _t - _p[31];                                                        \
      _p[31] = _t;                                                                 \
    }                                                                              \
  } while (0)
#else
#define BNV_PHX(i)
#endif

template <int NPROD>
__global__ __launch_bounds__(512, 2) void k_lattice_table_x(DecodeArgs A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const float voxel = A.grid.voxel_size;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = lane & 15, g = lane >> 4;
  const int64_t n_evals = A.entries ? (int64_t)A.n_list[1] : (int64_t)(*A.n_list) * 27;
  // HALF TILES in the tail.  A launch of T tiles on G workgroups takes ceil(T / G) rounds, and a shard of a spatially
  // sharded volume has only 5-8 tiles per workgroup: 7.2 tiles cost 8 rounds.  When the last round holds R <= G / 2
  // tiles, they are handed out as 2 R tiles of 64 evaluations (same weights from L2, half the MFMAs: ~0.6 of a round).
  const int64_t n_full_all = (n_evals + DM - 1) / DM;
  const int64_t rem = n_full_all % (int64_t)gridDim.x;
  const int64_t n_full = (A.half_tail && rem > 0 && 2 * rem <= (int64_t)gridDim.x) ? n_full_all - rem : n_full_all;
  const int64_t half0 = n_full * DM;   // first evaluation of the half tiles
  const int64_t n_tiles = n_full + (n_evals > half0 ? (n_evals - half0 + 63) / 64 : 0);
  // entry of evaluation slot se of a tile (-1: none)
  auto tile_entry = [&](int64_t t, int slot) -> int {
    if (t >= n_tiles) return -1;
    if (t < n_full) return lattice_entry(A, t * DM + slot, n_evals);
    return slot < 64 ? lattice_entry(A, half0 + (t - n_full) * 64 + slot, n_evals) : -1;
  };
  const float* pack = A.pack;
  const _Float16* px = (const _Float16*)(pack + SD_PACK_FLOATS);
  const float s5 = sinf(0.5f), c5 = cosf(0.5f);
  // Division of the per-tile side work (tools/phase_prof.py: with everything on threads 0..127 waves 0 and 1 were
  // ~1,400 cycles behind the others at two barriers of every tile):
  //  * staging of the next tile's network inputs: thread t stages octet so = t >> 7 (inputs 8 so .. 8 so + 7) of
  //    evaluation se = t & 127; octet 3 (inputs 24..31) is zero for good and written once;
  //  * the final 16-partial reduction and the table write: threads 128..255 (waves 2 and 3).
  const int se = threadIdx.x & (DM - 1);
  const int so = __builtin_amdgcn_readfirstlane(threadIdx.x >> 7);
  const bool writer = so == 1;

  // inputs 8 so .. 8 so + 7 of (entry ent, features f0 f1) into PARK at evaluation se
  auto stage_park = [&](int ent, const f32x4& f0, const f32x4& f1) {
    if (so == 3) return;
    float in[8];
#pragma unroll
    for (int f = 0; f < 8; ++f) in[f] = 0.f;
    if (ent >= 0) {
      const int l = ent & 31;
      const int lx = l / 9 - 1, ly = (l / 3) % 3 - 1, lz = l % 3 - 1;
      if (so == 0) {
        const int li[3] = {lx, ly, lz};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          in[a] = (float)li[a] * 0.5f;
          in[3 + a] = li[a] == 0 ? 0.f : (li[a] > 0 ? s5 : -s5);
        }
        in[6] = lx == 0 ? 1.f : c5;
        in[7] = ly == 0 ? 1.f : c5;
      } else if (so == 1) {
        const float fe[8] = {f0[0], f0[1], f0[2], f0[3], f1[0], f1[1], f1[2], f1[3]};
        check_feature_range(fe, pack[SD_BA + 1], A.vol.n_rows);
        in[0] = lz == 0 ? 1.f : c5;
#pragma unroll
        for (int f = 0; f < 4; ++f) in[1 + f] = f0[f];
#pragma unroll
        for (int f = 0; f < 3; ++f) in[5 + f] = f1[f];
      } else {
        in[0] = f1[3];
      }
    } else if (so == 0) {
      in[6] = in[7] = 1.f;   // what k_decode stages for an empty column: cos(0)
    } else if (so == 1) {
      in[0] = 1.f;
    }
    half8 hi, lo;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
      const _Float16 t = (_Float16)in[jj];
      hi[jj] = t;
      if (NPROD == 3) lo[jj] = (_Float16)(in[jj] - (float)t);
    }
    *(half8*)&lds[T_PARK_HI + (so * DM + se) * 4] = hi;
    if (NPROD == 3) *(half8*)&lds[T_PARK_LO + (so * DM + se) * 4] = lo;
  };
  auto load_feats = [&](int ent, f32x4& f0, f32x4& f1) {
    if (ent >= 0 && (so == 1 || so == 2)) {
      const size_t row = (size_t)(ent >> 5);
      if (so == 1) f0 = *(const f32x4*)&A.features[row * 8];
      f1 = *(const f32x4*)&A.features[row * 8 + 4];
    }
  };

  // ---- tiles are handed out DYNAMICALLY (one atomic per tile on a counter in the workspace, fetched one tile
  // ahead): when another stream's kernel still holds some CUs at launch (the next frame's encoder, an RCCL
  // collective), the workgroups that start late simply take fewer tiles instead of stretching the kernel's tail.
  // The first two tiles of a workgroup are static (b, b + grid): 2 x 256 atomics on ONE address at the start of every
  // launch serialised in the memory-side atomic unit for ~6 us before the first MFMA; dynamic ids start at 2 x grid.
  // Every loop iteration takes exactly one id and every tile is one iteration, so the counter ends at n_tiles: the
  // thread that draws n_tiles - 1 has drawn the launch's last id and puts the counter back to 0 for the next launch
  // (no exit count, no fence).
  __shared__ int s_tile[3];
  int* tile_ctr = (int*)A.n_list + 2;
  const int64_t dyn0 = 2 * (int64_t)gridDim.x;
  if (threadIdx.x == 0) {
    s_tile[0] = (int)blockIdx.x;
    s_tile[1] = (int)(blockIdx.x + gridDim.x);
  }
  if (so == 3) {   // octet 3 of PARK: inputs 24..31, always zero
    const half8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    *(half8*)&lds[T_PARK_HI + (3 * DM + se) * 4] = z;
    *(half8*)&lds[T_PARK_LO + (3 * DM + se) * 4] = z;
  }
  __syncthreads();
  int64_t tile = s_tile[0], tile_nx = s_tile[1];
  int ent_cur = -1, ent_nx = -1;
  f32x4 f0 = {0.f, 0.f, 0.f, 0.f}, f1 = {0.f, 0.f, 0.f, 0.f};
  ent_cur = tile_entry(tile, se);
  ent_nx = tile_entry(tile_nx, se);
  load_feats(ent_cur, f0, f1);
  stage_park(ent_cur, f0, f1);
  ARing ring;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)px, 0, SX_TOTAL * 2, 0x00020000);
  const int voff = lane * 16;
  constexpr int O0 = SX_W0 * 2, O1 = SX_W1 * 2, O2 = SX_W2 * 2, O3 = SX_W3 * 2;  // byte offsets of the layers
  {
#pragma unroll
    for (int p = 0; p < 2; ++p) {  // layer 0 has 2 units; its third request slot belongs to layer 1
      ring.hi[p] = load_frag(rs, voff, O0 + (w * 2 + p) * 2048);
      if (NPROD == 3) ring.lo[p] = load_frag(rs, voff, O0 + (w * 2 + p) * 2048 + 1024);
    }
    ring.hi[2] = load_frag(rs, voff, O1 + (w * 16) * 2048);
    if (NPROD == 3) ring.lo[2] = load_frag(rs, voff, O1 + (w * 16) * 2048 + 1024);
  }
  // LDS byte addresses of this lane (opaque to the optimiser: base + 16-bit immediates, encode_mlp.hip: EncLdsX)
  uint32_t act_hi, act_lo, park_hi, park_lo, st_hi, st_lo;
  {
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float*)lds;
    const uint32_t lane_off = (uint32_t)(g * DM + n) * 16u;
    act_hi = lds0 + L_HL * 4 + lane_off;
    act_lo = lds0 + L_HLO * 4 + lane_off;
    park_hi = lds0 + T_PARK_HI * 4 + lane_off;
    park_lo = lds0 + T_PARK_LO * 4 + lane_off;
    st_hi = act_hi + (uint32_t)w * 8192u;     // octet 4 w + g
    st_lo = act_lo + (uint32_t)w * 8192u;
    asm volatile("" : "+v"(act_hi), "+v"(act_lo), "+v"(park_hi), "+v"(park_lo), "+v"(st_hi), "+v"(st_lo));
  }
  // fc_alpha weights of this lane's eight features
  f32x4 wa0, wa1;
  wa0 = *(const f32x4*)&pack[SD_WA + 32 * w + 4 * g];
  wa1 = *(const f32x4*)&pack[SD_WA + 32 * w + 16 + 4 * g];
  __syncthreads();
#ifdef BNV_PHASE_PROF
  if (threadIdx.x < 256) ((unsigned long long*)(lds + T_TOTAL))[threadIdx.x] = 0;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) ((unsigned long long*)(lds + T_TOTAL))[(threadIdx.x >> 6) * 32 + 31] = clock64();
#endif

  auto one_tile = [&](auto half_tag) {
    constexpr bool HALF = decltype(half_tag)::value;
    // requests for the following tiles: the id of the tile after next (thread 0 asks now and publishes it behind
    // layer 0, so that the round trip of the atomic is off its wave's critical path), features of the next tile
    int next_id = 0;
    if (threadIdx.x == 0) {
      const int drawn = atomicAdd(tile_ctr, 1);
      if ((int64_t)drawn == n_tiles - 1) *tile_ctr = 0;   // the last draw of this launch
      next_id = (int)(dyn0 + drawn);
    }
    int ent_nx2 = -1;
    f0 = f32x4{0.f, 0.f, 0.f, 0.f};
    f1 = f32x4{0.f, 0.f, 0.f, 0.f};
    load_feats(ent_nx, f0, f1);
    f32x4 acc[2][8];
    BNV_PHX(0);
    chain_layer_x<2, 0, 16, NPROD, HALF>(rs, voff, O0, O1, pack + SD_B0, park_hi, park_lo, ring, acc, w, g);
    if (threadIdx.x == 0) s_tile[2] = next_id;
    BNV_PHX(1);
    __syncthreads();
    BNV_PHX(2);
    const int64_t tile_nx2 = s_tile[2];
    store_relu_x<NPROD, HALF>(st_hi, st_lo, acc);
    stage_park(ent_nx, f0, f1);  // PARK is free: every wave is past layer 0
    ent_nx2 = tile_entry(tile_nx2, se);
    BNV_PHX(3);
    __syncthreads();
    BNV_PHX(4);
    chain_layer_x<16, 2, 16, NPROD, HALF>(rs, voff, O1, O2, pack + SD_B0 + 256, act_hi, act_lo, ring, acc, w, g);
    BNV_PHX(5);
    __syncthreads();
    BNV_PHX(6);
    store_relu_x<NPROD, HALF>(st_hi, st_lo, acc);
    BNV_PHX(7);
    __syncthreads();
    BNV_PHX(8);
    chain_layer_x<16, 18, 16, NPROD, HALF>(rs, voff, O2, O3, pack + SD_B0 + 512, act_hi, act_lo, ring, acc, w, g);
    BNV_PHX(9);
    __syncthreads();
    BNV_PHX(10);
    store_relu_x<NPROD, HALF>(st_hi, st_lo, acc);
    BNV_PHX(11);
    __syncthreads();
    BNV_PHX(12);
    chain_layer_x<16, 34, 2, NPROD, HALF>(rs, voff, O3, O0, pack + SD_B0 + 768, act_hi, act_lo, ring, acc, w, g);
    ring.hi[2] = load_frag(rs, voff, O1 + (w * 16) * 2048);  // (50 + 2) % 5: layer 1's unit 0, next tile
    if (NPROD == 3) ring.lo[2] = load_frag(rs, voff, O1 + (w * 16) * 2048 + 1024);
    BNV_PHX(13);
    // fc_alpha: 256 -> 1.  Partial over this lane's 8 features, K-groups g and g + 2 combined across the lane
    // halves, 16 partials per evaluation through LDS
#pragma unroll
    for (int cb = 0; cb < (HALF ? 4 : 8); ++cb) {
      float sum = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) sum = fmaf(wa0[i], relu_bits(acc[0][cb][i]), sum);
#pragma unroll
      for (int i = 0; i < 4; ++i) sum = fmaf(wa1[i], relu_bits(acc[1][cb][i]), sum);
      sum += __shfl_xor(sum, 32, 64);
      if (g < 2) lds[L_PART + (w * 2 + g) * DM + cb * 16 + n] = sum;
    }
    BNV_PHX(14);
    __syncthreads();
    BNV_PHX(15);
    if (writer && ent_cur >= 0) {
      float sum = pack[SD_BA];
#pragma unroll
      for (int p = 0; p < 16; ++p) sum += lds[L_PART + p * DM + se];
      const int row = ent_cur >> 5;
      A.table[(size_t)row * 27 + (ent_cur & 31)] = __fmul_rn(sum, voxel);
      if (A.entries && A.need_mask) A.need_mask[row] = 0u;  // leave the per-row masks clean for the next call
    }
    ent_cur = ent_nx;
    ent_nx = ent_nx2;
    tile = tile_nx;
    tile_nx = tile_nx2;
    BNV_PHX(17);
  };
  while (tile < n_tiles) {
    if (__builtin_amdgcn_readfirstlane((int)(tile >= n_full))) one_tile(std::true_type{});
    else one_tile(std::false_type{});
  }
#ifdef BNV_PHASE_PROF
  __syncthreads();
  if (threadIdx.x < 256 && (threadIdx.x & 31) != 31)
    atomicAdd(&g_phase_cycles[threadIdx.x], ((unsigned long long*)(lds + T_TOTAL))[threadIdx.x]);
  if (threadIdx.x == 0) atomicAdd(&g_phase_cycles[31], 1ull);
#endif
}

// ---------------------------------------------------------------------------------------------------
// k_lattice_table_t: the lattice tables with the tiny-cuda-nn decoder (MLP mode 2), one WAVE per 32 entries.
// The generic k_decode<LATTICE, 2> is built around the fp32 decoder's tile: 512 threads, 141 KB of LDS (one workgroup
// per CU), the 128 staged inputs of a tile pass through LDS behind a barrier and only four of the eight waves run
// the (tiny) network: 0.162 ms per frame, 40 % of the tcnn frame's MLP time for 6 % of its FLOPs.  Here a wave
// loads its 32 entries, gathers their feature rows, builds the network's B operands in registers (positional
// encoding of a lattice offset: three values of {0, +-0.5} and their sin / cos), runs all four layers in registers
// with the weights in LDS (24.5 KB, staged once per workgroup) and writes its 32 table entries: no barrier, no LDS
// traffic for activations, 256-thread workgroups, four to five waves per SIMD.  Same operand values in the same MFMA
// order as the generic kernel: bit-identical tables (tests/test_gpu_parity.py).
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lattice_table_t(DecodeArgs A) {
  __shared__ __attribute__((aligned(16))) _Float16 wh[SdfPack::TOTAL];
  stage_to_lds<256>(A.pack, wh, SdfPack::TOTAL * 2);
  __syncthreads();
  const float voxel = A.grid.voxel_size;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 31, h = lane >> 5;
  const int64_t n_evals = A.entries ? (int64_t)A.n_list[1] : (int64_t)(*A.n_list) * 27;
  const int64_t n_tiles = (n_evals + 31) / 32;
  for (int64_t t = (int64_t)blockIdx.x * 4 + wave; t < n_tiles; t += (int64_t)gridDim.x * 4) {
    const int ent = lattice_entry(A, t * 32 + j, n_evals);
    float in[32];
#pragma unroll
    for (int f = 0; f < 32; ++f) in[f] = 1.0f;       // inputs 17..31: the padding of the tcnn encoding
    int row = 0, l = 0;
    if (ent >= 0) {
      row = ent >> 5;
      l = ent & 31;
      const float loc[3] = {(float)(l / 9 - 1) * 0.5f, (float)((l / 3) % 3 - 1) * 0.5f, (float)(l % 3 - 1) * 0.5f};
      const f32x4 f0 = *(const f32x4*)&A.features[(size_t)row * 8];
      const f32x4 f1 = *(const f32x4*)&A.features[(size_t)row * 8 + 4];
      // a lattice offset is -0.5, 0 or +0.5: its encoding is one of three constants (sinf / cosf cost more than
      // the tile's MFMAs; the operands are rounded to f16 below, where sin(0.5) and cos(0.5) sit 0.23 and 0.29 of a
      // spacing away from the nearest rounding boundary: the last bit of the fp32 value cannot matter)
      constexpr float kSinHalf = 0.479425538604203f, kCosHalf = 0.8775825618903728f;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        in[a] = loc[a];
        in[3 + a] = loc[a] == 0.f ? 0.f : (loc[a] > 0.f ? kSinHalf : -kSinHalf);
        in[6 + a] = loc[a] == 0.f ? 1.f : kCosHalf;
      }
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        in[9 + f] = f0[f];
        in[13 + f] = f1[f];
      }
    } else {
#pragma unroll
      for (int f = 0; f < 17; ++f) in[f] = 0.f;      // (an empty column; its output is not written)
    }
    half8 b[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) b[ks] = tcnn_input_frag(in, ks, h);
    const f32x16 o = tcnn_forward<2>(wh, lane, b);
    // output 0 = register 0 of the lanes with h == 0; the network returns fp16, and
    // half tensor * python float stays half (sparse_volume.py:813)
    if (h == 0 && ent >= 0) {
      float av = __fmul_rn((float)(_Float16)o[0], voxel);
      av = (float)(_Float16)av;
      A.table[(size_t)row * 27 + l] = av;
      if (A.entries && A.need_mask) A.need_mask[row] = 0u;   // leave the per-row masks clean for the next call
    }
  }
}

std::atomic<int> g_fused_mark{-1};  // bnv_set_option("fused_mark"): 1 / 0 force, -1 (default): by the call's size
std::atomic<int> g_mark_per_origin{1};   // bnv_set_option("mark_per_origin"): 1 = k_lattice_mark_o, 0 = k_lattice_mark (one thread per lattice point)
std::atomic<int> g_half_tail{1};    // bnv_set_option("half_tail"): k_lattice_table_x hands its last partial round out as half tiles
std::atomic<int> g_lattice_pipe{1}; // 1: k_lattice_table_x (cross-tile / cross-layer pipelined, 16x16x32 MFMA); 0: k_decode<LATTICE, 1>

#ifdef BNV_PHASE_PROF
constexpr int kProfLds = 2048;
#else
constexpr int kProfLds = 0;
#endif

// f(std::integral_constant<int, M>{}) for the front / back end `mode` of k_decode (MODE_PTS has kernels of its own)
template <class F>
static inline void dispatch_mode(int mode, F f) {
  if (mode == MODE_LATTICE) f(std::integral_constant<int, MODE_LATTICE>{});
  else if (mode == MODE_DENSE1) f(std::integral_constant<int, MODE_DENSE1>{});
  else f(std::integral_constant<int, MODE_DENSE>{});
}

// `mlp`: the arithmetic mode of the call (mlp_mode_of(grid.mlp_mode))
static int launch_decode(int mode, int mlp, const DecodeArgs& args, int64_t n_tiles_hint, hipStream_t stream,
                         int max_workgroups = 0) {
  int64_t grid = g_num_cus - g_reserve_cus.load(std::memory_order_relaxed);
  if (max_workgroups > 0 && grid > max_workgroups) grid = max_workgroups;   // (persistent kernels, dynamic tile hand-out)
  if (n_tiles_hint < grid) grid = n_tiles_hint;
  if (grid < 1) grid = 1;
  const bool lattice_pipe = g_lattice_pipe.load(std::memory_order_relaxed) != 0;
  if (mode == MODE_LATTICE && (mlp == 1 || mlp == 3) && lattice_pipe) {
    ProfScope prof(PROF_DECODE_LATTICE, stream);
    DecodeArgs ax = args;
    ax.half_tail = g_half_tail.load(std::memory_order_relaxed);
    if (mlp == 1)
      hipLaunchKernelGGL(k_lattice_table_x<3>, dim3((unsigned)grid), dim3(512), T_TOTAL * 4 + kProfLds, stream, ax);
    else
      hipLaunchKernelGGL(k_lattice_table_x<1>, dim3((unsigned)grid), dim3(512), T_TOTAL * 4 + kProfLds, stream, ax);
    BNV_LAUNCH_CHECK();
    return BNV_OK;
  }
  if (mode == MODE_LATTICE && mlp == 2 && lattice_pipe) {
    ProfScope prof(PROF_DECODE_LATTICE, stream);
    int64_t gt = (int64_t)g_num_cus * 4;                    // four 4-wave workgroups per CU, grid-stride over the tiles
    const int64_t wgs = (n_tiles_hint * (DM / 32) + 3) / 4;   // (the hint counts 128-evaluation tiles)
    if (wgs < gt) gt = wgs;
    if (gt < 1) gt = 1;
    hipLaunchKernelGGL(k_lattice_table_t, dim3((unsigned)gt), dim3(256), 0, stream, args);
    BNV_LAUNCH_CHECK();
    return BNV_OK;
  }
  ProfScope prof(mode == MODE_LATTICE ? PROF_DECODE_LATTICE : PROF_DECODE_DENSE, stream);
  dispatch_prec(mlp, [&](auto p) {
    dispatch_mode(mode, [&](auto m) {
      hipLaunchKernelGGL((k_decode<decltype(m)::value, decltype(p)::value>), dim3((unsigned)grid), dim3(512),
                         L_TOTAL * 4 + kProfLds, stream, args);
    });
  });
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

int lattice_table_impl(const bnv_volume_t* vol, const bnv_grid_t* grid, const float* features,
                       const float* sdfmlp_pack, int64_t n_voxels, int use_entries, void* ws_ptr, size_t ws_bytes,
                       int max_workgroups, bnv_stream_t stream) {
  if (g_num_cus <= 0) return BNV_ERR_NOT_INITIALISED;
  if (!vol_ok_ro(vol) || !grid || !features || !sdfmlp_pack || !ws_ptr || !mlp_mode_field_ok(grid->mlp_mode))
    return BNV_ERR_INVALID_ARGUMENT;
  LatticeWs ws;
  if (lattice_ws_layout(n_voxels, vol->row_capacity, (char*)ws_ptr, &ws) > ws_bytes)
    return BNV_ERR_WORKSPACE_TOO_SMALL;
  DecodeArgs a = {};
  a.vol = *vol;
  a.grid = *grid;
  a.features = features;
  a.pack = sdfmlp_pack;
  a.list = ws.list;
  a.n_list = ws.n_list;
  a.table = ws.table;
  a.need_mask = ws.need_mask;
  if (lattice_persist(vol)) {
    // ONE predicate for the three stages (mark, table, blend all ask lattice_persist(vol)): a call that switches the
    // persistent tables on works on the volume's own feature rows and on listed entries, or is rejected -- the marking
    // kernel has kept its books in lattice_have and the blend will read vol->lattice_table
    if (!use_entries || features != vol->features) return BNV_ERR_INVALID_ARGUMENT;
    a.table = vol->lattice_table;   // the listed entries are the ones the persistent table lacks
    a.need_mask = nullptr;
  }
  a.entries = use_entries ? ws.entries : nullptr;
  const int64_t evals = use_entries ? ws.entry_capacity : ws.list_capacity * 27;
  return launch_decode(MODE_LATTICE, mlp_mode_of(grid->mlp_mode), a, (evals + DM - 1) / DM, (hipStream_t)stream,
                       max_workgroups);
}

}  // namespace bnv

using namespace bnv;

extern "C" {

// every kernel that asks for more dynamic LDS than the default limit opts in once per process
int bnv_decode_init() {
  int rc = BNV_OK;
  for (int mlp = 0; mlp < 4; ++mlp)
    dispatch_prec(mlp, [&](auto p) {
      constexpr int P = decltype(p)::value;
      opt_in_lds(rc, (const void*)k_decode<MODE_LATTICE, P>, L_TOTAL * 4 + kProfLds);
      opt_in_lds(rc, (const void*)k_decode<MODE_DENSE, P>, L_TOTAL * 4 + kProfLds);
      opt_in_lds(rc, (const void*)k_decode<MODE_DENSE1, P>, L_TOTAL * 4 + kProfLds);
    });
  opt_in_lds(rc, (const void*)k_lattice_table_x<3>, T_TOTAL * 4 + kProfLds);
  opt_in_lds(rc, (const void*)k_lattice_table_x<1>, T_TOTAL * 4 + kProfLds);
  return rc != BNV_OK ? rc : decode_pts_init();
}

size_t bnv_sdfmlp_pack_floats(void) { return SD_PACK_FLOATS_X; }

#ifdef BNV_PHASE_PROF
// development builds only (not in include/bnv_fusion.h): read and reset the phase cycle counters
int bnv_dev_phase_read(unsigned long long* out256) {
  BNV_HIP_CHECK(hipDeviceSynchronize());
  BNV_HIP_CHECK(hipMemcpyFromSymbol(out256, HIP_SYMBOL(g_phase_cycles), 256 * sizeof(unsigned long long)));
  unsigned long long z[256] = {};
  BNV_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_phase_cycles), z, sizeof(z)));
  return BNV_OK;
}
#endif

int bnv_set_option(const char* name, int value) {
  if (!name) return BNV_ERR_INVALID_ARGUMENT;
  // plain words; flag: stored as value != 0
  static const struct { const char* name; std::atomic<int>* word; bool flag; } kWords[] = {
      {"lattice_pipe", &g_lattice_pipe, false},           {"mark_per_origin", &g_mark_per_origin, true},
      {"half_tail", &g_half_tail, true},                  {"fused_mark", &g_fused_mark, false},
      {"tcnn_block_encoder", &g_tcnn_block_encoder, true}, {"tcnn_shared_table", &g_tcnn_shared_table, true}};
  for (const auto& o : kWords)
    if (!strcmp(name, o.name)) {
      o.word->store(o.flag ? value != 0 : value, std::memory_order_relaxed);
      return BNV_OK;
    }
  if (!strcmp(name, "finalize_blocks")) {
    if (value < 0) return BNV_ERR_INVALID_ARGUMENT;
    g_finalize_blocks.store(value, std::memory_order_relaxed);
    return BNV_OK;
  }
  if (!strcmp(name, "reserve_cus")) {
    if (value < 0 || value >= g_num_cus) return BNV_ERR_INVALID_ARGUMENT;
    g_reserve_cus.store(value, std::memory_order_relaxed);
    return BNV_OK;
  }
  return BNV_ERR_INVALID_ARGUMENT;
}

int bnv_decode_dense(const float* feat_grid, const float* pts_weight, const int32_t dims[3], float voxel_size,
                     int32_t min_pts_in_grid, const float* sdfmlp_pack, const float* voxel_coords, int64_t n,
                     int32_t variant, int32_t mlp_mode, float* out_sdf, float* out_feats, int32_t* status,
                     bnv_stream_t stream) {
  if (g_num_cus <= 0) return BNV_ERR_NOT_INITIALISED;
  if (!feat_grid || !pts_weight || !dims || !sdfmlp_pack || n < 0 || !mlp_mode_field_ok(mlp_mode))
    return BNV_ERR_INVALID_ARGUMENT;
  const int mlp = mlp_mode_of(mlp_mode);
  if (variant < BNV_DENSE_CORNERS || variant > BNV_DENSE_GLOBAL) return BNV_ERR_INVALID_ARGUMENT;
  if (variant == BNV_DENSE_CORNERS && out_feats) return BNV_ERR_INVALID_ARGUMENT;
  if (dims[0] < 2 || dims[1] < 2 || dims[2] < 2) return BNV_ERR_INVALID_ARGUMENT;   // coords / (res - 1)
  if (n == 0) return BNV_OK;
  if (!voxel_coords || !out_sdf) return BNV_ERR_INVALID_ARGUMENT;
  DecodeArgs a = {};
  a.status = status;
  a.nf_out = out_feats;
  a.variant = variant == BNV_DENSE_GLOBAL ? 1 : 0;
  a.grid.voxel_size = voxel_size;
  a.grid.min_pts_in_grid = min_pts_in_grid;
  a.pack = sdfmlp_pack;
  a.coords = voxel_coords;
  a.n = n;
  a.is_coords = 1;
  a.out = out_sdf;
  a.feat_grid = feat_grid;
  a.pts_weight = pts_weight;
  a.dims[0] = dims[0];
  a.dims[1] = dims[1];
  a.dims[2] = dims[2];
  if (variant != BNV_DENSE_CORNERS) return launch_decode(MODE_DENSE1, mlp, a, (n + DM - 1) / DM, (hipStream_t)stream);
  return launch_decode(MODE_DENSE, mlp, a, (n + 15) / 16, (hipStream_t)stream);
}

int bnv_lattice_table(const bnv_volume_t* vol, const bnv_grid_t* grid, const float* features,
                      const float* sdfmlp_pack, int64_t n_voxels, int use_entries, void* ws_ptr, size_t ws_bytes,
                      bnv_stream_t stream) {
  return lattice_table_impl(vol, grid, features, sdfmlp_pack, n_voxels, use_entries, ws_ptr, ws_bytes, 0, stream);
}

}  // extern "C"
