// encode_mlp.hip -- the point encoders of the fp32 network (6 -> 128 -> 128 -> 128 -> 8, MLP modes 0, 1 and 3): per
// (point, corner) pair the MLP on MFMA (transposed chaining: layer L's D registers are layer L+1's B operands, no
// cross-lane traffic), then order-independent 64-bit fixed-point atomics into per-voxel accumulators (encode.hpp).
// Layout of one MFMA tile: 32 pairs = 32 consecutive points x one corner.  Exact fp32 (k_pointnet_scatter,
// 32x32x2 MFMA): lane l = (j = l & 31: pair, h = l >> 5); D register r of a 32-feature block holds feature
// (r&3) + 8*(r>>2) + 4*h of pair j, so the K-step that consumes D[r] as its B operand contracts features
// {f0(r), f0(r)+4}.  Split modes (k_pointnet_scatter_x, 16x16x32 MFMA): lane l = (n = l & 15, g = l >> 4), two
// column blocks of 16 pairs, eight row blocks of 16 features (layout at the kernel).  The packed A operands
// (weights) are pre-permuted on the host to match (bnv_fusion_amd/weights.py: pack_pointnet).
#include "encode.hpp"

namespace bnv {

// ---- k_pointnet_scatter: exact fp32 on the 32x32x2 MFMA ----------------------------------------------------------
__device__ __forceinline__ f32x16 relu16(f32x16 v) {
#pragma unroll
  for (int r = 0; r < 16; ++r) v[r] = relu_bits(v[r]);
  return v;
}

__device__ __forceinline__ f32x16 bias_init(const float* __restrict__ b, int mb, int h) {
  f32x16 v;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x4 t = *(const f32x4*)&b[mb * 32 + 8 * q + 4 * h];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[4 * q + i] = t[i];
  }
  return v;
}

// 128 -> 128 layer: out[mb] += W[mb][nb] * in[nb]
__device__ __forceinline__ void layer128(const float* __restrict__ wp, const float* __restrict__ bias,
                                         const f32x16 (&in)[4], f32x16 (&out)[4], int lane, int h) {
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) out[mb] = bias_init(bias, mb, h);
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      f32x4 a[4];
#pragma unroll
      for (int mb = 0; mb < 4; ++mb)
        a[mb] = *(const f32x4*)&wp[(((mb * 4 + nb) * 4 + rq) * 64 + lane) * 4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int mb = 0; mb < 4; ++mb)
          out[mb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mb][i], in[nb][4 * rq + i], out[mb], 0, 0, 0);
      }
    }
  }
}

__global__ __launch_bounds__(512, 2) void k_pointnet_scatter(
    const float* __restrict__ pts, int n_points, bnv_grid_t g, const float* __restrict__ wpack,
    const uint32_t* __restrict__ bitmap, const uint32_t* __restrict__ word_prefix,
    int32_t* __restrict__ counts, long long* __restrict__ acc, const int32_t* __restrict__ pair_list,
    const int32_t* __restrict__ n_pairs) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  // stage all packed weights into LDS once per workgroup (persistent grid)
  stage_to_lds<512>(wpack, lds, PN_TOTAL * 4);
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 31, h = lane >> 5;
  const PairTiles T = pair_tiles(n_points, pair_list, n_pairs);
  const int n_tiles = T.n_tiles;

  for (int t = blockIdx.x * 8 + wave; t < n_tiles; t += gridDim.x * 8) {
    int i = 0, k = 0;
    const bool have = tile_pair(T, t, j, &i, &k);
    float in0 = 0.f, in1 = 0.f, in2 = 0.f;  // this lane's half of the 6 inputs: features 2s + h
    int slot = -1;
    bool valid = false;
    if (have) {
      const float* p = pts + (size_t)i * 6;
      const float x = p[0], y = p[1], z = p[2];
      valid = in_bounds(x, y, z, g);
      if (valid) {
        const float xn = voxel_coord(x, g.bound_min[0], g.voxel_size);
        const float yn = voxel_coord(y, g.bound_min[1], g.voxel_size);
        const float zn = voxel_coord(z, g.bound_min[2], g.voxel_size);
        int gx, gy, gz;
        const uint32_t id = corner_voxel(k, xn, yn, zn, g, gx, gy, gz);
        if (voxel_owner(gx, gy, gz, g) == g.shard_rank) slot = slot_rank(bitmap[id >> 5], word_prefix[id >> 5], id);
        const float rx = relative_coord(xn, gx, g.voxel_size);
        const float ry = relative_coord(yn, gy, g.voxel_size);
        const float rz = relative_coord(zn, gz, g.voxel_size);
        // inputs [rx, ry, rz, nx, ny, nz]; K-step s contracts inputs (2s, 2s+1) = (h=0, h=1)
        in0 = h ? ry : rx;
        in1 = h ? p[3] : rz;
        in2 = h ? p[5] : p[4];
      }
    }
    // the tile is skipped when no lane contributes (wave-uniform branch)
    if (__ballot(slot >= 0) == 0ULL) continue;

    // ---- layer 1: 6 -> 128 --------------------------------------------------------------
    f32x16 ha[4], hb[4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) ha[mb] = bias_init(lds + PN_B1, mb, h);
    {
      const float bin[3] = {in0, in1, in2};
#pragma unroll
      for (int s = 0; s < 3; ++s) {
#pragma unroll
        for (int mb = 0; mb < 4; ++mb)
          ha[mb] = __builtin_amdgcn_mfma_f32_32x32x2f32(lds[PN_W1 + (s * 4 + mb) * 64 + lane], bin[s],
                                                        ha[mb], 0, 0, 0);
      }
    }
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) ha[mb] = relu16(ha[mb]);
    // ---- layers 2, 3: 128 -> 128 ---------------------------------------------------------
    layer128(lds + PN_W2, lds + PN_B2, ha, hb, lane, h);
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) hb[mb] = relu16(hb[mb]);
    layer128(lds + PN_W3, lds + PN_B3, hb, ha, lane, h);
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) ha[mb] = relu16(ha[mb]);
    // ---- layer 4: 128 -> 8 (rows 8..31 of the MFMA tile are zero padding) ------------------
    f32x16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
    {
      const f32x4 b4 = *(const f32x4*)&lds[PN_B4 + 4 * h];
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = b4[r];
    }
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        if (j < 8) a = *(const f32x4*)&lds[PN_W4 + ((((nb * 4 + rq) * 2 + h) * 8) + j) * 4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          o = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], ha[nb][4 * rq + i], o, 0, 0, 0);
      }
    }
    scatter_tile(o, slot, j, h, counts, acc);
  }
}

// Split-operand encoder (MLP modes 1 and 3): every fp32 operand is split into f16 hi + lo (x = hi + lo to ~22 bits;
// f16 subnormals are kept by the MFMA) and a.b ~ ah.bh + ah.bl + al.bh on the f16 MFMA with fp32 accumulation:
// fp32-class results at 16/3 x the fp32 MFMA rate (mode 3: ah.bh only).
// LDS reads of the split-operand encoder go through a handful of OPAQUE 32-bit base addresses plus compile-time
// byte offsets that fit the 16-bit immediate of ds_read_b128.  Written as plain pointer arithmetic on the 150 KB
// weight image the compiler kept ~40 VGPRs of pre-added addresses alive across the tile loop (and spilled the
// staged point of the next tile for them); with three weight bases (lane * 16 + 0 / 60 KB / 120 KB) and one for
// the biases it keeps four.
typedef __attribute__((address_space(3))) const half8 lds_half8_t;
typedef __attribute__((address_space(3))) const f32x4 lds_f32x4_t;
constexpr int kLdsWin = 61440;   // span of one weight base (< 64 KB immediate range, multiple of 1024)

#ifdef BNV_PHASE_PROF
__device__ unsigned long long g_enc_phase[8 * 16];
#define BNV_EPH(i)                                                                          \
  do {                                                                                      \
    if ((threadIdx.x & 63) == 0) {                                                          \
      unsigned long long* _p = (unsigned long long*)((char*)lds + PX_LDS_BYTES) + (threadIdx.x >> 6) * 16; \
      const unsigned long long _t = clock64();                                              \
      _p[i] += _t - _p[15];                                                                 \
      _p[15] = _t;                                                                          \
    }                                                                                       \
  } while (0)
constexpr int kEncProfLds = 8 * 16 * 8;
#else
#define BNV_EPH(i)
constexpr int kEncProfLds = 0;
#endif

// k_pointnet_scatter_x: the split-operand encoder on v_mfma_f32_16x16x32_f16.
// The kernel runs at the package power limit (tools/power_probe.py) and under that limit the 16x16x32 form
// delivers ~14 % more FLOP/s than the 32x32x16 form (tools/probe_shapes.hip).  Same
// arithmetic (three products, fp32 accumulation), same bytes from LDS, another shape of a wave's tile:
//  * lane (n = l & 15, g = l >> 4); a tile is still 32 pairs = 2 COLUMN blocks of 16 (pair p = 16 cb + n) and a
//    128-wide layer is 8 ROW blocks of 16 features: 16 accumulators of 4 registers, register i of acc[rb][cb] =
//    feature 16 rb + 4 g + i of pair 16 cb + n;
//  * chaining: a K-step is 32 deep, operand slot jj of K-group g is K index 8 g + jj.  The eight registers
//    {acc[2 s][cb][0..3], acc[2 s + 1][cb][0..3]} of a lane are exactly its operand of K-step s of the next layer
//    for column block cb (slot jj <-> feature 32 s + 16 (jj >> 2) + 4 g + (jj & 3)): no cross-lane traffic
//    between the layers, as before.  The weights are packed to that order on the host (weights.py:
//    _pack_pointnet_split16, encode.hpp: PX_*);
//  * a pair is STAGED by the two lanes (n, 2 c) and (n, 2 c + 1) of its column block c (both need its slot for the
//    scatter: they scatter output features 0..3 and 4..7); the first layer's inputs live in K-group 0, so lanes
//    g = 0 take the six inputs of pair 16 + n from lane l + 32;
//  * the last layer is ONE row block (8 of 16 rows used) instead of one 32-row tile (8 of 32): half the MFMA work
//    of that layer; its outputs for column block 1 go back to the lanes that staged those pairs (lane l + 32);
//  * the scatter's prefix sums are row-local (a DPP row = a column block of a feature half: 4 steps) and joined
//    across the two column blocks through lane 15.
struct EncLdsX {
  uint32_t w[3];   // lane * 16 + kLdsWin * {0, 1, 2}
  uint32_t b;      // biases: 4 * g floats into the bias block
};
__device__ __forceinline__ half8 ldsx_wfrag(const EncLdsX& L, int byte_off) {
  const int b = byte_off / kLdsWin;
  return *(lds_half8_t*)((b == 0 ? L.w[0] : (b == 1 ? L.w[1] : L.w[2])) + (uint32_t)(byte_off - b * kLdsWin));
}
__device__ __forceinline__ f32x4 ldsx_bias(const EncLdsX& L, int layer, int rb) {
  return *(lds_f32x4_t*)(L.b + (uint32_t)((layer * 128 + rb * 16) * 4));
}

// 128 -> 128 layer: 32 steps q = (K-step s = q >> 3, row block rb = q & 7), six MFMAs per step (two column blocks
// x three products; the two chains of a step alternate), the weight fragments of step q + 1 fetched before them
template <int NPROD>
__device__ __forceinline__ void layer128_x(const EncLdsX& L, int w_off, int layer, const half8 (&inh)[4][2],
                                           const half8 (&inl)[4][2], f32x4 (&out)[8][2]) {
#pragma unroll
  for (int rb = 0; rb < 8; ++rb) out[rb][0] = out[rb][1] = ldsx_bias(L, layer, rb);
  half8 ah[2], al[2];
#define BNV_LOAD_WX(q)                                                        \
  {                                                                           \
    const int wb = (w_off + (q) * 2 * 64 * 8) * 2;                            \
    ah[(q) & 1] = ldsx_wfrag(L, wb);                                          \
    if (NPROD == 3) al[(q) & 1] = ldsx_wfrag(L, wb + 1024);                   \
  }
  BNV_LOAD_WX(0);
#pragma unroll
  for (int q = 0; q < 32; ++q) {
    if (q + 1 < 32) BNV_LOAD_WX(q + 1);
    __builtin_amdgcn_sched_barrier(0);
    const int s = q >> 3, rb = q & 7;
    if constexpr (NPROD == 3) {
      out[rb][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[q & 1], inh[s][0], out[rb][0], 0, 0, 0);
      out[rb][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[q & 1], inh[s][1], out[rb][1], 0, 0, 0);
      out[rb][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[q & 1], inl[s][0], out[rb][0], 0, 0, 0);
      out[rb][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[q & 1], inl[s][1], out[rb][1], 0, 0, 0);
    }
    out[rb][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[q & 1], inh[s][0], out[rb][0], 0, 0, 0);
    out[rb][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[q & 1], inh[s][1], out[rb][1], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
#undef BNV_LOAD_WX
}

// ReLU + hi/lo split of a layer's accumulators into the next layer's operands
template <int NPROD>
__device__ __forceinline__ void split_x(const f32x4 (&acc)[8][2], half8 (&oh)[4][2], half8 (&ol)[4][2]) {
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      float x[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = relu_bits(acc[2 * s + (e >> 2)][cb][e & 3]);
      if (NPROD == 3) {
        split8_f16(x, oh[s][cb], ol[s][cb]);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) oh[s][cb][e] = (_Float16)x[e];
      }
    }
}

// Scatter of one tile: this lane holds output features 4 fh .. 4 fh + 3 (fh = g & 1) of pair p = 16 (g >> 1) + n: the
// 32 pairs of a feature half are DPP rows fh and fh + 2.  Same scheme as scatter_tile (run sums = differences of ONE
// inclusive prefix sum over the 32 pairs, exact in modular arithmetic; the run's pair count is its length): row-local
// prefix sums (4 DPP steps), then rows 2 and 3 add the totals of rows 0 and 1 (lane 15 of those rows).
__device__ __forceinline__ void scatter_tile_x(const f32x4& o, int slot, int n, int g, int32_t* __restrict__ counts,
                                               long long* __restrict__ acc) {
  uint32_t lo[4], hi[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) fixed_hi_lo(o[q], hi[q], lo[q]);
  asm volatile(BNV_SCAN_ROWS : BNV_SCAN_REGS(lo, hi) : : "vcc");
  {   // rows 2, 3 (pairs 16..31): + the total of pairs 0..15 of the same feature half (lane 15 of row g - 2)
    const int tsrc = ((g & 1) * 16 + 15) * 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t tl = (uint32_t)__builtin_amdgcn_ds_bpermute(tsrc, (int)lo[q]);
      const uint32_t th = (uint32_t)__builtin_amdgcn_ds_bpermute(tsrc, (int)hi[q]);
      if (g >= 2) {
        const unsigned long long v = (((unsigned long long)hi[q] << 32) | lo[q]) + (((unsigned long long)th << 32) | tl);
        lo[q] = (uint32_t)v;
        hi[q] = (uint32_t)(v >> 32);
      }
    }
  }
  const int p = (g >> 1) * 16 + n;
  const int slot15 = __builtin_amdgcn_readlane(slot, 15);                     // pair 15 (lanes 15 and 31 stage it)
  const int prev_row = __builtin_amdgcn_update_dpp(0, slot, 0x111 /* row_shr:1 */, 0xf, 0xf, false);
  const int prev = n == 0 ? slot15 : prev_row;
  const unsigned long long heads64 = __ballot(p == 0 || prev != slot);
  const uint32_t heads = ((uint32_t)heads64 & 0xffffu) | (((uint32_t)(heads64 >> 32) & 0xffffu) << 16);   // rows 0 and 2
  const int s = 31 - __clz((int)(heads & (0xffffffffu >> (31 - p))));         // head of this lane's run (bit 0 is set)
  const bool is_end = p == 31 || ((heads >> (p + 1)) & 1u);
  const int sp = s > 0 ? s - 1 : 0;                                            // pair holding P[s - 1]
  const int src = (((sp >> 4) * 2 + (g & 1)) * 16 + (sp & 15)) * 4;
  uint32_t plo[4], phi[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    plo[q] = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)lo[q]);
    phi[q] = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)hi[q]);
  }
#ifdef BNV_PROBE_NO_SCATTER   // development probe (tools/enc_time.py): keeps 1 of 64 workgroups' atomics
  if ((blockIdx.x & 63) != 0) return;
#endif
  if (slot >= 0 && is_end) {
    // run_to_global, spelt out: with the four sums formed first the compiler allocates k_pointnet_scatter_x differently
    unsigned long long* dst = (unsigned long long*)acc + ((uint32_t)slot * 8u + 4u * (uint32_t)(g & 1));
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      unsigned long long v = ((unsigned long long)hi[q] << 32) | lo[q];
      if (s > 0) v -= ((unsigned long long)phi[q] << 32) | plo[q];
      atomicAdd(dst + q, v);
    }
    if ((g & 1) == 0) atomicAdd(&counts[slot], p - s + 1);
  }
}

template <int NPROD>
__global__ __launch_bounds__(512, 2) __attribute__((amdgpu_num_vgpr(120))) void k_pointnet_scatter_x(
    const float* __restrict__ pts, int n_points, bnv_grid_t g, const float* __restrict__ wpack,
    const uint32_t* __restrict__ bitmap, const uint32_t* __restrict__ word_prefix,
    int32_t* __restrict__ counts, long long* __restrict__ acc, int32_t* __restrict__ error,
    const int32_t* __restrict__ pair_list, const int32_t* __restrict__ n_pairs) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const float n_cert = wpack[PN_CERT];
  float* lb = lds + PX_TOTAL / 2;                      // b1 b2 b3 b4
  for (int i = threadIdx.x; i < 128 * 3 + 8; i += 512) lb[i] = wpack[PN_B1 + i];
  stage_to_lds<512>(wpack + PX_OFF, lds, PX_TOTAL * 2);
  int* tile_ctr = (int*)((char*)lds + PX_TOTAL * 2 + (128 * 3 + 8) * 4);
  if (threadIdx.x == 0) *tile_ctr = 0;
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int n = lane & 15, gk = lane >> 4;          // K-group / accumulator row group
  const int pair = (gk >> 1) * 16 + n;              // the pair this lane stages and scatters
  const PairTiles T = pair_tiles(n_points, pair_list, n_pairs);
  const int n_tiles = T.n_tiles;
  const int nyz = g.n_xyz[1] * g.n_xyz[2];
  EncLdsX L;
  {
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float*)lds;
    L.w[0] = lds0 + lane * 16;
    L.w[1] = L.w[0] + kLdsWin;
    L.w[2] = L.w[0] + 2 * kLdsWin;
    L.b = lds0 + PX_TOTAL * 2 + gk * 16;
    asm volatile("" : "+v"(L.w[0]), "+v"(L.w[1]), "+v"(L.w[2]), "+v"(L.b));
  }

  // Software pipeline over this wave's tiles: while tile t runs its MLP, the point of tile t+2 and the
  // bitmap / prefix words of tile t+1 are in flight (three dependent memory latencies per tile).
  // The workgroup's tiles {8 b + k + i * 8 * gridDim} are handed to its 8 waves DYNAMICALLY (LDS counter):
  // of the two waves on a SIMD the older one wins issue arbitration and runs ~1.4x faster, so with a
  // static split the younger waves were still working when the older ones had finished
  // (tools/phase_prof.py).  The scatter is order-independent, so results do not depend on who takes what.
  const int tstep = gridDim.x * 8;
  auto grab = [&]() -> int {
    int c = 0;
    if (lane == 0) c = atomicAdd(tile_ctr, 1);
    c = __builtin_amdgcn_readfirstlane(c);
    return blockIdx.x * 8 + (c & 7) + (c >> 3) * tstep;
  };
  float raw[6];                 // stage 1 (tile t+2): the raw point and its corner
  int raw_k = 0;
  bool raw_ok = false;
  float nin[6];                 // stage 2 (tile t+1): network inputs (lanes of even g), voxel id, bitmap / prefix words
  uint32_t n_id = 0, n_word = 0, n_pref = 0;
  bool n_own = false;
  auto stage1 = [&](int t) {
    raw_ok = false;
    if (t < n_tiles) {
      int i = 0;
      if (tile_pair(T, t, pair, &i, &raw_k)) {
        const float* p = pts + (size_t)i * 6;
#pragma unroll
        for (int c = 0; c < 6; ++c) raw[c] = p[c];
        raw_ok = true;
      }
    }
  };
  auto stage2 = [&](int t) {
    n_own = false;
#pragma unroll
    for (int c = 0; c < 6; ++c) nin[c] = 0.f;
    if (raw_ok && in_bounds(raw[0], raw[1], raw[2], g)) {
      const int k = raw_k;
      const float xn = voxel_coord(raw[0], g.bound_min[0], g.voxel_size);
      const float yn = voxel_coord(raw[1], g.bound_min[1], g.voxel_size);
      const float zn = voxel_coord(raw[2], g.bound_min[2], g.voxel_size);
      int gx, gy, gz;
      corner_xyz(k, xn, yn, zn, gx, gy, gz);   // (not corner_voxel: the id in front of the ownership test changes the kernel's code)
      if (voxel_owner(gx, gy, gz, g) == g.shard_rank) {
        n_own = true;
        n_id = voxel_id(gx, gy, gz, nyz, g.n_xyz[2]);
        n_word = bitmap[n_id >> 5];
        n_pref = word_prefix[n_id >> 5];
      }
      if ((gk & 1) == 0) {
        nin[0] = relative_coord(xn, gx, g.voxel_size);
        nin[1] = relative_coord(yn, gy, g.voxel_size);
        nin[2] = relative_coord(zn, gz, g.voxel_size);
        nin[3] = raw[3];
        nin[4] = raw[4];
        nin[5] = raw[5];
      }
      if (!(fmaxf(fmaxf(fabsf(raw[3]), fabsf(raw[4])), fabsf(raw[5])) <= n_cert)) *error = 3;
    }
  };
  int t = grab();
  stage1(t);
  stage2(t);
  int t_next = grab(), t_next2 = 0;
  stage1(t_next);
#ifdef BNV_PHASE_PROF
  if ((threadIdx.x & 63) < 16)
    ((unsigned long long*)((char*)lds + PX_LDS_BYTES))[(threadIdx.x >> 6) * 16 + (threadIdx.x & 63)] = 0;
  if ((threadIdx.x & 63) == 0) ((unsigned long long*)((char*)lds + PX_LDS_BYTES))[(threadIdx.x >> 6) * 16 + 15] = clock64();
#endif

  for (; t < n_tiles; t = t_next, t_next = t_next2) {
    float in[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) in[c] = nin[c];
    const int slot = n_own ? slot_rank(n_word, n_pref, n_id) : -1;
    stage2(t_next);
    t_next2 = grab();
    stage1(t_next2);
    __builtin_amdgcn_sched_barrier(0);
    BNV_EPH(0);
    if (__ballot(slot >= 0) == 0ULL) continue;

    // ---- layer 1: 6 -> 128, one K-step of 32 (inputs in K-group 0: slots 0..5 of lanes g = 0) --------------
    f32x4 ha[8][2], hb[8][2];
    {
      half8 bh[2], bl[2];
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) {
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = 0.f;
#pragma unroll
        for (int e = 0; e < 6; ++e) {
          const float other = __shfl(in[e], (lane + 32) & 63, 64);   // pair 16 + n is staged by lane l + 32
          x[e] = gk == 0 ? (cb == 0 ? in[e] : other) : 0.f;
        }
        if (NPROD == 3) {
          split8_f16(x, bh[cb], bl[cb]);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) bh[cb][e] = (_Float16)x[e];
        }
      }
#pragma unroll
      for (int rb = 0; rb < 8; ++rb) {
        const half8 ahi = ldsx_wfrag(L, (PX_W1 + rb * 2 * 64 * 8) * 2), alo = ldsx_wfrag(L, (PX_W1 + rb * 2 * 64 * 8) * 2 + 1024);
        const f32x4 b = ldsx_bias(L, 0, rb);
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
          f32x4 c = b;
          if constexpr (NPROD == 3) {
            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(alo, bh[cb], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi, bl[cb], c, 0, 0, 0);
          }
          ha[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi, bh[cb], c, 0, 0, 0);
        }
      }
    }
    BNV_EPH(1);
    half8 sh[4][2], sl[4][2];
    split_x<NPROD>(ha, sh, sl);
    BNV_EPH(2);
    layer128_x<NPROD>(L, PX_W2, 1, sh, sl, hb);
    BNV_EPH(3);
    split_x<NPROD>(hb, sh, sl);
    BNV_EPH(4);
    layer128_x<NPROD>(L, PX_W3, 2, sh, sl, ha);
    BNV_EPH(5);
    split_x<NPROD>(ha, sh, sl);
    BNV_EPH(6);
    // ---- layer 4: 128 -> 8, one row block (rows >= 8 are zero weights); rows 4 g + i of lanes g >= 2 are unused
    f32x4 o[2];
    o[0] = o[1] = *(lds_f32x4_t*)(L.b + 384 * 4);
    {
      half8 w4h[4], w4l[4];
      __builtin_amdgcn_sched_barrier(0);  // keep these loads below layer 3 (register peak)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        w4h[s] = ldsx_wfrag(L, (PX_W4 + s * 2 * 64 * 8) * 2);
        if (NPROD == 3) w4l[s] = ldsx_wfrag(L, (PX_W4 + s * 2 * 64 * 8) * 2 + 1024);
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
          if constexpr (NPROD == 3) {
            o[cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w4l[s], sh[s][cb], o[cb], 0, 0, 0);
            o[cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w4h[s], sl[s][cb], o[cb], 0, 0, 0);
          }
          o[cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w4h[s], sh[s][cb], o[cb], 0, 0, 0);
        }
      }
    }
    // outputs of column block 1 back to the lanes that staged those pairs: lane (n, g) with g >= 2 takes features
    // 4 (g & 1) .. + 3 of pair 16 + n from lane l - 32
    f32x4 mine;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float other = __shfl(o[1][i], (lane + 32) & 63, 64);
      mine[i] = gk < 2 ? o[0][i] : other;
    }
    BNV_EPH(7);
    scatter_tile_x(mine, slot, n, gk, counts, acc);
    BNV_EPH(8);
  }
#ifdef BNV_PHASE_PROF
  if ((threadIdx.x & 63) < 15)
    atomicAdd(&g_enc_phase[(threadIdx.x >> 6) * 16 + (threadIdx.x & 63)],
              ((unsigned long long*)((char*)lds + PX_LDS_BYTES))[(threadIdx.x >> 6) * 16 + (threadIdx.x & 63)]);
#endif
}

int encode_init() {   // opt-in of this file's kernels to their dynamic LDS
  const hipFuncAttribute lds = hipFuncAttributeMaxDynamicSharedMemorySize;
  BNV_HIP_CHECK(hipFuncSetAttribute((const void*)k_pointnet_scatter, lds, PN_TOTAL * 4));
  BNV_HIP_CHECK(hipFuncSetAttribute((const void*)k_pointnet_scatter_x<3>, lds, PX_LDS_BYTES + kEncProfLds));
  BNV_HIP_CHECK(hipFuncSetAttribute((const void*)k_pointnet_scatter_x<1>, lds, PX_LDS_BYTES + kEncProfLds));
  return BNV_OK;
}

void launch_encoder_mlp(int mlp, int grid, const float* pts, int n, const bnv_grid_t& g, const float* pack,
                        const EncodeWs& ws, const int32_t* plist, hipStream_t stream) {
  if (mlp == 1 || mlp == 3)
    hipLaunchKernelGGL(mlp == 1 ? k_pointnet_scatter_x<3> : k_pointnet_scatter_x<1>, dim3(grid), dim3(512),
                       PX_LDS_BYTES + kEncProfLds, stream, pts, n, g, pack, ws.bitmap, ws.word_prefix, ws.counts,
                       ws.acc, &ws.ctl->error, plist, &ws.ctl->n_pairs);
  else
    hipLaunchKernelGGL(k_pointnet_scatter, dim3(grid), dim3(512), PN_TOTAL * 4, stream, pts, n, g, pack, ws.bitmap,
                       ws.word_prefix, ws.counts, ws.acc, plist, &ws.ctl->n_pairs);
}

}  // namespace bnv

#ifdef BNV_PHASE_PROF
extern "C" int bnv_dev_enc_phase_read(unsigned long long* out128) {
  BNV_HIP_CHECK(hipDeviceSynchronize());
  BNV_HIP_CHECK(hipMemcpyFromSymbol(out128, HIP_SYMBOL(bnv::g_enc_phase), 128 * sizeof(unsigned long long)));
  unsigned long long z[128] = {};
  BNV_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(bnv::g_enc_phase), z, sizeof(z)));
  return BNV_OK;
}
#endif
