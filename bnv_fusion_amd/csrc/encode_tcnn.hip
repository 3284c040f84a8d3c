// encode_tcnn.hip -- the point encoders of the reference's default tiny-cuda-nn checkpoint (MLP mode 2): per tile of 32
// (point, corner) pairs, and per block of 32 points for whole frames.  Pairs, slots and scatter: encode.hpp.
#include "encode.hpp"
#include "tcnn_mlp.hpp"

namespace bnv {

// k_pointnet_scatter_t: the tiny-cuda-nn point encoder of the reference's default checkpoint
// (pointnet_tcnn.ckpt; tcnnPointNetEncoder, pointnet_utils.py:269-294; FullyFusedMLP per
// src/models/tcnn_config.json): 6 inputs padded to 16 with 1.0 -> 64 -> 64 -> 64 -> 16 (first 8 used),
// ReLU, no bias, fp16 weights and activations.  Here: f16 MFMA with fp32 accumulation, activations
// rounded to f16 between layers and at the output, as the CUDA kernel stores them.
// Network, pack layout and wave tile: tcnn_mlp.hpp (NK0 = 1).
typedef TcnnPack<1> PointPack;

__global__ __launch_bounds__(256) void k_pointnet_scatter_t(
    const float* __restrict__ pts, int n_points, bnv_grid_t g, const float* __restrict__ wpack,
    const uint32_t* __restrict__ bitmap, const uint32_t* __restrict__ word_prefix,
    int32_t* __restrict__ counts, long long* __restrict__ acc, const int32_t* __restrict__ pair_list,
    const int32_t* __restrict__ n_pairs) {
  __shared__ __attribute__((aligned(16))) _Float16 wh[PointPack::TOTAL];
  stage_to_lds<256>(wpack, wh, PointPack::TOTAL * 2);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 31, h = lane >> 5;
  const PairTiles T = pair_tiles(n_points, pair_list, n_pairs);
  const int n_tiles = T.n_tiles;
  for (int t = blockIdx.x * 4 + wave; t < n_tiles; t += gridDim.x * 4) {
    int i = 0, k = 0;
    const bool have = tile_pair(T, t, j, &i, &k);
    // operand slots of this lane half: features 8 (jj >> 2) + 4 h + (jj & 3); inputs 0..5, the rest 1.0.  (Built here
    // and in k_pointnet_scatter_tb: through a shared inline function that kernel took 109 or more VGPRs for 104.)
    half8 b;
#pragma unroll
    for (int e = 0; e < 8; ++e) b[e] = (_Float16)1.0f;
    int slot = -1;
    if (have) {
      const float* p = pts + (size_t)i * 6;
      const float x = p[0], y = p[1], z = p[2];
      if (in_bounds(x, y, z, g)) {
        const float xn = voxel_coord(x, g.bound_min[0], g.voxel_size);
        const float yn = voxel_coord(y, g.bound_min[1], g.voxel_size);
        const float zn = voxel_coord(z, g.bound_min[2], g.voxel_size);
        int gx, gy, gz;
        const uint32_t id = corner_voxel(k, xn, yn, zn, g, gx, gy, gz);
        if (voxel_owner(gx, gy, gz, g) == g.shard_rank) slot = slot_rank(bitmap[id >> 5], word_prefix[id >> 5], id);
        if (h == 0) {
          b[0] = (_Float16)relative_coord(xn, gx, g.voxel_size);
          b[1] = (_Float16)relative_coord(yn, gy, g.voxel_size);
          b[2] = (_Float16)relative_coord(zn, gz, g.voxel_size);
          b[3] = (_Float16)p[3];
        } else {
          b[0] = (_Float16)p[4];
          b[1] = (_Float16)p[5];
        }
      }
    }
    if (__ballot(slot >= 0) == 0ULL) continue;
    const half8 x[1] = {b};
    f32x16 o = tcnn_forward<1>(wh, lane, x);
    // the network returns fp16; lane (j, h) holds outputs 4h .. 4h+3 of pair j
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = (float)(_Float16)o[q];
    scatter_tile(o, slot, j, h, counts, acc);
  }
}

// k_pointnet_scatter_tb: the tiny-cuda-nn encoder for WHOLE frames (unsharded encode), built around the scatter.
// With this small network the kernel's floor was its global atomics: 5.7 M device-scope 64-bit atomics per frame
// (366 MB of write traffic tallied at 64 B each) = 0.31 ms whatever the weights, against 0.22 ms without them
// (profiles/r02_power_probe.txt, r02_bench_line_tcnn.json).  Here a wave's unit of work is a BLOCK of 32 points --
// 8 x 4 pixels of the depth image when the frame's width is known, else 32 consecutive points -- with all EIGHT
// corner tiles of those points, and the per-voxel sums are formed in an LDS table before they go to the global
// accumulators (sums are integers: bit-identical in any order):
//  * the point is loaded and voxelised ONCE for its eight corners (3 + 6 IEEE divisions per point instead of 48:
//    the relative coordinate of an axis has two values, floor and ceil) and the 16 bitmap / prefix words of the
//    eight corners are requested together;
//  * the table (slot, count, 8 x i64; open addressing on a multiplicative hash of the slot, LDS compare-and-swap,
//    kAccProbes probes, then the run goes to the global accumulators itself) takes the run sums of the eight tiles
//    with LDS atomics.  How much that saves depends on the patch it covers -- measured on the bench frame (134 k
//    touched voxels): an 8 x 4 patch with its corners touches 40 voxels (383 k table entries per frame, each
//    flushed with 9 atomics), 8 x 8: 61 (295 k), 16 x 16: 173 (208 k), 32 x 16: 310 (186 k);
//  * SHARED = false (r03 first version): one 64-entry table per wave, flushed per block, no barrier;
//    SHARED = true: the workgroup's 8 waves take the 8 blocks of a 16 x 16 patch and share ONE 512-entry table,
//    flushed by all threads behind a barrier: 46 % fewer flushed entries for two barriers per patch.
//  512 threads share one copy of the weights (22.5 KB) + 36.9 KB of tables: two workgroups per CU.
// Sharded encodes (owned-pair list) keep k_pointnet_scatter_t.
constexpr int kAccProbes = 6;     // probes before a run goes to the global accumulators instead
constexpr int kAccCap = 64 * kTbWaves;
struct WgAcc {
  int key[kAccCap];
  int cnt[kAccCap];
  unsigned long long sum[kAccCap][8];
};

template <bool SHARED>
__global__ __launch_bounds__(64 * kTbWaves) void k_pointnet_scatter_tb(
    const float* __restrict__ pts, int n_points, int frame_w, bnv_grid_t g, const float* __restrict__ wpack,
    const uint32_t* __restrict__ bitmap, const uint32_t* __restrict__ word_prefix, int32_t* __restrict__ counts,
    long long* __restrict__ acc) {
  __shared__ __attribute__((aligned(16))) _Float16 wh[PointPack::TOTAL];
  __shared__ WgAcc T;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // the table region this wave inserts into: all of it, or its own 64 entries
  constexpr int kSpan = SHARED ? kAccCap : 64;
  constexpr int kHashShift = SHARED ? 32 - 9 : 32 - 6;
  static_assert(kAccCap == 512, "hash width");
  const int t_base = SHARED ? 0 : wave * 64;
  T.key[threadIdx.x] = -1;
  T.cnt[threadIdx.x] = 0;
#pragma unroll
  for (int f = 0; f < 8; ++f) T.sum[threadIdx.x][f] = 0ull;
  stage_to_lds<64 * kTbWaves>(wpack, wh, PointPack::TOTAL * 2);
  __syncthreads();
  const int j = lane & 31, h = lane >> 5;
  const int nyz = g.n_xyz[1] * g.n_xyz[2];
  const bool sharded = g.shard_world > 1;
  // blocks: 8 x 4 pixel patches of a frame_w-wide image, or runs of 32 points; a workgroup's 8 waves take the 2 x 4
  // blocks of a 16 x 16 patch (SHARED) or 8 consecutive blocks
  const bool image = frame_w > 0 && n_points % frame_w == 0;
  const int frame_h = image ? n_points / frame_w : 1;
  const int bw = image ? (frame_w + 7) >> 3 : 0, bh = image ? (frame_h + 3) >> 2 : 0;
  const int n_blocks = image ? bw * bh : (n_points + 31) >> 5;
  const int uw = (bw + 1) >> 1;
  const int n_units = (SHARED && image) ? uw * ((bh + 3) >> 2) : (n_blocks + kTbWaves - 1) / kTbWaves;
  // entry e of the table goes to the global accumulators and is empty again
  auto flush_entry = [&](int e) {
    const int key = T.key[e];
    if (key >= 0) {
      unsigned long long* dst = (unsigned long long*)acc + (uint32_t)key * 8u;
#pragma unroll
      for (int f = 0; f < 8; ++f) {
        atomicAdd(dst + f, T.sum[e][f]);
        T.sum[e][f] = 0ull;
      }
      atomicAdd(&counts[key], T.cnt[e]);
      T.key[e] = -1;
      T.cnt[e] = 0;
    }
  };
  for (int u = blockIdx.x; u < n_units; u += gridDim.x) {
    int i = -1;
    if (SHARED && image) {
      const int uy = u / uw, ux = u - uy * uw;
      const int by = uy * 4 + (wave >> 1), bx = ux * 2 + (wave & 1);
      const int x = bx * 8 + (j & 7), y = by * 4 + (j >> 3);
      if (bx < bw && x < frame_w && y < frame_h) i = y * frame_w + x;
    } else if (image) {
      const int b = u * kTbWaves + wave;
      const int by = b / bw, bx = b - by * bw;
      const int x = bx * 8 + (j & 7), y = by * 4 + (j >> 3);
      if (b < n_blocks && x < frame_w && y < frame_h) i = y * frame_w + x;
    } else if ((u * kTbWaves + wave) * 32 + j < n_points) {
      i = (u * kTbWaves + wave) * 32 + j;
    }
    bool valid = false;
    float px = 0.f, py = 0.f, pz = 0.f, n0 = 0.f, n1 = 0.f, n2 = 0.f;
    if (i >= 0) {
      const float* p = pts + (size_t)i * 6;
      px = p[0], py = p[1], pz = p[2], n0 = p[3], n1 = p[4], n2 = p[5];
      valid = in_bounds(px, py, pz, g);
    }
    if (__ballot(valid) != 0ULL) {
    // voxelisation of the point, once for its eight corners
    int lo3[3] = {0, 0, 0}, hi3[3] = {0, 0, 0};
    _Float16 rl[3], rh[3];     // relative coordinate of an axis towards its floor / ceil voxel, as the network takes it
    {
      const float c3[3] = {px, py, pz};
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float xn = valid ? voxel_coord(c3[a], g.bound_min[a], g.voxel_size) : 0.f;
        lo3[a] = (int)floorf(xn);
        hi3[a] = (int)ceilf(xn);
        rl[a] = (_Float16)relative_coord(xn, lo3[a], g.voxel_size);
        rh[a] = (_Float16)relative_coord(xn, hi3[a], g.voxel_size);
      }
    }
    // bitmap word + prefix of the eight corner voxels, all requested before the first is used
    uint32_t bw8[8], pf8[8], id8[8];
    bool own8[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int gx = (k & 1) ? hi3[0] : lo3[0], gy = (k & 2) ? hi3[1] : lo3[1], gz = (k & 4) ? hi3[2] : lo3[2];
      id8[k] = voxel_id(gx, gy, gz, nyz, g.n_xyz[2]);
      bw8[k] = 0u;
      pf8[k] = 0u;
      // sharded volume: only the pairs whose voxel this rank owns (ownership goes by 8^3-voxel blocks, a patch of
      // the image lies in one or two of them: most corner tiles are all or nothing and the others are skipped)
      own8[k] = valid && (!sharded || voxel_owner(gx, gy, gz, g) == g.shard_rank);
      if (own8[k]) {
        bw8[k] = bitmap[id8[k] >> 5];
        pf8[k] = word_prefix[id8[k] >> 5];
      }
    }
    const _Float16 hn0 = (_Float16)n0, hn1 = (_Float16)n1, hn2 = (_Float16)n2;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int slot = own8[k] ? slot_rank(bw8[k], pf8[k], id8[k]) : -1;
      if (sharded && __ballot(slot >= 0) == 0ULL) continue;     // nothing of this corner tile is ours
      half8 bop;
#pragma unroll
      for (int e = 0; e < 8; ++e) bop[e] = (_Float16)1.0f;
      if (valid) {
        if (h == 0) {
          bop[0] = (k & 1) ? rh[0] : rl[0];
          bop[1] = (k & 2) ? rh[1] : rl[1];
          bop[2] = (k & 4) ? rh[2] : rl[2];
          bop[3] = hn0;
        } else {
          bop[0] = hn1;
          bop[1] = hn2;
        }
      }
      const half8 x[1] = {bop};
      f32x16 o = tcnn_forward<1>(wh, lane, x);
      // the network returns fp16; lane (j, h) holds outputs 4h .. 4h+3 of pair j
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] = (float)(_Float16)o[q];
      unsigned long long v[4];
      bool is_end;
      int len;
      tile_run_sums(o, slot, j, h, v, is_end, len);
      if (slot >= 0 && is_end) {
        // the run's sums into the table (both halves of a pair probe the same way and meet in the same entry).
        // Slots are ranks of ascending voxel ids -- a z-run of voxels is a run of slots: the multiplicative hash
        // keeps the runs of different rows from piling into one probe chain
        int p = (int)(((uint32_t)slot * 0x9E3779B1u) >> kHashShift), found = -1;
        for (int probe = 0; probe < kAccProbes; ++probe) {
          const int old = atomicCAS(&T.key[t_base + p], -1, slot);
          if (old == -1 || old == slot) {
            found = t_base + p;
            break;
          }
          p = (p + 1) & (kSpan - 1);
        }
        if (found >= 0) {
#pragma unroll
          for (int q = 0; q < 4; ++q) atomicAdd(&T.sum[found][4 * h + q], v[q]);
          if (h == 0) atomicAdd(&T.cnt[found], len);
        } else {   // no room within kAccProbes probes: straight to the global accumulators (run_to_global spelt out: the call changes this kernel's code)
          unsigned long long* dst = (unsigned long long*)acc + ((uint32_t)slot * 8u + 4u * (uint32_t)h);
#pragma unroll
          for (int q = 0; q < 4; ++q) atomicAdd(dst + q, v[q]);
          if (h == 0) atomicAdd(&counts[slot], len);
        }
      }
    }
    }
    if constexpr (SHARED) {
      __syncthreads();            // every wave's runs are in the table
      flush_entry(threadIdx.x);
      __syncthreads();            // the table is empty before the next patch inserts
    } else {
      flush_entry(t_base + lane);
    }
  }
}

void launch_encoder_tcnn(bool blocks, int image_width, int grid, const float* pts, int n, const bnv_grid_t& g, const float* pack,
                         const EncodeWs& ws, const int32_t* plist, hipStream_t stream) {
  if (blocks) {   // (finds a shard's pairs itself: no plist)
    auto kern = g_tcnn_shared_table.load(std::memory_order_relaxed) ? k_pointnet_scatter_tb<true> : k_pointnet_scatter_tb<false>;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * kTbWaves), 0, stream, pts, n, image_width, g, pack, ws.bitmap,
                       ws.word_prefix, ws.counts, ws.acc);
  } else
    hipLaunchKernelGGL(k_pointnet_scatter_t, dim3(grid), dim3(256), 0, stream, pts, n, g, pack, ws.bitmap,
                       ws.word_prefix, ws.counts, ws.acc, plist, &ws.ctl->n_pairs);
}

}  // namespace bnv
