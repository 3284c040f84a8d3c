// encode.hip -- LitFusionPointNet.encode_pointcloud (reference local_point_fusion.py:81-165)
// as four gfx950 kernels (bnv_encode_begin = the first two, bnv_encode_finish = the last two).  Here: the chain around
// the point encoder and the entries; the encoder: encode_mlp.hip / encode_tcnn.hip; shared: encode.hpp; owners: shard.hip
//
//   k_mark / k_front_mark  points (or depth pixels: front end fused in, frontend.hpp) -> 8 corner voxels ->
//                     flag bytes in a grid byte map, plain stores, no atomics                 (HBM)
//   k_rank            one pass over the flagged chunks (decoupled look-back): bitmap words + popcount prefix --
//                     the rank of a voxel's bit IS its position in torch.unique's ascending output
//                     (replaces sort+unique)                                                   (HBM/L2)
//   k_pointnet_scatter[_x|_t]  per (point, corner) pair: 6->128->128->128->8 MLP on MFMA
//                     (transposed chaining: layer L's D registers are layer L+1's B operands, no
//                     cross-lane traffic), then order-independent 64-bit fixed-point atomics into
//                     per-voxel accumulators                                                   (MFMA)
//   k_finalize        mean, min-points filter, ordered compaction in one pass (look-back), unflatten,
//                     scratch cleanup, the frame's counters                                    (HBM)
#include "encode.hpp"
#include "frontend.hpp"
#include "scan.hpp"

namespace bnv {

// ------------------------------------------------------------------------------------------
// mark: one thread per point; flags its 8 corner voxels in the grid byte map
// ------------------------------------------------------------------------------------------
// One BYTE per voxel, written with plain stores: setting a flag is idempotent, so no atomic is needed, nothing is
// read back and nothing waits -- where the former bit map cost one visibility load + one device-scope atomicOr per
// (point, column): 32 us of a 42 us kernel (tools/probe_mark.hip: 4 us with byte stores).  A second byte per 64-voxel
// chunk lets k_rank find the touched chunks without reading the whole map (134 MB at 512^3).  ~20 pairs fall into each
// voxel and neighbouring pixels (= neighbouring lanes) mostly share it: a lane skips a column its predecessor writes.
// The number of valid points goes to valid_blocks[blockIdx.x] as a plain store: one atomicAdd per wave on a single
// counter serialises in the memory-side atomic unit at ~11 ns each -- 4,800 of them were 52 us per frame.
// Every thread of the (256-thread) workgroup must call this.  With pair_list set (sharded encode) the pairs this rank
// owns are listed as well (encode.hpp: list_owned_pairs).
__device__ __forceinline__ void mark_point(
    bool valid, float x, float y, float z, const bnv_grid_t& g, uint8_t* __restrict__ bytemap,
    uint8_t* __restrict__ chunk_flag, int32_t* __restrict__ valid_blocks, int point_index = 0,
    int32_t* __restrict__ pair_list = nullptr, int32_t* __restrict__ n_pairs = nullptr,
    int32_t* __restrict__ orphan_list = nullptr, int32_t* __restrict__ n_orphans = nullptr) {
  int fx = 0, cx = 0, fy = 0, cy = 0, fz = 0, cz = 0;
  if (valid) {
    const float xn = voxel_coord(x, g.bound_min[0], g.voxel_size);
    const float yn = voxel_coord(y, g.bound_min[1], g.voxel_size);
    const float zn = voxel_coord(z, g.bound_min[2], g.voxel_size);
    fx = (int)floorf(xn), cx = (int)ceilf(xn);
    fy = (int)floorf(yn), cy = (int)ceilf(yn);
    fz = (int)floorf(zn), cz = (int)ceilf(zn);
  }
  const int nyz = g.n_xyz[1] * g.n_xyz[2];
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int gx = (k & 1) ? cx : fx, gy = (k & 2) ? cy : fy;
    int a = valid ? (gx * nyz + gy * g.n_xyz[2] + fz) : -1;   // (floor == ceil duplicates just set the flag again)
    int b = valid ? a + (cz - fz) : -1;
    const int p0 = __shfl_up(a, 1), p1 = __shfl_up(b, 1);
    if (lane > 0 && p0 == a && p1 == b) continue;   // the previous lane flags the very same voxels
    if (a < 0) continue;
    bytemap[a] = 1;
    chunk_flag[a >> 6] = 1;
    if (b != a) {
      bytemap[b] = 1;
      if ((b >> 6) != (a >> 6)) chunk_flag[b >> 6] = 1;
    }
  }
  __shared__ int s_valid[4];
  const unsigned long long b = __ballot(valid);
  if (lane == 0) s_valid[threadIdx.x >> 6] = (int)__popcll(b);
  if (pair_list) {   // (workgroup-uniform)
    list_owned_pairs(valid, fx, cx, fy, cy, fz, cz, g, point_index, pair_list, n_pairs, orphan_list, n_orphans);
  } else {
    __syncthreads();
  }
  if (threadIdx.x == 0) valid_blocks[blockIdx.x] = s_valid[0] + s_valid[1] + s_valid[2] + s_valid[3];
}

__global__ __launch_bounds__(256) void k_mark(
    const float* __restrict__ pts, int n_points, bnv_grid_t g, uint8_t* __restrict__ bytemap,
    uint8_t* __restrict__ chunk_flag, int32_t* __restrict__ valid_blocks, int32_t* __restrict__ pair_list,
    int32_t* __restrict__ n_pairs, int32_t* __restrict__ orphan_list, int32_t* __restrict__ n_orphans) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool valid = false;
  float x = 0.f, y = 0.f, z = 0.f;
  if (i < n_points) {
    x = pts[(size_t)i * 6 + 0];
    y = pts[(size_t)i * 6 + 1];
    z = pts[(size_t)i * 6 + 2];
    valid = in_bounds(x, y, z, g);
  }
  mark_point(valid, x, y, z, g, bytemap, chunk_flag, valid_blocks, i, pair_list, n_pairs, orphan_list, n_orphans);
}

// The same, fused behind the depth front end (frontend.hpp): one thread per PIXEL computes the pixel's world point
// and normal in float64 as the reference's loader does, writes the float32 row of input_pts (NaN for an invalid
// pixel: rows stay in pixel order, nothing is compacted -- the encoder's bounds mask drops NaN rows wherever they
// are) and marks the point's voxels from the registers: the 7.4 MB of points are not read back, one launch less.
__global__ __launch_bounds__(256) void k_front_mark(
    FrontArgs a, float* __restrict__ out_pts, bnv_grid_t g, uint8_t* __restrict__ bytemap,
    uint8_t* __restrict__ chunk_flag, int32_t* __restrict__ valid_blocks, int32_t* __restrict__ pair_list,
    int32_t* __restrict__ n_pairs, int32_t* __restrict__ orphan_list, int32_t* __restrict__ n_orphans) {
  const int64_t n = (int64_t)a.H * a.W;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float p[6];
  bool have = false;
  if (i < n) have = front_point(a, (int)(i / a.W), (int)(i % a.W), p);
  if (i < n) {
    float* o = out_pts + (size_t)i * 6;
    typedef float f32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      f32x2 v;
      v[0] = have ? p[2 * r] : __builtin_nanf("");
      v[1] = have ? p[2 * r + 1] : __builtin_nanf("");
      *(f32x2*)(o + 2 * r) = v;
    }
  }
  const bool valid = have && in_bounds(p[0], p[1], p[2], g);
  mark_point(valid, p[0], p[1], p[2], g, bytemap, chunk_flag, valid_blocks, (int)i, pair_list, n_pairs, orphan_list,
             n_orphans);
}

// ------------------------------------------------------------------------------------------
// rank: sorted-unique without a sort.  One pass over the chunk flags (decoupled look-back over the workgroups); a
// flagged chunk's 64 voxel bytes become two bitmap words (and are cleared, with the flag, for the next frame):
// bitmap = one bit per touched voxel, word_prefix[w] = set bits before word w, ids[] = the set bits in ascending
// order (= torch.unique's output), ctl->n_unique = their number.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t bytes_to_bits16(const uint32_t (&v)[4]) {
  // 16 flag bytes (0 / 1) -> 16 bits: (b0 | b1 << 8 | b2 << 16 | b3 << 24) * 0x01020408 has b0..b3 in bits 24..27
  uint32_t r = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) r |= (((v[q] * 0x01020408u) >> 24) & 0xFu) << (4 * q);
  return r;
}

__global__ __launch_bounds__(kScanThreads) void k_rank(
    uint8_t* __restrict__ bytemap, uint8_t* __restrict__ chunk_flag, int64_t n_chunks,
    uint64_t* __restrict__ tile_state, uint32_t epoch, uint32_t* __restrict__ bitmap,
    uint32_t* __restrict__ word_prefix, int32_t* __restrict__ ids, int64_t max_unique, EncCtl* __restrict__ ctl,
    bnv_grid_t g, int32_t* __restrict__ defer_list) {
  __shared__ uint32_t wave_tot[kScanThreads / 64];
  __shared__ uint32_t s_excl;
  __shared__ int s_hist[64];
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const int64_t base = (int64_t)blockIdx.x * kRankTile + (int64_t)threadIdx.x * kRankItems;   // first chunk
  uint32_t flags = 0;
  if (base < n_chunks) flags = *(const uint32_t*)&chunk_flag[base];   // 4 chunk flags (n_chunks is a multiple of 4)
  uint32_t w[2 * kRankItems];
  uint32_t s = 0;
#pragma unroll
  for (int e = 0; e < kRankItems; ++e) {
    w[2 * e] = w[2 * e + 1] = 0u;
    if ((flags >> (8 * e)) & 0xffu) {
      u32x4* src = (u32x4*)&bytemap[(base + e) * 64];
      const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int hw = 0; hw < 2; ++hw) {
        const u32x4 lo = src[2 * hw], hi = src[2 * hw + 1];
        const uint32_t l4[4] = {lo[0], lo[1], lo[2], lo[3]}, h4[4] = {hi[0], hi[1], hi[2], hi[3]};
        w[2 * e + hw] = bytes_to_bits16(l4) | (bytes_to_bits16(h4) << 16);
        src[2 * hw] = z;       // consumed: clean for the next frame
        src[2 * hw + 1] = z;
      }
      s += __popc(w[2 * e]) + __popc(w[2 * e + 1]);
    }
  }
  if (flags) *(uint32_t*)&chunk_flag[base] = 0u;
  __shared__ int s_cur[64];
  if (g.shard_world > 1 && threadIdx.x < 64) {
    s_hist[threadIdx.x] = 0;
    s_cur[threadIdx.x] = 0;
  }
  uint32_t total;
  uint32_t run = block_exclusive_scan<kScanThreads>(s, wave_tot, &total);
  if (threadIdx.x < 64) {
    const uint32_t excl = lookback_exclusive(tile_state, (int)blockIdx.x, total, epoch);
    if (threadIdx.x == 0) {
      s_excl = excl;
      if (blockIdx.x == gridDim.x - 1) ctl->n_unique = (int32_t)(excl + total);
    }
  }
  __syncthreads();
  if (total == 0) return;  // nothing set in this tile: prefixes are never read for clear words
  run += s_excl;
  const int nyz = g.n_xyz[1] * g.n_xyz[2];
#pragma unroll
  for (int e = 0; e < 2 * kRankItems; ++e) {
    uint32_t bits = w[e];
    if (!bits) continue;
    const int64_t word = base * 2 + e;
    bitmap[word] = bits;
    word_prefix[word] = run;
    while (bits) {
      const int b = __ffs(bits) - 1;
      bits &= bits - 1;
      const int id = (int)(word * 32 + b);
      if (run < max_unique) ids[run] = id;
      else ctl->error = 1;
      ++run;
    }
  }
  if (g.shard_world > 1 && g.shard_state) {
    // first-touch ownership: the touched voxels of every block no frame has touched before are counted -- the
    // block's weight when k_shard_assign gives it an owner; the exchange bound follows in k_shard_own
    __syncthreads();
    ShardState S;
    shard_state_layout(g.n_xyz, g.shard_block_log2, (char*)g.shard_state, &S);
    const int sh = g.shard_block_log2, mb = (1 << sh) - 1;
    const int nby = (g.n_xyz[1] + mb) >> sh, nbz = (g.n_xyz[2] + mb) >> sh;
    const int64_t lo = s_excl, hi = (int64_t)s_excl + total < max_unique ? (int64_t)s_excl + total : max_unique;
    for (int64_t j = lo + threadIdx.x; j < hi; j += kScanThreads) {
      const int id = __hip_atomic_load(&ids[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int x = id / nyz, r = id - x * nyz, y = r / g.n_xyz[2], z = r - y * g.n_xyz[2];
      const int b = ((x >> sh) * nby + (y >> sh)) * nbz + (z >> sh);
      const uint8_t tb = S.table[b];
      // the frame's load per rank with the owners as they stand (region rule: who may take new territory)
      if (tb & kOwnAssigned) atomicAdd(&s_cur[tb & kOwnRank], 1);
      if (!(tb & kOwnTouched) && atomicAdd(&S.blk_w[b], 1u) == 0u) {
        // the block's first voxel: list the block (k_shard_assign sorts the list; past its capacity it scans the
        // weight table instead, so the count alone is what matters then)
        const uint32_t pos = (uint32_t)atomicAdd(&S.hdr->any_new, 1);
        if (pos < kNewListCap) S.new_list[pos] = (uint32_t)b;
      }
      // the exchange bound with the owners as they stand; a voxel next to a block that has no owner yet is left
      // to k_shard_own (behind this frame's k_shard_assign).  A frame without a new block defers nothing.
      const int st = shard_boundary_state(x, y, z, g);
      if (st == 1) atomicAdd(&s_hist[voxel_owner(x, y, z, g) & 63], 1);
      else if (st == 2) defer_list[atomicAdd(&ctl->n_deferred, 1)] = (int32_t)j;
    }
    __syncthreads();
    if (threadIdx.x < 64 && threadIdx.x < g.shard_world) {
      if (s_hist[threadIdx.x]) atomicAdd(&ctl->shard_boundary[threadIdx.x], s_hist[threadIdx.x]);
      if (s_cur[threadIdx.x]) atomicAdd(&S.hdr->cur[threadIdx.x], (uint32_t)s_cur[threadIdx.x]);
    }
  } else if (g.shard_world > 1) {
    // the exchange bound: touched BOUNDARY voxels per owner.  The set bits sit in a few threads (a thread holds 256
    // consecutive voxels), so the ~30 ownership hashes of a boundary test are spread over the workgroup: it walks
    // the ids it has just written (its own stretch of the sorted list), one voxel per thread and step
    __syncthreads();
    const int64_t lo = s_excl, hi = (int64_t)s_excl + total < max_unique ? (int64_t)s_excl + total : max_unique;
    for (int64_t j = lo + threadIdx.x; j < hi; j += kScanThreads) {
      const int id = __hip_atomic_load(&ids[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (written by other lanes of this workgroup)
      const int x = id / nyz, r = id - x * nyz, y = r / g.n_xyz[2], z = r - y * g.n_xyz[2];
      if (shard_is_boundary(x, y, z, g)) atomicAdd(&s_hist[voxel_owner(x, y, z, g) & 63], 1);
    }
    __syncthreads();
    if (threadIdx.x < 64 && threadIdx.x < g.shard_world && s_hist[threadIdx.x])
      atomicAdd(&ctl->shard_boundary[threadIdx.x], s_hist[threadIdx.x]);
  }
}

struct ValidFlags {  // 1 where the voxel in slot s is emitted
  const int32_t* counts;
  const int32_t* ids;
  bnv_grid_t g;
  int emit_all;
  __device__ uint32_t operator()(int64_t s) const {
    if (!emit_all && counts[s] < g.min_pts_in_grid) return 0;
    if (g.shard_world > 1) {
      const int id = ids[s];
      const int nyz = g.n_xyz[1] * g.n_xyz[2];
      const int x = id / nyz, r = id - x * nyz, y = r / g.n_xyz[2], z = r - y * g.n_xyz[2];
      if (voxel_owner(x, y, z, g) != g.shard_rank) return 0;
    }
    return 1;
  }
};

// ------------------------------------------------------------------------------------------
// finalize: mean, min-points filter, ORDERED compaction of the emitted voxels (one pass: decoupled look-back over the
// workgroups), unflatten, cleanup of the per-frame scratch; the workgroup of the last tile completes the frame's
// counters and clears the control block.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kFinTile) void k_finalize(
    bnv_grid_t g, int emit_all, uint32_t* __restrict__ bitmap, int32_t* __restrict__ ids, int32_t* __restrict__ counts,
    long long* __restrict__ acc, uint64_t* __restrict__ tile_state, uint32_t epoch, EncCtl* __restrict__ ctl,
    const int32_t* __restrict__ valid_blocks, int n_mark_blocks, float* __restrict__ out_feats,
    int64_t* __restrict__ out_pcounts, int64_t* __restrict__ out_flat, int64_t* __restrict__ out_grid,
    int64_t out_capacity, bnv_encode_counters_t* __restrict__ counters) {
  __shared__ uint32_t wave_tot[kFinTile / 64];
  __shared__ uint32_t s_excl;
  const int64_t n = ctl->n_unique;
  if (n == 0) {
    // no voxel touched (no point passed the bounds mask): workgroup 0 reports the empty frame
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      counters->n_valid_points = 0;
      counters->n_unique = 0;
      counters->n_out = 0;
      counters->n_avg_pts = 0.f;
      counters->error = ctl->error;
      counters->reserved[0] = counters->reserved[1] = counters->reserved[2] = 0;
      ctl->error = 0;
      ctl->n_pairs = 0;
      ctl->n_orphans = 0;
      ctl->n_deferred = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x < 64) ctl->shard_boundary[threadIdx.x] = 0;
    return;
  }
  // ONE slot per thread: consecutive threads read consecutive 64-byte accumulator rows (with 8 slots per thread
  // every thread walked its own 512-byte stretch and the kernel was latency-bound at 34 us for 25 MB)
  // The number of slots is only known on the device: the launch is sized for a few thousand tiles at most and the
  // workgroups stride over the tiles in increasing order (tile t waits for tile t - 1 only: a workgroup that is
  // behind never waits for one that is ahead).  It used to cover max_unique -- 9,600 workgroups at 640x480, of which
  // ~500 had a tile and the others read n_unique and left.
  for (int64_t tile = blockIdx.x; tile * kFinTile < n; tile += gridDim.x) {
  if (tile != (int64_t)blockIdx.x) __syncthreads();      // wave_tot / s_excl of the previous tile are no longer read
  const int64_t sl = tile * kFinTile + threadIdx.x;
  ValidFlags flags{counts, ids, g, emit_all};
  const uint32_t fl = sl < n ? flags(sl) : 0u;
  int id = 0, c = 0;
  long long a8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  // sharded encode: 1 / world of the touched voxels are this rank's; the accumulators of the others were never
  // written (count 0), so their 64-byte rows are neither read nor cleaned
  bool dirty = false;
  if (sl < n) {
    id = ids[sl];
    c = counts[sl];
    dirty = g.shard_world <= 1 || c != 0;
    if (dirty) {
      typedef long long i64x2 __attribute__((ext_vector_type(2)));
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const i64x2 v = *(const i64x2*)&acc[sl * 8 + 2 * q];
        a8[2 * q] = v[0];
        a8[2 * q + 1] = v[1];
      }
    }
  }
  uint32_t total;
  uint32_t run = block_exclusive_scan<kFinTile>(fl, wave_tot, &total);
  const bool last_tile = (tile + 1) * kFinTile >= n;
  if (threadIdx.x < 64) {
    const uint32_t excl = lookback_exclusive(tile_state, (int)tile, total, epoch);
    if (threadIdx.x == 0) s_excl = excl;
    if (last_tile) {
      // every other tile has published (so it has read ctl->n_unique): complete the counters, leave the
      // control block clean for the next frame
      int nv = 0;
      for (int b = threadIdx.x; b < n_mark_blocks; b += 64) nv += valid_blocks[b];
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) nv += __shfl_xor(nv, d, 64);
      if (threadIdx.x == 0) {
        const int32_t n_out = (int32_t)(excl + total);
        counters->n_valid_points = nv;
        counters->n_unique = (int32_t)n;
        counters->n_out = n_out;
        // n_avg_pts = mean over ALL U voxels of the pair count (local_point_fusion.py:143); every valid point
        // contributes exactly 8 pairs, so the fp32 sum torch.mean forms is exactly 8 * n_valid
        counters->n_avg_pts = __fdiv_rn((float)(8 * nv), (float)n);
        counters->error = ctl->error ? ctl->error : ((int64_t)n_out > out_capacity ? 2 : 0);
        counters->reserved[0] = ctl->n_pairs;   // sharded encode: the (point, corner) pairs this rank encoded
        counters->reserved[1] = counters->reserved[2] = 0;
        ctl->n_unique = 0;
        ctl->error = 0;
        ctl->n_pairs = 0;
        ctl->n_orphans = 0;
        ctl->n_deferred = 0;
      }
      ctl->shard_boundary[threadIdx.x] = 0;
    }
  }
  __syncthreads();
  if (sl >= n) continue;
  run += s_excl;
  if (fl && (int64_t)run < out_capacity) {
    const bool keep = c >= g.min_pts_in_grid;  // emit_all: features zeroed below min_pts (:126)
    const float inv_scale = 1.0f / kFixedScale;
    f32x4 o[2];
#pragma unroll
    for (int f = 0; f < 8; ++f) {
      // mean = sum / max(count, 1) (torch_scatter.scatter_mean); the fixed-point sum is exact
      const double sum = (double)a8[f] * (double)inv_scale;
      o[f >> 2][f & 3] = keep ? (float)(sum / (double)(c > 1 ? c : 1)) : 0.f;
    }
    *(f32x4*)&out_feats[(size_t)run * 8] = o[0];
    *(f32x4*)&out_feats[(size_t)run * 8 + 4] = o[1];
    out_pcounts[run] = c;
    out_flat[run] = id;
    const int nyz = g.n_xyz[1] * g.n_xyz[2];
    const int x = id / nyz, r = id - x * nyz, y = r / g.n_xyz[2], z = r - y * g.n_xyz[2];
    out_grid[(size_t)run * 3 + 0] = x;
    out_grid[(size_t)run * 3 + 1] = y;
    out_grid[(size_t)run * 3 + 2] = z;
  }
  // leave the scratch clean for the next frame
  if (dirty) {
    counts[sl] = 0;
    typedef long long i64x2 __attribute__((ext_vector_type(2)));
    const i64x2 z2 = {0, 0};
#pragma unroll
    for (int q = 0; q < 4; ++q) *(i64x2*)&acc[sl * 8 + 2 * q] = z2;
  }
  bitmap[id >> 5] = 0u;
  }
}

// ------------------------------------------------------------------------------------------
// k_voxelize_pairs (dense path + tests)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_voxelize_pairs(
    const float* __restrict__ pts, int n_points, bnv_grid_t g, int32_t* __restrict__ grid_ids,
    int64_t* __restrict__ flat_ids, float* __restrict__ rel_xyz, uint8_t* __restrict__ bound_mask) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_points) return;
  const float x = pts[(size_t)i * 6 + 0], y = pts[(size_t)i * 6 + 1], z = pts[(size_t)i * 6 + 2];
  if (bound_mask) bound_mask[i] = in_bounds(x, y, z, g) ? 1 : 0;
  const float xn = voxel_coord(x, g.bound_min[0], g.voxel_size);
  const float yn = voxel_coord(y, g.bound_min[1], g.voxel_size);
  const float zn = voxel_coord(z, g.bound_min[2], g.voxel_size);
  const int nyz = g.n_xyz[1] * g.n_xyz[2];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    int gx, gy, gz;
    corner_xyz(kCornerCeilBits[k], xn, yn, zn, gx, gy, gz);  // pair order follows the reference's corner order
    const size_t p = (size_t)k * n_points + i;
    if (grid_ids) {
      grid_ids[p * 3 + 0] = gx;
      grid_ids[p * 3 + 1] = gy;
      grid_ids[p * 3 + 2] = gz;
    }
    if (flat_ids) flat_ids[p] = (int64_t)(int)voxel_id(gx, gy, gz, nyz, g.n_xyz[2]);  // int32 arithmetic as the reference
    if (rel_xyz) {
      // relative_xyz = (xyz_normalized - grid_id) * voxel_size (local_point_fusion.py:163-164)
      rel_xyz[p * 3 + 0] = __fmul_rn(__fsub_rn(xn, (float)gx), g.voxel_size);
      rel_xyz[p * 3 + 1] = __fmul_rn(__fsub_rn(yn, (float)gy), g.voxel_size);
      rel_xyz[p * 3 + 2] = __fmul_rn(__fsub_rn(zn, (float)gz), g.voxel_size);
    }
  }
}

}  // namespace bnv

using namespace bnv;

// The tiny-cuda-nn block encoder finds a shard's pairs itself: `begin` then makes no pair list.  (begin and finish of
// one frame are called with the same grid, hence the same MLP mode: the mode follows the weight pack.)
static bool tcnn_blocks(const bnv_grid_t& g) {
  return mlp_mode_of(g.mlp_mode) == 2 && g_tcnn_block_encoder.load(std::memory_order_relaxed);
}
// the owned-pair list of a sharded encode; null where none is made (unsharded, block encoder)
static int32_t* pair_list_of(const EncodeWs& ws, const bnv_grid_t& g) {
  return (g.shard_world > 1 && !tcnn_blocks(g)) ? ws.pair_list : (int32_t*)nullptr;
}

// a mark kernel over n points (`in`: its arguments in front of the grid) with the frame's pair and orphan lists
template <typename K, typename... In>
static void launch_mark_points(K kernel, int64_t n, const EncodeWs& ws, const bnv_grid_t& g, hipStream_t stream, In... in) {
  hipLaunchKernelGGL(kernel, dim3(blocks_for(n, 256)), dim3(256), 0, stream, in..., g, ws.bytemap,
                     ws.chunk_flag, ws.valid_blocks, pair_list_of(ws, g), &ws.ctl->n_pairs,
                     g.shard_state ? ws.orphan_list : (int32_t*)nullptr, &ws.ctl->n_orphans);
}

// rank (sorted-unique); under first-touch ownership then: owners for the frame's new blocks, the owned-pair list and
// the exchange bound (`pts`: the frame's input_pts rows)
static int encode_rank(const EncodeWs& ws, const bnv_grid_t& g, const float* pts, int n_points, hipStream_t stream) {
  const int nb_chunks = (int)((ws.n_chunks + kRankTile - 1) / kRankTile);
  hipLaunchKernelGGL(k_rank, dim3(nb_chunks), dim3(kScanThreads), 0, stream, ws.bytemap, ws.chunk_flag, ws.n_chunks,
                     ws.tile_state, next_epoch(), ws.bitmap, ws.word_prefix, ws.ids, ws.max_unique, ws.ctl, g,
                     ws.defer_list);
  BNV_LAUNCH_CHECK();
  if (g.shard_world > 1 && g.shard_state) return launch_shard_own(ws, g, pts, n_points, pair_list_of(ws, g), stream);
  return BNV_OK;
}

static bool grid_ok(const bnv_grid_t& g) {
  return (int64_t)g.n_xyz[0] * g.n_xyz[1] * g.n_xyz[2] < (1LL << 31) && g.n_xyz[0] > 0 && g.n_xyz[1] > 0 &&
         g.n_xyz[2] > 0 && g.shard_world >= 1 && g.shard_world <= 64 && g.shard_rank >= 0 &&
         g.shard_rank < g.shard_world && mlp_mode_field_ok(g.mlp_mode);
}

// finish = PointNet + scatter (parts & 1), then mean + min-points filter + ordered compaction (parts & 2)
int bnv::encode_finish_parts(const float* input_pts, int64_t n_points, int image_width, const bnv_grid_t* grid_host,
                             const float* pointnet_pack, void* ws_ptr, size_t ws_bytes, int64_t ws_max_points,
                             float* out_feats, int64_t* out_pcounts, int64_t* out_flat_ids, int64_t* out_grid_ids,
                             int64_t out_capacity, int emit_all, bnv_encode_counters_t* counters, int max_workgroups,
                             int parts, bnv_stream_t stream_) {
  if (g_num_cus <= 0) return BNV_ERR_NOT_INITIALISED;
  if (image_width < 0 || max_workgroups < 0 || parts < 1 || parts > 3) return BNV_ERR_INVALID_ARGUMENT;
  if (!input_pts || !grid_host || !pointnet_pack || !ws_ptr || !counters || n_points < 0 ||
      n_points > (1 << 27) || ws_max_points < n_points)
    return BNV_ERR_INVALID_ARGUMENT;
  const bnv_grid_t g = *grid_host;
  if (!grid_ok(g)) return BNV_ERR_INVALID_ARGUMENT;
  hipStream_t stream = (hipStream_t)stream_;
  EncodeWs ws;
  if (encode_ws_layout(ws_max_points, g.n_xyz, (char*)ws_ptr, &ws) > ws_bytes) return BNV_ERR_WORKSPACE_TOO_SMALL;
  if (n_points == 0) {
    if (parts & 2) BNV_HIP_CHECK(hipMemsetAsync(counters, 0, sizeof(bnv_encode_counters_t), stream));
    return BNV_OK;
  }
  const int n = (int)n_points;
  // point encoder + scatter
  const int n_tiles = ((n + 31) / 32) * 8;
  const int reserve = g_reserve_cus.load(std::memory_order_relaxed);
  int grid_pn = g_num_cus - reserve > 0 ? g_num_cus - reserve : 1;
  if (max_workgroups > 0 && grid_pn > max_workgroups) grid_pn = max_workgroups;
  if (grid_pn > (n_tiles + 7) / 8) grid_pn = (n_tiles + 7) / 8;
  const int mlp = mlp_mode_of(g.mlp_mode);
  // sharded: owned pairs only -- from the list `begin` made, or (block encoder) by an ownership test in the kernel
  const int32_t* plist = pair_list_of(ws, g);
  if (parts & 1) {
    ProfScope prof(PROF_POINTNET, stream);
    if (tcnn_blocks(g)) {
      const int n_blocks = (n + 31) / 32 + 64;   // (an upper bound of the 8 x 4 patches as well, up to ragged edges)
      const int n_units = (n_blocks + kTbWaves - 1) / kTbWaves + 64;   // (16 x 16 patches: up to ragged edges)
      const int cus_tb = max_workgroups > 0 && max_workgroups < g_num_cus ? max_workgroups : g_num_cus;
      launch_encoder_tcnn(true, image_width, cus_tb * 2 < n_units ? cus_tb * 2 : n_units, input_pts, n, g,
                          pointnet_pack, ws, plist, stream);
    } else if (mlp == 2)
      launch_encoder_tcnn(false, 0, g_num_cus * 4 < (n_tiles + 3) / 4 ? g_num_cus * 4 : (n_tiles + 3) / 4, input_pts, n, g,
                          pointnet_pack, ws, plist, stream);
    else
      launch_encoder_mlp(mlp, grid_pn, input_pts, n, g, pointnet_pack, ws, plist, stream);
  }
  BNV_LAUNCH_CHECK();
  if (!(parts & 2)) return BNV_OK;
  // ordered compaction of the emitted voxels; the number of slots is only known on the device: a capped grid strides
  // over the tiles
  const int nb_max = (int)((ws.max_unique + kFinTile - 1) / kFinTile);
  // forward progress of the look-back needs every launched workgroup resident at once (a tile waits for its
  // predecessor's word): 1,024-thread workgroups, 2 per CU at most -- the option can lower the count, never raise it
  const int nb_res = 2 * g_num_cus;
  const int nb_opt = g_finalize_blocks.load(std::memory_order_relaxed);
  const int nb_cap = nb_opt > 0 && nb_opt < nb_res ? nb_opt : nb_res;
  const int nb_u = nb_max < nb_cap ? nb_max : nb_cap;
  hipLaunchKernelGGL(k_finalize, dim3(nb_u), dim3(kFinTile), 0, stream, g, emit_all, ws.bitmap, ws.ids,
                     ws.counts, ws.acc, ws.tile_state, next_epoch(), ws.ctl, ws.valid_blocks, (n + 255) / 256, out_feats,
                     out_pcounts, out_flat_ids, out_grid_ids, out_capacity, counters);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

// ==========================================================================================
// C ABI
// ==========================================================================================
extern "C" {

size_t bnv_pointnet_pack_floats(void) { return PN_PACK_FLOATS; }

size_t bnv_encode_workspace_bytes(int64_t max_points, const int32_t n_xyz[3]) {
  return encode_ws_layout(max_points, n_xyz, nullptr, nullptr);
}

size_t bnv_encode_shard_counts_offset(void) { return offsetof(EncCtl, shard_boundary); }

// ---- encode in two halves.  begin = voxelise (bounds mask, 8 corner voxels, bitmap) + sorted-unique (rank);
// finish = PointNet + scatter-mean + min-points filter + ordered compaction.  Everything between the two lives in
// the workspace; bnv_encode_pointcloud is begin + finish.

int bnv_encode_begin(const float* input_pts, int64_t n_points, const bnv_grid_t* grid_host, void* ws_ptr,
                     size_t ws_bytes, int64_t ws_max_points, bnv_stream_t stream_) {
  if (g_num_cus <= 0) return BNV_ERR_NOT_INITIALISED;
  if (!input_pts || !grid_host || !ws_ptr || n_points < 0 || n_points > (1 << 27) || ws_max_points < n_points)
    return BNV_ERR_INVALID_ARGUMENT;
  const bnv_grid_t g = *grid_host;
  if (!grid_ok(g)) return BNV_ERR_INVALID_ARGUMENT;
  hipStream_t stream = (hipStream_t)stream_;
  EncodeWs ws;
  // the layout is a function of the workspace's capacity, not of this frame's point count, so
  // the scratch the previous frame left clean stays where this frame expects it
  if (encode_ws_layout(ws_max_points, g.n_xyz, (char*)ws_ptr, &ws) > ws_bytes) return BNV_ERR_WORKSPACE_TOO_SMALL;
  if (n_points == 0) return BNV_OK;
  const int n = (int)n_points;
  launch_mark_points(k_mark, n, ws, g, stream, input_pts, n);
  BNV_LAUNCH_CHECK();
  return encode_rank(ws, g, input_pts, n, stream);
}

int bnv_encode_begin_depth(const void* depth, int depth_dtype, int H, int W, const double* intr_host,
                           const double* T_wc_host, double max_depth, const uint8_t* conf, int conf_level,
                           const bnv_grid_t* grid_host, void* ws_ptr, size_t ws_bytes, int64_t ws_max_points,
                           float* out_pts, bnv_stream_t stream_) {
  if (g_num_cus <= 0) return BNV_ERR_NOT_INITIALISED;
  if (!depth || !intr_host || !T_wc_host || !grid_host || !ws_ptr || !out_pts || H <= 0 || W <= 0 || depth_dtype < 0 ||
      depth_dtype > 2 || (int64_t)H * W > (1 << 27) || ws_max_points < (int64_t)H * W ||
      !front_conf_args_ok(conf, conf_level))
    return BNV_ERR_INVALID_ARGUMENT;
  const bnv_grid_t g = *grid_host;
  if (!grid_ok(g)) return BNV_ERR_INVALID_ARGUMENT;
  hipStream_t stream = (hipStream_t)stream_;
  EncodeWs ws;
  if (encode_ws_layout(ws_max_points, g.n_xyz, (char*)ws_ptr, &ws) > ws_bytes) return BNV_ERR_WORKSPACE_TOO_SMALL;
  FrontArgs a;
  front_args_fill(a, depth, depth_dtype, H, W, intr_host, T_wc_host, max_depth);
  a.conf = conf;
  a.conf_level = conf_level;
  const int64_t n = (int64_t)H * W;
  launch_mark_points(k_front_mark, n, ws, g, stream, a, out_pts);
  BNV_LAUNCH_CHECK();
  return encode_rank(ws, g, out_pts, (int)n, stream);
}

int bnv_encode_finish(const float* input_pts, int64_t n_points, int image_width, const bnv_grid_t* grid_host,
                      const float* pointnet_pack, void* ws_ptr, size_t ws_bytes, int64_t ws_max_points,
                      float* out_feats, int64_t* out_pcounts, int64_t* out_flat_ids, int64_t* out_grid_ids,
                      int64_t out_capacity, int emit_all, bnv_encode_counters_t* counters, bnv_stream_t stream) {
  return encode_finish_parts(input_pts, n_points, image_width, grid_host, pointnet_pack, ws_ptr, ws_bytes,
                             ws_max_points, out_feats, out_pcounts, out_flat_ids, out_grid_ids, out_capacity, emit_all,
                             counters, 0, 3, stream);
}

int bnv_encode_pointcloud(const float* input_pts, int64_t n_points, const bnv_grid_t* grid_host,
                          const float* pointnet_pack, void* ws_ptr, size_t ws_bytes, int64_t ws_max_points,
                          float* out_feats,
                          int64_t* out_pcounts, int64_t* out_flat_ids, int64_t* out_grid_ids,
                          int64_t out_capacity, int emit_all, bnv_encode_counters_t* counters,
                          bnv_stream_t stream) {
  if (!pointnet_pack || !counters) return BNV_ERR_INVALID_ARGUMENT;
  const int rc = bnv_encode_begin(input_pts, n_points, grid_host, ws_ptr, ws_bytes, ws_max_points, stream);
  if (rc != BNV_OK) return rc;
  return bnv_encode_finish(input_pts, n_points, 0, grid_host, pointnet_pack, ws_ptr, ws_bytes, ws_max_points, out_feats,
                           out_pcounts, out_flat_ids, out_grid_ids, out_capacity, emit_all, counters, stream);
}

int bnv_voxelize_pairs(const float* input_pts, int64_t n_points, const bnv_grid_t* grid_host,
                       int32_t* grid_ids, int64_t* flat_ids, float* rel_xyz, uint8_t* bound_mask,
                       bnv_stream_t stream) {
  if (!input_pts || !grid_host || n_points < 0 || n_points > (1 << 27)) return BNV_ERR_INVALID_ARGUMENT;
  if (n_points == 0) return BNV_OK;
  hipLaunchKernelGGL(k_voxelize_pairs, dim3(blocks_for(n_points, 256)), dim3(256), 0,
                     (hipStream_t)stream, input_pts, (int)n_points, *grid_host, grid_ids, flat_ids, rel_xyz,
                     bound_mask);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

}  // extern "C"
