// encode.hpp -- what encode.hip, encode_mlp.hip, encode_tcnn.hip and shard.hip share: the packed weights' layout, the
// workspace, the pair tiles, and the device helpers every point encoder is built from (corner voxel -> slot, run sums ->
// accumulators).
#pragma once
#include "bnv_common.hpp"
#include "shard.hpp"
#include "workspace.hpp"

namespace bnv {

// ---- packed point-encoder weights (floats) ----------------------------------------------------------------------
constexpr int PN_W1 = 0;                        // [3 kstep][4 mb][64 lane]
constexpr int PN_W2 = PN_W1 + 3 * 4 * 64;       // [4 mb][4 nb][4 rq][64 lane][4]
constexpr int PN_W3 = PN_W2 + 128 * 128;        // same
constexpr int PN_W4 = PN_W3 + 128 * 128;        // [4 nb][4 rq][2 h][8 n][4]
constexpr int PN_B1 = PN_W4 + 4 * 4 * 2 * 8 * 4;  // [128]
constexpr int PN_B2 = PN_B1 + 128;
constexpr int PN_B3 = PN_B2 + 128;
constexpr int PN_B4 = PN_B3 + 128;              // [8]
constexpr int PN_TOTAL = PN_B4 + 8;             // 34,952 floats = 139,808 B of LDS

// split-operand pack of the f16 modes (appended to the same pack, units: 16-bit halves from float offset PN_TOTAL),
// operand order of v_mfma_f32_16x16x32_f16 (k_pointnet_scatter_x)
constexpr int PX_W1 = 0;                          // [8 rb][hi/lo][64 lane][8]
constexpr int PX_W2 = PX_W1 + 8 * 2 * 64 * 8;     // [4 s][8 rb][hi/lo][64 lane][8]
constexpr int PX_W3 = PX_W2 + 4 * 8 * 2 * 64 * 8;
constexpr int PX_W4 = PX_W3 + 4 * 8 * 2 * 64 * 8; // [4 s][hi/lo][64 lane][8], rows >= 8 zero
constexpr int PX_TOTAL = PX_W4 + 4 * 2 * 64 * 8;  // 77,824 halves = 155,648 B
constexpr int PX_OFF = PN_TOTAL;                  // float offset of the PX pack in the packed weights
constexpr int PN_CERT = PN_TOTAL + PX_TOTAL / 2;  // [4]: certified bound on |normal component| of the split modes
constexpr int PN_PACK_FLOATS = PN_CERT + 4;
constexpr int PX_LDS_BYTES = PX_TOTAL * 2 + (128 * 3 + 8) * 4 + 32;  // halves + fp32 biases + tile counter (+ pad: lanes g = 3 read 16 B past b4) = 157,248 B

constexpr float kFixedScale = 4294967296.0f;    // 2^32: per-voxel sums are exact integers

// ---- workspace layout -------------------------------------------------------------------------------------------
// Control block: the first 512 bytes of the workspace.  All-zero between frames (k_finalize's closing workgroup
// leaves it so), so no kernel of a frame needs a memset in front of it.
struct EncCtl {
  int32_t n_pairs;             // sharded encode: (point, corner) pairs whose voxel this rank owns (mark kernel)
  int32_t n_unique;            // U: touched voxels (k_rank)
  int32_t error;               // != 0: a capacity was exceeded
  int32_t n_orphans;           // first-touch ownership: points with a corner voxel in a block that has no owner yet
  int32_t n_deferred;          // first-touch ownership: touched voxels whose boundary test waits for k_shard_assign
  int32_t pad[11];
  int32_t shard_boundary[64];  // sharded encode: touched BOUNDARY voxels owned by each rank (k_rank) -- an upper
                               // bound of the boundary records that rank will exchange for this frame, known on
                               // every rank (the voxelisation is replicated) before the encoder MLP starts
};
static_assert(align256(sizeof(EncCtl)) == 512, "control block");

struct EncodeWs {
  EncCtl* ctl;
  uint64_t* tile_state;   // [n_tiles] look-back state of k_rank / k_finalize (epoch-tagged, never cleared)
  int32_t* valid_blocks;  // [ceil(max_points / 256)] points that passed the bounds mask, per workgroup of the mark kernel
  int32_t* pair_list;     // [8 * max_points] sharded encode: (point << 3 | corner) of the pairs this rank owns
  int32_t* orphan_list;   // [max_points] first-touch ownership: points the mark kernel could not decide (k_shard_own)
  int32_t* defer_list;    // [max_unique] first-touch ownership: slots whose boundary test k_rank could not decide
  uint8_t* bytemap;       // [n_words * 32] one byte per voxel: set by the mark kernel, consumed and cleared by k_rank
  uint8_t* chunk_flag;    // [n_chunks] one byte per 64 voxels (2 bitmap words): any byte of the chunk set
  uint32_t* bitmap;       // [n_words] one bit per touched voxel: k_rank writes, the encoder reads, k_finalize clears
  uint32_t* word_prefix;  // [n_words]
  int32_t* ids;           // [max_unique] flat voxel id of slot s (ascending)
  int32_t* counts;        // [max_unique]
  long long* acc;         // [max_unique][8] fixed-point feature sums
  int64_t n_words;
  int64_t n_chunks;       // n_words / 2
  int64_t max_unique;
  int64_t n_tiles;
};

constexpr int kScanThreads = 256;
#ifndef BNV_FIN_THREADS
#define BNV_FIN_THREADS 1024
#endif
constexpr int kFinTile = BNV_FIN_THREADS;              // slots per workgroup (k_finalize: one per thread)
constexpr int kTbWaves = 8;   // k_pointnet_scatter_tb: waves per workgroup = 8 x 4-pixel blocks per 16 x 16 patch
constexpr int kRankItems = 4;
constexpr int kRankTile = kScanThreads * kRankItems;  // 1024 chunks (of 64 voxels = 2 bitmap words) per workgroup (k_rank)

static size_t encode_ws_layout(int64_t max_points, const int32_t n_xyz[3], char* base, EncodeWs* ws) {
  const int64_t nvox = (int64_t)n_xyz[0] * n_xyz[1] * n_xyz[2];
  const int64_t n_words = ((nvox + 31) / 32 + 7) / 8 * 8;   // whole chunks, whole u32x4 of chunk flags
  const int64_t n_chunks = n_words / 2;
  int64_t max_unique = 8 * max_points;
  if (max_unique > nvox) max_unique = nvox;
  if (max_unique < 1) max_unique = 1;
  const int64_t nb_words = (n_chunks + kRankTile - 1) / kRankTile;
  const int64_t nb_unique = (max_unique + kFinTile - 1) / kFinTile;
  const int64_t n_tiles = nb_words > nb_unique ? nb_words : nb_unique;
  const int64_t points = max_points > 0 ? max_points : 1;
  Carver c(base);
  EncodeWs w;   // (the pieces in the order they lie in the workspace)
  w.ctl = c.take<EncCtl>(1);   // control block first: its offset does not depend on the sizes
  w.tile_state = c.take<uint64_t>(n_tiles);
  w.valid_blocks = c.take<int32_t>((max_points + 255) / 256 + 1);
  w.pair_list = c.take<int32_t>(points * 8);
  w.orphan_list = c.take<int32_t>(points);
  w.bytemap = c.take<uint8_t>(n_words * 32);
  w.chunk_flag = c.take<uint8_t>(n_chunks);
  w.bitmap = c.take<uint32_t>(n_words);
  w.word_prefix = c.take<uint32_t>(n_words);
  w.ids = c.take<int32_t>(max_unique);
  w.counts = c.take<int32_t>(max_unique);
  w.acc = c.take<long long>(max_unique * 8);
  w.defer_list = c.take<int32_t>(max_unique);
  w.n_words = n_words, w.n_chunks = n_chunks, w.max_unique = max_unique, w.n_tiles = n_tiles;
  if (ws) *ws = w;
  return c.bytes();
}

// ---- corner k of the point at normalised coordinates (xn, yn, zn): ceil on x / y / z where bit 0 / 1 / 2 of k is set,
// else floor -> its voxel (gx, gy, gz) and flat id (int32 arithmetic as the reference).  corner_voxel is the two parts
// together; a kernel that must keep the id behind its ownership test calls them one by one. -------------------------
__device__ __forceinline__ void corner_xyz(int k, float xn, float yn, float zn, int& gx, int& gy, int& gz) {
  gx = (k & 1) ? (int)ceilf(xn) : (int)floorf(xn);
  gy = (k & 2) ? (int)ceilf(yn) : (int)floorf(yn);
  gz = (k & 4) ? (int)ceilf(zn) : (int)floorf(zn);
}
__device__ __forceinline__ uint32_t voxel_id(int gx, int gy, int gz, int nyz, int nz) {
  return (uint32_t)(gx * nyz + gy * nz + gz);
}
__device__ __forceinline__ uint32_t corner_voxel(int k, float xn, float yn, float zn, const bnv_grid_t& g, int& gx,
                                                 int& gy, int& gz) {
  corner_xyz(k, xn, yn, zn, gx, gy, gz);
  return voxel_id(gx, gy, gz, g.n_xyz[1] * g.n_xyz[2], g.n_xyz[2]);
}
// accumulator slot of a touched voxel: the rank of its bit (k_rank), from its bitmap word and that word's prefix.
// Apart from corner_voxel: the encoders request the two words of several voxels before they rank the first.
__device__ __forceinline__ int slot_rank(uint32_t word, uint32_t prefix, uint32_t id) {
  return (int)(prefix + __popc(word & ((1u << (id & 31)) - 1u)));
}

// Spatial sharding (g.shard_world > 1): the (point, corner) pairs of a 256-thread workgroup's points whose voxel THIS
// rank owns are appended to pair_list as (point << 3 | corner), in (corner, point) order so that neighbouring pixels
// stay neighbours and the encoder's wave-level run reduction keeps working.  The encoder forms its tiles from the list:
// 1 / world of the pairs instead of every tile that holds at least one owned pair (with 8^3-voxel blocks that was
// ~60 % of the tiles at world 8).  One atomicAdd per WORKGROUP on the list counter; every thread of the workgroup must
// call this (two barriers).
// First-touch ownership, mark kernel (orphan_list set): a point with a corner voxel in a block that has no owner YET
// (the frame's k_shard_assign has not run) lists nothing here and goes to orphan_list; k_shard_own lists its pairs
// once the owners are known.  A frame that touches no new block has no orphan.
__device__ __forceinline__ void list_owned_pairs(
    bool valid, int fx, int cx, int fy, int cy, int fz, int cz, const bnv_grid_t& g, int point_index,
    int32_t* __restrict__ pair_list, int32_t* __restrict__ n_pairs, int32_t* __restrict__ orphan_list = nullptr,
    int32_t* __restrict__ n_orphans = nullptr) {
  const int lane = threadIdx.x & 63;
  __shared__ int s_cnt[32];   // [corner][wave] owned pairs
  unsigned long long own[8];
  int owner8[8];
  bool orphan = false;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int gx = (k & 1) ? cx : fx, gy = (k & 2) ? cy : fy, gz = (k & 4) ? cz : fz;
    owner8[k] = valid ? voxel_owner(gx, gy, gz, g) : -2;
    orphan |= owner8[k] == -1;
  }
  if (orphan_list) {   // (workgroup-uniform)
    const unsigned long long ob = __ballot(orphan);
    if (ob) {
      int base = 0;
      if (lane == 0) base = atomicAdd(n_orphans, (int)__popcll(ob));
      base = __shfl(base, 0, 64);
      if (orphan) orphan_list[base + (int)__popcll(ob & ((1ull << lane) - 1ull))] = point_index;
    }
    if (orphan) valid = false;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    own[k] = __ballot(valid && owner8[k] == g.shard_rank);
    if (lane == 0) s_cnt[k * 4 + (threadIdx.x >> 6)] = (int)__popcll(own[k]);
  }
  __syncthreads();
  if (threadIdx.x < 64) {   // exclusive prefix of the 32 counts (first wave), then the workgroup's place in the list
    const int c = threadIdx.x < 32 ? s_cnt[threadIdx.x] : 0;
    int incl = c;
#pragma unroll
    for (int d = 1; d < 32; d <<= 1) {
      const int o = __shfl_up(incl, d, 64);
      if ((int)threadIdx.x >= d) incl += o;
    }
    const int total = __shfl(incl, 31, 64);
    int base = 0;
    if (threadIdx.x == 0 && total) base = atomicAdd(n_pairs, total);
    base = __shfl(base, 0, 64);
    if (threadIdx.x < 32) s_cnt[threadIdx.x] = base + incl - c;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if ((own[k] >> lane) & 1ull)
      pair_list[s_cnt[k * 4 + (threadIdx.x >> 6)] + (int)__popcll(own[k] & ((1ull << lane) - 1ull))] =
          (point_index << 3) | k;
}

// Tiles of the point encoder: 32 (point, corner) pairs.  Unsharded: tile t = corner t / n_pblocks of the 32 consecutive
// points of block t % n_pblocks.  Sharded: 32 consecutive entries of the owned-pair list the mark kernel built.
struct PairTiles {
  const int32_t* list;   // null: unsharded
  int n_pairs, n_points, n_pblocks, n_tiles;
};
__device__ __forceinline__ PairTiles pair_tiles(int n_points, const int32_t* __restrict__ pair_list,
                                                const int32_t* __restrict__ n_pairs) {
  PairTiles T;
  T.list = pair_list;
  T.n_points = n_points;
  T.n_pblocks = (n_points + 31) >> 5;
  T.n_pairs = pair_list ? *n_pairs : 0;
  T.n_tiles = pair_list ? (T.n_pairs + 31) >> 5 : T.n_pblocks * 8;
  return T;
}
// pair j of tile t -> point index and corner; false past the end
__device__ __forceinline__ bool tile_pair(const PairTiles& T, int t, int j, int* i, int* k) {
  if (T.list) {
    const int e = t * 32 + j;
    if (e >= T.n_pairs) return false;
    const int p = T.list[e];
    *i = p >> 3;
    *k = p & 7;
    return true;
  }
  *k = t / T.n_pblocks;
  *i = (t - *k * T.n_pblocks) * 32 + j;
  return *i < T.n_points;
}

// ---- scatter: a tile's outputs -> run sums -> per-voxel accumulators -------------------------------------------
// f -> rndne(f * 2^32) as a 64-bit integer in two halves, in 8 VALU ops: r = rndne(f * 2^32) is an integer-valued float
// (|r| < 2^63 for |feature| < 2^31), hi = floor(r / 2^32) is exact (a power-of-two scaling, then floor) and so is
// lo = r - hi * 2^32, in [0, 2^32) -- the same integer llrintf gives, without the generic f32 -> i64 conversion sequence
__device__ __forceinline__ void fixed_hi_lo(float f, uint32_t& hi, uint32_t& lo) {
  const float r = __builtin_rintf(f * kFixedScale);
  const float hf = __builtin_floorf(r * (1.0f / kFixedScale));
  hi = (uint32_t)(int)hf;
  lo = (uint32_t)__builtin_fmaf(hf, -kFixedScale, r);
}

// Inclusive prefix of four 64-bit values (lo / hi registers) over the 16 lanes of every DPP row: an add / add-with-carry
// pair per value and step.  ONE asm statement -- asm volatile(BNV_SCAN_ROWS [further steps] : BNV_SCAN_REGS(lo, hi) : :
// "vcc") -- because DPP reads need two wait states behind the VALU write of their source (every register is re-read
// eight instructions after it was written, s_nop 1 covers the entry) and the compiler sees no hazard inside inline asm.
// (The three macros stay defined behind this header: encode_mlp.hip's scatter_tile_x issues the same scan.)
#define BNV_SCAN_STEP(ctrl)                                                      \
  "v_add_co_u32_dpp %0, vcc, %0, %0 " ctrl "\n"                                  \
  "v_addc_co_u32_dpp %1, vcc, %1, %1, vcc " ctrl "\n"                            \
  "v_add_co_u32_dpp %2, vcc, %2, %2 " ctrl "\n"                                  \
  "v_addc_co_u32_dpp %3, vcc, %3, %3, vcc " ctrl "\n"                            \
  "v_add_co_u32_dpp %4, vcc, %4, %4 " ctrl "\n"                                  \
  "v_addc_co_u32_dpp %5, vcc, %5, %5, vcc " ctrl "\n"                            \
  "v_add_co_u32_dpp %6, vcc, %6, %6 " ctrl "\n"                                  \
  "v_addc_co_u32_dpp %7, vcc, %7, %7, vcc " ctrl "\n"
#define BNV_SCAN_ROWS                                                            \
  "s_nop 1\n"                                                                    \
  BNV_SCAN_STEP("row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1")             \
  BNV_SCAN_STEP("row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1")             \
  BNV_SCAN_STEP("row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1")             \
  BNV_SCAN_STEP("row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1")
#define BNV_SCAN_REGS(lo, hi) \
  "+v"(lo[0]), "+v"(hi[0]), "+v"(lo[1]), "+v"(hi[1]), "+v"(lo[2]), "+v"(hi[2]), "+v"(lo[3]), "+v"(hi[3])

// Run sums of one tile: lane (j, h) holds output features 4h .. 4h+3 of pair j.  Consecutive pairs are
// neighbouring pixels and mostly fall into the same voxel, so the tile's values are summed per RUN of equal slots
// and only the last lane of a run issues the atomics (bit-identical to per-pair atomics: the sums are integers).
// The kernel is bound by instruction issue, not by the MFMA pipe (tools/phase_prof.py), so
// this is written for instruction count:
//  * 2^32 fixed point by fixed_hi_lo;
//  * ONE unsegmented inclusive prefix sum P over the 32 lanes of a half (5 DPP steps: row_shr 1, 2, 4, 8 and
//    row_bcast:15, no LDS crossbar traffic), then run [s, e] = P[e] - P[s - 1] in modular arithmetic: lanes of other
//    runs -- invalid ones included -- cancel exactly, so nothing is masked; one ds_bpermute per register fetches P[s - 1];
//  * the run's pair count is its length.
// (Round 1's segmented Hillis-Steele scan over ds_bpermute took ~300 instructions per tile; this takes ~110.)
// Used where lane = (pair j, feature half h): the exact-fp32 and the tiny-cuda-nn encoders; the split modes have their
// own tile shape (encode_mlp.hip: scatter_tile_x).
// -> for the LAST lane of every run of equal slots: v[q] = the run's sum of output 4 h + q (2^32 fixed point), len = its
// pair count; is_end tells whether this lane is such a lane (lanes with slot < 0 form runs too: the caller skips them)
__device__ __forceinline__ void tile_run_sums(const f32x16& o, int slot, int j, int h, unsigned long long (&v)[4],
                                              bool& is_end, int& len) {
  uint32_t lo[4], hi[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) fixed_hi_lo(o[q], hi[q], lo[q]);
  asm volatile(BNV_SCAN_ROWS BNV_SCAN_STEP("row_bcast:15 row_mask:0xa bank_mask:0xf") : BNV_SCAN_REGS(lo, hi) : : "vcc");
  // run geometry from the heads mask of the half: head = first lane of a run
  const int prev = __builtin_amdgcn_update_dpp(0, slot, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
  const unsigned long long heads64 = __ballot(j == 0 || prev != slot);
  const uint32_t heads = h ? (uint32_t)(heads64 >> 32) : (uint32_t)heads64;
  const int s = 31 - __clz((int)(heads & (0xffffffffu >> (31 - j))));   // head of this lane's run (bit 0 is set)
  is_end = j == 31 || ((heads >> (j + 1)) & 1u);
  len = j - s + 1;
  const int src = (h * 32 + (s > 0 ? s - 1 : 0)) * 4;                      // lane holding P[s - 1]
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t plo = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)lo[q]);
    const uint32_t phi = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)hi[q]);
    v[q] = ((unsigned long long)hi[q] << 32) | lo[q];
    if (s > 0) v[q] -= ((unsigned long long)phi << 32) | plo;
  }
}

// a run's last lane adds its four sums (features 4 fh .. 4 fh + 3) to the voxel's accumulators, half 0 its length to the count
__device__ __forceinline__ void run_to_global(long long* __restrict__ acc, int32_t* __restrict__ counts, int slot,
                                              int fh, const unsigned long long (&v)[4], int len) {
  unsigned long long* dst = (unsigned long long*)acc + ((uint32_t)slot * 8u + 4u * (uint32_t)fh);   // 32-bit index: no loop-invariant 64-bit VGPR pair
#pragma unroll
  for (int q = 0; q < 4; ++q) atomicAdd(dst + q, v[q]);
  if (fh == 0) atomicAdd(&counts[slot], len);
}

__device__ __forceinline__ void scatter_tile(const f32x16& o, int slot, int j, int h, int32_t* __restrict__ counts,
                                             long long* __restrict__ acc) {
  unsigned long long v[4];
  bool is_end;
  int len;
  tile_run_sums(o, slot, j, h, v, is_end, len);
#ifdef BNV_PROBE_NO_SCATTER   // development probe (tools/): what do the scatter atomics cost?  keeps 1 of 64 tiles' atomics
  if ((blockIdx.x & 63) != 0) return;
#endif
  if (slot >= 0 && is_end) run_to_global(acc, counts, slot, h, v, len);
}

// ---- host, library-internal: launches of the kernels other files define (a kernel is launched from its own translation
// unit).  `plist`: the owned-pair list, or null.  encode_mlp.hip: MLP mode 0, 1 or 3 on `grid` workgroups; its LDS opt-ins
#define BNV_HIDDEN __attribute__((visibility("hidden")))
BNV_HIDDEN void launch_encoder_mlp(int mlp, int grid, const float* pts, int n, const bnv_grid_t& g, const float* pack,
                                   const EncodeWs& ws, const int32_t* plist, hipStream_t stream);
BNV_HIDDEN int encode_init();
// encode_tcnn.hip: the block encoder (whole frames of `image_width`, 0: unknown; no plist) or the tile encoder
BNV_HIDDEN void launch_encoder_tcnn(bool blocks, int image_width, int grid, const float* pts, int n, const bnv_grid_t& g,
                                    const float* pack, const EncodeWs& ws, const int32_t* plist, hipStream_t stream);
// shard.hip: first-touch ownership behind k_rank -- k_shard_assign, then k_shard_own on the frame's input_pts rows
BNV_HIDDEN int launch_shard_own(const EncodeWs& ws, const bnv_grid_t& g, const float* pts, int n, int32_t* plist,
                                hipStream_t stream);
// encode.hip: bnv_encode_finish with the two staging knobs of the frame pipeline (pipeline.hip).  The persistent
// point-encoder kernel runs on at most max_workgroups workgroups (one per CU; 0 = every CU): it fills a CU's LDS, so
// the pipeline leaves a share of the CUs to the small kernels of its other streams this way.  parts & 1 = the
// point-encoder MLP + scatter, parts & 2 = finalize (mean, filter, ordered compaction, counters, clean workspace); the
// two may go to different streams (the caller orders them: part 2 behind part 1).  bnv_encode_finish is (0, 3).
BNV_HIDDEN int encode_finish_parts(const float* input_pts, int64_t n_points, int image_width,
                                   const bnv_grid_t* grid_host, const float* pointnet_pack, void* ws, size_t ws_bytes,
                                   int64_t ws_max_points, float* out_feats, int64_t* out_pcounts, int64_t* out_flat_ids,
                                   int64_t* out_grid_ids, int64_t out_capacity, int emit_all,
                                   bnv_encode_counters_t* counters, int max_workgroups, int parts, bnv_stream_t stream);
#undef BNV_HIDDEN
}  // namespace bnv
