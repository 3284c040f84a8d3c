// lattice.hip -- bookkeeping of the lattice decode, with no MLP in it: which rows are origins of a call, the 27
// neighbour rows of every origin, the (row, l) table entries that live lattice points read (the work list of the table
// kernels, decode.hip) and the blend of the tables into the SDF of the 3x3x3 meshing lattice.
#include "decode_host.hpp"
#include "scan.hpp"
#include "volume_keys.hpp"
#include "sdf_mlp.hpp"   // sample_delta only (k_lattice_blend<true>): the TSDF prior at a corner

namespace bnv {

void lattice_ws_frame_words(void* ws_ptr, int64_t row_capacity, int32_t** origin_stamp, int32_t** ctl) {
  LatticeWs ws;
  lattice_ws_layout(1, row_capacity, (char*)ws_ptr, &ws);   // both sit in the part that depends on row_capacity only
  *origin_stamp = ws.origin_stamp;
  *ctl = ws.n_list;
}

constexpr int kOriginBit = 1 << 30;   // flag in nbr_rows entries (rows are < 2^30)

// origin_stamp[row of origin b] = epoch: which rows are decoded origins of this call
__global__ __launch_bounds__(256) void k_lattice_stamp(bnv_volume_t v, const int64_t* __restrict__ origins, int64_t n,
                                                       int64_t row_limit, int32_t* __restrict__ origin_stamp,
                                                       int32_t epoch, const int32_t* __restrict__ n_dev,
                                                       int32_t* __restrict__ n_list) {
  if (n_dev) n = (int64_t)*n_dev < n ? (int64_t)*n_dev : n;
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  // the control words of the stages behind (entries listed, tile counter of the table kernel, spare) are cleared
  // here: saves bnv_decode_lattice a memset launch per call
  if (n_list && b == 0) n_list[1] = n_list[2] = n_list[3] = 0;
  if (b >= n) return;
  const int row = volume_row(v, origins[b * 3 + 0], origins[b * 3 + 1], origins[b * 3 + 2]);
  if (row >= 0 && row < row_limit) origin_stamp[row] = epoch;
}

// row (| kOriginBit) of neighbour nb (0..26) of origin b, or -1: absent, below min_pts (such rows can only ever appear
// under a false mask) or beyond row_limit
__device__ __forceinline__ int lattice_neighbor_row(const bnv_volume_t& v, const int64_t* __restrict__ origins, int64_t b,
                                                    int nb, const float* __restrict__ weights, int64_t row_limit,
                                                    float min_pts, const int32_t* __restrict__ origin_stamp,
                                                    int32_t epoch) {
  const int64_t x = origins[b * 3 + 0] + (nb / 9 - 1);
  const int64_t y = origins[b * 3 + 1] + ((nb / 3) % 3 - 1);
  const int64_t z = origins[b * 3 + 2] + (nb % 3 - 1);
  int row = volume_row(v, x, y, z);
  if (row >= row_limit) row = -1;
  if (row < 0 || !(weights[row] >= min_pts)) return -1;
  const bool is_origin = origin_stamp && origin_stamp[row] == epoch;
  return row | (is_origin ? (1 << 30) : 0);
}

__global__ __launch_bounds__(256) void k_lattice_neighbors(bnv_volume_t v, const int64_t* __restrict__ origins,
                                                           int64_t n, const float* __restrict__ weights,
                                                           int64_t row_limit, float min_pts,
                                                           int32_t* __restrict__ nbr_rows,
                                                           int32_t* __restrict__ stamp, int32_t epoch,
                                                           int32_t* __restrict__ list, int32_t* __restrict__ n_list,
                                                           const uint8_t* __restrict__ row_skip,
                                                           int32_t* __restrict__ origin_stamp,
                                                           const int32_t* __restrict__ n_dev,
                                                           int32_t* __restrict__ ctl_clear) {
  if (n_dev) n = (int64_t)*n_dev < n ? (int64_t)*n_dev : n;  // count from device memory; n = grid capacity
  // origins stamped by the frame's upsert (bnv_volume_integrate with extras): no k_lattice_stamp launch in front of this
  // one, so the control words of the stages behind are cleared here
  if (ctl_clear && blockIdx.x == 0 && threadIdx.x == 0) ctl_clear[1] = ctl_clear[2] = ctl_clear[3] = 0;
  // grid-stride: the launch is sized for the CAPACITY (the count is on the device) but capped, so a frame that holds
  // a fraction of it (a shard's 1 / world) does not pay for ten thousand workgroups that only exit
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n * 27; t += (int64_t)gridDim.x * 256) {
    const int64_t b = t / 27;
    const int nb = (int)(t - b * 27);
    // (from the dense row index when the volume keeps one: the 27 look-ups of a voxel are 9 runs of 3 neighbouring
    // words, and neighbouring voxels share them -- against 27 hash probes that each pull a line of their own)
    const int r = lattice_neighbor_row(v, origins, b, nb, weights, row_limit, min_pts, origin_stamp, epoch);
    nbr_rows[t] = r;
    // list = rows whose table must be (re)computed here; halo rows (row_skip) get theirs by exchange
    const int row = r & ~(1 << 30);
    if (r >= 0 && list && !(row_skip && row_skip[row]) && atomicExch(&stamp[row], epoch) != epoch)
      list[atomicAdd(n_list, 1)] = row;
  }
}

// One thread per lattice point P = b + d / 2 (origin b, offset d): if all 8 corner voxels are usable (the point is
// LIVE), the (row, l) table entries it reads -- one per DISTINCT corner voxel c, l = the offset of P inside c -- go
// to the MLP work list, each exactly once.  Entries of masked points are never evaluated.
// An entry (row, l) names one physical point, and whether that point is live depends on the point alone.  So
//  * the entry of P in the origin's OWN row is appended by this thread, unconditionally: no other thread appends it;
//  * the entries in other corner rows that are ORIGINS of this call are left to those origins (P is one of their
//    27 points too, and they see the same live decision);
//  * entries in corner rows that are not decoded in this call (the fringe of the frame) belong to the origin
//    floor(P) if that voxel is decoded here; only if it is not are they contended: the first thread to flag
//    (row, l) in need_mask appends it.
// Both decisions are bit tests on two 27-bit masks per origin (usable neighbours, neighbours that are origins),
// cut out of the ballots of the staging loop.  (Until r03 every corner entry of a shared point went through a
// returning global atomicOr, and an owner rule decided which origin handled a shared point: 35 us.)
// A workgroup walks kMarkChunks chunks of 1,024 lattice points and collects the new entries in LDS; they go to the
// global list with ONE atomicAdd on the list counter per flush -- normally one per workgroup.  (Same-address
// atomics serialise in the memory-side atomic unit at ~11 ns each, tools/probe_mark.hip: one per 1,024 points was
// 29 us of serial time per frame; a decoupled look-back in its place was slower still, 57-78 us, because every
// workgroup then ends with two or three dependent memory round trips.)
#ifndef BNV_MARK_THREADS
#define BNV_MARK_THREADS 1024
#endif
#ifndef BNV_MARK_CHUNKS
#define BNV_MARK_CHUNKS 2
#endif
#ifndef BNV_MARK_SCAN
#define BNV_MARK_SCAN 0
#endif
constexpr int kMarkThreads = BNV_MARK_THREADS;
constexpr int kMarkChunks = BNV_MARK_CHUNKS;
constexpr int kMarkOrigins = kMarkThreads / 27 + 2;   // origins a chunk's lattice points can belong to
constexpr int kMarkBuf = kMarkChunks > 1 ? 16 * kMarkThreads : 8 * kMarkThreads;   // LDS entry buffer; a chunk appends at most 8 per thread
// FUSED: the neighbour rows are looked up HERE (and written to nbr_rows for the blend) instead of by a
// k_lattice_neighbors launch in front: one launch and one 10 MB round trip less per frame.  Needs the origin stamps
// of the call to be complete (k_lattice_stamp or the frame's upsert) and the control words cleared.
struct MarkFused {
  bnv_volume_t v;
  const int64_t* origins;
  const float* weights;
  int64_t row_limit;
  float min_pts;
  int32_t* nbr_rows_out;
  // Persistent tables (bnv_volume_t.lattice_have; null: none): bit l of have[row] = the entry (row, l) is in the
  // persistent table for the row's current features.  Entries in rows this call does not decode are listed only when
  // their bit is clear (and the bit is set: the table kernel behind fills them); the entries of the call's own rows
  // -- always listed, the upsert has just changed the rows -- set their bits for later frames.
  uint32_t* have;
};

template <bool FUSED>
__global__ __launch_bounds__(kMarkThreads) void k_lattice_mark(const int32_t* __restrict__ nbr_rows, int64_t n,
                                                               const int32_t* __restrict__ origin_stamp, int32_t epoch,
                                                               uint32_t* __restrict__ need_mask,
                                                               int32_t* __restrict__ entries,
                                                               int32_t* __restrict__ n_entries,
                                                               int64_t entry_capacity,
                                                               const int32_t* __restrict__ n_dev, MarkFused F) {
  if (n_dev) n = (int64_t)*n_dev < n ? (int64_t)*n_dev : n;
  // chunks per (virtual) workgroup: kMarkChunks -- or ONE when the launch's workgroups then still cover the call (a
  // shard's 1 / world of a frame): twice the workgroups at work, half the dependent chunk passes per workgroup
  const int CH = (n * 27 <= (int64_t)gridDim.x * kMarkThreads) ? 1 : kMarkChunks;
  if ((int64_t)blockIdx.x * kMarkThreads * CH >= n * 27) return;
  // (grid-stride over virtual workgroups vb: the launch is sized for the capacity, capped at two workgroups per CU)
  __shared__ int s_buf[kMarkBuf];
  __shared__ int s_nbr[kMarkOrigins * 27];
  __shared__ int s_corner[216 + 27];
  __shared__ uint32_t s_need[27];                              // the neighbours a lattice point's corners are
  constexpr int kMarkWords = (kMarkOrigins * 27 + 63) / 64 + 1;
  __shared__ unsigned long long s_ub[kMarkWords], s_ob[kMarkWords];   // bit i: s_nbr[i] usable / an origin of this call
#if BNV_MARK_SCAN
  __shared__ uint32_t s_wave[kMarkThreads / 64];
#endif
  __shared__ int s_count, s_base;
  __shared__ uint32_t s_have[kMarkOrigins];   // persistent tables: live-point bits of the chunk's origins
  if (threadIdx.x < 216) {
    const int p = threadIdx.x >> 3, k = threadIdx.x & 7;
    const int d[3] = {p / 9 - 1, (p / 3) % 3 - 1, p % 3 - 1};
    int nbi = 0, li = 0, dup = 0;   // ceil == floor on an axis with d == 0: same entry as the floor corner
    for (int a = 0; a < 3; ++a) {
      int nb_a = 0, loc2 = 0;
      if (d[a] != 0) {
        if ((k >> a) & 1) {
          nb_a = (d[a] + 1) / 2;
          loc2 = -1;
        } else {
          nb_a = (d[a] - 1) / 2;
          loc2 = 1;
        }
      } else if ((k >> a) & 1) {
        dup = 1;
      }
      nbi = nbi * 3 + (nb_a + 1);
      li = li * 3 + (loc2 + 1);
    }
    s_corner[threadIdx.x] = nbi | (li << 5) | (dup << 10);
  } else if (threadIdx.x < 216 + 27) {
    // neighbour index of the voxel floor(P) if some offset of P is negative, else -1 (the origin itself)
    const int p = threadIdx.x - 216;
    const int d[3] = {p / 9 - 1, (p / 3) % 3 - 1, p % 3 - 1};
    s_corner[threadIdx.x] = (d[0] < 0 || d[1] < 0 || d[2] < 0)
                                ? ((d[0] < 0 ? 0 : 1) * 3 + (d[1] < 0 ? 0 : 1)) * 3 + (d[2] < 0 ? 0 : 1)
                                : -1;
  }
  if (threadIdx.x < kMarkWords) s_ub[threadIdx.x] = s_ob[threadIdx.x] = 0ull;
  __syncthreads();
  if (threadIdx.x < 27) {
    uint32_t m = 0;
    for (int k = 0; k < 8; ++k) m |= 1u << (s_corner[threadIdx.x * 8 + k] & 31);
    s_need[threadIdx.x] = m;
  }
  for (int64_t vb = blockIdx.x; vb * kMarkThreads * CH < n * 27; vb += gridDim.x) {
  if (threadIdx.x == 0) s_count = 0;
  __syncthreads();
  for (int ch = 0; ch < CH; ++ch) {
    const int64_t t0 = (vb * CH + ch) * kMarkThreads;
    const bool last = ch == CH - 1 || t0 + kMarkThreads >= n * 27;
    // the neighbour rows of the chunk's origins: one coalesced read, then LDS
    const int64_t b0 = t0 / 27;
    for (int i = threadIdx.x; i < kMarkOrigins * 27; i += kMarkThreads) {
      const int64_t g = b0 * 27 + i;
      int r = -1;
      if (g < n * 27) {
        if constexpr (FUSED) {
          const int ob = i / 27;
          r = lattice_neighbor_row(F.v, F.origins, b0 + ob, i - ob * 27, F.weights, F.row_limit, F.min_pts, origin_stamp,
                                   epoch);
          F.nbr_rows_out[g] = r;   // (a chunk boundary inside an origin: both chunks write the same values)
        } else {
          r = nbr_rows[g];
        }
      }
      s_nbr[i] = r;
      if (i < kMarkOrigins) s_have[i] = 0u;
      const unsigned long long bu = __ballot(r >= 0), bo = __ballot(r >= 0 && (r & kOriginBit));
      if ((threadIdx.x & 63) == 0) {
        s_ub[i >> 6] = bu;
        s_ob[i >> 6] = bo;
      }
    }
    __syncthreads();
    const int64_t t = t0 + threadIdx.x;
    int ent[8];
    uint32_t keep = 0;    // bit k: ent[k] is appended by this thread
    if (t < n * 27) {
      const int64_t b = t / 27;
      const int p = (int)(t - b * 27);
      const int ob = (int)(b - b0);
      const int* nb27 = s_nbr + ob * 27;
      const int q = ob * 27, w = q >> 6, sh = q & 63;
      unsigned long long xu = s_ub[w] >> sh, xo = s_ob[w] >> sh;
      if (sh > 64 - 27) {
        xu |= s_ub[w + 1] << (64 - sh);
        xo |= s_ob[w + 1] << (64 - sh);
      }
      const uint32_t um = (uint32_t)xu & 0x7FFFFFFu, om = (uint32_t)xo & 0x7FFFFFFu, need = s_need[p];
      if ((um & need) == need) {     // live
        uint32_t rest = need & ~om;  // corner voxels nobody decodes in this call
        if (!((rest >> 13) & 1u)) {  // the origin's own row (always, but for a caller's stale stamp array)
          ent[0] = ((nb27[13] & ~kOriginBit) << 5) | p;     // P inside its origin: l = d
          keep = 1u;
          if (F.have) atomicOr(&s_have[ob], 1u << p);
        }
        // Entries in rows that are not decoded here belong to the origin floor(P) when that voxel is decoded in
        // this call (it is unique: no flag needed); else every origin that holds P asks need_mask
        const int dneg = s_corner[216 + p];
        const bool mine = dneg < 0;
        if (rest && (mine || !((om >> dneg) & 1u))) {
          // (rare) all atomics are issued before any result is looked at: one memory round trip, not up to eight
          int rowk[8], lk[8];
          uint32_t seen[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const int c = s_corner[p * 8 + k];     // nbi | li << 5 | dup << 10
            rowk[k] = (!(c >> 10) && ((rest >> (c & 31)) & 1u)) ? (nb27[c & 31] & ~kOriginBit) : -1;
            lk[k] = (c >> 5) & 31;
          }
          if (F.have) {   // persistent tables: the bit outlives the call (whoever finds it clear lists the entry)
#pragma unroll
            for (int k = 0; k < 8; ++k) seen[k] = rowk[k] >= 0 ? atomicOr(&F.have[rowk[k]], 1u << lk[k]) : 0u;
          } else {
#pragma unroll
            for (int k = 0; k < 8; ++k)
              seen[k] = (!mine && rowk[k] >= 0) ? atomicOr(&need_mask[rowk[k]], 1u << lk[k]) : 0u;
          }
          int at = (int)keep;
#pragma unroll
          for (int k = 0; k < 8; ++k)
            if (rowk[k] >= 0 && !((seen[k] >> lk[k]) & 1u)) {
              // (at most 8 distinct corners, the own row among them: at < 8)
              ent[at & 7] = (rowk[k] << 5) | lk[k];
              keep |= 1u << (at & 7);
              ++at;
            }
        }
      }
    }
#if BNV_MARK_SCAN
    // the threads' places in the LDS buffer: one block-wide scan of the counts (no LDS atomics)
    uint32_t tot;
    const uint32_t off = block_exclusive_scan<kMarkThreads>((uint32_t)__popc(keep), s_wave, &tot);
    const int at = s_count + (int)off;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if ((keep >> k) & 1u) s_buf[at + __popc(keep & ((1u << k) - 1u))] = ent[k];
    __syncthreads();
    if (threadIdx.x == 0) s_count += (int)tot;
    __syncthreads();
#else
    {
      // ent[0] (nearly every live point has exactly this one): one LDS atomic per wave, places by ballot
      const unsigned long long bal = __ballot(keep & 1u);
      int base0 = 0;
      if ((threadIdx.x & 63) == 0 && bal) base0 = atomicAdd(&s_count, __popcll(bal));
      base0 = __builtin_amdgcn_readfirstlane(base0);
      if (keep & 1u) s_buf[base0 + __popcll(bal & ((1ull << (threadIdx.x & 63)) - 1ull))] = ent[0];
      const uint32_t extra = keep >> 1;      // (rare) entries in rows that are not decoded in this call
      if (extra) {
        const int at = atomicAdd(&s_count, __popc(extra));
#pragma unroll
        for (int k = 1; k < 8; ++k)
          if ((extra >> (k - 1)) & 1u) s_buf[at + __popc(extra & ((1u << (k - 1)) - 1u))] = ent[k];
      }
    }
    __syncthreads();
#endif
    if (F.have) {   // (kernel-uniform) the own-row bits of the chunk's origins join the persistent masks
      if (threadIdx.x < kMarkOrigins && s_have[threadIdx.x]) {
        const int r13 = s_nbr[threadIdx.x * 27 + 13];
        if (r13 >= 0) atomicOr(&F.have[r13 & ~kOriginBit], s_have[threadIdx.x]);
      }
      __syncthreads();   // s_nbr / s_have are rewritten by the next chunk
    }
    const int cnt = s_count;
    if (cnt > 0 && (last || cnt > kMarkBuf - 8 * kMarkThreads)) {   // flush (block-uniform)
      if (threadIdx.x == 0) s_base = atomicAdd(n_entries, cnt);
      __syncthreads();
      // (only now has every wave read s_count above: resetting it next to the atomicAdd let a late wave see 0, skip
      // the flush and fall out of step with the workgroup's barriers)
      if (threadIdx.x == 0) s_count = 0;
      const int base = s_base;
      for (int i = threadIdx.x; i < cnt; i += kMarkThreads)
        if (base + i < entry_capacity) entries[base + i] = s_buf[i];
      __syncthreads();
    }
    if (last) break;
  }
  __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------
// k_lattice_mark_o (round 5): the same marking with ONE THREAD PER ORIGIN instead of one per lattice point.
// What k_lattice_mark spends its time on is not arithmetic (a few bit tests per point) but the per-chunk chain of
// barriers, LDS appends and flushes over 2.7 M threads, and -- fused with the neighbour look-up, on a shard -- ONE
// dependent three-load chain per thread.  Here a thread holds its origin's two 27-bit masks (usable neighbours,
// neighbours that are origins of the call) in registers and derives the live mask of its 27 lattice points with 27 bit
// tests; the own-row entries of a workgroup's 256 origins are placed by one block scan and leave through LDS as one
// coalesced copy (<= 27 per origin: the staging area of the neighbour rows is exactly large enough), the fringe
// entries (rows that are not decoded in this call: a few per cent) through a small LDS buffer; one global atomic per
// workgroup; fused, every thread has 27 independent look-up chains in flight.  Same entries as k_lattice_mark (in
// another order, which nothing depends on), same need_mask / lattice_have bookkeeping.
// ---------------------------------------------------------------------------------------------------
constexpr int kMoThreads = 256;                 // origins per workgroup
constexpr int kMoExtra = 3072;                  // LDS room for fringe entries of a workgroup (beyond it: direct appends)
constexpr int kMoWork = 2048;                   // LDS list of a workgroup's lattice points that have fringe corners
template <bool FUSED>
__global__ __launch_bounds__(kMoThreads) void k_lattice_mark_o(const int32_t* __restrict__ nbr_rows, int64_t n,
                                                               const int32_t* __restrict__ origin_stamp, int32_t epoch,
                                                               uint32_t* __restrict__ need_mask,
                                                               int32_t* __restrict__ entries,
                                                               int32_t* __restrict__ n_entries,
                                                               int64_t entry_capacity,
                                                               const int32_t* __restrict__ n_dev, MarkFused F) {
  if (n_dev) n = (int64_t)*n_dev < n ? (int64_t)*n_dev : n;
  if ((int64_t)blockIdx.x * kMoThreads >= n) return;
  __shared__ int s_nbr[kMoThreads * 27];        // neighbour rows of the workgroup's origins; then its own-row entries
  __shared__ int s_extra[kMoExtra];
  __shared__ int s_corner[216 + 27];
  __shared__ uint32_t s_need[27];
  __shared__ uint32_t s_wave[kMoThreads / 64];
  __shared__ uint32_t s_om[kMoThreads];
  __shared__ int s_work[kMoWork];
  __shared__ int s_nx, s_nw, s_base;
  if (threadIdx.x < 216) {
    const int p = threadIdx.x >> 3, k = threadIdx.x & 7;
    const int d[3] = {p / 9 - 1, (p / 3) % 3 - 1, p % 3 - 1};
    int nbi = 0, li = 0, dup = 0;   // ceil == floor on an axis with d == 0: same entry as the floor corner
    for (int a = 0; a < 3; ++a) {
      int nb_a = 0, loc2 = 0;
      if (d[a] != 0) {
        if ((k >> a) & 1) {
          nb_a = (d[a] + 1) / 2;
          loc2 = -1;
        } else {
          nb_a = (d[a] - 1) / 2;
          loc2 = 1;
        }
      } else if ((k >> a) & 1) {
        dup = 1;
      }
      nbi = nbi * 3 + (nb_a + 1);
      li = li * 3 + (loc2 + 1);
    }
    s_corner[threadIdx.x] = nbi | (li << 5) | (dup << 10);
  } else if (threadIdx.x < 216 + 27) {
    const int p = threadIdx.x - 216;
    const int d[3] = {p / 9 - 1, (p / 3) % 3 - 1, p % 3 - 1};
    s_corner[threadIdx.x] = (d[0] < 0 || d[1] < 0 || d[2] < 0)
                                ? ((d[0] < 0 ? 0 : 1) * 3 + (d[1] < 0 ? 0 : 1)) * 3 + (d[2] < 0 ? 0 : 1)
                                : -1;
  }
  __syncthreads();
  if (threadIdx.x < 27) {
    uint32_t m = 0;
    for (int k = 0; k < 8; ++k) m |= 1u << (s_corner[threadIdx.x * 8 + k] & 31);
    s_need[threadIdx.x] = m;
  }
  // the fringe entries of ONE live lattice point p of the origin whose neighbour rows are nb27 and origin mask om: the
  // corner rows that are not decoded in this call, each listed by whoever finds its bit clear.  All atomics of the
  // point are issued before any result is looked at (one memory round trip)
  auto fringe_point = [&](const int* nb27, uint32_t om, int p) {
    const uint32_t rest = s_need[p] & ~om;
    const bool mine = s_corner[216 + p] < 0;
    int rowk[8], lk[8];
    uint32_t seen[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int c = s_corner[p * 8 + k];     // nbi | li << 5 | dup << 10
      rowk[k] = (!(c >> 10) && ((rest >> (c & 31)) & 1u)) ? (nb27[c & 31] & ~kOriginBit) : -1;
      lk[k] = (c >> 5) & 31;
    }
    if (F.have) {   // persistent tables: the bit outlives the call
#pragma unroll
      for (int k = 0; k < 8; ++k) seen[k] = rowk[k] >= 0 ? atomicOr(&F.have[rowk[k]], 1u << lk[k]) : 0u;
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k)
        seen[k] = (!mine && rowk[k] >= 0) ? atomicOr(&need_mask[rowk[k]], 1u << lk[k]) : 0u;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (rowk[k] < 0 || ((seen[k] >> lk[k]) & 1u)) continue;
      const int e = (rowk[k] << 5) | lk[k];
      const int at = atomicAdd(&s_nx, 1);
      if (at < kMoExtra) {
        s_extra[at] = e;
      } else {   // (rare overflow of the LDS buffer: straight to the list)
        const int g = atomicAdd(n_entries, 1);
        if (g < entry_capacity) entries[g] = e;
      }
    }
  };
  for (int64_t vb = blockIdx.x; vb * kMoThreads < n; vb += gridDim.x) {
    const int64_t b0 = vb * kMoThreads;
    if (threadIdx.x == 0) s_nx = s_nw = 0;
    // the neighbour rows of the workgroup's origins
    bool staged = false;
    if constexpr (FUSED) {
      // With the dense row index a thread looks its OWN origin's 27 neighbours up in three rounds of independent loads
      // (27 index words; then 27 weights + 27 origin stamps) instead of 27 three-load chains one behind the other
      // (the generic look-up below branches between the loads, which keeps the compiler from overlapping them).
      if (F.v.brick) {
        staged = true;
        const int64_t bb = b0 + threadIdx.x;
        int rows[27];
        if (bb < n) {
          const int64_t ox = F.origins[bb * 3 + 0], oy = F.origins[bb * 3 + 1], oz = F.origins[bb * 3 + 2];
#pragma unroll
          for (int k = 0; k < 27; ++k) {
            const int64_t x = ox + (k / 9 - 1), y = oy + ((k / 3) % 3 - 1), z = oz + (k % 3 - 1);
            int64_t idx;
            rows[k] = brick_index(F.v, x, y, z, &idx) ? F.v.brick[idx] : -2;   // -2: outside the index (the hash decides)
          }
#pragma unroll
          for (int k = 0; k < 27; ++k) {
            if (rows[k] == -2)
              rows[k] = volume_row(F.v, ox + (k / 9 - 1), oy + ((k / 3) % 3 - 1), oz + (k % 3 - 1));
            if (rows[k] >= F.row_limit) rows[k] = -1;
          }
          float wk[27];
          int sk[27];
#pragma unroll
          for (int k = 0; k < 27; ++k) {
            const int rr = rows[k] < 0 ? 0 : rows[k];
            wk[k] = F.weights[rr];
            sk[k] = origin_stamp ? origin_stamp[rr] : 0;
          }
#pragma unroll
          for (int k = 0; k < 27; ++k) {
            int r = -1;
            if (rows[k] >= 0 && wk[k] >= F.min_pts) r = rows[k] | ((origin_stamp && sk[k] == epoch) ? kOriginBit : 0);
            s_nbr[threadIdx.x * 27 + k] = r;
          }
        } else {
#pragma unroll
          for (int k = 0; k < 27; ++k) s_nbr[threadIdx.x * 27 + k] = -1;
        }
      }
    }
#pragma unroll 9
    for (int i = threadIdx.x; i < (staged ? 0 : kMoThreads * 27); i += kMoThreads) {
      const int64_t g = b0 * 27 + i;
      int r = -1;
      if (g < n * 27) {
        if constexpr (FUSED) {
          // (no global store in this loop: a store the compiler cannot prove disjoint from the volume's arrays would
          // order the iterations' look-up chains one behind the other -- 81 dependent loads instead of 3)
          const int ob = i / 27;
          r = lattice_neighbor_row(F.v, F.origins, b0 + ob, i - ob * 27, F.weights, F.row_limit, F.min_pts, origin_stamp,
                                   epoch);
        } else {
          r = nbr_rows[g];
        }
      }
      s_nbr[i] = r;
    }
    __syncthreads();
    if constexpr (FUSED) {   // the blend reads the neighbour rows from global memory
      for (int i = threadIdx.x; i < kMoThreads * 27; i += kMoThreads)
        if (b0 * 27 + i < n * 27) F.nbr_rows_out[b0 * 27 + i] = s_nbr[i];
    }
    const int64_t b = b0 + threadIdx.x;
    const int* nb27 = s_nbr + threadIdx.x * 27;      // (stride 27 words: conflict-free across the lanes of a wave)
    uint32_t um = 0, om = 0;
    if (b < n) {
#pragma unroll
      for (int k = 0; k < 27; ++k) {
        const int r = nb27[k];
        um |= (r >= 0 ? 1u : 0u) << k;
        om |= ((r >= 0 && (r & kOriginBit)) ? 1u : 0u) << k;
      }
    }
    const int own_row = (um >> 13) & 1u ? (nb27[13] & ~kOriginBit) : -1;
    uint32_t live = 0;
#pragma unroll
    for (int p = 0; p < 27; ++p) live |= ((um & s_need[p]) == s_need[p] ? 1u : 0u) << p;
    if (b >= n) live = 0;
    // the points whose entry in the origin's OWN row this thread lists (always, but for a caller's stale stamp array)
    const uint32_t own = ((om >> 13) & 1u) ? live : 0u;
    if (own && F.have) atomicOr(&F.have[own_row], own);   // (the upsert cleared the word; nobody else sets bits of an origin's row)
    // fringe entries: corner rows that are not decoded in this call.  A thread only LISTS its points that have such
    // corners (origin << 5 | p); the whole workgroup then works the list off, one point per thread and step, the (up
    // to eight) returning atomics of a point in flight together -- an origin on the fringe has dozens of them, and
    // one thread taking them one round trip after the other held its workgroup for tens of microseconds
    s_om[threadIdx.x] = om;
    if (live) {
      for (int p = 0; p < 27; ++p) {
        if (!((live >> p) & 1u) || !(s_need[p] & ~om)) continue;
        const int dneg = s_corner[216 + p];
        if (dneg >= 0 && ((om >> dneg) & 1u)) continue;      // the origin floor(P) is decoded here: it lists them
        const int at = atomicAdd(&s_nw, 1);
        if (at < kMoWork) s_work[at] = (int)(threadIdx.x << 5) | p;
        else fringe_point(nb27, om, p);                       // (a call whose fringe dwarfs its origins: inline)
      }
    }
    __syncthreads();
    {
      const int nw = s_nw < kMoWork ? s_nw : kMoWork;
      for (int i = threadIdx.x; i < nw; i += kMoThreads) {
        const int wi = s_work[i];
        fringe_point(s_nbr + (wi >> 5) * 27, s_om[wi >> 5], wi & 31);
      }
    }
    uint32_t tot;
    const uint32_t off = block_exclusive_scan<kMoThreads>((uint32_t)__popc(own), s_wave, &tot);   // (two barriers: s_nbr is read out)
    {
      int at = (int)off;
      uint32_t m = own;
      while (m) {
        const int p = __ffs(m) - 1;
        m &= m - 1;
        s_nbr[at++] = (own_row << 5) | p;
      }
    }
    __syncthreads();
    const int nx = s_nx < kMoExtra ? s_nx : kMoExtra;
    if (threadIdx.x == 0) s_base = (tot + nx) ? atomicAdd(n_entries, (int)tot + nx) : 0;
    __syncthreads();
    const int base = s_base;
    for (int i = threadIdx.x; i < (int)tot; i += kMoThreads)
      if (base + i < entry_capacity) entries[base + i] = s_nbr[i];
    for (int i = threadIdx.x; i < nx; i += kMoThreads)
      if (base + (int)tot + i < entry_capacity) entries[base + (int)tot + i] = s_extra[i];
    __syncthreads();   // s_nbr / s_extra / s_nx are rewritten by the next round
  }
}

// DELTA = false: the streaming case (no TSDF prior): 8 table reads and a weighted sum, few registers -- it runs
// beside the persistent MLP kernels of the other streams.
#ifndef BNV_BLEND_PPT
#define BNV_BLEND_PPT 3
#endif
constexpr int kBlendPpt = BNV_BLEND_PPT;     // lattice points per thread of the streaming blend: their gathers are in flight together
template <bool DELTA>
__global__ __launch_bounds__(256) void k_lattice_blend(const int32_t* __restrict__ nbr_rows, int64_t n,
                                                       const float* __restrict__ table, bnv_grid_t g,
                                                       const int64_t* __restrict__ origins, bnv_sdf_delta_t delta,
                                                       float* __restrict__ out, const int32_t* __restrict__ n_dev) {
  if (n_dev) n = (int64_t)*n_dev < n ? (int64_t)*n_dev : n;
  constexpr int PPT = DELTA ? 1 : kBlendPpt;
  constexpr int TILE = 256 * PPT;
  // the neighbour rows of the block's origins: one coalesced read, then 8 LDS reads per lattice point
  __shared__ int s_nbr[(TILE / 27 + 2) * 27];
  // grid-stride over virtual workgroups vb (the launch is sized for the capacity, capped at 8 workgroups per CU: a
  // frame that holds a fraction of it does not pay for tens of thousands of workgroups that only exit)
  for (int64_t vb = blockIdx.x; vb * TILE < n * 27; vb += gridDim.x) {
  if (vb != (int64_t)blockIdx.x) __syncthreads();   // s_nbr of the previous round is no longer read
  const int64_t b0 = (vb * TILE) / 27;
  for (int i = threadIdx.x; i < (TILE / 27 + 2) * 27; i += 256) {
    const int64_t gidx = b0 * 27 + i;
    s_nbr[i] = gidx < n * 27 ? nbr_rows[gidx] : -1;
  }
  __syncthreads();
#pragma unroll
  for (int rep = 0; rep < PPT; ++rep) {
  const int64_t t = vb * TILE + rep * 256 + threadIdx.x;
  [&]() {
  if (t >= n * 27) return;
  const int64_t b = t / 27;
  const int p = (int)(t - b * 27);
  const int* nb27 = s_nbr + (int)(b - b0) * 27;
  const int d[3] = {p / 9 - 1, (p / 3) % 3 - 1, p % 3 - 1};  // lattice point = origin + 0.5 * d
  if constexpr (!DELTA) {
    // Every corner has the same weight 0.5^m (m = axes with a half-voxel offset) and the reference's normaliser, the
    // sequential sum of the 8 weights, is exactly 8 * 0.5^m: one pass, nothing kept in arrays; fully unrolled so
    // that the 8 gathers are in flight together (a partially unrolled 20-VGPR version took 43 us instead of 33).
    const int m = (d[0] != 0) + (d[1] != 0) + (d[2] != 0);
    const float wc = m == 0 ? 1.f : (m == 1 ? 0.5f : (m == 2 ? 0.25f : 0.125f));
    const float w = __fdiv_rn(wc, 8.f * wc);
    bool ok = true;
    int rowk[8], lk[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int cb = kCornerCeilBits[k];
      int nbi = 0, li = 0;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        int nb_a = 0, loc2 = 0;
        if (d[a] != 0) {
          if ((cb >> a) & 1) {
            nb_a = (d[a] + 1) / 2;
            loc2 = -1;
          } else {
            nb_a = (d[a] - 1) / 2;
            loc2 = 1;
          }
        }
        nbi = nbi * 3 + (nb_a + 1);
        li = li * 3 + (loc2 + 1);
      }
      rowk[k] = nb27[nbi];
      lk[k] = li;
      if (rowk[k] < 0) ok = false;
      rowk[k] &= ~kOriginBit;
    }
    if (!ok) {   // masked point (about half of them on a thin sheet): the constant, no table reads
      out[t] = g.voxel_size;
      return;
    }
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc = __fadd_rn(acc, __fmul_rn(table[(size_t)rowk[k] * 27 + lk[k]], w));
    out[t] = acc;
    return;
  }
  float wk[8];
  int rowk[8], lk[8];
  float ck[8][3];
  float norm = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int cb = kCornerCeilBits[k];
    int nbi = 0, li = 0;
    float w = 1.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      int nb_a = 0, loc2 = 0;  // neighbour offset of the corner voxel, 2 * local coordinate
      if (d[a] != 0) {
        if ((cb >> a) & 1) {
          nb_a = (d[a] + 1) / 2;
          loc2 = -1;
        } else {
          nb_a = (d[a] - 1) / 2;
          loc2 = 1;
        }
        w = __fmul_rn(w, 0.5f);
      }
      nbi = nbi * 3 + (nb_a + 1);
      li = li * 3 + (loc2 + 1);
      if (DELTA) ck[k][a] = (float)(origins[b * 3 + a] + nb_a);
    }
    wk[k] = w;
    lk[k] = li;
    rowk[k] = nb27[nbi] < 0 ? -1 : (nb27[nbi] & ~kOriginBit);
    norm = __fadd_rn(norm, w);
  }
  bool ok = true;
  float acc = 0.f, dacc = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float w = __fdiv_rn(wk[k], norm);
    if (rowk[k] < 0) ok = false;
    const float a = rowk[k] >= 0 ? table[(size_t)rowk[k] * 27 + lk[k]] : 0.f;
    acc = __fadd_rn(acc, __fmul_rn(a, w));
    if (DELTA) dacc = __fadd_rn(dacc, __fmul_rn(sample_delta(delta, g, ck[k]), w));
  }
  float o = ok ? acc : g.voxel_size;
  if (DELTA) o = __fadd_rn(o, dacc);
  out[t] = o;
  }();
  }
  }
}

// byte offset of one piece of the workspace of a call on n_voxels origins
template <class T>
static size_t ws_offset(int64_t n_voxels, int64_t row_capacity, T* LatticeWs::*piece) {
  LatticeWs ws;
  lattice_ws_layout(n_voxels, row_capacity, (char*)256, &ws);
  return (size_t)((char*)(ws.*piece) - (char*)256);
}

// k_lattice_stamp over the call's origins; clear_ctl: it also clears the control words of the stages behind
static int launch_stamp(const bnv_volume_t* vol, const int64_t* origins, int64_t n, int64_t row_limit,
                        const LatticeWs& ws, int32_t epoch, const int32_t* n_dev, bool clear_ctl, hipStream_t stream) {
  hipLaunchKernelGGL(k_lattice_stamp, dim3(blocks_for(n, 256)), dim3(256), 0, stream, *vol, origins, n,
                     row_limit, ws.origin_stamp, epoch, n_dev, clear_ctl ? ws.n_list : (int32_t*)nullptr);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

// the marking kernel of a call: one thread per origin or per lattice point; FUSED: it looks the neighbour rows up itself
template <bool FUSED>
static int launch_mark(const LatticeWs& ws, int64_t n, int32_t epoch, const int32_t* n_dev, const MarkFused& F,
                       bool per_origin, hipStream_t stream) {
  const int32_t* nbr_rows = FUSED ? nullptr : ws.nbr_rows;
  const dim3 mgrid(capped_grid((n * 27 + kMarkThreads * kMarkChunks - 1) / (kMarkThreads * kMarkChunks), 2));
  const dim3 ogrid(capped_grid((n + kMoThreads - 1) / kMoThreads, 4));
  if (per_origin)
    hipLaunchKernelGGL((k_lattice_mark_o<FUSED>), ogrid, dim3(kMoThreads), 0, stream, nbr_rows, n, ws.origin_stamp,
                       epoch, ws.need_mask, ws.entries, ws.n_list + 1, ws.entry_capacity, n_dev, F);
  else
    hipLaunchKernelGGL((k_lattice_mark<FUSED>), mgrid, dim3(kMarkThreads), 0, stream, nbr_rows, n, ws.origin_stamp,
                       epoch, ws.need_mask, ws.entries, ws.n_list + 1, ws.entry_capacity, n_dev, F);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

}  // namespace bnv

using namespace bnv;

extern "C" {

size_t bnv_decode_lattice_workspace_bytes(int64_t n_voxels, int64_t row_capacity) {
  return lattice_ws_layout(n_voxels, row_capacity, nullptr, nullptr);
}

size_t bnv_decode_lattice_count_offset(int64_t row_capacity) { return ws_offset(1, row_capacity, &LatticeWs::n_list); }

size_t bnv_decode_lattice_table_offset(int64_t row_capacity) { return ws_offset(1, row_capacity, &LatticeWs::table); }

size_t bnv_decode_lattice_list_offset(int64_t n_voxels, int64_t row_capacity) {
  return ws_offset(n_voxels, row_capacity, &LatticeWs::list);
}

static int lattice_neighbors_impl(const bnv_volume_t* vol, const bnv_grid_t* grid, const float* weights,
                                  int64_t row_limit, const int64_t* origins, int64_t n, const int32_t* n_dev,
                                  const uint8_t* row_skip, int build_list, void* ws_ptr, size_t ws_bytes, int32_t epoch,
                                  bool prestamped, bnv_stream_t stream_) {
  if (!vol_ok_ro(vol) || !grid || !weights || n < 0 || epoch == 0) return BNV_ERR_INVALID_ARGUMENT;
  if (!ws_ptr) return BNV_ERR_INVALID_ARGUMENT;
  LatticeWs ws;
  if (lattice_ws_layout(n, vol->row_capacity, (char*)ws_ptr, &ws) > ws_bytes) return BNV_ERR_WORKSPACE_TOO_SMALL;
  hipStream_t stream = (hipStream_t)stream_;
  if (build_list) BNV_HIP_CHECK(hipMemsetAsync(ws.n_list, 0, 16, stream));  // rows listed, (entries), tile counter, spare
  if (n == 0) return BNV_OK;
  if (!origins) return BNV_ERR_INVALID_ARGUMENT;
  if (!prestamped) BNV_TRY(launch_stamp(vol, origins, n, row_limit, ws, epoch, n_dev, !build_list, stream));
  hipLaunchKernelGGL(k_lattice_neighbors, dim3(capped_grid((n * 27 + 255) / 256, 16)), dim3(256), 0, stream, *vol, origins,
                     n, weights, row_limit, (float)grid->min_pts_in_grid, ws.nbr_rows, ws.stamp, epoch,
                     build_list ? ws.list : (int32_t*)nullptr, ws.n_list, row_skip, ws.origin_stamp, n_dev,
                     (prestamped && !build_list) ? ws.n_list : (int32_t*)nullptr);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

int bnv_lattice_neighbors(const bnv_volume_t* vol, const bnv_grid_t* grid, const float* weights, int64_t row_limit,
                          const int64_t* origins, int64_t n, const int32_t* n_dev, const uint8_t* row_skip,
                          int build_list, void* ws_ptr, size_t ws_bytes, int32_t epoch, bnv_stream_t stream) {
  return lattice_neighbors_impl(vol, grid, weights, row_limit, origins, n, n_dev, row_skip, build_list, ws_ptr,
                                ws_bytes, epoch, false, stream);
}

static int lattice_mark_impl(const bnv_volume_t* vol, int64_t n, const int32_t* n_dev, void* ws_ptr, size_t ws_bytes,
                             int32_t epoch, bool clear, bnv_stream_t stream_) {
  if (!vol_ok_ro(vol) || n < 0 || !ws_ptr || epoch == 0) return BNV_ERR_INVALID_ARGUMENT;
  LatticeWs ws;
  if (lattice_ws_layout(n, vol->row_capacity, (char*)ws_ptr, &ws) > ws_bytes) return BNV_ERR_WORKSPACE_TOO_SMALL;
  hipStream_t stream = (hipStream_t)stream_;
  // entries listed, tile counter of the table kernel, spare (bnv_decode_lattice: cleared by k_lattice_neighbors)
  if (clear) BNV_HIP_CHECK(hipMemsetAsync(ws.n_list + 1, 0, 12, stream));
  if (n == 0) return BNV_OK;
  MarkFused F = {};
  F.have = lattice_persist(vol) ? vol->lattice_have : nullptr;
  const bool per_origin = g_mark_per_origin.load(std::memory_order_relaxed) != 0;
  return launch_mark<false>(ws, n, epoch, n_dev, F, per_origin, stream);
}

// stamp (unless the frame's upsert did it) -> neighbours + mark in ONE launch
static int lattice_neighbors_mark_fused(const bnv_volume_t* vol, const bnv_grid_t* grid, const float* weights,
                                        int64_t row_limit, const int64_t* origins, int64_t n, const int32_t* n_dev,
                                        void* ws_ptr, size_t ws_bytes, int32_t epoch, bool prestamped,
                                        bnv_stream_t stream_) {
  if (!vol_ok_ro(vol) || !grid || !weights || n < 0 || epoch == 0 || !ws_ptr) return BNV_ERR_INVALID_ARGUMENT;
  LatticeWs ws;
  if (lattice_ws_layout(n, vol->row_capacity, (char*)ws_ptr, &ws) > ws_bytes) return BNV_ERR_WORKSPACE_TOO_SMALL;
  hipStream_t stream = (hipStream_t)stream_;
  if (n == 0) return BNV_OK;
  if (!origins) return BNV_ERR_INVALID_ARGUMENT;
  // (also clears the control words of the stages behind; prestamped: the frame's upsert has cleared them too)
  if (!prestamped) BNV_TRY(launch_stamp(vol, origins, n, row_limit, ws, epoch, n_dev, true, stream));
  MarkFused F = {};
  F.v = *vol;
  F.origins = origins;
  F.weights = weights;
  F.row_limit = row_limit;
  F.min_pts = (float)grid->min_pts_in_grid;
  F.nbr_rows_out = ws.nbr_rows;
  F.have = lattice_persist(vol) ? vol->lattice_have : nullptr;
  // (a shard's call keeps the per-point kernel: measured equal to slightly better there, profiles/r05_experiments.txt [e7])
  const bool per_origin = g_mark_per_origin.load(std::memory_order_relaxed) != 0 && grid->shard_world <= 1;
  return launch_mark<true>(ws, n, epoch, n_dev, F, per_origin, stream);
}

int bnv_lattice_mark(const bnv_volume_t* vol, int64_t n, const int32_t* n_dev, void* ws_ptr, size_t ws_bytes,
                     int32_t epoch, bnv_stream_t stream) {
  return lattice_mark_impl(vol, n, n_dev, ws_ptr, ws_bytes, epoch, true, stream);
}

int bnv_lattice_blend(const bnv_volume_t* vol, const bnv_grid_t* grid, const int64_t* origins, int64_t n,
                      const int32_t* n_dev, const bnv_sdf_delta_t* delta, void* ws_ptr, size_t ws_bytes,
                      float* out_sdf, bnv_stream_t stream) {
  if (!vol_ok_ro(vol) || !grid || n < 0 || !ws_ptr) return BNV_ERR_INVALID_ARGUMENT;
  if (n == 0) return BNV_OK;
  if (!origins || !out_sdf) return BNV_ERR_INVALID_ARGUMENT;
  LatticeWs ws;
  if (lattice_ws_layout(n, vol->row_capacity, (char*)ws_ptr, &ws) > ws_bytes) return BNV_ERR_WORKSPACE_TOO_SMALL;
  bnv_sdf_delta_t d = {};
  if (delta) d = *delta;
  const float* table = lattice_persist(vol) ? vol->lattice_table : ws.table;
  if (d.data)
    hipLaunchKernelGGL(k_lattice_blend<true>, dim3(capped_grid((n * 27 + 255) / 256, 8)), dim3(256), 0,
                       (hipStream_t)stream, ws.nbr_rows, n, table, *grid, origins, d, out_sdf, n_dev);
  else
    hipLaunchKernelGGL(k_lattice_blend<false>, dim3(capped_grid((n * 27 + 256 * kBlendPpt - 1) / (256 * kBlendPpt), 8)), dim3(256), 0,
                       (hipStream_t)stream, ws.nbr_rows, n, table, *grid, origins, d, out_sdf, n_dev);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

}  // extern "C"

// stages: 1 = neighbour rows + live entries, 2 = table MLP, 4 = blend
int bnv::decode_lattice_stages(const bnv_volume_t* vol, const bnv_grid_t* grid, const float* features,
                               const float* weights, int64_t row_limit, const float* sdfmlp_pack,
                               const int64_t* origins, int64_t n, const int32_t* n_dev, const bnv_sdf_delta_t* delta,
                               void* ws_ptr, size_t ws_bytes, int32_t epoch, bool prestamped, float* out_sdf,
                               int stages, bnv_stream_t stream) {
  if (g_num_cus <= 0) return BNV_ERR_NOT_INITIALISED;
  if (!features || !grid || n < 0 || ((stages & 2) && !sdfmlp_pack)) return BNV_ERR_INVALID_ARGUMENT;
  // persistent tables belong to the volume's own rows: have-bits set by a call that decodes other features would poison them
  if (lattice_persist(vol) && features != vol->features) return BNV_ERR_INVALID_ARGUMENT;
  if (n == 0) return BNV_OK;
  // neighbour rows -> entries read by live lattice points -> MLP on those entries only -> blend.  The marking kernel
  // looks the neighbour rows up itself (one launch and a 10 MB round trip less): always with the per-origin kernel on
  // a volume that keeps its dense row index (k_lattice_mark_o: a thread's 27 look-ups are three rounds of independent
  // loads; tiny-cuda-nn frame 0.254 -> 0.236 ms, fp32 frame unchanged, profiles/r05_experiments.txt [e7]); with the
  // per-point kernel only on small calls (a shard's 1 / world of a frame), where the 256-thread look-up kernel of its
  // own would cost more than it hides (48.7 us for the pair against 62.4 us fused on whole frames)
  if (stages & 1) {
    const int fused_opt = g_fused_mark.load(std::memory_order_relaxed);
    const bool per_origin = g_mark_per_origin.load(std::memory_order_relaxed) != 0;
    const bool fuse = fused_opt == 1 || (fused_opt < 0 && ((per_origin && vol->brick) || n <= 49152 || grid->shard_world > 1));   // (n may be a capacity: a shard's frame holds 1 / world of it)
    if (fuse) {
      BNV_TRY(lattice_neighbors_mark_fused(vol, grid, weights, row_limit, origins, n, n_dev, ws_ptr, ws_bytes, epoch,
                                           prestamped, stream));
    } else {
      BNV_TRY(lattice_neighbors_impl(vol, grid, weights, row_limit, origins, n, n_dev, nullptr, 0, ws_ptr, ws_bytes,
                                     epoch, prestamped, stream));
      BNV_TRY(lattice_mark_impl(vol, n, n_dev, ws_ptr, ws_bytes, epoch, false, stream));
    }
  }
  if (stages & 2) BNV_TRY(lattice_table_impl(vol, grid, features, sdfmlp_pack, n, 1, ws_ptr, ws_bytes, 0, stream));
  if (!(stages & 4) || !out_sdf) return BNV_OK;   // (the caller blends itself: the frame pipeline)
  return bnv_lattice_blend(vol, grid, origins, n, n_dev, delta, ws_ptr, ws_bytes, out_sdf, stream);
}

extern "C" int bnv_decode_lattice(const bnv_volume_t* vol, const bnv_grid_t* grid, const float* features,
                                  const float* weights, int64_t row_limit, const float* sdfmlp_pack,
                                  const int64_t* origins, int64_t n, const int32_t* n_dev, const bnv_sdf_delta_t* delta,
                                  void* ws_ptr, size_t ws_bytes, int32_t epoch, int prestamped, float* out_sdf,
                                  bnv_stream_t stream) {
  return decode_lattice_stages(vol, grid, features, weights, row_limit, sdfmlp_pack, origins, n, n_dev, delta, ws_ptr,
                               ws_bytes, epoch, prestamped != 0, out_sdf, 7, stream);
}
