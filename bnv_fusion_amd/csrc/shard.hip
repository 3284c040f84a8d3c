// shard.hip -- the exchange step of the spatially sharded volume (BASELINE.json north_star:
// "the active-voxel set shards by spatial hash across the GPUs ... with an RCCL all-gather over xGMI of
// boundary-voxel features before decode").  New design: the reference is single-GPU.
//
// A voxel is owned by hash(block coordinate) % world (bnv_common.hpp: voxel_owner).  Fusion needs no exchange: a
// (point, corner) pair belongs to exactly one voxel, every rank voxelises the whole frame and encodes / upserts only
// the voxels it owns.  Decode reads the 3x3x3 neighbourhood of a voxel, so a rank also needs the rows of foreign
// voxels that touch its own: GHOST rows.  A row changes only when its voxel is emitted by a frame's encode, so per
// frame every rank sends the rows it has just updated that are BOUNDARY voxels (some voxel of their 3x3x3
// neighbourhood belongs to another rank -- a function of the coordinates alone), one all-gather moves them, and
// every rank installs the records that touch voxels it owns.  After that the local volume (own rows + ghost rows)
// decodes exactly like the single-GPU volume.
//
//   k_shard_pack     this frame's emitted voxels that are boundary voxels -> 48-byte records (key, weight, feature)
//                    with their LIVE values (after the upsert), appended behind a header record that carries the count
//   k_shard_install  the other ranks' records that are adjacent to this rank: upsert as ghost rows (overwrite)
//
// HBM-bound and small: ~58 % of a frame's emitted voxels at 8^3-voxel blocks, 48 B each.
// First-touch ownership (bnv_grid_t.shard_state: a table instead of the hash) runs inside the encode, behind k_rank:
//   k_shard_assign / k_shard_own   owners for a frame's new blocks; the pair list and exchange bound left open till then
#include "encode.hpp"
#include "scan.hpp"
#include "volume_keys.hpp"

namespace bnv {

__global__ __launch_bounds__(256) void k_shard_pack(bnv_volume_t v, bnv_grid_t g, const int64_t* __restrict__ coords,
                                                    int64_t n, const int32_t* __restrict__ n_dev,
                                                    ShardRec* __restrict__ block, int64_t capacity) {
  if (n_dev) n = (int64_t)*n_dev < n ? (int64_t)*n_dev : n;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool send = false;
  int x = 0, y = 0, z = 0, row = -1;
  if (i < n) {
    x = (int)coords[i * 3 + 0];
    y = (int)coords[i * 3 + 1];
    z = (int)coords[i * 3 + 2];
    if (shard_is_boundary(x, y, z, g)) {
      row = volume_row(v, x, y, z);
      send = row >= 0;
    }
  }
  // append, wave-aggregated: one atomic per wave on the block's counter
  const unsigned long long m = __ballot(send);
  if (!m) return;
  const int lane = threadIdx.x & 63;
  const int leader = (int)__ffsll((long long)m) - 1;
  int base = 0;
  if (lane == leader) base = atomicAdd(&block[0].x, (int)__popcll(m));
  base = __shfl(base, leader, 64);
  if (!send) return;
  const int64_t slot = (int64_t)base + (int64_t)__popcll(m & ((1ull << lane) - 1ull));
  if (slot >= capacity) {
    block[0].z = 1;   // cannot happen when capacity >= the bound bnv_encode_begin reports; checked by the receiver
    return;
  }
  ShardRec r;
  r.x = x;
  r.y = y;
  r.z = z;
  r.w = v.weights[row];
#pragma unroll
  for (int f = 0; f < 8; ++f) r.f[f] = v.features[(size_t)row * 8 + f];
  block[1 + slot] = r;
}

__global__ void k_shard_pack_header(ShardRec* __restrict__ block, int rank) {
  block[0].x = 0;
  block[0].y = rank;
  block[0].z = 0;
}

// Ghost-row look-up of k_shard_install, one thread per record: the row of the record's voxel in
// this rank's volume, created (hash slot claimed by CAS, row number from a wave-aggregated atomic on the row counter:
// ghost rows need no particular order) when it does not exist yet.  Keys are unique over all records of a frame (every
// voxel has one owner, and an owner sends a voxel once), so a slot / row is touched by one thread only.  Every lane of
// the wave must call it (ballot); `want` = this lane holds a record for this rank.  -> row, or -1 (nothing to do, or an
// error that has been written to *error); *created tells a fresh row (coordinates, brick entry and num_hits are set).
__device__ __forceinline__ int64_t ghost_row(const bnv_volume_t& v, const ShardRec& r, bool want, bool* created_out,
                                             int32_t* __restrict__ error) {
  uint64_t key;
  int32_t slot = -1, created = 0;
  if (want) {
    if (pack_key(r.x, r.y, r.z, &key)) {
      const uint32_t mask = (uint32_t)(v.n_slots - 1);
      uint32_t s = mix64(key) & mask;
      for (uint32_t probe = 0; probe <= mask; ++probe) {
        uint64_t k = v.slot_keys[s];
        if (k == kEmptyKey) {
          k = atomicCAS((unsigned long long*)&v.slot_keys[s], (unsigned long long)kEmptyKey, (unsigned long long)key);
          if (k == kEmptyKey) {
            slot = (int32_t)s;
            created = 1;
            break;
          }
        }
        if (k == key) {
          slot = (int32_t)s;
          break;
        }
        s = (s + 1) & mask;
      }
      if (slot < 0) *error = 1;
    } else {
      *error = 2;
    }
  }
  const unsigned long long m = __ballot(created);
  int64_t row = -1;
  if (m) {
    const int lane = threadIdx.x & 63;
    const int leader = (int)__ffsll((long long)m) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(&v.n_rows[0], (int)__popcll(m));
    base = __shfl(base, leader, 64);
    if (created) row = (int64_t)base + (int64_t)__popcll(m & ((1ull << lane) - 1ull));
  }
  *created_out = created != 0;
  if (slot < 0) return -1;
  if (created) {
    if (row >= v.row_capacity) {
      *error = 3;
      return -1;
    }
    v.slot_rows[slot] = (int32_t)row;
    v.row_coords[row * 3 + 0] = r.x;
    v.row_coords[row * 3 + 1] = r.y;
    v.row_coords[row * 3 + 2] = r.z;
    brick_set(v, r.x, r.y, r.z, (int32_t)row);
    v.num_hits[row] = 0.f;
    return row;
  }
  row = v.slot_rows[slot];
  return (row < 0 || row >= v.row_capacity) ? -1 : row;
}

// one thread per (sender, record slot)
__global__ __launch_bounds__(256) void k_shard_install(bnv_volume_t v, bnv_grid_t g,
                                                       const ShardRec* __restrict__ blocks, int world,
                                                       int64_t capacity, int32_t* __restrict__ error,
                                                       ShardRec* __restrict__ own_block) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  // the frame pipeline (pipeline.hip) appends a frame's records from inside the upsert kernel; the block that was
  // just exchanged starts its next frame empty (the collective that read it is complete: this kernel is behind it)
  if (t == 0 && own_block) own_block[0].x = 0;
  const int sender = (int)(t / capacity);
  const int64_t i = t - (int64_t)sender * capacity;
  bool want = false;
  ShardRec r = {};
  if (sender < world && sender != g.shard_rank) {
    const ShardRec* blk = blocks + (size_t)sender * (size_t)(capacity + 1);
    int cnt = blk[0].x;
    // the sender's block overflowed, or it holds more records than were exchanged: records are missing
    if (blk[0].z || cnt > capacity) *error = 4;
    if (cnt > capacity) cnt = (int)capacity;
    if (i < cnt) {
      r = blk[1 + i];
      want = shard_adjacent_to(r.x, r.y, r.z, g, g.shard_rank);
    }
  }
  bool created;
  const int64_t row = ghost_row(v, r, want, &created, error);
  if (row < 0) return;
#pragma unroll
  for (int f = 0; f < 8; ++f) v.features[row * 8 + f] = r.f[f];
  v.weights[row] = r.w;
  if (v.lattice_have) v.lattice_have[row] = 0u;   // a ghost row with new values: its table entries are stale
}

// ---- first-touch ownership (bnv_grid_t.shard_state): owners for the blocks this frame touches for the first time ----
// ONE small workgroup (256 threads, no LDS to speak of: it must find room beside the persistent MLP kernels of the
// other streams, which leave a CU one wave slot per SIMD and little else -- the first version, 1,024 threads, sat in the
// front stream for the whole of a table kernel in every frame); nothing to do (one load) in a frame without a new
// block.  (1) the new blocks in ascending block order: k_rank has listed them (the first voxel that touches a block
// appends it), a bitonic sort of that list in place -- or, when a frame brings more than the list holds (the first
// frame of a scene), an ordered compaction of the dense weight table; (2) one wave walks them: a block that has no
// owner yet goes to the rank with the least load so far (lowest rank on ties), a block that was pinned earlier as
// somebody's neighbour keeps its owner, and either way its weight joins that rank's load; (3) the neighbour blocks of
// the new blocks that still have no owner are pinned to the lattice rule; (4) the weights are cleared.  Every rank
// runs this on the same replicated voxelisation, so every rank's table is the same -- no communication.
// ---- region rule (BNV_SHARD_RULE_REGION; include/bnv_fusion.h: bnv_grid_t.shard_state; host restatement:
// distributed.OwnershipModel) ----------------------------------------------------------------------------------------
// Table bytes are read and written with relaxed agent-scope atomics and a fence behind every store: the walk reads
// entries it has written a few iterations earlier.
__device__ __forceinline__ uint8_t own_load(const uint8_t* t, int64_t i) {
  return __hip_atomic_load(&t[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void own_store(uint8_t* t, int64_t i, uint8_t v) {
  __hip_atomic_store(&t[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// least-loaded rank (lowest rank on ties); load: lane r holds rank r's load
__device__ __forceinline__ int least_rank(unsigned long long load, int world) {
  const int lane = threadIdx.x & 63;
  unsigned long long key = lane < world ? ((load << 6) | (unsigned long long)lane) : ~0ull;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(key, d, 64);
    key = o < key ? o : key;
  }
  return (int)(key & 63ull);
}
// the first wave of k_shard_assign walks the frame's n_new blocks (new_list holds their WALK KEYS, ascending)
__device__ void shard_assign_region(const bnv_grid_t& g, const ShardState& S, uint32_t n_new, uint32_t n_touched) {
  const int lane = threadIdx.x & 63;
  const int world = g.shard_world, axis = S.hdr->axis;
  int nb3[3];
  shard_block_dims(g.n_xyz, g.shard_block_log2, nb3);
  uint32_t cur = lane < world ? S.hdr->cur[lane] : 0u;
  unsigned long long load = lane < world ? S.hdr->load[lane] : 0ull;
  const unsigned long long nt = n_touched;
  // neighbour this lane looks at (lanes 0..26; 13 = the block itself)
  const int ddx = lane / 9 - 1, ddy = (lane / 3) % 3 - 1, ddz = lane % 3 - 1;
  int recv = S.hdr->recv_p1 - 1;
  {
    const uint32_t cr = __shfl(cur, recv < 0 ? 0 : recv, 64);
    if (recv < 0 || (unsigned long long)cr * (unsigned)world >= nt) recv = least_rank(cur, world);
  }
  // (1) owners for the new blocks, in walk order
  for (uint32_t i = 0; i < n_new; ++i) {
    const uint32_t b = shard_walk_block(S.new_list[i], nb3, axis);
    const uint32_t w = S.blk_w[b];
    const uint8_t t = own_load(S.table, b);
    int r;
    if (t & kOwnAssigned) {
      r = (int)(t & kOwnRank);   // pinned earlier: cur counts its voxels already (k_rank)
    } else {
      const int bz = (int)(b % (uint32_t)nb3[2]), by = (int)((b / (uint32_t)nb3[2]) % (uint32_t)nb3[1]),
                bx = (int)(b / ((uint32_t)nb3[2] * (uint32_t)nb3[1]));
      const int x = bx + ddx, y = by + ddy, z = bz + ddz;
      uint8_t tv = 0;
      if (lane < 27 && (unsigned)x < (unsigned)nb3[0] && (unsigned)y < (unsigned)nb3[1] && (unsigned)z < (unsigned)nb3[2])
        tv = own_load(S.table, ((int64_t)x * nb3[1] + y) * nb3[2] + z);
      const int c = (int)(tv & kOwnRank);
      const uint32_t cc = __shfl(cur, c, 64);
      const bool cand = (tv & kOwnAssigned) && (unsigned long long)cc * (unsigned)world < nt;   // assigned and not full
      unsigned long long key = cand ? (((unsigned long long)cc << 6) | (unsigned long long)c) : ~0ull;
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(key, d, 64);
        key = o < key ? o : key;
      }
      if (key != ~0ull) {
        r = (int)(key & 63ull);
      } else {
        const uint32_t cr = __shfl(cur, recv, 64);
        if ((unsigned long long)cr * (unsigned)world >= nt) recv = least_rank(cur, world);
        r = recv;
      }
      if (lane == r) cur += w;
    }
    if (lane == r) load += w;
    if (lane == 0) own_store(S.table, b, (uint8_t)(r | kOwnAssigned | kOwnTouched));
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
  }
  // (2) the untouched neighbours of the new blocks are pinned: regions grow outwards
  {
    const uint32_t cr = __shfl(cur, recv, 64);
    if ((unsigned long long)cr * (unsigned)world * 8ull > 9ull * nt) recv = least_rank(cur, world);
  }
  for (uint32_t i = 0; i < n_new; ++i) {
    const uint32_t b = shard_walk_block(S.new_list[i], nb3, axis);
    int r = (int)(own_load(S.table, b) & kOwnRank);
    const uint32_t cr = __shfl(cur, r, 64);
    if ((unsigned long long)cr * (unsigned)world * 8ull > 9ull * nt) r = recv;   // overloaded: no pins for it
    const int bz = (int)(b % (uint32_t)nb3[2]), by = (int)((b / (uint32_t)nb3[2]) % (uint32_t)nb3[1]),
              bx = (int)(b / ((uint32_t)nb3[2] * (uint32_t)nb3[1]));
    const int x = bx + ddx, y = by + ddy, z = bz + ddz;
    if (lane == 13) S.blk_w[b] = 0u;
    else if (lane < 27 && (unsigned)x < (unsigned)nb3[0] && (unsigned)y < (unsigned)nb3[1] && (unsigned)z < (unsigned)nb3[2]) {
      const int64_t e = ((int64_t)x * nb3[1] + y) * nb3[2] + z;
      if (!(own_load(S.table, e) & kOwnAssigned)) own_store(S.table, e, (uint8_t)(r | kOwnAssigned));
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
  }
  if (lane < world) S.hdr->load[lane] = load;
  if (lane == 0) S.hdr->recv_p1 = recv + 1;
}

__global__ __launch_bounds__(256) void k_shard_assign(bnv_grid_t g, const EncCtl* __restrict__ ctl) {
  ShardState S;
  shard_state_layout(g.n_xyz, g.shard_block_log2, (char*)g.shard_state, &S);
  const uint32_t n_listed = (uint32_t)S.hdr->any_new;     // (k_rank counts the new blocks in it)
  // region rule: contiguous regions keep a rank's load level only while the view stays put; a frame whose most loaded
  // rank carries more than 1.3 x its share of the touched voxels means the camera sweeps -- from then on new territory
  // is handed out by the greedy rule (fine interleave: every rank holds an even sample of any view).  Sticky.
  __shared__ int s_inter;
  if (threadIdx.x < 64) {
    const int lane_ = threadIdx.x;
    uint32_t c = lane_ < g.shard_world ? S.hdr->cur[lane_] : 0u;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const uint32_t o = __shfl_xor(c, d, 64);
      c = o > c ? o : c;
    }
    if (lane_ == 0) {
      int inter = S.hdr->interleave;
      if (!inter && S.hdr->rule == BNV_SHARD_RULE_REGION &&
          (unsigned long long)c * (unsigned)g.shard_world * 10ull > 13ull * (unsigned long long)(uint32_t)ctl->n_unique) {
        inter = 1;
        S.hdr->interleave = 1;
      }
      s_inter = inter;
    }
  }
  __syncthreads();
  if (n_listed == 0) {
    if (threadIdx.x < 64) S.hdr->cur[threadIdx.x] = 0u;   // (k_rank of the NEXT frame adds to it)
    return;
  }
  const bool region = S.hdr->rule == BNV_SHARD_RULE_REGION && !s_inter;
  int nbw[3];
  shard_block_dims(g.n_xyz, g.shard_block_log2, nbw);
  const int axis = region ? S.hdr->axis : 0;
  __shared__ uint32_t wave_tot[4];
  __shared__ uint32_t s_n;
  const int lane = threadIdx.x & 63;
  uint32_t n_new;
  if (n_listed <= kNewListCap) {
    // bitonic sort of new_list[0, n_listed) padded with ~0 to the next power of two, in global memory (L2)
    uint32_t np2 = 1;
    while (np2 < n_listed) np2 <<= 1;
    if (axis != 0)   // the region rule walks in key order: sort the keys
      for (uint32_t i = threadIdx.x; i < n_listed; i += 256) S.new_list[i] = shard_walk_key(S.new_list[i], nbw, axis);
    for (uint32_t i = n_listed + threadIdx.x; i < np2; i += 256) S.new_list[i] = 0xffffffffu;
    __syncthreads();
    for (uint32_t k = 2; k <= np2; k <<= 1)
      for (uint32_t j = k >> 1; j > 0; j >>= 1) {
        for (uint32_t i = threadIdx.x; i < np2; i += 256) {
          const uint32_t l = i ^ j;
          if (l > i) {
            const uint32_t a = S.new_list[i], b = S.new_list[l];
            const bool up = (i & k) == 0;
            if ((a > b) == up) {
              S.new_list[i] = b;
              S.new_list[l] = a;
            }
          }
        }
        __syncthreads();
      }
    n_new = n_listed;
  } else {
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    for (int64_t b0 = 0; b0 < S.n_blocks; b0 += 256) {
      const int64_t b = b0 + threadIdx.x;   // (a walk key: the list comes out in walk order)
      const uint32_t f = (b < S.n_blocks && S.blk_w[shard_walk_block((uint32_t)b, nbw, axis)] > 0) ? 1u : 0u;
      uint32_t tot;
      const uint32_t pos = block_exclusive_scan<256>(f, wave_tot, &tot);
      const uint32_t base = s_n;
      if (f) S.new_list[base + pos] = (uint32_t)b;
      __syncthreads();
      if (threadIdx.x == 0) s_n = base + tot;
      __syncthreads();
    }
    n_new = s_n;
  }
  const int world = g.shard_world;
  if (region) {
    if (threadIdx.x < 64) {
      shard_assign_region(g, S, n_new, (uint32_t)ctl->n_unique);
      S.hdr->cur[lane] = 0u;
      if (lane == 0) S.hdr->any_new = 0;
    }
    return;
  }
  if (threadIdx.x < 64) {
    unsigned long long load = lane < world ? S.hdr->load[lane] : 0ull;
    for (uint32_t i0 = 0; i0 < n_new; i0 += 64) {
      // 64 entries at a time in registers: the walk itself then touches no memory
      const uint32_t i = i0 + lane;
      uint32_t mb = 0, mw = 0, mt = 0;
      if (i < n_new) {
        mb = S.new_list[i];
        mw = S.blk_w[mb];
        mt = S.table[mb];
      }
      int mine = -1;
      const int cnt = (int)(n_new - i0 < 64u ? n_new - i0 : 64u);
      for (int k = 0; k < cnt; ++k) {
        const uint32_t w = __shfl(mw, k, 64), t = __shfl(mt, k, 64);
        const int r = (t & kOwnAssigned) ? (int)(t & kOwnRank) : least_rank(load, world);
        if (lane == r) load += w;
        if (lane == k) mine = r;
      }
      if (i < n_new) S.table[mb] = (uint8_t)(mine | kOwnAssigned | kOwnTouched);
    }
    if (lane < world) S.hdr->load[lane] = load;
  }
  __syncthreads();
  // every new block has its owner now; blocks around them that nobody has touched yet are pinned to the lattice rule
  int nb3[3];
  shard_block_dims(g.n_xyz, g.shard_block_log2, nb3);
  for (uint64_t q = threadIdx.x; q < (uint64_t)n_new * 27u; q += 256) {
    const uint32_t b = S.new_list[q / 27u];
    const int d = (int)(q % 27u);
    if (d == 13) {
      S.blk_w[b] = 0u;   // (4)
      continue;
    }
    const int bz = (int)(b % (uint32_t)nb3[2]), by = (int)((b / (uint32_t)nb3[2]) % (uint32_t)nb3[1]),
              bx = (int)(b / ((uint32_t)nb3[2] * (uint32_t)nb3[1]));
    const int x = bx + d / 9 - 1, y = by + (d / 3) % 3 - 1, z = bz + d % 3 - 1;
    if ((unsigned)x >= (unsigned)nb3[0] || (unsigned)y >= (unsigned)nb3[1] || (unsigned)z >= (unsigned)nb3[2]) continue;
    uint8_t* e = &S.table[((int64_t)x * nb3[1] + y) * nb3[2] + z];
    if (!(*e & kOwnAssigned)) *e = (uint8_t)(shard_lattice_owner(x, y, z, world) | kOwnAssigned);   // (same value from every writer)
  }
  if (threadIdx.x == 0) S.hdr->any_new = 0;
  if (threadIdx.x < 64) S.hdr->cur[threadIdx.x] = 0u;
}

// With the owners of the frame's blocks known: the owned-pair list of the encoder (what the mark kernel does itself
// under the hash rule) and the exchange bound (what k_rank does itself under the hash rule).
__global__ __launch_bounds__(256) void k_shard_own(
    const float* __restrict__ pts, int n_points, bnv_grid_t g, int32_t* __restrict__ pair_list,
    int32_t* __restrict__ n_pairs, const int32_t* __restrict__ orphan_list, const int32_t* __restrict__ ids,
    const int32_t* __restrict__ defer_list, EncCtl* __restrict__ ctl) {
  if (pair_list) {
    // the points the mark kernel left undecided (a corner voxel in a block without an owner at that time)
    const int n_orph = ctl->n_orphans;
    for (int pb = blockIdx.x; pb * 256 < n_orph; pb += gridDim.x) {   // (workgroup-uniform trip count)
      const int o = pb * 256 + threadIdx.x;
      const int i = o < n_orph ? orphan_list[o] : n_points;
      bool valid = false;
      int fx = 0, cx = 0, fy = 0, cy = 0, fz = 0, cz = 0;
      if (i < n_points) {
        const float x = pts[(size_t)i * 6 + 0], y = pts[(size_t)i * 6 + 1], z = pts[(size_t)i * 6 + 2];
        valid = in_bounds(x, y, z, g);
        if (valid) {
          const float xn = voxel_coord(x, g.bound_min[0], g.voxel_size);
          const float yn = voxel_coord(y, g.bound_min[1], g.voxel_size);
          const float zn = voxel_coord(z, g.bound_min[2], g.voxel_size);
          fx = (int)floorf(xn), cx = (int)ceilf(xn);
          fy = (int)floorf(yn), cy = (int)ceilf(yn);
          fz = (int)floorf(zn), cz = (int)ceilf(zn);
        }
      }
      list_owned_pairs(valid, fx, cx, fy, cy, fz, cz, g, i, pair_list, n_pairs);
      __syncthreads();   // s_cnt is reused by the next block of points
    }
  }
  __shared__ int s_hist[64];
  if (threadIdx.x < 64) s_hist[threadIdx.x] = 0;
  __syncthreads();
  // the touched voxels whose boundary test k_rank had to leave open
  const int64_t n = ctl->n_deferred;
  const int nyz = g.n_xyz[1] * g.n_xyz[2];
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (int64_t)gridDim.x * 256) {
    const int id = ids[defer_list[q]];
    const int x = id / nyz, r = id - x * nyz, y = r / g.n_xyz[2], z = r - y * g.n_xyz[2];
    if (shard_is_boundary(x, y, z, g)) atomicAdd(&s_hist[voxel_owner(x, y, z, g) & 63], 1);
  }
  __syncthreads();
  if (threadIdx.x < 64 && threadIdx.x < g.shard_world && s_hist[threadIdx.x])
    atomicAdd(&ctl->shard_boundary[threadIdx.x], s_hist[threadIdx.x]);
}

int launch_shard_own(const EncodeWs& ws, const bnv_grid_t& g, const float* pts, int n_points, int32_t* pair_list,
                     hipStream_t stream) {
  hipLaunchKernelGGL(k_shard_assign, dim3(1), dim3(256), 0, stream, g, (const EncCtl*)ws.ctl);
  BNV_LAUNCH_CHECK();
  // (a frame without a new block leaves it nothing to do: a small grid that strides, not a workgroup per 256 points)
  const int nb = (int)blocks_for(n_points, 256);
  const int cap = 64;
  hipLaunchKernelGGL(k_shard_own, dim3(nb < cap ? (nb > 0 ? nb : 1) : cap), dim3(256), 0, stream, pts, n_points, g,
                     pair_list, &ws.ctl->n_pairs, ws.orphan_list, ws.ids, ws.defer_list, ws.ctl);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

}  // namespace bnv

using namespace bnv;

static bool shard_vol_ok(const bnv_volume_t* v) {
  return v && v->slot_keys && v->slot_rows && v->row_coords && v->features && v->weights && v->num_hits && v->n_rows &&
         v->n_slots > 0 && (v->n_slots & (v->n_slots - 1)) == 0 && v->row_capacity > 0 && v->n_feats == 8;
}

extern "C" {

size_t bnv_shard_state_bytes(const int32_t n_xyz[3], int32_t block_log2) {
  if (!n_xyz || block_log2 < 0 || block_log2 > 8) return 0;
  return shard_state_layout(n_xyz, block_log2, nullptr, nullptr);
}
int bnv_shard_state_configure(void* shard_state, int32_t rule, int32_t axis, bnv_stream_t stream) {
  if (!shard_state || (rule != BNV_SHARD_RULE_GREEDY && rule != BNV_SHARD_RULE_REGION) || axis < 0 || axis > 2)
    return BNV_ERR_INVALID_ARGUMENT;
  const int32_t words[2] = {rule, axis};
  BNV_HIP_CHECK(hipMemcpyAsync((char*)shard_state + offsetof(ShardHdr, rule), words, sizeof(words), hipMemcpyHostToDevice,
                               (hipStream_t)stream));
  BNV_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));   // (a set-up call: `words` lives on this stack frame)
  return BNV_OK;
}
size_t bnv_shard_state_loads_offset(void) { return offsetof(ShardHdr, load); }
size_t bnv_shard_state_table_offset(void) { return kShardHdrBytes; }

int bnv_shard_pack(const bnv_volume_t* vol, const bnv_grid_t* grid, const int64_t* coords, int64_t n,
                   const int32_t* n_dev, void* block, int64_t capacity, bnv_stream_t stream_) {
  if (!shard_vol_ok(vol) || !grid || !block || n < 0 || capacity < 0 || grid->shard_world < 1) return BNV_ERR_INVALID_ARGUMENT;
  if (n > 0 && !coords) return BNV_ERR_INVALID_ARGUMENT;
  hipStream_t stream = (hipStream_t)stream_;
  hipLaunchKernelGGL(k_shard_pack_header, dim3(1), dim3(1), 0, stream, (ShardRec*)block, grid->shard_rank);
  BNV_LAUNCH_CHECK();
  if (n == 0) return BNV_OK;
  hipLaunchKernelGGL(k_shard_pack, dim3(blocks_for(n, 256)), dim3(256), 0, stream, *vol, *grid, coords, n,
                     n_dev, (ShardRec*)block, capacity);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

int bnv_shard_install(const bnv_volume_t* vol, const bnv_grid_t* grid, const void* blocks, int world,
                      int64_t capacity, void* own_send_block, bnv_stream_t stream_) {
  if (!shard_vol_ok(vol) || !grid || !blocks || world < 1 || world != grid->shard_world || capacity < 0)
    return BNV_ERR_INVALID_ARGUMENT;
  if (capacity == 0 || world == 1) return BNV_OK;
  const int64_t total = (int64_t)world * capacity;
  hipLaunchKernelGGL(k_shard_install, dim3(blocks_for(total, 256)), dim3(256), 0, (hipStream_t)stream_, *vol,
                     *grid, (const ShardRec*)blocks, world, capacity, vol->n_rows + 1, (ShardRec*)own_send_block);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

}  // extern "C"
