// How a voxel coordinate finds its row in the sparse volume: the packed 64-bit key of the hash table and the dense
// row index (brick) that short-cuts it inside the grid.
#pragma once
#include "bnv_common.hpp"

namespace bnv {

// ---- packed volume keys -------------------------------------------------------------------
constexpr uint64_t kEmptyKey = ~0ULL;
constexpr int64_t kKeyOffset = 1 << 20;

__device__ __forceinline__ bool pack_key(int64_t x, int64_t y, int64_t z, uint64_t* key) {
  const int64_t a = x + kKeyOffset, b = y + kKeyOffset, c = z + kKeyOffset;
  if ((uint64_t)a >= (1u << 21) || (uint64_t)b >= (1u << 21) || (uint64_t)c >= (1u << 21)) return false;
  *key = ((uint64_t)a << 42) | ((uint64_t)b << 21) | (uint64_t)c;
  return true;
}

// Row of a key in the slot table, or -1.  Linear probing; rows < 0 are "being inserted".
__device__ __forceinline__ int volume_find(const uint64_t* __restrict__ slot_keys,
                                           const int32_t* __restrict__ slot_rows, uint32_t mask,
                                           uint64_t key) {
  uint32_t s = mix64(key) & mask;
  for (uint32_t probe = 0; probe <= mask; ++probe) {
    const uint64_t k = slot_keys[s];
    if (k == key) return slot_rows[s];
    if (k == kEmptyKey) return -1;
    s = (s + 1) & mask;
  }
  return -1;
}

// ---- dense row index of the grid (bnv_volume_t::brick) -----------------------------------------------------------
__device__ __forceinline__ bool brick_index(const bnv_volume_t& v, int64_t x, int64_t y, int64_t z, int64_t* idx) {
  if ((uint64_t)x >= (uint64_t)v.brick_dims[0] || (uint64_t)y >= (uint64_t)v.brick_dims[1] ||
      (uint64_t)z >= (uint64_t)v.brick_dims[2])
    return false;
  *idx = (x * v.brick_dims[1] + y) * v.brick_dims[2] + z;
  return true;
}

// a row was created for voxel (x, y, z)
__device__ __forceinline__ void brick_set(const bnv_volume_t& v, int64_t x, int64_t y, int64_t z, int32_t row) {
  int64_t idx;
  if (v.brick && brick_index(v, x, y, z, &idx)) v.brick[idx] = row;
}

// Row of voxel (x, y, z) or -1: from the brick when it is kept and the voxel is inside the grid, else from the hash.
__device__ __forceinline__ int volume_row(const bnv_volume_t& v, int64_t x, int64_t y, int64_t z) {
  int64_t idx;
  if (v.brick && brick_index(v, x, y, z, &idx)) return v.brick[idx];
  uint64_t key;
  if (!pack_key(x, y, z, &key)) return -1;
  return volume_find(v.slot_keys, v.slot_rows, (uint32_t)(v.n_slots - 1), key);
}

}  // namespace bnv
