// Ordered prefix sums on the device: over a wave, over a workgroup, over the workgroups of one launch (decoupled
// look-back), and the one-block top level of a three-launch scan.  Integer sums are exact in any order; the one
// float64 caller (eval.hip: k_face_area_prefix) takes the wave scan only and keeps its own association.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bnv {

// ---- wave-wide inclusive scan (Hillis-Steele, 6 steps) --------------------------------------------------------------
template <class T>
__device__ __forceinline__ T wave_inclusive_scan(T x) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T o = __shfl_up(x, d, 64);
    if (lane >= d) x += o;
  }
  return x;
}

// ---- block-wide exclusive scan of one value per thread (uint32_t or int64_t; THREADS / 64 words of LDS) -------------
// *block_total = the block's sum, in every thread.  Two barriers: the LDS words may be reused right after the call.
template <int THREADS, class T>
__device__ __forceinline__ T block_exclusive_scan(T v, T* lds_wave_totals, T* block_total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T incl = wave_inclusive_scan(v);
  if (lane == 63) lds_wave_totals[wave] = incl;
  __syncthreads();
  T base = 0, total = 0;
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) {
    const T t = lds_wave_totals[w];
    if (w < wave) base += t;
    total += t;
  }
  __syncthreads();
  *block_total = total;
  return base + incl - v;
}

// ---- top level of a three-launch scan: ONE block turns the block sums into exclusive offsets in place ---------------
// (launch 1 wrote block_sums[b] = the sum of block b; launch 3 adds block_sums[blockIdx.x] to its own block scan)
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_scan_top(uint32_t* __restrict__ block_sums, int n_blocks,
                                                      int32_t* __restrict__ total_out) {
  __shared__ uint32_t wave_tot[THREADS / 64];
  uint32_t carry = 0;
  for (int base = 0; base < n_blocks; base += THREADS) {
    const int i = base + threadIdx.x;
    const uint32_t v = (i < n_blocks) ? block_sums[i] : 0;
    uint32_t total;
    const uint32_t ex = block_exclusive_scan<THREADS>(v, wave_tot, &total);
    if (i < n_blocks) block_sums[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) *total_out = (int32_t)carry;
}

// ---- single-pass ordered prefix over the workgroups of ONE launch (decoupled look-back) -------------------------
// Replaces the three launches of a two-level scan (partial sums, top-level scan, apply).  state[tile] is ONE 64-bit
// word: bits 63..34 launch epoch | 33..32 flag (1 = this tile's aggregate, 2 = inclusive prefix up to and including
// this tile) | 31..0 value.  Words left behind by earlier launches carry older epochs and read as "not published
// yet", so the array is never cleared; every launch takes a fresh epoch from next_epoch().  Workgroups are
// dispatched in index order, so a predecessor is always resident or finished when a tile waits for it.
// lookback_exclusive is called by ALL lanes of the first wave of the block with the tile's aggregate (wave-uniform);
// `seed` is added to tile 0's prefix (e.g. the first free row).  Returns the exclusive prefix, in every lane.
uint32_t next_epoch();

__device__ __forceinline__ uint64_t lb_word(uint32_t epoch, uint32_t flag, uint32_t v) {
  return ((uint64_t)(epoch & 0x3fffffffu) << 34) | ((uint64_t)flag << 32) | (uint64_t)v;
}

__device__ __forceinline__ uint32_t lookback_exclusive(uint64_t* __restrict__ state, int tile, uint32_t agg,
                                                       uint32_t epoch, uint32_t seed = 0) {
  const int lane = threadIdx.x & 63;
  if (tile == 0) {
    if (lane == 0) __hip_atomic_store(&state[0], lb_word(epoch, 2, seed + agg), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return seed;
  }
  if (lane == 0) __hip_atomic_store(&state[tile], lb_word(epoch, 1, agg), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint32_t want = epoch & 0x3fffffffu;
  uint32_t excl = 0;
  for (int hi = tile - 1;; hi -= 64) {
    const int p = hi - lane;   // lane 0 looks at the nearest predecessor
    uint64_t w = 0;
    if (p >= 0) {
      do {
        w = __hip_atomic_load(&state[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } while ((uint32_t)(w >> 34) != want);
    }
    const bool incl = p >= 0 && ((uint32_t)(w >> 32) & 3u) == 2u;
    const unsigned long long m = __ballot(incl);
    const int first = m ? (int)__ffsll((long long)m) - 1 : 64;   // lane of the nearest inclusive prefix
    uint32_t v = (p >= 0 && lane <= first) ? (uint32_t)w : 0u;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    excl += v;
    if (m) break;   // (tile 0 always publishes an inclusive prefix, so the walk ends at the latest there)
  }
  if (lane == 0)
    __hip_atomic_store(&state[tile], lb_word(epoch, 2, excl + agg), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return excl;
}

}  // namespace bnv
