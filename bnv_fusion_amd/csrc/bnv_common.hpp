// Shared device helpers for the gfx950 kernels (wave64, CDNA4).  Compiled with
// -ffp-contract=off: every float op below rounds exactly once, like the reference's ATen CPU ops.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <cmath>

#include "../../include/bnv_fusion.h"

namespace bnv {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kWave = 64;
extern int g_num_cus;   // (these words: runtime.hip)
extern int g_last_hip_error;
// process-wide defaults / A-B switches: relaxed atomic words, read once per launch (bnv_set_mlp_mode, bnv_set_option)
extern std::atomic<int> g_mlp_mode;
extern std::atomic<int> g_reserve_cus;
extern std::atomic<int> g_tcnn_block_encoder;
extern std::atomic<int> g_tcnn_shared_table;
extern std::atomic<int> g_finalize_blocks;
// the arithmetic mode of a call: the grid's own (bnv_grid_t.mlp_mode = 1 + m) or the process default
static inline int mlp_mode_of(int32_t grid_mode) {
  return grid_mode >= 1 && grid_mode <= 4 ? grid_mode - 1 : g_mlp_mode.load(std::memory_order_relaxed);
}
static inline bool mlp_mode_field_ok(int32_t grid_mode) { return grid_mode >= 0 && grid_mode <= 4; }

// optional HIP-event timing of the dominant kernels (bnv_profile_enable / bnv_profile_read)
enum ProfKind { PROF_POINTNET = 0, PROF_DECODE_LATTICE = 1, PROF_DECODE_PTS = 2, PROF_DECODE_DENSE = 3, PROF_KINDS = 4 };
extern bool g_prof_on;
void prof_mark(int kind, bool begin, hipStream_t stream);
// ReLU as ONE instruction: v_max_i32 on the bit pattern (a float with the sign bit set is a negative
// int; -0.0 -> +0.0).  fmaxf() and fmed3 both cost an extra canonicalising v_max under IEEE mode, and an
// inline-asm v_max_f32 would hide the MFMA-result -> VALU hazard from the compiler.
__device__ __forceinline__ float relu_bits(float x) {
  const int b = __builtin_bit_cast(int, x);
  return __builtin_bit_cast(float, b > 0 ? b : 0);
}

// hi/lo f16 split of fp32 values for the split-operand MFMA modes: hi = rn16(x), lo = rn16(x - hi).  Written with
// v_cvt_pk_f16_f32 + v_fma_mixlo/mixhi_f16 (x - hi is formed in fp32 straight from the packed f16 hi and rounded once
// into the destination half): 1.5 VALU ops per value where the plain C++ form compiles to ~2.9 (cvt, cvt back, sub,
// cvt, pack).  Bit-identical to that form, subnormals and overflow included (tools/probe_split_mix.hip).  Plain asm
// (not volatile): the compiler still schedules and dead-code-eliminates it; its inputs come out of a v_max_i32 or a
// plain move, so no MFMA-result hazard is hidden from it.
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ void split_pair_f16(float a, float b, unsigned& hi, unsigned& lo) {
  asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(hi) : "v"(a), "v"(b));
  asm("v_fma_mixlo_f16 %0, -%1, 1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(lo) : "v"(hi), "v"(a));
  asm("v_fma_mixhi_f16 %0, -%1, 1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(lo) : "v"(hi), "v"(b));
}
__device__ __forceinline__ void split8_f16(const float (&x)[8], half8& hi, half8& lo) {
  typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
  u32x4_t h, l;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    unsigned hh, ll;
    split_pair_f16(x[2 * p], x[2 * p + 1], hh, ll);
    h[p] = hh;
    l[p] = ll;
  }
  hi = __builtin_bit_cast(half8, h);
  lo = __builtin_bit_cast(half8, l);
}

// Cooperative global -> LDS copy of `bytes` (a multiple of 16; src and dst 16-byte aligned) by the NT threads of a
// workgroup through the LDS-DMA path (global_load_lds_dwordx4: no VGPR round trip, every piece in flight at once).
// The persistent MLP kernels stage 20-150 KB of weights per workgroup before their first tile; written as a
// load / ds_write loop the compiler kept ONE 16-byte load in flight per thread (load, s_waitcnt vmcnt(0), ds_write,
// branch): 19 dependent memory round trips = ~15 us of every launch of the point encoder.  A wave's piece is 1 KB:
// wave-uniform LDS base + lane * 16.  Ends with vmcnt(0); the caller's __syncthreads() publishes the data.
template <int NT>
__device__ __forceinline__ void stage_to_lds(const void* __restrict__ src, void* __restrict__ lds_dst, int bytes) {
  typedef __attribute__((address_space(1))) const void gptr_t;
  typedef __attribute__((address_space(3))) void lptr_t;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const char* s = (const char*)src;
  char* d = (char*)lds_dst;
  for (int base = wave * 1024; base < bytes; base += NT * 16) {   // (wave-uniform loop)
    if (base + lane * 16 < bytes)
      __builtin_amdgcn_global_load_lds((gptr_t*)(s + base + lane * 16), (lptr_t*)(d + base), 16, 0, 0);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

struct ProfScope {
  int kind;
  hipStream_t stream;
  ProfScope(int k, hipStream_t s) : kind(k), stream(s) { if (g_prof_on) prof_mark(kind, true, stream); }
  ~ProfScope() { if (g_prof_on) prof_mark(kind, false, stream); }
};

#define BNV_HIP_CHECK(expr)                      \
  do {                                           \
    hipError_t _e = (expr);                      \
    if (_e != hipSuccess) {                      \
      bnv::g_last_hip_error = (int)_e;           \
      return BNV_ERR_HIP;                        \
    }                                            \
  } while (0)

#define BNV_LAUNCH_CHECK() BNV_HIP_CHECK(hipGetLastError())

// passes a failed step's code on to the caller
#define BNV_TRY(expr)              \
  do {                             \
    const int _rc = (expr);        \
    if (_rc != BNV_OK) return _rc; \
  } while (0)


// number of workgroups of `threads` threads that cover n items, one item per thread
inline unsigned blocks_for(int64_t n, int threads) { return (unsigned)((n + threads - 1) / threads); }

// argument check of the entry points: every one of the n host values is finite
template <class T>
inline bool all_finite(const T* v, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

// Corner order of get_neighbors (modules.py:590-655): bit0 = x uses ceil, bit1 = y, bit2 = z.
__device__ __constant__ const unsigned char kCornerCeilBits[8] = {0, 1, 2, 4, 3, 5, 6, 7};

// Normalised voxel coordinate of one axis: (x - bound_min) / voxel, two IEEE fp32 roundings
// (local_point_fusion.py:159-160).
__device__ __forceinline__ float voxel_coord(float x, float bmin, float voxel) {
  return __fdiv_rn(__fsub_rn(x, bmin), voxel);
}

__device__ __forceinline__ bool in_bounds(float x, float y, float z, const bnv_grid_t& g) {
  // strict, one-voxel margin (local_point_fusion.py:94-100); NaN fails every comparison.
  return (x < g.bound_hi[0]) && (y < g.bound_hi[1]) && (z < g.bound_hi[2]) &&
         (x > g.bound_lo[0]) && (y > g.bound_lo[1]) && (z > g.bound_lo[2]);
}

// rel = ((xn - gid) * voxel) / voxel  (local_point_fusion.py:163-164 then :59)
__device__ __forceinline__ float relative_coord(float xn, int gid, float voxel) {
  float t = __fsub_rn(xn, (float)gid);
  return __fdiv_rn(__fmul_rn(t, voxel), voxel);
}

__device__ __forceinline__ uint32_t mix64(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdULL;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ULL;
  k ^= k >> 33;
  return (uint32_t)k;
}

// workspace words of the lattice decode that kernels of other files touch (decode_host.hpp: lattice_ws_layout; lattice.hip)
void lattice_ws_frame_words(void* ws, int64_t row_capacity, int32_t** origin_stamp, int32_t** ctl);

}  // namespace bnv
