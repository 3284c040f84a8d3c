// The uniform-grid cell index of csrc/eval.hip (exact nearest neighbour) and csrc/meshsdf.hip (signed distance to a
// mesh): a grid over the bounding box of the finite inputs, built by count / scan / fill and searched ring by ring
// until a lower bound on the distance to every unvisited cell exceeds the best distance.
//
// This is the only place the index is written.  A user brings what differs on purpose: the struct that holds the grid
// (its first six words are the bounding-box keys), kCellTarget, what it files under a cell and does with a run of
// entries, and the last comparison of its stop test.  The clamped cell assignment, the slack terms of the bound and the
// order the cells of a ring are visited in are the ones below, so a fix or a tuning reaches every user.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "bnv_common.hpp"
#include "scan.hpp"

namespace bnv {
namespace {

constexpr int kScanThreads = 256, kScanItems = 4, kScanTile = kScanThreads * kScanItems;

__device__ __forceinline__ uint32_t f2ord(float x) {   // order-preserving float -> uint32
  const uint32_t b = __builtin_bit_cast(uint32_t, x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t k) {
  return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// the cell of a coordinate on one axis, clamped into the grid (a query outside the bounding box: the nearest cell)
__device__ __forceinline__ int cell_axis(float x, double lo, double inv_h, int dim) {
  double t = floor(((double)x - lo) * inv_h);
  t = fmin(fmax(t, 0.0), (double)(dim - 1));
  return (int)t;
}

// Bounding box of the finite points of X into box[0 .. 3) (min) and box[3 .. 6) (max) as f2ord keys: a wave reduction,
// the block's waves through LDS, one integer atomic min / max per component per block.
__global__ __launch_bounds__(256) void k_grid_bbox(const float* __restrict__ X, int64_t n, uint32_t* __restrict__ box) {
  uint32_t mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float x = X[i * 3], y = X[i * 3 + 1], z = X[i * 3 + 2];
    if (!finite3(x, y, z)) continue;
    const uint32_t k[3] = {f2ord(x), f2ord(y), f2ord(z)};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      mn[d] = min(mn[d], k[d]);
      mx[d] = max(mx[d], k[d]);
    }
  }
#pragma unroll
  for (int d = 0; d < 3; ++d)
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      mn[d] = min(mn[d], (uint32_t)__shfl_xor((int)mn[d], s, 64));
      mx[d] = max(mx[d], (uint32_t)__shfl_xor((int)mx[d], s, 64));
    }
  __shared__ uint32_t s_mn[4][3], s_mx[4][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0)
    for (int d = 0; d < 3; ++d) {
      s_mn[wave][d] = mn[d];
      s_mx[wave][d] = mx[d];
    }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int d = threadIdx.x;
    uint32_t a = s_mn[0][d], b = s_mx[0][d];
    for (int w = 1; w < 4; ++w) {
      a = min(a, s_mn[w][d]);
      b = max(b, s_mx[w][d]);
    }
    atomicMin(&box[d], a);
    atomicMax(&box[3 + d], b);
  }
}

// Clears the `bytes` of the struct at `head`, whose first six words are the box (static_assert it at the struct), and
// enqueues the bounding box of the n points of X into them.  An empty box (no finite point) reads min > max.
inline int grid_bbox(const float* X, int64_t n, void* head, size_t bytes, hipStream_t s) {
  BNV_HIP_CHECK(hipMemsetAsync(head, 0, bytes, s));
  BNV_HIP_CHECK(hipMemsetAsync(head, 0xff, 3 * sizeof(uint32_t), s));   // min = the largest key
  const unsigned blocks = std::min(blocks_for(n, 256), 2048u);
  hipLaunchKernelGGL(k_grid_bbox, dim3(blocks), dim3(256), 0, s, X, n, (uint32_t*)head);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

// Cell size rule.  n entries on an area A occupy ~A / h^2 cells of edge h, so h = sqrt(target * A / n) puts ~target
// entries in an occupied cell.  A is estimated by half the bounding box's surface, Lx Ly + Ly Lz + Lz Lx (a height
// field: ~its area; a closed room: half of it).  A set with no area: a line, h = target * L / n; a point, h = 1.
__device__ inline double grid_cell_edge(const double L[3], int64_t n_entries, double target) {
  const double n = (double)n_entries;
  const double S = L[0] * L[1] + L[1] * L[2] + L[2] * L[0];
  const double Lmax = fmax(L[0], fmax(L[1], L[2]));
  double h = S > 0.0 ? sqrt(target * S / n) : (Lmax > 0.0 ? target * Lmax / n : 1.0);
  if (!(h > 0.0) || !isfinite(h)) h = Lmax > 0.0 && isfinite(Lmax) ? Lmax : 1.0;
  return h;
}

// exclusive scan of count[0 .. n_bins) -> start (scan.hpp's block scan + decoupled look-back): one tile of
// kScanTile bins per workgroup, `state` one look-back word per tile, `epoch` from next_epoch()
__global__ __launch_bounds__(kScanThreads) void k_grid_scan(const uint32_t* __restrict__ count, int64_t n_bins,
                                                            uint32_t* __restrict__ start, uint64_t* __restrict__ state,
                                                            uint32_t epoch) {
  __shared__ uint32_t wave_tot[kScanThreads / 64];
  __shared__ uint32_t s_excl;
  const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  uint32_t v[kScanItems], s = 0;
#pragma unroll
  for (int e = 0; e < kScanItems; ++e) {
    v[e] = base + e < n_bins ? count[base + e] : 0u;
    s += v[e];
  }
  uint32_t total;
  uint32_t run = block_exclusive_scan<kScanThreads>(s, wave_tot, &total);
  if (threadIdx.x < 64) {
    const uint32_t excl = lookback_exclusive(state, (int)blockIdx.x, total, epoch);
    if (threadIdx.x == 0) s_excl = excl;
  }
  __syncthreads();
  run += s_excl;
#pragma unroll
  for (int e = 0; e < kScanItems; ++e) {
    if (base + e < n_bins) start[base + e] = run;
    run += v[e];
  }
}

// Ring r around cell c of a grid of dims[3] cells (x-major; start[] is the scan of the cell counts): the cells at
// Chebyshev distance r that lie inside the grid.  run(k0, k1) is called with the entries [k0, k1) of every piece, x
// outer, y inner; the cells of an (x, y) column are contiguous, so a column on the ring's shell is one piece.
template <class Run>
__device__ __forceinline__ void grid_ring(const int c[3], int r, const int dims[3], const uint32_t* __restrict__ start,
                                          Run&& run) {
  const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, dims[0] - 1);
  const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, dims[1] - 1);
  const int zl = c[2] - r, zh = c[2] + r;
  for (int x = x0; x <= x1; ++x)
    for (int y = y0; y <= y1; ++y) {
      const bool shell = x == c[0] - r || x == c[0] + r || y == c[1] - r || y == c[1] + r;
      // the ring's cells of this (x, y) column: a contiguous z-run on the shell, else its two ends
      for (int part = 0; part < (shell ? 1 : 2); ++part) {
        int za, zb;
        if (shell) {
          za = max(zl, 0);
          zb = min(zh, dims[2] - 1);
        } else {
          za = zb = part == 0 ? zl : zh;
          if (za < 0 || za >= dims[2]) continue;
        }
        if (za > zb) continue;
        const int64_t col = ((int64_t)x * dims[1] + y) * dims[2];
        const uint32_t e = start[col + zb + 1];
        run(start[col + za], e);
      }
    }
}

// The bound of the stop test after ring r around cell c (cell edge h, grid origin lo, entries inside [bmin, bmax]).
// An entry listed in a visited cell was tested as a whole.  A point of an unvisited cell lies beyond one face of the
// box of visited cells on some axis (by at least the query's distance to that face, minus a slack for the rounding of
// the cell assignment) and inside the bounding box on the other axes.  -> whether any face of that box is still inside
// the grid (false: the ring covers it, the search is over); lb: the lower bound on the real d^2 to anything unvisited.
// The user compares lb with its best distance, with the slack its own arithmetic needs.
__device__ __forceinline__ bool grid_ring_bound(const double lo[3], const double bmin[3], const double bmax[3],
                                                const int dims[3], double h, const int c[3], int r, const double q[3],
                                                double& lb) {
  double gd2[3], base = 0.0;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double g = fmax(fmax(bmin[d] - q[d], q[d] - bmax[d]), 0.0);
    gd2[d] = g * g;
    base += gd2[d];
  }
  lb = INFINITY;
  bool open = false;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double slack = 1e-12 * (fabs(q[d]) + fabs(lo[d]) + (double)dims[d] * h) + 1e-9 * h;
    if (c[d] - r > 0) {
      open = true;
      const double f = fmax(q[d] - (lo[d] + (double)(c[d] - r) * h) - slack, 0.0);
      lb = fmin(lb, f * f + (base - gd2[d]));
    }
    if (c[d] + r < dims[d] - 1) {
      open = true;
      const double f = fmax((lo[d] + (double)(c[d] + r + 1) * h) - q[d] - slack, 0.0);
      lb = fmin(lb, f * f + (base - gd2[d]));
    }
  }
  return open;
}

}  // namespace
}  // namespace bnv
