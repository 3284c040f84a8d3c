// The point index of the exact nearest-neighbour searches: csrc/eval.hip (bnv_nn_query, 1-NN of a query set) and
// csrc/cloud.hip (bnv_cloud_normals, k-NN self-join).  Two uniform grids (cell_grid.hpp) over the finite reference
// points -- a fine one and a coarse one with cells kCoarse times larger -- each built by box / parameters / count /
// scan / scatter into a cell-ordered float4 copy (x, y, z, bitcast(index)).  This is the only place that build is
// written; a user brings its cell target, its workspace layout, and what it does with a cell run.  The 1-NN ring walk
// of one query (nn_take, nn_rings, nn_search) is written here too: bnv_nn_query, bnv_cloud_index_nearest and the
// cloud-to-cloud aligner (csrc/cloud_register.hip) call the same code.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "bnv_common.hpp"
#include "cell_grid.hpp"
#include "scan.hpp"

namespace bnv {
namespace {

constexpr double kStopSlack = 1e-5;    // relative slack of the stop test (fp32 d^2 carries ~4 ulp of rounding)
constexpr int kFineRings = 8;          // rings of the fine grid before a query moves on to the coarse grid
constexpr double kCoarse = 4.0;        // coarse cell edge / fine cell edge
constexpr uint32_t kNoCell = 0xffffffffu;
constexpr double kNnCellTarget = 4.0;  // 1-NN over surface samples: ~4 of them in an occupied cell (grid_cell_edge)

struct NnParams {
  uint32_t bmin[3], bmax[3];   // order-preserving encodings of the finite reference points' bounding box
  int32_t dims[3];
  int32_t n_cells;             // 0: no finite reference point
  double lo[3], fmin[3], fmax[3];
  double h, inv_h;
};
static_assert(offsetof(NnParams, bmin) == 0 && offsetof(NnParams, bmax) == 12, "grid_bbox writes the first six words");

// the pieces of a workspace the build writes (the user's layout carves them)
struct NnIndex {
  NnParams* P;           // [2]: the fine grid, the coarse grid
  uint32_t* ref_count;   // [n_ref + 2]: per cell, then the scan's end sentinel
  uint32_t* ref_start;   // [n_ref + 2]
  uint32_t* ref_cell;    // [n_ref]
  uint32_t* ref_slot;    // [n_ref]
  float4* ref_sorted;    // [n_ref] (x, y, z, bitcast(index)) in cell order
  uint32_t* rc_count;    // the coarse grid's: [n_ref + 2]
  uint32_t* rc_start;    // [n_ref + 2]
  uint32_t* rc_cell;     // [n_ref]
  uint32_t* rc_slot;     // [n_ref]
  float4* rc_sorted;     // [n_ref]
  uint64_t* scan_state;  // [2 * tiles] look-back words of the two scans, tiles = nn_scan_tiles(n_ref)
};

inline int64_t nn_bins(int64_t n_ref) { return n_ref + 2; }
inline int64_t nn_scan_tiles(int64_t n_ref) { return (nn_bins(n_ref) + kScanTile - 1) / kScanTile; }

// the grid of cell size h (grown by 5/4 until it has at most `cap` cells) over the bounding box in P
__device__ void nn_grid(NnParams* __restrict__ P, const double L[3], double h, double cap) {
  double dims[3];
  for (;;) {
    for (int d = 0; d < 3; ++d) dims[d] = fmin(floor(L[d] / h) + 1.0, 2147483647.0);
    if (dims[0] * dims[1] * dims[2] <= cap) break;
    h *= 1.25;
  }
  for (int d = 0; d < 3; ++d) P->dims[d] = (int32_t)dims[d];
  P->n_cells = (int32_t)(dims[0] * dims[1] * dims[2]);
  P->h = h;
  P->inv_h = 1.0 / h;
}

// P[0]: the fine grid (cell_grid.hpp: grid_cell_edge with ~cell_target points in an occupied cell; volumetric sets,
// for which the area estimate asks for far more cells than points, are covered by the cap: h grows by 5/4 until the
// grid has at most max(n_ref, 1) cells); P[1]: the coarse grid, cells kCoarse times larger
__global__ void k_nn_params(NnParams* __restrict__ P, int64_t n_ref, double cell_target) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (P->bmin[0] > P->bmax[0]) {   // no finite reference point
    for (int g = 0; g < 2; ++g) {
      P[g].n_cells = 0;
      for (int d = 0; d < 3; ++d) {
        P[g].dims[d] = 1;
        P[g].lo[d] = P[g].fmin[d] = P[g].fmax[d] = 0.0;
      }
      P[g].h = P[g].inv_h = 1.0;
    }
    return;
  }
  double L[3];
  for (int d = 0; d < 3; ++d) {
    P->fmin[d] = P->lo[d] = (double)ord2f(P->bmin[d]);
    P->fmax[d] = (double)ord2f(P->bmax[d]);
    L[d] = P->fmax[d] - P->fmin[d];
  }
  const double cap = fmax((double)n_ref, 1.0);
  nn_grid(P, L, grid_cell_edge(L, n_ref, cell_target), cap);
  for (int d = 0; d < 3; ++d) {
    P[1].bmin[d] = P->bmin[d];
    P[1].bmax[d] = P->bmax[d];
    P[1].lo[d] = P->lo[d];
    P[1].fmin[d] = P->fmin[d];
    P[1].fmax[d] = P->fmax[d];
  }
  nn_grid(P + 1, L, P->h * kCoarse, cap);
}

// cell of every point (query: the clamped cell; non-finite: the extra bucket n_cells) and its slot in the cell.  The
// slots follow the order the atomics happen in; results do not depend on it (tie rule), only the layout does.
__global__ __launch_bounds__(256) void k_nn_count(const float* __restrict__ X, int64_t n, const NnParams* __restrict__ P,
                                                  int is_query, uint32_t* __restrict__ count,
                                                  uint32_t* __restrict__ cell_of, uint32_t* __restrict__ slot_of) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = X[i * 3], y = X[i * 3 + 1], z = X[i * 3 + 2];
  uint32_t c;
  if (!finite3(x, y, z) || P->n_cells == 0) {
    c = is_query ? (uint32_t)P->n_cells : kNoCell;
  } else {
    const int cx = cell_axis(x, P->lo[0], P->inv_h, P->dims[0]);
    const int cy = cell_axis(y, P->lo[1], P->inv_h, P->dims[1]);
    const int cz = cell_axis(z, P->lo[2], P->inv_h, P->dims[2]);
    c = (uint32_t)(((int64_t)cx * P->dims[1] + cy) * P->dims[2] + cz);
  }
  cell_of[i] = c;
  if (c != kNoCell) slot_of[i] = atomicAdd(&count[c], 1u);
}

__global__ __launch_bounds__(256) void k_nn_scatter(const float* __restrict__ X, int64_t n,
                                                    const uint32_t* __restrict__ cell_of,
                                                    const uint32_t* __restrict__ slot_of,
                                                    const uint32_t* __restrict__ start, float4* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = cell_of[i];
  if (c == kNoCell) return;
  out[start[c] + slot_of[i]] = make_float4(X[i * 3], X[i * 3 + 1], X[i * 3 + 2], __builtin_bit_cast(float, (int32_t)i));
}

__device__ __forceinline__ float nn_d2(float qx, float qy, float qz, const float4 r) {
  const float dx = __fsub_rn(qx, r.x), dy = __fsub_rn(qy, r.y), dz = __fsub_rn(qz, r.z);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// Can the search stop after ring r?  When the ring covers the grid, or when the lower bound on the real d^2 to every
// unvisited point (cell_grid.hpp: grid_ring_bound) exceeds the best fp32 d^2 by the relative slack (continue while it
// is <=).  `best`: the distance a new point has to beat -- the best of a 1-NN search, the k-th best of a k-NN search
// (+inf while its list is not full: continue).
__device__ __forceinline__ bool nn_can_stop(const NnParams& P, const int c[3], int r, const double q[3], float best) {
  double lb;
  if (!grid_ring_bound(P.lo, P.fmin, P.fmax, P.dims, P.h, c, r, q, lb)) return true;
  return lb > (double)best * (1.0 + kStopSlack) + 1e-30;
}

// (d2, idx) lexicographic: the lowest reference index wins a tie
__device__ __forceinline__ void nn_take(float d2, int32_t idx, float& best, int32_t& bi) {
  if (d2 < best || (d2 == best && idx < bi)) {
    best = d2;
    bi = idx;
  }
}

// Ring search of one query on one grid, from ring 0 up to ring `rmax` or until the stop test proves (best, bi) final
// (-> true).  A cell run is read straight from the cell-ordered copy of R (float4: one 16-byte load per point).
// (best, bi) come in as the caller's initial bound: (+inf, -1) for the nearest point whatever its distance; a finite
// `best` with bi = -1 for the nearest point with d2 < best (a point at exactly `best` does not beat index -1), and the
// stop test then ends the walk as soon as nothing unvisited can be that close.
__device__ __forceinline__ bool nn_rings(const NnParams& P, const uint32_t* __restrict__ rstart,
                                         const float4* __restrict__ Rs, const float4 qv, const double q[3], int rmax,
                                         float& best, int32_t& bi) {
  const int c[3] = {cell_axis(qv.x, P.lo[0], P.inv_h, P.dims[0]), cell_axis(qv.y, P.lo[1], P.inv_h, P.dims[1]),
                    cell_axis(qv.z, P.lo[2], P.inv_h, P.dims[2])};
  for (int r = 0; r <= rmax; ++r) {
    grid_ring(c, r, P.dims, rstart, [&](uint32_t k0, uint32_t k1) {
      for (uint32_t k = k0; k < k1; ++k) {
        const float4 rv = Rs[k];
        nn_take(nn_d2(qv.x, qv.y, qv.z, rv), __builtin_bit_cast(int32_t, rv.w), best, bi);
      }
    });
    if (nn_can_stop(P, c, r, q, best)) return true;
  }
  return false;
}

// The 1-NN search of one finite query over both grids of an index that holds a point (Pp[0].n_cells > 0): the first
// kFineRings rings of the fine grid, and a query they do not settle goes on with the best it has on the coarse grid
// (cells kCoarse times larger): points seen twice change nothing under the tie rule, and the coarse search is exact on
// its own.  (best, bi): nn_rings' initial bound in, the answer out.
__device__ __forceinline__ void nn_search(const NnParams* __restrict__ Pp, const float4* __restrict__ Rs,
                                          const uint32_t* __restrict__ rstart, const float4* __restrict__ Rc,
                                          const uint32_t* __restrict__ cstart, const float4 qv, float& best,
                                          int32_t& bi) {
  const double q[3] = {(double)qv.x, (double)qv.y, (double)qv.z};
  const NnParams& F = Pp[0];
  if (!nn_rings(F, rstart, Rs, qv, q, kFineRings, best, bi)) {
    const NnParams& G = Pp[1];
    nn_rings(G, cstart, Rc, qv, q, max(G.dims[0], max(G.dims[1], G.dims[2])), best, bi);
  }
}

// Enqueues the build of both grids over the n_ref points of `ref` (fp32 [n_ref, 3], device).  Everything the build
// accumulates into starts from a known state on every call (also when replayed from a graph): the counts, the
// look-back words (0 = an epoch next_epoch never hands out), the bounding box (grid_bbox).
inline int nn_build_index(const float* ref, int64_t n_ref, const NnIndex& w, double cell_target, hipStream_t s) {
  const int64_t n_bins = nn_bins(n_ref), tiles = nn_scan_tiles(n_ref);
  BNV_HIP_CHECK(hipMemsetAsync(w.ref_count, 0, (size_t)n_bins * 4, s));
  BNV_HIP_CHECK(hipMemsetAsync(w.rc_count, 0, (size_t)n_bins * 4, s));
  BNV_HIP_CHECK(hipMemsetAsync(w.scan_state, 0, (size_t)tiles * 2 * 8, s));
  const dim3 ref_blocks(blocks_for(n_ref, 256));
  if (const int e = grid_bbox(ref, n_ref, w.P, 2 * sizeof(NnParams), s)) return e;
  hipLaunchKernelGGL(k_nn_params, dim3(1), dim3(64), 0, s, w.P, n_ref, cell_target);
  BNV_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_nn_count, ref_blocks, dim3(256), 0, s, ref, n_ref, w.P, 0, w.ref_count, w.ref_cell, w.ref_slot);
  BNV_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_nn_count, ref_blocks, dim3(256), 0, s, ref, n_ref, w.P + 1, 0, w.rc_count, w.rc_cell, w.rc_slot);
  BNV_LAUNCH_CHECK();
  uint32_t* counts[2] = {w.ref_count, w.rc_count};
  uint32_t* starts[2] = {w.ref_start, w.rc_start};
  for (int k = 0; k < 2; ++k) {
    hipLaunchKernelGGL(k_grid_scan, dim3((unsigned)tiles), dim3(kScanThreads), 0, s, counts[k], n_bins, starts[k],
                       w.scan_state + k * tiles, next_epoch());
    BNV_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_nn_scatter, ref_blocks, dim3(256), 0, s, ref, n_ref, w.ref_cell, w.ref_slot, w.ref_start,
                     w.ref_sorted);
  BNV_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_nn_scatter, ref_blocks, dim3(256), 0, s, ref, n_ref, w.rc_cell, w.rc_slot, w.rc_start,
                     w.rc_sorted);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

}  // namespace
}  // namespace bnv
