// Mesh evaluation: area-weighted surface sampling and exact nearest neighbours on a uniform grid -- the hot path of
// the reference's mesh metric (src/scripts/evaluate_bnvf.py:9-31, src/scripts/compute_chamfer.py:36-75: trimesh
// sample_surface + a ball-tree NN query in both directions; bnv_fusion_amd/evaluate.py turns the distances into the
// figures).  Every result is bitwise reproducible from run to run: no float atomic feeds a result, the float64 area
// prefix is a fixed left-to-right chain of tile sums, and the NN tie rule makes the answer independent of the order
// the grid build's integer atomics happen to give the points inside a cell.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "../../include/bnv_fusion.h"
#include "bnv_common.hpp"
#include "cell_grid.hpp"
#include "nn_index.hpp"
#include "scan.hpp"
#include "workspace.hpp"

namespace bnv {

// =====================================================================================================================
// Surface sampling (trimesh.sample.sample_surface)
// =====================================================================================================================
constexpr int kAreaThreads = 256, kAreaItems = 8, kAreaTile = kAreaThreads * kAreaItems;
constexpr uint64_t kUnpublished = ~0ull;   // a NaN bit pattern no prefix of finite non-negative areas can take

struct SampleStatus {
  double total;        // sum of all face areas (the last prefix)
  uint32_t bad_faces;  // faces with a vertex index outside [0, n_vertices)
  uint32_t pad;
};

struct SampleWs {
  double* prefix;        // [F] inclusive prefix of the face areas
  uint64_t* tile_incl;   // [tiles] inclusive prefix up to each tile's last face (double bits), kUnpublished until set
  SampleStatus* status;
};

static size_t sample_ws_layout(int64_t n_faces, char* base, SampleWs* w) {
  Carver c(base);
  SampleWs t;
  t.prefix = c.take<double>(n_faces);
  t.tile_incl = c.take<uint64_t>((n_faces + kAreaTile - 1) / kAreaTile);
  t.status = c.take<SampleStatus>(1);
  if (w) *w = t;
  return c.bytes();
}

// fp32 cross product e1 x e2 and its length sqrt((cx*cx + cy*cy) + cz*cz): one rounding per operation
__device__ __forceinline__ void tri_cross(const float* __restrict__ V, int32_t i0, int32_t i1, int32_t i2, float e1[3],
                                          float e2[3], float c[3], float v0[3], float* len) {
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    v0[d] = V[(int64_t)i0 * 3 + d];
    e1[d] = __fsub_rn(V[(int64_t)i1 * 3 + d], v0[d]);
    e2[d] = __fsub_rn(V[(int64_t)i2 * 3 + d], v0[d]);
  }
  c[0] = __fsub_rn(__fmul_rn(e1[1], e2[2]), __fmul_rn(e1[2], e2[1]));
  c[1] = __fsub_rn(__fmul_rn(e1[2], e2[0]), __fmul_rn(e1[0], e2[2]));
  c[2] = __fsub_rn(__fmul_rn(e1[0], e2[1]), __fmul_rn(e1[1], e2[0]));
  // sqrt in float64 rounded once to fp32 is the correctly rounded fp32 sqrt (53 >= 2 * 24 + 2 bits)
  *len = (float)sqrt((double)__fadd_rn(__fadd_rn(__fmul_rn(c[0], c[0]), __fmul_rn(c[1], c[1])), __fmul_rn(c[2], c[2])));
}

// Face areas (0.5 * |e1 x e2| in fp32; 0 for a face with a bad index or a non-finite area) and their inclusive
// prefix in float64.  Inside a tile: a fixed tree (per-thread runs, wave shuffles, wave totals in order).  Across
// tiles: the decoupled look-back pattern of scan.hpp cut down to its immediate predecessor -- a tile waits for
// the inclusive prefix of tile - 1 and adds its own sum -- because float64 addition is not associative: the prefix
// of every face is then the same sum in the same order on every run.  Tiles are dispatched in index order, so the
// predecessor is resident or finished when a tile waits for it.
__global__ __launch_bounds__(kAreaThreads) void k_face_area_prefix(const float* __restrict__ V, int64_t n_vertices,
                                                                   const int32_t* __restrict__ Fc, int64_t n_faces,
                                                                   SampleWs ws) {
  __shared__ double s_wave[kAreaThreads / 64];
  __shared__ double s_excl;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t base = (int64_t)blockIdx.x * kAreaTile + (int64_t)threadIdx.x * kAreaItems;
  double run[kAreaItems];
  double acc = 0.0;
  uint32_t bad = 0;
#pragma unroll
  for (int e = 0; e < kAreaItems; ++e) {
    const int64_t f = base + e;
    double a = 0.0;
    if (f < n_faces) {
      const int32_t i0 = Fc[f * 3], i1 = Fc[f * 3 + 1], i2 = Fc[f * 3 + 2];
      if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= n_vertices || i1 >= n_vertices || i2 >= n_vertices) {
        bad = 1;
      } else {
        float e1[3], e2[3], c[3], v0[3], len;
        tri_cross(V, i0, i1, i2, e1, e2, c, v0, &len);
        const float af = __fmul_rn(0.5f, len);
        if (af > 0.0f && af <= 3.4028234663852886e38f) a = (double)af;   // NaN / inf count as degenerate
      }
    }
    acc += a;
    run[e] = acc;
  }
  if (bad) atomicOr(&ws.status->bad_faces, 1u);
  // wave inclusive scan of the per-thread sums (Hillis-Steele: the same tree every run)
  const double incl = wave_inclusive_scan(acc);
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  double wbase = 0.0, tile_sum = 0.0;
#pragma unroll
  for (int w = 0; w < kAreaThreads / 64; ++w) {
    if (w == wave) wbase = tile_sum;
    tile_sum += s_wave[w];
  }
  if (threadIdx.x == 0) {
    double excl = 0.0;
    if (blockIdx.x > 0) {
      uint64_t w;
      do {
        w = __hip_atomic_load(&ws.tile_incl[blockIdx.x - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } while (w == kUnpublished);
      excl = __builtin_bit_cast(double, w);
    }
    const double tile_incl = excl + tile_sum;
    __hip_atomic_store(&ws.tile_incl[blockIdx.x], __builtin_bit_cast(uint64_t, tile_incl), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    s_excl = excl;
  }
  __syncthreads();
  const double pre = (s_excl + wbase) + (incl - acc);   // everything before this thread's first face
#pragma unroll
  for (int e = 0; e < kAreaItems; ++e)
    if (base + e < n_faces) {
      ws.prefix[base + e] = pre + run[e];
      if (base + e == n_faces - 1) ws.status->total = pre + run[e];   // the total IS the last prefix
    }
}

// first index i in [0, n) with prefix[i] > key (n if none): a zero-area face never qualifies
__device__ __forceinline__ int64_t first_greater(const double* __restrict__ prefix, int64_t n, double key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (prefix[mid] > key) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_sample_surface(const float* __restrict__ V, const int32_t* __restrict__ Fc,
                                                        int64_t n_faces, const float* __restrict__ U, int64_t n,
                                                        SampleWs ws, float* __restrict__ pts,
                                                        int32_t* __restrict__ face_ids, float* __restrict__ normals) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double total = ws.status->total;
  const float u0 = U[i * 3], u1 = U[i * 3 + 1], u2 = U[i * 3 + 2];
  const double key = (double)(u0 > 0.0f ? u0 : 0.0f) * total;
  int64_t f = first_greater(ws.prefix, n_faces, key);
  // a uniform outside [0, 1) (or NaN): the last face of positive area -- the first whose prefix reaches the total
  if (f >= n_faces) f = first_greater(ws.prefix, n_faces, nextafter(total, -1.0));
  if (f >= n_faces) f = n_faces - 1;   // (unreachable: prefix[n_faces - 1] == total)
  float e1[3], e2[3], c[3], v0[3], len;
  tri_cross(V, Fc[f * 3], Fc[f * 3 + 1], Fc[f * 3 + 2], e1, e2, c, v0, &len);
  float a = u1, b = u2;
  if (__fadd_rn(a, b) > 1.0f) {   // fold the square onto the triangle (sample.py: random_lengths -= 1; abs)
    a = __fsub_rn(1.0f, a);
    b = __fsub_rn(1.0f, b);
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) pts[i * 3 + d] = __fadd_rn(__fadd_rn(v0[d], __fmul_rn(e1[d], a)), __fmul_rn(e2[d], b));
  face_ids[i] = (int32_t)f;
  if (normals) {
#pragma unroll
    for (int d = 0; d < 3; ++d) normals[i * 3 + d] = len > 0.0f ? (float)((double)c[d] / (double)len) : 0.0f;
  }
}

// =====================================================================================================================
// Exact nearest neighbour on a uniform grid
// =====================================================================================================================
// Cell size (cell_grid.hpp: grid_cell_edge): the inputs are surface samples, ~kCellTarget of them in an occupied cell.
// The index (two grids, count / scan / scatter), the stop test and the ring walk of one query (nn_search) are
// nn_index.hpp's, shared with csrc/cloud.hip and csrc/cloud_register.hip.
constexpr double kCellTarget = kNnCellTarget;

struct NnWs {
  NnParams* P;           // [2]: the fine grid, the coarse grid
  uint32_t* ref_count;   // [n_ref + 2]: per cell, then the scan's end sentinel
  uint32_t* ref_start;   // [n_ref + 2]
  uint32_t* q_count;     // [n_ref + 2]: per cell, + one bucket for non-finite queries
  uint32_t* q_start;     // [n_ref + 2]
  uint32_t* ref_cell;    // [n_ref]
  uint32_t* ref_slot;
  uint32_t* q_cell;      // [n_query]
  uint32_t* q_slot;
  uint64_t* scan_state;  // [3 * tiles] look-back words of the three scans
  float4* ref_sorted;    // [n_ref] (x, y, z, bitcast(index)) in cell order
  float4* q_sorted;      // [n_query]
  uint32_t* rc_count;    // the coarse grid's: [n_ref + 2]
  uint32_t* rc_start;    // [n_ref + 2]
  uint32_t* rc_cell;     // [n_ref]
  uint32_t* rc_slot;     // [n_ref]
  float4* rc_sorted;     // [n_ref]
};

static size_t nn_ws_layout(int64_t n_ref, int64_t n_query, char* base, NnWs* w) {
  const int64_t n_bins = n_ref + 2;
  const int64_t tiles = (n_bins + kScanTile - 1) / kScanTile;
  Carver c(base);
  NnWs t;
  t.P = c.take<NnParams>(2);
  t.ref_count = c.take<uint32_t>(n_bins);
  t.ref_start = c.take<uint32_t>(n_bins);
  t.q_count = c.take<uint32_t>(n_bins);
  t.q_start = c.take<uint32_t>(n_bins);
  t.ref_cell = c.take<uint32_t>(n_ref);
  t.ref_slot = c.take<uint32_t>(n_ref);
  t.q_cell = c.take<uint32_t>(n_query);
  t.q_slot = c.take<uint32_t>(n_query);
  t.scan_state = c.take<uint64_t>(tiles * 3);
  t.ref_sorted = c.take<float4>(n_ref);
  t.q_sorted = c.take<float4>(n_query);
  t.rc_count = c.take<uint32_t>(n_bins);
  t.rc_start = c.take<uint32_t>(n_bins);
  t.rc_cell = c.take<uint32_t>(n_ref);
  t.rc_slot = c.take<uint32_t>(n_ref);
  t.rc_sorted = c.take<float4>(n_ref);
  if (w) *w = t;
  return c.bytes();
}

// One thread per query (measured on the fine grid alone against one wave per query, whose lanes split every cell run
// and reduce the best per ring: 3.0 against 2.4 ms at 1M x 1M, 0.22 against 0.18 ms at 100k x 100k; surface cells
// hold a handful of points, too few for 64 lanes).  Queries arrive in the fine grid's cell order (q_sorted), so neighbouring threads
// walk the same cells.  A query that the first kFineRings rings of the fine grid do not settle (a query far from
// every reference point: the fine grid would visit ~(distance / h)^3 mostly empty cells) goes on with the best it
// has on the coarse grid (cells kCoarse times larger): points seen twice change nothing under the tie rule, and the
// coarse search is exact on its own.  kFineRings / kCoarse trade the two cases: 4 / 8 cost 1M x 1M 9.2 ms and a
// 100k query set lying up to a metre off a 2.4M-point mesh 1.6 s; 8 / 4: 5.7 ms and 2.4 s; the fine grid alone:
// 2.4 ms and 4.6 s.
__global__ __launch_bounds__(256) void k_nn_query(const float4* __restrict__ Qs, int64_t n_query,
                                                  const NnParams* __restrict__ Pp, const float4* __restrict__ Rs,
                                                  const uint32_t* __restrict__ rstart, const float4* __restrict__ Rc,
                                                  const uint32_t* __restrict__ cstart, float* __restrict__ d2_out,
                                                  int32_t* __restrict__ idx_out) {
  const int64_t item = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (item >= n_query) return;
  const float4 qv = Qs[item];
  const int32_t qi = __builtin_bit_cast(int32_t, qv.w);
  float best = INFINITY;
  int32_t bi = -1;
  if (Pp[0].n_cells > 0 && finite3(qv.x, qv.y, qv.z)) nn_search(Pp, Rs, rstart, Rc, cstart, qv, best, bi);
  d2_out[qi] = best;
  idx_out[qi] = bi;
}

}  // namespace bnv

using namespace bnv;

extern "C" {

int bnv_mesh_sample_surface_workspace(int64_t n_faces, int64_t* bytes) {
  if (!bytes || n_faces <= 0 || n_faces > INT32_MAX) return BNV_ERR_INVALID_ARGUMENT;
  *bytes = (int64_t)sample_ws_layout(n_faces, nullptr, nullptr);
  return BNV_OK;
}

int bnv_mesh_sample_surface(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces,
                            const float* uniforms, int64_t n, void* workspace, int64_t ws_bytes, float* points_out,
                            int32_t* face_ids_out, float* normals_out, bnv_stream_t stream) {
  if (!vertices || !faces || !uniforms || !workspace || !points_out || !face_ids_out) return BNV_ERR_INVALID_ARGUMENT;
  if (n_vertices <= 0 || n_vertices > INT32_MAX || n_faces <= 0 || n_faces > INT32_MAX || n <= 0 || n > INT32_MAX)
    return BNV_ERR_INVALID_ARGUMENT;
  SampleWs ws;
  if (ws_bytes < (int64_t)sample_ws_layout(n_faces, (char*)workspace, &ws)) return BNV_ERR_WORKSPACE_TOO_SMALL;
  hipStream_t s = (hipStream_t)stream;
  const int64_t tiles = (n_faces + kAreaTile - 1) / kAreaTile;
  BNV_HIP_CHECK(hipMemsetAsync(ws.tile_incl, 0xff, (size_t)tiles * 8, s));
  BNV_HIP_CHECK(hipMemsetAsync(ws.status, 0, sizeof(SampleStatus), s));
  hipLaunchKernelGGL(k_face_area_prefix, dim3((unsigned)tiles), dim3(kAreaThreads), 0, s, vertices, n_vertices, faces,
                     n_faces, ws);
  BNV_LAUNCH_CHECK();
  // the one read of device data: a mesh without area (or with a bad vertex index) cannot be sampled
  SampleStatus st;
  BNV_HIP_CHECK(hipMemcpyAsync(&st, ws.status, sizeof(st), hipMemcpyDeviceToHost, s));
  BNV_HIP_CHECK(hipStreamSynchronize(s));
  if (st.bad_faces || !(st.total > 0.0)) return BNV_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_sample_surface, dim3(blocks_for(n, 256)), dim3(256), 0, s, vertices, faces, n_faces,
                     uniforms, n, ws, points_out, face_ids_out, normals_out);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

int bnv_nn_workspace_bytes(int64_t n_ref, int64_t n_query, int64_t* bytes) {
  if (!bytes || n_ref <= 0 || n_query <= 0 || n_ref > INT32_MAX - 2 || n_query > INT32_MAX)
    return BNV_ERR_INVALID_ARGUMENT;
  *bytes = (int64_t)nn_ws_layout(n_ref, n_query, nullptr, nullptr);
  return BNV_OK;
}

int bnv_nn_query(const float* ref, int64_t n_ref, const float* query, int64_t n_query, void* workspace,
                 int64_t ws_bytes, float* d2_out, int32_t* idx_out, bnv_stream_t stream) {
  if (!ref || !query || !workspace || !d2_out || !idx_out) return BNV_ERR_INVALID_ARGUMENT;
  if (n_ref <= 0 || n_query <= 0 || n_ref > INT32_MAX - 2 || n_query > INT32_MAX) return BNV_ERR_INVALID_ARGUMENT;
  NnWs w;
  if (ws_bytes < (int64_t)nn_ws_layout(n_ref, n_query, (char*)workspace, &w)) return BNV_ERR_WORKSPACE_TOO_SMALL;
  hipStream_t s = (hipStream_t)stream;
  const int64_t n_bins = nn_bins(n_ref), tiles = nn_scan_tiles(n_ref);
  const NnIndex index = {w.P,        w.ref_count, w.ref_start, w.ref_cell,   w.ref_slot,  w.ref_sorted,
                         w.rc_count, w.rc_start,  w.rc_cell,   w.rc_slot,    w.rc_sorted, w.scan_state};
  if (const int e = nn_build_index(ref, n_ref, index, kCellTarget, s)) return e;
  // the queries in the fine grid's cell order: the same count / scan / scatter, from a known state on every call
  BNV_HIP_CHECK(hipMemsetAsync(w.q_count, 0, (size_t)n_bins * 4, s));
  BNV_HIP_CHECK(hipMemsetAsync(w.scan_state + 2 * tiles, 0, (size_t)tiles * 8, s));
  const dim3 q_blocks(blocks_for(n_query, 256));
  hipLaunchKernelGGL(k_nn_count, q_blocks, dim3(256), 0, s, query, n_query, w.P, 1, w.q_count, w.q_cell, w.q_slot);
  BNV_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_grid_scan, dim3((unsigned)tiles), dim3(kScanThreads), 0, s, w.q_count, n_bins, w.q_start,
                     w.scan_state + 2 * tiles, next_epoch());
  BNV_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_nn_scatter, q_blocks, dim3(256), 0, s, query, n_query, w.q_cell, w.q_slot, w.q_start,
                     w.q_sorted);
  BNV_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_nn_query, q_blocks, dim3(256), 0, s, w.q_sorted, n_query, w.P, w.ref_sorted, w.ref_start,
                     w.rc_sorted, w.rc_start, d2_out, idx_out);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

}  // extern "C"
