// Exact signed distance from arbitrary points to a triangle mesh: the ground truth of embedding-training patches cut
// from a user's meshes (bnv_fusion_amd/patches.py) and a public query of its own (evaluate.MeshSDF).  The reference
// has no counterpart: its patches (<data_dir>/local_shapes/*_noise) were made by a program that is not part of it.
//
// Index (bnv_mesh_sdf_build, all in the caller's workspace): per face the three vertices gathered next to each other,
// angle-weighted vertex pseudonormals and edge pseudonormals (Baerentzen & Aanaes 2005) as 64-bit fixed-point sums,
// the number of faces on every edge (1: boundary, > 2: non-manifold), and two uniform grids of triangle ids (count /
// scan / fill), the second with cells four times larger for queries far from the mesh.  Query (bnv_mesh_sdf_query):
// one thread per query walks the fine grid ring by ring, then the coarse one, until a lower bound on the distance to
// every unvisited cell exceeds the best distance; the closest point on a triangle is the seven-region case analysis
// in fp32 (one rounding per operation: -ffp-contract=off), the sign is that of (query - closest) . pseudonormal of the
// closest feature, taken in float64.  Results are bitwise reproducible: no float atomic feeds a result (the sums are
// integer), and a tie in d^2 goes to the lowest face index, so the order the grid's integer atomics give the
// triangles inside a cell does not matter.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/bnv_fusion.h"
#include "bnv_common.hpp"
#include "meshsdf.hpp"
#include "meshsdf_query.hpp"
#include "scan.hpp"

namespace bnv {
namespace {

// =====================================================================================================================
// Index build
// =====================================================================================================================
// The ladder of candidate grids over the bounding box.  Which level is used is decided once the (triangle, cell) pairs
// of every level are counted (k_msdf_pick): the workspace is a function of the two counts alone, so the grid adapts to
// it, not the other way round.
__global__ void k_msdf_levels(Header* __restrict__ H, int64_t n_vertices, int64_t n_faces, int64_t bytes) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  H->n_vertices = n_vertices;
  H->n_faces = n_faces;
  H->bytes = bytes;
  double L[3] = {0.0, 0.0, 0.0};
  if (H->bmin[0] <= H->bmax[0]) {
    for (int d = 0; d < 3; ++d) {
      H->fmin[d] = H->lo[d] = (double)ord2f(H->bmin[d]);
      H->fmax[d] = (double)ord2f(H->bmax[d]);
      L[d] = H->fmax[d] - H->fmin[d];
    }
  }
  const double Lmax = fmax(L[0], fmax(L[1], L[2]));
  double h = grid_cell_edge(L, n_faces, kCellTarget);
  for (int l = 0; l < kLevels; ++l) {
    if (l == kLevels - 1) h = fmax(h, 2.0 * Lmax + 1.0);   // one cell
    H->level[l].h = h;
    H->level[l].inv_h = 1.0 / h;
    for (int d = 0; d < 3; ++d) H->level[l].dims[d] = (int32_t)fmin(floor(L[d] / h) + 1.0, 2147483647.0);
    h *= kLadder;
  }
  double amax = 0.0;
  for (int d = 0; d < 3; ++d) amax = fmax(amax, fmax(fabs(H->fmin[d]), fabs(H->fmax[d])));
  H->eps_abs = 8.0 * 1.1920928955078125e-07 * amax;
}

// fixed-point add of a float64 vector (integer atomics: any order of the adds gives the same sum)
__device__ __forceinline__ void fixed_add3(long long* __restrict__ acc, const double v[3], double w) {
#pragma unroll
  for (int d = 0; d < 3; ++d)
    atomicAdd((unsigned long long*)&acc[d], (unsigned long long)__double2ll_rn(v[d] * w * kNormalScale));
}

// Per face: validity (k_face_area_prefix's rule: fp32 area 0.5 |e1 x e2| positive and finite, indices in range), the
// gathered vertices, the pseudonormal sums of its three vertices (weight: the face's angle there) and three edges
// (weight 1), and the number of cells its bounding box overlaps on every level of the ladder.
__global__ __launch_bounds__(256) void k_msdf_faces(const float* __restrict__ V, int64_t n_vertices,
                                                    const int32_t* __restrict__ Fc, int64_t n_faces, Ws W) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  Header* __restrict__ H = W.H;
  bool valid = false;
  float p[3][3];
  double P[3][3], nrm[3];
  int32_t idx[3] = {-1, -1, -1};
  if (f < n_faces) {
    idx[0] = Fc[f * 3];
    idx[1] = Fc[f * 3 + 1];
    idx[2] = Fc[f * 3 + 2];
    valid = idx[0] >= 0 && idx[1] >= 0 && idx[2] >= 0 && idx[0] < n_vertices && idx[1] < n_vertices &&
            idx[2] < n_vertices;
    if (valid) {
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          p[k][d] = V[(int64_t)idx[k] * 3 + d];
          P[k][d] = (double)p[k][d];
        }
      float e1[3], e2[3], c[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        e1[d] = p[1][d] - p[0][d];
        e2[d] = p[2][d] - p[0][d];
      }
      c[0] = e1[1] * e2[2] - e1[2] * e2[1];
      c[1] = e1[2] * e2[0] - e1[0] * e2[2];
      c[2] = e1[0] * e2[1] - e1[1] * e2[0];
      const float len = (float)sqrt((double)((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]));
      const float af = 0.5f * len;
      // the unit normal in float64 from the fp32 positions; a face whose fp32 area is rounding noise over an exactly
      // zero cross product has no normal and is skipped as well
      double a[3], b[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        a[d] = P[1][d] - P[0][d];
        b[d] = P[2][d] - P[0][d];
      }
      nrm[0] = a[1] * b[2] - a[2] * b[1];
      nrm[1] = a[2] * b[0] - a[0] * b[2];
      nrm[2] = a[0] * b[1] - a[1] * b[0];
      const double l = sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
      valid = af > 0.0f && af <= 3.4028234663852886e38f && l > 0.0;
#pragma unroll
      for (int d = 0; d < 3; ++d) nrm[d] /= l;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
      W.tri[f * 3 + k] = valid ? make_float4(p[k][0], p[k][1], p[k][2], __builtin_bit_cast(float, idx[k]))
                               : make_float4(0.f, 0.f, 0.f, __builtin_bit_cast(float, (int32_t)-1));
  }
  if (valid) {
    for (int k = 0; k < 3; ++k) {
      const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
      double a[3], b[3], x[3];
      for (int d = 0; d < 3; ++d) {
        a[d] = P[k1][d] - P[k][d];
        b[d] = P[k2][d] - P[k][d];
      }
      x[0] = a[1] * b[2] - a[2] * b[1];
      x[1] = a[2] * b[0] - a[0] * b[2];
      x[2] = a[0] * b[1] - a[1] * b[0];
      const double angle = atan2(sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]), a[0] * b[0] + a[1] * b[1] + a[2] * b[2]);
      fixed_add3(&W.vacc[(int64_t)idx[k] * 3], nrm, angle);
      // the edge (k, k1)
      const unsigned long long key = edge_key(idx[k], idx[k1]);
      uint32_t s = edge_slot0(key, W.ecap);
      for (uint32_t probe = 0; probe < W.ecap; ++probe) {
        const unsigned long long prev = atomicCAS(&W.ekey[s], kNoEdge, key);
        if (prev == kNoEdge || prev == key) {
          fixed_add3(&W.eacc[(int64_t)s * 3], nrm, 1.0);
          atomicAdd(&W.ecnt[s], 1u);
          break;
        }
        s = (s + 1) & (W.ecap - 1);
      }
    }
  }
  // cells the bounding box overlaps on every level, summed over the wave (every lane of the block arrives here)
  float mn[3] = {0.f, 0.f, 0.f}, mx[3] = {0.f, 0.f, 0.f};
  if (valid) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      mn[d] = fminf(p[0][d], fminf(p[1][d], p[2][d]));
      mx[d] = fmaxf(p[0][d], fmaxf(p[1][d], p[2][d]));
    }
  }
  for (int l = 0; l < kLevels; ++l) {
    const Level& G = H->level[l];
    double n = 1.0;
#pragma unroll
    for (int d = 0; d < 3; ++d)
      n *= (double)(cell_axis(mx[d], H->lo[d], G.inv_h, G.dims[d]) - cell_axis(mn[d], H->lo[d], G.inv_h, G.dims[d]) + 1);
    unsigned long long v = valid ? (unsigned long long)fmin(n, 4294967296.0) : 0ull;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&H->pairs[l], v);
  }
}

// the first level whose grid fits the workspace: cells and (triangle, cell) pairs; the last level (one cell) always does
__global__ void k_msdf_pick(Header* __restrict__ H, int64_t cellcap, int64_t paircap) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int l = 0;
  for (; l < kLevels - 1; ++l) {
    const Level& G = H->level[l];
    const double cells = (double)G.dims[0] * (double)G.dims[1] * (double)G.dims[2];
    if (cells <= (double)cellcap && H->pairs[l] <= (unsigned long long)paircap) break;
  }
  const Level& G = H->level[l];
  H->chosen = l;
  H->h = G.h;
  H->inv_h = G.inv_h;
  const bool any = H->pairs[kLevels - 1] > 0;   // a valid triangle exists
  for (int g = 0; g < 2; ++g) {
    int64_t n = 1;
    for (int d = 0; d < 3; ++d) {
      H->dims[g][d] = g == 0 ? G.dims[d] : ((G.dims[d] - 1) >> kCoarseShift) + 1;
      n *= H->dims[g][d];
    }
    H->n_cells[g] = any ? (int32_t)n : 0;
  }
  H->tests = 0;
  H->magic = kMagic;
}

// a vertex inherits the flags of its edges: on the boundary if an incident edge has one face, non-manifold if an
// incident edge has more than two
__global__ __launch_bounds__(256) void k_msdf_vflags(Ws W) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= W.ecap) return;
  const unsigned long long key = W.ekey[s];
  if (key == kNoEdge) return;
  const uint32_t c = W.ecnt[s];
  const uint32_t flag = c == 1 ? 0x10u : (c > 2 ? 0x20u : 0u);
  if (flag) {
    atomicOr(&W.vflag[(uint32_t)(key >> 32)], flag);
    atomicOr(&W.vflag[(uint32_t)key], flag);
  }
}

// cell range of a triangle's bounding box on grid g (coarse cell = fine cell >> kCoarseShift, so a triangle overlaps
// no more coarse cells than fine ones)
__device__ __forceinline__ void tri_cells(const Header& H, int g, const float4 a, const float4 b, const float4 c,
                                          int c0[3], int c1[3]) {
  const float mn[3] = {fminf(a.x, fminf(b.x, c.x)), fminf(a.y, fminf(b.y, c.y)), fminf(a.z, fminf(b.z, c.z))};
  const float mx[3] = {fmaxf(a.x, fmaxf(b.x, c.x)), fmaxf(a.y, fmaxf(b.y, c.y)), fmaxf(a.z, fmaxf(b.z, c.z))};
  const int sh = g ? kCoarseShift : 0;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    c0[d] = cell_axis(mn[d], H.lo[d], H.inv_h, H.dims[0][d]) >> sh;
    c1[d] = cell_axis(mx[d], H.lo[d], H.inv_h, H.dims[0][d]) >> sh;
  }
}

// FILL = false: count the triangles of every cell; FILL = true: write the ids (the slot inside a cell follows the
// order of the atomics; results do not depend on it -- tie rule)
template <bool FILL>
__global__ __launch_bounds__(256) void k_msdf_cells(Ws W, int g) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const Header& H = *W.H;
  if (f >= H.n_faces || H.n_cells[g] == 0) return;
  const float4 a = W.tri[f * 3], b = W.tri[f * 3 + 1], c = W.tri[f * 3 + 2];
  if (__builtin_bit_cast(int32_t, a.w) < 0) return;
  int c0[3], c1[3];
  tri_cells(H, g, a, b, c, c0, c1);
  for (int x = c0[0]; x <= c1[0]; ++x)
    for (int y = c0[1]; y <= c1[1]; ++y)
      for (int z = c0[2]; z <= c1[2]; ++z) {
        const int64_t cell = ((int64_t)x * H.dims[g][1] + y) * H.dims[g][2] + z;
        if (FILL) {
          const uint32_t left = atomicSub(&W.count[g][cell], 1u);
          const uint64_t slot = (uint64_t)W.start[g][cell] + left - 1u;
          if (slot < (uint64_t)W.paircap) W.ids[g][slot] = (uint32_t)f;
        } else {
          atomicAdd(&W.count[g][cell], 1u);
        }
      }
}

// =====================================================================================================================
// Query
// =====================================================================================================================

// One thread per query (eval.hip's k_nn_query: cells hold a handful of triangles, too few for 64 lanes).  The search
// itself (the closest point of a triangle, the rings of the two grids, the closest feature's flags) is
// meshsdf_query.hpp's, shared with csrc/register.hip.
__global__ __launch_bounds__(256) void k_msdf_query(char* __restrict__ ws, int64_t ws_bytes,
                                                    const float* __restrict__ Q, int64_t n_query,
                                                    float* __restrict__ sdf_out, int32_t* __restrict__ face_out,
                                                    float* __restrict__ closest_out, uint8_t* __restrict__ feature_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_query) return;
  const Header& H = *(const Header*)ws;
  const float qf[3] = {Q[i * 3], Q[i * 3 + 1], Q[i * 3 + 2]};
  const bool ok = msdf_usable(H, ws_bytes) && finite3(qf[0], qf[1], qf[2]);
  float sdf = __builtin_nanf("");
  int32_t face = -1;
  uint32_t feature = 0;
  float cpt[3] = {sdf, sdf, sdf};
  if (ok) {
    Ws W;
    msdf_layout(H.n_vertices, H.n_faces, ws, &W);
    const double q[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
    Best best;
    uint32_t tests = 0;
    msdf_search(H, W, qf, q, best, tests);
#ifdef BNV_MESHSDF_COUNT_TESTS
    atomicAdd(&W.H->tests, (unsigned long long)tests);
#endif
    if (best.face != INT32_MAX) {   // (always: the coarse search covers the grid, which holds a valid triangle)
    // the sign: (q - closest) . pseudonormal of the closest feature, in float64
    const float4 T[3] = {W.tri[(int64_t)best.face * 3], W.tri[(int64_t)best.face * 3 + 1],
                         W.tri[(int64_t)best.face * 3 + 2]};
    const int32_t vi0 = __builtin_bit_cast(int32_t, T[0].w), vi1 = __builtin_bit_cast(int32_t, T[1].w),
                  vi2 = __builtin_bit_cast(int32_t, T[2].w);
    double dot;
    if (best.code == 0) {
      // the face: (q - a) . (ab x ac), which equals (q - closest) . n for a closest point in the face's plane
      const double a[3] = {(double)T[1].x - (double)T[0].x, (double)T[1].y - (double)T[0].y, (double)T[1].z - (double)T[0].z};
      const double b[3] = {(double)T[2].x - (double)T[0].x, (double)T[2].y - (double)T[0].y, (double)T[2].z - (double)T[0].z};
      const double n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
      dot = ((q[0] - (double)T[0].x) * n[0] + (q[1] - (double)T[0].y) * n[1]) + (q[2] - (double)T[0].z) * n[2];
    } else {
      const double d[3] = {q[0] - (double)best.c[0], q[1] - (double)best.c[1], q[2] - (double)best.c[2]};
      const long long* acc;
      feature = msdf_feature(W, best, vi0, vi1, vi2, acc);
      dot = acc ? (d[0] * (double)acc[0] + d[1] * (double)acc[1]) + d[2] * (double)acc[2] : 0.0;
    }
    const float dist = (float)sqrt((double)best.d2);
    sdf = dot < 0.0 ? -dist : dist;
    face = best.face;
    cpt[0] = best.c[0];
    cpt[1] = best.c[1];
    cpt[2] = best.c[2];
    }
  }
  sdf_out[i] = sdf;
  if (face_out) face_out[i] = face;
  if (closest_out) {
    closest_out[i * 3] = cpt[0];
    closest_out[i * 3 + 1] = cpt[1];
    closest_out[i * 3 + 2] = cpt[2];
  }
  if (feature_out) feature_out[i] = (uint8_t)feature;
}

bool counts_ok(int64_t nv, int64_t nf) { return nv > 0 && nf > 0 && nv <= kMaxVertices && nf <= kMaxFaces; }

}  // namespace
}  // namespace bnv

using namespace bnv;

extern "C" {

int bnv_mesh_sdf_workspace_bytes(int64_t n_vertices, int64_t n_faces, int64_t* bytes) {
  if (!bytes || !counts_ok(n_vertices, n_faces)) return BNV_ERR_INVALID_ARGUMENT;
  *bytes = (int64_t)msdf_layout(n_vertices, n_faces, nullptr, nullptr);
  return BNV_OK;
}

int bnv_mesh_sdf_build(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces,
                       void* workspace, int64_t ws_bytes, bnv_stream_t stream) {
  if (!vertices || !faces || !workspace || !counts_ok(n_vertices, n_faces)) return BNV_ERR_INVALID_ARGUMENT;
  Ws W;
  const int64_t need = (int64_t)msdf_layout(n_vertices, n_faces, (char*)workspace, &W);
  if (ws_bytes < need) return BNV_ERR_INVALID_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  const int64_t n_bins = W.cellcap + 2;
  // everything the build accumulates into starts from a known state on every call
  BNV_HIP_CHECK(hipMemsetAsync(W.vacc, 0, (size_t)n_vertices * 24, s));
  BNV_HIP_CHECK(hipMemsetAsync(W.vflag, 0, (size_t)n_vertices * 4, s));
  BNV_HIP_CHECK(hipMemsetAsync(W.ekey, 0xff, (size_t)W.ecap * 8, s));
  BNV_HIP_CHECK(hipMemsetAsync(W.eacc, 0, (size_t)W.ecap * 24, s));
  BNV_HIP_CHECK(hipMemsetAsync(W.ecnt, 0, (size_t)W.ecap * 4, s));
  BNV_HIP_CHECK(hipMemsetAsync(W.count[0], 0, (size_t)n_bins * 4, s));
  BNV_HIP_CHECK(hipMemsetAsync(W.count[1], 0, (size_t)n_bins * 4, s));
  BNV_HIP_CHECK(hipMemsetAsync(W.scan_state, 0, (size_t)W.tiles * 2 * 8, s));
  const dim3 face_blocks(blocks_for(n_faces, 256));
  if (const int e = grid_bbox(vertices, n_vertices, W.H, sizeof(Header), s)) return e;   // clears the header
  hipLaunchKernelGGL(k_msdf_levels, dim3(1), dim3(64), 0, s, W.H, n_vertices, n_faces, need);
  BNV_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_msdf_faces, face_blocks, dim3(256), 0, s, vertices, n_vertices, faces, n_faces, W);
  BNV_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_msdf_pick, dim3(1), dim3(64), 0, s, W.H, W.cellcap, W.paircap);
  BNV_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_msdf_vflags, dim3(blocks_for(W.ecap, 256)), dim3(256), 0, s, W);
  BNV_LAUNCH_CHECK();
  for (int g = 0; g < 2; ++g) {
    hipLaunchKernelGGL(k_msdf_cells<false>, face_blocks, dim3(256), 0, s, W, g);
    BNV_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_grid_scan, dim3((unsigned)W.tiles), dim3(kScanThreads), 0, s, W.count[g], n_bins, W.start[g],
                       W.scan_state + g * W.tiles, next_epoch());
    BNV_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_msdf_cells<true>, face_blocks, dim3(256), 0, s, W, g);
    BNV_LAUNCH_CHECK();
  }
  return BNV_OK;
}

int bnv_mesh_sdf_query(const void* workspace, int64_t ws_bytes, const float* query, int64_t n_query, float* sdf_out,
                       int32_t* face_out, float* closest_out, uint8_t* feature_out, bnv_stream_t stream) {
  if (!workspace || !query || !sdf_out || n_query <= 0 || n_query > INT32_MAX) return BNV_ERR_INVALID_ARGUMENT;
  if (ws_bytes < (int64_t)msdf_layout(1, 1, nullptr, nullptr)) return BNV_ERR_INVALID_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_msdf_query, dim3(blocks_for(n_query, 256)), dim3(256), 0, s, (char*)workspace, ws_bytes,
                     query, n_query, sdf_out, face_out, closest_out, feature_out);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

}  // extern "C"
