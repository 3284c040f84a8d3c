// The device search of the mesh index (meshsdf.hpp), written once: csrc/meshsdf.hip answers point queries with it
// (k_msdf_query) and csrc/register.hip pairs a point cloud with the mesh (k_reg_accumulate).  The closest point of one
// triangle, the ring search over the two grids with its stop test, and the lookup of the closest feature's class,
// flags and pseudonormal sum.  fp32 where the closest point is formed, one rounding per operation
// (-ffp-contract=off); (d2, face) lexicographic, so the order of the triangles inside a cell does not matter.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bnv_common.hpp"
#include "meshsdf.hpp"

namespace bnv {
namespace {

__device__ __forceinline__ uint32_t edge_slot0(unsigned long long key, uint32_t ecap) { return mix64(key) & (ecap - 1); }
__device__ __forceinline__ unsigned long long edge_key(int32_t a, int32_t b) {
  const uint32_t lo = (uint32_t)min(a, b), hi = (uint32_t)max(a, b);
  return ((unsigned long long)lo << 32) | hi;
}

struct Best {
  float d2;
  int32_t face;
  int32_t code;   // 0 face | 1 edge ab, 2 edge bc, 3 edge ca | 4 vertex a, 5 vertex b, 6 vertex c
  float c[3];
};

// Closest point of triangle (a, b, c) to q: the seven Voronoi regions of the triangle (three vertices, three edges,
// the face), decided by the signs of the projections d1 .. d6 and of the barycentric numerators va, vb, vc.  fp32, one
// rounding per operation.  (d2, face) lexicographic: the lowest face index wins a tie.
__device__ __forceinline__ void tri_test(const float q[3], const float4 A, const float4 B, const float4 C, int32_t f,
                                         Best& best) {
  const float ab[3] = {B.x - A.x, B.y - A.y, B.z - A.z}, ac[3] = {C.x - A.x, C.y - A.y, C.z - A.z};
  const float ap[3] = {q[0] - A.x, q[1] - A.y, q[2] - A.z};
  const float bp[3] = {q[0] - B.x, q[1] - B.y, q[2] - B.z};
  const float cp[3] = {q[0] - C.x, q[1] - C.y, q[2] - C.z};
  const float d1 = (ab[0] * ap[0] + ab[1] * ap[1]) + ab[2] * ap[2], d2 = (ac[0] * ap[0] + ac[1] * ap[1]) + ac[2] * ap[2];
  const float d3 = (ab[0] * bp[0] + ab[1] * bp[1]) + ab[2] * bp[2], d4 = (ac[0] * bp[0] + ac[1] * bp[1]) + ac[2] * bp[2];
  const float d5 = (ab[0] * cp[0] + ab[1] * cp[1]) + ab[2] * cp[2], d6 = (ac[0] * cp[0] + ac[1] * cp[1]) + ac[2] * cp[2];
  const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  float s = 0.0f, t = 0.0f;   // closest = a + s ab + t ac
  int code;
  if (d1 <= 0.0f && d2 <= 0.0f) {
    code = 4;
  } else if (d3 >= 0.0f && d4 <= d3) {
    code = 5;
    s = 1.0f;
  } else if (d6 >= 0.0f && d5 <= d6) {
    code = 6;
    t = 1.0f;
  } else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
    code = 1;
    s = d1 / (d1 - d3);
  } else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
    code = 3;
    t = d2 / (d2 - d6);
  } else if (va <= 0.0f && (d4 - d3) >= 0.0f && (d5 - d6) >= 0.0f) {
    code = 2;
    t = (d4 - d3) / ((d4 - d3) + (d5 - d6));
    s = 1.0f - t;
  } else {
    code = 0;
    const float denom = 1.0f / ((va + vb) + vc);
    s = vb * denom;
    t = vc * denom;
  }
  float c[3];
  if (code == 5) {
    c[0] = B.x; c[1] = B.y; c[2] = B.z;
  } else if (code == 6) {
    c[0] = C.x; c[1] = C.y; c[2] = C.z;
  } else if (code == 2) {   // b + t (c - b)
    c[0] = B.x + t * (C.x - B.x);
    c[1] = B.y + t * (C.y - B.y);
    c[2] = B.z + t * (C.z - B.z);
  } else {
    c[0] = (A.x + s * ab[0]) + t * ac[0];
    c[1] = (A.y + s * ab[1]) + t * ac[1];
    c[2] = (A.z + s * ab[2]) + t * ac[2];
  }
  const float dx = q[0] - c[0], dy = q[1] - c[1], dz = q[2] - c[2];
  const float dd = (dx * dx + dy * dy) + dz * dz;
  if (dd < best.d2 || (dd == best.d2 && f < best.face)) {
    best.d2 = dd;
    best.face = f;
    best.code = code;
    best.c[0] = c[0];
    best.c[1] = c[1];
    best.c[2] = c[2];
  }
}

// Can the search stop after ring r of grid g (cell edge hh)?  When the ring covers the grid, or when the lower bound on
// the distance to every triangle not yet tested (cell_grid.hpp: grid_ring_bound; a point of a triangle lies in a cell
// the triangle is listed in) exceeds the best fp32 distance by the relative and the absolute slack (the fp32 closest
// point carries a few ulp of the largest coordinate).
__device__ __forceinline__ bool can_stop(const Header& H, int g, double hh, const int c[3], int r, const double q[3],
                                         float best_d2) {
  double lb;
  if (!grid_ring_bound(H.lo, H.fmin, H.fmax, H.dims[g], hh, c, r, q, lb)) return true;
  const double bd = sqrt((double)best_d2) * (1.0 + kStopSlack) + H.eps_abs;
  return lb > bd * bd;
}

// ring search of one query on grid g, rings 0 .. rmax, until the stop test proves `best` final (-> true)
__device__ __forceinline__ bool rings(const Header& H, const Ws& W, int g, const float qf[3], const double q[3],
                                      int rmax, Best& best, uint32_t& tests) {
  const int sh = g ? kCoarseShift : 0;
  const double hh = H.h * (double)(1 << sh);
  const int c[3] = {cell_axis(qf[0], H.lo[0], H.inv_h, H.dims[0][0]) >> sh,
                    cell_axis(qf[1], H.lo[1], H.inv_h, H.dims[0][1]) >> sh,
                    cell_axis(qf[2], H.lo[2], H.inv_h, H.dims[0][2]) >> sh};
  const int dims[3] = {H.dims[g][0], H.dims[g][1], H.dims[g][2]};
  const uint32_t* __restrict__ ids = W.ids[g];
  const float4* __restrict__ tri = W.tri;
  for (int r = 0; r <= rmax; ++r) {
    grid_ring(c, r, dims, W.start[g], [&](uint32_t k0, uint32_t k1) {
      for (uint32_t k = k0; k < k1; ++k) {
        const uint32_t f = ids[k];
        tri_test(qf, tri[(int64_t)f * 3], tri[(int64_t)f * 3 + 1], tri[(int64_t)f * 3 + 2], (int32_t)f, best);
        ++tests;
      }
    });
    if (can_stop(H, g, hh, c, r, q, best.d2)) return true;
  }
  return false;
}

// is the index at `ws` one a finite query can be answered from?
__device__ __forceinline__ bool msdf_usable(const Header& H, int64_t ws_bytes) {
  return H.magic == kMagic && H.bytes <= ws_bytes && H.n_cells[0] > 0;
}

// The whole search of one finite query: a query that the first kFineRings rings of the fine grid do not settle goes
// on, with the best it has, on the coarse grid, whose search is exact on its own; a triangle seen twice changes
// nothing under the tie rule.  best.face stays INT32_MAX only when nothing was found (never: the coarse search covers
// the grid, which holds a valid triangle).
__device__ __forceinline__ void msdf_search(const Header& H, const Ws& W, const float qf[3], const double q[3],
                                            Best& best, uint32_t& tests) {
  best.d2 = INFINITY;
  best.face = INT32_MAX;
  best.code = 0;
  best.c[0] = best.c[1] = best.c[2] = 0.0f;
  if (!rings(H, W, 0, qf, q, kFineRings, best, tests))
    rings(H, W, 1, qf, q, max(H.dims[1][0], max(H.dims[1][1], H.dims[1][2])), best, tests);
}

// The closest feature of a finished search that ended on an edge or a vertex (best.code != 0): its class (1 edge, 2
// vertex) with the boundary (0x10) and non-manifold (0x20) flags, and the fixed-point pseudonormal sum of that feature
// (nullptr for an edge the table does not hold).
__device__ __forceinline__ uint32_t msdf_feature(const Ws& W, const Best& best, int32_t vi0, int32_t vi1, int32_t vi2,
                                                 const long long*& acc) {
  uint32_t feature;
  acc = nullptr;
  if (best.code >= 4) {
    const int32_t v = best.code == 4 ? vi0 : (best.code == 5 ? vi1 : vi2);
    acc = &W.vacc[(int64_t)v * 3];
    feature = 2u | W.vflag[v];
  } else {
    const unsigned long long key = best.code == 1 ? edge_key(vi0, vi1)
                                   : (best.code == 2 ? edge_key(vi1, vi2) : edge_key(vi2, vi0));
    uint32_t s = edge_slot0(key, W.ecap);
    feature = 1u;
    for (uint32_t probe = 0; probe < W.ecap; ++probe) {
      const unsigned long long have = W.ekey[s];
      if (have == key) {
        acc = &W.eacc[(int64_t)s * 3];
        const uint32_t cnt = W.ecnt[s];
        feature |= cnt == 1 ? 0x10u : (cnt > 2 ? 0x20u : 0u);
        break;
      }
      if (have == kNoEdge) break;
      s = (s + 1) & (W.ecap - 1);
    }
  }
  return feature;
}

}  // namespace
}  // namespace bnv
