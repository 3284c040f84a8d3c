// The mesh index csrc/meshsdf.hip builds and both it and csrc/meshray.hip read: the header word layout, the carving of
// the caller's workspace (msdf_layout).  One definition, so the builder and every reader agree on it; which cell a
// coordinate falls into is csrc/cell_grid.hpp's rule.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "cell_grid.hpp"
#include "workspace.hpp"

namespace bnv {
namespace {

constexpr int kLevels = 24;               // candidate cell sizes h0 * kLadder^l; the last one is a single cell
constexpr double kLadder = 1.5;
constexpr double kCellTarget = 2.0;       // h0 = sqrt(kCellTarget * S / n_faces), S = half the bounding box's surface
constexpr int64_t kCellsPerFace = 8;      // the grid has at most kCellsPerFace * n_faces + 64 cells
constexpr int64_t kPairsPerFace = 8;      // ... and at most kPairsPerFace * n_faces + 64 (triangle, cell) pairs
constexpr int kFineRings = 4;             // rings of the fine grid before a query moves on to the coarse grid
constexpr int kCoarseShift = 2;           // coarse cell = fine cell >> 2 on every axis
constexpr double kStopSlack = 1e-5;       // relative slack of the stop test on the distance
constexpr double kNormalScale = 1099511627776.0;   // 2^40: fixed point of the pseudonormal sums
constexpr unsigned long long kNoEdge = ~0ull;
constexpr uint32_t kMagic = 0x4653444du;
constexpr int64_t kMaxFaces = 1 << 27, kMaxVertices = INT32_MAX;

struct Level {
  double h, inv_h;
  int32_t dims[3];
  int32_t pad;
};

struct Header {
  uint32_t bmin[3], bmax[3];   // order-preserving encodings of the finite vertices' bounding box (first: memset)
  unsigned long long tests;    // byte 24: triangle tests of all queries since the build (BNV_MESHSDF_COUNT_TESTS builds
                               // only; tools/mesh_sdf_bench.py reads it)
  uint32_t magic, pad0;
  int64_t n_vertices, n_faces, bytes;
  double lo[3], fmin[3], fmax[3];
  Level level[kLevels];
  unsigned long long pairs[kLevels];   // (triangle, cell) pairs the grid of every level would hold
  int32_t chosen, pad1;
  int32_t n_cells[2];                  // fine, coarse; 0: no valid triangle
  int32_t dims[2][3];
  double h, inv_h;                     // the fine grid's
  double eps_abs;                      // absolute slack of the stop test: 8 ulp of the largest coordinate
};
static_assert(offsetof(Header, bmin) == 0 && offsetof(Header, bmax) == 12, "grid_bbox writes the first six words");
static_assert(offsetof(Header, tests) == 24, "tools/mesh_sdf_bench.py reads the counter at byte 24");

struct Ws {
  Header* H;
  float4* tri;                 // [3 F]: (vertex k, bitcast(vertex index)); index -1: a skipped face
  long long* vacc;             // [3 V] angle-weighted normal sums, fixed point
  uint32_t* vflag;             // [V] 0x10 boundary, 0x20 non-manifold
  unsigned long long* ekey;    // [ecap] (lo vertex << 32) | hi vertex, kNoEdge: empty
  long long* eacc;             // [3 ecap] sums of the incident unit face normals, fixed point
  uint32_t* ecnt;              // [ecap] incident faces
  uint32_t* count[2];          // [cellcap + 2]
  uint32_t* start[2];          // [cellcap + 2]
  uint32_t* ids[2];            // [paircap]
  uint64_t* scan_state;        // [2 tiles]
  uint32_t ecap;
  int64_t cellcap, paircap, tiles;
};

__host__ __device__ inline size_t msdf_layout(int64_t nv, int64_t nf, char* base, Ws* w) {
  uint32_t ecap = 64;
  while ((int64_t)ecap < 4 * nf) ecap <<= 1;
  const int64_t cellcap = kCellsPerFace * nf + 64, paircap = kPairsPerFace * nf + 64;
  const int64_t n_bins = cellcap + 2, tiles = (n_bins + kScanTile - 1) / kScanTile;
  Carver c(base);
  Ws t;
  t.H = c.take<Header>(1);
  t.tri = c.take<float4>(3 * nf);
  t.vacc = c.take<long long>(3 * nv);
  t.vflag = c.take<uint32_t>(nv);
  t.ekey = c.take<unsigned long long>(ecap);
  t.eacc = c.take<long long>(3 * (size_t)ecap);
  t.ecnt = c.take<uint32_t>(ecap);
  t.count[0] = c.take<uint32_t>(n_bins);
  t.start[0] = c.take<uint32_t>(n_bins);
  t.count[1] = c.take<uint32_t>(n_bins);
  t.start[1] = c.take<uint32_t>(n_bins);
  t.ids[0] = c.take<uint32_t>(paircap);
  t.ids[1] = c.take<uint32_t>(paircap);
  t.scan_state = c.take<uint64_t>(tiles * 2);
  t.ecap = ecap;
  t.cellcap = cellcap;
  t.paircap = paircap;
  t.tiles = tiles;
  if (w) *w = t;
  return c.bytes();
}

}  // namespace
}  // namespace bnv
