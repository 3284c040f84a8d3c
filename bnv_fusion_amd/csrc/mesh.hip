// Per-voxel marching cubes on the decoded 3x3x3 SDF lattices.
//
// Reference: SparseVolume.meshlize, src/models/sparse_volume.py:697-766 -- for every active voxel whose
// lattice straddles the level (:742) skimage.measure.marching_cubes(sdf[3,3,3], level, spacing=0.5), then
// verts += origin - 0.5 (:749), * voxel_size + min_coords (:756); all voxels' meshes are concatenated.
// Here: two passes over the voxels (count triangles, then emit at the prefix-summed offsets), one thread per
// voxel walking its 8 cells; the output is a triangle soup in voxel / cell / table order, so it is
// reproducible.  The 256-case table is generated on the host (bnv_fusion_amd/mc_tables.py); scikit-image is
// not available, so the triangulation inside ambiguous cells is this table's, not Lewiner's (vertex
// positions -- the level crossings of the lattice edges -- are the same for every marching-cubes variant).
//
// HBM-bound: 108 B read per voxel (twice), 36 B written per triangle.
//
// Below the lattice mesher: dense marching cubes over the TSDF side volume (k_tm_*, TSDFVolume.get_mesh).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bnv_fusion.h"
#include "bnv_common.hpp"
#include "scan.hpp"
#include "workspace.hpp"

namespace bnv {

// cube edges as corner pairs; corner c = 4 dx + 2 dy + dz (the lattice's flatten order), as mc_tables.EDGES
__device__ const int8_t kMcEdgeA[12] = {0, 0, 0, 1, 1, 2, 2, 3, 4, 4, 5, 6};
__device__ const int8_t kMcEdgeB[12] = {1, 2, 4, 3, 5, 3, 6, 7, 5, 6, 7, 7};
constexpr int kMcRow = 16;  // table row: up to 5 triangles (15 edge ids) + terminator

__device__ __forceinline__ bool mc_gate(const float (&s)[27], float level) {
  float mx = s[0], mn = s[0];
#pragma unroll
  for (int i = 1; i < 27; ++i) {
    mx = fmaxf(mx, s[i]);
    mn = fminf(mn, s[i]);
  }
  return mx > level && mn < level;  // sparse_volume.py:742
}

__device__ __forceinline__ int mc_case(const float (&s)[27], int cx, int cy, int cz, float level) {
  int c = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float v = s[(cx + ((k >> 2) & 1)) * 9 + (cy + ((k >> 1) & 1)) * 3 + (cz + (k & 1))];
    c |= (v < level) << k;
  }
  return c;
}

__global__ __launch_bounds__(256) void k_mc_count(const float* __restrict__ sdf, int64_t n,
                                                  const int32_t* __restrict__ n_dev, float level,
                                                  const int8_t* __restrict__ table, int32_t* __restrict__ counts) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  if (n_dev && v >= *n_dev) {
    counts[v] = 0;
    return;
  }
  float s[27];
#pragma unroll
  for (int i = 0; i < 27; ++i) s[i] = sdf[v * 27 + i];
  int t = 0;
  if (mc_gate(s, level)) {
    for (int cell = 0; cell < 8; ++cell) {
      const int8_t* row = table + mc_case(s, cell >> 2, (cell >> 1) & 1, cell & 1, level) * kMcRow;
      for (int k = 0; k < kMcRow - 1 && row[k] >= 0; k += 3) ++t;
    }
  }
  counts[v] = t;
}

__global__ __launch_bounds__(256) void k_mc_emit(const float* __restrict__ sdf, const int64_t* __restrict__ origins,
                                                 int64_t n, const int32_t* __restrict__ n_dev, float level,
                                                 float voxel, float mx, float my, float mz,
                                                 const int8_t* __restrict__ table,
                                                 const int64_t* __restrict__ tri_offsets,
                                                 float* __restrict__ vertices) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n || (n_dev && v >= *n_dev)) return;
  float s[27];
#pragma unroll
  for (int i = 0; i < 27; ++i) s[i] = sdf[v * 27 + i];
  if (!mc_gate(s, level)) return;
  const float org[3] = {(float)origins[v * 3] - 0.5f, (float)origins[v * 3 + 1] - 0.5f, (float)origins[v * 3 + 2] - 0.5f};
  const float mn[3] = {mx, my, mz};
  float* out = vertices + tri_offsets[v] * 9;
  for (int cell = 0; cell < 8; ++cell) {
    const int cc[3] = {cell >> 2, (cell >> 1) & 1, cell & 1};
    const int8_t* row = table + mc_case(s, cc[0], cc[1], cc[2], level) * kMcRow;
    for (int k = 0; k < kMcRow - 1 && row[k] >= 0; ++k) {
      const int a = kMcEdgeA[row[k]], b = kMcEdgeB[row[k]];
      const int pa[3] = {cc[0] + ((a >> 2) & 1), cc[1] + ((a >> 1) & 1), cc[2] + (a & 1)};
      const int pb[3] = {cc[0] + ((b >> 2) & 1), cc[1] + ((b >> 1) & 1), cc[2] + (b & 1)};
      const float va = s[pa[0] * 9 + pa[1] * 3 + pa[2]], vb = s[pb[0] * 9 + pb[1] * 3 + pb[2]];
      const float t = __fdiv_rn(__fsub_rn(level, va), __fsub_rn(vb, va));
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        float p = __fadd_rn((float)pa[d], __fmul_rn(t, (float)(pb[d] - pa[d])));  // lattice index units
        p = __fmul_rn(p, 0.5f);                                                    // spacing (:719)
        p = __fadd_rn(p, org[d]);                                                  // :749
        out[d] = __fadd_rn(__fmul_rn(p, voxel), mn[d]);                            // :756
      }
      out += 3;
    }
  }
}

// ---- indexed output: per voxel a vertex list WITHOUT duplicates + faces indexing it, concatenated over the voxels
// the way SparseVolume.meshlize does (sparse_volume.py:740-756: faces + last_face_id; last_face_id += max(faces) + 1
// = the voxel's vertex count, every vertex being used).  A vertex of a voxel's mesh lies on one of the 54 edges of its
// 3x3x3 lattice, so a 54-bit mask of the sign-changing lattice edges names the voxel's vertices; they are emitted in
// ascending edge order and a triangle corner's local index is the rank of its edge's bit.
__device__ __forceinline__ int mc_lattice_edge(const int (&pa)[3], int axis) {
  // edge from node pa to pa + e_axis; 18 edges per axis
  if (axis == 0) return pa[0] * 9 + pa[1] * 3 + pa[2];
  if (axis == 1) return 18 + pa[0] * 6 + pa[1] * 3 + pa[2];
  return 36 + pa[0] * 6 + pa[1] * 2 + pa[2];
}

__device__ __forceinline__ unsigned long long mc_edge_mask(const float (&s)[27], float level) {
  unsigned long long m = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const bool in0 = s[i * 9 + j * 3 + k] < level;
        const int pa[3] = {i, j, k};
        if (i < 2 && in0 != (s[(i + 1) * 9 + j * 3 + k] < level)) m |= 1ull << mc_lattice_edge(pa, 0);
        if (j < 2 && in0 != (s[i * 9 + (j + 1) * 3 + k] < level)) m |= 1ull << mc_lattice_edge(pa, 1);
        if (k < 2 && in0 != (s[i * 9 + j * 3 + k + 1] < level)) m |= 1ull << mc_lattice_edge(pa, 2);
      }
  return m;
}

__global__ __launch_bounds__(256) void k_mc_count_indexed(const float* __restrict__ sdf, int64_t n,
                                                          const int32_t* __restrict__ n_dev, float level,
                                                          const int8_t* __restrict__ table,
                                                          int32_t* __restrict__ n_verts, int32_t* __restrict__ n_tris) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  int nv = 0, nt = 0;
  if (!(n_dev && v >= *n_dev)) {
    float s[27];
#pragma unroll
    for (int i = 0; i < 27; ++i) s[i] = sdf[v * 27 + i];
    if (mc_gate(s, level)) {
      nv = (int)__popcll(mc_edge_mask(s, level));
      for (int cell = 0; cell < 8; ++cell) {
        const int8_t* row = table + mc_case(s, cell >> 2, (cell >> 1) & 1, cell & 1, level) * kMcRow;
        for (int k = 0; k < kMcRow - 1 && row[k] >= 0; k += 3) ++nt;
      }
    }
  }
  n_verts[v] = nv;
  n_tris[v] = nt;
}

__global__ __launch_bounds__(256) void k_mc_emit_indexed(const float* __restrict__ sdf,
                                                         const int64_t* __restrict__ origins, int64_t n,
                                                         const int32_t* __restrict__ n_dev, float level, float voxel,
                                                         float mx, float my, float mz, const int8_t* __restrict__ table,
                                                         const int64_t* __restrict__ vert_offsets,
                                                         const int64_t* __restrict__ tri_offsets,
                                                         float* __restrict__ vertices, int64_t* __restrict__ faces) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n || (n_dev && v >= *n_dev)) return;
  float s[27];
#pragma unroll
  for (int i = 0; i < 27; ++i) s[i] = sdf[v * 27 + i];
  if (!mc_gate(s, level)) return;
  const unsigned long long mask = mc_edge_mask(s, level);
  const float org[3] = {(float)origins[v * 3] - 0.5f, (float)origins[v * 3 + 1] - 0.5f, (float)origins[v * 3 + 2] - 0.5f};
  const float mn[3] = {mx, my, mz};
  // vertices, ascending lattice-edge order
  float* vo = vertices + vert_offsets[v] * 3;
  for (int axis = 0; axis < 3; ++axis) {
    const int ni = axis == 0 ? 2 : 3, nj = axis == 1 ? 2 : 3, nk = axis == 2 ? 2 : 3;
    for (int i = 0; i < ni; ++i)
      for (int j = 0; j < nj; ++j)
        for (int k = 0; k < nk; ++k) {
          const int pa[3] = {i, j, k};
          if (!((mask >> mc_lattice_edge(pa, axis)) & 1ull)) continue;
          const int pb[3] = {i + (axis == 0), j + (axis == 1), k + (axis == 2)};
          const float va = s[pa[0] * 9 + pa[1] * 3 + pa[2]], vb = s[pb[0] * 9 + pb[1] * 3 + pb[2]];
          const float t = __fdiv_rn(__fsub_rn(level, va), __fsub_rn(vb, va));
#pragma unroll
          for (int d = 0; d < 3; ++d) {
            float p = __fadd_rn((float)pa[d], __fmul_rn(t, (float)(pb[d] - pa[d])));  // lattice index units
            p = __fmul_rn(p, 0.5f);                                                    // spacing (:719)
            p = __fadd_rn(p, org[d]);                                                  // :749
            vo[d] = __fadd_rn(__fmul_rn(p, voxel), mn[d]);                             // :756
          }
          vo += 3;
        }
  }
  // faces: cell / table order, global indices = the voxel's vertex offset + rank of the corner's lattice edge
  int64_t* fo = faces + tri_offsets[v] * 3;
  const int64_t base = vert_offsets[v];
  for (int cell = 0; cell < 8; ++cell) {
    const int cc[3] = {cell >> 2, (cell >> 1) & 1, cell & 1};
    const int8_t* row = table + mc_case(s, cc[0], cc[1], cc[2], level) * kMcRow;
    for (int k = 0; k < kMcRow - 1 && row[k] >= 0; ++k) {
      const int a = kMcEdgeA[row[k]], b = kMcEdgeB[row[k]];   // a < b, they differ in one bit
      const int pa[3] = {cc[0] + ((a >> 2) & 1), cc[1] + ((a >> 1) & 1), cc[2] + (a & 1)};
      const int axis = (a ^ b) == 4 ? 0 : ((a ^ b) == 2 ? 1 : 2);
      const int id = mc_lattice_edge(pa, axis);
      *fo++ = base + (int64_t)__popcll(mask & ((1ull << id) - 1ull));
    }
  }
}


// ---- dense marching cubes over a TSDF grid: TSDFVolume.get_mesh / get_point_cloud (third_parties/fusion.py:302-341).
// The reference runs skimage's marching_cubes_lewiner on the host copy of the [X, Y, Z] volume.  Here the volume is
// read in place on the device and meshed into a WELDED indexed mesh: one vertex per grid edge whose end values
// straddle the level, shared by the cells around it.  Conventions (shared with mc_tables.py and k_mc_* above):
//   cell based at grid point (i, j, k); corner c = 4 dx + 2 dy + dz at (i + dx, j + dy, k + dz); case bit c set when
//   tsdf < level; TRI_TABLE / EDGES / winding of mc_tables.py (face normals point toward increasing TSDF; the
//   triangulation inside ambiguous cells is that table's, not Lewiner's -- the vertex set is the same for both).
//   vertex on the edge a -> b = a + e_axis: t = (level - va) / (vb - va), index-space position a + t on that axis,
//   world = fl32(fl32(p * voxel) + origin) (fusion.py:330 in fp32).
//   normal: np.gradient of the volume at a and b (central (v[i+1] - v[i-1]) * 0.5 inside, one-sided at the border),
//   interpolated with the same t and normalised (a zero gradient gives a zero normal).
//   colour: color[rint(p)] (np.round, half to even) unfolded in fp32 as fusion.py:331-337.
//   order: vertices by the linear index of the owning (lower) grid point, then axis x, y, z; faces by the linear index
//   of the cell's base point, then table order.  observed_only: a cell emits only when its 8 corners have weight > 0,
//   a vertex exists only when an emitting cell uses it.
// Layout: tiles of 64 consecutive grid points (linear index), one wave each.  Pass 1 (k_tm_count) ballots three 64-bit
// "this point owns a vertex on its x / y / z edge" masks per tile and counts the tile's triangles; three small
// kernels scan the per-tile counts into offsets; pass 2 (k_tm_emit) writes vertices at the tile offset + the popcount
// of the tile's masks below the lane, and resolves every triangle corner the same way from its owner's tile -- no
// per-voxel id map.  Workspace: 40 B per tile (0.625 B per grid point) + 16 B per 1024 tiles.
constexpr int kTmWaves = 4;              // tiles (waves) per 256-thread block
constexpr int kTmScan = 1024;            // tiles per scan block

struct TmGrid {
  const float* tsdf;
  const float* weight;                   // read only when observed_only
  int64_t X, Y, Z, YZ, N;
  float level;
  int observed_only;
};

struct TmLayout {
  int64_t tiles, blocks;
  unsigned long long* masks;     // [tiles, 3]
  int64_t *voff, *toff, *bsum;   // [tiles], [tiles], [blocks, 2]
  size_t bytes;
};

static TmLayout tm_layout(int64_t n, const void* base) {
  Carver c(base);
  TmLayout L;
  L.tiles = (n + 63) / 64;
  L.blocks = (L.tiles + kTmScan - 1) / kTmScan;
  L.masks = c.take<unsigned long long>(L.tiles * 3);
  L.voff = c.take<int64_t>(L.tiles);
  L.toff = c.take<int64_t>(L.tiles);
  L.bsum = c.take<int64_t>(L.blocks * 2);
  L.bytes = c.bytes();
  return L;
}

__device__ __forceinline__ void tm_coords(const TmGrid& g, int64_t p, int64_t& i, int64_t& j, int64_t& k) {
  if (g.N <= (int64_t)0xffffffffu) {     // 32-bit division when the volume allows it
    const uint32_t q = (uint32_t)p, z = (uint32_t)g.Z, y = (uint32_t)g.Y;
    const uint32_t ij = q / z;
    k = q - ij * z;
    j = ij % y;
    i = ij / y;
  } else {
    const int64_t ij = p / g.Z;
    k = p - ij * g.Z;
    j = ij % g.Y;
    i = ij / g.Y;
  }
}

__device__ __forceinline__ int64_t tm_corner(const TmGrid& g, int64_t p, int c) {
  return p + ((c >> 2) & 1) * g.YZ + ((c >> 1) & 1) * g.Z + (c & 1);
}

// the cell based at (i, j, k) exists and, with observed_only, has all 8 corners observed
__device__ __forceinline__ bool tm_cell_on(const TmGrid& g, int64_t i, int64_t j, int64_t k) {
  if (i < 0 || j < 0 || k < 0 || i >= g.X - 1 || j >= g.Y - 1 || k >= g.Z - 1) return false;
  if (!g.observed_only) return true;
  const int64_t p = (i * g.Y + j) * g.Z + k;
  for (int c = 0; c < 8; ++c)
    if (!(g.weight[tm_corner(g, p, c)] > 0.f)) return false;
  return true;
}

__device__ __forceinline__ int tm_case(const TmGrid& g, int64_t p) {
  int cs = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) cs |= (g.tsdf[tm_corner(g, p, c)] < g.level) << c;
  return cs;
}

__device__ __forceinline__ int tm_ntri(const int8_t* __restrict__ table, int cs) {
  const int8_t* row = table + cs * kMcRow;
  int k = 0;
  while (k < kMcRow - 1 && row[k] >= 0) k += 3;
  return k / 3;
}

// does grid point (i, j, k) own a vertex on its edge along `axis`: the edge straddles the level and one of the (up to
// four) cells around it emits
__device__ __forceinline__ bool tm_owns(const TmGrid& g, int64_t p, int64_t i, int64_t j, int64_t k, bool in0,
                                        int axis) {
  const int64_t c[3] = {i, j, k};
  const int64_t n[3] = {g.X, g.Y, g.Z};
  if (c[axis] + 1 >= n[axis]) return false;
  const int64_t step = axis == 0 ? g.YZ : (axis == 1 ? g.Z : 1);
  if (in0 == (g.tsdf[p + step] < g.level)) return false;
  const int u = axis == 0 ? 1 : 0, v = axis == 2 ? 1 : 2;   // the two other axes
  for (int du = 0; du < 2; ++du)
    for (int dv = 0; dv < 2; ++dv) {
      int64_t b[3] = {i, j, k};
      b[u] -= du;
      b[v] -= dv;
      if (tm_cell_on(g, b[0], b[1], b[2])) return true;
    }
  return false;
}

__global__ __launch_bounds__(256) void k_tm_count(TmGrid g, const int8_t* __restrict__ table, int64_t tiles,
                                                  unsigned long long* __restrict__ masks,
                                                  int64_t* __restrict__ n_verts, int64_t* __restrict__ n_tris) {
  const int64_t tile = (int64_t)blockIdx.x * kTmWaves + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (tile >= tiles) return;             // uniform over the wave
  const int64_t p = tile * 64 + lane;
  bool ex = false, ey = false, ez = false;
  int nt = 0;
  if (p < g.N) {
    int64_t i, j, k;
    tm_coords(g, p, i, j, k);
    const bool in0 = g.tsdf[p] < g.level;
    ex = tm_owns(g, p, i, j, k, in0, 0);
    ey = tm_owns(g, p, i, j, k, in0, 1);
    ez = tm_owns(g, p, i, j, k, in0, 2);
    if (tm_cell_on(g, i, j, k)) nt = tm_ntri(table, tm_case(g, p));
  }
  const unsigned long long mx = __ballot(ex), my = __ballot(ey), mz = __ballot(ez);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nt += __shfl_xor(nt, o);
  if (lane == 0) {
    masks[tile * 3 + 0] = mx;
    masks[tile * 3 + 1] = my;
    masks[tile * 3 + 2] = mz;
    n_verts[tile] = __popcll(mx) + __popcll(my) + __popcll(mz);
    n_tris[tile] = nt;
  }
}

__global__ __launch_bounds__(kTmScan) void k_tm_scan_reduce(const int64_t* __restrict__ n_verts,
                                                            const int64_t* __restrict__ n_tris, int64_t tiles,
                                                            int64_t* __restrict__ bsum) {
  __shared__ int64_t lds[kTmScan / 64];
  const int64_t t = (int64_t)blockIdx.x * kTmScan + threadIdx.x;
  int64_t sv, st;
  block_exclusive_scan<kTmScan>(t < tiles ? n_verts[t] : 0, lds, &sv);
  block_exclusive_scan<kTmScan>(t < tiles ? n_tris[t] : 0, lds, &st);
  if (threadIdx.x == 0) {
    bsum[blockIdx.x * 2] = sv;
    bsum[blockIdx.x * 2 + 1] = st;
  }
}

// one block: the block sums -> exclusive offsets in place; totals[0] = V, totals[1] = T
__global__ __launch_bounds__(kTmScan) void k_tm_scan_top(int64_t* __restrict__ bsum, int64_t blocks,
                                                         int64_t* __restrict__ totals) {
  __shared__ int64_t lds[kTmScan / 64];
  int64_t cv = 0, ct = 0;
  for (int64_t b0 = 0; b0 < blocks; b0 += kTmScan) {
    const int64_t b = b0 + threadIdx.x;
    const int64_t xv = b < blocks ? bsum[b * 2] : 0, xt = b < blocks ? bsum[b * 2 + 1] : 0;
    int64_t sv, st;
    const int64_t ev = block_exclusive_scan<kTmScan>(xv, lds, &sv), et = block_exclusive_scan<kTmScan>(xt, lds, &st);
    if (b < blocks) {
      bsum[b * 2] = cv + ev;
      bsum[b * 2 + 1] = ct + et;
    }
    cv += sv;
    ct += st;
  }
  if (threadIdx.x == 0) {
    totals[0] = cv;
    totals[1] = ct;
  }
}

__global__ __launch_bounds__(kTmScan) void k_tm_scan_apply(int64_t* __restrict__ n_verts, int64_t* __restrict__ n_tris,
                                                           int64_t tiles, const int64_t* __restrict__ bsum) {
  __shared__ int64_t lds[kTmScan / 64];
  const int64_t t = (int64_t)blockIdx.x * kTmScan + threadIdx.x;
  int64_t sv, st;
  const int64_t ev = block_exclusive_scan<kTmScan>(t < tiles ? n_verts[t] : 0, lds, &sv);
  const int64_t et = block_exclusive_scan<kTmScan>(t < tiles ? n_tris[t] : 0, lds, &st);
  if (t < tiles) {
    n_verts[t] = bsum[blockIdx.x * 2] + ev;
    n_tris[t] = bsum[blockIdx.x * 2 + 1] + et;
  }
}

// global id of the vertex grid point q owns on its `axis` edge
__device__ __forceinline__ int64_t tm_vertex_id(const unsigned long long* __restrict__ masks,
                                                const int64_t* __restrict__ voff, int64_t q, int axis) {
  const int64_t t = q >> 6;
  const int l = (int)(q & 63);
  const unsigned long long below = (1ull << l) - 1ull;
  const unsigned long long mx = masks[t * 3], my = masks[t * 3 + 1], mz = masks[t * 3 + 2];
  int64_t id = voff[t] + __popcll(mx & below) + __popcll(my & below) + __popcll(mz & below);
  if (axis >= 1) id += (mx >> l) & 1ull;
  if (axis >= 2) id += (my >> l) & 1ull;
  return id;
}

// np.gradient of the volume at grid point (i, j, k), p its linear index (every dimension >= 2)
__device__ __forceinline__ void tm_grad(const TmGrid& g, int64_t p, int64_t i, int64_t j, int64_t k, float (&out)[3]) {
  const int64_t c[3] = {i, j, k}, n[3] = {g.X, g.Y, g.Z}, step[3] = {g.YZ, g.Z, 1};
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    if (c[d] == 0)
      out[d] = __fsub_rn(g.tsdf[p + step[d]], g.tsdf[p]);
    else if (c[d] == n[d] - 1)
      out[d] = __fsub_rn(g.tsdf[p], g.tsdf[p - step[d]]);
    else
      out[d] = __fmul_rn(__fsub_rn(g.tsdf[p + step[d]], g.tsdf[p - step[d]]), 0.5f);
  }
}

__global__ __launch_bounds__(256) void k_tm_emit(TmGrid g, const float* __restrict__ color,
                                                 const int8_t* __restrict__ table, int64_t tiles,
                                                 const unsigned long long* __restrict__ masks,
                                                 const int64_t* __restrict__ voff, const int64_t* __restrict__ toff,
                                                 float ox, float oy, float oz, float voxel, int64_t v_cap,
                                                 int64_t t_cap, float* __restrict__ vertices,
                                                 int64_t* __restrict__ faces, float* __restrict__ normals,
                                                 uint8_t* __restrict__ colors) {
  const int64_t tile = (int64_t)blockIdx.x * kTmWaves + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (tile >= tiles) return;             // uniform over the wave
  const int64_t p = tile * 64 + lane;
  const bool live = p < g.N;
  int64_t i = 0, j = 0, k = 0;
  if (live) tm_coords(g, p, i, j, k);
  if (faces) {
    // triangles of the cell based here, at the tile's offset + the triangles of the lanes below
    int cs = 0, nt = 0;
    if (live && tm_cell_on(g, i, j, k)) {
      cs = tm_case(g, p);
      nt = tm_ntri(table, cs);
    }
    const int64_t first = toff[tile] + wave_inclusive_scan<int64_t>(nt) - nt;
    if (nt && first + nt <= t_cap) {
      const int8_t* row = table + cs * kMcRow;
      int64_t* fo = faces + first * 3;
      for (int e = 0; e < 3 * nt; ++e) {
        const int a = kMcEdgeA[row[e]], b = kMcEdgeB[row[e]];   // a < b, they differ in one bit
        const int axis = (a ^ b) == 4 ? 0 : ((a ^ b) == 2 ? 1 : 2);
        fo[e] = tm_vertex_id(masks, voff, tm_corner(g, p, a), axis);
      }
    }
  }
  if (!live) return;
  const unsigned long long m[3] = {masks[tile * 3], masks[tile * 3 + 1], masks[tile * 3 + 2]};
  const unsigned long long below = (1ull << lane) - 1ull;
  int64_t id = voff[tile] + __popcll(m[0] & below) + __popcll(m[1] & below) + __popcll(m[2] & below);
  const float org[3] = {ox, oy, oz};
  for (int axis = 0; axis < 3; ++axis) {
    if (!((m[axis] >> lane) & 1ull)) continue;
    if (id >= v_cap) return;
    const int64_t step = axis == 0 ? g.YZ : (axis == 1 ? g.Z : 1);
    const float va = g.tsdf[p], vb = g.tsdf[p + step];
    const float t = __fdiv_rn(__fsub_rn(g.level, va), __fsub_rn(vb, va));
    float pi[3] = {(float)i, (float)j, (float)k};
    pi[axis] = __fadd_rn(pi[axis], t);
#pragma unroll
    for (int d = 0; d < 3; ++d) vertices[id * 3 + d] = __fadd_rn(__fmul_rn(pi[d], voxel), org[d]);
    if (normals) {
      float ga[3], gb[3], n[3];
      tm_grad(g, p, i, j, k, ga);
      tm_grad(g, p + step, i + (axis == 0), j + (axis == 1), k + (axis == 2), gb);
#pragma unroll
      for (int d = 0; d < 3; ++d) n[d] = __fadd_rn(ga[d], __fmul_rn(t, __fsub_rn(gb[d], ga[d])));
      const float len = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(n[0], n[0]), __fmul_rn(n[1], n[1])),
                                             __fmul_rn(n[2], n[2])));
#pragma unroll
      for (int d = 0; d < 3; ++d) normals[id * 3 + d] = len > 0.f ? __fdiv_rn(n[d], len) : 0.f;
    }
    if (colors) {
      float rgb = 0.f;
      if (color) {
        // clamped: a NaN or infinite TSDF value must not send the read outside the volume
        const int64_t ri = (int64_t)fminf(fmaxf(rintf(pi[0]), 0.f), (float)(g.X - 1));
        const int64_t rj = (int64_t)fminf(fmaxf(rintf(pi[1]), 0.f), (float)(g.Y - 1));
        const int64_t rk = (int64_t)fminf(fmaxf(rintf(pi[2]), 0.f), (float)(g.Z - 1));
        rgb = color[(ri * g.Y + rj) * g.Z + rk];
      }
      const float cb = floorf(__fdiv_rn(rgb, 65536.f));                                      // fusion.py:333-336
      const float rest = __fsub_rn(rgb, __fmul_rn(cb, 65536.f));
      const float cg = floorf(__fdiv_rn(rest, 256.f));
      const float cr = floorf(__fsub_rn(rest, __fmul_rn(cg, 256.f)));
      colors[id * 3 + 0] = (uint8_t)(int)cr;
      colors[id * 3 + 1] = (uint8_t)(int)cg;
      colors[id * 3 + 2] = (uint8_t)(int)cb;
    }
    ++id;
  }
}

}  // namespace bnv

using namespace bnv;

extern "C" {

int bnv_mc_count(const float* sdf, int64_t n, const int32_t* n_dev, float level, const int8_t* tri_table,
                 int32_t* counts, bnv_stream_t stream) {
  if (n < 0 || (n > 0 && (!sdf || !tri_table || !counts))) return BNV_ERR_INVALID_ARGUMENT;
  if (n == 0) return BNV_OK;
  hipLaunchKernelGGL(k_mc_count, dim3(blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, sdf, n, n_dev,
                     level, tri_table, counts);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

int bnv_mc_emit(const float* sdf, const int64_t* origins, int64_t n, const int32_t* n_dev, float level,
                float voxel_size, const float min_coords[3], const int8_t* tri_table, const int64_t* tri_offsets,
                float* vertices, bnv_stream_t stream) {
  if (n < 0 || (n > 0 && (!sdf || !origins || !min_coords || !tri_table || !tri_offsets || !vertices)))
    return BNV_ERR_INVALID_ARGUMENT;
  if (n == 0) return BNV_OK;
  hipLaunchKernelGGL(k_mc_emit, dim3(blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, sdf, origins, n,
                     n_dev, level, voxel_size, min_coords[0], min_coords[1], min_coords[2], tri_table, tri_offsets,
                     vertices);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

int bnv_mc_count_indexed(const float* sdf, int64_t n, const int32_t* n_dev, float level, const int8_t* tri_table,
                         int32_t* n_verts, int32_t* n_tris, bnv_stream_t stream) {
  if (n < 0 || (n > 0 && (!sdf || !tri_table || !n_verts || !n_tris))) return BNV_ERR_INVALID_ARGUMENT;
  if (n == 0) return BNV_OK;
  hipLaunchKernelGGL(k_mc_count_indexed, dim3(blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, sdf, n,
                     n_dev, level, tri_table, n_verts, n_tris);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

int bnv_mc_emit_indexed(const float* sdf, const int64_t* origins, int64_t n, const int32_t* n_dev, float level,
                        float voxel_size, const float min_coords[3], const int8_t* tri_table,
                        const int64_t* vert_offsets, const int64_t* tri_offsets, float* vertices, int64_t* faces,
                        bnv_stream_t stream) {
  if (n < 0 || (n > 0 && (!sdf || !origins || !min_coords || !tri_table || !vert_offsets || !tri_offsets || !vertices ||
                          !faces)))
    return BNV_ERR_INVALID_ARGUMENT;
  if (n == 0) return BNV_OK;
  hipLaunchKernelGGL(k_mc_emit_indexed, dim3(blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, sdf,
                     origins, n, n_dev, level, voxel_size, min_coords[0], min_coords[1], min_coords[2], tri_table,
                     vert_offsets, tri_offsets, vertices, faces);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}


static bool tm_dims(const int32_t* dim, int64_t& n) {
  if (!dim || dim[0] < 1 || dim[1] < 1 || dim[2] < 1) return false;
  n = (int64_t)dim[0] * dim[1] * dim[2];
  return true;
}

static TmGrid tm_grid(const float* tsdf, const float* weight, const int32_t* dim, float level, int observed_only) {
  TmGrid g;
  g.tsdf = tsdf;
  g.weight = weight;
  g.X = dim[0];
  g.Y = dim[1];
  g.Z = dim[2];
  g.YZ = g.Y * g.Z;
  g.N = g.X * g.YZ;
  g.level = level;
  g.observed_only = observed_only ? 1 : 0;
  return g;
}

int bnv_tsdf_mesh_workspace_bytes(const int32_t dim[3], int64_t* bytes) {
  int64_t n;
  if (!bytes || !tm_dims(dim, n)) return BNV_ERR_INVALID_ARGUMENT;
  *bytes = (int64_t)tm_layout(n, nullptr).bytes;
  return BNV_OK;
}

int bnv_tsdf_mesh_count(const float* tsdf, const float* weight, const int32_t dim[3], float level, int observed_only,
                        const int8_t* tri_table, void* workspace, int64_t ws_bytes, int64_t* totals,
                        bnv_stream_t stream) {
  int64_t n;
  if (!tsdf || !tm_dims(dim, n) || !tri_table || !workspace || !totals || (observed_only && !weight))
    return BNV_ERR_INVALID_ARGUMENT;
  const TmLayout L = tm_layout(n, workspace);
  if (ws_bytes < (int64_t)L.bytes) return BNV_ERR_WORKSPACE_TOO_SMALL;
  hipStream_t s = (hipStream_t)stream;
  if (dim[0] < 2 || dim[1] < 2 || dim[2] < 2) {   // no cell: an empty mesh
    BNV_HIP_CHECK(hipMemsetAsync(totals, 0, 2 * sizeof(int64_t), s));
    return BNV_OK;
  }
  const TmGrid g = tm_grid(tsdf, weight, dim, level, observed_only);
  hipLaunchKernelGGL(k_tm_count, dim3(blocks_for(L.tiles, kTmWaves)), dim3(256), 0, s, g, tri_table,
                     L.tiles, L.masks, L.voff, L.toff);
  BNV_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_tm_scan_reduce, dim3((unsigned)L.blocks), dim3(kTmScan), 0, s, L.voff, L.toff, L.tiles, L.bsum);
  BNV_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_tm_scan_top, dim3(1), dim3(kTmScan), 0, s, L.bsum, L.blocks, totals);
  BNV_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_tm_scan_apply, dim3((unsigned)L.blocks), dim3(kTmScan), 0, s, L.voff, L.toff, L.tiles, L.bsum);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

int bnv_tsdf_mesh_emit(const float* tsdf, const float* weight, const float* color, const int32_t dim[3],
                       const float origin[3], float voxel_size, float level, int observed_only,
                       const int8_t* tri_table, const void* workspace, int64_t ws_bytes, int64_t n_vertices,
                       int64_t n_faces, float* vertices, int64_t* faces, float* normals, uint8_t* colors,
                       bnv_stream_t stream) {
  int64_t n;
  if (!tsdf || !tm_dims(dim, n) || !origin || !tri_table || !workspace || !vertices || (observed_only && !weight) ||
      n_vertices < 0 || n_faces < 0)
    return BNV_ERR_INVALID_ARGUMENT;
  const TmLayout L = tm_layout(n, workspace);
  if (ws_bytes < (int64_t)L.bytes) return BNV_ERR_WORKSPACE_TOO_SMALL;
  if (dim[0] < 2 || dim[1] < 2 || dim[2] < 2 || n_vertices == 0) return BNV_OK;
  const TmGrid g = tm_grid(tsdf, weight, dim, level, observed_only);
  hipLaunchKernelGGL(k_tm_emit, dim3(blocks_for(L.tiles, kTmWaves)), dim3(256), 0,
                     (hipStream_t)stream, g, color, tri_table, L.tiles, (const unsigned long long*)L.masks,
                     (const int64_t*)L.voff, (const int64_t*)L.toff, origin[0], origin[1], origin[2],
                     voxel_size, n_vertices, n_faces, vertices, faces, normals, colors);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

}  // extern "C"
