// Mesh post-processing on the device: weld, cluster, clean and smooth -- mesh.post_process_mesh (the reference's
// o3d_helper.post_process_mesh, src/utils/o3d_helper.py:220-241) with the same output bit for bit.  The specification
// is in include/bnv_fusion.h ("Mesh post-processing").  Every result is reproducible from run to run: all arithmetic is
// float64 with one rounding per operation in a fixed order (no float atomics), the union-find's answer (the smallest
// member of every component) does not depend on the order unions arrive in, and the face dedupe keeps the smallest
// face index per key through an integer atomic-min.  Sorts and prefix sums are rocPRIM's device primitives.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "../../include/bnv_fusion.h"
#include "mesh_face.hpp"

namespace bnv {
namespace {

constexpr int kPostThreads = 256;
constexpr uint32_t kPadCluster = ~0u;
constexpr double kCellGrow = 1.0 + 1.0 / (1 << 20);   // cell edge = eps * kCellGrow: a pair at distance <= eps (the
constexpr double kCellLimit = 1073741824.0;           // fl64 test admits an ulp more) spans at most one cell per axis
                                                      // while |u| / cell < 2^30 (fl(u / cell) errs < 2^-23 there)

struct PostHdr {
  int32_t n_unique, n_clusters, n_vout, n_fout, error, pad[3];
};

struct PostWs {
  PostHdr* hdr;
  uint64_t* key[3];   // [V] sortable bits of u per axis
  uint64_t* ka;       // [V] gathered keys / cell hashes
  uint64_t* kb;       // [V] sorted keys / sorted cell hashes
  int32_t* pa;        // [V] permutation / sort values
  int32_t* pb;        // [V]
  int32_t* flag;      // [V] head flags, roots, used clusters
  int32_t* scan;      // [V] inclusive scans of flag
  int32_t* inv;       // [V] vertex -> unique point
  int32_t* parent;    // [V] union-find over unique points
  int32_t* cl;        // [V] unique point -> cluster
  uint32_t* ck;       // [V] cluster keys (pad: kPadCluster)
  uint32_t* cks;      // [V] sorted cluster keys
  int32_t* cstart;    // [V] first sorted position of every cluster; later: first edge of every output vertex
  double* U;          // [V, 3] unique points; later: the output vertices before smoothing
  double* mean;       // [V, 3] cluster means
  int32_t* canon;     // [T, 3] face corners as cluster labels, rotated (canon[3t] = -1: dropped)
  int32_t* slot_of;   // [T] hash slot of every kept face
  int32_t* keep;      // [T]
  int32_t* fscan;     // [T]
  int32_t* slots;     // [H] first face claiming a slot (-1 empty)
  uint32_t* minf;     // [H] smallest face index with the slot's key
  uint64_t* edges;    // [6T] directed edges (src << 32 | dst), pad kPadKey
  uint64_t* edges_s;  // [6T] sorted
  void* tmp;          // rocPRIM temporary storage
  size_t tmp_bytes;
  uint64_t H;
};

static size_t post_ws_layout(int64_t V, int64_t T, char* base, PostWs* w) {
  Carver c(base);
  PostWs l{};
  l.H = face_hash_slots(T);
  l.hdr = c.take<PostHdr>(1);
  for (int a = 0; a < 3; ++a) l.key[a] = c.take<uint64_t>(V);
  l.ka = c.take<uint64_t>(V);
  l.kb = c.take<uint64_t>(V);
  l.pa = c.take<int32_t>(V);
  l.pb = c.take<int32_t>(V);
  l.flag = c.take<int32_t>(V);
  l.scan = c.take<int32_t>(V);
  l.inv = c.take<int32_t>(V);
  l.parent = c.take<int32_t>(V);
  l.cl = c.take<int32_t>(V);
  l.ck = c.take<uint32_t>(V);
  l.cks = c.take<uint32_t>(V);
  l.cstart = c.take<int32_t>(V);
  l.U = c.take<double>(3 * V);
  l.mean = c.take<double>(3 * V);
  l.canon = c.take<int32_t>(3 * T);
  l.slot_of = c.take<int32_t>(T);
  l.keep = c.take<int32_t>(T);
  l.fscan = c.take<int32_t>(T);
  l.slots = c.take<int32_t>(l.H);
  l.minf = c.take<uint32_t>(l.H);
  l.edges = c.take<uint64_t>(6 * T);
  l.edges_s = c.take<uint64_t>(6 * T);
  l.tmp_bytes = std::max({prim_sort_bytes<uint64_t>(V), prim_sort_bytes<uint32_t>(V),
                          prim_sort_bytes<uint64_t>(6 * T, false), prim_scan_bytes(std::max(V, T))});
  l.tmp = c.take<char>(l.tmp_bytes);
  if (w) *w = l;
  return c.bytes();
}

// total order of doubles (no NaN) as unsigned integers; -0 was folded to +0 before
__device__ __forceinline__ uint64_t sortable(double u) {
  const uint64_t b = __builtin_bit_cast(uint64_t, u);
  return (b >> 63) ? ~b : (b | (1ull << 63));
}
__device__ __forceinline__ double unsortable(uint64_t k) {
  return __builtin_bit_cast(double, (k >> 63) ? (k & ~(1ull << 63)) : ~k);
}

__device__ __forceinline__ uint64_t cell_hash(int64_t x, int64_t y, int64_t z) {
  uint64_t h = (uint64_t)x * 0x9E3779B97F4A7C15ull;
  h ^= (uint64_t)y + 0xBF58476D1CE4E5B9ull + (h << 6) + (h >> 2);
  h ^= (uint64_t)z + 0x94D049BB133111EBull + (h << 6) + (h >> 2);
  h ^= h >> 31;
  h *= 0xD6E8FEB86659FD93ull;
  h ^= h >> 32;
  return h >> 1;   // never kPadKey
}

__device__ __forceinline__ int64_t cell_of(double u, double cell) {
  const double c = u / cell;
  return (int64_t)floor(fmin(fmax(c, -4.0 * kCellLimit), 4.0 * kCellLimit));
}

// ---- 1. exact weld: u = rint(x * 1e9) / 1e9 (np.round(x, 9)), unique rows in lexicographic order of u -------------
__global__ __launch_bounds__(kPostThreads) void k_pp_keys(const float* __restrict__ vin, int64_t V, double cell,
                                                          PostWs w) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V) return;
  int32_t err = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float x = vin[i * 3 + a];
    double u = 0.0;
    if (isfinite(x)) {
      u = __ddiv_rn(rint(__dmul_rn((double)x, 1e9)), 1e9);
      if (u == 0.0) u = 0.0;   // -0 and +0 are one row for np.unique
      if (cell > 0.0 && !(fabs(u) / cell < kCellLimit)) err |= kErrExtent;
    } else {
      err |= kErrNonFinite;
    }
    w.key[a][i] = sortable(u);
  }
  w.pa[i] = (int32_t)i;
  if (err) atomicOr(&w.hdr->error, err);
}

__global__ __launch_bounds__(kPostThreads) void k_pp_gather(const uint64_t* __restrict__ key,
                                                            const int32_t* __restrict__ perm, int64_t V,
                                                            uint64_t* __restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < V) out[k] = key[perm[k]];
}

__global__ __launch_bounds__(kPostThreads) void k_pp_heads(const int32_t* __restrict__ perm, int64_t V, PostWs w) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= V) return;
  int32_t head = 1;
  if (k > 0) {
    const int32_t p = perm[k], q = perm[k - 1];
    head = (w.key[0][p] != w.key[0][q]) | (w.key[1][p] != w.key[1][q]) | (w.key[2][p] != w.key[2][q]);
  }
  w.flag[k] = head;
}

__global__ __launch_bounds__(kPostThreads) void k_pp_unique(const int32_t* __restrict__ perm, int64_t V, PostWs w) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= V) return;
  const int32_t uid = w.scan[k] - 1, p = perm[k];
  w.inv[p] = uid;
  if (w.flag[k]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) w.U[(int64_t)uid * 3 + a] = unsortable(w.key[a][p]);
  }
  if (k == V - 1) w.hdr->n_unique = w.scan[k];
}

// ---- 2. clusters: connected components of (dx*dx + dy*dy) + dz*dz <= eps*eps over the unique points ---------------
__global__ __launch_bounds__(kPostThreads) void k_pp_cells(int64_t V, double cell, PostWs w) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V) return;
  const int64_t n = w.hdr->n_unique;
  w.parent[i] = (int32_t)i;
  w.pb[i] = (int32_t)i;
  if (cell > 0.0)
    w.ka[i] = i < n ? cell_hash(cell_of(w.U[i * 3], cell), cell_of(w.U[i * 3 + 1], cell),
                                cell_of(w.U[i * 3 + 2], cell))
                    : kPadKey;
}

// one thread per unique point i: the 27 cells around its own, every point j > i in them within eps joins i
__global__ __launch_bounds__(kPostThreads) void k_pp_union(int64_t V, double cell, double eps2, PostWs w) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = w.hdr->n_unique;
  if (i >= n) return;
  const double x = w.U[i * 3], y = w.U[i * 3 + 1], z = w.U[i * 3 + 2];
  const int64_t cx = cell_of(x, cell), cy = cell_of(y, cell), cz = cell_of(z, cell);
  for (int d = 0; d < 27; ++d) {
    const uint64_t h = cell_hash(cx + d % 3 - 1, cy + (d / 3) % 3 - 1, cz + d / 9 - 1);
    for (int64_t k = lower_bound_u64(w.kb, n, h); k < n && w.kb[k] == h; ++k) {
      const int32_t j = w.pa[k];
      if (j <= i) continue;
      const double dx = __dsub_rn(x, w.U[(int64_t)j * 3]), dy = __dsub_rn(y, w.U[(int64_t)j * 3 + 1]),
                   dz = __dsub_rn(z, w.U[(int64_t)j * 3 + 2]);
      const double d2 = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
      if (d2 <= eps2) uf_union<false>(w.parent, (int32_t)i, j);
    }
  }
}

__global__ __launch_bounds__(kPostThreads) void k_pp_roots(int64_t V, PostWs w) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V) return;
  const int64_t n = w.hdr->n_unique;
  int32_t is_root = 0;
  if (i < n) {
    const int32_t r = uf_find<false>(w.parent, (int32_t)i);
    w.cl[i] = r;   // the component's smallest member (turned into the cluster number below)
    is_root = r == (int32_t)i;
  }
  w.flag[i] = is_root;
}

// clusters numbered in ascending order of their smallest member (scipy's connected_components labels)
__global__ __launch_bounds__(kPostThreads) void k_pp_labels(int64_t V, PostWs w) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V) return;
  const int64_t n = w.hdr->n_unique;
  uint32_t c = kPadCluster;
  if (i < n) {
    c = (uint32_t)(w.scan[w.cl[i]] - 1);
    w.cl[i] = (int32_t)c;
  }
  w.ck[i] = c;
  w.pb[i] = (int32_t)i;
  w.cstart[i] = -1;
  if (i == 0) w.hdr->n_clusters = w.scan[V - 1];
}

// ---- 3. cluster means: members' u summed one after another in ascending index order, / count ----------------------
__global__ __launch_bounds__(kPostThreads) void k_pp_cstart(int64_t V, PostWs w) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= V || w.cks[k] == kPadCluster) return;
  if (k == 0 || w.cks[k] != w.cks[k - 1]) w.cstart[w.cks[k]] = (int32_t)k;
}

__global__ __launch_bounds__(kPostThreads) void k_pp_mean(int64_t V, PostWs w) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= w.hdr->n_clusters) return;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  int64_t cnt = 0;
  for (int64_t k = w.cstart[c]; k >= 0 && k < V && w.cks[k] == (uint32_t)c; ++k, ++cnt) {
    const int64_t m = w.pa[k];
    s0 = __dadd_rn(s0, w.U[m * 3]);
    s1 = __dadd_rn(s1, w.U[m * 3 + 1]);
    s2 = __dadd_rn(s2, w.U[m * 3 + 2]);
  }
  const double dc = (double)cnt;
  w.mean[c * 3] = __ddiv_rn(s0, dc);
  w.mean[c * 3 + 1] = __ddiv_rn(s1, dc);
  w.mean[c * 3 + 2] = __ddiv_rn(s2, dc);
}

// ---- 4. faces: the shared face step (mesh_face.hpp) over vertex -> unique point -> cluster ---------------------------
static FaceStep face_step(const PostWs& w) {
  return FaceStep{w.inv, w.cl, w.canon, w.slot_of, w.keep, w.fscan, w.slots, w.minf, w.flag, &w.hdr->error, w.H};
}

// ---- 5. referenced clusters only, in label order ------------------------------------------------------------------
__global__ __launch_bounds__(kPostThreads) void k_pp_vert_compact(int64_t V, int64_t T, PostWs w) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c == 0) {
    w.hdr->n_vout = w.scan[V - 1];
    w.hdr->n_fout = w.fscan[T - 1];
  }
  if (c >= w.hdr->n_clusters || !w.flag[c]) return;
  const int64_t o = w.scan[c] - 1;
  // U is free now: the output vertices before smoothing go there
#pragma unroll
  for (int a = 0; a < 3; ++a) w.U[o * 3 + a] = w.mean[c * 3 + a];
}

__global__ __launch_bounds__(kPostThreads) void k_pp_face_write(const int64_t* __restrict__ fin, int64_t T,
                                                                int64_t V, PostWs w, FaceStep fs,
                                                                int64_t* __restrict__ fout) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  uint64_t* e = w.edges + t * 6;
  int32_t c[3];
  if (!w.keep[t] || !face_clusters(fin, t, V, fs, c)) {
#pragma unroll
    for (int k = 0; k < 6; ++k) e[k] = kPadKey;
    return;
  }
  const int64_t o = w.fscan[t] - 1;
  uint64_t n[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    n[k] = (uint64_t)(w.scan[c[k]] - 1);   // original corner order
    fout[o * 3 + k] = (int64_t)n[k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const uint64_t a = n[k], b = n[(k + 1) % 3];
    e[2 * k] = a << 32 | b;
    e[2 * k + 1] = b << 32 | a;
  }
}

// ---- 6. one pass of simple Laplacian smoothing: (v + sum of distinct edge neighbours, ascending) / (1 + degree) ----
__global__ __launch_bounds__(kPostThreads) void k_pp_rows(int64_t E, PostWs w) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= E) return;
  const uint64_t e = w.edges_s[k];
  if (e == kPadKey) return;
  if (k == 0 || (w.edges_s[k - 1] >> 32) != (e >> 32)) w.cstart[e >> 32] = (int32_t)k;
}

__global__ __launch_bounds__(kPostThreads) void k_pp_smooth(int64_t E, PostWs w, float* __restrict__ vout) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= w.hdr->n_vout) return;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, deg = 0.0;
  const int64_t k0 = w.cstart[i];
  for (int64_t k = k0; k >= 0 && k < E && (w.edges_s[k] >> 32) == (uint64_t)i; ++k) {
    if (k > k0 && w.edges_s[k] == w.edges_s[k - 1]) continue;   // an edge two faces share counts once
    const int64_t j = (int64_t)(w.edges_s[k] & 0xffffffffull);
    s0 = __dadd_rn(s0, w.U[j * 3]);
    s1 = __dadd_rn(s1, w.U[j * 3 + 1]);
    s2 = __dadd_rn(s2, w.U[j * 3 + 2]);
    deg = __dadd_rn(deg, 1.0);
  }
  const double den = __dadd_rn(1.0, deg);
  vout[i * 3] = (float)__ddiv_rn(__dadd_rn(w.U[i * 3], s0), den);
  vout[i * 3 + 1] = (float)__ddiv_rn(__dadd_rn(w.U[i * 3 + 1], s1), den);
  vout[i * 3 + 2] = (float)__ddiv_rn(__dadd_rn(w.U[i * 3 + 2], s2), den);
}

__global__ void k_pp_counts(PostWs w, int64_t* counts) {
  const bool bad = w.hdr->error != 0;
  counts[0] = bad ? -1 : w.hdr->n_vout;
  counts[1] = bad ? -1 : w.hdr->n_fout;
}

// face-less input: the mesh as it is (the host function returns it unchanged); the finite check still applies
__global__ __launch_bounds__(kPostThreads) void k_pp_passthrough(const float* __restrict__ vin, int64_t V,
                                                                 float* __restrict__ vout, int32_t* __restrict__ err) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 3 * V) return;
  const float x = vin[i];
  vout[i] = x;
  if (!isfinite(x)) atomicOr(err, (int32_t)kErrNonFinite);
}

__global__ void k_pp_passthrough_counts(int64_t V, const int32_t* err, int64_t* counts) {
  counts[0] = *err ? -1 : V;
  counts[1] = *err ? -1 : 0;
}

}  // namespace
}  // namespace bnv

using namespace bnv;

extern "C" {

int bnv_mesh_post_workspace_bytes(int64_t n_vertices, int64_t n_faces, int64_t* bytes) {
  if (!bytes || !mesh_sizes_ok(n_vertices, n_faces)) return BNV_ERR_INVALID_ARGUMENT;
  *bytes = (int64_t)post_ws_layout(n_vertices, n_faces, nullptr, nullptr);
  return BNV_OK;
}

int bnv_mesh_post_process(const float* vertices, int64_t n_vertices, const int64_t* faces, int64_t n_faces,
                          double vertex_threshold, void* workspace, int64_t ws_bytes, float* vertices_out,
                          int64_t* faces_out, int64_t* counts, bnv_stream_t stream) {
  const int64_t V = n_vertices, T = n_faces;
  if (!counts || !mesh_sizes_ok(V, T)) return BNV_ERR_INVALID_ARGUMENT;
  if (!(vertex_threshold >= 0.0) || !std::isfinite(vertex_threshold)) return BNV_ERR_INVALID_ARGUMENT;
  if ((V && (!vertices || !vertices_out)) || (T && (!faces || !faces_out))) return BNV_ERR_INVALID_ARGUMENT;
  PostWs w;
  if (!workspace || ws_bytes < (int64_t)post_ws_layout(V, T, (char*)workspace, &w)) return BNV_ERR_WORKSPACE_TOO_SMALL;
  hipStream_t s = (hipStream_t)stream;
  BNV_HIP_CHECK(hipMemsetAsync(w.hdr, 0, sizeof(PostHdr), s));
  if (V == 0 || T == 0) {   // nothing to weld (V == 0 with faces: every face index is out of range)
    if (V) k_pp_passthrough<<<blocks_for(3 * V, kPostThreads), kPostThreads, 0, s>>>(vertices, V, vertices_out, &w.hdr->error);
    if (T) BNV_HIP_CHECK(hipMemsetAsync(&w.hdr->error, kErrFaceIndex, 1, s));
    k_pp_passthrough_counts<<<1, 1, 0, s>>>(T ? 0 : V, &w.hdr->error, counts);
    BNV_LAUNCH_CHECK();
    return BNV_OK;
  }
  const double eps = vertex_threshold, eps2 = eps * eps, cell = eps > 0.0 ? eps * kCellGrow : 0.0;
  const size_t v = (size_t)V;
  size_t tb = w.tmp_bytes;
  // 1. weld: three stable LSD passes (z, y, x) of the 64-bit axis keys, ties in vertex order
  k_pp_keys<<<blocks_for(V, kPostThreads), kPostThreads, 0, s>>>(vertices, V, cell, w);
  BNV_PRIM_CHECK(rocprim::radix_sort_pairs(w.tmp, tb, w.key[2], w.kb, w.pa, w.pb, v, 0, 64, s));
  k_pp_gather<<<blocks_for(V, kPostThreads), kPostThreads, 0, s>>>(w.key[1], w.pb, V, w.ka);
  BNV_PRIM_CHECK(rocprim::radix_sort_pairs(w.tmp, tb, w.ka, w.kb, w.pb, w.pa, v, 0, 64, s));
  k_pp_gather<<<blocks_for(V, kPostThreads), kPostThreads, 0, s>>>(w.key[0], w.pa, V, w.ka);
  BNV_PRIM_CHECK(rocprim::radix_sort_pairs(w.tmp, tb, w.ka, w.kb, w.pa, w.pb, v, 0, 64, s));
  k_pp_heads<<<blocks_for(V, kPostThreads), kPostThreads, 0, s>>>(w.pb, V, w);
  BNV_PRIM_CHECK(rocprim::inclusive_scan(w.tmp, tb, w.flag, w.scan, v, rocprim::plus<int32_t>(), s));
  k_pp_unique<<<blocks_for(V, kPostThreads), kPostThreads, 0, s>>>(w.pb, V, w);
  // 2. clusters (eps = 0: every unique point is its own)
  k_pp_cells<<<blocks_for(V, kPostThreads), kPostThreads, 0, s>>>(V, cell, w);
  if (cell > 0.0) {
    BNV_PRIM_CHECK(rocprim::radix_sort_pairs(w.tmp, tb, w.ka, w.kb, w.pb, w.pa, v, 0, 64, s));
    k_pp_union<<<blocks_for(V, kPostThreads), kPostThreads, 0, s>>>(V, cell, eps2, w);
  }
  k_pp_roots<<<blocks_for(V, kPostThreads), kPostThreads, 0, s>>>(V, w);
  BNV_PRIM_CHECK(rocprim::inclusive_scan(w.tmp, tb, w.flag, w.scan, v, rocprim::plus<int32_t>(), s));
  k_pp_labels<<<blocks_for(V, kPostThreads), kPostThreads, 0, s>>>(V, w);
  // 3. means (cluster keys sorted stably: members in ascending index order)
  BNV_PRIM_CHECK(rocprim::radix_sort_pairs(w.tmp, tb, w.ck, w.cks, w.pb, w.pa, v, 0, 32, s));
  k_pp_cstart<<<blocks_for(V, kPostThreads), kPostThreads, 0, s>>>(V, w);
  k_pp_mean<<<blocks_for(V, kPostThreads), kPostThreads, 0, s>>>(V, w);
  // 4. faces
  const FaceStep fs = face_step(w);
  BNV_TRY(run_face_step(faces, T, V, fs, V, w.tmp, w.tmp_bytes, s));
  // 5. referenced vertices
  BNV_PRIM_CHECK(rocprim::inclusive_scan(w.tmp, tb, w.flag, w.scan, v, rocprim::plus<int32_t>(), s));
  k_pp_vert_compact<<<blocks_for(V, kPostThreads), kPostThreads, 0, s>>>(V, T, w);
  k_pp_face_write<<<blocks_for(T, kPostThreads), kPostThreads, 0, s>>>(faces, T, V, w, fs, faces_out);
  // 6. smoothing over the sorted directed edges
  const int64_t E = 6 * T;
  BNV_PRIM_CHECK(rocprim::radix_sort_keys(w.tmp, tb, w.edges, w.edges_s, (size_t)E, 0, 64, s));
  BNV_HIP_CHECK(hipMemsetAsync(w.cstart, 0xff, v * 4, s));
  k_pp_rows<<<blocks_for(E, kPostThreads), kPostThreads, 0, s>>>(E, w);
  k_pp_smooth<<<blocks_for(V, kPostThreads), kPostThreads, 0, s>>>(E, w, vertices_out);
  k_pp_counts<<<1, 1, 0, s>>>(w, counts);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

}  // extern "C"
