// Rays against a triangle mesh: a depth camera that scans the user's mesh (bnv_fusion_amd/scan.py) and arbitrary rays
// (MeshScanner.cast), over the index csrc/meshsdf.hip builds (meshsdf.hpp: gathered vertices per face, a uniform grid
// of triangle ids), plus the depth sensor model the reference trains against (geometry.py: Simulator.simulate) as one
// kernel.
//
// Traversal (trace): one thread per ray.  The ray is clipped to the grid's box, then walks the fine grid cell by cell
// (3D-DDA).  The parameter at which it leaves a cell is recomputed from the integer cell index at every step, in
// float64, so nothing drifts.  Every triangle of a cell is tested; the best hit is kept across cells and is final as
// soon as it lies no further than the exit of the cell just visited (less a slack of a few fp32 ulp: a triangle is
// listed in every cell its box overlaps, so a hit beyond the cell is found again, or kept, later).
//
// Ray / triangle test (tri_hit): Woop, Benthin & Wald, "Watertight Ray/Triangle Intersection" (JCGT 2013).  The
// vertices are translated to the ray's origin and sheared so the ray runs along +z; the three 2D edge functions decide
// the hit.  Two faces that share an edge compute that edge's function from the same two sheared vertices, so the two
// values are exact negatives of each other: a ray cannot pass between them.  An edge function that is exactly zero in
// fp32 is redone in float64, where the two products are exact and the sign of their difference is the true sign.
// Two-sided (no culling).  fp32, one rounding per operation (-ffp-contract=off).  (t, face) lexicographic: the lowest
// face index wins a tie in t, so the order the grid's atomics gave the ids of a cell does not matter.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/bnv_fusion.h"
#include "bnv_common.hpp"
#include "meshsdf.hpp"

namespace bnv {
namespace {

constexpr int kMaxPoses = BNV_MESH_RENDER_MAX_POSES;

#ifdef BNV_MESHRAY_COUNT
__device__ unsigned long long g_ray_counts[2];   // cells stepped, triangles tested (tools/mesh_ray_bench.py)
#endif

struct Hit {
  float t, u, v;     // hit = (1 - u - v) a + u b + v c
  int32_t face;      // INT32_MAX: none
};

struct RayFrame {    // what Woop's test needs of a ray, once per ray
  int kx, ky, kz;
  float Sx, Sy, Sz;
};

__device__ __forceinline__ float pick(const float v[3], int k) { return k == 0 ? v[0] : (k == 1 ? v[1] : v[2]); }

__device__ __forceinline__ RayFrame ray_frame(const float d[3]) {
  RayFrame R;
  const float ax = fabsf(d[0]), ay = fabsf(d[1]), az = fabsf(d[2]);
  R.kz = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
  R.kx = R.kz == 2 ? 0 : R.kz + 1;
  R.ky = R.kx == 2 ? 0 : R.kx + 1;
  const float dz = pick(d, R.kz);
  if (dz < 0.0f) {   // keep the winding
    const int s = R.kx;
    R.kx = R.ky;
    R.ky = s;
  }
  R.Sx = pick(d, R.kx) / dz;
  R.Sy = pick(d, R.ky) / dz;
  R.Sz = 1.0f / dz;
  return R;
}

__device__ __forceinline__ void tri_hit(const float o[3], const RayFrame& R, const float4 A4, const float4 B4,
                                        const float4 C4, int32_t f, float t_min, float t_max, Hit& best) {
  const float A[3] = {A4.x - o[0], A4.y - o[1], A4.z - o[2]};
  const float B[3] = {B4.x - o[0], B4.y - o[1], B4.z - o[2]};
  const float C[3] = {C4.x - o[0], C4.y - o[1], C4.z - o[2]};
  const float Akz = pick(A, R.kz), Bkz = pick(B, R.kz), Ckz = pick(C, R.kz);
  const float Ax = pick(A, R.kx) - R.Sx * Akz, Ay = pick(A, R.ky) - R.Sy * Akz;
  const float Bx = pick(B, R.kx) - R.Sx * Bkz, By = pick(B, R.ky) - R.Sy * Bkz;
  const float Cx = pick(C, R.kx) - R.Sx * Ckz, Cy = pick(C, R.ky) - R.Sy * Ckz;
  float U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
  if (U == 0.0f || V == 0.0f || W == 0.0f) {
    U = (float)((double)Cx * (double)By - (double)Cy * (double)Bx);
    V = (float)((double)Ax * (double)Cy - (double)Ay * (double)Cx);
    W = (float)((double)Bx * (double)Ay - (double)By * (double)Ax);
  }
  if ((U < 0.0f || V < 0.0f || W < 0.0f) && (U > 0.0f || V > 0.0f || W > 0.0f)) return;
  const float det = (U + V) + W;
  if (det == 0.0f) return;
  const float Az = R.Sz * Akz, Bz = R.Sz * Bkz, Cz = R.Sz * Ckz;
  const float T = (U * Az + V * Bz) + W * Cz;
  const float t = T / det;
  if (!(t >= t_min && t <= t_max)) return;   // (NaN: no hit)
  if (t < best.t || (t == best.t && f < best.face)) {
    best.t = t;
    best.face = f;
    best.u = V / det;
    best.v = W / det;
  }
}

// The nearest hit of ray o + t d, t in [t_min, t_max], or best.face == INT32_MAX.  The caller has checked that the
// index is valid (magic, n_cells[0] > 0) and the ray finite.
__device__ __forceinline__ Hit trace(const Header& H, const Ws& W, const float o[3], const float d[3], float t_min,
                                     float t_max) {
  Hit best;
  best.t = INFINITY;
  best.u = best.v = 0.0f;
  best.face = INT32_MAX;
  if (d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f) return best;
  const int D[3] = {H.dims[0][0], H.dims[0][1], H.dims[0][2]};
  const double h = H.h;
  // clip to the grid's box [lo, lo + dims h], which holds the mesh's box
  double t0 = (double)t_min, t1 = (double)t_max;
  double od[3], dd[3], inv[3];
  float dmax = 0.0f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    od[a] = (double)o[a];
    dd[a] = (double)d[a];
    dmax = fmaxf(dmax, fabsf(d[a]));
    const double lo = H.lo[a], hi = H.lo[a] + (double)D[a] * h;
    if (d[a] == 0.0f) {
      inv[a] = 0.0;
      if (od[a] < lo || od[a] > hi) return best;
    } else {
      inv[a] = 1.0 / dd[a];
      const double ta = (lo - od[a]) * inv[a], tb = (hi - od[a]) * inv[a];
      t0 = fmax(t0, fmin(ta, tb));
      t1 = fmin(t1, fmax(ta, tb));
    }
  }
  if (!(t0 <= t1)) return best;
  int c[3], step[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    double k = floor(((od[a] + t0 * dd[a]) - H.lo[a]) * H.inv_h);
    k = fmin(fmax(k, 0.0), (double)(D[a] - 1));
    c[a] = (int)k;
    step[a] = d[a] > 0.0f ? 1 : (d[a] < 0.0f ? -1 : 0);
  }
  // a hit is final when it lies before the cell's exit by more than what fp32 can misplace it
  const double slack_abs = H.eps_abs / (double)dmax;
  const RayFrame R = ray_frame(d);
  const uint32_t* __restrict__ start = W.start[0];
  const uint32_t* __restrict__ ids = W.ids[0];
  const float4* __restrict__ tri = W.tri;
#ifdef BNV_MESHRAY_COUNT
  unsigned long long n_cells = 0, n_tests = 0;
#endif
  const int64_t max_steps = (int64_t)D[0] + D[1] + D[2] + 3;
  for (int64_t it = 0; it < max_steps; ++it) {
    const int64_t cell = ((int64_t)c[0] * D[1] + c[1]) * D[2] + c[2];
    const uint32_t e = start[cell + 1];
    for (uint32_t k = start[cell]; k < e; ++k) {
      const uint32_t f = ids[k];
      tri_hit(o, R, tri[(int64_t)f * 3], tri[(int64_t)f * 3 + 1], tri[(int64_t)f * 3 + 2], (int32_t)f, t_min, t_max,
              best);
#ifdef BNV_MESHRAY_COUNT
      ++n_tests;
#endif
    }
#ifdef BNV_MESHRAY_COUNT
    ++n_cells;
#endif
    // where the ray leaves this cell, from the cell index (no accumulation)
    double t_exit = INFINITY;
    int axis = -1;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (step[a] == 0) continue;
      const double plane = H.lo[a] + (double)(c[a] + (step[a] > 0 ? 1 : 0)) * h;
      const double ta = (plane - od[a]) * inv[a];
      if (ta < t_exit) {
        t_exit = ta;
        axis = a;
      }
    }
    if (best.face != INT32_MAX) {
      const double tb = (double)best.t;
      if (tb + 1e-5 * fabs(tb) + slack_abs <= t_exit) break;
    }
    if (axis < 0 || t_exit > t1) break;
    c[axis] += step[axis];
    if (c[axis] < 0 || c[axis] >= D[axis]) break;
  }
#ifdef BNV_MESHRAY_COUNT
  atomicAdd(&g_ray_counts[0], n_cells);
  atomicAdd(&g_ray_counts[1], n_tests);
#endif
  return best;
}

__device__ __forceinline__ bool index_ok(const Header& H, int64_t ws_bytes) {
  return H.magic == kMagic && H.bytes <= ws_bytes && H.n_cells[0] > 0;
}

// geometric normal (b - a) x (c - a) of a face, fp32
__device__ __forceinline__ void face_normal(const float4* __restrict__ tri, int32_t f, float n[3]) {
  const float4 A = tri[(int64_t)f * 3], B = tri[(int64_t)f * 3 + 1], C = tri[(int64_t)f * 3 + 2];
  const float e1[3] = {B.x - A.x, B.y - A.y, B.z - A.z}, e2[3] = {C.x - A.x, C.y - A.y, C.z - A.z};
  n[0] = e1[1] * e2[2] - e1[2] * e2[1];
  n[1] = e1[2] * e2[0] - e1[0] * e2[2];
  n[2] = e1[0] * e2[1] - e1[1] * e2[0];
}

__global__ __launch_bounds__(256) void k_ray_cast(const char* __restrict__ ws, int64_t ws_bytes,
                                                  const float* __restrict__ origins, const float* __restrict__ dirs,
                                                  int64_t n, float t_min, float t_max, float* __restrict__ t_out,
                                                  int32_t* __restrict__ face_out, float* __restrict__ uv_out,
                                                  uint8_t* __restrict__ flags_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Header& H = *(const Header*)ws;
  const float o[3] = {origins[i * 3], origins[i * 3 + 1], origins[i * 3 + 2]};
  const float d[3] = {dirs[i * 3], dirs[i * 3 + 1], dirs[i * 3 + 2]};
  float t = __builtin_nanf(""), u = t, v = t;
  int32_t face = -1;
  uint32_t flags = 0;
  if (index_ok(H, ws_bytes) && finite3(o[0], o[1], o[2]) && finite3(d[0], d[1], d[2])) {
    Ws W;
    msdf_layout(H.n_vertices, H.n_faces, const_cast<char*>(ws), &W);
    const Hit hit = trace(H, W, o, d, t_min, t_max);
    if (hit.face != INT32_MAX) {
      t = hit.t;
      u = hit.u;
      v = hit.v;
      face = hit.face;
      float nrm[3];
      face_normal(W.tri, face, nrm);
      flags = 1u | (((nrm[0] * d[0] + nrm[1] * d[1]) + nrm[2] * d[2]) > 0.0f ? 2u : 0u);
    }
  }
  t_out[i] = t;
  if (face_out) face_out[i] = face;
  if (uv_out) {
    uv_out[i * 2] = u;
    uv_out[i * 2 + 1] = v;
  }
  if (flags_out) flags_out[i] = (uint8_t)flags;
}

struct Cameras {
  float fx, fy, cx, cy;
  float T[kMaxPoses][12];   // rows of [R | t]
};

// A block is 16 x 16 pixels, each of its four waves an 8 x 8 tile: the lanes of a wave walk nearly the same cells.
__global__ __launch_bounds__(256) void k_render_depth(const char* __restrict__ ws, int64_t ws_bytes, Cameras cam,
                                                      int height, int width, float near, float max_depth,
                                                      float* __restrict__ depth_out, int32_t* __restrict__ face_out,
                                                      float* __restrict__ normal_out, uint32_t* __restrict__ seen,
                                                      int64_t n_seen) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int px = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
  const int py = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
  if (px >= width || py >= height) return;
  const int p = blockIdx.z;
  const Header& H = *(const Header*)ws;
  const float* T = cam.T[p];
  // the front end's arithmetic (frontend.hip): x = (u - cx) / fx, y = (v - cy) / fy, direction R (x, y, 1)
  const float x = ((float)px - cam.cx) / cam.fx, y = ((float)py - cam.cy) / cam.fy;
  const float o[3] = {T[3], T[7], T[11]};
  const float d[3] = {(T[0] * x + T[1] * y) + T[2], (T[4] * x + T[5] * y) + T[6], (T[8] * x + T[9] * y) + T[10]};
  float depth = 0.0f, nrm[3] = {0.0f, 0.0f, 0.0f};
  int32_t face = -1;
  if (index_ok(H, ws_bytes) && finite3(o[0], o[1], o[2]) && finite3(d[0], d[1], d[2])) {
    Ws W;
    msdf_layout(H.n_vertices, H.n_faces, const_cast<char*>(ws), &W);
    // the nearest surface is what the camera sees: one nearer than `near` hides what lies behind it
    const Hit hit = trace(H, W, o, d, 0.0f, max_depth);
    if (hit.face != INT32_MAX && hit.t > 0.0f && hit.t >= near && hit.t < max_depth) {
      depth = hit.t;
      face = hit.face;
      if (normal_out) {
        face_normal(W.tri, face, nrm);
        const float len = sqrtf((nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2]);
        const float s = ((nrm[0] * d[0] + nrm[1] * d[1]) + nrm[2] * d[2]) > 0.0f ? -1.0f : 1.0f;
#pragma unroll
        for (int a = 0; a < 3; ++a) nrm[a] = len > 0.0f ? s * (nrm[a] / len) : 0.0f;
      }
    }
  }
  if (seen) {
    // Neighbouring pixels mostly see the same face: up to four rounds in which the first lane still waiting adds the
    // number of lanes that share its face, then every lane left adds its own.  Integer adds: any grouping, the same sum.
    int32_t mine = (face >= 0 && face < n_seen) ? face : -1;
    for (int round = 0; round < 4; ++round) {
      const unsigned long long todo = __ballot(mine >= 0);
      if (todo == 0) break;
      const int leader = __ffsll(todo) - 1;
      const int32_t theirs = __shfl(mine, leader, 64);
      const unsigned long long same = __ballot(mine == theirs);
      if (lane == leader) atomicAdd(&seen[theirs], (uint32_t)__popcll(same));
      if (mine == theirs) mine = -1;
    }
    if (mine >= 0) atomicAdd(&seen[mine], 1u);
  }
  const int64_t at = ((int64_t)p * height + py) * width + px;
  depth_out[at] = depth;
  if (face_out) face_out[at] = face;
  if (normal_out) {
    normal_out[at * 3] = nrm[0];
    normal_out[at * 3 + 1] = nrm[1];
    normal_out[at * 3 + 2] = nrm[2];
  }
}

// =====================================================================================================================
// Depth sensor
// =====================================================================================================================
// Philox4x32-10 (Salmon et al., "Parallel Random Numbers: As Easy as 1, 2, 3", SC 2011)
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (uint32_t)p1;
    c[3] = (uint32_t)p0;
    c[0] = n0;
    c[2] = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// uniform in (0, 1) from the top 23 bits: (k + 0.5) 2^-23, exact in fp32
__device__ __forceinline__ float unit(uint32_t r) { return ((float)(r >> 9) + 0.5f) * 1.1920928955078125e-07f; }

// Simulator.simulate (geometry.py:42-72) per output pixel; the three normals are fp32 Box-Muller draws, everything
// after them float64 like the reference's Python floats.
__global__ __launch_bounds__(256) void k_depth_sensor(const float* __restrict__ clean, int height, int width,
                                                      const float* __restrict__ table, uint64_t seed, uint32_t frame,
                                                      double bf, double sigma_d, double sigma_px,
                                                      uint16_t* __restrict__ out) {
  const int c = blockIdx.x * 16 + (threadIdx.x & 15), r = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (c >= width || r >= height) return;
  uint32_t ctr[4] = {(uint32_t)(r * width + c), frame, 0u, 0u};
  philox4x32_10(ctr, (uint32_t)seed, (uint32_t)(seed >> 32));
  const float ra = sqrtf(-2.0f * logf(unit(ctr[0]))), rb = sqrtf(-2.0f * logf(unit(ctr[2])));
  const float pa = 6.2831854820251465f * unit(ctr[1]), pb = 6.2831854820251465f * unit(ctr[3]);
  const float n0 = ra * cosf(pa), n1 = ra * sinf(pa), n2 = rb * cosf(pb);
  const double xs = rint((double)c + sigma_px * (double)n0), ys = rint((double)r + sigma_px * (double)n1);
  const int x = (int)fmin(fmax(xs, 0.0), (double)(width - 1)), y = (int)fmin(fmax(ys, 0.0), (double)(height - 1));
  double d = (double)clean[(int64_t)(y - y % 2) * width + (x - x % 2)];
  if (table) {   // Simulator.undistort
    const int i2 = (int)((d + 1.0) / 2.0), i1 = i2 - 1;
    const double a = (d - (double)(i1 * 2 + 1)) / 2.0;
    const int tx = min((int)((int64_t)x * 80 / width), 79), ty = min((int)((int64_t)y * 80 / height), 79);
    const float* m = table + ((int64_t)ty * 80 + tx) * 5;
    const double f = (1.0 - a) * (double)m[min(max(i1, 0), 4)] + a * (double)m[min(max(i2, 0), 4)];
    d = f == 0.0 ? 0.0 : d / f;
  }
  double mm = 0.0;
  if (d > 0.0 && isfinite(d)) {
    const double k = rint((bf / d + sigma_d * (double)n2) * 8.0);
    if (k != 0.0) mm = trunc(bf * 8.0 / k * 1000.0);
  }
  out[(int64_t)r * width + c] = (uint16_t)fmin(fmax(mm, 0.0), 65535.0);
}

}  // namespace
}  // namespace bnv

using namespace bnv;

extern "C" {

int bnv_mesh_ray_workspace_bytes(int64_t n_vertices, int64_t n_faces, int64_t* bytes) {
  return bnv_mesh_sdf_workspace_bytes(n_vertices, n_faces, bytes);
}

int bnv_mesh_ray_cast(const void* workspace, int64_t ws_bytes, const float* origins, const float* dirs, int64_t n_rays,
                      float t_min, float t_max, float* t_out, int32_t* face_out, float* uv_out, uint8_t* flags_out,
                      bnv_stream_t stream) {
  if (!workspace || !origins || !dirs || !t_out || n_rays <= 0 || n_rays > INT32_MAX) return BNV_ERR_INVALID_ARGUMENT;
  if (!(t_min <= t_max)) return BNV_ERR_INVALID_ARGUMENT;
  if (ws_bytes < (int64_t)msdf_layout(1, 1, nullptr, nullptr)) return BNV_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_ray_cast, dim3(blocks_for(n_rays, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const char*)workspace, ws_bytes, origins, dirs, n_rays, t_min, t_max, t_out, face_out, uv_out,
                     flags_out);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

int bnv_mesh_render_depth(const void* workspace, int64_t ws_bytes, int n_poses, const float* K_host,
                          const float* poses_host, int height, int width, float near, float max_depth,
                          float* depth_out, int32_t* face_out, float* normals_out, uint32_t* seen, int64_t n_seen,
                          bnv_stream_t stream) {
  if (!workspace || !K_host || !poses_host || !depth_out) return BNV_ERR_INVALID_ARGUMENT;
  if (n_poses < 1 || n_poses > kMaxPoses || height < 1 || width < 1 || height > 32768 || width > 32768)
    return BNV_ERR_INVALID_ARGUMENT;
  if (!(near <= max_depth) || !(max_depth > 0.0f)) return BNV_ERR_INVALID_ARGUMENT;
  if (ws_bytes < (int64_t)msdf_layout(1, 1, nullptr, nullptr)) return BNV_ERR_INVALID_ARGUMENT;
  if (seen && n_seen < 1) return BNV_ERR_INVALID_ARGUMENT;
  if (!(K_host[0] != 0.0f) || !(K_host[4] != 0.0f)) return BNV_ERR_INVALID_ARGUMENT;
  Cameras cam;
  cam.fx = K_host[0];
  cam.fy = K_host[4];
  cam.cx = K_host[2];
  cam.cy = K_host[5];
  for (int p = 0; p < kMaxPoses; ++p)
    for (int k = 0; k < 12; ++k) cam.T[p][k] = p < n_poses ? poses_host[p * 16 + k] : 0.0f;
  const dim3 grid((unsigned)((width + 15) / 16), (unsigned)((height + 15) / 16), (unsigned)n_poses);
  hipLaunchKernelGGL(k_render_depth, grid, dim3(256), 0, (hipStream_t)stream, (const char*)workspace, ws_bytes, cam,
                     height, width, near, max_depth, depth_out, face_out, normals_out, seen, n_seen);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

int bnv_depth_sensor(const float* clean, int height, int width, const float* table, uint64_t seed, uint32_t frame,
                     double bf, double sigma_d, double sigma_px, uint16_t* out_mm, bnv_stream_t stream) {
  if (!clean || !out_mm || height < 1 || width < 1 || height > 32768 || width > 32768) return BNV_ERR_INVALID_ARGUMENT;
  if (!(bf > 0.0) || !(sigma_d >= 0.0) || !(sigma_px >= 0.0) || !(bf < 1e30) || !(sigma_d < 1e30) || !(sigma_px < 1e30))
    return BNV_ERR_INVALID_ARGUMENT;
  const dim3 grid((unsigned)((width + 15) / 16), (unsigned)((height + 15) / 16));
  hipLaunchKernelGGL(k_depth_sensor, grid, dim3(256), 0, (hipStream_t)stream, clean, height, width, table, seed, frame,
                     bf, sigma_d, sigma_px, out_mm);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

#ifdef BNV_MESHRAY_COUNT
// counting build only (tools/mesh_ray_bench.py): cells stepped and triangles tested since the last read
int bnv_mesh_ray_counts(unsigned long long out[2]) {
  BNV_HIP_CHECK(hipDeviceSynchronize());
  BNV_HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ray_counts), 16));
  const unsigned long long zero[2] = {0, 0};
  BNV_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_ray_counts), zero, 16));
  return BNV_OK;
}
#endif

}  // extern "C"
