// render.hip -- depth and normal images of the map from a camera pose (include/bnv_fusion.h: bnv_render_depth,
// bnv_tsdf_render_depth).  The reference has no such entry: its only renderer samples rays for the L1 loss
// (render_utils.py:461-560); this is the model view a fusion system shows.
//
// Neural volume, in rounds until no ray is active:
//   k_render_emit     every active ray walks its fixed sample schedule from its cursor, tests each sample's 8 decode
//                     corners against the volume (brick, else hash) and appends its next <= K in-domain samples to
//                     a compacted buffer (world coordinates; one atomic per wave), each run of them together with the
//                     out-of-domain sample right before it (decode_pts gives it its masked constant, no MLP);
//   bnv_decode_pts    the existing live-query-compacted decode runs on that buffer (the count is read on the host);
//   k_render_resolve  scans each ray's new values with the value carried from the previous round: a hit ends the
//                     ray, a ray whose schedule is exhausted retires, the rest form the next round's active list.
// Then k_render_hit_points + bnv_decode_pts (6 points per hit) + k_render_normals.  The TSDF side volume needs no
// MLP: k_tsdf_render walks the whole schedule per thread.  Both share ray setup, schedule and hit interpolation.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/bnv_fusion.h"
#include "bnv_common.hpp"
#include "scan.hpp"
#include "volume_keys.hpp"
#include "workspace.hpp"

namespace bnv {

constexpr int kRenderThreads = 256;
constexpr int kRenderWalk = 512;        // schedule samples a ray examines per round at most
constexpr int kRenderWindow = 64;       // emitted samples of a round lie within 64 steps of the round's first one
constexpr int kRenderMaxSteps = 1 << 24;

struct RenderCam {
  float R[9];     // camera-to-world rotation, row-major
  float o[3];     // camera centre (world)
  float fx, fy, cx, cy;
  int32_t H, W;
  float near_z, max_z;
  float lo[3], hi[3];  // sample box (world)
  float step;          // Euclidean sample spacing (world units)
};

struct Ray {
  float o[3], d[3];
  float nrm;      // |R (x, y, 1)|: z-depth = t / nrm
  float t0, t1;   // first sample at t0; samples while t <= t1
};

// include/bnv_fusion.h, "Rendering": every operation one IEEE fp32 rounding, in this order.
__device__ __forceinline__ Ray ray_setup(const RenderCam& c, int64_t pix) {
  Ray r;
  const int v = (int)(pix / c.W), u = (int)(pix - (int64_t)v * c.W);
  const float x = __fdiv_rn(__fsub_rn((float)u, c.cx), c.fx);
  const float y = __fdiv_rn(__fsub_rn((float)v, c.cy), c.fy);
  float dw[3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
    dw[a] = __fadd_rn(__fadd_rn(__fmul_rn(c.R[3 * a], x), __fmul_rn(c.R[3 * a + 1], y)), c.R[3 * a + 2]);
  r.nrm = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(dw[0], dw[0]), __fmul_rn(dw[1], dw[1])), __fmul_rn(dw[2], dw[2])));
  float tin = 0.f, tout = INFINITY;
  bool miss = false;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    r.o[a] = c.o[a];
    r.d[a] = __fdiv_rn(dw[a], r.nrm);
    if (r.d[a] == 0.f) {
      if (c.o[a] < c.lo[a] || c.o[a] > c.hi[a]) miss = true;
    } else {
      const float t1 = __fdiv_rn(__fsub_rn(c.lo[a], c.o[a]), r.d[a]);
      const float t2 = __fdiv_rn(__fsub_rn(c.hi[a], c.o[a]), r.d[a]);
      tin = fmaxf(tin, fminf(t1, t2));
      tout = fminf(tout, fmaxf(t1, t2));
    }
  }
  r.t0 = fmaxf(tin, __fmul_rn(c.near_z, r.nrm));
  r.t1 = fminf(tout, __fmul_rn(c.max_z, r.nrm));
  if (miss) r.t1 = -1.f;
  return r;
}

__device__ __forceinline__ float ray_t(const Ray& r, float step, int k) {
  return __fadd_rn(r.t0, __fmul_rn((float)k, step));
}

__device__ __forceinline__ void ray_pos(const Ray& r, float t, float (&p)[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) p[a] = __fadd_rn(r.o[a], __fmul_rn(t, r.d[a]));
}

// hit between consecutive in-domain samples (k - 1, k) with values (f0, f1): f0 > 0 >= f1
__device__ __forceinline__ bool is_crossing(float f0, float f1) { return f0 > 0.f && f1 <= 0.f; }

// t of the crossing: t(k-1) + (f0 / (f0 - f1)) * step
__device__ __forceinline__ float crossing_t(const Ray& r, float step, int k_prev, float f0, float f1) {
  return __fadd_rn(ray_t(r, step, k_prev), __fmul_rn(__fdiv_rn(f0, __fsub_rn(f0, f1)), step));
}

__device__ __forceinline__ void normalise3(float (&g)[3]) {
  const float l = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(g[0], g[0]), __fmul_rn(g[1], g[1])), __fmul_rn(g[2], g[2])));
#pragma unroll
  for (int a = 0; a < 3; ++a) g[a] = l > 0.f ? __fdiv_rn(g[a], l) : 0.f;
}

// wave-wide exclusive prefix of `count`; lane 63 reserves the wave's total from *counter (one atomic per wave)
__device__ __forceinline__ int32_t wave_alloc(int32_t count, int32_t* counter) {
  const int lane = threadIdx.x & 63;
  const int32_t incl = wave_inclusive_scan(count);
  const int32_t total = __shfl(incl, 63);
  int32_t base = 0;
  if (lane == 63 && total > 0) base = atomicAdd(counter, total);
  base = __shfl(base, 63);
  return base + incl - count;
}

// ---- neural volume -----------------------------------------------------------------------------------------------

struct RenderCtr {
  int32_t n_active[2];
  int32_t n_samples;
  int32_t n_hits;
  unsigned long long live;   // emitted samples whose 8 corner weights all reach min_pts_in_grid
  int32_t pad[10];
};

struct RenderWs {
  int32_t* cursor;     // [n] next schedule index, -1 = exhausted
  int32_t* prev_k;     // [n] index of the last decoded sample (-2: none)
  float* prev_f;       // [n] its value
  float* hit_t;        // [n] t of the hit, -1 = none
  int32_t* slot_base;  // [n] this round's samples of the ray: [slot_base, slot_base + slot_cnt)
  int32_t* slot_cnt;
  int32_t* active[2];  // [n] active ray lists (double-buffered)
  int32_t* hit_list;   // [n]
  int32_t* sample_k;   // [n (K + 1)] schedule index of an in-domain sample, or -1 - index of a run's lead-in sample
  float* pts;          // [n max(K + 1, 6) 3]
  float* vals;         // [n max(K + 1, 6)]
  RenderCtr* ctr;
};

static size_t render_ws_layout(int64_t n, int k, char* base, RenderWs* w) {
  const int64_t m = k + 1 > 6 ? k + 1 : 6;
  Carver c(base);
  RenderWs t;
  t.cursor = c.take<int32_t>(n);
  t.prev_k = c.take<int32_t>(n);
  t.prev_f = c.take<float>(n);
  t.hit_t = c.take<float>(n);
  t.slot_base = c.take<int32_t>(n);
  t.slot_cnt = c.take<int32_t>(n);
  t.active[0] = c.take<int32_t>(n);
  t.active[1] = c.take<int32_t>(n);
  t.hit_list = c.take<int32_t>(n);
  t.sample_k = c.take<int32_t>(n * (k + 1));
  t.pts = c.take<float>(n * m * 3);
  t.vals = c.take<float>(n * m);
  t.ctr = c.take<RenderCtr>(1);
  if (w) *w = t;
  return c.bytes();
}

struct NeuralField {
  bnv_volume_t vol;
  bnv_grid_t grid;
  const float* weights;
  int64_t row_limit;
};

__device__ __forceinline__ bool row_ok(const NeuralField& F, int64_t x, int64_t y, int64_t z, int* row) {
  const int r = volume_row(F.vol, x, y, z);
  *row = r;
  return r >= 0 && r < F.row_limit;
}

// the 8 corners k_decode_pts gathers at world point p (floor / ceil per axis of (p - bound_min) / voxel) are rows
// of the volume.  `cell`: the last full cell tested and its result (points strictly inside a cell share the answer).
__device__ __forceinline__ bool neural_in_domain(const NeuralField& F, const float (&p)[3], int64_t (&cell)[4]) {
  float fl[3], ce[3];
  bool interior = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float c = voxel_coord(p[a], F.grid.bound_min[a], F.grid.voxel_size);
    fl[a] = floorf(c);
    ce[a] = ceilf(c);
    interior = interior && fl[a] != ce[a];
  }
  const int64_t x = (int64_t)fl[0], y = (int64_t)fl[1], z = (int64_t)fl[2];
  if (interior && cell[0] == x && cell[1] == y && cell[2] == z) return cell[3] != 0;
  bool ok = true;
  for (int b = 0; b < 8 && ok; ++b) {
    int row;
    ok = row_ok(F, (int64_t)((b & 1) ? ce[0] : fl[0]), (int64_t)((b & 2) ? ce[1] : fl[1]),
                (int64_t)((b & 4) ? ce[2] : fl[2]), &row);
  }
  if (interior) {
    cell[0] = x;
    cell[1] = y;
    cell[2] = z;
    cell[3] = ok;
  }
  return ok;
}

// the decode would run the MLP at p (every corner weight >= min_pts_in_grid), for the statistics only
__device__ __forceinline__ bool neural_live(const NeuralField& F, const float (&p)[3]) {
  float fl[3], ce[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float c = voxel_coord(p[a], F.grid.bound_min[a], F.grid.voxel_size);
    fl[a] = floorf(c);
    ce[a] = ceilf(c);
  }
  for (int b = 0; b < 8; ++b) {
    int row;
    if (!row_ok(F, (int64_t)((b & 1) ? ce[0] : fl[0]), (int64_t)((b & 2) ? ce[1] : fl[1]),
                (int64_t)((b & 4) ? ce[2] : fl[2]), &row))
      return false;
    if (!(F.weights[row] >= (float)F.grid.min_pts_in_grid)) return false;
  }
  return true;
}

__global__ __launch_bounds__(kRenderThreads) void k_render_init(RenderCam cam, RenderWs w, int64_t n, float* depth,
                                                                float* normals) {
  const int64_t r = (int64_t)blockIdx.x * kRenderThreads + threadIdx.x;
  int32_t go = 0;
  if (r < n) {
    const Ray ray = ray_setup(cam, r);
    go = ray.t0 <= ray.t1 ? 1 : 0;
    w.cursor[r] = go ? 0 : -1;
    w.prev_k[r] = -2;
    w.prev_f[r] = 0.f;
    w.hit_t[r] = -1.f;
    depth[r] = 0.f;
    if (normals) normals[3 * r] = normals[3 * r + 1] = normals[3 * r + 2] = 0.f;
  }
  const int32_t slot = wave_alloc(go, &w.ctr->n_active[0]);
  if (go) w.active[0][slot] = (int32_t)r;
}

__global__ __launch_bounds__(kRenderThreads) void k_render_emit(RenderCam cam, RenderWs w, NeuralField F, int cur,
                                                                int k_max, int stats) {
  const int64_t i = (int64_t)blockIdx.x * kRenderThreads + threadIdx.x;
  const int32_t n_act = w.ctr->n_active[cur];
  const int32_t r = i < n_act ? w.active[cur][i] : -1;
  int32_t count = 0, kf = -1;
  unsigned long long mask = 0, lead = 0;   // bit b: sample kf + b is emitted / is a run's lead-in (out of domain)
  Ray ray;
  if (r >= 0) {
    ray = ray_setup(cam, r);
    int k = w.cursor[r];
    int last = w.prev_k[r];        // last emitted sample (carried between rounds)
    int64_t cell[4] = {INT64_MIN, 0, 0, 0};
    for (int s = 0; s < kRenderWalk; ++s) {
      const float t = ray_t(ray, cam.step, k);
      if (!(t <= ray.t1) || k >= kRenderMaxSteps) {
        k = -1;
        break;
      }
      float p[3];
      ray_pos(ray, t, p);
      if (neural_in_domain(F, p, cell)) {
        if (k >= 1 && last != k - 1) {      // a run starts: its lead-in sample k - 1 goes along
          if (kf < 0) kf = k - 1;
          mask |= 1ull << (k - 1 - kf);
          lead |= 1ull << (k - 1 - kf);
          ++count;
        }
        if (kf < 0) kf = k;
        mask |= 1ull << (k - kf);
        ++count;
        last = k;
      }
      ++k;
      if (count >= k_max || (kf >= 0 && k - kf >= kRenderWindow - 1)) break;
    }
    w.cursor[r] = k;
  }
  const int32_t base = wave_alloc(count, &w.ctr->n_samples);
  unsigned live = 0;
  if (r >= 0) {
    w.slot_base[r] = base;
    w.slot_cnt[r] = count;
    int j = 0;
    while (mask) {
      const int b = __builtin_ctzll(mask);
      mask &= mask - 1ull;
      const int k = kf + b;
      const bool is_lead = (lead >> b) & 1ull;
      float p[3];
      ray_pos(ray, ray_t(ray, cam.step, k), p);
      const int64_t q = (int64_t)base + j;
      w.pts[3 * q] = p[0];
      w.pts[3 * q + 1] = p[1];
      w.pts[3 * q + 2] = p[2];
      w.sample_k[q] = is_lead ? -1 - k : k;
      if (stats && !is_lead) live += neural_live(F, p) ? 1u : 0u;
      ++j;
    }
  }
  if (stats) {
    unsigned long long s = live;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&w.ctr->live, s);
  }
}

__global__ __launch_bounds__(kRenderThreads) void k_render_resolve(RenderCam cam, RenderWs w, int cur, int32_t n_act,
                                                                   float* depth) {
  const int64_t i = (int64_t)blockIdx.x * kRenderThreads + threadIdx.x;
  const int32_t r = i < n_act ? w.active[cur][i] : -1;
  int32_t keep = 0;
  if (r >= 0) {
    const Ray ray = ray_setup(cam, r);
    int pk = w.prev_k[r];
    float pf = w.prev_f[r];
    const int32_t base = w.slot_base[r], cnt = w.slot_cnt[r];
    bool hit = false;
    for (int j = 0; j < cnt; ++j) {
      const int code = w.sample_k[base + j];
      const bool in_domain = code >= 0;
      const int k = in_domain ? code : -1 - code;
      const float f = w.vals[base + j];
      if (in_domain && k == pk + 1 && is_crossing(pf, f)) {
        const float t = crossing_t(ray, cam.step, pk, pf, f);
        w.hit_t[r] = t;
        depth[r] = __fdiv_rn(t, ray.nrm);
        hit = true;
        break;
      }
      pk = k;
      pf = f;
    }
    w.prev_k[r] = pk;
    w.prev_f[r] = pf;
    keep = (!hit && w.cursor[r] >= 0) ? 1 : 0;
  }
  const int32_t slot = wave_alloc(keep, &w.ctr->n_active[cur ^ 1]);
  if (keep) w.active[cur ^ 1][slot] = r;
}

// the 6 central-difference points of every hit: p +- eps e_a, a = x, y, z (in that order)
__global__ __launch_bounds__(kRenderThreads) void k_render_hit_points(RenderCam cam, RenderWs w, int64_t n, float eps) {
  const int64_t r = (int64_t)blockIdx.x * kRenderThreads + threadIdx.x;
  const int32_t h = (r < n && w.hit_t[r] >= 0.f) ? 1 : 0;
  const int32_t slot = wave_alloc(h, &w.ctr->n_hits);
  if (!h) return;
  const Ray ray = ray_setup(cam, r);
  float p[3];
  ray_pos(ray, w.hit_t[r], p);
  w.hit_list[slot] = (int32_t)r;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int sgn = 0; sgn < 2; ++sgn) {
      float* q = w.pts + ((int64_t)slot * 6 + 2 * a + sgn) * 3;
#pragma unroll
      for (int b = 0; b < 3; ++b) q[b] = b == a ? (sgn ? __fsub_rn(p[b], eps) : __fadd_rn(p[b], eps)) : p[b];
    }
  }
}

__global__ __launch_bounds__(kRenderThreads) void k_render_normals(RenderWs w, int32_t n_hits, float* normals) {
  const int64_t j = (int64_t)blockIdx.x * kRenderThreads + threadIdx.x;
  if (j >= n_hits) return;
  const int32_t r = w.hit_list[j];
  float g[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) g[a] = __fsub_rn(w.vals[j * 6 + 2 * a], w.vals[j * 6 + 2 * a + 1]);
  normalise3(g);
#pragma unroll
  for (int a = 0; a < 3; ++a) normals[(int64_t)r * 3 + a] = g[a];
}

// ---- TSDF side volume --------------------------------------------------------------------------------------------

struct TsdfField {
  const float* tsdf;
  const float* weight;
  int32_t dim[3];
  float origin[3];
  float voxel;
};

__device__ __forceinline__ float lerp_rn(float a, float b, float f) { return __fadd_rn(a, __fmul_rn(f, __fsub_rn(b, a))); }

__device__ __forceinline__ int64_t tsdf_idx(const TsdfField& T, int x, int y, int z) {
  return ((int64_t)x * T.dim[1] + y) * T.dim[2] + z;
}

// trilinear TSDF at p: base corner i = floor(c), fraction f = c - i, c = (p - origin) / voxel; lerp along x, then y,
// then z.  In the domain iff the 8 corners i + {0,1}^3 lie in the grid with weight > 0.
__device__ __forceinline__ bool tsdf_sample(const TsdfField& T, const float (&p)[3], float* out) {
  int i[3];
  float f[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float c = __fdiv_rn(__fsub_rn(p[a], T.origin[a]), T.voxel);
    const float fl = floorf(c);
    if (!(fl >= 0.f) || !(fl < (float)(T.dim[a] - 1))) return false;
    i[a] = (int)fl;
    f[a] = __fsub_rn(c, fl);
  }
  float v[8];
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const int64_t idx = tsdf_idx(T, i[0] + (b & 1), i[1] + ((b >> 1) & 1), i[2] + ((b >> 2) & 1));
    if (!(T.weight[idx] > 0.f)) return false;
    v[b] = T.tsdf[idx];
  }
  const float y0 = lerp_rn(lerp_rn(v[0], v[1], f[0]), lerp_rn(v[2], v[3], f[0]), f[1]);
  const float y1 = lerp_rn(lerp_rn(v[4], v[5], f[0]), lerp_rn(v[6], v[7], f[0]), f[1]);
  *out = lerp_rn(y0, y1, f[2]);
  return true;
}

// gradient of the trilinear interpolant at p (cell clamped into the grid), normalised
__device__ __forceinline__ void tsdf_normal(const TsdfField& T, const float (&p)[3], float (&g)[3]) {
  int i[3];
  float f[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float c = __fdiv_rn(__fsub_rn(p[a], T.origin[a]), T.voxel);
    float fl = floorf(c);
    fl = fminf(fmaxf(fl, 0.f), (float)(T.dim[a] - 2));
    i[a] = (int)fl;
    f[a] = __fsub_rn(c, fl);
  }
  float v[8];
#pragma unroll
  for (int b = 0; b < 8; ++b) v[b] = T.tsdf[tsdf_idx(T, i[0] + (b & 1), i[1] + ((b >> 1) & 1), i[2] + ((b >> 2) & 1))];
  // d/dx: bilinear in (y, z) of the x differences; likewise for y and z
  g[0] = lerp_rn(lerp_rn(__fsub_rn(v[1], v[0]), __fsub_rn(v[3], v[2]), f[1]),
                 lerp_rn(__fsub_rn(v[5], v[4]), __fsub_rn(v[7], v[6]), f[1]), f[2]);
  g[1] = lerp_rn(lerp_rn(__fsub_rn(v[2], v[0]), __fsub_rn(v[3], v[1]), f[0]),
                 lerp_rn(__fsub_rn(v[6], v[4]), __fsub_rn(v[7], v[5]), f[0]), f[2]);
  g[2] = lerp_rn(lerp_rn(__fsub_rn(v[4], v[0]), __fsub_rn(v[5], v[1]), f[0]),
                 lerp_rn(__fsub_rn(v[6], v[2]), __fsub_rn(v[7], v[3]), f[0]), f[1]);
  normalise3(g);
}

__global__ __launch_bounds__(kRenderThreads) void k_tsdf_render(RenderCam cam, TsdfField T, int64_t n, float* depth,
                                                                float* normals) {
  const int64_t r = (int64_t)blockIdx.x * kRenderThreads + threadIdx.x;
  if (r >= n) return;
  const Ray ray = ray_setup(cam, r);
  float z = 0.f, g[3] = {0.f, 0.f, 0.f};
  int pk = -2;
  float pf = 0.f;
  for (int k = 0; k < kRenderMaxSteps; ++k) {
    const float t = ray_t(ray, cam.step, k);
    if (!(t <= ray.t1)) break;
    float p[3], f;
    ray_pos(ray, t, p);
    if (!tsdf_sample(T, p, &f)) continue;
    if (k == pk + 1 && is_crossing(pf, f)) {
      const float th = crossing_t(ray, cam.step, pk, pf, f);
      z = __fdiv_rn(th, ray.nrm);
      if (normals) {
        float ph[3];
        ray_pos(ray, th, ph);
        tsdf_normal(T, ph, g);
      }
      break;
    }
    pk = k;
    pf = f;
  }
  depth[r] = z;
  if (normals) {
    normals[3 * r] = g[0];
    normals[3 * r + 1] = g[1];
    normals[3 * r + 2] = g[2];
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------

// camera + box from the caller's arguments; false on an invalid camera
static bool make_cam(const float T_wc[16], const float K[9], int32_t H, int32_t W, float near_z, float max_depth,
                     float step_world, const float lo[3], const float hi[3], RenderCam* c) {
  if (!T_wc || !K || H <= 0 || W <= 0 || !all_finite(T_wc, 16) || !all_finite(K, 9)) return false;
  if (!(K[0] != 0.f) || !(K[4] != 0.f) || !(step_world > 0.f) || !isfinite(step_world)) return false;
  if (!(near_z >= 0.f) || !isfinite(near_z) || !(max_depth >= 0.f) || isnan(max_depth)) return false;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) c->R[3 * a + b] = T_wc[4 * a + b];
  for (int a = 0; a < 3; ++a) {
    c->o[a] = T_wc[4 * a + 3];
    c->lo[a] = lo[a];
    c->hi[a] = hi[a];
  }
  c->fx = K[0];
  c->fy = K[4];
  c->cx = K[2];
  c->cy = K[5];
  c->H = H;
  c->W = W;
  c->near_z = near_z;
  c->max_z = max_depth;
  c->step = step_world;
  return true;
}

static bool render_dims_ok(int32_t H, int32_t W, int32_t k) {
  if (H <= 0 || W <= 0 || k < 1 || k > kRenderWindow / 2) return false;
  const int64_t n = (int64_t)H * W, m = k + 1 > 6 ? k + 1 : 6;
  return n * m * 3 < INT32_MAX;
}

}  // namespace bnv

using namespace bnv;

extern "C" {

size_t bnv_render_workspace_bytes(int64_t n_rays, int32_t k) {
  if (n_rays <= 0 || k < 1 || k > kRenderWindow / 2 || n_rays * (k + 1 > 6 ? k + 1 : 6) * 3 >= INT32_MAX) return 0;
  return render_ws_layout(n_rays, k, nullptr, nullptr);
}

int bnv_render_depth(const bnv_volume_t* vol, const bnv_grid_t* grid, const float* features, const float* weights,
                     int64_t row_limit, const float* sdfmlp_pack, const bnv_sdf_delta_t* delta, const float T_wc[16],
                     const float K[9], int32_t H, int32_t W, float near_z, float max_depth, float step, int32_t k,
                     void* ws, size_t ws_bytes, float* depth_out, float* normals_out, int64_t* stats_host,
                     bnv_stream_t stream) {
  if (g_num_cus <= 0) return BNV_ERR_NOT_INITIALISED;
  if (!vol || !grid || !features || !weights || !sdfmlp_pack || !ws || !depth_out) return BNV_ERR_INVALID_ARGUMENT;
  if (!vol->slot_keys || !vol->slot_rows || vol->n_slots <= 0 || (vol->n_slots & (vol->n_slots - 1)) != 0)
    return BNV_ERR_INVALID_ARGUMENT;
  if (grid->shard_world > 1) return BNV_ERR_INVALID_ARGUMENT;
  if (!render_dims_ok(H, W, k) || !(step >= BNV_RENDER_MIN_STEP)) return BNV_ERR_INVALID_ARGUMENT;
  const int64_t n = (int64_t)H * W;
  RenderWs w;
  if (ws_bytes < render_ws_layout(n, k, (char*)ws, &w)) return BNV_ERR_WORKSPACE_TOO_SMALL;
  float lo[3], hi[3];
  for (int a = 0; a < 3; ++a) {
    lo[a] = grid->bound_min[a];
    const float span = (float)(grid->n_xyz[a] - 1) * grid->voxel_size;   // (two roundings: -ffp-contract=off)
    hi[a] = lo[a] + span;
  }
  RenderCam cam;
  if (!make_cam(T_wc, K, H, W, near_z, max_depth, step * grid->voxel_size, lo, hi, &cam))
    return BNV_ERR_INVALID_ARGUMENT;
  NeuralField F;
  F.vol = *vol;
  F.grid = *grid;
  F.weights = weights;
  F.row_limit = row_limit;
  hipStream_t s = (hipStream_t)stream;
  BNV_HIP_CHECK(hipMemsetAsync(w.ctr, 0, sizeof(RenderCtr), s));
  hipLaunchKernelGGL(k_render_init, dim3(blocks_for(n, kRenderThreads)), dim3(kRenderThreads), 0, s, cam, w, n, depth_out,
                     normals_out);
  BNV_LAUNCH_CHECK();
  int cur = 0;
  int64_t bound = n, rounds = 0, samples = 0;
  for (;;) {
    BNV_HIP_CHECK(hipMemsetAsync(&w.ctr->n_samples, 0, 4, s));
    BNV_HIP_CHECK(hipMemsetAsync(&w.ctr->n_active[cur ^ 1], 0, 4, s));
    if (bound > 0) {
      hipLaunchKernelGGL(k_render_emit, dim3(blocks_for(bound, kRenderThreads)), dim3(kRenderThreads), 0, s, cam, w, F, cur, (int)k,
                         stats_host ? 1 : 0);
      BNV_LAUNCH_CHECK();
    }
    // one host read per round: {active rays, samples emitted}
    RenderCtr h;
    BNV_HIP_CHECK(hipMemcpyAsync(&h, w.ctr, sizeof(h), hipMemcpyDeviceToHost, s));
    BNV_HIP_CHECK(hipStreamSynchronize(s));
    const int32_t n_act = h.n_active[cur];
    if (n_act <= 0) break;
    ++rounds;
    samples += h.n_samples;
    if (h.n_samples > 0) {
      const int rc = bnv_decode_pts(vol, grid, features, weights, row_limit, sdfmlp_pack, w.pts, h.n_samples, 0, delta,
                                    nullptr, 0, w.vals, stream);
      if (rc != BNV_OK) return rc;
    }
    hipLaunchKernelGGL(k_render_resolve, dim3(blocks_for(n_act, kRenderThreads)), dim3(kRenderThreads), 0, s, cam, w, cur, n_act,
                       depth_out);
    BNV_LAUNCH_CHECK();
    bound = n_act;
    cur ^= 1;
  }
  int32_t n_hits = 0;
  if (normals_out || stats_host) {
    hipLaunchKernelGGL(k_render_hit_points, dim3(blocks_for(n, kRenderThreads)), dim3(kRenderThreads), 0, s, cam, w, n,
                       BNV_RENDER_NORMAL_EPS * grid->voxel_size);
    BNV_LAUNCH_CHECK();
    BNV_HIP_CHECK(hipMemcpyAsync(&n_hits, &w.ctr->n_hits, 4, hipMemcpyDeviceToHost, s));
    BNV_HIP_CHECK(hipStreamSynchronize(s));
  }
  if (normals_out && n_hits > 0) {
    const int rc = bnv_decode_pts(vol, grid, features, weights, row_limit, sdfmlp_pack, w.pts, (int64_t)n_hits * 6, 0,
                                  delta, nullptr, 0, w.vals, stream);
    if (rc != BNV_OK) return rc;
    hipLaunchKernelGGL(k_render_normals, dim3(blocks_for(n_hits, kRenderThreads)), dim3(kRenderThreads), 0, s, w, n_hits, normals_out);
    BNV_LAUNCH_CHECK();
  }
  if (stats_host) {
    unsigned long long live = 0;
    BNV_HIP_CHECK(hipMemcpyAsync(&live, &w.ctr->live, 8, hipMemcpyDeviceToHost, s));
    BNV_HIP_CHECK(hipStreamSynchronize(s));
    stats_host[0] = rounds;
    stats_host[1] = samples;
    stats_host[2] = (int64_t)live;
    stats_host[3] = n_hits;
  }
  return BNV_OK;
}

int bnv_tsdf_render_depth(const float* tsdf, const float* weight, const int32_t dim[3], const float origin[3],
                          float voxel_size, const float T_wc[16], const float K[9], int32_t H, int32_t W, float near_z,
                          float max_depth, float step, float* depth_out, float* normals_out, bnv_stream_t stream) {
  if (g_num_cus <= 0) return BNV_ERR_NOT_INITIALISED;
  if (!tsdf || !weight || !dim || !origin || !depth_out || !(voxel_size > 0.f)) return BNV_ERR_INVALID_ARGUMENT;
  if (!render_dims_ok(H, W, 1) || !(step >= BNV_RENDER_MIN_STEP)) return BNV_ERR_INVALID_ARGUMENT;
  TsdfField T;
  float lo[3], hi[3];
  for (int a = 0; a < 3; ++a) {
    if (dim[a] < 2) return BNV_ERR_INVALID_ARGUMENT;
    T.dim[a] = dim[a];
    T.origin[a] = origin[a];
    lo[a] = origin[a];
    const float span = (float)(dim[a] - 1) * voxel_size;
    hi[a] = origin[a] + span;
  }
  T.tsdf = tsdf;
  T.weight = weight;
  T.voxel = voxel_size;
  RenderCam cam;
  if (!make_cam(T_wc, K, H, W, near_z, max_depth, step * voxel_size, lo, hi, &cam)) return BNV_ERR_INVALID_ARGUMENT;
  const int64_t n = (int64_t)H * W;
  hipLaunchKernelGGL(k_tsdf_render, dim3(blocks_for(n, kRenderThreads)), dim3(kRenderThreads), 0, (hipStream_t)stream, cam, T, n,
                     depth_out, normals_out);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

}  // extern "C"
