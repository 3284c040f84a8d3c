// Appearance of an extracted mesh on the device: area-weighted vertex normals and per-vertex colours blended from the
// RGB frames (mesh.vertex_normals_tensors / mesh.VertexColorer).  The specification is in include/bnv_fusion.h ("Mesh
// normals and colours"); tests/mesh_color_restatement.py restates it in numpy and matches it bit for bit.  One work
// item per face or per vertex, no LDS.  Every result is reproducible from run to run and independent of the order of
// the faces and of how the frames are split over launches: the normal sums are integers (rint(cross * 2^48)) added with
// 64-bit integer atomics, and each vertex's colour sums are float64 words that one thread alone updates, frame after
// frame in the order given.  All arithmetic is float64, one rounding per operation in the order written (no
// contraction); division and sqrt are correctly rounded.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/bnv_fusion.h"
#include "mesh_face.hpp"

namespace bnv {
namespace {

constexpr int kColorThreads = 256;
constexpr int kTotSlots = 64;                         // the exact area total is spread over this many words
constexpr double kNormalScale = 281474976710656.0;    // 2^48: |sum of rint(cross * 2^48)| < 2^61 below kAreaLimit

struct NormHdr {
  unsigned long long tot_hi[kTotSlots], tot_lo[kTotSlots];   // sums of q >> 31 and q & (2^31 - 1), q = rint(area 2^50)
  int32_t error, pad[3];
};

struct NormWs {
  NormHdr* hdr;
  unsigned long long* sums;   // [V, 3] int64 sums as their two's complement words
};

static size_t norm_ws_layout(int64_t V, char* base, NormWs* w) {
  Carver c(base);
  NormWs t;
  t.hdr = c.take<NormHdr>(1);
  t.sums = c.take<unsigned long long>(3 * V);
  if (w) *w = t;
  return c.bytes();
}

struct ColorWs {
  double* sums;     // [V, 4] sum_r, sum_g, sum_b, sum_w
  int32_t* count;   // [V] contributing frames
};

static size_t color_ws_layout(int64_t V, char* base, ColorWs* w) {
  Carver c(base);
  ColorWs t;
  t.sums = c.take<double>(4 * V);
  t.count = c.take<int32_t>(V);
  if (w) *w = t;
  return c.bytes();
}

// ---- vertex normals -------------------------------------------------------------------------------------------------
// one thread per face: the cross product as three integers into the sums of its three corners; the face's area in units
// of 2^-50 into the exact total (one atomic pair per wave, spread over kTotSlots words)
__global__ __launch_bounds__(kColorThreads) void k_vn_faces(const float* __restrict__ vin, int64_t V,
                                                            const int64_t* __restrict__ fin, int64_t T, NormWs w) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t q = 0;
  if (t < T) {
    int64_t c[3];
    const bool ok = load_face(fin, t, V, c);
    int32_t err = ok ? 0 : (int32_t)kErrFaceIndex;
    if (ok) {
      double cr[3];
      if (area_units(face_cross(vin, c, cr), q)) {   // (|cross| = 2 area < 2^13)
        const long long n[3] = {(long long)rint(__dmul_rn(cr[0], kNormalScale)),
                                (long long)rint(__dmul_rn(cr[1], kNormalScale)),
                                (long long)rint(__dmul_rn(cr[2], kNormalScale))};
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
          for (int a = 0; a < 3; ++a)
            if (n[a]) atomicAdd(&w.sums[c[k] * 3 + a], (unsigned long long)n[a]);
      } else {
        err |= kErrArea;
      }
    }
    if (err) atomicOr(&w.hdr->error, err);
  }
  unsigned long long hi, lo;
  wave_area_total(q, hi, lo);
  if ((threadIdx.x & 63) == 0 && (hi | lo)) {
    const int slot = (int)((blockIdx.x * (kColorThreads / 64) + (threadIdx.x >> 6)) % kTotSlots);
    atomicAdd(&w.hdr->tot_hi[slot], hi);
    atomicAdd(&w.hdr->tot_lo[slot], lo);
  }
}

// one thread per vertex: its sum as float64 (one rounding each), normalised; a zero sum gives (0, 0, 0)
__global__ __launch_bounds__(kColorThreads) void k_vn_normalize(const float* __restrict__ vin, int64_t V, NormWs w,
                                                                float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V) return;
  if (!(isfinite(vin[i * 3]) && isfinite(vin[i * 3 + 1]) && isfinite(vin[i * 3 + 2])))
    atomicOr(&w.hdr->error, (int32_t)kErrNonFinite);
  const long long sx = (long long)w.sums[i * 3], sy = (long long)w.sums[i * 3 + 1], sz = (long long)w.sums[i * 3 + 2];
  float nx = 0.0f, ny = 0.0f, nz = 0.0f;
  if (sx | sy | sz) {
    const double x = (double)sx, y = (double)sy, z = (double)sz;
    const double len = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y)), __dmul_rn(z, z)));
    nx = (float)__ddiv_rn(x, len);
    ny = (float)__ddiv_rn(y, len);
    nz = (float)__ddiv_rn(z, len);
  }
  out[i * 3] = nx;
  out[i * 3 + 1] = ny;
  out[i * 3 + 2] = nz;
}

__global__ void k_vn_status(NormWs w, int32_t* status) {
  unsigned long long hi = 0, lo = 0;
  for (int k = 0; k < kTotSlots; ++k) {
    hi += w.hdr->tot_hi[k];
    lo += w.hdr->tot_lo[k];
  }
  *status = (w.hdr->error || total_reaches_limit(hi, lo)) ? -1 : 0;
}

// ---- colours --------------------------------------------------------------------------------------------------------
struct ColorArgs {
  bnv_mesh_color_frame_t f[BNV_MESH_COLOR_MAX_FRAMES];
  int32_t shared[BNV_MESH_COLOR_MAX_FRAMES];   // the colour image has the depth image's size and intrinsics
  int32_t n_frames;
  double depth_tol, cos_min, near, max_depth;
};

__device__ __forceinline__ double color_depth(const bnv_mesh_color_frame_t& f, int y, int x) {
  const size_t i = (size_t)y * f.width + x;
  return f.depth_dtype == 0 ? __ddiv_rn((double)((const uint16_t*)f.depth)[i], 1000.0)
                            : (double)((const float*)f.depth)[i];
}

// u = (fx x) / z + cx; false unless 0 <= u <= n - 1 (NaN fails).  x0 = floor(u), x1 = min(x0 + 1, n - 1), fu = u - x0.
__device__ __forceinline__ bool color_project(double f, double c, double x, double z, int n, int& x0, int& x1,
                                              double& fu) {
  const double u = __dadd_rn(__ddiv_rn(__dmul_rn(f, x), z), c);
  if (!(u >= 0.0 && u <= (double)(n - 1))) return false;
  const double fl = floor(u);
  x0 = (int)fl;
  x1 = x0 + 1 < n ? x0 + 1 : n - 1;
  fu = __dsub_rn(u, fl);
  return true;
}

__global__ __launch_bounds__(kColorThreads) void k_color_accumulate(const float* __restrict__ vin,
                                                                    const float* __restrict__ nin, int64_t V,
                                                                    ColorWs w, ColorArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V) return;
  const double nx = (double)nin[i * 3], ny = (double)nin[i * 3 + 1], nz = (double)nin[i * 3 + 2];
  if (nx == 0.0 && ny == 0.0 && nz == 0.0) return;   // no normal: no view weight
  const double x0w = (double)vin[i * 3], x1w = (double)vin[i * 3 + 1], x2w = (double)vin[i * 3 + 2];
  double sr = w.sums[i * 4], sg = w.sums[i * 4 + 1], sb = w.sums[i * 4 + 2], sw = w.sums[i * 4 + 3];
  int32_t cnt = w.count[i];
  bool touched = false;
  for (int k = 0; k < a.n_frames; ++k) {   // (wave-uniform: the frame's words are scalar loads)
    const bnv_mesh_color_frame_t& f = a.f[k];
    // 1. camera point
    double p[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
      p[r] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(f.T_cw[4 * r], x0w), __dmul_rn(f.T_cw[4 * r + 1], x1w)),
                                 __dmul_rn(f.T_cw[4 * r + 2], x2w)),
                       f.T_cw[4 * r + 3]);
    if (!(p[2] > a.near && p[2] < a.max_depth)) continue;
    // 2. depth projection
    int xa, xb, ya, yb;
    double fu, fv;
    if (!color_project(f.K[0], f.K[2], p[0], p[2], f.width, xa, xb, fu)) continue;
    if (!color_project(f.K[1], f.K[3], p[1], p[2], f.height, ya, yb, fv)) continue;
    // 3. occlusion test: the bilinear neighbours that see this surface
    const double gu = __dsub_rn(1.0, fu), gv = __dsub_rn(1.0, fv);
    double bw[4] = {__dmul_rn(gu, gv), __dmul_rn(fu, gv), __dmul_rn(gu, fv), __dmul_rn(fu, fv)};
    const int cy[4] = {ya, ya, yb, yb}, cx[4] = {xa, xb, xa, xb};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const double d = color_depth(f, cy[c], cx[c]);
      bool pass = isfinite(d) && d > 0.0 && d < a.max_depth && fabs(__dsub_rn(d, p[2])) <= a.depth_tol;
      if (pass && f.conf) pass = (int)f.conf[(size_t)cy[c] * f.width + cx[c]] >= f.conf_level;
      if (!pass) bw[c] = 0.0;
    }
    const double wsum = __dadd_rn(__dadd_rn(__dadd_rn(bw[0], bw[1]), bw[2]), bw[3]);
    if (!(wsum > 0.0)) continue;
    // 4. view weight
    const double dx = __dsub_rn(f.center[0], x0w), dy = __dsub_rn(f.center[1], x1w), dz = __dsub_rn(f.center[2], x2w);
    const double len = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)));
    const double cosv =
        __ddiv_rn(__dadd_rn(__dadd_rn(__dmul_rn(nx, dx), __dmul_rn(ny, dy)), __dmul_rn(nz, dz)), len);
    if (!(cosv > a.cos_min)) continue;
    const double wt = __ddiv_rn(cosv, __dmul_rn(p[2], p[2]));
    // 5. colour sample
    int W_c = f.width;
    if (a.shared[k]) {
#pragma unroll
      for (int c = 0; c < 4; ++c) bw[c] = __ddiv_rn(bw[c], wsum);
    } else {
      W_c = f.color_width;
      if (!color_project(f.K_color[0], f.K_color[2], p[0], p[2], f.color_width, xa, xb, fu)) continue;
      if (!color_project(f.K_color[1], f.K_color[3], p[1], p[2], f.color_height, ya, yb, fv)) continue;
      const double hu = __dsub_rn(1.0, fu), hv = __dsub_rn(1.0, fv);
      bw[0] = __dmul_rn(hu, hv);
      bw[1] = __dmul_rn(fu, hv);
      bw[2] = __dmul_rn(hu, fv);
      bw[3] = __dmul_rn(fu, fv);
    }
    const uint8_t* q00 = f.rgb + ((size_t)ya * W_c + xa) * 3;
    const uint8_t* q01 = f.rgb + ((size_t)ya * W_c + xb) * 3;
    const uint8_t* q10 = f.rgb + ((size_t)yb * W_c + xa) * 3;
    const uint8_t* q11 = f.rgb + ((size_t)yb * W_c + xb) * 3;
    double col[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
      col[ch] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(bw[0], (double)q00[ch]), __dmul_rn(bw[1], (double)q01[ch])),
                                    __dmul_rn(bw[2], (double)q10[ch])),
                          __dmul_rn(bw[3], (double)q11[ch]));
    sr = __dadd_rn(sr, __dmul_rn(wt, col[0]));
    sg = __dadd_rn(sg, __dmul_rn(wt, col[1]));
    sb = __dadd_rn(sb, __dmul_rn(wt, col[2]));
    sw = __dadd_rn(sw, wt);
    cnt += 1;
    touched = true;
  }
  if (touched) {
    w.sums[i * 4] = sr;
    w.sums[i * 4 + 1] = sg;
    w.sums[i * 4 + 2] = sb;
    w.sums[i * 4 + 3] = sw;
    w.count[i] = cnt;
  }
}

struct Fill {
  uint8_t c[3];
};

__global__ __launch_bounds__(kColorThreads) void k_color_resolve(int64_t V, ColorWs w, Fill fill,
                                                                 uint8_t* __restrict__ colors,
                                                                 uint8_t* __restrict__ observed,
                                                                 double* __restrict__ sum_w_out,
                                                                 int32_t* __restrict__ count_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V) return;
  const int32_t cnt = w.count[i];
  const double sw = w.sums[i * 4 + 3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    uint8_t o = fill.c[ch];
    if (cnt > 0) {
      const double m = rint(__ddiv_rn(w.sums[i * 4 + ch], sw));   // half to even
      o = (uint8_t)(m >= 255.0 ? 255 : (m > 0.0 ? (int)m : 0));
    }
    colors[i * 3 + ch] = o;
  }
  observed[i] = cnt > 0;
  if (sum_w_out) sum_w_out[i] = sw;
  if (count_out) count_out[i] = cnt;
}

static bool color_sizes_ok(int64_t V) { return V > 0 && V <= INT32_MAX - 1; }

}  // namespace
}  // namespace bnv

using namespace bnv;

extern "C" {

int bnv_mesh_normals_workspace_bytes(int64_t n_vertices, int64_t* bytes) {
  if (!bytes || !color_sizes_ok(n_vertices)) return BNV_ERR_INVALID_ARGUMENT;
  *bytes = (int64_t)norm_ws_layout(n_vertices, nullptr, nullptr);
  return BNV_OK;
}

int bnv_mesh_vertex_normals(const float* vertices, int64_t n_vertices, const int64_t* faces, int64_t n_faces,
                            void* workspace, int64_t ws_bytes, float* normals_out, int32_t* status,
                            bnv_stream_t stream) {
  const int64_t V = n_vertices, T = n_faces;
  if (!vertices || !normals_out || !status || !color_sizes_ok(V) || T < 0 || T > INT32_MAX - 1 || (T && !faces))
    return BNV_ERR_INVALID_ARGUMENT;
  NormWs w;
  const size_t bytes = norm_ws_layout(V, (char*)workspace, &w);
  if (!workspace || ws_bytes < (int64_t)bytes) return BNV_ERR_WORKSPACE_TOO_SMALL;
  hipStream_t s = (hipStream_t)stream;
  BNV_HIP_CHECK(hipMemsetAsync(workspace, 0, bytes, s));
  if (T) k_vn_faces<<<blocks_for(T, kColorThreads), kColorThreads, 0, s>>>(vertices, V, faces, T, w);
  k_vn_normalize<<<blocks_for(V, kColorThreads), kColorThreads, 0, s>>>(vertices, V, w, normals_out);
  k_vn_status<<<1, 1, 0, s>>>(w, status);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

int bnv_mesh_color_workspace_bytes(int64_t n_vertices, int64_t* bytes) {
  if (!bytes || !color_sizes_ok(n_vertices)) return BNV_ERR_INVALID_ARGUMENT;
  *bytes = (int64_t)color_ws_layout(n_vertices, nullptr, nullptr);
  return BNV_OK;
}

int bnv_mesh_color_begin(void* workspace, int64_t ws_bytes, int64_t n_vertices, bnv_stream_t stream) {
  if (!color_sizes_ok(n_vertices)) return BNV_ERR_INVALID_ARGUMENT;
  const size_t bytes = color_ws_layout(n_vertices, nullptr, nullptr);
  if (!workspace || ws_bytes < (int64_t)bytes) return BNV_ERR_WORKSPACE_TOO_SMALL;
  BNV_HIP_CHECK(hipMemsetAsync(workspace, 0, bytes, (hipStream_t)stream));
  return BNV_OK;
}

int bnv_mesh_color_accumulate(const float* vertices, const float* normals, int64_t n_vertices,
                              const bnv_mesh_color_frame_t* frames_host, int32_t n_frames, double depth_tol,
                              double cos_min, double near, double max_depth, void* workspace, int64_t ws_bytes,
                              bnv_stream_t stream) {
  const int64_t V = n_vertices;
  if (!vertices || !normals || !frames_host || !color_sizes_ok(V) || n_frames < 1 ||
      n_frames > BNV_MESH_COLOR_MAX_FRAMES)
    return BNV_ERR_INVALID_ARGUMENT;
  if (!(std::isfinite(depth_tol) && depth_tol >= 0.0 && cos_min >= 0.0 && cos_min < 1.0 && std::isfinite(near) &&
        near >= 0.0 && std::isfinite(max_depth) && max_depth > near))
    return BNV_ERR_INVALID_ARGUMENT;
  ColorArgs a{};
  for (int k = 0; k < n_frames; ++k) {
    const bnv_mesh_color_frame_t& f = frames_host[k];
    if (!f.depth || !f.rgb || f.depth_dtype < 0 || f.depth_dtype > 1 || f.height <= 0 || f.width <= 0 ||
        f.color_height <= 0 || f.color_width <= 0 || f.height > 32768 || f.width > 32768 || f.color_height > 32768 ||
        f.color_width > 32768 || f.conf_level < 0 || (!f.conf && f.conf_level != 0))
      return BNV_ERR_INVALID_ARGUMENT;
    if (!all_finite(f.K, 4) || !all_finite(f.K_color, 4) || !all_finite(f.T_cw, 12) || !all_finite(f.center, 3))
      return BNV_ERR_INVALID_ARGUMENT;
    a.f[k] = f;
    a.shared[k] = f.color_height == f.height && f.color_width == f.width && f.K_color[0] == f.K[0] &&
                  f.K_color[1] == f.K[1] && f.K_color[2] == f.K[2] && f.K_color[3] == f.K[3];
  }
  ColorWs w;
  if (!workspace || ws_bytes < (int64_t)color_ws_layout(V, (char*)workspace, &w)) return BNV_ERR_WORKSPACE_TOO_SMALL;
  a.n_frames = n_frames;
  a.depth_tol = depth_tol;
  a.cos_min = cos_min;
  a.near = near;
  a.max_depth = max_depth;
  hipLaunchKernelGGL(k_color_accumulate, dim3(blocks_for(V, kColorThreads)), dim3(kColorThreads), 0, (hipStream_t)stream, vertices,
                     normals, V, w, a);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

int bnv_mesh_color_resolve(const void* workspace, int64_t ws_bytes, int64_t n_vertices, const uint8_t fill[3],
                           uint8_t* colors_out, uint8_t* observed_out, double* sum_w_out, int32_t* count_out,
                           bnv_stream_t stream) {
  const int64_t V = n_vertices;
  if (!fill || !colors_out || !observed_out || !color_sizes_ok(V)) return BNV_ERR_INVALID_ARGUMENT;
  ColorWs w;
  if (!workspace || ws_bytes < (int64_t)color_ws_layout(V, (char*)const_cast<void*>(workspace), &w))
    return BNV_ERR_WORKSPACE_TOO_SMALL;
  const Fill fl{{fill[0], fill[1], fill[2]}};
  hipLaunchKernelGGL(k_color_resolve, dim3(blocks_for(V, kColorThreads)), dim3(kColorThreads), 0, (hipStream_t)stream, V, w, fl,
                     colors_out, observed_out, sum_w_out, count_out);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

}  // extern "C"
