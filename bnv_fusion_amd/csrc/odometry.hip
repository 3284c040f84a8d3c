// Frame-to-frame RGB-D odometry: joint photometric and depth alignment of two consecutive frames.
// Semantics: include/bnv_fusion.h, "Odometry"; restated in float64 numpy by tests/odometry_restatement.py.
//
// A frame is prepared once (bnv_rgbd_prepare) into a pyramid in a caller-owned buffer and aligned twice: as the current
// frame of one pair and as the reference of the next.
//   k_rgbd_intensity  level 0: depth in metres (0 = invalid) and the colour image's luma on the depth image's grid.
//   k_rgbd_level      level l + 1 from level l: edge-aware 2 x 2 means.
//   k_rgbd_gradients  central differences of intensity and depth and the gradient-valid flag of one level.
//   k_rgbd_accumulate the hot path, in the shape of k_icp_accumulate (track.hip): a fixed grid of kBlocks x 256 threads,
//                     thread g takes the level's reference pixels g, g + G, ... into 29 float64 registers; two rows per
//                     pair (intensity, depth); icp_block_reduce; k_icp_solve (icp_solve.hpp) follows.
//
// Layout.  A level is an array of pixel records, float32 [H_l][W_l][8] = D, I, I_x, I_y, D_x, D_y, valid (1 or 0), 0:
// the six planes of a pixel interleaved and padded to 32 bytes.  A pair reads all six planes (and the flag) of the four
// pixels around its projection: as separate planes those are 6 planes x 2 rows = 12 cache lines or more; as records
// the two pixels of a row are 64 contiguous bytes, 32-byte aligned, so the four corners touch two lines (four when a
// row's pair straddles a 128-byte line) and every corner is two 16-byte loads.  The reference pixel reads the first
// half of its record (D, I), consecutive lanes consecutive records.  Levels follow each other in the buffer, each on a
// 256-byte boundary (workspace.hpp).
// float64 arithmetic throughout, one rounding per operation (-ffp-contract=off); what is stored is rounded to float32
// once.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/bnv_fusion.h"
#include "bnv_common.hpp"
#include "icp_solve.hpp"
#include "workspace.hpp"

namespace bnv {
namespace {

constexpr int kRec = 8;   // floats per pixel record

struct RgbdImage {   // what k_rgbd_intensity reads
  const void* depth;
  int dtype;         // 0: uint16 millimetres, 1: float32 metres
  int H, W;
  double fx, fy, cx, cy, max_depth;
  const uint8_t* rgb;   // [Hc, Wc, 3] or null
  int Hc, Wc;
  double fxc, fyc, cxc, cyc;
};

struct RgbdPair {    // one level of a pair; does not change over the level's iterations
  const float* ref;
  const float* cur;
  int H, W;
  double fx, fy, cx, cy;
  double s_int, s_depth;   // sqrt(1 - lambda), sqrt(lambda)
  double dist, depth_jump;   // depth_jump: the level's, 2^l times the call's
};

__device__ __forceinline__ double luma(const uint8_t* __restrict__ rgb, int64_t at) {
  return (0.299 * (double)rgb[at * 3] + 0.587 * (double)rgb[at * 3 + 1]) + 0.114 * (double)rgb[at * 3 + 2];
}

// first / one-past-last colour pixel whose centre lies in [p - 0.5, p + 0.5) of depth pixel p along one axis, clamped
// to the colour image, and the centre's colour coordinate
__device__ __forceinline__ void footprint(int p, double f, double c, double fc, double cc, int nc, int& first,
                                          int& last, double& mid) {
  const double lo = fc * ((((double)p - 0.5) - c) / f) + cc;
  const double hi = fc * ((((double)p + 0.5) - c) / f) + cc;
  mid = fc * (((double)p - c) / f) + cc;
  const double a = fmin(fmax(ceil(lo), 0.0), (double)nc), b = fmax(fmin(ceil(hi), (double)nc), a);
  first = (int)a;
  last = (int)b;
}

__device__ __forceinline__ void bilinear_axis(double mid, int nc, int& i0, int& i1, double& w) {
  const double x = fmin(fmax(mid, 0.0), (double)(nc - 1));
  const double f = fmin(floor(x), (double)(nc > 2 ? nc - 2 : 0));
  w = x - f;
  i0 = (int)f;
  i1 = i0 + 1 < nc - 1 ? i0 + 1 : nc - 1;
}

__global__ __launch_bounds__(256) void k_rgbd_intensity(RgbdImage f, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)f.H * f.W) return;
  const int v = (int)(i / f.W), u = (int)(i % f.W);
  const double d = f.dtype == 0 ? (double)((const uint16_t*)f.depth)[i] / 1000.0 : (double)((const float*)f.depth)[i];
  const bool ok = d > 0.0 && d <= f.max_depth && isfinite(d);
  double y = 0.0;
  if (f.rgb) {
    int j0, j1, i0, i1;
    double xm, ym;
    footprint(u, f.fx, f.cx, f.fxc, f.cxc, f.Wc, j0, j1, xm);
    footprint(v, f.fy, f.cy, f.fyc, f.cyc, f.Hc, i0, i1, ym);
    if (j1 > j0 && i1 > i0) {
      double acc = 0.0;
      for (int r = i0; r < i1; ++r)
        for (int c = j0; c < j1; ++c) acc = acc + luma(f.rgb, (int64_t)r * f.Wc + c);
      y = acc / ((double)(i1 - i0) * (double)(j1 - j0));
    } else {
      int bx0, bx1, by0, by1;
      double ax, ay;
      bilinear_axis(xm, f.Wc, bx0, bx1, ax);
      bilinear_axis(ym, f.Hc, by0, by1, ay);
      const double y00 = luma(f.rgb, (int64_t)by0 * f.Wc + bx0), y01 = luma(f.rgb, (int64_t)by0 * f.Wc + bx1);
      const double y10 = luma(f.rgb, (int64_t)by1 * f.Wc + bx0), y11 = luma(f.rgb, (int64_t)by1 * f.Wc + bx1);
      const double top = y00 + ax * (y01 - y00), bot = y10 + ax * (y11 - y10);
      y = top + ay * (bot - top);
    }
    y = y / 255.0;
  }
  out[i * kRec] = ok ? (float)d : 0.0f;
  out[i * kRec + 1] = (float)y;
}

// level l + 1 [Hn, Wn] from level l [H, W]; Hn = H / 2, Wn = W / 2
__global__ __launch_bounds__(256) void k_rgbd_level(const float* __restrict__ in, int W, int Hn, int Wn,
                                                    double depth_jump, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)Hn * Wn) return;
  const int v = (int)(i / Wn), u = (int)(i % Wn);
  double d[4], y[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t at = ((int64_t)(2 * v + (k >> 1)) * W + (2 * u + (k & 1))) * kRec;
    d[k] = (double)in[at];
    y[k] = (double)in[at + 1];
  }
  double dmin = INFINITY;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (d[k] > 0.0 && d[k] < dmin) dmin = d[k];
  double sd = 0.0, sy = 0.0, n = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (d[k] > 0.0 && d[k] - dmin <= depth_jump) {
      sd = sd + d[k];
      sy = sy + y[k];
      n = n + 1.0;
    }
  out[i * kRec] = n > 0.0 ? (float)(sd / n) : 0.0f;
  out[i * kRec + 1] = n > 0.0 ? (float)(sy / n) : 0.0f;
}

// fills slots 2 .. 7 of every record of one level
__global__ __launch_bounds__(256) void k_rgbd_gradients(float* __restrict__ lev, int H, int W, double depth_jump) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)H * W) return;
  const int v = (int)(i / W), u = (int)(i % W);
  float g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  bool ok = false;
  if (u >= 1 && u <= W - 2 && v >= 1 && v <= H - 2) {
    const double c = (double)lev[i * kRec];
    const int64_t nb[4] = {i - 1, i + 1, i - W, i + W};   // left, right, up, down
    double d[4], y[4];
    ok = c > 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      d[k] = (double)lev[nb[k] * kRec];
      y[k] = (double)lev[nb[k] * kRec + 1];
      ok = ok && d[k] > 0.0 && fabs(d[k] - c) <= depth_jump;
    }
    if (ok) {
      g[0] = (float)((y[1] - y[0]) / 2.0);
      g[1] = (float)((y[3] - y[2]) / 2.0);
      g[2] = (float)((d[1] - d[0]) / 2.0);
      g[3] = (float)((d[3] - d[2]) / 2.0);
    }
  }
  float* o = lev + i * kRec;
  o[2] = g[0];
  o[3] = g[1];
  o[4] = g[2];
  o[5] = g[3];
  o[6] = ok ? 1.0f : 0.0f;
  o[7] = 0.0f;
}

// the scaled row of image gradient (a, b), z-term c: J[6]
__device__ __forceinline__ void rgbd_row(double a, double b, double c, double s, const RgbdPair& f, const double (&Q)[3],
                                         double (&J)[6]) {
  a = s * a;
  b = s * b;
  c = s * c;
  const double gx = (a * f.fx) / Q[2], gy = (b * f.fy) / Q[2];
  const double gz = (0.0 - (gx * Q[0] + gy * Q[1]) / Q[2]) - c;
  J[0] = Q[1] * gz - Q[2] * gy;
  J[1] = Q[2] * gx - Q[0] * gz;
  J[2] = Q[0] * gy - Q[1] * gx;
  J[3] = gx;
  J[4] = gy;
  J[5] = gz;
}

__global__ __launch_bounds__(kThreads) void k_rgbd_accumulate(RgbdPair f, const double* __restrict__ pose,
                                                              const int32_t* __restrict__ status,
                                                              double* __restrict__ partials) {
  if (*status != BNV_ICP_OK) return;
  double T[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) T[i] = pose[i];
  double S[kSums];
#pragma unroll
  for (int i = 0; i < kSums; ++i) S[i] = 0.0;
  const int64_t n_pixels = (int64_t)f.H * f.W;
  const f32x4* __restrict__ ref = (const f32x4*)f.ref;
  const f32x4* __restrict__ cur = (const f32x4*)f.cur;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_pixels; i += (int64_t)kBlocks * kThreads) {
    const f32x4 p = ref[i * 2];
    const double z = (double)p[0];
    if (!(z > 0.0)) continue;
    const int v = (int)(i / f.W), u = (int)(i % f.W);
    const double x = ((double)u - f.cx) / f.fx, y = ((double)v - f.cy) / f.fy;
    const double P[3] = {x * z, y * z, z};
    double Q[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) Q[a] = ((T[a * 4] * P[0] + T[a * 4 + 1] * P[1]) + T[a * 4 + 2] * P[2]) + T[a * 4 + 3];
    if (!(Q[2] > 0.0)) continue;
    const double xq = f.fx * Q[0] / Q[2] + f.cx, yq = f.fy * Q[1] / Q[2] + f.cy;
    const double x0 = floor(xq), y0 = floor(yq);
    if (!(x0 >= 0.0 && x0 <= (double)(f.W - 2) && y0 >= 0.0 && y0 <= (double)(f.H - 2))) continue;   // (NaN too)
    const double ax = xq - x0, ay = yq - y0;
    const int64_t at = (int64_t)y0 * f.W + (int64_t)x0;
    const int64_t corner[4] = {at, at + 1, at + f.W, at + f.W + 1};
    double c[4][6];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const f32x4 lo = cur[corner[k] * 2], hi = cur[corner[k] * 2 + 1];
      c[k][0] = (double)lo[1];   // I
      c[k][1] = (double)lo[0];   // D
      c[k][2] = (double)lo[2];   // I_x
      c[k][3] = (double)lo[3];   // I_y
      c[k][4] = (double)hi[0];   // D_x
      c[k][5] = (double)hi[1];   // D_y
      ok = ok && hi[2] != 0.0f;
    }
    if (!ok) continue;
    const double dmax = fmax(fmax(c[0][1], c[1][1]), fmax(c[2][1], c[3][1]));
    const double dmin = fmin(fmin(c[0][1], c[1][1]), fmin(c[2][1], c[3][1]));
    if (!(dmax - dmin <= f.depth_jump)) continue;
    double s[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double top = c[0][k] + ax * (c[1][k] - c[0][k]), bot = c[2][k] + ax * (c[3][k] - c[2][k]);
      s[k] = top + ay * (bot - top);
    }
    const double rd = Q[2] - s[1];
    if (!(fabs(rd) <= f.dist)) continue;
    double J[6];
    rgbd_row(s[2], s[3], 0.0, f.s_int, f, Q, J);
    icp_add_row(S, J, f.s_int * ((double)p[1] - s[0]));
    rgbd_row(s[4], s[5], 1.0, f.s_depth, f, Q, J);
    icp_add_row(S, J, f.s_depth * rd);
    S[28] += 1.0;
  }
  icp_block_reduce(S, partials);
}

// the pyramid's sizes, or false when (H, W, levels) is not one
bool pyramid_ok(int32_t H, int32_t W, int32_t levels) {
  return H >= 1 && W >= 1 && H <= 32768 && W <= 32768 && levels >= 1 && levels <= kMaxLevels &&
         (H >> (levels - 1)) >= 1 && (W >> (levels - 1)) >= 1;
}

// a prepared frame: level l at out[l], [H >> l][W >> l][8] float32
size_t frame_layout(const void* base, int32_t H, int32_t W, int32_t levels, float** out) {
  Carver cv(base);
  for (int l = 0; l < levels; ++l) {
    float* p = cv.take<float>((size_t)(H >> l) * (size_t)(W >> l) * kRec);
    if (out) out[l] = p;
  }
  return cv.bytes();
}

bool intrinsics_ok(const double* K) { return K && all_finite(K, 9) && K[0] != 0.0 && K[4] != 0.0; }

inline int blocks_of(int64_t n) { return (int)((n + 255) / 256); }

}  // namespace
}  // namespace bnv

using namespace bnv;

extern "C" {

size_t bnv_rgbd_frame_bytes(int32_t H, int32_t W, int32_t levels) {
  return pyramid_ok(H, W, levels) ? frame_layout(nullptr, H, W, levels, nullptr) : 0;
}

size_t bnv_rgbd_align_bytes(int32_t n_steps, const int32_t* schedule_host) {
  const int64_t n_iter = schedule_iterations(n_steps, schedule_host, 0);
  return n_iter < 0 ? 0 : icp_workspace_bytes(n_iter);
}

int bnv_rgbd_prepare(const void* depth, int depth_dtype, int32_t H, int32_t W, const double K_host[9],
                     const uint8_t* rgb, int32_t H_c, int32_t W_c, const double K_c_host[9], int32_t levels,
                     double max_depth, double depth_jump, void* frame, size_t frame_bytes, bnv_stream_t stream) {
  if (!depth || !frame || !intrinsics_ok(K_host)) return BNV_ERR_INVALID_ARGUMENT;
  if (depth_dtype != 0 && depth_dtype != 1) return BNV_ERR_INVALID_ARGUMENT;
  if (!pyramid_ok(H, W, levels)) return BNV_ERR_INVALID_ARGUMENT;
  if (rgb && (H_c < 1 || W_c < 1 || H_c > 32768 || W_c > 32768 || !intrinsics_ok(K_c_host)))
    return BNV_ERR_INVALID_ARGUMENT;
  if (!(max_depth > 0.0) || !(depth_jump > 0.0) || !std::isfinite(max_depth) || !std::isfinite(depth_jump))
    return BNV_ERR_INVALID_ARGUMENT;
  if (frame_bytes < bnv_rgbd_frame_bytes(H, W, levels)) return BNV_ERR_WORKSPACE_TOO_SMALL;

  float* lev[kMaxLevels];
  frame_layout(frame, H, W, levels, lev);
  RgbdImage f;
  f.depth = depth;
  f.dtype = depth_dtype;
  f.H = H;
  f.W = W;
  f.fx = K_host[0];
  f.fy = K_host[4];
  f.cx = K_host[2];
  f.cy = K_host[5];
  f.max_depth = max_depth;
  f.rgb = rgb;
  f.Hc = rgb ? H_c : 0;
  f.Wc = rgb ? W_c : 0;
  f.fxc = rgb ? K_c_host[0] : 1.0;
  f.fyc = rgb ? K_c_host[4] : 1.0;
  f.cxc = rgb ? K_c_host[2] : 0.0;
  f.cyc = rgb ? K_c_host[5] : 0.0;
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_rgbd_intensity, dim3(blocks_of((int64_t)H * W)), dim3(256), 0, s, f, lev[0]);
  BNV_LAUNCH_CHECK();
  for (int l = 0; l < levels; ++l) {
    const int Hl = H >> l, Wl = W >> l;
    const double jump = depth_jump * (double)(1 << l);   // the level's pixels are 2^l as wide
    if (l) {
      hipLaunchKernelGGL(k_rgbd_level, dim3(blocks_of((int64_t)Hl * Wl)), dim3(256), 0, s, (const float*)lev[l - 1],
                         W >> (l - 1), Hl, Wl, jump, lev[l]);
      BNV_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_rgbd_gradients, dim3(blocks_of((int64_t)Hl * Wl)), dim3(256), 0, s, lev[l], Hl, Wl, jump);
    BNV_LAUNCH_CHECK();
  }
  return BNV_OK;
}

int bnv_rgbd_align(const void* ref_frame, const void* cur_frame, int32_t H, int32_t W, int32_t levels,
                   const double K_host[9], const double T_guess_host[16], int32_t n_steps,
                   const int32_t* schedule_host, double lambda_depth, double dist, double depth_jump,
                   double min_pair_share, double min_spread, void* workspace, size_t ws_bytes, double* pose_out,
                   double* poses_out, double* stats_out, int32_t* status_out, bnv_stream_t stream) {
  if (!ref_frame || !cur_frame || !T_guess_host || !schedule_host || !workspace || !pose_out || !stats_out ||
      !status_out || !intrinsics_ok(K_host))
    return BNV_ERR_INVALID_ARGUMENT;
  if (!pyramid_ok(H, W, levels)) return BNV_ERR_INVALID_ARGUMENT;
  const int64_t n_iter = schedule_iterations(n_steps, schedule_host, 0);
  if (n_iter < 0) return BNV_ERR_INVALID_ARGUMENT;
  for (int l = 0; l < n_steps; ++l)
    if (schedule_host[l * 2] >= levels) return BNV_ERR_INVALID_ARGUMENT;
  if (!all_finite(T_guess_host, 16)) return BNV_ERR_INVALID_ARGUMENT;
  if (!(lambda_depth >= 0.0 && lambda_depth <= 1.0) || !(dist > 0.0) || !(depth_jump > 0.0) ||
      !(min_pair_share >= 0.0) || !(min_spread >= 0.0) || !std::isfinite(dist) || !std::isfinite(depth_jump) ||
      !std::isfinite(min_pair_share) || !std::isfinite(min_spread))
    return BNV_ERR_INVALID_ARGUMENT;
  if (ws_bytes < icp_workspace_bytes(n_iter)) return BNV_ERR_WORKSPACE_TOO_SMALL;

  float *ref[kMaxLevels], *cur[kMaxLevels];
  frame_layout(ref_frame, H, W, levels, ref);
  frame_layout(cur_frame, H, W, levels, cur);
  double* partials = (double*)workspace;
  double* records = partials + (size_t)kBlocks * kSums;
  const hipStream_t s = (hipStream_t)stream;

  IcpInit init;
  for (int i = 0; i < 16; ++i) init.T0[i] = T_guess_host[i];
  init.n_iter = (int)n_iter;
  hipLaunchKernelGGL(k_icp_init, dim3(1), dim3(64), 0, s, init, pose_out, poses_out, stats_out, records, status_out);
  BNV_LAUNCH_CHECK();
  IcpSolve sol;
  for (int i = 0; i < 16; ++i) sol.T0[i] = T_guess_host[i];
  sol.min_spread = min_spread;
  sol.max_w = BNV_ICP_MAX_ROTATION;
  sol.max_v = BNV_ICP_MAX_TRANSLATION;
  sol.clamp = 0;
  sol.n_iter = (int)n_iter;
  RgbdPair f;
  f.s_int = sqrt(1.0 - lambda_depth);
  f.s_depth = sqrt(lambda_depth);
  f.dist = dist;
  int iter = 0;
  for (int l = 0; l < n_steps; ++l) {
    const int level = schedule_host[l * 2];
    const double scale = (double)(1 << level);
    f.ref = ref[level];
    f.cur = cur[level];
    f.H = H >> level;
    f.W = W >> level;
    f.fx = K_host[0] / scale;
    f.fy = K_host[4] / scale;
    f.cx = (K_host[2] + 0.5) / scale - 0.5;
    f.cy = (K_host[5] + 0.5) / scale - 0.5;
    f.depth_jump = depth_jump * scale;
    sol.min_pairs = min_pair_share * (double)((int64_t)f.H * f.W);
    for (int k = 0; k < schedule_host[l * 2 + 1]; ++k, ++iter) {
      hipLaunchKernelGGL(k_rgbd_accumulate, dim3(kBlocks), dim3(kThreads), 0, s, f, (const double*)pose_out,
                         (const int32_t*)status_out, partials);
      BNV_LAUNCH_CHECK();
      sol.iter = iter;
      hipLaunchKernelGGL(k_icp_solve, dim3(1), dim3(64), 0, s, sol, (const double*)partials, pose_out, poses_out,
                         stats_out, records, status_out);
      BNV_LAUNCH_CHECK();
    }
  }
  return BNV_OK;
}

}  // extern "C"
