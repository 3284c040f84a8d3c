// depth_filter.hip -- edge-preserving smoothing of a depth image in front of the front end and the tracker
// (bnv_depth_filter; include/bnv_fusion.h, "Depth filter").  Sensor depth is disparity-quantised: one step is
// z^2 / (8 * 35.130) in the reference's Kinect model (src/utils/geometry.py:54-69), 3.6 mm at 1 m and 32 mm at 3 m, and
// the 3x3 Sobel of frontend.hpp turns that staircase into poor normals.  The filter is a bilateral filter whose two
// kernels are Tukey biweights (1 - u^2)^2 instead of Gaussians: no transcendental function, so with float64
// arithmetic in a fixed tap order (compiled with -ffp-contract=off) tests/depth_filter_restatement.py matches it bit
// for bit.  The range width grows with z^2, as the sensor's noise does.
//
// One thread per output pixel, 32 x 8 pixel tiles: a wave is two rows of 32 pixels, so every tap is one ds_read_b64
// of 32 consecutive doubles per half wave -- no bank conflict at any radius or row pitch.  The tile's depth values,
// converted to metres and with validity folded in (0 = not a sample), sit in LDS with a halo of `radius`; pixels
// outside the image are 0 there, which is "no padding".  The spatial weights come with the kernel arguments (the
// index is wave-uniform: scalar loads).  One reciprocal per pixel, no division per tap.
#include "frontend.hpp"

#include <cmath>

namespace bnv {

constexpr int kDfTileW = 32;
constexpr int kDfTileH = 8;
constexpr int kDfThreads = kDfTileW * kDfTileH;
constexpr int kDfMaxRadius = 8;                    // BNV_DEPTH_FILTER_MAX_RADIUS
constexpr int kDfMaxTaps = (2 * kDfMaxRadius + 1) * (2 * kDfMaxRadius + 1);
constexpr int kDfLdsDoubles = (kDfTileW + 2 * kDfMaxRadius) * (kDfTileH + 2 * kDfMaxRadius);   // 9216 bytes

struct DepthFilterArgs {
  FrontArgs front;        // depth, dtype, H, W, max_depth, conf, conf_level: what depth_at / conf_ok read
  int r;
  double sigma_depth, range_cut;
  float* out;
  double wa[kDfMaxTaps];  // [(2r + 1), (2r + 1)] row-major; 0 where the tap is skipped (a <= 0)
};

__global__ __launch_bounds__(kDfThreads) void k_depth_filter(DepthFilterArgs p) {
  __shared__ double tile[kDfLdsDoubles];
  const FrontArgs& a = p.front;
  const int r = p.r;
  const int lw = kDfTileW + 2 * r, lh = kDfTileH + 2 * r;
  const int x0 = (int)blockIdx.x * kDfTileW, y0 = (int)blockIdx.y * kDfTileH;
  for (int i = (int)threadIdx.x; i < lw * lh; i += kDfThreads) {
    const int ly = i / lw, lx = i - ly * lw;
    const int gy = y0 - r + ly, gx = x0 - r + lx;
    double z = 0.0;
    if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
      z = depth_at(a, gy, gx);
      if (!conf_ok(a, (int64_t)gy * a.W + gx)) z = 0.0;
    }
    tile[i] = z;
  }
  __syncthreads();
  const int tx = (int)threadIdx.x % kDfTileW, ty = (int)threadIdx.x / kDfTileW;
  const int x = x0 + tx, y = y0 + ty;
  if (x >= a.W || y >= a.H) return;
  const double* centre = tile + (ty + r) * lw + (tx + r);
  const double zp = *centre;
  float o = 0.0f;
  if (zp > 0.0) {
    const double s = p.sigma_depth * zp * zp;
    const double c = p.range_cut * s;
    const double ic = 1.0 / c;
    double num = 0.0, den = 0.0;
    const int n = 2 * r + 1;
    for (int dy = -r; dy <= r; ++dy) {
      const double* row = centre + dy * lw;
      for (int dx = -r; dx <= r; ++dx) {
        const double wa = p.wa[(dy + r) * n + (dx + r)];
        if (wa == 0.0) continue;                   // (wave-uniform)
        const double zq = row[dx];
        const double diff = zq - zp;
        if (zq > 0.0 && fabs(diff) < c) {
          const double t = diff * ic;
          const double b = 1.0 - t * t;
          const double w = wa * (b * b);
          num += w * zq;
          den += w;
        }
      }
    }
    o = (float)(num / den);
  }
  p.out[(size_t)y * a.W + x] = o;
}

}  // namespace bnv

using namespace bnv;

extern "C" int bnv_depth_filter(const void* depth, int depth_dtype, int H, int W, double max_depth, int radius,
                                double sigma_depth, double range_cut, const uint8_t* conf, int conf_level, float* out,
                                bnv_stream_t stream_) {
  if (!depth || !out || H <= 0 || W <= 0 || depth_dtype < 0 || depth_dtype > 2 || H > 32768 || W > 32768 ||
      radius < 1 || radius > kDfMaxRadius || !front_conf_args_ok(conf, conf_level))
    return BNV_ERR_INVALID_ARGUMENT;
  if (!(std::isfinite(max_depth) && max_depth > 0.0 && std::isfinite(sigma_depth) && sigma_depth > 0.0 &&
        std::isfinite(range_cut) && range_cut > 0.0))
    return BNV_ERR_INVALID_ARGUMENT;
  // the kernel reads a halo: it cannot run in place, on any overlap of the two images
  const size_t n = (size_t)H * W, in_bytes = n * (depth_dtype == 0 ? 2 : depth_dtype == 1 ? 4 : 8);
  const uintptr_t d0 = (uintptr_t)depth, o0 = (uintptr_t)out;
  if (d0 < o0 + n * 4 && o0 < d0 + in_bytes) return BNV_ERR_INVALID_ARGUMENT;
  DepthFilterArgs p{};    // (everything the filter does not use, the weights of skipped taps included, stays 0)
  p.front.depth = depth;
  p.front.dtype = depth_dtype;
  p.front.H = H;
  p.front.W = W;
  p.front.max_depth = max_depth;
  p.front.conf = conf;
  p.front.conf_level = conf_level;
  p.r = radius;
  p.sigma_depth = sigma_depth;
  p.range_cut = range_cut;
  p.out = out;
  const int nt = 2 * radius + 1;
  for (int dy = -radius; dy <= radius; ++dy)
    for (int dx = -radius; dx <= radius; ++dx) {
      const double w = 1.0 - (double)(dy * dy + dx * dx) / (double)((radius + 1) * (radius + 1));
      p.wa[(dy + radius) * nt + (dx + radius)] = w > 0.0 ? w * w : 0.0;
    }
  const dim3 grid((unsigned)((W + kDfTileW - 1) / kDfTileW), (unsigned)((H + kDfTileH - 1) / kDfTileH));
  hipLaunchKernelGGL(k_depth_filter, grid, dim3(kDfThreads), 0, (hipStream_t)stream_, p);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}
