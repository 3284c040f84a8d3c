// plan.hip -- planning the fusion volume from the depth frames themselves (bnv_plan_extent, bnv_plan_count;
// include/bnv_fusion.h, "Volume planning"; bnv_fusion_amd/plan.py).  Two passes over the frames, both built on the
// float64 front end (frontend.hpp: pixel_valid, world_point) and on the encoder's voxelisation (bnv_common.hpp:
// in_bounds, voxel_coord; encode.hpp: corner_xyz, voxel_id), so that every number is the one a fusion run would see;
// before them an optional pass 0 (bnv_plan_normals) for scenes whose world frame is not the room's:
//
//   k_plan_normals  pass 0: per pixel with four valid neighbours a float64 normal, binned on a cube map; per bin the
//                   count and the fixed-point sum of the normals.  The host finds the Manhattan frame in it.
//   k_plan_extent  pass 1: per valid pixel and direction d, the bin of t = d . p in a histogram of uint64 counters that
//                   accumulates over the frames.  The host reads the histograms once and takes the (trimmed) extent
//                   along every direction from them: the bounds, and the yaw that minimises the footprint.
//   k_plan_count    pass 2: per valid pixel and candidate voxel size, the 8 corner voxels of the point go into a hash
//                   table (uint32 key claimed by CAS, uint32 pair count) -- the per-voxel pair counts the encoder's
//                   k_pointnet_scatter would accumulate, without the MLP.
//   k_plan_reduce   the table -> the frame's row (valid points, touched voxels, histogram of pair counts), leaving the
//                   table clean for the next frame;  k_plan_finish flags a table that went past half load.
//
// All of it is integer counting: any schedule gives the same result, tests/plan_restatement.py (passes 1 and 2) and
// tests/manhattan_restatement.py (pass 0) restate it in numpy.
#include "encode.hpp"
#include "frontend.hpp"
#include "workspace.hpp"

#include <cmath>

namespace bnv {

constexpr int kPlanThreads = 256;
constexpr int kPlanMaxDirs = 64;      // BNV_PLAN_MAX_DIRS
constexpr int kPlanMaxSizes = 8;      // BNV_PLAN_MAX_SIZES
constexpr int kPlanRowWords = 72;     // BNV_PLAN_ROW_WORDS
constexpr int kPlanHistCap = 64;      // BNV_PLAN_HIST_CAP: pair counts of 64 or more share the last histogram bin
constexpr int kPlanWindow = 256;      // bins of the in-workgroup window of pass 1 (one per thread)
constexpr uint32_t kPlanEmpty = 0xffffffffu;   // (voxel ids are below 2^31)
constexpr int64_t kPlanMaxPixels = (int64_t)1 << 24;

// ---- pass 0 ------------------------------------------------------------------------------------------------------
// The normal histogram of the Manhattan frame (plan.py: ManhattanFrame; tests/manhattan_restatement.py).  Per pixel a
// central-difference normal over a baseline of `step` pixels, float64 with one rounding per operation in the written
// order, rotated into the world, binned on a cube map of n_side x n_side cells a face.  What is accumulated per bin is
// integer: the count and the normal's components in 2^-20 fixed point.
struct PlanNormalsArgs {
  FrontArgs front;
  int step, n_side;
  double jump;
  unsigned long long* hist;   // [6 n_side^2][4]: count, sum n_x, sum n_y, sum n_z (two's complement)
};

constexpr int kPlanNormalSlots = 512;     // twice the workgroup's pixels: the LDS table never passes half load
constexpr double kPlanNormalScale = 1048576.0;   // 2^20

// depth in metres as this pass reads it: 0 < z <= max_depth and finite, and the confidence gate; else 0.  Deliberately
// not depth_at (frontend.hpp), whose mask is the reference's z < max_depth: pass 0 is defined with the inclusive bound
// of the tracking entries, and its gate applies to all five pixels of the stencil.  A pixel at exactly max_depth thus
// votes for a direction here and is no point in passes 1 and 2; it only votes, so no bound or count depends on it.
__device__ __forceinline__ double plan_normal_depth(const FrontArgs& a, int y, int x) {
  const size_t i = (size_t)y * a.W + x;
  double d;
  if (a.dtype == 0) d = __ddiv_rn((double)((const uint16_t*)a.depth)[i], 1000.0);
  else if (a.dtype == 1) d = (double)((const float*)a.depth)[i];
  else d = ((const double*)a.depth)[i];
  return (isfinite(d) && d > 0.0 && d <= a.max_depth && conf_ok(a, (int64_t)i)) ? d : 0.0;
}

__device__ __forceinline__ void plan_camera_point(const FrontArgs& a, int y, int x, double z, double (&p)[3]) {
  p[0] = __dmul_rn(__ddiv_rn(__dsub_rn((double)x, a.cx), a.fx), z);
  p[1] = __dmul_rn(__ddiv_rn(__dsub_rn((double)y, a.cy), a.fy), z);
  p[2] = z;
}

__device__ __forceinline__ double plan_dot3(double a0, double a1, double a2, double b0, double b1, double b2) {
  return __dadd_rn(__dadd_rn(__dmul_rn(a0, b0), __dmul_rn(a1, b1)), __dmul_rn(a2, b2));
}

// The bin and the fixed-point normal of pixel (y, x); false when the pixel does not count.
__device__ __forceinline__ bool plan_normal_of(const PlanNormalsArgs& p, int y, int x, int& bin, int (&fx)[3]) {
  const FrontArgs& a = p.front;
  const int s = p.step;
  if (x - s < 0 || x + s >= a.W || y - s < 0 || y + s >= a.H) return false;
  const double zc = plan_normal_depth(a, y, x);
  if (!(zc > 0.0)) return false;
  const double zl = plan_normal_depth(a, y, x - s), zr = plan_normal_depth(a, y, x + s);
  const double zu = plan_normal_depth(a, y - s, x), zd = plan_normal_depth(a, y + s, x);
  if (!(zl > 0.0 && zr > 0.0 && zu > 0.0 && zd > 0.0)) return false;
  const double gate = __dmul_rn(p.jump, zc);
  if (!(fabs(__dsub_rn(zl, zc)) <= gate && fabs(__dsub_rn(zr, zc)) <= gate && fabs(__dsub_rn(zu, zc)) <= gate &&
        fabs(__dsub_rn(zd, zc)) <= gate))
    return false;
  double pc[3], pl[3], pr[3], pu[3], pd[3];
  plan_camera_point(a, y, x, zc, pc);
  plan_camera_point(a, y, x - s, zl, pl);
  plan_camera_point(a, y, x + s, zr, pr);
  plan_camera_point(a, y - s, x, zu, pu);
  plan_camera_point(a, y + s, x, zd, pd);
  const double e[3] = {__dsub_rn(pr[0], pl[0]), __dsub_rn(pr[1], pl[1]), __dsub_rn(pr[2], pl[2])};
  const double f[3] = {__dsub_rn(pd[0], pu[0]), __dsub_rn(pd[1], pu[1]), __dsub_rn(pd[2], pu[2])};
  double n[3] = {__dsub_rn(__dmul_rn(e[1], f[2]), __dmul_rn(e[2], f[1])),
                 __dsub_rn(__dmul_rn(e[2], f[0]), __dmul_rn(e[0], f[2])),
                 __dsub_rn(__dmul_rn(e[0], f[1]), __dmul_rn(e[1], f[0]))};
  if (plan_dot3(n[0], n[1], n[2], pc[0], pc[1], pc[2]) > 0.0) {   // face the camera
    n[0] = -n[0];
    n[1] = -n[1];
    n[2] = -n[2];
  }
  double w[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) w[r] = plan_dot3(a.T[4 * r], a.T[4 * r + 1], a.T[4 * r + 2], n[0], n[1], n[2]);
  const double len = __dsqrt_rn(plan_dot3(w[0], w[1], w[2], w[0], w[1], w[2]));
  if (!(len > 0.0) || !isfinite(len)) return false;
#pragma unroll
  for (int r = 0; r < 3; ++r) w[r] = __ddiv_rn(w[r], len);
  int m = 0;
  if (fabs(w[1]) > fabs(w[m])) m = 1;
  if (fabs(w[2]) > fabs(w[m])) m = 2;   // (ties: the lower index)
  const double wm = m == 0 ? w[0] : (m == 1 ? w[1] : w[2]);
  const double wa = m == 0 ? w[1] : (m == 1 ? w[2] : w[0]);
  const double wb = m == 0 ? w[2] : (m == 1 ? w[0] : w[1]);
  const double am = fabs(wm);
  if (!(am > 0.0)) return false;        // (cannot happen for a finite positive length; keeps the divisions defined)
  const double side = (double)p.n_side;
  double qa = floor(__dmul_rn(__dmul_rn(__dadd_rn(__ddiv_rn(wa, am), 1.0), 0.5), side));
  double qb = floor(__dmul_rn(__dmul_rn(__dadd_rn(__ddiv_rn(wb, am), 1.0), 0.5), side));
  qa = !(qa >= 0.0) ? 0.0 : (qa > side - 1.0 ? side - 1.0 : qa);
  qb = !(qb >= 0.0) ? 0.0 : (qb > side - 1.0 ? side - 1.0 : qb);
  const int face = 2 * m + (wm < 0.0 ? 1 : 0);
  bin = (face * p.n_side + (int)qa) * p.n_side + (int)qb;
#pragma unroll
  for (int r = 0; r < 3; ++r) fx[r] = (int)rint(__dmul_rn(w[r], kPlanNormalScale));   // |.| <= 2^20
  return true;
}

// One thread per pixel.  The pixels of a workgroup on one wall share one or two bins, so nothing goes to global memory
// pixel by pixel: a workgroup sums what shares a bin in an LDS table keyed by bin (key claimed by CAS, linear probing;
// 256 pixels in 512 slots always find one) -- 256 normals of at most 2^20 a component fit int32 -- and then adds each
// occupied slot to the histogram with four 64-bit atomics on one 32-byte row.
__global__ __launch_bounds__(kPlanThreads) void k_plan_normals(PlanNormalsArgs p) {
  __shared__ uint32_t s_key[kPlanNormalSlots];
  __shared__ int s_val[kPlanNormalSlots][4];
  const FrontArgs& a = p.front;
  const int64_t n = (int64_t)a.H * a.W;
  const int64_t i = (int64_t)blockIdx.x * kPlanThreads + threadIdx.x;
  for (int s = threadIdx.x; s < kPlanNormalSlots; s += kPlanThreads) {
    s_key[s] = kPlanEmpty;
    s_val[s][0] = s_val[s][1] = s_val[s][2] = s_val[s][3] = 0;
  }
  int bin = 0, fx[3] = {0, 0, 0};
  const bool counts = i < n && plan_normal_of(p, (int)(i / a.W), (int)(i % a.W), bin, fx);
  __syncthreads();
  if (counts) {
    uint32_t s = ((uint32_t)bin * 0x9E3779B1u) >> 23;   // 9 bits: kPlanNormalSlots
    for (int probe = 0; probe < kPlanNormalSlots; ++probe) {
      uint32_t k = __hip_atomic_load(&s_key[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (k == kPlanEmpty) k = atomicCAS(&s_key[s], kPlanEmpty, (uint32_t)bin);
      if (k == kPlanEmpty || k == (uint32_t)bin) {
        atomicAdd(&s_val[s][0], 1);
        atomicAdd(&s_val[s][1], fx[0]);
        atomicAdd(&s_val[s][2], fx[1]);
        atomicAdd(&s_val[s][3], fx[2]);
        break;
      }
      s = (s + 1u) & (uint32_t)(kPlanNormalSlots - 1);
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < kPlanNormalSlots; s += kPlanThreads) {
    const uint32_t k = s_key[s];
    if (k == kPlanEmpty) continue;
    unsigned long long* row = p.hist + (size_t)k * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) atomicAdd(&row[c], (unsigned long long)(long long)s_val[s][c]);
  }
}

// ---- pass 1 ------------------------------------------------------------------------------------------------------
struct PlanExtentArgs {
  FrontArgs front;
  int n_dirs, n_bins;
  double bin_size;
  double dirs[kPlanMaxDirs * 3];
  unsigned long long* hist;   // [n_dirs][n_bins]
};

// Device-scope atomics on ONE address serialise at ~11 ns each, and a wall at constant x sends a
// whole frame into one bin of the x histogram.  So a workgroup first finds the range of bins its 256 pixels touch
// (wave reduce, then 4 words of LDS); a range of at most kPlanWindow bins is counted in an LDS window and every touched
// bin costs the workgroup ONE global atomic; a wider range (a frame seen at a grazing angle along d) goes to the global
// counters pixel by pixel -- its pixels are then spread over many addresses anyway.
__global__ __launch_bounds__(kPlanThreads) void k_plan_extent(PlanExtentArgs p) {
  __shared__ uint32_t win[kPlanWindow];
  __shared__ int s_lo[kPlanThreads / 64], s_hi[kPlanThreads / 64];
  const FrontArgs& a = p.front;
  const int64_t n = (int64_t)a.H * a.W;
  const int64_t i = (int64_t)blockIdx.x * kPlanThreads + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  bool valid = false;
  float pt[3] = {0.f, 0.f, 0.f};
  if (i < n) {
    const int y = (int)(i / a.W), x = (int)(i % a.W);
    valid = pixel_valid(a, y, x);
    if (valid) world_point(a, y, x, depth_at(a, y, x), pt);
  }
  win[threadIdx.x] = 0u;
  const double lim = (double)p.n_bins;
  for (int d = 0; d < p.n_dirs; ++d) {   // (uniform)
    int b = -1;
    if (valid) {
      const double t = (p.dirs[3 * d] * (double)pt[0] + p.dirs[3 * d + 1] * (double)pt[1]) + p.dirs[3 * d + 2] * (double)pt[2];
      double q = floor(t / p.bin_size);
      if (!(q >= -lim)) q = -lim;   // (also NaN: a point that overflowed float32 lands in overflow bin 0)
      if (!(q <= lim)) q = lim;
      long long bb = (long long)q + (long long)(p.n_bins / 2);
      bb = bb < 0 ? 0 : (bb > (long long)p.n_bins - 1 ? (long long)p.n_bins - 1 : bb);
      b = (int)bb;
    }
    int lo = valid ? b : 0x7fffffff, hi = b;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      const int ol = __shfl_xor(lo, s, 64), oh = __shfl_xor(hi, s, 64);
      lo = ol < lo ? ol : lo;
      hi = oh > hi ? oh : hi;
    }
    if (lane == 0) {
      s_lo[wave] = lo;
      s_hi[wave] = hi;
    }
    __syncthreads();   // (also: the window is clear -- zeroed above or by the flush of the previous direction)
#pragma unroll
    for (int w = 0; w < kPlanThreads / 64; ++w) {
      lo = s_lo[w] < lo ? s_lo[w] : lo;
      hi = s_hi[w] > hi ? s_hi[w] : hi;
    }
    unsigned long long* h = p.hist + (size_t)d * p.n_bins;
    if (hi < 0) {
      // no valid pixel in this workgroup
    } else if (hi - lo < kPlanWindow) {
      if (valid) atomicAdd(&win[b - lo], 1u);
    } else if (valid) {
      atomicAdd(&h[b], 1ull);
    }
    __syncthreads();
    if (hi >= 0 && hi - lo < kPlanWindow) {
      const uint32_t c = win[threadIdx.x];
      if (c) {
        atomicAdd(&h[lo + (int)threadIdx.x], (unsigned long long)c);   // (c > 0 only inside [lo, hi])
        win[threadIdx.x] = 0u;
      }
    }
  }
}

// ---- pass 2 ------------------------------------------------------------------------------------------------------
struct PlanTable {
  uint32_t* keys;     // [slots] voxel id or kPlanEmpty
  uint32_t* counts;   // [slots] (point, corner) pairs of that voxel
  int32_t* valid_blocks;   // [n_blocks] in-bounds points of each workgroup of k_plan_count
  uint32_t slots;     // a power of two
  int shift;          // 32 - log2(slots)
};

struct PlanCountArgs {
  FrontArgs front;
  int n_sizes;
  bnv_grid_t g[kPlanMaxSizes];
  PlanTable t[kPlanMaxSizes];
  long long* rows;    // [n_sizes][kPlanRowWords]
};

__device__ __forceinline__ void plan_insert(const PlanTable& t, uint32_t id, uint32_t len, long long* row) {
  uint32_t s = (id * 0x9E3779B1u) >> t.shift;
  const uint32_t mask = t.slots - 1u;
  for (uint32_t probe = 0; probe < t.slots; ++probe) {
    uint32_t k = __hip_atomic_load(&t.keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == kPlanEmpty) k = atomicCAS(&t.keys[s], kPlanEmpty, id);
    if (k == kPlanEmpty || k == id) {
      atomicAdd(&t.counts[s], len);
      return;
    }
    s = (s + 1u) & mask;
  }
  atomicOr((unsigned long long*)&row[2], 2ull);   // no free slot: the row is flagged, never silently short
}

// One thread per pixel.  Per candidate grid: the bounds mask and the 8 corner voxels of the encoder (mark_point /
// k_pointnet_scatter), corner by corner.  Neighbouring pixels are neighbouring lanes and mostly name the same voxel: the
// first lane of a run of EQUAL ADJACENT ids inserts the run's length, the others nothing (runs never join lanes that
// are not adjacent).  floor == ceil on an axis makes two corners of one point name the same voxel: both count, as the
// encoder counts them.
__global__ __launch_bounds__(kPlanThreads) void k_plan_count(PlanCountArgs p) {
  __shared__ int s_valid[kPlanMaxSizes][kPlanThreads / 64];
  const FrontArgs& a = p.front;
  const int64_t n = (int64_t)a.H * a.W;
  const int64_t i = (int64_t)blockIdx.x * kPlanThreads + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  bool have = false;
  float pt[3] = {0.f, 0.f, 0.f};
  if (i < n) {
    const int y = (int)(i / a.W), x = (int)(i % a.W);
    have = pixel_valid(a, y, x);
    if (have) world_point(a, y, x, depth_at(a, y, x), pt);
  }
  for (int s = 0; s < p.n_sizes; ++s) {   // (uniform)
    const bnv_grid_t& g = p.g[s];
    const PlanTable& t = p.t[s];
    long long* row = p.rows + (size_t)s * kPlanRowWords;
    const bool valid = have && in_bounds(pt[0], pt[1], pt[2], g);
    float xn = 0.f, yn = 0.f, zn = 0.f;
    if (valid) {
      xn = voxel_coord(pt[0], g.bound_min[0], g.voxel_size);
      yn = voxel_coord(pt[1], g.bound_min[1], g.voxel_size);
      zn = voxel_coord(pt[2], g.bound_min[2], g.voxel_size);
    }
    const int nyz = g.n_xyz[1] * g.n_xyz[2];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      uint32_t id = kPlanEmpty;
      if (valid) {
        int gx, gy, gz;
        corner_xyz(k, xn, yn, zn, gx, gy, gz);
        id = voxel_id(gx, gy, gz, nyz, g.n_xyz[2]);
      }
      const uint32_t prev = __shfl_up(id, 1, 64);
      const bool head = lane == 0 || prev != id;
      const unsigned long long heads = __ballot(head);
      if (head && id != kPlanEmpty) {
        const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
        const uint32_t len = above ? (uint32_t)__ffsll((long long)above) : (uint32_t)(64 - lane);
        plan_insert(t, id, len, row);
      }
    }
    const unsigned long long vb = __ballot(valid);
    if (lane == 0) s_valid[s][wave] = (int)__popcll(vb);
  }
  __syncthreads();
  if ((int)threadIdx.x < p.n_sizes) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < kPlanThreads / 64; ++w) c += s_valid[threadIdx.x][w];
    p.t[threadIdx.x].valid_blocks[blockIdx.x] = c;   // a plain store: no atomics on one counter (encode.hip: mark_point)
  }
}

// blockIdx.y = candidate.  Every workgroup turns kPlanThreads * 4 slots into counts (LDS histogram, one global atomic per
// touched bin) and empties them; workgroup 0 also sums the frame's in-bounds points.
constexpr int kPlanReduceItems = 4;
__global__ __launch_bounds__(kPlanThreads) void k_plan_reduce(PlanCountArgs p, int n_pixel_blocks) {
  __shared__ uint32_t s_hist[kPlanHistCap + 1];
  __shared__ uint32_t s_u;
  __shared__ long long s_nv[kPlanThreads / 64];
  const int s = blockIdx.y;
  const PlanTable& t = p.t[s];
  long long* row = p.rows + (size_t)s * kPlanRowWords;
  if (threadIdx.x <= kPlanHistCap) s_hist[threadIdx.x] = 0u;
  if (threadIdx.x == 0) s_u = 0u;
  __syncthreads();
  const uint64_t base = (uint64_t)blockIdx.x * (kPlanThreads * kPlanReduceItems);
  uint32_t u = 0;
#pragma unroll
  for (int e = 0; e < kPlanReduceItems; ++e) {
    const uint64_t slot = base + (uint64_t)e * kPlanThreads + threadIdx.x;
    if (slot < t.slots && t.keys[slot] != kPlanEmpty) {
      const uint32_t c = t.counts[slot];
      atomicAdd(&s_hist[c < (uint32_t)kPlanHistCap ? c : (uint32_t)kPlanHistCap], 1u);
      ++u;
      t.keys[slot] = kPlanEmpty;
      t.counts[slot] = 0u;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) u += __shfl_xor(u, d, 64);
  if ((threadIdx.x & 63) == 0 && u) atomicAdd(&s_u, u);
  __syncthreads();
  if (threadIdx.x <= kPlanHistCap && s_hist[threadIdx.x])
    atomicAdd((unsigned long long*)&row[4 + threadIdx.x], (unsigned long long)s_hist[threadIdx.x]);
  if (threadIdx.x == 0 && s_u) atomicAdd((unsigned long long*)&row[1], (unsigned long long)s_u);
  if (blockIdx.x == 0) {
    long long nv = 0;
    for (int b = threadIdx.x; b < n_pixel_blocks; b += kPlanThreads) nv += t.valid_blocks[b];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) nv += __shfl_xor(nv, d, 64);
    if ((threadIdx.x & 63) == 0) s_nv[threadIdx.x >> 6] = nv;
    __syncthreads();
    if (threadIdx.x == 0) {
      nv = 0;
#pragma unroll
      for (int w = 0; w < kPlanThreads / 64; ++w) nv += s_nv[w];
      atomicAdd((unsigned long long*)&row[0], (unsigned long long)nv);
    }
  }
}

// a table past half load: the row says so (status bit 0); the counts of such a row are still exact unless bit 1 is set
__global__ void k_plan_finish(PlanCountArgs p) {
  const int s = threadIdx.x;
  if (s >= p.n_sizes) return;
  long long* row = p.rows + (size_t)s * kPlanRowWords;
  if (row[1] * 2 > (long long)p.t[s].slots) row[2] |= 1;
}

// ---- host --------------------------------------------------------------------------------------------------------
static bool plan_frame_args_ok(const void* depth, int depth_dtype, int H, int W, const double* intr, const double* T_wc,
                               double max_depth, const uint8_t* conf, int conf_level) {
  if (!depth || !intr || !T_wc || H <= 0 || W <= 0 || H > 32768 || W > 32768 || (int64_t)H * W > kPlanMaxPixels ||
      depth_dtype < 0 || depth_dtype > 2 || !front_conf_args_ok(conf, conf_level))
    return false;
  if (!(std::isfinite(max_depth) && max_depth > 0.0)) return false;
  return all_finite(intr, 9) && all_finite(T_wc, 12) && intr[0] != 0.0 && intr[4] != 0.0;
}

static bool plan_grid_ok(const bnv_grid_t& g) {
  if (g.n_xyz[0] <= 0 || g.n_xyz[1] <= 0 || g.n_xyz[2] <= 0) return false;
  if ((int64_t)g.n_xyz[0] * g.n_xyz[1] * g.n_xyz[2] >= ((int64_t)1 << 31)) return false;   // int32 flat ids
  if (!(std::isfinite(g.voxel_size) && g.voxel_size > 0.f)) return false;
  for (int a = 0; a < 3; ++a)
    if (!(std::isfinite(g.bound_min[a]) && std::isfinite(g.bound_lo[a]) && std::isfinite(g.bound_hi[a]))) return false;
  return true;
}

// slots of one candidate's table: table_slots when the caller forces a size, else the smallest power of two that keeps
// the table at or below half load whatever the frame: 2 * min(8 H W, voxels)
static int64_t plan_table_slots(int H, int W, const bnv_grid_t& g, int64_t table_slots) {
  if (table_slots > 0) return table_slots;
  int64_t most = 8 * (int64_t)H * W;
  const int64_t nvox = (int64_t)g.n_xyz[0] * g.n_xyz[1] * g.n_xyz[2];
  if (most > nvox) most = nvox;
  int64_t slots = 64;
  while (slots < 2 * most) slots <<= 1;
  return slots;
}

static bool plan_slots_arg_ok(int64_t table_slots) {
  return table_slots == 0 || (table_slots >= 64 && table_slots <= ((int64_t)1 << 30) && (table_slots & (table_slots - 1)) == 0);
}

static size_t plan_ws_layout(int H, int W, const bnv_grid_t* grids, int n_sizes, int64_t table_slots, char* base,
                             PlanTable* tables) {
  const int64_t n_blocks = ((int64_t)H * W + kPlanThreads - 1) / kPlanThreads;
  Carver c(base);
  for (int s = 0; s < n_sizes; ++s) {
    const int64_t slots = plan_table_slots(H, W, grids[s], table_slots);
    PlanTable t;
    t.keys = c.take<uint32_t>(slots);
    t.counts = c.take<uint32_t>(slots);
    t.valid_blocks = c.take<int32_t>(n_blocks);
    t.slots = (uint32_t)slots;
    int lg = 0;
    while (((int64_t)1 << lg) < slots) ++lg;
    t.shift = 32 - lg;
    if (tables) tables[s] = t;
  }
  return c.bytes();
}

static bool plan_count_shape_ok(int H, int W, const bnv_grid_t* grids, int n_sizes, int64_t table_slots) {
  if (!grids || n_sizes < 1 || n_sizes > kPlanMaxSizes || H <= 0 || W <= 0 || H > 32768 || W > 32768 ||
      (int64_t)H * W > kPlanMaxPixels || !plan_slots_arg_ok(table_slots))
    return false;
  for (int s = 0; s < n_sizes; ++s)
    if (!plan_grid_ok(grids[s])) return false;
  return true;
}

}  // namespace bnv

using namespace bnv;

extern "C" size_t bnv_plan_workspace_bytes(int H, int W, const bnv_grid_t* grids_host, int n_sizes, int64_t table_slots) {
  if (!plan_count_shape_ok(H, W, grids_host, n_sizes, table_slots)) return 0;
  return plan_ws_layout(H, W, grids_host, n_sizes, table_slots, nullptr, nullptr);
}

extern "C" int bnv_plan_workspace_reset(void* workspace, size_t ws_bytes, int H, int W, const bnv_grid_t* grids_host,
                                        int n_sizes, int64_t table_slots, bnv_stream_t stream_) {
  if (!workspace || !plan_count_shape_ok(H, W, grids_host, n_sizes, table_slots)) return BNV_ERR_INVALID_ARGUMENT;
  PlanTable t[kPlanMaxSizes];
  if (plan_ws_layout(H, W, grids_host, n_sizes, table_slots, (char*)workspace, t) > ws_bytes)
    return BNV_ERR_WORKSPACE_TOO_SMALL;
  hipStream_t stream = (hipStream_t)stream_;
  for (int s = 0; s < n_sizes; ++s) {
    BNV_HIP_CHECK(hipMemsetAsync(t[s].keys, 0xff, (size_t)t[s].slots * 4, stream));
    BNV_HIP_CHECK(hipMemsetAsync(t[s].counts, 0, (size_t)t[s].slots * 4, stream));
  }
  return BNV_OK;
}

extern "C" int bnv_plan_normals(const void* depth, int depth_dtype, int H, int W, const double* intr_host,
                                const double* T_wc_host, double max_depth, const uint8_t* conf, int conf_level, int step,
                                double jump, int n_side, int64_t* hist, bnv_stream_t stream_) {
  if (!plan_frame_args_ok(depth, depth_dtype, H, W, intr_host, T_wc_host, max_depth, conf, conf_level) || !hist ||
      step < 1 || step > 64 || !(std::isfinite(jump) && jump > 0.0) || n_side < 4 || n_side > 64)
    return BNV_ERR_INVALID_ARGUMENT;
  PlanNormalsArgs p{};
  front_args_fill(p.front, depth, depth_dtype, H, W, intr_host, T_wc_host, max_depth);
  p.front.conf = conf;
  p.front.conf_level = conf_level;
  p.step = step;
  p.n_side = n_side;
  p.jump = jump;
  p.hist = (unsigned long long*)hist;
  const unsigned n_blocks = blocks_for((int64_t)H * W, kPlanThreads);
  hipLaunchKernelGGL(k_plan_normals, dim3(n_blocks), dim3(kPlanThreads), 0, (hipStream_t)stream_, p);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

extern "C" int bnv_plan_extent(const void* depth, int depth_dtype, int H, int W, const double* intr_host,
                               const double* T_wc_host, double max_depth, const uint8_t* conf, int conf_level,
                               const double* dirs_host, int n_dirs, double bin_size, int n_bins, uint64_t* hist,
                               bnv_stream_t stream_) {
  if (!plan_frame_args_ok(depth, depth_dtype, H, W, intr_host, T_wc_host, max_depth, conf, conf_level) || !dirs_host ||
      !hist || n_dirs < 1 || n_dirs > kPlanMaxDirs || n_bins < 2 || n_bins > 65536 || (n_bins & (n_bins - 1)) != 0)
    return BNV_ERR_INVALID_ARGUMENT;
  if (!(std::isfinite(bin_size) && bin_size > 0.0) || !all_finite(dirs_host, 3 * n_dirs))
    return BNV_ERR_INVALID_ARGUMENT;
  PlanExtentArgs p{};
  front_args_fill(p.front, depth, depth_dtype, H, W, intr_host, T_wc_host, max_depth);
  p.front.conf = conf;
  p.front.conf_level = conf_level;
  p.n_dirs = n_dirs;
  p.n_bins = n_bins;
  p.bin_size = bin_size;
  for (int i = 0; i < 3 * n_dirs; ++i) p.dirs[i] = dirs_host[i];
  p.hist = (unsigned long long*)hist;
  const unsigned n_blocks = blocks_for((int64_t)H * W, kPlanThreads);
  hipLaunchKernelGGL(k_plan_extent, dim3(n_blocks), dim3(kPlanThreads), 0, (hipStream_t)stream_, p);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}

extern "C" int bnv_plan_count(const void* depth, int depth_dtype, int H, int W, const double* intr_host,
                              const double* T_wc_host, double max_depth, const uint8_t* conf, int conf_level,
                              const bnv_grid_t* grids_host, int n_sizes, int64_t table_slots, void* workspace,
                              size_t ws_bytes, int64_t* rows_out, bnv_stream_t stream_) {
  if (!plan_frame_args_ok(depth, depth_dtype, H, W, intr_host, T_wc_host, max_depth, conf, conf_level) || !workspace ||
      !rows_out || !plan_count_shape_ok(H, W, grids_host, n_sizes, table_slots))
    return BNV_ERR_INVALID_ARGUMENT;
  PlanCountArgs p{};
  if (plan_ws_layout(H, W, grids_host, n_sizes, table_slots, (char*)workspace, p.t) > ws_bytes)
    return BNV_ERR_WORKSPACE_TOO_SMALL;
  front_args_fill(p.front, depth, depth_dtype, H, W, intr_host, T_wc_host, max_depth);
  p.front.conf = conf;
  p.front.conf_level = conf_level;
  p.n_sizes = n_sizes;
  uint32_t most_slots = 0;
  for (int s = 0; s < n_sizes; ++s) {
    p.g[s] = grids_host[s];
    most_slots = p.t[s].slots > most_slots ? p.t[s].slots : most_slots;
  }
  p.rows = (long long*)rows_out;
  hipStream_t stream = (hipStream_t)stream_;
  const int n_blocks = (int)blocks_for((int64_t)H * W, kPlanThreads);
  hipLaunchKernelGGL(k_plan_count, dim3((unsigned)n_blocks), dim3(kPlanThreads), 0, stream, p);
  BNV_LAUNCH_CHECK();
  const unsigned per_block = kPlanThreads * kPlanReduceItems;
  const unsigned rb = (most_slots + per_block - 1) / per_block;
  hipLaunchKernelGGL(k_plan_reduce, dim3(rb, (unsigned)n_sizes), dim3(kPlanThreads), 0, stream, p, n_blocks);
  BNV_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_plan_finish, dim3(1), dim3(64), 0, stream, p);
  BNV_LAUNCH_CHECK();
  return BNV_OK;
}
