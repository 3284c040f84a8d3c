// runtime.hip -- what the whole library links against: the device's size, the last HIP error, the process-wide option
// words, event timing of the dominant kernels, launch epochs of the look-back scans; bnv_init and the entries around them.
#include <utility>
#include <vector>

#include "encode.hpp"
#include "scan.hpp"

namespace bnv {

int g_num_cus = 0;
int g_last_hip_error = 0;
// Process-wide words, all relaxed atomics read once per launch.  The A/B switches choose between implementations with
// identical results; the MLP mode here is only the DEFAULT of calls whose grid does not name one (bnv_grid_t.mlp_mode).
std::atomic<int> g_reserve_cus{0};  // bnv_set_option("reserve_cus"): CUs the persistent MLP kernels leave to other streams
std::atomic<int> g_finalize_blocks{0};      // bnv_set_option("finalize_blocks"): workgroups of k_finalize (0: 2 per CU, which is also the most it may use); tests force the striding with a small value
std::atomic<int> g_tcnn_shared_table{1};    // bnv_set_option("tcnn_shared_table"): 1 = one LDS table per workgroup and 16 x 16 patch, 0 = per wave and block
std::atomic<int> g_tcnn_block_encoder{1};  // bnv_set_option("tcnn_block_encoder"): 1 = k_pointnet_scatter_tb for whole frames
std::atomic<int> g_mlp_mode{1};  // default arithmetic: 0 exact fp32 MFMA; 1 fp32 operands split into f16 hi+lo; 2 tcnn fp16 networks; 3 f16 operands

// ---- HIP-event timing of the dominant kernels, recorded on the stream they are launched on ----
bool g_prof_on = false;
static std::vector<std::pair<hipEvent_t, hipEvent_t>> g_prof_events[PROF_KINDS];
static size_t g_prof_used[PROF_KINDS] = {0, 0, 0, 0};

void prof_mark(int kind, bool begin, hipStream_t stream) {
  auto& ring = g_prof_events[kind];
  if (begin) {
    if (g_prof_used[kind] == ring.size()) {
      hipEvent_t a, b;
      if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
      ring.emplace_back(a, b);
    }
    (void)hipEventRecord(ring[g_prof_used[kind]].first, stream);
  } else if (g_prof_used[kind] < ring.size()) {
    (void)hipEventRecord(ring[g_prof_used[kind]].second, stream);
    ++g_prof_used[kind];
  }
}
// every launch of a look-back kernel takes a fresh epoch (scan.hpp: lookback_exclusive)
// (atomic: host threads driving different streams / volumes each get their own; the 30-bit tag never takes the value
// 0, which is what a zero-initialised workspace word carries)
static std::atomic<uint32_t> g_epoch{0};
uint32_t next_epoch() {
  uint32_t e;
  do e = g_epoch.fetch_add(1, std::memory_order_relaxed) + 1;
  while ((e & 0x3fffffffu) == 0);
  return e;
}
}  // namespace bnv

using namespace bnv;

extern "C" {

int bnv_init(int device) {
  BNV_HIP_CHECK(hipSetDevice(device));
  int cus = 0;
  BNV_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
  g_num_cus = cus;
  BNV_TRY(encode_init());   // (each part opts its own kernels in to their dynamic LDS)
  extern int bnv_decode_init();
  return bnv_decode_init();
}

int bnv_num_compute_units(void) { return g_num_cus; }
int bnv_last_hip_error(void) { return g_last_hip_error; }

const char* bnv_status_string(int s) {
  switch (s) {
    case BNV_OK: return "ok";
    case BNV_ERR_INVALID_ARGUMENT: return "invalid argument";
    case BNV_ERR_WORKSPACE_TOO_SMALL: return "workspace too small";
    case BNV_ERR_HIP: return "HIP runtime error";
    case BNV_ERR_NOT_INITIALISED: return "bnv_init not called";
    case BNV_ERR_CAPACITY: return "capacity exceeded";
    default: return "unknown";
  }
}

int bnv_set_mlp_mode(int mode) {
  if (mode < 0 || mode > 3) return BNV_ERR_INVALID_ARGUMENT;
  g_mlp_mode.store(mode, std::memory_order_relaxed);
  return BNV_OK;
}
int bnv_get_mlp_mode(void) { return g_mlp_mode.load(std::memory_order_relaxed); }

int bnv_profile_enable(int on) {
  for (int k = 0; k < PROF_KINDS; ++k) g_prof_used[k] = 0;
  g_prof_on = on != 0;
  return BNV_OK;
}

int bnv_profile_read(double* total_ms, int64_t* launches) {
  if (!total_ms || !launches) return BNV_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < PROF_KINDS; ++k) {
    double ms = 0.0;
    for (size_t i = 0; i < g_prof_used[k]; ++i) {
      float t = 0.f;
      BNV_HIP_CHECK(hipEventSynchronize(g_prof_events[k][i].second));
      BNV_HIP_CHECK(hipEventElapsedTime(&t, g_prof_events[k][i].first, g_prof_events[k][i].second));
      ms += t;
    }
    total_ms[k] = ms;
    launches[k] = (int64_t)g_prof_used[k];
  }
  return BNV_OK;
}

}  // extern "C"
