// What csrc/meshsdf.hip needs from the rest of the library, for tools/mesh_sdf_bench.py's counting build of that one
// file (-DBNV_MESHSDF_COUNT_TESTS): the HIP error word and the launch epochs of the look-back scan.
#include <atomic>
#include <stdint.h>

namespace bnv {
int g_last_hip_error = 0;
static std::atomic<uint32_t> g_epoch{0};
uint32_t next_epoch() {   // (runtime.hip's: the 30-bit tag never takes the value 0 of a cleared workspace word)
  uint32_t e;
  do e = g_epoch.fetch_add(1, std::memory_order_relaxed) + 1;
  while ((e & 0x3fffffffu) == 0);
  return e;
}
}  // namespace bnv
