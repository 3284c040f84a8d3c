// decode_host.hpp -- host-side pieces the decode files share (decode.hip, decode_pts.hip, lattice.hip): the lattice
// workspace layout, argument checks, grid sizing, the A/B option words and the arithmetic-mode dispatch.  No kernels.
#pragma once
#include <type_traits>

#include "bnv_common.hpp"
#include "workspace.hpp"

namespace bnv {

// bnv_set_option words of the lattice decode (defined in decode.hip)
extern std::atomic<int> g_fused_mark;
extern std::atomic<int> g_mark_per_origin;
extern std::atomic<int> g_half_tail;
extern std::atomic<int> g_lattice_pipe;

// ---- lattice decode: workspace ----------------------------------------------------------------
struct LatticeWs {
  int32_t* nbr_rows;  // [n][27]
  int32_t* list;      // [list_capacity] rows whose table is needed
  int32_t* n_list;    // [1]
  int32_t* stamp;     // [row_capacity]
  float* table;       // [row_capacity][27]
  uint32_t* need_mask;  // [row_capacity] bit l set: table[row][l] is read by a live lattice point
  int32_t* origin_stamp;  // [row_capacity] == epoch: the row's voxel is a decoded origin of this call
  int32_t* entries;   // [entry_capacity] (row << 5) | l
  int64_t list_capacity;
  int64_t entry_capacity;
};

static inline size_t lattice_ws_layout(int64_t n, int64_t row_capacity, char* base, LatticeWs* ws) {
  if (n < 1) n = 1;
  int64_t cap = 27 * n;
  if (cap > row_capacity) cap = row_capacity;
  int64_t ecap = 27 * cap;
  if (ecap > 216 * n) ecap = 216 * n;
  Carver c(base);
  LatticeWs t;
  // stamp and table first: they persist across calls with the same row_capacity
  t.stamp = c.take<int32_t>(row_capacity);
  t.table = c.take<float>(row_capacity * 27);
  t.need_mask = c.take<uint32_t>(row_capacity);
  t.origin_stamp = c.take<int32_t>(row_capacity);
  t.n_list = c.take<int32_t>(64);
  t.nbr_rows = c.take<int32_t>(n * 27);
  t.list = c.take<int32_t>(cap);
  t.entries = c.take<int32_t>(ecap);
  t.list_capacity = cap;
  t.entry_capacity = ecap;
  if (ws) *ws = t;
  return c.bytes();
}

// grid of a grid-stride kernel: the blocks the work needs, at most `per_cu` per CU
static inline unsigned capped_grid(int64_t blocks, int per_cu) {
  const int64_t cap = (int64_t)(g_num_cus > 0 ? g_num_cus : 256) * per_cu;
  return (unsigned)(blocks < 1 ? 1 : (blocks < cap ? blocks : cap));
}

static inline bool vol_ok_ro(const bnv_volume_t* v) {
  return v && v->slot_keys && v->slot_rows && v->n_slots > 0 && (v->n_slots & (v->n_slots - 1)) == 0 &&
         v->n_feats == 8;
}

// does this call work on the volume's persistent tables (include/bnv_fusion.h: bnv_volume_t.lattice_persist)?
static inline bool lattice_persist(const bnv_volume_t* vol) {
  return vol && vol->lattice_persist && vol->lattice_table && vol->lattice_have;
}

// f(std::integral_constant<int, P>{}) for the arithmetic mode `mlp` of a call (mlp_mode_of); out of range: mode 0
template <class F>
static inline void dispatch_prec(int mlp, F f) {
  if (mlp == 2) f(std::integral_constant<int, 2>{});
  else if (mlp == 1) f(std::integral_constant<int, 1>{});
  else if (mlp == 3) f(std::integral_constant<int, 3>{});
  else f(std::integral_constant<int, 0>{});
}

// lets `kernel` be launched with `bytes` of dynamic LDS; rc keeps the first failure
static inline void opt_in_lds(int& rc, const void* kernel, int bytes) {
  if (rc != BNV_OK) return;
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) {
    g_last_hip_error = (int)e;
    rc = BNV_ERR_HIP;
  }
}

// the table stage of the lattice decode (decode.hip) and the opt-in of decode_pts.hip's kernels to their dynamic LDS
// (bnv_decode_init); library-internal
__attribute__((visibility("hidden"))) int lattice_table_impl(const bnv_volume_t* vol, const bnv_grid_t* grid,
                                                             const float* features, const float* sdfmlp_pack,
                                                             int64_t n_voxels, int use_entries, void* ws_ptr,
                                                             size_t ws_bytes, int max_workgroups, bnv_stream_t stream);
__attribute__((visibility("hidden"))) int decode_pts_init();
// bnv_decode_lattice by stages (lattice.hip): 1 = neighbour rows + live entries, 2 = table MLP, 4 = blend into out_sdf.
// The frame pipeline (pipeline.hip) runs 1 | 2 on one stream and blends on another; bnv_decode_lattice is all three.
__attribute__((visibility("hidden"))) int decode_lattice_stages(
    const bnv_volume_t* vol, const bnv_grid_t* grid, const float* features, const float* weights, int64_t row_limit,
    const float* sdfmlp_pack, const int64_t* origins, int64_t n, const int32_t* n_dev, const bnv_sdf_delta_t* delta,
    void* ws, size_t ws_bytes, int32_t epoch, bool prestamped, float* out_sdf, int stages, bnv_stream_t stream);

}  // namespace bnv
