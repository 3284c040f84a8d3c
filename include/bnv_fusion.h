/*
 * bnv_fusion.h -- C ABI of the MI355X (gfx950) implementation of BNV-Fusion's per-frame
 * local-fusion + SDF-decode hot path.
 *
 * The reference (likojack/bnv_fusion) has no FFI for this path: the boundary there is a Python
 * duck type (LitFusionPointNet / SparseVolume).  The entry points below are what a binding of
 * those methods needs; each cites the reference code it replaces (paths relative to the
 * reference repo).  Conventions:
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - the caller owns all memory (the library never allocates device memory);
 *   - every function enqueues work on `stream` (a hipStream_t passed as void*) and returns
 *     immediately; it returns 0 on success or a negative bnv_status code, never throws;
 *   - counts that are only known on the device are written to caller-provided device structs;
 *     the caller synchronises the stream before reading them.
 *   - build: hipcc --offload-arch=gfx950 (bnv_fusion_amd/csrc/build.py); no CPU fallback exists.
 */
#ifndef BNV_FUSION_H
#define BNV_FUSION_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* bnv_stream_t; /* hipStream_t */

enum bnv_status {
  BNV_OK = 0,
  BNV_ERR_INVALID_ARGUMENT = -1,
  BNV_ERR_WORKSPACE_TOO_SMALL = -2,
  BNV_ERR_HIP = -3,          /* a HIP runtime call failed; see bnv_last_hip_error() */
  BNV_ERR_NOT_INITIALISED = -4,
  BNV_ERR_CAPACITY = -5
};

/* Voxel grid of one SparseVolume (sparse_volume.py:485-500, voxel_utils.py:83-88).  The float
 * members are the float32 values the reference holds: bound_min = float32(min_coords);
 * bound_lo = float32(min_coords) + float32(voxel), bound_hi = float32(max_coords) - float32(voxel)
 * evaluated in float32 (local_point_fusion.py:94-100). */
typedef struct bnv_grid {
  float bound_min[3];
  float bound_lo[3];
  float bound_hi[3];
  float voxel_size;
  int32_t n_xyz[3];
  int32_t min_pts_in_grid;
  /* spatial sharding of the active-voxel set: a voxel is owned by
   * hash(block coordinate) % shard_world, blocks of (1 << shard_block_log2)^3 voxels.
   * shard_world = 1 disables sharding. */
  int32_t shard_rank;
  int32_t shard_world;
  int32_t shard_block_log2;
  /* Arithmetic of the MLP kernels for calls made with this grid: 0 = the process default (bnv_set_mlp_mode),
   * BNV_GRID_MLP_MODE(m) = 1 + m selects mode m for these calls alone.  The mode belongs to the model (its weight
   * packs are laid out for it), so callers that hold several models -- or drive the library from several host
   * threads -- state it here instead of flipping the process default around their calls. */
  int32_t mlp_mode;
  /* Ownership rule of the sharding.  NULL: owner = hash(block coordinate) % shard_world, a pure function.  Else a
   * device buffer of bnv_shard_state_bytes() (zeroed once, the SAME evolving content on every rank -- the kernels
   * that update it work on the replicated voxelisation): FIRST-TOUCH ownership.  A block gets its owner in the frame
   * that first touches it: the new blocks of a frame, in ascending block order, go one by one to the rank that carries
   * the least load so far (load = touched voxels of a block in that frame); the 26 neighbour blocks of a newly
   * touched block that have no owner yet are pinned at the same moment to (bx + 5 by + 7 bz) % shard_world, so that
   * whenever a voxel is emitted every block of its 3x3x3 neighbourhood has an owner that never changes afterwards
   * (the boundary / ghost-row tests of the exchange rely on that).  Set by bnv_encode_begin* of the frame; every other
   * call only reads it.
   * That is BNV_SHARD_RULE_GREEDY, what a zeroed buffer means: blocks interleave finely, every rank holds an even
   * sample of ANY view (max / mean load 1.01-1.06) and ~1.2 x the single-GPU decode work is done in total (the halo).
   * bnv_shard_state_configure selects BNV_SHARD_RULE_REGION instead: contiguous regions.  cur[r] = the voxels THIS
   * frame touches in blocks rank r owns; a new block without an owner, in walk order (bands stacked along `axis`), goes
   * to the least-loaded not-full owner among its 26 neighbour blocks, else to the RECEIVER (the least-loaded rank, which
   * keeps that role until it is full: cur * world >= the frame's touched voxels); then the untouched neighbours of the
   * new blocks are pinned to the owner of the first new block (walk order) that reaches them -- regions grow outwards
   * -- or to the receiver when that owner carries more than 9/8 of its share.  Total decode work ~1.03-1.07 x single
   * GPU, a quarter of the boundary records; balanced while the view stays put or moves ACROSS the bands (1.04 on the
   * benchmark's pan with bands stacked along the vertical), not for a camera that sweeps a room (1.4-1.5).  Same
   * invariant, same determinism: every rank computes the same table. */
  void* shard_state;
} bnv_grid_t;
#define BNV_GRID_MLP_MODE(m) ((m) + 1)
#define BNV_SHARD_RULE_GREEDY 0
#define BNV_SHARD_RULE_REGION 1
/* Bytes of bnv_grid_t.shard_state for a grid of n_xyz voxels in blocks of (1 << block_log2)^3. */
size_t bnv_shard_state_bytes(const int32_t n_xyz[3], int32_t block_log2);
/* Selects the first-touch rule of a ZEROED shard_state buffer (before its first frame; the same call on every rank):
 * rule BNV_SHARD_RULE_*, axis 0 / 1 / 2 = the grid axis the region rule stacks its first bands along (the axis the
 * camera moves least along: the vertical).  Ordered on `stream` (and waited for: a set-up call). */
int bnv_shard_state_configure(void* shard_state, int32_t rule, int32_t axis, bnv_stream_t stream);
/* Byte offsets inside it: the per-rank loads (uint64[64]) and the owner table (one byte per block, index
 * (bx * nby + by) * nbz + bz; bits 0..5 owner, bit 6 assigned, bit 7 touched), for tools and tests. */
size_t bnv_shard_state_loads_offset(void);
size_t bnv_shard_state_table_offset(void);

/* Device-side result counters of bnv_encode_pointcloud. */
typedef struct bnv_encode_counters {
  int32_t n_valid_points; /* points that passed the bounds mask                                 */
  int32_t n_unique;       /* U : voxels touched by >= 1 (point, corner) pair                    */
  int32_t n_out;          /* U': rows written (count >= min_pts_in_grid and owned by this shard) */
  float n_avg_pts;        /* mean pair count over all U voxels (local_point_fusion.py:143)       */
  int32_t error;          /* != 0: an output capacity was exceeded                               */
  int32_t reserved[3];    /* [0]: sharded encode: (point, corner) pairs this shard encoded; others 0 */
} bnv_encode_counters_t;

/* Sparse feature volume = open-addressing hash (packed 3x21-bit key -> row) + dense row arrays
 * (replaces open3d.core.HashMap, sparse_volume.py:588-594).  All arrays are caller-owned. */
typedef struct bnv_volume {
  uint64_t* slot_keys;   /* [n_slots]  packed key, ~0 = empty                 */
  int32_t* slot_rows;    /* [n_slots]  row index                              */
  int64_t n_slots;       /* power of two                                      */
  int64_t* row_coords;   /* [row_capacity, 3] voxel coordinates (int64)       */
  float* features;       /* [row_capacity, n_feats]                           */
  float* weights;        /* [row_capacity]                                    */
  float* num_hits;       /* [row_capacity]                                    */
  int64_t row_capacity;
  int32_t* n_rows;       /* device int32[2]: {rows in use, sticky error of the upsert kernels: 0 ok, 1 slot table
                            full, 2 voxel coordinate outside the 21-bit key range, 3 row capacity exceeded};
                            bnv_volume_clear zeroes both                      */
  int32_t n_feats;       /* 8                                                 */
  /* Optional dense index of the volume's grid ("brick"): brick[(x * dims[1] + y) * dims[2] + z] = row of voxel
   * (x, y, z), or -1.  Maintained by every kernel that creates rows, for keys inside [0, dims); read by the decode
   * kernels in place of 27 hash probes per voxel (neighbouring voxels are neighbouring words: one cache line serves
   * a whole z-run, where every hash probe pulls a line of its own).  NULL: not kept (the hash is always complete). */
  int32_t* brick;
  int32_t brick_dims[3];
  /* Optional PERSISTENT lattice tables of the per-frame decode (bnv_frame_pipe_t; NULL: none).  lattice_table
   * [row_capacity * 27]: the SDF table entry of (row, lattice offset l), as bnv_lattice_table computes it;
   * lattice_have [row_capacity]: bit l set <=> that entry was computed from the row's CURRENT features.  Every kernel
   * of this library that writes a row's features clears the row's word (the upserts, the ghost-row install, insert);
   * the per-frame decode then evaluates only the entries a frame reads that are not there yet -- entries in rows the
   * frame did not update are carried over from earlier frames -- and the blend reads lattice_table.  A caller that
   * changes features by any other means zeroes lattice_have (the optimiser does not: it steps a COPY, to_tensor(), and
   * writes it back through insert, which clears the words); so does a caller that changes the SDF network's weights
   * (the entries are functions of both: SparseVolume.invalidate_tables, which the frame pipe calls when the model's
   * pack version moves).
   * bnv_volume_clear / bnv_volume_rehash leave both alone: the owner re-makes them with the row arrays. */
  float* lattice_table;
  uint32_t* lattice_have;
  /* 1: THIS call's lattice decode reads and extends the persistent tables (the frame pipeline sets it for its own
   * calls): its `features` argument must then be the volume's own array and the table stage must work on listed
   * entries -- anything else is rejected with BNV_ERR_INVALID_ARGUMENT (the three stages share ONE predicate);
   * 0: the call keeps to its workspace (every other decode: its features argument need not be the volume's). */
  int32_t lattice_persist;
} bnv_volume_t;

/* ------------------------------------------------------------------------------------------ */
int bnv_init(int device);           /* query the device, opt kernels in to large LDS          */
int bnv_num_compute_units(void);
const char* bnv_status_string(int status);
int bnv_last_hip_error(void);

/* Arithmetic of the two MLPs (point encoder, SDF decoder).  Both modes take fp32 inputs/weights and
 * accumulate in fp32:
 *   0  exact fp32: v_mfma_f32_32x32x2_f32 (bitwise an fp32 fmaf chain), 157 TFLOP/s peak;
 *   1  (default) split operands: every fp32 operand x = hi + lo with hi, lo in f16 (about 22 significant
 *      bits; f16 subnormals are kept), a.b ~ ah.bh + ah.bl + al.bh on the f16 MFMA (v_mfma_f32_16x16x32_f16 in
 *      the per-frame kernels, 32x32x16 in the generic decode and backward kernels): fp32-class accuracy
 *      (differences at the level of fp32 summation order) at 16/3 the MFMA rate;
 *   2  the tiny-cuda-nn networks of the reference's default checkpoint (pointnet_tcnn.ckpt): inputs
 *      padded with 1.0, 64-wide, no bias, fp16 weights and activations, f16 MFMA with fp32
 *      accumulation.  The pack buffers then hold the tcnn layouts (weights.py: pack_*_tcnn);
 *   3  the fp32 checkpoint with weights and activations rounded to f16 (the hi halves of mode 1's packs),
 *      ONE product per multiply-add on the f16 MFMA, fp32 accumulation: a third of mode 1's MFMAs and no lo
 *      conversions; per-layer relative error ~2^-11, SDF error ~1e-5 against the 1e-4 bar (features ~1e-3).
 *      The backward of decode_pts keeps the split arithmetic. */
/* The process DEFAULT: used by calls whose grid says mlp_mode = 0 (bnv_decode_dense: whose mlp_mode argument is 0).
 * A plain atomic word: setting it while another thread launches with mlp_mode = 0 changes that thread's arithmetic --
 * state the mode in the grid where that matters. */
int bnv_set_mlp_mode(int mode);
int bnv_get_mlp_mode(void);

/* Tuning switches (A/B experiments; defaults are the measured-best):
 *   "lattice_pipe"  1 (default): lattice-table MLP of modes 1 and 3 runs k_lattice_table_x (v_mfma_f32_16x16x32_f16,
 *                  operands prefetched across tiles and layers, dynamic tile hand-out); 0: the generic
 *                  k_decode<LATTICE> (32x32x16 MFMA; the same arithmetic in another summation grouping: tables equal
 *                  to ~1e-8, 8-10 % slower);
 *   "fused_mark"   -1 (default): bnv_decode_lattice looks the 27 neighbour rows up inside the live-entry marking kernel
 *                  for calls of up to 49,152 voxels and in a launch of its own above; 1 / 0 force either.
 *   "tcnn_block_encoder"  1 (default): whole-frame encodes with the tiny-cuda-nn networks run k_pointnet_scatter_tb
 *                  (32-point blocks x 8 corners, per-wave LDS accumulation of the voxel sums); 0: the per-tile kernel.
 *   "tcnn_shared_table"  1 (default): that kernel's 8 waves take the 8 blocks of a 16 x 16-pixel patch and sum them in
 *                  ONE LDS table per workgroup (flushed behind a barrier); 0: one table per wave, flushed per block.
 *   "finalize_blocks"  0 (default): the encoder's compaction kernel runs on 2 workgroups of 1,024 threads per CU
 *                  striding over its tiles; n > 0: on n workgroups, clamped to that same 2 per CU (tests force many
 *                  strides per workgroup with a small n).  The clamp is a forward-progress requirement, not a tuning
 *                  choice: a tile waits for its predecessor's look-back word, so every launched workgroup must be
 *                  resident at once.
 *   "reserve_cus"  0 (default); n: the persistent MLP kernels launch on (CUs - n) workgroups, leaving n CUs to
 *                  kernels of other streams (measured on one GPU with the two-stream frame pipeline: no gain for
 *                  n = 4, 8, 16 -- tools/ab_reserve.py; meant for an RCCL collective that must progress beside
 *                  the decode in the multi-GPU mode).
 * Unknown names return BNV_ERR_INVALID_ARGUMENT.  The switches are process-wide atomic words read at launch time:
 * they select between implementations that produce the same results (A/B timing), never the arithmetic. */
int bnv_set_option(const char* name, int value);

/* Optional timing of the dominant kernels with HIP events recorded on their launch stream.
 * kinds: 0 point-encoder MLP + scatter, 1 lattice-table SDF MLP, 2 decode_pts SDF MLP,
 * 3 dense-decode SDF MLP.  bnv_profile_read synchronises the recorded events and returns the
 * summed kernel time (ms) and launch count per kind since bnv_profile_enable(1). */
int bnv_profile_enable(int on);
int bnv_profile_read(double* total_ms_host /*[4]*/, int64_t* launches_host /*[4]*/);

/* Diagnostic (bench.py; no reference counterpart): the rate of f16 MFMAs this GPU sustains when NOTHING but
 * MFMAs is issued -- shape 0 = v_mfma_f32_32x32x16_f16 (`iters` x 12 per wave), 1 = v_mfma_f32_16x16x32_f16
 * (`iters` x 24: the same FLOPs), every CU, two waves per SIMD, operands 0 = zeros, 1 = uniform random f16.  The frame's MLP kernels run at the package power limit, where the clock (and the dense
 * MFMA rate) settles below the 2.4 GHz the 2.5 PFLOP/s peak is quoted at; this gives the ceiling that is actually
 * attainable on the box (the 16x16x32 form sustains ~14 % more than the 32x32x16 form), next to which bench.py
 * reports the dominant kernel.  Synchronises on `stream`; writes the
 * elapsed milliseconds and the FLOPs issued (2 x 32 x 32 x 16 per MFMA) to host memory. */
int bnv_probe_mfma_rate(int shape, int operands, int iters, void* stream, double* ms_host, double* flop_host);
/* Diagnostic: n_blocks single-wave workgroups that spin for `cycles` shader cycles on `stream`.  The runtime maps HIP
 * streams onto a few hardware queues (GPU_MAX_HW_QUEUES, default 4) and two streams that share one are served
 * strictly in submission order; one spin on each of two streams, timed with events, tells whether they overlap.  The
 * frame pipeline picks its encode stream that way (bnv_fusion_amd/streams.py). */
int bnv_probe_spin(int n_blocks, int64_t cycles, void* stream);

/* ---- front end: depth image -> input_pts (FusionInferenceAbstractDataset.__getitem__,
 * src/datasets/fusion_inference_dataset.py:40-90; geometry.py:150-171; kornia depth_to_normals) --------
 * depth [H,W]: dtype 0 = uint16 millimetres (the dataset's PNG, /1000. as common.py:93), 1 = float32
 * metres, 2 = float64 metres.  intr 3x3 and T_wc 4x4 row-major float64 on the HOST.  Float64
 * arithmetic in the reference's order, rounded once to float32; out_pts [n_out, 6] holds the valid
 * pixels (0 < depth < max_depth) in row-major order, capacity H*W rows; n_out is a device int32. */
size_t bnv_depth_workspace_bytes(int H, int W);
/* pad != 0: the rows [n_out, H*W) of out_pts are set to NaN by the same launch (a caller that hands the whole
 * H*W-row buffer on without reading n_out -- the encoder's bounds mask drops NaN rows -- needs no separate fill).
 * Depth-confidence gate (FusionInferenceDatasetARKit, fusion_inference_dataset.py:242-306): conf [H,W] uint8 on the
 * device (ARKit: 0 / 1 / 2); a pixel is a row when 0 < depth < max_depth AND conf >= conf_level.  The confidence
 * removes rows only: the normals' Sobel stencil still reads the depth of rejected neighbours.  conf NULL with
 * conf_level 0: no gate; conf NULL with conf_level > 0 (or conf_level < 0) is BNV_ERR_INVALID_ARGUMENT. */
int bnv_depth_to_points(const void* depth, int depth_dtype, int H, int W, const double* intr_host,
                        const double* T_wc_host, double max_depth, const uint8_t* conf, int conf_level, int pad,
                        void* ws, size_t ws_bytes, float* out_pts, int32_t* n_out, bnv_stream_t stream);

/* ---- TSDF side fusion: TSDFVolume.integrate (third_parties/fusion.py:68-141, called per frame from
 * run_e2e.py:99-109).  tsdf / weight / color [dx,dy,dz] f32 (color may be NULL); depth [h,w] (0 = invalid) with the
 * front end's dtype codes: 1 = float32 metres, 0 = uint16 millimetres as the dataset stores them, converted per sample
 * as depth_mm / 1000 (common.py:93) inside the kernel -- no float copy of the frame; any other depth_dtype is
 * BNV_ERR_INVALID_ARGUMENT; color_im [h,w] f32 folded b*65536+g*256+r or NULL; intr 3x3 and pose 4x4 row-major f32 on
 * the HOST; trunc_margin = 5 * voxel_size in the reference.  max_depth > 0: samples with depth >= max_depth are
 * invalid too -- the reference's loader zeroes them before the frame reaches either fusion (common.py:110-113 with
 * max_depth = model.ray_tracer.ray_max_dist, fusion_inference_dataset.py:28); <= 0: no cut.  gate: device int32 or
 * NULL; when *gate == 0 the launch does nothing -- NeuralMap.integrate returns before the TSDF fusion when the
 * encode found no in-bounds point (run_e2e.py:91-92), and the pipelined host does not know that count yet. */
int bnv_tsdf_integrate(float* tsdf, float* weight, float* color, const int32_t dim_host[3],
                       const float origin_host[3], float voxel_size, float trunc_margin,
                       const void* depth, int depth_dtype, const float* color_im, int im_h, int im_w,
                       const float intr_host[9], const float pose_host[16], float obs_weight,
                       float max_depth, const int32_t* gate, bnv_stream_t stream);
/* n_frames (<= BNV_TSDF_BATCH_MAX) consecutive uint16 depth frames in ONE launch: identical to n_frames calls of
 * bnv_tsdf_integrate (depth_dtype 0) in order.  depth_mm: HOST array of device pointers; color / color_im: the colour volume and a
 * HOST array of device pointers to the frames' folded colour images (entries may be NULL), or both NULL;
 * intr_host [n_frames, 9] and pose_host [n_frames, 16] row-major f32 on the host. */
#define BNV_TSDF_BATCH_MAX 8
int bnv_tsdf_integrate_batch_u16(float* tsdf, float* weight, float* color, const int32_t dim_host[3],
                                 const float origin_host[3], float voxel_size, float trunc_margin, int n_frames,
                                 const uint16_t* const* depth_mm, const float* const* color_im, int im_h, int im_w,
                                 const float* intr_host,
                                 const float* pose_host, float obs_weight, float max_depth, bnv_stream_t stream);

/* ---- spatially sharded volume: the exchange step (new design; bnv_fusion_amd/distributed.py).
 * Voxels are owned by hash(block coordinate) % shard_world (bnv_grid_t).  Per frame every rank sends the rows it has
 * just updated that are BOUNDARY voxels (a voxel of their 3x3x3 neighbourhood belongs to another rank), one
 * all-gather moves the blocks, every rank installs the records adjacent to voxels it owns as ghost rows.
 * A block is (1 + capacity) records of BNV_SHARD_RECORD_BYTES: record 0 is the header {int32 count, int32 sender
 * rank, int32 overflow flag}; a record is {int32 x, y, z; float weight; float feature[8]}.
 *   bnv_shard_pack     coords [n, 3] i64 = this frame's emitted voxels (n_dev: device count or NULL), values read
 *                      from the volume AFTER the frame's upsert; capacity >= the bound bnv_encode_begin leaves in the
 *                      workspace for this rank;
 *   bnv_shard_install  blocks = world blocks back to back (the all-gather's output); the own block is skipped; a
 *                      sender's overflow flag sets the volume's sticky error word to 4.  The header count of
 *                      own_send_block (the block this rank contributed to `blocks`; NULL: none) is set back to 0: the
 *                      block is then ready for the records bnv_volume_integrate appends for the next frame. */
#define BNV_SHARD_RECORD_BYTES 48
int bnv_shard_pack(const bnv_volume_t* vol, const bnv_grid_t* grid, const int64_t* coords, int64_t n,
                   const int32_t* n_dev, void* block, int64_t capacity, bnv_stream_t stream);
int bnv_shard_install(const bnv_volume_t* vol, const bnv_grid_t* grid, const void* blocks, int world,
                      int64_t capacity, void* own_send_block, bnv_stream_t stream);

/* ---- encode: LitFusionPointNet.encode_pointcloud (local_point_fusion.py:81-165) ------------ */

/* Bytes of scratch bnv_encode_pointcloud needs for up to max_points input points.  The scratch is
 * laid out for the max_points it was sized for: pass that same value as ws_max_points.
 * DESIGN LIMIT: the sorted-unique of the touched voxels is a bitmap rank, not a sort, so the scratch holds one
 * byte + one bit per voxel of the GRID (16.7 MB + 2 MB at 256^3, 134 MB + 16 MB at 512^3) next to the O(points)
 * arrays, flat voxel ids are int32, and grids of 2^31 voxels or more are rejected with BNV_ERR_INVALID_ARGUMENT
 * (about 1290^3).  The reference's torch.unique is O(points) with int64 ids (local_point_fusion.py:116-119) and has
 * no such bound; every BASELINE configuration (<= 512^3) is far inside it. */
size_t bnv_encode_workspace_bytes(int64_t max_points, const int32_t n_xyz[3]);

/* Packed-weight sizes (floats) of the fp32 point encoder / SDF decoder; layouts in DESIGN.md. */
size_t bnv_pointnet_pack_floats(void);
size_t bnv_sdfmlp_pack_floats(void);

/* The encode in two halves (bnv_encode_pointcloud below = begin + finish on the same arguments; everything between
 * the halves lives in the workspace):
 *   begin   bounds mask (local_point_fusion.py:94-104), 8-corner voxelisation (:153-165, modules.py:586-655) into a
 *           grid bitmap, sorted-unique of the touched voxels by bitmap rank (torch.unique, :118-119);
 *   finish  the point encoder on every (point, corner) pair, per-voxel mean, min-points filter, ordered repack.
 * bnv_encode_begin_depth fuses the depth front end in front of `begin` (depth, conf and conf_level as for
 * bnv_depth_to_points; conf NULL with conf_level 0: no gate): it writes input_pts rows IN PIXEL ORDER into out_pts
 * [H*W, 6] (NaN rows for invalid or rejected pixels -- nothing is compacted; the bounds mask drops NaN rows wherever
 * they are) and marks the voxels from registers; n_points of the matching finish call is H*W.
 * bnv_encode_finish, image_width: > 0 with n_points a multiple of it says that the points are the pixels of an image in
 * row-major order (the out_pts of bnv_encode_begin_depth) and lets the encoder work on 2-D pixel patches (the
 * tiny-cuda-nn encoder accumulates a patch's per-voxel sums on chip before touching the global accumulators:
 * neighbouring pixels in BOTH directions share voxels); 0 = no such structure.  Results are identical either way
 * (integer sums).
 * With spatial sharding (grid.shard_world > 1) `begin` also leaves, at byte offset bnv_encode_shard_counts_offset()
 * of the workspace, int32[shard_world]: the number of touched BOUNDARY voxels each rank owns (voxels with a foreign
 * voxel in their 3x3x3 neighbourhood).  The voxelisation is replicated, so every rank holds the same numbers: an
 * upper bound, known before the encoder runs, of the boundary records each rank exchanges for the frame
 * (bnv_shard_pack).  `finish` clears them. */
int bnv_encode_begin(const float* input_pts, int64_t n_points, const bnv_grid_t* grid_host, void* ws, size_t ws_bytes,
                     int64_t ws_max_points, bnv_stream_t stream);
int bnv_encode_begin_depth(const void* depth, int depth_dtype, int H, int W, const double* intr_host,
                           const double* T_wc_host, double max_depth, const uint8_t* conf, int conf_level,
                           const bnv_grid_t* grid_host, void* ws, size_t ws_bytes, int64_t ws_max_points,
                           float* out_pts, bnv_stream_t stream);
int bnv_encode_finish(const float* input_pts, int64_t n_points, int image_width, const bnv_grid_t* grid_host,
                      const float* pointnet_pack, void* ws, size_t ws_bytes, int64_t ws_max_points,
                      float* out_feats, int64_t* out_pcounts, int64_t* out_flat_ids, int64_t* out_grid_ids,
                      int64_t out_capacity, int emit_all, bnv_encode_counters_t* counters, bnv_stream_t stream);
size_t bnv_encode_shard_counts_offset(void);

/* input_pts [n_points, 6] f32 (world xyz, world normal).
 * Runs: bounds mask (:94-104), 8-corner voxelisation (:153-165, modules.py:586-655), the point
 * encoder on every (point, corner) pair (pointnet_utils.py:246-266, BatchNorm folded), sorted
 * unique voxel ids + counts (torch.unique, :118-119), per-voxel mean (torch_scatter.scatter_mean,
 * :125), min-points filter and repack (:143-151).
 * Outputs (capacity rows each): feats [.,8] f32, pcounts [.] i64, flat_ids [.] i64 ascending,
 * grid_ids [.,3] i64.  emit_all != 0 writes all U voxels with features zeroed where
 * count < min_pts (the return_dense=True contract, :126-141). */
int bnv_encode_pointcloud(const float* input_pts, int64_t n_points, const bnv_grid_t* grid_host,
                          const float* pointnet_pack, void* ws, size_t ws_bytes,
                          int64_t ws_max_points, float* out_feats, int64_t* out_pcounts, int64_t* out_flat_ids,
                          int64_t* out_grid_ids, int64_t out_capacity, int emit_all,
                          bnv_encode_counters_t* counters, bnv_stream_t stream);

/* get_relative_xyz + flatten for every pair, pair index p = corner * n_points + i
 * (local_point_fusion.py:106-117, voxel_utils.py:62-65).  No bounds mask (the caller compacts).
 * grid_ids [8n,3] i32, flat_ids [8n] i64, rel_xyz [8n,3] f32 = (xn - grid_id) * voxel_size.
 * Any output may be NULL. */
int bnv_voxelize_pairs(const float* input_pts, int64_t n_points, const bnv_grid_t* grid_host,
                       int32_t* grid_ids, int64_t* flat_ids, float* rel_xyz, uint8_t* bound_mask,
                       bnv_stream_t stream);

/* ---- volume: SparseVolume (sparse_volume.py:484-695) ---------------------------------------- */

int bnv_volume_clear(const bnv_volume_t* vol_host, bnv_stream_t stream);
/* Rebuild the slot table from row_coords[0:n_rows) (after the caller enlarged it). */
int bnv_volume_rehash(const bnv_volume_t* vol_host, bnv_stream_t stream);
size_t bnv_volume_workspace_bytes(int64_t max_keys);
/* Keys per workgroup of bnv_volume_integrate's single launch as this library was built (BNV_INT_THREADS): new rows are
 * numbered per workgroup and chained across workgroups, so frame sizes around its multiples are the edges of that
 * numbering (what tests size their frames by; nothing a caller has to respect). */
int bnv_volume_integrate_tile_keys(void);

/* LitFusionPointNet._integrate + _update (local_point_fusion.py:647-673) fused with
 * SparseVolume.query/insert (sparse_volume.py:561-585, 661-695): for n UNIQUE keys,
 * w = min(count/32, 1); f = (f_old*w_old + f*w)/(w_old + w); upsert.  coords [n,3] i64,
 * feats [n,8], pcounts [n] i64.  If n_dev (a device int32, e.g. &counters->n_out of the encode that
 * produced the inputs) is not NULL the element count is read on the device and n is only the
 * capacity the launch is sized for -- no host synchronisation between encode and integrate. */
/* extras_host (NULL: none of this) serves the per-frame pipeline: the same single launch then also (a) marks the rows
 * it touches as the ORIGINS of the frame's lattice decode in `lattice_ws` (the workspace bnv_decode_lattice is then
 * called with, prestamped and with the same stamp_epoch != 0; NULL: no stamps) and (b) with a sharded volume appends
 * the boundary voxels among the upserted keys -- with the values just written -- to shard_block as bnv_shard_pack would
 * (header count must be 0 or hold the records of this frame so far: bnv_shard_install leaves it so; NULL: no records).
 * Replaces the launches of k_lattice_stamp and bnv_shard_pack (local_point_fusion.py:647-673 has no counterpart of
 * either: new design). */
typedef struct bnv_integrate_extras {
  void* shard_block;             /* (1 + shard_block_capacity) records of BNV_SHARD_RECORD_BYTES, or NULL */
  int64_t shard_block_capacity;
  const bnv_grid_t* grid_host;   /* ownership predicates; needed with shard_block */
  void* lattice_ws;              /* lattice-decode workspace sized for vol->row_capacity, or NULL */
  int32_t stamp_epoch;
} bnv_integrate_extras_t;
int bnv_volume_integrate(const bnv_volume_t* vol_host, const int64_t* coords, const float* feats,
                         const int64_t* pcounts, int64_t n, const int32_t* n_dev, void* ws, size_t ws_bytes,
                         const bnv_integrate_extras_t* extras_host, bnv_stream_t stream);

/* The same for up to BNV_VOLUME_BATCH_MAX consecutive frames in ONE call (4 launches): the result -- row order, row
 * count, features, weights -- is identical to calling bnv_volume_integrate once per frame in order (the replay loop of
 * the frame-parallel multi-GPU mode, and any caller that holds several encoded frames; the reference integrates one
 * frame per call, local_point_fusion.py:647-673).  coords / feats / pcounts / n / n_dev: HOST arrays of n_frames
 * device pointers / counts (n_dev may be NULL, or hold NULLs).  slot_mask [n_slots] u32 and slot_items
 * [n_slots * BNV_VOLUME_BATCH_MAX] i32 are side tables that belong to the volume: slot_mask must be all zeros
 * before the first call (it is all zeros again after every call) and both must be re-made when the slot table is.
 * Workspace: bnv_volume_workspace_bytes(sum over frames of n rounded up to 256). */
#define BNV_VOLUME_BATCH_MAX 8
int bnv_volume_integrate_batch(const bnv_volume_t* vol_host, int n_frames, const int64_t* const* coords,
                               const float* const* feats, const int64_t* const* pcounts, const int64_t* n,
                               const int32_t* const* n_dev, uint32_t* slot_mask, int32_t* slot_items,
                               void* workspace, size_t workspace_bytes, bnv_stream_t stream);
/* SparseVolume.insert (upsert with explicit values), sparse_volume.py:561-585.  A key may occur several times in one
 * call: it gets ONE row, numbered at its first occurrence, holding the values of its last occurrence (what inserting
 * the occurrences one by one gives).  n < 2^31 - 256. */
int bnv_volume_insert(const bnv_volume_t* vol_host, const int64_t* coords, const float* feats,
                      const float* weights, const float* num_hits, int64_t n, void* ws,
                      size_t ws_bytes, bnv_stream_t stream);
/* SparseVolume.query / _query_tensor (sparse_volume.py:625-695): zeros for absent keys.
 * Values are read from (features, weights, num_hits) given here -- the live arrays or a
 * to_tensor() snapshot; rows >= row_limit count as absent.  out_rows (optional) gets the row or -1. */
int bnv_volume_query(const bnv_volume_t* vol_host, const int64_t* coords, int64_t n,
                     const float* features, const float* weights, const float* num_hits,
                     int64_t row_limit, float* out_feats, float* out_weights, float* out_hits,
                     int32_t* out_rows, bnv_stream_t stream);
/* SparseVolume.count_optim (sparse_volume.py:602-622): weights[row] += 1 once per distinct row. */
int bnv_volume_count_optim(const bnv_volume_t* vol_host, const int64_t* coords, int64_t n,
                           float* weights, int64_t row_limit, int32_t* stamp, int32_t epoch,
                           bnv_stream_t stream);

/* ---- decode --------------------------------------------------------------------------------- */

/* Optional TSDF prior sampled by nearest grid_sample (sparse_volume.py:819-832). */
typedef struct bnv_sdf_delta {
  const float* data; /* [dx, dy, dz] or NULL */
  int32_t dims[3];
} bnv_sdf_delta_t;

/* SparseVolume.decode_pts (sparse_volume.py:768-833) at arbitrary points: coords [n,3] f32,
 * voxel units if is_coords else world; out [n] f32.  split_mask NULL: one split, the plain weights (split_samples is
 * then ignored); else the ray splits of an optimiser step, see bnv_volume_count_optim_splits below. */
int bnv_decode_pts(const bnv_volume_t* vol_host, const bnv_grid_t* grid_host, const float* features,
                   const float* weights, int64_t row_limit, const float* sdfmlp_pack, const float* coords,
                   int64_t n, int is_coords, const bnv_sdf_delta_t* delta_host, const uint32_t* split_mask,
                   int64_t split_samples, float* out_sdf, bnv_stream_t stream);

/* Backward of bnv_decode_pts with respect to the volume features -- the autograd edge the global
 * optimiser relies on: run_e2e.py:111-162 turns volume.features into an nn.Parameter and
 * back-propagates render_utils.py:551-590 (calculate_loss) through SparseVolume.decode_pts
 * (sparse_volume.py:768-833).  grad_sdf [n] = d loss / d out_sdf; grad_features [row_limit, 8] is
 * ACCUMULATED into (the caller zeroes it).  The decoder weights are frozen and the points are data, so
 * nothing else receives gradient; sdf_delta is additive and does not enter.  sdfmlp_bwd_pack holds the
 * transposed layers: bnv_sdfmlp_bwd_pack_floats() floats for the fp32 decoder (weights.py: pack_sdf_mlp_bwd),
 * bnv_sdfmlp_tcnn_bwd_pack_floats() for the tiny-cuda-nn decoder of MLP mode 2 (pack_sdf_tcnn_bwd).  split_mask /
 * split_samples as for bnv_decode_pts. */
size_t bnv_sdfmlp_bwd_pack_floats(void);
size_t bnv_sdfmlp_tcnn_bwd_pack_floats(void);
int bnv_decode_pts_backward(const bnv_volume_t* vol_host, const bnv_grid_t* grid_host,
                            const float* features, const float* weights, int64_t row_limit,
                            const float* sdfmlp_pack, const float* sdfmlp_bwd_pack, const float* coords,
                            int64_t n, int is_coords, const uint32_t* split_mask, int64_t split_samples,
                            const float* grad_sdf, float* grad_features, bnv_stream_t stream);

/* ---- dataset formats (host only) ----------------------------------------------------------------- */

/* Reverses the PNG scanline filters of an inflated IDAT stream (the reference reads its 16-bit depth PNGs with
 * cv2.imread(path, -1), src/utils/common.py:93; bnv_fusion_amd/datasets.py parses the container).  raw: height
 * scanlines of 1 filter byte + row_bytes data bytes; bpp: bytes per pixel; out: height * row_bytes bytes. */
int bnv_png_unfilter(const uint8_t* raw, int height, int row_bytes, int bpp, uint8_t* out);

/* ---- global optimiser: ray sampling + SDF ray loss, fused ------------------------------------------ */

/* One ray split of render_utils.py:461-549 up to the decode.  Per ray: the ray through pixel uv
 * (get_camera_params / lift, :411-458; T_wc 4x4 and intr 3x3 row-major on the host), n_fine stratified
 * samples within +-truncated_dist of the observed surface point gt_pts and n_coarse between the camera and
 * it (hierarchical_sampling, :191-233; u_fine / u_coarse are the uniforms in [0,1) of the strata, supplied
 * by the caller), merged by distance -> pts [n, S, 3] (S = n_fine + n_coarse <= 64).  Per sample the L1
 * target of compute_sdf_loss (:508-549): +-distance to the nearest valid neighbour point (nb_pts
 * [n, n_nb, 3], nb_mask [n, n_nb]) clipped to +-truncated_dist, and weight = valid * ray_mask. */
int bnv_ray_samples(const float* uv, const float* gt_pts, const float* ray_mask, const float* nb_pts,
                    const float* nb_mask, int n_nb, const float T_wc[16], const float intr[9],
                    const float* u_fine, const float* u_coarse, int n, int n_fine, int n_coarse,
                    float truncated_dist, float* pts, float* target, float* weight, bnv_stream_t stream);
/* loss += sum_i weight_i |pred_i - target_i| / *n_valid (device scalars; loss is accumulated atomically)
 * and grad_i = d loss / d pred_i.  split_samples 0: one split; > 0: sample i belongs to split i / split_samples and
 * n_valid holds one scalar per split. */
int bnv_ray_loss(const float* pred, const float* target, const float* weight, const float* n_valid, int64_t m,
                 int64_t split_samples, float* loss, float* grad, bnv_stream_t stream);
/* SparseVolume.count_optim on the 8 corner voxels of m sample points (render_utils.py:491-493,
 * sparse_volume.py:602-622): weights[row] += 1 once per distinct row. */
int bnv_volume_count_optim_pts(const bnv_volume_t* vol_host, const bnv_grid_t* grid_host, const float* pts,
                               int64_t m, int is_coords, float* weights, int64_t row_limit,
                               int32_t* stamp, int32_t epoch, bnv_stream_t stream);

/* ---- one optimiser step in a handful of launches (round 6).  NeuralMap.optimize (run_e2e.py:111-162) cuts a step's
 * 5,000 rays into splits of train_ray_splits = 1,000 and runs render_with_rays -> count_optim -> decode_pts -> loss ->
 * backward split by split (render_utils.py:461-590).  What couples the splits is count_optim: a split's mask
 * decisions (min over the 8 corner weights >= min_pts, sparse_volume.py:816-818) see the +1s of the splits before it
 * and its own.  These entries run ALL splits of a step together and keep every decision: sample q belongs to split
 * q / split_samples (at most 31 splits);
 *   bnv_volume_count_optim_splits  bit s of split_mask[row] (uint32 per row of the to_tensor() snapshot, zeroed once by
 *                                  the caller) = split s touches the row; weights are NOT changed yet;
 *   bnv_decode_pts / bnv_decode_pts_backward   with that split_mask, the corner weights are
 *                                  weights[row] + 1 per split <= the query's that touches the row (exact fp32 adds);
 *   bnv_ray_loss                   with split_samples, one n_valid per split;
 *   bnv_optim_step                 forward + loss + backward of all samples in ONE kernel (fp32 decoder, split-f16
 *                                  arithmetic as bnv_decode_pts_backward): the L1 loss is elementwise, so a query's
 *                                  gradient is known in the tile that computes its value.  loss_and_counter: float[2],
 *                                  zeroed by the caller -- [0] accumulates the sum of the splits' losses, [1] is the
 *                                  kernel's chunk counter; pred (optional) [n] gets the decoded SDF; grad_features is
 *                                  accumulated into like bnv_decode_pts_backward's;
 *   bnv_volume_apply_split_counts  weights[row] += 1 per set bit (sequential adds), masks cleared: the state the
 *                                  split-by-split sequence leaves. */
int bnv_volume_count_optim_splits(const bnv_volume_t* vol_host, const bnv_grid_t* grid_host, const float* pts, int64_t m,
                                  int is_coords, int64_t row_limit, int64_t split_samples, uint32_t* split_mask,
                                  bnv_stream_t stream);
int bnv_volume_apply_split_counts(float* weights, uint32_t* split_mask, int64_t n_rows, bnv_stream_t stream);
int bnv_optim_step(const bnv_volume_t* vol_host, const bnv_grid_t* grid_host, const float* features,
                   const float* weights, int64_t row_limit, const float* sdfmlp_pack, const float* sdfmlp_bwd_pack,
                   const float* pts, int64_t n, int is_coords, const bnv_sdf_delta_t* delta_host,
                   const uint32_t* split_mask, int64_t split_samples, const float* target, const float* sample_weight,
                   const float* n_valid, float* loss_and_counter, float* pred, float* grad_features,
                   bnv_stream_t stream);

/* ---- per-voxel marching cubes on decoded lattices -------------------------------------------- */

/* SparseVolume.meshlize after the decode (sparse_volume.py:740-756): for every voxel whose 3x3x3
 * lattice sdf [n, 27] straddles `level` (max > level and min < level) the 8 cells are triangulated;
 * vertex = level crossing of a lattice edge (linear), in world units:
 * ((index + t) * 0.5 + origin - 0.5) * voxel_size + min_coords.  tri_table: int8 [256, 16] edge triples,
 * -1 terminated (bnv_fusion_amd/mc_tables.py; scikit-image's Lewiner tables are not available here, so
 * the triangulation inside ambiguous cells is that table's).  Two passes: bnv_mc_count writes the
 * triangle count of every voxel; the caller prefix-sums them (exclusive, int64) and sizes `vertices`
 * [3 T, 3] f32; bnv_mc_emit writes the triangle soup in voxel / cell / table order. */
int bnv_mc_count(const float* sdf, int64_t n, const int32_t* n_dev, float level, const int8_t* tri_table,
                 int32_t* counts, bnv_stream_t stream);
int bnv_mc_emit(const float* sdf, const int64_t* origins, int64_t n, const int32_t* n_dev, float level,
                float voxel_size, const float min_coords[3], const int8_t* tri_table,
                const int64_t* tri_offsets, float* vertices, bnv_stream_t stream);
/* The same meshes with shared vertices, laid out as SparseVolume.meshlize concatenates them
 * (sparse_volume.py:740-756): per voxel one vertex per sign-changing edge of its 3x3x3 lattice (ascending lattice-edge
 * order: x edges, y edges, z edges, node-major) and faces that index them, offset by the vertex counts of the voxels
 * before it (the reference's `faces + last_face_id; last_face_id += max(faces) + 1`).  count -> the caller's
 * exclusive prefix sums (vert_offsets, tri_offsets [n] i64) -> emit into vertices [V, 3] f32, faces [T, 3] i64. */
int bnv_mc_count_indexed(const float* sdf, int64_t n, const int32_t* n_dev, float level, const int8_t* tri_table,
                         int32_t* n_verts, int32_t* n_tris, bnv_stream_t stream);
int bnv_mc_emit_indexed(const float* sdf, const int64_t* origins, int64_t n, const int32_t* n_dev, float level,
                        float voxel_size, const float min_coords[3], const int8_t* tri_table,
                        const int64_t* vert_offsets, const int64_t* tri_offsets, float* vertices, int64_t* faces,
                        bnv_stream_t stream);

/* ---- dense marching cubes over the TSDF side volume (TSDFVolume.get_mesh / get_point_cloud, third_parties/fusion.py:
 * 302-341; the reference runs skimage's marching_cubes_lewiner on a host copy).  tsdf, weight, color: the [X, Y, Z] f32
 * volumes of bnv_tsdf_integrate, read in place; dim = {X, Y, Z}.  The output is a WELDED mesh: one vertex per grid
 * edge whose end values straddle `level` (case bit c of the cell based at (i, j, k) is set when tsdf < level at corner
 * c = 4 dx + 2 dy + dz; tri_table and winding as bnv_mc_*: face normals point toward increasing TSDF, and inside
 * ambiguous cells the triangulation is that table's, not Lewiner's -- the vertex set is the same for both).  Vertex on
 * the edge a -> a + e_axis: t = (level - va) / (vb - va), world = fl32(fl32((a + t e_axis) * voxel_size) + origin);
 * normal = the np.gradient of the volume at both ends interpolated with t and normalised (0 for a zero gradient);
 * colour = color[rint(a + t e_axis)] unfolded to r, g, b uint8 as fusion.py:331-337.  Vertices are ordered by the
 * linear index of the owning (lower) grid point, then axis x, y, z; faces by the linear index of the cell's base, then
 * table order.  observed_only != 0: a cell emits only when its 8 corners have weight > 0 and a vertex exists only when
 * an emitting cell uses it (weight must then be non-NULL).  A volume with a dimension below 2 has no cell: V = T = 0.
 * Workspace: bnv_tsdf_mesh_workspace_bytes (< 1 B per grid point).  bnv_tsdf_mesh_count fills it and writes the
 * totals {V, T} to the device int64[2] `totals`; the caller reads them back to size the outputs and calls
 * bnv_tsdf_mesh_emit with the same volume, dim, level, observed_only and workspace: vertices [V, 3] f32 (required),
 * faces [T, 3] i64, normals [V, 3] f32, colors [V, 3] u8 -- each of the last three may be NULL (a point cloud skips
 * the faces and normals); color may be NULL (colours are then 0).  n_vertices / n_faces: the capacities of the
 * outputs (rows); nothing is written beyond them.  Neither entry allocates or synchronises; bad arguments return
 * BNV_ERR_INVALID_ARGUMENT before any HIP call. */
int bnv_tsdf_mesh_workspace_bytes(const int32_t dim[3], int64_t* bytes);
int bnv_tsdf_mesh_count(const float* tsdf, const float* weight, const int32_t dim[3], float level, int observed_only,
                        const int8_t* tri_table, void* workspace, int64_t ws_bytes, int64_t* totals,
                        bnv_stream_t stream);
int bnv_tsdf_mesh_emit(const float* tsdf, const float* weight, const float* color, const int32_t dim[3],
                       const float origin[3], float voxel_size, float level, int observed_only,
                       const int8_t* tri_table, const void* workspace, int64_t ws_bytes, int64_t n_vertices,
                       int64_t n_faces, float* vertices, int64_t* faces, float* normals, uint8_t* colors,
                       bnv_stream_t stream);

size_t bnv_decode_lattice_workspace_bytes(int64_t n_voxels, int64_t row_capacity);
/* Byte offset, inside that workspace, of two int32 device counters: [0] rows listed by
 * bnv_lattice_neighbors(build_list), [1] table entries (= MLP evaluations) listed by bnv_lattice_mark /
 * evaluated by the last bnv_decode_lattice (for FLOP accounting). */
size_t bnv_decode_lattice_count_offset(int64_t row_capacity);
/* The same decode for the 3x3x3 lattice {-0.5,0,0.5}^3 around n integer voxel origins
 * (SparseVolume.meshlize's decode_pts call, sparse_volume.py:717-738): out [n,27] f32.
 * Evaluates the MLP once per (corner voxel, local offset) instead of 8x per lattice point.
 * n_dev: optional device-side count as in bnv_volume_integrate (n = capacity).
 * prestamped != 0: bnv_volume_integrate (extras->lattice_ws, stamp_epoch) has already stamped the origins in `ws` with
 * this `epoch` (the origins are exactly the keys of that upsert): one launch less.  0: the call stamps them itself. */
int bnv_decode_lattice(const bnv_volume_t* vol_host, const bnv_grid_t* grid_host,
                       const float* features, const float* weights, int64_t row_limit,
                       const float* sdfmlp_pack, const int64_t* origins, int64_t n, const int32_t* n_dev,
                       const bnv_sdf_delta_t* delta_host, void* ws, size_t ws_bytes, int32_t epoch,
                       int prestamped, float* out_sdf, bnv_stream_t stream);

/* The three stages of bnv_decode_lattice, callable separately so that a sharded volume can exchange
 * corner-voxel tables between them (bnv_fusion_amd/distributed.py).  They share one workspace:
 *   neighbors: row of each of the 27 neighbour voxels of every origin (-1: absent or weight below
 *              min_pts); with build_list, appends each distinct usable row (not flagged in
 *              row_skip) to the work list;
 *   mark:      (single-volume path) flags the (row, l) table entries read by LIVE lattice points --
 *              all 8 corner voxels usable -- and lists them; masked points cost no MLP work;
 *   table:     table[row][l] = SDF-MLP(enc(l), features[row]) * voxel for every listed entry
 *              (use_entries) or all 27 l of every listed row;
 *   blend:     out[n,27] from the neighbour rows and the table. */
int bnv_lattice_neighbors(const bnv_volume_t* vol_host, const bnv_grid_t* grid_host, const float* weights,
                          int64_t row_limit, const int64_t* origins, int64_t n, const int32_t* n_dev,
                          const uint8_t* row_skip, int build_list, void* ws, size_t ws_bytes, int32_t epoch,
                          bnv_stream_t stream);
int bnv_lattice_mark(const bnv_volume_t* vol_host, int64_t n, const int32_t* n_dev, void* ws, size_t ws_bytes,
                     int32_t epoch, bnv_stream_t stream);
int bnv_lattice_table(const bnv_volume_t* vol_host, const bnv_grid_t* grid_host, const float* features,
                      const float* sdfmlp_pack, int64_t n_voxels, int use_entries, void* ws, size_t ws_bytes,
                      bnv_stream_t stream);
int bnv_lattice_blend(const bnv_volume_t* vol_host, const bnv_grid_t* grid_host, const int64_t* origins,
                      int64_t n, const int32_t* n_dev, const bnv_sdf_delta_t* delta_host, void* ws,
                      size_t ws_bytes, float* out_sdf, bnv_stream_t stream);
/* Byte offsets of the table [row_capacity,27] f32 and of the row work list inside the workspace. */
size_t bnv_decode_lattice_table_offset(int64_t row_capacity);
size_t bnv_decode_lattice_list_offset(int64_t n_voxels, int64_t row_capacity);

/* LitFusionPointNet.decode_feature_grid_w_pts (local_point_fusion.py:265-370) on dense grids feat_grid [8,X,Y,Z],
 * pts_weight [X,Y,Z]; voxel_coords [n,3] f32 (voxel units) -> out_sdf [n].  `variant` selects the reference's branch:
 *   BNV_DENSE_CORNERS  global_coords=False, interpolate_decode=True (:281-329, the yaml configuration): 8 corner
 *                      evaluations per query, blended; a corner counts when its weight >= min_pts_in_grid, the query is
 *                      valid when ANY corner counts, otherwise out = voxel_size.  out_feats must be NULL.
 *   BNV_DENSE_NEAREST  global_coords=False, interpolate_decode=False (:288-292, 331-343): ONE evaluation at the
 *                      nearest voxel (torch.round, half to even), valid when that voxel's weight >= min_pts_in_grid.
 *   BNV_DENSE_GLOBAL   global_coords=True, the signature default (:345-367): features by trilinear grid_sample
 *                      (align_corners=True, zero padding), weight by nearest; the MLP sees voxel_coords / (res - 1),
 *                      the prediction is NOT scaled by voxel_size; valid when the nearest weight >= min_pts_in_grid.
 * out_feats (optional, NEAREST / GLOBAL) [n,8]: the features the evaluation used (the reference's second return value).
 * status (optional, device int32[2]): status[1] = 5 when a feature leaves the certified range of the split arithmetic
 * (the range guard of bnv_decode_pts, which reports through the volume's error word).
 * mlp_mode: the arithmetic mode of the call in the bnv_grid_t.mlp_mode encoding (0 = process default,
 * BNV_GRID_MLP_MODE(m) = mode m).
 * gradient=True is not offered: the reference's branch (:367-369) reads an undefined name and cannot run. */
enum { BNV_DENSE_CORNERS = 0, BNV_DENSE_NEAREST = 1, BNV_DENSE_GLOBAL = 2 };
int bnv_decode_dense(const float* feat_grid, const float* pts_weight, const int32_t dims_host[3],
                     float voxel_size, int32_t min_pts_in_grid, const float* sdfmlp_pack,
                     const float* voxel_coords, int64_t n, int32_t variant, int32_t mlp_mode, float* out_sdf,
                     float* out_feats, int32_t* status, bnv_stream_t stream);

/* ---- the per-frame chain as one object: NeuralMap.integrate (run_e2e.py:78-109: encode_pointcloud -> track_n_pts ->
 * _integrate -> TSDF side fusion) followed by the lattice decode of the frame's voxels (sparse_volume.py:697-738),
 * for one GPU or for one shard of a spatially sharded volume.  Replaces the per-stage calls
 * above on the per-frame path: a frame in flight occupies a SLOT of caller-owned persistent buffers and runs on two
 * streams -- the encode (a function of the frame only) on encode_stream, the volume-dependent part on main_stream --
 * so frame t+1's encode overlaps frame t's exchange + decode, and no stage needs a host-side allocation, event object
 * or size read.  Per frame and slot, in this order (bnv_frame_begin_* of the NEXT frame may come before
 * bnv_frame_bound of this one: the encode side then runs a frame ahead of the host):
 *   bnv_frame_begin_depth | _points   front_stream (encode_stream if none): front end + voxelise + rank; exchange bound
 *                                     -> pinned memory; encode_stream: point encoder + reduction + filter; TSDF side
 *                                     fusion (depth frames, if configured)
 *   bnv_frame_upsert                  main_stream: upsert + running average (+ boundary records into the slot's send
 *                                     block, + decode-origin stamps when lattice_ws is given)
 *   bnv_frame_bound                   HOST wait for the frame's exchange bound (max over ranks; 0 unsharded)
 *   [sharded: the caller all-gathers the first (1 + capacity) records of every rank's send block on main_stream]
 *   bnv_frame_finish                  main_stream: install ghost rows from `blocks`, neighbour rows + live entries +
 *                                     table MLP of the lattice decode (when lattice_ws is given); blend_stream
 *                                     (main_stream if none): blend into the slot's sdf, read-backs into the slot's
 *                                     pinned words
 *   bnv_frame_result                  HOST wait for the frame; copies the slot's pinned words out; frees the slot
 * The volume and its workspaces are passed per call (they are re-made when the volume grows).  The object owns HIP
 * events only; every buffer is the caller's and must outlive it. */
#define BNV_PIPE_MAX_SLOTS 8
#define BNV_PIPE_HOST_WORDS 96
/* int32 words of a slot's pinned area */
#define BNV_PIPE_WORD_COUNTERS 0  /* [8]  bnv_encode_counters_t of the frame                                     */
#define BNV_PIPE_WORD_STATUS 8    /* [2]  {volume row count, sticky upsert error} behind the frame               */
#define BNV_PIPE_WORD_EVALS 10    /* [1]  SDF-MLP evaluations of the frame's decode                              */
#define BNV_PIPE_WORD_BOUNDS 16   /* [shard_world] touched boundary voxels per rank (the exchange bound)         */

typedef struct bnv_frame_slot {
  float* input_pts;                 /* [max_points, 6]: written by the depth front end (may be NULL: point frames only) */
  float* feats;                     /* [out_capacity, 8]  */
  int64_t* pcounts;                 /* [out_capacity]     */
  int64_t* flat_ids;                /* [out_capacity]     */
  int64_t* grid_ids;                /* [out_capacity, 3]  */
  bnv_encode_counters_t* counters;  /* device             */
  float* sdf;                       /* [out_capacity, 27] or NULL (never decoding)                               */
  void* send_block;                 /* sharded: (1 + send_capacity) records, header {0, rank, 0} before first use */
  int32_t* host_words;              /* PINNED HOST memory, BNV_PIPE_HOST_WORDS int32                             */
} bnv_frame_slot_t;

typedef struct bnv_tsdf_desc {      /* TSDFVolume (third_parties/fusion.py:19-66); tsdf == NULL: no side fusion   */
  float* tsdf;
  float* weight;
  float* color;
  int32_t dim[3];
  float origin[3];
  float voxel_size, trunc_margin;
} bnv_tsdf_desc_t;

typedef struct bnv_frame_pipe_config {
  bnv_grid_t grid;
  int64_t max_points;               /* largest frame (H * W)                                                      */
  int64_t out_capacity;             /* rows of the slots' output arrays (>= 8 * max_points / min_pts + 1)         */
  int64_t send_capacity;            /* records of the slots' send blocks.  out_capacity is enough for what a rank
                                       SENDS (its emitted boundary voxels); the exchange bound of bnv_frame_bound
                                       counts TOUCHED boundary voxels and can be larger (small or sparse frames): the
                                       caller exchanges min(bound rounded up, send_capacity) records per rank, and
                                       bnv_frame_finish rejects a block_capacity above send_capacity             */
  const float* pointnet_pack;
  void* enc_ws;                     /* bnv_encode_workspace_bytes(enc_ws_max_points, grid.n_xyz), zeroed once     */
  size_t enc_ws_bytes;
  int64_t enc_ws_max_points;
  double max_depth;                 /* depth cut-off of the loader (common.py:110-113)                            */
  bnv_tsdf_desc_t tsdf;
  int32_t n_slots;
  bnv_frame_slot_t slots[BNV_PIPE_MAX_SLOTS];
  bnv_stream_t encode_stream, main_stream;
  /* Round 4 (all optional; zero = the two-stream pipeline of round 3):
   *   front_stream  the front end (voxelise + rank + exchange bound) runs here instead of on encode_stream, so the
   *                 encoder of the next frame is ready as soon as this frame's has finished;
   *   enc_ws2       a second encode workspace (same size as enc_ws, zeroed once): frames alternate, and the front end
   *                 of a frame only waits for the encoder of the frame before the last one;
   *   blend_stream  the decode's blend + the frame's read-backs run here instead of on main_stream, which goes
   *                 straight on to the next frame's upsert; the caller must then pass bnv_frame_upsert /
   *                 bnv_frame_finish alternating decode workspaces (the pipe orders a workspace's reuse itself);
   *   encoder_workgroups  the persistent point encoder is launched on this many workgroups (one per CU; 0 = all
   *                 CUs): the CUs it leaves are where the small kernels of the other streams run meanwhile. */
  void* enc_ws2;
  bnv_stream_t front_stream, blend_stream;
  int32_t encoder_workgroups;
} bnv_frame_pipe_config_t;

typedef struct bnv_frame_pipe bnv_frame_pipe_t;
/* A frame's read-backs in one launch for callers that drive the stages themselves: the encode's counters (8 int32)
 * and the volume's {row count, sticky error} (bnv_volume_t.n_rows) -> host_words[0..9], PINNED host memory (written
 * through its device mapping; two small copies if it has none).  Valid once `stream` has passed this point. */
int bnv_readback_words(const int32_t* counters, const int32_t* status, int32_t* host_words, bnv_stream_t stream);

int bnv_frame_pipe_create(const bnv_frame_pipe_config_t* config_host, bnv_frame_pipe_t** out);
int bnv_frame_pipe_destroy(bnv_frame_pipe_t* pipe);
/* Arithmetic mode (bnv_grid_t.mlp_mode encoding) of the frames begun from now on; a frame in flight keeps the mode it
 * was begun with through its decode.  The mode config.grid carried at creation applies until this is called. */
int bnv_frame_pipe_set_mlp_mode(bnv_frame_pipe_t* pipe, int32_t grid_mlp_mode);
/* depth as bnv_encode_begin_depth (dtype 0 = uint16 mm, 1 = float32 m); color_im: folded colour image or NULL.  The
 * device buffers of a frame (depth, conf, color_im, input_pts) are read by kernels enqueued up to the frame's
 * bnv_frame_upsert (the TSDF side fusion): they must stay valid until the frame's result is in.
 * conf / conf_level: the confidence gate of bnv_encode_begin_depth (conf NULL with conf_level 0: no gate).  The TSDF
 * side fusion ignores the confidence, as the reference's does; it still runs only when the frame keeps an in-bounds
 * point after the gate. */
int bnv_frame_begin_depth(bnv_frame_pipe_t* pipe, int slot, const void* depth, int depth_dtype, int H, int W,
                          const double* intr_host, const double* T_wc_host, const uint8_t* conf, int conf_level,
                          const float* color_im);
int bnv_frame_begin_points(bnv_frame_pipe_t* pipe, int slot, const float* input_pts, int64_t n_points);
/* The TSDF side fusion (run_e2e.py:99-109) of a frame begun with bnv_frame_begin_points that ALSO carries its depth
 * image -- the reference dataset's frames hold input_pts, rgbd, intr_mat and T_wc together (run_e2e.py:78-109) -- gated
 * on the device by the frame's in-bounds point count like the depth path's.  Between the frame's begin and its upsert;
 * a no-op without a TSDF volume in the config.  depth_dtype 0 = uint16 mm, 1 = float32 m. */
int bnv_frame_side_depth(bnv_frame_pipe_t* pipe, int slot, const void* depth, int depth_dtype, int H, int W,
                         const double* intr_host, const double* T_wc_host, const float* color_im);
/* Abandons a frame that was begun but not upserted (an announced frame that never came, an error on the way): its
 * encode runs to its end and leaves the workspaces clean, nothing of it reaches the feature volume, the slot is free
 * again (the next frame begun in it waits for the abandoned work).  What the encode side has already done stays done:
 * a TSDF side fusion enqueued by begin, the owners a sharded volume's first-touch table gave to new blocks (the same
 * on every rank that began the frame). */
int bnv_frame_cancel(bnv_frame_pipe_t* pipe, int slot);
/* The caller has re-made its decode workspaces (the volume grew): the pipe forgets the pointers it has seen, after
 * ordering main_stream behind the frames that used them.  No frame may sit between its upsert and its finish. */
int bnv_frame_pipe_forget_workspaces(bnv_frame_pipe_t* pipe);
int bnv_frame_upsert(bnv_frame_pipe_t* pipe, int slot, const bnv_volume_t* vol_host, void* vol_ws, size_t vol_ws_bytes,
                     void* lattice_ws, int32_t lattice_epoch);
int bnv_frame_bound(bnv_frame_pipe_t* pipe, int slot, int32_t* max_bound_host);
int bnv_frame_finish(bnv_frame_pipe_t* pipe, int slot, const bnv_volume_t* vol_host, const void* blocks,
                     int64_t block_capacity, const float* sdfmlp_pack, const bnv_sdf_delta_t* delta_host,
                     void* lattice_ws, size_t lattice_ws_bytes, int32_t lattice_epoch);
int bnv_frame_result(bnv_frame_pipe_t* pipe, int slot, int32_t* words_host /* [BNV_PIPE_HOST_WORDS] or NULL */);
/* 1: bnv_frame_result would not block; 0: the frame is still running */
int bnv_frame_ready(bnv_frame_pipe_t* pipe, int slot);
/* Diagnostic: GPU timestamps of a frame's stages (tools/spatial_single_rank.py --timeline).  _enable(1) creates timing
 * events and records a base event on main_stream; every frame BEGUN afterwards records BNV_PIPE_TIMELINE_POINTS events
 * on its streams; bnv_frame_timeline, called after bnv_frame_result of that frame and before its slot is begun again,
 * returns their times in ms since the base (NaN: the frame did not pass that point).  Points: 0 front end starts,
 * 1 exchange bound copied (front stream), 2 encoder starts, 3 encoder done, 4 finalize done, 5 upsert starts (the
 * slot's encode has arrived on main_stream), 6 upsert done, 7 finish starts (the caller's all-gather is through),
 * 8 ghost rows installed, 9 table MLP done (marking + table), 10 blend + read-back done.  The extra marker packets
 * cost a few us per frame: off by default. */
#define BNV_PIPE_TIMELINE_POINTS 11
int bnv_frame_pipe_timeline_enable(bnv_frame_pipe_t* pipe, int on);
int bnv_frame_timeline(bnv_frame_pipe_t* pipe, int slot, float* ms_host /* [BNV_PIPE_TIMELINE_POINTS] */);

/* ---- Mesh evaluation (bnv_fusion_amd/csrc/eval.hip; the reference's metric: src/scripts/evaluate_bnvf.py:9-31 and
 * src/scripts/compute_chamfer.py:36-75 -- surface samples, nearest neighbours both ways, distances -> figures).
 * Every result is bitwise reproducible from run to run. */

/* Workspace bytes of bnv_mesh_sample_surface for a mesh of n_faces faces -> *bytes (host). */
int bnv_mesh_sample_surface_workspace(int64_t n_faces, int64_t* bytes);
/* trimesh.sample.sample_surface with caller-supplied uniforms: face areas 0.5 |e1 x e2| (fp32; a face whose area is
 * not finite counts as zero), their inclusive prefix in float64, face = the first whose prefix is STRICTLY greater
 * than u0 * total (a zero-area face is never chosen); (a, b) = (u1, u2), folded to (1 - a, 1 - b) when a + b > 1;
 * point = (v0 + e1 a) + e2 b in fp32 with e1 = v1 - v0, e2 = v2 - v0.  vertices fp32 [n_vertices, 3], faces int32
 * [n_faces, 3], uniforms fp32 [n, 3] in [0, 1) -> points_out fp32 [n, 3], face_ids_out int32 [n], normals_out (NULL:
 * not written) fp32 [n, 3] = (e1 x e2) / |e1 x e2|.  BNV_ERR_INVALID_ARGUMENT also when the mesh has no area or a
 * face indexes outside [0, n_vertices): the one check that reads device data, after the area scan -- so this entry
 * waits for `stream` once and is not capturable into a graph. */
int bnv_mesh_sample_surface(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces,
                            const float* uniforms, int64_t n, void* workspace, int64_t ws_bytes, float* points_out,
                            int32_t* face_ids_out, float* normals_out, bnv_stream_t stream);
/* Workspace bytes of bnv_nn_query: a function of the two counts alone -> *bytes (host). */
int bnv_nn_workspace_bytes(int64_t n_ref, int64_t n_query, int64_t* bytes);
/* Exact nearest neighbour of every query point among the reference points (fp32 [n, 3] each), on a uniform grid
 * built on the device: d2_out[i] is bitwise the minimum over the reference set of the fp32 expression
 * (dx*dx + dy*dy) + dz*dz with dx = q.x - r.x, and idx_out[i] the LOWEST reference index attaining it.  A reference
 * point with a NaN or Inf coordinate is never returned; a query with one (or a reference set without a finite point)
 * gets d2 = +inf and index -1.  No allocation, synchronisation or host read: capturable into a graph. */
int bnv_nn_query(const float* ref, int64_t n_ref, const float* query, int64_t n_query, void* workspace,
                 int64_t ws_bytes, float* d2_out, int32_t* idx_out, bnv_stream_t stream);

/* ---- Point-cloud normals (bnv_fusion_amd/csrc/cloud.hip): the [N, 6] rows the encoder takes, for points that come
 * without a pixel grid (a LiDAR scan, an exported cloud, a PLY of points).  The reference has no such entry: its
 * normals come from a depth image.  tests/cloud_restatement.py restates what follows in numpy; the kernel equals it
 * bit for bit, and two calls give the same bits.
 *
 * Neighbours.  A self-join on the index of bnv_nn_query: for point i the finite points j (i itself first) ordered by
 * (d2, j) lexicographically, d2 the fp32 (dx*dx + dy*dy) + dz*dz of bnv_nn_query -- the lowest index wins a tie.  The
 * first k of them; with max_radius > 0 those of them with d2 <= r2, r2 = the fp32 product max_radius * max_radius (an
 * infinite r2 is no radius).  m = how many: at most min(k, finite points).  A point with a NaN / Inf coordinate is
 * neither a query nor a neighbour.
 * Plane.  In float64, neighbours in that order, one rounding per written operation: mean = (0 + p_1 + ... + p_m) / m per
 * axis; the six moments a_xx, a_xy, a_xz, a_yy, a_yz, a_zz = (0 + sum of d_u d_v) / m with d = p - mean; V = I; then
 * BNV_CLOUD_JACOBI_SWEEPS cyclic Jacobi sweeps over the pairs (0,1), (0,2), (1,2).  The rotation of pair (p, q), r the
 * third index, skipped when a_pq == 0:  theta = (a_qq - a_pp) / (2 a_pq);  t = (theta >= 0 ? 1 : -1) / (|theta| +
 * sqrt(theta theta + 1));  c = 1 / sqrt(t t + 1);  s = t c;  h = t a_pq;  a_pp -= h;  a_qq += h;  a_pq = 0;
 * (a_rp, a_rq) = (c a_rp - s a_rq, s a_rp + c a_rq);  for every row i of V: (v_ip, v_iq) = (c v_ip - s v_iq, s v_ip +
 * c v_iq).  Eigenvalues = the diagonal: lambda_0 the smallest (the first index among equals), lambda_2 the largest
 * (the last index among equals), lambda_1 the remaining one; the normal = V's column of lambda_0.
 * Rejection.  m < min_neighbors; not a plane: !(lambda_1 > 1e-6 lambda_2) (coincident points: lambda_2 = 0; collinear
 * points: lambda_1 is rounding noise; a NaN anywhere); an origin index outside [0, n_origins).  A rejected row and a
 * non-finite row are six NaNs (the encoder's bounds mask drops them), variation NaN, n_neighbors m (0: non-finite).
 * Orientation.  Away from the sensor, as the depth front end's normals point: dot = (n_x (p_x - o_x) + n_y (p_y - o_y))
 * + n_z (p_z - o_z) in float64, o = origins[origin_index[i]] (origin 0 without origin_index); the normal is negated
 * when dot < 0, an exact zero keeps the solver's sign.
 * Outputs, in the input's row order: input_pts_out fp32 [n, 6] = (x, y, z copied, the normal rounded once to fp32);
 * variation_out (NULL: not written) fp32 [n] = max(lambda_0, 0) / ((lambda_0 + lambda_1) + lambda_2) rounded once;
 * n_neighbors_out (NULL: not written) int32 [n]; status_out int32 [4] (device): [0] rejected rows (non-finite ones
 * included), [1] rows whose origin index is out of range, [2], [3] zero.
 * points fp32 [n, 3], origins fp32 [n_origins, 3], origin_index int32 [n] or NULL (device).  k in [BNV_CLOUD_MIN_K,
 * BNV_CLOUD_MAX_K], 3 <= min_neighbors <= k, max_radius finite and >= 0 (0: none), n in [1, 2^31 - 3]; anything else
 * is BNV_ERR_INVALID_ARGUMENT before any HIP call, a workspace below bnv_cloud_normals_bytes (named like
 * bnv_mesh_simplify_bytes; ~84 B per point) BNV_ERR_WORKSPACE_TOO_SMALL.  No allocation, synchronisation or host read:
 * the caller reads status_out.  Capturable into a graph. */
#define BNV_CLOUD_MIN_K 8
#define BNV_CLOUD_MAX_K 32
#define BNV_CLOUD_JACOBI_SWEEPS 6
int bnv_cloud_normals_bytes(int64_t n_points, int64_t* bytes);
int bnv_cloud_normals(const float* points, int64_t n_points, int32_t k, float max_radius, int32_t min_neighbors,
                      const float* origins, int64_t n_origins, const int32_t* origin_index, void* workspace,
                      int64_t ws_bytes, float* input_pts_out, float* variation_out, int32_t* n_neighbors_out,
                      int32_t* status_out, bnv_stream_t stream);

/* ---- Signed distance to a triangle mesh (bnv_fusion_amd/csrc/meshsdf.hip): the exact distance from arbitrary points
 * to the mesh, everywhere (no truncation band), negative inside for outward-oriented faces.  The reference has no such
 * entry; bnv_fusion_amd/patches.py cuts embedding-training patches with it.
 *
 * Index.  vertices fp32 [n_vertices, 3], faces int32 [n_faces, 3] (device).  A face is skipped when an index lies
 * outside [0, n_vertices), when its fp32 area 0.5 |e1 x e2| is not positive and finite (the rule of
 * bnv_mesh_sample_surface: zero area, a NaN / Inf vertex) or when its cross product is exactly zero in float64.  Of
 * the others the index holds: unit face normals n_f (float64 from the fp32 positions); vertex pseudonormals sum_f
 * angle_f(v) n_f and edge pseudonormals sum_f n_f over the incident faces (Baerentzen & Aanaes 2005), as 64-bit
 * fixed-point integer sums (2^-40), so the same inputs give the same bits on every run; the number of incident faces
 * of every edge (vertex index pairs: 1 = boundary, > 2 = non-manifold; a vertex inherits the flags of its edges); two
 * uniform grids of triangle ids, a triangle listed in every cell its bounding box overlaps.  Everything lives in the
 * caller's workspace (bytes: a function of the two counts alone; n_faces <= 2^27); the workspace IS the index and is
 * passed to bnv_mesh_sdf_query as built.  No allocation, synchronisation or host read.
 *
 * Query.  query fp32 [n_query, 3] -> sdf_out fp32 [n_query]; face_out int32 [n_query], closest_out fp32 [n_query, 3],
 * feature_out uint8 [n_query] (each may be NULL: not written).  Per triangle the closest point by the seven-region
 * (vertex / edge / face) case analysis in fp32, one rounding per operation; d2 = (dx dx + dy dy) + dz dz to that
 * point; the triangle of least d2 wins, the LOWEST face index among equals; |sdf| = sqrt(d2) correctly rounded.  The
 * sign is that of (query - closest) . pseudonormal of the closest feature -- the face, the edge or the vertex -- in
 * float64 (>= 0: outside).  feature = 0 face | 1 edge | 2 vertex, | BNV_MESH_SDF_BOUNDARY when that edge or vertex
 * lies on the mesh boundary (the sign there is not trustworthy), | BNV_MESH_SDF_NONMANIFOLD when it is non-manifold.
 * A query with a NaN / Inf coordinate, any query against an index without a valid face, or a workspace that does not
 * hold an index of at most ws_bytes gets sdf = NaN, face = -1, closest = NaN, feature = 0.
 * Null pointers (other than the optional outputs), counts <= 0 or out of range and a workspace smaller than
 * bnv_mesh_sdf_workspace_bytes are BNV_ERR_INVALID_ARGUMENT before any HIP call. */
#define BNV_MESH_SDF_BOUNDARY 0x10
#define BNV_MESH_SDF_NONMANIFOLD 0x20
int bnv_mesh_sdf_workspace_bytes(int64_t n_vertices, int64_t n_faces, int64_t* bytes);
int bnv_mesh_sdf_build(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces,
                       void* workspace, int64_t ws_bytes, bnv_stream_t stream);
int bnv_mesh_sdf_query(const void* workspace, int64_t ws_bytes, const float* query, int64_t n_query, float* sdf_out,
                       int32_t* face_out, float* closest_out, uint8_t* feature_out, bnv_stream_t stream);

/* ---- Rays against a triangle mesh and the depth sensor model (bnv_fusion_amd/csrc/meshray.hip;
 * bnv_fusion_amd/scan.py): scan a mesh into the depth sequence everything else here consumes.  The index is the one
 * bnv_mesh_sdf_build makes (bnv_mesh_ray_workspace_bytes == bnv_mesh_sdf_workspace_bytes); it is only read.
 *
 * bnv_mesh_ray_cast.  origins, dirs fp32 [n_rays, 3] (device; dirs need not be unit) -> per ray the nearest hit
 * o + t d with t in [t_min, t_max]: t_out fp32 (NaN: none), face_out int32 (-1: none), uv_out fp32 [n_rays, 2] with
 * hit = (1 - u - v) v0 + u v1 + v v2 (NaN: none), flags_out uint8: BNV_MESH_RAY_HIT, | BNV_MESH_RAY_BACK when the ray
 * meets the face from behind, d . ((v1 - v0) x (v2 - v0)) > 0.  The optional outputs may be NULL.  One thread per ray
 * walks the fine grid cell by cell (3D-DDA, after clipping the ray to the grid's box); the ray / triangle test is the
 * sheared-ray test of Woop, Benthin & Wald (2013) in fp32, one rounding per operation, an exactly zero edge function
 * redone in float64: a ray through an edge or vertex shared by two faces hits one of them.  Two-sided.  The lowest
 * face index wins a tie in t; the same inputs give the same bits.  A ray with a NaN / Inf component or a zero
 * direction, and any ray against an index without a valid face, gets (NaN, -1, NaN, 0).
 *
 * bnv_mesh_render_depth.  The camera form, for n_poses <= BNV_MESH_RENDER_MAX_POSES poses in one launch: K_host fp32
 * [9] row-major, poses_host fp32 [n_poses, 16] row-major camera-to-world (host).  The ray of pixel (u, v) has the
 * front end's arithmetic: x = (u - cx) / fx, y = (v - cy) / fy, origin T[:3, 3], direction R (x, y, 1) =
 * (R[a][0] x + R[a][1] y) + R[a][2] in fp32, so t is the z-depth the data sets store.  depth_out fp32 [n_poses, H, W]:
 * the nearest hit's t in metres, 0 where there is none or it lies outside [near, max_depth) or is not positive;
 * face_out int32 [n_poses, H, W] (NULL: not written; -1 where depth is 0); normals_out fp32 [n_poses, H, W, 3] (NULL:
 * not written): the unit geometric normal in world coordinates turned towards the camera (0 where depth is 0); seen
 * uint32 [n_seen] (NULL: none): += 1 at the face of every pixel with depth > 0 (integer atomics: order-free; faces >=
 * n_seen are not counted).
 *
 * bnv_depth_sensor.  The reference's Simulator.simulate (src/utils/geometry.py:42-72) per output pixel (r, c) of a
 * clean depth image fp32 [H, W] in metres -> out_mm uint16 [H, W]: x = clamp(rint(c + sigma_px n0)), y = clamp(rint(r
 * + sigma_px n1)); d = clean[y - y % 2, x - x % 2]; with a table fp32 [80, 80, 5] (NULL: none) d = undistort(x, y, d)
 * at table cell (y 80 / H, x 80 / W); d == 0 -> 0, else bf 8 / k with k = rint((bf / d + sigma_d n2) 8), k == 0 -> 0;
 * out = trunc(metres * 1000).  rint is round-half-even.  n0, n1, n2 are standard normals: Philox4x32-10 with key (seed
 * low word, seed high word) and counter (r W + c, frame, 0, 0) gives words w0 .. w3, uniforms ((w >> 9) + 0.5) 2^-23,
 * n0 = sqrt(-2 ln u0) cos(2 pi u1), n1 = sqrt(-2 ln u0) sin(2 pi u1), n2 = sqrt(-2 ln u2) cos(2 pi u3) in fp32; the
 * arithmetic after the draws is float64.  The reference's constants: bf 35.130, sigma_d 0.027778, sigma_px 0.25.
 *
 * Null pointers (other than the optional ones), counts and sizes <= 0 or out of range, t_min > t_max, near >
 * max_depth, more than BNV_MESH_RENDER_MAX_POSES poses and a workspace smaller than an index are
 * BNV_ERR_INVALID_ARGUMENT before any HIP call. */
#define BNV_MESH_RAY_HIT 1
#define BNV_MESH_RAY_BACK 2
#define BNV_MESH_RENDER_MAX_POSES 8
int bnv_mesh_ray_workspace_bytes(int64_t n_vertices, int64_t n_faces, int64_t* bytes);
int bnv_mesh_ray_cast(const void* workspace, int64_t ws_bytes, const float* origins, const float* dirs, int64_t n_rays,
                      float t_min, float t_max, float* t_out, int32_t* face_out, float* uv_out, uint8_t* flags_out,
                      bnv_stream_t stream);
int bnv_mesh_render_depth(const void* workspace, int64_t ws_bytes, int n_poses, const float* K_host,
                          const float* poses_host, int height, int width, float near, float max_depth,
                          float* depth_out, int32_t* face_out, float* normals_out, uint32_t* seen, int64_t n_seen,
                          bnv_stream_t stream);
int bnv_depth_sensor(const float* clean, int height, int width, const float* table, uint64_t seed, uint32_t frame,
                     double bf, double sigma_d, double sigma_px, uint16_t* out_mm, bnv_stream_t stream);

/* ---- Rendering (bnv_fusion_amd/csrc/render.hip): depth and normal images of the map from a camera pose.  The
 * reference has no such entry; these are the semantics SparseVolume.render_depth / TSDFVolume.render_depth expose and
 * the tests replay in float32 (every operation below is one IEEE fp32 rounding, in the order written, sqrt and division
 * correctly rounded; no contraction).
 *
 * Camera.  T_wc_host: float32 [4][4] row-major camera-to-world (camera looks along +z, y points down); K_host:
 * float32 [3][3] row-major pinhole matrix.  Pixel p = v W + u (u the column) has its centre at integer (u, v):
 *   x = (u - cx) / fx,  y = (v - cy) / fy,  w_a = (R[a][0] x + R[a][1] y) + R[a][2],  nrm = sqrt((w0 w0 + w1 w1) + w2 w2),
 *   d_a = w_a / nrm (unit direction), o = T_wc[:3, 3].  A point at Euclidean distance t has z-depth t / nrm.
 * Sample box.  lo = the grid's origin, hi_a = lo_a + (float)(n_a - 1) * voxel (the neural volume: lo = bound_min,
 * n = n_xyz; the TSDF volume: lo = origin, n = dim) -- the points whose interpolation corners can all lie in the grid.
 * Per axis with d_a != 0: t1 = (lo_a - o_a) / d_a, t2 = (hi_a - o_a) / d_a, tin = max(tin, min(t1, t2)),
 * tout = min(tout, max(t1, t2)) from tin = 0, tout = +inf; an axis with d_a == 0 and o_a outside [lo_a, hi_a] has no
 * sample.  t0 = max(tin, near * nrm), t1 = min(tout, max_depth * nrm).
 * Schedule.  s = step * voxel (voxel: the volume's own; step >= BNV_RENDER_MIN_STEP); sample k >= 0 lies at t_k = t0 + (float)k * s, point
 * p_k = o + t_k d (per axis o_a + t_k d_a), for every k with t_k <= t1.  Acceleration (brick, hash, the walk) only
 * decides which samples are evaluated, never where they lie.
 * Field and domain, neural volume: f(p) = bnv_decode_pts at world point p with the same rows, weights, row_limit,
 * network, mode and delta.  p is in the domain iff the 8 corners decode_pts gathers (floor / ceil per axis of
 * c = (p - bound_min) / voxel) are all rows r of the volume with r < row_limit.  The out-of-domain sample right before a
 * run of in-domain samples is the run's lead-in: decode_pts gives it its masked constant (voxel_size, plus the delta
 * when one is set -- a corner without a row is free space, as the mesh of the same state treats it), without the
 * MLP.  No other out-of-domain sample is decoded.
 * Field and domain, TSDF volume: c = (p - origin) / voxel, i = floor(c), f = c - i; in the domain iff the 8 grid
 * points i + {0,1}^3 lie in the grid and have weight > 0 (unobserved voxels hold -trunc_margin); f(p) = trilinear with
 * lerp(a, b, f) = a + f (b - a), along x (corner pairs differing in x), then y, then z.
 * Hit.  The first k >= 1 with sample k in the domain, sample k - 1 in the domain or k's lead-in (neural volume only;
 * the TSDF volume needs both in the domain) and f(k-1) > 0 >= f(k): a run whose lead-in (or, on the TSDF volume, whose
 * first sample) is at or below 0 is not a hit -- the ray started inside the surface or met a back face.  Without the
 * lead-in, a run of rows that begins inside the surface -- the positive side of a surface often lies in cells with a
 * corner missing -- would hide it.  t_hit = t_{k-1} + (f(k-1) / (f(k-1) - f(k))) s, depth = t_hit / nrm
 * (z-depth in metres; 0 = no hit, like the input depth images).
 * Normals (optional, world frame, unit length, 0 where there is no hit or the gradient is 0), at p_hit = o + t_hit d:
 * neural: g_a = f(p_hit + e e_a) - f(p_hit - e e_a) with e = BNV_RENDER_NORMAL_EPS * voxel (p_hit_a + e, p_hit_a - e);
 * TSDF: the gradient of the trilinear interpolant at p_hit (cell clamped into the grid); then g / sqrt((gx gx + gy gy)
 * + gz gz).  Outputs: depth_out f32 [H, W], normals_out f32 [H, W, 3] or NULL. */
#define BNV_RENDER_NORMAL_EPS 0.5f   /* central-difference offset of neural normals, in voxels */
#define BNV_RENDER_DEFAULT_K 8       /* in-domain samples a ray appends per round (plus a lead-in) */
#define BNV_RENDER_MIN_STEP 0.05f    /* smallest sample spacing, in voxels: smaller steps are BNV_ERR_INVALID_ARGUMENT */

/* Workspace bytes of bnv_render_depth for n_rays = H * W rays appending up to k (1..32) samples per round; 0 when the
 * arguments are out of range.  One workspace serves any number of renders of that size. */
size_t bnv_render_workspace_bytes(int64_t n_rays, int32_t k);
/* Renders the sparse neural volume (semantics above).  Rounds until no ray is active: every active ray appends its
 * next <= k in-domain samples to a compacted buffer, bnv_decode_pts evaluates them, a resolve pass records hits and
 * retires rays.  Each round reads two counters back to the host (the stream is synchronised once per round and once
 * for the normals), so this entry is not capturable into a graph.  stats_host (NULL: skipped): int64 [4] = {rounds,
 * samples decoded, of those the live ones (all corner weights >= min_pts_in_grid), hits}.  A sharded grid
 * (shard_world > 1) is BNV_ERR_INVALID_ARGUMENT.  The volume is only read. */
int bnv_render_depth(const bnv_volume_t* vol_host, const bnv_grid_t* grid_host, const float* features,
                     const float* weights, int64_t row_limit, const float* sdfmlp_pack,
                     const bnv_sdf_delta_t* delta_host, const float T_wc_host[16], const float K_host[9], int32_t H,
                     int32_t W, float near_z, float max_depth, float step, int32_t k, void* ws, size_t ws_bytes,
                     float* depth_out, float* normals_out, int64_t* stats_host, bnv_stream_t stream);
/* Renders the TSDF side volume (tsdf, weight: the [X, Y, Z] f32 volumes of bnv_tsdf_integrate, dim = {X, Y, Z},
 * origin / voxel_size their grid) with the same camera, schedule and hit rule; one launch, no host read. */
int bnv_tsdf_render_depth(const float* tsdf, const float* weight, const int32_t dim[3], const float origin_host[3],
                          float voxel_size, const float T_wc_host[16], const float K_host[9], int32_t H, int32_t W,
                          float near_z, float max_depth, float step, float* depth_out, float* normals_out,
                          bnv_stream_t stream);

/* ---- Mesh post-processing (bnv_fusion_amd/csrc/meshpost.hip): mesh.post_process_mesh on the device, the reference's
 * o3d_helper.post_process_mesh (src/utils/o3d_helper.py:220-241) as the host function restates it, with the same
 * output bit for bit.  All arithmetic is float64, one rounding per operation in the order written, no contraction.
 *
 * Input: vertices f32 [V, 3], faces i64 [T, 3], eps = vertex_threshold (finite, >= 0).
 * 1. Exact weld.  u = rint(x * 1e9) / 1e9 per coordinate (np.round(x, 9)); -0 is +0.  The distinct rows u, in
 *    lexicographic (x, y, z) order, are the unique points 0..n-1.  Float32 values closer than 1e-9 near 0 are one point.
 * 2. Clusters.  Unique points i and j are joined when (dx*dx + dy*dy) + dz*dz <= eps*eps (ties join); clusters are the
 *    connected components, numbered in ascending order of their smallest member (scipy's labelling).
 * 3. Cluster position: the members' u summed one after another in ascending index order, divided by the count.
 * 4. Faces: every corner -> unique point -> cluster.  Faces with two equal corners are dropped.  A face rotated so its
 *    smallest label comes first (cyclic order kept) is a duplicate of an earlier face with the same rotation: the first
 *    occurrence is kept, face order preserved.  A face with the reversed winding is not a duplicate.
 * 5. Only clusters the surviving faces reference are kept, in label order; the faces are renumbered.
 * 6. One pass of simple Laplacian smoothing: neighbours = the distinct vertices sharing a triangle edge;
 *    out = (v + sum of neighbours in ascending index order) / (1 + degree), rounded to float32.
 * A mesh without faces comes back unchanged (V' = V, T' = 0); every face degenerate gives V' = T' = 0.
 *
 * Workspace: bnv_mesh_post_workspace_bytes (~180 B per vertex + ~150 B per face; V, T < 2^31 - 1, else
 * BNV_ERR_INVALID_ARGUMENT).  bnv_mesh_post_process writes vertices_out f32 [V, 3] and faces_out i64 [T, 3] (capacities
 * of the input's size: V' <= V, T' <= T) and the device int64[2] counts = {V', T'}; the rows past the counts are
 * unspecified.  Input the device finds invalid -- a non-finite vertex, a face index outside [0, V), or (eps > 0) a
 * coordinate with |u| / eps >= 2^30, beyond which the neighbour grid's cells are not exact -- gives counts = {-1, -1}.
 * No allocation, synchronisation or host read: the caller reads the two counts. */
int bnv_mesh_post_workspace_bytes(int64_t n_vertices, int64_t n_faces, int64_t* bytes);
int bnv_mesh_post_process(const float* vertices, int64_t n_vertices, const int64_t* faces, int64_t n_faces,
                          double vertex_threshold, void* workspace, int64_t ws_bytes, float* vertices_out,
                          int64_t* faces_out, int64_t* counts, bnv_stream_t stream);

/* ---- Mesh components (bnv_fusion_amd/csrc/meshcomp.hip): connected components of a mesh's faces, their face counts and
 * areas, and the filter that removes the small ones -- mesh.connected_components / mesh.remove_small_components on the
 * device with the same output bit for bit.  This is the block the reference's o3d_helper.post_process_mesh documents
 * ("merge close vertices and remove small connected components") and keeps commented out (src/utils/o3d_helper.py:
 * 232-236: cluster_connected_triangles, drop components below surface_threshold, remove unreferenced vertices).
 * PARITY UNPINNED: Open3D's clustering rule is restated from memory.
 *
 * Input: vertices f32 [V, 3], faces i64 [T, 3], V, T < 2^31 - 1.
 * 1. Adjacency.  Face t has the undirected edges {f0, f1}, {f1, f2}, {f2, f0}; an edge whose two ends are the same
 *    index joins nothing.  Two faces are adjacent when they have an edge with the same two vertex INDICES (positions do
 *    not count: an unwelded soup has T components).  Winding does not matter, three or more faces on one edge are all
 *    adjacent, faces that share only a vertex are not.
 * 2. Components: the connected components of that adjacency, numbered 0..C-1 in ascending order of their smallest face
 *    index (scipy's labelling).  labels i32 [T].
 * 3. Areas, order-free and exact.  Per face in float64 from the float32 coordinates, one rounding per operation in the
 *    order written, no contraction: e1 = b - a, e2 = c - a; cx = e1y*e2z - e1z*e2y, cy = e1z*e2x - e1x*e2z,
 *    cz = e1x*e2y - e1y*e2x; area = 0.5 * sqrt((cx*cx + cy*cy) + cz*cz) with a correctly rounded sqrt;
 *    q = rint(area * 2^50) as int64, ties to even.  A component's area is (sum of q) / 2^50 with the sum taken in
 *    integers (any summation order gives the same bits) and converted to float64 once, to nearest even; its face count
 *    comes with it.  The input is refused when a vertex is non-finite, a face index is outside [0, V), or the mesh's
 *    total area reaches 2^12 square units (sum of q >= 2^62): the sums then cannot overflow.
 * 4. Filter (min_area finite >= 0, min_faces >= 0, keep_largest >= 0).  A component is kept iff area >= min_area
 *    (equality keeps; the reference removes component_surfaces < surface_threshold), n_faces >= min_faces, and
 *    keep_largest == 0 or the component is among the keep_largest largest by area over ALL components, ties going to
 *    the smaller label.  Kept faces keep their order; vertices referenced by a kept face keep their order and their
 *    bits, all others are dropped; faces are renumbered.  Nothing kept, or T = 0, gives V' = T' = 0.
 *
 * Workspace: bnv_mesh_components_workspace_bytes (148 B per face + 8 B per vertex; one workspace serves both entries;
 * V, T out of range: BNV_ERR_INVALID_ARGUMENT).  bnv_mesh_components writes labels i32 [T], n_faces_out i64 [T] and
 * areas_out f64 [T] (capacities of T: C <= T; entries past C are unspecified) and the device int64 count = C, or -1 for
 * input the device finds invalid.  bnv_mesh_filter_components writes vertices_out f32 [V, 3] and faces_out i64 [T, 3]
 * (capacities of the input's size) and the device int64[2] counts = {V', T'}, {-1, -1} for invalid input; rows past
 * the counts are unspecified.  No allocation, synchronisation or host read: the caller reads the counts. */
int bnv_mesh_components_workspace_bytes(int64_t n_vertices, int64_t n_faces, int64_t* bytes);
int bnv_mesh_components(const float* vertices, int64_t n_vertices, const int64_t* faces, int64_t n_faces,
                        void* workspace, int64_t ws_bytes, int32_t* labels, int64_t* n_faces_out, double* areas_out,
                        int64_t* count, bnv_stream_t stream);
int bnv_mesh_filter_components(const float* vertices, int64_t n_vertices, const int64_t* faces, int64_t n_faces,
                               double min_area, int64_t min_faces, int64_t keep_largest, void* workspace,
                               int64_t ws_bytes, float* vertices_out, int64_t* faces_out, int64_t* counts,
                               bnv_stream_t stream);

/* ---- Mesh simplification (bnv_fusion_amd/csrc/meshsimplify.hip): vertex clustering on a uniform grid with quadric
 * placement -- mesh.simplify_mesh on the device with the same output bit for bit.  All arithmetic is float64, one
 * rounding per operation in the order written, no contraction; sqrt and division are correctly rounded.
 * tests/mesh_simplify_restatement.py states every step as code.
 *
 * Input: vertices f32 [V, 3], faces i64 [T, 3], cell h > 0, placement, min_det >= 0.
 * 1. Cells.  i_a = floor(double(x_a) / h) per axis; key = (ix + 2^20) << 42 | (iy + 2^20) << 21 | (iz + 2^20).  Clusters
 *    are the distinct keys, numbered in ascending key order.  Cell centre c_a = (i_a + 0.5) * h.
 * 2. Mean: the float64 coordinates of ALL the cluster's vertices (referenced by a face or not), summed one after another
 *    in ascending vertex index, divided by their number.
 * 3. Quadric (BNV_SIMPLIFY_QUADRIC).  Corner 3 t + k belongs to the cluster of vertex faces[t][k]; a cluster's corners
 *    are taken in ascending corner id (a face with two corners in a cluster counts twice).  Per corner, with the face's
 *    vertices minus the cluster's cell centre as p0, p1, p2: e1 = p1 - p0, e2 = p2 - p0, n = (e1y*e2z - e1z*e2y,
 *    e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x), L = sqrt((n0*n0 + n1*n1) + n2*n2).  L == 0 or a repeated index: nothing.
 *    Else u = n / L, w = 0.5 * L, d = -((u0*p0x + u1*p0y) + u2*p0z); A_ij += (w*u_i)*u_j for ij = 00 01 02 11 12 22 and
 *    b_i += (w*d)*u_i.  Then c00 = A11*A22 - A12*A12, c01 = A02*A12 - A01*A22, c02 = A01*A12 - A02*A11,
 *    c11 = A00*A22 - A02*A02, c12 = A01*A02 - A00*A12, c22 = A00*A11 - A01*A01, det = (A00*c00 + A01*c01) + A02*c02,
 *    tr = (A00 + A11) + A22, r = -b, x_i = ((c_i0*r0 + c_i1*r1) + c_i2*r2) / det (c symmetric).  The position c + x is
 *    taken iff tr > 0, |det| >= min_det * (((tr/3)*(tr/3))*(tr/3)) and every |x_a| <= h; otherwise, and always with
 *    BNV_SIMPLIFY_MEAN, the mean.  The result is rounded to float32 once.
 * 4. Faces: the face step of the post-processing (corners -> clusters, faces with two equal clusters dropped, of faces
 *    with the same cyclic triple the first kept, input order kept); only referenced clusters come out, in key order.
 *
 * Workspace: bnv_mesh_simplify_bytes (~52 B per vertex + ~80 B per face; V < 2^31 - 1, T <= 2^30 so that corner ids fit
 * 32 bits, else BNV_ERR_INVALID_ARGUMENT).  bnv_mesh_simplify writes vertices_out f32 [V, 3] and faces_out i64 [T, 3]
 * (capacities of the input's size) and the device int64[2] counts = {V', T'}; rows past the counts are unspecified.
 * Nothing is clamped: a non-finite vertex, a face index outside [0, V) or a coordinate with |x| / h >= 2^20 gives
 * counts = {-1, -1}; a non-finite or non-positive cell, a non-finite or negative min_det or an unknown placement is
 * BNV_ERR_INVALID_ARGUMENT.  No faces (or no vertices) gives an empty mesh.  No allocation, synchronisation or host
 * read: the caller reads the two counts. */
#define BNV_SIMPLIFY_QUADRIC 0
#define BNV_SIMPLIFY_MEAN 1
int bnv_mesh_simplify_bytes(int64_t n_vertices, int64_t n_faces, int64_t* bytes);
int bnv_mesh_simplify(const float* vertices, int64_t n_vertices, const int64_t* faces, int64_t n_faces, double cell,
                      int32_t placement, double min_det, void* workspace, int64_t ws_bytes, float* vertices_out,
                      int64_t* faces_out, int64_t* counts, bnv_stream_t stream);

/* ---- Training of the local shape embedding (bnv_fusion_amd/csrc/train.hip): the reference's
 * LitFusionPointNet.training_step with training_global=False (local_point_fusion.py:381-460), in exact fp32.
 *
 * params: f32 [bnv_train_param_floats()], every trainable tensor of the state_dict, flattened in state_dict order:
 * conv1..4 (weight, bias), bn1..4 (weight, bias), geo_layer0..3 (weight, bias), fc_alpha (weight, bias).  running:
 * f32 [bnv_train_running_floats()], per BatchNorm layer its running_mean then its running_var.  grads, adam_m, adam_v:
 * f32 like params.  input_pts f32 [B, 64, 6] (xyz, normal; rows 0..n-1 of each patch are read), training_pts f32
 * [B, M, 3] and gt f32 [B, M], in voxel units.  Shapes: B >= 1, 1 <= n <= 64, B n >= 2, M >= 1, B M <= 2^24;
 * anything else is BNV_ERR_INVALID_ARGUMENT.
 *
 * bnv_train_step: encoder forward with train-mode BatchNorm (batch statistics over the B n rows, biased variance,
 * eps 1e-5; running stats updated with momentum 0.1 and the unbiased variance), per-patch mean -> feats [B, 8];
 * decoder over the B M rows [xyz, sin xyz, cos xyz, feat]; loss_out f32 [3] = {l1 + 0.001 reg, l1, reg} with
 * l1 = mean |pred - gt|, reg = mean_b |feats_b|; the gradient of every parameter into grads (overwritten; the conv
 * biases' is written as its exact value 0, train-mode BatchNorm removing them); then one
 * Adam step (torch's formula, step number adam_step >= 1) on params.  num_batches_tracked is the caller's.
 * bnv_train_eval_loss: the same forward with eval-mode BatchNorm (running stats), nothing written but
 * loss_out = {l1, l1, reg}.  Every sum over rows is reduced in a fixed order with no float atomics: results are
 * bit-reproducible for a given shape.  Both are a fixed sequence of launches on stream: no allocation,
 * synchronisation or host read.  Workspace: bnv_train_workspace_bytes(B, n, M) (0 for an invalid shape); one
 * workspace serves both entries for that shape. */
int64_t bnv_train_param_floats(void);
int64_t bnv_train_running_floats(void);
size_t bnv_train_workspace_bytes(int64_t B, int32_t n, int64_t M);
int bnv_train_step(float* params, float* grads, float* adam_m, float* adam_v, float* running, const float* input_pts,
                   const float* training_pts, const float* gt, int64_t B, int32_t n, int64_t M, float lr, float beta1,
                   float beta2, float eps, int64_t adam_step, float* loss_out, void* workspace, size_t ws_bytes,
                   bnv_stream_t stream);
int bnv_train_eval_loss(const float* params, const float* running, const float* input_pts, const float* training_pts,
                        const float* gt, int64_t B, int32_t n, int64_t M, float* loss_out, void* workspace,
                        size_t ws_bytes, bnv_stream_t stream);

/* ---- Training of the tiny-cuda-nn embedding (bnv_fusion_amd/csrc/train_tcnn.hip): the reference's default networks
 * (tiny_cuda: True; tcnnPointNetEncoder and tcnnNeRFModel, FullyFusedMLP 64 wide, 3 hidden layers, ReLU, no bias)
 * under LitFusionPointNet.training_step with training_global=False (local_point_fusion.py:381-460).
 *
 * params: f32 [bnv_train_tcnn_param_floats()] = 21,504: pointnet_backbone.model.params [10,240] (widths
 * 16 | 64 | 64 | 64 | 16) then nerf.model.params [11,264] (32 | 64 | 64 | 64 | 16), each the row-major [out, in]
 * matrices in layer order.  grads, adam_m, adam_v: f32 like params.  adam_step: int64 [1] on the device, the number
 * of Adam steps taken so far (0 at the start).  input_pts f32 [B, 64, 6] (rows 0..n-1 of each patch are read),
 * training_pts f32 [B, M, 3], gt f32 [B, M].  Shapes: B >= 1, 1 <= n <= 64, M >= 1, B M <= 2^24; anything else is
 * BNV_ERR_INVALID_ARGUMENT.
 *
 * Forward, the mode-2 arithmetic of the inference kernels: the input padded with 1.0 to 16 (encoder) / 32 (decoder)
 * columns and rounded to f16, weights rounded to f16, each layer an f16 product accumulated in fp32, ReLU after the
 * hidden layers, each layer output rounded to f16.  Encoder over the B n points, outputs 0..7; feats_b = f16(mean over
 * the patch's n points).  Decoder over the B M queries on [p, sin p, cos p, feats_b] (the decode path's encoding);
 * pred = output 0.  Loss: l1 = mean |pred - gt|, reg = mean_b |feats_b|_2, loss = l1 + 0.001 reg.
 * Backward: every f16 rounding is the identity (straight-through), sign(0) = 0, ReLU'(0) = 0; the gradient of every
 * weight (pad columns included; output rows nothing reads -- encoder 8..15, decoder 1..15 -- exactly 0).  Precision:
 * activations and weights are exact f16; each layer's incoming gradient is split into hi + lo f16 parts, two f16
 * products accumulated in fp32, near fp32.  End to end, with the f16 forward's rounding decisions (a value one ulp
 * off flips sign(pred - gt) or a ReLU), every gradient is within 5e-3 of its tensor's largest |gradient| of the
 * float64 restatement.
 *
 * bnv_train_tcnn_step: forward, loss, grads (overwritten), then, unless the loss or a gradient is not finite, one
 * Adam step (torch's formula; lr, betas, eps) on params with step number *adam_step + 1, which it stores.  loss_out
 * f32 [4] = {loss, l1, reg, skipped}: skipped = 1 when the step was skipped (params, adam_m, adam_v and *adam_step
 * untouched), else 0.
 * bnv_train_tcnn_eval_loss: forward and loss only; loss_out f32 [3] = {loss, l1, reg}.
 * bnv_train_tcnn_forward: forward only; feats f32 [B, 8], pred f32 [B, M] (f16 values).
 * Every sum over rows (weight gradients, patch means, d feats over M, the loss) is reduced in a fixed order with no
 * float atomics: results are bit-reproducible for a given shape.  Each entry is a fixed sequence of launches on
 * stream: no allocation, synchronisation or host read.  Workspace: bnv_train_tcnn_workspace_bytes(B, n, M) (0 for an
 * invalid shape); a workspace sized for n = 64 serves every n and all three entries. */
int64_t bnv_train_tcnn_param_floats(void);
size_t bnv_train_tcnn_workspace_bytes(int64_t B, int32_t n, int64_t M);
int bnv_train_tcnn_step(float* params, float* grads, float* adam_m, float* adam_v, int64_t* adam_step,
                        const float* input_pts, const float* training_pts, const float* gt, int64_t B, int32_t n,
                        int64_t M, float lr, float beta1, float beta2, float eps, float* loss_out, void* workspace,
                        size_t ws_bytes, bnv_stream_t stream);
int bnv_train_tcnn_eval_loss(const float* params, const float* input_pts, const float* training_pts, const float* gt,
                             int64_t B, int32_t n, int64_t M, float* loss_out, void* workspace, size_t ws_bytes,
                             bnv_stream_t stream);
int bnv_train_tcnn_forward(const float* params, const float* input_pts, const float* training_pts, int64_t B,
                           int32_t n, int64_t M, float* feats, float* pred, void* workspace, size_t ws_bytes,
                           bnv_stream_t stream);

/* ---- Tracking (bnv_fusion_amd/csrc/track.hip; bnv_fusion_amd/tracking.py): frame-to-model ICP.  Aligns a depth frame
 * to a view of the map -- the depth and world normals bnv_render_depth, bnv_tsdf_render_depth or
 * bnv_mesh_render_depth wrote -- by projective point-to-plane ICP and returns the corrected camera-to-world pose.  The
 * reference takes every pose as given and has no such entry; tests/track_restatement.py restates what follows in
 * numpy.  Every operation is one IEEE float64 rounding, in the order written (no contraction); division and sqrt are
 * correctly rounded.
 *
 * Inputs.  depth [H, W] (device): depth_dtype 0 = uint16 millimetres, d = (double)mm / 1000.0; 1 = float32 metres,
 * d = (double)m (the front end's conversions).  K_host float64 [9] row-major: fx = K[0], cx = K[2], fy = K[4],
 * cy = K[5].  The model view: model_depth f32 [H_m, W_m] z-depth in metres, 0 = nothing; model_normals f32
 * [H_m, W_m, 3] world frame, pointing to the free-space side, 0 = none; K_m_host its intrinsics; T_m_host float64 [16]
 * row-major its camera-to-world pose and T_m_inv_host the inverse [R^T, -R^T t], both from the caller.  T_guess_host:
 * the frame's camera-to-world pose to start from.  All matrices are host arrays; the images are only read.
 *
 * Schedule.  levels_host int32 [n_levels][2] = (stride, iterations), 1 <= n_levels <= BNV_ICP_MAX_LEVELS, stride >= 1,
 * iterations >= 0, at least one and at most 4096 iterations in all; tracking.DEFAULT_LEVELS is ((4, 4), (2, 5),
 * (1, 10)).  At stride s the sampled pixels are (u, v) = (s i, s j), i < ceil(W / s), j < ceil(H / s), numbered
 * j ceil(W / s) + i; association always goes into the full model view.  No filtered pyramid, no early termination:
 * n_iter = the sum of the iterations is fixed.
 *
 * A pair.  At the current estimate T = [R | t], sampled pixel (u, v) with depth d:
 *   valid iff 0 < d <= max_depth;  x = (u - cx) / fx,  y = (v - cy) / fy,  p_c = (x d, y d, d);
 *   p_w_a = ((R[a][0] p_c0 + R[a][1] p_c1) + R[a][2] p_c2) + t_a;   p_m = T_m_inv p_w in the same form;
 *   reject unless p_m2 > 0;   u' = rint(fx_m p_m0 / p_m2 + cx_m),  v' = rint(fy_m p_m1 / p_m2 + cy_m)  (half to even);
 *   reject unless 0 <= u' <= W_m - 1 and 0 <= v' <= H_m - 1;   d_m = model_depth(v', u'): reject unless d_m > 0 and
 *   finite;   n = model_normals(v', u'): reject when all three components are 0;
 *   q = T_m ((u' - cx_m) / fx_m d_m, (v' - cy_m) / fy_m d_m, d_m) in the form of p_w;   e = q - p_w;
 *   gates: (e0 e0 + e1 e1) + e2 e2 <= dist dist, and (n0 (t0 - q0) + n1 (t1 - q1)) + n2 (t2 - q2) > 0: the model's
 *   surface faces the frame's camera.  No robust weights: the gates are the outlier rule.
 *   r = (n0 e0 + n1 e1) + n2 e2 (a pair whose r is not finite is rejected),  J = [p_w x n, n] with
 *   (p_w x n)_0 = p_w1 n2 - p_w2 n1 and cyclic.  The twist xi = (w, v) multiplies on the left: T <- exp(xi^) T.
 * Sums.  BNV_ICP_SUMS = 29 float64 sums over the pairs: J_a J_b for a <= b row by row (21), J_a r (6), r r, 1.
 * A grid of BNV_ICP_BLOCKS blocks of 256 threads whatever the image; thread g takes the sampled pixels g, g + G, ...
 * (G = 256 BNV_ICP_BLOCKS) in that order; lanes are added by s += shfl_down(s, o) for o = 32, 16, ..., 1, the block's
 * four waves in wave order, the blocks in ascending order.  No float atomics: the same inputs give the same bits.
 *
 * Solve (a one-block launch per iteration).  pairs = the last sum, rmse = sqrt(sum r r / pairs) (0 without pairs).
 *   BNV_ICP_LOST        pairs == 0 or pairs < min_pair_share (sampled pixels of the level);
 *   BNV_ICP_DEGENERATE  spread < min_spread, spread = the smallest eigenvalue of A[3:, 3:] / pairs = (1 / pairs) sum
 *                       n n^T (six sweeps of cyclic Jacobi over (0,1), (0,2), (1,2)): the normals span too few
 *                       directions to hold the translation; or a pivot of the factorisation <= 0;
 *   BNV_ICP_JUMP        |w| > BNV_ICP_MAX_ROTATION or |v| > BNV_ICP_MAX_TRANSLATION;
 * tested in this order.  A xi = b by LDL^T without pivoting, column by column: D_j = A_jj - sum_k<j (L_jk L_jk) D_k,
 * L_ij = (A_ij - sum_k<j (L_ik L_jk) D_k) / D_j (k ascending), then L z = b, z_i / D_i, L^T xi = z.  exp(xi^) by
 * Rodrigues: th = |w|, K = [w]x, R = (I + a K) + b K K, V = (I + b K) + c K K, a = sin th / th, b = (1 - cos th) / th^2,
 * c = (th - sin th) / (th^2 th); below th < 1e-8 a = 1 - th^2 / 6, b = 0.5 - th^2 / 24, c = 1 / 6 - th^2 / 120.
 * T <- [R R_T | (R t_T) + V v], in device memory.
 * A status other than BNV_ICP_OK is sticky: the launch that finds it writes the status and sets pose_out back to
 * T_guess, bit for bit, and every later launch of the call returns right after reading the status.  Nothing is read
 * by the host between the first and the last launch, nothing is allocated or synchronised: the call can be captured
 * into a graph.
 *
 * Outputs (device).  pose_out f64 [16]; poses_out f64 [n_iter + 1, 16] or NULL: the estimate before every iteration
 * and the final one (rows the call did not reach hold T_guess); stats_out f64 [n_iter, 5] = pairs, rmse, |w|, |v|,
 * spread per iteration (0 for what was not computed; rows after a stop are 0); status_out int32 [1].
 * Workspace: bnv_icp_workspace_bytes(n_levels, levels_host) bytes (0 for an invalid schedule): the blocks' partial
 * rows f64 [BNV_ICP_BLOCKS, 29], then one record f64 [BNV_ICP_RECORD_DOUBLES] per iteration = the 29 sums, xi[6] and
 * a pad, for tests and diagnosis.
 * Null pointers (poses_out excepted), sizes <= 0 or > 32768, an invalid schedule, depth_dtype other than 0 / 1,
 * non-finite matrices, a zero focal length, max_depth or dist not positive and finite and negative or non-finite
 * thresholds are BNV_ERR_INVALID_ARGUMENT before any HIP call; a workspace below bnv_icp_workspace_bytes is
 * BNV_ERR_WORKSPACE_TOO_SMALL. */
#define BNV_ICP_OK 0
#define BNV_ICP_LOST 1
#define BNV_ICP_DEGENERATE 2
#define BNV_ICP_JUMP 3
#define BNV_ICP_MAX_LEVELS 8
#define BNV_ICP_BLOCKS 256
#define BNV_ICP_SUMS 29
#define BNV_ICP_RECORD_DOUBLES 36
#define BNV_ICP_MAX_ROTATION 0.1      /* radians per iteration */
#define BNV_ICP_MAX_TRANSLATION 0.2   /* metres per iteration */
size_t bnv_icp_workspace_bytes(int32_t n_levels, const int32_t* levels_host);
int bnv_icp_align(const void* depth, int depth_dtype, int32_t H, int32_t W, const double K_host[9], double max_depth,
                  const float* model_depth, const float* model_normals, int32_t H_m, int32_t W_m,
                  const double K_m_host[9], const double T_m_host[16], const double T_m_inv_host[16],
                  const double T_guess_host[16], int32_t n_levels, const int32_t* levels_host, double dist,
                  double min_pair_share, double min_spread, void* workspace, size_t ws_bytes, double* pose_out,
                  double* poses_out, double* stats_out, int32_t* status_out, bnv_stream_t stream);

/* ---- Odometry (bnv_fusion_amd/csrc/odometry.hip; bnv_fusion_amd/odometry.py): frame-to-frame RGB-D odometry.  Aligns
 * two consecutive frames (depth, and colour where there is one) by a joint photometric and depth alignment and returns
 * the motion between them: T maps reference-camera points to current-camera points.  The reference takes every pose as
 * given and has no such entry; tests/odometry_restatement.py restates what follows in numpy.  Every operation is one
 * IEEE float64 rounding, in the order written (no contraction); division and sqrt are correctly rounded; what is stored
 * in a prepared frame is rounded to float32 once.
 *
 * A prepared frame (bnv_rgbd_prepare; bnv_rgbd_frame_bytes(H, W, levels) bytes of device memory the caller owns, 0 for
 * invalid sizes) holds `levels` pyramid levels, level l of H >> l by W >> l pixels (1 <= levels <= BNV_ICP_MAX_LEVELS
 * and the last level at least 1 x 1), one after the other, each on a 256-byte boundary.  A level is an array of pixel
 * records float32 [H_l][W_l][8] = D, I, I_x, I_y, D_x, D_y, valid (1 or 0), 0.
 *
 * Intensity.  rgb uint8 [H_c, W_c, 3] (device) with intrinsics K_c_host, or NULL: I = 0 everywhere (align such frames
 * with lambda_depth = 1).  Y(j, i) = ((0.299 R + 0.587 G) + 0.114 B) of a colour pixel.  Depth pixel p along an axis
 * with (f, c) and the colour image's (f_c, c_c), n_c pixels: lo = f_c (((p - 0.5) - c) / f) + c_c, hi the same with
 * p + 0.5, mid with p; first = min(max(ceil(lo), 0), n_c), last = max(min(ceil(hi), n_c), first): the colour pixels
 * first .. last - 1 have their centres in the depth pixel's footprint.  With pixels on both axes I = (sum of Y over the
 * footprint in row-major order / (rows cols)) / 255, else the bilinear sample at (mid_x, mid_y), each clamped to
 * [0, n_c - 1]: i0 = min(floor(x), max(n_c - 2, 0)), a = x - i0, i1 = min(i0 + 1, n_c - 1);
 * top = Y00 + a_x (Y01 - Y00), bot = Y10 + a_x (Y11 - Y10), Y = top + a_y (bot - top); I = Y / 255.
 * Level 0.  d as for bnv_icp_align (depth_dtype 0 / 1); D = (float)d when 0 < d <= max_depth and d is finite, else 0.
 * depth_jump is the depth step between neighbouring pixels of level 0 that counts as an edge.  The pixels of level l
 * are 2^l as wide and the same surface slope steps 2^l as far between them, so level l uses jump_l = 2^l depth_jump
 * (exact): with one jump for all levels an oblique wall has no gradient-valid pixel left two levels up.
 * Level l + 1 takes each 2 x 2 block of level l (an odd last row or column is dropped): dmin = the smallest D > 0 of
 * the block; kept = the pixels with D > 0 and D - dmin <= jump_(l+1), so the foreground wins and nothing is averaged
 * across an edge; D and I are the sums over the kept pixels in row-major order / their number, 0 when none is kept.
 * Intrinsics of level l, s = 2^l: fx / s, fy / s, (cx + 0.5) / s - 0.5, (cy + 0.5) / s - 0.5.
 * Gradients.  A pixel is gradient-valid iff it is not on the level's border, D > 0 for it and its left, right, upper
 * and lower neighbour, and |D_neighbour - D| <= jump_l for each; then I_x = (I(u + 1) - I(u - 1)) / 2, I_y, D_x,
 * D_y alike; else all four are 0.
 *
 * A pair.  At the estimate T = [R | t], reference pixel (u, v) with z = D_ref > 0:
 *   x = (u - cx) / fx, y = (v - cy) / fy, P = (x z, y z, z);  Q_a = ((R[a][0] P0 + R[a][1] P1) + R[a][2] P2) + t_a;
 *   reject unless Q2 > 0;  xq = fx Q0 / Q2 + cx, yq = fy Q1 / Q2 + cy;  x0 = floor(xq), y0 = floor(yq); reject unless
 *   0 <= x0 <= W_l - 2 and 0 <= y0 <= H_l - 2;  the four pixels (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1)
 *   of the current frame must all be gradient-valid and max D - min D of the four <= jump_l;
 *   a = xq - x0, b = yq - y0; every plane c is sampled as top = c00 + a (c10 - c00), bot = c01 + a (c11 - c01),
 *   top + b (bot - top) -> I1, D1, Ix, Iy, Dx, Dy;  rd = Q2 - D1: reject unless |rd| <= dist.
 * Rows.  With s_I = sqrt(1 - lambda_depth), s_D = sqrt(lambda_depth), a row of image gradient (a, b), z-term c and
 * scale s: a' = s a, b' = s b, c' = s c; gx = (a' fx) / Q2, gy = (b' fy) / Q2,
 * gz = (0 - (gx Q0 + gy Q1) / Q2) - c'; J = [Q x g, g] with (Q x g)_0 = Q1 gz - Q2 gy and cyclic.  The pair adds the
 * intensity row (Ix, Iy, 0, s_I) with r = s_I (I_ref - I1), then the depth row (Dx, Dy, 1, s_D) with r = s_D rd.
 * J = -dr/dxi for the left twist xi = (w, v), Q' = Q + w x Q + v: A xi = sum J r is the system of bnv_icp_align, and
 * T <- exp(xi^) T.
 * Sums, solve, statuses, outputs and workspace are those of bnv_icp_align (BNV_ICP_*): the 29 sums take both rows of
 * every pair and count a pair once; thread g of the BNV_ICP_BLOCKS x 256 grid takes the level's reference pixels
 * g, g + G, ... (numbered v W_l + u); BNV_ICP_LOST compares pairs with min_pair_share H_l W_l; spread is the smallest
 * eigenvalue of A[3:, 3:] / pairs (a constant-colour fronto-parallel plane gives exactly 0).
 * Schedule.  schedule_host int32 [n_steps][2] = (pyramid level, iterations), 1 <= n_steps <= BNV_ICP_MAX_LEVELS,
 * 0 <= level < levels, iterations >= 0, at least one and at most 4096 iterations in all; odometry.DEFAULT_SCHEDULE is
 * ((2, 6), (1, 6), (0, 8)).  Workspace: bnv_rgbd_align_bytes(n_steps, schedule_host) bytes, laid out as
 * bnv_icp_align's.  Both frames must have been prepared with the same H, W, levels and intrinsics K_host.
 * Null pointers (rgb, poses_out excepted), invalid sizes or schedule, non-finite matrices, a zero focal length,
 * lambda_depth outside [0, 1], max_depth, dist or depth_jump not positive and finite and negative or non-finite
 * thresholds are BNV_ERR_INVALID_ARGUMENT before any HIP call; a buffer below its size entry is
 * BNV_ERR_WORKSPACE_TOO_SMALL.  No allocation, synchronisation or host read. */
size_t bnv_rgbd_frame_bytes(int32_t H, int32_t W, int32_t levels);
size_t bnv_rgbd_align_bytes(int32_t n_steps, const int32_t* schedule_host);
int bnv_rgbd_prepare(const void* depth, int depth_dtype, int32_t H, int32_t W, const double K_host[9],
                     const uint8_t* rgb, int32_t H_c, int32_t W_c, const double K_c_host[9], int32_t levels,
                     double max_depth, double depth_jump, void* frame, size_t frame_bytes, bnv_stream_t stream);
int bnv_rgbd_align(const void* ref_frame, const void* cur_frame, int32_t H, int32_t W, int32_t levels,
                   const double K_host[9], const double T_guess_host[16], int32_t n_steps,
                   const int32_t* schedule_host, double lambda_depth, double dist, double depth_jump,
                   double min_pair_share, double min_spread, void* workspace, size_t ws_bytes, double* pose_out,
                   double* poses_out, double* stats_out, int32_t* status_out, bnv_stream_t stream);

/* ---- Registration (bnv_fusion_amd/csrc/register.hip; bnv_fusion_amd/register.py): point-to-mesh ICP.  Aligns a point
 * cloud (a reconstruction's surface samples, in its own frame) to a triangle mesh (the ground truth) from a guess and
 * returns the rigid transform T that maps source points into the mesh's frame, so that a reconstruction can be scored
 * in the ground truth's frame.  No camera and no rendered view: every point is paired with the exact closest point of
 * the mesh, by the search of bnv_mesh_sdf_query over the index bnv_mesh_sdf_build made.  The reference has no such
 * entry; tests/register_restatement.py restates what follows in numpy.  Every operation is one IEEE float64 rounding,
 * in the order written (no contraction); division and sqrt are correctly rounded; the closest point is the fp32 one of
 * bnv_mesh_sdf_query, bit for bit.
 *
 * Inputs.  mesh_index / index_bytes: the workspace bnv_mesh_sdf_build filled, only read.  points f32 [n_points, 3]
 * (device), source frame, 1 <= n_points <= INT32_MAX.  T_guess_host float64 [16] row-major, source -> mesh.
 *
 * Schedule.  levels_host int32 [n_levels][2] = (stride, iterations) as for bnv_icp_align; dist_host float64
 * [n_levels]: the pairing gate of every level in metres; register.DEFAULT_LEVELS is ((4, 10, 0.2), (2, 6, 0.05),
 * (1, 4, 0.02)).  At stride s the sampled points are i = 0, s, 2 s, ...: n_s = ceil(n_points / s) of them, numbered
 * i / s.  n_iter = the sum of the iterations is fixed.
 *
 * A pair.  At the current estimate T = [R | t], sampled point p = points[i]:
 *   qd_a = ((R[a][0] p0 + R[a][1] p1) + R[a][2] p2) + t_a,  q = (float)qd;  a non-finite q is no pair;
 *   c = the closest point of the mesh to q and its feature, exactly what bnv_mesh_sdf_query answers for the query q
 *   (an index whose header does not fit index_bytes, or without a valid triangle, answers nothing: no pair);
 *   u = (double)q - (double)c,  d2 = (u0 u0 + u1 u1) + u2 u2,  d = sqrt(d2);   reject unless d2 <= dist dist;
 *   with reject_boundary, reject when the feature carries 0x10 (the closest edge or vertex lies on the rim of an open
 *   mesh: a source point that hangs over the rim must not pull);
 *   d == 0 counts as a pair and adds nothing else;  otherwise n = u / d, e = -u, r = (n0 e0 + n1 e1) + n2 e2,
 *   J = [q x n, n] on the float64 value of the fp32 q, (q x n)_0 = q1 n2 - q2 n1 and cyclic.  The twist xi = (w, v)
 *   multiplies on the left: T <- exp(xi^) T.  No robust weights: the gate is the outlier rule.
 * Sums.  Those of bnv_icp_align: thread g of the BNV_ICP_BLOCKS x 256 grid takes the sampled points g, g + G, ...
 *
 * Solve.  That of bnv_icp_align, with one difference: registration starts further off than a tracker does, so a step
 * beyond the limits is scaled, not refused: s = min(1, max_rotation / |w|, max_translation / |v|) and, when s < 1,
 * every xi_a <- xi_a s; |w| and |v| of the stats and the xi of the record are those of the applied step.
 * BNV_ICP_JUMP then only answers a step that is not finite.  BNV_ICP_LOST compares pairs with min_pair_share n_s.
 * A sticky status restores T_guess bit for bit.  Two launches per iteration; nothing is read by the host, allocated
 * or synchronised between the first and the last launch.
 *
 * Dumps (device, each optional).  q_out f32 [n_points, 3], closest_out f32 [n_points, 3], face_out int32 [n_points],
 * feature_out uint8 [n_points]: every iteration writes, for sampled point k of its level, row k: q, and the closest
 * point, face and feature (NaN, -1, 0 where the search answered nothing); rows n_s and up are not touched.  After the
 * call they hold the last iteration's values.
 * Outputs pose_out, poses_out (or NULL), stats_out, status_out and the workspace
 * (bnv_mesh_register_bytes: partial rows, then one record per iteration) are those of bnv_icp_align.
 * Null pointers (poses_out and the dumps excepted), n_points out of range, an invalid schedule, a dist that is not
 * positive and finite, a non-finite T_guess, negative or non-finite thresholds, step limits that are not positive and
 * finite and an index_bytes no index fits into are BNV_ERR_INVALID_ARGUMENT before any HIP call; a workspace below its
 * size entry is BNV_ERR_WORKSPACE_TOO_SMALL. */
size_t bnv_mesh_register_bytes(int32_t n_levels, const int32_t* levels_host);
int bnv_mesh_register(const void* mesh_index, int64_t index_bytes, const float* points, int64_t n_points,
                      const double T_guess_host[16], int32_t n_levels, const int32_t* levels_host,
                      const double* dist_host, int32_t reject_boundary, double min_pair_share, double min_spread,
                      double max_rotation, double max_translation, void* workspace, size_t ws_bytes,
                      double* pose_out, double* poses_out, double* stats_out, int32_t* status_out, float* q_out,
                      float* closest_out, int32_t* face_out, uint8_t* feature_out, bnv_stream_t stream);

/* ---- Cloud registration (bnv_fusion_amd/csrc/cloud_register.hip; bnv_fusion_amd/pointcloud.py: CloudIndex,
 * align_scans; bnv_fusion_amd/register.py: register_cloud): point-to-plane ICP of a point cloud against another point
 * cloud that carries normals -- a laser-scan ground truth that exists only as points, the union of the stations
 * already aligned -- and the persistent index of that target.  Returns the rigid T that maps source points into the
 * target's frame.  The reference has no such entry; tests/cloud_register_restatement.py restates what follows in
 * numpy.  Every float64 operation is one IEEE rounding, in the order written (no contraction); division and sqrt are
 * correctly rounded.
 *
 * Index.  input_pts f32 [n_points, 6] (device): positions and normals, the rows bnv_cloud_normals writes and the
 * encoder takes; 1 <= n_points <= 2^31 - 3.  Row j is rejected when a position or normal component is NaN / Inf (the
 * all-NaN rows bnv_cloud_normals makes of what it rejects) or when len = sqrt((nx nx + ny ny) + nz nz), in float64 of
 * the fp32 components, is below 1e-12.  The index holds, under a header (magic, n_points, layout version): the
 * positions copied (a rejected row: three NaNs), the normals (float)(n / len) (a rejected row: three NaNs), and the
 * two-level uniform grid of bnv_nn_query (the same cell target) over the copied positions.  The grid leaves out a
 * non-finite point, so a rejected row is never anyone's nearest neighbour.  Everything lives in the caller's workspace
 * (bnv_cloud_index_bytes: a function of n_points alone); the workspace IS the index and is passed on as built.
 * bnv_cloud_index_build makes no allocation, synchronisation or host read (the header is written by a kernel):
 * capturable into a graph.
 *
 * Nearest.  bnv_cloud_index_nearest: query f32 [n_query, 3], taken in the order given -> d2_out f32 [n_query], idx_out
 * int32 [n_query], exactly what bnv_nn_query answers against the positions the index kept: d2 bitwise the minimum of
 * the fp32 (dx dx + dy dy) + dz dz, idx the LOWEST index attaining it; (+inf, -1) for a non-finite query, an index
 * without a kept row, or memory that does not hold an index of at most index_bytes (a header that does not match).
 *
 * Register.  points f32 [n_points, 3] (device), source frame, 1 <= n_points <= INT32_MAX; source_normals f32
 * [n_points, 3] or NULL; T_guess_host, levels_host, dist_host, the sampled points and n_iter as for bnv_mesh_register.
 * A pair.  At the current estimate T = [R | t], sampled point p = points[i]:
 *   qd_a = ((R[a][0] p0 + R[a][1] p1) + R[a][2] p2) + t_a,  q = (float)qd;  a non-finite q has no candidate;
 *   g2 = (float)(dist dist), the product taken in float64;  the candidate j is the kept target row of least fp32
 *   d2 = (dx dx + dy dy) + dz dz, dx = q.x - c.x, among those with d2 <= g2, the LOWEST index among equals; none: no
 *   candidate.  (The ring walk starts from the bound nextafterf(g2, +inf) with index -1: the same answer as the
 *   unbounded search followed by the gate test, but a point far from the target stops after a ring or two.)  An index
 *   that bnv_cloud_index_nearest would not answer from has no candidate for any point.
 *   With source_normals, s = source_normals[i]: a non-finite s rejects the pair;  m_a = (R[a][0] s0 + R[a][1] s1) +
 *   R[a][2] s2,  cs = (m0 n0 + m1 n1) + m2 n2 with n the target's normal as float64;  keep when cs >= min_normal_cos
 *   (oriented != 0) or |cs| >= min_normal_cos (oriented == 0).  Without source_normals both arguments are ignored.
 *   Row: c = the target's position j, e_a = (double)c_a - (double)q_a,  r = (n0 e0 + n1 e1) + n2 e2,  J = [q x n, n] on
 *   the float64 value of the fp32 q, (q x n)_0 = q1 n2 - q2 n1 and cyclic;  pairs += 1 for every kept pair.  The twist
 *   multiplies on the left: T <- exp(xi^) T.  No robust weights: the gate is the outlier rule.
 * The sign of a target normal does not matter: negating n negates J and r, and every one of the 29 products is then
 * the same to the bit (and |cs| too), so a target needs only unoriented normals -- bnv_cloud_normals with any origin.
 * Sums, Solve, the sticky status, the outputs pose_out, poses_out (or NULL), stats_out, status_out and the workspace
 * (bnv_cloud_register_bytes = bnv_mesh_register_bytes) are those of bnv_mesh_register, the clamp included.  Two
 * launches per iteration; nothing is read by the host, allocated or synchronised.
 * Dumps (device, each optional).  q_out f32 [n_points, 3], index_out int32 [n_points]: every iteration writes, for
 * sampled point k of its level, row k: q and the candidate j (-1: none; the normal gate does not change it); rows n_s
 * and up are not touched.
 * Null pointers (source_normals, poses_out and the dumps excepted), counts out of range, an invalid schedule, a dist
 * that is not positive and finite, a non-finite T_guess, with source_normals a min_normal_cos outside [-1, 1],
 * negative or non-finite thresholds, step limits that are not positive and finite and an index_bytes no index fits
 * into are BNV_ERR_INVALID_ARGUMENT before any HIP call; a workspace below its size entry is
 * BNV_ERR_WORKSPACE_TOO_SMALL. */
int bnv_cloud_index_bytes(int64_t n_points, int64_t* bytes);
int bnv_cloud_index_build(const float* input_pts, int64_t n_points, void* workspace, int64_t ws_bytes,
                          bnv_stream_t stream);
int bnv_cloud_index_nearest(const void* cloud_index, int64_t index_bytes, const float* query, int64_t n_query,
                            float* d2_out, int32_t* idx_out, bnv_stream_t stream);
size_t bnv_cloud_register_bytes(int32_t n_levels, const int32_t* levels_host);
int bnv_cloud_register(const void* cloud_index, int64_t index_bytes, const float* points, int64_t n_points,
                       const float* source_normals, const double T_guess_host[16], int32_t n_levels,
                       const int32_t* levels_host, const double* dist_host, double min_normal_cos, int32_t oriented,
                       double min_pair_share, double min_spread, double max_rotation, double max_translation,
                       void* workspace, size_t ws_bytes, double* pose_out, double* poses_out, double* stats_out,
                       int32_t* status_out, float* q_out, int32_t* index_out, bnv_stream_t stream);

/* ---- Depth filter (bnv_fusion_amd/csrc/depth_filter.hip; bnv_fusion_amd/frontend.py: filter_depth): edge-preserving
 * smoothing of a depth image in front of the front end and the tracker.  Sensor depth is disparity-quantised (one
 * step of the reference's Kinect model is z^2 / (8 * 35.130): 3.6 mm at 1 m, 32 mm at 3 m) and the front end's 3x3
 * Sobel makes poor normals of such a staircase.  A bilateral filter whose spatial and range kernels are Tukey
 * biweights: float64 arithmetic in the order below, no transcendental function, one rounding to float32 at the end.
 *
 * depth [H, W] / depth_dtype / max_depth / conf / conf_level as for bnv_depth_to_points.  z(q) is the depth of
 * pixel q in metres as a double (uint16: (double)u / 1000.0); q is valid when 0 < z(q) < max_depth (NaN and inf are
 * not) and, with a confidence map, conf[q] >= conf_level.  Spatial weight of the offset (dy, dx), r = radius:
 * a = 1.0 - (double)(dy dy + dx dx) / (double)((r + 1) (r + 1)), wa = a a; taps with a <= 0 are skipped.  For a valid
 * centre p: s = sigma_depth z_p z_p, c = range_cut s, ic = 1.0 / c; over the taps in row-major order (dy = -r..r outer,
 * dx = -r..r inner) that lie inside the image (no padding), are valid and have |z_q - z_p| < c:
 *     t = (z_q - z_p) ic,  b = 1.0 - t t,  w = wa (b b),  num += w z_q,  den += w;
 * out[p] = (float)(num / den) (the centre tap always counts, with w = 1).  An invalid centre gives 0.0f.  out is
 * float32 metres [H, W], device memory.  The range width grows with z^2 as the sensor's noise does: sigma_depth is
 * the width in metres at 1 m.  Deterministic: the same input gives the same bits.
 * A null depth or out, out overlapping depth, H or W <= 0 or > 32768, depth_dtype other than 0 / 1 / 2, a radius
 * outside 1..BNV_DEPTH_FILTER_MAX_RADIUS, a max_depth, sigma_depth or range_cut that is not positive and finite, and
 * a confidence level without a map are BNV_ERR_INVALID_ARGUMENT before any HIP call. */
#define BNV_DEPTH_FILTER_MAX_RADIUS 8
int bnv_depth_filter(const void* depth, int depth_dtype, int H, int W, double max_depth, int radius,
                     double sigma_depth, double range_cut, const uint8_t* conf, int conf_level, float* out,
                     bnv_stream_t stream);

/* ---- Mesh normals and colours (bnv_fusion_amd/csrc/meshcolor.hip; bnv_fusion_amd/mesh.py: vertex_normals_tensors,
 * VertexColorer): the appearance of an extracted mesh -- area-weighted vertex normals, and per-vertex colours blended
 * from the RGB frames at full image resolution with a depth test against each frame's own depth image.  The reference
 * has no such stage (its only colour is the folded volume of TSDFVolume at the TSDF's voxel size);
 * tests/mesh_color_restatement.py restates what follows in numpy.  Every operation is one IEEE float64 rounding in the
 * order written (no contraction); division and sqrt are correctly rounded; rint is half to even.
 *
 * Normals.  vertices f32 [V, 3], faces i64 [T, 3], 1 <= V < 2^31 - 1, 0 <= T < 2^31 - 1.  Per face from the float32
 * coordinates: e1 = b - a, e2 = c - a; cx = e1y*e2z - e1z*e2y, cy = e1z*e2x - e1x*e2z, cz = e1x*e2y - e1y*e2x (the
 * area-weighted normal); q = (rint(cx 2^48), rint(cy 2^48), rint(cz 2^48)) as int64, added to the int64 sums of the
 * face's three corners with integer atomics: any order of the faces and any schedule gives the same sums.  Per vertex:
 * s = the three sums converted to float64 (to nearest even); a zero sum (an unreferenced vertex, degenerate faces only,
 * faces that cancel) gives (0, 0, 0); else len = sqrt((sx sx + sy sy) + sz sz), n = (float)(s / len).
 * The input is refused (device int32 *status = -1, else 0; normals_out is then unspecified) when a vertex is
 * non-finite, a face index is outside [0, V), or the mesh's total area reaches 2^12 square units (per face
 * area = 0.5 sqrt((cx cx + cy cy) + cz cz) must stay below 2^12 and the integer sum of rint(area 2^50) below 2^62,
 * the rule of bnv_mesh_components): |2 area 2^48| then stays inside int64.  Workspace:
 * bnv_mesh_normals_workspace_bytes (24 B per vertex + a header).  No allocation, synchronisation or host read.
 *
 * Colours.  The workspace (bnv_mesh_color_workspace_bytes) holds per vertex the float64 sums sum_r, sum_g, sum_b,
 * sum_w ([V, 4] at offset 0) and an int32 count of contributing frames ([V] at offset align256(32 V));
 * bnv_mesh_color_begin zeroes it.  bnv_mesh_color_accumulate adds 1 <= n_frames <= BNV_MESH_COLOR_MAX_FRAMES frames
 * in one launch.  One thread owns one vertex and walks the frames in the order given, so every vertex's additions
 * happen in frame order however the frames are split over launches: the result is bit-identical for any batching.
 * normals f32 [V, 3] (bnv_mesh_vertex_normals' output or the caller's own, unit length or zero).
 * A frame (bnv_mesh_color_frame_t, host memory; the images are device memory and only read): depth [height, width],
 * depth_dtype 0 = uint16 millimetres (d = (double)mm / 1000.0) or 1 = float32 metres; conf uint8 [height, width] or
 * NULL with conf_level as for bnv_depth_to_points (a pixel is kept when conf >= conf_level; a level without a
 * map is refused); rgb uint8 [color_height, color_width, 3]; K = (fx, fy, cx, cy) of the depth image and K_color of
 * the colour image (the same pose); T_cw float64 [12]: rows 0..2 of the WORLD-TO-CAMERA matrix, inverted by the caller
 * in float64; center: the camera centre in the world (the translation of T_wc).  Integer pixel coordinates are pixel
 * centres, the front end's convention.  Per vertex x (float32 as float64) with normal n and per frame:
 *   1. p_a = ((T[a][0] x0 + T[a][1] x1) + T[a][2] x2) + T[a][3];  skip unless near < p2 < max_depth.
 *   2. u = (fx p0) / p2 + cx,  v = (fy p1) / p2 + cy;  skip unless 0 <= u <= width - 1 and 0 <= v <= height - 1.
 *      x0 = floor(u), x1 = min(x0 + 1, width - 1), fu = u - x0; y0, y1, fv likewise.
 *   3. Bilinear weights of (y0, x0), (y0, x1), (y1, x0), (y1, x1): (1 - fu)(1 - fv), fu (1 - fv), (1 - fu) fv, fu fv.
 *      A neighbour passes when its depth d is finite, 0 < d < max_depth, its confidence passes the gate and
 *      |d - p2| <= depth_tol; the weight of one that does not is set to 0.  wsum = ((w0 + w1) + w2) + w3;  skip unless
 *      wsum > 0.  Background pixels at a silhouette are dropped, not blended in, and a vertex behind nearer geometry
 *      takes nothing from the frame.
 *   4. d = center - x, c = ((n0 d0 + n1 d1) + n2 d2) / sqrt((d0 d0 + d1 d1) + d2 d2);  skip unless c > cos_min;  a
 *      vertex whose normal is (0, 0, 0) takes part in no frame.  w = c / (p2 p2): proportional to the image area the
 *      surface element covers.
 *   5. When the colour image has the depth image's size and K_color == K: the corner weights are w_i / wsum at the
 *      same four pixels.  Otherwise u, v and the corners are recomputed with K_color and the colour image's size (skip
 *      when out of bounds) and the weights are the plain bilinear ones.  Per channel
 *      col = ((w0 c0 + w1 c1) + w2 c2) + w3 c3;  sum_rgb += w col,  sum_w += w,  count += 1.
 * bnv_mesh_color_resolve: colors_out uint8 [V, 3] = rint(sum / sum_w) clamped to [0, 255] where count > 0, else
 * fill[3]; observed_out uint8 [V] = count > 0; sum_w_out f64 [V] and count_out i32 [V] when not NULL.
 * Null pointers (conf, sum_w_out and count_out excepted), V <= 0, n_frames outside 1..BNV_MESH_COLOR_MAX_FRAMES, an
 * image size <= 0 or > 32768, depth_dtype other than 0 / 1, a non-finite K, K_color, T_cw or center, depth_tol
 * negative or non-finite, cos_min outside [0, 1), near negative or non-finite and max_depth not finite or <= near are
 * BNV_ERR_INVALID_ARGUMENT before any HIP call; a workspace below the size is BNV_ERR_WORKSPACE_TOO_SMALL.  Each
 * entry is a fixed sequence of launches on stream: no allocation, synchronisation or host read. */
#define BNV_MESH_COLOR_MAX_FRAMES 8
typedef struct {
  const void* depth;
  const uint8_t* conf;
  const uint8_t* rgb;
  int32_t depth_dtype, conf_level;
  int32_t height, width, color_height, color_width;
  double K[4];
  double K_color[4];
  double T_cw[12];
  double center[3];
} bnv_mesh_color_frame_t;
int bnv_mesh_normals_workspace_bytes(int64_t n_vertices, int64_t* bytes);
int bnv_mesh_vertex_normals(const float* vertices, int64_t n_vertices, const int64_t* faces, int64_t n_faces,
                            void* workspace, int64_t ws_bytes, float* normals_out, int32_t* status,
                            bnv_stream_t stream);
int bnv_mesh_color_workspace_bytes(int64_t n_vertices, int64_t* bytes);
int bnv_mesh_color_begin(void* workspace, int64_t ws_bytes, int64_t n_vertices, bnv_stream_t stream);
int bnv_mesh_color_accumulate(const float* vertices, const float* normals, int64_t n_vertices,
                              const bnv_mesh_color_frame_t* frames_host, int32_t n_frames, double depth_tol,
                              double cos_min, double near, double max_depth, void* workspace, int64_t ws_bytes,
                              bnv_stream_t stream);
int bnv_mesh_color_resolve(const void* workspace, int64_t ws_bytes, int64_t n_vertices, const uint8_t fill[3],
                           uint8_t* colors_out, uint8_t* observed_out, double* sum_w_out, int32_t* count_out,
                           bnv_stream_t stream);

/* ---- Volume planning (bnv_fusion_amd/csrc/plan.hip; bnv_fusion_amd/plan.py: VolumePlanner, plan_volume): the extent
 * of the scene and the per-frame voxel statistics of candidate voxel sizes, from the depth frames themselves and before
 * anything is fused.  Both passes read a frame exactly as bnv_encode_begin_depth does: depth / depth_dtype /
 * max_depth / conf / conf_level as for bnv_depth_to_points, a pixel is valid when 0 < z < max_depth and (with a
 * map) conf >= conf_level, and its world point p is the front end's float32 point (float32 pixel rays, float64
 * products with T_wc in the written order, one rounding).  Everything is integer counting: any schedule gives the same
 * numbers; tests/plan_restatement.py restates both passes in numpy.
 *
 * Pass 1, bnv_plan_extent.  dirs_host float64 [n_dirs, 3] (host), 1 <= n_dirs <= BNV_PLAN_MAX_DIRS; n_bins a power of
 * two in [2, 65536]; hist uint64 [n_dirs, n_bins], device memory the caller zeroes once and reads once: the counters
 * accumulate over calls.  Per valid pixel and direction d:
 *     t = (d0 (double)p0 + d1 (double)p1) + d2 (double)p2,  q = floor(t / bin_size) limited to [-n_bins, n_bins] (NaN:
 *     -n_bins),  b = clamp((int64)q + n_bins / 2, 0, n_bins - 1),  hist[d][b] += 1.
 * Bins 0 and n_bins - 1 are overflow bins.  A workgroup counts its 256 pixels in an LDS window first (one global atomic
 * per touched bin) unless they span more than 256 bins.
 *
 * Pass 2, bnv_plan_count.  T_wc_host is the ALIGNED pose (axis_align_mat @ T_wc, formed by the caller in float64);
 * grids_host: 1 <= n_sizes <= BNV_PLAN_MAX_SIZES grids as bnv_encode_* take them (the sharding and mode members are
 * not read), each of fewer than 2^31 voxels.  Per grid: every valid pixel whose point passes the encoder's bounds mask
 * counts as a point, and each of its 8 corner voxels (floor / ceil per axis of (p - bound_min) / voxel_size; two corners
 * that name the same voxel both count) as one (point, corner) pair of that voxel.  rows_out int64
 * [n_sizes, BNV_PLAN_ROW_WORDS], device memory zeroed by the caller, one row per grid for THIS frame:
 *     [0] points in bounds (nv)   [1] touched voxels (U)   [2] status   [3] 0
 *     [4 + c], c = 1 .. BNV_PLAN_HIST_CAP - 1: voxels with exactly c pairs;  [4 + BNV_PLAN_HIST_CAP]: with that many or
 *     more ([4] and the words behind the histogram stay 0).
 * The encoder's counters of the same frame follow: n_avg_pts = (float)(8 nv) / (float)U, rows written = the histogram's
 * sum from min_pts_in_grid up.  status bit 0: the hash table went past half load; bit 1: a pair found no free slot (the
 * row's counts are then short).  With table_slots = 0 every table has the smallest power of two of slots that is at least
 * 2 min(8 H W, voxels), so neither can happen; table_slots > 0 (a power of two, 64 .. 2^30) forces that size on every
 * table.  workspace: bnv_plan_workspace_bytes (8 B per slot and 4 B per 256 pixels, per grid; 0 for invalid arguments),
 * initialised once by bnv_plan_workspace_reset with the same H, W, grids and table_slots; every call leaves the tables
 * empty for the next frame.
 * Null pointers (conf excepted), H or W <= 0 or > 32768 or more than 2^24 pixels, depth_dtype other than 0 / 1 / 2, a
 * max_depth or bin_size that is not positive and finite, non-finite intrinsics, pose or directions, a zero focal
 * length, a confidence level without a map, n_dirs, n_bins, n_sizes or table_slots out of range and a grid with a
 * non-positive or non-finite member or 2^31 voxels or more are BNV_ERR_INVALID_ARGUMENT before any HIP call; a
 * workspace below the size is BNV_ERR_WORKSPACE_TOO_SMALL.  Fixed sequences of launches on stream: no allocation,
 * synchronisation or host read.
 *
 * Pass 0, bnv_plan_normals: the histogram of surface normals from which the host finds the scene's Manhattan frame
 * (plan.py: ManhattanFrame) when the world's axes are not the room's.  hist int64 [6 n_side^2, 4], device memory the
 * caller zeroes once: it accumulates over calls.  Pixel (v, u) counts under these rules, all in float64 with one
 * rounding per operation in the written order (tests/manhattan_restatement.py restates them in numpy):
 *     validity  the pixel and its four neighbours (v, u -+ step), (v -+ step, u) lie in the image and are valid: z finite,
 *               0 < z <= max_depth (uint16: z = d / 1000.0) and, with a map, conf >= conf_level -- inclusive, unlike the
 *               0 < z < max_depth of passes 1 and 2: a pixel at exactly max_depth votes for a direction here and is
 *               no point there;
 *     jump      each neighbour q has |z_q - z_c| <= jump * z_c;
 *     points    P = ((u - cx) / fx * z, (v - cy) / fy * z, z);
 *     normal    n = (P(u + step) - P(u - step)) x (P(v + step) - P(v - step)), each component a * b - c * d; negated
 *               when (n0 Pc0 + n1 Pc1) + n2 Pc2 > 0 (it faces the camera); w_r = (R_r0 n0 + R_r1 n1) + R_r2 n2 with R
 *               the rotation of T_wc; w / sqrt((w0 w0 + w1 w1) + w2 w2); a length that is 0 or not finite skips the pixel;
 *     bin       m the index of the largest |w_i| (ties: the lower), face = 2 m + (w_m < 0); for a = (m + 1) % 3 and
 *               b = (m + 2) % 3: i = clamp(floor(((w_a / |w_m| + 1) * 0.5) * n_side), 0, n_side - 1);
 *               bin = (face * n_side + i_a) * n_side + i_b;
 *     sums      hist[bin] += {1, rint(w_0 * 2^20), rint(w_1 * 2^20), rint(w_2 * 2^20)}.
 * Everything accumulated is an integer: the result does not depend on the schedule, the launch shape or the order of the
 * frames.  A workgroup sums what shares a bin in LDS and issues four 64-bit global atomics per distinct bin.
 * 1 <= step <= 64, jump positive and finite, 4 <= n_side <= 64 and the frame arguments as above, else
 * BNV_ERR_INVALID_ARGUMENT before any HIP call.  One launch on stream: no allocation, synchronisation or host read. */
#define BNV_PLAN_MAX_DIRS 64
#define BNV_PLAN_MAX_SIZES 8
#define BNV_PLAN_ROW_WORDS 72
#define BNV_PLAN_HIST_CAP 64
size_t bnv_plan_workspace_bytes(int H, int W, const bnv_grid_t* grids_host, int n_sizes, int64_t table_slots);
int bnv_plan_workspace_reset(void* workspace, size_t ws_bytes, int H, int W, const bnv_grid_t* grids_host, int n_sizes,
                             int64_t table_slots, bnv_stream_t stream);
int bnv_plan_extent(const void* depth, int depth_dtype, int H, int W, const double* intr_host, const double* T_wc_host,
                    double max_depth, const uint8_t* conf, int conf_level, const double* dirs_host, int n_dirs,
                    double bin_size, int n_bins, uint64_t* hist, bnv_stream_t stream);
int bnv_plan_count(const void* depth, int depth_dtype, int H, int W, const double* intr_host, const double* T_wc_host,
                   double max_depth, const uint8_t* conf, int conf_level, const bnv_grid_t* grids_host, int n_sizes,
                   int64_t table_slots, void* workspace, size_t ws_bytes, int64_t* rows_out, bnv_stream_t stream);
int bnv_plan_normals(const void* depth, int depth_dtype, int H, int W, const double* intr_host, const double* T_wc_host,
                     double max_depth, const uint8_t* conf, int conf_level, int step, double jump, int n_side,
                     int64_t* hist, bnv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* BNV_FUSION_H */
