// vtgs_kernels.h -- the ONE declaration of every kernel that is launched from a translation unit other than the one that
// defines it.  The defining file and every launching file include it, so a definition (or an explicit instantiation, which
// takes its type from here) that drifts from what a launcher sees does not compile.  Default template arguments sit here,
// the only place C++ allows them; launch bounds stay with the definitions.
#pragma once
#include "vtgs_internal.h"

namespace vtgs {

// ---- vtgs_binning.hip ------------------------------------------------------------------------------------------------------
template <int LDSBINS, int MODE>
__global__ void project_and_bin(
    CamScalars cs, const float* __restrict__ Vp, const float* __restrict__ PVp, int n,
    const float* __restrict__ means3D, const float* __restrict__ opacities,
    const float* __restrict__ scales, const float* __restrict__ rotations,
    int32_t* __restrict__ radii, GeomRec* __restrict__ geom, GaussAux* __restrict__ gaux,
    uint32_t* __restrict__ tile_cnt, unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals,
    Counters* __restrict__ ctr, BlockStats* __restrict__ block_stats, unsigned long long capacity, uint32_t tile_cap,
    DeferRec* __restrict__ defer_list);
template <int LDSBINS, int MODE>
__global__ void project_and_bin_capped(
    CamScalars cs, const float* __restrict__ Vp, const float* __restrict__ PVp, int n,
    const float* __restrict__ means3D, const float* __restrict__ opacities,
    const float* __restrict__ scales, const float* __restrict__ rotations,
    int32_t* __restrict__ radii, GeomRec* __restrict__ geom, GaussAux* __restrict__ gaux,
    uint32_t* __restrict__ tile_cnt, unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals,
    Counters* __restrict__ ctr, BlockStats* __restrict__ block_stats, unsigned long long capacity, uint32_t tile_cap,
    DeferRec* __restrict__ defer_list);
template <bool PLANNED>
__global__ void bin_deferred_splats(
    CamScalars cs, GaussAux* __restrict__ gaux, uint32_t* __restrict__ tile_cnt,
    unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals, Counters* __restrict__ ctr,
    const DeferRec* __restrict__ list, uint32_t n, unsigned long long capacity, uint32_t tile_cap, uint32_t large_grid);
__global__ void finalize_forward(const uint32_t* __restrict__ tile_cnt, uint32_t tiles,
                                 Counters* __restrict__ ctr, unsigned long long capacity,
                                 uint32_t tile_cap, const BlockStats* __restrict__ block_stats,
                                 uint32_t nblocks, VtgsForwardInfo* host_record,
                                 const uint32_t* __restrict__ plan, uint32_t* __restrict__ plan_next);
template <bool WIDE>
__global__ void sort_tiles(const uint32_t* __restrict__ tile_cnt, unsigned long long* __restrict__ keys,
                           uint32_t* __restrict__ vals, uint32_t* __restrict__ sorted_gid,
                           uint32_t* __restrict__ sorted_inst, uint32_t tile_first, uint32_t tiles,
                           uint32_t tile_cap, const Counters* __restrict__ ctr, int packed,
                           const uint32_t* __restrict__ plan, uint32_t bin_limit,
                           unsigned long long long_only_capacity, int mid_done);
__global__ void sort_long_lists(const uint32_t* __restrict__ tile_cnt, unsigned long long* __restrict__ keys,
                                uint32_t* __restrict__ vals, uint32_t* __restrict__ sorted_gid,
                                uint32_t* __restrict__ sorted_inst, uint32_t tile_first, uint32_t tiles,
                                uint32_t tile_cap, const Counters* __restrict__ ctr,
                                const uint32_t* __restrict__ plan, uint32_t bin_limit,
                                unsigned long long long_only_capacity, int counting, uint32_t lo);

// ---- vtgs_composite_q.hip: the product forward ------------------------------------------------------------------------------
template <int MODE>
__global__ void composite_forward_q(
    CamScalars cs, const float* __restrict__ bg, uint32_t nblk,
    const uint32_t* __restrict__ tile_cnt, uint32_t tile_cap, uint32_t* sorted_gid,
    const GeomRec* __restrict__ geom, const float* __restrict__ colors,
    float* __restrict__ out_color, float* __restrict__ out_depth, float* __restrict__ final_T,
    const Counters* __restrict__ ctr, const float* __restrict__ colors_b, float* __restrict__ out_color_b,
    int sort_mode, const unsigned long long* __restrict__ bin_keys, const uint32_t* __restrict__ bin_vals,
    uint32_t* sorted_inst, FinalizeArgs fin, uint8_t* __restrict__ qmask, uint32_t* __restrict__ step_counters);

// ---- vtgs_composite_backward.h: lane = pixel forms (PXL) in vtgs_composite_backward.hip, quad forms in the test-only library
template <int WAVES, bool DUAL, bool PXL, bool B1 = false>
__global__ void composite_backward_mx(
    CamScalars cs, const float* __restrict__ bg, uint32_t nblk,
    const uint32_t* __restrict__ tile_cnt, uint32_t tile_cap, const uint32_t* __restrict__ sorted_gid,
    const uint32_t* __restrict__ sorted_inst, const GeomRec* __restrict__ geom, const float* __restrict__ colors,
    const float* __restrict__ out_color, const float* __restrict__ grad_color, const float* __restrict__ final_T,
    float* __restrict__ grad_inst, const Counters* __restrict__ ctr, const float* __restrict__ colors_b,
    const float* __restrict__ out_color_b, const float* __restrict__ grad_color_b, uint32_t* __restrict__ dbg);

// ---- vtgs_gather.hip --------------------------------------------------------------------------------------------------------
template <bool DUAL, bool FRAME = false, bool COV3D = false, bool B1 = false>
__global__ void gather_splat_grads(
    CamScalars cs, const float* __restrict__ Vp, const float* __restrict__ PVp, int n,
    const float* __restrict__ means3D, const float* __restrict__ opacities,
    const float* __restrict__ scales, const float* __restrict__ rotations,
    const GaussAux* __restrict__ gaux, const float* __restrict__ grad_inst, int moments_scaled_by_opacity,
    float* __restrict__ g_means3D, float* __restrict__ g_means2D, float* __restrict__ g_colors,
    float* __restrict__ g_opacities, float* __restrict__ g_scales, float* __restrict__ g_rotations,
    const Counters* __restrict__ ctr, float* __restrict__ g_colors_b, FrameEpilogue fe = FrameEpilogue{});
__global__ void mark_visible_kernel(const float* __restrict__ Vp, int n,
                                    const float* __restrict__ means3D, uint8_t* __restrict__ out);

// ---- vtgs_frame.hip ---------------------------------------------------------------------------------------------------------
__global__ void band_owner_kernel(
    CamScalars cs, const float* __restrict__ Vp, const float* __restrict__ PVp, int n, const float* __restrict__ means3D,
    const float* __restrict__ scales, int scales_are_log, const float* __restrict__ cam_q, const float* __restrict__ cam_t,
    float margin_px, float growth, const uint8_t* __restrict__ owned, uint8_t* __restrict__ mask_out,
    uint32_t* __restrict__ escapes, int32_t* __restrict__ centre_rows);

// ---- vtgs_densify.hip: exact lower median (radix select) and the densification step ------------------------------------------
constexpr uint32_t kMedianChunk = 4096;     // values a workgroup of 256 takes per trip (16 per thread); grid-stride beyond kMedianMaxGrid
constexpr uint32_t kMedianMaxGrid = 1024;
// Head of the caller's scratch.  The three histograms and the NaN counter are zeroed by ONE fill in front of pass 0; the words
// behind them are written by workgroup 0 of a pass for the workgroups of the next (every field is written before it is read).
struct alignas(16) MedianScratch {
  uint32_t hist0[2048], hist1[2048], hist2[1024];   // key bits 31..21, 20..10, 9..0
  uint32_t nan_count, pad0[3];
  uint32_t digit0, rank1;        // pass 1: the bucket of hist0 that holds the rank, and the rank inside it
  uint32_t prefix2, rank2;       // pass 2: key bits 31..10 of the median, and the rank among the keys that share them
  float median;                  // densify_count: the value, for densify_emit
  uint32_t pad1[3];
};
constexpr size_t kMedianClearBytes = offsetof(MedianScratch, digit0);
static_assert(sizeof(MedianScratch) % 16 == 0 && offsetof(MedianScratch, hist1) % 16 == 0 && offsetof(MedianScratch, hist2) % 16 == 0,
              "MedianScratch: the bucket search reads the histograms as 16-byte words");
// what the median is taken of: `values`, or (values == NULL) the depth error |gt_depth - depth| * (gt_depth > 0) formed on the fly
struct MedianSource { const float* values; const float* depth; const float* gt_depth; };
template <int PASS>
__global__ void lower_median_pass(MedianSource src, uint32_t n, MedianScratch* __restrict__ ms);
__global__ void lower_median_finish(uint32_t n, MedianScratch* __restrict__ ms, float* __restrict__ out_median,
                                    uint32_t* __restrict__ out_nan_count);

constexpr uint32_t kDensifyChunk = 512;     // consecutive pixels per workgroup of 256 (two steps): one count per chunk
struct DensifyArgs {
  int W, H, dW, dH;                         // dW == 0: no dense set
  int rx, ry, mrx, mry;                     // dW / W, dH / H; dW / mask width, dH / mask height (the integer nearest rule)
  int mW;
  const float* depth_sil;                   // [3,H,W]; NULL = seed mode
  const float* gt_im; const float* gt_depth; const float* k;
  const float* gt_im_d; const float* gt_depth_d; const float* k_d;
  const uint8_t* mask;                      // NULL = all set
  const float* w2c; const float* cam_rots; const float* cam_trans; int frames, t;
  float sil_thres, time_value;
  int scale_columns, n, capacity;
  float* means3D; float* rgb; float* rot; float* opac; float* log_scales; float* timestep;
  MedianScratch* ms;
  uint32_t* counts;                         // [blocks_ori + blocks_dense] selected pixels per chunk, ori chunks first
  uint32_t* unexplained;                    // [blocks_ori] pixels of the non-presence mask per chunk
  uint32_t blocks_ori, blocks_dense;
  VtgsDensifyInfo* info;
};
__global__ void densify_count(DensifyArgs a);
__global__ void densify_emit(DensifyArgs a);

// ---- vtgs_keyframes.hip: keyframe overlap counts, all keyframes in one pass ----------------------------------------------------
constexpr uint32_t kKeyframeSliceMax = 256;   // keyframes per blockIdx.y slice at most: the LDS counters of a workgroup
struct alignas(16) KeyframeRow {              // written by keyframe_fold for keyframe_overlap (uniform loads)
  float m[12];                                // K [R|t] of the keyframe, row-major 3x4
  int32_t slot;                               // row of kf_depth (negative: the keyframe counts 0)
  uint32_t pad[3];
};
struct KeyframeArgs {
  int W, H;
  const float* depth; const float* k; const float* w2c;
  const int32_t* sampled_rc; int samples;     // NULL, 0: dense
  const float* kf_w2c; const float* kf_depth; const int32_t* slots; int K;
  float edge, thresh;
  uint8_t* pair_mask;
  KeyframeRow* rows;                          // [K]
  uint32_t* seen; uint32_t* repeated;         // sampled mode: a bit per pixel each, zeroed in front of keyframe_mark_repeats
  uint32_t* record;                           // [K + 3]
  uint32_t per_slice;                         // keyframes per blockIdx.y
};
__global__ void keyframe_fold(KeyframeArgs a);
__global__ void keyframe_mark_repeats(KeyframeArgs a);
// `rows` = a.rows as a read-only, non-aliased kernel argument: the loop's row loads become scalar loads
__global__ void keyframe_overlap(KeyframeArgs a, const KeyframeRow* __restrict__ rows);

// ---- vtgs_masks.hip: visibility, far-depth and outlier-depth masks of the tracking loss in one pass ----------------------------
struct alignas(16) MaskRow {                  // written by tracking_mask_fold for tracking_mask (uniform loads)
  float m[12];                                // K W_j[:3,:] inverse(curr_w2c), row-major 3x4
  uint32_t pad[4];
};
struct MaskArgs {
  int W, H, n;                                // n = overlapping frames, 0..3 (0: no visibility mask)
  const float* gt; const float* k; const float* curr_w2c;
  const float* ov_w2c0; const float* ov_w2c1; const float* ov_w2c2;
  const float* ov_depth0; const float* ov_depth1; const float* ov_depth2;
  float thres; int use_far; float far;
  const float* rendered;                      // plane 0 of the depth / silhouette render; NULL = no outlier mask
  float* err;                                 // [H*W] scratch, NULL = no outlier mask
  const float* median;                        // the lower median of err, in scratch
  MaskRow* rows;                              // [3]
  float* out; uint8_t* out_u8; uint8_t* out_bits;
};
__global__ void tracking_mask_fold(MaskArgs a);
__global__ void tracking_mask_error(MaskArgs a);
// `rows` = a.rows as a read-only, non-aliased kernel argument: the row loads become scalar loads
__global__ void tracking_mask(MaskArgs a, const MaskRow* __restrict__ rows);

// ---- the cross-check composites of the test-only libvtgs_xcheck.so (vtgs_xcheck_composites.hip, vtgs_composite_bq.hip) -------
__global__ void composite_forward(
    CamScalars cs, const float* __restrict__ bg, uint32_t nblk,
    const uint32_t* __restrict__ tile_cnt, uint32_t tile_cap, const uint32_t* __restrict__ sorted_gid,
    const GeomRec* __restrict__ geom, const float* __restrict__ colors,
    float* __restrict__ out_color, float* __restrict__ out_depth, float* __restrict__ final_T,
    const Counters* __restrict__ ctr);
template <int WAVES, bool DUAL>
__global__ void composite_forward_mx(
    CamScalars cs, const float* __restrict__ bg, uint32_t nblk,
    const uint32_t* __restrict__ tile_cnt, uint32_t tile_cap, const uint32_t* __restrict__ sorted_gid,
    const GeomRec* __restrict__ geom, const float* __restrict__ colors,
    float* __restrict__ out_color, float* __restrict__ out_depth, float* __restrict__ final_T,
    const Counters* __restrict__ ctr, const float* __restrict__ colors_b, float* __restrict__ out_color_b);
template <int WAVES, bool DUAL>
__global__ void composite_forward_px(
    CamScalars cs, const float* __restrict__ bg, uint32_t nblk,
    const uint32_t* __restrict__ tile_cnt, uint32_t tile_cap, const uint32_t* __restrict__ sorted_gid,
    const GeomRec* __restrict__ geom, const float* __restrict__ colors,
    float* __restrict__ out_color, float* __restrict__ out_depth, float* __restrict__ final_T,
    const Counters* __restrict__ ctr, const float* __restrict__ colors_b, float* __restrict__ out_color_b);
__global__ void composite_backward(
    CamScalars cs, const float* __restrict__ bg, uint32_t nblk16,
    const uint32_t* __restrict__ tile_cnt, uint32_t tile_cap, const uint32_t* __restrict__ sorted_gid,
    const uint32_t* __restrict__ sorted_inst, const GeomRec* __restrict__ geom, const float* __restrict__ colors,
    const float* __restrict__ out_color, const float* __restrict__ grad_color, const float* __restrict__ final_T,
    float* __restrict__ grad_inst, const Counters* __restrict__ ctr);
__global__ void composite_backward_q(
    CamScalars cs, const float* __restrict__ bg, uint32_t nblk,
    const uint32_t* __restrict__ tile_cnt, uint32_t tile_cap, const uint32_t* __restrict__ sorted_gid,
    const uint32_t* __restrict__ sorted_inst, const uint8_t* __restrict__ qmask, const GeomRec* __restrict__ geom,
    const float* __restrict__ colors, const float* __restrict__ out_color, const float* __restrict__ grad_color,
    const float* __restrict__ final_T, float* __restrict__ grad_inst, const Counters* __restrict__ ctr,
    uint32_t* __restrict__ step_counters);

}  // namespace vtgs
