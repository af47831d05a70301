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
