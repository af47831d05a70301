// vtgs_gather.hip -- the per-Gaussian end of the backward (gfx950, wave64): gather_splat_grads sums the (splat, tile) records
// that composite_backward_mx (vtgs_composite_backward.h) left in the scratch and runs the projection backward
// (splat_backward, vtgs_math.h) on the sums; mark_visible_kernel is the operator's markVisible.  Product only: libvtgs.so.
#include "vtgs_internal.h"
#include "vtgs_kernels.h"

namespace vtgs {

// one thread per Gaussian: re-centre and sum its instance records (fixed order), then the projection backward.
// FRAME (dual render of the fused caller chain): the adjoint of vtgs_prepare_frame runs here, on the gradients while they
// are still in registers -- same formulas and the same block reduction as prepare_frame_backward_kernel (vtgs_frame.hip);
// the results agree to float32 rounding -- instead of writing six dense [N, .] arrays for that kernel to read back
// (~160 bytes per Gaussian less traffic, one launch less; on a rank of the tile-row partition no dense zero arrays at all).
// COV3D (the operator's cov3D_precomp): `scales` holds the six covariance entries per Gaussian and g_scales receives their
// six gradients; `rotations` / g_rotations are not touched.
// B1: the 12-float records of composite_backward_mx<.., B1> (second image differentiated through its first channel only).
template <bool DUAL, bool FRAME, bool COV3D, bool B1>
__global__ __launch_bounds__(256) void gather_splat_grads(
    CamScalars cs, const float* __restrict__ Vp, const float* __restrict__ PVp, int n,
    const float* __restrict__ means3D, const float* __restrict__ opacities,
    const float* __restrict__ scales, const float* __restrict__ rotations,
    const GaussAux* __restrict__ gaux, const float* __restrict__ grad_inst, int moments_scaled_by_opacity,
    float* __restrict__ g_means3D, float* __restrict__ g_means2D, float* __restrict__ g_colors,
    float* __restrict__ g_opacities, float* __restrict__ g_scales, float* __restrict__ g_rotations,
    const Counters* __restrict__ ctr, float* __restrict__ g_colors_b, FrameEpilogue fe) {
  // Workgroups walk the map from its END: a SLAM map is appended to (densification, new submaps), and the appended Gaussians
  // are the ones the optimiser has grown the most -- the workgroups with the most records.  Started last they were the kernel's
  // tail; started first, the light workgroups fill in behind them.  (The per-workgroup pose partials keep their row: the
  // block index below is only the position in the map.)
  const uint32_t blk = gridDim.x - 1u - blockIdx.x;
  const int gid = (int)(blk * 256u + threadIdx.x);
  if (ctr->overflow) {
    // The forward did not complete: nothing valid to differentiate.  The Python layer never gets here (its checked forward
    // answers an overflow before it returns); a bare C-ABI caller that ignored the overflow of an asynchronous forward
    // gets DEFINED gradients -- zeros -- instead of whatever the output buffers held.
    if (gid < n) {
      if constexpr (FRAME) {
        const int row = fe.idx ? fe.idx[gid] : gid;
        if (fe.flags & 1u) {
          fe.g_means3D[3 * row] = fe.g_means3D[3 * row + 1] = fe.g_means3D[3 * row + 2] = 0.f;
          reinterpret_cast<float4*>(fe.g_unnorm_rot)[row] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (fe.flags & 4u) {
          fe.g_logit[row] = 0.f; fe.g_log_scales[row] = 0.f;
          fe.g_rgb[3 * row] = fe.g_rgb[3 * row + 1] = fe.g_rgb[3 * row + 2] = 0.f;
        }
      } else {
        for (int i = 0; i < 3; ++i) {
          if (g_means3D) g_means3D[3 * gid + i] = 0.f;
          if (g_means2D) g_means2D[3 * gid + i] = 0.f;
          if (g_colors) g_colors[3 * gid + i] = 0.f;
          if (g_scales && !COV3D) g_scales[3 * gid + i] = 0.f;
          if constexpr (DUAL) { if (g_colors_b) g_colors_b[3 * gid + i] = 0.f; }
        }
        if constexpr (COV3D) { if (g_scales) for (int i = 0; i < 6; ++i) g_scales[6 * gid + i] = 0.f; }
        if (g_opacities) g_opacities[gid] = 0.f;
        if (g_rotations && !COV3D) reinterpret_cast<float4*>(g_rotations)[gid] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    if constexpr (FRAME) {
      if ((fe.flags & 2u) && threadIdx.x < 12) fe.pose_partials[(size_t)blk * 12 + threadIdx.x] = 0.f;
    }
    return;
  }
  const CamParams cam = load_cam(cs, Vp, PVp);
  const bool live = gid < n;                     // nobody leaves: the wavefront sums the records of its big splats together
  // (an early exit for wavefronts without any instance -- 7/8 of them on a rank of an 8-way partition -- was measured and
  //  dropped: it puts the camera's scalar loads behind the gaux load for the wavefronts that stay, +2 us whole frame, +1 in a band)
  GaussAux ga = live ? gaux[gid] : GaussAux{0u, 0u};
  if ((unsigned long long)ga.inst_base + ga.inst_cnt > (unsigned long long)cs.scratch_records) ga.inst_cnt = 0u;   // (CamScalars::scratch_records)
  SplatGrads g;
  for (int i = 0; i < 3; ++i) { g.mean3D[i] = g.mean2D[i] = g.color[i] = g.scale[i] = 0.f; }
  g.opacity = 0.f; g.rot[0] = g.rot[1] = g.rot[2] = g.rot[3] = 0.f;
  float cb0 = 0.f, cb1 = 0.f, cb2 = 0.f;         // dual: dL/d(second render's colours)
  // ---- the gradient records of the wavefront's 64 splats -----------------------------------------------------------------
  // Round 6.  Until round 5 every lane walked ITS OWN records in a loop (the first four requested ahead, the rest one
  // dependent load after the other): a wavefront took as long as its largest splat, and an optimised SLAM map has a heavy tail
  // -- after 20 frames of mapping 8 % of the Gaussians of the synthetic Replica sequence have 7 .. 64 instances, so nearly every
  // wavefront holds one and ran 16 .. 64 serial trips to memory (152 us against 54 us on the fresh map,
  // gpurun_out/r6/slamlate_b_dens.txt).  Now: the first kGatherAhead records of every lane as before (in flight with the
  // projection's inputs; 93 % of the splats of a fresh map have no more) and the EXCESS records of the wavefront's splats as one
  // list, 64 records per step, every lane one record: position j of the list belongs to the last lane whose first position V is
  // <= j (six-step search over the lanes' scan with ds_bpermute); the lane re-centres its record with the owner's centre and
  // parks the ten sums in a 3 KB LDS window; then every owner adds ITS rows of the window, in index order -- the order the
  // per-lane loop had -- from LDS, not from memory.  No float atomics, no cross-lane float reduction.  (The list for ALL records
  // cost the fresh map 9 us: three windows where four loads in flight did, gpurun_out/r6/timing_g_head.log.)
  // A Gaussian with more than kBigInst instances (a splat grown over a hole of the map has thousands) is summed by the whole
  // wavefront instead, 64 records at a time with a butterfly at the end (its own fixed order).
  constexpr uint32_t kBigInst = 64;
  const bool big = ga.inst_cnt > kBigInst;
  // dual: 14 floats = seven float2 (56-byte stride); single render: 10 floats = five float2 (40-byte stride)
  auto load_record = [&](uint32_t inst, float4& a, float4& b, float4& c, float4& d) {
    if constexpr (B1) {
      const float4* rec = reinterpret_cast<const float4*>(grad_inst) + (size_t)inst * (kGradRecDual1 / 4);
      a = rec[0]; b = rec[1]; c = rec[2]; d = c;
    } else if constexpr (DUAL) {
      const float2* rec = reinterpret_cast<const float2*>(grad_inst) + (size_t)inst * (kGradRecDual / 2);
      const float2 f0 = rec[0], f1 = rec[1], f2 = rec[2], f3 = rec[3], f4 = rec[4], f5 = rec[5], f6 = rec[6];
      a = make_float4(f0.x, f0.y, f1.x, f1.y); b = make_float4(f2.x, f2.y, f3.x, f3.y);
      c = make_float4(f4.x, f4.y, f5.x, f5.y); d = make_float4(f6.x, 0.f, 0.f, 0.f);
    } else {
      const float2* rec = reinterpret_cast<const float2*>(grad_inst) + (size_t)inst * (kGradRec / 2);
      const float2 f0 = rec[0], f1 = rec[1], f2 = rec[2], f3 = rec[3], f4 = rec[4];
      a = make_float4(f0.x, f0.y, f1.x, f1.y); b = make_float4(f2.x, f2.y, f3.x, f3.y);
      c = make_float4(f4.x, f4.y, 0.f, 0.f); d = c;
    }
  };
  // record = tile-local moments (U0, UX, UY, UXX, UXY, UYY), colour sums (3 or 6), tile id; (u, v) = the splat's centre
  auto add_record = [&](SplatMoments& M, float& c0, float& c1, float& c2, float4 a, float4 b, float4 c, float4 d, float u, float v,
                        float ulo, float vlo) {
    uint32_t tile;
    if constexpr (B1) {
      tile = __float_as_uint(c.z);
      c0 += c.y;
    } else if constexpr (DUAL) {
      tile = __float_as_uint(d.x);
      c0 += c.y; c1 += c.z; c2 += c.w;
    } else {
      tile = __float_as_uint(c.y);
    }
    const int ty = (int)(tile / (uint32_t)cam.gx8), tx = (int)(tile - (uint32_t)ty * (uint32_t)cam.gx8);
    const float sx = (u - ((float)(tx * kSubTile) + 3.5f)) + ulo, sy = (v - ((float)(ty * kSubTile) + 3.5f)) + vlo;   // as tile_coefficients
    const float U0 = a.x, UX = a.y, UY = a.z, UXX = a.w, UXY = b.x, UYY = b.y;
    M.m[0] += U0;
    M.m[1] += sx * U0 - UX;                                     // d = centre - pixel = s - X
    M.m[2] += sy * U0 - UY;
    M.m[3] += sx * sx * U0 - 2.f * sx * UX + UXX;
    M.m[4] += sx * sy * U0 - sx * UY - sy * UX + UXY;
    M.m[5] += sy * sy * U0 - 2.f * sy * UY + UYY;
    M.m[6] += b.z; M.m[7] += b.w; M.m[8] += c.x;
  };
  float sc[3] = {0.f, 0.f, 0.f}, q[4] = {1.f, 0.f, 0.f, 0.f}, op = 0.f;
  float c6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, g6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  Splat sp{}; SplatAux aux{};
  SplatMoments mo;
  for (int k = 0; k < 9; ++k) mo.m[k] = 0.f;
  bool ok = false;
  constexpr uint32_t kGatherAhead = 4;
  // the wavefront's list of EXCESS records: lane l's sit at positions [V, V + my_cnt) (wave-level scan; a big splat is not in it)
  constexpr int kRow = 12;                                          // floats per parked record: 9 sums + up to 3 second-set colours
  __shared__ __attribute__((aligned(16))) float lds_rows[4][64 * kRow];
  float* __restrict__ rows = lds_rows[threadIdx.x >> 6];
  const int ln = lane_id();
  const uint32_t my_cnt = (live && !big && ga.inst_cnt > kGatherAhead) ? ga.inst_cnt - kGatherAhead : 0u;
  const uint32_t incl_cnt = wave_incl_scan(my_cnt);
  const uint32_t V = incl_cnt - my_cnt;
  const uint32_t T = (uint32_t)__builtin_amdgcn_readlane((int)incl_cnt, 63);
  auto owner_of = [&](uint32_t j) {                                 // last lane whose V <= j (j < T: that lane holds position j)
    int lo = 0, hi = 63;
#pragma unroll
    for (int it = 0; it < 6; ++it) {
      const int mid = (lo + hi + 1) >> 1;
      const uint32_t vm = (uint32_t)__builtin_amdgcn_ds_bpermute(mid << 2, (int)V);
      const bool le = vm <= j;
      lo = le ? mid : lo; hi = le ? hi : mid - 1;
    }
    return lo;
  };
  // the lane's first records are requested up front: their addresses only need gaux, so they are in flight together with the
  // inputs of the projection instead of behind its arithmetic
  float4 pa[kGatherAhead], pb[kGatherAhead], pc[kGatherAhead], pd[kGatherAhead];
  if (ga.inst_cnt && !big) {
#pragma unroll
    for (uint32_t i = 0; i < kGatherAhead; ++i)            // past the end: the last record again (a cache hit), unused
      load_record(ga.inst_base + min(i, ga.inst_cnt - 1u), pa[i], pb[i], pc[i], pd[i]);
  }
  // inputs of the projection; of the projection itself only the pixel centre is formed before the records are summed -- the
  // rest (and with it ~25 live registers: the backward's intermediates) follows behind the record phase
  float mean[3] = {0.f, 0.f, 0.f}, cu = 0.f, cv = 0.f, culo = 0.f, cvlo = 0.f;
  if (ga.inst_cnt) {
    mean[0] = means3D[3 * gid]; mean[1] = means3D[3 * gid + 1]; mean[2] = means3D[3 * gid + 2];
    if constexpr (COV3D) {
      for (int i = 0; i < 6; ++i) c6[i] = scales[6 * gid + i];
      op = opacities[gid];
    } else if (FRAME && cs.raw_act) {
      // the forward's VTGS_FORWARD_RAW_ACTIVATIONS (kernel-uniform): parameters in, activations here; the Gaussian's rotation
      // is read only when somebody wants its gradient (frame flag 1) -- the covariance s^2 I does not depend on it
      sc[0] = sc[1] = sc[2] = __expf(scales[gid]);
      op = 1.f / (1.f + __expf(-opacities[gid]));
      if constexpr (FRAME) {
        if (fe.flags & 1u) {
          const float4 u = reinterpret_cast<const float4*>(fe.unnorm_rot)[gid];
          const float un = rsqrtf(fmaxf(u.x * u.x + u.y * u.y + u.z * u.z + u.w * u.w, 1e-24f));
          q[0] = u.x * un; q[1] = u.y * un; q[2] = u.z * un; q[3] = u.w * un;
        }
      }
    } else {
      sc[0] = scales[3 * gid]; sc[1] = scales[3 * gid + 1]; sc[2] = scales[3 * gid + 2];
      const float4 q4 = reinterpret_cast<const float4*>(rotations)[gid];
      q[0] = q4.x; q[1] = q4.y; q[2] = q4.z; q[3] = q4.w;
      op = opacities[gid];
    }
    pixel_centre(cam, mean[0], mean[1], mean[2], cu, cv, culo, cvlo);
    if (!big) {
#pragma unroll
      for (uint32_t i = 0; i < kGatherAhead; ++i)
        if (i < ga.inst_cnt) add_record(mo, cb0, cb1, cb2, pa[i], pb[i], pc[i], pd[i], cu, cv, culo, cvlo);
    }
  }
  // (the list's first window goes out here, behind the lanes' own records: requested with them it kept sixteen more registers
  //  alive through the projection -- 144-158 VGPRs, three wavefronts per SIMD instead of four)
  float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = ra, rc = ra, rd = ra;
  int own = 0;
  bool have = (uint32_t)ln < T;
  if (T) {                                                          // wave-uniform
    own = owner_of(have ? (uint32_t)ln : 0u);                       // (every lane takes part in the permutes)
    const uint32_t ob = (uint32_t)__builtin_amdgcn_ds_bpermute(own << 2, (int)ga.inst_base);
    const uint32_t ov = (uint32_t)__builtin_amdgcn_ds_bpermute(own << 2, (int)V);
    if (have) load_record(ob + kGatherAhead + ((uint32_t)ln - ov), ra, rb, rc, rd);
  }
  for (uint32_t j0 = 0; j0 < T; j0 += 64u) {                        // wave-uniform
    {
      // my record of this window, re-centred with ITS owner's centre, parked in row `ln`
      const float ou = __int_as_float(__builtin_amdgcn_ds_bpermute(own << 2, __float_as_int(cu)));
      const float ovv = __int_as_float(__builtin_amdgcn_ds_bpermute(own << 2, __float_as_int(cv)));
      const float oul = __int_as_float(__builtin_amdgcn_ds_bpermute(own << 2, __float_as_int(culo)));
      const float ovl = __int_as_float(__builtin_amdgcn_ds_bpermute(own << 2, __float_as_int(cvlo)));
      SplatMoments one;
      for (int k = 0; k < 9; ++k) one.m[k] = 0.f;
      float o0 = 0.f, o1 = 0.f, o2 = 0.f;
      if (have) add_record(one, o0, o1, o2, ra, rb, rc, rd, ou, ovv, oul, ovl);
      float4* row = reinterpret_cast<float4*>(rows + ln * kRow);
      row[0] = make_float4(one.m[0], one.m[1], one.m[2], one.m[3]);
      row[1] = make_float4(one.m[4], one.m[5], one.m[6], one.m[7]);
      row[2] = make_float4(one.m[8], o0, o1, o2);
    }
    // the next window's records go out before this window's rows are added up
    const uint32_t jn = j0 + 64u + (uint32_t)ln;
    const bool have_n = jn < T;
    if (j0 + 64u < T) {                                             // wave-uniform
      own = owner_of(have_n ? jn : 0u);
      const uint32_t ob = (uint32_t)__builtin_amdgcn_ds_bpermute(own << 2, (int)ga.inst_base);
      const uint32_t ov = (uint32_t)__builtin_amdgcn_ds_bpermute(own << 2, (int)V);
      if (have_n) load_record(ob + kGatherAhead + (jn - ov), ra, rb, rc, rd);
    }
    have = have_n;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");          // the rows are written (one wavefront: LDS runs in order) ...
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // ... and every owner adds its rows of the window, in index order
    const uint32_t r0 = V > j0 ? V - j0 : 0u, r1 = min(V + my_cnt, j0 + 64u);
    for (uint32_t r = r0; r + j0 < r1 && my_cnt; ++r) {
      const float4* row = reinterpret_cast<const float4*>(rows + r * kRow);
      const float4 x0 = row[0], x1 = row[1], x2 = row[2];
      mo.m[0] += x0.x; mo.m[1] += x0.y; mo.m[2] += x0.z; mo.m[3] += x0.w;
      mo.m[4] += x1.x; mo.m[5] += x1.y; mo.m[6] += x1.z; mo.m[7] += x1.w;
      mo.m[8] += x2.x; cb0 += x2.y;
      if constexpr (DUAL && !B1) { cb1 += x2.z; cb2 += x2.w; }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");          // (the next window overwrites the rows)
    __builtin_amdgcn_wave_barrier();
  }
  for (unsigned long long rest = __ballot(big); rest; rest &= rest - 1ull) {     // wave-uniform
    const int src = __builtin_ctzll(rest);
    const uint32_t base = (uint32_t)__builtin_amdgcn_readlane((int)ga.inst_base, src);
    const uint32_t cnt = (uint32_t)__builtin_amdgcn_readlane((int)ga.inst_cnt, src);
    const float u = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cu), src));
    const float v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cv), src));
    const float ulo = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(culo), src));
    const float vlo = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cvlo), src));
    SplatMoments part;
    for (int k = 0; k < 9; ++k) part.m[k] = 0.f;
    float p0 = 0.f, p1 = 0.f, p2 = 0.f;
    for (uint32_t i = (uint32_t)lane_id(); i < cnt; i += 64u) {   // lane-strided partial sums, then a butterfly: fixed order
      float4 a, b, c, d;
      load_record(base + i, a, b, c, d);
      add_record(part, p0, p1, p2, a, b, c, d, u, v, ulo, vlo);
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) part.m[k] = wave_sum(part.m[k]);
    if constexpr (DUAL) { p0 = wave_sum(p0); p1 = wave_sum(p1); p2 = wave_sum(p2); }
    if (lane_id() == src) { mo = part; cb0 = p0; cb1 = p1; cb2 = p2; }
  }
  if (ga.inst_cnt) {
    const float centre4[4] = {cu, cv, culo, cvlo};                                            // (formed above: not computed twice)
    ok = project_splat(cam, mean, sc, q, op, sp, aux, COV3D ? c6 : nullptr, centre4);
  }
  if (ok) {
    if (moments_scaled_by_opacity) {        // the matrix-core backward accumulates u' = o*u
      const float io = 1.f / op;
      for (int k = 0; k < 6; ++k) mo.m[k] *= io;
    }
    splat_backward(cam, sc, q, op, sp, aux, mo, g, COV3D ? g6 : nullptr);
  }
  if constexpr (FRAME) {
    __shared__ float red[4][12];
    float acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0.f;
    if (live) {
      const FramePose P = load_pose(fe.cam_q, fe.cam_t, fe.depth_w2c);
      const int row = fe.idx ? fe.idx[gid] : gid;                              // owned sets: the Gaussian's row in the map
      const float x = fe.means3D_world[3 * row], y = fe.means3D_world[3 * row + 1], z = fe.means3D_world[3 * row + 2];
      float cx, cy, cz, zz;
      pose_apply(P, x, y, z, cx, cy, cz, zz);
      const float dz = cb0 + 2.f * zz * cb2;                                   // colours of the second render: [z, 1, z^2]
      const float g0 = g.mean3D[0] + dz * P.zr[0], g1 = g.mean3D[1] + dz * P.zr[1], g2 = g.mean3D[2] + dz * P.zr[2];
      if (fe.flags & 1u) {
        fe.g_means3D[3 * row] = P.R[0] * g0 + P.R[3] * g1 + P.R[6] * g2;
        fe.g_means3D[3 * row + 1] = P.R[1] * g0 + P.R[4] * g1 + P.R[7] * g2;
        fe.g_means3D[3 * row + 2] = P.R[2] * g0 + P.R[5] * g1 + P.R[8] * g2;
        const float4 u = reinterpret_cast<const float4*>(fe.unnorm_rot)[row];
        const float un = rsqrtf(fmaxf(u.x * u.x + u.y * u.y + u.z * u.z + u.w * u.w, 1e-24f));
        const float r[4] = {u.x * un, u.y * un, u.z * un, u.w * un};
        const float dot = r[0] * g.rot[0] + r[1] * g.rot[1] + r[2] * g.rot[2] + r[3] * g.rot[3];
        reinterpret_cast<float4*>(fe.g_unnorm_rot)[row] = make_float4((g.rot[0] - r[0] * dot) * un, (g.rot[1] - r[1] * dot) * un,
                                                                       (g.rot[2] - r[2] * dot) * un, (g.rot[3] - r[3] * dot) * un);
      }
      if (fe.flags & 4u) {
        // (op, sc[0] = sigmoid(logit), exp(log-scale): the forward's values, loaded or formed above; a Gaussian without
        //  instances never loaded them and has zero gradients)
        fe.g_logit[row] = g.opacity * op * (1.f - op);
        fe.g_log_scales[row] = sc[0] * (g.scale[0] + g.scale[1] + g.scale[2]);
        fe.g_rgb[3 * row] = g.color[0]; fe.g_rgb[3 * row + 1] = g.color[1]; fe.g_rgb[3 * row + 2] = g.color[2];
      }
      if (fe.flags & 2u) {
        acc[0] = g0; acc[1] = g1; acc[2] = g2;
        acc[3] = g0 * x; acc[4] = g0 * y; acc[5] = g0 * z;
        acc[6] = g1 * x; acc[7] = g1 * y; acc[8] = g1 * z;
        acc[9] = g2 * x; acc[10] = g2 * y; acc[11] = g2 * z;
      }
    }
    if (fe.flags & 2u) {                               // fixed-order block reduction, as in prepare_frame_backward_kernel
#pragma unroll
      for (int k = 0; k < 12; ++k) acc[k] = wave_sum(acc[k]);
      const int wv = (int)(threadIdx.x >> 6), l = lane_id();
      if (l == 0)
        for (int k = 0; k < 12; ++k) red[wv][k] = acc[k];
      __syncthreads();
      if (threadIdx.x < 12) fe.pose_partials[(size_t)blk * 12 + threadIdx.x] =
          red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    }
    return;
  }
  if (!live) return;
  // an output nobody asked for is NULL (wave-uniform tests): 68 bytes per Gaussian when all six are wanted, 24 in a
  // tracking iteration of the unfused loops (means3D + the screen-space term)
  if (g_means3D) { for (int i = 0; i < 3; ++i) g_means3D[3 * gid + i] = g.mean3D[i]; }
  if (g_means2D) { for (int i = 0; i < 3; ++i) g_means2D[3 * gid + i] = g.mean2D[i]; }
  if (g_colors) { for (int i = 0; i < 3; ++i) g_colors[3 * gid + i] = g.color[i]; }
  if constexpr (COV3D) {
    if (g_scales) { for (int i = 0; i < 6; ++i) g_scales[6 * gid + i] = g6[i]; }
  } else {
    if (g_scales) { for (int i = 0; i < 3; ++i) g_scales[3 * gid + i] = g.scale[i]; }
    if (g_rotations) reinterpret_cast<float4*>(g_rotations)[gid] = make_float4(g.rot[0], g.rot[1], g.rot[2], g.rot[3]);
  }
  if (g_opacities) g_opacities[gid] = g.opacity;
  if constexpr (DUAL) { if (g_colors_b) { g_colors_b[3 * gid] = cb0; g_colors_b[3 * gid + 1] = cb1; g_colors_b[3 * gid + 2] = cb2; } }
}
template __global__ decltype(gather_splat_grads<false>) gather_splat_grads<false>;
template __global__ decltype(gather_splat_grads<true>) gather_splat_grads<true>;
template __global__ decltype(gather_splat_grads<true, true>) gather_splat_grads<true, true>;
template __global__ decltype(gather_splat_grads<true, true, false, true>) gather_splat_grads<true, true, false, true>;
template __global__ decltype(gather_splat_grads<false, false, true>) gather_splat_grads<false, false, true>;

__global__ __launch_bounds__(256) void mark_visible_kernel(const float* __restrict__ Vp, int n,
                                                           const float* __restrict__ means3D, uint8_t* __restrict__ out) {
  const int gid = (int)(blockIdx.x * 256u + threadIdx.x);
  if (gid >= n) return;
  const float x = means3D[3 * gid], y = means3D[3 * gid + 1], z = means3D[3 * gid + 2];
  const float tz = fmaf(Vp[2], x, fmaf(Vp[6], y, fmaf(Vp[10], z, Vp[14])));
  out[gid] = tz > kNearCull ? 1 : 0;
}

}  // namespace vtgs
