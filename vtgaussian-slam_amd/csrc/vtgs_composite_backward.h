// vtgs_composite_backward.h -- the matrix-core backward composite, composite_backward_mx<WAVES, DUAL, PXL, B1> (gfx950, wave64).
//
// One template, two owners: vtgs_composite_backward.hip instantiates the lane = pixel forms (PXL) that libvtgs.so ships,
// vtgs_xcheck_composites.hip the quad forms (!PXL) that the tests cross-check them against.  Both replays write the same LDS
// images and share the contraction, so both live in the one kernel body and `if constexpr` selects between them.
//
// Work decomposition: ONE WAVEFRONT = ONE 8x8 PIXEL TILE; a workgroup is four independent wavefronts (the 2x2 tiles
// of one 16x16 block, XCD-swizzled so neighbours gather the same splats from the same L2).
//
// Semantics per pixel of the forward that is replayed: skip power>0; alpha=min(.99,o*exp(power));
// skip alpha<1/255; stop before adding when T(1-alpha)<1e-4; C+=c*alpha*T; D+=z*alpha*T; out=C+T*bg.  exp is v_exp_f32
// (exp2) of a pre-scaled quadratic form.
//
// Backward (Appendix A4, restated front-to-back): with g = dL/dcolor at the pixel, Cg = g.(out - T_final*bg)
// and the running prefix P_k = sum_{j<=k} (g.c_j) alpha_j T_j,
//     dL/dalpha_k = T_k (g.c_k) - (Cg - P_k + T_final (g.bg)) / (1 - alpha_k)
// so the list is replayed in the SAME order as the forward (identical skip/stop decisions by construction,
// no per-pixel contributor count to store) and the per-pixel state is two scalars (T, P).  Per splat the nine
// sums over the tile's 64 pixels are formed by an f32 MFMA contraction and stored as one 40-byte record per
// (splat, tile) instance (56 bytes in the dual render) -- plain stores, no float atomics, bitwise reproducible.
// gather_splat_grads (vtgs_gather.hip) then re-centres and sums each splat's contiguous run of records and runs
// splat_backward (vtgs_math.h).
#pragma once
#include "vtgs_internal.h"
#include "vtgs_composite_common.h"
#include "vtgs_kernels.h"

// Scheduling groups (profiles/r2_issue_rates.md 2: an MFMA and a vector instruction that alternate one by one cost 1.5x the
// sum of their parts).  Measured on the headline scene: backward sweeps + contraction grouped 190.6 us against 197.8 us
// ungrouped.  VTGS_PX_GROUP: the sweeps of px_backward_batch; VTGS_PX_GROUP2: the contraction.
#ifndef VTGS_PX_GROUP
#define VTGS_PX_GROUP 1
#endif
#ifndef VTGS_PX_GROUP2
#define VTGS_PX_GROUP2 1
#endif

namespace vtgs {

// ---------------------------------------------------------------------------------------------------
// Quad form (!PXL).  Lane = pixel column j x splat quad q, exponents from six 4-block MFMAs (mx_exponents,
// vtgs_composite_common.h).  Besides the transmittance, the gradient prefix
//     P_k = sum_{i<=k} (g.c_i) alpha_i T_i      is chained across the quad-lanes:  P_in(q) = P_batch + sum_{q'<q} T_in(q') S(q')
// with S the T-free local sum.  Per (pixel, splat) the lane produces u' = alpha_unclamped * dL/dalpha (= o * u of the
// scalar form; the gather kernel divides the six geometric sums by o) and w = alpha*T and writes them into two
// per-wavefront LDS images laid out [pixel quarter][splat][16 pixels + 4 pad].  (The lane = pixel replay, further down,
// fills the same images.)
//
// Both forms: the contraction over the 64 pixels runs on v_mfma_f32_4x4x1_16b_f32: 16 independent 4x4 blocks = 4 splat groups x
// 4 pixel quarters, each accumulating [4 splats] x [4 columns] over its 16 pixels -- one chain per column group
// (Phi0..3 | Phi4,5 | g0..2 [| g3..5]).  f32 MFMAs share the fp32 FMA lanes with the VALU on CDNA (same peak, no
// co-execution: measured by ablation), so what counts is MACs issued: the 16x16x4 form spends
// 32 instructions x 1024 MACs on 9 useful columns of 16, this form 48 x 256 with 9 (12) of 12 (16) useful.  The four
// pixel-quarter partials are summed across the 16-lane rows with v_permlane32_swap / v_permlane16_swap butterflies
// (two values per swap), which leaves lane (column c, splat group sg, row rho) holding the total of splat 4 sg + rho.
// ---------------------------------------------------------------------------------------------------
constexpr int kImgRow = 20;                 // floats per (splat, pixel quarter) row: 16 pixels + 4 pad (bank spread)
constexpr int kImgQuarter = 16 * kImgRow;   // 320 floats = 5 x 64 banks: the quarter does not move the bank
constexpr int kImgFloats = 4 * kImgQuarter; // one image (u' or w) per wavefront
constexpr int kPhiQuarter = 8 * kImgRow;    // Phi table [pixel quarter][8 columns][16 + 4 pad], shared by the workgroup

__device__ __forceinline__ float swap32_add(float a, float b) {    // rows (a0+a2, a1+a3, b0+b2, b1+b3)
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float swap16_add(float a, float b) {    // rows (a0+a1, b0+b1, a2+a3, b2+b3)
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// sum over the four 16-lane rows of the four registers of one chain: row rho of the result = total of register rho
__device__ __forceinline__ float quarter_sum(const f32x4& p) {
  return swap16_add(swap32_add(p[0], p[2]), swap32_add(p[1], p[3]));
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

// Per-pixel state; the two components of every f32x2 are the pixel blocks 2h and 2h+1 of half-pass h, so the
// element-wise arithmetic below compiles to packed v_pk_{mul,add,fma}_f32 (two pixels per instruction).
template <int NG>
struct MxBwdState {
  f32x2 Tb[2], Pb[2];      // transmittance / gradient prefix of pixel (blk, j) at the start of the batch (replicated over q)
  f32x2 CB[2];             // g.(out - T_final bg) + T_final (g.bg)
  float gown[NG];          // dL/dcolor of the lane's OWN pixel (lane L <-> pixel L): B operand of the g.c products
};

// g.c for 64 pixels x 16 splats: a rank-3 (dual: rank-6) bilinear form, so it comes out of the matrix cores in the
// same layout as the exponents (A = the lanes' own splat colours, B = the lanes' own pixel gradients).
template <int B, bool DUAL>
__device__ __forceinline__ f32x16 mx_gdotc(const MxSplat& m, const float (&g)[DUAL ? 6 : 3]) {
  f32x16 d = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  d = __builtin_amdgcn_mfma_f32_16x16x1f32(m.pay.x, g[0], d, 2, B, 0);
  d = __builtin_amdgcn_mfma_f32_16x16x1f32(m.pay.y, g[1], d, 2, B, 0);
  d = __builtin_amdgcn_mfma_f32_16x16x1f32(m.pay.z, g[2], d, 2, B, 0);
  if constexpr (DUAL) {
    d = __builtin_amdgcn_mfma_f32_16x16x1f32(m.pay.w, g[3], d, 2, B, 0);
    d = __builtin_amdgcn_mfma_f32_16x16x1f32(m.pay2.x, g[4], d, 2, B, 0);
    d = __builtin_amdgcn_mfma_f32_16x16x1f32(m.pay2.y, g[5], d, 2, B, 0);
  }
  return d;
}

template <int B, bool DUAL>
__device__ __forceinline__ void mx_backward_batch(MxBwdState<DUAL ? 6 : 3>& st, const MxSplat& m, const float (&Phi)[6],
                                                  float4* __restrict__ lds_xch, float* __restrict__ Us,
                                                  float* __restrict__ Ws, int l) {
  const int j = l & 15, q = l >> 4;
  const f32x16 d = mx_exponents<B>(m.K, Phi);
  const f32x16 gcv = mx_gdotc<B, DUAL>(m, st.gown);
  const f32x2 one = {1.f, 1.f};
  // two half-passes over the pixel groups {0,1} and {2,3}: halves the number of live per-pair values.
  // Everything that does not depend on the incoming transmittance / prefix is folded before the quad-lane exchange:
  //   u' = Gm (t gc - (CB - P) / (1 - a)),  t = Tin pl[r-1]   ==>   u' = Tin gt - (CB - P) gr,   w = Tin wl
  //   with gt = Gm pl[r-1] gc,  gr = Gm / (1 - a),  wl = a pl[r-1]   (pl[-1] = 1)
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    f32x2 gt[4], gr[4], wl[4], pl[4], S[4];
    const bool alive0 = st.Tb[h].x > 0.f, alive1 = st.Tb[h].y > 0.f;     // pixel not finished at the start of the batch
    {
      f32x2 Gm[4], a[4], gc[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float Gp0 = __builtin_amdgcn_exp2f(d[8 * h + r]), Gp1 = __builtin_amdgcn_exp2f(d[8 * h + 4 + r]);
        const float al0 = fminf(kAlphaMax, Gp0), al1 = fminf(kAlphaMax, Gp1);
        const bool v0 = al0 >= kAlphaMin, v1 = al1 >= kAlphaMin;
        a[r].x = v0 ? al0 : 0.f; a[r].y = v1 ? al1 : 0.f;
        Gm[r].x = (v0 && alive0) ? Gp0 : 0.f;                  // alpha_unclamped where this pair can contribute, else 0
        Gm[r].y = (v1 && alive1) ? Gp1 : 0.f;                  // (the 0.99 clamp passes the gradient through)
        gc[r].x = gcv[8 * h + r]; gc[r].y = gcv[8 * h + 4 + r];
      }
      const f32x2 om1 = one - a[1], om2 = one - a[2], om3 = one - a[3];
      pl[0] = one - a[0];
      pl[1] = pl[0] * om1;
      pl[2] = pl[1] * om2;
      pl[3] = pl[2] * om3;
      // 1 / (1 - a_r) for the four splats from ONE reciprocal of their product (v_rcp_f32 is quarter rate):
      //   1/pl3 -> 1/om3 = pl2/pl3,  1/pl2 = om3/pl3 -> 1/om2 = pl1/pl2, ...      (om >= 0.01, so pl3 >= 1e-8)
      const f32x2 i3 = {__builtin_amdgcn_rcpf(pl[3].x), __builtin_amdgcn_rcpf(pl[3].y)};
      const f32x2 i2 = i3 * om3, i1 = i2 * om2;
      gr[0] = Gm[0] * (i1 * om1); gr[1] = Gm[1] * (pl[0] * i1); gr[2] = Gm[2] * (pl[1] * i2); gr[3] = Gm[3] * (pl[2] * i3);
      const f32x2 tg1 = pl[0] * gc[1], tg2 = pl[1] * gc[2], tg3 = pl[2] * gc[3];
      S[0] = gc[0] * a[0];
      S[1] = __builtin_elementwise_fma(tg1, a[1], S[0]);
      S[2] = __builtin_elementwise_fma(tg2, a[2], S[1]);
      S[3] = __builtin_elementwise_fma(tg3, a[3], S[2]);
      wl[0] = a[0]; wl[1] = a[1] * pl[0]; wl[2] = a[2] * pl[1]; wl[3] = a[3] * pl[2];
      gt[0] = Gm[0] * gc[0]; gt[1] = Gm[1] * tg1; gt[2] = Gm[2] * tg2; gt[3] = Gm[3] * tg3;
    }
    // exchange (local product, local T-free prefix sum) of both pixel groups among the four quad-lanes of a pixel
    float4* xch = lds_xch + 64 * h;
    xch[l] = make_float4(pl[3].x, pl[3].y, S[3].x, S[3].y);
    const float4 x0 = xch[j], x1 = xch[16 + j], x2 = xch[32 + j], x3 = xch[48 + j];
    const f32x2 P0 = {x0.x, x0.y}, P1 = {x1.x, x1.y}, P2 = {x2.x, x2.y}, P3 = {x3.x, x3.y};
    const f32x2 S0 = {x0.z, x0.w}, S1 = {x1.z, x1.w}, S2 = {x2.z, x2.w}, S3 = {x3.z, x3.w};
    const f32x2 T0 = st.Tb[h];
    const f32x2 T1 = T0 * P0, T2 = T1 * P1, T3 = T2 * P2;
    const f32x2 Q0 = st.Pb[h];
    const f32x2 Q1 = __builtin_elementwise_fma(T0, S0, Q0), Q2 = __builtin_elementwise_fma(T1, S1, Q1),
                Q3 = __builtin_elementwise_fma(T2, S2, Q2);
    const f32x2 Tin = (q == 0) ? T0 : (q == 1) ? T1 : (q == 2) ? T2 : T3;
    const f32x2 Pin = (q == 0) ? Q0 : (q == 1) ? Q1 : (q == 2) ? Q2 : Q3;
    const f32x2 Tend = T3 * P3;
    const f32x2 Pend = __builtin_elementwise_fma(T3, S3, Q3);
    const bool cross = (alive0 && Tend.x < kTStop) || (alive1 && Tend.y < kTStop);
    bool stopped0 = false, stopped1 = false;
    if (__ballot(cross) != 0ull) {                              // wave-uniform; rarely true
      // exact stop rule: the first (quad, splat) in list order with T*(1-alpha) < 1e-4 ends the pixel before adding;
      // everything from there on (this quad and the quads behind it) contributes nothing
      const unsigned long long lower_q = 0x0001000100010001ull & ((q == 0) ? 0ull : ((1ull << (16 * q)) - 1ull));
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const float tin = i ? Tin.y : Tin.x;
        const bool was_alive = i ? alive1 : alive0;
        bool livep = true, any = false;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float wr = i ? wl[r].y : wl[r].x, plr = i ? pl[r].y : pl[r].x;     // wl > 0  <=>  alpha >= 1/255
          const bool stop = wr > 0.f && tin * plr < kTStop;
          any = any || (livep && stop);
          livep = livep && !stop;
          if (!livep) { if (i) { gt[r].y = 0.f; gr[r].y = 0.f; wl[r].y = 0.f; } else { gt[r].x = 0.f; gr[r].x = 0.f; wl[r].x = 0.f; } }
        }
        const unsigned long long bal = __ballot(any && was_alive) >> j;
        const bool pixel_stopped = (bal & 0x0001000100010001ull) != 0ull;
        if (i) stopped1 = pixel_stopped; else stopped0 = pixel_stopped;
        if ((bal & lower_q) != 0ull) {                          // a quad in front of mine already ended the pixel
#pragma unroll
          for (int r = 0; r < 4; ++r) { if (i) { gt[r].y = 0.f; gr[r].y = 0.f; wl[r].y = 0.f; } else { gt[r].x = 0.f; gr[r].x = 0.f; wl[r].x = 0.f; } }
        }
      }
    }
    // no predicates from here: gt = gr = 0 where the pair cannot contribute, wl = 0 for invalid pairs, Tin = 0 for dead pixels
    const f32x2 CB = st.CB[h];
    float* __restrict__ us = Us + (2 * h) * kImgQuarter + (4 * q) * kImgRow + j;   // pixel block = pixel quarter
    float* __restrict__ ws = Ws + (2 * h) * kImgQuarter + (4 * q) * kImgRow + j;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const f32x2 Pr = __builtin_elementwise_fma(Tin, S[r], Pin);      // prefix including this splat
      const f32x2 u = __builtin_elementwise_fma(Pr - CB, gr[r], Tin * gt[r]);
      const f32x2 w = Tin * wl[r];
      us[r * kImgRow] = u.x; us[r * kImgRow + kImgQuarter] = u.y;
      ws[r * kImgRow] = w.x; ws[r * kImgRow + kImgQuarter] = w.y;
    }
    st.Tb[h].x = (alive0 && !stopped0) ? Tend.x : 0.f;
    st.Tb[h].y = (alive1 && !stopped1) ? Tend.y : 0.f;
    st.Pb[h] = Pend;
  }
}

// ---- lane = pixel replay (PX): the backward twin of composite_forward_px -------------------------------------------------
// Exponents and g.c for the lane's own pixel x 16 splats from the A-broadcast 16-block MFMA; T and the gradient prefix P
// run inside the lane with the forward's recurrence (w = alpha T, T' = T - w: the stop decisions are the forward's by
// construction); u' and w go to the same LDS images, so the contraction below is shared with the quad form.  A pixel that
// has ended carries T = 0 and CB = P, which makes every later u' and w exactly zero without a mask.
// NG = image-gradient channels: 3 (one render), 6 (dual render) or 4 (dual render whose second image passes a gradient
// through its FIRST channel only -- the [z, 1, z^2] render under get_loss, where the silhouette only feeds comparisons and
// z^2 a detached uncertainty, src/vtgaussian_slam.py:466-521)
template <int G, int NG>
__device__ __forceinline__ f32x4 px_gdotc(const MxSplat& m, const float (&g)[NG]) {
  f32x4 d = {0.f, 0.f, 0.f, 0.f};
  d = __builtin_amdgcn_mfma_f32_4x4x1f32(m.pay.x, g[0], d, 4, G, 0);
  d = __builtin_amdgcn_mfma_f32_4x4x1f32(m.pay.y, g[1], d, 4, G, 0);
  d = __builtin_amdgcn_mfma_f32_4x4x1f32(m.pay.z, g[2], d, 4, G, 0);
  if constexpr (NG >= 4) d = __builtin_amdgcn_mfma_f32_4x4x1f32(m.pay.w, g[3], d, 4, G, 0);
  if constexpr (NG == 6) {
    d = __builtin_amdgcn_mfma_f32_4x4x1f32(m.pay2.x, g[4], d, 4, G, 0);
    d = __builtin_amdgcn_mfma_f32_4x4x1f32(m.pay2.y, g[5], d, 4, G, 0);
  }
  return d;
}

struct PxBwdState { float T, P, CB; bool done; };   // T frozen once the pixel has ended (as in the forward); done: ended / off-image

// One batch of 16 splats for the lane's pixel, in two sweeps so that no per-splat division is needed:
//   front to back:  alpha_k, w_k = alpha_k T_k (-> LDS), T_{k+1} = T_k - w_k, P_k = P_{k-1} + (g.c_k) w_k
//   back to front:  A = colour still behind splat k, seen from behind it = (CB - P_k) / T_{k+1}; anchored ONCE per batch at
//                   its end (for a pixel that has ended: in front of its ending splat, where T is frozen), then
//                   A_{k-1} = A_k + alpha_k (g.c_k - A_k), and
//                   u'_k = alpha_unclamped_k dL/dalpha_k = G_k T_k (g.c_k - A_k)          (the reference's recurrence)
// dL/dalpha_k = T_k g.c_k - (CB - P_k)/(1 - alpha_k) is the same thing since (CB - P_k)/(1 - alpha_k) = T_k A_k.
// `exact` is the forward's switch: straight to the exact sweep while pixels keep ending.
template <int B, int NG, bool CLAMP, bool EXACT_FIRST>
__device__ __forceinline__ void px_backward_batch(PxBwdState& st, bool& exact, const MxSplat& m, const float (&Phi)[6],
                                                  const float (&gown)[NG], float* __restrict__ Us,
                                                  float* __restrict__ Ws, int l) {
  const f32x4 d[4] = {px_exponents<4 * B>(m.K, Phi), px_exponents<4 * B + 1>(m.K, Phi), px_exponents<4 * B + 2>(m.K, Phi),
                      px_exponents<4 * B + 3>(m.K, Phi)};
  const f32x4 gcv[4] = {px_gdotc<4 * B, NG>(m, gown), px_gdotc<4 * B + 1, NG>(m, gown), px_gdotc<4 * B + 2, NG>(m, gown),
                        px_gdotc<4 * B + 3, NG>(m, gown)};
  float* __restrict__ us = Us + (l >> 4) * kImgQuarter + (l & 15);   // image [pixel quarter][splat][16 px]
  float* __restrict__ ws = Ws + (l >> 4) * kImgQuarter + (l & 15);
  float a[16], gT[16];                                         // alpha_k and G_k T_k (0 where the pair contributes nothing)
  float Pn = st.P;
  bool swept = false;
  const bool was_done = st.done;
  if constexpr (!EXACT_FIRST) {
    // front to back, optimistic: no stop test
    float Tn = st.done ? 0.f : st.T;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const float Gp = __builtin_amdgcn_exp2f(d[k >> 2][k & 3]);
      float w;
      if constexpr (CLAMP) {
        const float al = fminf(kAlphaMax, Gp);
        const bool valid = al >= kAlphaMin;
        a[k] = valid ? al : 0.f;
        gT[k] = valid ? Gp * Tn : 0.f;                         // the 0.99 clamp passes the gradient through
        w = a[k] * Tn;
      } else {                                                 // no clamp possible in this chunk: alpha == alpha_unclamped
        a[k] = (Gp >= kAlphaMin) ? Gp : 0.f;
        w = a[k] * Tn;
        gT[k] = w;
      }
      ws[k * kImgRow] = w;
      Pn = fmaf(gcv[k >> 2][k & 3], w, Pn);
      Tn = Tn - w;
    }
#if VTGS_PX_GROUP
    __builtin_amdgcn_sched_group_barrier(0x008, 24 + 4 * NG, 0);
    __builtin_amdgcn_sched_group_barrier(0x302, 400, 0);
#endif
    if (__ballot(!st.done && Tn < kTStop) == 0ull) { st.T = st.done ? st.T : Tn; swept = true; }
    else Pn = st.P;
  }
  if (!swept) {
    // exact sweep: from the ending splat on alpha and G T are zero, so the back sweep passes A through and writes zeros
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const float Gp = __builtin_amdgcn_exp2f(d[k >> 2][k & 3]);
      const float al = CLAMP ? fminf(kAlphaMax, Gp) : Gp;
      const float av = (al >= kAlphaMin) ? al : 0.f;
      const float wk = av * st.T;
      const float tn = st.T - wk;
      const bool stop = tn < kTStop;                           // a live pixel has T >= 1e-4: alpha = 0 cannot trigger it
      const bool live = !st.done && !stop;
      a[k] = live ? av : 0.f;
      gT[k] = live ? ((al >= kAlphaMin) ? Gp * st.T : 0.f) : 0.f;
      const float w = live ? wk : 0.f;
      ws[k * kImgRow] = w;
      Pn = fmaf(gcv[k >> 2][k & 3], w, Pn);
      st.T = live ? tn : st.T;
      st.done = st.done || stop;
    }
    exact = __builtin_popcountll(__ballot(st.done && !was_done)) >= kExactFirstEndings;   // as in the forward
  }
  // anchor: colour behind the batch (behind the ending splat for an ended pixel) per unit of transmittance there; T > 0
  float A = (st.CB - Pn) * __builtin_amdgcn_rcpf(st.T);
  st.P = Pn;
  // back to front
#pragma unroll
  for (int k = 15; k >= 0; --k) {
    const float t = gcv[k >> 2][k & 3] - A;
    us[k * kImgRow] = gT[k] * t;
    A = fmaf(a[k], t, A);
  }
}

// B1 (lane = pixel form of the dual render only): the second image's gradient is zero outside its first channel (CamScalars /
// FrameEpilogue flag 8, promised by the caller -- get_loss, whose loss touches the [z, 1, z^2] render through z alone).  Then
// g.c has four terms, not six; the second set's one colour sum rides in the idle fourth column of chain w (no fourth chain);
// a splat brings one colour of the second set, which leaves the registers for the single render's record prefetch; and a
// record is 12 floats (three aligned float4) instead of 14: 88 matrix instructions per batch instead of 112, 48-byte records.
template <int WAVES, bool DUAL, bool PXL, bool B1>
__global__ __launch_bounds__(64 * WAVES, 3) void composite_backward_mx(
    CamScalars cs, const float* __restrict__ bg, uint32_t nblk,
    const uint32_t* __restrict__ tile_cnt, uint32_t tile_cap, const uint32_t* __restrict__ sorted_gid,
    const uint32_t* __restrict__ sorted_inst, const GeomRec* __restrict__ geom, const float* __restrict__ colors,
    const float* __restrict__ out_color, const float* __restrict__ grad_color, const float* __restrict__ final_T,
    float* __restrict__ grad_inst, const Counters* __restrict__ ctr, const float* __restrict__ colors_b,
    const float* __restrict__ out_color_b, const float* __restrict__ grad_color_b, uint32_t* __restrict__ dbg) {
  static_assert(!B1 || (DUAL && PXL), "B1 is a form of the lane = pixel dual backward");
  constexpr int NG = DUAL ? (B1 ? 4 : 6) : 3;                 // image-gradient channels
  constexpr bool DUAL6 = DUAL && !B1;                         // both colour sets in full
#ifdef VTGS_Q_STAMPS
  const unsigned long long st0 = __builtin_amdgcn_s_memtime();
  const unsigned long long rt0 = __builtin_amdgcn_s_memrealtime();
  unsigned long long st_gather = 0ull, st_batch = 0ull, st_loop0 = 0ull;
  uint32_t nbatches = 0u;
#endif
  constexpr int REC = DUAL ? (B1 ? kGradRecDual1 : kGradRecDual) : kGradRec;   // floats per (splat, tile) record
  __shared__ float4 lds_xch_all[WAVES][PXL ? 1 : 128];
#ifdef VTGS_AB_BWD_PAD                                          // occupancy experiment: extra LDS so that fewer workgroups fit a CU
  __shared__ float ab_pad[VTGS_AB_BWD_PAD];
  if (cs.W < 0) { ab_pad[threadIdx.x] = 1.f; __syncthreads(); if (ab_pad[(threadIdx.x + 1) & 255] == 2.f) return; }
#endif
  __shared__ __attribute__((aligned(16))) float lds_uw[WAVES][2][kImgFloats];
  __shared__ __attribute__((aligned(16))) float lds_phi[4 * kPhiQuarter];
  // the contraction's dL/dcolor operands live in LDS ([wave][second set?][quarter][column][16 + 4]), not in 16 / 32 VGPRs:
  // round 3 -- the registers hold the NEXT chunk's geometry records instead (the gathers were 12 % of the wavefront's life)
  __shared__ __attribute__((aligned(16))) float lds_g_all[WAVES][(DUAL6 ? 2 : 1) * 16 * kImgRow];
  // Everything the wavefront needs before its first batch is requested up front -- flag, list length, image values, first
  // list entries -- and the flag is looked at afterwards: the prologue was four dependent round trips (15 % of the
  // wavefront's life, profiles/r3_stamps.md)
  const uint32_t overflow_flag = ctr->overflow;
  // Phi table for the contraction's B operands: [pixel quarter][column 0..7][pixel 0..15 (+4 pad)], columns 6,7 = 0
  for (int i = (int)threadIdx.x; i < 4 * kPhiQuarter; i += 64 * WAVES) {
    const int pqt = i / kPhiQuarter, c = (i - pqt * kPhiQuarter) / kImgRow, kk = i - pqt * kPhiQuarter - c * kImgRow;
    const int p = 16 * pqt + kk;
    const float PX = (float)(p & 7) - 3.5f, PY = (float)(p >> 3) - 3.5f;
    float v = 0.f;
    v = (c == 0) ? 1.f : v; v = (c == 1) ? PX : v; v = (c == 2) ? PY : v;
    v = (c == 3) ? PX * PX : v; v = (c == 4) ? PX * PY : v; v = (c == 5) ? PY * PY : v;
    lds_phi[i] = (kk < 16) ? v : 0.f;
  }
  const int gx16 = (cs.W + kBinTile - 1) / kBinTile;
  const int gx8 = (cs.W + kSubTile - 1) / kSubTile, gy8 = (cs.H + kSubTile - 1) / kSubTile;
  TileCoord tc = tile_coord<WAVES>(cs, nblk, gx16, gx8, gy8);
  const bool tile_ok = tc.tile_ok;                              // wave-uniform
  if (!tile_ok) { tc.tile = 0; tc.inside = false; }              // (its speculative loads below read tile 0's bin)
  const int l = lane_id();
  const int wv = (WAVES == 1) ? 0 : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  float4* lds_xch = lds_xch_all[wv];
  float* __restrict__ Us = lds_uw[wv][0];
  float* __restrict__ Ws = lds_uw[wv][1];
  const BinRange br = bin_range(cs, (uint32_t)tc.tile, tile_cap);
  const uint32_t s = br.s;
  const uint32_t list_len = min(tile_cnt[tc.tile], br.cap);
  // first list entries (a bin holds at least 64 slots: reading past a short list stays inside the workspace; masked later)
  uint32_t gid_first = sorted_gid[s + (uint32_t)lane_id()], inst_first = sorted_inst[s + (uint32_t)lane_id()];
  const size_t P = (size_t)cs.W * cs.H;
  const int j = l & 15, q = l >> 4;
  const int tx0 = tc.px - (l & 7), ty0 = tc.py - (l >> 3);
  const float cx = (float)tx0 + 3.5f, cy = (float)ty0 + 3.5f;
  const float X = (float)(l & 7) - 3.5f, Y = (float)(l >> 3) - 3.5f;
  const float Phi[6] = {1.f, X, Y, X * X, X * Y, Y * Y};
  const float b0 = bg[0], b1 = bg[1], b2 = bg[2];

  MxBwdState<NG> st;
  PxBwdState ps{1.f, 0.f, 0.f, !tc.inside};
  bool px_exact = false;
  if (PXL && tc.inside) {                                        // lane L <-> pixel L
    const size_t pix = (size_t)tc.py * cs.W + tc.px;
    const float g0 = grad_color[pix], g1 = grad_color[P + pix], g2 = grad_color[2 * P + pix];
    const float Tf = final_T[pix];
    ps.CB = g0 * (out_color[pix] - Tf * b0) + g1 * (out_color[P + pix] - Tf * b1) + g2 * (out_color[2 * P + pix] - Tf * b2)
            + Tf * (g0 * b0 + g1 * b1 + g2 * b2);
    if constexpr (DUAL6) {
      const float g3 = grad_color_b[pix], g4 = grad_color_b[P + pix], g5 = grad_color_b[2 * P + pix];
      ps.CB += g3 * (out_color_b[pix] - Tf * b0) + g4 * (out_color_b[P + pix] - Tf * b1) + g5 * (out_color_b[2 * P + pix] - Tf * b2)
               + Tf * (g3 * b0 + g4 * b1 + g5 * b2);
    } else if constexpr (B1) {
      const float g3 = grad_color_b[pix];
      ps.CB += g3 * (out_color_b[pix] - Tf * b0) + Tf * (g3 * b0);
    }
  }
#pragma unroll
  for (int blk = 0; blk < 4; ++blk) {
    if (PXL) break;
    if constexpr (!B1) {
    const int p = 16 * blk + j;
    const int qx = tx0 + (p & 7), qy = ty0 + (p >> 3);
    const bool in_img = qx < cs.W && qy < cs.H;
    float cb = 0.f;
    if (in_img) {
      const size_t pix = (size_t)qy * cs.W + qx;
      const float g0 = grad_color[pix], g1 = grad_color[P + pix], g2 = grad_color[2 * P + pix];
      const float Tf = final_T[pix];
      cb = g0 * (out_color[pix] - Tf * b0) + g1 * (out_color[P + pix] - Tf * b1) + g2 * (out_color[2 * P + pix] - Tf * b2)
           + Tf * (g0 * b0 + g1 * b1 + g2 * b2);
      if constexpr (DUAL) {
        const float g3 = grad_color_b[pix], g4 = grad_color_b[P + pix], g5 = grad_color_b[2 * P + pix];
        cb += g3 * (out_color_b[pix] - Tf * b0) + g4 * (out_color_b[P + pix] - Tf * b1) + g5 * (out_color_b[2 * P + pix] - Tf * b2)
              + Tf * (g3 * b0 + g4 * b1 + g5 * b2);
      }
    }
    if (blk & 1) { st.Tb[blk >> 1].y = in_img ? 1.f : 0.f; st.CB[blk >> 1].y = cb; st.Pb[blk >> 1].y = 0.f; }
    else         { st.Tb[blk >> 1].x = in_img ? 1.f : 0.f; st.CB[blk >> 1].x = cb; st.Pb[blk >> 1].x = 0.f; }
    }
  }
#pragma unroll
  for (int c = 0; c < NG; ++c) st.gown[c] = 0.f;
  if (tc.inside) {                                              // lane L <-> pixel L (tc.px, tc.py)
    const size_t pix = (size_t)tc.py * cs.W + tc.px;
    st.gown[0] = grad_color[pix]; st.gown[1] = grad_color[P + pix]; st.gown[2] = grad_color[2 * P + pix];
    if constexpr (DUAL) st.gown[3] = grad_color_b[pix];
    if constexpr (DUAL6) { st.gown[4] = grad_color_b[P + pix]; st.gown[5] = grad_color_b[2 * P + pix]; }
  }
  // Contraction roles: l = cj + 4 sg + 16 pq -- column cj of every group, splat group sg, pixel quarter pq.
  // A operand: row (l & 3) of block (sg, pq) = splat 4 sg + (l & 3) = image row (l & 15); B operand: column cj.
  const int cj = l & 3, pq = q;
  // dL/dcolor as the contraction's B operand: row (pq, channel) of set a at [(4 pq + channel) * kImgRow], 16 pixels + pad,
  // channel 3 = 0; dual: set b 320 floats on.  Written from the lanes' OWN pixel gradients (lane L = pixel L = pixel
  // (L & 15) of quarter L >> 4): no second trip to the image.
  float* lds_g = lds_g_all[wv];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    lds_g[(4 * pq + c) * kImgRow + j] = (c < 3) ? st.gown[c < 3 ? c : 0] : (B1 ? st.gown[B1 ? 3 : 0] : 0.f);   // B1: the second set's
    if constexpr (DUAL6) lds_g[16 * kImgRow + (4 * pq + c) * kImgRow + j] = (c < 3) ? st.gown[3 + (c < 3 ? c : 0)] : 0.f;   // one live channel
  }
  __syncthreads();                                            // the Phi table (and, per wavefront, the g image); before any exit
  if (overflow_flag) return;                                  // uniform over the grid: the forward did not complete
  if (!tile_ok || list_len == 0u) return;
  const uint32_t e = s + list_len;
  const float4* __restrict__ Ga4 = reinterpret_cast<const float4*>(lds_g + (4 * pq + cj) * kImgRow);
  const float4* __restrict__ Gb4 = reinterpret_cast<const float4*>(lds_g + 16 * kImgRow + (4 * pq + cj) * kImgRow);
  const float4* Ua4 = reinterpret_cast<const float4*>(Us + pq * kImgQuarter + (l & 15) * kImgRow);   // alias Us / Ws: no restrict
  const float4* Wa4 = reinterpret_cast<const float4*>(Ws + pq * kImgQuarter + (l & 15) * kImgRow);
  const float4* __restrict__ PhiA4 = reinterpret_cast<const float4*>(lds_phi + pq * kPhiQuarter + cj * kImgRow);
  const float4* __restrict__ PhiB4 = reinterpret_cast<const float4*>(lds_phi + pq * kPhiQuarter + (4 + cj) * kImgRow);
  const uint32_t tile_bits = (uint32_t)tc.tile;
  const bool skip_a = PXL && !B1 && (cs.bwd_flags & 1u) != 0u;   // (B1: chain w also carries the second set's column)
  // record columns: chain a -> 0..3, chain b -> 4, 5 (its lanes cj = 2, 3 hold padding and store nothing), chain w -> 6..8
  // and the tile id in 9 (dual: w -> 6..8 + tile id in 12, w2 -> 9..11, its lane cj = 3 stores nothing)
  const int col_b = 4 + cj;
  const bool b_live = cj < 2;
  // B1: chain w -> 6..9 (9 = the second set's first colour), the tile id in 10 from chain b's idle lane cj = 2
  const int col_w = (DUAL6 && cj == 3) ? 12 : 6 + cj;
  const int col_w2 = 9 + cj;

  uint32_t base = s;
#ifdef VTGS_Q_STAMPS
  st_loop0 = __builtin_amdgcn_s_memtime();
#endif
  // Software pipeline of the gather, two deep as in composite_forward_q: while chunk c is composited, the list entries of
  // chunk c + 2 and the geometry records + colours of chunk c + 1 are in flight (a lane past the end reads entry 0 of its bin).
  auto entry = [&](const uint32_t* __restrict__ list, uint32_t b) { const uint32_t p = b + (uint32_t)l; return list[p < e ? p : s]; };
  // the speculative first read went past the end of a short list, into slots nobody wrote: those lanes take entry 0 instead
  // (every id that is gathered through must be a written one -- an unwritten slot holds whatever the memory held before)
  const bool first_in = (uint32_t)l < list_len;
  const uint32_t gid0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)gid_first);    // lane 0 (all lanes active here): entry 0
  const uint32_t inst0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)inst_first);
  uint32_t gid_cur = first_in ? gid_first : gid0;
  uint32_t inst_cur = first_in ? inst_first : inst0;
  uint32_t gid_nxt = entry(sorted_gid, s + 64u), inst_nxt = entry(sorted_inst, s + 64u);
  float4 g0n, g1n;
  float cn[NG];
  auto fetch = [&](uint32_t gid) {
    const float4* gp = reinterpret_cast<const float4*>(geom + gid);
    g0n = gp[0]; g1n = gp[1];
    cn[0] = colors[3 * gid]; cn[1] = colors[3 * gid + 1]; cn[2] = colors[3 * gid + 2];
    if constexpr (DUAL) cn[3] = colors_b[3 * gid];
    if constexpr (DUAL6) { cn[4] = colors_b[3 * gid + 1]; cn[5] = colors_b[3 * gid + 2]; }
  };
  // (dual render: 14 more registers in flight across the batches push the kernel into scratch -- there the records are
  // requested at the top of their own chunk, as in round 2; the entries still come one chunk ahead)
  constexpr bool kRecordsAhead = !DUAL6;
  if constexpr (kRecordsAhead) fetch(gid_cur);
  for (; base < e; base += 64u) {
    const bool alive = PXL ? !ps.done : (st.Tb[0].x > 0.f || st.Tb[0].y > 0.f || st.Tb[1].x > 0.f || st.Tb[1].y > 0.f);
    if (__ballot(alive) == 0ull) break;
    const int n = (int)min(64u, e - base);
#ifdef VTGS_Q_STAMPS
    const unsigned long long sg0 = __builtin_amdgcn_s_memtime();
#endif
    if constexpr (!kRecordsAhead) fetch(gid_cur);
    MxSplat m;                                                  // this chunk's splats, from the records requested one chunk ago
    m.K[0] = -1e30f; m.K[1] = m.K[2] = m.K[3] = m.K[4] = m.K[5] = 0.f;
    m.pay = make_float4(0.f, 0.f, 0.f, 0.f); m.pay2 = make_float2(0.f, 0.f); m.hot = false;
    if (l < n) {
      tile_coefficients(g0n, g1n, cx, cy, m.K);
      m.hot = g1n.y > kClampGuard;
      m.pay = make_float4(cn[0], cn[1], cn[2], DUAL ? cn[DUAL ? 3 : 0] : g1n.z);
      if constexpr (DUAL6) m.pay2 = make_float2(cn[DUAL6 ? 4 : 0], cn[DUAL6 ? 5 : 0]);
    }
    const uint32_t my_inst = (l < n) ? inst_cur : 0u;
    gid_cur = gid_nxt; inst_cur = inst_nxt;
    gid_nxt = entry(sorted_gid, base + 128u); inst_nxt = entry(sorted_inst, base + 128u);
    if constexpr (kRecordsAhead) fetch(gid_cur);                 // next chunk's records: in flight during this chunk's batches
    const bool hot = __ballot(m.hot) != 0ull;                 // wave-uniform: some splat of the chunk may hit the 0.99 clamp
#ifdef VTGS_Q_STAMPS
    asm volatile("" :: "v"(m.K[0]), "v"(m.pay.x));
    __builtin_amdgcn_s_waitcnt(0x0070);                        // vmcnt(0): the chunk's gathers have arrived
    const unsigned long long sg1 = __builtin_amdgcn_s_memtime();
    st_gather += sg1 - sg0;
#endif
    const bool chunk_exact = px_exact;                        // exact sweep first for this chunk (pixels kept ending before it)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      if (16 * b >= n) break;                                 // wave-uniform
      if constexpr (PXL) {
#define VTGS_PX_BWD(CL, EX)                                                                               \
        {                                                                                                 \
          if (b == 0) px_backward_batch<0, NG, CL, EX>(ps, px_exact, m, Phi, st.gown, Us, Ws, l);         \
          if (b == 1) px_backward_batch<1, NG, CL, EX>(ps, px_exact, m, Phi, st.gown, Us, Ws, l);         \
          if (b == 2) px_backward_batch<2, NG, CL, EX>(ps, px_exact, m, Phi, st.gown, Us, Ws, l);         \
          if (b == 3) px_backward_batch<3, NG, CL, EX>(ps, px_exact, m, Phi, st.gown, Us, Ws, l);         \
        }
        if (chunk_exact) VTGS_PX_BWD(true, true)                // (one exact-first body: the clamped form is always valid)
        else             { if (hot) VTGS_PX_BWD(true, false) else VTGS_PX_BWD(false, false) }
#undef VTGS_PX_BWD
      } else {
        if constexpr (!B1) {
          if (b == 0) mx_backward_batch<0, DUAL>(st, m, Phi, lds_xch, Us, Ws, l);
          if (b == 1) mx_backward_batch<1, DUAL>(st, m, Phi, lds_xch, Us, Ws, l);
          if (b == 2) mx_backward_batch<2, DUAL>(st, m, Phi, lds_xch, Us, Ws, l);
          if (b == 3) mx_backward_batch<3, DUAL>(st, m, Phi, lds_xch, Us, Ws, l);
        }
      }
      const int nb = min(16, n - 16 * b);
      f32x4 Pa = {0.f, 0.f, 0.f, 0.f}, Pb = {0.f, 0.f, 0.f, 0.f}, Pw = {0.f, 0.f, 0.f, 0.f}, Pw2 = {0.f, 0.f, 0.f, 0.f};
      // SKIPA (wave-uniform, CamScalars::bwd_flags bit 0): dL/d(first colour set) is wanted by nobody -- a tracking iteration --
      // so chain w (16 of the 48 / 64 contraction MFMAs and its operand reads) is left out; its record columns stay unwritten
      // and the gather kernel does not store what it sums from them
#define VTGS_CONTRACT(SKIPA)                                                                                        \
      {                                                                                                             \
        _Pragma("unroll") for (int t4 = 0; t4 < 4; ++t4) {                                                          \
          const float4 ua = Ua4[t4], wa = Wa4[t4], ba = PhiA4[t4], bb = PhiB4[t4];                                  \
          const float uav[4] = {ua.x, ua.y, ua.z, ua.w}, wav[4] = {wa.x, wa.y, wa.z, wa.w};                         \
          const float bav[4] = {ba.x, ba.y, ba.z, ba.w}, bbv[4] = {bb.x, bb.y, bb.z, bb.w};                         \
          float gav[4] = {0.f, 0.f, 0.f, 0.f}, gbv[4] = {0.f, 0.f, 0.f, 0.f};                                       \
          if constexpr (!(SKIPA)) {                                                                                 \
            const float4 ga = Ga4[t4];                                                                              \
            gav[0] = ga.x; gav[1] = ga.y; gav[2] = ga.z; gav[3] = ga.w;                                             \
          }                                                                                                         \
          if constexpr (DUAL6) {                                                                                    \
            const float4 gb = Gb4[t4];                                                                              \
            gbv[0] = gb.x; gbv[1] = gb.y; gbv[2] = gb.z; gbv[3] = gb.w;                                             \
          }                                                                                                         \
          _Pragma("unroll") for (int e4 = 0; e4 < 4; ++e4) {                                                        \
            Pa = __builtin_amdgcn_mfma_f32_4x4x1f32(uav[e4], bav[e4], Pa, 0, 0, 0);                                 \
            Pb = __builtin_amdgcn_mfma_f32_4x4x1f32(uav[e4], bbv[e4], Pb, 0, 0, 0);                                 \
            if constexpr (!(SKIPA)) Pw = __builtin_amdgcn_mfma_f32_4x4x1f32(wav[e4], gav[e4], Pw, 0, 0, 0);         \
            if constexpr (DUAL6) Pw2 = __builtin_amdgcn_mfma_f32_4x4x1f32(wav[e4], gbv[e4], Pw2, 0, 0, 0);          \
          }                                                                                                         \
        }                                                                                                           \
        if (VTGS_PX_GROUP2) {                                                                                       \
          __builtin_amdgcn_sched_group_barrier(0x100, (DUAL6 ? 24 : 20) - ((SKIPA) ? 4 : 0), 1);  /* the image / Phi / g reads first ... */ \
          __builtin_amdgcn_sched_group_barrier(0x008, (DUAL6 ? 64 : 48) - ((SKIPA) ? 16 : 0), 1); /* ... then the contraction MFMAs back to back */ \
        }                                                                                                           \
      }
      if (skip_a) VTGS_CONTRACT(true) else VTGS_CONTRACT(false)
#undef VTGS_CONTRACT
      // lane (cj, sg, rho = l >> 4) ends up with the totals of splat 4 sg + rho
      const float Fa = quarter_sum(Pa), Fb = quarter_sum(Pb), Fw = skip_a ? 0.f : quarter_sum(Pw);   // (skip_a is wave-uniform)
      const float Fw2 = DUAL6 ? quarter_sum(Pw2) : 0.f;          // cross-lane: must run with all lanes active
      const int srow = (l & 12) + (l >> 4);                     // 4 sg + rho
      const uint32_t inst = (uint32_t)__shfl((int)my_inst, 16 * b + srow, 64);
      if (srow < nb && inst < cs.scratch_records) {
        float* __restrict__ rec = grad_inst + (size_t)inst * REC;
        rec[cj] = Fa;
        if (b_live) rec[col_b] = Fb;
        if constexpr (B1) {
          if (cj == 2) rec[10] = __uint_as_float(tile_bits);
          rec[col_w] = Fw;
        } else {
          rec[col_w] = (cj == 3) ? __uint_as_float(tile_bits) : Fw;
        }
        if constexpr (DUAL6) { if (cj < 3) rec[col_w2] = Fw2; }
      }
#ifdef VTGS_Q_STAMPS
      ++nbatches;
#endif
    }
#ifdef VTGS_Q_STAMPS
    st_batch += __builtin_amdgcn_s_memtime() - sg1;
#endif
  }
  for (; base < e; base += 64u) {
    const int n = (int)min(64u, e - base);
    const uint32_t inst = (l < n) ? sorted_inst[base + (uint32_t)l] : 0xFFFFFFFFu;
    if (l < n && inst < cs.scratch_records) {
      if constexpr (B1) {
        float4* p = reinterpret_cast<float4*>(grad_inst + (size_t)inst * REC);
        p[0] = p[1] = make_float4(0.f, 0.f, 0.f, 0.f);
        p[2] = make_float4(0.f, 0.f, __uint_as_float(tile_bits), 0.f);
      } else if constexpr (DUAL) {
        float2* p = reinterpret_cast<float2*>(grad_inst + (size_t)inst * REC);
        p[0] = p[1] = p[2] = p[3] = p[4] = p[5] = make_float2(0.f, 0.f);
        p[6] = make_float2(__uint_as_float(tile_bits), 0.f);
      } else {
        float2* p = reinterpret_cast<float2*>(grad_inst + (size_t)inst * REC);
        p[0] = p[1] = p[2] = p[3] = make_float2(0.f, 0.f);
        p[4] = make_float2(0.f, __uint_as_float(tile_bits));
      }
    }
  }
#ifdef VTGS_Q_STAMPS
  if (dbg && l == 0) {
    uint32_t* o = dbg + 64 + kStampWords * tc.tile;
    const unsigned long long se = __builtin_amdgcn_s_memtime();
    o[0] = (uint32_t)(st_loop0 - st0); o[1] = 0u; o[2] = (uint32_t)st_gather; o[3] = (uint32_t)st_batch;
    o[4] = (uint32_t)(se - st0); o[5] = nbatches; o[6] = e - s; o[7] = 0u;
    o[8] = (uint32_t)rt0; o[9] = (uint32_t)__builtin_amdgcn_s_memrealtime();
    o[10] = __builtin_amdgcn_s_getreg(4 | (31 << 11)); o[11] = __builtin_amdgcn_s_getreg(20 | (31 << 11));   // HW_ID, XCC_ID
  }
#endif
}

}  // namespace vtgs
