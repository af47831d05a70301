// vtgs_xcheck_composites.hip -- the cross-check composites of the TEST-ONLY libvtgs_xcheck.so (gfx950, wave64).
//
// Nothing in this file ships: libvtgs.so renders with composite_forward_q (vtgs_composite_q.hip) and differentiates with the
// lane = pixel instantiations of composite_backward_mx (vtgs_composite_backward.hip).  The kernels here are independent
// implementations of the same semantics (vtgs_composite_backward.h) that the GPU tests check the product against, launched
// by vtgs_xcheck.hip when an implementation switch asks for one:
//   * scalar forward / backward (VTGS_FWD_IMPL=0 / VTGS_BWD_IMPL=0): lane = pixel, one splat at a time broadcast with
//     v_readlane -- the first correct path of round 1;
//   * quad-form forward (VTGS_FWD_IMPL=1) and the quad-form instantiations of composite_backward_mx (VTGS_BWD_IMPL=1);
//   * lane = pixel forward (VTGS_FWD_IMPL=2), which composite_forward_q is tested against bit for bit.
// (The quadrant-queue backward, VTGS_BWD_IMPL=3, is vtgs_composite_bq.hip.)
// Work decomposition, as in the product: one wavefront = one 8x8 pixel tile; a workgroup is the 2x2 tiles of a 16x16 block.
#include "vtgs_composite_backward.h"

// the scheduling groups of px_backward_batch (vtgs_composite_backward.h) in the lane = pixel FORWARD: they raise its register
// pressure and slow it down, so they stay off
#ifndef VTGS_PX_GROUP_FWD
#define VTGS_PX_GROUP_FWD 0
#endif

namespace vtgs {

// Scalar ("readlane") forward composite: lane = pixel, splats broadcast one at a time (VTGS_FWD_IMPL=0).
__global__ __launch_bounds__(256) void composite_forward(
    CamScalars cs, const float* __restrict__ bg, uint32_t nblk,
    const uint32_t* __restrict__ tile_cnt, uint32_t tile_cap, const uint32_t* __restrict__ sorted_gid,
    const GeomRec* __restrict__ geom, const float* __restrict__ colors,
    float* __restrict__ out_color, float* __restrict__ out_depth, float* __restrict__ final_T,
    const Counters* __restrict__ ctr) {
  if (ctr->overflow) return;                     // bins hold unwritten slots after an overflow
  const int gx16 = (cs.W + kBinTile - 1) / kBinTile;
  const int gx8 = (cs.W + kSubTile - 1) / kSubTile, gy8 = (cs.H + kSubTile - 1) / kSubTile;
  const TileCoord tc = tile_coord<4>(cs, nblk, gx16, gx8, gy8);
  if (!tc.tile_ok) return;                       // wave-uniform
  const int l = lane_id();
  const float pxf = (float)tc.px, pyf = (float)tc.py;
  const BinRange br = bin_range(cs, (uint32_t)tc.tile, tile_cap);
  const uint32_t s = br.s, e = s + min(tile_cnt[tc.tile], br.cap);

  float T = 1.f, C0 = 0.f, C1 = 0.f, C2 = 0.f, D = 0.f;
  bool done = !tc.inside;
  for (uint32_t base = s; base < e; base += 64u) {
    if (__ballot(!done) == 0ull) break;
    const int n = (int)min(64u, e - base);
    const ChunkRec r = gather_chunk(sorted_gid, geom, colors, base + (uint32_t)l, l < n);
    for (int j = 0; j < n; ++j) {
      const float dx = (bcast_f(r.u, j) - pxf) + bcast_f(r.ulo, j), dy = (bcast_f(r.v, j) - pyf) + bcast_f(r.vlo, j);
      const float p2 = dx * (bcast_f(r.qa, j) * dx + bcast_f(r.qb, j) * dy) + bcast_f(r.qc, j) * dy * dy;
      const float alpha = fminf(kAlphaMax, bcast_f(r.op, j) * __builtin_amdgcn_exp2f(p2));
      const float Tn = T * (1.f - alpha);
      bool hit = !done && p2 <= 0.f && alpha >= kAlphaMin;
      if (hit && Tn < kTStop) { done = true; hit = false; }
      if (__ballot(hit) != 0ull) {               // wave-uniform: nobody adds this splat -> skip colour reads
        const float wgt = hit ? alpha * T : 0.f;
        C0 = fmaf(bcast_f(r.c0, j), wgt, C0);
        C1 = fmaf(bcast_f(r.c1, j), wgt, C1);
        C2 = fmaf(bcast_f(r.c2, j), wgt, C2);
        D = fmaf(bcast_f(r.depth, j), wgt, D);
        T = hit ? Tn : T;
      }
    }
  }
  if (tc.inside) {
    const size_t P = (size_t)cs.W * cs.H, pix = (size_t)tc.py * cs.W + tc.px;
    out_color[pix] = C0 + T * bg[0];
    out_color[P + pix] = C1 + T * bg[1];
    out_color[2 * P + pix] = C2 + T * bg[2];
    out_depth[pix] = D;
    final_T[pix] = T;
  }
}

// ---------------------------------------------------------------------------------------------------
// Forward composite, matrix-core quad form ("mx").  Exponents from mx_exponents (vtgs_composite_common.h): lane
// (j = L&15, q = L>>4) holds pixels 16*blk + j x splats 16*b + 4*q + r.
// Each lane therefore owns 4 pixels x 4 splats per batch; the per-splat payload (colour, depth) is read per quad
// from LDS, the transmittance is chained across the four quad-lanes of a pixel with one LDS exchange per batch
// (T_in = T_batch * prod of the earlier quads' local products), colour sums stay per lane and are reduced across
// the quad-lanes once per tile.  The stop rule T(1-alpha) < 1e-4 is evaluated exactly on a wave-uniform slow path
// that is taken only for batches in which some pixel's transmittance actually crosses 1e-4.
// The `power > 0` skip of the scalar form cannot trigger for a positive-definite conic and is not evaluated here
// (the exponent carries ~1e-5 absolute rounding from the expansion; alpha is still clamped to 0.99).
// ---------------------------------------------------------------------------------------------------
template <bool DUAL>
struct MxFwdState {
  float Tb[4];             // transmittance of pixel (blk, j) at the start of the batch; 0 = finished (replicated over q)
  float Tfin[4];           // set by the lane that stopped the pixel: T before the stopping splat
  float C[4][DUAL ? 6 : 4];   // this lane's share of colour (3) + depth sums of pixel (blk, j); dual: 6 colour sums
};

template <int B, bool DUAL>
__device__ __forceinline__ void mx_forward_batch(MxFwdState<DUAL>& st, const float (&K)[6], const float (&Phi)[6],
                                                 const float4* __restrict__ lds_pay, float4* __restrict__ lds_xch,
                                                 int l, const float2* __restrict__ lds_pay2 = nullptr) {
  const int j = l & 15, q = l >> 4;
  const f32x16 d = mx_exponents<B>(K, Phi);
  float4 pay[4];
  float2 pay2[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    pay[r] = lds_pay[16 * B + 4 * q + r];
    if (DUAL) pay2[r] = lds_pay2[16 * B + 4 * q + r];
  }
  const unsigned long long lower_q = 0x0001000100010001ull & ((q == 0) ? 0ull : ((1ull << (16 * q)) - 1ull));
  float2* xch2 = reinterpret_cast<float2*>(lds_xch);
  // two half-passes over the pixel groups {0,1} and {2,3} (keeps the live register set small)
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    float a[2][4], pl[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int blk = 2 * h + i;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float al = fminf(kAlphaMax, __builtin_amdgcn_exp2f(d[4 * blk + r]));
        a[i][r] = (al >= kAlphaMin) ? al : 0.f;
      }
      pl[i][0] = 1.f - a[i][0];
      pl[i][1] = pl[i][0] * (1.f - a[i][1]);
      pl[i][2] = pl[i][1] * (1.f - a[i][2]);
      pl[i][3] = pl[i][2] * (1.f - a[i][3]);
    }
    float2* xch = xch2 + 64 * h;
    xch[l] = make_float2(pl[0][3], pl[1][3]);
    const float2 x0 = xch[j], x1 = xch[16 + j], x2 = xch[32 + j], x3 = xch[48 + j];
    float Tin[2], Tend[2];
    bool cross = false;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int blk = 2 * h + i;
      const float P0 = i ? x0.y : x0.x, P1 = i ? x1.y : x1.x, P2 = i ? x2.y : x2.x, P3 = i ? x3.y : x3.x;
      const float e1 = P0, e2 = e1 * P1, e3 = e2 * P2;
      const float pre = (q == 0) ? 1.f : (q == 1) ? e1 : (q == 2) ? e2 : e3;
      Tin[i] = st.Tb[blk] * pre;
      Tend[i] = st.Tb[blk] * (e3 * P3);
      cross = cross || (st.Tb[blk] > 0.f && Tend[i] < kTStop);
    }
    const bool slow = __ballot(cross) != 0ull;                 // wave-uniform; rarely true
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int blk = 2 * h + i;
      const float t0 = Tin[i], t1 = t0 * pl[i][0], t2 = t0 * pl[i][1], t3 = t0 * pl[i][2];
      const float t[4] = {t0, t1, t2, t3};
      float w[4] = {a[i][0] * t0, a[i][1] * t1, a[i][2] * t2, a[i][3] * t3};
      const bool was_alive = st.Tb[blk] > 0.f;
      bool pixel_stopped = false;
      if (slow) {
        // exact stop rule: the first (quad, splat) in list order with T*(1-alpha) < 1e-4 ends the pixel, before adding
        bool livep = true, any = false;
        float tstop = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool stop = a[i][r] > 0.f && Tin[i] * pl[i][r] < kTStop;
          if (livep && stop) { tstop = t[r]; any = true; }
          livep = livep && !stop;
          w[r] = livep ? w[r] : 0.f;
        }
        const unsigned long long bal = __ballot(any && was_alive) >> j;
        const bool mine = was_alive && (bal & lower_q) == 0ull;    // no quad in front of mine ended the pixel
        pixel_stopped = (bal & 0x0001000100010001ull) != 0ull;
#pragma unroll
        for (int r = 0; r < 4; ++r) w[r] = mine ? w[r] : 0.f;
        if (mine && any) st.Tfin[blk] = tstop;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        st.C[blk][0] = fmaf(w[r], pay[r].x, st.C[blk][0]);
        st.C[blk][1] = fmaf(w[r], pay[r].y, st.C[blk][1]);
        st.C[blk][2] = fmaf(w[r], pay[r].z, st.C[blk][2]);
        st.C[blk][3] = fmaf(w[r], pay[r].w, st.C[blk][3]);
        if constexpr (DUAL) {
          st.C[blk][4] = fmaf(w[r], pay2[r].x, st.C[blk][4]);
          st.C[blk][5] = fmaf(w[r], pay2[r].y, st.C[blk][5]);
        }
      }
      st.Tb[blk] = (was_alive && !pixel_stopped) ? Tend[i] : 0.f;
    }
  }
}

template <int WAVES, bool DUAL>
__global__ __launch_bounds__(64 * WAVES, DUAL ? 3 : 4) void composite_forward_mx(
    CamScalars cs, const float* __restrict__ bg, uint32_t nblk,
    const uint32_t* __restrict__ tile_cnt, uint32_t tile_cap, const uint32_t* __restrict__ sorted_gid,
    const GeomRec* __restrict__ geom, const float* __restrict__ colors,
    float* __restrict__ out_color, float* __restrict__ out_depth, float* __restrict__ final_T,
    const Counters* __restrict__ ctr, const float* __restrict__ colors_b, float* __restrict__ out_color_b) {
  constexpr int NC = DUAL ? 6 : 4;                          // accumulated channels; + 1 row for T_final in the reduction
  __shared__ float4 lds_pay_all[WAVES][64];
  __shared__ float2 lds_pay2_all[DUAL ? WAVES : 1][DUAL ? 64 : 1];
  __shared__ float4 lds_xch_all[WAVES][64];
  __shared__ float lds_red_all[WAVES][(NC + 1) * 64 * 4];   // [value 0..NC][q][pixel 0..63]
  if (ctr->overflow) return;                                // bins hold unwritten slots after an overflow
  const int gx16 = (cs.W + kBinTile - 1) / kBinTile;
  const int gx8 = (cs.W + kSubTile - 1) / kSubTile, gy8 = (cs.H + kSubTile - 1) / kSubTile;
  const TileCoord tc = tile_coord<WAVES>(cs, nblk, gx16, gx8, gy8);   // lane L <-> pixel L of the tile (x = L&7, y = L>>3)
  if (!tc.tile_ok) return;
  const int l = lane_id();
  const int wv = (WAVES == 1) ? 0 : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  float4* lds_pay = lds_pay_all[wv];
  float2* lds_pay2 = lds_pay2_all[DUAL ? wv : 0];
  float4* lds_xch = lds_xch_all[wv];
  float* lds_red = lds_red_all[wv];
  const int j = l & 15, q = l >> 4;
  const int tx0 = tc.px - (l & 7), ty0 = tc.py - (l >> 3);
  const float cx = (float)tx0 + 3.5f, cy = (float)ty0 + 3.5f;
  const float X = (float)(l & 7) - 3.5f, Y = (float)(l >> 3) - 3.5f;
  const float Phi[6] = {1.f, X, Y, X * X, X * Y, Y * Y};
  const BinRange br = bin_range(cs, (uint32_t)tc.tile, tile_cap);
  const uint32_t s = br.s, e = s + min(tile_cnt[tc.tile], br.cap);

  MxFwdState<DUAL> st;
#pragma unroll
  for (int blk = 0; blk < 4; ++blk) {
    const int p = 16 * blk + j;                               // pixel (blk, j) of the tile
    const bool in_img = (tx0 + (p & 7)) < cs.W && (ty0 + (p >> 3)) < cs.H;
    st.Tb[blk] = in_img ? 1.f : 0.f;
    st.Tfin[blk] = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) st.C[blk][c] = 0.f;
  }
  for (uint32_t base = s; base < e; base += 64u) {
    const bool alive = st.Tb[0] > 0.f || st.Tb[1] > 0.f || st.Tb[2] > 0.f || st.Tb[3] > 0.f;
    if (__ballot(alive) == 0ull) break;
    const int n = (int)min(64u, e - base);
    const MxSplat m = mx_gather<DUAL>(sorted_gid, geom, colors, base + (uint32_t)l, l < n, cx, cy, colors_b);
    lds_pay[l] = m.pay;
    if (DUAL) lds_pay2[l] = m.pay2;
    mx_forward_batch<0, DUAL>(st, m.K, Phi, lds_pay, lds_xch, l, lds_pay2);
    if (n > 16) mx_forward_batch<1, DUAL>(st, m.K, Phi, lds_pay, lds_xch, l, lds_pay2);
    if (n > 32) mx_forward_batch<2, DUAL>(st, m.K, Phi, lds_pay, lds_xch, l, lds_pay2);
    if (n > 48) mx_forward_batch<3, DUAL>(st, m.K, Phi, lds_pay, lds_xch, l, lds_pay2);
  }
  // reduce the four quad-lanes of every pixel: lane L outputs pixel L = (blk = L>>4, j = L&15)
#pragma unroll
  for (int blk = 0; blk < 4; ++blk) {
    const int p = 16 * blk + j;
#pragma unroll
    for (int c = 0; c < NC; ++c) lds_red[(c * 4 + q) * 64 + p] = st.C[blk][c];
    lds_red[(NC * 4 + q) * 64 + p] = st.Tfin[blk];
  }
  float out[NC + 1];
#pragma unroll
  for (int c = 0; c < NC + 1; ++c)
    out[c] = lds_red[(c * 4 + 0) * 64 + l] + lds_red[(c * 4 + 1) * 64 + l] + lds_red[(c * 4 + 2) * 64 + l] + lds_red[(c * 4 + 3) * 64 + l];
  const float Tb_mine = (q == 0) ? st.Tb[0] : (q == 1) ? st.Tb[1] : (q == 2) ? st.Tb[2] : st.Tb[3];   // pixel L has blk == q
  const float T = (Tb_mine > 0.f) ? Tb_mine : out[NC];
  if (tc.inside) {
    const size_t P = (size_t)cs.W * cs.H, pix = (size_t)tc.py * cs.W + tc.px;
    out_color[pix] = out[0] + T * bg[0];
    out_color[P + pix] = out[1] + T * bg[1];
    out_color[2 * P + pix] = out[2] + T * bg[2];
    if constexpr (DUAL) {
      out_color_b[pix] = out[3] + T * bg[0];
      out_color_b[P + pix] = out[4] + T * bg[1];
      out_color_b[2 * P + pix] = out[5] + T * bg[2];
    } else {
      out_depth[pix] = out[3];
    }
    final_T[pix] = T;
  }
}
template __global__ decltype(composite_forward_mx<4, false>) composite_forward_mx<4, false>;
template __global__ decltype(composite_forward_mx<4, true>) composite_forward_mx<4, true>;

// ---------------------------------------------------------------------------------------------------
// Forward composite, lane = pixel ("px").  Same bilinear exponent, but from v_mfma_f32_4x4x1_16b_f32 with the A operand
// broadcast (cbsz = 4, abid = g): all 16 blocks multiply the four splats held by lanes 4g..4g+3 with their own four
// pixels, so lane L receives the exponents of splats 4g..4g+3 at ITS pixel L -- four MFMAs per rank-1 term give a lane
// one pixel x 16 splats (same MAC count as the 4-block form above, layout checked by tests/micro/mfma_layout.hip).
// The transmittance chain then runs inside the lane: no quad exchange, no per-lane selects, no reduction at the end;
// the per-splat payload is an LDS broadcast read.  A batch of 16 is first composited without the stop test; only if
// some pixel of the wavefront ends inside it (T(1 - alpha) < 1e-4) is the batch redone with the exact per-splat rule
// (wave-uniform branch, rare).  Per pixel this is the scalar kernel's recurrence: w = alpha T, C += w c, T' = T - w.
// ---------------------------------------------------------------------------------------------------
// State of a pixel: T = transmittance in front of the next splat, FROZEN once the pixel has ended (then it is the value
// the reference reports as final T: the transmittance in front of the ending splat); `done` marks ended / off-image pixels.
// `exact` (wave-uniform): after a batch in which several pixels ended, the next batch goes straight to the exact sweep, and
// keeps doing so while pixels keep ending -- in saturating scenes they end batch after batch, and optimistic-then-redo
// would cost more; where endings are sparse the optimistic sweep stays the first choice.
template <int B, bool DUAL, bool CLAMP, bool EXACT_FIRST>
__device__ __forceinline__ void px_forward_batch(float& T, bool& done, bool& exact, float (&C)[DUAL ? 6 : 4],
                                                 const float (&K)[6], const float (&Phi)[6],
                                                 const float4* __restrict__ lds_pay, const float2* __restrict__ lds_pay2) {
  constexpr int NC = DUAL ? 6 : 4;
  const f32x4 d[4] = {px_exponents<4 * B>(K, Phi), px_exponents<4 * B + 1>(K, Phi), px_exponents<4 * B + 2>(K, Phi),
                      px_exponents<4 * B + 3>(K, Phi)};
  auto alpha = [&](int k) {
    const float g = __builtin_amdgcn_exp2f(d[k >> 2][k & 3]);
    const float al = CLAMP ? fminf(kAlphaMax, g) : g;           // CLAMP == false: no splat of the chunk can reach 0.99
    return (al >= kAlphaMin) ? al : 0.f;
  };
  if constexpr (!EXACT_FIRST) {
    // optimistic sweep: no stop test
    float Tn = done ? 0.f : T, Cn[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) Cn[c] = C[c];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const float ak = alpha(k);
      const float4 py = lds_pay[16 * B + k];                     // same address in every lane: LDS broadcast
      const float w = ak * Tn;
      Cn[0] = fmaf(w, py.x, Cn[0]); Cn[1] = fmaf(w, py.y, Cn[1]); Cn[2] = fmaf(w, py.z, Cn[2]); Cn[3] = fmaf(w, py.w, Cn[3]);
      if constexpr (DUAL) {
        const float2 p2 = lds_pay2[16 * B + k];
        Cn[4] = fmaf(w, p2.x, Cn[4]); Cn[5] = fmaf(w, p2.y, Cn[5]);
      }
      Tn = Tn - w;                                               // T (1 - alpha), with the product already at hand
    }
#if VTGS_PX_GROUP_FWD
    // keep the 24 exponent MFMAs together, ahead of the vector sweep (tests/micro/mix_rate.hip: MFMA and vector
    // instructions alternating one by one cost 1.5x the sum of their separate issue times)
    __builtin_amdgcn_sched_group_barrier(0x008, 24, 0);
    __builtin_amdgcn_sched_group_barrier(0x102, 400, 0);
#endif
    if (__ballot(!done && Tn < kTStop) == 0ull) {                // nobody ends inside this batch
      T = done ? T : Tn;
#pragma unroll
      for (int c = 0; c < NC; ++c) C[c] = Cn[c];
      return;
    }
  }
  // exact sweep: the first splat with T (1 - alpha) < 1e-4 ends the pixel BEFORE it is added.  A live pixel has
  // T >= 1e-4, so an invalid pair (alpha = 0) can never trigger the test.
  const bool was_done = done;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const float ak = alpha(k);
    const float wk = ak * T;
    const float tn = T - wk;                                     // the same expression as in the optimistic sweep
    const bool stop = tn < kTStop;
    const bool live = !done && !stop;
    const float4 py = lds_pay[16 * B + k];
    const float w = live ? wk : 0.f;
    C[0] = fmaf(w, py.x, C[0]); C[1] = fmaf(w, py.y, C[1]); C[2] = fmaf(w, py.z, C[2]); C[3] = fmaf(w, py.w, C[3]);
    if constexpr (DUAL) {
      const float2 p2 = lds_pay2[16 * B + k];
      C[4] = fmaf(w, p2.x, C[4]); C[5] = fmaf(w, p2.y, C[5]);
    }
    T = live ? tn : T;
    done = done || stop;
  }
  // several pixels ended in this batch: a saturation front is passing, the next batch will very likely end more
  // (exact-first costs 14 instead of 10 instructions per pair, optimistic + redo 24: worth it above ~30 % odds)
  exact = __builtin_popcountll(__ballot(done && !was_done)) >= kExactFirstEndings;
}

template <int WAVES, bool DUAL>
__global__ __launch_bounds__(64 * WAVES, 3) void composite_forward_px(
    CamScalars cs, const float* __restrict__ bg, uint32_t nblk,
    const uint32_t* __restrict__ tile_cnt, uint32_t tile_cap, const uint32_t* __restrict__ sorted_gid,
    const GeomRec* __restrict__ geom, const float* __restrict__ colors,
    float* __restrict__ out_color, float* __restrict__ out_depth, float* __restrict__ final_T,
    const Counters* __restrict__ ctr, const float* __restrict__ colors_b, float* __restrict__ out_color_b) {
  constexpr int NC = DUAL ? 6 : 4;
  __shared__ float4 lds_pay_all[WAVES][64];
  __shared__ float2 lds_pay2_all[DUAL ? WAVES : 1][DUAL ? 64 : 1];
  if (ctr->overflow) return;                                // bins hold unwritten slots after an overflow
  const int gx16 = (cs.W + kBinTile - 1) / kBinTile;
  const int gx8 = (cs.W + kSubTile - 1) / kSubTile, gy8 = (cs.H + kSubTile - 1) / kSubTile;
  const TileCoord tc = tile_coord<WAVES>(cs, nblk, gx16, gx8, gy8);   // lane L <-> pixel L of the tile (x = L&7, y = L>>3)
  if (!tc.tile_ok) return;
  const int l = lane_id();
  const int wv = (WAVES == 1) ? 0 : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  float4* lds_pay = lds_pay_all[wv];
  float2* lds_pay2 = lds_pay2_all[DUAL ? wv : 0];
  const int tx0 = tc.px - (l & 7), ty0 = tc.py - (l >> 3);
  const float cx = (float)tx0 + 3.5f, cy = (float)ty0 + 3.5f;
  const float X = (float)(l & 7) - 3.5f, Y = (float)(l >> 3) - 3.5f;
  const float Phi[6] = {1.f, X, Y, X * X, X * Y, Y * Y};
  const BinRange br = bin_range(cs, (uint32_t)tc.tile, tile_cap);
  const uint32_t s = br.s, e = s + min(tile_cnt[tc.tile], br.cap);

  float T = 1.f, C[NC];
  bool done = !tc.inside, exact = false;
#pragma unroll
  for (int c = 0; c < NC; ++c) C[c] = 0.f;
  for (uint32_t base = s; base < e; base += 64u) {
    if (__ballot(!done) == 0ull) break;
    const int n = (int)min(64u, e - base);
    const MxSplat m = mx_gather<DUAL>(sorted_gid, geom, colors, base + (uint32_t)l, l < n, cx, cy, colors_b);
    lds_pay[l] = m.pay;
    if (DUAL) lds_pay2[l] = m.pay2;
    // wave-uniform choices per chunk: clamp-free sweeps unless some splat may reach the 0.99 clamp; exact sweep first
    // while pixels keep ending (set by the batches themselves)
    const bool hot = __ballot(m.hot) != 0ull;
#define VTGS_PX_FWD(CL, EX)                                                                           \
    {                                                                                                 \
      px_forward_batch<0, DUAL, CL, EX>(T, done, exact, C, m.K, Phi, lds_pay, lds_pay2);              \
      if (n > 16) px_forward_batch<1, DUAL, CL, EX>(T, done, exact, C, m.K, Phi, lds_pay, lds_pay2);  \
      if (n > 32) px_forward_batch<2, DUAL, CL, EX>(T, done, exact, C, m.K, Phi, lds_pay, lds_pay2);  \
      if (n > 48) px_forward_batch<3, DUAL, CL, EX>(T, done, exact, C, m.K, Phi, lds_pay, lds_pay2);  \
    }
    if (exact) VTGS_PX_FWD(true, true)                        // (one exact-first body: the clamped form is always valid)
    else       { if (hot) VTGS_PX_FWD(true, false) else VTGS_PX_FWD(false, false) }
#undef VTGS_PX_FWD
  }
  const float Tout = T;                                     // running value, or frozen in front of the ending splat
  if (tc.inside) {
    const size_t P = (size_t)cs.W * cs.H, pix = (size_t)tc.py * cs.W + tc.px;
    out_color[pix] = C[0] + Tout * bg[0];
    out_color[P + pix] = C[1] + Tout * bg[1];
    out_color[2 * P + pix] = C[2] + Tout * bg[2];
    if constexpr (DUAL) {
      out_color_b[pix] = C[3] + Tout * bg[0];
      out_color_b[P + pix] = C[4] + Tout * bg[1];
      out_color_b[2 * P + pix] = C[5] + Tout * bg[2];
    } else {
      out_depth[pix] = C[3];
    }
    final_T[pix] = Tout;
  }
}
template __global__ decltype(composite_forward_px<4, false>) composite_forward_px<4, false>;
template __global__ decltype(composite_forward_px<4, true>) composite_forward_px<4, true>;

// ---------------------------------------------------------------------------------------------------
// Backward composite.  Pixel-major replay produces, per (splat k, pixel p), two scalars:
//     u_kp = G_kp * dL/dalpha_kp      and      w_kp = alpha_kp * T_kp
// and the nine per-splat sums are a contraction over the 64 pixels of the tile:
//     S[k][0..5] = sum_p u_kp * phi_j(p),  phi = (1, X, Y, X^2, XY, Y^2),  X,Y = pixel - tile centre
//     S[k][6..8] = sum_p w_kp * g_ch(p)                                   (g = dL/dcolor)
// i.e. [16 splats x 64 px] x [64 px x 9] per batch of 16 splats -- run on the matrix cores with the exact-f32
// MFMA (v_mfma_f32_16x16x4_f32), which is otherwise idle and issues beside the VALU work of the co-resident
// wavefronts.  The lane<->pixel layout of the replay is transposed into the MFMA A-operand layout
// (lane = splat row i + 16 * k-slot) through a per-wavefront LDS image [16][65] (stride 65: conflict-free for
// both the row-wise ds_write_b32 and the column-wise ds_read_b32).  B (phi | g) lives in 16 VGPRs per lane for the
// whole tile.  The tile-local moments are re-centred on the splat in gather_splat_grads (the record carries the
// tile id), so nothing here depends on the splat position and there is no cross-lane reduction at all.
// ---------------------------------------------------------------------------------------------------
constexpr int kRowStride = 65;

__global__ __launch_bounds__(256) void composite_backward(
    CamScalars cs, const float* __restrict__ bg, uint32_t nblk16,
    const uint32_t* __restrict__ tile_cnt, uint32_t tile_cap, const uint32_t* __restrict__ sorted_gid,
    const uint32_t* __restrict__ sorted_inst, const GeomRec* __restrict__ geom, const float* __restrict__ colors,
    const float* __restrict__ out_color, const float* __restrict__ grad_color, const float* __restrict__ final_T,
    float* __restrict__ grad_inst, const Counters* __restrict__ ctr) {
  __shared__ float lds[4][2][16 * kRowStride];
  if (ctr->overflow) return;
  const int gx16 = (cs.W + kBinTile - 1) / kBinTile;
  const int gx8 = (cs.W + kSubTile - 1) / kSubTile, gy8 = (cs.H + kSubTile - 1) / kSubTile;
  const TileCoord tc = tile_coord<4>(cs, nblk16, gx16, gx8, gy8);
  if (!tc.tile_ok) return;
  const int l = lane_id();
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  float* __restrict__ Us = lds[wv][0];
  float* __restrict__ Ws = lds[wv][1];
  const float pxf = (float)tc.px, pyf = (float)tc.py;
  const BinRange br = bin_range(cs, (uint32_t)tc.tile, tile_cap);
  const uint32_t s = br.s, e = s + min(tile_cnt[tc.tile], br.cap);
  if (s == e) return;
  const size_t P = (size_t)cs.W * cs.H;

  float g0 = 0.f, g1 = 0.f, g2 = 0.f, Cg = 0.f, Bg = 0.f;
  if (tc.inside) {
    const size_t pix = (size_t)tc.py * cs.W + tc.px;
    g0 = grad_color[pix]; g1 = grad_color[P + pix]; g2 = grad_color[2 * P + pix];
    const float Tf = final_T[pix];
    const float b0 = bg[0], b1 = bg[1], b2 = bg[2];
    Cg = g0 * (out_color[pix] - Tf * b0) + g1 * (out_color[P + pix] - Tf * b1) + g2 * (out_color[2 * P + pix] - Tf * b2);
    Bg = Tf * (g0 * b0 + g1 * b1 + g2 * b2);
  }
  // B operand: lane (j = l&15, kk = l>>4), step t  <->  pixel p = 16*kk + t of the tile (p = lane index of the replay)
  const int bj = l & 15, bk = l >> 4;
  const int tx0 = tc.px - (l & 7), ty0 = tc.py - (l >> 3);          // tile origin
  float Bv[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const int p = 16 * bk + t;
    const float X = (float)(p & 7) - 3.5f, Y = (float)(p >> 3) - 3.5f;
    float v = 0.f;
    v = (bj == 0) ? 1.f : v; v = (bj == 1) ? X : v; v = (bj == 2) ? Y : v;
    v = (bj == 3) ? X * X : v; v = (bj == 4) ? X * Y : v; v = (bj == 5) ? Y * Y : v;
    if (bj >= 6 && bj <= 8) {
      const int qx = tx0 + (p & 7), qy = ty0 + (p >> 3);
      if (qx < cs.W && qy < cs.H) v = grad_color[(size_t)(bj - 6) * P + (size_t)qy * cs.W + qx];
    }
    Bv[t] = v;
  }
  const int a_off = bj * kRowStride + 16 * bk;                         // A operand: row = splat bj, k-slot bk
  const uint32_t tile_bits = (uint32_t)tc.tile;

  float T = 1.f, Pfx = 0.f;
  bool done = !tc.inside;
  uint32_t base = s;
  for (; base < e; base += 64u) {
    if (__ballot(!done) == 0ull) break;
    const int n = (int)min(64u, e - base);
    const ChunkRec r = gather_chunk(sorted_gid, geom, colors, base + (uint32_t)l, l < n);
    const uint32_t my_inst = (l < n) ? sorted_inst[base + (uint32_t)l] : 0u;
    for (int jb = 0; jb < n; jb += 16) {
      const int nb = min(16, n - jb);
      for (int jj = 0; jj < nb; ++jj) {
        const int j = jb + jj;
        const float su = bcast_f(r.u, j), sv = bcast_f(r.v, j);
        const float sa = bcast_f(r.qa, j), sb = bcast_f(r.qb, j), sc = bcast_f(r.qc, j);
        const float so = bcast_f(r.op, j);
        const float dx = (su - pxf) + bcast_f(r.ulo, j), dy = (sv - pyf) + bcast_f(r.vlo, j);
        const float p2 = dx * (sa * dx + sb * dy) + sc * dy * dy;
        const float G = __builtin_amdgcn_exp2f(p2);
        const float alpha = fminf(kAlphaMax, so * G);
        const float Tn = T * (1.f - alpha);
        bool hit = !done && p2 <= 0.f && alpha >= kAlphaMin;
        if (hit && Tn < kTStop) { done = true; hit = false; }
        float uu = 0.f, ww = 0.f;
        if (__ballot(hit) != 0ull) {
          const float c0 = bcast_f(r.c0, j), c1 = bcast_f(r.c1, j), c2 = bcast_f(r.c2, j);
          const float gc = g0 * c0 + g1 * c1 + g2 * c2;
          const float wgt = alpha * T;
          const float Pn = fmaf(gc, wgt, Pfx);
          const float dLda = T * gc - (Cg - Pn + Bg) * __builtin_amdgcn_rcpf(1.f - alpha);
          uu = hit ? G * dLda : 0.f;            // clamp at 0.99 passes the gradient through
          ww = hit ? wgt : 0.f;
          Pfx = hit ? Pn : Pfx;
          T = hit ? Tn : T;
        }
        Us[jj * kRowStride + l] = uu;
        Ws[jj * kRowStride + l] = ww;
      }
      // contraction over the 64 pixels on the matrix cores
      f32x4 D1 = {0.f, 0.f, 0.f, 0.f}, D2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        D1 = __builtin_amdgcn_mfma_f32_16x16x4f32(Us[a_off + t], Bv[t], D1, 0, 0, 0);
        D2 = __builtin_amdgcn_mfma_f32_16x16x4f32(Ws[a_off + t], Bv[t], D2, 0, 0, 0);
      }
      // D: col = l&15, row = 4*(l>>4) + reg.  Column j<6 from D1 (u x phi), 6..8 from D2 (w x g), 9 = tile id.
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int row = 4 * bk + rr;
        const uint32_t inst = (uint32_t)__shfl((int)my_inst, jb + row, 64);
        float val = (bj < 6) ? D1[rr] : D2[rr];
        val = (bj == 9) ? __uint_as_float(tile_bits) : val;
        val = (bj > 9) ? 0.f : val;
        if (row < nb && bj < kGradRec) grad_inst[(size_t)inst * kGradRec + bj] = val;
      }
    }
  }
  // every pixel finished before the end of the list: the remaining instances contribute nothing
  for (; base < e; base += 64u) {
    const int n = (int)min(64u, e - base);
    if (l < n) {
      const uint32_t inst = sorted_inst[base + (uint32_t)l];
      float2* p = reinterpret_cast<float2*>(grad_inst + (size_t)inst * kGradRec);
      p[0] = p[1] = p[2] = p[3] = make_float2(0.f, 0.f);
      p[4] = make_float2(0.f, __uint_as_float(tile_bits));
    }
  }
}

template __global__ decltype(composite_backward_mx<4, false, false>) composite_backward_mx<4, false, false>;
template __global__ decltype(composite_backward_mx<4, true, false>) composite_backward_mx<4, true, false>;

}  // namespace vtgs
