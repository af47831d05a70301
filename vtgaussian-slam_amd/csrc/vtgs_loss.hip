// vtgs_loss.hip -- SSIM of the mapping loss as two kernels.
//
// Replaces utils/slam_external.py:66-97 (calc_ssim / _ssim): five grouped 11x11 Gaussian convolutions (sigma 1.5,
// zero padding) + element-wise algebra + mean, and their autograd backward (five more convolutions).  The window is an
// outer product (utils/slam_external.py:60-63), so every blur is separable: a workgroup stages a (32+10)^2 patch of one
// channel in LDS, blurs rows then columns for the five moments, evaluates the SSIM map and reduces it to one partial sum
// (fixed order, no atomics).  When a gradient is wanted it also writes three per-pixel derivative maps
//     A = d/dmu1 - 2 mu1 d/ds11 - mu2 d/ds12,  B = d/ds11,  C = d/ds12     (derivatives of the SSIM map)
// and the backward is   dL/dx = g/(C H W) * ( blur(A) + 2 x blur(B) + y blur(C) )   -- three blurs, same tiling.
#include "../../include/vtgs.h"
#include "vtgs_host.h"
#include "vtgs_internal.h"

namespace vtgs {

constexpr int kST = 32;                 // output tile edge
constexpr int kSR = 5;                  // window radius
constexpr int kSP = kST + 2 * kSR;      // staged patch edge (42)

// The reference's 1-D window (utils/slam_external.py:54-56: float32(exp(-(x - 5)^2 / 4.5)) / their float32 sum), evaluated once
// on the host.  Round 4: every thread of both kernels used to evaluate it itself -- 11 exponentials and 11 IEEE divisions, a
// fifth of the forward kernel's instructions and over a quarter of the backward's.
// (round 5: both SSIM kernels are bound by vector issue -- ~5300 wave-instructions per tile, 4 cycles each on a 16-lane SIMD -- so
//  the blurs accumulate PAIRS of moments with packed v_pk_fma_f32 / v_pk_mul_f32: the same IEEE operations per component, the
//  same bits, 5 instead of 8 instructions per tap in the row pass and 3 instead of 5 in the column pass)
typedef float f32x2s __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void gauss11(float (&w)[11]) {
  constexpr float k[11] = {0.0010283802403137088f, 0.007598758675158024f, 0.036000773310661316f, 0.1093606948852539f,
                           0.21300554275512695f,   0.2660117447376251f,   0.21300554275512695f,  0.1093606948852539f,
                           0.036000773310661316f,  0.007598758675158024f, 0.0010283802403137088f};
#pragma unroll
  for (int i = 0; i < 11; ++i) w[i] = k[i];
}

// ---- what the two SSIM kernels share: which tile, which staged pixels, the blur ------------------------------------------
// tile b of a launch of C x tiles_y x tiles_x tiles whose first tile row is ty0
struct SsimTile { int c, ty, tx; };
__device__ __forceinline__ SsimTile ssim_tile(int b, int tiles_x, int tiles_y, int ty0) {
  const int c = b / (tiles_x * tiles_y), tb = b - c * tiles_x * tiles_y;
  return SsimTile{c, ty0 + tb / tiles_x, tb - (tb / tiles_x) * tiles_x};
}

// The thread's kStage positions in the staged patch of a tile: visit(k, gy, gx, in_patch) with the image row and column of
// position t + 256 k (in_patch: that position exists -- the last slot of most threads does not).
// (the staging was a third of the kernels' vector instructions: a division, 64-bit address arithmetic and a branch per
//  pixel.  Now: the position advances by 256 = 6 x 42 + 4, offsets are 32-bit from a uniform plane pointer, and the caller
//  loads a pixel it does not want from an offset that is always valid and replaces it by zero -- no branch)
constexpr int kStage = (kSP * kSP + 255) / 256;                       // 7 staged pixels per thread and image
template <class Visit>
__device__ __forceinline__ void ssim_stage_walk(const SsimTile& tile, Visit&& visit) {
  const int t = (int)threadIdx.x, x0 = tile.tx * kST - kSR, y0 = tile.ty * kST - kSR;
  int r = t / kSP, q = t - r * kSP;                                   // patch position of the thread's first staged pixel
#pragma unroll
  for (int k = 0; k < kStage; ++k) {
    visit(k, y0 + r, x0 + q, k < kStage - 1 || t + 256 * k < kSP * kSP);
    q += 256 - 6 * kSP; r += 6;
    if (q >= kSP) { q -= kSP; r += 1; }
  }
}

// Output o of the 11-tap blur over a register window: both passes of both kernels slide the window in registers, a work item
// produces FOUR adjacent outputs from 14 staged values instead of 4 x 11 (the kernels were bound by their LDS reads).  Every
// output accumulates its taps in the order 0..10, so the values are the ones of the one-output-per-item form.  T = f32x2s
// blurs a pair with one packed fma per tap.
template <class T>
__device__ __forceinline__ T blur11(const float (&w)[11], const T (&v)[14], int o) {
  T s = (T)0.f;
#pragma unroll
  for (int k = 0; k < 11; ++k) s = __builtin_elementwise_fma((T)w[k], v[o + k], s);
  return s;
}

__global__ __launch_bounds__(256) void ssim_forward_kernel(const float* __restrict__ img1, const float* __restrict__ img2,
                                                           int C, int H, int W, int tiles_x, int tiles_y,
                                                           float* __restrict__ partial, float* __restrict__ gmaps,
                                                           int ty0, int rb, int re) {
  // band form (tile-row multi-GPU partition): tiles_y tile rows starting at ty0 are launched and only the SSIM pixels of
  // rows [rb, re) are summed / get derivative maps; the staged context rows around them are read as they are (the caller
  // has put the neighbours' rows there).  Whole image: ty0 = 0, rb = 0, re = H.
  // pairs that are blurred together sit together in LDS (one ds_read_b64 = one packed operand, no register shuffling)
  __shared__ float2 pxy[kSP * kSP];                                   // (img1, img2)
  __shared__ float2 hzm[kSP * kST], hzs[kSP * kST];                   // row-blurred (x, y), (x^2, y^2)
  __shared__ float hzc[kSP * kST];                                    // row-blurred x y
  __shared__ float red[4];
  float w[11];
  gauss11(w);
  const int t = (int)threadIdx.x;
  // Round 5: a workgroup walks tiles b = blockIdx.x, + gridDim.x, ... (the grid is what fits the chip at once, vtgs_ssim_grid) and
  // requests the NEXT tile's patch into registers before it blurs the current one: a tile used to cost ~8 us of which the blurs
  // were ~3 -- the rest was the wait for its own 2 x 1764 pixels with three workgroups per CU to hide it behind.  Same arithmetic
  // per tile, same partial-sum slot per tile: bit-identical results.
  const int ntile = C * tiles_x * tiles_y;
  float ra[kStage], rd[kStage];
  auto fetch = [&](int bb) {
    const SsimTile tile = ssim_tile(bb, tiles_x, tiles_y, ty0);
    const float* __restrict__ p1 = img1 + (size_t)tile.c * H * W;
    const float* __restrict__ p2 = img2 + (size_t)tile.c * H * W;
    ssim_stage_walk(tile, [&](int k, int gy, int gx, bool in_patch) {
      const bool in = in_patch && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;   // zero padding
      const int o = in ? gy * W + gx : 0;
      const float a1 = p1[o], a2 = p2[o];
      ra[k] = in ? a1 : 0.f;
      rd[k] = in ? a2 : 0.f;
    });
  };
  if ((int)blockIdx.x < ntile) fetch((int)blockIdx.x);
  for (int b = (int)blockIdx.x; b < ntile; b += (int)gridDim.x) {
  const SsimTile tile = ssim_tile(b, tiles_x, tiles_y, ty0);
  const size_t plane = (size_t)tile.c * H * W;
#pragma unroll
  for (int k = 0; k < kStage; ++k) {
    const int i = t + 256 * k;
    if (i < kSP * kSP) pxy[i] = make_float2(ra[k], rd[k]);
  }
  __syncthreads();
  if (b + (int)gridDim.x < ntile) fetch(b + (int)gridDim.x);          // in flight during both passes
  for (int i = t; i < kSP * (kST / 4); i += 256) {                    // rows: 42 x 32 outputs, 4 per item (blur11)
    const int r = i / (kST / 4), q = 4 * (i - r * (kST / 4));
    f32x2s v[14], v2[14];
    float vxy[14];
#pragma unroll
    for (int k = 0; k < 14; ++k) {                                    // squares and the product once per staged pixel, not per tap
      const float2 pp = pxy[r * kSP + q + k];
      v[k] = f32x2s{pp.x, pp.y}; v2[k] = v[k] * v[k]; vxy[k] = pp.x * pp.y;
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const f32x2s m = blur11(w, v, o), sq = blur11(w, v2, o);
      const int j = r * kST + q + o;
      hzm[j] = make_float2(m.x, m.y); hzs[j] = make_float2(sq.x, sq.y); hzc[j] = blur11(w, vxy, o);
    }
  }
  __syncthreads();
  float acc = 0.f;
  const float c1 = 0.01f * 0.01f, c2 = 0.03f * 0.03f;
  {                                                                   // columns: 32 x 32 outputs, 4 rows per item
    const int q = t & (kST - 1), r0 = 4 * (t >> 5);                   // 256 items = 8 row groups x 32 columns
    f32x2s hm_[14], hs_[14];
    float hc_[14];
#pragma unroll
    for (int k = 0; k < 14; ++k) {
      const float2 a2 = hzm[(r0 + k) * kST + q], b2 = hzs[(r0 + k) * kST + q];
      hm_[k] = f32x2s{a2.x, a2.y}; hs_[k] = f32x2s{b2.x, b2.y}; hc_[k] = hzc[(r0 + k) * kST + q];
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const int gy = tile.ty * kST + r0 + o, gx = tile.tx * kST + q;
      const f32x2s mm = blur11(w, hm_, o), sq = blur11(w, hs_, o);
      const float xy = blur11(w, hc_, o);
      const float m1 = mm.x, m2 = mm.y, xx = sq.x, yy = sq.y;
      if (gy < H && gx < W && gy >= rb && gy < re) {
        const float s11 = xx - m1 * m1, s22 = yy - m2 * m2, s12 = xy - m1 * m2;
        const float a1 = 2.f * m1 * m2 + c1, a2 = 2.f * s12 + c2, b1 = m1 * m1 + m2 * m2 + c1, b2 = s11 + s22 + c2;
        // two reciprocals per pixel: hardware estimate + one Newton step (< 1 ulp; the IEEE division was ~10 instructions
        // each in a kernel bound by vector issue).  b1, b2 >= c1, c2 > 0.
        float r1 = __builtin_amdgcn_rcpf(b1), r2 = __builtin_amdgcn_rcpf(b2);
        r1 = fmaf(r1, fmaf(-b1, r1, 1.f), r1); r2 = fmaf(r2, fmaf(-b2, r2, 1.f), r2);
        const float ib = r1 * r2;
        const float ssim = a1 * a2 * ib;
        acc += ssim;
        if (gmaps) {
          const float d_mu1 = 2.f * m2 * a2 * ib - ssim * 2.f * m1 * r1;
          const float d_s11 = -ssim * r2, d_s12 = 2.f * a1 * ib;
          const size_t P3 = (size_t)C * H * W;
          float* __restrict__ gm0 = gmaps + plane;                    // uniform bases, 32-bit offsets
          float* __restrict__ gm1 = gm0 + P3;
          float* __restrict__ gm2 = gm1 + P3;
          const int o2 = gy * W + gx;
          gm0[o2] = d_mu1 - 2.f * m1 * d_s11 - m2 * d_s12;
          gm1[o2] = d_s11;
          gm2[o2] = d_s12;
        }
      }
    }
  }
  acc = wave_sum(acc);
  if ((t & 63) == 0) red[t >> 6] = acc;
  __syncthreads();
  if (t == 0) partial[b] = red[0] + red[1] + red[2] + red[3];
  __syncthreads();                                                    // red / hz / the patch are rewritten by the next tile
  }
}

__global__ __launch_bounds__(256) void ssim_backward_kernel(const float* __restrict__ img1, const float* __restrict__ img2,
                                                            const float* __restrict__ gmaps, const float* __restrict__ upstream,
                                                            int C, int H, int W, int tiles_x, int tiles_y,
                                                            float* __restrict__ g_img1, float ssim_coef, float l1_coef,
                                                            const float* __restrict__ l1_weight, int ty0, int rb, int re) {
  // band form: the derivative maps exist on rows [rb, re) only (anything else counts as zero); the gradient is written on
  // rows [rb - 5, re + 5) -- the blur carries it into the neighbours' rows -- and the L1 term belongs to rows [rb, re).
  __shared__ float2 pm01[kSP * kSP];                                  // maps A, B as a pair (see the forward), C apart
  __shared__ float pm2[kSP * kSP];
  __shared__ float2 hz01[kSP * kST];
  __shared__ float hz2[kSP * kST];
  float w[11];
  gauss11(w);
  const int t = (int)threadIdx.x;
  const size_t P3 = (size_t)C * H * W;
  const int ntile = C * tiles_x * tiles_y;                            // tiles walked with the next one's patch in flight (see the forward)
  float rm[3][kStage];
  const int row_lo = rb > 0 ? rb : 0, row_hi = re < H ? re : H;       // the maps exist on these rows
  auto fetch = [&](int bb) {
    const SsimTile tile = ssim_tile(bb, tiles_x, tiles_y, ty0);
    const float* __restrict__ g0 = gmaps + (size_t)tile.c * H * W;
    const float* __restrict__ g1 = g0 + P3;
    const float* __restrict__ g2 = g1 + P3;
    ssim_stage_walk(tile, [&](int k, int gy, int gx, bool in_patch) {
      const bool in = in_patch && gy >= row_lo && gy < row_hi && (unsigned)gx < (unsigned)W;   // the adjoint of a zero-padded blur is the same blur
      const int o = in ? gy * W + gx : row_lo * W;
      const float a0 = g0[o], a1 = g1[o], a2 = g2[o];
      rm[0][k] = in ? a0 : 0.f; rm[1][k] = in ? a1 : 0.f; rm[2][k] = in ? a2 : 0.f;
    });
  };
  if ((int)blockIdx.x < ntile) fetch((int)blockIdx.x);
  const float scale = upstream[0] * ssim_coef / (float)((size_t)C * H * W);
  const float l1s = upstream[0] * l1_coef;
  for (int b = (int)blockIdx.x; b < ntile; b += (int)gridDim.x) {
  const SsimTile tile = ssim_tile(b, tiles_x, tiles_y, ty0);
  const size_t plane = (size_t)tile.c * H * W;
#pragma unroll
  for (int k = 0; k < kStage; ++k) {
    const int i = t + 256 * k;
    if (i < kSP * kSP) { pm01[i] = make_float2(rm[0][k], rm[1][k]); pm2[i] = rm[2][k]; }
  }
  __syncthreads();
  if (b + (int)gridDim.x < ntile) fetch(b + (int)gridDim.x);
  for (int i = t; i < kSP * (kST / 4); i += 256) {                    // rows, four outputs per item (see the forward)
    const int r = i / (kST / 4), q = 4 * (i - r * (kST / 4));
    f32x2s v01[14];
    float v2_[14];
#pragma unroll
    for (int k = 0; k < 14; ++k) {
      const float2 pp = pm01[r * kSP + q + k];
      v01[k] = f32x2s{pp.x, pp.y}; v2_[k] = pm2[r * kSP + q + k];
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const f32x2s s01 = blur11(w, v01, o);
      const int j = r * kST + q + o;
      hz01[j] = make_float2(s01.x, s01.y); hz2[j] = blur11(w, v2_, o);
    }
  }
  __syncthreads();
  // dL/dimg1 = upstream * ( ssim_coef * d(mean SSIM)/dimg1 + l1_coef * sign(img1 - img2) )   (plain SSIM: 1, 0)
  {                                                                   // columns, four rows per item
    const int q = t & (kST - 1), r0 = 4 * (t >> 5);
    f32x2s h01[14];
    float h2_[14];
#pragma unroll
    for (int k = 0; k < 14; ++k) {
      const float2 pp = hz01[(r0 + k) * kST + q];
      h01[k] = f32x2s{pp.x, pp.y}; h2_[k] = hz2[(r0 + k) * kST + q];
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const int gy = tile.ty * kST + r0 + o, gx = tile.tx * kST + q;
      if (gy >= H || gx >= W || gy < rb - kSR || gy >= re + kSR) continue;
      const f32x2s s01 = blur11(w, h01, o);
      const float s0 = s01.x, s1 = s01.y, s2 = blur11(w, h2_, o);
      // (the tile's own pixels are read here, not with the next tile's patch: eight more registers in flight across the
      //  blurs cost the fourth wavefront per SIMD, 26 -> 29 us)
      const int o2 = gy * W + gx;                                     // uniform bases, 32-bit offsets
      const float x = (img1 + plane)[o2], y = (img2 + plane)[o2];
      const float lw = (gy >= rb && gy < re) ? (l1_weight ? l1s * (l1_weight + plane)[o2] : l1s) : 0.f;
      (g_img1 + plane)[o2] = scale * (s0 + 2.f * x * s1 + y * s2) + ((x > y) ? lw : (x < y) ? -lw : 0.f);
    }
  }
  __syncthreads();                                                    // hz / the patch are rewritten by the next tile
  }
}

// ---- masked L1 terms of get_loss (src/vtgaussian_slam.py:519-608), value and gradient images in one pass -------------
// mode 0 (tracking): mask = gt_depth > 0 & finite depth & finite uncertainty & silhouette > sil_thres;
//                    partial[b] = {sum_mask |gt_im - im| (3 channels), sum_mask |gt_depth - depth|, count}
// mode 1 (mapping):  mask = gt_depth > 0 & finite depth & finite uncertainty;   colour L1 over ALL pixels (it is a mean)
// mode 2 (tracking with neither use_sil_for_loss nor ignore_outlier_depth_loss, src/vtgaussian_slam.py:601-602): the depth
//                    term as in mode 0, the colour SUM over all pixels
// Gradient images hold d(sum)/d(im) and d(sum)/d(depth_sil[0]) (channels 1, 2 of depth_sil only enter detached masks).

// ---- what masked_l1_kernel (the value) and loss_backward_kernel (the gradient) share, so that both mask the same pixels ----
// the depth mask of one pixel; extra: the visibility / far-depth / outlier masks of the other datasets (1 when there is none)
__device__ __forceinline__ bool depth_mask(int mode, float sil_thres, float depth, float sil, float depth_sq, float gt_depth, float extra) {
  const float unc = depth_sq - depth * depth;
  bool m = gt_depth > 0.f && depth == depth && unc == unc;
  if (mode != 1) m = m && sil > sil_thres;
  return m && extra != 0.f;
}
// the colour terms run over the depth mask in mode 0 and over all pixels in modes 1 and 2
__device__ __forceinline__ bool colour_mask(int mode, bool m) { return mode == 0 ? m : true; }
// c * d|e|/dx for e = target - x on the mask, else 0
__device__ __forceinline__ float l1_grad(bool on, float e, float c) { return on ? (e > 0.f ? -c : (e < 0.f ? c : 0.f)) : 0.f; }
// s + |e| w of the colour sum.  Left to the compiler, which of these multiply-adds are fused changes with the code around
// them, and the partial sums with it; so contraction is off and the rounding is spelled out as both forms of the kernel have
// always had it: a pixel's first channel rounds its product before the addition, its other two are fused.
__device__ __forceinline__ float add_weighted_abs(float s, float e, float w, bool fused) {
#pragma clang fp contract(off)
  return fused ? fmaf(fabsf(e), w, s) : s + fabsf(e) * w;
}

// The pixels [p0, p1) of planes of stride P over a grid of 256-thread workgroups: body(PxCount<4>, i) for the groups of four
// in [p0, pv) when `aligned` (every base 16-byte aligned) and P and p0 are multiples of 4, then body(PxCount<1>, i) for
// [pv, p1) one by one.  A thread's sums take its fours first; the body runs the lanes of a four in order.
// (Round 5: a thread of the one-pixel form walked ~3 pixels one after the other with ten scalar loads each -- 12 us for 33 MB;
//  every reference frame size takes the float4 form)
template <int N> struct PxCount { static constexpr int value = N; };
template <class Body>
__device__ __forceinline__ void walk_pixels(int P, int p0, int p1, bool aligned, Body&& body) {
  const bool vec = (P & 3) == 0 && (p0 & 3) == 0 && aligned;
  const int pv = vec ? p0 + ((p1 - p0) & ~3) : p0;
  for (int i = p0 + 4 * (int)(blockIdx.x * 256u + threadIdx.x); i < pv; i += 4 * (int)(gridDim.x * 256u)) body(PxCount<4>{}, i);
  for (int i = pv + (int)(blockIdx.x * 256u + threadIdx.x); i < p1; i += (int)(gridDim.x * 256u)) body(PxCount<1>{}, i);
}

__global__ __launch_bounds__(256) void masked_l1_kernel(const float* __restrict__ im, const float* __restrict__ ds,
                                                        const float* __restrict__ gt_im, const float* __restrict__ gt_depth,
                                                        int P, float sil_thres, int mode, float* __restrict__ partial,
                                                        float* __restrict__ g_im, float* __restrict__ g_ds,
                                                        const float* __restrict__ extra_mask,
                                                        const float* __restrict__ color_weight, int p0, int p1) {
  // [p0, p1): the pixels this call sums (a band of rows of the tile-row partition); P stays the plane stride
  __shared__ float red[4][3];
  float s_im = 0.f, s_d = 0.f, cnt = 0.f;
  // N pixels: the masks, the three sums, and (optionally) the unscaled gradient images
  walk_pixels(P, p0, p1, all_aligned16(im, ds, gt_im, gt_depth, extra_mask, color_weight, g_im, g_ds), [&](auto n, int i) {
    using V = Px<decltype(n)::value>;
    const V depth = V::load(ds + i), sil = V::load(ds + P + i), dsq = V::load(ds + 2 * (size_t)P + i), gd = V::load(gt_depth + i);
    const V em = V::load_or_ones(extra_mask, i);
    V x[3], y[3], cw[3], gds, gim[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      x[c] = V::load(im + (size_t)c * P + i);
      y[c] = V::load(gt_im + (size_t)c * P + i);
      cw[c] = V::load_or_ones(color_weight, (size_t)c * P + i);     // mapping: 10 additional_mask + 0.8
    }
#pragma unroll
    for (int k = 0; k < decltype(n)::value; ++k) {
      const bool m = depth_mask(mode, sil_thres, depth[k], sil[k], dsq[k], gd[k], em[k]), mc = colour_mask(mode, m);
      const float d = gd[k] - depth[k];
      s_d += m ? fabsf(d) : 0.f;
      cnt += m ? 1.f : 0.f;
      gds[k] = l1_grad(m, d, 1.f);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float e = y[c][k] - x[c][k];
        s_im = mc ? add_weighted_abs(s_im, e, cw[c][k], c > 0) : s_im;
        gim[c][k] = l1_grad(mc, e, cw[c][k]);
      }
    }
    if (g_ds) { gds.store(g_ds + i); V::all(0.f).store(g_ds + P + i); V::all(0.f).store(g_ds + 2 * (size_t)P + i); }
    if (g_im) {
#pragma unroll
      for (int c = 0; c < 3; ++c) gim[c].store(g_im + (size_t)c * P + i);
    }
  });
  s_im = wave_sum(s_im); s_d = wave_sum(s_d); cnt = wave_sum(cnt);
  if (lane_id() == 0) { red[threadIdx.x >> 6][0] = s_im; red[threadIdx.x >> 6][1] = s_d; red[threadIdx.x >> 6][2] = cnt; }
  __syncthreads();
  if (threadIdx.x < 3) partial[blockIdx.x * 3 + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}


// ---- silhouette-threshold sweep (src/vtgaussian_slam.py:472-510): masked squared colour error per candidate ----------
struct SweepThresholds { float c[8]; int n; };

__global__ __launch_bounds__(256) void silhouette_sweep_kernel(const float* __restrict__ im, const float* __restrict__ sil,
                                                               const float* __restrict__ gt_im, const float* __restrict__ gt_depth,
                                                               int P, SweepThresholds th, float* __restrict__ partial,
                                                               int p0, int p1) {
  __shared__ float red[4][16];
  float sum[8], cnt[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { sum[k] = 0.f; cnt[k] = 0.f; }
  for (int i = p0 + (int)(blockIdx.x * 256u + threadIdx.x); i < p1; i += (int)(gridDim.x * 256u)) {
    const float e0 = gt_im[i] - im[i], e1 = gt_im[(size_t)P + i] - im[(size_t)P + i],
                e2 = gt_im[2 * (size_t)P + i] - im[2 * (size_t)P + i];
    const float sq = e0 * e0 + e1 * e1 + e2 * e2;
    const float s = sil[i];
    const bool valid = gt_depth[i] > 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const bool m = valid && k < th.n && s > th.c[k];
      sum[k] += m ? sq : 0.f;
      cnt[k] += m ? 1.f : 0.f;
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float a = wave_sum(sum[k]), b = wave_sum(cnt[k]);
    if (lane_id() == 0) { red[threadIdx.x >> 6][2 * k] = a; red[threadIdx.x >> 6][2 * k + 1] = b; }
  }
  __syncthreads();
  if ((int)threadIdx.x < 2 * th.n)
    partial[(size_t)blockIdx.x * 2 * th.n + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// seen = radius > 0 and the running maximum of the screen-space radius (src/vtgaussian_slam.py:681-689): four Gaussians per thread
__device__ __forceinline__ void seen_and_max_radius_block(uint32_t block, int n, const int32_t* __restrict__ radii, float* __restrict__ mx,
                                                          uint8_t* __restrict__ seen) {
  const int i0 = (int)(block * 1024u + threadIdx.x * 4u);
  if (i0 + 3 < n) {
    const int4 r = *reinterpret_cast<const int4*>(radii + i0);
    float4 m = *reinterpret_cast<const float4*>(mx + i0);
    m.x = fmaxf(m.x, (float)r.x); m.y = fmaxf(m.y, (float)r.y); m.z = fmaxf(m.z, (float)r.z); m.w = fmaxf(m.w, (float)r.w);
    *reinterpret_cast<float4*>(mx + i0) = m;
    *reinterpret_cast<uint32_t*>(seen + i0) = (r.x > 0 ? 1u : 0u) | (r.y > 0 ? 0x100u : 0u) | (r.z > 0 ? 0x10000u : 0u) | (r.w > 0 ? 0x1000000u : 0u);
  } else {
    for (int i = i0; i < min(n, i0 + 4); ++i) { mx[i] = fmaxf(mx[i], (float)radii[i]); seen[i] = radii[i] > 0 ? 1 : 0; }
  }
}
__global__ __launch_bounds__(256) void seen_and_max_radius_kernel(int n, const int32_t* __restrict__ radii, float* __restrict__ mx,
                                                                  uint8_t* __restrict__ seen) {
  seen_and_max_radius_block(blockIdx.x, n, radii, mx, seen);
}

// ---- whole loss of get_loss in a handful of launches (src/vtgaussian_slam.py:519-608, 678-679) ----------------------------
// value:    masked_l1_kernel (no gradient images) [+ ssim_forward_kernel] + loss_finalize_kernel
//           out = {loss, mask count, sum |gt_im - im|, sum |gt_depth - depth|, mean SSIM}
// gradient: loss_backward_kernel (depth plane, and the colour planes of the tracking loss)
//           [+ ssim_backward_kernel with the L1 term folded in for the mapping loss]; the upstream gradient is read from
//           device memory, so nothing waits for the host and no element-wise multiply follows.
__global__ __launch_bounds__(256) void loss_finalize_kernel(const float* __restrict__ l1_partial, uint32_t l1_rows,
                                                            const float* __restrict__ ssim_partial, uint32_t ssim_rows,
                                                            int mode, float w_im, float w_depth, float numel_im,
                                                            float* __restrict__ out, float l1_coef = 0.8f,
                                                            int raw = 0, int n_seen = 0, const int32_t* __restrict__ radii = nullptr,
                                                            float* __restrict__ max_radius = nullptr, uint8_t* __restrict__ seen = nullptr) {
  // Round 6: get_loss's bookkeeping (seen = radius > 0, the running maximum of the radius, src/vtgaussian_slam.py:681-689) rides in
  // this launch -- workgroups 1 .. ceil(n / 1024) -- instead of in one of its own: both depend on the render alone, and a
  // launch of a few microseconds of work costs ~5 us on this runtime (gpurun_out/r6/slamlate_b_dens.txt).
  if (blockIdx.x > 0) { seen_and_max_radius_block(blockIdx.x - 1u, n_seen, radii, max_radius, seen); return; }
  __shared__ float red[4][4];
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (uint32_t r = threadIdx.x; r < l1_rows; r += 256u) { a0 += l1_partial[3 * r]; a1 += l1_partial[3 * r + 1]; a2 += l1_partial[3 * r + 2]; }
  for (uint32_t r = threadIdx.x; r < ssim_rows; r += 256u) a3 += ssim_partial[r];
  a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2); a3 = wave_sum(a3);
  if (lane_id() == 0) { red[threadIdx.x >> 6][0] = a0; red[threadIdx.x >> 6][1] = a1; red[threadIdx.x >> 6][2] = a2; red[threadIdx.x >> 6][3] = a3; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float s_im = red[0][0] + red[1][0] + red[2][0] + red[3][0], s_d = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    const float cnt = red[0][2] + red[1][2] + red[2][2] + red[3][2];
    if (raw) {                                                // a band's additive sums (vtgs_slam_loss_band_sums)
      out[0] = s_im; out[1] = s_d; out[2] = cnt; out[3] = red[0][3] + red[1][3] + red[2][3] + red[3][3];
      out[4] = 0.f; out[5] = 0.f; out[6] = 0.f; out[7] = 0.f;
      return;
    }
    const float ssim = (red[0][3] + red[1][3] + red[2][3] + red[3][3]) / numel_im;
    // the two weighted terms the reference's get_loss reports beside their sum (weighted_losses['im'], ['depth'])
    const float t_im = (mode != 1) ? w_im * s_im : w_im * (l1_coef * s_im / numel_im + 0.2f * (1.f - ssim));
    const float t_d = (mode != 1) ? w_depth * s_d : w_depth * s_d / cnt;                   // tracking: masked SUMS, mapping: means
    out[0] = t_im + t_d; out[1] = cnt; out[2] = s_im; out[3] = s_d; out[4] = ssim; out[5] = t_im; out[6] = t_d; out[7] = 0.f;
  }
}

// mode 0 (tracking): g_im = up w_im sign(im - gt) on the mask, g_ds[0] = up w_depth sign(depth - gt) on the mask.
// mode 1 (mapping):  g_ds[0] = up w_depth / count * sign(depth - gt) on the mask; g_im comes from ssim_backward_kernel.
__global__ __launch_bounds__(256) void loss_backward_kernel(const float* __restrict__ im, const float* __restrict__ ds,
                                                            const float* __restrict__ gt_im, const float* __restrict__ gt_depth,
                                                            int P, float sil_thres, int mode, float w_im, float w_depth,
                                                            const float* __restrict__ upstream, const float* __restrict__ fwd_out,
                                                            float* __restrict__ g_im, float* __restrict__ g_ds,
                                                            const float* __restrict__ extra_mask, int p0, int p1) {
  const float up = upstream[0];
  const float cd = (mode != 1) ? up * w_depth : up * w_depth / fwd_out[1];
  const float ci = up * w_im;
  const bool aligned = all_aligned16(ds, gt_depth, g_ds, extra_mask) && (mode == 1 || all_aligned16(im, gt_im, g_im));
  walk_pixels(P, p0, p1, aligned, [&](auto n, int i) {
    constexpr int N = decltype(n)::value;
    using V = Px<N>;
    const V depth = V::load(ds + i), sil = V::load(ds + P + i), dsq = V::load(ds + 2 * (size_t)P + i), gd = V::load(gt_depth + i);
    const V em = V::load_or_ones(extra_mask, i);
    bool m[N];
    V g;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      m[k] = depth_mask(mode, sil_thres, depth[k], sil[k], dsq[k], gd[k], em[k]);
      g[k] = l1_grad(m[k], gd[k] - depth[k], cd);
    }
    g.store(g_ds + i); V::all(0.f).store(g_ds + P + i); V::all(0.f).store(g_ds + 2 * (size_t)P + i);
    if (mode != 1) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const V x = V::load(im + (size_t)c * P + i), y = V::load(gt_im + (size_t)c * P + i);
#pragma unroll
        for (int k = 0; k < N; ++k) g[k] = l1_grad(colour_mask(mode, m[k]), y[k] - x[k], ci);
        g.store(g_im + (size_t)c * P + i);
      }
    }
  });
}

// One band's share of the loss from its own sums and the sums over all bands ({sum_im, sum_depth, count, sum SSIM}): the
// shares of all bands add up to the full-frame loss of loss_finalize_kernel.  Only the mapping depth term is not additive
// (a masked MEAN: the band's sum over the GLOBAL count); the "1" of (1 - SSIM) goes to the first band.
__global__ void band_share_kernel(const float* __restrict__ own, const float* __restrict__ all, int mode, float w_im,
                                  float w_depth, float numel_im, float l1_coef, int first, float* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float s_im = own[0], s_d = own[1], cnt = all[2];
  const float t_im = (mode != 1) ? w_im * s_im : w_im * (l1_coef * s_im / numel_im + 0.2f * ((first ? 1.f : 0.f) - own[3] / numel_im));
  const float t_d = (mode != 1) ? w_depth * s_d : w_depth * s_d / cnt;
  out[0] = t_im + t_d; out[1] = cnt; out[2] = s_im; out[3] = s_d; out[4] = all[3] / numel_im; out[5] = t_im; out[6] = t_d; out[7] = 0.f;
}

}  // namespace vtgs

using namespace vtgs;

// ---- host side: each kernel that several entry points launch is launched by one function here, on the rows [rb, re) or the
// pixels [p0, p1) of the frame (the full-frame entry points: 0, H and 0, P) ---------------------------------------------------

// what the loss entry points have in common: the mode, the four inputs, the frame size and the optional planes
struct LossIn {
  int32_t mode;
  const float *im, *ds, *gt_im, *gt_depth;
  int32_t H, W;
  float sil_thres;
  const float *extra_mask, *color_weight;                             // color_weight: the mapping loss's only (else NULL)
  bool ok() const { return mode >= 0 && mode <= 2 && im && ds && gt_im && gt_depth && H > 0 && W > 0; }
  float numel_im() const { return (float)((size_t)3 * H * W); }
  float l1_coef() const { return color_weight ? 1.0f : 0.8f; }        // weighted: 10 additional_mask + 0.8 carries the 0.8
};
static LossIn loss_in(int32_t mode, const float* im, const float* ds, const float* gt_im, const float* gt_depth, int32_t H, int32_t W,
                      float sil_thres, const float* extra_mask, const float* color_weight) {
  return LossIn{mode, im, ds, gt_im, gt_depth, H, W, sil_thres, extra_mask, mode == 1 ? color_weight : nullptr};
}

// returns the rows of partial sums it writes
static uint32_t launch_masked_l1(hipStream_t st, const LossIn& in, int32_t p0, int32_t p1, float* partial, float* g_im, float* g_ds) {
  const uint32_t rows = vtgs_masked_l1_partial_rows(p1 - p0);
  hipLaunchKernelGGL(masked_l1_kernel, dim3(rows), dim3(256), 0, st, in.im, in.ds, in.gt_im, in.gt_depth, in.H * in.W, in.sil_thres,
                     in.mode, partial, g_im, g_ds, in.extra_mask, in.color_weight, p0, p1);
  return rows;
}

// workgroups of an SSIM launch over `tiles` tiles: what the chip holds at once (256 CUs x 3 workgroups of 41 KB LDS), every
// workgroup walking the same number of tiles when it can (ceil(tiles / rounds))
static inline uint32_t ssim_grid(uint32_t tiles, uint32_t per_cu = 3u) {   // (the backward's 37 KB: 4 per CU)
  const uint32_t kResident = 256u * per_cu;
  if (tiles <= kResident) return tiles ? tiles : 1u;
  const uint32_t rounds = (tiles + kResident - 1u) / kResident;
  return (tiles + rounds - 1u) / rounds;
}

// the tile rows that cover the image rows [lo, hi)
struct SsimRows { int tx, ty0, ty; };
static SsimRows ssim_rows(int32_t W, int32_t lo, int32_t hi) { return SsimRows{(W + kST - 1) / kST, lo / kST, (hi - 1) / kST - lo / kST + 1}; }

// SSIM sums (and derivative maps) of rows [rb, re); returns the rows of partial sums it writes
static uint32_t launch_ssim_forward(hipStream_t st, const float* img1, const float* img2, int32_t C, int32_t H, int32_t W, int32_t rb,
                                    int32_t re, float* partial, float* gmaps) {
  const SsimRows t = ssim_rows(W, rb, re);
  const uint32_t tiles = (uint32_t)(C * t.tx * t.ty);
  hipLaunchKernelGGL(ssim_forward_kernel, dim3(ssim_grid(tiles)), dim3(256), 0, st, img1, img2, C, H, W, t.tx, t.ty, partial, gmaps,
                     t.ty0, rb, re);
  return tiles;
}

// the gradient of the SSIM of rows [rb, re): it lands on rows [rb - 5, re + 5) of the image
static void launch_ssim_backward(hipStream_t st, const float* img1, const float* img2, const float* gmaps, const float* upstream,
                                 int32_t C, int32_t H, int32_t W, int32_t rb, int32_t re, float* g_img1, float ssim_coef, float l1_coef,
                                 const float* l1_weight) {
  const SsimRows t = ssim_rows(W, rb - kSR > 0 ? rb - kSR : 0, re + kSR < H ? re + kSR : H);
  hipLaunchKernelGGL(ssim_backward_kernel, dim3(ssim_grid((uint32_t)(C * t.tx * t.ty), 4u)), dim3(256), 0, st, img1, img2, gmaps,
                     upstream, C, H, W, t.tx, t.ty, g_img1, ssim_coef, l1_coef, l1_weight, t.ty0, rb, re);
}

// the sums of rows [rb, re) into `scratch`: masked L1 partials first, the SSIM partials of the mapping loss behind the L1
// partials of a whole frame (a band's too)
struct LossSums { uint32_t l1_rows, ssim_rows; float* ssim_partial; };
static LossSums launch_loss_sums(hipStream_t st, const LossIn& in, int32_t rb, int32_t re, float* scratch, float* ssim_grad_maps) {
  LossSums s;
  s.l1_rows = launch_masked_l1(st, in, rb * in.W, re * in.W, scratch, nullptr, nullptr);
  s.ssim_partial = scratch + (size_t)vtgs_masked_l1_partial_rows(in.H * in.W) * 3;
  s.ssim_rows = in.mode == 1 ? launch_ssim_forward(st, in.im, in.gt_im, 3, in.H, in.W, rb, re, s.ssim_partial, ssim_grad_maps) : 0u;
  return s;
}

// both gradient images of rows [rb, re) (fwd_out: the out8 whose count the mapping depth term divides by)
static void launch_loss_gradient(hipStream_t st, const LossIn& in, int32_t rb, int32_t re, float w_im, float w_depth,
                                 const float* ssim_grad_maps, const float* fwd_out, const float* upstream, float* g_im, float* g_ds) {
  const int32_t p0 = rb * in.W, p1 = re * in.W;
  hipLaunchKernelGGL(loss_backward_kernel, dim3(vtgs_masked_l1_partial_rows(p1 - p0)), dim3(256), 0, st, in.im, in.ds, in.gt_im,
                     in.gt_depth, in.H * in.W, in.sil_thres, in.mode, w_im, w_depth, upstream, fwd_out, g_im, g_ds, in.extra_mask, p0, p1);
  if (in.mode == 1)
    launch_ssim_backward(st, in.im, in.gt_im, ssim_grad_maps, upstream, 3, in.H, in.W, rb, re, g_im, -0.2f * w_im,
                         in.l1_coef() * w_im / in.numel_im(), in.color_weight);
}

static int silhouette_sweep(const char* what, const float* im, const float* silhouette, const float* gt_im, const float* gt_depth,
                            int32_t pixels, int32_t p0, int32_t p1, const float* thresholds, int32_t n_thresholds, float* partial_sums,
                            void* stream) {
  if (!im || !silhouette || !gt_im || !gt_depth || !thresholds || !partial_sums || pixels <= 0 || n_thresholds <= 0 ||
      n_thresholds > 8 || p0 < 0 || p1 <= p0 || p1 > pixels)
    return VTGS_ERR_INVALID_ARGUMENT;
  SweepThresholds th;
  th.n = n_thresholds;
  for (int k = 0; k < 8; ++k) th.c[k] = k < n_thresholds ? thresholds[k] : 0.f;
  hipLaunchKernelGGL(silhouette_sweep_kernel, dim3(vtgs_masked_l1_partial_rows(p1 - p0)), dim3(256), 0, (hipStream_t)stream, im,
                     silhouette, gt_im, gt_depth, pixels, th, partial_sums, p0, p1);
  return launch_status(what);
}

extern "C" {

uint32_t vtgs_masked_l1_partial_rows(int32_t pixels) {
  if (pixels <= 0) return 0;
  const uint32_t b = (uint32_t)((pixels + 255) / 256);
  return b < 1024u ? b : 1024u;
}

int vtgs_masked_l1(const float* im, const float* depth_sil, const float* gt_im, const float* gt_depth, int32_t pixels,
                   float sil_thres, int32_t mode, float* partial_sums, float* g_im, float* g_depth_sil, void* stream) {
  const LossIn in = loss_in(mode, im, depth_sil, gt_im, gt_depth, 1, pixels, sil_thres, nullptr, nullptr);   // one row of pixels
  if (!in.ok() || !partial_sums || !g_im || !g_depth_sil) return VTGS_ERR_INVALID_ARGUMENT;
  launch_masked_l1((hipStream_t)stream, in, 0, pixels, partial_sums, g_im, g_depth_sil);
  return launch_status(__func__);
}

int vtgs_silhouette_sweep(const float* im, const float* silhouette, const float* gt_im, const float* gt_depth,
                          int32_t pixels, const float* thresholds, int32_t n_thresholds, float* partial_sums, void* stream) {
  return silhouette_sweep(__func__, im, silhouette, gt_im, gt_depth, pixels, 0, pixels, thresholds, n_thresholds, partial_sums, stream);
}

int vtgs_silhouette_sweep_band(const float* im, const float* silhouette, const float* gt_im, const float* gt_depth,
                               int32_t pixels, int32_t pixel_begin, int32_t pixel_end, const float* thresholds,
                               int32_t n_thresholds, float* partial_sums, void* stream) {
  return silhouette_sweep(__func__, im, silhouette, gt_im, gt_depth, pixels, pixel_begin, pixel_end, thresholds, n_thresholds,
                          partial_sums, stream);
}

// seen_and_max_radius_block has no scalar fallback: radii / max_2d_radius are read as int4 / float4 and four `seen` bytes are
// stored as one uint32_t, so both entry points refuse pointers that are not aligned for that before any device work
static bool bookkeeping_aligned(const int32_t* radii, const float* max_2d_radius, const uint8_t* seen) {
  return (((uintptr_t)radii | (uintptr_t)max_2d_radius) & 15u) == 0u && ((uintptr_t)seen & 3u) == 0u;
}

int vtgs_seen_and_max_radius(int32_t n, const int32_t* radii, float* max_2d_radius, uint8_t* seen, void* stream) {
  if (n < 0 || (n > 0 && (!radii || !max_2d_radius || !seen))) return VTGS_ERR_INVALID_ARGUMENT;
  if (n == 0) return VTGS_OK;
  if (!bookkeeping_aligned(radii, max_2d_radius, seen)) return VTGS_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(seen_and_max_radius_kernel, dim3((uint32_t)((n + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream, n, radii,
                     max_2d_radius, seen);
  return launch_status(__func__);
}

uint32_t vtgs_ssim_partial_rows(int32_t channels, int32_t height, int32_t width) {
  if (channels <= 0 || height <= 0 || width <= 0) return 0;
  return (uint32_t)(channels * ((height + kST - 1) / kST) * ((width + kST - 1) / kST));
}

int vtgs_ssim_forward(const float* img1, const float* img2, int32_t channels, int32_t height, int32_t width,
                      float* partial_sums, float* grad_maps, void* stream) {
  if (!img1 || !img2 || !partial_sums || channels <= 0 || height <= 0 || width <= 0) return VTGS_ERR_INVALID_ARGUMENT;
  launch_ssim_forward((hipStream_t)stream, img1, img2, channels, height, width, 0, height, partial_sums, grad_maps);
  return launch_status(__func__);
}

int vtgs_ssim_backward(const float* img1, const float* img2, const float* grad_maps, const float* upstream,
                       int32_t channels, int32_t height, int32_t width, float* grad_img1, void* stream) {
  if (!img1 || !img2 || !grad_maps || !upstream || !grad_img1 || channels <= 0 || height <= 0 || width <= 0)
    return VTGS_ERR_INVALID_ARGUMENT;
  launch_ssim_backward((hipStream_t)stream, img1, img2, grad_maps, upstream, channels, height, width, 0, height, grad_img1, 1.f, 0.f,
                       nullptr);
  return launch_status(__func__);
}

size_t vtgs_loss_scratch_floats(int32_t height, int32_t width) {
  if (height <= 0 || width <= 0) return 0;
  return (size_t)vtgs_masked_l1_partial_rows(height * width) * 3 + vtgs_ssim_partial_rows(3, height, width);
}

// ---- whole loss of get_loss in a handful of launches (see loss_finalize_kernel) ---------------------------------------------
int vtgs_slam_loss_forward(int32_t mode, const float* im, const float* depth_sil, const float* gt_im, const float* gt_depth,
                           int32_t height, int32_t width, float sil_thres, float w_im, float w_depth, float* scratch,
                           float* ssim_grad_maps, float* out5, const float* extra_mask, const float* color_weight,
                           void* stream) {
  return vtgs_slam_loss_forward_seen(mode, im, depth_sil, gt_im, gt_depth, height, width, sil_thres, w_im, w_depth, scratch,
                                     ssim_grad_maps, out5, extra_mask, color_weight, 0, nullptr, nullptr, nullptr, stream);
}

int vtgs_slam_loss_forward_seen(int32_t mode, const float* im, const float* depth_sil, const float* gt_im, const float* gt_depth,
                                int32_t height, int32_t width, float sil_thres, float w_im, float w_depth, float* scratch,
                                float* ssim_grad_maps, float* out5, const float* extra_mask, const float* color_weight,
                                int32_t n, const int32_t* radii, float* max_2d_radius, uint8_t* seen, void* stream) {
  const LossIn in = loss_in(mode, im, depth_sil, gt_im, gt_depth, height, width, sil_thres, extra_mask, color_weight);
  if (!in.ok() || !scratch || !out5) return VTGS_ERR_INVALID_ARGUMENT;
  if (n < 0 || (n > 0 && (!radii || !max_2d_radius || !seen))) return VTGS_ERR_INVALID_ARGUMENT;
  if (n > 0 && !bookkeeping_aligned(radii, max_2d_radius, seen)) return VTGS_ERR_INVALID_ARGUMENT;
  hipStream_t st = (hipStream_t)stream;
  const LossSums s = launch_loss_sums(st, in, 0, height, scratch, ssim_grad_maps);
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1u + (uint32_t)((n + 1023) / 1024)), dim3(256), 0, st, scratch, s.l1_rows,
                     s.ssim_partial, s.ssim_rows, mode, w_im, w_depth, in.numel_im(), out5, in.l1_coef(), 0, (int)n, radii,
                     max_2d_radius, seen);
  return launch_status(__func__);
}

int vtgs_slam_loss_backward(int32_t mode, const float* im, const float* depth_sil, const float* gt_im, const float* gt_depth,
                            int32_t height, int32_t width, float sil_thres, float w_im, float w_depth,
                            const float* ssim_grad_maps, const float* fwd_out5, const float* upstream, float* g_im,
                            float* g_depth_sil, const float* extra_mask, const float* color_weight, void* stream) {
  const LossIn in = loss_in(mode, im, depth_sil, gt_im, gt_depth, height, width, sil_thres, extra_mask, color_weight);
  if (!in.ok() || !fwd_out5 || !upstream || !g_im || !g_depth_sil || (mode == 1 && !ssim_grad_maps)) return VTGS_ERR_INVALID_ARGUMENT;
  launch_loss_gradient((hipStream_t)stream, in, 0, height, w_im, w_depth, ssim_grad_maps, fwd_out5, upstream, g_im, g_depth_sil);
  return launch_status(__func__);
}

// ---- one band of the tile-row partition: additive sums, the band's share, its gradient images -----------
static bool band_ok(int32_t height, int32_t rb, int32_t re) { return rb >= 0 && re > rb && re <= height; }

int vtgs_slam_loss_band_sums(int32_t mode, const float* im, const float* depth_sil, const float* gt_im, const float* gt_depth,
                             int32_t height, int32_t width, int32_t row_begin, int32_t row_end, float sil_thres,
                             float* scratch, float* ssim_grad_maps, float* sums8, const float* extra_mask,
                             const float* color_weight, void* stream) {
  const LossIn in = loss_in(mode, im, depth_sil, gt_im, gt_depth, height, width, sil_thres, extra_mask, color_weight);
  if (!in.ok() || !scratch || !sums8 || !band_ok(height, row_begin, row_end)) return VTGS_ERR_INVALID_ARGUMENT;
  hipStream_t st = (hipStream_t)stream;
  const LossSums s = launch_loss_sums(st, in, row_begin, row_end, scratch, ssim_grad_maps);
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, st, scratch, s.l1_rows, s.ssim_partial, s.ssim_rows, mode, 0.f,
                     0.f, in.numel_im(), sums8, 0.8f, 1);
  return launch_status(__func__);
}

int vtgs_slam_loss_band_share(int32_t mode, const float* own_sums8, const float* all_sums8, int32_t height, int32_t width,
                              float w_im, float w_depth, int32_t has_color_weight, int32_t first_band, float* out8,
                              void* stream) {
  if ((mode < 0 || mode > 2) || !own_sums8 || !all_sums8 || !out8 || height <= 0 || width <= 0) return VTGS_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(band_share_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, own_sums8, all_sums8, mode, w_im, w_depth,
                     (float)((size_t)3 * height * width), (mode == 1 && has_color_weight) ? 1.0f : 0.8f, first_band, out8);
  return launch_status(__func__);
}

int vtgs_slam_loss_band_backward(int32_t mode, const float* im, const float* depth_sil, const float* gt_im,
                                 const float* gt_depth, int32_t height, int32_t width, int32_t row_begin, int32_t row_end,
                                 float sil_thres, float w_im, float w_depth, const float* ssim_grad_maps,
                                 const float* share_out8, const float* upstream, float* g_im, float* g_depth_sil,
                                 const float* extra_mask, const float* color_weight, void* stream) {
  const LossIn in = loss_in(mode, im, depth_sil, gt_im, gt_depth, height, width, sil_thres, extra_mask, color_weight);
  if (!in.ok() || !share_out8 || !upstream || !g_im || !g_depth_sil || !band_ok(height, row_begin, row_end) ||
      (mode == 1 && !ssim_grad_maps))
    return VTGS_ERR_INVALID_ARGUMENT;
  launch_loss_gradient((hipStream_t)stream, in, row_begin, row_end, w_im, w_depth, ssim_grad_maps, share_out8, upstream, g_im,
                       g_depth_sil);
  return launch_status(__func__);
}

}  // extern "C"

