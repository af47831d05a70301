// vtgs_masks.hip -- the detached masks of get_loss for TUM / ScanNet / ScanNet++ in one pass: visibility in up to three
// overlapping base frames, the far-depth filter and the outlier-depth mask, written as the loss node's float `extra_mask`.
//
// Replaces the torch chain of src/vtgaussian_slam.py:525-528 (50 x median outlier mask), :536-584 with get_vis_mask :376-404
// (a torch.where the host waits for, a torch.inverse, about a dozen element-wise / matmul launches and a grid_sample per
// overlapping frame) and :586-588 (far filter), plus the ANDs and the bool -> float conversion behind them.
//
//   tracking_mask_fold    one small workgroup: M_j = K W_j[:3,:] inverse(curr_w2c) per overlap, 3x4, products in double and
//                         rounded once, into 64-byte rows.  Every pose is read on the device (the current one is a slice of
//                         the parameters and changes every iteration).  inverse = the rigid [R^T | -R^T t].
//   tracking_mask_error   err[p] = |gt - depth| * (gt > 0) for the radix select of vtgs_densify.hip (outlier mask only)
//   tracking_mask         lane = pixel.  The folded rows are a read-only __restrict__ kernel argument, so they come through
//                         scalar loads.  No atomics, no LDS, no dependence between workgroups.
#include "../../include/vtgs.h"
#include "vtgs_internal.h"
#include "vtgs_kernels.h"

namespace vtgs {

__global__ __launch_bounds__(64) void tracking_mask_fold(MaskArgs a) {
  const int j = (int)threadIdx.x;
  if (j >= a.n) return;
  const float* __restrict__ c = a.curr_w2c;
  const float* __restrict__ k = a.k;
  const float* __restrict__ w = j == 0 ? a.ov_w2c0 : j == 1 ? a.ov_w2c1 : a.ov_w2c2;
  // inverse(curr_w2c) as the rigid inverse: rows of R^T, and -R^T t
  double inv[3][4];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    inv[r][0] = (double)c[r]; inv[r][1] = (double)c[4 + r]; inv[r][2] = (double)c[8 + r];
    inv[r][3] = -((double)c[r] * (double)c[3] + (double)c[4 + r] * (double)c[7] + (double)c[8 + r] * (double)c[11]);
  }
  double t[3][4];                                               // W_j[:3,:] inverse(curr_w2c)
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      t[r][q] = (double)w[4 * r] * inv[0][q] + (double)w[4 * r + 1] * inv[1][q] + (double)w[4 * r + 2] * inv[2][q] +
                (q == 3 ? (double)w[4 * r + 3] : 0.0);
  MaskRow row{};
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      row.m[4 * r + q] = (float)((double)k[3 * r] * t[0][q] + (double)k[3 * r + 1] * t[1][q] + (double)k[3 * r + 2] * t[2][q]);
  a.rows[j] = row;
}

__global__ __launch_bounds__(256) void tracking_mask_error(MaskArgs a) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= (uint32_t)(a.W * a.H)) return;
  const float gd = a.gt[p];
  a.err[p] = fabsf(gd - a.rendered[p]) * (gd > 0.f ? 1.f : 0.f);   // a literal product, as torch.abs(..) * (gt > 0)
}

// grid_sample(align_corners = True, padding_mode = 'zeros') at pixel coordinates (u, v): each of the four taps is tested
// against the image on its own; a point wholly outside, or a coordinate that is not finite, samples 0
__device__ __forceinline__ float sample_zero_pad(const float* __restrict__ img, int W, int H, float u, float v) {
  if (!(u > -1.f && u < (float)W && v > -1.f && v < (float)H)) return 0.f;
  const float x0f = floorf(u), y0f = floorf(v);
  const int x0 = (int)x0f, y0 = (int)y0f;                        // -1 .. W - 1, -1 .. H - 1
  const float wx1 = u - x0f, wx0 = (x0f + 1.f) - u, wy1 = v - y0f, wy0 = (y0f + 1.f) - v;
  const bool xl = x0 >= 0, xr = x0 + 1 < W, yt = y0 >= 0, yb = y0 + 1 < H;
  const int xa = xl ? x0 : 0, xb = xr ? x0 + 1 : W - 1, ya = yt ? y0 : 0, yc = yb ? y0 + 1 : H - 1;   // always inside
  const float* __restrict__ r0 = img + (size_t)ya * W;
  const float* __restrict__ r1 = img + (size_t)yc * W;
  const float nw = (xl && yt) ? r0[xa] : 0.f, ne = (xr && yt) ? r0[xb] : 0.f;
  const float sw = (xl && yb) ? r1[xa] : 0.f, se = (xr && yb) ? r1[xb] : 0.f;
  return nw * (wx0 * wy0) + ne * (wx1 * wy0) + sw * (wx0 * wy1) + se * (wx1 * wy1);
}

__global__ __launch_bounds__(256) void tracking_mask(MaskArgs a, const MaskRow* __restrict__ rows) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= (uint32_t)(a.W * a.H)) return;
  const float z = a.gt[p];
  bool keep = true;
  uint32_t bits = 0u;
  if (a.n > 0) {
    const int r = (int)(p / (uint32_t)a.W), c = (int)(p % (uint32_t)a.W);
    const float fx = a.k[0], fy = a.k[4], cx = a.k[2], cy = a.k[5];
    const float px = ((float)c - cx) / fx * z, py = ((float)r - cy) / fy * z;
    const bool valid = z >= 0.f;                                 // the reference's point list: gt_depth >= 0 (NaN: no)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if (j < a.n) {                                             // (uniform)
        const MaskRow* row = rows + j;
        const float qx = fmaf(row->m[0], px, fmaf(row->m[1], py, fmaf(row->m[2], z, row->m[3])));
        const float qy = fmaf(row->m[4], px, fmaf(row->m[5], py, fmaf(row->m[6], z, row->m[7])));
        const float qz = fmaf(row->m[8], px, fmaf(row->m[9], py, fmaf(row->m[10], z, row->m[11])));
        const float zp = qz + 1e-5f;
        const float u = qx / zp, v = qy / zp;
        const float* __restrict__ img = j == 0 ? a.ov_depth0 : j == 1 ? a.ov_depth1 : a.ov_depth2;
        const float d = sample_zero_pad(img, a.W, a.H, u, v);
        if (valid && fabsf(d - zp) < a.thres * fminf(d, zp)) bits |= 1u << j;
      }
    }
    keep = bits != 0u;
  }
  if (a.use_far) keep = keep && (z < a.far);
  if (a.err) keep = keep && (a.err[p] < 50.f * a.median[0]) && (z > 0.f);   // a NaN median: false everywhere
  a.out[p] = keep ? 1.f : 0.f;
  if (a.out_u8) a.out_u8[p] = keep ? 1 : 0;
  if (a.out_bits) a.out_bits[p] = (uint8_t)bits;
}

}  // namespace vtgs
