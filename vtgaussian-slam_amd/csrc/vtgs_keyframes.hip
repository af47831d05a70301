// vtgs_keyframes.hip -- keyframe / base-frame overlap selection: the counting of all keyframes in one pass over (points x keyframes).
//
// Replaces the per-keyframe torch loops of utils/keyframe_selection.py (keyframe_selection_overlap :40-116, ..._visbased
// :121-229, ..._visbased_earliest_dynamic_new_topkbase :581-724, find_earliest_keyframe :1581-1613) with get_pointcloud (:10-37):
// about fifteen launches, a grid_sample and a host-compared sum per keyframe there; k + 3 integers read once here.
//
//   keyframe_fold          K [R|t] of every selected keyframe (3x4, products in double, rounded once) into a table of 64-byte rows
//   keyframe_mark_repeats  sampled mode: two bits per pixel -- seen, and seen again.  A sample whose pixel has the second bit
//                          is dropped in all its copies (the reference's unique(..., return_counts=True) rule).
//   keyframe_overlap       lane = source point, formed once and kept in registers; a loop over the keyframes of this
//                          blockIdx.y slice reads the folded rows through scalar loads (a read-only
//                          __restrict__ kernel argument; behind the argument struct they were vector loads); ballot + popcount per wavefront into
//                          LDS counters, one global atomicAdd per keyframe per workgroup.  Integer adds: the record does not
//                          depend on the order of workgroups.
#include "../../include/vtgs.h"
#include "vtgs_internal.h"
#include "vtgs_kernels.h"

namespace vtgs {

__global__ __launch_bounds__(256) void keyframe_fold(KeyframeArgs a) {
  const float* __restrict__ k = a.k;
  for (int j = (int)(blockIdx.x * 256u + threadIdx.x); j < a.K; j += (int)(gridDim.x * 256u)) {
    const int s = a.slots ? a.slots[j] : j;
    KeyframeRow r{};
    r.slot = s;
    if (s >= 0) {
      const float* __restrict__ w = a.kf_w2c + (size_t)s * 16;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c)
          r.m[4 * i + c] = (float)((double)k[3 * i] * (double)w[c] + (double)k[3 * i + 1] * (double)w[4 + c] +
                                   (double)k[3 * i + 2] * (double)w[8 + c]);
    }
    a.rows[j] = r;
  }
}

__global__ __launch_bounds__(256) void keyframe_mark_repeats(KeyframeArgs a) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= a.samples) return;
  const int r = a.sampled_rc[2 * i], c = a.sampled_rc[2 * i + 1];
  if ((unsigned)r >= (unsigned)a.H || (unsigned)c >= (unsigned)a.W) return;
  const uint32_t p = (uint32_t)r * (uint32_t)a.W + (uint32_t)c, bit = 1u << (p & 31u);
  if (atomicOr(&a.seen[p >> 5], bit) & bit) atomicOr(&a.repeated[p >> 5], bit);
}

__global__ __launch_bounds__(256) void keyframe_overlap(KeyframeArgs a, const KeyframeRow* __restrict__ rows) {
  __shared__ uint32_t s_cnt[kKeyframeSliceMax];
  __shared__ uint32_t s_tot[2];
  const uint32_t t = threadIdx.x;
  const int j0 = (int)(blockIdx.y * a.per_slice), j1 = min(a.K, j0 + (int)a.per_slice);
  for (uint32_t i = t; i < (uint32_t)(j1 - j0); i += 256u) s_cnt[i] = 0u;
  if (t < 2u) s_tot[t] = 0u;
  __syncthreads();
  const size_t P = (size_t)a.W * a.H;
  const uint32_t S = a.sampled_rc ? (uint32_t)a.samples : (uint32_t)P;
  const uint32_t i = blockIdx.x * 256u + t;
  bool source = false, kept = false;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (i < S) {
    int r, c;
    bool in_image = true;
    if (a.sampled_rc) {
      r = a.sampled_rc[2 * i]; c = a.sampled_rc[2 * i + 1];
      in_image = (unsigned)r < (unsigned)a.H && (unsigned)c < (unsigned)a.W;
    } else {
      r = (int)(i / (uint32_t)a.W); c = (int)(i % (uint32_t)a.W);
    }
    if (in_image) {
      const uint32_t p = (uint32_t)r * (uint32_t)a.W + (uint32_t)c;
      const float z = a.depth[p];
      source = z > 0.f;
      if (source) {
        const float fx = a.k[0], fy = a.k[4], cx = a.k[2], cy = a.k[5];
        const float* __restrict__ w = a.w2c;
        const float dx = ((float)c - cx) / fx * z - w[3], dy = ((float)r - cy) / fy * z - w[7], dz = z - w[11];
        px = fmaf(w[8], dz, fmaf(w[4], dy, w[0] * dx));          // the rigid inverse: R^T (p_cam - t)
        py = fmaf(w[9], dz, fmaf(w[5], dy, w[1] * dx));
        pz = fmaf(w[10], dz, fmaf(w[6], dy, w[2] * dx));
        const bool origin = rintf(px * 1e4f) == 0.f && rintf(py * 1e4f) == 0.f && rintf(pz * 1e4f) == 0.f;
        const bool repeat = a.sampled_rc && ((a.repeated[p >> 5] >> (p & 31u)) & 1u);
        kept = !origin && !repeat;
      }
    }
  }
  const float hi_x = (float)a.W - a.edge, hi_y = (float)a.H - a.edge;
  for (int j = j0; j < j1; ++j) {
    const KeyframeRow* row = rows + j;                           // (uniform)
    const float qx = fmaf(row->m[0], px, fmaf(row->m[1], py, fmaf(row->m[2], pz, row->m[3])));
    const float qy = fmaf(row->m[4], px, fmaf(row->m[5], py, fmaf(row->m[6], pz, row->m[7])));
    const float qz = fmaf(row->m[8], px, fmaf(row->m[9], py, fmaf(row->m[10], pz, row->m[11])));
    const float zp = qz + 1e-5f;
    const float u = qx / zp, v = qy / zp;
    const int slot = row->slot;
    bool hit = kept && slot >= 0 && (u < hi_x) && (u > a.edge) && (v < hi_y) && (v > a.edge) && (zp > 0.f);
    if (hit && a.kf_depth) {
      // edge >= 0: 0 < u < W and 0 < v < H here, so only the taps at column W / row H can fall outside (zero padding)
      const float x0f = floorf(u), y0f = floorf(v);
      const int x0 = (int)x0f, y0 = (int)y0f;
      const float wx1 = u - x0f, wx0 = (x0f + 1.f) - u, wy1 = v - y0f, wy0 = (y0f + 1.f) - v;
      const float* __restrict__ img = a.kf_depth + (size_t)slot * P + (size_t)y0 * a.W + x0;
      const bool xi = x0 + 1 < a.W, yi = y0 + 1 < a.H;
      const float nw = img[0], ne = xi ? img[1] : 0.f, sw = yi ? img[a.W] : 0.f, se = (xi && yi) ? img[a.W + 1] : 0.f;
      const float d = nw * (wx0 * wy0) + ne * (wx1 * wy0) + sw * (wx0 * wy1) + se * (wx1 * wy1);
      hit = fabsf(d - zp) < a.thresh * fminf(d, zp);
    }
    const uint32_t cnt = (uint32_t)__popcll(__ballot(hit));
    if ((t & 63u) == 0u && cnt) atomicAdd(&s_cnt[j - j0], cnt);
    if (a.pair_mask && i < S) a.pair_mask[(size_t)j * S + i] = kept ? (hit ? 1 : 0) : 0xFF;
  }
  if (blockIdx.y == 0) {
    const uint32_t nk = (uint32_t)__popcll(__ballot(kept)), ns = (uint32_t)__popcll(__ballot(source));
    if ((t & 63u) == 0u) {
      if (nk) atomicAdd(&s_tot[0], nk);
      if (ns) atomicAdd(&s_tot[1], ns);
    }
  }
  __syncthreads();
  for (uint32_t q = t; q < (uint32_t)(j1 - j0); q += 256u)
    if (s_cnt[q]) atomicAdd(&a.record[j0 + (int)q], s_cnt[q]);
  if (blockIdx.y == 0 && t == 0 && s_tot[1]) {
    if (s_tot[0]) atomicAdd(&a.record[a.K], s_tot[0]);
    atomicAdd(&a.record[a.K + 1], s_tot[1]);
    if (s_tot[1] != s_tot[0]) atomicAdd(&a.record[a.K + 2], s_tot[1] - s_tot[0]);
  }
}

}  // namespace vtgs
