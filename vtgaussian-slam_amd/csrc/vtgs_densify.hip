// vtgs_densify.hip -- the step that makes the map grow, on the device: exact lower median + unexplained pixels -> new Gaussians.
//
// Replaces `add_new_gaussians_base_frame` (src/vtgaussian_slam.py:732-813) behind its render, with `get_pointcloud` (:76-128),
// `initialize_new_params` (:692-728) and the point-cloud half of `initialize_params_base_timestep` (:296-348): the reference
// takes depth_error.median(), forms two boolean masks, sends one through the host and cv2.resize, and gathers / concatenates.
//
//   lower_median_pass<0|1|2>   radix select over an order-preserving 32-bit key, 11 + 11 + 10 bits.  A workgroup builds the
//                              histogram of its values in LDS and merges the non-empty bins into the global histogram with
//                              integer atomics (order-independent: the result is exact and repeatable).  Pass k+1 keeps only
//                              the keys under the prefix found so far; every one of its workgroups finds the bucket of pass k
//                              itself from the <= 2048 global bins, so no launch sits between the passes and no workgroup
//                              ever waits on another.
//   lower_median_finish        one workgroup: bucket of the last histogram -> the value.  densify_count does the same step
//                              itself (every workgroup, redundantly) and needs no finish launch.
//   densify_count              a workgroup per chunk of kDensifyChunk consecutive pixels (original-resolution chunks first,
//                              then the chunks of the densification image): the number of selected pixels, from ballots.
//                              A pixel of the densification image re-evaluates the decision of its nearest original pixel.
//   densify_emit               the same decisions again; a workgroup sums the counts in front of it (a few thousand words),
//                              checks n + total <= capacity and writes its rows at n + offset + rank, ranks from ballots in
//                              lane order -- the row order of boolean-mask indexing followed by torch.cat.
#include "../../include/vtgs.h"
#include "vtgs_internal.h"
#include "vtgs_kernels.h"

namespace vtgs {

// float32 bits -> unsigned key with the same order (negatives: all bits flipped, others: sign bit set).  -0 sorts right below
// +0; torch.median compares them equal, so either is a correct median.
__device__ __forceinline__ uint32_t median_key(float v) {
  const uint32_t b = __float_as_uint(v);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float median_value(uint32_t k) {
  return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k);
}
// torch.abs(gt_depth - render_depth) * (gt_depth > 0): a literal product (inf * 0 = NaN, as there)
__device__ __forceinline__ float depth_error(float gd, float rd) { return fabsf(gd - rd) * (gd > 0.f ? 1.f : 0.f); }

__device__ __forceinline__ float median_load(const MedianSource& s, uint64_t i) {
  return s.values ? s.values[i] : depth_error(s.gt_depth[i], s.depth[i]);
}

// The bucket of a global histogram of BINS bins that holds `rank` (0-based, < the histogram's total), and the rank inside
// that bucket.  All 256 threads call it; a thread owns BINS / 256 consecutive bins (16- / 32-byte loads).
template <int BINS>
__device__ __forceinline__ void find_bucket(const uint32_t* __restrict__ hist, uint32_t rank, uint32_t* s_w /*[4]*/,
                                            uint32_t* s_res /*[2]*/, uint32_t& digit, uint32_t& rank_in) {
  constexpr int PER = BINS / 256;
  static_assert(PER == 4 || PER == 8, "bins per thread");
  const uint32_t t = threadIdx.x;
  uint32_t c[PER];
#pragma unroll
  for (int j = 0; j < PER; j += 4) {
    const uint4 q = reinterpret_cast<const uint4*>(hist)[(t * PER + j) >> 2];
    c[j] = q.x; c[j + 1] = q.y; c[j + 2] = q.z; c[j + 3] = q.w;
  }
  uint32_t sum = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) sum += c[j];
  const uint32_t incl = wave_incl_scan(sum);
  if ((t & 63u) == 63u) s_w[t >> 6] = incl;
  if (t == 0) { s_res[0] = 0u; s_res[1] = 0u; }
  __syncthreads();
  uint32_t excl = incl - sum;
  for (uint32_t w = 0; w < (t >> 6); ++w) excl += s_w[w];
  if (rank >= excl && rank - excl < sum) {                 // exactly one thread
    uint32_t r = rank - excl, d = 0;
    bool found = false;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      if (!found) {
        if (r < c[j]) { d = (uint32_t)j; found = true; } else r -= c[j];
      }
    }
    s_res[0] = t * PER + d; s_res[1] = r;
  }
  __syncthreads();
  digit = s_res[0]; rank_in = s_res[1];
  __syncthreads();
}

template <int PASS>
__global__ __launch_bounds__(256) void lower_median_pass(MedianSource src, uint32_t n, MedianScratch* __restrict__ ms) {
  constexpr int BINS = PASS == 2 ? 1024 : 2048;
  __shared__ uint32_t lh[BINS];
  __shared__ uint32_t s_w[4], s_res[2], s_nan;
  const uint32_t t = threadIdx.x;
  for (uint32_t i = t; i < (uint32_t)BINS; i += 256u) lh[i] = 0u;
  if (t == 0) s_nan = 0u;
  uint32_t prefix = 0;
  if (PASS == 1) {
    uint32_t d, r;
    find_bucket<2048>(ms->hist0, (n - 1u) >> 1, s_w, s_res, d, r);          // rank (n - 1) // 2: the LOWER median
    prefix = d;
    if (blockIdx.x == 0 && t == 0) { ms->digit0 = d; ms->rank1 = r; }
  } else if (PASS == 2) {
    uint32_t d, r;
    find_bucket<2048>(ms->hist1, ms->rank1, s_w, s_res, d, r);
    prefix = (ms->digit0 << 11) | d;
    if (blockIdx.x == 0 && t == 0) { ms->prefix2 = prefix; ms->rank2 = r; }
  }
  __syncthreads();
  uint32_t nans = 0;
  for (uint64_t base = (uint64_t)blockIdx.x * kMedianChunk; base < n; base += (uint64_t)gridDim.x * kMedianChunk) {
#pragma unroll 4
    for (uint32_t j = 0; j < kMedianChunk / 256u; ++j) {
      const uint64_t i = base + j * 256u + t;
      if (i < n) {
        const float v = median_load(src, i);
        const uint32_t key = median_key(v);
        if (PASS == 0) {
          nans += (v != v) ? 1u : 0u;
          atomicAdd(&lh[key >> 21], 1u);
        } else if (PASS == 1) {
          if ((key >> 21) == prefix) atomicAdd(&lh[(key >> 10) & 2047u], 1u);
        } else {
          if ((key >> 10) == prefix) atomicAdd(&lh[key & 1023u], 1u);
        }
      }
    }
  }
  if (PASS == 0 && nans) atomicAdd(&s_nan, nans);
  __syncthreads();
  uint32_t* __restrict__ gh = PASS == 0 ? ms->hist0 : PASS == 1 ? ms->hist1 : ms->hist2;
  for (uint32_t i = t; i < (uint32_t)BINS; i += 256u) {
    const uint32_t c = lh[i];
    if (c) atomicAdd(&gh[i], c);
  }
  if (PASS == 0 && t == 0 && s_nan) atomicAdd(&ms->nan_count, s_nan);
}
template __global__ decltype(lower_median_pass<0>) lower_median_pass<0>;
template __global__ decltype(lower_median_pass<1>) lower_median_pass<1>;
template __global__ decltype(lower_median_pass<2>) lower_median_pass<2>;

// the last step of the select, by a whole workgroup: NaN for n = 0 (nothing is read then) or with a NaN among the values
__device__ __forceinline__ float median_finish(uint32_t n, const MedianScratch* __restrict__ ms, uint32_t* s_w, uint32_t* s_res,
                                               uint32_t& nan_count) {
  nan_count = 0u;
  if (n == 0u) return __uint_as_float(0x7FC00000u);
  uint32_t d, r;
  find_bucket<1024>(ms->hist2, ms->rank2, s_w, s_res, d, r);
  nan_count = ms->nan_count;
  return nan_count ? __uint_as_float(0x7FC00000u) : median_value((ms->prefix2 << 10) | d);
}

__global__ __launch_bounds__(256) void lower_median_finish(uint32_t n, MedianScratch* __restrict__ ms, float* __restrict__ out_median,
                                                           uint32_t* __restrict__ out_nan_count) {
  __shared__ uint32_t s_w[4], s_res[2];
  uint32_t nan_count;
  const float m = median_finish(n, ms, s_w, s_res, nan_count);
  if (threadIdx.x == 0) {
    *out_median = m;
    if (out_nan_count) *out_nan_count = nan_count;
  }
}

// ---- densification ---------------------------------------------------------------------------------------------------------
// non_presence_mask of the reference (:748-756) at original-resolution pixel p; `thr` = 50 * median (NaN: never exceeded)
__device__ __forceinline__ bool ori_unexplained(const DensifyArgs& a, int p, float thr) {
  if (!a.depth_sil) return true;                                    // seed mode: every pixel
  const float gd = a.gt_depth[p], rd = a.depth_sil[p], sil = a.depth_sil[(size_t)a.W * a.H + p];
  return (sil < a.sil_thres) | ((rd > gd) & (depth_error(gd, rd) > thr));
}
// valid_depth & mask_variation[nearest] & non_presence_mask[nearest] (:775-788); nearest = integer division by the ratio
__device__ __forceinline__ bool dense_selected(const DensifyArgs& a, int pd, float thr) {
  if (!(a.gt_depth_d[pd] > 0.f)) return false;
  const int xd = pd % a.dW, yd = pd / a.dW;
  if (a.mask && !a.mask[(size_t)(yd / a.mry) * a.mW + xd / a.mrx]) return false;
  return ori_unexplained(a, (yd / a.ry) * a.W + xd / a.rx, thr);
}

__global__ __launch_bounds__(256) void densify_count(DensifyArgs a) {
  __shared__ uint32_t s_w[4], s_res[2], s_cnt[4], s_un[4];
  const uint32_t t = threadIdx.x;
  float thr = __uint_as_float(0x7FC00000u);
  if (a.depth_sil) {
    uint32_t nan_count;
    const float med = median_finish((uint32_t)(a.W * a.H), a.ms, s_w, s_res, nan_count);
    thr = 50.f * med;
    if (blockIdx.x == 0 && t == 0) a.ms->median = med;
  }
  const bool dense = blockIdx.x >= a.blocks_ori;
  const uint32_t chunk = dense ? blockIdx.x - a.blocks_ori : blockIdx.x;
  const uint32_t P = dense ? (uint32_t)(a.dW * a.dH) : (uint32_t)(a.W * a.H);
  uint32_t cnt = 0, un = 0;
#pragma unroll
  for (uint32_t s = 0; s < kDensifyChunk / 256u; ++s) {
    const uint32_t p = chunk * kDensifyChunk + s * 256u + t;
    bool sel = false, u = false;
    if (p < P) {
      if (dense) sel = dense_selected(a, (int)p, thr);
      else { u = ori_unexplained(a, (int)p, thr); sel = u && a.gt_depth[p] > 0.f; }
    }
    cnt += (uint32_t)__popcll(__ballot(sel));
    un += (uint32_t)__popcll(__ballot(u));
  }
  if ((t & 63u) == 0u) { s_cnt[t >> 6] = cnt; s_un[t >> 6] = un; }
  __syncthreads();
  if (t == 0) {
    a.counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    if (!dense) a.unexplained[blockIdx.x] = s_un[0] + s_un[1] + s_un[2] + s_un[3];
  }
}

__global__ __launch_bounds__(256) void densify_emit(DensifyArgs a) {
  constexpr uint32_t kSteps = kDensifyChunk / 256u;
  __shared__ uint32_t s_red[4][4], s_slot[kSteps * 4];
  const uint32_t t = threadIdx.x, w = t >> 6, b = blockIdx.x, G = a.blocks_ori + a.blocks_dense;
  // the counts in front of this chunk, all of them, those of the original image; workgroup 0 also the non-presence pixels
  uint32_t before = 0, total = 0, ori = 0, un = 0;
  for (uint32_t i = t; i < G; i += 256u) {
    const uint32_t c = a.counts[i];
    total += c;
    before += i < b ? c : 0u;
    ori += i < a.blocks_ori ? c : 0u;
  }
  if (b == 0) for (uint32_t i = t; i < a.blocks_ori; i += 256u) un += a.unexplained[i];
  for (int m = 1; m < 64; m <<= 1) {
    before += (uint32_t)__shfl_xor((int)before, m, 64);
    total += (uint32_t)__shfl_xor((int)total, m, 64);
    ori += (uint32_t)__shfl_xor((int)ori, m, 64);
    un += (uint32_t)__shfl_xor((int)un, m, 64);
  }
  if ((t & 63u) == 0u) { s_red[w][0] = before; s_red[w][1] = total; s_red[w][2] = ori; s_red[w][3] = un; }
  __syncthreads();
  before = s_red[0][0] + s_red[1][0] + s_red[2][0] + s_red[3][0];
  total = s_red[0][1] + s_red[1][1] + s_red[2][1] + s_red[3][1];
  ori = s_red[0][2] + s_red[1][2] + s_red[2][2] + s_red[3][2];
  un = s_red[0][3] + s_red[1][3] + s_red[2][3] + s_red[3][3];
  const bool overflow = (unsigned long long)a.n + total > (unsigned long long)a.capacity;
  const float nanf_ = __uint_as_float(0x7FC00000u);
  if (b == 0 && t == 0) {
    VtgsDensifyInfo* info = a.info;
    info->added_ori = ori; info->added_dense = total - ori; info->unexplained = un; info->overflow = overflow ? 1u : 0u;
    info->median = a.depth_sil ? a.ms->median : nanf_;
    info->nan_count = a.depth_sil ? a.ms->nan_count : 0u;
    info->pad = 0u;
    __threadfence_system();
    info->complete = 1u;                       // last: a host that polls a device-mapped record reads the rest after this
  }
  if (overflow || a.counts[b] == 0u) return;   // (workgroup-uniform)
  const float thr = a.depth_sil ? 50.f * a.ms->median : nanf_;
  const bool dense = b >= a.blocks_ori;
  const uint32_t chunk = dense ? b - a.blocks_ori : b;
  const int Wp = dense ? a.dW : a.W, Hp = dense ? a.dH : a.H;
  const uint32_t P = (uint32_t)(Wp * Hp);
  bool sel[kSteps];
#pragma unroll
  for (uint32_t s = 0; s < kSteps; ++s) {
    const uint32_t p = chunk * kDensifyChunk + s * 256u + t;
    sel[s] = false;
    if (p < P) sel[s] = dense ? dense_selected(a, (int)p, thr) : (ori_unexplained(a, (int)p, thr) && a.gt_depth[p] > 0.f);
    const unsigned long long m = __ballot(sel[s]);
    if ((t & 63u) == 0u) s_slot[s * 4u + w] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  // camera: get_pointcloud's intrinsics and the rigid inverse of w2c (R^T (p - t))
  const float* __restrict__ K = dense ? a.k_d : a.k;
  const float fx = K[0], fy = K[4], cx = K[2], cy = K[5];
  float R[9], T[3];
  if (a.w2c) {
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = a.w2c[4 * (i / 3) + i % 3];
    T[0] = a.w2c[3]; T[1] = a.w2c[7]; T[2] = a.w2c[11];
  } else {                                     // column t of the camera tensors, as vtgs_prepare_frame_slot reads it
    const float qs[4] = {a.cam_rots[a.t], a.cam_rots[a.frames + a.t], a.cam_rots[2 * a.frames + a.t], a.cam_rots[3 * a.frames + a.t]};
    const float ts[3] = {a.cam_trans[a.t], a.cam_trans[a.frames + a.t], a.cam_trans[2 * a.frames + a.t]};
    const float none[16] = {0.f};
    const FramePose Pz = load_pose(qs, ts, none);
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = Pz.R[i];
    T[0] = Pz.t[0]; T[1] = Pz.t[1]; T[2] = Pz.t[2];
  }
  const float* __restrict__ im = dense ? a.gt_im_d : a.gt_im;
  const float* __restrict__ gdp = dense ? a.gt_depth_d : a.gt_depth;
  const float fmean = (fx + fy) / 2.f;
#pragma unroll
  for (uint32_t s = 0; s < kSteps; ++s) {
    uint32_t row = (uint32_t)a.n + before;
    for (uint32_t q = 0; q < s * 4u + w; ++q) row += s_slot[q];          // the wavefronts of this chunk in pixel order
    const unsigned long long m = __ballot(sel[s]);
    if (!sel[s]) continue;
    row += (uint32_t)__popcll(m & ((1ull << (t & 63u)) - 1ull));
    if (row >= (uint32_t)a.capacity) continue;                           // (cannot happen: n + total <= capacity)
    const uint32_t p = chunk * kDensifyChunk + s * 256u + t;
    const int x = (int)(p % (uint32_t)Wp), y = (int)(p / (uint32_t)Wp);
    const float z = gdp[p] * 1.005f;                                      // get_pointcloud, factor 1.005
    const float pcx = ((float)x - cx + 0.5f) / fx * z, pcy = ((float)y - cy + 0.5f) / fy * z;
    const float dx = pcx - T[0], dy = pcy - T[1], dz = z - T[2];
    const size_t r = row;
    a.means3D[3 * r] = fmaf(R[6], dz, fmaf(R[3], dy, R[0] * dx));
    a.means3D[3 * r + 1] = fmaf(R[7], dz, fmaf(R[4], dy, R[1] * dx));
    a.means3D[3 * r + 2] = fmaf(R[8], dz, fmaf(R[5], dy, R[2] * dx));
    a.rgb[3 * r] = im[p]; a.rgb[3 * r + 1] = im[(size_t)P + p]; a.rgb[3 * r + 2] = im[2 * (size_t)P + p];
    a.rot[4 * r] = 1.f; a.rot[4 * r + 1] = 0.f; a.rot[4 * r + 2] = 0.f; a.rot[4 * r + 3] = 0.f;
    a.opac[r] = 0.f;
    const float ls = logf(z / fmean);                                     // log sqrt(mean3_sq_dist), mean3_sq_dist = (z / f)^2
    for (int c = 0; c < a.scale_columns; ++c) a.log_scales[(size_t)a.scale_columns * r + c] = ls;
    if (a.timestep) a.timestep[r] = a.time_value;
  }
}

}  // namespace vtgs
