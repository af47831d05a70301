// vtgs_adam.hip -- Adam over up to 8 tensors in one launch (src/vtgaussian_slam.py:180-187), whole tensors or listed rows.
#include "../../include/vtgs.h"
#include "vtgs_host.h"
#include "vtgs_internal.h"

namespace vtgs {

struct AdamLaunch {
  VtgsAdamGroup g[VTGS_ADAM_MAX_GROUPS];
  float step_size_scale;   // 1 / (1 - b1^step)
  float sqrt_bias2;        // sqrt(1 - b2^step)
  float beta1, beta2;
};

// one element of the update; the multiply-adds are spelled out (and contraction is off) so that the float4 form, the scalar
// tail and the row-list kernel produce the same bits whatever the compiler would fuse in each of them
__device__ __forceinline__ void adam_element(const AdamLaunch& a, const VtgsAdamGroup& g, float gr, float& m, float& v, float& p) {
#pragma clang fp contract(off)
  m = fmaf(1.f - a.beta1, gr - m, m);                                 // lerp, like torch
  v = fmaf(a.beta2, v, ((1.f - a.beta2) * gr) * gr);
  const float denom = sqrtf(v) / a.sqrt_bias2 + g.eps;
  p = fmaf(-(g.lr * a.step_size_scale), m / denom, p);
}
// the N elements at i: N = 4 as float4, N = 1 one float
template <int N>
__device__ __forceinline__ void adam_elements(const AdamLaunch& a, const VtgsAdamGroup& g, size_t i) {
  const Px<N> gr = Px<N>::load(g.grad + i);
  Px<N> m = Px<N>::load(g.exp_avg + i), v = Px<N>::load(g.exp_avg_sq + i), p = Px<N>::load(g.param + i);
#pragma unroll
  for (int k = 0; k < N; ++k) adam_element(a, g, gr[k], m[k], v[k], p[k]);
  m.store(g.exp_avg + i); v.store(g.exp_avg_sq + i); p.store(g.param + i);
}
// four elements per thread as float4 when the group's four arrays are 16-byte aligned (every torch allocation and the
// padded segments of the fused nodes' gradient blocks are): the one-float form ran at ~3 TB/s (27 us for the five trainable
// floats of 1 M Gaussians); same arithmetic per element
__global__ __launch_bounds__(256) void adam_step_kernel(AdamLaunch a) {
  const VtgsAdamGroup& g = a.g[blockIdx.y];
  const size_t i = ((size_t)blockIdx.x * 256u + threadIdx.x) * 4u;
  if (i >= g.count) return;
  if (all_aligned16(g.param, g.grad, g.exp_avg, g.exp_avg_sq) && i + 4u <= g.count) { adam_elements<4>(a, g, i); return; }
  for (size_t j = i; j < g.count && j < i + 4u; ++j) adam_elements<1>(a, g, j);
}

struct AdamRows { const int32_t* rows; int32_t n_rows; uint32_t width[VTGS_ADAM_MAX_GROUPS]; };
__global__ __launch_bounds__(256) void adam_step_rows_kernel(AdamLaunch a, AdamRows r) {
  const VtgsAdamGroup& g = a.g[blockIdx.y];
  const uint32_t w = r.width[blockIdx.y];
  const size_t j = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (w == 0u || j >= (size_t)r.n_rows * w) return;
  adam_elements<1>(a, g, (size_t)r.rows[j / w] * w + (j % w));
}

// What both entry points do before their launch: argument checks, the groups (null beyond n_groups), the bias corrections and
// `longest`, the most work items of one group -- its count, or for listed rows n_rows * (count / n_total_rows); 0 = no launch.
static int adam_fill(AdamLaunch& a, uint64_t& longest, const VtgsAdamGroup* groups, int32_t n_groups, int32_t step, float beta1,
                     float beta2, uint64_t n_total_rows = 1, uint64_t n_rows = 1) {
  longest = 0;
  if (!groups || n_groups <= 0 || n_groups > VTGS_ADAM_MAX_GROUPS || step <= 0 || !(beta1 >= 0.f && beta1 < 1.f) ||
      !(beta2 >= 0.f && beta2 < 1.f))
    return VTGS_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < VTGS_ADAM_MAX_GROUPS; ++k) {
    a.g[k] = k < n_groups ? groups[k] : VtgsAdamGroup{nullptr, nullptr, nullptr, nullptr, 0, 0.f, 0.f};
    if (a.g[k].count && (!a.g[k].param || !a.g[k].grad || !a.g[k].exp_avg || !a.g[k].exp_avg_sq)) return VTGS_ERR_INVALID_ARGUMENT;
    const uint64_t work = a.g[k].count / n_total_rows * n_rows;
    longest = work > longest ? work : longest;
  }
  if (longest > (uint64_t)0x7fffffff * 256u) return VTGS_ERR_INVALID_ARGUMENT;
  a.step_size_scale = (float)(1.0 / (1.0 - pow((double)beta1, (double)step)));   // lr / bias_correction1
  a.sqrt_bias2 = (float)sqrt(1.0 - pow((double)beta2, (double)step));
  a.beta1 = beta1;
  a.beta2 = beta2;
  return VTGS_OK;
}

}  // namespace vtgs

using namespace vtgs;

extern "C" {

int vtgs_adam_step(const VtgsAdamGroup* groups, int32_t n_groups, int32_t step, float beta1, float beta2, void* stream) {
  AdamLaunch a;
  uint64_t longest;
  const int rc = adam_fill(a, longest, groups, n_groups, step, beta1, beta2);
  if (rc != VTGS_OK || longest == 0) return rc;
  hipLaunchKernelGGL(adam_step_kernel, dim3((uint32_t)((longest + 1023) / 1024), (uint32_t)n_groups), dim3(256), 0,
                     (hipStream_t)stream, a);
  return launch_status(__func__);
}

int vtgs_adam_step_rows(const VtgsAdamGroup* groups, int32_t n_groups, int32_t step, float beta1, float beta2,
                        const int32_t* rows, int32_t n_rows, int32_t n_total_rows, void* stream) {
  if (n_rows < 0 || n_total_rows <= 0 || (n_rows > 0 && !rows)) return VTGS_ERR_INVALID_ARGUMENT;
  AdamLaunch a;
  uint64_t longest;
  const int rc = adam_fill(a, longest, groups, n_groups, step, beta1, beta2, (uint64_t)n_total_rows, (uint64_t)n_rows);
  if (rc != VTGS_OK) return rc;
  AdamRows r;
  r.rows = rows; r.n_rows = n_rows;
  for (int k = 0; k < VTGS_ADAM_MAX_GROUPS; ++k) {
    if (a.g[k].count % (uint64_t)n_total_rows) return VTGS_ERR_INVALID_ARGUMENT;
    r.width[k] = (uint32_t)(a.g[k].count / (uint64_t)n_total_rows);
  }
  if (longest == 0) return VTGS_OK;
  hipLaunchKernelGGL(adam_step_rows_kernel, dim3((uint32_t)((longest + 255) / 256), (uint32_t)n_groups), dim3(256), 0,
                     (hipStream_t)stream, a, r);
  return launch_status(__func__);
}

}  // extern "C"
