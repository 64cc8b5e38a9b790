// A guarded Adam step (include/crw_hip_guard.h): crw_adam_step's update behind a decision that the device makes -- refuse the step
// when the gradient holds a NaN or an infinity, scale the gradient when its norm exceeds max_norm -- without a host synchronisation.
// Three launches on the caller's stream:
//   1. guard_partial_kernel   block b: the fp64 sum of squares of g[b * 4096 .. (b + 1) * 4096) -> ws[b]          (reads g once)
//   2. guard_decide_kernel    ONE workgroup: joins the partials, decides, updates ctl, writes the decision record behind the partials
//   3. guard_update_kernel    adam_kernel of optim.hip on fl32(g * c) with the record's coefficients; returns at once when refused
// The decision is a kernel boundary away from its readers, so every workgroup of launch 3 sees the same one and no workgroup waits
// for another inside a launch.  The sums have a fixed order (no atomics): the same call gives the same bits.
// The update's arithmetic is adam_kernel's, expression for expression (tests/test_guard_gpu.py holds the two bit for bit); the scaled
// gradient is rounded on its own (scaled_grad), so that no contraction fuses the scaling into the moment updates.
// One route: there is no selector, so the route log has no name for it.
#include "crw_common.h"
#include "crw_hip_guard.h"

namespace crw {
namespace {

constexpr int GUARD_NT = 256;
constexpr int GUARD_F4 = CRW_GUARD_BLOCK_ELEMS / (4 * GUARD_NT);  // float4 per thread of a block's 4096 elements
static_assert(GUARD_F4 * 4 * GUARD_NT == CRW_GUARD_BLOCK_ELEMS, "a block's elements are whole float4 rounds");

struct GuardCtl {  // include/crw_hip_guard.h fixes the layout
  long long applied, skipped;
  double norm;
  float scale;
  int last_applied;
  char reserved[32];
};
static_assert(sizeof(GuardCtl) == CRW_GUARD_CTL_BYTES, "ctl is 64 bytes");

struct GuardDecision {  // behind the partials in ws; written by guard_decide_kernel, read by every thread of guard_update_kernel
  int apply;
  float c, neg_step, bc2_sqrt;
};

// the 256 accumulators of a workgroup, joined by halving: s[t] += s[t + h], h = 128 .. 1 -> s[0]
__device__ inline double tree_sum(double acc, double *s) {
  const int t = threadIdx.x;
  s[t] = acc;
  __syncthreads();
  for (int h = GUARD_NT / 2; h > 0; h >>= 1) {
    if (t < h) s[t] += s[t + h];
    __syncthreads();
  }
  return s[0];
}

__global__ __launch_bounds__(GUARD_NT) void guard_partial_kernel(const float *__restrict__ g, long n, double *__restrict__ part) {
  __shared__ double s[GUARD_NT];
  const long base = (long)blockIdx.x * CRW_GUARD_BLOCK_ELEMS;
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < GUARD_F4; ++j) {
    const long i = base + ((long)j * GUARD_NT + threadIdx.x) * 4;
    if (i + 4 <= n) {
      const float4 gv = *reinterpret_cast<const float4 *>(g + i);
      acc += (double)gv.x * (double)gv.x;
      acc += (double)gv.y * (double)gv.y;
      acc += (double)gv.z * (double)gv.z;
      acc += (double)gv.w * (double)gv.w;
    } else {
      for (long k = i; k < n; ++k) acc += (double)g[k] * (double)g[k];
    }
  }
  const double sum = tree_sum(acc, s);
  if (threadIdx.x == 0) part[blockIdx.x] = sum;
}

__global__ __launch_bounds__(GUARD_NT) void guard_decide_kernel(const double *__restrict__ part, long nblocks, GuardCtl *ctl,
                                                                GuardDecision *dec, int step, float max_norm, float lr,
                                                                float beta1, float beta2, float host_neg_step, float host_bc2_sqrt) {
  __shared__ double s[GUARD_NT];
  double acc = 0.0;
  for (long b = threadIdx.x; b < nblocks; b += GUARD_NT) acc += part[b];
  const double ss = tree_sum(acc, s);
  if (threadIdx.x != 0) return;
  const double norm = sqrt(ss);
  GuardDecision d;
  if (!isfinite(ss)) {
    ctl->skipped += 1;
    ctl->last_applied = 0;
    ctl->norm = norm;
    ctl->scale = 0.f;
    d.apply = 0;
    d.c = 0.f;
    d.neg_step = 0.f;
    d.bc2_sqrt = 1.f;
  } else {
    const long long skipped = ctl->skipped;
    float c = 1.f;
    if (max_norm > 0.f && max_norm < INFINITY) c = (float)fmin(1.0, (double)max_norm / (norm + 1e-6));
    d.apply = 1;
    d.c = c;
    if (skipped == 0) {  // crw_adam_step's own coefficients: the outputs are its bits
      d.neg_step = host_neg_step;
      d.bc2_sqrt = host_bc2_sqrt;
    } else {
      const long long t = (long long)step - skipped > 0 ? (long long)step - skipped : 1;
      const double bc1 = 1.0 - pow((double)beta1, (double)t), bc2 = 1.0 - pow((double)beta2, (double)t);
      d.neg_step = (float)(-(double)lr / bc1);
      d.bc2_sqrt = (float)sqrt(bc2);
    }
    ctl->applied += 1;
    ctl->last_applied = 1;
    ctl->norm = norm;
    ctl->scale = c;
  }
  *dec = d;
}

// g' = fl32(g * c): a product of its own.  The pragma keeps the compiler from fusing it into the subtraction and the products that
// consume it (device code is compiled with contraction on, and __fmul_rn is a plain product to it).
__device__ inline float scaled_grad(float g, float c) {
#pragma clang fp contract(off)
  return g * c;
}

__global__ __launch_bounds__(256) void guard_update_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                                                           float *__restrict__ v, long n, float w1, float b2, float w2, float eps,
                                                           const GuardDecision *__restrict__ dec) {
  const GuardDecision d = *dec;
  if (!d.apply) return;
  const float c = d.c, neg_step = d.neg_step, bc2_sqrt = d.bc2_sqrt;
  const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;
  auto one = [&](float &pp, float graw, float &mm, float &vv) {
    const float gg = scaled_grad(graw, c);
    mm = mm + w1 * (gg - mm);
    vv = vv * b2 + (w2 * gg) * gg;
    const float denom = sqrtf(vv) / bc2_sqrt + eps;
    pp = pp + neg_step * (mm / denom);
  };
  if (i + 4 <= n) {
    float4 pv = *reinterpret_cast<float4 *>(p + i), mv = *reinterpret_cast<float4 *>(m + i), vv = *reinterpret_cast<float4 *>(v + i);
    const float4 gv = *reinterpret_cast<const float4 *>(g + i);
    one(pv.x, gv.x, mv.x, vv.x);
    one(pv.y, gv.y, mv.y, vv.y);
    one(pv.z, gv.z, mv.z, vv.z);
    one(pv.w, gv.w, mv.w, vv.w);
    *reinterpret_cast<float4 *>(p + i) = pv;
    *reinterpret_cast<float4 *>(m + i) = mv;
    *reinterpret_cast<float4 *>(v + i) = vv;
  } else {
    for (long k = i; k < n; ++k) one(p[k], g[k], m[k], v[k]);
  }
}

inline long guard_blocks(long n) { return (n + CRW_GUARD_BLOCK_ELEMS - 1) / CRW_GUARD_BLOCK_ELEMS; }

}  // namespace
}  // namespace crw

extern "C" size_t crw_adam_guard_ws_bytes(long n) {
  return (n < 1 ? 0 : (size_t)crw::guard_blocks(n) * sizeof(double)) + sizeof(crw::GuardDecision);
}

extern "C" int crw_adam_step_guarded(float *p, const float *g, float *m, float *v, long n, float lr, float beta1, float beta2, float eps,
                                     int step, float max_norm, void *ctl, void *ws, size_t ws_bytes, crw_stream_t stream) {
  crw::clear_stale_error();
  if (!p || !g || !m || !v || n < 1 || step < 1 || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) ||
      (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15))
    return CRW_EINVAL;
  if (!(max_norm >= 0.f) || !ctl || !ws || (((uintptr_t)ctl | (uintptr_t)ws) & 7)) return CRW_EINVAL;
  const long nblocks = crw::guard_blocks(n);
  if (nblocks > 0x7fffffffL) return CRW_EINVAL;
  if (ws_bytes < crw_adam_guard_ws_bytes(n)) return CRW_EWORKSPACE;
  // the bias corrections of crw_adam_step for `step`: in double like the host code of torch.optim, then rounded once
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  const float neg_step = (float)(-(double)lr / bc1), bc2_sqrt = (float)sqrt(bc2);
  double *part = static_cast<double *>(ws);
  crw::GuardDecision *dec = reinterpret_cast<crw::GuardDecision *>(part + nblocks);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(crw::guard_partial_kernel, dim3((unsigned)nblocks), dim3(crw::GUARD_NT), 0, s, g, n, part);
  hipLaunchKernelGGL(crw::guard_decide_kernel, dim3(1), dim3(crw::GUARD_NT), 0, s, part, nblocks, static_cast<crw::GuardCtl *>(ctl), dec,
                     step, max_norm, lr, beta1, beta2, neg_step, bc2_sqrt);
  const long nthread = (n + 3) / 4;
  hipLaunchKernelGGL(crw::guard_update_kernel, dim3((unsigned)((nthread + 255) / 256)), dim3(256), 0, s, p, g, m, v, n, 1.0f - beta1,
                     beta2, 1.0f - beta2, eps, dec);
  return crw::check_launch();
}
