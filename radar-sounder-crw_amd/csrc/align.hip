// Segment-centred normalisation (include/crw_hip_align.h): crw_center_normalize.
//
// Launch 1 (center_partial_kernel): workgroup (j, s) sums the rows of slab j that lie in segment s, per channel, in fp64 -- thread
// (rsub, c) takes rows lo + rsub, lo + rsub + RS, ... in order, the RS sub-sums are joined through LDS in the order 0 .. RS - 1 --
// and writes partial[s][j][c] (zeros where the slab and the segment do not meet: every entry is written, so what the workspace
// held does not matter).
// Launch 2 (center_normalize_kernel): a workgroup owns CN_ROWS consecutive rows.  For every segment its rows touch it joins that
// segment's partials in fp64 into LDS by the same scheme -- thread (g, c) takes slabs g, g + G, ... in order, the G sub-sums are
// joined in the order 0 .. G - 1 --, divides by the row count, and its four waves then do what normalize_kernel (walk.hip) does on
// y = fp32(x - mean): the same loop order, the same wave reduction, the same division.
// The order of every sum is a function of (rows, C) and the offsets alone, and every workgroup that needs a mean computes the same
// bits from the same partials: nothing is exchanged and nothing is atomic.
// Both sums keep SUM_BATCH loads in flight and then add them in order: a loop of load-then-add pays one memory round trip per term.
#include "crw_common.h"
#include "crw_hip_align.h"

namespace crw {
namespace {

constexpr float EPS_NORM = 1e-12f;  // F.normalize default eps (walk.hip)
constexpr int CP_NT = 512, CP_MAX_SLABS = 64, CP_MIN_SLAB_ROWS = 32;
constexpr int CN_NT = 256, CN_ROWS = 64;
constexpr int SUM_BATCH = 8;

// sum of src[i * stride], i = first, first + step, ... < end, in that order, in fp64
template <class T>
__device__ __forceinline__ double ordered_sum(const T *src, long stride, int first, int step, int end) {
  double acc = 0.0;
  for (int i = first; i < end; i += SUM_BATCH * step) {
    double v[SUM_BATCH];
#pragma unroll
    for (int u = 0; u < SUM_BATCH; ++u) {
      const int k = i + u * step;
      v[u] = k < end ? (double)src[(long)k * stride] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < SUM_BATCH; ++u)
      if (i + u * step < end) acc += v[u];
  }
  return acc;
}

struct SegVals {
  int32_t b[CRW_ALIGN_MAX_BY_VALUE + 1];
};

// b_s, s in 0 .. S, whatever the device array holds: b_0 = 0, b_S = rows, monotone in between
__device__ inline int seg_bound(const int32_t *dev, const SegVals &v, int S, int rows, int s) {
  if (s <= 0) return 0;
  if (s >= S) return rows;
  if (!dev) return v.b[s];  // checked on the host
  int b = 0;
  for (int i = 1; i <= s; ++i) b = min(rows, max(b, dev[i]));
  return b;
}

inline int slab_count(int rows) { return min(CP_MAX_SLABS, (rows + CP_MIN_SLAB_ROWS - 1) / CP_MIN_SLAB_ROWS); }
inline int slab_rows(int rows) { const int n = slab_count(rows); return (rows + n - 1) / n; }

// CW: channels side by side (a power of two, <= CP_NT); RS = CP_NT / CW row sub-sequences
__global__ __launch_bounds__(CP_NT) void center_partial_kernel(const float *emb, int rows, int C, const int32_t *seg_dev, SegVals segv,
                                                               int S, int nslab, int srows, int cw, double *partial) {
  __shared__ double sub[CP_NT];
  const int j = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
  const int lo = max(seg_bound(seg_dev, segv, S, rows, s), j * srows);
  const int hi = min(seg_bound(seg_dev, segv, S, rows, s + 1), min(rows, (j + 1) * srows));
  const int rs = CP_NT / cw, cc = tid % cw, rsub = tid / cw;
  double *out = partial + ((long)s * nslab + j) * C;
  for (int c0 = 0; c0 < C; c0 += cw) {  // (block-uniform)
    const int c = c0 + cc;
    sub[tid] = c < C ? ordered_sum(emb + c, C, lo + rsub, rs, hi) : 0.0;
    __syncthreads();
    if (rsub == 0 && c < C) {
      double t = sub[cc];
      for (int u = 1; u < rs; ++u) t += sub[u * cw + cc];
      out[c] = t;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(CN_NT) void center_normalize_kernel(const float *emb, int rows, int C, const int32_t *seg_dev, SegVals segv,
                                                                 int S, int nslab, int cw, const double *partial, float *ehat, double *mean) {
  extern __shared__ __attribute__((aligned(16))) double mu[];  // [C]
  __shared__ double sub[CN_NT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = blockIdx.x * CN_ROWS, r1 = min(rows, r0 + CN_ROWS);
  if (mean && blockIdx.x == 0)  // an empty segment has no workgroup of its own: its row of `mean` is +0
    for (int s = 0; s < S; ++s)
      if (seg_bound(seg_dev, segv, S, rows, s) == seg_bound(seg_dev, segv, S, rows, s + 1))
        for (int c = tid; c < C; c += CN_NT) mean[(long)s * C + c] = 0.0;
  int s = 0;
  for (int row = r0; row < r1;) {  // (block-uniform: one pass per segment the rows touch)
    while (seg_bound(seg_dev, segv, S, rows, s + 1) <= row) ++s;  // ends: b_S = rows > row
    const int lo = seg_bound(seg_dev, segv, S, rows, s), hi = seg_bound(seg_dev, segv, S, rows, s + 1);
    const int end = min(r1, hi);
    const int ng = CN_NT / cw, cc = tid % cw, grp = tid / cw;  // cw channels side by side, ng slab sub-sequences
    for (int c0 = 0; c0 < C; c0 += cw) {                       // (block-uniform)
      const int c = c0 + cc;
      sub[tid] = c < C ? ordered_sum(partial + (long)s * nslab * C + c, C, grp, ng, nslab) : 0.0;
      __syncthreads();
      if (grp == 0 && c < C) {
        double t = sub[cc];
        for (int u = 1; u < ng; ++u) t += sub[u * cw + cc];
        t /= (double)(hi - lo);
        mu[c] = t;
        if (mean && row == lo) mean[(long)s * C + c] = t;  // the workgroup that holds the segment's first row
      }
      __syncthreads();
    }
    for (long r = row + wave; r < end; r += CN_NT / 64) {
      const float *x = emb + r * C;
      float ss = 0.f;
      for (int c = lane; c < C; c += 64) {
        const float y = (float)((double)x[c] - mu[c]);
        ss += y * y;
      }
      ss = wave_sum(ss);
      const float d = fmaxf(sqrtf(ss), EPS_NORM);
      for (int c = lane; c < C; c += 64) {
        const float y = (float)((double)x[c] - mu[c]);
        ehat[r * C + c] = y / d;
      }
    }
    __syncthreads();
    row = end;
  }
}

inline double *ws_doubles(void *ws) { return reinterpret_cast<double *>(((uintptr_t)ws + 7) & ~(uintptr_t)7); }

}  // namespace
}  // namespace crw

using namespace crw;

extern "C" {

size_t crw_center_normalize_ws_bytes(int rows, int C, int S) {
  if (rows < 1 || C < 1 || S < 1) return 8;
  return (size_t)S * slab_count(rows) * C * sizeof(double) + 8;  // + 8: the partials start at the next multiple of 8
}

int crw_center_normalize(const float *emb, int rows, int C, const int32_t *seg_dev, const int32_t *seg_host, int S, void *ws,
                         size_t ws_bytes, float *ehat, double *mean, crw_stream_t stream) {
  crw::clear_stale_error();
  if (!emb || !ehat || !ws || rows < 1 || C < 1 || C > CRW_ALIGN_MAX_CHANNELS || S < 1 || (seg_dev != nullptr) == (seg_host != nullptr) ||
      (((uintptr_t)mean) & 7))
    return CRW_EINVAL;
  if (S > (seg_host ? CRW_ALIGN_MAX_BY_VALUE : CRW_ALIGN_MAX_SEGMENTS)) return CRW_EINVAL;
  SegVals segv = {};
  if (seg_host) {
    if (seg_host[0] != 0 || seg_host[S] != rows) return CRW_EINVAL;
    for (int s = 0; s <= S; ++s) {
      if (s && seg_host[s] < seg_host[s - 1]) return CRW_EINVAL;
      segv.b[s] = seg_host[s];
    }
  }
  if (ws_bytes < crw_center_normalize_ws_bytes(rows, C, S)) return CRW_EWORKSPACE;
  double *partial = ws_doubles(ws);
  const int nslab = slab_count(rows), srows = slab_rows(rows);
  int cw = 1;  // channels side by side in the two sums: a power of two, at most a workgroup of launch 2
  while (cw < C && cw < CN_NT) cw *= 2;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(center_partial_kernel, dim3(nslab, S), dim3(CP_NT), 0, s, emb, rows, C, seg_dev, segv, S, nslab, srows, cw, partial);
  CRW_TRY(check_launch());
  hipLaunchKernelGGL(center_normalize_kernel, dim3((rows + CN_ROWS - 1) / CN_ROWS), dim3(CN_NT), (size_t)C * sizeof(double), s, emb, rows, C,
                     seg_dev, segv, S, nslab, cw, partial, ehat, mean);
  return check_launch();
}

}  // extern "C"
