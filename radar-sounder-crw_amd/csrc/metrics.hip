// Evaluation: the confusion matrix of a label map against its ground truth, with the reference's "remove uncertain class" masks
// (scripts/test/test_all.py:161-187: boolean-index copies, pred.cpu(), sklearn's classification_report + confusion_matrix)
// as ONE pass over the maps where they already are -- HBM.
//
// The kernel is a pure stream of P x (4+4[+4]) or P x (1+1[+1]) bytes and K*K <= 256 counters:
//   * every lane owns 16 consecutive pixels per step (one 16-byte load per int8 operand, four per fp32 operand, all issued
//     before the first use), a wave 1024 consecutive pixels, and the grid (256 CUs x 8 workgroups, not P / 256) strides over
//     the map.  Pointers / lengths that are not 16-byte multiples: a scalar head up to the first pixel at which every operand is
//     16-byte aligned and a scalar tail, spread over the grid one pixel per thread; operands whose misalignments differ have
//     no such pixel and take the scalar route for the whole map (correct, 1 or 4 bytes per lane).
//   * aggregation: label maps are layered, so a lane's 16 pixels -- and its next 16, one grid stride further along the same
//     rows -- nearly always fall into the same bin.  Each lane keeps ONE open run (bin, count) in registers across its whole
//     stream and touches LDS only when the bin changes: a layered map costs a handful of LDS adds per lane per call, where a
//     ballot per distinct bin costs a scalar round trip per pixel step whether or not anything changed.  The flush is an LDS add
//     into a WAVE-PRIVATE histogram (4 waves x (K*K+2) counters), so lanes of different waves never contend; uniformly random
//     labels (no runs at all) degrade to one LDS add per pixel spread over K*K addresses -- measured in
//     profiles/metrics_timing.log.
//   * bins K*K and K*K+1 count the masked and the invalid pixels, so dropped[] falls out of the same histogram.
//   * one global update per workgroup: its K*K+2 sums go to its own column of `ws` ([bin][workgroup]) by plain vector stores; a
//     second, tiny kernel (one workgroup per bin, coalesced loads of that bin's row) adds them in 64 bits into counts / dropped.
//     No atomics on global memory, nothing to pre-clear, and integer sums: bit-reproducible.
//   * 32-bit partials cannot overflow: the grid grows with P so that no workgroup sees more than 2^31 pixels (grid_for()),
//     which bounds every lane's run count, every LDS counter and every partial sum by 2^31 < 2^32.
#include "labelmap.h"

namespace crw {
using namespace labelmap;
namespace {

struct ConfArgs {
  const void *gt, *pred, *aux;
  size_t P;
  size_t head;      // pixels [0, head) and [tail0, P) are scalar work, [head, tail0) is whole 16-pixel lane chunks
  size_t tail0;
  int K;
  int ig, ip, ia;   // ignore labels (IGNORE_NONE = none)
  int dg, dp, da;   // dtype codes (scalar route)
  uint32_t *part;   // [K*K+2][gridDim.x]
};

// one open run per lane; flush = one add into the wave's private LDS histogram
struct Run {
  int bin;
  uint32_t n;
  uint32_t *h;
  __device__ inline void add(int b) {
    if (b != bin) {
      if (n) atomicAdd(&h[bin], n);
      bin = b;
      n = 0;
    }
    ++n;
  }
  __device__ inline void flush() {
    if (n) atomicAdd(&h[bin], n);
    n = 0;
  }
};

__device__ inline int bin_of(int g, int p, int a, const ConfArgs &c) {
  const int KK = c.K * c.K;
  if (g == c.ig || p == c.ip || a == c.ia) return KK;                          // masked
  if ((unsigned)g >= (unsigned)c.K || (unsigned)p >= (unsigned)c.K) return KK + 1;  // invalid: counted, binned nowhere
  return g * c.K + p;
}

template <typename CG, typename CP, typename CA>
__global__ __launch_bounds__(CONF_BLOCK) void confusion_kernel(ConfArgs c) {
  __shared__ uint32_t hist[CONF_WAVES][CONF_MAX_BINS];
  const int nbins = c.K * c.K + 2;
  for (int i = threadIdx.x; i < CONF_WAVES * CONF_MAX_BINS; i += CONF_BLOCK) (&hist[0][0])[i] = 0;
  __syncthreads();

  Run run{0, 0, hist[threadIdx.x / WAVE]};
  const size_t nthreads = (size_t)gridDim.x * CONF_BLOCK;
  const size_t tid = (size_t)blockIdx.x * CONF_BLOCK + threadIdx.x;

  // body: whole lane chunks, every load 16-byte aligned and inside [head, tail0)
  const size_t nchunk = (c.tail0 - c.head) / CONF_LANE_PIX;
  for (size_t ch = tid; ch < nchunk; ch += nthreads) {
    const size_t pix = c.head + ch * CONF_LANE_PIX;
    CG g;
    CP p;
    CA a;
    g.load(c.gt, pix);
    p.load(c.pred, pix);
    a.load(c.aux, pix);
#pragma unroll
    for (int j = 0; j < CONF_LANE_PIX; ++j) run.add(bin_of(g.code(j), p.code(j), a.code(j), c));
  }

  // head and tail (or, for operands that share no alignment, the whole map): one pixel per thread, bounds = [0, P)
  const size_t nscalar = c.head + (c.P - c.tail0);
  for (size_t i = tid; i < nscalar; i += nthreads) {
    const size_t pix = i < c.head ? i : c.tail0 + (i - c.head);
    const int a = c.aux ? code_at(c.aux, c.da, pix) : CODE_INVALID;
    run.add(bin_of(code_at(c.gt, c.dg, pix), code_at(c.pred, c.dp, pix), a, c));
  }
  run.flush();
  __syncthreads();

  for (int b = threadIdx.x; b < nbins; b += CONF_BLOCK) {
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < CONF_WAVES; ++w) s += hist[w][b];
    c.part[(size_t)b * gridDim.x + blockIdx.x] = s;
  }
}

// one workgroup per bin: 64-bit sum of that bin's row of partials (contiguous: coalesced loads, all in flight at once), in a
// fixed order
__global__ __launch_bounds__(CONF_BLOCK) void confusion_sum_kernel(const uint32_t *__restrict__ part, unsigned nrows, int K,
                                                                  int64_t *__restrict__ counts, int64_t *__restrict__ dropped) {
  __shared__ unsigned long long wsum[CONF_WAVES];
  const int b = blockIdx.x;
  const uint32_t *row = part + (size_t)b * nrows;
  unsigned long long s = 0;
#pragma unroll 8
  for (unsigned r = threadIdx.x; r < nrows; r += CONF_BLOCK) s += row[r];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (threadIdx.x % WAVE == 0) wsum[threadIdx.x / WAVE] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
#pragma unroll
    for (int w = 0; w < CONF_WAVES; ++w) t += wsum[w];
    if (b < K * K)
      counts[b] = (int64_t)t;
    else
      dropped[b - K * K] = (int64_t)t;
  }
}

template <typename CG, typename CP>
void launch_aux(int da, bool has_aux, unsigned grid, hipStream_t s, const ConfArgs &c) {
  if (!has_aux)
    hipLaunchKernelGGL((confusion_kernel<CG, CP, NoChunk>), dim3(grid), dim3(CONF_BLOCK), 0, s, c);
  else if (da == CRW_DT_F32)
    hipLaunchKernelGGL((confusion_kernel<CG, CP, Chunk<CRW_DT_F32>>), dim3(grid), dim3(CONF_BLOCK), 0, s, c);
  else
    hipLaunchKernelGGL((confusion_kernel<CG, CP, Chunk<CRW_DT_I8>>), dim3(grid), dim3(CONF_BLOCK), 0, s, c);
}

}  // namespace
}  // namespace crw

extern "C" size_t crw_confusion_ws_bytes(size_t P, int K) {
  if (K < 2 || K > 16) return 0;
  return crw::align_up((size_t)crw::grid_for(P) * (size_t)(K * K + 2) * sizeof(uint32_t), 16);
}

extern "C" int crw_confusion(const void *gt, int gt_dtype, const void *pred, int pred_dtype, const void *aux, int aux_dtype,
                             size_t P, int K, int ignore_gt, int ignore_pred, int ignore_aux, int64_t *counts, int64_t *dropped,
                             void *ws, size_t ws_bytes, crw_stream_t stream) {
  using namespace crw;
  clear_stale_error();
  if (K < 2 || K > 16 || !counts || !dropped || !dtype_ok(gt_dtype) || !dtype_ok(pred_dtype) || (aux && !dtype_ok(aux_dtype)))
    return CRW_EINVAL;
  if (P > 0 && (!gt || !pred)) return CRW_EINVAL;
  if (ignore_gt < -1 || ignore_pred < -1 || ignore_aux < -1 || (!aux && ignore_aux != -1)) return CRW_EINVAL;
  if ((gt_dtype == CRW_DT_F32 && ((uintptr_t)gt & 3)) || (pred_dtype == CRW_DT_F32 && ((uintptr_t)pred & 3)) ||
      (aux && aux_dtype == CRW_DT_F32 && ((uintptr_t)aux & 3)) || ((uintptr_t)counts & 7) || ((uintptr_t)dropped & 7))
    return CRW_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = P ? grid_for(P) : 0;
  if (P) {
    if (!ws || ((uintptr_t)ws & 3)) return CRW_EINVAL;
    if (ws_bytes < crw_confusion_ws_bytes(P, K)) return CRW_EWORKSPACE;
    ConfArgs c;
    c.gt = gt, c.pred = pred, c.aux = aux, c.P = P, c.K = K;
    c.ig = ignore_gt < 0 ? IGNORE_NONE : ignore_gt;
    c.ip = ignore_pred < 0 ? IGNORE_NONE : ignore_pred;
    c.ia = ignore_aux < 0 ? IGNORE_NONE : ignore_aux;
    c.dg = gt_dtype, c.dp = pred_dtype, c.da = aux ? aux_dtype : CRW_DT_I8;
    c.part = static_cast<uint32_t *>(ws);
    // the first pixel at which every operand sits on a 16-byte boundary (none: operands misaligned against each other)
    auto aligned_at = [&](size_t h) {
      return !(((uintptr_t)gt + h * elem(gt_dtype)) & 15) && !(((uintptr_t)pred + h * elem(pred_dtype)) & 15) &&
             (!aux || !(((uintptr_t)aux + h * elem(aux_dtype)) & 15));
    };
    size_t head = 0;
    while (head < 16 && !aligned_at(head)) ++head;
    if (head >= 16 || head >= P) {
      c.head = 0, c.tail0 = 0;  // everything scalar
    } else {
      c.head = head;
      c.tail0 = head + (P - head) / CONF_LANE_PIX * CONF_LANE_PIX;
    }
    const bool has_aux = aux != nullptr;
    if (gt_dtype == CRW_DT_F32 && pred_dtype == CRW_DT_F32)
      launch_aux<Chunk<CRW_DT_F32>, Chunk<CRW_DT_F32>>(c.da, has_aux, grid, s, c);
    else if (gt_dtype == CRW_DT_F32)
      launch_aux<Chunk<CRW_DT_F32>, Chunk<CRW_DT_I8>>(c.da, has_aux, grid, s, c);
    else if (pred_dtype == CRW_DT_F32)
      launch_aux<Chunk<CRW_DT_I8>, Chunk<CRW_DT_F32>>(c.da, has_aux, grid, s, c);
    else
      launch_aux<Chunk<CRW_DT_I8>, Chunk<CRW_DT_I8>>(c.da, has_aux, grid, s, c);
    CRW_TRY(check_launch());
  }
  hipLaunchKernelGGL(confusion_sum_kernel, dim3(K * K + 2), dim3(CONF_BLOCK), 0, s, static_cast<const uint32_t *>(ws), grid, K, counts,
                     dropped);
  return check_launch();
}
