// Confidence of a propagated label map, from the soft labels crw_labelprop_propagate already writes (L [T*N, M], one probability
// row per node; the upstream propagation class returns this next to the arg-max as `masks_pred_conf`, maskedatt.py CRW.forward):
//   crw_labelprop_confidence  L -> conf [N, T] (the layout of pred): largest probability, top-two margin or 1 - normalised entropy
//   crw_merge_confidence      per pixel, keep the pass -- forward or reverse -- that is surer
//   crw_calibration           reliability histogram of a confidence map against the ground truth, with crw_confusion's masks
// All three are streams over HBM with next to no arithmetic.
//
// crw_calibration follows metrics.hip (same grid, same 16-pixel lane chunks of 16-byte loads, same scalar head / tail for views
// into a wider map, same per-workgroup partials in `ws` added by a second tiny kernel) with one difference: next to the integer
// counts it sums the confidences of every bin in DOUBLE, and that sum has to come out bit-identical run after run.  So nothing
// here is an atomic.  At every pixel step the wave walks the distinct bins its 64 lanes hold (a ballot per bin: confidence maps
// are upsampled node maps, neighbouring lanes mostly agree), adds the bin's confidences over the lanes with a butterfly of
// __shfl_xor -- a fixed order -- and lane 0 adds the three numbers into the WAVE-PRIVATE histogram in LDS with plain loads and
// stores.  The four waves' histograms are added in wave order, the workgroups' partials in index order.  Uniformly random bins
// cost `bins` ballots per step (tools/confidence_timing.py times both).
#include "confidence_of.h"
#include "labelmap.h"

namespace crw {
using namespace labelmap;
namespace {

// ---- confidence of the soft labels ---------------------------------------------------------------------------------------------
constexpr int LC_BLOCK = 256;

// one node per thread, in L's order (rows of M floats: the threads of a wave read one contiguous stretch); conf is [N][T]
template <int KIND>
__global__ __launch_bounds__(LC_BLOCK) void labelprop_confidence_kernel(const float *__restrict__ L, int T, int N, int M, int t0,
                                                                        float ln_m, float *__restrict__ conf) {
  const long i = (long)blockIdx.x * LC_BLOCK + threadIdx.x;  // node (t - t0) * N + n
  if (i >= (long)(T - t0) * N) return;
  const int t = t0 + (int)(i / N), n = (int)(i % N);
  const float *row = L + ((long)t * N + n) * M;
  float p[16];
  if ((M & 3) == 0 && !((uintptr_t)L & 15)) {
#pragma unroll
    for (int m = 0; m < 16; m += 4)
      if (m < M) {
        const float4 v = *reinterpret_cast<const float4 *>(row + m);
        p[m] = v.x, p[m + 1] = v.y, p[m + 2] = v.z, p[m + 3] = v.w;
      }
  } else {
#pragma unroll
    for (int m = 0; m < 16; ++m)
      if (m < M) p[m] = row[m];
  }
  conf[(long)n * T + t] = confidence_of<KIND>(p, M, ln_m);
}

// ---- confidence-ruled merge ----------------------------------------------------------------------------------------------------
constexpr int MG_BLOCK = 256;

struct MergeArgs {
  const void *fl, *rl;      // labels of the two passes
  const float *fc, *rc;     // their confidences
  void *ol;
  float *oc;
  uint8_t *took;            // may be NULL
  size_t P, head, tail0;    // [head, tail0): whole 16-pixel lane chunks, every pointer 16-byte aligned there
};

__device__ inline float comp(const float4 &v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }

// Labels are copied, never decoded: the rule reads the confidences alone.  Every lane reads all of its pixels before it writes
// any of them, and no lane reads another's: out_* may alias fwd_* (or rev_*).
template <typename LAB>
__global__ __launch_bounds__(MG_BLOCK) void merge_confidence_kernel(MergeArgs a) {
  const size_t nthreads = (size_t)gridDim.x * MG_BLOCK;
  const size_t tid = (size_t)blockIdx.x * MG_BLOCK + threadIdx.x;
  const LAB *fl = static_cast<const LAB *>(a.fl), *rl = static_cast<const LAB *>(a.rl);
  LAB *ol = static_cast<LAB *>(a.ol);
  constexpr int LV = 16 / sizeof(LAB);   // labels per 16-byte load
  constexpr int NL = CONF_LANE_PIX / LV;  // 16-byte loads per chunk of labels
  typedef LAB lab_vec __attribute__((ext_vector_type(LV)));

  const size_t nchunk = (a.tail0 - a.head) / CONF_LANE_PIX;
  for (size_t ch = tid; ch < nchunk; ch += nthreads) {
    const size_t pix = a.head + ch * CONF_LANE_PIX;
    float4 fc[4], rc[4];
    lab_vec f[NL], r[NL];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      fc[j] = reinterpret_cast<const float4 *>(a.fc + pix)[j];
      rc[j] = reinterpret_cast<const float4 *>(a.rc + pix)[j];
    }
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      f[j] = reinterpret_cast<const lab_vec *>(fl + pix)[j];
      r[j] = reinterpret_cast<const lab_vec *>(rl + pix)[j];
    }
    uint32_t tk[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < CONF_LANE_PIX; ++j) {
      const float cf = comp(fc[j >> 2], j & 3), cr = comp(rc[j >> 2], j & 3);
      const bool take = cr > cf;  // false for a tie and for a NaN on either side
      const float c = take ? cr : cf;
      float4 &o = fc[j >> 2];
      if ((j & 3) == 0) o.x = c;
      if ((j & 3) == 1) o.y = c;
      if ((j & 3) == 2) o.z = c;
      if ((j & 3) == 3) o.w = c;
      f[j / LV][j % LV] = take ? r[j / LV][j % LV] : f[j / LV][j % LV];
      tk[j >> 2] |= (uint32_t)take << (8 * (j & 3));
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) reinterpret_cast<float4 *>(a.oc + pix)[j] = fc[j];
#pragma unroll
    for (int j = 0; j < NL; ++j) reinterpret_cast<lab_vec *>(ol + pix)[j] = f[j];
    if (a.took) *reinterpret_cast<uint4 *>(a.took + pix) = make_uint4(tk[0], tk[1], tk[2], tk[3]);
  }

  // head and tail (or, for pointers that share no alignment, the whole map): one pixel per thread
  const size_t nscalar = a.head + (a.P - a.tail0);
  for (size_t i = tid; i < nscalar; i += nthreads) {
    const size_t pix = i < a.head ? i : a.tail0 + (i - a.head);
    const float cf = a.fc[pix], cr = a.rc[pix];
    const LAB lf = fl[pix], lr = rl[pix];
    const bool take = cr > cf;
    a.oc[pix] = take ? cr : cf;
    ol[pix] = take ? lr : lf;
    if (a.took) a.took[pix] = take;
  }
}

// ---- calibration ---------------------------------------------------------------------------------------------------------------
constexpr int CAL_MAX_BINS = 64;
constexpr int CAL_ROWS = CAL_MAX_BINS + 3;  // + masked, invalid label, invalid confidence

struct CalArgs {
  const void *gt, *pred, *aux;
  const float *conf;
  size_t P, head, tail0;
  int K, bins;
  int ig, ip, ia;
  int dg, dp, da;
  uint32_t *part;   // [2 * bins + 3][gridDim.x]: pixels per bin, correct pixels per bin, the three dropped counts
  double *psum;     // [bins][gridDim.x]
};

// integer partial rows of `part`
__host__ __device__ inline int cal_int_rows(int bins) { return 2 * bins + 3; }

struct CalHist {
  uint32_t n[CAL_ROWS];
  uint32_t ok[CAL_MAX_BINS];
  double sum[CAL_MAX_BINS];
};

// row of the wave histogram a pixel falls into: its confidence bin, or bins + {0: masked, 1: invalid label, 2: invalid confidence}
// -- crw_confusion's tests in crw_confusion's order, then the confidence
__device__ inline int cal_row(int g, int p, int a, float c, const CalArgs &k) {
  if (g == k.ig || p == k.ip || a == k.ia) return k.bins;
  if ((unsigned)g >= (unsigned)k.K || (unsigned)p >= (unsigned)k.K) return k.bins + 1;
  if (!(c >= 0.f && c <= 1.f)) return k.bins + 2;  // NaN fails both
  const int b = (int)floorf(c * (float)k.bins);
  return b < k.bins - 1 ? b : k.bins - 1;
}

// One pixel per lane (`has`: the lane holds one): every distinct row among the lanes is reduced over the wave and added by lane 0.
// The loop runs on wave-uniform values only, so all 64 lanes take part in every shuffle.
__device__ inline void cal_wave_add(bool has, int row, bool correct, float c, int bins, CalHist *h) {
  unsigned long long todo = __ballot(has);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int r = __shfl(row, leader);
    const bool mine = has && row == r;
    const unsigned long long m = __ballot(mine);
    const unsigned long long mok = __ballot(mine && correct);
    if (r < bins) {
      double s = mine ? (double)c : 0.0;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
      if (threadIdx.x % WAVE == 0) {
        h->ok[r] += (uint32_t)__popcll(mok);
        h->sum[r] += s;
      }
    }
    if (threadIdx.x % WAVE == 0) h->n[r] += (uint32_t)__popcll(m);
    todo &= ~m;
  }
}

template <typename CG, typename CP, typename CA>
__global__ __launch_bounds__(CONF_BLOCK) void calibration_kernel(CalArgs c) {
  __shared__ CalHist hist[CONF_WAVES];
  for (int i = threadIdx.x; i < CONF_WAVES * CAL_ROWS; i += CONF_BLOCK) hist[i / CAL_ROWS].n[i % CAL_ROWS] = 0;
  for (int i = threadIdx.x; i < CONF_WAVES * CAL_MAX_BINS; i += CONF_BLOCK) {
    hist[i / CAL_MAX_BINS].ok[i % CAL_MAX_BINS] = 0;
    hist[i / CAL_MAX_BINS].sum[i % CAL_MAX_BINS] = 0.0;
  }
  __syncthreads();

  CalHist *h = &hist[threadIdx.x / WAVE];
  const int lane = threadIdx.x % WAVE;
  const size_t nthreads = (size_t)gridDim.x * CONF_BLOCK;
  const size_t wave0 = (size_t)blockIdx.x * CONF_BLOCK + (threadIdx.x - lane);  // the wave's first thread: uniform loop bounds

  // body: whole lane chunks, every load 16-byte aligned and inside [head, tail0)
  const size_t nchunk = (c.tail0 - c.head) / CONF_LANE_PIX;
  for (size_t w = wave0; w < nchunk; w += nthreads) {
    const size_t ch = w + lane;
    const bool has = ch < nchunk;
    CG g;
    CP p;
    CA a;
    float4 cf[4] = {};
    if (has) {
      const size_t pix = c.head + ch * CONF_LANE_PIX;
      g.load(c.gt, pix);
      p.load(c.pred, pix);
      a.load(c.aux, pix);
#pragma unroll
      for (int j = 0; j < 4; ++j) cf[j] = reinterpret_cast<const float4 *>(c.conf + pix)[j];
    }
#pragma unroll
    for (int j = 0; j < CONF_LANE_PIX; ++j) {
      int row = 0;
      bool ok = false;
      const float v = comp(cf[j >> 2], j & 3);
      if (has) {
        const int gj = g.code(j), pj = p.code(j);
        row = cal_row(gj, pj, a.code(j), v, c);
        ok = gj == pj;
      }
      cal_wave_add(has, row, ok, v, c.bins, h);
    }
  }

  // head and tail (or, for operands that share no alignment, the whole map): one pixel per lane, bounds = [0, P)
  const size_t nscalar = c.head + (c.P - c.tail0);
  for (size_t w = wave0; w < nscalar; w += nthreads) {
    const size_t i = w + lane;
    const bool has = i < nscalar;
    int row = 0;
    bool ok = false;
    float v = 0.f;
    if (has) {
      const size_t pix = i < c.head ? i : c.tail0 + (i - c.head);
      const int gj = code_at(c.gt, c.dg, pix), pj = code_at(c.pred, c.dp, pix);
      const int aj = c.aux ? code_at(c.aux, c.da, pix) : CODE_INVALID;
      v = c.conf[pix];
      row = cal_row(gj, pj, aj, v, c);
      ok = gj == pj;
    }
    cal_wave_add(has, row, ok, v, c.bins, h);
  }
  __syncthreads();

  // the workgroup's partials: its waves in wave order
  const int nint = cal_int_rows(c.bins);
  for (int r = threadIdx.x; r < nint; r += CONF_BLOCK) {
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < CONF_WAVES; ++w)
      s += r < c.bins ? hist[w].n[r] : r < 2 * c.bins ? hist[w].ok[r - c.bins] : hist[w].n[r - c.bins];
    c.part[(size_t)r * gridDim.x + blockIdx.x] = s;
  }
  for (int b = threadIdx.x; b < c.bins; b += CONF_BLOCK) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < CONF_WAVES; ++w) s += hist[w].sum[b];
    c.psum[(size_t)b * gridDim.x + blockIdx.x] = s;
  }
}

// One workgroup per output number.  Blocks [0, 2 * bins + 3): 64-bit sum of one row of integer partials.  Blocks behind them: the
// double sum of one bin's partials -- thread t adds partials t, t + 256, ... in that order, then the butterfly, then the waves in
// wave order: the same additions in the same order for the same grid.
__global__ __launch_bounds__(CONF_BLOCK) void calibration_sum_kernel(const uint32_t *__restrict__ part, const double *__restrict__ psum,
                                                                    unsigned nrows, int bins, int64_t *__restrict__ counts,
                                                                    double *__restrict__ conf_sum, int64_t *__restrict__ dropped) {
  __shared__ unsigned long long wsum[CONF_WAVES];
  __shared__ double dsum[CONF_WAVES];
  const int b = blockIdx.x, nint = cal_int_rows(bins);
  if (b < nint) {
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
      if (b < bins)
        counts[2 * b] = (int64_t)t;
      else if (b < 2 * bins)
        counts[2 * (b - bins) + 1] = (int64_t)t;
      else
        dropped[b - 2 * bins] = (int64_t)t;
    }
  } else {
    const double *row = psum + (size_t)(b - nint) * nrows;
    double s = 0.0;
    for (unsigned r = threadIdx.x; r < nrows; r += CONF_BLOCK) s += row[r];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (threadIdx.x % WAVE == 0) dsum[threadIdx.x / WAVE] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0.0;
#pragma unroll
      for (int w = 0; w < CONF_WAVES; ++w) t += dsum[w];
      conf_sum[b - nint] = t;
    }
  }
}

template <typename CG, typename CP>
void launch_cal_aux(int da, bool has_aux, unsigned grid, hipStream_t s, const CalArgs &c) {
  if (!has_aux)
    hipLaunchKernelGGL((calibration_kernel<CG, CP, NoChunk>), dim3(grid), dim3(CONF_BLOCK), 0, s, c);
  else if (da == CRW_DT_F32)
    hipLaunchKernelGGL((calibration_kernel<CG, CP, Chunk<CRW_DT_F32>>), dim3(grid), dim3(CONF_BLOCK), 0, s, c);
  else
    hipLaunchKernelGGL((calibration_kernel<CG, CP, Chunk<CRW_DT_I8>>), dim3(grid), dim3(CONF_BLOCK), 0, s, c);
}

size_t cal_int_bytes(unsigned grid, int bins) { return align_up((size_t)grid * cal_int_rows(bins) * sizeof(uint32_t), 16); }

}  // namespace
}  // namespace crw

extern "C" int crw_labelprop_confidence(const float *L, int T, int N, int M, int kind, int first_frame, float *conf,
                                        crw_stream_t stream) {
  using namespace crw;
  clear_stale_error();
  if (!L || !conf || T < 1 || N < 1 || M < 2 || M > 16 || first_frame < 1 || first_frame > T || ((uintptr_t)L & 3) ||
      ((uintptr_t)conf & 3) || kind < CRW_CONF_MAXPROB || kind > CRW_CONF_ENTROPY)
    return CRW_EINVAL;
  const int t0 = first_frame == 1 ? 0 : first_frame;
  const long nodes = (long)(T - t0) * N;
  if (nodes <= 0) return CRW_OK;
  const unsigned grid = (unsigned)((nodes + LC_BLOCK - 1) / LC_BLOCK);
  const float ln_m = logf((float)M);
  hipStream_t s = (hipStream_t)stream;
  if (kind == CRW_CONF_MAXPROB)
    hipLaunchKernelGGL(labelprop_confidence_kernel<CRW_CONF_MAXPROB>, dim3(grid), dim3(LC_BLOCK), 0, s, L, T, N, M, t0, ln_m, conf);
  else if (kind == CRW_CONF_MARGIN)
    hipLaunchKernelGGL(labelprop_confidence_kernel<CRW_CONF_MARGIN>, dim3(grid), dim3(LC_BLOCK), 0, s, L, T, N, M, t0, ln_m, conf);
  else
    hipLaunchKernelGGL(labelprop_confidence_kernel<CRW_CONF_ENTROPY>, dim3(grid), dim3(LC_BLOCK), 0, s, L, T, N, M, t0, ln_m, conf);
  return check_launch();
}

extern "C" int crw_merge_confidence(const void *fwd_lab, const float *fwd_conf, const void *rev_lab, const float *rev_conf,
                                    int lab_dtype, size_t P, void *out_lab, float *out_conf, uint8_t *took, crw_stream_t stream) {
  using namespace crw;
  clear_stale_error();
  if (!dtype_ok(lab_dtype)) return CRW_EINVAL;
  if (P == 0) return CRW_OK;
  if (!fwd_lab || !fwd_conf || !rev_lab || !rev_conf || !out_lab || !out_conf) return CRW_EINVAL;
  const size_t le = elem(lab_dtype);
  if ((((uintptr_t)fwd_conf | (uintptr_t)rev_conf | (uintptr_t)out_conf) & 3) ||
      (le == 4 && (((uintptr_t)fwd_lab | (uintptr_t)rev_lab | (uintptr_t)out_lab) & 3)))
    return CRW_EINVAL;
  MergeArgs a;
  a.fl = fwd_lab, a.rl = rev_lab, a.fc = fwd_conf, a.rc = rev_conf, a.ol = out_lab, a.oc = out_conf, a.took = took, a.P = P;
  // the first pixel at which every pointer sits on a 16-byte boundary (none: pointers misaligned against each other)
  auto aligned_at = [&](size_t h) {
    return !(((uintptr_t)fwd_conf + 4 * h) & 15) && !(((uintptr_t)rev_conf + 4 * h) & 15) && !(((uintptr_t)out_conf + 4 * h) & 15) &&
           !(((uintptr_t)fwd_lab + le * h) & 15) && !(((uintptr_t)rev_lab + le * h) & 15) && !(((uintptr_t)out_lab + le * h) & 15) &&
           (!took || !(((uintptr_t)took + h) & 15));
  };
  size_t head = 0;
  while (head < 16 && !aligned_at(head)) ++head;
  if (head >= 16 || head >= P) {
    CRW_ROUTE("confidence.merge_scalar");
    a.head = 0, a.tail0 = 0;  // everything scalar
  } else {
    CRW_ROUTE("confidence.merge_vector");
    a.head = head;
    a.tail0 = head + (P - head) / CONF_LANE_PIX * CONF_LANE_PIX;
  }
  const unsigned grid = grid_for(P);
  if (lab_dtype == CRW_DT_F32)
    hipLaunchKernelGGL(merge_confidence_kernel<float>, dim3(grid), dim3(MG_BLOCK), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(merge_confidence_kernel<int8_t>, dim3(grid), dim3(MG_BLOCK), 0, (hipStream_t)stream, a);
  return check_launch();
}

extern "C" size_t crw_calibration_ws_bytes(size_t P, int K, int bins) {
  if (K < 2 || K > 16 || bins < 1 || bins > crw::CAL_MAX_BINS) return 0;
  const unsigned grid = crw::grid_for(P);
  return crw::cal_int_bytes(grid, bins) + (size_t)grid * bins * sizeof(double);
}

extern "C" int crw_calibration(const void *gt, int gt_dtype, const void *pred, int pred_dtype, const float *conf, const void *aux,
                               int aux_dtype, size_t P, int K, int bins, int ignore_gt, int ignore_pred, int ignore_aux,
                               int64_t *counts, double *conf_sum, int64_t *dropped, void *ws, size_t ws_bytes, crw_stream_t stream) {
  using namespace crw;
  clear_stale_error();
  if (K < 2 || K > 16 || bins < 1 || bins > CAL_MAX_BINS || !counts || !conf_sum || !dropped || !dtype_ok(gt_dtype) ||
      !dtype_ok(pred_dtype) || (aux && !dtype_ok(aux_dtype)))
    return CRW_EINVAL;
  if (P > 0 && (!gt || !pred || !conf)) return CRW_EINVAL;
  if (ignore_gt < -1 || ignore_pred < -1 || ignore_aux < -1 || (!aux && ignore_aux != -1)) return CRW_EINVAL;
  if ((gt_dtype == CRW_DT_F32 && ((uintptr_t)gt & 3)) || (pred_dtype == CRW_DT_F32 && ((uintptr_t)pred & 3)) ||
      (aux && aux_dtype == CRW_DT_F32 && ((uintptr_t)aux & 3)) || ((uintptr_t)conf & 3) || ((uintptr_t)counts & 7) ||
      ((uintptr_t)conf_sum & 7) || ((uintptr_t)dropped & 7))
    return CRW_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = P ? grid_for(P) : 0;
  CalArgs c;
  c.part = nullptr, c.psum = nullptr;
  if (P) {
    if (!ws || ((uintptr_t)ws & 7)) return CRW_EINVAL;
    if (ws_bytes < crw_calibration_ws_bytes(P, K, bins)) return CRW_EWORKSPACE;
    c.gt = gt, c.pred = pred, c.aux = aux, c.conf = conf, c.P = P, c.K = K, c.bins = bins;
    c.ig = ignore_gt < 0 ? IGNORE_NONE : ignore_gt;
    c.ip = ignore_pred < 0 ? IGNORE_NONE : ignore_pred;
    c.ia = ignore_aux < 0 ? IGNORE_NONE : ignore_aux;
    c.dg = gt_dtype, c.dp = pred_dtype, c.da = aux ? aux_dtype : CRW_DT_I8;
    c.part = static_cast<uint32_t *>(ws);
    c.psum = reinterpret_cast<double *>(static_cast<char *>(ws) + cal_int_bytes(grid, bins));
    auto aligned_at = [&](size_t h) {
      return !(((uintptr_t)gt + h * elem(gt_dtype)) & 15) && !(((uintptr_t)pred + h * elem(pred_dtype)) & 15) &&
             !(((uintptr_t)conf + h * 4) & 15) && (!aux || !(((uintptr_t)aux + h * elem(aux_dtype)) & 15));
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
      launch_cal_aux<Chunk<CRW_DT_F32>, Chunk<CRW_DT_F32>>(c.da, has_aux, grid, s, c);
    else if (gt_dtype == CRW_DT_F32)
      launch_cal_aux<Chunk<CRW_DT_F32>, Chunk<CRW_DT_I8>>(c.da, has_aux, grid, s, c);
    else if (pred_dtype == CRW_DT_F32)
      launch_cal_aux<Chunk<CRW_DT_I8>, Chunk<CRW_DT_F32>>(c.da, has_aux, grid, s, c);
    else
      launch_cal_aux<Chunk<CRW_DT_I8>, Chunk<CRW_DT_I8>>(c.da, has_aux, grid, s, c);
    CRW_TRY(check_launch());
  }
  hipLaunchKernelGGL(calibration_sum_kernel, dim3(cal_int_rows(bins) + bins), dim3(CONF_BLOCK), 0, s, c.part, c.psum, grid, bins, counts,
                     conf_sum, dropped);
  return check_launch();
}
