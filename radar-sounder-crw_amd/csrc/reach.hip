// Accuracy against distance (include/crw_hip_reach.h): one confusion matrix per group of COLUMNS of a label map, with
// crw_confusion's mask and validity rules and crw_calibration's confidence test, in one pass over the maps where they lie.
//
// Where the counters sit.  The worst case is 64 groups x (16 x 16 + 3) counters = 66 KB of 32-bit counters.
//   * wave-private, crw_confusion's layout, is out: 4 waves x 66 KB exceeds the CU's 160 KB, and crw_confusion's flat stream
//     (a lane owns 16 consecutive pixels of a row) would have to look the group up per pixel: a lane's run of equal bins ends at
//     every group border.
//   * workgroup-shared [group][bin] makes the lanes of a wave meet on one address whenever neighbouring columns agree -- which
//     in a layered map is nearly always: 64-way serialised LDS atomics.
//   * chosen: a workgroup per strip of 64 columns, ONE LANE PER COLUMN (crw_horizons's geometry).  The group is a property of the
//     column, so a lane looks it up once, and the strip's histogram is [bin][lane]: the lane IS the live group, no counter is
//     shared inside a wave (every lane has its own LDS bank, an atomic never contends within a wave), and the LDS size does not
//     depend on `groups` at all: K*K x 64 counters, 6.5 KB at K = 5 and 65 KB at K = 16 (two capacities of one kernel text, 8
//     and 16 classes, so that the usual K keeps four workgroups on a CU; the three dropped counters live in registers).
//   * a wave reads 64 consecutive columns of one row (fp32: 256 contiguous bytes, int8: 64) and walks down its slab of rows,
//     REACH_UNROLL rows of every operand loaded before the first is used; the rows are cut into S slabs, one wave each, all in
//     the strip's workgroup (the slab waves share the strip's histogram through LDS atomics on distinct lanes' addresses).
//   * a lane keeps one open run (bin, count) in registers like crw_confusion's: down a column of a layered map the bin changes
//     a handful of times, so the LDS sees a handful of adds per lane.  The confidence is one fp64 add per pixel in a register.
//   * after a barrier the strip folds its columns into its groups: members[g] = the 64-bit set of lanes of group g, and thread
//     (g, bin) adds the member lanes' counters in lane order.  Every (group, bin) of the strip -- zeros included -- goes to its
//     own column of `ws` ([group * K*K + bin][strip], int64; the conf sums [group][strip], fp64: slabs, then lanes, in index
//     order), and a second, tiny kernel adds each row in a fixed order.  No global atomics, nothing to pre-clear:
//     bit-reproducible, the fp64 sums included.
//   * an excluded column (col_group >= groups) is never read: its lane adds its slab's rows to dropped[3].
// One route: there is no selector, so the route log has no name for it.
#include "labelmap.h"
#include "crw_hip_reach.h"

namespace crw {
using namespace labelmap;
namespace {

constexpr int REACH_MAX_SLABS = 8;
constexpr int REACH_UNROLL = 8;        // rows of every operand in flight per lane
constexpr int REACH_SUM_BLOCK = 256;
constexpr int REACH_DROPS = 4;
constexpr int REACH_PAD = WAVE + 1;    // the fold reads one lane of many bins at once: an odd pitch spreads them over the banks
constexpr int DT_NONE = -1;            // no aux operand
constexpr int GROUP_NONE = 255;

struct ReachArgs {
  const void *gt, *pred, *aux;
  const float *conf;
  const uint8_t *group;
  int rows, cols;
  size_t ld;
  int K, groups, S;
  int ig, ip, ia;
  int64_t *part;   // [groups*K*K + 4][gridDim.x]
  double *cpart;   // [groups][gridDim.x]
};

__host__ __device__ inline int slab_begin(int s, int rows, int S) { return (int)((long long)s * rows / S); }

template <int DT>
struct Raw {
  typedef float type;
  static __device__ inline float load(const void *b, size_t i) { return static_cast<const float *>(b)[i]; }
  static __device__ inline int code(float v) { return code_f32(v); }
};
template <>
struct Raw<CRW_DT_I8> {
  typedef int8_t type;
  static __device__ inline int8_t load(const void *b, size_t i) { return static_cast<const int8_t *>(b)[i]; }
  static __device__ inline int code(int8_t v) { return (int)v; }
};
template <>
struct Raw<DT_NONE> {
  typedef int type;
  static __device__ inline int load(const void *, size_t) { return 0; }
  static __device__ inline int code(int) { return CODE_INVALID; }  // never equals an ignore label
};

template <int DG, int DP, int DA, bool HC, int KCAP>
__global__ __launch_bounds__(REACH_MAX_SLABS *WAVE) void reach_kernel(ReachArgs c) {
  __shared__ uint32_t hist[KCAP * KCAP][REACH_PAD];  // [bin][column of the strip]
  __shared__ double csum[REACH_MAX_SLABS][WAVE];
  __shared__ unsigned long long wdrop[REACH_MAX_SLABS][REACH_DROPS];
  __shared__ unsigned long long members[CRW_REACH_MAX_GROUPS];
  __shared__ int group_of[WAVE];
  const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
  const int col = blockIdx.x * WAVE + lane;
  const int KK = c.K * c.K;

  for (int i = threadIdx.x; i < KK * WAVE; i += blockDim.x) hist[i / WAVE][i % WAVE] = 0;
  int g = GROUP_NONE;
  if (col < c.cols) g = c.group[col];
  const bool excluded = col < c.cols && g >= c.groups;
  const bool counted = col < c.cols && g < c.groups;
  if (wave == 0) group_of[lane] = counted ? g : GROUP_NONE;
  __syncthreads();

  // ---- scan of slab `wave`
  const int r0 = slab_begin(wave, c.rows, c.S), r1 = slab_begin(wave + 1, c.rows, c.S);
  unsigned long long drop[REACH_DROPS] = {0, 0, 0, excluded ? (unsigned long long)(r1 - r0) : 0ull};
  double cs = 0.0;
  if (counted && r1 > r0) {
    int bin = 0;
    uint32_t n = 0;
    auto step = [&](int gg, int pp, int aa, float cf) {
      const bool masked = gg == c.ig || pp == c.ip || aa == c.ia;
      const bool invalid = !masked && ((unsigned)gg >= (unsigned)c.K || (unsigned)pp >= (unsigned)c.K);
      const bool bad = HC && !masked && !invalid && !(cf >= 0.f && cf <= 1.f);  // NaN fails both
      drop[0] += masked, drop[1] += invalid, drop[2] += bad;
      if (masked || invalid || bad) return;
      const int b = gg * c.K + pp;
      if (b != bin) {
        if (n) atomicAdd(&hist[bin][lane], n);
        bin = b, n = 0;
      }
      ++n;
      if (HC) cs += (double)cf;
    };
    int r = r0;
    for (; r + REACH_UNROLL <= r1; r += REACH_UNROLL) {
      typename Raw<DG>::type gv[REACH_UNROLL];
      typename Raw<DP>::type pv[REACH_UNROLL];
      typename Raw<DA>::type av[REACH_UNROLL];
      float cv[REACH_UNROLL];
#pragma unroll
      for (int j = 0; j < REACH_UNROLL; ++j) {
        const size_t i = (size_t)(r + j) * c.ld + col;
        gv[j] = Raw<DG>::load(c.gt, i);
        pv[j] = Raw<DP>::load(c.pred, i);
        av[j] = Raw<DA>::load(c.aux, i);
        cv[j] = HC ? c.conf[i] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < REACH_UNROLL; ++j) step(Raw<DG>::code(gv[j]), Raw<DP>::code(pv[j]), Raw<DA>::code(av[j]), cv[j]);
    }
    for (; r < r1; ++r) {
      const size_t i = (size_t)r * c.ld + col;
      step(Raw<DG>::code(Raw<DG>::load(c.gt, i)), Raw<DP>::code(Raw<DP>::load(c.pred, i)), Raw<DA>::code(Raw<DA>::load(c.aux, i)),
           HC ? c.conf[i] : 0.f);
    }
    if (n) atomicAdd(&hist[bin][lane], n);
  }
  if (HC) csum[wave][lane] = cs;
#pragma unroll
  for (int q = 0; q < REACH_DROPS; ++q) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) drop[q] += __shfl_xor(drop[q], o);
    if (lane == 0) wdrop[wave][q] = drop[q];
  }
  for (int m = threadIdx.x; m < c.groups; m += blockDim.x) {
    unsigned long long set = 0;
    for (int l = 0; l < WAVE; ++l) set |= (unsigned long long)(group_of[l] == m) << l;
    members[m] = set;
  }
  __syncthreads();

  // ---- fold the strip's columns into its groups
  const int nint = c.groups * KK;
  for (int i = threadIdx.x; i < nint + REACH_DROPS; i += blockDim.x) {
    unsigned long long sum = 0;
    if (i < nint) {
      const uint32_t *row = hist[i % KK];
      for (unsigned long long set = members[i / KK]; set; set &= set - 1) sum += row[__ffsll(set) - 1];
    } else {
      for (int w = 0; w < c.S; ++w) sum += wdrop[w][i - nint];
    }
    c.part[(size_t)i * gridDim.x + blockIdx.x] = (int64_t)sum;
  }
  if (HC) {
    for (int m = threadIdx.x; m < c.groups; m += blockDim.x) {
      double sum = 0.0;
      for (int w = 0; w < c.S; ++w)
        for (unsigned long long set = members[m]; set; set &= set - 1) sum += csum[w][__ffsll(set) - 1];
      c.cpart[(size_t)m * gridDim.x + blockIdx.x] = sum;
    }
  }
}

// one workgroup per output: its row of strip partials (contiguous) is added in a fixed order -- rows [0, nint + 4) in int64,
// the conf rows behind them in fp64
__global__ __launch_bounds__(REACH_SUM_BLOCK) void reach_sum_kernel(const int64_t *__restrict__ part, const double *__restrict__ cpart,
                                                                    unsigned nstrips, int nint, int64_t *__restrict__ counts,
                                                                    int64_t *__restrict__ dropped, double *__restrict__ conf_sum) {
  __shared__ long long wint[REACH_SUM_BLOCK / WAVE];
  __shared__ double wdbl[REACH_SUM_BLOCK / WAVE];
  const int b = blockIdx.x;
  if (b < nint + REACH_DROPS) {
    const int64_t *row = part + (size_t)b * nstrips;
    long long s = 0;
    for (unsigned r = threadIdx.x; r < nstrips; r += REACH_SUM_BLOCK) s += row[r];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (threadIdx.x % WAVE == 0) wint[threadIdx.x / WAVE] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      long long t = 0;
#pragma unroll
      for (int w = 0; w < REACH_SUM_BLOCK / WAVE; ++w) t += wint[w];
      if (b < nint)
        counts[b] = (int64_t)t;
      else
        dropped[b - nint] = (int64_t)t;
    }
  } else {
    const int m = b - nint - REACH_DROPS;
    const double *row = cpart + (size_t)m * nstrips;
    double s = 0.0;
    for (unsigned r = threadIdx.x; r < nstrips; r += REACH_SUM_BLOCK) s += row[r];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);  // both partners add the same two numbers: every lane holds the same bits
    if (threadIdx.x % WAVE == 0) wdbl[threadIdx.x / WAVE] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0.0;
#pragma unroll
      for (int w = 0; w < REACH_SUM_BLOCK / WAVE; ++w) t += wdbl[w];
      conf_sum[m] = t;
    }
  }
}

template <int DG, int DP, int DA, bool HC>
void launch_cap(unsigned grid, hipStream_t s, const ReachArgs &c) {
  const dim3 block(c.S * WAVE);
  if (c.K <= 8)
    hipLaunchKernelGGL((reach_kernel<DG, DP, DA, HC, 8>), dim3(grid), block, 0, s, c);
  else
    hipLaunchKernelGGL((reach_kernel<DG, DP, DA, HC, 16>), dim3(grid), block, 0, s, c);
}

template <int DG, int DP, int DA>
void launch_conf(unsigned grid, hipStream_t s, const ReachArgs &c) {
  if (c.conf)
    launch_cap<DG, DP, DA, true>(grid, s, c);
  else
    launch_cap<DG, DP, DA, false>(grid, s, c);
}

template <int DG, int DP>
void launch_aux(int da, unsigned grid, hipStream_t s, const ReachArgs &c) {
  if (!c.aux)
    launch_conf<DG, DP, DT_NONE>(grid, s, c);
  else if (da == CRW_DT_F32)
    launch_conf<DG, DP, CRW_DT_F32>(grid, s, c);
  else
    launch_conf<DG, DP, CRW_DT_I8>(grid, s, c);
}

inline unsigned strips_of(int cols) { return (unsigned)((cols + WAVE - 1) / WAVE); }

// enough waves for 12 per CU on 256 CUs (24 576 columns: 8 slabs), slabs of at least 32 rows: crw_horizons's rule
inline int choose_slabs(int rows, int cols) {
  const unsigned strips = strips_of(cols);
  int S = strips ? (int)((3072 + strips - 1) / strips) : 1;
  if (S > rows / 32) S = rows / 32;
  if (S > REACH_MAX_SLABS) S = REACH_MAX_SLABS;
  return S < 1 ? 1 : S;
}

inline bool shape_ok(int rows, int cols, int K, int groups) {
  return K >= 2 && K <= 16 && groups >= 1 && groups <= CRW_REACH_MAX_GROUPS && rows >= 0 && cols >= 0;
}

}  // namespace
}  // namespace crw

extern "C" size_t crw_confusion_grouped_ws_bytes(int rows, int cols, int K, int groups) {
  if (!crw::shape_ok(rows, cols, K, groups) || rows == 0) return 0;
  return (size_t)crw::strips_of(cols) * (size_t)(groups * K * K + crw::REACH_DROPS + groups) * 8;
}

extern "C" int crw_confusion_grouped(const void *gt, int gt_dtype, const void *pred, int pred_dtype, const void *aux, int aux_dtype,
                                     const float *conf, int rows, int cols, size_t ld, const uint8_t *col_group, int groups, int K,
                                     int ignore_gt, int ignore_pred, int ignore_aux, int64_t *counts, double *conf_sum,
                                     int64_t *dropped, void *ws, size_t ws_bytes, crw_stream_t stream) {
  using namespace crw;
  clear_stale_error();
  if (!shape_ok(rows, cols, K, groups) || !counts || !dropped || !dtype_ok(gt_dtype) || !dtype_ok(pred_dtype) ||
      (aux && !dtype_ok(aux_dtype)))
    return CRW_EINVAL;
  if (ld < (size_t)cols || (conf == nullptr) != (conf_sum == nullptr)) return CRW_EINVAL;
  const bool pixels = rows > 0 && cols > 0;
  if (pixels && (!gt || !pred || !col_group)) return CRW_EINVAL;
  if (ignore_gt < -1 || ignore_pred < -1 || ignore_aux < -1 || (!aux && ignore_aux != -1)) return CRW_EINVAL;
  if ((gt_dtype == CRW_DT_F32 && ((uintptr_t)gt & 3)) || (pred_dtype == CRW_DT_F32 && ((uintptr_t)pred & 3)) ||
      (aux && aux_dtype == CRW_DT_F32 && ((uintptr_t)aux & 3)) || ((uintptr_t)conf & 3) || ((uintptr_t)counts & 7) ||
      ((uintptr_t)dropped & 7) || ((uintptr_t)conf_sum & 7))
    return CRW_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = pixels ? strips_of(cols) : 0;
  const int nint = groups * K * K;
  int64_t *part = static_cast<int64_t *>(ws);
  double *cpart = nullptr;
  if (grid) {
    if (!ws || ((uintptr_t)ws & 7)) return CRW_EINVAL;
    if (ws_bytes < crw_confusion_grouped_ws_bytes(rows, cols, K, groups)) return CRW_EWORKSPACE;
    cpart = reinterpret_cast<double *>(part + (size_t)(nint + REACH_DROPS) * grid);
    ReachArgs c;
    c.gt = gt, c.pred = pred, c.aux = aux, c.conf = conf, c.group = col_group, c.rows = rows, c.cols = cols, c.ld = ld;
    c.K = K, c.groups = groups;
    c.S = choose_slabs(rows, cols);
    if (c.S > rows) c.S = rows;
    c.ig = ignore_gt < 0 ? IGNORE_NONE : ignore_gt;
    c.ip = ignore_pred < 0 ? IGNORE_NONE : ignore_pred;
    c.ia = ignore_aux < 0 ? IGNORE_NONE : ignore_aux;
    c.part = part, c.cpart = cpart;
    if (gt_dtype == CRW_DT_F32 && pred_dtype == CRW_DT_F32)
      launch_aux<CRW_DT_F32, CRW_DT_F32>(aux_dtype, grid, s, c);
    else if (gt_dtype == CRW_DT_F32)
      launch_aux<CRW_DT_F32, CRW_DT_I8>(aux_dtype, grid, s, c);
    else if (pred_dtype == CRW_DT_F32)
      launch_aux<CRW_DT_I8, CRW_DT_F32>(aux_dtype, grid, s, c);
    else
      launch_aux<CRW_DT_I8, CRW_DT_I8>(aux_dtype, grid, s, c);
    CRW_TRY(check_launch());
  }
  hipLaunchKernelGGL(reach_sum_kernel, dim3(nint + REACH_DROPS + (conf ? groups : 0)), dim3(REACH_SUM_BLOCK), 0, s, part, cpart, grid,
                     nint, counts, dropped, conf_sum);
  return check_launch();
}
