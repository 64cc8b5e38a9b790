// Layer horizons: per column of a label map and per class, the first row of the first qualifying run (top), the last row of the
// last qualifying run (bottom) and the number of pixels in qualifying runs (count, the layer thickness) -- for gt and for pred,
// under crw_confusion's mask and validity rules -- and the per-class statistics of pred's picks against gt's.  One pass over the
// maps where they lie, like crw_confusion.
//
//   * one lane per column: a wave reads 64 consecutive columns of one row (fp32: 256 contiguous bytes per load instruction, int8:
//     64) and walks down the rows, HORIZ_UNROLL rows of every operand loaded before the first is used;
//   * a column's rows are cut into S slabs (row_slabs), one wave each, all S waves of a 64-column tile in ONE workgroup: the
//     join across the slab borders happens in LDS after a barrier and needs no second pass over memory;
//   * each lane keeps one open run per map in registers (label, start).  A run that closes strictly inside its slab and is long
//     enough updates the column's per-class state; that state is top = min of the starts, bottom = max of the ends, count = sum of
//     the lengths over the qualifying runs -- order-free integer operations, so the S waves share ONE state per column, in LDS as
//     [map][quantity][class][lane] (a register array indexed by the class would go to scratch), updated by LDS atomics that never
//     contend within a wave (every lane has its own address);
//   * the run that touches the slab's first row (head) and the one that touches its last row (tail) are not judged by the slab:
//     it leaves (label, length) of the head and (label, start) of the tail in LDS, and after the barrier wave 0 walks the S
//     summaries of its columns in row order with one carried run -- a head that continues the carried run extends it, over as
//     many borders as it spans (a head as long as its slab is carried on) -- and judges every joined run once;
//   * after a second barrier the waves share the classes: picks are written (coalesced, 64 columns per store), the per-column
//     differences are reduced over the wave by shuffles (counts by ballots) and lane 0 stores the tile's 18 partials per class to
//     `ws` ([K*18+2][tiles], int64); a second, tiny kernel adds (or, for the maxima, maximises) each row in a fixed order.  No
//     global atomics, nothing to pre-clear, integers only: bit-reproducible.
#include "labelmap.h"

namespace crw {
using namespace labelmap;
namespace {

constexpr int HORIZ_MAX_SLABS = 8;
constexpr int HORIZ_MAX_K = 16;
constexpr int HORIZ_UNROLL = 8;       // rows of every operand in flight per lane
constexpr int HORIZ_STATS = 18;
constexpr int HORIZ_MAX_ROWS = 32768;
constexpr int HORIZ_SUM_BLOCK = 256;
constexpr int DT_NONE = -1;           // no aux operand
constexpr int TOP = 0, BOTTOM = 1, COUNT = 2;

struct HorizArgs {
  const void *gt, *pred, *aux;
  int rows, cols;
  size_t ld;
  int K, S;
  int ig, ip, ia;
  int min_run, tol;
  int32_t *picks;   // [2][3][K][cols] or null
  int64_t *part;    // [K*18+2][gridDim.x]
};

__device__ inline long long imax(long long a, long long b) { return a > b ? a : b; }
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

// per-class state of the workgroup's 64 columns
struct State {
  int v[2][3][HORIZ_MAX_K][WAVE];
  __device__ inline void add_run(int m, int lab, int start, int len, int lane) {
    atomicMin(&v[m][TOP][lab][lane], start);
    atomicMax(&v[m][BOTTOM][lab][lane], start + len - 1);
    atomicAdd(&v[m][COUNT][lab][lane], len);
  }
};

// one open run of one map in a lane's registers
struct Open {
  int lab;     // class, -1: no class (masked / invalid), -2: nothing seen yet
  int start;
};

template <int DG, int DP, int DA>
__global__ __launch_bounds__(HORIZ_MAX_SLABS *WAVE) void horizons_kernel(HorizArgs c) {
  __shared__ State st;
  __shared__ int summary[HORIZ_MAX_SLABS][2][2][WAVE];  // [slab][map][head, tail][lane]
  __shared__ int wdrop[HORIZ_MAX_SLABS][2];
  const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
  const int col = blockIdx.x * WAVE + lane;
  const bool live = col < c.cols;

  for (int i = threadIdx.x; i < 2 * 3 * HORIZ_MAX_K * WAVE; i += blockDim.x) {
    const int q = i / (HORIZ_MAX_K * WAVE) % 3;
    (&st.v[0][0][0][0])[i] = q == TOP ? INT32_MAX : q == BOTTOM ? -1 : 0;
  }
  __syncthreads();

  // ---- scan of slab `wave`
  const int r0 = slab_begin(wave, c.rows, c.S), r1 = slab_begin(wave + 1, c.rows, c.S);
  int nmask = 0, ninv = 0;
  if (live && r1 > r0) {
    Open run[2] = {{-2, r0}, {-2, r0}};
    int head[2] = {0, 0};
    auto close = [&](int m, int end) {
      const int len = end - run[m].start;
      if (len == 0) return;  // nothing seen yet
      if (run[m].start == r0)
        head[m] = (len << 8) | (run[m].lab + 1);  // the slab's first run: judged by the join
      else if (run[m].lab >= 0 && len >= c.min_run)
        st.add_run(m, run[m].lab, run[m].start, len, lane);
    };
    auto step = [&](int r, int g, int p, int a) {
      const bool masked = g == c.ig || p == c.ip || a == c.ia;
      const bool invalid = !masked && ((unsigned)g >= (unsigned)c.K || (unsigned)p >= (unsigned)c.K);
      nmask += masked, ninv += invalid;
      if (masked || invalid) g = p = -1;
      if (g != run[0].lab) {
        close(0, r);
        run[0].lab = g, run[0].start = r;
      }
      if (p != run[1].lab) {
        close(1, r);
        run[1].lab = p, run[1].start = r;
      }
    };
    int r = r0;
    for (; r + HORIZ_UNROLL <= r1; r += HORIZ_UNROLL) {
      typename Raw<DG>::type g[HORIZ_UNROLL];
      typename Raw<DP>::type p[HORIZ_UNROLL];
      typename Raw<DA>::type a[HORIZ_UNROLL];
#pragma unroll
      for (int j = 0; j < HORIZ_UNROLL; ++j) {
        const size_t i = (size_t)(r + j) * c.ld + col;
        g[j] = Raw<DG>::load(c.gt, i);
        p[j] = Raw<DP>::load(c.pred, i);
        a[j] = Raw<DA>::load(c.aux, i);
      }
#pragma unroll
      for (int j = 0; j < HORIZ_UNROLL; ++j) step(r + j, Raw<DG>::code(g[j]), Raw<DP>::code(p[j]), Raw<DA>::code(a[j]));
    }
    for (; r < r1; ++r) {
      const size_t i = (size_t)r * c.ld + col;
      step(r, Raw<DG>::code(Raw<DG>::load(c.gt, i)), Raw<DP>::code(Raw<DP>::load(c.pred, i)), Raw<DA>::code(Raw<DA>::load(c.aux, i)));
    }
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      int tail = 0;
      if (run[m].start == r0)
        head[m] = ((r1 - r0) << 8) | (run[m].lab + 1);  // one run over the whole slab: no tail of its own
      else
        tail = (run[m].start << 8) | (run[m].lab + 1);
      summary[wave][m][0][lane] = head[m];
      summary[wave][m][1][lane] = tail;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nmask += __shfl_xor(nmask, o), ninv += __shfl_xor(ninv, o);
  if (lane == 0) wdrop[wave][0] = nmask, wdrop[wave][1] = ninv;
  __syncthreads();

  // ---- join: wave 0 walks its columns' slab summaries in row order
  if (wave == 0) {
    if (live) {
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        int olab = -1, ostart = 0, olen = 0;
        auto judge = [&]() {
          if (olab >= 0 && olen >= c.min_run) st.add_run(m, olab, ostart, olen, lane);
        };
        for (int s = 0; s < c.S; ++s) {
          const int b0 = slab_begin(s, c.rows, c.S), b1 = slab_begin(s + 1, c.rows, c.S);
          if (b1 == b0) continue;
          const int h = summary[s][m][0][lane];
          const int hl = (h & 0xff) - 1, hn = h >> 8;
          if (hl == olab && olen > 0) {
            olen += hn;  // the carried run reaches b0 - 1 by construction: it goes on
          } else {
            judge();
            olab = hl, ostart = b0, olen = hn;
          }
          if (hn < b1 - b0) {  // the head ended inside the slab: the slab has a tail run of its own
            judge();
            const int t = summary[s][m][1][lane];
            olab = (t & 0xff) - 1, ostart = t >> 8, olen = b1 - ostart;
          }
        }
        judge();
      }
    }
    if (threadIdx.x == 0) {
      long long dm = 0, di = 0;
      for (int w = 0; w < c.S; ++w) dm += wdrop[w][0], di += wdrop[w][1];
      c.part[(size_t)(c.K * HORIZ_STATS) * gridDim.x + blockIdx.x] = dm;
      c.part[(size_t)(c.K * HORIZ_STATS + 1) * gridDim.x + blockIdx.x] = di;
    }
  }
  __syncthreads();

  // ---- picks and the tile's statistics: the waves share the classes
  for (int k = wave; k < c.K; k += c.S) {
    int pick[2][3];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int n = st.v[m][COUNT][k][lane];
      pick[m][TOP] = n ? st.v[m][TOP][k][lane] : -1;
      pick[m][BOTTOM] = n ? st.v[m][BOTTOM][k][lane] : -1;
      pick[m][COUNT] = n;
      if (c.picks && live) {
#pragma unroll
        for (int q = 0; q < 3; ++q) c.picks[((size_t)(m * 3 + q) * c.K + k) * c.cols + col] = pick[m][q];
      }
    }
    const bool hg = live && pick[0][COUNT] > 0, hp = live && pick[1][COUNT] > 0;
    const bool both = hg && hp;
    long long out[HORIZ_STATS];
    out[0] = __popcll(__ballot(both));
    out[1] = __popcll(__ballot(hg && !hp));
    out[2] = __popcll(__ballot(hp && !hg));
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int d = both ? pick[1][q] - pick[0][q] : 0;
      int ad = d < 0 ? -d : d, sd = d, mx = ad;
      long long sq = (long long)d * d;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        ad += __shfl_xor(ad, o);
        sd += __shfl_xor(sd, o);
        mx = imax(mx, __shfl_xor(mx, o));
        sq += __shfl_xor(sq, o);
      }
      out[3 + 5 * q + 0] = ad;
      out[3 + 5 * q + 1] = sq;
      out[3 + 5 * q + 2] = mx;
      out[3 + 5 * q + 3] = __popcll(__ballot(both && (d < 0 ? -d : d) <= c.tol));
      out[3 + 5 * q + 4] = sd;
    }
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < HORIZ_STATS; ++j) c.part[(size_t)(k * HORIZ_STATS + j) * gridDim.x + blockIdx.x] = out[j];
    }
  }
}

// one workgroup per statistic: its row of tile partials (contiguous) is added -- the three maxima: maximised -- in a fixed order
__global__ __launch_bounds__(HORIZ_SUM_BLOCK) void horizons_sum_kernel(const int64_t *__restrict__ part, unsigned ntiles, int K,
                                                                        int64_t *__restrict__ stats, int64_t *__restrict__ dropped) {
  __shared__ long long wacc[HORIZ_SUM_BLOCK / WAVE];
  const int b = blockIdx.x;
  const int j = b % HORIZ_STATS;
  const bool is_max = b < K * HORIZ_STATS && j >= 3 && (j - 3) % 5 == 2;
  const int64_t *row = part + (size_t)b * ntiles;
  long long s = 0;  // every partial is >= 0 where the maximum is taken
  for (unsigned r = threadIdx.x; r < ntiles; r += HORIZ_SUM_BLOCK) s = is_max ? imax(s, (long long)row[r]) : s + row[r];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long t = __shfl_xor(s, o);
    s = is_max ? imax(s, t) : s + t;
  }
  if (threadIdx.x % WAVE == 0) wacc[threadIdx.x / WAVE] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long t = 0;
#pragma unroll
    for (int w = 0; w < HORIZ_SUM_BLOCK / WAVE; ++w) t = is_max ? imax(t, wacc[w]) : t + wacc[w];
    if (b < K * HORIZ_STATS)
      stats[b] = (int64_t)t;
    else
      dropped[b - K * HORIZ_STATS] = (int64_t)t;
  }
}

template <int DG, int DP>
void launch_aux(int da, unsigned grid, int S, hipStream_t s, const HorizArgs &c) {
  const dim3 block(S * WAVE);
  if (!c.aux)
    hipLaunchKernelGGL((horizons_kernel<DG, DP, DT_NONE>), dim3(grid), block, 0, s, c);
  else if (da == CRW_DT_F32)
    hipLaunchKernelGGL((horizons_kernel<DG, DP, CRW_DT_F32>), dim3(grid), block, 0, s, c);
  else
    hipLaunchKernelGGL((horizons_kernel<DG, DP, CRW_DT_I8>), dim3(grid), block, 0, s, c);
}

inline unsigned tiles_of(int cols) { return (unsigned)((cols + WAVE - 1) / WAVE); }

// row_slabs == 0: enough waves for 12 per CU on 256 CUs (the cfg5 width of 24 576 columns: 8 slabs), slabs of at least 32 rows
inline int choose_slabs(int rows, int cols) {
  const unsigned tiles = tiles_of(cols);
  int S = tiles ? (int)((3072 + tiles - 1) / tiles) : 1;
  if (S > rows / 32) S = rows / 32;
  if (S > HORIZ_MAX_SLABS) S = HORIZ_MAX_SLABS;
  return S < 1 ? 1 : S;
}

}  // namespace
}  // namespace crw

extern "C" size_t crw_horizons_ws_bytes(int rows, int cols, int K) {
  if (K < 2 || K > 16 || rows < 0 || rows > crw::HORIZ_MAX_ROWS || cols < 0) return 0;
  return crw::align_up((size_t)crw::tiles_of(cols) * (size_t)(K * crw::HORIZ_STATS + 2) * sizeof(int64_t), 16);
}

extern "C" int crw_horizons(const void *gt, int gt_dtype, const void *pred, int pred_dtype, const void *aux, int aux_dtype, int rows,
                            int cols, size_t ld, int K, int ignore_gt, int ignore_pred, int ignore_aux, int min_run, int tol,
                            int row_slabs, int32_t *picks, int64_t *stats, int64_t *dropped, void *ws, size_t ws_bytes,
                            crw_stream_t stream) {
  using namespace crw;
  clear_stale_error();
  if (K < 2 || K > 16 || !stats || !dropped || !dtype_ok(gt_dtype) || !dtype_ok(pred_dtype) || (aux && !dtype_ok(aux_dtype)))
    return CRW_EINVAL;
  if (rows < 0 || rows > HORIZ_MAX_ROWS || cols < 0 || ld < (size_t)cols || min_run < 1 || tol < 0 || row_slabs < 0 ||
      row_slabs > HORIZ_MAX_SLABS)
    return CRW_EINVAL;
  const bool pixels = rows > 0 && cols > 0;
  if (pixels && (!gt || !pred)) return CRW_EINVAL;
  if (ignore_gt < -1 || ignore_pred < -1 || ignore_aux < -1 || (!aux && ignore_aux != -1)) return CRW_EINVAL;
  if ((gt_dtype == CRW_DT_F32 && ((uintptr_t)gt & 3)) || (pred_dtype == CRW_DT_F32 && ((uintptr_t)pred & 3)) ||
      (aux && aux_dtype == CRW_DT_F32 && ((uintptr_t)aux & 3)) || ((uintptr_t)stats & 7) || ((uintptr_t)dropped & 7) ||
      ((uintptr_t)picks & 3))
    return CRW_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = tiles_of(cols);
  if (grid) {
    if (!ws || ((uintptr_t)ws & 7)) return CRW_EINVAL;
    if (ws_bytes < crw_horizons_ws_bytes(rows, cols, K)) return CRW_EWORKSPACE;
    HorizArgs c;
    c.gt = gt, c.pred = pred, c.aux = pixels ? aux : nullptr, c.rows = rows, c.cols = cols, c.ld = ld, c.K = K;
    c.S = row_slabs ? row_slabs : choose_slabs(rows, cols);
    if (c.S > rows) c.S = rows < 1 ? 1 : rows;
    c.ig = ignore_gt < 0 ? IGNORE_NONE : ignore_gt;
    c.ip = ignore_pred < 0 ? IGNORE_NONE : ignore_pred;
    c.ia = ignore_aux < 0 ? IGNORE_NONE : ignore_aux;
    c.min_run = min_run, c.tol = tol, c.picks = picks, c.part = static_cast<int64_t *>(ws);
    if (gt_dtype == CRW_DT_F32 && pred_dtype == CRW_DT_F32)
      launch_aux<CRW_DT_F32, CRW_DT_F32>(aux_dtype, grid, c.S, s, c);
    else if (gt_dtype == CRW_DT_F32)
      launch_aux<CRW_DT_F32, CRW_DT_I8>(aux_dtype, grid, c.S, s, c);
    else if (pred_dtype == CRW_DT_F32)
      launch_aux<CRW_DT_I8, CRW_DT_F32>(aux_dtype, grid, c.S, s, c);
    else
      launch_aux<CRW_DT_I8, CRW_DT_I8>(aux_dtype, grid, c.S, s, c);
    CRW_TRY(check_launch());
  }
  hipLaunchKernelGGL(horizons_sum_kernel, dim3(K * HORIZ_STATS + 2), dim3(HORIZ_SUM_BLOCK), 0, s, static_cast<const int64_t *>(ws), grid,
                     K, stats, dropped);
  return check_launch();
}
