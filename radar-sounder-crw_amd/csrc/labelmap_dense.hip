// Pixel-resolution label map from the soft labels of crw_labelprop_propagate (L [T*N, M], one probability row per node): the
// rows are interpolated bilinearly to [rows, cols] (half-pixel convention, the node is the centre of the cell it owns under the
// nearest stretch) and arg-maxed AFTER that -- the upstream routine's order (imported/crw.py:124-127), which the radar scripts
// replaced by arg-max + nearest.  The interpolated probabilities [M, rows, cols] are never written: a pixel's row lives in
// registers, the outputs are the label (fp32 or int8) and, optionally, the confidence of the interpolated row.
//
// Shape.  The kernel is bound by its stores (1 or 4 [+ 4] bytes per pixel); its input is small -- 295 KB for T = 256, N = 48,
// M = 6, well inside one XCD's 4 MiB L2 -- and a workgroup's tile of 16 rows x 256 columns touches a handful of nodes (4 x 10 at
// 410 x 8192), which stay in the CU's L1: the node rows are read straight from memory, lanes of a wave mostly from the same
// address, and a lane reads them once for consecutive pixels between the same knots.  What IS staged in LDS is the one expensive
// thing per pixel, the 64-bit integer division behind every knot: a workgroup computes the knots and weights of its 16 rows and
// 256 (+ 3) columns once, one division per thread, and every pixel looks its two up.
//
// A lane owns 4 consecutive pixels of a row that start on a 16-byte boundary of the fp32 outputs (a 4-byte boundary of an int8
// map) and writes each output with one vector store; the groups that stick out of the window at a row's head and tail -- the map
// may be a column window of a wider one, any pitch, any offset -- write their inside pixels one by one.  Plain stores only.
//
// crw_labelmap_dense_batch is the same map for the G configurations of a parameter sweep in one launch: the same kernel text
// (stage_knots, dense_row) with a loop over the configurations around a row.
//
// crw_labelmap_ordered[_batch] (the second half of this file) decode the same interpolated probabilities under a layer order: per
// pixel column the labelling that is monotone in `order` and maximises the sum of the probabilities it picks -- a dynamic
// programme down the column, a lane per column.  They live here because they read the pixels through knot, load_row and
// dense_pixel of this file; their own text starts at "ordered label maps".  crw_labelmap_ordered_joint[_batch] (the end of the file)
// are that decode over the interpolated rows of TWO passes, per pixel the surer one's: "joint ordered label maps".
// crw_labelmap_ordered_posterior / crw_labelmap_ordered_joint_posterior (after those) are the posterior over the monotone paths that
// the order defines, on the same evidence: per-pixel confidence of a decoded map and per-column error bars of its horizons; their
// _batch forms serve the G configurations of a sweep in one launch of the same kernel.
#include <cstdlib>
#include <type_traits>

#include "confidence_of.h"
#include "labelmap.h"

namespace crw {
using namespace labelmap;
namespace {

constexpr int DN_BLOCK = 256;                  // 4 waves, one row each per step
constexpr int DN_WAVES = DN_BLOCK / WAVE;
constexpr int DN_LANE_PIX = 4;                 // pixels per lane
constexpr int DN_COLS = WAVE * DN_LANE_PIX;    // columns per workgroup
constexpr int DN_ROWS = 16;                    // rows per workgroup
constexpr int DN_COL_KNOTS = DN_COLS + DN_LANE_PIX - 1;  // + the 3 columns a row's phase can shift the groups by

struct DenseArgs {  // L, lab, conf, lab_phase: configuration 0's
  const float *L;
  void *lab;
  float *conf;
  size_t ld;
  int T, N, M, rows, cols, flip;
  int lab_phase;  // element index (mod 4) of lab's first pixel within a 16-byte (int8: 4-byte) unit
  int conf_vec;   // conf shares that phase: 16-byte stores
  float ln_m;
  // the G configurations of crw_labelmap_dense_batch; crw_labelmap_dense is G = 1
  size_t l_stride;    // floats between the configurations' soft labels (T * N * M)
  size_t map_stride;  // elements between the configurations' windows
  int G, chunk;       // configurations, and how many of them a workgroup walks
};

struct DenseKnots {  // a workgroup's tile: the knot and weight of each of its columns and rows
  int col_j[DN_COL_KNOTS], row_i[DN_ROWS];
  float col_w[DN_COL_KNOTS], row_w[DN_ROWS];
};

// Knot and weight of output index x on an axis of `n_out` pixels over `n_in` nodes, in integers: a = (2x + 1) n_in - n_out over
// d = 2 n_out.  The knot is exact, the weight the correctly rounded quotient of two integers below 2^24.
__device__ inline void knot(int x, int n_in, int n_out, int *i0, float *w) {
  const long a = (2l * x + 1) * n_in - n_out, d = 2l * n_out;
  *i0 = 0, *w = 0.f;
  if (a <= 0) return;
  const long q = a / d;
  if (q >= n_in - 1) {
    *i0 = n_in - 1;
    return;
  }
  *i0 = (int)q;
  *w = (float)(a - q * d) / (float)d;
}

template <int MCAP>
__device__ inline void load_row(const float *__restrict__ row, int M, int vec, float (&p)[MCAP]) {
  if (vec == 4) {
#pragma unroll
    for (int m = 0; m < MCAP; m += 4)
      if (m < M) {
        const float4 v = *reinterpret_cast<const float4 *>(row + m);
        p[m] = v.x, p[m + 1] = v.y, p[m + 2] = v.z, p[m + 3] = v.w;
      }
  } else if (vec == 2) {
#pragma unroll
    for (int m = 0; m < MCAP; m += 2)
      if (m < M) {
        const float2 v = *reinterpret_cast<const float2 *>(row + m);
        p[m] = v.x, p[m + 1] = v.y;
      }
  } else {
#pragma unroll
    for (int m = 0; m < MCAP; ++m)
      if (m < M) p[m] = row[m];
  }
}

// One step of the interpolation, u = 1 - w: u * a + w * b.  The ONE text of this arithmetic: dense_pixel takes its three steps
// through it, and so do ordered_sides / ordered_values.  One text is not yet one result: left to itself the compiler contracts
// a * b + c * d to FMAs site by site (and turns (1 - w) * p into fma(-w, p, p)), differently in two instantiations and even
// between the pixels of one lane.  So the roundings are written out -- one product rounded, the other fused into the sum -- and
// contraction is off here.
__device__ __forceinline__ float dense_lerp(float w, float u, float a, float b) {
#pragma clang fp contract(off)
  return __builtin_fmaf(w, b, u * a);
}

// One pixel: its row interpolated between the four node rows (three dense_lerp steps per class), the arg-max (strict: a tie
// keeps the lowest class) and the confidence of the interpolated row.  Instantiated by every shape of the kernel.
template <int KIND, int MCAP>
__device__ __forceinline__ void dense_pixel(const float (&p00)[MCAP], const float (&p01)[MCAP], const float (&p10)[MCAP],
                                            const float (&p11)[MCAP], float wc, float wr, int M, float ln_m, float *lab,
                                            float *conf) {
  const float uc = 1.f - wc, ur = 1.f - wr;
  float v[16], top1 = 0.f;
  int best = 0;
#pragma unroll
  for (int m = 0; m < 16; ++m) {
    v[m] = 0.f;
    if (m < MCAP && m < M) {
      const float top = dense_lerp(wc, uc, p00[m], p01[m]);
      const float bot = dense_lerp(wc, uc, p10[m], p11[m]);
      v[m] = dense_lerp(wr, ur, top, bot);
      if (m == 0 || v[m] > top1) top1 = v[m], best = m;  // strict: a tie keeps the lowest class
    }
  }
  *lab = (float)best;
  *conf = KIND >= 0 ? confidence_of<(KIND >= 0 ? KIND : 0)>(v, M, ln_m) : 0.f;
}

// The knots and weights of the workgroup's 16 rows and 256 (+ 3) columns, one division per thread; they depend on the geometry
// alone.  Ends in the barrier after which every thread may read them.
__device__ inline void stage_knots(const DenseArgs &a, int row0, long colb, DenseKnots &k) {
  for (int i = threadIdx.x; i < DN_COL_KNOTS + DN_ROWS; i += DN_BLOCK) {
    int i0 = 0;
    float w = 0.f;
    if (i < DN_COL_KNOTS) {
      const long c = colb + i;
      if (c >= 0 && c < a.cols) knot(a.flip ? a.cols - 1 - (int)c : (int)c, a.T, a.cols, &i0, &w);
      k.col_j[i] = i0, k.col_w[i] = w;  // outside the window: node 0, never stored
    } else {
      const int r = row0 + (i - DN_COL_KNOTS);
      if (r < a.rows) knot(r, a.N, a.rows, &i0, &w);
      k.row_i[i - DN_COL_KNOTS] = i0, k.row_w[i - DN_COL_KNOTS] = w;
    }
  }
  __syncthreads();
}

// One row of one configuration: this lane's 4 pixels between the node rows i0 / i1 (weight wr) of the soft labels L, stored at
// `off` elements behind lab / conf (the row's start in the configuration's window).  The store phase, and with it the
// lane-to-column assignment and the row's head and tail, follows from `off`: neither the pitch nor the map stride need be a
// multiple of 4.
// KIND: a CRW_CONF_* kind, or -1 for no confidence map; MCAP: 4, 8 or 16 >= M, the classes a lane keeps registers for
template <typename LAB, int KIND, int MCAP>
__device__ __forceinline__ void dense_row(const DenseArgs &a, const DenseKnots &k, const float *__restrict__ L, size_t off,
                                          long colb, int lane, int i0, int i1, float wr) {
  const int M = a.M, N = a.N;
  const int vec = ((M & 3) == 0 && !((uintptr_t)L & 15)) ? 4 : ((M & 1) == 0 && !((uintptr_t)L & 7)) ? 2 : 1;
  LAB *lab = static_cast<LAB *>(a.lab) + off;
  float *conf = KIND >= 0 ? a.conf + off : nullptr;
  const int phase = (int)((a.lab_phase + off) & (DN_LANE_PIX - 1));
  const int kx = DN_LANE_PIX * lane - phase + (DN_LANE_PIX - 1);  // this lane's first entry of col_*
  const long c0 = colb + kx;                                      // its first column: -3 ... cols + 2
  if (c0 >= a.cols) return;

  float p00[MCAP], p01[MCAP], p10[MCAP], p11[MCAP];
  float lab4[DN_LANE_PIX], conf4[DN_LANE_PIX];
  int pj0 = -1, pj1 = -1;
#pragma unroll
  for (int e = 0; e < DN_LANE_PIX; ++e) {
    const int j0 = k.col_j[kx + e], j1 = j0 + 1 < a.T ? j0 + 1 : a.T - 1;
    const float wc = k.col_w[kx + e];
    if (j0 != pj0 || j1 != pj1) {  // consecutive pixels mostly sit between the same two frames
      load_row(L + ((size_t)j0 * N + i0) * M, M, vec, p00);
      load_row(L + ((size_t)j1 * N + i0) * M, M, vec, p01);
      load_row(L + ((size_t)j0 * N + i1) * M, M, vec, p10);
      load_row(L + ((size_t)j1 * N + i1) * M, M, vec, p11);
      pj0 = j0, pj1 = j1;
    }
    dense_pixel<KIND, MCAP>(p00, p01, p10, p11, wc, wr, M, a.ln_m, &lab4[e], &conf4[e]);
  }

  if (c0 >= 0 && c0 + DN_LANE_PIX <= a.cols) {  // a whole group: its first pixel sits on the vector boundary
    if (sizeof(LAB) == 4) {
      *reinterpret_cast<float4 *>(lab + c0) = make_float4(lab4[0], lab4[1], lab4[2], lab4[3]);
    } else {
      const uint32_t pk = (uint32_t)lab4[0] | (uint32_t)lab4[1] << 8 | (uint32_t)lab4[2] << 16 | (uint32_t)lab4[3] << 24;
      *reinterpret_cast<uint32_t *>(lab + c0) = pk;
    }
    if (KIND >= 0) {
      if (a.conf_vec) {  // conf shares the labels' phase in configuration 0, hence in every one
        *reinterpret_cast<float4 *>(conf + c0) = make_float4(conf4[0], conf4[1], conf4[2], conf4[3]);
      } else {
#pragma unroll
        for (int e = 0; e < DN_LANE_PIX; ++e) conf[c0 + e] = conf4[e];
      }
    }
  } else {  // head or tail of the row: the pixels inside the window, one by one
#pragma unroll
    for (int e = 0; e < DN_LANE_PIX; ++e) {
      const long c = c0 + e;
      if (c >= 0 && c < a.cols) {
        lab[c] = (LAB)lab4[e];
        if (KIND >= 0) conf[c] = conf4[e];
      }
    }
  }
}

// BATCH: the G configurations of a sweep's pass in ONE launch, L [G, T*N, M], configuration g's window `map_stride` elements behind
// configuration g - 1's.  A workgroup stages the knots of its 16 x 256 tile ONCE and walks `chunk` configurations with them
// (blockIdx.z: the chunk); chunk = 1 is the plain "one configuration per blockIdx.z" shape.  What changes with g: the four node
// rows (another slice of L), the output address, and with it the store phase -- exactly those of the one-map kernel on slice g's
// own base.  Without BATCH: one map, no loop.
template <typename LAB, int KIND, int MCAP, bool BATCH>
__global__ __launch_bounds__(DN_BLOCK) void labelmap_dense_kernel(DenseArgs a) {
  __shared__ DenseKnots k;
  const int row0 = blockIdx.x * DN_ROWS;
  const long colb = (long)blockIdx.y * DN_COLS - (DN_LANE_PIX - 1);  // column of col_*[0]
  stage_knots(a, row0, colb, k);

  const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
  const int g0 = blockIdx.z * a.chunk, g1 = g0 + a.chunk < a.G ? g0 + a.chunk : a.G;
  for (int rr = wave; rr < DN_ROWS; rr += DN_WAVES) {
    const int r = row0 + rr;
    if (r >= a.rows) break;
    const int i0 = k.row_i[rr], i1 = i0 + 1 < a.N ? i0 + 1 : a.N - 1;
    const float wr = k.row_w[rr];
    const size_t rowoff = (size_t)r * a.ld;
    if (BATCH) {
      for (int g = g0; g < g1; ++g)
        dense_row<LAB, KIND, MCAP>(a, k, a.L + (size_t)g * a.l_stride, (size_t)g * a.map_stride + rowoff, colb, lane, i0, i1, wr);
    } else {
      dense_row<LAB, KIND, MCAP>(a, k, a.L, rowoff, colb, lane, i0, i1, wr);
    }
  }
}

// The instantiation of either kernel family for a label dtype, a confidence kind (-1: none) and M classes: pick(LAB{}, KIND,
// MCAP), the two numbers as integral constants, MCAP the smallest of 4 / 8 / 16 that holds M.
template <int V>
using int_c = std::integral_constant<int, V>;

template <typename PICK>
auto kernel_for(int label_dtype, int kind, int M, PICK pick) {
  const auto by_m = [&](auto lab, auto k) {
    return M > 4 ? (M <= 8 ? pick(lab, k, int_c<8>{}) : pick(lab, k, int_c<16>{})) : pick(lab, k, int_c<4>{});
  };
  const auto by_kind = [&](auto lab) {
    return kind < 0 ? by_m(lab, int_c<-1>{})
                    : kind == CRW_CONF_MAXPROB ? by_m(lab, int_c<CRW_CONF_MAXPROB>{})
                    : kind == CRW_CONF_MARGIN ? by_m(lab, int_c<CRW_CONF_MARGIN>{}) : by_m(lab, int_c<CRW_CONF_ENTROPY>{});
  };
  return label_dtype == CRW_DT_F32 ? by_kind(float{}) : by_kind(int8_t{});
}

// configurations a workgroup walks with one set of knots: fastest or tied of 1 / 2 / 4 / 8 at G = 60, 410 x 3200, 5 - 17 % ahead of
// one configuration per blockIdx.z (tools/sweep_dense_timing.py, profiles/sweep_dense_timing.log)
constexpr int DN_BATCH_CHUNK = 4;

// CRW_DENSE_BATCH_CHUNK (read per call): the other kernel shapes, for the A/B of tools/sweep_dense_timing.py; 1 = one
// configuration per blockIdx.z.  The maps do not depend on it.
int batch_chunk(int G) {
  int chunk = DN_BATCH_CHUNK;
  if (const char *e = getenv("CRW_DENSE_BATCH_CHUNK")) {
    const int v = atoi(e);
    if (v >= 1) chunk = v;
  }
  return chunk < G ? chunk : G;
}

constexpr int MAX_SIDE = 1 << 22;  // 2 * side < 2^24: the weights' numerators and denominators are exact in fp32

// The arguments the dense and the ordered entry points share: checked (CRW_EINVAL), then written into `a`.  lab_phase and
// conf_vec are the dense kernels'; the ordered ones do not read them.
int dense_args(const float *L, int G, int T, int N, int M, int rows, int cols, int flip, int conf_kind, void *labels,
               int label_dtype, float *conf, size_t ld, size_t map_stride, int chunk, DenseArgs &a) {
  if (!L || !labels || G < 1 || G > 65535 || T < 1 || N < 1 || M < 2 || M > 16 || rows < 1 || cols < 1 || rows > MAX_SIDE ||
      cols > MAX_SIDE || !dtype_ok(label_dtype) || conf_kind < -1 || conf_kind > CRW_CONF_ENTROPY ||
      (conf_kind == -1) != (conf == nullptr) || ld < (size_t)cols || map_stride < (size_t)(rows - 1) * ld + (size_t)cols ||
      ((uintptr_t)L & 3) || ((uintptr_t)conf & 3) || (label_dtype == CRW_DT_F32 && ((uintptr_t)labels & 3)))
    return CRW_EINVAL;  // (a slice's base is configuration 0's plus whole elements: 4-byte aligned when that is)
  a.L = L, a.lab = labels, a.conf = conf, a.ld = ld;
  a.T = T, a.N = N, a.M = M, a.rows = rows, a.cols = cols, a.flip = flip != 0;
  a.lab_phase = (int)(((uintptr_t)labels / elem(label_dtype)) & (DN_LANE_PIX - 1));
  a.conf_vec = conf && (int)(((uintptr_t)conf / 4) & (DN_LANE_PIX - 1)) == a.lab_phase;
  a.ln_m = logf((float)M);
  a.l_stride = (size_t)T * N * M, a.map_stride = map_stride, a.G = G, a.chunk = chunk;
  return CRW_OK;
}

// Both entry points behind their signatures: the argument checks, the kernel's arguments, the launch.  `chunk`: the
// configurations a workgroup walks (the one-map entry point: G = 1, chunk = 1).
template <bool BATCH>
int dense_launch(const float *L, int G, int T, int N, int M, int rows, int cols, int flip, int conf_kind, void *labels,
                 int label_dtype, float *conf, size_t ld, size_t map_stride, int chunk, crw_stream_t stream) {
  clear_stale_error();
  DenseArgs a;
  if (const int st = dense_args(L, G, T, N, M, rows, cols, flip, conf_kind, labels, label_dtype, conf, ld, map_stride, chunk, a)) return st;
  // a row's groups: ceil((cols + phase) / 4) <= (cols + 3 + 3) / 4
  const unsigned groups = ((unsigned)cols + 2 * (DN_LANE_PIX - 1)) / DN_LANE_PIX;
  const dim3 grid(((unsigned)rows + DN_ROWS - 1) / DN_ROWS, (groups + WAVE - 1) / WAVE, ((unsigned)G + chunk - 1) / chunk);
  const auto kernel = kernel_for(label_dtype, conf_kind, M, [](auto lab, auto kind, auto mcap) {
    return labelmap_dense_kernel<decltype(lab), kind(), mcap(), BATCH>;
  });
  if constexpr (!BATCH) CRW_ROUTE("dense.single");
  else if (chunk > 1) CRW_ROUTE("dense.batch_chunked");
  else CRW_ROUTE("dense.batch_chunk1");
  hipLaunchKernelGGL(kernel, grid, dim3(DN_BLOCK), 0, (hipStream_t)stream, a);
  return check_launch();
}

}  // namespace
}  // namespace crw

extern "C" int crw_labelmap_dense_batch(const float *L, int G, int T, int N, int M, int rows, int cols, int flip, int conf_kind,
                                        void *labels, int label_dtype, float *conf, size_t ld, size_t map_stride,
                                        crw_stream_t stream) {
  return crw::dense_launch<true>(L, G, T, N, M, rows, cols, flip, conf_kind, labels, label_dtype, conf, ld, map_stride,
                                 crw::batch_chunk(G), stream);
}

extern "C" int crw_labelmap_dense(const float *L, int T, int N, int M, int rows, int cols, int flip, int conf_kind, void *labels,
                                  int label_dtype, float *conf, size_t ld, crw_stream_t stream) {
  // one map: nothing behind it to overlap, so any stride that covers it (checked: ld >= cols) serves
  return crw::dense_launch<false>(L, 1, T, N, M, rows, cols, flip, conf_kind, labels, label_dtype, conf, ld, (size_t)rows * ld, 1, stream);
}

// ------------------------------------------------------------------------------------------------------------ ordered label maps
// The labelling of a pixel column that respects a layer order.  order[0 ... S-1]: distinct classes, top to bottom; e[r][s] =
// v[r][c][order[s]], v the interpolated probability of dense_pixel.  In fp32, one rounded add per row:
//   D[0][s] = e[0][s];  D[r][s] = e[r][s] + max_{s' <= s} D[r-1][s'],  predecessor: the LOWEST s' that attains the prefix maximum;
//   last state: the LOWEST s that attains max_s D[rows-1][s];  backtrack;  label[r] = order[state[r]].
// The prefix arg-max does not decrease with s, so ONE bit per (row, state) -- "state s is a new prefix maximum" (strict >, bit 0
// always set) -- is the whole back-pointer: pred(s) = the highest set bit <= s.  A pixel's 16 bits are a uint16 word in the
// caller's workspace, [G][rows][cols rounded up to 64]: a wave's row of words is one 128-byte segment.
//
// Shape.  One lane per pixel column, one wave (= one workgroup) per 64 columns and configuration, ONE route for every size.  The
// lane's column knot never changes; the row knots are the wave's (64 at a time, one division per lane, handed round by readlane),
// and the four node rows are loaded once per run of rows between the same two of them (rows / N rows), outside the loop over the
// run: vector-memory operations return in order here, so a load inside it would make every row wait for the row before to
// store.  The lane keeps the node rows twice: permuted by `order` (S entries, what the scan adds) and, with a confidence kind,
// whole (what dense_pixel's confidence reads: conf does not depend on the decode and is dense_pixel's own, bit for bit).
// Forward: D[S] in registers, a word and a conf store per row.
// Backward: the words back, one label store per row -- a wave's row is one 64-byte (int8) or 256-byte (fp32) segment at any
// pitch, offset and phase, so there is no head or tail.  A lane reads only words it wrote itself: whatever the workspace held
// before is never read.  rows steps in series on cols / 64 waves: the kernel is bound by the latency of one step, not by memory
// (96 µs at 410 x 8192, M = 4, int8, where crw_labelmap_dense takes 10.6: profiles/ordered_timing.log).  The tests hold the map to
// feasibility and to an fp64 score within 2 (rows B + (rows^2 + 2 rows) 2^-25) of the optimum, B = 12 * 2^-24 the bound on an
// interpolated probability (DESIGN.md section 3b derives it).  Not measured: anything on a real radargram.
namespace crw {
namespace {

constexpr int OD_CHUNK = WAVE;  // row knots the wave holds at a time, a lane each
// back-pointer words the backward scan has in flight: its step is one dependent load otherwise (a label store of an int8 map may
// alias anything, so the compiler keeps load and store in order).  8 against 1: tools/ordered_timing.py, profiles/ordered_timing.log
constexpr int OD_BACK = 8;

struct OrderedArgs {
  DenseArgs d;          // lab_phase, conf_vec, chunk: unused
  uint64_t order;       // order[s] in bits 4s ... 4s + 3
  int S;
  uint16_t *ws;         // [G][rows][ws_ld]
  size_t ws_ld;         // cols rounded up to a multiple of 64
  int back;             // 1: the backward scan loads a word per step; otherwise OD_BACK words at a time
};

__device__ __forceinline__ int order_at(uint64_t order, int s) { return (int)(order >> (4 * s)) & 15; }

// The S entries of a node row that `order` names, in its order.
template <int SCAP>
__device__ __forceinline__ void load_ordered(const float *__restrict__ row, uint64_t order, int S, float (&p)[SCAP]) {
#pragma unroll
  for (int s = 0; s < SCAP; ++s)
    if (s < S) p[s] = row[order_at(order, s)];
}

// dense_pixel's interpolated values for the first S entries of the four rows -- its three dense_lerp steps: on rows permuted by
// load_ordered, e[s] is bit for bit the v[order[s]] dense_pixel computes (one text, and fmaf and a rounded product leave the
// compiler no choice).  In two halves, because a lane's column never changes: the first two steps once per pair of node rows
// (ordered_sides), the third once per pixel (ordered_values).
template <int SCAP>
__device__ __forceinline__ void ordered_sides(const float (&p00)[SCAP], const float (&p01)[SCAP], const float (&p10)[SCAP],
                                              const float (&p11)[SCAP], float wc, int S, float (&top)[SCAP], float (&bot)[SCAP]) {
  const float uc = 1.f - wc;
#pragma unroll
  for (int s = 0; s < SCAP; ++s) {
    top[s] = bot[s] = 0.f;
    if (s < S) {
      top[s] = dense_lerp(wc, uc, p00[s], p01[s]);
      bot[s] = dense_lerp(wc, uc, p10[s], p11[s]);
    }
  }
}

template <int SCAP>
__device__ __forceinline__ void ordered_values(const float (&top)[SCAP], const float (&bot)[SCAP], float wr, int S, float (&e)[SCAP]) {
  const float ur = 1.f - wr;
#pragma unroll
  for (int s = 0; s < SCAP; ++s) e[s] = s < S ? dense_lerp(wr, ur, top[s], bot[s]) : -INFINITY;  // beyond S: never a maximum
}

// lane `l` (uniform) of a value every lane holds, dead lanes included
__device__ __forceinline__ int lane_int(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ float lane_float(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// One row of the scan: D[r-1] -> D[r] under e[r], and the row's back-pointer word.  Adds, compares and selects only: nothing
// here can contract, nothing branches.  A state beyond S has e = -inf, so its D is -inf from row 0 on: never a prefix maximum,
// never the last state.
template <int MCAP>
__device__ __forceinline__ unsigned ordered_step(float (&D)[MCAP], const float (&e)[MCAP]) {
  float best = D[0];
  unsigned word = 1u;
  D[0] = e[0] + best;
#pragma unroll
  for (int s = 1; s < MCAP; ++s) {
    const bool up = D[s] > best;  // strict: the lowest state that attains the prefix maximum
    best = up ? D[s] : best;
    word |= up ? 1u << s : 0u;
    D[s] = e[s] + best;
  }
  return word;
}

// The backward scan of a live lane: the last state from D[rows-1], then up the column through the lane's own words; lab and ws
// are the lane's column (row 0), `back` OrderedArgs'.
template <typename LAB, int MCAP>
__device__ __forceinline__ void ordered_backtrack(const float (&D)[MCAP], LAB *lab, size_t ld, const uint16_t *ws, size_t ws_ld,
                                                  uint64_t order, int back, int rows) {
  int state = 0;
  float top = D[0];
#pragma unroll
  for (int s = 1; s < MCAP; ++s)
    if (D[s] > top) top = D[s], state = s;  // strict: the lowest state that attains the maximum (beyond S: -inf)
  int r = rows - 1;
  if (back != 1)
    for (; r >= OD_BACK; r -= OD_BACK) {  // rows r ... r - 7, all >= 1: their words first, then the chain through them
      unsigned words[OD_BACK];
#pragma unroll
      for (int k = 0; k < OD_BACK; ++k) words[k] = ws[(size_t)(r - k) * ws_ld];
#pragma unroll
      for (int k = 0; k < OD_BACK; ++k) {
        lab[(size_t)(r - k) * ld] = (LAB)order_at(order, state);
        state = 31 - __builtin_clz(words[k] & ((2u << state) - 1u));
      }
    }
  for (; r >= 1; --r) {
    lab[(size_t)r * ld] = (LAB)order_at(order, state);
    const unsigned word = ws[(size_t)r * ws_ld] & ((2u << state) - 1u);  // bit 0 is set: never empty
    state = 31 - __builtin_clz(word);
  }
  lab[0] = (LAB)order_at(order, state);
}

// KIND: a CRW_CONF_* kind, or -1 for no confidence map; MCAP: 4, 8 or 16 >= M >= S
template <typename LAB, int KIND, int MCAP>
__global__ __launch_bounds__(WAVE) void labelmap_ordered_kernel(OrderedArgs a) {
  const DenseArgs &d = a.d;
  const int M = d.M, N = d.N, S = a.S, rows = d.rows;
  const int lane = threadIdx.x, g = blockIdx.y;
  const long c = (long)blockIdx.x * WAVE + lane;
  const bool live = c < d.cols;  // a dead lane holds row knots and touches no memory
  const float *__restrict__ L = d.L + (size_t)g * d.l_stride;
  const int vec = ((M & 3) == 0 && !((uintptr_t)L & 15)) ? 4 : ((M & 1) == 0 && !((uintptr_t)L & 7)) ? 2 : 1;
  LAB *lab = static_cast<LAB *>(d.lab) + (size_t)g * d.map_stride + (live ? c : 0);
  float *conf = KIND >= 0 ? d.conf + (size_t)g * d.map_stride + (live ? c : 0) : nullptr;
  uint16_t *ws = a.ws + (size_t)g * rows * a.ws_ld + (live ? c : 0);

  int j0 = 0;
  float wc = 0.f;
  if (live) knot(d.flip ? d.cols - 1 - (int)c : (int)c, d.T, d.cols, &j0, &wc);
  const int j1 = j0 + 1 < d.T ? j0 + 1 : d.T - 1;

  // D[-1] = 0: row 0 is a step like every other, D[0][s] = e[0][s] + 0 exactly (its back-pointer word is written and never read)
  float D[MCAP];
#pragma unroll
  for (int s = 0; s < MCAP; ++s) D[s] = 0.f;
  for (int r0 = 0; r0 < rows; r0 += OD_CHUNK) {
    int ki = 0;  // row r0 + lane's knot and weight: one division per lane and 64 rows, handed round by readlane
    float kw = 0.f;
    if (r0 + lane < rows) knot(r0 + lane, N, rows, &ki, &kw);
    const int rn = rows - r0 < OD_CHUNK ? rows - r0 : OD_CHUNK;
    if (!live) continue;
    for (int rr = 0; rr < rn;) {  // a run of rows between the same two node rows (rows / N of them)
      const int i0 = lane_int(ki, rr), i1 = i0 + 1 < N ? i0 + 1 : N - 1;
      const float *n00 = L + ((size_t)j0 * N + i0) * M, *n01 = L + ((size_t)j1 * N + i0) * M;
      const float *n10 = L + ((size_t)j0 * N + i1) * M, *n11 = L + ((size_t)j1 * N + i1) * M;
      float q00[MCAP], q01[MCAP], q10[MCAP], q11[MCAP];  // the node rows permuted by order: the scan's
      float p00[MCAP], p01[MCAP], p10[MCAP], p11[MCAP];  // the whole node rows: the confidence's
      load_ordered(n00, a.order, S, q00), load_ordered(n01, a.order, S, q01);
      load_ordered(n10, a.order, S, q10), load_ordered(n11, a.order, S, q11);
      if (KIND >= 0) {
        load_row(n00, M, vec, p00), load_row(n01, M, vec, p01);
        load_row(n10, M, vec, p10), load_row(n11, M, vec, p11);
      }
      float top[MCAP], bot[MCAP], e[MCAP];
      ordered_sides(q00, q01, q10, q11, wc, S, top, bot);
      do {  // no load in here: the stores of one row need not land before the next row starts
        const int r = r0 + rr;
        const float wr = lane_float(kw, rr);
        ordered_values(top, bot, wr, S, e);
        if (KIND >= 0) {
          float argmax_label, cf;
          dense_pixel<KIND, MCAP>(p00, p01, p10, p11, wc, wr, M, d.ln_m, &argmax_label, &cf);
          conf[(size_t)r * d.ld] = cf;
        }
        ws[(size_t)r * a.ws_ld] = (uint16_t)ordered_step(D, e);
        ++rr;
      } while (rr < rn && lane_int(ki, rr) == i0);
    }
  }
  if (live) ordered_backtrack(D, lab, d.ld, ws, a.ws_ld, a.order, a.back, rows);
}

// CRW_ORDERED_BACK (read per call): 1 = the backward scan with one word in flight, the other arm of tools/ordered_timing.py's
// A/B.  The maps do not depend on it.
int ordered_back() {
  const char *e = getenv("CRW_ORDERED_BACK");
  return e && atoi(e) == 1 ? 1 : OD_BACK;
}

size_t ordered_ws_ld(int cols) { return ((size_t)cols + WAVE - 1) / WAVE * WAVE; }

size_t ordered_ws_bytes(int G, int rows, int cols) {
  if (G < 1 || rows < 1 || cols < 1) return 0;
  return (size_t)G * rows * ordered_ws_ld(cols) * sizeof(uint16_t);
}

// The order of a decode over the M classes of a.d: checked (CRW_EINVAL), then packed into `a`.
int ordered_order(const int *order, int S, OrderedArgs &a) {
  const int M = a.d.M;
  if (!order || S < 2 || S > M) return CRW_EINVAL;
  uint64_t packed = 0;
  unsigned seen = 0;
  for (int s = 0; s < S; ++s) {
    if (order[s] < 0 || order[s] >= M || (seen >> order[s] & 1)) return CRW_EINVAL;
    seen |= 1u << order[s];
    packed |= (uint64_t)order[s] << (4 * s);
  }
  a.order = packed, a.S = S;
  return CRW_OK;
}

// The order and the workspace of an ordered decode over the window a.d describes (G, M, rows, cols): checked (CRW_EINVAL,
// CRW_EWORKSPACE), then written into `a`.
int ordered_decode_args(const int *order, int S, void *ws, size_t ws_bytes, OrderedArgs &a) {
  if (!ws || ((uintptr_t)ws & 1)) return CRW_EINVAL;
  if (const int st = ordered_order(order, S, a)) return st;
  if (ws_bytes < ordered_ws_bytes(a.d.G, a.d.rows, a.d.cols)) return CRW_EWORKSPACE;
  a.ws = static_cast<uint16_t *>(ws), a.ws_ld = ordered_ws_ld(a.d.cols), a.back = ordered_back();
  if (a.back == 1) CRW_ROUTE("ordered.back_one_word");  // (the last check of every ordered decode: the launch follows)
  else CRW_ROUTE("ordered.back_default");
  return CRW_OK;
}

// Both entry points behind their signatures.  The argument checks are dense_args', then the order's and the workspace's;
// nothing is launched unless all pass.
int ordered_launch(const float *L, int G, int T, int N, int M, int rows, int cols, int flip, const int *order, int S, int conf_kind,
                   void *labels, int label_dtype, float *conf, size_t ld, size_t map_stride, void *ws, size_t ws_bytes,
                   crw_stream_t stream) {
  clear_stale_error();
  OrderedArgs a;
  if (const int st = dense_args(L, G, T, N, M, rows, cols, flip, conf_kind, labels, label_dtype, conf, ld, map_stride, 1, a.d)) return st;
  if (const int st = ordered_decode_args(order, S, ws, ws_bytes, a)) return st;
  const dim3 grid((unsigned)(a.ws_ld / WAVE), (unsigned)G);
  const auto kernel = kernel_for(label_dtype, conf_kind, M, [](auto lab, auto kind, auto mcap) {
    return labelmap_ordered_kernel<decltype(lab), kind(), mcap()>;
  });
  hipLaunchKernelGGL(kernel, grid, dim3(WAVE), 0, (hipStream_t)stream, a);
  return check_launch();
}

}  // namespace
}  // namespace crw

extern "C" size_t crw_labelmap_ordered_workspace(int G, int rows, int cols) { return crw::ordered_ws_bytes(G, rows, cols); }

extern "C" int crw_labelmap_ordered_batch(const float *L, int G, int T, int N, int M, int rows, int cols, int flip, const int *order,
                                          int S, int conf_kind, void *labels, int label_dtype, float *conf, size_t ld,
                                          size_t map_stride, void *ws, size_t ws_bytes, crw_stream_t stream) {
  return crw::ordered_launch(L, G, T, N, M, rows, cols, flip, order, S, conf_kind, labels, label_dtype, conf, ld, map_stride, ws,
                             ws_bytes, stream);
}

extern "C" int crw_labelmap_ordered(const float *L, int T, int N, int M, int rows, int cols, int flip, const int *order, int S,
                                    int conf_kind, void *labels, int label_dtype, float *conf, size_t ld, void *ws, size_t ws_bytes,
                                    crw_stream_t stream) {
  return crw::ordered_launch(L, 1, T, N, M, rows, cols, flip, order, S, conf_kind, labels, label_dtype, conf, ld, (size_t)rows * ld,
                             ws, ws_bytes, stream);
}

// ------------------------------------------------------------------------------------------------------ joint ordered label maps
// The ordered decode over the evidence of TWO passes, merged before the decode: per pixel the interpolated row of the surer source
// -- crw_merge_confidence's rule, source b where conf_b > conf_a strictly, source a otherwise (a tie, a NaN) -- and ONE dynamic
// programme down the column over the selected rows.  A per-pixel merge of two monotone maps need not be monotone; this map is, by
// construction, and its conf is the confidence merge's bit for bit.
//
// A source is a pass's soft labels with its own geometry along the columns: L [G][T*N*M], T frames under a `cols`-wide map of which
// the window is the columns col0 ... col0 + ncols - 1, mirrored with flip as crw_labelmap_dense mirrors them.  (The forward side
// of a corrected tail is a shorter item's whole map, its reverse side the tail columns of the full item's.)  N, M, rows, the order
// and the outputs are shared, so the wave's row knots serve both sources; a lane has two column knots.
//
// Shape: the ordered kernel's -- a lane per column, a wave per 64 columns and configuration, the loads outside the loop over a
// run of rows, the same step, back-pointer word, workspace layout and backward scan (ordered_step, ordered_backtrack).  Per run a
// lane keeps each source's node rows lerped along the columns (ordered_sides: its column weight never changes), whole for the
// confidence and permuted by `order` for the scan: 8 arrays of MCAP floats.  Per row: two whole interpolated rows and their
// confidences, the comparison, then ONE third lerp step per state on the selected source's sides -- every value is dense_pixel's
// (the same three dense_lerp steps on the same operands).  Register arrays are indexed by unrolled loops only.
namespace crw {
namespace {

struct JointSource {
  const float *L;   // configuration 0's
  size_t l_stride;  // T * N * M
  int T, cols, col0, flip;
};

struct JointArgs {
  OrderedArgs o;  // o.d: the shared window (cols = ncols), N, M, rows and outputs; its L, T, flip and l_stride are unused
  JointSource a, b;
};

// What a lane keeps of one source: the two frames its column lies between and the weight between them.
struct JointColumn {
  const float *f0, *f1;  // node 0's rows of frames j0, j1
  float wc;
  int vec;
};

__device__ __forceinline__ JointColumn joint_column(const JointSource &s, int g, long x, bool live, int N, int M) {
  JointColumn k;
  const float *L = s.L + (size_t)g * s.l_stride;
  int j0 = 0;
  k.wc = 0.f;
  if (live) {
    const int c = s.col0 + (int)x;
    knot(s.flip ? s.cols - 1 - c : c, s.T, s.cols, &j0, &k.wc);
  }
  const int j1 = j0 + 1 < s.T ? j0 + 1 : s.T - 1;
  k.f0 = L + (size_t)j0 * N * M, k.f1 = L + (size_t)j1 * N * M;
  k.vec = ((M & 3) == 0 && !((uintptr_t)L & 15)) ? 4 : ((M & 1) == 0 && !((uintptr_t)L & 7)) ? 2 : 1;
  return k;
}

// A source's sides for the run between node rows i0 / i1: dense_pixel's first two lerp steps, on the whole rows (top, bot: M
// entries) and on the rows permuted by `order` (qtop, qbot: S entries).
template <int MCAP>
__device__ __forceinline__ void joint_sides(const JointColumn &k, int i0, int i1, int M, uint64_t order, int S, float (&top)[MCAP],
                                            float (&bot)[MCAP], float (&qtop)[MCAP], float (&qbot)[MCAP]) {
  const float *n00 = k.f0 + (size_t)i0 * M, *n01 = k.f1 + (size_t)i0 * M;
  const float *n10 = k.f0 + (size_t)i1 * M, *n11 = k.f1 + (size_t)i1 * M;
  float q00[MCAP], q01[MCAP], q10[MCAP], q11[MCAP];
  float p00[MCAP], p01[MCAP], p10[MCAP], p11[MCAP];
  load_ordered(n00, order, S, q00), load_ordered(n01, order, S, q01);
  load_ordered(n10, order, S, q10), load_ordered(n11, order, S, q11);
  load_row(n00, M, k.vec, p00), load_row(n01, M, k.vec, p01);
  load_row(n10, M, k.vec, p10), load_row(n11, M, k.vec, p11);
  ordered_sides(q00, q01, q10, q11, k.wc, S, qtop, qbot);
  ordered_sides(p00, p01, p10, p11, k.wc, M, top, bot);
}

// The confidence of a pixel's whole interpolated row: dense_pixel's third lerp step and its confidence_of.
template <int KIND, int MCAP>
__device__ __forceinline__ float joint_confidence(const float (&top)[MCAP], const float (&bot)[MCAP], float wr, int M, float ln_m) {
  const float ur = 1.f - wr;
  float v[16];
#pragma unroll
  for (int m = 0; m < 16; ++m) {
    v[m] = 0.f;
    if (m < MCAP && m < M) v[m] = dense_lerp(wr, ur, top[m < MCAP ? m : 0], bot[m < MCAP ? m : 0]);
  }
  return confidence_of<KIND>(v, M, ln_m);
}

// KIND: a CRW_CONF_* kind (there is no joint map without one); MCAP: 4, 8 or 16 >= M >= S
template <typename LAB, int KIND, int MCAP>
__global__ __launch_bounds__(WAVE) void labelmap_ordered_joint_kernel(JointArgs a) {
  const OrderedArgs &o = a.o;
  const DenseArgs &d = o.d;
  const int M = d.M, N = d.N, S = o.S, rows = d.rows;
  // kernel_for's choice of MCAP and the order's check, said to the compiler: confidence_of walks 16 classes behind `m < M`, and
  // without this the row loop keeps the 16 - MCAP steps that can never run (about 190 -> 125 instructions per row at MCAP = 4 with
  // maxprob, 338 -> 227 us per call at 410 x 8192: tools/joint_timing.py)
  __builtin_assume(M <= MCAP && S <= M);
  const int lane = threadIdx.x, g = blockIdx.y;
  const long x = (long)blockIdx.x * WAVE + lane;
  const bool live = x < d.cols;  // a dead lane holds row knots and touches no memory
  LAB *lab = static_cast<LAB *>(d.lab) + (size_t)g * d.map_stride + (live ? x : 0);
  float *conf = d.conf ? d.conf + (size_t)g * d.map_stride + (live ? x : 0) : nullptr;  // null: the labels alone
  uint16_t *ws = o.ws + (size_t)g * rows * o.ws_ld + (live ? x : 0);
  const JointColumn ka = joint_column(a.a, g, x, live, N, M), kb = joint_column(a.b, g, x, live, N, M);

  float D[MCAP];  // D[-1] = 0, as in labelmap_ordered_kernel
#pragma unroll
  for (int s = 0; s < MCAP; ++s) D[s] = 0.f;
  for (int r0 = 0; r0 < rows; r0 += OD_CHUNK) {
    int ki = 0;  // row r0 + lane's knot and weight, both sources'
    float kw = 0.f;
    if (r0 + lane < rows) knot(r0 + lane, N, rows, &ki, &kw);
    const int rn = rows - r0 < OD_CHUNK ? rows - r0 : OD_CHUNK;
    if (!live) continue;
    for (int rr = 0; rr < rn;) {  // a run of rows between the same two node rows
      const int i0 = lane_int(ki, rr), i1 = i0 + 1 < N ? i0 + 1 : N - 1;
      float ta[MCAP], ba[MCAP], qta[MCAP], qba[MCAP], tb[MCAP], bb[MCAP], qtb[MCAP], qbb[MCAP];
      joint_sides(ka, i0, i1, M, o.order, S, ta, ba, qta, qba);
      joint_sides(kb, i0, i1, M, o.order, S, tb, bb, qtb, qbb);
      do {  // no load in here, for labelmap_ordered_kernel's reason
        const int r = r0 + rr;
        const float wr = lane_float(kw, rr);
        const float ca = joint_confidence<KIND>(ta, ba, wr, M, d.ln_m), cb = joint_confidence<KIND>(tb, bb, wr, M, d.ln_m);
        const bool took = cb > ca;  // crw_merge_confidence's comparison: a tie and a NaN keep source a
        if (conf) conf[(size_t)r * d.ld] = took ? cb : ca;
        float top[MCAP], bot[MCAP], e[MCAP];
#pragma unroll
        for (int s = 0; s < MCAP; ++s) top[s] = took ? qtb[s] : qta[s], bot[s] = took ? qbb[s] : qba[s];
        ordered_values(top, bot, wr, S, e);
        ws[(size_t)r * o.ws_ld] = (uint16_t)ordered_step(D, e);
        ++rr;
      } while (rr < rn && lane_int(ki, rr) == i0);
    }
  }
  if (live) ordered_backtrack(D, lab, d.ld, ws, o.ws_ld, o.order, o.back, rows);
}

// A source's own arguments: checked (CRW_EINVAL), then written into `s`.
int joint_source(const float *L, int T, int cols, int col0, int flip, int N, int M, int ncols, JointSource &s) {
  if (!L || ((uintptr_t)L & 3) || T < 1 || cols < 1 || cols > MAX_SIDE || col0 < 0 || col0 > cols || ncols > cols - col0) return CRW_EINVAL;
  s.L = L, s.l_stride = (size_t)T * N * M, s.T = T, s.cols = cols, s.col0 = col0, s.flip = flip != 0;
  return CRW_OK;
}

// Both entry points behind their signatures.  The checks of the shared arguments are dense_args' on the window (a confidence kind
// is mandatory, the map of it is not), then each source's, the order's and the workspace's; nothing is launched unless all pass.
int joint_launch(const float *La, int Ta, int cols_a, int col0_a, int flip_a, const float *Lb, int Tb, int cols_b, int col0_b,
                 int flip_b, int G, int N, int M, int rows, int ncols, const int *order, int S, int conf_kind, void *labels,
                 int label_dtype, float *conf, size_t ld, size_t map_stride, void *ws, size_t ws_bytes, crw_stream_t stream) {
  clear_stale_error();
  JointArgs a;
  if (conf_kind < 0 || conf_kind > CRW_CONF_ENTROPY) return CRW_EINVAL;
  if (const int st = dense_args(La, G, Ta, N, M, rows, ncols, flip_a, conf ? conf_kind : -1, labels, label_dtype, conf, ld, map_stride,
                                1, a.o.d))
    return st;
  if (const int st = joint_source(La, Ta, cols_a, col0_a, flip_a, N, M, ncols, a.a)) return st;
  if (const int st = joint_source(Lb, Tb, cols_b, col0_b, flip_b, N, M, ncols, a.b)) return st;
  if (const int st = ordered_decode_args(order, S, ws, ws_bytes, a.o)) return st;
  const dim3 grid((unsigned)(a.o.ws_ld / WAVE), (unsigned)G);
  const auto kernel = kernel_for(label_dtype, conf_kind, M, [](auto lab, auto kind, auto mcap) {
    return labelmap_ordered_joint_kernel<decltype(lab), (kind() < 0 ? 0 : kind()), mcap()>;  // (kind -1 never reaches here)
  });
  hipLaunchKernelGGL(kernel, grid, dim3(WAVE), 0, (hipStream_t)stream, a);
  return check_launch();
}

}  // namespace
}  // namespace crw

extern "C" int crw_labelmap_ordered_joint_batch(const float *La, int Ta, int cols_a, int col0_a, int flip_a, const float *Lb, int Tb,
                                                int cols_b, int col0_b, int flip_b, int G, int N, int M, int rows, int ncols,
                                                const int *order, int S, int conf_kind, void *labels, int label_dtype, float *conf,
                                                size_t ld, size_t map_stride, void *ws, size_t ws_bytes, crw_stream_t stream) {
  return crw::joint_launch(La, Ta, cols_a, col0_a, flip_a, Lb, Tb, cols_b, col0_b, flip_b, G, N, M, rows, ncols, order, S, conf_kind,
                           labels, label_dtype, conf, ld, map_stride, ws, ws_bytes, stream);
}

extern "C" int crw_labelmap_ordered_joint(const float *La, int Ta, int cols_a, int col0_a, int flip_a, const float *Lb, int Tb,
                                          int cols_b, int col0_b, int flip_b, int N, int M, int rows, int ncols, const int *order,
                                          int S, int conf_kind, void *labels, int label_dtype, float *conf, size_t ld, void *ws,
                                          size_t ws_bytes, crw_stream_t stream) {
  return crw::joint_launch(La, Ta, cols_a, col0_a, flip_a, Lb, Tb, cols_b, col0_b, flip_b, 1, N, M, rows, ncols, order, S, conf_kind,
                           labels, label_dtype, conf, ld, (size_t)rows * ld, ws, ws_bytes, stream);
}

// ------------------------------------------------------------------------------------------- posterior of the ordered label maps
// The confidence that belongs to the ordered decode: the posterior over the monotone paths of a column, with the interpolated
// probabilities as independent per-row evidence (include/crw_hip.h has the definition, DESIGN.md section 3d the bound).  With
// f[r][s] = max(e[r][s], floor), e the evidence labelmap_ordered_kernel / labelmap_ordered_joint_kernel decode (the same device
// functions: ordered_sides, ordered_values, joint_sides, joint_confidence), per column in fp32:
//   forward   a[0][s] = f[0][s],  a[r][s] = f[r][s] sum_{s' <= s} A[r-1][s'],  A[r] = a[r] * (1 / sum_s a[r][s]);
//   backward  b[rows-1][s] = 1,   b[r-1][s] = sum_{s' >= s} f[r][s'] B[r][s'],  B[r] = b[r] * (1 / b[r][0])  (b does not increase with
//             s: b[r][0] is its largest entry);
//   gamma[r][s] = A[r][s] b[r][s] / Z_r,  Z_r = sum_s A[r][s] b[r][s];
//   P(B_k = r+1) = (sum_{s < k} A[r][s]) b[r][k] / Z_r  (the boundary of layer k enters at row r+1: x_r < k <= x_{r+1}; r = rows-1: it
//   never enters),  P(B_k = 0) = sum_{s >= k} gamma[0][s].
// Every output is a sum of products of non-negative numbers: nothing cancels, so a relative error of the evidence stays a relative
// error of the outputs.  Prefix sums run upwards from state 0, suffix sums downwards from state S-1, contraction is off.
//
// Shape: the ordered kernel's -- a lane per column, a wave per 64 columns, the node rows loaded once per run of rows -- except that
// no lane is ever masked off around a scan (see the kernel: the lanes behind the window repeat its last column).  ONE kernel
// text for both entry points (KIND -1: one source, no selection), one text per scan step (posterior_forward_step,
// posterior_backward_step).  Forward scan: A in registers, its S values per row stored to the workspace [row][state][column rounded
// up to 64] -- a wave's store of one state is one 256-byte segment.  Backward scan: the runs of rows bottom to top, f recomputed, b
// carried, A read back one row ahead of its use (the load is issued before the row's stores), gamma formed, post stored, the 2 (S-1)
// moments accumulated.  The picks b^_k come from one pass over the column's labels before the scans.  A lane reads only what it
// wrote: whatever the workspace held before is never read.  The _batch entry points are the same kernel with the configuration
// as blockIdx.y (a sweep's window is 50 waves, its G = 60 configurations 3000): slice g of L, of the label / post maps, of hz and
// of the workspace; the one-map entry points are G = 1 of the same launcher.
namespace crw {
namespace {

struct PosteriorArgs {
  JointArgs j;     // j.o.d: the window; d.lab the labels (READ), d.conf / o.ws / o.back unused; j.b unused by the single call
  float floor;
  float *post;     // configuration 0's [rows] x [cols] window, pitch d.ld, d.map_stride between configurations; may be null
  float *hz;       // configuration 0's [3][S-1] rows of cols values, pitch hz_ld; may be null
  size_t hz_ld, hz_stride;  // hz_stride: between configurations
  float *alpha;    // [G][rows][S][a_ld]
  size_t a_ld;     // cols rounded up to a multiple of 64
};

// A source's sides for the run between node rows i0 / i1, the rows permuted by `order` alone: what labelmap_ordered_kernel keeps.
template <int MCAP>
__device__ __forceinline__ void column_sides(const JointColumn &k, int i0, int i1, int M, uint64_t order, int S, float (&qtop)[MCAP],
                                             float (&qbot)[MCAP]) {
  float q00[MCAP], q01[MCAP], q10[MCAP], q11[MCAP];
  load_ordered(k.f0 + (size_t)i0 * M, order, S, q00), load_ordered(k.f1 + (size_t)i0 * M, order, S, q01);
  load_ordered(k.f0 + (size_t)i1 * M, order, S, q10), load_ordered(k.f1 + (size_t)i1 * M, order, S, q11);
  ordered_sides(q00, q01, q10, q11, k.wc, S, qtop, qbot);
}

// What a lane keeps of a run of rows: source a's sides (KIND -1: those alone), or both sources' as labelmap_ordered_joint_kernel.
template <int KIND, int MCAP>
struct PosteriorSides {
  float qta[MCAP], qba[MCAP], ta[MCAP], ba[MCAP], qtb[MCAP], qbb[MCAP], tb[MCAP], bb[MCAP];

  __device__ __forceinline__ void load(const JointColumn &ka, const JointColumn &kb, int i0, int i1, int M, uint64_t order, int S) {
    if (KIND >= 0) {
      joint_sides(ka, i0, i1, M, order, S, ta, ba, qta, qba);
      joint_sides(kb, i0, i1, M, order, S, tb, bb, qtb, qbb);
    } else {
      column_sides(ka, i0, i1, M, order, S, qta, qba);
    }
  }

  // f[r][s] of the row with weight wr: the decode's e[r][s] (the joint kernel's selection with a KIND), floored; 0 beyond S.
  __device__ __forceinline__ void evidence(float wr, int M, int S, float ln_m, float floor, float (&f)[MCAP]) const {
    float top[MCAP], bot[MCAP], e[MCAP];
    bool took = false;
    if (KIND >= 0) {
      const float ca = joint_confidence<(KIND >= 0 ? KIND : 0)>(ta, ba, wr, M, ln_m);
      const float cb = joint_confidence<(KIND >= 0 ? KIND : 0)>(tb, bb, wr, M, ln_m);
      took = cb > ca;  // crw_merge_confidence's comparison: a tie and a NaN keep source a
    }
#pragma unroll
    for (int s = 0; s < MCAP; ++s) top[s] = took ? qtb[s] : qta[s], bot[s] = took ? qbb[s] : qba[s];
    ordered_values(top, bot, wr, S, e);
#pragma unroll
    for (int s = 0; s < MCAP; ++s) f[s] = s < S ? fmaxf(e[s], floor) : 0.f;
  }
};

// One row of the forward scan: A[r-1] -> A[r] under f[r].  Row 0 enters with A = (1, 0, ...): every prefix sum is 1.
template <int MCAP>
__device__ __forceinline__ void posterior_forward_step(float (&A)[MCAP], const float (&f)[MCAP]) {
#pragma clang fp contract(off)
  float run = 0.f, sum = 0.f;
#pragma unroll
  for (int s = 0; s < MCAP; ++s) {
    run += A[s];
    A[s] = f[s] * run;
    sum += A[s];
  }
  const float inv = 1.f / sum;  // sum >= f[S-1] * (the prefix over every state) > 0
#pragma unroll
  for (int s = 0; s < MCAP; ++s) A[s] *= inv;
}

// One row of the backward scan, row r: from b[r] (`b`), A[r] and f[r] -> gamma[r], the terms of the moments that belong to "the
// boundary enters at row r + 1", and b[r-1] (left in `b`).  pick[k] = b^_k.  Z_r < 2^-126 (the column's evidence contradicts the
// order over so many rows that A and b share no state fp32 can hold) gives gamma = 0 and no terms, not a NaN.
template <int MCAP>
__device__ __forceinline__ void posterior_backward_step(float (&b)[MCAP], const float (&A)[MCAP], const float (&f)[MCAP], int r,
                                                        const int (&pick)[MCAP], float (&gamma)[MCAP], float (&m1)[MCAP],
                                                        float (&m2)[MCAP]) {
#pragma clang fp contract(off)
  float Z = 0.f;
#pragma unroll
  for (int s = 0; s < MCAP; ++s) {
    gamma[s] = A[s] * b[s];
    Z += gamma[s];
  }
  const float inv = Z >= 0x1p-126f ? 1.f / Z : 0.f;  // (the reciprocal of a subnormal can be infinite)
#pragma unroll
  for (int s = 0; s < MCAP; ++s) gamma[s] *= inv;
  const float at = (float)(r + 1);
  float below = 0.f;  // sum_{s < k} A[r][s]
#pragma unroll
  for (int k = 1; k < MCAP; ++k) {
    below += A[k - 1];
    const float p = below * b[k] * inv;  // (b[k] = 0 beyond S)
    const float off = at - (float)pick[k];
    m1[k] += at * p;
    m2[k] += off * off * p;
  }
  const float binv = 1.f / b[0];  // b[0] >= f * B of the row below's largest entry > 0
  float run = 0.f;
#pragma unroll
  for (int s = MCAP - 1; s >= 0; --s) {
    run += f[s] * (b[s] * binv);
    b[s] = run;
  }
}

// The position of a label in `order`, -1 outside it (a label that is no integer included).
template <typename LAB>
__device__ __forceinline__ int label_position(LAB v, uint64_t order, int S) {
  const int code = std::is_same<LAB, float>::value ? code_f32((float)v) : (int)v;
  int pos = -1;
  for (int s = 0; s < S; ++s)
    if (order_at(order, s) == code) pos = s;
  return pos;
}

// KIND: -1 for crw_labelmap_ordered_posterior, a CRW_CONF_* kind for the joint call; MCAP: 4, 8 or 16 >= M >= S
template <typename LAB, int KIND, int MCAP>
__global__ __launch_bounds__(WAVE) void labelmap_posterior_kernel(PosteriorArgs a) {
  const OrderedArgs &o = a.j.o;
  const DenseArgs &d = o.d;
  const int M = d.M, N = d.N, S = o.S, rows = d.rows;
  __builtin_assume(M <= MCAP && S <= M && S >= 2);
  const int lane = threadIdx.x, g = blockIdx.y;  // the configuration is a grid dimension, as in labelmap_ordered_kernel
  const long x = (long)blockIdx.x * WAVE + lane;
  // A lane behind the window's last column runs both scans on that last column: it keeps its own workspace slots (the workspace
  // is 64 columns wide per wave) and stores post where that column's lane stores it, the same bits.  So EXEC is full from the first
  // row step to the last, and the row knots one lane computes and the others read (readlane) sit in registers that no copy under
  // a partial EXEC mask ever touches.  With `if (!live) continue` around the scans the compiler is free to move a lane's knots
  // through another register while the lanes behind the window are masked off, and what readlane then takes from those lanes is
  // garbage (seen at MCAP = 16 with a confidence kind, the one instantiation that parks the knots in AGPRs: wild node-row addresses
  // in a 1-column window).
  const bool live = x < d.cols;
  const long xc = live ? x : d.cols - 1;
  const size_t a_ld = a.a_ld, a_row = (size_t)S * a_ld;
  const LAB *__restrict__ lab = static_cast<const LAB *>(d.lab) + (size_t)g * d.map_stride + xc;
  float *__restrict__ post = a.post ? a.post + (size_t)g * d.map_stride + xc : nullptr;
  float *__restrict__ ws = a.alpha + (size_t)g * rows * a_row + x;  // x < a_ld
  const JointColumn ka = joint_column(a.j.a, g, xc, true, N, M);
  const JointColumn kb = KIND >= 0 ? joint_column(a.j.b, g, xc, true, N, M) : ka;
  PosteriorSides<KIND, MCAP> sides;
  float f[MCAP];

  // the picks: b^_k = the first row whose label's position is >= k (walked bottom to top: the last assignment is the first row)
  int pick[MCAP];
#pragma unroll
  for (int k = 0; k < MCAP; ++k) pick[k] = rows;
  if (a.hz)
    for (int r = rows - 1; r >= 0; --r) {
      const int pos = label_position(lab[(size_t)r * d.ld], o.order, S);
#pragma unroll
      for (int k = 1; k < MCAP; ++k) pick[k] = pos >= k ? r : pick[k];
    }

  // forward
  float A[MCAP];
#pragma unroll
  for (int s = 0; s < MCAP; ++s) A[s] = s == 0 ? 1.f : 0.f;
  for (int r0 = 0; r0 < rows; r0 += OD_CHUNK) {
    int ki = 0;  // row r0 + lane's knot and weight, as in labelmap_ordered_kernel
    float kw = 0.f;
    if (r0 + lane < rows) knot(r0 + lane, N, rows, &ki, &kw);
    const int rn = rows - r0 < OD_CHUNK ? rows - r0 : OD_CHUNK;
    for (int rr = 0; rr < rn;) {  // a run of rows between the same two node rows
      const int i0 = lane_int(ki, rr), i1 = i0 + 1 < N ? i0 + 1 : N - 1;
      sides.load(ka, kb, i0, i1, M, o.order, S);
      do {  // no load in here, for labelmap_ordered_kernel's reason
        sides.evidence(lane_float(kw, rr), M, S, d.ln_m, a.floor, f);
        posterior_forward_step(A, f);
        float *row = ws + (size_t)(r0 + rr) * a_row;
#pragma unroll
        for (int s = 0; s < MCAP; ++s)
          if (s < S) row[(size_t)s * a_ld] = A[s];
        ++rr;
      } while (rr < rn && lane_int(ki, rr) == i0);
    }
  }

  // backward: the same runs bottom to top.  `An`, `ln`: row r - 1's A and label, loaded while row r is worked on
  float b[MCAP], gamma[MCAP], m1[MCAP], m2[MCAP], An[MCAP];
  LAB ln = LAB(0);
#pragma unroll
  for (int s = 0; s < MCAP; ++s) b[s] = s < S ? 1.f : 0.f, gamma[s] = m1[s] = m2[s] = An[s] = 0.f;
  {
    const float *row = ws + (size_t)(rows - 1) * a_row;
#pragma unroll
    for (int s = 0; s < MCAP; ++s)
      if (s < S) An[s] = row[(size_t)s * a_ld];
    if (post) ln = lab[(size_t)(rows - 1) * d.ld];
  }
  for (int r0 = (rows - 1) / OD_CHUNK * OD_CHUNK; r0 >= 0; r0 -= OD_CHUNK) {
    int ki = 0;
    float kw = 0.f;
    if (r0 + lane < rows) knot(r0 + lane, N, rows, &ki, &kw);
    const int rn = rows - r0 < OD_CHUNK ? rows - r0 : OD_CHUNK;
    for (int rr = rn - 1; rr >= 0;) {
      const int i0 = lane_int(ki, rr), i1 = i0 + 1 < N ? i0 + 1 : N - 1;
      sides.load(ka, kb, i0, i1, M, o.order, S);
      do {
        const int r = r0 + rr;
        float Ar[MCAP];
#pragma unroll
        for (int s = 0; s < MCAP; ++s) Ar[s] = An[s];
        const LAB lr = ln;
        if (r > 0) {  // the row above: issued before this row's store
          const float *row = ws + (size_t)(r - 1) * a_row;
#pragma unroll
          for (int s = 0; s < MCAP; ++s)
            if (s < S) An[s] = row[(size_t)s * a_ld];
          if (post) ln = lab[(size_t)(r - 1) * d.ld];
        }
        sides.evidence(lane_float(kw, rr), M, S, d.ln_m, a.floor, f);
        posterior_backward_step(b, Ar, f, r, pick, gamma, m1, m2);
        if (post) {
          const int pos = label_position(lr, o.order, S);
          float p = 0.f;
#pragma unroll
          for (int s = 0; s < MCAP; ++s) p = s == pos ? gamma[s] : p;
          post[(size_t)r * d.ld] = fminf(p, 1.f);  // (the lanes behind the window: the last column's value again, to its address)
        }
        --rr;
      } while (rr >= 0 && lane_int(ki, rr) == i0);
    }
  }

  if (live && a.hz) {  // gamma is row 0's: P(B_k = 0) = sum_{s >= k} gamma[0][s], which closes the second moment
#pragma clang fp contract(off)
    float *hz = a.hz + (size_t)g * a.hz_stride + x;
    const size_t plane = (size_t)(S - 1) * a.hz_ld;
    float above = 0.f;
#pragma unroll
    for (int k = MCAP - 1; k >= 1; --k) {
      above += gamma[k];
      if (k < S) {
        const float at = (float)pick[k];
        hz[(size_t)(k - 1) * a.hz_ld] = at;
        hz[plane + (size_t)(k - 1) * a.hz_ld] = m1[k];
        hz[2 * plane + (size_t)(k - 1) * a.hz_ld] = sqrtf(m2[k] + at * at * above);
      }
    }
  }
}

size_t posterior_ws_bytes(int rows, int cols, int S) {
  if (rows < 1 || cols < 1 || S < 2 || S > 16) return 0;
  return (size_t)rows * S * ordered_ws_ld(cols) * sizeof(float);
}

// G slices of `each` elements of `size` bytes: false when their extent in bytes does not fit a size_t.
bool slices_fit(int G, size_t each, size_t size) { return each <= SIZE_MAX / size / (size_t)G; }

// What the one-map calls pass for the strides between configurations: one map's rows, one [3][S-1] block of hz rows.
size_t one_map(int rows, size_t ld) { return (size_t)(rows > 0 ? rows : 1) * ld; }
size_t one_hz(int S, size_t hz_ld) { return 3 * (size_t)(S > 1 ? S - 1 : 1) * hz_ld; }

size_t posterior_ws_bytes_batch(int G, int rows, int cols, int S) {
  const size_t one = posterior_ws_bytes(rows, cols, S);
  if (G < 1 || !one || !slices_fit(G, one, 1)) return 0;
  return (size_t)G * one;
}

// The four entry points behind their signatures (Lb null: the single calls, conf_kind -1; G = 1 with one map's extent as
// map_stride: the one-map calls).  The checks are the decode's -- dense_args' on the G windows, each source's, the order's -- then
// the posterior's own; nothing is launched unless all pass.
int posterior_launch(const float *La, int Ta, int cols_a, int col0_a, int flip_a, const float *Lb, int Tb, int cols_b, int col0_b,
                     int flip_b, int G, int N, int M, int rows, int ncols, const int *order, int S, int conf_kind, float floor,
                     const void *labels, int label_dtype, size_t ld, size_t map_stride, float *post, float *hz, size_t hz_ld,
                     size_t hz_stride, void *ws, size_t ws_bytes, crw_stream_t stream) {
  clear_stale_error();
  PosteriorArgs a;
  const bool joint = conf_kind >= 0;
  if (conf_kind < -1 || conf_kind > CRW_CONF_ENTROPY) return CRW_EINVAL;
  if (const int st = dense_args(La, G, Ta, N, M, rows, ncols, flip_a, -1, const_cast<void *>(labels), label_dtype, nullptr, ld,
                                map_stride, 1, a.j.o.d))
    return st;
  if (const int st = joint_source(La, Ta, cols_a, col0_a, flip_a, N, M, ncols, a.j.a)) return st;
  a.j.b = a.j.a;
  if (joint)
    if (const int st = joint_source(Lb, Tb, cols_b, col0_b, flip_b, N, M, ncols, a.j.b)) return st;
  if (const int st = ordered_order(order, S, a.j.o)) return st;
  if (!(floor >= 0x1p-20f && floor <= 0.25f)) return CRW_EINVAL;  // (a NaN fails both)
  if ((!post && !hz) || ((uintptr_t)post & 3) || ((uintptr_t)hz & 3) || (hz && hz_ld < (size_t)ncols) || !ws || ((uintptr_t)ws & 3))
    return CRW_EINVAL;
  // the G slices: hz's hold their [3][S-1] rows, and no slice's address wraps round
  if (hz && (!slices_fit(3 * (S - 1), hz_ld, sizeof(float)) || hz_stride < 3 * (size_t)(S - 1) * hz_ld)) return CRW_EINVAL;
  if (!slices_fit(G, map_stride, sizeof(float)) || !slices_fit(G, hz ? hz_stride : 1, sizeof(float)) ||
      !slices_fit(G, a.j.a.l_stride, sizeof(float)) || !slices_fit(G, a.j.b.l_stride, sizeof(float)))
    return CRW_EINVAL;
  const size_t need = posterior_ws_bytes_batch(G, rows, ncols, S);
  if (!need) return CRW_EINVAL;
  if (ws_bytes < need) return CRW_EWORKSPACE;
  a.j.o.ws = nullptr, a.j.o.ws_ld = 0, a.j.o.back = 0;
  a.floor = floor, a.post = post, a.hz = hz, a.hz_ld = hz_ld, a.hz_stride = hz_stride;
  a.alpha = static_cast<float *>(ws), a.a_ld = ordered_ws_ld(ncols);
  const dim3 grid((unsigned)(a.a_ld / WAVE), (unsigned)G);
  const auto kernel = kernel_for(label_dtype, conf_kind, M, [](auto lab, auto kind, auto mcap) {
    return labelmap_posterior_kernel<decltype(lab), kind(), mcap()>;
  });
  hipLaunchKernelGGL(kernel, grid, dim3(WAVE), 0, (hipStream_t)stream, a);
  return check_launch();
}

}  // namespace
}  // namespace crw

extern "C" size_t crw_labelmap_posterior_workspace(int rows, int cols, int S) { return crw::posterior_ws_bytes(rows, cols, S); }

extern "C" int crw_labelmap_ordered_posterior(const float *L, int T, int N, int M, int rows, int cols, int flip, const int *order,
                                              int S, float floor, const void *labels, int label_dtype, size_t ld, float *post,
                                              float *hz, size_t hz_ld, void *ws, size_t ws_bytes, crw_stream_t stream) {
  return crw::posterior_launch(L, T, cols, 0, flip, nullptr, 0, 0, 0, 0, 1, N, M, rows, cols, order, S, -1, floor, labels, label_dtype, ld,
                               crw::one_map(rows, ld), post, hz, hz_ld, crw::one_hz(S, hz_ld), ws, ws_bytes, stream);
}

extern "C" size_t crw_labelmap_posterior_workspace_batch(int G, int rows, int cols, int S) {
  return crw::posterior_ws_bytes_batch(G, rows, cols, S);
}

extern "C" int crw_labelmap_ordered_posterior_batch(const float *L, int G, int T, int N, int M, int rows, int cols, int flip,
                                                    const int *order, int S, float floor, const void *labels, int label_dtype,
                                                    size_t ld, size_t map_stride, float *post, float *hz, size_t hz_ld,
                                                    size_t hz_stride, void *ws, size_t ws_bytes, crw_stream_t stream) {
  return crw::posterior_launch(L, T, cols, 0, flip, nullptr, 0, 0, 0, 0, G, N, M, rows, cols, order, S, -1, floor, labels, label_dtype, ld,
                               map_stride, post, hz, hz_ld, hz_stride, ws, ws_bytes, stream);
}

extern "C" int crw_labelmap_ordered_joint_posterior(const float *La, int Ta, int cols_a, int col0_a, int flip_a, const float *Lb,
                                                    int Tb, int cols_b, int col0_b, int flip_b, int N, int M, int rows, int ncols,
                                                    const int *order, int S, int conf_kind, float floor, const void *labels,
                                                    int label_dtype, size_t ld, float *post, float *hz, size_t hz_ld, void *ws,
                                                    size_t ws_bytes, crw_stream_t stream) {
  if (conf_kind < 0) return CRW_EINVAL;  // mandatory, as for crw_labelmap_ordered_joint
  return crw::posterior_launch(La, Ta, cols_a, col0_a, flip_a, Lb, Tb, cols_b, col0_b, flip_b, 1, N, M, rows, ncols, order, S, conf_kind,
                               floor, labels, label_dtype, ld, crw::one_map(rows, ld), post, hz, hz_ld, crw::one_hz(S, hz_ld), ws,
                               ws_bytes, stream);
}

extern "C" int crw_labelmap_ordered_joint_posterior_batch(const float *La, int Ta, int cols_a, int col0_a, int flip_a, const float *Lb,
                                                          int Tb, int cols_b, int col0_b, int flip_b, int G, int N, int M, int rows,
                                                          int ncols, const int *order, int S, int conf_kind, float floor,
                                                          const void *labels, int label_dtype, size_t ld, size_t map_stride,
                                                          float *post, float *hz, size_t hz_ld, size_t hz_stride, void *ws,
                                                          size_t ws_bytes, crw_stream_t stream) {
  if (conf_kind < 0) return CRW_EINVAL;  // mandatory, as for crw_labelmap_ordered_joint_batch
  return crw::posterior_launch(La, Ta, cols_a, col0_a, flip_a, Lb, Tb, cols_b, col0_b, flip_b, G, N, M, rows, ncols, order, S, conf_kind,
                               floor, labels, label_dtype, ld, map_stride, post, hz, hz_ld, hz_stride, ws, ws_bytes, stream);
}
