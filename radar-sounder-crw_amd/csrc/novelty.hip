// Context novelty (include/crw_hip_novelty.h): how well a node's best key in its label-propagation context matches it.
//   nov[n][q] = 1 - max over the key frames f of frame n and the in-band nodes p (|p - q| < radius) of <ehat[n][q], ehat[f][p]>
//   score[n]  = mean of the `top` largest nov[n][.]
// The top-k kernels of labelprop.hip compute these products and keep softmax weights of the k best; the raw maximum is gone when
// they return.  This is labelprop_topk_mfma_kernel with its second half removed: the score phase is the same (16 queries x 16 keys
// per wave on v_mfma_f32_16x16x4_f32, exact fp32 products, two accumulation chains, the next key tile requested before this
// tile's MFMAs), but a score is never stored -- it goes into a band-masked running maximum held in the four accumulator rows a
// lane receives.  No candidate buffer, no chunks, no selection rounds, no index arithmetic.
// A workgroup owns a FRAME (its nov row stays in LDS for the frame score), so one launch writes both outputs and no global atomic
// is needed: the same call gives the same bits.  The host selector logs no route name: the `route` argument says which kernel ran.
#include "crw_common.h"
#include "crw_hip_novelty.h"

namespace crw {
namespace {

constexpr int NV_MAX_N = 4096;               // a frame's nov row and its `top` largest, sorted: 2 N floats of LDS
constexpr int NV_NT = 512, NV_NW = NV_NT / 64;  // matrix route: eight waves, two per SIMD cover each other's round trips
constexpr int NV_VT = 256;                   // vector route

// origin[] as the kernels of crw_hip_restart.h read it: 0 <= a < n whatever it holds
__device__ inline int nv_origin(const int32_t *origin, int n) { return min(max(origin[n], 0), n - 1); }

// score of the frame whose nov row (N floats) lies in LDS `row`: every value finds its rank by counting (ties: the lower node
// first, so the ranks are a permutation), the `top` first land in `srt` in descending order, one lane adds them in that order.
// The caller has synchronised after the last write to `row`.
__device__ inline void frame_score(const float *row, float *srt, int N, int top, float *out, int tid, int nt) {
  for (int i = tid; i < N; i += nt) {
    const float v = row[i];
    int rank = 0;
    for (int j = 0; j < N; ++j) {
      const float u = row[j];
      rank += (u > v || (u == v && j < i)) ? 1 : 0;
    }
    if (rank < top) srt[rank] = v;
  }
  __syncthreads();
  if (tid == 0) {
    float s = 0.f;
    for (int j = 0; j < top; ++j) s += srt[j];
    *out = s / (float)top;
  }
}

// ---- vector route: any C.  A wave per query node, a lane per key.
template <bool ORG>
__global__ __launch_bounds__(NV_VT) void novelty_vector_kernel(const float *__restrict__ ehat, int N, int C, int cxt, int radius,
                                                               int first_frame, int top, const int32_t *__restrict__ origin,
                                                               float *__restrict__ nov, float *__restrict__ score) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *row = smem, *srt = smem + N;
  const int na = blockIdx.x + first_frame, org = ORG ? nv_origin(origin, na) : 0, n = na - org;
  if (ORG) ehat += (long)org * N * C;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool trunc = n > cxt + 1;
  const int nf = trunc ? cxt + 1 : n;  // key frames: frame 0 (of the item that starts at the origin), then the last cxt

  for (int q = wave; q < N; q += NV_VT / 64) {
    const int lo = max(0, q - radius + 1), hi = min(N - 1, q + radius - 1), bw = hi - lo + 1;
    const float *qp = ehat + ((long)n * N + q) * C;
    float mx = -INFINITY;
    for (int cand = lane; cand < nf * bw; cand += 64) {
      const int p = cand / bw, m = lo + cand - p * bw;
      const int frame = trunc ? (p == 0 ? 0 : n - cxt + (p - 1)) : p;
      const float *kp = ehat + ((long)frame * N + m) * C;
      float d = 0.f;
      for (int c = 0; c < C; ++c) d += qp[c] * kp[c];
      mx = fmaxf(mx, d);
    }
    mx = wave_max(mx);  // the node itself is in its band in every key frame: finite
    if (lane == 0) {
      row[q] = 1.f - mx;
      nov[(long)(na - first_frame) * N + q] = 1.f - mx;
    }
  }
  __syncthreads();
  frame_score(row, srt, N, top, score + (na - first_frame), tid, NV_VT);
}

// ---- matrix route: C = 16 CSTEPS.  Per tile of 16 query nodes: item = (key frame p, 16-node key tile kt) over the union of the
// tile's bands, a wave per item.  Operand layout as in labelprop_topk_mfma_kernel: lane (r16, g) holds elements 16 j + 4 g .. + 3
// of row r16 of both operands, and receives the scores of queries 4 g + r (r = 0 .. 3) against key r16 of the tile.
template <int CSTEPS, bool ORG>
__global__ __launch_bounds__(NV_NT) void novelty_mfma_kernel(const float *__restrict__ ehat, int N, int cxt, int radius, int first_frame,
                                                             int top, const int32_t *__restrict__ origin, float *__restrict__ nov,
                                                             float *__restrict__ score) {
  constexpr int C = 16 * CSTEPS;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *row = smem, *srt = smem + N;
  __shared__ float wmax[2][NV_NW][16];  // per wave, the tile's 16 running maxima; two sets: ONE barrier per tile
  const int na = blockIdx.x + first_frame, org = ORG ? nv_origin(origin, na) : 0, n = na - org;
  if (ORG) ehat += (long)org * N * C;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, g = lane >> 4;
  const bool trunc = n > cxt + 1;
  const int nf = trunc ? cxt + 1 : n;

  const int ntiles = (N + 15) >> 4;
  for (int qt = 0; qt < ntiles; ++qt) {
    const int q0 = 16 * qt, nq = min(16, N - q0);
    const int ulo = max(0, q0 - radius + 1), uhi = min(N - 1, q0 + nq - 1 + radius - 1);
    const int kt_lo = ulo >> 4, nkt = (uhi >> 4) - kt_lo + 1;
    const int nitems = nf * nkt;
    // A operand: query row q0 + r16 (rows beyond the column repeat the last node: their maxima are never read)
    float4 a[CSTEPS];
    {
      const float *qp = ehat + ((long)n * N + min(q0 + r16, N - 1)) * C + 4 * g;
#pragma unroll
      for (int j = 0; j < CSTEPS; ++j) a[j] = *reinterpret_cast<const float4 *>(qp + 16 * j);
    }
    auto fetch = [&](int item, float4 (&b)[CSTEPS]) {
      const int p = item / nkt, kt = kt_lo + item - p * nkt;
      const int frame = trunc ? (p == 0 ? 0 : n - cxt + (p - 1)) : p;
      const float *kp = ehat + ((long)frame * N + min(16 * kt + r16, N - 1)) * C + 4 * g;  // rows beyond the column: masked below
#pragma unroll
      for (int j = 0; j < CSTEPS; ++j) b[j] = *reinterpret_cast<const float4 *>(kp + 16 * j);
    };
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    float4 b[CSTEPS], bn[CSTEPS];
    if (wave < nitems) fetch(wave, b);
    for (int item = wave; item < nitems; item += NV_NW) {  // (wave-uniform: every lane takes part in the MFMAs)
      if (item + NV_NW < nitems) fetch(item + NV_NW, bn);
      f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};  // even / odd steps: two independent chains
#pragma unroll
      for (int j = 0; j < CSTEPS; ++j) {
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].x, b[j].x, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].y, b[j].y, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].z, b[j].z, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].w, b[j].w, acc1, 0, 0, 0);
      }
      const int m = 16 * (kt_lo + item % nkt) + r16;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int d = m - (q0 + 4 * g + r);
        if (m < N && d > -radius && d < radius) mx[r] = fmaxf(mx[r], acc0[r] + acc1[r]);
      }
#pragma unroll
      for (int j = 0; j < CSTEPS; ++j) b[j] = bn[j];
    }
    // across the 16 key columns: the lanes of one group g
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) mx[r] = fmaxf(mx[r], __shfl_xor(mx[r], o));
      if (r16 == 0) wmax[qt & 1][wave][4 * g + r] = mx[r];  // -inf from a wave that had no item
    }
    __syncthreads();
    if (tid < nq) {
      float v = wmax[qt & 1][0][tid];
#pragma unroll
      for (int w = 1; w < NV_NW; ++w) v = fmaxf(v, wmax[qt & 1][w][tid]);
      row[q0 + tid] = 1.f - v;
      nov[(long)(na - first_frame) * N + q0 + tid] = 1.f - v;
    }
  }
  __syncthreads();
  frame_score(row, srt, N, top, score + (na - first_frame), tid, NV_NT);
}

template <int CSTEPS>
int launch_novelty_mfma(const float *ehat, int F, int N, int cxt, int radius, int first_frame, int top, const int32_t *origin, float *nov,
                        float *score, hipStream_t s) {
  const size_t lds = (size_t)2 * N * 4;
  if (origin)
    hipLaunchKernelGGL((novelty_mfma_kernel<CSTEPS, true>), dim3(F), dim3(NV_NT), lds, s, ehat, N, cxt, radius, first_frame, top, origin, nov,
                       score);
  else
    hipLaunchKernelGGL((novelty_mfma_kernel<CSTEPS, false>), dim3(F), dim3(NV_NT), lds, s, ehat, N, cxt, radius, first_frame, top, origin,
                       nov, score);
  return check_launch();
}

}  // namespace
}  // namespace crw

extern "C" int crw_labelprop_novelty(const float *ehat, int T, int N, int C, int cxt_size, int radius, int first_frame, int top,
                                     const int32_t *origin, float *nov, float *score, int route, crw_stream_t stream) {
  using namespace crw;
  clear_stale_error();
  if (!ehat || !nov || !score || T < 2 || N < 1 || N > NV_MAX_N || C < 1 || cxt_size < 1 || radius < 1 || first_frame < 1 ||
      first_frame >= T || top < 1 || top > N || route < 0 || route > 2)
    return CRW_EINVAL;
  const bool matrix_ok = (C == 16 || C == 32 || C == 64 || C == 128 || C == 256) && (((uintptr_t)ehat) & 15) == 0;
  if (route == 2 && !matrix_ok) return CRW_EINVAL;
  if (radius > N) radius = N;              // |p - q| < N always: the same band, and no overflow in q + radius
  if (cxt_size > T) cxt_size = T;          // likewise: a context longer than the item never truncates
  hipStream_t s = (hipStream_t)stream;
  const int F = T - first_frame;
  if (route != 1 && matrix_ok) {
    switch (C) {
      case 16: return launch_novelty_mfma<1>(ehat, F, N, cxt_size, radius, first_frame, top, origin, nov, score, s);
      case 32: return launch_novelty_mfma<2>(ehat, F, N, cxt_size, radius, first_frame, top, origin, nov, score, s);
      case 64: return launch_novelty_mfma<4>(ehat, F, N, cxt_size, radius, first_frame, top, origin, nov, score, s);
      case 128: return launch_novelty_mfma<8>(ehat, F, N, cxt_size, radius, first_frame, top, origin, nov, score, s);
      default: return launch_novelty_mfma<16>(ehat, F, N, cxt_size, radius, first_frame, top, origin, nov, score, s);
    }
  }
  const size_t lds = (size_t)2 * N * 4;
  if (origin)
    hipLaunchKernelGGL(novelty_vector_kernel<true>, dim3(F), dim3(NV_VT), lds, s, ehat, N, C, cxt_size, radius, first_frame, top, origin, nov,
                       score);
  else
    hipLaunchKernelGGL(novelty_vector_kernel<false>, dim3(F), dim3(NV_VT), lds, s, ehat, N, C, cxt_size, radius, first_frame, top, origin,
                       nov, score);
  return check_launch();
}
