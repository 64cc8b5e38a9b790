// Inference path: k-NN label propagation along the radargram (src/utils.py:134-161,
// src/imported/labelprop.py:67-115, src/imported/maskedatt.py:151-175) and the
// "horizontality" metric (src/utils.py:117-125).
//
// Restructured for the GPU: the reference recomputes, for every frame n, the affinity of frame n
// against the whole growing context and only then gathers labels.  Features never change, so
//   (1) crw_labelprop_topk computes the top-k weights/indices of ALL frames in one launch
//       (one workgroup per (query node, frame); only in-band keys |m-q| < radius are scored --
//       out-of-band keys carry logit -1e10/temp whose softmax weight is exactly 0 in fp32);
//   (2) crw_labelprop_gather is the only sequential part: a single workgroup walks the frames and
//       does the weighted label sums + argmax.
// Index quirk kept on purpose: indices address the truncated key list
// [frame 0, last cxt frames] but are applied to the untruncated label list.  The opt-in 'sliding' rule
// (crw_labelprop_propagate_sliding) applies them to the frames they were scored on instead; the lists are the same.
#include "crw_common.h"
#include "crw_hip_restart.h"
#include "crw_hip_longmem.h"
#include "crw_hip_align.h"
#include "crw_hip_sweepmem.h"
#include <cstdlib>
#include <type_traits>

namespace crw {
namespace {

constexpr int MAX_KNN = 64;

// Nodes of a frame form a gh x gw grid (node = i * gw + j; a radargram's patch column: gw = 1).  A key (i', j') is in band for the
// query (i, j) when (i - i')^2 + (j - j')^2 < radius^2 (MaskedAttention.make, src/imported/maskedatt.py:232-245); candidates are the
// keys of the clipped bounding box of that disc, in node order, and box keys outside the disc never score (the reference gives them
// logit -1e10 / temp: softmax weight exactly 0).
// ORG (crw_labelprop_topk_origin, include/crw_hip_restart.h): frame na is scored as frame n = na - a of the item that starts at its
// origin a = origin[na] -- the key base moves to frame a, the context arithmetic runs on n, the lists go to frame na's place.
__device__ inline int frame_origin(const int32_t *origin, int n) { return min(max(origin[n], 0), n - 1); }  // 0 <= a < n whatever it holds
// LM (the crw_labelprop_*_long entry points, include/crw_hip_longmem.h): the first K = n_long frames are long-term, where the
// other instances keep frame 0 alone -- list position p of a truncated list (n > K + cxt) is frame p while p < K, then the window
// n - cxt .. n - 1.  K = 1 is the other instances' arithmetic; they keep their own text, so their instruction streams stay.
// The number K travels in the place of the origin pointer, which an LM instance does not have: one 8-byte kernel argument either way,
// so the other instances keep their argument layout as well (the hidden arguments, blockDim among them, follow the last one).
// LB (crw_labelprop_topk_long_bias, include/crw_hip_align.h; LM instances only): `bias` is added to the cosine of the in-band keys at
// list positions p < K -- the long-term part; p < nf <= n, so that is p < min(n, K) -- by one rounded add in front of the division
// by temp.  It travels in the padding of the same 8-byte argument, which the other instances do not read.
struct LongFrames {
  int n;
  float bias;
};
template <bool LM>
using OriginArg = std::conditional_t<LM, LongFrames, const int32_t *__restrict__>;
template <bool LM>
__device__ __forceinline__ int long_frames(OriginArg<LM> a) {
  if constexpr (LM) return a.n;
  else return 1;
}
template <bool ORG, class Arg>
__device__ __forceinline__ int origin_at(Arg origin, int n) {
  if constexpr (ORG) return frame_origin(origin, n);
  else return 0;
}
template <bool ORG, bool LM, bool LB = false>
__global__ __launch_bounds__(256) void labelprop_topk_kernel(const float *__restrict__ ehat, int T, int N, int C,
                                                             int cxt, int radius, float temp, int knn,
                                                             int first_frame, int gw, float *__restrict__ W,
                                                             int32_t *__restrict__ I, int raw, OriginArg<LM> origin) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int q = blockIdx.x, na = blockIdx.y + first_frame, org = origin_at<ORG>(origin, na), n = na - org;
  if (ORG) ehat += (long)org * N * C;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = long_frames<LM>(origin);
  const bool trunc = n > cxt + K;
  const int nf = trunc ? cxt + K : n;
  const int gh = N / gw, qi = q / gw, qj = q - qi * gw;
  const int lo = max(0, qi - radius + 1), hi = min(gh - 1, qi + radius - 1);        // box rows
  const int lj = max(0, qj - radius + 1), hj = min(gw - 1, qj + radius - 1);        // box columns
  const int bwj = hj - lj + 1;
  const int bw = (hi - lo + 1) * bwj;                                               // keys of the box per context frame
  const int ncand = nf * bw;

  float *qv = smem;                       // [C] (padded to a multiple of 4)
  float *val = smem + ((C + 3) & ~3);     // [ncand]
  __shared__ float red_v[4];
  __shared__ int red_i[4];
  __shared__ float sel_v[MAX_KNN];
  __shared__ int sel_i[MAX_KNN];

  for (int c = tid; c < C; c += 256) qv[c] = ehat[((long)n * N + q) * C + c];
  __syncthreads();

  // 16 lanes per candidate
  const int sub = tid & 15, grp = tid >> 4;  // 16 groups per block
  for (int cand = grp; cand < ncand; cand += 16) {
    const int p = cand / bw, r = cand - p * bw;
    const int mi = lo + r / bwj, mj = lj + r % bwj, m = mi * gw + mj;
    const bool inside = (mi - qi) * (mi - qi) + (mj - qj) * (mj - qj) < radius * radius;  // (always, on an N x 1 grid)
    const int frame = LM ? ((!trunc || p < K) ? p : n - cxt + (p - K)) : (trunc ? (p == 0 ? 0 : n - cxt + (p - 1)) : p);
    const float *key = ehat + ((long)frame * N + m) * C;
    float d = 0.f;
    if ((C & 3) == 0) {
      for (int c = 4 * sub; c < C; c += 64) {
        const float4 kv = *reinterpret_cast<const float4 *>(key + c);
        const float4 qq = *reinterpret_cast<const float4 *>(qv + c);
        d += kv.x * qq.x + kv.y * qq.y + kv.z * qq.z + kv.w * qq.w;
      }
    } else {
      for (int c = sub; c < C; c += 16) d += key[c] * qv[c];
    }
    d += __shfl_xor(d, 8);
    d += __shfl_xor(d, 4);
    d += __shfl_xor(d, 2);
    d += __shfl_xor(d, 1);
    if constexpr (LB) {
      static_assert(LM, "the bias is the long-term keys'");
      if (sub == 0) val[cand] = inside ? (p < K ? __fadd_rn(d, origin.bias) : d) / temp : -INFINITY;
    } else {
      if (sub == 0) val[cand] = inside ? d / temp : -INFINITY;
    }
  }
  __syncthreads();

  // knn rounds of block-wide arg-max (ties -> lowest candidate index)
  for (int j = 0; j < knn; ++j) {
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int c = tid; c < ncand; c += 256) {
      const float v = val[c];
      if (v > bv || (v == bv && c < bi)) { bv = v; bi = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o);
      const int oi = __shfl_xor(bi, o);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { red_v[wave] = bv; red_i[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < 4; ++w)
        if (red_v[w] > bv || (red_v[w] == bv && red_i[w] < bi)) { bv = red_v[w]; bi = red_i[w]; }
      sel_v[j] = bv;
      sel_i[j] = bi;
      if (bi != 0x7fffffff && bv != -INFINITY) val[bi] = -INFINITY;
    }
    __syncthreads();
  }

  if (tid < knn) {
    const float vmax = sel_v[0];  // in-band key m == q always exists (radius >= 1)
    float ssum = 0.f;
    for (int j = 0; j < knn; ++j) ssum += (sel_v[j] == -INFINITY) ? 0.f : expf(sel_v[j] - vmax);
    const float v = sel_v[tid];
    float w = 0.f;
    int idx = 0;
    if (v != -INFINITY) {
      w = raw ? v : expf(v - vmax) / ssum;  // raw (crw_labelprop_topk_scores): the selected logit itself
      const int c = sel_i[tid], r = c % bw;
      idx = (c / bw) * N + (lo + r / bwj) * gw + lj + r % bwj;
    } else if (raw) {
      w = -INFINITY;
    }
    const long o = ((long)(na - first_frame) * knn + tid) * N + q;
    W[o] = w;
    I[o] = idx;
  }
}

// ---- the same lists on an N x 1 grid (a radargram's patch column), scores on the fp32 matrix cores ------------------------------
// The kernel above spends its time in vector arithmetic: 16 lanes per (query, key) pair, ~30 instructions for 128 multiply-adds.
// Here a workgroup owns 16 consecutive query nodes of a frame; S = Q K^T for 16 keys at a time is 32 v_mfma_f32_16x16x4_f32 (exact
// fp32 products, fp32 accumulation -- the summation order differs from the vector kernel's, as that one's differs from the
// reference's BLAS), a wave per (context frame, 16-node key tile), the next tile's rows requested before this one's MFMAs.  In-band
// scores go to LDS as val[query][candidate] in the reference's candidate order; selection: a wave per PAIR of queries with their candidates in
// registers (TK_NV per lane and query) -- no workgroup barrier inside the knn rounds --, same rule: highest value, then lowest candidate index.
constexpr int TK_Q = 16, TK_NV = 32, TK_NT = 512, TK_NW = TK_NT / 64;  // eight waves: two per SIMD cover each other's round trips
// NCH = 2: the context frames in two halves, one after the other through HALF the score buffer (two workgroups per CU: one's
// scoring -- matrix cores, loads, LDS scatter -- runs beside the other's selection -- vector compares), the first half's k best
// carried into the second selection as extra candidates: top-k(A u B) = top-k(top-k(A) u B), and the carried candidates have the
// lower indices, so "highest value, then lowest candidate index" picks the same list.  pf = context frames per chunk.
// NCH = 0: the same with a RUNTIME number of chunks, ceil(nf / pf), for candidate lists too long for two halves (radius 30 / 60 at
// 80 - 100 context frames: 3 888 / 11 781 candidates per query).  The argument holds chunk after chunk -- the k best carried into
// each selection come from earlier chunks, so they have the lowest indices -- and the chunk size is that of NCH = 2 (pf * max_bi
// <= 64 * TK_NV / 2 in registers, 64 KiB of scores at 1 024 candidates: two workgroups per CU).
template <int CSTEPS, int NCH, bool ORG, bool LM, bool LB = false>  // C / 16: float4 per lane and row; ORG, LM, LB: as in labelprop_topk_kernel
__global__ __launch_bounds__(TK_NT, NCH == 1 ? 2 : 4) void labelprop_topk_mfma_kernel(const float *__restrict__ ehat, int T, int N, int cxt, int radius,
                                                                           float temp, int knn, int first_frame, int maxcand, int pf,
                                                                           float *__restrict__ W, int32_t *__restrict__ I, int raw,
                                                                           OriginArg<LM> origin) {
  constexpr int C = 16 * CSTEPS, NV = TK_NV / (NCH == 1 ? 1 : 2);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *val = smem;  // [TK_Q][maxcand] (maxcand: candidates of ONE chunk)
  __shared__ float sel_v[TK_Q][MAX_KNN];
  __shared__ int sel_i[TK_Q][MAX_KNN];
  const int q0 = blockIdx.x * TK_Q, nq = min(TK_Q, N - q0), na = blockIdx.y + first_frame;
  const int org = origin_at<ORG>(origin, na), n = na - org;
  if (ORG) ehat += (long)org * N * C;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, g = lane >> 4;
  const int K = long_frames<LM>(origin);
  const bool trunc = n > cxt + K;
  const int nf = trunc ? cxt + K : n;

  const int ulo = max(0, q0 - radius + 1), uhi = min(N - 1, q0 + nq - 1 + radius - 1);
  const int kt_lo = ulo >> 4, nkt = (uhi >> 4) - kt_lo + 1;  // item = (context frame p, key tile kt)
  int lo_r[4], bw_r[4];  // bands of the four queries whose scores this lane receives (rows 4 g + r of the tile)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = q0 + 4 * g + r, lo = max(0, q - radius + 1), hi = min(N - 1, q + radius - 1);
    lo_r[r] = lo;
    bw_r[r] = q < N ? hi - lo + 1 : 0;
  }
  // selection: wave w takes the queries w and w + 8 TOGETHER -- two independent chains of compares / cross-lane exchanges in one
  // instruction stream
  const int u0 = wave, u1 = wave + TK_NW;
  int lo2[2], bw2[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int q = q0 + (h ? u1 : u0), lo = max(0, q - radius + 1), hi = min(N - 1, q + radius - 1);
    lo2[h] = lo;
    bw2[h] = hi - lo + 1;
  }

  const int nch = NCH ? NCH : (nf + pf - 1) / pf;
  for (int ch = 0; ch < nch; ++ch) {
    const int p0 = ch * pf, np = min(nf - p0, NCH == 1 ? nf : pf);  // this chunk's context frames [p0, p0 + np)
    if (np <= 0) break;                                            // (block-uniform)
    const int nitems = np * nkt;
    // A operand: query row q0 + r16 (rows beyond the column repeat the last node: their scores are never stored); lane group g holds
    // elements 16 j + 4 g .. + 3 of every 16 -- the k order of the MFMA steps, the same for both operands (per chunk: not live
    // through the selection)
    float4 a[CSTEPS];
    {
      const float *qp = ehat + ((long)n * N + min(q0 + r16, N - 1)) * C + 4 * g;
#pragma unroll
      for (int j = 0; j < CSTEPS; ++j) a[j] = *reinterpret_cast<const float4 *>(qp + 16 * j);
    }
    auto fetch = [&](int item, float4 (&b)[CSTEPS]) {
      const int p = p0 + item / nkt, kt = kt_lo + item % nkt;
      const int frame = LM ? ((!trunc || p < K) ? p : n - cxt + (p - K)) : (trunc ? (p == 0 ? 0 : n - cxt + (p - 1)) : p);
      const float *kp = ehat + ((long)frame * N + min(16 * kt + r16, N - 1)) * C + 4 * g;
#pragma unroll
      for (int j = 0; j < CSTEPS; ++j) b[j] = *reinterpret_cast<const float4 *>(kp + 16 * j);
    };
    // NCH = 1: the next item's key rows are requested before this one's MFMAs (two waves per SIMD); NCH = 2: four waves per SIMD
    // cover the round trip, and the second register set would not fit 128 registers
    float4 b[CSTEPS], bn[NCH == 1 ? CSTEPS : 1];
    if (NCH == 1 && wave < nitems) fetch(wave, b);
    for (int item = wave; item < nitems; item += TK_NW) {
      if constexpr (NCH == 1) {
        if (item + TK_NW < nitems) fetch(item + TK_NW, bn);
      } else {
        fetch(item, b);
      }
      f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};  // even / odd steps: two independent chains
#pragma unroll
      for (int j = 0; j < CSTEPS; ++j) {
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].x, b[j].x, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].y, b[j].y, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].z, b[j].z, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].w, b[j].w, acc1, 0, 0, 0);
      }
      const int pl = item / nkt, m = 16 * (kt_lo + item - pl * nkt) + r16;  // pl: frame slot inside the chunk
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rr = m - lo_r[r];
        if constexpr (LB) {
          static_assert(LM, "the bias is the long-term keys'");
          const float cs = acc0[r] + acc1[r];
          if (m < N && rr >= 0 && rr < bw_r[r])
            val[(4 * g + r) * maxcand + pl * bw_r[r] + rr] = (p0 + pl < K ? __fadd_rn(cs, origin.bias) : cs) / temp;
        } else {
          if (m < N && rr >= 0 && rr < bw_r[r]) val[(4 * g + r) * maxcand + pl * bw_r[r] + rr] = (acc0[r] + acc1[r]) / temp;
        }
      }
      if constexpr (NCH == 1) {
#pragma unroll
        for (int j = 0; j < CSTEPS; ++j) b[j] = bn[j];
      }
    }
    __syncthreads();

    {
      int nc2[2], base2[2];
      float v[2][NV], ve[2];
      int ie[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int u = h ? u1 : u0;
        nc2[h] = u < nq ? np * bw2[h] : 0;
        base2[h] = p0 * bw2[h];  // candidate index of the chunk's first candidate
#pragma unroll
        for (int i = 0; i < NV; ++i) {
          const int c = lane + 64 * i;
          v[h][i] = c < nc2[h] ? val[u * maxcand + c] : -INFINITY;
        }
        // the k best of the chunks before (lane j holds the j-th): lower candidate indices than anything in this chunk
        const bool carried = ch > 0 && u < nq && lane < knn;
        ve[h] = carried ? sel_v[u][lane] : -INFINITY;
        ie[h] = carried ? sel_i[u][lane] : 0x7fffffff;
        if (ve[h] == -INFINITY) ie[h] = 0x7fffffff;
      }
      for (int j = 0; j < knn; ++j) {
        float bv[2];
        int bi[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          float x = ve[h];
          int bs = -1;
#pragma unroll
          for (int i = 0; i < NV; ++i)
            if (v[h][i] > x) { x = v[h][i]; bs = i; }  // ties inside a lane: the carried one, then the lowest slot = the lowest index
          bv[h] = x;
          bi[h] = x == -INFINITY ? 0x7fffffff : (bs < 0 ? ie[h] : base2[h] + lane + 64 * bs);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const float ov = __shfl_xor(bv[h], o);
            const int oi = __shfl_xor(bi[h], o);
            if (ov > bv[h] || (ov == bv[h] && oi < bi[h])) { bv[h] = ov; bi[h] = oi; }
          }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if (lane == 0 && (h ? u1 : u0) < nq) {
            sel_v[h ? u1 : u0][j] = bv[h];
            sel_i[h ? u1 : u0][j] = bi[h];
          }
          if (bi[h] != 0x7fffffff) {
            if (ie[h] == bi[h]) {
              ve[h] = -INFINITY;
              ie[h] = 0x7fffffff;
            } else if (bi[h] >= base2[h] && ((bi[h] - base2[h]) & 63) == lane) {
              const int slot = (bi[h] - base2[h]) >> 6;
#pragma unroll
              for (int i = 0; i < NV; ++i)
                if (i == slot) v[h][i] = -INFINITY;
            }
          }
        }
      }
    }
    if (NCH != 1) __syncthreads();  // the next chunk's scores overwrite val; lane 0's sel stores are in LDS for the carried reads
  }
  {
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // lane 0's stores are in LDS before the wave reads them back
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int u = h ? u1 : u0;
      if (u < nq && lane < knn) {
        const float vmax = sel_v[u][0];  // the query's own node is always in its band (radius >= 1)
        float ssum = 0.f;
        for (int j = 0; j < knn; ++j) ssum += (sel_v[u][j] == -INFINITY) ? 0.f : expf(sel_v[u][j] - vmax);
        const float x = sel_v[u][lane];
        float w = 0.f;
        int idx = 0;
        if (x != -INFINITY) {
          w = raw ? x : expf(x - vmax) / ssum;  // raw (crw_labelprop_topk_scores): the selected logit itself
          const int c = sel_i[u][lane];
          idx = (c / bw2[h]) * N + lo2[h] + c % bw2[h];
        } else if (raw) {
          w = -INFINITY;
        }
        const long o = ((long)(na - first_frame) * knn + lane) * N + q0 + u;
        W[o] = w;
        I[o] = idx;
      }
    }
  }
}

// launch of a kernel whose dynamic LDS may pass the 64 KiB a kernel gets unasked: the limit is raised to 150 KiB once per kernel
// (`Kern` is a template argument, so every instantiation has its own flag)
template <auto Kern, class... Args>
int launch_big_lds(dim3 grid, dim3 block, size_t lds, hipStream_t s, Args... args) {
  static bool raised = false;
  if (!raised) {
    if (hipFuncSetAttribute((const void *)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024) != hipSuccess) {
      g_last_hip_error = (int)hipGetLastError();
      return CRW_EHIP;
    }
    raised = true;
  }
  hipLaunchKernelGGL(Kern, grid, block, lds, s, args...);
  return check_launch();
}

template <int CSTEPS, int NCH>
int launch_topk_mfma_n(const float *ehat, int T, int N, int cxt, int radius, float temp, int knn, int first_frame, int chunkcand, int pf,
                       float *W, int32_t *I, int raw, const int32_t *origin, int n_long, hipStream_t s, float long_bias = 0.f) {
  const dim3 grid((N + TK_Q - 1) / TK_Q, T - first_frame);
  const size_t lds = (size_t)TK_Q * chunkcand * 4;
  if constexpr (NCH == 1) CRW_ROUTE("labelprop.topk_mfma_chunks1");
  else if constexpr (NCH == 2) CRW_ROUTE("labelprop.topk_mfma_chunks2");
  else CRW_ROUTE("labelprop.topk_mfma_long");
  if (n_long && long_bias != 0.f)  // crw_labelprop_topk_long_bias: the LB instance (a zero bias runs the instance below)
    return launch_big_lds<labelprop_topk_mfma_kernel<CSTEPS, NCH, false, true, true>>(grid, dim3(TK_NT), lds, s, ehat, T, N, cxt, radius, temp,
                                                                                      knn, first_frame, chunkcand, pf, W, I, raw,
                                                                                      LongFrames{n_long, long_bias});
  if (n_long)  // crw_labelprop_topk_long: the LM instance, whatever n_long is (no origins there)
    return launch_big_lds<labelprop_topk_mfma_kernel<CSTEPS, NCH, false, true>>(grid, dim3(TK_NT), lds, s, ehat, T, N, cxt, radius, temp, knn,
                                                                                first_frame, chunkcand, pf, W, I, raw, LongFrames{n_long, 0.f});
  if (origin)
    return launch_big_lds<labelprop_topk_mfma_kernel<CSTEPS, NCH, true, false>>(grid, dim3(TK_NT), lds, s, ehat, T, N, cxt, radius, temp, knn,
                                                                                first_frame, chunkcand, pf, W, I, raw, origin);
  return launch_big_lds<labelprop_topk_mfma_kernel<CSTEPS, NCH, false, false>>(grid, dim3(TK_NT), lds, s, ehat, T, N, cxt, radius, temp, knn,
                                                                               first_frame, chunkcand, pf, W, I, raw, origin);
}

// max_nf context frames of max_bi in-band keys: in one piece, or -- when the scores of a 16-query tile fill more than half a CU's LDS --
// in two halves, so that two workgroups share a CU (CRW_LABELPROP_TOPK_CHUNKS=1: always one piece, A/B)
template <int CSTEPS>
int launch_topk_mfma(const float *ehat, int T, int N, int cxt, int radius, float temp, int knn, int first_frame, int max_nf, int max_bi, float *W,
                     int32_t *I, int raw, const int32_t *origin, int n_long, hipStream_t s, float long_bias = 0.f) {
  static const bool one = getenv("CRW_LABELPROP_TOPK_CHUNKS") && getenv("CRW_LABELPROP_TOPK_CHUNKS")[0] == '1';
  const long maxcand = (long)max_nf * max_bi;
  const int pf = (max_nf + 1) / 2;
  if (!one && CSTEPS <= 8 /* 256 channels: past 128 registers */ && (size_t)TK_Q * maxcand * 4 > 76 * 1024 && (long)pf * max_bi <= 64L * (TK_NV / 2))
    return launch_topk_mfma_n<CSTEPS, 2>(ehat, T, N, cxt, radius, temp, knn, first_frame, pf * max_bi, pf, W, I, raw, origin, n_long, s, long_bias);
  return launch_topk_mfma_n<CSTEPS, 1>(ehat, T, N, cxt, radius, temp, knn, first_frame, (int)maxcand, max_nf, W, I, raw, origin, n_long, s,
                                       long_bias);
}

// candidate lists past the two forms above (more than 64 * TK_NV candidates, or a tile's scores over 150 KiB): chunks of pf frames,
// pf * max_bi <= 1 024 (the registers of NCH = 2), as many as the lists need, the chunks made even (ceil(max_nf / nch) frames each).
// 256 channels are not offered: their operands alone fill the 128 registers of two workgroups per CU (the vector kernel takes them).
constexpr int TK_LONG_CAND = 64 * (TK_NV / 2);
template <int CSTEPS>
int launch_topk_mfma_long(const float *ehat, int T, int N, int cxt, int radius, float temp, int knn, int first_frame, int max_nf, int max_bi,
                          float *W, int32_t *I, int raw, const int32_t *origin, int n_long, hipStream_t s, float long_bias = 0.f) {
  static_assert(CSTEPS <= 8, "256 channels: past 128 registers");
  int pf = TK_LONG_CAND / max_bi;
  const int nch = (max_nf + pf - 1) / pf;
  pf = (max_nf + nch - 1) / nch;
  return launch_topk_mfma_n<CSTEPS, 0>(ehat, T, N, cxt, radius, temp, knn, first_frame, pf * max_bi, pf, W, I, raw, origin, n_long, s, long_bias);
}

__device__ inline float ld_l2(const float *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline void st_l2(float *p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// single workgroup; frame n reads soft labels written for earlier frames by other waves of this
// same workgroup: stores/loads are agent-scope (L2) and separated by vmcnt(0) + barrier.
// SLIDE (crw_labelprop_propagate_sliding): an index of frame n addresses the list it was scored on, [frame 0, frames n - cxt .. n - 1]
// -- slide_row() below; false: the indices are label rows as they stand (cxt unused).
__device__ inline int slide_row(int i, int n, int N, int cxt) { return (i >= N && n > cxt + 1) ? i + (n - cxt - 1) * N : i; }
// ORG (the crw_labelprop_propagate_origin entry points, include/crw_hip_restart.h): frame n is frame n - a of the item that starts at
// its origin a = origin[n] -- the same translation on n - a, then a frames further down L.  a = 0: slide_row's value.
// LM (crw_labelprop_propagate_long, include/crw_hip_longmem.h): K long-term frames in front of the window, and the index clamped into
// the list it addresses first, min(n, K + cxt) * N entries -- what the ring kernel does on every route, so that the routes agree on
// any list.  K = 1 and an index in range: slide_row's value.
template <bool ORG, bool LM = false>
__device__ inline int slide_row_at(int i, int n, int a, int N, int cxt, int K = 1) {
  if constexpr (LM) {
    i = min(max(i, 0), min(n, K + cxt) * N - 1);
    return (i >= K * N && n > cxt + K) ? i + (n - cxt - K) * N : i;
  }
  return ORG ? a * N + slide_row(i, n - a, N, cxt) : slide_row(i, n, N, cxt);
}
// An anchor mark (sliding entry points only, CRW_LABELPROP_ANCHOR_WEIGHT in the header): a slot-0 weight of exactly -inf says that
// the node is clamped to the class its RAW slot-0 index names, clamped into [0, M - 1].  No softmax weight has these bits, so every
// other list is read as before.  anchor_onehot: the value the clamped node's output (q, c) takes -- 1.0f or +0.0f, written as they are.
constexpr int ANCHOR_BITS = (int)0xFF800000u;
__device__ inline bool anchor_mark(float w0) { return __float_as_int(w0) == ANCHOR_BITS; }
__device__ inline float anchor_onehot(int i0, int M, int c) { return c == min(max(i0, 0), M - 1) ? 1.f : 0.f; }

// ---- the pieces every propagation kernel below shares: the tie rule and the frame-0 rule of "same operations in the same order per
// output, bit-identical L and pred" exist ONCE.  (The role kernels and the ring gathers stay separate texts: merged into one
// template / one function they measured 1 - 3 % slower, profiles/labelprop_refactor_timing.log.) ----
// pred[q, n] of the queries q0, q0 + step, ..: the arg-max of row q of frame n's [N, M] soft labels at `frame`.  The first maximum
// wins (strict >, the lowest class on ties: torch.argmax on distinct values).  ld reads one element: L2Load from L in the global
// kernel, PlainLoad (an LDS read) everywhere else.
struct PlainLoad {
  __device__ float operator()(const float *p) const { return *p; }
};
struct L2Load {
  __device__ float operator()(const float *p) const { return ld_l2(p); }
};
template <class Load>
__device__ __forceinline__ void argmax_rows(float *pred, int T, int N, int M, int n, int q0, int step, const float *frame, Load ld) {
  for (int q = q0; q < N; q += step) {
    const float *row = frame + q * M;
    float bv = ld(row);
    int bi = 0;
    for (int c = 1; c < M; ++c) {
      const float v = ld(row + c);
      if (v > bv) { bv = v; bi = c; }
    }
    pred[(long)q * T + n] = (float)bi;
  }
}

// frame 0: with a seed its one-hot rows go to L and the seed to pred[:, 0]; without one L holds the frame already (the caller's).
// COPY: either way a copy goes to l0 in LDS (a template argument, not a test of l0: the LDS store must follow L's load on every
// path, or hipcc carries that load as outstanding and puts s_waitcnt vmcnt(0) in front of the per-frame arg-max loops).  L2: agent-scope stores and loads (the kernels whose later frames read L back through L2), plain
// ones otherwise.
template <bool L2, bool COPY>
__device__ __forceinline__ void init_frame0(const float *seed, float *L, float *pred, float *l0, int T, int N, int M, int tid, int nt) {
  if (COPY || seed)
    for (int it = tid; it < N * M; it += nt) {
      float v;
      if (seed) {
        v = seed[it / M] == (float)(it % M) ? 1.f : 0.f;
        if (L2) st_l2(L + it, v);
        else L[it] = v;
      } else {
        v = L2 ? ld_l2(L + it) : L[it];
      }
      if (COPY) l0[it] = v;
    }
  if (seed)
    for (int q = tid; q < N; q += nt) pred[(long)q * T] = seed[q];
}

template <bool SLIDE, bool ORG, bool LM>
__global__ __launch_bounds__(1024) void labelprop_gather_kernel(const float *__restrict__ seed,
                                                                const float *__restrict__ W,
                                                                const int32_t *__restrict__ I, int T, int N, int M,
                                                                int knn, int first_frame, float *L,
                                                                float *__restrict__ pred, int cxt, OriginArg<LM> origin) {
  const int tid = threadIdx.x, nt = blockDim.x;
  init_frame0<true, false>(seed, L, pred, nullptr, T, N, M, tid, nt);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int n = first_frame; n < T; ++n) {
    const float *Wn = W + (long)(n - first_frame) * knn * N;
    const int32_t *In = I + (long)(n - first_frame) * knn * N;
    const int org = origin_at<ORG>(origin, n);
    for (int it = tid; it < N * M; it += nt) {
      const int q = it / M, c = it % M;
      float p = 0.f;
      const bool mk = SLIDE && anchor_mark(Wn[q]);  // an anchored node: its list is not a list -- every read goes to row 0
      for (int j = 0; j < knn; ++j) {
        const int r = SLIDE ? (mk ? 0 : slide_row_at<ORG, LM>(In[j * N + q], n, org, N, cxt, long_frames<LM>(origin))) : In[j * N + q];
        p += ld_l2(L + (long)r * M + c) * Wn[j * N + q];
      }
      if (mk) p = anchor_onehot(In[q], M, c);  // ... and the sum is dropped for the one-hot of its class
      st_l2(L + ((long)n * N + q) * M + c, p);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    argmax_rows(pred, T, N, M, n, tid, nt, L + (long)n * N * M, L2Load());
  }
}

// The same propagation with the soft labels of the most recent R frames (and of frame 0, the long-term frame every step
// reads) kept in LDS, the step's (weight, index) lists prefetched one frame ahead into a double-buffered LDS copy, and the
// arg-max read back from LDS: a frame costs LDS traffic and ONE barrier where the kernel above pays three L2 round trips
// (gather, store acknowledge, arg-max reload) -- 10 us per frame at [T, N] = [256, 48].  Labels older than R frames are read
// from L in global memory (written there by every frame as before; they are long since visible).  Same operations in the
// same order: bit-identical results.
constexpr int GATHER_NT = 256, GATHER_PF = 8;  // threads; prefetch registers per thread (knn * N <= 2048)
constexpr int GATHER_CH = 20;                  // neighbours whose LDS reads are in flight together (KNN = 20: one batch per output; 4: 0.64, 10: 0.61, 20: 0.58 ms per cfg5 pass)
// LM: likewise the long-term frames 1 .. K - 1 (frame 0 has its slot)
template <bool SLIDE, bool ORG, bool LM>  // ORG: a restart frame's long-term frame is an ordinary row of L -- in the ring while it is recent, from L afterwards
__global__ __launch_bounds__(GATHER_NT) void labelprop_gather_lds_kernel(const float *__restrict__ seed,
                                                                         const float *__restrict__ W,
                                                                         const int32_t *__restrict__ I, int T, int N, int M,
                                                                         int knn, int first_frame, float *L,
                                                                         float *__restrict__ pred, int R, int cxt,
                                                                         OriginArg<LM> origin) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, NM = N * M, KN = knn * N;
  float *l0 = sm, *ring = l0 + NM, *wbuf = ring + (long)R * NM;  // [NM], [R][NM], [2][KN]
  int *ibuf = reinterpret_cast<int *>(wbuf + 2 * KN);              // [2][KN]
  init_frame0<true, true>(seed, L, pred, l0, T, N, M, tid, GATHER_NT);
  for (int e = tid; e < KN; e += GATHER_NT) {
    wbuf[(first_frame & 1) * KN + e] = W[e];
    ibuf[(first_frame & 1) * KN + e] = I[e];
  }
  __syncthreads();
  const int RNM = R * NM;
  for (int n = first_frame; n < T; ++n) {
    const int cur = n & 1;
    const int org = origin_at<ORG>(origin, n);
    // next frame's lists: global -> registers now, -> LDS after this frame's arithmetic (unconditional, clamped loads)
    const long nxt = (long)(min(n + 1, T - 1) - first_frame) * KN;
    float pw[GATHER_PF];
    int pi[GATHER_PF];
#pragma unroll
    for (int u = 0; u < GATHER_PF; ++u) {
      const int e = min(tid + u * GATHER_NT, KN - 1);
      pw[u] = W[nxt + e];
      pi[u] = I[nxt + e];
    }
    // frames [lo_f, n - 1] live in the ring; a frame f sits at flat offset (f % R) * NM
    const int lo_f = max(first_frame, n - R + 1);
    const int lo_idx = lo_f * N;                       // first label-list row that is in the ring
    const int epoch_base = (n / R - 1) * RNM;          // flat offset of the older of the (at most) two ring epochs in view
    const float *wn = wbuf + cur * KN;
    const int *in = ibuf + cur * KN;
    float *slot = ring + (n % R) * NM;
    for (int it = tid; it < NM; it += GATHER_NT) {
      const int q = it / M, c = it % M;
      float p = 0.f;
      const bool mk = SLIDE && anchor_mark(wn[q]);  // an anchored node (slot 0 of the frame's lists in LDS): every read goes to row 0
      // GATHER_CH neighbours at a time: their (index, weight) reads and then their label reads are independent LDS round trips
      // (one neighbour after the other is two dependent round trips each: 3 of the 4 us a frame took); the sum stays in j order
      for (int j0 = 0; j0 < knn; j0 += GATHER_CH) {
        int idx[GATHER_CH];
        float w[GATHER_CH], v[GATHER_CH];
#pragma unroll
        for (int u = 0; u < GATHER_CH; ++u) {
          const int jj = min(j0 + u, knn - 1);
          idx[u] = SLIDE ? (mk ? 0 : slide_row_at<ORG, LM>(in[jj * N + q], n, org, N, cxt, long_frames<LM>(origin))) : in[jj * N + q];
          w[u] = wn[jj * N + q];
        }
#pragma unroll
        for (int u = 0; u < GATHER_CH; ++u) {
          // frame 0 sits in l0 = sm[0, NM), the ring behind it; a label older than the ring comes from global memory
          int off = idx[u] * M + c - epoch_base;
          if (off >= RNM) off -= RNM;
          const bool first = idx[u] < N, old = !first && idx[u] < lo_idx;
          const int a = first ? idx[u] * M + c : (old ? 0 : NM + off);
          v[u] = sm[a];
          if (old) v[u] = ld_l2(L + (long)idx[u] * M + c);
        }
#pragma unroll
        for (int u = 0; u < GATHER_CH; ++u)
          if (j0 + u < knn) p += v[u] * w[u];
      }
      if (mk) p = anchor_onehot(in[q], M, c);  // ... and the sum is dropped for the one-hot of its class
      st_l2(L + ((long)n * N + q) * M + c, p);
      slot[it] = p;
    }
#pragma unroll
    for (int u = 0; u < GATHER_PF; ++u) {
      const int e = tid + u * GATHER_NT;
      if (e < KN) {
        wbuf[(cur ^ 1) * KN + e] = pw[u];
        ibuf[(cur ^ 1) * KN + e] = pi[u];
      }
    }
    __syncthreads();
    argmax_rows(pred, T, N, M, n, tid, GATHER_NT, slot, PlainLoad());
  }
}

// ---- propagation when the lists' context bound is known (crw_labelprop_propagate) -------------------------------------------------
// Index quirk Q7 read the other way round: crw_labelprop_topk's indices address the TRUNCATED key list [frame 0, last cxt frames],
// i.e. they are < min(n, cxt + 1) * N, and the reference applies them to the UNTRUNCATED label list (src/imported/labelprop.py:
// 103-107 with src/imported/maskedatt.py:165-166) -- so frame n reads the soft labels of frames 0 .. min(n - 1, cxt) and nothing
// else.  Only the first cxt frames form a chain (frame n needs frame n - 1); every frame n > cxt depends on frames 0 .. cxt alone.
//   prefix kernel: ONE workgroup walks frames first_frame .. cxt with ALL their labels in LDS (direct addressing, no ring).  Roles by
//     wave: compute waves own one output (query, class) per lane and do nothing but the dependent chain -- label reads (addresses
//     and weights already in registers), the sum in neighbour order, the LDS + global store, then the NEXT frame's (index, weight)
//     reads from an LDS copy while the barrier gathers; loader waves, one frame each in rotation, keep the lists of the next frames
//     in flight from global memory and copy them into a double-buffered LDS slot two frames ahead; one more wave takes the
//     arg-max / pred store of the previous frame.  The per-frame barrier waits for LDS traffic only (lds_barrier): global loads and
//     stores stay in flight across frames, where labelprop_gather_lds_kernel's __syncthreads() drained them every frame (2.4 us per frame at cfg5).
//   tail kernel (labelprop_tail_batch_kernel): a workgroup per frame n > cxt, all at once, labels gathered from L in global memory (complete since the prefix).
// Same operations in the same order per output as the kernels above: bit-identical L and pred.
constexpr int PX_PF = 16, PX_NT = 512;  // list entries per loader lane and frame (a frame's lists: knn * N <= 64 * PX_PF); threads at most

template <int KP>
__global__ __launch_bounds__(PX_NT) void labelprop_prefix_kernel(const float *__restrict__ seed, const float *__restrict__ W,
                                                                   const int32_t *__restrict__ I, int T, int N, int M, int knn,
                                                                   int first_frame, int last_frame, float *L,
                                                                   float *__restrict__ pred, int ncw) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, lane = tid & 63, NM = N * M, KN = knn * N;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // wave-uniform roles: compute waves [0, ncw), D list loaders [ncw, nwaves - 1), ONE arg-max wave (the last).
  // Loader k owns the frames f with (f - first_frame) % D == k: in the phase of frame f it copies the lists of frame f + 2 from its
  // registers into LDS and requests those of frame f + 2 + D -- a wave has ONE request in flight and touches it D phases later, so
  // the s_waitcnt vmcnt(0) hipcc puts in front of the copy meets loads that are long back.  (Measured the other ways: the arg-max's
  // pred stores in a loader wave -- two event types on one counter, hipcc waits for everything: 1.36 us per frame; several register
  // sets in rotation in one wave -- hipcc's counted waits across the loop's back edge come out as vmcnt(0..14): the same.)
  const int nwaves = (int)blockDim.x >> 6, D = nwaves - 1 - ncw;
  const bool compute = wave < ncw, loader = !compute && wave < nwaves - 1, amax = wave == nwaves - 1;
  const int lk = wave - ncw, at = tid - (nwaves - 1) * 64;
  constexpr int KNP = 64 * PX_PF;                           // entries of a list slot in LDS
  float *lab = sm;                                          // [(last_frame + 1) * NM] soft labels, frame-major like L
  // [2][KNP] (index, weight bits) pairs of frames f, f + 1 (slot = frame & 1), 8-byte aligned: one ds_read_b64 per neighbour
  int2 *pl = reinterpret_cast<int2 *>(lab + (((long)(last_frame + 1) * NM + 1) & ~1L));

  // labels of the frames before first_frame: frame 0 from the seed when given, the rest from L (filled by the caller)
  init_frame0<false, true>(seed, L, pred, lab, T, N, M, tid, (int)blockDim.x);
  for (int it = NM + tid; it < first_frame * NM; it += (int)blockDim.x) lab[it] = L[it];

  float pw[PX_PF];
  int pi[PX_PF];
  auto svc_load = [&](int f) {  // (clamped, unconditional: a frame past the last one re-reads the last one's lists, never used)
    const long o = (long)(min(f, last_frame) - first_frame) * KN;
#pragma unroll
    for (int u = 0; u < PX_PF; ++u) {
      const int e = min(lane + u * 64, KN - 1);
      pw[u] = W[o + e];
      pi[u] = I[o + e];
    }
  };
  auto svc_store = [&](int f) {  // unconditional too: a slot holds 64 * PX_PF >= KN entries, the surplus repeats the last entry
#pragma unroll
    for (int u = 0; u < PX_PF; ++u) pl[(f & 1) * KNP + lane + u * 64] = int2{pi[u], __float_as_int(pw[u])};
  };
  if (loader) {  // lists of the first two frames -> LDS; then every loader requests its first frame
    if (lk == 0) {
      svc_load(first_frame);
      svc_store(first_frame);
    }
    if (lk == (D > 1 ? 1 : 0)) {
      svc_load(first_frame + 1);
      svc_store(first_frame + 1);
    }
    svc_load(first_frame + 2 + lk);
  }
  lds_barrier();

  // compute lane: output `tid` = (q, c); LDS offsets and weights of its neighbours for the coming frame in registers
  // (the surplus lanes of the last compute wave repeat output NM - 1: same reads, same sum, same stores -- no branch around the
  // chain: under `if (it < NM)` hipcc sinks the label reads into the branch and waits for them one by one, 24 LDS round trips)
  const int it = min(tid, NM - 1), q = it / M, c = it % M;
  int a[KP];
  float w[KP];
  auto fetch_lists = [&](int f, int (&ix)[KP], float (&ww)[KP]) {  // frame f's lists: LDS -> registers (no dependence on labels)
    const int2 *ln = pl + (f & 1) * KNP;
#pragma unroll
    for (int j = 0; j < KP; ++j) {
      const int2 e = ln[min(j, knn - 1) * N + q];
      ix[j] = e.x;
      ww[j] = __int_as_float(e.y);
    }
  };
  auto to_offsets = [&](int f, int (&ix)[KP], float (&ww)[KP]) {
#pragma unroll
    for (int j = 0; j < KP; ++j) {
      ix[j] = min(max(ix[j], 0), f * N - 1) * M + c;  // in range whatever the lists hold (topk: < min(f, cxt + 1) * N)
      if (j >= knn) ww[j] = 0.f;                      // padding slot: p + v * 0 = p
    }
  };
  if (compute) {
    fetch_lists(first_frame, a, w);
    to_offsets(first_frame, a, w);
  }
  lds_barrier();  // the read of slot first_frame & 1 above comes before loader 0's svc_store(first_frame + 2) into the same slot

  int turn = 0;  // (f - first_frame) % D
  for (int f = first_frame; f <= last_frame; ++f) {
    if (compute) {
      float v[KP];
#pragma unroll
      for (int j = 0; j < KP; ++j) v[j] = lab[a[j]];
      int na[KP];
      float nw[KP];
      fetch_lists(f + 1, na, nw);  // slot (f + 1) & 1: written before the previous barrier (past last_frame: unused)
      float p = 0.f;
#pragma unroll
      for (int j = 0; j < KP; ++j) p += v[j] * w[j];
      lab[(long)f * NM + it] = p;
      L[(long)f * NM + it] = p;
      to_offsets(f + 1, na, nw);
#pragma unroll
      for (int j = 0; j < KP; ++j) {
        a[j] = na[j];
        w[j] = nw[j];
      }
    } else if (loader) {
      if (turn == lk) {
        svc_store(f + 2);  // slot f & 1: last read (frame f's lists) before the previous barrier
        svc_load(f + 2 + D);
      }
    } else if (f > first_frame) {  // arg-max of the previous frame (first maximum wins, like torch.argmax on distinct values)
      argmax_rows(pred, T, N, M, f - 1, at, 64, lab + (long)(f - 1) * NM, PlainLoad());
    }
    turn = turn + 1 == D ? 0 : turn + 1;
    lds_barrier();
  }
  if (amax) {
    argmax_rows(pred, T, N, M, last_frame, at, 64, lab + (long)last_frame * NM, PlainLoad());
  }
}

// ---- propagation from the frames the lists were scored on (crw_labelprop_propagate_sliding) -------------------------------------
// The other reading of the lists: index i of frame n addresses [frame 0, frames n - cxt .. n - 1] once n > cxt + 1 (slide_row), so
// frame n needs frame n - 1 for every n -- ONE chain over all frames, no tail.  labelprop_prefix_kernel's roles and phases (compute
// waves with one output per lane, list loaders in rotation, one arg-max wave, lds_barrier() per frame), but the labels in LDS are
// frame 0 plus a RING of R = cxt + 1 frames: frame f >= 1 sits at NM + ((f - 1) % R) * NM.  Until the window slides that is the prefix
// kernel's direct address i * M + c; afterwards it is that plus ((n - cxt - 1) % R) * NM, wrapped once -- one add and one compare per
// neighbour, both kept per frame as running offsets (no division in the loop).  R = cxt + 1, not cxt: in phase n frame n is stored
// while other lanes still read frame n - cxt, so the slot it takes must be that of frame n - cxt - 1.
//
// ORG (crw_labelprop_propagate_origin, include/crw_hip_restart.h): frame n is frame n' = n - a of the item that starts at its origin
// a = origin[n].  The ring keeps its ABSOLUTE layout (frame f at slot (f - 1) % R), so the translation is the running `shift` again:
// ((a + max(0, n' - cxt - 1)) % R) * NM, which at a restart (a = n - 1) is the offset of the slot frame n itself takes, and from
// there advances as before once n' > cxt + 1; the clamp bound follows n'.  The long-term frame is no longer frame 0 and would leave
// the ring after R phases, so it has a slot of its own -- TWO of them: in phase a, frame a's rows become the long-term frame of
// phase a + 1 while other lanes still read the long-term frame of phase a.  The compute lanes of phase a store their output a second
// time, into the slot that is NOT being read, and the roles flip at the barrier (mb, the slot of the frame whose offsets are made
// next).  origin[] is copied to LDS once, clamped to [0, n - 1]; a sequence that breaks the chain rule (origin[n] neither origin[n - 1]
// nor n - 1) reads rows of the wrong frames but never outside the labels in LDS: n' here is counted, at most n.
//
// LM (crw_labelprop_propagate_long, include/crw_hip_longmem.h): K = n_long long-term frames.  lab is [K][NM] followed by the ring
// [R][NM]: frame f < K sits at slot f for good (frames first_frame .. K - 1 of the call are computed into their slots like any other),
// frame f >= K at K + (f - K) % R.  A list position below K * N is its own address; the window's positions take the running shift
// ((f - cxt - K) % R) * NM once f > K + cxt, wrapped once past the ring's end; the clamp bound is min(f, K + cxt) * N - 1.  Every
// expression below is written with K, LN = K * N and LNM = K * NM, which are the literals 1, N and NM in the other instances.
template <int KP, bool ORG, bool LM>
__global__ __launch_bounds__(PX_NT) void labelprop_slide_kernel(const float *__restrict__ seed, const float *__restrict__ W,
                                                                  const int32_t *__restrict__ I, int T, int N, int M, int knn,
                                                                  int first_frame, int cxt, int R, float *L, float *__restrict__ pred,
                                                                  int ncw, OriginArg<LM> origin) {
  static_assert(!(ORG && LM), "origins and a bank of long-term frames are not combined");
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, lane = tid & 63, NM = N * M, KN = knn * N, last_frame = T - 1;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // roles as in labelprop_prefix_kernel: compute waves [0, ncw), D list loaders, ONE arg-max wave (the last)
  const int nwaves = (int)blockDim.x >> 6, D = nwaves - 1 - ncw;
  const bool compute = wave < ncw, loader = !compute && wave < nwaves - 1, amax = wave == nwaves - 1;
  const int lk = wave - ncw, at = tid - (nwaves - 1) * 64;
  constexpr int KNP = 64 * PX_PF;
  // launch_chain sends knn to the smallest instance that holds it, so knn > KP - 8: slots j < KLO are real in every list here and
  // need neither the clamp to the last slot nor the padding test
  constexpr int KLO = KP - 8;
  const int RNM = R * NM;
  // K, K * N and K * NM as expressions the front end folds to the literals 1, N and NM of the other instances' text (a variable that
  // is 1, or long_frames(), reaches the optimiser as arithmetic: hipcc then groups first_frame - cxt - 1 in the prologue another way
  // and allocates the KP = 16 instance's registers differently -- tools/isa_diff.py --functions shows it)
  const int Kl = long_frames<LM>(origin);
#define K (LM ? Kl : 1)
#define LN (LM ? Kl * N : N)
#define LNM (LM ? Kl * NM : NM)
  float *lab = sm;                                                                   // [NM] frame 0 (LM: [K][NM]), [R][NM] the ring
  // ORG: [NM] the second long-term slot and origin[T] behind the ring, in whole frames (slide_origin_frames(), the launcher's count)
  const long nlab = ORG ? R + 2 + (T + NM - 1) / NM : R + K;
  int2 *pl = reinterpret_cast<int2 *>(lab + ((nlab * NM + 1) & ~1L));  // [2][KNP] (index, weight bits), slot = frame & 1
  int *orgs = reinterpret_cast<int *>(lab + (long)(R + 2) * NM);      // (ORG only)

  // frame 0 (from the seed when given) and the frames before first_frame that a frame of this call can read: the last cxt of them
  init_frame0<false, true>(seed, L, pred, lab, T, N, M, tid, (int)blockDim.x);
  int org0 = 0;  // ORG: the first frame's origin -- its rows are the first long-term frame (same lanes, after frame 0's copy)
  if constexpr (ORG) {
    for (int t = tid; t < T; t += (int)blockDim.x) orgs[t] = t ? frame_origin(origin, t) : 0;
    org0 = __builtin_amdgcn_readfirstlane(frame_origin(origin, first_frame));
    if (org0 > 0)
      for (int it = tid; it < NM; it += (int)blockDim.x) lab[it] = L[(long)org0 * NM + it];
  }
  if constexpr (LM)  // the long-term frames 1 .. K - 1 that the caller filled (frame 0: above)
    for (int it = NM + tid; it < min(K, first_frame) * NM; it += (int)blockDim.x) lab[it] = L[it];
  {
    const int fl = max(K, first_frame - cxt);
    for (int it = tid; it < (first_frame - fl) * NM; it += (int)blockDim.x) {
      const int f = fl + it / NM, r = it % NM;
      lab[LNM + ((f - K) % R) * NM + r] = L[(long)f * NM + r];
    }
  }

  float pw[PX_PF];
  int pi[PX_PF];
  auto svc_load = [&](int f) {  // (clamped, unconditional: a frame past the last one re-reads the last one's lists, never used)
    const long o = (long)(min(f, last_frame) - first_frame) * KN;
#pragma unroll
    for (int u = 0; u < PX_PF; ++u) {
      const int e = min(lane + u * 64, KN - 1);
      pw[u] = W[o + e];
      pi[u] = I[o + e];
    }
  };
  auto svc_store = [&](int f) {
#pragma unroll
    for (int u = 0; u < PX_PF; ++u) pl[(f & 1) * KNP + lane + u * 64] = int2{pi[u], __float_as_int(pw[u])};
  };
  if (loader) {
    if (lk == 0) {
      svc_load(first_frame);
      svc_store(first_frame);
    }
    if (lk == (D > 1 ? 1 : 0)) {
      svc_load(first_frame + 1);
      svc_store(first_frame + 1);
    }
    svc_load(first_frame + 2 + lk);
  }
  lds_barrier();

  const int it = min(tid, NM - 1), q = it / M, c = it % M;
  int a[KP];
  float w[KP];
  auto fetch_lists = [&](int f, int (&ix)[KP], float (&ww)[KP]) {
    const int2 *ln = pl + (f & 1) * KNP;
#pragma unroll
    for (int j = 0; j < KP; ++j) {
      const int2 e = ln[(j < KLO ? j : min(j, knn - 1)) * N + q];
      ix[j] = e.x;
      ww[j] = __int_as_float(e.y);
    }
  };
  // frame f's indices -> LDS offsets.  shift = ((f - cxt - 1) % R) * NM once the window slides, 0 before; the clamp keeps an index
  // inside the list it addresses (topk: < min(f, cxt + 1) * N), i.e. on rows before the frame's own and inside the ring
  // An anchored lane (anchor_mark on the slot-0 weight, the class from the RAW slot-0 index, before the clamp to a row below): mk and
  // the value oh its output takes are made here, one frame ahead and behind the previous frame's stores; the frame itself pays one
  // select on p.  The marked list's offsets stay in range like any other's, so its label reads are harmless and its sum is dropped.
  // ORG: f is the frame's number n' in the item that starts at its origin, mb the offset of its long-term slot (0 or NM + RNM)
  auto to_offsets = [&](int f, int shift, int mb, int (&ix)[KP], float (&ww)[KP], int &mk, int &oh) {
    const int lim = min(f, cxt + K) * N - 1;
    mk = anchor_mark(ww[0]) ? -1 : 0;
    oh = __float_as_int(anchor_onehot(ix[0], M, c));
#pragma unroll
    for (int j = 0; j < KP; ++j) {
      const int i = min(max(ix[j], 0), lim);
      int o = i * M + c;
      if constexpr (ORG) {  // two selects, no branch: as an if / else hipcc makes it a divergent branch per neighbour
        const int os = o + shift, ow = os >= NM + RNM ? os - RNM : os;
        o = i >= N ? ow : o + mb;
      } else if (i >= LN) {
        o += shift;
        if (o >= LNM + RNM) o -= RNM;
      }
      ix[j] = o;
      if (j >= KLO && j >= knn) ww[j] = 0.f;  // padding slot: p + v * 0 = p
    }
  };
  // running offsets (wave-uniform): shift of the frame whose offsets are made next, store slot of the frame computed next
  int shift = first_frame > cxt + 1 ? ((first_frame - cxt - 1) % R) * NM : 0;
  int wslot = NM + ((first_frame - 1) % R) * NM;
  if constexpr (LM) {  // the same two with K, and a first frame inside the bank
    shift = first_frame > cxt + K ? ((first_frame - cxt - K) % R) * NM : 0;
    wslot = first_frame < K ? first_frame * NM : LNM + ((first_frame - K) % R) * NM;
  }
  auto next_shift = [&](int f) {  // shift of frame f -> shift of frame f + 1
    if (f + 1 > cxt + K) {
      shift += NM;
      if (shift == RNM) shift = 0;
    }
  };
  // ORG, all wave-uniform and like `shift` those of the frame whose offsets are made next: np its number in the item that starts at
  // its origin, mb its long-term slot, rs: it restarts, i.e. the frame computed now is its origin and is stored to mb as well.
  // next_origin(g): frame g's -> frame g + 1's, called where wslot is frame g's slot (the next slot is the restart's shift + NM)
  int np = first_frame - org0, mb = 0;
  bool rs = false;
  if constexpr (ORG) shift = ((org0 + max(0, np - cxt - 1)) % R) * NM;
  // (o1: orgs[min(g + 1, last_frame)], read from LDS a phase ahead so that its round trip is not in front of the barrier)
  auto next_origin = [&](int g, int o1) {
    rs = __builtin_amdgcn_readfirstlane(o1) == g;
    if (rs) {
      np = 1;
      mb = mb ? 0 : NM + RNM;
      shift = wslot + NM == NM + RNM ? 0 : wslot;
    } else if (++np > cxt + 1) {
      shift += NM;
      if (shift == RNM) shift = 0;
    }
  };
  int amk = 0, aoh = 0;  // all ones where this lane's node is anchored in the frame computed next; the bits of the value it then takes
  if (compute) {
    fetch_lists(first_frame, a, w);
    to_offsets(ORG ? np : first_frame, shift, mb, a, w, amk, aoh);
  }
  if constexpr (ORG) {
    next_origin(first_frame, orgs[min(first_frame + 1, last_frame)]);  // (orgs[] is behind the barrier above)
  } else {
    next_shift(first_frame);
  }
  lds_barrier();  // the read of slot first_frame & 1 above comes before loader 0's svc_store(first_frame + 2) into the same slot

  int turn = 0;       // (f - first_frame) % D
  int pslot = wslot;  // slot of frame f - 1 (the arg-max wave's)
  for (int f = first_frame; f <= last_frame; ++f) {
    int o2 = 0;  // ORG: the origin of frame f + 2
    if constexpr (ORG) o2 = orgs[min(f + 2, last_frame)];
    if (compute) {
      float v[KP];
#pragma unroll
      for (int j = 0; j < KP; ++j) v[j] = lab[a[j]];
      int na[KP];
      float nw[KP];
      fetch_lists(f + 1, na, nw);  // slot (f + 1) & 1: written before the previous barrier (past last_frame: unused)
      float p = 0.f;
#pragma unroll
      for (int j = 0; j < KP; ++j) p += v[j] * w[j];
      // an anchored node: exactly 1.0f / +0.0f, and every later frame and the arg-max wave read the clamped row.  A bit select on
      // two VGPRs made a frame ahead, (amk & aoh) | (~amk & p).  Written as the instruction: from the C expression hipcc goes back to
      // a v_cndmask on a lane mask kept in SGPRs across the barrier, which spilled four more SGPRs in this loop.
      // (make EXTRA=-DCRW_LABELPROP_RING_NO_ANCHORS: the kernel without it, the arm tools/anchor_lists_timing.py --also measures)
#ifndef CRW_LABELPROP_RING_NO_ANCHORS
      asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(p) : "v"(amk), "v"(aoh), "v"(p));
#endif
      lab[wslot + it] = p;  // the slot of frame f - R: out of every window since frame f - 1
      // ORG, frame f is the next frame's origin: a second store, to the long-term slot nobody reads in this phase -- and otherwise
      // the first store again (no branch in the chain)
      if constexpr (ORG) lab[(rs ? mb : wslot) + it] = p;
      L[(long)f * NM + it] = p;
      // nothing of the next frame's offsets is scheduled above the stores: hipcc otherwise lifts the first clamp, and with it the
      // wait for the first list entry (an LDS round trip), in front of the remaining list reads and the LDS store
      __builtin_amdgcn_sched_barrier(0);
      to_offsets(ORG ? np : f + 1, shift, mb, na, nw, amk, aoh);
#pragma unroll
      for (int j = 0; j < KP; ++j) {
        a[j] = na[j];
        w[j] = nw[j];
      }
    } else if (loader) {
      if (turn == lk) {
        svc_store(f + 2);  // slot f & 1: last read (frame f's lists) before the previous barrier
        svc_load(f + 2 + D);
      }
    } else if (f > first_frame) {  // arg-max of the previous frame (first maximum wins); its slot is next written R - 1 phases on
      argmax_rows(pred, T, N, M, f - 1, at, 64, lab + pslot, PlainLoad());
    }
    turn = turn + 1 == D ? 0 : turn + 1;
    if constexpr (!ORG) next_shift(f + 1);
    pslot = wslot;
    wslot = wslot + NM == LNM + RNM ? LNM : wslot + NM;  // (LM: a long-term slot's successor is the next slot, the ring's first after K - 1)
    if constexpr (ORG) next_origin(f + 1, o2);
    lds_barrier();
  }
  if (amax) {
    argmax_rows(pred, T, N, M, last_frame, at, 64, lab + pslot, PlainLoad());
  }
#undef K
#undef LN
#undef LNM
}

// ---- hyper-parameter sweeps (crw_labelprop_sweep_weights, crw_labelprop_propagate_batch) ----------------------------------------
// The lists of knn = k are the first k entries of the lists of any larger knn (selection is sequential: highest score, then lowest
// candidate index), so ONE selection at kcap = max(knns) (crw_labelprop_topk_scores: the logits instead of their softmax) serves
// every knn of a (radius, temp) pair; what is per knn is the softmax over the first knn logits -- the epilogues' expression, in
// their order: vmax = v[0]; ssum over j = 0 .. knn-1 (a prefix of the running sum); expf(v - vmax) / ssum.
constexpr int SW_MAXK = 16;  // knn values per call
struct SweepKnns {
  int n, k[SW_MAXK];
};
__global__ __launch_bounds__(256) void labelprop_sweep_weights_kernel(const float *__restrict__ V, int F, int kcap, int N, int kmax,
                                                                      SweepKnns ks, float *__restrict__ W) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;  // (frame, query)
  if (e >= (long)F * N) return;
  const int f = (int)(e / N), q = (int)(e - (long)f * N);
  const float *v = V + (long)f * kcap * N + q;
  const float vmax = v[0];
  float S[SW_MAXK];
#pragma unroll
  for (int i = 0; i < SW_MAXK; ++i) S[i] = 1.f;
  float ssum = 0.f;
  for (int j = 0; j < kmax; ++j) {
    const float x = v[(long)j * N];
    ssum += (x == -INFINITY) ? 0.f : expf(x - vmax);
#pragma unroll
    for (int i = 0; i < SW_MAXK; ++i)
      if (i < ks.n && ks.k[i] == j + 1) S[i] = ssum;
  }
  for (int j = 0; j < kmax; ++j) {
    const float x = v[(long)j * N];
    const float ex = expf(x - vmax);
#pragma unroll
    for (int i = 0; i < SW_MAXK; ++i)
      if (i < ks.n) W[(((long)i * F + f) * kmax + j) * N + q] = (j < ks.k[i] && x != -INFINITY) ? ex / S[i] : 0.f;
  }
}

// G configurations' chained frames first_frame .. last_frame, a workgroup per configuration (the chains run side by side on different
// CUs, so a chain is kept simple: no roles, one barrier per frame).  Frame 0 and the most recent R frames' soft labels sit in LDS
// (the ring of labelprop_gather_lds_kernel, same addressing; R covers every chained frame where they fit), older ones and the
// caller's frames before first_frame come from L in global memory.  The lists are read from global memory PB_CH neighbours at a
// time (they do not depend on the chain); the sum runs in neighbour order from 0.f like every other propagation kernel here, and
// padding slots (weight exactly 0, a valid index) leave it as it is: p + v * 0.f == p for the finite labels.
constexpr int PB_CH = 16;
// SLIDE: slide_row() on every index before the clamp (crw_labelprop_propagate_sliding_batch); ORG: slide_row_at() with the frame's
// origin, one origin array for the G configurations (crw_labelprop_propagate_origin_batch)
// LM (crw_labelprop_propagate_long_batch, include/crw_hip_sweepmem.h): K = n_long long-term frames, [K][NM] in front of the ring
// [R][NM].  Frame f < K sits at slot f for good (the caller's are copied in, frames first_frame .. K - 1 of the call are computed
// into their slots like any other), frame f >= K at K + (f - K) % R; the ring holds frames this launch computed and nothing else.
// slide_row_at<false, true> clamps an index into the list it addresses and makes it a row of L below frame n; `first`, `old` and the
// ring's epochs are then those of the other instances with K * N in the place of N and frames counted from K.  No seed.
template <bool SLIDE, bool ORG, bool LM = false>
__global__ __launch_bounds__(1024) void labelprop_chain_batch_kernel(const float *__restrict__ seed, const float *__restrict__ W,
                                                                     const int32_t *__restrict__ I, long i_stride, int T, int N, int M,
                                                                     int knn, int first_frame, int last_frame, float *L,
                                                                     float *__restrict__ pred, int R, int cxt,
                                                                     OriginArg<LM> origin) {
  static_assert(!LM || (SLIDE && !ORG), "a bank of long-term frames: the sliding rule, no origins");
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, nt = (int)blockDim.x, NM = N * M, KN = knn * N, g = blockIdx.x;
  W += (long)g * (T - first_frame) * KN;
  I += (long)g * i_stride;
  L += (long)g * T * NM;
  pred += (long)g * N * T;
  const int K = long_frames<LM>(origin);
  float *l0 = sm, *ring = l0 + (LM ? K * NM : NM);  // [NM] (LM: [K][NM]), [R][NM]
  if constexpr (LM) {  // the long-term frames the caller filled
    for (int it = tid; it < min(K, first_frame) * NM; it += nt) l0[it] = ld_l2(L + it);
  } else {
    init_frame0<true, true>(seed, L, pred, l0, T, N, M, tid, nt);
  }
  __syncthreads();
  const int RNM = R * NM;
  for (int n = first_frame; n <= last_frame; ++n) {
    const float *Wn = W + (long)(n - first_frame) * KN;
    const int32_t *In = I + (long)(n - first_frame) * KN;
    // frames [lo_f, n - 1] live in the ring; a frame f sits at flat offset (f % R) * NM (LM: ((f - K) % R) * NM)
    const int lo_f = LM ? max(max(first_frame, K), n - R + 1) : max(first_frame, n - R + 1);
    const int lo_idx = lo_f * N;               // first label-list row that is in the ring
    // flat offset of the older of the (at most) two ring epochs in view (LM: in rows counted from frame K; unused while n < K)
    const int epoch_base = LM ? (max(n - K, 0) / R - 1) * RNM + K * NM : (n / R - 1) * RNM;
    const int row_lim = n * N - 1;
    const int org = origin_at<ORG>(origin, n);
    float *slot = LM ? (n < K ? l0 + n * NM : ring + ((n - K) % R) * NM) : ring + (n % R) * NM;
    for (int it = tid; it < NM; it += nt) {
      const int q = it / M, c = it % M;
      float p = 0.f;
      // an anchored node: the mark is configuration g's (W), the class may be shared (I with i_stride 0); its sum is dropped
      const bool mk = SLIDE && anchor_mark(Wn[q]);
      for (int j0 = 0; j0 < knn; j0 += PB_CH) {
        int idx[PB_CH];
        float w[PB_CH], v[PB_CH];
#pragma unroll
        for (int u = 0; u < PB_CH; ++u) {
          const int jj = min(j0 + u, knn - 1);
          const int raw_i = SLIDE ? slide_row_at<ORG, LM>(In[jj * N + q], n, org, N, cxt, K) : In[jj * N + q];
          idx[u] = min(max(raw_i, 0), row_lim);  // in range whatever the lists hold (topk: < min(n, cxt + 1) * N)
          w[u] = Wn[jj * N + q];
        }
#pragma unroll
        for (int u = 0; u < PB_CH; ++u) {
          // frame 0 sits in l0 = sm[0, NM), the ring behind it; a label older than the ring comes from global memory
          int off = idx[u] * M + c - epoch_base;
          if (off >= RNM) off -= RNM;
          const bool first = idx[u] < (LM ? K * N : N), old = !first && idx[u] < lo_idx;
          const int a = first ? idx[u] * M + c : (old ? 0 : (LM ? K * NM : NM) + off);
          v[u] = sm[a];
          if (old) v[u] = ld_l2(L + (long)idx[u] * M + c);
        }
#pragma unroll
        for (int u = 0; u < PB_CH; ++u)
          if (j0 + u < knn) p += v[u] * w[u];
      }
      if (mk) p = anchor_onehot(In[q], M, c);
      st_l2(L + ((long)n * N + q) * M + c, p);
      slot[it] = p;
    }
    __syncthreads();  // frame n's labels are in LDS; its slot is next written R frames (barriers) later
    argmax_rows(pred, T, N, M, n, tid, nt, slot, PlainLoad());
  }
}

// frames t0 .. T-1 of configuration g = blockIdx.y, none of which reads a label this launch writes: a workgroup per (frame,
// configuration), neighbours' labels from L (global memory).  One configuration (crw_labelprop_propagate): gridDim.y = 1, i_stride unused.
constexpr int TAIL_NT = 256, TAIL_CH = 16;
__global__ __launch_bounds__(TAIL_NT) void labelprop_tail_batch_kernel(const float *__restrict__ W, const int32_t *__restrict__ I,
                                                                       long i_stride, int T, int N, int M, int knn, int first_frame,
                                                                       int t0, float *L, float *__restrict__ pred) {
  extern __shared__ __attribute__((aligned(16))) float slot[];  // [N * M]
  const int tid = threadIdx.x, NM = N * M, n = t0 + blockIdx.x, g = blockIdx.y;
  const float *Wn = W + ((long)g * (T - first_frame) + (n - first_frame)) * knn * N;
  const int32_t *In = I + (long)g * i_stride + (long)(n - first_frame) * knn * N;
  L += (long)g * T * NM;
  pred += (long)g * N * T;
  const int row_lim = n * N - 1;
  for (int it = tid; it < NM; it += TAIL_NT) {
    const int q = it / M, c = it % M;
    float p = 0.f;
    for (int j0 = 0; j0 < knn; j0 += TAIL_CH) {
      int idx[TAIL_CH];
      float w[TAIL_CH], v[TAIL_CH];
#pragma unroll
      for (int u = 0; u < TAIL_CH; ++u) {
        const int jj = min(j0 + u, knn - 1);
        idx[u] = min(max(In[jj * N + q], 0), row_lim);
        w[u] = Wn[jj * N + q];
      }
#pragma unroll
      for (int u = 0; u < TAIL_CH; ++u) v[u] = L[(long)idx[u] * M + c];
#pragma unroll
      for (int u = 0; u < TAIL_CH; ++u)
        if (j0 + u < knn) p += v[u] * w[u];
    }
    L[((long)n * N + q) * M + c] = p;
    slot[it] = p;
  }
  __syncthreads();
  argmax_rows(pred, T, N, M, n, tid, TAIL_NT, slot, PlainLoad());
}

// xent[a, i] = logsumexp_c A_i[c, a] - A_i[a, a],  A_i[c, a] = <ehat[i,c,0:C-1], ehat[i,a,1:C]> / 0.1
__global__ __launch_bounds__(64) void xent_metric_kernel(const float *__restrict__ ehat, int T, int N, int C,
                                                         float *__restrict__ xent) {
  extern __shared__ float col[];  // [N]
  const int a = blockIdx.x, i = blockIdx.y, lane = threadIdx.x;
  const float *ea = ehat + ((long)i * N + a) * C + 1;
  float m = -INFINITY;
  for (int c = 0; c < N; ++c) {
    const float *ec = ehat + ((long)i * N + c) * C;
    float d = 0.f;
    for (int ch = lane; ch < C - 1; ch += 64) d += ec[ch] * ea[ch];
    d = wave_sum(d) / 0.1f;
    if (lane == 0) col[c] = d;
    m = fmaxf(m, d);
  }
  __syncthreads();
  float s = 0.f;
  for (int c = lane; c < N; c += 64) s += expf(col[c] - m);
  s = wave_sum(s);
  if (lane == 0) xent[(long)a * (T - 1) + i] = (logf(s) + m) - col[a];
}

// The same metric with a workgroup per FRAME: the frame's features sit in LDS twice (as they are, and shifted by one channel, so both
// operands of a pair are read as aligned float4), every thread takes N * N / 256 (c, a) pairs, then a thread per column does the
// log-sum-exp.  12240 one-wave workgroups with 48 serial wave reductions each took 92 us at cfg5 -- on the way to the host's
// change-point search, which is the tail of that step.
constexpr int XENT_NT = 256;
__global__ __launch_bounds__(XENT_NT) void xent_metric_frame_kernel(const float *__restrict__ ehat, int T, int N, int C, float *__restrict__ xent) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int LD = ((C + 3) & ~3) + 4;  // row stride: a multiple of 4 floats, consecutive rows 4 banks apart
  float *e0 = sm, *e1 = e0 + N * LD, *A = e1 + N * LD;  // e1[a][k] = e[a][k + 1]; A[c][a]
  const int i = blockIdx.x, tid = threadIdx.x;
  const float *src = ehat + (long)i * N * C;
  for (int it = tid; it < N * LD; it += XENT_NT) {
    const int r = it / LD, k = it - r * LD;
    e0[it] = k < C - 1 ? src[r * C + k] : 0.f;       // channels 0 .. C-2, zero beyond
    e1[it] = k < C - 1 ? src[r * C + k + 1] : 0.f;   // channels 1 .. C-1
  }
  __syncthreads();
  const int K4 = (C - 1 + 3) >> 2;
  for (int p = tid; p < N * N; p += XENT_NT) {
    const int c = p / N, a = p - c * N;
    const float4 *x = reinterpret_cast<const float4 *>(e0 + c * LD), *y = reinterpret_cast<const float4 *>(e1 + a * LD);
    float d = 0.f;
    for (int k = 0; k < K4; ++k) {
      const float4 u = x[k], v = y[k];
      d += u.x * v.x + u.y * v.y + u.z * v.z + u.w * v.w;
    }
    A[c * N + a] = d / 0.1f;
  }
  __syncthreads();
  for (int a = tid; a < N; a += XENT_NT) {
    float m = -INFINITY;
    for (int c = 0; c < N; ++c) m = fmaxf(m, A[c * N + a]);
    float sum = 0.f;
    for (int c = 0; c < N; ++c) sum += expf(A[c * N + a] - m);
    xent[(long)a * (T - 1) + i] = (logf(sum) + m) - A[a * N + a];
  }
}

}  // namespace
}  // namespace crw

using namespace crw;

namespace {

// one route choice for both output modes: raw = 0 softmax weights (crw_labelprop_topk_grid), 1 the selected logits
// (crw_labelprop_topk_scores) -- the same kernels, the same selection, another last line of the epilogue
// origin (crw_labelprop_topk_origin; NULL: every frame scores from frame 0): the route is still chosen from the whole call's
// arguments -- a restart frame has fewer candidates than the bound the route was chosen for, never more
// n_long (crw_labelprop_topk_long; 0: frame 0 alone is long-term, the instances the other entry points have always run): the lists
// hold up to n_long + cxt_size frames, and the routes are chosen for that length.  route: 0 auto, 1 the vector kernel, 2 the
// matrix-core kernels -- CRW_EINVAL where the forced one does not apply
int topk_grid(const float *ehat, int T, int N, int C, int cxt_size, int radius, float temp, int knn, int first_frame, int grid_w, float *W,
              int32_t *I, int raw, const int32_t *origin, crw_stream_t stream, int n_long = 0, int route = 0, float long_bias = 0.f) {
  crw::clear_stale_error();
  if (!ehat || !W || !I || T < 2 || N < 1 || C < 1 || cxt_size < 1 || radius < 1 || knn < 1 || knn > MAX_KNN ||
      !(temp > 0.f) || first_frame < 1 || first_frame >= T || grid_w < 1 || N % grid_w)
    return CRW_EINVAL;
  const long gh = N / grid_w;
  const long max_keys = (long)cxt_size + (n_long ? n_long : 1);
  const long max_nf = max_keys < T - 1 ? max_keys : T - 1;
  const long max_bi = (2L * radius - 1 < gh) ? 2L * radius - 1 : gh, max_bj = (2L * radius - 1 < grid_w) ? 2L * radius - 1 : grid_w;
  const size_t lds = (((size_t)C + 3) & ~(size_t)3) * 4 + (size_t)(max_nf * max_bi * max_bj) * 4;
  // a radargram's patch column with at least one full tile of queries: scores on the fp32 matrix cores (labelprop_topk_mfma_kernel).
  // CRW_LABELPROP_TOPK_VALU=1 keeps the vector kernel (A/B)
  static const bool valu = getenv("CRW_LABELPROP_TOPK_VALU") && getenv("CRW_LABELPROP_TOPK_VALU")[0] == '1';
  const long maxcand = max_nf * max_bi;
  const bool column = grid_w == 1 && !(route ? route == 1 : valu) && N >= TK_Q && (((uintptr_t)ehat) & 15) == 0;
  hipStream_t s = (hipStream_t)stream;
  if (column && (C == 64 || C == 128 || C == 256) && maxcand <= 64L * TK_NV && (size_t)TK_Q * maxcand * 4 <= 150 * 1024) {
    if (C == 64) return launch_topk_mfma<4>(ehat, T, N, cxt_size, radius, temp, knn, first_frame, (int)max_nf, (int)max_bi, W, I, raw, origin, n_long, s, long_bias);
    if (C == 128) return launch_topk_mfma<8>(ehat, T, N, cxt_size, radius, temp, knn, first_frame, (int)max_nf, (int)max_bi, W, I, raw, origin, n_long, s, long_bias);
    return launch_topk_mfma<16>(ehat, T, N, cxt_size, radius, temp, knn, first_frame, (int)max_nf, (int)max_bi, W, I, raw, origin, n_long, s, long_bias);
  }
  // longer lists (radius 30 / 60 at 80 - 100 context frames): any number of chunks; a single frame's band must fit one chunk
  if (column && (C == 64 || C == 128) && max_bi <= TK_LONG_CAND) {
    if (C == 64) return launch_topk_mfma_long<4>(ehat, T, N, cxt_size, radius, temp, knn, first_frame, (int)max_nf, (int)max_bi, W, I, raw, origin, n_long, s, long_bias);
    return launch_topk_mfma_long<8>(ehat, T, N, cxt_size, radius, temp, knn, first_frame, (int)max_nf, (int)max_bi, W, I, raw, origin, n_long, s, long_bias);
  }
  if (lds > 60 * 1024 || route == 2) return CRW_EINVAL;
  CRW_ROUTE("labelprop.topk_valu");
  if (n_long && long_bias != 0.f)
    hipLaunchKernelGGL((labelprop_topk_kernel<false, true, true>), dim3(N, T - first_frame), dim3(256), lds, (hipStream_t)stream, ehat, T, N, C,
                       cxt_size, radius, temp, knn, first_frame, grid_w, W, I, raw, LongFrames{n_long, long_bias});
  else if (n_long)
    hipLaunchKernelGGL((labelprop_topk_kernel<false, true>), dim3(N, T - first_frame), dim3(256), lds, (hipStream_t)stream, ehat, T, N, C,
                       cxt_size, radius, temp, knn, first_frame, grid_w, W, I, raw, LongFrames{n_long, 0.f});
  else if (origin)
    hipLaunchKernelGGL((labelprop_topk_kernel<true, false>), dim3(N, T - first_frame), dim3(256), lds, (hipStream_t)stream, ehat, T, N, C, cxt_size,
                       radius, temp, knn, first_frame, grid_w, W, I, raw, origin);
  else
    hipLaunchKernelGGL((labelprop_topk_kernel<false, false>), dim3(N, T - first_frame), dim3(256), lds, (hipStream_t)stream, ehat, T,
                       N, C, cxt_size, radius, temp, knn, first_frame, grid_w, W, I, raw, origin);
  return check_launch();
}

// what every propagation entry point refuses (each adds its own: cxt_size, G, the knn cap)
bool bad_propagate_args(const float *W, const int32_t *I, const float *L, const float *pred, int T, int N, int M, int knn, int first_frame) {
  return !W || !I || !L || !pred || T < 2 || N < 1 || M < 1 || knn < 1 || first_frame < 1 || first_frame >= T;
}

// the split of the reference rule: frames from t0 on read no label of the call -- one frame alone, or every frame beyond the context
// bound; the chained frames are first_frame .. t0 - 1 (none when t0 == first_frame)
int chain_end(int T, int first_frame, int cxt_size) {
  return (T - first_frame == 1) ? first_frame : (first_frame > cxt_size + 1 ? first_frame : (cxt_size + 1 < T ? cxt_size + 1 : T));
}

// frames t0 .. T - 1 of G configurations, all at once (nothing to do when t0 == T)
int launch_tail(const float *W, const int32_t *I, long i_stride, int G, int T, int N, int M, int knn, int first_frame, int t0, float *L,
                float *pred, hipStream_t s) {
  if (t0 >= T) return CRW_OK;
  hipLaunchKernelGGL(labelprop_tail_batch_kernel, dim3(T - t0, G), dim3(TAIL_NT), (size_t)N * M * 4, s, W, I, i_stride, T, N, M, knn,
                     first_frame, t0, L, pred);
  return check_launch();
}

// the role kernels (labelprop_prefix_kernel, labelprop_slide_kernel): compute waves (64 outputs each) + 1..4 list loaders (fewer
// when the outputs need more compute waves) + the arg-max wave; nlab frames of labels and the two list slots in LDS
int chain_ncw(long NM) { return (int)((NM + 63) / 64); }
int chain_nld(long NM) { return PX_NT / 64 - 1 - chain_ncw(NM) < 4 ? PX_NT / 64 - 1 - chain_ncw(NM) : 4; }
size_t chain_lds(long nlab, long NM) { return (size_t)(((nlab * NM + 1) & ~1L) * 4 + 16L * 64 * PX_PF); }
// ... and where it can run: the neighbours in registers (32 spill), at most 6 compute waves (N * M <= 384: a loader and the arg-max wave
// beside them), a frame's lists in the loader's registers, the labels within the 150 KiB
bool chain_fits(int knn, long NM, long KN, size_t lds) { return knn <= 24 && chain_nld(NM) >= 1 && KN <= 64 * PX_PF && lds <= 150 * 1024; }

// KP = knn rounded up to the register instances.  RING: the slide kernel (every frame chained, `last` unused), else the prefix kernel
// over frames first_frame .. last (cxt, R unused)
// origin (RING only, crw_labelprop_propagate_origin): the slide kernel's ORG instance; NULL: the instance it has always been
template <int KP, bool RING>
int launch_chain_kp(const float *seed, const float *W, const int32_t *I, int T, int N, int M, int knn, int first_frame, int last, int cxt, int R,
                    size_t lds, float *L, float *pred, const int32_t *origin, int n_long, hipStream_t s) {
  const int ncw = chain_ncw((long)N * M);
  const dim3 block((ncw + chain_nld((long)N * M) + 1) * 64);
  if constexpr (RING) {
    if (origin) CRW_ROUTE("labelprop.slide_ring_origin");
    else CRW_ROUTE("labelprop.slide_ring");
    if (n_long)  // crw_labelprop_propagate_long: the LM instance, whatever n_long is
      return launch_big_lds<labelprop_slide_kernel<KP, false, true>>(dim3(1), block, lds, s, seed, W, I, T, N, M, knn, first_frame, cxt, R, L,
                                                                     pred, ncw, LongFrames{n_long, 0});
    if (origin)
      return launch_big_lds<labelprop_slide_kernel<KP, true, false>>(dim3(1), block, lds, s, seed, W, I, T, N, M, knn, first_frame, cxt, R, L,
                                                                     pred, ncw, origin);
    return launch_big_lds<labelprop_slide_kernel<KP, false, false>>(dim3(1), block, lds, s, seed, W, I, T, N, M, knn, first_frame, cxt, R, L,
                                                                    pred, ncw, origin);
  } else {
    CRW_ROUTE("labelprop.propagate_prefix");
    return launch_big_lds<labelprop_prefix_kernel<KP>>(dim3(1), block, lds, s, seed, W, I, T, N, M, knn, first_frame, last, L, pred, ncw);
  }
}
template <bool RING>
int launch_chain(const float *seed, const float *W, const int32_t *I, int T, int N, int M, int knn, int first_frame, int last, int cxt, int R,
                 size_t lds, float *L, float *pred, const int32_t *origin, hipStream_t s, int n_long = 0) {
  if (knn <= 8) return launch_chain_kp<8, RING>(seed, W, I, T, N, M, knn, first_frame, last, cxt, R, lds, L, pred, origin, n_long, s);
  if (knn <= 16) return launch_chain_kp<16, RING>(seed, W, I, T, N, M, knn, first_frame, last, cxt, R, lds, L, pred, origin, n_long, s);
  return launch_chain_kp<24, RING>(seed, W, I, T, N, M, knn, first_frame, last, cxt, R, lds, L, pred, origin, n_long, s);
}
// frames of LDS the slide kernel's ORG instance keeps beside the two list slots: frame 0's slot, the ring, the second long-term
// slot, and origin[T] rounded up to whole frames
long slide_origin_frames(long R, long T, long NM) { return R + 2 + (T + NM - 1) / NM; }

// the one-workgroup walk over any lists (crw_labelprop_gather; SLIDE: the general route of crw_labelprop_propagate_sliding, the
// indices translated in the kernel)
// LM (crw_labelprop_propagate_long): n_long long-term frames, the same two selector sites
template <bool SLIDE, bool ORG = false, bool LM = false>
int launch_gather(const float *seed, const float *W, const int32_t *I, int T, int N, int M, int knn, int first_frame, int cxt, float *L,
                  float *pred, crw_stream_t stream, const int32_t *origin = nullptr, int n_long = 1) {
  crw::clear_stale_error();
  if (bad_propagate_args(W, I, L, pred, T, N, M, knn, first_frame)) return CRW_EINVAL;
  // LDS-resident form when the lists of a frame fit the prefetch registers and at least a few frames fit the ring
  const long NM = (long)N * M, KN = (long)knn * N;
  OriginArg<LM> origin_arg;
  if constexpr (LM) origin_arg = LongFrames{n_long, 0};
  else origin_arg = origin;
  const long budget = 150 * 1024 - 16 * KN;  // bytes left for frame 0 + the ring after the two (weight, index) list copies
  long R = budget > 0 ? budget / (4 * NM) - 1 : 0;
  if (R > T) R = T;
  static const char *force_global = getenv("CRW_LABELPROP_GATHER_GLOBAL");  // diagnostics: the L2-round-trip kernel
  if (KN <= (long)GATHER_NT * GATHER_PF && R >= 4 && (long)T * N < (1L << 30) / M && !force_global) {
    const size_t lds = (size_t)(4 * (NM * (R + 1) + 4 * KN));
    if constexpr (ORG) CRW_ROUTE("labelprop.slide_general_origin_lds");
    else if constexpr (SLIDE) CRW_ROUTE("labelprop.slide_general_lds");
    else CRW_ROUTE("labelprop.gather_lds");
    return launch_big_lds<labelprop_gather_lds_kernel<SLIDE, ORG, LM>>(dim3(1), dim3(GATHER_NT), lds, (hipStream_t)stream, seed, W, I, T, N, M,
                                                                       knn, first_frame, L, pred, (int)R, cxt, origin_arg);
  }
  if constexpr (ORG) CRW_ROUTE("labelprop.slide_general_origin_global");
  else if constexpr (SLIDE) CRW_ROUTE("labelprop.slide_general_global");
  else CRW_ROUTE("labelprop.gather_global");
  hipLaunchKernelGGL((labelprop_gather_kernel<SLIDE, ORG, LM>), dim3(1), dim3(1024), 0, (hipStream_t)stream, seed, W, I, T, N, M, knn,
                     first_frame, L, pred, cxt, origin_arg);
  return check_launch();
}

// the route of a batch launch: one site per name, shared by launch_propagate_batch and launch_propagate_long_batch (the batch with a
// bank of long-term frames is the sliding batch's route, as crw_labelprop_propagate_long goes through labelprop.slide_ring)
template <bool SLIDE, bool ORG>
void route_propagate_batch() {
  if constexpr (ORG) CRW_ROUTE("labelprop.batch_slide_origin");
  else if constexpr (SLIDE) CRW_ROUTE("labelprop.batch_slide");
  else CRW_ROUTE("labelprop.batch_reference");
}

// SLIDE: every frame is chained (last = T - 1, no tail launch), the indices translated in the kernel
template <bool SLIDE, bool ORG = false>
int launch_propagate_batch(const float *seed, const float *W, const int32_t *I, size_t i_stride, int G, int T, int N, int M, int knn,
                           int first_frame, int cxt_size, float *L, float *pred, crw_stream_t stream, const int32_t *origin = nullptr) {
  crw::clear_stale_error();
  if (bad_propagate_args(W, I, L, pred, T, N, M, knn, first_frame) || G < 1 || G > 65535 || knn > MAX_KNN || cxt_size < 1) return CRW_EINVAL;
  const long NM = (long)N * M;
  if ((long)T * N >= (1L << 30) / M || NM * 4 > 30 * 1024) return CRW_EINVAL;  // 32-bit label offsets; frame 0 + a ring of >= 4 frames in LDS
  const int t0 = SLIDE ? T : chain_end(T, first_frame, cxt_size), last = t0 - 1;
  hipStream_t s = (hipStream_t)stream;
  if (last >= first_frame || seed) {  // (no chained frame: the kernel writes frame 0 from the seed and returns)
    long R = (150L * 1024) / (4 * NM) - 1;
    if (R > last + 1) R = last + 1;
    if (R < 2) R = 2;
    const int nt = (int)(NM >= 1024 ? 1024 : (NM + 63) / 64 * 64);
    route_propagate_batch<SLIDE, ORG>();
    const int rc = launch_big_lds<labelprop_chain_batch_kernel<SLIDE, ORG>>(dim3(G), dim3(nt), (size_t)(4 * NM * (R + 1)), s, seed, W, I,
                                                                            (long)i_stride, T, N, M, knn, first_frame, last, L, pred, (int)R,
                                                                            cxt_size, origin);
    if (rc != CRW_OK) return rc;
  }
  return launch_tail(W, I, (long)i_stride, G, T, N, M, knn, first_frame, t0, L, pred, s);
}

// the LM instance (crw_labelprop_propagate_long_batch): every frame is chained, n_long long-term frames and a ring of at least two in LDS
int launch_propagate_long_batch(const float *W, const int32_t *I, size_t i_stride, int G, int T, int N, int M, int knn, int first_frame,
                                int cxt_size, int n_long, float *L, float *pred, crw_stream_t stream) {
  crw::clear_stale_error();
  if (bad_propagate_args(W, I, L, pred, T, N, M, knn, first_frame) || G < 1 || G > 65535 || knn > MAX_KNN || cxt_size < 1) return CRW_EINVAL;
  if (n_long < 1 || n_long > T - 1 || first_frame < 1 || first_frame > T - 1) return CRW_EINVAL;
  const long NM = (long)N * M;
  if ((long)T * N >= (1L << 30) / M || NM * 4 > 30 * 1024) return CRW_EINVAL;  // as launch_propagate_batch
  long R = (150L * 1024) / (4 * NM) - n_long;
  if (R < 2) return CRW_EINVAL;  // n_long + 2 frames do not fit: one condition per geometry (N * M, n_long)
  if (R > T - first_frame) R = T - first_frame;
  if (R < 2) R = 2;
  const int nt = (int)(NM >= 1024 ? 1024 : (NM + 63) / 64 * 64);
  route_propagate_batch<true, false>();
  return launch_big_lds<labelprop_chain_batch_kernel<true, false, true>>(dim3(G), dim3(nt), (size_t)(4 * NM * (R + n_long)), (hipStream_t)stream,
                                                                         nullptr, W, I, (long)i_stride, T, N, M, knn, first_frame, T - 1, L,
                                                                         pred, (int)R, cxt_size, LongFrames{n_long, 0});
}

}  // namespace

extern "C" {

int crw_labelprop_topk_grid(const float *ehat, int T, int N, int C, int cxt_size, int radius, float temp, int knn, int first_frame,
                            int grid_w, float *W, int32_t *I, crw_stream_t stream) {
  return topk_grid(ehat, T, N, C, cxt_size, radius, temp, knn, first_frame, grid_w, W, I, 0, nullptr, stream);
}

int crw_labelprop_topk_scores(const float *ehat, int T, int N, int C, int cxt_size, int radius, float temp, int kcap, int first_frame,
                              int grid_w, float *V, int32_t *I, crw_stream_t stream) {
  return topk_grid(ehat, T, N, C, cxt_size, radius, temp, kcap, first_frame, grid_w, V, I, 1, nullptr, stream);
}

int crw_labelprop_topk(const float *ehat, int T, int N, int C, int cxt_size, int radius, float temp, int knn,
                       int first_frame, float *W, int32_t *I, crw_stream_t stream) {
  return crw_labelprop_topk_grid(ehat, T, N, C, cxt_size, radius, temp, knn, first_frame, 1, W, I, stream);
}

int crw_labelprop_gather(const float *seed, const float *W, const int32_t *I, int T, int N, int M, int knn,
                         int first_frame, float *L, float *pred, crw_stream_t stream) {
  return launch_gather<false>(seed, W, I, T, N, M, knn, first_frame, 0, L, pred, stream);
}

int crw_labelprop_propagate(const float *seed, const float *W, const int32_t *I, int T, int N, int M, int knn, int first_frame,
                            int cxt_size, float *L, float *pred, crw_stream_t stream) {
  crw::clear_stale_error();
  if (bad_propagate_args(W, I, L, pred, T, N, M, knn, first_frame) || cxt_size < 1) return CRW_EINVAL;
  const long NM = (long)N * M, KN = (long)knn * N;
  const int t0 = chain_end(T, first_frame, cxt_size), last = t0 - 1;  // the chained frames first_frame .. last (none when last < first_frame)
  static const bool seq = getenv("CRW_LABELPROP_GATHER_SEQ") && getenv("CRW_LABELPROP_GATHER_SEQ")[0] == '1';  // A/B: one-workgroup walk
  const size_t px_lds = chain_lds(last + 1, NM);  // every chained frame's labels, direct addressing
  const bool px_ok = last < first_frame ? !seed  // (a seed and no chained frame: the general kernel initialises frame 0)
                                        : chain_fits(knn, NM, KN, px_lds);
  if (seq || !px_ok || NM * 4 > 60 * 1024 || (long)T * N >= (1L << 30) / M)
    return crw_labelprop_gather(seed, W, I, T, N, M, knn, first_frame, L, pred, stream);
  hipStream_t s = (hipStream_t)stream;
  if (last >= first_frame) {
    const int rc = launch_chain<false>(seed, W, I, T, N, M, knn, first_frame, last, 0, 0, px_lds, L, pred, nullptr, s);
    if (rc != CRW_OK) return rc;
  }
  return launch_tail(W, I, 0, 1, T, N, M, knn, first_frame, t0, L, pred, s);
}

int crw_labelprop_propagate_sliding(const float *seed, const float *W, const int32_t *I, int T, int N, int M, int knn, int first_frame,
                                    int cxt_size, float *L, float *pred, crw_stream_t stream) {
  crw::clear_stale_error();
  if (bad_propagate_args(W, I, L, pred, T, N, M, knn, first_frame) || cxt_size < 1) return CRW_EINVAL;
  const long NM = (long)N * M, KN = (long)knn * N;
  // the ring kernel where frame 0 + min(cxt + 1, T - 1) ring slots fit.
  // CRW_LABELPROP_SLIDING_GENERAL=1 (read per call): the general kernels instead (A/B, tools/sliding_timing.py)
  const char *gen = getenv("CRW_LABELPROP_SLIDING_GENERAL");
  const long R = cxt_size + 1 < T - 1 ? cxt_size + 1 : T - 1;
  const size_t lds = chain_lds(R + 1, NM);
  const bool ring = !(gen && gen[0] == '1') && chain_fits(knn, NM, KN, lds) && (long)T * N < (1L << 30) / M;
  if (!ring) return launch_gather<true>(seed, W, I, T, N, M, knn, first_frame, cxt_size, L, pred, stream);
  return launch_chain<true>(seed, W, I, T, N, M, knn, first_frame, T - 1, cxt_size, (int)R, lds, L, pred, nullptr, (hipStream_t)stream);
}

// ---- include/crw_hip_restart.h: the same entry points with a per-frame origin (the ORG instances of the kernels above) ----------
int crw_labelprop_topk_origin(const float *ehat, int T, int N, int C, int cxt_size, int radius, float temp, int k, int first_frame,
                              int grid_w, const int32_t *origin, float *WV, int32_t *I, int raw, crw_stream_t stream) {
  if (raw != 0 && raw != 1) return CRW_EINVAL;
  return topk_grid(ehat, T, N, C, cxt_size, radius, temp, k, first_frame, grid_w, WV, I, raw, origin, stream);
}

int crw_labelprop_propagate_origin(const float *seed, const float *W, const int32_t *I, int T, int N, int M, int knn, int first_frame,
                                   int cxt_size, const int32_t *origin, float *L, float *pred, crw_stream_t stream) {
  if (!origin) return crw_labelprop_propagate_sliding(seed, W, I, T, N, M, knn, first_frame, cxt_size, L, pred, stream);
  crw::clear_stale_error();
  if (bad_propagate_args(W, I, L, pred, T, N, M, knn, first_frame) || cxt_size < 1) return CRW_EINVAL;
  const long NM = (long)N * M, KN = (long)knn * N;
  // the ring kernel where its labels -- one more frame than without origins, and origin[T] -- still fit; the same switch as above
  const char *gen = getenv("CRW_LABELPROP_SLIDING_GENERAL");
  const long R = cxt_size + 1 < T - 1 ? cxt_size + 1 : T - 1;
  const size_t lds = chain_lds(slide_origin_frames(R, T, NM), NM);
  const bool ring = !(gen && gen[0] == '1') && chain_fits(knn, NM, KN, lds) && (long)T * N < (1L << 30) / M;
  if (!ring) return launch_gather<true, true>(seed, W, I, T, N, M, knn, first_frame, cxt_size, L, pred, stream, origin);
  return launch_chain<true>(seed, W, I, T, N, M, knn, first_frame, T - 1, cxt_size, (int)R, lds, L, pred, origin, (hipStream_t)stream);
}

int crw_labelprop_propagate_origin_batch(const float *seed, const float *W, const int32_t *I, size_t i_stride, int G, int T, int N, int M,
                                         int knn, int first_frame, int cxt_size, const int32_t *origin, float *L, float *pred,
                                         crw_stream_t stream) {
  if (!origin) return launch_propagate_batch<true>(seed, W, I, i_stride, G, T, N, M, knn, first_frame, cxt_size, L, pred, stream);
  return launch_propagate_batch<true, true>(seed, W, I, i_stride, G, T, N, M, knn, first_frame, cxt_size, L, pred, stream, origin);
}

// ---- include/crw_hip_longmem.h: n_long long-term frames in place of frame 0 alone (the LM instances of the kernels above) ------
int crw_labelprop_topk_long(const float *ehat, int T, int N, int C, int cxt_size, int n_long, int radius, float temp, int k, int first_frame,
                            float *WV, int32_t *I, int raw, int route, crw_stream_t stream) {
  if ((raw != 0 && raw != 1) || route < 0 || route > 2 || n_long < 1 || n_long > T - 1) return CRW_EINVAL;
  return topk_grid(ehat, T, N, C, cxt_size, radius, temp, k, first_frame, 1, WV, I, raw, nullptr, stream, n_long, route);
}

// include/crw_hip_align.h: the LB instances of the two top-k kernels; a zero bias is crw_labelprop_topk_long itself
int crw_labelprop_topk_long_bias(const float *ehat, int T, int N, int C, int cxt_size, int n_long, int radius, float temp, int k,
                                 int first_frame, float *WV, int32_t *I, int raw, int route, float long_bias, crw_stream_t stream) {
  if (!(long_bias - long_bias == 0.f)) return CRW_EINVAL;  // NaN, +-inf
  if ((raw != 0 && raw != 1) || route < 0 || route > 2 || n_long < 1 || n_long > T - 1) return CRW_EINVAL;
  return topk_grid(ehat, T, N, C, cxt_size, radius, temp, k, first_frame, 1, WV, I, raw, nullptr, stream, n_long, route, long_bias);
}

int crw_labelprop_propagate_long(const float *W, const int32_t *I, int T, int N, int M, int knn, int first_frame, int cxt_size, int n_long,
                                 float *L, float *pred, int route, crw_stream_t stream) {
  crw::clear_stale_error();
  if (bad_propagate_args(W, I, L, pred, T, N, M, knn, first_frame) || cxt_size < 1 || n_long < 1 || n_long > T - 1 || route < 0 || route > 2)
    return CRW_EINVAL;
  const long NM = (long)N * M, KN = (long)knn * N;
  // the ring kernel where n_long long-term frames + cxt_size + 1 ring slots fit (the bound does not look at T: one condition per
  // geometry); it keeps min(cxt_size + 1, T - n_long) ring slots.  The switch of crw_labelprop_propagate_sliding holds for route 0
  const char *gen = getenv("CRW_LABELPROP_SLIDING_GENERAL");
  const long R = cxt_size + 1 < T - n_long ? cxt_size + 1 : T - n_long;
  const bool fits = chain_fits(knn, NM, KN, chain_lds((long)cxt_size + 1 + n_long, NM)) && (long)T * N < (1L << 30) / M;
  if (route == 2 && !fits) return CRW_EINVAL;
  const bool ring = route ? route == 2 : fits && !(gen && gen[0] == '1');
  if (!ring) return launch_gather<true, false, true>(nullptr, W, I, T, N, M, knn, first_frame, cxt_size, L, pred, stream, nullptr, n_long);
  return launch_chain<true>(nullptr, W, I, T, N, M, knn, first_frame, T - 1, cxt_size, (int)R, chain_lds(R + n_long, NM), L, pred, nullptr,
                            (hipStream_t)stream, n_long);
}

// include/crw_hip_sweepmem.h: the LM instance of the batch kernel
int crw_labelprop_propagate_long_batch(const float *W, const int32_t *I, size_t i_stride, int G, int T, int N, int M, int knn,
                                       int first_frame, int cxt_size, int n_long, float *L, float *pred, crw_stream_t stream) {
  return launch_propagate_long_batch(W, I, i_stride, G, T, N, M, knn, first_frame, cxt_size, n_long, L, pred, stream);
}

int crw_labelprop_sweep_weights(const float *V, int F, int kcap, int N, const int *knns, int nk, float *W, crw_stream_t stream) {
  crw::clear_stale_error();
  if (!V || !W || !knns || F < 1 || N < 1 || kcap < 1 || kcap > MAX_KNN || nk < 1 || nk > SW_MAXK) return CRW_EINVAL;
  SweepKnns ks;
  ks.n = nk;
  int kmax = 0;
  for (int i = 0; i < SW_MAXK; ++i) {
    ks.k[i] = i < nk ? knns[i] : 0;
    if (i < nk && (knns[i] < 1 || knns[i] > kcap)) return CRW_EINVAL;
    if (ks.k[i] > kmax) kmax = ks.k[i];
  }
  const long FN = (long)F * N;
  if (FN > (1L << 30)) return CRW_EINVAL;
  hipLaunchKernelGGL(labelprop_sweep_weights_kernel, dim3((unsigned)((FN + 255) / 256)), dim3(256), 0, (hipStream_t)stream, V, F, kcap, N,
                     kmax, ks, W);
  return check_launch();
}

int crw_labelprop_propagate_batch(const float *seed, const float *W, const int32_t *I, size_t i_stride, int G, int T, int N, int M,
                                  int knn, int first_frame, int cxt_size, float *L, float *pred, crw_stream_t stream) {
  return launch_propagate_batch<false>(seed, W, I, i_stride, G, T, N, M, knn, first_frame, cxt_size, L, pred, stream);
}

int crw_labelprop_propagate_sliding_batch(const float *seed, const float *W, const int32_t *I, size_t i_stride, int G, int T, int N, int M,
                                          int knn, int first_frame, int cxt_size, float *L, float *pred, crw_stream_t stream) {
  return launch_propagate_batch<true>(seed, W, I, i_stride, G, T, N, M, knn, first_frame, cxt_size, L, pred, stream);
}

int crw_xent_metric(const float *ehat, int T, int N, int C, float *xent, crw_stream_t stream) {
  crw::clear_stale_error();
  if (!ehat || !xent || T < 2 || N < 1 || C < 2 || (size_t)N * 4 > 60 * 1024) return CRW_EINVAL;
  const size_t ld = (((size_t)C + 3) & ~(size_t)3) + 4, frame_lds = (2 * (size_t)N * ld + (size_t)N * N) * 4;
  if (frame_lds <= 64 * 1024) {  // a frame's features fit LDS twice: a workgroup per frame
    CRW_ROUTE("xent.frame");
    hipLaunchKernelGGL(xent_metric_frame_kernel, dim3(T - 1), dim3(XENT_NT), frame_lds, (hipStream_t)stream, ehat, T, N, C, xent);
    return check_launch();
  }
  CRW_ROUTE("xent.column");
  hipLaunchKernelGGL(xent_metric_kernel, dim3(N, T - 1), dim3(64), (size_t)N * 4, (hipStream_t)stream, ehat, T, N, C,
                     xent);
  return check_launch();
}

}  // extern "C"
