// Fused front end of the CNN encoder (src/encoder.py:13-24,46-47):
//     x [cin,16,16] -> conv1 5x5 pad 1 (cin->8) -> ReLU -> maxpool 2x2/1 -> conv2 5x5 pad 1 (8->32)
//       -> ReLU -> maxpool 2x2/1 -> [100][32] channels-last bf16 planes (hi[,lo]) for conv3.
// Persistent workgroups stream patches, the next patch prefetched into registers; everything between the 1 KB input patch
// and the 6.4 KB output planes stays in LDS.  Forward: two 512-thread workgroups per CU (60 KB of LDS each) that fill each
// other's barrier waits (0.27 -> 0.21 ms per 16128 patches against one 1024-thread workgroup); backward: one 1024-thread
// workgroup per CU (98 KB of LDS).
//   conv1 (25*cin MACs per output, 3 % of this stage): fp32 VALU, exact.
//   conv2 (200 MACs per output): implicit GEMM on v_mfma_f32_16x16x32_bf16 with k = (tap, ci): one
//     32-deep k-step = 4 taps x 8 input channels, so an A fragment is ONE 16-byte channels-last read
//     of the pixel shifted by the lane group's tap.  SPLIT = 3 uses hi/lo operand pairs (fp32-grade).
// A backward kernel takes the forward values of a patch from the forward's saved record (front_bwd_saved_kernel, training) or
// recomputes them (front_bwd_kernel; front_bwd_tile_kernel on patches of any size) and then runs, per patch,
//     pool2/ReLU2 backward -> conv2 weight gradient (MFMA, transposed LDS reads) and bias gradient
//     -> conv2 backward-data (MFMA) -> pool1/ReLU1 backward -> conv1 weight/bias gradient (VALU),
// one function per phase, shared by the three kernels, accumulating the weight gradients in registers over its slice of
// patches; slices are added in a fixed order by front_slice_sum_kernel (deterministic).
#include "bf16_mma.h"
#include <type_traits>
#include <cstdlib>

namespace crw {
namespace {

// geometry
constexpr int XPW = 18;                    // 16x16 input patch, padded by 1
constexpr int C1W = 14, C1N = C1W * C1W;   // conv1 output 14x14
constexpr int A1W = 13, A1PW = 15;         // pool1 output 13x13, padded by 1 -> 15x15
constexpr int C2W = 11, C2N = C2W * C2W;   // conv2 output 11x11 (121)
constexpr int OW = 10, ON = 100;           // pool2 output
constexpr int D2PW = 19;                   // conv2-output gradient padded by 4 (for backward-data)
// Those planes (and the backward weights) are stored as two 16-channel halves of 32-byte rows: with 64-byte rows
// the ds_read_b128 lane groups of an MFMA fragment read (lanes {0-3,12-15,20-27}, ...) collide in the LDS banks;
// with [half][row][32 B] the 16 lanes of a group cover all 64 banks (MI355X_MICROARCH.md, LDS table).
constexpr int D2HALF = D2PW * D2PW * 32;   // bytes per half plane
constexpr int KS2 = 7;                     // conv2 k-steps (28 taps, 25 real)
constexpr int NTH = 1024, NWV = NTH / 64;  // 16 waves per workgroup: the stage is LDS-latency bound, one
                                           // 144 KB workgroup per CU, so latency is hidden by waves, not by workgroups

// What the forward pass keeps per patch for the backward pass when training (crw_enc_front_fwd `saved`), so that the
// backward kernel does not recompute conv1 -> pool1 -> conv2:
//   a1 hi / lo planes  [169 pixels][8 ch] bf16 (2704 B each)   the pool1 output = conv2's input (its weight gradient needs it)
//   k2 codes           [100 outputs][32 ch] 1 byte              pool2: argmax position (2 bits, first maximum in row-major
//   k1 codes           [169 outputs][8 ch]  1 byte (pad to 1360) order = torch's tie rule) | 4 if the maximum is > 0 (ReLU gate)
constexpr int SV_A1 = 169 * 16, SV_K2 = 100 * 32, SV_K1 = 1360;
constexpr int SV_OFF_A1L = SV_A1, SV_OFF_K2 = 2 * SV_A1, SV_OFF_K1 = 2 * SV_A1 + SV_K2, SV_BYTES = 2 * SV_A1 + SV_K2 + SV_K1;  // 9968
static_assert(SV_BYTES % 16 == 0 && SV_A1 % 16 == 0 && SV_K2 % 16 == 0, "16-byte chunks");

struct FrontArgs {
  const float *x;            // [P][cin][16][16]
  const float *w1, *b1;      // [8][cin][5][5], [8]
  const uint16_t *w2h, *w2l; // packed conv2 weights [7][32 co][32 k], k = 8*(tap%4) + ci, tap = 4*s + ..
  const float *b2;           // [32]
  uint16_t *yh, *yl;         // out planes [P][100][32]
  int P, cin;
  char *saved;               // optional [P][SV_BYTES] (training: see above)
};

// ---- shared forward pieces ----------------------------------------------------------------------
// pixel index in a W x W map (c1r / c2r).  PAD = true (backward kernels): the map carries a one-pixel border (never read by a
// valid pooling window, never initialised), so the pooling backward reads a pixel's 3x3 neighbourhood at constant offsets.
template <int W, bool PAD>
__device__ inline int map_idx(int y, int x) { return PAD ? (y + 1) * (W + 2) + x + 1 : y * W + x; }

// An LDS layout lists its fields once, in carve(): a kernel carves its dynamic LDS with it, the host calls the same function on
// a null base for the byte count of the launch (lds_bytes below), so the two cannot disagree.
struct Carver {
  char *p;
  __host__ __device__ char *take(size_t bytes) {
    char *r = p;
    p += (bytes + 15) & ~(size_t)15;
    return r;
  }
};
template <class Layout, class... Geometry>
size_t lds_bytes(Geometry... g) {
  Layout l;
  return reinterpret_cast<size_t>(l.carve(nullptr, g...));
}

struct FwdLds {
  float *xs;      // [cin][xw][xw]: the padded patch [18][18], or a tile's window [20][20]
  float *w1;      // [cin][25][8 co] + b1[8]
  float *c1r;     // [c1w][c1w][8]
  char *a1h, *a1l;  // [225][8] bf16 (16 B per pixel)
  char *w2h, *w2l;  // [7][2 k halves][32 co][16 k] bf16 (w2_lds_chunk)
  float *c2r;     // [c2w][c2w][32]
  // c1w / c2w: rows of the conv1 / conv2 maps, + 2 where they carry the border of map_idx<.., true>
  __host__ __device__ char *carve(char *base, int cin, int xw, int c1w, int c2w) {
    Carver c{base};
    xs = (float *)c.take(sizeof(float) * cin * xw * xw);
    w1 = (float *)c.take(sizeof(float) * (8 * cin * 25 + 8));
    c1r = (float *)c.take(sizeof(float) * c1w * c1w * 8);
    a1h = c.take(A1PW * A1PW * 16);
    a1l = c.take(A1PW * A1PW * 16);
    w2h = c.take(KS2 * 32 * 32 * 2);
    w2l = c.take(KS2 * 32 * 32 * 2);
    c2r = (float *)c.take(sizeof(float) * c2w * c2w * 32);
    return c.p;
  }
};

// conv1 + bias + ReLU over the CW x CW positions of an XW-wide window: thread = (output pixel, 4 of the 8 channels): 392 threads
// on a 16x16 patch (18, 14), 512 on a tile (20, 16).  The LDS weights are laid out [ci][tap][8 co] so the four weights of a tap
// are one 16-byte broadcast read: 2 LDS reads per 4 FMAs.
template <int XW, int CW, bool PAD>
__device__ inline void conv1_relu(const FwdLds &L, int cin, int tid) {
  if (tid < CW * CW * 2) {
    const int pix = tid >> 1, c0 = 4 * (tid & 1);
    const int y = pix / CW, xx = pix % CW;
    float4 acc = *reinterpret_cast<const float4 *>(L.w1 + 8 * cin * 25 + c0);
    for (int ci = 0; ci < cin; ++ci) {
      const float *xs = L.xs + (ci * XW + y) * XW + xx;
      const float *w = L.w1 + ci * 25 * 8 + c0;
#pragma unroll
      for (int t = 0; t < 25; ++t) {
        const float v = xs[(t / 5) * XW + t % 5];
        const float4 wv = *reinterpret_cast<const float4 *>(w + t * 8);
        acc.x = fmaf(v, wv.x, acc.x);
        acc.y = fmaf(v, wv.y, acc.y);
        acc.z = fmaf(v, wv.z, acc.z);
        acc.w = fmaf(v, wv.w, acc.w);
      }
    }
    *reinterpret_cast<float4 *>(L.c1r + map_idx<CW, PAD>(y, xx) * 8 + c0) = float4{relu_nan(acc.x), relu_nan(acc.y), relu_nan(acc.z), relu_nan(acc.w)};
  }
}

// maxpool 2x2/1 of c1r -> a1 planes (interior of the 15x15 padded image)
__device__ inline int argmax4(float a, float b, float c, float d);
template <int SPLIT, bool PAD, int NT = NTH>
__device__ inline void pool1(const FwdLds &L, int tid, char *sv = nullptr) {  // sv: this patch's saved record (or null)
  constexpr int ROW = (PAD ? C1W + 2 : C1W) * 8;
  for (int e = tid; e < A1W * A1W * 8; e += NT) {
    const int c = e & 7, p = e >> 3, y = p / A1W, x = p % A1W;
    const float *s = L.c1r + map_idx<C1W, PAD>(y, x) * 8 + c;
    const float v = max4_nan(s[0], s[8], s[ROW], s[ROW + 8]);
    const uint16_t h = f2bf(v), l = bf_lo(v, h);
    const int o = ((y + 1) * A1PW + x + 1) * 16 + 2 * c;
    *reinterpret_cast<uint16_t *>(L.a1h + o) = h;
    if (SPLIT == 3) *reinterpret_cast<uint16_t *>(L.a1l + o) = l;
    if (sv) {
      reinterpret_cast<uint16_t *>(sv)[e] = h;
      if (SPLIT == 3) reinterpret_cast<uint16_t *>(sv + SV_OFF_A1L)[e] = l;
      sv[SV_OFF_K1 + e] = (char)(argmax4(s[0], s[8], s[ROW], s[ROW + 8]) | (v > 0.f ? 4 : 0));
    }
  }
}

// The same front end runs on patches of any size as (patch, 10x10 tile of the pool2 output map [H-6][W-6]) work items.  A tile's
// receptive field is a 20x20 window of the patch (zeros outside it): conv1 over 16x16 positions, pool1 over the 15x15 a1 window
// conv2 needs, then conv2 / pool2 exactly as on a 16x16 patch -- which is the one-tile case with the window's border ring
// outside the maps.
constexpr int MXW = 20, MC1W = 16;  // window / conv1 extent of a tile

// pool1 over the whole 15x15 a1 window of the tile at (oy0, ox0) of an H x W patch: local (r, c) = a1 map (oy0 + r - 1,
// ox0 + c - 1); where that lies outside the a1 map [H-3][W-3] the plane holds conv2's zero padding instead
template <int SPLIT, bool PAD, int NT = NTH>
__device__ inline void pool1_window(const FwdLds &L, int tid, int oy0, int ox0, int H, int W) {
  constexpr int ROW = (PAD ? MC1W + 2 : MC1W) * 8;
  for (int e = tid; e < A1PW * A1PW * 8; e += NT) {
    const int c = e & 7, q = e >> 3, r = q / A1PW, cc = q % A1PW;
    const int ay = oy0 + r - 1, ax = ox0 + cc - 1;
    float v = 0.f;
    if (ay >= 0 && ay < H - 3 && ax >= 0 && ax < W - 3) {
      const float *s1 = L.c1r + map_idx<MC1W, PAD>(r, cc) * 8 + c;
      v = max4_nan(s1[0], s1[8], s1[ROW], s1[ROW + 8]);
    }
    const uint16_t h = f2bf(v);
    *reinterpret_cast<uint16_t *>(L.a1h + q * 16 + 2 * c) = h;
    if (SPLIT == 3) *reinterpret_cast<uint16_t *>(L.a1l + q * 16 + 2 * c) = bf_lo(v, h);
  }
}

// conv2 forward weights in LDS: the packed global planes [7 k-steps][32 co][4 chunks of 8 k] are stored as
// [7][2 k halves][32 co][2 chunks] (32-byte rows): on 64-byte rows the ds_read_b128 lane groups of a B-fragment read
// collide 2-way, on the split layout they cover all 64 banks (same trick as the d2 planes).
__device__ inline int w2_lds_chunk(int e) {  // 16-byte chunk index: global -> LDS
  const int ch = e & 3, co = (e >> 2) & 31, s = e >> 7;
  return ((s * 2 + (ch >> 1)) * 32 + co) * 2 + (ch & 1);
}

// conv2 + bias + ReLU on the matrix cores -> c2r [121][32] fp32.  16 output tiles (8 row x 2 column): one per wave of a
// 1024-thread workgroup; a 512-thread workgroup gives each wave two row tiles of the same column tile, so the weight
// fragments are read once for both (6 LDS reads per 6 MFMAs instead of 8).
template <int SPLIT, bool PAD, int NT = NTH>
__device__ inline void conv2_relu(const FwdLds &L, float bias, int tid) {  // bias = b2[16 (wave & 1) + lane % 16]
  constexpr int NW = NT / 64, U = 16 / NW;
  static_assert(NW % 2 == 0 && 16 % NW == 0, "waves per workgroup");
  const int lane = tid & 63, wave = tid >> 6, g = lane >> 4, r16 = lane & 15;
  const int j = wave & 1;
  int base[U];  // padded a1 pixel of tap (0,0)
  f32x4 acc[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    int i0 = 16 * ((wave + NW * u) >> 1) + r16;
    if (i0 >= C2N) i0 = 0;
    base[u] = (i0 / C2W) * A1PW + (i0 % C2W);
    acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int s = 0; s < KS2; ++s) {
    int tap = 4 * s + g;
    if (tap > 24) tap = 24;  // k-steps beyond tap 24 carry zero weights
    const int toff = (tap / 5) * A1PW + (tap % 5);
    const int o = (((s * 2 + (g >> 1)) * 32 + 16 * j + r16) * 2 + (g & 1)) * 16;
    const bf8 bh = *reinterpret_cast<const bf8 *>(L.w2h + o);
    bf8 bl;
    if (SPLIT == 3) bl = *reinterpret_cast<const bf8 *>(L.w2l + o);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bf8 ah = *reinterpret_cast<const bf8 *>(L.a1h + (base[u] + toff) * 16);
      if (SPLIT == 3) {
        const bf8 al = *reinterpret_cast<const bf8 *>(L.a1l + (base[u] + toff) * 16);
        acc[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, acc[u], 0, 0, 0);
        acc[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, acc[u], 0, 0, 0);
      }
      acc[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, acc[u], 0, 0, 0);
    }
  }
  const int co = 16 * j + r16;
  const float b = bias;
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 16 * ((wave + NW * u) >> 1) + 4 * g + r;
      if (i < C2N) L.c2r[map_idx<C2W, PAD>(i / C2W, i % C2W) * 32 + co] = relu_nan(acc[u][r] + b);
    }
}

// conv1 weights + bias and the conv2 forward weights -> LDS
template <int SPLIT, int NT = NTH>
__device__ inline void stage_weights(const FwdLds &L, const FrontArgs &a, int tid) {
  for (int e = tid; e < 8 * a.cin * 25; e += NT) {  // [co][ci][tap] -> [ci][tap][co]
    const int t = e % 25, ci = (e / 25) % a.cin, co = e / (25 * a.cin);
    L.w1[(ci * 25 + t) * 8 + co] = a.w1[e];
  }
  if (tid < 8) L.w1[8 * a.cin * 25 + tid] = a.b1[tid];
  for (int e = tid; e < KS2 * 32 * 32 / 8; e += NT) {
    const int d = w2_lds_chunk(e);
    reinterpret_cast<uint4 *>(L.w2h)[d] = reinterpret_cast<const uint4 *>(a.w2h)[e];
    if (SPLIT == 3) reinterpret_cast<uint4 *>(L.w2l)[d] = reinterpret_cast<const uint4 *>(a.w2l)[e];
  }
}
// 16x16 kernels: the patch loop writes the interior of the padded patch and of the a1 planes only; their borders are zeroed here
template <int NT = NTH>
__device__ inline void zero_patch_borders(float *xs, char *a1h, char *a1l, int cin, int tid) {
  for (int e = tid; e < cin * XPW * XPW; e += NT) xs[e] = 0.f;
  for (int e = tid; e < A1PW * A1PW * 4; e += NT) {
    reinterpret_cast<uint32_t *>(a1h)[e] = 0;
    reinterpret_cast<uint32_t *>(a1l)[e] = 0;
  }
}

// NT = 512: two workgroups share a CU (60 KB of LDS and <= 128 registers each) and fill each other's barrier waits; at 1024 threads
// the 122 registers of the hi/lo instance admit one workgroup per CU only.
template <int SPLIT, int NT>
__global__ __launch_bounds__(NT) void front_fwd_kernel(FrontArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  FwdLds L;
  L.carve(lds, a.cin, XPW, C1W, C2W);
  const int tid = threadIdx.x;
  zero_patch_borders<NT>(L.xs, L.a1h, L.a1l, a.cin, tid);
  stage_weights<SPLIT, NT>(L, a, tid);
  __syncthreads();
  const float b2r = a.b2[16 * ((tid >> 6) & 1) + (tid & 15)];  // read once: the barriers in the loop are memory clobbers
  // the next patch (cin*256 <= 512 floats, one per thread) is fetched while the current one is processed
  const int nx = a.cin * 256;
  float x_r = blockIdx.x < a.P ? a.x[(long)blockIdx.x * nx + min(tid, nx - 1)] : 0.f;
  for (int pt = blockIdx.x; pt < a.P; pt += gridDim.x) {
    if (tid < nx) L.xs[((tid >> 8) * XPW + ((tid >> 4) & 15) + 1) * XPW + (tid & 15) + 1] = x_r;
    if (pt + (int)gridDim.x < a.P) x_r = a.x[(long)(pt + gridDim.x) * nx + min(tid, nx - 1)];
    lds_barrier();
    conv1_relu<XPW, C1W, false>(L, a.cin, tid);
    lds_barrier();
    char *sv = a.saved ? a.saved + (long)pt * SV_BYTES : nullptr;
    pool1<SPLIT, false, NT>(L, tid, sv);
    lds_barrier();
    conv2_relu<SPLIT, false, NT>(L, b2r, tid);
    lds_barrier();
    // maxpool 2x2/1 -> output planes [100][32]
    for (int e = tid; e < ON * 32; e += NT) {
      const int c = e & 31, q = e >> 5, y = q / OW, x = q % OW;
      const float *s = L.c2r + (y * C2W + x) * 32 + c;
      const float v = max4_nan(s[0], s[32], s[C2W * 32], s[C2W * 32 + 32]);
      const uint16_t h = f2bf(v);
      a.yh[(long)pt * ON * 32 + e] = h;
      if (SPLIT == 3) a.yl[(long)pt * ON * 32 + e] = bf_lo(v, h);
      if (sv) sv[SV_OFF_K2 + e] = (char)(argmax4(s[0], s[32], s[C2W * 32], s[C2W * 32 + 32]) | (v > 0.f ? 4 : 0));
    }
    // the next iteration's first barrier orders these c2r reads before conv2_relu overwrites it
  }
}

// ---- the same front end on patches of any size (inference): one (patch, tile) work item at a time (see pool1_window) ----
// Output: planes [P][(H-6)*(W-6)][32] for crw_enc_conv3x3_map.
struct FrontMapArgs {
  FrontArgs f;     // x: [P][cin][H][W]; yh/yl: [P][(H-6)*(W-6)][32]
  int H, W, tiles_x, tiles_y;
};

template <int SPLIT, int NT>
__global__ __launch_bounds__(NT) void front_fwd_map_kernel(FrontMapArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int cin = a.f.cin, tid = threadIdx.x;
  FwdLds L;
  L.carve(lds, cin, MXW, MC1W, C2W);
  stage_weights<SPLIT, NT>(L, a.f, tid);
  const float b2r = a.f.b2[16 * ((tid >> 6) & 1) + (tid & 15)];
  const int H = a.H, W = a.W, Ho = H - 6, Wo = W - 6, ntile = a.tiles_x * a.tiles_y;
  const long nwork = (long)a.f.P * ntile;
  __syncthreads();
  for (long wk = blockIdx.x; wk < nwork; wk += gridDim.x) {
    const int pt = (int)(wk / ntile), tile = (int)(wk % ntile);
    const int oy0 = (tile / a.tiles_x) * OW, ox0 = (tile % a.tiles_x) * OW;
    // 20x20 window of the patch: local (r, c) = image (oy0 + r - 2, ox0 + c - 2)
    for (int e = tid; e < cin * MXW * MXW; e += NT) {
      const int ci = e / (MXW * MXW), r = (e / MXW) % MXW, c = e % MXW;
      const int iy = oy0 + r - 2, ix = ox0 + c - 2;
      L.xs[e] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? a.f.x[(((long)pt * cin + ci) * H + iy) * W + ix] : 0.f;
    }
    lds_barrier();
    conv1_relu<MXW, MC1W, false>(L, cin, tid);
    lds_barrier();
    pool1_window<SPLIT, false, NT>(L, tid, oy0, ox0, H, W);
    lds_barrier();
    conv2_relu<SPLIT, false, NT>(L, b2r, tid);
    lds_barrier();
    for (int e = tid; e < ON * 32; e += NT) {  // maxpool 2x2/1 -> the in-map part of the output tile
      const int c = e & 31, q = e >> 5, y = q / OW, x = q % OW;
      if (oy0 + y < Ho && ox0 + x < Wo) {
        const float *s2 = L.c2r + (y * C2W + x) * 32 + c;
        const float v = max4_nan(s2[0], s2[32], s2[C2W * 32], s2[C2W * 32 + 32]);
        const uint16_t h = f2bf(v);
        const long o = (((long)pt * Ho + oy0 + y) * Wo + ox0 + x) * 32 + c;
        a.f.yh[o] = h;
        if (SPLIT == 3) a.f.yl[o] = bf_lo(v, h);
      }
    }
    // the next iteration's first barrier orders these c2r reads before conv2_relu overwrites it
  }
}

// fp32 conv2 weight [32][8][5][5] -> forward planes [7][32 co][32 k] (k = 8*(tap-4s) + ci, zero beyond tap 24)
//                                 -> backward planes [25 tap][8 ci][32 co]
__global__ __launch_bounds__(256) void pack_w2_kernel(const float *__restrict__ w, uint16_t *fh, uint16_t *fl,
                                                      uint16_t *bh, uint16_t *bl) {
  for (int e = blockIdx.x * 256 + threadIdx.x; e < KS2 * 32 * 32; e += gridDim.x * 256) {
    const int k = e & 31, co = (e >> 5) & 31, s = e >> 10;
    const int tap = 4 * s + (k >> 3), ci = k & 7;
    const float v = tap < 25 ? w[(co * 8 + ci) * 25 + tap] : 0.f;
    const uint16_t h = f2bf(v);
    fh[e] = h;
    if (fl) fl[e] = bf_lo(v, h);
  }
  for (int e = blockIdx.x * 256 + threadIdx.x; e < 25 * 8 * 32; e += gridDim.x * 256) {
    const int co = e & 31, ci = (e >> 5) & 7, tap = e >> 8;
    const float v = w[(co * 8 + ci) * 25 + tap];
    const uint16_t h = f2bf(v);
    bh[e] = h;
    if (bl) bl[e] = bf_lo(v, h);
  }
}

// ---- backward -------------------------------------------------------------------------------------
struct FrontBwdArgs {
  FrontArgs f;               // forward inputs (yh/yl unused)
  const uint16_t *w2bh, *w2bl;  // conv2 backward planes [25][8][32]
  const float *dy;           // [P][100][32] fp32 gradient of the pool2 output
  float *part;               // [nslice][PART] partial sums: dW2 [32][8][25], db2 [32], dW1 [8][cin][25], db1 [8]
  int patches_per_block;
  long long *stamps;         // `make STAMPS=1` builds: [grid][NPHASE] cycles per phase summed over the slice (else null)
  // tiled variant only (front_bwd_tile_kernel): patches are [P][cin][H][W], dy is the map [P][H-6][W-6][32], the unit of
  // work is (patch, 10x10 tile of that map) and `patches_per_block` counts units
  int H, W, tiles_x, tiles_y;
};
[[maybe_unused]] constexpr int NPHASE = 10;
#ifdef CRW_CONV_STAMPS
#define FRONT_STAMP(k)                                                       \
  if (a.stamps && tid == 0) {                                                \
    const long long now_ = (long long)__builtin_amdgcn_s_memtime();          \
    phase_[k] += now_ - prev_;                                               \
    prev_ = now_;                                                            \
  }
#else
#define FRONT_STAMP(k)
#endif

// index (0..3) of the first maximum of a 2x2 window in row-major order (torch's max_pool2d tie rule)
__device__ inline int argmax4(float a, float b, float c, float d) {
  int k = 0;
  float m = a;
  if (b > m) { m = b; k = 1; }
  if (c > m) { m = c; k = 2; }
  if (d > m) { m = d; k = 3; }
  return k;
}

// Gradient reaching pixel (y, x) of a W x W map through a 2x2/stride-1 max-pool whose (W-1) x (W-1) output has
// gradient dout: the up to four windows containing the pixel route their gradient to it iff it is the FIRST
// maximum of the window in row-major order (torch's tie rule, = argmax4 above).  The four windows only involve
// the pixel's 3x3 neighbourhood, read once (8 LDS reads instead of 16).  in: bordered map (map_idx with
// PAD), dout: [W-1][W-1], both channel-interleaved with CS floats per pixel; the ReLU gate (in[pixel] > 0) is applied here.
template <int W, int CS>
__device__ inline float pool_bwd_pixel(const float *__restrict__ in, const float *__restrict__ dout, int y, int x, int c) {
  // `in` is the bordered map [(W+2)][(W+2)][CS]: the 8 neighbours sit at constant offsets from the pixel.  All 13
  // LDS reads (pixel, neighbours, the 4 window gradients at clamped addresses) are unconditional and independent,
  // so they are in flight together; branches around single loads made each of them a separate round trip.
  const float *ctr = in + ((y + 1) * (W + 2) + x + 1) * CS + c;
  float nb[3][3], dv[2][2];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) nb[dy][dx] = ctr[((dy - 1) * (W + 2) + (dx - 1)) * CS];
#pragma unroll
  for (int dyw = 0; dyw < 2; ++dyw)
#pragma unroll
    for (int dxw = 0; dxw < 2; ++dxw) {
      const int wy = min(max(y - dyw, 0), W - 2), wx = min(max(x - dxw, 0), W - 2);
      dv[dyw][dxw] = dout[(wy * (W - 1) + wx) * CS + c];
    }
  const float mine = nb[1][1];
  float gsum = 0.f;
#pragma unroll
  for (int dyw = 0; dyw < 2; ++dyw)
#pragma unroll
    for (int dxw = 0; dxw < 2; ++dxw) {
      const int wy = y - dyw, wx = x - dxw;
      bool win = mine > 0.f && wy >= 0 && wy < W - 1 && wx >= 0 && wx < W - 1;  // ReLU; border values only meet invalid windows
      const int k = dyw * 2 + dxw;  // this pixel's position in the window
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j != k) {
          const float v = nb[1 - dyw + (j >> 1)][1 - dxw + (j & 1)];
          win = win && (j < k ? mine > v : mine >= v);
        }
      gsum += win ? dv[dyw][dxw] : 0.f;
    }
  return gsum;
}

// The same gradient from what the forward saved for a pooling output: a code byte per window (argmax position | 4 if the maximum
// is > 0, see SV_K2 / SV_K1) instead of the window's values -- 8 LDS reads per pixel instead of 13 and no comparisons.
// codes, dout: [WO][WO][CS] of the WO x WO pooling output; (y, x): pixel of the (WO+1) x (WO+1) input map.
template <int WO, int CS>
__device__ inline float pool_bwd_code(const char *__restrict__ codes, const float *__restrict__ dout, int y, int x, int c) {
  float gsum = 0.f;
#pragma unroll
  for (int dyw = 0; dyw < 2; ++dyw)
#pragma unroll
    for (int dxw = 0; dxw < 2; ++dxw) {
      const int wy = y - dyw, wx = x - dxw;
      const bool ok = wy >= 0 && wy < WO && wx >= 0 && wx < WO;
      const int idx = (min(max(wy, 0), WO - 1) * WO + min(max(wx, 0), WO - 1)) * CS + c;
      const int code = codes[idx];
      const float d = dout[idx];
      gsum += (ok && code == (4 | (dyw * 2 + dxw))) ? d : 0.f;  // this pixel is the window's first maximum and it is > 0
    }
  return gsum;
}

// ---- the phases of the three backward kernels -------------------------------------------------------------------------
// front_bwd_saved_kernel (training at 16x16, from the forward's saved record), front_bwd_kernel (16x16, recomputes the forward)
// and front_bwd_tile_kernel (any patch size, one tile at a time) differ in where the forward values come from and in the extents
// of the conv1 / pool1 maps (14 / 13 against a tile's 16 / 15).  From the pool2 backward on they run the functions below.

// LDS of the backward proper, behind each kernel's forward part
struct BwdLds {
  char *wbh, *wbl;  // conv2 backward weights [25 tap][2 co halves][8 ci][16 co] bf16
  char *d2h, *d2l;  // dC2 (masked), padded by 4, [co half][pix][16] bf16
  float *dyb;       // dy of this patch / tile [100][32]; dead after the pool2 backward, when dA1 (and dC1) alias it
  __host__ __device__ char *carve(char *base) {
    Carver c{base};
    wbh = c.take(25 * 8 * 32 * 2);
    wbl = c.take(25 * 8 * 32 * 2);
    d2h = c.take(2 * D2HALF);
    d2l = c.take(2 * D2HALF);
    dyb = (float *)c.take(sizeof(float) * ON * 32);
    return c.p;
  }
};
// the recomputing kernels: the forward's LDS with bordered conv maps (16x16: xw = 18, c1w = 14; tiles: 20, 16), then BwdLds
struct RecomputeLds {
  FwdLds F;
  BwdLds B;
  __host__ __device__ char *carve(char *base, int cin, int xw, int c1w) {
    return B.carve(F.carve(base, cin, xw, c1w + 2, C2W + 2));
  }
};
struct SavedLds {
  float *xs;        // [cin][18][18]
  char *a1h, *a1l;  // [225][8] bf16: the saved pool1 planes inside conv2's zero padding
  BwdLds B;
  char *k2s, *k1s;  // the saved pooling codes of this patch
  __host__ __device__ char *carve(char *base, int cin) {
    Carver c{base};
    xs = (float *)c.take(sizeof(float) * cin * XPW * XPW);
    a1h = c.take(A1PW * A1PW * 16);
    a1l = c.take(A1PW * A1PW * 16);
    c.p = B.carve(c.p);
    k2s = c.take(SV_K2);
    k1s = c.take(SV_K1);
    return c.p;
  }
};

// what a workgroup accumulates in registers over its slice of patches / units
struct BwdSums {
  // conv2 weight-gradient tiles: M = 32 co (2 tiles) x N = 13 tiles of (2 taps x 8 ci) = 26 tiles;
  // wave w owns tile w (and tile w + 16 for w < 10): tile t -> (co tile t & 1, N tile t >> 1)
  f32x4 wacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  float db2 = 0.f, db1 = 0.f, dw1[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
};

// once per workgroup: the backward weights -> LDS, and the padded gradient planes zeroed (their halo stays zero)
template <int SPLIT>
__device__ __forceinline__ void stage_bwd_constants(const BwdLds &B, const FrontBwdArgs &a, int tid) {
  for (int e = tid; e < 25 * 8 * 32 / 8; e += NTH) {
    // global [tap][8 ci][4 chunks of 8 co] -> LDS [tap][co half][8 ci][2 chunks]
    const int ch = e & 3, ci = (e >> 2) & 7, tap = e >> 5;
    const int d = ((tap * 2 + (ch >> 1)) * 8 + ci) * 2 + (ch & 1);
    reinterpret_cast<uint4 *>(B.wbh)[d] = reinterpret_cast<const uint4 *>(a.w2bh)[e];
    if (SPLIT == 3) reinterpret_cast<uint4 *>(B.wbl)[d] = reinterpret_cast<const uint4 *>(a.w2bl)[e];
  }
  for (int e = tid; e < 2 * D2HALF / 4; e += NTH) {
    reinterpret_cast<uint32_t *>(B.d2h)[e] = 0;
    reinterpret_cast<uint32_t *>(B.d2l)[e] = 0;
  }
}

// ---- pool2 + ReLU2 backward: dC2[pix][co] (masked) -> padded bf16 planes, bias gradient.  gsum_at(y, x, co): the gradient
// reaching conv2 output (y, x, co), from the recomputed values (pool_bwd_pixel) or from the saved codes (pool_bwd_code) ----
template <int SPLIT, class G>
__device__ __forceinline__ void pool2_bwd(const BwdLds &B, int tid, float &db2, G gsum_at) {
  for (int e = tid; e < C2N * 32; e += NTH) {
    const int co = e & 31, pix = e >> 5, y = pix / C2W, x = pix % C2W;
    const float gsum = gsum_at(y, x, co);
    db2 += gsum;  // thread t always meets channel t & 31
    const uint16_t h = f2bf(gsum);
    const int o = (co >> 4) * D2HALF + ((y + 4) * D2PW + x + 4) * 32 + 2 * (co & 15);
    *reinterpret_cast<uint16_t *>(B.d2h + o) = h;
    if (SPLIT == 3) *reinterpret_cast<uint16_t *>(B.d2l + o) = bf_lo(gsum, h);
  }
}

// ---- conv2 weight gradient: dW2[co][ci][tap] += sum_pix dC2[pix][co] * a1pad[pix + tap][ci] (MFMA, transposed LDS reads).
// d2h / d2l / a1h / a1l: LDS byte addresses of the gradient and pool1 planes ----
template <int SPLIT>
__device__ __forceinline__ void conv2_wgrad(f32x4 (&wacc)[2], uint32_t d2h_a, uint32_t d2l_a, uint32_t a1h_a, uint32_t a1l_a,
                                            int tid) {
  const int lane = tid & 63, wave = tid >> 6, g = lane >> 4;
  const int t16 = lane & 15, q = t16 >> 2, pq = t16 & 3;
#pragma unroll 1
  for (int ks = 0; ks < 4; ++ks) {  // 121 pixels in 4 k-steps of 32 (rows >= 121 hit a zero halo pixel of dC2)
    const int i_lo = 32 * ks + 8 * g + q, i_hi = i_lo + 4;
    const bool v_lo = i_lo < C2N, v_hi = i_hi < C2N;
    const int y_lo = v_lo ? i_lo / C2W : 0, x_lo = v_lo ? i_lo % C2W : 0;
    const int y_hi = v_hi ? i_hi / C2W : 0, x_hi = v_hi ? i_hi % C2W : 0;
    // A: dC2^T, rows = pixels (padded plane index, or halo pixel 0 for dummy rows), 16 co per tile
    const uint32_t ya_lo = (v_lo ? ((y_lo + 4) * D2PW + x_lo + 4) : 0) * 32 + 8 * (pq & 1) + 16 * (pq >> 1);
    const uint32_t ya_hi = (v_hi ? ((y_hi + 4) * D2PW + x_hi + 4) : 0) * 32 + 8 * (pq & 1) + 16 * (pq >> 1);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int tile = wave + NWV * u;
      if (tile < 26) {  // wave-uniform
        const int i = tile & 1, nt = tile >> 1;
        int tap = 2 * nt + (pq >> 1);
        if (tap > 24) tap = 24;  // the 26th tap does not exist: recompute tap 24, dropped at the end
        const int toff = (tap / 5) * A1PW + (tap % 5);
        // B: a1 padded plane [pix][8 ci] (16 B rows): fragment columns 0-7 = tap 2nt, 8-15 = tap 2nt+1
        const uint32_t xa_lo = ((y_lo * A1PW + x_lo) + toff) * 16 + 8 * (pq & 1);
        const uint32_t xa_hi = ((y_hi * A1PW + x_hi) + toff) * 16 + 8 * (pq & 1);
        const bf8 ah = tr_frag(d2h_a + ya_lo + D2HALF * i, d2h_a + ya_hi + D2HALF * i);
        const bf8 bh = tr_frag(a1h_a + xa_lo, a1h_a + xa_hi);
        bf8 al, bl;
        if (SPLIT == 3) {
          al = tr_frag(d2l_a + ya_lo + D2HALF * i, d2l_a + ya_hi + D2HALF * i);
          bl = tr_frag(a1l_a + xa_lo, a1l_a + xa_hi);
        }
        lds_reads_landed();
        if (SPLIT == 3) {
          wacc[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, wacc[u], 0, 0, 0);
          wacc[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, wacc[u], 0, 0, 0);
        }
        wacc[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, wacc[u], 0, 0, 0);
      }
    }
  }
}

// ---- conv2 backward-data: dA1[ya][xa][ci] = sum_{tap,co} dC2[ya - ty + 1][xa - tx + 1][co] W2[co][ci][tap] (MFMA) ----
// One image row of dA1 per wave, dealt to the 16 MFMA rows by LDS bank residue: a ds_read_b128 is served in 16-lane groups
// made of tile rows {0-3, 12-15} and {4-11}, conflict-free on these 32-byte pixel rows iff the pixel positions inside each set
// are distinct mod 8 -- rows 4-11 take x = 0..7, rows 0-3 and 12.. take x = 8.. up to the row's last pixel, which the
// remaining rows repeat (same address: broadcast).  Sixteen consecutive pixels of the 13-wide map (11 tiles) broke that at
// every row end; 13 tiles cost nothing, 5 of the 16 waves were idle in this phase.
template <int LAST>  // last pixel of the row (12 on a 16x16 patch, 14 in a tile's a1 window)
__device__ __forceinline__ int dealt_x(int row) {
  return (row >= 4 && row < 12) ? row - 4 : (row < 4 ? 8 + row : min(row, LAST));
}
// -> the four values of this lane (rows 4g..4g+3 of the wave's tile -> x = dealt_x(row), channel r16; lanes r16 < 8 are the
// ones to store).  base: padded dC2 pixel under tap (0,0) of this lane's dA1 pixel (MFMA row r16).
template <int SPLIT>
__device__ __forceinline__ f32x4 conv2_bwd_data(const BwdLds &B, int base, int g, int r16) {
  // Only 8 of the 16 MFMA output columns are real (8 input channels), so for bf16x3 the idle columns carry
  // a correction term: B columns 0-7 = Wh, 8-15 = Wl (lanes r16 >= 8 simply read the lo plane), hence
  //   ah x [Wh | Wl] -> columns 0-7 = ah*Wh, 8-15 = ah*Wl        al x [Wh | ..] -> columns 0-7 = al*Wh
  // two MFMAs and three LDS reads per tap instead of three and four; the halves meet in a lane shift.
  f32x4 dacc = f32x4{0.f, 0.f, 0.f, 0.f}, dacc1 = dacc;
  // B: backward weights, LDS layout [tap][co half][8 ci][16 co]: lane (ci = r16 & 7, k chunk g = co 8g..8g+7)
  // (copies: a choice between two fields of the layout struct, as an lvalue, would keep the whole struct in scratch)
  const char *const wbh = B.wbh, *const wbl = B.wbl;
  const char *wb = ((SPLIT == 3 && r16 >= 8) ? wbl : wbh) + (g >> 1) * 256 + (r16 & 7) * 32 + (g & 1) * 16;
  // taps shift the A pixel by -(ty*19 + tx); rebased so that every tap is a non-negative immediate
  const char *ab = B.d2h + (g >> 1) * D2HALF + (base - (4 * D2PW + 4)) * 32 + (g & 1) * 16;
  const long lo_a = B.d2l - B.d2h;
#pragma unroll
  for (int tap = 0; tap < 25; ++tap) {
    const int arel = ((4 - tap / 5) * D2PW + (4 - tap % 5)) * 32;
    const bf8 b = *reinterpret_cast<const bf8 *>(wb + tap * 512);
    const bf8 ah = *reinterpret_cast<const bf8 *>(ab + arel);
    if (SPLIT == 3) {
      const bf8 al = *reinterpret_cast<const bf8 *>(ab + lo_a + arel);
      dacc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, b, dacc1, 0, 0, 0);
    }
    dacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, b, dacc, 0, 0, 0);
  }
  if (SPLIT == 3) {
#pragma unroll
    for (int r = 0; r < 4; ++r) dacc[r] += __shfl_down(dacc[r], 8, 64) + dacc1[r];
  }
  return dacc;
}
// the 16x16 kernels' form of it: 13 waves, one 13-pixel row each -> dA1 [169][8], which aliases dyb
template <int SPLIT>
__device__ __forceinline__ void conv2_bwd_data_patch(const BwdLds &B, float *dA1, int tid) {
  const int lane = tid & 63, wave = tid >> 6, g = lane >> 4, r16 = lane & 15;
  f32x4 dacc = f32x4{0.f, 0.f, 0.f, 0.f};
  if (wave < A1W)  // wave-uniform; tap (0,0) of dA1 pixel (wave, x) is padded dC2 pixel (wave + 5, x + 5)
    dacc = conv2_bwd_data<SPLIT>(B, (wave + 5) * D2PW + dealt_x<A1W - 1>(r16) + 5, g, r16);
  lds_barrier();  // dyb (aliased by dA1) is no longer read
  if (wave < A1W && r16 < 8)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * g + r;  // rows 13-15 only repeated pixel 12
      if (row < A1W) dA1[(wave * A1W + dealt_x<A1W - 1>(row)) * 8 + r16] = dacc[r];
    }
}

// ---- conv1 weight gradient (VALU) over a CW x CW map of dC1 [8][CW*CW] and XW-wide input rows: thread = (co, ci, tap row ty,
// pixel-row part), nrp = CW / cin parts (560 threads on a 16x16 patch, 640 on a tile, for either cin).  It reads CH values of a
// dC1 row and the CH + 4 input values under them once and forms the 5 taps of that row from registers (32 LDS reads per 70
// FMAs at CH = 14; one output per thread needed 2 reads per FMA and was LDS-bound).  Lanes differ in y: the row strides are
// conflict-free.  CH = CW takes a pixel row at once; the tile kernel takes two halves, 8 + 12 values live at a time instead
// of 16 + 20 (the whole row put it 84 bytes per lane into scratch at its 128-register cap).  The row sums of an output meet in
// write_partials ----
template <int CW, int XW, int CH>
__device__ __forceinline__ void conv1_wgrad(const float *dC1, const float *xs, int cin, int nrp, int tid, float (&dw1)[5]) {
  static_assert(CW % CH == 0, "whole chunks");
  if (tid < 8 * cin * 5 * nrp) {
    const int rp = tid % nrp, q = tid / nrp, ty = q % 5, ci = (q / 5) % cin, co = q / (5 * cin);
    for (int y = rp; y < CW; y += nrp) {
      const float *dr = dC1 + co * CW * CW + y * CW, *xr = xs + (ci * XW + y + ty) * XW;
#pragma unroll 1
      for (int h = 0; h < CW; h += CH) {
        float dv[CH], xv[CH + 4];
#pragma unroll
        for (int x = 0; x < CH; ++x) dv[x] = dr[h + x];
#pragma unroll
        for (int x = 0; x < CH + 4; ++x) xv[x] = xr[h + x];
#pragma unroll
        for (int tx = 0; tx < 5; ++tx) {
          float s1 = 0.f;
#pragma unroll
          for (int x = 0; x < CH; ++x) s1 = fmaf(dv[x], xv[x + tx], s1);
          dw1[tx] += s1;
        }
      }
    }
  }
}

// ---- partial sums of this workgroup's slice -> workspace [dW2 [32][8][25] | db2 [32] | dW1 [8][cin][25] | db1 [8]];
// red: LDS scratch (the start of the workgroup's LDS: nothing there is live any more) ----
__device__ __forceinline__ void write_partials(const BwdSums &S, float *part, float *red, int cin, int nrp, int tid) {
  const int lane = tid & 63, wave = tid >> 6, g = lane >> 4, r16 = lane & 15;
  const int nout = 8 * cin * 25, nrowthr = 8 * cin * 5 * nrp;
  float *out = part + (long)blockIdx.x * (32 * 8 * 25 + 32 + nout + 8);
  // wacc[u][r] of tile t = wave + 16 u: dW2[co = 16 (t & 1) + 4 g + r][ci = r16 & 7][tap = 2 (t >> 1) + (r16 >> 3)]
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int tile = wave + NWV * u;
    const int tap = 2 * (tile >> 1) + (r16 >> 3);
    if (tile < 26 && tap < 25)
#pragma unroll
      for (int r = 0; r < 4; ++r) out[((16 * (tile & 1) + 4 * g + r) * 8 + (r16 & 7)) * 25 + tap] = S.wacc[u][r];
  }
  // db2: thread t summed channel t & 31 over its pixel subset -> reduce the 32 threads per channel through LDS
  __syncthreads();
  red[tid] = S.db2;
  __syncthreads();
  if (tid < 32) {
    float s = 0.f;
    for (int k = 0; k < NTH / 32; ++k) s += red[tid + 32 * k];
    out[32 * 8 * 25 + tid] = s;
  }
  __syncthreads();
  if (tid < nrowthr)
#pragma unroll
    for (int tx = 0; tx < 5; ++tx) red[tid * 5 + tx] = S.dw1[tx];  // [(co, ci, ty)][row part][tx]
  __syncthreads();
  if (tid < nout) {  // output o = ((co * cin + ci) * 5 + ty) * 5 + tx: add its row parts in a fixed order
    const int q = tid / 5, tx = tid % 5;
    float s = 0.f;
    for (int y = 0; y < nrp; ++y) s += red[(q * nrp + y) * 5 + tx];
    out[32 * 8 * 25 + 32 + tid] = s;
  }
  __syncthreads();
  red[tid] = S.db1;
  __syncthreads();
  if (tid < 8) {
    float s = 0.f;
    for (int k = 0; k < NTH / 8; ++k) s += red[tid + 8 * k];
    out[32 * 8 * 25 + 32 + nout + tid] = s;
  }
}

// ---- backward with recomputation (tests, CRW_FRONT_RECOMPUTE=1, the phase stamps) ---------------------------------------
template <int SPLIT>
__global__ __launch_bounds__(NTH) void front_bwd_kernel(FrontBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int cin = a.f.cin;
  RecomputeLds lay;
  lay.carve(lds, cin, XPW, C1W);
  const FwdLds &L = lay.F;
  const BwdLds &B = lay.B;
  float *dA1 = B.dyb, *dC1 = B.dyb + A1W * A1W * 8;  // dA1 [169][8] + dC1 [8][196] once dy is consumed
  static_assert(A1W * A1W * 8 + C1N * 8 <= ON * 32, "alias");

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15;
  zero_patch_borders(L.xs, L.a1h, L.a1l, cin, tid);
  stage_weights<SPLIT>(L, a.f, tid);
  stage_bwd_constants<SPLIT>(B, a, tid);
  __syncthreads();

  BwdSums S;
  const int nrp = C1W / cin;  // conv1 weight gradient: row parts of cin pixel rows each
  const uint32_t d2h_a = lds_addr_of(B.d2h), d2l_a = lds_addr_of(B.d2l), a1h_a = lds_addr_of(L.a1h), a1l_a = lds_addr_of(L.a1l);

  const int p_begin = blockIdx.x * a.patches_per_block;
  const int p_end = min(a.f.P, p_begin + a.patches_per_block);
#ifdef CRW_CONV_STAMPS
  long long phase_[NPHASE] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, prev_ = (long long)__builtin_amdgcn_s_memtime();
#endif
  const float b2r = a.f.b2[16 * (wave & 1) + r16];  // read once: the barriers in the loop are memory clobbers
  // x (cin*256 floats) and dy (3200 floats) of the NEXT patch are fetched into registers while the current
  // one is processed, so no phase waits on HBM
  constexpr int DYIT = (ON * 32 / 4 + NTH - 1) / NTH;  // float4 chunks of dy per thread (800 chunks)
  float4 dy_r[DYIT];
  float x_r = 0.f;                                      // cin*256 <= 512 floats: threads < cin*256 hold one each
  // buffer loads: base in a scalar resource descriptor, a 32-bit per-lane offset and a scalar per-patch offset --
  // no 64-bit per-lane pointers live across the patch loop (they were being spilled and reloaded every
  // iteration with a full vmcnt(0) wait); reads past the end of the tensors return 0
  const __amdgpu_buffer_rsrc_t dy_rs =
      __builtin_amdgcn_make_buffer_rsrc((void *)a.dy, 0, (int)((long)a.f.P * ON * 32 * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t x_rs =
      __builtin_amdgcn_make_buffer_rsrc((void *)a.f.x, 0, (int)((long)a.f.P * cin * 256 * 4), 0x00020000);
  auto fetch = [&](int pt) {
#pragma unroll
    for (int i = 0; i < DYIT; ++i)
      dy_r[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(dy_rs, (tid + i * NTH) * 16, pt * (ON * 32 * 4), 0));
    x_r = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(x_rs, tid * 4, pt * (cin * 256 * 4), 0));
  };
  if (p_begin < p_end) fetch(p_begin);
  for (int pt = p_begin; pt < p_end; ++pt) {
    // ---- recompute the forward of this patch ---------------------------------------------------
    if (tid < cin * 256) L.xs[((tid >> 8) * XPW + ((tid >> 4) & 15) + 1) * XPW + (tid & 15) + 1] = x_r;
#pragma unroll
    for (int i = 0; i < DYIT; ++i)
      if (tid + i * NTH < ON * 32 / 4) reinterpret_cast<float4 *>(B.dyb)[tid + i * NTH] = dy_r[i];
    if (pt + 1 < p_end) fetch(pt + 1);
    lds_barrier();
    FRONT_STAMP(0)
    conv1_relu<XPW, C1W, true>(L, cin, tid);
    lds_barrier();
    FRONT_STAMP(1)
    pool1<SPLIT, true>(L, tid);
    lds_barrier();
    FRONT_STAMP(2)
    conv2_relu<SPLIT, true>(L, b2r, tid);
    lds_barrier();
    FRONT_STAMP(3)

    pool2_bwd<SPLIT>(B, tid, S.db2, [&](int y, int x, int co) { return pool_bwd_pixel<C2W, 32>(L.c2r, B.dyb, y, x, co); });
    lds_barrier();
    FRONT_STAMP(4)
    conv2_wgrad<SPLIT>(S.wacc, d2h_a, d2l_a, a1h_a, a1l_a, tid);
    FRONT_STAMP(5)
    conv2_bwd_data_patch<SPLIT>(B, dA1, tid);
    lds_barrier();
    FRONT_STAMP(6)

    // ---- pool1 + ReLU1 backward -> dC1 [8][196] ----
    for (int e = tid; e < C1N * 8; e += NTH) {
      const int co = e & 7, pix = e >> 3, y = pix / C1W, x = pix % C1W;
      const float gsum = pool_bwd_pixel<C1W, 8>(L.c1r, dA1, y, x, co);
      dC1[co * C1N + pix] = gsum;  // channel-major: the weight-gradient threads read whole pixel rows
      S.db1 += gsum;               // thread t always meets channel t & 7
    }
    lds_barrier();
    FRONT_STAMP(7)
    conv1_wgrad<C1W, XPW, C1W>(dC1, L.xs, cin, nrp, tid, S.dw1);
    lds_barrier();  // next patch may overwrite xs / dyb
    FRONT_STAMP(8)
  }
#ifdef CRW_CONV_STAMPS
  if (a.stamps && tid == 0)
    for (int k = 0; k < NPHASE; ++k) a.stamps[(long)blockIdx.x * NPHASE + k] = phase_[k];
#endif
  write_partials(S, a.part, reinterpret_cast<float *>(lds), cin, nrp, tid);
}

// ---- backward on patches of any size (training at patch sizes other than 16x16) -----------------------------------------
// The unit of work is (patch, 10x10 tile of the pool2 output map), with the geometry of front_fwd_map_kernel (see pool1_window;
// an a1 position outside the a1 map passes no gradient).  Every gradient is linear in dy and every pooled output belongs to
// exactly one tile, so the per-tile contributions to dW1 / dW2 / db simply add up (overlapping windows recompute the same
// forward values, hence the same ReLU gates and arg-max choices).  The forward of a tile is the code of front_fwd_map_kernel
// on bordered maps; pool2 backward, the conv2 weight gradient, conv2 backward-data's tap loop, the conv1 weight gradient and the
// partial sums are the code of front_bwd_kernel.  Its own: loading a window and a tile of dy, the masked 15-pixel row store of
// conv2 backward-data, and the pool1 backward at the extents 16 / 15 instead of 14 / 13.
constexpr int TXW = MXW, TCW = MC1W, TCN = TCW * TCW, TAW = A1PW;  // 20, 16, 256, 15

template <int SPLIT>
__global__ __launch_bounds__(NTH) void front_bwd_tile_kernel(FrontBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int cin = a.f.cin;
  RecomputeLds lay;
  lay.carve(lds, cin, TXW, TCW);
  const FwdLds &L = lay.F;
  const BwdLds &B = lay.B;
  // dA1 [225][8] aliases dyb and dC1 [8][256] aliases c2r: both are dead after the pool2 backward phase (157 KB of LDS in all)
  float *dA1 = B.dyb, *dC1 = L.c2r;
  static_assert(TAW * TAW * 8 <= ON * 32 && TCN * 8 <= (C2W + 2) * (C2W + 2) * 32, "aliases");

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, r16 = lane & 15;
  stage_weights<SPLIT>(L, a.f, tid);
  stage_bwd_constants<SPLIT>(B, a, tid);
  __syncthreads();

  BwdSums S;
  const int nrp = TCW / cin;
  const uint32_t d2h_a = lds_addr_of(B.d2h), d2l_a = lds_addr_of(B.d2l), a1h_a = lds_addr_of(L.a1h), a1l_a = lds_addr_of(L.a1l);
  const int H = a.H, W = a.W, Ho = H - 6, Wo = W - 6, ntile = a.tiles_x * a.tiles_y;
  const int u_begin = blockIdx.x * a.patches_per_block;
  const int u_end = min(a.f.P * ntile, u_begin + a.patches_per_block);
  const float b2r = a.f.b2[16 * (wave & 1) + r16];

  for (int u = u_begin; u < u_end; ++u) {
    const int pt = u / ntile, tile = u % ntile;
    const int oy0 = (tile / a.tiles_x) * OW, ox0 = (tile % a.tiles_x) * OW;
    // ---- window of the patch and the tile of dy (zeros outside the patch / the map) ---------------------------
    for (int e = tid; e < cin * TXW * TXW; e += NTH) {
      const int ci = e / (TXW * TXW), r = (e / TXW) % TXW, c = e % TXW;
      const int iy = oy0 + r - 2, ix = ox0 + c - 2;
      const bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
      const float v = a.f.x[(((long)pt * cin + ci) * H + min(max(iy, 0), H - 1)) * W + min(max(ix, 0), W - 1)];
      L.xs[e] = ok ? v : 0.f;
    }
    for (int e = tid; e < ON * 32 / 4; e += NTH) {
      const int q = e >> 3, c4 = e & 7, y = q / OW, x = q % OW;
      const bool ok = oy0 + y < Ho && ox0 + x < Wo;
      const float4 v = *reinterpret_cast<const float4 *>(a.dy + (((long)pt * Ho + min(oy0 + y, Ho - 1)) * Wo + min(ox0 + x, Wo - 1)) * 32 + 4 * c4);
      reinterpret_cast<float4 *>(B.dyb)[e] = ok ? v : float4{0.f, 0.f, 0.f, 0.f};
    }
    lds_barrier();
    // ---- recompute the forward of this tile -------------------------------------------------------------------
    conv1_relu<TXW, TCW, true>(L, cin, tid);
    lds_barrier();
    pool1_window<SPLIT, true>(L, tid, oy0, ox0, H, W);
    lds_barrier();
    conv2_relu<SPLIT, true>(L, b2r, tid);
    lds_barrier();

    pool2_bwd<SPLIT>(B, tid, S.db2, [&](int y, int x, int co) { return pool_bwd_pixel<C2W, 32>(L.c2r, B.dyb, y, x, co); });
    lds_barrier();
    conv2_wgrad<SPLIT>(S.wacc, d2h_a, d2l_a, a1h_a, a1l_a, tid);
    // ---- conv2 backward-data: one row of the 15x15 a1 window per wave (15 waves), masked where the window leaves the a1 map;
    // a1 window position (wave, x) is the padded dC2 pixel (wave + 4, x + 4) under tap (0,0) ----
    if (wave < TAW) {
      const f32x4 dacc = conv2_bwd_data<SPLIT>(B, (wave + 4) * D2PW + dealt_x<TAW - 1>(r16) + 4, g, r16);
      if (r16 < 8) {
        // (opaque to the compiler: it would hoist the four rows' positions and LDS addresses out of the unit loop and, at the
        // 128-register cap of a 1024-thread workgroup, park them in scratch -- reloaded with an exposed latency each)
        int gq = g;
        asm volatile("" : "+v"(gq));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 4 * gq + r;
          const int x = dealt_x<TAW - 1>(row);
          const int ay = oy0 + wave - 1, ax = ox0 + x - 1;
          const bool ok = ay >= 0 && ay < H - 3 && ax >= 0 && ax < W - 3;
          if (row < TAW) dA1[(wave * TAW + x) * 8 + r16] = ok ? dacc[r] : 0.f;
        }
      }
    }
    lds_barrier();

    // ---- pool1 + ReLU1 backward -> dC1 [8][256] ---------------------------------------------------------------
    for (int e = tid; e < TCN * 8; e += NTH) {
      const int co = e & 7, pix = e >> 3, y = pix / TCW, x = pix % TCW;
      const float gsum = pool_bwd_pixel<TCW, 8>(L.c1r, dA1, y, x, co);
      dC1[co * TCN + pix] = gsum;
      S.db1 += gsum;
    }
    lds_barrier();
    conv1_wgrad<TCW, TXW, TCW / 2>(dC1, L.xs, cin, nrp, tid, S.dw1);
    lds_barrier();  // the next unit overwrites xs / dyb
  }
  write_partials(S, a.part, reinterpret_cast<float *>(lds), cin, nrp, tid);
}

// ---- backward without recomputation -------------------------------------------------------------------------------
// The same gradients from what the forward pass saved (pool1 planes + pooling codes, FrontArgs::saved): no conv1 / pool1 /
// conv2 recomputation (7.5 k of the 29 k cycles per patch of front_bwd_kernel) and the two pooling backward passes read
// one code byte per window instead of the window's values (pool_bwd_code).
// Phases per patch: registers -> LDS | pool2 backward | conv2 weight gradient + backward-data | pool1 backward | conv1
// weight gradient.  x, dy and the saved record of the NEXT patch are fetched into registers while this one is processed.
template <int SPLIT>
__global__ __launch_bounds__(NTH) void front_bwd_saved_kernel(FrontBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int cin = a.f.cin;
  SavedLds L;
  L.carve(lds, cin);
  const BwdLds &B = L.B;
  float *dA1 = B.dyb, *dC1 = B.dyb + A1W * A1W * 8;

  const int tid = threadIdx.x;
  zero_patch_borders(L.xs, L.a1h, L.a1l, cin, tid);
  stage_bwd_constants<SPLIT>(B, a, tid);
  __syncthreads();

  BwdSums S;
  const int nrp = C1W / cin;
  const uint32_t d2h_a = lds_addr_of(B.d2h), d2l_a = lds_addr_of(B.d2l), a1h_a = lds_addr_of(L.a1h), a1l_a = lds_addr_of(L.a1l);
  const int p_begin = blockIdx.x * a.patches_per_block;
  const int p_end = min(a.f.P, p_begin + a.patches_per_block);

  // prefetch registers: dy (one float4), x (one float), and one 16-byte chunk of the saved record per thread:
  // chunks 0..337 = a1 hi / lo planes, 338..537 = k2 codes, 538..622 = k1 codes
  constexpr int NA1 = 2 * SV_A1 / 16, NK2 = SV_K2 / 16, NK1 = SV_K1 / 16, NSV = NA1 + NK2 + NK1;
  static_assert(NSV <= NTH && ON * 32 / 4 <= NTH, "one chunk per thread");
  float4 dy_r;
  float x_r = 0.f;
  u4v sv_r;
  const __amdgpu_buffer_rsrc_t dy_rs = __builtin_amdgcn_make_buffer_rsrc((void *)a.dy, 0, (int)((long)a.f.P * ON * 32 * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t x_rs = __builtin_amdgcn_make_buffer_rsrc((void *)a.f.x, 0, (int)((long)a.f.P * cin * 256 * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t sv_rs = __builtin_amdgcn_make_buffer_rsrc((void *)a.f.saved, 0, (int)((long)a.f.P * SV_BYTES), 0x00020000);
  auto fetch = [&](int pt) {
    dy_r = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(dy_rs, tid * 16, pt * (ON * 32 * 4), 0));
    x_r = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(x_rs, tid * 4, pt * (cin * 256 * 4), 0));
    sv_r = __builtin_amdgcn_raw_buffer_load_b128(sv_rs, min(tid, NSV - 1) * 16, pt * SV_BYTES, 0);
  };
  if (p_begin < p_end) fetch(p_begin);
  for (int pt = p_begin; pt < p_end; ++pt) {
    // ---- registers -> LDS ----------------------------------------------------------------------
    if (tid < cin * 256) L.xs[((tid >> 8) * XPW + ((tid >> 4) & 15) + 1) * XPW + (tid & 15) + 1] = x_r;
    if (tid < ON * 32 / 4) reinterpret_cast<float4 *>(B.dyb)[tid] = dy_r;
    if (tid < NA1) {  // a1 plane chunk: pixel (tid % 169) of plane (tid / 169) -> interior of the padded 15x15 image
      const int pl = tid / (A1W * A1W), px = tid % (A1W * A1W);
      *reinterpret_cast<u4v *>((pl ? L.a1l : L.a1h) + ((px / A1W + 1) * A1PW + px % A1W + 1) * 16) = sv_r;
    } else if (tid < NA1 + NK2) {
      reinterpret_cast<u4v *>(L.k2s)[tid - NA1] = sv_r;
    } else if (tid < NSV) {
      reinterpret_cast<u4v *>(L.k1s)[tid - NA1 - NK2] = sv_r;
    }
    if (pt + 1 < p_end) fetch(pt + 1);
    lds_barrier();

    pool2_bwd<SPLIT>(B, tid, S.db2, [&](int y, int x, int co) { return pool_bwd_code<OW, 32>(L.k2s, B.dyb, y, x, co); });
    lds_barrier();
    conv2_wgrad<SPLIT>(S.wacc, d2h_a, d2l_a, a1h_a, a1l_a, tid);
    conv2_bwd_data_patch<SPLIT>(B, dA1, tid);
    lds_barrier();

    // ---- pool1 + ReLU1 backward from the codes -> dC1 [8][196] ----------------------------------------
    for (int e = tid; e < C1N * 8; e += NTH) {
      const int co = e & 7, pix = e >> 3, y = pix / C1W, x = pix % C1W;
      const float gsum = pool_bwd_code<A1W, 8>(L.k1s, dA1, y, x, co);
      dC1[co * C1N + pix] = gsum;
      S.db1 += gsum;
    }
    lds_barrier();
    conv1_wgrad<C1W, XPW, C1W>(dC1, L.xs, cin, nrp, tid, S.dw1);
    lds_barrier();
  }
  write_partials(S, a.part, reinterpret_cast<float *>(lds), cin, nrp, tid);
}

// out[e] = sum_k part[k * stride + e], e < n: one wave per output, lanes stride the slices, fixed
// shuffle tree (deterministic)
// (the four gradient tensors are consecutive segments of a slice's partial vector: one launch covers them all)
struct FrontSums {
  const float *part;
  int nslice, stride, n;
  int end[4];     // exclusive end of segment i in the partial vector
  float *dst[4];  // its output tensor
};
__global__ __launch_bounds__(256) void front_slice_sum_kernel(FrontSums a) {
  const int e = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (e >= a.n) return;
  float s = 0.f;
  for (int k = lane; k < a.nslice; k += 64) s += a.part[(long)k * a.stride + e];
  s = wave_sum(s);
  if (lane == 0) {
    const int seg = e < a.end[0] ? 0 : e < a.end[1] ? 1 : e < a.end[2] ? 2 : 3;
    a.dst[seg][e - (seg ? a.end[seg - 1] : 0)] = s;
  }
}

int front_slices(int P) { return P < 256 ? P : 256; }  // one 144 KB workgroup per CU

// threads per workgroup of the forward kernels: 512 (two workgroups per CU), CRW_FRONT_NT=1024 for the one-workgroup form
int front_fwd_threads() {
  static const int nt = [] { const char *e = getenv("CRW_FRONT_NT"); return e && atoi(e) == 1024 ? 1024 : 512; }();
  return nt;
}

// Launch a forward kernel given as its four instantiations {<1, 512>, <3, 512>, <1, 1024>, <3, 1024>}: up to 512 workgroups (two
// per CU at 512 threads), the dynamic-LDS limit raised once per instantiation where the layout needs more than 64 KB.
template <class Args>
int launch_front_fwd(void (*const (&kernels)[4])(Args), int split, const Args &a, long nwork, size_t lds, hipStream_t s) {
  static bool attr[4] = {false, false, false, false};
  const int nt = front_fwd_threads(), which = (nt == 1024 ? 2 : 0) + (split == 3 ? 1 : 0);
  if (!attr[which] && lds > 64 * 1024) {
    if (hipFuncSetAttribute((const void *)kernels[which], hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return CRW_EHIP;
    attr[which] = true;
  }
  if (nt == 1024) CRW_ROUTE("front.fwd_nt1024");  // (patch and map forms alike)
  else CRW_ROUTE("front.fwd_nt512");
  hipLaunchKernelGGL(kernels[which], dim3(nwork < 512 ? (int)nwork : 512), dim3(nt), lds, s, a);
  return check_launch();
}

// Launch a backward kernel (K1 / K3: its plain-bf16 / hi-lo instantiation) on a.part's `nslice` slices, then add the slices'
// partial vectors [dW2 | db2 | dW1 | db1] into the four output tensors in a fixed order.
template <void (*K1)(FrontBwdArgs), void (*K3)(FrontBwdArgs)>
int launch_front_bwd(int split, const FrontBwdArgs &a, int nslice, size_t lds, float *dw1, float *db1, float *dw2, float *db2,
                     hipStream_t s) {
  static bool attr[2] = {false, false};  // dynamic-LDS limit raised, per instantiation (this function exists once per kernel)
  void (*const kernel)(FrontBwdArgs) = split == 3 ? K3 : K1;
  if (!attr[split == 3]) {
    if (hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
      return CRW_EHIP;
    attr[split == 3] = true;
  }
  hipLaunchKernelGGL(kernel, dim3(nslice), dim3(NTH), lds, s, a);
  CRW_TRY(check_launch());
  const int n2 = 32 * 8 * 25, n1 = 8 * a.f.cin * 25, PART = n2 + 32 + n1 + 8;
  FrontSums fs{a.part, nslice, PART, PART, {n2, n2 + 32, n2 + 32 + n1, PART}, {dw2, db2, dw1, db1}};
  hipLaunchKernelGGL(front_slice_sum_kernel, dim3((fs.n + 3) / 4), dim3(256), 0, s, fs);
  return check_launch();
}

}  // namespace
}  // namespace crw

using namespace crw;

long long *g_front_stamps = nullptr;  // diagnostics (make STAMPS=1)

extern "C" {

#ifdef CRW_CONV_STAMPS
void crw_debug_front_stamps(long long *buf) { g_front_stamps = buf; }
#endif

// conv2 weight [32][8][5][5] fp32 -> forward planes [7][32][32] and backward planes [25][8][32] (bf16 hi[, lo])
int crw_enc_front_pack(const float *w2, uint16_t *fwd_hi, uint16_t *fwd_lo, uint16_t *bwd_hi, uint16_t *bwd_lo,
                       crw_stream_t stream) {
  clear_stale_error();
  if (!w2 || !fwd_hi || !bwd_hi || (fwd_lo == nullptr) != (bwd_lo == nullptr)) return CRW_EINVAL;
  hipLaunchKernelGGL(pack_w2_kernel, dim3(28), dim3(256), 0, (hipStream_t)stream, w2, fwd_hi, fwd_lo, bwd_hi, bwd_lo);
  return check_launch();
}

size_t crw_enc_front_saved_bytes(int P) { return P < 1 ? 0 : (size_t)P * SV_BYTES; }

int crw_enc_front_fwd(int split, const float *x, int P, int cin, const float *w1, const float *b1,
                      const uint16_t *w2_hi, const uint16_t *w2_lo, const float *b2, uint16_t *y_hi, uint16_t *y_lo,
                      void *saved, crw_stream_t stream) {
  clear_stale_error();
  if (!x || !w1 || !b1 || !w2_hi || !b2 || !y_hi || P < 1 || (cin != 1 && cin != 2) || (split != 1 && split != 3))
    return CRW_EINVAL;
  if (split == 3 && (!w2_lo || !y_lo)) return CRW_EINVAL;
  FrontArgs a{x, w1, b1, w2_hi, w2_lo, b2, y_hi, y_lo, P, cin, static_cast<char *>(saved)};
  static void (*const kernels[4])(FrontArgs) = {front_fwd_kernel<1, 512>, front_fwd_kernel<3, 512>, front_fwd_kernel<1, 1024>,
                                                front_fwd_kernel<3, 1024>};
  return launch_front_fwd(kernels, split, a, P, lds_bytes<FwdLds>(cin, XPW, C1W, C2W), (hipStream_t)stream);  // 60 KB of LDS
}

// front end on patches of any size (h, w >= 7), forward only: x [P][cin][H][W] -> planes [P][(H-6)*(W-6)][32]
int crw_enc_front_fwd_map(int split, const float *x, int P, int cin, int H, int W, const float *w1, const float *b1,
                          const uint16_t *w2_hi, const uint16_t *w2_lo, const float *b2, uint16_t *y_hi, uint16_t *y_lo,
                          crw_stream_t stream) {
  clear_stale_error();
  if (!x || !w1 || !b1 || !w2_hi || !b2 || !y_hi || P < 1 || (cin != 1 && cin != 2) || (split != 1 && split != 3) || H < 7 ||
      W < 7)
    return CRW_EINVAL;
  if (split == 3 && (!w2_lo || !y_lo)) return CRW_EINVAL;
  const int tx = (W - 6 + OW - 1) / OW, ty = (H - 6 + OW - 1) / OW;
  FrontMapArgs a{{x, w1, b1, w2_hi, w2_lo, b2, y_hi, y_lo, P, cin}, H, W, tx, ty};
  static void (*const kernels[4])(FrontMapArgs) = {front_fwd_map_kernel<1, 512>, front_fwd_map_kernel<3, 512>,
                                                   front_fwd_map_kernel<1, 1024>, front_fwd_map_kernel<3, 1024>};
  return launch_front_fwd(kernels, split, a, (long)P * tx * ty, lds_bytes<FwdLds>(cin, MXW, MC1W, C2W), (hipStream_t)stream);
}

size_t crw_enc_front_ws_bytes(int P, int cin) {
  if (P < 1 || (cin != 1 && cin != 2)) return 0;
  return (size_t)front_slices(P) * (32 * 8 * 25 + 32 + 8 * cin * 25 + 8) * sizeof(float);
}

// dy [P][100][32] fp32 -> dw2 [32][8][5][5], db2 [32], dw1 [8][cin][5][5], db1 [8]
int crw_enc_front_bwd(int split, const float *x, int P, int cin, const float *w1, const float *b1,
                      const uint16_t *w2_hi, const uint16_t *w2_lo, const float *b2, const uint16_t *w2b_hi,
                      const uint16_t *w2b_lo, const float *dy, const void *saved, float *dw1, float *db1, float *dw2, float *db2,
                      void *ws, size_t ws_bytes, crw_stream_t stream) {
  clear_stale_error();
  if (!x || !w1 || !b1 || !w2_hi || !b2 || !w2b_hi || !dy || !dw1 || !db1 || !dw2 || !db2 || !ws || P < 1 ||
      (cin != 1 && cin != 2) || (split != 1 && split != 3))
    return CRW_EINVAL;
  if (split == 3 && (!w2_lo || !w2b_lo)) return CRW_EINVAL;
  if (ws_bytes < crw_enc_front_ws_bytes(P, cin)) return CRW_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int nslice = front_slices(P), ppb = (P + nslice - 1) / nslice;
  FrontBwdArgs a{{x, w1, b1, w2_hi, w2_lo, b2, nullptr, nullptr, P, cin, const_cast<char *>(static_cast<const char *>(saved))},
                 w2b_hi, w2b_lo, dy, (float *)ws, ppb, g_front_stamps};
  static const char *force_rc = getenv("CRW_FRONT_RECOMPUTE");  // diagnostics / A-B: ignore the saved record
  if (saved && !(force_rc && force_rc[0] == '1')) {
    CRW_ROUTE("front.bwd_saved");
    return launch_front_bwd<front_bwd_saved_kernel<1>, front_bwd_saved_kernel<3>>(split, a, nslice, lds_bytes<SavedLds>(cin), dw1,
                                                                                  db1, dw2, db2, s);
  }
  CRW_ROUTE("front.bwd_recompute");
  return launch_front_bwd<front_bwd_kernel<1>, front_bwd_kernel<3>>(split, a, nslice, lds_bytes<RecomputeLds>(cin, XPW, C1W), dw1,
                                                                    db1, dw2, db2, s);
}

/* backward of the front end on patches of any size (h, w >= 7): x [P][cin][H][W], dy [P][H-6][W-6][32] fp32 (gradient of the
 * planes crw_enc_front_fwd_map produces) -> dw1, db1, dw2, db2.  ws: crw_enc_front_ws_bytes(P * tiles, cin). */
int crw_enc_front_bwd_map(int split, const float *x, int P, int cin, int H, int W, const float *w1, const float *b1,
                          const uint16_t *w2_hi, const uint16_t *w2_lo, const float *b2, const uint16_t *w2b_hi,
                          const uint16_t *w2b_lo, const float *dy, float *dw1, float *db1, float *dw2, float *db2, void *ws,
                          size_t ws_bytes, crw_stream_t stream) {
  clear_stale_error();
  if (!x || !w1 || !b1 || !w2_hi || !b2 || !w2b_hi || !dy || !dw1 || !db1 || !dw2 || !db2 || !ws || P < 1 ||
      (cin != 1 && cin != 2) || (split != 1 && split != 3) || H < 7 || W < 7)
    return CRW_EINVAL;
  if (split == 3 && (!w2_lo || !w2b_lo)) return CRW_EINVAL;
  const int tx = (W - 6 + OW - 1) / OW, ty = (H - 6 + OW - 1) / OW;
  const long units_l = (long)P * tx * ty;
  if (units_l > 0x7fffffffL) return CRW_EINVAL;
  const int units = (int)units_l;
  if (ws_bytes < crw_enc_front_ws_bytes(units, cin)) return CRW_EWORKSPACE;
  int nslice = front_slices(units);
  const int upb = (units + nslice - 1) / nslice;
  nslice = (units + upb - 1) / upb;
  FrontBwdArgs a{{x, w1, b1, w2_hi, w2_lo, b2, nullptr, nullptr, P, cin, nullptr}, w2b_hi, w2b_lo, dy, (float *)ws, upb, nullptr, H, W, tx, ty};
  CRW_ROUTE("front.bwd_tile");
  return launch_front_bwd<front_bwd_tile_kernel<1>, front_bwd_tile_kernel<3>>(split, a, nslice, lds_bytes<RecomputeLds>(cin, TXW, TCW),
                                                                              dw1, db1, dw2, db2, (hipStream_t)stream);
}

}  // extern "C"
