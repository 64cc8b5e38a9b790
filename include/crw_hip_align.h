/* Aligning a memory bank to its item: segment-centred features and a bias on the long-term keys.  A companion of crw_hip.h and
 * crw_hip_longmem.h (same conventions, same status codes, same CRW_ABI_VERSION).  Added at ABI 8 without a bump: a library built
 * before it still loads, the binding tells by symbol (crw_hip.has_align()).  The binding mirrors this header in
 * crw_hip.ALIGN_SIGNATURES; tests/test_align_host.py holds the two and the library against each other, and tests/test_align_gpu.py
 * runs every entry point over stale memory and between guard bands.
 *
 * CENTRING.  emb [rows, C] is cut into S >= 1 segments of consecutive rows by S + 1 row offsets b_0 = 0 <= b_1 <= ... <= b_S = rows.
 * For a row r of segment s (b_s <= r < b_s+1) and a channel c
 *   mean[s][c] = (sum of emb[r'][c] over the segment's rows, in fp64) / (b_s+1 - b_s)         (fp64)
 *   y[c]       = fp32(emb[r][c] - mean[s][c])                 (the subtraction in fp64: ONE fp32 rounding)
 *   ehat[r][c] = y[c] / max(sqrt(sum_c y[c]^2), 1e-12)        (exactly the arithmetic of crw_normalize on y)
 * so a segment whose means are all 0 gets crw_normalize's bits.  A segment of ONE row is its own mean: y = 0 in every channel and
 * ehat = 0 / 1e-12 = 0, the all-zero row (the convention F.normalize has for a zero vector; +0, but for an entry that is -0 on
 * input).  An empty segment writes nothing (its row of `mean` is +0).
 * The sums are bit-reproducible: per-slab partial sums in fp64 (launch 1), joined in fp64 by every workgroup that needs the mean
 * (launch 2), each in an order that (rows, C) and the offsets fix; no atomics.  The slabs depend on rows alone.
 * Offsets: seg_host (HOST pointer, S + 1 ints, S <= CRW_ALIGN_MAX_BY_VALUE; they travel by value as a kernel argument) is checked:
 * CRW_EINVAL unless 0 = b_0 <= ... <= b_S = rows.  seg_dev (DEVICE pointer, S + 1 ints, S <= CRW_ALIGN_MAX_SEGMENTS) cannot be
 * checked on the host: the kernels read b_0 as 0, b_S as rows and every other b_s as min(rows, max(b_s-1, seg_dev[s])), so no
 * content makes them leave the buffers.  Exactly one of the two is given.
 * ws: crw_center_normalize_ws_bytes(rows, C, S) bytes at any alignment (the partial sums; every byte read is written first).
 * mean (may be NULL): [S, C] fp64, 8-byte aligned.  ehat may be emb (in place: a row is read before it is written, by its own wave,
 * and launch 1 has finished).  CRW_EINVAL for S < 1, rows < 1, C < 1 or C > CRW_ALIGN_MAX_CHANNELS; CRW_EWORKSPACE for a small ws.
 *
 * BIAS.  crw_labelprop_topk_long with long_bias added to the fp32 cosine of every in-band key of the list's long-term part -- list
 * positions below min(n, n_long) * N -- by one rounded fp32 add, after the band mask has decided and before the division by temp:
 * logit = (cos + long_bias) / temp there, cos / temp elsewhere, masked keys stay masked.  Selection, tie rule, softmax and empty
 * slots as there; with raw = 1 the returned logits include the bias.  long_bias == 0 (either sign) IS crw_labelprop_topk_long: the
 * same kernels run and the outputs are its bits.  CRW_EINVAL for a bias that is not finite, and whatever crw_labelprop_topk_long
 * refuses.  Both routes (1 vector, 2 matrix cores) take the bias; the route log names them as it names the unbiased lists'. */
#ifndef CRW_HIP_ALIGN_H
#define CRW_HIP_ALIGN_H

#include "crw_hip_longmem.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CRW_ALIGN_MAX_BY_VALUE 8
#define CRW_ALIGN_MAX_SEGMENTS 1024
#define CRW_ALIGN_MAX_CHANNELS 4096

size_t crw_center_normalize_ws_bytes(int rows, int C, int S);

int crw_center_normalize(const float *emb, int rows, int C, const int32_t *seg_dev, const int32_t *seg_host, int S, void *ws,
                         size_t ws_bytes, float *ehat, double *mean, crw_stream_t stream);

int crw_labelprop_topk_long_bias(const float *ehat, int T, int N, int C, int cxt_size, int n_long, int radius, float temp, int k,
                                 int first_frame, float *WV, int32_t *I, int raw, int route, float long_bias, crw_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
