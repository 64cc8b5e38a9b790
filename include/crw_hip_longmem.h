/* Sliding-context label propagation with a bank of long-term frames: a companion of crw_hip.h (same conventions, same status codes,
 * same CRW_ABI_VERSION).  Added at ABI 8 without a bump: a library built before it still loads, the binding tells by symbol
 * (crw_hip.has_long_memory()).  The binding mirrors this header in crw_hip.LONGMEM_SIGNATURES; tests/test_longmem_host.py holds the
 * two and the library against each other, and tests/test_longmem_gpu.py runs every entry point over stale memory and between guard
 * bands.
 *
 * THE RULE (the 'sliding' reading of the lists only).  A call works on a virtual item of T frames ehat [T, N, C] whose first
 * K = n_long >= 1 frames are long-term: every later frame scores against them, however far the window has moved.  What sits in them
 * is the caller's choice -- labelled traces from elsewhere, then (or not) the item's own seeded frame.  For frame n >= first_frame:
 *   keys ...... frames 0 .. min(n, K) - 1, then frames max(K, n - cxt_size) .. n - 1: nf = min(n, K + cxt_size) frames;
 *   lists ..... the in-band nodes |p - q| < radius of every key frame (long-term frames included) in the order (list position, node);
 *               selection, tie rule, temperature, softmax and empty slots exactly as crw_labelprop_topk_grid / _topk_scores;
 *   rows ...... an index i addresses label row i if i < K * N or n <= K + cxt_size, else row i + (n - cxt_size - K) * N;
 *   labels .... L[n] = sum_j W[j] * L[row(I[j])] in neighbour order from 0.f, pred the first maximum, anchor marks as
 *               crw_labelprop_propagate_sliding reads them; an index outside [0, nf * N) is clamped into it (on every route).
 * Rows of L and columns of pred of the frames before first_frame are the caller's: they are read, never written.
 * n_long = 1 is the sliding rule of crw_hip.h, and every output then equals that of the entry points there bit for bit.
 * CRW_EINVAL for n_long < 1, n_long > T - 1 or first_frame outside 1 .. T - 1. */
#ifndef CRW_HIP_LONGMEM_H
#define CRW_HIP_LONGMEM_H

#include "crw_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* crw_labelprop_topk_grid (raw = 0: WV holds softmax weights) or crw_labelprop_topk_scores (raw = 1: the selected logits) under the
 * rule, on an N x 1 grid; the output layout [T - first_frame][k][N] and the limits as there, the lists up to n_long + cxt_size frames
 * long.  route: 0 chooses as crw_labelprop_topk_grid does for lists of that length, 1 is the vector kernel, 2 the matrix-core
 * kernels; CRW_EINVAL where the forced route does not apply. */
int crw_labelprop_topk_long(const float *ehat, int T, int N, int C, int cxt_size, int n_long, int radius, float temp, int k,
                            int first_frame, float *WV, int32_t *I, int raw, int route, crw_stream_t stream);

/* crw_labelprop_propagate_sliding under the rule, anchor marks included.  There is no seed argument: the caller fills the rows of L
 * (and whatever it wants in pred) before first_frame.  route: 0 chooses, 1 is the general one-workgroup walk with the translation in
 * the kernel, 2 the one-workgroup ring, which keeps the n_long long-term frames in LDS in front of its ring:
 * (cxt_size + 1 + n_long) * N * M * 4 bytes + 16 KiB of list slots <= 150 KiB, knn <= 24, N * M <= 384, knn * N <= 1024;
 * CRW_EINVAL for route 2 where that does not hold. */
int crw_labelprop_propagate_long(const float *W, const int32_t *I, int T, int N, int M, int knn, int first_frame, int cxt_size,
                                 int n_long, float *L, float *pred, int route, crw_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
