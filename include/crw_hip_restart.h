/* Anchored label propagation whose context restarts at a fully labelled trace: a companion of crw_hip.h (same conventions, same
 * status codes, same CRW_ABI_VERSION).  Added at ABI 8 without a bump: a library built before it still loads, the binding tells by
 * symbol (crw_hip.has_anchor_restart()).  The binding mirrors this header in crw_hip.RESTART_SIGNATURES; tests/test_restart_host.py
 * holds the two and the library against each other, and tests/test_restart_gpu.py runs every entry point over stale memory and
 * between guard bands.
 *
 * THE RULE.  origin [T] int32 (device) names for every frame n >= 1 the frame a = origin[n] its item starts at: frame n is
 * propagated as frame n' = n - a of the item that starts at frame a.
 *   lists ... the keys are frame a (the long-term frame, in place of frame 0) followed by frames max(a + 1, n - cxt_size) .. n - 1:
 *             what crw_labelprop_topk_grid / _topk_scores write for frame n - a when called on ehat + a * N * C with T - a frames;
 *   rows .... an index i addresses label row a * N + i if i < N or n' <= cxt_size + 1, else a * N + i + (n' - cxt_size - 1) * N;
 *   labels .. L[n] = sum_j W[j] * L[row(I[j])] in neighbour order from 0.f, pred the first maximum, anchor marks as
 *             crw_labelprop_propagate_sliding reads them (a marked node's row is one-hot before the next frame reads it).
 * Which frames are origins is the caller's policy (crw_hip.anchor_origins: frame 0 and every frame whose N nodes are all
 * anchored); the entry points take any sequence that obeys the CHAIN RULE origin[n] in {origin[n - 1], n - 1}, 0 <= origin[n] < n
 * (origin[0] is not read).  The caller checks the rule; the kernels clamp origin[n] into [0, n - 1], so no value addresses out of
 * range -- a sequence that breaks the rule gives defined but meaningless labels.  origin == NULL means all zero, and with origin all
 * zero every output equals the entry point without origins bit for bit. */
#ifndef CRW_HIP_RESTART_H
#define CRW_HIP_RESTART_H

#include "crw_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* crw_labelprop_topk_grid (raw = 0: WV holds softmax weights) or crw_labelprop_topk_scores (raw = 1: the selected logits) under the
 * rule; every other argument, the output layout [T - first_frame][k][N] and the limits as there.  The kernel route is chosen from
 * the whole call's arguments, as without origins: a restart frame scores fewer keys than the bound the route was chosen for. */
int crw_labelprop_topk_origin(const float *ehat, int T, int N, int C, int cxt_size, int radius, float temp, int k, int first_frame,
                              int grid_w, const int32_t *origin, float *WV, int32_t *I, int raw, crw_stream_t stream);

/* crw_labelprop_propagate_sliding under the rule, anchor marks included.  Routes as there; the one-workgroup ring route keeps a
 * second long-term slot and origin[] in LDS: (cxt_size + 3) * N * M * 4 + T * 4 bytes + 16 KiB of list slots <= 150 KiB. */
int crw_labelprop_propagate_origin(const float *seed, const float *W, const int32_t *I, int T, int N, int M, int knn, int first_frame,
                                   int cxt_size, const int32_t *origin, float *L, float *pred, crw_stream_t stream);

/* crw_labelprop_propagate_sliding_batch under the rule: ONE origin array shared by the G configurations. */
int crw_labelprop_propagate_origin_batch(const float *seed, const float *W, const int32_t *I, size_t i_stride, int G, int T, int N,
                                         int M, int knn, int first_frame, int cxt_size, const int32_t *origin, float *L, float *pred,
                                         crw_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
