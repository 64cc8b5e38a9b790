/* Context novelty of label propagation -- where a labelled trace would help: a companion of crw_hip.h (same conventions, same
 * status codes, same CRW_ABI_VERSION).  Added at ABI 8 without a bump: a library built before it still loads, the binding tells by
 * symbol (crw_hip.has_novelty()).  The binding mirrors this header in crw_hip.NOVELTY_SIGNATURES; tests/test_novelty_host.py holds
 * the two and the library against each other, and tests/test_novelty_gpu.py runs the entry point over stale memory and between
 * guard bands.
 *
 * THE DEFINITION (tests/novelty_ref.py).  Frame n >= 1 scores against the key frames of the top-k under either context rule: frame
 * a = origin[n] (include/crw_hip_restart.h; 0 without origins) followed by frames max(a + 1, n - cxt_size) .. n - 1, and of each
 * the in-band nodes p, |p - q| < radius, of an N x 1 grid.
 *   nov[n][q] = 1 - max over key frames f and in-band p of <ehat[n][q], ehat[f][p]>      (no temperature)
 *   score[n]  = the mean of the `top` largest nov[n][.]: added in descending order in fp32, then one division
 * How a score becomes a suggestion (the median over the neighbouring frames, the picks) is host work: crw_hip.suggest_frames. */
#ifndef CRW_HIP_NOVELTY_H
#define CRW_HIP_NOVELTY_H

#include "crw_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ehat [T][N][C] normalised features (device); origin [T] int32 (device) as in crw_hip_restart.h, clamped into [0, n - 1], NULL =
 * all zero; nov [T - first_frame][N] and score [T - first_frame] (device) are both written by ONE launch, a workgroup per frame,
 * without global atomics: the same call gives the same bits.
 * route: 0 the matrix route where it applies (C = 16, 32, 64, 128 or 256 and ehat 16-byte aligned: products on
 * v_mfma_f32_16x16x4_f32, a band-masked running maximum in the accumulator rows), else the vector route (a lane per key, any C);
 * 1 the vector route; 2 the matrix route, CRW_EINVAL where it does not apply.
 * CRW_EINVAL also for N > 4096 (a frame's nov row is sorted in LDS), top outside 1 .. N, first_frame outside 1 .. T - 1. */
int crw_labelprop_novelty(const float *ehat, int T, int N, int C, int cxt_size, int radius, int first_frame, int top,
                          const int32_t *origin, float *nov, float *score, int route, crw_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
