/* A memory bank in the parameter sweep: the batched form of crw_labelprop_propagate_long.  A companion of crw_hip.h and
 * crw_hip_longmem.h (same conventions, same status codes, same CRW_ABI_VERSION).  Added at ABI 8 without a bump: a library built
 * before it still loads, the binding tells by symbol (crw_hip.has_sweep_memory()).  The binding mirrors this header in
 * crw_hip.SWEEPMEM_SIGNATURES; tests/test_sweep_longmem_host.py holds the two and the library against each other, and
 * tests/test_sweep_longmem_gpu.py runs the entry point over stale memory and between guard bands.
 *
 * THE RULE is the one of crw_hip_longmem.h, unchanged: a virtual item of T frames whose first K = n_long >= 1 frames are long-term. */
#ifndef CRW_HIP_SWEEPMEM_H
#define CRW_HIP_SWEEPMEM_H

#include "crw_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* crw_labelprop_propagate_long for G configurations in one launch, a workgroup each; the layouts are those of
 * crw_labelprop_propagate_sliding_batch: W [G, T - first_frame, knn, N]; configuration g's indices start at I + g * i_stride (0: one I
 * shared by all); L [G, T * N, M], pred [G, N, T]; shorter lists are padded with weight exactly 0 and a valid index; anchor marks are
 * read as there.  There is no seed argument: the caller fills every L[g]'s rows (and whatever it wants in pred[g]'s columns) before
 * first_frame; they are read, never written.  Slice g of L and pred is bit for bit what crw_labelprop_propagate_long gives on
 * configuration g's lists, on either of its routes; with n_long = 1 and frame 0 filled from a seed, what
 * crw_labelprop_propagate_sliding_batch gives.  An index outside the list it addresses is clamped into it.
 * The n_long long-term frames sit in LDS in front of a ring of min(150 KiB / (4 N M) - n_long, T - first_frame) frames.
 * CRW_EINVAL: n_long < 1, n_long > T - 1, first_frame outside 1 .. T - 1, whatever crw_labelprop_propagate_sliding_batch refuses
 * (G outside 1 .. 65535, knn > 64, cxt_size < 1, N * M * 4 > 30 KiB, T * N * M >= 2^30), and -- one condition per geometry --
 * (n_long + 2) * N * M * 4 > 150 KiB: the bank and a two-frame ring do not fit; loop crw_labelprop_propagate_long over the G
 * slices there (the binding does). */
int crw_labelprop_propagate_long_batch(const float *W, const int32_t *I, size_t i_stride, int G, int T, int N, int M, int knn,
                                       int first_frame, int cxt_size, int n_long, float *L, float *pred, crw_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
