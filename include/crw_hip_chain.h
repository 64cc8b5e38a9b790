/* Conv-trunk chain of the CNN encoder: a companion of crw_hip.h (same conventions, same status codes, same CRW_ABI_VERSION).
 * Added at ABI 8 without a bump: a library built before it still loads, the binding tells by symbol (crw_hip.has_conv_chain())
 * and launches the layers one by one through crw_enc_conv3x3 when it is missing.  The binding mirrors this header in
 * crw_hip.CHAIN_SIGNATURES; tests/test_conv_chain_host.py holds the two and the library against each other, and
 * tests/test_conv_chain_gpu.py runs the entry point over stale memory and between guard bands. */
#ifndef CRW_HIP_CHAIN_H
#define CRW_HIP_CHAIN_H

#include "crw_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* conv3 -> conv4 -> conv5 (+ bias, ReLU, and the pooled mean of conv5) of 16x16 patches in one launch, split 3 only: what three
 * mode-0 calls of crw_enc_conv3x3 compute, bit for bit -- (32,64) on x into y3, (64,128) on y3 into y4, (128,128) on y4 into
 * y5_hi and gap -- with the activations handed from layer to layer inside the workgroup that owns the patch.  w*: the forward
 * planes of crw_enc_pack_weights.  Every plane [P][100][C] is written (the backward pass reads them); gap [P][128] may be
 * NULL, the biases may be NULL (zero).  Any other NULL pointer or split: CRW_EINVAL. */
int crw_enc_conv_fwd_chain(int split, int P, const uint16_t *x_hi, const uint16_t *x_lo, const uint16_t *w3_hi,
                           const uint16_t *w3_lo, const float *b3, const uint16_t *w4_hi, const uint16_t *w4_lo, const float *b4,
                           const uint16_t *w5_hi, const uint16_t *w5_lo, const float *b5, uint16_t *y3_hi, uint16_t *y3_lo,
                           uint16_t *y4_hi, uint16_t *y4_lo, uint16_t *y5_hi, float *gap, crw_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
