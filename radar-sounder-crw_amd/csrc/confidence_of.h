// The confidence of one probability row, as crw_labelprop_confidence (confidence.hip: a node's row of L) and crw_labelmap_dense
// (labelmap_dense.hip: a pixel's interpolated row) compute it -- one text, so the two kernels agree on every rule by construction.
#pragma once
#include "crw_common.h"

namespace crw {

template <int KIND>
__device__ inline float confidence_of(const float (&p)[16], int M, float ln_m) {
  if (KIND == CRW_CONF_ENTROPY) {
    float s = 0.f;
#pragma unroll
    for (int m = 0; m < 16; ++m)
      if (m < M) s += p[m] > 0.f ? p[m] * logf(p[m]) : 0.f;  // 0 ln 0 = 0
    const float c = 1.f + s / ln_m;
    return c != c ? c : fminf(fmaxf(c, 0.f), 1.f);
  }
  float m1 = p[0], m2 = -INFINITY;
#pragma unroll
  for (int m = 1; m < 16; ++m)
    if (m < M) {
      const float v = p[m];
      if (v > m1 || v != v) {
        m2 = m1;
        m1 = v;
      } else if (v > m2) {
        m2 = v;
      }
    }
  // a confidence is a number in [0, 1]: the rows of L sum to 1 within rounding only, so an entry (and a margin) can come out one or
  // two ulps above 1 -- that reads 1, every value up to 1 passes through bit for bit (NaN too)
  const float c = KIND == CRW_CONF_MAXPROB ? m1 : m1 - m2;
  return c > 1.f ? 1.f : c;
}

}  // namespace crw
