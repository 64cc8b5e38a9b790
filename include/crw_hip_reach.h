/* Accuracy against the distance from the nearest labelled trace: one confusion matrix per GROUP OF COLUMNS of a label map, in one
 * pass over the maps.  A companion of crw_hip.h (same conventions, same status codes, same CRW_ABI_VERSION).  Added at ABI 8
 * without a bump: a library built before it still loads, the binding tells by symbol (crw_hip.has_reach()).  The binding mirrors
 * this header in crw_hip.REACH_SIGNATURES; tests/test_reach_host.py holds the two and the library against each other, and
 * tests/test_reach_gpu.py runs the entry point over stale memory and between guard bands.
 *
 * OPERANDS.  crw_horizons's: gt, pred and aux (may be NULL) are [rows] x [cols] windows with ld >= cols ELEMENTS between rows, each
 * CRW_DT_F32 or CRW_DT_I8; conf (may be NULL) is fp32 with the same geometry.  No alignment beyond the element's is required and
 * nothing outside the windows is read.  col_group: DEVICE pointer, cols bytes, the group of every column.
 *
 * RULE for pixel (r, c), in this order:
 *   1. g = col_group[c]; g >= groups: dropped[3] += 1 (the column is excluded: its maps are not read);
 *   2. crw_confusion's mask test (gt == ignore_gt, pred == ignore_pred or aux == ignore_aux; -1: none): dropped[0] += 1;
 *   3. crw_confusion's validity test (gt and pred integers in [0, K)): dropped[1] += 1;
 *   4. with conf: NaN or a value outside [0, 1] (crw_calibration's test): dropped[2] += 1;
 *   5. otherwise counts[g][gt][pred] += 1 and conf_sum[g] += conf.
 * So sum(counts) + sum(dropped) == rows * cols.
 *
 * LIMITS.  2 <= K <= 16, 1 <= groups <= CRW_REACH_MAX_GROUPS; rows == 0 or cols == 0 is valid and gives zeros (no operand is
 * read, ws may be NULL).  conf_sum is NULL exactly when conf is.  CRW_EINVAL for anything else the checks can see (null or
 * misaligned pointers: fp32 operands 4 bytes, counts / conf_sum / dropped / ws 8 bytes; ld < cols; an ignore label below -1;
 * ignore_aux without aux), CRW_EWORKSPACE for ws_bytes < crw_confusion_grouped_ws_bytes(rows, cols, K, groups).
 *
 * OUTPUTS.  counts [groups][K][K] int64, conf_sum [groups] fp64, dropped [4] int64: complete in stream order, nothing to pre-clear,
 * every byte of ws that is read is written first.  No global atomics: the integers are bit-reproducible, and conf_sum is added in
 * an order that (rows, cols, col_group) fix -- one fp64 add per pixel down its column's slab of rows, then lanes, slabs and column
 * tiles in index order -- so it is bit-identical from run to run. */
#ifndef CRW_HIP_REACH_H
#define CRW_HIP_REACH_H

#include "crw_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CRW_REACH_MAX_GROUPS 64

size_t crw_confusion_grouped_ws_bytes(int rows, int cols, int K, int groups);

int crw_confusion_grouped(const void *gt, int gt_dtype, const void *pred, int pred_dtype, const void *aux, int aux_dtype,
                          const float *conf, int rows, int cols, size_t ld, const uint8_t *col_group, int groups, int K,
                          int ignore_gt, int ignore_pred, int ignore_aux, int64_t *counts, double *conf_sum, int64_t *dropped,
                          void *ws, size_t ws_bytes, crw_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
