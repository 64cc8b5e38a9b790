/*
 * crw_hip.h -- C ABI of libcrw_hip.so: the MI355X (gfx950) implementation of the
 * contrastive-random-walk hot path of jdalcorso/radar-sounder-crw.
 *
 * The reference is pure Python/PyTorch and has no FFI of its own; its hot path is the sequence
 * of ATen calls listed below.  Each entry point replaces one such group of calls
 * (file:line under the reference repo):
 *
 *   crw_affinity_fwd ........ F.normalize + einsum('bctn,bctm->btnm')/tau      src/model.py:22-26
 *   crw_walk_fwd ............ palindrome cat + (T-2)^2 x {softmax,bmm} +
 *                             (T-2) x cross_entropy + loss/N                  src/model.py:31-46
 *   crw_walk_bwd ............ autograd backward of the above                  (loss.backward(), scripts/train.py:71)
 *   crw_affinity_bwd ........ autograd backward of normalize+einsum           (same)
 *   crw_labelprop_topk ...... einsum + mask + /temp + truncation + topk +
 *                             softmax                                         src/imported/maskedatt.py:151-175
 *   crw_labelprop_gather .... weighted label sum + argmax, frame by frame     src/imported/labelprop.py:106-114, src/utils.py:152-160
 *   crw_labelprop_propagate . the same, chained prefix + parallel tail          (same lines; context bound of maskedatt.py:165-166)
 *   crw_labelprop_propagate_sliding(_batch)
 *                             the same sums with the indices applied to the      src/imported/crw.py (the vendored upstream routine
 *                             frames they were scored on (opt-in rule)           gathers from the scored frames; labelprop.py does not)
 *   crw_labelprop_topk_scores / crw_labelprop_sweep_weights / crw_labelprop_propagate_batch
 *                             the same lists and labels for a whole grid of
 *                             (radius, temp, knn) settings at once              scripts/launch/launch_test_batch.sh
 *   crw_xent_metric ......... "horizontality" metric                          src/utils.py:117-125
 *   crw_confusion ........... remove_unc masks + pred.cpu() + sklearn
 *                             classification_report / confusion_matrix counts scripts/test/test_all.py:161-187
 *   crw_labelprop_confidence / crw_merge_confidence / crw_calibration
 *                             the soft labels the scripts arg-max away          src/utils.py:160 (maskedatt.py CRW.forward:
 *                             (per-node confidence, a merge ruled by it,        masks_pred_conf), scripts/test/test_all.py:146-159
 *                             a reliability histogram): no reference twin
 *   crw_labelmap_dense ...... bilinear upsampling of the soft labels + argmax,   src/imported/crw.py:124-127 (the upstream routine;
 *                             the pixel map (and its confidence) in one pass     the radar scripts arg-max first and stretch the
 *                                                                                node map with Resize(NEAREST): no twin there)
 *   crw_labelmap_dense_batch  the same map for every configuration of a sweep     (no twin: scripts/launch/launch_test_batch.sh
 *                             in one launch                                       runs test_all.py per setting, nearest maps)
 *   crw_labelmap_ordered[_batch]  the same interpolated probabilities decoded      (no twin: no script of the reference uses the
 *                             under a layer order, a DP per pixel column          order of the layers down a trace)
 *   crw_labelmap_ordered_joint[_batch]  that decode over two passes' rows, per pixel  (no twin: test_all.py:146-159 merges the two
 *                             the surer pass's: an order-preserving merge          label maps by a class rule)
 *   crw_labelmap_ordered[_joint]_posterior[_batch]  the posterior of those decodes over  (no twin)
 *                             the monotone paths: confidence and horizon error bars
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless its name ends in _host;
 *   - tensors are dense row-major fp32 with the shapes given per function;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); nothing synchronises;
 *   - no allocation inside: workspaces are sized with the crw_*_bytes() queries and passed in;
 *   - return value: CRW_OK or an error code; nothing is thrown across the ABI;
 *   - Threads: the kernels' entry points keep no state between calls and may be called from any thread (one caller per stream).
 *     Two corners do keep state: crw_rn_train_fwd / crw_rn_train_bwd / crw_rn_eval_fwd order part of their work on one internal
 *     side stream PER DEVICE (created on first use, with its event pool) -- at most one host thread per device may be inside them
 *     at a time; and the crw_rn_timing_* diagnostic (one global record list).  Everything they enqueue on the side stream is joined
 *     back into the caller's stream before they return, on error paths too.
 *
 * Non-finite values (NaN, +inf, -inf; never told apart: the hi/lo bf16 split turns inf into NaN) on the training path -- the
 * encoders, crw_normalize, crw_affinity_fwd / _bwd, crw_walk_fwd / _bwd, crw_adam_step -- behave as in the reference's PyTorch ops
 * (relu, max_pool2d, clamp_min, softmax propagate them); DESIGN.md section 3e, tests/test_nonfinite_gpu.py:
 *   - no laundering: wherever the reference's output is non-finite, ours is (features, ehat, norm, A, At_out, loss, dA, demb,
 *     parameter gradients, BatchNorm running statistics, Adam's p / m / v); for A, the loss and the encoder features the masks are
 *     EQUAL (no spurious NaN either; a poison in the last frame, whose logits feed no cycle, leaves the loss finite); a row or
 *     column of A that holds a non-finite logit has a non-finite sum in the `stats` of crw_affinity_fwd;
 *   - no contamination: what the reference keeps bit-equal to its clean run stays bit-equal to OUR clean run -- the other patches
 *     of the CNN and of the eval-mode Resnet, the other batch items' A / At_out / dA / demb, the other elements of Adam's buffers;
 *   - finite inputs give the bits they always gave.
 * Label propagation on non-finite features is outside this contract.
 */
#ifndef CRW_HIP_H
#define CRW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumps when a signature changes.  Entry points added at 8 without a bump (pure additions, no existing signature touched; the
 * binding detects them by symbol, crw_hip.has_sweep()): crw_labelprop_topk_scores, crw_labelprop_sweep_weights,
 * crw_labelprop_propagate_batch; then crw_labelprop_confidence, crw_merge_confidence, crw_calibration_ws_bytes, crw_calibration
 * (crw_hip.has_confidence()); then crw_labelmap_dense (crw_hip.has_dense()); then crw_labelmap_dense_batch
 * (crw_hip.has_dense_batch()); then crw_horizons_ws_bytes, crw_horizons (crw_hip.has_horizons()); then
 * crw_labelprop_propagate_sliding, crw_labelprop_propagate_sliding_batch (crw_hip.has_sliding()); then
 * crw_labelmap_ordered_workspace, crw_labelmap_ordered, crw_labelmap_ordered_batch (crw_hip.has_ordered()); then
 * crw_labelmap_ordered_joint, crw_labelmap_ordered_joint_batch (crw_hip.has_joint()); then crw_labelmap_posterior_workspace,
 * crw_labelmap_ordered_posterior, crw_labelmap_ordered_joint_posterior (crw_hip.has_posterior()); then
 * crw_labelmap_posterior_workspace_batch, crw_labelmap_ordered_posterior_batch, crw_labelmap_ordered_joint_posterior_batch
 * (crw_hip.has_posterior_batch()); the conv-trunk chain of include/crw_hip_chain.h came the same way
 * (crw_hip.has_conv_chain()).  The ONE place the number is
 * written: crw_abi_version() returns it, the ctypes binding (crw_hip.ABI_VERSION) parses it from this header, and __graft_entry__.build() / the host tests compare
 * the two. */
#define CRW_ABI_VERSION 8

#define CRW_OK 0
#define CRW_EINVAL 1     /* bad shape / null pointer / unsupported size            */
#define CRW_EWORKSPACE 2 /* workspace too small                                     */
#define CRW_EHIP 3       /* a HIP launch failed (see crw_last_hip_error)            */

/* arithmetic used inside the transition-matrix chain */
#define CRW_CHAIN_F32 0  /* exact fp32 MFMA (v_mfma_f32_16x16x4_f32), parity path   */
#define CRW_CHAIN_BF16 1 /* bf16 operands, fp32 accumulate (v_mfma_f32_16x16x32_bf16) */
#define CRW_CHAIN_BF16X3 2 /* hi/lo bf16 operand pairs, 3 MFMAs per product: fp32-grade results */

typedef void *crw_stream_t;

/* library / build info ------------------------------------------------------------------- */
int crw_abi_version(void);          /* CRW_ABI_VERSION of the header the library was built with */
const char *crw_build_arch(void);   /* "gfx950"                                             */
int crw_last_hip_error(void);       /* last hipError_t seen by this thread (0 = none)       */

/* geometry ------------------------------------------------------------------------------- */
/* node count padded to the tile size of the chain GEMM (all internal NxN matrices are stored
 * [Np][Np] with zero padding). */
int crw_padded_nodes(int N, int chain);
/* bytes of the state buffer written by crw_walk_fwd and consumed by crw_walk_bwd */
size_t crw_walk_state_bytes(int B, int T, int N, int chain);
/* bytes of the scratch buffer needed by crw_walk_bwd */
size_t crw_walk_scratch_bytes(int B, int T, int N, int chain);

/* training path --------------------------------------------------------------------------- */
/* emb [B,T,N,C] raw encoder output -> ehat [B,T,N,C] (L2-normalised, eps 1e-12),
 * norm [B,T,N] (= max(||e||, eps)), A [B,T-1,N,N] = ehat_t ehat_{t+1}^T / tau.
 * stats (may be NULL): [4][B][T-1][N] = row max, row sum exp, column max, column sum exp of every A[b,t] -- the
 * statistics of the two softmaxes of src/model.py:44 (F = softmax(A), G = softmax(A^T)), produced in the epilogue of
 * the affinity tiles so that crw_walk_fwd needs no pass over A to find them; needs ws of crw_affinity_ws_bytes. */
size_t crw_affinity_ws_bytes(int B, int T, int N);
int crw_affinity_fwd(const float *emb, int B, int T, int N, int C, float tau,
                     float *ehat, float *norm, float *A, float *stats, void *ws, size_t ws_bytes, crw_stream_t stream);

/* A [B,T-1,N,N] -> loss[1] (= sum_k l_k / N, Appendix A.2 of SURVEY.md).
 * state: crw_walk_state_bytes(B,T,N) bytes, kept by the caller until crw_walk_bwd.
 * At_out: optional [B,T-2,N,N] copy of every per-cycle transition product (may be NULL).
 * chain: CRW_CHAIN_F32 | CRW_CHAIN_BF16 | CRW_CHAIN_BF16X3 (same value for fwd, bwd and the size
 * queries).   T < 3 -> loss = 0. */
int crw_walk_fwd(const float *A, const float *stats /* of crw_affinity_fwd, or NULL: computed here */, int B, int T, int N,
                 int chain, void *state, size_t state_bytes, float *At_out, float *loss, crw_stream_t stream);

/* gloss[1] (device scalar, dL/dloss) + the logits A the forward ran on + state -> dA [B,T-1,N,N]
 * (the two softmaxes are recomputed from A and the statistics kept in `state`: half the bytes of storing them). */
int crw_walk_bwd(const float *gloss, const float *A, int B, int T, int N, int chain,
                 void *state, size_t state_bytes, void *scratch, size_t scratch_bytes,
                 float *dA, crw_stream_t stream);

/* dA [B,T-1,N,N], ehat, norm -> demb [B,T,N,C]; dehat_ws is a [B,T,N,C] scratch. */
int crw_affinity_bwd(const float *dA, const float *ehat, const float *norm, int B, int T, int N, int C,
                     float tau, float *dehat_ws, float *demb, crw_stream_t stream);

/* inference path -------------------------------------------------------------------------- */
/* emb [T,N,C] raw -> ehat [T,N,C] (reuses the normalise kernel of crw_affinity_fwd). */
int crw_normalize(const float *emb, int rows, int C, float *ehat, float *norm, crw_stream_t stream);

/* For every frame n = first_frame..T-1 (first_frame >= 1; 1 = whole radargram, T-1 = the
 * reference's one-frame-at-a-time LabelPropVOS_CRW.predict) and query node q: top-`knn` keys among the context frames
 * (frame 0 + last `cxt_size` frames once n > cxt_size+1, else frames 0..n-1) restricted to the
 * band |m-q| < radius, logits <key,query>/temp, softmax over the knn.
 * W [T-first_frame,knn,N] weights, I [same] int32 indices into the (truncated) key list.
 * Requires 1 <= radius, 1 <= knn <= 64. Slots beyond the number of in-band keys get weight 0
 * (the reference fills them with masked keys whose softmax weight is exactly 0).
 * Scores are exact fp32 products accumulated in fp32: on the fp32 matrix cores when N >= 16, C is 64, 128 or 256 and ehat is 16-byte
 * aligned, else on the vector units -- the two differ in summation order only. */
int crw_labelprop_topk(const float *ehat, int T, int N, int C, int cxt_size, int radius, float temp,
                       int knn, int first_frame, float *W, int32_t *I, crw_stream_t stream);
/* The same on a 2-D node grid: the N nodes of a frame are an (N / grid_w) x grid_w grid in row-major order and the band is the
 * Euclidean disc (i - i')^2 + (j - j')^2 < radius^2 of MaskedAttention (src/imported/maskedatt.py:222-245); grid_w = 1 is
 * crw_labelprop_topk (a radargram's frames are N x 1 columns of patches, the only grid the reference's scripts produce). */
int crw_labelprop_topk_grid(const float *ehat, int T, int N, int C, int cxt_size, int radius, float temp, int knn, int first_frame,
                            int grid_w, float *W, int32_t *I, crw_stream_t stream);

/* seed [N] float class ids of frame 0 (NULL: rows of L for frames < first_frame are already
 * filled by the caller); W,I from crw_labelprop_topk with the same first_frame;
 * L [T*N, M] soft labels (frames >= first_frame written), pred [N,T] float class ids
 * (columns >= first_frame written; column 0 = seed when seed is given). */
int crw_labelprop_gather(const float *seed, const float *W, const int32_t *I, int T, int N, int M, int knn,
                         int first_frame, float *L, float *pred, crw_stream_t stream);
/* The same result for lists that come from crw_labelprop_topk(_grid) with context size `cxt_size` (same first_frame): their
 * indices address the truncated key list, i.e. frame n's are < min(n, cxt_size + 1) * N, and the reference applies them to the
 * untruncated label list (src/imported/labelprop.py:103-107 with src/imported/maskedatt.py:165-166) -- so only frames
 * first_frame .. cxt_size form a chain (one workgroup, all their labels in LDS) and every later frame reads frames 0 .. cxt_size
 * alone (one workgroup per frame, all at once).  Bit-identical L and pred; indices outside the bound are clamped to rows before
 * the frame's own, never out of range.  Falls back to crw_labelprop_gather where the chained frames' labels exceed the LDS. */
int crw_labelprop_propagate(const float *seed, const float *W, const int32_t *I, int T, int N, int M, int knn, int first_frame,
                            int cxt_size, float *L, float *pred, crw_stream_t stream);

/* Sweeps over (radius, temp, knn) -- the grid of the reference's scripts/launch/launch_test_batch.sh -- share everything that does
 * not depend on the setting.  Each entry point is defined by equality with one above.
 *
 * crw_labelprop_topk_scores: crw_labelprop_topk_grid with kcap (1 ... 64) in place of knn, through the same kernels and the same
 * route choice, with another last line of the epilogue: V [T-first_frame, kcap, N] is the selected logit fl(<key, query> / temp)
 * in selection order instead of its softmax weight (empty slot: V = -inf, I = 0).  I equals crw_labelprop_topk_grid(..., knn =
 * kcap)'s, and because selection is sequential (highest score, then lowest candidate index) its first k entries are the lists of
 * knn = k.  Selection is per temperature, on the quotient: fp32 division maps distinct scores onto equal quotients, and the tie
 * rule then orders them by index. */
int crw_labelprop_topk_scores(const float *ehat, int T, int N, int C, int cxt_size, int radius, float temp, int kcap, int first_frame,
                              int grid_w, float *V, int32_t *I, crw_stream_t stream);
/* V [F, kcap, N] of the call above, knns: nk (1 ... 16) values on the HOST, each 1 ... kcap -> W [nk, F, kmax, N], kmax = max(knns):
 * W[i][:, :knns[i], :] is bit-identical to the W of crw_labelprop_topk_grid(..., knn = knns[i]) (the epilogues' expression in their
 * order: vmax = V[0]; the sum over j < knn, -inf -> 0; expf(v - vmax) / sum), slots >= knns[i] are 0. */
int crw_labelprop_sweep_weights(const float *V, int F, int kcap, int N, const int *knns, int nk, float *W, crw_stream_t stream);
/* crw_labelprop_propagate for G configurations at once: W [G, T-first_frame, knn, N]; configuration g's indices start at
 * I + g * i_stride elements (0: one I shared by all); one seed [N] (or NULL: every L[g]'s frames < first_frame are filled);
 * L [G, T*N, M], pred [G, N, T].  knn is the length of the lists as stored: a configuration with fewer neighbours pads with
 * weights that are exactly 0 on valid indices (crw_labelprop_sweep_weights), which leaves every sum as it is.  Slice g of L and
 * pred is bit-identical to crw_labelprop_propagate on that configuration's lists.  A workgroup per configuration walks the
 * chained frames (frame 0 and a ring of recent frames in LDS, older labels from L), the frames beyond the context bound are a
 * grid over (frame, configuration).  CRW_EINVAL: G > 65535, knn > 64, N * M > 7680 (a ring of four frames must fit the LDS). */
int crw_labelprop_propagate_batch(const float *seed, const float *W, const int32_t *I, size_t i_stride, int G, int T, int N, int M,
                                  int knn, int first_frame, int cxt_size, float *L, float *pred, crw_stream_t stream);

/* The "sliding" context rule (opt-in; the reference's rule is the two entry points above).  W, I are the lists of
 * crw_labelprop_topk(_grid) / _topk_scores at `cxt_size`, untouched; an index i of frame n addresses the list it was SCORED on,
 * [frame 0, frames n - cxt_size .. n - 1], i.e. label row
 *     row(i, n) = i                                  if i < N or n <= cxt_size + 1
 *                 i + (n - cxt_size - 1) * N         otherwise
 * and L[n] = sum_j W[j] * L[row(I[j], n)] in neighbour order from 0.f, pred the first maximum.  Defined as bit-identical L and pred
 * to crw_labelprop_gather on lists whose indices were translated by row().  Every frame needs the one before it: one chain over all
 * frames, no parallel tail.  Route: one workgroup with frame 0 and a ring of cxt_size + 1 frames in LDS when
 * (cxt_size + 2) * N * M * 4 bytes + 16 KiB of list slots <= 150 KiB, knn <= 24, N * M <= 384 and knn * N <= 1024 (there an index
 * outside [0, min(n, cxt_size + 1) * N) is clamped into it); otherwise crw_labelprop_gather's kernels with the translation done in
 * the kernel (nothing is allocated, I is not copied).  CRW_LABELPROP_SLIDING_GENERAL=1 (read per call) takes the second route.
 *
 * ANCHOR MARKS (these two entry points only; the LDS of the first route does not grow for them).  A softmax weight is never
 * negative, so a list whose slot-0 weight W[f - first_frame][0][q] is EXACTLY -inf (bits 0xFF800000, CRW_LABELPROP_ANCHOR_WEIGHT)
 * is a mark: node q of frame f is anchored to the class its slot-0 index I[f - first_frame][0][q] names, clamped into [0, M - 1]
 * (like every index, it never addresses out of range).  For a marked node L[f*N + q] is exactly the one-hot of the class, written
 * as 1.0f and +0.0f, pred[q][f] is the class, the other slots of the list are ignored, and every later frame reads the clamped
 * row.  Every other weight value -- other negative values and NaN included -- means what it meant before, and lists without a mark
 * give the bits they gave before.  crw_labelprop_gather, crw_labelprop_propagate and crw_labelprop_propagate_batch know no mark
 * (under the reference rule an anchor beyond frame cxt_size would change only itself).  A library older than the marks has the
 * same entry points at the same ABI and turns the -inf into NaN: ask it with one tiny marked call (crw_hip.has_anchor_lists()). */
#define CRW_LABELPROP_ANCHOR_WEIGHT (-__builtin_inff())
int crw_labelprop_propagate_sliding(const float *seed, const float *W, const int32_t *I, int T, int N, int M, int knn, int first_frame,
                                    int cxt_size, float *L, float *pred, crw_stream_t stream);
/* G configurations at once, arguments and limits as crw_labelprop_propagate_batch: a workgroup per configuration walks ALL frames
 * first_frame .. T-1 (no second launch).  Slice g of L and pred is bit-identical to crw_labelprop_propagate_sliding on that
 * configuration's lists -- anchor marks included: the marks are configuration g's (W[g]), the classes may be shared (i_stride 0),
 * and a configuration padded to a longer knn keeps slot 0 as a real slot (knn >= 1). */
int crw_labelprop_propagate_sliding_batch(const float *seed, const float *W, const int32_t *I, size_t i_stride, int G, int T, int N,
                                          int M, int knn, int first_frame, int cxt_size, float *L, float *pred, crw_stream_t stream);

/* HOST function (no GPU work, host pointers): the change-point search of `propagate` (src/utils.py:125-132,
 * ruptures.Pelt(model="rbf").fit(signal).predict(pen)) -- PELT with the RBF kernel cost at ruptures' documented defaults
 * min_size 2, jump 5; gamma <= 0: the median heuristic.  signal [n] doubles -> sorted breakpoints bkps[0..count) (segment ends, the
 * last one is n); returns count >= 1, or a negative status.  The arithmetic of pelt.py in the same order (parity with ruptures
 * itself is unpinned: it is not installed here). */
int crw_pelt_rbf(const double *signal, int n, double pen, int min_size, int jump, double gamma, int *bkps, int max_bkps);

/* ehat [T,N,C] -> xent [N,T-1]  (channel-shifted within-frame affinity / 0.1, CE vs identity) */
int crw_xent_metric(const float *ehat, int T, int N, int C, float *xent, crw_stream_t stream);

/* evaluation ------------------------------------------------------------------------------ */
/* Confusion matrix of a label map against its ground truth, with the reference's "remove uncertain class" masks as arguments
 * (scripts/test/test_all.py:161-187) -- one pass over the maps in HBM instead of boolean-index copies, a device-to-host copy and
 * two sklearn calls.  gt, pred, aux (may be NULL): P labels each, dense, of the dtype their code names (CRW_DT_F32: what
 * `segment` returns, 4-byte aligned; CRW_DT_I8: what the drivers save); no other alignment is asked for (views into a wider map).
 * counts [K][K]: counts[g][p] = pixels with ground truth g and prediction p that survive the mask.  A pixel is masked -- counted
 * in dropped[0] -- when gt == ignore_gt, pred == ignore_pred or aux == ignore_aux (-1 = no such label; aux values are compared,
 * never binned, so an ignore label may lie outside [0, K)).  A surviving pixel whose gt or pred is not an integer in [0, K) (NaN
 * included) is counted in dropped[1] and in no bin; nothing is read out of bounds for any label value.
 * 2 <= K <= 16.  P == 0 is valid and gives zeros.  counts and dropped are complete in stream order after the call and need no
 * pre-clearing; integer sums: bit-reproducible.  ws: crw_confusion_ws_bytes(P, K) bytes (per-workgroup partial counts). */
#define CRW_DT_F32 0
#define CRW_DT_I8 1
size_t crw_confusion_ws_bytes(size_t P, int K);
int crw_confusion(const void *gt, int gt_dtype, const void *pred, int pred_dtype, const void *aux, int aux_dtype, size_t P, int K,
                  int ignore_gt, int ignore_pred, int ignore_aux, int64_t *counts /* [K][K] */,
                  int64_t *dropped /* [2]: masked, invalid */, void *ws, size_t ws_bytes, crw_stream_t stream);

/* Layer horizons and thickness of a label map against its ground truth: crw_confusion's operands, dtypes, mask and validity rules
 * (dropped[0] and dropped[1] equal crw_confusion's on the same maps), read as [rows] x [cols] windows with `ld` >= cols elements
 * between rows -- pixel (r, c) is element r * ld + c of every operand; nothing outside the windows is read, no alignment beyond
 * the element's is asked for.  A masked or invalid pixel has no class in either map.  A run is a maximal set of consecutive rows
 * of one column with one class in one map; it qualifies when it is at least min_run (>= 1) rows long.  Per map (0 gt, 1 pred),
 * class k and column: top = the first row of the first qualifying run of k, bottom = the last row of the last one, count = the
 * pixels in qualifying runs of k (the layer thickness); top = bottom = -1 and count = 0 when there is none.
 * picks (may be NULL: then nothing of size cols is written) [2][3][K][cols] int32: map x (top, bottom, count).
 * stats [K][18], over the columns: n_both (gt and pred have k), n_missing (gt only), n_spurious (pred only); then for top, bottom
 * and count in turn, over the n_both columns with d = pred - gt: sum |d|, sum d^2, max |d|, columns with |d| <= tol, sum d.
 * 2 <= K <= 16, tol >= 0, rows <= 32768 (d^2 < 2^30; every sum fits int64); rows == 0 or cols == 0 is valid and gives zero
 * statistics.  row_slabs: a column's rows are scanned in that many slabs, one wave each, joined afterwards (a run that spans
 * slab borders is judged once, at its whole length); 0 = the library chooses, 1 ... 8 forces the number (clamped to rows).
 * Outputs are complete in stream order and need no pre-clearing; no global atomics (per-workgroup partials in ws, added -- the
 * maxima: maximised -- by a second kernel in a fixed order): bit-reproducible.  ws: crw_horizons_ws_bytes(rows, cols, K) bytes,
 * 8-byte aligned (0: bad arguments, or cols == 0). */
size_t crw_horizons_ws_bytes(int rows, int cols, int K);
int crw_horizons(const void *gt, int gt_dtype, const void *pred, int pred_dtype, const void *aux, int aux_dtype, int rows, int cols,
                 size_t ld, int K, int ignore_gt, int ignore_pred, int ignore_aux, int min_run, int tol, int row_slabs,
                 int32_t *picks /* [2][3][K][cols]; may be NULL */, int64_t *stats /* [K][18] */,
                 int64_t *dropped /* [2]: masked, invalid */, void *ws, size_t ws_bytes, crw_stream_t stream);

/* confidence ------------------------------------------------------------------------------ */
/* Confidence of every node from the soft labels of crw_labelprop_propagate / _gather: L [T*N, M] (a probability row per node,
 * 4-byte aligned; 16-byte loads when it is 16-byte aligned and M % 4 == 0) -> conf [N, T], the layout of pred.  Columns >=
 * first_frame are written (first_frame >= 1), and column 0 as well when first_frame == 1: frame 0's rows are then the one-hot
 * seed, which gives 1 for every kind.  2 <= M <= 16.
 *   CRW_CONF_MAXPROB  max_m p_m (bitwise the largest entry)
 *   CRW_CONF_MARGIN   the largest entry minus the second largest, one fp32 subtraction; a duplicated maximum gives 0
 *                     (both: a result above 1 reads 1 -- propagated rows sum to 1 within rounding only, and a confidence is a
 *                     number in [0, 1], which crw_calibration insists on)
 *   CRW_CONF_ENTROPY  1 + sum_m p_m ln p_m / ln M with 0 ln 0 = 0, fp32, terms added in index order, clamped to [0, 1] */
#define CRW_CONF_MAXPROB 0
#define CRW_CONF_MARGIN 1
#define CRW_CONF_ENTROPY 2
int crw_labelprop_confidence(const float *L, int T, int N, int M, int kind, int first_frame, float *conf, crw_stream_t stream);

/* Per-pixel merge of two passes over the same P pixels by their confidence: the reverse pass wins where rev_conf > fwd_conf,
 * strictly -- a tie keeps the forward label, and so does a NaN on either side.  out_lab / out_conf = the winner's label (copied,
 * never decoded: any value) and confidence; took (uint8, may be NULL) = 1 where the reverse pass won.  lab_dtype: CRW_DT_F32 or
 * CRW_DT_I8, one dtype for the three label maps; no alignment beyond the element's is asked for (views into a wider map take a
 * scalar head / tail, or the scalar route throughout where the pointers share no 16-byte phase).  out_* may be fwd_*. */
int crw_merge_confidence(const void *fwd_lab, const float *fwd_conf, const void *rev_lab, const float *rev_conf, int lab_dtype,
                         size_t P, void *out_lab, float *out_conf, uint8_t *took, crw_stream_t stream);

/* Reliability histogram of a confidence map: crw_confusion's pass (its operands, dtypes, mask and validity rules, in its order --
 * dropped[0] and dropped[1] equal crw_confusion's on the same maps) with the surviving pixels binned by confidence instead of
 * by class pair.  conf: P fp32 values; bin b = min(bins - 1, (int)floorf(conf * bins)), the product in fp32; 1 <= bins <= 64.
 * counts [bins][2]: pixels, and pixels with gt == pred; conf_sum [bins] (double): the sum of the bin's confidences;
 * dropped [3]: masked, invalid label, invalid confidence (NaN or outside [0, 1]; checked last, counted in no bin).
 * P == 0 is valid and gives zeros; outputs are complete in stream order and need no pre-clearing.  The integers are
 * bit-reproducible; conf_sum is bit-identical from run to run on the same P and pointer alignment (no atomics: lanes, waves and
 * workgroups are added in a fixed order).  ws: crw_calibration_ws_bytes(P, K, bins) bytes, 8-byte aligned (0: bad K or bins). */
size_t crw_calibration_ws_bytes(size_t P, int K, int bins);
int crw_calibration(const void *gt, int gt_dtype, const void *pred, int pred_dtype, const float *conf, const void *aux, int aux_dtype,
                    size_t P, int K, int bins, int ignore_gt, int ignore_pred, int ignore_aux, int64_t *counts /* [bins][2] */,
                    double *conf_sum /* [bins] */, int64_t *dropped /* [3] */, void *ws, size_t ws_bytes, crw_stream_t stream);

/* dense label maps ------------------------------------------------------------------------ */
/* Pixel-resolution label map of one pass from its soft labels: L [T*N, M] (node (n, t) is row t*N + n; 4-byte aligned, wider
 * loads where its address and M allow) is interpolated bilinearly to [rows, cols] -- rows along the nodes n, columns along the
 * frames t -- and the interpolated row of every pixel is arg-maxed; the interpolated probabilities are never written.
 * Geometry: the half-pixel convention of F.interpolate(mode='bilinear', align_corners=False), in integers.  For output row r:
 * a = (2r + 1) N - rows, d = 2 rows (64-bit); a <= 0: i0 = i1 = 0, w = 0; else i0 = a / d; i0 >= N - 1: i0 = i1 = N - 1, w = 0;
 * else i1 = i0 + 1, w = (float)(a - i0 d) / (float)d -- exact knots, and a weight that is the correctly rounded fp32 quotient of
 * two integers fp32 holds exactly.  Columns likewise with T and cols.  1 <= rows, cols <= 2^22; T, N >= 1; 2 <= M <= 16.
 * Arithmetic, per class, fp32: v = (1-wr) ((1-wc) p00 + wc p01) + wr ((1-wc) p10 + wc p11), p01 the next frame's node, p10 the
 * next node; each of the three sums as fma(w, b, round((1-w) a)) -- written out, not left to the compiler's contraction, so every
 * pixel of this kernel and of crw_labelmap_dense_batch rounds alike.  Label: the class of the largest v, the lowest class on exact equality.  conf (conf_kind:
 * a CRW_CONF_* kind; -1: none, conf NULL): crw_labelprop_confidence's formula on the interpolated row.  L is assumed finite.
 * flip != 0: output column c holds what column cols - 1 - c would hold (the reverse pass's maps are mirrored).
 * labels (label_dtype CRW_DT_F32 or CRW_DT_I8) and conf are [rows] x [cols] windows of maps with `ld` >= cols elements between
 * rows (one pitch for both); no alignment beyond the element's is asked for: 16-byte stores (int8: packed 32-bit) where a lane's
 * 4 pixels lie inside the window on such a boundary, single pixels at a row's head and tail; nothing outside the window is
 * written.  One launch, plain vector stores, bit-reproducible. */
int crw_labelmap_dense(const float *L, int T, int N, int M, int rows, int cols, int flip, int conf_kind, void *labels,
                       int label_dtype, float *conf, size_t ld, crw_stream_t stream);
/* crw_labelmap_dense for the G configurations of a sweep's pass in ONE launch (no reference twin; correctness is equality with the
 * one-map call).  L [G, T*N, M], as crw_labelprop_propagate_batch leaves it; configuration g's outputs are the [rows] x [cols]
 * windows at labels + g * map_stride elements and conf + g * map_stride, pitch `ld` -- so maps[:, :, a:b] of a [G, rows, width]
 * tensor is a valid target.  Slice g is bit-identical to crw_labelmap_dense(L + g*T*N*M, ...) written into the same window, labels
 * and confidence (one device function holds the per-pixel arithmetic of both kernels); nothing outside the G windows is written.
 * crw_labelmap_dense's limits, and 1 <= G <= 65535, map_stride >= (rows-1)*ld + cols.  One launch, plain vector stores, no atomics,
 * bit-reproducible. */
int crw_labelmap_dense_batch(const float *L, int G, int T, int N, int M, int rows, int cols, int flip, int conf_kind, void *labels,
                             int label_dtype, float *conf, size_t ld, size_t map_stride, crw_stream_t stream);

/* Depth-ordered label maps: crw_labelmap_dense's interpolated probabilities v (the same device function, bit for bit), decoded
 * per pixel column under a layer order instead of arg-maxed pixel by pixel.  order_host: S distinct classes of 0 ... M-1, top to
 * bottom (a HOST array, read before the launch and passed to the kernel by value), 2 <= S <= M; a class outside it is never
 * written.  With e[r][s] = v[r][c][order[s]], per column c, in fp32, one rounded add per row:
 *   D[0][s] = e[0][s];   D[r][s] = e[r][s] + max_{s' <= s} D[r-1][s'],  predecessor: the LOWEST s' that attains the prefix maximum;
 *   last state: the LOWEST s that attains max_s D[rows-1][s];  backtrack;  label[r] = order[state[r]].
 * The labels of a column never step back in `order`; a column may start and end in any state, a layer may be absent.  The score is
 * the SUM of the probabilities (the expected number of right pixels), not of their logarithms: seed frames are one-hot, L holds
 * exact zeros.  Back-pointers: one bit per (row, state), "state s is a new prefix maximum" (strict >), a uint16 per pixel --
 * pred(s) is the highest set bit <= s, because the prefix arg-max does not decrease with s.  They live in `ws`
 * (crw_labelmap_ordered_workspace(G, rows, cols) bytes, 2-byte aligned; its layout is the kernel's; what it held before is never
 * read): too few bytes -> CRW_EWORKSPACE.  conf (conf_kind as for crw_labelmap_dense) is the confidence of the interpolated row,
 * bit for bit what crw_labelmap_dense writes: it does not depend on the decode.  labels / conf / ld / flip / label_dtype and every
 * limit: crw_labelmap_dense's; in addition order_host and ws non-null, its entries distinct and in range, 2 <= S <= M -- all
 * refused (CRW_EINVAL) before anything is launched.  One launch, one route for every size: a lane per column, a wave per 64
 * columns, rows steps in series; plain vector stores, no atomics, bit-reproducible. */
size_t crw_labelmap_ordered_workspace(int G, int rows, int cols);
int crw_labelmap_ordered(const float *L, int T, int N, int M, int rows, int cols, int flip, const int *order_host, int S,
                         int conf_kind, void *labels, int label_dtype, float *conf, size_t ld, void *ws, size_t ws_bytes,
                         crw_stream_t stream);
/* crw_labelmap_ordered for the G configurations of a sweep's pass in ONE launch (the configuration is a grid dimension): L, the
 * windows, l_stride = T*N*M and map_stride as for crw_labelmap_dense_batch, one `order` for all.  Slice g is bit-identical to
 * crw_labelmap_ordered(L + g*T*N*M, ...) written into the same window. */
int crw_labelmap_ordered_batch(const float *L, int G, int T, int N, int M, int rows, int cols, int flip, const int *order_host,
                               int S, int conf_kind, void *labels, int label_dtype, float *conf, size_t ld, size_t map_stride,
                               void *ws, size_t ws_bytes, crw_stream_t stream);

/* The ordered decode over the evidence of two passes, merged BEFORE the decode -- an order-preserving merge of a forward and a
 * reverse pass.  Two sources k = a, b: L_k [T_k*N, M] soft labels under a cols_k-wide map; the [rows] x [ncols] output window is the
 * columns col0_k ... col0_k + ncols - 1 of it, mirrored with flip_k as crw_labelmap_dense mirrors them.  N, M, rows, the order, the
 * confidence kind and the outputs are shared.  At output pixel (r, x), bit for bit in fp32:
 *   v_k, conf_k = what crw_labelmap_dense(L_k, T_k, N, M, rows, cols_k, flip_k, conf_kind) computes at pixel (r, col0_k + x)
 *                 (the same device function, the same three lerp steps);
 *   took = conf_b > conf_a  -- crw_merge_confidence's comparison: a tie keeps a, and so does a NaN on either side;
 *   e[r][s] = (took ? v_b : v_a)[order[s]];   then crw_labelmap_ordered's recurrence, tie rules and backtrack, unchanged;
 *   conf[r][x] = took ? conf_b : conf_a  -- what crw_merge_confidence writes for the two dense confidence maps.
 * The labels of a column never step back in `order`, whatever `took` does down the column.  conf_kind is mandatory (-1:
 * CRW_EINVAL); conf may be NULL: the labels alone are written.  ws: crw_labelmap_ordered_workspace(G, rows, ncols) bytes, as for
 * crw_labelmap_ordered (too few -> CRW_EWORKSPACE).  Per source: L_k non-null and 4-byte aligned (the two may be one pointer),
 * T_k >= 1, 1 <= cols_k <= 2^22, 0 <= col0_k, col0_k + ncols <= cols_k; the window, order_host, ws and every other limit:
 * crw_labelmap_ordered's with cols = ncols -- all refused (CRW_EINVAL) before anything is launched.  One launch, the ordered
 * kernel's shape: a lane per column, a wave per 64 columns; plain vector stores, no atomics, bit-reproducible. */
int crw_labelmap_ordered_joint(const float *La, int Ta, int cols_a, int col0_a, int flip_a, const float *Lb, int Tb, int cols_b,
                               int col0_b, int flip_b, int N, int M, int rows, int ncols, const int *order_host, int S,
                               int conf_kind, void *labels, int label_dtype, float *conf, size_t ld, void *ws, size_t ws_bytes,
                               crw_stream_t stream);
/* crw_labelmap_ordered_joint for the G configurations of a sweep in ONE launch: L_k [G, T_k*N, M], configuration g's windows at
 * labels + g * map_stride and conf + g * map_stride as for crw_labelmap_ordered_batch, one order and one geometry for all.  Slice g
 * is bit-identical to crw_labelmap_ordered_joint(La + g*Ta*N*M, ..., Lb + g*Tb*N*M, ...) written into the same window. */
int crw_labelmap_ordered_joint_batch(const float *La, int Ta, int cols_a, int col0_a, int flip_a, const float *Lb, int Tb, int cols_b,
                                     int col0_b, int flip_b, int G, int N, int M, int rows, int ncols, const int *order_host, int S,
                                     int conf_kind, void *labels, int label_dtype, float *conf, size_t ld, size_t map_stride,
                                     void *ws, size_t ws_bytes, crw_stream_t stream);

/* Posterior confidence and horizon error bars of an ordered map: the order constraint that defines the decode, read as a
 * distribution.  Per output column, with e[r][s] EXACTLY the evidence crw_labelmap_ordered decodes (the same device functions;
 * order, S, flip and the windows as there) and f[r][s] = max(e[r][s], floor), 2^-20 <= floor <= 0.25 (seed frames are one-hot, L
 * holds exact zeros): a path x is monotone, x_0 <= ... <= x_{rows-1} over the states 0 ... S-1, starts and ends anywhere, weighs
 * W(x) = prod_r f[r][x_r], and P(x) = W(x) / sum W.  gamma[r][s] = P(x_r = s).  For k = 1 ... S-1 the boundary B_k is the first
 * row with x_r >= k, `rows` if there is none: P(B_k <= r) = sum_{s >= k} gamma[r][s].
 *   post[r][c]     = gamma[r][pos(label[r][c])], pos the position in `order`; the labels are an INPUT (the window a decode wrote,
 *                    label_dtype CRW_DT_I8 or CRW_DT_F32, pitch ld, never written); a label outside `order` gives 0.  In [0, 1].
 *   hz[0][k-1][c]  = b^_k, the pick: the first row whose label's position is >= k, `rows` if none (an integer held in fp32)
 *   hz[1][k-1][c]  = E[B_k]
 *   hz[2][k-1][c]  = sqrt(E[(B_k - b^_k)^2]), the error bar of the pick, centred on the pick
 * post: a [rows] x [cols] window of pitch ld (the labels' pitch); hz: fp32 [3][S-1] rows of cols values, row q*(S-1) + k-1 at
 * hz + (q*(S-1) + k-1) * hz_ld, hz_ld >= cols -- the column window of a [3, S-1, width] tensor.  Either may be NULL, not both.
 * Arithmetic, fp32, forward-backward down the column, rescaled every row, contraction off, prefix sums upwards from state 0, suffix
 * sums downwards from state S-1:
 *   a[0][s] = f[0][s];  a[r][s] = f[r][s] * sum_{s' <= s} A[r-1][s'];  A[r][s] = a[r][s] * (1 / sum_s a[r][s])
 *   b[rows-1][s] = 1;   b[r-1][s] = sum_{s' >= s} f[r][s'] * (b[r][s'] * (1 / b[r][0]))  (b[r][0] is b[r]'s largest entry)
 *   gamma[r][s] = A[r][s] b[r][s] * (1 / Z_r),  Z_r = sum_s A[r][s] b[r][s]
 *   P(B_k = r+1) = ((sum_{s < k} A[r][s]) * b[r][k]) * (1 / Z_r)  (r = rows-1: the boundary is absent);  P(B_k = 0) = sum_{s >= k} gamma[0][s]
 *   E[B_k] = sum_r (r+1) P(B_k = r+1);  E[(B_k - b^_k)^2] = sum_r (r+1 - b^_k)^2 P(B_k = r+1) + b^_k^2 P(B_k = 0), rows bottom to top.
 * Every output is a sum of products of non-negative numbers.  A column whose evidence contradicts `order` over some 126 / log2(1 /
 * floor) rows in a row can underflow fp32 (Z_r < 2^-126): its gamma and boundary terms of that row read 0, never NaN.
 * ws: crw_labelmap_posterior_workspace(rows, cols, S) bytes (4 * rows * S * cols rounded up to 64 columns; 0 for a bad shape), 4-byte
 * aligned, the normalised forward messages [row][state][column]; what it held before is never read.  Every limit and refusal of
 * crw_labelmap_ordered applies (CRW_EINVAL); in addition floor out of range (a NaN included), both outputs NULL, post / hz / ws
 * unaligned, hz_ld < cols -> CRW_EINVAL; too few bytes -> CRW_EWORKSPACE; all before anything is launched.  One launch, a lane per
 * column, a wave per 64 columns, two scans of `rows` steps in series; plain vector stores, no atomics, bit-reproducible. */
size_t crw_labelmap_posterior_workspace(int rows, int cols, int S);
int crw_labelmap_ordered_posterior(const float *L, int T, int N, int M, int rows, int cols, int flip, const int *order_host, int S,
                                   float floor, const void *labels, int label_dtype, size_t ld, float *post, float *hz, size_t hz_ld,
                                   void *ws, size_t ws_bytes, crw_stream_t stream);
/* The same posterior over crw_labelmap_ordered_joint's evidence: e[r][s] = (took ? v_b : v_a)[order[s]], took = conf_b > conf_a on
 * the dense confidences of conf_kind (mandatory), the sources and the window as there (cols = ncols).  One kernel text and one
 * text per scan step serve both entry points: with both sources the same tensor and geometry (a tie keeps source a) the outputs
 * equal crw_labelmap_ordered_posterior's bit for bit.  Refusals: crw_labelmap_ordered_joint's and the posterior's. */
int crw_labelmap_ordered_joint_posterior(const float *La, int Ta, int cols_a, int col0_a, int flip_a, const float *Lb, int Tb,
                                         int cols_b, int col0_b, int flip_b, int N, int M, int rows, int ncols, const int *order_host,
                                         int S, int conf_kind, float floor, const void *labels, int label_dtype, size_t ld,
                                         float *post, float *hz, size_t hz_ld, void *ws, size_t ws_bytes, crw_stream_t stream);
/* The two posteriors for the G configurations of a sweep in ONE launch (the configuration is a grid dimension of the same kernel;
 * the one-map calls are G = 1 of the same launcher): L / La / Lb [G, T*N, M] as for crw_labelmap_ordered_batch / _joint_batch.
 * Configuration g reads its labels at labels + g * map_stride (elements of the label type) and writes post + g * map_stride, its
 * [3][S-1] rows of hz at hz + g * hz_stride, and uses slice g of ws (crw_labelmap_posterior_workspace_batch(G, rows, cols, S) bytes:
 * G times the one-map call's, 0 for a bad shape or a product that does not fit a size_t) -- so maps[:, :, a:b] of [G, rows, width]
 * tensors and hz[:, :, :, a:b] of a [G, 3, S-1, width] tensor are valid operands.  One order, one floor and one geometry serve all
 * configurations.  Slice g is bit-identical to the one-map entry point called on slice g's operands and the same window.  Every
 * refusal of the one-map calls applies; in addition G < 1 (or > 65535), map_stride < (rows - 1) * ld + cols, hz_stride < 3 * (S - 1) *
 * hz_ld when hz is given, and slices whose extent overflows a size_t -> CRW_EINVAL; too few workspace bytes -> CRW_EWORKSPACE; all
 * before anything is launched. */
size_t crw_labelmap_posterior_workspace_batch(int G, int rows, int cols, int S);
int crw_labelmap_ordered_posterior_batch(const float *L, int G, int T, int N, int M, int rows, int cols, int flip,
                                         const int *order_host, int S, float floor, const void *labels, int label_dtype, size_t ld,
                                         size_t map_stride, float *post, float *hz, size_t hz_ld, size_t hz_stride, void *ws,
                                         size_t ws_bytes, crw_stream_t stream);
int crw_labelmap_ordered_joint_posterior_batch(const float *La, int Ta, int cols_a, int col0_a, int flip_a, const float *Lb, int Tb,
                                               int cols_b, int col0_b, int flip_b, int G, int N, int M, int rows, int ncols,
                                               const int *order_host, int S, int conf_kind, float floor, const void *labels,
                                               int label_dtype, size_t ld, size_t map_stride, float *post, float *hz, size_t hz_ld,
                                               size_t hz_stride, void *ws, size_t ws_bytes, crw_stream_t stream);

/* building blocks exported for tests and the roofline bench --------------------------------- */
/* Weight gradient of the CNN encoder's linear head (nn.Linear(128, 128), src/encoder.py:40,55; autograd of
 * src/model.py:20): dw[o][i] = sum_p dy[p][o] x[p][i] as P/128 batched 128x128 fp32-MFMA products whose partial matrices
 * are added in a fixed order (a library GEMM runs this M=N=128, K=P shape on 16 workgroups).  P % 128 == 0. */
size_t crw_linear128_wgrad_ws_bytes(int P);
int crw_linear128_wgrad(const float *dy, const float *x, float *dw, int P, void *ws, size_t ws_bytes, crw_stream_t stream);

/* One Adam step (torch.optim.Adam defaults: no weight decay, no amsgrad -- the reference's optimizer, scripts/train.py:54,69) on a
 * flat fp32 parameter buffer p[n] with gradient g[n] and moment buffers m[n], v[n] (all 16-byte aligned); step = 1, 2, ...
 * Operation for operation the arithmetic of torch's default implementation; the host side keeps the module's parameters as views
 * of p (radar-sounder-crw_amd/optim.py) and the gradients as views of g (dist.FlatGradBucket). */
int crw_adam_step(float *p, const float *g, float *m, float *v, long n, float lr, float beta1, float beta2, float eps, int step,
                  crw_stream_t stream);

/* X [batch,n,n] (n multiple of 32, zero padded): C = op(A) * op(B) (+ C if beta), fp32 MFMA. */
int crw_gemm_f32(const float *A, const float *B, float *C, int n, int batch, int transA, int transB,
                 int beta, crw_stream_t stream);

/* encoder: hand-written 3x3 convolutions of CNN (conv3/conv4/conv5, src/encoder.py:26-35) --------- */
/* Activations are channels-last bf16 planes [P][100][C] ("hi" plane and, for split = 3, a "lo"
 * plane: x = hi + lo to ~1e-5 relative).  10x10 feature maps (16x16 input patches).
 * fp32 conv weight [cout][cin][3][3] -> forward planes and backward-data planes (taps flipped, cin <-> cout),
 * 9*cout*cin bf16 each, stored in MFMA fragment order (opaque to the caller); lo planes may be NULL
 * together (plain bf16). */
int crw_enc_pack_weights(const float *w, int cout, int cin, uint16_t *fwd_hi, uint16_t *fwd_lo,
                         uint16_t *bwd_hi, uint16_t *bwd_lo, crw_stream_t stream);
/* fp32 NCHW [P][C][10][10] (output of pool2) -> planes */
int crw_enc_pack_input(const float *x, int P, int C, uint16_t *x_hi, uint16_t *x_lo, crw_stream_t stream);
/* same for feature maps of any size: fp32 NCHW [P][C][H][W] -> planes [P][H*W][C] */
int crw_enc_pack_input_map(const float *x, int P, int C, int H, int W, uint16_t *x_hi, uint16_t *x_lo,
                           crw_stream_t stream);
/* mode 0: y = relu(conv3x3(x, w) + bias), optional gap[P][cout] = mean over pixels (AdaptiveAvgPool2d(1));
 * mode 1: backward-data, y = conv3x3(x = dY, w = backward planes), zeroed where mask_hi (the forward
 *         activation of the layer below, [P][100][cout]) is 0; bias ignored.
 * (cin, cout) in {(32,64),(64,128),(128,128),(128,64),(64,32)}.  Outputs: planes y_hi/y_lo and/or
 * y_f32 [P][100][cout] (fp32); y_lo may be NULL when only the hi plane of the result is needed.
 * gap (and gap_part of crw_enc_conv3x3_map) is produced by the kernels in which one wave owns all pixels of its channels: cout = 128
 * (every split), cout = 64 at split 1; any other request for it is refused with CRW_EINVAL before anything is launched -- never
 * CRW_OK with gap left unwritten.  Outputs are complete in stream order; what they held before is never read.
 * dgap (mode 1 only, may be NULL): fused ReLU + global-average-pool backward -- the input gradient
 * is dgap[P][cin] / 100 where x_hi (then the FORWARD activation plane of that layer) is non-zero;
 * x_lo is ignored. */
int crw_enc_conv3x3(int mode, int split, int P, int cin, int cout, const uint16_t *x_hi, const uint16_t *x_lo,
                    const uint16_t *w_hi, const uint16_t *w_lo, const float *bias, const uint16_t *mask_hi,
                    uint16_t *y_hi, uint16_t *y_lo, float *y_f32, float *gap, const float *dgap,
                    crw_stream_t stream);
/* The 3x3 layers on feature maps of ANY size (patch sizes other than 16x16; src/encoder.py:49-53 is size-agnostic):
 * planes are [P][H][W][C]; a workgroup computes one 10x10 output tile from the 12x12 window around it (zeros outside
 * the map).  mode 0: relu(conv + bias); y_hi/y_lo may be NULL when only the pooled result is wanted; gap_part
 * [P * ceil(H/10) * ceil(W/10)][cout] receives per-tile SUMS over the in-map pixels (the caller adds the tiles and
 * divides by H*W = AdaptiveAvgPool2d(1)).  mode 1: backward-data (w = the backward planes of crw_enc_pack_weights,
 * cin/cout swapped), output zeroed where mask_hi (activation map of the layer below, may be NULL) is 0; y_f32
 * (may be NULL): fp32 copy of the output [P][H][W][cout]. */
int crw_enc_conv3x3_map(int mode, int split, int P, int H, int W, int cin, int cout, const uint16_t *x_hi, const uint16_t *x_lo,
                        const uint16_t *w_hi, const uint16_t *w_lo, const float *bias, const uint16_t *mask_hi,
                        uint16_t *y_hi, uint16_t *y_lo, float *y_f32, float *gap_part, crw_stream_t stream);
/* weight / bias gradient of one 3x3 layer on feature maps of any size (autograd of src/encoder.py:49-53 at other patch
 * sizes): dY [P][H][W][cout], X [P][H][W][cin] planes -> dw [cout][cin][3][3], db [cout].
 * ws: crw_enc_wgrad_ws_bytes(P * ceil(H/10) * ceil(W/10), cin, cout, split). */
int crw_enc_conv3x3_wgrad_map(int split, int P, int H, int W, int cin, int cout, const uint16_t *dy_hi, const uint16_t *dy_lo,
                              const uint16_t *x_hi, const uint16_t *x_lo, float *dw, float *db, void *ws, size_t ws_bytes,
                              crw_stream_t stream);
/* dY planes [P][npix][C] = dgap[P][C] / npix where y_hi != 0 (backward of ReLU + global average pool; npix = 100 for
 * 16x16 patches, H*W of the conv3-5 feature map otherwise) */
int crw_enc_gap_bwd(const float *dgap, const uint16_t *y_hi, int P, int C, int npix, uint16_t *dy_hi, uint16_t *dy_lo,
                    crw_stream_t stream);
/* dw [cout][cin][3][3], db [cout] (fp32, overwritten) from dY planes [P][100][cout] and x planes [P][100][cin].
 * Per-slice partial sums go to `ws` (crw_enc_wgrad_ws_bytes) and are added in a fixed order:
 * no float atomics, bitwise reproducible.  dgap (may be NULL): as in crw_enc_conv3x3, dY = dgap/100
 * gated by dy_hi (= forward activation plane); dy_lo ignored. */
size_t crw_enc_wgrad_ws_bytes(int P, int cin, int cout, int split);
int crw_enc_conv3x3_wgrad(int split, int P, int cin, int cout, const uint16_t *dy_hi, const uint16_t *dy_lo,
                          const uint16_t *x_hi, const uint16_t *x_lo, const float *dgap, float *dw, float *db,
                          void *ws, size_t ws_bytes, crw_stream_t stream);

/* encoder front end: conv1 5x5 -> ReLU -> maxpool 2x2/1 -> conv2 5x5 -> ReLU -> maxpool 2x2/1, fused
 * (src/encoder.py:13-24,46-47; 16x16 patches, cin = 1 or 2 with pos_embed) -------------------------- */
/* conv2 weight [32][8][5][5] fp32 -> forward planes [7][32][32] and backward planes [25][8][32] */
int crw_enc_front_pack(const float *w2, uint16_t *fwd_hi, uint16_t *fwd_lo, uint16_t *bwd_hi, uint16_t *bwd_lo,
                       crw_stream_t stream);
/* x [P][cin][16][16] fp32 -> planes [P][100][32] (input of crw_enc_conv3x3 cin = 32).
 * saved (may be NULL; training): crw_enc_front_saved_bytes(P) bytes that receive, per patch, the pool1 output planes and one
 * code byte per pooling window (arg-max position + ReLU gate); crw_enc_front_bwd then needs no recomputation. */
size_t crw_enc_front_saved_bytes(int P);
int crw_enc_front_fwd(int split, const float *x, int P, int cin, const float *w1, const float *b1,
                      const uint16_t *w2_hi, const uint16_t *w2_lo, const float *b2, uint16_t *y_hi,
                      uint16_t *y_lo, void *saved, crw_stream_t stream);
/* The same front end on patches of any size h, w >= 7 (forward only, inference): x [P][cin][H][W] -> planes
 * [P][(H-6)*(W-6)][32] that feed crw_enc_conv3x3_map.  Work item = (patch, 10x10 tile of the output map). */
int crw_enc_front_fwd_map(int split, const float *x, int P, int cin, int H, int W, const float *w1, const float *b1,
                          const uint16_t *w2_hi, const uint16_t *w2_lo, const float *b2, uint16_t *y_hi, uint16_t *y_lo,
                          crw_stream_t stream);
/* backward: dy [P][100][32] fp32 -> dw1 [8][cin][5][5], db1 [8], dw2 [32][8][5][5], db2 [32]; partial sums per patch
 * slice in `ws`, added in a fixed order.  saved: the record crw_enc_front_fwd wrote for these patches, or NULL (the kernel
 * then recomputes conv1 -> pool1 -> conv2 per patch; same results, ~40 % more time). */
size_t crw_enc_front_ws_bytes(int P, int cin);
int crw_enc_front_bwd(int split, const float *x, int P, int cin, const float *w1, const float *b1,
                      const uint16_t *w2_hi, const uint16_t *w2_lo, const float *b2, const uint16_t *w2b_hi,
                      const uint16_t *w2b_lo, const float *dy, const void *saved, float *dw1, float *db1, float *dw2,
                      float *db2, void *ws, size_t ws_bytes, crw_stream_t stream);

/* The same backward on patches of any size h, w >= 7 (training at patch sizes other than 16x16): x [P][cin][H][W], dy
 * [P][H-6][W-6][32] fp32 = gradient of the planes of crw_enc_front_fwd_map.  Unit of work = (patch, 10x10 tile of that map);
 * ws: crw_enc_front_ws_bytes(P * ceil((H-6)/10) * ceil((W-6)/10), cin). */
int crw_enc_front_bwd_map(int split, const float *x, int P, int cin, int H, int W, const float *w1, const float *b1,
                          const uint16_t *w2_hi, const uint16_t *w2_lo, const float *b2, const uint16_t *w2b_hi,
                          const uint16_t *w2b_lo, const float *dy, float *dw1, float *db1, float *dw2, float *db2,
                          void *ws, size_t ws_bytes, crw_stream_t stream);

/* Resnet encoder (the reference's default model: src/encoder.py:63-89 stem, :109-155 BasicBlock, :157-272 body), forward AND
 * backward on hand-written kernels ----------------------------------------------------------------------------------------
 * Conventions of this group.  Ppad = crw_rn_padded_patches(P) (P rounded up to 128).  "planes" are channels-last bf16 pairs
 * (hi, lo; x = hi + lo) of shape [Ppad][pixels][C] whose rows P..Ppad-1 are ZERO; raw convolution outputs are fp32
 * [Ppad][pixels][C].  Every convolution runs as a matrix product ACROSS PATCHES (tile = 128 patches x 64/128 channels, one
 * group per output pixel, reduction over the kernel taps that fall inside the map) on v_mfma_f32_16x16x32_bf16 with hi/lo
 * operand pairs (3 products, fp32 accumulate).  Train-mode BatchNorm (nn.BatchNorm2d defaults) is split into: per-tile
 * column statistics from the convolution's epilogue -> crw_rn_bn_stats -> crw_rn_bn_apply / crw_rn_bn_pool; backward
 * crw_rn_bn_bwd / crw_rn_pool_bwd.  A BatchNorm's coefficients travel as coef[4][C] = scale, shift, mean, invstd. */
int crw_rn_padded_patches(int P);
/* conv weight [cout][cin][kh][kw] fp32 -> forward planes [cout][kh*kw][cin] and backward-data planes [cin][kh*kw][cout] */
int crw_rn_pack_conv(const float *w, int cout, int cin, int kh, int kw, uint16_t *fwd_hi, uint16_t *fwd_lo, uint16_t *bwd_hi,
                     uint16_t *bwd_lo, crw_stream_t stream);
/* stem convolution model.conv1 [64][3][7][7] (src/encoder.py:185) for h x w patches: forward planes [64][256] and the Toeplitz
 * planes [(h+2)][crw_rn_stem_cols(w)][crw_rn_stem_toeplitz_ld(w)] of its backward-data product.  crw_rn_stem_cols(w) = 3 * (w + 2)
 * rounded up to 64: the columns (ix * 3 + c) of one row of the stem's input gradient -- any patch width. */
int crw_rn_stem_toeplitz_ld(int w);
int crw_rn_stem_cols(int w);
int crw_rn_pack_stem(const float *w1, int h, int w, uint16_t *fwd_hi, uint16_t *fwd_lo, uint16_t *toep_hi, uint16_t *toep_lo,
                     crw_stream_t stream);
/* mode 0: forward of conv2d(kh x kw, stride, pad, no bias) -- a = input planes [Ppad][Hs*Ws][Cs], b = forward weight planes,
 *         out fp32 [Ppad][Hd*Wd][N] (N = cout);  a linear layer is the 1x1 case on a 1x1 map (bias: optional [N]).
 * mode 1: backward-data -- a = dZ planes on the OUTPUT map [Ppad][Hs*Ws][Cs] (Cs = cout), b = backward planes,
 *         out = gradient on the input map [Ppad][Hd*Wd][N] (N = cin).
 * mode 2: stem forward (7x7, stride 2) -- a = the zero-padded 4-channel map of crw_rn_stem_fwd [Ppad][Hs][Ws][4], b = forward
 *         stem planes, out [Ppad][Hd*Wd][64].
 * mode 3: stem backward-data -- a = dZ planes [Ppad][Hs*Ws][64], b = Toeplitz planes, N = crw_rn_stem_cols(w), out [Ppad][Hd][N]:
 *         row iy holds the gradient of the (h+2) x (w+2) map at (iy, ix), channel c in column ix * 3 + c.
 * part (may be NULL): crw_rn_conv_part_floats(P, Hd*Wd, N) floats of per-tile column sums / sums of squares for crw_rn_bn_stats. */
size_t crw_rn_conv_part_floats(int P, int G, int N);
int crw_rn_conv(int mode, int P, int Hs, int Ws, int Cs, int Hd, int Wd, int N, int kh, int kw, int stride, int pad,
                const uint16_t *a_hi, const uint16_t *a_lo, const uint16_t *b_hi, const uint16_t *b_lo, const float *bias, float *out,
                float *part, crw_stream_t stream);
/* weight gradient dw [cout][cin][kh][kw] (fp32, overwritten) from the input planes x [Ppad][Hin*Win][Cin] and the dZ planes
 * [Ppad][Hout*Wout][Cout]; mode 0 = convolution / linear layer, mode 2 = stem (x = the 4-channel map, Hin x Win = its size,
 * Cin = 4; dw = [64][3][7][7]).  Reduction over patches in slices, partial slabs in ws added in a fixed order. */
size_t crw_rn_wgrad_ws_bytes(int mode, int P, int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int kh, int kw, int stride, int pad);
int crw_rn_wgrad(int mode, int P, int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int kh, int kw, int stride, int pad,
                 const uint16_t *x_hi, const uint16_t *x_lo, const uint16_t *d_hi, const uint16_t *d_lo, float *dw, void *ws,
                 size_t ws_bytes, crw_stream_t stream);
/* batch statistics of a convolution output with G pixels per patch from its `part` -> coef[4][C]; run_mean / run_var (may be
 * NULL together) are updated like nn.BatchNorm2d in train mode (momentum on the batch mean and the unbiased batch variance) */
size_t crw_rn_bn_stats_ws_bytes(int C);
int crw_rn_bn_stats(const float *part, int P, int G, int C, const float *gamma, const float *beta, float *run_mean, float *run_var,
                    float momentum, float eps, float *coef, void *ws, size_t ws_bytes, crw_stream_t stream);
/* the same from `rows` partial rows [rows][C] of (sum, sum of squares) over `count` samples per channel (crw_rn_stem16_fwd's) */
int crw_rn_bn_stats_rows(const float *part, int rows, double count, int C, const float *gamma, const float *beta, float *run_mean,
                         float *run_var, float momentum, float eps, float *coef, void *ws, size_t ws_bytes, crw_stream_t stream);
/* y planes = relu?( Z * scale + shift [+ Zd * scale_d + shift_d] [+ residual planes] )   (src/encoder.py:138-153) */
int crw_rn_bn_apply(const float *Z, const float *coef, const float *Zd, const float *coef_d, const uint16_t *res_hi,
                    const uint16_t *res_lo, int P, int npix, int C, int relu, uint16_t *y_hi, uint16_t *y_lo, crw_stream_t stream);
/* y planes [Ppad][Ho*Wo][C] = maxpool3x3/2/1( relu( Z * scale + shift ) ), Z on an H x W map   (src/encoder.py:257-260);
 * amax (may be NULL; [Ppad][Ho*Wo][C] bytes): position ky * 3 + kx of the first maximum of every window (ATen's rule), for the
 * backward pass */
int crw_rn_bn_pool(const float *Z, const float *coef, int P, int H, int W, int C, uint16_t *y_hi, uint16_t *y_lo, uint8_t *amax,
                   crw_stream_t stream);
/* backward of y = relu(bn(Z) [+ bn_d(Zd)] [+ identity]): g = (g1 [+ g2]) where mask_hi (the hi plane of y) is non-zero;
 * dz planes = gradient of Z, dzd planes = gradient of Zd, g_out (may be NULL) = g in fp32 (the identity shortcut's share),
 * dgamma / dbeta [C] (and the shortcut BatchNorm's). */
size_t crw_rn_bn_bwd_ws_bytes(int P, int npix, int C);
int crw_rn_bn_bwd(const float *g1, const float *g2, const uint16_t *mask_hi, const float *Z, const float *coef, const float *Zd,
                  const float *coef_d, int P, int npix, int C, uint16_t *dz_hi, uint16_t *dz_lo, uint16_t *dzd_hi, uint16_t *dzd_lo,
                  float *g_out, float *dgamma, float *dbeta, float *dgamma_d, float *dbeta_d, void *ws, size_t ws_bytes,
                  crw_stream_t stream);
/* backward of crw_rn_bn_pool: d1 (+ d2, may be NULL) = gradient of the pooled map [Ppad][Ho*Wo][C] fp32, amax = the codes the
 * forward recorded -> dz planes [Ppad][H*W][C], dgamma / dbeta of that BatchNorm */
size_t crw_rn_pool_bwd_ws_bytes(int P, int H, int W, int C);
int crw_rn_pool_bwd(const float *d1, const float *d2, const uint8_t *amax, const float *Z, const float *coef, int P, int H, int W, int C,
                    uint16_t *dz_hi, uint16_t *dz_lo, float *dgamma, float *dbeta, void *ws, size_t ws_bytes, crw_stream_t stream);
/* stem: relu0(bn0(fc0(x))) with fc0 = Conv2d(cin, 3, 1, padding 1) (src/encoder.py:66-74,87): x [P][cin][h][w] -> the map planes
 * [Ppad][Hm][Wm][4] that feed the stem convolution (the (h+2) x (w+2) map at offset (3,3), zero elsewhere, channel 3 = 0);
 * bn0's batch statistics follow from the moments of x.  stem [32] floats = the record crw_rn_stem_bwd needs. */
size_t crw_rn_stem_ws_bytes(void);
int crw_rn_stem_fwd(const float *x, int P, int cin, int h, int w, int Hm, int Wm, const float *w0, const float *b0, const float *gamma,
                    const float *beta, float *run_mean, float *run_var, float momentum, float eps, uint16_t *map_hi, uint16_t *map_lo,
                    float *stem, void *ws, size_t ws_bytes, crw_stream_t stream);
/* dX0 = out of crw_rn_conv mode 3 -> dw0 [3][cin], db0 [3], dgamma0 [3], dbeta0 [3] */
int crw_rn_stem_bwd(const float *dX0, const float *x, const float *stem, const float *w0, const float *b0, int P, int cin, int h, int w,
                    float *dw0, float *db0, float *dgamma, float *dbeta, void *ws, size_t ws_bytes, crw_stream_t stream);
/* The stem for 16 x 16 patches, one PATCH per wave (what crw_rn_train_* use at that size; csrc/resnet_stem.hip): the map
 * relu0(bn0(fc0(x))) is rebuilt from the 1 KB patch inside each kernel (LDS image), the 7 x 7 weights live in LDS in MFMA fragment
 * order, and the backward-data pass never writes the gradient map -- only the sums bn0 / fc0 need leave it.
 *   crw_rn_stem_stats   : bn0's batch statistics (from the moments of x) -> stem[32] record (+ running statistics)
 *   crw_rn_pack_stem16  : model.conv1.weight [64][3][7][7] -> forward / transposed fragment packs (28672 bf16 each)
 *   crw_rn_stem16_fwd   : Z1 [P][81][64] fp32 + crw_rn_stem16_rows() partial rows [64] of (sum, sum of squares) for crw_rn_bn_stats_rows
 *   crw_rn_stem16_wgrad : dz planes [P][81][64] (gradient of Z1) -> dw1 [64][3][7][7]
 *   crw_rn_stem16_bwd   : dz planes -> dw0 [3][cin], db0 [3], dgamma0 [3], dbeta0 [3]
 * ws of the last two: crw_rn_stem16_ws_bytes(); of crw_rn_stem_stats: crw_rn_stem_ws_bytes(). */
int crw_rn_stem_stats(const float *x, int P, int cin, int h, int w, const float *w0, const float *b0, const float *gamma, const float *beta,
                      float *run_mean, float *run_var, float momentum, float eps, float *stem, void *ws, size_t ws_bytes,
                      crw_stream_t stream);
int crw_rn_stem16_rows(void);
int crw_rn_pack_stem16(const float *w1, uint16_t *wf, uint16_t *wt, crw_stream_t stream);
int crw_rn_stem16_fwd(const float *x, int P, int cin, const float *stem, const uint16_t *wf, float *Z1, float *part, crw_stream_t stream);
/* The same forward product for patches of ANY size (what crw_rn_train_fwd / crw_rn_eval_fwd use beyond 16 x 16, e.g. the 32 x 32
 * patches of scripts/test/test_mc1.py:19): a BAND of output rows per wave, the map rows it reads rebuilt from the patch in LDS.
 * Z1 [P][H1 * W1][64] fp32 (H1, W1 = the 7x7/2 output of the (h+2) x (w+2) map), part as crw_rn_stem16_fwd's.
 * crw_rn_stem_band_ok: 1 when the geometry is covered (output rows of at most 96 pixels, band image within the LDS), else 0 --
 * then mode 2 of crw_rn_conv on the crw_rn_stem_fwd map planes is the way. */
int crw_rn_stem_band_ok(int h, int w);
int crw_rn_stem_band_fwd(const float *x, int P, int cin, int h, int w, const float *stem, const uint16_t *wf, float *Z1, float *part,
                         crw_stream_t stream);
size_t crw_rn_stem16_ws_bytes(void);
int crw_rn_stem16_wgrad(const float *x, int P, int cin, const float *stem, const uint16_t *dz_hi, const uint16_t *dz_lo, float *dw, void *ws,
                        size_t ws_bytes, crw_stream_t stream);
int crw_rn_stem16_bwd(const float *x, int P, int cin, const float *stem, const float *w0, const float *b0, const uint16_t *wt,
                      const uint16_t *dz_hi, const uint16_t *dz_lo, float *dw0, float *db0, float *dgamma, float *dbeta, void *ws,
                      size_t ws_bytes, crw_stream_t stream);
/* fp32 [P][C] -> planes [Ppad][C] */
int crw_rn_split(const float *x, int P, int C, uint16_t *hi, uint16_t *lo, crw_stream_t stream);
/* out [C] = column sums of x [rows][C] (bias gradient of the head), fixed order */
size_t crw_rn_colsum_ws_bytes(int C);
int crw_rn_colsum(const float *x, int rows, int C, float *out, void *ws, size_t ws_bytes, crw_stream_t stream);

/* The whole encoder from native code: one call runs every launch of the forward (backward) pass on one workspace -- what the
 * host modules use (resnet_hip.py); the entry points above remain as the building blocks the tests exercise one by one.
 * Patches x [P][cin][h][w] of any size (cin = 1, or 2 with pos_embed); 16 x 16 -- the reference's default, scripts/train.py:24 --
 * takes the patch-per-wave stem kernels, other sizes (32 x 32: scripts/test/test_mc1.py:19) the gathered stem products, and where
 * layer4's map has more than one pixel the global average pool + linear head (src/encoder.py:264-266) run as one product over
 * that map.  prm / grads: the CRW_RN_NPARAM parameter tensors (gradients) in
 * nn.Module.named_parameters() order -- fc0.weight, fc0.bias, bn0.weight, bn0.bias, model.conv1.weight, model.bn1.{weight,bias},
 * model.layer{1..4}.0.{conv1.weight, bn1.weight, bn1.bias, conv2.weight, bn2.weight, bn2.bias [, downsample.0.weight,
 * downsample.1.weight, downsample.1.bias]}, model.fc.weight, model.fc.bias; run_mean / run_var (NULL together: not updated): the
 * CRW_RN_NBN BatchNorm buffers in module order (bn0, model.bn1, then per layer bn1, bn2 [, downsample.1]).
 * ws: crw_rn_train_ws_bytes; crw_rn_train_bwd needs the workspace exactly as crw_rn_train_fwd left it (activations, statistics,
 * packed weights) and the same x / prm.  out [P][128] fp32. */
#define CRW_RN_NPARAM 42
#define CRW_RN_NBN 13
size_t crw_rn_train_ws_bytes(int P, int cin, int h, int w);
int crw_rn_train_fwd(const float *x, int P, int cin, int h, int w, const float *const *prm, float *const *run_mean,
                     float *const *run_var, float momentum, float eps, float *out, void *ws, size_t ws_bytes, crw_stream_t stream);
int crw_rn_train_bwd(const float *dout, const float *x, int P, int cin, int h, int w, const float *const *prm, float *const *grads,
                     void *ws, size_t ws_bytes, crw_stream_t stream);
/* crw_rn_train_fwd when NO backward pass follows (the reference's test scripts: train-mode BatchNorm under torch.no_grad(),
 * scripts/test/test_mc1.py:40-46 with src/utils.py:108): same out, same running-statistics update; what only crw_rn_train_bwd
 * would read (the stem's map planes and Toeplitz weight packs at patch sizes other than 16 x 16) is not produced -- the workspace
 * must NOT be handed to crw_rn_train_bwd afterwards. */
int crw_rn_train_fwd_nograd(const float *x, int P, int cin, int h, int w, const float *const *prm, float *const *run_mean,
                            float *const *run_var, float momentum, float eps, float *out, void *ws, size_t ws_bytes, crw_stream_t stream);
/* The same forward with every BatchNorm in EVAL mode (nn.Module.eval(): normalise by the running statistics, update nothing) --
 * what the reference's scripts/test/test.py:42 runs before utils.propagate.  ws: crw_rn_train_ws_bytes. */
int crw_rn_eval_fwd(const float *x, int P, int cin, int h, int w, const float *const *prm, const float *const *run_mean,
                    const float *const *run_var, float eps, float *out, void *ws, size_t ws_bytes, crw_stream_t stream);
/* Diagnostic (bench.py's in-step roofline; the one stateful corner of the library, not thread-safe): while enabled, every
 * matrix-core launch of crw_rn_train_fwd / _bwd is bracketed by two HIP events on the launch stream.  After synchronising the
 * stream, crw_rn_timing_read fills up to `max` records in launch order and returns how many were taken; enable(…) resets.
 * kind 0 = crw_rn_conv (g = Hs, Ws, Cs, Hd, Wd, N), kind 1 = crw_rn_wgrad incl. its slab sum (g = Hin, Win, Cin, Hout, Wout, Cout). */
typedef struct {
  int kind, mode, g[6], k, stride, pad;
  float ms;
} crw_rn_timing_rec;
int crw_rn_timing_enable(int on);
int crw_rn_timing_read(crw_rn_timing_rec *out, int max);

/* bf16 matrix-core variant of the chain GEMM.  A, B fp32 [batch,n,n] (n multiple of 128) are first
 * converted into bf16 images inside `ws` (convert != 0; pass 0 to reuse the images of the previous
 * call, e.g. when timing the GEMM alone).  split = 1: plain bf16 operands; split = 3: hi/lo operand
 * pairs, Ah*Bh + Ah*Bl + Al*Bh, fp32-grade result.  C fp32. */
size_t crw_gemm_bf16_ws_bytes(int n, int batch, int split);
int crw_gemm_bf16(const float *A, const float *B, float *C, int n, int batch, int transA, int transB,
                  int beta, int split, void *ws, size_t ws_bytes, int convert, crw_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CRW_HIP_H */
