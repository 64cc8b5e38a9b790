/* A guarded Adam step: crw_adam_step that refuses a poisoned gradient and bounds a step's size, decided on the device.  A companion
 * of crw_hip.h (same conventions, same status codes, same CRW_ABI_VERSION).  Added at ABI 8 without a bump: a library built before it
 * still loads, the binding tells by symbol (crw_hip.has_guard()).  The binding mirrors this header in crw_hip.GUARD_SIGNATURES;
 * tests/test_guard_host.py holds the two and the library against each other, tests/guard_ref.py restates the rule as plain loops and
 * tests/test_guard_gpu.py runs the entry point over stale memory and between guard bands.
 *
 * THE RULE.  p, g, m, v [n] fp32 as crw_adam_step takes them; step = the number of calls including this one (the host keeps it).
 *   norm ...... ss = sum over i of (double)g[i]^2 and norm = sqrt(ss).  The order of the sum is fixed by n alone: block b owns the
 *               elements [b * 4096, (b + 1) * 4096), thread t of 256 adds the squares of its float4 j * 256 + t, j = 0 .. 3, in
 *               element order into one fp64 accumulator, the 256 accumulators are joined by a halving tree, and the per-block
 *               partials (fp64, in ws) are joined by one workgroup: thread t adds partials t, t + 256, ... in order, then the same
 *               tree.  No atomics: two runs give the same bits.  fp32 values squared in fp64 cannot overflow for n < 2^31, so ss is
 *               finite exactly when every g[i] is.
 *   skipped ... ss not finite: p, m and v keep their bits; ctl.skipped += 1, ctl.last_applied = 0, ctl.norm = sqrt(ss) (the
 *               non-finite value), ctl.scale = 0.
 *   applied ... otherwise: t = step - skipped (= applied + 1);
 *               c = fp32(min(1, max_norm / (norm + 1e-6))), the division in fp64, when 0 < max_norm < inf, else c = 1
 *               (torch.nn.utils.clip_grad_norm_'s coefficient on an fp64 norm);  g' = fl32(g[i] * c) -- g itself is never written;
 *               then crw_adam_step's arithmetic on g' at step t, operation for operation;
 *               ctl.applied += 1, ctl.last_applied = 1, ctl.norm = norm, ctl.scale = c.
 *   bias ...... while ctl.skipped == 0 the kernels use the two coefficients the host computed for `step`, exactly as crw_adam_step
 *               does: with c == 1 the outputs are crw_adam_step's bits.  Once a step has been skipped the device recomputes them in
 *               fp64 for t (1 - beta^t by the device's pow, each rounded once to fp32 as on the host).
 * One decision per call: a single workgroup makes it and writes it, with the coefficients, behind the partials in ws; every workgroup
 * of the update launch reads it from there, so a call never applies part of a buffer.  Three launches on `stream` (partials, decision,
 * update), no host synchronisation, no allocation, nothing read back.  The entry point has one route: there is no selector, so the
 * route log has no name for it.
 *
 * ctl: CRW_GUARD_CTL_BYTES of DEVICE memory, 8-byte aligned, zeroed by the caller once before the first step; only this entry point
 * writes it.  Layout (little endian, offsets in bytes):
 *    0  int64   applied        steps applied so far
 *    8  int64   skipped        steps refused so far
 *   16  double  norm           the last call's gradient norm (non-finite after a refused step)
 *   24  float   scale          the last call's clip coefficient c (0 after a refused step)
 *   28  int32   last_applied   1 when the last call applied its step, 0 when it refused it
 *   32  ...     reserved (never read; left as the caller zeroed it)
 * ws: crw_adam_guard_ws_bytes(n) bytes of device memory, 8-byte aligned; every byte that is read is written first by the same call.
 * CRW_EINVAL for whatever crw_adam_step refuses (a null or not 16-byte aligned p, g, m or v, n < 1, step < 1, a beta outside [0, 1)),
 * for a max_norm that is negative or NaN (0 and +inf: no clip), for a null or misaligned ctl or ws; CRW_EWORKSPACE for a small ws. */
#ifndef CRW_HIP_GUARD_H
#define CRW_HIP_GUARD_H

#include "crw_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CRW_GUARD_CTL_BYTES 64
#define CRW_GUARD_BLOCK_ELEMS 4096

/* ceil(n / CRW_GUARD_BLOCK_ELEMS) fp64 partials and the 16-byte decision record; 16 for n < 1 */
size_t crw_adam_guard_ws_bytes(long n);

int crw_adam_step_guarded(float *p, const float *g, float *m, float *v, long n, float lr, float beta1, float beta2, float eps,
                          int step, float max_norm, void *ctl, void *ws, size_t ws_bytes, crw_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
