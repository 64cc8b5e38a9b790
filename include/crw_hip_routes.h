/* The route log: which host-side selector branch launched (a companion of crw_hip.h; same status codes, same CRW_ABI_VERSION).
 * Added at ABI 8 without a bump: a library built before it still loads, the binding tells by symbol (crw_hip.has_routes()).  The
 * binding mirrors this header in crw_hip.ROUTES_SIGNATURES; tests/test_routes_host.py holds the two, the library and the
 * CRW_ROUTE("...") sites of csrc/ against each other, and tests/test_routes_gpu.py asserts the routes of calls on either side of
 * every selector's threshold.
 *
 * A ROUTE is a name that a selector (`launch_*`) passes to CRW_ROUTE (csrc/crw_common.h) immediately before the launch it decided
 * on; DESIGN.md section 8 lists every name with its selector and rule.  A site registers its name in a fixed process-wide table the
 * first time it is passed and bumps a relaxed atomic counter on every pass: host work only, no allocation, no device work.  With
 * CRW_ROUTE_LOG=<file> in the environment a name is also appended to that file as one line when it is registered (once per
 * process, O_APPEND): how a parent process learns what a child ran.  Both entry points take HOST pointers and are thread-safe
 * against running launches (counts read while another thread launches are a snapshot). */
#ifndef CRW_HIP_ROUTES_H
#define CRW_HIP_ROUTES_H

#include "crw_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* zero every counter (the names stay registered).  Returns CRW_OK. */
int crw_routes_clear(void);

/* names[i] / counts[i] of the first min(max, registered) sites in registration order (either array may be NULL; a name is a
 * string literal of the library, valid while it is loaded).  Returns the number of registered sites, which may exceed max. */
int crw_routes_read(const char **names, long *counts, int max);

#ifdef __cplusplus
}
#endif

#endif
