/*
 * murbknn.h — k nearest neighbours, local densities, density centre and core radius of a murbhip context's bodies: the
 * diagnostics a collisional code locates its cluster with (Casertano & Hut 1985).  An interface of its own beside murbhip.h,
 * murbfield.h and murbtidal.h (same library, libmurbhip.so; same conventions and return codes): the calls here are read-outs in
 * the sense of murbhip.h's call-order contract, and nothing declared in those headers changes its behaviour because of them.
 *
 * Definition (normative).  The r2 of a point p and a body j is the sweeps' own fp32 value, with d = q_j - p:
 *       r2 = fma(dz,dz, fma(dy,dy, fma(dx,dx, soft2)))
 *   Candidates of a point are all real bodies j except its skipped slot; for a body (murbknn_of) the skipped slot is the body
 *   itself.  Massless bodies are candidates.  The zero-mass padding slots that fill the layout never are.  Another body on the
 *   same point is a candidate (r2 = soft2).
 *   The result is the k smallest candidates under the total order (r2 as fp32, index), listed ascending: among equal r2 the
 *   lower index comes first, at the k-th place too.  Fewer than k candidates: the tail of the list is index -1, r2 = +inf.
 *   1 <= k <= MURBKNN_KMAX.
 *   Keys are unique, so the set and its order follow from the bodies alone, and the bits depend on nothing else: not on the
 *   j-chunk cut ("field_chunks"), on "field_batch", on `count`, on a point's place in the call, on the other points or on the
 *   run.  (The sums of the field read-out depend on the chunk count; a list does not.)
 *   With "nearest" 1, column 0 of a body's list is murbhip_download_nearest's (nn, r2) for the same state, bit for bit.
 *
 * Density (Casertano & Hut's unbiased estimator in its general-mass form), 2 <= k <= MURBKNN_KMAX.  Each operation below is one
 *   fp64 operation, without contraction:
 *       d2  = (double)r2_k - (double)soft2          (>= 0: every fma of the chain is monotone)
 *       M   = sum_{l = 1 .. k-1} (double)m_{j_l}    (in list order; the masses as uploaded)
 *       rho = (float)( M / (4.1887902047863905 * (d2 * sqrt(d2))) )
 *   The k-th neighbour and the body itself carry no mass in M.  d2 == 0 (k bodies on one point) gives +inf; fewer than k
 *   candidates give +0.
 *
 * Centre.  "Used" bodies are those with a finite rho.  All sums are fp64 on the device in a fixed order (the 256-body block
 *   sums of murbhip_energy's metrics, the block rows added in index order).  With S1 = sum rho and S2 = sum rho^2:
 *       X     = sum rho q / S1
 *       r_c   = sqrt( sum rho^2 |q - X|^2 / S2 )    (the NBODY6 convention)
 *       rho_c = S2 / S1
 *   The second moment is taken in a second pass about X; it is not expanded about the origin.
 *   out8 = {X_x, X_y, X_z, r_c, rho_c, S1, used, left out}.  S1 == 0: the first five values are NaN and the call returns 0.
 *
 * The bodies are the context's current ones on the device: positions as the last upload, initialisation or step left them,
 *   masses as uploaded.  Velocities are not read.  Nothing of the context changes: the calls write buffers of their own and the
 *   field read-out's point buffer, which no other call reads, and never the sweeps' partial rows, the accelerations, the
 *   remembered (a0, j0), phi, (nn, r2), the step proposal, levels or ticks.
 *
 * murbknn_of: the points are the listed bodies' current q, gathered on the device, each with itself skipped; bodies NULL: all n
 *   bodies in order (count must then be n).  The same body may be listed twice.
 * murbknn_at: px, py, pz the points; skip NULL, or per point a body index or -1 (none: a body on the point leads the list).
 *   idx and r2 are row-major, [p * k + l]; either may be NULL.
 * murbdensity_of: rho of the listed bodies (NULL: all n, in order).  murbdensity_centre: the density of every body, then the
 *   centre; out8 as above.
 * Call orders (murbhip.h, C1-C3).  All four are synchronous observers: deleting them from a sequence of calls changes no bit
 *   of anything read afterwards, murbfield.h's and murbtidal.h's read-outs included, and each returns the bits it returns as the
 *   only observer at that point.  A refused call returns its code and changes nothing.
 * State.  Synchronous: waits for enqueued work, uploads, sweeps, downloads.  Allowed under every "integrator" value and with
 *   "nearest", "contact" or "potential" on.  MURBHIP_E_STATE before the first upload or initialisation, on a context of several
 *   shards or ranks, and while a block is open (the bodies sit at different times).  count == 0 returns 0 and does nothing, in
 *   every state.  MURBHIP_E_INVALID: a NULL context; k outside [1, MURBKNN_KMAX] (densities: [2, MURBKNN_KMAX]); a NULL
 *   position array; a coordinate that is not finite; a skip entry outside [-1, n); a body index outside [0, n); bodies NULL
 *   with count != n; out8 or rho NULL.
 * There are no options of its own: the calls read "field_chunks" and "field_batch" (murbfield_set_option) through the field
 *   read-out's planning, so murbfield_layout plans them too.  Its chunk count is the most a launch is cut into along j: a list,
 *   unlike a sum, does not depend on the cut, and a launch whose groups of points fill the device is cut into fewer chunks
 *   (every chunk starts its lists empty); murbfield_layout's rows are an upper bound.
 * With murbhip's "profile" 2 the sweep launches of a call are recorded as spans of a kind of their own ("span_knn_ms_avg",
 *   "span_knn_count"); the force_* figures count force launches alone.
 *
 * Two host-only aids that need no device and no context:
 * murbknn_merge: the k first entries of the lexicographic merge of two lists sorted under the order above (k entries each,
 *   tails of -1 / +inf); the function the chunk fold uses.  The outputs alias no input.
 * murbknn_density: the formula above for one list; masses is indexed by the list's indices; soft2 = soft * soft in fp32.
 *   Both return MURBHIP_E_INVALID for k out of range or a NULL pointer.
 *
 * Not covered: several shards or ranks; block-open states; k > 32; neighbour lists as an integrator input (an Ahmad-Cohen
 *   scheme); neighbours within a radius (murbnbr.h: counts and full lists, per body or point).
 */
#ifndef MURBKNN_H_
#define MURBKNN_H_

#include "murbhip.h"

#define MURBKNN_KMAX 32

#ifdef __cplusplus
extern "C" {
#endif

int murbknn_of(murbhip_ctx* ctx, int k, unsigned long count, const int* bodies, int* idx, float* r2);
int murbknn_at(murbhip_ctx* ctx, int k, unsigned long count, const float* px, const float* py, const float* pz, const int* skip,
               int* idx, float* r2);
int murbdensity_of(murbhip_ctx* ctx, int k, unsigned long count, const int* bodies, float* rho);
int murbdensity_centre(murbhip_ctx* ctx, int k, double* out8);

int murbknn_merge(int k, const int* idx_a, const float* r2_a, const int* idx_b, const float* r2_b, int* idx_out, float* r2_out);
int murbknn_density(int k, const int* idx, const float* r2, const float* masses, float soft, float* rho_out);

#ifdef __cplusplus
}
#endif

#endif
