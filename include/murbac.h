/*
 * murbac.h — an Ahmad-Cohen neighbour scheme on resident lists: a 4th-order Hermite integrator with shared step dt in which the
 * full O(N^2) sweep happens only on every n_irr-th step (a REGULAR step); the steps between (IRREGULAR steps) evaluate each body's
 * neighbours alone, at O(list length), and extrapolate the rest of the force as a cubic in time (Ahmad & Cohen 1973; Makino &
 * Aarseth 1992 §4; Aarseth 2003 ch. 3).  What puts murbnbr.h's lists and murblist.h's list field to work: the lists stay on the
 * device from one regular step to the next.  An interface of its own beside murbhip.h (same library, libmurbhip.so; same
 * conventions and return codes); nothing declared in the other headers changes its behaviour because of it.
 *
 * State the scheme holds, all on the device, in buffers of its own that no read-out touches:
 *   L               the lists, CSR, ascending index, the body itself never listed
 *   (aI, jI)        the irregular force and jerk at the current time
 *   (aR, jR, a2R, a3R)  the regular force and its first three time derivatives at the time tR of the last regular step
 *   m               steps since the last regular one, in [0, n_irr)
 *   (a0, j0)        the TOTAL at the current time: the context's remembered Hermite evaluation, which murbhip_download_acc and
 *                   murbhip_download_jerk return
 *
 * Definition (normative).  Predictor and corrector are murbhip.h's Hermite ones; pair arithmetic and summation order of a list field
 * are murblist.h's; the lists' predicate is murbnbr.h's; all unchanged.
 *   Begin, at the current state.  L = murbnbr_of's lists of all bodies for h.  (aI, jI) = murbsplit_of's bits.  (a0, j0) =
 *     murbhip_compute_acc_jerk's bits.  aR = a0 - aI and jR = j0 - jI in fp32, one rounding each.  a2R = a3R = 0.  m = 0.
 *   Irregular step (m + 1 < n_irr).
 *     1  (qp, vp) from (q, v, a0, j0, dt) with the Hermite predictor.
 *     2  (aI1, jI1): the list field at each body's own (qp_i, vp_i) from the PREDICTED sources over L_i: bit for bit what
 *        murblist_at returns for those points and lists on a context that holds the predicted state.
 *     3  tau = (double)(m + 1) * (double)dt.  With fp64 intermediates, contraction off, left to right, one rounding at the end:
 *            aRtau = (float)(((aR + jR tau) + a2R (tau tau 0.5)) + a3R (tau tau tau / 6))
 *            jRtau = (float)((jR + a2R tau) + a3R (tau tau 0.5))
 *     4  a1 = aI1 + aRtau, j1 = jI1 + jRtau, in fp32.
 *     5  the Hermite corrector with (a0, j0, a1, j1, dt); then (a0, j0) <- (a1, j1), (aI, jI) <- (aI1, jI1), m <- m + 1.
 *   Regular step (m + 1 == n_irr).
 *     1  predict as above.
 *     2  (a1, j1): the full sweep at the predicted state, the Hermite step's rows summed in its order.
 *     3  (aIo, jIo): the list field over the OLD lists at the predicted state.  A1 = a1 - aIo, J1 = j1 - jIo, in fp32.
 *     4  T = (double)n_irr * (double)dt.  With A0 = aR, J0 = jR, in fp64:
 *            x2 = (-6 (A0 - A1) - T (4 J0 + 2 J1)) / (T T)         x3 = (12 (A0 - A1) + 6 T (J0 + J1)) / (T T T)
 *            a2R <- (float)(x2 + T x3)                             a3R <- (float)x3
 *        Makino & Aarseth's interpolation; both ends of it are taken on the same list.
 *     5  new lists L': murbnbr_of's predicate applied to the predicted records.  (aIn, jIn): the list field over L'.
 *        aR <- a1 - aIn, jR <- j1 - jIn, (aI, jI) <- (aIn, jIn), L <- L', m <- 0.
 *     6  the Hermite corrector with the TOTAL (a0, j0, a1, j1, dt); then (a0, j0) <- (a1, j1).
 *   tau and T use the dt of the step being taken; dt may differ between calls of murbac_steps.
 *   Two consequences.  With n_irr = 1, q, v, a0, j0 after any number of steps are bit for bit murbhip_steps' under "integrator" 2,
 *   for every h.  With h = 0 every aI is +0 and aR == a0 bit for bit.
 *
 * murbac_begin: h per body, or NULL with the common radius h_all, as in murbnbr_of.  n_irr in [1, 4096].  A live scheme is replaced.
 * murbac_steps: `steps` steps of size dt; enqueues and returns like murbhip_steps.  An irregular step makes no host round trip; a
 *   regular step makes one, to read the list sizes.  steps == 0 returns 0 where the call is otherwise accepted.
 * murbac_end: ends the scheme (no error if none is live).  The bodies stay where they are; the remembered (a0, j0) is kept where
 *   the last step was a regular one (m == 0: it is a full sweep's) and dropped otherwise.
 * murbac_state: out[0..8] = n_irr, m, steps taken, regular steps taken, total entries, longest list, empty lists, mean list, the
 *   time since murbac_begin (the fp64 sum of the steps' dt); out[9..15] are reserved and 0.  Without a live scheme all are 0.
 * murbac_lists: the resident lists in CSR form with murbnbr_of's capacity rule: offsets holds n + 1 entries; idx may be NULL with
 *   capacity 0 (the offsets alone); a capacity below the total returns MURBHIP_E_INVALID with complete offsets and an untouched idx.
 * murbac_forces: each argument may be NULL; each array it names holds n floats: irr = {aIx, aIy, aIz, jIx, jIy, jIz} at the current
 *   time, reg = {aR, jR} and reg2 = a2R, reg3 = a3R at tR.
 *
 * Rules.
 *   Requirements: "integrator" 2; one shard and one rank; no open block; no resident tracers; "nearest", "contact" and "potential"
 *     off (their side products would only be refreshed at regular steps).  Otherwise murbac_begin / murbac_steps return
 *     MURBHIP_E_STATE.  murbac_steps, murbac_lists and murbac_forces without a live scheme return MURBHIP_E_STATE.
 *   MURBHIP_E_INVALID, checked before any launch: a NULL context; n_irr out of range; a radius negative or not finite; dt not
 *     finite or <= 0; steps < 0; NULL offsets or out.
 *   What ends the scheme: any call that changes the bodies from outside or steps them another way ends it silently: upload,
 *     initialisation, murbhip_step(s) of at least one step, murbhip_evolve*, murbhip_integrate_host_acc, murbhip_block_set_levels,
 *     a change of a side option.  However a scheme ends, murbac_end included, the remembered (a0, j0) is kept only where the bodies
 *     are unchanged and the last step was a regular one (m == 0: it is a full sweep's); otherwise it is dropped, so that the next
 *     Hermite step evaluates afresh: murbac_end followed by murbhip_steps gives the bits murbhip_steps alone gives.  While a scheme
 *     is live murbhip_compute_acc_jerk is an observer: (a0, j0) is remembered, so it evaluates nothing and the downloads return the
 *     scheme's total.  No call of the other headers gains a refusal.
 *   A failed rebuild (a total beyond 2^31 - 1 entries: MURBHIP_E_INVALID; no memory: the allocation's code) returns the error,
 *     leaves the bodies at the end of the last completed step and ends the scheme.
 *   Call orders (murbhip.h, C1-C3).  Every read-out (field, tidal, knn, nbr, bind, bound, mst, sep, list, split) stays an observer
 *     while a scheme is live: deleting it from a sequence changes no bit of any later result of this header, and it returns the bits
 *     it returns as the only observer.  murbac_state, murbac_lists and murbac_forces are observers themselves (the latter two
 *     synchronise).  murbhip_energy and the downloads work between calls as after a Hermite step.
 *   Options.  None of its own.  With murbhip's "profile" 2 the list sweeps are "list" spans, the rebuild's count and fill sweeps "nbr"
 *     spans, the full sweep a force span, an irregular step's predictor an "ac_predict" span and either kind's last launch an
 *     "ac_correct" span ("span_ac_predict_ms_avg", "span_ac_correct_count", ...).
 *
 * Not covered: individual or block steps for the irregular force; NBODY6's derivative corrections for gained and lost neighbours
 *   (a2R and a3R are kept from the old list across a list change); adaptive dt, n_irr or radii; the neighbour predicate inside the
 *   acceleration + jerk sweep (it would remove the rebuild's O(N^2) pass); several shards or ranks; tracers and side products beside
 *   the scheme; fp64 sums; balancing long lists over waves.
 */
#ifndef MURBAC_H_
#define MURBAC_H_

#include "murbhip.h"

#ifdef __cplusplus
extern "C" {
#endif

int murbac_begin(murbhip_ctx* ctx, const float* h, float h_all, int n_irr);
int murbac_steps(murbhip_ctx* ctx, float dt, int steps);
int murbac_end(murbhip_ctx* ctx);
int murbac_state(murbhip_ctx* ctx, double out[16]);
int murbac_lists(murbhip_ctx* ctx, unsigned long* offsets, int* idx, unsigned long capacity);
int murbac_forces(murbhip_ctx* ctx, float* irr[6], float* reg[6], float* reg2[3], float* reg3[3]);

#ifdef __cplusplus
}
#endif

#endif
