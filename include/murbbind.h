/*
 * murbbind.h — bound pairs of a murbhip context's bodies: every body's most bound partner, the two-body elements of the mutual
 * bound pairs and the binary census a collisional code prints per output (number of binaries, their binding energy).  An
 * interface of its own beside murbhip.h, murbfield.h, murbtidal.h, murbknn.h and murbnbr.h (same library, libmurbhip.so; same
 * conventions and return codes): the calls here are read-outs in the sense of murbhip.h's call-order contract, and nothing
 * declared in those headers changes its behaviour because of them.
 *
 * Definition (normative).  For a point with position p, velocity u and gm_p, and a body j with its record's q_j, v_j, gm_j
 *   (gm_j the fp32 G * m the upload folds in), take d = q_j - p and w = v_j - u.  Each line is one fp32 operation:
 *       r2  = fma(dz,dz, fma(dy,dy, fma(dx,dx, soft2)))        (the sweeps' own r2)
 *       w2  = fma(wz,wz, fma(wy,wy, wx*wx))
 *       inv = v_rsq_f32(r2)
 *       gs  = gm_j + gm_p
 *       h   = fma(-gs, inv, 0.5f * w2)
 *   h is the specific orbital energy of the softened two-body problem, per unit reduced mass: negative when the pair is bound.
 *   The key is deliberately not the pair energy mu * h: m_i * m_j leaves the fp32 range in SI units, h also serves massless
 *   probes, and a = -G M / 2h follows from h directly.
 *   Candidates of a point are all real bodies j except its skipped slot; for a body (murbbind_of) the skipped slot is the body
 *   itself.  Massless bodies are candidates.  The zero-mass padding slots that fill the layout never are, though their h can
 *   well be the smallest.  Another body on the same point is a candidate.
 *   The result per point is (partner, h): the minimum under the total order (h as fp32, index); among equal h the lowest index
 *   wins.  A candidate whose h is NaN is never chosen, nor one whose h is +inf (w2 beyond the fp32 range).  With soft == 0 the
 *   forces' rule holds: a body on the point has inv = +inf, hence h = -inf where gs > 0 and NaN (not chosen) where gs == 0.
 *   A point with no candidate gets -1 and +inf.  -0 cannot arise.
 *   Consequences:
 *     h(i, j) == h(j, i) bit for bit: the differences are exact negatives of each other and the add commutes.
 *     The bits depend on the bodies and on the point's own inputs alone: not on the j-chunk cut ("field_chunks"), on
 *       "field_batch", on `count`, on the point's place in the call, on the other points or on the run.
 *     A pair (i, j) is MUTUAL when each is the other's partner.
 *     A pair is BOUND when it is mutual and its sweep value h < 0.
 *
 * murbbind_of: the points are the listed bodies' current q, v and gm, gathered on the device, each with itself skipped; bodies
 *   NULL: all n bodies in order (count must then be n).  The same body may be listed twice.  Either output may be NULL.
 * murbbind_at: probes of the caller's.  pvx, pvy, pvz all NULL: at rest.  m NULL: massless (gs = gm_j); otherwise
 *   gm_p = (float)g * m[p], the upload's one fp32 multiply.  skip NULL, or per point a body index or -1 (none).
 * murbbind_pairs: the sweep over all bodies, then the bound pairs with i < j, ascending in i.  Per pair six doubles
 *   elems[6 * p ..] = {a, e, P, h64, E_b, r}, computed in fp64 from the fp32 state; each line is one operation, none is
 *   contracted, and one inline function (csrc/murb_bind.h) serves the device and the host:
 *       d, w from the fp32 values (d = q_j - q_i, w = v_j - v_i, each component widened first)
 *       d2  = (dx*dx + dy*dy) + dz*dz            w2 likewise
 *       r   = sqrt(d2)                           rs = sqrt(d2 + (double)soft2)
 *       GM  = (double)gm_i + (double)gm_j
 *       h64 = 0.5*w2 - GM/rs
 *       a   = GM / (-2.0*h64)
 *       c   = d x w  (cx = dy*wz - dz*wy, ...)   L2 = (cx*cx + cy*cy) + cz*cz
 *       e   = sqrt(fmax(0, 1 + ((2.0*h64)*L2)/(GM*GM)))        (fmax: 0 where the argument is NaN)
 *       P   = 6.283185307179586 * sqrt(((a*a)*a)/GM)
 *       E_b = mu*h64          mu = (m_i*m_j)/(m_i + m_j), the masses as uploaded; 0 when m_i + m_j == 0
 *   Membership comes from the sweep's fp32 h, so the list follows from murbbind_of's arrays alone; the elements come from fp64.
 *   A pair within rounding of h = 0 may therefore show a <= 0 (and P NaN).  With r near the softening length the elements
 *   describe the softened problem, not Kepler's.  Two massless bodies (GM == 0) give E_b = 0, P NaN, a = -0 and e = +inf, or, at
 *   relative rest, a NaN and e = 0.
 *   One thread per body fills dense per-body arrays and the host compacts them in index order: no atomics.
 *   out8 = {bound pairs, sum E_b, hardest pair's i, its j, its E_b, smallest a, bodies whose partner has h < 0 (mutual or not),
 *   mutual pairs}.  The hardest pair is the one with the smallest E_b, the lowest i among equals.  sum E_b is fp64 in the fixed
 *   order of murbhip_energy's 256-body block sums, a pair counted at its lower index, the block rows added in index order.  With
 *   no pairs the entries for the hardest pair and the smallest a are NaN.
 *   i, j, elems all NULL ask for *count and out8 alone.  capacity < *count gives MURBHIP_E_INVALID with *count and out8 filled
 *   and the arrays untouched.
 * murbbind_elements: host-only, needs no device and no context: the same inline function for one pair, with gm = g * m in fp32
 *   and soft2 = soft * soft in fp32.  MURBHIP_E_INVALID: a NULL pointer, a value that is not finite, g, soft or a mass negative.
 *
 * The bodies are the context's current ones on the device: positions and velocities as the last upload, initialisation or step
 *   left them, masses as uploaded.  With "contact" on, the radii in the velocity records are not read.  Under "integrator" 1 in
 *   flight the velocities are the device's, half a step behind the positions (murbfield.h says the same of its jerks).  Nothing
 *   of the context changes: the calls write buffers of their own and the field read-out's point buffer, which no other call
 *   reads, and never the sweeps' partial rows, the accelerations, the remembered (a0, j0), phi, (nn, r2), the step proposal,
 *   levels or ticks.
 * Call orders (murbhip.h, C1-C3).  All three device calls are synchronous observers: deleting them from a sequence of calls
 *   changes no bit of anything read afterwards, the other read-outs included, and each returns the bits it returns as the only
 *   observer at that point.  A refused call returns its code and changes nothing.
 * State.  Synchronous: waits for enqueued work, uploads, sweeps, downloads.  Allowed under every "integrator" value and with
 *   "nearest", "contact" or "potential" on.  MURBHIP_E_STATE before the first upload or initialisation, on a context of several
 *   shards or ranks, and while a block is open (the bodies sit at different times).  count == 0 returns 0 and does nothing, in
 *   every state.  MURBHIP_E_INVALID: a NULL context; a NULL position array; some but not all velocity pointers NULL; a
 *   coordinate or velocity that is not finite; a mass that is negative or not finite; a skip entry outside [-1, n); a body
 *   index outside [0, n); bodies NULL with count != n; murbbind_pairs: count or out8 NULL, some but not all of i, j, elems NULL.
 * There are no options of its own: the calls read "field_chunks" and "field_batch" (murbfield_set_option) through the field
 *   read-out's planning.  As in murbknn.h its chunk count is the most a launch is cut into along j: a minimum does not depend
 *   on the cut.
 * With murbhip's "profile" 2 the sweep launches of a call are recorded as spans of a kind of their own ("span_bind_ms_avg",
 *   "span_bind_count"); the force_* figures count force launches alone.
 *
 * Not covered: several shards or ranks; block-open states; a binary stop for the evolve calls; regularisation; pair lists
 *   beyond mutual pairs (hierarchies); perturber lists.
 */
#ifndef MURBBIND_H_
#define MURBBIND_H_

#include "murbhip.h"

#ifdef __cplusplus
extern "C" {
#endif

int murbbind_of(murbhip_ctx* ctx, unsigned long count, const int* bodies, int* partner, float* h);
int murbbind_at(murbhip_ctx* ctx, unsigned long count, const float* px, const float* py, const float* pz, const float* pvx,
                const float* pvy, const float* pvz, const float* m, const int* skip, int* partner, float* h);
int murbbind_pairs(murbhip_ctx* ctx, int* i, int* j, double* elems, unsigned long capacity, unsigned long* count, double* out8);

int murbbind_elements(float g, float soft, const float* qi, const float* vi, float mi, const float* qj, const float* vj, float mj,
                      double* out6);

#ifdef __cplusplus
}
#endif

#endif
