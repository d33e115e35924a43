/*
 * murbbound.h — bound members of a murbhip context's bodies: the potential of a subset of the bodies at listed bodies or at
 * arbitrary points, membership by iterative unbinding, the bound mass and the Lagrangian radii of the members: the lines a
 * collisional code prints per output beside the density centre and the binary census.  An interface of its own beside
 * murbhip.h, murbfield.h, murbtidal.h, murbknn.h, murbnbr.h and murbbind.h (same library, libmurbhip.so; same conventions and
 * return codes): the calls here are read-outs in the sense of murbhip.h's call-order contract, and nothing declared in those
 * headers changes its behaviour because of them.
 *
 * 1. The potential sweep (normative).  For a point p with a skip entry, and a subset S of the bodies:
 *       phi_p = sum over the real bodies j in S, j != skip_p, of gm_j * inv
 *   with d = q_j - p, r2 = fma(dz,dz, fma(dy,dy, fma(dx,dx, soft2))) and inv = v_rsq_f32(r2): the sweeps' own (murbfield.h).
 *   gm_j is the fp32 G * m the upload folds in.  phi is positive, like "potential" and murbfield's phi.  This is the
 *   potential-only form of the field read-out: no acceleration, no jerk, no velocities.
 *   member: n bytes, a nonzero byte puts the body into S; NULL: all bodies.  The mask costs the loop nothing: a pack kernel
 *   writes a copy of the position + G m records in which the bodies outside S carry gm = +0, and the sweep reads that copy
 *   (the records themselves without a mask).  Two rules follow, bit for bit:
 *     Zero-mass rule.  phi under a mask equals phi without a mask on a context of the same n whose bodies outside S were
 *       uploaded with mass 0.
 *     Field rule.  With the same point, skip entry, bodies and "field_chunks", murbpot_at / murbpot_of return murbfield_at /
 *       murbfield_of's phi.
 *   The arithmetic is therefore the field sweep's: a lane's running sum takes every pair as ONE fused operation,
 *       ph = fma(gm_j * pm, inv, ph)
 *   with pm the 0/1 multiplier that is 0 in the tile of the point's own skipped slot alone (gm_j * 1 is exact, so outside that
 *   tile this is fma(gm_j, inv, ph); the product gm_j * inv is not rounded on its own: the field kernel's accumulation is
 *   compiled to this fused form).  The order is the lanes' steps in order: the chunk's tiles in layout order,
 *   the tile of the skipped slot adding zeros, then that tile again from memory with the slot's gm selected to 0; then the
 *   wave's fixed fold, then the chunks in ascending order, in fp32.  The chunk count and the launch cut are the field
 *   read-out's ("field_chunks", "field_batch": murbfield_set_option); a point's bits depend on its own inputs, the bodies, the
 *   mask and the chunk count alone.  With soft == 0 the forces' rule holds: NaN for a coincident pair (0 * inf under the
 *   multiplier or the mask as well).  NaN payloads are not promised.
 * murbpot_of: the points are the listed bodies' current positions, each with itself skipped; bodies NULL: all n bodies in
 *   order (count must then be n).  The same body may be listed twice.  A listed body need not be in S.
 * murbpot_at: points of the caller's.  skip NULL, or per point a body index or -1 (none).
 *
 * 2. Unbinding (normative): murbbound_members.  fp64 on the device, one operation per line, none contracted; the inline
 *   functions the device and the host share are in csrc/murb_bound.h.
 *   S_0 is `start` (n bytes, nonzero = in), or all real bodies when start is NULL.  For round t = 0, 1, ...:
 *     Frame.   frame_v given: V = frame_v (three doubles).  frame_v NULL: V = (sum over S_t of m v) / (sum over S_t of m), the
 *              masses as uploaded, each term (double)m * (double)v, the sums the 256-body block sums in murbhip_energy's fixed
 *              order with the block rows added in index order.  V = 0 when that mass is 0.
 *     Energy.  phi_i is the sweep above for every body i with the mask S_t, itself skipped.
 *              w = (double)v_i - V;   e_i = 0.5*((wx*wx + wy*wy) + wz*wz) - (double)phi_i
 *     Removal. S_{t+1} = { i in S_t : e_i < 0 }.  NaN is dropped.  Bodies only ever leave, so the loop ends.
 *     Stop.    Converged when S_{t+1} == S_t.  Otherwise the call stops after max_iter rounds (1 .. 4096) with `converged` 0
 *              and reports S_{max_iter}.
 *   Final pass.  e is filled for ALL real bodies from one evaluation against the final S and its V: a body outside S gets its
 *     energy against the members.  When the loop converged that evaluation is its last round's (same set, same frame, same
 *     bits).  Calling again with start = the returned member and max_iter = 1 continues the same sequence: one call of K rounds
 *     and K chained calls of one round return the same member, e and V bit for bit.
 *   member (n bytes, 0 / 1) and e (n doubles) may each be NULL.  out16, required:
 *     {members, bound mass, rounds run, converged (0 / 1), V (3), the members' centre of mass (3),
 *      K = sum over S of (0.5*m) |w|^2, W = -0.5 * sum over S of m * phi, K / |W|,
 *      bodies removed from start, real bodies with e >= 0, 0}
 *   in the same fixed block sums.  An empty S gives NaN for V, the centre and the ratio; members without mass give V = 0 and a
 *   NaN centre.
 *   Per round the host reads block rows alone (the count removed, the frame sums); the per-body arrays cross once, at the end.
 *   The implementation sweeps all bodies in every round; no bit depends on that.
 *
 * 3. Lagrangian radii: murbbound_radii, host only, needs no device and no context.  The members (member NULL: all n) are
 *   ordered by (d2, index), d2 = (dx*dx + dy*dy) + dz*dz in fp64 about centre3 with d = (double)q - centre.  radii[f] is
 *   sqrt(d2) of the first body at which the running fp64 mass, in that order, reaches frac[f] times the total of the same
 *   order.  frac lies in (0, 1].  NaN when the members' mass is 0.  MURBHIP_E_INVALID: a NULL array other than member, nfrac
 *   < 0, a coordinate, mass or centre that is not finite, a negative mass, a frac outside (0, 1].  nfrac == 0 returns 0.
 *
 * The bodies are the context's current ones on the device: positions and velocities as the last upload, initialisation or step
 *   left them, masses as uploaded.  With "contact" on, the radii in the velocity records are not read.  Under "integrator" 1 in
 *   flight the velocities are the device's, half a step behind the positions (murbfield.h says the same of its jerks).  Nothing
 *   of the context changes: the calls write buffers of their own and the field read-out's point buffer, which no other call
 *   reads, and never the sweeps' partial rows, the accelerations, the remembered (a0, j0), phi, (nn, r2), the step proposal,
 *   levels or ticks.
 * Call orders (murbhip.h, C1-C3).  The three device calls are synchronous observers: deleting them from a sequence of calls
 *   changes no bit of anything read afterwards, the other read-outs included, and each returns the bits it returns as the only
 *   observer at that point.  A refused call returns its code and changes nothing.
 * State.  Synchronous: waits for enqueued work, uploads, sweeps, downloads.  Allowed under every "integrator" value and with
 *   "nearest", "contact" or "potential" on.  MURBHIP_E_STATE before the first upload or initialisation, on a context of several
 *   shards or ranks, and while a block is open (the bodies sit at different times).  count == 0 returns 0 and does nothing, in
 *   every state.  MURBHIP_E_INVALID: a NULL context; a NULL position array or phi; a coordinate that is not finite; a skip
 *   entry outside [-1, n); a body index outside [0, n); bodies NULL with count != n; murbbound_members: out16 NULL, max_iter
 *   outside [1, 4096], a frame_v component that is not finite.
 * There are no options of its own: the calls read "field_chunks" and "field_batch" (murbfield_set_option) through the field
 *   read-out's planning.
 * With murbhip's "profile" 2 the sweep launches of a call are recorded as spans of a kind of their own ("span_pot_ms_avg",
 *   "span_pot_count"); the force_* figures count force launches alone.
 *
 * Not covered: the murb-hip command line and the tracking CSV; several shards or ranks; block-open states; re-admission of
 *   dropped bodies; a Jacobi (tidal) radius.
 */
#ifndef MURBBOUND_H_
#define MURBBOUND_H_

#include "murbhip.h"

#ifdef __cplusplus
extern "C" {
#endif

int murbpot_of(murbhip_ctx* ctx, unsigned long count, const int* bodies, const unsigned char* member, float* phi);
int murbpot_at(murbhip_ctx* ctx, unsigned long count, const float* px, const float* py, const float* pz, const int* skip,
               const unsigned char* member, float* phi);
int murbbound_members(murbhip_ctx* ctx, const unsigned char* start, const double* frame_v, int max_iter, unsigned char* member,
                      double* e, double* out16);

int murbbound_radii(unsigned long n, const float* qx, const float* qy, const float* qz, const float* m, const unsigned char* member,
                    const double* centre3, int nfrac, const double* frac, double* radii);

#ifdef __cplusplus
}
#endif

#endif
