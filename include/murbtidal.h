/*
 * murbtidal.h — tidal tensor at arbitrary points: the gradient of the acceleration that a murbhip context's bodies make at points
 * of the caller's.  An interface of its own beside murbhip.h and murbfield.h (same library, libmurbhip.so; same conventions and
 * return codes): both calls here are read-outs in the sense of murbhip.h's call-order contract, and nothing declared in
 * murbhip.h or murbfield.h changes its behaviour because of them.
 *
 * Definition.  With d = q_j - p and r^2 = |d|^2 + soft^2, over every real body j != skip_p
 *       T_ab(p) = d a_a / d p_b = sum G m_j ( 3 d_a d_b / r^5 - delta_ab / r^3 )
 * T is symmetric; its six components come back as txx, tyy, tzz, txy, txz, tyz.  Its eigenvalues are the stretch (> 0) and
 * compression (< 0) rates along its principal axes; without softening its trace is 0 outside the bodies, with softening it is
 * -3 soft^2 sum G m_j / r^5.  Differences of murbfield_at accelerations do not give it: the sums are fp32, and at a step small
 * enough to be local the differences are rounding noise.
 *
 * Arithmetic (normative; one fp32 sequence per pair, the sweeps' up to s).  Per point p and body j:
 *       dx = xj - px  (dy, dz alike)       r2 = fma(dz,dz, fma(dy,dy, fma(dx,dx, soft2)))       inv = v_rsq_f32(r2)
 *       inv2 = inv*inv      gi = Gm_j*inv      s = gi*inv2      s3 = 3*s
 *       nx = dx*inv  (ny, nz alike)        tx = s3*nx  (ty, tz alike)
 *       txx += fma(tx, nx, -s)     tyy += fma(ty, ny, -s)     tzz += fma(tz, nz, -s)
 *       txy = fma(tx, ny, txy)     txz = fma(tx, nz, txz)     tyz = fma(ty, nz, tyz)
 *   The pair's term s (3 n_a n_b - delta_ab) is formed PER PAIR, before it is summed: a diagonal made as "sum 3 s n_a n_a" minus a
 *   separately accumulated "sum s" would carry the rounding of two sums of order sum s each into a trace whose terms are
 *   -3 s soft2 inv2 per pair.  Here a pair's three diagonal terms cancel inside the pair, before any sum has rounded.
 *   Domain: murbhip_create's.  n is a unit vector's component (|n_a| <= 1), s = (G m inv) inv^2 is the sweeps' pair factor, and
 *   3 G m inv^5 is never formed on its own: like G inv^3 it would leave the fp32 range at large r.
 *   Units: with the masses x 2^m and the lengths and the softening x 2^k every result is the former one x 2^(m - 3k), bit for bit
 *   (inside the normal range: n is unchanged and every other step is scaled by a power of two).
 *   Summation is fp32: the lanes, the wave, then the chunks in ascending order.
 *
 * The bodies are the context's current ones on the device: positions and G m as the last upload, initialisation or step left
 * them.  Velocities are not read.  Points have no mass, and nothing of the context changes: the calls use the field read-out's
 * buffers (points, partial rows, results), which no other call reads, and never write the sweeps' partial rows, the
 * accelerations, the remembered (a0, j0), phi, (nn, r2), the step proposal, levels or ticks.
 *
 * Call orders (murbhip.h, C1-C3).  murbtidal_at and murbtidal_of are observers: deleting them from a sequence of calls changes
 *   no bit of anything read afterwards — murbfield_at / murbfield_of included, whose buffers they share: every call of either
 *   interface is synchronous and writes what it reads — and each returns the bits it returns as the only observer at that
 *   point.  A refused call returns its code and changes nothing.
 *
 * murbtidal_at: px, py, pz the points; skip NULL, or per point a body index or -1.  The skipped body is left out of all six sums
 *   BY SLOT: it never enters an fp32 sum (a point 1e-4 of the separation from a body it skips would otherwise lose every other
 *   body's term below that body's (sep / soft)^3).  Another body at the same position counts.  Padding slots have G m = 0 and add
 *   +0.  n = 1 with that body skipped gives +0.0f six times.  soft == 0 follows the forces' rule (NaN for a coincident pair).
 *   The six output pointers are one group: all set, or all NULL (the call then validates, runs and returns 0).  Results are in
 *   the caller's order.
 * murbtidal_of: the points are the listed bodies' current q, gathered on the device (no host round trip of the state), each with
 *   itself skipped.  The same body may be listed twice.
 * Reproducibility.  The bits of one point's six results depend on the point's own inputs and its skip entry, on the bodies, and
 *   on the j-chunk count — and on nothing else: not on `count`, the point's place in the arrays, the other points of the call,
 *   how the call is cut into launches, or the run.  There are no options of its own: the calls read "field_chunks" and
 *   "field_batch" (murbfield_set_option) through the field read-out's planning, so murbfield_layout plans them too, the chunk
 *   count is a function of the body count and of "field_chunks" alone, and no result depends on "field_batch".  The skipped slot
 *   is excluded per point, not per wave (a point's sums receive a chunk's tiles in layout order, then the tile of its skipped
 *   slot, whoever shares its wave).
 * State.  Synchronous: waits for enqueued work, uploads, sweeps, downloads.  Allowed under every "integrator" value and with
 *   "nearest", "contact" or "potential" on.  MURBHIP_E_STATE before the first upload or initialisation, on a context of several
 *   shards or ranks, and while a block is open (the bodies sit at different times).  count == 0 returns 0 and does nothing, in
 *   every state.  MURBHIP_E_INVALID: a NULL context; a NULL position array or `bodies`; some but not all of the six output
 *   pointers NULL; a coordinate that is not finite; a skip entry outside [-1, n); a body index outside [0, n).
 * With murbhip's "profile" 2 the sweep launches of a call are recorded as spans of a kind of their own ("span_tidal_ms_avg",
 *   "span_tidal_count"); the force_* figures count force launches alone.
 * Not covered: several shards or ranks; the tensor's time derivative; points with mass.
 */
#ifndef MURBTIDAL_H_
#define MURBTIDAL_H_

#include "murbhip.h"

#ifdef __cplusplus
extern "C" {
#endif

int murbtidal_at(murbhip_ctx* ctx, unsigned long count, const float* px, const float* py, const float* pz, const int* skip,
                 float* txx, float* tyy, float* tzz, float* txy, float* txz, float* tyz);
int murbtidal_of(murbhip_ctx* ctx, unsigned long count, const int* bodies, float* txx, float* tyy, float* tzz, float* txy,
                 float* txz, float* tyz);

#ifdef __cplusplus
}
#endif

#endif
