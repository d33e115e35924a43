/*
 * murblist.h — the field of LISTED bodies: acceleration, jerk and potential at a point from an explicit list of source bodies of a
 * murbhip context, at a cost of O(list length) instead of the O(N) of every other read-out; and the neighbour split of a body's
 * force built on it.  What consumes the lists murbnbr.h hands out: the irregular force of an Ahmad-Cohen scheme (a body's
 * neighbours alone; the regular remainder is the full field minus it), the perturbing force of listed perturbers on a binary,
 * the granular share of a body's force.  An interface of its own beside murbhip.h, murbfield.h and murbnbr.h (same library,
 * libmurbhip.so; same conventions and return codes): the calls here are read-outs in the sense of murbhip.h's call-order contract,
 * and nothing declared in those headers changes its behaviour because of them.
 *
 * Definition (normative).
 *   Lists.  Point p has the source list idx[offsets[p] .. offsets[p + 1]): CSR form with murbnbr_of's types, offsets holding
 *   count + 1 entries.  A list entry is a body index and is used exactly as given: there is no skip machinery; a body in its own
 *   list counts like any other (r2 = soft2: it adds G m / soft to phi and nothing to a; with soft == 0 it is a coincident pair);
 *   a body listed twice counts twice; the ORDER of the entries matters (it decides which lane adds which term).
 *   Pair arithmetic.  The Hermite sweeps' packed pair function, unchanged, with the point in the place of body i:
 *       d = q_j - p, w = v_j - pv, r2 = fma(dz,dz, fma(dy,dy, fma(dx,dx, soft2))), inv = v_rsq_f32(r2), gi = (G m_j) * inv,
 *       a += (gi * inv^2) * d,   j += (gi * inv^2) * (w - 3 (d.w) inv^2 d),   phi = the sum of gi
 *   The formulas and sign conventions are murbfield.h's (phi positive).
 *   Summation, fp32.  Entry e of a list of length L sits in lane (e >> 1) & 63, half e & 1, lane step e >> 7.  Per lane and half
 *   a running sum over the lane steps, ascending; then x + y of the two halves; then the wave sum of the force sweeps
 *   (murb_wave_sum).  There are no chunks and no partial rows.
 *   The slots of the last lane step past L add exactly +0 for every softening, 0 included: those lanes re-read the list's LAST
 *   entry with G m replaced by +0, so their products are +-0 whenever that entry's own term is finite; where it is not finite the
 *   sum is already NaN by the forces' rule (a coincident pair with soft == 0 gives NaN).
 *   An empty list gives +0.0f seven times.
 *   So a point's seven results depend on the point, the bodies and its own list in its own order, and on nothing else: not on
 *   `count`, on the point's place in the call, on the other points or their lists, on how the call is cut into launches
 *   ("field_batch") or ranges ("list_entries"), on any option, or on the run.  No atomic operation takes part.
 *
 * The bodies are the context's current ones on the device: positions, velocities and G m as the last upload, initialisation or
 *   step left them.  Nothing of the context changes: the calls write buffers of their own, the field read-out's point and result
 *   buffers and the neighbour read-out's list buffer, which no other call reads, and never the sweeps' partial rows, the
 *   accelerations, the remembered (a0, j0), phi, (nn, r2), the step proposal, levels or ticks.
 *
 * murblist_of: the points are the listed bodies' current q and v, gathered on the device; bodies NULL: all n bodies in order
 *   (count must then be n).  The same body may be listed twice.  The body itself is NOT left out of its list: leave it out of idx.
 * murblist_at: px, py, pz the points, pvx, pvy, pvz their velocities (all three, or all NULL: at rest).
 * Outputs: ax ay az (all three or none), jx jy jz (all three or none), phi (or NULL): `count` floats each.
 * murbsplit_of: the irregular force of the listed bodies.  The lists are murbnbr_of's for the same bodies, h and h_all: same
 *   predicate (r2 <= thr), ascending index, the body itself never listed.  They are produced into the neighbour read-out's device
 *   list buffer and consumed from it without a host round trip; ranges of points are cut by murbnbr_cut under "list_entries".
 *   counts (may be NULL): counts[p] is the list length.  The seven results are bit for bit murblist_of's on the lists murbnbr_of
 *   returns.  The regular force is murbfield_of's result minus this one, formed by the caller (in fp64, if one rounding matters).
 *
 * Call orders (murbhip.h, C1-C3).  All three are synchronous observers: deleting them from a sequence of calls changes no bit of
 *   anything read afterwards, the other read-outs included, and each returns the bits it returns as the only observer at that
 *   point.  A refused call returns its code and changes nothing: nothing is launched and no output is written.
 * State.  murbnbr.h's: synchronous; allowed under every "integrator" value and with "nearest", "contact" or "potential" on.
 *   MURBHIP_E_STATE before the first upload or initialisation, on a context of several shards or ranks, and while a block is open.
 *   count == 0 returns 0 and does nothing, in every state.  MURBHIP_E_INVALID, all checked on the host before any launch, so that
 *   the kernel never reads outside the records: a NULL context; NULL offsets; offsets[0] != 0; offsets not non-decreasing; NULL idx
 *   with a non-zero total; a list entry outside [0, n); a list longer than 2^30 entries; a body index outside [0, n); bodies NULL
 *   with count != n; a NULL position array; a group of pointers (pvx pvy pvz; ax ay az; jx jy jz) set in part; a coordinate or
 *   velocity that is not finite; a radius that is negative or not finite.
 * Options.  None of their own.  The calls read "field_batch" (murbfield_set_option: points per launch) and "list_entries"
 *   (murbnbr_set_option: entries staged per range of points; a single list longer than the list buffer grows it, as in
 *   murbnbr.h).  Both are result-neutral.  With murbhip's "profile" 2 the sweep launches are recorded as spans of a kind of
 *   their own ("span_list_ms_avg", "span_list_count"); murbsplit_of's count and fill sweeps stay "nbr" spans.
 *
 * Not covered: an Ahmad-Cohen integrator; lists resident across steps; several shards or ranks; block-open states; fp64 sums;
 *   balancing a few very long lists over waves (a list is one wave's work); weights per entry.
 */
#ifndef MURBLIST_H_
#define MURBLIST_H_

#include "murbhip.h"

#ifdef __cplusplus
extern "C" {
#endif

int murblist_of(murbhip_ctx* ctx, unsigned long count, const int* bodies, const unsigned long* offsets, const int* idx, float* ax,
                float* ay, float* az, float* jx, float* jy, float* jz, float* phi);
int murblist_at(murbhip_ctx* ctx, unsigned long count, const float* px, const float* py, const float* pz, const float* pvx,
                const float* pvy, const float* pvz, const unsigned long* offsets, const int* idx, float* ax, float* ay, float* az,
                float* jx, float* jy, float* jz, float* phi);
int murbsplit_of(murbhip_ctx* ctx, unsigned long count, const int* bodies, const float* h, float h_all, unsigned long* counts,
                 float* ax, float* ay, float* az, float* jx, float* jy, float* jz, float* phi);

#ifdef __cplusplus
}
#endif

#endif
