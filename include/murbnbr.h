/*
 * murbnbr.h — neighbours within a radius of a murbhip context's bodies: per body or per arbitrary point the COUNT and the LIST of
 * the bodies inside a sphere of its own radius h.  What a fixed k (murbknn.h) cannot answer: who is inside a body's neighbour
 * sphere (the input of an Ahmad-Cohen scheme), how many bodies lie within h of a point (number density at a fixed scale), which
 * bodies are linked at a linking length (friends-of-friends groups), which pairs are candidates for a close-encounter treatment.
 * An interface of its own beside murbhip.h, murbfield.h, murbtidal.h and murbknn.h (same library, libmurbhip.so; same
 * conventions and return codes): the calls here are read-outs in the sense of murbhip.h's call-order contract, and nothing
 * declared in those headers changes its behaviour because of them.
 *
 * Definition (normative).  The r2 of a point p and a body j is the sweeps' own fp32 value, with d = q_j - p:
 *       r2 = fma(dz,dz, fma(dy,dy, fma(dx,dx, soft2)))
 *   Candidates of a point are all real bodies j except its skipped slot; for a body (murbnbr_of) the skipped slot is the body
 *   itself.  Massless bodies are candidates.  The zero-mass padding slots that fill the layout never are.  Another body on the
 *   same point is a candidate (r2 = soft2).
 *   Threshold.  Per point, with its radius h:
 *       thr = (float)((double)h * h + (double)soft2)
 *   which is murbhip_set_encounter's rule; murbnbr_threshold gives it (soft2 = soft * soft in fp32).  Candidate j is a
 *   neighbour if and only if r2 <= thr (with <=: a body exactly on the sphere is inside).  h is an array of `count` radii, or
 *   NULL: then every point uses h_all (which is not read otherwise).  Radii must be finite and >= 0.  h == 0 lists the bodies on
 *   the point itself (r2 = soft2 = thr).  A thr that rounds to +inf makes every candidate a neighbour.
 *   Output, in CSR form.  offsets holds count + 1 entries and is required: offsets[0] = 0, offsets[count] is the total, and
 *   the neighbours of point p are idx[offsets[p] .. offsets[p + 1]) in ASCENDING BODY INDEX, r2 holding the sweep's value of
 *   each entry.
 *   Membership is a predicate of one pair and the order is the index's, so the bits depend on the bodies, the point and its h
 *   alone: not on the j-chunk cut ("field_chunks"), on "field_batch", on "list_entries", on `count`, on a point's place in the
 *   call, on the other points or on the run.  No atomic operation takes part.
 *   r2(i, j) == r2(j, i) bit for bit (the differences are exact negatives of each other), so with a common h body j is listed
 *   for body i if and only if i is listed for j.  An entry's r2 is murbknn_of's for the same pair, bit for bit.
 *
 * Count-only calls.  idx == NULL and r2 == NULL: only the count pass runs, offsets is filled, capacity is ignored.
 * Capacity.  idx or r2 given (either may be NULL alone): `capacity` is the number of entries each given array holds.  If
 *   offsets[count] > capacity, offsets is complete, idx and r2 are untouched, and the call returns MURBHIP_E_INVALID: the caller
 *   sizes its arrays from the offsets and calls again.
 *
 * The bodies are the context's current ones on the device: positions as the last upload, initialisation or step left them.
 *   Velocities and masses are not read.  Nothing of the context changes: the calls write buffers of their own and the field
 *   read-out's point buffer, which no other call reads, and never the sweeps' partial rows, the accelerations, the remembered
 *   (a0, j0), phi, (nn, r2), the step proposal, levels or ticks.
 *
 * murbnbr_of: the points are the listed bodies' current q, gathered on the device, each with itself skipped; bodies NULL: all n
 *   bodies in order (count must then be n).  The same body may be listed twice.
 * murbnbr_at: px, py, pz the points; skip NULL, or per point a body index or -1 (none: a body on the point is listed).
 * Call orders (murbhip.h, C1-C3).  Both are synchronous observers: deleting them from a sequence of calls changes no bit of
 *   anything read afterwards, the other read-outs included, and each returns the bits it returns as the only observer at that
 *   point.  A refused call returns its code and changes nothing.
 * State.  Synchronous: waits for enqueued work, uploads, sweeps, downloads.  Allowed under every "integrator" value and with
 *   "nearest", "contact" or "potential" on.  MURBHIP_E_STATE before the first upload or initialisation, on a context of several
 *   shards or ranks, and while a block is open (the bodies sit at different times).  count == 0 returns 0 and does nothing, in
 *   every state.  MURBHIP_E_INVALID: a NULL context; a NULL position array; NULL offsets; a coordinate that is not finite; a
 *   radius that is negative or not finite; a skip entry outside [-1, n); a body index outside [0, n); bodies NULL with
 *   count != n; a total beyond the capacity (above).
 * Options.  The calls read "field_chunks" and "field_batch" (murbfield_set_option) through the field read-out's planning.
 *   One option of their own, murbnbr_set_option / murbnbr_get_option:
 *       "list_entries"   the device list buffer's size in entries; 0 = the default, 1 << 26; at least 16, at most 1 << 30.
 *                        The lists of a launch's points are produced in consecutive ranges of points whose totals fit the
 *                        buffer; a single point whose list is longer grows the buffer to that list.  Result-neutral: it exists
 *                        so that the cut can be tested at small shapes.  murbnbr_get_option gives the value as resolved.
 * With murbhip's "profile" 2 the count and fill sweep launches of a call are recorded as spans of a kind of their own
 *   ("span_nbr_ms_avg", "span_nbr_count"); the force_* figures count force launches alone.
 *
 * Two host-only aids that need no device and no context:
 * murbnbr_threshold: thr of the rule above for one radius and softening length.  MURBHIP_E_INVALID: h or soft negative or not
 *   finite, thr NULL.
 * murbnbr_cut: the function that cuts a launch's points into ranges.  offsets: count + 1 non-decreasing entries; *last is the
 *   furthest point in (first, count] such that offsets[last] - offsets[first] <= entries, and first + 1 where even one list does
 *   not fit.  MURBHIP_E_INVALID: first >= count, or a NULL pointer.
 *
 * Not covered: several shards or ranks; block-open states; mass or other sums over the sphere (an fp32 sum would depend on the
 *   cut: take them from the list); lists kept on the device as an integrator's input; lists sorted by distance (murbknn.h serves
 *   that, up to k = 32).
 */
#ifndef MURBNBR_H_
#define MURBNBR_H_

#include "murbhip.h"

#ifdef __cplusplus
extern "C" {
#endif

int murbnbr_of(murbhip_ctx* ctx, unsigned long count, const int* bodies, const float* h, float h_all, unsigned long* offsets,
               int* idx, float* r2, unsigned long capacity);
int murbnbr_at(murbhip_ctx* ctx, unsigned long count, const float* px, const float* py, const float* pz, const int* skip,
               const float* h, float h_all, unsigned long* offsets, int* idx, float* r2, unsigned long capacity);
int murbnbr_set_option(murbhip_ctx* ctx, const char* key, long value);
int murbnbr_get_option(murbhip_ctx* ctx, const char* key, long* value);

int murbnbr_threshold(float h, float soft, float* thr);
int murbnbr_cut(unsigned long count, const unsigned long* offsets, unsigned long first, unsigned long entries, unsigned long* last);

#ifdef __cplusplus
}
#endif

#endif
