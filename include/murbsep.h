/*
 * murbsep.h — pair separations of a murbhip context's bodies: per point the sum of the distances to a subset of the bodies, and
 * over a call the pairs counted in radial bins that are read off the float bits of the squared separation.  The mean pair
 * separation of Cartwright & Whitworth's Q, a two-point correlation function, a fractal dimension and a shell profile about a
 * centre are read off them.  An interface of its own beside murbhip.h, murbfield.h, murbtidal.h, murbknn.h, murbnbr.h,
 * murbbind.h, murbbound.h and murbmst.h (same library, libmurbhip.so; same conventions and return codes): the calls here are
 * read-outs in the sense of murbhip.h's call-order contract, and nothing declared in those headers changes its behaviour because
 * of them.
 *
 * 1. Definition (normative).  For a point p and a subset S of the real bodies:
 *   member: n bytes, a nonzero byte puts the body into S; NULL: all bodies (murbpot_of's rule).
 *   For every body j in S, d = q_j - p and
 *       d2 = fma(dz,dz, fma(dy,dy, fma(dx,dx, +0.f)))
 *   the sweeps' r2 expression (murbfield.h) with soft2 replaced by +0: a separation is geometric, the context's softening never
 *   enters.
 *
 *   Sum.  sum_p = sum over j in S of r_pj with r = v_sqrt_f32(d2), the hardware's root (1 ulp).  A body at the point's own
 *     position has d2 == +0 and r == +0 exactly and adds nothing: a listed body is left out of its own sum with no skip entry.
 *     A slot that must not count (a body outside S, padding, the points that fill the last group of 16) adds +0.
 *     Order: a lane keeps one running fp32 sum for the even and one for the odd slot of its pair, over its lane steps in order,
 *     the chunk's tiles in layout order; the two are added, then the wave's fixed fold, then the chunks in ascending order in
 *     fp64.  The output is double.  A point's bits depend on the point, the bodies, the mask and "field_chunks" alone: not on
 *     "field_batch", the other points of the call, or whether a histogram is asked for.  d2 that overflows or is subnormal is not
 *     promised.
 *
 *   Histogram.  The bin of a pair is a function of the fp32 bits of its d2 alone.
 *     lo_exp: the lowest edge is d2 = 2^lo_exp, a normal float (-126 .. 127).
 *     sub in 0 .. 6: 2^sub bins per octave of d2 (half-octave of r), linear in d2 within the octave.
 *     bins in 1 .. 1022.
 *     With sh = 23 - sub:   k = (bits(d2) >> sh) - (bits(2^lo_exp) >> sh)
 *     Bin k holds the pair for 0 <= k < bins; k < 0 is "below"; k >= bins, +inf and NaN are "above".  A pair whose d2 equals an
 *     edge belongs to the bin above that edge.  The edges are exact floats:
 *         edge2[k] = float_from_bits(((bits(2^lo_exp) >> sh) + k) << sh),   k = 0 .. bins
 *     and the top edge must be finite.
 *     Counts are over the ordered (point, body in S) pairs of the call, unsigned long long.  out4 = {pairs, below, above, 0}:
 *       pairs = sum over the points of |S|, less 1 for every listed body of murbsep_of that is in S: that body's own entry
 *       (d2 == +0) is struck from "below".   below + sum of hist + above == pairs, always.
 *     Bodies outside S, padding and filler points never appear in any of the four.  Counts are integers: they do not depend on
 *     "field_chunks", "field_batch" or the other points of the call.
 *
 * murbsep_of: the points are the listed bodies' current positions; bodies NULL: all n bodies in order (count must then be n).
 *   The same body may be listed twice.  A listed body need not be in S.
 * murbsep_at: points of the caller's.  There is no skip entry: a point that coincides with a body gets r = 0 from it and one
 *   "below" entry, which is what the definition says.
 * sum: count doubles, or NULL with bins > 0.  bins == 0: no histogram (the sum-only sweep; lo_exp, sub, hist and out4 are not
 *   read).  hist: bins entries.
 * murbsep_bin: host only, needs no device and no context: -1 below, bins above, else the bin of d2.  The bits are read as
 *   unsigned: a set sign bit, which a sum of squares never has, lies above like NaN.  MURBHIP_E_INVALID for parameters out of
 *   range (never a bin: it is below -1).
 * murbsep_edges: host only: bins + 1 entries each, either array may be NULL but not both; edge_r = sqrt((double)edge2).
 *
 * How it is computed.  A mask kernel writes a copy of the position records in which every slot that must not
 *   count sits at x = +inf with a cap of +0 and every other slot carries a cap of +inf; the running sum takes min(r, cap), which
 *   is +0 for the +inf or NaN of such a slot, and its pair lands in "above", from which the exactly known number of such entries
 *   is taken.  The counts are 32-bit integer adds in a workgroup's own table, stored once per launch and added into 64-bit
 *   totals in row order: no float atomic and no global atomic.  The launches are cut so that no 32-bit counter can wrap.
 *
 * The bodies are the context's current ones on the device: positions as the last upload, initialisation or step left them.
 *   Nothing of the context changes: the calls write buffers of their own and the field read-out's point buffer, which no other
 *   call reads, and never the sweeps' partial rows, the accelerations, the remembered (a0, j0), phi, (nn, r2), the step proposal,
 *   levels or ticks.
 * Call orders (murbhip.h, C1-C3).  The two device calls are synchronous observers: deleting them from a sequence of calls
 *   changes no bit of anything read afterwards, the other read-outs included, and each returns the bits it returns as the only
 *   observer at that point.  A refused call returns its code and changes nothing.
 * State.  Synchronous: waits for enqueued work, uploads, sweeps, downloads.  Allowed under every "integrator" value and with
 *   "nearest", "contact" or "potential" on.  MURBHIP_E_STATE before the first upload or initialisation, on a context of several
 *   shards or ranks, and while a block is open (the bodies sit at different times).  count == 0 returns 0 and does nothing, in
 *   every state.  MURBHIP_E_INVALID: a NULL context; sum NULL together with bins == 0; hist or out4 NULL with bins > 0; lo_exp,
 *   sub or bins out of range, or a top edge that is not finite; a NULL position array; a coordinate that is not finite; a body
 *   index outside [0, n); bodies NULL with count != n.
 * There are no options of its own: the calls read "field_chunks" and "field_batch" (murbfield_set_option) through the field
 *   read-out's planning.
 * With murbhip's "profile" 2 the sweep launches of a call are recorded as spans of a kind of their own ("span_sep_ms_avg",
 *   "span_sep_count"); the force_* figures count force launches alone.
 *
 * Not covered: projected (2-D) separations; weights other than a mask; several shards or ranks; block-open states; pair symmetry
 *   (every ordered pair is swept); the murb-hip command line; a correctly rounded root.
 */
#ifndef MURBSEP_H_
#define MURBSEP_H_

#include "murbhip.h"

#ifdef __cplusplus
extern "C" {
#endif

int murbsep_of(murbhip_ctx* ctx, unsigned long count, const int* bodies, const unsigned char* member, double* sum, int lo_exp, int sub,
               int bins, unsigned long long* hist, unsigned long long* out4);
int murbsep_at(murbhip_ctx* ctx, unsigned long count, const float* px, const float* py, const float* pz, const unsigned char* member,
               double* sum, int lo_exp, int sub, int bins, unsigned long long* hist, unsigned long long* out4);

int murbsep_bin(int lo_exp, int sub, int bins, float d2);
int murbsep_edges(int lo_exp, int sub, int bins, float* edge2, double* edge_r);

#ifdef __cplusplus
}
#endif

#endif
