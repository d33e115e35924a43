/*
 * murbfield.h — field at arbitrary points: acceleration, jerk and potential that a murbhip context's bodies make at points of
 * the caller's.  An interface of its own beside murbhip.h (same library, libmurbhip.so; same conventions and return codes):
 * every call here is a read-out in the sense of murbhip.h's call-order contract, with options of its own, and nothing declared
 * in murbhip.h changes its behaviour because of it.
 *
 * The arithmetic is murbhip_compute_acc_jerk's and the "potential" option's with the point in the place of body i: with
 * d = q_j - p, w = v_j - pv, r2 = fma(dz,dz, fma(dy,dy, fma(dx,dx, soft2))) and inv the sweep's v_rsq_f32 of r2, over every real
 * body j != skip_p
 *       a_p = sum G m_j d inv^3      j_p = sum G m_j (w - 3 (d.w) d / r2) inv^3      phi_p = sum G m_j inv   (positive, like "potential")
 * The bodies are the context's current ones on the device: positions, velocities and G m as the last upload, initialisation or
 * step left them (under "integrator" 1 in flight the velocities are the device's, half a step behind).  Points have no mass, and
 * nothing of the context changes: the calls use buffers of their own (points, partial rows, results) and never write the sweeps'
 * partial rows, the accelerations, the remembered (a0, j0), phi, (nn, r2), the step proposal, levels or ticks.
 *
 * Call orders (murbhip.h, C1-C3).  murbfield_at and murbfield_of are observers: deleting them from a sequence of calls changes
 *   no bit of anything read afterwards, and each returns the bits it returns as the only observer at that point.  A refused call
 *   returns its code and changes nothing.  murbfield_set_option is an observer of everything murbhip.h declares: its keys are
 *   read by murbfield_at / murbfield_of and by murbtidal.h's murbtidal_at / murbtidal_of (which murbfield_layout plans too) and
 *   by nothing else.  tests/test_field_gpu.py checks this on runs of every integrator, and the values themselves against fp64
 *   at the state those runs leave.
 *
 * murbfield_at: px, py, pz the points; pvx, pvy, pvz their velocities, all three NULL = points at rest; skip NULL, or per point
 *   a body index or -1.  The skipped body is left out of all three sums BY SLOT: it never enters an fp32 sum (the reason
 *   murbhip_download_potential gives for phi; a point need not sit exactly on the body it skips, so it holds for a and j too).
 *   Another body at the same position counts.  Padding slots have G m = 0 and add +0.  n = 1 with that body skipped gives +0.0f
 *   everywhere.  soft == 0 follows the forces' rule (NaN for a coincident pair).  Each output group (ax, ay, az), (jx, jy, jz),
 *   phi may be NULL; results are in the caller's order.
 * murbfield_of: the points are the listed bodies' current q and v, gathered on the device (no host round trip of the state),
 *   each with itself skipped.  The same body may be listed twice.
 * Reproducibility.  The bits of one point's seven results depend on the point's own inputs and its skip entry, on the bodies, and
 *   on the j-chunk count — and on nothing else: not on `count`, the point's place in the arrays, the other points of the call,
 *   how the call is cut into launches, or the run.  The chunk count is therefore a function of the body count and of
 *   "field_chunks" alone, and the skipped slot is excluded per point, not per wave (a point's sums receive a chunk's
 *   tiles in layout order, then the tile of its skipped slot, whoever shares its wave).  Summation is fp32 throughout: the lanes,
 *   the wave, then the chunks in ascending order.
 * State.  Synchronous: waits for enqueued work, uploads, sweeps, downloads.  Allowed under every "integrator" value and with
 *   "nearest", "contact" or "potential" on (the radii in the velocity records are not read).  MURBHIP_E_STATE before the first
 *   upload or initialisation, on a context of several shards or ranks, and while a block is open (the bodies sit at different
 *   times).  count == 0 returns 0 and does nothing, in every state.  MURBHIP_E_INVALID: a NULL context; a NULL position array or `bodies`;
 *   some but not all of the three velocity pointers NULL; some but not all pointers of an output group NULL; a coordinate or
 *   velocity that is not finite; a skip entry outside [-1, n); a body index outside [0, n).
 * Not covered: several shards or ranks; points with mass; neighbours or contacts of points.
 */
#ifndef MURBFIELD_H_
#define MURBFIELD_H_

#include "murbhip.h"

#ifdef __cplusplus
extern "C" {
#endif

int murbfield_at(murbhip_ctx* ctx, unsigned long count, const float* px, const float* py, const float* pz, const float* pvx,
                 const float* pvy, const float* pvz, const int* skip, float* ax, float* ay, float* az, float* jx, float* jy,
                 float* jz, float* phi);
int murbfield_of(murbhip_ctx* ctx, unsigned long count, const int* bodies, float* ax, float* ay, float* az, float* jx, float* jy,
                 float* jz, float* phi);

/* Integer options of the two calls above.  Keys:
 *   "field_chunks"   j chunks a point's sums are cut into.  0 (default) = tiles / 8 kept within [1, 16], tiles = ceil(n / 512);
 *                    k > 0 = k, clamped to the tile count.  Never a function of the number of points.  The results depend on it
 *                    only through the chunk cut of the fp32 row sums
 *   "field_batch"    points per launch, a multiple of 16 up to 1 048 576; 0 (default) = 16 384.  Bounds the partial rows' memory
 *                    (32 bytes x points per launch x chunks).  No result depends on it
 * Other keys and values: MURBHIP_E_INVALID.  murbfield_get_option returns the value in force, defaults resolved.  With murbhip's
 * "profile" 2 the sweep launches of a call are recorded as spans of a kind of their own ("span_field_ms_avg", "span_field_count");
 * the force_* figures count force launches alone. */
int murbfield_set_option(murbhip_ctx* ctx, const char* key, long value);
int murbfield_get_option(murbhip_ctx* ctx, const char* key, long* value);

/* Host only, no device: the planning for n bodies under the two option values.  out4 = {chunks, groups of 16 points per full
 * launch, launches for a count of out4[3] on entry (or 0), partial-row entries per buffer = points per launch x chunks}; chunk c
 * sweeps the layout tiles [tiles c / chunks, tiles (c + 1) / chunks) with tiles = ceil(n / 512).  MURBHIP_E_INVALID for n == 0,
 * a NULL out4 or option values murbfield_set_option refuses. */
int murbfield_layout(unsigned long n, long chunks_option, long batch_option, unsigned long* out4);

#ifdef __cplusplus
}
#endif

#endif
