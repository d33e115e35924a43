/*
 * murbtracer.h — massless tracers: a second population of test particles resident on the device beside a murbhip context's
 * bodies, carried through the Hermite steps (murbhip_step / murbhip_steps under "integrator" 2, murbhip_evolve) at the
 * integrator's own accuracy, without a host round trip per step.  An interface of its own beside murbhip.h (same library,
 * libmurbhip.so; same conventions and return codes as murbfield.h and murbtidal.h).  murbhip.h's declarations, option keys and
 * call-order table stay as they are; with no tracers resident every result of every call there is what it is without this
 * header, bit for bit.
 *
 * Arithmetic.  A tracer feels the bodies and nothing feels a tracer.  Its acceleration and jerk are murbfield_at's for the same
 *   point, velocity and no skipped body: the same fp32 sequence per pair, the lanes, the wave, then the j chunks in ascending
 *   order, so the bits are EQUAL to murbfield_at's (ax .. jz) against the same bodies at the same chunk count.  Predictor and
 *   corrector are the bodies' (fp64 intermediates, no contraction, one rounding at the store): an fp64 restatement fed the same
 *   fp32 inputs reproduces them bit for bit.
 * A step, per step of the bodies and on the compute stream, enqueue-only:
 *       bodies' predictor; tracer predictor; bodies' sweep; tracer sweep AT THE BODIES' PREDICTED STATE (the records and
 *       velocities the bodies' sweep reads); bodies' corrector; tracer corrector.
 *   Under murbhip_evolve the tracer kernels read dt from the control block and do nothing once the run has ended, so an
 *   encounter or contact stop ends the run behind the hitting step for the tracers too.  When the tracers' (a0, j0) are not
 *   current (after an upload of tracers or of bodies) the next step or evolve call first evaluates them at the current state;
 *   that evaluation never touches the bodies' remembered (a0, j0).
 * Reproducibility.  A tracer's bits depend on its own state, the bodies and the chunk count, and on nothing else: not on
 *   `count`, its place in the arrays, the other tracers, "tracer_batch" or the run.  The last group of 16 is filled with copies
 *   of its first tracer, whose results are never stored.
 *
 * murbtracer_upload: `count` tracers at the bodies' current model time; replaces any earlier set; count == 0 clears; vx, vy, vz
 *   all NULL = at rest.
 * murbtracer_download: q and v; each of the six pointers may be NULL.  Waits for enqueued work.
 * murbtracer_download_forces: the remembered (a0, j0): after murbtracer_compute those of the current state, after a step
 *   those of the step's predicted end state (murbhip_download_jerk's rule).  Each output group (ax, ay, az), (jx, jy, jz) may
 *   be NULL.  Waits for enqueued work.  MURBHIP_E_STATE when no tracer evaluation is current.
 * murbtracer_compute: evaluates (a0, j0) of the tracers at the current state, enqueue-only; the tracers' counterpart of
 *   murbhip_compute_acc_jerk.  Does nothing when they are current.  MURBHIP_E_STATE before the bodies' first upload.
 * murbtracer_count, murbtracer_clear: the number of resident tracers; remove them (the buffers stay).
 *
 * State.
 *   Tracers need one shard and "integrator" 2: murbtracer_upload gives MURBHIP_E_STATE otherwise, and while a block is open
 *   (murbhip_evolve_block); murbtracer_clear is refused while a block is open too.
 *   While tracers are resident "integrator" cannot leave 2 ("contact"'s rule), and murbhip_evolve_block and
 *   murbhip_block_set_levels return MURBHIP_E_STATE.
 *   murbhip_upload, murbhip_init_bodies and murbhip_upload_radii keep the tracers' q and v and drop only their remembered
 *   evaluation.  "nearest", "contact" and "potential" may be on: tracers are no candidates and get no side product.
 *   murbfield.h's and murbtidal.h's read-outs change no tracer bit, and the tracers change none of theirs.
 *   MURBHIP_E_INVALID: a NULL context; a NULL position array; some but not all of the three velocity pointers NULL; a value that
 *   is not finite; some but not all pointers of an output group NULL; more than 2^30 tracers.
 *   A refused call changes nothing.
 * Not covered: block steps (murbhip_evolve_block); several shards or ranks; tracers' neighbours or contacts; tracers with mass;
 *   a flag of the command-line driver.
 */
#ifndef MURBTRACER_H_
#define MURBTRACER_H_

#include "murbhip.h"

#ifdef __cplusplus
extern "C" {
#endif

int murbtracer_upload(murbhip_ctx* ctx, unsigned long count, const float* qx, const float* qy, const float* qz, const float* vx,
                      const float* vy, const float* vz);
int murbtracer_download(murbhip_ctx* ctx, float* qx, float* qy, float* qz, float* vx, float* vy, float* vz);
int murbtracer_download_forces(murbhip_ctx* ctx, float* ax, float* ay, float* az, float* jx, float* jy, float* jz);
int murbtracer_compute(murbhip_ctx* ctx);
int murbtracer_count(murbhip_ctx* ctx, unsigned long* count);
int murbtracer_clear(murbhip_ctx* ctx);

/* Integer options.  Keys:
 *   "tracer_chunks"  j chunks a tracer's sums are cut into: exactly "field_chunks" of murbfield.h (0 (default) = tiles / 8 kept
 *                    within [1, 16]; k > 0 = k, clamped to the tile count), planned by the same function.  A function of the body
 *                    count and this option alone.  A change drops the tracers' remembered evaluation
 *   "tracer_batch"   tracers per sweep launch: exactly "field_batch" (a multiple of 16 up to 1 048 576; 0 (default) = 16 384).
 *                    Bounds the partial rows' memory.  No result depends on it
 *   "tracer_dt"      0 (default): the tracers follow the bodies' step; the bodies' trajectory, murbhip_evolve's out5 and every
 *                    read-out of the bodies are bit-identical to a run without tracers.  1: under murbhip_evolve each tracer's
 *                    Aarseth step (the bodies' criterion on its own a0, j0, a1, j1, same eta; eta_start |a0| / |j0| at the head
 *                    of a call without a proposal) also enters the step-size minimum: the tracers then change the bodies through
 *                    the step size alone.  With tracers resident a change drops murbhip_evolve's retained proposal, as an upload
 *                    or a clear does while the option is 1
 * Other keys and values: MURBHIP_E_INVALID.  murbtracer_get_option returns the value in force, defaults resolved.  With murbhip's
 * "profile" 2 the sweep launches of murbhip_step / murbhip_steps and murbtracer_compute are recorded as spans of a kind of their
 * own ("span_tracer_ms_avg", "span_tracer_count"); the force_* figures count force launches alone. */
int murbtracer_set_option(murbhip_ctx* ctx, const char* key, long value);
int murbtracer_get_option(murbhip_ctx* ctx, const char* key, long* value);

/* A testing and binding aid, not part of the contract above: what murbtracer_upload's argument check says to these arrays (0 or
 * MURBHIP_E_INVALID).  Host only, no device, no context; a caller of murbtracer_upload never needs it. */
int murbtracer_validate(unsigned long count, const float* qx, const float* qy, const float* qz, const float* vx, const float* vy,
                        const float* vz);

#ifdef __cplusplus
}
#endif

#endif
