/*
 * murbhip.h — C ABI of the MI355X-native all-pairs force + integrate path for MUrB.
 *
 * This is the drop-in boundary: everything the reference's `--im` implementations do on the
 * device side of SimulationNBodyInterface<T>::computeOneIteration()
 * (reference src/common/core/SimulationNBodyInterface.hpp:45) is reachable through these
 * entry points with plain pointers and sizes.  The only translation unit behind it that needs
 * hipcc is nbody-eurohpc_amd/csrc/murbhip.hip; host code (C++, or ctypes/cgo/JNI) links
 * libmurbhip.so and never sees a HIP header.
 *
 * Conventions
 *   - every function returns 0 on success, a negative value on failure:
 *       -1 … -1999    : -(hipError_t)
 *       -2000 … -2999 : MURBHIP_E_* argument / state errors
 *       -3000 … -3999 : -(3000 + ncclResult_t)
 *     murbhip_error_string() turns any of them into text.  The C++ wrapper maps non-zero to the
 *     reference's print-to-stderr + exit(code) convention
 *     (reference src/murb/implem/SimulationNBodyCUDATileFullDevice.cu:10-17).
 *   - a context is driven by ONE host thread (reference driver contract, src/murb/main.cpp:348-354).
 *   - step functions only enqueue work; murbhip_sync() is the per-iteration device sync the
 *     reference driver performs itself (src/murb/main.cpp:356-368).
 *   - arrays are fp32 SoA of n entries in the reference's body order (dataSoA_t,
 *     src/common/core/Bodies.hpp:15-24).  SIMD padding bodies (Bodies.cpp:201-213) are NOT passed
 *     in: they carry no mass and no implementation of the reference reads them in the j loop.
 */
#ifndef MURBHIP_H_
#define MURBHIP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Call orders.  A context remembers results of earlier calls (forces, the pair potential, the Hermite integrator's (a0, j0), its
 * step proposal, the metric sums, the bodies' levels) and every such shortcut is bit-identical to doing the work again.  Stated
 * once, for every entry point and option:
 *   Body-changing calls: murbhip_upload, murbhip_init_bodies, murbhip_upload_radii, murbhip_step(s), murbhip_evolve,
 *     murbhip_evolve_block, murbhip_integrate_host_acc, murbhip_block_set_levels, murbhip_set_encounter, and a murbhip_set_option
 *     that changes the value of any key not listed as result-neutral below.
 *   Observers: murbhip_compute_acc, murbhip_compute_acc_jerk, murbhip_energy, murbhip_moments, murbhip_potential_energy, every
 *     murbhip_download_*, murbhip_block_state, murbhip_evolve_dts, murbhip_encounters, murbhip_contacts, murbhip_sync,
 *     murbhip_warmup, murbhip_get_info; a value-changing set of a result-neutral key: "energy_sweep" (every murbhip_energy is
 *     the energy of the mode in force when it is called), "profile", "evolve_batch", "init_libm_fma"; and a change that is put
 *     back before the next body-changing call: "contact" 1 <-> 2, or murbhip_set_encounter(r) then (0).
 *   Refused calls: anything that returns MURBHIP_E_STATE or MURBHIP_E_INVALID.
 *   C1  Deleting every observer and every refused call from a sequence of calls changes no bit of anything read afterwards:
 *       state, accelerations and jerks, (nn, r2), (cp, gap2), phi, ticks and levels, out5 / out8, murbhip_evolve_dts and the hit
 *       lists, energies and moments.
 *   C2  An observer returns the bits it returns when it is the only observer at that point of the sequence.  murbhip_download_acc
 *       is meant as the pair murbhip_compute_acc; download or murbhip_compute_acc_jerk; download: on its own it returns what the
 *       evaluation that used the buffer last left there.
 *   C3  A refused call returns its documented code and changes nothing.
 *   C4  A value-changing murbhip_set_option of a key that enters the force plan or the layout of its partial rows — "variant",
 *       "jsplit", "taper", "diag_tri", "sym_red", "sym_waves", "sym_wide", "sym_pass_mb", "pad_aware", "xcd_order",
 *       "fuse_integrate", "overlap", "tri_first_pct", "tri_div" — drops the remembered forces and pair potential, and the metric
 *       sums kept for murbhip_energy / murbhip_moments with them.  It does not drop the Hermite memory or the levels, and it is
 *       no change of the bodies.  Results are thus a function of the state and of the options in force when the work is done,
 *       never of those in force when something was remembered.
 *   C5  While a block of murbhip_evolve_block is open, switching "nearest", "potential", or "contact" between 0 and non-zero is
 *       refused with MURBHIP_E_STATE.
 * tests/helpers/call_orders.py holds this classification as a table and tests/test_call_orders_gpu.py checks C1-C5 on sequences
 * generated from it. */
typedef struct murbhip_ctx murbhip_ctx;

#define MURBHIP_UNIQUE_ID_BYTES 128

#define MURBHIP_E_INVALID (-2000)   /* bad argument                                   */
#define MURBHIP_E_STATE (-2001)     /* call made in the wrong state (e.g. no upload)  */
#define MURBHIP_E_NO_DEVICE (-2002) /* no usable HIP device                           */
#define MURBHIP_E_NO_RCCL (-2003)   /* librccl could not be loaded                    */
#define MURBHIP_E_NOMEM (-2004)     /* host allocation failed                         */

/* ------------------------------------------------------------------ host-only helpers (no GPU needed) */

/* ABI version of this header (major*100 + minor). */
int murbhip_version(void);

/* Text for any return code of this library (static storage, never NULL). */
const char* murbhip_error_string(int code);

/* Block partition of n bodies over `world` ranks: first index and count of rank `rank`.
 * Same rule as the reference's MPI path: counts[r] = n/world + (r < n%world), displs = prefix sums
 * (reference src/murb/implem/SimulationNBodyMultiNode.cpp:76-91). */
int murbhip_partition(unsigned long n, int world, int rank, unsigned long* first, unsigned long* count);

/* Device slots each rank owns in the replicated position buffer: the largest slice rounded up to
 * the slice unit (a multiple of 1024 body slots).  Slots past a rank's count hold mass 0 and contribute
 * exactly 0 to every sum, so one equal-count all-gather replaces the reference's MPI_Allgatherv
 * (SimulationNBodyMultiNode.cpp:104-114). */
unsigned long murbhip_slice_slots(unsigned long n, int world);

/* Slot of body i in the replicated buffer (rank(i) * slice_slots + offset inside its slice). */
unsigned long murbhip_slot_of_body(unsigned long n, int world, unsigned long i);

/* The work list of rank `rank` under the multi-GPU pair-symmetric ("half ring") schedule: `*count`
 * items (i-side sub-block, j-side block), the first `*own_count` of which lie inside the rank's own slice.
 * A block is 1024 slots, a sub-block 1024/split.  Over all ranks every unordered pair of bodies is
 * covered exactly once (own-slice items cover both orders inside their diagonal blocks).  `pairs`
 * (2 ints per item, may be NULL to query the count) must hold `capacity` items.  Replaces the "who
 * computes what" of the reference's MPI path, which has every rank sweep all j for its i range
 * (SimulationNBodyMultiNode.cpp:151-170). */
int murbhip_schedule_items(unsigned long n, int world, int rank, int split, int* pairs, unsigned long capacity,
                           unsigned long* count, unsigned long* own_count);

/* Host only: the same work list as the pair-symmetric kernel consumes it, with the layout of its partial sums —
 * what murbhip_step builds for (n, world, rank) under the given plan (`split` i-side sub-blocks per block, `waves` 4 or 8
 * per workgroup, `taper_pct` % of each launch cut into finer items (+ 256: diagonal blocks as triangular pieces,
 * option "diag_tri"; + 512 x k, k = 0..3: the own-slice triangle's launches cut 2^k times finer, option "tri_div"), `tri_first_pct` % of the own-slice triangle in its first launch; exchange_mode != 0 or world > 1: the three-launch pipeline with separate rows for the own-slice
 * triangle).  Per item 8 longs: first i slot, number of i bodies, j block, flags, row set (0 main,
 * 1 own-slice triangle), float offset of its i-side output, of its j-side output, launch (0, 1, 2).
 * flags, exactly as the kernel reads them (MurbSymItem::flags, csrc/murb_kernels_sym.h; SymPiece, csrc/murb_schedule.h):
 *   bit 0      nothing is written on the j side (a diagonal item in its plain form - the full square with only the
 *              i side kept - or the LAST triangular piece of a diagonal block, which has no later step to apply)
 *   bit 1      diagonal item in its triangular form ("diag_tri"): the piece skips the j steps before its own
 *   bits 8-11  triangular form: first j step (of 128 bodies) the piece evaluates
 *   bits 12-15 triangular form: first j step whose terms are applied to BOTH sides (the steps before it, i.e. the
 *              piece's own, keep the i side only)  Per row-table
 * entry 7 longs: row set, destination slice chunk, block inside it, offset and count of its i rows, offset and count of
 * its j rows (rows are 1024 slots).  NULL arrays query the counts.  Exists so that "every cell of every row has exactly
 * one writer" and "every pair is evaluated once" can be checked without a GPU. */
int murbhip_schedule_layout(unsigned long n, int world, int rank, int split, int waves, int taper_pct, int tri_first_pct,
                            int exchange_mode, long* items, unsigned long item_capacity, unsigned long* item_count, long* rows,
                            unsigned long row_capacity, unsigned long* row_count, unsigned long* floats_main,
                            unsigned long* floats_tri);

/* ------------------------------------------------------------------ life cycle */

/* Number of visible HIP devices. */
int murbhip_device_count(int* count);

/* One GPU, whole problem.  Replaces what the reference does at construction of a device
 * implementation: CUDABodies allocation (src/common/core/CUDABodies.cu:12-31), acceleration and
 * GM buffers (SimulationNBodyCUDATileFullDevice.cu:181-199).  `g` is the gravitational constant
 * (SimulationNBodyInterface.hpp:18), `soft` the softening length (squared inside).
 * Units: any consistent system — SI, Henon units (G = M = 1), AU / solar masses / years.  `g` must be a finite number
 * greater than 0 (MURBHIP_E_INVALID otherwise, from every murbhip_create*: the upload folds G*m into the records and
 * murbhip_energy divides by it).  All arithmetic of the force path is fp32, so with r^2 = |q_j - q_i|^2 + soft^2 of any pair
 * (the self pair, r = soft, included), r^2, 1 / r^2, G m / r, the pair factor G m / r^3 and its products with the position and
 * velocity differences must be normal fp32 numbers; inside [2^-118, 2^120] for all of them every plan is within 2e-6 of an
 * fp64 evaluation ("Numeric domain").  Results scale exactly, bit for bit, under powers of two of the units.
 * `soft` == 0 is accepted, but the self pair is then 0 * inf = NaN on every plan, as in the reference. */
int murbhip_create(murbhip_ctx** out, unsigned long n, float soft, float g, int device);

/* One process driving `ndev` GPUs (bodies block-partitioned over them, positions exchanged every
 * step).  `devices` lists HIP device ordinals; the same ordinal may appear more than once (the
 * shards then share that GPU — used to exercise the sharded path on a one-GPU machine).
 * exchange: 0 = device-to-device copies and peer reads issued by this library, 1 = RCCL (all-gather of
 * positions, reduce-scatter of accelerations under the pair-symmetric schedule; ncclCommInitAll).
 * Threading: the CALLER stays single-threaded (the reference's driver contract, main.cpp:348-354), but the context owns
 * one host thread per shard that enqueues that shard's share of every step (murbhip_step returns when all of them have
 * finished enqueueing, never waits for the GPU); each thread drives its own communicator, no ncclGroupStart/End. */
int murbhip_create_sharded(murbhip_ctx** out, unsigned long n, float soft, float g, int ndev, const int* devices,
                           int exchange);

/* One process per GPU (torchrun / mpirun style).  Rank 0 calls murbhip_unique_id() and ships the
 * 128 bytes to every rank out of band; every rank then calls murbhip_create_rank().  Takes the place
 * of the reference's lazy MPI_Init/Comm_rank/Comm_size (SimulationNBodyMultiNode.cpp:62-73).
 * At most 64 ranks (MURBHIP_E_INVALID beyond: the per-slice tables of the half-ring schedule are fixed-size).
 * RCCL is bound at run time (librccl.so.1 by soname, so a host that already loaded RCCL shares it);
 * the environment variable MURBHIP_RCCL_LIBRARY names a specific library file to bind instead ("none": behave as
 * on a machine without RCCL: MURBHIP_E_NO_RCCL). */
int murbhip_unique_id(void* id_out /* MURBHIP_UNIQUE_ID_BYTES */);
int murbhip_create_rank(murbhip_ctx** out, unsigned long n, float soft, float g, int device, int rank, int world,
                        const void* unique_id);

int murbhip_destroy(murbhip_ctx* ctx);

/* ------------------------------------------------------------------ state in / out */

/* Host SoA -> device (all n bodies; every rank passes the full arrays, as every reference MPI rank
 * builds the full Bodies).  Replaces CUDABodies::memcpyBuffersOnDevice (CUDABodies.cu:34-49) and
 * devInitializeDevGM (SimulationNBodyCUDATileFullDevice.cu:41-45): G*m is folded in here. */
int murbhip_upload(murbhip_ctx* ctx, const float* qx, const float* qy, const float* qz, const float* vx,
                   const float* vy, const float* vz, const float* m);

/* Initial conditions generated ON THE DEVICE, instead of murbhip_upload: the n bodies of the reference's scheme "galaxy"
 * (Bodies::initGalaxy, src/common/core/Bodies.cpp:158-214) or "random" (initRandomly, :217-257) for srand(seed), bit-identical
 * to what the reference's host code computes on this machine — glibc's rand() sequence (jump-ahead on the linear TYPE_3
 * generator), the float/double mix of the reference's expressions as compiled with its flags, and glibc's sincosf
 * (csrc/murb_init.h).  Every shard fills its own copy of the replicated records; nothing crosses PCIe.  The host-side SIMD
 * padding bodies of the reference (Bodies.cpp:201-213) draw from rand() AFTER the n bodies and never reach the device.
 * Option "init_libm_fma": which build of glibc's sincosf to reproduce (1 = the -mfma one glibc selects on CPUs with FMA and
 * AVX2, 0 = the SSE2 one; -1, default = what this host's libm would pick). */
int murbhip_init_bodies(murbhip_ctx* ctx, const char* scheme, unsigned long seed);

/* Masses (and, after murbhip_init_bodies or murbhip_upload_radii, radii; `r` may be NULL; MURBHIP_E_STATE when it is not and no
 * radii were ever set) of all n bodies, device -> host: what a host mirror
 * needs to complete its dataSoA when the bodies were created on the device (rank mode: own slice only). */
int murbhip_download_mass(murbhip_ctx* ctx, float* m, float* r);

/* Device -> host SoA of all n bodies; waits for enqueued steps first.  This is the lazy D2H behind
 * CUDABodies::getDataSoA() (CUDABodies.cu:64-93).  Any pointer may be NULL.  In rank mode velocities
 * are only known for the caller's own slice: entries of other ranks are left untouched. */
int murbhip_download_state(murbhip_ctx* ctx, float* qx, float* qy, float* qz, float* vx, float* vy, float* vz);

/* Accelerations used by the most recent step (or murbhip_compute_acc), n entries each; other ranks'
 * entries untouched in rank mode.  Test hook, like getAccSoA()
 * (SimulationNBodyCUDATileFullDevice200k.cu:179-189). */
int murbhip_download_acc(murbhip_ctx* ctx, float* ax, float* ay, float* az);

/* ------------------------------------------------------------------ compute */

/* a_i = sum_j G m_j (q_j - q_i) / (|q_j - q_i|^2 + soft^2)^(3/2) for the current positions, no
 * integration.  Enqueue only.  (computeBodiesAcceleration: SimulationNBodyOptim.cpp:34-94,
 * device twin SimulationNBodyCUDATileFullDevice.cu:53-153.)  The result is remembered: a second call
 * without a state change in between costs nothing, and a murbhip_step() that follows directly reuses
 * the forces instead of evaluating them again (one shard; bit-identical either way). */
int murbhip_compute_acc(murbhip_ctx* ctx);

/* Accelerations AND their time derivatives ("jerks") in one all-pairs sweep, fp32, for the current positions and
 * velocities; no integration.  Enqueue only.  With d = q_j - q_i, w = v_j - v_i, r2 = |d|^2 + soft^2:
 *     a_i = sum_j G m_j d r2^(-3/2)          j_i = sum_j G m_j (w - 3 (d.w) d / r2) r2^(-3/2)
 * (csrc/murb_kernels_hermite.h; one shard only: MURBHIP_E_STATE otherwise, see "integrator" 2).  The result is remembered
 * like murbhip_compute_acc's: a second call without a state change in between costs nothing, and a Hermite step that
 * follows directly starts from it as its (a0, j0) — bit-identical either way.  After a Hermite step the remembered
 * evaluation is that step's own (a1, j1, taken at its predicted state: what the next step starts from), and the call
 * leaves it as it is.  murbhip_download_acc returns the accelerations (also when a force evaluation — murbhip_compute_acc,
 * murbhip_energy — used that buffer in between: the call then puts them back), murbhip_download_jerk the jerks. */
int murbhip_compute_acc_jerk(murbhip_ctx* ctx);

/* Jerks of the remembered acceleration + jerk evaluation (murbhip_compute_acc_jerk, or the last Hermite step), n entries
 * each; waits for enqueued work first.  Test hook, like murbhip_download_acc.  MURBHIP_E_STATE when no such evaluation is
 * current (none yet, or the bodies changed since: upload, device initialisation, murbhip_integrate_host_acc, a step of
 * another integrator). */
int murbhip_download_jerk(murbhip_ctx* ctx, float* jx, float* jy, float* jz);

/* Advance the bodies by `duration` seconds of model time with Hermite steps ("integrator" 2) whose common size the device
 * chooses (Makino & Aarseth 1992; Aarseth's criterion).  All bodies take the same step.  With |x| the Euclidean norm, (a0, j0)
 * and (a1, j1) the evaluations at both ends of the step of size dt just taken, for every real body (massless ones included)
 *     a2 = (-6 (a0 - a1) - dt (4 j0 + 2 j1)) / dt^2     a3 = (12 (a0 - a1) + 6 dt (j0 + j1)) / dt^3     a2 += dt a3
 *     dt_i = sqrt( eta (|a1| |a2| + |j1|^2) / (|j1| |a3| + |a2|^2) )
 * and the next step is min_i dt_i clamped to [dt_min, dt_max]; a dt_i that is not a finite positive number (0/0 for a lone
 * body) counts as +inf.  The first step of a call that finds no proposal — the remembered (a0, j0) were not left by an
 * adaptive step — is eta_start * min_i |a0| / |j0|, clamped likewise.  A candidate >= duration - t becomes
 * (float)(duration - t): that step is the last, and the clock is set to `duration` exactly.  No growth limiter.  The
 * criterion is evaluated in fp64 without contraction in the order fixed in csrc/murb_kernels_adaptive.h
 * (murb_evolve_body_step), and the chosen step is rounded once to fp32; the steps themselves are murbhip_step's,
 * bit for bit.  Step size, clock and the end of the run live on the device: the host enqueues batches of steps and looks
 * at the control block once per batch (one stream sync), so the call returns after a sync.
 *   out5 = { model time advanced, steps taken, smallest step, largest step, the clamped step proposed for the next one }.
 * max_steps ends the run early with code 0 and out5[0] < duration.  The remembered (a1, j1) serve the next step or the
 * next call like a Hermite step's (murbhip_download_acc / murbhip_download_jerk return them), together with the proposal;
 * any other change of the bodies drops all three.  murbhip_step and murbhip_evolve may be mixed.
 * MURBHIP_E_STATE unless "integrator" is 2 and the context has one shard; MURBHIP_E_INVALID for duration <= 0, eta <= 0,
 * eta_start <= 0, a dt_max that is not finite or <= 0, dt_min < 0, dt_min > dt_max, max_steps == 0. */
int murbhip_evolve(murbhip_ctx* ctx, double duration, double eta, double eta_start, float dt_min, float dt_max,
                   unsigned long max_steps, double* out5);

/* The step sizes the last murbhip_evolve used, oldest first.  The device keeps the last 4096 of a call; *count = how many
 * are kept (dts may be NULL to ask for the count alone; MURBHIP_E_INVALID when capacity is smaller).  Waits for enqueued
 * work. */
int murbhip_evolve_dts(murbhip_ctx* ctx, float* dts, unsigned long capacity, unsigned long* count);

/* Advance the bodies by `blocks` blocks of dt_max seconds with Hermite steps ("integrator" 2) of INDIVIDUAL size: every body
 * takes steps of its own, dt_i = dt_max 2^-k_i with a level k_i in [0, kmax] (hierarchical "block" steps, Makino 1991), so that
 * one tight pair no longer sets the step of every body.
 *   Time.  A block is cut into T = 2^kmax ticks.  Body i holds its level k_i and its own time t_i in ticks, an unsigned 32-bit
 *   number in [0, T); its step is T >> k_i ticks.  All bookkeeping is in integers, no floating-point time is accumulated:
 *   seconds are only ever formed as (double)ticks * ((double)dt_max * 2^-kmax), which is exact for kmax <= 20, and
 *   dt_i = dt_max 2^-k_i is exact in fp32.
 *   One block step:
 *    1. t_next = min_i (t_i + (T >> k_i)); the active set is every real body (massless ones included) that attains it.
 *    2. EVERY body is predicted to t_next with its own dt = (t_next - t_i) ticks in seconds, the exact fp64 value, by the
 *       predictor of a Hermite step (the fp64 coefficients dt, dt*dt*0.5, dt*dt*dt/6 formed from that dt; one rounding to
 *       fp32 per stored value).  An inactive body's q, v, a0, j0, t_i, k_i are not touched by the step, bit for bit.
 *    3. (a1, j1) of the active bodies only, at the predicted state of all n bodies (murbhip_compute_acc_jerk's arithmetic).
 *    4. Each active body is corrected from its own (q, v, a0, j0) at t_i with its dt_i, by the corrector of a Hermite step,
 *       in place; then (a0, j0) <- (a1, j1) and t_i <- t_next (0 when t_next == T).
 *    5. Its new level: req = murbhip_evolve's dt_i from (a0, j0, a1, j1, dt_i, eta), rounded to fp32 (+inf where that is not a
 *       finite positive number); k_req = the smallest k in [0, kmax] with dt_max 2^-k <= req (+inf gives 0); if no k qualifies,
 *       k_req = kmax and the step counts as CLAMPED (the cap is too coarse for that body: look at out8[5]).  If k_req > k_i:
 *       k_i <- k_req (several halvings at once are allowed).  Else if k_req < k_i and t_next is a multiple of 2 (T >> k_i):
 *       k_i <- k_i - 1 (one doubling, and only where the coarser grid has a point).  Else k_i stays.
 *    6. At t_next == T every body is active (all steps divide T): the block ends with all bodies synchronised.
 *   The call ends after `blocks` such boundaries, or after max_steps block steps, possibly inside a block.
 *   Starting levels.  Those a previous call left are kept when that call ended synchronised, dt_max and kmax are the same and
 *   nothing changed the bodies in between; otherwise k_i = k_req(eta_start |a0_i| / |j0_i|) (murbhip_evolve's starting rule per
 *   body, fp32) from the remembered evaluation or a fresh one.  A call that finds the context inside a block continues that
 *   block with the same dt_max and kmax (MURBHIP_E_STATE for others); `blocks` counts the boundaries still to reach.
 *   out8 = { model time advanced in seconds, block steps, body-steps (sum of the active sets' sizes: what the N^2 sweep is
 *            paid for), smallest dt_i used, largest, clamped steps, largest active set, 1 if synchronised at return }.
 * The active set, its size and the end of the run live on the device; the host enqueues batches of at most 64 block steps and
 * looks at the control block once per batch ("evolve_batch" fixes the batch length here too).  The order of the active list
 * is unspecified and no result depends on it: results are bit-reproducible from run to run.
 * MURBHIP_E_STATE unless "integrator" is 2 and the context has one shard; MURBHIP_E_INVALID for a dt_max that is not finite or
 * <= 0, blocks == 0, eta <= 0, eta_start <= 0, kmax outside 0 ... 20, dt_max 2^-kmax not a normal fp32 number, max_steps == 0.
 * While a block is open (a max_steps stop), murbhip_step(s), murbhip_evolve, murbhip_compute_acc, murbhip_compute_acc_jerk,
 * murbhip_energy, murbhip_moments and murbhip_warmup return MURBHIP_E_STATE; murbhip_upload, murbhip_init_bodies and
 * murbhip_integrate_host_acc close it and drop the levels; murbhip_download_state / _acc / _jerk return every body at its own
 * time (a test hook).  After a synchronised return the remembered (a0, j0) serve murbhip_step, murbhip_evolve and
 * murbhip_download_acc / _jerk exactly as a Hermite step's do. */
int murbhip_evolve_block(murbhip_ctx* ctx, float dt_max, unsigned long blocks, double eta, double eta_start, int kmax,
                         unsigned long max_steps, double* out8);

/* Test hooks of murbhip_evolve_block, like murbhip_download_jerk.  murbhip_block_state: the bodies' own times (ticks) and levels,
 * n entries each, either pointer may be NULL; waits for enqueued work; MURBHIP_E_STATE before the first murbhip_evolve_block or
 * murbhip_block_set_levels.  murbhip_block_set_levels: the next murbhip_evolve_block with that kmax starts from these levels
 * (all bodies at tick 0) instead of the starting rule; any change of the bodies drops them.  MURBHIP_E_INVALID for a level
 * outside [0, kmax], MURBHIP_E_STATE while a block is open or unless "integrator" is 2 with one shard. */
int murbhip_block_state(murbhip_ctx* ctx, unsigned int* ticks, int* levels);
int murbhip_block_set_levels(murbhip_ctx* ctx, const int* levels, int kmax);

/* Nearest neighbours from the Hermite sweeps, and an encounter stop.
 *   Option "nearest" (0 default, 1; one shard with "integrator" 2 only, MURBHIP_E_STATE otherwise).  With 1, every acceleration
 *   and jerk evaluation — murbhip_compute_acc_jerk, the sweep of a Hermite murbhip_step, the sweeps of murbhip_evolve, the active
 *   sweep and the starting evaluation of murbhip_evolve_block — also keeps, per real body i,
 *       nn_i   the index (in the caller's order, not a slot) of the nearest other real body, and
 *       r2_i   the sweep's own fp32 value fma(dz,dz, fma(dy,dy, fma(dx,dx, soft^2))) of that pair, d = q_j - q_i: softening
 *              included, the very number the force arithmetic used.
 *   Candidates are all real bodies j != i, massless ones included; never the body itself (its r2 = soft^2 is the smallest of
 *   all) and never the zero-mass padding slots that fill the layout up to whole blocks of 1024.  The minimum is lexicographic
 *   in (r2 as fp32, index): among equal r2 the lowest index wins, so the result does not depend on how the j range is cut
 *   ("jsplit", "block_units", the order of the active list) nor on the run: equal bits.  r2(i,j) == r2(j,i) bit for bit
 *   (negating the differences is exact).  A lone body (n = 1) gets index -1 and r2 = +inf.
 *   The values belong to the evaluation that produced them: after a step they are taken at that step's predicted end state,
 *   like (a1, j1).  Under block steps only the active bodies' entries are refreshed; an inactive body keeps its (nn, r2) bit
 *   for bit, exactly as it keeps its (a0, j0).  Switching the option drops the remembered evaluation, so a remembered
 *   (a0, j0) always has its neighbours beside it, and is refused (MURBHIP_E_STATE) while a block is open: the bodies sit at
 *   their own times and only some of them would have neighbours.  With 0 every result is what it was without the option, bit for bit.
 *   The nearest-neighbour sweeps are kernels of their own (csrc/murb_kernels_side.h; DESIGN.md 4.9 has their cost).
 * murbhip_download_nearest: n entries each, either pointer may be NULL; waits for enqueued work.  MURBHIP_E_STATE when
 *   "nearest" is 0 or no such evaluation is current (murbhip_download_jerk's rule; while a block is open it returns every
 *   body's values at its own time, like the other download hooks).
 * murbhip_set_encounter: radius 0 (default) = off; radius > 0 needs "nearest" 1 (MURBHIP_E_STATE otherwise, and setting
 *   "nearest" to 0 while a radius is set is refused the same way); not finite or < 0: MURBHIP_E_INVALID.  With
 *       thr = (float)((double)radius * radius + (double)soft^2)
 *   a step of murbhip_evolve or murbhip_evolve_block in which any body that took the step has r2_i <= thr is a hit: the step
 *   completes as usual (corrector, clock, counters, levels), the run ends behind it and the call returns 0 with
 *   out5[0] < duration, or with out8[7] == 0 if it stopped inside a block (the open block behaves exactly as after a
 *   max_steps stop).  A call always takes at least one step.  murbhip_step(s) never stops; it only keeps the neighbours.
 * murbhip_encounters: the pairs (i, nn_i, r2_i) of the hitting step, sorted by i; the device keeps at most 4096 of them,
 *   *count says how many there were (0: the last evolve call ended otherwise); `time` = the model time advanced in that call
 *   when the hit was seen.  The list is cleared at the head of every evolve call.  NULL arrays ask for the count (and time)
 *   alone; MURBHIP_E_INVALID when capacity < min(*count, 4096).
 * Not covered: several shards or ranks; the other integrators and the pair-symmetric force kernel; full neighbour lists
 * (an interface of their own, murbnbr.h: all bodies within a radius; per-body radii: "contact" below). */
int murbhip_download_nearest(murbhip_ctx* ctx, int* idx, float* r2);
int murbhip_set_encounter(murbhip_ctx* ctx, float radius);
int murbhip_encounters(murbhip_ctx* ctx, int* i, int* j, float* r2, unsigned long capacity, unsigned long* count, double* time);

/* Contacts by the bodies' radii from the Hermite sweeps, and a contact stop.
 *   Definition.  For real bodies i != j take r2_ij as the sweep's own fp32 value fma(dz,dz, fma(dy,dy, fma(dx,dx, soft2))) and
 *   soft2 as the fp32 the sweep uses.  Then, each line one fp32 operation:
 *       s_ij    = R_i + R_j
 *       e_ij    = r2_ij - soft2
 *       gap2_ij = fmaf(-s_ij, s_ij, e_ij)
 *   gap2 is the squared centre distance minus the squared sum of radii; the pair is in contact iff gap2_ij <= 0.
 *   gap2_ij == gap2_ji bit for bit (r2 is symmetric, the add commutes); a result of -0 cannot arise, so values compare as fp32
 *   numbers.  Per real body i the sweep keeps (cp_i, gap2_i): the lexicographic minimum of (gap2 as fp32, index in the caller's
 *   order) over all real bodies j != i, massless ones included; never the body itself, never the zero-mass padding slots.  A
 *   lone body gets -1 and +inf.  With all radii 0 cp_i is the geometrically nearest body.  In general it is NOT the nearest
 *   neighbour: a large body further away can overlap a body whose nearest neighbour does not touch it.  The bits do not depend
 *   on "jsplit", "block_units", the order of the active list, or the run.  The values belong to the evaluation that produced
 *   them (after a step: its predicted end state, like (a1, j1)); under block steps only the active bodies' entries are
 *   refreshed and an inactive body keeps its (cp, gap2) bit for bit.  Domain: radii finite and >= 0, s*s a finite fp32; r2's
 *   own rules are unchanged.
 *   Option "contact" (0 default, 1, 2; other values MURBHIP_E_INVALID; one shard with "integrator" 2 only, MURBHIP_E_STATE
 *   otherwise, and while it is non-zero "integrator" cannot leave 2).  1 keeps (cp, gap2) beside every acceleration + jerk
 *   evaluation — the evaluations "nearest" lists; 2 also turns the contact stop on.  It excludes "nearest": setting either to
 *   non-zero while the other is non-zero is MURBHIP_E_STATE (both use the same storage).  Switching between 0 and non-zero
 *   drops the remembered evaluation and is refused (MURBHIP_E_STATE) while a block is open; switching between 1 and 2 keeps
 *   the evaluation and an open block.  With 0 every result is what it was without the option, bit for bit.
 * murbhip_upload_radii: n radii in the caller's order.  MURBHIP_E_INVALID for NULL, a value that is not finite or a negative
 *   one; MURBHIP_E_STATE while a block is open or on a context of several shards or ranks.  Radii are 0 until first set;
 *   murbhip_upload leaves them as they are, murbhip_init_bodies replaces them with the scheme's.  Drops the remembered
 *   evaluation when "contact" is non-zero.  murbhip_download_mass(m, r) returns them afterwards.
 * murbhip_download_contact: murbhip_download_nearest's rules: n entries each, either pointer may be NULL; waits for enqueued
 *   work; MURBHIP_E_STATE when "contact" is 0 or no such evaluation is current; while a block is open it returns every body's
 *   values at its own time.
 * Contact stop ("contact" 2): a step of murbhip_evolve or murbhip_evolve_block in which any body that took the step has
 *   gap2_i <= 0 is a hit: the step completes as usual, the run ends behind it, with out5 / out8 and the open block exactly as
 *   after an encounter hit.  A call always takes at least one step.  murbhip_step(s) never stops.
 * murbhip_contacts: murbhip_encounters' semantics for the triples (i, cp_i, gap2_i) of the hitting step: sorted by i, at most
 *   4096 kept, *count says how many there were, cleared at the head of every evolve call.  While "contact" is non-zero
 *   murbhip_encounters reports 0, and murbhip_contacts reports 0 while it is 0.
 * Not covered: several shards or ranks; the other integrators; merging or removing bodies on the device (the Python helper
 *   murbhip.merge_contacts resolves a hit list on the host); restitution; "nearest" and "contact" at once. */
int murbhip_upload_radii(murbhip_ctx* ctx, const float* r);
int murbhip_download_contact(murbhip_ctx* ctx, int* idx, float* gap2);
int murbhip_contacts(murbhip_ctx* ctx, int* i, int* j, float* gap2, unsigned long capacity, unsigned long* count, double* time);

/* Per-body potential beside the Hermite sweeps ("integrator" 2): the quantity the force arithmetic forms on the way to the
 * pair factor, kept instead of thrown away — one more packed instruction per pair of interactions, no second N^2 pass.
 *   Definition.  For every real body i, massless ones included,
 *       phi_i = sum over real bodies j != i of  G m_j * inv_ij
 *   with inv_ij the sweep's own v_rsq_f32 of its own fp32 r2_ij = fma(dz,dz, fma(dy,dy, fma(dx,dx, soft2))): every term is the
 *   sweep's own G m_j * inv.  The sign is positive, like the "energy_sweep" potential phi_i = sum_j G m_j / r.  The body's own
 *   term G m_i / soft is left out BY SLOT: it is never added to an fp32 sum and subtracted again (with a small softening it is
 *   orders of magnitude above the pair terms and would take their low bits with it).  Another real body at the same position
 *   does count, with G m_j / soft: the exclusion is by slot, not by d == 0 or r2 == soft2.  Padding has G m = 0 and adds
 *   exactly +0.  A lone body gets +0.0f; with soft == 0 the forces' rule holds (NaN).  Summation is fp32 throughout — the
 *   lanes, the wave, then the partial rows in chunk order beside (a1, j1) — so the value depends on "jsplit" / "block_units"
 *   only through that cut, like the accelerations, and is bit-reproducible from run to run.  Domain: G m / r a normal fp32
 *   number, as murbhip_create already requires.  The values belong to the evaluation that produced them, like (a1, j1) and
 *   (nn, r2): after murbhip_compute_acc_jerk the current state, after a step that step's PREDICTED end state; under block
 *   steps only the active bodies' entries are refreshed and an inactive body keeps its phi bit for bit (at a synchronised
 *   boundary every body was active in the last block step, so all values belong to one state).
 *   Option "potential" (0 default, 1; other values MURBHIP_E_INVALID; one shard with "integrator" 2 only, MURBHIP_E_STATE
 *   otherwise, and while it is 1 "integrator" cannot leave 2).  It excludes "nearest" and "contact": setting it to non-zero
 *   while either is non-zero is MURBHIP_E_STATE, and so is setting either to non-zero while it is 1 (all three use the
 *   partial rows' fourth floats).  Switching it drops the remembered evaluation and is refused (MURBHIP_E_STATE) while a block
 *   is open.  With 0 every result is what it was without the option, bit for bit; with 1 accelerations, jerks, states, step
 *   sizes, levels and ticks are bit-identical to those with 0 under the same "jsplit" / "block_units".
 * murbhip_download_potential: n entries in the caller's order; waits for enqueued work.  MURBHIP_E_STATE when "potential" is 0
 *   or no such evaluation is current (murbhip_download_jerk's rule); while a block is open it returns every body's value at
 *   its own time.
 * murbhip_potential_energy: *w = -1/2 sum_i m_i phi_i of the remembered evaluation, summed in fp64 on the device in fixed
 *   order (the block sums of murbhip_energy's metrics, the masses as uploaded).  The download's state rules.  It is allowed
 *   while a block is open — a diagnostic where murbhip_energy refuses; the bodies' values then sit at their own times.  After
 *   a step the value belongs to the step's PREDICTED end state, not the corrected one: murbhip_energy remains the energy of
 *   the current state.
 * Not covered: several shards or ranks; the other integrators and the pair-symmetric kernel; "potential" together with
 *   "nearest" or "contact". */
int murbhip_download_potential(murbhip_ctx* ctx, float* phi);
int murbhip_potential_energy(murbhip_ctx* ctx, double* w);

/* Untimed device warm-up for about `milliseconds` (0 ... 10 000) of force evaluations on the current state, then a sync.
 * An MI355X needs ~40 ms of work to reach its steady clock after an idle spell (the first 12 ms run 25 % slow, DESIGN.md
 * §4.5) — as long as the reference's whole 200-iteration run at N = 30 000.  Construction is outside the reference's timing
 * window (main.cpp:353-371 times computeOneIteration() + the driver's sync only; the upload and the GM precompute of
 * SimulationNBodyCUDATileFullDevice.cu:191-215 are not in it), and this belongs there.  The state does not change and
 * nothing is remembered: the step that follows evaluates its own forces.  The number of evaluations is a function of n and
 * the number of ranks only (rank mode: the same count, hence the same collectives, on every rank). */
int murbhip_warmup(murbhip_ctx* ctx, double milliseconds);

/* One iteration = force + position/velocity update [+ position exchange].  Enqueue only.
 * (computeOneIteration: SimulationNBodyCUDATileFullDevice.cu:203-236; integrator semantics
 * Bodies.cpp:260-278 / CUDABodies.cu:126-153, including the fp64 intermediates.) */
int murbhip_step(murbhip_ctx* ctx, float dt);

/* `iterations` calls of murbhip_step in one go. */
int murbhip_steps(murbhip_ctx* ctx, float dt, int iterations);

/* Integrator alone with caller-supplied accelerations (host SoA, n entries): the overload
 * CUDABodies::updatePositionsAndVelocities(const accSoA_t&, T&) (CUDABodies.cu:355-370) that the
 * reference's test_CUDABodies.cpp:42-75 drives. */
int murbhip_integrate_host_acc(murbhip_ctx* ctx, const float* ax, const float* ay, const float* az, float dt);

/* Wait for everything enqueued on this context; returns the first asynchronous error, if any. */
int murbhip_sync(murbhip_ctx* ctx);

/* Mechanical energy of the current state: kinetic = sum 1/2 m v^2, potential = -1/2 sum_i sum_{j != i}
 * G m_i m_j / sqrt(r_ij^2 + soft^2) — the per-iteration metric of the reference's gpu+tracking
 * implementation (SimulationNBodyCUDAPropertyTracking.cu:217-304, summed there with cub).
 * Pair-symmetric plan (round 3): the potential comes out of a FORCE evaluation — two more packed instructions per 18 sum
 * G m_i G m_j / r of every pair a wave meets, one float per group of 4 i bodies behind the partial rows, fp64 from there on —
 * so there is no second N^2 sweep; the forces of that evaluation are remembered (bit-identical to a plain evaluation's),
 * and a step that follows directly only launches the state update (with several shards: state update + position
 * exchange).  A tracked iteration (energy, then step: `--im hip+tracking`) therefore costs ONE force evaluation: 6.9 ms
 * instead of 10.2 at N = 200 000 (6.1 untracked).  The pairs INSIDE a block of 1024 bodies are summed by a small kernel of their
 * own, in fp64 and without the bodies' own terms: the result is within 3e-8 of an fp64 evaluation from a few dozen bodies up.
 * Under the multi-pass evaluation (N > 2.4 M) the groups' sums are added up pass by pass.  In rank mode the potential covers the PAIRS this rank evaluated under the half-ring
 * schedule, the kinetic energy its own bodies: sum both over the ranks; the call is a collective (the force evaluation
 * contains the reduce-scatter) unless the forces of the current positions are already remembered.
 * One-sided plan (below 2 049 bodies; few bodies per rank) or option "energy_sweep" 1: one N^2 potential sweep on the device
 * (phi_i = sum_j G m_j / r), then -1/2 sum m_i phi_i; values cover the caller's own bodies.  On the one-sided plan the
 * sweep leaves a body's own term G m_i / soft out of its sum (by slot), instead of removing it from the fp32 total as the
 * reference does (.cu:287-294): with a small softening that term is orders of magnitude above the others (1e4 x for two
 * bodies of 1e30 kg 1e10 m apart at soft = 1e6 m) and took the low bits of the pair terms with it.
 * The per-body terms are summed in fp64 on the device (256-body block sums in a fixed order; the host adds the few hundred
 * block rows); waits for enqueued steps. */
int murbhip_energy(murbhip_ctx* ctx, double* kinetic, double* potential);

/* First moments of the current state, fp64 sums (on the device, like murbhip_energy) over the caller's own bodies:
 *   out10 = { Px, Py, Pz,  Lx, Ly, Lz,  Mx, My, Mz,  M }
 * linear momentum sum m v, angular momentum sum m (q x v), mass-weighted position sum m q and total
 * mass (centre of mass = M{x,y,z} / M).  These fill the ang_momentum / density_center columns the
 * reference's SimulationHistory reserves but never computes (SimulationHistory.hpp:13-15,
 * SimulationNBodyCUDAPropertyTracking.cu:5-8: only COMPUTE_ENERGY_METRIC is enabled).  In rank mode
 * sum the ten values over ranks. */
int murbhip_moments(murbhip_ctx* ctx, double* out10);

/* ------------------------------------------------------------------ tuning and measurement */

/* Integer options.  Keys:
 *   "variant"        force kernel variant.  0 = auto: the pair-symmetric kernel (8) on one
 *                    GPU from 4 097 bodies (5 blocks of 1024) up, except at 6 blocks, and in multi-GPU runs when a rank gets
 *                    >= 400 block pairs, the one-sided kernel otherwise (1; 2 = four i bodies per wave for a rank's slice of up
 *                    to 16 384 bodies; one GPU: with the state update in the tail of its launch, see "fuse_integrate").  1-6: one-sided variants, 7: persistent schedule
 *                    A plan key: a value-changing set drops the remembered forces and pair potential (C4)
 *   "jsplit"         one-sided variants: number of j-chunks a body's sum is split into; variant 7:
 *                    scheduling rounds; variant 8: i-side sub-blocks per item (1, 2, 4, 8, 16).  0 = auto
 *                    A plan key: a value-changing set drops the remembered forces and pair potential (C4)
 *   "taper"          variant 8: percentage (0..100) of each launch's work whose items are cut finer (the last
 *                    taper % in halves, the last taper/2 % in quarters): a shorter drain phase at the end of a launch.
 *                    -1 (default) = the plan's own choice
 *                    A plan key: a value-changing set drops the remembered forces and pair potential (C4)
 *   "sym_pass_mb"    variant 8, one GPU: budget in MiB for the partial sums of one pass (0 = default: a quarter of the
 *                    device memory).  A problem whose partial sums exceed it (N > ~2.4 M bodies by default) is
 *                    evaluated in several passes over ranges of j columns that share one buffer, their row sums
 *                    accumulated in fp64 ("sym_passes" of murbhip_get_info says how many)
 *                    A plan key: a value-changing set drops the remembered forces and pair potential (C4)
 *   "diag_tri"       variant 8: 1 = a diagonal block (i block = j block) is cut into pieces of 128 i bodies that only
 *                    evaluate the j bodies from their own position on (36 instead of 64 units of work per diagonal
 *                    block); 0 = the full square with the i side kept.  -1 (default) = the plan's own choice
 *                    A plan key: a value-changing set drops the remembered forces and pair potential (C4)
 *   "sym_red"        variant 8: how the i-side sums of a group are folded over the wave: 0 = in registers (permlane
 *                    swaps + DPP), 1 = through LDS (fewer VALU instructions).  -1 (default) = the plan's own choice
 *                    A plan key: a value-changing set drops the remembered forces and pair potential (C4)
 *   "sym_waves"      variant 8: waves per workgroup, 4 or 8; 0 = auto (one GPU up to 27 blocks: 8 or 4 by a measured table per
 *                    block count together with the item length, profiles/r03_small_plan_table.txt; 4 otherwise)
 *                    A plan key: a value-changing set drops the remembered forces and pair potential (C4)
 *   "sym_wide"       variant 8: the pair factor as (G m / r) (1 / r^2), one packed multiply more per 4 pair terms (+6 %), instead
 *                    of G m (1 / r^3), whose cube leaves the normal fp32 range for r beyond 2^42 length units.  -1 (default) =
 *                    chosen by every murbhip_upload: 1 where the diagonal of the bodies' bounding box and the softening, added
 *                    in quadrature, exceed 2^34 length units (2^8 of headroom for the system to expand) or the softening is
 *                    below 2^-40, else 0; murbhip_init_bodies keeps 0.  0 / 1 force a form
 *                    A plan key: a value-changing set drops the remembered forces and pair potential (C4)
 *   "pad_aware"      variant 8: 1 (default) = the zero-mass padding slots that fill a slice up to whole blocks of 1024 are
 *                    not walked: the emptier block of a pair goes on the walked (i) side and its items end at its last
 *                    real body; 0 = every block as if full (kept for the A/B: -3 % at N = 30 000, -4 % for a rank of 8
 *                    at N = 200 000)
 *                    A plan key: a value-changing set drops the remembered forces and pair potential (C4)
 *   "tri_div"        variant 8, several ranks: the items of the own-slice triangle's two launches (which run under the two
 *                    collectives and, with few blocks per slice, do not fill the chip) cut into 1, 2, 4 or 8 parts more
 *                    than the rectangles' items; 0 (default) = the plan's choice (~2 rounds of workgroups per launch)
 *                    A plan key: a value-changing set drops the remembered forces and pair potential (C4)
 *   "energy_sweep"   murbhip_energy on a pair-symmetric plan: 1 = the separate potential sweep of rounds 1-2 instead of the
 *                    pair potential summed inside a force evaluation (default 0); kept for the A/B and as a cross-check
 *   "xcd_order"      variant 8: 0 (default) = j-major item order (round-robin dispatch then gives XCD x the i
 *                    blocks x mod 8 of every j block); 1 = one contiguous run of items per XCD (measured:
 *                    more L2 misses, same time; kept for the comparison)
 *                    A plan key: a value-changing set drops the remembered forces and pair potential (C4)
 *   "profile"        1: bracket every force kernel with HIP events (read with murbhip_get_info); 2: also both collectives
 *                    on the exchange stream, the compute stream's waits for them (the EXPOSED part of the exchange) and
 *                    the compute stream's whole step - ~16 more event records per step, meant for a short diagnostic
 *                    run next to the timed one.  Setting it (to any value) drains the device and clears the samples
 *   "overlap"        sharded/rank mode: 0 = no overlap; 1 (default) = the own-slice work brackets the
 *                    exchanges on the compute stream; 2 = the own-slice triangle runs on a second,
 *                    lowest-priority compute stream next to the rectangle launch (pair-symmetric only)
 *                    A plan key: a value-changing set drops the remembered forces and pair potential (C4)
 *   "integrator"     0 (default) = the reference's update, Bodies.cpp:260-278; 1 = kick-drift-kick
 *                    leapfrog, the scheme the reference's gpu+leapfrog states (CUDABodies.cu:172-178) with
 *                    the force taken at the positions it belongs to: one force evaluation per step, the
 *                    device keeps v_{n-1/2}, murbhip_download_state applies the closing half kick (one
 *                    extra force evaluation; a collective in rank mode).  Cannot be changed between a
 *                    leapfrog step and the next murbhip_upload (MURBHIP_E_STATE); 2 = 4th-order Hermite
 *                    predictor-corrector (Makino & Aarseth 1992) in place of Bodies.cpp:260-278: predict q, v from
 *                    the remembered accelerations and jerks, ONE acceleration + jerk sweep at the predicted state
 *                    (murbhip_compute_acc_jerk's kernel, about twice the arithmetic of a force evaluation), correct;
 *                    the first step after a change of the bodies evaluates (a0, j0) at the current state first.
 *                    dt may change from step to step.  Device velocities are whole-step values: no closing kick, and
 *                    the option may be switched away from 2 at any time.  Single shard only: the sweep reads the
 *                    velocities of ALL bodies, which sharded and rank-mode contexts keep for their own slice alone
 *                    (they exchange positions, never velocities), so on a context of several shards or ranks, or
 *                    with "force_exchange" set, the value 2 is refused with MURBHIP_E_STATE (and "force_exchange"
 *                    is refused while the value is 2).  murbhip_evolve drives the same steps with sizes the device chooses,
 *                    murbhip_evolve_block gives every body a step of its own
 *   "evolve_batch"   murbhip_evolve: steps enqueued between two looks at the device's control block.  0 (default) = as
 *                    many as the remaining time takes at the step last seen, 64 at the most; 1..64 = exactly that many
 *                    (timing aid: a batch longer than the run needs ends in launches that find the done flag set and do
 *                    nothing, which tools/hermite_adaptive_rate.py times).  The results do not depend on it
 *   "init_libm_fma"  murbhip_init_bodies: which build of glibc's sincosf the device reproduces (-1 default, 0, 1; see there).  Read
 *                    by murbhip_init_bodies alone: result-neutral for everything else
 *   "block_units"    murbhip_evolve_block: U, the number of (group of 16 active bodies, j chunk) work units the active sweep
 *                    is cut into at least: chunks = ceil(U / groups) clamped to [1, layout tiles].  0 (default) = one per
 *                    workgroup the chip holds at once (5 per CU; info "block_units" / "block_grid"); up to 65 536.  The
 *                    results depend on it only through the chunk cut of the fp32 row sums
 *   "nearest"        0 (default), 1: the Hermite sweeps also keep every body's nearest neighbour and its r2 (see
 *                    murbhip_download_nearest above).  One shard with "integrator" 2 only (MURBHIP_E_STATE otherwise; while it is
 *                    1, "integrator" cannot leave 2, and it cannot return to 0 while an encounter radius is set).  Switching
 *                    it drops the remembered evaluation and is refused (MURBHIP_E_STATE) while a block is open (C5).  The active sweep then runs on 4 workgroups per CU instead of 5
 *   "contact"        0 (default), 1, 2: the Hermite sweeps also keep every body's contact partner by radii and its gap2; 2 adds
 *                    the contact stop (see murbhip_upload_radii above).  One shard with "integrator" 2 only; excludes "nearest".
 *                    The active sweep then runs on 4 workgroups per CU instead of 5
 *   "potential"      0 (default), 1: the Hermite sweeps also keep every body's potential phi_i (see murbhip_download_potential
 *                    above).  One shard with "integrator" 2 only; excludes "nearest" and "contact".  Switching it drops the
 *                    remembered evaluation.  The active sweep then runs on 4 workgroups per CU instead of 5
 *   "tri_first_pct"  "overlap" 1, pair-symmetric schedule: percentage (0..100, default 50) of the own-slice
 *                    triangle that is launched before the rectangles, i.e. under the all-gather of positions;
 *                    the rest runs under the reduce-scatter of accelerations.  A tuning knob for real
 *                    interconnect latencies (bench.py picks it per run, untimed)
 *                    A plan key: a value-changing set drops the remembered forces and pair potential (C4)
 *   "exchange_p2p"   RCCL exchange only (MURBHIP_E_STATE otherwise): 1 = both exchanges of a step as grouped ncclSend / ncclRecv
 *                    instead of collectives.  Accelerations: under the half-ring schedule a rank only has contributions for
 *                    the floor(W/2) slices ahead of it, so it sends those chunks straight to their owners and adds up the
 *                    floor(W/2) it receives (ncclReduceScatter moves and adds zeros for the other half); positions: every
 *                    slice straight to every peer.  One hop per message on a fully connected xGMI node.  0 (default) =
 *                    ncclReduceScatter + ncclAllGather.  UNMEASURED on hardware: bench.py times it beside the default for
 *                    N > 1 ("p2p_plan") so that the first multi-GPU run shows which to prefer
 *   "cu_reserve"     k >= 0 (default 0): the compute streams are re-created with a CU mask that leaves the k highest
 *                    CUs (8 = one per XCD, 16 = two per XCD) to the exchange stream.  The force kernels otherwise fill
 *                    every CU, and a collective's kernel (RCCL) has to wait ~0.1 ms for one of their workgroups to retire
 *                    (7 us with k = 8); but dispatch on a masked queue is slower: 6-8 % on long force launches, much more
 *                    on short ones.  bench.py times it per run for N > 1, like "tri_first_pct".
 *                    Two side effects of hipExtStreamCreateWithCUMask, which has no flags argument: (i) a masked stream
 *                    is BLOCKING with respect to the device's null stream, so a host application that works on stream 0
 *                    of the same device (torch's default stream) synchronises with the force kernels implicitly;
 *                    (ii) it has default priority.  The low-priority stream of "overlap" 2 therefore stays unmasked
 *                    (it keeps its priority and may use the reserved CUs)
 *   "fuse_integrate" 1 (default): one GPU, one-sided kernel with all j in one chunk (the default up to 6 blocks): the state
 *                    update runs in the tail of the force launch — one launch per step instead of two, bit-identical results
 *                    (N = 2 048: 7.2 instead of 13.4 us per step).  0 = two launches, and the round-2 rule for "variant" 0
 *                    (pair-symmetric from 3 blocks up)
 *                    A plan key: a value-changing set drops the remembered forces and pair potential (C4)
 *   "solo_shard"     r >= 0: in a sharded context only shard r launches force work (timing aid: the
 *                    isolated per-step timeline of one rank of W; results are meaningless).  -1 = off
 *   "force_exchange" 1: run the position exchange even with a single rank/shard (self-test of the
 *                    RCCL binding on a one-GPU machine; rank mode needs a unique id at creation)
 */
int murbhip_set_option(murbhip_ctx* ctx, const char* key, long value);

/* Numeric facts.  Keys: "cu_count", "clock_mhz", "n", "slots", "world", "rank", "jsplit", "variant", "cu_reserve", "sym_passes", "sym_waves", "sym_wide" (the form of the pair factor in use: 0 or 1; 0 on a one-sided plan), "taper",
 * "block_units", "block_grid" (work units and workgroups of murbhip_evolve_block's active sweep), "block_steps", "block_body_steps",
 * "block_clamped", "block_max_active" (the last murbhip_evolve_block call's counts), "nearest" (the option), "encounter_count" (hits of
 * the step that ended the last evolve call: murbhip_encounters' *count), "contact" (the option), "contact_count" (murbhip_contacts' *count), "potential" (the option),
 * "workgroups", "interactions_per_launch", "device_bytes", "hermite_parts" (j chunks of the acceleration + jerk sweep of
 * "integrator" 2: "jsplit" clamped to the layout tiles and 32, or the automatic rule), and the timing spans of the steps since "profile" was set (HIP
 * events on the library's own streams, all shards of this process; the call drains the device):
 *   "force_launches", "force_ms_avg", "force_ms_total"      every force launch
 *   "span_<kind>_ms_avg", "span_<kind>_count"               kind = tri1 | rect | tri2 (the three force launches of the exchange
 *       pipeline), reduce_scatter | all_gather (exchange stream: from "my input is ready" to "my output has arrived"),
 *       wait_gather | wait_reduce (compute stream idle, waiting for that collective), step (compute stream, first launch of
 *       a step to the end of its state update), field | tidal (compute stream: a sweep launch of the field read-out, murbfield.h,
 *       or of the tidal read-out, murbtidal.h; no part of the force_* figures); the last seven need "profile" 2
 *   "compute_wait_ms_per_step"                              (wait_gather + wait_reduce) per profiled step
 *   "spans_dropped"                                         1 when the event pool (4096 spans per shard) ran out
 *   "sym_launches"                                          pair-symmetric launches of any form (force, force + pair potential,
 *                                                           potential sweep) since "profile" was last set */
int murbhip_get_info(murbhip_ctx* ctx, const char* key, double* value);

#ifdef __cplusplus
}
#endif
#endif /* MURBHIP_H_ */
