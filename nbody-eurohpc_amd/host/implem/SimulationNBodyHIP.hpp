// `--im hip+tile` / `--im hip+tile+multi`: the MI355X implementation behind the reference's plugin
// interface.  It takes the place of SimulationNBodyCUDATileFullDevice
// (reference src/murb/implem/SimulationNBodyCUDATileFullDevice.hpp:11-35): device-resident bodies,
// one force launch + one integrate launch per iteration, nothing copied back unless asked.
#ifndef SIMULATION_N_BODY_HIP_HPP_
#define SIMULATION_N_BODY_HIP_HPP_

#include <memory>
#include <vector>

#include "core/HIPBodies.hpp"
#include "core/SimulationNBodyInterface.hpp"

template <typename T> class SimulationNBodyHIP : public SimulationNBodyInterface<T> {
  protected:
    std::shared_ptr<HIPBodies<T>> hipBodiesPtr;
    accSoA_t<T> accSoA;

  public:
    // `devices`: HIP ordinals to spread the bodies over ({0} = one GPU).  Needs a HIPBodiesAllocator.
    // Construction ends with an untimed device warm-up (warmUp below; MURBHIP_WARMUP_MS in the environment, default 50, 0 = none).
    SimulationNBodyHIP(const BodiesAllocatorInterface<T> &allocator, const T soft = 0.035f,
                       const std::vector<int> &devices = {0}, int exchange = 1);
    virtual ~SimulationNBodyHIP() = default;

    void computeOneIteration() override;   // enqueue only; the driver syncs (main.cpp:356-368)
    void synchronize();                    // that sync, for callers without HIP headers
    void warmUp(double milliseconds);      // force evaluations on the current state for about that long (state unchanged)
    const accSoA_t<T> &getAccSoA();        // accelerations of the last iteration (test hook)

    // What the bodies, as they are on the device, make at `count` points of the caller's: acceleration, jerk and potential
    // (murbfield_at's arguments and rules: velocities all three null = points at rest; skip null, or per point a body left
    // out, -1 = none; every output group may be null).  A read-out: synchronous, nothing of the simulation changes.  Returns
    // murbhip's code (0 = done) instead of ending the program: a refused call is the caller's to handle.
    int fieldAt(unsigned long count, const T *px, const T *py, const T *pz, const T *pvx, const T *pvy, const T *pvz, const int *skip,
                T *ax, T *ay, T *az, T *jx, T *jy, T *jz, T *phi);

    // The tidal tensor d a_a / d p_b of the bodies, as they are on the device, at `count` points of the caller's (murbtidal_at's
    // arguments and rules: skip null, or per point a body left out, -1 = none; the six outputs all set or all null).  A read-out
    // like fieldAt; returns murbhip's code.
    int tidalAt(unsigned long count, const T *px, const T *py, const T *pz, const int *skip, T *txx, T *tyy, T *tzz, T *txy, T *txz,
                T *tyz);

    // Density centre, core radius and core density of the bodies as they are on the device, from every body's local density
    // over its k nearest (murbdensity_centre's arguments and rules: out8 = {X_x, X_y, X_z, r_c, rho_c, sum rho, used, left out}).
    // A read-out like fieldAt; returns murbhip's code.
    int densityCentre(int k, double *out8);

    // Neighbours within h of every body as the bodies are on the device, in CSR form (murbnbr_of's rules, include/murbnbr.h):
    // offsets gets n + 1 entries, idx offsets[n]: body p's neighbours are idx[offsets[p] .. offsets[p + 1]) in ascending
    // index.  The count-only call, then the sized one.  A read-out like fieldAt; returns murbhip's code.
    int neighboursOf(float h, std::vector<unsigned long> &offsets, std::vector<int> &idx);

    // Bound pairs of the bodies as they are on the device (murbbind_pairs' rules, include/murbbind.h): the mutual pairs whose
    // sweep value h < 0, i < j ascending in i, with six doubles a pair in elems {a, e, P, h64, E_b, r}, and the census out8.
    // The count-only call, then the sized one.  A read-out like fieldAt; returns murbhip's code.
    int binaries(std::vector<int> &i, std::vector<int> &j, std::vector<double> &elems, double *out8);

    // Bound members of the bodies as they are on the device (murbbound_members' rules, include/murbbound.h): iterative unbinding
    // from all bodies in the members' own frame, at most maxIter rounds.  member gets n bytes (0 / 1), e the n energies per unit
    // mass against the final members, out16 the summary.  A read-out like fieldAt; returns murbhip's code.
    int boundMembers(int maxIter, std::vector<unsigned char> &member, std::vector<double> &e, double *out16);

    // Minimum spanning tree of all bodies as they are on the device (murbmst_of's rules, include/murbmst.h): the edges i < j
    // ascending by the key (r2, i, j) with the sweep's r2 and the fp64 length of each, out8 the summary {members, edges,
    // components, rounds, total, mean and longest length, 0}.  A read-out like fieldAt; returns murbhip's code.
    int spanningTree(std::vector<int> &i, std::vector<int> &j, std::vector<float> &r2, std::vector<double> &length, double *out8);

    // Mean pair separation of all bodies as they are on the device (murbsep_of's sums, include/murbsep.h): every body's sum of
    // distances to the others, added in index order in fp64, over n (n - 1); NaN for fewer than 2 bodies.  A read-out like
    // fieldAt; returns murbhip's code.
    int meanSeparation(double *mean);

    // The neighbour split of every body's force as the bodies are on the device (murbsplit_of's rules, include/murblist.h): counts
    // gets the n neighbour counts within h; irregular, total and regular 7 n floats each, the planes ax ay az jx jy jz phi one
    // after the other: the force of the neighbours alone, murbfield_of's of all other bodies, and total - irregular formed in
    // double and rounded once.  A read-out like fieldAt; returns murbhip's code.
    int forceSplit(float h, std::vector<unsigned long> &counts, std::vector<float> &irregular, std::vector<float> &total,
                   std::vector<float> &regular);

    // The Ahmad-Cohen neighbour scheme on the bodies as they are on the device (murbac_begin's and murbac_steps' arguments and rules,
    // include/murbac.h; needs the Hermite plugins): acBegin starts it with the common neighbour radius h and a full sweep on every
    // nIrr-th step, acSteps takes `steps` steps of dt (enqueue only, like computeOneIteration).  Both return murbhip's code.
    int acBegin(float h, int nIrr);
    int acSteps(float dt, int steps);

    // Massless tracers carried by the Hermite steps on the device (murbtracer_upload's arguments and rules: velocities all three
    // null = at rest, count 0 clears; needs the Hermite plugins, `hip+hermite` or `hip+hermite+adaptive`).  getTracers: the
    // resident tracers' state into arrays of as many entries as getTracerCount gives (null pointers are skipped).  All three return
    // murbhip's code.
    int setTracers(unsigned long count, const T *qx, const T *qy, const T *qz, const T *vx, const T *vy, const T *vz);
    int getTracers(T *qx, T *qy, T *qz, T *vx, T *vy, T *vz);
    int getTracerCount(unsigned long *count);
};

#endif
