// `--im hip+tracking`, `--im hip+leapfrog`, `--im hip+hermite`, `--im hip+hermite+adaptive` and `--im hip+hermite+block`: the MI355X path with a
// per-iteration metrics history —
// the counterparts of the reference's gpu+tracking (SimulationNBodyCUDAPropertyTracking.hpp, energy of
// the state each iteration starts from, computeOneIteration() at .cu:121-133) and gpu+leapfrog
// (SimulationNBodyCUDALeapfrog.hpp: same history, leapfrog integrator); hip+hermite has no counterpart there, nor has
// hip+hermite+adaptive, whose iteration advances the driver's dt in as many Hermite substeps as murbhip_evolve's criterion
// asks for (the history still has one row per iteration), nor hip+hermite+block, whose iteration is one block of
// murbhip_evolve_block: every body takes steps of its own size dt 2^-k, and every iteration returns synchronised.
//
// Filled per iteration: energy (kinetic + potential, reference definitions), |angular momentum| and the
// centre of mass — the reference reserves the last two columns but never computes them
// (SimulationNBodyCUDAPropertyTracking.cu:5-8).  `--im hip+tracking+density` is hip+tracking with the density centre
// over every body's 6 nearest neighbours (include/murbknn.h) in the centre's columns.
#ifndef SIMULATION_N_BODY_HIP_TRACKING_HPP_
#define SIMULATION_N_BODY_HIP_TRACKING_HPP_

#include <memory>
#include <vector>

#include "core/SimulationHistory.hpp"
#include "implem/SimulationNBodyHIP.hpp"

template <typename T, typename Q = double> class SimulationNBodyHIPTracking : public SimulationNBodyHIP<T> {
  public:
    struct Encounter {
        int i, j;      // body and its nearest neighbour
        float r2;      // the sweep's |q_j - q_i|^2 + soft^2 of the pair
    };

  protected:
    std::shared_ptr<SimulationHistory<Q>> history;
    int currentIteration = 0;
    bool adaptive = false;            // integrator 3: "integrator" 2 driven by murbhip_evolve; 4: by murbhip_evolve_block
    bool blockSteps = false;          // integrator 4
    bool hermite = false;             // integrators 2 to 5: the acceleration + jerk sweeps
    bool neighbourScheme = false;     // integrator 5: "integrator" 2 driven by murbac_steps (include/murbac.h)
    bool acBegun = false;             // ... whose scheme the first iteration begins
    T acRadius = 0;                   // ... with this common neighbour radius
    int acNirr = 8;                   // ... and a full sweep on every acNirr-th iteration
    bool potentialOn = false;         // ... keep every body's potential beside them (option "potential")
    int kmax = 12;                    // its deepest level (--kmax): steps down to dt 2^-kmax
    unsigned long bodySteps = 0, clampedSteps = 0;   // integrator 4: bodies advanced, and steps the cap was too coarse for
    double eta = 0.02;                // its accuracy parameter (--eta); the first step of all uses eta_start = 0.01
    unsigned long substeps = 0;       // substeps of all iterations so far
    double dtSmallest = 0, dtLargest = 0;   // ... and the range of their sizes
    T encounterRadius = 0;            // integrators 3 and 4: an iteration ends behind the substep in which two bodies come this close
    std::vector<Encounter> encounters;   // the pairs (i, nearest of i) of that substep, sorted by i (the device keeps 4096)
    unsigned long encounterCount = 0;    // ... how many there were; 0: the last iteration ran its whole dt
    double encounterTime = 0;            // ... and the model time that iteration had advanced
    bool contactStop = false;            // integrators 3 and 4: an iteration ends behind the substep in which two bodies touch
    T contactScale = 1;                  // ... their radii being the bodies' own times this
    std::vector<Encounter> contacts;     // (i, contact partner of i, gap2) of that substep, sorted by i (the device keeps 4096)
    unsigned long contactCount = 0;
    double contactTime = 0;
    bool densityCentreOn = false;        // the density_center columns hold the density centre, not the centre of mass

  public:
    // integrator: murbhip option "integrator" — 0 (false) the reference's update, 1 (true) kick-drift-kick leapfrog,
    // 2 4th-order Hermite, 3 option 2 with shared adaptive steps (murbhip_evolve), 4 option 2 with individual block steps
    // (murbhip_evolve_block; `substeps` then counts block steps).  The parameter used to be
    // `bool leapfrog`: callers that pass a bool get 0 / 1 as before.
    SimulationNBodyHIPTracking(const BodiesAllocatorInterface<T> &allocator, std::shared_ptr<SimulationHistory<Q>> history,
                               const T soft = 0.035f, const int integrator = 0, const std::vector<int> &devices = {0},
                               int exchange = 1);
    virtual ~SimulationNBodyHIPTracking() = default;

    void computeOneIteration() override;   // metrics of the current state -> history, then one step
    void computeMetrics();                 // fills row `currentIteration` (grows the history if needed)
    void readEncounters();                 // after an evolve call: count, time and pairs of the substep that ended it
    const std::shared_ptr<SimulationHistory<Q>> getHistory() const { return history; }
    void setEta(const double e) { eta = e; }
    void setKmax(const int k) { kmax = k; }
    bool isAdaptive() const { return adaptive; }
    bool hasBlockSteps() const { return blockSteps; }
    unsigned long getBodySteps() const { return bodySteps; }
    unsigned long getClampedSteps() const { return clampedSteps; }
    unsigned long getSubsteps() const { return substeps; }
    double getSmallestDt() const { return dtSmallest; }
    double getLargestDt() const { return dtLargest; }
    // hip+hermite+adaptive / hip+hermite+block (murbhip_set_encounter; switches the "nearest" option on): an iteration in which a
    // body that took a substep has its nearest neighbour within `radius` ends behind that substep, short of dt (under block
    // steps possibly inside a block: the caller then goes on with murbhip_evolve_block or uploads).  0 = off.  false for the
    // fixed-step integrators.
    bool setEncounterRadius(const T radius);
    unsigned long getEncounterCount() const { return encounterCount; }
    double getEncounterTime() const { return encounterTime; }
    const std::vector<Encounter> &getEncounters() const { return encounters; }
    // hip+hermite+adaptive / hip+hermite+block (murbhip_upload_radii, option "contact" 2): uploads the bodies' own radii
    // (dataSoA.r) times `scale` and ends an iteration behind the substep in which a body that took it touches another:
    // |q_j - q_i|^2 <= (r_i + r_j)^2, formed as include/murbhip.h defines gap2.  Excludes an encounter radius.  false for the
    // fixed-step integrators, for a scale that is not finite and positive, and beside an encounter radius.  In getContacts()
    // the member r2 of an entry holds gap2.
    bool setContactStop(const bool on, const T scale = 1);
    bool hasContactStop() const { return contactStop; }
    T getContactScale() const { return contactScale; }
    void readContacts();
    unsigned long getContactCount() const { return contactCount; }
    double getContactTime() const { return contactTime; }
    const std::vector<Encounter> &getContacts() const { return contacts; }
    // hip+hermite / hip+hermite+adaptive / hip+hermite+block (option "potential"): the sweeps keep every body's potential phi_i
    // (include/murbhip.h has the definition).  Excludes an encounter radius and the contact stop.  false for the other
    // integrators and beside either of the two.
    bool setPotential(const bool on);
    // hip+hermite+ac (integrator 5): the common neighbour radius and the regular steps' spacing, before the first iteration.
    // false for the other integrators, after the first iteration, for a radius negative or not finite, for nIrr outside [1, 4096].
    bool setNeighbourScheme(const T radius, const int nIrr);
    bool hasNeighbourScheme() const { return neighbourScheme; }
    bool hasPotential() const { return potentialOn; }
    // hip+tracking+density: the history's density_center columns hold the density centre over every body's 6 nearest
    // (densityCentre(6)) instead of the centre of mass.  Every integrator.
    void setDensityCentre(const bool on) { densityCentreOn = on; }
    bool hasDensityCentre() const { return densityCentreOn; }
    // phi_i of the last sweep in the bodies' order (murbhip_download_potential; after an iteration: of its last substep's
    // predicted end state); empty where the option is off or no sweep has run yet
    std::vector<float> getPotential() const;
};

#endif
