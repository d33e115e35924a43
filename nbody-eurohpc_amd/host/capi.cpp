// C ABI over the C++ host mirror, for the Python tests and bench.py (ctypes):
//   * the product's own initial conditions (so bench.py never needs the oracle for its inputs),
//   * the mirrored plugin classes driven exactly like the reference's tests drive the originals
//     (src/test/implem/test_SimulationNBody.cpp:28-71, test_CUDABodies.cpp:23-75).
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>

#include "core/Bodies.hpp"
#include "core/BodiesAllocator.hpp"
#include "core/SimulationHistory.hpp"
#include "implem/SimulationNBodyHIP.hpp"
#include "implem/SimulationNBodyHIPTracking.hpp"

namespace {
struct Sim {
    std::string scheme;
    SimulationNBodyHIP<float> *sim = nullptr;
    std::shared_ptr<SimulationHistory<double>> history;   // tracking sims only
};
void copyState(const dataSoA_t<float> &d, float *qx, float *qy, float *qz, float *vx, float *vy, float *vz, float *m,
               float *r)
{
    const size_t bytes = d.qx.size() * sizeof(float);
    const struct { float *dst; const std::vector<float> *src; } f[] = {
        {qx, &d.qx}, {qy, &d.qy}, {qz, &d.qz}, {vx, &d.vx}, {vy, &d.vy}, {vz, &d.vz}, {m, &d.m}, {r, &d.r}};
    for (const auto &e : f)
        if (e.dst) std::memcpy(e.dst, e.src->data(), bytes);
}
}  // namespace

extern "C" {

unsigned long murbhost_padding(unsigned long n, const char *scheme)
{
    return Bodies<float>(n, std::string(scheme)).getPadding();
}

// n + padding entries per array (NULL pointers are skipped)
void murbhost_init_bodies(unsigned long n, const char *scheme, unsigned long seed, float *qx, float *qy, float *qz,
                          float *vx, float *vy, float *vz, float *m, float *r)
{
    const Bodies<float> b(n, std::string(scheme), seed);
    copyState(b.getDataSoA(), qx, qy, qz, vx, vy, vz, m, r);
}

// host integrator alone (Bodies::updatePositionsAndVelocities), n entries out
void murbhost_integrate(unsigned long n, const char *scheme, const float *ax, const float *ay, const float *az, float dt,
                        int steps, int on_device, float *qx, float *qy, float *qz, float *vx, float *vy, float *vz)
{
    accSoA_t<float> acc;
    acc.ax.assign(ax, ax + n); acc.ay.assign(ay, ay + n); acc.az.assign(az, az + n);
    std::unique_ptr<Bodies<float>> b;
    if (on_device) {
        auto *hb = new HIPBodies<float>(n, std::string(scheme));
        hb->bindDevice(2e8f, 6.67384e-11f);
        b.reset(hb);
    } else b.reset(new Bodies<float>(n, std::string(scheme)));
    for (int s = 0; s < steps; ++s) b->updatePositionsAndVelocities(acc, dt);
    const auto &d = b->getDataSoA();
    const size_t bytes = n * sizeof(float);
    std::memcpy(qx, d.qx.data(), bytes); std::memcpy(qy, d.qy.data(), bytes); std::memcpy(qz, d.qz.data(), bytes);
    std::memcpy(vx, d.vx.data(), bytes); std::memcpy(vy, d.vy.data(), bytes); std::memcpy(vz, d.vz.data(), bytes);
}

void *murbhost_sim_create(unsigned long n, const char *scheme, float soft, float dt, int ndev, const int *devices,
                          int exchange)
{
    auto *h = new Sim;
    h->scheme = scheme;
    HIPBodiesAllocator<float> alloc(n, h->scheme);
    h->sim = new SimulationNBodyHIP<float>(alloc, soft, std::vector<int>(devices, devices + ndev), exchange);
    h->sim->setDt(dt);
    return h;
}
// --im hip+tracking (leapfrog = 0) / hip+leapfrog (1) / hip+hermite (2): the value is murbhip's option "integrator";
// hip+hermite+adaptive (3): option 2 driven by murbhip_evolve; hip+hermite+block (4): by murbhip_evolve_block; hip+hermite+ac (5): by
// murbac_steps
void *murbhost_tracking_create(unsigned long n, const char *scheme, float soft, float dt, int leapfrog, int ndev,
                               const int *devices, int exchange)
{
    auto *h = new Sim;
    h->scheme = scheme;
    h->history = std::make_shared<SimulationHistory<double>>();
    HIPBodiesAllocator<float> alloc(n, h->scheme);
    h->sim = new SimulationNBodyHIPTracking<float, double>(alloc, h->history, soft, leapfrog,
                                                           std::vector<int>(devices, devices + ndev), exchange);
    h->sim->setDt(dt);
    return h;
}
int murbhost_history_rows(void *p)
{
    auto *h = static_cast<Sim *>(p);
    return h->history ? h->history->getNumIterations() : -1;
}
// rows entries each; centers as x0,y0,z0,x1,...
void murbhost_history_get(void *p, double *energy, double *ang_momentum, double *centers)
{
    const auto &hist = *static_cast<Sim *>(p)->history;
    for (int i = 0; i < hist.getNumIterations(); ++i) {
        energy[i] = hist.getEnergyAt(i);
        ang_momentum[i] = hist.getAngMomentumAt(i);
        for (int k = 0; k < 3; ++k) centers[3 * i + k] = hist.getDensityCenterAt(i)[k];
    }
}
// SimulationHistory alone (no device): fill `rows` rows and write the CSV.  0, or -1 if the file cannot be opened.
int murbhost_history_csv(const char *path, int rows, const double *energy, const double *ang_momentum, const double *centers)
{
    SimulationHistory<double> hist(rows);
    for (int i = 0; i < rows; ++i) {
        hist.setEnergyAt(i, energy[i]);
        hist.setAngMomentumAt(i, ang_momentum[i]);
        hist.setDensityCenterAt(i, {centers[3 * i], centers[3 * i + 1], centers[3 * i + 2]});
    }
    try {
        hist.saveMetricsToCSV(path);
    } catch (const std::runtime_error &) {
        return -1;
    }
    return 0;
}
// hip+hermite+adaptive: {substeps so far, smallest dt, largest dt}; hip+hermite+block: block steps so far and the range of
// the bodies' own dt.  0, or -1 for a simulation with fixed steps.
int murbhost_sim_substeps(void *p, double *out3)
{
    auto *t = dynamic_cast<SimulationNBodyHIPTracking<float, double> *>(static_cast<Sim *>(p)->sim);
    if (!t || !t->isAdaptive()) return -1;
    out3[0] = (double)t->getSubsteps();
    out3[1] = t->getSmallestDt();
    out3[2] = t->getLargestDt();
    return 0;
}
// hip+hermite+ac (5): SimulationNBodyHIPTracking::setNeighbourScheme.  0, or -1 where it does not apply.
int murbhost_sim_set_ac(void *p, float rnb, int nirr)
{
    auto *t = dynamic_cast<SimulationNBodyHIPTracking<float, double> *>(static_cast<Sim *>(p)->sim);
    return t && t->setNeighbourScheme(rnb, nirr) ? 0 : -1;
}
// SimulationNBodyHIP::acBegin / acSteps on any simulation: murbhip's code
int murbhost_sim_ac_begin(void *p, float h, int nirr) { return static_cast<Sim *>(p)->sim->acBegin(h, nirr); }
int murbhost_sim_ac_steps(void *p, float dt, int steps) { return static_cast<Sim *>(p)->sim->acSteps(dt, steps); }
// hip+hermite+block: accuracy parameter and deepest level, before the first iteration.  0, or -1 for another simulation.
int murbhost_sim_set_block(void *p, double eta, int kmax)
{
    auto *t = dynamic_cast<SimulationNBodyHIPTracking<float, double> *>(static_cast<Sim *>(p)->sim);
    if (!t || !t->hasBlockSteps()) return -1;
    t->setEta(eta);
    t->setKmax(kmax);
    return 0;
}
// hip+hermite+block: {block steps so far (murbhost_sim_substeps' count), body-steps, clamped steps}.  0, or -1.
int murbhost_sim_block_counts(void *p, double *out3)
{
    auto *t = dynamic_cast<SimulationNBodyHIPTracking<float, double> *>(static_cast<Sim *>(p)->sim);
    if (!t || !t->hasBlockSteps()) return -1;
    out3[0] = (double)t->getSubsteps();
    out3[1] = (double)t->getBodySteps();
    out3[2] = (double)t->getClampedSteps();
    return 0;
}
// hip+hermite+adaptive / hip+hermite+block: SimulationNBodyHIPTracking::setEncounterRadius.  0, or -1 for another simulation.
int murbhost_sim_set_encounter(void *p, float radius)
{
    auto *t = dynamic_cast<SimulationNBodyHIPTracking<float, double> *>(static_cast<Sim *>(p)->sim);
    return t && t->setEncounterRadius(radius) ? 0 : -1;
}
// ... the pairs of the substep that ended the last iteration (murbhip_encounters' arguments; NULL arrays ask for *count and
// *time alone).  0, -1 for another simulation, -2 when capacity is smaller than the number of pairs kept.
int murbhost_sim_encounters(void *p, int *i, int *j, float *r2, unsigned long capacity, unsigned long *count, double *time)
{
    auto *t = dynamic_cast<SimulationNBodyHIPTracking<float, double> *>(static_cast<Sim *>(p)->sim);
    if (!t || !t->isAdaptive()) return -1;
    *count = t->getEncounterCount();
    if (time) *time = t->getEncounterTime();
    const auto &e = t->getEncounters();
    if ((!i && !j && !r2) || e.empty()) return 0;
    if (capacity < e.size()) return -2;
    for (size_t k = 0; k < e.size(); ++k) {
        if (i) i[k] = e[k].i;
        if (j) j[k] = e[k].j;
        if (r2) r2[k] = e[k].r2;
    }
    return 0;
}
// hip+hermite / hip+hermite+adaptive / hip+hermite+block: SimulationNBodyHIPTracking::setPotential.  0, or -1 where it does not
// apply (another simulation, an encounter radius or the contact stop set).
int murbhost_sim_set_potential(void *p, int on)
{
    auto *t = dynamic_cast<SimulationNBodyHIPTracking<float, double> *>(static_cast<Sim *>(p)->sim);
    return t && t->setPotential(on != 0) ? 0 : -1;
}
// ... every body's potential of the last sweep, n entries.  0, -1 for a simulation without the option, -2 before the first sweep.
int murbhost_sim_potential(void *p, float *phi)
{
    auto *t = dynamic_cast<SimulationNBodyHIPTracking<float, double> *>(static_cast<Sim *>(p)->sim);
    if (!t || !t->hasPotential() || !phi) return -1;
    const std::vector<float> v = t->getPotential();
    if (v.empty()) return -2;
    std::copy(v.begin(), v.end(), phi);
    return 0;
}
// hip+hermite+adaptive / hip+hermite+block: SimulationNBodyHIPTracking::setContactStop.  0, or -1 where it does not apply
// (another simulation, an encounter radius set, a scale that is not finite and positive).
int murbhost_sim_set_contact(void *p, int on, float rscale)
{
    auto *t = dynamic_cast<SimulationNBodyHIPTracking<float, double> *>(static_cast<Sim *>(p)->sim);
    return t && t->setContactStop(on != 0, rscale) ? 0 : -1;
}
// ... the triples (i, contact partner, gap2) of the substep that ended the last iteration (murbhip_contacts' arguments).
// 0, -1 for a simulation without a contact stop, -2 when capacity is smaller than the number kept.
int murbhost_sim_contacts(void *p, int *i, int *j, float *gap2, unsigned long capacity, unsigned long *count, double *time)
{
    auto *t = dynamic_cast<SimulationNBodyHIPTracking<float, double> *>(static_cast<Sim *>(p)->sim);
    if (!t || !t->isAdaptive() || !t->hasContactStop()) return -1;
    *count = t->getContactCount();
    if (time) *time = t->getContactTime();
    const auto &e = t->getContacts();
    if ((!i && !j && !gap2) || e.empty()) return 0;
    if (capacity < e.size()) return -2;
    for (size_t k = 0; k < e.size(); ++k) {
        if (i) i[k] = e[k].i;
        if (j) j[k] = e[k].j;
        if (gap2) gap2[k] = e[k].r2;
    }
    return 0;
}
// SimulationNBodyHIP::fieldAt (murbfield_at's arguments); murbhip's code
int murbhost_sim_field_at(void *p, unsigned long count, const float *px, const float *py, const float *pz, const float *pvx,
                          const float *pvy, const float *pvz, const int *skip, float *ax, float *ay, float *az, float *jx, float *jy,
                          float *jz, float *phi)
{
    return static_cast<Sim *>(p)->sim->fieldAt(count, px, py, pz, pvx, pvy, pvz, skip, ax, ay, az, jx, jy, jz, phi);
}
// SimulationNBodyHIP::tidalAt (murbtidal_at's arguments); murbhip's code
int murbhost_sim_tidal_at(void *p, unsigned long count, const float *px, const float *py, const float *pz, const int *skip,
                          float *txx, float *tyy, float *tzz, float *txy, float *txz, float *tyz)
{
    return static_cast<Sim *>(p)->sim->tidalAt(count, px, py, pz, skip, txx, tyy, tzz, txy, txz, tyz);
}
// SimulationNBodyHIP::densityCentre (murbdensity_centre's arguments); murbhip's code
int murbhost_sim_density_centre(void *p, int k, double *out8)
{
    return static_cast<Sim *>(p)->sim->densityCentre(k, out8);
}
// SimulationNBodyHIP::neighboursOf: offsets (n + 1 entries) always; idx where it is given and holds the total (capacity entries),
// else MURBHIP_E_INVALID (-2000) with the offsets complete, like murbnbr_of; murbhip's code
int murbhost_sim_neighbours_of(void *p, float h, unsigned long *offsets, int *idx, unsigned long capacity)
{
    std::vector<unsigned long> o;
    std::vector<int> i;
    const int rc = static_cast<Sim *>(p)->sim->neighboursOf(h, o, i);
    if (rc != 0) return rc;
    std::copy(o.begin(), o.end(), offsets);
    if (!idx) return 0;
    if (i.size() > capacity) return -2000;   // MURBHIP_E_INVALID
    std::copy(i.begin(), i.end(), idx);
    return 0;
}
// SimulationNBodyHIP::boundMembers: member (n bytes) and e (n doubles) where they are given, out16 always; murbhip's code
int murbhost_sim_bound_members(void *p, int max_iter, unsigned char *member, double *e, double *out16)
{
    std::vector<unsigned char> vm;
    std::vector<double> ve;
    const int rc = static_cast<Sim *>(p)->sim->boundMembers(max_iter, vm, ve, out16);
    if (rc != 0) return rc;
    if (member) std::copy(vm.begin(), vm.end(), member);
    if (e) std::copy(ve.begin(), ve.end(), e);
    return 0;
}
// SimulationNBodyHIP::spanningTree: out8 always; i, j, r2, length (capacity entries each) where they are given and hold the edges, else
// MURBHIP_E_INVALID (-2000) with out8 filled, like murbmst_of; murbhip's code
int murbhost_sim_spanning_tree(void *p, int *i, int *j, float *r2, double *length, unsigned long capacity, double *out8)
{
    std::vector<int> vi, vj;
    std::vector<float> vr;
    std::vector<double> vl;
    const int rc = static_cast<Sim *>(p)->sim->spanningTree(vi, vj, vr, vl, out8);
    if (rc != 0) return rc;
    if ((i || j || r2 || length) && capacity < vi.size()) return -2000;
    if (i) std::copy(vi.begin(), vi.end(), i);
    if (j) std::copy(vj.begin(), vj.end(), j);
    if (r2) std::copy(vr.begin(), vr.end(), r2);
    if (length) std::copy(vl.begin(), vl.end(), length);
    return 0;
}
// SimulationNBodyHIP::meanSeparation; murbhip's code
int murbhost_sim_mean_separation(void *p, double *mean) { return static_cast<Sim *>(p)->sim->meanSeparation(mean); }
// SimulationNBodyHIP::forceSplit: counts (n entries) and irregular, total, regular (7 n floats each: the planes ax ay az jx jy jz phi)
// where they are given; murbhip's code
int murbhost_sim_force_split(void *p, float h, unsigned long *counts, float *irregular, float *total, float *regular)
{
    std::vector<unsigned long> vc;
    std::vector<float> vi, vt, vr;
    const int rc = static_cast<Sim *>(p)->sim->forceSplit(h, vc, vi, vt, vr);
    if (rc != 0) return rc;
    if (counts) std::copy(vc.begin(), vc.end(), counts);
    if (irregular) std::copy(vi.begin(), vi.end(), irregular);
    if (total) std::copy(vt.begin(), vt.end(), total);
    if (regular) std::copy(vr.begin(), vr.end(), regular);
    return 0;
}
// SimulationNBodyHIP::binaries: *count and out8 always; i, j (capacity entries) and elems (6 * capacity) where they are given and
// hold the pairs, else MURBHIP_E_INVALID (-2000) with *count and out8 filled, like murbbind_pairs; murbhip's code
int murbhost_sim_binaries(void *p, int *i, int *j, double *elems, unsigned long capacity, unsigned long *count, double *out8)
{
    std::vector<int> vi, vj;
    std::vector<double> ve;
    const int rc = static_cast<Sim *>(p)->sim->binaries(vi, vj, ve, out8);
    if (rc != 0) return rc;
    *count = vi.size();
    if (!i) return 0;
    if (capacity < vi.size()) return -2000;
    std::copy(vi.begin(), vi.end(), i);
    std::copy(vj.begin(), vj.end(), j);
    std::copy(ve.begin(), ve.end(), elems);
    return 0;
}
// --im hip+tracking+density: SimulationNBodyHIPTracking::setDensityCentre.  0, or -1 for a simulation without a history.
int murbhost_sim_set_density_centre(void *p, int on)
{
    auto *t = dynamic_cast<SimulationNBodyHIPTracking<float, double> *>(static_cast<Sim *>(p)->sim);
    if (!t) return -1;
    t->setDensityCentre(on != 0);
    return 0;
}
// SimulationNBodyHIP::setTracers / getTracers (murbtracer_upload's and murbtracer_download's arguments); murbhip's code
int murbhost_sim_set_tracers(void *p, unsigned long count, const float *qx, const float *qy, const float *qz, const float *vx,
                             const float *vy, const float *vz)
{
    return static_cast<Sim *>(p)->sim->setTracers(count, qx, qy, qz, vx, vy, vz);
}
int murbhost_sim_get_tracers(void *p, unsigned long *count, float *qx, float *qy, float *qz, float *vx, float *vy, float *vz)
{
    if (count)
        if (const int rc = static_cast<Sim *>(p)->sim->getTracerCount(count)) return rc;
    if (!qx && !qy && !qz && !vx && !vy && !vz) return 0;   // the count alone
    return static_cast<Sim *>(p)->sim->getTracers(qx, qy, qz, vx, vy, vz);
}
int murbhost_sim_history_csv(void *p, const char *path)
{
    try {
        static_cast<Sim *>(p)->history->saveMetricsToCSV(path);
    } catch (const std::runtime_error &) {
        return -1;
    }
    return 0;
}

void murbhost_sim_destroy(void *p)
{
    auto *h = static_cast<Sim *>(p);
    if (h) { delete h->sim; delete h; }
}
void murbhost_sim_step(void *p, int iterations)
{
    auto *h = static_cast<Sim *>(p);
    for (int i = 0; i < iterations; ++i) h->sim->computeOneIteration();
    h->sim->synchronize();
}
// HIPBodies::initOnDevice with the scheme the simulation was created with
void murbhost_sim_init_on_device(void *p, unsigned long seed)
{
    auto *h = static_cast<Sim *>(p);
    std::dynamic_pointer_cast<HIPBodies<float>>(h->sim->getBodies())->initOnDevice(h->scheme, seed);
    // the device now holds the scheme's radii: a contact stop gets its scaled ones back
    if (auto *t = dynamic_cast<SimulationNBodyHIPTracking<float, double> *>(h->sim); t && t->hasContactStop())
        t->setContactStop(true, t->getContactScale());
}
unsigned long murbhost_sim_n(void *p) { return static_cast<Sim *>(p)->sim->getBodies()->getN(); }
float murbhost_sim_flops_per_ite(void *p) { return static_cast<Sim *>(p)->sim->getFlopsPerIte(); }
float murbhost_sim_allocated_bytes(void *p) { return static_cast<Sim *>(p)->sim->getAllocatedBytes(); }
void murbhost_sim_state(void *p, float *qx, float *qy, float *qz, float *vx, float *vy, float *vz, float *m, float *r)
{
    copyState(static_cast<Sim *>(p)->sim->getBodies()->getDataSoA(), qx, qy, qz, vx, vy, vz, m, r);
}
void murbhost_sim_acc(void *p, float *ax, float *ay, float *az)
{
    const auto &a = static_cast<Sim *>(p)->sim->getAccSoA();
    const size_t bytes = a.ax.size() * sizeof(float);
    std::memcpy(ax, a.ax.data(), bytes); std::memcpy(ay, a.ay.data(), bytes); std::memcpy(az, a.az.data(), bytes);
}

}  // extern "C"
