#include "implem/SimulationNBodyHIPTracking.hpp"

#include <algorithm>
#include <cmath>

#include "murbhip.h"

template <typename T, typename Q>
SimulationNBodyHIPTracking<T, Q>::SimulationNBodyHIPTracking(const BodiesAllocatorInterface<T> &allocator,
                                                             std::shared_ptr<SimulationHistory<Q>> history, const T soft,
                                                             const int integrator, const std::vector<int> &devices,
                                                             int exchange)
    : SimulationNBodyHIP<T>(allocator, soft, devices, exchange), history{history}, adaptive{integrator == 3 || integrator == 4},
      blockSteps{integrator == 4}, hermite{integrator >= 2 && integrator <= 5}, neighbourScheme{integrator == 5}
{
    if (!this->history) this->history = std::make_shared<SimulationHistory<Q>>();
    if (integrator)
        murbhipCheck(murbhip_set_option(this->hipBodiesPtr->getContext(), "integrator", adaptive || neighbourScheme ? 2 : integrator),
                     "murbhip_set_option(integrator)");
}

template <typename T, typename Q> void SimulationNBodyHIPTracking<T, Q>::computeMetrics()
{
    murbhip_ctx *ctx = this->hipBodiesPtr->getContext();
    double kinetic = 0, potential = 0, mom[10];
    murbhipCheck(murbhip_energy(ctx, &kinetic, &potential), "murbhip_energy");
    murbhipCheck(murbhip_moments(ctx, mom), "murbhip_moments");
    if (currentIteration >= history->getNumIterations()) history->setNumIterations(currentIteration + 1);
    history->setEnergyAt(currentIteration, (Q)(kinetic + potential));
    history->setAngMomentumAt(currentIteration, (Q)std::sqrt(mom[3] * mom[3] + mom[4] * mom[4] + mom[5] * mom[5]));
    const double mass = mom[9] != 0 ? mom[9] : 1;
    if (densityCentreOn) {   // hip+tracking+density: the density centre over every body's 6 nearest in the centre of mass's place
        double out8[8];
        murbhipCheck(this->densityCentre(6, out8), "murbdensity_centre");
        history->setDensityCenterAt(currentIteration, {(Q)out8[0], (Q)out8[1], (Q)out8[2]});
        return;
    }
    history->setDensityCenterAt(currentIteration, {(Q)(mom[6] / mass), (Q)(mom[7] / mass), (Q)(mom[8] / mass)});
}

template <typename T, typename Q> bool SimulationNBodyHIPTracking<T, Q>::setEncounterRadius(const T radius)
{
    if (!adaptive || (radius > 0 && (contactStop || potentialOn))) return false;
    murbhip_ctx *ctx = this->hipBodiesPtr->getContext();
    if (radius > 0) murbhipCheck(murbhip_set_option(ctx, "nearest", 1), "murbhip_set_option(nearest)");
    murbhipCheck(murbhip_set_encounter(ctx, (float)radius), "murbhip_set_encounter");
    encounterRadius = radius;
    return true;
}

template <typename T, typename Q> bool SimulationNBodyHIPTracking<T, Q>::setContactStop(const bool on, const T scale)
{
    if (!adaptive || encounterRadius > 0 || (on && potentialOn) || !(scale > 0) || !std::isfinite((double)scale)) return false;
    murbhip_ctx *ctx = this->hipBodiesPtr->getContext();
    if (on) {
        const auto &r = this->hipBodiesPtr->getDataSoA().r;
        const unsigned long n = this->hipBodiesPtr->getN();
        std::vector<float> radii(n);
        for (unsigned long k = 0; k < n; ++k) radii[k] = (float)(r[k] * scale);
        murbhipCheck(murbhip_upload_radii(ctx, radii.data()), "murbhip_upload_radii");
    }
    murbhipCheck(murbhip_set_option(ctx, "contact", on ? 2 : 0), "murbhip_set_option(contact)");
    contactStop = on;
    contactScale = scale;
    return true;
}

template <typename T, typename Q> bool SimulationNBodyHIPTracking<T, Q>::setNeighbourScheme(const T radius, const int nIrr)
{
    if (!neighbourScheme || acBegun || !(radius >= 0) || !std::isfinite((double)radius) || nIrr < 1 || nIrr > 4096) return false;
    acRadius = radius;
    acNirr = nIrr;
    return true;
}

template <typename T, typename Q> bool SimulationNBodyHIPTracking<T, Q>::setPotential(const bool on)
{
    if (!hermite || neighbourScheme || (on && (encounterRadius > 0 || contactStop))) return false;
    murbhipCheck(murbhip_set_option(this->hipBodiesPtr->getContext(), "potential", on ? 1 : 0), "murbhip_set_option(potential)");
    potentialOn = on;
    return true;
}

template <typename T, typename Q> std::vector<float> SimulationNBodyHIPTracking<T, Q>::getPotential() const
{
    std::vector<float> phi;
    if (!potentialOn) return phi;
    phi.resize(this->hipBodiesPtr->getN());
    if (murbhip_download_potential(this->hipBodiesPtr->getContext(), phi.data()) != 0) phi.clear();   // no sweep yet
    return phi;
}

template <typename T, typename Q> void SimulationNBodyHIPTracking<T, Q>::readContacts()
{
    murbhip_ctx *ctx = this->hipBodiesPtr->getContext();
    contacts.clear();
    murbhipCheck(murbhip_contacts(ctx, nullptr, nullptr, nullptr, 0, &contactCount, &contactTime), "murbhip_contacts");
    const unsigned long kept = std::min(contactCount, 4096ul);
    if (!kept) return;
    std::vector<int> i(kept), j(kept);
    std::vector<float> gap2(kept);
    murbhipCheck(murbhip_contacts(ctx, i.data(), j.data(), gap2.data(), kept, &contactCount, &contactTime), "murbhip_contacts");
    for (unsigned long k = 0; k < kept; ++k) contacts.push_back({i[k], j[k], gap2[k]});
}

template <typename T, typename Q> void SimulationNBodyHIPTracking<T, Q>::readEncounters()
{
    murbhip_ctx *ctx = this->hipBodiesPtr->getContext();
    encounters.clear();
    murbhipCheck(murbhip_encounters(ctx, nullptr, nullptr, nullptr, 0, &encounterCount, &encounterTime), "murbhip_encounters");
    const unsigned long kept = std::min(encounterCount, 4096ul);
    if (!kept) return;
    std::vector<int> i(kept), j(kept);
    std::vector<float> r2(kept);
    murbhipCheck(murbhip_encounters(ctx, i.data(), j.data(), r2.data(), kept, &encounterCount, &encounterTime), "murbhip_encounters");
    for (unsigned long k = 0; k < kept; ++k) encounters.push_back({i[k], j[k], r2[k]});
}

template <typename T, typename Q> void SimulationNBodyHIPTracking<T, Q>::computeOneIteration()
{
    computeMetrics();
    if (blockSteps) {   // one block of dt: every body in steps of its own, all synchronised at the end
        double out[8];
        this->hipBodiesPtr->invalidateDataSoA();
        murbhipCheck(murbhip_evolve_block(this->hipBodiesPtr->getContext(), this->dt, 1ul, eta, 0.01, kmax, ~0ul, out),
                     "murbhip_evolve_block");
        dtSmallest = substeps ? std::min(dtSmallest, out[3]) : out[3];
        dtLargest = std::max(dtLargest, out[4]);
        substeps += (unsigned long)out[1];
        bodySteps += (unsigned long)out[2];
        clampedSteps += (unsigned long)out[5];
        if (encounterRadius > 0) readEncounters();
        if (contactStop) readContacts();
    } else if (adaptive) {   // exactly dt of model time, in the substeps the criterion chooses; returns synchronised
        double out[5];
        this->hipBodiesPtr->invalidateDataSoA();
        murbhipCheck(murbhip_evolve(this->hipBodiesPtr->getContext(), (double)this->dt, eta, 0.01, 0.f, this->dt, 1000000ul, out),
                     "murbhip_evolve");
        dtSmallest = substeps ? std::min(dtSmallest, out[2]) : out[2];
        dtLargest = std::max(dtLargest, out[3]);
        substeps += (unsigned long)out[1];
        if (encounterRadius > 0) readEncounters();
        if (contactStop) readContacts();
    } else if (neighbourScheme) {   // one step of dt of the neighbour scheme, begun at the first iteration
        if (!acBegun) murbhipCheck(this->acBegin((float)acRadius, acNirr), "murbac_begin");
        acBegun = true;
        murbhipCheck(this->acSteps((float)this->dt, 1), "murbac_steps");
    } else SimulationNBodyHIP<T>::computeOneIteration();
    currentIteration++;
}

template class SimulationNBodyHIPTracking<float, double>;
template class SimulationNBodyHIPTracking<float, float>;
