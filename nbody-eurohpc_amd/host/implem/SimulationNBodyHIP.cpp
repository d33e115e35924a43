#include "implem/SimulationNBodyHIP.hpp"

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "murbbind.h"
#include "murbbound.h"
#include "murbmst.h"
#include "murbsep.h"
#include "murbfield.h"
#include "murbac.h"
#include "murbhip.h"
#include "murbknn.h"
#include "murblist.h"
#include "murbnbr.h"
#include "murbtidal.h"
#include "murbtracer.h"

template <typename T>
SimulationNBodyHIP<T>::SimulationNBodyHIP(const BodiesAllocatorInterface<T> &allocator, const T soft,
                                          const std::vector<int> &devices, int exchange)
    : SimulationNBodyInterface<T>(allocator, soft)
{
    const unsigned long n = this->getBodies()->getN();
    this->flopsPerIte = 20.f * (T)n * (T)n;   // the reference's count, every implementation (Optim.cpp:11)
    hipBodiesPtr = std::dynamic_pointer_cast<HIPBodies<T>>(this->bodies);
    if (!hipBodiesPtr) {
        std::fprintf(stderr, "SimulationNBodyHIP needs device bodies: construct it with a HIPBodiesAllocator\n");
        std::exit(EXIT_FAILURE);
    }
    hipBodiesPtr->bindDevice(this->soft, this->G, devices, exchange);
    accSoA.ax.resize(n); accSoA.ay.resize(n); accSoA.az.resize(n);
    // the device reaches its steady clock only after ~40 ms of work: get there before the caller's first
    // timed iteration.  Part of construction, like the reference's upload and GM precompute (FullDevice.cu:191-215).
    const char *ms = std::getenv("MURBHIP_WARMUP_MS");
    warmUp(ms && *ms ? std::atof(ms) : 50.0);
}

template <typename T> void SimulationNBodyHIP<T>::warmUp(double milliseconds)
{
    if (milliseconds > 0.0) murbhipCheck(murbhip_warmup(hipBodiesPtr->getContext(), milliseconds), "murbhip_warmup");
}

template <typename T> void SimulationNBodyHIP<T>::computeOneIteration()
{
    hipBodiesPtr->invalidateDataSoA();
    murbhipCheck(murbhip_step(hipBodiesPtr->getContext(), this->dt), "murbhip_step");
}

template <typename T> void SimulationNBodyHIP<T>::synchronize()
{
    murbhipCheck(murbhip_sync(hipBodiesPtr->getContext()), "murbhip_sync");
}

template <typename T> const accSoA_t<T> &SimulationNBodyHIP<T>::getAccSoA()
{
    murbhipCheck(murbhip_download_acc(hipBodiesPtr->getContext(), accSoA.ax.data(), accSoA.ay.data(),
                                      accSoA.az.data()), "murbhip_download_acc");
    return accSoA;
}

template <typename T>
int SimulationNBodyHIP<T>::fieldAt(unsigned long count, const T *px, const T *py, const T *pz, const T *pvx, const T *pvy, const T *pvz,
                                   const int *skip, T *ax, T *ay, T *az, T *jx, T *jy, T *jz, T *phi)
{
    return murbfield_at(hipBodiesPtr->getContext(), count, px, py, pz, pvx, pvy, pvz, skip, ax, ay, az, jx, jy, jz, phi);
}

template <typename T>
int SimulationNBodyHIP<T>::tidalAt(unsigned long count, const T *px, const T *py, const T *pz, const int *skip, T *txx, T *tyy, T *tzz,
                                   T *txy, T *txz, T *tyz)
{
    return murbtidal_at(hipBodiesPtr->getContext(), count, px, py, pz, skip, txx, tyy, tzz, txy, txz, tyz);
}

template <typename T> int SimulationNBodyHIP<T>::densityCentre(int k, double *out8)
{
    return murbdensity_centre(hipBodiesPtr->getContext(), k, out8);
}

template <typename T> int SimulationNBodyHIP<T>::neighboursOf(float h, std::vector<unsigned long> &offsets, std::vector<int> &idx)
{
    const unsigned long n = this->getBodies()->getN();
    offsets.assign(n + 1, 0ul);
    idx.clear();
    const int rc = murbnbr_of(hipBodiesPtr->getContext(), n, nullptr, nullptr, h, offsets.data(), nullptr, nullptr, 0);
    if (rc != 0 || offsets[n] == 0) return rc;
    idx.resize(offsets[n]);
    return murbnbr_of(hipBodiesPtr->getContext(), n, nullptr, nullptr, h, offsets.data(), idx.data(), nullptr, idx.size());
}

template <typename T>
int SimulationNBodyHIP<T>::binaries(std::vector<int> &i, std::vector<int> &j, std::vector<double> &elems, double *out8)
{
    unsigned long pairs = 0;
    i.clear();
    j.clear();
    elems.clear();
    const int rc = murbbind_pairs(hipBodiesPtr->getContext(), nullptr, nullptr, nullptr, 0, &pairs, out8);
    if (rc != 0 || pairs == 0) return rc;
    i.resize(pairs);
    j.resize(pairs);
    elems.resize(6 * pairs);
    return murbbind_pairs(hipBodiesPtr->getContext(), i.data(), j.data(), elems.data(), pairs, &pairs, out8);
}

template <typename T>
int SimulationNBodyHIP<T>::boundMembers(int maxIter, std::vector<unsigned char> &member, std::vector<double> &e, double *out16)
{
    const unsigned long n = this->getBodies()->getN();
    member.assign(n, 0);
    e.assign(n, 0.0);
    return murbbound_members(hipBodiesPtr->getContext(), nullptr, nullptr, maxIter, member.data(), e.data(), out16);
}

template <typename T>
int SimulationNBodyHIP<T>::spanningTree(std::vector<int> &i, std::vector<int> &j, std::vector<float> &r2, std::vector<double> &length,
                                        double *out8)
{
    const unsigned long n = this->getBodies()->getN(), capacity = n > 0 ? n - 1 : 0;   // a tree of n bodies has n - 1 edges
    i.assign(capacity, 0);
    j.assign(capacity, 0);
    r2.assign(capacity, 0.f);
    length.assign(capacity, 0.0);
    const int rc = murbmst_of(hipBodiesPtr->getContext(), nullptr, capacity, i.data(), j.data(), r2.data(), length.data(), nullptr, out8);
    if (rc != 0) return rc;
    const unsigned long edges = (unsigned long)out8[1];
    i.resize(edges);
    j.resize(edges);
    r2.resize(edges);
    length.resize(edges);
    return 0;
}

// the sums in index order: this file is compiled with -ffast-math, which would otherwise let the compiler reassociate them
__attribute__((optimize("no-fast-math"))) static double sumInOrder(const std::vector<double> &v)
{
    double total = 0.0;
    for (const double x : v) total += x;
    return total;
}

template <typename T>
int SimulationNBodyHIP<T>::meanSeparation(double *mean)
{
    const unsigned long n = this->getBodies()->getN();
    *mean = std::numeric_limits<double>::quiet_NaN();
    if (n < 2) return 0;
    std::vector<double> sum(n);
    const int rc = murbsep_of(hipBodiesPtr->getContext(), n, nullptr, nullptr, sum.data(), 0, 0, 0, nullptr, nullptr);
    if (rc != 0) return rc;
    *mean = sumInOrder(sum) / ((double)n * ((double)n - 1.0));
    return 0;
}

template <typename T> int SimulationNBodyHIP<T>::acBegin(float h, int nIrr)
{
    return murbac_begin(hipBodiesPtr->getContext(), nullptr, h, nIrr);
}

template <typename T> int SimulationNBodyHIP<T>::acSteps(float dt, int steps)
{
    hipBodiesPtr->invalidateDataSoA();
    return murbac_steps(hipBodiesPtr->getContext(), dt, steps);
}

template <typename T>
int SimulationNBodyHIP<T>::forceSplit(float h, std::vector<unsigned long> &counts, std::vector<float> &irregular, std::vector<float> &total,
                                      std::vector<float> &regular)
{
    const unsigned long n = this->getBodies()->getN();
    counts.assign(n, 0ul);
    irregular.assign(7 * n, 0.f);
    total.assign(7 * n, 0.f);
    regular.assign(7 * n, 0.f);
    if (n == 0) return 0;
    float *const i = irregular.data(), *const t = total.data();
    int rc = murbsplit_of(hipBodiesPtr->getContext(), n, nullptr, nullptr, h, counts.data(), i, i + n, i + 2 * n, i + 3 * n, i + 4 * n,
                          i + 5 * n, i + 6 * n);
    if (rc != 0) return rc;
    std::vector<int> all(n);
    for (unsigned long b = 0; b < n; ++b) all[b] = (int)b;
    rc = murbfield_of(hipBodiesPtr->getContext(), n, all.data(), t, t + n, t + 2 * n, t + 3 * n, t + 4 * n, t + 5 * n, t + 6 * n);
    if (rc != 0) return rc;
    for (unsigned long e = 0; e < 7 * n; ++e) regular[e] = (float)((double)total[e] - (double)irregular[e]);
    return 0;
}

template <typename T>
int SimulationNBodyHIP<T>::setTracers(unsigned long count, const T *qx, const T *qy, const T *qz, const T *vx, const T *vy, const T *vz)
{
    return murbtracer_upload(hipBodiesPtr->getContext(), count, qx, qy, qz, vx, vy, vz);
}

template <typename T> int SimulationNBodyHIP<T>::getTracers(T *qx, T *qy, T *qz, T *vx, T *vy, T *vz)
{
    return murbtracer_download(hipBodiesPtr->getContext(), qx, qy, qz, vx, vy, vz);
}

template <typename T> int SimulationNBodyHIP<T>::getTracerCount(unsigned long *count)
{
    return murbtracer_count(hipBodiesPtr->getContext(), count);
}

template class SimulationNBodyHIP<float>;
