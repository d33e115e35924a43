// TEST INFRASTRUCTURE — fp64 direct-sum "truth" for the all-pairs acceleration.
//
// Same formula as the reference (SimulationNBodyOptim.cpp:60-76 / SimulationNBodyNaive.cpp:40-50):
//   a_i = sum_j G m_j (q_j - q_i) / (|q_j - q_i|^2 + soft^2)^(3/2)
// evaluated from the fp32 state in double precision, G taken as the reference's fp32 constant
// (SimulationNBodyInterface.hpp:18) widened to double.  Compiled WITHOUT -ffast-math.  It is the
// yardstick that tells the GPU kernel's rounding noise from cpu+optim's own (cpu+optim
// itself sits 1.2e-5 max / 3e-6 rms away from this at N = 30 000).
#include <cmath>

extern "C" {

// Accelerations (double) of bodies [i0, i1) due to all n bodies.  OpenMP over i.
void oracle_accel_f64(unsigned long n, unsigned long i0, unsigned long i1, const float* qx, const float* qy,
                      const float* qz, const float* m, float soft, double* ax, double* ay, double* az)
{
    const double G = (double)6.67384e-11f;
    const double soft2 = (double)soft * (double)soft;
#pragma omp parallel for schedule(static)
    for (unsigned long i = i0; i < i1; ++i) {
        const double xi = qx[i], yi = qy[i], zi = qz[i];
        double sx = 0.0, sy = 0.0, sz = 0.0;
        for (unsigned long j = 0; j < n; ++j) {
            const double dx = (double)qx[j] - xi, dy = (double)qy[j] - yi, dz = (double)qz[j] - zi;
            const double d2 = dx * dx + dy * dy + dz * dz + soft2;
            const double inv = 1.0 / std::sqrt(d2);
            const double f = G * (double)m[j] * inv * inv * inv;
            sx += f * dx; sy += f * dy; sz += f * dz;
        }
        ax[i - i0] = sx; ay[i - i0] = sy; az[i - i0] = sz;
    }
}

// Accelerations of an arbitrary subset of bodies (spot checks at N = 200k / 1M).
void oracle_accel_f64_subset(unsigned long n, unsigned long nsub, const unsigned long* idx, const float* qx,
                             const float* qy, const float* qz, const float* m, float soft, double* ax, double* ay,
                             double* az)
{
    const double G = (double)6.67384e-11f;
    const double soft2 = (double)soft * (double)soft;
#pragma omp parallel for schedule(static)
    for (unsigned long k = 0; k < nsub; ++k) {
        const unsigned long i = idx[k];
        const double xi = qx[i], yi = qy[i], zi = qz[i];
        double sx = 0.0, sy = 0.0, sz = 0.0;
        for (unsigned long j = 0; j < n; ++j) {
            const double dx = (double)qx[j] - xi, dy = (double)qy[j] - yi, dz = (double)qz[j] - zi;
            const double d2 = dx * dx + dy * dy + dz * dz + soft2;
            const double inv = 1.0 / std::sqrt(d2);
            const double f = G * (double)m[j] * inv * inv * inv;
            sx += f * dx; sy += f * dy; sz += f * dz;
        }
        ax[k] = sx; ay[k] = sy; az[k] = sz;
    }
}

// Mechanical energy with the reference's definitions (SimulationNBodyCUDAPropertyTracking.cu:217-304):
// kinetic = sum 1/2 m v^2, potential = -1/2 sum_i sum_{j != i} G m_i m_j / sqrt(r_ij^2 + soft^2).
void oracle_energy_f64(unsigned long n, const float* qx, const float* qy, const float* qz, const float* vx,
                       const float* vy, const float* vz, const float* m, float soft, double* kinetic, double* potential)
{
    const double G = (double)6.67384e-11f;
    const double soft2 = (double)soft * (double)soft;
    double ke = 0.0, pe = 0.0;
#pragma omp parallel for schedule(static) reduction(+ : ke, pe)
    for (unsigned long i = 0; i < n; ++i) {
        ke += 0.5 * (double)m[i] * ((double)vx[i] * vx[i] + (double)vy[i] * vy[i] + (double)vz[i] * vz[i]);
        double phi = 0.0;
        for (unsigned long j = 0; j < n; ++j) {
            if (j == i) continue;
            const double dx = (double)qx[j] - qx[i], dy = (double)qy[j] - qy[i], dz = (double)qz[j] - qz[i];
            phi += G * (double)m[j] / std::sqrt(dx * dx + dy * dy + dz * dz + soft2);
        }
        pe -= 0.5 * (double)m[i] * phi;
    }
    *kinetic = ke;
    *potential = pe;
}

// Sparse-mass probes (tests/test_pair_coverage.py): the accelerations of ALL n bodies due to the nsrc bodies src[] alone,
// O(n nsrc).  Per body also the sum of the magnitudes of its source terms c_is = G m_s d_is / (|d_is|^2 + soft^2)^(3/2)
// (the scale the probe's error is measured against) and the smallest magnitude among them, s != i (what one missing or
// doubled term would change; +inf when i has no other source).  The self term is exactly 0 and counted nowhere.
void oracle_accel_f64_sources(unsigned long n, unsigned long nsrc, const unsigned long* src, const float* qx,
                              const float* qy, const float* qz, const float* m, float soft, double* ax, double* ay,
                              double* az, double* abs_sum, double* min_term)
{
    const double G = (double)6.67384e-11f;
    const double soft2 = (double)soft * (double)soft;
#pragma omp parallel for schedule(static)
    for (unsigned long i = 0; i < n; ++i) {
        const double xi = qx[i], yi = qy[i], zi = qz[i];
        double sx = 0.0, sy = 0.0, sz = 0.0, sa = 0.0, mn = HUGE_VAL;
        for (unsigned long k = 0; k < nsrc; ++k) {
            const unsigned long j = src[k];
            if (j == i) continue;
            const double dx = (double)qx[j] - xi, dy = (double)qy[j] - yi, dz = (double)qz[j] - zi;
            const double d2 = dx * dx + dy * dy + dz * dz;
            const double inv = 1.0 / std::sqrt(d2 + soft2);
            const double f = G * (double)m[j] * inv * inv * inv;
            const double mag = f * std::sqrt(d2);
            sx += f * dx; sy += f * dy; sz += f * dz;
            sa += mag;
            mn = mag < mn ? mag : mn;
        }
        ax[i] = sx; ay[i] = sy; az[i] = sz;
        abs_sum[i] = sa;
        min_term[i] = mn;
    }
}

// The potential energy of the same probes: only pairs of sources carry mass, so the sum of oracle_energy_f64 reduces to
// -sum_{s < t} G m_s m_t / sqrt(r_st^2 + soft^2) over the nsrc bodies src[] (distinct indices).  min_pair: the smallest
// magnitude of one pair's term.
void oracle_potential_f64_sources(unsigned long nsrc, const unsigned long* src, const float* qx, const float* qy,
                                  const float* qz, const float* m, float soft, double* potential, double* min_pair)
{
    const double G = (double)6.67384e-11f;
    const double soft2 = (double)soft * (double)soft;
    double pe = 0.0, mn = HUGE_VAL;
    for (unsigned long a = 0; a < nsrc; ++a)
        for (unsigned long b = a + 1; b < nsrc; ++b) {
            const unsigned long i = src[a], j = src[b];
            const double dx = (double)qx[j] - qx[i], dy = (double)qy[j] - qy[i], dz = (double)qz[j] - qz[i];
            const double t = G * (double)m[i] * (double)m[j] / std::sqrt(dx * dx + dy * dy + dz * dz + soft2);
            pe -= t;
            mn = t < mn ? t : mn;
        }
    *potential = pe;
    *min_pair = mn;
}

}  // extern "C"
