// Device functions the integrator launches of the MD loop share (ta_md.hip, ta_md_mtk.hip): the workgroup sum, the
// cell volume and the half-update of a Nose-Hoover chain.
#pragma once
#include <hip/hip_runtime.h>

#include "ta_device.h"
#include "ta_math.h"
#include "ta_md.h"

namespace ta {
namespace {

// the sum over the workgroup, the same value in every thread: lanes by wave_sum, waves one after another
__device__ __forceinline__ double md_block_sum(double v, double *s_wave, double *s_total) {
  v = wave_sum(v);
  const int wave = threadIdx.x >> 6, n_waves = (blockDim.x + 63) >> 6;
  if ((threadIdx.x & 63) == 0) s_wave[wave] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < n_waves; ++w) t += s_wave[w];
    *s_total = t;
  }
  __syncthreads();
  return *s_total;
}

__device__ __forceinline__ double md_cell_volume(const double *h) {
  return fabs(h[0] * (h[4] * h[8] - h[5] * h[7]) - h[1] * (h[3] * h[8] - h[5] * h[6]) + h[2] * (h[3] * h[7] - h[4] * h[6]));
}

// One half-update of a frame's chain over `delta` (thread 0 alone): L loops of d = delta / L, eta and veta
// [M] in place. K is the frame's kinetic energy before it; returns s, the factor of the frame's velocities
// (the kinetic energy is K s^2 afterwards). q1 = g kT0 tau^2, q = kT0 tau^2, gkT = g kT0.
__device__ __forceinline__ double md_nhc_half(double *eta, double *veta, int M, int L, double delta, double K,
                                              double gkT, double kT0, double q1, double q) {
  const double d = delta / (double)L, hd = 0.5 * d, qd = 0.25 * d;
  double s = 1.0;
  // the force on thermostat k from the values as they stand
  auto G = [&](int k) {
    if (k == 0) return (2.0 * K * s * s - gkT) / q1;
    return ((k == 1 ? q1 : q) * veta[k - 1] * veta[k - 1] - kT0) / q;
  };
  for (int l = 0; l < L; ++l) {
    veta[M - 1] += hd * G(M - 1);
    for (int k = M - 2; k >= 0; --k) {
      const double e = exp(-qd * veta[k + 1]);
      veta[k] = (veta[k] * e + hd * G(k)) * e;
    }
    s *= exp(-d * veta[0]);
    for (int k = 0; k < M; ++k) eta[k] += d * veta[k];
    for (int k = 0; k < M - 1; ++k) {
      const double e = exp(-qd * veta[k + 1]);
      veta[k] = (veta[k] * e + hd * G(k)) * e;
    }
    veta[M - 1] += hd * G(M - 1);
  }
  return s;
}

}  // namespace
}  // namespace ta
