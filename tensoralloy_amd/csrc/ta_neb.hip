// Band forces of a device-resident nudged elastic band (ta_relax_set_band): the two launches that sit
// between an evaluation and the two FIRE launches of ta_relax.hip.
//
// The resident batch of F >= 3 frames is the band: images 0 and F - 1 are fixed endpoints, images 1 .. F - 2
// move. All images have the same n atoms in the same order. With X_i, E_i, F_i the positions, energy and
// forces of image i, forces of `fixed` atoms read as 0, and ., |.| over the 3n components of an image
// (the improved tangent of Henkelman and Jonsson, J. Chem. Phys. 113, 9978; ASE's
// NEB(method='improvedtangent') with one spring constant k):
//     d+ = X_{i+1} - X_i,   d- = X_i - X_{i-1}               (plain differences, no minimum image)
//     if   E_{i+1} > E_i > E_{i-1}:  t = d+
//     elif E_{i+1} < E_i < E_{i-1}:  t = d-
//     else: hi = max(|E_{i+1}-E_i|, |E_{i-1}-E_i|), lo = min(the same two)
//           t = d+ hi + d- lo   if E_{i+1} > E_{i-1}   else   t = d+ lo + d- hi
//     tau = t / |t|                                           (t.t == 0: tau = 0)
//     B_i = F_i - (F_i.tau) tau + k (|d+| - |d-|) tau         ordinary image
//     B_c = F_c - 2 (F_c.tau) tau                             climbing image, if climb
//     B = 0 for images 0 and F - 1 and for every fixed atom
// The climbing image c is the interior image of highest energy, chosen anew by every launch; on a tie the
// lowest index wins.
//
// An interior image is cut into workgroups of `chunk` consecutive atoms, as a frame is in ta_relax.hip.
//   launch 1 (neb_reduce_kernel): every thread forms the un-normalised t of its atoms from the three images'
//     positions and the three energies (no reduction is needed for that); the workgroup leaves ONE partial
//     (t.t, F.t, d+.d+, d-.d-): threads in a fixed order, waves one after another, no floating-point atomics.
//   launch 2 (neb_apply_kernel): every workgroup adds the partials of its image in one fixed order (its first
//     wave: lane l takes partials l, l + 64, ..., then the lanes as in wave_sum), so all workgroups of an image
//     hold bitwise the same four numbers; thread 0 scans the F energies for the climbing image; then B goes
//     into the band-force array, and tau into a second one when the launch asks for it. It reads nothing that
//     a workgroup of the same launch writes.
// Both launches are predicated on the status word like the FIRE launches: behind a drift that left the list
// stale they return at once. The FIRE launches then run on B with the whole band as one pseudo-frame.
#include <hip/hip_runtime.h>

#include "ta_device.h"
#include "ta_math.h"
#include "ta_md_sweep.h"
#include "ta_neb.h"

namespace ta {
namespace {

constexpr int kNebThreads = 256;

// t = wp d+ + wm d- of an interior image from the energies of its lower neighbour, itself and its upper one
__device__ __forceinline__ void neb_tangent_weights(double em, double e0, double ep, double &wp, double &wm) {
  if (ep > e0 && e0 > em) {
    wp = 1.0, wm = 0.0;
  } else if (ep < e0 && e0 < em) {
    wp = 0.0, wm = 1.0;
  } else {
    const double up = fabs(ep - e0), dn = fabs(em - e0);
    const double hi = !(up <= dn) ? up : dn, lo = !(up <= dn) ? dn : up;  // (a NaN energy reaches t)
    if (ep > em) wp = hi, wm = lo; else wp = lo, wm = hi;
  }
}

__global__ __launch_bounds__(kNebThreads) void neb_reduce_kernel(NebLaunch a) {
  __shared__ double s_wave[4][kNebThreads / 64];
  if (md_stale(a.status, a.seq)) return;
  const int img = 1 + (int)blockIdx.x / a.blk_per_image;  // interior: 1 .. F - 2
  const int lo = ((int)blockIdx.x % a.blk_per_image) * a.chunk;
  const int hi = lo + a.chunk < a.n ? lo + a.chunk : a.n;
  double wp, wm;
  neb_tangent_weights(a.energy[img - 1], a.energy[img], a.energy[img + 1], wp, wm);
  const int64_t stride = 3 * (int64_t)a.n;
  const double *x0 = a.pos + img * stride, *xm = x0 - stride, *xp = x0 + stride;
  const double *f0 = a.forces + img * stride;
  const uint8_t *fixed = a.fixed + (int64_t)img * a.n;

  double tt = 0.0, ft = 0.0, pp = 0.0, mm = 0.0;
  for (int j = lo + (int)threadIdx.x; j < hi; j += kNebThreads) {
    const bool free_atom = !fixed[j];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double x = x0[3 * j + c];
      const double dp = xp[3 * j + c] - x, dm = x - xm[3 * j + c];
      const double t = wp * dp + wm * dm;
      tt += t * t;
      if (free_atom) ft += f0[3 * j + c] * t;
      pp += dp * dp;
      mm += dm * dm;
    }
  }
  tt = wave_sum(tt);
  ft = wave_sum(ft);
  pp = wave_sum(pp);
  mm = wave_sum(mm);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_wave[0][wave] = tt;
    s_wave[1][wave] = ft;
    s_wave[2][wave] = pp;
    s_wave[3][wave] = mm;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    double t = s_wave[threadIdx.x][0];
    for (int w = 1; w < kNebThreads / 64; ++w) t += s_wave[threadIdx.x][w];
    a.part[4 * (size_t)blockIdx.x + threadIdx.x] = t;
  }
}

__global__ __launch_bounds__(kNebThreads) void neb_apply_kernel(NebLaunch a) {
  __shared__ double s_sum[4];
  __shared__ int s_climb;
  if (md_stale(a.status, a.seq)) return;
  const int img = 1 + (int)blockIdx.x / a.blk_per_image;
  const int lo = ((int)blockIdx.x % a.blk_per_image) * a.chunk;
  const int hi = lo + a.chunk < a.n ? lo + a.chunk : a.n;
  if (threadIdx.x < 64) {
    // the first wave: lane l adds partials l, l + 64, ... of the image, then the lanes are added as in
    // wave_sum; the order depends on the band's layout alone, so it is the same in every workgroup
    double tt = 0.0, ft = 0.0, pp = 0.0, mm = 0.0;
    const int b0 = (img - 1) * a.blk_per_image;
    for (int b = (int)threadIdx.x; b < a.blk_per_image; b += 64) {
      const double *p = a.part + 4 * (size_t)(b0 + b);
      tt += p[0];
      ft += p[1];
      pp += p[2];
      mm += p[3];
    }
    tt = wave_sum(tt);
    ft = wave_sum(ft);
    pp = wave_sum(pp);
    mm = wave_sum(mm);
    if (threadIdx.x == 0) {
      s_sum[0] = tt, s_sum[1] = ft, s_sum[2] = pp, s_sum[3] = mm;
      int c = -1;
      if (a.climb) {  // the interior image of highest energy; a tie goes to the lowest index
        c = 1;
        for (int i = 2; i < a.n_images - 1; ++i)
          if (a.energy[i] > a.energy[c]) c = i;
      }
      s_climb = c;
      if (blockIdx.x == 0) *a.climbing = c;
    }
  }
  __syncthreads();
  const double tt = s_sum[0], ft = s_sum[1];
  const double inv = tt == 0.0 ? 0.0 : 1.0 / sqrt(tt);  // tau = t inv
  const double ftau = ft * inv;                         // F.tau
  const double along = s_climb == img ? -2.0 * ftau : a.k * (sqrt(s_sum[2]) - sqrt(s_sum[3])) - ftau;
  double wp, wm;
  neb_tangent_weights(a.energy[img - 1], a.energy[img], a.energy[img + 1], wp, wm);
  const int64_t stride = 3 * (int64_t)a.n;
  const double *x0 = a.pos + img * stride, *xm = x0 - stride, *xp = x0 + stride;
  const double *f0 = a.forces + img * stride;
  const uint8_t *fixed = a.fixed + (int64_t)img * a.n;
  double *band = a.band + img * stride;
  double *tau_out = a.tau ? a.tau + img * stride : nullptr;
  for (int j = lo + (int)threadIdx.x; j < hi; j += kNebThreads) {
    const bool free_atom = !fixed[j];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double x = x0[3 * j + c];
      const double tau = (wp * (xp[3 * j + c] - x) + wm * (x - xm[3 * j + c])) * inv;
      band[3 * j + c] = free_atom ? f0[3 * j + c] + along * tau : 0.0;
      if (tau_out) tau_out[3 * j + c] = tau;
    }
  }
}

}  // namespace

void launch_neb_force(const NebLaunch &a, hipStream_t s) {
  const int n_blk = (a.n_images - 2) * a.blk_per_image;
  if (n_blk <= 0) return;
  hipLaunchKernelGGL(neb_reduce_kernel, dim3((unsigned)n_blk), dim3(kNebThreads), 0, s, a);
  hipLaunchKernelGGL(neb_apply_kernel, dim3((unsigned)n_blk), dim3(kNebThreads), 0, s, a);
}

}  // namespace ta
