// Device-resident MD loop: the integrator launch of the Martyna-Tobias-Klein barostat (ta_md_set_mtk_barostat), the
// isothermal-isobaric ensemble with an isotropic or a diagonal strain rate, coupled to the Nose-Hoover chain of
// ta_md.hip and to a chain of its own (Martyna, Tobias, Klein, J. Chem. Phys. 101, 4177; the measure-preserving
// integrator of Tuckerman et al., J. Phys. A 39, 5629). The scheme, its masses and the conserved quantity are
// spelled out in include/tensoralloy_amd.h; the numbers below are those of its steps.
//
// One workgroup owns a whole frame, as in the chain and the Berendsen-barostat builds of md_integrate_kernel, and
// one launch closes step k (7, 8, 9), records, and opens step k + 1 (1 .. 5). The per-axis velocity factors are
// scalars of the frame, so ONE reduction of S_c = sum m v_c^2 after the pending half-kick serves everything:
//   first loop    v += dt/2 F/m (the half-kick of 7), S_x, S_y, S_z
//   thread 0      S_c <- exp(-dt alpha_c) S_c (the rest of 7); 8; 9 with S <- s^2 S; the record
//                 (K, epot, E_chain, E_baro, V, P_c of the state after 9); 1 with S <- s^2 S; 2; 3; the factors of 4
//                 and 5; the new cell into db.cells, s_c = prod exp(omega_c dt) since the list was built into
//                 baro_scale, and the limit of the strain-aware list test of the Berendsen barostat
//   second loop   v_c <- lambda_c v_c + dt/2 F/m with lambda_c = exp(-dt/2 alpha_c) s (closing) times s exp(-dt/2
//                 alpha_c') (opening); x_c <- exp(omega_c dt) x_c + dt exp(omega_c dt/2) v_c; the list test
// The last launch of a run (no drift) writes v_c <- (closing factor)_c s v_c instead. Everything thread 0 does is
// fp64 in a fixed order, without atomics, and sits behind the early return on the status word: a launch enqueued
// behind a stale list leaves omega and both chains alone. An exp(omega_c dt) that is not a finite number > 0 is
// made a NaN, which the host finds in the cells it downloads before the rebuild, as under the Berendsen barostat.
//
// No sampler that takes a snapshot from the integrator launch (ta_md_set_sampling, _sq, _flux) runs under a
// barostat, so this launch has no build that stores one.
#include <hip/hip_runtime.h>

#include "ta_device.h"
#include "ta_md.h"
#include "ta_md_device.h"
#include "ta_md_sweep.h"

namespace ta {
namespace {

// slots of the LDS block: the factors for the second loop, then the two chains while thread 0 works
constexpr int kMtkLambda = 0, kMtkE1 = 3, kMtkDtE2 = 6, kMtkScale = 9, kMtkLim2 = 12, kMtkEta = 13,
              kMtkVeta = kMtkEta + kMdMaxChain, kMtkXi = kMtkVeta + kMdMaxChain, kMtkVxi = kMtkXi + kMdMaxChain,
              kMtkWords = kMtkVxi + kMdMaxChain;

__global__ __launch_bounds__(1024) void md_integrate_mtk_kernel(MdLaunch a, MdMtkLaunch b) {
  __shared__ double s_wave[16];
  __shared__ double s_total;
  __shared__ double s_mtk[kMtkWords];
  // (0, or the value this very launch writes, or the mark of an earlier launch: the same branch in every thread)
  if (md_stale(a.status, a.seq)) return;
  const int f = (int)blockIdx.x;  // (the host made every workgroup a whole frame)
  const int64_t lo = a.atom_start[f], hi = a.atom_start[f + 1];
  const double hdt = 0.5 * a.dt;

  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    const double m = a.mass[i];
    double vx = a.vel[3 * i], vy = a.vel[3 * i + 1], vz = a.vel[3 * i + 2];
    if (a.kick2) {
      vx += hdt * a.forces[3 * i] / m;
      vy += hdt * a.forces[3 * i + 1] / m;
      vz += hdt * a.forces[3 * i + 2] / m;
      a.vel[3 * i] = vx;
      a.vel[3 * i + 1] = vy;
      a.vel[3 * i + 2] = vz;
    }
    sx += m * vx * vx;
    sy += m * vy * vy;
    sz += m * vz * vz;
  }
  sx = md_block_sum(sx, s_wave, &s_total);
  sy = md_block_sum(sy, s_wave, &s_total);
  sz = md_block_sum(sz, s_wave, &s_total);

  if (threadIdx.x == 0) {
    const int M = a.nhc_chain, Mp = b.chain;
    double *eta = s_mtk + kMtkEta, *veta = s_mtk + kMtkVeta, *xi = s_mtk + kMtkXi, *vxi = s_mtk + kMtkVxi;
    const size_t c0 = (size_t)f * kMdMaxChain;
    for (int k = 0; k < M; ++k) eta[k] = a.nhc_eta[c0 + k], veta[k] = a.nhc_veta[c0 + k];
    for (int k = 0; k < Mp; ++k) xi[k] = b.xi[c0 + k], vxi[k] = b.vxi[c0 + k];
    double om[3], S[3] = {sx, sy, sz}, h[9], free[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      om[c] = b.omega[3 * (size_t)f + c];
      free[c] = (b.iso || b.mask[c]) ? 1.0 : 0.0;
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) h[c] = a.cells[9 * (size_t)f + c];
    const double *W = a.virial + 9 * (size_t)f;
    const double kT0 = a.nhc_kT0;
    const double g = 3.0 * (double)(hi - lo) - (double)a.nhc_dof;  // (the host refused g < 1)
    const double gkT = g * kT0, q1 = g * a.nhc_q;
    const double db = b.iso ? 1.0 : free[0] + free[1] + free[2];
    const double dkT = db * kT0, qb1 = db * b.q, Wc = (g + 3.0) * b.q / 3.0;
    double V = md_cell_volume(h);
    // 3 and 8: omega_c += dt/2 G_c from S, V and the virial as they stand
    auto kick_omega = [&]() {
      const double K = 0.5 * (S[0] + S[1] + S[2]);
      double G[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) G[c] = free[c] * (S[c] - W[4 * c] - b.p0 * V + 2.0 * K / g) / Wc;
      if (b.iso) G[0] = G[1] = G[2] = (G[0] + G[1] + G[2]) / 3.0;
#pragma unroll
      for (int c = 0; c < 3; ++c) om[c] += hdt * G[c];
    };
    // 2 and the first part of 9: the barostat's chain from K_b, omega <- s_b omega
    auto chain_omega = [&]() {
      const double Kb = 0.5 * Wc * (om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
      const double sb = md_nhc_half(xi, vxi, Mp, b.loops, hdt, Kb, dkT, kT0, qb1, b.q);
#pragma unroll
      for (int c = 0; c < 3; ++c) om[c] *= sb;
    };
    // 1 and the second part of 9: the particle chain from K, S <- s^2 S
    auto chain_particles = [&]() {
      const double s = md_nhc_half(eta, veta, M, a.nhc_loops, hdt, 0.5 * (S[0] + S[1] + S[2]), gkT, kT0, q1, a.nhc_q);
#pragma unroll
      for (int c = 0; c < 3; ++c) S[c] *= s * s;
      return s;
    };
    // the factors of 4 and 7: exp(-dt/2 alpha_c), S_c taking its square
    auto strain_factors = [&](double *e) {
      const double tr = (om[0] + om[1] + om[2]) / g;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        e[c] = exp(-hdt * (om[c] + tr));
        S[c] *= e[c] * e[c];
      }
    };
    double lam[3] = {1.0, 1.0, 1.0};
    if (a.kick2) {  // close step k: the rest of 7, then 8 and 9
      strain_factors(lam);
      kick_omega();
      chain_omega();
      const double s1 = chain_particles();
#pragma unroll
      for (int c = 0; c < 3; ++c) lam[c] *= s1;
    }
    if (a.rec >= 0) {  // the state after the closing half-updates
      const size_t r = (size_t)a.rec * a.n_frames + f;
      a.ke_part[(size_t)a.rec * a.n_blk + blockIdx.x] = 0.5 * (S[0] + S[1] + S[2]);
      a.epot[r] = a.energy[f];
      double e = 0.5 * q1 * veta[0] * veta[0] + gkT * eta[0];
      for (int k = 1; k < M; ++k) e += 0.5 * a.nhc_q * veta[k] * veta[k] + kT0 * eta[k];
      a.nhc_rec[r] = e;
      e = b.p0 * V + 0.5 * Wc * (om[0] * om[0] + om[1] * om[1] + om[2] * om[2]) + 0.5 * qb1 * vxi[0] * vxi[0] + dkT * xi[0];
      for (int k = 1; k < Mp; ++k) e += 0.5 * b.q * vxi[k] * vxi[k] + kT0 * xi[k];
      b.rec[r] = e;
      double *br = a.baro_rec + 4 * r;
      br[0] = V, br[1] = (S[0] - W[0]) / V, br[2] = (S[1] - W[4]) / V, br[3] = (S[2] - W[8]) / V;
    }
    if (a.drift) {  // open step k + 1: 1, 2, 3 and the factors of 4 and 5
      const double s2 = chain_particles();
      chain_omega();
      kick_omega();
      double e4[3];
      strain_factors(e4);
      double n2 = 0.0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        lam[c] *= s2 * e4[c];
        double e1 = exp(om[c] * a.dt);
        if (!(e1 > 0.0) || isinf(e1)) e1 = nan("");  // (the host finds it in the cells)
        const double s_c = a.baro_scale[3 * (size_t)f + c] * e1;
        a.baro_scale[3 * (size_t)f + c] = s_c;
        s_mtk[kMtkE1 + c] = e1;
        s_mtk[kMtkDtE2 + c] = a.dt * exp(om[c] * hdt);
        s_mtk[kMtkScale + c] = s_c;
        n2 += (s_c - 1.0) * (s_c - 1.0);
#pragma unroll
        for (int r = 0; r < 3; ++r) a.cells[9 * (size_t)f + 3 * r + c] = h[3 * r + c] * e1;
      }
      const double lim = 0.5 * (a.skin - a.r_list * sqrt(n2));
      s_mtk[kMtkLim2] = lim > 0.0 ? lim * lim : -1.0;  // (a NaN strain: -1, every drift is stale)
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      s_mtk[kMtkLambda + c] = lam[c];
      b.omega[3 * (size_t)f + c] = om[c];
    }
    for (int k = 0; k < M; ++k) a.nhc_eta[c0 + k] = eta[k], a.nhc_veta[c0 + k] = veta[k];
    for (int k = 0; k < Mp; ++k) b.xi[c0 + k] = xi[k], b.vxi[c0 + k] = vxi[k];
  }
  __syncthreads();
  const double lam[3] = {s_mtk[kMtkLambda], s_mtk[kMtkLambda + 1], s_mtk[kMtkLambda + 2]};
  if (!a.drift) {  // the run ends on a whole step: the closing factors go into the velocities now
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
#pragma unroll
      for (int c = 0; c < 3; ++c) a.vel[3 * i + c] = lam[c] * a.vel[3 * i + c];
    }
    return;
  }
  double e1[3], dte2[3], sc[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) e1[c] = s_mtk[kMtkE1 + c], dte2[c] = s_mtk[kMtkDtE2 + c], sc[c] = s_mtk[kMtkScale + c];
  const double lim2 = s_mtk[kMtkLim2];
  int stale = 0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {  // (each thread meets its own atoms again)
    const double m = a.mass[i];
    double d2 = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double v = lam[c] * a.vel[3 * i + c] + hdt * a.forces[3 * i + c] / m;
      a.vel[3 * i + c] = v;
      const double x = e1[c] * a.pos[3 * i + c] + dte2[c] * v;
      a.pos[3 * i + c] = x;
      const double d = x - a.ref[3 * i + c] * sc[c];  // u = x_{k+1} - x_ref o s
      d2 += d * d;
    }
    stale |= !(d2 < lim2) ? 1 : 0;  // (a NaN fails the comparison too and is reported by the rebuild)
  }
  if (threadIdx.x == 0 && !(lim2 > 0.0)) stale = 1;
  if (__syncthreads_or(stale) && threadIdx.x == 0) {
    *static_cast<volatile unsigned *>(a.status) = a.seq + 1u;
    *static_cast<volatile unsigned *>(a.status_host) = a.seq + 1u;
  }
}

}  // namespace

void launch_md_mtk(const MdLaunch &a, const MdMtkLaunch &b, hipStream_t s) {
  if (a.n_frames <= 0) return;
  hipLaunchKernelGGL(md_integrate_mtk_kernel, dim3((unsigned)a.n_frames), dim3(1024), 0, s, a, b);
}

}  // namespace ta
