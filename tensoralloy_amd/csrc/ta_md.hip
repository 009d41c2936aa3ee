// Device-resident MD loop (ta_md_run): the integrator launch that sits between two force evaluations.
//
// Velocity Verlet as ASE's VelocityVerlet, Berendsen as NVTBerendsen.scale_velocities (no centre-of-mass
// fix), in the library's consistent units (a = F / m). One launch does, in this order:
//   1. the second half-kick of step k             v_k  = v' + dt/2 F_k / m
//   2. the kinetic energy of v_k, per workgroup, and the frame's potential energy, into the record
//   3. the Berendsen factor of the frame          v_k <- lambda v_k
//   4. the first half-kick of step k + 1          v'   = v_k + dt/2 F_k / m
//   5. the drift                                  x_{k+1} = x_k + dt v'
//   6. the skin test of ta_update_positions       !(|x_{k+1} - x_ref|^2 <= skin^2 / 4)
//
// A frame is cut into workgroups of `chunk` consecutive atoms; every workgroup leaves ONE kinetic-energy
// partial per record (threads in a fixed order, no floating-point atomics), which the host adds up frame by
// frame in workgroup order when the run returns. With a thermostat the factor of a frame needs the frame's
// whole kinetic energy before any velocity is scaled, so the host then makes `chunk` the largest frame
// (one workgroup per frame, 1024 threads).
//
// Langevin dynamics (md_integrate_kernel<true>) is ASE's second-order Langevin step without its
// centre-of-mass correction. Per atom and component, with the normals xi, eta of the step:
//     rv = c3_i xi - c4_i eta;  rp = c5_i eta
//     v += c1 F(x)/m - c2 v + rv;   x += dt v + rp;   v += c1 F(x_new)/m - c2 v + rv
// so the launch finishes step k - 1 with the noise of step k - 1, writes the record, and begins step k with
// the noise of step k. The normals are a pure function of (seed, absolute step, atom, component):
// Philox4x32-10 with key (seed lo, seed hi) and counter (atom, component, step lo, step hi), then
// Box-Muller on two 53-bit uniforms. Nothing per atom is kept between launches, and a step that is redone
// after a rebuild, enqueued behind a stale list or split over two runs draws the same numbers. There is
// no per-frame factor, so the chunked layout holds at any frame size.
//
// The barostat builds (md_integrate_kernel<., true>; ta_md_set_barostat) are ASE's NPTBerendsen (isotropic)
// and Inhomogeneous_NPTBerendsen (per axis) with ONE force evaluation per step. Per frame, with h the cell
// (rows are lattice vectors), V = |det h|, W the virial (dE / d strain) of the evaluation at x_k and S_c the
// sum of m v_c^2 over the frame's atoms, between steps 3 and 4 above (Langevin: before the first update):
//     P_c = (S_c - W_cc) / V            from the velocities as they stand, i.e. after the Berendsen factor
//     mu_c = 1 - (dt / taup) (beta / 3) (P0 - P_c)     isotropic: P_c -> (P_x + P_y + P_z) / 3; masked axis: 1
//     x_ic <- mu_c x_ic,  h[:, c] <- mu_c h[:, c]      velocities are not scaled, mu is not clamped
// The kicks and the drift of the step then use F_k, the forces at the UNSCALED x_k: what ASE does when forces
// are handed to step(); ASE evaluates again after the scaling when none are handed in, a difference of order
// 1 - mu per step. The three sums are needed before any position is scaled, so one workgroup owns a whole
// frame as with the Berendsen thermostat, under every thermostat setting; the recorded kinetic energy is
// (S_x + S_y + S_z) / 2, and the record also takes V and P_c of the recorded state (S_c before the Berendsen
// factor). Thread 0 writes the new cell into db.cells, which no other thread of the launch reads, and keeps
// s_c, the product of the mu_c since the list was built: h = h_ref diag(s), so with u_i = x_i - x_ref,i o s
// the list is stale when lim = (skin - (rc + skin) |s - 1|_2) / 2 <= 0 or some |u_i|^2 >= lim^2, the rule of
// ta_relax.hip with A = diag(s). A mu_c that is not a finite number > 0 is made a NaN, which the host finds
// in the cells it downloads before the rebuild.
//
// The Nose-Hoover chain builds (md_integrate_kernel<false, ., true>; ta_md_set_nose_hoover) wrap the velocity
// Verlet step into two half-updates of a chain of M thermostats per frame (Martyna, Tuckerman, Tobias, Klein,
// Mol. Phys. 87, 1117; masses as LAMMPS fix nvt, names as ASE's NoseHooverChainNVT; the scheme is spelled out
// in include/tensoralloy_amd.h). A half-update needs the frame's kinetic energy K and gives a factor s for the
// frame's velocities, so one workgroup owns a whole frame and one reduction serves both half-updates of a
// launch: after the pending half-kick and K, thread 0 closes step k (s1, K <- s1^2 K), the record takes
// K, epot and the chain terms of the conserved quantity, thread 0 opens step k + 1 from the updated K (s2),
// and the second loop scales by lambda = s1 s2 before its half-kick. The last launch of a run (no drift)
// writes v <- s1 v instead. Thread 0 keeps eta and veta in LDS while it works, in fp64 with exp(), and
// writes them back to [F][kMdMaxChain] arrays; the factors reach the other threads through LDS. All of it
// sits behind the early return on the status word: a launch enqueued behind a stale list leaves the chain alone.
//
// Sampling (ta_md_set_sampling): a launch whose step is due gets the rows of this sample in the position and the
// velocity ring (snap_x, snap_v; null otherwise) and runs the kSnap build of its variant. It stores x_k as it finds it,
// before its drift, and v_k as the record's kinetic energy sees it: after the pending half-kick (Langevin: the
// second update) in the first loop, under the chain s1 v behind the reduction, on the drift and on the no-drift
// path. The stores sit behind the early return; a launch that does not sample runs the build without them.
//
// The launch is predicated on a device word: a drift that finds an atom beyond skin / 2 writes its own
// sequence number + 1 there (and into a page-locked word the host reads after a stream wait), still
// writes valid positions, and every LATER launch returns at once. The host may therefore enqueue several
// steps ahead; the evaluations it enqueued for the stale list are overwritten after the rebuild.
#include <hip/hip_runtime.h>

#include "ta_device.h"
#include "ta_math.h"
#include "ta_md.h"
#include "ta_md_device.h"
#include "ta_md_sweep.h"

namespace ta {
namespace {

// Philox4x32-10 (Salmon et al., SC'11): ten rounds of two 32 x 32 -> 64 bit products
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(M0, c[0]), l0 = M0 * c[0], h1 = __umulhi(M1, c[2]), l1 = M1 * c[2];
    c[0] = h1 ^ c[1] ^ k0;
    c[1] = l1;
    c[2] = h0 ^ c[3] ^ k1;
    c[3] = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// the two standard normals of (seed, step, atom, component): u in (0, 1) from 27 + 26 bits, Box-Muller
__device__ __forceinline__ void md_normals(unsigned long long seed, long long step, uint32_t atom, uint32_t comp,
                                           double *xi, double *eta) {
  uint32_t w[4] = {atom, comp, (uint32_t)((unsigned long long)step & 0xffffffffull),
                   (uint32_t)((unsigned long long)step >> 32)};
  philox4x32_10(w, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32));
  const double u1 = ((double)(w[0] >> 5) * 67108864.0 + (double)(w[1] >> 6) + 0.5) * 0x1p-53;
  const double u2 = ((double)(w[2] >> 5) * 67108864.0 + (double)(w[3] >> 6) + 0.5) * 0x1p-53;
  const double r = sqrt(-2.0 * log(u1));
  double sn, cs;
  sincos(6.283185307179586 * u2, &sn, &cs);
  *xi = r * cs;
  *eta = r * sn;
}

__global__ __launch_bounds__(256) void md_noise_kernel(unsigned long long seed, long long step, long long n3,
                                                       double *xi, double *eta) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n3) return;
  md_normals(seed, step, (uint32_t)(j / 3), (uint32_t)(j % 3), &xi[j], &eta[j]);
}

// slots of the barostat's LDS block
constexpr int kBaroMu = 0, kBaroScale = 3, kBaroLim2 = 6, kBaroWords = 7;
// slots of the Nose-Hoover chain's LDS block
constexpr int kNhcS1 = 0, kNhcS2 = 1, kNhcEta = 2, kNhcVeta = 2 + kMdMaxChain, kNhcWords = 2 + 2 * kMdMaxChain;

// kLangevin = false: velocity Verlet with the optional Berendsen factor; true: the Langevin step.
// kBaro: the Berendsen barostat before the step (one workgroup per frame)
// kNhc: the Nose-Hoover chain around the velocity Verlet step (one workgroup per frame; never with kLangevin)
// kSnap: this launch samples (snap_x, snap_v are rows of the rings); without it the build is the one it was
template <bool kLangevin, bool kBaro, bool kNhc = false, bool kSnap = false>
__global__ __launch_bounds__(1024) void md_integrate_kernel(MdLaunch a) {
  __shared__ double s_wave[16];
  __shared__ double s_total;
  __shared__ double s_baro[kBaro ? kBaroWords : 1];  // (unused, and dropped, in the fixed-cell builds)
  __shared__ double s_nhc[kNhc ? kNhcWords : 1];     // (likewise without the chain)
  // (0, or the value this very launch writes, or the mark of an earlier launch: the same branch in every thread)
  if (md_stale(a.status, a.seq)) return;
  const int f = md_frame_of(a.blk_start, a.n_frames, (int)blockIdx.x);
  const int blk0 = a.blk_start[f];
  const int64_t f_lo = a.atom_start[f], f_hi = a.atom_start[f + 1];
  const int64_t lo = f_lo + (int64_t)((int)blockIdx.x - blk0) * a.chunk;
  const int64_t hi = lo + a.chunk < f_hi ? lo + a.chunk : f_hi;
  const double hdt = 0.5 * a.dt;

  double ke = 0.0;
  double sx = 0.0, sy = 0.0, sz = 0.0;  // (kBaro: the frame's sums of m v_c^2)
  for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    const double m = a.mass[i];
    double vx = a.vel[3 * i], vy = a.vel[3 * i + 1], vz = a.vel[3 * i + 2];
    if constexpr (kLangevin) {
      if (a.kick2) {  // the second update of the step before, with that step's noise
        const double rsm = 1.0 / sqrt(m);
        double v[3] = {vx, vy, vz};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          double xi, eta;
          md_normals(a.seed, a.step - 1, (uint32_t)i, (uint32_t)c, &xi, &eta);
          const double rv = a.c3 * rsm * xi - a.c4 * rsm * eta;
          v[c] += a.c1 * a.forces[3 * i + c] / m - a.c2 * v[c] + rv;
          a.vel[3 * i + c] = v[c];
        }
        vx = v[0], vy = v[1], vz = v[2];
      }
    } else if (a.kick2) {
      vx += hdt * a.forces[3 * i] / m;
      vy += hdt * a.forces[3 * i + 1] / m;
      vz += hdt * a.forces[3 * i + 2] / m;
      a.vel[3 * i] = vx;
      a.vel[3 * i + 1] = vy;
      a.vel[3 * i + 2] = vz;
    }
    if constexpr (kSnap) {  // the whole-step state of this launch's step; the chain's v waits for s1
      a.snap_x[3 * i] = a.pos[3 * i], a.snap_x[3 * i + 1] = a.pos[3 * i + 1], a.snap_x[3 * i + 2] = a.pos[3 * i + 2];
      if constexpr (!kNhc) a.snap_v[3 * i] = vx, a.snap_v[3 * i + 1] = vy, a.snap_v[3 * i + 2] = vz;
    }
    if constexpr (kBaro) {
      sx += m * vx * vx;
      sy += m * vy * vy;
      sz += m * vz * vz;
    } else {
      ke += 0.5 * m * (vx * vx + vy * vy + vz * vz);
    }
  }
  if constexpr (kBaro) {
    sx = md_block_sum(sx, s_wave, &s_total);
    sy = md_block_sum(sy, s_wave, &s_total);
    sz = md_block_sum(sz, s_wave, &s_total);
    ke = 0.5 * (sx + sy + sz);
  } else {
    ke = md_block_sum(ke, s_wave, &s_total);
  }
  double s1 = 1.0, s2 = 1.0;  // (kNhc: the factors of the closing and of the opening half-update)
  if constexpr (kNhc) {
    if (threadIdx.x == 0) {
      const int M = a.nhc_chain;
      double *eta = s_nhc + kNhcEta, *veta = s_nhc + kNhcVeta;
      const size_t c0 = (size_t)f * kMdMaxChain;
      for (int k = 0; k < M; ++k) eta[k] = a.nhc_eta[c0 + k], veta[k] = a.nhc_veta[c0 + k];
      const double g = 3.0 * (double)(f_hi - f_lo) - (double)a.nhc_dof;  // (the host refused g < 1)
      const double gkT = g * a.nhc_kT0, q1 = g * a.nhc_q;
      if (a.kick2) s1 = md_nhc_half(eta, veta, M, a.nhc_loops, hdt, ke, gkT, a.nhc_kT0, q1, a.nhc_q);
      if (a.rec >= 0) {  // the chain terms of H' beside K s1^2 and epot
        double e = 0.5 * q1 * veta[0] * veta[0] + gkT * eta[0];
        for (int k = 1; k < M; ++k) e += 0.5 * a.nhc_q * veta[k] * veta[k] + a.nhc_kT0 * eta[k];
        a.nhc_rec[(size_t)a.rec * a.n_frames + f] = e;
      }
      if (a.drift) s2 = md_nhc_half(eta, veta, M, a.nhc_loops, hdt, ke * (s1 * s1), gkT, a.nhc_kT0, q1, a.nhc_q);
      for (int k = 0; k < M; ++k) a.nhc_eta[c0 + k] = eta[k], a.nhc_veta[c0 + k] = veta[k];
      s_nhc[kNhcS1] = s1, s_nhc[kNhcS2] = s2;
    }
    __syncthreads();
    s1 = s_nhc[kNhcS1], s2 = s_nhc[kNhcS2];
    const double s1sq = s1 * s1;  // the recorded state is the one after the closing half-update
    ke *= s1sq;
    if constexpr (kBaro) sx *= s1sq, sy *= s1sq, sz *= s1sq;
  }
  if (threadIdx.x == 0 && a.rec >= 0) {
    a.ke_part[(size_t)a.rec * a.n_blk + blockIdx.x] = ke;
    if ((int)blockIdx.x == blk0) a.epot[(size_t)a.rec * a.n_frames + f] = a.energy[f];
    if constexpr (kBaro) {  // V and P_c of the recorded state
      const double *h = a.cells + 9 * (size_t)f, *W = a.virial + 9 * (size_t)f;
      const double V = md_cell_volume(h);
      double *r = a.baro_rec + 4 * ((size_t)a.rec * a.n_frames + f);
      r[0] = V, r[1] = (sx - W[0]) / V, r[2] = (sy - W[4]) / V, r[3] = (sz - W[8]) / V;
    }
  }
  if constexpr (kNhc) {
    if (!a.drift) {  // the run ends on a whole step: the closing factor goes into the velocities now
      for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double v = s1 * a.vel[3 * i + c];
          a.vel[3 * i + c] = v;
          if constexpr (kSnap) a.snap_v[3 * i + c] = v;
        }
      }
      return;
    }
  }
  if (!a.drift) return;

  double lambda = 1.0;
  if (!kLangevin && a.kT0 > 0.0 && ke > 0.0) {  // (the host made this workgroup the whole frame)
    const double kT = 2.0 * ke / (3.0 * (double)(f_hi - f_lo));
    lambda = sqrt(1.0 + (a.kT0 / kT - 1.0) * a.dt_over_tau);
    lambda = lambda > 1.1 ? 1.1 : (lambda < 0.9 ? 0.9 : lambda);
  }
  if constexpr (kNhc) lambda = s1 * s2;
  int stale = 0;
  double mu[3] = {1.0, 1.0, 1.0}, sc[3] = {1.0, 1.0, 1.0}, lim2 = a.lim2;
  if constexpr (kBaro) {
    if (threadIdx.x == 0) {
      double h[9];
#pragma unroll
      for (int c = 0; c < 9; ++c) h[c] = a.cells[9 * (size_t)f + c];
      const double *W = a.virial + 9 * (size_t)f;
      const double V = md_cell_volume(h);
      double l2 = lambda * lambda;
      if constexpr (kNhc) l2 = s2 * s2;  // (sx, sy, sz already carry s1^2)
      double P[3] = {(l2 * sx - W[0]) / V, (l2 * sy - W[4]) / V, (l2 * sz - W[8]) / V};
      if (a.baro_iso) P[0] = P[1] = P[2] = (P[0] + P[1] + P[2]) / 3.0;
      double n2 = 0.0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        double m_c = 1.0;
        if (a.baro_iso || a.baro_mask[c]) {
          m_c = 1.0 - a.baro_k * (a.baro_p0 - P[c]);
          if (!(m_c > 0.0) || isinf(m_c)) m_c = nan("");  // (the host finds it in the cells)
        }
        const double s_c = a.baro_scale[3 * (size_t)f + c] * m_c;
        a.baro_scale[3 * (size_t)f + c] = s_c;
        s_baro[kBaroMu + c] = m_c;
        s_baro[kBaroScale + c] = s_c;
        n2 += (s_c - 1.0) * (s_c - 1.0);
#pragma unroll
        for (int r = 0; r < 3; ++r) a.cells[9 * (size_t)f + 3 * r + c] = h[3 * r + c] * m_c;
      }
      const double lim = 0.5 * (a.skin - a.r_list * sqrt(n2));
      s_baro[kBaroLim2] = lim > 0.0 ? lim * lim : -1.0;  // (a NaN strain: -1, every drift is stale)
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) mu[c] = s_baro[kBaroMu + c], sc[c] = s_baro[kBaroScale + c];
    lim2 = s_baro[kBaroLim2];
  }
  for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {  // (each thread meets its own atoms again)
    const double m = a.mass[i];
    double rp[3] = {0.0, 0.0, 0.0};  // (Langevin: the random part of the drift)
    if constexpr (kLangevin) {
      const double rsm = 1.0 / sqrt(m);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        double xi, eta;
        md_normals(a.seed, a.step, (uint32_t)i, (uint32_t)c, &xi, &eta);
        const double rv = a.c3 * rsm * xi - a.c4 * rsm * eta;
        rp[c] = a.c5 * rsm * eta;
        double v = a.vel[3 * i + c];
        v += a.c1 * a.forces[3 * i + c] / m - a.c2 * v + rv;
        a.vel[3 * i + c] = v;
      }
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if constexpr (kNhc && kSnap) a.snap_v[3 * i + c] = s1 * a.vel[3 * i + c];  // (after the closing half-update)
        double v = lambda * a.vel[3 * i + c];
        v += hdt * a.forces[3 * i + c] / m;
        a.vel[3 * i + c] = v;
      }
    }
    if constexpr (kBaro) {  // the scaled x_k drifts; u = x_{k+1} - x_ref o s
      double x = mu[0] * a.pos[3 * i] + a.dt * a.vel[3 * i], y = mu[1] * a.pos[3 * i + 1] + a.dt * a.vel[3 * i + 1],
             z = mu[2] * a.pos[3 * i + 2] + a.dt * a.vel[3 * i + 2];
      if constexpr (kLangevin) x += rp[0], y += rp[1], z += rp[2];
      a.pos[3 * i] = x;
      a.pos[3 * i + 1] = y;
      a.pos[3 * i + 2] = z;
      const double dx = x - a.ref[3 * i] * sc[0], dy = y - a.ref[3 * i + 1] * sc[1], dz = z - a.ref[3 * i + 2] * sc[2];
      const double d2 = dx * dx + dy * dy + dz * dz;
      stale |= !(d2 < lim2) ? 1 : 0;  // (a NaN fails the comparison too and is reported by the rebuild)
    } else {
      double x = a.pos[3 * i] + a.dt * a.vel[3 * i], y = a.pos[3 * i + 1] + a.dt * a.vel[3 * i + 1],
             z = a.pos[3 * i + 2] + a.dt * a.vel[3 * i + 2];
      if constexpr (kLangevin) x += rp[0], y += rp[1], z += rp[2];
      a.pos[3 * i] = x;
      a.pos[3 * i + 1] = y;
      a.pos[3 * i + 2] = z;
      const double dx = x - a.ref[3 * i], dy = y - a.ref[3 * i + 1], dz = z - a.ref[3 * i + 2];
      const double d2 = dx * dx + dy * dy + dz * dz;
      stale |= !(d2 <= a.lim2) ? 1 : 0;  // (a NaN fails the comparison too and is reported by the rebuild)
    }
  }
  if constexpr (kBaro) {
    if (threadIdx.x == 0 && !(lim2 > 0.0)) stale = 1;  // (a frame without atoms strains the list too)
  }
  if (__syncthreads_or(stale) && threadIdx.x == 0) {
    *static_cast<volatile unsigned *>(a.status) = a.seq + 1u;
    *static_cast<volatile unsigned *>(a.status_host) = a.seq + 1u;
  }
}

// the build of a launch that samples, or the one without a snapshot store in it
template <bool kLangevin, bool kBaro, bool kNhc>
void md_launch_build(const MdLaunch &a, dim3 grid, dim3 block, hipStream_t s) {
  if (a.snap_x)
    hipLaunchKernelGGL((md_integrate_kernel<kLangevin, kBaro, kNhc, true>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((md_integrate_kernel<kLangevin, kBaro, kNhc, false>), grid, block, 0, s, a);
}

}  // namespace

void launch_md_integrate(const MdLaunch &a, int threads, hipStream_t s) {
  if (a.n_blk <= 0) return;
  const dim3 grid((unsigned)a.n_blk), block((unsigned)threads);
  if (a.nhc) {  // (ta_md_run made every workgroup a whole frame; ta_md_set_nose_hoover excludes Langevin)
    if (a.baro)
      md_launch_build<false, true, true>(a, grid, block, s);
    else
      md_launch_build<false, false, true>(a, grid, block, s);
    return;
  }
  if (a.baro) {  // (ta_md_run made every workgroup a whole frame)
    if (a.langevin)
      md_launch_build<true, true, false>(a, grid, block, s);
    else
      md_launch_build<false, true, false>(a, grid, block, s);
    return;
  }
  if (a.langevin)
    md_launch_build<true, false, false>(a, grid, block, s);
  else
    md_launch_build<false, false, false>(a, grid, block, s);
}

void launch_md_noise(unsigned long long seed, long long step, long long n, double *xi, double *eta, hipStream_t s) {
  if (n <= 0) return;
  const long long n3 = 3 * n;
  hipLaunchKernelGGL(md_noise_kernel, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, s, seed, step, n3, xi, eta);
}

}  // namespace ta
