// Device-resident structure relaxation (ta_relax_run): the two launches that sit between two force evaluations.
//
// FIRE (Bitzek et al., PRL 97, 170201) as ASE's FIRE with downhill_check = False, per frame, with F the
// forces at the current positions and all sums over the 3n components of the frame:
//     if max_i |F_i|^2 < fmax^2: the frame is converged and does not move again in this run
//     if first: v = 0
//     else if F.v > 0:  v = (1 - a) v + a F |v| / |F|;  if npos > nmin: dt = min(dt finc, dtmax), a = a fa;  npos += 1
//     else:             v = 0;  a = astart;  dt = dt fdec;  npos = 0
//     v += dt F;  dr = dt v;  if |dr| > maxstep: dr = dr maxstep / |dr|;  x += dr
//
// A frame is cut into workgroups of `chunk` consecutive atoms, as in the MD launch without a thermostat.
//   launch 1 (relax_reduce_kernel): every workgroup leaves ONE partial (F.v, F.F, v.v, max |F_i|^2) of its
//     atoms: threads in a fixed order, waves one after another, no floating-point atomics.
//   launch 2 (relax_step_kernel): every workgroup adds the partials of its frame in one fixed order (its
//     first wave: lane l takes partials l, l + 64, ..., then the lanes as in wave_sum), so all workgroups of
//     a frame hold bitwise the same four numbers and take the same branch; then the velocity
//     update, the drift and the skin test of ta_update_positions. |dr| comes from the three sums:
//     v_new = alpha v + beta F gives |v_new|^2 = alpha^2 v.v + 2 alpha beta F.v + beta^2 F.F, in which no term
//     is negative (alpha = 0 unless F.v > 0), so nothing cancels.
// The FIRE state of a frame is kept twice: launch k reads copy k & 1, and the frame's first workgroup writes
// copy (k + 1) & 1, so no workgroup reads what another one writes. A converged frame's workgroups write no
// position and no velocity; its first workgroup only carries the frozen record over to the other copy.
// When the last frame converges its workgroup writes 1 + seq into a page-locked word (the count of converged
// frames is an integer atomic).
//
// Both launches are predicated on the status word of the MD loop: a drift that finds an atom beyond skin / 2
// writes its own sequence number + 1 there, still writes valid positions, and every LATER launch returns at
// once. Atoms of the `fixed` mask have their force read as 0 everywhere and are never written.
//
// Cell mode (ta_relax_set_cell; the kCell builds of both launches): ASE's UnitCellFilter. With h0 the cell
// at ta_relax_set_cell, G a deformation gradient (h = h0 G^T, x_i = q_i G^T), cf the cell factor, p the
// external pressure and M the mask, the n + 3 rows [q_1 .. q_n ; cf G] are relaxed under the forces
//     f_i = F_i G,    f_cell = -((W + p V I) G^-T) o M / cf    (hydrostatic: I trace / 3 before the mask)
// with W the frame virial of the last evaluation and V = |det h|. The reduce launch sums f_i = F_i G over the
// atoms. In the step launch thread 0 of EVERY workgroup of the frame adds the three cell rows to the frame's
// sums (the same arithmetic on the same inputs: bitwise the same branch everywhere), and after the branch
// computes G' = G + dr_cell / cf, h' = h0 G'^T and A = h_ref^-1 h'; the atoms then move as q = x G^-T,
// q += dr, x = q G'^T (fixed atoms keep q: they move with the cell). G and the cell velocity are kept twice
// like the FIRE state; the frame's first workgroup alone writes the other copy and the new row of db.cells,
// which no workgroup of the step launch reads. The list test knows strain: with u_i = x_i - x_ref,i A the
// list is stale when lim = (skin - (rc + skin) |A - I|_F) / 2 <= 0 or some |u_i|^2 >= lim^2 (every pair
// vector obeys D_new = D_ref A + u_j - u_i and sigma_min(A) >= 1 - |A - I|_F).
#include <hip/hip_runtime.h>

#include "ta_device.h"
#include "ta_math.h"
#include "ta_md_sweep.h"
#include "ta_relax.h"

namespace ta {
namespace {

constexpr int kRelaxThreads = 256;

// o = m^-1 (row-major 3x3); returns det m
__device__ __forceinline__ double relax_inv3(const double *m, double *o) {
  const double c0 = m[4] * m[8] - m[5] * m[7], c1 = m[5] * m[6] - m[3] * m[8], c2 = m[3] * m[7] - m[4] * m[6];
  const double det = m[0] * c0 + m[1] * c1 + m[2] * c2;
  const double id = 1.0 / det;
  o[0] = c0 * id, o[1] = (m[2] * m[7] - m[1] * m[8]) * id, o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
  o[3] = c1 * id, o[4] = (m[0] * m[8] - m[2] * m[6]) * id, o[5] = (m[2] * m[3] - m[0] * m[5]) * id;
  o[6] = c2 * id, o[7] = (m[1] * m[6] - m[0] * m[7]) * id, o[8] = (m[0] * m[4] - m[1] * m[3]) * id;
  return det;
}

// h = h0 G^T (rows are lattice vectors)
__device__ __forceinline__ void relax_cell_of(const double *h0, const double *G, double *h) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) h[3 * r + c] = h0[3 * r] * G[3 * c] + h0[3 * r + 1] * G[3 * c + 1] + h0[3 * r + 2] * G[3 * c + 2];
}

// slots of the step launch's LDS block in cell mode
constexpr int kCellG = 0, kCellGinv = 9, kCellGnew = 18, kCellA = 27, kCellLim2 = 36, kCellWords = 37;

template <bool kCell>
__global__ __launch_bounds__(kRelaxThreads) void relax_reduce_kernel(RelaxLaunch a) {
  __shared__ double s_wave[4][kRelaxThreads / 64];
  if (md_stale(a.status, a.seq)) return;
  const int f = md_frame_of(a.blk_start, a.n_frames, (int)blockIdx.x);
  if (a.state[(size_t)(a.seq & 1u) * a.n_frames + f].converged) return;  // (the step launch does not read its partial)
  const int64_t f_hi = a.atom_start[f + 1];
  const int64_t lo = a.atom_start[f] + (int64_t)((int)blockIdx.x - a.blk_start[f]) * a.chunk;
  const int64_t hi = lo + a.chunk < f_hi ? lo + a.chunk : f_hi;

  double G[9];
  if constexpr (kCell) {
    const double *g = a.cell_G + 9 * ((size_t)(a.seq & 1u) * a.n_frames + f);
#pragma unroll
    for (int c = 0; c < 9; ++c) G[c] = g[c];
  }
  double vf = 0.0, ff = 0.0, vv = 0.0, m2 = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    if (a.fixed[i]) continue;
    double fx = a.forces[3 * i], fy = a.forces[3 * i + 1], fz = a.forces[3 * i + 2];
    if constexpr (kCell) {  // f_i = F_i G
      const double Fx = fx, Fy = fy, Fz = fz;
      fx = Fx * G[0] + Fy * G[3] + Fz * G[6];
      fy = Fx * G[1] + Fy * G[4] + Fz * G[7];
      fz = Fx * G[2] + Fy * G[5] + Fz * G[8];
    }
    const double vx = a.vel[3 * i], vy = a.vel[3 * i + 1], vz = a.vel[3 * i + 2];
    const double f2 = fx * fx + fy * fy + fz * fz;
    vf += fx * vx + fy * vy + fz * vz;
    ff += f2;
    vv += vx * vx + vy * vy + vz * vz;
    m2 = !(f2 <= m2) ? f2 : m2;  // (a NaN stays: the frame then never counts as converged)
  }
  vf = wave_sum(vf);
  ff = wave_sum(ff);
  vv = wave_sum(vv);
  // fmax drops a NaN: it is carried by F.F, which the step launch looks at
  m2 = wave_max(m2);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_wave[0][wave] = vf;
    s_wave[1][wave] = ff;
    s_wave[2][wave] = vv;
    s_wave[3][wave] = m2;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    double t = s_wave[threadIdx.x][0];
    for (int w = 1; w < kRelaxThreads / 64; ++w)
      t = threadIdx.x == 3 ? fmax(t, s_wave[3][w]) : t + s_wave[threadIdx.x][w];
    a.part[4 * (size_t)blockIdx.x + threadIdx.x] = t;
  }
}

template <bool kCell>
__global__ __launch_bounds__(kRelaxThreads) void relax_step_kernel(RelaxLaunch a) {
  __shared__ double s_sum[4];
  __shared__ double s_cell[kCell ? kCellWords : 1];  // (unused, and dropped, in the fixed-cell build)
  // (0, or the value this very launch writes, or the mark of an earlier launch: the same branch in every thread)
  if (md_stale(a.status, a.seq)) return;
  const int f = md_frame_of(a.blk_start, a.n_frames, (int)blockIdx.x);
  const int blk0 = a.blk_start[f], blk1 = a.blk_start[f + 1];
  const bool writer = (int)blockIdx.x == blk0 && threadIdx.x == 0;  // of the frame's record
  RelaxFrameState st = a.state[(size_t)(a.seq & 1u) * a.n_frames + f];
  RelaxFrameState *next = &a.state[(size_t)((a.seq + 1u) & 1u) * a.n_frames + f];
  // cell mode: thread 0 of every workgroup of the frame holds the same G, cell velocity and cell force
  double G[9], vc[9], fc[9], h0[9], cf = 1.0;
  double *G_next = nullptr, *vc_next = nullptr;
  if constexpr (kCell) {
    if (threadIdx.x == 0) {
      const size_t cur = 9 * ((size_t)(a.seq & 1u) * a.n_frames + f);
      const size_t nxt = 9 * ((size_t)((a.seq + 1u) & 1u) * a.n_frames + f);
#pragma unroll
      for (int c = 0; c < 9; ++c) G[c] = a.cell_G[cur + c], vc[c] = a.cell_vel[cur + c];
      G_next = a.cell_G + nxt;
      vc_next = a.cell_vel + nxt;
    }
  }
  if (st.converged) {
    if (writer) {
      *next = st;
      if constexpr (kCell) {
#pragma unroll
        for (int c = 0; c < 9; ++c) G_next[c] = G[c], vc_next[c] = vc[c];
      }
    }
    return;
  }
  if (threadIdx.x < 64) {
    // the first wave: lane l adds partials l, l + 64, ... of the frame, then the lanes are added as in
    // wave_sum; the order depends on the frame's layout alone, so it is the same in every workgroup
    double vf = 0.0, ff = 0.0, vv = 0.0, m2 = 0.0;
    for (int b = blk0 + (int)threadIdx.x; b < blk1; b += 64) {
      const double *p = a.part + 4 * (size_t)b;
      vf += p[0];
      ff += p[1];
      vv += p[2];
      m2 = fmax(m2, p[3]);
    }
    vf = wave_sum(vf);
    ff = wave_sum(ff);
    vv = wave_sum(vv);
    m2 = wave_max(m2);
    if constexpr (kCell) {
      if (threadIdx.x == 0) {
        // the three cell rows: f_cell = -((W + p V I) G^-T) o M / cf, from the virial of the last evaluation
        double Gi[9], h[9], W[9];
        relax_inv3(G, Gi);
        cf = a.cell_cf[f];
#pragma unroll
        for (int c = 0; c < 9; ++c) h0[c] = a.cell_h0[9 * (size_t)f + c], W[c] = a.virial[9 * (size_t)f + c];
        relax_cell_of(h0, G, h);
        const double pV = a.pressure * fabs(h[0] * (h[4] * h[8] - h[5] * h[7]) - h[1] * (h[3] * h[8] - h[5] * h[6]) +
                                            h[2] * (h[3] * h[7] - h[4] * h[6]));
        W[0] += pV, W[4] += pV, W[8] += pV;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c)
            fc[3 * r + c] = -(W[3 * r] * Gi[3 * c] + W[3 * r + 1] * Gi[3 * c + 1] + W[3 * r + 2] * Gi[3 * c + 2]);
        if (a.hydrostatic) {
          const double t = (fc[0] + fc[4] + fc[8]) / 3.0;
#pragma unroll
          for (int c = 0; c < 9; ++c) fc[c] = (c == 0 || c == 4 || c == 8) ? t : 0.0;
        }
        double c2 = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          double row = 0.0;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const double v = fc[3 * r + c] * a.cell_mask[3 * r + c] / cf;
            fc[3 * r + c] = v;
            vf += v * vc[3 * r + c];
            vv += vc[3 * r + c] * vc[3 * r + c];
            row += v * v;
          }
          ff += row;
          m2 = fmax(m2, row);
          c2 = fmax(c2, row);
        }
        if (writer) a.cell_fmax2[f] = c2;
#pragma unroll
        for (int c = 0; c < 9; ++c) s_cell[kCellG + c] = G[c], s_cell[kCellGinv + c] = Gi[c];
      }
    }
    if (threadIdx.x == 0) s_sum[0] = vf, s_sum[1] = ff, s_sum[2] = vv, s_sum[3] = m2;
  }
  __syncthreads();
  double vf = s_sum[0], vv = s_sum[2];
  const double ff = s_sum[1], m2 = s_sum[3];
  // (a NaN among the forces makes F.F a NaN: not converged, and the NaN positions fail the skin test)
  const bool converged = ff == ff && m2 < a.fmax2;
  if (converged || !a.drift) {
    if (writer) {
      st.converged = converged ? 1 : 0;
      st.fmax2 = ff == ff ? m2 : ff;
      *next = st;
      if constexpr (kCell) {
#pragma unroll
        for (int c = 0; c < 9; ++c) G_next[c] = G[c], vc_next[c] = vc[c];
      }
      if (converged && atomicAdd(a.n_converged, 1) == a.n_frames - 1)
        *static_cast<volatile unsigned *>(a.status_host + 1) = a.seq + 1u;
    }
    return;
  }

  double alpha = 0.0, beta = 0.0;  // v <- alpha v + beta F, the kick included
  if (st.first) {
    vf = vv = 0.0;
  } else if (vf > 0.0) {
    alpha = 1.0 - st.a;
    beta = st.a * sqrt(vv) / sqrt(ff);
    if (st.npos > a.nmin) {
      st.dt = fmin(st.dt * a.finc, a.dtmax);
      st.a *= a.fa;
    }
    st.npos += 1;
  } else {
    st.a = a.astart;
    st.dt *= a.fdec;
    st.npos = 0;
  }
  beta += st.dt;
  const double dt = st.dt;
  const double dr = dt * sqrt(alpha * alpha * vv + 2.0 * alpha * beta * vf + beta * beta * ff);
  const bool clamp = dr > a.maxstep;
  if (writer) {
    st.first = 0;
    st.steps += 1;
    st.fmax2 = m2;
    *next = st;
  }

  const int64_t f_hi = a.atom_start[f + 1];
  const int64_t lo = a.atom_start[f] + (int64_t)((int)blockIdx.x - blk0) * a.chunk;
  const int64_t hi = lo + a.chunk < f_hi ? lo + a.chunk : f_hi;
  int stale = 0;
  if constexpr (kCell) {
    if (threadIdx.x == 0) {
      // G' = G + dr_cell / cf, h' = h0 G'^T, A = h_ref^-1 h' and the list's limit under this strain
      double Gn[9], hn[9], hr[9], hri[9];
#pragma unroll
      for (int c = 0; c < 9; ++c) {
        const double v = alpha * vc[c] + beta * fc[c];
        double d = dt * v;
        if (clamp) d = d * a.maxstep / dr;
        vc[c] = v;
        Gn[c] = G[c] + d / cf;
        hr[c] = a.ref_cells[9 * (size_t)f + c];
      }
      relax_cell_of(h0, Gn, hn);
      relax_inv3(hr, hri);
      double n2 = 0.0;
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double v = hri[3 * r] * hn[c] + hri[3 * r + 1] * hn[3 + c] + hri[3 * r + 2] * hn[6 + c];
          s_cell[kCellA + 3 * r + c] = v;
          const double e = v - (r == c ? 1.0 : 0.0);
          n2 += e * e;
        }
      const double lim = 0.5 * (a.skin - a.r_list * sqrt(n2));
      s_cell[kCellLim2] = lim > 0.0 ? lim * lim : -1.0;  // (a NaN strain: -1, every drift is stale)
#pragma unroll
      for (int c = 0; c < 9; ++c) s_cell[kCellGnew + c] = Gn[c];
      if (writer) {
#pragma unroll
        for (int c = 0; c < 9; ++c) G_next[c] = Gn[c], vc_next[c] = vc[c], a.cells[9 * (size_t)f + c] = hn[c];
      }
    }
    __syncthreads();
    double Gi[9], Gn[9], A[9];
#pragma unroll
    for (int c = 0; c < 9; ++c)
      G[c] = s_cell[kCellG + c], Gi[c] = s_cell[kCellGinv + c], Gn[c] = s_cell[kCellGnew + c], A[c] = s_cell[kCellA + c];
    const double lim2 = s_cell[kCellLim2];
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
      const double x[3] = {a.pos[3 * i], a.pos[3 * i + 1], a.pos[3 * i + 2]};
      double q[3];  // q = x G^-T
#pragma unroll
      for (int c = 0; c < 3; ++c) q[c] = Gi[3 * c] * x[0] + Gi[3 * c + 1] * x[1] + Gi[3 * c + 2] * x[2];
      if (!a.fixed[i]) {
        const double F[3] = {a.forces[3 * i], a.forces[3 * i + 1], a.forces[3 * i + 2]};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double v = alpha * a.vel[3 * i + c] + beta * (F[0] * G[c] + F[1] * G[3 + c] + F[2] * G[6 + c]);
          a.vel[3 * i + c] = v;
          double d = dt * v;
          if (clamp) d = d * a.maxstep / dr;
          q[c] += d;
        }
      }
      double d2 = 0.0;  // x' = q G'^T (a fixed atom too: it moves with the cell), u = x' - x_ref A
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double xn = Gn[3 * c] * q[0] + Gn[3 * c + 1] * q[1] + Gn[3 * c + 2] * q[2];
        a.pos[3 * i + c] = xn;
        const double u = xn - (a.ref[3 * i] * A[c] + a.ref[3 * i + 1] * A[3 + c] + a.ref[3 * i + 2] * A[6 + c]);
        d2 += u * u;
      }
      stale |= !(d2 < lim2) ? 1 : 0;  // (a NaN fails the comparison too and is reported by the rebuild)
    }
    if (threadIdx.x == 0 && !(lim2 > 0.0)) stale = 1;  // (a frame without atoms in this workgroup strains the list too)
    if (__syncthreads_or(stale) && threadIdx.x == 0) {
      *static_cast<volatile unsigned *>(a.status) = a.seq + 1u;
      *static_cast<volatile unsigned *>(a.status_host) = a.seq + 1u;
    }
    return;
  }
  for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    double x[3] = {a.pos[3 * i], a.pos[3 * i + 1], a.pos[3 * i + 2]};
    if (!a.fixed[i]) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double v = alpha * a.vel[3 * i + c] + beta * a.forces[3 * i + c];
        a.vel[3 * i + c] = v;
        double d = dt * v;
        if (clamp) d = d * a.maxstep / dr;
        x[c] += d;
        a.pos[3 * i + c] = x[c];
      }
    }
    const double dx = x[0] - a.ref[3 * i], dy = x[1] - a.ref[3 * i + 1], dz = x[2] - a.ref[3 * i + 2];
    const double d2 = dx * dx + dy * dy + dz * dz;
    stale |= !(d2 <= a.lim2) ? 1 : 0;  // (a NaN fails the comparison too and is reported by the rebuild)
  }
  if (__syncthreads_or(stale) && threadIdx.x == 0) {
    *static_cast<volatile unsigned *>(a.status) = a.seq + 1u;
    *static_cast<volatile unsigned *>(a.status_host) = a.seq + 1u;
  }
}

}  // namespace

void launch_relax_step(const RelaxLaunch &a, hipStream_t s) {
  if (a.n_blk <= 0) return;
  if (a.cell) {
    hipLaunchKernelGGL(relax_reduce_kernel<true>, dim3((unsigned)a.n_blk), dim3(kRelaxThreads), 0, s, a);
    hipLaunchKernelGGL(relax_step_kernel<true>, dim3((unsigned)a.n_blk), dim3(kRelaxThreads), 0, s, a);
    return;
  }
  hipLaunchKernelGGL(relax_reduce_kernel<false>, dim3((unsigned)a.n_blk), dim3(kRelaxThreads), 0, s, a);
  hipLaunchKernelGGL(relax_step_kernel<false>, dim3((unsigned)a.n_blk), dim3(kRelaxThreads), 0, s, a);
}

}  // namespace ta
