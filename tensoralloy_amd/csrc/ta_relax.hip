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
#include <hip/hip_runtime.h>

#include "ta_device.h"
#include "ta_math.h"
#include "ta_relax.h"

namespace ta {
namespace {

constexpr int kRelaxThreads = 256;

// frame of this workgroup: the last f with blk_start[f] <= blockIdx.x (every frame has at least one)
__device__ __forceinline__ int relax_frame_of_block(const int32_t *blk_start, int n_frames) {
  int lo = 0, hi = n_frames - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (blk_start[mid] <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(kRelaxThreads) void relax_reduce_kernel(RelaxLaunch a) {
  __shared__ double s_wave[4][kRelaxThreads / 64];
  const unsigned mark = *static_cast<volatile unsigned *>(a.status);
  if (mark != 0u && mark <= a.seq) return;
  const int f = relax_frame_of_block(a.blk_start, a.n_frames);
  if (a.state[(size_t)(a.seq & 1u) * a.n_frames + f].converged) return;  // (the step launch does not read its partial)
  const int64_t f_hi = a.atom_start[f + 1];
  const int64_t lo = a.atom_start[f] + (int64_t)((int)blockIdx.x - a.blk_start[f]) * a.chunk;
  const int64_t hi = lo + a.chunk < f_hi ? lo + a.chunk : f_hi;

  double vf = 0.0, ff = 0.0, vv = 0.0, m2 = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    if (a.fixed[i]) continue;
    const double fx = a.forces[3 * i], fy = a.forces[3 * i + 1], fz = a.forces[3 * i + 2];
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

__global__ __launch_bounds__(kRelaxThreads) void relax_step_kernel(RelaxLaunch a) {
  __shared__ double s_sum[4];
  // (0, or the value this very launch writes, or the mark of an earlier launch: the same branch in every thread)
  const unsigned mark = *static_cast<volatile unsigned *>(a.status);
  if (mark != 0u && mark <= a.seq) return;
  const int f = relax_frame_of_block(a.blk_start, a.n_frames);
  const int blk0 = a.blk_start[f], blk1 = a.blk_start[f + 1];
  const bool writer = (int)blockIdx.x == blk0 && threadIdx.x == 0;  // of the frame's record
  RelaxFrameState st = a.state[(size_t)(a.seq & 1u) * a.n_frames + f];
  RelaxFrameState *next = &a.state[(size_t)((a.seq + 1u) & 1u) * a.n_frames + f];
  if (st.converged) {
    if (writer) *next = st;
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
  hipLaunchKernelGGL(relax_reduce_kernel, dim3((unsigned)a.n_blk), dim3(kRelaxThreads), 0, s, a);
  hipLaunchKernelGGL(relax_step_kernel, dim3((unsigned)a.n_blk), dim3(kRelaxThreads), 0, s, a);
}

}  // namespace ta
