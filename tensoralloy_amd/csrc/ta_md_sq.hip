// Structure factors inside the device MD loop (ta_md_set_sq): the three launches ta_md_run puts behind an
// integrator launch that wrote the whole-step state (x, v) of a sampled step. With the caller's Q integer triples
// n (Miller indices), the cell h of frame f (rows are lattice vectors) and s_i = x_i h^-1, the wave vector
// q = 2 pi h^-1 n has q . x_i = 2 pi n . s_i, and per frame f, element a and q
//     rho_a(q) = sum_{i in a} exp(+i 2 pi n . s_i),    j_a(q) = sum_{i in a} v_i exp(+i 2 pi n . s_i)
// Sample number n goes to slot n % L of a ring of amplitude rows and is correlated with the rows of the lags
// k = 0 .. min(n, L - 1), per ordered pair of elements (a, b):
//     A_rho[f][a][b][k][q] += Re(rho_a(q; n) conj rho_b(q; n - k))
//     A_L  [f][a][b][k][q] += Re((qhat . j_a(q; n)) conj (qhat . j_b(q; n - k)))     qhat = q / |q|, 0 for n = 0
//     A_J  [f][a][b][k][q] += Re(j_a(q; n) . conj j_b(q; n - k))
//
// 1. md_sq_amplitude_kernel. A workgroup is ONE wave. It owns a chunk of consecutive atoms of one frame (the plan,
//    blk_start, is ta_md_set_sq's) and kMdSqTile = 64 q-vectors: a lane is a q-vector. The chunk passes through LDS
//    in slabs of kMdSqSlab atoms: lane t forms s_t = x_t h^-1 of one atom (h^-1 from db.cells, per workgroup) and
//    stores it with v_t and the species. Then every lane walks the slab's atoms, all lanes reading the same LDS
//    word (a broadcast), with the species of the atom as a scalar: the branch on it is wave-uniform. The phase is
//    t = n . s, t - rint(t) (exact) and sincospi(2 t): no large argument ever reaches the reduction of sincos.
//    The sums live in registers, element by element (the chunk is staged once per element; staging is one atom
//    per lane against 64 phases per lane); their order is the atom order. No cross-lane operation anywhere.
//    One partial per (chunk, element, plane, q) goes to HBM, q fastest: 512 contiguous bytes per store.
// 2. md_sq_sum_kernel. One thread per (f, a, plane, q) adds the frame's chunks in index order into the ring row.
// 3. md_sq_corr_kernel. One thread per (f, a, b, q), q fastest, loops over the valid lags: ring rows and
//    accumulators are read coalesced, every accumulator element has one owner: a plain read-add-write.
//
// No floating-point atomics: the values do not depend on how a run is cut into calls. All three launches carry the
// integrator's status-word predicate: behind a stale list they write nothing, and the loop enqueues them again
// after the rebuild, when the integrator launch in front has written the same snapshot again.
#include <hip/hip_runtime.h>

#include "ta_device.h"
#include "ta_md.h"
#include "ta_md_sweep.h"

namespace ta {
namespace {

static_assert(kMdSqTile == 64 && kMdSqSlab == kMdSqTile, "one wave: lane t stages atom t of the slab and owns q-vector t of the tile");

// g = h^-1 (row-major, as h): adjugate over determinant
__device__ __forceinline__ void sq_inverse(const double *h, double *g) {
  const double c00 = h[4] * h[8] - h[5] * h[7], c01 = h[5] * h[6] - h[3] * h[8], c02 = h[3] * h[7] - h[4] * h[6];
  const double inv = 1.0 / (h[0] * c00 + h[1] * c01 + h[2] * c02);
  g[0] = c00 * inv, g[1] = (h[2] * h[7] - h[1] * h[8]) * inv, g[2] = (h[1] * h[5] - h[2] * h[4]) * inv;
  g[3] = c01 * inv, g[4] = (h[0] * h[8] - h[2] * h[6]) * inv, g[5] = (h[2] * h[3] - h[0] * h[5]) * inv;
  g[6] = c02 * inv, g[7] = (h[1] * h[6] - h[0] * h[7]) * inv, g[8] = (h[0] * h[4] - h[1] * h[3]) * inv;
}

template <bool kCurrents>
__global__ __launch_bounds__(kMdSqTile) void md_sq_amplitude_kernel(MdSqLaunch a) {
  constexpr int kPlanes = kCurrents ? 8 : 2;
  __shared__ double s_s[kMdSqSlab][3];
  __shared__ double s_v[kCurrents ? kMdSqSlab : 1][3];
  __shared__ int s_sp[kMdSqSlab];
  if (md_stale(a.status, a.seq)) return;
  const int blk = (int)blockIdx.x, lane = (int)threadIdx.x;
  const int f = md_frame_of(a.blk_start, a.n_frames, blk);
  const long long i_end = a.atom_start[f + 1];
  const long long i_lo = (long long)a.atom_start[f] + (long long)(blk - a.blk_start[f]) * a.chunk;
  const long long i_hi = i_lo + a.chunk < i_end ? i_lo + a.chunk : i_end;
  double g[9];
  sq_inverse(a.cells + 9 * (size_t)f, g);
  const int Q = a.n_q, E = a.n_elements;
  const int q = (int)blockIdx.y * kMdSqTile + lane;
  const bool own = q < Q;
  const double n0 = own ? (double)a.miller[3 * q] : 0.0, n1 = own ? (double)a.miller[3 * q + 1] : 0.0;
  const double n2 = own ? (double)a.miller[3 * q + 2] : 0.0;
  for (int e = 0; e < E; ++e) {
    double acc[kPlanes];
#pragma unroll
    for (int c = 0; c < kPlanes; ++c) acc[c] = 0.0;
    for (long long base = i_lo; base < i_hi; base += kMdSqSlab) {
      __syncthreads();  // (the slab before has been read)
      const long long i = base + lane;
      if (i < i_hi) {
        const double x = a.x[3 * i], y = a.x[3 * i + 1], z = a.x[3 * i + 2];
        s_s[lane][0] = x * g[0] + y * g[3] + z * g[6];
        s_s[lane][1] = x * g[1] + y * g[4] + z * g[7];
        s_s[lane][2] = x * g[2] + y * g[5] + z * g[8];
        if constexpr (kCurrents) s_v[lane][0] = a.v[3 * i], s_v[lane][1] = a.v[3 * i + 1], s_v[lane][2] = a.v[3 * i + 2];
        s_sp[lane] = a.species[i];
      }
      __syncthreads();
      const int cnt = (int)(i_hi - base < (long long)kMdSqSlab ? i_hi - base : (long long)kMdSqSlab);
      for (int j = 0; j < cnt; ++j) {
        if (__builtin_amdgcn_readfirstlane(s_sp[j]) != e) continue;  // (the same word in every lane)
        double t = n0 * s_s[j][0] + n1 * s_s[j][1] + n2 * s_s[j][2];
        t -= rint(t);  // exact: |t| <= 1/2 from here on
        double sn, cs;
        sincospi(2.0 * t, &sn, &cs);
        acc[0] += cs;
        acc[1] += sn;
        if constexpr (kCurrents) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const double v = s_v[j][c];
            acc[2 + 2 * c] += v * cs;
            acc[3 + 2 * c] += v * sn;
          }
        }
      }
    }
    if (own) {
#pragma unroll
      for (int c = 0; c < kPlanes; ++c) a.part[(((size_t)blk * E + e) * kPlanes + c) * Q + q] = acc[c];
    }
  }
}

// ring row of sample n [f][e][plane][q] = the partials of the frame's chunks, in chunk order
__global__ __launch_bounds__(256) void md_sq_sum_kernel(MdSqLaunch a) {
  if (md_stale(a.status, a.seq)) return;
  const int Q = a.n_q, E = a.n_elements, P = a.currents ? 8 : 2;
  const size_t row = (size_t)a.n_frames * E * P * Q;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= row) return;
  const size_t per_blk = (size_t)E * P * Q;
  const int f = (int)(idx / per_blk);
  const size_t rest = idx % per_blk;  // (e, plane, q) as the partials have them
  double sum = 0.0;
  for (int b = a.blk_start[f]; b < a.blk_start[f + 1]; ++b) sum += a.part[(size_t)b * per_blk + rest];
  a.ring[(size_t)(a.n % a.n_lags) * row + idx] = sum;
}

template <bool kCurrents>
__global__ __launch_bounds__(256) void md_sq_corr_kernel(MdSqLaunch a) {
  constexpr int kPlanes = kCurrents ? 8 : 2;
  if (md_stale(a.status, a.seq)) return;
  const int Q = a.n_q, E = a.n_elements, L = a.n_lags;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)a.n_frames * E * E * Q) return;
  const int q = (int)(idx % Q), eb = (int)((idx / Q) % E), ea = (int)((idx / ((size_t)Q * E)) % E);
  const int f = (int)(idx / ((size_t)Q * E * E));
  const size_t row = (size_t)a.n_frames * E * kPlanes * Q;
  const size_t at_a = (((size_t)f * E + ea) * kPlanes) * Q + q, at_b = (((size_t)f * E + eb) * kPlanes) * Q + q;
  const double *newest = a.ring + (size_t)(a.n % L) * row + at_a;
  double u[kPlanes];
#pragma unroll
  for (int c = 0; c < kPlanes; ++c) u[c] = newest[(size_t)c * Q];
  double qh[3] = {0.0, 0.0, 0.0}, ul_re = 0.0, ul_im = 0.0;
  if constexpr (kCurrents) {
    // q = 2 pi h^-1 n; qhat = q / |q| (the factor drops out), (0, 0, 0) for n = 0
    double g[9];
    sq_inverse(a.cells + 9 * (size_t)f, g);
    const double n0 = (double)a.miller[3 * q], n1 = (double)a.miller[3 * q + 1], n2 = (double)a.miller[3 * q + 2];
    qh[0] = g[0] * n0 + g[1] * n1 + g[2] * n2;
    qh[1] = g[3] * n0 + g[4] * n1 + g[5] * n2;
    qh[2] = g[6] * n0 + g[7] * n1 + g[8] * n2;
    const double norm = sqrt(qh[0] * qh[0] + qh[1] * qh[1] + qh[2] * qh[2]);
    const double inv = norm > 0.0 ? 1.0 / norm : 0.0;
    qh[0] *= inv, qh[1] *= inv, qh[2] *= inv;
    ul_re = qh[0] * u[2] + qh[1] * u[4] + qh[2] * u[6];
    ul_im = qh[0] * u[3] + qh[1] * u[5] + qh[2] * u[7];
  }
  const long long kmax = a.n < (long long)(L - 1) ? a.n : (long long)(L - 1);
  const size_t acc0 = (((size_t)f * E + ea) * E + eb) * L;
  for (long long k = 0; k <= kmax; ++k) {
    const double *old = a.ring + (size_t)((a.n - k) % L) * row + at_b;
    double w[kPlanes];
#pragma unroll
    for (int c = 0; c < kPlanes; ++c) w[c] = old[(size_t)c * Q];
    const size_t at = (acc0 + (size_t)k) * Q + q;
    a.acc_rho[at] += u[0] * w[0] + u[1] * w[1];
    if constexpr (kCurrents) {
      const double wl_re = qh[0] * w[2] + qh[1] * w[4] + qh[2] * w[6];
      const double wl_im = qh[0] * w[3] + qh[1] * w[5] + qh[2] * w[7];
      a.acc_l[at] += ul_re * wl_re + ul_im * wl_im;
      a.acc_j[at] += (u[2] * w[2] + u[3] * w[3]) + (u[4] * w[4] + u[5] * w[5]) + (u[6] * w[6] + u[7] * w[7]);
    }
  }
}

}  // namespace

void launch_md_sq(const MdSqLaunch &a, hipStream_t s) {
  if (a.n_blk <= 0 || a.n_q <= 0 || a.n_lags <= 0 || a.n < 0) return;
  const dim3 grid((unsigned)a.n_blk, (unsigned)((a.n_q + kMdSqTile - 1) / kMdSqTile));
  const size_t row = (size_t)a.n_frames * a.n_elements * (a.currents ? 8 : 2) * a.n_q;
  const size_t n_corr = (size_t)a.n_frames * a.n_elements * a.n_elements * a.n_q;
  if (a.currents)
    hipLaunchKernelGGL(md_sq_amplitude_kernel<true>, grid, dim3(kMdSqTile), 0, s, a);
  else
    hipLaunchKernelGGL(md_sq_amplitude_kernel<false>, grid, dim3(kMdSqTile), 0, s, a);
  hipLaunchKernelGGL(md_sq_sum_kernel, dim3((unsigned)((row + 255) / 256)), dim3(256), 0, s, a);
  if (a.currents)
    hipLaunchKernelGGL(md_sq_corr_kernel<true>, dim3((unsigned)((n_corr + 255) / 256)), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(md_sq_corr_kernel<false>, dim3((unsigned)((n_corr + 255) / 256)), dim3(256), 0, s, a);
}

}  // namespace ta
