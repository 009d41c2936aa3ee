// Heat current and pressure tensor inside the device MD loop (ta_md_set_flux): the three launches ta_md_run puts
// behind an integrator launch that wrote the velocities v(t) of a sampled whole-step state. The evaluation of x(t)
// that ran in front of that launch left, per directed pair p = (c -> n) of its list, the pair vector
// D_p = x_n + S h - x_c (pair_geom) and g_p = d e_c / d D_p (db.g), and per atom e_i (db.eatom); nothing rewrites
// them before the next evaluation, which is enqueued behind these launches. Per frame
//     J_conv = sum_i (1/2 m_i |v_i|^2 + e_i) v_i          J_pot = - sum_p D_p (g_p . v_n(p))
//     K_ab   = sum_i m_i v_ia v_ib                        W_ab  = 1/2 sum_p (g_pa D_pb + g_pb D_pa)
// and a sample's row is {J_conv[3], J_pot[3], K[6], W[6]} with the six components in the order xx yy zz yz xz xy.
//
// 1. md_flux_sweep_kernel. Laid out like force_gather_kernel: kMdFluxLanes = 16 lanes per centre, 16 centres per
//    pass of a 256-lane workgroup. A workgroup owns `chunk` consecutive atoms of one frame (the plan, blk_start, is
//    ta_md_set_flux's) and takes DeviceBatch as the force gather does, so it walks exactly the list that evaluation
//    walked: pair_start / pair_stop_of, the filtered list included. Per pair it streams the record and g (32 bytes
//    each) and gathers v_n (24 bytes); the reverse index is not read. Lane 0 of a centre adds the per-atom terms.
//    Every lane keeps 18 sums; the wavefront's sum (DPP rows, then two shuffles) and the four wavefronts in index
//    order give the workgroup's partial.
// 2. md_flux_sum_kernel. One workgroup per frame stages the frame's partials through LDS; lane c < 18 adds component c
//    in workgroup order into the ring row of sample n (slot n % n_lags) and onto `sums`.
// 3. md_flux_corr_kernel. One thread per (f, lag, component) multiplies the row against the row of that lag,
//    J = J_conv + J_pot and Pi = K - W: every accumulator element has one owner, a plain read-add-write.
//
// No floating-point atomics: every sum runs in an order that the list and the plan fix, so the values do not depend
// on how a run is cut into calls. All three launches carry the integrator's status-word predicate: behind a stale
// list they write nothing, and the loop enqueues them again after the rebuild.
#include <hip/hip_runtime.h>

#include "ta_device.h"
#include "ta_md.h"
#include "ta_md_sweep.h"
#include "ta_reduce.h"

namespace ta {
namespace {

static_assert(kMdFluxLanes == 16 && kMdFluxRow == 18, "a centre is one DPP row; a row is {J_conv, J_pot, K, W}");

__global__ __launch_bounds__(16 * kMdFluxLanes) void md_flux_sweep_kernel(MdFluxLaunch a, DeviceBatch b) {
  __shared__ double s_part[16 * kMdFluxLanes / 64][kMdFluxRow];
  if (md_stale(a.status, a.seq)) return;
  const int blk = (int)blockIdx.x;
  const int grp = (int)threadIdx.x / kMdFluxLanes, lane = (int)threadIdx.x & (kMdFluxLanes - 1);
  const int f = md_frame_of(a.blk_start, a.n_frames, blk);
  const long long i_end = b.atom_start[f + 1];
  const long long i_lo = (long long)b.atom_start[f] + (long long)(blk - a.blk_start[f]) * a.chunk;
  const long long i_hi = i_lo + a.chunk < i_end ? i_lo + a.chunk : i_end;
  double acc[kMdFluxRow];
#pragma unroll
  for (int c = 0; c < kMdFluxRow; ++c) acc[c] = 0.0;
  for (long long base = i_lo; base < i_hi; base += 16) {
    const long long i = base + grp;
    if (i >= i_hi) continue;
    const int q0 = b.pair_start[i], q1 = pair_stop_of(b, i);
    for (int q = q0 + lane; q < q1; q += kMdFluxLanes) {
      const double2 *rec = pair_geom(b, (size_t)q);
      const double2 *gp = reinterpret_cast<const double2 *>(b.g + 4 * (size_t)q);
      const double2 d0 = rec[0], d1 = rec[1], g0 = gp[0], g1 = gp[1];
      const double *vn = a.v + 3 * (size_t)b.pair_j[q];
      const double dx = d0.x, dy = d0.y, dz = d1.x, gx = g0.x, gy = g0.y, gz = g1.x;
      const double gv = gx * vn[0] + gy * vn[1] + gz * vn[2];
      acc[3] -= dx * gv;
      acc[4] -= dy * gv;
      acc[5] -= dz * gv;
      acc[12] += gx * dx;
      acc[13] += gy * dy;
      acc[14] += gz * dz;
      acc[15] += 0.5 * (gy * dz + gz * dy);
      acc[16] += 0.5 * (gx * dz + gz * dx);
      acc[17] += 0.5 * (gx * dy + gy * dx);
    }
    if (lane == 0) {
      const double m = a.mass[i], vx = a.v[3 * i], vy = a.v[3 * i + 1], vz = a.v[3 * i + 2];
      const double e = 0.5 * m * (vx * vx + vy * vy + vz * vz) + b.eatom[i];
      acc[0] += e * vx;
      acc[1] += e * vy;
      acc[2] += e * vz;
      acc[6] += m * vx * vx;
      acc[7] += m * vy * vy;
      acc[8] += m * vz * vz;
      acc[9] += m * vy * vz;
      acc[10] += m * vx * vz;
      acc[11] += m * vx * vy;
    }
  }
  const int wave = (int)threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < kMdFluxRow; ++c) {
    const double v = wave_sum(acc[c]);
    if ((threadIdx.x & 63) == 0) s_part[wave][c] = v;
  }
  __syncthreads();
  if (threadIdx.x < kMdFluxRow) {
    double v = 0.0;
    for (int w = 0; w < 16 * kMdFluxLanes / 64; ++w) v += s_part[w][threadIdx.x];
    a.part[(size_t)blk * kMdFluxRow + threadIdx.x] = v;
  }
}

// ring row of sample n [f][18] = the partials of the frame's workgroups, in index order; the row also goes onto sums.
// One workgroup per frame: the partials pass through LDS in tiles of kMdFluxSumTile (all lanes load, coalesced), and
// lane c < 18 adds component c of the tile's partials one after another: a chain of dependent global loads (250 of
// them for a 4000-atom frame) cost 75 us a sample, more than the pair sweep.
constexpr int kMdFluxSumTile = 128;

__global__ __launch_bounds__(256) void md_flux_sum_kernel(MdFluxLaunch a) {
  __shared__ double s_tile[kMdFluxSumTile * kMdFluxRow];
  if (md_stale(a.status, a.seq)) return;  // (the same word in every lane: the barriers below are uniform)
  const int f = (int)blockIdx.x, c = (int)threadIdx.x;
  const int b0 = a.blk_start[f], b1 = a.blk_start[f + 1];
  double sum = 0.0;
  for (int base = b0; base < b1; base += kMdFluxSumTile) {
    const int n = b1 - base < kMdFluxSumTile ? b1 - base : kMdFluxSumTile;
    __syncthreads();  // (the tile before has been read)
    for (int i = (int)threadIdx.x; i < n * kMdFluxRow; i += (int)blockDim.x) s_tile[i] = a.part[(size_t)base * kMdFluxRow + i];
    __syncthreads();
    if (c < kMdFluxRow)
      for (int k = 0; k < n; ++k) sum += s_tile[k * kMdFluxRow + c];
  }
  if (c < kMdFluxRow) {
    const size_t row = (size_t)a.n_frames * kMdFluxRow, idx = (size_t)f * kMdFluxRow + c;
    a.ring[(size_t)(a.n % a.n_lags) * row + idx] = sum;
    a.sums[idx] += sum;
  }
}

__global__ __launch_bounds__(256) void md_flux_corr_kernel(MdFluxLaunch a) {
  if (md_stale(a.status, a.seq)) return;
  const int L = a.n_lags;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)a.n_frames * L * 9) return;
  const int c = (int)(idx % 9), f = (int)(idx / ((size_t)9 * L));
  const long long k = (long long)((idx / 9) % L);
  if (k > a.n) return;  // (the lags held: 0 .. min(n, L - 1))
  const size_t row = (size_t)a.n_frames * kMdFluxRow;
  const double *u = a.ring + (size_t)(a.n % L) * row + (size_t)f * kMdFluxRow;
  const double *w = a.ring + (size_t)((a.n - k) % L) * row + (size_t)f * kMdFluxRow;
  if (c < 3)
    a.acc_heat[((size_t)f * L + (size_t)k) * 3 + c] += (u[c] + u[3 + c]) * (w[c] + w[3 + c]);
  else
    a.acc_press[((size_t)f * L + (size_t)k) * 6 + (c - 3)] += (u[3 + c] - u[9 + c]) * (w[3 + c] - w[9 + c]);
}

}  // namespace

void launch_md_flux(const MdFluxLaunch &a, const DeviceBatch &b, hipStream_t s) {
  if (a.n_blk <= 0 || a.n_lags <= 0 || a.n < 0 || a.n_frames <= 0) return;
  const size_t n_corr = (size_t)a.n_frames * a.n_lags * 9;
  hipLaunchKernelGGL(md_flux_sweep_kernel, dim3((unsigned)a.n_blk), dim3(16 * kMdFluxLanes), 0, s, a, b);
  hipLaunchKernelGGL(md_flux_sum_kernel, dim3((unsigned)a.n_frames), dim3(256), 0, s, a);
  hipLaunchKernelGGL(md_flux_corr_kernel, dim3((unsigned)((n_corr + 255) / 256)), dim3(256), 0, s, a);
}

}  // namespace ta
