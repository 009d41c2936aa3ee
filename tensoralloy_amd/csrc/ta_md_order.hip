// Bond-orientational order inside the device MD loop (ta_md_set_order): the two launches ta_md_run puts IN FRONT OF
// the integrator launch of a sampled step, while the device still holds the whole-step state x(t). For every
// centre i (species a) the neighbours are the entries (j, S) of the resident (skin) list with
//     d = x_j - x_i + S . h (fp64),   d . d < rb[a][b]^2,   b = species of j
// (md_entry of ta_md_sweep.h, then this test), N_b(i) of them. For every chosen degree l and m = 0 .. l
//     q_lm(i)    = (1 / N_b) sum_neigh Y_lm(d / |d|)                                   (pass 1)
//     qbar_lm(i) = (q_lm(i) + sum_neigh q_lm(j)) / (N_b + 1)                            (pass 2)
//     q_l        = sqrt(4 pi / (2 l + 1) (|q_l0|^2 + 2 sum_{m > 0} |q_lm|^2)),  qbar_l likewise from qbar_lm
//     s_ij       = Re sum_{m = -l .. l} q_lm(i) conj(q_lm(j)) / (|q_l(i)| |q_l(j)|)     for l = solid_degree
//     n_conn(i)  = number of neighbours with s_ij > c
// Negative m never appear: Y_{l, -m} = (-1)^m conj(Y_lm), so they double the terms m > 0 of every sum above.
//
// Y_lm without trigonometry: with t = z / r and e = (x + i y) / r
//     Y_lm = N_lm Q_l^m(t) e^m,   Q_l^m(t) = P_l^m(t) / (1 - t^2)^(m / 2)   (a polynomial in t: no pole at t = +-1)
//     Q_m^m = (-1)^m (2 m - 1)!!,  Q_{m+1}^m = (2 m + 1) t Q_m^m,
//     Q_l^m = ((2 l - 1) t Q_{l-1}^m - (l + m - 1) Q_{l-2}^m) / (l - m)
// (Condon-Shortley phase, as scipy.special.sph_harm). The N_lm come from the host in fp64.
//
// A workgroup of 256 threads (four waves) owns `chunk` consecutive centres of ONE frame (md_centres; ta_md_sweep.h
// holds what the launches on the resident list share). ONE WAVE takes one centre at a time and sweeps that centre's
// run pair_start[i] .. pair_start[i + 1] of the list, 64 entries a round, one entry per lane. Every term of a round
// (a lane outside the cutoff adds 0.0) is summed over the wave by the same butterfly (lane ^ 32, 16, .. 1) and one
// lane adds the round's sum to the centre's sum in LDS: rounds in list order. All sums are fp64 and their order
// is a function of the list alone, so a run reproduces itself bit for bit however it is cut into calls; another
// skin or rebuild pattern orders the list differently and the per-atom values then agree to rounding only.
//
// Pass 1 stores q_lm(i) and N_b(i). Pass 2 sweeps again: a lane inside the cutoff gathers q_lm(j) (8 B x 2 n_lm per
// atom: the table of a 4000-atom frame at degrees (4, 6) is 768 KB, L2-resident), adds it to the qbar sum and
// forms s_ij. q_l, qbar_l and n_conn of the centre are written per atom and kept in LDS; when all centres of the
// workgroup are done they are binned into the workgroup's LDS histograms with 32-bit integer LDS atomics,
//     hist_q / hist_qbar [f][a][degree][min(B - 1, floor(q B))],   hist_conn [f][a][min(n_conn, 31)],
// which are merged into the unsigned 64-bit accumulators in HBM with ONE integer global atomic per non-zero LDS
// bin. A NaN counts nowhere. Integer sums do not depend on the order of arrival. No floating-point atomics, and no
// workgroup waits for another.
//
// Tiling rule: the LDS histogram of q and qbar has at most kMdOrderLdsWords = 8192 words. When 2 E n_degrees n_bins
// exceeds that, the workgroup tiles over BINS: passes of floor(8192 / (2 E n_degrees)) bins each, every pass
// binning the per-atom values kept in LDS again. The sweep is not redone.
//
// The launch arguments are pinned in scalar registers in one round at entry. Both launches are predicated on the
// integrator's status word with the integrator's own test: a state that was reached on a stale list adds nothing
// and overwrites nothing, and the loop enqueues both launches again after the rebuild.
#include <hip/hip_runtime.h>

#include "ta_device.h"
#include "ta_md.h"
#include "ta_md_sweep.h"

namespace ta {
namespace {

constexpr int kOrderThreads = 256, kOrderWaves = kOrderThreads / 64;
static_assert(2 * kMaxElements * kMdOrderMaxDegrees <= kMdOrderLdsWords, "at least one bin per pass");
static_assert(13 + 12 + 11 + 10 == kMdOrderMaxLm && kMdOrderMaxL == 12 && kMdOrderMaxDegrees == 4, "the largest setting");

__device__ __forceinline__ void pin_args(const MdOrderLaunch &a) {
  pin_list(a.list);
  asm volatile("" ::"s"(a.rb2), "s"(a.norm), "s"(a.qlm), "s"(a.q), "s"(a.qbar), "s"(a.n_bonds), "s"(a.n_conn),
               "s"(a.hist_q), "s"(a.hist_qbar), "s"(a.hist_conn), "s"(a.n_bins), "s"(a.n_degrees), "s"(a.n_lm),
               "s"(a.solid), "s"(a.deg0), "s"(a.deg1), "s"(a.deg2), "s"(a.deg3), "s"(a.threshold));
}

// The sum over the 64 lanes, in every lane, by a tree that is the same for every call. This launch's own: the
// wave_sum of ta_math.h adds in another order, which would round every q_lm differently.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ int degree_of(const MdOrderLaunch &a, int d) {
  return d == 0 ? a.deg0 : d == 1 ? a.deg1 : d == 2 ? a.deg2 : a.deg3;
}

struct OrderNeighbour {
  double x, y, z;
  int j;
  bool ok;
};

// entry q + lane of the list as a neighbour of the centre (xi, yi, zi) of species sa (not ok beyond the run or the
// cutoff; a NaN is not ok)
__device__ __forceinline__ OrderNeighbour order_neighbour(const MdOrderLaunch &a, const double (&h)[9], int q, int q_hi,
                                                          int lane, double xi, double yi, double zi, int sa) {
  const MdList &l = a.list;
  const MdEntry e = md_entry(l, h, q, q_hi, lane, xi, yi, zi);
  OrderNeighbour n;
  n.x = e.x, n.y = e.y, n.z = e.z, n.j = e.j;
  n.ok = e.in_run && n.x * n.x + n.y * n.y + n.z * n.z < a.rb2[sa * l.n_elements + l.species[n.j]];
  return n;
}

// q_l of the n_l + 1 complex numbers at c: sqrt(4 pi / (2 l + 1) (|c_0|^2 + 2 sum_{m > 0} |c_m|^2)), scaled by s
__device__ __forceinline__ double order_invariant(const double *c, int l, double s) {
  double t = 0.0;
  for (int m = l; m >= 1; --m) t += (s * c[2 * m]) * (s * c[2 * m]) + (s * c[2 * m + 1]) * (s * c[2 * m + 1]);
  t = 2.0 * t + ((s * c[0]) * (s * c[0]) + (s * c[1]) * (s * c[1]));
  return sqrt(4.0 * M_PI / (double)(2 * l + 1) * t);
}

// Pass 1: q_lm(i) and N_b(i)
__global__ __launch_bounds__(kOrderThreads) void md_order_qlm_kernel(MdOrderLaunch a) {
  __shared__ double s_sum[kOrderWaves][2 * kMdOrderMaxLm];
  pin_args(a);
  const MdList &l = a.list;
  if (md_stale(l.status, l.seq)) return;
  const int lane = (int)threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int M2 = 2 * a.n_lm;
  const auto [f, i_lo, i_hi] = md_centres(l);
  if (i_lo >= i_hi) return;  // (the whole workgroup: an empty frame's one workgroup)
  double h[9];
  md_load_cell(l.cells, f, h);
  double *sum = s_sum[wave];
  for (int i = i_lo + wave; i < i_hi; i += kOrderWaves) {
    const int q_lo = l.pair_start[i], q_hi = l.pair_start[i + 1];
    const int sa = l.species[i];
    const double xi = l.pos[3 * (size_t)i], yi = l.pos[3 * (size_t)i + 1], zi = l.pos[3 * (size_t)i + 2];
    for (int t = lane; t < M2; t += 64) sum[t] = 0.0;
    wave_sync();
    int nb = 0;
    for (int q = q_lo; q < q_hi; q += 64) {
      const OrderNeighbour v = order_neighbour(a, h, q, q_hi, lane, xi, yi, zi, sa);
      const unsigned long long mask = __ballot(v.ok);
      if (mask == 0ull) continue;
      nb += __popcll(mask);
      // a lane outside the cutoff carries the direction (0, 0, 1) and adds 0.0
      const double rinv = v.ok ? 1.0 / sqrt(v.x * v.x + v.y * v.y + v.z * v.z) : 0.0;
      const double ex = v.ok ? v.x * rinv : 0.0, ey = v.ok ? v.y * rinv : 0.0, t = v.ok ? v.z * rinv : 1.0;
      int at = 0;
      for (int d = 0; d < a.n_degrees; ++d) {
        const int l = degree_of(a, d);
        double er = v.ok ? 1.0 : 0.0, ei = 0.0;  // e^m
        double qmm = 1.0;                        // Q_m^m
        for (int m = 0; m <= l; ++m, ++at) {
          double ql = qmm;
          if (m < l) {
            double p0 = qmm;
            ql = (double)(2 * m + 1) * t * p0;
            for (int ll = m + 2; ll <= l; ++ll) {
              const double p2 = ((double)(2 * ll - 1) * t * ql - (double)(ll + m - 1) * p0) / (double)(ll - m);
              p0 = ql;
              ql = p2;
            }
          }
          const double c = a.norm[at] * ql;
          const double yr = wave_sum(c * er), yi_ = wave_sum(c * ei);
          if (lane == 0) sum[2 * at] += yr, sum[2 * at + 1] += yi_;
          const double nr = er * ex - ei * ey;
          ei = er * ey + ei * ex;
          er = nr;
          qmm *= -(double)(2 * m + 1);
        }
      }
    }
    wave_sync();
    const double inv = nb > 0 ? 1.0 / (double)nb : 0.0;
    for (int t = lane; t < M2; t += 64) a.qlm[(size_t)i * M2 + t] = nb > 0 ? sum[t] * inv : 0.0;
    if (lane == 0) a.n_bonds[i] = nb;
    wave_sync();  // (before the sums are zeroed for the next centre)
  }
}

// Pass 2: qbar_lm, the invariants, the solid bonds, the histograms
__global__ __launch_bounds__(kOrderThreads) void md_order_bar_kernel(MdOrderLaunch a) {
  extern __shared__ unsigned s_hist[];  // min(2 E D n_bins, kMdOrderLdsWords) words of q and qbar, then E x 32 of n_conn
  __shared__ double s_cen[kOrderWaves][2 * kMdOrderMaxLm], s_sum[kOrderWaves][2 * kMdOrderMaxLm];
  __shared__ double s_val[kMdOrderMaxChunk][2 * kMdOrderMaxDegrees];  // q then qbar of the workgroup's centres
  __shared__ int s_conn[kMdOrderMaxChunk], s_sp[kMdOrderMaxChunk];
  pin_args(a);
  const MdList &l = a.list;
  if (md_stale(l.status, l.seq)) return;
  const int lane = (int)threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int E = l.n_elements, B = a.n_bins, D = a.n_degrees, M = a.n_lm, M2 = 2 * M;
  const auto [f, i_lo, i_hi] = md_centres(l);
  if (i_lo >= i_hi) return;  // (the whole workgroup: an empty frame's one workgroup)
  double h[9];
  md_load_cell(l.cells, f, h);
  // where the solid degree's q_lm start, and its l
  int so = 0;
  for (int d = 0; d < a.solid; ++d) so += degree_of(a, d) + 1;
  const int sl = degree_of(a, a.solid);
  double *cen = s_cen[wave], *sum = s_sum[wave];
  for (int i = i_lo + wave; i < i_hi; i += kOrderWaves) {
    const int q_lo = l.pair_start[i], q_hi = l.pair_start[i + 1];
    const int sa = l.species[i];
    const double xi = l.pos[3 * (size_t)i], yi = l.pos[3 * (size_t)i + 1], zi = l.pos[3 * (size_t)i + 2];
    for (int t = lane; t < M2; t += 64) cen[t] = sum[t] = a.qlm[(size_t)i * M2 + t];
    wave_sync();
    // |q_l(i)|^2 over all m of the solid degree
    double ni2 = 0.0;
    for (int m = sl; m >= 1; --m) ni2 += cen[2 * (so + m)] * cen[2 * (so + m)] + cen[2 * (so + m) + 1] * cen[2 * (so + m) + 1];
    ni2 = 2.0 * ni2 + (cen[2 * so] * cen[2 * so] + cen[2 * so + 1] * cen[2 * so + 1]);
    const double ni = sqrt(ni2);
    int nb = 0, nc = 0;
    for (int q = q_lo; q < q_hi; q += 64) {
      const OrderNeighbour v = order_neighbour(a, h, q, q_hi, lane, xi, yi, zi, sa);
      const unsigned long long mask = __ballot(v.ok);
      if (mask == 0ull) continue;
      nb += __popcll(mask);
      const double *qj = a.qlm + (size_t)v.j * M2;
      double dot = 0.0, nj2 = 0.0;
      for (int c = 0; c < M; ++c) {
        const double gr = v.ok ? qj[2 * c] : 0.0, gi = v.ok ? qj[2 * c + 1] : 0.0;
        const double sr = wave_sum(gr), si = wave_sum(gi);
        if (lane == 0) sum[2 * c] += sr, sum[2 * c + 1] += si;
        if (c >= so && c <= so + sl) {
          const double w = c == so ? 1.0 : 2.0;
          dot += w * (cen[2 * c] * gr + cen[2 * c + 1] * gi);
          nj2 += w * (gr * gr + gi * gi);
        }
      }
      const double nj = sqrt(nj2);
      const bool solid = v.ok && ni > 0.0 && nj > 0.0 && dot / (ni * nj) > a.threshold;
      nc += __popcll(__ballot(solid));
    }
    wave_sync();
    if (lane < D) {
      int at = 0;
      for (int d = 0; d < lane; ++d) at += degree_of(a, d) + 1;
      const int l = degree_of(a, lane);
      const double ql = order_invariant(cen + 2 * at, l, 1.0);
      const double qb = order_invariant(sum + 2 * at, l, 1.0 / (double)(nb + 1));
      a.q[(size_t)i * D + lane] = ql;
      a.qbar[(size_t)i * D + lane] = qb;
      s_val[i - i_lo][lane] = ql;
      s_val[i - i_lo][D + lane] = qb;
    }
    if (lane == 0) {
      a.n_conn[i] = nc;
      s_conn[i - i_lo] = nc;
      s_sp[i - i_lo] = sa;
    }
    wave_sync();  // (before the next centre's q_lm replace these)
  }
  // the workgroup's values into the histograms
  const int n_cen = i_hi - i_lo, ED = E * D;
  const int tile = B < kMdOrderLdsWords / (2 * ED) ? B : kMdOrderLdsWords / (2 * ED);  // bins per pass
  unsigned *s_hconn = s_hist + (2 * ED * B < kMdOrderLdsWords ? 2 * ED * B : kMdOrderLdsWords);
  const int n_conn_words = E * (kMdOrderMaxConn + 1);
  for (int t = (int)threadIdx.x; t < n_conn_words; t += kOrderThreads) s_hconn[t] = 0u;
  __syncthreads();  // (also: every wave's s_val, s_conn and s_sp are written)
  for (int t = (int)threadIdx.x; t < n_cen; t += kOrderThreads) {
    const int nc = s_conn[t];
    atomicAdd(&s_hconn[s_sp[t] * (kMdOrderMaxConn + 1) + (nc < kMdOrderMaxConn ? nc : kMdOrderMaxConn)], 1u);
  }
  __syncthreads();
  md_merge_counts<kOrderThreads>(s_hconn, n_conn_words, a.hist_conn + (size_t)f * n_conn_words);
  for (int k0 = 0; k0 < B; k0 += tile) {
    const int nk = B - k0 < tile ? B - k0 : tile;
    for (int t = (int)threadIdx.x; t < 2 * ED * nk; t += kOrderThreads) s_hist[t] = 0u;
    __syncthreads();
    for (int t = (int)threadIdx.x; t < n_cen * 2 * D; t += kOrderThreads) {
      const int ic = t / (2 * D), w = t % (2 * D), which = w / D, d = w % D;
      const double kf = floor(s_val[ic][w] * (double)B);
      if (!(kf >= 0.0)) continue;  // a NaN counts nowhere
      const int k = (kf < (double)(B - 1) ? (int)kf : B - 1) - k0;
      if (k < 0 || k >= nk) continue;  // another pass's
      atomicAdd(&s_hist[((which * E + s_sp[ic]) * D + d) * nk + k], 1u);
    }
    __syncthreads();
    md_merge_hist<kOrderThreads>(s_hist, ED, nk, a.hist_q + (size_t)f * ED * B, B, k0);  // (q first, then qbar)
    md_merge_hist<kOrderThreads>(s_hist + ED * nk, ED, nk, a.hist_qbar + (size_t)f * ED * B, B, k0);
    __syncthreads();
  }
}

}  // namespace

void launch_md_order(const MdOrderLaunch &a, hipStream_t s) {
  if (a.list.n_blk <= 0 || a.n_bins <= 0) return;
  const long long words = 2ll * a.list.n_elements * a.n_degrees * a.n_bins;
  const size_t lds = ((size_t)(words < kMdOrderLdsWords ? words : kMdOrderLdsWords) +
                      (size_t)a.list.n_elements * (kMdOrderMaxConn + 1)) * sizeof(unsigned);
  hipLaunchKernelGGL(md_order_qlm_kernel, dim3((unsigned)a.list.n_blk), dim3(kOrderThreads), 0, s, a);
  hipLaunchKernelGGL(md_order_bar_kernel, dim3((unsigned)a.list.n_blk), dim3(kOrderThreads), lds, s, a);
}

}  // namespace ta
