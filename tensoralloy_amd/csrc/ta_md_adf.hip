// Bond-angle distributions inside the device MD loop (ta_md_set_adf): the launch ta_md_run puts IN FRONT OF the
// integrator launch of a sampled step, while the device still holds the whole-step state x(t). For every centre
// i (species a) the neighbours are the entries (j, S) of the resident (skin) list with
//     d = x_j - x_i + S . h (fp64),   d . d < rb[a][b]^2,   b = species of j
// and every unordered pair {(j, S), (k, S')} of distinct neighbours counts once:
//     theta = atan2(|u x w|, u . w),  u = d_ij, w = d_ik;   kbin = min(B - 1, floor(theta / (pi / B)))   (fp64)
//     C[f][a][p][kbin] += 1,   p = b E - b (b - 1) / 2 + (c - b) for the species b <= c of the two neighbours
// A NaN counts nowhere. Nothing is stored per triple.
//
// A workgroup of 256 threads (four waves) owns `chunk` consecutive centres of ONE frame (md_centres; ta_md_sweep.h
// holds what the launches on the resident list share). ONE WAVE takes one centre at a time and sweeps that centre's
// run pair_start[i] .. pair_start[i + 1] of the list, 64 entries a round (md_entry). The neighbours that pass the
// cutoff are compacted (ballot and prefix count) into the wave's LDS slab (dx, dy, dz, species) of kMdAdfSlab
// entries; the n (n - 1) / 2 pairs of the slab are then spread evenly over the 64 lanes, whatever n is.
//
// A centre with more neighbours than the slab holds is swept in tiles: the slab takes the neighbours of as many
// whole rounds as fit (block A), the pairs inside A are counted as above, then every later entry of the run is
// read again, one per lane, and paired with all of A (the lanes read the slab entry by entry: one LDS broadcast
// each). The next block A starts where the last one ended. A pair inside one block is counted there, any other
// pair when the block of its earlier member meets its later member: every pair once, for any neighbour count.
//
// The workgroup's histogram [E][P][bins] is built in LDS with 32-bit integer LDS atomics (a workgroup sees fewer
// than 2^32 triples: 64 centres of 11000 neighbours each would be needed) and merged into the unsigned 64-bit
// accumulators in HBM with ONE integer global atomic per non-zero LDS bin. Integer sums do not depend on the
// order of arrival. No floating-point atomics.
//
// Tiling rule: the LDS histogram has at most kMdAdfLdsWords = 8192 words. When E P n_bins exceeds that, the
// workgroup tiles over BINS: passes of floor(8192 / (E P)) bins each, every pass redoing the sweep and counting
// the triples of its bin range. There is no other algorithm.
//
// The launch arguments are pinned in scalar registers in one round at entry. The launch is predicated on the
// integrator's status word with the integrator's own test: a state that was reached on a stale list adds
// nothing, and the loop enqueues the launch again after the rebuild.
#include <hip/hip_runtime.h>

#include "ta_device.h"
#include "ta_md.h"
#include "ta_md_sweep.h"

namespace ta {
namespace {

constexpr int kAdfThreads = 256, kAdfWaves = kAdfThreads / 64;
constexpr int kAdfSlabDoubles = 3 * kMdAdfSlab + kMdAdfSlab / 2;  // dx, dy, dz and the species of a slab
// The bin of a triple is floor(theta / dtheta) of the fp64 definition. Most triples are decided in single precision:
// with the six components rounded to float (2^-24 relative each), cross and dot product carry an absolute error below
// 1e-6 |u| |w|, so the angle one below 1e-6 rad, and atan2f adds at most two ulps of pi, 5e-7 rad. An angle that single
// precision puts further than kAdfSingleRad = 2e-5 rad (more than ten times that bound) from both edges of its bin is in
// that bin in fp64 as well. Every other triple (0.2 % of them at 180 bins, 5 % at 4096; a NaN among them, and bonds
// below 1e-5 A, whose products leave the range of float) is binned by the definition itself. The counts are those of
// the definition either way.
constexpr double kAdfSingleRad = 2.0e-5;
static_assert(kMdAdfSlab >= 64 && kMdAdfSlab % 64 == 0, "an empty slab takes one round of the list whole");
static_assert(kMaxElements * (kMaxElements * (kMaxElements + 1) / 2) <= kMdAdfLdsWords, "at least one bin per pass");

__device__ __forceinline__ void pin_args(const MdAdfLaunch &a) {
  pin_list(a.list);
  asm volatile("" ::"s"(a.rb2), "s"(a.counts), "s"(a.n_bins), "s"(a.dtheta));
}

struct AdfNeighbour {
  double x, y, z;
  int sp;
  bool ok;
};

__global__ __launch_bounds__(kAdfThreads) void md_adf_kernel(MdAdfLaunch a) {
  extern __shared__ double s_mem[];  // the four slabs, then min(E P n_bins, kMdAdfLdsWords) histogram words
  pin_args(a);
  const MdList &l = a.list;
  if (md_stale(l.status, l.seq)) return;
  const int E = l.n_elements, B = a.n_bins, P = E * (E + 1) / 2, EP = E * P;
  const int lane = (int)threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  double *sx = s_mem + wave * kAdfSlabDoubles, *sy = sx + kMdAdfSlab, *sz = sy + kMdAdfSlab;
  int *ss = reinterpret_cast<int *>(sz + kMdAdfSlab);
  unsigned *s_hist = reinterpret_cast<unsigned *>(s_mem + kAdfWaves * kAdfSlabDoubles);
  const auto [f, i_lo, i_hi] = md_centres(l);
  if (i_lo >= i_hi) return;  // (the whole workgroup: an empty frame's one workgroup)
  double h[9];
  md_load_cell(l.cells, f, h);
  const int tile = B < kMdAdfLdsWords / EP ? B : kMdAdfLdsWords / EP;  // bins per pass
  unsigned long long *acc = a.counts + (size_t)f * EP * B;
  const double inv_dtheta = 1.0 / a.dtheta, margin = kAdfSingleRad * inv_dtheta;  // (the margin in bins)
  for (int k0 = 0; k0 < B; k0 += tile) {
    const int nk = B - k0 < tile ? B - k0 : tile;
    for (int t = (int)threadIdx.x; t < EP * nk; t += kAdfThreads) s_hist[t] = 0u;
    __syncthreads();
    for (int i = i_lo + wave; i < i_hi; i += kAdfWaves) {
      const int q_lo = l.pair_start[i], q_hi = l.pair_start[i + 1];
      const int sa = l.species[i];
      const double xi = l.pos[3 * (size_t)i], yi = l.pos[3 * (size_t)i + 1], zi = l.pos[3 * (size_t)i + 2];
      unsigned *hist = s_hist + (size_t)sa * P * nk;
      // entry q + lane of the list as a neighbour of i (not ok beyond the run or the cutoff; a NaN is not ok)
      auto neighbour = [&](int q) {
        const MdEntry e = md_entry(l, h, q, q_hi, lane, xi, yi, zi);
        AdfNeighbour n;
        n.x = e.x, n.y = e.y, n.z = e.z;
        n.sp = l.species[e.j];
        n.ok = e.in_run && n.x * n.x + n.y * n.y + n.z * n.z < a.rb2[sa * E + n.sp];
        return n;
      };
      // the triple of the neighbours u (species b) and w (species c) of this centre
      auto count = [&](double ux, double uy, double uz, int b, double wx, double wy, double wz, int c) {
        // the bin from single precision where that decides it (see kAdfSingleRad), from the definition otherwise
        const float fux = (float)ux, fuy = (float)uy, fuz = (float)uz, fwx = (float)wx, fwy = (float)wy, fwz = (float)wz;
        const float fcx = fuy * fwz - fuz * fwy, fcy = fuz * fwx - fux * fwz, fcz = fux * fwy - fuy * fwx;
        const float fs = __builtin_amdgcn_sqrtf(fcx * fcx + fcy * fcy + fcz * fcz);  // (one ulp: inside the bound)
        const float fd = fux * fwx + fuy * fwy + fuz * fwz;
        const double t = (double)atan2f(fs, fd) * inv_dtheta;
        double kf = floor(t);
        // near an edge, not a number, or |u|^2 |w|^2 = |u x w|^2 + (u . w)^2 so small that a product went under
        if (!(t - kf > margin && t - kf < 1.0 - margin && fs * fs + fd * fd > 1.0e-20f)) {
          const double cx = uy * wz - uz * wy, cy = uz * wx - ux * wz, cz = ux * wy - uy * wx;
          const double theta = atan2(sqrt(cx * cx + cy * cy + cz * cz), ux * wx + uy * wy + uz * wz);
          kf = floor(theta / a.dtheta);
          if (!(kf >= 0.0)) return;  // a NaN counts nowhere
        }
        const int k = (kf < (double)(B - 1) ? (int)kf : B - 1) - k0;  // theta = pi belongs to the last bin
        if (k < 0 || k >= nk) return;                                 // another pass's
        const int lo = b < c ? b : c, hi = b < c ? c : b;
        atomicAdd(&hist[(lo * E - lo * (lo - 1) / 2 + (hi - lo)) * nk + k], 1u);
      };
      for (int qa = q_lo; qa < q_hi;) {
        // block A: the neighbours of as many whole rounds from qa on as the slab holds (one round at least)
        int n = 0, q = qa;
        for (; q < q_hi; q += 64) {
          const AdfNeighbour v = neighbour(q);
          const unsigned long long m = __ballot(v.ok);
          const int c = __popcll(m);
          if (n + c > kMdAdfSlab) break;
          if (v.ok) {
            const int at = n + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            sx[at] = v.x, sy[at] = v.y, sz[at] = v.z, ss[at] = v.sp;
          }
          n += c;
        }
        wave_sync();
        // the pairs inside A, t = kk (kk - 1) / 2 + jj for jj < kk, spread over the lanes: t = lane, lane + 64, ...
        int kk = (int)(0.5f * (1.0f + sqrtf(1.0f + 8.0f * (float)lane)));
        while (kk * (kk - 1) / 2 > lane) --kk;
        while ((kk + 1) * kk / 2 <= lane) ++kk;
        int jj = lane - kk * (kk - 1) / 2;
        for (int t = lane; t < n * (n - 1) / 2; t += 64) {
          count(sx[jj], sy[jj], sz[jj], ss[jj], sx[kk], sy[kk], sz[kk], ss[kk]);
          for (jj += 64; jj >= kk; ++kk) jj -= kk;  // row kk of the triangle has kk entries
        }
        // every later entry of the run against all of A (none when the run fitted the slab)
        for (int qb = q; qb < q_hi; qb += 64) {
          const AdfNeighbour v = neighbour(qb);
          if (__ballot(v.ok) == 0ull) continue;
          for (int m = 0; m < n; ++m)
            if (v.ok) count(sx[m], sy[m], sz[m], ss[m], v.x, v.y, v.z, v.sp);
        }
        wave_sync();
        qa = q;
      }
    }
    __syncthreads();
    md_merge_hist<kAdfThreads>(s_hist, EP, nk, acc, B, k0);
    __syncthreads();
  }
}

}  // namespace

void launch_md_adf(const MdAdfLaunch &a, hipStream_t s) {
  if (a.list.n_blk <= 0 || a.n_bins <= 0) return;
  const int E = a.list.n_elements;
  const long long words = (long long)E * (E * (E + 1) / 2) * a.n_bins;
  const size_t lds = (size_t)kAdfWaves * kAdfSlabDoubles * sizeof(double) +
                     (size_t)(words < kMdAdfLdsWords ? words : kMdAdfLdsWords) * sizeof(unsigned);
  hipLaunchKernelGGL(md_adf_kernel, dim3((unsigned)a.list.n_blk), dim3(kAdfThreads), lds, s, a);
}

}  // namespace ta
