// Partial pair distributions inside the device MD loop (ta_md_set_rdf): the launch ta_md_run puts IN FRONT OF
// the integrator launch of a sampled step, while the device still holds the whole-step state x(t). Every
// directed pair (i, j, S) of the resident (skin) list is counted once:
//     C[f][a][b][k] += 1,   a = species of the centre i, b = species of the neighbour j,
//                           k = floor(r / dr), dr = r_max / n_bins, r = |x_j - x_i + S . h| in fp64
// Pairs with k >= n_bins are dropped by that compare alone (there is no second test of r against r_max), and a
// self-image (i == j, S != 0) is a pair like any other. The resident list holds every pair below
// max(rcut, acut) whenever the integrator's list test holds, and r_max does not exceed that.
//
// A workgroup of 256 threads owns `chunk` consecutive centres of ONE frame (md_centres; ta_md_sweep.h holds what the
// launches on the resident list share). The pairs are sorted by centre and contiguous, so the workgroup's pairs are
// ONE run pair_start[first centre] .. pair_start[last centre + 1] of the list: thread t takes pairs t, t + 256, ... of
// that run, four at a time, with the centre from pair_i: every lane works whatever the neighbour counts are,
// and the list entries of the four pairs, then their position and species gathers, are in flight together (the
// sweep is two dependent rounds of loads per pair, so its time is latency over the pairs in flight).
//
// The workgroup's histogram [E][E][bins] is built in LDS with 32-bit integer LDS atomics (a workgroup sees
// fewer than 2^32 pairs) and merged into the unsigned 64-bit accumulators in HBM with ONE integer global atomic
// per non-zero LDS bin. Integer sums do not depend on the order of arrival: the counts are exact and do not
// depend on how a run is cut into calls. No floating-point atomics.
//
// Tiling rule: the LDS histogram has at most kMdRdfLdsWords = 8192 words (32 KB; the launch asks for the
// min(E^2 n_bins, 8192) words it needs, so that small histograms do not limit the workgroups per CU). When
// E^2 n_bins exceeds that, the workgroup tiles over BINS: passes of floor(8192 / E^2) bins each (at least 128,
// as E <= 8), every pass sweeping the workgroup's pairs again and counting those of its bin range. There is no
// other algorithm.
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

constexpr int kRdfThreads = 256, kRdfBatch = 4;
static_assert(kMaxElements * kMaxElements <= kMdRdfLdsWords, "at least one bin per pass");

__device__ __forceinline__ void pin_args(const MdRdfLaunch &a) {
  pin_list(a.list);
  asm volatile("" ::"s"(a.pair_i), "s"(a.counts), "s"(a.n_bins), "s"(a.dr));
}

__global__ __launch_bounds__(kRdfThreads) void md_rdf_kernel(MdRdfLaunch a) {
  extern __shared__ unsigned s_hist[];  // min(E^2 n_bins, kMdRdfLdsWords) words
  pin_args(a);
  const MdList &l = a.list;
  if (md_stale(l.status, l.seq)) return;
  const int E = l.n_elements, B = a.n_bins, EE = E * E;
  const auto [f, i_lo, i_hi] = md_centres(l);
  if (i_lo >= i_hi) return;  // (the whole workgroup: an empty frame's one workgroup)
  double h[9];
  md_load_cell(l.cells, f, h);
  const int q_lo = l.pair_start[i_lo], q_hi = l.pair_start[i_hi];
  const int tile = B < kMdRdfLdsWords / EE ? B : kMdRdfLdsWords / EE;  // bins per pass
  unsigned long long *acc = a.counts + (size_t)f * EE * B;
  for (int k0 = 0; k0 < B; k0 += tile) {
    const int nk = B - k0 < tile ? B - k0 : tile;
    for (int t = (int)threadIdx.x; t < EE * nk; t += kRdfThreads) s_hist[t] = 0u;
    __syncthreads();
    for (int q0 = q_lo + (int)threadIdx.x; q0 < q_hi; q0 += kRdfBatch * kRdfThreads) {
      // kRdfBatch pairs per thread and round, their loads issued together: the list entries, then the gathers
      // (a slot beyond the run repeats pair q0 and is not counted)
      int i[kRdfBatch], j[kRdfBatch], S[kRdfBatch][3], ab[kRdfBatch];
      double d[kRdfBatch][3];
      bool ok[kRdfBatch];
#pragma unroll
      for (int u = 0; u < kRdfBatch; ++u) {
        const int q = q0 + u * kRdfThreads;
        ok[u] = q < q_hi;
        const size_t qc = (size_t)(ok[u] ? q : q0);
        i[u] = a.pair_i[qc], j[u] = l.pair_j[qc];
        S[u][0] = l.pair_shift[3 * qc], S[u][1] = l.pair_shift[3 * qc + 1], S[u][2] = l.pair_shift[3 * qc + 2];
      }
#pragma unroll
      for (int u = 0; u < kRdfBatch; ++u) {
#pragma unroll
        for (int c = 0; c < 3; ++c) d[u][c] = l.pos[3 * (size_t)j[u] + c] - l.pos[3 * (size_t)i[u] + c];
        ab[u] = l.species[i[u]] * E + l.species[j[u]];
      }
#pragma unroll
      for (int u = 0; u < kRdfBatch; ++u) {
        double ix, iy, iz;
        md_image(h, S[u][0], S[u][1], S[u][2], ix, iy, iz);
        const double dx = d[u][0] + ix, dy = d[u][1] + iy, dz = d[u][2] + iz;
        const double kf = floor(sqrt(dx * dx + dy * dy + dz * dz) / a.dr);
        // k >= n_bins is dropped (a NaN distance counts nowhere); k outside [k0, k0 + nk) is another pass's
        const int k = kf < (double)B ? (int)kf - k0 : -1;
        if (ok[u] && k >= 0 && k < nk) atomicAdd(&s_hist[ab[u] * nk + k], 1u);
      }
    }
    __syncthreads();
    md_merge_hist<kRdfThreads>(s_hist, EE, nk, acc, B, k0);
    __syncthreads();
  }
}

}  // namespace

void launch_md_rdf(const MdRdfLaunch &a, hipStream_t s) {
  if (a.list.n_blk <= 0 || a.n_bins <= 0) return;
  const long long words = (long long)a.list.n_elements * a.list.n_elements * a.n_bins;
  const size_t lds = (size_t)(words < kMdRdfLdsWords ? words : kMdRdfLdsWords) * sizeof(unsigned);
  hipLaunchKernelGGL(md_rdf_kernel, dim3((unsigned)a.list.n_blk), dim3(kRdfThreads), lds, s, a);
}

}  // namespace ta
