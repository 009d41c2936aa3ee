// Device functions the launches of the resident loops share. The first two serve every launch that is predicated on
// the status word or cut into workgroups by blk_start (the MD integrators and samplers, ta_relax.hip, ta_neb.hip);
// the rest is the skeleton of the samplers that sweep the resident list through an MdList (ta_md_rdf.hip, _adf, _order,
// _cluster, _cna): the workgroup's centres, the cell, one entry of a centre's run as a displacement, the wave fence,
// the merge of an LDS histogram and the pin of the list's arguments. What a sampler accepts as a neighbour stays with
// the sampler.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ta_md.h"

namespace ta {
namespace {

// The integrator's test of the status word (0, or 1 + seq of the launch whose drift left the list stale): launch `seq`
// was enqueued behind a stale list and does nothing. The same word in every lane, so barriers behind it are uniform.
__device__ __forceinline__ bool md_stale(const unsigned *status, unsigned seq) {
  const unsigned mark = *static_cast<const volatile unsigned *>(status);
  return mark != 0u && mark <= seq;
}

// frame of workgroup `blk`: the last f < n_frames with blk_start[f] <= blk (blk_start[0] = 0; every frame has at
// least one workgroup)
__device__ __forceinline__ int md_frame_of(const int32_t *blk_start, int n_frames, int blk) {
  int lo = 0, hi = n_frames - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (blk_start[mid] <= blk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// The centres i_lo .. i_hi - 1 of workgroup blockIdx.x and their frame. i_lo >= i_hi in the one workgroup of an empty
// frame: the caller returns then, the whole workgroup.
struct MdCentres {
  int f, i_lo, i_hi;
};
__device__ __forceinline__ MdCentres md_centres(const MdList &l) {
  MdCentres c;
  c.f = md_frame_of(l.blk_start, l.n_frames, (int)blockIdx.x);
  const int i_end = l.atom_start[c.f + 1];
  c.i_lo = l.atom_start[c.f] + ((int)blockIdx.x - l.blk_start[c.f]) * l.chunk;
  c.i_hi = c.i_lo + l.chunk < i_end ? c.i_lo + l.chunk : i_end;
  return c;
}

// h = the cell of frame f (rows are lattice vectors)
__device__ __forceinline__ void md_load_cell(const double *cells, int f, double (&h)[9]) {
#pragma unroll
  for (int c = 0; c < 9; ++c) h[c] = cells[9 * (size_t)f + c];
}

// S . h, the image vector of the shift S
__device__ __forceinline__ void md_image(const double (&h)[9], double S0, double S1, double S2, double &x, double &y,
                                         double &z) {
  x = S0 * h[0] + S1 * h[3] + S2 * h[6];
  y = S0 * h[1] + S1 * h[4] + S2 * h[7];
  z = S0 * h[2] + S1 * h[5] + S2 * h[8];
}

// Entry q + lane of the run q .. q_hi - 1 of the centre at (xi, yi, zi): the neighbour j, its shift and
// d = (x_j - x_i) + S . h in fp64. A lane beyond the run repeats entry q (it reads nothing past the list) and says
// !in_run. The caller's test of d comes on top of in_run, with `<` on the accepting side: a NaN is never accepted.
struct MdEntry {
  double x, y, z;
  int j, S0, S1, S2;
  bool in_run;
};
__device__ __forceinline__ MdEntry md_entry(const MdList &l, const double (&h)[9], int q, int q_hi, int lane, double xi,
                                            double yi, double zi) {
  MdEntry e;
  e.in_run = q + lane < q_hi;
  const size_t qc = (size_t)(e.in_run ? q + lane : q);
  e.j = l.pair_j[qc];
  e.S0 = l.pair_shift[3 * qc], e.S1 = l.pair_shift[3 * qc + 1], e.S2 = l.pair_shift[3 * qc + 2];
  double ix, iy, iz;
  md_image(h, e.S0, e.S1, e.S2, ix, iy, iz);
  e.x = (l.pos[3 * (size_t)e.j] - xi) + ix;
  e.y = (l.pos[3 * (size_t)e.j + 1] - yi) + iy;
  e.z = (l.pos[3 * (size_t)e.j + 2] - zi) + iz;
  return e;
}

// what one lane of a wave wrote to the wave's part of LDS is read by its other lanes
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The merge of a workgroup's 32-bit LDS counters into the unsigned 64-bit accumulators in HBM, by the kThreads threads
// of the workgroup behind a __syncthreads() of the caller's: ONE relaxed integer atomic per non-zero word. Integer
// sums do not depend on the order of arrival.
__device__ __forceinline__ void md_add_count(unsigned long long *acc, unsigned c) {
  if (c != 0u) __hip_atomic_fetch_add(acc, (unsigned long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// s_cnt[n] onto acc[n]
template <int kThreads>
__device__ __forceinline__ void md_merge_counts(const unsigned *s_cnt, int n, unsigned long long *acc) {
  for (int t = (int)threadIdx.x; t < n; t += kThreads) md_add_count(acc + t, s_cnt[t]);
}
// s_hist[rows][nk], one pass of a histogram tiled over bins, onto the bins k0 .. k0 + nk - 1 of acc[rows][B]
template <int kThreads>
__device__ __forceinline__ void md_merge_hist(const unsigned *s_hist, int rows, int nk, unsigned long long *acc, int B,
                                              int k0) {
  for (int t = (int)threadIdx.x; t < rows * nk; t += kThreads)
    md_add_count(acc + (size_t)(t / nk) * B + (k0 + t % nk), s_hist[t]);
}

// the list's arguments that the kernels read, pinned in scalar registers in one round (n_blk is the launcher's)
__device__ __forceinline__ void pin_list(const MdList &l) {
  asm volatile("" ::"s"(l.pos), "s"(l.cells), "s"(l.species), "s"(l.atom_start), "s"(l.blk_start), "s"(l.pair_start),
               "s"(l.pair_j), "s"(l.pair_shift), "s"(l.status), "s"(l.seq), "s"(l.n_elements), "s"(l.n_frames),
               "s"(l.chunk));
}

}  // namespace
}  // namespace ta
