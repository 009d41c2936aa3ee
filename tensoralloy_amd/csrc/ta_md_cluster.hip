// Clusters of selected atoms inside the device MD loop (ta_md_set_clusters): the four launches ta_md_run puts IN
// FRONT OF the integrator launch of a sampled step, behind the bond-order launches of the same step, while the
// device still holds the whole-step state x(t).
//
// Atom i of species a is SELECTED when bit a of species_mask is set and (n_min == 0 or n_conn(i) >= n_min), n_conn
// being that of the bond-order launches for the same state. Two selected atoms i != j are LINKED when the resident
// (skin) list holds an entry (j, S) of centre i with
//     d = x_j - x_i + S . h (fp64),   d . d < rl[a][b]^2,   b = species of j
// (md_entry, then this test; ta_md_sweep.h holds what the launches on the resident list share; an image of i itself
// links nothing, several images of j link once). A cluster is a connected component of the selected atoms under
// links; its label is the smallest index of its members in the batch, its size the number of its atoms. Everything
// is an integer and a function of the state alone.
//
// 1. md_cluster_select_kernel   a thread per atom: parent[i] = i when selected, -1 otherwise; count[i] = 0.
// 2. md_cluster_link_kernel     lock-free union by index on parent[]. A workgroup of four waves owns `chunk`
//    consecutive centres of one frame (md_centres, on the plan of the bond-order launches); a wave takes one selected
//    centre at a time and sweeps its run of the list 64 entries a round, a lane per entry. A lane that holds a link
//    (i, j) with j < i (the list holds every link from both ends: the larger end joins the two, once)
//    walks both ends to their roots and, with hi and lo the larger and the smaller root, does
//        old = atomic fetch-min(&parent[hi], lo);
//    it is done when old == hi (hi was a root and now hangs under lo) or old == lo (someone else did it), and goes
//    on with the pair (old, lo) otherwise: hi had got a parent meanwhile, which must still be joined with lo.
//    parent[x] <= x holds at all times and parent[] is only ever lowered, so every walk and every retry strictly
//    descends and ends by itself whatever the other threads do; a value read late is a former ancestor, which
//    the same reasoning covers. No thread waits for another. The last root of a component is its smallest index.
//    A walk of several hops also lowers the parent of its first atom to the root it found, which shortens later walks.
//    Every access to parent[] in this launch is an agent-scope relaxed atomic: the L1s of the compute units and
//    the L2s of the dies are not coherent within a launch. All the same every loop is capped at the frame's atom
//    count; a lane that overruns sets the give-up word, which ta_md_run reads at its end.
// 3. md_cluster_flatten_kernel  a thread per atom: label[i] = root of i; the lanes of a wave that share a root add
//    their number to count[root] with one integer atomic.
// 4. md_cluster_summary_kernel  one workgroup per frame: size[i] = count[label[i]]; every root is one cluster and
//    goes into an LDS histogram (32-bit integer atomics, bin min(size, B) - 1), merged into the unsigned 64-bit
//    accumulator with one integer global atomic per non-zero bin; the frame's row {selected atoms, clusters, size
//    of the largest cluster, its label (the smallest among equals; -1 when nothing is selected)} comes from an
//    integer reduction over the workgroup. B <= TA_MD_MAX_BINS = kMdClusterLdsWords = 4096 words fit the LDS: no tiling.
// Launches 3 and 4 see what the launches before them wrote through the kernel boundary. No floating-point atomics,
// no grid barrier, no host wait.
//
// The launch arguments are pinned in scalar registers in one round at entry. All four launches are predicated on
// the integrator's status word with the integrator's own test: a state that was reached on a stale list adds
// nothing and overwrites nothing, and the loop enqueues the four launches again after the rebuild.
#include <hip/hip_runtime.h>

#include "ta_device.h"
#include "ta_md.h"
#include "ta_md_sweep.h"

namespace ta {
namespace {

constexpr int kClusterThreads = 256, kClusterWaves = kClusterThreads / 64;
constexpr int kClusterSummaryThreads = 1024, kClusterSummaryWaves = kClusterSummaryThreads / 64;

__device__ __forceinline__ void pin_args(const MdClusterLaunch &a) {
  pin_list(a.list);
  asm volatile("" ::"s"(a.rl2), "s"(a.n_conn), "s"(a.parent), "s"(a.count), "s"(a.label), "s"(a.size), "s"(a.hist),
               "s"(a.row), "s"(a.giveup), "s"(a.n_atoms), "s"(a.n_bins), "s"(a.n_min), "s"(a.species_mask));
}

__device__ __forceinline__ void give_up(const MdClusterLaunch &a) {
  __hip_atomic_store(a.giveup, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// x becomes its root as this thread sees it (a former root at worst); false after more than `cap` hops. A walk of
// more than one hop hangs its first atom directly under the root it found (an integer atomic minimum that nobody
// waits for: the root is below every atom of the walk and in their component, so the invariant holds), which
// keeps the walks short: every atom is the first atom of the walks of its own sweep.
__device__ __forceinline__ bool find_root(int32_t *parent, int &x, int cap) {
  const int first = x;
  for (int n = 0; n <= cap; ++n) {
    const int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == x) {
      if (n > 1) (void)__hip_atomic_fetch_min(parent + first, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return true;
    }
    if (p < 0) return false;  // (never: only selected atoms are walked)
    x = p;
  }
  return false;
}

// joins the components of a and b and leaves their root, as this thread saw it last, in a; false when a loop
// overran `cap`
__device__ __forceinline__ bool unite(int32_t *parent, int &a, int b, int cap) {
  for (int n = 0; n <= cap; ++n) {
    if (!find_root(parent, a, cap) || !find_root(parent, b, cap)) return false;
    if (a == b) return true;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = __hip_atomic_fetch_min(parent + hi, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    a = lo;
    if (old == hi || old == lo) return true;
    b = old;  // hi had a parent already: that one and lo are still to be joined (both below hi)
  }
  return false;
}

__global__ __launch_bounds__(kClusterThreads) void md_cluster_select_kernel(MdClusterLaunch a) {
  pin_args(a);
  const MdList &l = a.list;
  if (md_stale(l.status, l.seq)) return;
  const long long i = (long long)blockIdx.x * kClusterThreads + threadIdx.x;
  if (i >= a.n_atoms) return;
  bool sel = ((a.species_mask >> l.species[i]) & 1) != 0;
  if (a.n_min > 0) sel = sel && a.n_conn[i] >= a.n_min;
  a.parent[i] = sel ? (int32_t)i : -1;
  a.count[i] = 0;
}

__global__ __launch_bounds__(kClusterThreads) void md_cluster_link_kernel(MdClusterLaunch a) {
  pin_args(a);
  const MdList &l = a.list;
  if (md_stale(l.status, l.seq)) return;
  const int lane = (int)threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const auto [f, i_lo, i_hi] = md_centres(l);
  if (i_lo >= i_hi) return;  // (the whole workgroup: an empty frame's one workgroup)
  const int cap = l.atom_start[f + 1] - l.atom_start[f];
  double h[9];
  md_load_cell(l.cells, f, h);
  bool ok_all = true;
  for (int i = i_lo + wave; i < i_hi; i += kClusterWaves) {
    // (whether an atom is selected never changes within the launch)
    if (__hip_atomic_load(a.parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) continue;
    const int q_lo = l.pair_start[i], q_hi = l.pair_start[i + 1];
    const int sa = l.species[i];
    const double xi = l.pos[3 * (size_t)i], yi = l.pos[3 * (size_t)i + 1], zi = l.pos[3 * (size_t)i + 2];
    int up = i;  // an ancestor of i, the lowest this lane has seen: its walks start there, not at i again
    for (int q = q_lo; q < q_hi; q += 64) {
      const MdEntry e = md_entry(l, h, q, q_hi, lane, xi, yi, zi);
      const int j = e.j;
      // the list holds every link from both ends, as entry (j, S) of centre i and as entry (i, -S) of centre j, and
      // d is the same number but for its sign: the larger end joins the two, once
      const bool ok = e.in_run && j < i && e.x * e.x + e.y * e.y + e.z * e.z < a.rl2[sa * l.n_elements + l.species[j]];
      // the parent of j says whether j is selected, and is the first hop of its walk
      const int pj = ok ? __hip_atomic_load(a.parent + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : -1;
      if (pj >= 0) ok_all = unite(a.parent, up, pj, cap) && ok_all;
    }
  }
  if (!ok_all) give_up(a);
}

__global__ __launch_bounds__(kClusterThreads) void md_cluster_flatten_kernel(MdClusterLaunch a) {
  pin_args(a);
  const MdList &l = a.list;
  if (md_stale(l.status, l.seq)) return;
  const long long i = (long long)blockIdx.x * kClusterThreads + threadIdx.x;
  int root = -1;
  if (i < a.n_atoms && a.parent[i] >= 0) {
    const int f = md_frame_of(l.atom_start, l.n_frames + 1, (int)i);  // (the last f with atom_start[f] <= i)
    const int cap = l.atom_start[f + 1] - l.atom_start[f];
    root = (int)i;
    bool ok = false;
    for (int n = 0; n <= cap && !ok; ++n) {
      const int p = a.parent[root];
      ok = p == root;
      if (p < 0) break;  // (never)
      root = p;
    }
    if (!ok) {
      give_up(a);
      root = (int)i;  // (a valid index; the run fails)
    }
  }
  if (i < a.n_atoms) a.label[i] = root;
  // the lanes that share a root add their number once
  bool pending = root >= 0;
  while (true) {
    const unsigned long long todo = __ballot(pending);
    if (todo == 0ull) break;
    const int r0 = __shfl(root, __ffsll((long long)todo) - 1);
    const unsigned long long same = __ballot(pending && root == r0);
    if (pending && root == r0) {
      if (((int)threadIdx.x & 63) == __ffsll((long long)same) - 1)
        __hip_atomic_fetch_add(a.count + r0, __popcll(same), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      pending = false;
    }
  }
}

__global__ __launch_bounds__(kClusterSummaryThreads) void md_cluster_summary_kernel(MdClusterLaunch a) {
  extern __shared__ unsigned s_hist[];  // n_bins words
  __shared__ long long s_sel[kClusterSummaryWaves], s_clu[kClusterSummaryWaves];
  __shared__ unsigned long long s_best[kClusterSummaryWaves];
  pin_args(a);
  const MdList &l = a.list;
  if (md_stale(l.status, l.seq)) return;
  const int f = (int)blockIdx.x, B = a.n_bins;
  const int i_begin = l.atom_start[f], i_end = l.atom_start[f + 1];
  for (int t = (int)threadIdx.x; t < B; t += kClusterSummaryThreads) s_hist[t] = 0u;
  __syncthreads();
  // the largest size wins, among equals the smallest label: the largest key (size, INT32_MAX - label); 0: none
  long long n_sel = 0, n_clu = 0;
  unsigned long long best = 0ull;
  for (int i = i_begin + (int)threadIdx.x; i < i_end; i += kClusterSummaryThreads) {
    const int root = a.label[i];
    const int sz = root >= 0 ? a.count[root] : 0;
    a.size[i] = sz;
    if (root < 0) continue;
    ++n_sel;
    if (root != i || sz < 1) continue;  // (a root counts itself: sz >= 1)
    ++n_clu;
    atomicAdd(&s_hist[(sz < B ? sz : B) - 1], 1u);
    const unsigned long long key = ((unsigned long long)(unsigned)sz << 32) | (unsigned)(0x7fffffff - root);
    best = key > best ? key : best;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n_sel += __shfl_xor(n_sel, o);
    n_clu += __shfl_xor(n_clu, o);
    const unsigned long long other = __shfl_xor(best, o);
    best = other > best ? other : best;
  }
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  if (lane == 0) s_sel[wave] = n_sel, s_clu[wave] = n_clu, s_best[wave] = best;
  __syncthreads();  // (also: every wave's LDS bins are counted)
  if (threadIdx.x == 0) {
    for (int w = 1; w < kClusterSummaryWaves; ++w) {
      n_sel += s_sel[w];
      n_clu += s_clu[w];
      best = s_best[w] > best ? s_best[w] : best;
    }
    long long *row = a.row + 4 * (size_t)f;
    row[0] = n_sel;
    row[1] = n_clu;
    row[2] = (long long)(best >> 32);
    row[3] = best ? (long long)(0x7fffffff - (int)(unsigned)(best & 0xffffffffull)) : -1ll;
  }
  md_merge_counts<kClusterSummaryThreads>(s_hist, B, a.hist + (size_t)f * B);
}

}  // namespace

void launch_md_cluster(const MdClusterLaunch &a, hipStream_t s) {
  if (a.list.n_blk <= 0 || a.n_bins <= 0 || a.n_bins > kMdClusterLdsWords || a.n_atoms <= 0) return;
  const unsigned per_atom = (unsigned)((a.n_atoms + kClusterThreads - 1) / kClusterThreads);
  hipLaunchKernelGGL(md_cluster_select_kernel, dim3(per_atom), dim3(kClusterThreads), 0, s, a);
  hipLaunchKernelGGL(md_cluster_link_kernel, dim3((unsigned)a.list.n_blk), dim3(kClusterThreads), 0, s, a);
  hipLaunchKernelGGL(md_cluster_flatten_kernel, dim3(per_atom), dim3(kClusterThreads), 0, s, a);
  hipLaunchKernelGGL(md_cluster_summary_kernel, dim3((unsigned)a.list.n_frames), dim3(kClusterSummaryThreads),
                     (size_t)a.n_bins * sizeof(unsigned), s, a);
}

}  // namespace ta
