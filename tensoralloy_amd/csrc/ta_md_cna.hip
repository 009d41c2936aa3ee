// Common neighbour analysis inside the device MD loop (ta_md_set_cna): the launch ta_md_run puts IN FRONT OF the
// integrator launch of a sampled step, behind the order and cluster launches of that step, while the device still
// holds the whole-step state x(t). It gives every atom its lattice type (OVITO's numbering: 0 OTHER, 1 FCC, 2 HCP,
// 3 BCC, 4 ICO) by the conventional analysis of Honeycutt-Andersen / Faken-Jonsson, at a fixed cutoff (LAMMPS
// `compute cna/atom`) or adaptively (Stukowski 2012, OVITO's default).
//
// Candidates of a centre i are the entries (j, S) of the resident (skin) list with
//     d = x_j - x_i + S . h (fp64),   d . d < r^2,
// (md_entry, then this test; ta_md_sweep.h holds what the launches on the resident list share),
// r = r_max (adaptive) or r_cut (fixed); species do not enter; self-images and several images of one atom are
// neighbours like any other. They are ordered by the key (d . d, j, S0, S1, S2), so the selection is a function of
// the state and not of the order of the list.
//
// For N neighbour vectors and a cutoff rc, neighbours j, k are BONDED when |d_j - d_k| < rc. The signature of
// neighbour j is (n_cn, n_b, l_cb): the neighbours bonded to j, the bonds among those, and the most bonds in one
// connected set of those bonds. FCC: N = 12, twelve (4,2,1). HCP: N = 12, six (4,2,1) and six (4,2,2). ICO: N = 12,
// twelve (5,5,5). BCC: N = 14, eight (6,6,6) and six (4,4,4). Anything else is OTHER.
//     adaptive: fewer than 12 candidates: OTHER, r_local = 0. The 12 nearest with rc = (1 + sqrt 2) / 2 mean |d|
//               test FCC, HCP, ICO; if none matches and there are 14 candidates, the 14 nearest with
//               rc = (1 + sqrt 2) / 2 ((2 / sqrt 3) sum of the 8 nearest |d| + sum of the next 6) / 14 test BCC.
//               r_local is the rc of the last attempt made.
//     fixed:    all N candidates, rc = r_cut = r_local; N = 12 tests FCC, HCP, ICO, N = 14 tests BCC.
//
// A workgroup of 512 threads (eight waves: one centre per wave in a chunk of eight) owns `chunk` consecutive centres
// of ONE frame (md_centres, on the plan of the order launches). ONE WAVE takes one centre at a time
// and sweeps that centre's run pair_start[i] .. pair_start[i + 1] of the list, 64 entries a round, one entry per
// lane, and keeps the 14 smallest keys, sorted, in its part of LDS: a round's candidates that beat the 14th key held
// are ranked against the keys held and against each other, and every survivor stores itself at its rank. A round with
// many such candidates (the first of a centre) takes the ranks from d . d alone, by 14 + 64 broadcast reads at
// constant addresses with no dependent step; two equal d . d (a perfect lattice, the two images +-S of the centre
// itself) send it to the ranking by the whole key, which a round with few such candidates takes at once. Nothing is
// stored per candidate in HBM. The selected vectors then give the adjacency, one mask per neighbour, from the at most
// 91 pair distances spread over the lanes (LDS integer OR); lane j < N forms the signature of neighbour j with bit
// operations (popcount, a flood fill over masks for l_cb), and ballots decide the type. Lane 0 writes structure[i]
// and r_local[i] and counts the type in the workgroup's LDS counters, which go to counts[f][a][5] and to this
// sample's row series[f][5] with ONE integer global atomic per non-zero counter. The row is zeroed by a launch of its
// own in front, under the same predicate. Every output but r_local is an integer and a function of the state alone;
// r_local is a sum in the order of the sorted selection. No floating-point atomics, no grid barrier, and no workgroup
// waits for another.
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

constexpr int kCnaThreads = 512, kCnaWaves = kCnaThreads / 64;
constexpr int kCnaKeep = 14;   // the most neighbours an attempt looks at
constexpr int kCnaSlots = 16;  // their slots in LDS
constexpr int kCnaFewLive = 12;  // live candidates of a round up to which the exact ranking is the cheaper one
constexpr double kCnaFar = 1.0e300;  // d . d of an empty slot: behind every candidate
static_assert(kMdCnaTypes == 5, "OTHER, FCC, HCP, BCC, ICO");

// signatures as n_cn * 10000 + n_b * 100 + l_cb (n_b and l_cb are at most 78)
constexpr int kSig421 = 40201, kSig422 = 40202, kSig555 = 50505, kSig666 = 60606, kSig444 = 40404;

__device__ __forceinline__ void pin_args(const MdCnaLaunch &a) {
  pin_list(a.list);
  asm volatile("" ::"s"(a.structure), "s"(a.r_local), "s"(a.counts), "s"(a.row), "s"(a.mode), "s"(a.r2), "s"(a.r_cut));
}

// (d . d, j, S) of one candidate before that of another; S is packed so that its order is that of (S0, S1, S2)
__device__ __forceinline__ bool key_less(double d2a, int ja, unsigned long long sa, double d2b, int jb, unsigned long long sb) {
  return d2a < d2b || (d2a == d2b && (ja < jb || (ja == jb && sa < sb)));
}

__device__ __forceinline__ unsigned long long pack_shift(int S0, int S1, int S2) {
  constexpr long long bias = 1ll << 20;  // (|S| stays far below: a shift counts cells)
  return ((unsigned long long)(S0 + bias) << 42) | ((unsigned long long)(S1 + bias) << 21) | (unsigned long long)(S2 + bias);
}

// the wave's part of LDS: the neighbours kept, sorted by key, a round's keys, and the adjacency masks
struct CnaWave {
  double x[kCnaSlots], y[kCnaSlots], z[kCnaSlots], d2[kCnaSlots];
  unsigned long long s[kCnaSlots];
  int j[kCnaSlots];
  unsigned adj[kCnaSlots];
  double nd2[64];
  unsigned long long ns[64];
  int nj[64];
};

// The signatures of the n nearest neighbours kept in `w` under the bond cutoff rc2 (squared), as the number of
// neighbours with each of the five signatures the structures are made of (the same in every lane).
struct CnaTally {
  int c421, c422, c555, c666, c444;
};

__device__ __forceinline__ CnaTally cna_signatures(CnaWave &w, int n, double rc2, int lane) {
  if (lane < kCnaSlots) w.adj[lane] = 0u;
  wave_sync();
  // pair p of the n (n - 1) / 2: (j, k), j < k, row by row
  const int n_pairs = n * (n - 1) / 2;
  for (int p = lane; p < n_pairs; p += 64) {
    int j = 0, rem = p;
    while (rem >= n - 1 - j) rem -= n - 1 - j, ++j;
    const int k = j + 1 + rem;
    const double dx = w.x[j] - w.x[k], dy = w.y[j] - w.y[k], dz = w.z[j] - w.z[k];
    if (dx * dx + dy * dy + dz * dz < rc2) {
      atomicOr(&w.adj[j], 1u << k);
      atomicOr(&w.adj[k], 1u << j);
    }
  }
  wave_sync();
  int sig = 0;
  if (lane < n) {
    const unsigned cm = w.adj[lane];  // the common neighbours of the centre and neighbour `lane`
    int nb2 = 0;
    for (unsigned m = cm; m; m &= m - 1u) nb2 += __popc(w.adj[__ffs(m) - 1] & cm);
    // the most bonds in one connected set: flood fill from the lowest node left
    int lmax = 0;
    unsigned left = cm;
    while (left) {
      unsigned comp = left & (0u - left), grown = comp;
      do {
        comp = grown;
        for (unsigned m = comp; m; m &= m - 1u) grown |= w.adj[__ffs(m) - 1] & cm;
      } while (grown != comp);
      int b2 = 0;
      for (unsigned m = comp; m; m &= m - 1u) b2 += __popc(w.adj[__ffs(m) - 1] & comp);
      lmax = b2 / 2 > lmax ? b2 / 2 : lmax;
      left &= ~comp;
    }
    sig = __popc(cm) * 10000 + (nb2 / 2) * 100 + lmax;
  }
  CnaTally t;
  t.c421 = __popcll(__ballot(sig == kSig421));
  t.c422 = __popcll(__ballot(sig == kSig422));
  t.c555 = __popcll(__ballot(sig == kSig555));
  t.c666 = __popcll(__ballot(sig == kSig666));
  t.c444 = __popcll(__ballot(sig == kSig444));
  wave_sync();  // (before the masks are zeroed again)
  return t;
}

__device__ __forceinline__ int cna_type12(const CnaTally &t) {
  return t.c421 == 12 ? kMdCnaFcc : (t.c421 == 6 && t.c422 == 6) ? kMdCnaHcp : t.c555 == 12 ? kMdCnaIco : kMdCnaOther;
}

__device__ __forceinline__ int cna_type14(const CnaTally &t) {
  return (t.c666 == 8 && t.c444 == 6) ? kMdCnaBcc : kMdCnaOther;
}

// this sample's row of the series starts from zero
__global__ __launch_bounds__(64) void md_cna_zero_kernel(MdCnaLaunch a) {
  if (md_stale(a.list.status, a.list.seq)) return;
  const int n = a.list.n_frames * kMdCnaTypes;
  for (int t = (int)(blockIdx.x * blockDim.x + threadIdx.x); t < n; t += (int)(gridDim.x * blockDim.x)) a.row[t] = 0ull;
}

__global__ __launch_bounds__(kCnaThreads) void md_cna_kernel(MdCnaLaunch a) {
  __shared__ CnaWave s_wave[kCnaWaves];
  __shared__ unsigned s_cnt[kMaxElements * kMdCnaTypes];
  pin_args(a);
  const MdList &l = a.list;
  if (md_stale(l.status, l.seq)) return;
  const int lane = (int)threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const auto [f, i_lo, i_hi] = md_centres(l);
  if (i_lo >= i_hi) return;  // (the whole workgroup: an empty frame's one workgroup)
  const int n_cnt = l.n_elements * kMdCnaTypes;
  for (int t = (int)threadIdx.x; t < n_cnt; t += kCnaThreads) s_cnt[t] = 0u;
  __syncthreads();
  double h[9];
  md_load_cell(l.cells, f, h);
  CnaWave &w = s_wave[wave];
  for (int i = i_lo + wave; i < i_hi; i += kCnaWaves) {
    const int q_lo = l.pair_start[i], q_hi = l.pair_start[i + 1];
    const double xi = l.pos[3 * (size_t)i], yi = l.pos[3 * (size_t)i + 1], zi = l.pos[3 * (size_t)i + 2];
    int n_keep = 0, n_cand = 0;  // neighbours kept (at most 14) and candidates seen
    if (lane < kCnaSlots) w.d2[lane] = kCnaFar;
    wave_sync();
    for (int q = q_lo; q < q_hi; q += 64) {
      const MdEntry e = md_entry(l, h, q, q_hi, lane, xi, yi, zi);
      const int j = e.j;
      const double dx = e.x, dy = e.y, dz = e.z, d2 = dx * dx + dy * dy + dz * dz;
      const unsigned long long sk = pack_shift(e.S0, e.S1, e.S2);
      const bool ok = e.in_run && d2 < a.r2;  // (a NaN is no candidate)
      const unsigned long long okm = __ballot(ok);
      if (okm == 0ull) continue;
      n_cand += __popcll(okm);
      // only what beats the 14th key held can enter
      bool live = ok;
      if (n_keep == kCnaKeep) live = ok && key_less(d2, j, sk, w.d2[kCnaKeep - 1], w.j[kCnaKeep - 1], w.s[kCnaKeep - 1]);
      const unsigned long long livem = __ballot(live);
      if (livem == 0ull) continue;
      w.nd2[lane] = live ? d2 : kCnaFar, w.nj[lane] = j, w.ns[lane] = sk;
      // lane k < n_keep takes neighbour k along: its rank grows by the candidates in front of it
      double kx = 0.0, ky = 0.0, kz = 0.0, kd2 = kCnaFar;
      unsigned long long ks = 0ull;
      int kj = 0;
      if (lane < n_keep) kx = w.x[lane], ky = w.y[lane], kz = w.z[lane], kd2 = w.d2[lane], ks = w.s[lane], kj = w.j[lane];
      wave_sync();  // (the round's keys are in LDS)
      // A round with many live candidates (the first ones of a centre) takes the ranks from d . d alone: 14 + 64
      // broadcast reads at constant addresses (an empty slot and a lane that is not live hold kCnaFar), no dependent
      // step. Two equal d . d anywhere send it to the exact loops, which a round with few live candidates takes at once:
      // one dependent step per slot held and per live candidate.
      int rank = 0, krank = lane;
      bool exact = __popcll(livem) <= kCnaFewLive;
      if (!exact) {
        bool tie = false;
#pragma unroll
        for (int k = 0; k < kCnaKeep; ++k) {
          const double b = w.d2[k];
          rank += (live && b < d2) ? 1 : 0;
          tie = tie || (live && b == d2);
        }
#pragma unroll 16
        for (int s = 0; s < 64; ++s) {
          const double b = w.nd2[s];
          rank += (live && b < d2) ? 1 : 0;
          tie = tie || (live && s != lane && b == d2);
          krank += (b < kd2) ? 1 : 0;
        }
        exact = __ballot(tie) != 0ull;
      }
      if (exact) {  // by the whole key (d . d, j, S)
        rank = 0, krank = lane;
        for (int k = 0; k < n_keep; ++k) {
          const bool front = live && key_less(d2, j, sk, w.d2[k], w.j[k], w.s[k]);
          rank += (live && !front) ? 1 : 0;  // (among equals the one held comes first)
          const int n_front = __popcll(__ballot(front));
          if (lane == k) krank += n_front;
        }
        for (unsigned long long m = livem; m; m &= m - 1ull) {
          const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
          const double bd2 = w.nd2[src];
          const int bj = w.nj[src];
          const unsigned long long bs = w.ns[src];
          // (among equals the lower lane comes first)
          const bool behind = key_less(bd2, bj, bs, d2, j, sk) || (!key_less(d2, j, sk, bd2, bj, bs) && src < lane);
          rank += (live && src != lane && behind) ? 1 : 0;
        }
      }
      if (lane < n_keep && krank < kCnaKeep)
        w.x[krank] = kx, w.y[krank] = ky, w.z[krank] = kz, w.d2[krank] = kd2, w.s[krank] = ks, w.j[krank] = kj;
      if (live && rank < kCnaKeep)
        w.x[rank] = dx, w.y[rank] = dy, w.z[rank] = dz, w.d2[rank] = d2, w.s[rank] = sk, w.j[rank] = j;
      const int n_new = n_keep + __popcll(livem);
      n_keep = n_new < kCnaKeep ? n_new : kCnaKeep;
      wave_sync();
    }
    wave_sync();
    int type = kMdCnaOther;
    double r_local = 0.0;
    if (a.mode == kMdCnaFixed) {
      r_local = a.r_cut;
      if (n_cand == 12) type = cna_type12(cna_signatures(w, 12, a.r2, lane));
      if (n_cand == 14) type = cna_type14(cna_signatures(w, 14, a.r2, lane));
    } else if (n_cand >= 12) {
      constexpr double kScale = 1.2071067811865475244;  // (1 + sqrt 2) / 2
      double sum = 0.0;
      for (int k = 0; k < 12; ++k) sum += sqrt(w.d2[k]);
      r_local = kScale * (sum / 12.0);
      type = cna_type12(cna_signatures(w, 12, r_local * r_local, lane));
      if (type == kMdCnaOther && n_cand >= 14) {
        double s8 = 0.0, s6 = 0.0;
        for (int k = 0; k < 8; ++k) s8 += sqrt(w.d2[k]);
        for (int k = 8; k < 14; ++k) s6 += sqrt(w.d2[k]);
        r_local = kScale * ((1.1547005383792515290 * s8 + s6) / 14.0);  // 2 / sqrt 3
        type = cna_type14(cna_signatures(w, 14, r_local * r_local, lane));
      }
    }
    if (lane == 0) {
      a.structure[i] = type;
      a.r_local[i] = r_local;
      atomicAdd(&s_cnt[l.species[i] * kMdCnaTypes + type], 1u);
    }
    wave_sync();  // (before the next centre's neighbours replace these)
  }
  __syncthreads();
  md_merge_counts<kCnaThreads>(s_cnt, n_cnt, a.counts + (size_t)f * n_cnt);
  if ((int)threadIdx.x < kMdCnaTypes) {  // the row is summed over the species
    unsigned c = 0u;
    for (int e = 0; e < l.n_elements; ++e) c += s_cnt[e * kMdCnaTypes + (int)threadIdx.x];
    if (c != 0u)
      __hip_atomic_fetch_add(a.row + (size_t)f * kMdCnaTypes + threadIdx.x, (unsigned long long)c, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace

void launch_md_cna(const MdCnaLaunch &a, hipStream_t s) {
  if (a.list.n_blk <= 0) return;
  const int n_row = a.list.n_frames * kMdCnaTypes;
  hipLaunchKernelGGL(md_cna_zero_kernel, dim3((unsigned)((n_row + 63) / 64)), dim3(64), 0, s, a);
  hipLaunchKernelGGL(md_cna_kernel, dim3((unsigned)a.list.n_blk), dim3(kCnaThreads), 0, s, a);
}

}  // namespace ta
