// Time correlations inside the device MD loop (ta_md_set_sampling): the launch ta_md_run puts behind an
// integrator launch that sampled. The integrator wrote sample n, the whole-step state (x, v), into slot
// n % L of two rings [L][N][3]; here that row is correlated with the rows of the lags k = 0 .. min(n, L - 1)
// (slot (n - k) % L), per frame f and element e:
//     A_v[f][e][k] += sum_i v_i(n) . v_i(n - k),   A_x[f][e][k] += sum_i |x_i(n) - x_i(n - k)|^2
//
// A dot product and a squared distance are sums over components, so a ring row is taken as 3 N plain doubles:
// double j belongs to atom j / 3. A workgroup of 256 threads owns kMdCorrChunk = 768 consecutive doubles of one
// frame (256 atoms) and kMdCorrLagTile lags. Thread t holds doubles t, t + 256 and t + 512 of the chunk's part
// of the newest row in registers and meets the same three of every older row: each wave instruction reads 512
// contiguous bytes, and a row is read once per lag tile, from the last-level cache while the ring fits there
// (the traffic is about (valid lags) x N x 48 bytes per sample). The plan is the launch's own: a 4000-atom
// frame at L = 256 is 16 chunks x 32 lag tiles = 512 workgroups.
//
// Sums are taken in a fixed order: the three doubles of a thread, the lanes of a wave (wave_sum), the four
// waves one after another, one partial per (chunk, e, k) into HBM, and a second small launch adds a frame's
// chunks in index order onto the accumulators. No floating-point atomics, so the value does not depend on how
// a run is cut into calls. Both launches are predicated on the integrator's status word with the integrator's
// own test: behind a stale list they add nothing, and the loop enqueues them again after the rebuild.
#include <hip/hip_runtime.h>

#include "ta_device.h"
#include "ta_math.h"
#include "ta_md.h"
#include "ta_md_sweep.h"

namespace ta {
namespace {

constexpr int kCorrThreads = 256, kCorrWaves = kCorrThreads / 64;
static_assert(kMdCorrChunk == 3 * kCorrThreads, "three ring doubles per thread");
static_assert(2 * kMaxElements * kMdCorrLagTile <= kCorrThreads, "one thread per partial of the tile");

__global__ __launch_bounds__(kCorrThreads) void md_corr_kernel(MdCorrLaunch a) {
  __shared__ double s_part[kCorrWaves][2][kMaxElements][kMdCorrLagTile];
  if (md_stale(a.status, a.seq)) return;
  const int L = a.n_lags, E = a.n_elements;
  const long long kmax = a.n < (long long)(L - 1) ? a.n : (long long)(L - 1);
  const int k0 = (int)blockIdx.y * kMdCorrLagTile;
  if ((long long)k0 > kmax) return;  // (the whole workgroup: the ring has no row for this tile yet)
  const int f = md_frame_of(a.blk_start, a.n_frames, (int)blockIdx.x);
  const long long j_hi = 3ll * a.atom_start[f + 1];
  const long long j_lo = 3ll * a.atom_start[f] + (long long)((int)blockIdx.x - a.blk_start[f]) * kMdCorrChunk;
  const size_t row = 3 * (size_t)a.n_atoms;
  const double *xn = a.ring_x + (size_t)(a.n % L) * row, *vn = a.ring_v + (size_t)(a.n % L) * row;
  double x1[3], v1[3];
  int sp[3];
  bool ok[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const long long j = j_lo + c * kCorrThreads + (int)threadIdx.x;
    ok[c] = j < j_hi;
    x1[c] = ok[c] ? xn[j] : 0.0;
    v1[c] = ok[c] ? vn[j] : 0.0;
    sp[c] = ok[c] ? a.species[j / 3] : -1;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n_k = (int)((long long)(k0 + kMdCorrLagTile - 1) <= kmax ? kMdCorrLagTile : kmax - k0 + 1);
  for (int kk = 0; kk < n_k; ++kk) {
    const size_t slot = (size_t)((a.n - (k0 + kk)) % L);
    const double *xo = a.ring_x + slot * row, *vo = a.ring_v + slot * row;
    double pv[3], px[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const long long j = j_lo + c * kCorrThreads + (int)threadIdx.x;
      const double x0 = ok[c] ? xo[j] : 0.0, v0 = ok[c] ? vo[j] : 0.0;
      const double d = x1[c] - x0;
      pv[c] = v1[c] * v0;
      px[c] = d * d;
    }
    for (int e = 0; e < E; ++e) {
      double tv = 0.0, tx = 0.0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        tv += sp[c] == e ? pv[c] : 0.0;
        tx += sp[c] == e ? px[c] : 0.0;
      }
      tv = wave_sum(tv);
      tx = wave_sum(tx);
      if (lane == 0) s_part[wave][0][e][kk] = tv, s_part[wave][1][e][kk] = tx;
    }
  }
  __syncthreads();
  // one thread per (which, e, kk): the waves in order, one partial of this chunk
  const int t = (int)threadIdx.x;
  if (t < 2 * E * kMdCorrLagTile) {
    const int kk = t % kMdCorrLagTile, e = (t / kMdCorrLagTile) % E, w = t / (kMdCorrLagTile * E);
    if (kk < n_k) {
      double sum = 0.0;
      for (int wv = 0; wv < kCorrWaves; ++wv) sum += s_part[wv][w][e][kk];
      a.part[(((size_t)blockIdx.x * 2 + w) * E + e) * L + (k0 + kk)] = sum;
    }
  }
}

// acc[f][e][k] += the partials of the frame's chunks, in chunk order; one thread per (f, e, k), k <= min(n, L - 1)
__global__ __launch_bounds__(256) void md_corr_add_kernel(MdCorrLaunch a) {
  if (md_stale(a.status, a.seq)) return;
  const int L = a.n_lags, E = a.n_elements;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)a.n_frames * E * L) return;
  const int k = (int)(idx % L), e = (int)((idx / L) % E), f = (int)(idx / ((long long)L * E));
  if ((long long)k > a.n) return;
  double sv = 0.0, sx = 0.0;
  for (int b = a.blk_start[f]; b < a.blk_start[f + 1]; ++b) {
    sv += a.part[(((size_t)b * 2 + 0) * E + e) * L + k];
    sx += a.part[(((size_t)b * 2 + 1) * E + e) * L + k];
  }
  a.acc_v[idx] += sv;
  a.acc_x[idx] += sx;
}

}  // namespace

void launch_md_correlate(const MdCorrLaunch &a, hipStream_t s) {
  if (a.n_chunks <= 0 || a.n_lags <= 0 || a.n < 0) return;
  const long long lags = a.n < (long long)a.n_lags ? a.n + 1 : (long long)a.n_lags;  // the rows the ring holds
  const unsigned tiles = (unsigned)((lags + kMdCorrLagTile - 1) / kMdCorrLagTile);
  hipLaunchKernelGGL(md_corr_kernel, dim3((unsigned)a.n_chunks, tiles), dim3(kCorrThreads), 0, s, a);
  const long long n_acc = (long long)a.n_frames * a.n_elements * a.n_lags;
  hipLaunchKernelGGL(md_corr_add_kernel, dim3((unsigned)((n_acc + 255) / 256)), dim3(256), 0, s, a);
}

}  // namespace ta
