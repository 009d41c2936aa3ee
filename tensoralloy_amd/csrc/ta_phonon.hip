// Harmonic phonons on the device (ta_phonon_*): dynamical matrices of a batch of q-points from the force-constant
// rows of the home cell, a batched Hermitian eigensolver, and the phonon density of states. All fp64.
//
// 1. phonon_dynmat_kernel. One thread per (q, b, b'). With r running over the shortest vectors from home atom b to
//    the periodic images of supercell atom s (phonopy's convention: every image within a tolerance of the minimum,
//    each weighted 1 / multiplicity; the lists are the host's),
//        D[q][3b+a][3b'+c] = (m_b m_b')^(-1/2) sum_{s: basis_of[s] = b'} Phi_ac(b, s) (1/mult) sum_r exp(i q.r)
//    s and r ascend: one thread owns an entry, the order is fixed and there is no atomic. The phase q.r goes to
//    sincos() as it is: the device routine reduces its argument itself (to ~1 ulp of the result at any magnitude),
//    so the only error that grows with |q.r| is the rounding of the product, eps |q.r|, which every fp64
//    evaluation of exp(i q.r) from Cartesian q and r shares. (ta_md_sq.hip reduces first because there the phase
//    is 2 pi n.s with an integer n, where the reduction is exact. Here nothing exact is at hand.)
//
// 2. phonon_eigh_kernel. Cyclic Jacobi on the Hermitian part of each matrix, in LDS, in the round-robin (Brent-Luk)
//    ordering: np = n rounded up to even players, np - 1 rounds per sweep, np / 2 disjoint rotations per round; the
//    player an odd n is padded with is a decoupled row, its rotations are skipped. A round is three phases with a
//    barrier behind each: (1) a thread per pair forms the rotation that zeroes A[p][q], (2) A <- A J and V <- V J, a
//    thread per (pair, row), (3) A <- J^H A, a thread per (pair, column); the rotated entry is then set to zero and
//    the diagonal made real explicitly. Before every sweep the off-diagonal Frobenius norm is formed in a fixed
//    order; a matrix is done when it is <= n eps ||A||_F and is counted in `info` if kPhononSweepCap sweeps did not
//    get it there. Eigenvalues leave in ascending order (rank by counting, ties by index), eigenvectors with them.
//
//    LDS layout: split complex. A matrix is two planes of doubles (real, imaginary), V two more, row-major with
//    the row stride ld = n | 1 doubles. Interleaved 16-byte elements at stride n would put the lanes of a column
//    access (phase 2: lane = row) on stride 4 n dwords, a 2- to 16-way conflict for even n; with 8-byte elements
//    and an odd stride the 32 lanes of a ds_read_b64 group hit 32 distinct double-wide banks, and a row access
//    (phase 3: lane = column) is contiguous. n = 48 with vectors: 4 x 48 x 49 x 8 B = 75 KB, one matrix per
//    workgroup of 256 threads. Small matrices share a workgroup: a matrix gets the power of two of threads that
//    covers its (np / 2) n work items (at least 8), so a workgroup solves 32 matrices of order 3 at a time.
//
// 3. phonon_dos_kernel + phonon_dos_sum_kernel. A workgroup takes a slab of kPhononDosSlab consecutive q-points,
//    whatever the host's chunking. nu = sign(l) sqrt(|l|) factor, k = floor((nu - nu_min) * inv_dnu): a
//    subtraction, then a multiplication, nothing an FMA can contract. Total counts: LDS integer atomics, then
//    64-bit integer atomics to HBM. Per-atom weights sum_a |e_ba|^2: thread t owns the bins k = t mod 256, walks
//    the slab's modes in index order and adds the weights of the modes in its bins to the slab's own row, plain
//    read-add-write; the sum kernel then adds the slabs in index order to the running row. Since slabs do not
//    depend on the chunking, chunked and unchunked runs give the same bits.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <map>
#include <mutex>
#include <stdexcept>

#include "ta_phonon.h"

namespace ta {
namespace {

constexpr int kThreads = 256;
constexpr int kLdsLimit = 160 * 1024 - 1024;  // (room for the kernel's static words)

__device__ __forceinline__ double phonon_nu(double lam, double factor) { return copysign(sqrt(fabs(lam)) * factor, lam); }

__global__ __launch_bounds__(kThreads) void phonon_dynmat_kernel(PhononDynmatLaunch a) {
  const int nb = a.n_basis, N = a.N, n = 3 * nb;
  const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= a.Q * nb * nb) return;
  const int bp = (int)(idx % nb), b = (int)((idx / nb) % nb);
  const long long qi = idx / ((long long)nb * nb);
  const double qx = a.q[3 * qi], qy = a.q[3 * qi + 1], qz = a.q[3 * qi + 2];
  double re[9], im[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) re[c] = im[c] = 0.0;
  for (int s = 0; s < N; ++s) {
    if (a.basis_of[s] != bp) continue;
    const int lo = a.start[(size_t)b * N + s], hi = a.start[(size_t)b * N + s + 1];
    if (hi <= lo) continue;
    double pr = 0.0, pi = 0.0;
    for (int v = lo; v < hi; ++v) {
      const double x = qx * a.vec[3 * (size_t)v] + qy * a.vec[3 * (size_t)v + 1] + qz * a.vec[3 * (size_t)v + 2];
      double sn, cs;
      sincos(x, &sn, &cs);
      pr += cs;
      pi += sn;
    }
    const double wt = 1.0 / (double)(hi - lo);
    pr *= wt;
    pi *= wt;
    const double *phi = a.phi + ((size_t)b * N + s) * 9;
#pragma unroll
    for (int c = 0; c < 9; ++c) re[c] += phi[c] * pr, im[c] += phi[c] * pi;
  }
  const double scale = 1.0 / sqrt(a.mass[b] * a.mass[bp]);
  double *D = a.D + (size_t)qi * n * n * 2;
#pragma unroll
  for (int c = 0; c < 9; ++c) {
    const size_t e = (size_t)(3 * b + c / 3) * n + (3 * bp + c % 3);
    D[2 * e] = re[c] * scale;
    D[2 * e + 1] = im[c] * scale;
  }
}

// shape of the solver's launch for order n
struct EighPlan {
  int np, ld, tpm, mpb, per_matrix;  // players, row stride, threads per matrix, matrices per block, doubles per matrix
};

EighPlan eigh_plan(int n, bool vectors) {
  EighPlan p;
  p.np = n < 2 ? 2 : n + (n & 1);
  p.ld = n | 1;
  const int items = (p.np / 2) * n;
  int tpm = 8;
  while (tpm < items && tpm < kThreads) tpm *= 2;
  p.tpm = tpm;
  p.mpb = kThreads / tpm;
  // planes, rotations (c, s.re, s.im per pair), row sums, then n ranks and the done flag as ints
  p.per_matrix = (vectors ? 4 : 2) * n * p.ld + 3 * (p.np / 2) + n + (n + 2 + 1) / 2;
  return p;
}

// pair k of round r among np players (np even): player np - 1 stays, the others go round
__device__ __forceinline__ void round_robin_pair(int k, int r, int np, int &p, int &q) {
  const int m = np - 1;
  int x, y;
  if (k == 0) {
    x = m, y = r;
  } else {
    x = (r + k) % m, y = (r - k + m) % m;
  }
  p = x < y ? x : y;
  q = x < y ? y : x;
}

template <bool kVec>
__global__ __launch_bounds__(kThreads) void phonon_eigh_kernel(PhononEighLaunch a, EighPlan pl) {
  extern __shared__ double s_mem[];
  const int n = a.n, np = pl.np, ld = pl.ld, tpm = pl.tpm, half = np / 2, plane = n * ld;
  const int slot = (int)threadIdx.x / tpm, t = (int)threadIdx.x % tpm;
  const long long mat = (long long)blockIdx.x * pl.mpb + slot;
  const bool live = mat < a.batch;
  double *Are = s_mem + (size_t)slot * pl.per_matrix, *Aim = Are + plane;
  double *Vre = Aim + plane, *Vim = Vre + (kVec ? plane : 0);
  double *rot = Are + (kVec ? 4 : 2) * plane, *red = rot + 3 * half;
  int *rank = reinterpret_cast<int *>(red + n), *flag = rank + n;
  if (live) {
    const double *A = a.A + (size_t)mat * n * n * 2;
    for (int e = t; e < n * n; e += tpm) {
      const int i = e / n, j = e % n;
      const size_t ij = (size_t)i * n + j, ji = (size_t)j * n + i;
      Are[i * ld + j] = 0.5 * (A[2 * ij] + A[2 * ji]);
      Aim[i * ld + j] = 0.5 * (A[2 * ij + 1] - A[2 * ji + 1]);
      if constexpr (kVec) Vre[i * ld + j] = i == j ? 1.0 : 0.0, Vim[i * ld + j] = 0.0;
    }
  }
  __syncthreads();
  if (live)
    for (int i = t; i < n; i += tpm) {
      double sum = 0.0;
      for (int j = 0; j < n; ++j) sum += Are[i * ld + j] * Are[i * ld + j] + Aim[i * ld + j] * Aim[i * ld + j];
      red[i] = sum;
    }
  __syncthreads();
  double thr = 0.0;  // (thread 0 of the matrix)
  if (live && t == 0) {
    double sum = 0.0;
    for (int i = 0; i < n; ++i) sum += red[i];
    thr = (double)n * DBL_EPSILON * sqrt(sum);
  }
  if (t == 0) flag[0] = live ? 0 : 1;
  for (int sweep = 0;; ++sweep) {
    __syncthreads();  // (red is free again, flag is written)
    if (live && !flag[0])
      for (int i = t; i < n; i += tpm) {
        double sum = 0.0;
        for (int j = 0; j < n; ++j)
          if (j != i) sum += Are[i * ld + j] * Are[i * ld + j] + Aim[i * ld + j] * Aim[i * ld + j];
        red[i] = sum;
      }
    __syncthreads();
    if (live && t == 0 && !flag[0]) {
      double sum = 0.0;
      for (int i = 0; i < n; ++i) sum += red[i];
      if (sqrt(sum) <= thr) flag[0] = 1;
    }
    __syncthreads();
    const bool active = live && !flag[0];
    if (!__syncthreads_or(active ? 1 : 0)) break;
    if (sweep == kPhononSweepCap) {
      if (active && t == 0) atomicAdd(a.info, 1ull);
      break;
    }
    for (int r = 0; r < np - 1; ++r) {
      if (active)
        for (int k = t; k < half; k += tpm) {
          int p, q;
          round_robin_pair(k, r, np, p, q);
          double c = 1.0, sr = 0.0, si = 0.0;
          if (q < n) {
            const double br = Are[p * ld + q], bi = Aim[p * ld + q], ab = hypot(br, bi);
            if (ab > 0.0) {
              const double tau = (Are[q * ld + q] - Are[p * ld + p]) / (2.0 * ab);
              const double tt = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
              c = 1.0 / sqrt(1.0 + tt * tt);
              const double s = tt * c;
              sr = s * (br / ab), si = s * (bi / ab);
            }
          }
          rot[3 * k] = c, rot[3 * k + 1] = sr, rot[3 * k + 2] = si;
        }
      __syncthreads();
      if (active)
        for (int id = t; id < half * n; id += tpm) {  // A <- A J, V <- V J: lane = row
          const int k = id / n, i = id % n;
          const double c = rot[3 * k], sr = rot[3 * k + 1], si = rot[3 * k + 2];
          if (sr == 0.0 && si == 0.0) continue;
          int p, q;
          round_robin_pair(k, r, np, p, q);
          {
            const double xr = Are[i * ld + p], xi = Aim[i * ld + p], yr = Are[i * ld + q], yi = Aim[i * ld + q];
            Are[i * ld + p] = c * xr - (sr * yr + si * yi);
            Aim[i * ld + p] = c * xi - (sr * yi - si * yr);
            Are[i * ld + q] = (sr * xr - si * xi) + c * yr;
            Aim[i * ld + q] = (sr * xi + si * xr) + c * yi;
          }
          if constexpr (kVec) {
            const double xr = Vre[i * ld + p], xi = Vim[i * ld + p], yr = Vre[i * ld + q], yi = Vim[i * ld + q];
            Vre[i * ld + p] = c * xr - (sr * yr + si * yi);
            Vim[i * ld + p] = c * xi - (sr * yi - si * yr);
            Vre[i * ld + q] = (sr * xr - si * xi) + c * yr;
            Vim[i * ld + q] = (sr * xi + si * xr) + c * yi;
          }
        }
      __syncthreads();
      if (active)
        for (int id = t; id < half * n; id += tpm) {  // A <- J^H A: lane = column
          const int k = id / n, j = id % n;
          const double c = rot[3 * k], sr = rot[3 * k + 1], si = rot[3 * k + 2];
          if (sr == 0.0 && si == 0.0) continue;
          int p, q;
          round_robin_pair(k, r, np, p, q);
          const double xr = Are[p * ld + j], xi = Aim[p * ld + j], yr = Are[q * ld + j], yi = Aim[q * ld + j];
          double pr = c * xr - (sr * yr - si * yi), pi = c * xi - (sr * yi + si * yr);
          double qr = (sr * xr + si * xi) + c * yr, qi = (sr * xi - si * xr) + c * yi;
          if (j == q) pr = 0.0, pi = 0.0, qi = 0.0;  // the entry the rotation zeroes; a real diagonal
          if (j == p) qr = 0.0, qi = 0.0, pi = 0.0;
          Are[p * ld + j] = pr, Aim[p * ld + j] = pi;
          Are[q * ld + j] = qr, Aim[q * ld + j] = qi;
        }
      __syncthreads();
    }
  }
  // (every thread of the block left the loop behind the same barrier)
  if (live)
    for (int i = t; i < n; i += tpm) {
      const double d = Are[i * ld + i];
      int rk = 0;
      for (int j = 0; j < n; ++j) {
        const double e = Are[j * ld + j];
        rk += (e < d || (e == d && j < i)) ? 1 : 0;
      }
      rank[i] = rk;
      a.w[(size_t)mat * n + rk] = d;
    }
  if constexpr (kVec) {
    __syncthreads();
    if (live) {
      double *V = a.V + (size_t)mat * n * n * 2;
      for (int e = t; e < n * n; e += tpm) {
        const int m = e / n, i = e % n;
        const size_t o = (size_t)rank[m] * n + i;
        V[2 * o] = Vre[i * ld + m];
        V[2 * o + 1] = Vim[i * ld + m];
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void phonon_frequency_kernel(const double *w, double *nu, long long n, double factor) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) nu[i] = phonon_nu(w[i], factor);
}

__global__ __launch_bounds__(kThreads) void phonon_phi_kernel(const double *raw, double *phi, int n_basis, int N) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (long long)n_basis * N * 9) return;
  const int c = (int)(i % 3), al = (int)((i / 3) % 3), s = (int)((i / 9) % N), b = (int)(i / (9ll * N));
  phi[i] = -raw[((size_t)(3 * b + al) * N + s) * 3 + c];
}

__global__ __launch_bounds__(kThreads) void phonon_dos_kernel(PhononDosLaunch a) {
  extern __shared__ unsigned s_words[];  // [n_bins] counts, then [kPhononDosSlab n] bins, then the outside count
  unsigned *s_hist = s_words;
  int *s_bin = reinterpret_cast<int *>(s_words + a.n_bins);
  unsigned *s_out = s_words + a.n_bins + kPhononDosSlab * a.n;
  const int t = (int)threadIdx.x, n = a.n, B = a.n_bins, nb = n / 3;
  const long long q0 = (long long)blockIdx.x * kPhononDosSlab;
  const int nq = (int)(a.Q - q0 < kPhononDosSlab ? a.Q - q0 : kPhononDosSlab), modes = nq * n;
  for (int k = t; k < B; k += kThreads) s_hist[k] = 0u;
  if (t == 0) *s_out = 0u;
  __syncthreads();
  for (int e = t; e < modes; e += kThreads) {
    const double nu = phonon_nu(a.w[(size_t)q0 * n + e], a.factor);
    const double d = nu - a.nu_min;
    const double x = d * a.inv_dnu;
    const int k = (x >= 0.0 && x < (double)B) ? (int)floor(x) : -1;  // (a NaN counts as outside)
    s_bin[e] = k;
    if (k >= 0) atomicAdd(&s_hist[k], 1u); else atomicAdd(s_out, 1u);
  }
  __syncthreads();
  for (int k = t; k < B; k += kThreads) {
    const unsigned c = s_hist[k];
    if (c != 0u) __hip_atomic_fetch_add(a.total + k, (unsigned long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (t == 0 && *s_out != 0u)
    __hip_atomic_fetch_add(a.info, (unsigned long long)*s_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (!a.slab_part) return;
  double *part = a.slab_part + (size_t)blockIdx.x * nb * B;
  for (int b = 0; b < nb; ++b)
    for (int k = t; k < B; k += kThreads) part[(size_t)b * B + k] = 0.0;
  for (int e = 0; e < modes; ++e) {  // thread t owns the bins k = t mod kThreads: mode order, no atomics
    const int k = s_bin[e];
    if (k < 0 || (k % kThreads) != t) continue;
    const double *v = a.V + ((size_t)q0 * n + e) * n * 2;
    for (int b = 0; b < nb; ++b) {
      double wgt = 0.0;
#pragma unroll
      for (int c = 0; c < 6; ++c) wgt += v[6 * b + c] * v[6 * b + c];
      part[(size_t)b * B + k] += wgt;
    }
  }
}

__global__ __launch_bounds__(kThreads) void phonon_dos_sum_kernel(const double *slab_part, double *partial, long long cells,
                                                                  int n_slabs) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= cells) return;
  double acc = partial[i];
  for (int sl = 0; sl < n_slabs; ++sl) acc += slab_part[(size_t)sl * cells + i];
  partial[i] = acc;
}

unsigned blocks_of(long long n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// more than 64 KB of dynamic LDS has to be asked for, per kernel and device: the launch's own amount (the kernel's
// static words count against the same 160 KB)
void allow_lds(const void *kernel, size_t bytes) {
  static std::mutex mu;
  static std::map<std::pair<const void *, int>, size_t> allowed;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) throw std::runtime_error("hipGetDevice failed");
  const auto key = std::make_pair(kernel, dev);
  std::lock_guard<std::mutex> lock(mu);
  auto it = allowed.find(key);
  if (it != allowed.end() && it->second >= bytes) return;
  if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
    throw std::runtime_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
  allowed[key] = bytes;
}

}  // namespace

int phonon_eigh_matrices_per_block(int n) { return eigh_plan(n, true).mpb; }

void launch_phonon_dynmat(const PhononDynmatLaunch &a, hipStream_t s) {
  const long long threads = a.Q * a.n_basis * a.n_basis;
  if (threads <= 0) return;
  hipLaunchKernelGGL(phonon_dynmat_kernel, dim3(blocks_of(threads)), dim3(kThreads), 0, s, a);
}

void launch_phonon_eigh(const PhononEighLaunch &a, hipStream_t s) {
  if (a.batch <= 0 || a.n <= 0) return;
  if (a.n > kPhononMaxOrder) throw std::invalid_argument("phonon eigensolver: order above TA_PHONON_MAX_ORDER");
  const bool vec = a.V != nullptr;
  const EighPlan pl = eigh_plan(a.n, vec);
  const size_t lds = (size_t)pl.mpb * pl.per_matrix * sizeof(double);
  if (lds > (size_t)kLdsLimit) throw std::invalid_argument("phonon eigensolver: the matrices do not fit the LDS");
  const unsigned grid = (unsigned)((a.batch + pl.mpb - 1) / pl.mpb);
  if (vec) {
    if (lds > 64 * 1024) allow_lds(reinterpret_cast<const void *>(phonon_eigh_kernel<true>), lds);
    hipLaunchKernelGGL(phonon_eigh_kernel<true>, dim3(grid), dim3(kThreads), lds, s, a, pl);
  } else {
    if (lds > 64 * 1024) allow_lds(reinterpret_cast<const void *>(phonon_eigh_kernel<false>), lds);
    hipLaunchKernelGGL(phonon_eigh_kernel<false>, dim3(grid), dim3(kThreads), lds, s, a, pl);
  }
}

void launch_phonon_frequencies(const double *w, double *nu, long long n, double factor, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(phonon_frequency_kernel, dim3(blocks_of(n)), dim3(kThreads), 0, s, w, nu, n, factor);
}

void launch_phonon_dos(const PhononDosLaunch &a, hipStream_t s) {
  if (a.Q <= 0 || a.n_bins <= 0) return;
  const int slabs = (int)((a.Q + kPhononDosSlab - 1) / kPhononDosSlab);
  const size_t lds = ((size_t)a.n_bins + (size_t)kPhononDosSlab * a.n + 1) * sizeof(unsigned);
  hipLaunchKernelGGL(phonon_dos_kernel, dim3((unsigned)slabs), dim3(kThreads), lds, s, a);
  if (a.slab_part) {
    const long long cells = (long long)(a.n / 3) * a.n_bins;
    hipLaunchKernelGGL(phonon_dos_sum_kernel, dim3(blocks_of(cells)), dim3(kThreads), 0, s, a.slab_part, a.partial, cells,
                       slabs);
  }
}

void launch_phonon_phi_from_tangents(const double *raw, double *phi, int n_basis, int N, hipStream_t s) {
  const long long n = (long long)n_basis * N * 9;
  if (n <= 0) return;
  hipLaunchKernelGGL(phonon_phi_kernel, dim3(blocks_of(n)), dim3(kThreads), 0, s, raw, phi, n_basis, N);
}

}  // namespace ta
