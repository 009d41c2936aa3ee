// Temperature-dependent atomic head (TemperatureDependentAtomicNN, reference
// nn/atomic/finite_temperature.py:211-304; layers as convolution1x1, convolutional.py:257-290) on the
// fp64 matrix cores. For atom i of element e in frame f, T = T_f (eV):
//
//   x = minmax(G_i);  H = H_e(x) (linear output of width K, with bias);  z = [H, T]
//   U_i = U_e(z);  s_i = S_e(z);  S_i = s_i T (algo "Sommerfeld") or s_i;  F_i = U_i - T S_i
//   dF/dz[:K] = dU/dz[:K] - T c ds/dz[:K],  c = T (Sommerfeld) or 1;  dF/dG = J_H(x)^T dF/dz[:K]
//
// F_i goes where the plain MLP's atomic energy goes (`eatom`) and dF/dG where dE/dG goes (`dEdG`), so
// the descriptor backward kernels, the force gather and the frame reduce give the forces, the virial
// and the frame total of F unchanged. U_i and S_i go to two buffers of their own.
//
// One workgroup owns 16 atoms of one element (all elements in one launch, blocks element after
// element as in mlp_all_kernel); every layer is an `mlp_tile_gemm` (v_mfma_f64_16x16x4f64). LDS:
//   A, B  [16][sP]  activations / deltas of whichever net runs (H, then U, then S, then H backward)
//   z     [16][sz]  [H, T, 0...] (input of U and S)
//   g     [16][sz]  dF/dz, accumulated by the U and S backward sweeps
//   da               act'(z) of every hidden layer at its own stride np + 2: H's first, then ONE region
//                    that U and then S use in turn (in LDS when it fits, else the global scratch slab)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>

#include "ta_device.h"
#include "ta_mlp_tile.h"

namespace ta {

struct TdTiles {
  int32_t tile_start[kMaxElements + 1];  // first block of every element
  int32_t elem_start[kMaxElements + 1];  // first entry of every element in `atoms`
  int nel;
};

struct TdShape {
  int sP, sz;        // row strides of A / B and of z / g
  int K;             // width of H's output
  int da_h;          // doubles of H's act' region (per tile); U / S follow behind it
  int da_tile;       // doubles of the whole act' region per tile
  int act_h, act;    // activations of H and of U / S
  int sommerfeld;
};

namespace {

constexpr size_t kTdLdsLimit = 150 * 1024;

// doubles of act' storage of one net: one [16][np + 2] block per hidden layer
__host__ __device__ inline int td_da_doubles(const MlpDev &net) {
  int n = 0;
  for (int l = 0; l < net.n_layers; ++l)
    if (net.layer[l].act) n += kMlpRows * (net.layer[l].np + 2);
  return n;
}

// Forward through `net` from X ([16][sx], zero padded to layer 0's kp). Hidden layers park act'(z) in
// `da`; rows >= nrows give 0. Returns the buffer (A or B, stride sP) that holds the output layer.
__device__ __forceinline__ double *td_forward(const MlpDev &net, int act, const double *X, int sx, double *A,
                                              double *B, int sP, double *da, int nrows, int lane, int wave,
                                              int nwaves) {
  const double *cur = X;
  int scur = sx;
  double *out = A;
  for (int l = 0; l < net.n_layers; ++l) {
    const MlpLayerDev ly = net.layer[l];
    double *dst = (cur == A) ? B : A;
    const int sd = ly.np + 2;
    mlp_tile_gemm<16>(cur, scur, ly.w, ly.np, ly.kp, ly.np, ly.b, lane, wave, nwaves,
                      [&](int row, int col, double z) {
                        double h = 0.0, dh = 0.0;
                        if (row < nrows) {
                          h = z;
                          dh = 1.0;
                          if (ly.act) activation_fn(act, z, h, dh);
                          if (ly.res) h += cur[row * scur + col];  // convolutional.py:272-273
                        }
                        dst[row * sP + col] = h;
                        if (ly.act) da[row * sd + col] = dh;
                      });
    __syncthreads();
    if (ly.act) da += kMlpRows * sd;
    cur = dst;
    scur = sP;
    out = dst;
  }
  return out;
}

// Backward through `net`: on entry `cur` ([16][sP], one of A / B) holds the seed d(out)/d(net output)
// over the output layer's np columns. Layers L-1 .. 1 run in LDS (ping-pong with `other`); layer 0's
// GEMM hands delta_in[row][col] (col < layer 0's kp) to `emit0`.
template <typename Emit>
__device__ __forceinline__ void td_backward(const MlpDev &net, double *cur, double *other, int sP,
                                            const double *da, int lane, int wave, int nwaves, Emit emit0) {
  const int tid = threadIdx.x, nthreads = blockDim.x;
  int off[kMaxLayers];
  {
    int o = 0;
    for (int l = 0; l < net.n_layers; ++l) {
      off[l] = o;
      if (net.layer[l].act) o += kMlpRows * (net.layer[l].np + 2);
    }
  }
  for (int l = net.n_layers - 1; l >= 0; --l) {
    const MlpLayerDev ly = net.layer[l];
    const double *dal = da + off[l];
    const int sd = ly.np + 2;
    if (ly.res)  // keep delta for the skip connection
      for (int idx = tid; idx < kMlpRows * ly.np; idx += nthreads) {
        const int row = idx / ly.np, col = idx - row * ly.np;
        other[row * sP + col] = cur[row * sP + col];
      }
    if (ly.act)
      for (int idx = tid; idx < kMlpRows * ly.np; idx += nthreads) {
        const int row = idx / ly.np, col = idx - row * ly.np;
        cur[row * sP + col] *= dal[row * sd + col];
      }
    __syncthreads();
    if (l > 0) {
      const bool res = ly.res != 0;
      mlp_tile_gemm<16>(cur, sP, ly.wt, ly.kp, ly.np, ly.kp, nullptr, lane, wave, nwaves,
                        [&](int row, int col, double z) {
                          other[row * sP + col] = z + (res ? other[row * sP + col] : 0.0);
                        });
      __syncthreads();
      double *t = cur;
      cur = other;
      other = t;
    } else {
      mlp_tile_gemm<16>(cur, sP, ly.wt, ly.kp, ly.np, ly.kp, nullptr, lane, wave, nwaves, emit0);
      __syncthreads();
    }
  }
}

// seed of a scalar output: 1 in column 0 of the (padded) output layer
__device__ __forceinline__ void td_unit_seed(double *buf, int sP, int np) {
  for (int idx = threadIdx.x; idx < kMlpRows * np; idx += blockDim.x) {
    const int row = idx / np, col = idx - row * np;
    buf[row * sP + col] = (col == 0) ? 1.0 : 0.0;
  }
  __syncthreads();
}

// nets: [H[0..nel) | U[0..nel) | S[0..nel)]
template <int THREADS>
__global__ __launch_bounds__(THREADS) void td_all_kernel(const MlpDev *__restrict__ nets, TdTiles tiles, TdShape sh,
                                                         int ndim, const int32_t *__restrict__ atoms,
                                                         const int32_t *__restrict__ frame_of_atom,
                                                         const double *__restrict__ T, const double *__restrict__ G,
                                                         double *__restrict__ dEdG, double *__restrict__ eatom,
                                                         double *__restrict__ u_atom, double *__restrict__ s_atom,
                                                         double *scratch) {
  extern __shared__ double lds[];
  __shared__ double rowT[kMlpRows], rowU[kMlpRows], rowS[kMlpRows];
  const int sP = sh.sP, sz = sh.sz, K = sh.K;
  double *A = lds, *B = A + kMlpRows * sP, *zb = B + kMlpRows * sP, *gb = zb + kMlpRows * sz;
  double *da = scratch ? scratch + (size_t)blockIdx.x * sh.da_tile : gb + kMlpRows * sz;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = THREADS / 64;

  int e = 0;
  while (e + 1 < tiles.nel && (int)blockIdx.x >= tiles.tile_start[e + 1]) ++e;
  const int nel = tiles.nel;
  const MlpDev &H = nets[e], &U = nets[nel + e], &S = nets[2 * nel + e];
  const int32_t *el_atoms = atoms + tiles.elem_start[e];
  const int n_atoms = tiles.elem_start[e + 1] - tiles.elem_start[e];
  const int a0 = ((int)blockIdx.x - tiles.tile_start[e]) * kMlpRows;
  const int nrows = min(kMlpRows, n_atoms - a0);

  // 1. H input: min-max scaled descriptors, zero padded (as mlp_tile); the rows' temperatures
  const int kp0 = H.layer[0].kp;
  for (int idx = tid; idx < kMlpRows * kp0; idx += THREADS) {
    const int row = idx / kp0, k = idx - row * kp0;
    double x = 0.0;
    if (row < nrows && k < ndim) {
      x = G[(size_t)el_atoms[a0 + row] * ndim + k];
      if (H.xlo) {
        const double den = H.xhi[k] - H.xlo[k];
        x = (den != 0.0) ? (H.xhi[k] - x) / den : 0.0;  // div_no_nan, atomic.py:195
      }
    }
    A[row * sP + k] = x;
  }
  if (tid < kMlpRows) rowT[tid] = tid < nrows ? T[frame_of_atom[el_atoms[a0 + tid]]] : 0.0;
  __syncthreads();

  // 2. H forward, then z = [H, T] zero padded to U's (= S's) first-layer kp
  const double *hout = td_forward(H, sh.act_h, A, sP, A, B, sP, da, nrows, lane, wave, nwaves);
  const int zp = U.layer[0].kp;
  for (int idx = tid; idx < kMlpRows * zp; idx += THREADS) {
    const int row = idx / zp, k = idx - row * zp;
    double v = 0.0;
    if (k < K) v = hout[row * sP + k];
    else if (k == K) v = rowT[row];  // _add_electron_temperature, finite_temperature.py:94-118
    zb[row * sz + k] = v;
  }
  __syncthreads();

  double *dan = da + sh.da_h;
  // 3. U forward and backward to z: g = dU/dz
  {
    double *uo = td_forward(U, sh.act, zb, sz, A, B, sP, dan, nrows, lane, wave, nwaves);
    if (tid < kMlpRows) rowU[tid] = uo[tid * sP];
    __syncthreads();
    td_unit_seed(uo, sP, U.layer[U.n_layers - 1].np);
    td_backward(U, uo, uo == A ? B : A, sP, dan, lane, wave, nwaves,
                [&](int row, int col, double v) { gb[row * sz + col] = v; });
  }
  // 4. S forward and backward to z (same act' region): g -= T c ds/dz
  {
    double *so = td_forward(S, sh.act, zb, sz, A, B, sP, dan, nrows, lane, wave, nwaves);
    if (tid < kMlpRows) rowS[tid] = so[tid * sP];
    __syncthreads();
    td_unit_seed(so, sP, S.layer[S.n_layers - 1].np);
    const int somm = sh.sommerfeld;
    td_backward(S, so, so == A ? B : A, sP, dan, lane, wave, nwaves, [&](int row, int col, double v) {
      const double t = rowT[row];
      gb[row * sz + col] -= (somm ? t * t : t) * v;
    });
  }
  // 5. H backward from the vector seed dF/dz[:K] (H's output layer is linear: no act', no skip)
  const int npH = H.layer[H.n_layers - 1].np;
  for (int idx = tid; idx < kMlpRows * npH; idx += THREADS) {
    const int row = idx / npH, col = idx - row * npH;
    A[row * sP + col] = col < K ? gb[row * sz + col] : 0.0;
  }
  __syncthreads();
  td_backward(H, A, B, sP, da, lane, wave, nwaves, [&](int row, int k, double d) {
    if (row >= nrows || k >= ndim) return;
    if (H.xlo) {
      const double den = H.xhi[k] - H.xlo[k];
      d = (den != 0.0) ? -d / den : 0.0;
    }
    dEdG[(size_t)el_atoms[a0 + row] * ndim + k] = d;
  });

  // 6. per-atom U, S and F = U - T S
  if (tid < nrows) {
    const int atom = el_atoms[a0 + tid];
    const double t = rowT[tid], u = rowU[tid];
    const double s = sh.sommerfeld ? rowS[tid] * t : rowS[tid];
    u_atom[atom] = u;
    s_atom[atom] = s;
    eatom[atom] = u - t * s;
  }
}

// more than 64 KB of dynamic LDS needs the attribute; set once per kernel and device
template <typename Kern>
void td_allow_lds(Kern kernel, size_t bytes) {
  if (bytes <= 64 * 1024) return;
  static std::mutex mu;
  static std::map<std::pair<const void *, int>, bool> done;
  int dev = 0;
  (void)hipGetDevice(&dev);
  const auto key = std::make_pair(reinterpret_cast<const void *>(kernel), dev);
  std::lock_guard<std::mutex> lock(mu);
  if (done.count(key)) return;
  if (hipFuncSetAttribute(key.first, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTdLdsLimit) != hipSuccess)
    throw std::runtime_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
  done[key] = true;
}

struct TdPlan {
  TdShape sh;
  size_t lds_bytes;  // dynamic LDS of one workgroup
  bool da_in_lds;
  int threads;
};

TdPlan td_plan(const MlpDev *nets, int nel, int K, int act_h, int act, int sommerfeld, bool da_global) {
  TdPlan p;
  int w = 0, wz = 0, dah = 0, dan = 0, widest = 0;
  for (int e = 0; e < nel; ++e) {
    const MlpDev &h = nets[e];
    w = std::max(w, std::max(h.max_kp, h.max_np));
    dah = std::max(dah, td_da_doubles(h));
    for (int q = 1; q <= 2; ++q) {
      const MlpDev &n = nets[q * nel + e];
      wz = std::max(wz, n.layer[0].kp);
      for (int l = 0; l < n.n_layers; ++l) {
        w = std::max(w, n.layer[l].np);
        if (l > 0) w = std::max(w, n.layer[l].kp);
      }
      dan = std::max(dan, td_da_doubles(n));
    }
    widest = std::max(widest, std::max(h.max_np, std::max(nets[nel + e].max_np, nets[2 * nel + e].max_np)));
  }
  p.sh.sP = w + 2;
  p.sh.sz = wz + 2;
  p.sh.K = K;
  p.sh.da_h = dah;
  p.sh.da_tile = dah + dan;
  p.sh.act_h = act_h;
  p.sh.act = act;
  p.sh.sommerfeld = sommerfeld;
  const size_t base = (size_t)2 * kMlpRows * (p.sh.sP + p.sh.sz) * sizeof(double);
  const size_t with_da = base + (size_t)p.sh.da_tile * sizeof(double);
  p.da_in_lds = with_da <= kTdLdsLimit && !da_global;
  p.lds_bytes = p.da_in_lds ? with_da : base;
  if (p.lds_bytes > kTdLdsLimit)
    throw std::domain_error("finite-temperature network too wide for the LDS tile: " + std::to_string(p.lds_bytes) +
                            " B of LDS per workgroup, limit " + std::to_string(kTdLdsLimit));
  p.threads = widest >= 128 ? 512 : 256;
  return p;
}

}  // namespace

// global scratch doubles a launch over this batch needs (0 when the act' region fits in LDS)
size_t td_scratch_doubles(const MlpDev *nets, int nel, int K, const int32_t *elem_start, bool da_global) {
  const TdPlan p = td_plan(nets, nel, K, 0, 0, 0, da_global);
  if (p.da_in_lds) return 0;
  size_t tiles = 0;
  for (int e = 0; e < nel; ++e) tiles += (size_t)(elem_start[e + 1] - elem_start[e] + kMlpRows - 1) / kMlpRows;
  return tiles * (size_t)p.sh.da_tile;
}

// `nets_dev`: device copy of `nets_host[0 .. 3 nel)`; T [n_frames], u_atom / s_atom [N]; da_global: Options::mlp_da_global
void launch_td_all(const MlpDev *nets_dev, const MlpDev *nets_host, int nel, int K, int act_h, int act,
                   int sommerfeld, int ndim, const DeviceBatch &b, bool da_global, const double *T, double *u_atom,
                   double *s_atom, double *scratch, hipStream_t s, MlpLaunchInfo *info) {
  if (info) *info = MlpLaunchInfo{};
  TdTiles t;
  t.nel = nel;
  int blocks = 0;
  for (int e = 0; e < nel; ++e) {
    t.tile_start[e] = blocks;
    t.elem_start[e] = b.elem_start[e];
    blocks += (b.elem_start[e + 1] - b.elem_start[e] + kMlpRows - 1) / kMlpRows;
  }
  t.tile_start[nel] = blocks;
  t.elem_start[nel] = b.elem_start[nel];
  for (int e = nel + 1; e <= kMaxElements; ++e) t.tile_start[e] = t.elem_start[e] = 0;
  if (blocks == 0) return;
  const TdPlan p = td_plan(nets_host, nel, K, act_h, act, sommerfeld, da_global);
  if (p.da_in_lds) scratch = nullptr;
  else if (!scratch) throw std::runtime_error("finite-temperature head: scratch slab missing");
  if (info)
    *info = MlpLaunchInfo{TA_MLP_TD, p.threads, 0, 0, blocks, 1, (long long)p.lds_bytes,
                          p.da_in_lds ? TA_MLP_DA_LDS : TA_MLP_DA_GLOBAL};
  auto go = [&](auto kernel, int threads) {
    td_allow_lds(kernel, p.lds_bytes);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(threads), p.lds_bytes, s, nets_dev, t, p.sh, ndim,
                       b.elem_atoms, b.frame_of_atom, T, b.G, b.dEdG, b.eatom, u_atom, s_atom, scratch);
  };
  if (p.threads == 512) go(td_all_kernel<512>, 512);
  else go(td_all_kernel<256>, 256);
}

}  // namespace ta
