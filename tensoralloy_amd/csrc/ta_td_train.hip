// Loss gradient of a temperature-dependent model (TemperatureDependentAtomicNN, reference
// nn/atomic/finite_temperature.py:211-388) with respect to the weights of its H, U and S nets.
//
// For atom i of element e in frame f, T = T_f, c = T (algo "Sommerfeld") or 1:
//   x = minmax(G_i),  H = H_e(x),  z = [H, T],  U = U_e(z),  s = S_e(z),  S = c s,  F = U - T c s.
// With per-frame coefficients a = dL/dU_f, b = dL/dF_f, g = dL/dS_f and the force / stress direction
// (dR, dh) of F (ta_train.hip: D_delta F = sum_atoms dF/dG . dG), the gradient is
//   d/dtheta [ sum_f (a U_f + b F_f + g S_f) + D_delta F ],   D_delta F = sum_i (dU/dz - T c ds/dz) . z'_i,
//   z' = [J_H(x) x', 0],  x' = minmax'(G) dG_i   (T carries no tangent).
// Per tile of 16 atoms of one element, the forward-over-reverse sweep of mlp_grad2_kernel runs on each
// net in turn:
//   1. H forward with its tangent: z and z';
//   2. U and S forward from (z, z');
//   3. U reverse with seeds kappa = a + b, nu = 1; S reverse with kappa = c (g - T b), nu = -T c. Both
//      give dtheta of their net, and their input adjoints (kappa_z, nu_z) are summed;
//   4. H reverse from the vector seeds (kappa_z, nu_z)[:K] (the T column dropped): dtheta_H.
// Per layer of every net the forward parks x, x', a'(z) and a''(z) z' in the workgroup's slab of a
// global scratch buffer (LDS holds only the ping-pong activations and z, z'). Weight gradients are
// 16 x 16 x 4 MFMA tiles (K = the 16 rows) added into the workgroup's slice of a partial buffer, which
// ta_train.hip's grad_reduce_kernel sums in a fixed order: no atomics, bitwise reproducible.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>

#include "ta_device.h"
#include "ta_launch.h"
#include "ta_mlp_tile.h"

namespace ta {

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;  // persistent workgroups, as mlp_grad2_kernel
constexpr size_t kLdsLimit = 150 * 1024;

struct TdGradTiles {
  int32_t tile_start[kMaxElements + 1];  // first tile of every element
  int32_t elem_start[kMaxElements + 1];  // first entry of every element in `atoms`
  int32_t net_off[3 * kMaxElements];     // first parameter of net q * nel + el in the flat vector
  int nel, n_params;
};

struct TdGradShape {
  int sP, sz;         // row strides of the ping-pong buffers and of z / z'
  int K;              // width of H's output
  int act_h, act;     // activations of H and of U / S
  int sommerfeld;
  size_t slab_wg;     // scratch doubles of one workgroup
};

// Forward with tangent through `net` (mlp_grad2_kernel's sweep). Input (X, Xt) at stride `sx`, zero
// padded to layer 0's kp; `sc` = [x | x' | a' | a'' z'] x L slabs of [16][sP]. Rows >= nrows give 0.
// Returns the buffer pair (one of X0 / X1, T0 / T1) that holds the output layer.
__device__ __forceinline__ void tdg_forward(const MlpDev &net, int act, const double *X, const double *Xt, int sx,
                                            double *X0, double *X1, double *T0, double *T1, int sP, double *sc,
                                            int nrows, int lane, int wave, int nwaves, double *&outX,
                                            double *&outT) {
  const int tid = threadIdx.x, L = net.n_layers;
  const size_t slab = (size_t)kMlpRows * sP;
  double *xs = sc, *ts = sc + L * slab, *da = sc + 2 * L * slab, *dd = sc + 3 * L * slab;
  const double *curX = X, *curT = Xt;
  int scur = sx;
  double *nxtX = X0, *nxtT = T0;
  for (int l = 0; l < L; ++l) {
    const MlpLayerDev ly = net.layer[l];
    double *xl = xs + l * slab, *tl = ts + l * slab, *dal = da + l * slab, *ddl = dd + l * slab;
    for (int idx = tid; idx < kMlpRows * ly.kp; idx += kThreads) {
      const int row = idx / ly.kp, k = idx - row * ly.kp;
      xl[row * sP + k] = curX[row * scur + k];
      tl[row * sP + k] = curT[row * scur + k];
    }
    // z' first (parked in nxtT), then z with the activation applied to both
    mlp_tile_gemm<4>(curT, scur, ly.w, ly.np, ly.kp, ly.np, nullptr, lane, wave, nwaves,
                     [&](int row, int col, double zt) { nxtT[row * sP + col] = zt; });
    mlp_tile_gemm<4>(curX, scur, ly.w, ly.np, ly.kp, ly.np, ly.b, lane, wave, nwaves,
                     [&](int row, int col, double z) {
                       double h = 0.0, dh = 0.0, d2 = 0.0, ht = 0.0;
                       if (row < nrows) {
                         const double zt = nxtT[row * sP + col];  // written by this same lane
                         h = z;
                         dh = 1.0;
                         if (ly.act) activation_fn2(act, z, h, dh, d2);
                         ht = dh * zt;
                         d2 *= zt;
                         if (ly.res) {  // convolutional.py:272-273 (l > 0: cur is at stride sP)
                           h += curX[row * scur + col];
                           ht += curT[row * scur + col];
                         }
                       }
                       nxtX[row * sP + col] = h;
                       nxtT[row * sP + col] = ht;
                       dal[row * sP + col] = dh;
                       ddl[row * sP + col] = d2;
                     });
    __syncthreads();
    curX = nxtX;
    curT = nxtT;
    scur = sP;
    nxtX = (nxtX == X0) ? X1 : X0;
    nxtT = (nxtT == T0) ? T1 : T0;
  }
  outX = const_cast<double *>(curX);
  outT = const_cast<double *>(curT);
}

// Reverse sweep through `net`: on entry (curX, curT) hold the adjoints (kappa, nu) of the output layer
// over its np columns. Adds dW, db into `out` (the net's block of the workgroup's partial slice). With
// EMIT, layer 0's input adjoints go to emitX(row, col, v) / emitT(row, col, v) (col < layer 0's kp).
template <bool EMIT, typename EX, typename ET>
__device__ __forceinline__ void tdg_reverse(const MlpDev &net, double *curX, double *curT, double *nxtX,
                                            double *nxtT, int sP, const double *sc, double *out, int lane,
                                            int wave, int nwaves, EX emitX, ET emitT) {
  const int tid = threadIdx.x, L = net.n_layers, m16 = lane & 15, q4 = lane >> 4;
  const size_t slab = (size_t)kMlpRows * sP;
  const double *xs = sc, *ts = sc + L * slab, *da = sc + 2 * L * slab, *dd = sc + 3 * L * slab;
  int w_off[kMaxLayers];
  {
    int o = 0;
    for (int l = 0; l < L; ++l) {
      w_off[l] = o;
      o += net.layer[l].k * net.layer[l].n + net.layer[l].n;
    }
  }
  for (int l = L - 1; l >= 0; --l) {
    const MlpLayerDev ly = net.layer[l];
    const double *xl = xs + l * slab, *tl = ts + l * slab, *dal = da + l * slab, *ddl = dd + l * slab;
    if (ly.res)
      for (int idx = tid; idx < kMlpRows * ly.np; idx += kThreads) {
        const int row = idx / ly.np, col = idx - row * ly.np;
        nxtX[row * sP + col] = curX[row * sP + col];
        nxtT[row * sP + col] = curT[row * sP + col];
      }
    for (int idx = tid; idx < kMlpRows * ly.np; idx += kThreads) {
      const int row = idx / ly.np, col = idx - row * ly.np;
      const double kap = curX[row * sP + col], nu = curT[row * sP + col];
      curX[row * sP + col] = kap * dal[row * sP + col] + nu * ddl[row * sP + col];  // lambda
      curT[row * sP + col] = nu * dal[row * sP + col];                              // mu
    }
    __syncthreads();
    // dW[k][n] = sum_rows x[row][k] lambda[row][n] + x'[row][k] mu[row][n];  db[n] = sum_rows lambda[row][n]
    const int nkt = ly.kp / 16, nnt = ly.np / 16;
    double *ow = out + w_off[l], *ob = ow + ly.k * ly.n;
    for (int tile = wave; tile < nkt * nnt; tile += nwaves) {
      const int kt = tile / nnt, nt = tile - kt * nnt;
      mlp_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int row = 4 * s + q4;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xl[row * sP + 16 * kt + m16], curX[row * sP + 16 * nt + m16],
                                                   acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(tl[row * sP + 16 * kt + m16], curT[row * sP + 16 * nt + m16],
                                                   acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = 16 * kt + q4 + 4 * r, n = 16 * nt + m16;
        if (k < ly.k && n < ly.n) ow[k * ly.n + n] += acc[r];
      }
    }
    for (int n = tid; n < ly.n; n += kThreads) {
      double s = 0.0;
      for (int row = 0; row < kMlpRows; ++row) s += curX[row * sP + n];
      ob[n] += s;
    }
    if (l > 0) {
      // kappa_in = lambda W^T (+ kappa),  nu_in = mu W^T (+ nu)
      const bool res = ly.res != 0;
      double *dstX = nxtX, *dstT = nxtT;
      mlp_tile_gemm<4>(curX, sP, ly.wt, ly.kp, ly.np, ly.kp, nullptr, lane, wave, nwaves,
                       [&](int row, int col, double z) { dstX[row * sP + col] = z + (res ? dstX[row * sP + col] : 0.0); });
      mlp_tile_gemm<4>(curT, sP, ly.wt, ly.kp, ly.np, ly.kp, nullptr, lane, wave, nwaves,
                       [&](int row, int col, double z) { dstT[row * sP + col] = z + (res ? dstT[row * sP + col] : 0.0); });
      __syncthreads();
      double *t = curX; curX = nxtX; nxtX = t;
      t = curT; curT = nxtT; nxtT = t;
    } else if constexpr (EMIT) {
      mlp_tile_gemm<4>(curX, sP, ly.wt, ly.kp, ly.np, ly.kp, nullptr, lane, wave, nwaves, emitX);
      mlp_tile_gemm<4>(curT, sP, ly.wt, ly.kp, ly.np, ly.kp, nullptr, lane, wave, nwaves, emitT);
      __syncthreads();
    } else {
      __syncthreads();  // the next tile's input overwrites what the dW tiles read
    }
  }
}

__device__ __forceinline__ void tdg_seed(double *X, double *Xt, int sP, int np, const double *kap,
                                         const double *nu) {
  for (int idx = threadIdx.x; idx < kMlpRows * np; idx += kThreads) {
    const int row = idx / np, col = idx - row * np;
    X[row * sP + col] = col == 0 ? kap[row] : 0.0;
    Xt[row * sP + col] = col == 0 ? nu[row] : 0.0;
  }
  __syncthreads();
}

// nets: [H[0..nel) | U[0..nel) | S[0..nel)]; coeff = [a | b | g], n_frames each; dG may be null (no
// direction: the energy terms alone)
__global__ __launch_bounds__(kThreads) void td_grad2_kernel(const MlpDev *__restrict__ nets, TdGradTiles tiles,
                                                            TdGradShape sh, int ndim, const int32_t *__restrict__ atoms,
                                                            const int32_t *__restrict__ frame_of_atom,
                                                            const double *__restrict__ T, const double *__restrict__ G,
                                                            const double *__restrict__ dG,
                                                            const double *__restrict__ coeff, int n_frames,
                                                            double *scratch, double *partial) {
  extern __shared__ double lds[];
  __shared__ double rowT[kMlpRows], kapU[kMlpRows], nuU[kMlpRows], kapS[kMlpRows], nuS[kMlpRows];
  const int sP = sh.sP, sz = sh.sz, K = sh.K;
  const size_t slab = (size_t)kMlpRows * sP;
  double *X0 = lds, *X1 = X0 + slab, *T0 = X1 + slab, *T1 = T0 + slab;
  double *zX = T1 + slab, *zT = zX + kMlpRows * sz;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = kThreads >> 6;
  const int nel = tiles.nel;
  double *sc = scratch + (size_t)blockIdx.x * sh.slab_wg;
  double *out = partial + (size_t)blockIdx.x * tiles.n_params;
  for (int k = tid; k < tiles.n_params; k += kThreads) out[k] = 0.0;
  const int n_tiles = tiles.tile_start[nel];
  for (int tile_id = blockIdx.x; tile_id < n_tiles; tile_id += gridDim.x) {
    int e = 0;
    while (e + 1 < nel && tile_id >= tiles.tile_start[e + 1]) ++e;
    const MlpDev &H = nets[e], &U = nets[nel + e], &S = nets[2 * nel + e];
    const int32_t *el_atoms = atoms + tiles.elem_start[e];
    const int n_atoms = tiles.elem_start[e + 1] - tiles.elem_start[e];
    const int a0 = (tile_id - tiles.tile_start[e]) * kMlpRows;
    const int nrows = min(kMlpRows, n_atoms - a0);
    double *scH = sc, *scU = scH + 4 * H.n_layers * slab, *scS = scU + 4 * U.n_layers * slab;
    __syncthreads();

    // per-row temperature and seeds of the U and S outputs (0 on padding rows)
    if (tid < kMlpRows) {
      double t = 0.0, ku = 0.0, nu = 0.0, ks = 0.0, ns = 0.0;
      if (tid < nrows) {
        const int f = frame_of_atom[el_atoms[a0 + tid]];
        t = T[f];
        const double a = coeff[f], b = coeff[n_frames + f], g = coeff[2 * n_frames + f];
        const double c = sh.sommerfeld ? t : 1.0;
        ku = a + b;
        nu = 1.0;
        ks = c * (g - t * b);
        ns = -t * c;
      }
      rowT[tid] = t;
      kapU[tid] = ku;
      nuU[tid] = nu;
      kapS[tid] = ks;
      nuS[tid] = ns;
    }
    // H input x and its tangent x' (min-max scaled: x = (xhi - G) / (xhi - xlo), x' = -dG / (xhi - xlo))
    const int kp0 = H.layer[0].kp;
    for (int idx = tid; idx < kMlpRows * kp0; idx += kThreads) {
      const int row = idx / kp0, k = idx - row * kp0;
      double x = 0.0, xt = 0.0;
      if (row < nrows && k < ndim) {
        const size_t id = (size_t)el_atoms[a0 + row];
        x = G[id * ndim + k];
        xt = dG ? dG[id * ndim + k] : 0.0;
        if (H.xlo) {
          const double den = H.xhi[k] - H.xlo[k];
          x = (den != 0.0) ? (H.xhi[k] - x) / den : 0.0;  // div_no_nan, atomic.py:195
          xt = (den != 0.0) ? -xt / den : 0.0;
        }
      }
      X1[row * sP + k] = x;
      T1[row * sP + k] = xt;
    }
    __syncthreads();

    // 1. H forward with tangent; z = [H, T, 0 ...], z' = [H', 0 ...] padded to U's (= S's) kp
    double *oX, *oT;
    tdg_forward(H, sh.act_h, X1, T1, sP, X0, X1, T0, T1, sP, scH, nrows, lane, wave, nwaves, oX, oT);
    const int zp = U.layer[0].kp;
    for (int idx = tid; idx < kMlpRows * zp; idx += kThreads) {
      const int row = idx / zp, k = idx - row * zp;
      double v = 0.0, vt = 0.0;
      if (k < K) {
        v = oX[row * sP + k];
        vt = oT[row * sP + k];
      } else if (k == K) {
        v = rowT[row];  // _add_electron_temperature, finite_temperature.py:94-118
      }
      zX[row * sz + k] = v;
      zT[row * sz + k] = vt;
    }
    __syncthreads();

    // 2. U and S forward (their layer-0 inputs are parked in the scratch: z / z' are free afterwards)
    tdg_forward(U, sh.act, zX, zT, sz, X0, X1, T0, T1, sP, scU, nrows, lane, wave, nwaves, oX, oT);
    tdg_forward(S, sh.act, zX, zT, sz, X0, X1, T0, T1, sP, scS, nrows, lane, wave, nwaves, oX, oT);

    // 3. U reverse: (kappa_z, nu_z) = its input adjoints; S reverse adds its own
    tdg_seed(X0, T0, sP, U.layer[U.n_layers - 1].np, kapU, nuU);
    tdg_reverse<true>(U, X0, T0, X1, T1, sP, scU, out + tiles.net_off[nel + e], lane, wave, nwaves,
                      [&](int row, int col, double v) { zX[row * sz + col] = v; },
                      [&](int row, int col, double v) { zT[row * sz + col] = v; });
    tdg_seed(X0, T0, sP, S.layer[S.n_layers - 1].np, kapS, nuS);
    tdg_reverse<true>(S, X0, T0, X1, T1, sP, scS, out + tiles.net_off[2 * nel + e], lane, wave, nwaves,
                      [&](int row, int col, double v) { zX[row * sz + col] += v; },
                      [&](int row, int col, double v) { zT[row * sz + col] += v; });

    // 4. H reverse from the vector seeds (kappa_z, nu_z)[:K]; H's output layer is linear
    const int npH = H.layer[H.n_layers - 1].np;
    for (int idx = tid; idx < kMlpRows * npH; idx += kThreads) {
      const int row = idx / npH, col = idx - row * npH;
      X0[row * sP + col] = col < K ? zX[row * sz + col] : 0.0;
      T0[row * sP + col] = col < K ? zT[row * sz + col] : 0.0;
    }
    __syncthreads();
    auto none = [](int, int, double) {};
    tdg_reverse<false>(H, X0, T0, X1, T1, sP, scH, out + tiles.net_off[e], lane, wave, nwaves, none, none);
  }
}

struct TdGradPlan {
  TdGradTiles tiles;
  TdGradShape sh;
  size_t lds_bytes;
  int blocks;
};

TdGradPlan td_grad_plan(const MlpDev *nets, int nel, int K, const int32_t *elem_start) {
  TdGradPlan p;
  int w = 0, wz = 0;
  size_t layers = 0;
  int off = 0;
  for (int j = 0; j < 3 * nel; ++j) {
    const MlpDev &n = nets[j];
    p.tiles.net_off[j] = off;
    for (int l = 0; l < n.n_layers; ++l) {
      off += n.layer[l].k * n.layer[l].n + n.layer[l].n;
      w = std::max(w, n.layer[l].np);
      if (j < nel || l > 0) w = std::max(w, n.layer[l].kp);
    }
    if (j >= nel) wz = std::max(wz, n.layer[0].kp);
  }
  for (int e = 0; e < nel; ++e)
    layers = std::max(layers, (size_t)(nets[e].n_layers + nets[nel + e].n_layers + nets[2 * nel + e].n_layers));
  for (int j = 3 * nel; j < 3 * kMaxElements; ++j) p.tiles.net_off[j] = off;
  p.tiles.nel = nel;
  p.tiles.n_params = off;
  int tiles = 0;
  for (int e = 0; e < nel; ++e) {
    p.tiles.tile_start[e] = tiles;
    p.tiles.elem_start[e] = elem_start[e];
    tiles += (elem_start[e + 1] - elem_start[e] + kMlpRows - 1) / kMlpRows;
  }
  p.tiles.tile_start[nel] = tiles;
  p.tiles.elem_start[nel] = elem_start[nel];
  for (int e = nel + 1; e <= kMaxElements; ++e) p.tiles.tile_start[e] = p.tiles.elem_start[e] = 0;
  w = std::max(w, wz);  // the scratch keeps U's and S's layer-0 inputs z, z' at stride sP
  p.sh.sP = w + 2;
  p.sh.sz = wz + 2;
  p.sh.K = K;
  p.sh.act_h = p.sh.act = p.sh.sommerfeld = 0;
  p.sh.slab_wg = layers * 4 * kMlpRows * (size_t)p.sh.sP;
  p.lds_bytes = (size_t)kMlpRows * (4 * p.sh.sP + 2 * p.sh.sz) * sizeof(double);
  if (p.lds_bytes > kLdsLimit) throw std::domain_error("finite-temperature network too wide for the training tile");
  p.blocks = std::min(tiles, kMaxBlocks);
  return p;
}

}  // namespace

int td_param_count(const MlpDev *nets, int nel) {
  int n = 0;
  for (int j = 0; j < 3 * nel; ++j)
    for (int l = 0; l < nets[j].n_layers; ++l) n += nets[j].layer[l].k * nets[j].layer[l].n + nets[j].layer[l].n;
  return n;
}

// doubles of scratch and partial space one launch over this batch needs
void td_grad2_sizes(const MlpDev *nets, int nel, int K, const int32_t *elem_start, size_t *scratch,
                    size_t *partial) {
  const TdGradPlan p = td_grad_plan(nets, nel, K, elem_start);
  *scratch = (size_t)p.blocks * p.sh.slab_wg;
  *partial = (size_t)p.blocks * (size_t)p.tiles.n_params;
}

// grad (device, td_param_count doubles) = d/dtheta [sum_f (a U_f + b F_f + g S_f) + D_delta F];
// `coeff` = [a | b | g] (device, 3 n_frames), `dG` = directional derivative of the descriptors [N][ndim]
// or null, `T` = electron temperature per frame
void launch_td_grad2(const MlpDev *nets_dev, const MlpDev *nets_host, int nel, int K, int act_h, int act,
                     int sommerfeld, int ndim, const DeviceBatch &b, const double *T, const double *dG,
                     const double *coeff, double *scratch, double *partial, double *grad, hipStream_t s) {
  TdGradPlan p = td_grad_plan(nets_host, nel, K, b.elem_start);
  if (p.blocks == 0) {
    (void)hipMemsetAsync(grad, 0, (size_t)p.tiles.n_params * sizeof(double), s);
    return;
  }
  p.sh.act_h = act_h;
  p.sh.act = act;
  p.sh.sommerfeld = sommerfeld;
  if (p.lds_bytes > 64 * 1024)
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(td_grad2_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit) != hipSuccess)
      throw std::runtime_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
  hipLaunchKernelGGL(td_grad2_kernel, dim3((unsigned)p.blocks), dim3(kThreads), p.lds_bytes, s, nets_dev, p.tiles,
                     p.sh, ndim, b.elem_atoms, b.frame_of_atom, T, b.G, dG, coeff, b.n_frames, scratch, partial);
  launch_grad_reduce(partial, p.blocks, p.tiles.n_params, grad, s);
}

}  // namespace ta
