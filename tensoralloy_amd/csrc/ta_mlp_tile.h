// 16-row MLP tile on the fp64 matrix cores, shared by the stand-alone MLP
// kernels (ta_mlp.hip), the nn-EAM embedding kernels (ta_eam.hip), the
// temperature-dependent head (ta_td.hip) and the training kernels.
//
// Replaces `convolution1x1` (reference nn/convolutional.py:154-300) and the
// part of `tf.gradients` that flows through it, plus the min-max scaling of
// nn/atomic/atomic.py:157-195.
//
// One workgroup owns 16 rows (the M dimension of v_mfma_f64_16x16x4_f64); its
// wavefronts split the 16-column output tiles. Layer inputs live in LDS as
// [16][stride] row-major (A operand: lane l reads X[l & 15][4 kk + (l >> 4)]);
// weights stream from L2 (B operand: lane l reads W[4 kk + (l >> 4)][16 nt +
// (l & 15)], 16 consecutive doubles per k row) in batches of 4 k-steps. The f64
// accumulator tile holds Z[(l >> 4) + 4 r][l & 15] in register r. Activation
// derivatives are parked in `da` (global scratch or LDS) for the backward
// sweep, which runs the same tiles against the transposed weights.
//
// Two bodies: `mlp_tile` takes every network; `mlp_tile_scalar` takes the
// usual shape (hidden layers without skips, one linear output unit) and leaves
// out the padded output-layer GEMMs and every elementwise pass of the former.
#pragma once
#include <hip/hip_runtime.h>

#include "ta_device.h"
#include "ta_math.h"

// -DTA_PHASE_STAMPS builds of ta_mlp.hip define this before the include: TA_MLP_STAMP(k) stamps phase k
#ifndef TA_MLP_STAMP
#define TA_MLP_STAMP(k) ((void)0)
#endif

namespace ta {

typedef double mlp_f64x4 __attribute__((ext_vector_type(4)));
constexpr int kMlpRows = 16;

// Z[16][np] = X[16][kp] . W[kp][np] (+ bias), result handed to `emit(row, col, z)`.
// PF = k-steps whose B operands are fetched from L2 before the first of them is used (4 or 16:
// one dependent load round per PF k-steps).
template <int PF, typename Emit>
__device__ __forceinline__ void mlp_tile_gemm(const double *X, int xstride, const double *W,
                                              int wstride, int kp, int np, const double *bias,
                                              int lane, int wave, int nwaves, Emit emit) {
  const int m = lane & 15, kq = lane >> 4;
  for (int nt = wave; nt < np / 16; nt += nwaves) {
    const int col = 16 * nt + m;
    const double b0 = bias ? bias[col] : 0.0;
    mlp_f64x4 acc = {b0, b0, b0, b0};
    const int nk = kp / 4;  // kp is a multiple of 16 -> nk is a multiple of 4
    int kk0 = 0;
    if constexpr (PF > 4) {
      for (; kk0 + PF <= nk; kk0 += PF) {
        double w[PF];
#pragma unroll
        for (int j = 0; j < PF; ++j) w[j] = W[(size_t)(4 * (kk0 + j) + kq) * wstride + col];
#pragma unroll
        for (int j = 0; j < PF; ++j)
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(X[m * xstride + 4 * (kk0 + j) + kq], w[j], acc, 0, 0, 0);
      }
    }
    for (; kk0 < nk; kk0 += 4) {
      double a[4], w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        w[j] = W[(size_t)(4 * (kk0 + j) + kq) * wstride + col];
        a[j] = X[m * xstride + 4 * (kk0 + j) + kq];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[j], w[j], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) emit(kq + 4 * r, col, acc[r]);
  }
}

// Forward + backward-to-inputs for 16 rows. On entry buf0[row][k] holds the RAW
// descriptors of the rows (k < ndim); rows >= nrows are ignored. All threads of
// the workgroup must call it. `emit_energy(row, y)` and `emit_grad(row, k, dE/dG)`
// are called for row < nrows.
template <int PF = 4, typename EmitE, typename EmitG>
__device__ __forceinline__ void mlp_tile(const MlpDev &mlp, int act, int ndim, int nrows,
                                         double *buf0, double *buf1, int stride, double *da,
                                         EmitE emit_energy, EmitG emit_grad) {
  const int tid = threadIdx.x, nthreads = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6, nwaves = nthreads >> 6;
  const int L = mlp.n_layers;

  // layer-0 input: (optionally min-max scaled) descriptors, zero padded
  const int kp0 = mlp.layer[0].kp;
  for (int idx = tid; idx < kMlpRows * kp0; idx += nthreads) {
    const int row = idx / kp0, k = idx - row * kp0;
    double x = 0.0;
    if (row < nrows && k < ndim) {
      x = buf0[row * stride + k];
      if (mlp.xlo) {
        const double den = mlp.xhi[k] - mlp.xlo[k];
        x = (den != 0.0) ? (mlp.xhi[k] - x) / den : 0.0;  // div_no_nan, atomic.py:195
      }
    }
    buf1[row * stride + k] = x;
  }
  __syncthreads();

  double *cur = buf1, *nxt = buf0;
  for (int l = 0; l < L; ++l) {
    const MlpLayerDev ly = mlp.layer[l];
    double *dal = da + (size_t)l * kMlpRows * stride;
    mlp_tile_gemm<PF>(cur, stride, ly.w, ly.np, ly.kp, ly.np, ly.b, lane, wave, nwaves,
                  [&](int row, int col, double z) {
                    // rows beyond nrows are padding: no transcendental work for them
                    double h = 0.0, dh = 0.0;
                    if (row < nrows) {
                      h = z;
                      dh = 1.0;
                      if (ly.act) activation_fn(act, z, h, dh);
                      if (ly.res) h += cur[row * stride + col];  // convolutional.py:272-273
                    }
                    nxt[row * stride + col] = h;
                    dal[row * stride + col] = dh;
                  });
    __syncthreads();
    TA_MLP_STAMP(2 + l);
    double *t = cur;
    cur = nxt;
    nxt = t;
  }
  // atomic energies: column 0 of the (padded) output layer
  if (tid < nrows) emit_energy(tid, cur[tid * stride]);
  __syncthreads();
  TA_MLP_STAMP(2 + L);

  // backward: delta = dE_atom / d(layer output); start from the output column
  const int npL = mlp.layer[L - 1].np;
  for (int idx = tid; idx < kMlpRows * npL; idx += nthreads) {
    const int row = idx / npL, col = idx - row * npL;
    cur[row * stride + col] = (col == 0) ? 1.0 : 0.0;
  }
  __syncthreads();
  for (int l = L - 1; l >= 0; --l) {
    const MlpLayerDev ly = mlp.layer[l];
    const double *dal = da + (size_t)l * kMlpRows * stride;
    // dz = delta * act'(z), in place; keep delta for the skip connection
    if (ly.res) {
      for (int idx = tid; idx < kMlpRows * ly.np; idx += nthreads) {
        const int row = idx / ly.np, col = idx - row * ly.np;
        nxt[row * stride + col] = cur[row * stride + col];
      }
    }
    for (int idx = tid; idx < kMlpRows * ly.np; idx += nthreads) {
      const int row = idx / ly.np, col = idx - row * ly.np;
      cur[row * stride + col] *= dal[row * stride + col];
    }
    __syncthreads();
    // delta_prev[16][kp] = dz[16][np] . W^T[np][kp]  (+ delta when skip)
    const bool res = ly.res != 0;
    double *dst = nxt;
    mlp_tile_gemm<PF>(cur, stride, ly.wt, ly.kp, ly.np, ly.kp, nullptr, lane, wave, nwaves,
                  [&](int row, int col, double z) {
                    const double skip = res ? dst[row * stride + col] : 0.0;
                    dst[row * stride + col] = z + skip;
                  });
    __syncthreads();
    TA_MLP_STAMP(2 + L + (L - l));
    double *t = cur;
    cur = nxt;
    nxt = t;
  }
  for (int idx = tid; idx < kMlpRows * ndim; idx += nthreads) {
    const int row = idx / ndim, k = idx - row * ndim;
    if (row >= nrows) continue;
    double d = cur[row * stride + k];
    if (mlp.xlo) {
      const double den = mlp.xhi[k] - mlp.xlo[k];
      d = (den != 0.0) ? -d / den : 0.0;
    }
    emit_grad(row, k, d);
  }
  __syncthreads();
  TA_MLP_STAMP(3 + 2 * L);
}

// ---- the tile body for scalar-output networks -------------------------------------------------------
// Hidden layers 0 .. L-2 without skip connections, output layer L-1 with one linear unit (`mlp_tile_scalar_ok`,
// decided on the host per network). The output layer is not a GEMM here: y = b + h . w_out is a dot product
// folded into the emit of the last hidden layer, and the backward sweep starts from dz = w_out * act' of that
// layer instead of a one-hot delta pushed through a 16 -> np GEMM. Every backward emit multiplies by act' of the
// layer below and stores that layer's dz; the layer-0 emit hands dE/dG out of the accumulators.
// L - 1 forward and L - 1 backward GEMM phases, 2 L - 3 workgroup barriers after the staging one, no
// elementwise pass (mlp_tile: 2 L phases, 4 L + 1 barriers, 2 L + 1 passes).

// host: does `mlp_tile_scalar` take this network?
inline bool mlp_tile_scalar_ok(const MlpDev &mlp) {
  const int L = mlp.n_layers;
  if (L < 2) return false;
  for (int l = 0; l < L; ++l)
    if (mlp.layer[l].res) return false;
  for (int l = 0; l + 1 < L; ++l)
    if (!mlp.layer[l].act || mlp.layer[l + 1].kp != mlp.layer[l].np) return false;
  return mlp.layer[L - 1].n == 1 && !mlp.layer[L - 1].act;
}

// Layer-0 input of `mlp_tile_scalar`, one pass and one barrier: buf[row][k] = the (optionally min-max scaled)
// descriptor `load(row, k)` for row < nrows, k < ndim, zero up to the padded width. THREADS % 256 == 0.
template <int THREADS, typename Load>
__device__ __forceinline__ void mlp_tile_stage(const MlpDev &mlp, int ndim, int nrows, double *buf, int stride,
                                               Load load) {
  const int kp0 = mlp.layer[0].kp;
  const int row = (threadIdx.x >> 4) & (kMlpRows - 1);
  for (int k = (threadIdx.x & 15) + 16 * (threadIdx.x >> 8); k < kp0; k += 16 * (THREADS / 256)) {
    double x = 0.0;
    if (row < nrows && k < ndim) {
      x = load(row, k);
      if (mlp.xlo) {
        const double den = mlp.xhi[k] - mlp.xlo[k];
        x = (den != 0.0) ? (mlp.xhi[k] - x) / den : 0.0;  // div_no_nan, atomic.py:195
      }
    }
    buf[row * stride + k] = x;
  }
  __syncthreads();
}

// Forward + backward-to-inputs for 16 rows of a network `mlp_tile_scalar_ok` accepts. On entry buf0 holds the
// layer-0 input (mlp_tile_stage). All threads of the workgroup must call it. `emit_energy(row, y)` and
// `emit_grad(row, k, dE/dG)` are called for row < nrows. The last slab of `da` (act' of the output layer in
// mlp_tile) holds the partial energies of the last hidden layer's column tiles.
template <int PF = 4, typename EmitE, typename EmitG>
__device__ __forceinline__ void mlp_tile_scalar(const MlpDev &mlp, int act, int ndim, int nrows, double *buf0,
                                                double *buf1, int stride, double *da, EmitE emit_energy,
                                                EmitG emit_grad) {
  const int tid = threadIdx.x, nthreads = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6, nwaves = nthreads >> 6;
  const int L = mlp.n_layers;
  double *cur = buf0, *nxt = buf1;
  int stamp = 2;

  // Forward. ONE GEMM call site for every hidden layer and one for every backward layer, the last hidden layer
  // and layer 0 being run-time cases of the emits. With a call site of its own for each (35 KB of code instead of
  // 20 KB) the last hidden layer of the 8-64-64-1 network took 4.8 us against 3.6 us now and 3.0 us for the same
  // GEMM in mlp_tile (profiles/mlp_scalar_tile_notes.md); supposed cause: the kernel runs its code once per
  // workgroup, so every further inlined copy of the k loop and of the activation switch is fetched cold.
  // The last hidden layer's output is consumed on the spot: column tile nt of a lane's DPP row (16 lanes, one row
  // of the tile, 16 columns) sums h * w_out into esum[nt][row], and dz = w_out * act' goes to `nxt`. Padded
  // columns carry act(0) != 0 and vanish because w_out is zero there (checked at upload).
  const double *wout = mlp.layer[L - 1].wt;  // row 0 of the transposed copy: w_out[k], k < kp
  double *esum = da + (size_t)(L - 1) * kMlpRows * stride;
  for (int l = 0; l + 1 < L; ++l) {
    const MlpLayerDev ly = mlp.layer[l];
    const bool last = l + 2 == L;
    double *dal = da + (size_t)l * kMlpRows * stride;
    // w_out of the wavefront's first tile is in flight while the GEMM runs
    const int col_first = 16 * wave + (lane & 15);
    const double wo_first = last && col_first < ly.np ? wout[col_first] : 0.0;
    mlp_tile_gemm<PF>(cur, stride, ly.w, ly.np, ly.kp, ly.np, ly.b, lane, wave, nwaves,
                      [&](int row, int col, double z) {
                        // rows beyond nrows are padding: no transcendental work for them
                        double h = 0.0, dh = 0.0;
                        if (row < nrows) activation_fn(act, z, h, dh);
                        if (last) {
                          const double wo = col == col_first ? wo_first : wout[col];
                          nxt[row * stride + col] = wo * dh;
                          const double e = row16_sum(h * wo);
                          if ((col & 15) == 0) esum[(col >> 4) * kMlpRows + row] = e;
                        } else {
                          nxt[row * stride + col] = h;
                          dal[row * stride + col] = dh;
                        }
                      });
    __syncthreads();
    TA_MLP_STAMP(stamp++);
    double *t = cur;
    cur = nxt;
    nxt = t;
  }
  // atomic energies: the tiles in ascending order, then the output bias
  if (tid < nrows) {
    double y = esum[tid];
    for (int nt = 1; nt < mlp.layer[L - 2].np / 16; ++nt) y += esum[nt * kMlpRows + tid];
    emit_energy(tid, y + mlp.layer[L - 1].b[0]);
  }
  TA_MLP_STAMP(stamp++);
  // Backward: cur = dz of layer l; delta = dz . W_l^T. Above layer 0 the emit stores dz of layer l - 1 = delta *
  // act'(z_{l-1}); the layer-0 emit applies the min-max factor and hands dE/dG out of the accumulators.
  for (int l = L - 2; l >= 0; --l) {
    const MlpLayerDev ly = mlp.layer[l];
    const double *dal = da + (size_t)(l > 0 ? l - 1 : 0) * kMlpRows * stride;
    mlp_tile_gemm<PF>(cur, stride, ly.wt, ly.kp, ly.np, ly.kp, nullptr, lane, wave, nwaves,
                      [&](int row, int col, double z) {
                        if (l > 0) {
                          nxt[row * stride + col] = z * dal[row * stride + col];
                        } else if (row < nrows && col < ndim) {
                          double d = z;
                          if (mlp.xlo) {
                            const double den = mlp.xhi[col] - mlp.xlo[col];
                            d = (den != 0.0) ? -d / den : 0.0;
                          }
                          emit_grad(row, col, d);
                        }
                      });
    if (l > 0) __syncthreads();
    TA_MLP_STAMP(stamp++);
    double *t = cur;
    cur = nxt;
    nxt = t;
  }
}

inline int mlp_stride(const MlpDev &mlp) {
  const int w = mlp.max_np > mlp.max_kp ? mlp.max_np : mlp.max_kp;
  return w + 2;
}

}  // namespace ta
