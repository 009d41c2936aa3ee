// C ABI of libtensoralloy_amd.so: context, device memory, launch sequencing.
// Declarations and the reference interfaces they replace: include/tensoralloy_amd.h
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "ta_context.h"

using namespace ta::host;

namespace {

thread_local std::string g_create_error;

// Small transfers between the page-locked staging buffers and device memory as a kernel ON the
// compute stream (the device reads / writes the mapped host memory over PCIe) instead of an
// asynchronous copy: a copy command goes to a DMA engine behind cross-queue barriers, about 10 us
// of latency each way, which is what one MD step of a 4000-atom frame (96 KB in, 128 KB out) pays.
__global__ __launch_bounds__(256) void staged_copy_kernel(double *__restrict__ dst,
                                                          const double *__restrict__ src, size_t n) {
  for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (size_t)gridDim.x * 256) dst[k] = src[k];
}
constexpr size_t kStagedCopyMaxBytes = 4u << 20;  // beyond that the DMA engine's bandwidth wins

}  // namespace

void ta::host::staged_copy(double *dst, const double *src, size_t n, bool to_host, const ta::Options &opt,
                           hipStream_t s) {
  if (n == 0) return;
  if (n * sizeof(double) > kStagedCopyMaxBytes || opt.staged_copy_dma) {
    HIP_CHECK(hipMemcpyAsync(dst, src, n * sizeof(double), to_host ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice, s));
    return;
  }
  const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 256);
  hipLaunchKernelGGL(staged_copy_kernel, dim3(blocks), dim3(256), 0, s, dst, src, n);
  HIP_CHECK(hipGetLastError());
}

// Wait for the stream on the latency-critical paths (one MD step has three waits around ~50 us kernels):
// poll the stream for a short while before blocking, since a blocked thread is woken by an interrupt
// many microseconds after the work is done. Options::sync_blocking goes straight to the blocking wait.
void ta::host::wait_stream(hipStream_t s, const ta::Options &opt) {
  if (!opt.sync_blocking) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
      const hipError_t e = hipStreamQuery(s);
      if (e == hipSuccess) return;
      if (e != hipErrorNotReady) {
        (void)hipGetLastError();
        break;  // let the blocking wait report it
      }
      if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(400)) break;
    }
  }
  HIP_CHECK(hipStreamSynchronize(s));
}

int ta::host::fail(ta_context *h, int code, const std::string &msg) {
  if (h)
    h->err = msg;
  else
    g_create_error = msg;
  return code;
}

// temperature-dependent models have no analytic Hessian-vector products
std::string ta::host::td_inference_only(const char *fn) {
  return std::string(fn) + ": not available for finite-temperature (temperature-dependent) models "
         "(no analytic Hessian-vector products)";
}

// eam/fs models evaluate energies, forces and virials only
std::string ta::host::fs_inference_only(const char *fn) {
  return std::string(fn) + ": not available for eam/fs models (inference only: no weight, constant or loss "
         "gradients and no analytic Hessian-vector products; differences of the forces give the latter)";
}

namespace {

template <typename T>
T *upload(ta_context *h, const std::vector<T> &v) {
  T *d = nullptr;
  size_t n = v.size() ? v.size() : 1;
  HIP_CHECK(hipMalloc((void **)&d, n * sizeof(T)));
  h->model_allocs.push_back(d);
  if (!v.empty()) HIP_CHECK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return d;
}

int round_up(int x, int m) { return (x + m - 1) / m * m; }

// Power series in u of Hd(u) = exp(-beta u) * 0.5 (1 + cos(pi sqrt(u))) on [0, 1]
// (cosine cutoff nn/cutoff.py:43-48 times the Gaussian of sf.py:166-168 for the
// third side of a triple), in long double, economised to 12, 16 or 24 coefficients when
// the error bound is below 1e-17 (1e-15 for the derivative), otherwise n_hd = 0 (exact path).
void hd_series(int cutoff, double beta, ta::AngChunk &ch) {
  ch.n_hd = 0;
  for (double &c : ch.hd) c = 0.0;
  if (cutoff != TA_CUTOFF_COSINE || !(beta >= 0.0)) return;
  constexpr int NT = 64;
  const long double pi2 = 9.869604401089358618834490999876151135L;
  long double fc[NT], ex[NT], prod[NT];
  long double t = 1.0L;  // (-pi^2)^k / (2k)!
  for (int k = 0; k < NT; ++k) {
    fc[k] = 0.5L * t + (k == 0 ? 0.5L : 0.0L);
    t *= -pi2 / (long double)((2 * k + 1) * (2 * k + 2));
  }
  t = 1.0L;  // (-beta)^k / k!
  for (int k = 0; k < NT; ++k) {
    ex[k] = t;
    t *= -(long double)beta / (long double)(k + 1);
  }
  for (int k = 0; k < NT; ++k) {
    long double acc = 0.0L;
    for (int j = 0; j <= k; ++j) acc += fc[j] * ex[k - j];
    prod[k] = acc;
  }
  // Chebyshev economisation: starting from the degree-(N0 - 1) Taylor polynomial, the leading term
  // a_n u^n is replaced by a_n (u^n - T*_n(u) / L_n), T*_n(u) = T_n(2u - 1) with leading coefficient
  // L_n = 2^(2n-1); that changes the polynomial by at most |a_n| / L_n on [0, 1] and its derivative
  // by at most 2 n^2 |a_n| / L_n, and lowers the degree by one. Repeated down to n coefficients, this
  // reaches the fp64 rounding floor with 12 coefficients for the default beta where the plain
  // series needs 16 (4 / 8 fewer FMAs per triple in the forward / backward kernels).
  constexpr int N0 = 40;
  static long double tstar[N0][N0];  // tstar[n][k]: coefficient of u^k in T*_n
  static bool have_t = false;
  if (!have_t) {
    for (auto &row : tstar)
      for (auto &c : row) c = 0.0L;
    tstar[0][0] = 1.0L;
    tstar[1][0] = -1.0L;
    tstar[1][1] = 2.0L;
    for (int n = 1; n + 1 < N0; ++n)
      for (int k = 0; k <= n + 1; ++k)
        tstar[n + 1][k] = (k > 0 ? 4.0L * tstar[n][k - 1] : 0.0L) - 2.0L * tstar[n][k] - tstar[n - 1][k];
    have_t = true;
  }
  long double tail0 = 0.0L, dtail0 = 0.0L;
  for (int k = N0; k < NT; ++k) {
    tail0 += fabsl(prod[k]);
    dtail0 += (long double)k * fabsl(prod[k]);
  }
  for (int n : {12, 16, 24}) {
    long double a[N0];
    for (int k = 0; k < N0; ++k) a[k] = prod[k];
    long double err = tail0, derr = dtail0;
    for (int d = N0 - 1; d >= n; --d) {
      const long double q = a[d] / tstar[d][d];
      for (int k = 0; k <= d; ++k) a[k] -= q * tstar[d][k];
      err += fabsl(q);
      derr += 2.0L * (long double)d * (long double)d * fabsl(q);
    }
    if (err < 1e-17L && derr < 1e-15L) {
      ch.n_hd = n;
      for (int k = 0; k < n; ++k) ch.hd[k] = (double)a[k];
      return;
    }
  }
}

void build_mlp(ta_context *h, const ta_model_desc *m, int ndim);

void build_sf_model(ta_context *h, const ta_model_desc *m) {
  using namespace ta;
  SFParams &sf = h->sf;
  std::memset(&sf, 0, sizeof(sf));
  const int nel = m->n_elements;
  if (m->n_eta < 1 || m->n_omega < 1 || !m->eta || !m->omega)
    throw std::invalid_argument("eta / omega must be non-empty");
  if (m->n_eta * m->n_omega > kMaxRadial)
    throw std::domain_error("more than 64 radial (eta x omega) combinations");
  if (!(m->rcut > 0.0)) throw std::invalid_argument("rcut must be positive");
  sf.rcut = m->rcut;
  sf.acut = m->angular ? m->acut : m->rcut;
  if (m->angular && !(m->acut > 0.0)) throw std::invalid_argument("acut must be positive");
  sf.inv_rc2 = 1.0 / (sf.rcut * sf.rcut);
  sf.inv_ac2 = 1.0 / (sf.acut * sf.acut);
  sf.two_inv_ac2 = 2.0 * sf.inv_ac2;
  sf.eps = m->eps > 0.0 ? m->eps : 1e-14;  // Precision.high / medium eps, precision.py:113-114
  sf.n_elements = nel;
  sf.n_rad = m->n_eta * m->n_omega;
  sf.angular = m->angular ? 1 : 0;
  sf.cutoff = m->cutoff_function;
  if (sf.cutoff != TA_CUTOFF_COSINE && sf.cutoff != TA_CUTOFF_POLYNOMIAL)
    throw std::invalid_argument("unknown cutoff function");
  // ParameterGrid order: eta outer, omega fastest (sf.py:47-48)
  for (int e = 0; e < m->n_eta; ++e)
    for (int o = 0; o < m->n_omega; ++o) {
      sf.eta[e * m->n_omega + o] = m->eta[e];
      sf.omega[e * m->n_omega + o] = m->omega[o];
    }
  for (int c = 1; c < sf.n_rad; ++c) {
    if ((c & 3) == 0 || sf.omega[c] != sf.omega[c - 1] || !(sf.eta[c - 1] > 0.0)) continue;
    const double k = sf.eta[c] / sf.eta[c - 1];
    if (k >= 2.0 && k <= 16.0 && k == std::nearbyint(k) && k * sf.eta[c - 1] == sf.eta[c] &&
        !h->opt.no_eta_chain)
      sf.eta_pow[c] = (signed char)k;
  }
  sf.n_radial_dim = nel * sf.n_rad;
  sf.n_ang = 0;
  sf.n_beta = 0;
  if (m->angular) {
    if (m->n_beta < 1 || m->n_gamma < 1 || m->n_zeta < 1 || !m->beta || !m->gamma || !m->zeta)
      throw std::invalid_argument("beta / gamma / zeta must be non-empty for an angular model");
    if (m->n_beta > kMaxBetaSlots)
      throw std::domain_error("more than 3 beta values are not supported by the pair record");
    sf.n_beta = m->n_beta;
    for (int k = 0; k < m->n_beta; ++k) sf.beta[k] = m->beta[k];
    sf.n_ang = m->n_beta * m->n_gamma * m->n_zeta;
    // channel (ib, ig, iz) -> (ib * n_gamma + ig) * n_zeta + iz  (zeta fastest, sf.py:49-51)
    for (int pass = 0; pass < 2; ++pass)
    for (int b0 = 0; b0 < m->n_beta; b0 += (pass == 0 ? 2 : 1))
      for (int g0 = 0; g0 < m->n_gamma; g0 += 2)
        for (int z0 = 0; z0 < m->n_zeta; z0 += 2) {
          ChunkPlan cp;
          std::memset(&cp, 0, sizeof(cp));
          cp.nb = std::min(pass == 0 ? 2 : 1, m->n_beta - b0);
          cp.ng = std::min(2, m->n_gamma - g0);
          cp.nz = std::min(2, m->n_zeta - z0);
          for (int ib = 0; ib < cp.nb; ++ib) {
            cp.ch.beta[ib] = m->beta[b0 + ib];
            cp.ch.hslot[ib] = b0 + ib;
          }
          cp.ch.safe_pow = m->safe_pow ? 1 : 0;
          for (int ig = 0; ig < cp.ng; ++ig) cp.ch.gamma[ig] = m->gamma[g0 + ig];
          for (int iz = 0; iz < cp.nz; ++iz) {
            const double z = m->zeta[z0 + iz];
            cp.ch.zeta[iz] = z;
            cp.ch.kz[iz] = std::pow(2.0, 1.0 - z);
            const double zr = std::nearbyint(z);
            cp.ch.zeta_int[iz] = (zr == z && z >= 1.0 && z <= 1024.0) ? (int)zr : -1;
          }
          for (int ib = 0; ib < cp.nb; ++ib)
            for (int ig = 0; ig < cp.ng; ++ig)
              for (int iz = 0; iz < cp.nz; ++iz)
                cp.ch.chan[(ib * cp.ng + ig) * cp.nz + iz] =
                    ((b0 + ib) * m->n_gamma + (g0 + ig)) * m->n_zeta + (z0 + iz);
          if (pass == 1) hd_series(sf.cutoff, cp.ch.beta[0], cp.ch);
          (pass == 0 ? h->chunks : h->chunks_v2).push_back(cp);
        }
  }
  const int n_aterms = m->angular ? nel * (nel + 1) / 2 : 0;
  (void)0;
  sf.ndim = sf.n_radial_dim + n_aterms * sf.n_ang;
  h->rmax = std::max(sf.rcut, sf.acut);
  build_mlp(h, m, sf.ndim);
}

// one network's weights (layer_sizes `sizes[0..L]`, weights from `wsrc`, advanced past them) -> padded
// device copies, both orientations. The output layer is linear; ResNet skips as convolutional.py:272.
void build_net(ta_context *h, ta::MlpDev &md, int L, const int32_t *sizes, const double *&wsrc, int resnet) {
  using namespace ta;
  if (L < 1 || L > kMaxLayers) throw std::domain_error("MLP depth out of range (1..8 layers)");
  md.n_layers = L;
  md.max_np = md.max_kp = 0;
  for (int l = 0; l < L; ++l) {
    MlpLayerDev &ly = md.layer[l];
    ly.k = sizes[l];
    ly.n = sizes[l + 1];
    if (ly.k < 1 || ly.n < 1 || ly.k > 512 || ly.n > 512)
      throw std::domain_error("MLP layer width out of range (1..512)");
    ly.kp = round_up(ly.k, 16);
    ly.np = round_up(ly.n, 16);
    ly.act = (l < L - 1) ? 1 : 0;
    // ResNet skip: hidden layer j > 0 with equal widths (convolutional.py:272)
    ly.res = (resnet && l > 0 && l < L - 1 && ly.k == ly.n) ? 1 : 0;
    std::vector<double> w((size_t)ly.kp * ly.np, 0.0), wt((size_t)ly.np * ly.kp, 0.0), bb(ly.np, 0.0);
    for (int k = 0; k < ly.k; ++k)
      for (int n = 0; n < ly.n; ++n) {
        const double v = wsrc[(size_t)k * ly.n + n];
        w[(size_t)k * ly.np + n] = v;
        wt[(size_t)n * ly.kp + k] = v;
      }
    wsrc += (size_t)ly.k * ly.n;
    for (int n = 0; n < ly.n; ++n) bb[n] = wsrc[n];
    wsrc += ly.n;
    // mlp_tile_scalar reads the scalar output layer as the vector wt[0 .. kp): hidden units beyond the logical
    // width carry act(0) != 0 and drop out only because these entries are zero
    if (l == L - 1 && ly.n == 1)
      for (int k = ly.k; k < ly.kp; ++k)
        if (wt[k] != 0.0) throw std::logic_error("padded output weights are not zero");
    ly.w = upload(h, w);
    ly.wt = upload(h, wt);
    ly.b = upload(h, bb);
    md.max_np = std::max(md.max_np, ly.np);
    md.max_kp = std::max(md.max_kp, ly.kp);
  }
}

// per-element MLP weights -> padded device copies, both orientations. Temperature-dependent models:
// 3 n_elements nets H[el], U[el], S[el] (ta_model_desc.finite_temperature)
void build_mlp(ta_context *h, const ta_model_desc *m, int ndim) {
  using namespace ta;
  const int nel = m->n_elements;
  if (!m->n_layers || !m->layer_sizes || !m->weights)
    throw std::invalid_argument("MLP description missing");
  h->activation = m->activation;
  if (m->activation < 0 || m->activation > TA_ACT_ELU)
    throw std::invalid_argument("unknown activation");
  const int td = m->finite_temperature;
  const int32_t *sizes = m->layer_sizes;
  const double *wsrc = m->weights;
  if (td) {
    if ((td & ~(TA_TD_ON | TA_TD_SOMMERFELD | (0xff << TA_TD_ACT_SHIFT))) || !(td & TA_TD_ON))
      throw std::invalid_argument("unknown finite_temperature bits");
    h->td = true;
    h->td_sommerfeld = (td & TA_TD_SOMMERFELD) != 0;
    h->td_act = (td >> TA_TD_ACT_SHIFT) & 0xff;
    if (h->td_act > TA_ACT_ELU) throw std::invalid_argument("unknown activation of the H nets");
    h->td_K = 0;
    for (int q = 0; q < 3; ++q)
      for (int el = 0; el < nel; ++el) {
        MlpDev &md = h->td_nets[q * nel + el];
        const int L = m->n_layers[q * nel + el];
        if (L < 1 || L > kMaxLayers) throw std::domain_error("MLP depth out of range (1..8 layers)");
        if (q == 0) {
          if (sizes[0] != ndim) throw std::invalid_argument("H input size does not match the descriptor length");
          if (el == 0) h->td_K = sizes[L];
          if (sizes[L] != h->td_K) throw std::invalid_argument("H output width differs between elements");
        } else {
          if (sizes[0] != h->td_K + 1) throw std::invalid_argument("U / S input size must be the H width + 1");
          if (sizes[L] != 1) throw std::invalid_argument("U / S output size must be 1");
        }
        build_net(h, md, L, sizes, wsrc, m->use_resnet_dt);
        if (q == 0 && m->minmax_scale) {
          if (!m->xlo || !m->xhi) throw std::invalid_argument("minmax_scale set but xlo/xhi missing");
          std::vector<double> lo(m->xlo + (size_t)el * ndim, m->xlo + (size_t)(el + 1) * ndim);
          std::vector<double> hi(m->xhi + (size_t)el * ndim, m->xhi + (size_t)(el + 1) * ndim);
          md.xlo = upload(h, lo);
          md.xhi = upload(h, hi);
        }
        sizes += L + 1;
      }
    std::vector<MlpDev> all(h->td_nets, h->td_nets + 3 * nel);
    h->td_dev = upload(h, all);
    return;
  }
  for (int el = 0; el < nel; ++el) {
    MlpDev &md = h->mlp[el];
    const int L = m->n_layers[el];
    if (L < 1 || L > kMaxLayers) throw std::domain_error("MLP depth out of range (1..8 layers)");
    if (sizes[0] != ndim)
      throw std::invalid_argument("MLP input size does not match the descriptor length");
    if (sizes[L] != 1) throw std::invalid_argument("MLP output size must be 1");
    build_net(h, md, L, sizes, wsrc, m->use_resnet_dt);
    if (m->minmax_scale) {
      if (!m->xlo || !m->xhi) throw std::invalid_argument("minmax_scale set but xlo/xhi missing");
      std::vector<double> lo(m->xlo + (size_t)el * ndim, m->xlo + (size_t)(el + 1) * ndim);
      std::vector<double> hi(m->xhi + (size_t)el * ndim, m->xhi + (size_t)(el + 1) * ndim);
      md.xlo = upload(h, lo);
      md.xhi = upload(h, hi);
    }
    sizes += L + 1;
  }
  {
    std::vector<MlpDev> all(h->mlp, h->mlp + nel);
    h->mlp_dev = upload(h, all);
  }
}

void upload_batch(ta_context *h) {
  using namespace ta;
  HostPairs &hp = h->hp;
  DeviceBatch &db = h->db;
  const size_t N = (size_t)hp.n_atoms, P = (size_t)hp.n_pairs;
  const int nel = h->n_elements;
  const size_t F = (size_t)db.n_frames;
  db.n_atoms = hp.n_atoms;
  db.n_pairs = hp.n_pairs;
  db.nnl_max = hp.nnl_max;

  auto put = [&](auto &buf, const auto &vec) {
    buf.ensure(vec.size());
    if (!vec.empty())
      HIP_CHECK(hipMemcpyAsync(buf.ptr, vec.data(), vec.size() * sizeof(vec[0]),
                               hipMemcpyHostToDevice, h->stream));
  };
  if (h->pairs_on_device) {
    h->pair_i.ensure(P);
    h->pair_j.ensure(P);
    h->pair_shift.ensure(3 * P);
    h->pair_rev.ensure(P);
  } else {
    put(h->pair_start, hp.pair_start);
    put(h->seg_start, hp.seg_start);
    put(h->pair_i, hp.pair_i);
    put(h->pair_j, hp.pair_j);
    put(h->pair_shift, hp.pair_shift);
    put(h->pair_rev, hp.pair_rev);
  }

  const bool has_mlp = h->kind == TA_MODEL_SF_MLP || h->kind == TA_MODEL_GRAP_MLP;
  const int D = has_mlp ? h->sf.ndim : 1;
  h->rec.ensure(P * kRecDoubles);
  if (h->kind == TA_MODEL_SF_MLP && h->sf.angular) {
    h->part4.ensure((size_t)nel * h->sf.n_ang * P);
    // one 64-bit candidate mask per pair and per block of 64 rotation steps (n/2 steps in all)
    h->masks.ensure((size_t)((hp.nnl_max / 2 + 63) / 64 + 1) * P);
  }
  h->G.ensure(N * D);
  h->dEdG.ensure(N * D);
  h->g.ensure(4 * P);
  h->wat.ensure(9 * N);
  h->bpart.ensure(10 * ((N + 15) / 16) + 10);
  h->fown.ensure(12 * N + 12);
  h->results.ensure(10 * F + 4 * N);
  h->benergy.ensure(1);

  db.pair_start = h->pair_start.ptr;
  db.seg_start = h->seg_start.ptr;
  db.pair_i = h->pair_i.ptr;
  db.pair_j = h->pair_j.ptr;
  db.pair_shift = h->pair_shift.ptr;
  db.pair_rev = h->pair_rev.ptr;
  db.rec = h->rec.ptr;
  db.part4 = h->part4.ptr;
  db.masks = h->masks.ptr;
  db.G = h->G.ptr;
  db.dEdG = h->dEdG.ptr;
  db.g = h->g.ptr;
  db.wat = h->wat.ptr;
  db.bpart = h->bpart.ptr;
  db.fown = h->fown.ptr;
  db.energy = h->results.ptr;
  db.virial = h->results.ptr + F;
  db.eatom = h->results.ptr + 10 * F;
  db.forces = h->results.ptr + 10 * F + N;
  db.batch_energy = h->benergy.ptr;
}

ta::NlWork nl_work(ta_context *h) {
  return ta::NlWork{h->nl_wrap.ptr,       h->nl_binid.ptr,     h->nl_bin_count.ptr, h->nl_bin_start.ptr,
                    h->nl_bin_cursor.ptr, h->nl_bin_atoms.ptr, h->nl_recs.ptr,      h->nl_counts.ptr,
                    h->seg_start.ptr,     h->nl_stats.ptr};
}

// Neighbour list on the device, part 1. Leaves the counts in h->hp (n_pairs, n_triples, nnl_max,
// pair_start) for the sizing done by the caller. The packed input (positions, species, grids ...) is
// already on its way to the device.
//
// One-pass builder (ta_nlist.hip::nl_build) first: it also WRITES the pairs (key order) while they fit
// the pair arrays as they stand; when they do not (first batch, or a list that grew) the arrays grow and
// it runs again. The two-pass builder (count, sizes to the host, fill) stays for what the one-pass one
// declines: more than 384 neighbours per atom, shifts beyond +-511 cells, Options::nl_two_pass.
void build_pairs_on_device(ta_context *h, size_t N, int n_bins) {
  using namespace ta;
  HostPairs &hp = h->hp;
  hipStream_t s = h->stream;
  const int nel = h->n_elements;
  h->nl_wrap.ensure(3 * N);
  h->nl_binid.ensure(N);
  h->nl_bin_start.ensure((size_t)n_bins + 1);
  h->nl_bin_atoms.ensure(N);
  h->nl_recs.ensure(N);
  h->seg_start.ensure(N * (nel + 1) + 1);
  h->pair_start.ensure(N + 1);
  // counts and per-atom offsets come back through page-locked memory
  h->stage_out.ensure(64 + (N + 1) * sizeof(int32_t));
  unsigned long long *stats = reinterpret_cast<unsigned long long *>(h->stage_out.ptr);
  int32_t *starts = reinterpret_cast<int32_t *>(h->stage_out.ptr + 64);
  const int32_t *si = reinterpret_cast<const int32_t *>(stats);
  const bool two_pass_only = h->opt.nl_two_pass;
  h->nl_sorted = false;
  const bool kernel_writes_host = !h->opt.nl_copy_starts;
  if (!two_pass_only) {
    {  // the zero block stays clean from list to list while its layout (atoms, bins) does not change
      const unsigned long long *before = h->nl_zero.ptr;
      h->nl_zero.ensure(nl_build_zero_words((int)N, n_bins));
      if (h->nl_zero.ptr != before || h->nl_zero_atoms != (int64_t)N || h->nl_zero_bins != n_bins) h->nl_zero_clean = false;
      h->nl_zero_atoms = (int64_t)N;
      h->nl_zero_bins = n_bins;
    }
    h->nl_rev_done = false;
    for (int attempt = 0; attempt < 2 && !h->nl_sorted; ++attempt) {
      const size_t capacity = std::min(std::min(h->pair_i.cap, h->pair_j.cap), h->pair_shift.cap / 3);
      // the reverse index is launched right behind the pairs, before the count is known here: over as many
      // pairs as the previous list of these atoms had (+ a quarter), at most what the arrays hold
      h->pair_rev.ensure(capacity);
      const size_t guess = (hp.n_atoms == (int64_t)N && hp.n_pairs > 0) ? (size_t)hp.n_pairs + (size_t)hp.n_pairs / 4 + 4096
                                                                         : capacity;
      const size_t rev_cover = std::min(std::min(capacity, guess), (size_t)INT32_MAX);
      NlWork w = nl_work(h);
      // the kernel writes the per-atom offsets to the page-locked buffer itself; the statistics follow
      // in one small copy kernel once every group is through
      nl_build((int)N, n_bins, nel, h->r_list, h->db.pos, h->db.species, h->db.frame_of_atom, h->d_grids, w,
               h->nl_zero.ptr, h->nl_zero_clean, (long long)std::min<size_t>(capacity, (size_t)INT32_MAX), h->pair_start.ptr,
               kernel_writes_host ? starts : nullptr, h->pair_i.ptr, h->pair_j.ptr, h->pair_shift.ptr,
               h->pair_rev.ptr, (long long)rev_cover, s);
      HIP_CHECK(hipGetLastError());
      h->nl_zero_clean = false;  // until this list is through (an exception below leaves it marked dirty)
      if (!kernel_writes_host)
        staged_copy(reinterpret_cast<double *>(starts), reinterpret_cast<const double *>(h->pair_start.ptr),
                    (N + 2) / 2, true, h->opt, s);
      staged_copy(reinterpret_cast<double *>(stats), reinterpret_cast<const double *>(h->nl_zero.ptr), 8, true, h->opt, s);
      wait_stream(s, h->opt);
      h->nl_zero_clean = N > 0;  // the kernels ran to the end: histogram cleared, the rest is cleared on entry
      if (si[3] != 0) break;  // beyond the one-pass builder's limits
      if (stats[4] > (unsigned long long)INT32_MAX) throw std::runtime_error("batch too large for 32-bit pair indices");
      if (stats[4] <= capacity) {
        h->nl_sorted = true;
        h->nl_rev_done = stats[4] <= rev_cover;  // (else fill_pairs_on_device launches it over the whole list)
        if (h->nl_rev_done && si[6] != 0)
          throw std::runtime_error("neighbour list is not symmetric (reverse pair missing)");
      } else {
        h->pair_i.ensure((size_t)stats[4]);
        h->pair_j.ensure((size_t)stats[4]);
        h->pair_shift.ensure(3 * (size_t)stats[4]);
      }
    }
    if (h->nl_sorted) h->nl_stats_ptr = h->nl_zero.ptr;
  }
  if (!h->nl_sorted) {
    h->nl_bin_count.ensure((size_t)n_bins + 1);
    h->nl_bin_cursor.ensure((size_t)n_bins + 1);
    h->nl_counts.ensure(N * (nel + 1) + 1);
    h->nl_stats.ensure(8);
    NlWork w = nl_work(h);
    nl_count((int)N, n_bins, nel, h->r_list, h->db.pos, h->db.species, h->db.frame_of_atom, h->d_grids, w,
             h->pair_start.ptr, s);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(stats, h->nl_stats.ptr, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(starts, h->pair_start.ptr, (N + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (stats[4] > (unsigned long long)INT32_MAX || si[4] < 0 || (unsigned long long)si[4] != stats[4])
      throw std::runtime_error("batch too large for 32-bit pair indices");
    h->nl_stats_ptr = h->nl_stats.ptr;
  }
  hp.n_atoms = (int64_t)N;
  hp.n_pairs = (int64_t)stats[4];
  hp.n_triples = (int64_t)stats[0];
  hp.nnl_max = si[2];
  hp.pair_start.assign(starts, starts + N + 1);
  hp.seg_start.clear();
  hp.pair_i.clear();
  hp.pair_j.clear();
  hp.pair_shift.clear();
  hp.pair_rev.clear();
  h->pairs_on_device = true;
}

// part 2, after the pair buffers are sized: the pairs (two-pass builder only) and the reverse index
void fill_pairs_on_device(ta_context *h) {
  using namespace ta;
  if (h->nl_sorted) {
    nl_reverse_sorted(h->hp.n_pairs, h->n_elements, h->db.species, h->seg_start.ptr, h->pair_i.ptr,
                      h->pair_j.ptr, h->pair_shift.ptr, h->pair_rev.ptr, h->nl_stats_ptr, h->stream);
  } else {
    NlWork w = nl_work(h);
    nl_fill((int)h->hp.n_atoms, h->hp.n_pairs, h->n_elements, h->r_list, h->db.pos, h->db.species,
            h->db.frame_of_atom, h->d_grids, w, h->pair_i.ptr, h->pair_j.ptr, h->pair_shift.ptr,
            h->pair_rev.ptr, h->stream);
  }
  HIP_CHECK(hipGetLastError());
}

#ifdef TA_PHASE_STAMPS
// diagnostic builds: phase stamps of the angular kernels of the LAST evaluation, written to the file
// named by TA_PHASE_STAMPS_OUT (Options::phase_stamps_out) at ta_destroy (scripts/phase_stamps.sh)
// (kernel 0 / 1: the angular kernels; kernel 2: the MLP tile kernel, workgroups that stamped nothing left out)
static size_t mlp_stamp_blocks(const ta_context *h) {  // at least the grid of a tile launch
  return (size_t)h->db.n_atoms / ta::kMlpStampRows + (size_t)h->n_elements + 1;
}
static void dump_stamps(ta_context *h) {
  const std::string &path = h->opt.phase_stamps_out;
  if (path.empty() || !h->db.stamps || h->db.n_blk <= 0) return;
  const size_t n_mlp = mlp_stamp_blocks(h);
  const size_t n = (size_t)(2 * h->db.n_blk + n_mlp) * ta::kStampSlots;
  std::vector<unsigned long long> v(n);
  (void)hipStreamSynchronize(h->stream);
  (void)hipMemcpy(v.data(), h->db.stamps, n * sizeof(unsigned long long), hipMemcpyDeviceToHost);
  FILE *fp = std::fopen(path.c_str(), "w");
  if (!fp) return;
  for (int k = 0; k < 2; ++k)
    for (int b = 0; b < h->db.n_blk; ++b) {
      std::fprintf(fp, "%d %d", k, b);
      for (int q = 0; q < ta::kStampSlots; ++q)
        std::fprintf(fp, " %llu", v[((size_t)k * h->db.n_blk + b) * ta::kStampSlots + q]);
      std::fprintf(fp, "\n");
    }
  for (size_t b = 0; b < n_mlp; ++b) {
    const unsigned long long *row = &v[((size_t)2 * h->db.n_blk + b) * ta::kStampSlots];
    if (!row[0]) continue;
    std::fprintf(fp, "2 %zu", b);
    for (int q = 0; q < ta::kStampSlots; ++q) std::fprintf(fp, " %llu", row[q]);
    std::fprintf(fp, "\n");
  }
  std::fclose(fp);
}
#endif

// per-atom head on the descriptors: the MLP, or the temperature-dependent H / U / S nets
void launch_head(ta_context *h, const ta::DeviceBatch &db, hipStream_t s) {
  if (h->td)
    ta::launch_td_all(h->td_dev, h->td_nets, h->n_elements, h->td_K, h->td_act, h->activation,
                      h->td_sommerfeld ? 1 : 0, h->sf.ndim, db, h->opt.mlp_da_global, h->td_T.ptr, h->td_u.ptr, h->td_s.ptr,
                      h->mlp_scratch.ptr, s, &h->last_mlp_launch);
  else
    ta::launch_mlp_all(h->mlp_dev, h->mlp, h->n_elements, h->activation, h->sf.ndim, db, h->opt, h->mlp_scratch.ptr,
                       s, &h->last_mlp_launch);
}

}  // namespace

// The forward launches of the second-generation angular path, one per chunk. `tri`: the backward launches of
// this evaluation are asked to take the triangle build. The full job list is left out only when EVERY one of
// them does (a chunk that falls back to the per-apex kernel reads it), and the handle remembers which.
void ta::host::forward_v2_launches(ta_context *h, bool tri) {
  using namespace ta;
  bool unread = tri && h->db.job_word_own && h->db.job_count_own && h->db.job_count;
  for (const ChunkPlan &cp : h->chunks_v2) unread = unread && v2_backward_takes_triangles(h->sf, cp.ch, cp.ng, cp.nz);
  bool geometry = true;
  size_t left = h->chunks_v2.size();
  for (const ChunkPlan &cp : h->chunks_v2) {
    --left;
    launch_g4_forward_v2(h->sf, cp.ch, cp.ng, cp.nz, geometry, left == 0, unread, h->db, h->opt, h->stream);
    geometry = false;
  }
  h->full_jobs_valid = !unread;
}

void ta::host::compute_impl(ta_context *h, uint32_t want, bool timed, double *slot_ms) {
  using namespace ta;
#ifdef TA_PHASE_STAMPS
  if (h->db.n_blk > 0) {
    const size_t n_mlp = mlp_stamp_blocks(h);
    h->stamp_buf.ensure((size_t)(2 * h->db.n_blk + n_mlp) * ta::kStampSlots + 8);
    h->db.stamps = h->stamp_buf.ptr;
    h->db.mlp_stamps = h->stamp_buf.ptr + (size_t)2 * h->db.n_blk * ta::kStampSlots;
    (void)hipMemsetAsync(h->db.stamps, 0,
                         (size_t)(2 * h->db.n_blk + n_mlp) * ta::kStampSlots * sizeof(unsigned long long), h->stream);
  }
#endif
  h->db.rec4 = nullptr;  // only the second-generation angular path below sets it
  h->db.own_sums = 0;    // likewise
  const DeviceBatch &db = h->db;
  hipStream_t s = h->stream;
  const bool need_forces = (want & (TA_WANT_FORCES | TA_WANT_VIRIAL)) != 0;
  auto begin = [&](int slot) {
    if (timed) HIP_CHECK(hipEventRecord(h->ev[2 * slot], s));
  };
  auto end = [&](int slot) {
    if (timed) HIP_CHECK(hipEventRecord(h->ev[2 * slot + 1], s));
  };
  bool used[TA_N_KERNEL_SLOTS] = {false};

  // energies again on the descriptors already resident (training steps: only the MLP changed)
  const bool has_mlp = h->kind == TA_MODEL_SF_MLP || h->kind == TA_MODEL_GRAP_MLP;
  if ((want & TA_WANT_REUSE_DESCRIPTORS) && has_mlp && h->descriptors_valid && !need_forces) {
    begin(TA_K_MLP);
    launch_head(h, db, s);
    end(TA_K_MLP);
    used[TA_K_MLP] = true;
  } else if (h->kind == TA_MODEL_SF_MLP) {
    // second-generation angular path: 32-byte pair records {D, r^2} in the same buffer
    // (Options::full_records keeps the 64-byte ones for A/B runs)
    h->db.rec4 = (h->sf.angular && h->use_v2 && !h->opt.full_records) ? h->db.rec : nullptr;
    if (!h->use_v2) {
      // second-generation forward kernels compute the pair geometry while staging
      begin(TA_K_PAIR_GEOMETRY);
      launch_pair_geometry(h->sf, db, s);
      end(TA_K_PAIR_GEOMETRY);
      used[TA_K_PAIR_GEOMETRY] = true;
    }
    h->sf.ang_scale = h->use_v2 ? 1.0 : 0.5;
    // triangle-once backward pass: the forward launches also leave the owned job lists
    // (while cells relax or follow a barostat, a list stays valid until a width has shrunk by
    // rmax / (rmax + skin): the wider test)
    const bool tri_cells = (h->relax.cell.on || h->md.moves_cells()) ? h->tri_cells_wide_ok : h->tri_cells_ok;
    // (its owner puts the gradient of all three terms of a triangle onto its own two pairs: g is then a partition of
    // the forces, not d e_c / d D_p, which a run that samples the heat current reads)
    const bool tri = h->use_v2 && h->triangles && tri_cells && h->n_elements == 1 && need_forces && !h->centre_gradients;
    h->db.job_word_own = (tri && h->db.job_count) ? h->job_word_own.ptr : nullptr;
    h->db.job_count_own = (tri && h->db.job_count) ? h->job_count_own.ptr : nullptr;
    h->last_bwd_variant = 0;
    // the second-generation forward kernel assembles the descriptors itself in its last launch
    const bool reduce_in_forward = h->sf.angular && h->use_v2;
    if (h->sf.angular) {
      begin(TA_K_G4_FORWARD);
      if (h->use_v2)
        forward_v2_launches(h, tri);
      else
        for (const ChunkPlan &cp : h->chunks) launch_g4_forward(h->sf, cp.ch, cp.nb, cp.ng, cp.nz, db, s);
      end(TA_K_G4_FORWARD);
      used[TA_K_G4_FORWARD] = true;
    }
    if (!reduce_in_forward) {
      begin(TA_K_DESCRIPTOR_REDUCE);
      launch_descriptor_reduce(h->sf, db, s);
      end(TA_K_DESCRIPTOR_REDUCE);
      used[TA_K_DESCRIPTOR_REDUCE] = true;
    }
    begin(TA_K_MLP);
    launch_head(h, db, s);
    end(TA_K_MLP);
    used[TA_K_MLP] = true;
    if (need_forces) {
      begin(TA_K_BACKWARD);
      if (h->sf.angular) {
        bool first = true;
        if (h->use_v2)
          for (const ChunkPlan &cp : h->chunks_v2) {
            h->last_bwd_variant |= launch_backward_v2(h->sf, cp.ch, cp.ng, cp.nz, first, tri, db, h->opt, s);
            first = false;
          }
        else
          for (const ChunkPlan &cp : h->chunks) {
            launch_backward(h->sf, cp.ch, cp.nb, cp.ng, cp.nz, first, false, db, s);
            first = false;
          }
      } else {
        AngChunk dummy;
        std::memset(&dummy, 0, sizeof(dummy));
        launch_backward(h->sf, dummy, 1, 1, 1, true, true, db, s);
      }
      end(TA_K_BACKWARD);
      used[TA_K_BACKWARD] = true;
      begin(TA_K_FORCE_GATHER);
      launch_force_gather(h->sf, db, h->opt.gather_w, s);
      end(TA_K_FORCE_GATHER);
      used[TA_K_FORCE_GATHER] = true;
    }
  } else if (h->kind == TA_MODEL_GRAP_MLP) {
    // 32-byte pair records, as on the second-generation angular path; the `nn` filter network evaluated
    // exactly takes r from the full records its geometry pre-pass writes (through its table it has no pre-pass)
    const bool net_exact = ta::grap_uses_filter_net(h->grap) && !ta::grap_filter_table_knots(h->grap);
    h->db.rec4 = (!net_exact && !h->opt.full_records) ? h->db.rec : nullptr;
    begin(TA_K_GRAP);
    launch_grap_forward(h->grap, db, h->sf.eps, s);  // computes the pair geometry while staging
    end(TA_K_GRAP);
    used[TA_K_GRAP] = true;
    begin(TA_K_MLP);
    launch_head(h, db, s);
    end(TA_K_MLP);
    used[TA_K_MLP] = true;
    if (need_forces) {
      begin(TA_K_BACKWARD);
      h->db.own_sums = h->opt.no_own_sums ? 0 : 1;  // one wavefront per centre: the sums are nearly free there
      launch_grap_backward(h->grap, db, s);
      end(TA_K_BACKWARD);
      used[TA_K_BACKWARD] = true;
      begin(TA_K_FORCE_GATHER);
      launch_force_gather(h->sf, db, h->opt.gather_w, s);
      end(TA_K_FORCE_GATHER);
      used[TA_K_FORCE_GATHER] = true;
    }
  } else {
    h->db.rec4 = h->opt.full_records ? nullptr : h->db.rec;  // 32-byte pair records {D, r^2}
    begin(TA_K_EAM);
    eam_compute(h->eam, db, want, s, nullptr);
    end(TA_K_EAM);
    used[TA_K_EAM] = true;
  }
  begin(TA_K_FRAME_REDUCE);
  {
    // MD step (ta_step / ta_step_view): the last kernel also writes the results' page-locked image
    double *mirror = nullptr;
    int64_t n_tail = 0;
    h->mirror_want = 0;
    if (h->mirror_next && !timed) {
      const size_t N = (size_t)db.n_atoms, F = (size_t)db.n_frames;
      h->stage_out.ensure((10 * F + 4 * N + 2) * sizeof(double));
      mirror = reinterpret_cast<double *>(h->stage_out.ptr);
      n_tail = (int64_t)(need_forces ? 4 * N : N);
      h->mirror_want = want | TA_WANT_ENERGY | TA_WANT_ATOMIC;
    }
    launch_frame_reduce(db, need_forces, mirror, n_tail, s);
  }
  end(TA_K_FRAME_REDUCE);
  used[TA_K_FRAME_REDUCE] = true;
  HIP_CHECK(hipGetLastError());
  h->last_want = want;
  h->descriptors_valid = true;

  if (timed) {
    HIP_CHECK(hipStreamSynchronize(s));
    for (int k = 0; k < TA_N_KERNEL_SLOTS; ++k) {
      if (!used[k]) continue;
      float ms = 0.f;
      HIP_CHECK(hipEventElapsedTime(&ms, h->ev[2 * k], h->ev[2 * k + 1]));
      slot_ms[k] += ms;
    }
  }
}

extern "C" {

int ta_abi_version(void) { return TA_ABI_VERSION; }
int ta_model_desc_size(void) { return (int)sizeof(ta_model_desc); }

int ta_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char *ta_last_error(ta_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int ta_create(const ta_model_desc *model, int device, ta_handle *out) {
  if (!model || !out) return fail(nullptr, TA_ERR_INVALID, "null argument");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, TA_ERR_HIP, "no HIP device available: this library has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(nullptr, TA_ERR_INVALID, "device index out of range");
  if (model->n_elements < 1 || model->n_elements > ta::kMaxElements)
    return fail(nullptr, TA_ERR_UNSUPPORTED, "n_elements must be in 1..8");
  ta_context *h = new ta_context();
  h->opt = ta::options_from_env();
  h->device = device;
  h->kind = model->kind;
  h->n_elements = model->n_elements;
  int rc = guarded(h, [&]() {
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
      throw HipError(std::string("device is ") + prop.gcnArchName +
                     ", this library is built for gfx950 only");
    HIP_CHECK(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    h->stream = h->own_stream;
    for (auto &e : h->ev) HIP_CHECK(hipEventCreate(&e));
    if (model->kind == TA_MODEL_SF_MLP) {
      build_sf_model(h, model);
    } else if (model->kind == TA_MODEL_GRAP_MLP) {
      if (model->cutoff_function != TA_CUTOFF_COSINE && model->cutoff_function != TA_CUTOFF_POLYNOMIAL)
        throw std::invalid_argument("unknown cutoff function");
      std::string err;
      h->grap = ta::grap_create(model, err);
      if (!h->grap) throw std::invalid_argument(err);
      h->rmax = model->rcut;
      std::memset(&h->sf, 0, sizeof(h->sf));
      h->sf.n_elements = model->n_elements;
      h->sf.eps = model->eps > 0.0 ? model->eps : 1e-14;
      h->sf.ndim = ta::grap_ndim(h->grap);
      build_mlp(h, model, h->sf.ndim);
    } else if (model->kind == TA_MODEL_EAM_ALLOY || model->kind == TA_MODEL_EAM_ADP || model->kind == TA_MODEL_EAM_FS) {
      std::string err;
      h->eam = ta::eam_create(model, h->opt, err);
      if (!h->eam) throw std::invalid_argument(err);
      h->rmax = model->rcut;
      std::memset(&h->sf, 0, sizeof(h->sf));
      h->sf.n_elements = model->n_elements;
      h->sf.eps = model->eps > 0.0 ? model->eps : 1e-14;
    } else {
      throw std::invalid_argument("unknown model kind");
    }
  });
  if (rc != TA_OK) {
    g_create_error = h->err;
    ta_destroy(h);
    return rc;
  }
  *out = h;
  return TA_OK;
}

int ta_destroy(ta_handle h) {
  if (!h) return TA_OK;
  (void)hipSetDevice(h->device);
#ifdef TA_PHASE_STAMPS
  dump_stamps(h);
#endif
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (void *p : h->model_allocs) (void)hipFree(p);
  if (h->eam) ta::eam_destroy(h->eam);
  if (h->grap) ta::grap_destroy(h->grap);
  for (auto &e : h->ev)
    if (e) (void)hipEventDestroy(e);
  if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
  delete h;
  return TA_OK;
}

}  // extern "C" (reopened below)

namespace {
// job lists of the angular kernels (ta_kernels_v2.hip::make_jobs): room for `n_blk` workgroups
void ensure_job_lists(ta_context *h, size_t n_blk) {
  if (h->opt.no_jobs || !h->use_v2 || n_blk == 0) {  // (no_jobs, A/B switch: per-lane masks + re-dealing)
    h->db.job_count = nullptr;
    return;
  }
  const int stride = ta::v2_job_stride(h->db.cap);
  h->job_word.ensure(n_blk * (size_t)stride + 8);
  h->job_count.ensure(n_blk + 8);
  if (h->n_elements == 1) {  // the triangle-once builds are one-element ones
    h->job_word_own.ensure(n_blk * (size_t)stride + 8);
    h->job_count_own.ensure(n_blk + 8);
  }
  h->db.job_word = h->job_word.ptr;
  h->db.job_count = h->job_count.ptr;
  h->db.job_stride = stride;
}

// MD loop with a Verlet skin: the evaluation kernels get the EXACT list of the current positions,
// extracted from the resident skin list on the device (ta_nlist.hip::nl_filter; no host round trip),
// so they never pay for the skin. Only for models whose kernels are driven by centres (second-
// generation symmetry-function kernels, plain EAM); the others run on the skin list itself, where
// pairs beyond the cutoff contribute nothing.
bool filter_applies(const ta_context *h) {
  if (!(h->skin > 0.0) || h->hp.n_atoms == 0 || h->opt.no_list_filter) return false;
  if (h->kind == TA_MODEL_SF_MLP) return h->use_v2;
  if (h->kind == TA_MODEL_EAM_ALLOY || h->kind == TA_MODEL_EAM_FS) return ta::eam_is_plain(h->eam) && !h->centre_gradients;
  return false;
}
}  // namespace

void ta::host::set_centre_gradients(ta_context *h, bool on) {
  if (h->centre_gradients == on) return;
  h->centre_gradients = on;
  if (!h->eam) return;
  ta::eam_set_pair_route(h->eam, on);
  if (!h->have_batch) return;
  if (on && h->filtered) {  // back to the resident list, as set_frames_impl left it
    h->db.pair_start = h->pair_start.ptr;
    h->db.pair_stop = nullptr;
    h->db.seg_start = h->seg_start.ptr;
    h->db.pair_i = h->pair_i.ptr;
    h->db.pair_j = h->pair_j.ptr;
    h->db.pair_shift = h->pair_shift.ptr;
    h->db.pair_rev = h->pair_rev.ptr;
    h->db.slot_q = h->db.rev_super = h->db.rev_map = nullptr;
    h->filtered = false;
  } else if (!on && filter_applies(h)) {
    apply_filter(h);
  }
  ta::eam_set_list_cutoff(h->eam, (h->skin > 0.0 && !h->filtered) ? h->rmax : 0.0);
}

void ta::host::apply_filter(ta_context *h) {
  using namespace ta;
  const size_t N = (size_t)h->hp.n_atoms, P = (size_t)h->hp.n_pairs;
  const int nel = h->n_elements;
  h->ex_pair_i.ensure(P + 1);
  h->ex_pair_j.ensure(P + 1);
  h->ex_pair_shift.ensure(3 * P + 3);
  h->ex_pair_rev.ensure(P + 1);
  h->ex_pair_start.ensure(N + 1);
  h->ex_pair_stop.ensure(N + 1);
  h->ex_seg_start.ensure(N * (nel + 1) + 1);
  h->ex_map.ensure(P + 1);
  const int n_run_slots = nl_filter_blocks((int)N);
  h->ex_blk.ensure((size_t)n_run_slots + 4);
  h->ex_hdr.ensure((size_t)n_run_slots + 1);
  const bool blocks = h->kind == TA_MODEL_SF_MLP;
  // symmetry-function models: no reverse-index launch; force_gather looks the reverse pair up through the map
  // (Options::filter_rev_kernel: the launch, for A/B)
  const bool indirect = blocks && !h->opt.filter_rev_kernel;
  if (indirect) h->ex_slot_q.ensure(P + 1);
  nl_filter((int)N, (int64_t)P, nel, h->rmax, h->db.pos, h->db.cells, h->db.frame_of_atom,
            h->pair_start.ptr, h->seg_start.ptr, h->pair_j.ptr, h->pair_shift.ptr, h->pair_rev.ptr, h->ex_map.ptr,
            h->ex_seg_start.ptr, h->ex_pair_start.ptr, h->ex_pair_stop.ptr, h->ex_pair_i.ptr, h->ex_pair_j.ptr,
            h->ex_pair_shift.ptr, h->ex_pair_rev.ptr, indirect ? h->ex_slot_q.ptr : nullptr, h->db.cap,
            blocks ? h->ex_blk.ptr : nullptr, blocks ? h->ex_hdr.ptr : nullptr, h->stream);
  h->db.slot_q = indirect ? h->ex_slot_q.ptr : nullptr;
  h->db.rev_super = indirect ? h->pair_rev.ptr : nullptr;
  h->db.rev_map = indirect ? h->ex_map.ptr : nullptr;
  HIP_CHECK(hipGetLastError());
  h->db.pair_start = h->ex_pair_start.ptr;
  h->db.pair_stop = h->ex_pair_stop.ptr;
  h->db.seg_start = h->ex_seg_start.ptr;
  h->db.pair_i = h->ex_pair_i.ptr;
  h->db.pair_j = h->ex_pair_j.ptr;
  h->db.pair_shift = h->ex_pair_shift.ptr;
  h->db.pair_rev = h->ex_pair_rev.ptr;
  if (blocks) {
    h->db.blk_center = h->ex_blk.ptr;
    h->db.blk_hdr = h->ex_hdr.ptr;
    h->db.n_blk = n_run_slots;  // 16 run slots per group of 16 centres; unused ones are empty runs
    h->db.blk_groups = n_run_slots / 16;
    h->db.n_blk_dev = nullptr;
    ensure_job_lists(h, (size_t)n_run_slots);
  }
  h->filtered = true;
}

namespace {
// The triangle-once backward pass needs the three vertices of every triangle to be distinct atoms. Two
// images of one atom are a lattice vector L apart, and |L| is at least the smallest perpendicular width of
// the cell over the periodic axes (some component n_k of L is non-zero, and the projection of L on the
// normal of the other two cell vectors is n_k times width k). A triangle's sides are below acut, so when
// every periodic width exceeds acut no triangle holds two images of one atom, and each vertex sees the
// triangle exactly once among its own triples. The test asks for widths above max(rcut, acut) = rmax.
bool cells_admit_triangles(double rmax, int32_t n_frames, const ta_frame *frames) {
  for (int f = 0; f < n_frames; ++f) {
    const double *c = frames[f].cell;
    const double vol = std::fabs(c[0] * (c[4] * c[8] - c[5] * c[7]) - c[1] * (c[3] * c[8] - c[5] * c[6]) +
                                 c[2] * (c[3] * c[7] - c[4] * c[6]));
    for (int k = 0; k < 3; ++k) {
      if (!frames[f].pbc[k]) continue;
      const double *u = c + 3 * ((k + 1) % 3), *v = c + 3 * ((k + 2) % 3);
      const double nx = u[1] * v[2] - u[2] * v[1], ny = u[2] * v[0] - u[0] * v[2], nz = u[0] * v[1] - u[1] * v[0];
      const double area = std::sqrt(nx * nx + ny * ny + nz * nz);
      if (!(vol > rmax * area)) return false;  // width = vol / area (a degenerate cell fails too)
    }
  }
  return true;
}

// the body of ta_set_frames (also the rebuild path of ta_update_positions); throws
void set_frames_impl(ta_context *h, int32_t n_frames, const ta_frame *frames, ta_batch_info *info) {
  for (int f = 0; f < n_frames; ++f) {
    const ta_frame &fr = frames[f];
    if (fr.n_atoms < 0 || (fr.n_atoms > 0 && (!fr.species || !fr.positions)) || !fr.cell || !fr.pbc)
      throw std::invalid_argument("frame " + std::to_string(f) + ": null array");
  }
  const auto t_begin = std::chrono::steady_clock::now();
  if (h->upload_pending) {  // stage_in is about to be rewritten
    HIP_CHECK(hipStreamSynchronize(h->stream));
    h->upload_pending = false;
  }
  // no batch is resident until this call has succeeded: a failure below (allocation, too many
  // neighbours, asymmetric list ...) must not leave the previous batch's flags standing over
  // buffers that were already regrown or repointed
  h->have_batch = false;
  h->descriptors_valid = false;
  h->jvp_valid = false;
  h->full_jobs_valid = false;
  h->mirror_want = 0;  // (stage_out carries the builder's counts from here on)
  h->filtered = false;
  h->db.slot_q = h->db.rev_super = h->db.rev_map = nullptr;
  h->db.pair_stop = nullptr;
  h->db.blk_groups = 0;
  h->db.n_blk_dev = nullptr;
  h->r_list = h->rmax + h->skin;
  h->tri_cells_ok = cells_admit_triangles(h->rmax, n_frames, frames);
  h->tri_cells_wide_ok = cells_admit_triangles(h->r_list, n_frames, frames);
  size_t N = 0;
  for (int f = 0; f < n_frames; ++f) N += (size_t)frames[f].n_atoms;
  if (N >= (1u << 30)) throw std::runtime_error("batch too large for 32-bit atom indices");
  const size_t F = (size_t)n_frames;
  const int nel = h->n_elements;
  // packed input, every section 16-byte aligned
  auto align16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
  const size_t o_pos = 0;
  const size_t o_cells = align16(o_pos + 3 * N * sizeof(double));
  const size_t o_grids = align16(o_cells + 9 * F * sizeof(double));
  const size_t o_species = align16(o_grids + F * sizeof(ta::NlGrid));
  const size_t o_foa = align16(o_species + N * sizeof(int32_t));
  const size_t o_astart = align16(o_foa + N * sizeof(int32_t));
  const size_t o_elem = align16(o_astart + (F + 1) * sizeof(int32_t));
  const size_t o_blk = align16(o_elem + N * sizeof(int32_t));
  // the run headers (ta::BlockHeader, 64-byte aligned) go behind the run starts actually written, so that one
  // copy takes both; room for one run per atom
  auto align64 = [](size_t x) { return (x + 63) & ~(size_t)63; };
  const size_t total = align64(o_blk + (N + 2) * sizeof(int32_t)) + (N + 1) * sizeof(ta::BlockHeader);
  h->stage_in.ensure(total);
  h->inbuf.ensure(total);
  char *hb = h->stage_in.ptr;
  double *pos = reinterpret_cast<double *>(hb + o_pos);
  double *cells = reinterpret_cast<double *>(hb + o_cells);
  ta::NlGrid *grids = reinterpret_cast<ta::NlGrid *>(hb + o_grids);
  int32_t *species = reinterpret_cast<int32_t *>(hb + o_species);
  int32_t *foa = reinterpret_cast<int32_t *>(hb + o_foa);
  int32_t *astart = reinterpret_cast<int32_t *>(hb + o_astart);
  int32_t *elem_atoms = reinterpret_cast<int32_t *>(hb + o_elem);
  size_t a = 0;
  astart[0] = 0;
  for (int f = 0; f < n_frames; ++f) {
    const ta_frame &fr = frames[f];
    const size_t n = (size_t)fr.n_atoms;
    if (n) {
      std::memcpy(&pos[3 * a], fr.positions, 3 * n * sizeof(double));
      std::memcpy(&species[a], fr.species, n * sizeof(int32_t));
    }
    std::memcpy(&cells[9 * (size_t)f], fr.cell, 9 * sizeof(double));
    for (size_t i = a; i < a + n; ++i) {
      foa[i] = f;
      if (species[i] < 0 || species[i] >= nel)
        throw std::runtime_error("frame " + std::to_string(f) + ": species index out of range");
      if (!std::isfinite(pos[3 * i]) || !std::isfinite(pos[3 * i + 1]) || !std::isfinite(pos[3 * i + 2]))
        throw std::runtime_error("frame " + std::to_string(f) + ": non-finite position");
    }
    a += n;
    astart[f + 1] = (int32_t)a;
  }
  {  // atoms grouped by element for the batched MLP
    std::vector<int32_t> count(nel + 1, 0);
    for (size_t i = 0; i < N; ++i) count[species[i] + 1]++;
    for (int e = 0; e < nel; ++e) count[e + 1] += count[e];
    for (int e = 0; e <= nel; ++e) h->db.elem_start[e] = count[e];
    std::vector<int32_t> fill(count.begin(), count.end() - 1);
    for (size_t i = 0; i < N; ++i) elem_atoms[fill[species[i]]++] = (int32_t)i;
  }
  // Neighbour list: on the device (ta_nlist.hip; cells thinner than the cutoff along a periodic axis
  // included since round 3: one bin there, several images of it), the host builder (ta_neighbor.cpp)
  // only for singular / incomplete cells, cells below ~1 A of height, or Options::host_nl.
  const auto t_nl = std::chrono::steady_clock::now();
  int n_bins = 0;
  bool device_nl = N > 0 && !h->opt.host_nl;
  for (int f = 0; f < n_frames && device_nl; ++f) {
    device_nl = ta::nl_make_grid(frames[f], h->r_list, n_bins, grids[f]);
    if (device_nl) n_bins += ta::nl_bins(grids[f]);
    if (n_bins > (1 << 24)) device_nl = false;
  }
  if (!device_nl) std::memset(static_cast<void *>(grids), 0, F * sizeof(ta::NlGrid));
  // one upload for everything but blk_center (which needs the pair counts)
  if (o_blk)  // (small batches: by a kernel reading the page-locked buffer, see staged_copy; sections are 16-byte aligned)
    staged_copy(reinterpret_cast<double *>(h->inbuf.ptr), reinterpret_cast<const double *>(hb), o_blk / sizeof(double),
                false, h->opt, h->stream);
  char *db_ = h->inbuf.ptr;
  h->db.n_frames = n_frames;
  h->db.pos = reinterpret_cast<double *>(db_ + o_pos);
  h->db.cells = reinterpret_cast<double *>(db_ + o_cells);
  h->d_grids = reinterpret_cast<ta::NlGrid *>(db_ + o_grids);
  h->db.species = reinterpret_cast<int32_t *>(db_ + o_species);
  h->db.frame_of_atom = reinterpret_cast<int32_t *>(db_ + o_foa);
  h->db.atom_start = reinterpret_cast<int32_t *>(db_ + o_astart);
  h->db.elem_atoms = reinterpret_cast<int32_t *>(db_ + o_elem);
  h->db.blk_center = reinterpret_cast<int32_t *>(db_ + o_blk);
  if (device_nl) {
    h->hp.atom_start.assign(astart, astart + F + 1);
    h->hp.frame_of_atom.assign(foa, foa + N);
    build_pairs_on_device(h, N, n_bins);
  } else {
    h->pairs_on_device = false;
    ta::build_pairs(n_frames, frames, nel, h->r_list, h->hp);
  }
  double nl_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_nl).count();
  upload_batch(h);
  const auto t_fill = std::chrono::steady_clock::now();
  const bool list_done = h->pairs_on_device && h->nl_sorted && h->nl_rev_done;  // nothing left but the run packing
  if (h->pairs_on_device && !list_done) {
    fill_pairs_on_device(h);
    // "reverse pair missing" counter, read after the synchronisation below
    staged_copy(reinterpret_cast<double *>(h->stage_out.ptr), reinterpret_cast<const double *>(h->nl_stats_ptr),
                8, true, h->opt, h->stream);
  }
  // second-generation angular kernels: workgroups own whole centres (<= kCap pairs)
  // second-generation kernels: 1-3 elements for every channel grid; 4 and 5 elements for
  // launches of 2 gammas x 2 zetas (the default grid) only
  bool shapes_ok = h->n_elements <= 3;
  if (h->n_elements == 4 || h->n_elements == 5) {
    shapes_ok = !h->chunks_v2.empty();
    for (const ChunkPlan &cp : h->chunks_v2) shapes_ok = shapes_ok && cp.ng == 2 && cp.nz == 2;
  }
  h->use_v2 = h->kind == TA_MODEL_SF_MLP && h->sf.angular && shapes_ok &&
              h->hp.nnl_max <= ta::kCapMax && !h->opt.force_v1;
  const int cap = std::max(ta::kCapMin, (h->hp.nnl_max + 63) / 64 * 64);
  h->db.cap = cap;
  {
    int32_t *blk = reinterpret_cast<int32_t *>(hb + o_blk);
    int nb = 0;
    if (h->use_v2 && N) {
      blk[nb++] = 0;
      int32_t load = 0, ncent = 0;
      for (size_t i = 0; i < N; ++i) {
        const int32_t cnt = h->hp.pair_start[i + 1] - h->hp.pair_start[i];
        if (load + cnt > cap || ncent >= ta::kMaxCentersPerBlock) {
          blk[nb++] = (int32_t)i;
          load = 0;
          ncent = 0;
        }
        load += cnt;
        ++ncent;
      }
      blk[nb++] = (int32_t)N;
    }
    h->db.n_blk = nb ? nb - 1 : 0;
    h->res_n_blk = h->db.n_blk;
    h->o_blk = o_blk;
    // one header per run: what the angular workgroup of the run reads instead of the list
    const size_t o_hdr = align64(o_blk + (size_t)nb * sizeof(int32_t));
    ta::BlockHeader *hdr = reinterpret_cast<ta::BlockHeader *>(hb + o_hdr);
    const int block = std::min(cap, 256);  // lanes of an angular workgroup
    for (int r = 0; r < h->db.n_blk; ++r) {
      const int32_t *ps = h->hp.pair_start.data() + blk[r];
      ta::make_block_header(hdr[r], blk[r], blk[r + 1] - blk[r], ps[0], block, [&](int k) { return ps[k + 1] - ps[k]; });
    }
    h->db.blk_hdr = reinterpret_cast<const ta::BlockHeader *>(db_ + o_hdr);
    ensure_job_lists(h, (size_t)h->db.n_blk);
    if (nb) {
      const size_t bytes = o_hdr + (size_t)h->db.n_blk * sizeof(ta::BlockHeader) - o_blk;  // a multiple of 16
      if (list_done)  // a kernel on the compute stream reads the page-locked buffer: no DMA hand-over
        staged_copy(reinterpret_cast<double *>(db_ + o_blk), reinterpret_cast<const double *>(blk), bytes / sizeof(double),
                    false, h->opt, h->stream);
      else
        HIP_CHECK(hipMemcpyAsync(db_ + o_blk, blk, bytes, hipMemcpyHostToDevice, h->stream));
    }
  }
  if (h->kind == TA_MODEL_SF_MLP) {
    if (!h->use_v2 && ta::g4_lds_bytes(h->hp.nnl_max) > 160 * 1024 && h->sf.angular)
      throw std::domain_error("more than 1150 neighbours per atom exceed the LDS staging buffer");
    size_t need = ta::mlp_all_scratch_doubles(h->mlp, h->n_elements, h->db.elem_start);
    h->mlp_scratch.ensure(need);
  } else if (h->kind == TA_MODEL_GRAP_MLP) {
    h->mlp_scratch.ensure(ta::mlp_all_scratch_doubles(h->mlp, h->n_elements, h->db.elem_start));
    ta::grap_ensure(h->grap, h->db);
  } else {
    ta::eam_ensure(h->eam, h->db);
  }
  if (h->td) {
    const size_t N = (size_t)h->db.n_atoms;
    h->mlp_scratch.ensure(ta::td_scratch_doubles(h->td_nets, h->n_elements, h->td_K, h->db.elem_start, h->opt.mlp_da_global));
    h->td_u.ensure(N + 1);
    h->td_s.ensure(N + 1);
    h->td_T.ensure((size_t)h->db.n_frames + 1);
  }
  // what ta_update_positions needs: the geometry this list was built for and the frames' shapes
  // (host-side copies, made while the device still works on the reverse index)
  h->o_pos = o_pos;
  h->o_cells = o_cells;
  h->o_species = o_species;
  h->ref_pos.assign(pos, pos + 3 * N);
  h->ref_cells.assign(cells, cells + 9 * F);
  h->keep_species.assign(species, species + N);
  h->keep_natoms.resize(F);
  h->keep_pbc.resize(3 * F);
  for (size_t f = 0; f < F; ++f) {
    h->keep_natoms[f] = frames[f].n_atoms;
    for (int a3 = 0; a3 < 3; ++a3) h->keep_pbc[3 * f + a3] = frames[f].pbc[a3] ? 1 : 0;
  }
  if (list_done) {
    // one-pass builder: the list was complete (and checked) at the builder's own wait; the run packing is
    // in flight out of stage_in, whose next writer waits for the stream (upload_pending)
    h->upload_pending = true;
  } else {
    wait_stream(h->stream, h->opt);  // staging buffers are reused by the next call
    h->upload_pending = false;
  }
  if (h->pairs_on_device && !list_done) {
    nl_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_fill).count();
    if (reinterpret_cast<const int32_t *>(h->stage_out.ptr)[6] != 0)
      throw std::runtime_error("neighbour list is not symmetric (reverse pair missing)");
  }
  if (filter_applies(h)) apply_filter(h);
  if (h->eam) ta::eam_set_list_cutoff(h->eam, (h->skin > 0.0 && !h->filtered) ? h->rmax : 0.0);
  ++h->n_list_builds;
  h->have_batch = true;
  if (info) {
    info->n_frames = n_frames;
    info->n_atoms = h->hp.n_atoms;
    info->n_pairs = h->hp.n_pairs;
    info->n_triples = h->hp.n_triples;
    info->nnl_max = h->hp.nnl_max;
    info->descriptor_dim = (h->kind == TA_MODEL_SF_MLP || h->kind == TA_MODEL_GRAP_MLP) ? h->sf.ndim : 0;
    info->nl_on_device = h->pairs_on_device ? 1 : 0;
    info->reserved_ = 0;
    info->nl_ms = nl_ms;
    info->set_frames_ms =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  }
}
}  // namespace

void ta::host::rebuild_list(ta_context *h, const double *positions, const double *cells) {
  const size_t F = h->keep_natoms.size();
  std::vector<ta_frame> frames(F);
  const std::vector<int32_t> species(h->keep_species), pbc(h->keep_pbc), natoms(h->keep_natoms);
  const std::vector<double> old_cells(h->ref_cells);
  size_t a = 0;
  for (size_t f = 0; f < F; ++f) {
    frames[f].n_atoms = natoms[f];
    frames[f].species = species.data() + a;
    frames[f].positions = positions + 3 * a;
    frames[f].cell = (cells ? cells : old_cells.data()) + 9 * f;
    frames[f].pbc = pbc.data() + 3 * f;
    a += (size_t)natoms[f];
  }
  set_frames_impl(h, (int32_t)F, frames.data(), nullptr);
}

extern "C" {

int ta_set_frames(ta_handle h, int32_t n_frames, const ta_frame *frames, ta_batch_info *info) {
  if (!h) return TA_ERR_INVALID;
  if (n_frames < 0 || (n_frames > 0 && !frames)) return fail(h, TA_ERR_INVALID, "bad frames argument");
  h->md.valid = false;  // masses and velocities belong to the batch that leaves
  h->relax.valid = false;
  h->relax.cell.on = false;
  h->relax.band.on = h->relax.band.ran = false;
  h->phonon.valid = h->phonon.have_phi = false;  // the supercell description belongs to the frame that leaves
  return guarded(h, [&]() {
    set_frames_impl(h, n_frames, frames, info);
    if (h->td)  // every frame starts at T = 0, the reference's default (universal.py:295)
      HIP_CHECK(hipMemsetAsync(h->td_T.ptr, 0, (size_t)n_frames * sizeof(double), h->stream));
  });
}

int ta_set_electron_temperatures(ta_handle h, int32_t n_frames, const double *T) {
  if (!h) return TA_ERR_INVALID;
  if (!h->td) return fail(h, TA_ERR_INVALID, "ta_set_electron_temperatures: not a temperature-dependent model");
  if (!h->have_batch && h->keep_natoms.empty()) return fail(h, TA_ERR_INVALID, "no resident batch");
  if (n_frames != (int32_t)h->keep_natoms.size() || (n_frames > 0 && !T))
    return fail(h, TA_ERR_INVALID, "ta_set_electron_temperatures: one temperature per frame of the batch");
  for (int32_t f = 0; f < n_frames; ++f)
    if (!std::isfinite(T[f])) return fail(h, TA_ERR_INVALID, "electron temperatures must be finite");
  return guarded(h, [&]() {
    // nothing enqueued before may still read the old values; the copy is done when the call returns
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (n_frames > 0) {
      HIP_CHECK(hipMemcpyAsync(h->td_T.ptr, T, (size_t)n_frames * sizeof(double), hipMemcpyHostToDevice, h->stream));
      HIP_CHECK(hipStreamSynchronize(h->stream));
    }
  });
}

int ta_get_td_results(ta_handle h, double *energy, double *eentropy, double *energy_atomic, double *eentropy_atomic) {
  if (!h) return TA_ERR_INVALID;
  if (!h->td) return fail(h, TA_ERR_INVALID, "ta_get_td_results: not a temperature-dependent model");
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "no resident batch");
  return guarded(h, [&]() {
    const size_t N = (size_t)h->db.n_atoms, F = h->keep_natoms.size();
    std::vector<double> u(N), s(N);
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (N) {
      HIP_CHECK(hipMemcpy(u.data(), h->td_u.ptr, N * sizeof(double), hipMemcpyDeviceToHost));
      HIP_CHECK(hipMemcpy(s.data(), h->td_s.ptr, N * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (energy_atomic && N) std::memcpy(energy_atomic, u.data(), N * sizeof(double));
    if (eentropy_atomic && N) std::memcpy(eentropy_atomic, s.data(), N * sizeof(double));
    size_t a = 0;
    for (size_t f = 0; f < F; ++f) {
      double su = 0.0, ss = 0.0;
      for (int32_t k = 0; k < h->keep_natoms[f]; ++k, ++a) {
        su += u[a];
        ss += s[a];
      }
      if (energy) energy[f] = su;
      if (eentropy) eentropy[f] = ss;
    }
  });
}

int ta_set_skin(ta_handle h, double skin) {
  if (!h) return TA_ERR_INVALID;
  if (!(skin >= 0.0) || !std::isfinite(skin)) return fail(h, TA_ERR_INVALID, "skin must be a finite length >= 0");
  if (skin != h->skin) {
    h->skin = skin;
    h->have_batch = false;  // the resident list was built for another cutoff
    h->descriptors_valid = false;
  }
  return TA_OK;
}

int ta_update_positions(ta_handle h, const double *positions, const double *cells, int32_t *rebuilt) {
  if (!h || !positions) return fail(h, TA_ERR_INVALID, "null argument");
  if (h->ref_pos.empty() && h->keep_natoms.empty())
    return fail(h, TA_ERR_INVALID, "ta_update_positions called before ta_set_frames");
  return guarded(h, [&]() {
    const size_t N = h->keep_species.size(), F = h->keep_natoms.size();
    // The list stays valid while every atom is within skin / 2 of where it was when the list was
    // built and the cells are the same: two atoms then approach each other by less than skin, so
    // every pair inside rmax is still in the list (pairs beyond rmax contribute nothing: cutoff
    // functions, or the explicit test of the EAM / ADP kernels). Checked on the host: the
    // positions pass through here anyway and no device round trip is needed.
    bool keep = h->have_batch && h->skin > 0.0;
    if (keep && cells) keep = std::memcmp(cells, h->ref_cells.data(), 9 * F * sizeof(double)) == 0;
    if (keep) {
      // Optimistic order: the coordinates go up and the exact list of the step is extracted (device work)
      // BEFORE the host has checked the displacements, which it then does while the device is busy. A list
      // that turns out stale is rebuilt below; what was launched for it is overwritten by the rebuild.
      if (h->upload_pending) {  // the staging buffer must be free again
        HIP_CHECK(hipStreamSynchronize(h->stream));
        h->upload_pending = false;
      }
      double *stage = reinterpret_cast<double *>(h->stage_in.ptr + h->o_pos);
      std::memcpy(stage, positions, 3 * N * sizeof(double));
      staged_copy(h->db.pos, stage, 3 * N, false, h->opt, h->stream);
      h->upload_pending = true;
      if (h->filtered) apply_filter(h);  // the exact list of the new positions, on the device
      h->descriptors_valid = false;
      h->jvp_valid = false;
      h->full_jobs_valid = false;
      const double lim2 = 0.25 * h->skin * h->skin;
      const double *ref = h->ref_pos.data();
      for (size_t i = 0; i < N; ++i) {
        const double dx = positions[3 * i] - ref[3 * i], dy = positions[3 * i + 1] - ref[3 * i + 1],
                     dz = positions[3 * i + 2] - ref[3 * i + 2];
        const double d2 = dx * dx + dy * dy + dz * dz;
        if (!(d2 <= lim2)) {  // (a NaN fails the comparison too and is reported by the rebuild)
          keep = false;
          break;
        }
      }
    }
    if (rebuilt) *rebuilt = keep ? 0 : 1;
    if (keep) {
      ++h->n_list_reuses;
      return;
    }
    rebuild_list(h, positions, cells);
    if (cells && h->relax.cell.on && h->relax.valid && F) {
      // the caller's cells replace the relaxed ones: they are h0 from here on, G = I, the cell velocities 0
      HIP_CHECK(hipMemcpy(h->relax.cell.h0.ptr, h->ref_cells.data(), 9 * F * sizeof(double), hipMemcpyHostToDevice));
      h->relax.cell.reset_deformation(F);
    }
  });
}

int ta_list_stats(ta_handle h, int64_t *n_builds, int64_t *n_reuses) {
  if (!h) return TA_ERR_INVALID;
  if (n_builds) *n_builds = h->n_list_builds;
  if (n_reuses) *n_reuses = h->n_list_reuses;
  return TA_OK;
}

int ta_list_sizes(ta_handle h, int64_t *n_pairs, int64_t *n_triples, int32_t *nnl_max) {
  if (!h) return TA_ERR_INVALID;
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "no resident batch");
  if (n_pairs) *n_pairs = h->hp.n_pairs;
  if (n_triples) *n_triples = h->hp.n_triples;
  if (nnl_max) *nnl_max = h->hp.nnl_max;
  return TA_OK;
}

int ta_compute(ta_handle h, uint32_t want) {
  if (!h) return TA_ERR_INVALID;
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "ta_compute called before ta_set_frames");
  return guarded(h, [&]() { compute_impl(h, want, false, nullptr); });
}

int ta_synchronize(ta_handle h) {
  if (!h) return TA_ERR_INVALID;
  return guarded(h, [&]() { HIP_CHECK(hipStreamSynchronize(h->stream)); });
}

namespace {
// one download of the span of [energy F | virial 9F | atomic N | forces 3N] that is asked for into the
// page-locked staging buffer; returns the pointer that indexes it like h->results (null: nothing asked)
const double *results_to_stage(ta_context *h, bool energy, bool forces, bool virial, bool atomic, double *descriptors) {
  const size_t N = (size_t)h->db.n_atoms, F = (size_t)h->db.n_frames;
  hipStream_t s = h->stream;
  const bool have_forces = (h->last_want & (TA_WANT_FORCES | TA_WANT_VIRIAL)) != 0;
  if ((forces || virial) && !have_forces)
    throw std::invalid_argument("forces / virial requested but the last ta_compute did not produce them");
  if (descriptors && h->kind != TA_MODEL_SF_MLP && h->kind != TA_MODEL_GRAP_MLP)
    throw std::invalid_argument("descriptors are only defined for symmetry-function and GRAP models");
  size_t lo = (size_t)-1, hi = 0;
  auto need = [&](bool on, size_t off, size_t n) {
    if (!on || n == 0) return;
    lo = std::min(lo, off);
    hi = std::max(hi, off + n);
  };
  need(energy, 0, F);
  need(virial, F, 9 * F);
  need(atomic, 10 * F, N);
  need(forces, 10 * F + N, 3 * N);
  const double *stage = nullptr;
  const bool fv = (h->mirror_want & (TA_WANT_FORCES | TA_WANT_VIRIAL)) != 0;
  if (hi > lo && h->mirror_want && (!(forces || virial) || fv)) {
    stage = reinterpret_cast<const double *>(h->stage_out.ptr);  // already there (frame_reduce_kernel's mirror)
  } else if (hi > lo) {
    h->mirror_want = 0;
    h->stage_out.ensure((hi - lo) * sizeof(double));
    stage = reinterpret_cast<const double *>(h->stage_out.ptr) - lo;
    staged_copy(reinterpret_cast<double *>(h->stage_out.ptr), h->results.ptr + lo, hi - lo, true, h->opt, s);
  }
  if (descriptors && N)
    HIP_CHECK(hipMemcpyAsync(descriptors, h->db.G, N * h->sf.ndim * sizeof(double), hipMemcpyDeviceToHost, s));
  wait_stream(s, h->opt);
  h->upload_pending = false;
  return stage;
}
}  // namespace

int ta_get_results(ta_handle h, double *energy, double *forces, double *virial, double *atomic,
                   double *descriptors) {
  if (!h) return TA_ERR_INVALID;
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "no resident batch");
  return guarded(h, [&]() {
    const size_t N = (size_t)h->db.n_atoms, F = (size_t)h->db.n_frames;
    const double *stage = results_to_stage(h, energy != nullptr, forces != nullptr, virial != nullptr,
                                           atomic != nullptr, descriptors);
    if (energy && F) std::memcpy(energy, stage, F * sizeof(double));
    if (virial && F) std::memcpy(virial, stage + F, 9 * F * sizeof(double));
    if (atomic && N) std::memcpy(atomic, stage + 10 * F, N * sizeof(double));
    if (forces && N) std::memcpy(forces, stage + 10 * F + N, 3 * N * sizeof(double));
  });
}

int ta_view_results(ta_handle h, uint32_t want, const double **energy, const double **forces,
                    const double **virial, const double **atomic) {
  if (!h) return TA_ERR_INVALID;
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "no resident batch");
  return guarded(h, [&]() {
    const size_t N = (size_t)h->db.n_atoms, F = (size_t)h->db.n_frames;
    const bool fv = (want & (TA_WANT_FORCES | TA_WANT_VIRIAL)) != 0;
    const double *stage = results_to_stage(h, energy != nullptr, forces && fv, virial && fv,
                                           atomic && (want & TA_WANT_ATOMIC), nullptr);
    if (energy) *energy = (stage && F) ? stage : nullptr;
    if (virial) *virial = (stage && fv && F) ? stage + F : nullptr;
    if (atomic) *atomic = (stage && (want & TA_WANT_ATOMIC) && N) ? stage + 10 * F : nullptr;
    if (forces) *forces = (stage && fv && N) ? stage + 10 * F + N : nullptr;
  });
}

int ta_step(ta_handle h, const double *positions, const double *cells, uint32_t want, double *energy,
            double *forces, double *virial, double *atomic, int32_t *rebuilt) {
  int rc = ta_update_positions(h, positions, cells, rebuilt);
  if (rc != TA_OK) return rc;
  h->mirror_next = true;
  rc = ta_compute(h, want);
  h->mirror_next = false;
  if (rc != TA_OK) return rc;
  return ta_get_results(h, energy, forces, virial, atomic, nullptr);
}

int ta_step_view(ta_handle h, const double *positions, const double *cells, uint32_t want, const double **energy,
                 const double **forces, const double **virial, const double **atomic, int32_t *rebuilt) {
  int rc = ta_update_positions(h, positions, cells, rebuilt);
  if (rc != TA_OK) return rc;
  h->mirror_next = true;
  rc = ta_compute(h, want);
  h->mirror_next = false;
  if (rc != TA_OK) return rc;
  return ta_view_results(h, want, energy, forces, virial, atomic);
}

int ta_eval(ta_handle h, int32_t n_frames, const ta_frame *frames, uint32_t want, double *energy,
            double *forces, double *virial, double *atomic) {
  int rc = ta_set_frames(h, n_frames, frames, nullptr);
  if (rc != TA_OK) return rc;
  rc = ta_compute(h, want);
  if (rc != TA_OK) return rc;
  return ta_get_results(h, energy, forces, virial, atomic, nullptr);
}

int ta_time_compute(ta_handle h, uint32_t want, int32_t warmup, int32_t steps, double *total_ms,
                    double *kernel_ms) {
  if (!h) return TA_ERR_INVALID;
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "no resident batch");
  if (steps < 1 || warmup < 0) return fail(h, TA_ERR_INVALID, "steps must be >= 1, warmup >= 0");
  return guarded(h, [&]() {
    hipStream_t s = h->stream;
    for (int k = 0; k < warmup; ++k) compute_impl(h, want, false, nullptr);
    HIP_CHECK(hipStreamSynchronize(s));
    hipEvent_t e0 = h->ev[2 * TA_N_KERNEL_SLOTS], e1 = h->ev[2 * TA_N_KERNEL_SLOTS + 1];
    HIP_CHECK(hipEventRecord(e0, s));
    for (int k = 0; k < steps; ++k) compute_impl(h, want, false, nullptr);
    HIP_CHECK(hipEventRecord(e1, s));
    HIP_CHECK(hipStreamSynchronize(s));
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    if (total_ms) *total_ms = ms;
    if (kernel_ms) {
      double acc[TA_N_KERNEL_SLOTS] = {0};
      for (int k = 0; k < steps; ++k) compute_impl(h, want, true, acc);
      for (int k = 0; k < TA_N_KERNEL_SLOTS; ++k) kernel_ms[k] = acc[k] / steps;
    }
  });
}

int ta_batch_energy_device_ptr(ta_handle h, void **dptr) {
  if (!h || !dptr) return TA_ERR_INVALID;
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "no resident batch");
  *dptr = h->db.batch_energy;
  return TA_OK;
}

namespace {
// 16 B per lane and four independent loads in flight per lane before the first store (a one-load
// grid-stride loop reached 4.8 TB/s of the 6.3 TB/s the microarch guide measures for a float4 copy)
__global__ __launch_bounds__(256) void hbm_copy_kernel(const double2 *__restrict__ src,
                                                       double2 *__restrict__ dst, size_t n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; k + 3 * stride < n; k += 4 * stride) {
    const double2 a = src[k], b = src[k + stride], c = src[k + 2 * stride], d = src[k + 3 * stride];
    dst[k] = a;
    dst[k + stride] = b;
    dst[k + 2 * stride] = c;
    dst[k + 3 * stride] = d;
  }
  for (; k < n; k += stride) dst[k] = src[k];
}
// the same with non-temporal loads and stores (streamed once: nothing to keep in L2 / MALL)
__global__ __launch_bounds__(256) void hbm_copy_nt_kernel(const double2 *__restrict__ src,
                                                          double2 *__restrict__ dst, size_t n) {
  typedef double d2 __attribute__((ext_vector_type(2)));
  const d2 *s = reinterpret_cast<const d2 *>(src);
  d2 *d = reinterpret_cast<d2 *>(dst);
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; k + 3 * stride < n; k += 4 * stride) {
    const d2 a = __builtin_nontemporal_load(s + k), b = __builtin_nontemporal_load(s + k + stride),
             c = __builtin_nontemporal_load(s + k + 2 * stride), e = __builtin_nontemporal_load(s + k + 3 * stride);
    __builtin_nontemporal_store(a, d + k);
    __builtin_nontemporal_store(b, d + k + stride);
    __builtin_nontemporal_store(c, d + k + 2 * stride);
    __builtin_nontemporal_store(e, d + k + 3 * stride);
  }
  for (; k < n; k += stride) d[k] = s[k];
}
}  // namespace

namespace {
// unordered {j, k} of one centre with r_ij, r_ik and r_jk all below acut: the triples whose G4 term
// is not identically zero (one wavefront per centre, lane a walks b > a; reads the pair records)
// `owned`: only the triples whose centre owns the triangle (ta::owns_triangle)
__global__ __launch_bounds__(256) void count_triples_kernel(ta::DeviceBatch b, double ac2, double eps,
                                                            unsigned long long *out, int owned) {
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (i >= b.n_atoms) return;
  const int p0 = b.pair_start[i], p1 = ta::pair_stop_of(b, i);
  unsigned long long n = 0;
  for (int pa = p0 + lane; pa < p1; pa += 64) {
    const double2 *ra = ta::pair_geom(b, (size_t)pa);
    const double ax = ra[0].x, ay = ra[0].y, az = ra[1].x;
    if (!(ra[1].y < ac2)) continue;
    for (int pb = pa + 1; pb < p1; ++pb) {
      const double2 *rb = ta::pair_geom(b, (size_t)pb);
      const double ex = rb[0].x - ax, ey = rb[0].y - ay, ez = rb[1].x - az;
      n += (rb[1].y < ac2 && ex * ex + ey * ey + ez * ez + eps < ac2 &&
            (!owned || ta::owns_triangle((int32_t)i, b.pair_j[pa], b.pair_j[pb]))) ? 1ull : 0ull;
    }
  }
  for (int off = 32; off; off >>= 1) n += __shfl_xor(n, off);
  if (lane == 0 && n) atomicAdd(out, n);
}
}  // namespace

int ta_count_contributing_triples(ta_handle h, int64_t *n_contributing) {
  if (!h || !n_contributing) return fail(h, TA_ERR_INVALID, "null argument");
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "no resident batch");
  if (h->kind != TA_MODEL_SF_MLP || !h->sf.angular)
    return fail(h, TA_ERR_INVALID, "only symmetry-function models with angular terms have triples");
  return guarded(h, [&]() {
    compute_impl(h, TA_WANT_ENERGY, false, nullptr);  // fills the pair records
    h->nl_stats.ensure(8);
    hipStream_t s = h->stream;
    HIP_CHECK(hipMemsetAsync(h->nl_stats.ptr, 0, sizeof(unsigned long long), s));
    const int64_t N = h->db.n_atoms;
    if (N)
      hipLaunchKernelGGL(count_triples_kernel, dim3((unsigned)((N * 64 + 255) / 256)), dim3(256), 0, s, h->db,
                         h->sf.acut * h->sf.acut, h->sf.eps, h->nl_stats.ptr, 0);
    HIP_CHECK(hipGetLastError());
    unsigned long long v = 0;
    HIP_CHECK(hipMemcpyAsync(&v, h->nl_stats.ptr, sizeof(v), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    *n_contributing = (int64_t)v;
  });
}

int ta_count_owned_triangles(ta_handle h, int64_t *n_owned) {
  if (!h || !n_owned) return fail(h, TA_ERR_INVALID, "null argument");
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "no resident batch");
  if (h->kind != TA_MODEL_SF_MLP || !h->sf.angular)
    return fail(h, TA_ERR_INVALID, "only symmetry-function models with angular terms have triples");
  return guarded(h, [&]() {
    compute_impl(h, TA_WANT_ENERGY, false, nullptr);  // fills the pair records
    h->nl_stats.ensure(8);
    hipStream_t s = h->stream;
    HIP_CHECK(hipMemsetAsync(h->nl_stats.ptr, 0, sizeof(unsigned long long), s));
    const int64_t N = h->db.n_atoms;
    if (N)
      hipLaunchKernelGGL(count_triples_kernel, dim3((unsigned)((N * 64 + 255) / 256)), dim3(256), 0, s, h->db,
                         h->sf.acut * h->sf.acut, h->sf.eps, h->nl_stats.ptr, 1);
    HIP_CHECK(hipGetLastError());
    unsigned long long v = 0;
    HIP_CHECK(hipMemcpyAsync(&v, h->nl_stats.ptr, sizeof(v), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    *n_owned = (int64_t)v;
  });
}

int ta_set_triangles(ta_handle h, int on) {
  if (!h) return TA_ERR_INVALID;
  h->triangles = on != 0;
  return TA_OK;
}

int ta_backward_variant(ta_handle h, int32_t *variant) {
  if (!h || !variant) return fail(h, TA_ERR_INVALID, "null argument");
  *variant = h->last_bwd_variant;
  return TA_OK;
}

int ta_mlp_launch_info(ta_handle h, int64_t *info) {
  if (!h || !info) return fail(h, TA_ERR_INVALID, "null argument");
  const ta::MlpLaunchInfo &m = h->last_mlp_launch;
  info[0] = m.family;
  info[1] = m.threads;
  info[2] = m.lh;
  info[3] = m.nt;
  info[4] = m.grid_x;
  info[5] = m.grid_y;
  info[6] = m.lds_bytes;
  info[7] = m.da;
  return TA_OK;
}

int ta_mlp_tile_body(ta_handle h, int32_t *body) {
  if (!h || !body) return fail(h, TA_ERR_INVALID, "null argument");
  *body = h->last_mlp_launch.body;
  return TA_OK;
}

int ta_triangle_owner(int64_t n, const int32_t *abc, int32_t *owner) {
  if (n < 0 || (n > 0 && (!abc || !owner))) return TA_ERR_INVALID;
  for (int64_t t = 0; t < n; ++t) {
    int32_t a = abc[3 * t], b = abc[3 * t + 1], c = abc[3 * t + 2];
    if (a > b) std::swap(a, b);
    if (b > c) std::swap(b, c);
    if (a > b) std::swap(a, b);
    const int32_t sorted[3] = {a, b, c};
    owner[t] = (a == b || b == c) ? -1 : sorted[ta::triangle_owner_rank((uint32_t)a + (uint32_t)b + (uint32_t)c)];
  }
  return TA_OK;
}

int ta_measure_hbm_copy(ta_handle h, int64_t bytes, int32_t reps, double *gbs) {
  if (!h || !gbs || bytes < 16 || reps < 1) return fail(h, TA_ERR_INVALID, "bad argument");
  return guarded(h, [&]() {
    const size_t n = (size_t)bytes / 16;
    double2 *src = nullptr, *dst = nullptr;
    HIP_CHECK(hipMalloc((void **)&src, n * 16));
    if (hipMalloc((void **)&dst, n * 16) != hipSuccess) {
      (void)hipFree(src);
      throw std::bad_alloc();
    }
    hipStream_t s = h->stream;
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    HIP_CHECK(hipMemsetAsync(src, 0, n * 16, s));
    const int per_cu = h->opt.copy_wg_per_cu;
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, (size_t)256 * std::max(1, per_cu));
    // three ways to copy, the fastest counts (measured on this pool: 4.8-5.2, 5.0-5.5 and 5.0-5.5 TB/s
    // read + written; the microarch guide quotes 6.29 for a float4 copy): the grid-stride kernel, the
    // runtime's device-to-device copy, the kernel with non-temporal loads and stores
    const int only = h->opt.copy_mode;
    double best = 0.0;
    for (int mode = 0; mode < 3; ++mode) {
      if (only >= 0 && mode != only) continue;
      auto one = [&]() {
        if (mode == 1) (void)hipMemcpyAsync(dst, src, n * 16, hipMemcpyDeviceToDevice, s);
        else if (mode == 2) hipLaunchKernelGGL(hbm_copy_nt_kernel, dim3(blocks), dim3(256), 0, s, src, dst, n);
        else hipLaunchKernelGGL(hbm_copy_kernel, dim3(blocks), dim3(256), 0, s, src, dst, n);
      };
      for (int k = 0; k < 2; ++k) one();
      HIP_CHECK(hipEventRecord(e0, s));
      for (int k = 0; k < reps; ++k) one();
      HIP_CHECK(hipEventRecord(e1, s));
      HIP_CHECK(hipEventSynchronize(e1));
      float ms = 0.f;
      HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
      if (ms > 0.f) best = std::max(best, 2.0 * (double)(n * 16) * reps / (ms * 1e-3) / 1e9);
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipFree(src);
    (void)hipFree(dst);
    *gbs = best;
  });
}

int ta_set_stream(ta_handle h, void *stream) {
  if (!h) return TA_ERR_INVALID;
  return guarded(h, [&]() {
    HIP_CHECK(hipStreamSynchronize(h->stream));
    h->upload_pending = false;
    h->stream = stream ? (hipStream_t)stream : h->own_stream;
  });
}

int ta_copy_batch_energy(ta_handle h, void *dst_device) {
  if (!h || !dst_device) return TA_ERR_INVALID;
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "no resident batch");
  return guarded(h, [&]() {
    HIP_CHECK(hipMemcpyAsync(dst_device, h->db.batch_energy, sizeof(double),
                             hipMemcpyDeviceToDevice, h->stream));
  });
}

int ta_set_batch_energy_target(ta_handle h, void *dst_device) {
  if (!h) return TA_ERR_INVALID;
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "no resident batch");
  // no synchronisation: only launches made after this call see the new target
  h->db.batch_energy = dst_device ? static_cast<double *>(dst_device) : h->benergy.ptr;
  return TA_OK;
}

int ta_neighbor_list(const ta_frame *frame, int32_t n_elements, double rc, int64_t *n_pairs,
                     int32_t **i, int32_t **j, int32_t **shift, int32_t **rev) {
  if (!frame || !n_pairs || n_elements < 1 || !(rc > 0.0))
    return fail(nullptr, TA_ERR_INVALID, "bad argument");
  try {
    ta::HostPairs hp;
    ta::build_pairs(1, frame, n_elements, rc, hp);
    const size_t P = (size_t)hp.n_pairs;
    *n_pairs = hp.n_pairs;
    auto dup = [&](const std::vector<int32_t> &v) {
      int32_t *p = (int32_t *)std::malloc((v.size() ? v.size() : 1) * sizeof(int32_t));
      if (!p) throw std::bad_alloc();
      if (!v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(int32_t));
      return p;
    };
    (void)P;
    if (i) *i = dup(hp.pair_i);
    if (j) *j = dup(hp.pair_j);
    if (shift) *shift = dup(hp.pair_shift);
    if (rev) *rev = dup(hp.pair_rev);
    return TA_OK;
  } catch (const std::bad_alloc &) {
    return fail(nullptr, TA_ERR_NOMEM, "host allocation failed");
  } catch (const std::exception &e) {
    return fail(nullptr, TA_ERR_INVALID, e.what());
  }
}

void ta_free(void *p) { std::free(p); }

int ta_eam_tabulate(ta_handle h, int32_t n_r, const double *r, int32_t n_rho, const double *rho,
                    double *rho_of_r, double *phi_of_r, double *embed_of_rho, double *u_of_r,
                    double *w_of_r) {
  if (!h) return TA_ERR_INVALID;
  if (h->kind != TA_MODEL_EAM_ALLOY && h->kind != TA_MODEL_EAM_ADP && h->kind != TA_MODEL_EAM_FS)
    return fail(h, TA_ERR_INVALID, "ta_eam_tabulate needs an EAM / ADP model");
  if (n_r < 0 || n_rho < 0 || (n_r > 0 && (!r || !rho_of_r || !phi_of_r)) ||
      (n_rho > 0 && (!rho || !embed_of_rho)))
    return fail(h, TA_ERR_INVALID, "bad table arguments");
  return guarded(h, [&]() {
    const size_t nel = (size_t)h->n_elements, npair = nel * (nel + 1) / 2;
    const size_t nrho = h->kind == TA_MODEL_EAM_FS ? nel * nel : nel;  // eam/fs: rho[centre][neighbour]
    const bool adp = h->kind == TA_MODEL_EAM_ADP && u_of_r && w_of_r;
    DevBuf<double> buf;
    const size_t n_in = (size_t)n_r + (size_t)n_rho;
    const size_t n_out = (nrho + npair * (adp ? 3 : 1)) * (size_t)n_r + nel * (size_t)n_rho;
    buf.ensure(n_in + n_out + 8);
    double *d_r = buf.ptr, *d_rho = d_r + n_r;
    double *d_rho_r = d_rho + n_rho, *d_phi = d_rho_r + nrho * n_r, *d_embed = d_phi + npair * n_r;
    double *d_u = adp ? d_embed + nel * n_rho : nullptr, *d_w = adp ? d_u + npair * n_r : nullptr;
    hipStream_t s = h->stream;
    if (n_r) HIP_CHECK(hipMemcpyAsync(d_r, r, (size_t)n_r * sizeof(double), hipMemcpyHostToDevice, s));
    if (n_rho) HIP_CHECK(hipMemcpyAsync(d_rho, rho, (size_t)n_rho * sizeof(double), hipMemcpyHostToDevice, s));
    ta::eam_tabulate(h->eam, n_r, d_r, n_rho, d_rho, d_rho_r, d_phi, d_embed, d_u, d_w, s);
    HIP_CHECK(hipGetLastError());
    auto back = [&](double *dst, const double *src, size_t n) {
      if (dst && n) HIP_CHECK(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToHost, s));
    };
    back(rho_of_r, d_rho_r, nrho * n_r);
    back(phi_of_r, d_phi, npair * n_r);
    back(embed_of_rho, d_embed, nel * n_rho);
    if (adp) {
      back(u_of_r, d_u, npair * n_r);
      back(w_of_r, d_w, npair * n_r);
    }
    HIP_CHECK(hipStreamSynchronize(s));
  });
}

int ta_get_pairs(ta_handle h, int32_t *i, int32_t *j, int32_t *shift) {
  if (!h) return TA_ERR_INVALID;
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "no resident batch");
  const size_t P = (size_t)h->hp.n_pairs;
  if (h->pairs_on_device) {
    return guarded(h, [&]() {
      HIP_CHECK(hipStreamSynchronize(h->stream));
      // the RESIDENT list (n_pairs of ta_batch_info): under a Verlet skin that is the skin list, not
      // the exact list the kernels extract from it per step (whose arrays are defined only up to
      // their own, smaller count)
      const int32_t *pi = h->filtered ? h->pair_i.ptr : h->db.pair_i;
      const int32_t *pj = h->filtered ? h->pair_j.ptr : h->db.pair_j;
      const int32_t *ps = h->filtered ? h->pair_shift.ptr : h->db.pair_shift;
      if (i && P) HIP_CHECK(hipMemcpy(i, pi, P * sizeof(int32_t), hipMemcpyDeviceToHost));
      if (j && P) HIP_CHECK(hipMemcpy(j, pj, P * sizeof(int32_t), hipMemcpyDeviceToHost));
      if (shift && P) HIP_CHECK(hipMemcpy(shift, ps, 3 * P * sizeof(int32_t), hipMemcpyDeviceToHost));
    });
  }
  if (i) std::memcpy(i, h->hp.pair_i.data(), P * sizeof(int32_t));
  if (j) std::memcpy(j, h->hp.pair_j.data(), P * sizeof(int32_t));
  if (shift) std::memcpy(shift, h->hp.pair_shift.data(), 3 * P * sizeof(int32_t));
  return TA_OK;
}

// which == TA_LIST_KERNEL on a skin-filtered batch: the exact list (ex_* arrays); else the resident one
static bool list_view_is_exact(const ta_context *h, int32_t which) { return which == TA_LIST_KERNEL && h->filtered; }

int ta_list_info(ta_handle h, int32_t which, int64_t *info) {
  if (!h || !info) return fail(h, TA_ERR_INVALID, "null argument");
  if (which != TA_LIST_RESIDENT && which != TA_LIST_KERNEL) return fail(h, TA_ERR_INVALID, "ta_list_info: unknown view");
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "no resident batch");
  const bool exact = list_view_is_exact(h, which);
  info[0] = h->hp.n_atoms;
  info[1] = h->n_elements;
  info[2] = h->hp.n_pairs;  // the exact list is compacted in place: same slots, some unused
  info[3] = exact ? (h->kind == TA_MODEL_SF_MLP ? h->db.n_blk : 0) : h->res_n_blk;
  info[4] = h->db.cap;
  info[5] = h->pairs_on_device ? (h->nl_sorted ? 1 : 2) : 0;
  info[6] = exact ? 1 : 0;
  info[7] = exact && h->db.slot_q ? 1 : 0;
  return TA_OK;
}

int ta_get_list(ta_handle h, int32_t which, int32_t *pair_start, int32_t *pair_stop, int32_t *seg_start,
                int32_t *pair_i, int32_t *pair_j, int32_t *pair_shift, int32_t *pair_rev, int32_t *blk_center) {
  if (!h) return TA_ERR_INVALID;
  if (which != TA_LIST_RESIDENT && which != TA_LIST_KERNEL) return fail(h, TA_ERR_INVALID, "ta_get_list: unknown view");
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "no resident batch");
  return guarded(h, [&]() {
    const bool exact = list_view_is_exact(h, which);
    const size_t N = (size_t)h->hp.n_atoms, P = (size_t)h->hp.n_pairs, nseg = N * (size_t)(h->n_elements + 1);
    HIP_CHECK(hipStreamSynchronize(h->stream));
    auto get = [&](int32_t *dst, const int32_t *src, size_t n) {
      if (dst && n) HIP_CHECK(hipMemcpy(dst, src, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    };
    // starts and stops are needed here as well (closing entries, the indirect reverse index)
    std::vector<int32_t> start(N + 1, 0), stop(N, 0);
    get(start.data(), exact ? h->ex_pair_start.ptr : h->pair_start.ptr, exact ? N : N + 1);
    if (exact) {
      start[N] = (int32_t)P;  // where a further group would begin: the end of the skin list
      get(stop.data(), h->ex_pair_stop.ptr, N);
    } else {
      for (size_t i = 0; i < N; ++i) stop[i] = start[i + 1];
    }
    if (pair_start) std::memcpy(pair_start, start.data(), (N + 1) * sizeof(int32_t));
    if (pair_stop && N) std::memcpy(pair_stop, stop.data(), N * sizeof(int32_t));
    if (seg_start) {
      // the closing entry: the device builders write one, read as it stands; the host builder and the filter
      // keep none, there it is the last centre's stop
      const bool dev_close = !exact && h->pairs_on_device && N;
      get(seg_start, exact ? h->ex_seg_start.ptr : h->seg_start.ptr, nseg + (dev_close ? 1 : 0));
      if (!dev_close) seg_start[nseg] = N ? stop[N - 1] : 0;
    }
    get(pair_i, exact ? h->ex_pair_i.ptr : h->pair_i.ptr, P);
    get(pair_j, exact ? h->ex_pair_j.ptr : h->pair_j.ptr, P);
    get(pair_shift, exact ? h->ex_pair_shift.ptr : h->pair_shift.ptr, 3 * P);
    if (pair_rev && P) {
      if (exact && h->db.slot_q) {
        // pair_rev_of (ta_device.h) on the host, for the slots some centre owns
        std::vector<int32_t> slot_q(P), rev_super(P), rev_map(P);
        get(slot_q.data(), h->db.slot_q, P);
        get(rev_super.data(), h->db.rev_super, P);
        get(rev_map.data(), h->db.rev_map, P);
        for (size_t p = 0; p < P; ++p) pair_rev[p] = -1;
        for (size_t i = 0; i < N; ++i)
          for (int32_t p = start[i]; p < stop[i]; ++p) {
            const int32_t q = (p >= 0 && (size_t)p < P) ? slot_q[p] : -1;
            const int32_t r = (q >= 0 && (size_t)q < P) ? rev_super[q] : -1;
            if (p >= 0 && (size_t)p < P) pair_rev[p] = (r >= 0 && (size_t)r < P) ? rev_map[r] : -1;
          }
      } else {
        get(pair_rev, exact ? h->ex_pair_rev.ptr : h->pair_rev.ptr, P);
      }
    }
    if (blk_center) {
      if (exact) {
        if (h->kind == TA_MODEL_SF_MLP) get(blk_center, h->ex_blk.ptr, (size_t)h->db.n_blk + 1);
      } else if (h->res_n_blk > 0) {
        get(blk_center, reinterpret_cast<const int32_t *>(h->inbuf.ptr + h->o_blk), (size_t)h->res_n_blk + 1);
      }
    }
  });
}

}  // extern "C"
