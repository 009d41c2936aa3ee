// C ABI, the derivative half: weights, filter networks and constants as parameters, their loss gradients, and the
// Hessian-vector products. Nothing here is on the step path (ta_api.hip), which calls none of it.
//
// The entry points share grow-only buffers on the handle. Who sizes what, before its first launch that reads it:
//   train_grad                   every gradient entry point: its parameter count (+ 8)
//   train_coeff                  upload_frame_coeff: F doubles, 3 F for the temperature-dependent [a | b | g]
//   train_scratch, train_partial ensure_mlp_grad_buffers (first or second order, largest element); the
//                                temperature-dependent path by td_grad2_sizes; the EAM gradients keep their own
//   tan_dir                      upload_direction: 3 N + 9 F; ta_hessian_vectors of the descriptor models likewise
//   tan_dD, tan_dG               ensure_tangents: 4 P and N D
//   jvp_J                        ensure_pair_jacobians: D 4 P, valid while jvp_valid (one batch, one filter network)
//   filt_scratch                 ta_grap_loss_gradient; hvp_buf: the two branches of ta_hessian_vectors, each its layout
// Every entry point calls ensure on every buffer it reads and refills it: it assumes nothing about the caller before
// it, neither sizes nor contents (DevBuf::ensure carries no contents over). tests/test_gpu_train_entries.py holds
// every entry point to that, in both orders and across a larger batch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "ta_context.h"

using namespace ta::host;

namespace {

int64_t mlp_params(const ta_context *h) {
  int64_t n = 0;
  for (int e = 0; e < h->n_elements; ++e) n += ta::mlp_param_count(h->mlp[e]);
  return n;
}

// Per-pair buffers of these entries (tangents, Jacobian) are sized and walked by the resident
// list's pair count. Under a Verlet skin the kernels run on the exact list extracted from it
// (apply_filter: only the first pair_start[N] entries of the ex_* arrays are defined), so the two
// do not match: refuse instead of reading the undefined tail. Training never needs a skin.
std::string filtered_refusal(const char *who) {
  return std::string(who) + ": not available on a skin-filtered batch; ta_set_skin(h, 0) and ta_set_frames first";
}

std::string expected_room(const char *who, int64_t n) {
  return std::string(who) + ": expected room for " + std::to_string(n) + " values";
}

// one network's weights from the flat layout (per layer W[k][n] then b[n]) into its padded device copies,
// both orientations; `src` advances past them
void upload_net_weights(ta::MlpDev &md, const double *&src) {
  for (int l = 0; l < md.n_layers; ++l) {
    ta::MlpLayerDev &ly = md.layer[l];
    std::vector<double> w((size_t)ly.kp * ly.np, 0.0), wt((size_t)ly.np * ly.kp, 0.0), bb(ly.np, 0.0);
    for (int k = 0; k < ly.k; ++k)
      for (int n = 0; n < ly.n; ++n) {
        const double v = src[(size_t)k * ly.n + n];
        w[(size_t)k * ly.np + n] = v;
        wt[(size_t)n * ly.kp + k] = v;
      }
    src += (size_t)ly.k * ly.n;
    for (int n = 0; n < ly.n; ++n) bb[n] = src[n];
    src += ly.n;
    HIP_CHECK(hipMemcpy(ly.w, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(ly.wt, wt.data(), wt.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(ly.b, bb.data(), bb.size() * sizeof(double), hipMemcpyHostToDevice));
  }
}

// the evaluation of a GRAP filter network changed (table <-> exact): what either left behind is stale, and
// the exact evaluation needs its per-pair buffer
void grap_filter_mode_changed(ta_context *h) {
  h->descriptors_valid = false;
  h->jvp_valid = false;
  if (h->have_batch) ta::grap_ensure(h->grap, h->db);
}
// Weight gradients and training differentiate the filter network itself (Hbuf, Jacobians of the exact
// filters): the handle evaluates it exactly from here on, as an EAM handle does its nn pair functions
void mark_grap_trained(ta_context *h) {
  if (h->kind != TA_MODEL_GRAP_MLP || !h->grap || !ta::grap_uses_filter_net(h->grap)) return;
  const bool was_on = ta::grap_filter_table_knots(h->grap) != 0;
  if (was_on) HIP_CHECK(hipStreamSynchronize(h->stream));
  ta::grap_mark_trained(h->grap);
  if (was_on) grap_filter_mode_changed(h);
}
// Gradients differentiate the networks of an EAM / ADP model themselves: from here on the handle evaluates its nn
// pair functions exactly, not through their tables (eam_set_nn_tables), into the per-pair columns of that evaluation
void eam_exact_networks(ta_context *h) {
  if (ta::eam_nn_tables_on(h->eam)) HIP_CHECK(hipStreamSynchronize(h->stream));
  ta::eam_mark_trained(h->eam);
  ta::eam_ensure(h->eam, h->db);
}

// The dE/dD launches of the resident batch alone, on the dE/dG that is in `db.dEdG` (the forward pass of this
// batch has run: pair records, candidate masks and, for GRAP, the moments are resident). A copy of the backward
// launches of compute_impl on purpose: compute_impl is the measured step path and takes no branch for a caller
// that wants part of it; this one runs once per descriptor channel and batch, always per apex (no triangle
// build), and never timed. A change of a backward launch's arguments there is a change here.
void backward_only(ta_context *h) {
  using namespace ta;
  const DeviceBatch &db = h->db;
  hipStream_t s = h->stream;
  if (h->kind == TA_MODEL_SF_MLP) {
    if (h->sf.angular) {
      bool first = true;
      if (h->use_v2) {
        // the per-apex kernel walks the FULL job list of the resident forward pass; an evaluation whose
        // backward launches were all triangle builds left none, so the forward launches run again and write it
        // (same geometry, same descriptors; dE/dG is the caller's and stays)
        if (db.job_count && !h->full_jobs_valid) forward_v2_launches(h, false);
        for (const ChunkPlan &cp : h->chunks_v2) {
          // per apex: the callers keep g[p] per pair (J[c][p]), which the triangle pass distributes differently
          launch_backward_v2(h->sf, cp.ch, cp.ng, cp.nz, first, false, db, h->opt, s);
          first = false;
        }
      } else
        for (const ChunkPlan &cp : h->chunks) {
          launch_backward(h->sf, cp.ch, cp.nb, cp.ng, cp.nz, first, false, db, s);
          first = false;
        }
    } else {
      AngChunk dummy;
      std::memset(&dummy, 0, sizeof(dummy));
      launch_backward(h->sf, dummy, 1, 1, 1, true, true, db, s);
    }
  } else {
    launch_grap_backward(h->grap, db, s);
  }
}
// J[c][p] = dG_{i(p), c} / dD_p of the resident batch: the backward kernels with a one-hot dE/dG, once per
// channel and once per batch (ta_loss_gradient, ta_hessian_vectors of the descriptor models)
void ensure_pair_jacobians(ta_context *h) {
  hipStream_t s = h->stream;
  const size_t N = (size_t)h->db.n_atoms, P = (size_t)h->db.n_pairs;
  const int D = h->sf.ndim;
  if (!h->descriptors_valid || !h->jvp_valid)
    compute_impl(h, TA_WANT_ENERGY, false, nullptr);  // pair records, masks, moments, descriptors
  if (h->jvp_valid) return;
  h->jvp_J.ensure((size_t)D * 4 * P + 8);
  for (int c = 0; c < D; ++c) {
    ta::launch_one_hot(h->db.dEdG, (int64_t)N, D, c, s);
    backward_only(h);
    if (P)
      HIP_CHECK(hipMemcpyAsync(h->jvp_J.ptr + (size_t)c * 4 * P, h->db.g, 4 * P * sizeof(double),
                               hipMemcpyDeviceToDevice, s));
  }
  HIP_CHECK(hipGetLastError());
  h->jvp_valid = true;
}

// what becomes of the half of a direction (dR [N][3], dh [F][9]) that the caller left out
enum class Absent {
  stays_null,   // the kernel takes a null for "no such term" (eam_loss_gradient)
  zero_beside,  // zeroed beside the other half; without either, both stay null and nothing is touched
  zeroed,       // zeroed: the kernel reads both halves
};
struct Direction {
  double *dR, *dh;
};
Direction upload_direction(ta_context *h, const double *dR, const double *dh, Absent absent) {
  if (absent == Absent::zero_beside && !dR && !dh) return {nullptr, nullptr};
  hipStream_t s = h->stream;
  const size_t N = (size_t)h->db.n_atoms, F = (size_t)h->db.n_frames;
  h->tan_dir.ensure(3 * N + 9 * F + 8);
  double *d_dR = h->tan_dir.ptr, *d_dh = h->tan_dir.ptr + 3 * N;
  const bool zero = absent != Absent::stays_null;
  if (dR) HIP_CHECK(hipMemcpyAsync(d_dR, dR, 3 * N * sizeof(double), hipMemcpyHostToDevice, s));
  else if (zero) HIP_CHECK(hipMemsetAsync(d_dR, 0, 3 * N * sizeof(double), s));
  if (dh) HIP_CHECK(hipMemcpyAsync(d_dh, dh, 9 * F * sizeof(double), hipMemcpyHostToDevice, s));
  else if (zero) HIP_CHECK(hipMemsetAsync(d_dh, 0, 9 * F * sizeof(double), s));
  return {dR || zero ? d_dR : nullptr, dh || zero ? d_dh : nullptr};
}

// The loss coefficients of the frames, `n_rows` host rows of F, into train_coeff. One row (dL/dE_f): absent in,
// null out, which the kernels take for "no energy term". Three rows, [a | b | g] = dL/dU_f, dL/dF_f, dL/dS_f of the
// temperature-dependent loss: the kernel reads them all, an absent row is zeroed.
double *upload_frame_coeff(ta_context *h, const double *const *rows, int n_rows) {
  hipStream_t s = h->stream;
  const size_t F = (size_t)h->db.n_frames;
  h->train_coeff.ensure((size_t)n_rows * F + 8);
  if (n_rows == 1 && !rows[0]) return nullptr;
  for (int q = 0; q < n_rows && F; ++q) {
    double *dst = h->train_coeff.ptr + q * F;
    if (rows[q]) HIP_CHECK(hipMemcpyAsync(dst, rows[q], F * sizeof(double), hipMemcpyHostToDevice, s));
    else HIP_CHECK(hipMemsetAsync(dst, 0, F * sizeof(double), s));
  }
  return h->train_coeff.ptr;
}

void ensure_tangents(ta_context *h) {
  h->tan_dD.ensure(4 * (size_t)h->db.n_pairs + 8);
  h->tan_dG.ensure((size_t)h->db.n_atoms * (size_t)h->sf.ndim + 8);
}
// direction -> pairs -> descriptors: G-dot of (dR, dh) in tan_dG, through the pair Jacobians
void descriptor_tangent(ta_context *h, const double *dR, const double *dh) {
  ensure_pair_jacobians(h);
  ensure_tangents(h);
  const Direction d = upload_direction(h, dR, dh, Absent::zeroed);
  ta::launch_pair_tangent(h->db, d.dR, d.dh, h->tan_dD.ptr, h->stream);
  ta::launch_descriptor_jvp(h->db, h->sf.ndim, h->jvp_J.ptr, h->tan_dD.ptr, h->tan_dG.ptr, h->stream);
}

// scratch and partial sums of the per-element weight-gradient passes (the largest element), and the gradient
void ensure_mlp_grad_buffers(ta_context *h, bool second_order) {
  size_t scratch = 0, partial = 0;
  for (int e = 0; e < h->n_elements; ++e) {
    const int n_el = h->db.elem_start[e + 1] - h->db.elem_start[e];
    scratch = std::max(scratch, second_order ? ta::mlp_grad2_scratch_doubles(h->mlp[e], n_el)
                                             : ta::mlp_grad_scratch_doubles(h->mlp[e], n_el));
    partial = std::max(partial, ta::mlp_grad_partial_doubles(h->mlp[e], n_el));
  }
  h->train_scratch.ensure(scratch + 8);
  h->train_partial.ensure(partial + 8);
  h->train_grad.ensure((size_t)mlp_params(h) + 8);
}
// one second-order pass per element on the descriptor tangent dG: the elements' gradients one after the other in
// train_grad; `extra` [N][D]: kappa = c w + H_mlp G-dot (w-dot without coefficients), or null
void launch_mlp_grad2_all(ta_context *h, const double *dG, const double *coeff, double *extra) {
  size_t off = 0;
  for (int e = 0; e < h->n_elements; ++e) {
    const int n_el = h->db.elem_start[e + 1] - h->db.elem_start[e];
    ta::launch_mlp_grad2(h->mlp[e], h->activation, h->sf.ndim, h->db.elem_atoms + h->db.elem_start[e], n_el, h->db, dG,
                         coeff, h->train_scratch.ptr, h->train_partial.ptr, h->train_grad.ptr + off, h->stream, extra);
    off += (size_t)ta::mlp_param_count(h->mlp[e]);
  }
}

// How every gradient entry point ends: the launches' error state, the first n of train_grad to the host, with `dG_out`
// the descriptor tangent [N][D] behind them, and the wait. `wait` = false: the caller enqueues more and waits itself.
void download_grad(ta_context *h, double *grad, int64_t n, double *dG_out = nullptr, bool wait = true) {
  hipStream_t s = h->stream;
  const size_t N = (size_t)h->db.n_atoms;
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(grad, h->train_grad.ptr, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
  if (dG_out && N)
    HIP_CHECK(hipMemcpyAsync(dG_out, h->tan_dG.ptr, N * (size_t)h->sf.ndim * sizeof(double), hipMemcpyDeviceToHost, s));
  if (wait) HIP_CHECK(hipStreamSynchronize(s));
}

// dW [n_dir][F][9]: the per-frame sums of per-atom virial rows [n_dir][N][9], in atom order
void frame_sums_of_rows(const ta_context *h, const double *rows, size_t n_dir, double *dW) {
  const size_t N = (size_t)h->db.n_atoms, F = (size_t)h->db.n_frames;
  const std::vector<int32_t> &foa = h->hp.frame_of_atom;
  std::fill(dW, dW + n_dir * F * 9, 0.0);
  for (size_t d = 0; d < n_dir; ++d)
    for (size_t i = 0; i < N; ++i)
      for (int k = 0; k < 9; ++k) dW[(d * F + (size_t)foa[i]) * 9 + k] += rows[(d * N + i) * 9 + k];
}

// ta_hessian_vectors of the descriptor + MLP models. Per direction: D-dot per pair, G-dot through the pair
// Jacobians, w-dot = H_mlp G-dot from the second-order MLP pass, then g and g-dot from the dual-arithmetic
// backward expression (ta_hvp.hip).
void hvp_descriptor_models(ta_context *h, int32_t n_dir, int32_t first, const double *dR, const double *dh, double *dF,
                           double *dW, double *dF_dev) {
  const size_t N = (size_t)h->db.n_atoms, F = (size_t)h->db.n_frames;
  if (n_dir == 0 || N == 0) return;
  const bool grap_model = h->kind == TA_MODEL_GRAP_MLP, unit = !dR && !dh;
  hipStream_t s = h->stream;
  const size_t P = (size_t)h->db.n_pairs, nd = (size_t)n_dir;
  const int D = h->sf.ndim;
  // The pair Jacobians and the second derivatives are those of the exact filter network: a handle with the
  // filter table on evaluates exactly for the duration of this call (same result as one that never had a
  // table) and takes the table up again afterwards, with nothing of either evaluation left valid.
  struct ExactFilters {
    ta_context *h;
    bool resume;
    ~ExactFilters() {
      if (!resume) return;
      (void)hipStreamSynchronize(h->stream);
      ta::grap_suspend_filter_tables(h->grap, false);
      h->descriptors_valid = false;
      h->jvp_valid = false;
    }
  } exact{h, grap_model && ta::grap_filter_table_knots(h->grap) != 0};
  if (exact.resume) {
    HIP_CHECK(hipStreamSynchronize(s));
    ta::grap_suspend_filter_tables(h->grap, true);
    grap_filter_mode_changed(h);
  }
  ensure_pair_jacobians(h);
  compute_impl(h, TA_WANT_ENERGY, false, nullptr);  // dE/dG of the resident positions (the one-hots overwrote it)
  ensure_mlp_grad_buffers(h, true);
  h->tan_dir.ensure(3 * N + 9 * F + 8);
  ensure_tangents(h);
  // Dv, gv, gd [P][4]; w-dot [N][D]; F-dot [N][3], W-dot rows [N][9] of one direction
  h->hvp_buf.ensure(12 * P + N * (size_t)D + 12 * N + 64);
  double *Dv = h->hvp_buf.ptr, *gv = Dv + 4 * P, *gd = gv + 4 * P, *wdot = gd + 4 * P, *fdot = wdot + N * (size_t)D,
         *wrow = fdot + 3 * N;
  ta::launch_pair_vec(h->db, Dv, s);
  std::vector<double> dir_R(3 * N), dir_h(9 * F), rows(9 * N);
  double *d_dR = h->tan_dir.ptr, *d_dh = h->tan_dir.ptr + 3 * N;
  for (size_t d = 0; d < nd; ++d) {
    if (unit) {
      std::fill(dir_R.begin(), dir_R.end(), 0.0);
      dir_R[(size_t)first + d] = 1.0;
    } else if (dR) {
      std::copy(dR + d * 3 * N, dR + (d + 1) * 3 * N, dir_R.begin());
    } else {
      std::fill(dir_R.begin(), dir_R.end(), 0.0);
    }
    if (dh) std::copy(dh + d * 9 * F, dh + (d + 1) * 9 * F, dir_h.begin());
    else std::fill(dir_h.begin(), dir_h.end(), 0.0);
    HIP_CHECK(hipMemcpyAsync(d_dR, dir_R.data(), 3 * N * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_dh, dir_h.data(), 9 * F * sizeof(double), hipMemcpyHostToDevice, s));
    ta::launch_pair_tangent(h->db, d_dR, d_dh, h->tan_dD.ptr, s);
    ta::launch_descriptor_jvp(h->db, D, h->jvp_J.ptr, h->tan_dD.ptr, h->tan_dG.ptr, s);
    launch_mlp_grad2_all(h, h->tan_dG.ptr, nullptr, wdot);
    if (grap_model) {
      ta::launch_grap_hvp(h->grap, h->db, h->sf.eps, Dv, h->tan_dD.ptr, wdot, gv, gd, s);
    } else if (h->sf.angular) {
      bool first_launch = true;
      for (const ChunkPlan &cp : h->chunks) {
        ta::launch_backward_hvp(h->sf, cp.ch, cp.nb, cp.ng, cp.nz, first_launch, true, h->db, Dv, h->tan_dD.ptr, wdot,
                                gv, gd, s);
        first_launch = false;
      }
    } else {
      ta::AngChunk dummy;
      std::memset(&dummy, 0, sizeof(dummy));
      ta::launch_backward_hvp(h->sf, dummy, 1, 1, 1, true, false, h->db, Dv, h->tan_dD.ptr, wdot, gv, gd, s);
    }
    ta::launch_hvp_gather(h->db, Dv, h->tan_dD.ptr, gv, gd, fdot, dW ? wrow : nullptr, s);
    HIP_CHECK(hipGetLastError());
    if (dF) HIP_CHECK(hipMemcpyAsync(dF + d * 3 * N, fdot, 3 * N * sizeof(double), hipMemcpyDeviceToHost, s));
    if (dF_dev) HIP_CHECK(hipMemcpyAsync(dF_dev + d * 3 * N, fdot, 3 * N * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (dW) HIP_CHECK(hipMemcpyAsync(rows.data(), wrow, 9 * N * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));  // (the direction buffers are reused)
    if (dW) frame_sums_of_rows(h, rows.data(), 1, dW + d * F * 9);
  }
}

// ta_hessian_vectors of the EAM / ADP models: every direction in one set of launches (ta_eam.hip::eam_hvp)
void hvp_eam(ta_context *h, int32_t n_dir, int32_t first, const double *dR, const double *dh, double *dF, double *dW,
             double *dF_dev) {
  const size_t N = (size_t)h->db.n_atoms, F = (size_t)h->db.n_frames;
  if (n_dir == 0 || N == 0) return;
  hipStream_t s = h->stream;
  compute_impl(h, TA_WANT_ENERGY, false, nullptr);  // F'(rho_i) of the resident positions
  const size_t nd = (size_t)n_dir;
  const size_t extra_n = ta::eam_hvp_extra_doubles(h->eam, h->db, n_dir);
  h->hvp_buf.ensure(nd * N * (1 + 3 + (dW ? 9 : 0)) + (dR ? nd * N * 3 : 0) + (dh ? nd * F * 9 : 0) + extra_n + 8);
  double *p = h->hvp_buf.ptr;
  double *extra = extra_n ? p : nullptr;
  p += extra_n;
  double *dFdot = p; p += nd * N;
  double *fdot = p; p += nd * N * 3;
  double *wdot = nullptr;
  if (dW) { wdot = p; p += nd * N * 9; }
  double *d_dR = nullptr, *d_dh = nullptr;
  if (dR) {
    d_dR = p; p += nd * N * 3;
    HIP_CHECK(hipMemcpyAsync(d_dR, dR, nd * N * 3 * sizeof(double), hipMemcpyHostToDevice, s));
  }
  if (dh) {
    d_dh = p; p += nd * F * 9;
    HIP_CHECK(hipMemcpyAsync(d_dh, dh, nd * F * 9 * sizeof(double), hipMemcpyHostToDevice, s));
  }
  ta::eam_hvp(h->eam, h->db, n_dir, !dR && !dh, first, d_dR, d_dh, dFdot, fdot, wdot, extra, s);
  HIP_CHECK(hipGetLastError());
  if (dF) HIP_CHECK(hipMemcpyAsync(dF, fdot, nd * N * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (dF_dev) HIP_CHECK(hipMemcpyAsync(dF_dev, fdot, nd * N * 3 * sizeof(double), hipMemcpyDeviceToDevice, s));
  std::vector<double> wat;
  if (dW) {
    wat.resize(nd * N * 9);
    HIP_CHECK(hipMemcpyAsync(wat.data(), wdot, nd * N * 9 * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  HIP_CHECK(hipStreamSynchronize(s));
  if (dW) frame_sums_of_rows(h, wat.data(), nd, dW);
}

}  // namespace

namespace ta {
namespace host {

int hessian_vectors_impl(ta_context *h, int32_t n_dir, int32_t first, const double *dR, const double *dh, double *dF,
                         double *dW, double *dF_dev) {
  if (!h || (!dF && !dF_dev) || n_dir < 0) return TA_ERR_INVALID;
  if (h->td) return fail(h, TA_ERR_UNSUPPORTED, td_inference_only("ta_hessian_vectors"));
  if (h->kind == TA_MODEL_EAM_FS) return fail(h, TA_ERR_INVALID, fs_inference_only("ta_hessian_vectors"));
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "no resident batch");
  const bool grap_model = h->kind == TA_MODEL_GRAP_MLP;
  const bool sf_model = h->kind == TA_MODEL_SF_MLP || grap_model;  // the descriptor + MLP models
  if (sf_model) {
    if (h->filtered) return fail(h, TA_ERR_UNSUPPORTED, filtered_refusal("ta_hessian_vectors"));
    if (grap_model && !ta::grap_hvp_supported(h->grap))
      return fail(h, TA_ERR_UNSUPPORTED, "ta_hessian_vectors: analytic second derivatives of GRAP models exist for the "
                                         "sf / morse / density / pexp filters, not for the filter network");
    for (const ChunkPlan &cp : h->chunks)
      for (int iz = 0; iz < cp.nz && !grap_model; ++iz)
        if (cp.ch.zeta_int[iz] <= 0)
          return fail(h, TA_ERR_UNSUPPORTED, "ta_hessian_vectors: integer zetas only");
  } else if (!h->eam || !ta::eam_hvp_supported(h->eam)) {
    return fail(h, TA_ERR_UNSUPPORTED, "ta_hessian_vectors: analytic second derivatives exist for the symmetry-function and GRAP "
                                       "models and for EAM / ADP models whose functions are of the Zjw04 family, networks or tabulated");
  }
  if (!dR && !dh && (first < 0 || (size_t)first + (size_t)n_dir > 3 * (size_t)h->db.n_atoms))
    return fail(h, TA_ERR_INVALID, "ta_hessian_vectors: without dR / dh the directions are unit displacements "
                                   "first .. first + n_dir - 1 of the 3 N");
  if ((size_t)n_dir > 65535) return fail(h, TA_ERR_INVALID, "ta_hessian_vectors: at most 65535 directions per call");
  return guarded(h, [&]() { (sf_model ? hvp_descriptor_models : hvp_eam)(h, n_dir, first, dR, dh, dF, dW, dF_dev); });
}

}  // namespace host
}  // namespace ta

extern "C" {

int ta_param_count(ta_handle h, int64_t *n_params) {
  if (!h || !n_params) return TA_ERR_INVALID;
  if (h->td) {  // H of every element, then U, then S
    *n_params = ta::td_param_count(h->td_nets, h->n_elements);
    return TA_OK;
  }
  if (h->eam) {  // the nn functions of an EAM / ADP model, slot after slot
    *n_params = ta::eam_param_count(h->eam);
    return TA_OK;
  }
  if (h->kind != TA_MODEL_SF_MLP && h->kind != TA_MODEL_GRAP_MLP)
    return fail(h, TA_ERR_INVALID, "the model has no MLP");
  *n_params = mlp_params(h);
  return TA_OK;
}

int ta_update_weights(ta_handle h, const double *weights, int64_t n_weights) {
  if (!h || !weights) return TA_ERR_INVALID;
  if (h->eam)
    return guarded(h, [&]() {
      HIP_CHECK(hipStreamSynchronize(h->stream));  // nothing may still read the old weights
      ta::eam_update_weights(h->eam, weights, n_weights);
    });
  if (!h->td && h->kind != TA_MODEL_SF_MLP && h->kind != TA_MODEL_GRAP_MLP)
    return fail(h, TA_ERR_INVALID, "the model has no MLP");
  return guarded(h, [&]() {
    // temperature-dependent: H, U, S of every element, in place (the device copy of the net descriptions, td_dev,
    // keeps its pointers)
    ta::MlpDev *nets = h->td ? h->td_nets : h->mlp;
    const int n_nets = h->td ? 3 * h->n_elements : h->n_elements;
    const int64_t want = h->td ? ta::td_param_count(h->td_nets, h->n_elements) : mlp_params(h);
    if (n_weights != want)
      throw std::invalid_argument("ta_update_weights: expected " + std::to_string(want) + " values");
    HIP_CHECK(hipStreamSynchronize(h->stream));  // nothing may still read the old weights
    const double *src = weights;
    for (int j = 0; j < n_nets; ++j) upload_net_weights(nets[j], src);
  });
}

int ta_energy_gradient(ta_handle h, const double *frame_coeff, double *grad, int64_t n_grad) {
  if (!h || !frame_coeff || !grad) return TA_ERR_INVALID;
  if (h->td)  // frame_coeff = dL/dF_f
    return ta_td_loss_gradient(h, frame_coeff, nullptr, nullptr, nullptr, nullptr, grad, n_grad, nullptr);
  if (h->kind == TA_MODEL_EAM_FS) return fail(h, TA_ERR_INVALID, fs_inference_only("ta_energy_gradient"));
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "no resident batch");
  if (h->eam)
    return guarded(h, [&]() {
      const int64_t total = ta::eam_param_count(h->eam);
      if (n_grad != total) throw std::invalid_argument(expected_room("ta_energy_gradient", total));
      if (total == 0) return;
      if (h->filtered) throw std::domain_error(filtered_refusal("ta_energy_gradient"));
      eam_exact_networks(h);
      // every function depends on the weights: the forward pass runs again (rho, F', moments)
      compute_impl(h, TA_WANT_ENERGY, false, nullptr);
      h->train_grad.ensure((size_t)total + 8);
      const double *coeff = upload_frame_coeff(h, &frame_coeff, 1);
      ta::eam_energy_gradient(h->eam, h->db, coeff, h->train_grad.ptr, h->stream);
      download_grad(h, grad, total);
    });
  if (h->kind != TA_MODEL_SF_MLP && h->kind != TA_MODEL_GRAP_MLP)
    return fail(h, TA_ERR_INVALID, "the model has no MLP");
  return guarded(h, [&]() {
    const int64_t total = mlp_params(h);
    if (n_grad != total) throw std::invalid_argument(expected_room("ta_energy_gradient", total));
    mark_grap_trained(h);
    // descriptors do not depend on the weights: computed once per resident batch
    if (!h->descriptors_valid) compute_impl(h, TA_WANT_ENERGY, false, nullptr);
    ensure_mlp_grad_buffers(h, false);
    const double *coeff = upload_frame_coeff(h, &frame_coeff, 1);
    size_t off = 0;
    for (int e = 0; e < h->n_elements; ++e) {
      const int n_el = h->db.elem_start[e + 1] - h->db.elem_start[e];
      ta::launch_mlp_grad(h->mlp[e], h->activation, h->sf.ndim, h->db.elem_atoms + h->db.elem_start[e], n_el,
                          h->db, coeff, h->train_scratch.ptr, h->train_partial.ptr, h->train_grad.ptr + off, h->stream);
      off += (size_t)ta::mlp_param_count(h->mlp[e]);
    }
    download_grad(h, grad, total);
  });
}

int ta_loss_gradient(ta_handle h, const double *frame_coeff, const double *dR, const double *dh, double *grad,
                     int64_t n_grad, double *dG_out) {
  if (!h || !grad) return TA_ERR_INVALID;
  if (h->td) {  // frame_coeff = dL/dF_f, the direction that of F
    if (!frame_coeff && !dR && !dh) return fail(h, TA_ERR_INVALID, "nothing to differentiate");
    return ta_td_loss_gradient(h, frame_coeff, nullptr, nullptr, dR, dh, grad, n_grad, dG_out);
  }
  if (h->kind == TA_MODEL_EAM_FS) return fail(h, TA_ERR_INVALID, fs_inference_only("ta_loss_gradient"));
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "no resident batch");
  if (!dR && !dh) {
    if (!frame_coeff) return fail(h, TA_ERR_INVALID, "nothing to differentiate");
    return ta_energy_gradient(h, frame_coeff, grad, n_grad);
  }
  if (h->eam) {
    // nn functions of an EAM / ADP model: one second-order pass per network, ta_eam.hip::eam_loss_gradient
    if (!ta::eam_loss_gradient_supported(h->eam))
      return fail(h, TA_ERR_UNSUPPORTED, "ta_loss_gradient: the analytic force / stress term covers EAM / ADP models "
                                         "whose analytic parts are of the Zjw04 family or tabulated");
    if (h->filtered) return fail(h, TA_ERR_UNSUPPORTED, filtered_refusal("ta_loss_gradient"));
    return guarded(h, [&]() {
      const int64_t total = ta::eam_param_count(h->eam);
      if (n_grad != total) throw std::invalid_argument(expected_room("ta_loss_gradient", total));
      if (dG_out) throw std::invalid_argument("ta_loss_gradient: dG_out is for the descriptor models");
      if (total == 0) return;
      eam_exact_networks(h);
      compute_impl(h, TA_WANT_ENERGY, false, nullptr);  // rho, F', per-pair columns with the current weights
      h->train_grad.ensure((size_t)total + 8);
      const Direction d = upload_direction(h, dR, dh, Absent::stays_null);
      const double *coeff = upload_frame_coeff(h, &frame_coeff, 1);
      ta::eam_loss_gradient(h->eam, h->db, coeff, d.dR, d.dh, h->train_grad.ptr, h->stream);
      download_grad(h, grad, total);
    });
  }
  if (h->kind != TA_MODEL_SF_MLP && h->kind != TA_MODEL_GRAP_MLP)
    return fail(h, TA_ERR_UNSUPPORTED, "ta_loss_gradient: the analytic force / stress term exists for the per-atom MLP models");
  if (h->filtered) return fail(h, TA_ERR_UNSUPPORTED, filtered_refusal("ta_loss_gradient"));
  return guarded(h, [&]() {
    const int64_t total = mlp_params(h);
    if (n_grad != total) throw std::invalid_argument(expected_room("ta_loss_gradient", total));
    mark_grap_trained(h);
    descriptor_tangent(h, dR, dh);
    ensure_mlp_grad_buffers(h, true);
    const double *coeff = upload_frame_coeff(h, &frame_coeff, 1);
    launch_mlp_grad2_all(h, h->tan_dG.ptr, coeff, nullptr);
    download_grad(h, grad, total, dG_out);
  });
}

int ta_td_loss_gradient(ta_handle h, const double *coeff_free_energy, const double *coeff_energy,
                        const double *coeff_eentropy, const double *dR, const double *dh, double *grad,
                        int64_t n_grad, double *dG_out) {
  if (!h || !grad) return TA_ERR_INVALID;
  if (!h->td) return fail(h, TA_ERR_INVALID, "ta_td_loss_gradient: not a temperature-dependent model");
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "no resident batch");
  const bool direction = dR || dh;
  if (direction && h->filtered) return fail(h, TA_ERR_UNSUPPORTED, filtered_refusal("ta_td_loss_gradient"));
  return guarded(h, [&]() {
    const int nel = h->n_elements;
    const int64_t total = ta::td_param_count(h->td_nets, nel);
    if (n_grad != total) throw std::invalid_argument(expected_room("ta_td_loss_gradient", total));
    if (dG_out && !direction) throw std::invalid_argument("ta_td_loss_gradient: dG_out needs a direction");
    mark_grap_trained(h);
    if (direction)
      descriptor_tangent(h, dR, dh);
    else if (!h->descriptors_valid)
      compute_impl(h, TA_WANT_ENERGY, false, nullptr);  // descriptors do not depend on the weights: once per batch
    size_t scratch = 0, partial = 0;
    ta::td_grad2_sizes(h->td_nets, nel, h->td_K, h->db.elem_start, &scratch, &partial);
    h->train_scratch.ensure(scratch + 8);
    h->train_partial.ensure(partial + 8);
    h->train_grad.ensure((size_t)total + 8);
    const double *host_coeff[3] = {coeff_energy, coeff_free_energy, coeff_eentropy};  // [a | b | g]
    const double *coeff = upload_frame_coeff(h, host_coeff, 3);
    ta::launch_td_grad2(h->td_dev, h->td_nets, nel, h->td_K, h->td_act, h->activation, h->td_sommerfeld ? 1 : 0,
                        h->sf.ndim, h->db, h->td_T.ptr, direction ? h->tan_dG.ptr : nullptr, coeff,
                        h->train_scratch.ptr, h->train_partial.ptr, h->train_grad.ptr, h->stream);
    download_grad(h, grad, total, dG_out);
  });
}

int ta_filter_param_count(ta_handle h, int64_t *n_params) {
  if (!h || !n_params) return TA_ERR_INVALID;
  *n_params = (h->kind == TA_MODEL_GRAP_MLP && h->grap) ? ta::grap_filter_param_count(h->grap) : 0;
  return TA_OK;
}

int ta_update_filter_weights(ta_handle h, const double *weights, int64_t n_weights) {
  if (!h || !weights) return TA_ERR_INVALID;
  if (h->kind != TA_MODEL_GRAP_MLP || !h->grap || !ta::grap_uses_filter_net(h->grap))
    return fail(h, TA_ERR_INVALID, "ta_update_filter_weights: the model has no filter network");
  return guarded(h, [&]() {
    HIP_CHECK(hipStreamSynchronize(h->stream));  // nothing may still read the old network
    // the descriptors, the filter values behind them and the pair Jacobian all belong to the old network
    h->descriptors_valid = false;
    h->jvp_valid = false;
    try {
      ta::grap_update_filter_weights(h->grap, weights, n_weights, h->stream);  // rebuilds the table when it is on
    } catch (...) {
      grap_filter_mode_changed(h);  // (a table that could not be rebuilt was dropped)
      throw;
    }
  });
}

int ta_set_filter_tables(ta_handle h, int on, int32_t n_knots) {
  if (!h) return TA_ERR_INVALID;
  if (n_knots != 0 && (n_knots < 5 || n_knots > (1 << 20) + 1))
    return fail(h, TA_ERR_INVALID, "ta_set_filter_tables: 5 .. 2^20 + 1 knots, or 0 for the default");
  if (h->kind != TA_MODEL_GRAP_MLP || !h->grap || !ta::grap_uses_filter_net(h->grap)) return TA_OK;
  // nothing changes (same knot count already in use, or a trained handle asked for tables): nothing is invalidated
  if (ta::grap_filter_table_target(h->grap, on != 0, n_knots) == ta::grap_filter_table_knots(h->grap)) return TA_OK;
  return guarded(h, [&]() {
    HIP_CHECK(hipStreamSynchronize(h->stream));
    try {
      ta::grap_set_filter_tables(h->grap, on != 0, n_knots, h->stream);
    } catch (...) {
      grap_filter_mode_changed(h);
      throw;
    }
    grap_filter_mode_changed(h);
  });
}

int ta_filter_table_knots(ta_handle h, int32_t *n_knots) {
  if (!h || !n_knots) return TA_ERR_INVALID;
  *n_knots = (h->kind == TA_MODEL_GRAP_MLP && h->grap) ? ta::grap_filter_table_knots(h->grap) : 0;
  return TA_OK;
}

int ta_grap_loss_gradient(ta_handle h, const double *frame_coeff, const double *dR, const double *dh, double *grad,
                          int64_t n_grad) {
  if (!h || !grad) return TA_ERR_INVALID;
  if (h->td)
    return fail(h, TA_ERR_UNSUPPORTED, "ta_grap_loss_gradient: the filter network of a temperature-dependent model "
                                       "is not trained");
  if (h->kind != TA_MODEL_GRAP_MLP || !h->grap)
    return fail(h, TA_ERR_UNSUPPORTED, "ta_grap_loss_gradient: not a GRAP model");
  {
    const std::string why = ta::grap_filter_train_refusal(h->grap);
    if (!why.empty()) return fail(h, TA_ERR_UNSUPPORTED, "ta_grap_loss_gradient: " + why);
  }
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "no resident batch");
  if (!frame_coeff && !dR && !dh) return fail(h, TA_ERR_INVALID, "nothing to differentiate");
  if (h->filtered) return fail(h, TA_ERR_UNSUPPORTED, filtered_refusal("ta_grap_loss_gradient"));
  return guarded(h, [&]() {
    const int64_t n_mlp = mlp_params(h), n_filter = ta::grap_filter_param_count(h->grap);
    if (n_grad != n_mlp + n_filter) throw std::invalid_argument(expected_room("ta_grap_loss_gradient", n_mlp + n_filter));
    mark_grap_trained(h);
    // descriptors, filter values (Hbuf) and dE/dG of the current weights and network
    compute_impl(h, TA_WANT_ENERGY, false, nullptr);
    hipStream_t s = h->stream;
    const size_t N = (size_t)h->db.n_atoms, P = (size_t)h->db.n_pairs;
    const int D = h->sf.ndim;
    ensure_tangents(h);
    // [pair vectors 4 P | kappa N D | the filter gradient's scratch]
    h->filt_scratch.ensure(4 * P + N * (size_t)D + ta::grap_filter_grad_doubles(h->grap, h->db) + 8);
    double *Dv = h->filt_scratch.ptr, *kappa = Dv + 4 * P, *fscratch = kappa + N * (size_t)D;
    ta::launch_pair_vec(h->db, Dv, s);
    if (dR || dh) {
      const Direction d = upload_direction(h, dR, dh, Absent::zeroed);
      ta::launch_pair_tangent(h->db, d.dR, d.dh, h->tan_dD.ptr, s);
      // G-dot in one launch, by dual arithmetic through the forward expression
      ta::launch_grap_filter_tangent(h->grap, h->db, h->sf.eps, Dv, h->tan_dD.ptr, h->tan_dG.ptr, s);
    } else {
      HIP_CHECK(hipMemsetAsync(h->tan_dD.ptr, 0, 4 * P * sizeof(double), s));
      HIP_CHECK(hipMemsetAsync(h->tan_dG.ptr, 0, N * (size_t)D * sizeof(double), s));
    }
    // MLP part and kappa = c w + H_mlp G-dot: one second-order pass per element
    ensure_mlp_grad_buffers(h, true);
    const double *coeff = upload_frame_coeff(h, &frame_coeff, 1);
    if (N) HIP_CHECK(hipMemsetAsync(kappa, 0, N * (size_t)D * sizeof(double), s));
    launch_mlp_grad2_all(h, h->tan_dG.ptr, coeff, kappa);
    download_grad(h, grad, n_mlp, nullptr, false);
    // filter part: per-pair adjoints (a, b), then the second-order sweep through the network (synchronises)
    ta::grap_filter_gradient(h->grap, h->db, h->sf.eps, Dv, h->tan_dD.ptr, kappa, fscratch, grad + n_mlp, s);
    HIP_CHECK(hipStreamSynchronize(s));
  });
}

int ta_constant_count(ta_handle h, int64_t *n_constants) {
  if (!h || !n_constants) return TA_ERR_INVALID;
  if (!h->eam) return fail(h, TA_ERR_INVALID, "the model has no empirical potential");
  *n_constants = ta::eam_constant_count(h->eam);
  return TA_OK;
}

int ta_get_constants(ta_handle h, double *constants, int64_t n_constants) {
  if (!h || !constants) return TA_ERR_INVALID;
  if (!h->eam) return fail(h, TA_ERR_INVALID, "the model has no empirical potential");
  if (n_constants != ta::eam_constant_count(h->eam)) return fail(h, TA_ERR_INVALID, "ta_get_constants: wrong length");
  ta::eam_get_constants(h->eam, constants);
  return TA_OK;
}

int ta_update_constants(ta_handle h, const double *constants, int64_t n_constants) {
  if (!h || !constants) return TA_ERR_INVALID;
  if (!h->eam) return fail(h, TA_ERR_INVALID, "the model has no empirical potential");
  return guarded(h, [&]() {
    HIP_CHECK(hipStreamSynchronize(h->stream));
    ta::eam_update_constants(h->eam, constants, n_constants);
  });
}

int ta_constant_gradient(ta_handle h, const double *frame_coeff, const double *dR, const double *dh, double *grad,
                         int64_t n_grad) {
  if (!h || !grad) return TA_ERR_INVALID;
  if (h->kind == TA_MODEL_EAM_FS) return fail(h, TA_ERR_INVALID, fs_inference_only("ta_constant_gradient"));
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "no resident batch");
  if (!h->eam) return fail(h, TA_ERR_INVALID, "the model has no empirical potential");
  if (!frame_coeff && !dR && !dh) return fail(h, TA_ERR_INVALID, "nothing to differentiate");
  if (h->filtered) return fail(h, TA_ERR_UNSUPPORTED, filtered_refusal("ta_constant_gradient"));
  return guarded(h, [&]() {
    const int64_t total = ta::eam_constant_count(h->eam);
    if (n_grad != total) throw std::invalid_argument(expected_room("ta_constant_gradient", total));
    // positions, cells and the list's cutoff test as the inference kernels see them; models with nn functions
    // beside the analytic ones: the networks evaluated exactly (per-pair columns, F'), as for their own gradient
    if (ta::eam_param_count(h->eam) > 0) eam_exact_networks(h);
    compute_impl(h, TA_WANT_ENERGY, false, nullptr);
    h->train_grad.ensure((size_t)total + 8);
    const double *coeff = upload_frame_coeff(h, &frame_coeff, 1);
    const Direction d = upload_direction(h, dR, dh, Absent::zero_beside);
    ta::eam_constant_gradient(h->eam, h->db, coeff, d.dR, d.dh, h->train_grad.ptr, h->stream);
    download_grad(h, grad, total);
  });
}

int ta_hessian_vectors(ta_handle h, int32_t n_dir, int32_t first, const double *dR, const double *dh, double *dF,
                       double *dW) {
  if (!h || !dF || n_dir < 0) return TA_ERR_INVALID;
  return hessian_vectors_impl(h, n_dir, first, dR, dh, dF, dW, nullptr);
}

int ta_set_nn_tables(ta_handle h, int on) {
  if (!h) return TA_ERR_INVALID;
  if (!h->eam) return TA_OK;
  return guarded(h, [&]() {
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (h->filtered && !on)
      throw std::domain_error("ta_set_nn_tables: a skin-filtered batch is resident; ta_set_frames again afterwards "
                              "(set the mode before ta_set_frames)");
    ta::eam_set_nn_tables(h->eam, on != 0);
    if (h->have_batch) ta::eam_ensure(h->eam, h->db);
  });
}

}  // extern "C"
