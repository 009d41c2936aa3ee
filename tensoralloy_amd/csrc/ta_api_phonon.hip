// C ABI of the harmonic-phonon path: the ta_phonon_* entry points (include/tensoralloy_amd.h). The launches are in
// ta_phonon.hip; the force constants come from the analytic Hessian-vector products (ta_api_train.hip:
// hessian_vectors_impl) and stay on the device.
//
// Work space, all in ta_context::phonon, sized for one chunk of q-points (Qc = q_chunk, a multiple of the DOS slab):
//   q [Qc][3] | D [Qc][n][n] complex | w [Qc][n] | V [Qc][n][n] complex (when asked for) | nu [Qc][n]
//   counts: [n_bins] total counts, then the two info words (unconverged matrices, modes outside the range)
//   dos_slab [slabs of the chunk][n_basis][n_bins], dos_part [n_basis][n_bins]
#include <algorithm>
#include <cmath>
#include <cstring>

#include "ta_context.h"
#include "ta_phonon.h"

using namespace ta::host;

namespace {

constexpr size_t kWorkBytes = 128u << 20;  // what a chunk's D and V may take
constexpr size_t kSlabBytes = 64u << 20;   // ... and the DOS slabs' partial rows

int64_t round_up_slab(int64_t q) { return (q + ta::kPhononDosSlab - 1) / ta::kPhononDosSlab * ta::kPhononDosSlab; }

int64_t default_chunk(int n) {
  const int64_t per_q = (int64_t)n * n * 32 + (int64_t)n * 16 + 24;
  int64_t q = (int64_t)kWorkBytes / per_q;
  q = std::min<int64_t>(std::max<int64_t>(q, ta::kPhononDosSlab), (int64_t)1 << 20);
  return q / ta::kPhononDosSlab * ta::kPhononDosSlab;
}

// the info words of this call, zeroed (and the bins in front of them)
unsigned long long *reset_counts(ta_context *h, int n_bins) {
  PhononState &ph = h->phonon;
  ph.counts.ensure((size_t)n_bins + 2);
  HIP_CHECK(hipMemsetAsync(ph.counts.ptr, 0, ((size_t)n_bins + 2) * sizeof(unsigned long long), h->stream));
  return ph.counts.ptr + n_bins;
}

// D and its eigensystem for the q-points [c0, c0 + qc) of the caller's list: ph.w, and ph.V when `vectors`
void solve_chunk(ta_context *h, const double *q_cart, int64_t c0, int64_t qc, bool vectors, unsigned long long *info) {
  PhononState &ph = h->phonon;
  const int n = 3 * ph.n_basis;
  hipStream_t s = h->stream;
  ph.q.ensure((size_t)qc * 3);
  ph.D.ensure((size_t)qc * n * n * 2);
  ph.w.ensure((size_t)qc * n);
  if (vectors) ph.V.ensure((size_t)qc * n * n * 2);
  HIP_CHECK(hipMemcpyAsync(ph.q.ptr, q_cart + 3 * c0, (size_t)qc * 3 * sizeof(double), hipMemcpyHostToDevice, s));
  ta::PhononDynmatLaunch d;
  d.phi = ph.phi.ptr, d.basis_of = ph.basis_of.ptr, d.mass = ph.mass.ptr, d.start = ph.start.ptr, d.vec = ph.vec.ptr;
  d.q = ph.q.ptr, d.D = ph.D.ptr, d.n_basis = ph.n_basis, d.N = ph.N, d.Q = qc;
  ta::launch_phonon_dynmat(d, s);
  ta::PhononEighLaunch e;
  e.A = ph.D.ptr, e.w = ph.w.ptr, e.V = vectors ? ph.V.ptr : nullptr, e.info = info, e.n = n, e.batch = qc;
  ta::launch_phonon_eigh(e, s);
  HIP_CHECK(hipGetLastError());
}

const char *need_phi(ta_context *h, const char *who, std::string &msg) {
  if (!h->have_batch || !h->phonon.valid) msg = std::string(who) + " called before ta_phonon_set_cell (ta_set_frames drops the phonon state)";
  else if (!h->phonon.have_phi) msg = std::string(who) + ": no force constants (ta_phonon_force_constants or ta_phonon_load_force_constants first)";
  else return nullptr;
  return msg.c_str();
}

}  // namespace

extern "C" {

int ta_phonon_eigh_group(int32_t n) {
  if (n < 1 || n > TA_PHONON_MAX_ORDER) return 0;
  return ta::phonon_eigh_matrices_per_block(n);
}

int ta_phonon_set_cell(ta_handle h, const ta_phonon_params *p, const int32_t *basis_of, const double *mass,
                       const int32_t *start, const double *vec) {
  if (!h) return TA_ERR_INVALID;
  if (!p || !basis_of || !mass || !start || !vec) return fail(h, TA_ERR_INVALID, "ta_phonon_set_cell: null argument");
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "ta_phonon_set_cell: no resident batch");
  if (h->db.n_frames != 1)
    return fail(h, TA_ERR_INVALID, "ta_phonon_set_cell: the resident batch must be ONE frame, the supercell (it has " +
                                       std::to_string(h->db.n_frames) + ")");
  const int64_t N = h->db.n_atoms;
  const int nb = p->n_basis;
  if (nb < 1 || nb > N || 3 * (int64_t)nb > TA_PHONON_MAX_ORDER)
    return fail(h, TA_ERR_INVALID, "ta_phonon_set_cell: n_basis must lie in 1 .. min(n_atoms, " +
                                       std::to_string(TA_PHONON_MAX_ORDER / 3) + "), the eigensolver's cap");
  if (p->q_chunk < 0) return fail(h, TA_ERR_INVALID, "ta_phonon_set_cell: q_chunk must be >= 0");
  for (int64_t s = 0; s < N; ++s)
    if (basis_of[s] < 0 || basis_of[s] >= nb || (s < nb && basis_of[s] != s))
      return fail(h, TA_ERR_INVALID, "ta_phonon_set_cell: basis_of[" + std::to_string(s) + "] is not a home-cell atom "
                                     "(the first n_basis atoms are the home cell, each its own image)");
  for (int b = 0; b < nb; ++b)
    if (!std::isfinite(mass[b]) || !(mass[b] > 0.0))
      return fail(h, TA_ERR_INVALID, "ta_phonon_set_cell: masses must be finite and > 0");
  const size_t pairs = (size_t)nb * (size_t)N;
  if (start[0] != 0) return fail(h, TA_ERR_INVALID, "ta_phonon_set_cell: start[0] must be 0");
  for (size_t i = 0; i < pairs; ++i)
    if (start[i + 1] < start[i])
      return fail(h, TA_ERR_INVALID, "ta_phonon_set_cell: start is not monotone at pair " + std::to_string(i));
  const size_t n_vec = (size_t)start[pairs];
  for (size_t i = 0; i < 3 * n_vec; ++i)
    if (!std::isfinite(vec[i])) return fail(h, TA_ERR_INVALID, "ta_phonon_set_cell: a vector is not finite");
  return guarded(h, [&]() {
    PhononState &ph = h->phonon;
    ph.valid = ph.have_phi = false;
    HIP_CHECK(hipStreamSynchronize(h->stream));
    ph.basis_of.ensure((size_t)N);
    ph.mass.ensure((size_t)nb);
    ph.start.ensure(pairs + 1);
    ph.vec.ensure(3 * n_vec + 3);
    ph.phi.ensure(pairs * 9);
    HIP_CHECK(hipMemcpy(ph.basis_of.ptr, basis_of, (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(ph.mass.ptr, mass, (size_t)nb * sizeof(double), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(ph.start.ptr, start, (pairs + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
    if (n_vec) HIP_CHECK(hipMemcpy(ph.vec.ptr, vec, 3 * n_vec * sizeof(double), hipMemcpyHostToDevice));
    ph.n_basis = nb;
    ph.N = (int)N;
    ph.q_chunk = p->q_chunk > 0 ? round_up_slab(p->q_chunk) : default_chunk(3 * nb);
    ph.valid = true;
  });
}

int ta_phonon_force_constants(ta_handle h, double *phi) {
  if (!h) return TA_ERR_INVALID;
  if (!h->have_batch || !h->phonon.valid)
    return fail(h, TA_ERR_INVALID, "ta_phonon_force_constants called before ta_phonon_set_cell (ta_set_frames drops the phonon state)");
  PhononState &ph = h->phonon;
  const int n = 3 * ph.n_basis;
  const size_t count = (size_t)ph.n_basis * ph.N * 9;
  ph.have_phi = false;
  int rc = guarded(h, [&]() { ph.D.ensure(count); });  // (the tangents [n][N][3] rest in the chunk's D until transposed)
  if (rc != TA_OK) return rc;
  rc = hessian_vectors_impl(h, n, 0, nullptr, nullptr, nullptr, nullptr, ph.D.ptr);
  if (rc != TA_OK) return rc;
  return guarded(h, [&]() {
    ta::launch_phonon_phi_from_tangents(ph.D.ptr, ph.phi.ptr, ph.n_basis, ph.N, h->stream);
    HIP_CHECK(hipGetLastError());
    if (phi) HIP_CHECK(hipMemcpyAsync(phi, ph.phi.ptr, count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
    ph.have_phi = true;
  });
}

int ta_phonon_load_force_constants(ta_handle h, const double *phi) {
  if (!h) return TA_ERR_INVALID;
  if (!phi) return fail(h, TA_ERR_INVALID, "ta_phonon_load_force_constants: null argument");
  if (!h->have_batch || !h->phonon.valid)
    return fail(h, TA_ERR_INVALID, "ta_phonon_load_force_constants called before ta_phonon_set_cell (ta_set_frames drops the phonon state)");
  PhononState &ph = h->phonon;
  const size_t count = (size_t)ph.n_basis * ph.N * 9;
  for (size_t i = 0; i < count; ++i)
    if (!std::isfinite(phi[i])) return fail(h, TA_ERR_INVALID, "ta_phonon_load_force_constants: a force constant is not finite");
  ph.have_phi = false;
  return guarded(h, [&]() {
    HIP_CHECK(hipStreamSynchronize(h->stream));
    HIP_CHECK(hipMemcpy(ph.phi.ptr, phi, count * sizeof(double), hipMemcpyHostToDevice));
    ph.have_phi = true;
  });
}

int ta_phonon_frequencies(ta_handle h, int64_t Q, const double *q_cart, double *freq_THz, double *eigvec, int64_t *info) {
  if (!h) return TA_ERR_INVALID;
  std::string msg;
  if (need_phi(h, "ta_phonon_frequencies", msg)) return fail(h, TA_ERR_INVALID, msg);
  if (Q < 0 || (Q > 0 && (!q_cart || !freq_THz)) || !info) return fail(h, TA_ERR_INVALID, "ta_phonon_frequencies: bad argument");
  for (int64_t i = 0; i < 3 * Q; ++i)
    if (!std::isfinite(q_cart[i])) return fail(h, TA_ERR_INVALID, "ta_phonon_frequencies: a wave vector is not finite");
  return guarded(h, [&]() {
    PhononState &ph = h->phonon;
    const int n = 3 * ph.n_basis;
    hipStream_t s = h->stream;
    unsigned long long *d_info = reset_counts(h, 0);
    for (int64_t c0 = 0; c0 < Q; c0 += ph.q_chunk) {
      const int64_t qc = std::min(ph.q_chunk, Q - c0);
      solve_chunk(h, q_cart, c0, qc, eigvec != nullptr, d_info);
      ph.nu.ensure((size_t)qc * n);
      ta::launch_phonon_frequencies(ph.w.ptr, ph.nu.ptr, qc * n, TA_PHONON_THZ, s);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipMemcpyAsync(freq_THz + c0 * n, ph.nu.ptr, (size_t)qc * n * sizeof(double), hipMemcpyDeviceToHost, s));
      if (eigvec)
        HIP_CHECK(hipMemcpyAsync(eigvec + c0 * n * n * 2, ph.V.ptr, (size_t)qc * n * n * 2 * sizeof(double),
                                 hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));  // (the chunk's buffers are reused)
    }
    unsigned long long words[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(words, d_info, sizeof(words), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    info[0] = (int64_t)words[0];
  });
}

int ta_phonon_dos(ta_handle h, int64_t Q, const double *q_cart, int32_t n_bins, double nu_min, double nu_max,
                  uint64_t *total, double *partial, int64_t *info) {
  if (!h) return TA_ERR_INVALID;
  std::string msg;
  if (need_phi(h, "ta_phonon_dos", msg)) return fail(h, TA_ERR_INVALID, msg);
  if (Q < 0 || (Q > 0 && !q_cart) || !total || !info) return fail(h, TA_ERR_INVALID, "ta_phonon_dos: bad argument");
  if (n_bins < 1 || n_bins > TA_MD_MAX_BINS)
    return fail(h, TA_ERR_INVALID, "ta_phonon_dos: n_bins must lie in 1 .. " + std::to_string(TA_MD_MAX_BINS));
  if (!std::isfinite(nu_min) || !std::isfinite(nu_max) || !(nu_max > nu_min))
    return fail(h, TA_ERR_INVALID, "ta_phonon_dos: nu_min and nu_max must be finite, nu_max > nu_min");
  for (int64_t i = 0; i < 3 * Q; ++i)
    if (!std::isfinite(q_cart[i])) return fail(h, TA_ERR_INVALID, "ta_phonon_dos: a wave vector is not finite");
  return guarded(h, [&]() {
    PhononState &ph = h->phonon;
    const int n = 3 * ph.n_basis;
    hipStream_t s = h->stream;
    const size_t cells = (size_t)ph.n_basis * n_bins;
    unsigned long long *d_info = reset_counts(h, n_bins);
    int64_t chunk = ph.q_chunk;
    if (partial) {  // the slabs' rows bound the chunk too; still whole slabs, so the sums keep their order
      const int64_t slabs = std::max<int64_t>(1, (int64_t)(kSlabBytes / (cells * sizeof(double))));
      chunk = std::min(chunk, slabs * ta::kPhononDosSlab);
      ph.dos_part.ensure(cells);
      ph.dos_slab.ensure((size_t)(chunk / ta::kPhononDosSlab) * cells);
      HIP_CHECK(hipMemsetAsync(ph.dos_part.ptr, 0, cells * sizeof(double), s));
    }
    for (int64_t c0 = 0; c0 < Q; c0 += chunk) {
      const int64_t qc = std::min(chunk, Q - c0);
      solve_chunk(h, q_cart, c0, qc, partial != nullptr, d_info);
      ta::PhononDosLaunch a;
      a.w = ph.w.ptr, a.V = partial ? ph.V.ptr : nullptr, a.total = ph.counts.ptr, a.info = d_info + 1;
      a.slab_part = partial ? ph.dos_slab.ptr : nullptr, a.partial = partial ? ph.dos_part.ptr : nullptr;
      a.nu_min = nu_min, a.inv_dnu = (double)n_bins / (nu_max - nu_min), a.factor = TA_PHONON_THZ;
      a.n = n, a.n_bins = n_bins, a.Q = qc;
      ta::launch_phonon_dos(a, s);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipStreamSynchronize(s));  // (the chunk's buffers are reused; q_cart's next rows go up)
    }
    std::vector<unsigned long long> host((size_t)n_bins + 2);
    HIP_CHECK(hipMemcpyAsync(host.data(), ph.counts.ptr, host.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    if (partial) HIP_CHECK(hipMemcpyAsync(partial, ph.dos_part.ptr, cells * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    for (int k = 0; k < n_bins; ++k) total[k] = host[k];
    info[0] = (int64_t)host[n_bins];
    info[1] = (int64_t)host[(size_t)n_bins + 1];
  });
}

int ta_phonon_eigh(ta_handle h, int32_t n, int64_t batch, const double *A, double *w, double *V, int64_t *info) {
  if (!h) return TA_ERR_INVALID;
  if (n < 1 || batch < 0 || (batch > 0 && (!A || !w)) || !info) return fail(h, TA_ERR_INVALID, "ta_phonon_eigh: bad argument");
  if (n > TA_PHONON_MAX_ORDER)
    return fail(h, TA_ERR_UNSUPPORTED, "ta_phonon_eigh: order " + std::to_string(n) + " is above the solver's cap, " +
                                           std::to_string(TA_PHONON_MAX_ORDER));
  return guarded(h, [&]() {
    PhononState &ph = h->phonon;
    hipStream_t s = h->stream;
    const size_t nn2 = (size_t)n * n * 2;
    unsigned long long *d_info = reset_counts(h, 0);
    const int64_t chunk = default_chunk(n);
    for (int64_t c0 = 0; c0 < batch; c0 += chunk) {
      const int64_t bc = std::min(chunk, batch - c0);
      ph.D.ensure((size_t)bc * nn2);
      ph.w.ensure((size_t)bc * n);
      if (V) ph.V.ensure((size_t)bc * nn2);
      HIP_CHECK(hipMemcpyAsync(ph.D.ptr, A + c0 * nn2, (size_t)bc * nn2 * sizeof(double), hipMemcpyHostToDevice, s));
      ta::PhononEighLaunch e;
      e.A = ph.D.ptr, e.w = ph.w.ptr, e.V = V ? ph.V.ptr : nullptr, e.info = d_info, e.n = n, e.batch = bc;
      ta::launch_phonon_eigh(e, s);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipMemcpyAsync(w + c0 * n, ph.w.ptr, (size_t)bc * n * sizeof(double), hipMemcpyDeviceToHost, s));
      if (V) HIP_CHECK(hipMemcpyAsync(V + c0 * nn2, ph.V.ptr, (size_t)bc * nn2 * sizeof(double), hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
    }
    unsigned long long word = 0;
    HIP_CHECK(hipMemcpyAsync(&word, d_info, sizeof(word), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    info[0] = (int64_t)word;
  });
}

}  // extern "C"
