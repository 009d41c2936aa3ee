// C ABI of the device-resident relaxation: the ta_relax_* entry points (include/tensoralloy_amd.h), cell and band
// mode included. The loop itself is in ta_resident.hip; the FIRE launches are in ta_relax.hip, the band launches in
// ta_neb.hip.
#include <cmath>
#include <cstring>

#include "ta_context.h"
#include "ta_md.h"
#include "ta_neb.h"
#include "ta_relax.h"

using namespace ta::host;

namespace {

// the optimiser at its start: dt, a = astart, npos = 0, no step taken
ta::RelaxFrameState fire_start(const ta_fire_params &p) {
  ta::RelaxFrameState st;
  st.dt = p.dt;
  st.a = p.astart;
  st.fmax2 = 0.0;
  st.npos = 0;
  st.first = 1;
  st.converged = 0;
  st.steps = 0;
  return st;
}

}  // namespace

extern "C" {

int ta_relax_init(ta_handle h, const ta_fire_params *p, const uint8_t *fixed) {
  if (!h) return TA_ERR_INVALID;
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "ta_relax_init: no resident batch");
  ta_fire_params q = {0.1, 1.0, 0.2, 1.1, 0.5, 0.1, 0.99, 5};  // ASE's defaults
  if (p) q = *p;
  auto positive = [](double v) { return std::isfinite(v) && v > 0.0; };
  if (!positive(q.dt)) return fail(h, TA_ERR_INVALID, "ta_relax_init: dt must be finite and > 0");
  if (!positive(q.dtmax)) return fail(h, TA_ERR_INVALID, "ta_relax_init: dtmax must be finite and > 0");
  if (!positive(q.maxstep)) return fail(h, TA_ERR_INVALID, "ta_relax_init: maxstep must be finite and > 0");
  if (!std::isfinite(q.finc) || q.finc < 1.0) return fail(h, TA_ERR_INVALID, "ta_relax_init: finc must be finite and >= 1");
  if (!(q.fdec > 0.0 && q.fdec < 1.0)) return fail(h, TA_ERR_INVALID, "ta_relax_init: fdec must lie in (0, 1)");
  if (!(q.fa > 0.0 && q.fa < 1.0)) return fail(h, TA_ERR_INVALID, "ta_relax_init: fa must lie in (0, 1)");
  if (!(q.astart > 0.0 && q.astart <= 1.0)) return fail(h, TA_ERR_INVALID, "ta_relax_init: astart must lie in (0, 1]");
  if (q.nmin < 0) return fail(h, TA_ERR_INVALID, "ta_relax_init: nmin must be >= 0");
  return guarded(h, [&]() {
    RelaxState &rx = h->relax;
    const size_t N = h->keep_species.size(), F = h->keep_natoms.size();
    rx.valid = false;
    HIP_CHECK(hipStreamSynchronize(h->stream));
    h->upload_pending = false;
    rx.vel.ensure(3 * N + 1);
    rx.fixed.ensure(N + 1);
    rx.state.ensure(2 * F + 1);
    rx.count.ensure(1);
    h->res.ref.ensure(3 * N + 1);
    h->res.ref_builds = -1;  // ta_relax_run uploads ref_pos
    h->res.status.ensure(2);
    h->res.status_host.ensure(64);
    if (N) {
      HIP_CHECK(hipMemset(rx.vel.ptr, 0, 3 * N * sizeof(double)));
      if (fixed) {
        std::vector<uint8_t> mask(N);
        for (size_t i = 0; i < N; ++i) mask[i] = fixed[i] ? 1 : 0;
        HIP_CHECK(hipMemcpy(rx.fixed.ptr, mask.data(), N, hipMemcpyHostToDevice));
        rx.fixed_host = mask;
      } else {
        HIP_CHECK(hipMemset(rx.fixed.ptr, 0, N));
        rx.fixed_host.assign(N, 0);
      }
    } else {
      rx.fixed_host.clear();
    }
    rx.state_host.assign(F, fire_start(q));
    rx.cell.on = false;
    rx.band.on = rx.band.ran = false;
    rx.cell.reset_deformation(F);
    rx.p = q;
    h->res.chunk = 0;  // (the workgroup layout is planned for this batch by the next run)
    h->res.blk_start_host.clear();
    rx.valid = true;
  });
}

int ta_relax_run(ta_handle h, int32_t max_steps, double fmax, uint32_t want, int32_t *steps, int32_t *converged,
                 double *fmax_out, int32_t *n_rebuilds) {
  if (!h) return TA_ERR_INVALID;
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "ta_relax_run: no resident batch");
  if (!h->relax.valid)
    return fail(h, TA_ERR_INVALID, "ta_relax_run called before ta_relax_init (ta_set_frames drops the relaxation state)");
  if (max_steps < 0) return fail(h, TA_ERR_INVALID, "ta_relax_run: max_steps must be >= 0");
  if (!std::isfinite(fmax) || !(fmax > 0.0)) return fail(h, TA_ERR_INVALID, "ta_relax_run: fmax must be finite and > 0");
  if (n_rebuilds) *n_rebuilds = 0;
  want |= TA_WANT_ENERGY | TA_WANT_FORCES;
  want &= ~(uint32_t)TA_WANT_REUSE_DESCRIPTORS;
  RelaxState &rx = h->relax;
  ResidentLoop &res = h->res;
  const bool cell = rx.cell.on;
  const bool band = rx.band.on;  // (never with `cell`)
  if (cell) want |= TA_WANT_VIRIAL;  // the force on the cell rows
  // a run that fails leaves positions and velocities somewhere on its way and the host's image of the
  // per-frame records behind them: the state is dropped, and only ta_relax_init makes a new one
  rx.valid = false;
  rx.band.ran = false;
  res.cell_running = cell;
  const int rc = guarded(h, [&]() {
    const size_t N = h->keep_species.size(), F = h->keep_natoms.size();
    hipStream_t s = h->stream;
    md_plan_blocks(h, ta::kMdChunk);
    // band mode: the FIRE launches see the whole band as one pseudo-frame of N atoms; the band launches cut
    // every interior image into its own workgroups
    const int band_n = band ? h->keep_natoms[0] : 0;
    const int band_blk_per_image = std::max(1, (band_n + ta::kMdChunk - 1) / ta::kMdChunk);
    const size_t n_blk = band ? std::max<size_t>(1, (N + ta::kMdChunk - 1) / ta::kMdChunk) : (size_t)res.n_blk;
    rx.part.ensure(4 * n_blk + 1);
    if (band) rx.band.part.ensure(4 * (F - 2) * (size_t)band_blk_per_image + 1);
    HIP_CHECK(hipStreamSynchronize(s));
    // every frame is tested against this run's fmax: a frame frozen by an earlier run may wake
    std::vector<ta::RelaxFrameState> &st = rx.state_host;
    for (auto &r : st) r.converged = 0, r.steps = 0;
    if (F) HIP_CHECK(hipMemcpy(rx.state.ptr, st.data(), F * sizeof(ta::RelaxFrameState), hipMemcpyHostToDevice));
    if (band) {  // the band's one record into copy 0, the pseudo-frame's layout next to the climbing word
      rx.band.state_host.converged = 0, rx.band.state_host.steps = 0;
      HIP_CHECK(hipMemcpy(rx.band.state.ptr, &rx.band.state_host, sizeof(ta::RelaxFrameState), hipMemcpyHostToDevice));
      const int32_t layout[5] = {0, (int32_t)N, 0, (int32_t)n_blk, -1};
      HIP_CHECK(hipMemcpy(rx.band.layout.ptr, layout, sizeof(layout), hipMemcpyHostToDevice));
    }
    HIP_CHECK(hipMemset(rx.count.ptr, 0, sizeof(int)));
    if (cell && F) {  // the current G and cell velocity into copy 0, the cells of the resident list next to res.ref
      HIP_CHECK(hipMemcpy(rx.cell.G.ptr, rx.cell.G_host.data(), 9 * F * sizeof(double), hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(rx.cell.vel.ptr, rx.cell.vel_host.data(), 9 * F * sizeof(double), hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(res.ref_cells.ptr, h->ref_cells.data(), 9 * F * sizeof(double), hipMemcpyHostToDevice));
    }
    resident_begin(h);
    volatile unsigned *status_host = res.host_words();

    const ta_fire_params &p = rx.p;
    ta::RelaxLaunch a;
    a.vel = rx.vel.ptr;
    a.fixed = rx.fixed.ptr;
    a.ref = res.ref.ptr;
    a.blk_start = res.blk_start.ptr;
    a.part = rx.part.ptr;
    a.state = rx.state.ptr;
    a.n_converged = rx.count.ptr;
    a.status = res.status.ptr;
    a.status_host = const_cast<unsigned *>(status_host);
    a.dtmax = p.dtmax, a.maxstep = p.maxstep, a.finc = p.finc, a.fdec = p.fdec, a.astart = p.astart, a.fa = p.fa;
    a.nmin = p.nmin;
    a.fmax2 = fmax * fmax;
    a.lim2 = h->skin > 0.0 ? 0.25 * h->skin * h->skin : -1.0;  // skin = 0: every step rebuilds
    a.n_frames = (int)F;
    a.n_blk = (int)n_blk;
    a.chunk = ta::kMdChunk;
    a.cell = cell ? 1 : 0;
    a.virial = nullptr, a.cells = nullptr;
    a.ref_cells = res.ref_cells.ptr, a.cell_h0 = rx.cell.h0.ptr, a.cell_cf = rx.cell.cf.ptr;
    a.cell_G = rx.cell.G.ptr, a.cell_vel = rx.cell.vel.ptr, a.cell_fmax2 = rx.cell.fmax2.ptr;
    {
      const int32_t *m = rx.cell.p.mask;  // Voigt xx yy zz yz xz xy
      const int32_t full[9] = {m[0], m[5], m[4], m[5], m[1], m[3], m[4], m[3], m[2]};
      for (int c = 0; c < 9; ++c) a.cell_mask[c] = full[c] ? 1.0 : 0.0;
    }
    a.pressure = rx.cell.p.pressure;
    a.skin = h->skin;
    a.r_list = h->rmax + h->skin;
    a.hydrostatic = rx.cell.p.hydrostatic ? 1 : 0;
    ta::NebLaunch nb = {};
    if (band) {
      a.fixed = rx.band.fixed.ptr;
      a.blk_start = rx.band.layout.ptr + 2;
      a.state = rx.band.state.ptr;
      a.n_frames = 1;
      nb.fixed = rx.band.fixed.ptr;
      nb.part = rx.band.part.ptr;
      nb.band = rx.band.force.ptr;
      nb.climbing = rx.band.layout.ptr + 4;
      nb.status = res.status.ptr;
      nb.k = rx.band.p.k;
      nb.n_images = (int)F, nb.n = band_n, nb.chunk = ta::kMdChunk, nb.blk_per_image = band_blk_per_image;
      nb.climb = rx.band.p.climb ? 1 : 0;
    }
    // B (and, with `tangents`, tau) of the resident evaluation
    auto band_force = [&](int k, bool tangents) {
      nb.pos = h->db.pos;
      nb.forces = h->db.forces;
      nb.energy = h->db.energy;
      nb.tau = tangents ? rx.band.tau.ptr : nullptr;
      nb.seq = (unsigned)k;
      ta::launch_neb_force(nb, s);
      HIP_CHECK(hipGetLastError());
    };
    int launched = 0;  // launches that ran: the current copy of the state is launched & 1
    auto step = [&](int k, bool drift) {
      // (a rebuild may have moved the batch's arrays: the pointers are taken at every launch)
      a.pos = h->db.pos;
      a.forces = h->db.forces;
      a.atom_start = h->db.atom_start;
      a.virial = h->db.virial;
      a.cells = h->db.cells;
      a.seq = (unsigned)k;
      a.drift = drift ? 1 : 0;
      if (band) {  // FIRE runs on the band forces of the pseudo-frame; the last launch of a run leaves tau too
        band_force(k, !drift);
        a.forces = rx.band.force.ptr;
        a.atom_start = rx.band.layout.ptr;
      }
      ta::launch_relax_step(a, s);
      HIP_CHECK(hipGetLastError());
      launched = k + 1;
    };

    h->jvp_valid = false;
    compute_impl(h, want, false, nullptr);  // F of the state at entry
    int rebuilds = 0;
    bool all_converged = false;
    // the launch at which the last frame converged, and every launch behind it, moved nothing
    auto finished = [&](int k, int k_end) {
      const unsigned done = status_host[1];
      if (done == 0u) return -1;
      if ((int)done - 1 < k || (int)done - 1 >= k_end) throw std::runtime_error("ta_relax_run: inconsistent done word");
      all_converged = true;
      return (int)done - 1;
    };
    const int done_steps = resident_steps(h, "ta_relax_run", max_steps, want, [&](int q) { step(q, true); }, finished,
                                          &rebuilds, n_rebuilds);
    if (!all_converged) step(done_steps, false);  // the test of the last evaluation
    else if (band) band_force(done_steps, true);  // (the converged state's B again, with tau)
    HIP_CHECK(hipStreamSynchronize(s));
    h->upload_pending = false;
    if (n_rebuilds) *n_rebuilds = rebuilds;
    if (band) {
      ta::RelaxFrameState &b = rx.band.state_host;
      HIP_CHECK(hipMemcpy(&b, rx.band.state.ptr + (size_t)(launched & 1), sizeof(ta::RelaxFrameState), hipMemcpyDeviceToHost));
      for (size_t f = 0; f < F; ++f) {
        if (steps) steps[f] = b.steps;
        if (converged) converged[f] = b.converged;
        if (fmax_out) fmax_out[f] = std::sqrt(b.fmax2);
      }
      rx.band.energy_host.resize(F);  // what ta_relax_get_band hands out next to B and tau of this state
      HIP_CHECK(hipMemcpy(rx.band.energy_host.data(), h->db.energy, F * sizeof(double), hipMemcpyDeviceToHost));
      return;
    }
    if (F)
      HIP_CHECK(hipMemcpy(st.data(), rx.state.ptr + (size_t)(launched & 1) * F, F * sizeof(ta::RelaxFrameState),
                          hipMemcpyDeviceToHost));
    for (size_t f = 0; f < F; ++f) {
      if (steps) steps[f] = st[f].steps;
      if (converged) converged[f] = st[f].converged;
      if (fmax_out) fmax_out[f] = std::sqrt(st[f].fmax2);
    }
    if (cell && F) {
      HIP_CHECK(hipMemcpy(rx.cell.G_host.data(), rx.cell.G.ptr + 9 * (size_t)(launched & 1) * F,
                          9 * F * sizeof(double), hipMemcpyDeviceToHost));
      HIP_CHECK(hipMemcpy(rx.cell.vel_host.data(), rx.cell.vel.ptr + 9 * (size_t)(launched & 1) * F,
                          9 * F * sizeof(double), hipMemcpyDeviceToHost));
      resident_final_cells(h, "ta_relax_run", want, &rebuilds, n_rebuilds);
    }
  });
  res.cell_running = false;
  if (rc == TA_OK) rx.valid = true, rx.band.ran = band;
  else rx.cell.on = rx.band.on = false;
  return rc;
}

int ta_relax_get_state(ta_handle h, double *positions, double *velocities, double *dt, double *a, int32_t *npos) {
  if (!h) return TA_ERR_INVALID;
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "ta_relax_get_state: no resident batch");
  if (!h->relax.valid) return fail(h, TA_ERR_INVALID, "ta_relax_get_state called before ta_relax_init");
  return guarded(h, [&]() {
    const RelaxState &rx = h->relax;
    const size_t N = h->keep_species.size(), F = h->keep_natoms.size();
    HIP_CHECK(hipStreamSynchronize(h->stream));
    h->upload_pending = false;
    if (positions && N) HIP_CHECK(hipMemcpy(positions, h->db.pos, 3 * N * sizeof(double), hipMemcpyDeviceToHost));
    if (velocities && N)
      HIP_CHECK(hipMemcpy(velocities, rx.vel.ptr, 3 * N * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t f = 0; f < F; ++f) {  // (band mode: the band's one record for every frame)
      const ta::RelaxFrameState &r = rx.band.on ? rx.band.state_host : rx.state_host[f];
      if (dt) dt[f] = r.dt;
      if (a) a[f] = r.a;
      if (npos) npos[f] = r.npos;
    }
  });
}

int ta_relax_set_cell(ta_handle h, int on, const ta_relax_cell_params *p) {
  if (!h) return TA_ERR_INVALID;
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "ta_relax_set_cell: no resident batch");
  if (!h->relax.valid) return fail(h, TA_ERR_INVALID, "ta_relax_set_cell called before ta_relax_init");
  auto &cell = h->relax.cell;
  if (!on) {
    cell.on = false;  // (the cells stay as they are)
    return TA_OK;
  }
  if (h->relax.band.on)
    return fail(h, TA_ERR_INVALID, "ta_relax_set_cell: the band option is on (ta_relax_set_band); cells along a band stay fixed");
  ta_relax_cell_params q = {0.0, 0.0, {1, 1, 1, 1, 1, 1}, 0, 0};
  if (p) q = *p;
  if (!std::isfinite(q.cell_factor) || q.cell_factor < 0.0)
    return fail(h, TA_ERR_INVALID, "ta_relax_set_cell: cell_factor must be finite and >= 0");
  if (!std::isfinite(q.pressure)) return fail(h, TA_ERR_INVALID, "ta_relax_set_cell: pressure must be finite");
  bool any = false;
  for (int c = 0; c < 6; ++c) any = any || q.mask[c] != 0;
  if (!any) return fail(h, TA_ERR_INVALID, "ta_relax_set_cell: mask leaves no component of the cell free");
  const size_t F = h->keep_natoms.size();
  std::vector<double> cf(F);
  for (size_t f = 0; f < F; ++f) {
    for (int k = 0; k < 3; ++k)
      if (!h->keep_pbc[3 * f + k])
        return fail(h, TA_ERR_INVALID, "ta_relax_set_cell: frame " + std::to_string(f) + " is not periodic along all three axes");
    const double *c = h->ref_cells.data() + 9 * f;
    const double det = c[0] * (c[4] * c[8] - c[5] * c[7]) - c[1] * (c[3] * c[8] - c[5] * c[6]) + c[2] * (c[3] * c[7] - c[4] * c[6]);
    if (!std::isfinite(det) || !(std::fabs(det) > 0.0))
      return fail(h, TA_ERR_INVALID, "ta_relax_set_cell: the cell of frame " + std::to_string(f) + " is singular");
    cf[f] = q.cell_factor > 0.0 ? q.cell_factor : (double)std::max(1, h->keep_natoms[f]);
  }
  return guarded(h, [&]() {
    HIP_CHECK(hipStreamSynchronize(h->stream));
    h->upload_pending = false;
    cell.h0.ensure(9 * F + 1);
    cell.cf.ensure(F + 1);
    cell.G.ensure(2 * 9 * F + 1);
    cell.vel.ensure(2 * 9 * F + 1);
    cell.fmax2.ensure(F + 1);
    h->res.ref_cells.ensure(9 * F + 1);
    if (F) {
      HIP_CHECK(hipMemcpy(cell.h0.ptr, h->ref_cells.data(), 9 * F * sizeof(double), hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(cell.cf.ptr, cf.data(), F * sizeof(double), hipMemcpyHostToDevice));
      HIP_CHECK(hipMemset(cell.fmax2.ptr, 0, F * sizeof(double)));
    }
    cell.reset_deformation(F);
    cell.p = q;
    cell.on = true;
  });
}

int ta_relax_get_cell(ta_handle h, double *cells, double *deform, double *cell_velocities, double *cell_fmax) {
  if (!h) return TA_ERR_INVALID;
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "ta_relax_get_cell: no resident batch");
  if (!h->relax.valid) return fail(h, TA_ERR_INVALID, "ta_relax_get_cell called before ta_relax_init");
  return guarded(h, [&]() {
    const auto &cell = h->relax.cell;
    const size_t F = h->keep_natoms.size();
    HIP_CHECK(hipStreamSynchronize(h->stream));
    h->upload_pending = false;
    if (!F) return;
    // (between runs ref_cells is the image of the device's cells)
    if (cells) std::memcpy(cells, h->ref_cells.data(), 9 * F * sizeof(double));
    if (deform) std::memcpy(deform, cell.G_host.data(), 9 * F * sizeof(double));
    if (cell_velocities) std::memcpy(cell_velocities, cell.vel_host.data(), 9 * F * sizeof(double));
    if (cell_fmax) {
      if (cell.fmax2.ptr) {
        HIP_CHECK(hipMemcpy(cell_fmax, cell.fmax2.ptr, F * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t f = 0; f < F; ++f) cell_fmax[f] = std::sqrt(cell_fmax[f]);
      } else {
        for (size_t f = 0; f < F; ++f) cell_fmax[f] = 0.0;
      }
    }
  });
}

int ta_relax_set_band(ta_handle h, int on, const ta_band_params *p) {
  if (!h) return TA_ERR_INVALID;
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "ta_relax_set_band: no resident batch");
  if (!h->relax.valid) return fail(h, TA_ERR_INVALID, "ta_relax_set_band called before ta_relax_init");
  RelaxState &rx = h->relax;
  const size_t N = h->keep_species.size(), F = h->keep_natoms.size();
  ta_band_params q = {0.1, 0, 0};  // ASE's spring constant
  if (on) {
    if (p) q = *p;
    if (F < 3) return fail(h, TA_ERR_INVALID, "ta_relax_set_band: a band needs at least 3 frames, the batch has " + std::to_string(F));
    const size_t n = (size_t)h->keep_natoms[0];
    for (size_t f = 1; f < F; ++f) {
      const std::string who = "ta_relax_set_band: frame " + std::to_string(f) + " differs from frame 0 in its ";
      if ((size_t)h->keep_natoms[f] != n) return fail(h, TA_ERR_INVALID, who + "atom count");
      if (!std::equal(h->keep_species.begin(), h->keep_species.begin() + n, h->keep_species.begin() + f * n))
        return fail(h, TA_ERR_INVALID, who + "species");
      if (!std::equal(h->ref_cells.begin(), h->ref_cells.begin() + 9, h->ref_cells.begin() + 9 * f))
        return fail(h, TA_ERR_INVALID, who + "cell");
      if (!std::equal(h->keep_pbc.begin(), h->keep_pbc.begin() + 3, h->keep_pbc.begin() + 3 * f))
        return fail(h, TA_ERR_INVALID, who + "pbc");
    }
    if (!std::isfinite(q.k) || !(q.k > 0.0)) return fail(h, TA_ERR_INVALID, "ta_relax_set_band: k must be finite and > 0");
    if (rx.cell.on)
      return fail(h, TA_ERR_INVALID, "ta_relax_set_band: the cell option is on (ta_relax_set_cell); cells along a band stay fixed");
  }
  return guarded(h, [&]() {
    auto &band = rx.band;
    HIP_CHECK(hipStreamSynchronize(h->stream));
    h->upload_pending = false;
    // the optimiser starts again, in either direction: v = 0, dt, a = astart, npos = 0, first
    band.state_host = fire_start(rx.p);
    rx.state_host.assign(F, band.state_host);
    if (N) HIP_CHECK(hipMemset(rx.vel.ptr, 0, 3 * N * sizeof(double)));
    band.ran = false;
    if (!on) {
      band.on = false;
      return;
    }
    const size_t n = (size_t)h->keep_natoms[0];
    band.force.ensure(3 * N + 1);
    band.tau.ensure(3 * N + 1);
    band.fixed.ensure(N + 1);
    band.state.ensure(2);
    band.layout.ensure(5);
    std::vector<uint8_t> mask(rx.fixed_host);  // the user's mask OR-ed with the two endpoint images
    mask.resize(N, 0);
    std::fill(mask.begin(), mask.begin() + n, 1);
    std::fill(mask.end() - n, mask.end(), 1);
    if (N) {
      HIP_CHECK(hipMemcpy(band.fixed.ptr, mask.data(), N, hipMemcpyHostToDevice));
      HIP_CHECK(hipMemset(band.force.ptr, 0, 3 * N * sizeof(double)));  // (the endpoints' rows stay 0)
      HIP_CHECK(hipMemset(band.tau.ptr, 0, 3 * N * sizeof(double)));
    }
    band.p = q;
    band.on = true;
  });
}

int ta_relax_get_band(ta_handle h, double *band_forces, double *tangents, double *energies, int32_t *climbing) {
  if (!h) return TA_ERR_INVALID;
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "ta_relax_get_band: no resident batch");
  if (!h->relax.valid) return fail(h, TA_ERR_INVALID, "ta_relax_get_band called before ta_relax_init");
  const auto &band = h->relax.band;
  if (!band.on) return fail(h, TA_ERR_INVALID, "ta_relax_get_band: the band option is off (ta_relax_set_band)");
  if (!band.ran)
    return fail(h, TA_ERR_INVALID, "ta_relax_get_band: no ta_relax_run of this band yet (max_steps = 0 counts)");
  return guarded(h, [&]() {
    const size_t N = h->keep_species.size(), F = h->keep_natoms.size();
    HIP_CHECK(hipStreamSynchronize(h->stream));
    h->upload_pending = false;
    if (band_forces && N) HIP_CHECK(hipMemcpy(band_forces, band.force.ptr, 3 * N * sizeof(double), hipMemcpyDeviceToHost));
    if (tangents && N) HIP_CHECK(hipMemcpy(tangents, band.tau.ptr, 3 * N * sizeof(double), hipMemcpyDeviceToHost));
    if (energies) std::memcpy(energies, band.energy_host.data(), F * sizeof(double));
    if (climbing) HIP_CHECK(hipMemcpy(climbing, band.layout.ptr + 4, sizeof(int32_t), hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
