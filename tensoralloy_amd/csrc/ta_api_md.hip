// C ABI of the device-resident MD loop: the ta_md_* entry points (include/tensoralloy_amd.h). The loop itself
// is in ta_resident.hip; the integrator (ta_md_mtk.hip: under the Martyna-Tobias-Klein barostat), correlation, pair-distribution, bond-angle and bond-order launches are in
// ta_md.hip, ta_md_corr.hip, ta_md_rdf.hip, ta_md_adf.hip and ta_md_order.hip; the cluster launches in
// ta_md_cluster.hip, the common neighbour analysis in ta_md_cna.hip, the structure-factor launches in ta_md_sq.hip,
// the heat-current and pressure-tensor launches in ta_md_flux.hip.
//
// The eight samplers (ta_md_set_sampling, _rdf, _adf, _order, _clusters, _cna, _sq, _flux) share one host-side lifecycle,
// written once below: md_alloc_layout, md_sampler_ready, md_sampler_off / md_sampler_set, and the loops of ta_md_init
// and ta_md_run. To add a sampler:
//   1. ta_sampler_text.h: its texts, a constant in md_text;
//   2. ta_context.h: a struct on MdSampler in MdState with its Setting, its buffers with the accessors that state their
//      layout, and its release(), and its place in for_each_sampler;
//   3. here: its md_alloc (buffer sizes and uploads), md_launch (the launch struct's run-constant fields) and md_enqueue
//      (where md_due says so: the fields of this launch and the launch, under the integrator's predicate with seq = k,
//      IN FRONT OF the integrator launch of step k or BEHIND it with the snapshot it wrote), its setter (parameter
//      checks, then md_sampler_off or md_sampler_set) and its getters (md_sampler_ready, fill_info, copy_series); its
//      cross-checks, if any, in md_run_refusals;
//   4. ta_md_run: its launch struct, its place in front of or behind the integrator in a step, and in the end_run order.
#include <cmath>
#include <cstring>

#include "ta_context.h"
#include "ta_md.h"

using namespace ta::host;

static_assert(sizeof(int64_t) == sizeof(unsigned long long), "the getters copy the counts as they are");

namespace {

// `chunk` consecutive items of one frame per workgroup, at least one workgroup per frame: the first workgroup of
// every frame, [F + 1], where frame f has per_atom * n_atoms items
std::vector<int32_t> frame_blocks(const ta_context *h, int per_atom, int chunk) {
  const size_t F = h->keep_natoms.size();
  std::vector<int32_t> start(F + 1, 0);
  for (size_t f = 0; f < F; ++f)
    start[f + 1] = start[f] + std::max(1, (per_atom * h->keep_natoms[f] + chunk - 1) / chunk);
  return start;
}

template <typename T>
void zero(DevBuf<T> &b, size_t n) {
  HIP_CHECK(hipMemset(b.ptr, 0, std::max<size_t>(n, 1) * sizeof(T)));
}
template <typename T>
void upload(DevBuf<T> &b, const std::vector<T> &v) {
  HIP_CHECK(hipMemcpy(b.ptr, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
}
// the squares of the cutoffs `r`[E][E] of a setting
void upload_squares(DevBuf<double> &b, std::vector<double> r) {
  for (double &x : r) x *= x;
  upload(b, r);
}

// Allocating sampler `x` for the resident batch, around the feature's own part: the stream is waited for (an earlier
// run's launches use the old buffers), everything is released, the launch's workgroup layout is planned (`chunk` of
// the frame's per_atom * n_atoms items each), try_buffers(n_blk) allocates the feature's buffers, fill() zeroes its
// accumulators and uploads its data, and the schedule starts with no sample taken. False when the device has no room
// (everything is released then); throws otherwise.
template <typename S, typename Try, typename Fill>
bool md_alloc_layout(ta_context *h, S &x, int64_t every, int per_atom, int chunk, Try &&try_buffers, Fill &&fill) {
  const size_t F = h->keep_natoms.size();
  HIP_CHECK(hipStreamSynchronize(h->stream));
  x.release();
  const std::vector<int32_t> start = frame_blocks(h, per_atom, chunk);
  if (!try_buffers((size_t)start[F]) || !x.blk.try_exact(F + 1)) {
    x.release();
    return false;
  }
  fill();
  upload(x.blk, start);
  x.n_blk = (int)start[F];
  x.chunk = chunk;
  x.sched.every = every;
  x.sched.start(h->md.step);
  x.sched.valid = true;
  return true;
}

// the part of a launch's list view that is fixed for a ta_md_run: the predicate's word and the plan of sampler x
void md_fixed_list(const ta_context *h, const MdSampler &x, ta::MdList &l) {
  l.blk_start = x.blk.ptr;
  l.status = h->res.status.ptr;
  l.n_elements = h->n_elements, l.n_frames = (int)h->keep_natoms.size();
  l.n_blk = x.n_blk, l.chunk = x.chunk;
}

// the neighbour-list view of launch `k` of a run: the state and the (skin) list of the batch, not the exact one filtered
// from it (a rebuild may have moved them: taken at every launch)
void point_at_list(const ta_context *h, ta::MdList &l, int k) {
  l.pos = h->db.pos;
  l.cells = h->db.cells;
  l.species = h->db.species;
  l.atom_start = h->db.atom_start;
  l.pair_start = h->pair_start.ptr;
  l.pair_j = h->pair_j.ptr;
  l.pair_shift = h->pair_shift.ptr;
  l.seq = (unsigned)k;
}

// Launch k of the run that began at absolute step step0 holds the whole-step state t = step0 + k; sampler x samples it
// when this says so. Sample number, ring slot and series row are functions of t alone (ta_schedule.h), so the launches
// that returned early behind a stale list and are enqueued again after the rebuild write what they would have written.
bool md_due(const MdSampler &x, int64_t step0, int k) { return x.run && x.sched.due(step0, k); }

// Where the integrator launch of a step writes the whole-step state (x, v) for the launches behind it: the slot of the
// correlation ring when md_set_sampling is due at launch k, else the rows of md_set_sq when that is due, else the rows
// of md_set_flux when that is due, else nowhere
struct MdSnapshot {
  double *x = nullptr, *v = nullptr;
};
MdSnapshot md_snapshot(const MdState::Corr &corr, const MdState::Sq &sq, const MdState::Flux &flux, size_t N, int64_t step0,
                       int k) {
  if (md_due(corr, step0, k)) {
    const int64_t n = corr.sched.index(step0 + k);
    return {corr.slot(corr.ring_x, n, N), corr.slot(corr.ring_v, n, N)};
  }
  if (md_due(sq, step0, k)) return {sq.snap_x.ptr, sq.snap_v.ptr};
  if (md_due(flux, step0, k)) return {flux.snap_x.ptr, flux.snap_v.ptr};
  return {};
}

// Every sampler x has three functions, one beside the other. md_alloc(h, x, s): x allocated for setting `s` (its own, or
// a setter's candidate) as md_alloc_layout says. md_launch(h, x): its launch struct with every field that is fixed for
// a ta_md_run (a pointer into a part of a buffer stays null while the sampler is not in the run). md_enqueue: see the file's head.
// Here: the rings, the accumulators and the partials of the correlation launch
bool md_alloc(ta_context *h, MdState::Corr &c, const MdState::Corr::Setting &s) {
  const size_t N = h->keep_species.size(), F = h->keep_natoms.size();
  const size_t L = (size_t)s.p.n_lags, E = (size_t)h->n_elements, n_acc = s.n_acc(F, E);
  return md_alloc_layout(
      h, c, s.p.sample_every, 3, ta::kMdCorrChunk,
      [&](size_t n_blk) {
        return c.ring_x.try_exact(L * 3 * N) && c.ring_v.try_exact(L * 3 * N) && c.acc.try_exact(n_acc) &&
               c.part.try_exact(n_blk * 2 * E * L);
      },
      [&]() { zero(c.acc, n_acc); });
}
ta::MdCorrLaunch md_launch(const ta_context *h, const MdState::Corr &x) {
  const size_t F = h->keep_natoms.size(), E = (size_t)h->n_elements;
  ta::MdCorrLaunch c;
  c.ring_x = x.ring_x.ptr, c.ring_v = x.ring_v.ptr;
  c.blk_start = x.blk.ptr, c.part = x.part.ptr;
  c.acc_v = x.acc_v(), c.acc_x = x.run ? x.acc_x(F, E) : nullptr;
  c.status = h->res.status.ptr;
  c.n_atoms = (long long)h->keep_species.size();
  c.n_lags = x.set.p.n_lags, c.n_elements = h->n_elements, c.n_frames = (int)F, c.n_chunks = x.n_blk;
  return c;
}
// directly behind the launch that sampled into the ring, under the same predicate
void md_enqueue(const ta_context *h, const MdState::Corr &x, ta::MdCorrLaunch &c, int64_t step0, int k, const MdSnapshot &) {
  if (!md_due(x, step0, k)) return;
  c.species = h->db.species, c.atom_start = h->db.atom_start;
  c.seq = (unsigned)k, c.n = (long long)x.sched.index(step0 + k);
  ta::launch_md_correlate(c, h->stream);
  HIP_CHECK(hipGetLastError());
}

// the counts
bool md_alloc(ta_context *h, MdState::Rdf &g, const MdState::Rdf::Setting &s) {
  const size_t N = h->keep_species.size(), F = h->keep_natoms.size();
  const size_t E = (size_t)h->n_elements, n_acc = F * E * E * (size_t)s.p.n_bins;
  return md_alloc_layout(
      h, g, s.p.sample_every, 1, ta::md_rdf_chunk((long long)N), [&](size_t) { return g.acc.try_exact(n_acc); },
      [&]() { zero(g.acc, n_acc); });
}
ta::MdRdfLaunch md_launch(const ta_context *h, const MdState::Rdf &x) {
  ta::MdRdfLaunch g;
  md_fixed_list(h, x, g.list);
  g.counts = x.acc.ptr, g.n_bins = x.set.p.n_bins;
  g.dr = x.run ? x.set.p.r_max / (double)x.set.p.n_bins : 1.0;
  return g;
}
// Pair distributions: the state t = step0 + k is counted by a launch IN FRONT OF the integrator launch of step k, whose
// drift leaves x(t). With seq = k the integrator's predicate skips exactly the states that were reached on a stale
// list; after the rebuild the launch is enqueued again with the rest and counts then.
void md_enqueue(const ta_context *h, const MdState::Rdf &x, ta::MdRdfLaunch &g, int64_t step0, int k) {
  if (!md_due(x, step0, k)) return;
  point_at_list(h, g.list, k);
  g.pair_i = h->pair_i.ptr;
  ta::launch_md_rdf(g, h->stream);
  HIP_CHECK(hipGetLastError());
}

// the counts and the squared cutoffs
bool md_alloc(ta_context *h, MdState::Adf &g, const MdState::Adf::Setting &s) {
  const size_t N = h->keep_species.size(), F = h->keep_natoms.size();
  const size_t E = (size_t)h->n_elements, n_acc = F * E * (E * (E + 1) / 2) * (size_t)s.p.n_bins;
  return md_alloc_layout(
      h, g, s.p.sample_every, 1, ta::md_adf_chunk((long long)N),
      [&](size_t) { return g.acc.try_exact(n_acc) && g.rb2.try_exact(E * E); },
      [&]() {
        zero(g.acc, n_acc);
        upload_squares(g.rb2, s.rb);
      });
}
ta::MdAdfLaunch md_launch(const ta_context *h, const MdState::Adf &x) {
  ta::MdAdfLaunch t;
  md_fixed_list(h, x, t.list);
  t.rb2 = x.rb2.ptr, t.counts = x.acc.ptr, t.n_bins = x.set.p.n_bins;
  t.dtheta = x.run ? M_PI / (double)x.set.p.n_bins : 1.0;
  return t;
}
// Bond-angle distributions: a launch of their own in the same place as the pair distributions', under the same
// predicate (no volume enters, so they run under the barostat too: db.cells are those of the state t)
void md_enqueue(const ta_context *h, const MdState::Adf &x, ta::MdAdfLaunch &t, int64_t step0, int k) {
  if (!md_due(x, step0, k)) return;
  point_at_list(h, t.list, k);
  ta::launch_md_adf(t, h->stream);
  HIP_CHECK(hipGetLastError());
}

// the counts, the squared cutoffs, the N_lm and the per-atom arrays
bool md_alloc(ta_context *h, MdState::Order &g, const MdState::Order::Setting &s) {
  const size_t N = h->keep_species.size(), F = h->keep_natoms.size();
  const size_t E = (size_t)h->n_elements, n_acc = s.n_acc(F, E);
  // N_lm = sqrt((2 l + 1) / (4 pi) (l - m)! / (l + m)!), degree by degree, m = 0 .. l
  std::vector<double> norm;
  int solid = 0;
  for (int d = 0; d < s.p.n_degrees; ++d) {
    const int l = s.p.degrees[d];
    if (l == s.p.solid_degree) solid = d;
    for (int m = 0; m <= l; ++m) {
      long double ratio = 1.0L;
      for (int k = l - m + 1; k <= l + m; ++k) ratio /= (long double)k;
      norm.push_back((double)std::sqrt((long double)(2 * l + 1) / (4.0L * 3.14159265358979323846264338327950288L) * ratio));
    }
  }
  const size_t M = norm.size();
  return md_alloc_layout(
      h, g, s.p.sample_every, 1, ta::md_order_chunk((long long)N),
      [&](size_t) {
        return g.acc.try_exact(n_acc) && g.rb2.try_exact(E * E) && g.norm.try_exact(M) && g.qlm.try_exact(2 * M * N + 1) &&
               g.per_atom.try_exact(2 * s.n_q(N) + 1) && g.per_atom_int.try_exact(2 * N + 1);
      },
      [&]() {
        zero(g.acc, n_acc);
        upload_squares(g.rb2, s.rb);
        upload(g.norm, norm);
        g.n_lm = (int)M;
        g.solid = solid;
      });
}
ta::MdOrderLaunch md_launch(const ta_context *h, const MdState::Order &x) {
  const size_t N = h->keep_species.size(), F = h->keep_natoms.size(), E = (size_t)h->n_elements;
  const auto &p = x.set.p;
  ta::MdOrderLaunch o;
  md_fixed_list(h, x, o.list);
  o.rb2 = x.rb2.ptr, o.norm = x.norm.ptr, o.qlm = x.qlm.ptr;
  o.q = x.q(), o.qbar = x.run ? x.qbar(N) : nullptr;
  o.n_bonds = x.n_bonds(), o.n_conn = x.run ? x.n_conn(N) : nullptr;
  o.hist_q = x.hist_q();
  o.hist_qbar = x.run ? x.hist_qbar(F, E) : nullptr, o.hist_conn = x.run ? x.hist_conn(F, E) : nullptr;
  o.n_bins = p.n_bins;
  o.n_degrees = p.n_degrees, o.n_lm = x.n_lm, o.solid = x.solid;
  o.deg0 = p.degrees[0], o.deg1 = p.degrees[1], o.deg2 = p.degrees[2], o.deg3 = p.degrees[3];
  o.threshold = p.solid_threshold;
  return o;
}
// Bond-orientational order: its two launches in the same place as the pair distributions', under the same predicate
// (no volume either)
void md_enqueue(const ta_context *h, const MdState::Order &x, ta::MdOrderLaunch &o, int64_t step0, int k) {
  if (!md_due(x, step0, k)) return;
  point_at_list(h, o.list, k);
  ta::launch_md_order(o, h->stream);
  HIP_CHECK(hipGetLastError());
}

// the histogram, the series, the give-up word, the squared cutoffs and the per-atom arrays; the layout is the link
// launch's
bool md_alloc(ta_context *h, MdState::Cluster &g, const MdState::Cluster::Setting &s) {
  static_assert(TA_MD_MAX_BINS <= ta::kMdClusterLdsWords, "the summary launch keeps all bins of a frame in LDS");
  const size_t N = h->keep_species.size(), F = h->keep_natoms.size(), E = (size_t)h->n_elements;
  const size_t n_hist = s.n_hist(F), n_series = s.n_series(F);
  return md_alloc_layout(
      h, g, s.p.sample_every, 1, ta::md_order_chunk((long long)N),
      [&](size_t) {
        return g.acc.try_exact(n_hist) && g.series.try_exact(n_series) && g.rl2.try_exact(E * E) &&
               g.per_atom.try_exact(g.n_per_atom(N) + 1) && g.giveup.try_exact(4);
      },
      [&]() {
        zero(g.acc, n_hist);
        zero(g.series, n_series);
        zero(g.giveup, 4);
        upload_squares(g.rl2, s.rl);
      });
}
ta::MdClusterLaunch md_launch(const ta_context *h, const MdState::Cluster &x) {
  const size_t N = h->keep_species.size();
  ta::MdClusterLaunch cl;
  md_fixed_list(h, x, cl.list);
  cl.rl2 = x.rl2.ptr, cl.hist = x.acc.ptr, cl.giveup = x.giveup.ptr;
  cl.n_conn = x.run && x.set.p.n_min > 0 ? h->md.order.n_conn(N) : nullptr;
  cl.parent = x.parent(), cl.count = x.run ? x.count(N) : nullptr;
  cl.label = x.run ? x.label(N) : nullptr, cl.size = x.run ? x.size(N) : nullptr;
  cl.n_atoms = (long long)N;
  cl.n_bins = x.set.p.n_bins;
  cl.n_min = x.set.p.n_min, cl.species_mask = x.set.p.species_mask;
  return cl;
}
// Clusters: four launches in the same place as the pair distributions', behind the order launches of the step (n_min > 0
// reads their n_conn), under the same predicate (no volume either)
void md_enqueue(const ta_context *h, const MdState::Cluster &x, ta::MdClusterLaunch &cl, int64_t step0, int k) {
  if (!md_due(x, step0, k)) return;
  point_at_list(h, cl.list, k);
  cl.row = x.series_row(x.sched.index(step0 + k), h->keep_natoms.size());
  ta::launch_md_cluster(cl, h->stream);
  HIP_CHECK(hipGetLastError());
}

// the counts, the series and the per-atom arrays
bool md_alloc(ta_context *h, MdState::Cna &g, const MdState::Cna::Setting &s) {
  static_assert(TA_MD_CNA_TYPES == ta::kMdCnaTypes && TA_MD_CNA_ADAPTIVE == ta::kMdCnaAdaptive &&
                    TA_MD_CNA_FIXED == ta::kMdCnaFixed, "the header and the launch agree");
  const size_t N = h->keep_species.size(), F = h->keep_natoms.size(), E = (size_t)h->n_elements;
  const size_t n_acc = s.n_acc(F, E), n_series = s.n_series(F);
  return md_alloc_layout(
      h, g, s.p.sample_every, 1, ta::md_order_chunk((long long)N),
      [&](size_t) {
        return g.acc.try_exact(n_acc) && g.series.try_exact(n_series) && g.structure.try_exact(N + 1) &&
               g.r_local.try_exact(N + 1);
      },
      [&]() {
        zero(g.acc, n_acc);
        zero(g.series, n_series);
      });
}
ta::MdCnaLaunch md_launch(const ta_context *h, const MdState::Cna &x) {
  const auto &p = x.set.p;
  const double r = p.mode == TA_MD_CNA_FIXED ? p.r_cut : p.r_max;
  ta::MdCnaLaunch cn;
  md_fixed_list(h, x, cn.list);
  cn.structure = x.structure.ptr, cn.r_local = x.r_local.ptr, cn.counts = x.acc.ptr;
  cn.mode = p.mode, cn.r_cut = p.r_cut, cn.r2 = r * r;
  return cn;
}
// Common neighbour analysis: its launch in the same place as the pair distributions', behind the order and cluster
// launches, under the same predicate (no volume either); sample n counts into row n % n_series, which a launch in front
// zeroes
void md_enqueue(const ta_context *h, const MdState::Cna &x, ta::MdCnaLaunch &cn, int64_t step0, int k) {
  if (!md_due(x, step0, k)) return;
  point_at_list(h, cn.list, k);
  cn.row = x.series_row(x.sched.index(step0 + k), h->keep_natoms.size());
  ta::launch_md_cna(cn, h->stream);
  HIP_CHECK(hipGetLastError());
}

// the Miller triples, an empty ring, the accumulators, the partials of the amplitude launch and the snapshot rows
bool md_alloc(ta_context *h, MdState::Sq &g, const MdState::Sq::Setting &s) {
  const size_t N = h->keep_species.size(), F = h->keep_natoms.size();
  const size_t E = (size_t)h->n_elements, Q = (size_t)s.p.n_q, L = (size_t)s.p.n_lags, n_acc = s.n_acc(F, E);
  return md_alloc_layout(
      h, g, s.p.sample_every, 1, ta::md_sq_chunk((long long)N),
      [&](size_t n_blk) {
        return g.acc.try_exact(n_acc) && g.ring.try_exact(L * s.row(F, E)) && g.part.try_exact(n_blk * E * s.planes() * Q) &&
               g.snap_x.try_exact(3 * N) && g.snap_v.try_exact(3 * N) && g.miller_dev.try_exact(3 * Q);
      },
      [&]() {
        zero(g.acc, n_acc);
        upload(g.miller_dev, s.miller);
      });
}
ta::MdSqLaunch md_launch(const ta_context *h, const MdState::Sq &x) {
  const size_t F = h->keep_natoms.size(), E = (size_t)h->n_elements;
  const auto &p = x.set.p;
  ta::MdSqLaunch u;
  u.blk_start = x.blk.ptr, u.miller = x.miller_dev.ptr, u.part = x.part.ptr, u.ring = x.ring.ptr;
  u.acc_rho = x.acc_rho(), u.status = h->res.status.ptr;
  u.acc_l = x.run && p.currents ? x.acc_l(F, E) : nullptr, u.acc_j = x.run && p.currents ? x.acc_j(F, E) : nullptr;
  u.n_q = p.n_q, u.n_lags = p.n_lags, u.n_elements = h->n_elements, u.n_frames = (int)F;
  u.n_blk = x.n_blk, u.chunk = x.chunk, u.currents = p.currents;
  return u;
}
// Structure factors: the integrator launch of a due step writes the whole-step state (x, v) where md_snapshot says; the
// three launches go BEHIND it, under the same predicate, and read that snapshot
void md_enqueue(const ta_context *h, const MdState::Sq &x, ta::MdSqLaunch &u, int64_t step0, int k, const MdSnapshot &snap) {
  if (!md_due(x, step0, k)) return;
  u.x = snap.x, u.v = snap.v;
  u.cells = h->db.cells, u.species = h->db.species, u.atom_start = h->db.atom_start;
  u.seq = (unsigned)k, u.n = (long long)x.sched.index(step0 + k);
  ta::launch_md_sq(u, h->stream);
  HIP_CHECK(hipGetLastError());
}

// an empty ring, the accumulators {sums, a_heat, a_press}, the partials of the pair sweep and the snapshot rows
bool md_alloc(ta_context *h, MdState::Flux &g, const MdState::Flux::Setting &s) {
  static_assert(TA_MD_FLUX_ROW == ta::kMdFluxRow, "the header and the launch agree");
  const size_t N = h->keep_species.size(), F = h->keep_natoms.size(), L = (size_t)s.p.n_lags, R = ta::kMdFluxRow;
  const size_t n_acc = s.n_acc(F);
  return md_alloc_layout(
      h, g, s.p.sample_every, 1, ta::md_flux_chunk((long long)N),
      [&](size_t n_blk) {
        return g.acc.try_exact(n_acc) && g.ring.try_exact(L * s.row(F)) && g.part.try_exact(n_blk * R) &&
               g.snap_x.try_exact(3 * N) && g.snap_v.try_exact(3 * N);
      },
      [&]() { zero(g.acc, n_acc); });
}
ta::MdFluxLaunch md_launch(const ta_context *h, const MdState::Flux &x) {
  const size_t F = h->keep_natoms.size();
  ta::MdFluxLaunch fx;
  fx.mass = h->md.mass.ptr, fx.blk_start = x.blk.ptr, fx.part = x.part.ptr, fx.ring = x.ring.ptr;
  fx.sums = x.sums(), fx.status = h->res.status.ptr;
  fx.acc_heat = x.run ? x.acc_heat(F) : nullptr, fx.acc_press = x.run ? x.acc_press(F) : nullptr;
  fx.n_lags = x.set.p.n_lags, fx.n_frames = (int)F, fx.n_blk = x.n_blk, fx.chunk = x.chunk;
  return fx;
}
// Heat current and pressure tensor: the three launches go BEHIND the integrator launch as well (v(t) exists only after
// its closing half-kick), under the same predicate. They read the velocities of the snapshot (md_snapshot) and, through
// DeviceBatch, the list, pair records, g and eatom of the evaluation of x(t), which nothing rewrites before the next
// compute_impl, enqueued behind them.
void md_enqueue(const ta_context *h, const MdState::Flux &x, ta::MdFluxLaunch &fx, int64_t step0, int k, const MdSnapshot &snap) {
  if (!md_due(x, step0, k)) return;
  fx.v = snap.v, fx.seq = (unsigned)k, fx.n = (long long)x.sched.index(step0 + k);
  ta::launch_md_flux(fx, h->db, h->stream);
  HIP_CHECK(hipGetLastError());
}

// What ta_md_set_sq and the barostat ask of the resident frames: periodic along all three axes, a cell that can be
// inverted. The messages begin with `who` and say `why` of the first. Returns 0 or the error code.
int md_frames_periodic(ta_context *h, const std::string &who, const char *why) {
  const size_t F = h->keep_natoms.size();
  for (size_t f = 0; f < F; ++f) {
    for (int k = 0; k < 3; ++k)
      if (!h->keep_pbc[3 * f + k])
        return fail(h, TA_ERR_INVALID, who + "frame " + std::to_string(f) + " is not periodic along all three axes" + why);
    const double *c = h->ref_cells.data() + 9 * f;
    const double det = c[0] * (c[4] * c[8] - c[5] * c[7]) - c[1] * (c[3] * c[8] - c[5] * c[6]) + c[2] * (c[3] * c[7] - c[4] * c[6]);
    if (!std::isfinite(det) || !(std::fabs(det) > 0.0))
      return fail(h, TA_ERR_INVALID, who + "the cell of frame " + std::to_string(f) + " is singular");
  }
  return TA_OK;
}
int md_sq_frames(ta_context *h) { return md_frames_periodic(h, "ta_md_set_sq: ", "; the wave vectors are those of the cell"); }

// The bond cutoffs [E][E] of ta_md_set_adf, ta_md_set_order and ta_md_set_clusters (`who`): r_bond for every pair, or
// r_bond_pairs; the messages call them `one` and `pairs`. Returns 0 with `rb` filled, or the error code: a cutoff
// not finite, <= 0 or above the model's, or no symmetry.
int md_bond_cutoffs(ta_context *h, const std::string &who, double r_bond, const double *r_bond_pairs, std::vector<double> &rb,
                    const char *one = "r_bond", const char *pairs = "r_bond_pairs") {
  const size_t E = (size_t)h->n_elements;
  rb.assign(E * E, r_bond);
  if (r_bond_pairs) rb.assign(r_bond_pairs, r_bond_pairs + E * E);
  const char *name = r_bond_pairs ? pairs : one;
  for (size_t k = 0; k < E * E; ++k) {
    const std::string what = who + ": " + name +
                             (r_bond_pairs ? "[" + std::to_string(k / E) + "][" + std::to_string(k % E) + "]" : std::string());
    if (!std::isfinite(rb[k]) || !(rb[k] > 0.0)) return fail(h, TA_ERR_INVALID, what + " must be a finite distance > 0");
    if (rb[k] > h->rmax)
      return fail(h, TA_ERR_INVALID, what + " = " + std::to_string(rb[k]) + " exceeds the model's cutoff max(rcut, acut) = " +
                                     std::to_string(h->rmax) + "; the neighbour list is not complete beyond that");
  }
  for (size_t a = 0; a < E; ++a)
    for (size_t b = a + 1; b < E; ++b)
      if (rb[a * E + b] != rb[b * E + a])
        return fail(h, TA_ERR_INVALID, who + ": " + pairs + " is not symmetric: [" + std::to_string(a) + "][" +
                                       std::to_string(b) + "] differs from [" + std::to_string(b) + "][" + std::to_string(a) + "]");
  return TA_OK;
}

// what every call about the resident MD state needs; returns 0 or the error code
int md_resident(ta_context *h, const std::string &who) {
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, who + ": no resident batch");
  if (!h->md.valid) return fail(h, TA_ERR_INVALID, who + " called before ta_md_init");
  return TA_OK;
}

// what ta_md_get_chain and ta_md_set_chain need; returns 0 or the error code
int md_chain_ready(ta_context *h, const char *who) {
  if (const int rc = md_resident(h, who)) return rc;
  if (!h->md.nhc.on)
    return fail(h, TA_ERR_INVALID, std::string(who) + ": the Nose-Hoover chain thermostat is off (ta_md_set_nose_hoover)");
  return TA_OK;
}

// what ta_md_get_mtk_state and ta_md_set_mtk_state need; returns 0 or the error code
int md_mtk_ready(ta_context *h, const char *who) {
  if (const int rc = md_resident(h, who)) return rc;
  if (!h->md.mtk.on)
    return fail(h, TA_ERR_INVALID, std::string(who) + ": the Martyna-Tobias-Klein barostat is off (ta_md_set_mtk_barostat)");
  return TA_OK;
}

// what the getters of sampler `x` need: it is on and holds the data of runs that succeeded; returns 0 or the error code
int md_sampler_ready(ta_context *h, const MdSampler &x, const char *who) {
  if (const int rc = md_resident(h, who)) return rc;
  if (!x.on) return fail(h, TA_ERR_INVALID, ta::md_text_off(x.text, who));
  if (!x.sched.valid) return fail(h, TA_ERR_INVALID, ta::md_text_invalid(x.text, who));
  return TA_OK;
}

// A setter whose parameters say "off": the sampler goes off and gives back what it holds on the device
template <typename S>
int md_sampler_off(ta_context *h, S &x) {
  x.on = false;
  return guarded(h, [&]() {
    HIP_CHECK(hipStreamSynchronize(h->stream));
    x.release();
  });
}

// A setter whose parameters passed its checks: with a resident batch behind ta_md_init (that batch_check, if any,
// accepts), sampler x is allocated for the candidate `s` and keeps it as its setting. It is off while that has not
// succeeded; TA_ERR_NOMEM names `what` there was no room for.
template <typename S>
int md_sampler_set(ta_context *h, S &x, const typename S::Setting &s, const std::string &what,
                   int (*batch_check)(ta_context *) = nullptr) {
  if (const int rc = md_resident(h, x.text.setter)) return rc;
  if (batch_check)
    if (const int rc = batch_check(h)) return rc;
  bool nomem = false;
  const int rc = guarded(h, [&]() {
    x.on = false;  // (until the buffers exist)
    nomem = !md_alloc(h, x, s);
    if (!nomem) {
      x.set = s;
      x.on = true;
    }
  });
  if (rc == TA_OK && nomem) return fail(h, TA_ERR_NOMEM, ta::md_text_nomem(x.text, x.text.setter, what));
  return rc;
}

// What ta_md_run refuses before anything is touched: its arguments, the resident frames under the barostat and the
// chain, the samplers that exclude the barostat, and what the clusters need of the order parameters. Returns 0 or the
// error code.
int md_run_refusals(ta_context *h, int32_t n_steps, double dt, int32_t record_every) {
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "ta_md_run: no resident batch");
  if (!h->md.valid) return fail(h, TA_ERR_INVALID, "ta_md_run called before ta_md_init (ta_set_frames drops the MD state)");
  if (n_steps < 0 || record_every < 1) return fail(h, TA_ERR_INVALID, "ta_md_run: n_steps >= 0 and record_every >= 1 are needed");
  if (!std::isfinite(dt)) return fail(h, TA_ERR_INVALID, "ta_md_run: dt must be finite");
  const MdState &md = h->md;
  if (md.langevin.friction > 0.0 && dt < 0.0) return fail(h, TA_ERR_INVALID, "ta_md_run: Langevin dynamics needs dt >= 0");
  const bool baro = md.moves_cells();
  if (md.mtk.on) {  // it is coupled to the particle chain and takes kT0 from it
    if (md.berendsen.kT0 > 0.0)
      return fail(h, TA_ERR_INVALID, "ta_md_run: the Martyna-Tobias-Klein barostat (ta_md_set_mtk_barostat) is on and so is the "
                                     "Berendsen thermostat; it needs the Nose-Hoover chain (ta_md_set_nose_hoover) instead");
    if (md.langevin.friction > 0.0)
      return fail(h, TA_ERR_INVALID, "ta_md_run: the Martyna-Tobias-Klein barostat (ta_md_set_mtk_barostat) is on and so is the "
                                     "Langevin thermostat; it needs the Nose-Hoover chain (ta_md_set_nose_hoover) instead");
    if (!md.nhc.on)
      return fail(h, TA_ERR_INVALID, "ta_md_run: the Martyna-Tobias-Klein barostat (ta_md_set_mtk_barostat) is on and the "
                                     "Nose-Hoover chain thermostat is off (ta_md_set_nose_hoover); it takes kT0 from the chain");
  }
  if (baro)
    if (const int bad = md_frames_periodic(h, "ta_md_run: the barostat is on and ", "")) return bad;
  for (size_t f = 0; md.nhc.on && f < h->keep_natoms.size(); ++f)
    if (3 * (int64_t)h->keep_natoms[f] - (int64_t)md.nhc.p.dof_removed < 1)
      return fail(h, TA_ERR_INVALID, "ta_md_run: the Nose-Hoover chain is on and frame " + std::to_string(f) +
                                     " has fewer than one degree of freedom (3 n_atoms - dof_removed)");
  // the samplers that need one cell for the whole run, in the order they are refused in
  const std::pair<bool, const char *> no_barostat[] = {
      {md.corr.on, "ta_md_run: sampling (ta_md_set_sampling) and the barostat (ta_md_set_barostat) are both on; "
                   "displacements in a moving cell are not defined: switch one of them off"},
      {md.rdf.on, "ta_md_run: the pair distributions (ta_md_set_rdf) and the barostat (ta_md_set_barostat) are both on; "
                  "normalising the counts needs one volume: switch one of them off"},
      {md.sq.on, "ta_md_run: the structure factors (ta_md_set_sq) and the barostat (ta_md_set_barostat) are both on; cell "
                 "and positions of a snapshot would belong to different states: switch one of them off"},
      {md.flux.on, "ta_md_run: the heat current and pressure tensor (ta_md_set_flux) and the barostat (ta_md_set_barostat) "
                   "are both on; normalising the correlations needs one volume: switch one of them off"}};
  for (const auto &x : no_barostat)
    if (x.first && baro) {
      std::string why = x.second;  // (the same reasons under either barostat: the one that is on is named)
      if (md.mtk.on) why.replace(why.find("ta_md_set_barostat"), std::strlen("ta_md_set_barostat"), "ta_md_set_mtk_barostat");
      return fail(h, TA_ERR_INVALID, why);
    }
  if (md.cluster.on && md.cluster.set.p.n_min > 0) {  // n_conn of the order launches for the same state is read
    if (!md.order.on)
      return fail(h, TA_ERR_INVALID, "ta_md_run: the cluster analysis (ta_md_set_clusters) has n_min > 0 and reads n_conn, but "
                                     "the bond-orientational order parameters (ta_md_set_order) are off");
    if (!md.order.sched.valid)
      return fail(h, TA_ERR_INVALID, "ta_md_run: the cluster analysis (ta_md_set_clusters) has n_min > 0 and reads n_conn, but a "
                                     "ta_md_run failed and left the data of ta_md_set_order invalid; call ta_md_set_order again");
    if (md.cluster.set.p.sample_every % md.order.set.p.sample_every != 0)
      return fail(h, TA_ERR_INVALID, "ta_md_run: the cluster analysis (ta_md_set_clusters) has n_min > 0 and its sample_every = " +
                                     std::to_string(md.cluster.set.p.sample_every) + " is no multiple of that of ta_md_set_order, " +
                                     std::to_string(md.order.set.p.sample_every) + ": n_conn of a sampled state would be missing");
    if (md.cluster.sched.origin < md.order.sched.origin)
      return fail(h, TA_ERR_INVALID, "ta_md_run: the cluster analysis (ta_md_set_clusters) has n_min > 0 and its first sample, step " +
                                     std::to_string(md.cluster.sched.origin) + ", is in front of the first one of ta_md_set_order, "
                                     "step " + std::to_string(md.order.sched.origin) + ": switch the order parameters on first");
  }
  return TA_OK;
}

// The integrator launch's arguments that are fixed for a ta_md_run of time step dt in workgroups of `chunk` atoms: the
// buffers, the thermostat that is on (Berendsen, Langevin or the chain; never two), the barostat and the skin
ta::MdLaunch md_launch(const ta_context *h, double dt, int chunk) {
  const MdState &md = h->md;
  const ResidentLoop &res = h->res;
  const bool thermostat = md.berendsen.kT0 > 0.0, langevin = md.langevin.friction > 0.0, baro = md.moves_cells(), nhc = md.nhc.on;
  ta::MdLaunch a;
  a.vel = md.vel.ptr, a.mass = md.mass.ptr, a.epot = md.epot.ptr, a.ke_part = md.ke.ptr;
  a.ref = res.ref.ptr, a.blk_start = res.blk_start.ptr;
  a.status = res.status.ptr, a.status_host = const_cast<unsigned *>(res.host_words());
  a.dt = dt;
  a.kT0 = langevin ? md.langevin.kT0 : md.berendsen.kT0;
  a.dt_over_tau = thermostat ? dt / md.berendsen.tau : 0.0;
  a.langevin = langevin ? 1 : 0, a.seed = md.langevin.seed;
  a.c1 = a.c2 = a.c3 = a.c4 = a.c5 = 0.0;
  if (langevin) {  // ASE's Langevin.updatevars with sigma_i = sqrt(2 kT0 fr) / sqrt(m_i)
    const double fr = md.langevin.friction, sigma = std::sqrt(2.0 * md.langevin.kT0 * fr);
    a.c1 = dt / 2.0 - dt * dt * fr / 8.0;
    a.c2 = dt * fr / 2.0 - dt * dt * fr * fr / 8.0;
    a.c3 = std::sqrt(dt) * sigma / 2.0 - std::pow(dt, 1.5) * fr * sigma / 8.0;
    a.c5 = std::pow(dt, 1.5) * sigma / (2.0 * std::sqrt(3.0));
    a.c4 = fr / 2.0 * a.c5;
  }
  a.lim2 = h->skin > 0.0 ? 0.25 * h->skin * h->skin : -1.0;  // skin = 0: every step rebuilds
  a.n_frames = (int)h->keep_natoms.size(), a.n_blk = res.n_blk, a.chunk = chunk;
  a.baro = baro ? 1 : 0, a.baro_iso = md.baro.p.isotropic ? 1 : 0;
  a.cells = nullptr, a.virial = nullptr;
  a.baro_scale = md.baro.scale.ptr, a.baro_rec = md.baro.rec.ptr;
  a.baro_p0 = md.baro.p.pressure;
  a.baro_k = md.baro.on ? dt / md.baro.p.taup * md.baro.p.compressibility / 3.0 : 0.0;
  for (int c = 0; c < 3; ++c) a.baro_mask[c] = md.baro.p.mask[c] ? 1 : 0;
  a.skin = h->skin, a.r_list = h->rmax + h->skin;
  a.nhc = nhc ? 1 : 0;
  a.nhc_chain = md.nhc.p.chain, a.nhc_loops = md.nhc.p.loops, a.nhc_dof = md.nhc.p.dof_removed;
  a.nhc_kT0 = nhc ? md.nhc.p.kT0 : 0.0;
  a.nhc_q = nhc ? md.nhc.p.kT0 * md.nhc.p.tau * md.nhc.p.tau : 0.0;
  a.nhc_eta = md.nhc.eta.ptr, a.nhc_veta = md.nhc.veta.ptr, a.nhc_rec = md.nhc.rec.ptr;
  return a;
}
// The Martyna-Tobias-Klein launch's arguments beside those (fixed for a ta_md_run)
ta::MdMtkLaunch md_mtk_launch(const ta_context *h) {
  const MdState &md = h->md;
  ta::MdMtkLaunch b;
  b.omega = md.mtk.omega.ptr, b.xi = md.mtk.xi.ptr, b.vxi = md.mtk.vxi.ptr, b.rec = md.mtk.rec.ptr;
  b.p0 = md.mtk.p.pressure;
  b.q = md.mtk.on ? md.nhc.p.kT0 * md.mtk.p.tau_p * md.mtk.p.tau_p : 0.0;
  b.chain = md.mtk.p.chain, b.loops = md.mtk.p.loops, b.iso = md.mtk.p.isotropic ? 1 : 0;
  for (int c = 0; c < 3; ++c) b.mask[c] = md.mtk.p.mask[c] ? 1 : 0;
  return b;
}
// The integrator launch k of the run that began at absolute step step0: it finishes step k - 1, records every
// record_every-th state, writes the snapshot and, with `drift`, begins step k
void md_enqueue(const ta_context *h, ta::MdLaunch &a, const ta::MdMtkLaunch &mtk, int threads, int64_t step0, int k,
                bool drift, int record_every, const MdSnapshot &snap) {
  // (a rebuild may have moved the batch's arrays: the pointers are taken at every launch)
  a.pos = h->db.pos, a.forces = h->db.forces, a.energy = h->db.energy, a.atom_start = h->db.atom_start;
  a.cells = h->db.cells, a.virial = h->db.virial;
  a.seq = (unsigned)k, a.step = (long long)(step0 + k);  // (a step redone after a rebuild keeps its index)
  a.kick2 = k > 0 ? 1 : 0;  // the state at entry is a whole step
  a.drift = drift ? 1 : 0;
  a.rec = (k % record_every == 0) ? (long long)(k / record_every) : -1;
  a.snap_x = snap.x, a.snap_v = snap.v;
  if (h->md.mtk.on)  // (no sampler that takes a snapshot runs under a barostat)
    ta::launch_md_mtk(a, mtk, h->stream);
  else
    ta::launch_md_integrate(a, threads, h->stream);
  HIP_CHECK(hipGetLastError());
}

// What a ta_md_run that succeeded leaves on the host, n_rec records each: the barostat's {V, P} (with the final cells on
// a list of their own, and handed to a cell relaxation whose cells they replace: `cells_at_entry` are those the run
// began with), the chain's terms, and to `epot` and `ekin` (either may be null) the potential energy and the kinetic
// energy summed over a frame's workgroups
void md_read_records(ta_context *h, size_t n_rec, uint32_t want, const std::vector<double> &cells_at_entry, double *epot,
                     double *ekin, int *rebuilds, int32_t *n_rebuilds) {
  MdState &md = h->md;
  const size_t F = h->keep_natoms.size(), n_blk = (size_t)h->res.n_blk;
  if (md.moves_cells() && F) {
    std::vector<double> rec(4 * n_rec * F);
    HIP_CHECK(hipMemcpy(rec.data(), md.baro.rec.ptr, rec.size() * sizeof(double), hipMemcpyDeviceToHost));
    md.baro.rec_volume.resize(n_rec * F);
    md.baro.rec_press.resize(3 * n_rec * F);
    for (size_t j = 0; j < n_rec * F; ++j) {
      md.baro.rec_volume[j] = rec[4 * j];
      for (int c = 0; c < 3; ++c) md.baro.rec_press[3 * j + c] = rec[4 * j + 1 + c];
    }
    resident_final_cells(h, "ta_md_run", want, rebuilds, n_rebuilds);
    if (h->relax.cell.on && h->relax.valid &&
        std::memcmp(cells_at_entry.data(), h->ref_cells.data(), 9 * F * sizeof(double)) != 0) {
      // the barostat's cells replace the relaxed ones: they are h0 from here on, G = I, the cell velocities 0
      HIP_CHECK(hipMemcpy(h->relax.cell.h0.ptr, h->ref_cells.data(), 9 * F * sizeof(double), hipMemcpyHostToDevice));
      h->relax.cell.reset_deformation(F);
    }
    md.baro.rec_valid = true;
  }
  if (md.nhc.on) {
    md.nhc.rec_host.resize(n_rec * F);
    if (F) HIP_CHECK(hipMemcpy(md.nhc.rec_host.data(), md.nhc.rec.ptr, n_rec * F * sizeof(double), hipMemcpyDeviceToHost));
    md.nhc.rec_valid = true;
  }
  if (md.mtk.on) {
    md.mtk.rec_host.resize(n_rec * F);
    if (F) HIP_CHECK(hipMemcpy(md.mtk.rec_host.data(), md.mtk.rec.ptr, n_rec * F * sizeof(double), hipMemcpyDeviceToHost));
    md.mtk.rec_valid = true;
  }
  if (epot && F) HIP_CHECK(hipMemcpy(epot, md.epot.ptr, n_rec * F * sizeof(double), hipMemcpyDeviceToHost));
  if (ekin && F) {
    std::vector<double> part(n_rec * n_blk);
    HIP_CHECK(hipMemcpy(part.data(), md.ke.ptr, part.size() * sizeof(double), hipMemcpyDeviceToHost));
    const std::vector<int32_t> &start = h->res.blk_start_host;
    for (size_t r = 0; r < n_rec; ++r)
      for (size_t f = 0; f < F; ++f) {
        double t = 0.0;
        for (int32_t b = start[f]; b < start[f + 1]; ++b) t += part[r * n_blk + (size_t)b];
        ekin[r * F + f] = t;
      }
  }
}

// what the getters of a ring ask of the window [first_lag, first_lag + n) of the `held` newest `rows` ("snapshots",
// "rows"); returns 0 or the error code
int md_ring_window(ta_context *h, const std::string &who, int32_t first_lag, int32_t n, int64_t held, const char *rows) {
  if (first_lag < 0) return fail(h, TA_ERR_INVALID, who + ": first_lag must be >= 0");
  if (n < 0) return fail(h, TA_ERR_INVALID, who + ": n must be >= 0");
  if ((int64_t)first_lag + n > held)
    return fail(h, TA_ERR_INVALID, who + ": first_lag + n = " + std::to_string((int64_t)first_lag + n) + " exceeds the " +
                                   std::to_string(held) + " " + rows + " held (min(n_samples, n_lags))");
  return TA_OK;
}

// the four words every sampler's getter begins its info with: samples taken, `size` (the feature's), sample_every, the
// step of the newest sample
void fill_info(int64_t *info, const MdSampler &x, int64_t size) {
  info[0] = x.sched.taken();
  info[1] = size;
  info[2] = x.sched.every;
  info[3] = x.sched.last;
}

// The held rows of the series ring of sampler x (clusters, CNA) for F frames, oldest first, to `series` and their steps
// to `steps` (either may be null). Returns the rows held.
template <typename S>
int64_t copy_series(const S &x, size_t F, int64_t *series, int64_t *steps) {
  static_assert(sizeof(*x.series.ptr) == sizeof(int64_t), "the rows are copied as they are");
  const size_t row = x.set.row(F);
  const int64_t taken = x.sched.taken(), held = std::min<int64_t>(taken, x.set.p.n_series);
  for (int64_t j = 0; j < held; ++j) {
    const int64_t idx = taken - held + j;  // sample number
    if (series && row)
      HIP_CHECK(hipMemcpy(series + (size_t)j * row, x.series_row(idx, F), row * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (steps) steps[j] = x.sched.step(idx);
  }
  return held;
}

}  // namespace

extern "C" {

int ta_md_init(ta_handle h, const double *masses, const double *velocities) {
  if (!h || !masses) return fail(h, TA_ERR_INVALID, "ta_md_init: null argument");
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "ta_md_init: no resident batch");
  const size_t N = h->keep_species.size();
  for (size_t i = 0; i < N; ++i)
    if (!(masses[i] > 0.0) || !std::isfinite(masses[i]))
      return fail(h, TA_ERR_INVALID, "ta_md_init: mass of atom " + std::to_string(i) + " is not a finite number > 0");
  if (velocities)
    for (size_t i = 0; i < 3 * N; ++i)
      if (!std::isfinite(velocities[i])) return fail(h, TA_ERR_INVALID, "ta_md_init: non-finite velocity");
  const ta::MdSamplerText *nomem = nullptr;  // of the first sampler, in their canonical order, that found no room
  // (a batch the wave vectors are not defined for: the feature goes off, as when there is no room for it)
  const bool sq_unfit = h->md.sq.on && md_sq_frames(h) != TA_OK;
  const std::string sq_why = sq_unfit ? h->err : std::string();
  const int rc = guarded(h, [&]() {
    auto &md = h->md;
    md.valid = false;
    HIP_CHECK(hipStreamSynchronize(h->stream));
    h->upload_pending = false;
    md.mass.ensure(N + 1);
    md.vel.ensure(3 * N + 1);
    h->res.ref.ensure(3 * N + 1);
    h->res.status.ensure(2);
    h->res.status_host.ensure(64);
    const size_t n_chain = h->keep_natoms.size() * ta::kMdMaxChain;  // every frame's chain starts at rest
    md.nhc.eta.ensure(n_chain + 1);
    md.nhc.veta.ensure(n_chain + 1);
    HIP_CHECK(hipMemset(md.nhc.eta.ptr, 0, (n_chain + 1) * sizeof(double)));
    HIP_CHECK(hipMemset(md.nhc.veta.ptr, 0, (n_chain + 1) * sizeof(double)));
    md.nhc.rec_valid = false;
    md.mtk.omega.ensure(3 * h->keep_natoms.size() + 1);  // every frame's barostat starts at rest as well
    md.mtk.xi.ensure(n_chain + 1);
    md.mtk.vxi.ensure(n_chain + 1);
    HIP_CHECK(hipMemset(md.mtk.omega.ptr, 0, (3 * h->keep_natoms.size() + 1) * sizeof(double)));
    HIP_CHECK(hipMemset(md.mtk.xi.ptr, 0, (n_chain + 1) * sizeof(double)));
    HIP_CHECK(hipMemset(md.mtk.vxi.ptr, 0, (n_chain + 1) * sizeof(double)));
    md.mtk.rec_valid = false;
    if (N) {
      HIP_CHECK(hipMemcpy(md.mass.ptr, masses, N * sizeof(double), hipMemcpyHostToDevice));
      if (velocities)
        HIP_CHECK(hipMemcpy(md.vel.ptr, velocities, 3 * N * sizeof(double), hipMemcpyHostToDevice));
      else
        HIP_CHECK(hipMemset(md.vel.ptr, 0, 3 * N * sizeof(double)));
    }
    h->res.ref_builds = -1;  // ta_md_run uploads ref_pos
    h->res.chunk = 0;
    h->res.blk_start_host.clear();
    md.step = 0;
    md.baro.rec_valid = false;
    for_each_sampler(md, [&](auto &x) {  // empty buffers for this batch from the stored setting, or none
      if (sq_unfit && static_cast<MdSampler *>(&x) == &md.sq) {
        x.on = false;
        HIP_CHECK(hipStreamSynchronize(h->stream));
        x.release();
      }
      if (x.on && !md_alloc(h, x, x.set)) {
        x.on = false;
        if (!nomem) nomem = &x.text;
      }
    });
    md.valid = true;
  });
  if (rc == TA_OK && nomem) return fail(h, TA_ERR_NOMEM, ta::md_text_init_nomem(*nomem));
  if (rc == TA_OK && sq_unfit) return fail(h, TA_ERR_INVALID, "ta_md_init: " + sq_why + "; the feature is off");
  return rc;
}

int ta_md_set_thermostat(ta_handle h, double kT0, double tau) {
  if (!h) return TA_ERR_INVALID;
  if (std::isnan(kT0) || std::isinf(kT0)) return fail(h, TA_ERR_INVALID, "ta_md_set_thermostat: kT0 must be finite");
  if (kT0 > 0.0 && (!(tau > 0.0) || !std::isfinite(tau)))
    return fail(h, TA_ERR_INVALID, "ta_md_set_thermostat: tau must be a finite time > 0");
  if (kT0 > 0.0 && h->md.langevin.friction > 0.0)
    return fail(h, TA_ERR_INVALID, "ta_md_set_thermostat: the Langevin thermostat is on; switch it off "
                                   "(ta_md_set_langevin with friction 0) before the Berendsen thermostat goes on");
  if (kT0 > 0.0 && h->md.nhc.on)
    return fail(h, TA_ERR_INVALID, "ta_md_set_thermostat: the Nose-Hoover chain thermostat is on; switch it off "
                                   "(ta_md_set_nose_hoover with NULL) before the Berendsen thermostat goes on");
  h->md.berendsen.kT0 = kT0 > 0.0 ? kT0 : 0.0;
  h->md.berendsen.tau = kT0 > 0.0 ? tau : 0.0;
  return TA_OK;
}

int ta_md_set_langevin(ta_handle h, double kT0, double friction, uint64_t seed) {
  if (!h) return TA_ERR_INVALID;
  if (!(friction >= 0.0) || !std::isfinite(friction))
    return fail(h, TA_ERR_INVALID, "ta_md_set_langevin: friction must be a finite rate >= 0");
  if (!(kT0 >= 0.0) || !std::isfinite(kT0))
    return fail(h, TA_ERR_INVALID, "ta_md_set_langevin: kT0 must be finite and >= 0");
  if (friction > 0.0 && h->md.berendsen.kT0 > 0.0)
    return fail(h, TA_ERR_INVALID, "ta_md_set_langevin: the Berendsen thermostat is on; switch it off "
                                   "(ta_md_set_thermostat with kT0 0) before the Langevin thermostat goes on");
  if (friction > 0.0 && h->md.nhc.on)
    return fail(h, TA_ERR_INVALID, "ta_md_set_langevin: the Nose-Hoover chain thermostat is on; switch it off "
                                   "(ta_md_set_nose_hoover with NULL) before the Langevin thermostat goes on");
  h->md.langevin.friction = friction;
  h->md.langevin.kT0 = friction > 0.0 ? kT0 : 0.0;
  h->md.langevin.seed = seed;
  return TA_OK;
}

int ta_md_set_nose_hoover(ta_handle h, const ta_md_nhc_params *p) {
  if (!h) return TA_ERR_INVALID;
  if (p && std::isnan(p->kT0)) return fail(h, TA_ERR_INVALID, "ta_md_set_nose_hoover: kT0 must be finite");
  auto &nhc = h->md.nhc;
  if (!p || !(p->kT0 > 0.0)) {
    nhc.on = false;
    return TA_OK;
  }
  if (!std::isfinite(p->kT0)) return fail(h, TA_ERR_INVALID, "ta_md_set_nose_hoover: kT0 must be finite");
  if (!(p->tau > 0.0) || !std::isfinite(p->tau))
    return fail(h, TA_ERR_INVALID, "ta_md_set_nose_hoover: tau must be a finite time > 0");
  if (p->chain < 1 || p->chain > TA_MD_MAX_CHAIN)
    return fail(h, TA_ERR_INVALID, "ta_md_set_nose_hoover: chain must be 1 .. " + std::to_string(TA_MD_MAX_CHAIN));
  if (p->loops < 1 || p->loops > 16) return fail(h, TA_ERR_INVALID, "ta_md_set_nose_hoover: loops must be 1 .. 16");
  if (p->dof_removed < 0) return fail(h, TA_ERR_INVALID, "ta_md_set_nose_hoover: dof_removed must be >= 0");
  if (h->md.berendsen.kT0 > 0.0)
    return fail(h, TA_ERR_INVALID, "ta_md_set_nose_hoover: the Berendsen thermostat is on; switch it off "
                                   "(ta_md_set_thermostat with kT0 0) before the Nose-Hoover chain goes on");
  if (h->md.langevin.friction > 0.0)
    return fail(h, TA_ERR_INVALID, "ta_md_set_nose_hoover: the Langevin thermostat is on; switch it off "
                                   "(ta_md_set_langevin with friction 0) before the Nose-Hoover chain goes on");
  if (nhc.on && nhc.p.chain != p->chain && h->md.valid) {
    // another chain length: the slots beyond the old one hold nothing, the chain starts again at rest
    const size_t n_chain = h->keep_natoms.size() * ta::kMdMaxChain;
    const int rc = guarded(h, [&]() {
      HIP_CHECK(hipStreamSynchronize(h->stream));
      HIP_CHECK(hipMemset(nhc.eta.ptr, 0, (n_chain + 1) * sizeof(double)));
      HIP_CHECK(hipMemset(nhc.veta.ptr, 0, (n_chain + 1) * sizeof(double)));
    });
    if (rc != TA_OK) return rc;
  }
  nhc.p = *p;
  nhc.on = true;
  return TA_OK;
}

int ta_md_get_chain(ta_handle h, double *eta, double *veta) {
  if (!h) return TA_ERR_INVALID;
  if (const int rc = md_chain_ready(h, "ta_md_get_chain")) return rc;
  return guarded(h, [&]() {
    const size_t F = h->keep_natoms.size(), M = (size_t)h->md.nhc.p.chain;
    HIP_CHECK(hipStreamSynchronize(h->stream));
    std::vector<double> buf(F * ta::kMdMaxChain);
    for (int w = 0; w < 2; ++w) {
      double *out = w ? veta : eta;
      if (!out || !F) continue;
      HIP_CHECK(hipMemcpy(buf.data(), w ? h->md.nhc.veta.ptr : h->md.nhc.eta.ptr, buf.size() * sizeof(double),
                          hipMemcpyDeviceToHost));
      for (size_t f = 0; f < F; ++f)
        for (size_t k = 0; k < M; ++k) out[f * M + k] = buf[f * ta::kMdMaxChain + k];
    }
  });
}

int ta_md_set_chain(ta_handle h, const double *eta, const double *veta) {
  if (!h) return TA_ERR_INVALID;
  if (const int rc = md_chain_ready(h, "ta_md_set_chain")) return rc;
  const size_t F = h->keep_natoms.size(), M = (size_t)h->md.nhc.p.chain;
  for (size_t j = 0; j < F * M; ++j) {
    if (eta && !std::isfinite(eta[j])) return fail(h, TA_ERR_INVALID, "ta_md_set_chain: non-finite eta");
    if (veta && !std::isfinite(veta[j])) return fail(h, TA_ERR_INVALID, "ta_md_set_chain: non-finite veta");
  }
  return guarded(h, [&]() {
    HIP_CHECK(hipStreamSynchronize(h->stream));
    std::vector<double> buf(F * ta::kMdMaxChain + 1);
    for (int w = 0; w < 2; ++w) {
      const double *in = w ? veta : eta;
      std::fill(buf.begin(), buf.end(), 0.0);
      if (in)
        for (size_t f = 0; f < F; ++f)
          for (size_t k = 0; k < M; ++k) buf[f * ta::kMdMaxChain + k] = in[f * M + k];
      HIP_CHECK(hipMemcpy(w ? h->md.nhc.veta.ptr : h->md.nhc.eta.ptr, buf.data(), buf.size() * sizeof(double),
                          hipMemcpyHostToDevice));
    }
  });
}

int ta_md_get_chain_records(ta_handle h, double *e_chain) {
  if (!h) return TA_ERR_INVALID;
  if (const int rc = md_resident(h, "ta_md_get_chain_records")) return rc;
  if (!h->md.nhc.rec_valid)
    return fail(h, TA_ERR_INVALID, "ta_md_get_chain_records: the last ta_md_run of this batch had no Nose-Hoover chain");
  const std::vector<double> &rec = h->md.nhc.rec_host;
  if (e_chain && !rec.empty()) std::memcpy(e_chain, rec.data(), rec.size() * sizeof(double));
  return TA_OK;
}

int ta_md_set_sampling(ta_handle h, const ta_md_sampling_params *p) {
  if (!h) return TA_ERR_INVALID;
  if (!p || p->n_lags == 0) return md_sampler_off(h, h->md.corr);
  if (p->n_lags < 0 || p->n_lags > TA_MD_MAX_LAGS)
    return fail(h, TA_ERR_INVALID, "ta_md_set_sampling: n_lags must be 0 .. " + std::to_string(TA_MD_MAX_LAGS));
  if (p->sample_every < 1) return fail(h, TA_ERR_INVALID, "ta_md_set_sampling: sample_every must be >= 1");
  return md_sampler_set(h, h->md.corr, {*p}, "rings of n_lags = " + std::to_string(p->n_lags) + " snapshots");
}

int ta_md_get_correlations(ta_handle h, double *vacf_sum, double *msd_sum, int64_t *info) {
  if (!h) return TA_ERR_INVALID;
  if (const int rc = md_sampler_ready(h, h->md.corr, "ta_md_get_correlations")) return rc;
  return guarded(h, [&]() {
    const auto &corr = h->md.corr;
    const size_t F = h->keep_natoms.size(), E = (size_t)h->n_elements, n = corr.set.n_sums(F, E);
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (vacf_sum && n) HIP_CHECK(hipMemcpy(vacf_sum, corr.acc_v(), n * sizeof(double), hipMemcpyDeviceToHost));
    if (msd_sum && n) HIP_CHECK(hipMemcpy(msd_sum, corr.acc_x(F, E), n * sizeof(double), hipMemcpyDeviceToHost));
    if (info) fill_info(info, corr, corr.set.p.n_lags);
  });
}

int ta_md_get_samples(ta_handle h, int32_t first_lag, int32_t n, double *positions, double *velocities,
                      int64_t *steps) {
  if (!h) return TA_ERR_INVALID;
  if (const int rc = md_sampler_ready(h, h->md.corr, "ta_md_get_samples")) return rc;
  const auto &corr = h->md.corr;
  const int64_t taken = corr.sched.taken(), L = corr.set.p.n_lags, held = std::min(taken, L);
  if (const int bad = md_ring_window(h, "ta_md_get_samples", first_lag, n, held, "snapshots")) return bad;
  return guarded(h, [&]() {
    const size_t N = h->keep_species.size(), row = 3 * N;
    HIP_CHECK(hipStreamSynchronize(h->stream));
    for (int32_t j = 0; j < n; ++j) {
      const int64_t idx = taken - 1 - first_lag - j;  // sample number
      if (positions && row)
        HIP_CHECK(hipMemcpy(positions + (size_t)j * row, corr.slot(corr.ring_x, idx, N), row * sizeof(double), hipMemcpyDeviceToHost));
      if (velocities && row)
        HIP_CHECK(hipMemcpy(velocities + (size_t)j * row, corr.slot(corr.ring_v, idx, N), row * sizeof(double), hipMemcpyDeviceToHost));
      if (steps) steps[j] = corr.sched.step(idx);
    }
  });
}

int ta_md_set_rdf(ta_handle h, const ta_md_rdf_params *p) {
  if (!h) return TA_ERR_INVALID;
  if (!p || p->n_bins == 0) return md_sampler_off(h, h->md.rdf);
  if (p->n_bins < 0 || p->n_bins > TA_MD_MAX_BINS)
    return fail(h, TA_ERR_INVALID, "ta_md_set_rdf: n_bins must be 0 .. " + std::to_string(TA_MD_MAX_BINS));
  if (p->sample_every < 1) return fail(h, TA_ERR_INVALID, "ta_md_set_rdf: sample_every must be >= 1");
  if (!std::isfinite(p->r_max) || !(p->r_max > 0.0))
    return fail(h, TA_ERR_INVALID, "ta_md_set_rdf: r_max must be a finite distance > 0");
  if (p->r_max > h->rmax)
    return fail(h, TA_ERR_INVALID, "ta_md_set_rdf: r_max = " + std::to_string(p->r_max) + " exceeds the model's cutoff max(rcut, acut) = " +
                                   std::to_string(h->rmax) + "; the neighbour list is not complete beyond that");
  return md_sampler_set(h, h->md.rdf, {*p}, "counts of n_bins = " + std::to_string(p->n_bins));
}

int ta_md_get_rdf(ta_handle h, int64_t *counts, int64_t *info, double *r_max) {
  if (!h) return TA_ERR_INVALID;
  const auto &rdf = h->md.rdf;
  if (const int rc = md_sampler_ready(h, rdf, "ta_md_get_rdf")) return rc;
  return guarded(h, [&]() {
    const size_t E = (size_t)h->n_elements, n = h->keep_natoms.size() * E * E * (size_t)rdf.set.p.n_bins;
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (counts && n) HIP_CHECK(hipMemcpy(counts, rdf.acc.ptr, n * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (info) fill_info(info, rdf, rdf.set.p.n_bins);
    if (r_max) *r_max = rdf.set.p.r_max;
  });
}

int ta_md_set_adf(ta_handle h, const ta_md_adf_params *p, const double *r_bond_pairs) {
  if (!h) return TA_ERR_INVALID;
  if (!p || p->n_bins == 0) return md_sampler_off(h, h->md.adf);
  if (p->n_bins < 0 || p->n_bins > TA_MD_MAX_BINS)
    return fail(h, TA_ERR_INVALID, "ta_md_set_adf: n_bins must be 0 .. " + std::to_string(TA_MD_MAX_BINS));
  if (p->sample_every < 1) return fail(h, TA_ERR_INVALID, "ta_md_set_adf: sample_every must be >= 1");
  std::vector<double> rb;
  if (const int bad = md_bond_cutoffs(h, "ta_md_set_adf", p->r_bond, r_bond_pairs, rb)) return bad;
  return md_sampler_set(h, h->md.adf, {*p, rb}, "counts of n_bins = " + std::to_string(p->n_bins));
}

int ta_md_get_adf(ta_handle h, int64_t *counts, int64_t *info, double *r_bond_pairs) {
  if (!h) return TA_ERR_INVALID;
  const auto &adf = h->md.adf;
  if (const int rc = md_sampler_ready(h, adf, "ta_md_get_adf")) return rc;
  return guarded(h, [&]() {
    const size_t E = (size_t)h->n_elements;
    const size_t n = h->keep_natoms.size() * E * (E * (E + 1) / 2) * (size_t)adf.set.p.n_bins;
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (counts && n) HIP_CHECK(hipMemcpy(counts, adf.acc.ptr, n * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (info) fill_info(info, adf, adf.set.p.n_bins);
    if (r_bond_pairs) std::memcpy(r_bond_pairs, adf.set.rb.data(), E * E * sizeof(double));
  });
}

int ta_md_set_order(ta_handle h, const ta_md_order_params *p, const double *r_bond_pairs) {
  if (!h) return TA_ERR_INVALID;
  if (!p || p->n_bins == 0) return md_sampler_off(h, h->md.order);
  if (p->n_bins < 0 || p->n_bins > TA_MD_MAX_BINS)
    return fail(h, TA_ERR_INVALID, "ta_md_set_order: n_bins must be 0 .. " + std::to_string(TA_MD_MAX_BINS));
  if (p->sample_every < 1) return fail(h, TA_ERR_INVALID, "ta_md_set_order: sample_every must be >= 1");
  if (p->n_degrees < 1 || p->n_degrees > TA_MD_ORDER_MAX_DEGREES)
    return fail(h, TA_ERR_INVALID, "ta_md_set_order: n_degrees must be 1 .. " + std::to_string(TA_MD_ORDER_MAX_DEGREES));
  bool solid_found = false;
  for (int d = 0; d < p->n_degrees; ++d) {
    if (p->degrees[d] < 1 || p->degrees[d] > TA_MD_ORDER_MAX_L)
      return fail(h, TA_ERR_INVALID, "ta_md_set_order: degrees[" + std::to_string(d) + "] = " + std::to_string(p->degrees[d]) +
                                     " must be 1 .. " + std::to_string(TA_MD_ORDER_MAX_L));
    for (int e = 0; e < d; ++e)
      if (p->degrees[e] == p->degrees[d])
        return fail(h, TA_ERR_INVALID, "ta_md_set_order: degrees[" + std::to_string(d) + "] = " + std::to_string(p->degrees[d]) +
                                       " is given twice");
    solid_found = solid_found || p->degrees[d] == p->solid_degree;
  }
  if (!solid_found)
    return fail(h, TA_ERR_INVALID, "ta_md_set_order: solid_degree = " + std::to_string(p->solid_degree) + " is not among the degrees");
  if (!std::isfinite(p->solid_threshold) || !(p->solid_threshold > -1.0 && p->solid_threshold < 1.0))
    return fail(h, TA_ERR_INVALID, "ta_md_set_order: solid_threshold must be a finite number inside (-1, 1)");
  std::vector<double> rb;
  if (const int bad = md_bond_cutoffs(h, "ta_md_set_order", p->r_bond, r_bond_pairs, rb)) return bad;
  ta_md_order_params clean = *p;
  for (int d = p->n_degrees; d < TA_MD_ORDER_MAX_DEGREES; ++d) clean.degrees[d] = 0;
  return md_sampler_set(h, h->md.order, {clean, rb}, "buffers of n_bins = " + std::to_string(p->n_bins));
}

int ta_md_get_order(ta_handle h, int64_t *hist_q, int64_t *hist_qbar, int64_t *hist_conn, int64_t *info,
                    double *r_bond_pairs) {
  if (!h) return TA_ERR_INVALID;
  if (const int bad = md_sampler_ready(h, h->md.order, "ta_md_get_order")) return bad;
  const auto &order = h->md.order;
  return guarded(h, [&]() {
    const size_t E = (size_t)h->n_elements, F = h->keep_natoms.size();
    const size_t n_hist = order.set.n_hist(F, E), n_conn = order.set.n_hist_conn(F, E);
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (hist_q && n_hist) HIP_CHECK(hipMemcpy(hist_q, order.hist_q(), n_hist * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (hist_qbar && n_hist)
      HIP_CHECK(hipMemcpy(hist_qbar, order.hist_qbar(F, E), n_hist * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (hist_conn && n_conn)
      HIP_CHECK(hipMemcpy(hist_conn, order.hist_conn(F, E), n_conn * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (info) fill_info(info, order, order.set.p.n_bins);
    if (r_bond_pairs) std::memcpy(r_bond_pairs, order.set.rb.data(), E * E * sizeof(double));
  });
}

int ta_md_get_order_atoms(ta_handle h, double *q, double *qbar, int32_t *n_bonds, int32_t *n_conn, double *qlm) {
  if (!h) return TA_ERR_INVALID;
  if (const int bad = md_sampler_ready(h, h->md.order, "ta_md_get_order_atoms")) return bad;
  const auto &order = h->md.order;
  if (order.sched.last < 0) return fail(h, TA_ERR_INVALID, "ta_md_get_order_atoms: no sample has been taken yet");
  return guarded(h, [&]() {
    const size_t N = h->keep_species.size(), n_q = order.set.n_q(N), M = (size_t)order.n_lm;
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (!N) return;
    if (q) HIP_CHECK(hipMemcpy(q, order.q(), n_q * sizeof(double), hipMemcpyDeviceToHost));
    if (qbar) HIP_CHECK(hipMemcpy(qbar, order.qbar(N), n_q * sizeof(double), hipMemcpyDeviceToHost));
    if (n_bonds) HIP_CHECK(hipMemcpy(n_bonds, order.n_bonds(), N * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (n_conn) HIP_CHECK(hipMemcpy(n_conn, order.n_conn(N), N * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (qlm) HIP_CHECK(hipMemcpy(qlm, order.qlm.ptr, N * 2 * M * sizeof(double), hipMemcpyDeviceToHost));
  });
}

int ta_md_set_clusters(ta_handle h, const ta_md_cluster_params *p, const double *r_link_pairs) {
  if (!h) return TA_ERR_INVALID;
  if (!p || p->n_bins == 0) return md_sampler_off(h, h->md.cluster);
  if (p->n_bins < 0 || p->n_bins > TA_MD_MAX_BINS)
    return fail(h, TA_ERR_INVALID, "ta_md_set_clusters: n_bins must be 0 .. " + std::to_string(TA_MD_MAX_BINS));
  if (p->n_series < 1 || p->n_series > TA_MD_CLUSTER_MAX_SERIES)
    return fail(h, TA_ERR_INVALID, "ta_md_set_clusters: n_series must be 1 .. " + std::to_string(TA_MD_CLUSTER_MAX_SERIES));
  if (p->sample_every < 1) return fail(h, TA_ERR_INVALID, "ta_md_set_clusters: sample_every must be >= 1");
  if (p->n_min < 0 || p->n_min > TA_MD_ORDER_MAX_CONN)
    return fail(h, TA_ERR_INVALID, "ta_md_set_clusters: n_min must be 0 .. " + std::to_string(TA_MD_ORDER_MAX_CONN));
  if (p->species_mask == 0) return fail(h, TA_ERR_INVALID, "ta_md_set_clusters: species_mask selects no element");
  if (p->species_mask < 0 || (h->n_elements < 31 && (p->species_mask >> h->n_elements) != 0))
    return fail(h, TA_ERR_INVALID, "ta_md_set_clusters: species_mask = " + std::to_string(p->species_mask) +
                                   " has a bit at or above n_elements = " + std::to_string(h->n_elements));
  std::vector<double> rl;
  const double r_link = !r_link_pairs && std::isnan(p->r_link) ? h->rmax : p->r_link;  // NaN: the model's cutoff
  if (const int bad = md_bond_cutoffs(h, "ta_md_set_clusters", r_link, r_link_pairs, rl, "r_link", "r_link_pairs")) return bad;
  ta_md_cluster_params clean = *p;
  clean.r_link = r_link;
  return md_sampler_set(h, h->md.cluster, {clean, rl}, "buffers of n_bins = " + std::to_string(p->n_bins) + " and n_series = " +
                                                     std::to_string(p->n_series));
}

int ta_md_get_clusters(ta_handle h, int64_t *hist, int64_t *series, int64_t *steps, int64_t *info, double *r_link_pairs) {
  if (!h) return TA_ERR_INVALID;
  if (const int bad = md_sampler_ready(h, h->md.cluster, "ta_md_get_clusters")) return bad;
  const auto &cluster = h->md.cluster;
  return guarded(h, [&]() {
    const size_t E = (size_t)h->n_elements, F = h->keep_natoms.size(), n_hist = cluster.set.n_hist(F);
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (hist && n_hist) HIP_CHECK(hipMemcpy(hist, cluster.acc.ptr, n_hist * sizeof(int64_t), hipMemcpyDeviceToHost));
    const int64_t held = copy_series(cluster, F, series, steps);
    if (info) {
      fill_info(info, cluster, cluster.set.p.n_bins);
      info[4] = held;
      info[5] = cluster.set.p.n_series;
    }
    if (r_link_pairs) std::memcpy(r_link_pairs, cluster.set.rl.data(), E * E * sizeof(double));
  });
}

int ta_md_get_cluster_atoms(ta_handle h, int32_t *label, int32_t *size) {
  if (!h) return TA_ERR_INVALID;
  if (const int bad = md_sampler_ready(h, h->md.cluster, "ta_md_get_cluster_atoms")) return bad;
  const auto &cluster = h->md.cluster;
  if (cluster.sched.last < 0) return fail(h, TA_ERR_INVALID, "ta_md_get_cluster_atoms: no sample has been taken yet");
  return guarded(h, [&]() {
    const size_t N = h->keep_species.size();
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (!N) return;
    if (label) HIP_CHECK(hipMemcpy(label, cluster.label(N), N * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (size) HIP_CHECK(hipMemcpy(size, cluster.size(N), N * sizeof(int32_t), hipMemcpyDeviceToHost));
  });
}

int ta_md_set_cna(ta_handle h, const ta_md_cna_params *p) {
  if (!h) return TA_ERR_INVALID;
  if (!p || p->n_series == 0) return md_sampler_off(h, h->md.cna);
  if (p->mode != TA_MD_CNA_ADAPTIVE && p->mode != TA_MD_CNA_FIXED)
    return fail(h, TA_ERR_INVALID, "ta_md_set_cna: mode = " + std::to_string(p->mode) + " must be TA_MD_CNA_ADAPTIVE (0) or "
                                   "TA_MD_CNA_FIXED (1)");
  if (p->n_series < 0 || p->n_series > TA_MD_CLUSTER_MAX_SERIES)
    return fail(h, TA_ERR_INVALID, "ta_md_set_cna: n_series must be 0 .. " + std::to_string(TA_MD_CLUSTER_MAX_SERIES));
  if (p->sample_every < 1) return fail(h, TA_ERR_INVALID, "ta_md_set_cna: sample_every must be >= 1");
  const bool fixed = p->mode == TA_MD_CNA_FIXED;
  const char *name = fixed ? "r_cut" : "r_max";
  const double r = fixed ? p->r_cut : std::isnan(p->r_max) ? h->rmax : p->r_max;  // r_max = NaN: the model's cutoff
  if (!std::isfinite(r) || !(r > 0.0))
    return fail(h, TA_ERR_INVALID, std::string("ta_md_set_cna: ") + name + " must be a finite distance > 0");
  if (r > h->rmax)
    return fail(h, TA_ERR_INVALID, std::string("ta_md_set_cna: ") + name + " = " + std::to_string(r) +
                                   " exceeds the model's cutoff max(rcut, acut) = " + std::to_string(h->rmax) +
                                   "; the neighbour list is not complete beyond that");
  ta_md_cna_params clean = *p;
  if (fixed) clean.r_max = 0.0; else clean.r_max = r, clean.r_cut = 0.0;
  return md_sampler_set(h, h->md.cna, {clean}, "buffers of n_series = " + std::to_string(p->n_series));
}

int ta_md_get_cna(ta_handle h, int64_t *counts, int64_t *series, int64_t *steps, int64_t *info) {
  if (!h) return TA_ERR_INVALID;
  if (const int bad = md_sampler_ready(h, h->md.cna, "ta_md_get_cna")) return bad;
  const auto &cna = h->md.cna;
  return guarded(h, [&]() {
    const size_t E = (size_t)h->n_elements, F = h->keep_natoms.size(), n_acc = cna.set.n_acc(F, E);
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (counts && n_acc) HIP_CHECK(hipMemcpy(counts, cna.acc.ptr, n_acc * sizeof(int64_t), hipMemcpyDeviceToHost));
    const int64_t held = copy_series(cna, F, series, steps);
    if (info) {
      fill_info(info, cna, cna.set.p.mode);
      info[4] = held;
      info[5] = cna.set.p.n_series;
    }
  });
}

int ta_md_get_cna_atoms(ta_handle h, int32_t *structure, double *r_local) {
  if (!h) return TA_ERR_INVALID;
  if (const int bad = md_sampler_ready(h, h->md.cna, "ta_md_get_cna_atoms")) return bad;
  const auto &cna = h->md.cna;
  if (cna.sched.last < 0) return fail(h, TA_ERR_INVALID, "ta_md_get_cna_atoms: no sample has been taken yet");
  return guarded(h, [&]() {
    const size_t N = h->keep_species.size();
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (!N) return;
    if (structure) HIP_CHECK(hipMemcpy(structure, cna.structure.ptr, N * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (r_local) HIP_CHECK(hipMemcpy(r_local, cna.r_local.ptr, N * sizeof(double), hipMemcpyDeviceToHost));
  });
}

int ta_md_set_sq(ta_handle h, const ta_md_sq_params *p, const int32_t *miller) {
  if (!h) return TA_ERR_INVALID;
  if (!p || p->n_q == 0) return md_sampler_off(h, h->md.sq);
  if (p->n_q < 0 || p->n_q > TA_MD_SQ_MAX_Q)
    return fail(h, TA_ERR_INVALID, "ta_md_set_sq: n_q must be 0 .. " + std::to_string(TA_MD_SQ_MAX_Q));
  if (p->n_lags < 1 || p->n_lags > TA_MD_MAX_LAGS)
    return fail(h, TA_ERR_INVALID, "ta_md_set_sq: n_lags must be 1 .. " + std::to_string(TA_MD_MAX_LAGS));
  if (p->sample_every < 1) return fail(h, TA_ERR_INVALID, "ta_md_set_sq: sample_every must be >= 1");
  if (p->currents != 0 && p->currents != 1) return fail(h, TA_ERR_INVALID, "ta_md_set_sq: currents must be 0 or 1");
  if (!miller) return fail(h, TA_ERR_INVALID, "ta_md_set_sq: miller is NULL");
  for (int j = 0; j < 3 * p->n_q; ++j)
    if (miller[j] < -TA_MD_SQ_MAX_INDEX || miller[j] > TA_MD_SQ_MAX_INDEX)
      return fail(h, TA_ERR_INVALID, "ta_md_set_sq: miller[" + std::to_string(j / 3) + "][" + std::to_string(j % 3) + "] = " +
                                     std::to_string(miller[j]) + " must be within +-" + std::to_string(TA_MD_SQ_MAX_INDEX));
  const std::vector<int32_t> triples(miller, miller + 3 * (size_t)p->n_q);
  return md_sampler_set(h, h->md.sq, {*p, triples}, "n_q = " + std::to_string(p->n_q) + " vectors at n_lags = " + std::to_string(p->n_lags),
                        md_sq_frames);
}

int ta_md_get_sq(ta_handle h, double *a_rho, double *a_l, double *a_j, int64_t *info, int32_t *miller) {
  if (!h) return TA_ERR_INVALID;
  if (const int bad = md_sampler_ready(h, h->md.sq, "ta_md_get_sq")) return bad;
  const auto &sq = h->md.sq;
  if ((a_l || a_j) && !sq.set.p.currents)
    return fail(h, TA_ERR_INVALID, "ta_md_get_sq: a_l and a_j need the currents (ta_md_sq_params.currents = 1)");
  return guarded(h, [&]() {
    const size_t F = h->keep_natoms.size(), E = (size_t)h->n_elements, n = sq.set.n_sums(F, E);
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (a_rho && n) HIP_CHECK(hipMemcpy(a_rho, sq.acc_rho(), n * sizeof(double), hipMemcpyDeviceToHost));
    if (a_l && n) HIP_CHECK(hipMemcpy(a_l, sq.acc_l(F, E), n * sizeof(double), hipMemcpyDeviceToHost));
    if (a_j && n) HIP_CHECK(hipMemcpy(a_j, sq.acc_j(F, E), n * sizeof(double), hipMemcpyDeviceToHost));
    if (info) {
      info[0] = sq.sched.taken();
      info[1] = sq.set.p.n_q;
      info[2] = sq.set.p.n_lags;
      info[3] = sq.set.p.sample_every;
      info[4] = sq.sched.last;
      info[5] = sq.set.p.currents;
      info[6] = sq.chunk;
      info[7] = 0;
    }
    if (miller) std::memcpy(miller, sq.set.miller.data(), sq.set.miller.size() * sizeof(int32_t));
  });
}

int ta_md_get_sq_amplitudes(ta_handle h, int32_t first_lag, int32_t n, double *rho, double *cur, int64_t *steps) {
  if (!h) return TA_ERR_INVALID;
  if (const int bad = md_sampler_ready(h, h->md.sq, "ta_md_get_sq_amplitudes")) return bad;
  const auto &sq = h->md.sq;
  const int64_t taken = sq.sched.taken(), L = sq.set.p.n_lags, held = std::min(taken, L);
  if (const int bad = md_ring_window(h, "ta_md_get_sq_amplitudes", first_lag, n, held, "rows")) return bad;
  if (cur && !sq.set.p.currents)
    return fail(h, TA_ERR_INVALID, "ta_md_get_sq_amplitudes: cur needs the currents (ta_md_sq_params.currents = 1)");
  return guarded(h, [&]() {
    const size_t F = h->keep_natoms.size(), E = (size_t)h->n_elements, FE = F * E;
    const size_t Q = (size_t)sq.set.p.n_q, P = sq.set.planes(), row = sq.set.row(F, E);
    HIP_CHECK(hipStreamSynchronize(h->stream));
    std::vector<double> buf(row);
    for (int32_t j = 0; j < n; ++j) {
      const int64_t idx = taken - 1 - first_lag - j;  // sample number
      if (steps) steps[j] = sq.sched.step(idx);
      if (!row || (!rho && !cur)) continue;
      HIP_CHECK(hipMemcpy(buf.data(), sq.ring_row(idx, F, E), row * sizeof(double), hipMemcpyDeviceToHost));
      // the device row is [f][e][plane][q]; the caller's arrays have q before the components
      for (size_t fe = 0; fe < FE; ++fe)
        for (size_t q = 0; q < Q; ++q) {
          const double *src = buf.data() + fe * P * Q + q;
          if (rho)
            for (size_t c = 0; c < 2; ++c) rho[(((size_t)j * FE + fe) * Q + q) * 2 + c] = src[c * Q];
          if (cur)
            for (size_t c = 0; c < 6; ++c) cur[(((size_t)j * FE + fe) * Q + q) * 6 + c] = src[(2 + c) * Q];
        }
    }
  });
}

int ta_md_set_flux(ta_handle h, const ta_md_flux_params *p) {
  if (!h) return TA_ERR_INVALID;
  if (!p || p->n_lags == 0) return md_sampler_off(h, h->md.flux);
  if (p->n_lags < 0 || p->n_lags > TA_MD_MAX_LAGS)
    return fail(h, TA_ERR_INVALID, "ta_md_set_flux: n_lags must be 0 .. " + std::to_string(TA_MD_MAX_LAGS));
  if (p->sample_every < 1) return fail(h, TA_ERR_INVALID, "ta_md_set_flux: sample_every must be >= 1");
  return md_sampler_set(h, h->md.flux, {*p}, "n_lags = " + std::to_string(p->n_lags) + " rows");
}

int ta_md_get_flux(ta_handle h, double *sums, double *a_heat, double *a_press, int64_t *info) {
  if (!h) return TA_ERR_INVALID;
  if (const int bad = md_sampler_ready(h, h->md.flux, "ta_md_get_flux")) return bad;
  const auto &fx = h->md.flux;
  return guarded(h, [&]() {
    const size_t F = h->keep_natoms.size();
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (sums && F) HIP_CHECK(hipMemcpy(sums, fx.sums(), fx.set.row(F) * sizeof(double), hipMemcpyDeviceToHost));
    if (a_heat && F) HIP_CHECK(hipMemcpy(a_heat, fx.acc_heat(F), fx.set.n_heat(F) * sizeof(double), hipMemcpyDeviceToHost));
    if (a_press && F) HIP_CHECK(hipMemcpy(a_press, fx.acc_press(F), fx.set.n_press(F) * sizeof(double), hipMemcpyDeviceToHost));
    if (info) {
      int64_t most = 0;
      for (size_t f = 0; f < F; ++f)
        most = std::max<int64_t>(most, std::max(1, (h->keep_natoms[f] + fx.chunk - 1) / fx.chunk));
      info[0] = fx.sched.taken();
      info[1] = fx.set.p.n_lags;
      info[2] = fx.set.p.sample_every;
      info[3] = fx.sched.last;
      info[4] = fx.sched.taken() ? fx.sched.origin : -1;
      info[5] = fx.chunk;
      info[6] = most;
      info[7] = ta::kMdFluxLanes;
    }
  });
}

int ta_md_get_flux_rows(ta_handle h, int32_t first_lag, int32_t n, double *rows, int64_t *steps) {
  if (!h) return TA_ERR_INVALID;
  if (const int bad = md_sampler_ready(h, h->md.flux, "ta_md_get_flux_rows")) return bad;
  const auto &fx = h->md.flux;
  const int64_t taken = fx.sched.taken(), L = fx.set.p.n_lags, held = std::min(taken, L);
  if (const int bad = md_ring_window(h, "ta_md_get_flux_rows", first_lag, n, held, "rows")) return bad;
  return guarded(h, [&]() {
    const size_t F = h->keep_natoms.size(), row = fx.set.row(F);
    HIP_CHECK(hipStreamSynchronize(h->stream));
    for (int32_t j = 0; j < n; ++j) {
      const int64_t idx = taken - 1 - first_lag - j;  // sample number
      if (steps) steps[j] = fx.sched.step(idx);
      if (rows && row)
        HIP_CHECK(hipMemcpy(rows + (size_t)j * row, fx.ring_row(idx, F), row * sizeof(double), hipMemcpyDeviceToHost));
    }
  });
}

int ta_md_noise(ta_handle h, int64_t step, double *xi, double *eta) {
  if (!h) return TA_ERR_INVALID;
  if (!xi || !eta) return fail(h, TA_ERR_INVALID, "ta_md_noise: null argument");
  if (const int rc = md_resident(h, "ta_md_noise")) return rc;
  if (step < 0) return fail(h, TA_ERR_INVALID, "ta_md_noise: step must be >= 0");
  return guarded(h, [&]() {
    const size_t N = h->keep_species.size();
    if (!N) return;
    auto &noise = h->md.langevin.noise;
    noise.ensure(6 * N);
    ta::launch_md_noise(h->md.langevin.seed, step, (long long)N, noise.ptr, noise.ptr + 3 * N, h->stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(h->stream));
    HIP_CHECK(hipMemcpy(xi, noise.ptr, 3 * N * sizeof(double), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(eta, noise.ptr + 3 * N, 3 * N * sizeof(double), hipMemcpyDeviceToHost));
  });
}

int ta_md_set_barostat(ta_handle h, const ta_md_barostat_params *p) {
  if (!h) return TA_ERR_INVALID;
  if (p && !std::isfinite(p->taup)) return fail(h, TA_ERR_INVALID, "ta_md_set_barostat: taup must be finite");
  if (!p || !(p->taup > 0.0)) {
    h->md.baro.on = false;
    return TA_OK;
  }
  if (!std::isfinite(p->pressure)) return fail(h, TA_ERR_INVALID, "ta_md_set_barostat: pressure must be finite");
  if (!std::isfinite(p->compressibility) || p->compressibility < 0.0)
    return fail(h, TA_ERR_INVALID, "ta_md_set_barostat: compressibility must be finite and >= 0");
  if (!p->isotropic && !p->mask[0] && !p->mask[1] && !p->mask[2])
    return fail(h, TA_ERR_INVALID, "ta_md_set_barostat: mask leaves no axis of the cell free");
  if (h->md.mtk.on)
    return fail(h, TA_ERR_INVALID, "ta_md_set_barostat: the Martyna-Tobias-Klein barostat is on; switch it off "
                                   "(ta_md_set_mtk_barostat with NULL) before the Berendsen barostat goes on");
  h->md.baro.p = *p;
  h->md.baro.on = true;
  return TA_OK;
}

int ta_md_get_cell(ta_handle h, double *cells) {
  if (!h) return TA_ERR_INVALID;
  if (!cells) return fail(h, TA_ERR_INVALID, "ta_md_get_cell: null argument");
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "ta_md_get_cell: no resident batch");
  // (between runs ref_cells is the image of the device's cells)
  const size_t F = h->keep_natoms.size();
  if (F) std::memcpy(cells, h->ref_cells.data(), 9 * F * sizeof(double));
  return TA_OK;
}

int ta_md_get_records(ta_handle h, double *volume, double *press) {
  if (!h) return TA_ERR_INVALID;
  if (const int rc = md_resident(h, "ta_md_get_records")) return rc;
  const auto &baro = h->md.baro;
  if (!baro.rec_valid)
    return fail(h, TA_ERR_INVALID, "ta_md_get_records: the last ta_md_run of this batch had no barostat");
  if (volume && !baro.rec_volume.empty())
    std::memcpy(volume, baro.rec_volume.data(), baro.rec_volume.size() * sizeof(double));
  if (press && !baro.rec_press.empty())
    std::memcpy(press, baro.rec_press.data(), baro.rec_press.size() * sizeof(double));
  return TA_OK;
}

int ta_md_set_mtk_barostat(ta_handle h, const ta_md_mtk_params *p) {
  if (!h) return TA_ERR_INVALID;
  if (p && !std::isfinite(p->tau_p)) return fail(h, TA_ERR_INVALID, "ta_md_set_mtk_barostat: tau_p must be finite");
  auto &mtk = h->md.mtk;
  if (!p || !(p->tau_p > 0.0)) {
    mtk.on = false;
    return TA_OK;
  }
  if (!std::isfinite(p->pressure)) return fail(h, TA_ERR_INVALID, "ta_md_set_mtk_barostat: pressure must be finite");
  if (p->chain < 1 || p->chain > TA_MD_MAX_CHAIN)
    return fail(h, TA_ERR_INVALID, "ta_md_set_mtk_barostat: chain must be 1 .. " + std::to_string(TA_MD_MAX_CHAIN));
  if (p->loops < 1 || p->loops > 16) return fail(h, TA_ERR_INVALID, "ta_md_set_mtk_barostat: loops must be 1 .. 16");
  if (!p->isotropic && !p->mask[0] && !p->mask[1] && !p->mask[2])
    return fail(h, TA_ERR_INVALID, "ta_md_set_mtk_barostat: mask leaves no axis of the cell free");
  if (h->md.baro.on)
    return fail(h, TA_ERR_INVALID, "ta_md_set_mtk_barostat: the Berendsen barostat is on; switch it off "
                                   "(ta_md_set_barostat with NULL) before the Martyna-Tobias-Klein barostat goes on");
  if (mtk.on && mtk.p.chain != p->chain && h->md.valid) {
    // another chain length: the slots beyond the old one hold nothing, the barostat's chain starts again at rest
    const size_t n_chain = h->keep_natoms.size() * ta::kMdMaxChain;
    const int rc = guarded(h, [&]() {
      HIP_CHECK(hipStreamSynchronize(h->stream));
      HIP_CHECK(hipMemset(mtk.xi.ptr, 0, (n_chain + 1) * sizeof(double)));
      HIP_CHECK(hipMemset(mtk.vxi.ptr, 0, (n_chain + 1) * sizeof(double)));
    });
    if (rc != TA_OK) return rc;
  }
  mtk.p = *p;
  mtk.on = true;
  return TA_OK;
}

int ta_md_get_mtk_state(ta_handle h, double *omega, double *xi, double *vxi) {
  if (!h) return TA_ERR_INVALID;
  if (const int rc = md_mtk_ready(h, "ta_md_get_mtk_state")) return rc;
  return guarded(h, [&]() {
    const size_t F = h->keep_natoms.size(), M = (size_t)h->md.mtk.p.chain;
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (omega && F) HIP_CHECK(hipMemcpy(omega, h->md.mtk.omega.ptr, 3 * F * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<double> buf(F * ta::kMdMaxChain);
    for (int w = 0; w < 2; ++w) {
      double *out = w ? vxi : xi;
      if (!out || !F) continue;
      HIP_CHECK(hipMemcpy(buf.data(), w ? h->md.mtk.vxi.ptr : h->md.mtk.xi.ptr, buf.size() * sizeof(double),
                          hipMemcpyDeviceToHost));
      for (size_t f = 0; f < F; ++f)
        for (size_t k = 0; k < M; ++k) out[f * M + k] = buf[f * ta::kMdMaxChain + k];
    }
  });
}

int ta_md_set_mtk_state(ta_handle h, const double *omega, const double *xi, const double *vxi) {
  if (!h) return TA_ERR_INVALID;
  if (const int rc = md_mtk_ready(h, "ta_md_set_mtk_state")) return rc;
  const size_t F = h->keep_natoms.size(), M = (size_t)h->md.mtk.p.chain;
  for (size_t j = 0; omega && j < 3 * F; ++j)
    if (!std::isfinite(omega[j])) return fail(h, TA_ERR_INVALID, "ta_md_set_mtk_state: non-finite omega");
  for (size_t j = 0; j < F * M; ++j) {
    if (xi && !std::isfinite(xi[j])) return fail(h, TA_ERR_INVALID, "ta_md_set_mtk_state: non-finite xi");
    if (vxi && !std::isfinite(vxi[j])) return fail(h, TA_ERR_INVALID, "ta_md_set_mtk_state: non-finite vxi");
  }
  return guarded(h, [&]() {
    HIP_CHECK(hipStreamSynchronize(h->stream));
    std::vector<double> buf(std::max<size_t>(3 * F, F * ta::kMdMaxChain) + 1, 0.0);
    if (omega) std::copy(omega, omega + 3 * F, buf.begin());
    HIP_CHECK(hipMemcpy(h->md.mtk.omega.ptr, buf.data(), (3 * F + 1) * sizeof(double), hipMemcpyHostToDevice));
    for (int w = 0; w < 2; ++w) {
      const double *in = w ? vxi : xi;
      std::fill(buf.begin(), buf.end(), 0.0);
      if (in)
        for (size_t f = 0; f < F; ++f)
          for (size_t k = 0; k < M; ++k) buf[f * ta::kMdMaxChain + k] = in[f * M + k];
      HIP_CHECK(hipMemcpy(w ? h->md.mtk.vxi.ptr : h->md.mtk.xi.ptr, buf.data(), (F * ta::kMdMaxChain + 1) * sizeof(double),
                          hipMemcpyHostToDevice));
    }
  });
}

int ta_md_get_mtk_records(ta_handle h, double *e_baro) {
  if (!h) return TA_ERR_INVALID;
  if (const int rc = md_resident(h, "ta_md_get_mtk_records")) return rc;
  if (!h->md.mtk.rec_valid)
    return fail(h, TA_ERR_INVALID, "ta_md_get_mtk_records: the last ta_md_run of this batch had no Martyna-Tobias-Klein barostat");
  const std::vector<double> &rec = h->md.mtk.rec_host;
  if (e_baro && !rec.empty()) std::memcpy(e_baro, rec.data(), rec.size() * sizeof(double));
  return TA_OK;
}

int ta_md_run(ta_handle h, int32_t n_steps, double dt, uint32_t want, int32_t record_every, double *epot,
              double *ekin, int32_t *n_rebuilds) {
  if (!h) return TA_ERR_INVALID;
  if (const int bad = md_run_refusals(h, n_steps, dt, record_every)) return bad;
  MdState &md = h->md;
  ResidentLoop &res = h->res;
  const bool baro = md.moves_cells(), nhc = md.nhc.on;
  if (n_rebuilds) *n_rebuilds = 0;
  want |= TA_WANT_ENERGY | TA_WANT_FORCES;
  want &= ~(uint32_t)TA_WANT_REUSE_DESCRIPTORS;
  if (baro) want |= TA_WANT_VIRIAL;  // the pressure
  md.baro.rec_valid = false;
  md.nhc.rec_valid = false;
  md.mtk.rec_valid = false;
  for_each_sampler(md, [&](MdSampler &x) { x.begin_run(!h->keep_species.empty()); });
  res.cell_running = md.baro.running = baro;
  const int rc = guarded(h, [&]() {
    const size_t N = h->keep_species.size(), F = h->keep_natoms.size();
    // while the heat current is sampled every evaluation of the run leaves g_p = d e_c / d D_p (put back below)
    set_centre_gradients(h, md.flux.run);
    // with Berendsen scaling one workgroup owns a whole frame: the factor needs the frame's kinetic energy
    // (the barostat: the frame's three sums of m v_c^2; the Nose-Hoover chain: the kinetic energy again)
    const bool whole_frames = md.berendsen.kT0 > 0.0 || baro || nhc;
    int chunk = ta::kMdChunk;
    if (whole_frames)
      for (size_t f = 0; f < F; ++f) chunk = std::max(chunk, h->keep_natoms[f]);
    const int threads = whole_frames ? 1024 : 256;
    md_plan_blocks(h, chunk);
    const size_t n_rec = (size_t)(n_steps / record_every) + 1;
    md.epot.ensure(n_rec * F + 1);
    md.ke.ensure(n_rec * (size_t)res.n_blk + 1);
    if (nhc) md.nhc.rec.ensure(n_rec * F + 1);
    if (md.mtk.on) md.mtk.rec.ensure(n_rec * F + 1);
    const std::vector<double> cells_at_entry(baro ? h->ref_cells : std::vector<double>());
    if (baro) {  // every run starts on a list built for the resident cells: the cumulative scale is 1
      md.baro.rec.ensure(4 * n_rec * F + 1);
      md.baro.scale.ensure(3 * F + 1);
      md.baro.ones.assign(3 * F, 1.0);
      HIP_CHECK(hipStreamSynchronize(h->stream));
      if (F) HIP_CHECK(hipMemcpy(md.baro.scale.ptr, md.baro.ones.data(), 3 * F * sizeof(double), hipMemcpyHostToDevice));
    }
    resident_begin(h);

    const int64_t step0 = md.step;  // absolute index of this run's first step
    auto integrator = md_launch(h, dt, chunk);
    const auto mtk = md_mtk_launch(h);
    auto order = md_launch(h, md.order);
    auto cluster = md_launch(h, md.cluster);
    auto cna = md_launch(h, md.cna);
    auto adf = md_launch(h, md.adf);
    auto rdf = md_launch(h, md.rdf);
    auto corr = md_launch(h, md.corr);
    auto sq = md_launch(h, md.sq);
    auto flux = md_launch(h, md.flux);
    // launch k: the samplers of the state t = step0 + k in front, the integrator, the samplers of its snapshot behind
    auto integrate = [&](int k, bool drift) {
      md_enqueue(h, md.order, order, step0, k);
      md_enqueue(h, md.cluster, cluster, step0, k);
      md_enqueue(h, md.cna, cna, step0, k);
      md_enqueue(h, md.adf, adf, step0, k);
      md_enqueue(h, md.rdf, rdf, step0, k);
      const MdSnapshot snap = md_snapshot(md.corr, md.sq, md.flux, N, step0, k);
      md_enqueue(h, integrator, mtk, threads, step0, k, drift, record_every, snap);
      md_enqueue(h, md.corr, corr, step0, k, snap);
      md_enqueue(h, md.sq, sq, step0, k, snap);
      md_enqueue(h, md.flux, flux, step0, k, snap);
    };

    h->jvp_valid = false;
    compute_impl(h, want, false, nullptr);  // F_0 and the record of the state at entry
    int rebuilds = 0;
    resident_steps(h, "ta_md_run", n_steps, want, [&](int q) { integrate(q, true); },
                   [](int, int) { return -1; }, &rebuilds, n_rebuilds);
    integrate(n_steps, false);  // the pending half-kick and the last record
    HIP_CHECK(hipStreamSynchronize(h->stream));
    h->upload_pending = false;
    md.step = step0 + n_steps;
    // The order in which the samplers' data become valid again is behaviour: corr, rdf, adf, order, sq, flux, then cluster
    // behind its give-up check, then cna. After a give-up, cluster and cna stay invalid and the six in front are valid.
    for (MdSampler *x : std::initializer_list<MdSampler *>{&md.corr, &md.rdf, &md.adf, &md.order, &md.sq, &md.flux})
      x->end_run(md.step);
    if (md.cluster.run) {
      unsigned gave_up = 0u;
      HIP_CHECK(hipMemcpy(&gave_up, md.cluster.giveup.ptr, sizeof(unsigned), hipMemcpyDeviceToHost));
      if (gave_up) {  // the data stay invalid
        HIP_CHECK(hipMemset(md.cluster.giveup.ptr, 0, 4 * sizeof(unsigned)));
        throw HipError("ta_md_run: a loop of the cluster link launch overran its cap; the cluster data are invalid");
      }
    }
    md.cluster.end_run(md.step);
    md.cna.end_run(md.step);
    if (n_rebuilds) *n_rebuilds = rebuilds;
    md_read_records(h, n_rec, want, cells_at_entry, epot, ekin, &rebuilds, n_rebuilds);
  });
  res.cell_running = md.baro.running = false;
  if (h->centre_gradients) {  // the evaluations of other calls take their usual builds again
    const std::string why = h->err;
    const int back = guarded(h, [&]() { set_centre_gradients(h, false); });
    if (rc != TA_OK) h->err = why;
    else if (back != TA_OK) return back;
  }
  return rc;
}

int ta_md_get_state(ta_handle h, double *positions, double *velocities) {
  if (!h) return TA_ERR_INVALID;
  if (const int rc = md_resident(h, "ta_md_get_state")) return rc;
  return guarded(h, [&]() {
    const size_t N = h->keep_species.size();
    HIP_CHECK(hipStreamSynchronize(h->stream));
    h->upload_pending = false;
    if (positions && N) HIP_CHECK(hipMemcpy(positions, h->db.pos, 3 * N * sizeof(double), hipMemcpyDeviceToHost));
    if (velocities && N) HIP_CHECK(hipMemcpy(velocities, h->md.vel.ptr, 3 * N * sizeof(double), hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
