// The handle behind the C ABI and what the host translation units (ta_api, ta_api_train, ta_api_md, ta_api_relax,
// ta_resident .hip) share: error mapping, self-freeing buffers, and the helpers that ta_api.hip defines
// for the others. Private to the library; the public interface is include/tensoralloy_amd.h.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "ta_device.h"
#include "ta_internal.h"
#include "ta_launch.h"
#include "ta_relax.h"
#include "ta_sampler_text.h"
#include "ta_schedule.h"

namespace ta {
namespace host {

struct HipError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

#define HIP_CHECK(expr)                                                                                    \
  do {                                                                                                     \
    hipError_t _e = (expr);                                                                                \
    if (_e != hipSuccess)                                                                                  \
      throw ::ta::host::HipError(std::string(#expr) + ": " + hipGetErrorString(_e) + " (" __FILE__ ":" +   \
                                 std::to_string(__LINE__) + ")");                                          \
  } while (0)

// grow-only device buffer; frees itself with its owner (the device of the handle must be current)
template <typename T>
struct DevBuf {
  T *ptr = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { release(); }
  void ensure(size_t n) {
    if (n <= cap) return;
    // the old allocation stays valid until the new one exists: a failed hipMalloc must not
    // leave a dangling pointer behind (contents are not carried over: every user refills)
    size_t want = n + n / 8 + 64;
    T *fresh = nullptr;
    hipError_t e = hipMalloc((void **)&fresh, want * sizeof(T));
    if (e != hipSuccess && ptr) {  // retry once with the old block returned first
      (void)hipGetLastError();
      HIP_CHECK(hipFree(ptr));
      ptr = nullptr;
      cap = 0;
      e = hipMalloc((void **)&fresh, want * sizeof(T));
    }
    if (e != hipSuccess) {
      (void)hipGetLastError();
      throw HipError(std::string("hipMalloc of ") + std::to_string(want * sizeof(T)) + " bytes: " +
                     hipGetErrorString(e));
    }
    if (ptr) HIP_CHECK(hipFree(ptr));
    ptr = fresh;
    cap = want;
  }
  // exactly n elements (a ring may take gigabytes: no head room); false when the device has no room
  bool try_exact(size_t n) {
    release();
    T *fresh = nullptr;
    if (hipMalloc((void **)&fresh, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    ptr = fresh;
    cap = std::max<size_t>(n, 1);
    return true;
  }
  void release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    cap = 0;
  }
};

// release() of every buffer given, of whatever element types
template <typename... B>
void release_all(B &...bufs) {
  (bufs.release(), ...);
}

// grow-only page-locked host buffer (staging for the packed uploads / downloads); frees itself likewise
struct PinnedBuf {
  char *ptr = nullptr;
  size_t cap = 0;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf &) = delete;
  PinnedBuf &operator=(const PinnedBuf &) = delete;
  ~PinnedBuf() { release(); }
  void ensure(size_t n) {
    if (n <= cap) return;
    if (ptr) HIP_CHECK(hipHostFree(ptr));
    ptr = nullptr;
    cap = 0;
    size_t want = n + n / 8 + 256;
    HIP_CHECK(hipHostMalloc((void **)&ptr, want, hipHostMallocDefault));
    cap = want;
  }
  void release() {
    if (ptr) (void)hipHostFree(ptr);
    ptr = nullptr;
    cap = 0;
  }
};

struct ChunkPlan {
  ta::AngChunk ch;
  int nb, ng, nz;
};

// What the loop of the device-resident runs (ta_resident.hip) keeps, for ta_md_run and ta_relax_run alike: the
// status words and their page-locked twins; the positions (and, in a run that moves the cells, the cells) the
// resident list was built for, the device twins of ref_pos / ref_cells as of list build number `ref_builds`;
// the workgroup layout (`chunk` atoms each) that blk_start holds.
struct ResidentLoop {
  DevBuf<unsigned> status;
  PinnedBuf status_host;
  DevBuf<double> ref, ref_cells;
  int64_t ref_builds = -1;
  DevBuf<int32_t> blk_start;
  std::vector<int32_t> blk_start_host;
  int chunk = 0, n_blk = 0;
  bool cell_running = false;  // a run that moves the cells (cell relaxation, barostat) is under way: rebuilds take them from the device
  volatile unsigned *host_words() const { return reinterpret_cast<volatile unsigned *>(status_host.ptr); }
};

// What every sampler of the MD loop keeps besides its own buffers (their shared lifecycle is in ta_api_md.hip): its
// texts, whether it is on, the workgroup layout of its launch for the resident batch (`blk` [F + 1]: the first
// workgroup of every frame, `chunk` items each), its schedule, and its part in the ta_md_run under way. A feature
// adds a `Setting set` (the C parameter struct and whatever else allocating for it needs), its buffers and a
// release() that frees them and ends in release_layout(). Where one buffer holds several arrays, or a ring holds rows,
// the Setting says how long each is and the struct where each starts (for F frames, E elements, N atoms of the
// resident batch): the only statement of that layout, which md_alloc, md_launch, the enqueue and the getters of
// ta_api_md.hip all go through.
struct MdSampler {
  const MdSamplerText &text;
  bool on = false;
  DevBuf<int32_t> blk;
  int n_blk = 0, chunk = 0;
  SampleSchedule sched;
  bool was_valid = false, run = false;  // set by begin_run
  explicit MdSampler(const MdSamplerText &t) : text(t) {}
  void release_layout() {
    blk.release();
    n_blk = 0;
    sched.valid = false;
    sched.last = -1;
  }
  // a ta_md_run begins: the data are invalid until end_run; `run`: the sampler has launches in it
  void begin_run(bool have_atoms) {
    was_valid = sched.suspend();
    run = on && was_valid && have_atoms;
  }
  // the run (and whatever else the feature checks) succeeded and ended at absolute step `step`
  void end_run(int64_t step) {
    if (run) sched.finish(step);
    sched.valid = was_valid;
  }
};

// device-resident MD loop (ta_api_md.hip; the integrator launch is in ta_md.hip): masses, velocities, the
// records of the running ta_md_run, the steps integrated since ta_md_init (the noise's step counter and the
// clock of the sample schedules), and one struct per feature with its setting, buffers and host records
struct MdState {
  bool valid = false;
  DevBuf<double> mass, vel, epot, ke;
  int64_t step = 0;
  struct {  // ta_md_set_thermostat; off while kT0 == 0
    double kT0 = 0.0, tau = 0.0;
  } berendsen;
  struct {  // ta_md_set_langevin; off while friction == 0: bath, friction, the key of the noise, ta_md_noise's scratch
    double kT0 = 0.0, friction = 0.0;
    uint64_t seed = 0;
    DevBuf<double> noise;
  } langevin;
  // Nose-Hoover chain (ta_md_set_nose_hoover): the chain state [F][TA_MD_MAX_CHAIN] (zeroed by ta_md_init), the
  // record of the running ta_md_run and the host's copy [n_rec][F] of the last successful run's chain terms
  struct {
    bool on = false;
    ta_md_nhc_params p = {0.0, 0.0, 3, 1, 0};
    DevBuf<double> eta, veta, rec;
    bool rec_valid = false;
    std::vector<double> rec_host;
  } nhc;
  // Berendsen barostat (ta_md_set_barostat): the cumulative scale of every frame since its list was built with
  // the ones that reset it, the device records {V, P_x, P_y, P_z} of the running ta_md_run and the host's copy
  // of the last successful run's, [n_rec][F] and [n_rec][F][3]
  struct {
    bool on = false;
    bool running = false;  // a barostat run is under way: a rebuild resets the cumulative scale
    ta_md_barostat_params p = {0.0, 0.0, 0.0, {1, 1, 1}, 1};
    DevBuf<double> scale, rec;
    std::vector<double> ones;
    bool rec_valid = false;
    std::vector<double> rec_volume, rec_press;
  } baro;
  // Martyna-Tobias-Klein barostat (ta_md_set_mtk_barostat): the strain rates [F][3] and the barostat's chain
  // [F][TA_MD_MAX_CHAIN] (zeroed by ta_md_init), the record of E_baro of the running ta_md_run and the host's copy
  // [n_rec][F] of the last successful run's. While it runs it uses what `baro` keeps for a run that moves the cells:
  // scale, ones, rec {V, P_c}, rec_volume, rec_press and `running`
  struct {
    bool on = false;
    ta_md_mtk_params p = {0.0, 0.0, 3, 1, {1, 1, 1}, 1};
    DevBuf<double> omega, xi, vxi, rec;
    bool rec_valid = false;
    std::vector<double> rec_host;
  } mtk;
  bool moves_cells() const { return baro.on || mtk.on; }  // a barostat is on: ta_md_run moves the cells
  // Sampling (ta_md_set_sampling): the rings [L][N][3], the accumulators [2][F][E][L] (v . v, then |dx|^2), the
  // correlation launch's partials; its layout is in chunks of kMdCorrChunk ring doubles
  struct Corr : MdSampler {
    Corr() : MdSampler(md_text::corr) {}
    struct Setting {
      ta_md_sampling_params p = {0, 1};
      size_t n_sums(size_t F, size_t E) const { return F * E * (size_t)p.n_lags; }  // of v . v; as many of |dx|^2
      size_t n_acc(size_t F, size_t E) const { return 2 * n_sums(F, E); }
    } set;
    DevBuf<double> ring_x, ring_v, acc, part;
    double *acc_v() const { return acc.ptr; }
    double *acc_x(size_t F, size_t E) const { return acc.ptr + set.n_sums(F, E); }
    // where sample n is held in a ring
    double *slot(const DevBuf<double> &ring, int64_t n, size_t N) const { return ring.ptr + (size_t)(n % set.p.n_lags) * 3 * N; }
    void release() {  // frees what sampling holds on the device; the setting stays
      release_all(ring_x, ring_v, acc, part);
      release_layout();
    }
  } corr;
  // Pair distributions (ta_md_set_rdf): the counts [F][E][E][n_bins]
  struct Rdf : MdSampler {
    Rdf() : MdSampler(md_text::rdf) {}
    struct Setting {
      ta_md_rdf_params p = {0.0, 0, 1};
    } set;
    DevBuf<unsigned long long> acc;
    void release() {  // frees what the pair distributions hold on the device; the setting stays
      acc.release();
      release_layout();
    }
  } rdf;
  // Bond-angle distributions (ta_md_set_adf): the bond cutoffs [E][E] of the setting, their squares on the
  // device, the counts [F][E][E (E + 1) / 2][n_bins]
  struct Adf : MdSampler {
    Adf() : MdSampler(md_text::adf) {}
    struct Setting {
      ta_md_adf_params p = {0.0, 0, 1};
      std::vector<double> rb;
    } set;
    DevBuf<double> rb2;
    DevBuf<unsigned long long> acc;
    void release() {  // frees what the bond-angle distributions hold on the device; the setting stays
      release_all(rb2, acc);
      release_layout();
    }
  } adf;
  // Bond-orientational order (ta_md_set_order): the bond cutoffs [E][E] of the setting, their squares and the N_lm
  // on the device, the counts (hist_q, hist_qbar [F][E][D][n_bins], then hist_conn [F][E][32], one buffer) and the
  // per-atom arrays of the newest sample (q_lm [N][n_lm][2]; q, qbar [N][D] in `per_atom`; N_b, n_conn [N] in
  // `per_atom_int`)
  struct Order : MdSampler {
    Order() : MdSampler(md_text::order) {}
    struct Setting {
      ta_md_order_params p = {0.0, 0.0, 0, 1, 0, {0, 0, 0, 0}, 0};
      std::vector<double> rb;
      size_t n_hist(size_t F, size_t E) const { return F * E * (size_t)p.n_degrees * (size_t)p.n_bins; }  // hist_q; hist_qbar
      static size_t n_hist_conn(size_t F, size_t E) { return F * E * (TA_MD_ORDER_MAX_CONN + 1); }
      size_t n_acc(size_t F, size_t E) const { return 2 * n_hist(F, E) + n_hist_conn(F, E); }
      size_t n_q(size_t N) const { return N * (size_t)p.n_degrees; }  // q; qbar
    } set;
    DevBuf<double> rb2, norm, qlm, per_atom;
    DevBuf<int32_t> per_atom_int;
    DevBuf<unsigned long long> acc;
    int n_lm = 0, solid = 0;
    unsigned long long *hist_q() const { return acc.ptr; }
    unsigned long long *hist_qbar(size_t F, size_t E) const { return acc.ptr + set.n_hist(F, E); }
    unsigned long long *hist_conn(size_t F, size_t E) const { return acc.ptr + 2 * set.n_hist(F, E); }
    double *q() const { return per_atom.ptr; }
    double *qbar(size_t N) const { return per_atom.ptr + set.n_q(N); }
    int32_t *n_bonds() const { return per_atom_int.ptr; }
    int32_t *n_conn(size_t N) const { return per_atom_int.ptr + N; }
    void release() {  // frees what the order parameters hold on the device; the setting stays
      release_all(rb2, norm, qlm, per_atom, per_atom_int, acc);
      release_layout();
    }
  } order;
  // Clusters of selected atoms (ta_md_set_clusters): the link cutoffs [E][E] of the setting and their squares on the
  // device, the per-atom arrays (parent, count, label, size, [N] each, one buffer), the histogram [F][n_bins], the
  // ring of series rows [n_series][F][4] and the give-up word of the link launch
  struct Cluster : MdSampler {
    Cluster() : MdSampler(md_text::cluster) {}
    struct Setting {
      ta_md_cluster_params p = {0.0, 0, 0, 0, 1, 1};
      std::vector<double> rl;
      size_t n_hist(size_t F) const { return F * (size_t)p.n_bins; }
      static size_t row(size_t F) { return F * 4; }  // words of a row of the series
      size_t n_series(size_t F) const { return (size_t)p.n_series * row(F); }
    } set;
    DevBuf<double> rl2;
    DevBuf<int32_t> per_atom;
    DevBuf<unsigned long long> acc;
    DevBuf<long long> series;
    DevBuf<unsigned> giveup;
    static size_t n_per_atom(size_t N) { return 4 * N; }
    int32_t *parent() const { return per_atom.ptr; }
    int32_t *count(size_t N) const { return per_atom.ptr + N; }
    int32_t *label(size_t N) const { return per_atom.ptr + 2 * N; }
    int32_t *size(size_t N) const { return per_atom.ptr + 3 * N; }
    long long *series_row(int64_t n, size_t F) const { return series.ptr + (size_t)(n % set.p.n_series) * set.row(F); }  // of sample n
    void release() {  // frees what the clusters hold on the device; the setting stays
      release_all(rl2, per_atom, acc, series, giveup);
      release_layout();
    }
  } cluster;
  // Common neighbour analysis (ta_md_set_cna): the setting (r_max resolved), the per-atom arrays of the newest sample,
  // the counts [F][E][5] and the ring of series rows [n_series][F][5]
  struct Cna : MdSampler {
    Cna() : MdSampler(md_text::cna) {}
    struct Setting {
      ta_md_cna_params p = {0.0, 0.0, 0, 0, 1};
      static size_t n_acc(size_t F, size_t E) { return F * E * TA_MD_CNA_TYPES; }
      static size_t row(size_t F) { return F * TA_MD_CNA_TYPES; }  // words of a row of the series
      size_t n_series(size_t F) const { return (size_t)p.n_series * row(F); }
    } set;
    DevBuf<int32_t> structure;
    DevBuf<double> r_local;
    DevBuf<unsigned long long> acc, series;
    unsigned long long *series_row(int64_t n, size_t F) const { return series.ptr + (size_t)(n % set.p.n_series) * set.row(F); }  // of sample n
    void release() {  // frees what the analysis holds on the device; the setting stays
      release_all(structure, r_local, acc, series);
      release_layout();
    }
  } cna;
  // Structure factors (ta_md_set_sq): the Miller triples [Q][3] of the setting and their device twin, the ring of
  // amplitude rows [L][F][E][planes][Q] (planes = 2, or 8 with currents), the accumulators (A_rho, then A_L and
  // A_J with currents, [F][E][E][L][Q] each, one buffer), the amplitude launch's partials, and the two rows [N][3]
  // the integrator writes a sampled state to when md_set_sampling's ring does not take it
  struct Sq : MdSampler {
    Sq() : MdSampler(md_text::sq) {}
    struct Setting {
      ta_md_sq_params p = {0, 1, 1, 0};
      std::vector<int32_t> miller;
      size_t planes() const { return p.currents ? 8 : 2; }
      size_t row(size_t F, size_t E) const { return F * E * planes() * (size_t)p.n_q; }  // doubles of a row of the ring
      size_t n_sums(size_t F, size_t E) const { return F * E * E * (size_t)p.n_lags * (size_t)p.n_q; }  // A_rho; A_L; A_J
      size_t n_acc(size_t F, size_t E) const { return (p.currents ? 3 : 1) * n_sums(F, E); }
    } set;
    DevBuf<int32_t> miller_dev;
    DevBuf<double> ring, acc, part, snap_x, snap_v;
    double *acc_rho() const { return acc.ptr; }
    double *acc_l(size_t F, size_t E) const { return acc.ptr + set.n_sums(F, E); }  // (with currents)
    double *acc_j(size_t F, size_t E) const { return acc.ptr + 2 * set.n_sums(F, E); }
    double *ring_row(int64_t n, size_t F, size_t E) const { return ring.ptr + (size_t)(n % set.p.n_lags) * set.row(F, E); }  // of sample n
    void release() {  // frees what the structure factors hold on the device; the setting stays
      release_all(ring, acc, part, snap_x, snap_v, miller_dev);
      release_layout();
    }
  } sq;
  // Heat current and pressure tensor (ta_md_set_flux): the ring of rows [L][F][18], the accumulators (sums [F][18],
  // a_heat [F][L][3], a_press [F][L][6], one buffer in that order), the pair sweep's partials, and the two rows [N][3]
  // the integrator writes a sampled state to when neither md_set_sampling's ring nor md_set_sq's rows take it
  struct Flux : MdSampler {
    Flux() : MdSampler(md_text::flux) {}
    struct Setting {
      ta_md_flux_params p = {0, 1};
      static size_t row(size_t F) { return F * TA_MD_FLUX_ROW; }  // doubles of a row of the ring, and of the sums
      size_t n_heat(size_t F) const { return F * (size_t)p.n_lags * 3; }
      size_t n_press(size_t F) const { return F * (size_t)p.n_lags * 6; }
      size_t n_acc(size_t F) const { return row(F) + n_heat(F) + n_press(F); }
    } set;
    DevBuf<double> ring, acc, part, snap_x, snap_v;
    double *sums() const { return acc.ptr; }
    double *acc_heat(size_t F) const { return acc.ptr + set.row(F); }
    double *acc_press(size_t F) const { return acc.ptr + set.row(F) + set.n_heat(F); }
    double *ring_row(int64_t n, size_t F) const { return ring.ptr + (size_t)(n % set.p.n_lags) * set.row(F); }  // of sample n
    void release() {  // frees what the sampler holds on the device; the setting stays
      release_all(ring, acc, part, snap_x, snap_v);
      release_layout();
    }
  } flux;
};

// every sampler of the MD loop in the canonical order: the one ta_md_init allocates them in and reports the first
// failure in (fn takes the feature's own struct: a generic lambda)
template <typename Fn>
void for_each_sampler(MdState &md, Fn &&fn) {
  fn(md.corr), fn(md.rdf), fn(md.adf), fn(md.order), fn(md.cluster), fn(md.cna), fn(md.sq), fn(md.flux);
}

// device-resident relaxation (ta_api_relax.hip; the launches are in ta_relax.hip): FIRE velocities of its own,
// the mask of fixed atoms (and the host's copy of ta_relax_init's), the two copies of the per-frame state with
// the host's image of the current one, the workgroups' partial sums and the count of converged frames
struct RelaxState {
  bool valid = false;
  ta_fire_params p = {0.1, 1.0, 0.2, 1.1, 0.5, 0.1, 0.99, 5};
  DevBuf<double> vel, part;
  DevBuf<uint8_t> fixed;
  DevBuf<ta::RelaxFrameState> state;
  DevBuf<int> count;
  std::vector<ta::RelaxFrameState> state_host;
  std::vector<uint8_t> fixed_host;
  // cell mode (ta_relax_set_cell): h0 and the cell factor of every frame, the deformation gradient and the cell
  // velocity (two copies on the device like `state`, the current one on the host between runs)
  struct {
    bool on = false;
    ta_relax_cell_params p = {0.0, 0.0, {1, 1, 1, 1, 1, 1}, 0, 0};
    DevBuf<double> h0, cf, G, vel, fmax2;
    std::vector<double> G_host, vel_host;
    void reset_deformation(size_t F) {  // G = I and the cell at rest, for F frames
      G_host.assign(9 * F, 0.0);
      for (size_t f = 0; f < F; ++f) G_host[9 * f] = G_host[9 * f + 4] = G_host[9 * f + 8] = 1.0;
      vel_host.assign(9 * F, 0.0);
    }
  } cell;
  // band mode (ta_relax_set_band; the band launches are in ta_neb.hip): the frames are the images of a nudged
  // elastic band and FIRE runs on the band forces with the whole band as ONE pseudo-frame. The band owns its
  // force and tangent arrays, the partials of its two launches, the mask (the user's OR-ed with the two endpoint
  // images), the two copies of the one FIRE record and the pseudo-frame's layout {atom_start[2], blk_start[2],
  // climbing image}.
  struct {
    bool on = false;
    bool ran = false;  // a band run left B, tau and the climbing image of the resident state
    ta_band_params p = {0.1, 0, 0};
    DevBuf<double> force, tau, part;
    DevBuf<uint8_t> fixed;
    DevBuf<ta::RelaxFrameState> state;
    DevBuf<int32_t> layout;
    ta::RelaxFrameState state_host = {};
    std::vector<double> energy_host;  // [F] image energies of the state the last band run ended on
  } band;
};

// harmonic phonons (ta_api_phonon.hip; the launches are in ta_phonon.hip): the supercell description of
// ta_phonon_set_cell, the force-constant rows of the home cell, and the work space of a chunk of q-points
struct PhononState {
  bool valid = false;    // ta_phonon_set_cell has run for the resident frame
  bool have_phi = false;
  int n_basis = 0, N = 0;
  int64_t q_chunk = 0;   // q-points per pass, a multiple of the DOS slab
  DevBuf<int32_t> basis_of, start;
  DevBuf<double> mass, vec, phi, q, D, w, V, nu, dos_part, dos_slab;
  DevBuf<unsigned long long> counts;  // [n_bins] total, then the two info words
};

}  // namespace host
}  // namespace ta

struct ta_context {
  template <typename T>
  using DevBuf = ta::host::DevBuf<T>;
  using PinnedBuf = ta::host::PinnedBuf;
  using ChunkPlan = ta::host::ChunkPlan;

  ta::Options opt;  // the environment switches as they stood when ta_create ran
  int device = 0;
  hipStream_t stream = nullptr;      // stream all work is enqueued on
  hipStream_t own_stream = nullptr;  // created by ta_create
  int kind = 0;
  int n_elements = 0;
  int activation = 0;
  double rmax = 0.0;
  ta::SFParams sf;
  std::vector<ChunkPlan> chunks;     // first-generation kernels: up to 2 betas per launch
  std::vector<ChunkPlan> chunks_v2;  // second-generation kernels: one beta per launch
  bool use_v2 = false;
  ta::MlpDev *mlp_dev = nullptr;     // device copy of mlp[0..n_elements)
  ta::MlpDev mlp[ta::kMaxElements];
  // temperature-dependent head (ta_model_desc.finite_temperature): nets H[el], U[el], S[el]
  bool td = false, td_sommerfeld = false;
  int td_act = 0, td_K = 0;
  ta::MlpDev td_nets[3 * ta::kMaxElements];
  ta::MlpDev *td_dev = nullptr;
  std::vector<void *> model_allocs;
  ta::EamModel *eam = nullptr;
  ta::GrapModel *grap = nullptr;

  ta::HostPairs hp;
  ta::DeviceBatch db;
  bool have_batch = false;
  uint32_t last_want = 0;

  // Inputs travel in one packed upload: [pos | cells | grids | species | frame_of_atom |
  // atom_start | elem_atoms | blk_center]; results come back in one packed download:
  // [energy F | virial 9F | atomic N | forces 3N].
  PinnedBuf stage_in, stage_out;
  DevBuf<char> inbuf;
  DevBuf<double> results;
  size_t o_blk = 0;  // byte offset of blk_center in the packed input
  int res_n_blk = 0;  // runs of the resident list's packing (db.n_blk is the exact list's while `filtered`)
  DevBuf<double> rec, part4, G, dEdG, g, wat, bpart, fown, benergy, mlp_scratch;
  DevBuf<double> td_T, td_u, td_s;  // electron temperature per frame; U and S per atom
  DevBuf<unsigned long long> masks;
  DevBuf<uint32_t> job_word;
  DevBuf<int32_t> job_count;
  // triangle-once backward pass (ta_set_triangles): the owned job lists, the handle's option, whether the
  // resident batch's cells admit the ownership rule, and the builds the last backward pass ran
  DevBuf<uint32_t> job_word_own;
  DevBuf<int32_t> job_count_own;
  bool triangles = true;
  // A ta_md_run that samples the heat current is under way (set_centre_gradients): every evaluation leaves
  // g_p = d e_c / d D_p, the gradient of the CENTRE's energy alone, in db.g together with the pair records. The
  // triangle-once build and the folded EAM / ADP force kernels do not, and step aside while this is set.
  bool centre_gradients = false;
  // the last second-generation forward pass left the full job list (db.job_word / job_count) behind: it
  // does not when every backward launch of its evaluation read the owned lists (forward_v2_launches)
  bool full_jobs_valid = false;
  bool tri_cells_ok = false;
  bool tri_cells_wide_ok = false;  // every periodic width exceeds rmax + skin: what the cell relaxation asks for
  int last_bwd_variant = 0;
  ta::MlpLaunchInfo last_mlp_launch;  // ta_mlp_launch_info
  DevBuf<int32_t> pair_start, seg_start, pair_i, pair_j, pair_shift, pair_rev;
  ta::NlGrid *d_grids = nullptr;  // view into inbuf
  // device neighbour list (ta_nlist.hip)
  DevBuf<int32_t> nl_wrap, nl_binid, nl_bin_count, nl_bin_start, nl_bin_cursor, nl_bin_atoms, nl_counts;
  DevBuf<unsigned long long> nl_stats, nl_zero;
  unsigned long long *nl_stats_ptr = nullptr;  // statistics block of the builder that made the list
  bool nl_sorted = false;  // list in key order (one-pass builder): reverse pairs by binary search
  bool nl_rev_done = false;  // ... and the reverse index is already there (launched behind the pairs)
  bool nl_zero_clean = false;  // nl_zero is all zero where the next list needs it (see nl_build)
  int64_t nl_zero_atoms = -1;
  int nl_zero_bins = -1;
  DevBuf<double> hvp_buf;  // ta_hessian_vectors: tangents in, force / virial tangents out
#ifdef TA_PHASE_STAMPS
  DevBuf<unsigned long long> stamp_buf;
#endif
  DevBuf<ta::NlRec> nl_recs;
  bool pairs_on_device = false;  // hp holds only the counts; ta_get_pairs downloads on demand
  bool descriptors_valid = false;  // db.G holds the resident batch's descriptors
  DevBuf<double> train_scratch, train_partial, train_grad, train_coeff;
  // force / stress terms of the loss: J[c][p] = dG_c / dD_p of the resident batch (made once per
  // batch by one backward launch per descriptor channel), the direction and its images
  DevBuf<double> jvp_J, tan_dD, tan_dG, tan_dir;
  DevBuf<double> filt_scratch;  // ta_grap_loss_gradient: pair vectors, w-dot, per-pair adjoints, partial sums
  bool jvp_valid = false;

  // MD loop (ta_set_skin / ta_update_positions): the list covers rmax + skin and is kept while no
  // atom has moved more than skin / 2 from where it was when the list was built
  double skin = 0.0;
  double r_list = 0.0;                         // rmax + skin: cutoff of the resident list
  std::vector<int32_t> keep_species;           // [N]
  std::vector<int32_t> keep_natoms, keep_pbc;  // [F], [3 F]: what a rebuild needs besides stage_in
  std::vector<double> ref_pos, ref_cells;      // positions / cells the resident list was built for
  size_t o_pos = 0, o_cells = 0, o_species = 0;  // byte offsets in the packed input
  // exact list of the current step, extracted on the device from the resident skin list (nl_filter)
  DevBuf<int32_t> ex_pair_i, ex_pair_j, ex_pair_shift, ex_pair_rev, ex_pair_start, ex_pair_stop, ex_seg_start, ex_counts,
      ex_map, ex_blk, ex_slot_q;
  DevBuf<ta::BlockHeader> ex_hdr;              // the exact list's run headers (DeviceBatch::blk_hdr)
  bool filtered = false;                       // db points at the ex_* arrays
  // a copy out of stage_in may still be in flight (set by ta_update_positions, cleared by every wait
  // for the stream on the step path): whoever rewrites stage_in waits for the stream first. (An event
  // recorded behind the copy cost a 5 us bubble between the copy and the next kernel of every MD step.)
  bool upload_pending = false;
  // ta_step: the next compute mirrors its results into stage_out (frame_reduce_kernel); `mirror_want` = the
  // want bits whose results the page-locked image holds right now (0: none), cleared by whoever reuses stage_out
  bool mirror_next = false;
  uint32_t mirror_want = 0;
  int64_t n_list_builds = 0, n_list_reuses = 0;

  ta::host::ResidentLoop res;  // ta_md_run and ta_relax_run: the loop they share
  ta::host::MdState md;
  ta::host::RelaxState relax;
  ta::host::PhononState phonon;

  hipEvent_t ev[2 * TA_N_KERNEL_SLOTS + 2] = {nullptr};
  std::string err;
};

namespace ta {
namespace host {

// ta_api.hip
int fail(ta_context *h, int code, const std::string &msg);  // keeps the message for ta_last_error; returns code
// `to_host`: the copy direction of the fallback, which Options::staged_copy_dma always takes (A/B switch)
void staged_copy(double *dst, const double *src, size_t n, bool to_host, const ta::Options &opt, hipStream_t s);
void wait_stream(hipStream_t s, const ta::Options &opt);
void compute_impl(ta_context *h, uint32_t want, bool timed, double *slot_ms);
// for ta_api_train.hip: the forward launches of the second-generation angular path alone (`tri`: see the definition),
// and the texts of the two inference-only refusals
void forward_v2_launches(ta_context *h, bool tri);
std::string td_inference_only(const char *fn);
std::string fs_inference_only(const char *fn);
void apply_filter(ta_context *h);
// Switches ta_context::centre_gradients. A plain EAM model then evaluates through eam_pair_kernel and the force
// gather, on the resident (skin) list itself: its per-pair launches walk [0, n_pairs), which the exact list of
// apply_filter does not admit. Switched off, the exact list comes back. Throws.
void set_centre_gradients(ta_context *h, bool on);
// the resident frames again with new coordinates (cells: null = unchanged): the rebuild path of
// ta_update_positions and the resident runs; throws
void rebuild_list(ta_context *h, const double *positions, const double *cells);

// ta_api_train.hip
// ta_hessian_vectors with the force tangents left on the device as well: dF_dev [n_dir][N][3] (either of dF,
// dF_dev may be null, not both). Same checks, same return codes, same values.
int hessian_vectors_impl(ta_context *h, int32_t n_dir, int32_t first, const double *dR, const double *dh, double *dF,
                         double *dW, double *dF_dev);

// ta_resident.hip
// workgroups of the integrator launch: `chunk` consecutive atoms of one frame each, at least one per frame
void md_plan_blocks(ta_context *h, int chunk);
// what every resident run does before its first launch: where the host built the list that is resident, its
// positions go up once as res.ref; the status words are reset
void resident_begin(ta_context *h);
// The loop that ta_md_run and ta_relax_run share (see ta_resident.hip). Returns the steps done; throws.
int resident_steps(ta_context *h, const char *who, int n_steps, uint32_t want, const std::function<void(int)> &enqueue,
                   const std::function<int(int, int)> &finished, int *rebuilds, int32_t *n_rebuilds);
// after a run that moved the cells (F > 0): where they differ from ref_cells, one list for the final state and
// the evaluation again on it, counted in *rebuilds and *n_rebuilds (may be null). `who` names the caller in the
// messages.
void resident_final_cells(ta_context *h, const char *who, uint32_t want, int *rebuilds, int32_t *n_rebuilds);

// runs fn with the handle's device current and maps what it throws to the error codes of the C ABI
template <typename F>
int guarded(ta_context *h, F &&fn) {
  try {
    if (h) HIP_CHECK(hipSetDevice(h->device));
    fn();
    return TA_OK;
  } catch (const HipError &e) {
    return fail(h, TA_ERR_HIP, e.what());
  } catch (const std::domain_error &e) {
    return fail(h, TA_ERR_UNSUPPORTED, e.what());
  } catch (const std::invalid_argument &e) {
    return fail(h, TA_ERR_INVALID, e.what());
  } catch (const std::bad_alloc &) {
    return fail(h, TA_ERR_NOMEM, "host allocation failed");
  } catch (const std::exception &e) {
    return fail(h, TA_ERR_INVALID, e.what());
  }
}

}  // namespace host
}  // namespace ta
