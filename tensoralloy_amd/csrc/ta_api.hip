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

#include "ta_device.h"
#include "ta_internal.h"
#include "ta_md.h"
#include "ta_neb.h"
#include "ta_relax.h"

namespace ta {
size_t mlp_scratch_doubles(const MlpDev &mlp);
void launch_mlp_impl(const MlpDev &mlp, int activation, int ndim, const int32_t *atoms, int n_atoms,
                     const DeviceBatch &b, const Options &opt, double *scratch, hipStream_t s,
                     MlpLaunchInfo *info = nullptr);
size_t mlp_all_scratch_doubles(const MlpDev *mlps_host, int nel, const int32_t *elem_start);
size_t td_scratch_doubles(const MlpDev *nets, int nel, int K, const int32_t *elem_start, bool da_global);
void launch_td_all(const MlpDev *nets_dev, const MlpDev *nets_host, int nel, int K, int act_h, int act,
                   int sommerfeld, int ndim, const DeviceBatch &b, bool da_global, const double *T, double *u_atom,
                   double *s_atom, double *scratch, hipStream_t s, MlpLaunchInfo *info = nullptr);
void launch_mlp_all(const MlpDev *mlps_dev, const MlpDev *mlps_host, int nel, int activation, int ndim,
                    const DeviceBatch &b, const Options &opt, double *scratch, hipStream_t s,
                    MlpLaunchInfo *info = nullptr);
// weight gradients (ta_train.hip)
int mlp_param_count(const MlpDev &mlp);
size_t mlp_grad_scratch_doubles(const MlpDev &mlp, int n_atoms);
size_t mlp_grad_partial_doubles(const MlpDev &mlp, int n_atoms);
void launch_mlp_grad(const MlpDev &mlp, int activation, int ndim, const int32_t *atoms, int n_atoms,
                     const DeviceBatch &b, const double *frame_coeff, double *scratch, double *partial,
                     double *grad, hipStream_t s);
size_t mlp_grad2_scratch_doubles(const MlpDev &mlp, int n_atoms);
void launch_mlp_grad2(const MlpDev &mlp, int activation, int ndim, const int32_t *atoms, int n_atoms,
                      const DeviceBatch &b, const double *dG, const double *frame_coeff, double *scratch,
                      double *partial, double *grad, hipStream_t s, double *kappa_out = nullptr);
// weight gradients of the temperature-dependent head (ta_td_train.hip)
int td_param_count(const MlpDev *nets, int nel);
void td_grad2_sizes(const MlpDev *nets, int nel, int K, const int32_t *elem_start, size_t *scratch,
                    size_t *partial);
void launch_td_grad2(const MlpDev *nets_dev, const MlpDev *nets_host, int nel, int K, int act_h, int act,
                     int sommerfeld, int ndim, const DeviceBatch &b, const double *T, const double *dG,
                     const double *coeff, double *scratch, double *partial, double *grad, hipStream_t s);
// analytic Hessian-vector products of the descriptor models (ta_hvp.hip)
void launch_pair_vec(const DeviceBatch &b, double *Dv, hipStream_t s);
void launch_backward_hvp(const SFParams &sf, const AngChunk &ch, int nb, int ng, int nz, bool first, bool angular,
                         const DeviceBatch &b, const double *Dv, const double *Dd, const double *wdot, double *gv,
                         double *gd, hipStream_t s);
void launch_hvp_gather(const DeviceBatch &b, const double *Dv, const double *Dd, const double *gv, const double *gd,
                       double *fdot, double *wdot_at, hipStream_t s);
void launch_pair_tangent(const DeviceBatch &b, const double *dR, const double *dh, double *dD, hipStream_t s);
void launch_descriptor_jvp(const DeviceBatch &b, int ndim, const double *J, const double *dD, double *dG,
                           hipStream_t s);
void launch_one_hot(double *dEdG, int64_t n_atoms, int ndim, int c, hipStream_t s);
// GRAP (ta_grap.hip)
struct GrapModel;
bool grap_hvp_supported(const GrapModel *);
void launch_grap_hvp(GrapModel *, const DeviceBatch &b, double eps, const double *Dv, const double *Dd,
                     const double *wdot, double *gv, double *gd, hipStream_t s);
GrapModel *grap_create(const ta_model_desc *m, std::string &err);
int grap_ndim(const GrapModel *g);
bool grap_uses_filter_net(const GrapModel *g);
void grap_destroy(GrapModel *);
void grap_ensure(GrapModel *, const DeviceBatch &b);
void launch_grap_forward(GrapModel *, const DeviceBatch &b, double eps, hipStream_t s);
void launch_grap_backward(GrapModel *, const DeviceBatch &b, hipStream_t s);
// training the GRAP filter network (ta_grap.hip)
int64_t grap_filter_param_count(const GrapModel *g);
void grap_update_filter_weights(GrapModel *g, const double *flat, int64_t n, hipStream_t s);
int grap_filter_table_knots(const GrapModel *g);
void grap_set_filter_tables(GrapModel *g, bool on, int n_knots, hipStream_t s);
int grap_filter_table_target(const GrapModel *g, bool on, int n_knots);
void grap_mark_trained(GrapModel *g);
void grap_suspend_filter_tables(GrapModel *g, bool suspend);
std::string grap_filter_train_refusal(const GrapModel *g);
size_t grap_filter_grad_doubles(const GrapModel *g, const DeviceBatch &b);
void launch_grap_filter_tangent(GrapModel *g, const DeviceBatch &b, double eps, const double *Dv, const double *Dd,
                                double *Gdot, hipStream_t s);
void grap_filter_gradient(GrapModel *g, const DeviceBatch &b, double eps, const double *Dv, const double *Dd,
                          const double *kappa, double *scratch, double *grad, hipStream_t s);
// EAM / ADP (ta_eam.hip)
struct EamModel;
EamModel *eam_create(const ta_model_desc *m, const Options &opt, std::string &err);
void eam_destroy(EamModel *);
void eam_ensure(EamModel *, const DeviceBatch &b);
void eam_tabulate(EamModel *m, int n_r, const double *r, int n_rho, const double *rho, double *rho_of_r,
                  double *phi_of_r, double *embed_of_rho, double *u_of_r, double *w_of_r,
                  hipStream_t s);
void eam_compute(EamModel *, const DeviceBatch &b, uint32_t want, hipStream_t s,
                 hipEvent_t *ev /* 2 events or null */);
void eam_set_list_cutoff(EamModel *, double rc /* 0: the list is exact, no test */);
bool eam_is_plain(const EamModel *);
void eam_set_nn_tables(EamModel *, bool on);
bool eam_hvp_supported(const EamModel *);
size_t eam_hvp_extra_doubles(const EamModel *, const DeviceBatch &b, int n_dir);
void eam_hvp(EamModel *, const DeviceBatch &b, int n_dir, bool unit, int first, const double *dR, const double *dh,
             double *dFdot, double *fdot, double *wdot, double *extra, hipStream_t s);
bool eam_nn_tables_on(const EamModel *);
void eam_mark_trained(EamModel *);
int64_t eam_param_count(const EamModel *);
void eam_update_weights(EamModel *, const double *flat, int64_t n);
int64_t eam_constant_count(const EamModel *);
void eam_get_constants(const EamModel *, double *flat);
void eam_update_constants(EamModel *, const double *flat, int64_t n);
void eam_constant_gradient(EamModel *, const DeviceBatch &b, const double *frame_coeff, const double *dR,
                           const double *dh, double *grad, hipStream_t s);
void eam_energy_gradient(EamModel *, const DeviceBatch &b, const double *frame_coeff, double *grad,
                         hipStream_t s);
bool eam_loss_gradient_supported(const EamModel *);
void eam_loss_gradient(EamModel *, const DeviceBatch &b, const double *frame_coeff, const double *dR,
                       const double *dh, double *grad, hipStream_t s);
}  // namespace ta

namespace {

thread_local std::string g_create_error;

struct HipError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

#define HIP_CHECK(expr)                                                                      \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess)                                                                    \
      throw HipError(std::string(#expr) + ": " + hipGetErrorString(_e) + " (" __FILE__ ":" + \
                     std::to_string(__LINE__) + ")");                                        \
  } while (0)

// grow-only device buffer
template <typename T>
struct DevBuf {
  T *ptr = nullptr;
  size_t cap = 0;
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
  void release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    cap = 0;
  }
};

// Small transfers between the page-locked staging buffers and device memory as a kernel ON the
// compute stream (the device reads / writes the mapped host memory over PCIe) instead of an
// asynchronous copy: a copy command goes to a DMA engine behind cross-queue barriers, about 10 us
// of latency each way, which is what one MD step of a 4000-atom frame (96 KB in, 128 KB out) pays.
__global__ __launch_bounds__(256) void staged_copy_kernel(double *__restrict__ dst,
                                                          const double *__restrict__ src, size_t n) {
  for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (size_t)gridDim.x * 256) dst[k] = src[k];
}
constexpr size_t kStagedCopyMaxBytes = 4u << 20;  // beyond that the DMA engine's bandwidth wins

// `to_host`: the copy direction of the fallback, which Options::staged_copy_dma always takes (A/B switch)
void staged_copy(double *dst, const double *src, size_t n, bool to_host, const ta::Options &opt, hipStream_t s) {
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
void wait_stream(hipStream_t s, const ta::Options &opt) {
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

// grow-only page-locked host buffer (staging for the packed uploads / downloads)
struct PinnedBuf {
  char *ptr = nullptr;
  size_t cap = 0;
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

}  // namespace

struct ta_context {
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

  // device-resident MD loop (ta_md_init / ta_md_run; the integrator launch is in ta_md.hip): masses,
  // velocities and the positions the resident list was built for (the device twin of ref_pos, as of
  // list build number `md_ref_builds`); records of the running ta_md_run; the status word and its
  // page-locked twin; the workgroup layout (`md_chunk` atoms each) that md_blk_start holds
  bool md_valid = false;
  DevBuf<double> md_mass, md_vel, md_ref, md_epot, md_ke;
  DevBuf<int32_t> md_blk_start;
  DevBuf<unsigned> md_status;
  PinnedBuf md_status_host;
  std::vector<int32_t> md_blk_start_host;
  int md_chunk = 0, md_n_blk = 0;
  int64_t md_ref_builds = -1;
  double md_kT0 = 0.0, md_tau = 0.0;
  // Nose-Hoover chain (ta_md_set_nose_hoover; off while md_nhc_on is false): the setting, the chain state
  // [F][TA_MD_MAX_CHAIN] (zeroed by ta_md_init), the record of the running ta_md_run and the host's copy
  // of the last successful run's chain terms
  bool md_nhc_on = false;
  ta_md_nhc_params md_nhc_p = {0.0, 0.0, 3, 1, 0};
  DevBuf<double> md_nhc_eta, md_nhc_veta, md_nhc_rec;
  bool md_nhc_rec_valid = false;
  std::vector<double> md_rec_chain;  // [n_rec][F]
  // Sampling (ta_md_set_sampling; off while md_samp_on is false): the setting; the rings [L][N][3], the
  // accumulators [2][F][E][L] (v . v, then |dx|^2), the correlation launch's partials and chunk layout; the
  // absolute step of sample 0 (a multiple of sample_every) and of the newest sample (-1: none); whether the
  // data are those of a run that succeeded
  bool md_samp_on = false;
  ta_md_sampling_params md_samp_p = {0, 1};
  DevBuf<double> md_ring_x, md_ring_v, md_corr_acc, md_corr_part;
  DevBuf<int32_t> md_corr_blk;
  int md_corr_chunks = 0;
  int64_t md_samp_origin = 0, md_samp_last = -1;
  bool md_samp_valid = false;
  // Pair distributions (ta_md_set_rdf; off while md_rdf_on is false): the setting; the counts [F][E][E][n_bins],
  // the launch's workgroup layout; the absolute step of sample 0 (a multiple of sample_every) and of the newest
  // sample (-1: none); whether the counts are those of a run that succeeded
  bool md_rdf_on = false;
  ta_md_rdf_params md_rdf_p = {0.0, 0, 1};
  DevBuf<unsigned long long> md_rdf_acc;
  DevBuf<int32_t> md_rdf_blk;
  int md_rdf_n_blk = 0, md_rdf_chunk = 0;
  int64_t md_rdf_origin = 0, md_rdf_last = -1;
  bool md_rdf_valid = false;
  // Langevin (ta_md_set_langevin; off while md_friction == 0): bath, friction, the key of the noise; the
  // steps integrated since ta_md_init (the noise's step counter) and the scratch of ta_md_noise
  double md_lv_kT0 = 0.0, md_friction = 0.0;
  uint64_t md_seed = 0;
  int64_t md_step = 0;
  DevBuf<double> md_noise;
  // Berendsen barostat (ta_md_set_barostat; off while md_baro_on is false): the setting, the cumulative
  // scale of every frame since its list was built with the ones that reset it, the device records
  // {V, P_x, P_y, P_z} of the running ta_md_run and the host's copy of the last successful run's
  bool md_baro_on = false;
  bool md_baro_running = false;  // a barostat run is under way: a rebuild resets the cumulative scale
  ta_md_barostat_params md_baro_p = {0.0, 0.0, 0.0, {1, 1, 1}, 1};
  DevBuf<double> md_baro_scale, md_baro_rec;
  std::vector<double> md_baro_ones;
  bool md_rec_valid = false;
  std::vector<double> md_rec_volume, md_rec_press;  // [n_rec][F], [n_rec][F][3]

  // device-resident relaxation (ta_relax_init / ta_relax_run; the launches are in ta_relax.hip): FIRE
  // velocities of its own, the mask of fixed atoms, the two copies of the per-frame state with the host's
  // image of the current one, the workgroups' partial sums and the count of converged frames. The status
  // words, md_ref and the workgroup layout are the MD loop's.
  bool relax_valid = false;
  ta_fire_params relax_p = {0.1, 1.0, 0.2, 1.1, 0.5, 0.1, 0.99, 5};
  DevBuf<double> relax_vel, relax_part;
  DevBuf<uint8_t> relax_fixed;
  DevBuf<ta::RelaxFrameState> relax_state;
  DevBuf<int> relax_count;
  std::vector<ta::RelaxFrameState> relax_state_host;
  // cell mode of the relaxation (ta_relax_set_cell): h0 and the cell factor of every frame, the deformation
  // gradient and the cell velocity (two copies on the device like relax_state, the current one on the host
  // between runs), the reference cells of the resident list next to md_ref
  bool relax_cell_on = false;
  bool cell_running = false;  // a run that moves the cells (cell relaxation, barostat) is under way: rebuilds take them from the device
  ta_relax_cell_params relax_cell_p = {0.0, 0.0, {1, 1, 1, 1, 1, 1}, 0, 0};
  DevBuf<double> relax_cell_h0, relax_cell_cf, relax_cell_G, relax_cell_vel, relax_cell_fmax2, md_ref_cells;
  std::vector<double> relax_cell_G_host, relax_cell_vel_host;
  // band mode of the relaxation (ta_relax_set_band; the band launches are in ta_neb.hip): the frames are the
  // images of a nudged elastic band and FIRE runs on the band forces with the whole band as ONE pseudo-frame.
  // The band owns its force and tangent arrays, the partials of its two launches, the mask (the user's OR-ed
  // with the two endpoint images), the two copies of the one FIRE record and the pseudo-frame's layout
  // {atom_start[2], blk_start[2], climbing image}.
  bool relax_band_on = false;
  bool relax_band_ran = false;  // a band run left B, tau and the climbing image of the resident state
  ta_band_params relax_band_p = {0.1, 0, 0};
  std::vector<uint8_t> relax_fixed_host;  // the mask of ta_relax_init
  DevBuf<double> band_force, band_tau, band_part;
  DevBuf<uint8_t> band_fixed;
  DevBuf<ta::RelaxFrameState> band_state;
  DevBuf<int32_t> band_layout;
  ta::RelaxFrameState band_state_host = {};
  std::vector<double> band_energy_host;  // [F] image energies of the state the last band run ended on

  hipEvent_t ev[2 * TA_N_KERNEL_SLOTS + 2] = {nullptr};
  std::string err;
};

namespace {

int fail(ta_context *h, int code, const std::string &msg) {
  if (h)
    h->err = msg;
  else
    g_create_error = msg;
  return code;
}

// temperature-dependent models have no analytic Hessian-vector products
std::string td_inference_only(const char *fn) {
  return std::string(fn) + ": not available for finite-temperature (temperature-dependent) models "
         "(no analytic Hessian-vector products)";
}

// eam/fs models evaluate energies, forces and virials only
std::string fs_inference_only(const char *fn) {
  return std::string(fn) + ": not available for eam/fs models (inference only: no weight, constant or loss "
         "gradients and no analytic Hessian-vector products; differences of the forces give the latter)";
}

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
static void dump_stamps(ta_context *h) {
  const std::string &path = h->opt.phase_stamps_out;
  if (path.empty() || !h->db.stamps || h->db.n_blk <= 0) return;
  const size_t n = (size_t)2 * h->db.n_blk * ta::kStampSlots;
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

// The forward launches of the second-generation angular path, one per chunk. `tri`: the backward launches of
// this evaluation are asked to take the triangle build. The full job list is left out only when EVERY one of
// them does (a chunk that falls back to the per-apex kernel reads it), and the handle remembers which.
void forward_v2_launches(ta_context *h, bool tri) {
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

void compute_impl(ta_context *h, uint32_t want, bool timed, double *slot_ms) {
  using namespace ta;
#ifdef TA_PHASE_STAMPS
  if (h->db.n_blk > 0) {
    h->stamp_buf.ensure((size_t)2 * h->db.n_blk * ta::kStampSlots + 8);
    h->db.stamps = h->stamp_buf.ptr;
    (void)hipMemsetAsync(h->db.stamps, 0, (size_t)2 * h->db.n_blk * ta::kStampSlots * sizeof(unsigned long long),
                         h->stream);
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
    const bool tri_cells = (h->relax_cell_on || h->md_baro_on) ? h->tri_cells_wide_ok : h->tri_cells_ok;
    const bool tri = h->use_v2 && h->triangles && tri_cells && h->n_elements == 1 && need_forces;
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

}  // namespace

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
  h->stage_in.release(); h->stage_out.release(); h->inbuf.release(); h->results.release();
  h->rec.release(); h->part4.release(); h->G.release();
  h->dEdG.release(); h->g.release(); h->wat.release(); h->bpart.release(); h->fown.release();
  h->benergy.release(); h->mlp_scratch.release();
  h->train_scratch.release(); h->train_partial.release(); h->train_grad.release(); h->train_coeff.release();
  h->jvp_J.release(); h->tan_dD.release(); h->tan_dG.release(); h->tan_dir.release();
  h->pair_start.release(); h->seg_start.release(); h->pair_i.release(); h->pair_j.release();
  h->pair_shift.release(); h->pair_rev.release();
  for (auto *b : {&h->ex_pair_i, &h->ex_pair_j, &h->ex_pair_shift, &h->ex_pair_rev, &h->ex_pair_start, &h->ex_pair_stop,
                  &h->ex_seg_start, &h->ex_counts, &h->ex_map, &h->ex_blk, &h->ex_slot_q})
    b->release();
  h->ex_hdr.release();
  h->masks.release(); h->job_word.release(); h->job_count.release();
  h->job_word_own.release(); h->job_count_own.release();
  for (auto *b : {&h->nl_wrap, &h->nl_binid, &h->nl_bin_count, &h->nl_bin_start, &h->nl_bin_cursor,
                  &h->nl_bin_atoms, &h->nl_counts})
    b->release();
  h->nl_stats.release();
  h->nl_zero.release();
  h->hvp_buf.release();
  h->filt_scratch.release();
  h->nl_recs.release();
  for (auto *b : {&h->md_mass, &h->md_vel, &h->md_ref, &h->md_epot, &h->md_ke, &h->md_noise, &h->md_nhc_eta,
                  &h->md_nhc_veta, &h->md_nhc_rec, &h->md_ring_x, &h->md_ring_v, &h->md_corr_acc, &h->md_corr_part})
    b->release();
  h->md_corr_blk.release();
  h->md_rdf_acc.release();
  h->md_rdf_blk.release();
  h->md_blk_start.release();
  h->md_status.release();
  h->md_status_host.release();
  h->relax_vel.release();
  h->relax_part.release();
  h->relax_fixed.release();
  h->relax_state.release();
  h->relax_count.release();
  for (auto *b : {&h->band_force, &h->band_tau, &h->band_part}) b->release();
  h->band_fixed.release();
  h->band_state.release();
  h->band_layout.release();
  for (auto *b : {&h->relax_cell_h0, &h->relax_cell_cf, &h->relax_cell_G, &h->relax_cell_vel, &h->relax_cell_fmax2,
                  &h->md_ref_cells})
    b->release();
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
  if (h->kind == TA_MODEL_EAM_ALLOY || h->kind == TA_MODEL_EAM_FS) return ta::eam_is_plain(h->eam);
  return false;
}

void apply_filter(ta_context *h) {
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
// the resident frames again with new coordinates (cells: null = unchanged): the rebuild path of
// ta_update_positions and ta_md_run; throws
void rebuild_list(ta_context *h, const double *positions, const double *cells) {
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
}  // namespace

extern "C" {

int ta_set_frames(ta_handle h, int32_t n_frames, const ta_frame *frames, ta_batch_info *info) {
  if (!h) return TA_ERR_INVALID;
  if (n_frames < 0 || (n_frames > 0 && !frames)) return fail(h, TA_ERR_INVALID, "bad frames argument");
  h->md_valid = false;  // masses and velocities belong to the batch that leaves
  h->relax_valid = false;
  h->relax_cell_on = false;
  h->relax_band_on = h->relax_band_ran = false;
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
    if (cells && h->relax_cell_on && h->relax_valid && F) {
      // the caller's cells replace the relaxed ones: they are h0 from here on, G = I, the cell velocities 0
      HIP_CHECK(hipMemcpy(h->relax_cell_h0.ptr, h->ref_cells.data(), 9 * F * sizeof(double), hipMemcpyHostToDevice));
      h->relax_cell_G_host.assign(9 * F, 0.0);
      for (size_t f = 0; f < F; ++f) h->relax_cell_G_host[9 * f] = h->relax_cell_G_host[9 * f + 4] = h->relax_cell_G_host[9 * f + 8] = 1.0;
      h->relax_cell_vel_host.assign(9 * F, 0.0);
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

namespace {
// workgroups of the integrator launch: `chunk` consecutive atoms of one frame each, at least one per frame
void md_plan_blocks(ta_context *h, int chunk) {
  if (chunk == h->md_chunk && !h->md_blk_start_host.empty()) return;
  const size_t F = h->keep_natoms.size();
  std::vector<int32_t> &start = h->md_blk_start_host;
  start.assign(F + 1, 0);
  for (size_t f = 0; f < F; ++f)
    start[f + 1] = start[f] + std::max(1, (h->keep_natoms[f] + chunk - 1) / chunk);
  h->md_blk_start.ensure(F + 1);
  HIP_CHECK(hipStreamSynchronize(h->stream));  // (an earlier run's launches read the old layout)
  HIP_CHECK(hipMemcpy(h->md_blk_start.ptr, start.data(), (F + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
  h->md_chunk = chunk;
  h->md_n_blk = start[F];
}

// frees what sampling holds on the device; the setting stays
void md_sampling_release(ta_context *h) {
  for (auto *b : {&h->md_ring_x, &h->md_ring_v, &h->md_corr_acc, &h->md_corr_part}) b->release();
  h->md_corr_blk.release();
  h->md_corr_chunks = 0;
  h->md_samp_valid = false;
  h->md_samp_last = -1;
}

// exactly n elements (the ring may take gigabytes: no head room); false when the device has no room
extern "C++" template <typename T>
bool md_alloc_exact(DevBuf<T> &b, size_t n) {
  b.release();
  T *fresh = nullptr;
  if (hipMalloc((void **)&fresh, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  b.ptr = fresh;
  b.cap = std::max<size_t>(n, 1);
  return true;
}

// Rings, zeroed accumulators and the correlation launch's chunk layout for the resident batch under setting
// `p`, with no sample held: sample 0 will be the first multiple of sample_every at or behind the steps
// integrated so far. False when the device has no room (everything is released then); throws otherwise.
bool md_sampling_alloc(ta_context *h, const ta_md_sampling_params &p) {
  const size_t N = h->keep_species.size(), F = h->keep_natoms.size();
  const size_t L = (size_t)p.n_lags, E = (size_t)h->n_elements;
  HIP_CHECK(hipStreamSynchronize(h->stream));  // (an earlier run's launches read the old buffers)
  md_sampling_release(h);
  std::vector<int32_t> start(F + 1, 0);
  for (size_t f = 0; f < F; ++f)
    start[f + 1] = start[f] + std::max(1, (3 * h->keep_natoms[f] + ta::kMdCorrChunk - 1) / ta::kMdCorrChunk);
  const size_t n_chunks = (size_t)start[F], n_acc = 2 * F * E * L;
  if (!md_alloc_exact(h->md_ring_x, L * 3 * N) || !md_alloc_exact(h->md_ring_v, L * 3 * N) ||
      !md_alloc_exact(h->md_corr_acc, n_acc) || !md_alloc_exact(h->md_corr_part, n_chunks * 2 * E * L) ||
      !md_alloc_exact(h->md_corr_blk, F + 1)) {
    md_sampling_release(h);
    return false;
  }
  HIP_CHECK(hipMemset(h->md_corr_acc.ptr, 0, std::max<size_t>(n_acc, 1) * sizeof(double)));
  HIP_CHECK(hipMemcpy(h->md_corr_blk.ptr, start.data(), (F + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
  h->md_corr_chunks = (int)n_chunks;
  const int64_t s = p.sample_every;
  h->md_samp_origin = (h->md_step + s - 1) / s * s;
  h->md_samp_last = -1;
  h->md_samp_valid = true;
  return true;
}

// frees what the pair distributions hold on the device; the setting stays
void md_rdf_release(ta_context *h) {
  h->md_rdf_acc.release();
  h->md_rdf_blk.release();
  h->md_rdf_n_blk = 0;
  h->md_rdf_valid = false;
  h->md_rdf_last = -1;
}

// Zeroed counts and the launch's workgroup layout for the resident batch under setting `p`, with no sample
// taken: sample 0 will be the first multiple of sample_every at or behind the steps integrated so far. False
// when the device has no room (everything is released then); throws otherwise.
bool md_rdf_alloc(ta_context *h, const ta_md_rdf_params &p) {
  const size_t N = h->keep_species.size(), F = h->keep_natoms.size();
  const size_t E = (size_t)h->n_elements, n_acc = F * E * E * (size_t)p.n_bins;
  HIP_CHECK(hipStreamSynchronize(h->stream));  // (an earlier run's launches add to the old buffer)
  md_rdf_release(h);
  const int chunk = ta::md_rdf_chunk((long long)N);
  std::vector<int32_t> start(F + 1, 0);
  for (size_t f = 0; f < F; ++f) start[f + 1] = start[f] + std::max(1, (h->keep_natoms[f] + chunk - 1) / chunk);
  if (!md_alloc_exact(h->md_rdf_acc, n_acc) || !md_alloc_exact(h->md_rdf_blk, F + 1)) {
    md_rdf_release(h);
    return false;
  }
  HIP_CHECK(hipMemset(h->md_rdf_acc.ptr, 0, std::max<size_t>(n_acc, 1) * sizeof(unsigned long long)));
  HIP_CHECK(hipMemcpy(h->md_rdf_blk.ptr, start.data(), (F + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
  h->md_rdf_n_blk = (int)start[F];
  h->md_rdf_chunk = chunk;
  const int64_t s = p.sample_every;
  h->md_rdf_origin = (h->md_step + s - 1) / s * s;
  h->md_rdf_last = -1;
  h->md_rdf_valid = true;
  return true;
}

// The loop that ta_md_run and ta_relax_run share. `enqueue(q)` puts the launches of step q on the stream
// (they are predicated on the status word and test the skin / 2 rule after their drift); this loop follows
// each with the exact list of the step and an evaluation, looks at the page-locked status word every
// kMdLookahead steps, and where a drift left the list stale rebuilds it from the device's positions and
// goes on behind that step. After a look that found the list valid, `finished(k, k_end)` may name the step
// in [k, k_end) from which on the launches moved nothing (-1: none): the loop ends there. Returns the
// steps done; F of the state at entry must be resident. `*rebuilds` counts the lists built, `*n_rebuilds`
// (may be null) follows it so that a run that fails reports what it did. Throws.
extern "C++" template <class Enqueue, class Finished>
int resident_steps(ta_context *h, const char *who, int n_steps, uint32_t want, Enqueue &&enqueue,
                   Finished &&finished, int *rebuilds, int32_t *n_rebuilds) {
  const size_t N = h->keep_species.size();
  hipStream_t s = h->stream;
  volatile unsigned *status_host = reinterpret_cast<volatile unsigned *>(h->md_status_host.ptr);
  const int look = h->skin > 0.0 ? ta::kMdLookahead : 1;
  std::vector<double> x, cells;
  const size_t F = h->keep_natoms.size();
  int k = 0;
  while (k < n_steps) {
    // steps k .. k_end - 1 without a look at the device: integrator, exact list of the step, evaluation
    const int k_end = (int)std::min<int64_t>(n_steps, (int64_t)k + look);
    for (int q = k; q < k_end; ++q) {
      enqueue(q);
      if (h->filtered) apply_filter(h);
      compute_impl(h, want, false, nullptr);
    }
    wait_stream(s, h->opt);
    h->upload_pending = false;
    const unsigned mark = status_host[0];
    if (mark == 0u) {
      const int fin = finished(k, k_end);
      if (fin >= 0) {
        h->n_list_reuses += fin - k;
        return fin;
      }
      h->n_list_reuses += k_end - k;
      k = k_end;
      continue;
    }
    // the drift of step q left the list stale: the launches behind it did nothing, the evaluations
    // behind it ran on the stale list and are overwritten now
    const int q = (int)mark - 1;
    if (q < k || q >= k_end) throw std::runtime_error(std::string(who) + ": inconsistent status word");
    h->n_list_reuses += q - k;
    x.resize(3 * N);
    if (N) HIP_CHECK(hipMemcpy(x.data(), h->db.pos, 3 * N * sizeof(double), hipMemcpyDeviceToHost));
    if (h->cell_running) {  // the cells moved on the device: ref_cells are those of the stale list
      cells.resize(9 * F);
      if (F) HIP_CHECK(hipMemcpy(cells.data(), h->db.cells, 9 * F * sizeof(double), hipMemcpyDeviceToHost));
      if (h->md_baro_running) {  // a scale factor that was no finite number > 0 left NaNs in its frame's cell
        for (size_t f = 0; f < F; ++f) {
          bool ok = true;
          for (int c = 0; c < 9; ++c) ok = ok && std::isfinite(cells[9 * f + c]);
          if (!ok) {
            h->have_batch = false;  // (positions and cells of the frame are lost)
            h->md_valid = false;
            throw std::invalid_argument(std::string(who) + ": the barostat's scale factor of frame " + std::to_string(f) +
                                        " at step " + std::to_string(q + 1) + " is not a finite number > 0");
          }
        }
      }
    }
    status_host[0] = 0u;
    HIP_CHECK(hipMemsetAsync(h->md_status.ptr, 0, 2 * sizeof(unsigned), s));
    try {
      rebuild_list(h, x.data(), h->cell_running ? cells.data() : nullptr);
    } catch (const HipError &e) {
      throw HipError(std::string(who) + ": list rebuild after step " + std::to_string(q + 1) + " failed: " + e.what());
    } catch (const std::exception &e) {
      throw std::runtime_error(std::string(who) + ": list rebuild after step " + std::to_string(q + 1) +
                               " failed: " + e.what());
    }
    if (N) HIP_CHECK(hipMemcpyAsync(h->md_ref.ptr, h->db.pos, 3 * N * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (h->cell_running && F) {
      if (h->md_baro_running)  // the barostat keeps the scale since the build, not the list's cells
        HIP_CHECK(hipMemcpyAsync(h->md_baro_scale.ptr, h->md_baro_ones.data(), 3 * F * sizeof(double), hipMemcpyHostToDevice, s));
      else
        HIP_CHECK(hipMemcpyAsync(h->md_ref_cells.ptr, h->db.cells, 9 * F * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    h->md_ref_builds = h->n_list_builds;
    compute_impl(h, want, false, nullptr);
    ++*rebuilds;
    if (n_rebuilds) *n_rebuilds = *rebuilds;
    k = q + 1;
  }
  return n_steps;
}
}  // namespace

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
  bool ring_nomem = false, rdf_nomem = false;
  const int rc = guarded(h, [&]() {
    h->md_valid = false;
    HIP_CHECK(hipStreamSynchronize(h->stream));
    h->upload_pending = false;
    h->md_mass.ensure(N + 1);
    h->md_vel.ensure(3 * N + 1);
    h->md_ref.ensure(3 * N + 1);
    h->md_status.ensure(2);
    h->md_status_host.ensure(64);
    const size_t n_chain = h->keep_natoms.size() * ta::kMdMaxChain;  // every frame's chain starts at rest
    h->md_nhc_eta.ensure(n_chain + 1);
    h->md_nhc_veta.ensure(n_chain + 1);
    HIP_CHECK(hipMemset(h->md_nhc_eta.ptr, 0, (n_chain + 1) * sizeof(double)));
    HIP_CHECK(hipMemset(h->md_nhc_veta.ptr, 0, (n_chain + 1) * sizeof(double)));
    h->md_nhc_rec_valid = false;
    if (N) {
      HIP_CHECK(hipMemcpy(h->md_mass.ptr, masses, N * sizeof(double), hipMemcpyHostToDevice));
      if (velocities)
        HIP_CHECK(hipMemcpy(h->md_vel.ptr, velocities, 3 * N * sizeof(double), hipMemcpyHostToDevice));
      else
        HIP_CHECK(hipMemset(h->md_vel.ptr, 0, 3 * N * sizeof(double)));
    }
    h->md_ref_builds = -1;  // ta_md_run uploads ref_pos
    h->md_chunk = 0;
    h->md_blk_start_host.clear();
    h->md_step = 0;
    h->md_rec_valid = false;
    if (h->md_samp_on && !md_sampling_alloc(h, h->md_samp_p)) {  // an empty ring for this batch, or none
      h->md_samp_on = false;
      ring_nomem = true;
    }
    if (h->md_rdf_on && !md_rdf_alloc(h, h->md_rdf_p)) {  // zero counts for this batch, or none
      h->md_rdf_on = false;
      rdf_nomem = true;
    }
    h->md_valid = true;
  });
  if (rc == TA_OK && ring_nomem)
    return fail(h, TA_ERR_NOMEM, "ta_md_init: no device memory for the rings of ta_md_set_sampling; sampling is off");
  if (rc == TA_OK && rdf_nomem)
    return fail(h, TA_ERR_NOMEM, "ta_md_init: no device memory for the counts of ta_md_set_rdf; the feature is off");
  return rc;
}

int ta_md_set_thermostat(ta_handle h, double kT0, double tau) {
  if (!h) return TA_ERR_INVALID;
  if (std::isnan(kT0) || std::isinf(kT0)) return fail(h, TA_ERR_INVALID, "ta_md_set_thermostat: kT0 must be finite");
  if (kT0 > 0.0 && (!(tau > 0.0) || !std::isfinite(tau)))
    return fail(h, TA_ERR_INVALID, "ta_md_set_thermostat: tau must be a finite time > 0");
  if (kT0 > 0.0 && h->md_friction > 0.0)
    return fail(h, TA_ERR_INVALID, "ta_md_set_thermostat: the Langevin thermostat is on; switch it off "
                                   "(ta_md_set_langevin with friction 0) before the Berendsen thermostat goes on");
  if (kT0 > 0.0 && h->md_nhc_on)
    return fail(h, TA_ERR_INVALID, "ta_md_set_thermostat: the Nose-Hoover chain thermostat is on; switch it off "
                                   "(ta_md_set_nose_hoover with NULL) before the Berendsen thermostat goes on");
  h->md_kT0 = kT0 > 0.0 ? kT0 : 0.0;
  h->md_tau = kT0 > 0.0 ? tau : 0.0;
  return TA_OK;
}

int ta_md_set_langevin(ta_handle h, double kT0, double friction, uint64_t seed) {
  if (!h) return TA_ERR_INVALID;
  if (!(friction >= 0.0) || !std::isfinite(friction))
    return fail(h, TA_ERR_INVALID, "ta_md_set_langevin: friction must be a finite rate >= 0");
  if (!(kT0 >= 0.0) || !std::isfinite(kT0))
    return fail(h, TA_ERR_INVALID, "ta_md_set_langevin: kT0 must be finite and >= 0");
  if (friction > 0.0 && h->md_kT0 > 0.0)
    return fail(h, TA_ERR_INVALID, "ta_md_set_langevin: the Berendsen thermostat is on; switch it off "
                                   "(ta_md_set_thermostat with kT0 0) before the Langevin thermostat goes on");
  if (friction > 0.0 && h->md_nhc_on)
    return fail(h, TA_ERR_INVALID, "ta_md_set_langevin: the Nose-Hoover chain thermostat is on; switch it off "
                                   "(ta_md_set_nose_hoover with NULL) before the Langevin thermostat goes on");
  h->md_friction = friction;
  h->md_lv_kT0 = friction > 0.0 ? kT0 : 0.0;
  h->md_seed = seed;
  return TA_OK;
}

int ta_md_set_nose_hoover(ta_handle h, const ta_md_nhc_params *p) {
  if (!h) return TA_ERR_INVALID;
  if (p && std::isnan(p->kT0)) return fail(h, TA_ERR_INVALID, "ta_md_set_nose_hoover: kT0 must be finite");
  if (!p || !(p->kT0 > 0.0)) {
    h->md_nhc_on = false;
    return TA_OK;
  }
  if (!std::isfinite(p->kT0)) return fail(h, TA_ERR_INVALID, "ta_md_set_nose_hoover: kT0 must be finite");
  if (!(p->tau > 0.0) || !std::isfinite(p->tau))
    return fail(h, TA_ERR_INVALID, "ta_md_set_nose_hoover: tau must be a finite time > 0");
  if (p->chain < 1 || p->chain > TA_MD_MAX_CHAIN)
    return fail(h, TA_ERR_INVALID, "ta_md_set_nose_hoover: chain must be 1 .. " + std::to_string(TA_MD_MAX_CHAIN));
  if (p->loops < 1 || p->loops > 16) return fail(h, TA_ERR_INVALID, "ta_md_set_nose_hoover: loops must be 1 .. 16");
  if (p->dof_removed < 0) return fail(h, TA_ERR_INVALID, "ta_md_set_nose_hoover: dof_removed must be >= 0");
  if (h->md_kT0 > 0.0)
    return fail(h, TA_ERR_INVALID, "ta_md_set_nose_hoover: the Berendsen thermostat is on; switch it off "
                                   "(ta_md_set_thermostat with kT0 0) before the Nose-Hoover chain goes on");
  if (h->md_friction > 0.0)
    return fail(h, TA_ERR_INVALID, "ta_md_set_nose_hoover: the Langevin thermostat is on; switch it off "
                                   "(ta_md_set_langevin with friction 0) before the Nose-Hoover chain goes on");
  if (h->md_nhc_on && h->md_nhc_p.chain != p->chain && h->md_valid) {
    // another chain length: the slots beyond the old one hold nothing, the chain starts again at rest
    const size_t n_chain = h->keep_natoms.size() * ta::kMdMaxChain;
    const int rc = guarded(h, [&]() {
      HIP_CHECK(hipStreamSynchronize(h->stream));
      HIP_CHECK(hipMemset(h->md_nhc_eta.ptr, 0, (n_chain + 1) * sizeof(double)));
      HIP_CHECK(hipMemset(h->md_nhc_veta.ptr, 0, (n_chain + 1) * sizeof(double)));
    });
    if (rc != TA_OK) return rc;
  }
  h->md_nhc_p = *p;
  h->md_nhc_on = true;
  return TA_OK;
}

namespace {
// what ta_md_get_chain and ta_md_set_chain need; returns 0 or the error code
int md_chain_ready(ta_context *h, const char *who) {
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, std::string(who) + ": no resident batch");
  if (!h->md_valid) return fail(h, TA_ERR_INVALID, std::string(who) + " called before ta_md_init");
  if (!h->md_nhc_on)
    return fail(h, TA_ERR_INVALID, std::string(who) + ": the Nose-Hoover chain thermostat is off (ta_md_set_nose_hoover)");
  return TA_OK;
}
}  // namespace

int ta_md_get_chain(ta_handle h, double *eta, double *veta) {
  if (!h) return TA_ERR_INVALID;
  if (const int rc = md_chain_ready(h, "ta_md_get_chain")) return rc;
  return guarded(h, [&]() {
    const size_t F = h->keep_natoms.size(), M = (size_t)h->md_nhc_p.chain;
    HIP_CHECK(hipStreamSynchronize(h->stream));
    std::vector<double> buf(F * ta::kMdMaxChain);
    for (int w = 0; w < 2; ++w) {
      double *out = w ? veta : eta;
      if (!out || !F) continue;
      HIP_CHECK(hipMemcpy(buf.data(), w ? h->md_nhc_veta.ptr : h->md_nhc_eta.ptr, buf.size() * sizeof(double),
                          hipMemcpyDeviceToHost));
      for (size_t f = 0; f < F; ++f)
        for (size_t k = 0; k < M; ++k) out[f * M + k] = buf[f * ta::kMdMaxChain + k];
    }
  });
}

int ta_md_set_chain(ta_handle h, const double *eta, const double *veta) {
  if (!h) return TA_ERR_INVALID;
  if (const int rc = md_chain_ready(h, "ta_md_set_chain")) return rc;
  const size_t F = h->keep_natoms.size(), M = (size_t)h->md_nhc_p.chain;
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
      HIP_CHECK(hipMemcpy(w ? h->md_nhc_veta.ptr : h->md_nhc_eta.ptr, buf.data(), buf.size() * sizeof(double),
                          hipMemcpyHostToDevice));
    }
  });
}

int ta_md_get_chain_records(ta_handle h, double *e_chain) {
  if (!h) return TA_ERR_INVALID;
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "ta_md_get_chain_records: no resident batch");
  if (!h->md_valid) return fail(h, TA_ERR_INVALID, "ta_md_get_chain_records called before ta_md_init");
  if (!h->md_nhc_rec_valid)
    return fail(h, TA_ERR_INVALID, "ta_md_get_chain_records: the last ta_md_run of this batch had no Nose-Hoover chain");
  if (e_chain && !h->md_rec_chain.empty())
    std::memcpy(e_chain, h->md_rec_chain.data(), h->md_rec_chain.size() * sizeof(double));
  return TA_OK;
}

int ta_md_set_sampling(ta_handle h, const ta_md_sampling_params *p) {
  if (!h) return TA_ERR_INVALID;
  if (!p || p->n_lags == 0) {
    h->md_samp_on = false;
    return guarded(h, [&]() {
      HIP_CHECK(hipStreamSynchronize(h->stream));
      md_sampling_release(h);
    });
  }
  if (p->n_lags < 0 || p->n_lags > TA_MD_MAX_LAGS)
    return fail(h, TA_ERR_INVALID, "ta_md_set_sampling: n_lags must be 0 .. " + std::to_string(TA_MD_MAX_LAGS));
  if (p->sample_every < 1) return fail(h, TA_ERR_INVALID, "ta_md_set_sampling: sample_every must be >= 1");
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "ta_md_set_sampling: no resident batch");
  if (!h->md_valid) return fail(h, TA_ERR_INVALID, "ta_md_set_sampling called before ta_md_init");
  bool nomem = false;
  const int rc = guarded(h, [&]() {
    h->md_samp_on = false;  // (until the rings exist)
    nomem = !md_sampling_alloc(h, *p);
    if (!nomem) {
      h->md_samp_p = *p;
      h->md_samp_on = true;
    }
  });
  if (rc == TA_OK && nomem)
    return fail(h, TA_ERR_NOMEM, "ta_md_set_sampling: no device memory for rings of n_lags = " + std::to_string(p->n_lags) +
                                 " snapshots; sampling is off");
  return rc;
}

namespace {
// what the two getters of the sampled data need; returns 0 or the error code
int md_samples_ready(ta_context *h, const char *who) {
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, std::string(who) + ": no resident batch");
  if (!h->md_valid) return fail(h, TA_ERR_INVALID, std::string(who) + " called before ta_md_init");
  if (!h->md_samp_on) return fail(h, TA_ERR_INVALID, std::string(who) + ": sampling is off (ta_md_set_sampling)");
  if (!h->md_samp_valid)
    return fail(h, TA_ERR_INVALID, std::string(who) + ": a ta_md_run failed and left the sampled data invalid; call "
                                   "ta_md_set_sampling or ta_md_init again");
  return TA_OK;
}

int64_t md_samples_taken(const ta_context *h) {
  return h->md_samp_last < 0 ? 0 : (h->md_samp_last - h->md_samp_origin) / h->md_samp_p.sample_every + 1;
}
}  // namespace

int ta_md_get_correlations(ta_handle h, double *vacf_sum, double *msd_sum, int64_t *info) {
  if (!h) return TA_ERR_INVALID;
  if (const int rc = md_samples_ready(h, "ta_md_get_correlations")) return rc;
  return guarded(h, [&]() {
    const size_t n = h->keep_natoms.size() * (size_t)h->n_elements * (size_t)h->md_samp_p.n_lags;
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (vacf_sum && n) HIP_CHECK(hipMemcpy(vacf_sum, h->md_corr_acc.ptr, n * sizeof(double), hipMemcpyDeviceToHost));
    if (msd_sum && n) HIP_CHECK(hipMemcpy(msd_sum, h->md_corr_acc.ptr + n, n * sizeof(double), hipMemcpyDeviceToHost));
    if (info) {
      info[0] = md_samples_taken(h);
      info[1] = h->md_samp_p.n_lags;
      info[2] = h->md_samp_p.sample_every;
      info[3] = h->md_samp_last;
    }
  });
}

int ta_md_get_samples(ta_handle h, int32_t first_lag, int32_t n, double *positions, double *velocities,
                      int64_t *steps) {
  if (!h) return TA_ERR_INVALID;
  if (const int rc = md_samples_ready(h, "ta_md_get_samples")) return rc;
  const int64_t taken = md_samples_taken(h), L = h->md_samp_p.n_lags, held = std::min(taken, L);
  if (first_lag < 0) return fail(h, TA_ERR_INVALID, "ta_md_get_samples: first_lag must be >= 0");
  if (n < 0) return fail(h, TA_ERR_INVALID, "ta_md_get_samples: n must be >= 0");
  if ((int64_t)first_lag + n > held)
    return fail(h, TA_ERR_INVALID, "ta_md_get_samples: first_lag + n = " + std::to_string((int64_t)first_lag + n) +
                                   " exceeds the " + std::to_string(held) + " snapshots held (min(n_samples, n_lags))");
  return guarded(h, [&]() {
    const size_t row = 3 * h->keep_species.size();
    HIP_CHECK(hipStreamSynchronize(h->stream));
    for (int32_t j = 0; j < n; ++j) {
      const int64_t idx = taken - 1 - first_lag - j;  // sample number
      const size_t slot = (size_t)(idx % L);
      if (positions && row)
        HIP_CHECK(hipMemcpy(positions + (size_t)j * row, h->md_ring_x.ptr + slot * row, row * sizeof(double), hipMemcpyDeviceToHost));
      if (velocities && row)
        HIP_CHECK(hipMemcpy(velocities + (size_t)j * row, h->md_ring_v.ptr + slot * row, row * sizeof(double), hipMemcpyDeviceToHost));
      if (steps) steps[j] = h->md_samp_origin + idx * h->md_samp_p.sample_every;
    }
  });
}

int ta_md_set_rdf(ta_handle h, const ta_md_rdf_params *p) {
  if (!h) return TA_ERR_INVALID;
  if (!p || p->n_bins == 0) {
    h->md_rdf_on = false;
    return guarded(h, [&]() {
      HIP_CHECK(hipStreamSynchronize(h->stream));
      md_rdf_release(h);
    });
  }
  if (p->n_bins < 0 || p->n_bins > TA_MD_MAX_BINS)
    return fail(h, TA_ERR_INVALID, "ta_md_set_rdf: n_bins must be 0 .. " + std::to_string(TA_MD_MAX_BINS));
  if (p->sample_every < 1) return fail(h, TA_ERR_INVALID, "ta_md_set_rdf: sample_every must be >= 1");
  if (!std::isfinite(p->r_max) || !(p->r_max > 0.0))
    return fail(h, TA_ERR_INVALID, "ta_md_set_rdf: r_max must be a finite distance > 0");
  if (p->r_max > h->rmax)
    return fail(h, TA_ERR_INVALID, "ta_md_set_rdf: r_max = " + std::to_string(p->r_max) + " exceeds the model's cutoff max(rcut, acut) = " +
                                   std::to_string(h->rmax) + "; the neighbour list is not complete beyond that");
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "ta_md_set_rdf: no resident batch");
  if (!h->md_valid) return fail(h, TA_ERR_INVALID, "ta_md_set_rdf called before ta_md_init");
  bool nomem = false;
  const int rc = guarded(h, [&]() {
    h->md_rdf_on = false;  // (until the counts exist)
    nomem = !md_rdf_alloc(h, *p);
    if (!nomem) {
      h->md_rdf_p = *p;
      h->md_rdf_on = true;
    }
  });
  if (rc == TA_OK && nomem)
    return fail(h, TA_ERR_NOMEM, "ta_md_set_rdf: no device memory for counts of n_bins = " + std::to_string(p->n_bins) +
                                 "; the feature is off");
  return rc;
}

int ta_md_get_rdf(ta_handle h, int64_t *counts, int64_t *info, double *r_max) {
  if (!h) return TA_ERR_INVALID;
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "ta_md_get_rdf: no resident batch");
  if (!h->md_valid) return fail(h, TA_ERR_INVALID, "ta_md_get_rdf called before ta_md_init");
  if (!h->md_rdf_on) return fail(h, TA_ERR_INVALID, "ta_md_get_rdf: the pair distributions are off (ta_md_set_rdf)");
  if (!h->md_rdf_valid)
    return fail(h, TA_ERR_INVALID, "ta_md_get_rdf: a ta_md_run failed and left the counts invalid; call ta_md_set_rdf or "
                                   "ta_md_init again");
  return guarded(h, [&]() {
    const size_t E = (size_t)h->n_elements, n = h->keep_natoms.size() * E * E * (size_t)h->md_rdf_p.n_bins;
    HIP_CHECK(hipStreamSynchronize(h->stream));
    static_assert(sizeof(int64_t) == sizeof(unsigned long long), "the counts are copied as they are");
    if (counts && n) HIP_CHECK(hipMemcpy(counts, h->md_rdf_acc.ptr, n * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (info) {
      info[0] = h->md_rdf_last < 0 ? 0 : (h->md_rdf_last - h->md_rdf_origin) / h->md_rdf_p.sample_every + 1;
      info[1] = h->md_rdf_p.n_bins;
      info[2] = h->md_rdf_p.sample_every;
      info[3] = h->md_rdf_last;
    }
    if (r_max) *r_max = h->md_rdf_p.r_max;
  });
}

int ta_md_noise(ta_handle h, int64_t step, double *xi, double *eta) {
  if (!h) return TA_ERR_INVALID;
  if (!xi || !eta) return fail(h, TA_ERR_INVALID, "ta_md_noise: null argument");
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "ta_md_noise: no resident batch");
  if (!h->md_valid) return fail(h, TA_ERR_INVALID, "ta_md_noise called before ta_md_init");
  if (step < 0) return fail(h, TA_ERR_INVALID, "ta_md_noise: step must be >= 0");
  return guarded(h, [&]() {
    const size_t N = h->keep_species.size();
    if (!N) return;
    h->md_noise.ensure(6 * N);
    ta::launch_md_noise(h->md_seed, step, (long long)N, h->md_noise.ptr, h->md_noise.ptr + 3 * N, h->stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(h->stream));
    HIP_CHECK(hipMemcpy(xi, h->md_noise.ptr, 3 * N * sizeof(double), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(eta, h->md_noise.ptr + 3 * N, 3 * N * sizeof(double), hipMemcpyDeviceToHost));
  });
}

int ta_md_set_barostat(ta_handle h, const ta_md_barostat_params *p) {
  if (!h) return TA_ERR_INVALID;
  if (p && !std::isfinite(p->taup)) return fail(h, TA_ERR_INVALID, "ta_md_set_barostat: taup must be finite");
  if (!p || !(p->taup > 0.0)) {
    h->md_baro_on = false;
    return TA_OK;
  }
  if (!std::isfinite(p->pressure)) return fail(h, TA_ERR_INVALID, "ta_md_set_barostat: pressure must be finite");
  if (!std::isfinite(p->compressibility) || p->compressibility < 0.0)
    return fail(h, TA_ERR_INVALID, "ta_md_set_barostat: compressibility must be finite and >= 0");
  if (!p->isotropic && !p->mask[0] && !p->mask[1] && !p->mask[2])
    return fail(h, TA_ERR_INVALID, "ta_md_set_barostat: mask leaves no axis of the cell free");
  h->md_baro_p = *p;
  h->md_baro_on = true;
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
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "ta_md_get_records: no resident batch");
  if (!h->md_valid) return fail(h, TA_ERR_INVALID, "ta_md_get_records called before ta_md_init");
  if (!h->md_rec_valid)
    return fail(h, TA_ERR_INVALID, "ta_md_get_records: the last ta_md_run of this batch had no barostat");
  if (volume && !h->md_rec_volume.empty())
    std::memcpy(volume, h->md_rec_volume.data(), h->md_rec_volume.size() * sizeof(double));
  if (press && !h->md_rec_press.empty())
    std::memcpy(press, h->md_rec_press.data(), h->md_rec_press.size() * sizeof(double));
  return TA_OK;
}

int ta_md_run(ta_handle h, int32_t n_steps, double dt, uint32_t want, int32_t record_every, double *epot,
              double *ekin, int32_t *n_rebuilds) {
  if (!h) return TA_ERR_INVALID;
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "ta_md_run: no resident batch");
  if (!h->md_valid) return fail(h, TA_ERR_INVALID, "ta_md_run called before ta_md_init (ta_set_frames drops the MD state)");
  if (n_steps < 0 || record_every < 1) return fail(h, TA_ERR_INVALID, "ta_md_run: n_steps >= 0 and record_every >= 1 are needed");
  if (!std::isfinite(dt)) return fail(h, TA_ERR_INVALID, "ta_md_run: dt must be finite");
  if (h->md_friction > 0.0 && dt < 0.0) return fail(h, TA_ERR_INVALID, "ta_md_run: Langevin dynamics needs dt >= 0");
  const bool baro = h->md_baro_on;
  if (baro) {
    const size_t F = h->keep_natoms.size();
    for (size_t f = 0; f < F; ++f) {
      for (int k = 0; k < 3; ++k)
        if (!h->keep_pbc[3 * f + k])
          return fail(h, TA_ERR_INVALID, "ta_md_run: the barostat is on and frame " + std::to_string(f) +
                                         " is not periodic along all three axes");
      const double *c = h->ref_cells.data() + 9 * f;
      const double det = c[0] * (c[4] * c[8] - c[5] * c[7]) - c[1] * (c[3] * c[8] - c[5] * c[6]) + c[2] * (c[3] * c[7] - c[4] * c[6]);
      if (!std::isfinite(det) || !(std::fabs(det) > 0.0))
        return fail(h, TA_ERR_INVALID, "ta_md_run: the barostat is on and the cell of frame " + std::to_string(f) + " is singular");
    }
  }
  const bool nhc = h->md_nhc_on;
  if (nhc) {
    const size_t F = h->keep_natoms.size();
    for (size_t f = 0; f < F; ++f)
      if (3 * (int64_t)h->keep_natoms[f] - (int64_t)h->md_nhc_p.dof_removed < 1)
        return fail(h, TA_ERR_INVALID, "ta_md_run: the Nose-Hoover chain is on and frame " + std::to_string(f) +
                                       " has fewer than one degree of freedom (3 n_atoms - dof_removed)");
  }
  const bool samp = h->md_samp_on;
  if (samp && baro)
    return fail(h, TA_ERR_INVALID, "ta_md_run: sampling (ta_md_set_sampling) and the barostat (ta_md_set_barostat) are both "
                                   "on; displacements in a moving cell are not defined: switch one of them off");
  const bool rdf = h->md_rdf_on;
  if (rdf && baro)
    return fail(h, TA_ERR_INVALID, "ta_md_run: the pair distributions (ta_md_set_rdf) and the barostat (ta_md_set_barostat) are "
                                   "both on; normalising the counts needs one volume: switch one of them off");
  if (n_rebuilds) *n_rebuilds = 0;
  want |= TA_WANT_ENERGY | TA_WANT_FORCES;
  want &= ~(uint32_t)TA_WANT_REUSE_DESCRIPTORS;
  if (baro) want |= TA_WANT_VIRIAL;  // the pressure
  h->md_rec_valid = false;
  h->md_nhc_rec_valid = false;
  const bool samp_was_valid = h->md_samp_valid;
  h->md_samp_valid = false;  // (until this run has succeeded)
  const bool rdf_was_valid = h->md_rdf_valid;
  h->md_rdf_valid = false;
  h->cell_running = h->md_baro_running = baro;
  const int rc = guarded(h, [&]() {
    const size_t N = h->keep_species.size(), F = h->keep_natoms.size();
    hipStream_t s = h->stream;
    const bool thermostat = h->md_kT0 > 0.0, langevin = h->md_friction > 0.0;  // (never both)
    // with Berendsen scaling one workgroup owns a whole frame: the factor needs the frame's kinetic energy
    // (the barostat: the frame's three sums of m v_c^2; the Nose-Hoover chain: the kinetic energy again)
    int chunk = ta::kMdChunk;
    if (thermostat || baro || nhc)
      for (size_t f = 0; f < F; ++f) chunk = std::max(chunk, h->keep_natoms[f]);
    const int threads = (thermostat || baro || nhc) ? 1024 : 256;
    md_plan_blocks(h, chunk);
    const size_t n_blk = (size_t)h->md_n_blk, n_rec = (size_t)(n_steps / record_every) + 1;
    h->md_epot.ensure(n_rec * F + 1);
    h->md_ke.ensure(n_rec * n_blk + 1);
    if (nhc) h->md_nhc_rec.ensure(n_rec * F + 1);
    const std::vector<double> cells_at_entry(baro ? h->ref_cells : std::vector<double>());
    if (baro) {  // every run starts on a list built for the resident cells: the cumulative scale is 1
      h->md_baro_rec.ensure(4 * n_rec * F + 1);
      h->md_baro_scale.ensure(3 * F + 1);
      h->md_baro_ones.assign(3 * F, 1.0);
      HIP_CHECK(hipStreamSynchronize(s));
      if (F) HIP_CHECK(hipMemcpy(h->md_baro_scale.ptr, h->md_baro_ones.data(), 3 * F * sizeof(double), hipMemcpyHostToDevice));
    }
    if (h->md_ref_builds != h->n_list_builds) {  // the host built the list that is resident: its positions go up once
      HIP_CHECK(hipStreamSynchronize(s));
      if (N) HIP_CHECK(hipMemcpy(h->md_ref.ptr, h->ref_pos.data(), 3 * N * sizeof(double), hipMemcpyHostToDevice));
      h->md_ref_builds = h->n_list_builds;
    }
    volatile unsigned *status_host = reinterpret_cast<volatile unsigned *>(h->md_status_host.ptr);
    status_host[0] = 0u;  // (no launch that writes it is in flight: every run ends with a wait)
    HIP_CHECK(hipMemsetAsync(h->md_status.ptr, 0, 2 * sizeof(unsigned), s));

    ta::MdLaunch a;
    a.vel = h->md_vel.ptr;
    a.mass = h->md_mass.ptr;
    a.ref = h->md_ref.ptr;
    a.blk_start = h->md_blk_start.ptr;
    a.epot = h->md_epot.ptr;
    a.ke_part = h->md_ke.ptr;
    a.status = h->md_status.ptr;
    a.status_host = const_cast<unsigned *>(status_host);
    a.dt = dt;
    a.kT0 = langevin ? h->md_lv_kT0 : h->md_kT0;
    a.dt_over_tau = thermostat ? dt / h->md_tau : 0.0;
    a.langevin = langevin ? 1 : 0;
    a.seed = h->md_seed;
    a.c1 = a.c2 = a.c3 = a.c4 = a.c5 = 0.0;
    if (langevin) {  // ASE's Langevin.updatevars with sigma_i = sqrt(2 kT0 fr) / sqrt(m_i)
      const double fr = h->md_friction, sigma = std::sqrt(2.0 * h->md_lv_kT0 * fr);
      a.c1 = dt / 2.0 - dt * dt * fr / 8.0;
      a.c2 = dt * fr / 2.0 - dt * dt * fr * fr / 8.0;
      a.c3 = std::sqrt(dt) * sigma / 2.0 - std::pow(dt, 1.5) * fr * sigma / 8.0;
      a.c5 = std::pow(dt, 1.5) * sigma / (2.0 * std::sqrt(3.0));
      a.c4 = fr / 2.0 * a.c5;
    }
    const int64_t step0 = h->md_step;  // absolute index of this run's first step
    a.lim2 = h->skin > 0.0 ? 0.25 * h->skin * h->skin : -1.0;  // skin = 0: every step rebuilds
    a.n_frames = (int)F;
    a.n_blk = (int)n_blk;
    a.chunk = chunk;
    a.baro = baro ? 1 : 0;
    a.baro_iso = h->md_baro_p.isotropic ? 1 : 0;
    a.cells = nullptr, a.virial = nullptr;
    a.baro_scale = h->md_baro_scale.ptr;
    a.baro_rec = h->md_baro_rec.ptr;
    a.baro_p0 = h->md_baro_p.pressure;
    a.baro_k = baro ? dt / h->md_baro_p.taup * h->md_baro_p.compressibility / 3.0 : 0.0;
    for (int c = 0; c < 3; ++c) a.baro_mask[c] = h->md_baro_p.mask[c] ? 1 : 0;
    a.skin = h->skin;
    a.r_list = h->rmax + h->skin;
    a.nhc = nhc ? 1 : 0;
    a.nhc_chain = h->md_nhc_p.chain, a.nhc_loops = h->md_nhc_p.loops, a.nhc_dof = h->md_nhc_p.dof_removed;
    a.nhc_kT0 = nhc ? h->md_nhc_p.kT0 : 0.0;
    a.nhc_q = nhc ? h->md_nhc_p.kT0 * h->md_nhc_p.tau * h->md_nhc_p.tau : 0.0;
    a.nhc_eta = h->md_nhc_eta.ptr, a.nhc_veta = h->md_nhc_veta.ptr, a.nhc_rec = h->md_nhc_rec.ptr;
    // Sampling: the launch of step k holds the whole-step state t = step0 + k. It samples when t is a multiple
    // of sample_every at or behind sample 0, except launch 0 where the last launch of the run before sampled
    // that very state. Sample number and ring slot are functions of t alone, so the launches that returned
    // early behind a stale list and are enqueued again after the rebuild write what they would have written.
    const bool sampling = samp && samp_was_valid && N > 0;
    const int64_t samp_s = h->md_samp_p.sample_every, samp_L = h->md_samp_p.n_lags;
    const int64_t samp_origin = h->md_samp_origin, samp_last = h->md_samp_last;
    ta::MdCorrLaunch c;
    c.ring_x = h->md_ring_x.ptr, c.ring_v = h->md_ring_v.ptr;
    c.blk_start = h->md_corr_blk.ptr;
    c.part = h->md_corr_part.ptr;
    c.acc_v = h->md_corr_acc.ptr;
    c.acc_x = sampling ? h->md_corr_acc.ptr + F * (size_t)h->n_elements * (size_t)samp_L : nullptr;
    c.status = h->md_status.ptr;
    c.n_atoms = (long long)N;
    c.n_lags = (int)samp_L, c.n_elements = h->n_elements, c.n_frames = (int)F, c.n_chunks = h->md_corr_chunks;
    // Pair distributions: the state t = step0 + k is counted by a launch IN FRONT OF the integrator launch of
    // step k, whose drift leaves x(t). With seq = k the integrator's predicate skips exactly the states that
    // were reached on a stale list; after the rebuild the launch is enqueued again with the rest and counts
    // then. Launch 0 does not count the state the last launch of the run before counted.
    const bool rdf_run = rdf && rdf_was_valid && N > 0;
    const int64_t rdf_s = h->md_rdf_p.sample_every, rdf_origin = h->md_rdf_origin, rdf_last = h->md_rdf_last;
    ta::MdRdfLaunch g;
    g.blk_start = h->md_rdf_blk.ptr;
    g.counts = h->md_rdf_acc.ptr;
    g.status = h->md_status.ptr;
    g.n_bins = h->md_rdf_p.n_bins, g.n_elements = h->n_elements, g.n_frames = (int)F;
    g.n_blk = h->md_rdf_n_blk, g.chunk = h->md_rdf_chunk;
    g.dr = rdf_run ? h->md_rdf_p.r_max / (double)h->md_rdf_p.n_bins : 1.0;
    auto integrate = [&](int k, bool drift) {
      if (rdf_run) {
        const int64_t t = step0 + k;
        if (t >= rdf_origin && (t - rdf_origin) % rdf_s == 0 && !(k == 0 && t == rdf_last)) {
          g.pos = h->db.pos;
          g.cells = h->db.cells;
          g.species = h->db.species;
          g.atom_start = h->db.atom_start;
          g.pair_start = h->pair_start.ptr;  // the resident list, not the exact one filtered from it
          g.pair_i = h->pair_i.ptr;
          g.pair_j = h->pair_j.ptr;
          g.pair_shift = h->pair_shift.ptr;
          g.seq = (unsigned)k;
          ta::launch_md_rdf(g, s);
          HIP_CHECK(hipGetLastError());
        }
      }
      // (a rebuild may have moved the batch's arrays: the pointers are taken at every launch)
      a.pos = h->db.pos;
      a.forces = h->db.forces;
      a.energy = h->db.energy;
      a.atom_start = h->db.atom_start;
      a.cells = h->db.cells;
      a.virial = h->db.virial;
      a.seq = (unsigned)k;
      a.step = (long long)(step0 + k);  // (a step redone after a rebuild keeps its index)
      a.kick2 = k > 0 ? 1 : 0;  // the state at entry is a whole step
      a.drift = drift ? 1 : 0;
      a.rec = (k % record_every == 0) ? (long long)(k / record_every) : -1;
      a.snap_x = a.snap_v = nullptr;
      const int64_t t = step0 + k;
      const bool due = sampling && t >= samp_origin && (t - samp_origin) % samp_s == 0 && !(k == 0 && t == samp_last);
      if (due) {
        c.n = (long long)((t - samp_origin) / samp_s);
        const size_t slot = (size_t)(c.n % samp_L);
        a.snap_x = h->md_ring_x.ptr + slot * 3 * N;
        a.snap_v = h->md_ring_v.ptr + slot * 3 * N;
      }
      ta::launch_md_integrate(a, threads, s);
      HIP_CHECK(hipGetLastError());
      if (due) {  // directly behind the launch that sampled, under the same predicate
        c.species = h->db.species;
        c.atom_start = h->db.atom_start;
        c.seq = (unsigned)k;
        ta::launch_md_correlate(c, s);
        HIP_CHECK(hipGetLastError());
      }
    };

    h->jvp_valid = false;
    compute_impl(h, want, false, nullptr);  // F_0 and the record of the state at entry
    int rebuilds = 0;
    resident_steps(h, "ta_md_run", n_steps, want, [&](int q) { integrate(q, true); },
                   [](int, int) { return -1; }, &rebuilds, n_rebuilds);
    integrate(n_steps, false);  // the pending half-kick and the last record
    HIP_CHECK(hipStreamSynchronize(s));
    h->upload_pending = false;
    h->md_step = step0 + n_steps;
    if (sampling && h->md_step >= samp_origin)  // the newest sample: the last multiple of sample_every reached
      h->md_samp_last = std::max(samp_last, samp_origin + (h->md_step - samp_origin) / samp_s * samp_s);
    h->md_samp_valid = samp_was_valid;
    if (rdf_run && h->md_step >= rdf_origin)
      h->md_rdf_last = std::max(rdf_last, rdf_origin + (h->md_step - rdf_origin) / rdf_s * rdf_s);
    h->md_rdf_valid = rdf_was_valid;
    if (n_rebuilds) *n_rebuilds = rebuilds;
    if (baro && F) {
      std::vector<double> rec(4 * n_rec * F);
      HIP_CHECK(hipMemcpy(rec.data(), h->md_baro_rec.ptr, rec.size() * sizeof(double), hipMemcpyDeviceToHost));
      h->md_rec_volume.resize(n_rec * F);
      h->md_rec_press.resize(3 * n_rec * F);
      for (size_t j = 0; j < n_rec * F; ++j) {
        h->md_rec_volume[j] = rec[4 * j];
        for (int c = 0; c < 3; ++c) h->md_rec_press[3 * j + c] = rec[4 * j + 1 + c];
      }
      // The cells moved under a list built for others: one list for the final state, as at the end of a cell
      // relaxation, so that ref_pos and ref_cells are what ta_update_positions, ta_step, a fixed-cell run and
      // ta_relax_run take them for. The evaluation is repeated on it; results agree up to summation order.
      std::vector<double> cells(9 * F);
      HIP_CHECK(hipMemcpy(cells.data(), h->db.cells, 9 * F * sizeof(double), hipMemcpyDeviceToHost));
      if (std::memcmp(cells.data(), h->ref_cells.data(), 9 * F * sizeof(double)) != 0) {
        std::vector<double> x(3 * N);
        if (N) HIP_CHECK(hipMemcpy(x.data(), h->db.pos, 3 * N * sizeof(double), hipMemcpyDeviceToHost));
        try {
          rebuild_list(h, x.data(), cells.data());
        } catch (const HipError &e) {
          throw HipError(std::string("ta_md_run: list rebuild for the final cells failed: ") + e.what());
        } catch (const std::exception &e) {
          throw std::runtime_error(std::string("ta_md_run: list rebuild for the final cells failed: ") + e.what());
        }
        if (N) HIP_CHECK(hipMemcpyAsync(h->md_ref.ptr, h->db.pos, 3 * N * sizeof(double), hipMemcpyDeviceToDevice, s));
        h->md_ref_builds = h->n_list_builds;
        compute_impl(h, want, false, nullptr);
        HIP_CHECK(hipStreamSynchronize(s));
        h->upload_pending = false;
        ++rebuilds;
        if (n_rebuilds) *n_rebuilds = rebuilds;
      }
      if (h->relax_cell_on && h->relax_valid &&
          std::memcmp(cells_at_entry.data(), h->ref_cells.data(), 9 * F * sizeof(double)) != 0) {
        // the barostat's cells replace the relaxed ones: they are h0 from here on, G = I, the cell velocities 0
        HIP_CHECK(hipMemcpy(h->relax_cell_h0.ptr, h->ref_cells.data(), 9 * F * sizeof(double), hipMemcpyHostToDevice));
        h->relax_cell_G_host.assign(9 * F, 0.0);
        for (size_t f = 0; f < F; ++f) h->relax_cell_G_host[9 * f] = h->relax_cell_G_host[9 * f + 4] = h->relax_cell_G_host[9 * f + 8] = 1.0;
        h->relax_cell_vel_host.assign(9 * F, 0.0);
      }
      h->md_rec_valid = true;
    }
    if (nhc) {
      h->md_rec_chain.resize(n_rec * F);
      if (F) HIP_CHECK(hipMemcpy(h->md_rec_chain.data(), h->md_nhc_rec.ptr, n_rec * F * sizeof(double), hipMemcpyDeviceToHost));
      h->md_nhc_rec_valid = true;
    }
    if (epot && F) HIP_CHECK(hipMemcpy(epot, h->md_epot.ptr, n_rec * F * sizeof(double), hipMemcpyDeviceToHost));
    if (ekin && F) {
      std::vector<double> part(n_rec * n_blk);
      HIP_CHECK(hipMemcpy(part.data(), h->md_ke.ptr, part.size() * sizeof(double), hipMemcpyDeviceToHost));
      const std::vector<int32_t> &start = h->md_blk_start_host;
      for (size_t r = 0; r < n_rec; ++r)
        for (size_t f = 0; f < F; ++f) {
          double t = 0.0;
          for (int32_t b = start[f]; b < start[f + 1]; ++b) t += part[r * n_blk + (size_t)b];
          ekin[r * F + f] = t;
        }
    }
  });
  h->cell_running = h->md_baro_running = false;
  return rc;
}

int ta_md_get_state(ta_handle h, double *positions, double *velocities) {
  if (!h) return TA_ERR_INVALID;
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "ta_md_get_state: no resident batch");
  if (!h->md_valid) return fail(h, TA_ERR_INVALID, "ta_md_get_state called before ta_md_init");
  return guarded(h, [&]() {
    const size_t N = h->keep_species.size();
    HIP_CHECK(hipStreamSynchronize(h->stream));
    h->upload_pending = false;
    if (positions && N) HIP_CHECK(hipMemcpy(positions, h->db.pos, 3 * N * sizeof(double), hipMemcpyDeviceToHost));
    if (velocities && N) HIP_CHECK(hipMemcpy(velocities, h->md_vel.ptr, 3 * N * sizeof(double), hipMemcpyDeviceToHost));
  });
}

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
    const size_t N = h->keep_species.size(), F = h->keep_natoms.size();
    h->relax_valid = false;
    HIP_CHECK(hipStreamSynchronize(h->stream));
    h->upload_pending = false;
    h->relax_vel.ensure(3 * N + 1);
    h->relax_fixed.ensure(N + 1);
    h->relax_state.ensure(2 * F + 1);
    h->relax_count.ensure(1);
    h->md_ref.ensure(3 * N + 1);
    h->md_ref_builds = -1;  // ta_relax_run uploads ref_pos
    h->md_status.ensure(2);
    h->md_status_host.ensure(64);
    if (N) {
      HIP_CHECK(hipMemset(h->relax_vel.ptr, 0, 3 * N * sizeof(double)));
      if (fixed) {
        std::vector<uint8_t> mask(N);
        for (size_t i = 0; i < N; ++i) mask[i] = fixed[i] ? 1 : 0;
        HIP_CHECK(hipMemcpy(h->relax_fixed.ptr, mask.data(), N, hipMemcpyHostToDevice));
        h->relax_fixed_host = mask;
      } else {
        HIP_CHECK(hipMemset(h->relax_fixed.ptr, 0, N));
        h->relax_fixed_host.assign(N, 0);
      }
    } else {
      h->relax_fixed_host.clear();
    }
    ta::RelaxFrameState st;
    st.dt = q.dt;
    st.a = q.astart;
    st.fmax2 = 0.0;
    st.npos = 0;
    st.first = 1;
    st.converged = 0;
    st.steps = 0;
    h->relax_state_host.assign(F, st);
    h->relax_cell_on = false;
    h->relax_band_on = h->relax_band_ran = false;
    h->relax_cell_G_host.assign(9 * F, 0.0);
    for (size_t f = 0; f < F; ++f) h->relax_cell_G_host[9 * f] = h->relax_cell_G_host[9 * f + 4] = h->relax_cell_G_host[9 * f + 8] = 1.0;
    h->relax_cell_vel_host.assign(9 * F, 0.0);
    h->relax_p = q;
    h->md_chunk = 0;  // (the workgroup layout is planned for this batch by the next run)
    h->md_blk_start_host.clear();
    h->relax_valid = true;
  });
}

int ta_relax_run(ta_handle h, int32_t max_steps, double fmax, uint32_t want, int32_t *steps, int32_t *converged,
                 double *fmax_out, int32_t *n_rebuilds) {
  if (!h) return TA_ERR_INVALID;
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "ta_relax_run: no resident batch");
  if (!h->relax_valid)
    return fail(h, TA_ERR_INVALID, "ta_relax_run called before ta_relax_init (ta_set_frames drops the relaxation state)");
  if (max_steps < 0) return fail(h, TA_ERR_INVALID, "ta_relax_run: max_steps must be >= 0");
  if (!std::isfinite(fmax) || !(fmax > 0.0)) return fail(h, TA_ERR_INVALID, "ta_relax_run: fmax must be finite and > 0");
  if (n_rebuilds) *n_rebuilds = 0;
  want |= TA_WANT_ENERGY | TA_WANT_FORCES;
  want &= ~(uint32_t)TA_WANT_REUSE_DESCRIPTORS;
  const bool cell = h->relax_cell_on;
  const bool band = h->relax_band_on;  // (never with `cell`)
  if (cell) want |= TA_WANT_VIRIAL;  // the force on the cell rows
  // a run that fails leaves positions and velocities somewhere on its way and the host's image of the
  // per-frame records behind them: the state is dropped, and only ta_relax_init makes a new one
  h->relax_valid = false;
  h->relax_band_ran = false;
  h->cell_running = cell;
  const int rc = guarded(h, [&]() {
    const size_t N = h->keep_species.size(), F = h->keep_natoms.size();
    hipStream_t s = h->stream;
    md_plan_blocks(h, ta::kMdChunk);
    // band mode: the FIRE launches see the whole band as one pseudo-frame of N atoms; the band launches cut
    // every interior image into its own workgroups
    const int band_n = band ? h->keep_natoms[0] : 0;
    const int band_blk_per_image = std::max(1, (band_n + ta::kMdChunk - 1) / ta::kMdChunk);
    const size_t n_blk = band ? std::max<size_t>(1, (N + ta::kMdChunk - 1) / ta::kMdChunk) : (size_t)h->md_n_blk;
    h->relax_part.ensure(4 * n_blk + 1);
    if (band) h->band_part.ensure(4 * (F - 2) * (size_t)band_blk_per_image + 1);
    HIP_CHECK(hipStreamSynchronize(s));
    if (h->md_ref_builds != h->n_list_builds) {  // the host built the list that is resident: its positions go up once
      if (N) HIP_CHECK(hipMemcpy(h->md_ref.ptr, h->ref_pos.data(), 3 * N * sizeof(double), hipMemcpyHostToDevice));
      h->md_ref_builds = h->n_list_builds;
    }
    // every frame is tested against this run's fmax: a frame frozen by an earlier run may wake
    std::vector<ta::RelaxFrameState> &st = h->relax_state_host;
    for (auto &r : st) r.converged = 0, r.steps = 0;
    if (F) HIP_CHECK(hipMemcpy(h->relax_state.ptr, st.data(), F * sizeof(ta::RelaxFrameState), hipMemcpyHostToDevice));
    if (band) {  // the band's one record into copy 0, the pseudo-frame's layout next to the climbing word
      h->band_state_host.converged = 0, h->band_state_host.steps = 0;
      HIP_CHECK(hipMemcpy(h->band_state.ptr, &h->band_state_host, sizeof(ta::RelaxFrameState), hipMemcpyHostToDevice));
      const int32_t layout[5] = {0, (int32_t)N, 0, (int32_t)n_blk, -1};
      HIP_CHECK(hipMemcpy(h->band_layout.ptr, layout, sizeof(layout), hipMemcpyHostToDevice));
    }
    HIP_CHECK(hipMemset(h->relax_count.ptr, 0, sizeof(int)));
    if (cell && F) {  // the current G and cell velocity into copy 0, the cells of the resident list next to md_ref
      HIP_CHECK(hipMemcpy(h->relax_cell_G.ptr, h->relax_cell_G_host.data(), 9 * F * sizeof(double), hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(h->relax_cell_vel.ptr, h->relax_cell_vel_host.data(), 9 * F * sizeof(double), hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(h->md_ref_cells.ptr, h->ref_cells.data(), 9 * F * sizeof(double), hipMemcpyHostToDevice));
    }
    volatile unsigned *status_host = reinterpret_cast<volatile unsigned *>(h->md_status_host.ptr);
    status_host[0] = status_host[1] = 0u;  // (no launch that writes them is in flight: every run ends with a wait)
    HIP_CHECK(hipMemsetAsync(h->md_status.ptr, 0, 2 * sizeof(unsigned), s));

    const ta_fire_params &p = h->relax_p;
    ta::RelaxLaunch a;
    a.vel = h->relax_vel.ptr;
    a.fixed = h->relax_fixed.ptr;
    a.ref = h->md_ref.ptr;
    a.blk_start = h->md_blk_start.ptr;
    a.part = h->relax_part.ptr;
    a.state = h->relax_state.ptr;
    a.n_converged = h->relax_count.ptr;
    a.status = h->md_status.ptr;
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
    a.ref_cells = h->md_ref_cells.ptr, a.cell_h0 = h->relax_cell_h0.ptr, a.cell_cf = h->relax_cell_cf.ptr;
    a.cell_G = h->relax_cell_G.ptr, a.cell_vel = h->relax_cell_vel.ptr, a.cell_fmax2 = h->relax_cell_fmax2.ptr;
    {
      const int32_t *m = h->relax_cell_p.mask;  // Voigt xx yy zz yz xz xy
      const int32_t full[9] = {m[0], m[5], m[4], m[5], m[1], m[3], m[4], m[3], m[2]};
      for (int c = 0; c < 9; ++c) a.cell_mask[c] = full[c] ? 1.0 : 0.0;
    }
    a.pressure = h->relax_cell_p.pressure;
    a.skin = h->skin;
    a.r_list = h->rmax + h->skin;
    a.hydrostatic = h->relax_cell_p.hydrostatic ? 1 : 0;
    ta::NebLaunch nb = {};
    if (band) {
      a.fixed = h->band_fixed.ptr;
      a.blk_start = h->band_layout.ptr + 2;
      a.state = h->band_state.ptr;
      a.n_frames = 1;
      nb.fixed = h->band_fixed.ptr;
      nb.part = h->band_part.ptr;
      nb.band = h->band_force.ptr;
      nb.climbing = h->band_layout.ptr + 4;
      nb.status = h->md_status.ptr;
      nb.k = h->relax_band_p.k;
      nb.n_images = (int)F, nb.n = band_n, nb.chunk = ta::kMdChunk, nb.blk_per_image = band_blk_per_image;
      nb.climb = h->relax_band_p.climb ? 1 : 0;
    }
    // B (and, with `tangents`, tau) of the resident evaluation
    auto band_force = [&](int k, bool tangents) {
      nb.pos = h->db.pos;
      nb.forces = h->db.forces;
      nb.energy = h->db.energy;
      nb.tau = tangents ? h->band_tau.ptr : nullptr;
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
        a.forces = h->band_force.ptr;
        a.atom_start = h->band_layout.ptr;
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
      ta::RelaxFrameState &b = h->band_state_host;
      HIP_CHECK(hipMemcpy(&b, h->band_state.ptr + (size_t)(launched & 1), sizeof(ta::RelaxFrameState), hipMemcpyDeviceToHost));
      for (size_t f = 0; f < F; ++f) {
        if (steps) steps[f] = b.steps;
        if (converged) converged[f] = b.converged;
        if (fmax_out) fmax_out[f] = std::sqrt(b.fmax2);
      }
      h->band_energy_host.resize(F);  // what ta_relax_get_band hands out next to B and tau of this state
      HIP_CHECK(hipMemcpy(h->band_energy_host.data(), h->db.energy, F * sizeof(double), hipMemcpyDeviceToHost));
      return;
    }
    if (F)
      HIP_CHECK(hipMemcpy(st.data(), h->relax_state.ptr + (size_t)(launched & 1) * F, F * sizeof(ta::RelaxFrameState),
                          hipMemcpyDeviceToHost));
    for (size_t f = 0; f < F; ++f) {
      if (steps) steps[f] = st[f].steps;
      if (converged) converged[f] = st[f].converged;
      if (fmax_out) fmax_out[f] = std::sqrt(st[f].fmax2);
    }
    if (cell && F) {
      HIP_CHECK(hipMemcpy(h->relax_cell_G_host.data(), h->relax_cell_G.ptr + 9 * (size_t)(launched & 1) * F,
                          9 * F * sizeof(double), hipMemcpyDeviceToHost));
      HIP_CHECK(hipMemcpy(h->relax_cell_vel_host.data(), h->relax_cell_vel.ptr + 9 * (size_t)(launched & 1) * F,
                          9 * F * sizeof(double), hipMemcpyDeviceToHost));
      // The cells moved under a list built for others: one list for the final state, so that ref_pos and
      // ref_cells (the host's image of the resident geometry) are what ta_update_positions, ta_md_run and a
      // fixed-cell run take them for. The evaluation is repeated on it; results agree up to summation order.
      std::vector<double> cells(9 * F);
      HIP_CHECK(hipMemcpy(cells.data(), h->db.cells, 9 * F * sizeof(double), hipMemcpyDeviceToHost));
      if (std::memcmp(cells.data(), h->ref_cells.data(), 9 * F * sizeof(double)) != 0) {
        std::vector<double> x(3 * N);
        if (N) HIP_CHECK(hipMemcpy(x.data(), h->db.pos, 3 * N * sizeof(double), hipMemcpyDeviceToHost));
        try {
          rebuild_list(h, x.data(), cells.data());
        } catch (const HipError &e) {
          throw HipError(std::string("ta_relax_run: list rebuild for the final cells failed: ") + e.what());
        } catch (const std::exception &e) {
          throw std::runtime_error(std::string("ta_relax_run: list rebuild for the final cells failed: ") + e.what());
        }
        if (N) HIP_CHECK(hipMemcpyAsync(h->md_ref.ptr, h->db.pos, 3 * N * sizeof(double), hipMemcpyDeviceToDevice, s));
        h->md_ref_builds = h->n_list_builds;
        compute_impl(h, want, false, nullptr);
        HIP_CHECK(hipStreamSynchronize(s));
        h->upload_pending = false;
        ++rebuilds;
        if (n_rebuilds) *n_rebuilds = rebuilds;
      }
    }
  });
  h->cell_running = false;
  if (rc == TA_OK) h->relax_valid = true, h->relax_band_ran = band;
  else h->relax_cell_on = h->relax_band_on = false;
  return rc;
}

int ta_relax_get_state(ta_handle h, double *positions, double *velocities, double *dt, double *a, int32_t *npos) {
  if (!h) return TA_ERR_INVALID;
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "ta_relax_get_state: no resident batch");
  if (!h->relax_valid) return fail(h, TA_ERR_INVALID, "ta_relax_get_state called before ta_relax_init");
  return guarded(h, [&]() {
    const size_t N = h->keep_species.size(), F = h->keep_natoms.size();
    HIP_CHECK(hipStreamSynchronize(h->stream));
    h->upload_pending = false;
    if (positions && N) HIP_CHECK(hipMemcpy(positions, h->db.pos, 3 * N * sizeof(double), hipMemcpyDeviceToHost));
    if (velocities && N)
      HIP_CHECK(hipMemcpy(velocities, h->relax_vel.ptr, 3 * N * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t f = 0; f < F; ++f) {  // (band mode: the band's one record for every frame)
      const ta::RelaxFrameState &r = h->relax_band_on ? h->band_state_host : h->relax_state_host[f];
      if (dt) dt[f] = r.dt;
      if (a) a[f] = r.a;
      if (npos) npos[f] = r.npos;
    }
  });
}

int ta_relax_set_cell(ta_handle h, int on, const ta_relax_cell_params *p) {
  if (!h) return TA_ERR_INVALID;
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "ta_relax_set_cell: no resident batch");
  if (!h->relax_valid) return fail(h, TA_ERR_INVALID, "ta_relax_set_cell called before ta_relax_init");
  if (!on) {
    h->relax_cell_on = false;  // (the cells stay as they are)
    return TA_OK;
  }
  if (h->relax_band_on)
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
    h->relax_cell_h0.ensure(9 * F + 1);
    h->relax_cell_cf.ensure(F + 1);
    h->relax_cell_G.ensure(2 * 9 * F + 1);
    h->relax_cell_vel.ensure(2 * 9 * F + 1);
    h->relax_cell_fmax2.ensure(F + 1);
    h->md_ref_cells.ensure(9 * F + 1);
    if (F) {
      HIP_CHECK(hipMemcpy(h->relax_cell_h0.ptr, h->ref_cells.data(), 9 * F * sizeof(double), hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(h->relax_cell_cf.ptr, cf.data(), F * sizeof(double), hipMemcpyHostToDevice));
      HIP_CHECK(hipMemset(h->relax_cell_fmax2.ptr, 0, F * sizeof(double)));
    }
    h->relax_cell_G_host.assign(9 * F, 0.0);
    for (size_t f = 0; f < F; ++f) h->relax_cell_G_host[9 * f] = h->relax_cell_G_host[9 * f + 4] = h->relax_cell_G_host[9 * f + 8] = 1.0;
    h->relax_cell_vel_host.assign(9 * F, 0.0);
    h->relax_cell_p = q;
    h->relax_cell_on = true;
  });
}

int ta_relax_get_cell(ta_handle h, double *cells, double *deform, double *cell_velocities, double *cell_fmax) {
  if (!h) return TA_ERR_INVALID;
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "ta_relax_get_cell: no resident batch");
  if (!h->relax_valid) return fail(h, TA_ERR_INVALID, "ta_relax_get_cell called before ta_relax_init");
  return guarded(h, [&]() {
    const size_t F = h->keep_natoms.size();
    HIP_CHECK(hipStreamSynchronize(h->stream));
    h->upload_pending = false;
    if (!F) return;
    // (between runs ref_cells is the image of the device's cells)
    if (cells) std::memcpy(cells, h->ref_cells.data(), 9 * F * sizeof(double));
    if (deform) std::memcpy(deform, h->relax_cell_G_host.data(), 9 * F * sizeof(double));
    if (cell_velocities) std::memcpy(cell_velocities, h->relax_cell_vel_host.data(), 9 * F * sizeof(double));
    if (cell_fmax) {
      if (h->relax_cell_fmax2.ptr) {
        HIP_CHECK(hipMemcpy(cell_fmax, h->relax_cell_fmax2.ptr, F * sizeof(double), hipMemcpyDeviceToHost));
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
  if (!h->relax_valid) return fail(h, TA_ERR_INVALID, "ta_relax_set_band called before ta_relax_init");
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
    if (h->relax_cell_on)
      return fail(h, TA_ERR_INVALID, "ta_relax_set_band: the cell option is on (ta_relax_set_cell); cells along a band stay fixed");
  }
  return guarded(h, [&]() {
    HIP_CHECK(hipStreamSynchronize(h->stream));
    h->upload_pending = false;
    // the optimiser starts again, in either direction: v = 0, dt, a = astart, npos = 0, first
    ta::RelaxFrameState st;
    st.dt = h->relax_p.dt;
    st.a = h->relax_p.astart;
    st.fmax2 = 0.0;
    st.npos = 0;
    st.first = 1;
    st.converged = 0;
    st.steps = 0;
    h->relax_state_host.assign(F, st);
    h->band_state_host = st;
    if (N) HIP_CHECK(hipMemset(h->relax_vel.ptr, 0, 3 * N * sizeof(double)));
    h->relax_band_ran = false;
    if (!on) {
      h->relax_band_on = false;
      return;
    }
    const size_t n = (size_t)h->keep_natoms[0];
    h->band_force.ensure(3 * N + 1);
    h->band_tau.ensure(3 * N + 1);
    h->band_fixed.ensure(N + 1);
    h->band_state.ensure(2);
    h->band_layout.ensure(5);
    std::vector<uint8_t> mask(h->relax_fixed_host);  // the user's mask OR-ed with the two endpoint images
    mask.resize(N, 0);
    std::fill(mask.begin(), mask.begin() + n, 1);
    std::fill(mask.end() - n, mask.end(), 1);
    if (N) {
      HIP_CHECK(hipMemcpy(h->band_fixed.ptr, mask.data(), N, hipMemcpyHostToDevice));
      HIP_CHECK(hipMemset(h->band_force.ptr, 0, 3 * N * sizeof(double)));  // (the endpoints' rows stay 0)
      HIP_CHECK(hipMemset(h->band_tau.ptr, 0, 3 * N * sizeof(double)));
    }
    h->relax_band_p = q;
    h->relax_band_on = true;
  });
}

int ta_relax_get_band(ta_handle h, double *band_forces, double *tangents, double *energies, int32_t *climbing) {
  if (!h) return TA_ERR_INVALID;
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "ta_relax_get_band: no resident batch");
  if (!h->relax_valid) return fail(h, TA_ERR_INVALID, "ta_relax_get_band called before ta_relax_init");
  if (!h->relax_band_on) return fail(h, TA_ERR_INVALID, "ta_relax_get_band: the band option is off (ta_relax_set_band)");
  if (!h->relax_band_ran)
    return fail(h, TA_ERR_INVALID, "ta_relax_get_band: no ta_relax_run of this band yet (max_steps = 0 counts)");
  return guarded(h, [&]() {
    const size_t N = h->keep_species.size(), F = h->keep_natoms.size();
    HIP_CHECK(hipStreamSynchronize(h->stream));
    h->upload_pending = false;
    if (band_forces && N) HIP_CHECK(hipMemcpy(band_forces, h->band_force.ptr, 3 * N * sizeof(double), hipMemcpyDeviceToHost));
    if (tangents && N) HIP_CHECK(hipMemcpy(tangents, h->band_tau.ptr, 3 * N * sizeof(double), hipMemcpyDeviceToHost));
    if (energies) std::memcpy(energies, h->band_energy_host.data(), F * sizeof(double));
    if (climbing) HIP_CHECK(hipMemcpy(climbing, h->band_layout.ptr + 4, sizeof(int32_t), hipMemcpyDeviceToHost));
  });
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
  int64_t n = 0;
  for (int e = 0; e < h->n_elements; ++e) n += ta::mlp_param_count(h->mlp[e]);
  *n_params = n;
  return TA_OK;
}

namespace {
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
}  // namespace

int ta_update_weights(ta_handle h, const double *weights, int64_t n_weights) {
  if (!h || !weights) return TA_ERR_INVALID;
  if (h->td)  // in place: the device copy of the net descriptions (td_dev) keeps its pointers
    return guarded(h, [&]() {
      const int64_t want = ta::td_param_count(h->td_nets, h->n_elements);
      if (n_weights != want)
        throw std::invalid_argument("ta_update_weights: expected " + std::to_string(want) + " values");
      HIP_CHECK(hipStreamSynchronize(h->stream));  // nothing may still read the old weights
      const double *src = weights;
      for (int j = 0; j < 3 * h->n_elements; ++j) upload_net_weights(h->td_nets[j], src);
    });
  if (h->eam)
    return guarded(h, [&]() {
      HIP_CHECK(hipStreamSynchronize(h->stream));  // nothing may still read the old weights
      ta::eam_update_weights(h->eam, weights, n_weights);
    });
  if (h->kind != TA_MODEL_SF_MLP && h->kind != TA_MODEL_GRAP_MLP)
    return fail(h, TA_ERR_INVALID, "the model has no MLP");
  return guarded(h, [&]() {
    int64_t want = 0;
    for (int e = 0; e < h->n_elements; ++e) want += ta::mlp_param_count(h->mlp[e]);
    if (n_weights != want)
      throw std::invalid_argument("ta_update_weights: expected " + std::to_string(want) + " values");
    HIP_CHECK(hipStreamSynchronize(h->stream));  // nothing may still read the old weights
    const double *src = weights;
    for (int e = 0; e < h->n_elements; ++e) upload_net_weights(h->mlp[e], src);
  });
}

namespace {
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
}  // namespace

int ta_energy_gradient(ta_handle h, const double *frame_coeff, double *grad, int64_t n_grad) {
  if (!h || !frame_coeff || !grad) return TA_ERR_INVALID;
  if (h->td)  // frame_coeff = dL/dF_f
    return ta_td_loss_gradient(h, frame_coeff, nullptr, nullptr, nullptr, nullptr, grad, n_grad, nullptr);
  if (h->kind == TA_MODEL_EAM_FS) return fail(h, TA_ERR_INVALID, fs_inference_only("ta_energy_gradient"));
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "no resident batch");
  if (h->eam)
    return guarded(h, [&]() {
      const int64_t total = ta::eam_param_count(h->eam);
      if (n_grad != total)
        throw std::invalid_argument("ta_energy_gradient: expected room for " + std::to_string(total) + " values");
      if (total == 0) return;
      // weight gradients differentiate the networks themselves: from here on this handle evaluates its
      // nn pair functions exactly, not through their tables (eam_set_nn_tables)
      if (h->filtered)
        throw std::domain_error("ta_energy_gradient: not available on a skin-filtered batch; "
                                "ta_set_skin(h, 0) and ta_set_frames first");
      if (ta::eam_nn_tables_on(h->eam)) HIP_CHECK(hipStreamSynchronize(h->stream));
      ta::eam_mark_trained(h->eam);
      ta::eam_ensure(h->eam, h->db);  // the per-pair columns of the exact evaluation
      // every function depends on the weights: the forward pass runs again (rho, F', moments)
      compute_impl(h, TA_WANT_ENERGY, false, nullptr);
      hipStream_t s = h->stream;
      const size_t F = (size_t)h->db.n_frames;
      h->train_grad.ensure((size_t)total + 8);
      h->train_coeff.ensure(F + 8);
      if (F) HIP_CHECK(hipMemcpyAsync(h->train_coeff.ptr, frame_coeff, F * sizeof(double), hipMemcpyHostToDevice, s));
      ta::eam_energy_gradient(h->eam, h->db, h->train_coeff.ptr, h->train_grad.ptr, s);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipMemcpyAsync(grad, h->train_grad.ptr, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
    });
  if (h->kind != TA_MODEL_SF_MLP && h->kind != TA_MODEL_GRAP_MLP)
    return fail(h, TA_ERR_INVALID, "the model has no MLP");
  return guarded(h, [&]() {
    int64_t total = 0;
    for (int e = 0; e < h->n_elements; ++e) total += ta::mlp_param_count(h->mlp[e]);
    if (n_grad != total)
      throw std::invalid_argument("ta_energy_gradient: expected room for " + std::to_string(total) + " values");
    mark_grap_trained(h);
    // descriptors do not depend on the weights: computed once per resident batch
    if (!h->descriptors_valid) compute_impl(h, TA_WANT_ENERGY, false, nullptr);
    hipStream_t s = h->stream;
    const size_t F = (size_t)h->db.n_frames;
    size_t scratch = 0, partial = 0;
    for (int e = 0; e < h->n_elements; ++e) {
      const int n_el = h->db.elem_start[e + 1] - h->db.elem_start[e];
      scratch = std::max(scratch, ta::mlp_grad_scratch_doubles(h->mlp[e], n_el));
      partial = std::max(partial, ta::mlp_grad_partial_doubles(h->mlp[e], n_el));
    }
    h->train_scratch.ensure(scratch + 8);
    h->train_partial.ensure(partial + 8);
    h->train_grad.ensure((size_t)total + 8);
    h->train_coeff.ensure(F + 8);
    if (F) HIP_CHECK(hipMemcpyAsync(h->train_coeff.ptr, frame_coeff, F * sizeof(double), hipMemcpyHostToDevice, s));
    size_t off = 0;
    for (int e = 0; e < h->n_elements; ++e) {
      const int n_el = h->db.elem_start[e + 1] - h->db.elem_start[e];
      ta::launch_mlp_grad(h->mlp[e], h->activation, h->sf.ndim, h->db.elem_atoms + h->db.elem_start[e], n_el,
                          h->db, h->train_coeff.ptr, h->train_scratch.ptr, h->train_partial.ptr,
                          h->train_grad.ptr + off, s);
      off += (size_t)ta::mlp_param_count(h->mlp[e]);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(grad, h->train_grad.ptr, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  });
}

namespace {
// the dE/dD launches of compute_impl alone, on the dE/dG that is in `db.dEdG` (the forward pass of
// this batch has run: pair records, candidate masks and, for GRAP, the moments are resident)
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
}  // namespace

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
    // nn functions of an EAM / ADP model (round 3): one second-order pass per network, ta_eam.hip::eam_loss_gradient
    if (!ta::eam_loss_gradient_supported(h->eam))
      return fail(h, TA_ERR_UNSUPPORTED, "ta_loss_gradient: the analytic force / stress term covers EAM / ADP models "
                                         "whose analytic parts are of the Zjw04 family or tabulated");
    if (h->filtered)
      return fail(h, TA_ERR_UNSUPPORTED, "ta_loss_gradient: not available on a skin-filtered batch; "
                                         "ta_set_skin(h, 0) and ta_set_frames first");
    return guarded(h, [&]() {
      const int64_t total = ta::eam_param_count(h->eam);
      if (n_grad != total)
        throw std::invalid_argument("ta_loss_gradient: expected room for " + std::to_string(total) + " values");
      if (dG_out) throw std::invalid_argument("ta_loss_gradient: dG_out is for the descriptor models");
      if (total == 0) return;
      if (ta::eam_nn_tables_on(h->eam)) HIP_CHECK(hipStreamSynchronize(h->stream));
      ta::eam_mark_trained(h->eam);  // exact networks from here on (see ta_energy_gradient)
      ta::eam_ensure(h->eam, h->db);
      compute_impl(h, TA_WANT_ENERGY, false, nullptr);  // rho, F', per-pair columns with the current weights
      hipStream_t s = h->stream;
      const size_t N = (size_t)h->db.n_atoms, F = (size_t)h->db.n_frames;
      h->train_grad.ensure((size_t)total + 8);
      h->train_coeff.ensure(F + 8);
      h->tan_dir.ensure(3 * N + 9 * F + 8);
      double *d_dR = h->tan_dir.ptr, *d_dh = h->tan_dir.ptr + 3 * N;
      if (dR) HIP_CHECK(hipMemcpyAsync(d_dR, dR, 3 * N * sizeof(double), hipMemcpyHostToDevice, s));
      if (dh) HIP_CHECK(hipMemcpyAsync(d_dh, dh, 9 * F * sizeof(double), hipMemcpyHostToDevice, s));
      if (frame_coeff && F)
        HIP_CHECK(hipMemcpyAsync(h->train_coeff.ptr, frame_coeff, F * sizeof(double), hipMemcpyHostToDevice, s));
      ta::eam_loss_gradient(h->eam, h->db, frame_coeff ? h->train_coeff.ptr : nullptr, dR ? d_dR : nullptr,
                            dh ? d_dh : nullptr, h->train_grad.ptr, s);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipMemcpyAsync(grad, h->train_grad.ptr, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
    });
  }
  if (h->kind != TA_MODEL_SF_MLP && h->kind != TA_MODEL_GRAP_MLP)
    return fail(h, TA_ERR_UNSUPPORTED, "ta_loss_gradient: the analytic force / stress term exists for the per-atom MLP models");
  // Per-pair buffers of this entry (tangents, Jacobian) are sized and walked by the resident
  // list's pair count. Under a Verlet skin the kernels run on the exact list extracted from it
  // (apply_filter: only the first pair_start[N] entries of the ex_* arrays are defined), so the two
  // do not match: refuse instead of reading the undefined tail. Training never needs a skin.
  if (h->filtered)
    return fail(h, TA_ERR_UNSUPPORTED, "ta_loss_gradient: not available on a skin-filtered batch; "
                                       "ta_set_skin(h, 0) and ta_set_frames first");
  return guarded(h, [&]() {
    int64_t total = 0;
    for (int e = 0; e < h->n_elements; ++e) total += ta::mlp_param_count(h->mlp[e]);
    if (n_grad != total)
      throw std::invalid_argument("ta_loss_gradient: expected room for " + std::to_string(total) + " values");
    mark_grap_trained(h);
    hipStream_t s = h->stream;
    const size_t N = (size_t)h->db.n_atoms, P = (size_t)h->db.n_pairs, F = (size_t)h->db.n_frames;
    const int D = h->sf.ndim;
    ensure_pair_jacobians(h);
    // direction -> pairs -> descriptors
    h->tan_dir.ensure(3 * N + 9 * F + 8);
    h->tan_dD.ensure(4 * P + 8);
    h->tan_dG.ensure(N * (size_t)D + 8);
    double *d_dR = h->tan_dir.ptr, *d_dh = h->tan_dir.ptr + 3 * N;
    if (dR) HIP_CHECK(hipMemcpyAsync(d_dR, dR, 3 * N * sizeof(double), hipMemcpyHostToDevice, s));
    else HIP_CHECK(hipMemsetAsync(d_dR, 0, 3 * N * sizeof(double), s));
    if (dh) HIP_CHECK(hipMemcpyAsync(d_dh, dh, 9 * F * sizeof(double), hipMemcpyHostToDevice, s));
    else HIP_CHECK(hipMemsetAsync(d_dh, 0, 9 * F * sizeof(double), s));
    ta::launch_pair_tangent(h->db, d_dR, d_dh, h->tan_dD.ptr, s);
    ta::launch_descriptor_jvp(h->db, D, h->jvp_J.ptr, h->tan_dD.ptr, h->tan_dG.ptr, s);
    size_t scratch = 0, partial = 0;
    for (int e = 0; e < h->n_elements; ++e) {
      const int n_el = h->db.elem_start[e + 1] - h->db.elem_start[e];
      scratch = std::max(scratch, ta::mlp_grad2_scratch_doubles(h->mlp[e], n_el));
      partial = std::max(partial, ta::mlp_grad_partial_doubles(h->mlp[e], n_el));
    }
    h->train_scratch.ensure(scratch + 8);
    h->train_partial.ensure(partial + 8);
    h->train_grad.ensure((size_t)total + 8);
    h->train_coeff.ensure(F + 8);
    if (frame_coeff && F)
      HIP_CHECK(hipMemcpyAsync(h->train_coeff.ptr, frame_coeff, F * sizeof(double), hipMemcpyHostToDevice, s));
    size_t off = 0;
    for (int e = 0; e < h->n_elements; ++e) {
      const int n_el = h->db.elem_start[e + 1] - h->db.elem_start[e];
      ta::launch_mlp_grad2(h->mlp[e], h->activation, D, h->db.elem_atoms + h->db.elem_start[e], n_el, h->db,
                           h->tan_dG.ptr, frame_coeff ? h->train_coeff.ptr : nullptr, h->train_scratch.ptr,
                           h->train_partial.ptr, h->train_grad.ptr + off, s);
      off += (size_t)ta::mlp_param_count(h->mlp[e]);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(grad, h->train_grad.ptr, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, s));
    if (dG_out && N)
      HIP_CHECK(hipMemcpyAsync(dG_out, h->tan_dG.ptr, N * (size_t)D * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  });
}

int ta_td_loss_gradient(ta_handle h, const double *coeff_free_energy, const double *coeff_energy,
                        const double *coeff_eentropy, const double *dR, const double *dh, double *grad,
                        int64_t n_grad, double *dG_out) {
  if (!h || !grad) return TA_ERR_INVALID;
  if (!h->td) return fail(h, TA_ERR_INVALID, "ta_td_loss_gradient: not a temperature-dependent model");
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "no resident batch");
  const bool direction = dR || dh;
  // the per-pair buffers of the direction follow the resident list (see ta_loss_gradient)
  if (direction && h->filtered)
    return fail(h, TA_ERR_UNSUPPORTED, "ta_td_loss_gradient: not available on a skin-filtered batch; "
                                       "ta_set_skin(h, 0) and ta_set_frames first");
  return guarded(h, [&]() {
    const int nel = h->n_elements;
    const int64_t total = ta::td_param_count(h->td_nets, nel);
    if (n_grad != total)
      throw std::invalid_argument("ta_td_loss_gradient: expected room for " + std::to_string(total) + " values");
    if (dG_out && !direction) throw std::invalid_argument("ta_td_loss_gradient: dG_out needs a direction");
    mark_grap_trained(h);
    hipStream_t s = h->stream;
    const size_t N = (size_t)h->db.n_atoms, P = (size_t)h->db.n_pairs, F = (size_t)h->db.n_frames;
    const int D = h->sf.ndim;
    if (direction) {
      ensure_pair_jacobians(h);
      h->tan_dir.ensure(3 * N + 9 * F + 8);
      h->tan_dD.ensure(4 * P + 8);
      h->tan_dG.ensure(N * (size_t)D + 8);
      double *d_dR = h->tan_dir.ptr, *d_dh = h->tan_dir.ptr + 3 * N;
      if (dR) HIP_CHECK(hipMemcpyAsync(d_dR, dR, 3 * N * sizeof(double), hipMemcpyHostToDevice, s));
      else HIP_CHECK(hipMemsetAsync(d_dR, 0, 3 * N * sizeof(double), s));
      if (dh) HIP_CHECK(hipMemcpyAsync(d_dh, dh, 9 * F * sizeof(double), hipMemcpyHostToDevice, s));
      else HIP_CHECK(hipMemsetAsync(d_dh, 0, 9 * F * sizeof(double), s));
      ta::launch_pair_tangent(h->db, d_dR, d_dh, h->tan_dD.ptr, s);
      ta::launch_descriptor_jvp(h->db, D, h->jvp_J.ptr, h->tan_dD.ptr, h->tan_dG.ptr, s);
    } else if (!h->descriptors_valid) {
      compute_impl(h, TA_WANT_ENERGY, false, nullptr);  // descriptors do not depend on the weights: once per batch
    }
    size_t scratch = 0, partial = 0;
    ta::td_grad2_sizes(h->td_nets, nel, h->td_K, h->db.elem_start, &scratch, &partial);
    h->train_scratch.ensure(scratch + 8);
    h->train_partial.ensure(partial + 8);
    h->train_grad.ensure((size_t)total + 8);
    h->train_coeff.ensure(3 * F + 8);
    // [a | b | g]: dL/dU_f, dL/dF_f, dL/dS_f; NULL = 0
    const double *host_coeff[3] = {coeff_energy, coeff_free_energy, coeff_eentropy};
    for (int q = 0; q < 3 && F; ++q) {
      double *dst = h->train_coeff.ptr + q * F;
      if (host_coeff[q]) HIP_CHECK(hipMemcpyAsync(dst, host_coeff[q], F * sizeof(double), hipMemcpyHostToDevice, s));
      else HIP_CHECK(hipMemsetAsync(dst, 0, F * sizeof(double), s));
    }
    ta::launch_td_grad2(h->td_dev, h->td_nets, nel, h->td_K, h->td_act, h->activation, h->td_sommerfeld ? 1 : 0, D,
                        h->db, h->td_T.ptr, direction ? h->tan_dG.ptr : nullptr, h->train_coeff.ptr,
                        h->train_scratch.ptr, h->train_partial.ptr, h->train_grad.ptr, s);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(grad, h->train_grad.ptr, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, s));
    if (dG_out && N)
      HIP_CHECK(hipMemcpyAsync(dG_out, h->tan_dG.ptr, N * (size_t)D * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
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
  if (h->filtered)  // see ta_loss_gradient
    return fail(h, TA_ERR_UNSUPPORTED, "ta_grap_loss_gradient: not available on a skin-filtered batch; "
                                       "ta_set_skin(h, 0) and ta_set_frames first");
  return guarded(h, [&]() {
    int64_t n_mlp = 0;
    for (int e = 0; e < h->n_elements; ++e) n_mlp += ta::mlp_param_count(h->mlp[e]);
    const int64_t n_filter = ta::grap_filter_param_count(h->grap);
    if (n_grad != n_mlp + n_filter)
      throw std::invalid_argument("ta_grap_loss_gradient: expected room for " + std::to_string(n_mlp + n_filter) +
                                  " values");
    const bool direction = dR || dh;
    mark_grap_trained(h);
    // descriptors, filter values (Hbuf) and dE/dG of the current weights and network
    compute_impl(h, TA_WANT_ENERGY, false, nullptr);
    hipStream_t s = h->stream;
    const size_t N = (size_t)h->db.n_atoms, P = (size_t)h->db.n_pairs, F = (size_t)h->db.n_frames;
    const int D = h->sf.ndim;
    h->tan_dir.ensure(3 * N + 9 * F + 8);
    h->tan_dD.ensure(4 * P + 8);
    h->tan_dG.ensure(N * (size_t)D + 8);
    // [pair vectors 4 P | kappa N D | the filter gradient's scratch]
    h->filt_scratch.ensure(4 * P + N * (size_t)D + ta::grap_filter_grad_doubles(h->grap, h->db) + 8);
    double *Dv = h->filt_scratch.ptr, *kappa = Dv + 4 * P, *fscratch = kappa + N * (size_t)D;
    ta::launch_pair_vec(h->db, Dv, s);
    if (direction) {
      double *d_dR = h->tan_dir.ptr, *d_dh = h->tan_dir.ptr + 3 * N;
      if (dR) HIP_CHECK(hipMemcpyAsync(d_dR, dR, 3 * N * sizeof(double), hipMemcpyHostToDevice, s));
      else HIP_CHECK(hipMemsetAsync(d_dR, 0, 3 * N * sizeof(double), s));
      if (dh) HIP_CHECK(hipMemcpyAsync(d_dh, dh, 9 * F * sizeof(double), hipMemcpyHostToDevice, s));
      else HIP_CHECK(hipMemsetAsync(d_dh, 0, 9 * F * sizeof(double), s));
      ta::launch_pair_tangent(h->db, d_dR, d_dh, h->tan_dD.ptr, s);
      // G-dot in one launch, by dual arithmetic through the forward expression
      ta::launch_grap_filter_tangent(h->grap, h->db, h->sf.eps, Dv, h->tan_dD.ptr, h->tan_dG.ptr, s);
    } else {
      HIP_CHECK(hipMemsetAsync(h->tan_dD.ptr, 0, 4 * P * sizeof(double), s));
      HIP_CHECK(hipMemsetAsync(h->tan_dG.ptr, 0, N * (size_t)D * sizeof(double), s));
    }
    // MLP part and kappa = c w + H_mlp G-dot: one second-order pass per element
    size_t scratch = 0, partial = 0;
    for (int e = 0; e < h->n_elements; ++e) {
      const int n_el = h->db.elem_start[e + 1] - h->db.elem_start[e];
      scratch = std::max(scratch, ta::mlp_grad2_scratch_doubles(h->mlp[e], n_el));
      partial = std::max(partial, ta::mlp_grad_partial_doubles(h->mlp[e], n_el));
    }
    h->train_scratch.ensure(scratch + 8);
    h->train_partial.ensure(partial + 8);
    h->train_grad.ensure((size_t)n_mlp + 8);
    h->train_coeff.ensure(F + 8);
    if (frame_coeff && F)
      HIP_CHECK(hipMemcpyAsync(h->train_coeff.ptr, frame_coeff, F * sizeof(double), hipMemcpyHostToDevice, s));
    if (N) HIP_CHECK(hipMemsetAsync(kappa, 0, N * (size_t)D * sizeof(double), s));
    size_t off = 0;
    for (int e = 0; e < h->n_elements; ++e) {
      const int n_el = h->db.elem_start[e + 1] - h->db.elem_start[e];
      ta::launch_mlp_grad2(h->mlp[e], h->activation, D, h->db.elem_atoms + h->db.elem_start[e], n_el, h->db,
                           h->tan_dG.ptr, frame_coeff ? h->train_coeff.ptr : nullptr, h->train_scratch.ptr,
                           h->train_partial.ptr, h->train_grad.ptr + off, s, kappa);
      off += (size_t)ta::mlp_param_count(h->mlp[e]);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(grad, h->train_grad.ptr, (size_t)n_mlp * sizeof(double), hipMemcpyDeviceToHost, s));
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
  if (h->filtered)  // see ta_loss_gradient
    return fail(h, TA_ERR_UNSUPPORTED, "ta_constant_gradient: not available on a skin-filtered batch; "
                                       "ta_set_skin(h, 0) and ta_set_frames first");
  return guarded(h, [&]() {
    const int64_t total = ta::eam_constant_count(h->eam);
    if (n_grad != total)
      throw std::invalid_argument("ta_constant_gradient: expected room for " + std::to_string(total) + " values");
    // positions, cells and the list's cutoff test as the inference kernels see them; models with nn functions
    // beside the analytic ones: the networks evaluated exactly (per-pair columns, F'), as for their own gradient
    if (ta::eam_param_count(h->eam) > 0) {
      if (ta::eam_nn_tables_on(h->eam)) HIP_CHECK(hipStreamSynchronize(h->stream));
      ta::eam_mark_trained(h->eam);
      ta::eam_ensure(h->eam, h->db);
    }
    compute_impl(h, TA_WANT_ENERGY, false, nullptr);
    hipStream_t s = h->stream;
    const size_t N = (size_t)h->db.n_atoms, F = (size_t)h->db.n_frames;
    h->train_grad.ensure((size_t)total + 8);
    h->train_coeff.ensure(F + 8);
    if (frame_coeff && F)
      HIP_CHECK(hipMemcpyAsync(h->train_coeff.ptr, frame_coeff, F * sizeof(double), hipMemcpyHostToDevice, s));
    double *d_dR = nullptr, *d_dh = nullptr;
    if (dR || dh) {
      h->tan_dir.ensure(3 * N + 9 * F + 8);
      d_dR = h->tan_dir.ptr;
      d_dh = h->tan_dir.ptr + 3 * N;
      if (dR) HIP_CHECK(hipMemcpyAsync(d_dR, dR, 3 * N * sizeof(double), hipMemcpyHostToDevice, s));
      else HIP_CHECK(hipMemsetAsync(d_dR, 0, 3 * N * sizeof(double), s));
      if (dh) HIP_CHECK(hipMemcpyAsync(d_dh, dh, 9 * F * sizeof(double), hipMemcpyHostToDevice, s));
      else HIP_CHECK(hipMemsetAsync(d_dh, 0, 9 * F * sizeof(double), s));
    }
    ta::eam_constant_gradient(h->eam, h->db, frame_coeff ? h->train_coeff.ptr : nullptr, d_dR, d_dh,
                              h->train_grad.ptr, s);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(grad, h->train_grad.ptr, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
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

int ta_hessian_vectors(ta_handle h, int32_t n_dir, int32_t first, const double *dR, const double *dh, double *dF,
                       double *dW) {
  if (!h || !dF || n_dir < 0) return TA_ERR_INVALID;
  if (h->td) return fail(h, TA_ERR_UNSUPPORTED, td_inference_only("ta_hessian_vectors"));
  if (h->kind == TA_MODEL_EAM_FS) return fail(h, TA_ERR_INVALID, fs_inference_only("ta_hessian_vectors"));
  if (!h->have_batch) return fail(h, TA_ERR_INVALID, "no resident batch");
  const bool grap_model = h->kind == TA_MODEL_GRAP_MLP;
  const bool sf_model = h->kind == TA_MODEL_SF_MLP || grap_model;  // the descriptor + MLP models
  if (sf_model) {
    if (h->filtered)
      return fail(h, TA_ERR_UNSUPPORTED, "ta_hessian_vectors: not available on a skin-filtered batch; "
                                         "ta_set_skin(h, 0) and ta_set_frames first");
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
  const size_t N = (size_t)h->db.n_atoms, F = (size_t)h->db.n_frames;
  const bool unit = !dR && !dh;
  if (unit && (first < 0 || (size_t)first + (size_t)n_dir > 3 * N))
    return fail(h, TA_ERR_INVALID, "ta_hessian_vectors: without dR / dh the directions are unit displacements "
                                   "first .. first + n_dir - 1 of the 3 N");
  if ((size_t)n_dir > 65535) return fail(h, TA_ERR_INVALID, "ta_hessian_vectors: at most 65535 directions per call");
  if (sf_model)
    return guarded(h, [&]() {
      // Per direction: D-dot per pair, G-dot through the pair Jacobians, w-dot = H_mlp G-dot from the
      // second-order MLP pass, then g and g-dot from the dual-arithmetic backward expression (ta_hvp.hip).
      if (n_dir == 0 || N == 0) return;
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
      size_t scratch = 0, partial = 0, total = 0;
      for (int e = 0; e < h->n_elements; ++e) {
        const int n_el = h->db.elem_start[e + 1] - h->db.elem_start[e];
        scratch = std::max(scratch, ta::mlp_grad2_scratch_doubles(h->mlp[e], n_el));
        partial = std::max(partial, ta::mlp_grad_partial_doubles(h->mlp[e], n_el));
        total += (size_t)ta::mlp_param_count(h->mlp[e]);
      }
      h->train_scratch.ensure(scratch + 8);
      h->train_partial.ensure(partial + 8);
      h->train_grad.ensure(total + 8);
      h->tan_dir.ensure(3 * N + 9 * F + 8);
      h->tan_dD.ensure(4 * P + 8);
      h->tan_dG.ensure(N * (size_t)D + 8);
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
        size_t off = 0;
        for (int e = 0; e < h->n_elements; ++e) {
          const int n_el = h->db.elem_start[e + 1] - h->db.elem_start[e];
          ta::launch_mlp_grad2(h->mlp[e], h->activation, D, h->db.elem_atoms + h->db.elem_start[e], n_el, h->db,
                               h->tan_dG.ptr, nullptr, h->train_scratch.ptr, h->train_partial.ptr,
                               h->train_grad.ptr + off, s, wdot);
          off += (size_t)ta::mlp_param_count(h->mlp[e]);
        }
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
        HIP_CHECK(hipMemcpyAsync(dF + d * 3 * N, fdot, 3 * N * sizeof(double), hipMemcpyDeviceToHost, s));
        if (dW) HIP_CHECK(hipMemcpyAsync(rows.data(), wrow, 9 * N * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));  // (the direction buffers are reused)
        if (dW) {
          std::fill(dW + d * F * 9, dW + (d + 1) * F * 9, 0.0);
          const std::vector<int32_t> &foa = h->hp.frame_of_atom;
          for (size_t i = 0; i < N; ++i)
            for (int k = 0; k < 9; ++k) dW[(d * F + (size_t)foa[i]) * 9 + k] += rows[9 * i + k];
        }
      }
    });
  return guarded(h, [&]() {
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
    ta::eam_hvp(h->eam, h->db, n_dir, unit, first, d_dR, d_dh, dFdot, fdot, wdot, extra, s);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(dF, fdot, nd * N * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    std::vector<double> wat;
    if (dW) {
      wat.resize(nd * N * 9);
      HIP_CHECK(hipMemcpyAsync(wat.data(), wdot, nd * N * 9 * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    HIP_CHECK(hipStreamSynchronize(s));
    if (dW) {  // per-frame sums of the per-atom rows, in atom order
      std::fill(dW, dW + nd * F * 9, 0.0);
      const std::vector<int32_t> &foa = h->hp.frame_of_atom;
      for (size_t d = 0; d < nd; ++d)
        for (size_t i = 0; i < N; ++i) {
          const size_t f = (size_t)foa[i];
          for (int k = 0; k < 9; ++k) dW[(d * F + f) * 9 + k] += wat[(d * N + i) * 9 + k];
        }
    }
  });
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
    buf.release();
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
