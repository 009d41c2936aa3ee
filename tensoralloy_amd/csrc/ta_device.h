// Device-side data structures and launcher declarations (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "ta_options.h"
#include "tensoralloy_amd.h"

namespace ta {

constexpr int kMaxRadial = 64;    // n_eta * n_omega
constexpr int kMaxElements = 8;
constexpr int kMaxBetaSlots = 3;  // H_beta slots in a pair record
constexpr int kRecDoubles = 8;    // pair record = 64 bytes
constexpr int kMaxLayers = 8;
constexpr int kCapMin = 192;      // pair records one v2 workgroup (one wavefront) stages in LDS
constexpr int kCapMax = 1024;
constexpr int kMaxCentersPerBlock = 16;  // centres one angular workgroup may own
constexpr int kMaxHd = 24;        // coefficients of the Hd(u) expansion
constexpr int kMlpStampRows = 16;  // ... atoms per workgroup of the MLP tile kernels (kMlpRows)
constexpr int kStampSlots = 10;   // -DTA_PHASE_STAMPS builds: stamps per angular workgroup (DeviceBatch::stamps)

// Symmetry-function constants, passed by value to every kernel.
struct SFParams {
  double rcut, acut;
  double inv_rc2, inv_ac2;  // 1 / rcut^2, 1 / acut^2
  double two_inv_ac2;       // 2 / acut^2 (du/dr = 2 r / acut^2: one scalar operand in the triple bodies)
  double eps;               // added under the square root (universal.py:470-472)
  double ang_scale;         // 0.5 when every {j,k} is visited twice (v1 kernels), else 1
  int n_elements;
  int n_rad;                // radial parameter combinations (eta x omega)
  int n_ang;                // angular parameter combinations (beta x gamma x zeta)
  int n_radial_dim;         // n_elements * n_rad
  int ndim;                 // descriptor length per atom
  int angular;
  int cutoff;               // TA_CUTOFF_*
  int n_beta;
  double eta[kMaxRadial], omega[kMaxRadial];
  double beta[kMaxBetaSlots];
  // Power chain of the radial exponentials: eta_pow[c] = k >= 2 when eta[c] = k eta[c - 1] exactly,
  // omega[c] = omega[c - 1] and c - 1 lies in the same group of four channels, so that
  // exp(-eta[c] x) = exp(-eta[c - 1] x)^k costs a few multiplications instead of an exponential
  // (the reference's default grid eta = {0.05, 4, 20, 80}: two exponentials instead of four);
  // 0 = evaluate the exponential.
  signed char eta_pow[kMaxRadial];
};

// One launch of the angular kernels handles NB x NG x NZ channels.
struct AngChunk {
  double beta[2];
  int hslot[2];      // which H slot of the pair record holds exp(-beta r^2/ac^2) fc(r)
  double gamma[2];
  double zeta[2];
  double kz[2];      // 2^(1 - zeta)
  int zeta_int[2];   // zeta as integer >= 1, or -1 when not an integer
  int chan[8];       // [(ib*NG + ig)*NZ + iz] -> channel index in [0, n_ang)
  int safe_pow;      // 1: the masked `safe_pow` of extension/grad_ops.py:16-66 for non-integer zeta
  int n_hd;          // 0 (exact), 12, 16 or 24 coefficients of Hd(u) = exp(-beta u) fc(u)
  double hd[kMaxHd]; // power-series coefficients in u (v2 kernels, beta[0] only)
};

struct BlockHeader;

struct DeviceBatch {
  int64_t n_atoms = 0, n_pairs = 0;
  int n_frames = 0, nnl_max = 0;
  // inputs
  double *pos = nullptr;         // [N][3]
  double *cells = nullptr;       // [F][9]
  int32_t *species = nullptr;    // [N]
  int32_t *frame_of_atom = nullptr;
  int32_t *atom_start = nullptr; // [F+1]
  int32_t *pair_start = nullptr; // [N+1]
  // [N] or null. Null: the pairs of centre i end where those of i + 1 begin. Set on the MD path
  // (ta_nlist.hip::nl_filter), whose exact list keeps every group of 16 centres at the group's offset
  // in the skin list (no prefix sum over the whole batch), so groups are separated by unused slots.
  int32_t *pair_stop = nullptr;
  int32_t *seg_start = nullptr;  // [N][nel+1]
  int32_t *pair_i = nullptr, *pair_j = nullptr, *pair_shift = nullptr, *pair_rev = nullptr;
  // MD path of the symmetry-function models: the exact list has no reverse index of its own; the reverse of
  // slot p is rev_map[rev_super[slot_q[p]]] (slot -> skin-list pair -> its reverse there -> that pair's slot),
  // looked up by the one kernel that needs it (force_gather) instead of a launch that writes it out
  const int32_t *slot_q = nullptr, *rev_super = nullptr, *rev_map = nullptr;
  int32_t *blk_center = nullptr; // [n_blk+1] first centre of every v2 workgroup
  // [n_blk] what a second-generation angular workgroup needs to know about its run, written by whoever
  // writes blk_center (see BlockHeader); the GRAP and first-generation kernels and ta_get_list read blk_center
  const BlockHeader *blk_hdr = nullptr;
  int n_blk = 0;
  // MD step (ta_nlist.hip::filter_group_kernel): > 0 = number of groups of 16 centres, each owning 16
  // run slots of which the later ones are usually empty. Workgroup b then takes slot
  // 16 (b mod groups) + b / groups, so that the slots in use come first in launch order (interleaved
  // with the empty ones they ran on half of the shader engines: 48 -> 77 us for the forward kernel)
  int blk_groups = 0;
  const int32_t *n_blk_dev = nullptr;  // MD loop: the packing was made on the device, `n_blk` is only an upper
                                       // bound of the grid; workgroups beyond *n_blk_dev leave at once
  int cap = kCapMin;             // records per v2 workgroup (multiple of 64)
  int32_t *elem_atoms = nullptr; // atoms grouped by element
  int32_t elem_start[kMaxElements + 1] = {0};

  // work buffers
  double *rec = nullptr;    // [P][8]  {Dx,Dy,Dz,r2,1/r,H0,H1,H2}
  double *rec4 = nullptr;   // [P][4]  {Dx,Dy,Dz,r2}: compact records of the second-generation angular,
                            // GRAP and EAM / ADP paths (set instead of `rec`: half the record traffic
                            // of the forward, backward and gather kernels; 1/r is recomputed)
  double *part4 = nullptr;  // [nel*n_ang][P] per-pair partial angular sums
  unsigned long long *masks = nullptr;  // [ceil(nnl_max/128)][P] candidate masks, forward -> backward
  // Lane balance of the angular kernels: the forward kernel cuts every lane's 64 candidate positions
  // into four windows of 16, makes every non-empty window a job, sorts the jobs by size and leaves
  // the list here for the backward kernel: per workgroup `job_count[blk]` words at
  // [blk * job_stride ..): bits 0-7 the pair (item of the workgroup), bits 8-9 the window, bits
  // 16-31 the window's candidate bits. null: the per-lane masks above are used.
  uint32_t *job_word = nullptr;
  int32_t *job_count = nullptr;
  int job_stride = 0;
  // Triangle-once backward (one-element default-grid builds, see owns_triangle): the forward kernel
  // also leaves the list restricted to the triangles the centre owns, in the same word format and at
  // the same place per workgroup; job_count_own[blk] = -1: no list (the backward kernel then tests
  // ownership per triple). null: not made in this evaluation.
  uint32_t *job_word_own = nullptr;
  int32_t *job_count_own = nullptr;
  double *G = nullptr;      // [N][D]
  double *dEdG = nullptr;   // [N][D]
  double *eatom = nullptr;  // [N]
  double *g = nullptr;      // [P][4]  dE/dD per directed pair (x, y, z, pad)
  double *forces = nullptr; // [N][3]
  double *wat = nullptr;    // [N][9] per-atom virial (only atoms of groups that straddle two frames)
  // Per-atom own-side sums {sum_p g[p] (3), sum_p g[p] (x) D[p] (9)} over the atom's pairs, left by the
  // GRAP backward kernel (one wavefront per centre: nearly free there); force_gather then only gathers
  // g[rev p]. `own_sums` != 0: valid for this evaluation. (The angular backward kernel does not: its
  // per-centre reduction cost what the gather saved, profiles/r02_tuning_notes.md.)
  double *fown = nullptr;
  int own_sums = 0;
#ifdef TA_PHASE_STAMPS
  // diagnostic builds only (scripts/phase_stamps.sh): s_memrealtime (100 MHz) at the phase boundaries
  // of the angular kernels, [kernel 0 / 1][workgroup][kStampSlots]
  unsigned long long *stamps = nullptr;
  // ... and of the 16-row MLP tile kernels, [workgroup][kStampSlots] (ta_mlp.hip::TA_MLP_STAMP)
  unsigned long long *mlp_stamps = nullptr;
#endif
  double *bpart = nullptr;  // [ceil(N / 16)][10] {E, W[9]} of every group of 16 consecutive atoms
  double *energy = nullptr; // [F]
  double *virial = nullptr; // [F][9]
  double *batch_energy = nullptr;  // [1]
};

// One run of the angular workgroup packing (a run slot of `blk_center`) as ONE 64-byte record, so that a
// workgroup learns its centres, its pairs and every centre's first pair with a single (scalar) load
// instead of the chain blk_center -> pair_start -> pair_i -> pair_start / pair_stop, each link one L2
// round trip that nothing in the workgroup can proceed past. Written with the packing, by
// make_block_header; nothing in it changes between the packing and the evaluation.
struct alignas(64) BlockHeader {
  int32_t c0;        // first centre of the run
  int32_t info;      // bits 0-7: centres of the run, 0 = unused run slot; kHdrOnePass
  int32_t s0;        // first pair of the run in the list
  int32_t M;         // pairs of the run (<= cap <= kCapMax)
  uint16_t rel[24];  // rel[k], k <= centres: first pair of centre c0 + k relative to s0; M from `centres` on
};
static_assert(sizeof(BlockHeader) == 64, "one 64-byte record per run slot");
static_assert(kMaxCentersPerBlock + 1 <= 24 && kCapMax < (1 << 16), "16-bit entries, one per centre and the end");
// every pair of the run has a lane (M <= workgroup size) and every centre's rotation schedule fits one
// 64-bit candidate mask (n / 2 <= 64): the angular kernels take their single-scan paths
constexpr int32_t kHdrOnePass = 1 << 8;

// `count(k)`: pairs of centre c0 + k; `block`: lanes of an angular workgroup, min(cap, 256)
template <class CountFn>
__host__ __device__ inline void make_block_header(BlockHeader &h, int c0, int ncent, int s0, int block, CountFn count) {
  int m = 0;
  bool wide = false;
  for (int k = 0; k < 24; ++k) {
    h.rel[k] = (uint16_t)m;
    if (k < ncent) {
      const int n = count(k);
      wide = wide || (n >> 1) > 64;
      m += n;
    }
  }
  h.c0 = c0;
  h.s0 = s0;
  h.M = m;
  h.info = ncent | ((ncent > 0 && m <= block && !wide) ? kHdrOnePass : 0);
}

// What a workgroup of the angular backward kernel needs before its staging barrier, as the FIRST kernel
// parameter: one 64-byte line of the argument segment, read in one round of scalar loads (two 32-byte loads and
// one wait) at the kernel's top, so that the header load, the dE/dG loads of the coefficient tables and the job
// words are issued after ONE argument round trip. SFParams, AngChunk and DeviceBatch stay as parameters for
// everything that is needed later. Filled by the launcher from DeviceBatch (make_launch_head), never kept anywhere.
// (The forward kernel keeps its parameters: the same head measured nothing there, profiles/launch_head_notes.md.)
struct alignas(64) LaunchHead {
  const BlockHeader *blk_hdr;
  const int32_t *n_blk_dev;   // DeviceBatch::n_blk_dev; no launch of this library sets it today (always null)
  const int32_t *job_count;   // the list the launch reads: DeviceBatch::job_count or job_count_own
  const uint32_t *job_word;   // likewise job_word or job_word_own
  const double *dEdG;
  const int32_t *pair_j;
  int32_t blk_groups;
  int32_t flags;              // the launch's flag word (was the last kernel parameter)
  int32_t ndim;               // SFParams::ndim
  uint32_t stride_nrad;       // bits 0-15 DeviceBatch::job_stride, bits 16-23 SFParams::n_rad
};
static_assert(sizeof(LaunchHead) == 64 && alignof(LaunchHead) == 64, "one line of the argument segment");
static_assert(std::is_trivially_copyable<LaunchHead>::value && std::is_standard_layout<LaunchHead>::value,
              "passed by value in the argument segment");
static_assert(4 * kCapMax < (1 << 16) && kMaxRadial < (1 << 8), "job_stride and n_rad share a word");

// Ownership of an angular triangle. A triangle {i, j, k} of three DISTINCT atoms (all three sides
// below acut) is evaluated once in the backward pass, by one of its vertices: with the indices sorted,
// a < b < c, the owner is the one at rank t(a + b + c) in {0, 1, 2}, a multiplicative hash of the
// (symmetric) index sum. Every vertex reaches the same owner from its own view, and a centre's
// triangles spread over all three ranks, so every centre owns about a third of its triangles ("the
// smallest index owns" would give some centres all of theirs and others none). The atoms are distinct
// whenever every periodic cell width exceeds acut: two images of one atom are at least one width apart.
// (Fibonacci hashing modulo 2^24: 24-bit multiplications, full rate on the device)
__host__ __device__ inline int triangle_owner_rank(uint32_t index_sum) {
#ifdef __HIP_DEVICE_COMPILE__
  const uint32_t h = __umul24(index_sum, 0x9E3779u);
#else
  const uint32_t h = index_sum * 0x9E3779u;  // the same low 24 bits
#endif
  return (int)(((h & 0xFFFFFFu) * 3u) >> 24);
}
// centre i owns the triangle {i, j, k}
__host__ __device__ inline bool owns_triangle(int32_t i, int32_t j, int32_t k) {
  return triangle_owner_rank((uint32_t)i + (uint32_t)j + (uint32_t)k) == (j < i ? 1 : 0) + (k < i ? 1 : 0);
}

// end of centre i's pairs (see DeviceBatch::pair_stop)
#ifdef __HIPCC__
__device__ __forceinline__ int pair_stop_of(const DeviceBatch &b, int64_t i) {
  return b.pair_stop ? b.pair_stop[i] : b.pair_start[i + 1];
}
#endif

// {Dx, Dy}, {Dz, r^2} of pair q, from the compact or the full record
#ifdef __HIPCC__
__device__ __forceinline__ int pair_rev_of(const DeviceBatch &b, int q) {
  return b.slot_q ? b.rev_map[b.rev_super[b.slot_q[q]]] : b.pair_rev[q];
}
__device__ __forceinline__ const double2 *pair_geom(const DeviceBatch &b, size_t q) {
  return reinterpret_cast<const double2 *>(b.rec4 ? b.rec4 + 4 * q : b.rec + kRecDoubles * q);
}
// 16-byte write-through stores (the `sc1` cache policy) for bulk data that only a LATER kernel reads: the
// line goes to memory at once and does not stay dirty in the writing XCD's L2, so the release at the
// kernel's end has nothing of it left to write back. Only the 16-byte form: narrower write-through stores
// cost several times as much per byte. `base` and `bytes` must be wave-uniform (they become the buffer
// descriptor, in scalar registers); stores at or beyond `bytes` are dropped by the range check.
struct WtSlice {
  __amdgpu_buffer_rsrc_t rsrc;
};
__device__ __forceinline__ WtSlice wt_slice(void *base, uint32_t bytes) {
  WtSlice s;
  s.rsrc = __builtin_amdgcn_make_buffer_rsrc(base, 0, (int)bytes, 0x00020000);
  return s;
}
__device__ __forceinline__ void wt_store16(const WtSlice &s, uint32_t byte_offset, double2 v) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const u32x4 w = {(uint32_t)__double2loint(v.x), (uint32_t)__double2hiint(v.x), (uint32_t)__double2loint(v.y),
                   (uint32_t)__double2hiint(v.y)};
  __builtin_amdgcn_raw_buffer_store_b128(w, s.rsrc, (int)byte_offset, 0, 16);  // aux 16 = sc1
}
#endif
// When a launch stores its hand-over data write-through: while all of it (32 bytes per pair) would fit in the
// eight 4 MB L2s and so stay dirty until the kernel's end. A larger batch evicts most of its output while it
// runs, nothing is left for the boundary, and plain stores are the cheaper ones there.
constexpr size_t kWtMaxBytes = (size_t)32 << 20;
inline bool wt_handover(const DeviceBatch &b) { return 32 * (size_t)b.n_pairs <= kWtMaxBytes; }

// Per-element MLP on the device: padded weights, both orientations.
struct MlpLayerDev {
  int k, n;        // logical in / out
  int kp, np;      // padded: kp % 4 == 0, np % 16 == 0
  double *w;       // [kp][np]
  double *wt;      // [np][kp]
  double *b;       // [np]
  int act;         // apply activation
  int res;         // resnet skip
};
struct MlpDev {
  int n_layers = 0;  // incl. output layer
  MlpLayerDev layer[kMaxLayers];
  double *xlo = nullptr, *xhi = nullptr;  // [D] or null
  int max_np = 0, max_kp = 0;
};

// What the per-atom network launch of an evaluation was (ta_mlp_launch_info): host bookkeeping written
// where the launch is issued, never read by the dispatch. `family` is a TA_MLP_* and `da` a TA_MLP_DA_* constant of tensoralloy_amd.h.
struct MlpLaunchInfo {
  int family = 0;   // TA_MLP_NONE = nothing launched
  int threads = 0;  // workgroup size
  int lh = 0;       // hidden layers of the wave / quad build, else 0
  int nt = 0;       // wavefronts per tile of the quad build, else 0
  int grid_x = 0, grid_y = 0;
  long long lds_bytes = 0;  // dynamic LDS of one workgroup
  int da = 0;               // where act' lived
  int body = 0;             // TA_MLP_BODY_*: which body a tile launch ran (ta_mlp_tile_body)
};

void launch_pair_geometry(const SFParams &sf, const DeviceBatch &b, hipStream_t s);
void launch_g4_forward(const SFParams &sf, const AngChunk &ch, int nb, int ng, int nz,
                       const DeviceBatch &b, hipStream_t s);
void launch_descriptor_reduce(const SFParams &sf, const DeviceBatch &b, hipStream_t s);
void launch_mlp(const SFParams &sf, const MlpDev &mlp, int activation, int element,
                const DeviceBatch &b, hipStream_t s);
void launch_backward(const SFParams &sf, const AngChunk &ch, int nb, int ng, int nz,
                     bool first, bool radial_only, const DeviceBatch &b, hipStream_t s);
void launch_force_gather(const SFParams &sf, const DeviceBatch &b, int gather_w, hipStream_t s);  // Options::gather_w
void launch_frame_reduce(const DeviceBatch &b, bool want_virial, double *mirror, int64_t n_tail, hipStream_t s);

size_t g4_lds_bytes(int nnl_max);

// second-generation angular kernels (ta_kernels_v2.hip); `ch` holds one beta
size_t v2_lds_bytes(bool backward, int cap, int n_local = 0, int nspec = 0, bool triangles = false);
int v2_job_stride(int cap);
// `reduce`: last forward launch of an evaluation, also assembles the descriptor vectors
// `full_list_unread`: no backward launch of this evaluation reads DeviceBatch::job_word (every one of them
// takes the triangle build and reads job_word_own): the launch leaves job_count[blk] = -1 and no full list.
// Honoured only where the launch makes the owned lists.
void launch_g4_forward_v2(const SFParams &sf, const AngChunk &ch, int ng, int nz, bool geometry,
                          bool reduce, bool full_list_unread, const DeviceBatch &b, const Options &opt, hipStream_t s);
// Whether launch_backward_v2(.., triangles = true, ..) takes the triangle-once build for this chunk: one
// element, the default zeta grid {1, 4}, an Hd series of 12 or 16 coefficients
bool v2_backward_takes_triangles(const SFParams &sf, const AngChunk &ch, int ng, int nz);
// `triangles`: one-element default-grid chunks take the triangle-once build (b.job_word_own made by the
// forward launch, or ownership tested per triple). Returns the build used: 1 per apex, 2 triangles.
int launch_backward_v2(const SFParams &sf, const AngChunk &ch, int ng, int nz, bool first, bool triangles,
                       const DeviceBatch &b, const Options &opt, hipStream_t s);

// device-side neighbour list (ta_nlist.hip)
struct NlGrid {  // linked-cell grid of one frame, in fractional coordinates
  double h[9];
  double hinv[9];
  double lo[3];     // lower edge of the grid (0 on periodic axes)
  double inv_w[3];  // bins per unit of fractional coordinate
  int32_t nb[3];
  int32_t pbc[3];
  int32_t bin_offset;  // first bin of this frame in the batch-wide bin arrays
  int32_t pad_;
  // neighbouring bins looked at along each axis: offsets -m .. m (1 unless the cell is thinner than the
  // cutoff along a periodic axis: then nb = 1 there and m = floor(rmax / height) + 1 images of the one bin)
  int32_t m[3];
  int32_t ortho;    // cell vectors mutually orthogonal: the per-axis gaps to a bin add in quadrature
  double bw[3];     // perpendicular (Cartesian) width of one bin along each axis; 0 = unknown, no pruning
};
struct NlRec {  // one atom, stored in bin order
  double x, y, z;
  int32_t wx, wy, wz;  // integer wrap into the cell
  int32_t j;           // atom index
  int32_t sp;          // species
  int32_t pad_;
};
struct NlWork {  // device work buffers, sized by the caller
  int32_t *wrap;        // [3 N] integer wrap of each atom into its cell
  int32_t *binid;       // [N]
  int32_t *bin_count;   // [n_bins + 1]
  int32_t *bin_start;   // [n_bins + 1]
  int32_t *bin_cursor;  // [n_bins + 1]
  int32_t *bin_atoms;   // [N]
  NlRec *recs;          // [N]
  int32_t *counts;      // [N (nel + 1) + 1]
  int32_t *seg_start;   // [N (nel + 1) + 1]
  // 8 words. stats[0] = number of triples; as int32: [2] nnl_max, [4] number of pairs (32-bit scan
  // total), [6] pairs without a reverse partner (must stay 0); stats[4] = number of pairs, 64-bit
  unsigned long long *stats;
};
bool nl_make_grid(const ta_frame &fr, double rmax, int bin_offset, NlGrid &g);
int nl_bins(const NlGrid &g);
void nl_count(int n_atoms, int n_bins, int nel, double rmax, const double *pos, const int32_t *species,
              const int32_t *frame_of_atom, const NlGrid *grids, NlWork &w, int32_t *pair_start,
              hipStream_t s);
size_t nl_build_zero_words(int n_atoms, int n_bins);
void nl_build(int n_atoms, int n_bins, int nel, double rmax, const double *pos, const int32_t *species,
              const int32_t *frame_of_atom, const NlGrid *grids, NlWork &w, unsigned long long *zero,
              bool zero_is_clean, long long capacity, int32_t *pair_start, int32_t *host_pair_start,
              int32_t *pair_i, int32_t *pair_j, int32_t *pair_shift, int32_t *pair_rev, long long rev_cover,
              hipStream_t s);
void nl_reverse_sorted(int64_t n_pairs, int nel, const int32_t *species, const int32_t *seg_start,
                       const int32_t *pair_i, const int32_t *pair_j, const int32_t *pair_shift,
                       int32_t *pair_rev, unsigned long long *stats, hipStream_t s);
int nl_filter_blocks(int n_atoms);
void nl_filter(int n_atoms, int64_t n_super, int nel, double rmax, const double *pos, const double *cells,
               const int32_t *frame_of_atom, const int32_t *start_super, const int32_t *seg_super,
               const int32_t *pj_super, const int32_t *ps_super, const int32_t *rev_super, int32_t *map,
               int32_t *seg_exact, int32_t *pair_start, int32_t *pair_stop, int32_t *pi_out, int32_t *pj_out,
               int32_t *ps_out, int32_t *rev_out, int32_t *slot_q, int cap, int32_t *blk_center, BlockHeader *blk_hdr,
               hipStream_t s);
void nl_fill(int n_atoms, int64_t n_pairs, int nel, double rmax, const double *pos,
             const int32_t *species, const int32_t *frame_of_atom, const NlGrid *grids, NlWork &w,
             int32_t *pair_i, int32_t *pair_j, int32_t *pair_shift, int32_t *pair_rev, hipStream_t s);

}  // namespace ta
