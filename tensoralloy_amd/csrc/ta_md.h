// Arguments of the MD integrator launch (ta_md.hip), filled by ta_md_run (ta_api_md.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ta {

constexpr int kMdChunk = 1024;      // atoms per workgroup without Berendsen scaling (256 threads, 4 atoms each)
constexpr int kMdLookahead = 4;     // steps ta_md_run enqueues between two looks at the status word
constexpr int kMdMaxChain = 8;      // TA_MD_MAX_CHAIN: slots per frame of the Nose-Hoover chain arrays

struct MdLaunch {
  double *pos;                // [N][3] db.pos, caller's atom order
  double *vel;                // [N][3]
  const double *forces;       // [N][3] of the evaluation before this launch
  const double *mass;         // [N]
  const double *ref;          // [N][3] positions the resident list was built for
  const double *energy;       // [F] frame energies of the evaluation before this launch
  const int32_t *atom_start;  // [F + 1]
  const int32_t *blk_start;   // [F + 1] first workgroup of each frame
  double *epot;               // [n_rec][F]
  double *ke_part;            // [n_rec][n_blk]
  unsigned *status;           // device word: 0, or 1 + seq of the launch whose drift left the list stale
  unsigned *status_host;      // the same, page-locked
  double dt, kT0, dt_over_tau;
  double lim2;                // skin^2 / 4; negative: every drift is stale (skin = 0)
  long long rec;              // record slot, -1: none
  unsigned seq;               // steps of this run before this launch
  int n_frames, n_blk, chunk;
  int kick2;                  // the second half-kick is pending
  int drift;                  // 0: only finish the step (last launch of a run)
  // Langevin (langevin != 0; kT0 is then the bath's, and no Berendsen factor is applied): the absolute
  // index of the step this launch begins (steps integrated since ta_md_init before it), the key of the
  // noise, and the parts of ASE's c1 .. c5 that do not depend on the atom:
  //   c1 = dt/2 - dt^2 fr/8, c2 = dt fr/2 - dt^2 fr^2/8, c3_i = c3 / sqrt(m_i), likewise c4_i and c5_i
  int langevin;
  long long step;
  unsigned long long seed;
  double c1, c2, c3, c4, c5;
  // Barostat (baro != 0; every workgroup is then a whole frame): db.cells and the frame virials of the
  // evaluation before this launch, the cumulative scale s_c since the list was built, the record
  // {V, P_x, P_y, P_z}, the target pressure, k = (dt / taup) (beta / 3), the free axes (read unless
  // baro_iso), and skin and rc + skin of the strain-aware list test (which replaces lim2)
  int baro, baro_iso;
  double *cells;              // [F][9]
  const double *virial;       // [F][9]
  double *baro_scale;         // [F][3]
  double *baro_rec;           // [n_rec][F][4]
  double baro_p0, baro_k;
  int baro_mask[3];
  double skin, r_list;
  // Nose-Hoover chain (nhc != 0; every workgroup is then a whole frame, kT0 above is 0): the target, tau^2
  // kT0 (Q_k for k >= 2; Q_1 = g Q_k with g = 3 n - nhc_dof), chain length M and loops L of a half-update,
  // the chain state [F][kMdMaxChain] and the record of the chain terms of H'
  int nhc, nhc_chain, nhc_loops, nhc_dof;
  double nhc_kT0, nhc_q;
  double *nhc_eta, *nhc_veta;  // [F][kMdMaxChain]
  double *nhc_rec;             // [n_rec][F]
  // Sampling (ta_md_set_sampling): this sample's rows [N][3] of the position and the velocity ring, both null
  // in a launch that does not sample (the launcher picks the kSnap build from them). x(t) is stored before the
  // drift, v(t) as the record's kinetic energy sees it.
  double *snap_x, *snap_v;
};

// What the Martyna-Tobias-Klein launch (ta_md_mtk.hip) takes beside an MdLaunch with baro = nhc = 1 and every
// workgroup a whole frame (n_blk = n_frames): the strain rates, the barostat's chain and the record of E_baro, the
// target pressure, kT0 taup^2 (Q'_k for k >= 2; Q'_1 = d_b Q'_k, W_c = (g + 3) Q'_k / 3), chain length and loops of
// a half-update of the barostat's chain, and the free axes (read unless iso). MdLaunch's baro_p0, baro_k, baro_iso
// and baro_mask are not read.
struct MdMtkLaunch {
  double *omega;      // [F][3]
  double *xi, *vxi;   // [F][kMdMaxChain]
  double *rec;        // [n_rec][F]
  double p0, q;
  int chain, loops, iso;
  int mask[3];
};

constexpr int kMdCorrChunk = 768;  // ring doubles (256 atoms x 3) per workgroup of the correlation launch
constexpr int kMdCorrLagTile = 8;   // lags per workgroup of the correlation launch

// Arguments of the correlation launch (ta_md_corr.hip) that ta_md_run puts behind an integrator launch that
// sampled: sample n (in ring slot n % n_lags) against the rows of the lags 0 .. min(n, n_lags - 1).
struct MdCorrLaunch {
  const double *ring_x, *ring_v;  // [n_lags][N][3]
  const int32_t *species;         // [N]
  const int32_t *atom_start;      // [F + 1]
  const int32_t *blk_start;       // [F + 1] first chunk of kMdCorrChunk ring doubles of each frame (at least one each)
  double *part;                   // [n_chunks][2][E][n_lags] per-workgroup sums: v . v, then |dx|^2
  double *acc_v, *acc_x;          // [F][E][n_lags] the accumulators
  const unsigned *status;         // the integrator's status word and
  unsigned seq;                   // sequence number: the same predicate
  long long n;                    // index of the newest sample
  long long n_atoms;              // N
  int n_lags, n_elements, n_frames, n_chunks;
};

// What every launch that sweeps the resident (skin) list takes, as the first member `list` of its arguments: the
// whole-step state and the list (taken at every launch: a rebuild may have moved them), the integrator's predicate,
// and the launch's plan of `chunk` consecutive centres of one frame per workgroup (fixed for a run). The device
// functions on it are in ta_md_sweep.h.
struct MdList {
  const double *pos;              // [N][3] db.pos
  const double *cells;            // [F][9]
  const int32_t *species;         // [N]
  const int32_t *atom_start;      // [F + 1]
  const int32_t *blk_start;       // [F + 1] first workgroup of each frame (at least one each)
  const int32_t *pair_start;      // [N + 1] the resident list: centre i owns pair_start[i] .. pair_start[i + 1] - 1
  const int32_t *pair_j;          // [P]
  const int32_t *pair_shift;      // [P][3]
  const unsigned *status;         // the integrator's status word and
  unsigned seq;                   // sequence number: the same predicate
  int n_elements, n_frames, n_blk, chunk;
};

constexpr int kMdRdfLdsWords = 8192;  // most 32-bit bins of the pair-distribution launch's LDS histogram (32 KB)

// Centres per workgroup of the pair-distribution launch for a batch of n_atoms: small batches spread over the
// chip, large ones merge fewer histograms (the plan, blk_start, is made once by ta_md_set_rdf)
inline int md_rdf_chunk(long long n_atoms) { return n_atoms <= 16384 ? 8 : 64; }

// Arguments of the pair-distribution launch (ta_md_rdf.hip) that ta_md_run puts in front of the integrator
// launch of a sampled step: the resident (skin) list, the positions and cells of that whole-step state.
struct MdRdfLaunch {
  MdList list;
  const int32_t *pair_i;          // [P] the centre of every pair
  unsigned long long *counts;     // [F][E][E][n_bins] the accumulators
  int n_bins;
  double dr;                      // r_max / n_bins
};

constexpr int kMdAdfLdsWords = 8192;  // most 32-bit bins of the bond-angle launch's LDS histogram (32 KB)
constexpr int kMdAdfSlab = 128;       // neighbours a wave of the bond-angle launch holds in LDS at a time

// Centres per workgroup (four waves, one centre each at a time) of the bond-angle launch for a batch of n_atoms:
// small batches spread over the chip, large ones merge fewer histograms (the plan, blk_start, is made once by
// ta_md_set_adf)
inline int md_adf_chunk(long long n_atoms) { return n_atoms <= 16384 ? 8 : 64; }

// Arguments of the bond-angle launch (ta_md_adf.hip) that ta_md_run puts in front of the integrator launch of a
// sampled step: the resident (skin) list, the positions and cells of that whole-step state.
struct MdAdfLaunch {
  MdList list;
  const double *rb2;              // [E][E] squares of the bond cutoffs
  unsigned long long *counts;     // [F][E][E (E + 1) / 2][n_bins] the accumulators
  int n_bins;
  double dtheta;                  // pi / n_bins
};

constexpr int kMdOrderLdsWords = 8192;   // most 32-bit bins of the order launch's LDS histogram of q and q-bar (32 KB)
constexpr int kMdOrderMaxDegrees = 4;    // TA_MD_ORDER_MAX_DEGREES
constexpr int kMdOrderMaxL = 12;         // TA_MD_ORDER_MAX_L
constexpr int kMdOrderMaxConn = 31;      // TA_MD_ORDER_MAX_CONN
constexpr int kMdOrderMaxLm = 46;        // most (l, m >= 0) of a setting: degrees 12, 11, 10, 9
constexpr int kMdOrderMaxChunk = 64;     // most centres of a workgroup (their values wait in LDS for the binning)

// Centres per workgroup (four waves, one centre each at a time) of the two order launches for a batch of n_atoms:
// small batches spread over the chip, large ones merge fewer histograms (the plan, blk_start, is made once by
// ta_md_set_order). 64 centres keep a workgroup's LDS (32 KB of bins, 4.5 KB of per-atom values, 6 KB of wave
// sums) at 43 KB: three workgroups of four waves fit the 160 KB of a compute unit.
inline int md_order_chunk(long long n_atoms) { return n_atoms <= 16384 ? 8 : kMdOrderMaxChunk; }

// Arguments of the two bond-orientational order launches (ta_md_order.hip) that ta_md_run puts in front of the
// integrator launch of a sampled step, in stream order: the resident (skin) list, the positions and cells of that
// whole-step state. Pass 1 writes qlm and n_bonds, pass 2 reads them and writes everything else.
struct MdOrderLaunch {
  MdList list;
  const double *rb2;              // [E][E] squares of the bond cutoffs
  const double *norm;             // [n_lm] N_lm of every (degree, m >= 0), degree by degree
  double *qlm;                    // [N][n_lm][2] q_lm of the newest sample
  double *q, *qbar;               // [N][n_degrees]
  int32_t *n_bonds, *n_conn;      // [N]
  unsigned long long *hist_q, *hist_qbar;  // [F][E][n_degrees][n_bins] the accumulators
  unsigned long long *hist_conn;           // [F][E][kMdOrderMaxConn + 1]
  int n_bins;
  int n_degrees, n_lm, solid;    // solid: index of solid_degree among the degrees
  int deg0, deg1, deg2, deg3;     // the degrees (0 beyond n_degrees)
  double threshold;               // c of the solid-bond test
};

constexpr int kMdClusterLdsWords = 4096;  // 32-bit bins of the cluster summary's LDS histogram (16 KB): TA_MD_MAX_BINS, no tiling

// Arguments of the four cluster launches (ta_md_cluster.hip) that ta_md_run puts in front of the integrator launch
// of a sampled step, behind the order launches of that step and in stream order: select, link, flatten, summarise.
// The link launch has the workgroup layout of the order launches (md_order_chunk); select and flatten take a thread
// per atom, the summary a workgroup per frame.
struct MdClusterLaunch {
  MdList list;
  const double *rl2;              // [E][E] squares of the link cutoffs
  const int32_t *n_conn;          // [N] of the order launches for the same state; read when n_min > 0
  int32_t *parent, *count;        // [N] the union-find forest (-1: not selected) and the atoms under every root
  int32_t *label, *size;          // [N] of the newest sample
  unsigned long long *hist;       // [F][n_bins] the accumulator
  long long *row;                 // [F][4] this sample's row of the series
  unsigned *giveup;               // set when a loop overran its cap
  long long n_atoms;              // N
  int n_bins;
  int n_min, species_mask;
};

constexpr int kMdCnaTypes = 5;  // TA_MD_CNA_TYPES, OVITO's numbering:
constexpr int kMdCnaOther = 0, kMdCnaFcc = 1, kMdCnaHcp = 2, kMdCnaBcc = 3, kMdCnaIco = 4;
constexpr int kMdCnaAdaptive = 0, kMdCnaFixed = 1;  // TA_MD_CNA_ADAPTIVE, TA_MD_CNA_FIXED

// Arguments of the common neighbour analysis (ta_md_cna.hip) that ta_md_run puts in front of the integrator launch of
// a sampled step, behind the order and cluster launches of that step: a launch that zeroes this sample's row of the
// series and the analysis itself, which has the workgroup layout of the order launches (md_order_chunk).
struct MdCnaLaunch {
  MdList list;
  int32_t *structure;             // [N] of the newest sample
  double *r_local;                // [N] likewise
  unsigned long long *counts;     // [F][E][kMdCnaTypes] the accumulator
  unsigned long long *row;        // [F][kMdCnaTypes] this sample's row of the series
  int mode;                       // kMdCnaAdaptive or kMdCnaFixed
  double r2;                      // square of the candidates' reach: r_max (adaptive) or r_cut (fixed)
  double r_cut;                   // fixed mode: the bond cutoff and r_local of every atom
};

constexpr int kMdSqTile = 64;   // q-vectors per workgroup of the amplitude launch: one wave, a lane is a q-vector
constexpr int kMdSqSlab = 64;    // atoms a workgroup of the amplitude launch holds in LDS at a time
constexpr int kMdSqMaxQ = 4096;  // TA_MD_SQ_MAX_Q

// Atoms per workgroup of the amplitude launch for a batch of n_atoms: small batches spread over the chip, large
// ones write fewer partials (the plan, blk_start, is made once by ta_md_set_sq). The chunk is also the longest
// chain of additions of one partial.
inline int md_sq_chunk(long long n_atoms) { return n_atoms <= 16384 ? 64 : 1024; }

// Arguments of the three structure-factor launches (ta_md_sq.hip) that ta_md_run puts behind an integrator launch
// that wrote the whole-step state (x, v) of a sampled step to `x` / `v`: the amplitudes rho_a(q) (and j_a(q) with
// currents) of sample n per chunk, their sum in chunk order into ring slot n % n_lags, and the correlation of that
// row with the rows of the lags 0 .. min(n, n_lags - 1). A row is [F][E][planes][Q] with planes = 2 (Re, Im of rho)
// or 8 (then Re, Im of j_x, j_y, j_z): q fastest.
struct MdSqLaunch {
  const double *x, *v;            // [N][3] the snapshot the integrator launch in front wrote
  const double *cells;            // [F][9]
  const int32_t *species;         // [N]
  const int32_t *atom_start;      // [F + 1]
  const int32_t *blk_start;       // [F + 1] first chunk of each frame (at least one each)
  const int32_t *miller;          // [Q][3]
  double *part;                   // [n_blk][E][planes][Q] per-workgroup sums
  double *ring;                   // [n_lags] rows
  double *acc_rho, *acc_l, *acc_j;  // [F][E][E][n_lags][Q] the accumulators (acc_l, acc_j: with currents)
  const unsigned *status;         // the integrator's status word and
  unsigned seq;                   // sequence number: the same predicate
  long long n;                    // index of the newest sample
  int n_q, n_lags, n_elements, n_frames, n_blk, chunk, currents;
};

constexpr int kMdFluxLanes = 16;  // lanes per centre of the pair sweep (one DPP row, as in the force gather)
constexpr int kMdFluxRow = 18;    // doubles of a sample's row: J_conv[3], J_pot[3], K[6], W[6] (xx yy zz yz xz xy)

// Atoms per workgroup of the pair sweep for a batch of n_atoms: one pass of 16 centres for small batches, four for
// large ones, which write fewer partials (the plan, blk_start, is made once by ta_md_set_flux)
inline int md_flux_chunk(long long n_atoms) { return n_atoms <= 16384 ? 16 : 64; }

// Arguments of the three heat-current / pressure-tensor launches (ta_md_flux.hip) that ta_md_run puts behind an
// integrator launch that wrote the velocities of a sampled whole-step state to `v`: the pair sweep over the list,
// records, g and eatom of the evaluation in front of that launch (DeviceBatch, the second kernel argument), the sum
// of the workgroups' partials into ring slot n % n_lags and onto `sums`, and the correlation of that row with the
// rows of the lags 0 .. min(n, n_lags - 1). A row is [F][kMdFluxRow].
struct MdFluxLaunch {
  const double *v;                // [N][3] the velocities the integrator launch in front wrote
  const double *mass;             // [N]
  const int32_t *blk_start;       // [F + 1] first workgroup of each frame (at least one each)
  double *part;                   // [n_blk][kMdFluxRow] per-workgroup sums
  double *ring;                   // [n_lags] rows
  double *sums;                   // [F][kMdFluxRow] the sum of all rows
  double *acc_heat;               // [F][n_lags][3] sum over time origins of J_a(n) J_a(n - k), J = J_conv + J_pot
  double *acc_press;              // [F][n_lags][6] likewise of Pi_ab(n) Pi_ab(n - k), Pi = K - W
  const unsigned *status;         // the integrator's status word and
  unsigned seq;                   // sequence number: the same predicate
  long long n;                    // index of the newest sample
  int n_lags, n_frames, n_blk, chunk;
};

struct DeviceBatch;

void launch_md_integrate(const MdLaunch &a, int threads, hipStream_t s);

void launch_md_mtk(const MdLaunch &a, const MdMtkLaunch &b, hipStream_t s);

void launch_md_flux(const MdFluxLaunch &a, const DeviceBatch &b, hipStream_t s);

void launch_md_correlate(const MdCorrLaunch &a, hipStream_t s);

void launch_md_rdf(const MdRdfLaunch &a, hipStream_t s);

void launch_md_adf(const MdAdfLaunch &a, hipStream_t s);

void launch_md_order(const MdOrderLaunch &a, hipStream_t s);

void launch_md_cluster(const MdClusterLaunch &a, hipStream_t s);

void launch_md_cna(const MdCnaLaunch &a, hipStream_t s);

void launch_md_sq(const MdSqLaunch &a, hipStream_t s);

// xi, eta [n][3] (device): the normals md_integrate draws for absolute step `step`, atoms 0 .. n - 1
void launch_md_noise(unsigned long long seed, long long step, long long n, double *xi, double *eta, hipStream_t s);

}  // namespace ta
