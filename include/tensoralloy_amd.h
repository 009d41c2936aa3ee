/*
 * tensoralloy_amd.h — C ABI of libtensoralloy_amd.so (MI355X / gfx950 only).
 *
 * The reference (Bismarrck/tensoralloy) has NO native plugin ABI: its hot path
 * is a frozen TensorFlow-1 graph executed by `Session.run`
 * (tensoralloy/calculator.py:335-370). This library is what sits UNDER the
 * reference's two Python surfaces instead of that graph:
 *
 *   tensoralloy/calculator.py:31-383      TensorAlloyCalculator.calculate
 *   tensoralloy/transformer/universal.py  UniversalTransformer (feed dict)
 *
 * Each entry point below names the reference interface it replaces. All
 * buffers are caller-owned, C-contiguous; the library copies host->device and
 * never keeps a host pointer after the call returns. A handle owns one device
 * and one HIP stream; a handle is not thread-safe, different handles may be
 * used from different threads. Every function returns TA_OK (0) or a negative
 * error code; `ta_last_error` gives the message.
 *
 * There is no CPU fallback: without a gfx950 device `ta_create` fails with
 * TA_ERR_HIP.
 */
#ifndef TENSORALLOY_AMD_H
#define TENSORALLOY_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ta_context *ta_handle;

enum {
  TA_OK = 0,
  TA_ERR_INVALID = -1,     /* bad argument / inconsistent model  -> ValueError  */
  TA_ERR_UNSUPPORTED = -2, /* model feature not implemented      -> ValueError  */
  TA_ERR_HIP = -3,         /* HIP runtime failure / no device    -> RuntimeError */
  TA_ERR_NOMEM = -4
};

/* `want` bits of ta_compute / ta_eval: which outputs of
 * tensoralloy/nn/basic.py:679-787 (`BasicNN.build`) are produced. */
enum {
  TA_WANT_ENERGY = 1,      /* Output/Energy/energy     atomic.py:289-302        */
  TA_WANT_FORCES = 2,      /* Output/Forces/forces     basic.py:277-290         */
  TA_WANT_VIRIAL = 4,      /* Output/Stress (virial)   basic.py:293-331         */
  TA_WANT_ATOMIC = 8,      /* Output/Energy/atomic     atomic.py:289-299        */
  TA_WANT_DESCRIPTORS = 16, /* Atomic/<El> descriptors  sf.py:184-215 (debug)   */
  TA_WANT_REUSE_DESCRIPTORS = 32 /* energy-only call on the descriptors of the last ta_compute of
                                    this batch (only the MLP weights changed: training steps) */
};

enum { TA_MODEL_SF_MLP = 1, TA_MODEL_EAM_ALLOY = 2, TA_MODEL_EAM_ADP = 3, TA_MODEL_GRAP_MLP = 4,
       TA_MODEL_EAM_FS = 5 /* eam/fs (Finnis-Sinclair, nn/eam/fs.py): inference only, see n_eam_nets */ };
enum { TA_CUTOFF_COSINE = 0, TA_CUTOFF_POLYNOMIAL = 1 }; /* nn/cutoff.py:20-85 */

/* activation ids follow `actfn_map` of atomic.py:323 for 0..3 */
enum {
  TA_ACT_RELU = 0, TA_ACT_SOFTPLUS = 1, TA_ACT_TANH = 2, TA_ACT_SQUAREPLUS = 3,
  TA_ACT_LEAKY_RELU = 4, TA_ACT_SIGMOID = 5, TA_ACT_SOFTSIGN = 6, TA_ACT_ELU = 7
};

/*
 * Model description = what `BasicNN.export` bakes into the frozen graph
 * (basic.py:1075-1092): `UniversalTransformer.as_dict()` (universal.py:323-331),
 * `SymmetryFunction.as_dict()` (sf.py:58-68), `AtomicNN.as_dict()`
 * (atomic.py:116-132) and the variables `Atomic/<El>/Conv1d{j}/{kernel,bias}`,
 * `Atomic/<El>/Output/{kernel,bias}`, `Atomic/<El>/MinMax/{xlo,xhi}`.
 * Elements are the SORTED unique symbols (utils.py:262); species indices in
 * frames index this list.
 */
typedef struct {
  int32_t kind;            /* TA_MODEL_*                                        */
  int32_t n_elements;
  double rcut;             /* UniversalTransformer.rcut                          */
  double acut;             /* UniversalTransformer.acut (== rcut if not angular) */
  int32_t angular;         /* G4 terms present                                   */
  int32_t cutoff_function; /* TA_CUTOFF_*                                        */

  /* SymmetryFunction parameter axes; grids are eta x omega (omega fastest) and
   * beta x gamma x zeta (zeta fastest), sf.py:47-51. */
  int32_t n_eta, n_omega, n_beta, n_gamma, n_zeta;
  const double *eta, *omega, *beta, *gamma, *zeta;

  /* per-element MLP (convolution1x1, convolutional.py:154-300) */
  int32_t activation;      /* TA_ACT_*                                           */
  int32_t use_resnet_dt;
  int32_t minmax_scale;    /* atomic.py:157-195                                  */
  const int32_t *n_layers; /* [n_elements] dense layers incl. the output layer   */
  const int32_t *layer_sizes; /* per element [in, h1, ..., 1], concatenated      */
  const double *weights;   /* per element, per layer: W[in][out] row-major, then
                              b[out] (zeros when the layer has no bias)          */
  const double *xlo, *xhi; /* [n_elements * in] when minmax_scale, else NULL     */

  /* EAM / ADP analytic potentials (nn/eam/potentials/zjw04.py, mishin.py), one flat block:
   *   per element (sorted): 20 constants -- Zjw04 [r_eq f_eq rho_e rho_s alpha beta A B kappa lamda
   *     Fn0 Fn1 Fn2 Fn3 F0 F1 F2 F3 eta Fe], AgSutton90 [a b] (sutton90.py:37-44) or AgrawalBe "Be/1"
   *     [A B D alpha re F0 F1 beta gamma m rc] (agrawal.py:49-55) or RWGrimes "grimes" [G n A rho C D
   *     gamma r0] (grimmes.py:33-37), zero padded -- + embed kind (0 Zjw04 piecewise, 1 Zjw04xc
   *     blended) + potential kind (0 Zjw04 family, 1 sutton90, 2 Be/1, 3 grimes);
   *   per element pair a <= b (upper triangle, row-major): phi kind (0 Zjw04, 1 Zjw04xcp own
   *     constants) + [r_eq A B alpha beta kappa lamda];
   *   ADP only, per pair: [d1 d2 d3 q1 q2 q3 h rc] (all zero = no angular term).           */
  int32_t n_eam_params;
  const double *eam_params;

  /* added under sqrt(D.D + eps) (universal.py:470-472): 1e-14 for 'high' precision models,
   * 1e-8 for 'medium' ones (precision.py:113-114). 0 selects 1e-14. Arithmetic is fp64
   * either way.                                                                      */
  double eps;

  /* GRAP descriptor (TA_MODEL_GRAP_MLP; nn/atomic/grap.py:272-704), with the MLP fields above and
   * `rcut`, `cutoff_function`: [algorithm (0 sf, 1 morse, 2 density, 3 pexp), K filters,
   * max moment (0..3), legacy_mode, symmetric, moment mask (bit m: moment m listed), then K x 3
   * filter constants: sf (eta, omega, -), morse (D, gamma, r0), density (A, beta, re),
   * pexp (rl, pl, -)].                                                                    */
  int32_t n_grap_params;
  const double *grap_params;

  /* EAM / ADP "nn" functions -- the reference's default potentials (nn/eam/alloy.py:110-112,
   * adp.py:120-124): rho(r), F(rho), phi(r), u(r), w(r) given by `convolution1x1` on the scalar
   * argument (nn/eam/eam.py:174-190; no output bias). 0 = every function is analytic. Otherwise
   * the number of function slots, 2 n_elements + n_pairs (ADP: + 2 n_pairs), in the order
   * rho[element], embed[element], phi[pair a <= b], dipole[pair], quadrupole[pair]; `n_layers`
   * [slot] (0 = analytic function, read from `eam_params`), `layer_sizes` ([1, h1, ..., 1] per
   * nn slot) and `weights` (as above, per nn slot) describe them, `activation` applies to all.
   * TA_MODEL_EAM_FS (nn/eam/fs.py): n_elements^2 + n_elements + n_pairs slots in the order
   * rho[centre][neighbour] (centre-major over the sorted elements: rho_AB = density at an A centre
   * from a B neighbour), embed[element], phi[pair a <= b]. Every slot is an nn function or
   * tabulated (n_eam_nets is never 0; `eam_params` is read for nothing but must have its usual
   * size). eam/fs models are inference only: ta_energy_gradient, ta_loss_gradient,
   * ta_constant_gradient and ta_hessian_vectors return TA_ERR_INVALID for them. */
  int32_t n_eam_nets;

  /* EAM / ADP tabulated functions: a LAMMPS setfl / adp file's rho(r), F(rho), phi(r), u(r), w(r)
   * (io/lammps.py:62-235), evaluated as natural cubic splines the way the reference's
   * `CubicInterpolator(x, y, natural_boundary=True)` does (potentials/tests/test_mishin.py:60-70;
   * `spline@...` potentials, train/training.py:258-262). Same slots as the nn functions
   * (`n_eam_nets` must be set): `eam_table_n[slot]` = number of knots (0 = not tabulated; knots at
   * k * eam_table_dx[slot]), `eam_table_coef` = per tabulated slot (n - 1) x 4 doubles, the cubic
   * c0 + c1 t + c2 t^2 + c3 t^3 of every interval with t = x - x_k. Arguments beyond the last knot
   * use the last interval's cubic. All three NULL = no tables. */
  const int32_t *eam_table_n;
  const double *eam_table_dx;
  const double *eam_table_coef;

  /* 1: powers with a non-integer exponent ((1 + gamma cos)^zeta, sf.py:162-164) use the reference's
   * custom-gradient `safe_pow` (extension/grad_ops.py:16-66, selected there by the environment
   * variable TENSORALLOY_USE_CUSTOM_POW): an infinite value and an infinite or NaN derivative factor
   * become 0. 0: plain pow, as `tf.pow`. Integer exponents are products and never singular. */
  int32_t safe_pow;

  /* Temperature-dependent models (TemperatureDependentAtomicNN, nn/atomic/finite_temperature.py:211-304)
   * on TA_MODEL_SF_MLP and TA_MODEL_GRAP_MLP. 0 = plain per-element MLP. Otherwise bit 0 = 1, bit 1 =
   * algo "Sommerfeld" (S = s(z) T instead of s(z)), bits 8-15 = the TA_ACT_* of the H nets
   * (FiniteTemperatureOptions.activation). `n_layers`, `layer_sizes` and `weights` then describe
   * 3 n_elements nets in the order H[element], U[element], S[element]: H maps the (min-max scaled,
   * `xlo` / `xhi`) descriptors to K features (linear output layer with bias); U and S map
   * z = [H, T] (K + 1 inputs, T = the frame's electron temperature in eV) to one output with
   * `activation`. Per atom F = U - T S is the energy whose forces and virial are computed; U and S
   * come from ta_get_td_results. Trainable: the parameter vector of ta_param_count /
   * ta_update_weights is H of every element, then U, then S, in that net order; ta_td_loss_gradient
   * differentiates a loss of U, F and S and the forces and stress of F; ta_energy_gradient and
   * ta_loss_gradient take their coefficients as dL/dF. ta_hessian_vectors returns TA_ERR_UNSUPPORTED. */
  int32_t finite_temperature;
} ta_model_desc;

enum { TA_TD_ON = 1, TA_TD_SOMMERFELD = 2, TA_TD_ACT_SHIFT = 8 };

/* One structure = what `UniversalTransformer.get_np_feed_dict(atoms)`
 * (universal.py:851-893) receives: an `ase.Atoms`. Atom order is the caller's
 * (ASE) order; the GSL/VAP permutation (vap.py:26-137) is applied by the
 * Python boundary, not here. */
typedef struct {
  int32_t n_atoms;
  const int32_t *species;  /* [n_atoms] index into the sorted element list       */
  const double *positions; /* [n_atoms][3] Angstrom                              */
  const double *cell;      /* [3][3] row-major lattice vectors                   */
  const int32_t *pbc;      /* [3]                                                */
} ta_frame;

typedef struct {
  int32_t n_frames;
  int64_t n_atoms;         /* total over frames                                  */
  int64_t n_pairs;         /* directed pairs within max(rcut, acut)  (= nij)     */
  int64_t n_triples;       /* sum_i n_i (n_i - 1) / 2               (= nijk)     */
  int32_t nnl_max;         /* max neighbours of one centre                       */
  int32_t descriptor_dim;  /* D per atom                                         */
  int32_t nl_on_device;    /* 1: neighbour list built by the GPU kernels, 0: host */
  int32_t reserved_;
  double nl_ms;            /* wall time of the neighbour-list part of ta_set_frames */
  double set_frames_ms;    /* wall time of the whole ta_set_frames call          */
} ta_batch_info;

/* number of kernel-timing slots filled by ta_time_compute */
#define TA_N_KERNEL_SLOTS 10
/* slot ids */
enum {
  TA_K_PAIR_GEOMETRY = 0, TA_K_G4_FORWARD = 1, TA_K_DESCRIPTOR_REDUCE = 2,
  TA_K_MLP = 3, TA_K_BACKWARD = 4, TA_K_FORCE_GATHER = 5, TA_K_FRAME_REDUCE = 6,
  TA_K_EAM = 7,
  TA_K_NEIGHBOR_UPDATE = 8, /* ta_update_positions: displacement check (+ list rebuild) */
  TA_K_GRAP = 9   /* GRAP moments + features (forward) */
};

int ta_device_count(void);

/* Version of this header's ABI (bumped whenever a struct layout or the signature of an existing entry
 * point changes; entry points that are only added leave it alone, a binding finds them by name) and
 * sizeof(ta_model_desc) as the library was compiled: a binding checks both before the first real
 * call, so that a stale or foreign build of the library is refused instead of misreading a struct.
 * (The reference has no counterpart: its "ABI" is the frozen graph's `Metadata/api`, basic.py:43.) */
#define TA_ABI_VERSION 5
int ta_abi_version(void);
int ta_model_desc_size(void);

/* replaces TensorAlloyCalculator.__init__ graph import + Session creation
 * (calculator.py:40-87): validates the model, uploads weights to `device`. */
int ta_create(const ta_model_desc *model, int device, ta_handle *out);
int ta_destroy(ta_handle h);
const char *ta_last_error(ta_handle h); /* h may be NULL: last create error */

/* replaces UniversalTransformer.get_np_feed_dict (universal.py:851-893):
 * neighbour list (ASE `neighbor_list('ijS')` semantics, universal.py:58),
 * pair buffers sorted by centre, reverse-pair index; uploads everything so the
 * batch is resident in HBM. Frames are independent units. */
int ta_set_frames(ta_handle h, int32_t n_frames, const ta_frame *frames,
                  ta_batch_info *info);

/* MD loop. The reference rebuilds its whole feed dict for every call of `calculate`
 * (calculator.py:355-366 -> get_np_feed_dict, universal.py:851-893). Here the resident batch keeps
 * its atoms, species and periodicity; only coordinates travel:
 *   ta_set_skin          Verlet skin (Angstrom, >= 0; default 0). Lists built from now on cover
 *                        max(rcut, acut) + skin. Pairs beyond the cutoff contribute nothing (cutoff
 *                        functions; explicit r < rcut test in the EAM / ADP kernels), so results are
 *                        those of the exact list up to summation order. Changing the skin drops the
 *                        resident list (the next ta_update_positions / ta_set_frames rebuilds it).
 *   ta_update_positions  positions [n_atoms_total][3] (and cells [n_frames][9], or NULL = unchanged)
 *                        for the frames of the last ta_set_frames, in the same order. The list is
 *                        reused while no atom is further than skin / 2 from where it was when the
 *                        list was built and no cell has changed; otherwise it is rebuilt exactly as
 *                        ta_set_frames does. *rebuilt (may be NULL) = 1 when it was rebuilt.
 *                        With skin = 0 every call rebuilds. Asynchronous on the reuse path.
 *   ta_list_stats        lists built / reused by this handle so far.
 *   ta_list_sizes        directed pairs, triples and the largest per-(centre, species) neighbour
 *                        count of the RESIDENT list (what ta_batch_info reported at ta_set_frames,
 *                        refreshed when ta_update_positions rebuilt the list; nij / nijk / nnl_max
 *                        of the reference's metadata, transformer/universal.py:878-887).
 *                        Any pointer may be NULL. */
int ta_set_skin(ta_handle h, double skin);
int ta_update_positions(ta_handle h, const double *positions, const double *cells, int32_t *rebuilt);
int ta_list_stats(ta_handle h, int64_t *n_builds, int64_t *n_reuses);
int ta_list_sizes(ta_handle h, int64_t *n_pairs, int64_t *n_triples, int32_t *nnl_max);

/* replaces Session.run(ops, feed_dict) (calculator.py:368): enqueues the
 * kernels on the handle's stream; asynchronous. */
int ta_compute(ta_handle h, uint32_t want);

/* copies results device->host and synchronises. Any pointer may be NULL.
 *   energy      [n_frames]            eV (temperature-dependent models: the free energy F = U - T S)
 *   forces      [n_atoms_total][3]    eV/A        (caller's atom order)
 *   virial      [n_frames][9]         eV, W_ab = sum_pairs dE/dD_a * D_b
 *   atomic      [n_atoms_total]       eV
 *   descriptors [n_atoms_total][D]    raw G (before min-max)             */
int ta_get_results(ta_handle h, double *energy, double *forces, double *virial,
                   double *atomic, double *descriptors);

/* Temperature-dependent models only (TA_ERR_INVALID otherwise).
 *   ta_set_electron_temperatures  T [n_frames] in eV for the frames of the last ta_set_frames (the
 *                        reference's `etemperature`, universal.py:295). ta_set_frames resets every T to
 *                        0; ta_update_positions, ta_step and list reuses keep them.
 *   ta_get_td_results    after ta_compute: the internal energy U and the electron entropy S per frame
 *                        [n_frames] and per atom [n_atoms_total] (caller's atom order); the frame
 *                        values are the sums of the atom values. Any pointer may be NULL. */
int ta_set_electron_temperatures(ta_handle h, int32_t n_frames, const double *T);
int ta_get_td_results(ta_handle h, double *energy, double *eentropy, double *energy_atomic,
                      double *eentropy_atomic);

/* ta_set_frames + ta_compute + ta_get_results */
int ta_eval(ta_handle h, int32_t n_frames, const ta_frame *frames, uint32_t want,
            double *energy, double *forces, double *virial, double *atomic);

/* One MD / relaxation step in ONE call: ta_update_positions + ta_compute + ta_get_results (what
 * `TensorAlloyCalculator.calculate` does per call once the structure is resident, calculator.py:335-370;
 * one library entry instead of three saves the binding's round trips between them). Arguments as
 * those three; forces / virial / atomic / rebuilt may be NULL. */
int ta_step(ta_handle h, const double *positions, const double *cells, uint32_t want, double *energy,
            double *forces, double *virial, double *atomic, int32_t *rebuilt);

/* The same results WITHOUT the copy into caller arrays: pointers into the handle's page-locked staging
 * buffer, where the device wrote them (layout as ta_get_results; NULL for what `want` did not ask for).
 * They stay valid until the next call on this handle. For bindings that wrap the memory as arrays
 * (numpy.ctypeslib): one MD step hands back 128 KB for a 4000-atom frame, and copying them out of
 * freshly DMA-written memory costs the host more than the transfer itself.
 *   ta_view_results  after ta_compute;  ta_step_view = ta_update_positions + ta_compute + ta_view_results */
int ta_view_results(ta_handle h, uint32_t want, const double **energy, const double **forces,
                    const double **virial, const double **atomic);
int ta_step_view(ta_handle h, const double *positions, const double *cells, uint32_t want, const double **energy,
                 const double **forces, const double **virial, const double **atomic, int32_t *rebuilt);

/* Device-resident MD loop: n steps of the resident batch in ONE call, with positions, velocities and
 * forces staying on the device (ta_step crosses the host twice per step). Consistent units, a = F / m:
 * with lengths in A, energies in eV and masses in amu the time unit is A sqrt(amu / eV) (ASE's units).
 * One step is velocity Verlet as ASE's VelocityVerlet:
 *     v' = v + dt/2 F(x)/m;   x <- x + dt v';   v <- v' + dt/2 F(x)/m
 * Positions stay unwrapped, cells fixed (unless ta_md_set_barostat says otherwise). Before each step a Berendsen thermostat (ASE's
 * NVTBerendsen.scale_velocities) may scale the velocities of every frame by
 *     lambda = sqrt(1 + (kT0 / kT - 1) dt / tau) clamped to [0.9, 1.1],  kT = 2 KE / (3 n_atoms of the frame)
 * (lambda = 1 when KE = 0). The centre-of-mass momentum is NOT removed, neither at ta_md_init nor by the
 * thermostat: hand in velocities without drift.
 *   ta_md_init           masses [n_atoms_total] (finite, > 0) and velocities [n_atoms_total][3] (NULL = 0)
 *                        of the resident batch, caller's atom order. Needs a resident batch. ta_set_frames
 *                        (and ta_eval) drop the MD state; ta_update_positions / ta_step keep it, so a
 *                        host-driven step may be mixed in between two runs.
 *   ta_md_set_thermostat kT0 (energy) and tau (time); kT0 <= 0 switches the thermostat off (the default).
 *   ta_md_run            n_steps steps of length dt. epot / ekin [n_steps / record_every + 1][n_frames] or
 *                        NULL: the frame energy the model reports (temperature-dependent models: F) and the
 *                        kinetic energy, for the state at entry (record 0) and after every record_every-th
 *                        step; with a thermostat, ekin is the value before that step's scaling.
 *                        n_steps = 0 evaluates the state at entry and writes that one record. On return
 *                        the results of the last evaluation are resident as after
 *                        ta_compute(want | ENERGY | FORCES) (ta_get_results / ta_view_results work), and the
 *                        list bookkeeping is as if ta_update_positions had driven every step: each step
 *                        counts as a list reuse or a list build in ta_list_stats, *n_rebuilds (may be
 *                        NULL) = lists built by this run. The skin / 2 rule of ta_update_positions is tested
 *                        on the device after every drift, and forces from a list that fails it never enter
 *                        a kick: the run stops there, rebuilds from the device's positions and goes on.
 *                        With skin = 0 every step rebuilds (correct, slow: one host round trip per step).
 *                        A run without rebuilds moves no per-atom array between host and device. A rebuild
 *                        that fails (non-finite coordinates ...) ends the run with an error that names the
 *                        step; nothing is launched after it and no batch is resident.
 *   ta_md_get_state      positions / velocities [n_atoms_total][3] of the resident state; either may be NULL.
 *
 * Langevin dynamics (canonical sampling) replaces the step by the second-order scheme of ASE's Langevin,
 * without its centre-of-mass correction. With the friction fr (1 / time), sigma_i = sqrt(2 kT0 fr / m_i) and
 *     c1 = dt/2 - dt^2 fr/8                             c2 = dt fr/2 - dt^2 fr^2/8
 *     c3_i = sqrt(dt) sigma_i/2 - dt^1.5 fr sigma_i/8   c5_i = dt^1.5 sigma_i/(2 sqrt 3)   c4_i = fr/2 c5_i
 * step k draws two standard normals xi, eta per atom and component and does
 *     rv = c3_i xi - c4_i eta;   rp = c5_i eta
 *     v += c1 F(x)/m - c2 v + rv;   x += dt v + rp;   v += c1 F(x_new)/m - c2 v + rv
 * kT0 = 0 with fr > 0 is damped dynamics. The normals are made on the device and are a pure function of
 * (seed, step, atom, component), so a run split over several ta_md_run calls, another skin or a step
 * redone after a list rebuild sees the same numbers: Philox4x32-10 with
 *     key     (seed & 0xffffffff, seed >> 32)
 *     counter (i, c, step & 0xffffffff, step >> 32)   i: index of the atom in the resident batch (caller's
 *             order over all frames), c: 0, 1, 2 = x, y, z, step: steps integrated since ta_md_init
 *             (ta_md_run advances it by n_steps when it succeeds, ta_md_init sets it to 0)
 * and from the output words w0 .. w3, all in fp64,
 *     u1 = ((w0 >> 5) 2^26 + (w1 >> 6) + 0.5) 2^-53,  u2 likewise from w2, w3
 *     xi = sqrt(-2 ln u1) cos(2 pi u2),   eta = sqrt(-2 ln u1) sin(2 pi u2)
 *   ta_md_set_langevin   kT0 (energy, finite, >= 0), friction (finite, >= 0; 0 switches Langevin off, the
 *                        default) and the seed. A property of the handle like the Berendsen setting
 *                        (ta_set_frames keeps it). Only one thermostat at a time: TA_ERR_INVALID while the
 *                        Berendsen thermostat is on, and ta_md_set_thermostat with kT0 > 0 is refused
 *                        while Langevin is on. With Langevin, ekin records the kinetic energy after the
 *                        step, and ta_md_run needs dt >= 0.
 *   ta_md_noise          xi, eta [n_atoms_total][3]: the normals of absolute step `step` (>= 0) under the
 *                        handle's seed, from the device function the integrator calls, so that a caller
 *                        can reproduce a trajectory on the host. Needs ta_md_init.
 *
 * Constant pressure: a Berendsen barostat, ASE's NPTBerendsen (isotropic) and Inhomogeneous_NPTBerendsen (per
 * axis), computed inside the integrator launch with ONE force evaluation per step. Per frame, with h the cell
 * (rows are lattice vectors), V = |det h|, W the library's virial (dE / d strain) of the evaluation at x_k, P0
 * the target pressure, beta the compressibility and taup a time, step k -> k + 1 does, in this order:
 *     1. the thermostat's velocity part (Berendsen: v <- lambda v; Langevin: nothing here; Nose-Hoover chain,
 *        below: the opening half-update)
 *     2. P_c = (sum_i m_i v_ic^2 - W_cc) / V for c = x, y, z, from the velocities as they stand after 1.
 *        isotropic: P = (P_x + P_y + P_z) / 3 and mu_x = mu_y = mu_z = 1 - (dt / taup) (beta / 3) (P0 - P)
 *        with a mask: mu_c = 1 - (dt / taup) (beta / 3) (P0 - P_c) on free axes, mu_c = 1 exactly on the others
 *        x_ic <- mu_c x_ic and h[:, c] <- mu_c h[:, c]: a diagonal strain on Cartesian components, which is
 *        ASE's row scaling for the axis-aligned orthorhombic cells its class assumes and is defined for
 *        triclinic cells too. Velocities are not scaled by mu and mu is not clamped, both as in ASE.
 *     3. the rest of the step unchanged (the half-kick and drift, or Langevin's first update and drift), with
 *        F_k, the forces evaluated at the UNSCALED x_k. This is what ASE does when forces are handed to
 *        step(); ASE evaluates again after the scaling when none are handed in. The difference is of
 *        order 1 - mu per step.
 * The barostat composes with every thermostat setting: none, Berendsen, Langevin, Nose-Hoover chain. It needs the frame's three
 * sums of m v_c^2 before any position is scaled, so one workgroup of 1024 threads owns a whole frame, as with
 * the Berendsen thermostat; the recorded kinetic energy is half the total of the three sums.
 *   ta_md_set_barostat   NULL or taup <= 0 switches the barostat off (the default). A property of the handle
 *                        like the thermostats (ta_set_frames keeps it). TA_ERR_INVALID, with the argument
 *                        named by ta_last_error and the setting left as it was: pressure or taup not finite,
 *                        compressibility not finite or < 0, isotropic == 0 with a mask of all zeros.
 *   ta_md_run            with the barostat on: TA_WANT_VIRIAL is added to `want`. TA_ERR_INVALID for a batch
 *                        with a frame that is not periodic along all three axes or has a singular cell. The
 *                        cells change on the device, so the list test knows strain as in ta_relax_run: the
 *                        launch keeps s_c, the product of the mu_c since the list was built (h = h_ref diag(s)),
 *                        and with u_i = x_i - x_ref,i o s and rc = max(rcut, acut) the list is stale when
 *                        lim = (skin - (rc + skin) |s - 1|_2) / 2 <= 0 or some |u_i|^2 >= lim^2 (s = 1: the
 *                        skin / 2 rule). Rebuilds take the cells from the device. While the barostat is on,
 *                        the triangle-once backward pass is selected as under ta_relax_set_cell: only when
 *                        every periodic width of the list's cells exceeds rc + skin. A mu_c that is not a
 *                        finite number > 0 ends the run with TA_ERR_INVALID that names the frame and the
 *                        step; the MD state is dropped and no batch is resident. A run that ends with cells
 *                        other than its list's cells builds one list for the final state and evaluates it
 *                        again (counted in *n_rebuilds and ta_list_stats; an n_steps = 0 run moves no cell
 *                        and builds nothing), exactly the rule of ta_relax_run: ta_step,
 *                        ta_update_positions(cells = NULL), a fixed-cell ta_md_run and ta_relax_run then
 *                        find the final cells. If ta_relax_set_cell is on, the moved cells become its h0,
 *                        with G = I and cell velocities 0, as for cells handed to ta_update_positions.
 *   ta_md_get_cell       cells [n_frames][9]: the resident cells.
 *   ta_md_get_records    volume [n_rec][n_frames], press [n_rec][n_frames][3] (either may be NULL) of the last
 *                        successful barostat run, at the slots of its epot / ekin: V and P_c of the recorded
 *                        state from the recorded kinetic sums (with Berendsen scaling: the sums before the
 *                        scaling). TA_ERR_INVALID when the last run had no barostat.
 *
 * Nose-Hoover chain (deterministic, time-reversible canonical sampling): names as ASE's NoseHooverChainNVT
 * (tdamp = tau, tchain = chain, tloop = loops), masses as LAMMPS fix nvt with Tdamp = tau. Every frame has
 * g = 3 n_atoms - dof_removed degrees of freedom and its own chain of M thermostats with positions eta_k,
 * velocities veta_k and masses Q_1 = g kT0 tau^2, Q_k = kT0 tau^2 (k >= 2). With K the frame's kinetic energy,
 *     G_1 = (2 K - g kT0) / Q_1,   G_k = (Q_{k-1} veta_{k-1}^2 - kT0) / Q_k   (k >= 2)
 * One half-update over Delta = dt / 2 is L loops of d = Delta / L, with s starting at 1 and G_1 evaluated with
 * the current K s^2:
 *     veta_M += (d/2) G_M
 *     for k = M-1 .. 1:  a = exp(-(d/4) veta_{k+1});  veta_k = (veta_k a + (d/2) G_k) a
 *     s *= exp(-d veta_1);   eta_k += d veta_k (all k)
 *     for k = 1 .. M-1:  a = exp(-(d/4) veta_{k+1});  veta_k = (veta_k a + (d/2) G_k) a   (G_k as they now stand)
 *     veta_M += (d/2) G_M
 * then v <- s v for the frame's atoms and K <- K s^2 (M = 1: the two loops over k are empty and G_M is G_1).
 * A step is: half-update, the velocity Verlet step above, half-update. The conserved quantity per frame is
 *     H' = K + E_pot + E_chain,   E_chain = sum_k Q_k veta_k^2 / 2 + g kT0 eta_1 + kT0 sum_{k>=2} eta_k
 * Under this thermostat record 0 is the state at entry and record r > 0 the state AFTER the closing half-update
 * of its step: ekin is K s^2 and e_chain the chain terms as they stand then, so ekin + epot + e_chain is H' at
 * every slot (under Berendsen ekin is the value before the scaling). The centre-of-mass momentum is not
 * removed: hand in velocities without drift and choose dof_removed to match. One workgroup owns a whole frame,
 * as with the Berendsen thermostat, and the chain arithmetic is one thread's, in fp64.
 * The barostat composes with it: step 1 of its order is the opening half-update, so the pressure behind mu is
 * that of the velocities after it, and the recorded press is that of the recorded state.
 *   ta_md_set_nose_hoover  NULL or kT0 <= 0 switches it off (the default; always allowed). A property of the
 *                        handle like the other thermostats: ta_set_frames keeps the setting and drops the MD
 *                        state, chain included; ta_md_init sets every chain to eta = veta = 0, and so does a
 *                        call that changes `chain` while the thermostat is on. Only one thermostat at a time:
 *                        TA_ERR_INVALID while Berendsen or Langevin is on, and both refuse to go on while this
 *                        one is. TA_ERR_INVALID, with the argument named by ta_last_error and the setting left
 *                        as it was: kT0 not finite, tau not a finite time > 0, chain outside
 *                        1 .. TA_MD_MAX_CHAIN, loops outside 1 .. 16, dof_removed < 0.
 *   ta_md_run            TA_ERR_INVALID for a batch in which some frame has g < 1.
 *   ta_md_get_chain      eta / veta [n_frames][chain] of the resident state; either may be NULL. Needs
 *                        ta_md_init and the thermostat on, as does
 *   ta_md_set_chain      the restart call: finite values [n_frames][chain], NULL = zeros. With the positions and
 *                        velocities of ta_md_get_state handed to ta_set_frames / ta_md_init, a run goes on
 *                        where another stopped.
 *   ta_md_get_chain_records  e_chain [n_rec][n_frames] of the last successful run, at the slots of its epot /
 *                        ekin. TA_ERR_INVALID when that run did not use this thermostat.
 *
 * Isothermal-isobaric ensemble: a Martyna-Tobias-Klein barostat (Martyna, Tobias, Klein, J. Chem. Phys. 101, 4177;
 * the measure-preserving integrator of Tuckerman et al., J. Phys. A 39, 5629; what LAMMPS calls fix npt and ASE
 * IsotropicMTKNPT / MTKNPT), coupled to the Nose-Hoover chain above and to a chain of its own, per frame and inside
 * the integrator launch. Unlike the Berendsen barostat it samples the ensemble: the volume fluctuates as the
 * compressibility says. Two modes: isotropic, one strain rate from the mean driving force; per axis, a diagonal
 * strain-rate tensor in which every free axis follows its own pressure and a masked axis keeps its length exactly.
 * A fully flexible cell and a run without the thermostat are not provided: the barostat needs the Nose-Hoover
 * chain on and takes kT0 from it. Per frame: n atoms, g = 3 n - dof_removed, kT0 and tau the chain's, P0 the target
 * pressure, tau_p the barostat's time, h the cell (rows are lattice vectors), V = |det h|, W_vir the virial (dE / d
 * strain) of the last evaluation, S_c = sum_i m_i v_ic^2, K = (S_x + S_y + S_z) / 2, free_c in {0, 1} the free axes
 * (isotropic: all three), d_b = 1 (isotropic) or sum_c free_c. State: the strain rates omega_c and the barostat's
 * chain (xi_k, vxi_k), k = 1 .. M_p. Masses:
 *     W_c = (g + 3) kT0 tau_p^2 / 3,   Q'_1 = d_b kT0 tau_p^2,   Q'_k = kT0 tau_p^2 (k >= 2)
 * Driving force, and what follows from omega:
 *     G_c = free_c [S_c - W_vir,cc - P0 V + 2 K / g] / W_c        isotropic: the three G_c are replaced by their mean
 *     alpha_c = omega_c + (omega_x + omega_y + omega_z) / g,       K_b = sum_c W_c omega_c^2 / 2
 * half(chain, K, dof, tau) is the half-update over dt / 2 spelled out above with (g, tau) -> (dof, tau); it returns
 * the factor s. One step from (x, v, h, omega, chains) with F and W_vir of x, h:
 *     1. s = half(particle chain, K, g, tau);  v <- s v
 *     2. s_b = half(barostat chain, K_b, d_b, tau_p);  omega <- s_b omega
 *     3. omega_c += (dt/2) G_c          K and S_c as they stand after 1, V and W_vir of the current state
 *     4. v_c <- v_c exp(-(dt/2) alpha_c);  then v += (dt/2) F/m
 *     5. x_c <- exp(omega_c dt) x_c + dt exp(omega_c dt/2) v_c;  h[:, c] <- exp(omega_c dt) h[:, c]
 *     6. evaluate F and W_vir at the new x, h
 *     7. v += (dt/2) F/m;  then v_c <- v_c exp(-(dt/2) alpha_c)        alpha from the omega of 3
 *     8. omega_c += (dt/2) G_c          from the new S_c, K, V, W_vir
 *     9. s_b = half(barostat chain, K_b, d_b, tau_p);  omega <- s_b omega;  then s = half(particle chain, K, g, tau);
 *        v <- s v
 * The conserved quantity per frame is
 *     H' = K + E_pot + E_chain + E_baro
 *     E_baro = P0 V + K_b + sum_k Q'_k vxi_k^2 / 2 + d_b kT0 xi_1 + kT0 sum_{k>=2} xi_k
 * Its excursion falls by 4 per halving of dt, and a run reversed (v, omega, veta, vxi -> -) returns to its start.
 * Record 0 is the state at entry and record r > 0 the state after step 9 of its step, so ekin + epot + e_chain +
 * e_baro is H' at every slot. One workgroup owns a whole frame; the chain and barostat arithmetic is one thread's,
 * in fp64 with a fixed order.
 *   ta_md_set_mtk_barostat  NULL or tau_p <= 0 switches it off (the default; always allowed). A property of the
 *                        handle like the other settings (ta_set_frames keeps it). TA_ERR_INVALID, with the argument
 *                        named by ta_last_error and the setting left as it was: pressure or tau_p not finite, chain
 *                        outside 1 .. TA_MD_MAX_CHAIN, loops outside 1 .. 16, isotropic == 0 with a mask of all
 *                        zeros, the Berendsen barostat on (and ta_md_set_barostat refuses to go on while this one
 *                        is: only one barostat at a time). A call that changes `chain` while the barostat is on
 *                        puts the barostat's chain at rest, as ta_md_set_nose_hoover does with its own.
 *   ta_md_run            with this barostat on: TA_ERR_INVALID while the Nose-Hoover chain is off or the Berendsen
 *                        or the Langevin thermostat is on, for a batch with a frame that is not periodic along all
 *                        three axes or has a singular cell, and with the samplers that refuse the Berendsen barostat
 *                        (ta_md_set_sampling, _rdf, _sq, _flux), for the same reasons. Everything ta_md_run does for
 *                        the Berendsen barostat holds unchanged: TA_WANT_VIRIAL is added to `want`; the launch
 *                        keeps s_c, the product of the exp(omega_c dt) since the list was built, and the list test
 *                        is the one stated there; rebuilds take the cells from the device; the triangle-once
 *                        backward pass is selected by the wider rule; an exp(omega_c dt) that is not a finite
 *                        number > 0 ends the run with TA_ERR_INVALID; a run that moved the cells ends with one list
 *                        for the final cells, which ta_relax_set_cell takes over as its h0. A launch enqueued behind
 *                        a stale list leaves omega and both chains alone.
 *   ta_md_get_records    volume and press of the recorded states (after step 9), as under the Berendsen barostat.
 *   ta_md_get_mtk_state  omega [n_frames][3], xi / vxi [n_frames][chain] of the resident state; any may be NULL.
 *                        Needs ta_md_init and this barostat on, as does
 *   ta_md_set_mtk_state  the restart call: finite values, NULL = zeros. ta_md_init zeroes all three. With
 *                        ta_md_get_state, ta_md_get_chain and ta_md_get_cell a run goes on exactly where another
 *                        stopped.
 *   ta_md_get_mtk_records  e_baro [n_rec][n_frames] of the last successful run, at the slots of its epot / ekin.
 *                        TA_ERR_INVALID when that run did not use this barostat.
 *
 * Time correlations inside the loop (opt-in; with sampling never switched on nothing changes). Let t be the
 * absolute step (steps integrated since ta_md_init, the counter of the Langevin noise). With n_lags = L and
 * sample_every = s the whole-step state (x(t), v(t)) of every t with t % s == 0 is sampled, once: the positions
 * as the device holds them (unwrapped), and the velocities whose kinetic energy the record slot of that step
 * holds (velocity Verlet / Berendsen: after the second half-kick, before the next Berendsen factor; Langevin:
 * after the second update of step t - 1; Nose-Hoover chain: after the closing half-update). Samples are numbered
 * n = 0, 1, ... from the first one taken after sampling was switched on; sample n lives in slot n % L of a ring
 * [L][n_atoms_total][3] in device memory, written by the integrator launch. Behind every launch that sampled a
 * correlation kernel adds, for every lag k = 0 .. min(n, L - 1), frame f and element e of the model,
 *     A_v[f][e][k] += sum over atoms i of f with species e of  v_i(n) . v_i(n - k)
 *     A_x[f][e][k] += sum over the same atoms of               |x_i(n) - x_i(n - k)|^2
 * in a fixed order (no floating-point atomics), so the sums do not depend on how a run is cut into calls, on
 * the skin or on list rebuilds beyond what the trajectories themselves differ by. The number of time origins at
 * lag k is max(0, n_samples - k); normalising by it and by the atoms of (f, e) gives the velocity
 * autocorrelation and the mean-square displacement. No centre-of-mass correction is made.
 *   ta_md_set_sampling   NULL or n_lags == 0 switches sampling off (the default; always allowed) and frees the
 *                        ring. Switching on needs a resident batch and ta_md_init; it allocates the rings and
 *                        the accumulators [n_frames][n_elements][n_lags] x 2, zeroes the accumulators and
 *                        forgets earlier samples (so does every further call). A property of the handle like
 *                        the thermostats: ta_set_frames keeps the setting and drops the data with the MD state;
 *                        ta_md_init starts an empty ring and zero accumulators. TA_ERR_INVALID, with the
 *                        argument named by ta_last_error and the setting left as it was: n_lags outside
 *                        0 .. 4096, sample_every < 1. TA_ERR_NOMEM when the device allocation fails; sampling
 *                        is then off.
 *   ta_md_run            TA_ERR_INVALID while sampling and the barostat are both on (displacements in a moving
 *                        cell are not defined here). A run that fails leaves the correlation data invalid: both
 *                        getters are TA_ERR_INVALID until ta_md_set_sampling or ta_md_init is called again.
 *   ta_md_get_correlations  vacf_sum / msd_sum [n_frames][n_elements][n_lags]: the raw sums A_v / A_x;
 *                        info [4] = {n_samples, n_lags, sample_every, absolute step of the newest sample or -1}.
 *                        Any pointer may be NULL.
 *   ta_md_get_samples    the snapshots first_lag .. first_lag + n - 1 back from the newest one (0 = the newest):
 *                        positions / velocities [n][n_atoms_total][3] and their absolute steps [n]; any pointer
 *                        may be NULL. TA_ERR_INVALID when first_lag < 0, n < 0 or first_lag + n exceeds the
 *                        min(n_samples, n_lags) snapshots held.
 *
 * Partial pair distributions inside the loop (opt-in; with it never switched on nothing changes). With n_bins = B,
 * r_max and sample_every = s the whole-step state x(t) of every absolute step t with t % s == 0, from the first
 * such step at or behind the call that switched the feature on, is sampled, once, however the run is cut into
 * calls and whatever steps are redone after a list rebuild. A launch in front of the integrator launch of that
 * step counts every directed pair (i, j, S) of the resident neighbour list, with the positions (unwrapped) and
 * the cells as the device holds them:
 *     C[f][a][b][k] += 1    a = species of the centre i, b = species of the neighbour j, f their frame,
 *                           k = floor(r / dr),  dr = r_max / B,  r = |x_j - x_i + S . h| in fp64
 * Pairs with k >= B are dropped; that compare alone decides (a pair exactly at r_max is dropped, there is no
 * second test of r against r_max). A self-image (i == j, S != 0) counts like any other pair. The counts are
 * unsigned 64-bit integers, summed with integer atomics: they are exact and do not depend on how a run is cut.
 * Since every unordered pair is listed from both ends, C[f][a][b][k] == C[f][b][a][k].
 *     g_ab(r_k) = C[a][b][k] V / (n_samples N_a N_b (4 pi / 3) ((k + 1)^3 - k^3) dr^3)
 * for a frame periodic along all three axes, with N_a N_b (not N_a (N_b - delta_ab)) in the denominator.
 * Sampling under the barostat is out of scope: normalising integer counts needs ONE volume.
 *   ta_md_set_rdf        NULL or n_bins == 0 switches it off (the default; always allowed) and frees the
 *                        accumulators. Switching on needs a resident batch and ta_md_init; it allocates the
 *                        accumulators [n_frames][n_elements][n_elements][n_bins], zeroes them and the sample
 *                        counter (so does every further call). A property of the handle with the life cycle of
 *                        ta_md_set_sampling, and independent of it: ta_set_frames keeps the setting and drops the
 *                        data with the MD state (the device memory of the old batch's counts is freed by the
 *                        next ta_md_init, ta_md_set_rdf or ta_destroy); ta_md_init starts from zero counts.
 *                        TA_ERR_INVALID, with the
 *                        argument named by ta_last_error and the setting left as it was: n_bins outside
 *                        0 .. TA_MD_MAX_BINS; sample_every < 1; r_max not finite, <= 0, or greater than
 *                        max(rcut, acut) of the model (the neighbour list is not complete beyond that).
 *                        TA_ERR_NOMEM when the device allocation fails; the feature is then off.
 *   ta_md_run            TA_ERR_INVALID while this feature and the barostat are both on. A run that fails leaves
 *                        the counts invalid: ta_md_get_rdf is TA_ERR_INVALID until ta_md_set_rdf or ta_md_init
 *                        is called again.
 *   ta_md_get_rdf        counts [n_frames][n_elements][n_elements][n_bins]; info [4] = {n_samples, n_bins,
 *                        sample_every, absolute step of the newest sample or -1}; *r_max. Any pointer may be
 *                        NULL.
 *
 * Bond-angle distributions inside the loop (opt-in; with it never switched on nothing changes): the distribution of
 * the angles j-i-k between the bonds of a centre i to its neighbours, the three-body companion of g_ab(r).
 * Parameters: n_bins = B, sample_every = s and a symmetric bond cutoff rb[a][b] per pair of elements (r_bond: the
 * same value for all pairs). The whole-step state of every absolute step t with t % s == 0, from the first such
 * step at or behind the call that switched the feature on, is sampled, once, however the run is cut into calls and
 * whatever steps are redone after a list rebuild (the schedule of ta_md_set_rdf, kept separately). A launch in
 * front of the integrator launch of that step takes, for every centre i of species a, as neighbours the entries
 * (j, S) of the resident neighbour list with
 *     d = x_j - x_i + S . h  (fp64, positions unwrapped and cells as the device holds them),
 *     d . d < rb[a][b]^2,    b = species of j
 * A self-image, or two images of one atom, are neighbours like any other. Every unordered pair {(j, S), (k, S')}
 * of distinct neighbours of i counts once:
 *     u = d_ij, w = d_ik
 *     theta = atan2(|u x w|, u . w)   in [0, pi]
 *     kbin = min(B - 1, floor(theta / (pi / B)))
 *     p = b E - b (b - 1) / 2 + (c - b)  for the species b <= c of the two neighbours,  P = E (E + 1) / 2
 *     C[f][a][p][kbin] += 1           (unsigned 64-bit, integer atomics: exact, whatever the order)
 * atan2 of cross and dot product needs no normalisation and is well conditioned at 0 and pi. A NaN counts
 * nowhere; theta = pi belongs to the last bin. No volume enters: unlike the pair distributions this feature runs
 * under the barostat, with the cells of the sampled state, and under every thermostat, independently of
 * ta_md_set_sampling and ta_md_set_rdf.
 *   ta_md_set_adf        NULL or n_bins == 0 switches it off (the default; always allowed) and frees the
 *                        accumulators. r_bond_pairs [n_elements][n_elements], or NULL: r_bond for every pair
 *                        (with r_bond_pairs given r_bond is not read). Switching on needs a resident batch and
 *                        ta_md_init; it allocates the accumulators [n_frames][n_elements][P][n_bins], zeroes them
 *                        and the sample counter (so does every further call). The life cycle is that of
 *                        ta_md_set_rdf: ta_set_frames keeps the setting and drops the data with the MD state;
 *                        ta_md_init starts from zero counts. TA_ERR_INVALID, with the argument named by
 *                        ta_last_error and the setting left as it was: n_bins outside 0 .. TA_MD_MAX_BINS;
 *                        sample_every < 1; a cutoff not finite, <= 0, or greater than max(rcut, acut) of the model
 *                        (the neighbour list is not complete beyond that); r_bond_pairs not symmetric.
 *                        TA_ERR_NOMEM when the device allocation fails; the feature is then off.
 *   ta_md_run            A run that fails leaves the counts invalid: ta_md_get_adf is TA_ERR_INVALID until
 *                        ta_md_set_adf or ta_md_init is called again.
 *   ta_md_get_adf        counts [n_frames][n_elements][P][n_bins]; info [4] as ta_md_get_rdf; r_bond_pairs
 *                        [n_elements][n_elements], the cutoffs in use. Any pointer may be NULL.
 *
 * Bond-orientational order inside the loop (opt-in; with it never switched on nothing changes): the Steinhardt order
 * parameters q_l of every atom, their neighbour average (Lechner and Dellago, J. Chem. Phys. 129, 114707) and the
 * count of "solid bonds" (ten Wolde, Ruiz-Montero and Frenkel), which tell crystalline atoms from disordered ones
 * and fcc from bcc from hcp. Parameters: up to TA_MD_ORDER_MAX_DEGREES degrees l, each 1 .. TA_MD_ORDER_MAX_L, in
 * any order and without duplicates; n_bins = B, sample_every = s; a symmetric bond cutoff rb[a][b] per pair of
 * elements (r_bond: the same value for all pairs); solid_degree, one of the degrees, and solid_threshold = c. The
 * schedule is that of ta_md_set_adf, kept separately. Two launches in front of the integrator launch of a sampled
 * step take, for every centre i of species a, the neighbours of ta_md_set_adf: the entries (j, S) of the resident
 * list with d = x_j - x_i + S . h (fp64), d . d < rb[a][b]^2; a self-image, or several images of one atom, are
 * separate neighbours. With N_b(i) their number, for every degree l and m = 0 .. l
 *     q_lm(i)    = (1 / N_b) sum_neigh Y_lm(d / |d|)       Y_lm as scipy.special.sph_harm (Condon-Shortley phase);
 *                                                          Y_{l,-m} = (-1)^m conj(Y_lm) is never stored
 *     q_l(i)     = sqrt(4 pi / (2 l + 1) (|q_l0|^2 + 2 sum_{m > 0} |q_lm|^2))
 *     qbar_lm(i) = (q_lm(i) + sum_neigh q_lm(j)) / (N_b(i) + 1),   qbar_l from qbar_lm as q_l from q_lm
 *     s_ij       = Re sum_{m = -l .. l} q_lm(i) conj(q_lm(j)) / (|q_l(i)| |q_l(j)|)   for l = solid_degree, with
 *                  |q_l| the 2-norm over all m; a centre or a neighbour with |q_l| = 0 forms no solid bond
 *     n_conn(i)  = number of neighbours with s_ij > c
 * An atom without neighbours has q_lm = 0 and q_l = qbar_l = 0, never NaN. Y_lm is evaluated without trigonometry
 * from z / r and (x + i y) / r, so the poles are no special case. All sums are fp64 in an order that the resident
 * list fixes: a run cut into calls reproduces the uncut run bit for bit. Another skin or another pattern of list
 * rebuilds orders the list differently; per-atom values then agree to rounding (1e-13), not bitwise.
 * Accumulated over the samples as unsigned 64-bit integer counts, per frame f and species a of the centre:
 *     hist_q    [f][a][degree][k],  k = min(B - 1, floor(q_l B))      (q_l <= 1 by the addition theorem)
 *     hist_qbar [f][a][degree][k]   likewise for qbar_l
 *     hist_conn [f][a][min(n_conn, TA_MD_ORDER_MAX_CONN)]
 * A NaN counts nowhere. Kept per atom for the NEWEST sample only and overwritten at every sample: q, qbar
 * [n_atoms][n_degrees], N_b and n_conn [n_atoms], q_lm [n_atoms][sum (l + 1)][2] (degree by degree in the order
 * given, m = 0 .. l, real then imaginary part): the classification of the state at info[3]. No volume enters: the
 * feature runs under the barostat, with the cells of the sampled state, under every thermostat, and
 * independently of ta_md_set_sampling, ta_md_set_rdf and ta_md_set_adf. ta_md_run with n_steps = 0 samples the
 * resident state once: ta_md_init + ta_md_set_order + ta_md_run(0) analyses a static structure.
 *   ta_md_set_order      NULL or n_bins == 0 switches it off (the default; always allowed) and frees the buffers.
 *                        r_bond_pairs as for ta_md_set_adf. Switching on needs a resident batch and ta_md_init; it
 *                        allocates and zeroes the counts and the sample counter (so does every further call). The
 *                        life cycle is that of ta_md_set_adf: ta_set_frames keeps the setting and drops the data
 *                        with the MD state; ta_md_init starts from zero counts. TA_ERR_INVALID, with the argument
 *                        named by ta_last_error and the setting left as it was: n_bins outside
 *                        0 .. TA_MD_MAX_BINS; sample_every < 1; n_degrees outside 1 .. TA_MD_ORDER_MAX_DEGREES; a
 *                        degree outside 1 .. TA_MD_ORDER_MAX_L or given twice; solid_degree not among the
 *                        degrees; solid_threshold not finite or not inside (-1, 1); a cutoff not finite, <= 0, or
 *                        greater than max(rcut, acut) of the model; r_bond_pairs not symmetric. TA_ERR_NOMEM when
 *                        the device allocation fails; the feature is then off.
 *   ta_md_run            A run that fails leaves the counts invalid: both getters are TA_ERR_INVALID until
 *                        ta_md_set_order or ta_md_init is called again.
 *   ta_md_get_order      hist_q, hist_qbar [n_frames][n_elements][n_degrees][n_bins]; hist_conn
 *                        [n_frames][n_elements][TA_MD_ORDER_MAX_CONN + 1]; info [4] as ta_md_get_adf; r_bond_pairs
 *                        [n_elements][n_elements], the cutoffs in use. Any pointer may be NULL.
 *   ta_md_get_order_atoms  the per-atom arrays of the newest sample (above); TA_ERR_INVALID while no sample has
 *                        been taken. Any pointer may be NULL.
 *
 * Clusters of solid or selected atoms inside the loop (opt-in; with it never switched on nothing changes): the
 * connected components of the selected atoms, for the size of the largest crystalline nucleus as a function of
 * time (n_min > 0) and for the clusters of chosen elements in a solid solution (n_min = 0). Parameters: a
 * species_mask, n_min, n_bins = B, n_series = T, sample_every = s and a symmetric link cutoff rl[a][b] per pair of
 * elements (r_link: the same value for all pairs; NaN: max(rcut, acut) of the model), at most max(rcut, acut). The
 * schedule is that of ta_md_set_adf, kept separately. At a sampled whole-step state
 *     atom i of species a is SELECTED when bit a of species_mask is set and (n_min == 0 or n_conn(i) >= n_min),
 *         n_conn being that of ta_md_set_order for the same state;
 *     two selected atoms i != j are LINKED when the resident list holds an entry (j, S) of centre i with
 *         d = x_j - x_i + S . h (fp64, unwrapped positions and cells as the device holds them), d . d < rl[a][b]^2;
 *         an entry that is an image of i itself links nothing, several images of j link i and j once;
 *     a CLUSTER is a connected component of the selected atoms under links. Its size is its number of atoms, not
 *         images: a cluster that percolates through the periodic boundary is one cluster. Its LABEL is the smallest
 *         index of its members, in the caller's atom order over the whole batch.
 * Every output is an integer and a function of the state alone: exact, whatever the order in which threads arrive,
 * the skin, the pattern of list rebuilds or the way a run is cut into calls. Four launches in front of the integrator
 * launch of a sampled step, behind the order launches of that step (select; a lock-free union by index with integer
 * atomic minima; flatten; summarise): no host wait, no grid barrier, no floating-point atomics. Kept per atom for
 * the NEWEST sample only: label [n_atoms] (-1 when not selected) and size [n_atoms] (0 when not selected).
 * Accumulated over the samples as unsigned 64-bit integer counts:
 *     hist[f][k] += number of clusters of frame f with k = min(size, B) - 1      (the last bin collects sizes >= B)
 * A time series on the device: sample n writes the row series[n % T][f][4] = {selected atoms, clusters, size of the
 * largest cluster, label of the largest (among equals the smallest label); {0, 0, 0, -1} when nothing is selected}
 * and its absolute step into steps[n % T]; the newest T rows are kept. No volume enters: the feature runs under the
 * barostat, with the cells of the sampled state, under every thermostat, and independently of the other observables
 * but for this: n_min > 0 reads the n_conn of ta_md_set_order for the same state. ta_md_run with n_steps = 0 samples
 * the resident state once.
 *   ta_md_set_clusters   NULL or n_bins == 0 switches it off (the default; always allowed) and frees the buffers.
 *                        r_link_pairs: NULL, or [n_elements][n_elements] symmetric cutoffs that replace r_link.
 *                        Switching on needs a resident batch and ta_md_init; it allocates and zeroes the histogram,
 *                        the series and the sample counter (so does every further call). The life cycle is that of
 *                        ta_md_set_adf: ta_set_frames keeps the setting and drops the data with the MD state;
 *                        ta_md_init starts from zero. TA_ERR_INVALID, with the argument named by ta_last_error and
 *                        the setting left as it was: n_bins outside 0 .. TA_MD_MAX_BINS; n_series outside
 *                        1 .. TA_MD_CLUSTER_MAX_SERIES; sample_every < 1; n_min outside 0 .. TA_MD_ORDER_MAX_CONN;
 *                        species_mask zero or with a bit at or above n_elements; a cutoff not finite (but for
 *                        r_link = NaN), <= 0, or greater than max(rcut, acut) of the model; r_link_pairs not
 *                        symmetric. TA_ERR_NOMEM when the device allocation fails; the feature is then off.
 *   ta_md_run            With n_min > 0, TA_ERR_INVALID (ta_last_error names the reason) unless ta_md_set_order is
 *                        on, this sample_every is a multiple of the order feature's and this schedule's first
 *                        sample is not in front of the order schedule's. TA_ERR_HIP when a loop of the link launch
 *                        overran its cap (never, by construction). A run that fails leaves the data invalid: both
 *                        getters are TA_ERR_INVALID until ta_md_set_clusters or ta_md_init is called again.
 *   ta_md_get_clusters   hist [n_frames][n_bins]; series [rows held][n_frames][4] and steps [rows held], oldest
 *                        first; info [6] = {n_samples, n_bins, sample_every, absolute step of the newest sample or
 *                        -1, rows held = min(n_samples, T), T}; r_link_pairs [n_elements][n_elements], the cutoffs
 *                        in use. Any pointer may be NULL.
 *   ta_md_get_cluster_atoms  label and size of the newest sample (above); TA_ERR_INVALID while no sample has been
 *                        taken. Any pointer may be NULL.
 *
 * Common neighbour analysis inside the loop (opt-in; with it never switched on nothing changes): the lattice type
 * of every atom, OVITO's numbering 0 OTHER, 1 FCC, 2 HCP, 3 BCC, 4 ICO, by the conventional analysis of
 * Honeycutt-Andersen / Faken-Jonsson at a fixed cutoff (LAMMPS `compute cna/atom`) or adaptively (Stukowski 2012,
 * OVITO's default). Parameters: mode, r_cut, r_max, n_series = T, sample_every = s. The schedule is that of
 * ta_md_set_adf, kept separately. At a sampled whole-step state
 *     the CANDIDATES of centre i are the entries (j, S) of the resident list with d = x_j - x_i + S . h (fp64,
 *         unwrapped positions and cells as the device holds them), d . d < r^2, r = r_max (adaptive) or r_cut (fixed).
 *         Species do not enter; self-images and several images of one atom are neighbours like any other. They are
 *         ordered by the key (d . d, j, S0, S1, S2), so the selection does not depend on the order of the list;
 *     for N neighbour vectors and a cutoff rc, neighbours j, k are BONDED when |d_j - d_k| < rc; the SIGNATURE of
 *         neighbour j is (n_cn, n_b, l_cb): the neighbours bonded to j, the bonds among those, the most bonds in
 *         one connected set of those bonds. FCC: N = 12, twelve (4,2,1). HCP: N = 12, six (4,2,1) and six (4,2,2).
 *         ICO: N = 12, twelve (5,5,5). BCC: N = 14, eight (6,6,6) and six (4,4,4). Anything else is OTHER;
 *     ADAPTIVE: fewer than 12 candidates: OTHER, r_local = 0. Else the 12 nearest with rc = (1 + sqrt 2) / 2 mean |d|
 *         test FCC, HCP, ICO; if none matches and there are at least 14 candidates, the 14 nearest with
 *         rc = (1 + sqrt 2) / 2 ((2 / sqrt 3) sum of the 8 nearest |d| + sum of the next 6) / 14 test BCC.
 *         r_local is the rc of the last attempt made;
 *     FIXED: all N candidates, rc = r_cut = r_local; N = 12 tests FCC, HCP, ICO, N = 14 tests BCC, any other N is OTHER.
 * Every output but r_local is an integer and a function of the state alone: exact, whatever the skin, the pattern of
 * list rebuilds or the way a run is cut into calls; r_local is a sum in the order of the sorted selection and
 * reproduces itself bit for bit. A launch that zeroes the sample's row and the analysis go in front of the integrator
 * launch of a sampled step, behind the order and cluster launches of that step: no host wait, no grid barrier, no
 * floating-point atomics. Kept per atom for the NEWEST sample only: structure [n_atoms] and r_local [n_atoms].
 * Accumulated over the samples as unsigned 64-bit integer counts:
 *     counts[f][a][type] += atoms of species a of frame f with that type
 * A time series on the device: sample n writes the row series[n % T][f][5], the atoms of every type summed over the
 * species, and its absolute step into steps[n % T]; the newest T rows are kept. No volume enters: the feature runs
 * under the barostat, with the cells of the sampled state, under every thermostat, and independently of the other
 * observables. ta_md_run with n_steps = 0 analyses the resident state once.
 *   ta_md_set_cna        NULL or n_series == 0 switches it off (the default; always allowed) and frees the buffers.
 *                        Switching on needs a resident batch and ta_md_init; it allocates and zeroes the counts, the
 *                        series and the sample counter (so does every further call). The life cycle is that of
 *                        ta_md_set_adf: ta_set_frames keeps the setting and drops the data with the MD state;
 *                        ta_md_init starts from zero. TA_ERR_INVALID, with the argument named by ta_last_error and
 *                        the setting left as it was: mode neither TA_MD_CNA_ADAPTIVE nor TA_MD_CNA_FIXED; n_series
 *                        outside 0 .. TA_MD_CLUSTER_MAX_SERIES; sample_every < 1; r_cut (fixed mode) or r_max
 *                        (adaptive mode) not finite (but for r_max = NaN: the model's cutoff), <= 0, or greater than
 *                        max(rcut, acut) of the model. TA_ERR_NOMEM when the device allocation fails; the feature is
 *                        then off.
 *   ta_md_run            A run that fails leaves the data invalid: both getters are TA_ERR_INVALID until
 *                        ta_md_set_cna or ta_md_init is called again.
 *   ta_md_get_cna        counts [n_frames][n_elements][5]; series [rows held][n_frames][5] and steps [rows held],
 *                        oldest first; info [6] = {n_samples, mode, sample_every, absolute step of the newest sample
 *                        or -1, rows held = min(n_samples, T), T}. Any pointer may be NULL.
 *   ta_md_get_cna_atoms  structure and r_local of the newest sample (above); TA_ERR_INVALID while no sample has been
 *                        taken. Any pointer may be NULL.
 *
 * Structure factors inside the loop (opt-in; with it never switched on nothing changes): the static structure
 * factor S(q), the intermediate scattering function F(q, t) and the longitudinal and transverse current
 * correlations, by a direct sum over the atoms, so that nothing stops at the model's cutoff. The caller gives
 * n_q = Q integer triples n[Q][3] (Miller indices, |n_c| <= TA_MD_SQ_MAX_INDEX), shared by all frames. With h the
 * cell of frame f (rows are lattice vectors) and s_i = x_i h^-1 the wave vector is q = 2 pi h^-1 n, so that
 * q . x_i = 2 pi n . s_i: commensurate with every frame's own cell, and unchanged when an atom moves by a lattice
 * vector (the positions are unwrapped). Everything is fp64. At the whole-step state (x(t), v(t)) of every absolute
 * step t with t % sample_every == 0, from the first such step at or behind the call that switched the feature on
 * (the state and the velocities are those ta_md_set_sampling samples), per frame f, element a and vector q
 *     rho_a(q) = sum_{i in a} exp(+i 2 pi n . s_i)
 *     j_a(q)   = sum_{i in a} v_i exp(+i 2 pi n . s_i)        (three Cartesian components; with currents = 1)
 * with the phase reduced exactly (n . s minus the nearest integer) before sine and cosine are taken. Sample number
 * m lives in slot m % n_lags of a ring of amplitude rows on the device and is correlated with the rows of the lags
 * k = 0 .. min(m, n_lags - 1), over every time origin, per ordered pair of elements (a, b):
 *     A_rho[f][a][b][k][q] += Re(rho_a(q; m) conj rho_b(q; m - k))
 *     A_L  [f][a][b][k][q] += Re((qhat . j_a(q; m)) conj (qhat . j_b(q; m - k)))     qhat = q / |q|, 0 for n = 0
 *     A_J  [f][a][b][k][q] += Re(j_a(q; m) . conj j_b(q; m - k))                     (trace of the current tensor)
 * The number of time origins at lag k is max(0, n_samples - k). F_ab(q, t_k) = A_rho[k] / (origins sqrt(N_a N_b))
 * are the Ashcroft-Langreth partials, S_ab(q) = F_ab(q, 0); (A_J - A_L) / 2 is the transverse part. n_lags = 1 is
 * the static case. All sums have a fixed order (the atoms of a chunk in index order, then the chunks of a frame
 * in index order; no floating-point atomics): a run cut into calls reproduces the uncut run bit for bit. Device
 * memory: the ring takes n_lags F E Q (1 or 4) 16 bytes, every accumulator F E^2 n_lags Q 8 bytes.
 * Independent of every other observable and of the thermostat; ta_md_run with n_steps = 0 samples the resident
 * state once: ta_md_init + ta_md_set_sq + ta_md_run(0) analyses a static structure.
 *   ta_md_set_sq         NULL or n_q == 0 switches it off (the default; always allowed) and frees the buffers.
 *                        Switching on needs a resident batch and ta_md_init; it allocates and zeroes the
 *                        accumulators and forgets earlier samples (so does every further call). The life cycle is
 *                        that of ta_md_set_sampling: ta_set_frames keeps the setting and drops the data with the MD
 *                        state; ta_md_init starts an empty ring and zero accumulators. TA_ERR_INVALID, with the
 *                        argument named by ta_last_error and the setting left as it was: n_q outside
 *                        0 .. TA_MD_SQ_MAX_Q; n_lags outside 1 .. TA_MD_MAX_LAGS; sample_every < 1; currents not
 *                        0 or 1; miller NULL or an index beyond TA_MD_SQ_MAX_INDEX; a frame that is not periodic
 *                        along all three axes or whose cell is singular. TA_ERR_NOMEM when the device allocation
 *                        fails; the feature is then off.
 *   ta_md_run            TA_ERR_INVALID while this feature and the barostat are both on (cell and positions of the
 *                        snapshot would belong to different states). A run that fails leaves the data invalid:
 *                        both getters are TA_ERR_INVALID until ta_md_set_sq or ta_md_init is called again.
 *   ta_md_get_sq         a_rho, a_l, a_j [n_frames][n_elements][n_elements][n_lags][n_q]: the raw sums; info [8] =
 *                        {n_samples, n_q, n_lags, sample_every, absolute step of the newest sample or -1, currents,
 *                        atoms per workgroup of the amplitude launch (the longest chain of additions of one
 *                        partial sum; a frame's partials are then added one after another), 0}; miller [n_q][3].
 *                        Any pointer may be NULL; a_l or a_j without currents is TA_ERR_INVALID.
 *   ta_md_get_sq_amplitudes  the amplitude rows first_lag .. first_lag + n - 1 back from the newest one (0 = the
 *                        newest): rho [n][n_frames][n_elements][n_q][2] (real, imaginary), cur
 *                        [n][n_frames][n_elements][n_q][3][2] and their absolute steps [n]; any pointer may be
 *                        NULL. TA_ERR_INVALID when first_lag < 0, n < 0, first_lag + n exceeds the
 *                        min(n_samples, n_lags) rows held, or cur is asked for without currents.
 *
 * Heat current and pressure tensor inside the loop (opt-in; with it never switched on nothing changes): the two
 * Green-Kubo observables, which need the model's per-atom energies e_i and per-pair gradients and so cannot be
 * made from a dumped trajectory. With p = (c -> n) a directed pair of the list the evaluation ran on,
 * D_p = x_n + S h - x_c its pair vector and g_p = d e_c / d D_p the gradient of the CENTRE's energy, at the
 * whole-step state (x(t), v(t)) of every absolute step t with t % sample_every == 0 (the schedule of ta_md_set_sq),
 * per frame
 *     J_conv = sum_i (1/2 m_i |v_i|^2 + e_i) v_i
 *     J_pot  = - sum_p D_p (g_p . v_n(p))          (Fan et al., PRB 92, 094301)
 *     K_ab   = sum_i m_i v_ia v_ib                 W_ab = 1/2 sum_p (g_pa D_pb + g_pb D_pa)
 * with ab in the order xx yy zz yz xz xy; Pi_ab = K_ab - W_ab = P_ab V, the sign of the barostat's record. A
 * sample's row is {J_conv[3], J_pot[3], K[6], W[6]}: TA_MD_FLUX_ROW = 18 doubles per frame. The device keeps the
 * last n_lags rows in a ring, the sum of all rows (for the means) and, over every time origin, with J = J_conv +
 * J_pot and sample number m against the lags k = 0 .. min(m, n_lags - 1),
 *     a_heat [f][k][a]  += J_a(m) J_a(m - k)             a_press[f][k][ab] += Pi_ab(m) Pi_ab(m - k)
 * The number of time origins at lag k is max(0, n_samples - k). No centre-of-mass correction is made, and no
 * partial-enthalpy correction for mixtures: in a mixture the heat current contains the interdiffusion part. Units
 * are the caller's: energy length / time for J, energy for K, W and Pi. Everything is fp64 and no sum uses
 * floating-point atomics (a centre's pairs over 16 lanes, the centres of a workgroup, then the workgroups of a frame
 * in index order): a run cut into calls reproduces the uncut run bit for bit, another skin reproduces it to
 * rounding. While a ta_md_run has this sampler running, and only then, its evaluations leave g_p as defined above:
 * one-element symmetry-function models take the per-apex backward build, not the triangle-once one, and
 * EAM / ADP / eam/fs models with analytic or tabulated pair functions take the pair kernel and the force gather on
 * the resident list, not the folded force kernels. The trajectory of such a run agrees with that of a run without
 * the sampler to rounding, not bit for bit, and a step costs more (profiles/md_flux.md).
 *   ta_md_set_flux       NULL or n_lags == 0 switches it off (the default; always allowed) and frees the buffers.
 *                        Switching on needs a resident batch and ta_md_init; it allocates and zeroes the
 *                        accumulators and forgets earlier samples (so does every further call). The life cycle is
 *                        that of ta_md_set_sampling. TA_ERR_INVALID, with the argument named by ta_last_error and
 *                        the setting left as it was: n_lags outside 0 .. TA_MD_MAX_LAGS; sample_every < 1.
 *                        TA_ERR_NOMEM when the device allocation fails; the feature is then off.
 *   ta_md_run            TA_ERR_INVALID while this feature and the barostat are both on (normalising needs one
 *                        volume). A run that fails leaves the data invalid: both getters are TA_ERR_INVALID until
 *                        ta_md_set_flux or ta_md_init is called again.
 *   ta_md_get_flux       sums [n_frames][18], a_heat [n_frames][n_lags][3], a_press [n_frames][n_lags][6]: the raw
 *                        sums; info [8] = {n_samples, n_lags, sample_every, absolute step of the newest sample or
 *                        -1, absolute step of the first sample, atoms per workgroup of the pair sweep, most
 *                        workgroups of one frame (a frame's partials are added one after another), lanes per
 *                        centre}. Any pointer may be NULL.
 *   ta_md_get_flux_rows  the rows first_lag .. first_lag + n - 1 back from the newest one (0 = the newest): rows
 *                        [n][n_frames][18] and their absolute steps [n]; either may be NULL. TA_ERR_INVALID when
 *                        first_lag < 0, n < 0 or first_lag + n exceeds the min(n_samples, n_lags) rows held. */
#define TA_MD_MAX_CHAIN 8
#define TA_MD_MAX_LAGS 4096
#define TA_MD_MAX_BINS 4096
typedef struct {
  double r_max;          /* finite, > 0, <= max(rcut, acut) of the model */
  int32_t n_bins;        /* B, 1 .. TA_MD_MAX_BINS; 0 switches the feature off (the default) */
  int32_t sample_every;  /* s >= 1 */
} ta_md_rdf_params;
typedef struct {
  double r_bond;         /* bond cutoff of every pair of elements when r_bond_pairs is NULL */
  int32_t n_bins;        /* B, 1 .. TA_MD_MAX_BINS; 0 switches the feature off (the default) */
  int32_t sample_every;  /* s >= 1 */
} ta_md_adf_params;
#define TA_MD_ORDER_MAX_DEGREES 4
#define TA_MD_ORDER_MAX_L 12
#define TA_MD_ORDER_MAX_CONN 31
typedef struct {
  double r_bond;           /* bond cutoff of every pair of elements when r_bond_pairs is NULL */
  double solid_threshold;  /* c, inside (-1, 1) */
  int32_t n_bins;          /* B, 1 .. TA_MD_MAX_BINS; 0 switches the feature off (the default) */
  int32_t sample_every;    /* s >= 1 */
  int32_t n_degrees;       /* 1 .. TA_MD_ORDER_MAX_DEGREES */
  int32_t degrees[4];      /* l, 1 .. TA_MD_ORDER_MAX_L each, no duplicates; read up to n_degrees */
  int32_t solid_degree;    /* one of the degrees */
} ta_md_order_params;
#define TA_MD_CLUSTER_MAX_SERIES 1048576
typedef struct {
  double r_link;          /* link cutoff of every pair when r_link_pairs is NULL; NaN: the model's cutoff */
  int32_t n_min;          /* 0 .. TA_MD_ORDER_MAX_CONN; 0: n_conn is not read */
  int32_t species_mask;   /* bit a: element a can be selected; non-zero, no bit at or above n_elements */
  int32_t n_bins;         /* B, 1 .. TA_MD_MAX_BINS; 0 switches the feature off (the default) */
  int32_t n_series;       /* T, 1 .. TA_MD_CLUSTER_MAX_SERIES */
  int32_t sample_every;   /* s >= 1 */
} ta_md_cluster_params;
#define TA_MD_CNA_ADAPTIVE 0
#define TA_MD_CNA_FIXED 1
#define TA_MD_CNA_TYPES 5
typedef struct {
  double r_cut;          /* fixed mode: finite, > 0, <= max(rcut, acut); ignored in adaptive mode */
  double r_max;          /* adaptive mode: candidate reach, finite, > 0, <= max(rcut, acut); NaN: the model's cutoff */
  int32_t mode;          /* TA_MD_CNA_ADAPTIVE or TA_MD_CNA_FIXED */
  int32_t n_series;      /* T, 1 .. TA_MD_CLUSTER_MAX_SERIES; 0 switches the feature off (the default) */
  int32_t sample_every;  /* s >= 1 */
} ta_md_cna_params;
typedef struct {
  int32_t n_lags;      /* L, 1 .. TA_MD_MAX_LAGS; 0 switches sampling off (the default) */
  int32_t sample_every;  /* s >= 1 */
} ta_md_sampling_params;
#define TA_MD_SQ_MAX_Q 4096
#define TA_MD_SQ_MAX_INDEX 64
typedef struct {
  int32_t n_q;           /* Q, 1 .. TA_MD_SQ_MAX_Q; 0 switches the feature off (the default) */
  int32_t n_lags;        /* L, 1 .. TA_MD_MAX_LAGS; 1: the static structure factor only */
  int32_t sample_every;  /* s >= 1 */
  int32_t currents;      /* 0, or 1: j_a(q), A_L and A_J as well */
} ta_md_sq_params;
#define TA_MD_FLUX_ROW 18
typedef struct {
  int32_t n_lags;        /* L, 1 .. TA_MD_MAX_LAGS; 0 switches the feature off (the default) */
  int32_t sample_every;  /* s >= 1 */
} ta_md_flux_params;
typedef struct {
  double kT0;           /* target, energy; <= 0 switches the thermostat off (the default) */
  double tau;           /* time, finite, > 0 */
  int32_t chain;        /* M, 1 .. TA_MD_MAX_CHAIN */
  int32_t loops;        /* L, 1 .. 16 */
  int32_t dof_removed;  /* >= 0; g = 3 n_atoms - dof_removed */
} ta_md_nhc_params;
typedef struct {
  double pressure;         /* target, energy / volume (eV / A^3) */
  double taup;             /* time constant; <= 0: barostat off */
  double compressibility;  /* volume / energy (A^3 / eV) */
  int32_t mask[3];         /* x, y, z: non-zero = the axis is free; read when isotropic == 0 */
  int32_t isotropic;       /* non-zero: one factor from the mean of the three pressures */
} ta_md_barostat_params;
typedef struct {
  double pressure;      /* P0, energy / volume (eV / A^3) */
  double tau_p;         /* time constant; <= 0: barostat off */
  int32_t chain;        /* M_p, 1 .. TA_MD_MAX_CHAIN */
  int32_t loops;        /* loops of a half-update of the barostat's chain, 1 .. 16 */
  int32_t mask[3];      /* x, y, z: non-zero = the axis is free; read when isotropic == 0 */
  int32_t isotropic;    /* non-zero: one strain rate from the mean driving force */
} ta_md_mtk_params;
int ta_md_init(ta_handle h, const double *masses, const double *velocities);
int ta_md_set_thermostat(ta_handle h, double kT0, double tau);
int ta_md_set_langevin(ta_handle h, double kT0, double friction, uint64_t seed);
int ta_md_noise(ta_handle h, int64_t step, double *xi, double *eta);
int ta_md_run(ta_handle h, int32_t n_steps, double dt, uint32_t want, int32_t record_every, double *epot,
              double *ekin, int32_t *n_rebuilds);
int ta_md_get_state(ta_handle h, double *positions, double *velocities);
int ta_md_set_barostat(ta_handle h, const ta_md_barostat_params *p);
int ta_md_get_cell(ta_handle h, double *cells);
int ta_md_get_records(ta_handle h, double *volume, double *press);
int ta_md_set_nose_hoover(ta_handle h, const ta_md_nhc_params *p);
int ta_md_get_chain(ta_handle h, double *eta, double *veta);
int ta_md_set_chain(ta_handle h, const double *eta, const double *veta);
int ta_md_get_chain_records(ta_handle h, double *e_chain);
int ta_md_set_mtk_barostat(ta_handle h, const ta_md_mtk_params *p);
int ta_md_get_mtk_state(ta_handle h, double *omega, double *xi, double *vxi);
int ta_md_set_mtk_state(ta_handle h, const double *omega, const double *xi, const double *vxi);
int ta_md_get_mtk_records(ta_handle h, double *e_baro);
int ta_md_set_sampling(ta_handle h, const ta_md_sampling_params *p);
int ta_md_get_correlations(ta_handle h, double *vacf_sum, double *msd_sum, int64_t *info);
int ta_md_get_samples(ta_handle h, int32_t first_lag, int32_t n, double *positions, double *velocities,
                      int64_t *steps);
int ta_md_set_rdf(ta_handle h, const ta_md_rdf_params *p);
int ta_md_get_rdf(ta_handle h, int64_t *counts, int64_t *info, double *r_max);
int ta_md_set_adf(ta_handle h, const ta_md_adf_params *p, const double *r_bond_pairs);
int ta_md_get_adf(ta_handle h, int64_t *counts, int64_t *info, double *r_bond_pairs);
int ta_md_set_order(ta_handle h, const ta_md_order_params *p, const double *r_bond_pairs);
int ta_md_get_order(ta_handle h, int64_t *hist_q, int64_t *hist_qbar, int64_t *hist_conn, int64_t *info,
                    double *r_bond_pairs);
int ta_md_get_order_atoms(ta_handle h, double *q, double *qbar, int32_t *n_bonds, int32_t *n_conn, double *qlm);
int ta_md_set_clusters(ta_handle h, const ta_md_cluster_params *p, const double *r_link_pairs);
int ta_md_get_clusters(ta_handle h, int64_t *hist, int64_t *series, int64_t *steps, int64_t *info, double *r_link_pairs);
int ta_md_get_cluster_atoms(ta_handle h, int32_t *label, int32_t *size);
int ta_md_set_cna(ta_handle h, const ta_md_cna_params *p);
int ta_md_get_cna(ta_handle h, int64_t *counts, int64_t *series, int64_t *steps, int64_t *info);
int ta_md_get_cna_atoms(ta_handle h, int32_t *structure, double *r_local);
int ta_md_set_sq(ta_handle h, const ta_md_sq_params *p, const int32_t *miller);
int ta_md_get_sq(ta_handle h, double *a_rho, double *a_l, double *a_j, int64_t *info, int32_t *miller);
int ta_md_get_sq_amplitudes(ta_handle h, int32_t first_lag, int32_t n, double *rho, double *cur, int64_t *steps);
int ta_md_set_flux(ta_handle h, const ta_md_flux_params *p);
int ta_md_get_flux(ta_handle h, double *sums, double *a_heat, double *a_press, int64_t *info);
int ta_md_get_flux_rows(ta_handle h, int32_t first_lag, int32_t n, double *rows, int64_t *steps);

/* Device-resident structure relaxation: the resident batch is brought to a force minimum in ONE call, every
 * frame on its own, with positions, velocities and forces staying on the device. The optimiser is FIRE
 * (Bitzek et al., PRL 97, 170201) as ASE's FIRE with downhill_check = False. Per frame, with F the forces at
 * the current positions and |.|, . over all 3 n components of the frame:
 *     before every step:  if max_i |F_i|^2 < fmax^2: the frame is converged; it does not move again in this run
 *     if first:         v = 0
 *     else if F.v > 0:  v = (1 - a) v + a F |v| / |F|;  if npos > nmin: dt = min(dt finc, dtmax), a = a fa;  npos += 1
 *     else:             v = 0;  a = astart;  dt = dt fdec;  npos = 0
 *     v += dt F;  dr = dt v;  if |dr| > maxstep: dr = dr maxstep / |dr|;  x += dr
 * (ASE's units: its FIRE treats every mass as 1.) Cells stay fixed unless ta_relax_set_cell says otherwise, positions unwrapped. Atoms of the `fixed`
 * mask have their forces read as 0 everywhere above, the convergence test included (ASE's FixAtoms), and
 * their positions are never written. Converged frames stay in the batch and are still evaluated: a run costs
 * (steps of the slowest frame) x (one evaluation of the whole batch).
 *   ta_fire_params      ASE's names; NULL at ta_relax_init means ASE's defaults
 *                       dt 0.1, dtmax 1.0, maxstep 0.2, finc 1.1, fdec 0.5, astart 0.1, fa 0.99, nmin 5.
 *   ta_relax_init       Needs a resident batch. Resets the state of every frame: v = 0, dt, a = astart,
 *                       npos = 0. fixed [n_atoms_total] (non-zero = fixed) or NULL. ta_set_frames (and ta_eval)
 *                       drop the state; ta_update_positions / ta_step keep it. The relaxation owns its
 *                       velocities: those of ta_md_init are left alone.
 *                       TA_ERR_INVALID, with the argument named by ta_last_error: dt, dtmax or maxstep not
 *                       finite or <= 0, finc < 1, fdec or fa outside (0, 1), astart outside (0, 1], nmin < 0.
 *   ta_relax_run        Continues from the kept state (v, dt, a, npos of every frame), so a run may be cut into
 *                       several calls, and a second run with a smaller fmax carries on: frames frozen by an
 *                       earlier run are tested against the new fmax and wake if they fail it. Ends when every
 *                       frame is converged, or when the frames that are not have taken max_steps steps in this
 *                       run; max_steps = 0 evaluates the state, tests it and moves nothing.
 *                       steps [n_frames]: steps the frame took in this run; converged [n_frames]: 1 / 0;
 *                       fmax_out [n_frames]: max_i |F_i| (free atoms) of the frame's final state; any may be NULL.
 *                       On return the results of the last evaluation, which is one of the final positions, are
 *                       resident as after ta_compute(want | ENERGY | FORCES), and the list bookkeeping is as
 *                       ta_md_run leaves it: each step of the run (of its slowest frame) counts as a list reuse
 *                       or a list build in ta_list_stats, *n_rebuilds (may be NULL) = lists built by this run,
 *                       rebuilds happen as in ta_md_run (skin / 2 rule tested on the device after every
 *                       drift; a failed rebuild ends the run with an error that names the step), so a
 *                       following ta_md_run or ta_step works. The host looks at the device every few steps
 *                       only, so up to 3 evaluations are enqueued past the step at which the last frame
 *                       converged; they re-evaluate unchanged positions.
 *                       A run that fails (a rebuild that finds non-finite coordinates, a device error) drops
 *                       the relaxation state, as the positions and velocities then stand somewhere on the
 *                       way: ta_relax_run and ta_relax_get_state are TA_ERR_INVALID until ta_relax_init.
 *                       A refused argument leaves the state as it was.
 *                       Every workgroup (1024 atoms) re-adds all partial sums of its frame with one
 *                       wavefront: 32 bytes per 1024 atoms of the frame, so the work per frame grows with
 *                       the square of its workgroups; negligible up to some 1e6 atoms per frame.
 *                       TA_ERR_INVALID: before ta_relax_init, fmax not finite or <= 0, max_steps < 0.
 *   ta_relax_get_state  positions / velocities [n_atoms_total][3], dt / a / npos [n_frames] of the kept state;
 *                       any may be NULL. */
typedef struct {
  double dt, dtmax, maxstep, finc, fdec, astart, fa;
  int32_t nmin;
} ta_fire_params;
int ta_relax_init(ta_handle h, const ta_fire_params *p, const uint8_t *fixed);
int ta_relax_run(ta_handle h, int32_t max_steps, double fmax, uint32_t want, int32_t *steps, int32_t *converged,
                 double *fmax_out, int32_t *n_rebuilds);
int ta_relax_get_state(ta_handle h, double *positions, double *velocities, double *dt, double *a, int32_t *npos);

/* Cells relaxed together with the atoms (ASE's UnitCellFilter under the FIRE above). Per frame of n atoms, with
 * h0 the cell when the option was switched on (rows are lattice vectors), G a 3x3 deformation gradient that
 * starts at the identity, cf the cell factor, p an external pressure and M a symmetric 0/1 mask:
 *     h = h0 G^T,   x_i = q_i G^T,   generalised coordinates: the n + 3 rows [q_1 .. q_n ; cf G]
 *     f_i    = F_i G                               (a fixed atom: 0)
 *     f_cell = -((W + p V I) G^-T) o M / cf        (hydrostatic: f_cell = I trace(f_cell) / 3 before the mask)
 * with W the library's virial (dE / d strain) and V = |det h| of the current state: minus the gradient of
 * E + p V. FIRE is the recurrence above with every ., |.| and the maxstep clamp over all 3 (n + 3)
 * components, n + 3 velocity rows, and the convergence test max_row |f_row|^2 < fmax^2 over all n + 3 rows.
 * A step with the clamped dr: q_i = x_i G^-T (recomputed from the positions, not stored); q_i += dr_i;
 * G += dr_cell / cf; h = h0 G^T; x_i = q_i G^T. Fixed atoms keep their q_i, so they move affinely with the
 * cell: the one difference from "never written" above. G may pick up a rotation (W G^-T is not symmetric),
 * as in ASE.
 *   ta_relax_cell_params  cell_factor 0 = the atoms of the frame (ASE's default); pressure in eV / A^3; mask in
 *                       Voigt order xx yy zz yz xz xy, non-zero = free; hydrostatic != 0 = ASE's
 *                       hydrostatic_strain. NULL at ta_relax_set_cell: cell_factor 0, pressure 0, mask all 1.
 *   ta_relax_set_cell   Needs ta_relax_init, which switches the option off again (as do ta_set_frames and a run
 *                       that fails). on != 0: h0 = the resident cells, G = I and cell velocities 0 for every
 *                       frame; the FIRE state of the atoms stays. on = 0: back to fixed cells; the current
 *                       cells stay. TA_ERR_INVALID with the argument named by ta_last_error and the state left
 *                       as it was: a frame that is not periodic along all three axes or has a singular cell,
 *                       cell_factor negative or not finite, pressure not finite, a mask of all zeros.
 *                       Cells handed to ta_update_positions / ta_step while the option is on replace the
 *                       relaxed ones: they become h0, G = I and the cell velocities 0.
 *   ta_relax_run        with the option on: TA_WANT_VIRIAL is added to `want`; fmax_out is the maximum over
 *                       all n + 3 rows. The cells change on the device, so the list test knows strain: with
 *                       h_ref, x_ref the cell and positions the list was built for, rc = max(rcut, acut),
 *                       A = h_ref^-1 h and u_i = x_i - x_ref,i A, every pair vector obeys
 *                       D_new = D_ref A + (u_j - u_i), and sigma_min(A) >= 1 - |A - I|_F; the list is stale when
 *                       lim = (skin - (rc + skin) |A - I|_F) / 2 <= 0 or some |u_i|^2 >= lim^2 (A = I: the
 *                       skin / 2 rule; skin = 0: every step rebuilds). A periodic width shrinks by less than
 *                       rc / (rc + skin) while a list is valid, so while the option is on the triangle-once
 *                       backward pass is selected only when every periodic width of the list's cells exceeds
 *                       rc + skin (ta_backward_variant reports what ran). When a run ends with cells other
 *                       than those of its list, it builds one list for the final state and evaluates it
 *                       again (counted in *n_rebuilds and ta_list_stats; results agree up to summation
 *                       order): ta_md_run, ta_step, ta_update_positions and a fixed-cell ta_relax_run then
 *                       find the cells the list was built for, and "cells = NULL: unchanged" of
 *                       ta_update_positions means the relaxed cells. A run may still be cut into several calls.
 *   ta_relax_get_cell   cells [n_frames][9] (= h0 G^T), deform [n_frames][9] (G), cell_velocities
 *                       [n_frames][9] (of the rows cf G), cell_fmax [n_frames] (max row |f_cell| of the last
 *                       state a cell run tested; 0 before one); any may be NULL. Needs ta_relax_init; with the
 *                       option never switched on G = I and the velocities are 0. */
typedef struct {
  double cell_factor;
  double pressure;
  int32_t mask[6];
  int32_t hydrostatic;
  int32_t reserved_;
} ta_relax_cell_params;
int ta_relax_set_cell(ta_handle h, int on, const ta_relax_cell_params *p);
int ta_relax_get_cell(ta_handle h, double *cells, double *deform, double *cell_velocities, double *cell_fmax);

/* Minimum-energy paths: a nudged elastic band under the FIRE above. The resident batch of F >= 3 frames is the
 * band: image 0 and image F - 1 are fixed endpoints, images 1 .. F - 2 move. All images have the same n atoms
 * in the same order with the same species, and the same cell and periodicity. Positions are unwrapped, and
 * differences between images are plain differences, with no minimum-image convention. With X_i, E_i, F_i the
 * positions, energy and forces of image i, forces of `fixed` atoms read as 0, and ., |.| taken over the 3n
 * components of an image:
 *     d+ = X_{i+1} - X_i,   d- = X_i - X_{i-1}
 *     if   E_{i+1} > E_i > E_{i-1}:  t = d+
 *     elif E_{i+1} < E_i < E_{i-1}:  t = d-
 *     else: hi = max(|E_{i+1}-E_i|, |E_{i-1}-E_i|), lo = min(the same two)
 *           t = d+ hi + d- lo   if E_{i+1} > E_{i-1}   else   t = d+ lo + d- hi
 *     tau = t / |t|                      (t.t == 0: tau = 0)
 *     B_i = F_i - (F_i.tau) tau + k (|d+| - |d-|) tau          ordinary image
 *     B_c = F_c - 2 (F_c.tau) tau                               climbing image, if climb
 *     B = 0 for images 0 and F-1 and for every fixed atom
 * This is the improved tangent of Henkelman and Jonsson (J. Chem. Phys. 113, 9978); it matches ASE's
 * NEB(method='improvedtangent', climb=...) with a single spring constant k. The climbing image c is the
 * interior image of highest energy, re-chosen at every step; on a tie the lowest index wins.
 * FIRE then runs on B exactly as documented for ta_relax_run, but as ONE system over the whole band, as ASE
 * does when an optimiser is attached to a NEB: one dt, one a and one npos; F.v, |F|, |v| and the maxstep clamp
 * are taken over all 3n(F - 2) moving components; convergence is max over all moving atoms of |B_i| < fmax. No
 * image freezes on its own: an image under fmax now may be over it once its neighbours move. Both endpoint
 * images are still evaluated at every step.
 *   ta_band_params      k in eV / A^2; climb != 0: the climbing image. NULL at ta_relax_set_band: k = 0.1
 *                       (ASE's default), climb = 0.
 *   ta_relax_set_band   Needs ta_relax_init, which supplies the FIRE parameters and the `fixed` mask and
 *                       switches the option off again (as do ta_set_frames and a run that fails). on != 0
 *                       resets the FIRE state of the band: v = 0, dt, a = astart, npos = 0, first; calling it
 *                       again, for example to turn climb on after a first run, restarts the optimiser, as one
 *                       does with ASE. on = 0 returns to independent frames with their per-frame states reset
 *                       the same way, also when the band was not on: unlike ta_relax_set_cell(on = 0), which only
 *                       drops its flag, this call always zeroes the FIRE velocities and resets dt, a and npos of
 *                       every frame, so do not call it in the middle of a relaxation whose state is to carry
 *                       on. TA_ERR_INVALID, with the argument named by ta_last_error and the state
 *                       left as it was: fewer than 3 frames; frames that differ in atom count, species order,
 *                       cell or pbc; k not finite or <= 0; the cell option (ta_relax_set_cell) is on.
 *                       ta_relax_set_cell(on != 0) while the band is on is TA_ERR_INVALID.
 *   ta_relax_run        with the option on: steps [f] and converged [f] carry the band's one value for every f;
 *                       fmax_out [f] is the band's max |B_i| over the moving atoms; max_steps = 0 evaluates,
 *                       forms B and tests, and moves nothing. The skin / 2 test per atom, the rebuilds and the
 *                       list bookkeeping are those of a run without the option. ta_relax_get_state reports
 *                       the band's dt / a / npos for every frame.
 *   ta_relax_get_band   band_forces / tangents [n_atoms_total][3] (B and tau; rows of the endpoint images are
 *                       0), energies [n_frames], *climbing (image index, -1 without climb) of the state the
 *                       last band run ended on; any may be NULL. Needs a band run to have been made since
 *                       ta_relax_set_band(on != 0); max_steps = 0 counts. */
typedef struct {
  double k;
  int32_t climb;
  int32_t reserved_;
} ta_band_params;
int ta_relax_set_band(ta_handle h, int on, const ta_band_params *p);
int ta_relax_get_band(ta_handle h, double *band_forces, double *tangents, double *energies, int32_t *climbing);

/* Enqueue all further work of this handle on `stream` (a hipStream_t of the
 * handle's device owned by the caller, e.g. the stream a RCCL collective is
 * ordered against); NULL restores the handle's own stream (to name the legacy
 * default stream, whose handle is also 0, pass hipStreamLegacy). Drains the old
 * stream first. */
int ta_set_stream(ta_handle h, void *stream);

/* blocks until the handle's stream is idle */
int ta_synchronize(ta_handle h);

/* sum of the resident batch's frame energies, left on the device for a
 * collective: returns a device pointer to one double (valid until destroy). */
int ta_batch_energy_device_ptr(ta_handle h, void **dptr);

/* enqueues, on the handle's stream, a device-to-device copy of that double into
 * `dst_device` (e.g. the buffer a RCCL all-reduce will sum across ranks). */
int ta_copy_batch_energy(ta_handle h, void *dst_device);
/* Alternative without the copy: later ta_compute calls write the batch energy (one double) straight
 * to `dst_device` (caller-owned device memory, e.g. the buffer a collective reduces in place);
 * NULL restores the library's own buffer. Takes effect for launches made after the call;
 * ta_set_frames restores the library's own buffer. */
int ta_set_batch_energy_target(ta_handle h, void *dst_device);

/* Host-only (no GPU needed): the neighbour list the library builds for one
 * frame, i.e. `ase.neighborlist.neighbor_list('ijS', atoms, rc)` as called at
 * transformer/universal.py:58, sorted by centre then neighbour species then
 * distance. Output arrays are malloc'ed by the library; release with ta_free.
 * rev[p] = index of the reverse pair (j -> i, -S). */
int ta_neighbor_list(const ta_frame *frame, int32_t n_elements, double rc, int64_t *n_pairs,
                     int32_t **i, int32_t **j, int32_t **shift /*[n][3]*/, int32_t **rev);
void ta_free(void *p);

/* --- training support: gradients with respect to the network weights -----------
 * Parameter vector layout = `ta_model_desc.weights`: per element (sorted) -- for EAM / ADP models
 * per nn-function slot (rho[element], embed[element], phi / dipole / quadrupole[pair]; analytic and
 * tabulated slots hold nothing) --, per layer W[in][out] row-major then b[out]. */

/* length of that vector */
int ta_param_count(ta_handle h, int64_t *n_params);

/* replace the MLP weights of a live handle (an optimiser step), same layout */
int ta_update_weights(ta_handle h, const double *weights, int64_t n_weights);

/* grad = sum_f frame_coeff[f] * dE_f/dtheta for the resident batch: with frame_coeff[f] = dL/dE_f
 * this is the gradient of a loss L(E_1 .. E_F), what `tf.gradients(loss, variables)` gives for the
 * energy term of nn/losses.py:204-285. The batch's descriptors are computed once and reused. */
int ta_energy_gradient(ta_handle h, const double *frame_coeff, double *grad, int64_t n_grad);

/* The whole loss gradient of an energy + forces + stress loss (nn/losses.py:204-437 through
 * `tf.gradients`, nn/opt.py:89-166) for the per-atom MLP models, analytically. With u = dL/dF per
 * atom and the symmetric Y = (dL/dstress) / V per frame, sum u.F + sum Y.W is the directional
 * derivative D_delta E of the energy along
 *     dR = R.Y - u   [n_atoms_total][3],      dh = h.Y   [n_frames][9]
 * (W = -F^T R + (dE/dh)^T h, basic.py:306-316), and
 *     grad = d/dtheta ( sum_f frame_coeff[f] E_f  +  D_delta E ).
 * The descriptors do not depend on theta: their Jacobian with respect to the pair vectors is made
 * once per resident batch (one backward launch per descriptor channel), every call then costs a
 * pair sweep and ONE second-order pass through the MLP. frame_coeff, dR, dh may each be NULL (= 0).
 * dG_out (may be NULL): the directional derivative of the raw descriptors [n_atoms_total][D] that
 * entered the pass (parity tests).
 * EAM / ADP models with nn functions (the reference's default potentials, alloy.py:110-112, adp.py:120-124)
 * since round 3: every network enters D_delta E through its value and its input derivative at known
 * points, so the gradient is one second-order pass per network over its rows (pairs / atoms); dG_out
 * must be NULL. The sutton90 / Be/1 / grimes families: TA_ERR_UNSUPPORTED (callers difference
 * ta_energy_gradient on displaced frames instead). */
int ta_loss_gradient(ta_handle h, const double *frame_coeff, const double *dR, const double *dh,
                     double *grad, int64_t n_grad, double *dG_out);

/* The loss gradient of a temperature-dependent model (ta_model_desc.finite_temperature), whose loss
 * has three energy terms (finite_temperature.py:358-388): with per-frame coefficients
 * b = coeff_free_energy (dL/dF_f), a = coeff_energy (dL/dU_f), g = coeff_eentropy (dL/dS_f) and the
 * force / stress direction (dR, dh) of F, built as for ta_loss_gradient,
 *     grad = d/dtheta ( sum_f (a U_f + b F_f + g S_f)  +  D_delta F ).
 * One second-order pass per 16-atom tile through H, U and S (ta_td_train.hip). Any coefficient array
 * and the direction may be NULL (= 0); dG_out as for ta_loss_gradient (needs a direction). Returns
 * TA_ERR_INVALID for a model that is not temperature-dependent, and TA_ERR_UNSUPPORTED for a direction
 * on a skin-filtered batch. On such a model ta_energy_gradient(h, c, ...) and
 * ta_loss_gradient(h, c, dR, dh, ...) are this call with b = c and a = g = NULL. */
int ta_td_loss_gradient(ta_handle h, const double *coeff_free_energy, const double *coeff_energy,
                        const double *coeff_eentropy, const double *dR, const double *dh, double *grad,
                        int64_t n_grad, double *dG_out);

/* The `nn` filter network of a GRAP model (grap.py:620-643) as trainable parameters, as the reference
 * trains it by default (NNAlgorithm.trainable, grap.py:235). Layout of its vector: per layer
 * W[in][out] row-major, then b[out] (zeros where a layer has no bias: the output layer).
 *   ta_filter_param_count    its length; 0 for a model without a filter network
 *   ta_update_filter_weights replace the network of a live handle (synchronises the stream first); the
 *                            resident descriptors and pair Jacobians are recomputed on their next use
 *   ta_grap_loss_gradient    grad = [MLP weights (ta_param_count) | filter network (ta_filter_param_count)]
 *                            of d/dtheta ( sum_f frame_coeff[f] E_f + D_delta E ), arguments as
 *                            ta_loss_gradient (frame_coeff, dR, dh may each be NULL = 0; dR = dh = NULL:
 *                            the energy term only). The descriptors' tangent comes from dual arithmetic
 *                            through the forward expression (no pair Jacobian), the MLP part from its
 *                            second-order pass, the filter part from per-pair adjoints of the network's
 *                            value and r-derivative and a second-order sweep through the network.
 *                            TA_ERR_UNSUPPORTED for models that are not GRAP with the `nn` algorithm, for
 *                            temperature-dependent models and on a skin-filtered batch. */
int ta_filter_param_count(ta_handle h, int64_t *n_params);
int ta_update_filter_weights(ta_handle h, const double *weights, int64_t n_weights);
int ta_grap_loss_gradient(ta_handle h, const double *frame_coeff, const double *dR, const double *dh,
                          double *grad, int64_t n_grad);

/* Constants of the analytic functions of an EAM model as trainable parameters. The reference makes
 * every constant of its empirical potentials a tf.Variable (potentials/potentials.py:129-163;
 * zjw04.py: shared variables per element) trained under the same loss. Layout of the vector:
 * element e, constant k -> [20 e + k] in the order of the model description's `eam_el` rows
 * (Zjw04: r_eq f_eq rho_e rho_s alpha beta A B kappa lamda Fn0..Fn3 F0..F3 eta Fe), then the
 * Zjw04xcp cross terms [20 nel + 7 pt + q] (r_eq A B alpha beta kappa lamda), pt = sorted pair type,
 * then for ADP models the dipole / quadrupole constants [20 nel + 7 npt + 8 pt + k]
 * (d1 d2 d3 q1 q2 q3 h rc; mishin.py:62-66).
 *   ta_constant_count     length of the vector
 *   ta_get_constants      current values
 *   ta_update_constants   new values (finite); synchronises the stream first
 *   ta_constant_gradient  d/dconstants of  sum_f frame_coeff[f] E_f + D_(dR, dh) E  on the resident
 *                         batch, arguments as ta_loss_gradient. Forward-mode (dual numbers), one
 *                         pass over the pairs per constant in a single launch. Models that mix
 *                         networks or tables with analytic functions (round 3): the functions
 *                         without constants enter as plain values (exact forward pass), an
 *                         embedding network through F', F''; callers take the weights' half of
 *                         the gradient from ta_loss_gradient. */
int ta_constant_count(ta_handle h, int64_t *n_constants);
int ta_get_constants(ta_handle h, double *constants, int64_t n_constants);
int ta_update_constants(ta_handle h, const double *constants, int64_t n_constants);
int ta_constant_gradient(ta_handle h, const double *frame_coeff, const double *dR, const double *dh,
                         double *grad, int64_t n_grad);

/* Analytic second derivatives of the resident batch's energy: for each of `n_dir` directions
 * (dR [n_dir][n_atoms_total][3] displacements of the atoms, dh [n_dir][n_frames][9] of the cells; either
 * may be NULL; BOTH NULL = unit displacements first .. first + n_dir - 1 of the 3 N, direction d moving
 * atom d / 3 along axis d % 3; `first` is ignored otherwise)
 * the directional derivative of the forces, dF [n_dir][n_atoms_total][3] = d F / d eps = -(H v), and of
 * the virials, dW [n_dir][n_frames][9] (may be NULL). Replaces `tf.hessians(energy, positions)`
 * (nn/basic.py:411-421: Hessian column d = -dF[d]) and the cell derivative of the virial behind the
 * elastic constants (nn/constraint/elastic.py:24-44: dh = unit matrices, dR = NULL). Forward-mode
 * (dual-number) tangents through the analytic force kernels: exact, no step size. Available for EAM and
 * ADP models whose functions are of the Zjw04 / MishinH families, tabulated or networks (nn pair functions through
 * their tables, embedding networks by a second-derivative sweep), and (round 3) for the
 * symmetry-function + MLP models with integer zetas and the GRAP + MLP models (per direction: the descriptors' tangent through the
 * pair Jacobians, the MLP's Hessian-vector product, then the backward expression in dual arithmetic);
 * TA_ERR_UNSUPPORTED otherwise (the caller then differences the analytic forces). At most 65535
 * directions per call. */
int ta_hessian_vectors(ta_handle h, int32_t n_dir, int32_t first, const double *dR, const double *dh, double *dF,
                       double *dW);

/* "nn" pair functions of an EAM / ADP model (rho(r), phi(r), u(r), w(r) as `convolution1x1` networks of
 * the pair distance, nn/eam/eam.py:174-190 — the reference's DEFAULT potentials, alloy.py:110-112):
 * `on` != 0 evaluates them through cubic Hermite tables of 32769 knots over [0, rcut] that the
 * library builds from the networks (value and derivative exact at every knot; rebuilt by
 * ta_update_weights), `on` = 0 evaluates the networks for every pair. Tables are the default for
 * inference (environment TA_EAM_NN_TABLES=0 turns them off at ta_create); they differ from the exact
 * evaluation by ~1e-12 eV per structure, and they are how the reference deploys these potentials
 * itself (`export_to_setfl`, alloy.py:198-381, with a ~30x coarser table). Weight gradients
 * (ta_energy_gradient) need the networks: the first such call switches the handle to exact
 * evaluation for good, after which `on` != 0 is ignored. The embedding networks F(rho) are always
 * exact. No effect on models without nn pair functions. Drops nothing resident: the next
 * ta_compute uses the new mode (call ta_set_frames again if a Verlet skin is in use). */
int ta_set_nn_tables(ta_handle h, int on);

/* The `nn` filter network of a GRAP model (grap.py:620-643) through a table, for inference. `on` != 0
 * tabulates the network once, as cubic Hermite pieces of all K outputs over the network's own input x
 * (h_abck_modifier 0: r in [0, rcut]; 1: r / rcov in [0, rcut / min rcov]; 2: exp(-r / rcov) in [0, 1];
 * rcov of the centre's element), value and x-derivative exact at every knot, `n_knots` knots (0 = the
 * library default, 4097; otherwise 5 .. 2^20 + 1, else TA_ERR_INVALID). A step then costs one 32-byte
 * read and 3 to 5 FMAs per (pair, filter) instead of the network, and the per-pair filter buffer and the
 * geometry pre-pass are gone. Forces use the derivative of the same cubic, so energy and forces stay
 * consistent. `on` = 0 drops the table. OFF by default: the exact evaluation is what a handle does unless
 * asked. At the default knot count the two differ by less than 1e-11 eV and 1e-10 eV/A per structure.
 * Synchronises the stream and invalidates the resident descriptors and pair Jacobians; nothing resident is
 * lost, Verlet-skin lists included. ta_update_filter_weights rebuilds the table. Entries that form a weight
 * gradient on a GRAP handle (ta_energy_gradient, ta_loss_gradient, ta_grap_loss_gradient,
 * ta_td_loss_gradient) need the network itself: the first such call switches the handle to exact
 * evaluation for good, after which `on` != 0 is ignored. ta_hessian_vectors evaluates exactly for the
 * duration of the call and leaves the table on. No effect (TA_OK) on a model without a filter network.
 *   ta_filter_table_knots    the knot count in use, 0 while the handle evaluates the network exactly */
int ta_set_filter_tables(ta_handle h, int on, int32_t n_knots);
int ta_filter_table_knots(ta_handle h, int32_t *n_knots);

/* Tables of an EAM / ADP model's functions (analytic, nn or tabulated) on caller-supplied abscissae: what
 * `EamAlloyNN.export_to_setfl` (nn/eam/alloy.py:198-381) evaluates through a TF session before it
 * writes a LAMMPS setfl file. Rows: elements (sorted) for rho(r) [n_elements][n_r] and F(rho)
 * [n_elements][n_rho]; element pairs a <= b (upper triangle, row-major) for phi(r), and for an
 * ADP model u(r), w(r) (may be NULL), each [n_pairs][n_r]. For an eam/fs model `rho_of_r` is
 * [n_elements^2][n_r], rows rho[centre][neighbour] in the slot order of `n_eam_nets`. Evaluated by
 * the same device functions the energy kernels use. */
int ta_eam_tabulate(ta_handle h, int32_t n_r, const double *r, int32_t n_rho, const double *rho,
                    double *rho_of_r, double *phi_of_r, double *embed_of_rho, double *u_of_r,
                    double *w_of_r);

/* --- measurement and diagnostics ------------------------------------------------------------------
 * Used by bench.py, scripts/ and tests/ only; NOT part of the drop-in path (nothing in
 * tensoralloy_amd/calculator.py or transformer/ calls them, and the reference has no counterpart). */

/* Measurement (bench.py): runs `warmup` untimed then `steps` timed passes of
 * ta_compute over the resident batch, timed with HIP events on the handle's
 * stream. total_ms = wall of the `steps` passes; kernel_ms[k] (may be NULL) =
 * average duration per pass of kernel slot k, measured in a second run with
 * events around every launch. */
int ta_time_compute(ta_handle h, uint32_t want, int32_t warmup, int32_t steps,
                    double *total_ms, double *kernel_ms /*[TA_N_KERNEL_SLOTS]*/);

/* Measurement (bench.py, SURVEY 8(d) "achievable-copy figure"): device-to-device copy of `bytes`
 * bytes on the handle's stream, three ways (grid-stride kernel with 16 B per lane and four loads in
 * flight, the same with non-temporal accesses, the runtime's hipMemcpyAsync), each with `reps` timed
 * repetitions after 2 untimed ones; *gbs = the best (bytes read + bytes written) / average time, GB/s. */
int ta_measure_hbm_copy(ta_handle h, int64_t bytes, int32_t reps, double *gbs);

/* Measurement (bench.py, SURVEY 8(d) FP64 figure): number of unordered neighbour pairs {j, k} of the
 * resident batch's centres with r_ij, r_ik and r_jk all below acut, i.e. the triples whose G4 term
 * (sf.py:126-173) is not identically zero; ta_batch_info.n_triples counts all of them. Runs one
 * energy evaluation first (the count reads the pair records). */
int ta_count_contributing_triples(ta_handle h, int64_t *n_contributing);

/* Triangle-once angular backward pass. A triangle {i, j, k} of three distinct atoms with all sides below
 * acut adds a G4 term at each of its three apexes; the backward pass of one-element models with the
 * default zeta grid (1, 4) evaluates the three terms together, once, at the triangle's owner: with the
 * atom indices sorted, a < b < c, the owner is the one at rank t(a + b + c) in {0, 1, 2}
 * (ta_device.h: triangle_owner_rank). It is used when every periodic cell width of the batch exceeds
 * max(rcut, acut) (two images of one atom are then never in one triangle); otherwise, and for every
 * other model, the per-apex pass runs. Forces, energies and virials are the same up to the order of
 * the sums.
 *   ta_set_triangles         `on` = 0 keeps the per-apex pass for this handle (default 1); takes effect
 *                            at the next ta_compute.
 *   ta_backward_variant      the angular backward builds the last evaluation with forces ran:
 *                            0 none, bit 0 per apex, bit 1 triangles.
 *   ta_count_owned_triangles like ta_count_contributing_triples, restricted to the triples whose centre
 *                            owns the triangle (3 x owned = contributing when the triangle pass applies).
 *   ta_triangle_owner        the rule on the host: owner[t] = the owning atom of triangle
 *                            {abc[3t], abc[3t+1], abc[3t+2]}, or -1 when the three are not distinct. */
int ta_set_triangles(ta_handle h, int on);
int ta_backward_variant(ta_handle h, int32_t *variant);
int ta_count_owned_triangles(ta_handle h, int64_t *n_owned);
int ta_triangle_owner(int64_t n, const int32_t *abc, int32_t *owner);

/* Which per-atom network kernel the last evaluation launched (read-only; the dispatch does not read it).
 * The network runs as one of several builds chosen by shape and batch size: the generic 16-row tile, one
 * wavefront per tile (1-3 hidden layers up to 64 wide, from 1024 tiles), four or eight wavefronts per
 * tile (widths up to 64 / 128, fewer tiles), each as a one-element and an all-elements launch, or the
 * temperature-dependent head.
 *   info[0] family: TA_MLP_NONE (nothing launched yet), TA_MLP_TILE, TA_MLP_TILE_ALL, TA_MLP_WAVE,
 *           TA_MLP_WAVE_ALL, TA_MLP_QUAD, TA_MLP_QUAD_ALL or TA_MLP_TD
 *   info[1] threads per workgroup
 *   info[2] hidden layers of the wave / quad build (template argument LH), else 0
 *   info[3] wavefronts per tile of the quad build (NT: 4 or 8), else 0
 *   info[4], info[5] grid size x, y
 *   info[6] dynamic LDS bytes per workgroup
 *   info[7] activation derivatives: TA_MLP_DA_REGISTERS (wave, quad), TA_MLP_DA_LDS or TA_MLP_DA_GLOBAL (the
 *           global scratch slab) */
enum { TA_MLP_NONE = 0, TA_MLP_TILE = 1, TA_MLP_TILE_ALL = 2, TA_MLP_WAVE = 3, TA_MLP_WAVE_ALL = 4, TA_MLP_QUAD = 5,
       TA_MLP_QUAD_ALL = 6, TA_MLP_TD = 7 };
enum { TA_MLP_DA_REGISTERS = 0, TA_MLP_DA_LDS = 1, TA_MLP_DA_GLOBAL = 2 };
int ta_mlp_launch_info(ta_handle h, int64_t *info /*[8]*/);

/* Which body the 16-row tile kernels of the last evaluation ran (read-only, like ta_mlp_launch_info):
 * TA_MLP_BODY_NONE when the last launch was not a tile launch, TA_MLP_BODY_GENERIC (every network shape),
 * TA_MLP_BODY_SCALAR (hidden layers without skip connections and one linear output unit: no padded output-layer
 * GEMMs, no elementwise passes) or, for an all-elements launch whose networks differ, TA_MLP_BODY_MIXED. Elements
 * without atoms in the batch do not count. TA_MLP_TILE_GENERIC=1 in the environment at ta_create forces the
 * generic body. */
enum { TA_MLP_BODY_NONE = 0, TA_MLP_BODY_GENERIC = 1, TA_MLP_BODY_SCALAR = 2, TA_MLP_BODY_MIXED = 3 };
int ta_mlp_tile_body(ta_handle h, int32_t *body);

/* debugging / parity: host copy of the pair list of the resident batch
 * (centre, neighbour, shift[3]) in the library's order. Arrays sized n_pairs. */
int ta_get_pairs(ta_handle h, int32_t *i, int32_t *j, int32_t *shift /*[n][3]*/);

/* debugging / parity: the whole neighbour list as the kernels read it (read-only; changes no state).
 * Two views: TA_LIST_RESIDENT is the list that was built (under a Verlet skin, the skin list);
 * TA_LIST_KERNEL is the list the next evaluation runs on: the exact list extracted from the skin list
 * where the model's kernels take one (second-generation symmetry-function kernels, plain EAM), else the
 * resident list again.
 *   ta_list_info  info[0] atoms, [1] elements, [2] n_slots: length of the pair arrays (the exact list is
 *                 compacted in place, group by group of 16 centres, so it has the skin list's slots and
 *                 leaves some unused), [3] n_blk: runs of the angular kernels' workgroup packing (0:
 *                 none), [4] cap: pair records one such workgroup stages, [5] builder of the resident
 *                 list: 0 host, 1 one-pass, 2 two-pass, [6] 1 when this view is an exact list extracted
 *                 from a skin list, [7] 1 when its reverse index is the lookup through the skin list
 *                 (no array of its own on the device).
 *   ta_get_list   waits for the stream and copies to the host; null pointers are skipped. Centre i owns
 *                 the slots [pair_start[i], pair_stop[i]); pair_stop[i] = pair_start[i + 1] where the
 *                 device keeps no stops. pair_start[atoms] is the end of the resident list in both views.
 *                 seg_start[i (elements + 1) + s] is the first slot of centre i whose neighbour is of
 *                 element s; its closing entry [atoms (elements + 1)] is read from the device where a
 *                 device builder made the resident list, else it is the last centre's stop.
 *                 pair_rev[p] is the slot of the reverse pair (j -> i, -S); where the device looks it up
 *                 (info[7]) the same lookup is made here for the slots a centre owns, -1 elsewhere.
 *                 blk_center[b] is the first centre of run b, blk_center[n_blk] closes the last run; not
 *                 written when n_blk = 0. Slots no centre owns hold no defined values. */
enum { TA_LIST_RESIDENT = 0, TA_LIST_KERNEL = 1 };
int ta_list_info(ta_handle h, int32_t which, int64_t *info /*[8]*/);
int ta_get_list(ta_handle h, int32_t which, int32_t *pair_start /*[N+1]*/, int32_t *pair_stop /*[N]*/,
                int32_t *seg_start /*[N*(nel+1)+1]*/, int32_t *pair_i, int32_t *pair_j,
                int32_t *pair_shift /*[n_slots][3]*/, int32_t *pair_rev, int32_t *blk_center /*[n_blk+1]*/);

/* Harmonic phonons (replaces the phonopy step behind analysis/phonon.py: dynamical matrices, frequencies,
 * normal modes and the density of states from the force constants of a supercell). Everything is fp64, there
 * are no floating-point atomics and every sum has a fixed order: the same inputs give the same bits, however the
 * q-points are chunked. Complex arrays are interleaved (re, im) doubles.
 *   TA_PHONON_MAX_ORDER   the eigensolver's largest matrix: 3 n_basis <= 48, that is 16 atoms in the home cell
 *                         (with eigenvectors one such matrix takes 75 KB of a workgroup's LDS).
 *   TA_PHONON_THZ         nu [THz] = sign(l) sqrt(|l|) TA_PHONON_THZ for an eigenvalue l in eV / A^2 / amu:
 *                         1000 fs / (2 pi) with fs = one femtosecond in A sqrt(amu / eV). Imaginary modes
 *                         come out negative.
 *   ta_phonon_set_cell    declares the ONE resident frame (N atoms) a supercell whose first n_basis atoms are
 *                         the home cell. basis_of [N]: the home atom each atom is an image of (basis_of[b] = b
 *                         for b < n_basis); mass [n_basis] amu, > 0; start [n_basis N + 1], vec [start[last]][3]:
 *                         for the pair (b, s) at b N + s the shortest vectors (A) from home atom b to the
 *                         periodic images of atom s under the supercell lattice, each weighted 1 / their number
 *                         (phonopy's convention). q_chunk: q-points per internal pass, rounded up to a multiple
 *                         of 64; 0 = chosen to keep the work space near 128 MB. Drops force constants set
 *                         before. TA_ERR_INVALID: no or more than one resident frame, n_basis outside
 *                         1 .. min(N, TA_PHONON_MAX_ORDER / 3), a basis_of outside the home cell, a mass that is
 *                         not finite and > 0, start[0] != 0 or start not monotone. ta_set_frames drops the state.
 *   ta_phonon_force_constants   Phi[b][s][a][c] = d2E / d x_ba d x_sc = -dF of ta_hessian_vectors for the unit
 *                         displacements 0 .. 3 n_basis - 1, kept on the device; phi [n_basis][N][3][3] (may be
 *                         NULL) receives a copy. Fails as ta_hessian_vectors does for models without the
 *                         analytic path.
 *   ta_phonon_load_force_constants   the same slot from the host (finite differences, a file).
 *   ta_phonon_frequencies q_cart [Q][3] Cartesian wave vectors in 1 / A (2 pi included). Builds
 *                             D[q][3b+a][3b'+c] = (m_b m_b')^(-1/2) sum_{s in b'} Phi_ac(b, s) (1/mult) sum_r exp(i q.r)
 *                         and solves its Hermitian part (D + D^H) / 2. freq [Q][n] THz ascending (n = 3 n_basis);
 *                         eigvec [Q][n][n] complex or NULL, row m = the unit eigenvector of mode m;
 *                         info[0] = matrices the solver did not converge (0 in a sound run; never silent).
 *   ta_phonon_dos         histogram of the same frequencies, which never leave the device: bin
 *                         k = floor((nu - nu_min) * inv_dnu) with inv_dnu = n_bins / (nu_max - nu_min) formed
 *                         in double by the library; total [n_bins] counts of modes; partial
 *                         [n_basis][n_bins] (may be NULL) the modes' weights sum_a |e_ba|^2 per home atom;
 *                         info[0] as above, info[1] = modes outside [nu_min, nu_max), which are counted nowhere
 *                         else. n_bins 1 .. TA_MD_MAX_BINS, nu_max > nu_min, both finite.
 *   ta_phonon_eigh        the eigensolver alone, on `batch` caller matrices A [batch][n][n] complex (row-major;
 *                         the Hermitian part is solved): w [batch][n] ascending, V [batch][n][n] as eigvec or NULL,
 *                         info[0] unconverged matrices. Cyclic Jacobi in a parallel ordering until the
 *                         off-diagonal norm is <= n eps ||A||_F. Needs no resident batch. n above
 *                         TA_PHONON_MAX_ORDER: TA_ERR_UNSUPPORTED.
 *   ta_phonon_eigh_group  matrices of order n one workgroup of the solver takes (for tests of its edges). */
#define TA_PHONON_MAX_ORDER 48
#define TA_PHONON_THZ (1000.0 * 0.09822694788464063 / (2.0 * 3.141592653589793))
typedef struct ta_phonon_params {
  int32_t n_basis;
  int32_t q_chunk;
} ta_phonon_params;
int ta_phonon_set_cell(ta_handle h, const ta_phonon_params *p, const int32_t *basis_of, const double *mass,
                       const int32_t *start, const double *vec);
int ta_phonon_force_constants(ta_handle h, double *phi);
int ta_phonon_load_force_constants(ta_handle h, const double *phi);
int ta_phonon_frequencies(ta_handle h, int64_t Q, const double *q_cart, double *freq_THz, double *eigvec,
                          int64_t *info /*[1]*/);
int ta_phonon_dos(ta_handle h, int64_t Q, const double *q_cart, int32_t n_bins, double nu_min, double nu_max,
                  uint64_t *total, double *partial, int64_t *info /*[2]*/);
int ta_phonon_eigh(ta_handle h, int32_t n, int64_t batch, const double *A, double *w, double *V, int64_t *info /*[1]*/);
int ta_phonon_eigh_group(int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* TENSORALLOY_AMD_H */
