"""
Molecular dynamics on the device: `DeviceMD` drives `Engine.md_run` (`ta_md_run`), which integrates the
resident batch for n steps without moving coordinates, velocities or forces through the host.

Units are ASE's: Angstrom, eV, amu, and therefore the time unit Angstrom sqrt(amu / eV); `fs` and `kB`
are the same numbers as `ase.units.fs` and `ase.units.kB`. The integrator is ASE's `VelocityVerlet`, with
one of three thermostats: ASE's `NVTBerendsen.scale_velocities` (`taut`), which steers the temperature but
does not sample the canonical ensemble; the second-order scheme of ASE's `Langevin` (`friction`), which
does, with noise; or a Nose-Hoover chain (`tdamp`), which does without any. None of them removes the
centre-of-mass momentum (`maxwell_boltzmann(..., zero_momentum=True)` hands
out velocities without any; under Langevin the centre of mass then diffuses like one heavy particle).

The Langevin noise is made on the device by a counter-based generator (Philox4x32-10, then Box-Muller): a
pure function of (seed, step since the start, atom, component). A trajectory therefore depends on the seed
alone, not on how `run` is cut into calls, on the skin or on list rebuilds, and `Engine.md_noise(step)` hands
out the very numbers of a step.

The Nose-Hoover chain (names as ASE's `NoseHooverChainNVT`: `tdamp`, `tchain`, `tloop`; masses as LAMMPS
`fix nvt`) is deterministic and time-reversible, so velocity autocorrelations, diffusion constants and spectra
can be taken from the thermostatted run. Every frame has g = 3 n - `dof_removed` degrees of freedom and a
chain of `tchain` thermostats (eta_k, veta_k) with Q_1 = g kT tdamp^2 and Q_k = kT tdamp^2; a step is a
half-update of the chain over dt / 2 (`tloop` loops), the velocity Verlet step, and another half-update, each
of which multiplies the frame's velocities by one factor. The scheme is written out in
include/tensoralloy_amd.h. The conserved quantity
    H' = ekin + epot + sum_k Q_k veta_k^2 / 2 + g kT eta_1 + kT sum_{k>=2} eta_k
is what `get_conserved_energy()` returns; the records of a run under this thermostat are taken after the
closing half-update of a step, so that the three parts add up to H' at every slot (`Engine.md_run` hands out
the chain part as `echain`). To restart, keep `Engine.md_state()` and `Engine.md_chain()` and hand them to
`set_frames` / `md_init` and `Engine.md_set_chain`.

Constant pressure: with `pressure`, `taup` and `compressibility` the cells follow a Berendsen barostat (ASE's
`NPTBerendsen`; with a `mask` of three flags its `Inhomogeneous_NPTBerendsen`), under any of the thermostat
settings. The scaling factor is computed inside the integrator launch from the forces of the unscaled
positions, one force evaluation per step (what ASE does when forces are handed to its `step`). `GPa` and `bar`
are the same numbers as `ase.units.GPa` and `ase.units.bar`.

The isothermal-isobaric ensemble: with `pressure` and `pdamp` (names as ASE's `IsotropicMTKNPT`: `pdamp`, `pchain`,
`ploop`; LAMMPS `fix npt`) the cells follow a Martyna-Tobias-Klein barostat instead, coupled to the Nose-Hoover chain
(`temperature_K`, `tdamp`, which it needs) and to a chain of `pchain` thermostats of its own. Where the Berendsen
barostat relaxes a cell towards a pressure and suppresses its fluctuations, this one samples the ensemble: thermal
expansion, densities, coexistence and, from <dV^2>, the compressibility (`isothermal_compressibility`) come out
right. Without a `mask` one strain rate follows the mean driving force; with one, every free axis has its own rate
and a masked axis keeps its length exactly. State per frame: the strain rates omega_c and the chain (xi_k, vxi_k);
masses W_c = (g + 3) kT pdamp^2 / 3, Q'_1 = d_b kT pdamp^2, Q'_k = kT pdamp^2 with d_b = 1 (isotropic) or the
number of free axes. A step is: the two chains' half-updates, a half-kick of omega by
G_c = [sum m v_c^2 - W_cc - P0 V + 2 ekin / g] / W_c, the velocities scaled by exp(-(dt/2) (omega_c + tr omega / g))
and kicked, x_c <- exp(omega_c dt) x_c + dt exp(omega_c dt / 2) v_c with the cell's column scaled likewise, the
evaluation, and the same in reverse; it is written out in include/tensoralloy_amd.h. The conserved quantity gains
    ebaro = P0 V + sum_c W_c omega_c^2 / 2 + sum_k Q'_k vxi_k^2 / 2 + d_b kT xi_1 + kT sum_{k>=2} xi_k
which `get_conserved_energy()` includes. To restart, keep `Engine.md_mtk_state()` and `Engine.md_cells()` beside the
state and the chain, and hand them to `set_frames` / `md_init`, `md_set_chain` and `Engine.md_set_mtk_state`.

Time correlations: with `n_lags` (and `sample_every`) the loop itself keeps the last `n_lags` sampled
whole-step states in a ring on the device and, at every sample, adds the velocity autocorrelation
<v(t0 + k) . v(t0)> and the mean-square displacement <|x(t0 + k) - x(t0)|^2> at all lags k, per frame and per
element, over every time origin t0 it has seen (`Engine.md_set_sampling`; `DeviceMD.get_vacf`, `get_msd`,
`get_samples`). The run is not cut and no per-atom data cross the bus. Positions are the unwrapped ones the
integrator holds, and no centre-of-mass correction is made: velocities without net momentum keep the centre of
mass at rest under NVE and the Nose-Hoover chain; under Langevin its diffusion is part of the result. Sampling
under the barostat is refused. `vdos` turns a VACF into a vibrational density of states, `diffusion_coefficient`
fits the slope of an MSD (Einstein) and `green_kubo_diffusion` integrates a VACF (Green-Kubo).

Pair distributions: with `rdf_bins` (and `rdf_rmax`, `rdf_every`) the loop counts, at every sampled step, the
pairs of its resident neighbour list below `rdf_rmax` into integer histograms per frame and pair of elements,
on the device (`Engine.md_set_rdf`; `DeviceMD.get_rdf`). The counts are exact integers and do not depend on how
a run is cut. `rdf` normalises counts to g_ab(r), `coordination_number` integrates g_ab to a neighbour count.
Independent of `n_lags`; refused under the barostat, where there is no single volume to normalise with.

Bond-angle distributions: with `adf_bins` (and `adf_rbond`, `adf_every`) the loop counts, at every sampled step
and for every centre, the angle j-i-k between every two of its neighbours below the bond cutoff into integer
histograms over [0, pi] per frame, species of the centre and pair of species of the two neighbours, on the device
(`Engine.md_set_adf`; `DeviceMD.get_adf`): the three-body companion of g(r), which tells a liquid from a glass
from a defective crystal. The counts are exact integers and do not depend on how a run is cut. `adf` normalises
them to a probability density per degree. No volume enters, so this runs under the barostat as well, and
independently of `n_lags` and `rdf_bins`.

Bond-orientational order: with `order_bins` (and `order_degrees`, `order_rbond`, `order_every`, `order_solid`) the
loop evaluates, at every sampled step and for every atom, the Steinhardt parameters q_l of its bonds, their
neighbour average qbar_l and the number of solid bonds n_conn, on the device (`Engine.md_set_order`;
`DeviceMD.get_order`, `DeviceMD.get_order_atoms`): the per-atom answer to "which atoms are crystalline, and in
which lattice". Histograms over the samples are exact integers; the per-atom values are those of the newest sample.
`order_distribution` normalises a histogram of q, `solid_fraction` and `classify_solid` apply the usual test
n_conn >= n_min. Runs under the barostat and independently of the other observables.

Clusters: with `cluster_bins` (and `cluster_rlink`, `cluster_nmin`, `cluster_species`, `cluster_series`,
`cluster_every`) the loop finds, at every sampled step, the connected components of the selected atoms on the device
(`Engine.md_set_clusters`; `DeviceMD.get_clusters`): the size of the largest crystalline nucleus as a function of
time (`cluster_nmin` > 0, on top of `order_bins`) or the clusters of chosen elements in a solid solution
(`cluster_species`). Every result is an exact integer and a function of the state alone. `largest_cluster` reads the
time series, `cluster_size_distribution` the histogram, `clusters_from_labels` the per-atom labels. Runs under the
barostat and every thermostat.

Common neighbour analysis: with `cna` ("adaptive" or "fixed"; and `cna_rcut`, `cna_rmax`, `cna_series`, `cna_every`) the
loop gives, at every sampled step, every atom its lattice type on the device (`Engine.md_set_cna`;
`DeviceMD.get_structure_types`, `DeviceMD.get_structure_counts`): 0 other, 1 fcc, 2 hcp, 3 bcc, 4 ico (`CNA_NAMES`), as
OVITO's common neighbour analysis and LAMMPS `compute cna/atom` do. Every type is an exact integer and a function of
the state alone. `structure_fractions` normalises the counts. Runs under the barostat and every thermostat.

Structure factors: with `sq_miller` (and `sq_lags`, `sq_every`, `sq_currents`) the loop sums, at every sampled step,
the density amplitudes rho_a(q) = sum_i exp(i q . x_i) of every element over ALL atoms of a frame, at the wave
vectors q = 2 pi h^-1 n of the integer triples given (`q_points` lists those below a |q|), keeps the last `sq_lags`
rows on the device and correlates them at every lag (`Engine.md_set_sq`; `DeviceMD.get_structure_factor`,
`get_intermediate_scattering`): the static structure factor S(q) that diffraction measures, which a Fourier
transform of a g(r) that stops at the model's cutoff cannot give, the intermediate scattering function F(q, t) and,
with `sq_currents`, the longitudinal and transverse current correlations C_L(q, t), C_T(q, t), from which phonon
dispersions, sound velocities and damping are read. `intermediate_scattering` and `structure_factor` normalise the
sums (Ashcroft-Langreth partials), `transverse_current` splits the current trace, `dynamic_structure_factor`
transforms to S(q, nu), `shell_average` bins over |q|. Everything is fp64 with a fixed order of addition: a run cut
into calls gives the same bits. Refused under the barostat.

Heat current and pressure tensor: with `flux_lags` (and `flux_every`) the loop makes, at every sampled step, the heat
current J = J_conv + J_pot and the pressure tensor Pi = K - W = P V of every frame from the model's per-atom energies
and per-pair gradients, which exist only on the device and only for one evaluation, keeps the last `flux_lags` rows
and correlates them at every lag (`Engine.md_set_flux`; `DeviceMD.get_heat_current_acf`, `get_pressure_acf`):
the two Green-Kubo observables, the lattice thermal conductivity (`green_kubo_thermal_conductivity`) and the shear
viscosity (`green_kubo_viscosity`), that a dumped trajectory cannot give. `heat_current_acf` and `pressure_acf`
normalise the sums. No centre-of-mass correction is made and no partial-enthalpy correction for mixtures: in a
mixture J contains the interdiffusion part. Everything is fp64 with a fixed order of addition. While it is on, the
evaluations of a run take the builds that leave the centre-side pair gradients, so the trajectory agrees with an
unsampled one to rounding, not bit for bit. Refused under the barostat.
"""
from __future__ import annotations

import numpy as np

fs = 0.09822694788464063      # one femtosecond in Angstrom sqrt(amu / eV)
kB = 8.617330337217213e-05    # eV / K
GPa = 1.0 / 160.21766208      # eV / Angstrom^3
bar = 1.0e-4 * GPa

__all__ = ["fs", "kB", "GPa", "bar", "maxwell_boltzmann", "DeviceMD", "vdos", "diffusion_coefficient",
           "green_kubo_diffusion", "rdf", "coordination_number", "adf", "order_distribution", "solid_fraction",
           "classify_solid", "largest_cluster", "cluster_size_distribution", "clusters_from_labels", "CNA_NAMES", "structure_fractions", "q_points", "intermediate_scattering", "structure_factor", "transverse_current",
           "dynamic_structure_factor", "shell_average", "heat_current_acf", "pressure_acf",
           "green_kubo_thermal_conductivity", "green_kubo_viscosity"]


def maxwell_boltzmann(masses, kT, rng, zero_momentum=True):
    """Velocities [n, 3] drawn from the Maxwell-Boltzmann distribution at `kT` (eV) for `masses` (amu):
    every component is normal with variance kT / m. `rng` is a `numpy.random.RandomState` (or anything
    with `standard_normal`). `zero_momentum` subtracts the centre-of-mass velocity afterwards."""
    m = np.asarray(masses, dtype=np.float64).ravel()
    if not np.all(np.isfinite(m)) or np.any(m <= 0.0):
        raise ValueError("maxwell_boltzmann: masses must be finite and > 0")
    if not (kT >= 0.0):
        raise ValueError("maxwell_boltzmann: kT must be >= 0")
    v = rng.standard_normal((len(m), 3)) * np.sqrt(kT / m)[:, None]
    if zero_momentum and len(m):
        v -= (m[:, None] * v).sum(axis=0) / m.sum()
    return v


def isothermal_compressibility(volumes, temperature_K):
    """<dV^2> / (kB T <V>) in A^3 / eV from the volumes [n] of one frame along a run in the isothermal-isobaric
    ensemble (`pdamp`; the Berendsen barostat suppresses these fluctuations and gives no such number)."""
    V = np.asarray(volumes, dtype=np.float64)
    if V.ndim != 1 or len(V) < 2:
        raise ValueError("isothermal_compressibility: the volumes [n] of one frame, n >= 2, are needed")
    if not (np.isfinite(temperature_K) and temperature_K > 0.0):
        raise ValueError("isothermal_compressibility: temperature_K must be finite and > 0")
    mean = V.mean()
    return float(((V - mean) ** 2).mean() / (kB * temperature_K * mean))


def _trapezoid(y, dx):
    y = np.asarray(y, dtype=np.float64)
    return dx * (y.sum(axis=-1) - 0.5 * (y[..., 0] + y[..., -1]))


def vdos(vacf, dt_sample, window="hann"):
    """Vibrational density of states from a velocity autocorrelation `vacf` [..., L] (L >= 2) sampled every
    `dt_sample` (ASE time units): returns (nu, g) with nu [L] in THz, nu_j = j / (2 (L - 1) dt_sample), up to the
    Nyquist frequency, and g [..., L] the one-sided cosine transform of c_k = vacf_k / vacf_0,
        g(nu_j) ~ w_0 c_0 / 2 + sum_{k=1}^{L-2} w_k c_k cos(pi j k / (L - 1)) + w_{L-1} c_{L-1} cos(pi j) / 2
    (the trapezoid rule in time). `window`: "hann", w_k = (1 + cos(pi k / (L - 1))) / 2, which takes the
    truncated tail to zero, or None, w_k = 1. g is scaled so that its integral over nu by the trapezoid rule on
    this grid is 1 (per THz)."""
    c = np.asarray(vacf, dtype=np.float64)
    w, k = _cosine_weights("vdos", "vacf", c, dt_sample, window)
    L = len(k)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = c / c[..., :1]
    g = (c * w) @ np.cos(np.pi * np.outer(k, k) / (L - 1))
    nu = k / (2.0 * (L - 1) * (dt_sample / fs) * 1.0e-3)   # 1 / ps
    with np.errstate(divide="ignore", invalid="ignore"):
        g = g / _trapezoid(g, nu[1] - nu[0])[..., None]
    return nu, g


def _cosine_weights(who, what, c, dt_sample, window):
    """The checks of a one-sided cosine transform of `c` [..., L] and its weights: the window times the trapezoid
    rule's halves at both ends, and the lags arange(L)."""
    L = c.shape[-1] if c.ndim else 0
    if L < 2:
        raise ValueError(f"{who}: a {what} with at least two lags along the last axis is needed")
    if not (np.isfinite(dt_sample) and dt_sample > 0.0):
        raise ValueError(f"{who}: dt_sample must be a finite time > 0")
    k = np.arange(L)
    if window == "hann":
        w = 0.5 * (1.0 + np.cos(np.pi * k / (L - 1)))
    elif window is None:
        w = np.ones(L)
    else:
        raise ValueError(f"{who}: window must be 'hann' or None")
    w[0] *= 0.5
    w[-1] *= 0.5
    return w, k


def diffusion_coefficient(msd, dt_sample, fit=None):
    """Einstein relation: the least-squares slope (with a free intercept) of `msd` [..., L] against the lag times
    k dt_sample over the lags `fit` = (lo, hi), i.e. lo .. hi - 1, divided by 6: D in A^2 per ASE time unit
    (multiply by `fs` for A^2 / fs). 0 <= lo < hi <= L is required, and two lags at least, since a slope needs
    two points; default: the upper half of the lags, (L // 2, L)."""
    y = np.asarray(msd, dtype=np.float64)
    L = y.shape[-1] if y.ndim else 0
    if not (np.isfinite(dt_sample) and dt_sample > 0.0):
        raise ValueError("diffusion_coefficient: dt_sample must be a finite time > 0")
    if fit is None:
        fit = (L // 2, L)
    if np.shape(fit) != (2,) or int(fit[0]) != fit[0] or int(fit[1]) != fit[1]:
        raise ValueError("diffusion_coefficient: fit must be two integers (lo, hi)")
    lo, hi = int(fit[0]), int(fit[1])
    if not (0 <= lo < hi <= L):
        raise ValueError(f"diffusion_coefficient: fit = (lo, hi) needs 0 <= lo < hi <= {L} lags")
    if hi - lo < 2:
        raise ValueError("diffusion_coefficient: fit must span at least two lags")
    t = np.arange(lo, hi) * float(dt_sample)
    tc = t - t.mean()
    yy = y[..., lo:hi]
    slope = ((yy - yy.mean(axis=-1, keepdims=True)) * tc).sum(axis=-1) / (tc * tc).sum()
    return slope / 6.0


def green_kubo_diffusion(vacf, dt_sample):
    """Green-Kubo relation: the integral of `vacf` [..., L] over the lag times by the trapezoid rule, divided by
    3: D in A^2 per ASE time unit. The integral is cut at the last lag; choose n_lags so that the vacf has
    decayed there."""
    c = np.asarray(vacf, dtype=np.float64)
    if c.ndim == 0 or c.shape[-1] < 1:
        raise ValueError("green_kubo_diffusion: a vacf with lags along the last axis is needed")
    if not (np.isfinite(dt_sample) and dt_sample > 0.0):
        raise ValueError("green_kubo_diffusion: dt_sample must be a finite time > 0")
    return _trapezoid(c, float(dt_sample)) / 3.0


def _shell_volumes(n_bins, dr):
    k = np.arange(n_bins, dtype=np.float64)
    return (4.0 * np.pi / 3.0) * ((k + 1.0) ** 3 - k ** 3) * dr ** 3


def rdf(counts, n_samples, n_by_element, volume, r_max, pbc=None):
    """Partial pair distribution functions from the integer pair counts of the device loop (`Engine.md_rdf`):
    `counts` [..., E, E, B] directed pairs of a centre of element a and a neighbour of element b in bin k
    (k = floor(r / dr), dr = `r_max` / B), summed over `n_samples` samples; `n_by_element` [..., E] atoms per
    element; `volume` [...] of the cell. Returns (r, g): the bin centres r_k = (k + 1/2) dr [B] and
        g_ab(r_k) = C[a][b][k] V / (n_samples N_a N_b (4 pi / 3) ((k + 1)^3 - k^3) dr^3)
    [..., E, E, B]. The normalisation uses N_a N_b, not N_a (N_b - delta_ab): g_aa of an ideal gas is
    (N_a - 1) / N_a, not 1, which matters for small cells only. Rows with N_a N_b == 0 (an element the frame
    does not hold) and everything with `n_samples` == 0 are NaN. g is defined against the mean density of a
    periodic cell: a `volume` that is not finite and > 0, or a `pbc` ([..., 3], optional) that is not periodic
    in all three directions, raises ValueError; the counts of such frames are still meaningful."""
    c = np.asarray(counts)
    if c.ndim < 3 or c.shape[-2] != c.shape[-3] or c.shape[-1] < 1:
        raise ValueError("rdf: counts must be [..., n_elements, n_elements, n_bins]")
    B = c.shape[-1]
    if not (np.isfinite(r_max) and r_max > 0.0):
        raise ValueError("rdf: r_max must be a finite distance > 0")
    if int(n_samples) != n_samples or n_samples < 0:
        raise ValueError("rdf: n_samples must be an integer >= 0")
    if pbc is not None and not np.all(pbc):
        raise ValueError("rdf: g(r) needs a frame periodic in all three directions (the counts need not)")
    V = np.asarray(volume, dtype=np.float64)
    if not np.all(np.isfinite(V) & (V > 0.0)):
        raise ValueError("rdf: volume must be finite and > 0")
    n = np.asarray(n_by_element, dtype=np.float64)
    if n.shape != c.shape[:-2]:
        raise ValueError("rdf: n_by_element must be [..., n_elements], matching counts")
    if V.shape not in ((), c.shape[:-3]):
        raise ValueError("rdf: one volume, or one per frame of counts, is needed")
    dr = float(r_max) / B
    r = (np.arange(B) + 0.5) * dr
    den = float(n_samples) * n[..., :, None] * n[..., None, :]
    den = den[..., None] * _shell_volumes(B, dr)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(den > 0.0, c * V[..., None, None, None] / den, np.nan)
    return r, g


def coordination_number(g, r, density_b, r_cut):
    """Neighbours of element b around an atom of element a within `r_cut`: the running integral of
    4 pi r^2 rho_b g_ab(r), from `g` [..., B] on the bin centres `r` [B] of `rdf` (uniform bins from 0) and
    the number density `density_b` = N_b / V (a scalar, or an array that broadcasts against g without its
    last axis). It is evaluated from the shell volumes (4 pi / 3) ((k + 1)^3 - k^3) dr^3 that `rdf` divided by,
    over the bins whose centres lie below `r_cut`, so it returns the counts / (n_samples N_a) that went in,
    not a quadrature of them."""
    g = np.asarray(g, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    if r.ndim != 1 or len(r) < 1 or g.ndim < 1 or g.shape[-1] != len(r):
        raise ValueError("coordination_number: g [..., n_bins] on the bin centres r [n_bins] is needed")
    dr = 2.0 * float(r[0])
    if not (np.isfinite(dr) and dr > 0.0 and np.allclose(r, (np.arange(len(r)) + 0.5) * dr, rtol=1e-9, atol=0.0)):
        raise ValueError("coordination_number: r must be the centres (k + 1/2) dr of uniform bins from 0")
    if not np.isfinite(r_cut):
        raise ValueError("coordination_number: r_cut must be finite")
    inside = r < r_cut
    shells = np.where(inside, _shell_volumes(len(r), dr), 0.0)
    return np.asarray(density_b, dtype=np.float64) * (np.where(inside, g, 0.0) * shells).sum(axis=-1)


def adf(counts):
    """Bond-angle distributions from the integer triple counts of the device loop (`Engine.md_adf`): `counts`
    [..., E, P, B], triples of a centre of element a and two neighbours of the pair of elements p in bin k of B
    uniform bins over [0, 180] degrees. Returns (theta, p): the bin centres theta_k = (k + 1/2) 180 / B in
    degrees [B] and the probability density per degree [..., E, P, B]: every row [a][p] times the bin width
    180 / B sums to 1. A row without any triple is NaN."""
    c = np.asarray(counts)
    if c.ndim < 3 or c.shape[-1] < 1:
        raise ValueError("adf: counts must be [..., n_elements, n_pairs, n_bins]")
    B = c.shape[-1]
    width = 180.0 / B
    theta = (np.arange(B) + 0.5) * width
    total = c.sum(axis=-1, keepdims=True).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(total > 0.0, c / (total * width), np.nan)
    return theta, p


def order_distribution(hist):
    """Distributions of an order parameter from the integer counts of the device loop (`Engine.md_order`): `hist`
    [..., B] (`hist_q` or `hist_qbar`, [n_frames, n_elements, n_degrees, B]), atoms in bin k of B uniform bins over
    [0, 1]. Returns (q, p): the bin centres q_k = (k + 1/2) / B [B] and the probability density per unit q
    [..., B]: every row times the bin width 1 / B sums to 1. A row without atoms is NaN."""
    c = np.asarray(hist)
    if c.ndim < 1 or c.shape[-1] < 1:
        raise ValueError("order_distribution: hist must be [..., n_bins]")
    B = c.shape[-1]
    q = (np.arange(B) + 0.5) / B
    total = c.sum(axis=-1, keepdims=True).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(total > 0.0, c * B / total, np.nan)
    return q, p


def solid_fraction(hist_conn, n_min):
    """Share of the sampled atoms with at least `n_min` solid bonds, from the counts `hist_conn` [..., C] of the
    device loop (`Engine.md_order`; bin k = atoms with min(n_conn, C - 1) == k, so 0 <= `n_min` <= C - 1):
    [...], per frame and element for the engine's [n_frames, n_elements, 32]. NaN where no atom was sampled."""
    c = np.asarray(hist_conn)
    n_min = int(n_min)
    if c.ndim < 1 or c.shape[-1] < 1:
        raise ValueError("solid_fraction: hist_conn must be [..., n_conn_bins]")
    if not 0 <= n_min <= c.shape[-1] - 1:
        raise ValueError(f"solid_fraction: n_min must be 0 .. {c.shape[-1] - 1} (the last bin holds everything above)")
    total = c.sum(axis=-1).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(total > 0.0, c[..., n_min:].sum(axis=-1) / total, np.nan)


def classify_solid(n_conn, n_min):
    """The test of `solid_fraction` atom by atom: a bool array, True where `n_conn` (`Engine.md_order_atoms`)
    is at least `n_min`."""
    return np.asarray(n_conn) >= int(n_min)


def largest_cluster(series, steps, dt):
    """(t, size): the times `steps` dt [rows] and the size of the largest cluster [rows, n_frames] from the time
    series of the device loop (`Engine.md_clusters`: `series` int [rows, n_frames, 4], `steps` [rows])."""
    ser, st = np.asarray(series), np.asarray(steps)
    if ser.ndim != 3 or ser.shape[-1] != 4 or st.shape != ser.shape[:1]:
        raise ValueError("largest_cluster: series must be [rows, n_frames, 4] and steps [rows]")
    return st.astype(np.float64) * float(dt), ser[:, :, 2].copy()


def cluster_size_distribution(hist, n_samples=None):
    """(sizes, mean): the sizes 1 .. B [B] and the mean number of clusters of each size per sample and frame [B]
    from the counts `hist` [..., B] of the device loop (`Engine.md_clusters`; the last bin holds every size >= B),
    summed over the leading axes (frames). `n_samples`: the samples the counts were summed over (default 1)."""
    c = np.asarray(hist)
    if c.ndim < 1 or c.shape[-1] < 1:
        raise ValueError("cluster_size_distribution: hist must be [..., n_bins]")
    n = 1 if n_samples is None else int(n_samples)
    if n < 1:
        raise ValueError("cluster_size_distribution: n_samples must be >= 1")
    frames = int(np.prod(c.shape[:-1])) if c.ndim > 1 else 1
    total = c.reshape(-1, c.shape[-1]).sum(axis=0).astype(np.float64)
    return np.arange(1, c.shape[-1] + 1), total / float(n * max(frames, 1))


def clusters_from_labels(label):
    """(sizes, members): the cluster sizes, largest first (among equals the smaller label first), and for each the
    sorted indices of its atoms, from the per-atom labels of the device loop (`Engine.md_cluster_atoms`; -1 marks an
    atom that is not selected)."""
    lab = np.asarray(label)
    if lab.ndim != 1:
        raise ValueError("clusters_from_labels: label must be [n_atoms]")
    groups = {}
    for i, l in enumerate(lab.tolist()):
        if l >= 0:
            groups.setdefault(l, []).append(i)
    keys = sorted(groups, key=lambda l: (-len(groups[l]), l))
    return np.array([len(groups[l]) for l in keys], dtype=np.int64), [np.array(groups[l], dtype=np.int64) for l in keys]


CNA_NAMES = ("other", "fcc", "hcp", "bcc", "ico")   # the structure types of the device loop, OVITO's numbering


def structure_fractions(counts):
    """The fractions of the structure types from the counts `counts` [..., 5] or the series of the device loop
    (`Engine.md_cna`): the last axis divided by its sum, NaN for a row without atoms."""
    c = np.asarray(counts)
    if c.ndim < 1 or c.shape[-1] != len(CNA_NAMES):
        raise ValueError(f"structure_fractions: counts must be [..., {len(CNA_NAMES)}]")
    c = c.astype(np.float64)
    total = c.sum(axis=-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(total > 0.0, c / total, np.nan)


def q_points(cell, q_max, max_index=64):
    """The integer triples n [Q, 3] (int32) of all wave vectors q = 2 pi h^-1 n of `cell` (h [3, 3], rows are lattice
    vectors) with 0 < |q| <= `q_max` (1 / A), one of each pair +-n (the first non-zero index is positive), ordered by
    |q|. Since n_c = q . a_c / (2 pi), |n_c| <= q_max |a_c| / (2 pi); triples with an index beyond `max_index` (at
    most 64, what the device takes) are left out."""
    h = np.asarray(cell, dtype=np.float64)
    if h.shape != (3, 3) or not np.all(np.isfinite(h)) or not abs(np.linalg.det(h)) > 0.0:
        raise ValueError("q_points: cell must be a finite, non-singular [3, 3] matrix")
    if not (np.isfinite(q_max) and q_max > 0.0):
        raise ValueError("q_points: q_max must be finite and > 0")
    if int(max_index) != max_index or not 1 <= max_index <= 64:
        raise ValueError("q_points: max_index must be an integer 1 .. 64")
    top = np.minimum(np.floor(q_max * np.linalg.norm(h, axis=1) / (2.0 * np.pi) * (1.0 + 1e-12)).astype(int), int(max_index))
    n = np.stack(np.meshgrid(*[np.arange(-t, t + 1) for t in top], indexing="ij"), axis=-1).reshape(-1, 3)
    first = np.where(n[:, 0] != 0, n[:, 0], np.where(n[:, 1] != 0, n[:, 1], n[:, 2]))
    n = n[first > 0]
    q = np.linalg.norm(2.0 * np.pi * n @ np.linalg.inv(h).T, axis=1)
    keep = q <= q_max
    n, q = n[keep], q[keep]
    return np.ascontiguousarray(n[np.argsort(q, kind="stable")], dtype=np.int32)


def intermediate_scattering(acc, n_samples, n_by_element):
    """Ashcroft-Langreth partial intermediate scattering functions from the sums of the device loop
    (`Engine.md_sq`): `acc` [..., E, E, L, Q] (`a_rho`; `a_l` or `transverse_current(a_j, a_l)` give the current
    correlations C_L, C_T in the same way), `n_by_element` [..., E] atoms per element. Returns
        F_ab(q, t_k) = A[a][b][k][q] / ((n_samples - k) sqrt(N_a N_b))
    [..., E, E, L, Q]: NaN where an element is absent and at lags without a time origin (k >= n_samples)."""
    a = np.asarray(acc, dtype=np.float64)
    if a.ndim < 4 or a.shape[-3] != a.shape[-4]:
        raise ValueError("intermediate_scattering: acc must be [..., n_elements, n_elements, n_lags, n_q]")
    if int(n_samples) != n_samples or n_samples < 0:
        raise ValueError("intermediate_scattering: n_samples must be an integer >= 0")
    n = np.asarray(n_by_element, dtype=np.float64)
    if n.shape != a.shape[:-3]:
        raise ValueError("intermediate_scattering: n_by_element must be [..., n_elements], matching acc")
    origins = np.maximum(0, int(n_samples) - np.arange(a.shape[-2])).astype(np.float64)
    den = np.sqrt(n[..., :, None] * n[..., None, :])[..., None, None] * origins[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0.0, a / den, np.nan)


def structure_factor(a_rho, n_samples, n_by_element):
    """(S_ab, S): the partial static structure factors S_ab(q) = F_ab(q, 0) [..., E, E, Q] of
    `intermediate_scattering` and the total S(q) = sum_ab sqrt(c_a c_b) S_ab(q) [..., Q] with c_a = N_a / N (for one
    element S = S_aa; for a mixture the structure factor of equal scattering lengths, |sum_i exp(i q . x_i)|^2 / N).
    An absent element has NaN partials and no share in S."""
    f = intermediate_scattering(a_rho, n_samples, n_by_element)[..., 0, :]
    n = np.asarray(n_by_element, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = n / n.sum(axis=-1, keepdims=True)
    w = np.sqrt(c[..., :, None] * c[..., None, :])[..., None]
    total = np.where(w > 0.0, w * f, 0.0).sum(axis=(-3, -2))
    sampled = (n.sum(axis=-1)[..., None] > 0.0) & (int(n_samples) > 0)
    return f, np.where(sampled, total, np.nan)


def transverse_current(a_j, a_l):
    """(A_J - A_L) / 2: the current correlation per transverse direction, from the trace of the current tensor and its
    longitudinal part (`Engine.md_sq`: `a_j`, `a_l`). Normalise it with `intermediate_scattering`."""
    return 0.5 * (np.asarray(a_j, dtype=np.float64) - np.asarray(a_l, dtype=np.float64))


def dynamic_structure_factor(F, dt_sample, window="hann"):
    """Dynamic structure factor from an intermediate scattering function (or spectra of C_L, C_T from the current
    correlations): `F` [..., L, Q] (L >= 2 lags along the last axis but one, as `intermediate_scattering` returns
    it) sampled every `dt_sample` (ASE time units). Returns (nu, S): nu [L] in THz on the grid of `vdos`,
    nu_j = j / (2 (L - 1) dt_sample), and
        S(q, nu_j) = 2 dt (w_0 F_0 / 2 + sum_{k=1}^{L-2} w_k F_k cos(pi j k / (L - 1)) + w_{L-1} F_{L-1} cos(pi j) / 2)
    [..., L, Q] with dt in ps: the cosine transform of `vdos` (the trapezoid rule in time, `window` "hann" or None)
    without its normalisations, so that the integral of S over nu from -inf to inf is F(q, 0)."""
    f = np.moveaxis(np.asarray(F, dtype=np.float64), -2, -1) if np.ndim(F) >= 2 else np.asarray(F, dtype=np.float64)
    if f.ndim < 2:
        raise ValueError("dynamic_structure_factor: F must be [..., n_lags, n_q]")
    w, k = _cosine_weights("dynamic_structure_factor", "F", f, dt_sample, window)
    L = len(k)
    s = (f * w) @ np.cos(np.pi * np.outer(k, k) / (L - 1))
    dt_ps = (dt_sample / fs) * 1.0e-3
    nu = k / (2.0 * (L - 1) * dt_ps)
    return nu, np.moveaxis(2.0 * dt_ps * s, -1, -2)


def shell_average(values, q_norm, n_bins):
    """Average over shells of |q|: `values` [..., Q] at the wave vectors of length `q_norm` [Q], in `n_bins` uniform
    bins over (0, max |q|]. Returns (q, mean, counts): the mean |q| of every shell [n_bins] (NaN for an empty one),
    the mean of the values [..., n_bins] (NaN likewise) and the number of vectors per shell."""
    v = np.asarray(values, dtype=np.float64)
    qn = np.asarray(q_norm, dtype=np.float64)
    if qn.ndim != 1 or v.ndim < 1 or v.shape[-1] != len(qn) or len(qn) < 1:
        raise ValueError("shell_average: values [..., n_q] and q_norm [n_q] are needed")
    if int(n_bins) != n_bins or n_bins < 1:
        raise ValueError("shell_average: n_bins must be an integer >= 1")
    if not (np.all(np.isfinite(qn)) and np.all(qn >= 0.0) and qn.max() > 0.0):
        raise ValueError("shell_average: q_norm must be finite, >= 0 and not all 0")
    n_bins = int(n_bins)
    k = np.minimum(np.ceil(qn / qn.max() * n_bins).astype(int) - 1, n_bins - 1)   # (edges belong to the shell below)
    inside = k >= 0   # (q = 0 belongs to no shell)
    onehot = (k[inside, None] == np.arange(n_bins)[None, :]).astype(np.float64)
    counts = onehot.sum(axis=0).astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(counts > 0, qn[inside] @ onehot / counts, np.nan)
        mean = np.where(counts > 0, v[..., inside] @ onehot / counts, np.nan)
    return q, mean, counts


def _origins(who, acc, n_samples):
    a = np.asarray(acc, dtype=np.float64)
    if a.ndim < 2:
        raise ValueError(f"{who}: the sums must be [..., n_lags, components]")
    n = int(n_samples) - np.arange(a.shape[-2])
    return a, np.where(n > 0, n, 1).astype(np.float64), n > 0


def heat_current_acf(a_heat, n_samples):
    """<J_a(t_k) J_a(0)> [..., 3, n_lags] from the sums `a_heat` [..., n_lags, 3] of `Engine.md_flux`: lag k is
    divided by its n_samples - k time origins (NaN where there is none). The mean of J is not subtracted: it
    vanishes in equilibrium. Units: (eV A / ASE time)^2."""
    a, n, ok = _origins("heat_current_acf", a_heat, n_samples)
    return np.swapaxes(np.where(ok[:, None], a / n[:, None], np.nan), -1, -2)


def pressure_acf(a_press, sums, n_samples):
    """<dPi_ab(t_k) dPi_ab(0)> [..., 6, n_lags] (xx yy zz yz xz xy) from the sums `a_press` [..., n_lags, 6] and
    `sums` [..., 18] of `Engine.md_flux`: lag k is divided by its n_samples - k time origins (NaN where there is
    none), and the SQUARED MEAN of Pi_ab = K_ab - W_ab over all samples, taken from `sums`, is subtracted, so that the
    diagonal components fluctuate about the mean pressure (the shear components have mean zero in a liquid and keep
    a residual stress in a solid). Units: eV^2."""
    a, n, ok = _origins("pressure_acf", a_press, n_samples)
    r = np.asarray(sums, dtype=np.float64)
    if r.shape[-1] != 18 or r.shape[:-1] != a.shape[:-2] or a.shape[-1] != 6:
        raise ValueError("pressure_acf: a_press [..., n_lags, 6] and sums [..., 18] are needed")
    mean = (r[..., 6:12] - r[..., 12:18]) / max(int(n_samples), 1)
    return np.swapaxes(np.where(ok[:, None], a / n[:, None] - mean[..., None, :] ** 2, np.nan), -1, -2)


_EV_IN_J = 1.0e-21 / GPa      # 1 eV / A^3 = (1 / GPa) GPa
_TIME_IN_S = 1.0e-15 / fs     # one ASE time unit in seconds


def _running_integral(y, dx):
    y = np.asarray(y, dtype=np.float64)
    return np.stack([_trapezoid(y[..., :k + 1], dx) for k in range(y.shape[-1])], axis=-1)


def _green_kubo_arguments(who, acf, volume, temperature_K, dt_sample):
    c = np.asarray(acf, dtype=np.float64)
    if c.ndim < 2 or c.shape[-1] < 1:
        raise ValueError(f"{who}: acf must be [..., components, n_lags]")
    v = np.asarray(volume, dtype=np.float64)
    if not (np.all(np.isfinite(v)) and np.all(v > 0.0)):
        raise ValueError(f"{who}: volume must be finite and > 0")
    if not (np.isfinite(temperature_K) and temperature_K > 0.0):
        raise ValueError(f"{who}: temperature_K must be finite and > 0")
    if not (np.isfinite(dt_sample) and dt_sample > 0.0):
        raise ValueError(f"{who}: dt_sample must be a finite time > 0")
    return c, v[..., None, None] if v.ndim else v


def green_kubo_thermal_conductivity(acf, volume, temperature_K, dt_sample):
    """Running Green-Kubo integral kappa_a(t_k) = 1 / (V kB T^2) int_0^{t_k} <J_a(t) J_a(0)> dt [..., 3, n_lags], in
    W / (m K), of a heat-current autocorrelation `acf` [..., 3, n_lags] (`heat_current_acf`) sampled every `dt_sample`
    (ASE time units) in the volume `volume` (A^3; a scalar or one per leading index) at `temperature_K`
    (trapezoidal rule). Read the plateau; the mean of the three axes is the conductivity of an isotropic system."""
    c, v = _green_kubo_arguments("green_kubo_thermal_conductivity", acf, volume, temperature_K, dt_sample)
    si = _EV_IN_J / (1.0e-10 * _TIME_IN_S)   # eV / (A ASE-time K) in W / (m K)
    return _running_integral(c, float(dt_sample)) / (v * kB * float(temperature_K) ** 2) * si


def green_kubo_viscosity(acf, volume, temperature_K, dt_sample):
    """Running Green-Kubo integral eta_ab(t_k) = 1 / (V kB T) int_0^{t_k} <Pi_ab(t) Pi_ab(0)> dt over the shear
    components yz, xz, xy [..., 3, n_lags], in mPa s, of a pressure-tensor autocorrelation `acf` [..., 6, n_lags]
    (`pressure_acf`) sampled every `dt_sample` (ASE time units) in the volume `volume` (A^3) at `temperature_K`
    (trapezoidal rule). Read the plateau; the mean of the three is the shear viscosity of an isotropic liquid."""
    c, v = _green_kubo_arguments("green_kubo_viscosity", acf, volume, temperature_K, dt_sample)
    if c.shape[-2] != 6:
        raise ValueError("green_kubo_viscosity: acf must be [..., 6, n_lags]")
    si = _EV_IN_J / 1.0e-30 * _TIME_IN_S * 1.0e3   # eV ASE-time / A^3 in mPa s
    return _running_integral(c[..., 3:6, :], float(dt_sample)) / (v * kB * float(temperature_K)) * si


class DeviceMD:
    """
    NVE (velocity Verlet), Berendsen NVT, Langevin NVT or Nose-Hoover chain NVT dynamics of one structure or of a batch of
    independent structures, integrated on the GPU.

    engine_or_calculator : an `Engine`, or a `TensorAlloyCalculator` whose engine and skin are used (its
                           cached results are invalidated by every run)
    atoms_or_list        : one `Atoms` or a list of them (they become the resident batch); velocities are
                           taken from `atoms.get_velocities()` where the object has them, else 0
    timestep             : in ASE time units (e.g. `1.0 * fs`)
    temperature_K, taut  : both given: Berendsen thermostat with that target and time constant
    temperature_K, friction : both given: Langevin thermostat with that bath temperature (>= 0; 0 is damped
                           dynamics) and friction (1 / ASE time unit, e.g. `0.01 / fs`)
    temperature_K, tdamp : both given: Nose-Hoover chain thermostat with that target (> 0) and time constant
                           (> 0, e.g. `20 * fs`); excludes `taut` and `friction`
    tchain, tloop        : thermostats per chain (1 .. 8) and loops per half-update (1 .. 16)
    dof_removed          : degrees of freedom taken off 3 n of every frame in the chain's g (3 for velocities
                           without centre-of-mass motion)
    seed                 : of the Langevin noise, 0 .. 2^64 - 1; the same seed gives the same trajectory
    pressure, taup, compressibility : all three given: Berendsen barostat with that target (eV / A^3, e.g.
                           `1.0 * GPa`), time constant (> 0) and compressibility (A^3 / eV, >= 0), with any
                           thermostat setting; every frame must be periodic along all three axes
    mask                 : None = isotropic; three flags (x, y, z) = each free axis follows its own pressure
    pressure, pdamp      : both given, with `temperature_K` and `tdamp`: Martyna-Tobias-Klein barostat with that
                           target and time constant (> 0, e.g. `1000 * fs`); excludes `taup` and `compressibility`;
                           `mask` as above; every frame must be periodic along all three axes
    pchain, ploop        : thermostats of the barostat's chain (1 .. 8) and loops per half-update (1 .. 16)
    n_lags, sample_every : `n_lags` given (1 .. 4096): the loop samples every `sample_every`-th step (the state at
                           construction is the first sample) and accumulates the velocity autocorrelation and
                           the mean-square displacement at `n_lags` lags on the device (`get_vacf`, `get_msd`,
                           `get_samples`); excludes the barostat. The ring takes 2 x n_lags x n_atoms x 24 bytes
    rdf_bins, rdf_rmax, rdf_every : `rdf_bins` given (1 .. 4096): the loop counts the pairs below `rdf_rmax`
                           (default and largest value: the model's cutoff) of every `rdf_every`-th step (the
                           state at construction is the first sample) into `rdf_bins` bins per pair of elements
                           on the device (`get_rdf`); excludes the barostat. Without `rdf_bins` no method of
                           the pair distributions is called on the engine, unless its `md_rdf_bins` says that an
                           earlier `DeviceMD` left them on: they are then switched off
    adf_bins, adf_rbond, adf_every : `adf_bins` given (1 .. 4096): the loop counts the bond angles between the
                           neighbours below `adf_rbond` (one distance or [n_elements, n_elements]; default and
                           largest value: the model's cutoff) of every `adf_every`-th step (the state at
                           construction is the first sample) into `adf_bins` bins over [0, pi] on the device
                           (`get_adf`); runs under the barostat too. Without `adf_bins` no method of the
                           bond-angle distributions is called on the engine, unless its `md_adf_bins` says that
                           an earlier `DeviceMD` left them on: they are then switched off
    order_bins, order_degrees, order_rbond, order_every, order_solid : `order_bins` given (1 .. 4096): the loop
                           evaluates the Steinhardt parameters q_l of `order_degrees` (default (4, 6); up to 4 of
                           1 .. 12), their neighbour averages and the solid bonds of `order_solid` = (degree,
                           threshold) (default (6, 0.5)) among the neighbours below `order_rbond` (as `adf_rbond`)
                           of every `order_every`-th step on the device (`get_order`, `get_order_atoms`); runs
                           under the barostat too. Without `order_bins` no method of the order parameters is
                           called on the engine, unless its `md_order_bins` says that an earlier `DeviceMD` left
                           them on: they are then switched off
    cluster_bins, cluster_rlink, cluster_nmin, cluster_species, cluster_series, cluster_every : `cluster_bins` given
                           (1 .. 4096): the loop finds the clusters of the atoms of `cluster_species` (symbols or
                           indices; default: all) with at least `cluster_nmin` solid bonds (default 0: no test;
                           > 0 needs `order_bins` and a `cluster_every` that is a multiple of `order_every`), linked
                           below `cluster_rlink` (as `adf_rbond`), of every `cluster_every`-th step on the device,
                           and keeps the last `cluster_series` rows (default 1) of the time series
                           (`get_clusters`); runs under the barostat too. Without `cluster_bins` no method of the
                           clusters is called on the engine, unless its `md_cluster_bins` says that an earlier
                           `DeviceMD` left them on: they are then switched off
    cna, cna_rcut, cna_rmax, cna_series, cna_every : `cna` given ("adaptive" or "fixed"): the loop gives every atom
                           its lattice type (0 other, 1 fcc, 2 hcp, 3 bcc, 4 ico) at every `cna_every`-th step on the
                           device, adaptively among the list entries within `cna_rmax` (default: the model's cutoff)
                           or with every neighbour within `cna_rcut` (fixed mode, which needs it), and keeps the last
                           `cna_series` rows (default 1) of the counts (`get_structure_types`,
                           `get_structure_counts`); runs under the barostat too. Without `cna` no method of the
                           analysis is called on the engine, unless its `md_cna_series` says that an earlier
                           `DeviceMD` left it on: it is then switched off
    sq_miller, sq_lags, sq_every, sq_currents : `sq_miller` given (int [Q, 3], 1 .. 4096 triples with |n_c| <= 64,
                           e.g. from `q_points`): the loop sums the density amplitudes at the wave vectors
                           q = 2 pi h^-1 n of every `sq_every`-th step over all atoms (the state at construction is
                           the first sample), keeps `sq_lags` rows (default 1: the static structure factor only) and
                           correlates them on the device, with `sq_currents` the currents as well
                           (`get_structure_factor`, `get_intermediate_scattering`); needs frames periodic in all three
                           directions and excludes the barostat. Without `sq_miller` no method of the structure
                           factors is called on the engine, unless its `md_sq_vectors` says that an earlier
                           `DeviceMD` left them on: they are then switched off
    flux_lags, flux_every : `flux_lags` given (1 .. 4096): the loop makes the heat current and the pressure tensor of
                           every `flux_every`-th step (the state at construction is the first sample), keeps
                           `flux_lags` rows and correlates them on the device (`get_heat_current_acf`,
                           `get_pressure_acf`); excludes the barostat. Without `flux_lags` no method of the sampler
                           is called on the engine, unless its `md_flux_lags` says that an earlier `DeviceMD` left
                           it on: it is then switched off

    Under the barostat the cell of every `Atoms` follows (the atoms are not scaled again), and every `run` call
    that moved the cells ends with one neighbour-list build for the final cells: an observer at interval 1
    therefore costs a build per step. `Engine.md_run(..., record_every=...)` gives per-step traces of energy,
    volume and pressure without cutting the run.
    """

    def __init__(self, engine_or_calculator, atoms_or_list, timestep, temperature_K=None, taut=None,
                 velocities=None, masses=None, friction=None, seed=0, pressure=None, taup=None,
                 compressibility=None, mask=None, tdamp=None, tchain=3, tloop=1, dof_removed=0, pdamp=None, pchain=3,
                 ploop=1, n_lags=None,
                 sample_every=1, rdf_bins=None, rdf_rmax=None, rdf_every=1, adf_bins=None, adf_rbond=None,
                 adf_every=1, order_degrees=None, order_rbond=None, order_bins=None, order_every=1, order_solid=None,
                 sq_miller=None, sq_lags=None, sq_every=1, sq_currents=False, cluster_bins=None, cluster_rlink=None,
                 cluster_nmin=0, cluster_species=None, cluster_series=1, cluster_every=1, cna=None, cna_rcut=None,
                 cna_rmax=None, cna_series=1, cna_every=1, flux_lags=None, flux_every=1):
        if not (np.isfinite(timestep) and timestep > 0.0):
            raise ValueError("DeviceMD: timestep must be a finite time > 0")
        self._mtk = pdamp is not None
        if self._mtk and taup is not None:
            raise ValueError("DeviceMD: pdamp (Martyna-Tobias-Klein barostat) and taup (Berendsen barostat) exclude each "
                             "other: only one barostat at a time")
        barostat = (pressure, pdamp) if self._mtk else (pressure, taup, compressibility)
        self._barostat = any(p is not None for p in barostat)
        if n_lags is not None:
            whole = lambda a: isinstance(a, (int, np.integer)) and not isinstance(a, bool)
            if not (whole(n_lags) and 1 <= n_lags <= 4096):
                raise ValueError("DeviceMD: n_lags must be an integer 1 .. 4096")
            if not (whole(sample_every) and sample_every >= 1):
                raise ValueError("DeviceMD: sample_every must be an integer >= 1")
            if self._barostat:
                raise ValueError("DeviceMD: n_lags (sampling) excludes the barostat (pressure, taup, compressibility): "
                                 "displacements in a moving cell are not defined")
        elif sample_every != 1:
            raise ValueError("DeviceMD: sample_every belongs to sampling (n_lags)")
        if rdf_bins is not None:
            whole = lambda a: isinstance(a, (int, np.integer)) and not isinstance(a, bool)
            if not (whole(rdf_bins) and 1 <= rdf_bins <= 4096):
                raise ValueError("DeviceMD: rdf_bins must be an integer 1 .. 4096")
            if not (whole(rdf_every) and rdf_every >= 1):
                raise ValueError("DeviceMD: rdf_every must be an integer >= 1")
            if rdf_rmax is not None and not (np.isfinite(rdf_rmax) and rdf_rmax > 0.0):
                raise ValueError("DeviceMD: rdf_rmax must be a finite distance > 0")
            if self._barostat:
                raise ValueError("DeviceMD: rdf_bins (pair distributions) excludes the barostat (pressure, taup, "
                                 "compressibility): normalising the counts needs one volume")
        elif rdf_every != 1 or rdf_rmax is not None:
            raise ValueError("DeviceMD: rdf_every and rdf_rmax belong to the pair distributions (rdf_bins)")
        if adf_bins is not None:
            whole = lambda a: isinstance(a, (int, np.integer)) and not isinstance(a, bool)
            if not (whole(adf_bins) and 1 <= adf_bins <= 4096):
                raise ValueError("DeviceMD: adf_bins must be an integer 1 .. 4096")
            if not (whole(adf_every) and adf_every >= 1):
                raise ValueError("DeviceMD: adf_every must be an integer >= 1")
            if adf_rbond is not None:
                rb = np.asarray(adf_rbond, dtype=np.float64)
                if rb.ndim not in (0, 2) or rb.size == 0 or not (np.all(np.isfinite(rb)) and np.all(rb > 0.0)):
                    raise ValueError("DeviceMD: adf_rbond must be a finite distance > 0, or a square matrix of them")
                if rb.ndim == 2 and (rb.shape[0] != rb.shape[1] or not np.array_equal(rb, rb.T)):
                    raise ValueError("DeviceMD: adf_rbond must be a finite distance > 0, or a square matrix of them, "
                                     "symmetric")
        elif adf_every != 1 or adf_rbond is not None:
            raise ValueError("DeviceMD: adf_every and adf_rbond belong to the bond-angle distributions (adf_bins)")
        if order_bins is not None:
            whole = lambda a: isinstance(a, (int, np.integer)) and not isinstance(a, bool)
            if not (whole(order_bins) and 1 <= order_bins <= 4096):
                raise ValueError("DeviceMD: order_bins must be an integer 1 .. 4096")
            if not (whole(order_every) and order_every >= 1):
                raise ValueError("DeviceMD: order_every must be an integer >= 1")
            degrees = (4, 6) if order_degrees is None else tuple(np.atleast_1d(order_degrees).tolist())
            if not (1 <= len(degrees) <= 4 and all(whole(l) and 1 <= l <= 12 for l in degrees)
                    and len(set(degrees)) == len(degrees)):
                raise ValueError("DeviceMD: order_degrees must be 1 .. 4 distinct integers 1 .. 12")
            solid = (6, 0.5) if order_solid is None else tuple(order_solid)
            if not (len(solid) == 2 and solid[0] in degrees and np.isfinite(solid[1]) and -1.0 < solid[1] < 1.0):
                raise ValueError("DeviceMD: order_solid must be (one of order_degrees, a threshold inside (-1, 1))")
            if order_rbond is not None:
                rb = np.asarray(order_rbond, dtype=np.float64)
                if rb.ndim not in (0, 2) or rb.size == 0 or not (np.all(np.isfinite(rb)) and np.all(rb > 0.0)):
                    raise ValueError("DeviceMD: order_rbond must be a finite distance > 0, or a square matrix of them")
                if rb.ndim == 2 and (rb.shape[0] != rb.shape[1] or not np.array_equal(rb, rb.T)):
                    raise ValueError("DeviceMD: order_rbond must be a finite distance > 0, or a square matrix of them, "
                                     "symmetric")
        elif order_every != 1 or order_rbond is not None or order_degrees is not None or order_solid is not None:
            raise ValueError("DeviceMD: order_degrees, order_rbond, order_every and order_solid belong to the "
                             "bond-orientational order (order_bins)")
        if cluster_bins is not None:
            whole = lambda a: isinstance(a, (int, np.integer)) and not isinstance(a, bool)
            if not (whole(cluster_bins) and 1 <= cluster_bins <= 4096):
                raise ValueError("DeviceMD: cluster_bins must be an integer 1 .. 4096")
            if not (whole(cluster_every) and cluster_every >= 1):
                raise ValueError("DeviceMD: cluster_every must be an integer >= 1")
            if not (whole(cluster_series) and 1 <= cluster_series <= 1048576):
                raise ValueError("DeviceMD: cluster_series must be an integer 1 .. 1048576")
            if not (whole(cluster_nmin) and 0 <= cluster_nmin <= 31):
                raise ValueError("DeviceMD: cluster_nmin must be an integer 0 .. 31")
            if cluster_nmin > 0 and order_bins is None:
                raise ValueError("DeviceMD: cluster_nmin > 0 reads the solid bonds of the bond-orientational order "
                                 "(order_bins)")
            if cluster_nmin > 0 and cluster_every % order_every != 0:
                raise ValueError("DeviceMD: with cluster_nmin > 0, cluster_every must be a multiple of order_every")
            if cluster_species is not None:
                sp = [cluster_species] if isinstance(cluster_species, (str, int, np.integer)) else list(cluster_species)
                if not sp or not all(isinstance(e, str) or (whole(e) and e >= 0) for e in sp):
                    raise ValueError("DeviceMD: cluster_species must be element symbols or indices >= 0, at least one")
            if cluster_rlink is not None:
                rb = np.asarray(cluster_rlink, dtype=np.float64)
                if rb.ndim not in (0, 2) or rb.size == 0 or not (np.all(np.isfinite(rb)) and np.all(rb > 0.0)):
                    raise ValueError("DeviceMD: cluster_rlink must be a finite distance > 0, or a square matrix of them")
                if rb.ndim == 2 and (rb.shape[0] != rb.shape[1] or not np.array_equal(rb, rb.T)):
                    raise ValueError("DeviceMD: cluster_rlink must be a finite distance > 0, or a square matrix of them, "
                                     "symmetric")
        elif (cluster_every != 1 or cluster_rlink is not None or cluster_nmin != 0 or cluster_species is not None
              or cluster_series != 1):
            raise ValueError("DeviceMD: cluster_rlink, cluster_nmin, cluster_species, cluster_series and cluster_every "
                             "belong to the cluster analysis (cluster_bins)")
        if cna is not None:
            whole = lambda a: isinstance(a, (int, np.integer)) and not isinstance(a, bool)
            if cna not in ("adaptive", "fixed"):
                raise ValueError("DeviceMD: cna must be 'adaptive' or 'fixed'")
            if not (whole(cna_every) and cna_every >= 1):
                raise ValueError("DeviceMD: cna_every must be an integer >= 1")
            if not (whole(cna_series) and 1 <= cna_series <= 1048576):
                raise ValueError("DeviceMD: cna_series must be an integer 1 .. 1048576")
            if cna == "fixed" and cna_rcut is None:
                raise ValueError("DeviceMD: cna = 'fixed' needs cna_rcut")
            if cna == "fixed" and cna_rmax is not None:
                raise ValueError("DeviceMD: cna_rmax belongs to cna = 'adaptive'")
            if cna == "adaptive" and cna_rcut is not None:
                raise ValueError("DeviceMD: cna_rcut belongs to cna = 'fixed'")
            for name, r in (("cna_rcut", cna_rcut), ("cna_rmax", cna_rmax)):
                if r is not None and not (np.ndim(r) == 0 and np.isfinite(r) and r > 0.0):
                    raise ValueError(f"DeviceMD: {name} must be a finite distance > 0")
        elif cna_every != 1 or cna_rcut is not None or cna_rmax is not None or cna_series != 1:
            raise ValueError("DeviceMD: cna_rcut, cna_rmax, cna_series and cna_every belong to the common neighbour "
                             "analysis (cna)")
        if sq_miller is not None:
            whole = lambda a: isinstance(a, (int, np.integer)) and not isinstance(a, bool)
            miller = np.asarray(sq_miller)
            if (miller.ndim != 2 or miller.shape[1] != 3 or not 1 <= len(miller) <= 4096
                    or not np.issubdtype(miller.dtype, np.integer) or np.abs(miller).max() > 64):
                raise ValueError("DeviceMD: sq_miller must be 1 .. 4096 integer triples [n_q, 3] with indices within +-64")
            if sq_lags is not None and not (whole(sq_lags) and 1 <= sq_lags <= 4096):
                raise ValueError("DeviceMD: sq_lags must be an integer 1 .. 4096")
            if not (whole(sq_every) and sq_every >= 1):
                raise ValueError("DeviceMD: sq_every must be an integer >= 1")
            if not isinstance(sq_currents, (bool, np.bool_)):
                raise ValueError("DeviceMD: sq_currents must be True or False")
            if self._barostat:
                raise ValueError("DeviceMD: sq_miller (structure factors) excludes the barostat (pressure, taup, "
                                 "compressibility): cell and positions of a snapshot would belong to different states")
        elif sq_lags is not None or sq_every != 1 or sq_currents is not False:
            raise ValueError("DeviceMD: sq_lags, sq_every and sq_currents belong to the structure factors (sq_miller)")
        if flux_lags is not None:
            whole = lambda a: isinstance(a, (int, np.integer)) and not isinstance(a, bool)
            if not (whole(flux_lags) and 1 <= flux_lags <= 4096):
                raise ValueError("DeviceMD: flux_lags must be an integer 1 .. 4096")
            if not (whole(flux_every) and flux_every >= 1):
                raise ValueError("DeviceMD: flux_every must be an integer >= 1")
            if self._barostat:
                raise ValueError("DeviceMD: flux_lags (heat current and pressure tensor) excludes the barostat "
                                 "(pressure, taup, compressibility): normalising the correlations needs one volume")
        elif flux_every != 1:
            raise ValueError("DeviceMD: flux_every belongs to the heat current and pressure tensor (flux_lags)")
        if self._mtk:
            if pressure is None or tdamp is None:
                raise ValueError("DeviceMD: the Martyna-Tobias-Klein barostat needs pressure with pdamp, and the Nose-Hoover "
                                 "chain thermostat (temperature_K, tdamp), whose temperature it takes")
            if compressibility is not None:
                raise ValueError("DeviceMD: compressibility belongs to the Berendsen barostat (taup), not to pdamp")
            if not np.isfinite(pressure):
                raise ValueError("DeviceMD: pressure must be finite")
            if not (np.isfinite(pdamp) and pdamp > 0.0):
                raise ValueError("DeviceMD: pdamp must be a finite time > 0")
            if not 1 <= int(pchain) <= 8:
                raise ValueError("DeviceMD: pchain must be 1 .. 8")
            if not 1 <= int(ploop) <= 16:
                raise ValueError("DeviceMD: ploop must be 1 .. 16")
            if mask is not None and (np.shape(mask) != (3,) or not np.any(mask)):
                raise ValueError("DeviceMD: mask must have three flags (x, y, z), at least one of them set")
        elif self._barostat:
            if any(p is None for p in barostat):
                raise ValueError("DeviceMD: the barostat needs pressure, taup and compressibility")
            if not np.isfinite(pressure):
                raise ValueError("DeviceMD: pressure must be finite")
            if not (np.isfinite(taup) and taup > 0.0):
                raise ValueError("DeviceMD: taup must be a finite time > 0")
            if not (np.isfinite(compressibility) and compressibility >= 0.0):
                raise ValueError("DeviceMD: compressibility must be finite and >= 0")
            if mask is not None and (np.shape(mask) != (3,) or not np.any(mask)):
                raise ValueError("DeviceMD: mask must have three flags (x, y, z), at least one of them set")
        elif mask is not None:
            raise ValueError("DeviceMD: mask belongs to the barostat (pressure, taup, compressibility)")
        if taut is not None and friction is not None:
            raise ValueError("DeviceMD: taut (Berendsen) and friction (Langevin) exclude each other")
        if tdamp is not None:
            if taut is not None or friction is not None:
                raise ValueError("DeviceMD: tdamp (Nose-Hoover chain) excludes taut (Berendsen) and friction (Langevin)")
            if temperature_K is None:
                raise ValueError("DeviceMD: the Nose-Hoover chain thermostat needs temperature_K with tdamp")
            if not (np.isfinite(tdamp) and tdamp > 0.0):
                raise ValueError("DeviceMD: tdamp must be a finite time > 0")
            if not (np.isfinite(temperature_K) and temperature_K > 0.0):
                raise ValueError("DeviceMD: temperature_K must be finite and > 0")
            if not 1 <= int(tchain) <= 8:
                raise ValueError("DeviceMD: tchain must be 1 .. 8")
            if not 1 <= int(tloop) <= 16:
                raise ValueError("DeviceMD: tloop must be 1 .. 16")
            if int(dof_removed) < 0:
                raise ValueError("DeviceMD: dof_removed must be >= 0")
        elif friction is not None:
            if temperature_K is None:
                raise ValueError("DeviceMD: the Langevin thermostat needs temperature_K with friction")
            if not (np.isfinite(friction) and friction > 0.0):
                raise ValueError("DeviceMD: friction must be a finite rate > 0")
            if not (np.isfinite(temperature_K) and temperature_K >= 0.0):
                raise ValueError("DeviceMD: temperature_K must be finite and >= 0")
            if not 0 <= int(seed) < 2 ** 64:
                raise ValueError("DeviceMD: the seed must fit an unsigned 64-bit integer")
        else:
            if (temperature_K is None) != (taut is None):
                raise ValueError("DeviceMD: the thermostat needs both temperature_K and taut (Berendsen) "
                                 "or temperature_K and friction (Langevin)")
            if temperature_K is not None and not (temperature_K > 0.0 and taut > 0.0):
                raise ValueError("DeviceMD: temperature_K and taut must be > 0")
        self._single = not isinstance(atoms_or_list, (list, tuple))
        self.atoms_list = [atoms_or_list] if self._single else list(atoms_or_list)
        if not self.atoms_list:
            raise ValueError("DeviceMD: at least one structure is needed")
        self._calc = None
        engine = engine_or_calculator
        if hasattr(engine_or_calculator, "_engine"):  # a TensorAlloyCalculator
            self._calc = engine_or_calculator
            engine = self._calc._engine
        if not hasattr(engine, "md_run"):
            raise ValueError("DeviceMD: an Engine or a TensorAlloyCalculator is needed")
        self.engine = engine
        self.dt = float(timestep)
        self.nsteps = 0
        self._observers = []
        n = sum(len(a) for a in self.atoms_list)
        if velocities is None:
            parts = []
            for a in self.atoms_list:
                get = getattr(a, "get_velocities", None)
                v = get() if get is not None else None
                parts.append(np.zeros((len(a), 3)) if v is None else np.asarray(v, dtype=np.float64))
            velocities = np.concatenate(parts) if parts else np.zeros((0, 3))
        velocities = np.ascontiguousarray(velocities, dtype=np.float64).reshape(-1, 3)
        if len(velocities) != n:
            raise ValueError("DeviceMD: velocities for every atom are needed")
        if masses is not None and len(np.ravel(masses)) != n:
            raise ValueError("DeviceMD: one mass for every atom is needed")
        engine.set_frames(self.atoms_list)
        engine.md_init(masses, velocities)
        self._chain = tdamp is not None
        if self._chain:   # (one thermostat at a time: the others go off first)
            engine.md_set_thermostat(0.0, 0.0)
            engine.md_set_langevin(0.0, 0.0, 0)
            engine.md_set_nose_hoover(kB * temperature_K, tdamp, int(tchain), int(tloop), int(dof_removed))
        elif friction is not None:
            engine.md_set_nose_hoover(0.0)
            engine.md_set_thermostat(0.0, 0.0)
            engine.md_set_langevin(kB * temperature_K, friction, int(seed))
        else:
            engine.md_set_nose_hoover(0.0)
            engine.md_set_langevin(0.0, 0.0, 0)
            engine.md_set_thermostat(kB * temperature_K if temperature_K is not None else 0.0,
                                     taut if taut is not None else 0.0)
        if self._mtk:   # (one barostat at a time: the other goes off first)
            engine.md_set_barostat(0.0, 0.0, 0.0)
            engine.md_set_mtk(pressure, pdamp, int(pchain), int(ploop), mask)
        else:
            if getattr(engine, "_md_mtk", 0):   # (an earlier DeviceMD left it on)
                engine.md_set_mtk(0.0, 0.0)
            if self._barostat:
                engine.md_set_barostat(pressure, taup, compressibility, mask)
            else:
                engine.md_set_barostat(0.0, 0.0, 0.0)
        self._lags = int(n_lags) if n_lags is not None else 0
        self._sample_every = int(sample_every)
        engine.md_set_sampling(self._lags, self._sample_every)   # (state 0 is the first sample)
        self._rdf_bins = int(rdf_bins) if rdf_bins is not None else 0
        # Opt-in: an engine that is never asked for pair distributions needs none of their methods, and none is
        # called on it. Deliberately one exception: an engine that says (`md_rdf_bins`) that an earlier DeviceMD
        # left them on is told to switch them off, so that this run neither pays for them nor is refused under
        # the barostat because of them.
        if self._rdf_bins:
            engine.md_set_rdf(self._rdf_bins, rdf_rmax, int(rdf_every))
        elif getattr(engine, "md_rdf_bins", 0):
            engine.md_set_rdf(0)
        self._adf_bins = int(adf_bins) if adf_bins is not None else 0
        if self._adf_bins:   # (opt-in in the same way)
            engine.md_set_adf(self._adf_bins, adf_rbond, int(adf_every))
        elif getattr(engine, "md_adf_bins", 0):
            engine.md_set_adf(0)
        self._order_bins = int(order_bins) if order_bins is not None else 0
        if self._order_bins:   # (opt-in in the same way)
            engine.md_set_order(degrees, order_rbond, self._order_bins, int(order_every), solid)
        elif getattr(engine, "md_order_bins", 0):
            engine.md_set_order(n_bins=0)
        self._cluster_bins = int(cluster_bins) if cluster_bins is not None else 0
        if self._cluster_bins:   # (opt-in in the same way; behind the order parameters it may read)
            engine.md_set_clusters(cluster_rlink, int(cluster_nmin), cluster_species, self._cluster_bins,
                                   int(cluster_series), int(cluster_every))
        elif getattr(engine, "md_cluster_bins", 0):
            engine.md_set_clusters(n_bins=0)
        self._cna = cna
        if cna is not None:   # (opt-in in the same way)
            engine.md_set_cna(cna, cna_rcut, cna_rmax, int(cna_series), int(cna_every))
        elif getattr(engine, "md_cna_series", 0):
            engine.md_set_cna(n_series=0)
        self._sq = sq_miller is not None
        self._sq_every, self._sq_currents = int(sq_every), bool(sq_currents)
        if self._sq:   # (opt-in in the same way)
            engine.md_set_sq(np.ascontiguousarray(miller, dtype=np.int32), 1 if sq_lags is None else int(sq_lags),
                             self._sq_every, self._sq_currents)
        elif getattr(engine, "md_sq_vectors", 0):
            engine.md_set_sq(None)
        self._flux_lags = int(flux_lags) if flux_lags is not None else 0
        self._flux_every = int(flux_every)
        if self._flux_lags:   # (opt-in in the same way)
            engine.md_set_flux(self._flux_lags, self._flux_every)
        elif getattr(engine, "md_flux_lags", 0):
            engine.md_set_flux(0)
        self._natoms = np.array([len(a) for a in self.atoms_list], dtype=np.int64)
        self.velocities = velocities.copy()
        self.epot = self.ekin = None   # per-frame records of the last state
        self.echain = None   # ... under the Nose-Hoover chain: the chain terms of the conserved quantity
        self.ebaro = None    # ... under the Martyna-Tobias-Klein barostat: its terms of the conserved quantity
        self.volume = self.press = None   # ... under the barostat: V [n_frames] and P_c [n_frames, 3]
        self.n_rebuilds = 0
        self._refresh(engine.md_run(0, self.dt))

    def attach(self, fn, interval=1):
        """Call `fn()` after every `interval` steps of `run` (the run is cut into chunks there)."""
        if int(interval) < 1:
            raise ValueError("DeviceMD.attach: interval must be >= 1")
        self._observers.append((fn, int(interval)))

    def _refresh(self, out):
        self.epot, self.ekin = out["epot"][-1].copy(), out["ekin"][-1].copy()
        self.n_rebuilds += out["n_rebuilds"]
        if self._chain:
            self.echain = out["echain"][-1].copy()
        if self._mtk:
            self.ebaro = out["ebaro"][-1].copy()
        x, v = self.engine.md_state()
        self.velocities = v
        a = 0
        for atoms, n in zip(self.atoms_list, self._natoms):
            atoms.positions[:] = x[a:a + n]
            if hasattr(atoms, "set_velocities"):
                atoms.set_velocities(v[a:a + n])
            a += n
        if self._barostat:
            self.volume, self.press = out["volume"][-1].copy(), out["press"][-1].copy()
            for atoms, h in zip(self.atoms_list, self.engine.md_cells()):
                atoms.set_cell(h, scale_atoms=False)   # (the device scaled the positions)
        if self._calc is not None:  # what the calculator cached belongs to other coordinates
            self._calc.reset()
            self._calc._forces_local = None

    def run(self, steps):
        """`steps` more steps; afterwards the `Atoms` objects hold the new positions."""
        steps = int(steps)
        if steps < 0:
            raise ValueError("DeviceMD.run: steps must be >= 0")
        done = 0
        while done < steps:
            chunk = steps - done
            for _, interval in self._observers:
                chunk = min(chunk, interval - (self.nsteps % interval))
            out = self.engine.md_run(chunk, self.dt, record_every=chunk)
            done += chunk
            self.nsteps += chunk
            self._refresh(out)
            for fn, interval in self._observers:
                if self.nsteps % interval == 0:
                    fn()

    def get_potential_energy(self):
        return float(self.epot[0]) if self._single else self.epot.copy()

    def get_kinetic_energy(self):
        return float(self.ekin[0]) if self._single else self.ekin.copy()

    def get_conserved_energy(self):
        """ekin + epot + the chain terms per frame: the conserved quantity of the Nose-Hoover chain dynamics; with
        `pdamp`, + the barostat's terms (`ebaro`): that of the Martyna-Tobias-Klein dynamics. Needs the Nose-Hoover
        chain thermostat."""
        if self.echain is None:
            raise ValueError("DeviceMD.get_conserved_energy: the Nose-Hoover chain thermostat is off (temperature_K, tdamp)")
        e = self.ekin + self.epot + self.echain
        if self._mtk:
            e = e + self.ebaro
        return float(e[0]) if self._single else e

    def _correlation(self, who, key):
        if not self._lags:
            raise ValueError(f"DeviceMD.{who}: sampling is off (n_lags)")
        c = self.engine.md_correlations()[key]
        t = np.arange(self._lags) * self._sample_every * self.dt
        return t, (c[0] if self._single else c)

    def get_vacf(self):
        """(t, vacf): the lag times arange(n_lags) * sample_every * timestep and the velocity autocorrelation
        <v(t0 + t) . v(t0)> per atom [n_elements, n_lags] (a batch: [n_frames, n_elements, n_lags]), averaged over
        the atoms of an element and over every time origin sampled so far; NaN where there is none yet or the
        frame has no atom of the element. No centre-of-mass correction. Needs `n_lags`."""
        return self._correlation("get_vacf", "vacf")

    def get_msd(self):
        """(t, msd): as `get_vacf` for the mean-square displacement <|x(t0 + t) - x(t0)|^2> of the unwrapped
        positions. Needs `n_lags`."""
        return self._correlation("get_msd", "msd")

    def get_samples(self, n=None):
        """The last `n` sampled states the device holds (default: all, at most `n_lags`), oldest first: a dict
        `x`, `v` [n, n_atoms, 3] and `steps` [n] (steps since construction). Needs `n_lags`."""
        if not self._lags:
            raise ValueError("DeviceMD.get_samples: sampling is off (n_lags)")
        return self.engine.md_samples(n)

    def get_rdf(self):
        """(r, g): the bin centres [rdf_bins] and the partial pair distribution functions g_ab(r)
        [n_elements, n_elements, rdf_bins] (a batch: [n_frames, n_elements, n_elements, rdf_bins]) over every
        state sampled so far, normalised as `rdf` does (NaN where the frame has no atom of an element or nothing
        was sampled yet). Raises ValueError for a frame that is not periodic in all three directions; its counts
        are in `engine.md_rdf()`. Needs `rdf_bins`."""
        if not self._rdf_bins:
            raise ValueError("DeviceMD.get_rdf: the pair distributions are off (rdf_bins)")
        out = self.engine.md_rdf()
        r, g = rdf(out["counts"], out["n_samples"], out["n_by_element"], out["volumes"], out["r_max"], pbc=out["pbc"])
        return r, (g[0] if self._single else g)

    def get_adf(self):
        """(theta, p): the bin centres in degrees [adf_bins] and the bond-angle distributions
        [n_elements, P, adf_bins] (a batch: [n_frames, n_elements, P, adf_bins]) over every state sampled so far,
        normalised as `adf` does: a probability density per degree for every species of the centre and pair of
        species of the neighbours (`engine.md_adf()["pairs"]`), NaN where there was no triple. The counts are in
        `engine.md_adf()`. Needs `adf_bins`."""
        if not self._adf_bins:
            raise ValueError("DeviceMD.get_adf: the bond-angle distributions are off (adf_bins)")
        theta, p = adf(self.engine.md_adf()["counts"])
        return theta, (p[0] if self._single else p)

    def get_order(self):
        """(q, p, pbar): the bin centres [order_bins] and the distributions of q_l and of the neighbour average
        qbar_l, [n_elements, n_degrees, order_bins] each (a batch: [n_frames, ...]), over every atom of every state
        sampled so far, normalised as `order_distribution` does, NaN for an element without atoms. The counts,
        `hist_conn` among them, are in `engine.md_order()`. Needs `order_bins`."""
        if not self._order_bins:
            raise ValueError("DeviceMD.get_order: the bond-orientational order is off (order_bins)")
        out = self.engine.md_order()
        q, p = order_distribution(out["hist_q"])
        pbar = order_distribution(out["hist_qbar"])[1]
        return q, (p[0] if self._single else p), (pbar[0] if self._single else pbar)

    def get_clusters(self):
        """The clusters the loop has found: the dict of `Engine.md_clusters` (`hist`, `series`, `steps`, ...) with
        `label`, `size` and `step` of `Engine.md_cluster_atoms` for the newest sampled state, the atoms of a batch in
        the order of the frames. `largest_cluster(series, steps, dt)` gives the nucleus size against time. Needs
        `cluster_bins`."""
        if not self._cluster_bins:
            raise ValueError("DeviceMD.get_clusters: the cluster analysis is off (cluster_bins)")
        out = self.engine.md_clusters()
        out.update(self.engine.md_cluster_atoms())
        return out

    def get_structure_types(self):
        """The lattice type of every atom in the newest sampled state: the dict of `Engine.md_cna_atoms` (`structure`:
        0 other, 1 fcc, 2 hcp, 3 bcc, 4 ico; `r_local`; `step`), the atoms of a batch in the order of the frames. Needs
        `cna`."""
        if self._cna is None:
            raise ValueError("DeviceMD.get_structure_types: the common neighbour analysis is off (cna)")
        return self.engine.md_cna_atoms()

    def get_structure_counts(self):
        """The atoms of every lattice type the loop has counted: the dict of `Engine.md_cna` (`counts` [n_frames,
        n_elements, 5], `series` [rows, n_frames, 5], `steps`, ...); `structure_fractions` normalises them. Needs
        `cna`."""
        if self._cna is None:
            raise ValueError("DeviceMD.get_structure_counts: the common neighbour analysis is off (cna)")
        return self.engine.md_cna()

    def get_order_atoms(self):
        """The order parameters of every atom in the newest sampled state: the dict of `Engine.md_order_atoms`
        (`q`, `qbar`, `n_bonds`, `n_conn`, `qlm`, `step`), the atoms of a batch in the order of the frames.
        `classify_solid(n_conn, n_min)` marks the solid ones. Needs `order_bins`."""
        if not self._order_bins:
            raise ValueError("DeviceMD.get_order_atoms: the bond-orientational order is off (order_bins)")
        return self.engine.md_order_atoms()

    def get_structure_factor(self):
        """(q, q_norm, S_ab, S): the wave vectors [n_q, 3] and their lengths [n_q] (1 / A) for the frame's cell, the
        Ashcroft-Langreth partial structure factors [n_elements, n_elements, n_q] and the total S(q) [n_q] over every
        state sampled so far, as `structure_factor` normalises them (a batch: a leading axis n_frames on all four).
        NaN where the frame has no atom of an element or nothing was sampled yet. Needs `sq_miller`."""
        if not self._sq:
            raise ValueError("DeviceMD.get_structure_factor: the structure factors are off (sq_miller)")
        out = self.engine.md_sq()
        s_ab, s = structure_factor(out["a_rho"], out["n_samples"], out["n_by_element"])
        res = (out["q"], out["q_norm"], s_ab, s)
        return tuple(r[0] for r in res) if self._single else res

    def get_intermediate_scattering(self):
        """(t, F): the lag times arange(sq_lags) * sq_every * timestep and the partial intermediate scattering
        functions F_ab(q, t) [n_elements, n_elements, sq_lags, n_q] (a batch: [n_frames, ...]) over every time origin
        sampled so far, as `intermediate_scattering` normalises them. With `sq_currents`: (t, F, C_L, C_T), the
        longitudinal current correlation and the transverse one per direction, normalised in the same way.
        `dynamic_structure_factor` transforms each of them to frequencies. Needs `sq_miller`."""
        if not self._sq:
            raise ValueError("DeviceMD.get_intermediate_scattering: the structure factors are off (sq_miller)")
        out = self.engine.md_sq()
        t = np.arange(out["n_lags"]) * self._sq_every * self.dt
        res = [intermediate_scattering(out["a_rho"], out["n_samples"], out["n_by_element"])]
        if self._sq_currents:
            res.append(intermediate_scattering(out["a_l"], out["n_samples"], out["n_by_element"]))
            res.append(intermediate_scattering(transverse_current(out["a_j"], out["a_l"]), out["n_samples"],
                                               out["n_by_element"]))
        return (t,) + tuple(r[0] if self._single else r for r in res)

    def get_heat_current_acf(self):
        """(t, C): the lag times arange(flux_lags) * flux_every * timestep and <J_a(t) J_a(0)> [3, flux_lags] (a
        batch: [n_frames, 3, flux_lags]) over every time origin sampled so far, as `heat_current_acf` normalises it;
        `green_kubo_thermal_conductivity` integrates it. Needs `flux_lags`."""
        if not self._flux_lags:
            raise ValueError("DeviceMD.get_heat_current_acf: the heat current is off (flux_lags)")
        out = self.engine.md_flux()
        c = heat_current_acf(out["a_heat"], out["n_samples"])
        return np.arange(out["n_lags"]) * self._flux_every * self.dt, c[0] if self._single else c

    def get_pressure_acf(self):
        """(t, C): the lag times and <dPi_ab(t) dPi_ab(0)> [6, flux_lags] (xx yy zz yz xz xy; a batch: [n_frames, 6,
        flux_lags]) with Pi = P V, the squared mean over all samples subtracted, as `pressure_acf` normalises it;
        `green_kubo_viscosity` integrates its shear components. Needs `flux_lags`."""
        if not self._flux_lags:
            raise ValueError("DeviceMD.get_pressure_acf: the pressure tensor is off (flux_lags)")
        out = self.engine.md_flux()
        c = pressure_acf(out["a_press"], out["sums"], out["n_samples"])
        return np.arange(out["n_lags"]) * self._flux_every * self.dt, c[0] if self._single else c

    def get_volume(self):
        """Cell volume per frame, in A^3."""
        v = np.array([abs(np.linalg.det(np.asarray(a.get_cell(complete=True)))) for a in self.atoms_list])
        return float(v[0]) if self._single else v

    def get_cell(self):
        """The cell [3, 3] (a batch: [n_frames, 3, 3]) as the library holds it."""
        h = self.engine.md_cells()
        return h[0] if self._single else h

    def get_pressure(self):
        """(P_x + P_y + P_z) / 3 of the last state per frame, in eV / A^3: kinetic part included, as the barostat
        sees it. Needs the barostat."""
        if self.press is None:
            raise ValueError("DeviceMD.get_pressure: the barostat is off (pressure, taup, compressibility)")
        p = self.press.mean(axis=1)
        return float(p[0]) if self._single else p

    def get_temperature(self):
        """2 KE / (3 N kB) per frame, in K."""
        t = 2.0 * self.ekin / (3.0 * np.maximum(self._natoms, 1) * kB)
        return float(t[0]) if self._single else t
