"""
Harmonic phonons from the analytic Hessian: frequencies, bands, density of states and thermal properties.

Takes the place of the phonopy step behind the reference's `analysis/phonon.py`. The force constants of the
home-cell atoms come from `ta_hessian_vectors` and stay on the device; the dynamical matrices of a batch of
q-points, their eigensystems and the DOS histogram are device kernels (`csrc/ta_phonon.hip`). What is left to
NumPy is geometry (supercell, shortest vectors, meshes, paths) and the thermal sums over frequencies.

Conventions: D(q)[3b+a, 3b'+c] = (m_b m_b')^(-1/2) sum_{s in b'} Phi_ac(b, s) (1/mult) sum_r exp(i q.r), r over the
shortest vectors from home atom b to the images of supercell atom s (phonopy's); q in reduced coordinates of the
primitive cell's reciprocal lattice; frequencies in THz, imaginary modes negative.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .atoms import Atoms, atomic_masses

THZ = _lib.TA_PHONON_THZ       # THz per sqrt(eV / A^2 / amu): 1000 fs / (2 pi), fs as in md.py
THZ_TO_EV = 4.135667696e-3     # h nu in eV for nu = 1 THz
THZ_TO_CM = 33.3564095198152   # 1 THz in cm^-1
KB = 8.617333262e-5            # eV / K
SYMPREC = 1e-5


def shortest_vectors(positions, cell, n_basis, pbc=(True, True, True), symprec=SYMPREC):
    """CSR list of the shortest vectors from the home atoms b < n_basis to the periodic images of every atom s
    of the supercell: (start [n_basis N + 1] int32, vectors [*, 3]), pair (b, s) at b N + s. Every image among
    the 27 neighbouring cells whose length is within `symprec` of the pair's minimum is listed (their weight is
    1 / their number), in the order of the image index. The supercell should be compact enough for its 27
    neighbours to hold the nearest images (any cell whose reduced form it is)."""
    positions = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    N = len(positions)
    rng = [(-1, 0, 1) if p else (0,) for p in np.asarray(pbc, dtype=bool)]
    shifts = np.array([(i, j, k) for i in rng[0] for j in rng[1] for k in rng[2]], dtype=np.float64) @ cell
    d = positions[None, :, :] - positions[:n_basis, None, :]             # [nb, N, 3]
    cand = d[:, :, None, :] + shifts[None, None, :, :]                   # [nb, N, S, 3]
    length = np.sqrt((cand ** 2).sum(-1))
    keep = length - length.min(axis=2, keepdims=True) < symprec
    counts = keep.sum(axis=2).reshape(-1)
    start = np.zeros(n_basis * N + 1, dtype=np.int32)
    np.cumsum(counts, out=start[1:])
    return start, np.ascontiguousarray(cand[keep])


def reciprocal(cell):
    """Rows = reciprocal lattice vectors with the 2 pi: q_cart = q_reduced @ reciprocal(cell)."""
    return 2.0 * np.pi * np.linalg.inv(np.asarray(cell, dtype=np.float64).reshape(3, 3)).T


def mesh_points(n1, n2, n3, shift=False):
    """Reduced coordinates [n1 n2 n3, 3] of a uniform mesh: (k + s) / n, k = 0 .. n - 1, with s = 1/2 when
    `shift` (the mesh then avoids Gamma), else 0 (Gamma-centred). The last index runs fastest."""
    s = 0.5 if shift else 0.0
    axes = [(np.arange(n) + s) / n for n in (int(n1), int(n2), int(n3))]
    g = np.meshgrid(*axes, indexing="ij")
    return np.stack([x.reshape(-1) for x in g], axis=1)


def band_path(paths, npoints, recip):
    """q-points along explicit paths. `paths`: a list of paths, each a list of reduced q-points; every segment
    between two consecutive points is sampled with `npoints` points, ends included. Returns (q_reduced [M, 3],
    distance [M]) with the distance in 1/Angstrom accumulated along each path and continuing from path to path."""
    qs, dist, d0 = [], [], 0.0
    for path in paths:
        path = np.asarray(path, dtype=np.float64).reshape(-1, 3)
        for a, b in zip(path[:-1], path[1:]):
            t = np.linspace(0.0, 1.0, int(npoints))
            seg = a[None, :] + t[:, None] * (b - a)[None, :]
            qs.append(seg)
            dist.append(d0 + t * np.linalg.norm((b - a) @ recip))
            d0 = dist[-1][-1]
    if not qs:
        return np.zeros((0, 3)), np.zeros(0)
    return np.concatenate(qs), np.concatenate(dist)


def harmonic_thermal(freq_THz, T, n_q, cutoff=0.01):
    """Harmonic free energy, entropy and heat capacity per cell from mode frequencies (THz) of `n_q` q-points
    at the temperatures T (K): F = sum [h nu / 2 + kT ln(1 - exp(-h nu / kT))] / n_q (eV),
    S = k sum [x / (exp(x) - 1) - ln(1 - exp(-x))] / n_q and C_v = k sum x^2 exp(x) / (exp(x) - 1)^2 / n_q
    (eV / K), x = h nu / kT. Modes with nu <= cutoff (acoustic modes at Gamma, imaginary modes) are skipped and
    counted."""
    nu = np.asarray(freq_THz, dtype=np.float64).reshape(-1)
    use = nu > cutoff
    e = nu[use] * THZ_TO_EV
    T = np.atleast_1d(np.asarray(T, dtype=np.float64))
    F, S, Cv = np.zeros(len(T)), np.zeros(len(T)), np.zeros(len(T))
    for i, t in enumerate(T):
        if t <= 0.0:
            F[i] = 0.5 * e.sum()
            continue
        x = e / (KB * t)
        em = np.exp(-x)
        log_term = np.log1p(-em)
        F[i] = (0.5 * e + KB * t * log_term).sum()
        S[i] = KB * (x * em / (-np.expm1(-x)) - log_term).sum()
        Cv[i] = KB * (x * x * em / np.expm1(-x) ** 2).sum()
    return {"temperatures": T, "free_energy": F / n_q, "entropy": S / n_q, "heat_capacity": Cv / n_q,
            "skipped": int((~use).sum())}


class Phonons:
    """Phonons of `atoms` (the primitive or any home cell) with a `supercell=(n1, n2, n3)` of it.

    `Phonons(calculator_or_engine, atoms, supercell)` builds the supercell with the home cell first, makes it
    the engine's resident frame, hands the shortest-vector lists to the library and computes the force constants
    with the analytic Hessian-vector products (ValueError for models that have none; use
    `from_force_constants` with finite-difference constants then)."""

    def __init__(self, calculator_or_engine, atoms, supercell=(1, 1, 1), masses=None, q_chunk=0, _phi=None,
                 _super=None, _mapping=None):
        self.engine = getattr(calculator_or_engine, "_engine", calculator_or_engine)
        self.n_basis = len(atoms)
        self.supercell = tuple(int(x) for x in supercell)
        pbc = np.asarray(atoms.pbc, dtype=bool)
        if any(n != 1 and not p for n, p in zip(self.supercell, pbc)):
            raise ValueError("Phonons: a supercell can only repeat periodic directions")
        self.primitive_cell = np.asarray(atoms.get_cell(complete=True), dtype=np.float64)
        self.recip = reciprocal(self.primitive_cell)
        self.super_atoms = _super if _super is not None else atoms.repeat(self.supercell)
        N = len(self.super_atoms)
        self.basis_of = np.asarray(_mapping if _mapping is not None else np.arange(N) % self.n_basis, dtype=np.int32)
        self.masses = np.asarray(masses if masses is not None else [atomic_masses[z] for z in atoms.numbers],
                                 dtype=np.float64)
        self.start, self.vectors = shortest_vectors(self.super_atoms.positions,
                                                    self.super_atoms.get_cell(complete=True), self.n_basis, pbc)
        self.engine.set_frames([self.super_atoms])
        self.engine.phonon_set_cell(self.n_basis, self.basis_of, self.masses, self.start, self.vectors, q_chunk)
        if _phi is None:
            self.force_constants = self.engine.phonon_force_constants()
        else:
            phi = np.asarray(_phi, dtype=np.float64)
            if phi.shape == (N, N, 3, 3):
                phi = phi[:self.n_basis]
            self.force_constants = np.ascontiguousarray(phi)
            self.engine.phonon_load_force_constants(self.force_constants)

    @classmethod
    def from_force_constants(cls, calculator_or_engine, force_constants, supercell_atoms, n_basis,
                             supercell=(1, 1, 1), mapping=None, masses=None, q_chunk=0):
        """Phonons from ready force constants Phi [N, N, 3, 3] or [n_basis, N, 3, 3] (eV / A^2) of the
        `supercell_atoms`, whose first `n_basis` atoms are the home cell and whose cell is `supercell` repeats of
        the primitive cell; `mapping[s]` = the home atom that atom s is an image of (default s mod n_basis)."""
        sup = supercell_atoms
        cell = np.asarray(sup.get_cell(complete=True)) / np.asarray(supercell, dtype=np.float64)[:, None]
        home = Atoms(numbers=sup.numbers[:n_basis], positions=sup.positions[:n_basis], cell=cell, pbc=sup.pbc)
        return cls(calculator_or_engine, home, supercell, masses=masses, q_chunk=q_chunk, _phi=force_constants,
                   _super=sup, _mapping=mapping)

    # -- q-points ------------------------------------------------------------------------
    def q_cartesian(self, q_reduced):
        return np.asarray(q_reduced, dtype=np.float64).reshape(-1, 3) @ self.recip

    def frequencies(self, q_reduced, eigenvectors=False):
        """Frequencies [Q, 3 n_basis] in THz at reduced q-points; with `eigenvectors` also [Q, n, n] complex,
        row m = the unit eigenvector of mode m of the mass-weighted dynamical matrix."""
        return self.engine.phonon_frequencies(self.q_cartesian(q_reduced), eigenvectors=eigenvectors)

    def band_structure(self, paths, npoints=51):
        """(distances [M], frequencies [M, n]) along explicit paths of reduced q-points (see `band_path`)."""
        q, dist = band_path(paths, npoints, self.recip)
        return dist, self.frequencies(q)

    def mesh(self, n1, n2, n3, shift=False):
        return mesh_points(n1, n2, n3, shift)

    def dos(self, mesh, n_bins, nu_range, partial=False):
        """Phonon DOS over a mesh ((n1, n2, n3) or (n1, n2, n3, shift), or an array of reduced q-points):
        a dict with `frequencies` (bin centres, THz), `total` (modes per bin), `outside` and, with `partial`,
        the per-atom weights [n_basis, n_bins]. The histogram is formed on the device."""
        q = mesh_points(*mesh) if np.ndim(mesh) == 1 else np.asarray(mesh, dtype=np.float64)
        lo, hi = float(nu_range[0]), float(nu_range[1])
        out = self.engine.phonon_dos(self.q_cartesian(q), n_bins, lo, hi, partial=partial)
        out["frequencies"] = lo + (np.arange(int(n_bins)) + 0.5) * ((hi - lo) / int(n_bins))
        out["n_q"] = len(q)
        return out

    def thermal_properties(self, T, mesh, cutoff=0.01):
        """Harmonic free energy (eV), entropy and C_v (eV / K) per home cell at the temperatures T (K) from the
        mesh frequencies (`harmonic_thermal`)."""
        q = mesh_points(*mesh) if np.ndim(mesh) == 1 else np.asarray(mesh, dtype=np.float64)
        return harmonic_thermal(self.frequencies(q), T, len(q), cutoff)
