"""
Minimum-energy paths on the device: `DeviceNEB` drives `Engine.relax_run` in band mode
(`Engine.relax_set_band`, `ta_relax_set_band`), which takes FIRE steps of a nudged elastic band without
moving coordinates, forces or tangents through the host.

The images are the resident batch: the first and the last are fixed endpoints, the others move under the
improved-tangent band force of Henkelman and Jonsson (ASE's `NEB(method='improvedtangent', climb=...)` with
one spring constant `k`), and one FIRE with ASE's parameter names and defaults optimises the whole band, as
ASE does when an optimiser is attached to a `NEB`. Differences between images are plain differences of the
coordinates as given, with no minimum-image convention: build the band with `interpolate`, which unwraps it.
"""
from __future__ import annotations

import numpy as np

from .optimize import _check_params
from .utils import fixed_atoms_mask

__all__ = ["DeviceNEB", "interpolate"]


def _cell(atoms):
    return np.asarray(atoms.get_cell(complete=True), dtype=np.float64).reshape(3, 3)


def _pbc(atoms):
    return np.broadcast_to(np.asarray(atoms.pbc, dtype=bool), (3,))


def _same_system(a, b):
    """None, or what differs between two images."""
    if len(a) != len(b):
        return "atom count"
    if not np.array_equal(np.asarray(a.numbers), np.asarray(b.numbers)):
        return "species"
    if not np.array_equal(_cell(a), _cell(b)):
        return "cell"
    if not np.array_equal(_pbc(a), _pbc(b)):
        return "pbc"
    return None


def interpolate(initial, final, n_images, mic=True):
    """`n_images` images (both endpoints included) on the straight line from `initial` to `final`, as a list
    of new `Atoms`. With `mic` the displacement of every atom from `initial` to `final` is taken by minimum
    image once (along the periodic axes), so the images are unwrapped and consecutive: the last one may differ
    from `final` by lattice vectors."""
    n_images = int(n_images)
    if n_images < 2:
        raise ValueError("interpolate: n_images must be >= 2 (the endpoints are counted)")
    what = _same_system(initial, final)
    if what is not None:
        raise ValueError(f"interpolate: initial and final differ in their {what}")
    d = np.asarray(final.positions, dtype=np.float64) - np.asarray(initial.positions, dtype=np.float64)
    pbc = _pbc(initial)
    if mic and pbc.any():
        cell = _cell(initial)
        frac = np.linalg.solve(cell.T, d.T).T
        frac[:, pbc] -= np.round(frac[:, pbc])
        d = frac @ cell
    images = []
    for i in range(n_images):
        atoms = initial.copy()
        atoms.positions[:] = np.asarray(initial.positions, dtype=np.float64) + d * (i / (n_images - 1))
        images.append(atoms)
    return images


class DeviceNEB:
    """
    Nudged elastic band of `images` on the GPU, optimised by one FIRE over the whole band.

    engine_or_calculator : an `Engine`, or a `TensorAlloyCalculator` whose engine and skin are used (its
                           cached results are invalidated by every run)
    images               : list of at least 3 `Atoms` with the same atoms in the same order, the same cell and
                           pbc; the first and the last stay where they are (they become the resident batch)
    k                    : spring constant, eV / A^2 (ASE's default)
    climb                : the interior image of highest energy climbs (re-chosen at every step)
    fixed                : boolean mask or list of indices over the n atoms of ONE image, applied to every
                           image: these atoms do not move and do not count towards convergence
    dt, maxstep, dtmax, Nmin, finc, fdec, astart, fa : as ASE's `FIRE`
    """

    def __init__(self, engine_or_calculator, images, k=0.1, climb=False, fixed=None, dt=0.1, maxstep=0.2,
                 dtmax=1.0, Nmin=5, finc=1.1, fdec=0.5, astart=0.1, fa=0.99):
        _check_params(dt, maxstep, dtmax, Nmin, finc, fdec, astart, fa)
        if not (np.isfinite(k) and k > 0.0):
            raise ValueError("DeviceNEB: k must be finite and > 0")
        self.images = list(images)
        if len(self.images) < 3:
            raise ValueError("DeviceNEB: a band needs at least 3 images (two endpoints and one between them)")
        first = self.images[0]
        for i, atoms in enumerate(self.images[1:], start=1):
            what = _same_system(first, atoms)
            if what is not None:
                raise ValueError(f"DeviceNEB: image {i} differs from image 0 in its {what}")
        n = len(first)
        pbc = _pbc(first)
        if pbc.any() and n:
            # plain differences between images stand for the path only while no atom jumps across the cell
            cell = _cell(first)
            x = np.stack([np.asarray(a.positions, dtype=np.float64) for a in self.images])
            frac = np.linalg.solve(cell.T, np.diff(x, axis=0).reshape(-1, 3).T).T.reshape(len(self.images) - 1, n, 3)
            jump = np.abs(frac[:, :, pbc]).max(axis=2)
            if jump.max() >= 0.5:
                i, j = np.unravel_index(int(jump.argmax()), jump.shape)
                raise ValueError(f"DeviceNEB: atom {j} moves by {jump[i, j]:.3f} of a periodic cell vector between "
                                 f"images {i} and {i + 1}; the band takes plain differences between images, "
                                 f"so it must be unwrapped (see interpolate)")
        mask = None
        if fixed is not None:
            mask = np.tile(fixed_atoms_mask(fixed, n, "DeviceNEB"), len(self.images))
        self._calc = None
        engine = engine_or_calculator
        if hasattr(engine_or_calculator, "_engine"):  # a TensorAlloyCalculator
            self._calc = engine_or_calculator
            engine = self._calc._engine
        if not hasattr(engine, "relax_set_band"):
            raise ValueError("DeviceNEB: an Engine or a TensorAlloyCalculator is needed")
        self.engine = engine
        self.fixed = mask
        self.k = float(k)
        self.climb = bool(climb)
        self.nsteps = 0
        self.n_rebuilds = 0
        self.converged = False
        self.fmax = None       # the band's max |B_i| of the last state
        self._band = None
        self._observers = []
        self._n = n
        engine.set_frames(self.images)
        engine.relax_init(fixed=mask, dt=dt, dtmax=dtmax, maxstep=maxstep, finc=finc, fdec=fdec, astart=astart,
                          fa=fa, nmin=int(Nmin))
        engine.relax_set_band(True, k=self.k, climb=self.climb)
        self._refresh(engine.relax_run(0, np.finfo(np.float64).tiny))   # energies and band forces of the start

    def attach(self, fn, interval=1):
        """Call `fn()` after every `interval` steps of `run` (the run is cut into chunks there)."""
        if int(interval) < 1:
            raise ValueError("DeviceNEB.attach: interval must be >= 1")
        self._observers.append((fn, int(interval)))

    def set_climb(self, climb=True):
        """Switch the climbing image on or off. The optimiser starts again (v = 0, dt, a), as one does with ASE
        when a converged band is refined with a climbing image."""
        self.climb = bool(climb)
        self.engine.relax_set_band(True, k=self.k, climb=self.climb)
        self._refresh(self.engine.relax_run(0, np.finfo(np.float64).tiny))

    def _refresh(self, out):
        self.fmax, self.converged = float(out["fmax"][0]), bool(out["converged"][0])
        self.n_rebuilds += out["n_rebuilds"]
        self._band = self.engine.relax_band_state()
        x = self.engine.relax_state()["positions"].reshape(len(self.images), self._n, 3)
        for atoms, xi in zip(self.images, x):
            atoms.positions[:] = xi
        if self._calc is not None:  # what the calculator cached belongs to other coordinates
            self._calc.reset()
            self._calc._forces_local = None

    def run(self, fmax=0.05, steps=100000):
        """Optimise until max |B_i| < `fmax` (eV / A) over all moving atoms of the band, or `steps` more steps
        were taken. Returns whether it converged. Afterwards the `Atoms` of the images hold the new positions."""
        steps = int(steps)
        if steps < 0:
            raise ValueError("DeviceNEB.run: steps must be >= 0")
        if not (np.isfinite(fmax) and fmax > 0.0):
            raise ValueError("DeviceNEB.run: fmax must be finite and > 0")
        done = 0
        while True:
            chunk = steps - done
            for _, interval in self._observers:
                chunk = min(chunk, interval - (self.nsteps % interval))
            out = self.engine.relax_run(chunk, fmax)
            taken = int(out["steps"][0])
            done += taken
            self.nsteps += taken
            self._refresh(out)
            if taken:
                for fn, interval in self._observers:
                    if self.nsteps % interval == 0:
                        fn()
            if self.converged or done >= steps:
                break
        return self.converged

    def get_energies(self):
        """Energies [n_images] of the last state."""
        return self._band["energies"].copy()

    def get_forces(self):
        """Band forces [n_images, n, 3] of the last state (0 on the endpoints and on fixed atoms)."""
        return self._band["forces"].reshape(len(self.images), self._n, 3).copy()

    def get_tangents(self):
        """Unit tangents [n_images, n, 3] of the last state (0 on the endpoints)."""
        return self._band["tangents"].reshape(len(self.images), self._n, 3).copy()

    def get_climbing_image(self):
        """Index of the climbing image of the last state, -1 without `climb`."""
        return self._band["climbing"]

    def get_barrier(self):
        """Highest image energy minus the energy of image 0, eV."""
        e = self._band["energies"]
        return float(e.max() - e[0])
