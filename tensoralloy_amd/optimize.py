"""
Structure relaxation on the device: `DeviceFIRE` drives `Engine.relax_run` (`ta_relax_run`), which takes
FIRE steps of the resident batch without moving coordinates, velocities or forces through the host.

The optimiser is ASE's `FIRE` with `downhill_check=False` and the same parameter names and defaults. Every
structure of a batch is relaxed on its own: it has its own time step and mixing factor, and it stops moving
when its largest force drops below `fmax` while the others go on. Converged structures stay in the batch
and are still evaluated, so a run costs (steps of the slowest structure) x (one evaluation of the batch).
Cells stay fixed unless `cell=True`: then the cell of every structure is relaxed with its atoms as ASE's
`UnitCellFilter` does it (`Engine.relax_set_cell`), to zero stress or to the pressure `scalar_pressure`.
"""
from __future__ import annotations

import numpy as np

from .utils import fixed_atoms_mask

__all__ = ["DeviceFIRE"]


def _check_params(dt, maxstep, dtmax, Nmin, finc, fdec, astart, fa):
    for name, v in (("dt", dt), ("dtmax", dtmax), ("maxstep", maxstep)):
        if not (np.isfinite(v) and v > 0.0):
            raise ValueError(f"DeviceFIRE: {name} must be finite and > 0")
    if not (np.isfinite(finc) and finc >= 1.0):
        raise ValueError("DeviceFIRE: finc must be finite and >= 1")
    for name, v in (("fdec", fdec), ("fa", fa)):
        if not 0.0 < v < 1.0:
            raise ValueError(f"DeviceFIRE: {name} must lie in (0, 1)")
    if not 0.0 < astart <= 1.0:
        raise ValueError("DeviceFIRE: astart must lie in (0, 1]")
    if int(Nmin) != Nmin or Nmin < 0:
        raise ValueError("DeviceFIRE: Nmin must be an integer >= 0")


class DeviceFIRE:
    """
    FIRE relaxation of one structure or of a batch of independent structures on the GPU.

    engine_or_calculator : an `Engine`, or a `TensorAlloyCalculator` whose engine and skin are used (its
                           cached results are invalidated by every run)
    atoms_or_list        : one `Atoms` or a list of them (they become the resident batch)
    fixed                : boolean mask or list of indices over the concatenated atoms: these atoms do not
                           move and their forces do not count towards convergence (ASE's `FixAtoms`)
    dt, maxstep, dtmax, Nmin, finc, fdec, astart, fa : as ASE's `FIRE`
    cell                 : relax the cells too (ASE's `UnitCellFilter`); `fmax` then also bounds the rows of the
                           generalised cell force, and fixed atoms move affinely with the cell
    mask, scalar_pressure, hydrostatic_strain, cell_factor : as ASE's `UnitCellFilter` (mask: 6 Voigt entries
                           xx, yy, zz, yz, xz, xy or 3 x 3; pressure in eV / A^3; cell_factor None = atoms of
                           the structure); only with `cell=True`
    """

    def __init__(self, engine_or_calculator, atoms_or_list, fixed=None, dt=0.1, maxstep=0.2, dtmax=1.0, Nmin=5,
                 finc=1.1, fdec=0.5, astart=0.1, fa=0.99, cell=False, mask=None, scalar_pressure=0.0,
                 hydrostatic_strain=False, cell_factor=None):
        _check_params(dt, maxstep, dtmax, Nmin, finc, fdec, astart, fa)
        if not cell and (mask is not None or scalar_pressure != 0.0 or hydrostatic_strain or cell_factor is not None):
            raise ValueError("DeviceFIRE: mask, scalar_pressure, hydrostatic_strain and cell_factor need cell=True")
        self._single = not isinstance(atoms_or_list, (list, tuple))
        self.atoms_list = [atoms_or_list] if self._single else list(atoms_or_list)
        if not self.atoms_list:
            raise ValueError("DeviceFIRE: at least one structure is needed")
        n = sum(len(a) for a in self.atoms_list)
        if fixed is not None:
            fixed = fixed_atoms_mask(fixed, n, "DeviceFIRE")
        self._calc = None
        engine = engine_or_calculator
        if hasattr(engine_or_calculator, "_engine"):  # a TensorAlloyCalculator
            self._calc = engine_or_calculator
            engine = self._calc._engine
        if not hasattr(engine, "relax_run"):
            raise ValueError("DeviceFIRE: an Engine or a TensorAlloyCalculator is needed")
        self.engine = engine
        self.fixed = fixed
        self.nsteps = 0
        self._observers = []
        self._natoms = np.array([len(a) for a in self.atoms_list], dtype=np.int64)
        self.energy = self.fmax = None   # per-frame values of the last state
        self.converged = np.zeros(len(self.atoms_list), dtype=bool)
        self.n_rebuilds = 0
        engine.set_frames(self.atoms_list)
        engine.relax_init(fixed=fixed, dt=dt, dtmax=dtmax, maxstep=maxstep, finc=finc, fdec=fdec, astart=astart,
                          fa=fa, nmin=int(Nmin))
        self.cell = bool(cell)
        if self.cell:
            engine.relax_set_cell(True, cell_factor=cell_factor, pressure=scalar_pressure, mask=mask,
                                  hydrostatic=hydrostatic_strain)
        self._refresh(engine.relax_run(0, np.finfo(np.float64).tiny))   # energy and forces of the start

    def attach(self, fn, interval=1):
        """Call `fn()` after every `interval` steps of `run` (the run is cut into chunks there)."""
        if int(interval) < 1:
            raise ValueError("DeviceFIRE.attach: interval must be >= 1")
        self._observers.append((fn, int(interval)))

    def _refresh(self, out):
        self.energy, self.fmax, self.converged = out["energy"], out["fmax"], out["converged"]
        self.n_rebuilds += out["n_rebuilds"]
        x = self.engine.relax_state()["positions"]
        a = 0
        for atoms, n in zip(self.atoms_list, self._natoms):
            atoms.positions[:] = x[a:a + n]
            a += n
        if self.cell:
            for atoms, h in zip(self.atoms_list, self.engine.relax_cell_state()["cells"]):
                atoms.set_cell(h, scale_atoms=False)
        if self._calc is not None:  # what the calculator cached belongs to other coordinates
            self._calc.reset()
            self._calc._forces_local = None

    def run(self, fmax=0.05, steps=100000):
        """Relax until every structure has max |F_i| < `fmax` (eV / A) or `steps` more steps were taken.
        Returns whether it converged: one bool, or an array of bools for a list of structures. Afterwards
        the `Atoms` objects hold the new positions."""
        steps = int(steps)
        if steps < 0:
            raise ValueError("DeviceFIRE.run: steps must be >= 0")
        if not (np.isfinite(fmax) and fmax > 0.0):
            raise ValueError("DeviceFIRE.run: fmax must be finite and > 0")
        done = 0
        while True:
            chunk = steps - done
            for _, interval in self._observers:
                chunk = min(chunk, interval - (self.nsteps % interval))
            out = self.engine.relax_run(chunk, fmax)
            taken = int(out["steps"].max()) if len(out["steps"]) else 0
            done += taken
            self.nsteps += taken
            self._refresh(out)
            if taken:
                for fn, interval in self._observers:
                    if self.nsteps % interval == 0:
                        fn()
            if self.converged.all() or done >= steps:
                break
        return bool(self.converged[0]) if self._single else self.converged.copy()

    def get_potential_energy(self):
        return float(self.energy[0]) if self._single else self.energy.copy()

    def get_stress(self):
        """Stress W / V of the last state in Voigt order (xx, yy, zz, yz, xz, xy), eV / A^3: [6] for one
        structure, [n, 6] for a list."""
        from . import _lib
        w = self.engine.fetch(_lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES | _lib.TA_WANT_VIRIAL)["virial"]
        s = w / self.engine._volumes[:, None, None]
        voigt = np.stack([s[:, 0, 0], s[:, 1, 1], s[:, 2, 2], s[:, 1, 2], s[:, 0, 2], s[:, 0, 1]], axis=1)
        return voigt[0] if self._single else voigt

    def get_forces(self):
        """Forces [n_atoms, 3] of the last state (all structures concatenated), fixed atoms' set to 0."""
        from . import _lib
        f = self.engine.fetch(_lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES)["forces"].copy()
        if self.fixed is not None:
            f[self.fixed] = 0.0
        return f
