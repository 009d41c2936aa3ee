"""
`Engine`: thin Python owner of one `ta_handle` (one GPU, one HIP stream).

This is the only place where Python meets the C ABI for evaluation. It plays
the role of `tf.Session` in the reference calculator (calculator.py:79, :368):
load once, then run many structures. Frames of a batch are independent units
and are evaluated by a single set of kernel launches.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, List, Sequence

import numpy as np

from . import _lib
from .utils import GPa


class Engine:
    def __init__(self, nn, device: int = 0):
        self._lib = _lib.load()
        self._nn = nn
        self._clf = nn.transformer
        if self._clf is None:
            raise ValueError("A descriptor transformer must be attached.")
        desc, keep = nn.to_desc()
        self._handle = C.c_void_p()
        rc = self._lib.ta_create(C.byref(desc), int(device), C.byref(self._handle))
        del keep
        if rc != _lib.TA_OK:
            _lib.check(self._lib, None, rc)
        self.device = int(device)
        self.info = None
        self._frames = None
        self._volumes = None
        self._relax_cell = False   # `relax_set_cell` is on: `relax_run` moves the cells
        self._md_barostat = False  # `md_set_barostat` is on: `md_run` moves the cells
        self._md_chain = 0         # `md_set_nose_hoover` is on: thermostats per chain
        self._md_mtk = 0           # `md_set_mtk` is on: thermostats of the barostat's chain; `md_run` moves the cells
        self._md_lags = 0          # `md_set_sampling` is on: snapshots in the ring
        self._md_bins = 0          # `md_set_rdf` is on: bins of the pair distributions
        self._md_adf_bins = 0      # `md_set_adf` is on: bins of the bond-angle distributions
        self._md_order_bins = 0    # `md_set_order` is on: bins of the order-parameter histograms,
        self._md_order_degrees = ()        # its degrees
        self._md_order_solid = (0, 0.0)    # and (solid_degree, threshold)
        self._md_sq = (0, 1, False)        # `md_set_sq` is on: (n_q, n_lags, currents)
        self._md_flux_lags = 0             # `md_set_flux` is on: n_lags
        self._md_cluster = (0, 1)          # `md_set_clusters` is on: (n_bins, n_series)
        self._md_cna = 0                   # `md_set_cna` is on: n_series
        self._n_elements = int(desc.n_elements)
        # what the neighbour list is complete for: max(rcut, acut), acut counting for angular models only
        self._md_cutoff = max(float(desc.rcut), float(desc.acut)) if int(desc.angular) else float(desc.rcut)
        self._md_sig = None   # (n, numbers, pbc) of the single resident frame of `evaluate_md`
        self._md_cell = None
        self.batch_generation = 0  # bumped whenever the resident batch or its coordinates change
        # temperature-dependent models: electron temperature (eV) of every resident frame
        self.finite_temperature = bool(getattr(nn, "is_finite_temperature", False))
        self._etemperatures = None

    # -- lifetime ----------------------------------------------------------------
    def close(self):
        if getattr(self, "_handle", None) is not None and self._handle.value:
            self._lib.ta_destroy(self._handle)
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        _lib.check(self._lib, self._handle, rc)

    # -- batch ----------------------------------------------------------------------
    def set_frames(self, atoms_list: Sequence) -> _lib.BatchInfo:
        """Neighbour lists + upload; afterwards the batch is resident in HBM."""
        frames = []
        periodic = self._clf.periodic
        for atoms in atoms_list:
            pbc = np.asarray(atoms.pbc, dtype=bool) if periodic else np.zeros(3, dtype=bool)
            frames.append(_lib.FrameArrays(self._clf.species_indices(atoms), atoms.positions,
                                           np.asarray(atoms.get_cell(complete=True)), pbc))
        arr = (_lib.Frame * max(len(frames), 1))(*[f.as_struct() for f in frames])
        info = _lib.BatchInfo()
        self._check(self._lib.ta_set_frames(self._handle, len(frames), arr, C.byref(info)))
        self.info = info
        self._frames = frames
        self.batch_generation += 1  # what is resident changed (train.Trainer's shortcut checks this)
        self._md_sig = None
        self._relax_cell = False
        self._phonon = None  # `phonon_set_cell` belongs to the batch that leaves
        self._volumes = np.array([abs(np.linalg.det(f.cell)) for f in frames])
        self._natoms = np.array([len(f.species) for f in frames], dtype=np.int64)
        self._numbers = np.concatenate([np.asarray(a.numbers, dtype=np.int64) for a in atoms_list]) \
            if len(frames) else np.zeros(0, dtype=np.int64)
        if self.finite_temperature:
            # the reference's `etemperature` feature, 0 when the structure has none (universal.py:295)
            self.set_electron_temperatures([float(a.info.get("etemperature", 0.0)) for a in atoms_list])
        return info

    def set_electron_temperatures(self, temperatures):
        """Electron temperature (eV) of every resident frame (temperature-dependent models only).
        `set_frames` takes them from `atoms.info["etemperature"]`; coordinate updates keep them."""
        T = np.ascontiguousarray(temperatures, dtype=np.float64).ravel()
        self._check(self._lib.ta_set_electron_temperatures(self._handle, len(T), _lib.as_dp(T)))
        self._etemperatures = T

    def _td_results(self, out: dict) -> dict:
        """Temperature-dependent models: `out` holds F (the library's energy, and per atom when
        fetched); add U as `energy` / `atomic`, F as `free_energy` / `free_energy_atomic` and S as
        `eentropy` / `eentropy_atomic`."""
        N, F = int(self.info.n_atoms), int(self.info.n_frames)
        u, s, ua, sa = np.empty(F), np.empty(F), np.empty(N), np.empty(N)
        self._check(self._lib.ta_get_td_results(self._handle, _lib.as_dp(u), _lib.as_dp(s), _lib.as_dp(ua),
                                                _lib.as_dp(sa)))
        out = dict(out)
        out["free_energy"] = out["energy"]
        if out.get("atomic") is not None:
            out["free_energy_atomic"] = out["atomic"]
        out["energy"], out["atomic"] = u, ua
        out["eentropy"], out["eentropy_atomic"] = s, sa
        return out

    def set_nn_tables(self, on: bool):
        """nn pair functions of an EAM / ADP model through the library's Hermite tables (default for
        inference) or evaluated exactly for every pair (`ta_set_nn_tables`). Set it before
        `set_frames`."""
        self._check(self._lib.ta_set_nn_tables(self._handle, 1 if on else 0))

    def set_filter_tables(self, on: bool = True, knots=None):
        """The `nn` filter network of a GRAP model through a device-built cubic Hermite table of `knots`
        knots (None: the library default, `grap.FILTER_TABLE_KNOTS`) instead of evaluated for every pair
        (`ta_set_filter_tables`). For inference, off by default; the resident batch stays. A weight gradient
        or a training step on this engine turns it off for good; models without a filter network ignore it."""
        n = 0 if knots is None else int(knots)
        if knots is not None and n == 0:
            raise ValueError("set_filter_tables: knots=None selects the default; 0 is not a knot count")
        self._check(self._lib.ta_set_filter_tables(self._handle, 1 if on else 0, n))

    @property
    def filter_table_knots(self) -> int:
        """Knots of the filter table in use; 0 while the filter network is evaluated exactly."""
        n = C.c_int32(0)
        self._check(self._lib.ta_filter_table_knots(self._handle, C.byref(n)))
        return int(n.value)

    def set_skin(self, skin: float):
        """Verlet skin in Angstrom for the lists built from now on (0 = exact list)."""
        self._check(self._lib.ta_set_skin(self._handle, float(skin)))

    def update_positions(self, positions, cells=None) -> bool:
        """New coordinates for the resident frames (all atoms of the batch, in order; `cells`
        [n_frames, 3, 3] or None = unchanged). Returns True when the neighbour list was rebuilt."""
        pos = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 3)
        if len(pos) != int(self.info.n_atoms):
            raise ValueError("positions for every atom of the resident batch are needed")
        null = C.POINTER(C.c_double)()
        cptr = null
        if cells is not None:
            cells = np.ascontiguousarray(cells, dtype=np.float64).reshape(-1, 3, 3)
            if len(cells) != int(self.info.n_frames):
                raise ValueError("one cell per resident frame")
            cptr = _lib.as_dp(cells)
        rebuilt = C.c_int32(0)
        self._check(self._lib.ta_update_positions(self._handle, _lib.as_dp(pos), cptr, C.byref(rebuilt)))
        self.batch_generation += 1
        if cells is not None:  # only once the call has succeeded
            self._volumes = np.abs(np.linalg.det(cells))
        if rebuilt.value:
            # a rebuilt list has new pair / triple counts: scripts derive bytes per evaluation from them
            n_pairs, n_triples, nnl = C.c_int64(0), C.c_int64(0), C.c_int32(0)
            self._check(self._lib.ta_list_sizes(self._handle, C.byref(n_pairs), C.byref(n_triples), C.byref(nnl)))
            self.info.n_pairs, self.info.n_triples, self.info.nnl_max = n_pairs.value, n_triples.value, nnl.value
        return bool(rebuilt.value)

    def _view_array(self, ptr, shape):
        """numpy array over library memory at `ptr`; the staging buffer does not move between steps, so the
        wrapper is made once per (address, shape)."""
        addr = C.cast(ptr, C.c_void_p).value
        if not addr:
            return None
        key = (addr, shape)
        arr = self._view_cache.get(key)
        if arr is None:
            if len(self._view_cache) > 16:
                self._view_cache.clear()
            n = int(np.prod(shape))
            arr = np.frombuffer((C.c_double * n).from_address(addr), dtype=np.float64).reshape(shape)
            self._view_cache[key] = arr
        return arr

    def step(self, positions, want: int, cells=None, view=False) -> dict:
        """One MD step of the resident batch in one library call (`ta_step`): new coordinates in,
        evaluation, results out. Same result dict as `fetch`; the output arrays are reused from call to
        call (copy what must outlive the next step). `view=True` (`ta_step_view`): the arrays ARE the
        library's page-locked staging memory the device wrote, valid until the next call on this engine
        (no copy out of it: 128 KB per step for 4000 atoms)."""
        pos = positions if (type(positions) is np.ndarray and positions.dtype == np.float64 and
                            positions.flags.c_contiguous) else np.ascontiguousarray(positions, dtype=np.float64)
        N, F = int(self.info.n_atoms), int(self.info.n_frames)
        if pos.size != 3 * N:
            raise ValueError("positions for every atom of the resident batch are needed")
        st = self.__dict__.get("_step_state")
        if st is None:   # ctypes objects of the call, made once
            null = C.POINTER(C.c_double)()
            ptrs = tuple(C.POINTER(C.c_double)() for _ in range(4))
            rebuilt = C.c_int32(0)
            st = self._step_state = (null, ptrs, tuple(C.byref(p) for p in ptrs), rebuilt, C.byref(rebuilt))
            self._view_cache = {}
        null, ptrs, refs, rebuilt, rebuilt_ref = st
        cptr = null
        if cells is not None:
            cells = np.ascontiguousarray(cells, dtype=np.float64).reshape(-1, 3, 3)
            if len(cells) != F:
                raise ValueError("one cell per resident frame")
            cptr = _lib.as_dp(cells)
        want = int(want)
        want_f = bool(want & (_lib.TA_WANT_FORCES | _lib.TA_WANT_VIRIAL))
        if view:
            rc = self._lib.ta_step_view(self._handle, pos.ctypes.data_as(_lib._dp), cptr, want, refs[0], refs[1],
                                        refs[2], refs[3], rebuilt_ref)
            if rc:
                self._check(rc)
            energy = self._view_array(ptrs[0], (F,))
            if energy is None:
                energy = np.empty(0)
            forces, virial = self._view_array(ptrs[1], (N, 3)), self._view_array(ptrs[2], (F, 3, 3))
            atomic = self._view_array(ptrs[3], (N,))
        else:
            buf = getattr(self, "_step_buf", None)
            if buf is None or buf[0] != (N, F):
                buf = ((N, F), np.empty(F), np.empty((N, 3)), np.empty((F, 3, 3)), np.empty(N))
                self._step_buf = buf
            _, energy, forces, virial, atomic = buf
            self._check(self._lib.ta_step(
                self._handle, _lib.as_dp(pos), cptr, want, _lib.as_dp(energy),
                _lib.as_dp(forces) if want_f else null, _lib.as_dp(virial) if want_f else null,
                _lib.as_dp(atomic) if want & _lib.TA_WANT_ATOMIC else null, rebuilt_ref))
        self.batch_generation += 1
        if cells is not None:
            self._volumes = np.abs(np.linalg.det(cells))
        if rebuilt.value:
            n_pairs, n_triples, nnl = C.c_int64(0), C.c_int64(0), C.c_int32(0)
            self._check(self._lib.ta_list_sizes(self._handle, C.byref(n_pairs), C.byref(n_triples), C.byref(nnl)))
            self.info.n_pairs, self.info.n_triples, self.info.nnl_max = n_pairs.value, n_triples.value, nnl.value
        out = {"energy": energy}
        if want_f and forces is not None:
            out["forces"], out["virial"] = forces, virial
        if want & _lib.TA_WANT_ATOMIC and atomic is not None:
            out["atomic"] = atomic
        if self.finite_temperature:
            out = self._td_results(out)
        return out

    # -- device-resident MD loop -------------------------------------------------------------
    # what this side keeps of every sampler's setting, by the setter the library's messages name: (attribute, its value
    # while the sampler is off)
    _MD_OFF = {"ta_md_set_sampling": ("_md_lags", 0), "ta_md_set_rdf": ("_md_bins", 0), "ta_md_set_adf": ("_md_adf_bins", 0),
               "ta_md_set_order": ("_md_order_bins", 0), "ta_md_set_clusters": ("_md_cluster", (0, 1)),
               "ta_md_set_cna": ("_md_cna", 0), "ta_md_set_sq": ("_md_sq", (0, 1, False)),
               "ta_md_set_flux": ("_md_flux_lags", 0)}

    def _need_batch(self, who):
        if self.info is None:
            raise ValueError(f"{who}: no resident batch (call set_frames first)")

    def _md_by_element(self):
        """Atoms per frame and element of the resident batch, int64 [n_frames, n_elements]."""
        E = self._n_elements
        return np.array([np.bincount(fr.species, minlength=E)[:E] for fr in self._frames], dtype=np.int64).reshape(-1, E)

    def _md_pair_cutoffs(self, who, name, r, default):
        """The cutoff argument `name` = `r` of setter `who`, one distance (None: `default`) or an [n_elements, n_elements]
        matrix, as the library takes it: (the distance or the matrix's largest, pointer to the matrix or NULL)."""
        E = self._n_elements
        if r is None:
            r = default
        if np.ndim(r) == 0:
            return float(r), C.POINTER(C.c_double)()
        m = np.ascontiguousarray(r, dtype=np.float64)
        if m.shape != (E, E):
            raise ValueError(f"{who}: {name} must be one distance or [{E}, {E}] (n_elements of the model)")
        return float(m.max()), _lib.as_dp(m)

    def md_init(self, masses=None, velocities=None):
        """Masses (amu; default: `atoms.atomic_masses` by atomic number) and velocities
        (A / (A sqrt(amu / eV)), ASE's unit; default 0) of every atom of the resident batch, for
        `md_run` (`ta_md_init`). `set_frames` drops them; `update_positions` / `step` keep them."""
        self._need_batch("md_init")
        N = int(self.info.n_atoms)
        if masses is None:
            from .atoms import atomic_masses
            masses = np.array([atomic_masses[z] for z in self._numbers], dtype=np.float64)
        m = np.ascontiguousarray(masses, dtype=np.float64).ravel()
        if len(m) != N:
            raise ValueError("md_init: one mass for every atom of the resident batch is needed")
        vptr = C.POINTER(C.c_double)()
        if velocities is not None:
            v = np.ascontiguousarray(velocities, dtype=np.float64)
            if v.size != 3 * N:
                raise ValueError("md_init: velocities [n_atoms, 3] for every atom of the resident batch are needed")
            vptr = _lib.as_dp(v)
        rc = self._lib.ta_md_init(self._handle, _lib.as_dp(m), vptr)
        if rc == _lib.TA_ERR_NOMEM:   # no room for what a setting needs: the library switched that setting off
            msg = self._lib.ta_last_error(self._handle) or b""
            for setter, (attr, off) in self._MD_OFF.items():
                if setter.encode() in msg:
                    setattr(self, attr, off)
        elif rc == _lib.TA_ERR_INVALID and b"ta_md_set_sq" in (self._lib.ta_last_error(self._handle) or b""):
            self._md_sq = (0, 1, False)   # (a batch without wave vectors: the library switched the feature off)
        self._check(rc)

    def md_set_thermostat(self, kT=0.0, tau=0.0):
        """Berendsen thermostat of `md_run`: target kT (eV) and time constant (ASE time units);
        kT <= 0 switches it off (the default)."""
        self._check(self._lib.ta_md_set_thermostat(self._handle, float(kT), float(tau)))

    def md_set_langevin(self, kT=0.0, friction=0.0, seed=0):
        """Langevin thermostat of `md_run` (`ta_md_set_langevin`): bath kT (eV, >= 0), friction (1 / ASE time
        unit; 0 switches it off, the default) and the seed (0 .. 2^64 - 1) of the counter-based noise. It and
        the Berendsen thermostat exclude each other: switch the one that is on off first."""
        seed = int(seed)
        if not 0 <= seed < 2 ** 64:
            raise ValueError("md_set_langevin: the seed must fit an unsigned 64-bit integer")
        self._check(self._lib.ta_md_set_langevin(self._handle, float(kT), float(friction), seed))

    def md_set_sampling(self, n_lags=0, sample_every=1):
        """Time correlations inside `md_run` (`ta_md_set_sampling`): with `n_lags` = L (1 .. 4096) the loop keeps
        the last L sampled whole-step states (x, v) in a ring on the device, samples every step t (counted since
        `md_init`) with t % `sample_every` == 0, and at every sample adds the velocity autocorrelation and the
        mean-square displacement at all L lags, per frame and per element, onto accumulators that stay on the
        device (`md_correlations`, `md_samples`). `n_lags` = 0 switches it off (the default) and frees the ring.
        Needs `md_init`; every call starts an empty ring and zero accumulators, as `md_init` does. The setting
        stays on across `set_frames`. No centre-of-mass correction is made. `md_run` refuses to sample under the
        barostat. The ring takes 2 x L x n_atoms x 24 bytes of device memory."""
        p = _lib.MdSamplingParams(int(n_lags), int(sample_every))
        rc = self._lib.ta_md_set_sampling(self._handle, C.byref(p))
        if rc == _lib.TA_ERR_NOMEM:   # (no room for the rings: the library switched sampling off)
            self._md_lags = 0
        self._check(rc)
        self._md_lags = int(n_lags)

    def _md_corr_shape(self, who):
        self._need_batch(who)
        return int(self.info.n_frames), self._n_elements, max(self._md_lags, 1)

    def md_correlations(self):
        """What the loop has accumulated since sampling was switched on (`ta_md_get_correlations`), a dict:
        `vacf_sum`, `msd_sum` [n_frames, n_elements, n_lags]: sums over time origins and over the atoms of a frame
        with that species of v(n) . v(n - k) and |x(n) - x(n - k)|^2 (positions unwrapped, no centre-of-mass
        correction: under Langevin the diffusion of the centre of mass is included);
        `n_origins` [n_lags] = max(0, n_samples - k); `counts` [n_frames, n_elements] atoms per frame and element;
        `vacf`, `msd`: the sums over n_origins x counts, NaN where that is 0;
        `n_samples`, `sample_every`, `last_step` (absolute step of the newest sample, -1: none)."""
        F, E, L = self._md_corr_shape("md_correlations")
        vs, xs = np.zeros((F, E, L)), np.zeros((F, E, L))
        info = (C.c_int64 * 4)()
        self._check(self._lib.ta_md_get_correlations(self._handle, _lib.as_dp(vs), _lib.as_dp(xs), info))
        n_samples = int(info[0])
        n_origins = np.maximum(0, n_samples - np.arange(L)).astype(np.int64)
        counts = self._md_by_element()
        den = (counts[:, :, None] * n_origins[None, None, :]).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            vacf = np.where(den > 0, vs / den, np.nan)
            msd = np.where(den > 0, xs / den, np.nan)
        return {"vacf": vacf, "msd": msd, "vacf_sum": vs, "msd_sum": xs, "n_origins": n_origins, "counts": counts,
                "n_samples": n_samples, "sample_every": int(info[2]), "last_step": int(info[3])}

    def md_samples(self, n=None):
        """The last `n` sampled states, oldest first (`ta_md_get_samples`; default: all the ring holds,
        min(n_samples, n_lags)): a dict `x`, `v` [n, n_atoms, 3] and `steps` [n] (absolute steps). The first way
        to trajectory frames that does not cut a run."""
        F, E, L = self._md_corr_shape("md_samples")
        null = C.POINTER(C.c_double)()
        if n is None:
            info = (C.c_int64 * 4)()
            self._check(self._lib.ta_md_get_samples(self._handle, 0, 0, null, null, None))   # (its own refusals)
            self._check(self._lib.ta_md_get_correlations(self._handle, null, null, info))
            n = min(int(info[0]), int(info[1]))
        n = int(n)
        if n < 0:
            raise ValueError("md_samples: n must be >= 0")
        N = int(self.info.n_atoms)
        x, v = np.empty((max(n, 1), N, 3)), np.empty((max(n, 1), N, 3))
        steps = np.zeros(max(n, 1), dtype=np.int64)
        self._check(self._lib.ta_md_get_samples(self._handle, 0, n, _lib.as_dp(x), _lib.as_dp(v),
                                                steps.ctypes.data_as(C.POINTER(C.c_int64))))
        return {"x": x[:n][::-1].copy(), "v": v[:n][::-1].copy(), "steps": steps[:n][::-1].copy()}

    def md_set_rdf(self, n_bins=0, r_max=None, sample_every=1):
        """Partial pair distributions inside `md_run` (`ta_md_set_rdf`): with `n_bins` = B (1 .. 4096) the loop
        counts, at every step t (counted since `md_init`) with t % `sample_every` == 0, every directed pair of the
        resident neighbour list below `r_max` (default: the model's cutoff max(rcut, acut), which is also the
        largest value allowed) into integer histograms of B bins per frame and pair of elements, which stay on
        the device (`md_rdf`). `n_bins` = 0 switches it off (the default) and frees them. Needs `md_init`; every
        call starts from zero counts, as `md_init` does. The setting stays on across `set_frames`. Independent of
        `md_set_sampling`. `md_run` refuses it under the barostat."""
        if r_max is None:
            r_max = self._md_cutoff
        p = _lib.MdRdfParams(float(r_max), int(n_bins), int(sample_every))
        rc = self._lib.ta_md_set_rdf(self._handle, C.byref(p))
        if rc == _lib.TA_ERR_NOMEM:   # (no room for the counts: the library switched the feature off)
            self._md_bins = 0
        self._check(rc)
        self._md_bins = int(n_bins)

    @property
    def md_rdf_bins(self):
        """Bins of the pair distributions `md_set_rdf` switched on, 0 while they are off."""
        return self._md_bins

    def md_rdf(self):
        """What the loop has counted since `md_set_rdf` (`ta_md_get_rdf`), a dict: `counts` int64 [n_frames,
        n_elements, n_elements, n_bins], counts[f, a, b, k] = directed pairs of a centre of species a and a
        neighbour of species b in frame f with floor(r / (r_max / n_bins)) == k, summed over the samples;
        `n_samples`, `r_max`, `sample_every`, `last_step` (absolute step of the newest sample, -1: none);
        `n_by_element` [n_frames, n_elements] atoms per frame and element, `volumes` [n_frames] and `pbc`
        [n_frames, 3] of the resident frames: what `md.rdf` normalises the counts with."""
        self._need_batch("md_rdf")
        F, E, B = int(self.info.n_frames), self._n_elements, max(self._md_bins, 1)
        counts = np.zeros((F, E, E, B), dtype=np.int64)
        info = (C.c_int64 * 4)()
        r_max = C.c_double(0.0)
        self._check(self._lib.ta_md_get_rdf(self._handle, counts.ctypes.data_as(C.POINTER(C.c_int64)), info,
                                            C.byref(r_max)))
        n_by_element = self._md_by_element()
        return {"counts": counts, "n_samples": int(info[0]), "r_max": float(r_max.value),
                "sample_every": int(info[2]), "last_step": int(info[3]), "n_by_element": n_by_element,
                "volumes": self._volumes.copy(), "pbc": np.array([fr.pbc != 0 for fr in self._frames]).reshape(F, 3)}

    def md_set_adf(self, n_bins=0, r_bond=None, sample_every=1):
        """Bond-angle distributions inside `md_run` (`ta_md_set_adf`): with `n_bins` = B (1 .. 4096) the loop
        counts, at every step t (counted since `md_init`) with t % `sample_every` == 0, for every centre the angle
        between every unordered pair of its neighbours below the bond cutoff `r_bond` into integer histograms of B
        bins over [0, pi] per frame, species of the centre and unordered pair of species of the two neighbours,
        which stay on the device (`md_adf`). `r_bond`: one distance, or a symmetric [n_elements, n_elements]
        matrix of cutoffs per pair of elements (centre, neighbour); None: the model's cutoff max(rcut, acut), which
        is also the largest value allowed. `n_bins` = 0 switches it off (the default) and frees them. Needs
        `md_init`; every call starts from zero counts, as `md_init` does. The setting stays on across
        `set_frames`. Independent of `md_set_sampling` and `md_set_rdf`; runs under the barostat too."""
        scalar, pairs = self._md_pair_cutoffs("md_set_adf", "r_bond", r_bond, self._md_cutoff)
        p = _lib.MdAdfParams(scalar, int(n_bins), int(sample_every))
        rc = self._lib.ta_md_set_adf(self._handle, C.byref(p), pairs)
        if rc == _lib.TA_ERR_NOMEM:   # (no room for the counts: the library switched the feature off)
            self._md_adf_bins = 0
        self._check(rc)
        self._md_adf_bins = int(n_bins)

    @property
    def md_adf_bins(self):
        """Bins of the bond-angle distributions `md_set_adf` switched on, 0 while they are off."""
        return self._md_adf_bins

    def md_adf(self):
        """What the loop has counted since `md_set_adf` (`ta_md_get_adf`), a dict: `counts` int64 [n_frames,
        n_elements, P, n_bins], counts[f, a, p, k] = triples of a centre of species a in frame f and two of its
        neighbours of species `pairs[p]` = (b, c), b <= c, with min(n_bins - 1, floor(theta / (pi / n_bins))) == k,
        summed over the samples; `pairs`: the P = n_elements (n_elements + 1) / 2 tuples (b, c) in the order of p;
        `r_bond` [n_elements, n_elements]: the cutoffs in use; `n_samples`, `n_bins`, `sample_every`, `last_step`
        (absolute step of the newest sample, -1: none). `md.adf` normalises the counts."""
        self._need_batch("md_adf")
        F, E, B = int(self.info.n_frames), self._n_elements, max(self._md_adf_bins, 1)
        pairs = [(b, c) for b in range(E) for c in range(b, E)]
        counts = np.zeros((F, E, len(pairs), B), dtype=np.int64)
        info = (C.c_int64 * 4)()
        r_bond = np.zeros((E, E))
        self._check(self._lib.ta_md_get_adf(self._handle, counts.ctypes.data_as(C.POINTER(C.c_int64)), info,
                                            _lib.as_dp(r_bond)))
        return {"counts": counts, "n_samples": int(info[0]), "n_bins": int(info[1]), "sample_every": int(info[2]),
                "last_step": int(info[3]), "r_bond": r_bond, "pairs": pairs}

    def md_set_order(self, degrees=(4, 6), r_bond=None, n_bins=0, sample_every=1, solid=(6, 0.5)):
        """Bond-orientational order inside `md_run` (`ta_md_set_order`): with `n_bins` = B (1 .. 4096) the loop
        evaluates, at every step t (counted since `md_init`) with t % `sample_every` == 0, for every atom the
        Steinhardt parameters q_l of the `degrees` l (up to 4 of them, 1 .. 12, any order), their neighbour average
        qbar_l (Lechner and Dellago) and the number n_conn of solid bonds: neighbours j with
        Re sum_m q_lm(i) conj(q_lm(j)) / (|q_l(i)| |q_l(j)|) > c for `solid` = (l, c), l one of the degrees, c inside
        (-1, 1). The neighbours are those below the bond cutoff `r_bond`, as for `md_set_adf`: one distance, or a
        symmetric [n_elements, n_elements] matrix; None: the model's cutoff max(rcut, acut), the largest value
        allowed. q_l and qbar_l are counted into integer histograms of B bins over [0, 1] and n_conn into one of
        0 .. 31, per frame and species of the atom (`md_order`); the per-atom values of the newest sample stay on
        the device as well (`md_order_atoms`). `n_bins` = 0 switches it off (the default) and frees the buffers.
        Needs `md_init`; every call starts from zero counts, as `md_init` does. The setting stays on across
        `set_frames`. Independent of `md_set_sampling`, `md_set_rdf` and `md_set_adf`; runs under the barostat too.
        `md_run(0, dt)` samples the resident state once: `md_init`, `md_set_order`, `md_run(0, dt)` analyses a
        static structure."""
        scalar, pairs = self._md_pair_cutoffs("md_set_order", "r_bond", r_bond, self._md_cutoff)
        degrees = [int(l) for l in np.atleast_1d(degrees)]
        solid_degree, threshold = solid
        p = _lib.MdOrderParams(scalar, float(threshold), int(n_bins), int(sample_every), len(degrees),   # (the library
                               (C.c_int32 * 4)(*degrees[:4]), int(solid_degree))                         # counts them)
        rc = self._lib.ta_md_set_order(self._handle, C.byref(p), pairs)
        if rc == _lib.TA_ERR_NOMEM:   # (no room for the buffers: the library switched the feature off)
            self._md_order_bins = 0
        self._check(rc)
        self._md_order_bins = int(n_bins)
        if n_bins:
            self._md_order_degrees, self._md_order_solid = tuple(degrees), (int(solid_degree), float(threshold))

    @property
    def md_order_bins(self):
        """Bins of the order-parameter histograms `md_set_order` switched on, 0 while the feature is off."""
        return self._md_order_bins

    def md_order(self):
        """What the loop has counted since `md_set_order` (`ta_md_get_order`), a dict: `hist_q`, `hist_qbar` int64
        [n_frames, n_elements, n_degrees, n_bins], hist_q[f, a, d, k] = atoms of species a in frame f with
        min(n_bins - 1, floor(q_l n_bins)) == k for l = `degrees`[d], summed over the samples, hist_qbar likewise
        for the neighbour average; `hist_conn` int64 [n_frames, n_elements, 32]: atoms by min(n_conn, 31);
        `degrees`, `solid` (degree, threshold), `r_bond` [n_elements, n_elements]: the setting in use;
        `n_samples`, `n_bins`, `sample_every`, `last_step` (absolute step of the newest sample, -1: none);
        `n_by_element` [n_frames, n_elements] atoms per frame and element. `md.order_distribution` and
        `md.solid_fraction` normalise the counts."""
        self._need_batch("md_order")
        F, E, B = int(self.info.n_frames), self._n_elements, max(self._md_order_bins, 1)
        D = max(len(self._md_order_degrees), 1)
        hist_q, hist_qbar = np.zeros((F, E, D, B), dtype=np.int64), np.zeros((F, E, D, B), dtype=np.int64)
        hist_conn = np.zeros((F, E, _lib.TA_MD_ORDER_MAX_CONN + 1), dtype=np.int64)
        info = (C.c_int64 * 4)()
        r_bond = np.zeros((E, E))
        ip = C.POINTER(C.c_int64)
        self._check(self._lib.ta_md_get_order(self._handle, hist_q.ctypes.data_as(ip), hist_qbar.ctypes.data_as(ip),
                                              hist_conn.ctypes.data_as(ip), info, _lib.as_dp(r_bond)))
        n_by_element = self._md_by_element()
        return {"hist_q": hist_q, "hist_qbar": hist_qbar, "hist_conn": hist_conn, "degrees": self._md_order_degrees,
                "solid": self._md_order_solid, "r_bond": r_bond, "n_samples": int(info[0]), "n_bins": int(info[1]),
                "sample_every": int(info[2]), "last_step": int(info[3]), "n_by_element": n_by_element}

    def md_order_atoms(self):
        """The order parameters of every atom in the newest sampled state (`ta_md_get_order_atoms`), a dict: `q`,
        `qbar` [n_atoms, n_degrees]; `n_bonds`, `n_conn` int32 [n_atoms]: neighbours below the bond cutoff and solid
        bonds among them; `qlm` complex [n_atoms, sum (l + 1)]: q_lm degree by degree in the order of `degrees`,
        m = 0 .. l; `step`: the absolute step of that state. Costs a host sync and no list rebuild. Refused until
        the first sample has been taken."""
        self._need_batch("md_order_atoms")
        N, D = int(self.info.n_atoms), max(len(self._md_order_degrees), 1)
        M = max(sum(l + 1 for l in self._md_order_degrees), 1)
        q, qbar, qlm = np.zeros((N, D)), np.zeros((N, D)), np.zeros((N, M, 2))
        n_bonds, n_conn = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
        info = (C.c_int64 * 4)()
        self._check(self._lib.ta_md_get_order_atoms(self._handle, _lib.as_dp(q), _lib.as_dp(qbar),
                                                    n_bonds.ctypes.data_as(C.POINTER(C.c_int32)),
                                                    n_conn.ctypes.data_as(C.POINTER(C.c_int32)), _lib.as_dp(qlm)))
        self._check(self._lib.ta_md_get_order(self._handle, None, None, None, info, C.POINTER(C.c_double)()))
        return {"q": q, "qbar": qbar, "n_bonds": n_bonds, "n_conn": n_conn, "qlm": qlm[..., 0] + 1j * qlm[..., 1],
                "step": int(info[3])}

    def md_set_clusters(self, r_link=None, n_min=0, species=None, n_bins=0, n_series=1, sample_every=1):
        """Clusters of solid or selected atoms inside `md_run` (`ta_md_set_clusters`): with `n_bins` = B (1 .. 4096)
        the loop finds, at every step t (counted since `md_init`) with t % `sample_every` == 0, the connected
        components of the selected atoms on the device. An atom is selected when its element is among `species`
        (element symbols or indices; None: all) and, with `n_min` > 0, it has at least `n_min` solid bonds (the
        n_conn of `md_set_order` for the same state: that feature must then be on, with a `sample_every` that
        divides this one, and switched on first). Two selected atoms are linked when they are closer than `r_link`:
        one distance, or a symmetric [n_elements, n_elements] matrix; None: the model's cutoff max(rcut, acut), the
        largest value allowed. A cluster's size counts atoms, not images; its label is the smallest index of its
        members in the batch. Every result is an integer and a function of the state alone. The loop counts the
        clusters by size into a histogram of B bins per frame (the last one collects sizes >= B) and keeps the last
        `n_series` rows {selected atoms, clusters, size of the largest, its label} per frame (`md_clusters`); label
        and size of every atom of the newest sample stay on the device as well (`md_cluster_atoms`). `n_bins` = 0
        switches it off (the default) and frees the buffers. Needs `md_init`; every call starts from zero, as
        `md_init` does. The setting stays on across `set_frames`. Runs under the barostat and every thermostat.
        `md_run(0, dt)` samples the resident state once."""
        E = self._n_elements
        # (for NaN the library takes the model's cutoff)
        scalar, pairs = self._md_pair_cutoffs("md_set_clusters", "r_link", r_link, float("nan"))
        if species is None:
            mask = (1 << E) - 1
        else:
            mask, names = 0, list(self._clf.elements)
            for sp in ([species] if isinstance(species, (str, int, np.integer)) else list(species)):
                if isinstance(sp, str):
                    if sp not in names:
                        raise ValueError(f"md_set_clusters: {sp!r} is not an element of the model ({names})")
                    sp = names.index(sp)
                if not 0 <= int(sp) < E:
                    raise ValueError(f"md_set_clusters: species index {sp} is outside 0 .. {E - 1}")
                mask |= 1 << int(sp)
        p = _lib.MdClusterParams(scalar, int(n_min), int(mask), int(n_bins), int(n_series), int(sample_every))
        rc = self._lib.ta_md_set_clusters(self._handle, C.byref(p), pairs)
        if rc == _lib.TA_ERR_NOMEM:   # (no room for the buffers: the library switched the feature off)
            self._md_cluster = (0, 1)
        self._check(rc)
        self._md_cluster = (int(n_bins), int(n_series) if n_bins else 1)

    @property
    def md_cluster_bins(self):
        """Bins of the cluster-size histogram `md_set_clusters` switched on, 0 while the feature is off."""
        return self._md_cluster[0]

    def md_clusters(self):
        """What the loop has found since `md_set_clusters` (`ta_md_get_clusters`), a dict: `hist` int64 [n_frames,
        n_bins], hist[f, k] = clusters of frame f with min(size, n_bins) - 1 == k, summed over the samples; `series`
        int64 [rows, n_frames, 4]: {selected atoms, clusters, size of the largest cluster, its label (-1: nothing
        selected)} of the newest `rows` = min(n_samples, n_series) samples, oldest first, and `steps` int64 [rows],
        their absolute steps; `n_samples`, `n_bins`, `sample_every`, `last_step` (absolute step of the newest sample,
        -1: none), `rows`, `n_series`; `r_link` [n_elements, n_elements]: the cutoffs in use.
        `md.largest_cluster` and `md.cluster_size_distribution` read them."""
        self._need_batch("md_clusters")
        F, E = int(self.info.n_frames), self._n_elements
        B, T = max(self._md_cluster[0], 1), max(self._md_cluster[1], 1)
        ip = C.POINTER(C.c_int64)
        info = (C.c_int64 * 6)()
        self._check(self._lib.ta_md_get_clusters(self._handle, None, None, None, info, C.POINTER(C.c_double)()))
        rows = int(info[4])
        hist = np.zeros((F, B), dtype=np.int64)
        series, steps = np.zeros((max(rows, 1), F, 4), dtype=np.int64), np.zeros(max(rows, 1), dtype=np.int64)
        r_link = np.zeros((E, E))
        self._check(self._lib.ta_md_get_clusters(self._handle, hist.ctypes.data_as(ip), series.ctypes.data_as(ip),
                                                 steps.ctypes.data_as(ip), info, _lib.as_dp(r_link)))
        return {"hist": hist, "series": series[:rows], "steps": steps[:rows], "n_samples": int(info[0]),
                "n_bins": int(info[1]), "sample_every": int(info[2]), "last_step": int(info[3]), "rows": rows,
                "n_series": int(info[5]), "r_link": r_link}

    def md_cluster_atoms(self):
        """Cluster of every atom in the newest sampled state (`ta_md_get_cluster_atoms`), a dict: `label` int32
        [n_atoms], the smallest index of the atom's cluster in the batch, -1 for an atom that is not selected;
        `size` int32 [n_atoms], the atoms of that cluster, 0 likewise; `step`: the absolute step of that state. Costs
        a host sync and no list rebuild. Refused until the first sample has been taken."""
        self._need_batch("md_cluster_atoms")
        N = int(self.info.n_atoms)
        label, size = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
        info = (C.c_int64 * 6)()
        self._check(self._lib.ta_md_get_cluster_atoms(self._handle, label.ctypes.data_as(C.POINTER(C.c_int32)),
                                                      size.ctypes.data_as(C.POINTER(C.c_int32))))
        self._check(self._lib.ta_md_get_clusters(self._handle, None, None, None, info, C.POINTER(C.c_double)()))
        return {"label": label, "size": size, "step": int(info[3])}

    def md_set_cna(self, mode="adaptive", r_cut=None, r_max=None, n_series=1, sample_every=1):
        """Common neighbour analysis inside `md_run` (`ta_md_set_cna`): with `n_series` = T >= 1 the loop gives, at every
        step t (counted since `md_init`) with t % `sample_every` == 0, every atom its lattice type on the device: 0
        other, 1 fcc, 2 hcp, 3 bcc, 4 ico (`md.CNA_NAMES`, OVITO's numbering). `mode` "adaptive" (OVITO's default,
        Stukowski 2012) takes the 12, then the 14 nearest of the list entries within `r_max` (None: the model's cutoff
        max(rcut, acut), the largest value allowed) and a bond cutoff from their mean distance; "fixed" (LAMMPS
        `compute cna/atom`) takes every neighbour within `r_cut`, which is the bond cutoff too. Every result but
        `r_local` is an integer and a function of the state alone. The loop counts the atoms per frame, species and
        type and keeps the last `n_series` rows of the counts per frame (`md_cna`); type and bond cutoff of every atom
        of the newest sample stay on the device as well (`md_cna_atoms`). `n_series` = 0 switches it off (the default)
        and frees the buffers. Needs `md_init`; every call starts from zero, as `md_init` does. The setting stays on
        across `set_frames`. Runs under the barostat and every thermostat. `md_run(0, dt)` analyses the resident state
        once."""
        modes = {"adaptive": _lib.TA_MD_CNA_ADAPTIVE, "fixed": _lib.TA_MD_CNA_FIXED}
        if isinstance(mode, str):
            if mode not in modes:
                raise ValueError(f"md_set_cna: mode must be 'adaptive' or 'fixed', not {mode!r}")
            mode = modes[mode]
        if int(mode) == _lib.TA_MD_CNA_FIXED and r_cut is None and n_series:
            raise ValueError("md_set_cna: the fixed mode needs r_cut")
        p = _lib.MdCnaParams(0.0 if r_cut is None else float(r_cut), float("nan") if r_max is None else float(r_max),
                             int(mode), int(n_series), int(sample_every))
        rc = self._lib.ta_md_set_cna(self._handle, C.byref(p))
        if rc == _lib.TA_ERR_NOMEM:   # (no room for the buffers: the library switched the feature off)
            self._md_cna = 0
        self._check(rc)
        self._md_cna = int(n_series)

    @property
    def md_cna_series(self):
        """Rows of the series `md_set_cna` switched on, 0 while the feature is off."""
        return self._md_cna

    def md_cna(self):
        """What the loop has found since `md_set_cna` (`ta_md_get_cna`), a dict: `counts` int64 [n_frames, n_elements,
        5], the atoms of every frame and species with each type (`md.CNA_NAMES`), summed over the samples; `series`
        int64 [rows, n_frames, 5]: the atoms of every type of the newest `rows` = min(n_samples, n_series) samples,
        oldest first, and `steps` int64 [rows], their absolute steps; `n_samples`, `mode` ("adaptive" or "fixed"),
        `sample_every`, `last_step` (absolute step of the newest sample, -1: none), `rows`, `n_series`.
        `md.structure_fractions` normalises counts or series."""
        self._need_batch("md_cna")
        F, E, K = int(self.info.n_frames), self._n_elements, _lib.TA_MD_CNA_TYPES
        ip = C.POINTER(C.c_int64)
        info = (C.c_int64 * 6)()
        self._check(self._lib.ta_md_get_cna(self._handle, None, None, None, info))
        rows = int(info[4])
        counts = np.zeros((F, E, K), dtype=np.int64)
        series, steps = np.zeros((max(rows, 1), F, K), dtype=np.int64), np.zeros(max(rows, 1), dtype=np.int64)
        self._check(self._lib.ta_md_get_cna(self._handle, counts.ctypes.data_as(ip), series.ctypes.data_as(ip),
                                            steps.ctypes.data_as(ip), info))
        return {"counts": counts, "series": series[:rows], "steps": steps[:rows], "n_samples": int(info[0]),
                "mode": "fixed" if int(info[1]) == _lib.TA_MD_CNA_FIXED else "adaptive", "sample_every": int(info[2]),
                "last_step": int(info[3]), "rows": rows, "n_series": int(info[5])}

    def md_cna_atoms(self):
        """Lattice type of every atom in the newest sampled state (`ta_md_get_cna_atoms`), a dict: `structure` int32
        [n_atoms] (0 other, 1 fcc, 2 hcp, 3 bcc, 4 ico); `r_local` [n_atoms], the bond cutoff of the attempt that
        decided (adaptive mode; 0 with fewer than 12 candidates) or `r_cut` (fixed mode); `step`: the absolute step of
        that state. Costs a host sync and no list rebuild. Refused until the first sample has been taken."""
        self._need_batch("md_cna_atoms")
        N = int(self.info.n_atoms)
        structure, r_local = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.float64)
        info = (C.c_int64 * 6)()
        self._check(self._lib.ta_md_get_cna_atoms(self._handle, structure.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  _lib.as_dp(r_local)))
        self._check(self._lib.ta_md_get_cna(self._handle, None, None, None, info))
        return {"structure": structure, "r_local": r_local, "step": int(info[3])}

    def md_set_sq(self, miller=None, n_lags=1, sample_every=1, currents=False):
        """Structure factors inside `md_run` (`ta_md_set_sq`): `miller` int [Q, 3] (1 .. 4096 triples, |n_c| <= 64;
        `md.q_points` makes them) are the wave vectors q = 2 pi h^-1 n of every frame's own cell. At every step t
        (counted since `md_init`) with t % `sample_every` == 0 the loop sums rho_a(q) = sum_i exp(i q . x_i) per
        frame and element (with `currents` also j_a(q) = sum_i v_i exp(i q . x_i)) over ALL atoms, in fp64, keeps the
        last `n_lags` rows in a ring on the device and adds Re(rho_a(q; n) conj rho_b(q; n - k)) (with `currents`
        the longitudinal part and the trace of the current correlations too) at every lag k onto accumulators that
        stay on the device (`md_sq`, `md_sq_amplitudes`). `n_lags` = 1 is the static structure factor alone.
        `miller` None or empty switches it off (the default) and frees the buffers. Needs `md_init` and frames
        periodic in all three directions; every call starts an empty ring and zero accumulators, as `md_init`
        does. The setting stays on across `set_frames`. Independent of the other observables; `md_run` refuses it
        under the barostat. Device memory: the ring takes n_lags x n_frames x n_elements x Q x 16 bytes (x 4 with
        `currents`), each of the one (three) accumulators n_frames x n_elements^2 x n_lags x Q x 8 bytes: 64 frames
        of two elements at Q = 1000 and 256 lags are 524 MB per accumulator."""
        null = C.POINTER(C.c_int32)()
        if miller is None or np.size(miller) == 0:
            self._check(self._lib.ta_md_set_sq(self._handle, None, null))
            self._md_sq = (0, 1, False)
            return
        m = np.asarray(miller)
        if m.ndim != 2 or m.shape[1] != 3 or not np.issubdtype(m.dtype, np.integer):
            raise ValueError("md_set_sq: miller must be integers [n_q, 3]")
        if np.abs(m).max() > _lib.TA_MD_SQ_MAX_INDEX:
            raise ValueError(f"md_set_sq: the Miller indices must be within +-{_lib.TA_MD_SQ_MAX_INDEX}")
        if len(m) > _lib.TA_MD_SQ_MAX_Q:
            raise ValueError(f"md_set_sq: at most {_lib.TA_MD_SQ_MAX_Q} wave vectors")
        m = np.ascontiguousarray(m, dtype=np.int32)
        p = _lib.MdSqParams(len(m), int(n_lags), int(sample_every), int(bool(currents)))
        rc = self._lib.ta_md_set_sq(self._handle, C.byref(p), m.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc == _lib.TA_ERR_NOMEM:   # (no room: the library switched the feature off)
            self._md_sq = (0, 1, False)
        self._check(rc)
        self._md_sq = (len(m), int(n_lags), bool(currents))

    @property
    def md_sq_vectors(self):
        """Wave vectors per frame that `md_set_sq` switched on, 0 while the feature is off."""
        return self._md_sq[0]

    def md_sq(self):
        """What the loop has accumulated since `md_set_sq` (`ta_md_get_sq`), a dict: `a_rho` [n_frames, n_elements,
        n_elements, n_lags, n_q]: sums over the time origins of Re(rho_a(q; n) conj rho_b(q; n - k)); with currents
        `a_l` and `a_j` likewise for the longitudinal current and for the trace of the current tensor (None
        without); `miller` int32 [n_q, 3]; `q` [n_frames, n_q, 3] = 2 pi h^-1 n and `q_norm` [n_frames, n_q] for the
        resident cells; `n_origins` [n_lags] = max(0, n_samples - k); `n_by_element` [n_frames, n_elements];
        `n_samples`, `n_lags`, `sample_every`, `last_step` (absolute step of the newest sample, -1: none),
        `currents`, `chunk` (atoms per workgroup of the amplitude launch). `md.intermediate_scattering` and
        `md.structure_factor` normalise the sums."""
        self._need_batch("md_sq")
        F, E = int(self.info.n_frames), self._n_elements
        Q, L, cur = max(self._md_sq[0], 1), self._md_sq[1], self._md_sq[2]
        a_rho = np.zeros((F, E, E, L, Q))
        a_l, a_j = (np.zeros((F, E, E, L, Q)), np.zeros((F, E, E, L, Q))) if cur else (None, None)
        info = (C.c_int64 * 8)()
        miller = np.zeros((Q, 3), dtype=np.int32)
        null = C.POINTER(C.c_double)()
        self._check(self._lib.ta_md_get_sq(self._handle, _lib.as_dp(a_rho), _lib.as_dp(a_l) if cur else null,
                                           _lib.as_dp(a_j) if cur else null, info,
                                           miller.ctypes.data_as(C.POINTER(C.c_int32))))
        n_by_element = self._md_by_element()
        q = 2.0 * np.pi * np.einsum("fjc,qc->fqj", np.linalg.inv(self.md_cells()), miller.astype(np.float64))
        n_samples = int(info[0])
        return {"a_rho": a_rho, "a_l": a_l, "a_j": a_j, "miller": miller, "q": q, "q_norm": np.linalg.norm(q, axis=-1),
                "n_origins": np.maximum(0, n_samples - np.arange(L)).astype(np.int64), "n_by_element": n_by_element,
                "n_samples": n_samples, "n_lags": int(info[2]), "sample_every": int(info[3]), "last_step": int(info[4]),
                "currents": bool(info[5]), "chunk": int(info[6])}

    def md_sq_amplitudes(self, n=None):
        """The last `n` amplitude rows the ring holds, oldest first (`ta_md_get_sq_amplitudes`; default: all,
        min(n_samples, n_lags)): a dict `rho` complex [n, n_frames, n_elements, n_q], `cur` complex
        [n, n_frames, n_elements, n_q, 3] (None without currents) and `steps` [n] (absolute steps)."""
        self._need_batch("md_sq_amplitudes")
        null = C.POINTER(C.c_double)()
        if n is None:
            info = (C.c_int64 * 8)()
            self._check(self._lib.ta_md_get_sq_amplitudes(self._handle, 0, 0, null, null, None))   # (its own refusals)
            self._check(self._lib.ta_md_get_sq(self._handle, null, null, null, info, C.POINTER(C.c_int32)()))
            n = min(int(info[0]), int(info[2]))
        n = int(n)
        if n < 0:
            raise ValueError("md_sq_amplitudes: n must be >= 0")
        F, E = int(self.info.n_frames), self._n_elements
        Q, cur = max(self._md_sq[0], 1), self._md_sq[2]
        rho = np.zeros((max(n, 1), F, E, Q, 2))
        j = np.zeros((max(n, 1), F, E, Q, 3, 2)) if cur else None
        steps = np.zeros(max(n, 1), dtype=np.int64)
        self._check(self._lib.ta_md_get_sq_amplitudes(self._handle, 0, n, _lib.as_dp(rho), _lib.as_dp(j) if cur else null,
                                                      steps.ctypes.data_as(C.POINTER(C.c_int64))))
        rho = (rho[..., 0] + 1j * rho[..., 1])[:n][::-1].copy()
        if cur:
            j = (j[..., 0] + 1j * j[..., 1])[:n][::-1].copy()
        return {"rho": rho, "cur": j, "steps": steps[:n][::-1].copy()}

    def md_set_flux(self, n_lags=0, sample_every=1):
        """Heat current and pressure tensor inside `md_run` (`ta_md_set_flux`), the two Green-Kubo observables. At
        every step t (counted since `md_init`) with t % `sample_every` == 0 the loop makes, per frame and in fp64,
        the row {J_conv[3], J_pot[3], K[6], W[6]} (six components: xx yy zz yz xz xy) from the per-atom energies and
        per-pair gradients of the evaluation of that state: J_conv = sum_i (m_i |v_i|^2 / 2 + e_i) v_i,
        J_pot = - sum_p D_p (g_p . v_n), K_ab = sum_i m_i v_ia v_ib, W_ab the symmetrised virial, Pi = K - W = P V.
        It keeps the last `n_lags` rows in a ring on the device and adds J_a(n) J_a(n - k) (J = J_conv + J_pot) and
        Pi_ab(n) Pi_ab(n - k) at every lag k onto accumulators that stay on the device (`md_flux`, `md_flux_rows`).
        No centre-of-mass correction and no partial-enthalpy correction for mixtures is made. `n_lags` = 0 switches
        it off (the default) and frees the buffers. Needs `md_init`; every call starts an empty ring and zero
        accumulators, as `md_init` does. The setting stays on across `set_frames`. It runs under every thermostat
        and beside every other sampler; `md_run` refuses it under the barostat. While it is on, the evaluations of
        `md_run` take the builds that leave the centre-side pair gradients (per-apex instead of triangle-once; pair
        kernel and force gather instead of the folded EAM / ADP force kernels): the trajectory agrees with an
        unsampled run to rounding, not bit for bit."""
        p = _lib.MdFluxParams(int(n_lags), int(sample_every))
        rc = self._lib.ta_md_set_flux(self._handle, C.byref(p))
        if rc == _lib.TA_ERR_NOMEM:   # (no room: the library switched the feature off)
            self._md_flux_lags = 0
        self._check(rc)
        self._md_flux_lags = int(n_lags)

    @property
    def md_flux_lags(self):
        """Rows per frame that `md_set_flux` switched on, 0 while the feature is off."""
        return self._md_flux_lags

    def _md_flux_info(self, who):
        self._need_batch(who)
        info = (C.c_int64 * 8)()
        null = C.POINTER(C.c_double)()
        self._check(self._lib.ta_md_get_flux(self._handle, null, null, null, info))
        return info

    def md_flux(self):
        """What the loop has accumulated since `md_set_flux` (`ta_md_get_flux`), a dict: `sums` [n_frames, 18] (the sum
        of all rows), `a_heat` [n_frames, n_lags, 3] and `a_press` [n_frames, n_lags, 6] (sums over the time origins
        of J_a(n) J_a(n - k) and Pi_ab(n) Pi_ab(n - k)); `n_origins` [n_lags] = max(0, n_samples - k); `n_samples`,
        `n_lags`, `sample_every`, `last_step` and `first_step` (absolute steps of the newest and the first sample,
        -1: none), `chunk` (atoms per workgroup of the pair sweep), `blocks_per_frame` (the most workgroups of one
        frame) and `lanes` (lanes per centre). `md.heat_current_acf` and `md.pressure_acf` normalise the sums."""
        info = self._md_flux_info("md_flux")
        F, L = int(self.info.n_frames), int(info[1])
        sums, a_heat, a_press = np.zeros((F, _lib.TA_MD_FLUX_ROW)), np.zeros((F, L, 3)), np.zeros((F, L, 6))
        self._check(self._lib.ta_md_get_flux(self._handle, _lib.as_dp(sums), _lib.as_dp(a_heat), _lib.as_dp(a_press), info))
        n_samples = int(info[0])
        return {"sums": sums, "a_heat": a_heat, "a_press": a_press,
                "n_origins": np.maximum(0, n_samples - np.arange(L)).astype(np.int64), "n_samples": n_samples,
                "n_lags": L, "sample_every": int(info[2]), "last_step": int(info[3]), "first_step": int(info[4]),
                "chunk": int(info[5]), "blocks_per_frame": int(info[6]), "lanes": int(info[7])}

    def md_flux_rows(self, n=None):
        """The last `n` rows the ring holds, oldest first (`ta_md_get_flux_rows`; default: all, min(n_samples,
        n_lags)): a dict `rows` [n, n_frames, 18], its views `j_conv`, `j_pot` [n, n_frames, 3] and `kinetic`,
        `virial` [n, n_frames, 6], and `steps` [n] (absolute steps)."""
        if self.info is not None:   # (its own refusals)
            self._check(self._lib.ta_md_get_flux_rows(self._handle, 0, 0, C.POINTER(C.c_double)(), None))
        info = self._md_flux_info("md_flux_rows")
        if n is None:
            n = min(int(info[0]), int(info[1]))
        n = int(n)
        if n < 0:
            raise ValueError("md_flux_rows: n must be >= 0")
        F = int(self.info.n_frames)
        rows = np.zeros((max(n, 1), F, _lib.TA_MD_FLUX_ROW))
        steps = np.zeros(max(n, 1), dtype=np.int64)
        self._check(self._lib.ta_md_get_flux_rows(self._handle, 0, n, _lib.as_dp(rows),
                                                  steps.ctypes.data_as(C.POINTER(C.c_int64))))
        rows = rows[:n][::-1].copy()
        return {"rows": rows, "j_conv": rows[..., 0:3], "j_pot": rows[..., 3:6], "kinetic": rows[..., 6:12],
                "virial": rows[..., 12:18], "steps": steps[:n][::-1].copy()}

    def md_noise(self, step: int):
        """(xi, eta) [n_atoms, 3]: the standard normals the Langevin step with absolute index `step` (steps
        integrated since `md_init`) draws under the seed of `md_set_langevin`, made by the device function
        the integrator calls (`ta_md_noise`). Needs `md_init`."""
        self._need_batch("md_noise")
        step = int(step)
        if not -2 ** 63 <= step < 2 ** 63:
            raise ValueError("md_noise: the step must fit a signed 64-bit integer")
        N = int(self.info.n_atoms)
        xi, eta = np.empty((N, 3)), np.empty((N, 3))
        self._check(self._lib.ta_md_noise(self._handle, step, _lib.as_dp(xi), _lib.as_dp(eta)))
        return xi, eta

    def md_set_barostat(self, pressure=0.0, taup=0.0, compressibility=0.0, mask=None):
        """Berendsen barostat of `md_run` (`ta_md_set_barostat`; ASE's `NPTBerendsen`, with a `mask` its
        `Inhomogeneous_NPTBerendsen`): target `pressure` (eV / A^3), time constant `taup` (ASE time units; <= 0
        switches it off, the default), `compressibility` (A^3 / eV) and `mask`: None = isotropic, one factor
        from the mean pressure; three flags (x, y, z) = every free axis follows its own pressure, the others
        keep their length exactly. It composes with either thermostat and stays on across `set_frames`."""
        iso = mask is None
        m = np.ones(3, dtype=np.int64) if iso else np.asarray(mask)
        if m.shape != (3,):
            raise ValueError("md_set_barostat: mask must have three entries (x, y, z)")
        bp = _lib.MdBarostatParams(float(pressure), float(taup), float(compressibility),
                                   (C.c_int32 * 3)(*[int(bool(v)) for v in m]), 1 if iso else 0)
        self._check(self._lib.ta_md_set_barostat(self._handle, C.byref(bp)))
        self._md_barostat = bool(taup > 0.0)

    def md_set_nose_hoover(self, kT=0.0, tau=0.0, chain=3, loops=1, dof_removed=0):
        """Nose-Hoover chain thermostat of `md_run` (`ta_md_set_nose_hoover`; ASE's `NoseHooverChainNVT` with
        tdamp = `tau`, tchain = `chain`, tloop = `loops`): target kT (eV; <= 0 switches it off, the default),
        time constant (ASE time units), thermostats per chain (1 .. 8), loops per half-update (1 .. 16) and
        the degrees of freedom to take off 3 n_atoms of every frame. Every frame has its own chain; `md_init`
        puts it at rest. It excludes the Berendsen and the Langevin thermostat: switch the one that is on off
        first. `md_run` then also returns `echain`, and `epot + ekin + echain` is conserved."""
        p = _lib.MdNhcParams(float(kT), float(tau), int(chain), int(loops), int(dof_removed))
        self._check(self._lib.ta_md_set_nose_hoover(self._handle, C.byref(p)))
        self._md_chain = int(chain) if kT > 0.0 else 0

    def md_chain(self):
        """(eta, veta) [n_frames, chain]: positions and velocities of every frame's thermostat chain as the
        device holds them (`ta_md_get_chain`). Needs `md_init` and `md_set_nose_hoover`."""
        self._need_batch("md_chain")
        shape = (int(self.info.n_frames), max(self._md_chain, 1))
        eta, veta = np.empty(shape), np.empty(shape)
        self._check(self._lib.ta_md_get_chain(self._handle, _lib.as_dp(eta), _lib.as_dp(veta)))
        return eta, veta

    def md_set_chain(self, eta=None, veta=None):
        """Restart: hand the chains the (eta, veta) [n_frames, chain] of an earlier `md_chain` (None = zeros),
        after `set_frames` + `md_init` with the positions and velocities of that moment (`ta_md_set_chain`)."""
        self._need_batch("md_set_chain")
        n = int(self.info.n_frames) * max(self._md_chain, 1)
        arrays = []
        for name, a in (("eta", eta), ("veta", veta)):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float64)
                if a.size != n:
                    raise ValueError(f"md_set_chain: {name} [n_frames, chain] for every frame of the resident batch is needed")
            arrays.append(a)
        null = C.POINTER(C.c_double)()
        self._check(self._lib.ta_md_set_chain(self._handle, *[null if a is None else _lib.as_dp(a) for a in arrays]))

    def md_set_mtk(self, pressure=0.0, pdamp=0.0, chain=3, loops=1, mask=None):
        """Martyna-Tobias-Klein barostat of `md_run` (`ta_md_set_mtk_barostat`; ASE's `IsotropicMTKNPT` / `MTKNPT`
        with pdamp, pchain = `chain`, ploop = `loops`; LAMMPS `fix npt`): the isothermal-isobaric ensemble, volume
        fluctuations included. Target `pressure` (eV / A^3), time constant `pdamp` (ASE time units; <= 0 switches
        it off, the default), thermostats of the barostat's own chain (1 .. 8), loops per half-update (1 .. 16) and
        `mask`: None = isotropic, one strain rate from the mean driving force; three flags (x, y, z) = every free
        axis follows its own pressure, the others keep their length exactly. `md_run` needs the Nose-Hoover chain
        (`md_set_nose_hoover`) on beside it, whose kT it takes, and the Berendsen barostat off. It stays on across
        `set_frames`; `md_init` puts it at rest. `md_run` then also returns `ebaro`, and `epot + ekin + echain +
        ebaro` is conserved."""
        iso = mask is None
        m = np.ones(3, dtype=np.int64) if iso else np.asarray(mask)
        if m.shape != (3,):
            raise ValueError("md_set_mtk: mask must have three entries (x, y, z)")
        p = _lib.MdMtkParams(float(pressure), float(pdamp), int(chain), int(loops),
                             (C.c_int32 * 3)(*[int(bool(v)) for v in m]), 1 if iso else 0)
        self._check(self._lib.ta_md_set_mtk_barostat(self._handle, C.byref(p)))
        self._md_mtk = int(chain) if pdamp > 0.0 else 0

    def md_mtk_state(self):
        """(omega [n_frames, 3], xi, vxi [n_frames, chain]): strain rates and the barostat's chain of every frame
        as the device holds them (`ta_md_get_mtk_state`). Needs `md_init` and `md_set_mtk`."""
        self._need_batch("md_mtk_state")
        F = int(self.info.n_frames)
        omega, xi, vxi = np.empty((F, 3)), np.empty((F, max(self._md_mtk, 1))), np.empty((F, max(self._md_mtk, 1)))
        self._check(self._lib.ta_md_get_mtk_state(self._handle, _lib.as_dp(omega), _lib.as_dp(xi), _lib.as_dp(vxi)))
        return omega, xi, vxi

    def md_set_mtk_state(self, omega=None, xi=None, vxi=None):
        """Restart: hand the barostat the (omega, xi, vxi) of an earlier `md_mtk_state` (None = zeros), after
        `set_frames` + `md_init` + `md_set_chain` with the state of that moment (`ta_md_set_mtk_state`)."""
        self._need_batch("md_set_mtk_state")
        F = int(self.info.n_frames)
        arrays = []
        for name, a, n in (("omega [n_frames, 3]", omega, 3 * F), ("xi [n_frames, chain]", xi, F * max(self._md_mtk, 1)),
                           ("vxi [n_frames, chain]", vxi, F * max(self._md_mtk, 1))):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float64)
                if a.size != n:
                    raise ValueError(f"md_set_mtk_state: {name} for every frame of the resident batch is needed")
            arrays.append(a)
        null = C.POINTER(C.c_double)()
        self._check(self._lib.ta_md_set_mtk_state(self._handle, *[null if a is None else _lib.as_dp(a) for a in arrays]))

    def md_cells(self):
        """Cells [n_frames, 3, 3] of the resident batch as the library holds them (`ta_md_get_cell`)."""
        self._need_batch("md_cells")
        cells = np.empty((int(self.info.n_frames), 3, 3))
        self._check(self._lib.ta_md_get_cell(self._handle, _lib.as_dp(cells)))
        return cells

    def md_records(self, n_rec: int):
        """(volume [n_rec, n_frames], press [n_rec, n_frames, 3]) of the last `md_run` under the barostat
        (`ta_md_get_records`); `n_rec` = that run's n_steps // record_every + 1."""
        self._need_batch("md_records")
        F = int(self.info.n_frames)
        volume, press = np.empty((int(n_rec), F)), np.empty((int(n_rec), F, 3))
        self._check(self._lib.ta_md_get_records(self._handle, _lib.as_dp(volume), _lib.as_dp(press)))
        return volume, press

    def md_run(self, n_steps: int, dt: float, record_every: int = 1, want: int = None) -> dict:
        """`n_steps` velocity-Verlet (or, with `md_set_langevin`, Langevin) steps of length `dt` (ASE time units) of the resident batch on the
        device (`ta_md_run`): no per-atom traffic while the neighbour list holds. Returns
        `epot` / `ekin` [n_steps // record_every + 1, n_frames] (entry state first) and `n_rebuilds`.
        Afterwards `fetch(want | ENERGY | FORCES)` hands out the results of the last step.
        With `md_set_barostat` on, the cells follow the pressure, the dict also holds `volume` [n_rec, n_frames]
        and `press` [n_rec, n_frames, 3] (eV / A^3, per axis) of the recorded states, and a run that moved the
        cells ends with one list build for the final cells (counted in `n_rebuilds`).
        With `md_set_nose_hoover` on, the dict also holds `echain` [n_rec, n_frames], every record after the
        first is the state after the closing half-update of its step, and `epot + ekin + echain` is the
        conserved quantity.
        With `md_set_mtk` on, the dict holds `volume` and `press` as under the Berendsen barostat and `ebaro`
        [n_rec, n_frames], and `epot + ekin + echain + ebaro` is the conserved quantity."""
        self._need_batch("md_run")
        n_steps, record_every = int(n_steps), int(record_every)
        if n_steps < 0 or record_every < 1:
            raise ValueError("md_run: n_steps >= 0 and record_every >= 1 are needed")
        if want is None:
            want = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES
        F = int(self.info.n_frames)
        n_rec = n_steps // record_every + 1
        epot, ekin = np.empty((n_rec, F)), np.empty((n_rec, F))
        rebuilds = C.c_int32(0)
        rc = self._lib.ta_md_run(self._handle, n_steps, float(dt), int(want), record_every, _lib.as_dp(epot),
                                 _lib.as_dp(ekin), C.byref(rebuilds))
        self.batch_generation += 1  # the coordinates changed (also when the run ended early)
        self._check(rc)
        if rebuilds.value:
            n_pairs, n_triples, nnl = C.c_int64(0), C.c_int64(0), C.c_int32(0)
            self._check(self._lib.ta_list_sizes(self._handle, C.byref(n_pairs), C.byref(n_triples), C.byref(nnl)))
            self.info.n_pairs, self.info.n_triples, self.info.nnl_max = n_pairs.value, n_triples.value, nnl.value
        out = {"epot": epot, "ekin": ekin, "n_rebuilds": int(rebuilds.value)}
        if self._md_chain:   # the chain terms of the conserved quantity, at the slots of epot / ekin
            out["echain"] = np.empty((n_rec, F))
            self._check(self._lib.ta_md_get_chain_records(self._handle, _lib.as_dp(out["echain"])))
        if self._md_mtk:   # the barostat's terms of the conserved quantity
            out["ebaro"] = np.empty((n_rec, F))
            self._check(self._lib.ta_md_get_mtk_records(self._handle, _lib.as_dp(out["ebaro"])))
        if self._md_barostat or self._md_mtk:   # the cells moved on the device: stress and pressure follow them
            out["volume"], out["press"] = self.md_records(n_rec)
            self._volumes = np.abs(np.linalg.det(self.md_cells()))
            self._md_sig = None
        return out

    def md_state(self):
        """(positions, velocities) [n_atoms, 3] of the resident batch as the device holds them."""
        self._need_batch("md_state")
        N = int(self.info.n_atoms)
        x, v = np.empty((N, 3)), np.empty((N, 3))
        self._check(self._lib.ta_md_get_state(self._handle, _lib.as_dp(x), _lib.as_dp(v)))
        return x, v

    # -- device-resident relaxation ----------------------------------------------------------
    def relax_init(self, fixed=None, **params):
        """FIRE state of every frame of the resident batch for `relax_run` (`ta_relax_init`): v = 0, dt,
        a = astart. `fixed`: boolean mask [n_atoms] or indices of atoms that do not move and do not count
        towards convergence. `params`: dt, dtmax, maxstep, finc, fdec, astart, fa, nmin (ASE's FIRE defaults).
        `set_frames` drops the state; `update_positions` / `step` keep it."""
        self._need_batch("relax_init")
        p = dict(dt=0.1, dtmax=1.0, maxstep=0.2, finc=1.1, fdec=0.5, astart=0.1, fa=0.99, nmin=5)
        unknown = sorted(set(params) - set(p))
        if unknown:
            raise ValueError(f"relax_init: unknown parameter {unknown[0]!r} (known: {', '.join(p)})")
        p.update(params)
        if int(p["nmin"]) != p["nmin"]:
            raise ValueError("relax_init: nmin must be an integer")
        fp = _lib.FireParams(*(float(p[k]) for k in ("dt", "dtmax", "maxstep", "finc", "fdec", "astart", "fa")),
                             max(-1, min(int(p["nmin"]), 2 ** 31 - 1)))
        N = int(self.info.n_atoms)
        mptr = C.POINTER(C.c_uint8)()
        if fixed is not None:
            from .utils import fixed_atoms_mask
            mask = np.ascontiguousarray(fixed_atoms_mask(fixed, N, "relax_init"), dtype=np.uint8)
            mptr = mask.ctypes.data_as(C.POINTER(C.c_uint8))
        self._check(self._lib.ta_relax_init(self._handle, C.byref(fp), mptr))
        self._relax_cell = False

    def relax_set_cell(self, on=True, cell_factor=None, pressure=0.0, mask=None, hydrostatic=False):
        """Relax the cells together with the atoms in `relax_run` (`ta_relax_set_cell`; ASE's `UnitCellFilter`):
        the cells now resident become h0, the deformation gradient G = I. `cell_factor`: None = the atoms of
        each frame; `pressure`: external scalar pressure in eV / A^3; `mask`: 6 Voigt entries (xx, yy, zz, yz,
        xz, xy) or a symmetric 3 x 3 array, non-zero = free (None: all free); `hydrostatic`: only the volume
        changes. `on=False` returns to fixed cells and keeps the current ones. Needs `relax_init`, which
        switches the option off again."""
        self._need_batch("relax_set_cell")
        if not on:
            self._check(self._lib.ta_relax_set_cell(self._handle, 0, None))
            self._relax_cell = False
            return
        if mask is None:
            m = np.ones(6, dtype=np.int64)
        else:
            m = np.asarray(mask)
            if m.shape == (3, 3):
                if not np.array_equal(m != 0, (m != 0).T):
                    raise ValueError("relax_set_cell: a 3 x 3 mask must be symmetric")
                m = np.array([m[0, 0], m[1, 1], m[2, 2], m[1, 2], m[0, 2], m[0, 1]])
            if m.shape != (6,):
                raise ValueError("relax_set_cell: mask must have 6 Voigt entries or be a 3 x 3 array")
            m = (m != 0).astype(np.int64)
        cp = _lib.RelaxCellParams(0.0 if cell_factor is None else float(cell_factor), float(pressure),
                                  (C.c_int32 * 6)(*[int(v) for v in m]), 1 if hydrostatic else 0, 0)
        self._check(self._lib.ta_relax_set_cell(self._handle, 1, C.byref(cp)))
        self._relax_cell = True

    def relax_cell_state(self) -> dict:
        """cells (= h0 G^T), deform (G), cell_velocities [n_frames, 3, 3] and cell_fmax [n_frames] (largest row
        of the generalised cell force at the last state a cell run tested) of the relaxation
        (`ta_relax_get_cell`)."""
        self._need_batch("relax_cell_state")
        F = int(self.info.n_frames)
        cells, G, v, fm = np.empty((F, 3, 3)), np.empty((F, 3, 3)), np.empty((F, 3, 3)), np.empty(F)
        self._check(self._lib.ta_relax_get_cell(self._handle, _lib.as_dp(cells), _lib.as_dp(G), _lib.as_dp(v),
                                                _lib.as_dp(fm)))
        return {"cells": cells, "deform": G, "cell_velocities": v, "cell_fmax": fm}

    def relax_set_band(self, on=True, k=0.1, climb=False):
        """Treat the resident batch as the images of a nudged elastic band in `relax_run`
        (`ta_relax_set_band`): the first and the last frame are fixed endpoints, the others move under the
        improved-tangent band force with one spring constant `k` (eV / A^2), and with `climb` the interior
        image of highest energy climbs. FIRE then runs over the whole band as one system. Every call with
        `on` restarts the optimiser (v = 0, dt, a); `on=False` returns to independent frames and resets their
        FIRE states the same way, also when the band was not on. Needs
        `relax_init`, which supplies the FIRE parameters and the fixed mask and switches the option off again."""
        self._need_batch("relax_set_band")
        if not on:
            self._check(self._lib.ta_relax_set_band(self._handle, 0, None))
            return
        bp = _lib.BandParams(float(k), 1 if climb else 0, 0)
        self._check(self._lib.ta_relax_set_band(self._handle, 1, C.byref(bp)))

    def relax_band_state(self) -> dict:
        """forces (the band forces B) and tangents [n_atoms, 3], energies [n_frames] and climbing (image index,
        -1 without climb) of the state the last band run ended on (`ta_relax_get_band`)."""
        self._need_batch("relax_band_state")
        N, F = int(self.info.n_atoms), int(self.info.n_frames)
        b, t, e = np.empty((N, 3)), np.empty((N, 3)), np.empty(F)
        c = C.c_int32(-1)
        self._check(self._lib.ta_relax_get_band(self._handle, _lib.as_dp(b), _lib.as_dp(t), _lib.as_dp(e), C.byref(c)))
        return {"forces": b, "tangents": t, "energies": e, "climbing": int(c.value)}

    def relax_run(self, max_steps: int, fmax: float, want: int = None) -> dict:
        """FIRE steps of the resident batch on the device (`ta_relax_run`) until every frame has
        max_i |F_i| < `fmax` (eV / A) or the others have taken `max_steps` steps; continues from the state the
        last run left. Returns per frame `steps` (taken in this run), `converged`, `fmax` (of the final state)
        and `energy`, and `n_rebuilds`. Afterwards `fetch(want | ENERGY | FORCES)` hands out the results of
        the final state."""
        self._need_batch("relax_run")
        max_steps = int(max_steps)
        if max_steps < 0:
            raise ValueError("relax_run: max_steps must be >= 0")
        if want is None:
            want = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES
        F = int(self.info.n_frames)
        steps, conv = np.zeros(F, dtype=np.int32), np.zeros(F, dtype=np.int32)
        fm = np.empty(F)
        rebuilds = C.c_int32(0)
        rc = self._lib.ta_relax_run(self._handle, max_steps, float(fmax), int(want), _lib.as_ip(steps),
                                    _lib.as_ip(conv), _lib.as_dp(fm), C.byref(rebuilds))
        self.batch_generation += 1  # the coordinates changed (also when the run ended early)
        if rc != _lib.TA_OK:
            self._relax_cell = False   # (a failed run drops the relaxation state, the cell option with it)
        self._check(rc)
        null = C.POINTER(C.c_double)()
        if rebuilds.value:
            n_pairs, n_triples, nnl = C.c_int64(0), C.c_int64(0), C.c_int32(0)
            self._check(self._lib.ta_list_sizes(self._handle, C.byref(n_pairs), C.byref(n_triples), C.byref(nnl)))
            self.info.n_pairs, self.info.n_triples, self.info.nnl_max = n_pairs.value, n_triples.value, nnl.value
        if self._relax_cell:   # the cells moved on the device: stress and pressure follow them
            cells = np.empty((F, 3, 3))
            self._check(self._lib.ta_relax_get_cell(self._handle, _lib.as_dp(cells), null, null, null))
            self._volumes = np.abs(np.linalg.det(cells))
            self._md_sig = None
        energy = np.empty(F)
        self._check(self._lib.ta_get_results(self._handle, _lib.as_dp(energy), null, null, null, null))
        return {"steps": steps.astype(np.int64), "converged": conv.astype(bool), "fmax": fm, "energy": energy,
                "n_rebuilds": int(rebuilds.value)}

    def relax_state(self) -> dict:
        """positions, velocities [n_atoms, 3] and dt, a, npos [n_frames] of the relaxation as the device holds them."""
        self._need_batch("relax_state")
        N, F = int(self.info.n_atoms), int(self.info.n_frames)
        x, v = np.empty((N, 3)), np.empty((N, 3))
        dt, a, npos = np.empty(F), np.empty(F), np.zeros(F, dtype=np.int32)
        self._check(self._lib.ta_relax_get_state(self._handle, _lib.as_dp(x), _lib.as_dp(v), _lib.as_dp(dt),
                                                 _lib.as_dp(a), _lib.as_ip(npos)))
        return {"positions": x, "velocities": v, "dt": dt, "a": a, "npos": npos.astype(np.int64)}

    def list_stats(self):
        """(lists built, lists reused) by this engine."""
        a, b = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.ta_list_stats(self._handle, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def compute(self, want: int):
        self._check(self._lib.ta_compute(self._handle, int(want)))

    def set_stream(self, stream_ptr):
        """Run on a caller-owned hipStream_t (int handle); None = the engine's own stream.
        0 is the handle of the legacy default stream (what `torch.cuda.current_stream().cuda_stream`
        returns when no other stream was made current): it is passed on as `hipStreamLegacy`,
        because a NULL argument means "the handle's own stream" to the C ABI."""
        HIP_STREAM_LEGACY = 1  # hip_runtime_api.h: #define hipStreamLegacy ((hipStream_t)1)
        if stream_ptr is None:
            ptr = 0
        else:
            ptr = int(stream_ptr) or HIP_STREAM_LEGACY
        self._check(self._lib.ta_set_stream(self._handle, C.c_void_p(ptr)))

    def synchronize(self):
        self._check(self._lib.ta_synchronize(self._handle))

    def fetch(self, want: int, descriptors=False) -> dict:
        """Copy back what `want` asked for; arrays cover the whole batch."""
        info = self.info
        N, F = int(info.n_atoms), int(info.n_frames)
        # (the library fills every array it is handed, or fails)
        out = {"energy": np.empty(F)}
        forces = virial = atomic = desc = None
        if want & (_lib.TA_WANT_FORCES | _lib.TA_WANT_VIRIAL):
            forces = np.empty((N, 3))
            virial = np.empty((F, 3, 3))
        if want & _lib.TA_WANT_ATOMIC:
            atomic = np.empty(N)
        if descriptors:
            desc = np.empty((N, int(info.descriptor_dim)))
        null = C.POINTER(C.c_double)()
        self._check(self._lib.ta_get_results(
            self._handle, _lib.as_dp(out["energy"]),
            _lib.as_dp(forces) if forces is not None else null,
            _lib.as_dp(virial) if virial is not None else null,
            _lib.as_dp(atomic) if atomic is not None else null,
            _lib.as_dp(desc) if desc is not None else null))
        if forces is not None:
            out["forces"], out["virial"] = forces, virial
        if atomic is not None:
            out["atomic"] = atomic
        if desc is not None:
            scale = getattr(self._nn, "descriptor_scale", None)
            out["descriptors"] = desc * scale() if scale is not None else desc
        if self.finite_temperature:
            out = self._td_results(out)
        return out

    def evaluate(self, atoms_list: Sequence, want: int = None, descriptors=False) -> List[dict]:
        """One dict per frame: energy, atomic, forces, virial, stress (Voigt,
        eV/A^3), total_pressure (GPa) in the caller's atom order."""
        if want is None:
            want = (_lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES | _lib.TA_WANT_VIRIAL |
                    _lib.TA_WANT_ATOMIC)
        self.set_frames(atoms_list)
        self.compute(want)
        return self._per_frame(self.fetch(want, descriptors=descriptors))

    def _per_frame(self, res: dict) -> List[dict]:
        out, a = [], 0
        for f, n in enumerate(self._natoms):
            d = {"energy": float(res["energy"][f])}
            if "atomic" in res:
                d["atomic"] = res["atomic"][a:a + n]
            for key in ("free_energy", "eentropy"):
                if key in res:
                    d[key] = float(res[key][f])
            for key in ("free_energy_atomic", "eentropy_atomic"):
                if key in res:
                    d[key] = res[key][a:a + n]
            if "forces" in res:
                d["forces"] = res["forces"][a:a + n]
                w = res["virial"][f]
                d["virial"] = w
                # a frame without three lattice vectors has no volume (ASE's `get_volume`, which
                # feeds the reference's `volume` placeholder at universal.py:865, raises for it):
                # the virial is still defined, stress and pressure are not and are left out
                if self._volumes[f] > 0.0:
                    s = w / self._volumes[f]                       # basic.py:317
                    d["stress"] = np.array([s[0, 0], s[1, 1], s[2, 2], s[1, 2], s[0, 2], s[0, 1]])
                    d["total_pressure"] = float(np.trace(s) / (-3.0 * GPa))  # basic.py:403-405
            if "descriptors" in res:
                d["descriptors"] = res["descriptors"][a:a + n]
            out.append(d)
            a += n
        return out

    def evaluate_md(self, atoms, want: int = None, descriptors=False) -> dict:
        """One structure, as `evaluate([atoms])[0]`, but when it is the system of the previous call
        (same atoms, species, periodicity) only its coordinates are sent and the neighbour list is
        kept as long as the Verlet skin allows (`set_skin`): the MD / relaxation loop of the
        reference's calculator (calculator.py:335-370) without its per-call feed-dict rebuild."""
        if want is None:
            want = (_lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES | _lib.TA_WANT_VIRIAL |
                    _lib.TA_WANT_ATOMIC)
        periodic = self._clf.periodic
        pbc = tuple(bool(x) for x in atoms.pbc) if periodic else (False, False, False)
        sig = (len(atoms), np.asarray(atoms.numbers).tobytes(), pbc)
        cell = np.ascontiguousarray(atoms.get_cell(complete=True), dtype=np.float64).reshape(3, 3)
        if sig == self._md_sig and self.info is not None and self.finite_temperature:
            T = float(atoms.info.get("etemperature", 0.0))
            if self._etemperatures is None or self._etemperatures[0] != T:
                self.set_electron_temperatures([T])
        if sig == self._md_sig and self.info is not None and not descriptors:
            same_cell = np.array_equal(cell, self._md_cell)
            res = self.step(atoms.positions, want, None if same_cell else cell[None], view=True)
            self._md_cell = cell
            # (the staging memory is rewritten by the next call: hand out copies, the only ones made)
            return self._per_frame({k: v.copy() for k, v in res.items()})[0]
        if sig == self._md_sig and self.info is not None:
            same_cell = np.array_equal(cell, self._md_cell)
            self.update_positions(atoms.positions, None if same_cell else cell[None])
            self._md_cell = cell
        else:
            self.set_frames([atoms])
            self._md_sig, self._md_cell = sig, cell
        self.compute(want)
        return self._per_frame(self.fetch(want, descriptors=descriptors))[0]

    # -- measurement -------------------------------------------------------------------
    def time_compute(self, want: int, warmup: int, steps: int, per_kernel=True):
        total = C.c_double(0.0)
        slots = np.zeros(_lib.TA_N_KERNEL_SLOTS)
        self._check(self._lib.ta_time_compute(
            self._handle, int(want), int(warmup), int(steps), C.byref(total),
            _lib.as_dp(slots) if per_kernel else C.POINTER(C.c_double)()))
        return total.value, dict(zip(_lib.KERNEL_SLOTS, slots.tolist()))

    def count_contributing_triples(self) -> int:
        """Triples of the resident batch with all three sides below acut (non-zero G4 terms)."""
        n = C.c_int64(0)
        self._check(self._lib.ta_count_contributing_triples(self._handle, C.byref(n)))
        return int(n.value)

    def count_owned_triangles(self) -> int:
        """Contributing triples whose centre owns the triangle (`ta_count_owned_triangles`)."""
        n = C.c_int64(0)
        self._check(self._lib.ta_count_owned_triangles(self._handle, C.byref(n)))
        return int(n.value)

    def set_triangles(self, on: bool):
        """Triangle-once angular backward pass where it applies (default) or the per-apex one
        (`ta_set_triangles`); takes effect at the next evaluation."""
        self._check(self._lib.ta_set_triangles(self._handle, 1 if on else 0))

    def backward_variant(self) -> int:
        """Angular backward builds of the last evaluation with forces: bit 0 per apex, bit 1 triangles."""
        v = C.c_int32(0)
        self._check(self._lib.ta_backward_variant(self._handle, C.byref(v)))
        return int(v.value)

    def mlp_launch(self) -> dict:
        """What the last per-atom network launch of this engine was (`ta_mlp_launch_info`): `family` (tile,
        tile_all, wave, wave_all, quad, quad_all, td, or none), `threads` per workgroup, `lh` / `nt` (hidden
        layers and wavefronts per tile of the wave / quad builds, else 0), `grid` (x, y), dynamic `lds_bytes`
        and `da`, where the activation derivatives lived (registers, lds or global)."""
        v = (C.c_int64 * 8)()
        self._check(self._lib.ta_mlp_launch_info(self._handle, v))
        return {"family": _lib.TA_MLP_FAMILY[int(v[0])], "threads": int(v[1]), "lh": int(v[2]), "nt": int(v[3]),
                "grid": (int(v[4]), int(v[5])), "lds_bytes": int(v[6]), "da": _lib.TA_MLP_DA[int(v[7])]}

    def mlp_tile_body(self) -> str:
        """Which body the tile kernels of the last per-atom network launch ran (`ta_mlp_tile_body`): "scalar"
        (hidden layers without skips, one linear output unit), "generic", "mixed" (an all-elements launch whose
        networks differ) or "none" when the last launch was not a tile launch."""
        v = C.c_int32(0)
        self._check(self._lib.ta_mlp_tile_body(self._handle, C.byref(v)))
        return _lib.TA_MLP_BODY[int(v.value)]

    def measure_hbm_copy(self, nbytes: int = 1 << 30, reps: int = 10) -> float:
        """Achievable device-to-device copy rate in GB/s (read + written bytes)."""
        g = C.c_double(0.0)
        self._check(self._lib.ta_measure_hbm_copy(self._handle, int(nbytes), int(reps), C.byref(g)))
        return g.value

    def batch_energy_device_ptr(self) -> int:
        p = C.c_void_p()
        self._check(self._lib.ta_batch_energy_device_ptr(self._handle, C.byref(p)))
        return p.value

    def copy_batch_energy(self, dst_device_ptr: int):
        """Enqueue a D2D copy of the batch energy (one double) on the engine's stream."""
        self._check(self._lib.ta_copy_batch_energy(self._handle, C.c_void_p(int(dst_device_ptr))))

    # -- training support ---------------------------------------------------
    def param_count(self) -> int:
        n = C.c_int64(0)
        self._check(self._lib.ta_param_count(self._handle, C.byref(n)))
        return int(n.value)

    def update_weights(self, flat):
        """Replace the MLP weights of the live handle (layout of `train.flatten_weights`)."""
        flat = np.ascontiguousarray(flat, dtype=np.float64).ravel()
        self._check(self._lib.ta_update_weights(self._handle, _lib.as_dp(flat), len(flat)))

    def energy_gradient(self, frame_coeff) -> np.ndarray:
        """sum_f frame_coeff[f] dE_f/dtheta for the resident batch, flat parameter layout."""
        coeff = np.ascontiguousarray(frame_coeff, dtype=np.float64).ravel()
        if len(coeff) != int(self.info.n_frames):
            raise ValueError("one coefficient per resident frame")
        grad = np.zeros(self.param_count())
        self._check(self._lib.ta_energy_gradient(self._handle, _lib.as_dp(coeff), _lib.as_dp(grad), len(grad)))
        return grad

    def loss_gradient(self, frame_coeff=None, dR=None, dh=None, return_tangent=False):
        """d/dtheta (sum_f frame_coeff[f] E_f + D_delta E) for the resident batch, delta = (dR
        [n_atoms, 3], dh [n_frames, 3, 3]): the gradient of an energy + forces + stress loss in one
        analytic pass (`ta_loss_gradient`); flat parameter layout."""
        null = C.POINTER(C.c_double)()
        N, F = int(self.info.n_atoms), int(self.info.n_frames)

        def arr(a, shape):
            if a is None:
                return None, null
            a = np.ascontiguousarray(a, dtype=np.float64).reshape(shape)
            return a, _lib.as_dp(a)
        c, cp = arr(frame_coeff, (F,))
        r, rp = arr(dR, (N, 3))
        hh, hp = arr(dh, (F, 9))
        grad = np.zeros(self.param_count())
        tangent = np.zeros((N, int(self.info.descriptor_dim))) if return_tangent else None
        self._check(self._lib.ta_loss_gradient(self._handle, cp, rp, hp, _lib.as_dp(grad), len(grad),
                                               _lib.as_dp(tangent) if return_tangent else null))
        if return_tangent:   # directional derivative of the raw descriptors [N, D]
            scale = getattr(self._nn, "descriptor_scale", None)
            return grad, (tangent * scale() if scale is not None else tangent)
        return grad

    # -- the GRAP `nn` filter network as trainable parameters -----------------------------
    def filter_param_count(self) -> int:
        """Length of the filter network's flat vector (0 without one): per layer W[in][out], b[out]."""
        n = C.c_int64(0)
        self._check(self._lib.ta_filter_param_count(self._handle, C.byref(n)))
        return int(n.value)

    def update_filter_weights(self, flat):
        """Replace the filter network of the live handle (layout of `filter_param_count`); the resident
        descriptors are recomputed on their next use."""
        flat = np.ascontiguousarray(flat, dtype=np.float64).ravel()
        self._check(self._lib.ta_update_filter_weights(self._handle, _lib.as_dp(flat), len(flat)))

    def grap_loss_gradient(self, frame_coeff=None, dR=None, dh=None) -> np.ndarray:
        """`loss_gradient` of a GRAP/nn model with respect to [MLP weights | filter network]
        (`ta_grap_loss_gradient`); dR = dh = None: the energy term only."""
        null = C.POINTER(C.c_double)()
        N, F = int(self.info.n_atoms), int(self.info.n_frames)

        def arr(a, shape):
            if a is None:
                return None, null
            a = np.ascontiguousarray(a, dtype=np.float64).reshape(shape)
            return a, _lib.as_dp(a)
        c, cp = arr(frame_coeff, (F,))
        r, rp = arr(dR, (N, 3))
        hh, hp = arr(dh, (F, 9))
        grad = np.zeros(self.param_count() + self.filter_param_count())
        self._check(self._lib.ta_grap_loss_gradient(self._handle, cp, rp, hp, _lib.as_dp(grad), len(grad)))
        return grad

    def td_loss_gradient(self, coeff_free_energy=None, coeff_energy=None, coeff_eentropy=None, dR=None, dh=None,
                         return_tangent=False):
        """Temperature-dependent models: d/dtheta (sum_f (a_f U_f + b_f F_f + g_f S_f) + D_delta F) for the
        resident batch, b = `coeff_free_energy`, a = `coeff_energy`, g = `coeff_eentropy` (one per frame,
        None = 0) and delta = (dR, dh) the force / stress direction of F as in `loss_gradient`
        (`ta_td_loss_gradient`); flat parameter layout (H, U, S nets). `return_tangent` (needs a
        direction) also returns the directional derivative of the raw descriptors [N, D]."""
        null = C.POINTER(C.c_double)()
        N, F = int(self.info.n_atoms), int(self.info.n_frames)

        def arr(a, shape):
            if a is None:
                return None, null
            a = np.ascontiguousarray(a, dtype=np.float64).reshape(shape)
            return a, _lib.as_dp(a)
        b, bp = arr(coeff_free_energy, (F,))
        a, ap = arr(coeff_energy, (F,))
        g, gp = arr(coeff_eentropy, (F,))
        r, rp = arr(dR, (N, 3))
        hh, hp = arr(dh, (F, 9))
        grad = np.zeros(self.param_count())
        tangent = np.zeros((N, int(self.info.descriptor_dim))) if return_tangent else None
        self._check(self._lib.ta_td_loss_gradient(self._handle, bp, ap, gp, rp, hp, _lib.as_dp(grad), len(grad),
                                                  _lib.as_dp(tangent) if return_tangent else null))
        if return_tangent:
            scale = getattr(self._nn, "descriptor_scale", None)
            return grad, (tangent * scale() if scale is not None else tangent)
        return grad

    # -- constants of the analytic EAM functions as parameters (potentials.py:129-163) ---------
    def constant_count(self) -> int:
        n = C.c_int64(0)
        self._check(self._lib.ta_constant_count(self._handle, C.byref(n)))
        return int(n.value)

    def constants(self) -> np.ndarray:
        """Flat vector: 20 per element (the model's `eam_el` rows), then 7 per sorted pair type
        (Zjw04xcp cross terms)."""
        out = np.zeros(self.constant_count())
        self._check(self._lib.ta_get_constants(self._handle, _lib.as_dp(out), len(out)))
        return out

    def update_constants(self, flat):
        flat = np.ascontiguousarray(flat, dtype=np.float64).ravel()
        self._check(self._lib.ta_update_constants(self._handle, _lib.as_dp(flat), len(flat)))

    def constant_gradient(self, frame_coeff=None, dR=None, dh=None) -> np.ndarray:
        """d/dconstants (sum_f frame_coeff[f] E_f + D_delta E) for the resident batch
        (`ta_constant_gradient`), arguments as `loss_gradient`."""
        null = C.POINTER(C.c_double)()
        N, F = int(self.info.n_atoms), int(self.info.n_frames)

        def arr(a, shape):
            if a is None:
                return None, null
            a = np.ascontiguousarray(a, dtype=np.float64).reshape(shape)
            return a, _lib.as_dp(a)
        c, cp = arr(frame_coeff, (F,))
        r, rp = arr(dR, (N, 3))
        hh, hp = arr(dh, (F, 9))
        grad = np.zeros(self.constant_count())
        self._check(self._lib.ta_constant_gradient(self._handle, cp, rp, hp, _lib.as_dp(grad), len(grad)))
        return grad

    def hessian_vectors(self, dR=None, dh=None, want_virial=False):
        """Analytic directional derivatives of the forces (and virials) of the resident batch
        (`ta_hessian_vectors`): dR [n_dir, N, 3] and / or dh [n_dir, F, 3, 3]; both None = the 3 N unit
        displacements. Returns dF [n_dir, N, 3] (= -H v) and, with `want_virial`, dW [n_dir, F, 3, 3].
        Raises ValueError for models without the analytic path."""
        N, F = int(self.info.n_atoms), int(self.info.n_frames)
        null = C.POINTER(C.c_double)()
        rp = hp = null
        if dR is None and dh is None:
            n_dir = 3 * N
        else:
            n_dir = len(dR) if dR is not None else len(dh)
        if dR is not None:
            dR = np.ascontiguousarray(dR, dtype=np.float64).reshape(n_dir, N, 3)
            rp = _lib.as_dp(dR)
        if dh is not None:
            dh = np.ascontiguousarray(dh, dtype=np.float64).reshape(n_dir, F, 9)
            hp = _lib.as_dp(dh)
        dF = np.zeros((n_dir, N, 3))
        dW = np.zeros((n_dir, F, 3, 3)) if want_virial else None
        # at most 65535 directions per library call; the unit displacements are chunked by `first`
        chunk = 32768 if (dR is None and dh is None) else n_dir
        for first in range(0, n_dir, max(chunk, 1)):
            m = min(chunk, n_dir - first)
            self._check(self._lib.ta_hessian_vectors(
                self._handle, m, first, rp, hp, _lib.as_dp(dF[first:]),
                _lib.as_dp(dW[first:]) if want_virial else null))
        return (dF, dW) if want_virial else dF

    # -- harmonic phonons (ta_phonon_*; `phonons.Phonons` is the user-facing class) ----------------
    def phonon_set_cell(self, n_basis, basis_of, masses, start, vectors, q_chunk=0):
        """Declare the one resident frame a supercell whose first `n_basis` atoms are the home cell
        (`ta_phonon_set_cell`): basis_of [N], masses [n_basis] amu, and the CSR list (start [n_basis N + 1],
        vectors [*, 3] in Angstrom) of the shortest vectors from every home atom to the images of every atom."""
        self._need_batch("phonon_set_cell")
        basis_of = np.ascontiguousarray(basis_of, dtype=np.int32).reshape(-1)
        masses = np.ascontiguousarray(masses, dtype=np.float64).reshape(-1)
        start = np.ascontiguousarray(start, dtype=np.int32).reshape(-1)
        vectors = np.ascontiguousarray(vectors, dtype=np.float64).reshape(-1, 3)
        N, n_basis = int(self.info.n_atoms), int(n_basis)
        if len(basis_of) != N or len(masses) != n_basis or len(start) != n_basis * N + 1 or \
                (len(start) and len(vectors) < start[-1]):
            raise ValueError("phonon_set_cell: basis_of [N], masses [n_basis], start [n_basis N + 1] and "
                             "vectors [start[-1], 3] are expected")
        p = _lib.PhononParams(n_basis, int(q_chunk))
        vec = vectors if len(vectors) else np.zeros((1, 3))
        self._check(self._lib.ta_phonon_set_cell(self._handle, C.byref(p), _lib.as_ip(basis_of), _lib.as_dp(masses),
                                                 _lib.as_ip(start), _lib.as_dp(vec)))
        self._phonon = (n_basis, N)

    def _phonon_shape(self, who):
        self._need_batch(who)
        shape = getattr(self, "_phonon", None)
        if shape is None or shape[1] != int(self.info.n_atoms):
            raise ValueError(f"{who} called before phonon_set_cell")
        return shape

    def phonon_force_constants(self) -> np.ndarray:
        """Phi [n_basis, N, 3, 3] of the home-cell atoms from the analytic Hessian-vector products; it stays
        on the device for `phonon_frequencies` / `phonon_dos`. ValueError for models without the analytic path."""
        nb, N = self._phonon_shape("phonon_force_constants")
        phi = np.zeros((nb, N, 3, 3))
        self._check(self._lib.ta_phonon_force_constants(self._handle, _lib.as_dp(phi)))
        return phi

    def phonon_load_force_constants(self, phi):
        nb, N = self._phonon_shape("phonon_load_force_constants")
        phi = np.ascontiguousarray(phi, dtype=np.float64)
        if phi.shape != (nb, N, 3, 3):
            raise ValueError(f"phonon_load_force_constants: Phi must be [{nb}, {N}, 3, 3]")
        self._check(self._lib.ta_phonon_load_force_constants(self._handle, _lib.as_dp(phi)))

    def phonon_frequencies(self, q_cart, eigenvectors=False):
        """Frequencies [Q, n] in THz (ascending, imaginary modes negative) at the Cartesian wave vectors q_cart
        [Q, 3] in 1/Angstrom; with `eigenvectors` also the modes [Q, n, n] complex, row m = mode m. Raises
        RuntimeError if the solver left a matrix unconverged."""
        nb, _ = self._phonon_shape("phonon_frequencies")
        q = np.ascontiguousarray(q_cart, dtype=np.float64).reshape(-1, 3)
        n, Q = 3 * nb, len(q)
        freq = np.zeros((Q, n))
        vec = np.zeros((Q, n, n), dtype=np.complex128) if eigenvectors else None
        info = np.zeros(1, dtype=np.int64)
        null = C.POINTER(C.c_double)()
        self._check(self._lib.ta_phonon_frequencies(
            self._handle, Q, _lib.as_dp(q if Q else np.zeros((1, 3))), _lib.as_dp(freq if Q else np.zeros(1)),
            vec.ctypes.data_as(C.POINTER(C.c_double)) if eigenvectors and Q else null,
            info.ctypes.data_as(C.POINTER(C.c_int64))))
        if info[0]:
            raise RuntimeError(f"phonon_frequencies: the eigensolver left {int(info[0])} matrices unconverged")
        return (freq, vec) if eigenvectors else freq

    def phonon_dos(self, q_cart, n_bins, nu_min, nu_max, partial=False) -> dict:
        """Histogram of the frequencies at q_cart, formed on the device: `total` [n_bins] uint64 counts of
        modes in the bins k = floor((nu - nu_min) * (n_bins / (nu_max - nu_min))), `outside` = modes beyond
        the range (counted nowhere else), and with `partial` the per-home-atom weights [n_basis, n_bins]."""
        nb, _ = self._phonon_shape("phonon_dos")
        q = np.ascontiguousarray(q_cart, dtype=np.float64).reshape(-1, 3)
        n_bins = int(n_bins)
        total = np.zeros(max(n_bins, 1), dtype=np.uint64)
        part = np.zeros((nb, max(n_bins, 1))) if partial else None
        info = np.zeros(2, dtype=np.int64)
        null = C.POINTER(C.c_double)()
        self._check(self._lib.ta_phonon_dos(
            self._handle, len(q), _lib.as_dp(q if len(q) else np.zeros((1, 3))), n_bins, float(nu_min), float(nu_max),
            total.ctypes.data_as(C.POINTER(C.c_uint64)), _lib.as_dp(part) if partial else null,
            info.ctypes.data_as(C.POINTER(C.c_int64))))
        if info[0]:
            raise RuntimeError(f"phonon_dos: the eigensolver left {int(info[0])} matrices unconverged")
        out = {"total": total, "outside": int(info[1])}
        if partial:
            out["partial"] = part
        return out

    def phonon_eigh(self, A, eigenvectors=True):
        """The batched Hermitian eigensolver alone: A [batch, n, n] complex (its Hermitian part is solved),
        n <= TA_PHONON_MAX_ORDER. Returns (w [batch, n] ascending, V [batch, n, n] with row m = eigenvector m
        or None, unconverged count)."""
        A = np.ascontiguousarray(A, dtype=np.complex128)
        if A.ndim != 3 or A.shape[1] != A.shape[2]:
            raise ValueError("phonon_eigh: A must be [batch, n, n]")
        batch, n = A.shape[0], A.shape[1]
        w = np.zeros((batch, n))
        V = np.zeros((batch, n, n), dtype=np.complex128) if eigenvectors else None
        info = np.zeros(1, dtype=np.int64)
        dp = C.POINTER(C.c_double)
        self._check(self._lib.ta_phonon_eigh(
            self._handle, n, batch, A.ctypes.data_as(dp) if batch else dp(), _lib.as_dp(w) if batch else dp(),
            V.ctypes.data_as(dp) if eigenvectors and batch else dp(), info.ctypes.data_as(C.POINTER(C.c_int64))))
        return w, V, int(info[0])

    def energies(self, reuse_descriptors=True) -> np.ndarray:
        """Frame energies of the resident batch; with `reuse_descriptors` only the MLP is re-run."""
        want = _lib.TA_WANT_ENERGY | (_lib.TA_WANT_REUSE_DESCRIPTORS if reuse_descriptors else 0)
        self.compute(want)
        return self.fetch(_lib.TA_WANT_ENERGY)["energy"]

    def set_batch_energy_target(self, dst_device_ptr):
        """Later `compute` calls write the batch energy straight to this device address
        (None = the library's own buffer): no copy before a collective."""
        self._check(self._lib.ta_set_batch_energy_target(self._handle, C.c_void_p(int(dst_device_ptr or 0))))

    def eam_tabulate(self, r, rho) -> dict:
        """rho(r), phi(r), F(rho) (and u, w for ADP) of an EAM model on the given abscissae,
        evaluated by the device functions of the energy kernels. Rows: sorted elements; pairs
        a <= b in upper-triangle order; for eam/fs the rho rows are rho[centre][neighbour],
        centre-major."""
        r = np.ascontiguousarray(r, dtype=np.float64).ravel()
        rho = np.ascontiguousarray(rho, dtype=np.float64).ravel()
        nel = len(self._nn.elements)
        npair = nel * (nel + 1) // 2
        adp = getattr(self._nn, "tag", "") == "adp"
        nrho = nel * nel if getattr(self._nn, "tag", "") == "fs" else nel
        out = {"rho": np.zeros((nrho, len(r))), "phi": np.zeros((npair, len(r))),
               "embed": np.zeros((nel, len(rho)))}
        null = C.POINTER(C.c_double)()
        if adp:
            out["u"], out["w"] = np.zeros((npair, len(r))), np.zeros((npair, len(r)))
        self._check(self._lib.ta_eam_tabulate(
            self._handle, len(r), _lib.as_dp(r), len(rho), _lib.as_dp(rho), _lib.as_dp(out["rho"]),
            _lib.as_dp(out["phi"]), _lib.as_dp(out["embed"]),
            _lib.as_dp(out["u"]) if adp else null, _lib.as_dp(out["w"]) if adp else null))
        out["pairs"] = [self._nn.elements[a] + self._nn.elements[b]
                        for a in range(nel) for b in range(a, nel)]
        return out

    def pairs(self):
        P = int(self.info.n_pairs)
        i = np.zeros(max(P, 1), dtype=np.int32)
        j = np.zeros(max(P, 1), dtype=np.int32)
        s = np.zeros((max(P, 1), 3), dtype=np.int32)
        self._check(self._lib.ta_get_pairs(self._handle, _lib.as_ip(i), _lib.as_ip(j), _lib.as_ip(s)))
        return i[:P], j[:P], s[:P]

    def list_layout(self, which="resident") -> dict:
        """The neighbour list as the kernels read it (`ta_list_info`, `ta_get_list`; debugging / parity).
        `which`: "resident", the list that was built (under a skin the skin list), or "kernel", the list the
        next evaluation runs on (the exact list where one is extracted, else the resident one). Returns the
        `info` dict (atoms, elements, n_slots, n_blk, cap, builder: host / one_pass / two_pass, filtered,
        rev_indirect) and the arrays pair_start [N + 1], pair_stop [N], seg_start [N, elements + 1] (and its
        closing entry `seg_close`), pair_i, pair_j, pair_shift [n_slots, 3], pair_rev and blk_center [n_blk + 1]
        (None without run packing)."""
        view = _lib.TA_LIST_VIEW[which]
        v = (C.c_int64 * 8)()
        self._check(self._lib.ta_list_info(self._handle, view, v))
        info = {"atoms": int(v[0]), "elements": int(v[1]), "n_slots": int(v[2]), "n_blk": int(v[3]), "cap": int(v[4]),
                "builder": _lib.TA_LIST_BUILDER[int(v[5])], "filtered": bool(v[6]), "rev_indirect": bool(v[7])}
        N, nel, P, nb = info["atoms"], info["elements"], info["n_slots"], info["n_blk"]
        z = lambda *shape: np.zeros(shape, dtype=np.int32)
        start, stop, seg = z(N + 1), z(max(N, 1)), z(N * (nel + 1) + 1)
        pi, pj, ps, rev, blk = z(max(P, 1)), z(max(P, 1)), z(max(P, 1), 3), z(max(P, 1)), z(nb + 1)
        self._check(self._lib.ta_get_list(self._handle, view, _lib.as_ip(start), _lib.as_ip(stop), _lib.as_ip(seg),
                                          _lib.as_ip(pi), _lib.as_ip(pj), _lib.as_ip(ps), _lib.as_ip(rev),
                                          _lib.as_ip(blk)))
        return {"info": info, "pair_start": start, "pair_stop": stop[:N], "seg_start": seg[:N * (nel + 1)].reshape(N, nel + 1),
                "seg_close": int(seg[-1]), "pair_i": pi[:P], "pair_j": pj[:P], "pair_shift": ps[:P], "pair_rev": rev[:P],
                "blk_center": blk if nb > 0 else None}
