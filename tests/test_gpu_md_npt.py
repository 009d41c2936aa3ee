"""GPU: the Berendsen barostat of the device MD loop (`ta_md_set_barostat`, the kBaro builds of csrc/ta_md.hip)
against the NumPy reference (tests/md_npt_reference.py) driven by the CPU oracle or by a second engine's
`Engine.step(x, cells=h)`.

Parity bound 1e-9 (A, A per time unit, eV, eV / A^3): the bound and the reasoning of tests/test_gpu_md.py. The
scaling multiplies x and h by factors that carry the force bound's 1e-13 relative error through (beta / 3)
(dt / taup) = 0.015, far below it. Every comparison first asserts on the reference log that no staleness
decision is marginal (`assert_not_marginal`).

The anchor: 32 Ni atoms (fcc 2 x 2 x 2, jitter 0.02, seed 3), Zjw04, rc = 6, velocities
maxwell_boltzmann(kB 300, RandomState(3)), dt = 1 fs, Berendsen thermostat at 300 K with taut = 20 fs,
beta = 0.9 A^3 / eV. Figures of the reference with the oracle (P and V as the barostat of a step sees them):
  A  cell and atoms scaled 1.02, P0 = 0, taup = 20 fs, skin 0.5, 40 steps: no rebuild, P from -0.05581 eV / A^3
     (-8.94 GPa) to -0.00635, V from 371.53 to 356.09 A^3 at the last step, mu of step 0 0.99916283
  B  scaled 1.03, taup = 10 fs, skin 0.3, 36 steps: one rebuild, after the drift of step 11, by strain alone:
     lim = 0.0538, max |u| = 0.0592 (both far below skin / 2 = 0.15), plain displacement 0.2033; the next one
     would come at step 40
  C  mask (1, 1, 0), P0 = 5 GPa, scale 1.0, taup = 20 fs, 40 steps: no rebuild, V from 350.10 to 344.94
"""
import functools

import numpy as np
import pytest

from tests import md_npt_reference as npt
from tests import md_reference
from tests.helpers import fcc, make_eam, make_grap_nn, make_nn, oracle_eam_eval
from tensoralloy_amd import _lib, md
from tensoralloy_amd.atoms import atomic_masses

pytestmark = pytest.mark.gpu

DT = md.fs
TOL = 1e-9
WANT = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES | _lib.TA_WANT_VIRIAL
RC = 6.0
BETA = 0.9
THERMO = (md.kB * 300.0, 20 * DT)
KEYS = ("x", "v", "cells", "epot", "ekin", "volume", "press")
CASES = {  # scale, P0, taup, skin, steps, mask
    "A": (1.02, 0.0, 20 * DT, 0.5, 40, None),
    "B": (1.03, 0.0, 10 * DT, 0.3, 36, None),
    "C": (1.0, 5.0 * md.GPa, 20 * DT, 0.5, 40, (1, 1, 0)),
}


def _masses(frames):
    return np.array([atomic_masses[z] for a in frames for z in a.numbers], dtype=np.float64)


def _positions(frames):
    return np.concatenate([a.positions for a in frames])


def _cells(frames):
    return np.array([np.asarray(a.get_cell(complete=True)) for a in frames])


def _natoms(frames):
    return [len(a) for a in frames]


def _velocities(frames, T=300.0, seed=3):
    rng = np.random.RandomState(seed)
    return np.concatenate([md.maxwell_boltzmann(_masses([a]), md.kB * T, rng) for a in frames])


def _strained(atoms, strain):
    a = atoms.copy()
    a.set_cell(np.asarray(a.get_cell(complete=True)) @ (np.eye(3) * strain if np.isscalar(strain) else np.asarray(strain)),
               scale_atoms=True)
    return a


@functools.lru_cache(maxsize=None)
def _ni():
    return make_eam(["Ni"], RC, potential="zjw04")


@functools.lru_cache(maxsize=None)
def _anchor(scale=1.02):
    return _strained(fcc(rep=(2, 2, 2), jitter=0.02, seed=3), float(scale))


def _oracle_forces(nn, frames):
    """Callback of the reference: the CPU oracle, frame by frame."""
    natoms = _natoms(frames)

    def force(x, cells):
        e, f, w, a0 = [], [], [], 0
        for atoms, n, h in zip(frames, natoms, cells):
            a = atoms.copy()
            a.set_cell(h)
            a.positions[:] = x[a0:a0 + n]
            o = oracle_eam_eval(nn, a)
            e.append(o["energy"])
            f.append(o["forces"])
            w.append(o["virial"])
            a0 += n
        return np.array(e), np.concatenate(f), np.array(w)
    return force


def _engine_forces(other):
    """Callback from a second engine with skin 0 through `Engine.step(x, cells=h)`: a new list at every call."""
    def force(x, cells):
        r = other.step(np.ascontiguousarray(x), WANT, cells=np.ascontiguousarray(cells))
        return r["energy"].copy(), r["forces"].copy(), r["virial"].copy()
    return force


def _freeze(out):
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _reference(force, frames, v0, steps, p0, taup, skin, mask=None, thermostat=THERMO, **kw):
    kT0, tau = thermostat or (0.0, 0.0)
    ref = npt.run(force, _positions(frames), v0, _masses(frames), _cells(frames), DT, steps, p0, taup, BETA, mask=mask,
                  natoms=_natoms(frames), skin=skin, rc=RC, kT0=kT0, tau=tau, **kw)
    npt.assert_not_marginal(ref, skin)
    return ref


def _setup(eng, frames, v0, skin, barostat, thermostat=THERMO, langevin=None):
    eng.set_skin(skin)
    eng.set_frames(frames)
    eng.md_init(None, v0)
    if thermostat:
        eng.md_set_thermostat(*thermostat)
    if langevin:
        eng.md_set_langevin(*langevin)
    if barostat:
        eng.md_set_barostat(*barostat)


def _collect(eng, outs):
    x, v = eng.md_state()
    res = dict(x=x, v=v, cells=eng.md_cells(), n_rebuilds=sum(o["n_rebuilds"] for o in outs))
    for k in ("epot", "ekin", "volume", "press"):
        if k in outs[0]:
            res[k] = np.concatenate([o[k][1 if j else 0:] for j, o in enumerate(outs)])
    return res


def _device(nn, frames, v0, skin, steps, barostat, thermostat=THERMO, langevin=None, splits=None):
    """The state and the records of `steps` steps on the device (`splits`: in several md_run calls);
    `barostat` = (P0, taup, beta, mask)."""
    from tensoralloy_amd import Engine
    with Engine(nn) as eng:
        _setup(eng, frames, v0, skin, barostat, thermostat, langevin)
        return _collect(eng, [eng.md_run(n, DT) for n in (splits or [steps])])


def _assert_parity(dev, ref, tol=TOL, what="", keys=KEYS):
    gaps = {k: float(np.abs(dev[k] - ref[k]).max()) for k in keys}
    print("parity gaps", what, gaps, "rebuilds", dev["n_rebuilds"], ref.get("rebuild_steps"), ref.get("end_rebuild"))
    for k in keys:
        assert dev[k].shape == ref[k].shape, k
    for k, g in gaps.items():
        assert g < tol, gaps


def _assert_rebuilds(dev, ref):
    """The rebuilds the strain-aware rule asks for, and the one for the final cells where the run moved them."""
    assert dev["n_rebuilds"] == ref["n_rebuilds"] + int(ref["end_rebuild"]), (dev["n_rebuilds"], ref["rebuild_steps"],
                                                                              ref["end_rebuild"])


def _barostat_pressure(ref, case, k):
    """The (mean) pressure the barostat of step k saw, back from its factor."""
    _, p0, taup, _, _, _ = CASES[case]
    return p0 - (1.0 - ref["mu"][k, 0].mean()) / (DT / taup * BETA / 3.0)


@functools.lru_cache(maxsize=None)
def _case_inputs(case):
    scale, p0, taup, skin, steps, mask = CASES[case]
    atoms = _anchor(scale)
    return atoms, _velocities([atoms]), (p0, taup, BETA, mask)


@functools.lru_cache(maxsize=None)
def _case_reference(case):
    _, p0, taup, skin, steps, mask = CASES[case]
    atoms, v0, _ = _case_inputs(case)
    return _freeze(_reference(_oracle_forces(_ni(), [atoms]), [atoms], v0, steps, p0, taup, skin, mask=mask))


@functools.lru_cache(maxsize=None)
def _case_device(case):
    _, _, _, skin, steps, _ = CASES[case]
    atoms, v0, barostat = _case_inputs(case)
    return _freeze(_device(_ni(), [atoms], v0, skin, steps, barostat))


# -- A ---------------------------------------------------------------------------------------------------
def test_parity_without_rebuild(lib):
    ref, dev = _case_reference("A"), _case_device("A")
    assert ref["rebuild_steps"] == [] and ref["end_rebuild"]
    assert abs(_barostat_pressure(ref, "A", 0) - -0.05581) < 5e-6
    assert abs(_barostat_pressure(ref, "A", 0) / md.GPa - -8.94) < 5e-3
    assert abs(_barostat_pressure(ref, "A", 39) - -0.00635) < 5e-6
    assert abs(ref["volume"][0, 0] - 371.53) < 5e-3 and abs(ref["volume"][39, 0] - 356.09) < 5e-3
    assert np.abs(ref["mu"][0, 0] - 0.99916283).max() < 5e-9
    assert dev["epot"].shape == (41, 1) and dev["press"].shape == (41, 1, 3)
    _assert_parity(dev, ref, what="A")
    assert dev["n_rebuilds"] == 1   # the build for the final cells


# -- B ---------------------------------------------------------------------------------------------------
def test_rebuild_caused_by_strain_alone(lib):
    ref, dev = _case_reference("B"), _case_device("B")
    assert ref["rebuild_steps"] == [11] and ref["end_rebuild"]
    rec = ref["log"][10]
    assert rec["step"] == 11
    assert abs(rec["lim"][0] - 0.0538) < 5e-5 and abs(rec["umax"][0] - 0.0592) < 5e-5 and abs(rec["dmax"][0] - 0.2033) < 5e-5
    assert rec["lim"][0] < rec["umax"][0] < 0.15   # stale by the strain-aware rule, while |u| is far below skin / 2
    assert all(r["umax"][0] < 0.15 for r in ref["log"])
    assert dev["n_rebuilds"] == ref["n_rebuilds"] + 1
    _assert_parity(dev, ref, what="B")


# -- C ---------------------------------------------------------------------------------------------------
def test_mask(lib):
    ref, dev = _case_reference("C"), _case_device("C")
    atoms, _, _ = _case_inputs("C")
    assert ref["rebuild_steps"] == [] and ref["end_rebuild"]
    assert abs(ref["volume"][0, 0] - 350.10) < 5e-3 and abs(ref["volume"][39, 0] - 344.94) < 5e-3
    h0 = _cells([atoms])[0]
    assert np.array_equal(dev["cells"][0][:, 2], h0[:, 2]) and np.array_equal(ref["cells"][0][:, 2], h0[:, 2])
    assert np.abs(dev["cells"][0][:, :2] - h0[:, :2]).max() > 1e-2
    assert abs(dev["cells"][0][0, 0] - dev["cells"][0][1, 1]) > 1e-6   # each free axis has its own factor
    _assert_parity(dev, ref, what="C")
    assert dev["n_rebuilds"] == 1


# -- D ---------------------------------------------------------------------------------------------------
def test_without_thermostat(lib):
    _, p0, taup, skin, _, _ = CASES["A"]
    atoms, v0, barostat = _case_inputs("A")
    ref = _reference(_oracle_forces(_ni(), [atoms]), [atoms], v0, 30, p0, taup, skin, thermostat=None)
    dev = _device(_ni(), [atoms], v0, skin, 30, barostat, thermostat=None)
    _assert_rebuilds(dev, ref)
    _assert_parity(dev, ref, what="NPH")
    assert np.abs(dev["x"] - _case_device("A")["x"]).max() > 1e-6   # (the thermostat is missed)


def test_with_langevin(lib):
    from tensoralloy_amd import Engine
    _, p0, taup, skin, _, _ = CASES["A"]
    atoms, v0, barostat = _case_inputs("A")
    langevin = (md.kB * 300.0, 0.01 / DT, 20240611)
    with Engine(_ni()) as eng:
        _setup(eng, [atoms], v0, skin, barostat, thermostat=None, langevin=langevin)
        dev = _collect(eng, [eng.md_run(30, DT)])
        ref = _reference(_oracle_forces(_ni(), [atoms]), [atoms], v0, 30, p0, taup, skin, thermostat=None,
                         friction=langevin[1], lv_kT0=langevin[0], noise=eng.md_noise)
    _assert_rebuilds(dev, ref)
    _assert_parity(dev, ref, what="Langevin")


# -- E ---------------------------------------------------------------------------------------------------
def test_batch_of_unlike_frames(lib):
    """[the anchor (below the target pressure), 108 atoms in a triclinic cell, the anchor's lattice scaled 0.98
    (above it)]: every frame gets its own factors, as in its single-frame run and as the reference driven by a
    second engine."""
    from tensoralloy_amd import Engine
    nn = _ni()
    big = _strained(fcc(rep=(3, 3, 3), jitter=0.03, seed=4), [[0.98, 0, .01], [0, 1.02, 0], [0, 0, 1.0]])
    frames = [_anchor(1.02), big, _anchor(0.98)]
    natoms = _natoms(frames)
    assert natoms == [32, 108, 32]
    v0 = _velocities(frames, seed=11)
    _, p0, taup, skin, _, _ = CASES["A"]
    barostat = (p0, taup, BETA, None)
    with Engine(nn) as other:
        other.set_skin(0.0)
        other.set_frames(frames)
        ref = _reference(_engine_forces(other), frames, v0, 20, p0, taup, skin)
    dev = _device(nn, frames, v0, skin, 20, barostat)
    _assert_rebuilds(dev, ref)
    _assert_parity(dev, ref, what="batch")
    V0, V1 = dev["volume"][0], dev["volume"][-1]
    print("volumes", V0, V1, "pressures", dev["press"][0].mean(axis=1))
    assert V1[0] < V0[0] and V1[2] > V0[2] and dev["press"][0, 0].mean() < p0 < dev["press"][0, 2].mean()
    assert abs(dev["cells"][1][0, 2]) > 1e-2   # (the triclinic frame's off-diagonal entry is scaled with its column)
    start = np.concatenate([[0], np.cumsum(natoms)])
    for f, atoms in enumerate(frames):
        s = slice(start[f], start[f + 1])
        alone = _device(nn, [atoms], v0[s], skin, 20, barostat)
        gaps = dict(x=np.abs(alone["x"] - dev["x"][s]).max(), v=np.abs(alone["v"] - dev["v"][s]).max(),
                    cells=np.abs(alone["cells"][0] - dev["cells"][f]).max(),
                    epot=np.abs(alone["epot"][:, 0] - dev["epot"][:, f]).max(),
                    ekin=np.abs(alone["ekin"][:, 0] - dev["ekin"][:, f]).max(),
                    volume=np.abs(alone["volume"][:, 0] - dev["volume"][:, f]).max(),
                    press=np.abs(alone["press"][:, 0] - dev["press"][:, f]).max())
        print("frame", f, gaps)
        assert max(gaps.values()) < TOL, (f, gaps)


# -- F ---------------------------------------------------------------------------------------------------
def test_frame_above_1024_atoms(lib):
    """1372 atoms in one workgroup of 1024 threads: each thread meets several atoms."""
    from tensoralloy_amd import Engine
    nn = _ni()
    big = _strained(fcc(rep=(7, 7, 7), jitter=0.02, seed=8), 1.02)
    assert len(big) == 1372
    v0 = _velocities([big], seed=8)
    _, p0, taup, _, _, _ = CASES["A"]
    with Engine(nn) as other:
        other.set_skin(0.0)
        other.set_frames([big])
        ref = _reference(_engine_forces(other), [big], v0, 5, p0, taup, 0.3)
    dev = _device(nn, [big], v0, 0.3, 5, (p0, taup, BETA, None))
    _assert_rebuilds(dev, ref)
    _assert_parity(dev, ref, what="1372 atoms")
    assert dev["volume"][-1, 0] < 0.995 * dev["volume"][0, 0]


# -- G ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["sf_triangles", "sf_per_apex", "grap", "adp"])
def test_model_families(lib, family):
    """10 steps against a second engine. Periodic widths of the 2 x 2 x 2 frame: 7.19 A at scale 1.02 and 6.94 A
    at scale 0.985. With rc = 6.0 and skin 0.5 the former exceed rc + skin and the triangle-once backward pass
    runs; with rc = 6.45 the latter lie between rc and rc + skin, where a valid list no longer guarantees widths
    above rc, and the per-apex pass must run while the barostat is on. The randomly initialised SF network has a
    pressure of its own, of the order of -1 eV / A^3, which grows as the cell shrinks (by some 20 eV / A^3 per unit
    of linear strain), so no cell survives ten steps at P0 = 0: for it the target is the pressure of the initial
    state + 0.01 eV / A^3, from which the factors stay within 5e-3 of 1 over the ten steps."""
    from tensoralloy_amd import Engine
    rcut = 6.45 if family == "sf_per_apex" else 6.0
    if family.startswith("sf"):
        nn = make_nn(["Ni"], rcut, True, [8])
    elif family == "grap":
        nn = make_grap_nn(["Ni"], rcut, [16])
    else:
        nn = make_eam(["Ni"], rcut, adp=True)
    frames = [_anchor(0.985 if family == "sf_per_apex" else 1.02)]
    v0 = _velocities(frames)
    _, p0, taup, skin, _, _ = CASES["A"]
    with Engine(nn) as other:
        other.set_skin(0.0)
        other.set_frames(frames)
        if family.startswith("sf"):
            _, _, W = _engine_forces(other)(_positions(frames), _cells(frames))
            S, V = npt.frame_sums(_masses(frames), v0, [32]), npt.volumes(_cells(frames))
            p0 = float(((S - np.diagonal(W, axis1=1, axis2=2)) / V[:, None]).mean()) + 0.01
        ref = npt.run(_engine_forces(other), _positions(frames), v0, _masses(frames), _cells(frames), DT, 10, p0, taup,
                      BETA, natoms=[32], skin=skin, rc=rcut, kT0=THERMO[0], tau=THERMO[1])
    npt.assert_not_marginal(ref, skin)
    print(family, "P0", p0, "mu", ref["mu"][0, 0], ref["mu"][-1, 0], "V", ref["volume"][0, 0], ref["volume"][-1, 0])
    assert np.abs(ref["mu"] - 1.0).max() < 5e-3 and abs(ref["mu"][0, 0, 0] - 1.0) > 1e-4
    with Engine(nn) as eng:
        _setup(eng, frames, v0, skin, None)
        if family == "sf_per_apex":   # with fixed cells the widths admit the triangle pass
            eng.md_run(0, DT)
            assert eng.backward_variant() == 2
        eng.md_set_barostat(p0, taup, BETA)
        dev = _collect(eng, [eng.md_run(10, DT)])
        variant = eng.backward_variant()
    if family.startswith("sf"):
        assert variant == (2 if family == "sf_triangles" else 1), variant
    _assert_rebuilds(dev, ref)
    _assert_parity(dev, ref, what=family)


# -- H ---------------------------------------------------------------------------------------------------
def test_split_runs_and_hand_over(lib):
    """13 + 0 + 27 steps against 40: every run that moved the cells ends with the list for its final cells, so
    the next evaluates on another list than the whole run does, and the states agree up to summation order.
    Afterwards the host-side list state is that of the final cells."""
    from tensoralloy_amd import Engine
    nn = _ni()
    _, _, _, skin, steps, _ = CASES["A"]
    atoms, v0, barostat = _case_inputs("A")
    whole = _case_device("A")
    with Engine(nn) as eng:
        _setup(eng, [atoms], v0, skin, barostat)
        before = eng.list_stats()
        outs = [eng.md_run(n, DT) for n in (13, 0, 27)]
        after = eng.list_stats()
        split = _collect(eng, outs)
        assert [o["n_rebuilds"] for o in outs] == [1, 0, 1]   # (no mid-run rebuild in this case; the empty run moves no cell)
        assert np.abs(outs[1]["epot"] - outs[0]["epot"][-1:]).max() < TOL and outs[1]["volume"].shape == (1, 1)
        assert after[0] - before[0] == 2 and sum(after) - sum(before) == steps + 2
        _assert_parity(split, whole, what="13 + 0 + 27")
        # the list the run left is the one of the final cells
        final = atoms.copy()
        final.set_cell(split["cells"][0])
        final.positions[:] = split["x"]
        o = oracle_eam_eval(nn, final)
        again = eng.step(split["x"], WANT)
        assert sum(eng.list_stats()) - sum(after) == 1 and eng.list_stats()[0] == after[0]   # reused
        gaps = dict(energy=abs(again["energy"][0] - o["energy"]), forces=np.abs(again["forces"] - o["forces"]).max(),
                    virial=np.abs(again["virial"][0] - o["virial"]).max())
        print("step after the run", gaps)
        assert max(gaps.values()) < TOL, gaps
        assert np.array_equal(eng.md_cells()[0], split["cells"][0])
        # a fixed-cell run carries on from there
        eng.md_set_barostat(0.0, 0.0, 0.0)
        out = eng.md_run(5, DT)
        assert "volume" not in out
        x, v = eng.md_state()
        assert np.array_equal(eng.md_cells()[0], split["cells"][0])
        with pytest.raises(ValueError, match="had no barostat"):
            eng.md_records(6)

    def force(xx):
        a = final.copy()
        a.positions[:] = xx
        r = oracle_eam_eval(nn, a)
        return np.array([r["energy"]]), r["forces"]
    ref = md_reference.run(force, split["x"], split["v"], _masses([atoms]), DT, 5, kT0=THERMO[0], tau=THERMO[1])
    gaps = dict(x=np.abs(x - ref["x"]).max(), v=np.abs(v - ref["v"]).max(), epot=np.abs(out["epot"] - ref["epot"]).max(),
                ekin=np.abs(out["ekin"] - ref["ekin"]).max())
    print("fixed-cell run after the barostat", gaps)
    assert max(gaps.values()) < TOL, gaps


# -- I ---------------------------------------------------------------------------------------------------
def test_barostat_off_leaves_no_trace(lib):
    """Set and switched off again, the barostat leaves no trace: the arrays of a Berendsen NVT run are those of
    an engine that never had one, bit for bit."""
    from tensoralloy_amd import Engine
    _, _, _, skin, steps, _ = CASES["A"]
    atoms, v0, barostat = _case_inputs("A")
    plain = _device(_ni(), [atoms], v0, skin, steps, None)
    with Engine(_ni()) as eng:
        _setup(eng, [atoms], v0, skin, barostat)
        eng.md_set_barostat(0.0, 0.0, 0.0)
        out = eng.md_run(steps, DT)
        off = _collect(eng, [out])
    assert "volume" not in out and plain["n_rebuilds"] == off["n_rebuilds"]
    for k in ("x", "v", "cells", "epot", "ekin"):
        assert np.array_equal(plain[k], off[k]), k
    assert np.array_equal(off["cells"], _cells([atoms]))
    assert np.abs(plain["x"] - _case_device("A")["x"]).max() > 1e-3   # (the barostat itself is not a no-op)


# -- J ---------------------------------------------------------------------------------------------------
def test_refusals(lib):
    from tensoralloy_amd import Atoms, Engine
    nn = _ni()
    _, _, _, skin, _, _ = CASES["A"]
    atoms, v0, barostat = _case_inputs("A")
    p0, taup, beta, _ = barostat
    good = _device(nn, [atoms], v0, skin, 3, barostat)
    with Engine(nn) as eng:
        _setup(eng, [atoms], v0, skin, barostat)
        for args, what in [((float("nan"), taup, beta), "pressure must be finite"),
                           ((float("inf"), taup, beta), "pressure must be finite"),
                           ((p0, float("nan"), beta), "taup must be finite"),
                           ((p0, float("inf"), beta), "taup must be finite"),
                           ((p0, taup, -1.0), "compressibility must be finite and >= 0"),
                           ((p0, taup, float("nan")), "compressibility must be finite and >= 0"),
                           ((p0, taup, beta, (0, 0, 0)), "mask leaves no axis")]:
            with pytest.raises(ValueError, match=what):
                eng.md_set_barostat(*args)
        with pytest.raises(ValueError, match="three entries"):
            eng.md_set_barostat(p0, taup, beta, (1, 1))
        with pytest.raises(ValueError, match="had no barostat"):   # no run yet
            eng.md_records(1)
        same = _collect(eng, [eng.md_run(3, DT)])   # the refused calls left the setting as it was
        for k in KEYS:
            assert np.array_equal(good[k], same[k]), k
        eng.set_frames([atoms])                     # keeps the setting, drops the MD state
        with pytest.raises(ValueError, match="before ta_md_init"):
            eng.md_records(1)
        eng.md_init(None, v0)
        eng.md_set_thermostat(*THERMO)
        kept = _collect(eng, [eng.md_run(3, DT)])
        for k in KEYS:
            assert np.array_equal(good[k], kept[k]), k
    slab = atoms.copy()
    slab.pbc = [True, True, False]
    with Engine(nn) as eng:
        _setup(eng, [atoms, slab], np.concatenate([v0, v0]), skin, barostat)
        x0, vv0 = eng.md_state()
        stats = eng.list_stats()
        with pytest.raises(ValueError, match="frame 1 is not periodic along all three axes"):
            eng.md_run(3, DT)
        x1, vv1 = eng.md_state()
        assert np.array_equal(x0, x1) and np.array_equal(vv0, vv1) and eng.list_stats() == stats
        assert np.array_equal(eng.md_cells(), _cells([atoms, slab]))
        eng.md_set_barostat(0.0, 0.0, 0.0)   # without the barostat the batch runs
        assert eng.md_run(1, DT)["n_rebuilds"] == 0


# -- K ---------------------------------------------------------------------------------------------------
def test_device_md_driver(lib):
    """`DeviceMD` under the barostat: the cell of the `Atoms` follows without the atoms being scaled again, and
    the observers see volume and pressure."""
    from tensoralloy_amd import DeviceMD, Engine
    _, p0, taup, skin, steps, _ = CASES["A"]
    atoms, v0, _ = _case_inputs("A")
    atoms = atoms.copy()
    dev = _case_device("A")
    seen = []
    with Engine(_ni()) as eng:
        eng.set_skin(skin)
        dyn = DeviceMD(eng, atoms, DT, temperature_K=300.0, taut=20 * DT, velocities=v0, pressure=p0, taup=taup,
                       compressibility=BETA)
        assert abs(dyn.get_volume() - dev["volume"][0, 0]) < 1e-9 and dyn.n_rebuilds == 0
        assert abs(dyn.get_pressure() - dev["press"][0, 0].mean()) < 1e-15
        dyn.attach(lambda: seen.append((dyn.nsteps, dyn.get_volume(), dyn.get_pressure())), interval=15)
        dyn.run(steps)
        cell = dyn.get_cell()
    assert [s for s, _, _ in seen] == [15, 30]
    assert abs(seen[1][1] - dev["volume"][30, 0]) < 1e-9 and abs(seen[1][2] - dev["press"][30, 0].mean()) < TOL
    assert dyn.n_rebuilds == 3   # one build for the final cells of each of the three runs
    assert np.abs(atoms.positions - dev["x"]).max() < TOL and np.abs(dyn.velocities - dev["v"]).max() < TOL
    assert np.array_equal(np.asarray(atoms.get_cell(complete=True)), cell)
    assert np.abs(cell - dev["cells"][0]).max() < TOL
    assert abs(dyn.get_volume() - dev["volume"][-1, 0]) < 1e-9 and abs(dyn.get_pressure() - dev["press"][-1, 0].mean()) < TOL
    assert abs(dyn.get_potential_energy() - dev["epot"][-1, 0]) < TOL
