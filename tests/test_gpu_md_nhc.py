"""GPU: the Nose-Hoover chain thermostat of the device MD loop (`ta_md_set_nose_hoover`, the kNhc builds of
csrc/ta_md.hip) against the NumPy reference (tests/md_nhc_reference.py) driven by the CPU oracle or by a second
engine's `Engine.step`.

dt = 1 fs; tau = 20 dt, M = 3, L = 1 unless a test says otherwise. Parity bound 1e-9 on x, v, epot, ekin and
echain: the bound of tests/test_gpu_md.py by its own argument (the factor s adds two exp() of at most 2 ulp
per step); for eta and veta 1e-9 x max(1, max |reference|).
"""
import functools

import numpy as np
import pytest

from tests import md_nhc_reference as nhc
from tests.helpers import fcc, make_eam, make_grap_nn, make_nn
from tests.test_gpu_md import (DT, NI_CASES, TOL, WANT, _device_run as _nve_device_run, _masses, _ni_reference,
                               _ni_setup, _oracle_forces, _positions, _velocities)
from tests.test_gpu_sf import _alloy
from tensoralloy_amd import Atoms, md

pytestmark = pytest.mark.gpu

KT0, TAU = md.kB * 600.0, 20 * DT
TARGET_K = {"cold": 600.0, "hot": 2000.0}   # the cold case is heated; the hot one is held where it starts
KEYS = ("x", "v", "epot", "ekin", "echain")


def _device_run(nn, frames, v0, skin, steps, kT0=KT0, tau=TAU, splits=None, barostat=None, **chain):
    """The state, the chains and the records of `steps` steps on the device (`splits`: in several md_run calls)."""
    from tensoralloy_amd import Engine
    with Engine(nn) as eng:
        eng.set_skin(skin)
        eng.set_frames(frames)
        eng.md_init(None, v0)
        eng.md_set_nose_hoover(kT0, tau, **chain)
        if barostat:
            eng.md_set_barostat(*barostat)
        outs = [eng.md_run(n, DT) for n in (splits or [steps])]
        x, v = eng.md_state()
        eta, veta = eng.md_chain()
        res = dict(x=x, v=v, eta=eta, veta=veta, n_rebuilds=sum(o["n_rebuilds"] for o in outs))
        if barostat:
            res["cells"] = eng.md_cells()
    for k in ("epot", "ekin", "echain", "volume", "press"):
        if k in outs[0]:
            res[k] = np.concatenate([o[k][1 if j else 0:] for j, o in enumerate(outs)])
    return res


def _assert_parity(dev, ref, tol=TOL, keys=KEYS):
    gaps = {k: float(np.abs(dev[k] - ref[k]).max()) for k in keys + ("eta", "veta")}
    print("parity gaps", gaps, "rebuilds", dev["n_rebuilds"], ref["n_rebuilds"])
    for k in keys + ("eta", "veta"):
        assert dev[k].shape == ref[k].shape, k
    for k in keys:
        assert gaps[k] < tol, gaps
    for k in ("eta", "veta"):
        assert gaps[k] < tol * max(1.0, float(np.abs(ref[k]).max())), gaps


def _engine_forces(other):
    def force(x):
        r = other.step(x, WANT)
        return r["energy"].copy(), r["forces"].copy()
    return force


def _freeze(out):
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _ni_nhc_reference(case):
    nn, atoms = _ni_setup()
    T, skin, steps = NI_CASES[case]
    v0 = _velocities([atoms], T, 3)
    return v0, _freeze(nhc.run(_oracle_forces(nn, [atoms]), atoms.positions, v0, _masses([atoms]), DT, steps,
                               md.kB * TARGET_K[case], TAU, skin=skin))


@functools.lru_cache(maxsize=None)
def _ni_nhc_device(case):
    nn, atoms = _ni_setup()
    T, skin, steps = NI_CASES[case]
    v0, _ = _ni_nhc_reference(case)
    return _freeze(_device_run(nn, [atoms], v0, skin, steps, kT0=md.kB * TARGET_K[case]))


# -- 1, 2 ------------------------------------------------------------------------------------------------
def test_parity_with_the_oracle_without_rebuild(lib):
    _, ref = _ni_nhc_reference("cold")
    dev = _ni_nhc_device("cold")
    assert ref["n_rebuilds"] == 0 and dev["n_rebuilds"] == 0
    assert dev["echain"].shape == (41, 1) and dev["eta"].shape == (1, 3)
    _assert_parity(dev, ref)
    _, nve = _ni_reference("cold")
    assert np.abs(dev["v"] - nve["v"]).max() > 1e-4   # (the thermostat is not a bystander)


def test_parity_with_rebuilds_mid_run(lib):
    """2000 K, held at 2000 K. Launches enqueued behind a stale list return before they touch the chain: a chain
    advanced by a skipped launch would show here."""
    _, ref = _ni_nhc_reference("hot")
    dev = _ni_nhc_device("hot")
    assert ref["rebuild_steps"] == [4, 8, 12, 17, 22, 28, 34, 39, 44, 49, 53, 57]
    assert dev["n_rebuilds"] == ref["n_rebuilds"] and 2 <= dev["n_rebuilds"] < 60
    _assert_parity(dev, ref)


# -- 3 ---------------------------------------------------------------------------------------------------
def test_split_runs(lib):
    """10 + 20 steps against 30 in one call. The second run gets K of its first launch by reduction where the
    whole run has s1^2 K: a 1e-16 relative difference with nothing to amplify it in 20 fs."""
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 2000.0, 3)
    kT0 = md.kB * TARGET_K["hot"]
    whole = _device_run(nn, [atoms], v0, 0.1, 30, kT0=kT0)
    split = _device_run(nn, [atoms], v0, 0.1, 30, kT0=kT0, splits=[10, 20])
    assert split["n_rebuilds"] == whole["n_rebuilds"] >= 2
    _assert_parity(split, whole, tol=1e-12)
    ref = nhc.run(_oracle_forces(nn, [atoms]), atoms.positions, v0, _masses([atoms]), DT, 30, kT0, TAU, skin=0.1)
    assert whole["n_rebuilds"] == ref["n_rebuilds"]
    _assert_parity(whole, ref)


# -- 4 ---------------------------------------------------------------------------------------------------
def test_skin_zero_rebuilds_at_every_step(lib):
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 300.0, 3)
    ref = nhc.run(_oracle_forces(nn, [atoms]), atoms.positions, v0, _masses([atoms]), DT, 5, KT0, TAU, skin=0.0)
    dev = _device_run(nn, [atoms], v0, 0.0, 5)
    assert dev["n_rebuilds"] == 5 and ref["n_rebuilds"] == 5
    _assert_parity(dev, ref)


# -- 5 ---------------------------------------------------------------------------------------------------
def test_frame_above_1024_atoms(lib):
    """1372 atoms in one workgroup of 1024 threads: threads stride over the atoms."""
    from tensoralloy_amd import Engine
    nn = make_eam(["Ni"], 6.0, potential="zjw04")
    frames = [fcc(rep=(7, 7, 7), jitter=0.02, seed=3)]
    assert len(frames[0]) == 1372
    v0 = _velocities(frames, 300.0, 5)
    with Engine(nn) as other:
        other.set_skin(0.0)
        other.set_frames(frames)
        ref = nhc.run(_engine_forces(other), _positions(frames), v0, _masses(frames), DT, 10, KT0, TAU, skin=0.3)
    dev = _device_run(nn, frames, v0, 0.3, 10)
    assert dev["n_rebuilds"] == ref["n_rebuilds"]
    _assert_parity(dev, ref)


# -- 6 ---------------------------------------------------------------------------------------------------
def test_batch_of_unlike_frames(lib):
    """Four frames at once, every one with its own chain. The lone atom (g = 3) feels no force: its epot is
    constant and its trajectory that of a force-free one-atom reference run."""
    nn = make_eam(["Mo", "Ni"], 6.0, potential="zjw04")
    lone = Atoms(symbols=["Ni"], positions=[[10.0, 10.0, 10.0]], cell=np.diag([20.0, 20.0, 20.0]), pbc=True)
    frames = [fcc(rep=(2, 2, 2), jitter=0.02, seed=3), _alloy(["Ni", "Mo"], rep=(2, 2, 3)),
              fcc(rep=(3, 3, 3), jitter=0.02, seed=4), lone]
    natoms = [len(a) for a in frames]
    assert natoms == [32, 48, 108, 1]
    v0 = _velocities(frames, 300.0, 11)
    v0[-1] = [0.01, -0.02, 0.03]
    dev = _device_run(nn, frames, v0, 0.3, 20)
    ref = nhc.run(_oracle_forces(nn, frames), _positions(frames), v0, _masses(frames), DT, 20, KT0, TAU, natoms=natoms)
    assert dev["eta"].shape == (4, 3) and dev["echain"].shape == (21, 4)
    _assert_parity(dev, ref)
    for f in range(4):   # no two chains alike
        for j in range(f):
            assert np.abs(dev["veta"][f] - dev["veta"][j]).max() > 1e-6, (f, j)
    assert np.all(dev["epot"][:, 3] == dev["epot"][0, 3])
    free = lambda x: (np.zeros(1), np.zeros_like(x))
    alone = nhc.run(free, lone.positions, v0[-1:], _masses([lone]), DT, 20, KT0, TAU)
    gaps = dict(x=np.abs(alone["x"] - dev["x"][-1:]).max(), v=np.abs(alone["v"] - dev["v"][-1:]).max(),
                ekin=np.abs(alone["ekin"][:, 0] - dev["ekin"][:, 3]).max(),
                echain=np.abs(alone["echain"][:, 0] - dev["echain"][:, 3]).max(),
                veta=np.abs(alone["veta"][0] - dev["veta"][3]).max())
    print("lone atom", gaps)
    assert max(gaps.values()) < 1e-12, gaps
    assert np.abs(dev["v"][-1] - v0[-1]).max() > 1e-6   # (its chain acts on it)


# -- 7 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", [dict(chain=1), dict(chain=8, loops=4), dict(dof_removed=3)],
                         ids=["M1", "M8_L4", "dof3"])
def test_chain_shapes(lib, chain):
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 300.0, 3)
    ref = nhc.run(_oracle_forces(nn, [atoms]), atoms.positions, v0, _masses([atoms]), DT, 20, KT0, TAU, skin=0.5, **chain)
    dev = _device_run(nn, [atoms], v0, 0.5, 20, **chain)
    assert dev["eta"].shape == (1, chain.get("chain", 3))
    _assert_parity(dev, ref)


# -- 8 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["sf", "grap"])
def test_model_families(lib, family):
    from tensoralloy_amd import Engine
    if family == "sf":
        nn, frames = make_nn(["Ni"], 6.0, True, [8]), [fcc(rep=(2, 2, 2), jitter=0.02, seed=3)]
    else:
        nn, frames = make_grap_nn(["Ni"], 6.0, [16]), [fcc(rep=(2, 2, 2), jitter=0.02, seed=3)]
    v0 = _velocities(frames, 300.0, 5)
    with Engine(nn) as other:
        other.set_skin(0.0)
        other.set_frames(frames)
        ref = nhc.run(_engine_forces(other), _positions(frames), v0, _masses(frames), DT, 20, KT0, TAU, skin=0.3)
    dev = _device_run(nn, frames, v0, 0.3, 20)
    assert dev["n_rebuilds"] == ref["n_rebuilds"]
    _assert_parity(dev, ref)


# -- 9 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [None, (1, 0, 1)], ids=["isotropic", "masked"])
def test_with_the_barostat(lib, mask):
    """The anchor case of tests/test_gpu_md_npt.py (case A) under this thermostat, 20 steps: the opening
    half-update is the thermostat's velocity part of the barostat's order."""
    from tests import test_gpu_md_npt as t_npt
    _, p0, taup, skin, _, _ = t_npt.CASES["A"]
    atoms, v0, _ = t_npt._case_inputs("A")
    oracle = t_npt._oracle_forces(t_npt._ni(), [atoms])
    ref = nhc.run(oracle, atoms.positions, v0, _masses([atoms]), DT, 20, KT0, TAU, skin=skin,
                  barostat=dict(pressure=p0, taup=taup, beta=t_npt.BETA, mask=mask, cells=t_npt._cells([atoms]),
                                rc=t_npt.RC))
    dev = _device_run(t_npt._ni(), [atoms], v0, skin, 20, barostat=(p0, taup, t_npt.BETA, mask))
    assert dev["n_rebuilds"] == ref["n_rebuilds"] + int(ref["end_rebuild"])
    _assert_parity(dev, ref, tol=t_npt.TOL, keys=KEYS + ("cells", "volume", "press"))
    h0 = t_npt._cells([atoms])[0]
    assert np.abs(dev["cells"][0][:, 0] - h0[:, 0]).max() > 1e-3
    if mask is not None:
        assert np.array_equal(dev["cells"][0][:, 1], h0[:, 1])


# -- 10 --------------------------------------------------------------------------------------------------
def test_chain_round_trip_and_restart(lib):
    from tensoralloy_amd import Engine
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 300.0, 3)
    dev = _ni_nhc_device("cold")
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        eng.set_frames([atoms])
        eng.md_init(None, v0)
        eng.md_set_nose_hoover(KT0, TAU)
        eta, veta = eng.md_chain()
        assert eta.shape == (1, 3) and not eta.any() and not veta.any()   # md_init left the chain at rest
        put_eta, put_veta = np.array([[0.1, -0.2, 0.3]]), np.array([[-0.01, 0.02, 0.03]])
        eng.md_set_chain(put_eta, put_veta)
        eta, veta = eng.md_chain()
        assert np.array_equal(eta, put_eta) and np.array_equal(veta, put_veta)
        eng.md_set_chain(veta=put_veta)   # (None = zeros)
        eta, veta = eng.md_chain()
        assert not eta.any() and np.array_equal(veta, put_veta)
        eng.md_set_chain()
        first = eng.md_run(15, DT)
        x, v = eng.md_state()
        eta, veta = eng.md_chain()
        assert np.abs(veta).max() > 1e-6
    cut = atoms.copy()
    cut.positions[:] = x
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        eng.md_set_nose_hoover(KT0, TAU)
        eng.set_frames([cut])     # (keeps the setting)
        eng.md_init(None, v)      # (zeroes the chain)
        assert not eng.md_chain()[1].any()
        eng.md_set_chain(eta, veta)
        second = eng.md_run(25, DT)
        x2, v2 = eng.md_state()
        eta2, veta2 = eng.md_chain()
    res = dict(x=x2, v=v2, eta=eta2, veta=veta2, n_rebuilds=0)
    for k in ("epot", "ekin", "echain"):
        res[k] = np.concatenate([first[k], second[k][1:]])
    _assert_parity(res, dev, tol=1e-12)


# -- 11 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("berendsen", [False, True])
def test_existing_path_untouched(lib, berendsen):
    """Switched on, used, and switched off again: the velocity-Verlet / Berendsen run that follows is the run
    of an engine that never heard of it, bit for bit."""
    from tensoralloy_amd import Engine
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 300.0, 3)

    def run(eng):
        eng.set_frames([atoms])
        eng.md_init(None, v0)
        if berendsen:
            eng.md_set_thermostat(KT0, TAU)
        out = eng.md_run(40, DT)
        assert "echain" not in out
        x, v = eng.md_state()
        return dict(x=x, v=v, epot=out["epot"], ekin=out["ekin"])

    with Engine(nn) as eng:
        eng.set_skin(0.5)
        fresh = run(eng)
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        eng.set_frames([atoms])
        eng.md_init(None, v0)
        eng.md_set_nose_hoover(KT0, TAU)
        assert "echain" in eng.md_run(3, DT)
        eng.md_set_nose_hoover(0.0)
        after = run(eng)
    for k in ("x", "v", "epot", "ekin"):
        assert np.array_equal(fresh[k], after[k]), k
    assert np.abs(fresh["x"] - atoms.positions).max() > 1e-3


# -- 12 --------------------------------------------------------------------------------------------------
def test_device_md_driver(lib):
    """`DeviceMD(..., tdamp=)`: runs cut at the observers' intervals continue the chain."""
    from tensoralloy_amd import DeviceMD, Engine
    nn, atoms = _ni_setup()
    atoms = atoms.copy()
    v0, _ = _ni_nhc_reference("cold")
    dev = _ni_nhc_device("cold")
    seen = []
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        dyn = DeviceMD(eng, atoms, DT, temperature_K=600.0, tdamp=TAU, velocities=v0)
        assert dyn.get_conserved_energy() == dev["ekin"][0, 0] + dev["epot"][0, 0]
        dyn.attach(lambda: seen.append((dyn.nsteps, dyn.get_kinetic_energy(), dyn.get_conserved_energy())), interval=15)
        dyn.run(40)
        assert [s for s, _, _ in seen] == [15, 30]
        for step, ekin, h in seen:
            assert abs(ekin - dev["ekin"][step, 0]) < 1e-12
            assert abs(h - (dev["ekin"] + dev["epot"] + dev["echain"])[step, 0]) < 1e-12
        assert np.abs(atoms.positions - dev["x"]).max() < 1e-12 and np.abs(dyn.velocities - dev["v"]).max() < 1e-12
        assert dyn.get_conserved_energy() == dyn.ekin[0] + dyn.epot[0] + dyn.echain[0]
        assert abs(dyn.get_conserved_energy() - (dev["ekin"] + dev["epot"] + dev["echain"])[-1, 0]) < 1e-12
        assert np.abs(eng.md_chain()[1] - dev["veta"]).max() < 1e-12
        # a Berendsen driver on the same engine afterwards: the constructor switched this thermostat off
        other = DeviceMD(eng, _ni_setup()[1].copy(), DT, temperature_K=600.0, taut=TAU, velocities=v0)
        other.run(5)
        with pytest.raises(ValueError, match="Nose-Hoover chain thermostat is off"):
            other.get_conserved_energy()
        with pytest.raises(ValueError, match="thermostat is off"):
            eng.md_chain()
    ber = _nve_device_run(nn, [_ni_setup()[1]], v0, 0.5, 5, thermostat=(KT0, TAU))
    assert np.abs(other.velocities - ber["v"]).max() < 1e-12


# -- 13 --------------------------------------------------------------------------------------------------
def test_refusals(lib):
    from tensoralloy_amd import Engine
    nn, atoms = _ni_setup()
    nan, inf = float("nan"), float("inf")
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        eng.md_set_nose_hoover(KT0, TAU, chain=2, loops=2, dof_removed=3)
        for kw, what in ((dict(kT=nan), "kT0 must be finite"), (dict(kT=inf), "kT0 must be finite"),
                         (dict(tau=0.0), "tau must be"), (dict(tau=-1.0), "tau must be"), (dict(tau=nan), "tau must be"),
                         (dict(tau=inf), "tau must be"), (dict(chain=0), "chain must be 1 .. 8"),
                         (dict(chain=9), "chain must be 1 .. 8"), (dict(loops=0), "loops must be 1 .. 16"),
                         (dict(loops=17), "loops must be 1 .. 16"), (dict(dof_removed=-1), "dof_removed must be >= 0")):
            args = dict(kT=KT0, tau=TAU)
            args.update(kw)
            with pytest.raises(ValueError, match="ta_md_set_nose_hoover: " + what):
                eng.md_set_nose_hoover(**args)
        # one thermostat at a time, in both directions; the refused calls left the setting as it was
        with pytest.raises(ValueError, match="ta_md_set_thermostat: the Nose-Hoover chain thermostat is on"):
            eng.md_set_thermostat(KT0, TAU)
        with pytest.raises(ValueError, match="ta_md_set_langevin: the Nose-Hoover chain thermostat is on"):
            eng.md_set_langevin(KT0, 0.01 / DT, 1)
        eng.md_set_thermostat(0.0, 0.0)        # switching off is always allowed
        eng.md_set_langevin(0.0, 0.0, 0)
        eng.set_frames([atoms])
        with pytest.raises(ValueError, match="ta_md_get_chain called before ta_md_init"):
            eng.md_chain()
        with pytest.raises(ValueError, match="ta_md_set_chain called before ta_md_init"):
            eng.md_set_chain()
        eng.md_init()
        assert eng.md_chain()[0].shape == (1, 2)   # (chain = 2 survived the refused calls)
        with pytest.raises(ValueError, match="eta"):
            eng.md_set_chain(np.zeros((1, 3)))
        with pytest.raises(ValueError, match="non-finite veta"):
            eng.md_set_chain(None, np.array([[0.0, nan]]))
        eng.md_set_nose_hoover(0.0)
        with pytest.raises(ValueError, match="thermostat is off"):
            eng.md_chain()
        out = eng.md_run(1, DT)
        assert "echain" not in out
        eng.md_set_thermostat(KT0, TAU)
        with pytest.raises(ValueError, match="ta_md_set_nose_hoover: the Berendsen thermostat is on"):
            eng.md_set_nose_hoover(KT0, TAU)
        eng.md_set_thermostat(0.0, 0.0)
        eng.md_set_langevin(KT0, 0.01 / DT, 1)
        with pytest.raises(ValueError, match="ta_md_set_nose_hoover: the Langevin thermostat is on"):
            eng.md_set_nose_hoover(KT0, TAU)
        eng.md_set_nose_hoover(0.0)            # ... off stays allowed
        eng.md_set_langevin(0.0, 0.0, 0)
        # g < 1: a lone atom with dof_removed = 3
        lone = Atoms(symbols=["Ni"], positions=[[10.0, 10.0, 10.0]], cell=np.diag([20.0, 20.0, 20.0]), pbc=True)
        eng.md_set_nose_hoover(KT0, TAU, dof_removed=3)
        eng.set_frames([atoms, lone])
        eng.md_init()
        with pytest.raises(ValueError, match="frame 1 has fewer than one degree of freedom"):
            eng.md_run(1, DT)
        eng.md_set_nose_hoover(KT0, TAU, dof_removed=2)
        assert eng.md_run(1, DT)["echain"].shape == (2, 2)


# -- 14 --------------------------------------------------------------------------------------------------
def test_thermalisation(lib):
    """256 Ni atoms from 300 K to a 900 K target, dt = 2 fs, tau = 50 fs, 2000 steps, on the device alone. With
    sigma_T / T = sqrt(2 / 3N) = 5.1 % and about 20 independent samples of length 2 tau in the second half, the
    standard error of the mean temperature is about 1.1 %: 5 % is more than 4 standard errors. H' wanders at
    most 5 x what E does in an NVE device run of the same length from the same start (the condition of the CPU
    test on the 32-atom case; the NumPy reference with the CPU oracle gives 898.0 K and 3.5 x on this case)."""
    from tensoralloy_amd import Engine
    nn = make_eam(["Ni"], 6.0, potential="zjw04")
    frames = [fcc(rep=(4, 4, 4))]
    n = len(frames[0])
    assert n == 256
    v0 = _velocities(frames, 300.0, 7)
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        eng.set_frames(frames)
        eng.md_init(None, v0)
        nve = eng.md_run(2000, 2 * DT)
        eng.set_frames(frames)
        eng.md_init(None, v0)
        eng.md_set_nose_hoover(md.kB * 900.0, 50 * DT)
        out = eng.md_run(2000, 2 * DT)
    T = 2.0 * out["ekin"][:, 0] / (3 * n * md.kB)
    H = (out["ekin"] + out["epot"] + out["echain"])[:, 0]
    E = (nve["ekin"] + nve["epot"])[:, 0]
    d_H, d_E = np.abs(H - H[0]).max(), np.abs(E - E[0]).max()
    print("mean T of the second half", T[1000:].mean(), "start", T[0], "excursion of H'", d_H, "of E (NVE)", d_E,
          "ratio", d_H / d_E)
    assert abs(T[1000:].mean() - 900.0) < 0.05 * 900.0
    assert d_E > 0.0 and d_H <= 5.0 * d_E
