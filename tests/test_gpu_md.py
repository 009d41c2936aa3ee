"""GPU: the device-resident MD loop (`ta_md_run`, csrc/ta_md.hip) against the NumPy reference loop
(tests/md_reference.py) driven by the CPU oracle or by a second engine's `Engine.step`.

Every case: dt = 1 fs, tens of steps, at most 108 atoms per frame. Parity bound 1e-9 (A, A per time unit,
eV): the fp64 force bounds of the project give about 1e-13 per step in v, so 1e-9 is >= 100 x the rounding
accumulated over 40 steps and about 10^4 below what one missing half-kick moves an atom in one step (4e-5 A).
"""
import functools

import numpy as np
import pytest

from tests import md_reference
from tests.helpers import fcc, make_eam, make_grap_nn, make_nn, oracle_eam_eval
from tests.test_gpu_sf import _alloy
from tensoralloy_amd import Atoms, _lib, md
from tensoralloy_amd.atoms import atomic_masses

pytestmark = pytest.mark.gpu

DT = md.fs
TOL = 1e-9
WANT = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES


def _masses(frames):
    return np.array([atomic_masses[z] for a in frames for z in a.numbers], dtype=np.float64)


def _velocities(frames, T, seed):
    rng = np.random.RandomState(seed)
    return np.concatenate([md.maxwell_boltzmann(_masses([a]), md.kB * T, rng) for a in frames])


def _positions(frames):
    return np.concatenate([a.positions for a in frames])


def _oracle_forces(nn, frames):
    """Force callback of the reference loop: the CPU oracle, frame by frame."""
    natoms = [len(a) for a in frames]

    def force(x):
        e, f, a0 = [], [], 0
        for atoms, n in zip(frames, natoms):
            a = atoms.copy()
            a.positions[:] = x[a0:a0 + n]
            o = oracle_eam_eval(nn, a)
            e.append(o["energy"])
            f.append(o["forces"])
            a0 += n
        return np.array(e), np.concatenate(f)
    return force


def _device_run(nn, frames, v0, skin, steps, thermostat=None, splits=None):
    """x, v, epot, ekin, n_rebuilds of `steps` steps on the device (`splits`: in several md_run calls)."""
    from tensoralloy_amd import Engine
    with Engine(nn) as eng:
        eng.set_skin(skin)
        eng.set_frames(frames)
        eng.md_init(None, v0)
        if thermostat:
            eng.md_set_thermostat(*thermostat)
        epot, ekin, rebuilds = [], [], 0
        for k, n in enumerate(splits or [steps]):
            out = eng.md_run(n, DT)
            epot.append(out["epot"][1 if k else 0:])
            ekin.append(out["ekin"][1 if k else 0:])
            rebuilds += out["n_rebuilds"]
        x, v = eng.md_state()
    return dict(x=x, v=v, epot=np.concatenate(epot), ekin=np.concatenate(ekin), n_rebuilds=rebuilds)


def _assert_parity(dev, ref, tol=TOL):
    gaps = {k: float(np.abs(dev[k] - ref[k]).max()) for k in ("x", "v", "epot", "ekin")}
    print("parity gaps", gaps, "rebuilds", dev["n_rebuilds"], ref["n_rebuilds"])
    assert dev["epot"].shape == ref["epot"].shape and dev["ekin"].shape == ref["ekin"].shape
    for k, g in gaps.items():
        assert g < tol, gaps


# -- the Ni zjw04 cases shared by several tests: (temperature, skin, steps) ---------------------------
NI_CASES = {"cold": (300.0, 0.5, 40), "hot": (2000.0, 0.1, 60)}


@functools.lru_cache(maxsize=None)
def _ni_setup():
    nn = make_eam(["Ni"], 6.0, potential="zjw04")
    atoms = fcc(rep=(2, 2, 2), jitter=0.02, seed=3)
    return nn, atoms


@functools.lru_cache(maxsize=None)
def _ni_reference(case, berendsen=False):
    nn, atoms = _ni_setup()
    T, skin, steps = NI_CASES[case]
    v0 = _velocities([atoms], T, 3)
    kw = dict(kT0=md.kB * 600.0, tau=20 * DT) if berendsen else {}
    ref = md_reference.run(_oracle_forces(nn, [atoms]), atoms.positions, v0, _masses([atoms]), DT, steps,
                           skin=skin, **kw)
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return v0, ref


@functools.lru_cache(maxsize=None)
def _ni_device(case):
    nn, atoms = _ni_setup()
    T, skin, steps = NI_CASES[case]
    v0, _ = _ni_reference(case)
    return _device_run(nn, [atoms], v0, skin, steps)


def test_parity_with_the_oracle_without_rebuild(lib):
    _, ref = _ni_reference("cold")
    dev = _ni_device("cold")
    assert ref["n_rebuilds"] == 0 and dev["n_rebuilds"] == 0
    assert dev["epot"].shape == (41, 1)
    _assert_parity(dev, ref)


def test_parity_with_rebuilds_mid_run(lib):
    _, ref = _ni_reference("hot")
    dev = _ni_device("hot")
    assert ref["rebuild_steps"] == [4, 8, 12, 17, 23, 30, 37, 43, 49, 54, 59]  # (steps after whose drift)
    assert 2 <= dev["n_rebuilds"] < 60
    assert dev["n_rebuilds"] == ref["n_rebuilds"]
    _assert_parity(dev, ref)


@pytest.mark.parametrize("family", ["sf", "grap", "adp"])
def test_model_families(lib, family):
    """SF G2+G4 runs on the exact list filtered from the skin list, GRAP and ADP on the skin list itself.
    Reference forces: a second engine with skin 0 through `Engine.step` (an exact list at every step)."""
    from tensoralloy_amd import Engine
    if family == "sf":
        nn, frames = make_nn(["Ni"], 6.0, True, [8]), [fcc(rep=(2, 2, 2), jitter=0.02, seed=3)]
    elif family == "grap":
        nn, frames = make_grap_nn(["Ni"], 6.0, [16]), [fcc(rep=(2, 2, 2), jitter=0.02, seed=3)]
    else:
        nn, frames = make_eam(["Mo", "Ni"], 5.5, adp=True), [_alloy(["Ni", "Mo"], rep=(2, 2, 2))]
    v0 = _velocities(frames, 600.0, 5)
    with Engine(nn) as other:
        other.set_skin(0.0)
        other.set_frames(frames)

        def force(x):
            r = other.step(x, WANT)
            return r["energy"].copy(), r["forces"].copy()
        ref = md_reference.run(force, _positions(frames), v0, _masses(frames), DT, 20, skin=0.3)
    dev = _device_run(nn, frames, v0, 0.3, 20)
    assert dev["n_rebuilds"] == ref["n_rebuilds"]
    _assert_parity(dev, ref)


def test_batch_of_unlike_frames(lib):
    """Four frames at once, 108 atoms (no multiple of 64) and a lone atom without any pair among them: every
    frame as when run alone on the device (1e-12) and as the host reference (1e-9)."""
    nn = make_eam(["Mo", "Ni"], 6.0, potential="zjw04")
    lone = Atoms(symbols=["Ni"], positions=[[10.0, 10.0, 10.0]], cell=np.diag([20.0, 20.0, 20.0]), pbc=True)
    frames = [fcc(rep=(2, 2, 2), jitter=0.02, seed=3), _alloy(["Ni", "Mo"], rep=(2, 2, 3)),
              fcc(rep=(3, 3, 3), jitter=0.02, seed=4), lone]
    natoms = [len(a) for a in frames]
    assert natoms == [32, 48, 108, 1]
    v0 = _velocities(frames, 600.0, 11)
    v0[-1] = [0.01, -0.02, 0.03]
    dev = _device_run(nn, frames, v0, 0.3, 20)
    ref = md_reference.run(_oracle_forces(nn, frames), _positions(frames), v0, _masses(frames), DT, 20,
                           natoms=natoms)
    _assert_parity(dev, ref)
    a = 0
    for f, (atoms, n) in enumerate(zip(frames, natoms)):
        alone = _device_run(nn, [atoms], v0[a:a + n], 0.3, 20)
        gaps = dict(x=np.abs(alone["x"] - dev["x"][a:a + n]).max(), v=np.abs(alone["v"] - dev["v"][a:a + n]).max(),
                    epot=np.abs(alone["epot"][:, 0] - dev["epot"][:, f]).max(),
                    ekin=np.abs(alone["ekin"][:, 0] - dev["ekin"][:, f]).max())
        print("frame", f, gaps)
        assert max(gaps.values()) < 1e-12, (f, gaps)
        a += n
    # the lone atom feels no force: its velocity and kinetic energy do not change by a bit
    assert np.array_equal(dev["v"][-1], v0[-1])
    assert np.all(dev["ekin"][:, 3] == dev["ekin"][0, 3]) and dev["ekin"][0, 3] > 0.0
    assert np.all(dev["epot"][:, 3] == dev["epot"][0, 3])


def test_berendsen(lib):
    nn, atoms = _ni_setup()
    v0, ref = _ni_reference("cold", True)
    dev = _device_run(nn, [atoms], v0, 0.5, 40, thermostat=(md.kB * 600.0, 20 * DT))
    _assert_parity(dev, ref)
    to_K = 2.0 / (3 * len(atoms) * md.kB)
    T0, T_ref, T_dev = ref["ekin"][0, 0] * to_K, ref["ekin"][-1, 0] * to_K, dev["ekin"][-1, 0] * to_K
    print("temperatures", T0, T_ref, T_dev)
    assert T0 < T_ref < 600.0       # the reference heats towards the target
    assert T_dev - T0 >= (T_ref - T0) * (1.0 - 1e-6)
    _, nve = _ni_reference("cold")
    assert T_ref > nve["ekin"][-1, 0] * to_K   # ... which the run without a thermostat does not


def test_split_runs_and_host_coherence(lib):
    """30 steps = 10 + 20 steps (with list rebuilds on the way), and the host-side list state after a run is
    what a host-driven loop would have left: `Engine.step` at the final positions gives the forces of the run."""
    from tensoralloy_amd import Engine
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 2000.0, 3)
    whole = _device_run(nn, [atoms], v0, 0.1, 30)
    with Engine(nn) as eng:
        eng.set_skin(0.1)
        info = eng.set_frames([atoms])
        eng.md_init(None, v0)
        generation = eng.batch_generation
        before = sum(eng.list_stats())
        a = eng.md_run(10, DT)
        b = eng.md_run(20, DT)
        assert eng.batch_generation == generation + 2
        assert sum(eng.list_stats()) - before == 30
        x, v = eng.md_state()
        left = eng.fetch(WANT)
        assert a["n_rebuilds"] + b["n_rebuilds"] == whole["n_rebuilds"] >= 2
        assert int(eng.info.n_pairs) > 0 and eng.info is info
        again = eng.step(x, WANT)
        print("step after run", np.abs(again["forces"] - left["forces"]).max())
        assert np.abs(again["forces"] - left["forces"]).max() < 1e-10
        assert abs(again["energy"][0] - left["energy"][0]) < 1e-10
        assert left["energy"][0] == b["epot"][-1, 0]
    split = dict(x=x, v=v, epot=np.concatenate([a["epot"], b["epot"][1:]]),
                 ekin=np.concatenate([a["ekin"], b["ekin"][1:]]), n_rebuilds=whole["n_rebuilds"])
    assert np.array_equal(a["epot"][-1], b["epot"][0]) and np.array_equal(a["ekin"][-1], b["ekin"][0])
    _assert_parity(split, whole, tol=1e-12)


def test_skin_zero_rebuilds_at_every_step(lib):
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 300.0, 3)
    ref = md_reference.run(_oracle_forces(nn, [atoms]), atoms.positions, v0, _masses([atoms]), DT, 5, skin=0.0)
    dev = _device_run(nn, [atoms], v0, 0.0, 5)
    assert dev["n_rebuilds"] == 5 and ref["n_rebuilds"] == 5
    _assert_parity(dev, ref)


@pytest.mark.parametrize("case", ["cold", "hot"])
def test_energy_conservation(lib, case):
    """NVE: the total energy of the device run wanders no more than twice what the reference loop's does."""
    _, ref = _ni_reference(case)
    dev = _ni_device(case)
    e_ref, e_dev = (ref["epot"] + ref["ekin"])[:, 0], (dev["epot"] + dev["ekin"])[:, 0]
    d_ref, d_dev = np.abs(e_ref - e_ref[0]).max(), np.abs(e_dev - e_dev[0]).max()
    print("energy drift", case, d_ref, d_dev)
    assert d_ref > 0.0 and d_dev <= 2.0 * d_ref


def test_record_every(lib):
    nn, atoms = _ni_setup()
    from tensoralloy_amd import Engine
    dev = _ni_device("cold")
    v0, _ = _ni_reference("cold")
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        eng.set_frames([atoms])
        eng.md_init(None, v0)
        out = eng.md_run(40, DT, record_every=7)
    assert out["epot"].shape == (6, 1)
    assert np.abs(out["epot"] - dev["epot"][::7]).max() < 1e-12
    assert np.abs(out["ekin"] - dev["ekin"][::7]).max() < 1e-12


def test_refusals(lib):
    from tensoralloy_amd import Engine
    nn, atoms = _ni_setup()
    n = len(atoms)
    with Engine(nn) as eng:
        with pytest.raises(ValueError, match="no resident batch"):
            eng.md_init()
        eng.set_skin(0.5)
        eng.set_frames([atoms])
        with pytest.raises(ValueError, match="before ta_md_init"):
            eng.md_run(1, DT)
        with pytest.raises(ValueError, match="before ta_md_init"):
            eng.md_state()
        bad = _masses([atoms])
        bad[5] = 0.0
        with pytest.raises(ValueError, match="mass of atom 5"):
            eng.md_init(bad)
        bad[5] = float("inf")
        with pytest.raises(ValueError, match="mass of atom 5"):
            eng.md_init(bad)
        with pytest.raises(ValueError, match="one mass"):
            eng.md_init(np.ones(n + 1))
        with pytest.raises(ValueError, match="velocities"):
            eng.md_init(None, np.zeros((n - 1, 3)))
        with pytest.raises(ValueError, match="before ta_md_init"):   # none of the failed calls left a state
            eng.md_run(1, DT)
        eng.md_init()
        with pytest.raises(ValueError, match="n_steps"):
            eng.md_run(-1, DT)
        with pytest.raises(ValueError, match="record_every"):
            eng.md_run(1, DT, record_every=0)
        out = eng.md_run(0, DT)
        assert out["epot"].shape == (1, 1) and out["ekin"].shape == (1, 1) and out["n_rebuilds"] == 0
        assert out["ekin"][0, 0] == 0.0   # no velocities given: at rest
        assert abs(out["epot"][0, 0] - oracle_eam_eval(nn, atoms)["energy"]) < TOL
        x, v = eng.md_state()
        assert np.array_equal(x, atoms.positions) and not v.any()
        eng.update_positions(atoms.positions)   # keeps the MD state
        eng.md_run(1, DT)
        eng.set_frames([atoms])                 # drops it
        with pytest.raises(ValueError, match="before ta_md_init"):
            eng.md_run(1, DT)


def test_device_md_driver(lib):
    """`DeviceMD`: runs cut at the observers' intervals, positions written back into the Atoms object."""
    from tensoralloy_amd import DeviceMD, Engine
    nn, atoms = _ni_setup()
    atoms = atoms.copy()
    v0, _ = _ni_reference("cold")
    dev = _ni_device("cold")
    seen = []
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        dyn = DeviceMD(eng, atoms, DT, velocities=v0)
        assert dyn.get_kinetic_energy() == dev["ekin"][0, 0]
        dyn.attach(lambda: seen.append((dyn.nsteps, dyn.get_kinetic_energy())), interval=15)
        dyn.run(40)
    assert [s for s, _ in seen] == [15, 30]
    assert abs(seen[1][1] - dev["ekin"][30, 0]) < 1e-12
    assert np.abs(atoms.positions - dev["x"]).max() < 1e-12 and np.abs(dyn.velocities - dev["v"]).max() < 1e-12
    assert abs(dyn.get_temperature() - 2.0 * dev["ekin"][-1, 0] / (3 * len(atoms) * md.kB)) < 1e-9
    assert abs(dyn.get_potential_energy() - dev["epot"][-1, 0]) < 1e-12
