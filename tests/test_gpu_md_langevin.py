"""GPU: the Langevin thermostat of the device-resident MD loop (`ta_md_set_langevin`, `ta_md_noise`,
csrc/ta_md.hip) against the NumPy reference (tests/md_langevin_reference.py) driven by the CPU oracle or by a
second engine's `Engine.step`.

Every case: dt = 1 fs, at most 1200 steps and 1372 atoms. Noise bound 1e-13: the normals are bounded by
sqrt(2 * 53 * ln 2) = 8.6, whose ulp is 1.8e-15, and are a handful of library calls of <= 2 ulp each.
Trajectory bound 1e-9 (A, A per time unit, eV), the bound and the argument of tests/test_gpu_md.py: the
noise adds its 1e-13 times c3 <= 1e-3 per step to the 1e-13 per step of the forces.
"""
import functools

import numpy as np
import pytest

from tests import md_langevin_reference as lv
from tests import md_reference
from tests.helpers import fcc, make_eam, make_grap_nn, make_nn, oracle_eam_eval
from tests.test_gpu_md import _assert_parity, _masses, _ni_setup, _oracle_forces, _positions, _velocities
from tests.test_gpu_sf import _alloy
from tensoralloy_amd import Atoms, _lib, md

pytestmark = pytest.mark.gpu

DT = md.fs
TOL = 1e-9
NOISE_TOL = 1e-13
WANT = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES
FRICTION = 0.01 / md.fs
SEED = 0x9E3779B97F4A7C15   # (a seed with a high word: both key words are in use)


def _device_run(nn, frames, v0, skin, steps, langevin, splits=None):
    """x, v, epot, ekin, n_rebuilds of `steps` Langevin steps on the device; `langevin` = (kT, friction, seed)."""
    from tensoralloy_amd import Engine
    with Engine(nn) as eng:
        eng.set_skin(skin)
        eng.set_frames(frames)
        eng.md_init(None, v0)
        eng.md_set_langevin(*langevin)
        epot, ekin, rebuilds = [], [], 0
        for k, n in enumerate(splits or [steps]):
            out = eng.md_run(n, DT)
            epot.append(out["epot"][1 if k else 0:])
            ekin.append(out["ekin"][1 if k else 0:])
            rebuilds += out["n_rebuilds"]
        x, v = eng.md_state()
    return dict(x=x, v=v, epot=np.concatenate(epot), ekin=np.concatenate(ekin), n_rebuilds=rebuilds)


def _freeze(ref):
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref


# -- the Ni zjw04 cases: (start temperature, bath temperature, friction, skin, steps) ------------------------
NI_CASES = {"cold": (300.0, 600.0, FRICTION, 0.5, 40), "hot": (2000.0, 2000.0, FRICTION, 0.1, 60),
            "hot30": (2000.0, 2000.0, FRICTION, 0.1, 30), "damped": (300.0, 0.0, 0.05 / md.fs, 0.5, 40)}


@functools.lru_cache(maxsize=None)
def _ni_reference(case):
    nn, atoms = _ni_setup()
    T, T_bath, fr, skin, steps = NI_CASES[case]
    v0 = _velocities([atoms], T, 3)
    ref = lv.run(_oracle_forces(nn, [atoms]), atoms.positions, v0, _masses([atoms]), DT, steps,
                 kT0=md.kB * T_bath, friction=fr, seed=SEED, skin=skin)
    v0.setflags(write=False)
    return v0, _freeze(ref)


@functools.lru_cache(maxsize=None)
def _ni_device(case):
    nn, atoms = _ni_setup()
    T, T_bath, fr, skin, steps = NI_CASES[case]
    v0, _ = _ni_reference(case)
    return _device_run(nn, [atoms], v0, skin, steps, (md.kB * T_bath, fr, SEED))


def test_noise_parity(lib):
    from tensoralloy_amd import Engine
    nn = make_eam(["Ni"], 6.0, potential="zjw04")
    lone = Atoms(symbols=["Ni"], positions=[[10.0, 10.0, 10.0]], cell=np.diag([20.0, 20.0, 20.0]), pbc=True)
    frames = [fcc(rep=(2, 2, 2), jitter=0.02, seed=3), fcc(rep=(3, 3, 3), jitter=0.02, seed=4), lone]
    n = sum(len(a) for a in frames)
    assert [len(a) for a in frames] == [32, 108, 1]
    worst = 0.0
    with Engine(nn) as eng:
        eng.set_frames(frames)
        eng.md_init()
        eng.md_set_langevin(md.kB * 600.0, FRICTION, SEED)
        seen = {}
        for step in (0, 1, 7, 2 ** 32 + 5):
            xi, eta = eng.md_noise(step)
            r_xi, r_eta = lv.normals(SEED, step, n)
            assert xi.shape == eta.shape == (n, 3)
            gap = max(np.abs(xi - r_xi).max(), np.abs(eta - r_eta).max())
            print("noise gap at step", step, gap)
            worst = max(worst, gap)
            again = eng.md_noise(step)
            assert np.array_equal(again[0], xi) and np.array_equal(again[1], eta)
            seen[step] = xi
        print("noise gap, largest", worst)
        assert worst <= NOISE_TOL
        assert not np.array_equal(seen[5 + 2 ** 32], eng.md_noise(5)[0])   # the high word of the step counts
        eng.md_set_langevin(md.kB * 600.0, FRICTION, SEED + 1)
        assert not np.array_equal(eng.md_noise(7)[0], seen[7])
        eng.md_set_langevin(md.kB * 600.0, FRICTION, SEED & 0xFFFFFFFF)      # ... and that of the seed
        assert not np.array_equal(eng.md_noise(7)[0], seen[7])
        eng.md_set_langevin(md.kB * 300.0, 2.0 * FRICTION, SEED)             # the bath is not in the noise
        assert np.array_equal(eng.md_noise(7)[0], seen[7])


def test_parity_with_the_oracle_without_rebuild(lib):
    _, ref = _ni_reference("cold")
    dev = _ni_device("cold")
    assert ref["n_rebuilds"] == 0 and dev["n_rebuilds"] == 0
    assert dev["epot"].shape == (41, 1)
    _assert_parity(dev, ref)
    # the thermostat did something: velocity Verlet from the same start ends elsewhere
    nn, atoms = _ni_setup()
    v0, _ = _ni_reference("cold")
    nve = md_reference.run(_oracle_forces(nn, [atoms]), atoms.positions, v0, _masses([atoms]), DT, 40)
    assert np.abs(nve["v"] - ref["v"]).max() > 1e-4


def test_parity_with_rebuilds_mid_run(lib):
    """Steps behind a stale list are enqueued, skipped and redone: they draw the noise of their index again."""
    _, ref = _ni_reference("hot")
    dev = _ni_device("hot")
    print("rebuild steps", ref["rebuild_steps"])
    assert dev["n_rebuilds"] == ref["n_rebuilds"] and 2 <= ref["n_rebuilds"] < 60
    _assert_parity(dev, ref)


def test_split_runs(lib):
    """30 steps = 10 + 20 steps: the step counter goes on from one `md_run` to the next."""
    nn, atoms = _ni_setup()
    v0, ref = _ni_reference("hot30")
    whole = _ni_device("hot30")
    T, T_bath, fr, skin, steps = NI_CASES["hot30"]
    split = _device_run(nn, [atoms], v0, skin, steps, (md.kB * T_bath, fr, SEED), splits=[10, 20])
    assert split["n_rebuilds"] == whole["n_rebuilds"] >= 2
    _assert_parity(split, whole, tol=1e-12)
    _assert_parity(whole, ref)


def test_skin_zero_rebuilds_at_every_step(lib):
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 300.0, 3)
    ref = lv.run(_oracle_forces(nn, [atoms]), atoms.positions, v0, _masses([atoms]), DT, 5,
                 kT0=md.kB * 600.0, friction=FRICTION, seed=SEED, skin=0.0)
    dev = _device_run(nn, [atoms], v0, 0.0, 5, (md.kB * 600.0, FRICTION, SEED))
    assert dev["n_rebuilds"] == 5 and ref["n_rebuilds"] == 5
    _assert_parity(dev, ref)


def test_frame_of_several_workgroups(lib):
    """1372 atoms are two workgroups of the chunked layout. Reference forces: a second engine with skin 0
    through `Engine.step` (an exact list at every step)."""
    from tensoralloy_amd import Engine
    nn = make_eam(["Ni"], 6.0, potential="zjw04")
    frames = [fcc(rep=(7, 7, 7), jitter=0.02, seed=3)]
    assert len(frames[0]) == 1372
    v0 = _velocities(frames, 600.0, 5)
    with Engine(nn) as other:
        other.set_skin(0.0)
        other.set_frames(frames)

        def force(x):
            r = other.step(x, WANT)
            return r["energy"].copy(), r["forces"].copy()
        ref = lv.run(force, _positions(frames), v0, _masses(frames), DT, 10, kT0=md.kB * 600.0, friction=FRICTION,
                     seed=SEED, skin=0.3)
    dev = _device_run(nn, frames, v0, 0.3, 10, (md.kB * 600.0, FRICTION, SEED))
    assert dev["n_rebuilds"] == ref["n_rebuilds"]
    _assert_parity(dev, ref)


def test_batch_of_unlike_frames(lib):
    """Four frames at once; the atom index of the noise runs over the whole batch. The lone atom feels no
    force: it is an exact Ornstein-Uhlenbeck process driven by the noise of atom 188."""
    nn = make_eam(["Mo", "Ni"], 6.0, potential="zjw04")
    lone = Atoms(symbols=["Ni"], positions=[[10.0, 10.0, 10.0]], cell=np.diag([20.0, 20.0, 20.0]), pbc=True)
    frames = [fcc(rep=(2, 2, 2), jitter=0.02, seed=3), _alloy(["Ni", "Mo"], rep=(2, 2, 3)),
              fcc(rep=(3, 3, 3), jitter=0.02, seed=4), lone]
    natoms = [len(a) for a in frames]
    assert natoms == [32, 48, 108, 1]
    v0 = _velocities(frames, 600.0, 11)
    v0[-1] = [0.01, -0.02, 0.03]
    langevin = (md.kB * 600.0, FRICTION, SEED)
    dev = _device_run(nn, frames, v0, 0.3, 20, langevin)
    ref = lv.run(_oracle_forces(nn, frames), _positions(frames), v0, _masses(frames), DT, 20, kT0=langevin[0],
                 friction=FRICTION, seed=SEED, natoms=natoms)
    _assert_parity(dev, ref)
    assert np.all(dev["epot"][:, 3] == dev["epot"][0, 3])
    # ... which a reference batch of 189 free particles reproduces for its last atom, and one of 1 does not
    free = lambda x: (np.zeros(1), np.zeros_like(x))
    ou = lv.run(free, _positions(frames), v0, _masses(frames), DT, 20, kT0=langevin[0], friction=FRICTION, seed=SEED)
    assert np.abs(ou["x"][-1] - dev["x"][-1]).max() < 1e-12 and np.abs(ou["v"][-1] - dev["v"][-1]).max() < 1e-12
    alone = lv.run(free, lone.positions, v0[-1:], _masses([lone]), DT, 20, kT0=langevin[0], friction=FRICTION,
                   seed=SEED)
    assert np.abs(alone["x"] - dev["x"][-1:]).max() > 1e-6


@pytest.mark.parametrize("family", ["sf", "grap"])
def test_model_families(lib, family):
    from tensoralloy_amd import Engine
    if family == "sf":
        nn, frames = make_nn(["Ni"], 6.0, True, [8]), [fcc(rep=(2, 2, 2), jitter=0.02, seed=3)]
    else:
        nn, frames = make_grap_nn(["Ni"], 6.0, [16]), [fcc(rep=(2, 2, 2), jitter=0.02, seed=3)]
    v0 = _velocities(frames, 600.0, 5)
    with Engine(nn) as other:
        other.set_skin(0.0)
        other.set_frames(frames)

        def force(x):
            r = other.step(x, WANT)
            return r["energy"].copy(), r["forces"].copy()
        ref = lv.run(force, _positions(frames), v0, _masses(frames), DT, 20, kT0=md.kB * 600.0, friction=FRICTION,
                     seed=SEED, skin=0.3)
    dev = _device_run(nn, frames, v0, 0.3, 20, (md.kB * 600.0, FRICTION, SEED))
    assert dev["n_rebuilds"] == ref["n_rebuilds"]
    _assert_parity(dev, ref)


def test_thermalisation(lib):
    """512 Ni atoms 12 A apart (rc = 6: no pair ever forms) from rest in a bath of 900 K, friction 0.1 / fs,
    1200 steps: free particles, so the dynamics is linear and rounding does not grow. The device's mean
    temperature over steps 200 .. 1200 is within 2 % of the bath's, the bound of the CPU test of the
    reference loop (standard error 0.36 %, bias of the scheme O((fr dt)^2) = 1 %)."""
    nn = make_eam(["Ni"], 6.0, potential="zjw04")
    g = np.arange(8) * 12.0 + 6.0
    pts = np.array([[x, y, z] for x in g for y in g for z in g])
    atoms = Atoms(symbols=["Ni"] * 512, positions=pts, cell=np.diag([96.0, 96.0, 96.0]), pbc=True)
    v0 = np.zeros((512, 3))
    kT0, fr = md.kB * 900.0, 0.1 / md.fs
    dev = _device_run(nn, [atoms], v0, 0.5, 1200, (kT0, fr, SEED))
    assert dev["epot"].shape == (1201, 1)
    assert np.all(dev["epot"] == dev["epot"][0])          # A: no pair in any record
    e0 = oracle_eam_eval(nn, atoms)
    assert not np.any(e0["forces"])
    free = lambda x: (np.array([e0["energy"]]), np.zeros_like(x))
    ref = lv.run(free, pts, v0, _masses([atoms]), DT, 1200, kT0=kT0, friction=fr, seed=SEED, skin=0.5)
    assert dev["n_rebuilds"] >= 2 and dev["n_rebuilds"] == ref["n_rebuilds"]   # B
    _assert_parity(dev, ref)                              # C
    T = 2.0 * dev["ekin"][:, 0] / (3 * 512 * md.kB)
    T_ref = 2.0 * ref["ekin"][:, 0] / (3 * 512 * md.kB)
    print("mean temperature: device", T[200:].mean(), "reference", T_ref[200:].mean())
    assert T[0] == 0.0
    assert abs(T[200:].mean() / 900.0 - 1.0) < 0.02       # D
    assert abs(T_ref[200:].mean() / 900.0 - 1.0) < 0.02


def test_damping(lib):
    """kT0 = 0 with a friction: no noise, the run loses energy."""
    _, ref = _ni_reference("damped")
    dev = _ni_device("damped")
    _assert_parity(dev, ref)
    e = (dev["epot"] + dev["ekin"])[:, 0]
    print("total energy", e[0], "->", e[-1])
    assert e[-1] < e[0]


@pytest.mark.parametrize("berendsen", [False, True])
def test_existing_path_untouched(lib, berendsen):
    """Langevin switched on, used, and switched off again: the velocity-Verlet / Berendsen run that follows is
    the run of an engine that never heard of it, bit for bit."""
    from tensoralloy_amd import Engine
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 300.0, 3)
    thermostat = (md.kB * 600.0, 20 * DT)

    def run(eng):
        eng.set_frames([atoms])
        eng.md_init(None, v0)
        if berendsen:
            eng.md_set_thermostat(*thermostat)
        out = eng.md_run(40, DT)
        x, v = eng.md_state()
        return dict(x=x, v=v, epot=out["epot"], ekin=out["ekin"])

    with Engine(nn) as eng:
        eng.set_skin(0.5)
        fresh = run(eng)
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        eng.set_frames([atoms])
        eng.md_init(None, v0)
        eng.md_set_langevin(md.kB * 600.0, FRICTION, SEED)
        eng.md_run(3, DT)
        eng.md_set_langevin(friction=0.0)
        after = run(eng)
    for k in ("x", "v", "epot", "ekin"):
        assert np.array_equal(fresh[k], after[k]), k
    assert np.abs(fresh["x"] - atoms.positions).max() > 1e-3


def test_device_md_driver(lib):
    """`DeviceMD` with `friction`: the run cut at the observers' intervals (and the zero-step run of the
    constructor) is the uncut run of the same seed."""
    from tensoralloy_amd import DeviceMD, Engine
    nn, atoms = _ni_setup()
    atoms = atoms.copy()
    v0, _ = _ni_reference("cold")
    dev = _ni_device("cold")
    seen = []
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        dyn = DeviceMD(eng, atoms, DT, temperature_K=600.0, friction=FRICTION, seed=SEED, velocities=v0)
        dyn.attach(lambda: seen.append(dyn.nsteps), interval=15)
        dyn.run(40)
        assert seen == [15, 30]
        assert np.abs(atoms.positions - dev["x"]).max() < 1e-12 and np.abs(dyn.velocities - dev["v"]).max() < 1e-12
        assert abs(dyn.get_kinetic_energy() - dev["ekin"][-1, 0]) < 1e-12
        # a Berendsen driver on the same engine switches Langevin off first
        DeviceMD(eng, atoms, DT, temperature_K=600.0, taut=20 * DT, velocities=v0).run(2)
        with pytest.raises(ValueError, match="Berendsen"):
            eng.md_set_langevin(md.kB * 600.0, FRICTION, SEED)


def test_refusals(lib):
    from tensoralloy_amd import Engine
    nn, atoms = _ni_setup()
    kT = md.kB * 600.0
    with Engine(nn) as eng:
        with pytest.raises(ValueError, match="no resident batch"):
            eng.md_noise(0)
        eng.set_skin(0.5)
        eng.set_frames([atoms])
        with pytest.raises(ValueError, match="before ta_md_init"):
            eng.md_noise(0)
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="friction"):
                eng.md_set_langevin(kT, bad, 1)
            with pytest.raises(ValueError, match="kT0"):
                eng.md_set_langevin(bad, FRICTION, 1)
        with pytest.raises(ValueError, match="seed"):
            eng.md_set_langevin(kT, FRICTION, -1)
        eng.md_init()
        with pytest.raises(ValueError, match="step"):
            eng.md_noise(-1)
        eng.md_set_thermostat(kT, 20 * DT)
        with pytest.raises(ValueError, match="Berendsen.*Langevin|Langevin.*Berendsen"):
            eng.md_set_langevin(kT, FRICTION, 1)
        eng.md_set_langevin(kT, 0.0, 1)          # off stays allowed
        eng.md_set_thermostat(0.0, 0.0)
        eng.md_set_langevin(kT, FRICTION, 1)
        with pytest.raises(ValueError, match="Berendsen.*Langevin|Langevin.*Berendsen"):
            eng.md_set_thermostat(kT, 20 * DT)
        eng.md_set_thermostat(0.0, 0.0)          # off stays allowed
        with pytest.raises(ValueError, match="dt"):
            eng.md_run(1, -DT)
        eng.set_frames([atoms])                   # keeps the setting, drops the MD state
        with pytest.raises(ValueError, match="before ta_md_init"):
            eng.md_noise(0)
        eng.md_init()
        a = eng.md_run(2, DT)
        assert a["ekin"][0, 0] == 0.0 and a["ekin"][-1, 0] > 0.0   # Langevin is still on: the bath heats
