"""GPU: time correlations inside the device MD loop (`ta_md_set_sampling`; the snapshot stores of csrc/ta_md.hip
and the correlation launch of csrc/ta_md_corr.hip) against the NumPy definition (tests/md_corr_reference.py).

Two bounds, both derived:
 (a) the correlator against `correlate` fed with the device's own snapshots: per entry
     |dev - ref| <= n_terms eps sum|terms|, the worst case of any summation order (an entry without terms: equal).
     Where the ring has wrapped, the snapshots come from a twin run with a ring that holds them all; its last
     rows must be bit-equal to the small ring's.
 (b) the device against the oracle-driven reference trajectory: snapshots within the project's TOL = 1e-9 on x
     and v (tests/test_gpu_md.py), sums within that propagated through the products: 2 max|v_ref| TOL per scalar
     product of the VACF (2 x 3 per atom) and 2 max|x_ref(n) - x_ref(n - k)| x 2 TOL per scalar square of the
     MSD, each times the number of terms.
dt = 1 fs everywhere.
"""
import functools

import numpy as np
import pytest

from tests import md_corr_reference as corr
from tests.helpers import fcc, make_eam, make_nn
from tests.test_gpu_md import DT, NI_CASES, TOL, WANT, _masses, _ni_reference, _ni_setup, _oracle_forces, _positions, _velocities
from tests.test_gpu_sf import _alloy
from tensoralloy_amd import Atoms, md

pytestmark = pytest.mark.gpu

KT0, TAU = md.kB * 600.0, 20 * DT
FRICTION, SEED = 0.01 / md.fs, 0x9E3779B97F4A7C15
EPS = np.finfo(np.float64).eps

SETUPS = {
    "nve": lambda eng: None,
    "berendsen": lambda eng: eng.md_set_thermostat(KT0, TAU),
    "langevin": lambda eng: eng.md_set_langevin(KT0, FRICTION, SEED),
    "nhc": lambda eng: eng.md_set_nose_hoover(KT0, TAU, chain=3),
}


def _freeze(out):
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
        elif isinstance(a, dict):
            _freeze(a)
    return out


def _run(nn, frames, v0, skin, runs, n_lags=None, s=1, integrator="nve", off_again=False):
    """State, records, correlations and snapshots of the runs `runs` (steps per md_run call) on the device.
    `n_lags` None: sampling is never set; `off_again`: set, then switched off before the first run."""
    from tensoralloy_amd import Engine
    with Engine(nn) as eng:
        eng.set_skin(skin)
        eng.set_frames(frames)
        eng.md_init(None, v0)
        SETUPS[integrator](eng)
        if n_lags is not None:
            eng.md_set_sampling(n_lags, s)
            if off_again:
                eng.md_set_sampling(0)
        outs = [eng.md_run(n, DT) for n in runs]
        x, v = eng.md_state()
        res = dict(x=x, v=v, n_rebuilds=sum(o["n_rebuilds"] for o in outs))
        if n_lags is not None and not off_again:
            res["corr"], res["samples"] = eng.md_correlations(), eng.md_samples()
    for k in ("epot", "ekin", "echain"):
        if k in outs[0]:
            res[k] = np.concatenate([o[k][1 if j else 0:] for j, o in enumerate(outs)])
    return _freeze(res)


def _species(nn, frames):
    els = list(nn.elements)
    return np.array([els.index(sym) for a in frames for sym in a.get_chemical_symbols()])


def _assert_a(dev, xs, vs, natoms, species, E, L):
    """Bound (a): `dev["corr"]` against the definition on the snapshots xs, vs (every sample, oldest first)."""
    ref = corr.correlate(xs, vs, natoms, species, E, L)
    c = dev["corr"]
    assert c["vacf_sum"].shape == (len(natoms), E, L) and c["n_samples"] == len(xs)
    for key, nt, ab in (("vacf_sum", "n_terms_v", "abs_v"), ("msd_sum", "n_terms_x", "abs_x")):
        bound = ref[nt] * EPS * ref[ab]
        gap = np.abs(c[key] - ref[key])
        has = bound > 0
        print(f"(a) {key}: largest gap / bound", float((gap[has] / bound[has]).max()) if has.any() else 0.0)
        assert np.all(gap <= bound), (key, float(gap.max()))
    assert np.array_equal(c["n_origins"], ref["n_origins"]) and np.array_equal(c["counts"], ref["counts"])
    for key in ("vacf", "msd"):
        assert np.array_equal(np.isnan(c[key]), np.isnan(ref[key])), key
    assert np.all(c["msd_sum"][..., 0] == 0.0)
    return ref


def _assert_b(dev, xs, vs, steps, natoms, species, E, L, tol=TOL):
    """Bound (b): the snapshots the ring holds and the sums against the reference samples xs, vs at `steps`."""
    smp, c = dev["samples"], dev["corr"]
    held = min(len(xs), L)
    assert np.array_equal(smp["steps"], np.asarray(steps)[-held:]) and c["last_step"] == steps[-1]
    gx, gv = float(np.abs(smp["x"] - xs[-held:]).max()), float(np.abs(smp["v"] - vs[-held:]).max())
    print("(b) snapshot gaps", gx, gv)
    assert gx < tol and gv < tol
    ref = corr.correlate(xs, vs, natoms, species, E, L)
    vmax = float(np.abs(vs).max())
    dmax = np.array([max([float(np.abs(xs[n] - xs[n - k]).max()) for n in range(k, len(xs))], default=0.0) for k in range(L)])
    bound_v = ref["n_terms_v"] * 2.0 * vmax * tol
    bound_x = ref["n_terms_x"] * 2.0 * dmax[None, None, :] * 2.0 * tol
    for key, bound in (("vacf_sum", bound_v), ("msd_sum", bound_x)):
        gap = np.abs(c[key] - ref[key])
        has = bound > 0
        print(f"(b) {key}: largest gap / bound", float((gap[has] / bound[has]).max()) if has.any() else 0.0)
        assert np.all(gap <= bound), (key, float(gap.max()))
    return ref


# -- the 32-atom Ni cases of tests/test_gpu_md.py ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ni_trajectory(case, integrator="nve", steps=None):
    """The oracle-driven whole-step reference trajectory (xs, vs, ekin) of an NI_CASES case."""
    nn, atoms = _ni_setup()
    T, _, n = NI_CASES[case]
    n = steps or n
    v0 = _velocities([atoms], T, 3)
    args = (_oracle_forces(nn, [atoms]), atoms.positions, v0, _masses([atoms]), DT, n)
    if integrator == "nve":
        out = corr.trajectory_verlet(*args)
    elif integrator == "berendsen":
        out = corr.trajectory_verlet(*args, kT0=KT0, tau=TAU)
    elif integrator == "langevin":
        out = corr.trajectory_langevin(*args, KT0, FRICTION, SEED)
    else:
        out = corr.trajectory_nhc(*args, KT0, TAU, chain=3)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _ni_device(case, L, s=1, steps=None, runs=None, skin=None, integrator="nve"):
    nn, atoms = _ni_setup()
    T, case_skin, n = NI_CASES[case]
    n = steps or n
    return _run(nn, [atoms], _velocities([atoms], T, 3), case_skin if skin is None else skin, list(runs or [n]), L, s,
                integrator)


def _ni_check(case, L, s=1, steps=None, runs=None, skin=None):
    """Bounds (a) and (b) of an NVE run of a 32-atom case; the snapshots of (a) are the twin's (ring of 64)."""
    n = steps or NI_CASES[case][2]
    dev = _ni_device(case, L, s, steps, runs, skin)
    # (the twin: the same run, cut into the same calls, with a ring that keeps every state)
    twin = _ni_device(case, 64, 1, steps if (skin is not None or runs) else None, runs, skin)
    idx = np.arange(0, n + 1, s)
    xs, vs = twin["samples"]["x"][idx], twin["samples"]["v"][idx]
    assert np.array_equal(twin["samples"]["steps"][idx], idx)
    held = min(len(idx), L)
    assert np.array_equal(dev["samples"]["x"], xs[-held:]) and np.array_equal(dev["samples"]["v"], vs[-held:])
    _assert_a(dev, xs, vs, [32], np.zeros(32, dtype=int), 1, L)
    rx, rv, _ = _ni_trajectory(case)
    _assert_b(dev, rx[idx], rv[idx], idx, [32], np.zeros(32, dtype=int), 1, L)
    return dev


# -- 1 -----------------------------------------------------------------------------------------------------------
def test_nve_without_rebuild(lib):
    dev = _ni_check("cold", 8)
    c = dev["corr"]
    assert dev["n_rebuilds"] == 0
    assert (c["n_samples"], c["sample_every"], c["last_step"]) == (41, 1, 40)
    assert np.array_equal(c["n_origins"], 41 - np.arange(8)) and np.array_equal(c["counts"], [[32]])
    assert np.all(c["msd"][..., 0] == 0.0) and np.all(c["msd"][..., 1:] > 0.0)
    # one element, equal masses: m / 2 x the lag-0 sum is the kinetic energy summed over the sampled steps
    m = _masses([_ni_setup()[1]])
    assert np.all(m == m[0])
    assert abs(0.5 * m[0] * c["vacf_sum"][0, 0, 0] - dev["ekin"][:, 0].sum()) <= 1e-12 * dev["ekin"][:, 0].sum()


def test_twin_ring_not_yet_full(lib):
    """The ring of 64 that serves the other tests as the record of every snapshot: 41 samples, lags 41 .. 63 empty."""
    dev = _ni_device("cold", 64)
    smp = dev["samples"]
    _assert_a(dev, smp["x"], smp["v"], [32], np.zeros(32, dtype=int), 1, 64)
    assert np.all(dev["corr"]["vacf_sum"][..., 41:] == 0.0) and np.all(np.isnan(dev["corr"]["vacf"][..., 41:]))


# -- 2 -----------------------------------------------------------------------------------------------------------
def test_nve_with_rebuilds_mid_run(lib):
    """A dozen rebuilds inside look-ahead windows: a sample added twice, or skipped behind a stale list, shows."""
    dev = _ni_check("hot", 8)
    _, ref = _ni_reference("hot")
    assert dev["n_rebuilds"] == ref["n_rebuilds"] >= 10
    assert dev["corr"]["n_samples"] == 61


def test_nve_skin_zero_rebuilds_at_every_step(lib):
    dev = _ni_check("cold", 8, steps=5, skin=0.0)
    assert dev["n_rebuilds"] == 5 and dev["corr"]["n_samples"] == 6   # (the reference's rule: every drift is stale)


# -- 3 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L, s, steps, n_samples", [(1, 1, 40, 41), (5, 1, 22, 23), (16, 1, 5, 6), (8, 3, 40, 14)],
                         ids=["L1", "L5_wrapped", "L16_not_full", "every3"])
def test_ring_edges(lib, L, s, steps, n_samples):
    dev = _ni_check("cold", L, s, steps=None if steps == 40 else steps)
    c = dev["corr"]
    assert c["n_samples"] == n_samples and c["sample_every"] == s and c["last_step"] == (steps // s) * s
    assert len(dev["samples"]["steps"]) == min(L, n_samples)
    if n_samples < L:
        assert np.all(c["vacf_sum"][..., n_samples:] == 0.0) and np.all(c["msd_sum"][..., n_samples:] == 0.0)
        assert np.all(np.isnan(c["vacf"][..., n_samples:])) and np.all(np.isnan(c["msd"][..., n_samples:]))
        assert not np.any(np.isnan(c["vacf"][..., :n_samples]))


# -- 4 -----------------------------------------------------------------------------------------------------------
def test_split_runs(lib):
    """7 + 13 + 20 steps against 40 in one call, every third step sampled. Steps 7 and 20 are no samples, and the
    state two runs share is sampled once. The project's split-run bound is 1e-12 on x and v."""
    whole = _ni_device("cold", 8, 3)
    split = _ni_check("cold", 8, 3, runs=(7, 13, 20))
    assert split["corr"]["n_samples"] == whole["corr"]["n_samples"] == 14
    twin = _ni_device("cold", 64)
    idx = np.arange(0, 41, 3)
    _assert_b(split, twin["samples"]["x"][idx], twin["samples"]["v"][idx], idx, [32], np.zeros(32, dtype=int), 1, 8, tol=1e-12)
    # runs that end on a sampled step: 6 + 6 + 9 of 21, and a run of no step at all
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 300.0, 3)
    cut = _run(nn, [atoms], v0, 0.5, [6, 0, 6, 9], 8, 3)
    one = _run(nn, [atoms], v0, 0.5, [21], 8, 3)
    assert cut["corr"]["n_samples"] == one["corr"]["n_samples"] == 8
    idx = np.arange(0, 22, 3)
    _assert_b(cut, twin["samples"]["x"][idx], twin["samples"]["v"][idx], idx, [32], np.zeros(32, dtype=int), 1, 8, tol=1e-12)
    _assert_b(one, twin["samples"]["x"][idx], twin["samples"]["v"][idx], idx, [32], np.zeros(32, dtype=int), 1, 8, tol=1e-12)


# -- 5 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator", ["berendsen", "langevin", "nhc"])
def test_every_integrator_build(lib, integrator):
    """20 steps, a ring of 32 that holds all 21 samples, against the reference trajectory of the integrator."""
    dev = _ni_device("cold", 32, 1, 20, None, None, integrator)
    smp = dev["samples"]
    assert np.array_equal(smp["steps"], np.arange(21))
    sp = np.zeros(32, dtype=int)
    _assert_a(dev, smp["x"], smp["v"], [32], sp, 1, 32)
    rx, rv, ekin = _ni_trajectory("cold", integrator, 20)
    _assert_b(dev, rx, rv, np.arange(21), [32], sp, 1, 32)
    assert np.abs(dev["ekin"] - ekin).max() < TOL
    # the sampled velocities are those of the record: for the chain they carry s1
    m = _masses([_ni_setup()[1]])
    ke = 0.5 * (m[None, :, None] * smp["v"] ** 2).sum(axis=(1, 2))
    assert np.abs(ke - dev["ekin"][:, 0]).max() < 1e-12 * ke.max()
    nve = _ni_trajectory("cold")[1][:21]
    assert np.abs(rv - nve).max() > 1e-5   # (the thermostat is not a bystander)


@pytest.mark.parametrize("integrator", ["nhc", "nve"])
def test_frame_above_1024_atoms(lib, integrator):
    """1372 atoms: six chunks of the correlation launch, the last one partly filled; under the chain one integrator
    workgroup whose threads stride over the atoms, without it two. Bound (a), 6 steps, a ring of 4 (wrapped)."""
    nn = make_eam(["Ni"], 6.0, potential="zjw04")
    frames = [fcc(rep=(7, 7, 7), jitter=0.02, seed=3)]
    assert len(frames[0]) == 1372
    v0 = _velocities(frames, 300.0, 5)
    dev = _run(nn, frames, v0, 0.3, [6], 4, 1, integrator)
    twin = _run(nn, frames, v0, 0.3, [6], 8, 1, integrator)
    xs, vs = twin["samples"]["x"], twin["samples"]["v"]
    assert len(xs) == 7 and np.array_equal(dev["samples"]["x"], xs[-4:]) and np.array_equal(dev["samples"]["v"], vs[-4:])
    sp = np.zeros(1372, dtype=int)
    _assert_a(dev, xs, vs, [1372], sp, 1, 4)
    _assert_a(twin, xs, vs, [1372], sp, 1, 8)


# -- 6 -----------------------------------------------------------------------------------------------------------
def test_batch_of_unlike_frames_and_elements(lib):
    """Three frames of a two-element SF model: 32 Ni (no Mo at all), one lone Ni atom, a 48-atom Ni-Mo cell. A
    ring of 12 (one and a half lag tiles) that 11 samples do not fill."""
    from tensoralloy_amd import Engine
    nn = make_nn(["Mo", "Ni"], 6.0, True, [8])
    lone = Atoms(symbols=["Ni"], positions=[[10.0, 10.0, 10.0]], cell=np.diag([20.0, 20.0, 20.0]), pbc=True)
    frames = [fcc(rep=(2, 2, 2), jitter=0.02, seed=3), lone, _alloy(["Ni", "Mo"], rep=(2, 2, 3))]
    natoms = [len(a) for a in frames]
    assert natoms == [32, 1, 48]
    sp = _species(nn, frames)
    ni, mo = list(nn.elements).index("Ni"), list(nn.elements).index("Mo")
    v0 = np.array(_velocities(frames, 300.0, 11))
    v0[32] = [0.01, -0.02, 0.03]
    dev = _run(nn, frames, v0, 0.3, [10], 12)
    smp, c = dev["samples"], dev["corr"]
    _assert_a(dev, smp["x"], smp["v"], natoms, sp, 2, 12)
    with Engine(nn) as other:
        other.set_skin(0.0)
        other.set_frames(frames)

        def force(x):
            r = other.step(x, WANT)
            return r["energy"].copy(), r["forces"].copy()
        rx, rv, _ = corr.trajectory_verlet(force, _positions(frames), v0, _masses(frames), DT, 10, natoms=natoms)
    _assert_b(dev, rx, rv, np.arange(11), natoms, sp, 2, 12)
    want = np.zeros((3, 2), dtype=np.int64)
    want[0, ni], want[1, ni], want[2, ni], want[2, mo] = 32, 1, 24, 24
    assert np.array_equal(c["counts"], want)
    for f in (0, 1):   # no Mo: zero sums, NaN normalised
        assert np.all(c["vacf_sum"][f, mo] == 0.0) and np.all(c["msd_sum"][f, mo] == 0.0)
        assert np.all(np.isnan(c["vacf"][f, mo])) and np.all(np.isnan(c["msd"][f, mo]))
    assert not np.any(np.isnan(c["vacf"][2, :, :11])) and np.all(np.isnan(c["vacf"][..., 11]))
    # the lone atom flies free: v . v at every lag, |k dt v|^2
    v2 = float((v0[32] ** 2).sum())
    k = np.arange(11)
    assert np.abs(c["vacf"][1, ni, :11] - v2).max() < 1e-15
    # (ten drifts near x = 10, each rounded to an ulp of 10 at most, in a displacement of |v| 10 dt at most)
    assert np.abs(c["msd"][1, ni, :11] - (k * DT) ** 2 * v2).max() < 2.0 * 10 * DT * np.sqrt(v2) * 10 * np.spacing(10.0)


# -- 7 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator", ["nve", "langevin", "nhc"])
def test_sampling_is_a_pure_observer(lib, integrator):
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 2000.0, 3)
    plain = _run(nn, [atoms], v0, 0.1, [9, 11], None, 1, integrator)
    keys = ("x", "v", "epot", "ekin") + (("echain",) if integrator == "nhc" else ())
    for label, other in (("on", _run(nn, [atoms], v0, 0.1, [9, 11], 6, 2, integrator)),
                         ("off again", _run(nn, [atoms], v0, 0.1, [9, 11], 6, 2, integrator, off_again=True))):
        assert other["n_rebuilds"] == plain["n_rebuilds"] >= 1, label
        for k in keys:
            assert np.array_equal(other[k], plain[k]), (label, k)


# -- 8 -----------------------------------------------------------------------------------------------------------
def test_life_cycle_and_refusals(lib):
    from tensoralloy_amd import Engine
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 300.0, 3)
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        with pytest.raises(ValueError, match="no resident batch"):
            eng.md_correlations()
        eng.md_set_sampling(0)   # off is always allowed
        eng.set_frames([atoms])
        for call in (eng.md_correlations, eng.md_samples):
            with pytest.raises(ValueError, match="called before ta_md_init"):
                call()
        with pytest.raises(ValueError, match="ta_md_set_sampling called before ta_md_init"):
            eng.md_set_sampling(8)
        eng.md_init(None, v0)
        with pytest.raises(ValueError, match=r"ta_md_get_correlations: sampling is off \(ta_md_set_sampling\)"):
            eng.md_correlations()
        with pytest.raises(ValueError, match=r"ta_md_get_samples: sampling is off \(ta_md_set_sampling\)"):
            eng.md_samples()
        eng.md_set_sampling(8, 2)
        for what, args in (("n_lags", (-1, 1)), ("n_lags", (4097, 1)), ("sample_every", (8, 0)), ("sample_every", (8, -2))):
            with pytest.raises(ValueError, match="ta_md_set_sampling: " + what):
                eng.md_set_sampling(*args)
        c = eng.md_correlations()   # ... and a refused call left the setting as it was
        assert c["vacf"].shape == (1, 1, 8) and (c["n_samples"], c["sample_every"], c["last_step"]) == (0, 2, -1)
        assert np.all(np.isnan(c["vacf"])) and np.all(c["vacf_sum"] == 0.0)
        assert eng.md_samples()["x"].shape == (0, 32, 3)
        out = eng.md_run(10, DT)
        assert set(out) == {"epot", "ekin", "n_rebuilds"}   # the result dict is unchanged
        assert eng.md_correlations()["n_samples"] == 6 and len(eng.md_samples()["steps"]) == 6
        assert np.array_equal(eng.md_samples(2)["steps"], [8, 10])
        with pytest.raises(ValueError, match="ta_md_get_samples: first_lag \\+ n = 7 exceeds the 6 snapshots held"):
            eng.md_samples(7)
        # the barostat and sampling together: refused by the run, both named, nothing lost
        x0, v_before = eng.md_state()
        before = eng.md_correlations()
        eng.md_set_barostat(0.0, 100 * DT, 1.0)
        with pytest.raises(ValueError, match=r"ta_md_run: sampling \(ta_md_set_sampling\) and the barostat \(ta_md_set_barostat\)"):
            eng.md_run(5, DT)
        eng.md_set_barostat(0.0, 0.0, 0.0)
        x1, v1 = eng.md_state()
        after = eng.md_correlations()
        assert np.array_equal(x0, x1) and np.array_equal(v_before, v1)
        assert np.array_equal(before["vacf_sum"], after["vacf_sum"]) and after["n_samples"] == 6
        # setting it again zeroes; sample 0 is then the first multiple of sample_every not behind the step
        eng.md_run(1, DT)   # step 11
        eng.md_set_sampling(4, 3)
        c = eng.md_correlations()
        assert c["vacf"].shape == (1, 1, 4) and c["n_samples"] == 0 and np.all(c["vacf_sum"] == 0.0)
        eng.md_run(5, DT)   # steps 12 .. 16: samples at 12 and 15
        assert np.array_equal(eng.md_samples()["steps"], [12, 15])
        # set_frames keeps the setting and drops the data with the MD state; md_init starts afresh
        eng.set_frames([atoms])
        with pytest.raises(ValueError, match="ta_md_get_correlations called before ta_md_init"):
            eng.md_correlations()
        eng.md_init(None, v0)
        c = eng.md_correlations()
        assert c["vacf"].shape == (1, 1, 4) and (c["n_samples"], c["sample_every"], c["last_step"]) == (0, 3, -1)
        assert np.all(c["vacf_sum"] == 0.0) and np.all(c["msd_sum"] == 0.0)
        eng.md_run(3, DT)
        assert np.array_equal(eng.md_samples()["steps"], [0, 3])
        eng.md_set_sampling(0)
        with pytest.raises(ValueError, match="sampling is off"):
            eng.md_samples()


def test_device_md_end_to_end(lib):
    from tensoralloy_amd import Engine
    nn, atoms = _ni_setup()
    atoms = atoms.copy()
    v0 = _velocities([atoms], 300.0, 3)
    with Engine(nn) as eng:
        dyn = md.DeviceMD(eng, atoms, DT, velocities=v0, n_lags=8, sample_every=2)
        dyn.run(7)
        dyn.run(5)
        c = eng.md_correlations()
        assert (c["n_samples"], c["last_step"]) == (7, 12)
        t, vacf = dyn.get_vacf()
        t2, msd = dyn.get_msd()
        assert np.array_equal(t, np.arange(8) * 2 * DT) and np.array_equal(t, t2)
        assert vacf.shape == msd.shape == (1, 8)
        assert np.array_equal(vacf, c["vacf"][0], equal_nan=True) and np.array_equal(msd, c["msd"][0], equal_nan=True)
        smp = dyn.get_samples()
        assert np.array_equal(smp["steps"], np.arange(0, 13, 2)) and np.array_equal(smp["x"][0], _ni_setup()[1].positions)
        assert np.array_equal(smp["v"][0], v0) and np.array_equal(smp["x"][-1], atoms.positions)
        assert np.array_equal(dyn.get_samples(3)["x"], smp["x"][-3:])
        twin = _ni_device("cold", 64)["samples"]   # (another skin, another cut: the project's parity bound)
        assert np.abs(smp["x"] - twin["x"][0:13:2]).max() < TOL and np.abs(smp["v"] - twin["v"][0:13:2]).max() < TOL
        plain = md.DeviceMD(eng, atoms, DT, velocities=v0)   # n_lags None: sampling is set off
        for call in (plain.get_vacf, plain.get_msd, plain.get_samples):
            with pytest.raises(ValueError, match=r"sampling is off \(n_lags\)"):
                call()
        with pytest.raises(ValueError, match="sampling is off"):
            eng.md_correlations()
