"""GPU: partial pair distributions inside the device MD loop (`ta_md_set_rdf`, csrc/ta_md_rdf.hip) against the
NumPy definition (tests/md_rdf_reference.py), which sweeps all periodic images by brute force and shares nothing
with the library's neighbour list.

The counts are integers, so the comparison is EXACT. That needs no pair on a bin edge: every exact-count test
first asserts, on the reference alone, that no r / dr of its snapshots lies within 1e-9 of an integer. The device
and the reference form r from the same doubles in another order, a few ulps (1e-15 relative) apart, so 1e-9 bins
is six orders of magnitude of room; with 1e4 .. 1e5 pair distances per case the nearest edge is typically 1e-5
bins away. The snapshots are the device's own whole-step states: `md_state()` between the calls of a cut run, or
the position ring of `md_set_sampling`. Positions are thermalised (a jittered lattice moved by the dynamics),
dt = 1 fs, at most 140 atoms and 30 steps (one case of 20000 atoms samples its entry state only).

The run that fails (for the getter behind it) fails on the host: its record buffers, 2^31 records of 128 frames,
are 2.5 TB that no device has, and `ta_md_run` allocates them before it enqueues anything.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import md_rdf_reference as ref
from tests.helpers import fcc, make_eam, make_nn
from tests.test_gpu_md import DT, WANT, _ni_setup, _velocities
from tests.test_gpu_sf import _alloy
from tensoralloy_amd import Atoms, md

pytestmark = pytest.mark.gpu

KT0, TAU = md.kB * 600.0, 20 * DT
FRICTION, SEED = 0.01 / md.fs, 0x9E3779B97F4A7C15
EDGE = 1e-9   # bins: no pair of the reference may be nearer to a bin edge

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


def _run(nn, frames, v0, skin, runs, bins=None, r_max=None, every=1, integrator="nve", lags=None):
    """The runs `runs` (steps per md_run call) on the device: final state, records, the whole-step positions at
    entry and behind every call (`states`, at the absolute steps `steps`), and with `bins` the counts (`rdf`).
    `lags`: `md_set_sampling(lags, 1)` is on as well and its ring is returned (`samples`)."""
    from tensoralloy_amd import Engine
    with Engine(nn) as eng:
        eng.set_skin(skin)
        eng.set_frames(frames)
        eng.md_init(None, v0)
        SETUPS[integrator](eng)
        if lags is not None:
            eng.md_set_sampling(lags, 1)
        if bins is not None:
            eng.md_set_rdf(bins, r_max, every)
        states, steps, outs = [eng.md_state()[0]], [0], []
        for n in runs:
            outs.append(eng.md_run(n, DT))
            states.append(eng.md_state()[0])
            steps.append(steps[-1] + n)
        x, v = eng.md_state()
        res = dict(x=x, v=v, n_rebuilds=sum(o["n_rebuilds"] for o in outs), states=np.array(states), steps=np.array(steps))
        if bins is not None:
            res["rdf"] = eng.md_rdf()
        if lags is not None:
            res["samples"] = eng.md_samples()
    for k in ("epot", "ekin", "echain"):
        if k in outs[0]:
            res[k] = np.concatenate([o[k][1 if j else 0:] for j, o in enumerate(outs)])
    return _freeze(res)


def _describe(nn, frames):
    els = list(nn.elements)
    species = np.array([els.index(sym) for a in frames for sym in a.get_chemical_symbols()])
    cells = np.array([np.asarray(a.get_cell(complete=True)) for a in frames])
    pbc = np.array([np.broadcast_to(np.asarray(a.pbc, dtype=bool), (3,)) for a in frames])
    return dict(cells=cells, pbc=pbc, species=species, natoms=[len(a) for a in frames], n_elements=len(els))


def _reference(nn, frames, snapshots, bins, r_max):
    counts, gap = ref.pair_counts(snapshots, n_bins=bins, r_max=r_max, **_describe(nn, frames))
    print("reference: pairs", int(counts.sum()), "nearest bin edge", gap, "bins")
    assert gap > EDGE, gap   # (on the reference alone: the exact comparison below means something)
    counts.setflags(write=False)
    return counts


def _sampled(dev, every):
    """The states of a run cut at every sample: those at the multiples of `every`."""
    keep = dev["steps"] % every == 0
    keep[1:] &= dev["steps"][1:] != dev["steps"][:-1]   # (a call of 0 steps repeats a state, it is sampled once)
    return dev["states"][keep], dev["steps"][keep]


def _assert_counts(dev, want, n_samples, every, last_step, r_max):
    got = dev["rdf"]
    assert got["counts"].dtype == np.int64 and got["counts"].shape == want.shape
    assert (got["n_samples"], got["sample_every"], got["last_step"]) == (n_samples, every, last_step)
    assert got["r_max"] == r_max
    diff = got["counts"] != want
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5], got["counts"][diff][:5], want[diff][:5])


# -- 1: single frame, the full ladder ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ni_model(model):
    nn, atoms = _ni_setup()   # 32 Ni atoms, cell 7.05 < 2 rc: self-images and several shifts per neighbour
    if model == "g2":
        nn = make_nn(["Ni"], 6.0, False, [8])
    return nn, atoms


def _cuts(steps, every):
    return [every] * (steps // every) + ([steps % every] if steps % every else [])


@functools.lru_cache(maxsize=None)
def _ni_run(model, every, cut, bins=64, steps=20):
    nn, atoms = _ni_model(model)
    v0 = _velocities([atoms], 600.0, 3)
    return _run(nn, [atoms], v0, 0.3, _cuts(steps, every) if cut else [steps], bins, None, every)


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("model", ["eam", "g2"])
def test_single_frame_against_the_reference(lib, model, every):
    nn, atoms = _ni_model(model)
    dev = _ni_run(model, every, True)
    xs, steps = _sampled(dev, every)
    assert np.array_equal(steps, np.arange(0, 21, every))
    want = _reference(nn, [atoms], xs, 64, 6.0)
    assert want[0, 0, 0, :16].sum() == 0 and want.sum() > 20 * len(xs) * 32   # nothing below 1.5 A, shells beyond
    _assert_counts(dev, want, len(xs), every, int(steps[-1]), 6.0)   # r_max None: the model's cutoff


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("model", ["eam", "g2"])
def test_uncut_run_gives_the_integers_of_the_cut_run(lib, model, every):
    cut, uncut = _ni_run(model, every, True), _ni_run(model, every, False)
    assert np.array_equal(uncut["x"], cut["x"]) and np.array_equal(uncut["v"], cut["v"])
    for key in ("n_samples", "sample_every", "last_step", "r_max"):
        assert uncut["rdf"][key] == cut["rdf"][key], key
    assert np.array_equal(uncut["rdf"]["counts"], cut["rdf"]["counts"])
    assert cut["rdf"]["counts"].sum() > 0


# -- 2: two elements, one of them absent from one frame ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _nimo():
    nn = make_eam(["Mo", "Ni"], 6.0, potential="zjw04")
    frames = [_alloy(["Ni", "Mo"], rep=(2, 2, 2)), fcc(rep=(2, 2, 2), jitter=0.02, seed=3)]
    return nn, frames, _velocities(frames, 600.0, 5)


def test_two_elements_one_absent_from_a_frame(lib):
    nn, frames, v0 = _nimo()
    mo, ni = list(nn.elements).index("Mo"), list(nn.elements).index("Ni")
    dev = _run(nn, frames, v0, 0.3, _cuts(10, 2), 48, 5.5, 2)
    xs, steps = _sampled(dev, 2)
    want = _reference(nn, frames, xs, 48, 5.5)
    _assert_counts(dev, want, 6, 2, 10, 5.5)
    c = dev["rdf"]["counts"]
    assert np.array_equal(c, np.swapaxes(c, 1, 2))   # every pair is listed from both ends
    assert c[0, mo, ni].sum() > 0 and c[0, mo, mo].sum() > 0
    assert c[1, ni, ni].sum() > 0 and c[1, mo].sum() == 0 and c[1, :, mo].sum() == 0   # no Mo in frame 1
    assert np.array_equal(dev["rdf"]["n_by_element"][:, mo], [16, 0])


# -- 3: two frames of different sizes, one of them triclinic -----------------------------------------------------
def _sheared(atoms):
    m = np.eye(3) + np.array([[0.0, 0.0, 0.0], [0.12, 0.0, 0.0], [-0.07, 0.09, 0.0]])
    return Atoms(symbols=atoms.get_chemical_symbols(), positions=atoms.positions @ m,
                 cell=np.asarray(atoms.get_cell(complete=True)) @ m, pbc=True)


def test_two_frames_of_different_sizes_one_triclinic(lib):
    nn = _ni_setup()[0]
    frames = [_sheared(fcc(rep=(2, 2, 2), jitter=0.02, seed=3)), fcc(rep=(3, 3, 3), jitter=0.02, seed=4)]
    assert [len(a) for a in frames] == [32, 108]   # 108: no multiple of the 8 centres of a workgroup
    v0 = _velocities(frames, 600.0, 11)
    dev = _run(nn, frames, v0, 0.3, _cuts(8, 4), 50, 5.0, 4)
    xs, steps = _sampled(dev, 4)
    want = _reference(nn, frames, xs, 50, 5.0)
    assert want[0].sum() > 0 and want[1].sum() > want[0].sum()
    _assert_counts(dev, want, 3, 4, 8, 5.0)


# -- 4: a cluster: counts, but no g(r) ---------------------------------------------------------------------------
def test_cluster_counts_but_no_normalisation(lib):
    from tensoralloy_amd import Engine
    nn = _ni_setup()[0]
    block = fcc(rep=(2, 2, 2), jitter=0.02, seed=3)
    atoms = Atoms(symbols=block.get_chemical_symbols(), positions=block.positions + 6.0, cell=np.diag([20.0] * 3), pbc=False)
    x0 = atoms.positions.copy()
    with Engine(nn) as eng:
        dyn = md.DeviceMD(eng, atoms, DT, velocities=_velocities([atoms], 300.0, 3), rdf_bins=40, rdf_every=5)
        dyn.run(5)
        out = eng.md_rdf()
        want = _reference(nn, [atoms], np.stack([x0, atoms.positions]), 40, 6.0)
        assert want.sum() > 0 and not out["pbc"].any()
        assert (out["n_samples"], out["last_step"]) == (2, 5) and np.array_equal(out["counts"], want)
        with pytest.raises(ValueError, match="periodic in all three"):
            dyn.get_rdf()


# -- 5: list rebuilds in the middle of a run, together with md_set_sampling --------------------------------------
def test_rebuilds_and_the_position_ring(lib):
    """2000 K with a skin of 0.1: the run rebuilds its list several times, inside the windows of steps that the
    loop enqueues ahead. The snapshots are this run's own: the ring of `md_set_sampling`, on at the same time."""
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 2000.0, 3)
    dev = _run(nn, [atoms], v0, 0.1, [30], 64, None, 1, lags=32)
    assert dev["n_rebuilds"] >= 3
    assert np.array_equal(dev["samples"]["steps"], np.arange(31))
    want = _reference(nn, [atoms], dev["samples"]["x"], 64, 6.0)
    _assert_counts(dev, want, 31, 1, 30, 6.0)   # 31 samples: nothing counted twice or skipped around a redone step
    # skin 0 rebuilds at every step; every third state is sampled
    dev = _run(nn, [atoms], v0, 0.0, [7], 64, None, 3, lags=8)
    assert dev["n_rebuilds"] == 7
    want = _reference(nn, [atoms], dev["samples"]["x"][0::3], 64, 6.0)
    _assert_counts(dev, want, 3, 3, 6, 6.0)


# -- 6: edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [1, 4096])
def test_one_bin_and_the_tiled_histogram(lib, bins):
    """4096 bins of two elements are 16384 LDS words: the workgroups tile over the bins, in two passes."""
    nn, frames, v0 = _nimo()
    dev = _run(nn, frames, v0, 0.3, [4], bins, None, 4)   # r_max: the cutoff itself
    want = _reference(nn, frames, dev["states"], bins, 6.0)
    _assert_counts(dev, want, 2, 4, 4, 6.0)
    if bins == 4096:   # both halves of the tiling hold pairs
        assert want[..., :2048].sum() > 0 and want[..., 2048:].sum() > 0


def test_batch_above_16384_atoms_takes_the_wide_workgroups(lib):
    """Above 16384 atoms a workgroup owns 64 centres instead of 8. Five 4000-atom frames, two of them distinct:
    every frame's integers are those of the same frame sampled alone, which the narrow workgroups count (the
    entry state only: its coordinates are the same doubles in both runs; the brute-force reference would take
    minutes at this size)."""
    nn = _ni_setup()[0]
    a, b = fcc(rep=(10, 10, 10), jitter=0.05, seed=1), fcc(rep=(10, 10, 10), jitter=0.05, seed=2)
    frames = [a, b, a, b, a]
    v = {id(a): _velocities([a], 600.0, 7), id(b): _velocities([b], 600.0, 8)}
    dev = _run(nn, frames, np.concatenate([v[id(f)] for f in frames]), 0.3, [0], 128, None, 1)
    alone = {id(f): _run(nn, [f], v[id(f)], 0.3, [0], 128, None, 1) for f in (a, b)}
    assert dev["rdf"]["n_samples"] == 1 and dev["rdf"]["counts"].shape == (5, 1, 1, 128)
    for k, f in enumerate(frames):
        one = alone[id(f)]
        assert np.array_equal(dev["states"][:, 4000 * k:4000 * (k + 1)], one["states"])   # the same coordinates
        assert one["rdf"]["counts"].sum() > 4000 * 60
        assert np.array_equal(dev["rdf"]["counts"][k], one["rdf"]["counts"][0]), k
    assert not np.array_equal(dev["rdf"]["counts"][0], dev["rdf"]["counts"][1])


def test_sample_every_beyond_the_run_samples_the_entry_state_once(lib):
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 600.0, 3)
    dev = _run(nn, [atoms], v0, 0.3, [0, 5, 0, 6], 32, 4.0, 50)
    want = _reference(nn, [atoms], dev["states"][:1], 32, 4.0)
    _assert_counts(dev, want, 1, 50, 0, 4.0)
    # a call of 0 steps between two runs counts nothing twice either
    dev = _run(nn, [atoms], v0, 0.3, [0, 4, 0, 0, 4], 32, 4.0, 4)
    xs, steps = _sampled(dev, 4)
    assert np.array_equal(steps, [0, 4, 8])
    _assert_counts(dev, _reference(nn, [atoms], xs, 32, 4.0), 3, 4, 8, 4.0)


# -- 7: composition ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator", ["nve", "berendsen", "langevin", "nhc"])
def test_every_thermostat_and_a_pure_observer(lib, integrator):
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 2000.0, 3)
    plain = _run(nn, [atoms], v0, 0.1, [4, 4, 3], None, None, 1, integrator)
    dev = _run(nn, [atoms], v0, 0.1, [4, 4, 3], 64, 5.0, 4, integrator)
    assert dev["n_rebuilds"] == plain["n_rebuilds"] >= 1
    for k in ("x", "v", "epot", "ekin", "states") + (("echain",) if integrator == "nhc" else ()):
        assert np.array_equal(dev[k], plain[k]), k   # bit for bit: the launch only reads the state
    xs, steps = _sampled(dev, 4)
    assert np.array_equal(steps, [0, 4, 8])
    _assert_counts(dev, _reference(nn, [atoms], xs, 64, 5.0), 3, 4, 8, 5.0)


def test_device_md_end_to_end(lib):
    from tensoralloy_amd import Engine
    nn, atoms = _ni_setup()
    atoms = atoms.copy()
    x0 = atoms.positions.copy()
    v0 = _velocities([atoms], 600.0, 3)
    with Engine(nn) as eng:
        dyn = md.DeviceMD(eng, atoms, DT, velocities=v0, temperature_K=600.0, tdamp=20 * DT, rdf_bins=60, rdf_every=6,
                          n_lags=4, sample_every=2)
        dyn.run(6)
        x6 = atoms.positions.copy()
        dyn.run(5)
        out = eng.md_rdf()
        assert (out["n_samples"], out["last_step"], out["r_max"]) == (2, 6, 6.0)
        want = _reference(nn, [atoms], np.stack([x0, x6]), 60, 6.0)
        assert np.array_equal(out["counts"], want)
        r, g = dyn.get_rdf()
        assert r.shape == (60,) and g.shape == (1, 1, 60) and np.array_equal(r, (np.arange(60) + 0.5) * 0.1)
        r2, g2 = md.rdf(want[0], 2, [32], atoms.get_volume(), 6.0)
        assert np.array_equal(g, g2)
        # the first shell of fcc: twelve neighbours below 3.0 A at 600 K
        assert md.coordination_number(g[0, 0], r, 32 / atoms.get_volume(), 3.0) == pytest.approx(12.0, abs=1e-9)
        assert eng.md_correlations()["n_samples"] == 6   # md_set_sampling goes its own way: steps 0, 2, .., 10
        plain = md.DeviceMD(eng, atoms, DT, velocities=v0)   # rdf_bins None: the feature is set off
        with pytest.raises(ValueError, match=r"pair distributions are off \(rdf_bins\)"):
            plain.get_rdf()
        with pytest.raises(ValueError, match=r"pair distributions are off \(ta_md_set_rdf\)"):
            eng.md_rdf()


# -- 8: life cycle and refusals ----------------------------------------------------------------------------------
def test_life_cycle_and_refusals(lib):
    from tensoralloy_amd import Engine
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 300.0, 3)
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        with pytest.raises(ValueError, match="no resident batch"):
            eng.md_rdf()
        eng.md_set_rdf(0)   # off is always allowed
        with pytest.raises(ValueError, match="ta_md_set_rdf: no resident batch"):
            eng.md_set_rdf(8)
        eng.set_frames([atoms])
        with pytest.raises(ValueError, match="ta_md_get_rdf called before ta_md_init"):
            eng.md_rdf()
        with pytest.raises(ValueError, match="ta_md_set_rdf called before ta_md_init"):
            eng.md_set_rdf(8)
        eng.md_init(None, v0)
        with pytest.raises(ValueError, match=r"ta_md_get_rdf: the pair distributions are off \(ta_md_set_rdf\)"):
            eng.md_rdf()
        eng.md_set_rdf(8, 4.0, 2)
        for what, args in (("n_bins", (-1, 4.0, 1)), ("n_bins", (4097, 4.0, 1)), ("sample_every", (8, 4.0, 0)),
                           ("sample_every", (8, 4.0, -2)), ("r_max", (8, 0.0, 1)), ("r_max", (8, -1.0, 1)),
                           ("r_max", (8, float("nan"), 1)), ("r_max", (8, float("inf"), 1))):
            with pytest.raises(ValueError, match="ta_md_set_rdf: " + what):
                eng.md_set_rdf(*args)
        with pytest.raises(ValueError, match=r"ta_md_set_rdf: r_max = 6\.00001\d* exceeds the model's cutoff.*not complete beyond"):
            eng.md_set_rdf(8, 6.00001, 1)
        out = eng.md_rdf()   # ... and a refused call left the setting as it was
        assert out["counts"].shape == (1, 1, 1, 8) and not out["counts"].any()
        assert (out["n_samples"], out["sample_every"], out["last_step"], out["r_max"]) == (0, 2, -1, 4.0)
        res = eng.md_run(10, DT)
        assert set(res) == {"epot", "ekin", "n_rebuilds"}   # the result dict is unchanged
        assert (eng.md_rdf()["n_samples"], eng.md_rdf()["last_step"]) == (6, 10)
        # the barostat and the pair distributions together: refused by the run, both named, nothing lost
        x0, v_before = eng.md_state()
        before = eng.md_rdf()
        eng.md_set_barostat(0.0, 100 * DT, 1.0)
        with pytest.raises(ValueError, match=r"ta_md_run: the pair distributions \(ta_md_set_rdf\) and the barostat \(ta_md_set_barostat\)"):
            eng.md_run(5, DT)
        eng.md_set_barostat(0.0, 0.0, 0.0)
        x1, v1 = eng.md_state()
        after = eng.md_rdf()
        assert np.array_equal(x0, x1) and np.array_equal(v_before, v1)
        assert np.array_equal(before["counts"], after["counts"]) and after["n_samples"] == 6
        # setting it again zeroes; sample 0 is then the first multiple of sample_every not behind the step
        eng.md_run(1, DT)   # step 11
        eng.md_set_rdf(4, None, 3)
        out = eng.md_rdf()
        assert out["counts"].shape == (1, 1, 1, 4) and out["n_samples"] == 0 and not out["counts"].any() and out["r_max"] == 6.0
        eng.md_run(5, DT)   # steps 12 .. 16: samples at 12 and 15
        assert (eng.md_rdf()["n_samples"], eng.md_rdf()["last_step"]) == (2, 15)
        # set_frames keeps the setting and drops the data with the MD state; md_init starts from zero counts
        eng.set_frames([atoms])
        with pytest.raises(ValueError, match="ta_md_get_rdf called before ta_md_init"):
            eng.md_rdf()
        eng.md_init(None, v0)
        out = eng.md_rdf()
        assert out["counts"].shape == (1, 1, 1, 4) and not out["counts"].any()
        assert (out["n_samples"], out["sample_every"], out["last_step"]) == (0, 3, -1)
        eng.md_run(3, DT)
        assert (eng.md_rdf()["n_samples"], eng.md_rdf()["last_step"]) == (2, 3)
        eng.md_set_rdf(0)
        with pytest.raises(ValueError, match="pair distributions are off"):
            eng.md_rdf()
        eng.md_set_barostat(0.0, 100 * DT, 1.0)   # with the feature off the barostat runs
        eng.md_run(2, DT)


def test_getter_after_a_failed_run(lib):
    """A run that fails leaves the counts invalid until `md_set_rdf` or `md_init` is called again. The failure:
    n_steps = 2^31 - 1 with a record of 128 frames at every step asks for 2^31 x 128 x 8 bytes x 9/8 = 2.5 TB of
    `epot` records. `ta_md_run` allocates them first, inside its guarded body and behind the point where it marks
    the counts invalid; the allocation is refused and nothing is launched: positions and velocities are untouched.
    (Called through the C ABI with null record pointers, so that the host allocates nothing either.)"""
    from tensoralloy_amd import Engine, _lib
    nn, atoms = _ni_setup()
    frames = [atoms] * 128
    v0 = np.tile(_velocities([atoms], 300.0, 3), (128, 1))
    null = C.POINTER(C.c_double)()

    def failing_run(eng):
        x0, v_before = eng.md_state()
        rc = eng._lib.ta_md_run(eng._handle, 2 ** 31 - 1, DT, WANT, 1, null, null, None)
        msg = eng._lib.ta_last_error(eng._handle).decode()
        print("failed run:", rc, msg)
        assert rc in (_lib.TA_ERR_HIP, _lib.TA_ERR_NOMEM) and "hipMalloc" in msg
        x1, v1 = eng.md_state()
        assert np.array_equal(x0, x1) and np.array_equal(v_before, v1)

    refusal = r"ta_md_get_rdf: a ta_md_run failed and left the counts invalid; call ta_md_set_rdf or ta_md_init again"
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        eng.set_frames(frames)
        eng.md_init(None, v0)
        eng.md_set_rdf(16, 4.0, 1)
        eng.md_run(2, DT)
        assert eng.md_rdf()["n_samples"] == 3
        failing_run(eng)
        with pytest.raises(ValueError, match=refusal):
            eng.md_rdf()
        eng.md_run(1, DT)   # the loop goes on (step 3) and counts nothing; the getter still refuses
        with pytest.raises(ValueError, match=refusal):
            eng.md_rdf()
        eng.md_set_rdf(16, 4.0, 1)   # set again: zero counts, sample 0 is the state of step 3
        out = eng.md_rdf()
        assert (out["n_samples"], out["last_step"]) == (0, -1) and not out["counts"].any()
        eng.md_run(2, DT)
        out = eng.md_rdf()
        assert (out["n_samples"], out["last_step"]) == (3, 5)
        assert out["counts"][0].sum() > 0 and out["counts"][127].sum() > 0
        failing_run(eng)
        with pytest.raises(ValueError, match=refusal):
            eng.md_rdf()
        eng.md_init(None, v0)   # ... or md_init: the setting is kept, the counts start from zero
        out = eng.md_rdf()
        assert (out["n_samples"], out["sample_every"], out["last_step"]) == (0, 1, -1) and not out["counts"].any()
        eng.md_run(1, DT)
        assert eng.md_rdf()["n_samples"] == 2
