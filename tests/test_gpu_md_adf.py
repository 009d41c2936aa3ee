"""GPU: bond-angle distributions inside the device MD loop (`ta_md_set_adf`, csrc/ta_md_adf.hip) against the NumPy
definition (tests/md_adf_reference.py), which sweeps all atoms and all periodic images by brute force and shares
nothing with the library's neighbour list.

The counts are integers, so the comparison is EXACT. That needs no angle on a bin edge and no neighbour on a
cutoff: every exact test first asserts, on the reference alone, that no theta / dtheta of its snapshots lies within
1e-9 of an integer 1 .. B - 1 and that no r / rb lies within 1e-9 of 1. This is a condition on the inputs, not a
tolerance: the device and the reference form theta and r from the same doubles with a few ulps (1e-16 relative, at
most 4e-13 bins at B = 4096) between them; with 1e4 .. 1e6 triples per case the nearest edge is typically 1e-5 ..
1e-7 bins away. A perfect fcc lattice has all its angles at 60 / 90 / 120 / 180 degrees, bin edges at B = 180, so
every test starts from seeded, jittered positions; where lattice vectors themselves are neighbours (self-images in
a cell below the cutoff, exactly 90 degrees apart in a cubic cell) B is 181. The snapshots are the device's own
whole-step states: `md_state()` between the calls of a cut run, or the position ring of `md_set_sampling`.

The run that fails (for the getter behind it) fails on the host: its record buffers, 2^31 records of 128 frames,
are 2.5 TB that no device has, and `ta_md_run` allocates them before it enqueues anything.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from tests import md_adf_reference as ref
from tests import md_rdf_reference as rdf_ref
from tests.helpers import fcc, make_eam
from tests.test_gpu_md import DT, WANT, _ni_setup, _velocities
from tests.test_gpu_md_rdf import SETUPS, _describe, _freeze, _nimo, _sampled, _sheared
from tensoralloy_amd import Atoms, md

pytestmark = pytest.mark.gpu

EDGE = 1e-9   # bins, and relative distance to a cutoff: nothing of the reference may be nearer


@functools.lru_cache(maxsize=None)
def _kernel_constant(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "tensoralloy_amd", "csrc", "ta_md.h")) as fp:
        return int(re.search(r"constexpr int %s = (\d+);" % name, fp.read()).group(1))


def _run(nn, frames, v0, skin, runs, bins=None, r_bond=None, every=1, integrator="nve", lags=None, dt=DT,
         barostat=None):
    """The runs `runs` (steps per md_run call) on the device: final state, records, the whole-step positions (and
    cells) at entry and behind every call (`states`, `cells`, at the absolute steps `steps`), and with `bins` the
    counts (`adf`). `lags`: `md_set_sampling(lags, 1)` is on as well and its ring is returned (`samples`)."""
    from tensoralloy_amd import Engine
    with Engine(nn) as eng:
        eng.set_skin(skin)
        eng.set_frames(frames)
        eng.md_init(None, v0)
        SETUPS[integrator](eng)
        if barostat is not None:
            eng.md_set_barostat(*barostat)
        if lags is not None:
            eng.md_set_sampling(lags, 1)
        if bins is not None:
            eng.md_set_adf(bins, r_bond, every)
        states, cells, steps, outs = [eng.md_state()[0]], [eng.md_cells()], [0], []
        for n in runs:
            outs.append(eng.md_run(n, dt))
            states.append(eng.md_state()[0])
            cells.append(eng.md_cells())
            steps.append(steps[-1] + n)
        x, v = eng.md_state()
        res = dict(x=x, v=v, n_rebuilds=sum(o["n_rebuilds"] for o in outs), states=np.array(states),
                   cells=np.array(cells), steps=np.array(steps))
        if bins is not None:
            res["adf"] = eng.md_adf()
        if lags is not None:
            res["samples"] = eng.md_samples()
    for k in ("epot", "ekin", "echain"):
        if k in outs[0]:
            res[k] = np.concatenate([o[k][1 if j else 0:] for j, o in enumerate(outs)])
    return _freeze(res)


def _reference(nn, frames, snapshots, bins, r_bond, cells=None, stats=None):
    d = _describe(nn, frames)
    if cells is not None:
        d["cells"] = cells
    counts, gap_theta, gap_r = ref.triple_counts(snapshots, n_bins=bins, r_bond=r_bond, stats=stats, **d)
    print("reference: triples", int(counts.sum()), "nearest bin edge", gap_theta, "bins, nearest cutoff", gap_r)
    assert gap_theta >= EDGE and gap_r >= EDGE, (gap_theta, gap_r)   # (on the reference alone)
    counts.setflags(write=False)
    return counts


def _assert_counts(dev, want, n_samples, every, last_step, r_bond=None):
    got = dev["adf"]
    E = want.shape[1]
    assert got["counts"].dtype == np.int64 and got["counts"].shape == want.shape
    assert (got["n_samples"], got["n_bins"], got["sample_every"], got["last_step"]) == (n_samples, want.shape[-1], every, last_step)
    assert got["pairs"] == [(b, c) for b in range(E) for c in range(b, E)]
    if r_bond is not None:
        assert np.array_equal(got["r_bond"], np.broadcast_to(np.asarray(r_bond, dtype=np.float64), (E, E)))
    diff = got["counts"] != want
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5], got["counts"][diff][:5], want[diff][:5])


# -- 1, 2: single frame; cutting --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ni108():
    return _ni_setup()[0], fcc(rep=(3, 3, 3), jitter=0.05, seed=17)


@functools.lru_cache(maxsize=None)
def _ni108_run(every, runs):
    nn, atoms = _ni108()
    return _run(nn, [atoms], _velocities([atoms], 600.0, 3), 0.3, list(runs), 180, 3.0, every, lags=16)


@pytest.mark.parametrize("every", [1, 3])
def test_single_frame_against_the_reference(lib, every):
    nn, atoms = _ni108()
    dev = _ni108_run(every, (12,))
    assert np.array_equal(dev["samples"]["steps"], np.arange(13))
    stats = {}
    want = _reference(nn, [atoms], dev["samples"]["x"][::every], 180, 3.0, stats=stats)
    assert abs(stats["n_neighbours"].mean() - 12.0) < 0.5   # the first shell of fcc
    assert want.sum() > 50 * 108 * len(range(0, 13, every))
    _assert_counts(dev, want, len(range(0, 13, every)), every, 12 // every * every, 3.0)


@pytest.mark.parametrize("every", [1, 3])
def test_cut_run_gives_the_integers_of_the_uncut_run(lib, every):
    uncut, cut = _ni108_run(every, (12,)), _ni108_run(every, (5, 0, 1, 4, 2))
    assert np.array_equal(uncut["x"], cut["x"]) and np.array_equal(uncut["v"], cut["v"])
    for key in ("n_samples", "n_bins", "sample_every", "last_step"):
        assert uncut["adf"][key] == cut["adf"][key], key
    assert np.array_equal(uncut["adf"]["counts"], cut["adf"]["counts"]) and cut["adf"]["counts"].sum() > 0


# -- 3: two elements, a cutoff per pair, one element absent from one frame -------------------------------------
def test_two_elements_with_a_cutoff_per_pair(lib):
    nn, frames, v0 = _nimo()
    mo, ni = list(nn.elements).index("Mo"), list(nn.elements).index("Ni")
    rb = np.zeros((2, 2))
    rb[mo, mo], rb[ni, ni], rb[mo, ni], rb[ni, mo] = 3.9, 2.9, 3.3, 3.3
    dev = _run(nn, frames, v0, 0.3, [10], 90, rb, 2, lags=16)
    want = _reference(nn, frames, dev["samples"]["x"][::2], 90, rb)
    _assert_counts(dev, want, 6, 2, 10, rb)
    c = dev["adf"]["counts"]
    pairs = dev["adf"]["pairs"]
    for a in (mo, ni):   # frame 0 holds both elements: every block [a][p] has triples
        for p in range(3):
            assert c[0, a, p].sum() > 0, (a, pairs[p])
    # the three cutoffs matter: with any one of them everywhere the counts of frame 0 differ
    for r in (2.9, 3.3, 3.9):
        other, _, _ = ref.triple_counts(dev["samples"]["x"][::2], n_bins=90, r_bond=r, **_describe(nn, frames))
        assert not np.array_equal(other[0], want[0]), r
    # no Mo in frame 1: only Ni centres with two Ni neighbours
    only = pairs.index((ni, ni))
    assert c[1, ni, only].sum() > 0 and c[1, mo].sum() == 0
    assert all(c[1, ni, p].sum() == 0 for p in range(3) if p != only)


# -- 4: frames of different sizes, one triclinic, one a cluster ---------------------------------------------------
def test_unequal_frames_one_triclinic_one_cluster(lib):
    nn = _ni_setup()[0]
    block = fcc(rep=(2, 2, 2), jitter=0.05, seed=5)
    cluster = Atoms(symbols=block.get_chemical_symbols(), positions=block.positions + 6.0, cell=np.diag([20.0] * 3), pbc=False)
    frames = [_sheared(fcc(rep=(2, 2, 2), jitter=0.05, seed=3)), fcc(rep=(3, 3, 3), jitter=0.05, seed=4), cluster]
    assert [len(a) for a in frames] == [32, 108, 32]   # 108: no multiple of the 8 centres of a workgroup
    v0 = _velocities(frames, 600.0, 11)
    dev = _run(nn, frames, v0, 0.3, [8], 120, 3.1, 4, lags=16)
    stats = {}
    want = _reference(nn, frames, dev["samples"]["x"][::4], 120, 3.1, stats=stats)
    n = stats["n_neighbours"]   # frame by frame, three snapshots each
    assert n[:3 * 140].mean() > 11.0 and n[3 * 140:].min() <= 5   # the corner atoms of the cluster have few neighbours
    assert want[1].sum() > want[0].sum() > want[2].sum() > 0
    _assert_counts(dev, want, 3, 4, 8, 3.1)


# -- 5: the bond cutoff at the model's cutoff in a cell far smaller than it --------------------------------------
def test_long_cutoff_in_a_tiny_cell_takes_the_tiled_sweep(lib):
    """Four Ni atoms in a cubic cell of 3.2 A under a model with a cutoff of 6.5 A: every centre has some 140
    neighbours, more than the kMdAdfSlab = 128 a wave holds in LDS at a time, among them its own images and
    several images of every other atom. Lattice vectors are neighbours here and are exactly 90 degrees apart:
    B = 181 keeps them off the bin edges."""
    nn = make_eam(["Ni"], 6.5, potential="zjw04")
    atoms = fcc(a=3.2, rep=(1, 1, 1), jitter=0.05, seed=9)
    dev = _run(nn, [atoms], _velocities([atoms], 300.0, 3), 0.3, [2, 2], 181, None, 2)
    xs, steps = _sampled(dev, 2)
    assert np.array_equal(steps, [0, 2, 4])
    stats = {}
    want = _reference(nn, [atoms], xs, 181, 6.5, stats=stats)
    print("neighbours per centre:", stats["n_neighbours"])
    assert stats["n_neighbours"].max() > _kernel_constant("kMdAdfSlab") == 128
    assert want[0, 0, 0, 180] >= 3 * 4 * 16   # the 32 lattice vectors below 6.5 A in opposite pairs: 180 degrees
    _assert_counts(dev, want, 3, 2, 4, 6.5)   # r_bond None: the model's cutoff
    # ... and the 32-atom cell of 7.05 A at its model's cutoff of 6.0 A (some 80 neighbours: the slab alone)
    nn, atoms = _ni_setup()
    dev = _run(nn, [atoms], _velocities([atoms], 600.0, 3), 0.3, [3], 180, None, 3, lags=4)
    stats = {}
    want = _reference(nn, [atoms], dev["samples"]["x"][::3], 180, 6.0, stats=stats)
    assert 64 < stats["n_neighbours"].max() <= 128
    _assert_counts(dev, want, 2, 3, 3, 6.0)


# -- 6: edges of the bin count -----------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [1, 4096])
def test_one_bin_and_the_tiled_histogram(lib, bins):
    """4096 bins of two elements are 2 x 3 x 4096 = 24576 LDS words: the workgroups tile over the bins, in four
    passes of 1365 bins."""
    nn, frames, v0 = _nimo()
    dev = _run(nn, frames, v0, 0.3, [4], bins, 3.3, 4)
    stats = {}
    want = _reference(nn, frames, dev["states"], bins, 3.3, stats=stats)
    _assert_counts(dev, want, 2, 4, 4, 3.3)
    n = stats["n_neighbours"]
    assert want.sum() == (n * (n - 1) // 2).sum() > 0   # every triple lands somewhere
    if bins == 1:
        assert want.shape == (2, 2, 3, 1)
    else:
        per_pass = _kernel_constant("kMdAdfLdsWords") // (2 * 3)
        assert per_pass < 4096
        assert per_pass == 1365   # passes of bins 0 .. 1364, .. 2729, .. 4094 and the last bin alone
        for lo in (0, per_pass, 2 * per_pass):   # the three wide passes hold triples
            assert want[..., lo:lo + per_pass].sum() > 0, lo


# -- 7: the launch plan above 16384 atoms ------------------------------------------------------------------------
def test_batch_above_16384_atoms_takes_the_wide_workgroups(lib):
    """Above 16384 atoms a workgroup owns 64 centres instead of 8. Five 4000-atom frames, two of them distinct:
    every frame's integers are those of the same frame sampled alone, which the narrow workgroups count (the
    entry state only: its coordinates are the same doubles in both runs; the brute-force reference would take
    minutes at this size)."""
    nn = _ni_setup()[0]
    a, b = fcc(rep=(10, 10, 10), jitter=0.05, seed=1), fcc(rep=(10, 10, 10), jitter=0.05, seed=2)
    frames = [a, b, a, b, a]
    v = {id(a): _velocities([a], 600.0, 7), id(b): _velocities([b], 600.0, 8)}
    dev = _run(nn, frames, np.concatenate([v[id(f)] for f in frames]), 0.3, [0], 180, 3.0, 1)
    alone = {id(f): _run(nn, [f], v[id(f)], 0.3, [0], 180, 3.0, 1) for f in (a, b)}
    assert dev["adf"]["n_samples"] == 1 and dev["adf"]["counts"].shape == (5, 1, 1, 180)
    for k, f in enumerate(frames):
        one = alone[id(f)]
        assert np.array_equal(dev["states"][:, 4000 * k:4000 * (k + 1)], one["states"])   # the same coordinates
        assert one["adf"]["counts"].sum() > 4000 * 50
        assert np.array_equal(dev["adf"]["counts"][k], one["adf"]["counts"][0]), k
    assert not np.array_equal(dev["adf"]["counts"][0], dev["adf"]["counts"][1])


# -- 8: list rebuilds in the middle of a run ----------------------------------------------------------------------
def test_rebuilds_inside_the_window(lib):
    """2000 K with a skin of 0.1: the run rebuilds its list several times, inside the windows of steps that the
    loop enqueues ahead. The snapshots are this run's own: the ring of `md_set_sampling`, on at the same time."""
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 2000.0, 3)
    dev = _run(nn, [atoms], v0, 0.1, [30], 180, 3.0, 1, lags=32)
    assert dev["n_rebuilds"] >= 3
    assert np.array_equal(dev["samples"]["steps"], np.arange(31))
    want = _reference(nn, [atoms], dev["samples"]["x"], 180, 3.0)
    _assert_counts(dev, want, 31, 1, 30, 3.0)   # 31 samples: nothing counted twice or skipped around a redone step
    # skin 0 rebuilds at every step; every third state is sampled
    dev = _run(nn, [atoms], v0, 0.0, [7], 180, 3.0, 3, lags=8)
    assert dev["n_rebuilds"] == 7
    want = _reference(nn, [atoms], dev["samples"]["x"][0::3], 180, 3.0)
    _assert_counts(dev, want, 3, 3, 6, 3.0)


# -- 9: thermostats, a pure observer, the barostat ---------------------------------------------------------------
@pytest.mark.parametrize("integrator", ["nve", "berendsen", "langevin", "nhc"])
def test_every_thermostat(lib, integrator):
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 2000.0, 3)
    plain = _run(nn, [atoms], v0, 0.1, [4, 4, 3], None, None, 1, integrator)
    dev = _run(nn, [atoms], v0, 0.1, [4, 4, 3], 180, 3.0, 4, integrator)
    assert dev["n_rebuilds"] == plain["n_rebuilds"] >= 1
    for k in ("x", "v", "epot", "ekin", "states") + (("echain",) if integrator == "nhc" else ()):
        assert np.array_equal(dev[k], plain[k]), k   # bit for bit: the launch only reads the state
    xs, steps = _sampled(dev, 4)
    assert np.array_equal(steps, [0, 4, 8])
    _assert_counts(dev, _reference(nn, [atoms], xs, 180, 3.0), 3, 4, 8, 3.0)


def test_a_pure_observer(lib):
    """dt = 0: the state does not move, every step samples it again."""
    nn, atoms = _ni_setup()
    dev = _run(nn, [atoms], _velocities([atoms], 600.0, 3), 0.3, [3, 2], 180, 3.0, 1, dt=0.0)
    assert np.array_equal(dev["states"][0], dev["x"])
    one = _reference(nn, [atoms], dev["states"][:1], 180, 3.0)
    _assert_counts(dev, 6 * one, 6, 1, 5, 3.0)


def test_under_the_barostat_with_the_cells_of_the_sampled_state(lib):
    """Cell and atoms scaled by 1.02, P0 = 0, taup = 20 fs: the cell shrinks from the first step on. The run cut
    at every sampled step hands out the positions (`md_state`) and the cells (`ta_md_get_cell`) of those states
    for the reference; one uncut run must give the same integers. The bonds reach to 6.0 A, with images of the
    7.19 A cell among the neighbours, so that the cells enter."""
    nn, atoms = _ni_setup()
    big = Atoms(symbols=atoms.get_chemical_symbols(), positions=atoms.positions * 1.02,
                cell=np.asarray(atoms.get_cell(complete=True)) * 1.02, pbc=True)
    v0 = _velocities([big], 600.0, 3)
    baro = (0.0, 20 * DT, 0.9)
    cut = _run(nn, [big], v0, 0.3, [3, 3, 2], 180, 5.9, 3, "berendsen", barostat=baro)
    uncut = _run(nn, [big], v0, 0.3, [8], 180, 5.9, 3, "berendsen", barostat=baro)
    xs, steps = _sampled(cut, 3)
    cells = cut["cells"][np.isin(cut["steps"], steps)]
    assert np.array_equal(steps, [0, 3, 6]) and cells.shape == (3, 1, 3, 3)
    assert abs(np.linalg.det(cells[2, 0])) < abs(np.linalg.det(cells[1, 0])) < abs(np.linalg.det(cells[0, 0]))
    want = _reference(nn, [big], xs, 180, 5.9, cells=cells)
    stale, _, _ = ref.triple_counts(xs, n_bins=180, r_bond=5.9, **_describe(nn, [big]))
    assert not np.array_equal(stale, want)   # (with the cell of the entry state throughout the counts differ)
    _assert_counts(cut, want, 3, 3, 6, 5.9)
    _assert_counts(uncut, want, 3, 3, 6, 5.9)


# -- 10: life cycle and refusals ---------------------------------------------------------------------------------
def test_life_cycle_and_refusals(lib):
    from tensoralloy_amd import Engine
    nn, frames, v0 = _nimo()
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        with pytest.raises(ValueError, match="no resident batch"):
            eng.md_adf()
        eng.md_set_adf(0)   # off is always allowed
        assert eng.md_adf_bins == 0
        with pytest.raises(ValueError, match="ta_md_set_adf: no resident batch"):
            eng.md_set_adf(8)
        eng.set_frames(frames)
        with pytest.raises(ValueError, match="ta_md_get_adf called before ta_md_init"):
            eng.md_adf()
        with pytest.raises(ValueError, match="ta_md_set_adf called before ta_md_init"):
            eng.md_set_adf(8)
        eng.md_init(None, v0)
        with pytest.raises(ValueError, match=r"ta_md_get_adf: the bond-angle distributions are off \(ta_md_set_adf\)"):
            eng.md_adf()
        rb = np.array([[3.5, 3.2], [3.2, 3.0]])
        eng.md_set_adf(8, rb, 2)
        assert eng.md_adf_bins == 8
        nan, inf = float("nan"), float("inf")
        for what, args in (("n_bins", (-1, 3.0, 1)), ("n_bins", (4097, 3.0, 1)), ("sample_every", (8, 3.0, 0)),
                           ("sample_every", (8, 3.0, -2)), ("r_bond must", (8, 0.0, 1)), ("r_bond must", (8, -1.0, 1)),
                           ("r_bond must", (8, nan, 1)), ("r_bond must", (8, inf, 1)),
                           (r"r_bond_pairs\[0\]\[1\] must", (8, [[3.0, nan], [nan, 3.0]], 1)),
                           (r"r_bond_pairs\[1\]\[1\] must", (8, [[3.0, 3.0], [3.0, 0.0]], 1)),
                           (r"r_bond_pairs\[1\]\[0\] = 6\.5\d* exceeds the model's cutoff", (8, [[3.0, 3.0], [6.5, 3.0]], 1)),
                           (r"r_bond_pairs is not symmetric: \[0\]\[1\]", (8, [[3.0, 3.1], [3.2, 3.0]], 1))):
            with pytest.raises(ValueError, match="ta_md_set_adf: " + what):
                eng.md_set_adf(*args)
        with pytest.raises(ValueError, match=r"ta_md_set_adf: r_bond = 6\.00001\d* exceeds the model's cutoff.*not complete beyond"):
            eng.md_set_adf(8, 6.00001, 1)
        with pytest.raises(ValueError, match=r"md_set_adf: r_bond must be one distance or \[2, 2\]"):
            eng.md_set_adf(8, [3.0, 3.0, 3.0], 1)
        out = eng.md_adf()   # ... and a refused call left the setting as it was
        assert out["counts"].shape == (2, 2, 3, 8) and not out["counts"].any() and np.array_equal(out["r_bond"], rb)
        assert (out["n_samples"], out["n_bins"], out["sample_every"], out["last_step"]) == (0, 8, 2, -1)
        res = eng.md_run(10, DT)
        assert set(res) == {"epot", "ekin", "n_rebuilds"}   # the result dict is unchanged
        out = eng.md_adf()
        assert (out["n_samples"], out["last_step"]) == (6, 10) and out["counts"].sum() > 0
        # setting it again zeroes; sample 0 is then the first multiple of sample_every not behind the step
        eng.md_run(1, DT)   # step 11
        eng.md_set_adf(4, None, 3)
        out = eng.md_adf()
        assert out["counts"].shape == (2, 2, 3, 4) and out["n_samples"] == 0 and not out["counts"].any()
        assert np.array_equal(out["r_bond"], np.full((2, 2), 6.0))
        eng.md_run(5, DT)   # steps 12 .. 16: samples at 12 and 15
        assert (eng.md_adf()["n_samples"], eng.md_adf()["last_step"]) == (2, 15)
        # off and on again: zero counts
        eng.md_set_adf(0)
        assert eng.md_adf_bins == 0
        with pytest.raises(ValueError, match="bond-angle distributions are off"):
            eng.md_adf()
        eng.md_run(1, DT)   # step 17, nothing counted
        eng.md_set_adf(4, 3.0, 3)
        out = eng.md_adf()
        assert out["n_samples"] == 0 and not out["counts"].any()
        # set_frames keeps the setting and drops the data with the MD state; md_init starts from zero counts
        eng.set_frames(frames)
        with pytest.raises(ValueError, match="ta_md_get_adf called before ta_md_init"):
            eng.md_adf()
        eng.md_init(None, v0)
        out = eng.md_adf()
        assert out["counts"].shape == (2, 2, 3, 4) and not out["counts"].any() and np.array_equal(out["r_bond"], np.full((2, 2), 3.0))
        assert (out["n_samples"], out["sample_every"], out["last_step"]) == (0, 3, -1)
        eng.md_run(3, DT)
        assert (eng.md_adf()["n_samples"], eng.md_adf()["last_step"]) == (2, 3)
        # the barostat does not exclude this feature
        eng.md_set_barostat(0.0, 100 * DT, 1.0)
        eng.md_run(3, DT)
        assert (eng.md_adf()["n_samples"], eng.md_adf()["last_step"]) == (3, 6)


def test_getter_after_a_failed_run(lib):
    """A run that fails leaves the counts invalid until `md_set_adf` or `md_init` is called again. The failure:
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

    refusal = r"ta_md_get_adf: a ta_md_run failed and left the counts invalid; call ta_md_set_adf or ta_md_init again"
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        eng.set_frames(frames)
        eng.md_init(None, v0)
        eng.md_set_adf(16, 3.0, 1)
        eng.md_run(2, DT)
        assert eng.md_adf()["n_samples"] == 3
        failing_run(eng)
        with pytest.raises(ValueError, match=refusal):
            eng.md_adf()
        eng.md_run(1, DT)   # the loop goes on (step 3) and counts nothing; the getter still refuses
        with pytest.raises(ValueError, match=refusal):
            eng.md_adf()
        eng.md_set_adf(16, 3.0, 1)   # set again: zero counts, sample 0 is the state of step 3
        out = eng.md_adf()
        assert (out["n_samples"], out["last_step"]) == (0, -1) and not out["counts"].any()
        eng.md_run(2, DT)
        out = eng.md_adf()
        assert (out["n_samples"], out["last_step"]) == (3, 5)
        assert out["counts"][0].sum() > 0 and out["counts"][127].sum() > 0
        failing_run(eng)
        with pytest.raises(ValueError, match=refusal):
            eng.md_adf()
        eng.md_init(None, v0)   # ... or md_init: the setting is kept, the counts start from zero
        out = eng.md_adf()
        assert (out["n_samples"], out["sample_every"], out["last_step"]) == (0, 1, -1) and not out["counts"].any()
        eng.md_run(1, DT)
        assert eng.md_adf()["n_samples"] == 2


# -- 11: end to end ----------------------------------------------------------------------------------------------
def test_device_md_end_to_end_with_the_other_observables(lib):
    from tensoralloy_amd import Engine
    nn, atoms = _ni_setup()
    atoms = atoms.copy()
    x0 = atoms.positions.copy()
    v0 = _velocities([atoms], 600.0, 3)
    with Engine(nn) as eng:
        dyn = md.DeviceMD(eng, atoms, DT, velocities=v0, temperature_K=600.0, tdamp=20 * DT, adf_bins=180, adf_rbond=3.0,
                          adf_every=3, rdf_bins=60, rdf_every=6, n_lags=16, sample_every=1)
        dyn.run(6)
        x6 = atoms.positions.copy()
        dyn.run(5)
        samples = eng.md_samples()
        assert np.array_equal(samples["steps"], np.arange(12))
        assert np.array_equal(samples["x"][0], x0) and np.array_equal(samples["x"][6], x6)
        out = eng.md_adf()
        assert (out["n_samples"], out["n_bins"], out["sample_every"], out["last_step"]) == (4, 180, 3, 9)
        want = _reference(nn, [atoms], samples["x"][0:10:3], 180, 3.0)
        assert np.array_equal(out["counts"], want)
        theta, p = dyn.get_adf()
        assert theta.shape == (180,) and p.shape == (1, 1, 180) and np.array_equal(theta, np.arange(180) + 0.5)
        assert (p[0, 0] * 1.0).sum() == pytest.approx(1.0, abs=1e-12)   # bins of one degree
        assert np.array_equal(p, md.adf(want[0])[1])
        assert p[0, 0, 50:70].sum() > 0.25 and p[0, 0, :40].sum() == 0.0   # fcc: a peak at 60 degrees, nothing below 40
        # the pair distributions (steps 0 and 6) and the correlations (12 samples) beside it, against their references
        rdf = eng.md_rdf()
        want_rdf, gap = rdf_ref.pair_counts(np.stack([x0, x6]), n_bins=60, r_max=6.0, **_describe(nn, [atoms]))
        assert gap > EDGE and (rdf["n_samples"], rdf["last_step"]) == (2, 6) and np.array_equal(rdf["counts"], want_rdf)
        corr = eng.md_correlations()
        assert corr["n_samples"] == 12
        dx = samples["x"][3:] - samples["x"][:-3]
        assert corr["msd"][0, 0, 3] == pytest.approx((dx * dx).sum(axis=-1).mean(), rel=1e-12)
        vv = (samples["v"][3:] * samples["v"][:-3]).sum(axis=-1).mean()
        assert corr["vacf"][0, 0, 3] == pytest.approx(vv, rel=1e-12)
        plain = md.DeviceMD(eng, atoms, DT, velocities=v0)   # adf_bins None: the feature is set off
        assert eng.md_adf_bins == 0
        with pytest.raises(ValueError, match=r"bond-angle distributions are off \(adf_bins\)"):
            plain.get_adf()
        with pytest.raises(ValueError, match=r"bond-angle distributions are off \(ta_md_set_adf\)"):
            eng.md_adf()


def test_a_run_without_the_feature_is_bit_identical(lib):
    """`DeviceMD(adf_bins=None)` on an engine that had the feature on, against a handle that never heard of it."""
    from tensoralloy_amd import Engine
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 2000.0, 3)

    def trajectory(eng, first):
        a = atoms.copy()
        if first:
            md.DeviceMD(eng, a.copy(), DT, velocities=v0, adf_bins=32, adf_rbond=3.0).run(3)
        eng.set_skin(0.1)
        dyn = md.DeviceMD(eng, a, DT, velocities=v0, temperature_K=600.0, tdamp=20 * DT)
        out = eng.md_run(12, DT)
        return out, eng.md_state(), dyn

    with Engine(nn) as eng_a, Engine(nn) as eng_b:
        out_a, (xa, va), _ = trajectory(eng_a, True)
        out_b, (xb, vb), _ = trajectory(eng_b, False)
        assert eng_a.md_adf_bins == 0
        assert set(out_a) == set(out_b) and out_a["n_rebuilds"] == out_b["n_rebuilds"] >= 1
        for k in ("epot", "ekin", "echain"):
            assert np.array_equal(out_a[k], out_b[k]), k
        assert np.array_equal(xa, xb) and np.array_equal(va, vb)
