"""GPU: the common neighbour analysis inside the device MD loop (`ta_md_set_cna`, csrc/ta_md_cna.hip) against the
brute-force definition (tests/md_cna_reference.py), which sweeps all atoms and all periodic images, has a sort, an
adjacency and a chain search of its own and shares nothing with the library's neighbour list.

Every integer is compared EXACTLY, `r_local` to 1e-12 relative. That needs no candidate on the reach, no tie at the
edge of a selection and no neighbour pair on a bond cutoff: every exact test first asserts, on the reference alone, that
`gap_r`, `gap_sel` and `gap_bond` are at least 1e-9. The snapshots are the device's own whole-step states: `md_state()`
between the calls of a cut run, or the position ring of `md_set_sampling`.

The run that fails (for the getters behind it) fails on the host, as in tests/test_gpu_md_order.py: its record
buffers are 2.5 TB that no device has, and `ta_md_run` allocates them before it enqueues anything.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import md_cna_reference as ref
from tests.helpers import fcc, hcp
from tests.test_gpu_md import DT, WANT, _ni_setup, _velocities
from tests.test_gpu_md_clusters import _half_ordered
from tests.test_gpu_md_rdf import SETUPS, _describe, _freeze, _nimo, _sampled
from tensoralloy_amd import Atoms, md

pytestmark = pytest.mark.gpu

EDGE = 1e-9        # conditions on the reference, not tolerances
R_MODEL = 6.0      # max(rcut, acut) of the models of these tests: the default reach
R_LOCAL_TOL = 1e-12


def _setting(mode="adaptive", r_cut=None, r_max=None, n_series=1, sample_every=1):
    return dict(mode=mode, r_cut=r_cut, r_max=r_max, n_series=n_series, sample_every=sample_every)


def _run(nn, frames, v0, skin, runs, cna=None, order=None, cluster=None, integrator="nve", lags=None, dt=DT, barostat=None):
    """The runs `runs` (steps per md_run call) on the device: final state, the whole-step positions (and cells) at
    entry and behind every call (`states`, `cells`, at the absolute steps `steps`), and with `cna` (the arguments of
    `md_set_cna`) what `md_cna` and `md_cna_atoms` return (`cna`, `atoms`). `order`, `cluster`: `md_set_order` and
    `md_set_clusters` are on as well; `lags`: `md_set_sampling(lags, 1)` too (`samples`)."""
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
        if order is not None:
            eng.md_set_order(*order)
        if cluster is not None:
            eng.md_set_clusters(**cluster)
        if cna is not None:
            eng.md_set_cna(**cna)
        states, cells, steps, outs = [eng.md_state()[0]], [eng.md_cells()], [0], []
        for n in runs:
            outs.append(eng.md_run(n, dt))
            states.append(eng.md_state()[0])
            cells.append(eng.md_cells())
            steps.append(steps[-1] + n)
        x, v = eng.md_state()
        res = dict(x=x, v=v, n_rebuilds=sum(o["n_rebuilds"] for o in outs), states=np.array(states),
                   cells=np.array(cells), steps=np.array(steps))
        if cna is not None:
            res["cna"] = eng.md_cna()
            res["atoms"] = eng.md_cna_atoms()
        if order is not None:
            res["order"] = eng.md_order()
            res["order_atoms"] = eng.md_order_atoms()
        if cluster is not None:
            res["clusters"] = eng.md_clusters()
            res["cluster_atoms"] = eng.md_cluster_atoms()
        if lags is not None:
            res["samples"] = eng.md_samples()
    for k in ("epot", "ekin"):
        res[k] = np.concatenate([o[k][1 if j else 0:] for j, o in enumerate(outs)])
    return _freeze(res)


def _reference(nn, frames, snapshots, setting, cells=None):
    """The reference on the snapshots (one per sample), after the conditions on the reference alone."""
    d = _describe(nn, frames)
    if cells is not None:
        d["cells"] = cells
    r_max = R_MODEL if setting["r_max"] is None else setting["r_max"]
    out = ref.cna(snapshots, mode=setting["mode"], r_cut=setting["r_cut"], r_max=r_max, **d)
    print("reference: gaps", out["gap_r"], out["gap_sel"], out["gap_bond"], "rows",
          out["series"].reshape(len(snapshots), -1).tolist()[:13])
    assert out["gap_r"] >= EDGE and out["gap_sel"] >= EDGE and out["gap_bond"] >= EDGE   # (on the reference alone)
    return _freeze(out)


def _assert_cna(dev, want, setting, sample_steps):
    """Counts, series rows (the newest n_series, oldest first, with their steps), info and per-atom arrays."""
    got, atoms = dev["cna"], dev["atoms"]
    n, T, every = len(sample_steps), setting["n_series"], setting["sample_every"]
    rows = min(n, T)
    assert (got["n_samples"], got["mode"], got["sample_every"], got["last_step"], got["rows"], got["n_series"]) == \
        (n, setting["mode"], every, sample_steps[-1], rows, T)
    assert got["counts"].dtype == np.int64 and got["counts"].shape == want["counts"].shape
    assert np.array_equal(got["counts"], want["counts"]), (got["counts"].tolist(), want["counts"].tolist())
    assert got["series"].dtype == np.int64 and got["series"].shape == (rows,) + want["series"].shape[1:]
    assert np.array_equal(got["series"], want["series"][n - rows:]), (got["series"].tolist(), want["series"][n - rows:].tolist())
    assert np.array_equal(got["steps"], np.asarray(sample_steps)[n - rows:])
    assert atoms["step"] == sample_steps[-1]
    assert atoms["structure"].dtype == np.int32 and atoms["r_local"].dtype == np.float64
    assert np.array_equal(atoms["structure"], want["structure"]), np.argwhere(atoms["structure"] != want["structure"])[:5]
    err = np.abs(atoms["r_local"] - want["r_local"]) / np.maximum(want["r_local"], 1.0)
    print("r_local: largest relative difference", err.max())
    assert np.all(err <= R_LOCAL_TOL) and np.array_equal(atoms["r_local"] == 0.0, want["r_local"] == 0.0)
    # every atom of every sample once
    assert np.array_equal(got["counts"].sum(axis=1), want["series"].sum(axis=0))


def _static(nn, frames, setting):
    """`md_run(0)` on the frames as they are, against the reference on the device's own state."""
    dev = _run(nn, frames, None, 0.3, [0], setting)
    want = _reference(nn, frames, dev["states"][:1], setting)
    _assert_cna(dev, want, setting, [0])
    return dev, want


def _ni(positions, cell, pbc=True):
    return Atoms(symbols=["Ni"] * len(positions), positions=positions, cell=cell, pbc=pbc)


def _bcc():
    return _ni(*ref.bcc_lattice(2.87, (4, 4, 4), 0.02))


# -- 1: structures with known answers -----------------------------------------------------------------------------
KNOWN = {
    "fcc": (lambda: fcc(rep=(3, 3, 3), jitter=0.02), None, [0, 108, 0, 0, 0]),
    "bcc": (_bcc, None, [0, 0, 0, 128, 0]),
    "hcp": (lambda: hcp(symbol="Ni", rep=(4, 4, 3), jitter=0.02), None, [0, 0, 96, 0, 0]),
    # not periodic: with the model's reach every shell atom sees the twelve others, with 4.5 A only eleven
    "ico": (lambda: _ni(*ref.icosahedron(2.5, 20.0), pbc=False), None, [12, 0, 0, 0, 1]),
    "ico-short": (lambda: _ni(*ref.icosahedron(2.5, 20.0), pbc=False), 4.5, [12, 0, 0, 0, 1]),
}


@pytest.mark.parametrize("case", list(KNOWN))
def test_known_structures(lib, case):
    build, r_max, counts = KNOWN[case]
    nn = _ni_setup()[0]
    dev, want = _static(nn, [build()], _setting(r_max=r_max))
    assert dev["cna"]["counts"].tolist() == [[counts]] and dev["cna"]["series"].tolist() == [[counts]]
    if case.startswith("ico"):
        assert dev["atoms"]["structure"].tolist() == [ref.ICO] + [ref.OTHER] * 12
        assert np.all((dev["atoms"]["r_local"][1:] == 0.0) == (r_max is not None))   # fewer than 12 candidates


def test_perfect_bcc_with_exact_ties(lib):
    """Lattice constant and sites are binary fractions: the eight first and the six second neighbours tie exactly among
    themselves, the 12th candidate with the 13th. Whichever twelve the tie-break selects are not FCC, HCP or ICO, and
    the fourteen are BCC (tests/test_md_cna_cpu.py shows that on the reference with two tie-breaks), so the types are
    compared exactly all the same; `gap_sel` is 0 by construction and is the one condition not asked for."""
    nn = _ni_setup()[0]
    atoms = _ni(*ref.bcc_lattice(2.875, (4, 4, 4), 0.0))
    setting = _setting()
    dev = _run(nn, [atoms], None, 0.3, [0], setting)
    want = ref.cna(dev["states"][:1], mode="adaptive", r_max=R_MODEL, **_describe(nn, [atoms]))
    assert want["gap_sel"] == 0.0 and want["gap_r"] >= EDGE and want["gap_bond"] >= EDGE
    _assert_cna(dev, _freeze(want), setting, [0])
    assert dev["cna"]["counts"].tolist() == [[[0, 0, 0, 128, 0]]]
    assert np.allclose(dev["atoms"]["r_local"], ref.SCALE * 2.875, rtol=1e-14)


# -- 2: a stacking fault ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", [_setting(), _setting("fixed", r_cut=3.0)], ids=["adaptive", "fixed"])
def test_two_hcp_layers_in_an_fcc_stack(lib, setting):
    nn = _ni_setup()[0]
    x, cell, layer = ref.close_packed_stack("ABCABCAB", 2.5, (4, 4), 0.02)
    dev, want = _static(nn, [_ni(x, cell)], setting)
    assert np.array_equal(dev["atoms"]["structure"], np.where((layer == 0) | (layer == 7), ref.HCP, ref.FCC))
    assert dev["cna"]["counts"].tolist() == [[[0, 96, 32, 0, 0]]]


# -- 3: batches -----------------------------------------------------------------------------------------------------
def test_frames_of_different_sizes(lib):
    """108, 128, 108 and 5 atoms: the offsets of the frames, chunks of 8 centres that end inside a frame, and a frame
    smaller than a chunk (not periodic: no atom of it has twelve candidates)."""
    nn, half, ordered = _half_ordered()
    small = _ni(10.0 + 2.5 * np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0.9, 0.8, 0.7]]), np.eye(3) * 20.0, False)
    frames = [fcc(rep=(3, 3, 3), jitter=0.02), _bcc(), half, small]
    dev, want = _static(nn, frames, _setting())
    counts = dev["cna"]["counts"][:, 0]
    assert counts[0].tolist() == [0, 108, 0, 0, 0] and counts[1].tolist() == [0, 0, 0, 128, 0] and counts[3].tolist() == [5, 0, 0, 0, 0]
    assert counts[2].tolist() == [92, 16, 0, 0, 0]   # (the ordered half less its two interfaces)
    assert np.all(dev["atoms"]["r_local"][-5:] == 0.0)


def test_two_elements(lib):
    nn, frames, v0 = _nimo()
    setting = _setting(n_series=4, sample_every=2)
    dev = _run(nn, frames, v0, 0.3, [2, 2], setting)
    xs, steps = _sampled(dev, 2)
    assert np.array_equal(steps, [0, 2, 4])
    want = _reference(nn, frames, xs, setting)
    _assert_cna(dev, want, setting, [0, 2, 4])
    mo, ni = list(nn.elements).index("Mo"), list(nn.elements).index("Ni")
    counts = dev["cna"]["counts"]
    assert counts[0, mo].sum() > 0 and counts[0, ni].sum() > 0 and counts[1, mo].sum() == 0 and counts[1, ni].sum() == 3 * 32
    assert np.array_equal(counts.sum(axis=1), dev["cna"]["series"].sum(axis=0))


# -- 4: the reach of the adaptive mode ----------------------------------------------------------------------------
def test_reach_edges(lib):
    """3.0 A leaves the twelve first neighbours of the jittered lattice and nothing for a second attempt; 2.3 A leaves
    nothing; in the half-ordered frame 3.0 A leaves 5 to 16 candidates, on both sides of 12 and of 14."""
    nn, half, ordered = _half_ordered()
    atoms = fcc(rep=(3, 3, 3), jitter=0.02)
    dev, want = _static(nn, [atoms], _setting(r_max=3.0))
    assert dev["cna"]["counts"].tolist() == [[[0, 108, 0, 0, 0]]] and np.all(dev["atoms"]["r_local"] > 2.9)
    dev, want = _static(nn, [atoms], _setting(r_max=2.3))
    assert dev["cna"]["counts"].tolist() == [[[108, 0, 0, 0, 0]]] and np.all(dev["atoms"]["r_local"] == 0.0)
    dev, want = _static(nn, [half], _setting(r_max=3.0))
    n_cand = np.array([len(dist) for _, dist in ref.candidates(dev["states"][0], half.get_cell(complete=True), [True] * 3, 3.0)[0]])
    assert n_cand.min() < 12 and (n_cand == 12).any() and (n_cand == 13).any() and n_cand.max() >= 14
    assert np.array_equal(dev["atoms"]["r_local"] == 0.0, n_cand < 12)
    # the model's reach: 78 neighbours of the lattice and the skin's, more than one round of 64 entries
    dev, want = _static(nn, [half], _setting())
    assert min(len(dist) for _, dist in ref.candidates(dev["states"][0], half.get_cell(complete=True), [True] * 3, R_MODEL)[0]) > 64


# -- 5: the fixed mode ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build, r_cut, counts", [
    (lambda: fcc(rep=(3, 3, 3), jitter=0.02), 3.0, [0, 108, 0, 0, 0]),   # 12 neighbours
    (_bcc, 3.4, [0, 0, 0, 128, 0]),                                     # 8 + 6 below the third shell at 4.06 A
    (lambda: fcc(rep=(3, 3, 3), jitter=0.02), 4.5, [108, 0, 0, 0, 0]),   # 12 + 6 + 24
    (_bcc, 2.7, [128, 0, 0, 0, 0]),                                     # 8
], ids=["fcc-12", "bcc-14", "fcc-42", "bcc-8"])
def test_fixed_mode(lib, build, r_cut, counts):
    nn = _ni_setup()[0]
    dev, want = _static(nn, [build()], _setting("fixed", r_cut=r_cut))
    assert dev["cna"]["counts"].tolist() == [[counts]] and np.all(dev["atoms"]["r_local"] == r_cut)


def test_fixed_mode_on_the_half_ordered_frame(lib):
    nn, half, ordered = _half_ordered()
    dev, want = _static(nn, [half], _setting("fixed", r_cut=3.0))
    assert 0 < dev["cna"]["counts"][0, 0, ref.FCC] < 108


# -- 6: dynamics ----------------------------------------------------------------------------------------------------
# The half-ordered frame at 2000 K: the forces of the disordered half move atoms by more than half a skin of 0.1 A inside
# twelve steps.
ORDER = ((4, 6), 3.0, 16, 1, (6, 0.5))
CLUSTER = dict(r_link=3.0, n_min=8, species=None, n_bins=32, n_series=16, sample_every=1)


@functools.lru_cache(maxsize=None)
def _dynamics_run(skin, runs, every=1, n_series=16, integrator="nve", others=False, on=True, lags=16):
    nn, half, ordered = _half_ordered()
    setting = _setting(n_series=n_series, sample_every=every)
    return _run(nn, [half], _velocities([half], 2000.0, 3), skin, list(runs), setting if on else None,
                ORDER if others else None, CLUSTER if others else None, integrator=integrator, lags=lags)


@functools.lru_cache(maxsize=None)
def _dynamics_reference():
    nn, half, ordered = _half_ordered()
    dev = _dynamics_run(0.1, (12,))
    assert np.array_equal(dev["samples"]["steps"], np.arange(13))
    return _reference(nn, [half], dev["samples"]["x"], _setting(n_series=16))


def test_dynamics_with_rebuilds_inside_the_window(lib):
    dev = _dynamics_run(0.1, (12,))
    assert dev["n_rebuilds"] > 0
    want = _dynamics_reference()
    assert len({tuple(r) for r in want["series"][:, 0].tolist()}) > 1   # (the rows change along the run)
    _assert_cna(dev, want, _setting(n_series=16), list(range(13)))   # 13 samples: nothing twice or skipped around a redone step
    # a cut run equals the uncut run: the integers exactly, r_local bit for bit
    cut = _dynamics_run(0.1, (5, 7))
    assert np.array_equal(cut["x"], dev["x"]) and np.array_equal(cut["v"], dev["v"])
    for key in ("counts", "series", "steps"):
        assert np.array_equal(cut["cna"][key], dev["cna"][key]), key
    assert np.array_equal(cut["atoms"]["structure"], dev["atoms"]["structure"])
    assert np.array_equal(cut["atoms"]["r_local"], dev["atoms"]["r_local"])
    assert cut["cna"]["n_samples"] == 13 and cut["atoms"]["step"] == 12
    # with the feature on, the trajectory and the records are bitwise those of a run without it
    off = _dynamics_run(0.1, (12,), on=False)
    assert "cna" not in off and off["n_rebuilds"] == dev["n_rebuilds"]
    for k in ("x", "v", "epot", "ekin", "states"):
        assert np.array_equal(dev[k], off[k]), k


@pytest.mark.parametrize("every, n_series", [(2, 4), (3, 2), (3, 5)])
def test_the_series_keeps_the_newest_rows(lib, every, n_series):
    """Samples 0, s, 2 s .. of the same trajectory: their rows are those of the run that sampled every step."""
    full, want = _dynamics_run(0.1, (12,)), _dynamics_reference()
    dev = _dynamics_run(0.1, (5, 7), every, n_series)
    assert np.array_equal(dev["x"], full["x"])
    sample_steps = list(range(0, 13, every))
    rows = min(len(sample_steps), n_series)
    got = dev["cna"]
    assert (got["n_samples"], got["sample_every"], got["last_step"], got["rows"], got["n_series"]) == \
        (len(sample_steps), every, sample_steps[-1], rows, n_series)
    assert np.array_equal(got["steps"], sample_steps[-rows:])
    assert np.array_equal(got["series"], want["series"][sample_steps[-rows:]])
    assert np.array_equal(got["counts"].sum(axis=1), want["series"][sample_steps].sum(axis=0))
    assert dev["atoms"]["step"] == 12 and np.array_equal(dev["atoms"]["structure"], full["atoms"]["structure"])
    assert np.array_equal(dev["atoms"]["r_local"], full["atoms"]["r_local"])


def test_a_large_skin_gives_the_same_integers(lib):
    """Another skin orders the list differently and rebuilds it elsewhere; the trajectory then agrees to rounding
    only. The selection does not depend on the order of the list."""
    dev, calm = _dynamics_run(0.1, (12,)), _dynamics_run(1.0, (12,))
    assert dev["n_rebuilds"] > calm["n_rebuilds"]
    assert np.abs(dev["x"] - calm["x"]).max() < 1e-10
    for key in ("counts", "series", "steps"):   # (no gap of the reference below 1e-9: the same integers)
        assert np.array_equal(calm["cna"][key], dev["cna"][key]), key
    assert np.array_equal(calm["atoms"]["structure"], dev["atoms"]["structure"])
    assert np.allclose(calm["atoms"]["r_local"], dev["atoms"]["r_local"], rtol=1e-9, atol=0.0)


def test_under_the_chain_thermostat(lib):
    nn, half, ordered = _half_ordered()
    dev = _dynamics_run(0.1, (12,), 4, 8, "nhc")
    want = _reference(nn, [half], dev["samples"]["x"][::4], _setting(n_series=8, sample_every=4))
    _assert_cna(dev, want, _setting(n_series=8, sample_every=4), [0, 4, 8, 12])


def test_under_the_barostat_with_the_cells_of_the_sampled_state(lib):
    """P0 = 0, taup = 20 fs: the cell changes from the first step on. The run cut at every sampled step hands out
    positions and cells of those states; one uncut run gives the same integers."""
    nn, half, ordered = _half_ordered()
    v0 = _velocities([half], 2000.0, 3)
    baro = (0.0, 20 * DT, 0.9)
    setting = _setting(n_series=4, sample_every=3)
    cut = _run(nn, [half], v0, 0.1, [3, 3, 2], setting, integrator="berendsen", barostat=baro)
    uncut = _run(nn, [half], v0, 0.1, [8], setting, integrator="berendsen", barostat=baro)
    xs, steps = _sampled(cut, 3)
    cells = cut["cells"][np.isin(cut["steps"], steps)]
    assert np.array_equal(steps, [0, 3, 6]) and cells.shape == (3, 1, 3, 3)
    assert len({abs(np.linalg.det(c[0])) for c in cells}) == 3
    want = _reference(nn, [half], xs, setting, cells=cells)
    for dev in (cut, uncut):
        _assert_cna(dev, want, setting, [0, 3, 6])
    assert np.array_equal(cut["atoms"]["r_local"], uncut["atoms"]["r_local"])


# -- 7: beside the other observables ------------------------------------------------------------------------------
def test_beside_the_order_parameters_and_the_clusters(lib):
    """All three in one run: the analysis gives what it gives alone, the order parameters and the clusters (n_min = 8,
    which reads the order launches' n_conn) what they give without it."""
    alone = _dynamics_run(0.1, (12,))
    both = _dynamics_run(0.1, (12,), others=True, on=False)
    three = _dynamics_run(0.1, (12,), others=True)
    assert np.array_equal(three["x"], alone["x"]) and three["n_rebuilds"] == alone["n_rebuilds"] > 0
    for key in ("counts", "series", "steps", "n_samples", "last_step"):
        assert np.array_equal(three["cna"][key], alone["cna"][key]), key
    for key in ("structure", "r_local"):
        assert np.array_equal(three["atoms"][key], alone["atoms"][key]), key
    for part in ("order", "order_atoms", "clusters", "cluster_atoms"):
        assert set(three[part]) == set(both[part])
        for key, value in both[part].items():
            assert np.array_equal(three[part][key], value), (part, key)
    assert both["clusters"]["n_samples"] == 13 and both["clusters"]["series"][:, 0, 0].max() > 0


# -- 8: life cycle and errors ---------------------------------------------------------------------------------------
def test_life_cycle_and_argument_errors(lib):
    from tensoralloy_amd import Engine
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 300.0, 3)
    with Engine(nn) as eng:
        with pytest.raises(ValueError, match="no resident batch"):
            eng.md_cna()
        with pytest.raises(ValueError, match="no resident batch"):
            eng.md_cna_atoms()
        eng.md_set_cna(n_series=0)   # off is always allowed
        with pytest.raises(ValueError, match="ta_md_set_cna: no resident batch"):
            eng.md_set_cna()
        eng.set_frames([atoms])
        with pytest.raises(ValueError, match="ta_md_get_cna called before ta_md_init"):
            eng.md_cna()
        with pytest.raises(ValueError, match="ta_md_get_cna_atoms called before ta_md_init"):
            eng.md_cna_atoms()
        with pytest.raises(ValueError, match="ta_md_set_cna called before ta_md_init"):
            eng.md_set_cna()
        eng.md_init(None, v0)
        with pytest.raises(ValueError, match=r"ta_md_get_cna: the common neighbour analysis is off \(ta_md_set_cna\)"):
            eng.md_cna()
        with pytest.raises(ValueError, match=r"ta_md_get_cna_atoms: the common neighbour analysis is off"):
            eng.md_cna_atoms()
        eng.md_set_cna("fixed", r_cut=3.0, n_series=3, sample_every=2)
        eng.md_run(2, DT)
        before = eng.md_cna()
        assert (before["n_samples"], before["mode"], before["sample_every"], before["last_step"]) == (2, "fixed", 2, 2)
        # an invalid argument is named and leaves setting and data as they were
        nan, inf = float("nan"), float("inf")
        for kw, what in [
            (dict(mode=2), r"mode = 2 must be TA_MD_CNA_ADAPTIVE \(0\) or TA_MD_CNA_FIXED \(1\)"),
            (dict(mode=-1), "mode = -1 must be"),
            (dict(n_series=-1), "n_series must be 0 .. 1048576"),
            (dict(n_series=1048577), "n_series must be 0 .. 1048576"),
            (dict(sample_every=0), "sample_every must be >= 1"),
            (dict(mode="fixed", r_cut=nan), "r_cut must be a finite distance > 0"),
            (dict(mode="fixed", r_cut=inf), "r_cut must be a finite distance > 0"),
            (dict(mode="fixed", r_cut=0.0), "r_cut must be a finite distance > 0"),
            (dict(mode="fixed", r_cut=-3.0), "r_cut must be a finite distance > 0"),
            (dict(mode="fixed", r_cut=6.01), r"r_cut = 6.01\d* exceeds the model's cutoff max\(rcut, acut\) = 6.0"),
            (dict(r_max=inf), "r_max must be a finite distance > 0"),
            (dict(r_max=0.0), "r_max must be a finite distance > 0"),
            (dict(r_max=-1.0), "r_max must be a finite distance > 0"),
            (dict(r_max=6.01), r"r_max = 6.01\d* exceeds the model's cutoff"),
        ]:
            with pytest.raises(ValueError, match="ta_md_set_cna: " + what):
                eng.md_set_cna(**kw)
            after = eng.md_cna()
            assert all(np.array_equal(after[k], before[k]) for k in before), kw
        with pytest.raises(ValueError, match="md_set_cna: mode must be 'adaptive' or 'fixed'"):
            eng.md_set_cna("interval")
        with pytest.raises(ValueError, match="md_set_cna: the fixed mode needs r_cut"):
            eng.md_set_cna("fixed")
        # the other mode's distance is ignored
        eng.md_set_cna("adaptive", r_cut=nan, r_max=None, n_series=2)
        out = eng.md_cna()
        assert (out["n_samples"], out["mode"], out["last_step"], out["rows"], out["n_series"]) == (0, "adaptive", -1, 0, 2)
        assert not out["counts"].any() and out["series"].shape == (0, 1, 5) and out["steps"].shape == (0,)
        with pytest.raises(ValueError, match="ta_md_get_cna_atoms: no sample has been taken yet"):
            eng.md_cna_atoms()
        res = eng.md_run(0, DT)   # the resident state (step 2) once
        assert set(res) == {"epot", "ekin", "n_rebuilds"}   # the result dict is unchanged
        eng.md_run(0, DT)         # ... and not twice
        out = eng.md_cna()
        assert (out["n_samples"], out["last_step"], out["steps"].tolist()) == (1, 2, [2]) and out["counts"].sum() == 32
        assert eng.md_cna_atoms()["step"] == 2
        # off and on again
        eng.md_set_cna(n_series=0)
        assert eng.md_cna_series == 0
        with pytest.raises(ValueError, match="common neighbour analysis is off"):
            eng.md_cna()
        eng.md_run(1, DT)
        eng.md_set_cna(n_series=2, sample_every=2)
        eng.md_run(3, DT)   # steps 3 .. 6: the samples are those of the steps 4 and 6
        out = eng.md_cna()
        assert (out["n_samples"], out["last_step"], out["steps"].tolist()) == (2, 6, [4, 6])
        # set_frames keeps the setting and drops the data; md_init starts from zero
        eng.set_frames([atoms, atoms])
        with pytest.raises(ValueError, match="ta_md_get_cna called before ta_md_init"):
            eng.md_cna()
        eng.md_init(None, np.tile(v0, (2, 1)))
        out = eng.md_cna()
        assert (out["n_samples"], out["sample_every"], out["n_series"], out["last_step"]) == (0, 2, 2, -1)
        assert out["counts"].shape == (2, 1, 5) and not out["counts"].any()
        eng.md_run(2, DT)
        out = eng.md_cna()
        assert out["n_samples"] == 2 and out["counts"].sum(axis=(1, 2)).tolist() == [64, 64]
        assert np.array_equal(out["series"][:, 0], out["series"][:, 1])   # the two frames are the same
        # the barostat does not exclude this feature, nor do the other observables
        eng.md_set_barostat(0.0, 100 * DT, 1.0)
        eng.md_set_adf(16, 3.0, 1)
        eng.md_run(2, DT)
        assert (eng.md_cna()["n_samples"], eng.md_cna()["last_step"]) == (3, 4)
        eng.md_init(None, np.tile(v0, (2, 1)))
        assert eng.md_cna()["n_samples"] == 0 and not eng.md_cna()["counts"].any()


def test_getters_after_a_failed_run(lib):
    """A run that fails leaves the data invalid until `md_set_cna` or `md_init` is called again. The failure:
    n_steps = 2^31 - 1 with a record of 128 frames at every step asks for 2.5 TB of `epot` records. `ta_md_run`
    allocates them first, inside its guarded body and behind the point where it marks the data invalid; the
    allocation is refused and nothing is launched: positions and velocities are untouched. (Called through the C
    ABI with null record pointers, so that the host allocates nothing either.)"""
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

    refusal = r"ta_md_get_cna%s: a ta_md_run failed and left the data invalid; call ta_md_set_cna or ta_md_init again"
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        eng.set_frames(frames)
        eng.md_init(None, v0)
        eng.md_set_cna(n_series=4)
        eng.md_run(2, DT)
        assert eng.md_cna()["n_samples"] == 3
        failing_run(eng)
        with pytest.raises(ValueError, match=refusal % ""):
            eng.md_cna()
        with pytest.raises(ValueError, match=refusal % "_atoms"):
            eng.md_cna_atoms()
        eng.md_run(1, DT)   # the loop goes on (step 3) and counts nothing; the getters still refuse
        with pytest.raises(ValueError, match=refusal % ""):
            eng.md_cna()
        eng.md_set_cna(n_series=4)   # set again: zero counts, sample 0 is the state of step 3
        out = eng.md_cna()
        assert (out["n_samples"], out["last_step"]) == (0, -1) and not out["counts"].any()
        eng.md_run(2, DT)
        out = eng.md_cna()
        assert (out["n_samples"], out["last_step"], out["steps"].tolist()) == (3, 5, [3, 4, 5])
        assert out["counts"][0].sum() == out["counts"][127].sum() == 3 * 32 and eng.md_cna_atoms()["step"] == 5
        failing_run(eng)
        with pytest.raises(ValueError, match=refusal % ""):
            eng.md_cna()
        eng.md_init(None, v0)   # ... or md_init: the setting is kept, the counts start from zero
        out = eng.md_cna()
        assert (out["n_samples"], out["n_series"], out["last_step"]) == (0, 4, -1) and not out["counts"].any()
        eng.md_run(1, DT)
        assert eng.md_cna()["n_samples"] == 2


# -- DeviceMD ---------------------------------------------------------------------------------------------------------
def test_device_md_end_to_end(lib):
    from tensoralloy_amd import Engine
    nn, half, ordered = _half_ordered()
    atoms = half.copy()
    v0 = _velocities([atoms], 2000.0, 3)
    setting = _setting(n_series=8, sample_every=3)
    with Engine(nn) as eng:
        dyn = md.DeviceMD(eng, atoms, DT, velocities=v0, cna="adaptive", cna_series=8, cna_every=3, n_lags=16, sample_every=1)
        dyn.run(6)
        dyn.run(5)
        samples = eng.md_samples()
        assert np.array_equal(samples["steps"], np.arange(12))
        want = _reference(nn, [atoms], samples["x"][0:10:3], setting)
        out = dyn.get_structure_counts()
        assert (out["n_samples"], out["mode"], out["sample_every"], out["last_step"], out["rows"]) == (4, "adaptive", 3, 9, 4)
        assert np.array_equal(out["series"], want["series"]) and out["steps"].tolist() == [0, 3, 6, 9]
        assert np.array_equal(out["counts"], want["counts"])
        types = dyn.get_structure_types()
        assert types["step"] == 9 and np.array_equal(types["structure"], want["structure"])
        frac = md.structure_fractions(out["series"])
        assert frac.shape == (4, 1, 5) and np.allclose(frac.sum(axis=-1), 1.0)
        fixed = md.DeviceMD(eng, atoms, DT, velocities=v0, cna="fixed", cna_rcut=3.0)
        fixed.run(0)
        assert fixed.get_structure_counts()["mode"] == "fixed" and np.all(fixed.get_structure_types()["r_local"] == 3.0)
        plain = md.DeviceMD(eng, atoms, DT, velocities=v0)   # cna None: the feature is set off
        assert eng.md_cna_series == 0
        with pytest.raises(ValueError, match=r"common neighbour analysis is off \(cna\)"):
            plain.get_structure_counts()
        with pytest.raises(ValueError, match=r"common neighbour analysis is off \(cna\)"):
            plain.get_structure_types()
        with pytest.raises(ValueError, match=r"common neighbour analysis is off \(ta_md_set_cna\)"):
            eng.md_cna()
    for kw, what in [(dict(cna="interval"), "cna must be 'adaptive' or 'fixed'"), (dict(cna="fixed"), "cna = 'fixed' needs cna_rcut"),
                     (dict(cna="adaptive", cna_rcut=3.0), "cna_rcut belongs to cna = 'fixed'"),
                     (dict(cna="fixed", cna_rcut=3.0, cna_rmax=4.0), "cna_rmax belongs to cna = 'adaptive'"),
                     (dict(cna="adaptive", cna_every=0), "cna_every must be an integer >= 1"),
                     (dict(cna="adaptive", cna_series=0), "cna_series must be an integer 1 .. 1048576"),
                     (dict(cna="adaptive", cna_rmax=-1.0), "cna_rmax must be a finite distance > 0"),
                     (dict(cna_every=2), ".* belong to the common neighbour analysis")]:
        with pytest.raises(ValueError, match="DeviceMD: " + what):
            md.DeviceMD(None, atoms, DT, **kw)
