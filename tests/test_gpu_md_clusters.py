"""GPU: clusters of solid or selected atoms inside the device MD loop (`ta_md_set_clusters`, csrc/ta_md_cluster.hip)
against the brute-force definition (tests/md_cluster_reference.py), which sweeps all atoms and all periodic images, has
a union-find of its own and shares nothing with the library's neighbour list.

Every quantity is an integer and every comparison is EXACT. That needs no pair on a link cutoff and, with n_min > 0,
no bond on the solid threshold: every exact test first asserts, on the reference alone, that no r / rl lies within
1e-9 of 1 and, with n_min > 0, the conditions of tests/test_gpu_md_order.py on the order reference (no s_ij within 1e-8
of c, no |q_solid| of an atom with neighbours below 1e-3). The snapshots are the device's own whole-step states:
`md_state()` between the calls of a cut run, or the position ring of `md_set_sampling`.

The run that fails (for the getters behind it) fails on the host, as in tests/test_gpu_md_order.py: its record
buffers are 2.5 TB that no device has, and `ta_md_run` allocates them before it enqueues anything.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import md_cluster_reference as ref
from tests import md_order_reference as order_ref
from tests.helpers import fcc, make_eam
from tests.test_gpu_md import DT, WANT, _ni_setup, _velocities
from tests.test_gpu_md_rdf import SETUPS, _describe, _freeze, _nimo, _sampled, _sheared
from tensoralloy_amd import Atoms, md

pytestmark = pytest.mark.gpu

EDGE_R, EDGE_S, MIN_NORM = 1e-9, 1e-8, 1e-3   # conditions on the reference, not tolerances
ORDER = ((4, 6), 3.0, 16, 1, (6, 0.5))        # md_set_order beside n_min > 0: degrees, r_bond, bins, every, solid


def _setting(r_link=3.0, n_min=0, species=None, n_bins=32, n_series=1, sample_every=1):
    return dict(r_link=r_link, n_min=n_min, species=species, n_bins=n_bins, n_series=n_series, sample_every=sample_every)


def _run(nn, frames, v0, skin, runs, cluster=None, order=None, integrator="nve", lags=None, dt=DT, barostat=None):
    """The runs `runs` (steps per md_run call) on the device: final state, records, the whole-step positions (and
    cells) at entry and behind every call (`states`, `cells`, at the absolute steps `steps`), and with `cluster` (the
    arguments of `md_set_clusters`; `order`: those of `md_set_order`, switched on first) what `md_clusters` and
    `md_cluster_atoms` return (`clusters`, `atoms`). `lags`: `md_set_sampling(lags, 1)` is on as well (`samples`)."""
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
        states, cells, steps, outs = [eng.md_state()[0]], [eng.md_cells()], [0], []
        for n in runs:
            outs.append(eng.md_run(n, dt))
            states.append(eng.md_state()[0])
            cells.append(eng.md_cells())
            steps.append(steps[-1] + n)
        x, v = eng.md_state()
        res = dict(x=x, v=v, n_rebuilds=sum(o["n_rebuilds"] for o in outs), states=np.array(states),
                   cells=np.array(cells), steps=np.array(steps))
        if cluster is not None:
            res["clusters"] = eng.md_clusters()
            res["atoms"] = eng.md_cluster_atoms()
        if order is not None:
            res["order_atoms"] = eng.md_order_atoms()
        if lags is not None:
            res["samples"] = eng.md_samples()
    for k in ("epot", "ekin", "echain"):
        if k in outs[0]:
            res[k] = np.concatenate([o[k][1 if j else 0:] for j, o in enumerate(outs)])
    return _freeze(res)


def _reference(nn, frames, snapshots, cluster, order=None, cells=None):
    """The reference on the snapshots (one per sample), after the conditions on the reference alone."""
    d = _describe(nn, frames)
    if cells is not None:
        d["cells"] = cells
    els, E = list(nn.elements), len(nn.elements)
    species = cluster["species"]
    mask = (1 << E) - 1 if species is None else sum(1 << (els.index(s) if isinstance(s, str) else int(s)) for s in species)
    n_conn = None
    if cluster["n_min"] > 0:
        degrees, r_bond, _, _, solid = order
        n_conn = []
        for n, x in enumerate(snapshots):
            dn = dict(d, cells=np.asarray(d["cells"]).reshape((-1, len(frames), 3, 3))[n if cells is not None else 0])
            o = order_ref.order_parameters(x[None], degrees=degrees, n_bins=8, r_bond=r_bond, solid=solid, **dn)
            assert o["gap_r"] >= EDGE_R and o["gap_s"] >= EDGE_S and o["min_norm"] >= MIN_NORM   # (on the reference alone)
            n_conn.append(o["n_conn"])
    out = ref.clusters(snapshots, r_link=cluster["r_link"], species_mask=mask, n_bins=cluster["n_bins"], n_min=cluster["n_min"],
                       n_conn=n_conn, **d)
    print("reference: nearest link cutoff", out["gap_r"], "rows", out["series"].reshape(len(snapshots), -1).tolist()[:13])
    assert out["gap_r"] >= EDGE_R, out["gap_r"]   # (on the reference alone)
    out["n_conn"] = None if n_conn is None else n_conn[-1]
    return _freeze(out)


def _assert_clusters(dev, want, cluster, sample_steps):
    """Histogram, series rows (the newest n_series, oldest first, with their steps), info and per-atom arrays."""
    got, atoms = dev["clusters"], dev["atoms"]
    n, T, every = len(sample_steps), cluster["n_series"], cluster["sample_every"]
    rows = min(n, T)
    assert (got["n_samples"], got["n_bins"], got["sample_every"], got["last_step"], got["rows"], got["n_series"]) == \
        (n, cluster["n_bins"], every, sample_steps[-1], rows, T)
    assert got["hist"].dtype == np.int64 and got["hist"].shape == want["hist"].shape
    assert np.array_equal(got["hist"], want["hist"]), (got["hist"].tolist(), want["hist"].tolist())
    assert got["series"].dtype == np.int64 and got["series"].shape == (rows,) + want["series"].shape[1:]
    assert np.array_equal(got["series"], want["series"][n - rows:]), (got["series"].tolist(), want["series"][n - rows:].tolist())
    assert np.array_equal(got["steps"], np.asarray(sample_steps)[n - rows:])
    assert atoms["step"] == sample_steps[-1]
    assert atoms["label"].dtype == np.int32 and atoms["size"].dtype == np.int32
    assert np.array_equal(atoms["label"], want["label"]), np.argwhere(atoms["label"] != want["label"])[:5]
    assert np.array_equal(atoms["size"], want["size"]), np.argwhere(atoms["size"] != want["size"])[:5]
    # every cluster of every sample once: sum_k hist = clusters; the atoms behind a root are its size
    assert np.array_equal(got["hist"].sum(axis=1), want["series"][:, :, 1].sum(axis=0))
    sizes, members = md.clusters_from_labels(atoms["label"])
    assert all(np.all(atoms["size"][m] == s) for s, m in zip(sizes, members))


def _sizes(label):
    return md.clusters_from_labels(label)[0].tolist()


# -- 1: the half-ordered frame ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _half_ordered():
    nn = _ni_setup()[0]
    atoms = fcc(rep=(3, 3, 3), jitter=0.0)
    x = np.asarray(atoms.positions).copy()
    ordered = x[:, 2] < 0.5 * np.asarray(atoms.get_cell(complete=True))[2, 2] - 0.1
    rng = np.random.RandomState(134)
    x += np.where(ordered[:, None], 0.02, 0.6) * rng.standard_normal(x.shape)
    return nn, Atoms(symbols=["Ni"] * 108, positions=x, cell=np.asarray(atoms.get_cell(complete=True)), pbc=True), ordered


@pytest.mark.parametrize("n_min, n_sel", [(8, 54), (12, 18), (0, 108)])
def test_half_ordered_frame(lib, n_min, n_sel):
    nn, frame, ordered = _half_ordered()
    setting = _setting(3.0, n_min, n_bins=128)
    dev = _run(nn, [frame], np.zeros((108, 3)), 0.3, [0], setting, ORDER if n_min else None)
    want = _reference(nn, [frame], dev["states"][:1], setting, ORDER)
    assert want["series"].tolist() == [[[n_sel, 1, n_sel, int(np.nonzero(want["label"] >= 0)[0][0])]]]   # one cluster
    _assert_clusters(dev, want, setting, [0])
    if n_min:
        assert np.array_equal(dev["order_atoms"]["n_conn"], want["n_conn"])
        assert np.array_equal(dev["atoms"]["label"] >= 0, md.classify_solid(dev["order_atoms"]["n_conn"], n_min))
    if n_min == 8:
        assert np.array_equal(dev["atoms"]["label"] >= 0, ordered)
    t, largest = md.largest_cluster(dev["clusters"]["series"], dev["clusters"]["steps"], DT)
    assert t.tolist() == [0.0] and largest.tolist() == [[n_sel]]


# -- 2: species selection without the order feature --------------------------------------------------------------
@pytest.mark.parametrize("seed, sizes", [(1, [17, 2, 1, 1]), (3, [5, 4, 2, 1])])
def test_species_selection_without_the_order_feature(lib, seed, sizes):
    nn = make_eam(["Mo", "Ni"], 6.0, potential="zjw04")
    base = fcc(rep=(3, 3, 3), jitter=0.05, seed=17)
    minority = np.random.RandomState(seed).rand(108) < 0.15
    frame = Atoms(symbols=["Mo" if m else "Ni" for m in minority], positions=base.positions,
                  cell=np.asarray(base.get_cell(complete=True)), pbc=True)
    for n_bins in (32, 4):   # 4: sizes 17 and 5 land in the overflow bin
        setting = _setting(3.0, 0, ("Mo",), n_bins)
        dev = _run(nn, [frame], np.zeros((108, 3)), 0.3, [0], setting)
        want = _reference(nn, [frame], dev["states"][:1], setting)
        assert want["gap_r"] > 0.09 and _sizes(want["label"]) == sizes
        _assert_clusters(dev, want, setting, [0])
        assert np.array_equal(dev["atoms"]["label"] >= 0, minority) and _sizes(dev["atoms"]["label"]) == sizes
        assert dev["clusters"]["hist"][0, min(sizes[0], n_bins) - 1] >= 1
        sz, mean = md.cluster_size_distribution(dev["clusters"]["hist"], 1)
        assert mean.sum() == len(sizes) and np.array_equal(sz, np.arange(1, n_bins + 1))
    by_index = _run(nn, [frame], np.zeros((108, 3)), 0.3, [0], _setting(3.0, 0, [list(nn.elements).index("Mo")], 4))
    assert np.array_equal(by_index["atoms"]["label"], dev["atoms"]["label"])   # symbols or indices


# -- 3: chains: long parent chains, contention, chunk boundaries ---------------------------------------------------
def _chain(n, cuts, seed):
    """n Ni atoms on a line along x, 2.5 A apart, indices permuted; the gaps in front of the positions `cuts` are
    3.5 A. The cell closes the line through the boundary with a gap of 2.5 A."""
    perm = np.random.RandomState(seed).permutation(n)
    pos = 2.5 * np.arange(n)
    for c in cuts:
        pos[c:] += 1.0
    x = np.zeros((n, 3))
    x[perm, 0] = pos
    x[:, 1:] = 6.0
    cell = np.diag([2.5 * n + 1.0 * len(cuts), 12.0, 12.0])
    return Atoms(symbols=["Ni"] * n, positions=x, cell=cell, pbc=True), perm


@pytest.mark.parametrize("n", [65, 257, 1000])
@pytest.mark.parametrize("closed", [True, False])
def test_chains(lib, n, closed):
    nn = _ni_setup()[0]
    cuts = [] if closed else sorted(np.random.RandomState(n).choice(np.arange(1, n), size=4, replace=False).tolist())
    frame, perm = _chain(n, cuts, seed=n + 1)
    setting = _setting(3.0, 0, None, 4096 if n == 1000 else 64)
    dev = _run(nn, [frame], np.zeros((n, 3)), 0.3, [0], setting)
    want = _reference(nn, [frame], dev["states"][:1], setting)
    if closed:
        known = [n]   # one percolating cluster: atoms, not images
    else:   # the pieces between the cuts; the last and the first meet through the boundary
        edges = [0] + cuts + [n]
        pieces = [edges[k + 1] - edges[k] for k in range(len(cuts) + 1)]
        known = sorted(pieces[1:-1] + [pieces[0] + pieces[-1]], reverse=True)
    assert _sizes(want["label"]) == known and want["gap_r"] > 0.16
    _assert_clusters(dev, want, setting, [0])
    assert _sizes(dev["atoms"]["label"]) == known
    if closed:
        assert np.array_equal(dev["atoms"]["label"], [0] * n) and dev["clusters"]["series"][0, 0].tolist() == [n, 1, n, 0]
    else:
        members = md.clusters_from_labels(dev["atoms"]["label"])[1]
        assert all(int(dev["atoms"]["label"][m[0]]) == int(m.min()) for m in members)   # the label is the smallest member
        assert sorted(perm[cuts[0]:cuts[1]].tolist()) in [sorted(m.tolist()) for m in members]   # a piece between two cuts


# -- 4: batch edges -------------------------------------------------------------------------------------------------
def test_frames_of_1_7_and_108_atoms_one_sheared(lib):
    """A single atom in a cubic cell of 2.5 A (its images lie below the link cutoff and link nothing: one cluster of
    1), 7 atoms (fewer than the 8 centres of a workgroup) and a sheared cell of 108. Labels are indices in the batch."""
    nn = _ni_setup()[0]
    one = Atoms(symbols=["Ni"], positions=[[0.3, 0.1, -0.2]], cell=np.diag([2.5] * 3), pbc=True)
    eight = fcc(rep=(2, 1, 1), jitter=0.05, seed=5)
    seven = Atoms(symbols=["Ni"] * 7, positions=eight.positions[:7], cell=np.asarray(eight.get_cell(complete=True)), pbc=True)
    frames = [one, seven, _sheared(fcc(rep=(3, 3, 3), jitter=0.05, seed=4))]
    v0 = _velocities(frames, 300.0, 11)
    v0[0] = 0.0
    for r_link in (3.0, 2.3):   # 2.3: below the nearest-neighbour distance 2.49, jitter and shear decide
        setting = _setting(r_link, 0, None, 16, 2, 4)
        dev = _run(nn, frames, v0, 0.3, [4, 4], setting)
        xs, steps = _sampled(dev, 4)
        assert np.array_equal(steps, [0, 4, 8])
        want = _reference(nn, frames, xs, setting)
        _assert_clusters(dev, want, setting, [0, 4, 8])
        got = dev["atoms"]
        assert got["label"][0] == 0 and got["size"][0] == 1 and dev["clusters"]["series"][-1, 0].tolist() == [1, 1, 1, 0]
        assert got["label"][1:8].min() == 1 and got["label"][8:].min() == 8   # batch-global indices
        assert dev["clusters"]["hist"][0].tolist() == [3] + [0] * 15
    assert len(_sizes(got["label"])) > 20   # (2.3 A splits the frames into many clusters: 36 in the state at entry)


def test_a_frame_with_nothing_selected(lib):
    """Frame 1 of the Ni-Mo batch holds no Mo: its row is {0, 0, 0, -1}, its labels -1 and its sizes 0."""
    nn, frames, v0 = _nimo()
    setting = _setting(3.0, 0, ("Mo",), 8)
    dev = _run(nn, frames, v0, 0.3, [0], setting)
    want = _reference(nn, frames, dev["states"][:1], setting)
    _assert_clusters(dev, want, setting, [0])
    assert dev["clusters"]["series"][0, 1].tolist() == [0, 0, 0, -1] and not dev["clusters"]["hist"][1].any()
    assert np.all(dev["atoms"]["label"][32:] == -1) and not dev["atoms"]["size"][32:].any()
    assert dev["clusters"]["series"][0, 0, 0] == 16


def test_several_images_of_one_neighbour_in_a_cell_below_the_cutoff(lib):
    """32 Ni atoms in a cubic cell of 6.4 A under a model with a cutoff of 6.5 A, links up to the cutoff (r_link None):
    some 140 entries per centre (three rounds of 64 per wave), among them the centre's own images and several images
    of every other atom. One cluster of 32 atoms. With 2.2 A, under the nearest-neighbour distance 2.26 A, the jitter
    decides."""
    nn = make_eam(["Ni"], 6.5, potential="zjw04")
    atoms = fcc(a=3.2, rep=(2, 2, 2), jitter=0.05, seed=9)
    for r_link in (None, 2.2):
        setting = _setting(r_link, 0, None, 40, 3, 2)
        dev = _run(nn, [atoms], _velocities([atoms], 300.0, 3), 0.3, [2, 2], setting)
        xs, steps = _sampled(dev, 2)
        assert np.array_equal(steps, [0, 2, 4])
        want = _reference(nn, [atoms], xs, dict(setting, r_link=6.5 if r_link is None else r_link))
        assert np.array_equal(dev["clusters"]["r_link"], [[6.5 if r_link is None else r_link]])   # None: the model's cutoff
        _assert_clusters(dev, want, setting, [0, 2, 4])
        if r_link is None:
            assert dev["clusters"]["series"][:, 0].tolist() == [[32, 1, 32, 0]] * 3 and dev["clusters"]["hist"][0, 31] == 3


# -- 5: dynamics ----------------------------------------------------------------------------------------------------
# Dynamics at 2000 K from a lattice jittered by 0.02 A: links below the nearest-neighbour distance 2.49 A, so that they
# come and go; and solid atoms by a threshold of 0.993, which the first 12 fs of thermal motion take atoms across (on
# the CPU reference: jitters of 0.04 to 0.07 A leave 4 to 30 of the 32 atoms below 9 such bonds)
DYNAMICS = {
    "links": (_setting(2.45, 0, None, 32, 16), None),
    "solid": (_setting(3.0, 9, None, 32, 16), ((4, 6), 3.0, 16, 1, (6, 0.993))),
}


@functools.lru_cache(maxsize=None)
def _dynamics_run(case, skin, runs, on=True):
    nn, atoms = _ni_setup()
    setting, order = DYNAMICS[case]
    return _run(nn, [atoms], _velocities([atoms], 2000.0, 3), skin, list(runs), setting if on else None,
                order if on else None, lags=16)


@pytest.mark.parametrize("case", list(DYNAMICS))
def test_dynamics_with_rebuilds_inside_the_window(lib, case):
    nn, atoms = _ni_setup()
    setting, order = DYNAMICS[case]
    dev = _dynamics_run(case, 0.1, (12,))
    assert dev["n_rebuilds"] > 0 and np.array_equal(dev["samples"]["steps"], np.arange(13))
    want = _reference(nn, [atoms], dev["samples"]["x"], setting, order)
    assert len({tuple(r) for r in want["series"][:, 0, :3].tolist()}) > 1   # (the rows change along the run)
    _assert_clusters(dev, want, setting, list(range(13)))   # 13 samples: nothing twice or skipped around a redone step
    # a cut run equals the uncut run exactly
    cut = _dynamics_run(case, 0.1, (5, 0, 1, 4, 2))
    assert np.array_equal(cut["x"], dev["x"]) and np.array_equal(cut["v"], dev["v"])
    for key in ("hist", "series", "steps"):
        assert np.array_equal(cut["clusters"][key], dev["clusters"][key]), key
    for key in ("label", "size"):
        assert np.array_equal(cut["atoms"][key], dev["atoms"][key]), key
    assert cut["clusters"]["n_samples"] == 13 and cut["atoms"]["step"] == 12
    # with the feature on, the trajectory and the records are bitwise those of a run without it
    off = _dynamics_run(case, 0.1, (12,), False)
    assert "clusters" not in off and off["n_rebuilds"] == dev["n_rebuilds"]
    for k in ("x", "v", "epot", "ekin", "states"):
        assert np.array_equal(dev[k], off[k]), k
    assert np.array_equal(dev["samples"]["x"], off["samples"]["x"])


@pytest.mark.parametrize("case", list(DYNAMICS))
def test_a_large_skin_gives_the_same_integers(lib, case):
    """Another skin orders the list differently and rebuilds it elsewhere; the trajectory then agrees to rounding
    only, so the reference runs on this run's own states."""
    nn, atoms = _ni_setup()
    setting, order = DYNAMICS[case]
    calm = _dynamics_run(case, 0.6, (12,))
    assert calm["n_rebuilds"] == 0
    want = _reference(nn, [atoms], calm["samples"]["x"], setting, order)
    _assert_clusters(calm, want, setting, list(range(13)))
    dev = _dynamics_run(case, 0.1, (12,))
    assert np.abs(dev["x"] - calm["x"]).max() < 1e-9
    for key in ("hist", "series"):   # (no pair within 1e-9 of a cutoff: the same integers)
        assert np.array_equal(calm["clusters"][key], dev["clusters"][key]), key
    assert np.array_equal(calm["atoms"]["label"], dev["atoms"]["label"])


@pytest.mark.parametrize("integrator", ["nve", "berendsen", "langevin", "nhc"])
def test_every_thermostat(lib, integrator):
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 2000.0, 3)
    setting = _setting(2.45, 0, None, 32, 8, 4)
    plain = _run(nn, [atoms], v0, 0.1, [4, 4, 3], None, integrator=integrator)
    dev = _run(nn, [atoms], v0, 0.1, [4, 4, 3], setting, integrator=integrator)
    assert dev["n_rebuilds"] == plain["n_rebuilds"] >= 1
    for k in ("x", "v", "epot", "ekin", "states") + (("echain",) if integrator == "nhc" else ()):
        assert np.array_equal(dev[k], plain[k]), k   # bit for bit: the launches only read the state
    xs, steps = _sampled(dev, 4)
    assert np.array_equal(steps, [0, 4, 8])
    want = _reference(nn, [atoms], xs, setting)
    _assert_clusters(dev, want, setting, [0, 4, 8])


def test_under_the_barostat_with_the_cells_of_the_sampled_state(lib):
    """Cell and atoms scaled by 1.02, P0 = 0, taup = 20 fs: the cell shrinks from the first step on. Links below 2.5 A,
    next to the nearest-neighbour distance 2.54 A of the scaled lattice, some of them through the boundary. The run
    cut at every sampled step hands out positions and cells of those states; one uncut run gives the same integers."""
    nn, atoms = _ni_setup()
    big = Atoms(symbols=atoms.get_chemical_symbols(), positions=atoms.positions * 1.02,
                cell=np.asarray(atoms.get_cell(complete=True)) * 1.02, pbc=True)
    v0 = _velocities([big], 600.0, 3)
    baro = (0.0, 20 * DT, 0.9)
    setting = _setting(2.5, 0, None, 32, 4, 3)
    cut = _run(nn, [big], v0, 0.3, [3, 3, 2], setting, integrator="berendsen", barostat=baro)
    uncut = _run(nn, [big], v0, 0.3, [8], setting, integrator="berendsen", barostat=baro)
    xs, steps = _sampled(cut, 3)
    cells = cut["cells"][np.isin(cut["steps"], steps)]
    assert np.array_equal(steps, [0, 3, 6]) and cells.shape == (3, 1, 3, 3)
    assert abs(np.linalg.det(cells[2, 0])) < abs(np.linalg.det(cells[1, 0])) < abs(np.linalg.det(cells[0, 0]))
    want = _reference(nn, [big], xs, setting, cells=cells)
    for dev in (cut, uncut):
        _assert_clusters(dev, want, setting, [0, 3, 6])


# -- 6: the series ---------------------------------------------------------------------------------------------------
def test_the_series_keeps_the_newest_rows_in_order(lib):
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 2000.0, 3)
    setting = _setting(2.45, 0, None, 32, 4, 1)
    dev = _run(nn, [atoms], v0, 0.3, [2, 4], setting, lags=8)
    want = _reference(nn, [atoms], dev["samples"]["x"], setting)
    _assert_clusters(dev, want, setting, list(range(7)))   # 7 samples, rows of the steps 3, 4, 5, 6
    assert dev["clusters"]["steps"].tolist() == [3, 4, 5, 6] and dev["clusters"]["series"].shape == (4, 1, 4)
    t, largest = md.largest_cluster(dev["clusters"]["series"], dev["clusters"]["steps"], DT)
    assert np.array_equal(t, DT * np.arange(3, 7)) and np.array_equal(largest[:, 0], want["series"][3:, 0, 2])


def test_every_fourth_step_under_an_order_feature_of_every_second(lib):
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 2000.0, 3)
    setting, order = _setting(3.0, 9, None, 32, 8, 4), ((4, 6), 3.0, 16, 2, (6, 0.993))
    dev = _run(nn, [atoms], v0, 0.3, [4, 4, 2], setting, order)
    xs, steps = _sampled(dev, 4)
    assert np.array_equal(steps, [0, 4, 8])
    want = _reference(nn, [atoms], xs, setting, order)
    _assert_clusters(dev, want, setting, [0, 4, 8])
    assert dev["order_atoms"]["step"] == 10   # (the order feature has moved on; the clusters are those of step 8)


# -- 7: refusals, life cycle, a failed run, DeviceMD ------------------------------------------------------------------
def test_md_run_refusals(lib):
    from tensoralloy_amd import Engine
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 300.0, 3)
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        eng.set_frames([atoms])
        eng.md_init(None, v0)
        eng.md_set_clusters(3.0, 8, None, 16)
        with pytest.raises(ValueError, match=r"ta_md_run: the cluster analysis \(ta_md_set_clusters\) has n_min > 0 and reads "
                                             r"n_conn, but .*\(ta_md_set_order\) are off"):
            eng.md_run(1, DT)
        x, v = eng.md_state()
        assert np.array_equal(v, v0)   # nothing ran
        eng.md_set_order((4, 6), 3.0, 16, 2)
        eng.md_set_clusters(3.0, 8, None, 16, 1, 3)
        with pytest.raises(ValueError, match=r"ta_md_run: .*sample_every = 3 is no multiple of that of ta_md_set_order, 2"):
            eng.md_run(1, DT)
        eng.md_set_clusters(3.0, 8, None, 16, 1, 4)
        eng.md_run(3, DT)   # step 3
        assert eng.md_clusters()["n_samples"] == 1
        eng.md_set_clusters(3.0, 8, None, 16, 1, 4)   # first sample: step 4
        eng.md_run(2, DT)   # step 5
        eng.md_set_order((4, 6), 3.0, 16, 2)          # first sample: step 6, behind the clusters'
        with pytest.raises(ValueError, match=r"ta_md_run: .*its first sample, step 4, is in front of the first one of "
                                             r"ta_md_set_order, step 6"):
            eng.md_run(1, DT)
        eng.md_set_clusters(3.0, 8, None, 16, 1, 4)   # first sample: step 8
        eng.md_run(3, DT)
        assert (eng.md_clusters()["n_samples"], eng.md_clusters()["last_step"]) == (1, 8)
        eng.md_set_order(n_bins=0)
        eng.md_set_clusters(3.0, 0, None, 16, 1, 3)   # n_min 0 needs no order feature
        eng.md_run(1, DT)
        assert (eng.md_clusters()["n_samples"], eng.md_clusters()["last_step"]) == (1, 9)


def test_life_cycle_and_argument_errors(lib):
    from tensoralloy_amd import Engine
    nn, frames, v0 = _nimo()
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        with pytest.raises(ValueError, match="no resident batch"):
            eng.md_clusters()
        with pytest.raises(ValueError, match="no resident batch"):
            eng.md_cluster_atoms()
        eng.md_set_clusters(n_bins=0)   # off is always allowed
        assert eng.md_cluster_bins == 0
        with pytest.raises(ValueError, match="ta_md_set_clusters: no resident batch"):
            eng.md_set_clusters(n_bins=8)
        eng.set_frames(frames)
        with pytest.raises(ValueError, match="ta_md_get_clusters called before ta_md_init"):
            eng.md_clusters()
        with pytest.raises(ValueError, match="ta_md_get_cluster_atoms called before ta_md_init"):
            eng.md_cluster_atoms()
        with pytest.raises(ValueError, match="ta_md_set_clusters called before ta_md_init"):
            eng.md_set_clusters(n_bins=8)
        eng.md_init(None, v0)
        with pytest.raises(ValueError, match=r"ta_md_get_clusters: the cluster analysis is off \(ta_md_set_clusters\)"):
            eng.md_clusters()
        with pytest.raises(ValueError, match=r"ta_md_get_cluster_atoms: the cluster analysis is off"):
            eng.md_cluster_atoms()
        rl = np.array([[3.5, 3.2], [3.2, 3.0]])
        eng.md_set_clusters(rl, 0, ("Mo",), 8, 3, 2)
        assert eng.md_cluster_bins == 8
        nan, inf = float("nan"), float("inf")
        good = dict(r_link=3.0, n_min=0, species=None, n_bins=8, n_series=1, sample_every=1)
        for what, change in (("n_bins", dict(n_bins=-1)), ("n_bins", dict(n_bins=4097)), ("sample_every", dict(sample_every=0)),
                             ("sample_every", dict(sample_every=-2)), ("n_series must be 1 .. 1048576", dict(n_series=0)),
                             ("n_series must be 1 .. 1048576", dict(n_series=1048577)), ("n_min must be 0 .. 31", dict(n_min=-1)),
                             ("n_min must be 0 .. 31", dict(n_min=32)),
                             ("r_link must", dict(r_link=0.0)), ("r_link must", dict(r_link=-1.0)), ("r_link must", dict(r_link=inf)),
                             (r"r_link_pairs\[0\]\[1\] must", dict(r_link=[[3.0, nan], [nan, 3.0]])),
                             (r"r_link_pairs\[1\]\[1\] must", dict(r_link=[[3.0, 3.0], [3.0, 0.0]])),
                             (r"r_link_pairs\[1\]\[0\] = 6\.5\d* exceeds the model's cutoff", dict(r_link=[[3.0, 3.0], [6.5, 3.0]])),
                             (r"r_link_pairs is not symmetric: \[0\]\[1\]", dict(r_link=[[3.0, 3.1], [3.2, 3.0]])),
                             (r"r_link = 6\.00001\d* exceeds the model's cutoff.*not complete beyond", dict(r_link=6.00001))):
            with pytest.raises(ValueError, match="ta_md_set_clusters: " + what):
                eng.md_set_clusters(**dict(good, **change))
        p = eng._lib.ta_md_set_clusters   # the mask, through the C ABI
        from tensoralloy_amd import _lib
        for mask, what in ((0, "species_mask selects no element"), (4, "species_mask = 4 has a bit at or above n_elements = 2"),
                           (-1, "species_mask = -1 has a bit at or above n_elements = 2")):
            params = _lib.MdClusterParams(3.0, 0, mask, 8, 1, 1)
            assert p(eng._handle, C.byref(params), None) == _lib.TA_ERR_INVALID
            assert what in eng._lib.ta_last_error(eng._handle).decode()
        with pytest.raises(ValueError, match=r"md_set_clusters: r_link must be one distance or \[2, 2\]"):
            eng.md_set_clusters(**dict(good, r_link=[3.0, 3.0, 3.0]))
        with pytest.raises(ValueError, match="md_set_clusters: 'Fe' is not an element of the model"):
            eng.md_set_clusters(**dict(good, species=("Fe",)))
        with pytest.raises(ValueError, match="md_set_clusters: species index 2 is outside 0 .. 1"):
            eng.md_set_clusters(**dict(good, species=(2,)))
        out = eng.md_clusters()   # ... and a refused call left the setting as it was
        assert out["hist"].shape == (2, 8) and not out["hist"].any() and out["series"].shape == (0, 2, 4) and out["steps"].shape == (0,)
        assert np.array_equal(out["r_link"], rl)
        assert (out["n_samples"], out["n_bins"], out["sample_every"], out["last_step"], out["rows"], out["n_series"]) == (0, 8, 2, -1, 0, 3)
        with pytest.raises(ValueError, match="ta_md_get_cluster_atoms: no sample has been taken yet"):
            eng.md_cluster_atoms()
        res = eng.md_run(10, DT)
        assert set(res) == {"epot", "ekin", "n_rebuilds"}   # the result dict is unchanged
        out = eng.md_clusters()
        assert (out["n_samples"], out["last_step"], out["rows"]) == (6, 10, 3) and out["steps"].tolist() == [6, 8, 10]
        assert out["hist"].sum() == out["hist"][0].sum() > 0 and np.all(out["series"][:, 1] == [0, 0, 0, -1])
        assert eng.md_cluster_atoms()["step"] == 10
        # setting it again zeroes; sample 0 is then the first multiple of sample_every not behind the step
        eng.md_run(1, DT)   # step 11
        eng.md_set_clusters(None, 0, None, 4, 2, 3)
        out = eng.md_clusters()
        assert out["hist"].shape == (2, 4) and out["n_samples"] == 0 and not out["hist"].any()
        assert np.array_equal(out["r_link"], np.full((2, 2), 6.0))   # None: the model's cutoff
        with pytest.raises(ValueError, match="no sample has been taken yet"):
            eng.md_cluster_atoms()
        eng.md_run(5, DT)   # steps 12 .. 16: samples at 12 and 15
        out = eng.md_clusters()
        assert (out["n_samples"], out["last_step"], eng.md_cluster_atoms()["step"]) == (2, 15, 15) and out["steps"].tolist() == [12, 15]
        assert out["series"][:, :, :3].tolist() == [[[32, 1, 32]] * 2] * 2 and out["hist"][:, 3].tolist() == [2, 2]
        # off and on again: zero counts
        eng.md_set_clusters(n_bins=0)
        assert eng.md_cluster_bins == 0
        with pytest.raises(ValueError, match="cluster analysis is off"):
            eng.md_clusters()
        eng.md_run(1, DT)   # step 17, nothing found
        eng.md_set_clusters(3.0, 0, ("Ni", "Mo"), 4, 2, 3)
        assert eng.md_clusters()["n_samples"] == 0
        # set_frames keeps the setting and drops the data with the MD state; md_init starts from zero
        eng.set_frames(frames)
        with pytest.raises(ValueError, match="ta_md_get_clusters called before ta_md_init"):
            eng.md_clusters()
        eng.md_init(None, v0)
        out = eng.md_clusters()
        assert out["hist"].shape == (2, 4) and not out["hist"].any() and np.array_equal(out["r_link"], np.full((2, 2), 3.0))
        assert (out["n_samples"], out["sample_every"], out["last_step"], out["n_series"]) == (0, 3, -1, 2)
        eng.md_run(3, DT)
        assert (eng.md_clusters()["n_samples"], eng.md_clusters()["last_step"]) == (2, 3)
        # the barostat does not exclude this feature, nor do the other observables
        eng.md_set_barostat(0.0, 100 * DT, 1.0)
        eng.md_set_adf(16, 3.0, 1)
        eng.md_run(3, DT)
        assert (eng.md_clusters()["n_samples"], eng.md_clusters()["last_step"]) == (3, 6)
        assert eng.md_adf()["n_samples"] == 4


def test_getters_after_a_failed_run(lib):
    """A run that fails leaves the data invalid until `md_set_clusters` or `md_init` is called again. The failure is
    that of tests/test_gpu_md_order.py: 2^31 - 1 steps with a record of 128 frames at every step."""
    from tensoralloy_amd import Engine, _lib
    nn, atoms = _ni_setup()
    frames = [atoms] * 128
    v0 = np.tile(_velocities([atoms], 300.0, 3), (128, 1))
    null = C.POINTER(C.c_double)()

    def failing_run(eng):
        x0, v_before = eng.md_state()
        rc = eng._lib.ta_md_run(eng._handle, 2 ** 31 - 1, DT, WANT, 1, null, null, None)
        msg = eng._lib.ta_last_error(eng._handle).decode()
        assert rc in (_lib.TA_ERR_HIP, _lib.TA_ERR_NOMEM) and "hipMalloc" in msg
        x1, v1 = eng.md_state()
        assert np.array_equal(x0, x1) and np.array_equal(v_before, v1)

    refusal = r"ta_md_get_cluster%s: a ta_md_run failed and left the data invalid; call ta_md_set_clusters or ta_md_init again"
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        eng.set_frames(frames)
        eng.md_init(None, v0)
        eng.md_set_clusters(3.0, 0, None, 32, 2, 1)
        eng.md_run(2, DT)
        out = eng.md_clusters()
        assert out["n_samples"] == 3 and out["series"].shape == (2, 128, 4)
        assert np.array_equal(out["series"][-1, :, 3], 32 * np.arange(128))   # labels are indices in the batch
        assert out["hist"][:, 31].tolist() == [3] * 128
        failing_run(eng)
        with pytest.raises(ValueError, match=refusal % "s"):
            eng.md_clusters()
        with pytest.raises(ValueError, match=refusal % "_atoms"):
            eng.md_cluster_atoms()
        eng.md_run(1, DT)   # the loop goes on (step 3) and finds nothing; the getters still refuse
        with pytest.raises(ValueError, match=refusal % "s"):
            eng.md_clusters()
        eng.md_set_clusters(3.0, 0, None, 32, 2, 1)   # set again: zero, sample 0 is the state of step 3
        out = eng.md_clusters()
        assert (out["n_samples"], out["last_step"]) == (0, -1) and not out["hist"].any()
        eng.md_run(2, DT)
        out = eng.md_clusters()
        assert (out["n_samples"], out["last_step"]) == (3, 5) and out["steps"].tolist() == [4, 5]
        assert eng.md_cluster_atoms()["step"] == 5
        failing_run(eng)
        with pytest.raises(ValueError, match=refusal % "s"):
            eng.md_clusters()
        eng.md_init(None, v0)   # ... or md_init: the setting is kept, the data start from zero
        out = eng.md_clusters()
        assert (out["n_samples"], out["sample_every"], out["last_step"]) == (0, 1, -1) and not out["hist"].any()
        eng.md_run(1, DT)
        assert eng.md_clusters()["n_samples"] == 2


def test_device_md_end_to_end(lib):
    from tensoralloy_amd import Engine
    nn, atoms = _ni_setup()
    atoms = atoms.copy()
    v0 = _velocities([atoms], 2000.0, 3)
    setting, order = _setting(3.0, 9, ("Ni",), 32, 8, 3), ((4, 6), 3.0, 16, 3, (6, 0.993))
    with Engine(nn) as eng:
        dyn = md.DeviceMD(eng, atoms, DT, velocities=v0, order_bins=16, order_rbond=3.0, order_every=3,
                          order_solid=(6, 0.993), cluster_bins=32, cluster_rlink=3.0, cluster_nmin=9,
                          cluster_species=("Ni",), cluster_series=8, cluster_every=3, n_lags=16, sample_every=1)
        dyn.run(6)
        dyn.run(5)
        samples = eng.md_samples()
        assert np.array_equal(samples["steps"], np.arange(12))
        want = _reference(nn, [atoms], samples["x"][0:10:3], setting, order)
        out = dyn.get_clusters()
        assert (out["n_samples"], out["n_bins"], out["sample_every"], out["last_step"], out["rows"]) == (4, 32, 3, 9, 4)
        assert np.array_equal(out["hist"], want["hist"]) and np.array_equal(out["series"], want["series"])
        assert out["steps"].tolist() == [0, 3, 6, 9] and out["step"] == 9
        assert np.array_equal(out["label"], want["label"]) and np.array_equal(out["size"], want["size"])
        plain = md.DeviceMD(eng, atoms, DT, velocities=v0)   # cluster_bins None: the feature is set off
        assert eng.md_cluster_bins == 0
        with pytest.raises(ValueError, match=r"cluster analysis is off \(cluster_bins\)"):
            plain.get_clusters()
        with pytest.raises(ValueError, match=r"cluster analysis is off \(ta_md_set_clusters\)"):
            eng.md_clusters()
