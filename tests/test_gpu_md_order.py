"""GPU: bond-orientational order inside the device MD loop (`ta_md_set_order`, csrc/ta_md_order.hip) against the NumPy
definition (tests/md_order_reference.py), which sweeps all atoms and all periodic images by brute force, takes Y_lm
from NumPy's Legendre polynomials and shares nothing with the library's neighbour list or its recurrences.

Per-atom arrays of the newest sample (q, qbar, q_lm) are compared with the absolute bound TOL; N_b and n_conn are
integers and compared exactly. TOL is 100 x the largest device-minus-reference difference of any per-atom value over
the cases of this file in the first GPU run (profiles/md_order.md); the issue caps it at 1e-10: the norm is
1-Lipschitz in the q_lm, and fp64 sums of at most 500 terms bounded by 1 leave about 1e-13. Every comparison prints
its largest difference (`order-diff`).

The histograms are integers and compared EXACTLY. That needs no value on a bin edge, no neighbour on a cutoff and no
bond on the solid threshold: every exact test first asserts, on the reference alone, that no q B or qbar B lies within
1e-7 of an integer 1 .. B - 1 (above B x TOL for B <= 256), no r / rb within 1e-9 of 1, no s_ij within 1e-8 of c, and
that no |q_solid| of an atom with neighbours is below 1e-3. A perfect lattice puts every atom on one value, so the
tests start from seeded, jittered positions; the perfect-fcc case compares per-atom values and hist_conn only. The
snapshots are the device's own whole-step states: `md_state()` between the calls of a cut run, or the position ring
of `md_set_sampling`.

The run that fails (for the getters behind it) fails on the host: its record buffers, 2^31 records of 128 frames, are
2.5 TB that no device has, and `ta_md_run` allocates them before it enqueues anything.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import md_order_reference as ref
from tests.helpers import fcc, make_eam
from tests.test_gpu_md import DT, WANT, _ni_setup, _velocities
from tests.test_gpu_md_rdf import SETUPS, _describe, _freeze, _nimo, _sampled, _sheared
from tensoralloy_amd import Atoms, md

pytestmark = pytest.mark.gpu

TOL = 8.9e-14   # 100 x 8.9e-16, the largest difference of the first GPU run (the two-element case); the cap is 1e-10
EDGE_BIN, EDGE_R, EDGE_S, MIN_NORM = 1e-7, 1e-9, 1e-8, 1e-3   # conditions on the reference, not tolerances


def _run(nn, frames, v0, skin, runs, bins=None, r_bond=None, every=1, degrees=(4, 6), solid=(6, 0.5), integrator="nve",
         lags=None, dt=DT, barostat=None):
    """The runs `runs` (steps per md_run call) on the device: final state, records, the whole-step positions (and
    cells) at entry and behind every call (`states`, `cells`, at the absolute steps `steps`), and with `bins` the
    counts (`order`) and the per-atom arrays of the newest sample (`atoms`). `lags`: `md_set_sampling(lags, 1)` is
    on as well and its ring is returned (`samples`)."""
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
            eng.md_set_order(degrees, r_bond, bins, every, solid)
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
            res["order"] = eng.md_order()
            res["atoms"] = eng.md_order_atoms()
        if lags is not None:
            res["samples"] = eng.md_samples()
    for k in ("epot", "ekin", "echain"):
        if k in outs[0]:
            res[k] = np.concatenate([o[k][1 if j else 0:] for j, o in enumerate(outs)])
    return _freeze(res)


def _reference(nn, frames, snapshots, bins, r_bond, degrees=(4, 6), solid=(6, 0.5), cells=None, bin_edges=True):
    d = _describe(nn, frames)
    if cells is not None:
        d["cells"] = cells
    out = ref.order_parameters(snapshots, degrees=degrees, n_bins=bins, r_bond=r_bond, solid=solid, **d)
    print("reference: nearest bin edge", out["gap_bin"], "bins, nearest cutoff", out["gap_r"], "nearest threshold",
          out["gap_s"], "smallest norm", out["min_norm"])
    assert out["gap_r"] >= EDGE_R and out["gap_s"] >= EDGE_S and out["min_norm"] >= MIN_NORM   # (on the reference alone)
    if bin_edges:
        assert out["gap_bin"] >= EDGE_BIN, out["gap_bin"]
    return _freeze(out)


def _assert_atoms(name, got, want, step):
    """The per-atom arrays of the newest sample: integers exactly, the rest within TOL (the largest difference is
    printed)."""
    assert got["step"] == step
    assert got["n_bonds"].dtype == np.int32 and got["n_conn"].dtype == np.int32
    assert np.array_equal(got["n_bonds"], want["n_bonds"]), np.argwhere(got["n_bonds"] != want["n_bonds"])[:5]
    assert np.array_equal(got["n_conn"], want["n_conn"]), np.argwhere(got["n_conn"] != want["n_conn"])[:5]
    worst = 0.0
    for key in ("q", "qbar", "qlm"):
        assert got[key].shape == want[key].shape, key
        assert np.all(np.isfinite(got[key])), key
        worst = max(worst, float(np.abs(got[key] - want[key]).max()))
    print("order-diff", name, worst)
    assert worst <= TOL, (name, worst)


def _assert_counts(dev, want, n_samples, every, last_step, r_bond=None, degrees=(4, 6), solid=(6, 0.5), hist_q=True):
    got = dev["order"]
    E = want["hist_conn"].shape[1]
    assert (got["n_samples"], got["n_bins"], got["sample_every"], got["last_step"]) == \
        (n_samples, want["hist_q"].shape[-1], every, last_step)
    assert got["degrees"] == tuple(degrees) and got["solid"] == tuple(solid)
    if r_bond is not None:
        assert np.array_equal(got["r_bond"], np.broadcast_to(np.asarray(r_bond, dtype=np.float64), (E, E)))
    for key in ("hist_q", "hist_qbar", "hist_conn") if hist_q else ("hist_conn",):
        assert got[key].dtype == np.int64 and got[key].shape == want[key].shape, key
        diff = got[key] != want[key]
        assert not diff.any(), (key, int(diff.sum()), np.argwhere(diff)[:5], got[key][diff][:5], want[key][diff][:5])
    n_atoms = got["n_by_element"]
    assert np.array_equal(got["hist_conn"].sum(axis=-1), n_samples * n_atoms)   # every atom of every sample, once
    assert np.array_equal(got["hist_q"].sum(axis=-1), n_samples * np.repeat(n_atoms[:, :, None], len(degrees), axis=2))
    assert np.array_equal(got["hist_qbar"].sum(axis=-1), got["hist_q"].sum(axis=-1))


# -- 1, 2, 3: single frame; cutting; the trajectory is untouched ------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ni108():
    return _ni_setup()[0], fcc(rep=(3, 3, 3), jitter=0.05, seed=17)


@functools.lru_cache(maxsize=None)
def _ni108_run(every, runs):
    nn, atoms = _ni108()
    return _run(nn, [atoms], _velocities([atoms], 600.0, 3), 0.3, list(runs), 200 if every else None, 3.0, every or 1,
                lags=16)


@pytest.mark.parametrize("every", [1, 3])
def test_single_frame_against_the_reference(lib, every):
    nn, atoms = _ni108()
    dev = _ni108_run(every, (12,))
    assert np.array_equal(dev["samples"]["steps"], np.arange(13))
    want = _reference(nn, [atoms], dev["samples"]["x"][::every], 200, 3.0)
    assert abs(want["n_bonds"].mean() - 12.0) < 0.5   # the first shell of fcc
    _assert_counts(dev, want, len(range(0, 13, every)), every, 12 // every * every, 3.0)
    _assert_atoms("single-%d" % every, dev["atoms"], want, 12 // every * every)
    assert dev["atoms"]["qlm"].shape == (108, 12) and dev["atoms"]["q"].shape == (108, 2)


@pytest.mark.parametrize("every", [1, 3])
def test_cut_run_reproduces_the_uncut_run_bit_for_bit(lib, every):
    uncut, cut = _ni108_run(every, (12,)), _ni108_run(every, (5, 0, 1, 4, 2))
    assert np.array_equal(uncut["x"], cut["x"]) and np.array_equal(uncut["v"], cut["v"])
    for key in ("n_samples", "n_bins", "sample_every", "last_step"):
        assert uncut["order"][key] == cut["order"][key], key
    for key in ("hist_q", "hist_qbar", "hist_conn"):
        assert np.array_equal(uncut["order"][key], cut["order"][key]) and cut["order"][key].sum() > 0, key
    assert uncut["atoms"]["step"] == cut["atoms"]["step"]
    for key in ("q", "qbar", "n_bonds", "n_conn", "qlm"):
        assert np.array_equal(uncut["atoms"][key], cut["atoms"][key]), key   # bitwise: the list fixes the order of the sums


def test_switching_the_feature_on_leaves_the_trajectory_bitwise_unchanged(lib):
    on, off = _ni108_run(1, (12,)), _ni108_run(0, (12,))
    assert "order" in on and "order" not in off
    for k in ("x", "v", "epot", "ekin", "states"):
        assert np.array_equal(on[k], off[k]), k
    assert np.array_equal(on["samples"]["x"], off["samples"]["x"]) and on["n_rebuilds"] == off["n_rebuilds"]


# -- 4: two elements, a cutoff per pair, one element absent from one frame, atoms without neighbours ----------
def test_two_elements_with_a_cutoff_per_pair_and_atoms_without_neighbours(lib):
    """Mo - Mo bonds below 1.5 A: none. Mo - Ni bonds below 2.45 A, under the nearest-neighbour distance 2.546 A of
    the a = 3.6 lattice: a few, from the jitter, and some Mo atoms have no neighbour at all."""
    nn, frames, v0 = _nimo()
    mo, ni = list(nn.elements).index("Mo"), list(nn.elements).index("Ni")
    rb = np.zeros((2, 2))
    rb[mo, mo], rb[ni, ni], rb[mo, ni], rb[ni, mo] = 1.5, 3.0, 2.45, 2.45
    dev = _run(nn, frames, v0, 0.3, [10], 100, rb, 2, lags=16)
    want = _reference(nn, frames, dev["samples"]["x"][::2], 100, rb)
    _assert_counts(dev, want, 6, 2, 10, rb)
    _assert_atoms("two-elements", dev["atoms"], want, 10)
    got, species = dev["atoms"], _describe(nn, frames)["species"]
    lone = got["n_bonds"] == 0
    assert lone.any() and np.all(species[lone] == mo) and (got["n_bonds"][species == mo] > 0).any()
    assert not got["q"][lone].any() and not got["qbar"][lone].any() and not got["n_conn"][lone].any()   # 0, never NaN
    assert not got["qlm"][lone].any()
    h = dev["order"]
    assert h["hist_q"][0, mo, 0, 0] >= lone.sum() and h["hist_qbar"][0, mo, 1, 0] >= lone.sum()   # ... and bin 0
    assert h["hist_conn"][0, mo, 0] >= lone.sum()
    assert np.array_equal(h["n_by_element"][:, mo], [16, 0])
    assert h["hist_q"][1, mo].sum() == 0 and h["hist_conn"][1, mo].sum() == 0 and h["hist_q"][1, ni].sum() == 2 * 6 * 32
    # the cutoffs matter: with 3.0 everywhere the integers differ
    other = ref.order_parameters(dev["samples"]["x"][::2], degrees=(4, 6), n_bins=100, r_bond=3.0, solid=(6, 0.5),
                                 **_describe(nn, frames))
    assert not np.array_equal(other["hist_q"][0], want["hist_q"][0]) and np.array_equal(other["hist_q"][1], want["hist_q"][1])


# -- 5: four degrees, unsorted, the largest l and odd l ---------------------------------------------------------
def test_four_unsorted_degrees_with_the_largest_and_odd_ones(lib):
    nn, atoms = _ni_setup()
    degrees, solid = (1, 12, 7, 2), (12, 0.3)
    dev = _run(nn, [atoms], _velocities([atoms], 600.0, 3), 0.3, [6], 128, 3.0, 3, degrees, solid, lags=8)
    want = _reference(nn, [atoms], dev["samples"]["x"][::3], 128, 3.0, degrees, solid)
    _assert_counts(dev, want, 3, 3, 6, 3.0, degrees, solid)
    _assert_atoms("four-degrees", dev["atoms"], want, 6)
    assert dev["atoms"]["qlm"].shape == (32, 2 + 13 + 8 + 3) and dev["atoms"]["q"].shape == (32, 4)
    q = dev["atoms"]["q"]
    assert q[:, 1].min() > 0.3 > q[:, 0].max()   # q12 of an fcc shell is large, q1 of a near-centrosymmetric one small


# -- 6: more than 64 neighbours: several rounds per wave, self-images -------------------------------------------
def test_many_neighbours_and_self_images_in_a_cell_below_the_cutoff(lib):
    """32 Ni atoms in a cubic cell of 6.4 A under a model with a cutoff of 6.5 A, bonds up to the cutoff: every
    centre has some 140 neighbours (three rounds of 64 per wave), among them its own images along the cell edges
    and several images of other atoms. B = 201 as in the bond-angle tests where lattice vectors are neighbours."""
    nn = make_eam(["Ni"], 6.5, potential="zjw04")
    atoms = fcc(a=3.2, rep=(2, 2, 2), jitter=0.05, seed=9)
    assert np.asarray(atoms.get_cell(complete=True))[0, 0] < 6.5
    dev = _run(nn, [atoms], _velocities([atoms], 300.0, 3), 0.3, [2, 2], 201, None, 2)
    xs, steps = _sampled(dev, 2)
    assert np.array_equal(steps, [0, 2, 4])
    want = _reference(nn, [atoms], xs, 201, 6.5)
    print("neighbours per centre:", want["n_bonds"].min(), "..", want["n_bonds"].max())
    assert want["n_bonds"].min() > 128
    _assert_counts(dev, want, 3, 2, 4, 6.5)   # r_bond None: the model's cutoff
    _assert_atoms("many-neighbours", dev["atoms"], want, 4)


# -- 7: batch edges ---------------------------------------------------------------------------------------------
def test_frames_of_1_7_and_108_atoms_one_sheared(lib):
    """A single atom in a cubic cell of 2.5 A (its six nearest images are its only neighbours below 3.0 A: the
    simple-cubic shell), 7 atoms (fewer than the 8 centres of a workgroup) and a sheared cell of 108 (a chunk
    boundary inside the frame: 13 workgroups of 8 and one of 4)."""
    nn = _ni_setup()[0]
    one = Atoms(symbols=["Ni"], positions=[[0.3, 0.1, -0.2]], cell=np.diag([2.5] * 3), pbc=True)
    eight = fcc(rep=(2, 1, 1), jitter=0.05, seed=5)
    seven = Atoms(symbols=["Ni"] * 7, positions=eight.positions[:7], cell=np.asarray(eight.get_cell(complete=True)), pbc=True)
    frames = [one, seven, _sheared(fcc(rep=(3, 3, 3), jitter=0.05, seed=4))]
    assert [len(a) for a in frames] == [1, 7, 108]
    v0 = _velocities(frames, 300.0, 11)
    v0[0] = 0.0
    dev = _run(nn, frames, v0, 0.3, [4, 4], 150, 3.0, 4)
    xs, steps = _sampled(dev, 4)
    assert np.array_equal(steps, [0, 4, 8])
    want = _reference(nn, frames, xs, 150, 3.0)
    _assert_counts(dev, want, 3, 4, 8, 3.0)
    _assert_atoms("batch-edges", dev["atoms"], want, 8)
    got = dev["atoms"]
    assert got["n_bonds"][0] == 6 and got["n_conn"][0] == 6   # its own images: s_ij = 1
    assert got["q"][0] == pytest.approx([np.sqrt(7.0 / 12.0), np.sqrt(1.0 / 8.0)], abs=TOL)
    assert got["qbar"][0] == pytest.approx(got["q"][0], abs=TOL)


# -- 8: list rebuilds in the middle of a run ----------------------------------------------------------------------
def test_rebuilds_inside_the_window(lib):
    """2000 K with a skin of 0.1: the run rebuilds its list inside the windows of steps that the loop enqueues
    ahead. One sample per scheduled step all the same, the integers of the reference, and the per-atom values of
    a run with a large skin (another list order) to rounding, not bit for bit."""
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 2000.0, 3)
    dev = _run(nn, [atoms], v0, 0.1, [12], 120, 3.0, 1, lags=16)
    assert dev["n_rebuilds"] > 0
    assert np.array_equal(dev["samples"]["steps"], np.arange(13))
    want = _reference(nn, [atoms], dev["samples"]["x"], 120, 3.0)
    _assert_counts(dev, want, 13, 1, 12, 3.0)   # 13 samples: nothing counted twice or skipped around a redone step
    _assert_atoms("rebuilds", dev["atoms"], want, 12)
    calm = _run(nn, [atoms], v0, 0.6, [12], 120, 3.0, 1)
    assert calm["n_rebuilds"] == 0
    _assert_atoms("large-skin", calm["atoms"], want, 12)
    _assert_atoms("rebuilds-vs-large-skin", dev["atoms"], calm["atoms"], 12)


# -- 9: thermostats, the barostat -------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator", ["nve", "berendsen", "langevin", "nhc"])
def test_every_thermostat(lib, integrator):
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 2000.0, 3)
    plain = _run(nn, [atoms], v0, 0.1, [4, 4, 3], None, None, 1, integrator=integrator)
    dev = _run(nn, [atoms], v0, 0.1, [4, 4, 3], 120, 3.0, 4, integrator=integrator)
    assert dev["n_rebuilds"] == plain["n_rebuilds"] >= 1
    for k in ("x", "v", "epot", "ekin", "states") + (("echain",) if integrator == "nhc" else ()):
        assert np.array_equal(dev[k], plain[k]), k   # bit for bit: the launches only read the state
    xs, steps = _sampled(dev, 4)
    assert np.array_equal(steps, [0, 4, 8])
    want = _reference(nn, [atoms], xs, 120, 3.0)
    _assert_counts(dev, want, 3, 4, 8, 3.0)
    _assert_atoms("thermostat-" + integrator, dev["atoms"], want, 8)


def test_under_the_barostat_with_the_cells_of_the_sampled_state(lib):
    """Cell and atoms scaled by 1.02, P0 = 0, taup = 20 fs: the cell shrinks from the first step on. The run cut
    at every sampled step hands out the positions (`md_state`) and the cells (`md_cells`) of those states for the
    reference; one uncut run must give the same integers. The bonds reach to 5.9 A, with images of the 7.19 A
    cell among the neighbours, so that the cells enter."""
    nn, atoms = _ni_setup()
    big = Atoms(symbols=atoms.get_chemical_symbols(), positions=atoms.positions * 1.02,
                cell=np.asarray(atoms.get_cell(complete=True)) * 1.02, pbc=True)
    v0 = _velocities([big], 600.0, 3)
    baro = (0.0, 20 * DT, 0.9)
    cut = _run(nn, [big], v0, 0.3, [3, 3, 2], 120, 5.9, 3, integrator="berendsen", barostat=baro)
    uncut = _run(nn, [big], v0, 0.3, [8], 120, 5.9, 3, integrator="berendsen", barostat=baro)
    xs, steps = _sampled(cut, 3)
    cells = cut["cells"][np.isin(cut["steps"], steps)]
    assert np.array_equal(steps, [0, 3, 6]) and cells.shape == (3, 1, 3, 3)
    assert abs(np.linalg.det(cells[2, 0])) < abs(np.linalg.det(cells[1, 0])) < abs(np.linalg.det(cells[0, 0]))
    want = _reference(nn, [big], xs, 120, 5.9, cells=cells)
    stale = ref.order_parameters(xs, degrees=(4, 6), n_bins=120, r_bond=5.9, solid=(6, 0.5), **_describe(nn, [big]))
    assert np.abs(stale["q"] - want["q"]).max() > 1e-9   # (with the cell of the entry state the values differ)
    for name, dev in (("barostat-cut", cut), ("barostat-uncut", uncut)):
        _assert_counts(dev, want, 3, 3, 6, 5.9)
        _assert_atoms(name, dev["atoms"], want, 6)


# -- 10: a static structure through md_run(0) -------------------------------------------------------------------
def test_perfect_fcc_at_step_0(lib):
    nn = _ni_setup()[0]
    atoms = fcc(rep=(3, 3, 3), jitter=0.0)
    dev = _run(nn, [atoms], np.zeros((108, 3)), 0.3, [0], 64, 3.0, 1)
    want = _reference(nn, [atoms], dev["states"][:1], 64, 3.0, bin_edges=False)   # (every atom on one value)
    _assert_counts(dev, want, 1, 1, 0, 3.0, hist_q=False)
    _assert_atoms("perfect-fcc", dev["atoms"], want, 0)
    got = dev["atoms"]
    assert np.abs(got["q"] - [np.sqrt(7.0 / 192.0), np.sqrt(169.0 / 512.0)]).max() <= TOL
    assert np.abs(got["qbar"] - [np.sqrt(7.0 / 192.0), np.sqrt(169.0 / 512.0)]).max() <= TOL
    assert np.array_equal(got["n_bonds"], [12] * 108) and np.array_equal(got["n_conn"], [12] * 108)
    hist = dev["order"]["hist_conn"]
    assert hist[0, 0, 12] == 108 == hist.sum()


# -- 11: an ordered and a disordered half -----------------------------------------------------------------------
def test_a_frame_half_ordered_half_disordered(lib):
    """108 atoms: the lower half of the cell jittered by 0.02 A, the upper half by 0.6 A. With at least 8 solid
    bonds an atom counts as solid. Measured (device and reference alike): all 54 ordered atoms are solid, the two
    layers next to the disordered half included, and none of the 54 disordered ones."""
    nn = _ni_setup()[0]
    atoms = fcc(rep=(3, 3, 3), jitter=0.0)
    x = np.asarray(atoms.positions).copy()
    ordered = x[:, 2] < 0.5 * np.asarray(atoms.get_cell(complete=True))[2, 2] - 0.1
    assert ordered.sum() == 54
    rng = np.random.RandomState(134)   # (no two atoms nearer than 1.1 A)
    x += np.where(ordered[:, None], 0.02, 0.6) * rng.standard_normal(x.shape)
    frame = Atoms(symbols=["Ni"] * 108, positions=x, cell=np.asarray(atoms.get_cell(complete=True)), pbc=True)
    dev = _run(nn, [frame], np.zeros((108, 3)), 0.3, [0], 100, 3.0, 1)
    want = _reference(nn, [frame], dev["states"][:1], 100, 3.0)
    _assert_counts(dev, want, 1, 1, 0, 3.0)
    _assert_atoms("mixed", dev["atoms"], want, 0)
    solid = md.classify_solid(dev["atoms"]["n_conn"], 8)
    assert np.array_equal(solid, md.classify_solid(want["n_conn"], 8))
    print("solid atoms: ordered half", int(solid[ordered].sum()), "of 54, disordered half", int(solid[~ordered].sum()), "of 54")
    assert solid[ordered].sum() > solid[~ordered].sum()   # more solid atoms in the ordered half
    frac = md.solid_fraction(dev["order"]["hist_conn"], 8)
    assert frac.shape == (1, 1) and frac[0, 0] == pytest.approx(solid.mean(), abs=1e-15)
    q, p = md.order_distribution(dev["order"]["hist_q"])
    assert p.shape == (1, 1, 2, 100) and (p[0, 0, 1] / 100.0).sum() == pytest.approx(1.0, abs=1e-12)


# -- 12: life cycle and refusals --------------------------------------------------------------------------------
def test_life_cycle_and_refusals(lib):
    from tensoralloy_amd import Engine
    nn, frames, v0 = _nimo()
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        with pytest.raises(ValueError, match="no resident batch"):
            eng.md_order()
        with pytest.raises(ValueError, match="no resident batch"):
            eng.md_order_atoms()
        eng.md_set_order(n_bins=0)   # off is always allowed
        assert eng.md_order_bins == 0
        with pytest.raises(ValueError, match="ta_md_set_order: no resident batch"):
            eng.md_set_order(n_bins=8)
        eng.set_frames(frames)
        with pytest.raises(ValueError, match="ta_md_get_order called before ta_md_init"):
            eng.md_order()
        with pytest.raises(ValueError, match="ta_md_get_order_atoms called before ta_md_init"):
            eng.md_order_atoms()
        with pytest.raises(ValueError, match="ta_md_set_order called before ta_md_init"):
            eng.md_set_order(n_bins=8)
        eng.md_init(None, v0)
        with pytest.raises(ValueError, match=r"ta_md_get_order: the bond-orientational order parameters are off \(ta_md_set_order\)"):
            eng.md_order()
        with pytest.raises(ValueError, match=r"ta_md_get_order_atoms: the bond-orientational order parameters are off"):
            eng.md_order_atoms()
        rb = np.array([[3.5, 3.2], [3.2, 3.0]])
        eng.md_set_order((6, 4), rb, 8, 2, (4, 0.25))
        assert eng.md_order_bins == 8
        nan, inf = float("nan"), float("inf")
        good = dict(degrees=(4, 6), r_bond=3.0, n_bins=8, sample_every=1, solid=(6, 0.5))
        for what, change in (("n_bins", dict(n_bins=-1)), ("n_bins", dict(n_bins=4097)), ("sample_every", dict(sample_every=0)),
                             ("sample_every", dict(sample_every=-2)),
                             ("n_degrees must be 1 .. 4", dict(degrees=())), ("n_degrees must be 1 .. 4", dict(degrees=(1, 2, 3, 4, 6))),
                             (r"degrees\[1\] = 0 must be 1 .. 12", dict(degrees=(6, 0))),
                             (r"degrees\[0\] = 13 must be 1 .. 12", dict(degrees=(13, 6))),
                             (r"degrees\[2\] = 6 is given twice", dict(degrees=(6, 4, 6))),
                             ("solid_degree = 8 is not among the degrees", dict(solid=(8, 0.5))),
                             ("solid_threshold must", dict(solid=(6, 1.0))), ("solid_threshold must", dict(solid=(6, -1.0))),
                             ("solid_threshold must", dict(solid=(6, nan))), ("solid_threshold must", dict(solid=(6, inf))),
                             ("r_bond must", dict(r_bond=0.0)), ("r_bond must", dict(r_bond=-1.0)),
                             ("r_bond must", dict(r_bond=nan)), ("r_bond must", dict(r_bond=inf)),
                             (r"r_bond_pairs\[0\]\[1\] must", dict(r_bond=[[3.0, nan], [nan, 3.0]])),
                             (r"r_bond_pairs\[1\]\[1\] must", dict(r_bond=[[3.0, 3.0], [3.0, 0.0]])),
                             (r"r_bond_pairs\[1\]\[0\] = 6\.5\d* exceeds the model's cutoff", dict(r_bond=[[3.0, 3.0], [6.5, 3.0]])),
                             (r"r_bond_pairs is not symmetric: \[0\]\[1\]", dict(r_bond=[[3.0, 3.1], [3.2, 3.0]])),
                             (r"r_bond = 6\.00001\d* exceeds the model's cutoff.*not complete beyond", dict(r_bond=6.00001))):
            with pytest.raises(ValueError, match="ta_md_set_order: " + what):
                eng.md_set_order(**dict(good, **change))
        with pytest.raises(ValueError, match=r"md_set_order: r_bond must be one distance or \[2, 2\]"):
            eng.md_set_order(**dict(good, r_bond=[3.0, 3.0, 3.0]))
        out = eng.md_order()   # ... and a refused call left the setting as it was
        assert out["hist_q"].shape == out["hist_qbar"].shape == (2, 2, 2, 8) and out["hist_conn"].shape == (2, 2, 32)
        assert not out["hist_q"].any() and not out["hist_qbar"].any() and not out["hist_conn"].any()
        assert out["degrees"] == (6, 4) and out["solid"] == (4, 0.25) and np.array_equal(out["r_bond"], rb)
        assert (out["n_samples"], out["n_bins"], out["sample_every"], out["last_step"]) == (0, 8, 2, -1)
        with pytest.raises(ValueError, match="ta_md_get_order_atoms: no sample has been taken yet"):
            eng.md_order_atoms()
        res = eng.md_run(10, DT)
        assert set(res) == {"epot", "ekin", "n_rebuilds"}   # the result dict is unchanged
        out = eng.md_order()
        assert (out["n_samples"], out["last_step"]) == (6, 10) and out["hist_conn"].sum() == 6 * 64
        assert eng.md_order_atoms()["step"] == 10
        # setting it again zeroes; sample 0 is then the first multiple of sample_every not behind the step
        eng.md_run(1, DT)   # step 11
        eng.md_set_order((6,), None, 4, 3, (6, 0.5))
        out = eng.md_order()
        assert out["hist_q"].shape == (2, 2, 1, 4) and out["n_samples"] == 0 and not out["hist_q"].any() and not out["hist_conn"].any()
        assert np.array_equal(out["r_bond"], np.full((2, 2), 6.0))
        with pytest.raises(ValueError, match="no sample has been taken yet"):
            eng.md_order_atoms()
        eng.md_run(5, DT)   # steps 12 .. 16: samples at 12 and 15
        assert (eng.md_order()["n_samples"], eng.md_order()["last_step"], eng.md_order_atoms()["step"]) == (2, 15, 15)
        assert eng.md_order_atoms()["qlm"].shape == (64, 7)
        # off and on again: zero counts
        eng.md_set_order(n_bins=0)
        assert eng.md_order_bins == 0
        with pytest.raises(ValueError, match="order parameters are off"):
            eng.md_order()
        eng.md_run(1, DT)   # step 17, nothing counted
        eng.md_set_order((4, 6), 3.0, 4, 3)
        out = eng.md_order()
        assert out["n_samples"] == 0 and not out["hist_q"].any()
        # set_frames keeps the setting and drops the data with the MD state; md_init starts from zero counts
        eng.set_frames(frames)
        with pytest.raises(ValueError, match="ta_md_get_order called before ta_md_init"):
            eng.md_order()
        eng.md_init(None, v0)
        out = eng.md_order()
        assert out["hist_q"].shape == (2, 2, 2, 4) and not out["hist_q"].any() and np.array_equal(out["r_bond"], np.full((2, 2), 3.0))
        assert (out["n_samples"], out["sample_every"], out["last_step"]) == (0, 3, -1)
        eng.md_run(3, DT)
        assert (eng.md_order()["n_samples"], eng.md_order()["last_step"]) == (2, 3)
        # the barostat does not exclude this feature, nor do the other observables
        eng.md_set_barostat(0.0, 100 * DT, 1.0)
        eng.md_set_adf(16, 3.0, 1)
        eng.md_run(3, DT)
        assert (eng.md_order()["n_samples"], eng.md_order()["last_step"]) == (3, 6)
        assert eng.md_adf()["n_samples"] == 4


def test_getters_after_a_failed_run(lib):
    """A run that fails leaves the counts invalid until `md_set_order` or `md_init` is called again. The failure:
    n_steps = 2^31 - 1 with a record of 128 frames at every step asks for 2.5 TB of `epot` records. `ta_md_run`
    allocates them first, inside its guarded body and behind the point where it marks the counts invalid; the
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

    refusal = r"ta_md_get_order%s: a ta_md_run failed and left the counts invalid; call ta_md_set_order or ta_md_init again"
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        eng.set_frames(frames)
        eng.md_init(None, v0)
        eng.md_set_order((4, 6), 3.0, 16, 1)
        eng.md_run(2, DT)
        assert eng.md_order()["n_samples"] == 3
        failing_run(eng)
        with pytest.raises(ValueError, match=refusal % ""):
            eng.md_order()
        with pytest.raises(ValueError, match=refusal % "_atoms"):
            eng.md_order_atoms()
        eng.md_run(1, DT)   # the loop goes on (step 3) and counts nothing; the getters still refuse
        with pytest.raises(ValueError, match=refusal % ""):
            eng.md_order()
        eng.md_set_order((4, 6), 3.0, 16, 1)   # set again: zero counts, sample 0 is the state of step 3
        out = eng.md_order()
        assert (out["n_samples"], out["last_step"]) == (0, -1) and not out["hist_q"].any() and not out["hist_conn"].any()
        eng.md_run(2, DT)
        out = eng.md_order()
        assert (out["n_samples"], out["last_step"]) == (3, 5)
        assert out["hist_q"][0].sum() == out["hist_q"][127].sum() == 3 * 32 * 2
        assert eng.md_order_atoms()["step"] == 5
        failing_run(eng)
        with pytest.raises(ValueError, match=refusal % ""):
            eng.md_order()
        eng.md_init(None, v0)   # ... or md_init: the setting is kept, the counts start from zero
        out = eng.md_order()
        assert (out["n_samples"], out["sample_every"], out["last_step"]) == (0, 1, -1) and not out["hist_q"].any()
        eng.md_run(1, DT)
        assert eng.md_order()["n_samples"] == 2


# -- the tiled histogram and DeviceMD ---------------------------------------------------------------------------
def test_the_tiled_histogram_rebins_the_stored_values(lib):
    """4096 bins of two elements and four degrees are 2 x 2 x 4 x 4096 = 65536 LDS words: the workgroups tile over
    the bins in passes of 8192 / 16 = 512 bins. The values of the same state at 64 bins are the coarse-grained ones."""
    nn, frames, v0 = _nimo()
    degrees, solid = (4, 6, 8, 10), (6, 0.5)
    fine = _run(nn, frames, v0, 0.3, [0], 4096, 3.3, 1, degrees, solid)
    coarse = _run(nn, frames, v0, 0.3, [0], 64, 3.3, 1, degrees, solid)
    for key in ("q", "qbar", "n_conn", "qlm"):
        assert np.array_equal(fine["atoms"][key], coarse["atoms"][key]), key
    want = _reference(nn, frames, fine["states"][:1], 4096, 3.3, degrees, solid, bin_edges=False)
    assert want["gap_bin"] >= 4096 * TOL   # (the condition at this bin count)
    _assert_counts(fine, want, 1, 1, 0, 3.3, degrees, solid)
    for key in ("hist_q", "hist_qbar"):
        h = fine["order"][key]
        assert np.array_equal(h.reshape(h.shape[:-1] + (64, 64)).sum(axis=-1), coarse["order"][key]), key
        assert len({k // 512 for k in np.nonzero(h.sum(axis=(0, 1, 2)))[0]}) >= 3   # several passes hold atoms
    assert np.array_equal(fine["order"]["hist_conn"], coarse["order"]["hist_conn"])


def test_device_md_end_to_end(lib):
    from tensoralloy_amd import Engine
    nn, atoms = _ni_setup()
    atoms = atoms.copy()
    x0 = atoms.positions.copy()
    v0 = _velocities([atoms], 600.0, 3)
    with Engine(nn) as eng:
        dyn = md.DeviceMD(eng, atoms, DT, velocities=v0, temperature_K=600.0, tdamp=20 * DT, order_bins=80, order_rbond=3.0,
                          order_every=3, adf_bins=90, adf_rbond=3.0, n_lags=16, sample_every=1)
        dyn.run(6)
        dyn.run(5)
        samples = eng.md_samples()
        assert np.array_equal(samples["steps"], np.arange(12)) and np.array_equal(samples["x"][0], x0)
        out = eng.md_order()
        assert (out["n_samples"], out["n_bins"], out["sample_every"], out["last_step"]) == (4, 80, 3, 9)
        want = _reference(nn, [atoms], samples["x"][0:10:3], 80, 3.0)
        for key in ("hist_q", "hist_qbar", "hist_conn"):
            assert np.array_equal(out[key], want[key]), key
        per_atom = dyn.get_order_atoms()
        _assert_atoms("device-md", per_atom, want, 9)
        q, p, pbar = dyn.get_order()
        assert q.shape == (80,) and p.shape == pbar.shape == (1, 2, 80)
        assert np.array_equal(p, md.order_distribution(want["hist_q"][0])[1])
        assert (p[0, 1] / 80.0).sum() == pytest.approx(1.0, abs=1e-12)
        assert eng.md_adf()["n_samples"] == 12   # the bond-angle distributions beside it
        plain = md.DeviceMD(eng, atoms, DT, velocities=v0)   # order_bins None: the feature is set off
        assert eng.md_order_bins == 0
        with pytest.raises(ValueError, match=r"bond-orientational order is off \(order_bins\)"):
            plain.get_order()
        with pytest.raises(ValueError, match=r"bond-orientational order is off \(order_bins\)"):
            plain.get_order_atoms()
        with pytest.raises(ValueError, match=r"order parameters are off \(ta_md_set_order\)"):
            eng.md_order()
