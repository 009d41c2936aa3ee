"""GPU: cells relaxed together with the atoms by the device FIRE loop (`ta_relax_set_cell`, the kCell builds of
csrc/ta_relax.hip) against the NumPy reference (tests/relax_cell_reference.py) driven by the CPU oracle or by a
second engine's `Engine.step(x, cells=h)`.

Parity bound 1e-9 (A, eV) on positions, deformation gradient, cells, velocities (atoms and cell rows), energy, dt
and a; npos, steps and converged flags exactly: the bound and the reasoning of tests/test_gpu_relax.py. The
positions pass through q = x G^-T, x = q' G'^T at every step, which costs a few ulp of x (1e-15) per step and
does not show at 1e-9. Every comparison first asserts on the reference log that no branch decision is marginal
(`assert_not_marginal`). The anchor: 32 Ni atoms (fcc 2 x 2 x 2, jitter 0.03, seed 3), Zjw04, rc = 6, strained
by [[1.03, .01, 0], [0, .98, .005], [0, 0, 1.01]], ASE's default parameters, fmax = 1e-3, skin 0.5: the reference
with the oracle converges after 96 steps without a rebuild at p = 0 (smallest |cos(F, v)| 1.2e-2, clamp margin
0.50, fmax margin 4e-2) and after 99 steps with one rebuild, at step 61, at p = 0.05 eV / A^3 (3.8e-2, 3.3e-2,
0.13).
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import relax_cell_reference as rc
from tests.helpers import fcc, make_eam, make_grap_nn, make_nn, oracle_eam_eval
from tensoralloy_amd import _lib

pytestmark = pytest.mark.gpu

TOL = 1e-9
WANT = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES | _lib.TA_WANT_VIRIAL
NEVER = 1e-10   # an fmax no test run reaches
RC = 6.0
STRAIN = np.array([[1.03, .01, 0], [0, .98, .005], [0, 0, 1.01]])


def _positions(frames):
    return np.concatenate([a.positions for a in frames])


def _cells(frames):
    return np.array([np.asarray(a.get_cell(complete=True)) for a in frames])


def _natoms(frames):
    return [len(a) for a in frames]


@functools.lru_cache(maxsize=None)
def _ni():
    return make_eam(["Ni"], RC, potential="zjw04")


def _strained(atoms, strain):
    a = atoms.copy()
    a.set_cell(np.asarray(a.get_cell(complete=True)) @ np.asarray(strain), scale_atoms=True)
    return a


@functools.lru_cache(maxsize=None)
def _anchor():
    return _strained(fcc(rep=(2, 2, 2), jitter=0.03, seed=3), STRAIN)


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
    for a in list(out.values()) + list(out["state"].values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _state_of(eng, out, steps, rebuilds, outs, listed):
    st, cs = eng.relax_state(), eng.relax_cell_state()
    return dict(x=st["positions"], v=st["velocities"], dt=st["dt"], a=st["a"], npos=st["npos"], G=cs["deform"],
                vc=cs["cell_velocities"], cells=cs["cells"], cell_fmax=cs["cell_fmax"], steps=steps,
                converged=out["converged"], fmax=out["fmax"], energy=out["energy"], n_rebuilds=rebuilds, outs=outs,
                listed=listed)


def _device(nn, frames, runs, skin=0.5, fixed=None, cell=None, **params):
    """The device cell relaxation of `frames` in the `relax_run` calls `runs` = [(max_steps, fmax), ...]; `cell`:
    keywords of `Engine.relax_set_cell`."""
    from tensoralloy_amd import Engine
    with Engine(nn) as eng:
        eng.set_skin(skin)
        eng.set_frames(frames)
        eng.relax_init(fixed=fixed, **params)
        eng.relax_set_cell(True, **(cell or {}))
        before = sum(eng.list_stats())
        steps, rebuilds, outs = 0, 0, []
        for max_steps, fmax in runs:
            out = eng.relax_run(max_steps, fmax)
            steps = steps + out["steps"]
            rebuilds += out["n_rebuilds"]
            outs.append(dict(out, x=eng.relax_state()["positions"], cells=eng.relax_cell_state()["cells"]))
        return _state_of(eng, out, steps, rebuilds, outs, sum(eng.list_stats()) - before)


def _reference(force, frames, max_steps, fmax, skin=0.5, fixed=None, cell=None, **params):
    c = dict(cell or {})
    st = rc.new_state(_positions(frames), _cells(frames), _natoms(frames), cell_factor=c.get("cell_factor"),
                      pressure=c.get("pressure", 0.0), mask=c.get("mask"), hydrostatic=c.get("hydrostatic", False),
                      **params)
    return rc.run(force, st, max_steps, fmax, fixed=fixed, skin=skin, rc=RC)


def _assert_parity(dev, ref, tol=TOL, what=""):
    gaps = {k: float(np.abs(dev[k] - ref[k]).max()) for k in ("x", "v", "G", "vc", "cells", "energy", "dt", "a")}
    print("parity gaps", what, gaps, "steps", dev["steps"], ref["steps"], "rebuilds", dev["n_rebuilds"],
          ref["n_rebuilds"], ref.get("end_rebuild"))
    assert np.array_equal(dev["npos"], ref["npos"]), (dev["npos"], ref["npos"])
    assert np.array_equal(dev["steps"], ref["steps"]), (dev["steps"], ref["steps"])
    assert np.array_equal(dev["converged"], ref["converged"])
    for k, g in gaps.items():
        assert g < tol, gaps


def _assert_rebuilds(dev, ref):
    """The rebuilds the strain-aware rule asks for, and the one for the final cells where the run moved them."""
    assert dev["n_rebuilds"] == ref["n_rebuilds"] + int(ref["end_rebuild"]), (dev["n_rebuilds"], ref["rebuild_steps"],
                                                                              ref["end_rebuild"])


@functools.lru_cache(maxsize=None)
def _ref_anchor(pressure):
    atoms = _anchor()
    return _freeze(_reference(_oracle_forces(_ni(), [atoms]), [atoms], 300, 1e-3, cell=dict(pressure=pressure)))


# -- 1 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pressure", [0.0, 0.05])
def test_parity_with_the_oracle(lib, pressure):
    """The anchor frame through `DeviceFIRE(cell=True)` to fmax = 1e-3: the trajectory of the reference, a
    stress of -p I within what fmax allows, the cell h0 G^T, and the cell written into the `Atoms`."""
    from tensoralloy_amd import DeviceFIRE, Engine
    ref = _ref_anchor(pressure)
    rc.assert_not_marginal(ref, fmax=1e-3)
    assert ref["converged"].all() and ref["steps"][0] == (96 if pressure == 0.0 else 99)
    assert ref["rebuild_steps"] == ([] if pressure == 0.0 else [61]) and ref["end_rebuild"]
    atoms = _anchor().copy()
    h0 = np.asarray(atoms.get_cell(complete=True)).copy()
    with Engine(_ni()) as eng:
        eng.set_skin(0.5)
        opt = DeviceFIRE(eng, atoms, cell=True, scalar_pressure=pressure)
        assert opt.nsteps == 0 and np.array_equal(np.asarray(atoms.get_cell(complete=True)), h0)
        assert opt.run(fmax=1e-3, steps=300) is True
        out = dict(converged=opt.converged, fmax=opt.fmax, energy=opt.energy)
        dev = _state_of(eng, out, np.array([opt.nsteps]), opt.n_rebuilds, [], 0)
        stress = opt.get_stress()
        n = len(atoms)
    _assert_parity(dev, ref, what=f"p = {pressure}")
    _assert_rebuilds(dev, ref)
    assert abs(dev["fmax"][0] - ref["fmax"][0]) < TOL and abs(dev["cell_fmax"][0] - ref["cell_fmax"][0]) < TOL
    V = abs(np.linalg.det(dev["cells"][0]))
    s = np.array([[stress[0], stress[5], stress[4]], [stress[5], stress[1], stress[3]], [stress[4], stress[3], stress[2]]])
    rows = np.sqrt(((s + pressure * np.eye(3)) ** 2).sum(axis=1)) * V / n
    print("stress", stress, "rows", rows, "lattice constants", np.linalg.norm(dev["cells"][0], axis=1) / 2)
    assert rows.max() < 1e-3 and np.abs(np.diag(s) + pressure).max() < 1e-4
    assert np.abs(dev["cells"][0] - h0 @ dev["G"][0].T).max() < 1e-13
    assert np.array_equal(np.asarray(atoms.get_cell(complete=True)), dev["cells"][0])
    assert np.array_equal(atoms.positions, dev["x"]) and atoms.get_volume() == pytest.approx(V, rel=1e-15)
    if pressure == 0.0:
        assert np.all(np.abs(np.linalg.norm(dev["cells"][0], axis=1) / 2 - 3.51955) < 2.5e-4)


# -- 2 ---------------------------------------------------------------------------------------------------
SHRINK = dict(strain=np.diag([1.06, 1.0, 1.0]), skin=0.2, steps=40)


@functools.lru_cache(maxsize=None)
def _ref_shrink():
    """The frame centred on the origin (no |x| above 2.9 A) and stretched by 6 % along x: on its way back the
    strain uses the skin up at steps 11 and 31 (lim drops to 0.019 and 0.008 A against |u| of 0.031 and 0.012)
    while no atom is further than 0.087 A < skin / 2 from where the list was built."""
    atoms = fcc(rep=(2, 2, 2), jitter=0.01, seed=3)
    atoms.positions[:] -= np.asarray(atoms.get_cell(complete=True)).sum(axis=0) / 2 - 3.524 / 4
    atoms = _strained(atoms, SHRINK["strain"])
    return atoms, _freeze(_reference(_oracle_forces(_ni(), [atoms]), [atoms], SHRINK["steps"], NEVER,
                                     skin=SHRINK["skin"]))


def test_rebuilds_triggered_by_strain(lib):
    """A stretched cell with little jitter shrinks back: the strain alone uses the skin up while no atom has
    moved skin / 2 from where the list was built. The device rebuilds at the reference's steps: a run of m
    steps builds one list for every rebuild step <= m and one more for its final cells unless step m itself
    rebuilt, so the counts of the runs of s - 1, s and s + 1 steps pin every rebuild step s."""
    from tensoralloy_amd import Engine
    atoms, ref = _ref_shrink()
    skin, total = SHRINK["skin"], SHRINK["steps"]
    rc.assert_not_marginal(ref)
    rebuilds = ref["rebuild_steps"]
    print("rebuilds", ref["rebuild_info"])
    assert rebuilds == [11, 31] and rebuilds[-1] < total
    assert all(i["plain"] < 0.5 * skin for i in ref["rebuild_info"])   # the fixed-cell rule would not have fired

    def expected(m):
        return sum(1 for s in rebuilds if s <= m) + (0 if m in rebuilds or m == 0 else 1)
    lengths = sorted({m for s in rebuilds for m in (s - 1, s, s + 1)} | {total})
    for m in lengths:
        dev = _device(_ni(), [atoms], [(m, NEVER)], skin=skin)
        assert dev["n_rebuilds"] == expected(m), (m, dev["n_rebuilds"], expected(m), rebuilds)
        assert dev["listed"] == m + (0 if m in rebuilds or m == 0 else 1)
    _assert_parity(dev, ref, what="strain rebuilds")
    final = atoms.copy()
    final.set_cell(dev["cells"][0])
    final.positions[:] = dev["x"]
    with Engine(_ni()) as eng:   # skin 0: an exact list
        fresh = eng.evaluate([final], want=WANT)[0]
    print("energy", dev["energy"][0], fresh["energy"])
    assert abs(dev["energy"][0] - fresh["energy"]) < 1e-10


# -- 3 ---------------------------------------------------------------------------------------------------
def test_batch_of_three_frames(lib):
    """[32 strained, 108 strained otherwise, 32 relaxed before]: each frame as in its solo run, the relaxed one
    frozen at the first test, the others freezing on their own."""
    nn = _ni()
    done = _ref_anchor(0.0)
    relaxed = _anchor().copy()
    relaxed.set_cell(done["cells"][0])
    relaxed.positions[:] = done["x"]
    big = _strained(fcc(rep=(3, 3, 3), jitter=0.03, seed=4), [[0.98, 0, .01], [0, 1.02, 0], [0, 0, 1.0]])
    frames = [_anchor(), big, relaxed]
    natoms = _natoms(frames)
    assert natoms == [32, 108, 32] and done["fmax"][0] < 0.97e-3
    dev = _device(nn, frames, [(300, 1e-3)])
    print("steps", dev["steps"], "fmax", dev["fmax"])
    assert dev["converged"].all() and dev["steps"][2] == 0 and len(set(dev["steps"])) == 3
    assert dev["steps"][0] == done["steps"][0]
    start = np.concatenate([[0], np.cumsum(natoms)])
    assert np.array_equal(dev["x"][start[2]:], relaxed.positions) and np.array_equal(dev["cells"][2], _cells([relaxed])[0])
    assert np.array_equal(dev["G"][2], np.eye(3))
    for f, atoms in enumerate(frames):
        alone = _device(nn, [atoms], [(300, 1e-3)])
        s = slice(start[f], start[f + 1])
        gaps = dict(x=np.abs(alone["x"] - dev["x"][s]).max(), v=np.abs(alone["v"] - dev["v"][s]).max(),
                    G=np.abs(alone["G"][0] - dev["G"][f]).max(), cells=np.abs(alone["cells"][0] - dev["cells"][f]).max(),
                    vc=np.abs(alone["vc"][0] - dev["vc"][f]).max(), energy=abs(alone["energy"][0] - dev["energy"][f]),
                    dt=abs(alone["dt"][0] - dev["dt"][f]))
        print("frame", f, gaps)
        assert alone["steps"][0] == dev["steps"][f] and alone["npos"][0] == dev["npos"][f]
        assert max(gaps.values()) < 1e-10, (f, gaps)
    # cut where the first of the two moving frames converges: it does not move again while the other goes on
    first, last = (0, 1) if dev["steps"][0] < dev["steps"][1] else (1, 0)
    k0 = int(dev["steps"][first])
    split = _device(nn, frames, [(k0, 1e-3), (300, 1e-3)])
    cut, rest = split["outs"]
    assert cut["converged"][first] and not cut["converged"][last] and rest["steps"][first] == 0
    s = slice(start[first], start[first + 1])
    assert np.array_equal(split["x"][s], cut["x"][s]) and np.array_equal(split["cells"][first], cut["cells"][first])
    s = slice(start[last], start[last + 1])
    assert np.abs(split["x"][s] - cut["x"][s]).max() > 1e-9
    assert np.array_equal(split["steps"], dev["steps"]) and np.abs(split["x"] - dev["x"]).max() < 1e-10


# -- 4 ---------------------------------------------------------------------------------------------------
def test_more_than_one_workgroup_per_frame(lib):
    """1372 atoms (7 x 7 x 7 cells) are two workgroups of the launches: both add the same cell rows to the
    frame's sums and only the first writes G and the cell. Reference forces and virials: a second engine. Cell
    factor 200, so that the cell rows carry a visible share of the step."""
    from tensoralloy_amd import Engine
    nn = _ni()
    big = _strained(fcc(rep=(7, 7, 7), jitter=0.03, seed=8), [[1.01, .004, 0], [0, .99, 0], [0, .002, 1.005]])
    assert len(big) == 1372
    with Engine(nn) as other:
        other.set_skin(0.0)
        other.set_frames([big])
        ref = _reference(_engine_forces(other), [big], 10, NEVER, skin=0.3, cell=dict(cell_factor=200.0))
    rc.assert_not_marginal(ref)
    dev = _device(nn, [big], [(10, NEVER)], skin=0.3, cell=dict(cell_factor=200.0))
    _assert_rebuilds(dev, ref)
    _assert_parity(dev, ref, what="1372 atoms")
    assert np.abs(dev["G"][0] - np.eye(3)).max() > 1e-4   # (with the default factor, 1372, ten steps move G by 1e-5)


# -- 5 ---------------------------------------------------------------------------------------------------
def test_mask_and_hydrostatic(lib):
    nn, atoms = _ni(), _anchor()
    force = _oracle_forces(nn, [atoms])
    cell = dict(mask=[1, 1, 0, 0, 0, 1])
    ref = _reference(force, [atoms], 30, NEVER, cell=cell)
    rc.assert_not_marginal(ref)
    dev = _device(nn, [atoms], [(30, NEVER)], cell=cell)
    _assert_parity(dev, ref, what="mask xx yy xy")
    G = dev["G"][0]
    assert np.array_equal(G[2], [0.0, 0.0, 1.0]) and np.array_equal(G[:, 2], [0.0, 0.0, 1.0])
    assert not dev["vc"][0][2].any() and not dev["vc"][0][:, 2].any()
    assert abs(G[0, 0] - 1.0) > 1e-3 and abs(G[0, 1]) > 1e-5 and abs(G[1, 0]) > 1e-5
    cell = dict(hydrostatic=True, pressure=0.02)
    ref = _reference(force, [atoms], 30, NEVER, cell=cell)
    rc.assert_not_marginal(ref)
    dev = _device(nn, [atoms], [(30, NEVER)], cell=cell)
    _assert_parity(dev, ref, what="hydrostatic")
    G = dev["G"][0]
    assert np.abs(G - np.eye(3) * G[0, 0]).max() < 1e-14 and abs(G[0, 0] - 1.0) > 1e-3


# -- 6 ---------------------------------------------------------------------------------------------------
def test_fixed_atoms_move_with_the_cell(lib):
    nn, atoms = _ni(), _anchor()
    mask = np.zeros(len(atoms), dtype=bool)
    mask[[0, 5, 17, 31]] = True
    ref = _reference(_oracle_forces(nn, [atoms]), [atoms], 30, NEVER, fixed=mask)
    rc.assert_not_marginal(ref)
    dev = _device(nn, [atoms], [(30, NEVER)], fixed=mask)
    _assert_parity(dev, ref, what="fixed atoms")
    q = dev["x"][mask] @ np.linalg.inv(dev["G"][0]).T
    print("fixed atoms: q gap", np.abs(q - atoms.positions[mask]).max())
    assert np.abs(q - atoms.positions[mask]).max() < 1e-12 and not dev["v"][mask].any()
    assert np.abs(dev["x"][mask] - atoms.positions[mask]).max() > 1e-3   # ... while x moved with the cell


# -- 7 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["sf_triangles", "sf_per_apex", "grap", "adp"])
def test_model_families(lib, family):
    """10 steps against a second engine. The frame's periodic widths are 6.91 to 7.26 A and skin is 0.5: with
    rc = 6.0 they exceed rc + skin and the triangle-once backward pass runs; with rc = 6.45 they lie between rc
    and rc + skin, where a valid list no longer guarantees widths above rc, and the per-apex pass must run."""
    from tensoralloy_amd import Engine
    rcut = 6.45 if family == "sf_per_apex" else 6.0
    if family.startswith("sf"):
        nn = make_nn(["Ni"], rcut, True, [8])
    elif family == "grap":
        nn = make_grap_nn(["Ni"], rcut, [16])
    else:
        nn = make_eam(["Ni"], rcut, adp=True)
    frames = [_strained(fcc(rep=(2, 2, 2), jitter=0.02, seed=3), STRAIN)]
    with Engine(nn) as other:
        other.set_skin(0.0)
        other.set_frames(frames)
        st = rc.new_state(_positions(frames), _cells(frames), _natoms(frames))
        ref = rc.run(_engine_forces(other), st, 10, NEVER, skin=0.5, rc=rcut)
    rc.assert_not_marginal(ref)
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        eng.set_frames(frames)
        eng.relax_init()
        if family == "sf_per_apex":   # with fixed cells the widths admit the triangle pass
            eng.relax_run(0, NEVER)
            assert eng.backward_variant() == 2
        eng.relax_set_cell(True)
        out = eng.relax_run(10, NEVER)
        variant = eng.backward_variant()
        dev = _state_of(eng, out, out["steps"], out["n_rebuilds"], [], 0)
    if family.startswith("sf"):
        assert variant == (2 if family == "sf_triangles" else 1), variant
    _assert_rebuilds(dev, ref)
    _assert_parity(dev, ref, what=family)


# -- 8 ---------------------------------------------------------------------------------------------------
def test_split_runs(lib):
    """7 + 13 steps against 20. The first run ends with the list for its final cells, so the second evaluates on
    another list than the whole run does: the states agree up to summation order."""
    nn, atoms = _ni(), _anchor()
    whole = _device(nn, [atoms], [(20, NEVER)], cell=dict(pressure=0.05))
    split = _device(nn, [atoms], [(7, NEVER), (13, NEVER)], cell=dict(pressure=0.05))
    assert list(split["outs"][0]["steps"]) == [7] and list(split["outs"][1]["steps"]) == [13]
    assert whole["n_rebuilds"] == 1 and split["n_rebuilds"] == 2
    gaps = {k: float(np.abs(split[k] - whole[k]).max()) for k in ("x", "v", "G", "vc", "cells", "dt", "a")}
    print("7 + 13 against 20", gaps, abs(split["energy"][0] - whole["energy"][0]))
    assert max(gaps.values()) < 1e-12 and np.array_equal(split["npos"], whole["npos"])
    assert abs(split["energy"][0] - whole["energy"][0]) < 1e-10
    # a second run with a smaller fmax carries on
    ref = _ref_anchor(0.05)
    dev = _device(nn, [atoms], [(300, 1e-2), (300, 1e-3)], cell=dict(pressure=0.05))
    assert dev["outs"][0]["converged"].all() and dev["converged"].all()
    assert 0 < dev["outs"][0]["steps"][0] < ref["steps"][0] and dev["outs"][1]["steps"][0] > 0
    assert dev["fmax"][0] < 1e-3 and abs(dev["energy"][0] - ref["energy"][0]) < 1e-6


# -- 9 ---------------------------------------------------------------------------------------------------
def test_after_a_cell_run(lib):
    from tensoralloy_amd import Engine
    nn, atoms = _ni(), _anchor()
    with Engine(nn) as eng:
        eng.set_skin(0.3)
        eng.set_frames([atoms])
        eng.relax_init()
        eng.relax_set_cell(True)
        out = eng.relax_run(25, NEVER)
        x, cells = eng.relax_state()["positions"], eng.relax_cell_state()["cells"]
        assert np.abs(cells[0] - _cells([atoms])[0]).max() > 1e-3
        assert eng._volumes[0] == pytest.approx(abs(np.linalg.det(cells[0])), rel=1e-15)
        final = atoms.copy()
        final.set_cell(cells[0])
        final.positions[:] = x
        with Engine(nn) as other:
            fresh = other.evaluate([final], want=WANT)[0]
        assert abs(out["energy"][0] - fresh["energy"]) < 1e-10
        stress = eng._per_frame(eng.fetch(WANT))[0]["stress"]     # W / V of the relaxed cell
        assert np.abs(stress - fresh["stress"]).max() < 1e-10
        # a host-driven step with cells=None means the relaxed cell
        builds = eng.list_stats()[0]
        again = eng.step(x, WANT)
        assert eng.list_stats()[0] == builds and abs(again["energy"][0] - fresh["energy"]) < 1e-10
        assert np.abs(again["virial"][0] - fresh["virial"]).max() < 1e-9
        # the MD loop starts from the relaxed state and keeps the cell
        eng.md_init()
        md = eng.md_run(5, 1.0)
        assert abs(md["epot"][0, 0] - out["energy"][0]) < 1e-10
        eng.update_positions(x)
        # cells from the caller replace the relaxed ones: they are h0 of what follows
        mine = cells * 1.001
        eng.update_positions(x * 1.001, mine)
        now = eng.relax_cell_state()
        assert np.array_equal(now["cells"], mine) and np.array_equal(now["deform"][0], np.eye(3))
        assert not now["cell_velocities"].any()
        eng.relax_run(3, NEVER)
        now = eng.relax_cell_state()
        assert np.abs(now["cells"][0] - mine[0] @ now["deform"][0].T).max() < 1e-13
        assert np.abs(now["deform"][0] - np.eye(3)).max() > 1e-6
        eng.update_positions(x, cells)
        # fixed cells again: the cell stays, the atoms go on
        eng.relax_set_cell(False)
        fixed = eng.relax_run(10, NEVER)
        after = eng.relax_cell_state()
        assert list(fixed["steps"]) == [10] and np.array_equal(after["cells"], cells)
        assert np.abs(eng.relax_state()["positions"] - x).max() > 1e-6
        final.positions[:] = eng.relax_state()["positions"]
        with Engine(nn) as other:
            fresh = other.evaluate([final], want=WANT)[0]
        assert abs(fixed["energy"][0] - fresh["energy"]) < 1e-10


# -- 10 --------------------------------------------------------------------------------------------------
def test_refusals(lib):
    from tensoralloy_amd import Engine
    nn, atoms = _ni(), _anchor()

    def refused(eng, code, name):
        msg = eng._lib.ta_last_error(eng._handle).decode()
        assert code == _lib.TA_ERR_INVALID and name in msg, (code, name, msg)

    def params(cell_factor=0.0, pressure=0.0, mask=(1, 1, 1, 1, 1, 1), hydrostatic=0):
        return _lib.RelaxCellParams(cell_factor, pressure, (C.c_int32 * 6)(*mask), hydrostatic, 0)

    with Engine(nn) as eng:
        with pytest.raises(ValueError, match="no resident batch"):
            eng.relax_set_cell(True)
        eng.set_skin(0.5)
        eng.set_frames([atoms])
        set_cell = lambda p: eng._lib.ta_relax_set_cell(eng._handle, 1, C.byref(p))
        refused(eng, set_cell(params()), "before ta_relax_init")
        with pytest.raises(ValueError, match="before ta_relax_init"):
            eng.relax_cell_state()
        eng.relax_init()
        eng.relax_set_cell(True, pressure=0.05, cell_factor=10.0)
        eng.relax_run(3, NEVER)
        kept = eng.relax_cell_state()
        bad = [("cell_factor", dict(cell_factor=-1.0)), ("cell_factor", dict(cell_factor=float("nan"))),
               ("cell_factor", dict(cell_factor=float("inf"))), ("pressure", dict(pressure=float("nan"))),
               ("pressure", dict(pressure=float("inf"))), ("mask", dict(mask=(0, 0, 0, 0, 0, 0)))]
        for name, kw in bad:
            refused(eng, set_cell(params(**kw)), name)
            with pytest.raises(ValueError, match=name):
                eng.relax_set_cell(True, **kw)
        with pytest.raises(ValueError, match="mask"):
            eng.relax_set_cell(True, mask=[1, 1, 1])
        now = eng.relax_cell_state()      # none of the refused calls touched G, the velocities or the parameters
        assert all(np.array_equal(now[k], kept[k]) for k in kept)
        whole = _device(nn, [atoms], [(6, NEVER)], cell=dict(pressure=0.05, cell_factor=10.0))
        eng.relax_run(3, NEVER)
        assert np.abs(eng.relax_cell_state()["deform"] - whole["G"]).max() < 1e-12
        assert eng._lib.ta_relax_set_cell(eng._handle, 1, None) == _lib.TA_OK     # NULL: the defaults
        assert np.array_equal(eng.relax_cell_state()["deform"][0], np.eye(3))
        eng.relax_init()                  # switches the option off
        before = eng.relax_cell_state()["cells"]
        eng.relax_run(3, NEVER)
        assert np.array_equal(eng.relax_cell_state()["cells"], before)
    slab = atoms.copy()
    slab.pbc = [True, True, False]
    with Engine(nn) as eng:
        eng.set_frames([atoms, slab])
        eng.relax_init()
        with pytest.raises(ValueError, match="frame 1 is not periodic"):
            eng.relax_set_cell(True)
        assert list(eng.relax_run(2, NEVER)["steps"]) == [2, 2]   # fixed cells, as before the refusal


# -- 11 --------------------------------------------------------------------------------------------------
def test_option_off_is_the_fixed_cell_run(lib):
    """Switched on and off again before the run, the option leaves no trace: positions, velocities, dt and a
    are those of an engine that never heard of it, bit for bit."""
    from tensoralloy_amd import Engine
    nn, atoms = _ni(), _anchor()
    states = []
    for touch in (False, True):
        with Engine(nn) as eng:
            eng.set_skin(0.5)
            eng.set_frames([atoms])
            eng.relax_init(maxstep=0.05, dt=0.3)
            if touch:
                eng.relax_set_cell(True, pressure=0.05)
                eng.relax_set_cell(False)
            out = eng.relax_run(30, NEVER)
            states.append((eng.relax_state(), out))
    (a, out_a), (b, out_b) = states
    for k in ("positions", "velocities", "dt", "a", "npos"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(out_a["energy"], out_b["energy"]) and out_a["n_rebuilds"] == out_b["n_rebuilds"]
