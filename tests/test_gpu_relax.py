"""GPU: the device-resident FIRE relaxation (`ta_relax_run`, csrc/ta_relax.hip) against the NumPy reference
(tests/relax_reference.py) driven by the CPU oracle or by a second engine's `Engine.step`.

Parity bound 1e-9 (A, eV) on positions, FIRE velocities, energies, dt and a; npos, steps and converged flags
exactly. It is the bound of the MD tests, by the same reasoning: the fp64 force gaps of the project give about
1e-13 per step, and the damped map contracts them instead of spreading them. A trajectory comparison means
something only while no branch decision is marginal, so every test first asserts on the reference log that
|F.v| >= 1e-6 |v||F|, ||dr| - maxstep| >= 1e-6 maxstep and, where steps to convergence are counted,
|max|F| - fmax| >= 1e-6 fmax at every step (`relax_reference.assert_not_marginal`). Jitters, seeds and
parameters were chosen with the oracle so that these hold with three orders of magnitude to spare or more.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import md_reference
from tests import relax_reference as rr
from tests.helpers import fcc, make_eam, make_grap_nn, make_nn, oracle_eam_eval
from tensoralloy_amd import _lib, md
from tensoralloy_amd.atoms import atomic_masses

pytestmark = pytest.mark.gpu

TOL = 1e-9
WANT = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES
NEVER = 1e-10   # an fmax no test run reaches


def _positions(frames):
    return np.concatenate([a.positions for a in frames])


def _natoms(frames):
    return [len(a) for a in frames]


@functools.lru_cache(maxsize=None)
def _ni():
    return make_eam(["Ni"], 6.0, potential="zjw04")


def _oracle_forces(nn, frames):
    """Force callback of the reference: the CPU oracle, frame by frame."""
    natoms = _natoms(frames)

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


def _engine_forces(other):
    """Force callback from a second engine with skin 0 through `Engine.step` (an exact list at every call)."""
    def force(x):
        r = other.step(np.ascontiguousarray(x), WANT)
        return r["energy"].copy(), r["forces"].copy()
    return force


def _freeze(out):
    for a in list(out.values()) + list(out["state"].values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _device(nn, frames, runs, skin=0.5, fixed=None, **params):
    """The device relaxation of `frames` in the `relax_run` calls `runs` = [(max_steps, fmax), ...]: the state
    at the end, the dict of the last run, total steps per frame and total rebuilds."""
    from tensoralloy_amd import Engine
    with Engine(nn) as eng:
        eng.set_skin(skin)
        eng.set_frames(frames)
        eng.relax_init(fixed=fixed, **params)
        before = sum(eng.list_stats())
        steps, rebuilds, outs = 0, 0, []
        for max_steps, fmax in runs:
            out = eng.relax_run(max_steps, fmax)
            steps = steps + out["steps"]
            rebuilds += out["n_rebuilds"]
            outs.append(dict(out, x=eng.relax_state()["positions"]))
        st = eng.relax_state()
        listed = sum(eng.list_stats()) - before
    return dict(x=st["positions"], v=st["velocities"], dt=st["dt"], a=st["a"], npos=st["npos"], steps=steps,
                converged=out["converged"], fmax=out["fmax"], energy=out["energy"], n_rebuilds=rebuilds,
                outs=outs, listed=listed)


def _assert_parity(dev, ref, tol=TOL, what=""):
    gaps = {k: float(np.abs(dev[k] - ref[k]).max()) for k in ("x", "v", "energy", "dt", "a")}
    print("parity gaps", what, gaps, "steps", dev["steps"], ref["steps"], "rebuilds", dev["n_rebuilds"],
          ref["n_rebuilds"])
    assert np.array_equal(dev["npos"], ref["npos"]), (dev["npos"], ref["npos"])
    assert np.array_equal(dev["steps"], ref["steps"]), (dev["steps"], ref["steps"])
    assert np.array_equal(dev["converged"], ref["converged"])
    for k, g in gaps.items():
        assert g < tol, gaps


# -- the Ni zjw04 frames shared by several tests --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _frame(rep=(2, 2, 2), jitter=0.05, seed=3):
    return fcc(rep=rep, jitter=jitter, seed=seed)


HARD = dict(maxstep=0.05, dt=0.3)   # with jitter 0.1: 28 clamped steps, 5 uphill resets, dt grows after nmin


@functools.lru_cache(maxsize=None)
def _ref_hard(steps=40, skin=0.5):
    atoms = _frame(jitter=0.1)
    return _freeze(rr.run(_oracle_forces(_ni(), [atoms]), rr.new_state(atoms.positions, **HARD), steps, NEVER,
                          skin=skin))


@functools.lru_cache(maxsize=None)
def _ref_converged(fixed=None):
    atoms = _frame()
    mask = None
    if fixed is not None:
        mask = np.zeros(len(atoms), dtype=bool)
        mask[list(fixed)] = True
    return _freeze(rr.run(_oracle_forces(_ni(), [atoms]), rr.new_state(atoms.positions), 300, 1e-3, fixed=mask,
                          skin=0.5))


def test_parity_with_the_oracle(lib):
    """32 atoms, jitter 0.1, 40 steps that do not converge, with parameters under which the trajectory takes
    every branch: an uphill reset, a growing dt after nmin downhill steps and the maxstep clamp."""
    ref = _ref_hard()
    rr.assert_not_marginal(ref)
    steps = [e for e in rr.flat_log(ref) if "branch" in e]
    assert len(steps) == 40 and steps[0]["branch"] == "first"
    assert any(e["branch"] == "reset" for e in steps)
    assert any(e["dt_grew"] for e in steps)
    assert any(e["clamped"] for e in steps) and not all(e["clamped"] for e in steps)
    dev = _device(_ni(), [_frame(jitter=0.1)], [(40, NEVER)], **HARD)
    assert not dev["converged"].any() and dev["n_rebuilds"] == ref["n_rebuilds"]
    _assert_parity(dev, ref)
    assert abs(dev["fmax"][0] - ref["fmax"][0]) < TOL


def test_convergence(lib):
    from tensoralloy_amd import Engine
    ref = _ref_converged()
    rr.assert_not_marginal(ref, fmax=1e-3)
    assert ref["converged"].all() and ref["steps"][0] == 67
    atoms = _frame()
    dev = _device(_ni(), [atoms], [(300, 1e-3)])
    assert dev["converged"].all()
    _assert_parity(dev, ref)
    with Engine(_ni()) as eng:   # an independent evaluation of the final and of the first positions
        final = atoms.copy()
        final.positions[:] = dev["x"]
        res = eng.evaluate([final, atoms], want=WANT)
    fmax = np.sqrt((res[0]["forces"] ** 2).sum(axis=1).max())
    print("fmax", fmax, dev["fmax"][0], "energy", res[0]["energy"], res[1]["energy"])
    assert fmax < 1e-3 and abs(dev["fmax"][0] - fmax) < TOL
    assert abs(dev["energy"][0] - res[0]["energy"]) < TOL and res[0]["energy"] < res[1]["energy"] - 1e-3


def test_batch_of_three_frames(lib):
    """4, 32 and 108 atoms converge after 35, 67 and 66 steps: each freezes on its own while the others go on."""
    nn = _ni()
    frames = [_frame((1, 1, 1), 0.05, 5), _frame(), _frame((3, 3, 3), 0.03, 4)]
    natoms = _natoms(frames)
    assert natoms == [4, 32, 108]
    ref = rr.run(_oracle_forces(nn, frames), rr.new_state(_positions(frames), natoms), 300, 1e-3, skin=0.5)
    rr.assert_not_marginal(ref, fmax=1e-3)
    assert ref["converged"].all() and len(set(ref["steps"])) == 3
    dev = _device(nn, frames, [(300, 1e-3)])
    _assert_parity(dev, ref)
    assert dev["listed"] == ref["steps"].max()
    start = np.concatenate([[0], np.cumsum(natoms)])
    for f, atoms in enumerate(frames):   # every frame as when relaxed alone on the device
        alone = _device(nn, [atoms], [(300, 1e-3)])
        s = slice(start[f], start[f + 1])
        gaps = dict(x=np.abs(alone["x"] - dev["x"][s]).max(), v=np.abs(alone["v"] - dev["v"][s]).max(),
                    energy=abs(alone["energy"][0] - dev["energy"][f]), dt=abs(alone["dt"][0] - dev["dt"][f]))
        print("frame", f, gaps)
        assert alone["steps"][0] == dev["steps"][f] and alone["npos"][0] == dev["npos"][f]
        assert max(gaps.values()) < 1e-10, (f, gaps)
    # a run cut at the steps at which the first and the second frame converge: from its step on a frame does
    # not move by a bit while the others go on
    order = [int(f) for f in np.argsort(ref["steps"])]
    k0, k1 = int(ref["steps"][order[0]]), int(ref["steps"][order[1]])
    split = _device(nn, frames, [(k0, 1e-3), (k1 - k0, 1e-3), (300, 1e-3)])
    cut0, cut1, rest = split["outs"]
    assert list(cut0["converged"]) == [f == order[0] for f in range(3)] and list(cut0["steps"]) == [k0] * 3
    assert list(cut1["converged"]) == [f in order[:2] for f in range(3)] and cut1["steps"][order[0]] == 0
    assert rest["converged"].all() and rest["steps"][order[0]] == 0 and rest["steps"][order[1]] == 0
    for f, cut in ((order[0], cut0), (order[1], cut1)):
        s = slice(start[f], start[f + 1])
        assert np.array_equal(split["x"][s], cut["x"][s]), f
    s = slice(start[order[2]], start[order[2] + 1])
    assert np.abs(split["x"][s] - cut1["x"][s]).max() > 1e-9   # ... while the last one went on
    assert np.abs(split["x"] - dev["x"]).max() < 1e-12 and np.array_equal(split["steps"], dev["steps"])


def test_large_frame_converges_first(lib):
    """[1176, 32]: the frame of two workgroups (jitter 0.01) reaches fmax = 0.05 after 11 steps, the small one
    (jitter 0.1) does not within 20. Both workgroups of the converged frame, the one that keeps the frame's
    record and the other, leave its atoms alone: positions and velocities stay as they were, bit for bit."""
    from tensoralloy_amd import Engine
    nn = _ni()
    frames = [_frame((7, 7, 6), 0.01, 8), _frame(jitter=0.1)]
    natoms = _natoms(frames)
    with Engine(nn) as other:
        other.set_skin(0.0)
        other.set_frames(frames)
        ref = rr.run(_engine_forces(other), rr.new_state(_positions(frames), natoms), 20, 0.05, skin=0.3)
    rr.assert_not_marginal(ref, fmax=0.05)
    assert list(ref["converged"]) == [True, False] and list(ref["steps"]) == [11, 20]
    with Engine(nn) as eng:
        eng.set_skin(0.3)
        eng.set_frames(frames)
        eng.relax_init()
        a = eng.relax_run(11, 0.05)
        at_11 = eng.relax_state()
        b = eng.relax_run(9, 0.05)
        end = eng.relax_state()
    assert list(a["converged"]) == [True, False] and list(a["steps"]) == [11, 11]
    assert list(b["converged"]) == [True, False] and list(b["steps"]) == [0, 9]
    big = slice(0, 1176)
    for k in ("positions", "velocities"):
        assert np.array_equal(end[k][big], at_11[k][big]), k
        assert np.abs(end[k][1176:] - at_11[k][1176:]).max() > 1e-9, k
    dev = dict(x=end["positions"], v=end["velocities"], dt=end["dt"], a=end["a"], npos=end["npos"],
               steps=a["steps"] + b["steps"], converged=b["converged"], energy=b["energy"],
               n_rebuilds=a["n_rebuilds"] + b["n_rebuilds"])
    _assert_parity(dev, ref, what="[1176, 32], the large frame frozen")
    # in one run the same: the frozen frame's workgroups return while the small frame steps on
    whole = _device(nn, frames, [(20, 0.05)], skin=0.3)
    assert np.abs(whole["x"][big] - at_11["positions"][big]).max() < 1e-12 and list(whole["steps"]) == [11, 20]


def test_more_than_one_workgroup_per_frame(lib):
    """1176 atoms (7 x 7 x 6 cells) are two workgroups of the launches; in the batch [1176, 32] the frame
    boundary falls inside a chunk of 1024. Reference forces: a second engine with skin 0."""
    from tensoralloy_amd import Engine
    nn = _ni()
    big, small = _frame((7, 7, 6), 0.05, 8), _frame(jitter=0.1)
    assert len(big) == 1176
    for frames in ([big], [big, small]):
        with Engine(nn) as other:
            other.set_skin(0.0)
            other.set_frames(frames)
            ref = rr.run(_engine_forces(other), rr.new_state(_positions(frames), _natoms(frames)), 15, NEVER,
                         skin=0.3)
        rr.assert_not_marginal(ref)
        dev = _device(nn, frames, [(15, NEVER)], skin=0.3)
        assert dev["n_rebuilds"] == ref["n_rebuilds"]
        _assert_parity(dev, ref, what=f"{_natoms(frames)}")


def test_rebuilds(lib):
    """Jitter 0.1 and skin 0.05: the first five steps rebuild one after another, later ones inside a window of
    enqueued steps. The result does not depend on the skin."""
    nn, atoms = _ni(), _frame(jitter=0.1)
    force = _oracle_forces(nn, [atoms])
    refs = {skin: rr.run(force, rr.new_state(atoms.positions), 25, NEVER, skin=skin) for skin in (0.0, 0.05, 0.5)}
    ref = refs[0.05]
    rr.assert_not_marginal(ref)
    assert ref["rebuild_steps"][:5] == [1, 2, 3, 4, 5] and 5 < ref["n_rebuilds"] < 25
    assert refs[0.0]["n_rebuilds"] == 25 and refs[0.5]["n_rebuilds"] <= 2
    runs = {skin: _device(nn, [atoms], [(25, NEVER)], skin=skin) for skin in refs}
    for skin, dev in runs.items():
        assert dev["n_rebuilds"] == refs[skin]["n_rebuilds"], skin
        _assert_parity(dev, ref, what=f"skin {skin}")
        assert dev["listed"] == 25   # every step is one list build or one reuse
    for k in ("x", "v", "energy", "dt", "a"):
        assert np.abs(runs[0.0][k] - runs[0.5][k]).max() < TOL and np.abs(runs[0.05][k] - runs[0.5][k]).max() < TOL


def test_split_runs(lib):
    nn, atoms = _ni(), _frame(jitter=0.1)
    whole = _device(nn, [atoms], [(20, NEVER)], skin=0.05, **HARD)
    split = _device(nn, [atoms], [(7, NEVER), (13, NEVER)], skin=0.05, **HARD)
    assert list(split["outs"][0]["steps"]) == [7] and list(split["outs"][1]["steps"]) == [13]
    assert split["n_rebuilds"] == whole["n_rebuilds"] >= 1
    _assert_parity(split, whole, tol=1e-12, what="7 + 13 against 20")
    _assert_parity(whole, _ref_hard(20, 0.05))
    # a second run with a smaller fmax carries v, dt, a and npos on and wakes the frozen frame
    atoms = _frame()
    first = _ref_converged()
    second = rr.run(_oracle_forces(nn, [atoms]), first["state"], 300, 1e-4, skin=0.5)
    rr.assert_not_marginal(second, fmax=1e-4)
    assert second["converged"].all() and second["steps"][0] > 5
    assert rr.flat_log(second)[0]["branch"] in ("mix", "reset")   # not the first step again
    dev = _device(nn, [atoms], [(300, 1e-3), (300, 1e-4)])
    assert dev["outs"][0]["converged"].all() and dev["outs"][1]["steps"][0] == second["steps"][0]
    total = dict(second, steps=first["steps"] + second["steps"])
    _assert_parity(dev, total, what="fmax 1e-3, then 1e-4")
    carried = rr.flat_log(second)[0]["dt"]   # the first step of the second run starts from the dt of the first
    assert carried != 0.1 and 0.5 * first["dt"][0] <= carried <= 1.1 * first["dt"][0]
    assert dev["fmax"][0] < 1e-4 and dev["npos"][0] == second["npos"][0]


def test_fixed_mask(lib):
    from tensoralloy_amd import Engine
    nn, atoms = _ni(), _frame()
    fixed = (0, 5, 17, 31)
    mask = np.zeros(len(atoms), dtype=bool)
    mask[list(fixed)] = True
    ref = _ref_converged(fixed)
    rr.assert_not_marginal(ref, fmax=1e-3)
    assert ref["converged"].all() and ref["steps"][0] != _ref_converged()["steps"][0]
    for arg in (mask, list(fixed)):
        dev = _device(nn, [atoms], [(300, 1e-3)], fixed=arg)
        assert np.array_equal(dev["x"][mask], atoms.positions[mask]) and not dev["v"][mask].any()
        _assert_parity(dev, ref)
    with Engine(nn) as eng:   # converged on the free atoms only: the fixed ones still feel 0.3 eV / A and more
        final = atoms.copy()
        final.positions[:] = dev["x"]
        f = np.sqrt((eng.evaluate([final], want=WANT)[0]["forces"] ** 2).sum(axis=1))
    print("forces on fixed atoms", f[mask], "largest on a free atom", f[~mask].max(), dev["fmax"][0])
    assert f[mask].min() > 0.1 and f[~mask].max() < 1e-3 and abs(f[~mask].max() - dev["fmax"][0]) < TOL


@pytest.mark.parametrize("family", ["sf", "grap"])
def test_model_families(lib, family):
    """SF G2+G4 runs on the exact list filtered from the skin list, GRAP on the skin list itself."""
    from tensoralloy_amd import Engine
    if family == "sf":
        nn = make_nn(["Ni"], 6.0, True, [8])
    else:
        nn = make_grap_nn(["Ni"], 6.0, [16])
    frames = [_frame(jitter=0.02)]
    with Engine(nn) as other:
        other.set_skin(0.0)
        other.set_frames(frames)
        ref = rr.run(_engine_forces(other), rr.new_state(_positions(frames)), 15, NEVER, skin=0.3)
    rr.assert_not_marginal(ref)
    dev = _device(nn, frames, [(15, NEVER)], skin=0.3)
    assert dev["n_rebuilds"] == ref["n_rebuilds"]
    _assert_parity(dev, ref, what=family)


def test_md_after_relaxation(lib):
    from tensoralloy_amd import Engine
    nn, atoms = _ni(), _frame(jitter=0.1)
    masses = np.array([atomic_masses[z] for z in atoms.numbers], dtype=np.float64)
    v0 = md.maxwell_boltzmann(masses, md.kB * 300.0, np.random.RandomState(3))
    with Engine(nn) as eng:
        eng.set_skin(0.3)
        eng.set_frames([atoms])
        eng.relax_init()
        eng.relax_run(10, NEVER)
        relaxed = eng.relax_state()
        eng.md_init(None, v0)
        out = eng.md_run(5, md.fs)
        x, v = eng.md_state()
        after = eng.relax_state()   # the relaxation keeps its own velocities
        assert np.array_equal(after["velocities"], relaxed["velocities"]) and np.array_equal(after["positions"], x)
        again = eng.step(x, WANT)   # ... and a host-driven step works on what the run left
        assert abs(again["energy"][0] - out["epot"][-1, 0]) < 1e-10
        eng.set_frames([atoms])     # drops the relaxation state
        with pytest.raises(ValueError, match="before ta_relax_init"):
            eng.relax_run(1, 1e-3)
        with pytest.raises(ValueError, match="before ta_relax_init"):
            eng.relax_state()
    ref = md_reference.run(_oracle_forces(nn, [atoms]), relaxed["positions"], v0, masses, md.fs, 5)
    gaps = dict(x=np.abs(x - ref["x"]).max(), v=np.abs(v - ref["v"]).max(),
                epot=np.abs(out["epot"] - ref["epot"]).max(), ekin=np.abs(out["ekin"] - ref["ekin"]).max())
    print("md after relaxation", gaps)
    assert max(gaps.values()) < TOL, gaps


def test_refusals(lib):
    from tensoralloy_amd import Engine
    nn, atoms = _ni(), _frame()
    null_i, null_d = C.POINTER(C.c_int32)(), C.POINTER(C.c_double)()

    def refused(eng, rc, name):
        msg = eng._lib.ta_last_error(eng._handle).decode()
        assert rc == _lib.TA_ERR_INVALID and name in msg, (rc, name, msg)

    with Engine(nn) as eng:
        with pytest.raises(ValueError, match="no resident batch"):
            eng.relax_init()
        eng.set_skin(0.5)
        eng.set_frames([atoms])
        run = lambda steps, fmax: eng._lib.ta_relax_run(eng._handle, steps, fmax, WANT, null_i, null_i, null_d, null_i)
        refused(eng, run(1, 1e-3), "before ta_relax_init")
        good = dict(rr.DEFAULTS)
        bad = [("dt", 0.0), ("dt", float("nan")), ("dt", float("inf")), ("dtmax", -1.0), ("dtmax", float("inf")),
               ("maxstep", 0.0), ("maxstep", float("nan")), ("finc", 0.99), ("finc", float("nan")), ("fdec", 0.0),
               ("fdec", 1.0), ("fdec", float("nan")), ("fa", 0.0), ("fa", 1.0), ("astart", 0.0), ("astart", 1.01),
               ("astart", float("nan")), ("nmin", -1)]
        for name, value in bad:
            p = dict(good, **{name: value})
            fp = _lib.FireParams(*(p[k] for k in ("dt", "dtmax", "maxstep", "finc", "fdec", "astart", "fa")), p["nmin"])
            refused(eng, eng._lib.ta_relax_init(eng._handle, C.byref(fp), C.POINTER(C.c_uint8)()), name)
            with pytest.raises(ValueError, match=name):
                eng.relax_init(**{name: value})
        refused(eng, run(1, 1e-3), "before ta_relax_init")   # none of the failed calls left a state
        with pytest.raises(ValueError, match="unknown parameter"):
            eng.relax_init(timestep=0.1)
        with pytest.raises(ValueError, match="fixed"):
            eng.relax_init(fixed=np.zeros(len(atoms) + 1, dtype=bool))
        assert eng._lib.ta_relax_init(eng._handle, None, None) == _lib.TA_OK   # NULL: defaults, nothing fixed
        st = eng.relax_state()
        assert st["dt"][0] == 0.1 and st["a"][0] == 0.1 and st["npos"][0] == 0 and not st["velocities"].any()
        refused(eng, run(-1, 1e-3), "max_steps")
        for fmax in (0.0, -1.0, float("nan"), float("inf")):
            refused(eng, run(1, fmax), "fmax")
        with pytest.raises(ValueError, match="max_steps"):
            eng.relax_run(-1, 1e-3)
        # max_steps = 0: the flags of the state at entry, and nothing moves
        out = eng.relax_run(0, 1e-3)
        o = oracle_eam_eval(nn, atoms)
        fmax0 = np.sqrt((o["forces"] ** 2).sum(axis=1).max())
        assert list(out["steps"]) == [0] and not out["converged"][0] and out["n_rebuilds"] == 0
        assert abs(out["fmax"][0] - fmax0) < TOL and abs(out["energy"][0] - o["energy"]) < TOL
        out = eng.relax_run(0, 2.0 * fmax0)
        assert list(out["steps"]) == [0] and out["converged"][0]
        st = eng.relax_state()
        assert np.array_equal(st["positions"], atoms.positions) and not st["velocities"].any()
        assert st["dt"][0] == 0.1 and st["npos"][0] == 0
        eng.update_positions(atoms.positions)   # keeps the relaxation state
        assert list(eng.relax_run(2, NEVER)["steps"]) == [2]


def test_device_fire_through_a_calculator(lib, tmp_path):
    from tensoralloy_amd import DeviceFIRE, TensorAlloyCalculator
    nn = _ni()
    atoms = _frame().copy()
    start = atoms.positions.copy()
    ref = _ref_converged()
    calc = TensorAlloyCalculator(nn.export(str(tmp_path / "ni")))
    seen = []
    opt = DeviceFIRE(calc, atoms)
    e0 = opt.get_potential_energy()
    assert abs(e0 - oracle_eam_eval(nn, atoms)["energy"]) < TOL and opt.nsteps == 0
    opt.attach(lambda: seen.append((opt.nsteps, opt.get_potential_energy())), interval=25)
    assert opt.run(fmax=1e-3, steps=300) is True
    assert opt.nsteps == ref["steps"][0] and [s for s, _ in seen] == [25, 50]
    assert seen[0][1] < e0 and opt.get_potential_energy() < seen[1][1]
    assert np.abs(atoms.positions - ref["x"]).max() < TOL and np.abs(atoms.positions - start).max() > 1e-3
    assert np.sqrt((opt.get_forces() ** 2).sum(axis=1).max()) < 1e-3
    f = calc.get_forces(atoms)   # the calculator evaluates the relaxed positions, not what it had cached
    assert np.sqrt((np.asarray(f, dtype=np.float64) ** 2).sum(axis=1).max()) < 1e-3
    assert abs(calc.get_potential_energy(atoms) - opt.get_potential_energy()) < 1e-6
    # a list of structures gives an array of flags
    pair = [_frame().copy(), _frame((1, 1, 1), 0.05, 5).copy()]
    flags = DeviceFIRE(calc._engine, pair).run(fmax=1e-3, steps=40)
    assert list(flags) == [False, True]
