"""CPU: the NumPy FIRE reference (tests/relax_reference.py) on analytic potentials, the argument checks of
`DeviceFIRE` that need no device, and the binding's export list."""
import numpy as np
import pytest

from tests import relax_reference as rr


def _bowl(k, x_min, natoms=None):
    """E = 1/2 sum k (x - x_min)^2 per frame: anisotropic when `k` differs between components."""
    k, x_min = np.asarray(k, dtype=np.float64), np.asarray(x_min, dtype=np.float64)
    natoms = [len(x_min)] if natoms is None else natoms
    start = np.concatenate([[0], np.cumsum(natoms)])

    def force(x):
        d = x - x_min
        e = 0.5 * (k * d * d).sum(axis=1)
        return np.array([e[a:b].sum() for a, b in zip(start[:-1], start[1:])]), -k * d
    return force


def _one_frame():
    rng = np.random.RandomState(7)
    x_min = rng.uniform(0.0, 4.0, (6, 3))
    k = np.tile([1.0, 7.0, 30.0], (6, 1)) * rng.uniform(0.8, 1.2, (6, 1))
    return _bowl(k, x_min), x_min, x_min + rng.normal(0.0, 0.3, (6, 3))


def _two_frames():
    """Frame 0 (3 atoms, stiff and close to its minimum) converges long before frame 1 (5 atoms, soft, far)."""
    rng = np.random.RandomState(11)
    x_min = rng.uniform(0.0, 4.0, (8, 3))
    k = np.concatenate([np.full((3, 3), 5.0), np.tile([0.5, 3.0, 12.0], (5, 1))])
    x0 = x_min + np.concatenate([rng.normal(0.0, 0.01, (3, 3)), rng.normal(0.0, 0.4, (5, 3))])
    return _bowl(k, x_min, [3, 5]), x_min, x0, [3, 5]


def test_converges_on_an_anisotropic_bowl():
    force, x_min, x0 = _one_frame()
    out = rr.run(force, rr.new_state(x0), 2000, 1e-6)
    assert out["converged"].all() and 10 < out["steps"][0] < 2000
    assert out["fmax"][0] < 1e-6 and np.abs(out["x"] - x_min).max() < 1e-5
    assert out["energy"][0] < force(x0)[0][0]
    branches = {e.get("branch") for e in rr.flat_log(out)}
    assert {"first", "mix", "reset"} <= branches    # the bowl is steep enough to overshoot


def test_bounds_hold_at_every_step():
    force, _, x0 = _one_frame()
    for params in (dict(), dict(maxstep=0.02, dt=0.3), dict(dtmax=0.25, nmin=0)):
        out = rr.run(force, rr.new_state(x0, **params), 300, 1e-8)
        p = out["state"]["params"]
        log = rr.flat_log(out)
        steps = [e for e in log if "branch" in e]
        assert len(steps) == out["steps"][0] > 20
        assert steps[0]["branch"] == "first" and all(e["branch"] != "first" for e in steps[1:])
        for e in steps:
            assert e["dt"] <= p["dtmax"]
            assert e["dr_applied"] <= p["maxstep"] * (1 + 1e-15)   # the displacement that was added to x
            assert e["clamped"] == (e["dr"] > p["maxstep"])
        assert any(e["clamped"] for e in steps) or "maxstep" not in params


def test_split_run_equals_whole_run():
    force, _, x0 = _one_frame()
    whole = rr.run(force, rr.new_state(x0), 20, 1e-12)
    first = rr.run(force, rr.new_state(x0), 7, 1e-12)
    second = rr.run(force, first["state"], 13, 1e-12)
    assert first["steps"][0] == 7 and second["steps"][0] == 13 and whole["steps"][0] == 20
    for key in ("x", "v", "dt", "a", "npos", "energy", "fmax"):
        assert np.array_equal(second[key], whole[key]), key


def test_fixed_atoms():
    force, x_min, x0 = _one_frame()
    fixed = np.zeros(6, dtype=bool)
    fixed[[1, 4]] = True
    out = rr.run(force, rr.new_state(x0), 2000, 1e-6, fixed=fixed)
    assert out["converged"].all()
    assert np.array_equal(out["x"][fixed], x0[fixed]) and not out["v"][fixed].any()
    assert np.abs(out["x"][~fixed] - x_min[~fixed]).max() < 1e-5
    # the fixed atoms still feel a force far above fmax: it does not count
    assert np.sqrt((force(out["x"])[1][fixed] ** 2).sum(axis=1)).min() > 1e-2
    # all atoms fixed: converged at once, nothing moves
    none = rr.run(force, rr.new_state(x0), 10, 1e-6, fixed=np.ones(6, dtype=bool))
    assert none["converged"].all() and none["steps"][0] == 0 and np.array_equal(none["x"], x0)


def test_early_frame_freezes_while_the_other_goes_on():
    force, x_min, x0, natoms = _two_frames()
    out = rr.run(force, rr.new_state(x0, natoms), 3000, 1e-4)
    assert out["converged"].all() and 0 < out["steps"][0] < out["steps"][1]
    k0 = int(out["steps"][0])
    at_k0 = rr.run(force, rr.new_state(x0, natoms), k0, 1e-4)
    assert at_k0["converged"][0] and not at_k0["converged"][1]
    assert np.array_equal(at_k0["x"][:3], out["x"][:3])          # frame 0 did not move after it converged
    assert np.abs(at_k0["x"][3:] - out["x"][3:]).max() > 1e-3   # frame 1 did
    # each frame as when relaxed alone
    for f, s in enumerate((slice(0, 3), slice(3, 8))):
        def alone_force(x, s=s, f=f):
            full = out["x"].copy()
            full[s] = x
            e, g = force(full)
            return e[f:f + 1], g[s]
        alone = rr.run(alone_force, rr.new_state(x0[s]), 3000, 1e-4)
        assert alone["steps"][0] == out["steps"][f] and np.array_equal(alone["x"], out["x"][s])
    # a smaller fmax wakes the frozen frame, with its state carried on
    again = rr.run(force, out["state"], 3000, 1e-7)
    assert again["converged"].all() and again["steps"][0] > 0 and again["fmax"].max() < 1e-7


def test_device_fire_refuses_bad_arguments_without_a_device():
    from tensoralloy_amd import Atoms, DeviceFIRE

    class NoDevice:   # stands where an Engine would: touching it is a failure
        def __getattr__(self, name):
            if name == "_engine":
                raise AttributeError(name)
            raise AssertionError(f"the device was reached ({name})")

    atoms = Atoms(symbols=["Ni", "Ni"], positions=[[0, 0, 0], [2.0, 0, 0]], cell=np.diag([8.0] * 3), pbc=True)
    bad = [dict(dt=0.0), dict(dt=float("nan")), dict(dtmax=-1.0), dict(dtmax=float("inf")), dict(maxstep=0.0),
           dict(finc=0.9), dict(fdec=0.0), dict(fdec=1.0), dict(fa=1.0), dict(fa=-0.1), dict(astart=0.0),
           dict(astart=1.5), dict(Nmin=-1), dict(Nmin=2.5)]
    for kw in bad:
        name = next(iter(kw))
        with pytest.raises(ValueError, match=name):
            DeviceFIRE(NoDevice(), atoms, **kw)
    with pytest.raises(ValueError, match="at least one structure"):
        DeviceFIRE(NoDevice(), [])
    with pytest.raises(ValueError, match="fixed"):
        DeviceFIRE(NoDevice(), atoms, fixed=[True, False, True])
    with pytest.raises(ValueError, match="fixed"):
        DeviceFIRE(NoDevice(), atoms, fixed=[2])
    with pytest.raises(ValueError, match="fixed"):
        DeviceFIRE(NoDevice(), atoms, fixed=[0.5])
    with pytest.raises(ValueError, match="Engine or a TensorAlloyCalculator"):
        DeviceFIRE(object(), atoms)


def test_new_entries_are_exported():
    from tensoralloy_amd import _lib
    import tensoralloy_amd
    for name in ("ta_relax_init", "ta_relax_run", "ta_relax_get_state"):
        assert name in _lib.EXPORTED_SYMBOLS
    assert "ta_relax.hip" in _lib.SOURCES
    assert "DeviceFIRE" in tensoralloy_amd.__all__
    for name in ("relax_init", "relax_run", "relax_state"):
        assert callable(getattr(tensoralloy_amd.Engine, name))
