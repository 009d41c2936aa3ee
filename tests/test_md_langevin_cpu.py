"""CPU: the NumPy reference of the Langevin step (tests/md_langevin_reference.py) -- the Philox4x32-10 known
answers, the moments of the normals, the zero-friction limit, fluctuation-dissipation -- and the argument
checks of `DeviceMD` that need no device."""
import numpy as np
import pytest

from tests import md_langevin_reference as lv
from tests import md_reference
from tests.test_md_cpu import _oscillator
from tensoralloy_amd import md

# counter, key, output: the Random123 known-answer vectors of philox4x32_10
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_known_answers():
    for counter, key, want in KNOWN_ANSWERS:
        got = lv.philox4x32_10(np.array(counter, dtype=np.uint64), key)
        assert got.dtype == np.uint32 and tuple(int(w) for w in got) == want
    # vectorised: the three counters of the last key at once give the same words as one by one
    batch = lv.philox4x32_10(np.array([k[0] for k in KNOWN_ANSWERS], dtype=np.uint64), KNOWN_ANSWERS[2][1])
    assert tuple(int(w) for w in batch[2]) == KNOWN_ANSWERS[2][2]


def test_moments_of_the_normals():
    """10^6 normals (atoms 0 .. 166666 x 3 components x {xi, eta} is 2 x 500001) at a step beyond 2^32, so
    that the high word of the step is in the counter. Bounds: five standard errors of the estimators."""
    n_atoms = 166667
    step = 2 ** 32 + 12345
    xi, eta = lv.normals(2024, step, n_atoms)
    assert xi.shape == eta.shape == (n_atoms, 3)
    z = np.concatenate([xi.ravel(), eta.ravel()])
    n = z.size
    assert n >= 10 ** 6
    mean, var, cross = z.mean(), z.var(), (xi * eta).mean()
    print("mean", mean, "var - 1", var - 1.0, "<xi eta>", cross, "max", np.abs(z).max())
    assert abs(mean) < 5.0 / np.sqrt(n)
    assert abs(var - 1.0) < 5.0 * np.sqrt(2.0 / n)
    assert abs(cross) < 5.0 / np.sqrt(n)
    assert np.all(np.isfinite(z)) and np.abs(z).max() <= np.sqrt(2.0 * 54 * np.log(2.0))
    # the high word matters, and so do the seed, the atom and the component
    assert not np.array_equal(xi[:100], lv.normals(2024, step - 2 ** 32, 100)[0])
    assert not np.array_equal(xi[:100], lv.normals(2025, step, 100)[0])
    assert np.array_equal(xi[40:100], lv.normals(2024, step, 60, first_atom=40)[0])
    assert len(np.unique(xi[:100])) == 300


def test_zero_friction_is_velocity_verlet():
    force = _oscillator()
    x0, v0, m = np.array([[0.3, -0.2, 0.1]]), np.array([[0.05, 0.4, -0.3]]), np.array([1.7])
    a = md_reference.run(force, x0, v0, m, 0.05, 200, skin=0.2)
    b = lv.run(force, x0, v0, m, 0.05, 200, kT0=0.3, friction=0.0, seed=9, skin=0.2)
    for k in ("x", "v", "epot", "ekin"):
        assert np.abs(a[k] - b[k]).max() <= 1e-14, k
    assert a["rebuild_steps"] == b["rebuild_steps"] and a["n_rebuilds"] >= 1


def test_fluctuation_dissipation():
    """512 free particles from rest in a bath of 900 K, friction 0.1 / fs, dt = 1 fs: the mean of
    2 KE / (3 N kB) over steps 200 .. 1200 is within 2 % of 900 K. v^2 decorrelates in 1 / (2 fr) = 5 steps:
    about 100 independent samples of 1536 components, standard error sqrt(2 / 1536) / 10 = 0.36 %, so 2 % is
    above five standard errors plus the scheme's O((fr dt)^2) = 1 % bias."""
    n = 512
    m = np.full(n, 58.6934)
    force = lambda x: (np.zeros(1), np.zeros_like(x))
    r = lv.run(force, np.zeros((n, 3)), np.zeros((n, 3)), m, md.fs, 1200, kT0=md.kB * 900.0,
               friction=0.1 / md.fs, seed=7)
    T = 2.0 * r["ekin"][:, 0] / (3 * n * md.kB)
    assert T.shape == (1201,) and T[0] == 0.0
    mean = T[200:].mean()
    print("mean temperature", mean)
    assert abs(mean / 900.0 - 1.0) < 0.02
    # the same seed gives the same trajectory, another one does not; a run cut in two is the whole run
    again = lv.run(force, np.zeros((n, 3)), np.zeros((n, 3)), m, md.fs, 50, kT0=md.kB * 900.0,
                   friction=0.1 / md.fs, seed=7)
    assert np.array_equal(again["ekin"], r["ekin"][:51])
    rest = lv.run(force, again["x"], again["v"], m, md.fs, 30, kT0=md.kB * 900.0, friction=0.1 / md.fs, seed=7,
                  first_step=50)
    assert np.array_equal(rest["ekin"], r["ekin"][50:81])
    other = lv.run(force, np.zeros((n, 3)), np.zeros((n, 3)), m, md.fs, 50, kT0=md.kB * 900.0,
                   friction=0.1 / md.fs, seed=8)
    assert not np.array_equal(other["ekin"], again["ekin"])


def test_damping_without_a_bath():
    """kT0 = 0 with friction > 0: no noise, the oscillator loses energy monotonically over a period."""
    force = _oscillator()
    x0, v0, m = np.array([[0.3, -0.2, 0.1]]), np.array([[0.05, 0.4, -0.3]]), np.array([1.7])
    r = lv.run(force, x0, v0, m, 0.05, 200, kT0=0.0, friction=0.5, seed=1)
    e = (r["epot"] + r["ekin"])[:, 0]
    assert np.all(np.diff(e) < 0.0) and e[-1] < 0.05 * e[0]


def test_device_md_argument_errors():
    from tests.helpers import fcc
    atoms = fcc(rep=(1, 1, 1))

    class Recorder:  # stands in for an engine: anything it is asked to do is a failure of the checks
        def md_run(self, *a, **k):
            raise AssertionError("reached the engine")
        set_frames = md_init = md_set_thermostat = md_set_langevin = md_noise = md_run

    with pytest.raises(ValueError, match="exclude"):
        md.DeviceMD(Recorder(), atoms, md.fs, temperature_K=300.0, taut=10 * md.fs, friction=0.01 / md.fs)
    with pytest.raises(ValueError, match="exclude"):
        md.DeviceMD(Recorder(), atoms, md.fs, taut=10 * md.fs, friction=0.01 / md.fs)
    with pytest.raises(ValueError, match="temperature_K"):
        md.DeviceMD(Recorder(), atoms, md.fs, friction=0.01 / md.fs)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="friction"):
            md.DeviceMD(Recorder(), atoms, md.fs, temperature_K=300.0, friction=bad)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature_K"):
            md.DeviceMD(Recorder(), atoms, md.fs, temperature_K=bad, friction=0.01 / md.fs)
    for bad in (-1, 2 ** 64):
        with pytest.raises(ValueError, match="seed"):
            md.DeviceMD(Recorder(), atoms, md.fs, temperature_K=300.0, friction=0.01 / md.fs, seed=bad)
    with pytest.raises(ValueError, match="both"):   # as before: a temperature alone selects nothing
        md.DeviceMD(Recorder(), atoms, md.fs, temperature_K=300.0)
    with pytest.raises(AssertionError, match="reached the engine"):   # a valid Langevin request gets through
        md.DeviceMD(Recorder(), atoms, md.fs, temperature_K=0.0, friction=0.01 / md.fs, seed=2 ** 64 - 1)
