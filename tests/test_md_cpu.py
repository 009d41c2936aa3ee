"""CPU: the NumPy reference of the device MD loop (tests/md_reference.py), the Maxwell-Boltzmann sampler,
the unit constants and the argument checks of `DeviceMD` that need no device."""
import numpy as np
import pytest

from tests import md_reference
from tensoralloy_amd import md


def _oscillator(k=2.5):
    """Three independent harmonic oscillators (one atom, x / y / z) with spring constant k."""
    def force(x):
        return np.array([0.5 * k * (x * x).sum()]), -k * x
    return force


def test_reference_is_time_reversible():
    force = _oscillator()
    x0, v0, m = np.array([[0.3, -0.2, 0.1]]), np.array([[0.05, 0.4, -0.3]]), np.array([1.7])
    fwd = md_reference.run(force, x0, v0, m, 0.05, 200)
    back = md_reference.run(force, fwd["x"], -fwd["v"], m, 0.05, 200)
    assert np.abs(back["x"] - x0).max() < 1e-12
    assert np.abs(back["v"] + v0).max() < 1e-12


def test_reference_energy_error_scales_with_dt_squared():
    force = _oscillator()
    x0, v0, m = np.array([[0.3, -0.2, 0.1]]), np.array([[0.05, 0.4, -0.3]]), np.array([1.7])
    err = []
    for dt in (0.04, 0.02, 0.01):
        r = md_reference.run(force, x0, v0, m, dt, int(round(4.0 / dt)))
        e = (r["epot"] + r["ekin"])[:, 0]
        err.append(np.abs(e - e[0]).max())
    # velocity Verlet: the energy error is O(dt^2), so halving dt divides it by 4 (up to O(dt^4))
    assert 3.8 < err[0] / err[1] < 4.2 and 3.8 < err[1] / err[2] < 4.2, err


def test_reference_counts_rebuilds_by_the_half_skin_rule():
    force = lambda x: (np.zeros(1), np.zeros_like(x))          # free flight along x at speed 1
    x0, v0, m = np.zeros((1, 3)), np.array([[1.0, 0.0, 0.0]]), np.ones(1)
    r = md_reference.run(force, x0, v0, m, 0.1, 10, skin=0.5)  # 0.25 is passed after steps 3, 6 and 9
    assert r["rebuild_steps"] == [3, 6, 9] and r["n_rebuilds"] == 3
    assert md_reference.run(force, x0, v0, m, 0.1, 5, skin=0.0)["n_rebuilds"] == 5
    assert md_reference.run(force, x0, v0, m, 0.1, 5)["n_rebuilds"] == 0


def test_reference_berendsen_moves_towards_the_target():
    force = lambda x: (np.zeros(1), np.zeros_like(x))
    rng = np.random.RandomState(0)
    m = np.full(50, 58.6934)
    v0 = md.maxwell_boltzmann(m, md.kB * 300.0, rng)
    r = md_reference.run(force, np.zeros((50, 3)), v0, m, md.fs, 200, kT0=md.kB * 600.0, tau=20 * md.fs)
    T = 2.0 * r["ekin"][:, 0] / (3 * 50 * md.kB)
    assert np.all(np.diff(T) > 0.0) and abs(T[-1] - 600.0) < 1.0
    # the factor is clamped to [0.9, 1.1]
    assert md_reference.berendsen_factors(np.array([1e-9]), [50], 1.0, 1.0, 1.0)[0] == 1.1
    assert md_reference.berendsen_factors(np.array([0.0]), [50], 1.0, 1.0, 1.0)[0] == 1.0


def test_maxwell_boltzmann_moments():
    rng = np.random.RandomState(7)
    m = np.tile([58.6934, 95.95], 50000)        # 10^5 atoms
    kT = md.kB * 700.0
    v = md.maxwell_boltzmann(m, kT, rng)
    assert np.abs((m[:, None] * v).sum(axis=0)).max() < 1e-9 * np.abs(m[:, None] * v).sum()
    mv2 = (m[:, None] * v * v).mean()           # <m v_c^2> = kT for every component
    assert abs(mv2 / kT - 1.0) < 0.02
    for sel in (slice(0, None, 2), slice(1, None, 2)):   # ... and for each species
        assert abs((m[sel, None] * v[sel] ** 2).mean() / kT - 1.0) < 0.02
    raw = md.maxwell_boltzmann(m[:10], kT, np.random.RandomState(1), zero_momentum=False)
    assert np.abs((m[:10, None] * raw).sum(axis=0)).max() > 0.0
    with pytest.raises(ValueError):
        md.maxwell_boltzmann([1.0, 0.0], kT, rng)
    with pytest.raises(ValueError):
        md.maxwell_boltzmann([1.0], -1.0, rng)


def test_unit_constants():
    # CODATA 2014, as ASE: eV = e, amu, kB in J / K
    e, amu, k = 1.6021766208e-19, 1.660539040e-27, 1.38064852e-23
    assert md.fs == pytest.approx(1e-15 / (1e-10 * np.sqrt(amu / e)), rel=1e-12)
    assert md.kB == pytest.approx(k / e, rel=1e-12)
    assert md.fs == 0.09822694788464063 and md.kB == 8.617330337217213e-05
    import tensoralloy_amd
    assert tensoralloy_amd.DeviceMD is md.DeviceMD and tensoralloy_amd.maxwell_boltzmann is md.maxwell_boltzmann


def test_device_md_argument_errors():
    from tests.helpers import fcc
    atoms = fcc(rep=(1, 1, 1))

    class NoEngine:
        pass

    class Recorder:  # stands in for an engine: anything it is asked to do is a failure of the checks
        def md_run(self, *a, **k):
            raise AssertionError("reached the engine")
        set_frames = md_init = md_set_thermostat = md_run

    with pytest.raises(ValueError, match="timestep"):
        md.DeviceMD(Recorder(), atoms, 0.0)
    with pytest.raises(ValueError, match="timestep"):
        md.DeviceMD(Recorder(), atoms, float("nan"))
    with pytest.raises(ValueError, match="both"):
        md.DeviceMD(Recorder(), atoms, md.fs, temperature_K=300.0)
    with pytest.raises(ValueError, match="both"):
        md.DeviceMD(Recorder(), atoms, md.fs, taut=10 * md.fs)
    with pytest.raises(ValueError, match="> 0"):
        md.DeviceMD(Recorder(), atoms, md.fs, temperature_K=-1.0, taut=10 * md.fs)
    with pytest.raises(ValueError, match="at least one"):
        md.DeviceMD(Recorder(), [], md.fs)
    with pytest.raises(ValueError, match="Engine"):
        md.DeviceMD(NoEngine(), atoms, md.fs)
    with pytest.raises(ValueError, match="velocities"):
        md.DeviceMD(Recorder(), atoms, md.fs, velocities=np.zeros((3, 3)))
    with pytest.raises(ValueError, match="mass"):
        md.DeviceMD(Recorder(), atoms, md.fs, masses=np.ones(3))
