"""CPU: the NumPy reference of the Berendsen barostat (tests/md_npt_reference.py) on an ideal gas, where the
scheme has a closed form, and the argument refusals of `DeviceMD` that need no device.

Ideal gas: F = 0, W = 0, so the velocities never change, P_c = sum m v_c^2 / V, P = 2 KE / (3 V), and with the
isotropic barostat the volume follows V <- mu^3 V with mu = 1 - (dt / taup) (beta / 3) (P0 - 2 KE / (3 V))."""
import numpy as np
import pytest

from tests import md_npt_reference as npt
from tensoralloy_amd import md

DT = md.fs


def _gas(n=20, seed=5, L=12.0):
    rng = np.random.RandomState(seed)
    m = rng.uniform(10.0, 60.0, n)
    x = rng.uniform(0.0, L, (n, 3))
    v = md.maxwell_boltzmann(m, md.kB * 500.0, rng)
    return x, v, m, np.diag([L, 1.1 * L, 0.9 * L])


def _free(x, cells):
    return np.zeros(len(cells)), np.zeros_like(x), np.zeros((len(cells), 3, 3))


def test_units():
    assert md.GPa == 1.0 / 160.21766208
    assert abs(md.bar / md.GPa - 1e-4) < 1e-19


def test_ideal_gas_volume_recurrence():
    x, v, m, h = _gas()
    p0, taup, beta, n = 2.0 * md.GPa, 15 * DT, 40.0, 25
    r = npt.run(_free, x, v, m, [h], DT, n, p0, taup, beta)
    ke = 0.5 * (m[:, None] * v * v).sum()
    assert np.array_equal(r["v"], v)                      # no force, no thermostat: not touched
    assert np.all(r["ekin"] == r["ekin"][0]) and abs(r["ekin"][0, 0] - ke) < 1e-12 * ke
    V = abs(np.linalg.det(h))
    for k in range(n):
        assert abs(r["volume"][k, 0] - V) < 1e-12 * V
        P = 2.0 * ke / (3.0 * V)
        assert abs(r["press"][k, 0].mean() - P) < 1e-12 * P
        mu = 1.0 - DT / taup * beta / 3.0 * (p0 - P)
        assert np.abs(r["mu"][k, 0] - mu).max() < 1e-15
        V = mu ** 3 * V
    assert abs(r["volume"][n, 0] - V) < 1e-12 * V
    assert V < 0.999 * abs(np.linalg.det(h))              # the gas is below the target pressure: it was compressed
    # positions: x_n = prod(mu) x_0 + dt v sum_k prod_{j > k} mu_j
    mus = r["mu"][:, 0, 0]
    tail = np.array([np.prod(mus[k + 1:]) for k in range(n)])
    assert np.abs(r["x"] - (np.prod(mus) * x + DT * v * tail.sum())).max() < 1e-10
    assert np.abs(r["cells"][0] - np.prod(mus) * h).max() < 1e-12


def test_masked_axis_stays_bit_identical():
    x, v, m, h = _gas(seed=7)
    h = h + np.array([[0, 0, 0], [0.3, 0, 0], [0.2, -0.4, 0]])   # triclinic: rows with x and y components
    r = npt.run(_free, x, v, m, [h], DT, 30, 1.0 * md.GPa, 10 * DT, 30.0, mask=(1, 0, 1))
    assert np.array_equal(r["cells"][0][:, 1], h[:, 1])
    assert np.all(r["mu"][:, 0, 1] == 1.0)
    assert np.all(r["mu"][:, 0, 0] != 1.0) and np.all(r["mu"][:, 0, 2] != 1.0)
    assert np.all(r["mu"][:, 0, 0] != r["mu"][:, 0, 2])      # each free axis follows its own pressure
    # with no force the y coordinates are those of plain drift, to the bit
    y = x[:, 1].copy()
    for _ in range(30):
        y = y + DT * v[:, 1]
    assert np.array_equal(r["x"][:, 1], y)


def test_strain_aware_rebuild_count():
    """An ideal gas far below the target pressure: the strain alone uses the skin up. With rc + skin = 6.3 and
    skin = 0.3 the limit reaches 0 when |s - 1|_2 = 0.3 / 6.3; cold atoms (no drift to speak of) get there first
    through |u| >= lim."""
    x, v, m, h = _gas(seed=9)
    v = 1e-6 * v
    r = npt.run(_free, x, v, m, [h], DT, 60, 50.0 * md.GPa, 10 * DT, 1.0, skin=0.3, rc=6.0)
    npt.assert_not_marginal(r, 0.3)
    assert r["n_rebuilds"] >= 2
    first = r["rebuild_steps"][0]
    rec = r["log"][first - 1]
    assert rec["step"] == first and rec["lim"][0] <= rec["umax"][0] < 1e-3   # stale, and not by |u| against skin / 2
    assert r["log"][first - 2]["lim"][0] > r["log"][first - 2]["umax"][0]    # ... and not a step earlier
    assert r["end_rebuild"] == (r["rebuild_steps"][-1] != 60)


def test_device_md_refusals_without_a_device():
    from tensoralloy_amd import DeviceMD
    args = (object(), [object()], DT)
    with pytest.raises(ValueError, match="needs pressure, taup and compressibility"):
        DeviceMD(*args, pressure=0.0)
    with pytest.raises(ValueError, match="needs pressure, taup and compressibility"):
        DeviceMD(*args, pressure=0.0, taup=1.0)
    with pytest.raises(ValueError, match="pressure must be finite"):
        DeviceMD(*args, pressure=float("nan"), taup=1.0, compressibility=1.0)
    with pytest.raises(ValueError, match="taup must be a finite time > 0"):
        DeviceMD(*args, pressure=0.0, taup=0.0, compressibility=1.0)
    with pytest.raises(ValueError, match="taup must be a finite time > 0"):
        DeviceMD(*args, pressure=0.0, taup=float("inf"), compressibility=1.0)
    with pytest.raises(ValueError, match="compressibility must be finite and >= 0"):
        DeviceMD(*args, pressure=0.0, taup=1.0, compressibility=-1.0)
    with pytest.raises(ValueError, match="mask must have three flags"):
        DeviceMD(*args, pressure=0.0, taup=1.0, compressibility=1.0, mask=(0, 0, 0))
    with pytest.raises(ValueError, match="mask must have three flags"):
        DeviceMD(*args, pressure=0.0, taup=1.0, compressibility=1.0, mask=(1, 1))
    with pytest.raises(ValueError, match="mask belongs to the barostat"):
        DeviceMD(*args, mask=(1, 1, 1))
