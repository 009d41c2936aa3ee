"""CPU: the heat current and pressure tensor of the device MD loop: the self-checks of the finite-difference
reference (tests/md_flux_reference.py), which show that a case's bound is small before the GPU is asked, the helpers of
`tensoralloy_amd.md` (`heat_current_acf`, `pressure_acf`, `green_kubo_thermal_conductivity`, `green_kubo_viscosity`),
the argument checks of `DeviceMD` and the C ABI of `ta_md_set_flux` / `ta_md_get_flux` / `ta_md_get_flux_rows`."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from tests import md_flux_reference as ref
from tests.helpers import fcc, make_nn
from tensoralloy_amd import Atoms, md


@functools.lru_cache(maxsize=None)
def _ni():
    """32 Ni atoms, a = 3.524, jitter 0.08, G2 + G4 with rcut = acut = 3.0: every cell height exceeds twice the cutoff."""
    nn = make_nn(["Ni"], 3.0, True, [16, 16], acut=3.0)
    atoms = fcc(rep=(2, 2, 2), jitter=0.08, seed=3)
    rng = np.random.RandomState(5)
    m = np.full(32, 58.6934)
    v = md.maxwell_boltzmann(m, md.kB * 600.0, rng)
    return nn, atoms, v, m


@functools.lru_cache(maxsize=None)
def _ni_row():
    nn, atoms, v, m = _ni()
    return ref.row_from_matrix(ref.oracle_for(nn, atoms), atoms.positions, v, m, np.asarray(atoms.get_cell(complete=True)),
                               atoms.pbc)


def test_reference_matrix_gives_the_oracles_forces_and_virial():
    out = _ni_row()
    print("matrix against the analytic forces:", out["force_gap"], " W against the oracle's virial:", out["virial_gap"],
          " |J_pot|:", np.linalg.norm(out["row"][3:6]), " largest fd bound:", out["fd"].max())
    assert out["force_gap"] < 1e-10 and out["virial_gap"] < 1e-9
    assert np.linalg.norm(out["row"][3:6]) > 1e-3 and np.abs(out["row"][12:18]).max() > 1e-2
    # the bound of a comparison is small against the numbers it bounds
    assert out["fd"].max() < 1e-8 and np.all(out["fd"][3:6] < 1e-6 * out["terms"][3:6])
    assert np.all(out["fd"][[0, 1, 2, 6, 7, 8, 9, 10, 11]] == 0.0)   # the per-atom parts have no finite difference


def test_reference_cluster_identity_agrees_with_the_full_matrix():
    """A free cluster: the identity with one directional derivative against the full matrix."""
    nn, atoms, v, m = _ni()
    keep = np.argsort(np.linalg.norm(atoms.positions - atoms.positions.mean(axis=0), axis=1))[:13]
    cluster = Atoms(symbols=["Ni"] * 13, positions=atoms.positions[keep], cell=np.eye(3) * 30.0, pbc=False)
    evaluate = ref.oracle_for(nn, cluster)
    full = ref.row_from_matrix(evaluate, cluster.positions, v[keep], m[keep], np.eye(3) * 30.0, cluster.pbc)
    short = ref.cluster_row(evaluate, cluster.positions, v[keep], m[keep])
    gap = np.abs(full["row"] - short["row"])
    print("identity against the matrix:", gap.max(), " bounds:", (full["fd"] + short["fd"]).max())
    assert np.all(gap <= full["fd"] + short["fd"] + 2.0 ** -53 * 400 * full["terms"]) and gap.max() < 1e-9
    assert np.linalg.norm(short["row"][3:6]) > 1e-4


def test_reference_rows_in_closed_form():
    """Two atoms bound by a pair energy e_0 = e_1 = k r^2 / 2: de_j/dr_i is k (r_i - r_other) for both j."""
    k = 0.7
    x = np.array([[0.0, 0.0, 0.0], [1.5, 0.4, -0.3]])
    v = np.array([[0.2, -0.1, 0.05], [-0.3, 0.25, 0.1]])
    m = np.array([2.0, 3.0])

    def evaluate(y):
        d = y[1] - y[0]
        e = 0.5 * k * (d @ d)
        f = 2.0 * k * d   # the total energy is k r^2
        return dict(atomic=np.array([e, e]), forces=np.array([f, -f]), virial=np.outer(d, f))

    out = ref.row_from_matrix(evaluate, x, v, m, np.eye(3), [False] * 3)
    d = x[1] - x[0]
    # J_pot = d_10 (de_1/dr_0 . v_0) + d_01 (de_0/dr_1 . v_1) = d (-k d . v_0) - d (k d . v_1)
    want = -k * d * (d @ v[0]) - k * d * (d @ v[1])
    assert np.abs(out["row"][3:6] - want).max() < 1e-12
    e = 0.5 * k * (d @ d)
    assert np.abs(out["row"][0:3] - sum((0.5 * m[i] * v[i] @ v[i] + e) * v[i] for i in range(2))).max() < 1e-15
    assert out["row"][6] == pytest.approx(m[0] * v[0, 0] ** 2 + m[1] * v[1, 0] ** 2, rel=1e-15)
    assert out["row"][9] == pytest.approx(m[0] * v[0, 1] * v[0, 2] + m[1] * v[1, 1] * v[1, 2], rel=1e-15)
    w = 2.0 * k * np.outer(d, d)   # W = sum_p D_p (x) g_p
    assert np.abs(out["row"][12:18] - ref._six(w)).max() < 1e-12 and out["virial_gap"] < 1e-12 and out["force_gap"] < 1e-12
    short = ref.cluster_row(evaluate, x, v, m)
    assert np.abs(short["row"] - out["row"]).max() < 1e-12


def test_reference_accumulators():
    rng = np.random.RandomState(2)
    rows = rng.standard_normal((5, 2, 18))
    sums, a_heat, a_press, t_heat, t_press = ref.accumulate(rows, 3)
    j, p = rows[..., 0:3] + rows[..., 3:6], rows[..., 6:12] - rows[..., 12:18]
    assert np.abs(sums - rows.sum(axis=0)).max() < 1e-14
    assert np.abs(a_heat[:, 0] - (j * j).sum(axis=0)).max() < 1e-13
    assert np.abs(a_press[1, 2] - (p[2:, 1] * p[:-2, 1]).sum(axis=0)).max() < 1e-13
    assert np.all(t_heat >= np.abs(a_heat)) and np.all(t_press >= np.abs(a_press))


def test_acf_normalisation():
    a_heat = np.arange(24, dtype=np.float64).reshape(1, 4, 6)[..., :3] + 1.0
    c = md.heat_current_acf(a_heat, 3)
    assert c.shape == (1, 3, 4)
    assert np.array_equal(c[0, :, 0], a_heat[0, 0] / 3.0) and np.array_equal(c[0, :, 2], a_heat[0, 2] / 1.0)
    assert np.all(np.isnan(c[0, :, 3]))   # lag 3 of three samples has no time origin
    sums = np.zeros((1, 18))
    sums[0, 6:12], sums[0, 12:18] = 9.0 * np.arange(1, 7), 3.0 * np.arange(1, 7)   # mean Pi = 2 (1 .. 6)
    a_press = np.full((1, 4, 6), 30.0)
    p = md.pressure_acf(a_press, sums, 3)
    assert p.shape == (1, 6, 4)
    assert np.array_equal(p[0, :, 0], 10.0 - (2.0 * np.arange(1, 7)) ** 2) and np.all(np.isnan(p[0, :, 3]))
    assert np.array_equal(md.pressure_acf(a_press[0], sums[0], 3), p[0], equal_nan=True)
    with pytest.raises(ValueError, match="pressure_acf"):
        md.pressure_acf(a_press, sums[:, :17], 3)


# CODATA 2014, the set behind the package's `fs`, `kB` and `GPa`
E_CHARGE, AMU, K_BOLTZMANN = 1.6021766208e-19, 1.660539040e-27, 1.38064852e-23


def test_green_kubo_integrals_of_an_exponential():
    """<J J>(t) = c0 exp(-t / tau): the integral is c0 tau (1 - exp(-t / tau)); the unit factors from the constants."""
    t_ase = 1.0e-10 * np.sqrt(AMU / E_CHARGE)   # one ASE time unit in seconds
    assert md.fs == pytest.approx(1.0e-15 / t_ase, rel=1e-9) and md.kB == pytest.approx(K_BOLTZMANN / E_CHARGE, rel=1e-9)
    L, dt, tau = 4001, 0.5 * md.fs, 80.0 * md.fs
    t = np.arange(L) * dt
    volume, T = 1234.5, 700.0
    c0 = np.array([2.0, 3.0, 0.5])
    acf = c0[:, None] * np.exp(-t / tau)[None, :]
    kappa = md.green_kubo_thermal_conductivity(acf, volume, T, dt)
    assert kappa.shape == (3, L) and np.all(kappa[:, 0] == 0.0)
    # eV^2 A^2 / t_ase / (A^3 eV/K K^2) = eV / (A t_ase K)
    want = c0 * tau * (1.0 - np.exp(-t[-1] / tau)) / (volume * md.kB * T * T) * E_CHARGE / (1.0e-10 * t_ase)
    assert np.allclose(kappa[:, -1], want, rtol=1e-5, atol=0.0)   # (the trapezoidal rule: (dt / tau)^2 / 12)
    mid = L // 7
    assert np.allclose(kappa[:, mid], want * (1.0 - np.exp(-t[mid] / tau)) / (1.0 - np.exp(-t[-1] / tau)), rtol=1e-5)
    acf6 = np.concatenate([np.zeros((3, L)), acf])
    eta = md.green_kubo_viscosity(acf6, volume, T, dt)
    # eV^2 t_ase / (A^3 eV) = eV t_ase / A^3, in mPa s
    want = c0 * tau * (1.0 - np.exp(-t[-1] / tau)) / (volume * md.kB * T) * E_CHARGE / 1.0e-30 * t_ase * 1.0e3
    assert eta.shape == (3, L) and np.allclose(eta[:, -1], want, rtol=1e-5, atol=0.0)
    # leading axes and one volume per frame
    k2 = md.green_kubo_thermal_conductivity(np.stack([acf, 2.0 * acf]), [volume, 2.0 * volume], T, dt)
    assert k2.shape == (2, 3, L) and np.allclose(k2[0], kappa, rtol=1e-15) and np.allclose(k2[1], kappa, rtol=1e-14)
    for bad in (dict(volume=0.0), dict(temperature_K=-1.0), dict(dt_sample=0.0)):
        kw = dict(acf=acf, volume=volume, temperature_K=T, dt_sample=dt)
        kw.update(bad)
        with pytest.raises(ValueError, match="green_kubo_thermal_conductivity"):
            md.green_kubo_thermal_conductivity(**kw)
    with pytest.raises(ValueError, match=r"acf must be \[..., 6, n_lags\]"):
        md.green_kubo_viscosity(acf, volume, T, dt)


def test_helpers_are_exported():
    for name in ("heat_current_acf", "pressure_acf", "green_kubo_thermal_conductivity", "green_kubo_viscosity"):
        assert name in md.__all__ and callable(getattr(md, name))


def test_device_md_argument_errors_and_opt_in():
    atoms = fcc(rep=(1, 1, 1))
    calls = []

    class Reached(Exception):
        pass

    class Old:   # the engine as it was before this sampler
        def _ok(self, *a, **k):
            return None
        set_frames = md_init = md_set_thermostat = md_set_langevin = md_set_nose_hoover = md_set_barostat = _ok
        md_set_sampling = _ok

        def md_run(self, n, dt, **k):
            raise Reached("md_run")

    class New(Old):
        def md_set_flux(self, *a):
            calls.append(a)
            raise Reached("md_set_flux")

    for bad in (0, -1, 4097, 2.5, True):
        with pytest.raises(ValueError, match="flux_lags must be"):
            md.DeviceMD(New(), atoms, md.fs, flux_lags=bad)
    for bad in (0, -3, 1.5, False):
        with pytest.raises(ValueError, match="flux_every must be"):
            md.DeviceMD(New(), atoms, md.fs, flux_lags=4, flux_every=bad)
    with pytest.raises(ValueError, match="flux_every belongs to"):
        md.DeviceMD(New(), atoms, md.fs, flux_every=2)
    with pytest.raises(ValueError, match=r"flux_lags \(heat current and pressure tensor\) excludes the barostat"):
        md.DeviceMD(New(), atoms, md.fs, flux_lags=4, pressure=0.0, taup=100 * md.fs, compressibility=1.0)
    with pytest.raises(Reached, match="md_set_flux"):
        md.DeviceMD(New(), atoms, md.fs, flux_lags=16, flux_every=3)
    assert calls == [(16, 3)]
    with pytest.raises(Reached, match="md_run"):   # nothing new is called when flux_lags is None
        md.DeviceMD(Old(), atoms, md.fs)
    with pytest.raises(Reached, match="md_run"):
        md.DeviceMD(New(), atoms, md.fs, n_lags=8)
    assert len(calls) == 1

    class LeftOn(New):   # an engine on which an earlier DeviceMD left the sampler on says so ...
        md_flux_lags = 64

    with pytest.raises(Reached, match="md_set_flux"):   # ... and is told to switch it off: the one deliberate call
        md.DeviceMD(LeftOn(), atoms, md.fs)
    assert calls[1] == (0,)


def test_abi_of_the_flux_calls(lib):
    from tensoralloy_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "tensoralloy_amd.h")) as fp:
        header = re.sub(r"/\*.*?\*/", "", fp.read(), flags=re.S)
    for name in ("ta_md_set_flux", "ta_md_get_flux", "ta_md_get_flux_rows"):
        assert re.search(r"\bint %s\s*\(ta_handle h," % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert re.search(r"^#define TA_MD_FLUX_ROW 18$", header, re.M) and _lib.TA_MD_FLUX_ROW == 18
    assert re.search(r"^#define TA_ABI_VERSION 5$", header, re.M) and _lib.TA_ABI_VERSION == 5
    assert lib.ta_abi_version() == 5
    struct = re.search(r"typedef struct \{([^}]*)\} ta_md_flux_params;", header).group(1)
    names = ["n_lags", "sample_every"]
    assert re.findall(r"\bint32_t\s+(\w+);", struct) == names
    assert C.sizeof(_lib.MdFluxParams) == 8 and [f[0] for f in _lib.MdFluxParams._fields_] == names
    assert "ta_md_flux.hip" in _lib.SOURCES


def test_sampler_text():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "tensoralloy_amd", "csrc", "ta_sampler_text.h")) as fp:
        text = fp.read()
    assert re.search(r'constexpr MdSamplerText flux = \{"ta_md_set_flux", "the heat current and pressure tensor are off"', text)
