"""CPU: the NumPy reference of the Nose-Hoover chain thermostat (tests/md_nhc_reference.py) against an
adaptive integration of the continuous equations of motion, its conserved quantity on the Ni oracle case of
tests/test_gpu_md.py, the ABI of the four new calls and the argument checks of `DeviceMD` that need no device.

The continuous equations (per frame; K the kinetic energy, G_k as in the reference's docstring):
    dx/dt = v,  dv/dt = F/m - veta_1 v,  deta_k/dt = veta_k,  dveta_k/dt = G_k - veta_{k+1} veta_k  (veta_{M+1} = 0)
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import md_nhc_reference as nhc
from tests import md_reference
from tensoralloy_amd import md

N_OSC = 8   # atoms: 24 harmonic oscillators
KT0, TAU, T_END = 0.4, 0.7, 2.0


def _oscillators():
    rng = np.random.RandomState(7)
    k = 1.0 + 2.0 * rng.rand(N_OSC, 3)
    m = 1.0 + rng.rand(N_OSC)
    x0 = 0.3 * rng.standard_normal((N_OSC, 3))
    v0 = 0.6 * rng.standard_normal((N_OSC, 3))

    def force(x):
        return np.array([0.5 * (k * x * x).sum()]), -k * x
    return force, k, m, x0, v0


def _exact(M):
    """The state (x, v, eta, veta) at T_END of the continuous equations, by DOP853 at rtol 1e-13."""
    from scipy.integrate import solve_ivp
    _, k, m, x0, v0 = _oscillators()
    n3, g = 3 * N_OSC, 3 * N_OSC
    Q = nhc.chain_masses(g, KT0, TAU, M)

    def rhs(t, y):
        x, v = y[:n3].reshape(-1, 3), y[n3:2 * n3].reshape(-1, 3)
        veta = y[2 * n3 + M:]
        K = 0.5 * (m[:, None] * v * v).sum()
        G = np.empty(M)
        G[0] = (2.0 * K - g * KT0) / Q[0]
        G[1:] = (Q[:-1] * veta[:-1] ** 2 - KT0) / Q[1:]
        dveta = G - np.append(veta[1:], 0.0) * veta
        return np.concatenate([v.ravel(), (-k * x / m[:, None] - veta[0] * v).ravel(), veta, dveta])
    y0 = np.concatenate([x0.ravel(), v0.ravel(), np.zeros(2 * M)])
    sol = solve_ivp(rhs, (0.0, T_END), y0, method="DOP853", rtol=1e-13, atol=1e-14)
    assert sol.success
    return sol.y[:, -1]


def _state(out):
    return np.concatenate([out["x"].ravel(), out["v"].ravel(), out["eta"].ravel(), out["veta"].ravel()])


@pytest.mark.parametrize("loops", [1, 3])
def test_second_order_against_the_continuous_equations(loops):
    force, _, m, x0, v0 = _oscillators()
    exact = _exact(3)
    errs = []
    for dt in (0.02, 0.01, 0.005):
        out = nhc.run(force, x0, v0, m, dt, int(round(T_END / dt)), KT0, TAU, chain=3, loops=loops)
        errs.append(np.abs(_state(out) - exact).max())
    ratios = [errs[0] / errs[1], errs[1] / errs[2]]
    print("end-state errors", errs, "ratios", ratios)
    assert errs[0] > 1e-8   # (the thermostat acted: the error is the scheme's, far above the solver's)
    for r in ratios:
        assert 3.5 <= r <= 4.5, (errs, ratios)


def test_chain_lengths_and_loops():
    """M = 1 and M = 8 run and conserve H' to O(dt^2); L = 4 differs from L = 1 by O(dt^2)."""
    force, _, m, x0, v0 = _oscillators()
    for M in (1, 8):
        exc = []
        for dt in (0.02, 0.01):
            out = nhc.run(force, x0, v0, m, dt, int(round(T_END / dt)), KT0, TAU, chain=M)
            assert out["eta"].shape == (1, M) and np.all(np.isfinite(_state(out)))
            H = (out["epot"] + out["ekin"] + out["echain"])[:, 0]
            exc.append(np.abs(H - H[0]).max())
        print("M", M, "excursions of H'", exc)
        assert 0.0 < exc[1] and 3.0 <= exc[0] / exc[1] <= 5.0, (M, exc)
        assert np.abs(out["v"] - md_reference.run(force, x0, v0, m, dt, int(round(T_END / dt)))["v"]).max() > 1e-3
    gaps = []
    for dt in (0.02, 0.01):
        one = nhc.run(force, x0, v0, m, dt, int(round(T_END / dt)), KT0, TAU, chain=3, loops=1)
        four = nhc.run(force, x0, v0, m, dt, int(round(T_END / dt)), KT0, TAU, chain=3, loops=4)
        gaps.append(np.abs(_state(one) - _state(four)).max())
    print("L = 4 against L = 1", gaps)
    assert gaps[1] > 0.0 and 3.5 <= gaps[0] / gaps[1] <= 4.5, gaps


def test_conserved_quantity_on_the_ni_case():
    """32 Ni atoms, Zjw04, 300 K start, 600 K target, tau = 20 fs, 40 steps of 1 fs with the CPU oracle: H'
    wanders at most 5 x what E does in the NVE reference run from the same start (2.6 x when this was written;
    a missing or mis-signed chain term shows as eV, the excursions are below a meV)."""
    from tests.helpers import fcc, make_eam, oracle_eam_eval
    from tensoralloy_amd.atoms import atomic_masses
    nn = make_eam(["Ni"], 6.0, potential="zjw04")
    atoms = fcc(rep=(2, 2, 2), jitter=0.02, seed=3)
    m = np.array([atomic_masses[z] for z in atoms.numbers], dtype=np.float64)
    v0 = md.maxwell_boltzmann(m, md.kB * 300.0, np.random.RandomState(3))

    def force(x):
        a = atoms.copy()
        a.positions[:] = x
        o = oracle_eam_eval(nn, a)
        return np.array([o["energy"]]), o["forces"]
    out = nhc.run(force, atoms.positions, v0, m, md.fs, 40, md.kB * 600.0, 20 * md.fs)
    nve = md_reference.run(force, atoms.positions, v0, m, md.fs, 40)
    H = (out["epot"] + out["ekin"] + out["echain"])[:, 0]
    E = (nve["epot"] + nve["ekin"])[:, 0]
    d_H, d_E = np.abs(H - H[0]).max(), np.abs(E - E[0]).max()
    print("excursion of H'", d_H, "of E (NVE)", d_E, "ratio", d_H / d_E)
    assert out["echain"][0, 0] == 0.0 and out["echain"][-1, 0] != 0.0   # (the chain starts at rest and acts)
    assert out["ekin"][-1, 0] > nve["ekin"][-1, 0]                        # ... towards the hotter target
    assert d_E > 0.0 and d_H <= 5.0 * d_E


def test_abi_of_the_chain_calls(lib):
    from tensoralloy_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "tensoralloy_amd.h")) as fp:
        header = re.sub(r"/\*.*?\*/", "", fp.read(), flags=re.S)
    for name in ("ta_md_set_nose_hoover", "ta_md_get_chain", "ta_md_set_chain", "ta_md_get_chain_records"):
        assert re.search(r"\bint %s\s*\(ta_handle h," % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert re.search(r"^#define TA_MD_MAX_CHAIN 8$", header, re.M) and _lib.TA_MD_MAX_CHAIN == 8
    assert re.search(r"^#define TA_ABI_VERSION 5$", header, re.M) and _lib.TA_ABI_VERSION == 5
    assert C.sizeof(_lib.MdNhcParams) == 32
    assert [f[0] for f in _lib.MdNhcParams._fields_] == ["kT0", "tau", "chain", "loops", "dof_removed"]
    assert _lib.MdNhcParams.tau.offset == 8 and _lib.MdNhcParams.chain.offset == 16
    assert _lib.MdNhcParams.dof_removed.offset == 24


def test_device_md_argument_errors():
    from tests.helpers import fcc
    atoms = fcc(rep=(1, 1, 1))

    class Recorder:  # stands in for an engine: anything it is asked to do is a failure of the checks
        def md_run(self, *a, **k):
            raise AssertionError("reached the engine")
        set_frames = md_init = md_set_thermostat = md_set_langevin = md_set_nose_hoover = md_run

    ok = dict(temperature_K=300.0, tdamp=20 * md.fs)
    with pytest.raises(ValueError, match="tdamp .* excludes"):
        md.DeviceMD(Recorder(), atoms, md.fs, taut=10 * md.fs, **ok)
    with pytest.raises(ValueError, match="tdamp .* excludes"):
        md.DeviceMD(Recorder(), atoms, md.fs, friction=0.01 / md.fs, **ok)
    with pytest.raises(ValueError, match="needs temperature_K with tdamp"):
        md.DeviceMD(Recorder(), atoms, md.fs, tdamp=20 * md.fs)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tdamp must be"):
            md.DeviceMD(Recorder(), atoms, md.fs, temperature_K=300.0, tdamp=bad)
        with pytest.raises(ValueError, match="temperature_K must be"):
            md.DeviceMD(Recorder(), atoms, md.fs, temperature_K=bad, tdamp=20 * md.fs)
    for bad in (0, 9):
        with pytest.raises(ValueError, match="tchain"):
            md.DeviceMD(Recorder(), atoms, md.fs, tchain=bad, **ok)
    for bad in (0, 17):
        with pytest.raises(ValueError, match="tloop"):
            md.DeviceMD(Recorder(), atoms, md.fs, tloop=bad, **ok)
    with pytest.raises(ValueError, match="dof_removed"):
        md.DeviceMD(Recorder(), atoms, md.fs, dof_removed=-1, **ok)
    # the messages of the argument combinations that existed before stay
    with pytest.raises(ValueError, match=r"taut \(Berendsen\) and friction \(Langevin\) exclude each other"):
        md.DeviceMD(Recorder(), atoms, md.fs, taut=10 * md.fs, friction=0.01 / md.fs, **ok)
    with pytest.raises(ValueError, match="the thermostat needs both temperature_K and taut"):
        md.DeviceMD(Recorder(), atoms, md.fs, temperature_K=300.0)
    with pytest.raises(AssertionError, match="reached the engine"):   # a valid request gets through
        md.DeviceMD(Recorder(), atoms, md.fs, tchain=8, tloop=16, dof_removed=3, **ok)
