"""CPU: the NumPy reference of the loop's time correlations (tests/md_corr_reference.py), the helpers that turn a
VACF or an MSD into a spectrum or a diffusion coefficient, the argument checks of `DeviceMD` that need no
device, and the ABI of the three new calls."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import md_corr_reference as corr
from tensoralloy_amd import md


def _hand_made():
    """Three samples of two frames: atoms 0 (element 0) and 1 (element 1), and atom 2 (element 0) alone."""
    xs = np.array([[[0, 0, 0], [1, 0, 0], [0, 0, 0]],
                   [[1, 0, 0], [1, 2, 0], [0, 0, 3]],
                   [[3, 0, 0], [1, 2, 2], [0, 4, 3]]], dtype=np.float64)
    vs = np.array([[[1, 0, 0], [0, 2, 0], [1, 1, 0]],
                   [[2, 0, 0], [0, 1, 0], [0, 1, 0]],
                   [[-1, 0, 0], [0, 0, 1], [2, 0, 0]]], dtype=np.float64)
    return xs, vs, [2, 1], [0, 1, 0]


def test_correlate_against_values_worked_out_by_hand():
    xs, vs, natoms, species = _hand_made()
    out = corr.correlate(xs, vs, natoms, species, 2, 2)
    # lag 0: |v|^2 summed over the three samples; lag 1: v(1).v(0) + v(2).v(1)
    assert np.array_equal(out["vacf_sum"], [[[6.0, 0.0], [6.0, 2.0]], [[7.0, 1.0], [0.0, 0.0]]])
    # lag 1: |x(1) - x(0)|^2 + |x(2) - x(1)|^2
    assert np.array_equal(out["msd_sum"], [[[0.0, 5.0], [0.0, 8.0]], [[0.0, 25.0], [0.0, 0.0]]])
    assert np.array_equal(out["n_origins"], [3, 2])
    assert np.array_equal(out["counts"], [[1, 1], [1, 0]])
    assert np.array_equal(out["vacf"][0], [[2.0, 0.0], [2.0, 1.0]])
    assert np.array_equal(out["vacf"][1, 0], [7.0 / 3.0, 0.5])
    assert np.array_equal(out["msd"][0], [[0.0, 2.5], [0.0, 4.0]]) and np.array_equal(out["msd"][1, 0], [0.0, 12.5])
    assert np.array_equal(out["n_terms_v"][0, 0], [9, 6]) and out["abs_v"][0, 0, 1] == 4.0   # |2| + |-2|


def test_correlate_edges():
    xs, vs, natoms, species = _hand_made()
    out = corr.correlate(xs, vs, natoms, species, 2, 5)   # more lags than samples
    assert np.all(out["msd"][..., 0][out["counts"] > 0] == 0.0) and np.all(out["msd_sum"][..., 0] == 0.0)
    assert np.all(np.isnan(out["vacf"][1, 1])) and np.all(np.isnan(out["msd"][1, 1]))   # no atom of element 1
    assert np.all(out["vacf_sum"][1, 1] == 0.0)
    assert np.array_equal(out["n_origins"], [3, 2, 1, 0, 0])
    assert np.all(out["vacf_sum"][..., 3:] == 0.0) and np.all(np.isnan(out["vacf"][..., 3:]))
    one = corr.correlate(xs, vs, natoms, species, 2, 1)   # a ring of one slot: lag 0 alone
    assert np.array_equal(one["vacf_sum"][..., 0], out["vacf_sum"][..., 0]) and one["vacf"].shape == (2, 2, 1)


def test_trajectory_builders_reproduce_the_whole_run_references():
    from tests import md_langevin_reference, md_nhc_reference, md_reference
    k = 2.5
    force = lambda x: (np.array([0.5 * k * (x * x).sum()]), -k * x)
    x0, v0, m = np.array([[0.3, -0.2, 0.1], [0.1, 0.2, -0.4]]), np.array([[0.05, 0.4, -0.3], [-0.2, 0.1, 0.3]]), np.array([1.7, 0.9])
    cases = [
        (corr.trajectory_verlet(force, x0, v0, m, 0.05, 12), md_reference.run(force, x0, v0, m, 0.05, 12)),
        (corr.trajectory_verlet(force, x0, v0, m, 0.05, 12, kT0=0.2, tau=1.0),
         md_reference.run(force, x0, v0, m, 0.05, 12, kT0=0.2, tau=1.0)),
        (corr.trajectory_langevin(force, x0, v0, m, 0.05, 12, 0.1, 0.5, 7),
         md_langevin_reference.run(force, x0, v0, m, 0.05, 12, 0.1, 0.5, 7)),
        (corr.trajectory_nhc(force, x0, v0, m, 0.05, 12, 0.1, 1.0), md_nhc_reference.run(force, x0, v0, m, 0.05, 12, 0.1, 1.0)),
    ]
    for (xs, vs, ekin), whole in cases:
        assert xs.shape == vs.shape == (13, 2, 3) and ekin.shape == (13, 1)
        assert np.array_equal(xs[0], x0) and np.array_equal(vs[0], v0)
        assert np.abs(xs[-1] - whole["x"]).max() < 1e-13 and np.abs(vs[-1] - whole["v"]).max() < 1e-13
        assert np.abs(ekin - whole["ekin"]).max() < 1e-13
        # the sampled velocities are those whose kinetic energy the record holds
        assert np.abs(0.5 * (m[None, :, None] * vs * vs).sum(axis=(1, 2)) - whole["ekin"][:, 0]).max() < 1e-13


@pytest.mark.parametrize("window", ["hann", None])
def test_vdos_of_a_cosine(window):
    L, dt = 256, 2.0 * md.fs
    nu0 = 7.3   # THz
    t_ps = np.arange(L) * 2.0e-3
    nu, g = md.vdos(3.0 * np.cos(2.0 * np.pi * nu0 * t_ps), dt, window=window)
    assert nu.shape == g.shape == (L,)
    assert nu[0] == 0.0 and abs(nu[-1] - 1.0 / (2.0 * 2.0e-3)) < 1e-9 * nu[-1]   # up to Nyquist, 250 THz
    assert np.argmax(g) == np.argmin(np.abs(nu - nu0))
    d = nu[1] - nu[0]
    assert abs(d * (g.sum() - 0.5 * (g[0] + g[-1])) - 1.0) < 1e-12
    # batched along leading axes, every row normalised on its own
    nu2, g2 = md.vdos(np.stack([np.cos(2.0 * np.pi * nu0 * t_ps), 2.0 * np.cos(2.0 * np.pi * 20.0 * t_ps)]), dt, window=window)
    assert g2.shape == (2, L) and np.abs(g2[0] - g).max() < 1e-12
    assert np.argmax(g2[1]) == np.argmin(np.abs(nu - 20.0))


def test_vdos_refusals():
    with pytest.raises(ValueError, match="two lags"):
        md.vdos(np.ones(1), md.fs)
    with pytest.raises(ValueError, match="dt_sample"):
        md.vdos(np.ones(8), 0.0)
    with pytest.raises(ValueError, match="window"):
        md.vdos(np.ones(8), md.fs, window="blackman")


def test_diffusion_coefficient_of_a_straight_line():
    D, dt, L = 0.0137, 3.0 * md.fs, 64
    t = np.arange(L) * dt
    for fit in ((0, L), (10, 50), None):
        got = md.diffusion_coefficient(6.0 * D * t, dt, fit=fit) if fit else md.diffusion_coefficient(6.0 * D * t, dt)
        print(fit, abs(got - D) / D)
        assert abs(got - D) <= 1e-14 * D, (fit, got)
    # two points: the slope is one difference of values near 1.5 that are 0.024 apart, each rounded to eps / 2
    # relative: at most 2 x 1.1e-16 x 1.5 / 0.024 = 1.4e-14 relative
    got = md.diffusion_coefficient(6.0 * D * t, dt, fit=(62, 64))
    assert abs(got - D) <= 2e-14 * D, got
    # an offset (the ballistic part) does not change the slope but is rounded with the values: (0.4 + 1.5) / 1.4
    # (largest value over the rise across the fit) times a few eps, far below 1e-13; leading axes are kept
    both = md.diffusion_coefficient(np.stack([6.0 * D * t + 0.4, 12.0 * D * t]), dt, fit=(8, 64))
    assert both.shape == (2,) and abs(both[0] - D) / D < 1e-13 and abs(both[1] - 2.0 * D) / D < 1e-13


def test_diffusion_coefficient_refuses_bad_fits():
    y = np.arange(16.0)
    for fit in ((4, 4), (5, 4), (0, 17), (-1, 8)):
        with pytest.raises(ValueError, match="lo < hi"):
            md.diffusion_coefficient(y, md.fs, fit=fit)
    with pytest.raises(ValueError, match="two lags"):
        md.diffusion_coefficient(y, md.fs, fit=(3, 4))
    with pytest.raises(ValueError, match="two integers"):
        md.diffusion_coefficient(y, md.fs, fit=(1.5, 8))
    with pytest.raises(ValueError, match="two integers"):
        md.diffusion_coefficient(y, md.fs, fit=(1, 2, 3))
    with pytest.raises(ValueError, match="dt_sample"):
        md.diffusion_coefficient(y, -1.0, fit=(0, 16))


def test_green_kubo_is_the_trapezoid_integral():
    D0, tau, dt, L = 0.8, 40.0 * md.fs, 1.0 * md.fs, 600
    t = np.arange(L) * dt
    c = D0 * np.exp(-t / tau)
    want = dt * (c[0] / 2 + c[1:-1].sum() + c[-1] / 2) / 3.0
    got = md.green_kubo_diffusion(c, dt)
    assert abs(got - want) <= 1e-14 * want
    assert abs(got - D0 * tau / 3.0) < 1e-3 * D0 * tau / 3.0   # (the exponential has decayed, dt << tau)
    assert md.green_kubo_diffusion(np.stack([c, 2 * c]), dt).shape == (2,)
    with pytest.raises(ValueError, match="dt_sample"):
        md.green_kubo_diffusion(c, float("nan"))


def test_helpers_are_exported():
    for name in ("vdos", "diffusion_coefficient", "green_kubo_diffusion", "DeviceMD"):
        assert name in md.__all__ and callable(getattr(md, name))


def test_device_md_argument_errors():
    from tests.helpers import fcc
    atoms = fcc(rep=(1, 1, 1))

    class Recorder:  # stands in for an engine: anything it is asked to do is a failure of the checks
        def md_run(self, *a, **k):
            raise AssertionError("reached the engine")
        set_frames = md_init = md_set_thermostat = md_set_langevin = md_set_nose_hoover = md_set_sampling = md_run

    for bad in (0, -1, 4097, 2.5, True, float("nan")):
        with pytest.raises(ValueError, match="n_lags must be"):
            md.DeviceMD(Recorder(), atoms, md.fs, n_lags=bad)
    for bad in (0, -3, 1.5, False):
        with pytest.raises(ValueError, match="sample_every must be"):
            md.DeviceMD(Recorder(), atoms, md.fs, n_lags=8, sample_every=bad)
    with pytest.raises(ValueError, match="sample_every belongs to sampling"):
        md.DeviceMD(Recorder(), atoms, md.fs, sample_every=2)
    with pytest.raises(ValueError, match=r"n_lags \(sampling\) excludes the barostat"):
        md.DeviceMD(Recorder(), atoms, md.fs, n_lags=8, pressure=0.0, taup=100 * md.fs, compressibility=1.0)
    with pytest.raises(AssertionError, match="reached the engine"):   # a valid request gets through
        md.DeviceMD(Recorder(), atoms, md.fs, n_lags=4096, sample_every=7, temperature_K=300.0, tdamp=20 * md.fs)


def test_abi_of_the_sampling_calls(lib):
    from tensoralloy_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "tensoralloy_amd.h")) as fp:
        header = re.sub(r"/\*.*?\*/", "", fp.read(), flags=re.S)
    for name in ("ta_md_set_sampling", "ta_md_get_correlations", "ta_md_get_samples"):
        assert re.search(r"\bint %s\s*\(ta_handle h," % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert re.search(r"^#define TA_MD_MAX_LAGS 4096$", header, re.M) and _lib.TA_MD_MAX_LAGS == 4096
    assert re.search(r"^#define TA_ABI_VERSION 5$", header, re.M) and _lib.TA_ABI_VERSION == 5
    assert C.sizeof(_lib.MdSamplingParams) == 8
    assert [f[0] for f in _lib.MdSamplingParams._fields_] == ["n_lags", "sample_every"]
    assert "ta_md_corr.hip" in _lib.SOURCES
