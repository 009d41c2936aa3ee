"""CPU: the NumPy band reference (tests/neb_reference.py) on an analytic surface and on hand-made energies,
`interpolate` and the argument checks of `DeviceNEB` that need no device, and the new entries of the ABI."""
import re

import numpy as np
import pytest

from tests import neb_reference as nr


def _surface(x):
    """E = (x^2 - 1)^2 + 2 (y - x^2 + 1)^2 + z^2 of one atom per image: minima (+-1, 0, 0), saddle (0, -1, 0)
    with E = 1; the minimum-energy path bends through y < 0."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    u = x[:, 1] - x[:, 0] ** 2 + 1.0
    e = (x[:, 0] ** 2 - 1.0) ** 2 + 2.0 * u ** 2 + x[:, 2] ** 2
    g = np.stack([4.0 * x[:, 0] * (x[:, 0] ** 2 - 1.0) - 8.0 * x[:, 0] * u, 4.0 * u, 2.0 * x[:, 2]], axis=1)
    return e, -g


def _random_band(nim=5, n=4, seed=1):
    rng = np.random.RandomState(seed)
    X = np.cumsum(rng.normal(0.0, 0.3, (nim, n, 3)), axis=0)
    F = rng.normal(0.0, 1.0, (nim, n, 3))
    return X, F


def test_climbing_band_finds_the_saddle_of_an_analytic_surface():
    X0 = np.zeros((7, 1, 3))
    X0[:, 0, 0] = np.linspace(-1.0, 1.0, 7)
    assert abs(_surface([[0.0, -1.0, 0.0]])[0][0] - 1.0) < 1e-15 and not _surface([[0.0, -1.0, 0.0]])[1].any()
    out = nr.run(_surface, nr.new_state(X0), 400, 1e-6, k=1.0, climb=True)
    print("steps", out["steps"], "fmax", out["fmax"], "saddle image", out["x"][3, 0], out["energy"][3])
    assert out["converged"] and 20 < out["steps"] <= 400 and out["fmax"] < 1e-6
    assert out["climbing"] == 3 and all(e["climbing"] == 3 for e in out["log"])
    assert np.abs(out["x"][3, 0] - [0.0, -1.0, 0.0]).max() < 1e-6
    assert abs(out["energy"][3] - 1.0) < 1e-10
    assert np.array_equal(out["x"][[0, -1]], X0[[0, -1]])          # the endpoints did not move
    assert out["x"][1:-1, 0, 1].max() < -0.1                       # the path left the straight line
    # without climbing the same band converges too, and its highest image stays below the saddle
    plain = nr.run(_surface, nr.new_state(X0), 400, 1e-6, k=1.0)
    assert plain["converged"] and plain["climbing"] == -1 and plain["energy"].max() <= 1.0 + 1e-12


def test_tangent_branches_and_ties():
    X, F = _random_band()
    dp, dm = X[2] - X[1], X[1] - X[0]
    unit = lambda t: t / np.sqrt(np.vdot(t, t))
    # rising: d+; falling: d-
    assert nr.tangent_case(0.0, 1.0, 2.0) == "up" and nr.tangent_case(2.0, 1.0, 0.0) == "down"
    _, tau, _ = nr.band_forces(X, [0.0, 1.0, 2.0, 3.0, 4.0], F, 0.1)
    assert np.allclose(tau[1], unit(dp), rtol=0, atol=1e-15)
    _, tau, _ = nr.band_forces(X, [4.0, 3.0, 2.0, 1.0, 0.0], F, 0.1)
    assert np.allclose(tau[1], unit(dm), rtol=0, atol=1e-15)
    # a maximum whose upper neighbour is the higher one: d+ hi + d- lo, hi = |E_0 - E_1| = 1, lo = 0.25
    assert nr.tangent_case(0.0, 1.0, 0.75) == "mixed"
    _, tau, _ = nr.band_forces(X, [0.0, 1.0, 0.75, 0.5, 0.0], F, 0.1)
    assert np.allclose(tau[1], unit(dp * 1.0 + dm * 0.25), rtol=0, atol=1e-15)
    # ... the lower neighbour the higher one: d+ lo + d- hi
    _, tau, _ = nr.band_forces(X, [0.75, 1.0, 0.0, 0.5, 0.0], F, 0.1)
    assert np.allclose(tau[1], unit(dp * 0.25 + dm * 1.0), rtol=0, atol=1e-15)
    # a minimum is mixed as well
    _, tau, _ = nr.band_forces(X, [1.0, 0.0, 0.5, 0.7, 0.0], F, 0.1)
    assert np.allclose(tau[1], unit(dp * 0.5 + dm * 1.0), rtol=0, atol=1e-15)   # (the lower neighbour is higher)
    # ties: an image level with a neighbour is neither rising nor falling; equal neighbours take the second form
    assert nr.tangent_case(1.0, 1.0, 2.0) == "mixed" and nr.tangent_case(2.0, 1.0, 1.0) == "mixed"
    _, tau, _ = nr.band_forces(X, [1.0, 1.0, 2.0, 3.0, 4.0], F, 0.1)
    assert np.allclose(tau[1], unit(dp), rtol=0, atol=1e-15)       # hi = 1 on d+, lo = 0 on d-
    _, tau, _ = nr.band_forces(X, [0.0, 1.0, 0.0, 0.5, 0.0], F, 0.1)
    assert np.allclose(tau[1], unit(dp + dm), rtol=0, atol=1e-15)
    # coincident images: t = 0 gives tau = 0 and B = F
    Xc = X.copy()
    Xc[1] = Xc[0]
    Xc[2] = Xc[0]
    B, tau, _ = nr.band_forces(Xc, [0.0, 1.0, 2.0, 3.0, 4.0], F, 0.1)
    assert not tau[1].any() and np.array_equal(B[1], F[1])
    # the climbing image: the interior image of highest energy, the lowest index on a tie, never an endpoint
    assert nr.band_forces(X, [9.0, 1.0, 3.0, 2.0, 9.0], F, 0.1, climb=True)[2] == 2
    assert nr.band_forces(X, [9.0, 3.0, 3.0, 3.0, 9.0], F, 0.1, climb=True)[2] == 1
    assert nr.band_forces(X, [0.0, 1.0, 2.0, 2.0, 5.0], F, 0.1, climb=True)[2] == 2
    assert nr.band_forces(X, [0.0, 1.0, 2.0, 2.0, 5.0], F, 0.1, climb=False)[2] == -1


def test_projections():
    X, F = _random_band(nim=6, n=5, seed=4)
    E = [0.0, 0.4, 1.3, 1.1, 0.2, 0.1]
    fixed = np.zeros(5, dtype=bool)
    fixed[[1, 3]] = True
    k = 0.7
    for mask in (None, fixed):
        free = np.ones(5, dtype=bool) if mask is None else ~mask
        Fm = np.where(free[None, :, None], F, 0.0)
        for climb in (False, True):
            B, tau, c = nr.band_forces(X, E, F, k, climb, mask)
            assert c == (2 if climb else -1)
            assert not B[0].any() and not B[-1].any() and not tau[0].any() and not tau[-1].any()
            assert not B[:, ~free].any()
            for i in range(1, 5):
                assert abs(np.vdot(tau[i], tau[i]) - 1.0) < 1e-14
                dp, dm = X[i + 1] - X[i], X[i] - X[i - 1]
                spring = k * (np.sqrt(np.vdot(dp, dp)) - np.sqrt(np.vdot(dm, dm)))
                # over the free atoms B = F + (coefficient) tau, so B.tau_free is known in closed form
                tf = np.where(free[:, None], tau[i], 0.0)
                w = float(np.vdot(tf, tf))   # 1 without a mask
                ftau = float(np.vdot(Fm[i], tau[i]))
                got = float(np.vdot(B[i], tau[i]))
                if i == c:
                    assert abs(got - (ftau - 2.0 * ftau * w)) < 1e-13
                else:
                    assert abs(got - (ftau + (spring - ftau) * w)) < 1e-13
                if mask is None:   # B.tau = k (|d+| - |d-|) on ordinary images, -F.tau on the climbing one
                    assert abs(got - (-ftau if i == c else spring)) < 1e-13
                    # the component of B perpendicular to tau is that of F
                    assert np.abs((B[i] - got * tau[i]) - (F[i] - ftau * tau[i])).max() < 1e-13


def test_run_keeps_endpoints_and_fixed_atoms_and_splits():
    rng = np.random.RandomState(2)
    centres = rng.uniform(-0.2, 0.2, (3, 3))

    def force(x):   # three atoms per image in a bowl each, coupled to nothing: the band contracts along itself
        x = x.reshape(-1, 3, 3)
        d = x - centres
        return 0.5 * (d * d).sum(axis=(1, 2)) * np.array([1.0, 2.0, 3.0, 2.5, 1.5]), -d.reshape(-1, 3)

    X0 = np.cumsum(rng.normal(0.0, 0.2, (5, 3, 3)), axis=0)
    fixed = np.array([False, True, False])
    whole = nr.run(force, nr.new_state(X0), 20, 1e-12, k=0.5, fixed=fixed, skin=0.1)
    assert whole["steps"] == 20 and not whole["converged"]
    assert np.array_equal(whole["x"][[0, -1]], X0[[0, -1]]) and np.array_equal(whole["x"][:, 1], X0[:, 1])
    assert not whole["v"][[0, -1]].any() and not whole["v"][:, 1].any()
    assert np.abs(whole["x"][1:-1, 0] - X0[1:-1, 0]).max() > 1e-3
    first = nr.run(force, nr.new_state(X0), 7, 1e-12, k=0.5, fixed=fixed, skin=0.1)
    second = nr.run(force, first["state"], 13, 1e-12, k=0.5, fixed=fixed, skin=0.1)
    for key in ("x", "v", "dt", "a", "npos", "energy", "fmax", "band"):
        assert np.array_equal(second[key], whole[key]), key
    assert first["n_rebuilds"] + second["n_rebuilds"] == whole["n_rebuilds"]
    assert len(whole["log"]) == 21 and whole["log"][0]["branch"] == "first" and "branch" not in whole["log"][-1]


def _pair(shift=(0.0, 0.0, 0.0)):
    from tensoralloy_amd import Atoms
    a = Atoms(symbols=["Ni", "Ni"], positions=[[0.5, 0.5, 0.5], [2.0, 0.5, 0.5]], cell=np.diag([8.0] * 3), pbc=True)
    b = a.copy()
    b.positions[1] += shift
    return a, b


def test_interpolate():
    from tensoralloy_amd import interpolate
    a, b = _pair((1.0, 0.4, 0.0))
    images = interpolate(a, b, 5)
    assert len(images) == 5 and all(im is not a and im is not b for im in images)
    for i, im in enumerate(images):
        assert np.allclose(im.positions, a.positions + (b.positions - a.positions) * i / 4, rtol=0, atol=1e-15)
        assert np.array_equal(np.asarray(im.get_cell(complete=True)), np.asarray(a.get_cell(complete=True)))
    # across the boundary: 0.5 -> 7.9 is a move of -0.6 by minimum image, and the images stay consecutive
    c = a.copy()
    c.positions[0, 0] = 7.9
    images = interpolate(a, c, 4)
    assert np.allclose([im.positions[0, 0] for im in images], [0.5, 0.3, 0.1, -0.1], rtol=0, atol=1e-14)
    plain = interpolate(a, c, 4, mic=False)
    assert np.allclose([im.positions[0, 0] for im in plain], 0.5 + 7.4 * np.arange(4) / 3, rtol=0, atol=1e-14)
    # an open axis is never wrapped
    o, p = _pair()
    o.pbc = p.pbc = [False, True, True]
    p.positions[0, 0] = 7.9
    assert np.allclose(interpolate(o, p, 3)[1].positions[0, 0], 4.2, rtol=0, atol=1e-14)
    with pytest.raises(ValueError, match="n_images"):
        interpolate(a, b, 1)
    d = a.copy()
    d.set_cell(np.diag([8.0, 8.0, 9.0]))
    with pytest.raises(ValueError, match="cell"):
        interpolate(a, d, 3)


def test_device_neb_refuses_bad_arguments_without_a_device():
    from tensoralloy_amd import Atoms, DeviceNEB, interpolate

    class NoDevice:   # stands where an Engine would: touching it is a failure
        def __getattr__(self, name):
            if name == "_engine":
                raise AttributeError(name)
            raise AssertionError(f"the device was reached ({name})")

    a, b = _pair((1.0, 0.0, 0.0))
    band = interpolate(a, b, 4)
    for kw in (dict(dt=0.0), dict(maxstep=float("nan")), dict(fdec=1.0), dict(astart=1.5), dict(Nmin=2.5)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            DeviceNEB(NoDevice(), band, **kw)
    for k in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="k must be"):
            DeviceNEB(NoDevice(), band, k=k)
    with pytest.raises(ValueError, match="at least 3 images"):
        DeviceNEB(NoDevice(), band[:2])
    other = Atoms(symbols=["Ni"] * 3, positions=np.zeros((3, 3)), cell=np.diag([8.0] * 3), pbc=True)
    with pytest.raises(ValueError, match="image 2 .* atom count"):
        DeviceNEB(NoDevice(), band[:2] + [other] + band[2:])
    species = band[1].copy()
    species.numbers[1] = 29
    with pytest.raises(ValueError, match="image 1 .* species"):
        DeviceNEB(NoDevice(), [band[0], species, band[2]])
    cell = band[3].copy()
    cell.set_cell(np.diag([8.0, 8.0, 8.5]))
    with pytest.raises(ValueError, match="image 3 .* cell"):
        DeviceNEB(NoDevice(), band[:3] + [cell])
    pbc = band[2].copy()
    pbc.pbc = [True, True, False]
    with pytest.raises(ValueError, match="image 2 .* pbc"):
        DeviceNEB(NoDevice(), band[:2] + [pbc])
    # a wrapped band: atom 1 jumps by 0.5 of the cell between images 1 and 2
    wrapped = [im.copy() for im in band]
    for im in wrapped[2:]:
        im.positions[1, 0] += 4.0
    with pytest.raises(ValueError, match="atom 1 moves by 0.5.. of a periodic cell vector between images 1 and 2"):
        DeviceNEB(NoDevice(), wrapped)
    for fixed in ([True, False, True], [2], [0.5], np.zeros(8, dtype=bool)):   # over ONE image's atoms
        with pytest.raises(ValueError, match="fixed"):
            DeviceNEB(NoDevice(), band, fixed=fixed)
    with pytest.raises(ValueError, match="Engine or a TensorAlloyCalculator"):
        DeviceNEB(object(), band)


def test_new_entries_are_declared_and_exported():
    import tensoralloy_amd
    from tensoralloy_amd import _lib
    header = (_lib.INCLUDE_DIR / "tensoralloy_amd.h").read_text()
    assert re.search(r"^int ta_relax_set_band\(ta_handle h, int on, const ta_band_params \*p\);", header, re.M)
    assert re.search(r"^int ta_relax_get_band\(ta_handle h, double \*band_forces, double \*tangents, "
                     r"double \*energies, int32_t \*climbing\);", header, re.M)
    assert re.search(r"typedef struct \{\s*double k;\s*int32_t climb;\s*int32_t reserved_;\s*\} ta_band_params;", header)
    assert re.search(r"^#define TA_ABI_VERSION 5$", header, re.M) and _lib.TA_ABI_VERSION == 5
    for name in ("ta_relax_set_band", "ta_relax_get_band"):
        assert name in _lib.EXPORTED_SYMBOLS
    assert "ta_neb.hip" in _lib.SOURCES
    assert [f[0] for f in _lib.BandParams._fields_] == ["k", "climb", "reserved_"]
    for name in ("DeviceNEB", "interpolate"):
        assert name in tensoralloy_amd.__all__
    for name in ("relax_set_band", "relax_band_state"):
        assert callable(getattr(tensoralloy_amd.Engine, name))
