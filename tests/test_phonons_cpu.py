"""Host side of the phonon path (no GPU): the shortest-vector lists of `phonons.py` against the restatement's own
image search, mesh and band-path geometry, the thermal sums against the closed form of one oscillator, the ABI."""
import os
import re

import numpy as np
import pytest

from tests import phonon_reference as R
from tests.conftest import GOLDEN, ROOT


def _fixture():
    d = np.load(os.path.join(GOLDEN, "Ni_fc2.npz"))
    return d["fc2"].astype(np.float64), d["frac"], d["cell"]


def _sheared():
    """2 x 2 x 1 repeats of a sheared two-atom cell, the second atom off every symmetric position."""
    cell = np.array([[3.1, 0.0, 0.0], [0.9, 2.8, 0.0], [0.4, -0.6, 5.2]])
    home = np.array([[0.0, 0.0, 0.0], [0.31, 0.52, 0.47]]) @ cell
    pos = [home]
    for x, y in ((0, 1), (1, 0), (1, 1)):
        pos.append(home + np.array([x, y, 0.0]) @ cell)
    return np.concatenate(pos), cell * np.array([2.0, 2.0, 1.0])[:, None], 2


@pytest.mark.parametrize("case", ["fixture", "sheared"])
def test_shortest_vectors_against_the_reference_search(case):
    from tensoralloy_amd.phonons import shortest_vectors
    if case == "fixture":
        _, frac, cell = _fixture()
        pos, nb = frac @ cell, 4
    else:
        pos, cell, nb = _sheared()
    N = len(pos)
    start, vec = shortest_vectors(pos, cell, nb)
    ref = R.shortest_images(pos, cell, nb)
    assert start[0] == 0 and start[-1] == len(vec) and np.all(np.diff(start) >= 1)
    n_multi = 0
    for b in range(nb):
        for s in range(N):
            got = vec[start[b * N + s]:start[b * N + s + 1]]
            want = np.array(ref[b][s])
            assert got.shape == want.shape, (b, s)
            assert np.array_equal(got, want), (b, s)     # the same expression d + t . cell, in the same order
            weights = np.full(len(got), 1.0 / len(got))
            assert abs(weights.sum() - 1.0) < 4 * R.EPS  # multiplicities sum to 1 per pair
            n_multi += len(got) > 1
    # the fixture's 2 x 2 x 2 cell puts atoms on the Wigner-Seitz boundary: lists with 2, 4 and 8 images
    if case == "fixture":
        assert sorted(set(np.diff(start))) == [1, 2, 4, 8] and n_multi > 0
        assert len(vec) == 252


def test_non_periodic_directions_have_no_images():
    from tensoralloy_amd.phonons import shortest_vectors
    pos = np.array([[0.0, 0.0, 0.0], [4.9, 0.0, 0.0]])
    start, vec = shortest_vectors(pos, np.eye(3) * 5.0, 2, pbc=(False, False, False))
    assert list(np.diff(start)) == [1, 1, 1, 1] and np.array_equal(vec[1], [4.9, 0.0, 0.0])
    start, vec = shortest_vectors(pos, np.eye(3) * 5.0, 2, pbc=(True, False, False))
    assert np.allclose(vec[start[1]:start[2]], [[-0.1, 0.0, 0.0]])


def test_mesh_geometry():
    from tensoralloy_amd.phonons import mesh_points
    q = mesh_points(2, 3, 4)
    assert q.shape == (24, 3) and np.array_equal(q[0], [0, 0, 0]) and np.array_equal(q[1], [0, 0, 0.25])
    assert np.array_equal(q[-1], [0.5, 2 / 3, 0.75])
    qs = mesh_points(2, 3, 4, shift=True)
    assert np.allclose(qs - q, [0.25, 1 / 6, 0.125]) and not np.any(np.all(qs == 0, axis=1))
    assert len({tuple(r) for r in q}) == 24


def test_band_path_geometry():
    from tensoralloy_amd.phonons import band_path, reciprocal
    cell = np.array([[0.0, 1.76, 1.76], [1.76, 0.0, 1.76], [1.76, 1.76, 0.0]])
    B = reciprocal(cell)
    assert np.allclose(cell @ B.T, 2 * np.pi * np.eye(3))
    G, X, L = [0, 0, 0], [0.5, 0, 0.5], [0.5, 0.5, 0.5]
    q, d = band_path([[G, X], [G, L]], 11, B)
    assert q.shape == (22, 3) and d.shape == (22,)
    assert np.allclose(q[0], G) and np.allclose(q[10], X) and np.allclose(q[11], G) and np.allclose(q[21], L)
    assert np.all(np.diff(d[:11]) > 0) and d[11] == d[10]
    assert abs(d[10] - 2 * np.pi / 3.52) < 1e-12                   # |Gamma X| of fcc with a = 3.52
    assert abs((d[21] - d[11]) - np.sqrt(3) * np.pi / 3.52) < 1e-12
    q3, d3 = band_path([[G, X, L]], 5, B)
    assert len(q3) == 10 and np.allclose(q3[4], X) and np.allclose(q3[5], X) and d3[5] == d3[4]


def test_thermal_properties_of_one_einstein_frequency():
    from tensoralloy_amd.phonons import KB, harmonic_thermal
    nu = 7.5
    freq = np.array([nu] * 6 + [0.0, -1.0, 0.005])                 # two q-points of three modes, three skipped
    T = np.array([0.0, 50.0, 300.0, 1000.0, 1.0e5])
    out = harmonic_thermal(freq, T, n_q=2)
    assert out["skipped"] == 3
    assert abs(out["free_energy"][0] - 3 * 0.5 * nu * R.THZ_TO_EV) < 1e-15 and out["entropy"][0] == 0.0
    for i in range(1, len(T)):
        F, S, Cv = R.einstein(nu, T[i])
        # three modes per cell; the two evaluations differ by the rounding of exp / log1p near their arguments
        assert abs(out["free_energy"][i] - 3 * F) < 1e-12 * abs(3 * F)
        assert abs(out["entropy"][i] - 3 * S) < 1e-12 * abs(3 * S)
        assert abs(out["heat_capacity"][i] - 3 * Cv) < 1e-12 * abs(3 * Cv)
    # high-temperature limit: C_v -> k per mode, with the first correction -x^2 / 12 (x = h nu / kT = 3.6e-3)
    x = nu * R.THZ_TO_EV / (KB * 1.0e5)
    assert abs(out["heat_capacity"][-1] / (3 * KB) - (1.0 - x * x / 12.0)) < x ** 4
    # F = E - T S with E = sum h nu (1/2 + n): consistency of the three formulas
    n_bose = 1.0 / np.expm1(nu * R.THZ_TO_EV / (KB * 300.0))
    E = 3 * nu * R.THZ_TO_EV * (0.5 + n_bose)
    assert abs(out["free_energy"][2] - (E - 300.0 * out["entropy"][2])) < 1e-12


def test_reference_binning_and_frequency_factor():
    from tensoralloy_amd import _lib, md, phonons
    assert _lib.TA_PHONON_THZ == 1000.0 * md.fs / (2.0 * np.pi) == R.THZ == phonons.THZ
    assert abs(R.THZ - 15.6333) < 1e-4
    k = R.bin_index([-0.1, 0.0, 0.999, 1.0, 9.99, 10.0, np.nan], 0.0, 10.0, 10)
    assert list(k) == [-1, 0, 0, 1, 9, -1, -1]
    assert np.allclose(R.from_thz(R.to_thz(np.array([-2.0, 0.0, 3.0]))), [-2.0, 0.0, 3.0])


def test_abi_lists_the_phonon_symbols():
    from tensoralloy_amd import _lib
    names = ["ta_phonon_set_cell", "ta_phonon_force_constants", "ta_phonon_load_force_constants",
             "ta_phonon_frequencies", "ta_phonon_dos", "ta_phonon_eigh", "ta_phonon_eigh_group"]
    header = open(os.path.join(ROOT, "include", "tensoralloy_amd.h")).read()
    for name in names:
        assert name in _lib.EXPORTED_SYMBOLS
        assert re.search(r"\bint %s\(" % name, header), name
    assert "ta_phonon.hip" in _lib.SOURCES and "ta_api_phonon.hip" in _lib.SOURCES
    assert int(re.search(r"#define TA_PHONON_MAX_ORDER (\d+)", header).group(1)) == _lib.TA_PHONON_MAX_ORDER == 48
    assert int(re.search(r"#define TA_ABI_VERSION (\d+)", header).group(1)) == _lib.TA_ABI_VERSION


def test_library_exports_the_phonon_symbols(lib):
    import ctypes
    from tensoralloy_amd import _lib
    for name in _lib.EXPORTED_SYMBOLS:
        if name.startswith("ta_phonon"):
            assert hasattr(lib, name), name
    assert ctypes.sizeof(_lib.PhononParams) == 8
    # matrices per workgroup of the solver: many small ones share a workgroup, the cap takes one
    assert lib.ta_phonon_eigh_group(3) == 32 and lib.ta_phonon_eigh_group(48) == 1
    assert lib.ta_phonon_eigh_group(49) == 0
