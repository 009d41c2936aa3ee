"""CPU: the pair distributions of the device MD loop: the NumPy reference of the counts
(tests/md_rdf_reference.py) against counts worked out by hand, `md.rdf` and `md.coordination_number`, the argument
checks of `DeviceMD` and the C ABI of `ta_md_set_rdf` / `ta_md_get_rdf`."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import md_rdf_reference as ref
from tensoralloy_amd import md


def test_reference_against_counts_by_hand():
    """Cubic cell of edge 2, dr = 0.5, r_max = 2.5, elements A = 0, B = 1:
    A0 (0, 0, 0), A1 (0, 0, 0.9), B (1.5, 0, 0). Images are (2 l, 2 m, 2 n) apart.
     self-images        : the six at distance 2 (k = 4) of each atom; the next, 2 sqrt 2 = 2.83, are outside
     A0 -> A1 (and back): 0.9 (k 1); 1.1 (k 2); (+-2, 0, 0.9), (0, +-2, 0.9) at 2.193 and the same four with -1.1
                          at 2.283 (k 4, eight in all); 2.9 and 3.1 and the rest are outside
     A0 -> B  (and back): 1.5 (k 3); -0.5 (k 1); (-0.5, +-2, 0), (-0.5, 0, +-2) at 2.062 (k 4, four);
                          (1.5, +-2, 0), (1.5, 0, +-2) and (-2.5, 0, 0) lie EXACTLY on r_max = 2.5: dropped
     A1 -> B  (and back): (1.5, 0, -0.9) 1.749 and (1.5, 0, 1.1) 1.860 (k 3); (-0.5, 0, -0.9) 1.030 and
                          (-0.5, 0, 1.1) 1.208 (k 2); (-0.5, +-2, -0.9) 2.249 and (-0.5, +-2, 1.1) 2.337 (k 4,
                          four); (1.5, +-2, .) at 2.66 and beyond are outside
    """
    x = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.9], [1.5, 0.0, 0.0]])
    counts, gap = ref.pair_counts(x[None], [2.0 * np.eye(3)], [[True] * 3], [0, 0, 1], [3], 2, 5, 2.5)
    assert counts.shape == (1, 2, 2, 5) and counts.dtype == np.int64
    want = np.zeros((2, 2, 5), dtype=np.int64)
    want[0, 0] = [0, 2, 2, 0, 12 + 16]
    want[0, 1] = want[1, 0] = [0, 1, 2, 3, 8]
    want[1, 1] = [0, 0, 0, 0, 6]
    assert np.array_equal(counts[0], want), counts[0]
    assert gap == 0.0   # (the self-images at 2 and the pairs at 2.5 sit on bin edges, exactly)
    # the same atoms unwrapped by lattice vectors, twice: the same pairs, twice
    moved = x + np.array([[2.0, 0.0, 0.0], [0.0, -4.0, 2.0], [-2.0, 2.0, 0.0]])
    twice, _ = ref.pair_counts(np.stack([x, moved]), [2.0 * np.eye(3)], [[True] * 3], [0, 0, 1], [3], 2, 5, 2.5)
    assert np.array_equal(twice[0], 2 * want)
    # without periodicity: the three direct distances 0.9, 1.5, 1.749, each from both ends
    open_, gap = ref.pair_counts(x[None], [2.0 * np.eye(3)], [[False] * 3], [0, 0, 1], [3], 2, 5, 2.5)
    want = np.zeros((2, 2, 5), dtype=np.int64)
    want[0, 0, 1] = 2
    want[0, 1, 3] = want[1, 0, 3] = 2
    assert np.array_equal(open_[0], want) and gap == 0.0   # (1.5 / 0.5 = 3)
    # the distance to the nearest bin edge, in bins: 0.9, 1.5 and 1.749 over dr = 0.65 are 1.385, 2.308 and 2.691
    _, gap = ref.pair_counts(x[None], [2.0 * np.eye(3)], [[False] * 3], [0, 0, 1], [3], 2, 4, 2.6)
    assert gap == pytest.approx(1.5 / 0.65 - 2.0, abs=1e-12)


def test_rdf_of_an_ideal_gas_is_one():
    """800 uniform random points of two elements in a cube of edge 10, minimum-image counts below r_max = 4 in
    8 bins. A bin expects n = N_a N_b v_k / V directed pairs (a != b; N_a (N_a - 1) v_k / V for a == b, which
    the N_a N_b normalisation turns into (N_a - 1) / N_a), half as many independent ones: the relative
    sampling error of g is sqrt(2 / n), and 5 of them are allowed for the 32 values."""
    rng = np.random.RandomState(7)
    N, Lbox, r_max, B = 800, 10.0, 4.0, 8
    x = rng.rand(N, 3) * Lbox
    sp = (rng.rand(N) < 0.3).astype(int)
    d = x[None] - x[:, None]
    d -= Lbox * np.rint(d / Lbox)
    k = np.floor(np.sqrt((d * d).sum(-1)) / (r_max / B)).astype(int)
    np.fill_diagonal(k, B)
    counts = np.zeros((2, 2, B), dtype=np.int64)
    for a in range(2):
        for b in range(2):
            kk = k[np.ix_(sp == a, sp == b)].ravel()
            counts[a, b] = np.bincount(kk[kk < B], minlength=B)
    n_el = np.bincount(sp, minlength=2)
    r, g = md.rdf(counts, 1, n_el, Lbox ** 3, r_max)
    assert r.shape == (B,) and np.allclose(r, (np.arange(B) + 0.5) * 0.5) and g.shape == (2, 2, B)
    shells = 4.0 * np.pi / 3.0 * ((np.arange(B) + 1.0) ** 3 - np.arange(B) ** 3) * 0.5 ** 3
    for a in range(2):
        for b in range(2):
            expect = (n_el[a] - 1.0) / n_el[a] if a == b else 1.0
            sigma = np.sqrt(2.0 / (n_el[a] * n_el[b] * shells / Lbox ** 3))
            print(a, b, np.abs(g[a, b] - expect) / sigma)
            assert np.all(np.abs(g[a, b] - expect) < 5.0 * sigma), (a, b)
    # leading axes: two frames at once, the second with twice the samples and twice the counts
    r2, g2 = md.rdf(np.stack([counts, 2 * counts]), 1, np.stack([n_el, n_el]), np.array([Lbox ** 3, 0.5 * Lbox ** 3]), r_max)
    assert np.array_equal(g2[0], g) and np.allclose(g2[1], g, rtol=1e-15)


def test_rdf_refuses_what_is_not_periodic():
    c = np.ones((1, 1, 4), dtype=np.int64)
    with pytest.raises(ValueError, match="periodic in all three"):
        md.rdf(c, 1, [4], 100.0, 3.0, pbc=[True, True, False])
    with pytest.raises(ValueError, match="periodic in all three"):
        md.rdf(c[None], 1, [[4]], [100.0], 3.0, pbc=[[False] * 3])
    with pytest.raises(ValueError, match="volume"):
        md.rdf(c, 1, [4], 0.0, 3.0)
    with pytest.raises(ValueError, match="r_max"):
        md.rdf(c, 1, [4], 100.0, float("inf"))
    with pytest.raises(ValueError, match="n_by_element"):
        md.rdf(c, 1, [4, 4], 100.0, 3.0)
    r, g = md.rdf(c, 1, [4], 100.0, 3.0, pbc=[True, True, True])
    assert np.all(np.isfinite(g))


def test_rdf_is_nan_where_an_element_is_absent():
    c = np.zeros((2, 2, 4), dtype=np.int64)
    c[0, 0] = [0, 3, 5, 7]
    r, g = md.rdf(c, 2, [5, 0], 50.0, 2.0)
    assert np.all(np.isfinite(g[0, 0])) and g[0, 0, 0] == 0.0
    assert np.all(np.isnan(g[0, 1])) and np.all(np.isnan(g[1, 0])) and np.all(np.isnan(g[1, 1]))
    assert np.all(np.isnan(md.rdf(c, 0, [5, 3], 50.0, 2.0)[1]))   # nothing sampled yet


def test_coordination_number_of_fcc_is_twelve():
    """Perfect fcc (a = 3.524, 2 x 2 x 2 cells, 32 atoms): twelve neighbours at a / sqrt 2 = 2.492, the next six at
    3.524. Counted below 3.0 in 30 bins over 3 samples of the same lattice, the integral to 2.8 returns the
    counts / (n_samples N) exactly: all twelve neighbours fall into ONE bin, so the sum has one term,
    (C V / (n N N v_k)) v_k N / V with C = 3 x 32 x 12, in which the shell volume v_k that `rdf` divided by is the
    very double that `coordination_number` multiplies by; the result is 12.0, not 12 within a tolerance."""
    from tests.helpers import fcc
    atoms = fcc(rep=(2, 2, 2), jitter=0.0)
    x = np.asarray(atoms.positions)
    cell = np.asarray(atoms.get_cell(complete=True))
    counts, gap = ref.pair_counts(np.stack([x, x, x]), [cell], [[True] * 3], np.zeros(32, dtype=int), [32], 1, 30, 3.0)
    assert gap > 1e-3 and counts.sum() == 3 * 32 * 12 and np.count_nonzero(counts) == 1
    V = abs(np.linalg.det(cell))
    r, g = md.rdf(counts[0], 3, [32], V, 3.0)
    n = md.coordination_number(g[0, 0], r, 32 / V, 2.8)
    assert n == 12.0
    assert md.coordination_number(g[0, 0], r, 32 / V, 2.0) == 0.0
    assert md.coordination_number(g, r, 32 / V, 2.8).shape == (1, 1)
    with pytest.raises(ValueError, match="uniform bins"):
        md.coordination_number(g[0, 0], r + 0.1, 32 / V, 2.8)


def test_helpers_are_exported():
    for name in ("rdf", "coordination_number"):
        assert name in md.__all__ and callable(getattr(md, name))


def test_device_md_argument_errors():
    from tests.helpers import fcc
    atoms = fcc(rep=(1, 1, 1))

    class Recorder:  # stands in for an engine: anything it is asked to do is a failure of the checks
        def md_run(self, *a, **k):
            raise AssertionError("reached the engine")
        set_frames = md_init = md_set_thermostat = md_set_langevin = md_set_nose_hoover = md_set_sampling = md_run
        md_set_barostat = md_set_rdf = md_rdf = md_run

    for bad in (0, -1, 4097, 2.5, True, float("nan")):
        with pytest.raises(ValueError, match="rdf_bins must be"):
            md.DeviceMD(Recorder(), atoms, md.fs, rdf_bins=bad)
    for bad in (0, -3, 1.5, False):
        with pytest.raises(ValueError, match="rdf_every must be"):
            md.DeviceMD(Recorder(), atoms, md.fs, rdf_bins=8, rdf_every=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="rdf_rmax must be"):
            md.DeviceMD(Recorder(), atoms, md.fs, rdf_bins=8, rdf_rmax=bad)
    with pytest.raises(ValueError, match="belong to the pair distributions"):
        md.DeviceMD(Recorder(), atoms, md.fs, rdf_every=2)
    with pytest.raises(ValueError, match="belong to the pair distributions"):
        md.DeviceMD(Recorder(), atoms, md.fs, rdf_rmax=3.0)
    with pytest.raises(ValueError, match=r"rdf_bins \(pair distributions\) excludes the barostat"):
        md.DeviceMD(Recorder(), atoms, md.fs, rdf_bins=8, pressure=0.0, taup=100 * md.fs, compressibility=1.0)
    with pytest.raises(AssertionError, match="reached the engine"):   # a valid request gets through
        md.DeviceMD(Recorder(), atoms, md.fs, rdf_bins=4096, rdf_rmax=3.0, rdf_every=7)


def test_device_md_hands_a_valid_request_to_md_set_rdf():
    """An engine stand-in that plays along until `md_set_rdf`: it is reached with the arguments as given, and an
    engine without any of the new methods serves a DeviceMD that does not ask for pair distributions."""
    from tests.helpers import fcc
    atoms = fcc(rep=(1, 1, 1))
    calls = []

    class Reached(Exception):
        pass

    class Old:   # the engine as it was before the pair distributions
        def _ok(self, *a, **k):
            return None
        set_frames = md_init = md_set_thermostat = md_set_langevin = md_set_nose_hoover = md_set_barostat = _ok
        md_set_sampling = _ok

        def md_run(self, n, dt, **k):
            raise Reached("md_run")

    class New(Old):
        def md_set_rdf(self, *a):
            calls.append(a)
            raise Reached("md_set_rdf")

    with pytest.raises(Reached, match="md_set_rdf"):
        md.DeviceMD(New(), atoms, md.fs, rdf_bins=64, rdf_rmax=4.5, rdf_every=3)
    assert calls == [(64, 4.5, 3)]
    with pytest.raises(Reached, match="md_set_rdf"):
        md.DeviceMD(New(), atoms, md.fs, rdf_bins=np.int64(16))
    assert calls[1] == (16, None, 1)   # (None: the engine takes the model's cutoff)
    with pytest.raises(Reached, match="md_run"):   # nothing new is called when rdf_bins is None
        md.DeviceMD(Old(), atoms, md.fs)
    with pytest.raises(Reached, match="md_run"):
        md.DeviceMD(New(), atoms, md.fs, n_lags=8)
    assert len(calls) == 2

    class LeftOn(New):   # an engine on which an earlier DeviceMD left the pair distributions on says so ...
        md_rdf_bins = 64

    with pytest.raises(Reached, match="md_set_rdf"):   # ... and is told to switch them off: the one deliberate call
        md.DeviceMD(LeftOn(), atoms, md.fs)
    assert calls[2] == (0,)


def test_abi_of_the_rdf_calls(lib):
    from tensoralloy_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "tensoralloy_amd.h")) as fp:
        header = re.sub(r"/\*.*?\*/", "", fp.read(), flags=re.S)
    for name in ("ta_md_set_rdf", "ta_md_get_rdf"):
        assert re.search(r"\bint %s\s*\(ta_handle h," % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert re.search(r"^#define TA_MD_MAX_BINS 4096$", header, re.M) and _lib.TA_MD_MAX_BINS == 4096
    assert re.search(r"^#define TA_ABI_VERSION 5$", header, re.M) and _lib.TA_ABI_VERSION == 5
    struct = re.search(r"typedef struct \{([^}]*)\} ta_md_rdf_params;", header).group(1)
    assert re.findall(r"\b(?:double|int32_t)\s+(\w+);", struct) == ["r_max", "n_bins", "sample_every"]
    assert C.sizeof(_lib.MdRdfParams) == 16
    assert [f[0] for f in _lib.MdRdfParams._fields_] == ["r_max", "n_bins", "sample_every"]
    assert (_lib.MdRdfParams.r_max.offset, _lib.MdRdfParams.n_bins.offset, _lib.MdRdfParams.sample_every.offset) == (0, 8, 12)
    assert "ta_md_rdf.hip" in _lib.SOURCES
