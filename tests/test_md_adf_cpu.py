"""CPU: the bond-angle distributions of the device MD loop: the NumPy reference of the counts
(tests/md_adf_reference.py) against counts worked out by hand, `md.adf`, the argument checks of `DeviceMD` and the
C ABI of `ta_md_set_adf` / `ta_md_get_adf`."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import md_adf_reference as ref
from tensoralloy_amd import md


def test_reference_on_ideal_fcc():
    """Perfect fcc (a = 3.524, 2 x 2 x 2 cells, 32 atoms), bonds below 3.0: the twelve nearest neighbours at 2.492.
    Their 66 pairs subtend 60 (24 pairs), 90 (12), 120 (24) and 180 degrees (6). With B = 25 the bins are 7.2 degrees
    wide and no ideal angle sits on an inner edge: 60 / 7.2 = 8.33, 90 / 7.2 = 12.5, 120 / 7.2 = 16.67, and 180
    degrees belongs to the last bin."""
    from tests.helpers import fcc
    atoms = fcc(rep=(2, 2, 2), jitter=0.0)
    x = np.asarray(atoms.positions)
    stats = {}
    counts, gap_theta, gap_r = ref.triple_counts(x[None], [np.asarray(atoms.get_cell(complete=True))], [[True] * 3],
                                                 np.zeros(32, dtype=int), [32], 1, 25, 3.0, stats=stats)
    assert counts.shape == (1, 1, 1, 25) and counts.dtype == np.int64
    assert np.array_equal(stats["n_neighbours"], [12] * 32)
    want = np.zeros(25, dtype=np.int64)
    want[[8, 12, 16, 24]] = [24, 12, 24, 6]
    assert np.array_equal(counts[0, 0, 0], 32 * want), counts[0, 0, 0]
    assert gap_theta > 0.3    # 8.33: a third of a bin from the nearest edge
    assert gap_r == pytest.approx(1.0 - 3.524 / np.sqrt(2.0) / 3.0, abs=1e-12)   # the first shell is the nearest to 3.0
    # two snapshots of the same lattice, the second unwrapped by lattice vectors: the same triples, twice
    moved = x + np.array([7.048, -14.096, 0.0])
    twice, _, _ = ref.triple_counts(np.stack([x, moved]), [np.asarray(atoms.get_cell(complete=True))], [[True] * 3],
                                    np.zeros(32, dtype=int), [32], 1, 25, 3.0)
    assert np.array_equal(twice, 2 * counts)


def test_reference_pair_indexing_on_two_elements():
    """Two clusters, elements A = 0 and B = 1, bonds below 1.2, B = 3 bins of 60 degrees (90 / 60 = 1.5: bin 1).
     A at the origin with A (1, 0, 0), B (0, 1, 0), B (0, 0, 1): three right angles, two of the pair (A, B) and one
       of (B, B); the three outer atoms are sqrt 2 apart and have the centre as their one neighbour: no triple
     B at (5, 5, 5) with A (5.9, 5, 5) and A (5, 5.9, 5): one right angle of the pair (A, A) around a B
    p(b, c) = b E - b (b - 1) / 2 + (c - b): (A, A) 0, (A, B) 1, (B, B) 2."""
    x = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [5, 5, 5], [5.9, 5, 5], [5, 5.9, 5]])
    sp = [0, 0, 1, 1, 1, 0, 0]
    counts, gap_theta, gap_r = ref.triple_counts(x[None], [20.0 * np.eye(3)], [[False] * 3], sp, [7], 2, 3, 1.2)
    want = np.zeros((2, 3, 3), dtype=np.int64)
    want[0, 1, 1], want[0, 2, 1], want[1, 0, 1] = 2, 1, 1
    assert np.array_equal(counts[0], want), counts[0]
    assert gap_theta == pytest.approx(0.5, abs=1e-12)
    assert gap_r == pytest.approx(0.9 * np.sqrt(2.0) / 1.2 - 1.0, abs=1e-12)   # the two A around the B: 1.273 apart
    # a cutoff per pair of elements. A - B bonds below 0.95 only: around the origin the two B at distance 1 are
    # no neighbours any more and one neighbour makes no angle; around (5, 5, 5) the A at 0.9 stay
    rb = np.array([[1.2, 0.95], [0.95, 1.2]])
    cut, _, _ = ref.triple_counts(x[None], [20.0 * np.eye(3)], [[False] * 3], sp, [7], 2, 3, rb)
    want1 = np.zeros((2, 3, 3), dtype=np.int64)
    want1[1, 0, 1] = 1
    assert np.array_equal(cut[0], want1), cut[0]
    # A - A bonds below 0.95 only:
    rb = np.array([[0.95, 1.2], [1.2, 0.95]])
    cut, _, _ = ref.triple_counts(x[None], [20.0 * np.eye(3)], [[False] * 3], sp, [7], 2, 3, rb)
    want2 = np.zeros((2, 3, 3), dtype=np.int64)
    want2[0, 2, 1], want2[1, 0, 1] = 1, 1   # the A - A bond is gone, and with it the two (A, B) angles
    assert np.array_equal(cut[0], want2), cut[0]
    # the order of p for three elements is that of the nested loops b <= c
    E = 3
    pairs = [(b, c) for b in range(E) for c in range(b, E)]
    for p, (b, c) in enumerate(pairs):
        assert ref.pair_index(np.int64(b), np.int64(c), E) == p == ref.pair_index(np.int64(c), np.int64(b), E)


def test_reference_counts_angles_of_zero_and_pi():
    """Three collinear atoms: around the middle one 180 degrees (the last bin, by the min), around an outer one the
    two others in the same direction: 0 degrees (bin 0)."""
    x = np.array([[0.0, 0, 0], [1, 0, 0], [2, 0, 0]])
    counts, gap_theta, _ = ref.triple_counts(x[None], [20.0 * np.eye(3)], [[False] * 3], [0, 0, 0], [3], 1, 7, 2.5)
    want = np.zeros(7, dtype=np.int64)
    want[0], want[6] = 2, 1
    assert np.array_equal(counts[0, 0, 0], want) and gap_theta == np.inf


def test_adf_normalisation_and_nan_rows():
    c = np.zeros((2, 3, 6), dtype=np.int64)
    c[0, 0] = [0, 3, 5, 7, 0, 1]
    c[1, 2] = [4, 0, 0, 0, 0, 0]
    theta, p = md.adf(c)
    assert np.array_equal(theta, [15.0, 45.0, 75.0, 105.0, 135.0, 165.0]) and p.shape == (2, 3, 6)
    assert np.allclose(p[0, 0] * 30.0, np.array([0, 3, 5, 7, 0, 1]) / 16.0, rtol=1e-15, atol=0.0)
    assert (p[0, 0] * 30.0).sum() == pytest.approx(1.0, abs=1e-15) and (p[1, 2] * 30.0).sum() == pytest.approx(1.0, abs=1e-15)
    for a, q in ((0, 1), (0, 2), (1, 0), (1, 1)):
        assert np.all(np.isnan(p[a, q])), (a, q)
    # leading axes: frames
    theta2, p2 = md.adf(np.stack([c, 3 * c]))
    assert np.array_equal(p2[0], p, equal_nan=True) and np.allclose(p2[1], p, rtol=1e-15, equal_nan=True)
    with pytest.raises(ValueError, match="counts must be"):
        md.adf(np.zeros((3, 4)))
    assert "adf" in md.__all__ and callable(md.adf)


def test_device_md_argument_errors():
    from tests.helpers import fcc
    atoms = fcc(rep=(1, 1, 1))

    class Recorder:  # stands in for an engine: anything it is asked to do is a failure of the checks
        def md_run(self, *a, **k):
            raise AssertionError("reached the engine")
        set_frames = md_init = md_set_thermostat = md_set_langevin = md_set_nose_hoover = md_set_sampling = md_run
        md_set_barostat = md_set_rdf = md_rdf = md_set_adf = md_adf = md_run

    for bad in (0, -1, 4097, 2.5, True, float("nan")):
        with pytest.raises(ValueError, match="adf_bins must be"):
            md.DeviceMD(Recorder(), atoms, md.fs, adf_bins=bad)
    for bad in (0, -3, 1.5, False):
        with pytest.raises(ValueError, match="adf_every must be"):
            md.DeviceMD(Recorder(), atoms, md.fs, adf_bins=8, adf_every=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf"), [3.0, 3.0], [[3.0, 2.0], [2.5, 3.0]], [[3.0, -1.0], [-1.0, 3.0]]):
        with pytest.raises(ValueError, match="adf_rbond must be"):
            md.DeviceMD(Recorder(), atoms, md.fs, adf_bins=8, adf_rbond=bad)
    with pytest.raises(ValueError, match="belong to the bond-angle distributions"):
        md.DeviceMD(Recorder(), atoms, md.fs, adf_every=2)
    with pytest.raises(ValueError, match="belong to the bond-angle distributions"):
        md.DeviceMD(Recorder(), atoms, md.fs, adf_rbond=3.0)
    with pytest.raises(AssertionError, match="reached the engine"):   # a valid request gets through,
        md.DeviceMD(Recorder(), atoms, md.fs, adf_bins=4096, adf_rbond=3.0, adf_every=7)
    with pytest.raises(AssertionError, match="reached the engine"):   # under the barostat too
        md.DeviceMD(Recorder(), atoms, md.fs, adf_bins=8, pressure=0.0, taup=100 * md.fs, compressibility=1.0)


def test_device_md_hands_a_valid_request_to_md_set_adf():
    """An engine stand-in that plays along until `md_set_adf`: it is reached with the arguments as given, and an
    engine without any of the new methods serves a DeviceMD that does not ask for bond-angle distributions."""
    from tests.helpers import fcc
    atoms = fcc(rep=(1, 1, 1))
    calls = []

    class Reached(Exception):
        pass

    class Old:   # the engine as it was before the bond-angle distributions
        def _ok(self, *a, **k):
            return None
        set_frames = md_init = md_set_thermostat = md_set_langevin = md_set_nose_hoover = md_set_barostat = _ok
        md_set_sampling = md_set_rdf = _ok

        def md_run(self, n, dt, **k):
            raise Reached("md_run")

    class New(Old):
        def md_set_adf(self, *a):
            calls.append(a)
            raise Reached("md_set_adf")

    with pytest.raises(Reached, match="md_set_adf"):
        md.DeviceMD(New(), atoms, md.fs, adf_bins=180, adf_rbond=3.0, adf_every=4)
    assert calls == [(180, 3.0, 4)]
    with pytest.raises(Reached, match="md_set_adf"):
        md.DeviceMD(New(), atoms, md.fs, adf_bins=np.int64(16))
    assert calls[1] == (16, None, 1)   # (None: the engine takes the model's cutoff)
    rb = [[3.0, 2.5], [2.5, 2.0]]
    with pytest.raises(Reached, match="md_set_adf"):
        md.DeviceMD(New(), atoms, md.fs, adf_bins=8, adf_rbond=rb, rdf_bins=8)   # (behind the pair distributions)
    assert calls[2] == (8, rb, 1)
    with pytest.raises(Reached, match="md_run"):   # nothing new is called when adf_bins is None
        md.DeviceMD(Old(), atoms, md.fs)
    with pytest.raises(Reached, match="md_run"):
        md.DeviceMD(New(), atoms, md.fs, n_lags=8, rdf_bins=8)
    assert len(calls) == 3

    class LeftOn(New):   # an engine on which an earlier DeviceMD left the feature on says so ...
        md_adf_bins = 180

    with pytest.raises(Reached, match="md_set_adf"):   # ... and is told to switch it off: the one deliberate call
        md.DeviceMD(LeftOn(), atoms, md.fs)
    assert calls[3] == (0,)


def test_get_adf_needs_adf_bins():
    from tests.helpers import fcc
    atoms = fcc(rep=(1, 1, 1))

    class Quiet:   # an engine that plays along to the end of the constructor
        def _ok(self, *a, **k):
            return None
        set_frames = md_init = md_set_thermostat = md_set_langevin = md_set_nose_hoover = md_set_barostat = _ok
        md_set_sampling = _ok

        def md_run(self, n, dt, **k):
            return {"epot": np.zeros((1, 1)), "ekin": np.zeros((1, 1)), "n_rebuilds": 0}

        def md_state(self):
            return np.asarray(atoms.positions).copy(), np.zeros((4, 3))

    dyn = md.DeviceMD(Quiet(), atoms, md.fs)
    with pytest.raises(ValueError, match=r"bond-angle distributions are off \(adf_bins\)"):
        dyn.get_adf()


def test_abi_of_the_adf_calls(lib):
    from tensoralloy_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "tensoralloy_amd.h")) as fp:
        header = re.sub(r"/\*.*?\*/", "", fp.read(), flags=re.S)
    for name in ("ta_md_set_adf", "ta_md_get_adf"):
        assert re.search(r"\bint %s\s*\(ta_handle h," % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert re.search(r"\bint ta_md_set_adf\s*\(ta_handle h, const ta_md_adf_params \*p, const double \*r_bond_pairs\);", header)
    assert re.search(r"\bint ta_md_get_adf\s*\(ta_handle h, int64_t \*counts, int64_t \*info, double \*r_bond_pairs\);", header)
    assert re.search(r"^#define TA_MD_MAX_BINS 4096$", header, re.M) and _lib.TA_MD_MAX_BINS == 4096
    assert re.search(r"^#define TA_ABI_VERSION 5$", header, re.M) and _lib.TA_ABI_VERSION == 5
    assert lib.ta_abi_version() == 5
    struct = re.search(r"typedef struct \{([^}]*)\} ta_md_adf_params;", header).group(1)
    assert re.findall(r"\b(?:double|int32_t)\s+(\w+);", struct) == ["r_bond", "n_bins", "sample_every"]
    assert C.sizeof(_lib.MdAdfParams) == 16
    assert [f[0] for f in _lib.MdAdfParams._fields_] == ["r_bond", "n_bins", "sample_every"]
    assert (_lib.MdAdfParams.r_bond.offset, _lib.MdAdfParams.n_bins.offset, _lib.MdAdfParams.sample_every.offset) == (0, 8, 12)
    assert "ta_md_adf.hip" in _lib.SOURCES
