"""CPU: the brute-force definition of the common neighbour analysis (tests/md_cna_reference.py), which the GPU tests
hold the device loop to, on inputs with known answers; and the `md` helpers that read the loop's counts."""
import numpy as np
import pytest

from tests import md_cna_reference as ref
from tests.helpers import fcc, hcp
from tensoralloy_amd import md

R_MAX = 6.0   # the reach of the adaptive mode in these tests: beyond the 14th neighbour of every lattice here


def _frame(atoms):
    return np.asarray(atoms.positions), np.asarray(atoms.get_cell(complete=True)), np.ones(3, dtype=bool)


def _cna(x, cell, pbc=(True, True, True), **kw):
    kw.setdefault("r_max", R_MAX)
    return ref.cna(np.asarray(x)[None], np.asarray(cell)[None], np.asarray(pbc)[None], np.zeros(len(x), dtype=int),
                   [len(x)], 1, **kw)


def _assert_gaps(out, least=1e-9):
    print("gaps", out["gap_r"], out["gap_sel"], out["gap_bond"])
    assert out["gap_r"] >= least and out["gap_sel"] >= least and out["gap_bond"] >= least


def test_names_and_numbers():
    assert md.CNA_NAMES == ("other", "fcc", "hcp", "bcc", "ico")
    assert (ref.OTHER, ref.FCC, ref.HCP, ref.BCC, ref.ICO) == (0, 1, 2, 3, 4)


def test_jittered_fcc_is_fcc():
    x, cell, pbc = _frame(fcc(rep=(3, 3, 3), jitter=0.02))
    out = _cna(x, cell)
    _assert_gaps(out)
    assert out["counts"].tolist() == [[[0, 108, 0, 0, 0]]] and out["series"].tolist() == [[[0, 108, 0, 0, 0]]]
    assert np.all(out["structure"] == ref.FCC)
    # rc = (1 + sqrt 2) / 2 times the mean first-neighbour distance, a / sqrt 2, to the jitter
    assert np.allclose(out["r_local"], ref.SCALE * 3.524 / np.sqrt(2.0), rtol=0.02)


def test_jittered_bcc_is_bcc():
    x, cell = ref.bcc_lattice(2.87, (4, 4, 4), 0.02)
    out = _cna(x, cell)
    _assert_gaps(out)
    assert out["counts"].tolist() == [[[0, 0, 0, 128, 0]]]
    assert np.allclose(out["r_local"], ref.SCALE * 2.87, rtol=0.02)   # (2 / sqrt 3) (sqrt 3 / 2) a = a


def test_jittered_hcp_is_hcp():
    x, cell, pbc = _frame(hcp(rep=(4, 4, 3), jitter=0.02))
    out = _cna(x, cell)
    _assert_gaps(out)
    assert out["counts"].tolist() == [[[0, 0, 96, 0, 0]]]


def test_icosahedron_centre_is_ico_and_its_shell_is_other():
    x, cell = ref.icosahedron(2.5, 20.0)
    out = _cna(x, cell, pbc=(False, False, False))
    _assert_gaps(out)
    assert out["structure"].tolist() == [ref.ICO] + [ref.OTHER] * 12
    assert out["counts"].tolist() == [[[12, 0, 0, 0, 1]]]
    # every shell atom has the twelve others within reach: the attempt is made and fails
    assert np.allclose(out["r_local"][0], ref.SCALE * 2.5) and np.all(out["r_local"][1:] > 0.0)


def test_molten_fcc_is_other():
    x, cell, pbc = _frame(fcc(rep=(3, 3, 3), jitter=0.6))
    out = _cna(x, cell)
    _assert_gaps(out)
    assert out["counts"].tolist() == [[[108, 0, 0, 0, 0]]]


def test_fewer_than_twelve_candidates_is_other_with_r_local_zero():
    x, cell, pbc = _frame(fcc(rep=(3, 3, 3), jitter=0.02))
    out = _cna(x, cell, r_max=2.3)   # below the first shell at 2.49
    assert np.all(out["structure"] == ref.OTHER) and np.all(out["r_local"] == 0.0)
    assert out["gap_sel"] == np.inf and out["gap_bond"] == np.inf


def test_perfect_bcc_is_bcc_whatever_the_tie_break():
    """The 12th and the 13th neighbour of a perfect bcc lattice are both second neighbours at exactly a: the selection
    of twelve depends on the tie-break, the result does not (the twelve are never FCC, HCP or ICO, the fourteen are BCC)."""
    x, cell = ref.bcc_lattice(2.875, (4, 4, 4), 0.0)   # (binary fractions: the distances tie exactly)
    first, second = _cna(x, cell, tie="forward"), _cna(x, cell, tie="reverse")
    assert first["gap_sel"] == 0.0 and second["gap_sel"] == 0.0
    for out in (first, second):
        assert out["counts"].tolist() == [[[0, 0, 0, 128, 0]]]
    assert np.allclose(first["r_local"], second["r_local"], rtol=1e-14)
    # the two orders do select different twelve
    a, _ = ref.candidates(x, cell, (True, True, True), R_MAX, "forward")
    b, _ = ref.candidates(x, cell, (True, True, True), R_MAX, "reverse")
    assert not np.array_equal(a[0][0][:12], b[0][0][:12]) and np.array_equal(a[0][1], b[0][1])


def test_stacking_fault_layers():
    x, cell, layer = ref.close_packed_stack("ABCABCAB", 2.5, (4, 4), 0.02)
    want = np.where((layer == 0) | (layer == 7), ref.HCP, ref.FCC)
    adaptive = _cna(x, cell)
    fixed = _cna(x, cell, mode=ref.FIXED, r_cut=3.0)
    for out in (adaptive, fixed):
        _assert_gaps(out)
        assert np.array_equal(out["structure"], want)
        assert out["counts"].tolist() == [[[0, 96, 32, 0, 0]]]
    assert np.all(fixed["r_local"] == 3.0)


def test_fixed_mode_counts_decide():
    x, cell, pbc = _frame(fcc(rep=(3, 3, 3), jitter=0.02))
    assert _cna(x, cell, mode=ref.FIXED, r_cut=3.0)["counts"].tolist() == [[[0, 108, 0, 0, 0]]]     # 12 neighbours
    assert _cna(x, cell, mode=ref.FIXED, r_cut=4.5)["counts"].tolist() == [[[108, 0, 0, 0, 0]]]     # 12 + 6 + 24
    xb, cb = ref.bcc_lattice(2.87, (4, 4, 4), 0.02)
    assert _cna(xb, cb, mode=ref.FIXED, r_cut=3.4)["counts"].tolist() == [[[0, 0, 0, 128, 0]]]      # 8 + 6, below 4.06
    assert _cna(xb, cb, mode=ref.FIXED, r_cut=2.7)["counts"].tolist() == [[[128, 0, 0, 0, 0]]]      # 8


def test_signatures_of_the_perfect_shells():
    d = np.array([[1, 1, 0], [1, -1, 0], [-1, 1, 0], [-1, -1, 0], [1, 0, 1], [1, 0, -1], [-1, 0, 1], [-1, 0, -1],
                  [0, 1, 1], [0, 1, -1], [0, -1, 1], [0, -1, -1]], dtype=float)
    sigs, gap = ref.signatures(d, 1.2 * np.sqrt(2.0))
    assert sigs == [(4, 2, 1)] * 12 and gap > 0.1
    ico, _ = ref.icosahedron(1.0, 0.0)
    sigs, _ = ref.signatures(ico[1:], ref.SCALE)
    assert sigs == [(5, 5, 5)] * 12


def test_two_species_and_two_frames_are_counted_apart():
    x1, c1, _ = _frame(fcc(rep=(3, 3, 3), jitter=0.02))
    x2, c2 = ref.bcc_lattice(2.87, (4, 4, 4), 0.02)
    species = np.r_[np.arange(108) % 2, np.zeros(128, dtype=int)]
    out = ref.cna(np.vstack([x1, x2])[None], np.array([c1, c2]), np.ones((2, 3), dtype=bool), species, [108, 128], 2,
                  r_max=R_MAX)
    assert out["counts"].tolist() == [[[0, 54, 0, 0, 0], [0, 54, 0, 0, 0]], [[0, 0, 0, 128, 0], [0, 0, 0, 0, 0]]]
    assert out["series"].tolist() == [[[0, 108, 0, 0, 0], [0, 0, 0, 128, 0]]]


def test_structure_fractions():
    counts = np.array([[[0, 54, 0, 0, 0], [6, 42, 6, 0, 0]], [[0, 0, 0, 0, 0], [1, 1, 1, 1, 0]]])
    got = md.structure_fractions(counts)
    assert got.shape == counts.shape and got.dtype == np.float64
    assert got[0, 0].tolist() == [0.0, 1.0, 0.0, 0.0, 0.0]
    assert np.allclose(got[0, 1], [1 / 9, 7 / 9, 1 / 9, 0.0, 0.0])
    assert np.all(np.isnan(got[1, 0])) and got[1, 1].tolist() == [0.25, 0.25, 0.25, 0.25, 0.0]
    assert md.structure_fractions([3, 1, 0, 0, 0]).tolist() == [0.75, 0.25, 0.0, 0.0, 0.0]
    with pytest.raises(ValueError, match=r"structure_fractions: counts must be \[..., 5\]"):
        md.structure_fractions(np.zeros((2, 4)))
