"""CPU: the bond-orientational order parameters of the device MD loop: the NumPy reference
(tests/md_order_reference.py) against closed forms on ideal shells, the `md.*` helpers on hand-made counts, the
argument checks of `DeviceMD` and the C ABI of `ta_md_set_order` / `ta_md_get_order` / `ta_md_get_order_atoms`."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import md_order_reference as ref
from tensoralloy_amd import md

GOLD = (1.0 + np.sqrt(5.0)) / 2.0
A = np.sqrt(8.0 / 3.0)   # c / a of ideal hcp


def _perms(v, even_only=False):
    import itertools
    out = set()
    for p in ([(0, 1, 2), (1, 2, 0), (2, 0, 1)] if even_only else itertools.permutations(range(3))):
        for s in itertools.product((1, -1), repeat=3):
            out.add(tuple(s[k] * v[p[k]] for k in range(3)))
    return np.array(sorted(out), dtype=np.float64)


SHELLS = {   # the bond vectors of a centre, and q4, q6
    "fcc12": (_perms((1, 1, 0)), np.sqrt(7.0 / 192.0), np.sqrt(169.0 / 512.0)),
    "sc6": (_perms((1, 0, 0)), np.sqrt(7.0 / 12.0), np.sqrt(1.0 / 8.0)),
    "bcc8": (_perms((1, 1, 1)), 0.509175, 0.628539),
    "bcc14": (np.concatenate([_perms((1, 1, 1)), _perms((2, 0, 0))]), 0.036370, 0.510688),
    "hcp12": (np.array([[1, 0, 0], [-1, 0, 0], [0.5, np.sqrt(0.75), 0], [-0.5, np.sqrt(0.75), 0], [0.5, -np.sqrt(0.75), 0],
                        [-0.5, -np.sqrt(0.75), 0]] +
                       [[0.5, np.sqrt(1.0 / 12.0), s * A / 2] for s in (1, -1)] + [[-0.5, np.sqrt(1.0 / 12.0), s * A / 2] for s in (1, -1)] +
                       [[0.0, -np.sqrt(1.0 / 3.0), s * A / 2] for s in (1, -1)]), 0.097222, 0.484762),
    "ico12": (_perms((0, 1, GOLD), even_only=True), 0.0, 0.663325),
}


def _q(l, bonds):
    return ref.invariant(l, ref.ylm(l, bonds).mean(axis=0))


@pytest.mark.parametrize("shell", list(SHELLS))
def test_reference_on_ideal_shells(shell):
    bonds, q4, q6 = SHELLS[shell]
    n = {"fcc12": 12, "sc6": 6, "bcc8": 8, "bcc14": 14, "hcp12": 12, "ico12": 12}[shell]
    assert len(bonds) == n
    exact = shell in ("fcc12", "sc6")
    assert _q(4, bonds) == pytest.approx(q4, abs=1e-14 if exact else 5e-7)
    assert _q(6, bonds) == pytest.approx(q6, abs=1e-14 if exact else 5e-7)
    assert _q(2, bonds) == pytest.approx(0.0, abs=1e-14)   # every shell of the table
    if shell == "hcp12":   # all twelve at distance 1: the ideal axis ratio
        assert np.allclose(np.sqrt((bonds * bonds).sum(axis=1)), 1.0, rtol=1e-15)
    if shell != "hcp12":   # inversion symmetry: odd degrees vanish
        for l in (1, 3, 5, 7, 11):
            assert _q(l, bonds) == pytest.approx(0.0, abs=1e-14), l


def test_addition_theorem_and_the_poles():
    rng = np.random.RandomState(7)
    d = np.concatenate([rng.standard_normal((40, 3)), [[0, 0, 1.0], [0, 0, -2.5], [1e-200, 0, 1.0]]])
    for l in range(1, 13):
        y = ref.ylm(l, d)
        assert np.all(np.isfinite(y.real)) and np.all(np.isfinite(y.imag))
        total = np.abs(y[:, 0]) ** 2 + 2.0 * (np.abs(y[:, 1:]) ** 2).sum(axis=1)   # over m = -l .. l
        assert np.allclose(total, (2 * l + 1) / (4.0 * np.pi), rtol=1e-13, atol=0.0), l
        assert np.allclose(y[-3, 0], np.sqrt((2 * l + 1) / (4.0 * np.pi)), rtol=1e-14)        # Y_l0 at the north pole
        assert np.allclose(y[-2, 0], (-1) ** l * np.sqrt((2 * l + 1) / (4.0 * np.pi)), rtol=1e-14)
        assert np.all(y[-3, 1:] == 0.0) and np.all(y[-2, 1:] == 0.0)
    # against the trigonometric form, l = 2: Y_21 = -sqrt(15 / 8 pi) sin cos e^{i phi}, Y_22 = sqrt(15 / 32 pi) sin^2 e^{2 i phi}
    th, ph = 0.7, -2.1
    v = np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
    y = ref.ylm(2, 3.3 * v)
    assert y[0] == pytest.approx(np.sqrt(5.0 / (16.0 * np.pi)) * (3.0 * np.cos(th) ** 2 - 1.0), abs=1e-15)
    assert y[1] == pytest.approx(-np.sqrt(15.0 / (8.0 * np.pi)) * np.sin(th) * np.cos(th) * np.exp(1j * ph), abs=1e-15)
    assert y[2] == pytest.approx(np.sqrt(15.0 / (32.0 * np.pi)) * np.sin(th) ** 2 * np.exp(2j * ph), abs=1e-15)


def _fcc_frame(rep, jitter, seed=1):
    from tests.helpers import fcc
    atoms = fcc(rep=rep, jitter=jitter, seed=seed)
    return np.asarray(atoms.positions, dtype=np.float64), np.asarray(atoms.get_cell(complete=True), dtype=np.float64)


def _params(x, cell, degrees=(4, 6), bins=50, r_bond=3.0, solid=(6, 0.5)):
    return ref.order_parameters(x[None], [cell], [[True] * 3], np.zeros(len(x), dtype=int), [len(x)], 1, degrees, bins,
                                r_bond, solid)


def test_rotation_invariance_of_q_and_qbar():
    x, cell = _fcc_frame((2, 2, 2), 0.08)
    rng = np.random.RandomState(3)
    rot, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    a = _params(x, cell, degrees=(4, 6, 7, 12), solid=(12, 0.5))
    b = _params(x @ rot, cell @ rot, degrees=(4, 6, 7, 12), solid=(12, 0.5))
    assert np.array_equal(a["n_bonds"], b["n_bonds"]) and a["n_bonds"].min() >= 10
    assert np.allclose(a["q"], b["q"], rtol=0.0, atol=1e-13) and np.allclose(a["qbar"], b["qbar"], rtol=0.0, atol=1e-13)
    assert np.array_equal(a["n_conn"], b["n_conn"])
    assert not np.allclose(a["qlm"], b["qlm"], atol=1e-3)   # (the q_lm themselves do turn)
    assert a["q"].max() <= 1.0 and a["q"].std(axis=0).min() > 1e-4


def test_perfect_periodic_fcc():
    x, cell = _fcc_frame((2, 2, 2), 0.0)
    out = _params(x, cell)
    assert np.array_equal(out["n_bonds"], [12] * 32) and np.array_equal(out["n_conn"], [12] * 32)   # s_ij = 1 > 0.5
    assert np.allclose(out["q"], [np.sqrt(7.0 / 192.0), np.sqrt(169.0 / 512.0)], rtol=0.0, atol=1e-14)
    assert np.allclose(out["qbar"], out["q"], rtol=0.0, atol=1e-14)   # every neighbour has the centre's q_lm
    assert out["gap_s"] == pytest.approx(0.5, abs=1e-13) and out["min_norm"] > 0.5
    assert out["gap_r"] == pytest.approx(1.0 - 3.524 / np.sqrt(2.0) / 3.0, abs=1e-12)
    assert out["hist_conn"].shape == (1, 1, 32) and out["hist_conn"][0, 0, 12] == 32 == out["hist_conn"].sum()
    assert out["hist_q"].shape == (1, 1, 2, 50) and out["hist_q"][0, 0, 0, 9] == 32 and out["hist_q"][0, 0, 1, 28] == 32
    assert out["qlm"].shape == (32, 5 + 7)
    # a cutoff below the first shell: no neighbours, everything 0, bin 0
    lone = _params(x, cell, r_bond=2.0)
    assert not lone["n_bonds"].any() and not lone["n_conn"].any() and not lone["q"].any() and not lone["qbar"].any()
    assert lone["hist_q"][0, 0, :, 0].tolist() == [32, 32] and lone["hist_conn"][0, 0, 0] == 32
    assert lone["min_norm"] == np.inf and lone["gap_s"] == np.inf


def test_helpers_on_hand_made_counts():
    h = np.zeros((2, 3, 4), dtype=np.int64)
    h[0, 0] = [1, 0, 3, 4]
    h[1, 2] = [0, 5, 0, 0]
    q, p = md.order_distribution(h)
    assert np.array_equal(q, [0.125, 0.375, 0.625, 0.875]) and p.shape == (2, 3, 4)
    assert np.allclose(p[0, 0], np.array([1, 0, 3, 4]) / 8.0 * 4.0, rtol=1e-15) and (p[0, 0] / 4.0).sum() == pytest.approx(1.0)
    assert np.array_equal(p[1, 2], [0.0, 4.0, 0.0, 0.0])
    assert np.all(np.isnan(p[0, 1])) and np.all(np.isnan(p[1, 0]))
    with pytest.raises(ValueError, match="hist must be"):
        md.order_distribution(np.zeros((3, 0)))
    conn = np.zeros((2, 2, 32), dtype=np.int64)
    conn[0, 0, [0, 7, 8, 12, 31]] = [10, 5, 1, 3, 1]
    conn[1, 1, 12] = 4
    frac = md.solid_fraction(conn, 8)
    assert frac.shape == (2, 2) and frac[0, 0] == pytest.approx(5.0 / 20.0) and frac[1, 1] == 1.0
    assert np.isnan(frac[0, 1]) and np.isnan(frac[1, 0])
    assert md.solid_fraction(conn, 0)[0, 0] == 1.0 and md.solid_fraction(conn, 31)[0, 0] == pytest.approx(1.0 / 20.0)
    for bad in (-1, 32):
        with pytest.raises(ValueError, match="n_min must be 0 .. 31"):
            md.solid_fraction(conn, bad)
    got = md.classify_solid(np.array([0, 7, 8, 12], dtype=np.int32), 8)
    assert got.dtype == bool and got.tolist() == [False, False, True, True]
    for name in ("order_distribution", "solid_fraction", "classify_solid"):
        assert name in md.__all__ and callable(getattr(md, name))


def test_device_md_argument_errors():
    from tests.helpers import fcc
    atoms = fcc(rep=(1, 1, 1))

    class Recorder:  # stands in for an engine: anything it is asked to do is a failure of the checks
        def md_run(self, *a, **k):
            raise AssertionError("reached the engine")
        set_frames = md_init = md_set_thermostat = md_set_langevin = md_set_nose_hoover = md_set_sampling = md_run
        md_set_barostat = md_set_rdf = md_set_adf = md_set_order = md_order = md_order_atoms = md_run

    for bad in (0, -1, 4097, 2.5, True):
        with pytest.raises(ValueError, match="order_bins must be"):
            md.DeviceMD(Recorder(), atoms, md.fs, order_bins=bad)
    for bad in (0, -3, 1.5, False):
        with pytest.raises(ValueError, match="order_every must be"):
            md.DeviceMD(Recorder(), atoms, md.fs, order_bins=8, order_every=bad)
    for bad in ((), (0, 6), (4, 13), (4, 4), (1, 2, 3, 4, 5), (4.5, 6)):
        with pytest.raises(ValueError, match="order_degrees must be"):
            md.DeviceMD(Recorder(), atoms, md.fs, order_bins=8, order_degrees=bad, order_solid=(6, 0.5))
    for bad in ((8, 0.5), (6, 1.0), (6, -1.0), (6, float("nan")), (6,)):
        with pytest.raises(ValueError, match="order_solid must be"):
            md.DeviceMD(Recorder(), atoms, md.fs, order_bins=8, order_solid=bad)
    for bad in (0.0, -1.0, float("nan"), [3.0, 3.0], [[3.0, 2.0], [2.5, 3.0]]):
        with pytest.raises(ValueError, match="order_rbond must be"):
            md.DeviceMD(Recorder(), atoms, md.fs, order_bins=8, order_rbond=bad)
    for kw in (dict(order_every=2), dict(order_rbond=3.0), dict(order_degrees=(4,)), dict(order_solid=(6, 0.5))):
        with pytest.raises(ValueError, match="belong to the bond-orientational order"):
            md.DeviceMD(Recorder(), atoms, md.fs, **kw)
    with pytest.raises(AssertionError, match="reached the engine"):   # a valid request gets through, under the barostat too
        md.DeviceMD(Recorder(), atoms, md.fs, order_bins=8, pressure=0.0, taup=100 * md.fs, compressibility=1.0)


def test_device_md_hands_a_valid_request_to_md_set_order():
    from tests.helpers import fcc
    atoms = fcc(rep=(1, 1, 1))
    calls = []

    class Reached(Exception):
        pass

    class Old:   # the engine as it was before the order parameters
        def _ok(self, *a, **k):
            return None
        set_frames = md_init = md_set_thermostat = md_set_langevin = md_set_nose_hoover = md_set_barostat = _ok
        md_set_sampling = md_set_rdf = md_set_adf = _ok

        def md_run(self, n, dt, **k):
            raise Reached("md_run")

    class New(Old):
        def md_set_order(self, *a, **k):
            calls.append((a, k))
            raise Reached("md_set_order")

    with pytest.raises(Reached, match="md_set_order"):
        md.DeviceMD(New(), atoms, md.fs, order_bins=100, order_rbond=3.0, order_every=4)
    assert calls == [(((4, 6), 3.0, 100, 4, (6, 0.5)), {})]
    with pytest.raises(Reached, match="md_set_order"):
        md.DeviceMD(New(), atoms, md.fs, order_bins=np.int64(16), order_degrees=(12, 1), order_solid=(12, -0.2), adf_bins=8)
    assert calls[1] == (((12, 1), None, 16, 1, (12, -0.2)), {})
    with pytest.raises(Reached, match="md_run"):   # nothing new is called when order_bins is None
        md.DeviceMD(Old(), atoms, md.fs)
    assert len(calls) == 2

    class LeftOn(New):   # an engine on which an earlier DeviceMD left the feature on is told to switch it off
        md_order_bins = 50

    with pytest.raises(Reached, match="md_set_order"):
        md.DeviceMD(LeftOn(), atoms, md.fs)
    assert calls[2] == ((), {"n_bins": 0})


def test_abi_of_the_order_calls(lib):
    from tensoralloy_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "tensoralloy_amd.h")) as fp:
        header = re.sub(r"/\*.*?\*/", "", fp.read(), flags=re.S)
    for name in ("ta_md_set_order", "ta_md_get_order", "ta_md_get_order_atoms"):
        assert re.search(r"\bint %s\s*\(ta_handle h," % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert re.search(r"\bint ta_md_set_order\s*\(ta_handle h, const ta_md_order_params \*p, const double \*r_bond_pairs\);", header)
    assert re.search(r"\bint ta_md_get_order\s*\(ta_handle h, int64_t \*hist_q, int64_t \*hist_qbar, int64_t \*hist_conn, "
                     r"int64_t \*info,\s+double \*r_bond_pairs\);", header)
    assert re.search(r"\bint ta_md_get_order_atoms\s*\(ta_handle h, double \*q, double \*qbar, int32_t \*n_bonds, "
                     r"int32_t \*n_conn, double \*qlm\);", header)
    for name, value in (("TA_MD_ORDER_MAX_DEGREES", 4), ("TA_MD_ORDER_MAX_L", 12), ("TA_MD_ORDER_MAX_CONN", 31)):
        assert re.search(r"^#define %s %d$" % (name, value), header, re.M) and getattr(_lib, name) == value
    assert ref.MAX_CONN == 31
    assert re.search(r"^#define TA_ABI_VERSION 5$", header, re.M) and lib.ta_abi_version() == 5
    struct = re.search(r"typedef struct \{([^}]*)\} ta_md_order_params;", header).group(1)
    names = ["r_bond", "solid_threshold", "n_bins", "sample_every", "n_degrees", "degrees", "solid_degree"]
    assert re.findall(r"\b(?:double|int32_t)\s+(\w+)(?:\[4\])?;", struct) == names
    assert re.search(r"int32_t\s+degrees\[4\];", struct)
    assert C.sizeof(_lib.MdOrderParams) == 48
    assert [f[0] for f in _lib.MdOrderParams._fields_] == names
    assert [getattr(_lib.MdOrderParams, n).offset for n in names] == [0, 8, 16, 20, 24, 28, 44]
    assert "ta_md_order.hip" in _lib.SOURCES
    # the launch's constants are those of the header
    with open(os.path.join(root, "tensoralloy_amd", "csrc", "ta_md.h")) as fp:
        text = fp.read()
    for name, value in (("kMdOrderMaxDegrees", 4), ("kMdOrderMaxL", 12), ("kMdOrderMaxConn", 31), ("kMdOrderMaxLm", 46),
                        ("kMdOrderLdsWords", 8192)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1)) == value, name
