"""CPU: the structure factors of the device MD loop: the long-double NumPy reference (tests/md_sq_reference.py)
against values worked out by hand, the helpers of `tensoralloy_amd.md` (`q_points`, `intermediate_scattering`,
`structure_factor`, `transverse_current`, `dynamic_structure_factor`, `shell_average`), the argument checks of
`DeviceMD` and the C ABI of `ta_md_set_sq` / `ta_md_get_sq` / `ta_md_get_sq_amplitudes`."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import md_sq_reference as ref
from tensoralloy_amd import md


def _cube(m, a=2.0):   # (a power of two: the fractional coordinates are exact)
    g = np.arange(m)
    x = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) * a
    return x.astype(np.float64), np.eye(3) * a * m


def test_reference_simple_cubic_lattice():
    """m^3 atoms on a simple-cubic lattice in a cell of m lattice constants: rho(n) = N where every index is a
    multiple of m (a reciprocal-lattice vector of the crystal) and 0 elsewhere."""
    m = 3
    x, cell = _cube(m)
    miller = np.array([[i, j, k] for i in range(-4, 5) for j in range(-4, 5) for k in range(0, 7)])
    rho, cur, reach = ref.amplitudes(x, None, cell, np.zeros(len(x), dtype=int), 1, miller)
    bragg = np.all(miller % m == 0, axis=1)
    assert bragg.sum() >= 27 and (~bragg).sum() > 400 and cur is None
    assert np.abs(rho[0][bragg] - len(x)).max() < 1e-15 * len(x)
    assert np.abs(rho[0][~bragg]).max() < 1e-15 * len(x)
    assert reach.shape == (1, len(miller)) and reach.max() == pytest.approx(4 * 2 / 3 * 2 + 6 * 2 / 3, abs=1e-12)


def test_reference_two_atoms_two_elements_in_closed_form():
    """A at the origin, B at fractional (1/4, 1/2, 0) of a triclinic cell: rho_A = 1, rho_B = exp(2 pi i (n_0 / 4 +
    n_1 / 2)); with velocities v_A, v_B the currents are v_A and v_B rho_B, and
    A_rho[A][B] = Re(rho_A conj rho_B) = cos(2 pi (n_0 / 4 + n_1 / 2))."""
    cell = np.array([[4.0, 0.0, 0.0], [0.7, 3.0, 0.0], [-0.4, 0.9, 5.0]])
    x = np.array([[0.0, 0.0, 0.0], 0.25 * cell[0] + 0.5 * cell[1]])
    v = np.array([[0.3, -0.2, 0.1], [-0.5, 0.4, 0.25]])
    miller = np.array([[0, 0, 0], [1, 0, 0], [2, 1, 0], [1, 1, 3], [-3, 2, 1], [4, 0, -2]])
    out = ref.structure_factors(x[None], v[None], cell, [0, 1], 2, miller, 1, chain=3)
    want_b = np.exp(2j * np.pi * (miller[:, 0] / 4.0 + miller[:, 1] / 2.0))
    assert np.abs(out["rho"][0, 0] - 1.0).max() < 1e-15 and np.abs(out["rho"][0, 1] - want_b).max() < 1e-15
    assert np.abs(out["cur"][0, 0] - v[0][None, :]).max() < 1e-15
    assert np.abs(out["cur"][0, 1] - want_b[:, None] * v[1][None, :]).max() < 1e-15
    a = out["a_rho"]
    assert a.shape == (2, 2, 1, 6)
    assert np.abs(a[0, 0, 0] - 1.0).max() < 1e-15 and np.abs(a[1, 1, 0] - 1.0).max() < 1e-15
    assert np.abs(a[0, 1, 0] - want_b.real).max() < 1e-15 and np.array_equal(a[0, 1], a[1, 0])
    # the trace of the current tensor: v_a . v_b Re(rho_a conj rho_b); its longitudinal part: (qhat . v_a)(qhat . v_b)
    assert np.abs(out["a_j"][0, 1, 0] - v[0] @ v[1] * want_b.real).max() < 1e-15
    q = 2.0 * np.pi * miller @ np.linalg.inv(cell).T
    assert np.abs(out["q"] - q).max() < 1e-14
    qhat = q[1:] / np.linalg.norm(q[1:], axis=1)[:, None]
    assert np.abs(out["a_l"][0, 1, 0, 1:] - (qhat @ v[0]) * (qhat @ v[1]) * want_b.real[1:]).max() < 1e-15
    assert out["a_l"][0, 1, 0, 0] == 0.0 and out["a_l"][0, 0, 0, 0] == 0.0   # n = 0: qhat = (0, 0, 0)
    assert np.abs(out["a_j"][0, 0, 0] - v[0] @ v[0]).max() < 1e-15
    for key in ("rho_bound", "cur_bound", "a_rho_bound", "a_l_bound", "a_j_bound"):
        assert np.all(out[key][..., 1:] > 0.0) and np.all(out[key] < 1e-12), key   # (n = 0 has no longitudinal part)


def test_reference_lattice_moves_and_rigid_translations():
    rng = np.random.RandomState(3)
    cell = np.array([[5.0, 0.0, 0.0], [1.1, 4.5, 0.0], [0.3, -0.8, 6.0]])
    x = rng.rand(40, 3) @ cell
    v = rng.standard_normal((40, 3))
    sp = (rng.rand(40) < 0.4).astype(int)
    miller = np.array([[1, 0, 0], [0, 2, -1], [3, 3, 1], [-2, 5, 7], [64, -64, 64]])
    base = ref.structure_factors(np.stack([x, x + 0.01 * v]), np.stack([v, v]), cell, sp, 2, miller, 2, chain=41)
    # atoms moved by lattice vectors, each by its own: nothing changes but the rounding of the moved coordinates to
    # doubles, 2^-53 of |s| <= 4 each, which the largest triple (192 in all) turns into 2 pi 192 4 2^-53 of phase per atom
    moved = x + rng.randint(-3, 4, size=(40, 3)) @ cell
    far = ref.structure_factors(np.stack([moved, moved + 0.01 * v]), np.stack([v, v]), cell, sp, 2, miller, 2, chain=41)
    tol = 40 * 2.0 * np.pi * 192 * 4 * 2.0 ** -53
    assert np.abs(far["rho"] - base["rho"]).max() < tol and np.abs(far["cur"] - base["cur"]).max() < 4.0 * tol
    assert np.abs(far["rho"] - base["rho"])[..., :4].max() < 1e-13   # (the small triples)
    for key in ("a_rho", "a_l", "a_j"):
        assert np.abs(far[key] - base[key]).max() < 1e-9, key
    # a rigid translation by d multiplies every rho by exp(i q . d) and leaves the accumulators alone
    d = np.array([0.37, -1.3, 2.2])
    shifted = ref.structure_factors(np.stack([x + d, x + 0.01 * v + d]), np.stack([v, v]), cell, sp, 2, miller, 2, chain=41)
    phase = np.exp(1j * (base["q"] @ d))
    assert np.abs(shifted["rho"] - base["rho"] * phase[None, None, :]).max() < 1e-12
    assert np.abs(shifted["rho"] - base["rho"]).max() > 1.0
    for key in ("a_rho", "a_l", "a_j"):
        assert np.abs(shifted[key] - base[key]).max() < 1e-11, key
    assert np.all(base["a_rho_bound"] < 1e-9) and np.abs(base["a_rho"]).max() > 10.0


def test_structure_factor_of_an_ideal_gas_is_one():
    """2000 uniform random points in a cube of edge 20: |rho(q)|^2 / N is exponentially distributed with mean 1 and
    variance 1, independently for the q of a shell (one of each +-n pair), so the mean over a shell of n_k vectors
    has the sampling error sqrt(1 / n_k): five of them are allowed in each of the 7 shells that hold a vector."""
    rng = np.random.RandomState(11)
    N, edge = 2000, 20.0
    cell = np.eye(3) * edge
    x = rng.rand(N, 3) * edge
    miller = md.q_points(cell, 2.2)
    assert 600 < len(miller) < 800
    rho = ref.amplitudes(x, None, cell, np.zeros(N, dtype=int), 1, miller)[0].astype(np.complex128)
    a_rho = (np.abs(rho) ** 2).reshape(1, 1, 1, -1)
    s_ab, s = md.structure_factor(a_rho, 1, [N])
    assert s_ab.shape == (1, 1, len(miller)) and np.array_equal(s, s_ab[0, 0])
    q_norm = np.linalg.norm(2.0 * np.pi * miller / edge, axis=1)
    q, mean, counts = md.shell_average(s, q_norm, 8)
    print(counts, (mean - 1.0) * np.sqrt(counts))
    assert counts.sum() == len(miller) and counts[0] == 0 and np.isnan(mean[0])   # (2 pi / 20 lies beyond 2.2 / 8)
    q, mean, counts = q[1:], mean[1:], counts[1:]
    assert counts.min() >= 7
    assert np.all(np.abs(mean - 1.0) < 5.0 / np.sqrt(counts))
    assert np.all(np.diff(q) > 0.0) and q[-1] <= 2.2


def test_q_points():
    cell = np.array([[4.0, 0.0, 0.0], [1.0, 5.0, 0.0], [0.0, -2.0, 7.0]])
    n = md.q_points(cell, 3.0)
    assert n.dtype == np.int32 and n.ndim == 2 and n.shape[1] == 3
    q = np.linalg.norm(2.0 * np.pi * n @ np.linalg.inv(cell).T, axis=1)
    assert np.all(q > 0.0) and np.all(q <= 3.0) and np.all(np.diff(q) >= -1e-12)
    both = {tuple(t) for t in n} | {tuple(-t) for t in n}
    assert len(both) == 2 * len(n)   # one of each +-n pair
    # brute force over a box that is certainly large enough
    g = np.arange(-12, 13)
    box = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    qb = np.linalg.norm(2.0 * np.pi * box @ np.linalg.inv(cell).T, axis=1)
    assert ((qb > 0.0) & (qb <= 3.0)).sum() == 2 * len(n)
    assert np.abs(md.q_points(cell, 3.0, max_index=2)).max() == 2
    for bad in (dict(cell=np.zeros((3, 3)), q_max=1.0), dict(cell=cell, q_max=0.0), dict(cell=cell, q_max=float("nan")),
                dict(cell=cell, q_max=1.0, max_index=65), dict(cell=cell[:2], q_max=1.0)):
        with pytest.raises(ValueError, match="q_points"):
            md.q_points(**bad)


def test_normalisation_and_absent_elements():
    acc = np.zeros((2, 2, 3, 4))
    acc[0, 0] = np.arange(12).reshape(3, 4) + 1.0
    f = md.intermediate_scattering(acc, 2, [5, 0])
    assert np.array_equal(f[0, 0, 0], acc[0, 0, 0] / (2 * 5.0)) and np.array_equal(f[0, 0, 1], acc[0, 0, 1] / (1 * 5.0))
    assert np.all(np.isnan(f[0, 0, 2]))   # lag 2 of two samples has no time origin
    assert np.all(np.isnan(f[0, 1])) and np.all(np.isnan(f[1, 0])) and np.all(np.isnan(f[1, 1]))
    s_ab, s = md.structure_factor(acc, 2, [5, 0])
    assert np.array_equal(s_ab[0, 0], f[0, 0, 0]) and np.array_equal(s, f[0, 0, 0])   # the absent element has no share
    assert np.all(np.isnan(md.structure_factor(acc, 0, [5, 0])[1]))
    # two elements: S = sum_ab sqrt(c_a c_b) S_ab = |rho_0 + rho_1|^2 / N
    rho = np.array([1.5 - 0.5j, -0.25 + 2.0j])
    a = (rho[:, None] * np.conj(rho[None, :])).real.reshape(2, 2, 1, 1)
    s_ab, s = md.structure_factor(a, 1, [3, 7])
    assert s_ab[0, 1, 0] == pytest.approx(a[0, 1, 0, 0] / np.sqrt(21.0), rel=1e-15)
    assert s[0] == pytest.approx(abs(rho.sum()) ** 2 / 10.0, rel=1e-14)
    # leading axes
    f2 = md.intermediate_scattering(np.stack([acc, 2 * acc]), 2, [[5, 0], [5, 0]])
    assert np.array_equal(f2[0, 0, 0], f[0, 0], equal_nan=True) and np.array_equal(f2[1, 0, 0, :2], 2 * f[0, 0, :2])
    with pytest.raises(ValueError, match="n_by_element"):
        md.intermediate_scattering(acc, 2, [5, 0, 1])
    with pytest.raises(ValueError, match="n_samples"):
        md.intermediate_scattering(acc, -1, [5, 0])
    with pytest.raises(ValueError, match="acc must be"):
        md.intermediate_scattering(np.zeros((2, 3, 1, 4)), 1, [5, 0])


def test_longitudinal_and_transverse_split_of_a_plane_wave():
    """v_i = e cos(q0 . x_i) on a 4^3 lattice: j(q0) = e N / 2. For e along q0 the current is longitudinal, A_L =
    A_J = N^2 / 4 and nothing is transverse; for e across q0, A_L = 0 and the transverse part per direction is
    A_J / 2 = N^2 / 8."""
    x, cell = _cube(4)
    miller = np.array([[1, 0, 0], [0, 1, 0]])
    q0 = 2.0 * np.pi * np.array([1.0, 0.0, 0.0]) / cell[0, 0]
    N = len(x)
    for e, want_l, want_t in ((np.array([1.0, 0.0, 0.0]), N * N / 4.0, 0.0), (np.array([0.0, 0.0, 1.0]), 0.0, N * N / 8.0)):
        v = np.cos(x @ q0)[:, None] * e[None, :]
        out = ref.structure_factors(x[None], v[None], cell, np.zeros(N, dtype=int), 1, miller, 1, chain=N)
        t = md.transverse_current(out["a_j"], out["a_l"])
        assert out["a_l"][0, 0, 0, 0] == pytest.approx(want_l, abs=1e-9) and t[0, 0, 0, 0] == pytest.approx(want_t, abs=1e-9)
        assert abs(out["a_j"][0, 0, 0, 1]) < 1e-9   # nothing at another wave vector
        c_t = md.intermediate_scattering(t, 1, [N])
        assert c_t[0, 0, 0, 0] == pytest.approx(want_t / N, abs=1e-9)


def test_dynamic_structure_factor_peaks_at_the_frequency_of_a_damped_cosine():
    L, dt = 257, 2.0 * md.fs
    t_ps = np.arange(L) * 2.0e-3
    nu0 = np.array([5.0, 12.5])   # THz
    F = (np.exp(-t_ps[:, None] / 0.15) * np.cos(2.0 * np.pi * nu0[None, :] * t_ps[:, None]))
    nu, s = md.dynamic_structure_factor(F, dt)
    assert nu.shape == (L,) and s.shape == (L, 2) and nu[0] == 0.0 and nu[-1] == pytest.approx(250.0, rel=1e-12)
    assert np.array_equal(nu, md.vdos(F[:, 0], dt)[0])   # the grid of vdos
    peak = nu[np.argmax(s, axis=0)]
    assert np.all(np.abs(peak - nu0) <= nu[1])
    # without a window the integral over the two-sided spectrum gives F(q, 0) back: 2 x trapezoid over nu >= 0
    nu, s = md.dynamic_structure_factor(F, dt, window=None)
    total = 2.0 * (nu[1] - nu[0]) * (s.sum(axis=0) - 0.5 * (s[0] + s[-1]))
    assert np.allclose(total, 1.0, atol=1e-9)
    # leading axes stay where they are: [E, E, L, Q]
    nu, s4 = md.dynamic_structure_factor(np.broadcast_to(F, (2, 2, L, 2)), dt, window=None)
    assert s4.shape == (2, 2, L, 2) and np.array_equal(s4[1, 0], s)
    with pytest.raises(ValueError, match="window"):
        md.dynamic_structure_factor(F, dt, window="blackman")
    with pytest.raises(ValueError, match="at least two lags"):
        md.dynamic_structure_factor(F[:1], dt)
    with pytest.raises(ValueError, match="dt_sample"):
        md.dynamic_structure_factor(F, 0.0)


def test_shell_average():
    q_norm = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 2.0])
    values = np.array([[9.0, 1.0, 3.0, 5.0, 7.0, 9.0], [0.0, 2.0, 2.0, 4.0, 4.0, 6.0]])
    q, mean, counts = md.shell_average(values, q_norm, 2)
    assert np.array_equal(counts, [2, 3])   # q = 0 belongs to no shell; an edge (1.0) to the shell below
    assert np.array_equal(q, [0.75, 5.5 / 3]) and np.allclose(mean, [[2.0, 7.0], [2.0, 14.0 / 3]], rtol=1e-15)
    q, mean, counts = md.shell_average(values[0], q_norm, 8)
    assert counts.sum() == 5 and np.isnan(mean[0]) and np.isnan(q[0]) and mean[-1] == 8.0
    with pytest.raises(ValueError, match="n_bins"):
        md.shell_average(values, q_norm, 0)
    with pytest.raises(ValueError, match="q_norm"):
        md.shell_average(values, np.zeros(6), 2)
    with pytest.raises(ValueError, match="values"):
        md.shell_average(values[:, :5], q_norm, 2)


def test_helpers_are_exported():
    for name in ("q_points", "intermediate_scattering", "structure_factor", "transverse_current",
                 "dynamic_structure_factor", "shell_average"):
        assert name in md.__all__ and callable(getattr(md, name))


def test_device_md_argument_errors():
    from tests.helpers import fcc
    atoms = fcc(rep=(1, 1, 1))
    ok = np.array([[1, 0, 0], [0, 1, 1]])

    class Recorder:  # stands in for an engine: anything it is asked to do is a failure of the checks
        def md_run(self, *a, **k):
            raise AssertionError("reached the engine")
        set_frames = md_init = md_set_thermostat = md_set_langevin = md_set_nose_hoover = md_set_sampling = md_run
        md_set_barostat = md_set_sq = md_sq = md_run

    for bad in (np.zeros((0, 3), dtype=int), np.array([1, 0, 0]), np.array([[1, 0]]), np.array([[1.0, 0.0, 0.0]]),
                np.array([[65, 0, 0]]), np.array([[0, -65, 0]]), np.zeros((4097, 3), dtype=int)):
        with pytest.raises(ValueError, match="sq_miller must be"):
            md.DeviceMD(Recorder(), atoms, md.fs, sq_miller=bad)
    for bad in (0, -1, 4097, 2.5, True):
        with pytest.raises(ValueError, match="sq_lags must be"):
            md.DeviceMD(Recorder(), atoms, md.fs, sq_miller=ok, sq_lags=bad)
    for bad in (0, -3, 1.5, False):
        with pytest.raises(ValueError, match="sq_every must be"):
            md.DeviceMD(Recorder(), atoms, md.fs, sq_miller=ok, sq_every=bad)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="sq_currents must be"):
            md.DeviceMD(Recorder(), atoms, md.fs, sq_miller=ok, sq_currents=bad)
    for extra in (dict(sq_lags=4), dict(sq_every=2), dict(sq_currents=True)):
        with pytest.raises(ValueError, match="belong to the structure factors"):
            md.DeviceMD(Recorder(), atoms, md.fs, **extra)
    with pytest.raises(ValueError, match=r"sq_miller \(structure factors\) excludes the barostat"):
        md.DeviceMD(Recorder(), atoms, md.fs, sq_miller=ok, pressure=0.0, taup=100 * md.fs, compressibility=1.0)
    with pytest.raises(AssertionError, match="reached the engine"):   # a valid request gets through
        md.DeviceMD(Recorder(), atoms, md.fs, sq_miller=ok, sq_lags=4096, sq_every=7, sq_currents=True)


def test_device_md_hands_a_valid_request_to_md_set_sq():
    """An engine stand-in that plays along until `md_set_sq`: it is reached with the arguments as given, and an
    engine without any of the new methods serves a DeviceMD that does not ask for structure factors."""
    from tests.helpers import fcc
    atoms = fcc(rep=(1, 1, 1))
    calls = []

    class Reached(Exception):
        pass

    class Old:   # the engine as it was before the structure factors
        def _ok(self, *a, **k):
            return None
        set_frames = md_init = md_set_thermostat = md_set_langevin = md_set_nose_hoover = md_set_barostat = _ok
        md_set_sampling = _ok

        def md_run(self, n, dt, **k):
            raise Reached("md_run")

    class New(Old):
        def md_set_sq(self, *a):
            calls.append(a)
            raise Reached("md_set_sq")

    miller = [[1, 0, 0], [0, 2, -1]]
    with pytest.raises(Reached, match="md_set_sq"):
        md.DeviceMD(New(), atoms, md.fs, sq_miller=miller, sq_lags=16, sq_every=3, sq_currents=True)
    assert calls[0][0].dtype == np.int32 and np.array_equal(calls[0][0], miller) and calls[0][1:] == (16, 3, True)
    with pytest.raises(Reached, match="md_set_sq"):
        md.DeviceMD(New(), atoms, md.fs, sq_miller=np.array(miller, dtype=np.int64))
    assert calls[1][1:] == (1, 1, False)   # (the static structure factor alone)
    with pytest.raises(Reached, match="md_run"):   # nothing new is called when sq_miller is None
        md.DeviceMD(Old(), atoms, md.fs)
    with pytest.raises(Reached, match="md_run"):
        md.DeviceMD(New(), atoms, md.fs, n_lags=8)
    assert len(calls) == 2

    class LeftOn(New):   # an engine on which an earlier DeviceMD left the structure factors on says so ...
        md_sq_vectors = 64

    with pytest.raises(Reached, match="md_set_sq"):   # ... and is told to switch them off: the one deliberate call
        md.DeviceMD(LeftOn(), atoms, md.fs)
    assert calls[2] == (None,)


def test_abi_of_the_sq_calls(lib):
    from tensoralloy_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "tensoralloy_amd.h")) as fp:
        header = re.sub(r"/\*.*?\*/", "", fp.read(), flags=re.S)
    for name in ("ta_md_set_sq", "ta_md_get_sq", "ta_md_get_sq_amplitudes"):
        assert re.search(r"\bint %s\s*\(ta_handle h," % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert re.search(r"^#define TA_MD_SQ_MAX_Q 4096$", header, re.M) and _lib.TA_MD_SQ_MAX_Q == 4096
    assert re.search(r"^#define TA_MD_SQ_MAX_INDEX 64$", header, re.M) and _lib.TA_MD_SQ_MAX_INDEX == 64
    assert re.search(r"^#define TA_ABI_VERSION 5$", header, re.M) and _lib.TA_ABI_VERSION == 5
    struct = re.search(r"typedef struct \{([^}]*)\} ta_md_sq_params;", header).group(1)
    names = ["n_q", "n_lags", "sample_every", "currents"]
    assert re.findall(r"\bint32_t\s+(\w+);", struct) == names
    assert C.sizeof(_lib.MdSqParams) == 16 and [f[0] for f in _lib.MdSqParams._fields_] == names
    assert [getattr(_lib.MdSqParams, n).offset for n in names] == [0, 4, 8, 12]
    assert "ta_md_sq.hip" in _lib.SOURCES
