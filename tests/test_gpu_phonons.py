"""Harmonic phonons on the device (`ta_phonon_*`, csrc/ta_phonon.hip) against tests/phonon_reference.py.

The unit of every bound on the eigensolver is u = n eps ||A||_F per matrix. The margin is not chosen: NumPy's
own error against mpmath (50 digits) is measured in that unit on the matrices of order <= 12 (`numpy_margin`,
0.37 when this was written), and the device gets MARGIN = 4 x max(that, 1) units against mpmath; against NumPy
the triangle inequality adds NumPy's own share. Jacobi is at least as accurate as LAPACK's tridiagonal path, so
a small factor suffices."""
import itertools
import os

import numpy as np
import pytest

from tests import phonon_reference as R
from tests.conftest import GOLDEN
from tests.helpers import fcc, make_eam, make_nn

pytestmark = pytest.mark.gpu

EPS = R.EPS
NI_MASS = 58.6934


@pytest.fixture(scope="module")
def margins():
    ref_set = R.mp_reference_set()
    r_np = R.numpy_margin(ref_set)
    dev = 4.0 * max(r_np, 1.0)
    print(f"numpy-vs-mpmath {r_np:.3f} u -> device margin {dev:.3f} u")
    return {"set": {(n, kind): (A, w) for n, kind, A, w in ref_set}, "numpy": r_np, "device": dev}


@pytest.fixture(scope="module")
def engine(lib):
    from tensoralloy_amd import Engine
    with Engine(make_eam(["Ni"], 6.0)) as eng:
        yield eng


@pytest.fixture(scope="module")
def fixture_phonons(engine):
    """The reference's force constants (a 2 x 2 x 2 supercell of the cubic 4-atom Ni cell) loaded into the device
    slot, with everything the restatement needs beside them."""
    from tensoralloy_amd import Atoms
    from tensoralloy_amd.phonons import Phonons
    d = np.load(os.path.join(GOLDEN, "Ni_fc2.npz"))
    fc2, frac, cell = d["fc2"].astype(np.float64), d["frac"], d["cell"]
    sup = Atoms(symbols=["Ni"] * 32, positions=frac @ cell, cell=cell, pbc=True)
    basis_of, moved = R.translation_table(frac, 4, (2, 2, 2))
    ph = Phonons.from_force_constants(engine, fc2, sup, 4, supercell=(2, 2, 2), mapping=basis_of, masses=[NI_MASS] * 4,
                                      q_chunk=64)
    images = R.shortest_images(sup.positions, cell, 4)
    return {"ph": ph, "phi": np.ascontiguousarray(fc2[:4]), "fc2": fc2, "basis_of": basis_of, "moved": moved,
            "images": images, "masses": np.full(4, NI_MASS), "sup": sup}


# -- 1. the eigensolver alone ---------------------------------------------------------------------

@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("n", [1, 2, 3, 9, 12, 47, 48])
def test_eigh(lib, engine, margins, n, kind):
    group = lib.ta_phonon_eigh_group(n)
    assert group >= 1
    M, r_np = margins["device"], margins["numpy"]
    for batch in (1, 2 * group + 1):
        A = R.eigh_cases(n, batch, kind)
        w, V, info = engine.phonon_eigh(A)
        w_only, none, info2 = engine.phonon_eigh(A, eigenvectors=False)
        assert info == 0 and info2 == 0 and none is None
        u = R.unit_of(A)                                       # [batch]
        assert np.all(np.abs(w - w_only).max(axis=1) <= M * u)   # the build without V: the same rotations
        assert np.all(np.diff(w, axis=1) >= 0.0)
        w_np = np.linalg.eigvalsh(A)
        err = np.abs(w - w_np).max(axis=1)
        res = np.array([np.linalg.norm(a @ v.T - v.T * wk[None, :], axis=0).max() for a, v, wk in zip(A, V, w)])
        orth = np.array([np.abs(v.conj() @ v.T - np.eye(n)).max() for v in V])
        scale = np.where(u > 0, u, 1.0)
        print(f"n {n} {kind} batch {batch}: eig vs numpy {np.max(err / scale):.3f} u, residual "
              f"{np.max(res / scale):.3f} u, orthogonality {orth.max() / (n * EPS):.3f} n eps")
        assert np.all(err <= (M + max(r_np, 1.0)) * u)
        assert np.all(res <= M * u)
        assert np.all(orth <= M * n * EPS)
        if n <= 12:
            A_mp, w_mp = margins["set"][(n, kind)]
            k = min(batch, len(A_mp))
            assert np.array_equal(A[:k], A_mp[:k])
            err_mp = np.abs(w[:k] - w_mp[:k]).max(axis=1)
            print(f"    vs mpmath {np.max(err_mp / scale[:k]):.3f} u")
            assert np.all(err_mp <= M * u[:k])


def test_eigh_takes_the_hermitian_part_and_refuses_orders_above_the_cap(engine, margins):
    rng = np.random.RandomState(3)
    X = rng.normal(size=(5, 6, 6)) + 1j * rng.normal(size=(5, 6, 6))
    w, _, info = engine.phonon_eigh(X)
    H = 0.5 * (X + X.conj().transpose(0, 2, 1))
    assert info == 0 and np.all(np.abs(w - np.linalg.eigvalsh(H)).max(axis=1) <= (margins["device"] + max(margins["numpy"], 1.0)) * R.unit_of(H))
    with pytest.raises(ValueError, match="cap"):
        engine.phonon_eigh(np.zeros((1, 49, 49), dtype=complex))


# -- 2. the reference's force constants -------------------------------------------------------------

def _lambda_bound(fx, D_norm, margin, n):
    """|lambda_device - lambda_reference|: the solver's bound, margin n eps ||D||_F, plus the rounding of D(q)
    itself, margin eps sum |Phi| / m."""
    return margin * (n * EPS * D_norm + EPS * np.abs(fx["phi"]).sum() / fx["masses"].min())


def _union_bound(fx, H_circ, margins, n, n_full):
    """The same for the union over the commensurate q against `eigvalsh` of the full n_full x n_full matrix:
    the blocks D(q) are a unitary transform of H_circ, so ||D(q)||_F <= ||H_circ||_F; the device's share is its
    margin in units of order n, NumPy's its measured one (at least 1) in units of order n_full."""
    norm = np.linalg.norm(H_circ)
    return (margins["device"] * n + max(margins["numpy"], 1.0) * n_full) * EPS * norm + \
        margins["device"] * EPS * np.abs(fx["phi"]).sum() / fx["masses"].min()


def _compare_frequencies(fx, q_red, margins):
    ph, n = fx["ph"], 12
    q_red = np.asarray(q_red, dtype=float).reshape(-1, 3)
    nu = ph.frequencies(q_red)
    assert nu.shape == (len(q_red), n)
    worst = 0.0
    for q, got in zip(q_red, nu):
        D = R.dynamical_matrix(fx["phi"], fx["basis_of"], fx["masses"], fx["images"], q @ ph.recip)
        lam = R.eigenvalues(D)
        D_norm = np.linalg.norm(0.5 * (D + D.conj().T))
        tol = _lambda_bound(fx, D_norm, margins["device"] + max(margins["numpy"], 1.0), n)
        # in lambda, every mode (the conversion back costs a few eps |lambda|)
        d_lam = np.abs(R.from_thz(got) - lam)
        worst = max(worst, (d_lam / tol).max())
        assert np.all(d_lam <= tol + 8 * EPS * np.abs(lam)), (q, d_lam.max(), tol)
        # in nu, through |sqrt a - sqrt b| <= |a - b| / sqrt(max(a, floor)), for the modes that are not at zero:
        # those within the floor n eps ||D|| (acoustic modes at Gamma) are compared in lambda alone
        floor = max(n * EPS * D_norm, 100.0 * tol)
        big = np.abs(lam) > floor
        tol_nu = R.THZ * tol / np.sqrt(np.maximum(np.abs(lam), floor)) + 8 * EPS * np.abs(R.to_thz(lam))
        assert np.all(np.abs(got - R.to_thz(lam))[big] <= tol_nu[big]), (q, got, R.to_thz(lam))
    print(f"{len(q_red)} q-points: worst |d lambda| = {worst:.3f} of the bound")
    return nu


def test_fixture_frequencies_at_special_and_general_points(fixture_phonons, margins):
    q = [[0, 0, 0], [0.5, 0, 0], [0.5, 0.5, 0], [0.5, 0.5, 0.5], [0.3, 0.1, 0.2], [-0.41, 0.27, 0.05], [1.3, -2.1, 0.2]]
    nu = _compare_frequencies(fixture_phonons, q, margins)
    # what the reference's fixture gives (checked on the CPU): Gamma 0.002 x 3, 6.445 x 6, 9.553 x 3; X 4.668 x 4
    assert np.all(np.abs(nu[0][:3]) < 0.005)
    assert np.allclose(nu[0][3:9], 6.445, atol=1e-3) and np.allclose(nu[0][9:], 9.553, atol=1e-3)
    assert np.allclose(nu[1][:4], 4.668, atol=1e-3)


def test_fixture_band_path(fixture_phonons, margins):
    ph = fixture_phonons["ph"]
    dist, nu = ph.band_structure([[[0, 0, 0], [0.5, 0, 0]]], npoints=11)
    assert dist.shape == (11,) and nu.shape == (11, 12)
    assert abs(dist[-1] - np.pi / 3.52) < 1e-12
    q = np.linspace(0, 1, 11)[:, None] * np.array([[0.5, 0, 0]])
    assert np.array_equal(nu, _compare_frequencies(fixture_phonons, q, margins))


def test_fixture_commensurate_points_give_the_supercell_spectrum(fixture_phonons, margins):
    """The 96 eigenvalues of the full mass-weighted supercell Hessian = the union over the 8 commensurate q of the
    12 eigenvalues of D(q): independent of the image convention, since every image of a pair has the same phase
    there. Exactly so for the Hessian the home rows imply under the lattice translations (H_circ); the fixture's
    own 32 x 32 blocks differ from that by its float32 noise, which Weyl's inequality bounds by
    ||H_full - H_circ||_2 (2.6e-7 here), a property of the fixture."""
    fx = fixture_phonons
    ph = fx["ph"]
    q = np.array(list(itertools.product([0.0, 0.5], repeat=3)))
    nu, vec = ph.frequencies(q, eigenvectors=True)
    lam = np.sort(R.from_thz(nu).reshape(-1))
    masses = np.full(32, NI_MASS)
    H_circ = R.mass_weighted(R.circulant_hessian(fx["phi"], fx["moved"], 4), masses)
    H_full = R.mass_weighted(fx["fc2"].transpose(0, 2, 1, 3), masses)
    tol = _union_bound(fx, H_circ, margins, 12, 96)
    e_circ = np.linalg.eigvalsh(H_circ)
    print(f"union vs circulant {np.abs(lam - e_circ).max():.3e} (bound {tol:.3e})")
    assert np.all(np.abs(lam - e_circ) <= tol + 8 * EPS * np.abs(e_circ))
    weyl = np.linalg.norm(H_full - H_circ, 2)
    assert weyl < 1e-6
    assert np.all(np.abs(lam - np.linalg.eigvalsh(H_full)) <= weyl + tol)
    # the modes: unit rows, and D v = lambda v against the restatement's D
    for qi, (qr, w, V) in enumerate(zip(q, R.from_thz(nu), vec)):
        D = R.dynamical_matrix(fx["phi"], fx["basis_of"], fx["masses"], fx["images"], qr @ ph.recip)
        D = 0.5 * (D + D.conj().T)
        u = 12 * EPS * np.linalg.norm(D)
        assert np.abs(V.conj() @ V.T - np.eye(12)).max() <= margins["device"] * 12 * EPS
        res = np.linalg.norm(D @ V.T - V.T * w[None, :], axis=0).max()
        assert res <= _lambda_bound(fx, np.linalg.norm(D), margins["device"] + 1.0, 12) + 8 * EPS * np.abs(w).max(), (qi, res, u)


# -- 3. end to end with a model -------------------------------------------------------------------

def _model_case(kind):
    from tensoralloy_amd import Atoms
    if kind == "eam_ni_fcc":      # one-atom fcc primitive cell, 3 x 3 x 3: n = 3, N = 27
        a = 3.52
        home = Atoms(symbols=["Ni"], positions=[[0.0, 0.0, 0.0]],
                     cell=np.array([[0, a / 2, a / 2], [a / 2, 0, a / 2], [a / 2, a / 2, 0]]), pbc=True)
        return make_eam(["Ni"], 6.0), home, (3, 3, 3)
    a = 3.1                       # B2 MoNi with the Ni atom off the body centre, 2 x 2 x 2: n = 6, N = 16
    home = Atoms(symbols=["Mo", "Ni"], positions=[[0.0, 0.0, 0.0], [0.52 * a, 0.49 * a, 0.5 * a]], cell=np.eye(3) * a,
                 pbc=True)
    return make_nn(["Mo", "Ni"], 4.5, kind == "sf_moni_b2_angular", [16, 16]), home, (2, 2, 2)


@pytest.mark.parametrize("kind", ["eam_ni_fcc", "sf_moni_b2", "sf_moni_b2_angular"])
def test_model_force_constants_and_commensurate_frequencies(lib, margins, kind):
    """The device slot holds -dF of `ta_hessian_vectors` for the unit displacements of the home cell: bit for bit
    what a separate `Engine.hessian_vectors()` call returns, for the models whose evaluation is deterministic (EAM,
    radial symmetry functions). The angular forward sweep accumulates descriptors with LDS floating-point atomics,
    so two evaluations of such a model differ in the last bits of their sums whoever asks; there the comparison
    allows 64 eps of the largest force constant (last-bit differences of sums of some tens of terms)."""
    from tensoralloy_amd import Engine
    from tensoralloy_amd.atoms import atomic_masses
    from tensoralloy_amd.phonons import Phonons
    nn, home, reps = _model_case(kind)
    nb, n = len(home), 3 * len(home)
    with Engine(nn) as eng:
        ph = Phonons(eng, home, supercell=reps)
        N = len(ph.super_atoms)
        dF = eng.hessian_vectors()                                   # [3 N, N, 3], the same resident frame
        phi = ph.force_constants
        assert phi.shape == (nb, N, 3, 3)
        want = -dF[:n].reshape(nb, 3, N, 3).transpose(0, 2, 1, 3)
        if kind.endswith("angular"):
            assert np.abs(phi - want).max() <= 64 * EPS * np.abs(want).max()
        else:
            assert np.array_equal(phi, want)                         # bit for bit
            assert np.array_equal(eng.phonon_force_constants(), want)
        frac = np.linalg.solve(np.asarray(ph.super_atoms.get_cell(complete=True)).T, ph.super_atoms.positions.T).T
        basis_of, moved = R.translation_table(frac, nb, reps)
        assert np.array_equal(basis_of, ph.basis_of)
        q = np.array(list(itertools.product(*[np.arange(r) / r for r in reps])))
        nu = ph.frequencies(q)
        nu_gamma = nu[0]
    masses = np.array([atomic_masses[z] for z in ph.super_atoms.numbers])
    H_full = R.mass_weighted((-dF).reshape(N, 3, N, 3), masses)
    H_circ = R.mass_weighted(R.circulant_hessian(phi, moved, nb), masses)
    fx = {"phi": phi, "masses": masses[:nb]}
    tol = _union_bound(fx, H_circ, margins, n, 3 * N)
    lam = np.sort(R.from_thz(nu).reshape(-1))
    e_circ = np.linalg.eigvalsh(H_circ)
    # a model's Hessian is translation invariant to rounding: the distance to the circulant form is of that size
    weyl = np.linalg.norm(H_full - H_circ, 2)
    print(f"{kind}: union vs circulant {np.abs(lam - e_circ).max():.3e} (bound {tol:.3e}), Weyl distance {weyl:.3e}")
    assert weyl < 1e-9 * max(1.0, np.abs(e_circ).max())
    assert np.all(np.abs(lam - e_circ) <= tol + 8 * EPS * np.abs(e_circ))
    assert np.all(np.abs(lam - np.linalg.eigvalsh(H_full)) <= tol + weyl + 8 * EPS * np.abs(e_circ))
    # acoustic modes at Gamma: D(0) = sum_s Phi(b, s) / m, zero by the sum rule up to the rounding of the sum
    lam_gamma = R.from_thz(nu_gamma)
    acoustic = np.sort(np.abs(lam_gamma))[:3]
    sum_rule = np.abs(phi.sum(axis=1)).max() / masses[:nb].min()     # what the model's own Phi leaves at q = 0
    assert np.all(acoustic <= tol + 3 * nb * sum_rule), (acoustic, tol, sum_rule)


def test_cluster_frequencies_and_normal_modes_through_the_calculator(lib, margins, tmp_path):
    from tensoralloy_amd import Atoms, TensorAlloyCalculator, UniversalTransformer
    from tensoralloy_amd.atoms import atomic_masses
    from tensoralloy_amd.eam import EamAlloyNN
    from tensoralloy_amd.phonons import THZ, THZ_TO_CM
    nn = EamAlloyNN(["Ni"], "zjw04", export_properties=["energy", "forces", "hessian"])
    nn.attach_transformer(UniversalTransformer(["Ni"], rcut=6.0))
    calc = TensorAlloyCalculator(nn.export(str(tmp_path / "Ni_cluster")))
    pos = np.array([[0, 0, 0], [2.4, 0.1, 0], [1.1, 2.2, 0.2], [1.2, 0.8, 2.1], [3.1, 2.0, 1.9]]) + 8.0
    atoms = Atoms(symbols=["Ni"] * 5, positions=pos, cell=np.eye(3) * 20.0, pbc=False)
    freq, modes = calc.get_frequencies_and_normal_modes(atoms)
    assert freq.shape == (15,) and modes.shape == (15, 15)
    inv = 1.0 / np.sqrt(np.repeat([atomic_masses[28]] * 5, 3))
    H = calc.get_hessian(atoms)
    Hm = 0.5 * (H + H.T) * inv[:, None] * inv[None, :]
    lam = np.linalg.eigvalsh(Hm)
    u = 15 * EPS * np.linalg.norm(Hm)
    got = np.sign(freq) * (np.abs(freq) / (THZ * THZ_TO_CM)) ** 2
    # the device's margin, NumPy's own share, and one unit for the two roundings of the mass weighting
    M = margins["device"] + max(margins["numpy"], 1.0) + 1.0
    assert np.all(np.abs(got - lam) <= M * u + 8 * EPS * np.abs(lam)), np.abs(got - lam).max() / u
    assert np.abs(modes.conj() @ modes.T - np.eye(15)).max() <= margins["device"] * 15 * EPS
    assert np.linalg.norm(Hm @ modes.T - modes.T * got[None, :], axis=0).max() <= M * u
    assert np.all(np.abs(freq[np.argsort(np.abs(got))[:3]]) < 1e-3)   # three rigid translations cost nothing


def test_models_without_analytic_second_derivatives_are_refused(lib):
    from tensoralloy_amd import Atoms, Engine
    from tensoralloy_amd.phonons import Phonons
    from tests.test_gpu_eam_fs import _random_nn
    home = Atoms(symbols=["Al", "Fe"], positions=[[0, 0, 0], [1.45, 1.45, 1.45]], cell=np.eye(3) * 2.9, pbc=True)
    with Engine(_random_nn(["Al", "Fe"])) as eng:
        with pytest.raises(ValueError, match="eam/fs"):
            Phonons(eng, home, supercell=(2, 2, 2))


# -- 4. density of states -------------------------------------------------------------------------

def test_dos_counts_partial_weights_and_chunking(fixture_phonons, engine, margins):
    from tensoralloy_amd.phonons import mesh_points
    fx = fixture_phonons
    ph = fx["ph"]                                   # q_chunk = 64: the 216 q-points take four passes
    q = mesh_points(6, 6, 6, shift=True)
    nu = ph.frequencies(q)
    assert nu.shape == (216, 12)
    lo, hi, bins = 2.0, 9.0, 70                     # modes below 2 and above 9 THz fall outside
    k = R.bin_index(nu.reshape(-1), lo, hi, bins)
    want = np.bincount(k[k >= 0], minlength=bins)
    outside = int((k < 0).sum())
    assert 0 < outside < 2592 and want.sum() + outside == 2592
    out = ph.dos((6, 6, 6, True), bins, (lo, hi), partial=True)
    assert out["total"].dtype == np.uint64 and np.array_equal(out["total"].astype(np.int64), want)
    assert out["outside"] == outside and out["n_q"] == 216
    assert np.array_equal(ph.dos(q, bins, (lo, hi))["total"], out["total"])     # without the eigenvectors
    # every mode's weights sum to |e|^2 = 1 up to the eigenvectors' normalisation, n eps per mode
    assert out["partial"].shape == (4, bins)
    assert np.all(np.abs(out["partial"].sum(axis=0) - want) <= margins["device"] * 12 * EPS * np.maximum(want, 1))
    assert np.all(out["partial"] >= 0.0)
    # one pass over all q-points: the same bits
    engine.phonon_set_cell(4, ph.basis_of, ph.masses, ph.start, ph.vectors, q_chunk=0)
    engine.phonon_load_force_constants(fx["phi"])
    try:
        whole = ph.dos(q, bins, (lo, hi), partial=True)
        assert np.array_equal(ph.frequencies(q), nu)
        assert np.array_equal(whole["total"], out["total"]) and whole["outside"] == outside
        assert np.array_equal(whole["partial"], out["partial"])
    finally:
        engine.phonon_set_cell(4, ph.basis_of, ph.masses, ph.start, ph.vectors, q_chunk=64)
        engine.phonon_load_force_constants(fx["phi"])


# -- 5. refusals ------------------------------------------------------------------------------------

def test_refusals(lib):
    from tensoralloy_amd import Engine
    from tensoralloy_amd.phonons import shortest_vectors
    atoms = fcc(rep=(1, 1, 1), jitter=0.0)
    cell = np.asarray(atoms.get_cell(complete=True))
    start, vec = shortest_vectors(atoms.positions, cell, 4)
    masses = [NI_MASS] * 4
    with Engine(make_eam(["Ni"], 6.0)) as eng:
        with pytest.raises(ValueError, match="no resident batch"):
            eng.phonon_set_cell(4, np.arange(4), masses, start, vec)
        eng.set_frames([atoms, atoms])                                          # two resident frames
        s8, v8 = shortest_vectors(np.concatenate([atoms.positions] * 2), cell, 4)
        with pytest.raises(ValueError, match="ONE frame"):
            eng.phonon_set_cell(4, np.arange(8) % 4, masses, s8, v8)
        big = fcc(rep=(3, 3, 2), jitter=0.0)                                    # 72 atoms, all of them home cell
        eng.set_frames([big])
        sb, vb = shortest_vectors(big.positions, np.asarray(big.get_cell(complete=True)), 17)
        with pytest.raises(ValueError, match="cap"):
            eng.phonon_set_cell(17, np.arange(72) % 17, [NI_MASS] * 17, sb, vb)
        eng.set_frames([atoms])
        with pytest.raises(ValueError, match="before phonon_set_cell"):
            eng.phonon_frequencies(np.zeros((1, 3)))
        bad = start.copy()
        bad[5] = bad[4] - 1
        with pytest.raises(ValueError, match="not monotone"):
            eng.phonon_set_cell(4, np.arange(4), masses, bad, vec)
        with pytest.raises(ValueError, match="home-cell atom"):
            eng.phonon_set_cell(4, [0, 1, 2, 4], masses, start, vec)
        eng.phonon_set_cell(4, np.arange(4), masses, start, vec)
        with pytest.raises(ValueError, match="no force constants"):
            eng.phonon_frequencies(np.zeros((1, 3)))
        with pytest.raises(ValueError, match="no force constants"):
            eng.phonon_dos(np.zeros((1, 3)), 10, 0.0, 10.0)
        eng.phonon_force_constants()
        assert eng.phonon_frequencies(np.zeros((1, 3))).shape == (1, 12)
        with pytest.raises(ValueError, match="n_bins"):
            eng.phonon_dos(np.zeros((1, 3)), 0, 0.0, 10.0)
        eng.set_frames([atoms])                                                 # drops the phonon state
        with pytest.raises(ValueError, match="before phonon_set_cell"):
            eng.phonon_force_constants()
