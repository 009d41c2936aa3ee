"""NumPy restatement of the harmonic-phonon path (test infrastructure only): the definition of D(q) with its own
image search, `eigvalsh`, the binning expression, the closed-form thermal properties of one oscillator, and an
mpmath eigenvalue reference at 50 digits for small matrices.

    D(q)[3b+a, 3b'+c] = (m_b m_b')^(-1/2) sum_{s: basis_of[s] = b'} Phi_ac(b, s) (1/mult) sum_r exp(i q.r)

with r over the shortest vectors from home atom b to the periodic images of supercell atom s (all images whose
length is within `symprec` of the minimum)."""
import itertools

import numpy as np

EPS = np.finfo(np.float64).eps
THZ = 1000.0 * 0.09822694788464063 / (2.0 * np.pi)   # THz per sqrt(eV / A^2 / amu), fs of tensoralloy_amd.md
THZ_TO_EV = 4.135667696e-3
KB = 8.617333262e-5


def shortest_images(positions, cell, n_basis, pbc=(True, True, True), symprec=1e-5):
    """images[b][s] = list of the shortest vectors from atom b to the images of atom s (plain loops)."""
    positions, cell = np.asarray(positions, float), np.asarray(cell, float)
    rng = [(-1, 0, 1) if p else (0,) for p in pbc]
    out = []
    for b in range(n_basis):
        row = []
        for s in range(len(positions)):
            cand = [positions[s] - positions[b] + np.array(t, float) @ cell for t in itertools.product(*rng)]
            lens = [np.sqrt(v @ v) for v in cand]
            lo = min(lens)
            row.append([v for v, l in zip(cand, lens) if l - lo < symprec])
        out.append(row)
    return out


def dynamical_matrix(phi, basis_of, masses, images, q_cart):
    """D(q) [n, n] complex from phi [n_basis, N, 3, 3]."""
    nb, N = phi.shape[0], phi.shape[1]
    D = np.zeros((3 * nb, 3 * nb), dtype=complex)
    for b in range(nb):
        for s in range(N):
            bp = basis_of[s]
            vecs = np.array(images[b][s])
            phase = np.exp(1j * (vecs @ q_cart)).sum() / len(vecs)
            D[3 * b:3 * b + 3, 3 * bp:3 * bp + 3] += phi[b, s] * phase / np.sqrt(masses[b] * masses[bp])
    return D


def eigenvalues(D):
    return np.linalg.eigvalsh(0.5 * (D + D.conj().T))


def to_thz(lam):
    return np.sign(lam) * np.sqrt(np.abs(lam)) * THZ


def from_thz(nu):
    return np.sign(nu) * (np.abs(nu) / THZ) ** 2


def bin_index(nu, nu_min, nu_max, n_bins):
    """The library's binning expression: a subtraction, then a multiplication, then floor. -1 = outside."""
    inv = float(n_bins) / (float(nu_max) - float(nu_min))
    x = (np.asarray(nu, float) - float(nu_min)) * inv
    k = np.floor(x)
    return np.where((x >= 0.0) & (x < n_bins), k, -1).astype(np.int64)


def einstein(nu_thz, T):
    """(F eV, S eV/K, C_v eV/K) of ONE harmonic oscillator of frequency nu at temperature T > 0, closed form."""
    e = nu_thz * THZ_TO_EV
    x = e / (KB * T)
    F = 0.5 * e + KB * T * np.log(1.0 - np.exp(-x))
    S = KB * (x / (np.exp(x) - 1.0) - np.log(1.0 - np.exp(-x)))
    Cv = KB * x * x * np.exp(x) / (np.exp(x) - 1.0) ** 2
    return F, S, Cv


def translation_table(frac, n_basis, reps):
    """For the supercell of `reps` repeats whose first n_basis atoms are the home cell: (basis_of [N],
    moved [T, N]) with moved[t][s] = the atom that s lands on under lattice translation t (t = 0 first), and
    image_of [T, n_basis] = the atom that home atom b lands on. From fractional coordinates of the supercell."""
    frac = np.asarray(frac, float)
    reps = np.asarray(reps)
    N = len(frac)

    def find(x):
        d = frac - x[None, :]
        d -= np.rint(d)
        i = np.argmin((d ** 2).sum(1))
        assert (d[i] ** 2).sum() < 1e-10
        return i
    shifts = [np.array(t, float) / reps for t in itertools.product(*[range(r) for r in reps])]
    moved = np.array([[find(frac[s] + t) for s in range(N)] for t in shifts])
    basis_of = np.zeros(N, dtype=np.int64)
    for t in range(len(shifts)):
        for b in range(n_basis):
            basis_of[moved[t][b]] = b
    return basis_of, moved


def circulant_hessian(phi_rows, moved, n_basis):
    """The full [N, 3, N, 3] Hessian that the home rows imply under the supercell's lattice translations:
    H[T b, T s] = Phi(b, s) for every translation T."""
    N = phi_rows.shape[1]
    H = np.zeros((N, 3, N, 3))
    for t in range(len(moved)):
        for b in range(n_basis):
            for s in range(N):
                H[moved[t][b], :, moved[t][s], :] = phi_rows[b, s]
    return H


def mass_weighted(H, masses_all):
    n = len(masses_all)
    inv = 1.0 / np.sqrt(np.repeat(masses_all, 3))
    M = H.reshape(3 * n, 3 * n) * inv[:, None] * inv[None, :]
    return 0.5 * (M + M.T)


# -- eigensolver cases --------------------------------------------------------------------------
KINDS = ("random", "diagonal", "zero", "degenerate")


def eigh_cases(n, batch, kind, seed=0):
    """[batch, n, n] complex Hermitian test matrices. `degenerate`: eigenvalues in 8-fold degenerate groups
    (n-fold below 8) under a random unitary, plus a Hermitian perturbation of 1e-9."""
    rng = np.random.RandomState(1000 * n + 7 * KINDS.index(kind) + seed)
    A = np.zeros((batch, n, n), dtype=complex)
    for k in range(batch):
        X = rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n))
        H = 0.5 * (X + X.conj().T)
        if kind == "random":
            A[k] = H
        elif kind == "diagonal":
            A[k] = np.diag(rng.normal(size=n) * 10.0 ** rng.randint(-3, 4))
        elif kind == "degenerate":
            U = np.linalg.qr(X)[0]
            d = np.repeat(rng.normal(size=(n + 7) // 8), 8)[:n]
            B = (U * d[None, :]) @ U.conj().T + 1e-9 * H
            A[k] = 0.5 * (B + B.conj().T)
    return A


def unit_of(A):
    """n eps ||A||_F per matrix: the unit of every bound on the eigensolver."""
    n = A.shape[-1]
    return n * EPS * np.sqrt((np.abs(A) ** 2).sum(axis=(-2, -1)))


def mp_eigvalsh(A, digits=50):
    """Ascending eigenvalues of one Hermitian matrix (order <= 12) by mpmath at `digits` digits, as floats."""
    import mpmath
    assert A.shape[0] <= 12
    with mpmath.workdps(digits):
        M = mpmath.matrix(A.shape[0], A.shape[1])
        for i in range(A.shape[0]):
            for j in range(A.shape[1]):
                M[i, j] = mpmath.mpc(A[i, j].real, A[i, j].imag)
        E = mpmath.mp.eigh(M, eigvals_only=True)
        return np.array(sorted(float(mpmath.re(e)) for e in E))


MP_ORDERS = (1, 2, 3, 9, 12)
MP_PER_CASE = 2   # matrices per (order, kind) that get the mpmath reference


def mp_reference_set():
    """[(n, kind, A [MP_PER_CASE, n, n], w_mp [MP_PER_CASE, n])] for the orders <= 12: computed once, shared."""
    out = []
    for n in MP_ORDERS:
        for kind in KINDS:
            A = eigh_cases(n, MP_PER_CASE, kind)
            out.append((n, kind, A, np.array([mp_eigvalsh(a) for a in A])))
    return out


def numpy_margin(ref_set):
    """max over the mpmath set of |eigvalsh - mpmath| / (n eps ||A||_F): NumPy's own error in the tests' unit
    (matrices of norm 0 excluded)."""
    worst = 0.0
    for n, kind, A, w_mp in ref_set:
        u = unit_of(A)
        for a, w, ui in zip(A, w_mp, u):
            if ui > 0.0:
                worst = max(worst, np.abs(np.linalg.eigvalsh(a) - w).max() / ui)
    return worst
