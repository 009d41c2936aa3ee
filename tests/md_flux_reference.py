"""Reference for the heat current and the pressure tensor of the device MD loop (`ta_md_set_flux`): NumPy and the
project's CPU oracles, nothing of the library.

A sample's row is {J_conv[3], J_pot[3], K[6], W[6]} (six components: xx yy zz yz xz xy) with
    J_conv = sum_i (1/2 m_i |v_i|^2 + e_i) v_i             K_ab = sum_i m_i v_ia v_ib
    J_pot  = sum_i sum_j d_ji (de_j/dr_i . v_i)            W_ab = - sym sum_i sum_j d_ji,a de_j/dr_i,b
where d_ji is r_j - r_i (its minimum image in a periodic frame, whose cell heights must all exceed twice the cutoff).
The matrix de_j/dr_i comes from central differences of the oracle's `atomic` energies at the steps h, 2h and 4h,
Richardson-extrapolated over (h, 2h); the same extrapolation over (2h, 4h) gives the reference's own uncertainty,
which is propagated to every one of the 18 numbers and is the bound of a comparison, together with a rounding term
2^-53 x (additions in the longest chain) x (sum of the |terms| of the number). A free cluster also has the identity
    J_pot = sum_j r_j d/d eps e_j(x + eps v) + sum_i r_i (F_i . v_i)
which needs one directional derivative only."""
import numpy as np

H = 1e-3
COMPONENTS = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))   # xx yy zz yz xz xy


def oracle_for(nn, atoms):
    """x [N, 3] -> the oracle's dict (atomic, forces, virial) of `atoms` moved to x, for every model kind."""
    from tests import helpers
    from tensoralloy_amd.eam import EamAlloyNN, AdpNN
    symbols, cell, pbc = atoms.get_chemical_symbols(), np.asarray(atoms.get_cell(complete=True)), atoms.pbc
    eps = 1e-8 if getattr(nn, "precision", "high") == "medium" else 1e-14
    if type(nn).__name__ == "EamFsNN":
        from tests.fs_reference import fs_evaluate
        from tensoralloy_amd import Atoms
        return lambda x: fs_evaluate(nn, Atoms(symbols=symbols, positions=x, cell=cell, pbc=pbc))
    if isinstance(nn, (EamAlloyNN, AdpNN)):
        from oracle.eam import evaluate
        model = helpers.oracle_eam_model(nn)
        return lambda x: evaluate(model, symbols, x, cell, pbc, eps=eps)
    if type(nn.descriptor).__name__ == "GenericRadialAtomicPotential":
        from oracle.grap import evaluate
        model = helpers.oracle_grap_model(nn)
        return lambda x: evaluate(model, symbols, x, cell, pbc, eps=eps)
    from oracle.sf import evaluate
    model = helpers.oracle_model(nn)
    return lambda x: evaluate(model, symbols, x, cell, pbc, want_forces=True, eps=eps)


def _central(atomic, x, h):
    n = len(x)
    m = np.zeros((n, n, 3))   # [j, i, c] = d e_j / d x_ic
    for i in range(n):
        for c in range(3):
            xp, xm = x.copy(), x.copy()
            xp[i, c] += h
            xm[i, c] -= h
            m[:, i, c] = (atomic(xp) - atomic(xm)) / (2.0 * h)
    return m


def energy_matrix(evaluate, x, h=H):
    """(M, dM): d e_j / d x_ic [j, i, c] extrapolated over (h, 2h), and its distance from the one over (2h, 4h)."""
    atomic = lambda y: np.asarray(evaluate(y)["atomic"], dtype=np.float64)
    m1, m2, m4 = (_central(atomic, x, s * h) for s in (1.0, 2.0, 4.0))
    fine, coarse = (4.0 * m1 - m2) / 3.0, (4.0 * m2 - m4) / 3.0
    return fine, np.abs(fine - coarse)


def _mic(x, cell, pbc):
    d = x[:, None, :] - x[None, :, :]   # [j, i] = r_j - r_i
    if np.any(pbc):
        s = d @ np.linalg.inv(cell)
        s -= np.round(s) * np.asarray(pbc, dtype=np.float64)
        d = s @ cell
    return d


def _six(t):
    """[..., 3, 3] -> the six symmetrised components."""
    return np.stack([0.5 * (t[..., a, b] + t[..., b, a]) for a, b in COMPONENTS], axis=-1)


def per_atom_part(e, v, m):
    """(values, terms): J_conv and K, entries 0:3 and 6:12 of a row, and the sums of their |terms|."""
    v, m, e = np.asarray(v, dtype=np.float64), np.asarray(m, dtype=np.float64), np.asarray(e, dtype=np.float64)
    row, terms = np.zeros(18), np.zeros(18)
    w = 0.5 * m * (v * v).sum(axis=1) + e
    row[0:3], terms[0:3] = (w[:, None] * v).sum(axis=0), np.abs(w[:, None] * v).sum(axis=0)
    kk = m[:, None, None] * v[:, :, None] * v[:, None, :]
    row[6:12], terms[6:12] = _six(kk.sum(axis=0)), _six(np.abs(kk).sum(axis=0))
    return row, terms


def row_from_matrix(evaluate, x, v, m, cell, pbc, h=H):
    """The row of the state (x, v) from the full matrix: dict `row`, `fd` (the propagated uncertainty of the finite
    differences), `terms` (sum of |terms|), and the self-checks `force_gap` (the matrix against the oracle's analytic
    forces) and `virial_gap` (W against the oracle's virial)."""
    x, v = np.asarray(x, dtype=np.float64), np.asarray(v, dtype=np.float64)
    out = evaluate(x)
    M, dM = energy_matrix(evaluate, x, h)
    d = _mic(x, np.asarray(cell, dtype=np.float64), pbc)
    row, terms = per_atom_part(out["atomic"], v, m)
    fd = np.zeros(18)
    mv = np.einsum("jic,ic->ji", M, v)
    row[3:6] = np.einsum("jia,ji->a", d, mv)
    terms[3:6] = np.einsum("jia,ji->a", np.abs(d), np.abs(mv))
    fd[3:6] = np.einsum("jia,ji->a", np.abs(d), np.einsum("jic,ic->ji", dM, np.abs(v)))
    row[12:18] = _six(-np.einsum("jia,jib->ab", d, M))
    terms[12:18] = _six(np.einsum("jia,jib->ab", np.abs(d), np.abs(M)))
    fd[12:18] = _six(np.einsum("jia,jib->ab", np.abs(d), dM))
    forces = -M.sum(axis=0)
    return dict(row=row, fd=fd, terms=terms, force_gap=float(np.abs(forces - out["forces"]).max()),
                virial_gap=float(np.abs(row[12:18] - _six(np.asarray(out["virial"]))).max()), matrix=M, matrix_fd=dM)


def cluster_row(evaluate, x, v, m, h=H):
    """The row of a free cluster by the identity: J_pot from one directional derivative along v (Richardson over the
    steps eps, 2 eps, 4 eps with eps max|v| = h) and the oracle's analytic forces, W from the oracle's virial."""
    x, v = np.asarray(x, dtype=np.float64), np.asarray(v, dtype=np.float64)
    out = evaluate(x)
    row, terms = per_atom_part(out["atomic"], v, m)
    fd = np.zeros(18)
    vmax = float(np.abs(v).max())
    if vmax > 0.0:
        eps = h / vmax
        atomic = lambda y: np.asarray(evaluate(y)["atomic"], dtype=np.float64)
        d1, d2, d4 = ((atomic(x + s * eps * v) - atomic(x - s * eps * v)) / (2.0 * s * eps) for s in (1.0, 2.0, 4.0))
        fine, coarse = (4.0 * d1 - d2) / 3.0, (4.0 * d2 - d4) / 3.0
        fv = (np.asarray(out["forces"]) * v).sum(axis=1)
        row[3:6] = (x * fine[:, None]).sum(axis=0) + (x * fv[:, None]).sum(axis=0)
        terms[3:6] = (np.abs(x) * np.abs(fine)[:, None]).sum(axis=0) + (np.abs(x) * np.abs(fv)[:, None]).sum(axis=0)
        fd[3:6] = (np.abs(x) * np.abs(fine - coarse)[:, None]).sum(axis=0)
    row[12:18] = _six(np.asarray(out["virial"]))
    terms[12:18] = _six(np.abs(x).T @ np.abs(np.asarray(out["forces"])))   # W = - sum_i r_i (x) F_i in a free cluster
    return dict(row=row, fd=fd, terms=terms)


def bound(ref, chain):
    """The bound of every one of the 18 numbers: the finite differences' uncertainty and the rounding term."""
    return ref["fd"] + 2.0 ** -53 * chain * ref["terms"]


def accumulate(rows, n_lags):
    """What the device keeps, from rows [S, F, 18] in sample order: (sums [F, 18], a_heat [F, L, 3], a_press [F, L, 6],
    and the sums of the |products| behind a_heat and a_press), in long double."""
    r = np.asarray(rows, dtype=np.longdouble)
    S, F = r.shape[:2]
    j, p = r[..., 0:3] + r[..., 3:6], r[..., 6:12] - r[..., 12:18]
    a_heat, a_press = np.zeros((F, n_lags, 3), dtype=np.longdouble), np.zeros((F, n_lags, 6), dtype=np.longdouble)
    t_heat, t_press = np.zeros_like(a_heat), np.zeros_like(a_press)
    for n in range(S):
        for k in range(min(n, n_lags - 1) + 1):
            a_heat[:, k] += j[n] * j[n - k]
            a_press[:, k] += p[n] * p[n - k]
            t_heat[:, k] += np.abs(j[n] * j[n - k])
            t_press[:, k] += np.abs(p[n] * p[n - k])
    return r.sum(axis=0), a_heat, a_press, t_heat, t_press
