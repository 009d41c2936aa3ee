"""
Plain-numpy second derivatives of a pair-functional EAM energy (test infrastructure only),

    E = sum_i F_{s_i}(rho_i) + 1/2 sum_{i -> j} phi_{s_i s_j}(r_ij),      rho_i = sum_{i -> j} rho_{s_j}(r_ij),

along one direction (dR, dh) of positions and cell: `hvp` returns d F / d eps [N, 3] and d W / d eps [3, 3] of
the forces and the virial as oracle/eam.py::evaluate defines them (directed pairs from
oracle.neighbors.neighbor_list, g_p = dE / dD_p of the centre's terms, F_i = sum g_p - sum g_rev(p),
W = sum g_p x D_p). Written from the formula, not from the library's kernels: with D' = dR_j - dR_i + S.dh,
r' = D.D' / r, rho_i' = sum rho'(r) r' and s_p = F'(rho_i) rho'(r) + phi'(r) / 2,

    s_p' = F''(rho_i) rho_i' rho'(r) + (F'(rho_i) rho''(r) + phi''(r) / 2) r',
    g_p' = (s_p' / r - s_p r' / r^2) D + (s_p / r) D'.

Every function is a callable x -> (f, f', f''):
  * `spline`: the natural cubic spline of a table, scipy's CubicSpline exactly as oracle/eam.py::spline_function
    builds it (the setfl models: forces of a spline model are only C1, no finite difference converges there);
  * `hermite`: the cubic Hermite pieces on the library's documented knots k rcut / 32768 through the values and
    derivatives of a smooth function there (nn pair functions through their tables: the function the library
    says it evaluates);
  * `with_second`: a smooth (f, f') pair and f'' from a 1-D 4th-order central difference of f' (validation of
    this module against the stencil of the oracle's forces on an analytic model).
ADP (dipole / quadrupole functions u, w, tabulated or not) is out of scope: those rows are held to the stencil of
the oracle's forces instead (test_gpu_hvp_oracle.py).
"""
import numpy as np

NN_TABLE_KNOTS = 32769   # kNnTableKnots: knots k rcut / 32768 of an nn pair function's table


def spline(table):
    from scipy.interpolate import CubicSpline
    cs = CubicSpline(np.asarray(table[0], dtype=np.float64), np.asarray(table[1], dtype=np.float64),
                     bc_type="natural", extrapolate=True)
    return lambda x: (cs(x), cs(x, 1), cs(x, 2))


def hermite(fn, rcut, knots=NN_TABLE_KNOTS):
    """`fn`: x -> (f, f'). Pieces c0 + c1 t + c2 t^2 + c3 t^3, t = x - x_k, matching f and f' at both ends;
    beyond the last knot the last piece continues."""
    dx = rcut / (knots - 1)
    xk = np.arange(knots) * dx
    f, d = fn(xk)
    slope = (f[1:] - f[:-1]) / dx
    c2 = (3.0 * slope - 2.0 * d[:-1] - d[1:]) / dx
    c3 = (d[:-1] + d[1:] - 2.0 * slope) / (dx * dx)

    def ev(x):
        x = np.asarray(x, dtype=np.float64)
        k = np.clip((x / dx).astype(np.int64), 0, knots - 2)
        t = x - xk[k]
        return (f[k] + t * (d[k] + t * (c2[k] + t * c3[k])), d[k] + t * (2.0 * c2[k] + 3.0 * t * c3[k]),
                2.0 * c2[k] + 6.0 * t * c3[k])
    return ev


def with_second(fn, step=1e-3):
    """`fn`: x -> (f, f') of a smooth function; f'' = (f'(x - 2s) - 8 f'(x - s) + 8 f'(x + s) - f'(x + 2s)) / 12 s."""
    def ev(x):
        x = np.asarray(x, dtype=np.float64)
        f, d = fn(x)
        d2 = (fn(x - 2 * step)[1] - 8.0 * fn(x - step)[1] + 8.0 * fn(x + step)[1] - fn(x + 2 * step)[1]) / (12 * step)
        return f, d, d2
    return ev


def hvp(elements, rcut, symbols, positions, cell, pbc, dR, dh, rho, phi, embed, eps=1e-14):
    """rho[el], embed[el], phi["AB" (sorted)]: callables x -> (f, f', f''). Returns dF [N, 3], dW [3, 3]."""
    from oracle.neighbors import _complete_cell, neighbor_list
    els = sorted(elements)
    R = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    N = len(R)
    pbc = np.asarray(pbc, dtype=bool).reshape(3)
    h = _complete_cell(np.asarray(cell, dtype=np.float64), pbc)
    dR = np.zeros((N, 3)) if dR is None else np.asarray(dR, dtype=np.float64).reshape(N, 3)
    dh = np.zeros((3, 3)) if dh is None else np.asarray(dh, dtype=np.float64).reshape(3, 3)
    sym = list(symbols)
    pi, pj, pS = neighbor_list(R, h, pbc, rcut)
    S = pS.astype(np.float64)
    D = R[pj] - R[pi] + S @ h
    T = dR[pj] - dR[pi] + S @ dh
    r = np.sqrt(np.sum(D * D, axis=1) + eps)
    rd = np.sum(D * T, axis=1) / r
    P = len(pi)
    d1, d2, p1, p2 = np.zeros(P), np.zeros(P), np.zeros(P), np.zeros(P)
    f0 = np.zeros(P)
    si = np.array([els.index(s) for s in sym])[pi] if P else np.zeros(0, dtype=int)
    sj = np.array([els.index(s) for s in sym])[pj] if P else np.zeros(0, dtype=int)
    for b, eb in enumerate(els):
        m = sj == b
        if m.any():
            f0[m], d1[m], d2[m] = rho[eb](r[m])
        for a, ea in enumerate(els):
            mm = m & (si == a)
            if mm.any():
                _, p1[mm], p2[mm] = phi["".join(sorted([ea, eb]))](r[mm])
    dens, densdot = np.zeros(N), np.zeros(N)
    np.add.at(dens, pi, f0)
    np.add.at(densdot, pi, d1 * rd)
    F1, F2 = np.zeros(N), np.zeros(N)
    spec = np.array([els.index(s) for s in sym])
    for a, ea in enumerate(els):
        m = spec == a
        if m.any():
            _, F1[m], F2[m] = embed[ea](dens[m])
    s = F1[pi] * d1 + 0.5 * p1
    sdot = F2[pi] * densdot[pi] * d1 + (F1[pi] * d2 + 0.5 * p2) * rd
    g = (s / r)[:, None] * D
    gdot = (sdot / r - s * rd / (r * r))[:, None] * D + (s / r)[:, None] * T
    dF = np.zeros((N, 3))
    np.add.at(dF, pi, gdot)
    np.add.at(dF, pj, -gdot)
    dW = gdot.T @ D + g.T @ T
    return dF, dW
