"""The NumPy definition of the structure factors of the device MD loop (`ta_md_set_sq`), evaluated in
`np.longdouble`: s = x h^-1, the exact fractional part of n . s, then the sums over atoms and the correlations over
time origins as include/tensoralloy_amd.h writes them. It shares nothing with the library.

It also evaluates, from the reference's own numbers alone, the error bound the GPU tests hold the device to. For
every rho_a(q)
    B = N_a 2^-53 (16 + 2 pi 4 kappa_inf(h) max_i sum_c |n_c s_ic| + m)
with 16 for the arithmetic of one term, the middle term for the rounding of the phase n . s through an fp64 inverse
cell, and m the longest chain of additions (atoms per workgroup plus workgroups per frame, both from the device's
plan). A current component has the bound B |v|_max. An accumulator has the propagated bound
    sum over origins of (|u_a| B_b + |u_b| B_a)  +  2^-52 sum over origins of |term|
"""
import numpy as np

LD = np.longdouble
PI = LD(4) * np.arctan(LD(1))
EPS53 = 2.0 ** -53


def inverse(cell):
    """h^-1 of a [3, 3] cell in long double (adjugate over determinant)."""
    h = np.asarray(cell, dtype=LD)
    adj = np.empty((3, 3), dtype=LD)
    for i in range(3):
        for j in range(3):
            r = [k for k in range(3) if k != j]
            c = [k for k in range(3) if k != i]
            adj[i, j] = (-1) ** (i + j) * (h[r[0], c[0]] * h[r[1], c[1]] - h[r[0], c[1]] * h[r[1], c[0]])
    det = h[0, 0] * adj[0, 0] + h[0, 1] * adj[1, 0] + h[0, 2] * adj[2, 0]
    return adj / det


def q_vectors(cell, miller):
    """q = 2 pi h^-1 n [Q, 3] and qhat = q / |q| ((0, 0, 0) for n = 0), long double."""
    q = 2 * PI * np.asarray(miller, dtype=LD) @ inverse(cell).T
    norm = np.sqrt((q * q).sum(axis=1))
    qhat = np.where(norm[:, None] > 0, q / np.where(norm > 0, norm, LD(1))[:, None], LD(0))
    return q, qhat


def amplitudes(x, v, cell, species, n_elements, miller):
    """One frame: rho [E, Q] and cur [E, Q, 3] (complex long double; cur None without v) of the atoms at x [N, 3]
    with velocities v, and `reach` [E, Q] = max over the atoms of element a of sum_c |n_c s_ic| (0 without atoms)."""
    n = np.asarray(miller, dtype=LD)
    s = np.asarray(x, dtype=LD) @ inverse(cell)
    species = np.asarray(species)
    Q = len(n)
    rho = np.zeros((n_elements, Q), dtype=np.clongdouble)
    cur = np.zeros((n_elements, Q, 3), dtype=np.clongdouble) if v is not None else None
    reach = np.zeros((n_elements, Q))
    picks = [species == a for a in range(n_elements)]
    for lo in range(0, Q, 64):   # (blocks of q-vectors: [64, N] long doubles at a time)
        blk = slice(lo, min(lo + 64, Q))
        t = n[blk] @ s.T                 # [q, N]
        t = t - np.rint(t)               # the exact fractional part
        phase = 2 * PI * t
        e = np.cos(phase) + 1j * np.sin(phase)
        spread = np.abs(n[blk]).astype(np.float64) @ np.abs(s).astype(np.float64).T   # sum_c |n_c s_ic|, [q, N]
        for a, pick in enumerate(picks):
            if not pick.any():
                continue
            rho[a, blk] = e[:, pick].sum(axis=1)
            if v is not None:
                cur[a, blk] = e[:, pick] @ np.asarray(v, dtype=LD)[pick]
            reach[a, blk] = spread[:, pick].max(axis=1)
    return rho, cur, reach


def amplitude_bound(cell, species, n_elements, reach, chain, v_max=None):
    """B [E, Q] of rho (or of a current component with `v_max`, the largest |v_ic| of the frame)."""
    h = np.asarray(cell, dtype=np.float64)
    kappa = np.abs(h).sum(axis=1).max() * np.abs(np.linalg.inv(h)).sum(axis=1).max()
    n_a = np.bincount(np.asarray(species), minlength=n_elements)[:n_elements].astype(np.float64)
    b = n_a[:, None] * EPS53 * (16.0 + 2.0 * np.pi * 4.0 * kappa * reach + float(chain))
    return b if v_max is None else b * float(v_max)


def correlate(u, bound, n_lags):
    """u [n_samples, E, Q, C] complex (C components), bound [n_samples, E, Q] of every component: returns
    (A [E, E, L, Q] float64 from long double sums, its bound [E, E, L, Q]) with
    A[a][b][k][q] = sum over origins n >= k of Re sum_c u[n][a][q][c] conj u[n - k][b][q][c]."""
    S, E, Q, C = u.shape
    acc = np.zeros((E, E, n_lags, Q), dtype=LD)
    err = np.zeros((E, E, n_lags, Q))
    mag = np.abs(u).astype(np.float64)
    for k in range(min(n_lags, S)):
        new, old = u[k:], u[:S - k]
        for a in range(E):
            for b in range(E):
                term = (new[:, a] * np.conj(old[:, b])).real.sum(axis=-1)           # [origins, Q]
                acc[a, b, k] = term.sum(axis=0)
                size = (mag[k:, a] * mag[:S - k, b]).sum(axis=-1)
                carried = (mag[k:, a].sum(axis=-1) * bound[:S - k, b] + mag[:S - k, b].sum(axis=-1) * bound[k:, a])
                err[a, b, k] = carried.sum(axis=0) + 2.0 * EPS53 * size.sum(axis=0)
    return acc.astype(np.float64), err


def structure_factors(xs, vs, cell, species, n_elements, miller, n_lags, chain):
    """One frame over the samples xs [S, N, 3] (vs [S, N, 3] or None): a dict of `rho` [S, E, Q], `cur` [S, E, Q, 3]
    (complex128, rounded from long double), their bounds `rho_bound`, `cur_bound` [S, E, Q], and `a_rho`, `a_l`,
    `a_j` [E, E, L, Q] with `a_rho_bound`, `a_l_bound`, `a_j_bound`. `chain` is m of the bound."""
    S = len(xs)
    q, qhat = q_vectors(cell, miller)
    rho, cur, rb, cb = [], [], [], []
    for n in range(S):
        r, c, reach = amplitudes(xs[n], None if vs is None else vs[n], cell, species, n_elements, miller)
        rho.append(r)
        rb.append(amplitude_bound(cell, species, n_elements, reach, chain))
        if vs is not None:
            cur.append(c)
            cb.append(amplitude_bound(cell, species, n_elements, reach, chain, np.abs(vs[n]).max() if len(vs[n]) else 0.0))
    rho, rb = np.array(rho), np.array(rb)
    out = {"rho": rho.astype(np.complex128), "rho_bound": rb, "q": q.astype(np.float64)}
    out["a_rho"], out["a_rho_bound"] = correlate(rho[..., None], rb, n_lags)
    if vs is not None:
        cur, cb = np.array(cur), np.array(cb)
        out["cur"], out["cur_bound"] = cur.astype(np.complex128), cb
        out["a_j"], out["a_j_bound"] = correlate(cur, cb, n_lags)
        lon = (cur * qhat[None, None, :, :]).sum(axis=-1, keepdims=True)
        # (qhat . j has the three components' bounds weighted by |qhat_c|, and the rounding of the projection itself)
        weight = np.abs(qhat).sum(axis=1).astype(np.float64)
        lb = cb * weight[None, None, :] + 4.0 * EPS53 * np.abs(cur).sum(axis=-1).astype(np.float64)
        out["a_l"], out["a_l_bound"] = correlate(lon, lb, n_lags)
    return out
