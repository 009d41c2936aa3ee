"""NumPy definition of the bond-orientational order parameters of the device MD loop (`ta_md_set_order`), for tests.
It shares nothing with the library's neighbour list: every frame is swept by brute force over all atoms and all
periodic images that can lie within the largest bond cutoff (the image reach is that of tests/md_rdf_reference.py, as
in tests/md_adf_reference.py), and nothing with the kernel's recurrences: Y_lm comes from NumPy's Legendre polynomials,

    Y_lm(t, e) = N_lm (-1)^m [d^m P_l / dt^m](t) e^m,   t = z / r,  e = (x + i y) / r,
    N_lm = sqrt((2 l + 1) / (4 pi) (l - m)! / (l + m)!)   from exact integer factorials,

which is scipy.special.sph_harm's Y_lm (Condon-Shortley phase) without trigonometry.

    neighbours of i (species a): every (j, S) != (i, 0) with |d| < rb[a][b], d = x_j - x_i + S . h, b = species(j)
    q_lm(i)    = mean over the neighbours of Y_lm(d / |d|), 0 without neighbours        (m = 0 .. l)
    q_l        = sqrt(4 pi / (2 l + 1) (|q_l0|^2 + 2 sum_{m > 0} |q_lm|^2))
    qbar_lm(i) = (q_lm(i) + sum over the neighbours of q_lm(j)) / (N_b + 1), qbar_l from it as q_l from q_lm
    s_ij       = Re sum_{m = -l .. l} q_lm(i) conj(q_lm(j)) / (|q_l(i)| |q_l(j)|) for l = solid_degree
    n_conn(i)  = number of neighbours with s_ij > c (none for a centre or a neighbour with |q_l| = 0)
"""
import itertools
from math import factorial, pi, sqrt

import numpy as np
from numpy.polynomial import legendre

from tests.md_rdf_reference import _widths

MAX_CONN = 31


def norm_lm(l, m):
    """N_lm, from exact integers."""
    return sqrt((2 * l + 1) * factorial(l - m) / (4.0 * pi * factorial(l + m)))


def ylm(l, d):
    """Y_lm of the directions of the vectors `d` [..., 3] for m = 0 .. l: complex [..., l + 1]."""
    d = np.asarray(d, dtype=np.float64)
    r = np.sqrt((d * d).sum(axis=-1))
    t, e = d[..., 2] / r, (d[..., 0] + 1j * d[..., 1]) / r
    coeff = np.zeros(l + 1)
    coeff[l] = 1.0
    out = np.empty(d.shape[:-1] + (l + 1,), dtype=np.complex128)
    for m in range(l + 1):
        dm = legendre.legder(coeff, m) if m else coeff
        out[..., m] = norm_lm(l, m) * (-1) ** m * legendre.legval(t, dm) * e ** m
    return out


def invariant(l, qlm):
    """q_l of q_lm [..., l + 1] (m = 0 .. l)."""
    p = np.abs(qlm) ** 2
    return np.sqrt(4.0 * pi / (2 * l + 1) * (p[..., 0] + 2.0 * p[..., 1:].sum(axis=-1)))


def full_norm(qlm):
    """The 2-norm of q_lm over m = -l .. l, from the m = 0 .. l in `qlm` [..., l + 1]."""
    p = np.abs(qlm) ** 2
    return np.sqrt(p[..., 0] + 2.0 * p[..., 1:].sum(axis=-1))


def neighbours(x, h, pbc, sp, rb):
    """Brute force: for every atom of one frame the list of (j, d) of its neighbours, and the smallest |r / rb - 1|
    over every candidate."""
    n = len(x)
    cut = rb[sp[:, None], sp[None, :]]
    r_max = float(rb.max())
    widths = _widths(h, pbc)
    frac = x @ np.linalg.inv(h) if np.any(pbc) else np.zeros_like(x)
    spread = frac.max(axis=0) - frac.min(axis=0)
    reach = [int(np.floor(r_max / w + s)) if np.isfinite(w) else 0 for w, s in zip(widths, spread)]
    d0 = x[None, :, :] - x[:, None, :]
    found = [([], []) for _ in range(n)]
    gap_r = np.inf
    for S in itertools.product(*[range(-m, m + 1) for m in reach]):
        d = d0 + np.asarray(S, dtype=np.float64) @ h
        r2 = (d * d).sum(axis=-1)
        keep = np.ones((n, n), dtype=bool)
        if S == (0, 0, 0):
            np.fill_diagonal(keep, False)   # an atom is no neighbour of itself
        if keep.any():
            gap_r = min(gap_r, float(np.abs(np.sqrt(r2[keep]) / cut[keep] - 1.0).min()))
        near = keep & (r2 < cut * cut)
        for i in np.nonzero(near.any(axis=1))[0]:
            found[i][0].append(np.nonzero(near[i])[0])
            found[i][1].append(d[i, near[i]])
    out = []
    for js, ds in found:
        out.append((np.concatenate(js), np.concatenate(ds)) if js else (np.zeros(0, dtype=np.int64), np.zeros((0, 3))))
    return out, gap_r


def order_parameters(snapshots, cells, pbc, species, natoms, n_elements, degrees, n_bins, r_bond, solid):
    """`snapshots` [n_samples, N, 3] (all frames, atom order of the batch), `cells` [F, 3, 3] (or one set per
    snapshot, [n_samples, F, 3, 3]), `pbc` [F, 3], `species` [N], `natoms` [F], `degrees` the l, `r_bond` a distance
    or [E, E], `solid` = (solid_degree, c). Returns a dict:
      q, qbar [N, D]; n_bonds, n_conn [N]; qlm complex [N, sum (l + 1)]: the LAST snapshot's per-atom arrays
      hist_q, hist_qbar [F, E, D, n_bins], hist_conn [F, E, 32]: int64, over all snapshots
      gap_bin: the smallest distance of any q B or qbar B to an integer 1 .. B - 1; gap_r: the smallest
      |r / rb - 1| over every candidate neighbour; gap_s: the smallest |s_ij - c| over every bond whose two norms
      are not 0; min_norm: the smallest |q_l| of solid_degree among atoms with neighbours (inf: none)."""
    xs = np.asarray(snapshots, dtype=np.float64)
    cells = np.asarray(cells, dtype=np.float64)
    F, E, B = len(natoms), int(n_elements), int(n_bins)
    cells = np.broadcast_to(cells.reshape((-1, F, 3, 3)), (len(xs), F, 3, 3))
    pbc = np.asarray(pbc).reshape(-1, 3)
    species = np.asarray(species, dtype=np.int64)
    rb = np.broadcast_to(np.asarray(r_bond, dtype=np.float64), (E, E))
    degrees = [int(l) for l in degrees]
    D, N = len(degrees), xs.shape[1]
    off = np.concatenate([[0], np.cumsum([l + 1 for l in degrees])])
    sd, c = degrees.index(int(solid[0])), float(solid[1])
    hist_q, hist_qbar = np.zeros((F, E, D, B), dtype=np.int64), np.zeros((F, E, D, B), dtype=np.int64)
    hist_conn = np.zeros((F, E, MAX_CONN + 1), dtype=np.int64)
    gaps = dict(gap_bin=np.inf, gap_r=np.inf, gap_s=np.inf, min_norm=np.inf)
    last = None
    for x_all, h_all in zip(xs, cells):
        qlm = np.zeros((N, off[-1]), dtype=np.complex128)
        qbar_lm = np.zeros_like(qlm)
        nb, nc = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
        lists = []
        a0 = 0
        for f in range(F):
            n = int(natoms[f])
            if n:
                found, gap_r = neighbours(x_all[a0:a0 + n], h_all[f], pbc[f], species[a0:a0 + n], rb)
                gaps["gap_r"] = min(gaps["gap_r"], gap_r)
                lists += [(a0 + js, ds) for js, ds in found]
            a0 += n
        for i, (js, ds) in enumerate(lists):
            nb[i] = len(js)
            if len(js):
                for k, l in enumerate(degrees):
                    qlm[i, off[k]:off[k + 1]] = ylm(l, ds).sum(axis=0) / len(js)
        norms = full_norm(qlm[:, off[sd]:off[sd + 1]])
        if (nb > 0).any():
            gaps["min_norm"] = min(gaps["min_norm"], float(norms[nb > 0].min()))
        w = np.full(degrees[sd] + 1, 2.0)
        w[0] = 1.0
        for i, (js, ds) in enumerate(lists):
            qbar_lm[i] = (qlm[i] + qlm[js].sum(axis=0)) / (len(js) + 1)
            if len(js) and norms[i] > 0.0:
                ok = norms[js] > 0.0
                qi, qj = qlm[i, off[sd]:off[sd + 1]], qlm[js[ok], off[sd]:off[sd + 1]]
                s = (w * (qi * np.conj(qj)).real).sum(axis=-1) / (norms[i] * norms[js[ok]])
                if len(s):
                    gaps["gap_s"] = min(gaps["gap_s"], float(np.abs(s - c).min()))
                nc[i] = int((s > c).sum())
        q = np.stack([invariant(l, qlm[:, off[k]:off[k + 1]]) for k, l in enumerate(degrees)], axis=1)
        qbar = np.stack([invariant(l, qbar_lm[:, off[k]:off[k + 1]]) for k, l in enumerate(degrees)], axis=1)
        frame_of = np.repeat(np.arange(F), np.asarray(natoms, dtype=np.int64))
        for vals, hist in ((q, hist_q), (qbar, hist_qbar)):
            t = vals * B
            edge = np.rint(t)
            inner = (edge >= 1) & (edge <= B - 1)
            if inner.any():
                gaps["gap_bin"] = min(gaps["gap_bin"], float(np.abs(t[inner] - edge[inner]).min()))
            kbin = np.minimum(B - 1, np.floor(t).astype(np.int64))
            for k in range(D):
                np.add.at(hist, (frame_of, species, k, kbin[:, k]), 1)
        np.add.at(hist_conn, (frame_of, species, np.minimum(nc, MAX_CONN)), 1)
        last = dict(q=q, qbar=qbar, n_bonds=nb, n_conn=nc, qlm=qlm)
    return dict(last, hist_q=hist_q, hist_qbar=hist_qbar, hist_conn=hist_conn, **gaps)
