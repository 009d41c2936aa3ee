"""NumPy definition of the bond-angle counts of the device MD loop (`ta_md_set_adf`), for tests. It shares nothing
with the library's neighbour list: every frame is swept by brute force over all atoms and all periodic images that
can lie within the largest bond cutoff (the image reach is that of tests/md_rdf_reference.py).

    neighbours of i (species a): every (j, S) != (i, 0) with |d| < rb[a][b], d = x_j - x_i + S . h, b = species(j)
    C[f][a][p][k] = number of unordered pairs {(j, S), (k', S')} of distinct neighbours of a centre i of frame f with
                    species(i) = a, p = p(b, c) for the species b <= c of the two, over all snapshots, and
                    k = min(B - 1, floor(theta / (pi / B))), theta = atan2(|u x w|, u . w) of the two vectors d
"""
import itertools

import numpy as np

from tests.md_rdf_reference import _widths


def pair_index(b, c, n_elements):
    """p of the unordered species pair: b E - b (b - 1) / 2 + (c - b) for b <= c."""
    b, c = np.minimum(b, c), np.maximum(b, c)
    return b * n_elements - b * (b - 1) // 2 + (c - b)


def triple_counts(snapshots, cells, pbc, species, natoms, n_elements, n_bins, r_bond, stats=None):
    """`snapshots` [n_samples, N, 3] (all frames, atom order of the batch), `cells` [F, 3, 3] (or one set per
    snapshot, [n_samples, F, 3, 3]), `pbc` [F, 3], `species` [N], `natoms` [F], `r_bond` a distance or [E, E].
    Returns (counts [F, E, P, n_bins] int64, gap_theta, gap_r): gap_theta is the smallest distance of any
    theta / dtheta to an integer 1 .. n_bins - 1 over every triple met, gap_r the smallest |r / rb - 1| over every
    candidate neighbour (inf when there is none): counts from arithmetic in another order are the same integers
    while both are far above the rounding. `stats` (a dict, optional) receives `n_neighbours`: the neighbour
    count of every centre of every snapshot, in order."""
    xs = np.asarray(snapshots, dtype=np.float64)
    cells = np.asarray(cells, dtype=np.float64)
    F, E, B = len(natoms), int(n_elements), int(n_bins)
    cells = np.broadcast_to(cells.reshape((-1, F, 3, 3)), (len(xs), F, 3, 3))
    pbc = np.asarray(pbc).reshape(-1, 3)
    species = np.asarray(species, dtype=np.int64)
    rb = np.broadcast_to(np.asarray(r_bond, dtype=np.float64), (E, E))
    r_max = float(rb.max())
    P = E * (E + 1) // 2
    dtheta = np.pi / B
    counts = np.zeros((F, E, P, B), dtype=np.int64)
    gap_theta, gap_r = np.inf, np.inf
    n_neighbours = []
    a0 = 0
    for f in range(F):
        n = int(natoms[f])
        sp = species[a0:a0 + n]
        cut = rb[sp[:, None], sp[None, :]]   # [i, j]
        for x, h in zip(xs[:, a0:a0 + n], cells[:, f]):
            if n == 0:
                continue
            widths = _widths(h, pbc[f])
            frac = x @ np.linalg.inv(h) if np.any(pbc[f]) else np.zeros_like(x)
            spread = frac.max(axis=0) - frac.min(axis=0)
            reach = [int(np.floor(r_max / w + s)) if np.isfinite(w) else 0 for w, s in zip(widths, spread)]
            d0 = x[None, :, :] - x[:, None, :]   # [i, j] = x_j - x_i
            found = [[] for _ in range(n)]       # per centre: (vectors [m, 3], species [m]) of every image
            for S in itertools.product(*[range(-m, m + 1) for m in reach]):
                d = d0 + np.asarray(S, dtype=np.float64) @ h
                r = np.sqrt((d * d).sum(axis=-1))
                keep = np.ones((n, n), dtype=bool)
                if S == (0, 0, 0):
                    np.fill_diagonal(keep, False)   # an atom is no neighbour of itself
                if keep.any():
                    gap_r = min(gap_r, float(np.abs(r[keep] / cut[keep] - 1.0).min()))
                near = keep & ((d * d).sum(axis=-1) < cut * cut)
                for i in np.nonzero(near.any(axis=1))[0]:
                    found[i].append((d[i, near[i]], sp[near[i]]))
            for i in range(n):
                m = sum(len(v) for v, _ in found[i])
                n_neighbours.append(m)
                if m < 2:
                    continue
                v = np.concatenate([v for v, _ in found[i]])
                s = np.concatenate([s for _, s in found[i]])
                j, k = np.triu_indices(m, 1)
                u, w = v[j], v[k]
                cross = np.cross(u, w)
                theta = np.arctan2(np.sqrt((cross * cross).sum(axis=-1)), (u * w).sum(axis=-1))
                t = theta / dtheta
                ok = ~np.isnan(t)   # a NaN counts nowhere
                t = t[ok]
                edge = np.rint(t)
                inner = (edge >= 1) & (edge <= B - 1)
                if inner.any():
                    gap_theta = min(gap_theta, float(np.abs(t[inner] - edge[inner]).min()))
                kbin = np.minimum(B - 1, np.floor(t).astype(np.int64))
                p = pair_index(s[j][ok], s[k][ok], E)
                counts[f, sp[i]] += np.bincount(p * B + kbin, minlength=P * B).reshape(P, B)
        a0 += n
    if stats is not None:
        stats["n_neighbours"] = np.array(n_neighbours, dtype=np.int64)
    return counts, gap_theta, gap_r
