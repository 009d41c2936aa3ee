"""NumPy definition of the pair counts of the device MD loop (`ta_md_set_rdf`), for tests. It shares nothing
with the library's neighbour list: every frame is swept by brute force over all atom pairs and all periodic
images that can lie within r_max.

    C[f][a][b][k] = number of directed pairs (i, j, S), (j, S) != (i, 0), of frame f over all snapshots with
                    species(i) = a, species(j) = b and floor(|x_j - x_i + S . h| / dr) = k < n_bins, dr = r_max / n_bins
"""
import itertools

import numpy as np


def _widths(cell, pbc):
    """Perpendicular width of the cell along every periodic axis, inf along the others."""
    vol = abs(np.linalg.det(cell))
    widths = np.array([vol / np.linalg.norm(np.cross(cell[(c + 1) % 3], cell[(c + 2) % 3])) for c in range(3)])
    return np.where(np.asarray(pbc, dtype=bool), widths, np.inf)


def pair_counts(snapshots, cells, pbc, species, natoms, n_elements, n_bins, r_max):
    """`snapshots` [n_samples, N, 3] (all frames, atom order of the batch), `cells` [F, 3, 3], `pbc` [F, 3],
    `species` [N], `natoms` [F]. Returns (counts [F, E, E, n_bins] int64, gap): gap is the smallest distance of
    any r / dr below n_bins + 1/2 to an integer, over every pair met (inf when there is none): counts of a
    summation in another order are the same integers while gap is far above the rounding of r / dr."""
    xs = np.asarray(snapshots, dtype=np.float64)
    cells = np.asarray(cells, dtype=np.float64).reshape(-1, 3, 3)
    pbc = np.asarray(pbc).reshape(-1, 3)
    species = np.asarray(species, dtype=np.int64)
    F, E, B = len(natoms), int(n_elements), int(n_bins)
    dr = float(r_max) / B
    counts = np.zeros((F, E, E, B), dtype=np.int64)
    gap = np.inf
    a0 = 0
    for f in range(F):
        n = int(natoms[f])
        sp = species[a0:a0 + n]
        h = cells[f]
        widths = _widths(h, pbc[f])
        ab = (sp[:, None] * E + sp[None, :]).ravel()
        for x in xs[:, a0:a0 + n]:
            if n == 0:
                continue
            # Images to sweep: along axis c a pair is |frac_j - frac_i + S_c| width_c apart at least, and the
            # fractional coordinates of the (unwrapped) atoms differ by their spread at most, so a pair within
            # r_max has |S_c| <= r_max / width_c + spread_c
            frac = x @ np.linalg.inv(h) if np.any(pbc[f]) else np.zeros_like(x)
            spread = frac.max(axis=0) - frac.min(axis=0)
            reach = [int(np.floor(r_max / w + s)) if np.isfinite(w) else 0 for w, s in zip(widths, spread)]
            d0 = x[None, :, :] - x[:, None, :]   # [i, j] = x_j - x_i
            for S in itertools.product(*[range(-m, m + 1) for m in reach]):
                d = d0 + np.asarray(S, dtype=np.float64) @ h
                u = (np.sqrt((d * d).sum(axis=-1)) / dr).ravel()
                keep = np.ones(n * n, dtype=bool)
                if S == (0, 0, 0):
                    keep[::n + 1] = False   # an atom is no neighbour of itself
                near = keep & (u < B + 0.5)
                if near.any():
                    gap = min(gap, float(np.abs(u[near] - np.rint(u[near])).min()))
                k = np.floor(u)
                take = keep & (k < B)
                idx = ab[take] * B + k[take].astype(np.int64)
                counts[f] += np.bincount(idx, minlength=E * E * B).reshape(E, E, B)
        a0 += n
    return counts, gap
