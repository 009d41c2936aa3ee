"""NumPy / Python definition of the common neighbour analysis of the device MD loop (`ta_md_set_cna`), for tests. It
shares nothing with the library's neighbour list: every frame is swept by brute force over all atoms and all periodic
images that can lie within the reach, and the sort, the adjacency and the chain search are its own.

    candidates of i:   every (j, S) but (i, 0) with d = x_j - x_i + S . h, d . d < r^2 (r_max adaptive, r_cut fixed),
                       sorted by the key (d . d, j, S0, S1, S2)
    bonded j, k:       |d_j - d_k| < rc
    signature of j:    (neighbours bonded to j, bonds among those, most bonds in one connected set of those bonds)
    FCC 12 x (4,2,1); HCP 6 x (4,2,1) + 6 x (4,2,2); ICO 12 x (5,5,5); BCC 8 x (6,6,6) + 6 x (4,4,4); else OTHER
    adaptive:          < 12 candidates: OTHER, r_local 0; the 12 nearest, rc = (1 + sqrt 2) / 2 mean |d|: FCC, HCP, ICO;
                       else with >= 14 candidates the 14 nearest,
                       rc = (1 + sqrt 2) / 2 ((2 / sqrt 3) sum of 8 nearest |d| + sum of next 6) / 14: BCC
    fixed:             all N candidates, rc = r_cut; N = 12: FCC, HCP, ICO; N = 14: BCC; else OTHER
"""
import itertools
import math

import numpy as np

from tests.md_rdf_reference import _widths

OTHER, FCC, HCP, BCC, ICO = range(5)
ADAPTIVE, FIXED = "adaptive", "fixed"
SCALE = (1.0 + math.sqrt(2.0)) / 2.0


def bcc_lattice(a=2.87, rep=(4, 4, 4), jitter=0.02, seed=0):
    """(positions, cell) of a bcc crystal with Gaussian jitter."""
    base = np.array([[0.0, 0.0, 0.0], [0.5, 0.5, 0.5]]) * a
    pts = np.array([base + np.array([i, j, k]) * a for i in range(rep[0]) for j in range(rep[1])
                    for k in range(rep[2])]).reshape(-1, 3)
    pts = pts + np.random.RandomState(seed).normal(0.0, jitter, pts.shape) if jitter else pts
    return pts, np.diag([a * rep[0], a * rep[1], a * rep[2]])


def icosahedron(radius=2.5, box=20.0):
    """(positions, cell): a centre and the twelve corners of a regular icosahedron around it, in the middle of a box."""
    g = (1.0 + math.sqrt(5.0)) / 2.0
    corners = np.array([p for a in (-1.0, 1.0) for b in (-g, g) for p in ((0, a, b), (a, b, 0), (b, 0, a))])
    corners *= radius / math.sqrt(1.0 + g * g)
    return np.vstack([np.zeros((1, 3)), corners]) + box / 2.0, np.eye(3) * box


def close_packed_stack(sequence="ABCABCAB", a=2.5, rep=(4, 4), jitter=0.02, seed=0):
    """(positions, cell, layer of every atom): close-packed layers stacked in `sequence`, periodic: in ABCABCAB the
    layers 0 and 7 are hcp (their two neighbour layers are alike), the other six fcc."""
    cell = np.array([[a * rep[0], 0.0, 0.0], [-a * rep[1] / 2.0, a * rep[1] * math.sqrt(3.0) / 2.0, 0.0],
                     [0.0, 0.0, a * math.sqrt(2.0 / 3.0) * len(sequence)]])
    a1, a2 = cell[0] / rep[0], cell[1] / rep[1]
    offs = {"A": 0.0, "B": 1.0, "C": 2.0}
    pts, layer = [], []
    for n, s in enumerate(sequence):
        for i in range(rep[0]):
            for j in range(rep[1]):
                pts.append((i + offs[s] / 3.0) * a1 + (j + 2.0 * offs[s] / 3.0) * a2 + n * cell[2] / len(sequence))
                layer.append(n)
    pts = np.array(pts)
    pts = pts + np.random.RandomState(seed).normal(0.0, jitter, pts.shape) if jitter else pts
    return pts, cell, np.array(layer)


def candidates(x, cell, pbc, r, tie="forward"):
    """For every atom of one frame (`x` [n, 3], `cell` [3, 3], `pbc` [3]) the candidates within `r`, sorted: a list
    of (d [k, 3], dist [k]); `tie` "reverse" breaks ties of d . d by descending (j, S) instead (tests only). Also
    the smallest |dist / r - 1| over every pair looked at."""
    x = np.asarray(x, dtype=np.float64)
    cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    n = len(x)
    reach = [int(math.ceil(r / w)) if np.isfinite(w) else 0 for w in _widths(cell, pbc)]
    shifts = np.array(list(itertools.product(*[range(-k, k + 1) for k in reach])), dtype=np.int64)
    offs = shifts.astype(np.float64) @ cell
    out, gap = [], np.inf
    for i in range(n):
        d = (x[None, :, :] - x[i]) + offs[:, None, :]           # [n_shifts, n, 3]
        d2 = np.einsum("sjc,sjc->sj", d, d)
        keep = np.ones_like(d2, dtype=bool)
        keep[np.all(shifts == 0, axis=1), i] = False            # the atom itself
        dist = np.sqrt(d2[keep])
        if len(dist):
            gap = min(gap, float(np.abs(dist / r - 1.0).min()))
        sel = keep & (d2 < r * r)
        s_idx, j_idx = np.nonzero(sel)
        sign = 1 if tie == "forward" else -1
        S = shifts[s_idx]
        order = np.lexsort((sign * S[:, 2], sign * S[:, 1], sign * S[:, 0], sign * j_idx, d2[s_idx, j_idx]))
        s_idx, j_idx = s_idx[order], j_idx[order]
        out.append((d[s_idx, j_idx], np.sqrt(d2[s_idx, j_idx])))
    return out, gap


def signatures(d, rc):
    """The signatures (n_cn, n_b, l_cb) of the neighbour vectors `d` [N, 3] under the bond cutoff `rc`, and the smallest
    | |d_j - d_k| / rc - 1 | over the pairs."""
    N = len(d)
    sep = np.sqrt(((d[:, None, :] - d[None, :, :]) ** 2).sum(axis=-1))
    off = ~np.eye(N, dtype=bool)
    gap = float(np.abs(sep[off] / rc - 1.0).min()) if N > 1 else np.inf
    bonded = (sep < rc) & off
    sigs = []
    for j in range(N):
        common = [k for k in range(N) if bonded[j, k]]
        bonds = [(a, b) for a, b in itertools.combinations(common, 2) if bonded[a, b]]
        # the most bonds in one connected set of bonds: walk the bonds that share an atom
        left, longest = set(bonds), 0
        while left:
            stack, size = [left.pop()], 0
            while stack:
                a, b = stack.pop()
                size += 1
                touching = [e for e in left if a in e or b in e]
                for e in touching:
                    left.discard(e)
                stack.extend(touching)
            longest = max(longest, size)
        sigs.append((len(common), len(bonds), longest))
    return sigs, gap


def _type12(sigs):
    n421, n422, n555 = sigs.count((4, 2, 1)), sigs.count((4, 2, 2)), sigs.count((5, 5, 5))
    if n421 == 12:
        return FCC
    if n421 == 6 and n422 == 6:
        return HCP
    if n555 == 12:
        return ICO
    return OTHER


def _type14(sigs):
    return BCC if sigs.count((6, 6, 6)) == 8 and sigs.count((4, 4, 4)) == 6 else OTHER


def _ordered_sum(values):
    total = 0.0
    for v in values:
        total += float(v)
    return total


def classify(d, dist, mode, r_cut=None):
    """One atom from its sorted candidates: (type, r_local, gap_sel, gap_bond)."""
    n, gap_sel, gap_bond = len(dist), np.inf, np.inf
    if mode == FIXED:
        kind = OTHER
        if n in (12, 14):
            sigs, gap_bond = signatures(d, r_cut)
            kind = _type12(sigs) if n == 12 else _type14(sigs)
        return kind, float(r_cut), gap_sel, gap_bond
    if n < 12:
        return OTHER, 0.0, gap_sel, gap_bond
    if n > 12:
        gap_sel = (dist[12] - dist[11]) / dist[11]
    rc = SCALE * (_ordered_sum(dist[:12]) / 12.0)
    sigs, gap_bond = signatures(d[:12], rc)
    kind = _type12(sigs)
    if kind == OTHER and n >= 14:
        if n > 14:
            gap_sel = min(gap_sel, (dist[14] - dist[13]) / dist[13])
        rc = SCALE * ((2.0 / math.sqrt(3.0) * _ordered_sum(dist[:8]) + _ordered_sum(dist[8:14])) / 14.0)
        sigs, gap = signatures(d[:14], rc)
        gap_bond = min(gap_bond, gap)
        kind = _type14(sigs)
    return kind, rc, gap_sel, gap_bond


def cna(snapshots, cells, pbc, species, natoms, n_elements, mode=ADAPTIVE, r_cut=None, r_max=None, tie="forward"):
    """`snapshots` [n_samples, N, 3] (all frames, atom order of the batch), `cells` [F, 3, 3] (or one set per snapshot),
    `pbc` [F, 3], `species` [N], `natoms` [F]; `r_max` (adaptive) or `r_cut` (fixed) as the device has them. Returns a
    dict:
      structure [N] int64, r_local [N]: the LAST snapshot's per-atom arrays
      counts [F, E, 5] int64 over all snapshots; series [n_samples, F, 5] int64
      gap_r: the smallest |d / r - 1| of any pair against r_max or r_cut
      gap_sel: the smallest relative distance gap between the 12th and 13th nearest candidates of an atom (and the 14th
               and 15th where the second attempt is made)
      gap_bond: the smallest | |d_j - d_k| / rc - 1 | over every neighbour pair of every attempt made."""
    xs = np.asarray(snapshots, dtype=np.float64)
    F, E = len(natoms), int(n_elements)
    cells = np.broadcast_to(np.asarray(cells, dtype=np.float64).reshape((-1, F, 3, 3)), (len(xs), F, 3, 3))
    pbc = np.asarray(pbc).reshape(-1, 3)
    species = np.asarray(species, dtype=np.int64)
    reach = float(r_cut if mode == FIXED else r_max)
    N = xs.shape[1]
    counts = np.zeros((F, E, 5), dtype=np.int64)
    series = np.zeros((len(xs), F, 5), dtype=np.int64)
    gap_r = gap_sel = gap_bond = np.inf
    structure, r_local = None, None
    for n, (x_all, h_all) in enumerate(zip(xs, cells)):
        structure, r_local = np.zeros(N, dtype=np.int64), np.zeros(N)
        a0 = 0
        for f in range(F):
            m = int(natoms[f])
            if m:
                found, gap = candidates(x_all[a0:a0 + m], h_all[f], pbc[f], reach, tie)
                gap_r = min(gap_r, gap)
                for i, (d, dist) in enumerate(found):
                    kind, rc, g_sel, g_bond = classify(d, dist, mode, r_cut)
                    structure[a0 + i], r_local[a0 + i] = kind, rc
                    gap_sel, gap_bond = min(gap_sel, g_sel), min(gap_bond, g_bond)
                    counts[f, species[a0 + i], kind] += 1
                    series[n, f, kind] += 1
            a0 += m
    return dict(structure=structure, r_local=r_local, counts=counts, series=series, gap_r=gap_r, gap_sel=gap_sel,
                gap_bond=gap_bond)
