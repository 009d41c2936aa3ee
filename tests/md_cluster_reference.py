"""NumPy / Python definition of the cluster analysis of the device MD loop (`ta_md_set_clusters`), for tests. It
shares nothing with the library's neighbour list: every frame is swept by brute force over all atoms and all periodic
images that can lie within the largest link cutoff (`neighbours` of tests/md_order_reference.py), and the components
come from a union-find of its own.

    atom i (species a) is selected: bit a of species_mask is set and (n_min == 0 or n_conn(i) >= n_min)
    selected i != j are linked:     some image S has |x_j - x_i + S . h| < rl[a][b]  (an image of i itself links nothing)
    cluster:                        a connected component of the selected atoms; size = atoms, not images
    label:                          the smallest index of its members in the atom order of the whole batch
    hist[f][min(size, B) - 1]       += 1 per cluster of frame f and sample
    row[f]                          = {selected, clusters, largest size, its label (smallest among equals)}, or
                                      {0, 0, 0, -1} when nothing is selected
"""
import numpy as np

from tests.md_order_reference import neighbours


def components(n, links, selected):
    """Union-find over the atoms 0 .. n - 1: `links` pairs (i, j), `selected` bool [n]; links with an end that is not
    selected are dropped. Returns label [n] (smallest member, -1: not selected) and size [n] (0: not selected)."""
    parent = list(range(n))

    def find(a):
        root = a
        while parent[root] != root:
            root = parent[root]
        while parent[a] != root:
            parent[a], a = root, parent[a]
        return root

    for i, j in links:
        if i != j and selected[i] and selected[j]:
            a, b = find(int(i)), find(int(j))
            if a != b:
                parent[max(a, b)] = min(a, b)
    label, size = np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=np.int64)
    smallest = {}
    for i in range(n):
        if selected[i]:
            r = find(i)
            smallest.setdefault(r, i)   # (i ascends: the first member seen is the smallest)
            label[i] = smallest[r]
    for i in range(n):
        if selected[i]:
            size[i] = int((label == label[i]).sum())
    return label, size


def clusters(snapshots, cells, pbc, species, natoms, n_elements, r_link, species_mask, n_bins, n_min=0, n_conn=None):
    """`snapshots` [n_samples, N, 3] (all frames, atom order of the batch), `cells` [F, 3, 3] (or one set per
    snapshot), `pbc` [F, 3], `species` [N], `natoms` [F], `r_link` a distance or [E, E], `species_mask` the bits of
    the elements that can be selected, `n_conn` [n_samples, N] when `n_min` > 0. Returns a dict:
      label, size [N]: the LAST snapshot's per-atom arrays (labels are indices in the batch)
      hist [F, n_bins] int64 over all snapshots; series [n_samples, F, 4] int64
      gap_r: the smallest |r / rl - 1| over every candidate pair of every snapshot."""
    xs = np.asarray(snapshots, dtype=np.float64)
    F, E, B = len(natoms), int(n_elements), int(n_bins)
    cells = np.broadcast_to(np.asarray(cells, dtype=np.float64).reshape((-1, F, 3, 3)), (len(xs), F, 3, 3))
    pbc = np.asarray(pbc).reshape(-1, 3)
    species = np.asarray(species, dtype=np.int64)
    rl = np.broadcast_to(np.asarray(r_link, dtype=np.float64), (E, E))
    N = xs.shape[1]
    hist = np.zeros((F, B), dtype=np.int64)
    series = np.zeros((len(xs), F, 4), dtype=np.int64)
    gap_r, label, size = np.inf, None, None
    for n, (x_all, h_all) in enumerate(zip(xs, cells)):
        selected = ((int(species_mask) >> species) & 1).astype(bool)
        if n_min > 0:
            selected &= np.asarray(n_conn)[n] >= n_min
        label, size = np.full(N, -1, dtype=np.int64), np.zeros(N, dtype=np.int64)
        a0 = 0
        for f in range(F):
            m = int(natoms[f])
            series[n, f] = (0, 0, 0, -1)
            if m:
                found, gap = neighbours(x_all[a0:a0 + m], h_all[f], pbc[f], species[a0:a0 + m], rl)
                gap_r = min(gap_r, gap)
                links = [(i, int(j)) for i, (js, _) in enumerate(found) for j in js]
                lab, siz = components(m, links, selected[a0:a0 + m])
                label[a0:a0 + m] = np.where(lab >= 0, lab + a0, -1)
                size[a0:a0 + m] = siz
                roots = np.nonzero(lab == np.arange(m))[0]
                for r in roots:
                    hist[f, min(int(siz[r]), B) - 1] += 1
                if len(roots):
                    best = min(roots, key=lambda r: (-int(siz[r]), int(r)))
                    series[n, f] = (int(selected[a0:a0 + m].sum()), len(roots), int(siz[best]), int(best) + a0)
            a0 += m
    return dict(label=label, size=size, hist=hist, series=series, gap_r=gap_r)
