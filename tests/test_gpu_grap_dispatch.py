"""
The GRAP kernels (ta_grap.hip) build by build and edge by edge, against the oracle (oracle/grap.py) at fp64 bounds.

One evaluation of a GRAP model selects
  * `grap_forward_kernel<MC>` / `grap_backward_kernel<MC>`: MC = 20 for max_moment <= 3 (nd = 1, 4, 10, 20
    packed components), MC = 56 for max_moment 4 and 5 (nd = 35, 56);
  * the number of 16-filter tiles: the forward `kt` loop (K <= 16: one tile; 17 <= K <= 32: two, the second
    one re-reading the pair records the first one wrote) and the backward `Kp` loop;
  * the segment chunking: every (centre, species) segment is staged kFwdChunk = kBwdChunk = 64 pairs at a
    time, so segment lengths 0, < 64, = 64, 65..128 and > 128 take different paths;
  * for the `nn` algorithm, `grap_nn_filter_kernel<ACT, NT>` (ACT softplus or generic, NT = 2 or 4 from the
    widest padded layer after the first), a grid-stride loop over at most 2048 x 4 x 16 = 131,072 pairs per
    trip, with the weights as one LDS image of at most 150 KB;
  * the force gather's 16-lane build at or above 16384 atoms.
`selection` restates these rules on the CPU from the model and the frames alone; every row asserts that it
selects what it is named after (and that its longest and shortest segments lie in the row's window), and
`test_rows_cover_every_combination` that the rows together reach every combination.

Bounds: north_star (1e-6 eV, 1e-5 eV/A, virial `test_gpu_sf.W_TOL`) and what fp64 kernels owe an fp64
oracle: descriptors to 1e-10 x max(1, max|G|), energies to 1e-9 x max(1, |E|), forces to
1e-9 x max(1, max|F|), virial to 1e-8 x max(1, max|W|). New-mode moment 0 is sgn(P0) sqrt(P0^2 + 1e-16),
ill-conditioned where P0 ~ 0: rows held to these bounds keep min |P0| over non-empty blocks above
`P0_MARGIN`; the exact-zero case (empty blocks) has rows of its own.

Hessian-vector products (`ta_hessian_vectors`, `grap_hvp_kernel`) are held to a 4th-order central stencil of
the ORACLE's analytic forces and virial (not the GPU's), to 1e-8 x max(1, max|ref|).
"""
import math
from collections import namedtuple

import numpy as np
import pytest

from tests.helpers import fcc, make_grap_nn, oracle_grap_eval, oracle_grap_model, run_child
from tests.test_gpu_sf_dispatch import alloy, check, drop
from tensoralloy_amd import Atoms

gpu = pytest.mark.gpu

G_REL = 1e-10                       # descriptors: x max(1, max|G|)
HVP_REL = 1e-8                      # Hessian-vector products: x max(1, max|ref|)
P0_MARGIN = 1e-6                    # min |P0| over non-empty blocks of new-mode rows held to fp64 bounds
N_COMP = {0: 1, 1: 4, 2: 10, 3: 20, 4: 35, 5: 56}
CHUNK = 64                          # kFwdChunk = kBwdChunk
NN_GRID_PAIRS = 2048 * 4 * 16       # pairs one trip of the nn pre-pass grid covers
WIDE_GATHER = 16384                 # force_gather: 16 lanes per atom at or above this many atoms
NET_LDS_MAX = 150 * 1024
EIGHT = ["Al", "Co", "Cu", "Fe", "Mo", "Nb", "Ni", "Ti"]   # kMaxElements = 8
SF32 = {"eta": [0.1, 0.3, 0.6, 1.0, 1.5, 2.0, 3.0, 4.0], "omega": [0.0, 1.0, 2.0, 3.0]}   # 'cross': K = 32


# -- the selection rules, restated ---------------------------------------------------------------------------

def pad16(n):
    return (n + 15) // 16 * 16


def net_sizes(nn):
    return [1] + [np.shape(w)[1] for w, _ in nn.descriptor.filter_weights]


def net_lds_bytes(sizes):
    """build_filter_net: the LDS image of grap_nn_filter_kernel for layer widths [1, h1, ..., K]."""
    pads = [pad16(s) for s in sizes[1:]]
    wstride = lambda n: n + 16 if n % 32 == 0 else n
    xs = max([16] + pads) + 2
    doubles = 2 * pads[0] + sum(pads[l - 1] * wstride(pads[l]) + pads[l] for l in range(1, len(pads)))
    return 8 * (doubles + 4 * 2 * 16 * xs)


def net_class(nn):
    """launch_grap_forward: (ACT, NT) of grap_nn_filter_kernel, or None for analytic filters."""
    if nn.descriptor.algorithm.name != "nn":
        return None
    pads = [pad16(s) for s in net_sizes(nn)[1:]]
    ntmax = max([1] + [p // 16 for p in pads[1:]])
    act = "softplus" if nn.descriptor.algorithm.activation.lower() == "softplus" else "generic"
    return act, 2 if ntmax <= 2 else 4


def frame_pairs(nn, atoms, rc=None):
    from oracle.neighbors import _complete_cell, neighbor_list
    R = np.asarray(atoms.positions, dtype=float)
    h = _complete_cell(np.asarray(atoms.get_cell(complete=True), dtype=float), np.asarray(atoms.pbc))
    return (R, h) + tuple(neighbor_list(R, h, np.asarray(atoms.pbc), rc or nn.transformer.rcut))


def segment_counts(nn, atoms):
    """[N, nel]: pairs of every (centre, neighbour species) segment, the kernels' unit of work."""
    _, _, i, j, _ = frame_pairs(nn, atoms)
    sp = np.array([nn.elements.index(s) for s in atoms.get_chemical_symbols()])
    counts = np.zeros((len(atoms), len(nn.elements)), dtype=np.int64)
    np.add.at(counts, (i, sp[j]), 1)
    return counts


def seg_class(n):
    return "0" if n == 0 else "<64" if n < CHUNK else "=64" if n == CHUNK else "65..128" if n <= 2 * CHUNK else ">128"


def selection(nn, frames):
    d = nn.descriptor
    nd = N_COMP[d.max_moment]
    counts = np.concatenate([segment_counts(nn, a).ravel() for a in frames])
    return dict(nd=nd, MC=20 if nd <= 20 else 56, K=len(d.algorithm), ktiles=(len(d.algorithm) + 15) // 16,
                filter="nn" if d.algorithm.name == "nn" else "analytic", net=net_class(nn),
                n_atoms=sum(len(a) for a in frames), n_pairs=int(counts.sum()),
                seg_min=int(counts.min()), seg_max=int(counts.max()),
                seg_classes={seg_class(int(n)) for n in np.unique(counts)})


def p0_min(nn, atoms):
    """min |P0| over the non-empty (centre, block, filter) entries whose terms H_k(r_j) change sign: there P0
    is a cancelling sum and its sign is not robust (morse filters). Entries of one-signed terms keep their sign
    whatever their size (pexp filters of ~1e-39 are fine) and count only if they underflow below 1e-300."""
    from oracle.grap import _moments
    m = oracle_grap_model(nn)
    m.moment_tensors = [0]
    g = _moments(m, atoms.get_chemical_symbols(), atoms.positions, np.asarray(atoms.get_cell(complete=True)),
                 atoms.pbc, 1e-14)
    shape = g["P"].shape[:3]
    pos, neg = np.zeros(shape), np.zeros(shape)
    np.add.at(pos, (g["pi"], g["block"]), np.maximum(g["H"], 0.0))
    np.add.at(neg, (g["pi"], g["block"]), np.minimum(g["H"], 0.0))
    n = np.zeros(shape[:2])
    np.add.at(n, (g["pi"], g["block"]), 1.0)
    P0 = np.abs(g["P"][..., 0])
    mixed = (pos > 0) & (neg < 0)
    P0 = np.where(mixed | (P0 < 1e-300), P0, np.inf)[n > 0]
    return P0.min() if P0.size else np.inf


# -- models and frames ----------------------------------------------------------------------------------------

def pexp(K, r0=1.0, dr=0.2, p0=5.0, dp=0.25):
    return {"rl": [r0 + dr * (k % 16) + 0.05 * (k // 16) for k in range(K)],
            "pl": [p0 - dp * (k % 16) + 0.1 * (k // 16) for k in range(K)]}


def sf_pair(K):
    return {"eta": [0.1 + 0.3 * k for k in range(K)], "omega": [0.2 * (k % 7) for k in range(K)]}


def grap(els, rc=6.0, algo="pexp", par=None, mom=(0, 1, 2, 3), hidden=(16,), **kw):
    return make_grap_nn(list(els), rc, list(hidden), algo, par, moment_tensors=list(mom), **kw)


def nn_net(els, hidden, K=16, act="softplus", resnet=True, modifier=0, mom=(0, 1, 2, 3), rc=6.0, seed=611):
    par = {"hidden_sizes": list(hidden), "num_filters": K, "activation": act, "use_resnet_dt": resnet,
           "h_abck_modifier": modifier}
    return make_grap_nn(list(els), rc, [16], "nn", par, moment_tensors=list(mom), seed=seed)


def shell_cluster(n, centre="Ni", other="Ni", rc=6.0, seed=0, r_lo=2.0):
    """Non-periodic: one centre with exactly n neighbours of species `other` at distinct radii in
    [r_lo, rc - 0.3] along a Fibonacci spiral: every atom has at most n neighbours, the centre exactly n."""
    rng = np.random.RandomState(seed + n)
    k = np.arange(n) + 0.5
    phi, th = np.arccos(1 - 2 * k / max(n, 1)), np.pi * (1 + 5 ** 0.5) * k
    u = np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], axis=1)
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    radii = np.linspace(r_lo, rc - 0.3, max(n, 1))[:n]
    rng.shuffle(radii)
    pos = np.concatenate([np.zeros((1, 3)), (u @ Q) * radii[:, None]]) + 20.0
    return Atoms(symbols=[centre] + [other] * n, positions=pos, cell=np.eye(3) * 40.0, pbc=False)


def isolated_frame(els, seed=3):
    """Non-periodic: three isolated atoms, a dimer, and an fcc blob with only the first element."""
    blob = fcc(els[0], rep=(1, 1, 2), a=3.6, seed=seed).positions + 30.0
    far = np.array([[0.0, 0.0, 0.0], [15.0, 0.0, 0.0], [0.0, 15.0, 0.0], [15.0, 15.0, 0.0], [17.3, 15.2, 0.4]])
    syms = [els[-1], els[0], els[-1], els[0], els[-1]] + [els[0]] * len(blob)
    return Atoms(symbols=syms, positions=np.concatenate([far, blob]), cell=np.eye(3) * 60.0, pbc=False)


Row = namedtuple("Row", "id reach model frames shortest longest")
ANY = (0, 10 ** 9)


def _rows():
    M2, M3 = ["Mo", "Ni"], ["Al", "Cu", "Ni"]
    rows = [
        # new mode, each max_moment (nd = 1 .. 56); each analytic family, both cutoffs, K = 1, 16, 17, 32
        Row("mm0-pexp-K16", dict(nd=1, MC=20, ktiles=1),
            lambda: grap(["Ni"], par=pexp(16), mom=[0]), lambda: [fcc(rep=(2, 2, 2), seed=1)], (70, 90), (70, 90)),
        Row("mm1-sf-K17-poly", dict(nd=4, MC=20, ktiles=2),
            lambda: grap(M2, algo="sf", par=sf_pair(17), mom=[1], cutoff="polynomial"),
            lambda: [alloy(M2, seed=2)], (25, 55), (25, 55)),
        Row("mm2-density-K1-sym", dict(nd=10, MC=20, ktiles=1),
            lambda: grap(M2, algo="density", par={"A": [1.0], "beta": [2.0], "re": [3.5]}, mom=[0, 2],
                         symmetric=True), lambda: [alloy(M2, seed=3)], (25, 55), (25, 55)),
        Row("mm3-morse-K32-sym", dict(nd=20, MC=20, ktiles=2),
            lambda: grap(M2, algo="morse", par={"D": [0.5, 1.0], "gamma": [0.8, 1.0, 1.2, 1.4],
                                                "r0": [1.0, 1.2, 1.4, 1.6]},
                         mom=[0, 1, 2, 3], symmetric=True, param_space_method="cross"),
            lambda: [alloy(M2, seed=4)], (25, 55), (25, 55)),
        Row("mm4-pexp-K17-3el", dict(nd=35, MC=56, ktiles=2),
            lambda: grap(M3, par=pexp(17), mom=[4], symmetric=True, cutoff="polynomial"),
            lambda: [alloy(M3, rep=(2, 2, 3), seed=5)], (15, 40), (15, 40)),
        Row("mm5-sf-K1", dict(nd=56, MC=56, ktiles=1),
            lambda: grap(M2, algo="sf", par={"eta": [0.5], "omega": [1.0]}, mom=[0, 1, 5]),
            lambda: [alloy(M2, seed=6)], (25, 55), (25, 55)),
        Row("mm5-density-K16-3el", dict(nd=56, MC=56, ktiles=1),
            lambda: grap(M3, algo="density", par={"A": [1.0, 2.0], "beta": [1.0, 2.0, 3.0, 4.0],
                                                  "re": [3.0, 4.0]}, mom=range(6), param_space_method="cross"),
            lambda: [alloy(M3, seed=7)], (15, 40), (15, 40)),
        # legacy moment subsets
        Row("legacy-0", dict(nd=1, MC=20, ktiles=1),
            lambda: grap(["Ni"], algo="morse", par={"D": [1.0, 0.5], "gamma": [1.0, 1.5], "r0": [3.3, 2.4]},
                         mom=[0], legacy_mode=True), lambda: [fcc(rep=(2, 2, 2), seed=8)], (70, 90), (70, 90)),
        Row("legacy-1", dict(nd=4, MC=20, ktiles=2),
            lambda: grap(M2, par=pexp(20), mom=[1], legacy_mode=True), lambda: [alloy(M2, seed=9)],
            (25, 55), (25, 55)),
        Row("legacy-2", dict(nd=10, MC=20, ktiles=1),
            lambda: grap(M2, algo="sf", par=sf_pair(6), mom=[2], legacy_mode=True, cutoff="polynomial"),
            lambda: [alloy(M2, seed=10)], (25, 55), (25, 55)),
        Row("legacy-02", dict(nd=10, MC=20, ktiles=1),
            lambda: grap(["Ni"], algo="density", par={"A": [1.0], "beta": [1.0, 3.0], "re": [4.0]},
                         mom=[0, 2], legacy_mode=True, param_space_method="cross"),
            lambda: [fcc(rep=(2, 2, 2), seed=11)], (70, 90), (70, 90)),
        Row("legacy-012-K32", dict(nd=10, MC=20, ktiles=2),
            lambda: grap(M3, par=pexp(32), mom=[0, 1, 2], legacy_mode=True), lambda: [alloy(M3, seed=12)],
            (15, 40), (15, 40)),
        # the largest shapes the library accepts: K = 32 with moments 0..5 (two elements: 384 features; the MLP
        # takes at most 512, so eight elements are refused, see `c_refusals`), and kMaxElements = 8 with moments
        # 0..5 at K = 10 (480 features)
        Row("max-K32-mm5-2el", dict(nd=56, MC=56, ktiles=2),
            lambda: grap(M2, algo="sf", par=SF32, mom=range(6), param_space_method="cross"),
            lambda: [alloy(M2, seed=13)], (25, 55), (25, 55)),
        Row("max-8el-K10-mm5", dict(nd=56, MC=56, ktiles=1),
            lambda: grap(EIGHT, par=pexp(10, r0=1.8), mom=range(6)),
            lambda: [alloy(EIGHT, rep=(3, 3, 2), seed=13)], (1, 20), (1, 20)),
        # the nn filter network: {softplus, generic} x {NT 2, NT 4}, widths 1 and 64, 8 layers, resnet on / off,
        # modifiers 0 / 1 / 2, K = 32, the LDS image near its limit
        Row("nn-softplus-nt2", dict(nd=20, MC=20, ktiles=1, net=("softplus", 2)),
            lambda: nn_net(["Ni"], [32, 32, 32]), lambda: [fcc(rep=(2, 2, 2), seed=14)], (70, 90), (70, 90)),
        Row("nn-softplus-nt4-K32-lds", dict(nd=20, MC=20, ktiles=2, net=("softplus", 4)),
            lambda: nn_net(M2, [64, 64], K=32, mom=[0, 1, 2, 3]), lambda: [alloy(M2, seed=15)], (25, 55), (25, 55)),
        Row("nn-tanh-nt2-width1-mm5-K20", dict(nd=56, MC=56, ktiles=2, net=("generic", 2)),
            lambda: nn_net(M2, [1, 16], K=20, act="tanh", resnet=False, modifier=1, mom=range(6)),
            lambda: [alloy(M2, seed=16)], (25, 55), (25, 55)),
        Row("nn-elu-nt4-8layers-mm4", dict(nd=35, MC=56, ktiles=1, net=("generic", 4)),
            lambda: nn_net(M2, [16, 16, 16, 16, 16, 16, 64], K=12, act="elu", modifier=2, mom=range(5)),
            lambda: [alloy(M2, seed=17)], (25, 55), (25, 55)),
        Row("nn-tanh-nt4-K32-mod2", dict(nd=10, MC=20, ktiles=2, net=("generic", 4)),
            lambda: nn_net(["Ni"], [24, 40], K=32, act="tanh", modifier=2, mom=[0, 1, 2]),
            lambda: [fcc(rep=(2, 2, 2), seed=18)], (70, 90), (70, 90)),
    ]
    # segment lengths: one centre with exactly n neighbours (chunk edges at 64 and 128)
    for n in (0, 1, 15, 16, 17, 63, 64, 65, 128, 129, 250):
        rows.append(Row(f"seg{n}", dict(nd=20, MC=20, ktiles=2),
                        lambda: grap(["Ni"], par=pexp(20, r0=1.5)), lambda n=n: [shell_cluster(n)],
                        (0 if n == 0 else 1, n), (n, n)))
    for n in (1, 17, 64, 65, 129, 250):   # the centre's own-species segment is empty
        rows.append(Row(f"seg{n}-binary-mm4", dict(nd=35, MC=56, ktiles=1),
                        lambda: grap(M2, algo="sf", par=sf_pair(8), mom=range(5)),
                        lambda n=n: [shell_cluster(n, "Mo", "Ni")], (0, 0), (n, n)))
    for n in (63, 129):
        rows.append(Row(f"seg{n}-binary-nn", dict(nd=20, MC=20, ktiles=2, net=("softplus", 2)),
                        lambda: nn_net(M2, [32, 32], K=17), lambda n=n: [shell_cluster(n, "Mo", "Ni")],
                        (0, 0), (n, n)))
    return rows


ROWS = _rows()


def check_g(r, o, tag, scale_from=None):
    """`check` (north_star + fp64 bounds) and the descriptors to 1e-10 x max(1, max|G|)."""
    dev = check(r, o, tag, descriptors=False)
    G = o["descriptors"]
    dG = np.abs(r["descriptors"] - G).max(initial=0.0)
    print(f"DEV {tag} G={dG:.2e}")
    assert dG < G_REL * max(1.0, np.abs(G).max(initial=0.0)), (tag, dG)
    assert all(np.all(np.isfinite(r[k])) for k in ("descriptors", "forces", "virial", "atomic")), tag
    return dict(dev, G=dG)


def assert_reach(row, nn, frames):
    sel = selection(nn, frames)
    for k, v in row.reach.items():
        assert sel[k] == v, (row.id, k, sel[k], v)
    assert row.shortest[0] <= sel["seg_min"] <= row.shortest[1], (row.id, sel["seg_min"], row.shortest)
    assert row.longest[0] <= sel["seg_max"] <= row.longest[1], (row.id, sel["seg_max"], row.longest)
    if not nn.descriptor.legacy_mode:
        for a in frames:
            assert p0_min(nn, a) > P0_MARGIN, (row.id, p0_min(nn, a))
    return sel


def evaluate(nn, frames, eng=None):
    from tensoralloy_amd import Engine
    if eng is not None:
        return eng.evaluate(frames, descriptors=True), int(eng.info.n_pairs)
    with Engine(nn) as e:
        return e.evaluate(frames, descriptors=True), int(e.info.n_pairs)


# -- CPU: the rows and the restatement -------------------------------------------------------------------------

def test_restatement_of_the_net_builds():
    """CPU: ACT / NT and the LDS image of the network shapes the rows and refusals use."""
    assert net_class(nn_net(["Ni"], [32, 32, 32])) == ("softplus", 2)
    assert net_class(nn_net(["Ni"], [32, 48])) == ("softplus", 4)          # NT from the widest layer after the first
    assert net_class(nn_net(["Ni"], [64, 16], K=16)) == ("softplus", 2)    # ... not from the first
    assert net_class(nn_net(["Ni"], [16], K=17, act="tanh")) == ("generic", 2)
    assert net_class(grap(["Ni"])) is None
    assert net_lds_bytes([1, 64, 64, 32]) == 134912                        # accepted, 132 KB
    assert net_lds_bytes([1, 64, 64, 64, 16]) == 159872 > NET_LDS_MAX       # refused


def test_rows_cover_every_combination():
    """CPU: every row selects what it is named after, and the rows together reach {MC 20, 56} x {K <= 16,
    17..32} x {analytic, nn}, {softplus, generic} x {NT 2, 4} and every segment class."""
    combos, nets, segs = set(), set(), set()
    for row in ROWS:
        nn, frames = row.model(), row.frames()
        sel = assert_reach(row, nn, frames)
        combos.add((sel["MC"], sel["ktiles"], sel["filter"]))
        if sel["net"]:
            nets.add(sel["net"])
            assert net_lds_bytes(net_sizes(nn)) <= NET_LDS_MAX, row.id
        segs |= sel["seg_classes"]
    assert combos == {(mc, kt, f) for mc in (20, 56) for kt in (1, 2) for f in ("analytic", "nn")}, combos
    assert nets == {(a, nt) for a in ("softplus", "generic") for nt in (2, 4)}, nets
    assert segs == {"0", "<64", "=64", "65..128", ">128"}, segs
    assert {s.descriptor.max_moment for s in (r.model() for r in ROWS)} == set(range(6))
    for n in (64, 65, 129, 250):   # the chunk edges sit in the centre's own segment
        assert segment_counts(grap(["Ni"]), shell_cluster(n))[0, 0] == n


def test_scale_rows_select_their_paths():
    """CPU: the > 131,072-pair nn row, the production frame, the > 16384-atom batch and the 64-frame batch."""
    nn, frames = big_nn()
    sel = selection(nn, frames)
    assert sel["n_pairs"] > NN_GRID_PAIRS and sel["net"] == ("softplus", 2), sel["n_pairs"]
    nn, frames = production()
    sel = selection(nn, frames)
    assert sel["n_atoms"] == 4000 and sel["K"] == 16 and sel["nd"] == 20
    nn, frames = wide_batch()
    assert selection(nn, frames)["n_atoms"] >= WIDE_GATHER
    nn, frames = batch_64()
    assert len(frames) == 64 and len({len(a) for a in frames}) > 1


def fsum_descriptors(nn, atoms):
    """The new-mode descriptors with P[i, b, k, d] summed exactly (math.fsum), then Q = T . P^2 and
    G0 = sgn(P0) sqrt(Q0 + 1e-16): a restatement of oracle/grap.py free of in-order rounding."""
    from oracle.grap import _moments, multiplicity_tensor
    m = oracle_grap_model(nn)
    g = _moments(m, atoms.get_chemical_symbols(), atoms.positions, np.asarray(atoms.get_cell(complete=True)),
                 atoms.pbc, 1e-14)
    N, nel, K, nd = g["P"].shape
    P = np.zeros_like(g["P"])
    terms = g["H"][:, :, None] * g["M"][:, None, :]
    for i in range(N):
        for b in range(nel):
            sel = np.nonzero((g["pi"] == i) & (g["block"] == b))[0]
            for k in range(K):
                for d in range(nd):
                    P[i, b, k, d] = math.fsum(terms[sel, k, d].tolist())
    T = multiplicity_tensor(m.max_moment, m.symmetric)
    Q = np.einsum("nbkd,dm->nbkm", P ** 2, T)
    Q[..., 0] = np.sign(P[..., 0]) * np.sqrt(Q[..., 0] + 1e-16)
    return Q.reshape(N, -1)


def test_oracle_sums_are_not_what_the_bound_measures():
    """CPU: on the longest segment of the table (250 neighbours) and a small periodic frame, the oracle's
    in-order sums agree with exactly rounded ones far below 1e-10: the descriptor bound measures the
    kernels, not the oracle."""
    for nn, atoms in ((grap(["Ni"], par=pexp(20, r0=1.5)), shell_cluster(250)),
                      (grap(["Mo", "Ni"], algo="sf", par=sf_pair(8), mom=range(5)), alloy(["Mo", "Ni"], seed=3))):
        G = oracle_grap_eval(nn, atoms)["descriptors"]
        d = np.abs(fsum_descriptors(nn, atoms) - G).max()
        assert d < 1e-3 * G_REL * max(1.0, np.abs(G).max()), d


# -- GPU: the rows --------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_dispatch_row(lib, row):
    nn, frames = row.model(), row.frames()
    assert_reach(row, nn, frames)
    res, _ = evaluate(nn, frames)
    for k, (atoms, r) in enumerate(zip(frames, res)):
        check_g(r, oracle_grap_eval(nn, atoms), f"{row.id}/frame{k}")


# -- scale rows ------------------------------------------------------------------------------------------------

def big_nn():
    """~1800 Ni atoms at rc 6: ~141k pairs, more than one trip of the nn pre-pass grid."""
    return nn_net(["Ni"], [32, 32], K=16, mom=[0, 1, 2]), [fcc(rep=(8, 8, 7), seed=21)]


def production():
    """scripts/bench_grap.py: the 4000-atom Ni frame of bench.py, pexp K = 16, moments 0..3, rc 6, MLP 64-64."""
    from bench import ni_frame
    from tensoralloy_amd import AtomicNN, UniversalTransformer
    from tensoralloy_amd.grap import GenericRadialAtomicPotential
    gd = GenericRadialAtomicPotential(["Ni"], "pexp", pexp(16), moment_tensors=[0, 1, 2, 3], legacy_mode=False)
    nn = AtomicNN(["Ni"], gd, hidden_sizes=[64, 64], activation="softplus", minmax_scale=False,
                  export_properties=("energy", "forces", "stress"))
    nn.attach_transformer(UniversalTransformer(["Ni"], rcut=6.0))
    nn.initialize(seed=611)
    return nn, [ni_frame(611)]


def wide_batch():
    """An uneven 18427-atom batch (16-lane force gather)."""
    nn = grap(["Mo", "Ni"], algo="sf", par={"eta": [0.1, 0.5, 1.0, 2.0], "omega": [0.0, 1.0]},
              mom=[0, 1, 2], param_space_method="cross")
    return nn, [alloy(["Mo", "Ni"], rep=(16, 16, 16), seed=22), drop(alloy(["Mo", "Ni"], rep=(8, 8, 8), seed=23), 5)]


def batch_64():
    nn = grap(["Mo", "Ni"], par=pexp(10), mom=[0, 1, 2, 3])
    frames = [drop(alloy(["Mo", "Ni"], seed=100 + k, jitter=0.03 + 0.001 * k), k % 5) if k % 5 else
              alloy(["Mo", "Ni"], seed=100 + k, jitter=0.03 + 0.001 * k) for k in range(64)]
    return nn, frames


@gpu
@pytest.mark.parametrize("case", ["nn-beyond-one-grid-trip", "production", "wide-batch", "64-frames"])
def test_scale_rows(lib, case):
    nn, frames = {"nn-beyond-one-grid-trip": big_nn, "production": production, "wide-batch": wide_batch,
                  "64-frames": batch_64}[case]()
    res, n_pairs = evaluate(nn, frames)
    if case == "nn-beyond-one-grid-trip":
        assert n_pairs > NN_GRID_PAIRS, n_pairs
    if case == "wide-batch":
        assert sum(len(a) for a in frames) >= WIDE_GATHER
    if case == "64-frames":
        assert len({round(r["energy"], 9) for r in res}) == 64
    for k, (atoms, r) in enumerate(zip(frames, res)):
        if case != "64-frames" or k % 9 == 0 or k == 63:
            assert p0_min(nn, atoms) > P0_MARGIN, (case, k)
        check_g(r, oracle_grap_eval(nn, atoms), f"{case}-{n_pairs}pairs/frame{k}")


@gpu
@pytest.mark.parametrize("algo", ["pexp", "nn"])
def test_reused_engine_grows_and_shrinks(lib, algo):
    """One engine: small, large (Pbuf and, for nn, Hbuf grow), then a different small batch that reads a
    Hbuf larger than its pairs (stale rows beyond them are padding); each against the oracle."""
    from tensoralloy_amd import Engine
    nn = nn_net(["Mo", "Ni"], [32, 32], K=17) if algo == "nn" else grap(["Mo", "Ni"], par=pexp(17))
    batches = [[alloy(["Mo", "Ni"], seed=31)],
               [alloy(["Mo", "Ni"], rep=(5, 5, 5), seed=32), alloy(["Mo", "Ni"], rep=(3, 3, 3), seed=33)],
               [drop(alloy(["Mo", "Ni"], seed=34), 3), shell_cluster(17, "Mo", "Ni")]]
    with Engine(nn) as eng:
        pairs = []
        for s, frames in enumerate(batches):
            res, n_pairs = evaluate(nn, frames, eng)
            pairs.append(n_pairs)
            for k, (atoms, r) in enumerate(zip(frames, res)):
                check_g(r, oracle_grap_eval(nn, atoms), f"reuse-{algo}/batch{s}/frame{k}")
    assert pairs[0] < pairs[1] and pairs[2] < pairs[1] // 10, pairs


@gpu
@pytest.mark.parametrize("nspec", [2, 3])
def test_absent_species_and_isolated_atoms(lib, nspec):
    """A frame without the last species, and a non-periodic frame with isolated atoms and a dimer: the
    features of every empty block are exactly 0 (P0 = 0: the sgn(0) branches of the forward and backward
    kernels), every result is finite, everything matches the oracle."""
    els = ["Al", "Cu", "Ni"][:nspec] if nspec == 3 else ["Mo", "Ni"]
    for algo in ("pexp", "nn"):
        nn = nn_net(els, [32, 32], K=17, mom=range(5)) if algo == "nn" else grap(els, par=pexp(12), mom=range(4))
        frames = [alloy(els[:-1], seed=41), isolated_frame(els), alloy(els, rep=(2, 2, 3), seed=42)]
        res, _ = evaluate(nn, frames)
        K, nf = len(nn.descriptor.algorithm), nn.descriptor.features_per_filter
        for k, (atoms, r) in enumerate(zip(frames, res)):
            counts = segment_counts(nn, atoms)
            sym = atoms.get_chemical_symbols()
            from oracle.sf import radial_term_index
            empty = 0
            for c in range(len(atoms)):
                for sb, el in enumerate(nn.elements):
                    if counts[c, sb] == 0:
                        tb = radial_term_index(nn.elements, sym[c], el)
                        assert np.all(r["descriptors"][c, tb * K * nf:(tb + 1) * K * nf] == 0.0), (algo, k, c, el)
                        empty += 1
            assert (empty > 0) == (k < 2), (algo, k, empty)
            check_g(r, oracle_grap_eval(nn, atoms), f"empty-{nspec}el-{algo}/frame{k}")


# -- the library's switches, each in a fresh process ------------------------------------------------------------

def switch_cases():
    """(name, model, frames): an analytic row (compact records by default) and an nn row."""
    return [("pexp-K17", grap(["Mo", "Ni"], par=pexp(17), mom=range(4)),
             [alloy(["Mo", "Ni"], seed=51), drop(alloy(["Mo", "Ni"], rep=(2, 2, 3), seed=52), 3)]),
            ("nn-mm5", nn_net(["Mo", "Ni"], [32, 32], K=12, mom=range(6), modifier=1),
             [alloy(["Mo", "Ni"], seed=53)])]


@gpu
@pytest.mark.parametrize("var", ["TA_FULL_RECORDS", "TA_NO_OWN_SUMS"])
def test_switches_in_a_fresh_process(lib, var):
    """TA_FULL_RECORDS (64-byte pair records on the analytic path) and TA_NO_OWN_SUMS (force_gather without
    the backward's own-side sums): against the oracle and against the default process's results at 1e-12."""
    out = run_child("tests.test_gpu_grap_dispatch:switch_cases", {var: "1"})
    cases = switch_cases()
    assert [c["name"] for c in out] == [c[0] for c in cases]
    for case, (name, nn, frames) in zip(out, cases):
        base, _ = evaluate(nn, frames)
        for k, (atoms, r, b) in enumerate(zip(frames, case["res"], base)):
            check_g(r, oracle_grap_eval(nn, atoms), f"{var}/{name}/frame{k}")
            for key in ("descriptors", "forces", "virial", "atomic"):
                d = np.abs(r[key] - b[key]).max()
                assert d <= 1e-12 * max(1.0, np.abs(b[key]).max()), (var, name, key, d)
            assert abs(r["energy"] - b["energy"]) <= 1e-12 * max(1.0, abs(b["energy"])), (var, name)


# -- MD path: GRAP runs on the skin list itself (pairs beyond rc in its segments) ---------------------------------

@gpu
@pytest.mark.parametrize("algo", ["pexp", "nn"])
@pytest.mark.parametrize("nspec", [1, 2])
def test_md_skin_list_against_the_oracle(lib, algo, nspec):
    """ta_update_positions + compute and ta_step on an uneven 2-frame batch with a Verlet skin: list reuses,
    rebuilds and a cell change, every step against the oracle at the new geometry."""
    from tensoralloy_amd import Engine, _lib
    els = ["Mo", "Ni"][:nspec] if nspec == 2 else ["Ni"]
    want = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES | _lib.TA_WANT_VIRIAL | _lib.TA_WANT_ATOMIC
    nn = nn_net(els, [32, 32], K=17) if algo == "nn" else grap(els, par=pexp(17))
    frames = [drop(alloy(els, rep=(3, 2, 2), seed=61), 3), drop(alloy(els, rep=(2, 2, 3), a=3.55, seed=62), 2)]
    sizes = np.cumsum([0] + [len(a) for a in frames])
    cells = np.array([np.asarray(a.get_cell()) for a in frames])
    rng = np.random.RandomState(nspec)
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        eng.set_frames(frames)
        pos = np.concatenate([a.positions for a in frames])
        for step in range(7):
            pos = pos + rng.normal(0, 0.2 if step % 3 == 2 else 0.02, pos.shape)
            new_cells = None
            if step == 5:   # a cell change: strain every frame by 1 %
                cells = cells * 1.01
                pos = pos * 1.01
                new_cells = cells
            if step % 2:
                got = {k: np.array(v) for k, v in eng.step(pos, want, cells=new_cells).items()}
            else:
                eng.update_positions(pos, cells=new_cells)
                eng.compute(want)
                got = eng.fetch(want)
            for f, atoms in enumerate(frames):
                moved = Atoms(symbols=atoms.get_chemical_symbols(), positions=pos[sizes[f]:sizes[f + 1]],
                              cell=cells[f], pbc=True)
                r = dict(energy=got["energy"][f], atomic=got["atomic"][sizes[f]:sizes[f + 1]],
                         forces=got["forces"][sizes[f]:sizes[f + 1]], virial=got["virial"][f])
                assert p0_min(nn, moved) > P0_MARGIN
                check(r, oracle_grap_eval(nn, moved), f"md-{algo}-{nspec}el/step{step}/frame{f}", descriptors=False)
        builds, reuses = eng.list_stats()
        assert builds + reuses == 8 and builds >= 2 and reuses >= 2, (builds, reuses)


# -- refusals ---------------------------------------------------------------------------------------------------

def _crafted(head, tail):
    return np.concatenate([np.array(head, dtype=np.float64), np.asarray(tail, dtype=np.float64)])


def c_refusals():
    """(name, model, message): models whose grap_params `grap_create` / `build_filter_net` refuse. The first
    four bypass the Python checks with a hand-written parameter block."""
    out = []
    for name, head, tail, msg in (
            ("K33", [3, 33, 2, 0, 0, 7], np.tile([2.0, 3.0, 0.0], 33), "1..32 radial filters"),
            ("moment6", [3, 4, 6, 0, 0, 127], np.tile([2.0, 3.0, 0.0], 4), "should be <= 5"),
            ("legacy-moment3", [3, 4, 3, 1, 0, 9], np.tile([2.0, 3.0, 0.0], 4), "moments 0, 1, 2 only"),
            ("legacy-nn", [4, 16, 2, 1, 0, 7], [], "non-legacy")):
        nn = grap(["Ni"], par=pexp(4), mom=[0, 1, 2])
        nn.descriptor.flat_parameters = lambda h=head, t=tail: _crafted(h, t)
        out.append((name, nn, msg))
    out.append(("9-layers", nn_net(["Ni"], [16] * 8), "2..8 dense layers"))
    out.append(("width65", nn_net(["Ni"], [65]), "layer widths 1..64"))
    out.append(("lds", nn_net(["Ni"], [64, 64, 64]), "LDS image"))
    out.append(("8el-K32-mm5", grap(EIGHT, algo="sf", par=SF32, mom=range(6), param_space_method="cross"),
                "1..512"))   # 1536 features: the MLP's input limit
    return out


def test_python_refusals():
    """CPU: the Python side refuses K = 33, max_moment 6, legacy with moment 3 and legacy `nn`."""
    with pytest.raises(ValueError, match="at most 32 radial filters"):
        grap(["Ni"], par=pexp(33))
    with pytest.raises(ValueError, match="should be <= 5"):
        grap(["Ni"], mom=[0, 6])
    with pytest.raises(ValueError, match="moments 0, 1, 2 only"):
        grap(["Ni"], mom=[0, 3], legacy_mode=True).descriptor.flat_parameters()
    with pytest.raises(ValueError, match="legacy_mode=False"):
        make_grap_nn(["Ni"], 6.0, [16], "nn", legacy_mode=True)
    lds = {name: nn for name, nn, _ in c_refusals()}["lds"]
    assert net_lds_bytes(net_sizes(lds)) > NET_LDS_MAX


@gpu
def test_refusals_then_a_valid_model(lib):
    """Every C-side refusal ends in a ValueError naming the limit; the process then evaluates a valid model
    (the near-limit LDS image) correctly."""
    from tensoralloy_amd import Engine
    for name, nn, msg in c_refusals():
        with pytest.raises(ValueError, match=msg):
            Engine(nn)
    nn, frames = nn_net(["Mo", "Ni"], [64, 64], K=32), [alloy(["Mo", "Ni"], seed=71)]
    res, _ = evaluate(nn, frames)
    check_g(res[0], oracle_grap_eval(nn, frames[0]), "after-refusals")


# -- Hessian-vector products against the oracle ---------------------------------------------------------------

def hvp_cases():
    """Cutoffs in the gap between two neighbour shells (fcc Ni: 5.57 / 6.10 A, a = 3.6: 5.69 / 6.24 A), so that
    no pair comes near rc within the stencil's reach (`rc_margin`)."""
    M2, NI, AL = ["Mo", "Ni"], 5.84, 5.96
    ni = lambda seed: fcc(rep=(2, 2, 2), seed=seed, jitter=0.05)
    return {
        "pexp": (lambda: grap(["Ni"], NI, par=pexp(16), mom=range(4), hidden=[32, 32]), lambda: ni(3)),
        "sf-poly": (lambda: grap(["Ni"], NI, algo="sf", par=sf_pair(6), mom=range(3), cutoff="polynomial",
                                 symmetric=True), lambda: ni(4)),
        "morse": (lambda: grap(["Ni"], NI, algo="morse", par={"D": [1.0, 0.5], "gamma": [1.0, 1.4], "r0": [1.2, 1.6]},
                               mom=range(4)), lambda: ni(5)),
        "density": (lambda: grap(["Ni"], NI, algo="density", par={"A": [1.0], "beta": [1.0, 2.0, 4.0], "re": [4.0]},
                                 mom=range(6), param_space_method="cross"), lambda: ni(6)),
        "legacy": (lambda: grap(["Ni"], NI, algo="sf", par=sf_pair(4), mom=[0, 2], legacy_mode=True), lambda: ni(7)),
        "two-elements": (lambda: grap(M2, AL, par=pexp(17), mom=range(4), symmetric=True), lambda: alloy(M2, seed=11)),
        "nn-mod2": (lambda: nn_net(M2, [32, 32], K=8, modifier=2, rc=AL), lambda: alloy(M2, seed=9)),
        # K = 32 and moments 0..5 fill grap_hvp_kernel's per-lane H[32], Hp[32], M[56]; one element: the
        # second-order MLP pass takes at most 288 features
        "max-K32-mm5": (lambda: grap(["Ni"], NI, algo="sf", par=SF32, mom=range(6), param_space_method="cross"),
                        lambda: ni(10)),
    }


HVP_EPS = 5e-4


def hvp_directions(atoms, seed=2):
    n = len(atoms)
    rng = np.random.RandomState(seed)
    dR = rng.normal(size=(2, n, 3))
    dh = rng.normal(size=(2, 3, 3)) * 0.3
    dR[1] = 0.0   # a pure cell direction
    return dR, dh


def stencil(nn, atoms, dR, dh, eps, evaluator=oracle_grap_eval):
    """dF, dW along (dR, dh): (f(-2e) - 8 f(-e) + 8 f(e) - f(2e)) / (12 e) of the oracle's forces / virial
    (`evaluator`: the oracle of the model's family; test_gpu_hvp_oracle.py passes the SF and EAM ones)."""
    h = np.asarray(atoms.get_cell(complete=True), dtype=float)
    F, W = 0.0, 0.0
    for s, c in ((2, -1.0), (1, 8.0), (-1, -8.0), (-2, 1.0)):
        a = Atoms(symbols=atoms.get_chemical_symbols(), positions=atoms.positions + s * eps * dR,
                  cell=h + s * eps * dh, pbc=atoms.pbc)
        o = evaluator(nn, a)
        F = F + c * o["forces"] / (12 * eps)
        W = W + c * o["virial"] / (12 * eps)
    return F, W


def rc_margin(nn, atoms, dR, dh, rc=None):
    """min over pairs near rc of |r - rc| / |dD|: how far (in units of the step) the stencil stays from rc
    (`rc`: another radius than the model's rcut, e.g. its angular cutoff)."""
    rc = rc or nn.transformer.rcut
    R, h, i, j, S = frame_pairs(nn, atoms, rc + 0.5)
    D = R[j] - R[i] + S @ h
    dD = dR[j] - dR[i] + S @ dh
    r = np.linalg.norm(D, axis=1)
    return (np.abs(r - rc) / np.maximum(np.linalg.norm(dD, axis=1), 1e-300)).min()


@pytest.mark.parametrize("kind", list(hvp_cases()))
def test_stencil_is_far_below_the_bound(kind):
    """CPU: the 4th-order stencil with step e and e/2 agree to 2 % of the HVP bound (the error of step e is
    its truncation, 16 times that of e/2; below e/2 rounding takes over), and no pair comes within 8 steps
    of rc along either direction (the stencil reaches 2)."""
    model, frame = hvp_cases()[kind]
    nn, atoms = model(), frame()
    dR, dh = hvp_directions(atoms)
    for d in range(2):
        assert rc_margin(nn, atoms, dR[d], dh[d]) > 8 * HVP_EPS, kind
        F1, W1 = stencil(nn, atoms, dR[d], dh[d], HVP_EPS)
        F2, W2 = stencil(nn, atoms, dR[d], dh[d], HVP_EPS / 2)
        assert np.abs(F1 - F2).max() < 2e-2 * HVP_REL * max(1.0, np.abs(F1).max()), (kind, d, np.abs(F1 - F2).max())
        assert np.abs(W1 - W2).max() < 2e-2 * HVP_REL * max(1.0, np.abs(W1).max()), (kind, d, np.abs(W1 - W2).max())


@gpu
@pytest.mark.parametrize("kind", list(hvp_cases()))
def test_hessian_vectors_against_the_oracle(lib, kind):
    from tensoralloy_amd import Engine
    model, frame = hvp_cases()[kind]
    nn, atoms = model(), frame()
    dR, dh = hvp_directions(atoms)
    with Engine(nn) as eng:
        eng.set_frames([atoms])
        dF, dW = eng.hessian_vectors(dR=dR, dh=dh[:, None], want_virial=True)
    for d in range(2):
        F, W = stencil(nn, atoms, dR[d], dh[d], HVP_EPS)
        devF, devW = np.abs(dF[d] - F).max(), np.abs(dW[d, 0] - W).max()
        print(f"DEV hvp-{kind}/dir{d} dF={devF:.2e} dW={devW:.2e}")
        assert devF < HVP_REL * max(1.0, np.abs(F).max()), (kind, d, devF)
        assert devW < HVP_REL * max(1.0, np.abs(W).max()), (kind, d, devW)
