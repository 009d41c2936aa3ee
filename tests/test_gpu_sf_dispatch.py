"""
The second-generation angular kernels (ta_kernels_v2.hip) instantiation by instantiation, against the C oracle.

The host dispatcher picks one `g4_forward_v2_kernel` / `backward_v2_kernel` build per launch from
  * the (species, gamma, zeta) chunk shape: the 14 keys of `TA_DISPATCH_V2`;
  * the length of the Hd(u) series `hd_series` (ta_api.hip) derives from beta: 12, 16, 24 or 0 (exact);
  * whether the chunk's zeta is exactly (1, 4);
  * the records-per-workgroup cap: 192 (`kCapMin`, with builds of its own) or up to 1024 from `nnl_max`.
Every row below names the build it is meant to reach and asserts the inputs that select it (the series
class of its beta, restated on the CPU in `test_hd_series_classes_of_the_rows`, and `nnl_max` inside its
window), so a change of geometry or series cannot quietly move a row to another build.

Besides the north_star bounds (1e-6 eV, 1e-5 eV/A), results are held to what fp64 kernels owe an fp64
oracle: descriptors to 1e-10, energies to 1e-9 x max(1, |E|), forces to 1e-9 x max(1, max|F|), virial to
1e-8 x max(1, max|W|). A series coefficient off by one part in 1e-8 passes north_star and fails these.

Also here: the environment switches TA_NO_JOBS, TA_FWD_WPE, TA_BWD_WPE and TA_FULL_RECORDS, which the library
reads when a handle is created and keeps for that handle (each set before its engine exists and deleted
after), and the MD path (exact list filtered on the device from the skin list) for multi-species models.

The first-generation kernels (ta_kernels.hip) appear here only as the fallback beyond 1024 neighbours; their
eight builds, their chunk chain and their callers are held to the same bounds in tests/test_gpu_sf_v1.py.
"""
import os

import numpy as np
import pytest

from tests.helpers import fcc, make_nn, mirror_launch
from tensoralloy_amd import Atoms

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_TOL, F_TOL, W_TOL = 1e-6, 1e-5, 1e-6     # north_star (virial: test_gpu_sf's bound)
G_TOL = 1e-10                               # descriptors
E_REL, F_REL, W_REL = 1e-9, 1e-9, 1e-8      # x max(1, |E|), max(1, max|F|), max(1, max|W|)

ELEMENTS = {1: ["Ni"], 2: ["Mo", "Ni"], 3: ["Al", "Cu", "Ni"], 4: ["Al", "Cu", "Mo", "Ni"],
            5: ["Al", "Co", "Cu", "Fe", "Ni"]}
KEYS = [111, 112, 121, 122, 211, 212, 221, 222, 311, 312, 321, 322, 422, 522]   # TA_DISPATCH_V2

# class -> (beta, cutoff, n_hd the series must pick, zeta for nz = 2, zeta for nz = 1)
CLASSES = {
    "h12": (0.005, "cosine", 12, (1.0, 4.0), None),          # <.., 12, true, kCapMin[, 6]> / <.., 12, true, 0>
    "h16": (0.2, "cosine", 16, (1.0, 4.0), None),            # <.., 16, true, 0>
    "generic": (0.05, "cosine", 12, (1.0, 2.0), (2.0,)),     # <.., 16, false, 0>: any n_hd <= 16, other zeta
    "h24": (3.0, "cosine", 24, (1.0, 4.0), (4.0,)),          # <.., 24, false, 0>
    "exact_cos": (10.0, "cosine", 0, (1.0, 2.0), (1.0,)),    # <.., 0, false, 0>
    "exact_poly": (1.0, "polynomial", 0, (1.0, 4.0), (2.0,)),
}
# cap -> (rc, nnl_max window) for the 32-atom fcc cell of `alloy` (a = 3.6)
CAPS = {192: (5.0, 1, 192), 256: (8.6, 193, 256), 1024: (14.05, 961, 1024), "v1": (14.5, 1025, 1150)}

MULTI = dict(beta=[0.005, 3.0, 10.0], gamma=[1.0, -1.0, 0.5], zeta=[1.0, 4.0, 2.0])   # h12 + h24 + exact


def hd_series_length(beta, cutoff="cosine"):
    """`hd_series` (ta_api.hip) restated in long double: the number of coefficients (12, 16, 24) of the
    Chebyshev-economised series of Hd(u) = exp(-beta u) (1 + cos(pi sqrt u)) / 2 whose error bound is below
    1e-17 (1e-15 for the derivative), or 0 = the exact path."""
    if cutoff != "cosine" or not beta >= 0.0:
        return 0
    L = np.longdouble
    NT, N0 = 64, 40
    pi2 = L("9.869604401089358618834490999876151135")
    fc, ex = np.zeros(NT, dtype=L), np.zeros(NT, dtype=L)
    t = L(1)
    for k in range(NT):
        fc[k] = L(0.5) * t + (L(0.5) if k == 0 else L(0))
        t *= -pi2 / L((2 * k + 1) * (2 * k + 2))
    t = L(1)
    for k in range(NT):
        ex[k] = t
        t *= -L(beta) / L(k + 1)
    prod = np.array([sum((fc[j] * ex[k - j] for j in range(k + 1)), L(0)) for k in range(NT)], dtype=L)
    ts = np.zeros((N0, N0), dtype=L)            # ts[n][k]: coefficient of u^k in T*_n(u) = T_n(2u - 1)
    ts[0, 0], ts[1, 0], ts[1, 1] = 1, -1, 2
    for n in range(1, N0 - 1):
        for k in range(n + 2):
            ts[n + 1, k] = (4 * ts[n, k - 1] if k > 0 else L(0)) - 2 * ts[n, k] - ts[n - 1, k]
    tail = np.sum(np.abs(prod[N0:]))
    dtail = np.sum(np.arange(N0, NT).astype(L) * np.abs(prod[N0:]))
    for n in (12, 16, 24):
        a, err, derr = prod[:N0].copy(), tail, dtail
        for d in range(N0 - 1, n - 1, -1):
            q = a[d] / ts[d, d]
            a[:d + 1] -= q * ts[d, :d + 1]
            err += abs(q)
            derr += 2 * L(d) * L(d) * abs(q)
        if err < L("1e-17") and derr < L("1e-15"):
            return n
    return 0


def alloy(elements, rep=(2, 2, 2), a=3.6, seed=3, jitter=0.05):
    """fcc cell with the elements dealt in turn and shuffled: every species pair is present."""
    atoms = fcc(rep=rep, a=a, seed=seed, jitter=jitter)
    syms = [elements[k % len(elements)] for k in range(len(atoms))]
    np.random.RandomState(seed).shuffle(syms)
    return Atoms(symbols=syms, positions=atoms.positions, cell=np.asarray(atoms.get_cell()), pbc=True)


def drop(atoms, n):
    """`atoms` without its last `n` atoms (uneven frame sizes)."""
    return Atoms(symbols=atoms.get_chemical_symbols()[:-n], positions=atoms.positions[:-n],
                 cell=np.asarray(atoms.get_cell()), pbc=atoms.pbc)


def sparse_cluster(elements, seed=5):
    """Non-periodic: isolated atoms, dimers and one trimer far apart, then a compact group: most centres
    have 0 or 1 neighbour, so one angular workgroup owns its full 16 centres."""
    rng = np.random.RandomState(seed)
    pos, k = [], 0
    for g in range(14):
        base = np.array([(g % 4) * 9.0, (g // 4) * 9.0, 0.0])
        n = [1, 2, 2, 3][g % 4]
        for m in range(n):
            pos.append(base + np.array([1.0 + 1.1 * m, 0.3 * m, 0.2 * m]) + rng.normal(0, 0.05, 3))
            k += 1
    blob = fcc(rep=(1, 1, 2), a=3.6, seed=seed).positions + np.array([0.0, 0.0, 12.0])
    pos = np.concatenate([np.array(pos), blob])
    syms = [elements[i % len(elements)] for i in range(len(pos))]
    return Atoms(symbols=syms, positions=pos, cell=np.zeros((3, 3)), pbc=False)


def rc_for_nnl(atoms, target, rc_hi=9.5):
    """A cutoff for which the largest neighbour count of `atoms` is exactly `target`: halfway between the
    distance that lets the first atom reach `target` neighbours and the one that lets any reach target + 1."""
    from oracle.neighbors import neighbor_list
    R, h = atoms.positions, np.asarray(atoms.get_cell(complete=True))
    i, j, S = neighbor_list(R, h, atoms.pbc, rc_hi)
    d = np.linalg.norm(R[j] - R[i] + S @ h, axis=1)
    per = [np.sort(d[i == a]) for a in range(len(atoms))]
    lo = min(p[target - 1] for p in per)
    hi = min(p[target] for p in per)
    assert hi - lo > 1e-6, (lo, hi)
    return 0.5 * (lo + hi)


def c_oracle(nn, atoms):
    from bench import host_cores
    from oracle import csf
    from tests.helpers import oracle_model
    m = oracle_model(nn)
    return csf.run(m, csf.prepare(m, atoms.get_chemical_symbols(), atoms.positions,
                                  np.asarray(atoms.get_cell(complete=True)), atoms.pbc), True, host_cores())


def descriptors_fsum(nn, atoms):
    """The oracle's descriptors (oracle/sf.py: same terms, symmetric triples, acut = rc) with every sum
    exactly rounded (math.fsum). The C oracle adds the up to 5e5 triple terms of a centre one after the
    other, which alone costs ~2e-10 at 1000 neighbours: above a few hundred neighbours that, not the
    kernels, is what a 1e-10 bound would measure."""
    import math
    from oracle.neighbors import neighbor_list
    from oracle.sf import angular_params, angular_term_index, cutoff, radial_params, radial_term_index
    from tests.helpers import oracle_model
    m = oracle_model(nn)
    assert m.acut == m.rcut and m.symmetric and m.angular
    els, sym = m.elements, atoms.get_chemical_symbols()
    rad, ang = radial_params(m.eta, m.omega), angular_params(m.beta, m.gamma, m.zeta)
    nr, na = len(rad), len(ang)
    R, h = atoms.positions, np.asarray(atoms.get_cell(complete=True))
    i, j, S = neighbor_list(R, h, atoms.pbc, m.rcut)
    D = R[j] - R[i] + S @ h
    r = np.sqrt(np.sum(D * D, axis=1) + 1e-14)
    G = np.zeros((len(R), m.ndim))
    for c in range(len(R)):
        sel = np.nonzero(i == c)[0]
        Dc, rr, jj = D[sel], r[sel], j[sel]
        f, _ = cutoff(rr, m.rcut, m.cutoff_function)
        pt = np.array([radial_term_index(els, sym[c], sym[b]) for b in jj], dtype=np.int64)
        for k, (eta, omega) in enumerate(rad):
            v = np.exp(-eta * (rr - omega) ** 2 / m.rcut ** 2) * f
            for t in np.unique(pt):
                G[c, t * nr + k] = math.fsum(v[pt == t].tolist())
        ta, tb = np.triu_indices(len(sel), 1)
        ra, rb = rr[ta], rr[tb]
        Djk = Dc[tb] - Dc[ta]
        rd = np.sqrt(np.sum(Djk * Djk, axis=1) + 1e-14)
        fprod = f[ta] * f[tb] * cutoff(rd, m.rcut, m.cutoff_function)[0]
        cos = (ra * ra + rb * rb - rd * rd) / (2.0 * ra * rb)
        z = (ra * ra + rb * rb + rd * rd) / m.rcut ** 2
        sj = np.array([els.index(x) for x in sym])[jj]
        tt = np.array([[angular_term_index(els, els[a], els[b]) for b in range(len(els))] for a in range(len(els))])
        tt = tt[sj[ta], sj[tb]]
        for k, (beta, gamma, zeta) in enumerate(ang):
            v = 2.0 ** (1.0 - zeta) * (1.0 + gamma * cos) ** zeta * np.exp(-beta * z) * fprod
            for t in np.unique(tt):
                G[c, m.n_radial + t * na + k] = math.fsum(v[tt == t].tolist())
    return G


def check(r, o, tag="", descriptors=True):
    """north_star and the fp64 bounds; returns the deviations (also printed, for the record)."""
    dev = dict(E=abs(r["energy"] - o["energy"]), e=np.abs(r["atomic"] - o["atomic"]).max(initial=0.0),
               F=np.abs(r["forces"] - o["forces"]).max(initial=0.0), W=np.abs(r["virial"] - o["virial"]).max())
    if descriptors:
        dev["G"] = np.abs(r["descriptors"] - o["descriptors"]).max(initial=0.0)
    print(f"DEV {tag} " + " ".join(f"{k}={v:.2e}" for k, v in dev.items()))
    assert dev["E"] < E_TOL and dev["e"] < E_TOL and dev["F"] < F_TOL and dev["W"] < W_TOL, (tag, dev)
    e_scale = max(1.0, abs(o["energy"]))
    assert dev["E"] < E_REL * e_scale, (tag, dev)
    assert dev["e"] < E_REL * e_scale, (tag, dev)
    assert dev["F"] < F_REL * max(1.0, np.abs(o["forces"]).max(initial=0.0)), (tag, dev)
    assert dev["W"] < W_REL * max(1.0, np.abs(o["virial"]).max()), (tag, dev)
    if descriptors:
        assert dev["G"] < G_TOL, (tag, dev)
    return dev


def run_rows(nn, frames, window, tag):
    from tensoralloy_amd import Engine
    with Engine(nn) as eng:
        res = eng.evaluate(frames, descriptors=True)
        nnl = int(eng.info.nnl_max)
        assert window[0] <= nnl <= window[1], (tag, nnl, window)
    for k, (atoms, r) in enumerate(zip(frames, res)):
        o = c_oracle(nn, atoms)
        if window[0] > 384:   # descriptors: exactly rounded sums (see descriptors_fsum)
            o["descriptors"] = descriptors_fsum(nn, atoms)
        check(r, o, f"{tag}/frame{k}")
    return res


def _matrix():
    rows = []
    for key in KEYS:
        nspec, ng, nz = key // 100, key // 10 % 10, key % 10
        for cls, (beta, cutoff, n_hd, z2, z1) in CLASSES.items():
            zeta = z2 if nz == 2 else z1
            if zeta is None:
                continue
            caps = (192, 256) if cls == "h12" else (192,)   # cap != kCapMin: the <.., 12, true, 0> builds
            for cap in caps:
                rows.append((key, cls, cap))
    return rows


MATRIX = _matrix()


def matrix_model(key, cls, cap):
    nspec, ng, nz = key // 100, key // 10 % 10, key % 10
    beta, cutoff, n_hd, z2, z1 = CLASSES[cls]
    kw = dict(eta=[0.05, 4.0, 20.0], beta=[beta], gamma=[1.0, -1.0][:ng], zeta=list(z2 if nz == 2 else z1))
    return make_nn(ELEMENTS[nspec], CAPS[cap][0], True, [16], cutoff=cutoff, sf_kwargs=kw, seed=key)


def test_hd_series_classes_of_the_rows():
    """CPU: each row's beta lands in the series class the row is named after."""
    assert [hd_series_length(b) for b in (0.005, 0.05, 0.1, 1.0, 2.0, 4.0, 8.0)] == [12, 12, 16, 16, 24, 24, 0]
    for cls, (beta, cutoff, n_hd, _, _) in CLASSES.items():
        assert hd_series_length(beta, cutoff) == n_hd, cls
    assert [hd_series_length(b) for b in MULTI["beta"]] == [12, 24, 0]
    keys = {k for k, _, _ in MATRIX}
    assert keys == set(KEYS) and len(MATRIX) == 8 * 7 + 6 * 4


def test_rows_geometry_windows():
    """CPU: the cells and cutoffs of the cap windows give the neighbour counts the rows assert on the GPU."""
    from oracle.neighbors import neighbor_list
    for cap, (rc, lo, hi) in CAPS.items():
        atoms = alloy(ELEMENTS[1])
        i, _, _ = neighbor_list(atoms.positions, np.asarray(atoms.get_cell()), atoms.pbc, rc)
        assert lo <= np.bincount(i).max() <= hi, cap
    atoms = alloy(ELEMENTS[1])
    for target in (192, 193):
        i, _, _ = neighbor_list(atoms.positions, np.asarray(atoms.get_cell()), atoms.pbc, rc_for_nnl(atoms, target))
        assert np.bincount(i).max() == target


@gpu
@pytest.mark.parametrize("key,cls,cap", MATRIX, ids=[f"{k}-{c}-cap{p}" for k, c, p in MATRIX])
def test_dispatch_matrix(lib, key, cls, cap):
    nspec = key // 100
    nn = matrix_model(key, cls, cap)
    frames = [alloy(ELEMENTS[nspec])]
    if cap == 192:
        frames.append(alloy(ELEMENTS[nspec], rep=(2, 2, 3), seed=17, jitter=0.08))
    _, lo, hi = CAPS[cap]
    run_rows(nn, frames, (lo, hi), f"{key}-{cls}-cap{cap}")


@gpu
@pytest.mark.parametrize("nspec", [1, 5])
def test_cap_1024_largest_lds(lib, nspec):
    """nnl_max in 961-1024: cap 1024, the largest forward LDS footprint (~84 KB with one species, ~138 KB with
    five and the job lists), default grid and a mixed-class grid."""
    frame = alloy(ELEMENTS[nspec])
    rc, lo, hi = CAPS[1024]
    run_rows(make_nn(ELEMENTS[nspec], rc, True, [16], sf_kwargs=dict(eta=[0.05, 4.0])), [frame], (lo, hi),
             f"cap1024-{nspec}el")
    if nspec == 1:
        nn = make_nn(ELEMENTS[1], rc, True, [16], sf_kwargs=dict(eta=[0.05], beta=[3.0, 10.0]))
        run_rows(nn, [frame], (lo, hi), "cap1024-h24-exact")


@gpu
def test_first_generation_fallback_and_clean_refusal(lib):
    """nnl_max 1025-1150: beyond kCapMax, the first-generation kernels (still correct). Above their LDS limit
    (~1150) the batch is refused with a ValueError and the handle stays usable."""
    from tensoralloy_amd import Engine
    rc, lo, hi = CAPS["v1"]
    run_rows(make_nn(ELEMENTS[1], rc, True, [16], sf_kwargs=dict(eta=[0.05, 4.0])), [alloy(ELEMENTS[1])],
             (lo, hi), "v1-fallback")
    nn = make_nn(ELEMENTS[2], 15.5, True, [16], sf_kwargs=dict(eta=[0.05, 4.0]))
    small = sparse_cluster(ELEMENTS[2])
    with Engine(nn) as eng:
        with pytest.raises(ValueError, match="1150 neighbours"):
            eng.set_frames([alloy(ELEMENTS[2])])   # ~1365 neighbours
        assert eng._lib.ta_compute(eng._handle, 1) != 0    # nothing resident to run on
        r = eng.evaluate([small], descriptors=True)[0]
        assert int(eng.info.nnl_max) <= 1150
    check(r, c_oracle(nn, small), "after-refusal")


@gpu
@pytest.mark.parametrize("nspec", [1, 2])
@pytest.mark.parametrize("target", [192, 193])
def test_exact_cap_boundary(lib, nspec, target):
    """nnl_max exactly 192 (the kCapMin builds) and 193 (cap 256, the generic-cap builds)."""
    atoms = alloy(ELEMENTS[nspec])
    rc = rc_for_nnl(atoms, target)
    nn = make_nn(ELEMENTS[nspec], rc, True, [16], sf_kwargs=dict(eta=[0.05, 4.0]))
    run_rows(nn, [atoms], (target, target), f"nnl{target}")


@gpu
@pytest.mark.parametrize("nspec", [1, 2, 3])
@pytest.mark.parametrize("cap", [192, 256])
def test_multi_chunk_mixed_classes(lib, nspec, cap):
    """beta (0.005, 3, 10) x gamma (1, -1, 0.5) x zeta (1, 4, 2): H12, H24 and exact launches in one model,
    full and partial (ng, nz) chunks (keys x22, x21, x12, x11), `first` = 1 then 0 in the backward chain."""
    rc, lo, hi = CAPS[cap]
    nn = make_nn(ELEMENTS[nspec], rc, True, [16, 16], sf_kwargs=dict(eta=[0.05, 4.0], **MULTI), minmax=True)
    frames = [alloy(ELEMENTS[nspec], seed=31)]
    if cap == 192:
        frames.append(alloy(ELEMENTS[nspec], rep=(3, 2, 2), seed=32))
    run_rows(nn, frames, (lo, hi), f"multi-{nspec}el-cap{cap}")


@gpu
@pytest.mark.parametrize("nspec", [2, 3, 5])
def test_absent_species_and_sparse_centres(lib, nspec):
    """Frames where a species is missing (empty segments) and where most centres have 0 or 1 neighbour
    (16 centres per workgroup), in one uneven batch."""
    els = ELEMENTS[nspec]
    nn = make_nn(els, 5.0, True, [16], sf_kwargs=dict(eta=[0.05, 4.0]))
    frames = [alloy(els[:-1] if nspec > 2 else els[:1], seed=41), sparse_cluster(els),
              alloy(els, rep=(2, 2, 3), seed=42), sparse_cluster(els[1:], seed=6)]
    run_rows(nn, frames, (1, 192), f"sparse-{nspec}el")
    nn = make_nn(els, 5.0, True, [16], sf_kwargs=dict(eta=[0.05], beta=[3.0], zeta=[1.0, 2.0]))
    run_rows(nn, frames, (1, 192), f"sparse-{nspec}el-h24")


# -- switches read at ta_create, held by the handle ---------------------------------------------------------

def switch_cases():
    """(name, model, frames): one- and two-element default-grid models at cap 192 and at cap 256, and the
    one-gamma grid at cap 192 (keys 112 / 212 of the kCapMin builds)."""
    out = []
    for nspec in (1, 2):
        els = ELEMENTS[nspec]
        out.append((f"{nspec}el-cap192", make_nn(els, 6.0, True, [16, 16]),
                    [alloy(els, rep=(3, 3, 3)), alloy(els, a=3.4, seed=4)]))
        out.append((f"{nspec}el-ng1-cap192", make_nn(els, 5.0, True, [16], sf_kwargs=dict(gamma=[1.0])),
                    [alloy(els, seed=6)]))
        out.append((f"{nspec}el-cap256", make_nn(els, 8.6, True, [16], sf_kwargs=dict(eta=[0.05, 4.0])),
                    [alloy(els, seed=5)]))
    return out


@gpu
@pytest.mark.parametrize("var,value", [("TA_NO_JOBS", "1"), ("TA_FWD_WPE", "5"), ("TA_BWD_WPE", "6"),
                                       ("TA_FULL_RECORDS", "1")])
def test_switches_set_before_the_engine(lib, monkeypatch, var, value):
    """TA_NO_JOBS (per-lane masks, lanes re-dealt by popcount), TA_FWD_WPE=5 / TA_BWD_WPE=6 (the other kCapMin
    builds), TA_FULL_RECORDS (64-byte pair records): the library reads each in ta_create and keeps it with the
    handle, so each is in the environment only while its engine is made."""
    from tensoralloy_amd import Engine
    for name, nn, frames in switch_cases():
        monkeypatch.setenv(var, value)
        eng = Engine(nn)
        monkeypatch.delenv(var)
        with eng:
            res = eng.evaluate(frames, descriptors=True)
            nnl = int(eng.info.nnl_max)
        assert (nnl <= 192) == name.endswith("cap192") and nnl <= 256, (name, nnl)
        for k, (atoms, r) in enumerate(zip(frames, res)):
            check(r, c_oracle(nn, atoms), f"{var}={value}/{name}/frame{k}")


@gpu
def test_switches_belong_to_the_handle(lib, monkeypatch):
    """Two engines of one model side by side: A made under TA_MLP_QUAD_KERNEL, TA_HOST_NL and TA_NO_JOBS, B
    after all three were deleted. Each keeps what it was made with, call after call, and a switch set once
    both exist (TA_MLP_TILE_KERNEL) reaches neither."""
    from tensoralloy_amd import Engine
    nn = make_nn(ELEMENTS[1], 5.0, True, [16, 16])
    atoms = alloy(ELEMENTS[1])
    frames = [atoms]
    o = c_oracle(nn, atoms)
    made_with = {"TA_MLP_QUAD_KERNEL": "1", "TA_HOST_NL": "1", "TA_NO_JOBS": "1"}
    for var, value in made_with.items():
        monkeypatch.setenv(var, value)
    a = Engine(nn)
    for var in made_with:
        monkeypatch.delenv(var)
    b = Engine(nn)
    monkeypatch.setenv("TA_MLP_TILE_KERNEL", "1")
    expect = {"A": ("quad", mirror_launch(nn, frames, "TA_MLP_QUAD_KERNEL"), 0),
              "B": ("tile", mirror_launch(nn, frames, None), 1)}
    with a, b:
        for k, (tag, eng) in enumerate([("A", a), ("B", b), ("A", a)]):
            r = eng.evaluate(frames, descriptors=True)[0]
            family, launch, on_device = expect[tag]
            assert int(eng.info.nnl_max) <= 192
            assert eng.mlp_launch()["family"] == family and eng.mlp_launch() == launch, (tag, eng.mlp_launch())
            assert int(eng.info.nl_on_device) == on_device, tag
            check(r, o, f"handle-{tag}/call{k}")


# -- MD path: the exact list filtered on the device from the resident skin list ------------------------------

@gpu
@pytest.mark.parametrize("nspec,rc", [(2, 6.0), (3, 5.5), (5, 5.0), (2, 8.6)], ids=["2el", "3el", "5el", "2el-cap256"])
def test_md_skin_list_against_the_oracle(lib, nspec, rc):
    """ta_update_positions + compute and ta_step on an uneven 3-frame batch with a Verlet skin: list reuses
    and rebuilds, every step against the oracle at the new positions."""
    from tensoralloy_amd import Engine, _lib
    els = ELEMENTS[nspec]
    want = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES | _lib.TA_WANT_VIRIAL | _lib.TA_WANT_ATOMIC
    kw = dict(eta=[0.05, 4.0]) if rc > 8 else None
    nn = make_nn(els, rc, True, [16, 16], sf_kwargs=kw)
    # 45 + 62 + 69 atoms: groups of 16 centres straddle the frame boundaries
    frames = [drop(alloy(els, rep=(3, 2, 2), seed=51), 3), drop(alloy(els, rep=(2, 2, 4), a=3.55, seed=52), 2),
              drop(alloy(els, rep=(3, 3, 2), seed=53), 3)]
    sizes = np.cumsum([0] + [len(a) for a in frames])
    rng = np.random.RandomState(nspec)
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        eng.set_frames(frames)
        pos = np.concatenate([a.positions for a in frames])
        for step in range(6):
            # small steps keep the list; every third step moves far enough to force a rebuild
            pos = pos + rng.normal(0, 0.2 if step % 3 == 2 else 0.02, pos.shape)
            if step % 2:
                got = eng.step(pos, want)
                got = {k: np.array(v) for k, v in got.items()}
            else:
                eng.update_positions(pos)
                eng.compute(want)
                got = eng.fetch(want)
            nnl = int(eng.info.nnl_max)
            assert (nnl > 192) == (rc > 8), nnl
            for f, atoms in enumerate(frames):
                moved = Atoms(symbols=atoms.get_chemical_symbols(), positions=pos[sizes[f]:sizes[f + 1]],
                              cell=np.asarray(atoms.get_cell()), pbc=True)
                r = dict(energy=got["energy"][f], atomic=got["atomic"][sizes[f]:sizes[f + 1]],
                         forces=got["forces"][sizes[f]:sizes[f + 1]], virial=got["virial"][f])
                check(r, c_oracle(nn, moved), f"md-{nspec}el-rc{rc}/step{step}/frame{f}", descriptors=False)
        builds, reuses = eng.list_stats()
        assert builds + reuses == 7 and builds >= 2 and reuses >= 2, (builds, reuses)
