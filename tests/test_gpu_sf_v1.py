"""
The first-generation angular kernels (ta_kernels.hip) build by build and caller by caller, against the C oracle.

They serve every symmetry-function model the second-generation dispatcher turns away: six to eight elements,
four or five elements with a (gamma, zeta) grid other than 2 x 2, more than 1024 neighbours per atom, and
TA_FORCE_V1. The host cuts the (beta, gamma, zeta) grid into chunks of at most 2 x 2 x 2 channels
(`chunk_plan` below restates it); every chunk is one `g4_forward_kernel<NB, NG, NZ>` and one
`backward_kernel<NB, NG, NZ>` launch, the first of the backward chain with `first` = 1 (it writes g and adds the
radial part), the later ones with `first` = 0 (they add onto g). `test_rows_cover_every_build` shows on the CPU
that the rows below reach each of the eight builds as chunk 0 and as a later chunk.

Bounds: `check()` of test_gpu_sf_dispatch.py, unchanged (north_star, descriptors 1e-10, E and e 1e-9, F 1e-9,
W 1e-8 relative). Proof of path: after its evaluation every angular row asserts that no run packing exists
(`n_blk` == 0) and that no second-generation backward build ran (`backward_variant()` == 0), which is what the
dispatcher leaves when it chose these kernels; `test_control_second_generation` shows both are non-zero otherwise.

Also here: these kernels on a Verlet skin list (they run on the padded list itself and rely on every u < 1 test),
inside the device MD loop, radial-only models of several elements (`g2_backward_kernel`), and the width limit
of the per-atom network behind wide descriptors. The training entry points on these kernels:
test_gpu_train_scale.py (rows `v1-*`).
"""
import numpy as np
import pytest

from tests.helpers import TILE_ROWS, make_nn, mirror_launch, mlp_stride, net_of, oracle_eval
from tests.test_gpu_nlist_layout import EL8
from tests.test_gpu_sf_dispatch import (CAPS, E_REL, E_TOL, ELEMENTS, G_TOL, MULTI, alloy, c_oracle, check, drop,
                                        sparse_cluster)
from tensoralloy_amd import Atoms

gpu = pytest.mark.gpu

E2, E3, E4 = ELEMENTS[2], ELEMENTS[3], ELEMENTS[4]
E6 = ["Al", "Co", "Cu", "Fe", "Mo", "Ni"]
KEYS = [111, 112, 121, 122, 211, 212, 221, 222]     # TA_DISPATCH (ta_kernels.hip)
ETA2 = dict(eta=[0.05, 4.0])
LDS_LIMIT = 160 * 1024          # LDS one workgroup may ask for on gfx950
MAX_WIDTH = 512                 # widest layer input or output `build_net` (ta_api.hip) accepts


def chunk_plan(beta, gamma, zeta):
    """The chunk planner of the first-generation path (ta_api.hip, pass 0) restated: betas, gammas and zetas in
    steps of two, in this loop order; key = nb * 100 + ng * 10 + nz; `first` for chunk 0 only."""
    out = []
    for b0 in range(0, len(beta), 2):
        for g0 in range(0, len(gamma), 2):
            for z0 in range(0, len(zeta), 2):
                b, g, z = beta[b0:b0 + 2], gamma[g0:g0 + 2], zeta[z0:z0 + 2]
                out.append(dict(key=len(b) * 100 + len(g) * 10 + len(z), first=not out, beta=list(b), gamma=list(g),
                                zeta=list(z)))
    return out


def grid_a(key):
    nb, ng, nz = key // 100, key // 10 % 10, key % 10
    return dict(eta=[0.05, 4.0, 20.0], beta=[0.005, 3.0][:nb], gamma=[1.0, -1.0][:ng],
                zeta=[1.0, 4.0] if nz == 2 else [2.0])


def _models():
    """name -> (builder, TA_FORCE_V1 needed, elements). rc 5.0 and hidden [16] unless the row is about them."""
    m = {}
    for key in KEYS:   # a. one chunk of every build, `first` = 1
        m[f"a-{key}"] = (lambda key=key: make_nn(E2, 5.0, True, [16], sf_kwargs=grid_a(key), seed=key), True, 2)
    # b. 3 x 3 x 3: chunks 222, 221, 212, 211, 122, 121, 112, 111, chosen by the dispatcher (4 elements, not 2 x 2)
    m["b-multi-4el"] = (lambda: make_nn(E4, 5.0, True, [16, 16], sf_kwargs=dict(**ETA2, **MULTI), minmax=True), False, 4)
    # c. two chunks of key 222
    m["c-222-twice"] = (lambda: make_nn(E2, 5.0, True, [16], sf_kwargs=dict(
        **ETA2, beta=[0.005, 3.0], gamma=[1.0, -1.0], zeta=[1.0, 4.0, 2.0, 16.0])), True, 2)
    # d. 193-256 neighbours: a workgroup of 256 pairs starts and ends inside centres, 256 + 2 nnl records staged
    m["d-staging-cap256"] = (lambda: make_nn(E2, CAPS[256][0], True, [16, 16], sf_kwargs=dict(**ETA2, **MULTI),
                                             minmax=True), True, 2)
    # e. six and eight (kMaxElements) elements, default angular grid
    m["e-6el"] = (lambda: make_nn(E6, 5.0, True, [16], sf_kwargs=ETA2), False, 6)
    m["e-8el"] = (lambda: make_nn(EL8, 5.0, True, [16], sf_kwargs=ETA2), False, 8)
    # f. variants, six elements through the dispatcher
    m["f-poly-acut4"] = (lambda: make_nn(E6, 5.0, True, [16], cutoff="polynomial", acut=4.0, sf_kwargs=ETA2), False, 6)
    m["f-acut6"] = (lambda: make_nn(E6, 5.0, True, [16], acut=6.0, sf_kwargs=ETA2), False, 6)
    m["f-medium"] = (lambda: make_nn(E6, 5.0, True, [16], sf_kwargs=ETA2, precision="medium"), False, 6)
    m["f-zeta-1.5-4"] = (lambda: make_nn(E6, 5.0, True, [16], sf_kwargs=dict(**ETA2, zeta=[1.5, 4.0])), False, 6)
    m["f-zeta-2.5"] = (lambda: make_nn(E6, 5.0, True, [16], sf_kwargs=dict(**ETA2, zeta=[2.5])), False, 6)
    # ... and at rc 6.5, where the cosine of a pair with itself rounds above 1 (test_self_pair_cosine_above_one)
    m["f-zeta-1.5-4-rc6.5"] = (lambda: make_nn(E6, 6.5, True, [16], sf_kwargs=dict(**ETA2, zeta=[1.5, 4.0])), False, 6)
    # (two hidden layers: a skip connection needs a hidden layer l > 0 of equal width)
    m["f-resnet-tanh"] = (lambda: make_nn(E6, 5.0, True, [16, 16], activation="tanh", resnet=True, sf_kwargs=ETA2),
                          False, 6)
    # 5b. the widest descriptor `build_net` accepts from this grid: MULTI without its third gamma, D = 390
    m["wide-6el"] = (lambda: make_nn(E6, 5.0, True, [16, 16], sf_kwargs=dict(
        **ETA2, beta=MULTI["beta"], gamma=MULTI["gamma"][:2], zeta=MULTI["zeta"]), minmax=True), False, 6)
    return m


MODELS = _models()


def grid_of(nn):
    d = nn.descriptor.as_dict()
    return [float(x) for x in d["beta"]], [float(x) for x in d["gamma"]], [float(x) for x in d["zeta"]]


def dispatcher_takes_v2(nn):
    """`use_v2` of ta_set_frames restated for at most 1024 neighbours and no TA_FORCE_V1."""
    n, (_, gamma, zeta) = len(nn.elements), grid_of(nn)
    return n <= 3 or (n <= 5 and len(gamma) % 2 == 0 and len(zeta) % 2 == 0)


def test_rows_cover_every_build():
    """CPU: the rows reach all eight builds as chunk 0 and as a later chunk, a non-integer zeta in a chunk of
    each nz, the element counts they claim, and none of the rows left to the dispatcher is a second-generation
    shape."""
    as_first, as_later, non_integer_nz = set(), set(), set()
    for name, (build, forced, n_el) in MODELS.items():
        nn = build()
        assert len(nn.elements) == n_el, name
        assert forced == dispatcher_takes_v2(nn), name
        plan = chunk_plan(*grid_of(nn))
        assert [c["first"] for c in plan] == [True] + [False] * (len(plan) - 1)
        for c in plan:
            (as_first if c["first"] else as_later).add(c["key"])
            if any(z != round(z) for z in c["zeta"]):
                non_integer_nz.add(c["key"] % 10)
    assert as_first == set(KEYS) and as_later == set(KEYS), (sorted(as_first), sorted(as_later))
    assert non_integer_nz == {1, 2}
    assert [c["key"] for c in chunk_plan(*grid_of(MODELS["b-multi-4el"][0]()))] == [222, 221, 212, 211, 122, 121, 112, 111]
    assert [c["key"] for c in chunk_plan(*grid_of(MODELS["c-222-twice"][0]()))] == [222, 222]
    assert [c["key"] for c in chunk_plan(*grid_of(MODELS["e-8el"][0]()))] == [122]
    for key in KEYS:
        assert [c["key"] for c in chunk_plan(*grid_of(MODELS[f"a-{key}"][0]()))] == [key]
    assert MODELS["b-multi-4el"][0]().ndim() == 278
    assert {n for _, _, n in MODELS.values()} == {2, 4, 6, 8}


def self_pair_bases(atoms, rc, eps=1e-14):
    """1 - cos(theta) of every pair taken with itself, in the arithmetic of `g4_forward_kernel`: r^2 = D.D + eps,
    1 / r, d^2 = eps, cos = (r^2 + r^2 - d^2) * 0.5 * (1 / r) * (1 / r)."""
    from oracle.neighbors import neighbor_list
    R, h = atoms.positions, np.asarray(atoms.get_cell(complete=True))
    i, j, S = neighbor_list(R, h, atoms.pbc, rc)
    D = R[j] - R[i] + S @ h
    r2 = D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1] + D[:, 2] * D[:, 2] + eps
    inv = 1.0 / np.sqrt(r2)
    return 1.0 - (r2 + r2 - eps) * 0.5 * inv * inv


def test_self_pair_cosine_above_one():
    """CPU: why row f-zeta-1.5-4-rc6.5 exists. A lane of the forward kernel walks every neighbour of its centre,
    its own pair included, and masks that term. Its cosine is 1 - eps / (2 r^2): for r^2 above about 25 that is
    less than an ulp below 1, and with the rounding of 1 / r it lands above 1 for some pairs, so 1 + gamma cos is
    negative for gamma = -1 and pow(base, 1.5) is NaN. A term masked by multiplication (NaN * 0) poisons the sum;
    it has to be masked by selection. The frame of the row has such pairs at rc 6.5 and none at rc 5.0."""
    frame = alloy(E6, seed=61)
    assert (self_pair_bases(frame, 6.5) < 0.0).sum() >= 2
    assert (self_pair_bases(frame, 5.0) < 0.0).sum() == 0


def nnl_of(frames, r):
    from oracle.neighbors import neighbor_list
    return max(int(np.bincount(neighbor_list(a.positions, np.asarray(a.get_cell(complete=True)), a.pbc, r)[0],
                               minlength=1).max()) for a in frames)


# -- GPU ------------------------------------------------------------------------------------------------------

def engine(nn, monkeypatch, forced):
    """TA_FORCE_V1 is read in ta_create and kept by the handle: in the environment only while the engine is made."""
    from tensoralloy_amd import Engine
    if forced:
        monkeypatch.setenv("TA_FORCE_V1", "1")
    try:
        return Engine(nn)
    finally:
        if forced:
            monkeypatch.delenv("TA_FORCE_V1")


def assert_v1(eng, tag):
    info = eng.list_layout("kernel")["info"]
    assert info["n_blk"] == 0 and not info["filtered"] and eng.backward_variant() == 0, (tag, info)


def run_v1(monkeypatch, name, frames, window=(1, 192), oracle=c_oracle):
    build, forced, _ = MODELS[name]
    nn = build()
    with engine(nn, monkeypatch, forced) as eng:
        res = eng.evaluate(frames, descriptors=True)
        nnl = int(eng.info.nnl_max)
        assert_v1(eng, name)
        launch = eng.mlp_launch()
    assert window[0] <= nnl <= window[1], (name, nnl, window)
    for k, (atoms, r) in enumerate(zip(frames, res)):
        check(r, oracle(nn, atoms), f"{name}/frame{k}")
    return nn, launch


def uneven(els, seed, a=3.6):
    """32 + 43 atoms."""
    return [alloy(els, a=a, seed=seed), drop(alloy(els, rep=(3, 2, 2), a=a, seed=seed + 1), 5)]


def edge_frames(els, seed=41):
    """An alloy without the last element, isolated atoms and centres with 0 or 1 neighbour (`pair_i` skips
    centres, the last workgroup is partial), a 48-atom alloy, a sparse frame without the first element."""
    return [alloy(els[:-1], seed=seed), sparse_cluster(els), alloy(els, rep=(2, 2, 3), seed=seed + 1),
            sparse_cluster(els[1:], seed=6)]


@gpu
def test_control_second_generation(lib):
    """The proof of path is not vacuous: a one-element default-grid model leaves run packing and a
    second-generation backward build behind."""
    from tensoralloy_amd import Engine
    nn = make_nn(["Ni"], 5.0, True, [16], sf_kwargs=ETA2)
    frame = alloy(["Ni"])
    with Engine(nn) as eng:
        r = eng.evaluate([frame], descriptors=True)[0]
        assert eng.list_layout("kernel")["info"]["n_blk"] > 0 and eng.backward_variant() != 0
    check(r, c_oracle(nn, frame), "control")


@gpu
@pytest.mark.parametrize("key", KEYS)
def test_single_chunk_of_every_build(lib, monkeypatch, key):
    run_v1(monkeypatch, f"a-{key}", [alloy(E2, seed=10 + key % 7)])


@gpu
def test_multi_chunk_through_the_dispatcher(lib, monkeypatch):
    """Eight chunks, one of every build, `first` = 1 then 0 seven times; `chan[]` is the identity in none of them."""
    run_v1(monkeypatch, "b-multi-4el", uneven(E4, 21))


@gpu
def test_later_chunk_of_key_222(lib, monkeypatch):
    run_v1(monkeypatch, "c-222-twice", [alloy(E2, seed=23)])


@gpu
def test_staging_windows(lib, monkeypatch):
    _, lo, hi = CAPS[256]
    run_v1(monkeypatch, "d-staging-cap256", [alloy(E2, seed=24)], window=(lo, hi))


@gpu
@pytest.mark.parametrize("name", ["e-6el", "e-8el"])
def test_element_count_edges(lib, monkeypatch, name):
    run_v1(monkeypatch, name, edge_frames(MODELS[name][0]().elements))


@gpu
def test_first_and_last_element_absent(lib, monkeypatch):
    """Eight elements, two of them nowhere in the batch: empty `elem_start` ranges and segments, no network tile."""
    els = EL8[1:-1]
    run_v1(monkeypatch, "e-8el", [alloy(els, seed=43), sparse_cluster(els), drop(alloy(els, rep=(3, 2, 2), seed=44), 5)])


@gpu
@pytest.mark.parametrize("name", ["f-poly-acut4", "f-acut6", "f-zeta-1.5-4", "f-zeta-2.5", "f-zeta-1.5-4-rc6.5",
                                  "f-resnet-tanh"])
def test_variants(lib, monkeypatch, name):
    """acut < rc with the polynomial cutoff; acut > rc (the list is built at acut, G2 must vanish beyond rc);
    non-integer zetas (`safe_pow_value` / `safe_pow_grad`) in a chunk of two zetas and of one; skip connections."""
    run_v1(monkeypatch, name, uneven(E6, 61))


@gpu
def test_medium_precision(lib, monkeypatch):
    """eps = 1e-8 under every root. Reference: the Python oracle, which takes eps; the C oracle has 1e-14 built in
    and differs from it by 2e-8 eV on a medium model (the two agree to 1e-15 otherwise)."""
    run_v1(monkeypatch, "f-medium", uneven(E6, 61), oracle=oracle_eval)


@gpu
def test_collinear_non_integer_zeta(lib, monkeypatch):
    """The geometry and tolerances of test_gpu_sf.py::test_safe_pow_edge_non_integer_zeta on these kernels."""
    pos = np.array([[0.0, 0.0, 0.0], [1.3, 0.0, 0.0], [2.9, 0.0, 0.0], [0.4, 1.7, 0.3]])
    atoms = Atoms(symbols=["Ni"] * 4, positions=pos + 10.0, cell=np.eye(3) * 30.0, pbc=False)
    got = {}
    for custom in (False, True):
        for zeta in ([0.5, 1.5], [1.0, 2.5]):
            nn = make_nn(["Ni"], 4.0, True, [8], sf_kwargs=dict(eta=[0.5], zeta=zeta, gamma=[1.0, -1.0]))
            nn.use_custom_pow = custom
            with engine(nn, monkeypatch, True) as eng:
                r = eng.evaluate([atoms])[0]
                assert_v1(eng, (custom, zeta))
            o = oracle_eval(nn, atoms)
            assert np.isfinite(r["energy"]) and np.all(np.isfinite(r["forces"])) and np.all(np.isfinite(o["forces"]))
            assert abs(r["energy"] - o["energy"]) < E_TOL
            scale = max(1.0, np.abs(o["forces"]).max())
            assert np.abs(r["forces"] - o["forces"]).max() < (0.05 * scale if min(zeta) < 1.0 else 1e-5)
            got[(custom, tuple(zeta))] = r
    for zeta in ((0.5, 1.5), (1.0, 2.5)):
        a, b = got[(False, zeta)], got[(True, zeta)]
        assert a["energy"] == b["energy"] and np.array_equal(a["forces"], b["forces"])


@gpu
@pytest.mark.parametrize("els", [E2, E3, E6], ids=["2el", "3el", "6el"])
def test_radial_only_several_elements(lib, els):
    """`g2_backward_kernel` with `radial_term()` of unlike species; one frame lacks the last element. (No angular
    launch: the proof of path does not apply.)"""
    from tensoralloy_amd import Engine
    nn = make_nn(els, 5.0, False, [16], sf_kwargs=dict(eta=[0.05, 4.0, 20.0], omega=[0.0, 1.5]))
    frames = [alloy(els, seed=71), drop(alloy(els[:-1], rep=(3, 2, 2), seed=72), 5)]
    with Engine(nn) as eng:
        res = eng.evaluate(frames, descriptors=True)
    for k, (atoms, r) in enumerate(zip(frames, res)):
        check(r, c_oracle(nn, atoms), f"g2-{len(els)}el/frame{k}")


@gpu
def test_energy_only_then_full(lib, monkeypatch):
    """ENERGY | ATOMIC: no backward launch, descriptors through `descriptor_reduce_kernel`; then a full
    evaluation of other frames on the same engine, where a stale g or part4 would show."""
    from tensoralloy_amd import _lib
    nn = MODELS["e-6el"][0]()
    first, second = uneven(E6, 81), [alloy(E6, rep=(3, 2, 2), seed=83), alloy(E6, seed=84)]
    with engine(nn, monkeypatch, False) as eng:
        res = eng.evaluate(first, want=_lib.TA_WANT_ENERGY | _lib.TA_WANT_ATOMIC, descriptors=True)
        assert_v1(eng, "energy-only")
        full = eng.evaluate(second, descriptors=True)
        assert_v1(eng, "full")
    for k, (atoms, r) in enumerate(zip(first, res)):
        o = c_oracle(nn, atoms)
        assert "forces" not in r
        dev = (abs(r["energy"] - o["energy"]), np.abs(r["atomic"] - o["atomic"]).max(),
               np.abs(r["descriptors"] - o["descriptors"]).max())
        print(f"DEV energy-only/frame{k} E={dev[0]:.2e} e={dev[1]:.2e} G={dev[2]:.2e}")
        assert dev[0] < E_REL * max(1.0, abs(o["energy"])) and dev[1] < E_REL * max(1.0, abs(o["energy"])), dev
        assert dev[2] < G_TOL, dev
    for k, (atoms, r) in enumerate(zip(second, full)):
        check(r, c_oracle(nn, atoms), f"after-energy-only/frame{k}")


# -- on the skin list -------------------------------------------------------------------------------------------

SKIN = 0.5


@pytest.mark.parametrize("name,seed", [("b-multi-4el", 21), ("e-6el", 91)])
def test_skin_list_holds_padded_pairs(name, seed):
    """CPU: the frames of the skin test have more neighbours at rc + skin than at rc."""
    nn = MODELS[name][0]()
    frames = uneven(nn.elements, seed)
    assert nnl_of(frames, 5.0 + SKIN) > nnl_of(frames, 5.0)


@gpu
@pytest.mark.parametrize("name,seed", [("b-multi-4el", 21), ("e-6el", 91)])
def test_skin_list(lib, monkeypatch, name, seed):
    """These kernels get no exact list: under a skin they run on the padded list. Three small moves, one atom
    moved beyond skin / 2, one change of the cells; ta_update_positions + compute, ta_step and ta_step_view in
    turn, each state against the oracle."""
    from tensoralloy_amd import _lib
    want = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES | _lib.TA_WANT_VIRIAL | _lib.TA_WANT_ATOMIC
    nn = MODELS[name][0]()
    frames = uneven(nn.elements, seed)
    sizes = np.cumsum([0] + [len(a) for a in frames])
    exact, padded = nnl_of(frames, 5.0), nnl_of(frames, 5.0 + SKIN)
    rng = np.random.RandomState(seed)
    pos = np.concatenate([a.positions for a in frames])
    cells = np.array([np.asarray(a.get_cell(complete=True)) for a in frames])
    with engine(nn, monkeypatch, False) as eng:
        eng.set_skin(SKIN)
        eng.set_frames(frames)
        assert int(eng.info.nnl_max) == padded > exact, (int(eng.info.nnl_max), padded, exact)
        for move in range(5):
            new_cells = None
            if move < 3:
                pos = pos + rng.normal(0, 0.02, pos.shape)
            elif move == 3:
                pos = pos.copy()
                pos[7] += [0.3, 0.0, 0.0]            # one atom beyond skin / 2
            else:
                cells = cells * 1.004
                pos = pos * 1.004
                new_cells = cells
            descriptors = None
            if move % 3 == 0:
                eng.update_positions(pos, new_cells)
                eng.compute(want)
                got = eng.fetch(want, descriptors=True)
                descriptors = got["descriptors"]
            else:
                got = eng.step(pos, want, cells=new_cells, view=(move % 3 == 2))
                got = {k: np.array(v) for k, v in got.items()}
            assert_v1(eng, (name, move))
            for f, atoms in enumerate(frames):
                moved = Atoms(symbols=atoms.get_chemical_symbols(), positions=pos[sizes[f]:sizes[f + 1]],
                              cell=cells[f], pbc=True)
                r = dict(energy=got["energy"][f], atomic=got["atomic"][sizes[f]:sizes[f + 1]],
                         forces=got["forces"][sizes[f]:sizes[f + 1]], virial=got["virial"][f])
                if descriptors is not None:
                    r["descriptors"] = descriptors[sizes[f]:sizes[f + 1]]
                check(r, c_oracle(nn, moved), f"skin-{name}/move{move}/frame{f}", descriptors=descriptors is not None)
        builds, reuses = eng.list_stats()
        assert builds + reuses == 6 and builds >= 2 and reuses >= 2, (builds, reuses)


# -- inside the device MD loop ----------------------------------------------------------------------------------

@gpu
def test_device_md_loop(lib, monkeypatch):
    """`ta_md_run`, 12 NVE steps of 1 fs from 300 K on the skin list, against tests/md_reference.py driven by a
    second engine with an exact list at every step (the pattern and the bound of
    test_gpu_md.py::test_model_families)."""
    from tests import md_reference
    from tests.test_gpu_md import DT, WANT, _assert_parity, _masses, _velocities
    nn = MODELS["e-6el"][0]()
    frames = [alloy(E6, seed=95, jitter=0.02)]
    v0 = _velocities(frames, 300.0, 5)
    with engine(nn, monkeypatch, False) as other:
        other.set_skin(0.0)
        other.set_frames(frames)

        def force(x):
            r = other.step(x, WANT)
            return r["energy"].copy(), r["forces"].copy()
        ref = md_reference.run(force, frames[0].positions, v0, _masses(frames), DT, 12, skin=SKIN)
        assert_v1(other, "md reference")
    with engine(nn, monkeypatch, False) as eng:
        eng.set_skin(SKIN)
        eng.set_frames(frames)
        eng.md_init(None, v0)
        out = eng.md_run(12, DT)
        x, v = eng.md_state()
        assert_v1(eng, "md loop")
    dev = dict(x=x, v=v, epot=out["epot"], ekin=out["ekin"], n_rebuilds=out["n_rebuilds"])
    assert dev["epot"].shape == (13, 1)
    assert dev["n_rebuilds"] == ref["n_rebuilds"]
    _assert_parity(dev, ref)


# -- wide descriptors into the per-atom network tile ------------------------------------------------------------

def tile_lds_bytes(width):
    """Dynamic LDS of the generic tile behind a descriptor of `width`: 2 x 16 x (padded width + 2) doubles."""
    return 2 * TILE_ROWS * ((width + 15) // 16 * 16 + 2) * 8


def test_tile_width_limit():
    """CPU: many elements mean wide descriptors, and the generic tile's LDS grows with the padded descriptor
    length. The library bounds it where the model is made: `build_net` refuses a layer wider than 512, so the
    tile asks for at most 131,584 B, below the 160 KB a gfx950 workgroup may have (the tile kernels have no static
    LDS: `group_segment_fixed_size` 0 in the metadata of all four builds). The eight-element 3 x 3 x 3 model
    (D = 988) would need 254,464 B and the six-element one (D = 579) 152,064 B; both stop at the width limit."""
    wide = MODELS["wide-6el"][0]()
    assert wide.ndim() == 390 and tile_lds_bytes(390) == 102912
    assert 2 * TILE_ROWS * max(mlp_stride(net_of(wide, el)) for el in wide.elements) * 8 == 102912
    assert tile_lds_bytes(MAX_WIDTH) == 131584 <= LDS_LIMIT
    six = make_nn(E6, 5.0, True, [16, 16], sf_kwargs=dict(**ETA2, **MULTI))
    eight = make_nn(EL8, 5.0, True, [16, 16], sf_kwargs=dict(**ETA2, **MULTI))
    assert (six.ndim(), eight.ndim()) == (579, 988)
    assert 2 * TILE_ROWS * mlp_stride(net_of(six, "Ni")) * 8 == tile_lds_bytes(579) == 152064
    assert 2 * TILE_ROWS * mlp_stride(net_of(eight, "Ni")) * 8 == tile_lds_bytes(988) == 254464 > LDS_LIMIT
    assert min(six.ndim(), eight.ndim()) > MAX_WIDTH


@gpu
def test_wide_descriptor_accepted(lib, monkeypatch):
    """Six elements, beta 3 x gamma 2 x zeta 3: D = 390, row stride 402, 102,912 B of dynamic LDS (static: 0) in
    `mlp_all_kernel<256>`, act' in the global slab. The widest descriptor any test evaluates."""
    frames = uneven(E6, 61)
    nn, launch = run_v1(monkeypatch, "wide-6el", frames)
    assert launch == mirror_launch(nn, frames), launch
    assert (launch["family"], launch["da"], launch["lds_bytes"], launch["threads"]) == ("tile_all", "global", 102912, 256)


@gpu
def test_too_wide_descriptor_refused_then_a_valid_model(lib, monkeypatch):
    """Eight elements with the 3 x 3 x 3 grid (D = 988; 254,464 B in the tile) and six (D = 579): refused when
    the engine is made, with a ValueError that names the limit; nothing reaches the device. The process then
    evaluates the eight-element default-grid model correctly."""
    from tensoralloy_amd import Engine
    for els in (EL8, E6):
        nn = make_nn(els, 5.0, True, [16, 16], sf_kwargs=dict(**ETA2, **MULTI))
        with pytest.raises(ValueError, match=r"MLP layer width out of range \(1\.\.512\)"):
            Engine(nn)
    run_v1(monkeypatch, "e-8el", edge_frames(EL8))
