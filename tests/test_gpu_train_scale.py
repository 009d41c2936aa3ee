"""GPU: the training-gradient kernels (csrc/ta_train.hip, ta_td_train.hip, ta_hvp.hip) at the shapes toy tests
never reach, against float64 references that do not share code with them.

* More than 1024 tiles of 16 rows: the gradient kernels run at most `kMaxBlocks` = 1024 persistent workgroups,
  so only then does a workgroup take a second tile (cross-tile accumulation, reuse of its scratch) and
  `grad_reduce_kernel` add a full set of partial slices. SF models from 16,385 atoms of one element on, nn-EAM
  networks from 16,385 pair rows on.
* Dynamic LDS above 64 KB: `mlp_grad2_kernel` asks for 4 x 16 x stride doubles (stride = widest padded layer + 2),
  above 64 KB from width 128 on; `mlp_grad_kernel` and the generic forward tile ask for 2 x 16 x stride, above
  64 KB from width 256 on. A network too wide for one workgroup is refused with a ValueError.
* Every activation through the second-order pass (a''), an element absent from the batch, the descriptor
  Jacobian of `ta_loss_gradient` across the angular dispatch, and Hessian-vector products of a wide model and of
  a batch above 1024 tiles.

MLP gradients are held to 1e-9 x max(1, |ref|) against oracle/train.py (checked by finite differences in
tests/test_train_cpu.py) on the GPU's own descriptors G and tangents dG; G itself is pinned to the oracle on a
small frame of every model, dG by sixth-order central differences of the GPU's descriptors (part D)."""
import numpy as np
import pytest

from tensoralloy_amd import Atoms, Engine, _lib
from tests.helpers import (fcc, make_eam, make_grap_nn, make_nn, oracle_eam_eval, oracle_eval, oracle_grap_eval,
                           oracle_grap_model, oracle_model)

pytestmark = pytest.mark.gpu

ROWS = 16              # rows of one tile (kMlpRows)
MAX_BLOCKS = 1024      # persistent workgroups of the gradient kernels (kMaxBlocks)
LDS_64K = 64 * 1024
RC = 4.75              # between the 4th and 5th fcc shells of Ni (a = 3.524): no pair sits near the cutoff


def _stride(nn):
    """Row stride of the gradient tiles (ta_mlp_tile.h::mlp_stride): widest padded layer + 2."""
    widths = [nn.ndim()] + [w for h in nn.hidden_sizes.values() for w in h] + [1]
    return max(-(-w // 16) * 16 for w in widths) + 2


def lds_bytes(nn, slabs):
    """Dynamic LDS of one launch: 2 slabs (mlp_grad_kernel, generic forward tile) or 4 (mlp_grad2_kernel)."""
    return slabs * ROWS * _stride(nn) * 8


def tiles(frames, element):
    n = sum(s == element for a in frames for s in a.get_chemical_symbols())
    return -(-n // ROWS), n


def _relabel(atoms, picks, symbol):
    syms = atoms.get_chemical_symbols()
    for k in picks:
        syms[k] = symbol
    return Atoms(symbols=syms, positions=atoms.positions, cell=np.asarray(atoms.get_cell(complete=True)),
                 pbc=atoms.pbc)


def big_frames(minority=None):
    """16,500 atoms (1032 tiles, the last one ragged) in five differently jittered fcc frames; with `minority`
    seven of them relabelled to that element."""
    frames = [fcc(rep=(10, 10, 10), jitter=0.04 + 0.01 * k, seed=100 + k) for k in range(4)]
    frames.append(fcc(rep=(5, 5, 5), jitter=0.07, seed=110))
    if minority:
        frames[0] = _relabel(frames[0], [3, 1000, 2999], minority)
        frames[4] = _relabel(frames[4], [17, 301, 402, 499], minority)
    return frames


def small_frames(elements):
    from tests.test_gpu_sf_dispatch import alloy
    return [alloy(elements, rep=(2, 2, 2), a=3.52, seed=3), alloy(elements, rep=(2, 2, 3), a=3.52, seed=8)]


def _is_grap(nn):
    return type(nn.descriptor).__name__ == "GenericRadialAtomicPotential"


def pin_descriptors(nn, atoms):
    """The GPU's descriptors of `atoms` against the oracle's (the G every reference below starts from)."""
    with Engine(nn) as eng:
        G = eng.evaluate([atoms], descriptors=True)[0]["descriptors"]
    o = (oracle_grap_eval if _is_grap(nn) else oracle_eval)(nn, atoms)["descriptors"]
    assert np.abs(G - o).max() < 1e-10 * max(1.0, np.abs(o).max()), np.abs(G - o).max()


def reference(nn, frames, G, dG, coeff):
    """oracle/train.py on the GPU's G and dG, one frame coefficient per atom: (energy gradient, loss gradient)."""
    from oracle.train import flatten, tangent_weight_gradients, weight_gradients
    assert np.all(nn.descriptor_scale() == 1.0)   # G, dG as the library and the oracle's model see them
    m = oracle_grap_model(nn) if _is_grap(nn) else oracle_model(nn)
    syms = [s for a in frames for s in a.get_chemical_symbols()]
    c = np.repeat(coeff, [len(a) for a in frames])
    e = flatten(m, weight_gradients(m, syms, G, c))
    g = flatten(m, tangent_weight_gradients(m, syms, G, dG, c)) if dG is not None else None
    return e, g


def gradients(eng, frames, seed=5):
    """(G, energy gradient, loss gradient, dG, coeff) of the resident batch along a random (dR, dh)."""
    rng = np.random.RandomState(seed)
    res = eng.evaluate(frames, descriptors=True)
    G = np.concatenate([r["descriptors"] for r in res])
    coeff = rng.randn(len(frames))
    dR = rng.randn(len(G), 3) * 0.3
    dh = rng.randn(len(frames), 3, 3) * 0.05
    ge = eng.energy_gradient(coeff)
    gl, dG = eng.loss_gradient(coeff, dR, dh, return_tangent=True)
    return G, ge, gl, dG, coeff


def assert_close(got, ref, tol=1e-9, what=""):
    err = np.abs(got - ref).max()
    assert err <= tol * max(1.0, np.abs(ref).max()), (what, err, np.abs(ref).max())


def check_against_oracle(nn, frames, what):
    with Engine(nn) as eng:
        eng.set_frames(frames)
        G, ge, gl, dG, coeff = gradients(eng, frames)
    assert np.abs(dG).max() > 0.0
    re, rl = reference(nn, frames, G, dG, coeff)
    assert_close(ge, re, what=f"{what}: energy gradient")
    assert_close(gl, rl, what=f"{what}: loss gradient")
    assert np.abs(gl - ge).max() > 1e-6 * np.abs(ge).max()    # the direction term is really there


# -- A. persistent-workgroup loop: more than 1024 tiles of one element -----------------------------------------

@pytest.mark.parametrize("elements", [("Ni",), ("Mo", "Ni")], ids=["Ni", "NiMo"])
def test_more_than_1024_tiles_against_oracle(lib, elements):
    nn = make_nn(list(elements), RC, True, [32, 32])
    frames = big_frames(minority="Mo" if len(elements) == 2 else None)
    n_tiles, n_ni = tiles(frames, "Ni")
    assert n_tiles > MAX_BLOCKS and n_ni % ROWS != 0, (n_tiles, n_ni)
    if len(elements) == 2:
        assert tiles(frames, "Mo") == (1, 7)
    pin_descriptors(nn, small_frames(list(elements))[0])
    check_against_oracle(nn, frames, "+".join(elements))


# -- A. widths on both sides of the 64 KB LDS boundaries ---------------------------------------------------------

WIDTHS = {   # name: (make_nn keyword arguments or "grap", mlp_grad / forward above 64 KB, mlp_grad2 above 64 KB)
    "h112": (dict(hidden=[112, 112]), False, False),
    "h128": (dict(hidden=[128, 128]), False, True),
    "h240": (dict(hidden=[240]), False, True),
    "h256": (dict(hidden=[256, 256]), True, True),
    "h128_resnet": (dict(hidden=[128, 128], resnet=True), False, True),
    "h128_minmax": (dict(hidden=[128, 128], minmax=True), False, True),
    "h32_64_128": (dict(hidden=[32, 64, 128]), False, True),
    "h20_50": (dict(hidden=[20, 50]), False, False),
    "grap_wide_descriptor": ("grap", False, True),
}


def width_model(name):
    kw = WIDTHS[name][0]
    if kw == "grap":
        nn = make_grap_nn(["Mo", "Ni"], RC, [16], moment_tensors=[0, 1, 2, 3, 4, 5])
        assert nn.ndim() > 112
        return nn
    return make_nn(["Mo", "Ni"], RC, True, kw["hidden"], resnet=kw.get("resnet", False),
                   minmax=kw.get("minmax", False), seed=13)


def test_width_table_sits_where_it_says():
    """CPU: each row of WIDTHS is on the side of the 64 KB boundaries its flags claim."""
    for name, (_, above2, above4) in WIDTHS.items():
        nn = width_model(name)
        assert (lds_bytes(nn, 2) > LDS_64K) == above2, (name, lds_bytes(nn, 2))
        assert (lds_bytes(nn, 4) > LDS_64K) == above4, (name, lds_bytes(nn, 4))
        assert lds_bytes(nn, 4) <= 150 * 1024, name


@pytest.mark.parametrize("name", list(WIDTHS))
def test_wide_networks_against_oracle(lib, name):
    nn = width_model(name)
    frames = small_frames(["Mo", "Ni"])
    pin_descriptors(nn, frames[0])
    check_against_oracle(nn, frames, name)


# -- A. every activation through the second-order pass -------------------------------------------------------

@pytest.mark.parametrize("activation", sorted(_lib.TA_ACT))
def test_every_activation_against_oracle(lib, activation):
    nn = make_nn(["Mo", "Ni"], RC, True, [24, 16], activation=activation, resnet=True, seed=21)
    frames = small_frames(["Mo", "Ni"])
    pin_descriptors(nn, frames[0])
    check_against_oracle(nn, frames, activation)


SATURATING_SCALE = 30.0     # on the first layer's weights; the test asserts what it has to achieve


def oracle_preactivations(nn, frames, monkeypatch):
    """Every argument the oracle's own forward pass (oracle/sf.py::apply_mlp) hands to its activation."""
    import oracle.sf as osf
    seen, real = [], osf.activation

    def recording(name, z):
        seen.append(np.array(z, dtype=float).ravel())
        return real(name, z)

    with monkeypatch.context() as patch:
        patch.setattr(osf, "activation", recording)
        results = [oracle_eval(nn, a) for a in frames]
    return np.concatenate(seen), results


@pytest.mark.parametrize("activation", sorted(_lib.TA_ACT))
def test_every_saturated_activation_against_oracle(lib, monkeypatch, activation):
    """The network of test_every_activation_against_oracle with its first layer scaled up until at least 1 % of the
    oracle's own pre-activations lie above 40 and at least 1 % below -40 (where softplus is max(x, 0) to double
    precision and 1 - tanh^2 has cancelled to 0): forward, backward and second-order tiles against the same oracle
    at the same bounds. tests/test_gpu_math.py holds the activations themselves to a 50-digit reference out there."""
    nn = make_nn(["Mo", "Ni"], RC, True, [24, 16], activation=activation, resnet=True, seed=21)
    for el in nn.elements:
        W, b = nn.weights[el][0]
        nn.weights[el][0] = (W * SATURATING_SCALE, b)
    frames = small_frames(["Mo", "Ni"])
    z, results = oracle_preactivations(nn, frames, monkeypatch)
    n_hidden = sum(len(a) for a in frames) * (24 + 16)
    assert z.size == n_hidden and np.all(np.isfinite(z))
    assert (z > 40.0).mean() >= 0.01 and (z < -40.0).mean() >= 0.01, ((z > 40.0).mean(), (z < -40.0).mean())
    for r in results:
        assert np.isfinite(r["energy"]) and np.all(np.isfinite(r["forces"]))
    check_against_oracle(nn, frames, activation + " (saturated)")


# -- A. an element absent from the batch -----------------------------------------------------------------------

def test_absent_element_slice_is_exactly_zero(lib):
    from oracle.train import flatten
    nn = make_nn(["Mo", "Ni"], RC, True, [32, 32])
    both = small_frames(["Mo", "Ni"])
    only_ni = [fcc(rep=(2, 2, 2), jitter=0.06, seed=4), fcc(rep=(2, 2, 3), jitter=0.05, seed=9)]
    m = oracle_model(nn)
    absent = flatten(m, {el: [(np.full(np.shape(W), el == "Mo"), np.full(np.shape(W)[1], el == "Mo"))
                              for W, _ in m.weights[el]] for el in m.elements}).astype(bool)
    with Engine(nn) as eng:
        eng.set_frames(both)
        _, ge0, gl0, _, _ = gradients(eng, both)
        assert np.abs(ge0[absent]).max() > 0.0 and np.abs(gl0[absent]).max() > 0.0
        eng.set_frames(only_ni)
        G, ge, gl, dG, coeff = gradients(eng, only_ni)
    assert np.all(ge[absent] == 0.0) and np.all(gl[absent] == 0.0)
    re, rl = reference(nn, only_ni, G, dG, coeff)
    assert_close(ge, re, what="energy gradient")
    assert_close(gl, rl, what="loss gradient")


def test_too_wide_for_the_second_order_tile_is_refused(lib):
    """Widest layer 320: mlp_grad2 would need 4 x 16 x 322 doubles (161 KB) of LDS. `ta_loss_gradient` and
    `ta_hessian_vectors` refuse with a ValueError; evaluation and the energy gradient (82 KB, above 64 KB)
    still run, and agree with the oracle."""
    nn = make_nn(["Mo", "Ni"], RC, True, [320], seed=3)
    assert lds_bytes(nn, 4) > 150 * 1024 and LDS_64K < lds_bytes(nn, 2) <= 150 * 1024
    frames = small_frames(["Mo", "Ni"])
    pin_descriptors(nn, frames[0])
    coeff = np.array([0.7, -1.3])
    N = sum(len(a) for a in frames)
    dR = np.random.RandomState(1).randn(N, 3)
    with Engine(nn) as eng:
        res = eng.evaluate(frames, descriptors=True)
        with pytest.raises(ValueError, match="too wide"):
            eng.loss_gradient(coeff, dR)
        with pytest.raises(ValueError, match="too wide"):
            eng.hessian_vectors(dR=dR[None])
        ge = eng.energy_gradient(coeff)
        again = eng.evaluate(frames)
    for r, o, a in zip(res, again, frames):
        assert abs(r["energy"] - o["energy"]) < 1e-10 * max(1.0, abs(r["energy"]))
        assert abs(r["energy"] - oracle_eval(nn, a)["energy"]) < 1e-9 * max(1.0, abs(r["energy"]))
    G = np.concatenate([r["descriptors"] for r in res])
    re, _ = reference(nn, frames, G, None, coeff)
    assert_close(ge, re, what="energy gradient")


# -- B. nn-EAM / ADP networks over pairs ----------------------------------------------------------------------

def _nimo_alloy(rep=(2, 2, 2), seed=3):
    from tests.test_gpu_sf import _alloy
    return _alloy(["Ni", "Mo"], rep=rep, seed=seed)


EAM_KINDS = {
    "eam_ni": lambda: (make_eam(["Ni"], 6.0, potential=None, hidden_sizes=[16, 8]), fcc(rep=(2, 2, 2), jitter=0.08)),
    "eam_binary_mixed": lambda: (make_eam(["Mo", "Ni"], 6.0, hidden_sizes=[12], potential={
        "Ni": {"rho": "nn", "embed": "zjw04"}, "Mo": {"rho": "zjw04", "embed": "nn"},
        "NiNi": {"phi": "zjw04"}, "MoNi": {"phi": "nn"}, "MoMo": {"phi": "nn"}}), _nimo_alloy()),
    "adp_all_nn": lambda: (make_eam(["Mo", "Ni"], 5.5, adp=True, potential=None, hidden_sizes=[8, 8]), _nimo_alloy()),
}


def _copy(atoms):
    return Atoms(numbers=np.asarray(atoms.numbers).copy(), positions=atoms.positions.copy(),
                 cell=np.asarray(atoms.get_cell(complete=True)).copy(), pbc=np.asarray(atoms.pbc).copy())


@pytest.mark.parametrize("kind", list(EAM_KINDS))
def test_nn_eam_gradients_are_additive_over_copies(lib, kind):
    """K copies of one frame (the frames test_gpu_train.py pins by finite differences) with distinct frame
    coefficients: energy_gradient(c) = sum c_k g1 and loss_gradient(c, tiled dR, dh) = sum c_k g1 + K g_dir,1,
    over several hundred thousand pair rows."""
    nn, atoms = EAM_KINDS[kind]()
    K = 96
    rng = np.random.RandomState(7)
    dR1 = rng.randn(len(atoms), 3) * 0.3
    dh1 = rng.randn(1, 3, 3) * 0.2
    with Engine(nn) as eng:
        eng.set_frames([atoms])
        g1 = eng.energy_gradient(np.ones(1))
        gdir1 = eng.loss_gradient(np.zeros(1), dR1, dh1)
    coeff = rng.randn(K)
    with Engine(nn) as eng:
        eng.set_frames([_copy(atoms) for _ in range(K)])
        n_pairs = int(eng.info.n_pairs)
        ge = eng.energy_gradient(coeff)
        gl = eng.loss_gradient(coeff, np.tile(dR1, (K, 1)), np.repeat(dh1, K, axis=0))
    assert n_pairs > 8 * ROWS * MAX_BLOCKS, n_pairs
    assert np.abs(gdir1).max() > 1e-3
    assert_close(ge, coeff.sum() * g1, 1e-10, "energy gradient")
    assert_close(gl, coeff.sum() * g1 + K * gdir1, 1e-10, "loss gradient")


def _eam_direction_check(nn, frames, seed=11, tol=2e-6):
    """(a) of test_nn_eam_analytic_force_stress_loss_gradient: the direction term of `ta_loss_gradient` against
    the central difference of `ta_energy_gradient` on displaced frames. Returns (masked energy gradient, frame
    coefficients, pair count of the batch)."""
    from tensoralloy_amd.train import trainable_mask
    rng = np.random.RandomState(seed)
    coeff = rng.randn(len(frames))
    dR = [rng.randn(len(a), 3) * 0.3 for a in frames]
    dh = [rng.randn(3, 3) * 0.2 for _ in frames]
    mask = trainable_mask(nn)

    def displaced(eps):
        return [Atoms(numbers=np.asarray(a.numbers).copy(), positions=a.positions + eps * dR[k],
                      cell=np.asarray(a.get_cell(complete=True)) + eps * dh[k], pbc=np.asarray(a.pbc).copy())
                for k, a in enumerate(frames)]

    with Engine(nn) as eng:
        eng.set_frames(frames)
        n_pairs = int(eng.info.n_pairs)
        g = eng.loss_gradient(coeff, np.concatenate(dR), np.array(dh)) * mask
        g_dir = eng.loss_gradient(None, np.concatenate(dR), np.array(dh)) * mask
        g_e = eng.energy_gradient(coeff) * mask
        e = 1e-4
        eng.set_frames(displaced(e))
        gp = eng.energy_gradient(np.ones(len(frames)))
        eng.set_frames(displaced(-e))
        gm = eng.energy_gradient(np.ones(len(frames)))
    fd = (gp - gm) / (2 * e) * mask
    scale = max(1.0, np.abs(g).max())
    assert np.abs(g_dir - fd).max() < tol * scale, np.abs(g_dir - fd).max() / scale
    assert np.abs(g - (g_e + fd)).max() < tol * scale
    assert np.abs(g_dir).max() > 1e-3
    return g_e, coeff, n_pairs


def test_nn_eam_full_size_frame(lib):
    """One 4000-atom frame at rc 6.5: some 350,000 pair rows through mlp_grad2 over the pairs. The nn functions
    have no cutoff (oracle/eam.py), so the energy jumps where a pair crosses rc: a small jitter keeps every pair
    distance well clear of rc (0.09 A below the 7th shell) for the displaced frames of the difference."""
    nn = make_eam(["Ni"], 6.5, potential=None, hidden_sizes=[16, 8])
    _, _, n_pairs = _eam_direction_check(nn, [fcc(rep=(10, 10, 10), jitter=0.01, seed=12)])
    assert -(-n_pairs // ROWS) > MAX_BLOCKS, n_pairs


def test_nn_eam_wide_networks(lib):
    """[128, 128] networks: 66,560 B of LDS in mlp_grad2 over the pairs. The direction term by finite
    differences, the energy gradient in single weights against the oracle's energies."""
    from tensoralloy_amd.train import flatten_weights, unflatten_weights
    nn = make_eam(["Ni"], 6.0, potential=None, hidden_sizes=[128, 128])
    assert 4 * ROWS * (128 + 2) * 8 > LDS_64K
    frames = [fcc(rep=(2, 2, 2), jitter=0.08)]
    g_e, coeff, _ = _eam_direction_check(nn, frames)
    theta, saved = flatten_weights(nn), nn.weights

    def oracle_loss(vec):
        nn.weights = unflatten_weights(nn, vec)
        try:
            return sum(c * oracle_eam_eval(nn, a)["energy"] for a, c in zip(frames, coeff))
        finally:
            nn.weights = saved

    live = np.flatnonzero(g_e)
    picks = list(np.random.RandomState(5).choice(live, size=8, replace=False)) + [live[0], live[-1]]
    scale = max(1.0, np.abs(g_e).max())
    for k in picks:
        d = 1e-5
        tp, tm = theta.copy(), theta.copy()
        tp[k] += d
        tm[k] -= d
        num = (oracle_loss(tp) - oracle_loss(tm)) / (2 * d)
        assert abs(g_e[k] - num) < 2e-6 * scale, (k, g_e[k], num)


# -- C. temperature-dependent training -------------------------------------------------------------------------

def _td_model(hidden, elements=("Mo", "Ni")):
    from tests.test_gpu_td_train import _base, td_from
    static = {el: -1.0 - 0.5 * i for i, el in enumerate(elements)}
    return td_from(_base("sf", list(elements)), (20, 20, 9), hidden, act_h="tanh", activation="softplus",
                   static=static)


def _with_temperatures(frames, temperatures):
    for a, T in zip(frames, temperatures):
        a.info["etemperature"] = T
    return frames


def _td_check(nn, frames, seed=3):
    from tests.test_gpu_td_train import _engine_inputs, _per_atom, _symbols
    from tests.td_train_reference import td_loss_gradient_reference
    F, N = len(frames), sum(len(a) for a in frames)
    rng = np.random.RandomState(seed)
    a, b, g = rng.normal(size=F), rng.normal(size=F), rng.normal(size=F)
    dR, dh = 0.3 * rng.normal(size=(N, 3)), 0.05 * rng.normal(size=(F, 3, 3))
    with Engine(nn, device=0) as eng:
        _, G, T = _engine_inputs(eng, frames)
        got, dG = eng.td_loss_gradient(b, a, g, dR, dh, return_tangent=True)
        energy_only = eng.td_loss_gradient(b, a, g)
    syms = _symbols(frames)
    per = [_per_atom(frames, c) for c in (a, b, g)]
    ref = td_loss_gradient_reference(nn, syms, G, dG, T, *per)
    assert_close(got, ref, what="td loss gradient")
    ref0 = td_loss_gradient_reference(nn, syms, G, np.zeros_like(G), T, *per)
    assert_close(energy_only, ref0, what="td energy terms")


def test_td_loss_gradient_more_than_1024_tiles(lib):
    nn = _td_model((32, 32))
    frames = _with_temperatures(big_frames(minority="Mo"), (0.0, 0.3, 0.8, 1.3, 2.0))
    assert sum(tiles(frames, el)[0] for el in ("Mo", "Ni")) > MAX_BLOCKS
    _td_check(nn, frames)


def _td_lds_bytes(nn):
    """lds_bytes of td_grad_plan (ta_td_train.hip): 16 x (4 sP + 2 sz) doubles."""
    hidden = max(-(-w // 16) * 16 for w in [nn.ndim()] + [w for h in nn.hidden_sizes.values() for w in h])
    sP = max(hidden, 32) + 2          # (the U / S nets are 20 wide, padded 32)
    sz = 16 + 2                       # their layer-0 input: K = 9 columns and T, padded 16
    return ROWS * (4 * sP + 2 * sz) * 8


def test_td_wide_network_takes_the_attribute_path(lib):
    nn = _td_model((128, 128))
    assert LDS_64K < _td_lds_bytes(nn) <= 150 * 1024, _td_lds_bytes(nn)
    frames = _with_temperatures(small_frames(["Mo", "Ni"]), (0.2, 1.1))
    _td_check(nn, frames)


def test_td_too_wide_network_is_refused_cleanly(lib):
    nn = _td_model((320,))
    assert _td_lds_bytes(nn) > 150 * 1024, _td_lds_bytes(nn)
    frames = _with_temperatures(small_frames(["Mo", "Ni"]), (0.2, 1.1))
    c = np.array([0.4, -0.9])
    with Engine(nn, device=0) as eng:
        first = eng.evaluate(frames)
        with pytest.raises(ValueError, match="too wide"):
            eng.td_loss_gradient(c, c, c)
        again = eng.evaluate(frames)
    for r, o in zip(first, again):
        assert abs(r["energy"] - o["energy"]) < 1e-10 * max(1.0, abs(r["energy"]))
        assert np.abs(r["forces"] - o["forces"]).max() < 1e-10


# -- D. the descriptor Jacobian across the angular dispatch ----------------------------------------------------

def _dispatch_rows():
    from tests.test_gpu_sf_dispatch import (CAPS, ELEMENTS, MULTI, alloy, matrix_model, sparse_cluster)
    rows = {}
    for key, cls, cap in ((112, "h12", 192), (222, "h16", 192), (322, "h24", 192), (522, "exact_poly", 192),
                          (212, "h12", 256), (121, "exact_cos", 192)):
        nspec = key // 100
        rows[f"{key}-{cls}-cap{cap}"] = lambda key=key, cls=cls, cap=cap, nspec=nspec: (
            matrix_model(key, cls, cap), [alloy(ELEMENTS[nspec])], (CAPS[cap][1], CAPS[cap][2]))
    for nspec in (1, 5):
        rows[f"cap1024-{nspec}el"] = lambda nspec=nspec: (
            make_nn(ELEMENTS[nspec], CAPS[1024][0], True, [16], sf_kwargs=dict(eta=[0.05, 4.0])),
            [alloy(ELEMENTS[nspec])], (CAPS[1024][1], CAPS[1024][2]))
    for nspec, cap in ((2, 192), (3, 256)):
        rows[f"multi-{nspec}el-cap{cap}"] = lambda nspec=nspec, cap=cap: (
            make_nn(ELEMENTS[nspec], CAPS[cap][0], True, [16, 16], sf_kwargs=dict(eta=[0.05, 4.0], **MULTI),
                    minmax=True),
            [alloy(ELEMENTS[nspec], seed=31)], (CAPS[cap][1], CAPS[cap][2]))
    for nspec in (3, 5):
        els = ELEMENTS[nspec]
        rows[f"sparse-{nspec}el"] = lambda els=els: (
            make_nn(els, 5.0, True, [16], sf_kwargs=dict(eta=[0.05, 4.0])),
            [alloy(els[:-1], seed=41), sparse_cluster(els), alloy(els, rep=(2, 2, 3), seed=42),
             sparse_cluster(els[1:], seed=6)], (1, 192))
    # first-generation angular kernels (tests/test_gpu_sf_v1.py): `backward_only` runs their chunk chain once per
    # descriptor with a one-hot dE/dG
    from tests.test_gpu_sf_v1 import MODELS, edge_frames, uneven
    # a = 3.35: rc = 5.0 lies between the 4th and the 5th shell (4.74, 5.30). In the a = 3.6 frames of
    # test_gpu_sf_v1.py one pair sits 9e-5 A from the cutoff and crosses it inside the stencil; the difference
    # quotient of the ORACLE's descriptors then changes by 1.6e-5 between e = 1e-3 and 5e-4 (6e-12 here).
    rows["v1-multi-4el"] = lambda: (MODELS["b-multi-4el"][0](), uneven(ELEMENTS[4], 21, a=3.35), (1, 192))
    rows["v1-6el-sparse"] = lambda: (MODELS["e-6el"][0](), edge_frames(MODELS["e-6el"][0]().elements), (1, 192))
    rows["v1-forced-211"] = lambda: (MODELS["a-211"][0](), [alloy(ELEMENTS[2])], (1, 192))
    return rows


DISPATCH = _dispatch_rows()
V1_ROWS = {"v1-multi-4el": False, "v1-6el-sparse": False, "v1-forced-211": True}   # row: needs TA_FORCE_V1


def _engine(nn, monkeypatch, row):
    """Rows of V1_ROWS: the engine the dispatcher (or TA_FORCE_V1, read when it is made) gives these kernels."""
    from tests.test_gpu_sf_v1 import engine
    return engine(nn, monkeypatch, V1_ROWS.get(row, False))


def _assert_first_generation(eng, row):
    assert eng.list_layout("kernel")["info"]["n_blk"] == 0, row


@pytest.mark.parametrize("row", list(DISPATCH))
def test_descriptor_tangent_across_the_dispatch(lib, monkeypatch, row):
    """dG of `ta_loss_gradient` against a sixth-order central difference of the GPU's own descriptors (which
    test_gpu_sf_dispatch.py and test_gpu_sf_v1.py pin to the oracle) along a random (dR, dh)."""
    nn, frames, window = DISPATCH[row]()
    rng = np.random.RandomState(5)
    dR = [rng.randn(len(a), 3) * 0.3 for a in frames]
    dh = [rng.randn(3, 3) * 0.05 if np.any(a.pbc) else np.zeros((3, 3)) for a in frames]
    e = 1e-3
    with _engine(nn, monkeypatch, row) as eng:
        eng.set_frames(frames)
        nnl = int(eng.info.nnl_max)
        assert window[0] <= nnl <= window[1], (row, nnl)
        if row in V1_ROWS:
            _assert_first_generation(eng, row)
        _, dG = eng.loss_gradient(np.ones(len(frames)), np.concatenate(dR), np.array(dh), return_tangent=True)

        def G_at(t):
            moved = [Atoms(numbers=np.asarray(a.numbers).copy(), positions=a.positions + t * d_r,
                           cell=np.asarray(a.get_cell()) + t * d_h, pbc=np.asarray(a.pbc).copy())
                     for a, d_r, d_h in zip(frames, dR, dh)]
            return np.concatenate([r["descriptors"] for r in eng.evaluate(moved, descriptors=True)])
        dG_fd = (45.0 * (G_at(e) - G_at(-e)) - 9.0 * (G_at(2 * e) - G_at(-2 * e)) +
                 (G_at(3 * e) - G_at(-3 * e))) / (60.0 * e)
    assert np.abs(dG).max() > 1e-3
    assert np.abs(dG - dG_fd).max() < 1e-6 * max(1.0, np.abs(dG_fd).max()), (row, np.abs(dG - dG_fd).max())


def test_loss_gradient_on_the_first_generation_kernels(lib, monkeypatch):
    """`ta_energy_gradient` and `ta_loss_gradient` of the four-element 3 x 3 x 3 model (eight chunks per one-hot
    backward chain) against oracle/train.py on the GPU's G and dG: the comparison and the 1e-9 bound of
    `check_against_oracle`; G is pinned to the oracle by test_gpu_sf_v1.py, dG by the row `v1-multi-4el` above."""
    row = "v1-multi-4el"
    nn, frames, _ = DISPATCH[row]()
    with _engine(nn, monkeypatch, row) as eng:
        eng.set_frames(frames)
        _assert_first_generation(eng, row)
        G, ge, gl, dG, coeff = gradients(eng, frames)
        _assert_first_generation(eng, row)
    assert np.abs(dG).max() > 0.0
    re, rl = reference(nn, frames, G, dG, coeff)
    assert_close(ge, re, what=f"{row}: energy gradient")
    assert_close(gl, rl, what=f"{row}: loss gradient")
    assert np.abs(gl - ge).max() > 1e-6 * np.abs(ge).max()    # the direction term is really there


# -- E. Hessian-vector products --------------------------------------------------------------------------------

def test_hessian_vectors_of_the_wide_nimo_model(lib):
    """The [128, 128] Ni-Mo model of the C3 configuration (mlp_grad2 at 66,560 B of LDS) against central
    differences of the GPU's forces and virial (test_gpu_sf.py::test_analytic_hessian_vectors_of_the_descriptor_models;
    the same kernels against the oracle at 1e-8: test_gpu_hvp_oracle.py)."""
    from tests.test_gpu_sf import _alloy
    nn = make_nn(["Ni", "Mo"], 6.5, True, [128, 128])
    assert lds_bytes(nn, 4) > LDS_64K
    atoms = _alloy(["Ni", "Ni", "Ni", "Mo"], rep=(2, 2, 2), seed=4)
    atoms = Atoms(symbols=atoms.get_chemical_symbols(),
                  positions=atoms.positions + np.random.RandomState(9).normal(0, 0.08, atoms.positions.shape),
                  cell=np.asarray(atoms.get_cell(complete=True)), pbc=True)
    n = len(atoms)
    h = np.asarray(atoms.get_cell(complete=True), dtype=float)
    rng = np.random.RandomState(2)
    dR = rng.normal(size=(2, n, 3))
    dh = rng.normal(size=(2, 1, 3, 3)) * 0.3
    dR[1] = 0.0
    eps = 1e-4
    with Engine(nn) as eng:
        eng.set_frames([atoms])
        dF, dW = eng.hessian_vectors(dR=dR, dh=dh, want_virial=True)
        for d in range(2):
            fd_F, fd_W = 0.0, 0.0
            for sgn in (1.0, -1.0):
                a = Atoms(symbols=atoms.get_chemical_symbols(), positions=atoms.positions + sgn * eps * dR[d],
                          cell=h + sgn * eps * dh[d, 0], pbc=True)
                r = eng.evaluate([a], want=1 | 2 | 4)[0]
                fd_F = fd_F + sgn * r["forces"] / (2 * eps)
                fd_W = fd_W + sgn * r["virial"] / (2 * eps)
            assert np.abs(dF[d] - fd_F).max() < 2e-6 * max(1.0, np.abs(fd_F).max()), (d, np.abs(dF[d] - fd_F).max())
            assert np.abs(dW[d, 0] - fd_W).max() < 2e-6 * max(1.0, np.abs(fd_W).max()), (d, np.abs(dW[d, 0] - fd_W).max())


def test_hessian_vectors_of_copies_above_1024_tiles(lib):
    """65 copies of a 256-atom frame (1040 tiles) with the same per-copy direction: every copy's dF and dW equal
    the single frame's (batches of DIFFERENT frames, against the oracle: test_gpu_hvp_oracle.py)."""
    nn = make_nn(["Ni"], RC, True, [32, 32])
    atoms = fcc(rep=(4, 4, 4), jitter=0.08, seed=14)
    K, n = 65, len(atoms)
    assert -(-K * n // ROWS) > MAX_BLOCKS
    rng = np.random.RandomState(3)
    dR1 = rng.normal(size=(1, n, 3))
    dh1 = rng.normal(size=(1, 1, 3, 3)) * 0.2
    with Engine(nn) as eng:
        eng.set_frames([atoms])
        dF1, dW1 = eng.hessian_vectors(dR=dR1, dh=dh1, want_virial=True)
    with Engine(nn) as eng:
        eng.set_frames([_copy(atoms) for _ in range(K)])
        dF, dW = eng.hessian_vectors(dR=np.tile(dR1, (1, K, 1)), dh=np.repeat(dh1, K, axis=1), want_virial=True)
    dF = dF.reshape(K, n, 3)
    scale_F, scale_W = max(1.0, np.abs(dF1).max()), max(1.0, np.abs(dW1).max())
    assert np.abs(dF - dF1[0][None]).max() < 1e-10 * scale_F
    assert np.abs(dW[0] - dW1[0, 0][None]).max() < 1e-10 * scale_W
