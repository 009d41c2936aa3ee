"""GPU: the training and derivative entry points of the C ABI (csrc/ta_api_train.hip) as one family.

(a) Every checked refusal of every entry point, for every model kind: the error code and the message the
    caller reads, the function name it carries included. Each case returns before any launch.
(b) The grow-only buffers the entry points share on the handle (train_*, tan_*, jvp_J, filt_scratch,
    hvp_buf): whatever ran on the handle before, in whichever order and with a larger batch in between,
    every entry point gives what it gives as the first call on a fresh handle."""
import ctypes as C
import functools

import numpy as np
import pytest

from tensoralloy_amd import Atoms, Engine, _lib
from tests.helpers import fcc, make_eam, make_grap_nn, make_nn

pytestmark = pytest.mark.gpu

OK, INV, UNS = _lib.TA_OK, _lib.TA_ERR_INVALID, _lib.TA_ERR_UNSUPPORTED
NULL = _lib._dp()
ELS = ["Mo", "Ni"]
SF_KW = {"eta": [0.1, 1.0], "omega": [0.0], "beta": [0.005], "gamma": [1.0, -1.0], "zeta": [1.0, 4.0]}
FILTER_NET = {"hidden_sizes": [8], "num_filters": 4, "activation": "softplus", "use_resnet_dt": False,
              "h_abck_modifier": 0}
# embedding networks beside analytic densities and pair functions: every EAM entry point serves this one
NN_EMBED = {"Mo": {"rho": "zjw04", "embed": "nn"}, "Ni": {"rho": "zjw04", "embed": "nn"},
            "MoMo": {"phi": "zjw04"}, "MoNi": {"phi": "zjw04"}, "NiNi": {"phi": "zjw04"}}
KINDS = ["sf", "grap-pexp", "grap-nn", "td", "eam", "eam-nn", "eam-nn-pair", "fs"]
EAM = ("eam", "eam-nn", "eam-nn-pair")
SKIN_FILTERS = ("sf", "td") + EAM   # kinds whose kernels run on the exact list extracted from a skin list


@functools.lru_cache(maxsize=None)
def model(kind):
    """Two elements (a non-zero offset of the second element's gradient), one hidden layer of 8."""
    if kind == "sf":
        return make_nn(ELS, 4.5, True, [8], sf_kwargs=SF_KW)
    if kind == "grap-pexp":
        return make_grap_nn(ELS, 4.5, [8], algorithm="pexp", moment_tensors=(0, 1, 2))
    if kind == "grap-nn":
        return make_grap_nn(ELS, 4.5, [8], "nn", dict(FILTER_NET), moment_tensors=(0, 1, 2))
    if kind == "td":
        from tests.test_gpu_td_train import td_from
        return td_from(make_nn(ELS, 4.5, True, [8], sf_kwargs=SF_KW), (8, 5), (8,))
    if kind == "eam":
        return make_eam(ELS, 5.5, potential="zjw04")
    if kind == "eam-nn":
        return make_eam(ELS, 5.5, potential=NN_EMBED, hidden_sizes=[8])
    if kind == "eam-nn-pair":   # every function a network: pair functions through their tables until trained
        return make_eam(ELS, 5.5, potential=None, hidden_sizes=[8])
    from tests.test_gpu_eam_fs import _random_nn
    return _random_nn(["Al", "Fe"], hidden_sizes=[8])


def frame(kind, rep, seed):
    els = ["Al", "Fe"] if kind == "fs" else ELS
    a = fcc(els[0], rep=rep, jitter=0.05, seed=seed)
    out = Atoms(symbols=[els[i % 2] for i in range(len(a))], positions=a.positions,
                cell=np.asarray(a.get_cell(complete=True)), pbc=True)
    out.info["etemperature"] = 0.1 * rep[2]
    return out


def batch(kind, which):
    """"small": two frames of different sizes (32 + 48 atoms); "large": more frames, atoms and pairs."""
    reps = [(2, 2, 2), (2, 2, 3)] if which == "small" else [(2, 2, 3), (2, 3, 3), (2, 2, 2)]
    return [frame(kind, rep, 40 + k) for k, rep in enumerate(reps)]


# ---- (a) refusals -------------------------------------------------------------------------------------------------

def dp(a):
    return NULL if a is None else _lib.as_dp(a)


class Raw:
    """The ctypes symbols themselves (the wrappers of engine.py refuse some of these before the library sees them):
    returns the code and the message of ta_last_error."""

    def __init__(self, eng, n_atoms, n_frames):
        self.eng, self.N, self.F = eng, n_atoms, n_frames
        rng = np.random.RandomState(3)
        self.c, self.dR, self.dh = rng.normal(size=n_frames), rng.normal(size=(n_atoms, 3)), rng.normal(size=(n_frames, 9))
        self.dG = np.zeros((n_atoms, 64))
        self.out = np.zeros(max(4096, 12 * n_atoms + 18 * n_frames))   # room for any gradient or dF / dW of 2 directions

    def __call__(self, fn, *args):
        rc = getattr(self.eng._lib, fn)(self.eng._handle, *args)
        msg = self.eng._lib.ta_last_error(self.eng._handle)
        return rc, (msg.decode("utf-8", "replace") if msg else "")

    def count(self, fn):
        n = C.c_int64(0)
        rc, _ = self(fn, C.byref(n))
        return rc, int(n.value)

    def energy_gradient(self, c, n):
        return self("ta_energy_gradient", dp(c), dp(self.out), n)

    def loss_gradient(self, c, dR, dh, n, dG=None):
        return self("ta_loss_gradient", dp(c), dp(dR), dp(dh), dp(self.out), n, dp(dG))

    def td_loss_gradient(self, b, dR, dh, n, dG=None):
        return self("ta_td_loss_gradient", dp(b), NULL, NULL, dp(dR), dp(dh), dp(self.out), n, dp(dG))

    def grap_loss_gradient(self, c, dR, dh, n):
        return self("ta_grap_loss_gradient", dp(c), dp(dR), dp(dh), dp(self.out), n)

    def constant_gradient(self, c, dR, dh, n):
        return self("ta_constant_gradient", dp(c), dp(dR), dp(dh), dp(self.out), n)

    def hessian_vectors(self, n_dir, first, dR=None):
        return self("ta_hessian_vectors", n_dir, first, dp(dR), NULL, dp(self.out), NULL)


def fs_text(fn):
    return fn + ": not available for eam/fs models (inference only"


def skin_text(fn):
    return fn + ": not available on a skin-filtered batch; ta_set_skin(h, 0) and ta_set_frames first"


NO_BATCH = "no resident batch"
NOTHING = "nothing to differentiate"
NO_POTENTIAL = "the model has no empirical potential"
NOT_TD = "ta_td_loss_gradient: not a temperature-dependent model"
TD_HVP = "ta_hessian_vectors: not available for finite-temperature (temperature-dependent) models"


def grap_loss_refusal(kind):
    """What ta_grap_loss_gradient answers before it looks at the batch; None: the model is served."""
    if kind == "td":
        return UNS, "ta_grap_loss_gradient: the filter network of a temperature-dependent model is not trained"
    if kind == "grap-pexp":
        return UNS, "ta_grap_loss_gradient: the model's radial filters are analytic functions, not the `nn` filter network"
    return None if kind == "grap-nn" else (UNS, "ta_grap_loss_gradient: not a GRAP model")


def rows_without_batch(kind, r):
    """(what, (code, message), expected code, expected fragment) on a handle that has no batch yet."""
    fs, td = kind == "fs", kind == "td"
    rows = [
        ("energy_gradient", r.energy_gradient(r.c, 8), INV, fs_text("ta_energy_gradient") if fs else NO_BATCH),
        ("loss_gradient dR", r.loss_gradient(r.c, r.dR, None, 8), INV, fs_text("ta_loss_gradient") if fs else NO_BATCH),
        # a temperature-dependent handle looks at the arguments first, the others at the batch
        ("loss_gradient nothing", r.loss_gradient(None, None, None, 8), INV,
         fs_text("ta_loss_gradient") if fs else NOTHING if td else NO_BATCH),
        ("td_loss_gradient", r.td_loss_gradient(r.c, None, None, 8), INV, NO_BATCH if td else NOT_TD),
        ("grap_loss_gradient", r.grap_loss_gradient(r.c, r.dR, None, 8)) + (grap_loss_refusal(kind) or (INV, NO_BATCH)),
        ("constant_gradient", r.constant_gradient(r.c, None, None, 8), INV,
         fs_text("ta_constant_gradient") if fs else NO_BATCH),
        ("hessian_vectors", r.hessian_vectors(3, 0)) +
        ((UNS, TD_HVP) if td else (INV, fs_text("ta_hessian_vectors") if fs else NO_BATCH)),
        ("set_filter_tables", r("ta_set_filter_tables", 1, 3), INV, "ta_set_filter_tables: 5 .. 2^20 + 1 knots"),
        ("update_filter_weights", r("ta_update_filter_weights", dp(r.out), 1), INV,
         "ta_update_filter_weights: " + ("expected " if kind == "grap-nn" else "the model has no filter network")),
        ("update_weights", r("ta_update_weights", dp(r.out), 1), INV,
         "ta_update_weights: " + ("wrong number of values" if kind in EAM or fs else "expected ")),
    ]
    if kind in EAM or fs:
        rows += [("get_constants", r("ta_get_constants", dp(r.out), 1), INV, "ta_get_constants: wrong length"),
                 ("update_constants", r("ta_update_constants", dp(r.out), 1), INV,
                  "ta_update_constants: wrong number of values")]
    else:
        n = C.c_int64(0)
        rows += [("constant_count", r("ta_constant_count", C.byref(n)), INV, NO_POTENTIAL),
                 ("get_constants", r("ta_get_constants", dp(r.out), 1), INV, NO_POTENTIAL),
                 ("update_constants", r("ta_update_constants", dp(r.out), 1), INV, NO_POTENTIAL)]
    return rows


def rows_with_batch(kind, r, n_params, n_filter, n_const):
    fs, td, eam = kind == "fs", kind == "td", kind in EAM
    wrong = n_params + 1
    room = ": expected room for " + str(n_params) + " values"
    rows = [("energy_gradient no coefficients", r.energy_gradient(None, n_params), INV, None),
            ("hessian_vectors n_dir < 0", r.hessian_vectors(-1, 0), INV, None)]
    if fs:
        return rows + [
            ("energy_gradient", r.energy_gradient(r.c, n_params), INV, fs_text("ta_energy_gradient")),
            ("loss_gradient", r.loss_gradient(r.c, r.dR, r.dh, n_params), INV, fs_text("ta_loss_gradient")),
            ("loss_gradient nothing", r.loss_gradient(None, None, None, n_params), INV, fs_text("ta_loss_gradient")),
            ("constant_gradient", r.constant_gradient(r.c, r.dR, None, n_const), INV, fs_text("ta_constant_gradient")),
            ("hessian_vectors", r.hessian_vectors(3, 0), INV, fs_text("ta_hessian_vectors")),
            ("td_loss_gradient", r.td_loss_gradient(r.c, None, None, n_params), INV, NOT_TD),
            ("grap_loss_gradient", r.grap_loss_gradient(r.c, None, None, n_params)) + grap_loss_refusal(kind)]
    # delegations carry the delegate's name: to ta_td_loss_gradient, and without a direction to ta_energy_gradient
    name = "ta_td_loss_gradient" if td else "ta_energy_gradient"
    rows += [
        ("energy_gradient n_grad", r.energy_gradient(r.c, wrong), INV, name + room),
        ("loss_gradient nothing", r.loss_gradient(None, None, None, n_params), INV, NOTHING),
        ("loss_gradient energy only n_grad", r.loss_gradient(r.c, None, None, wrong), INV, name + room),
        ("loss_gradient n_grad", r.loss_gradient(r.c, r.dR, None, wrong), INV,
         ("ta_td_loss_gradient" if td else "ta_loss_gradient") + room),
        ("loss_gradient dh n_grad", r.loss_gradient(None, None, r.dh, wrong), INV,
         ("ta_td_loss_gradient" if td else "ta_loss_gradient") + room),
    ]
    if td:
        rows += [("td_loss_gradient n_grad", r.td_loss_gradient(r.c, r.dR, None, wrong), INV, "ta_td_loss_gradient" + room),
                 ("td_loss_gradient dG_out", r.td_loss_gradient(r.c, None, None, n_params, r.dG), INV,
                  "ta_td_loss_gradient: dG_out needs a direction"),
                 ("hessian_vectors", r.hessian_vectors(3, 0), UNS, TD_HVP)]
    else:
        rows += [("td_loss_gradient", r.td_loss_gradient(r.c, r.dR, None, n_params), INV, NOT_TD)]
    if kind == "grap-nn":
        rows += [("grap_loss_gradient nothing", r.grap_loss_gradient(None, None, None, n_params + n_filter), INV, NOTHING),
                 ("grap_loss_gradient n_grad", r.grap_loss_gradient(r.c, r.dR, None, n_params), INV,
                  "ta_grap_loss_gradient: expected room for " + str(n_params + n_filter) + " values")]
    else:
        rows += [("grap_loss_gradient", r.grap_loss_gradient(r.c, r.dR, None, n_params)) + grap_loss_refusal(kind)]
    if eam:
        rows += [("loss_gradient dG_out", r.loss_gradient(r.c, r.dR, None, n_params, r.dG), INV,
                  "ta_loss_gradient: dG_out is for the descriptor models"),
                 ("constant_gradient nothing", r.constant_gradient(None, None, None, n_const), INV, NOTHING),
                 ("constant_gradient n_grad", r.constant_gradient(r.c, r.dR, None, n_const + 1), INV,
                  "ta_constant_gradient: expected room for " + str(n_const) + " values")]
    else:
        rows += [("constant_gradient", r.constant_gradient(r.c, r.dR, None, 8), INV, NO_POTENTIAL)]
    if not td:
        rows += [("hessian_vectors unit range", r.hessian_vectors(2, 3 * r.N - 1), INV,
                  "ta_hessian_vectors: without dR / dh the directions are unit displacements"),
                 ("hessian_vectors 65536", r.hessian_vectors(65536, 0, r.dR), INV,
                  "ta_hessian_vectors: at most 65535 directions per call")]
    return rows


def rows_on_skin(kind, r, n_params, n_const):
    """On a skin-filtered batch. (GRAP models run on the skin list itself and are served.)"""
    td, eam = kind == "td", kind in EAM
    name = "ta_td_loss_gradient" if td else "ta_loss_gradient"
    rows = [("loss_gradient dR", r.loss_gradient(r.c, r.dR, None, n_params), UNS, skin_text(name)),
            ("loss_gradient dh", r.loss_gradient(None, None, r.dh, n_params), UNS, skin_text(name))]
    if td:
        rows += [("td_loss_gradient", r.td_loss_gradient(r.c, r.dR, None, n_params), UNS, skin_text(name))]
    if kind == "sf":
        rows += [("hessian_vectors", r.hessian_vectors(3, 0), UNS, skin_text("ta_hessian_vectors"))]
    if eam:
        rows += [("constant_gradient", r.constant_gradient(r.c, None, None, n_const), UNS, skin_text("ta_constant_gradient")),
                 ("set_nn_tables off", r("ta_set_nn_tables", 0), UNS, "ta_set_nn_tables: a skin-filtered batch is resident")]
        if n_params:   # (without networks ta_energy_gradient has nothing to do and says so before it looks)
            rows += [("energy_gradient", r.energy_gradient(r.c, n_params), UNS, skin_text("ta_energy_gradient"))]
    return rows


def assert_rows(kind, stage, rows):
    for what, (rc, msg), want_rc, fragment in rows:
        print(f"REFUSAL {kind} {stage} {what}: rc={rc} {msg!r}")
        assert rc == want_rc, (kind, stage, what, rc, msg)
        assert fragment is None or fragment in msg, (kind, stage, what, msg, fragment)


@pytest.mark.parametrize("kind", KINDS)
def test_refusal_matrix(lib, kind):
    frames = batch(kind, "small")
    N, F = sum(len(a) for a in frames), len(frames)
    with Engine(model(kind)) as eng:
        r = Raw(eng, N, F)
        rc, n_params = r.count("ta_param_count")
        assert rc == OK and (n_params > 0) == (kind != "eam")
        rc, n_filter = r.count("ta_filter_param_count")
        assert rc == OK and (n_filter > 0) == (kind == "grap-nn")
        rc, n_const = r.count("ta_constant_count")
        assert rc == (OK if kind in EAM or kind == "fs" else INV)
        knots = C.c_int32(-1)
        assert r("ta_filter_table_knots", C.byref(knots))[0] == OK and knots.value == 0
        assert_rows(kind, "no-batch", rows_without_batch(kind, r))
        info = eng.set_frames(frames)
        assert int(info.n_atoms) == N and int(info.n_frames) == F
        assert_rows(kind, "batch", rows_with_batch(kind, r, n_params, n_filter, n_const))
        if kind in SKIN_FILTERS:
            n_exact = int(info.n_pairs)
            eng.set_skin(0.5)
            assert int(eng.set_frames(frames).n_pairs) > n_exact
            assert_rows(kind, "skin", rows_on_skin(kind, r, n_params, n_const))


# ---- (b) call order on one handle ----------------------------------------------------------------------------------

def directions(eng):
    N, F = int(eng.info.n_atoms), int(eng.info.n_frames)
    rng = np.random.RandomState(7 + N)
    return rng.normal(size=F), rng.normal(size=(N, 3)), 0.05 * rng.normal(size=(F, 3, 3))


def hvp_unit(eng):
    """Three unit displacements that straddle two atoms, and the virial: one library call (the wrapper does all 3 N)."""
    N, F = int(eng.info.n_atoms), int(eng.info.n_frames)
    dF, dW = np.zeros((3, N, 3)), np.zeros((3, F, 3, 3))
    eng._check(eng._lib.ta_hessian_vectors(eng._handle, 3, 3 * (N // 2) + 2, NULL, NULL, _lib.as_dp(dF), _lib.as_dp(dW)))
    return dF, dW


def hvp_directions(eng):
    _, dR, dh = directions(eng)
    return eng.hessian_vectors(dR=np.stack([dR, -0.5 * dR[::-1]]), dh=np.stack([dh, 2.0 * dh[::-1]]), want_virial=True)


def td_full(eng):
    c, dR, dh = directions(eng)
    return eng.td_loss_gradient(c, 0.5 * c, -c, dR, dh, return_tangent=True)


def loss_both(eng):
    c, dR, dh = directions(eng)
    return eng.loss_gradient(c, dR, dh, return_tangent=True)


CALLS = {
    "energy_gradient": lambda e: e.energy_gradient(directions(e)[0]),
    "loss_gradient dR": lambda e: e.loss_gradient(directions(e)[0], directions(e)[1]),
    "loss_gradient dR alone": lambda e: e.loss_gradient(None, directions(e)[1]),
    "loss_gradient dh alone": lambda e: e.loss_gradient(None, None, directions(e)[2]),
    "loss_gradient both": lambda e: e.loss_gradient(*directions(e)),
    "loss_gradient both, tangent": loss_both,
    "hessian_vectors unit": hvp_unit,
    "hessian_vectors dR dh": hvp_directions,
    "grap_loss_gradient energy": lambda e: e.grap_loss_gradient(directions(e)[0]),
    "grap_loss_gradient both": lambda e: e.grap_loss_gradient(*directions(e)),
    "td_loss_gradient U alone": lambda e: e.td_loss_gradient(None, directions(e)[0]),
    "td_loss_gradient all, tangent": td_full,
    "constant_gradient energy": lambda e: e.constant_gradient(directions(e)[0]),
    "constant_gradient dR": lambda e: e.constant_gradient(directions(e)[0], directions(e)[1]),
    "constant_gradient dh alone": lambda e: e.constant_gradient(None, None, directions(e)[2]),
}
# smallest need of the shared buffers first; consecutive calls need different sizes of them
DESCRIPTOR_ORDER = ["energy_gradient", "loss_gradient dR", "loss_gradient dh alone", "hessian_vectors unit",
                    "hessian_vectors dR dh", "loss_gradient both, tangent"]
EAM_ORDER = ["constant_gradient energy", "constant_gradient dR", "energy_gradient", "loss_gradient dR alone",
             "constant_gradient dh alone", "loss_gradient both"]
ORDER = {
    "sf": DESCRIPTOR_ORDER,
    "grap-pexp": DESCRIPTOR_ORDER,
    "grap-nn": ["energy_gradient", "loss_gradient dR", "loss_gradient dh alone", "hessian_vectors unit",
                "grap_loss_gradient energy", "grap_loss_gradient both", "loss_gradient both, tangent"],
    "td": ["energy_gradient", "td_loss_gradient U alone", "loss_gradient dR", "td_loss_gradient all, tangent"],
    "eam": EAM_ORDER + ["hessian_vectors dR dh", "hessian_vectors unit"],
    "eam-nn": EAM_ORDER + ["hessian_vectors dR dh", "hessian_vectors unit"],
    # a weight or constant gradient leaves the pair networks exact, where second derivatives are refused
    "eam-nn-pair": EAM_ORDER,
}
# The kinds whose entry points reproduce a fresh handle's arrays bit for bit. The angular symmetry functions ("sf",
# "td") sum with floating-point atomics and differ in the last bits (up to 5e-15 on gradients of 30).
BITWISE = ("grap-pexp", "grap-nn", "eam", "eam-nn")


def arrays(out):
    return [np.asarray(a) for a in (out if isinstance(out, tuple) else (out,))]


@functools.lru_cache(maxsize=None)
def fresh(kind, which, name):
    """The entry point as the first call on a handle of its own: the reference, computed once."""
    with Engine(model(kind)) as eng:
        eng.set_frames(batch(kind, which))
        return arrays(CALLS[name](eng))


def assert_same(kind, tag, name, got, ref):
    for k, (g, r) in enumerate(zip(arrays(got), ref)):
        assert g.shape == r.shape
        if r.size == 0:   # a model without networks has no weight gradient
            assert kind == "eam"
            continue
        dev, bound = np.abs(g - r).max(), 1e-12 * max(1.0, np.abs(r).max())
        print(f"ORDER {kind} {tag} {name} [{k}]: |ref|max={np.abs(r).max():.3e} dev={dev:.3e} "
              f"bitwise={bool(np.array_equal(g, r))}")
        # (a model whose functions are all networks reads no constant: that gradient is zero)
        zero_by_design = kind == "eam-nn-pair" and name.startswith("constant_gradient")
        assert np.isfinite(g).all() and (np.abs(r).max() > 0.0 or zero_by_design), (kind, tag, name, k)
        assert dev <= bound, (kind, tag, name, k, dev, bound)
        if kind in BITWISE and not (kind == "grap-nn" and name.startswith("hessian_vectors")):
            assert np.array_equal(g, r), (kind, tag, name, k, dev)


@pytest.mark.parametrize("order", ["ascending", "descending"])
@pytest.mark.parametrize("kind", [k for k in KINDS if k != "fs"])
def test_call_order_on_one_handle(lib, kind, order):
    names = ORDER[kind] if order == "ascending" else ORDER[kind][::-1]
    refs = {name: fresh(kind, "small", name) for name in names}
    mid = names[len(names) // 2]
    ref_large = fresh(kind, "large", mid)
    with Engine(model(kind)) as eng:
        eng.set_frames(batch(kind, "small"))
        for name in names:
            if name == mid:   # a batch with more atoms, pairs and frames, then the first one again
                eng.set_frames(batch(kind, "large"))
                assert_same(kind, order + " large", name, CALLS[name](eng), ref_large)
                eng.set_frames(batch(kind, "small"))
            assert_same(kind, order, name, CALLS[name](eng), refs[name])
