"""
The EAM / ADP / eam/fs kernels (ta_eam.hip) build by build, against the oracle at fp64 bounds.

`eam_compute` and the nn-function setup of `eam_create` pick, per launch,
  * `eam_atom_kernel<OTHER, W, FS>` and, with forces folded into one pass per centre,
    `eam_force_kernel<OTHER, W, FS>` or `adp_force_kernel<OTHER, W>`; otherwise `eam_pair_kernel<OTHER, FS>`
    and the shared force gather. OTHER: an element whose analytic functions are sutton90, Be/1 or grimes.
    W (lanes per atom): 16 for EAM and eam/fs, for ADP 32 below 32768 atoms and 16 at or above;
  * the atom kernel's geometry mode: 1 = pair records written by `eam_geom_kernel` (exact nn pair
    functions), 2 = D computed and not stored (every other model); the folded force kernels recompute D;
  * for exact nn pair functions (tables off): `eam_nn_pair_fast_kernel<ACT, NT, FS>` when every pair network
    is 1 -> H1 -> H2 -> 1 with one padded H2 <= 64 (NT = H2 / 16) and an LDS image <= 64 KB,
    `eam_nn_pair_1h_kernel<ACT, FS>` when every one is 1 -> H -> 1, else (or under TA_EAM_NN_GENERIC) the
    generic tile `eam_nn_pair_kernel`; ACT is softplus or "other" (-1, the activation read at run time);
  * `eam_nn_embed_kernel<FS>` for embedding networks.
`eam_builds` restates these rules on the CPU; every row asserts that its model and batch select the builds
the row is named after, and `test_rows_cover_every_build` that the rows together reach every build the
restatement can produce (`reachable_builds`).

Combinations that cannot be reached: eam/fs with OTHER (EamFsNN has no analytic functions, eam.py
`EamFsNN._setup_potentials`, and `by_model` tests `fs` before `other`); eam/fs ADP (`adp_force_kernel` has
no FS parameter: ADP and eam/fs are different model kinds).

Bounds: north_star (1e-6 eV, 1e-5 eV/A) and what fp64 kernels owe an fp64 reference: energies to
1e-9 x max(1, |E|), forces to 1e-9 x max(1, max|F|), virial to 1e-8 x max(1, max|W|) (`check` of
test_gpu_sf_dispatch), for analytic functions, spline tables and exact networks. The reference is the oracle
(oracle/eam.py) for eam/alloy and ADP and its eam/fs restatement (tests/fs_reference.py) for eam/fs. The
Hermite tables the library builds from nn pair functions are another function: rows that use them are held
to north_star against the reference and to 1e-9 eV / 1e-8 eV/A / 1e-7 eV against the exact networks.

The library reads TA_EAM_NN_TABLES / TA_EAM_NN_GENERIC when a handle is created: the rows under them set the
switch before their engine exists and delete it after.
"""
import functools
import tempfile
from collections import namedtuple

import numpy as np
import pytest

from tests.fs_reference import fs_evaluate
from tests.helpers import fcc, golden_setfl, hcp, make_eam, oracle_eam_eval
from tests.test_gpu_sf_dispatch import E_REL, E_TOL, F_REL, F_TOL, W_REL, W_TOL, check, drop
from tests.test_gpu_sf import _alloy

gpu = pytest.mark.gpu

E, F, V, A = 1, 2, 4, 8          # TA_WANT_ENERGY / FORCES / VIRIAL / ATOMIC
FULL = E | F | V | A
FAST_ROWS, ONE_H_PAIRS = 2048 * 4 * 16, 4096 * 256   # grid caps of the fast and 1h nn pair kernels
ADP_NARROW = 32768                                     # ADP: W = 16 at or above this many atoms


# -- the selection rules, restated ---------------------------------------------------------------------------

def _family(nn):
    from tensoralloy_amd.eam import AdpNN, EamFsNN
    return "fs" if isinstance(nn, EamFsNN) else "adp" if isinstance(nn, AdpNN) else "alloy"


def pair_nets(nn):
    """Layer widths [H1, ..., 1] of every nn PAIR function (rho, phi, dipole, quadrupole; not embed)."""
    out = []
    for slot in nn.nn_functions():
        if slot is not None and slot[1] != "embed":
            out.append([w.shape[1] for w, _ in nn.weights[slot[0]][slot[1]]])
    return out


def nn_pair_class(nn, generic_env=False):
    """eam_create (ta_eam.hip, `add` and the choice after it): ("fast", act, NT), ("1h", act), ("generic",)
    or None (no nn pair function)."""
    nets = pair_nets(nn)
    if not nets:
        return None
    act = "softplus" if nn._activation.lower() == "softplus" else "other"
    pad = lambda n: (n + 15) // 16 * 16
    fast = all(len(s) == 3 and pad(s[1]) <= 64 for s in nets) and len({pad(s[1]) for s in nets}) == 1
    if fast:
        h2 = pad(nets[0][1])
        s2 = h2 + 16 if h2 % 32 == 0 else h2
        lds = max((2 * pad(s[0]) + pad(s[0]) * s2 + 2 * h2 + 2) * 8 for s in nets)
        if lds <= 64 * 1024 and not generic_env:
            return ("fast", act, h2 // 16)
    if all(len(s) == 2 for s in nets) and not generic_env:
        return ("1h", act)
    return ("generic",)


def eam_builds(nn, n_atoms, want=FULL, tables=True, env=None):
    """The kernel builds (and path arguments) one evaluation of `nn` on a batch of `n_atoms` launches
    (`eam_compute`). `tables`: what `set_nn_tables` left on; `env`: the library's switches."""
    env = env or {}
    fam = _family(nn)
    fs = fam == "fs"
    other = not fs and any(k != "zjw" for k in nn._el_kind.values())
    cls = nn_pair_class(nn, "TA_EAM_NN_GENERIC" in env)
    tables = tables and not env.get("TA_EAM_NN_TABLES", "1").startswith("0")
    nets_on = cls is not None and not tables
    W = 16 if fam != "adp" or n_atoms >= ADP_NARROW else 32
    want_f = bool(want & (F | V))
    fold = want_f and not nets_on
    b = lambda *a: ",".join(str(x).lower() for x in a)
    out = {f"eam_atom_kernel<{b(other, W, fs)}>", f"geom_done={1 if nets_on else 2}"}
    if nets_on:
        if cls[0] == "fast":
            out.add(f"eam_nn_pair_fast_kernel<{cls[1]},{cls[2]},{b(fs)}>")
        elif cls[0] == "1h":
            out.add(f"eam_nn_pair_1h_kernel<{cls[1]},{b(fs)}>")
        else:
            out.add(f"eam_nn_pair_kernel<{b(fs)}>")
    if any(s is not None and s[1] == "embed" for s in nn.nn_functions()):
        out.add(f"eam_nn_embed_kernel<{b(fs)}>")
    if want_f:
        if fold and fam == "adp":
            out.add(f"adp_force_kernel<{b(other, W)}>")
        elif fold:
            out.add(f"eam_force_kernel<{b(other, W, fs)}>")
        else:
            out |= {f"eam_pair_kernel<{b(other, fs)}>", "force_gather"}
    return out


def reachable_builds():
    """Every build `eam_compute` can launch (see the module docstring for the unreachable ones)."""
    b = lambda *a: ",".join(str(x).lower() for x in a)
    combos = [(False, False), (True, False), (False, True)]        # (OTHER, FS)
    out = {"geom_done=1", "geom_done=2", "force_gather"}
    for o, fs in combos:
        out |= {f"eam_pair_kernel<{b(o, fs)}>", f"eam_atom_kernel<{b(o, 16, fs)}>", f"eam_force_kernel<{b(o, 16, fs)}>"}
    for o in (False, True):                                        # ADP (never eam/fs)
        out.add(f"eam_atom_kernel<{b(o, 32, False)}>")
        for W in (16, 32):
            out.add(f"adp_force_kernel<{b(o, W)}>")
    for fs in (False, True):
        out |= {f"eam_nn_pair_kernel<{b(fs)}>", f"eam_nn_embed_kernel<{b(fs)}>"}
        for act in ("softplus", "other"):
            out.add(f"eam_nn_pair_1h_kernel<{act},{b(fs)}>")
            for nt in (1, 2, 3, 4):
                out.add(f"eam_nn_pair_fast_kernel<{act},{nt},{b(fs)}>")
    return out


# -- models and frames ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _tmp():
    return tempfile.mkdtemp(prefix="eam_dispatch_")


def mendelev():
    from tensoralloy_amd import UniversalTransformer
    from tensoralloy_amd.eam import EamFsNN
    nn = EamFsNN.from_setfl(golden_setfl("Mendelev_Al_Fe_thinned.fs.eam", _tmp()))
    nn.attach_transformer(UniversalTransformer(["Al", "Fe"], rcut=6.5, angular=False))
    return nn


def fs_nn(hidden=None, activation=None, elements=("Al", "Fe"), rcut=6.0, seed=5, out_scale=0.05):
    from tensoralloy_amd import UniversalTransformer
    from tensoralloy_amd.eam import EamFsNN
    nn = EamFsNN(list(elements), hidden_sizes=hidden, activation=activation)
    nn.attach_transformer(UniversalTransformer(list(elements), rcut=rcut, angular=False))
    nn.initialize(seed=seed, bias_scale=0.1)
    for sec in nn.weights.values():
        for layers in sec.values():
            w, bias = layers[-1]
            layers[-1] = (w * out_scale, bias)
    return nn


AG_ADP = {"AgAg": dict(zip(["d1", "d2", "d3", "q1", "q2", "q3", "h", "rc"],
                           [0.0044657, -1.3702, -0.09611, 6.4502, 0.02608, -6.0208, 3.323, 5.168]))}


def adp_other():
    """ADP with a sutton90 element (MishinH dipole / quadrupole with the Ni-Ni constants)."""
    pots = {"Ag": {"rho": "sutton90", "embed": "sutton90"},
            "AgAg": {"phi": "sutton90", "dipole": "mishinh", "quadrupole": "mishinh"}}
    return make_eam(["Ag"], 7.0, adp=True, potential=pots, parameters=AG_ADP)


def other_nn_pair():
    """An OTHER element whose density is a network: exact pair networks with the OTHER kernels. The density
    network's output is flipped to positive densities (sutton90's F = -sqrt(rho))."""
    pots = {"Ag": {"rho": "nn", "embed": "sutton90"}, "AgAg": {"phi": "sutton90"}}
    nn = make_eam(["Ag"], 7.0, potential=pots, hidden_sizes=[32, 32])
    w, bias = nn.weights["Ag"]["rho"][-1]
    nn.weights["Ag"]["rho"][-1] = (-w, None if bias is None else -bias)
    return nn


def ag(rep=(2, 2, 2), seed=3):
    return [fcc("Ag", a=4.09, rep=rep, jitter=0.08, seed=seed)]


def nimo(seed=3):
    return [_alloy(["Ni", "Ni", "Mo"], rep=(2, 2, 2), seed=seed)]


def alfe(seed=3):
    return [_alloy(["Al", "Fe", "Fe"], rep=(2, 2, 2), a=3.6, seed=seed)]


def bcc_fe(rep=(3, 3, 3), seed=7):
    from tensoralloy_amd import Atoms
    a = 2.855312
    base = np.array([[0, 0, 0], [.5, .5, .5]]) * a
    pts = np.array([base + np.array([x, y, z]) * a
                    for x in range(rep[0]) for y in range(rep[1]) for z in range(rep[2])]).reshape(-1, 3)
    rng = np.random.RandomState(seed)
    pts = pts + rng.normal(0.0, 0.05, pts.shape)
    syms = ["Fe"] * len(pts)
    for k in rng.choice(len(pts), len(pts) // 5, replace=False):
        syms[k] = "Al"
    return Atoms(symbols=syms, positions=pts, cell=np.diag(np.array(rep) * a), pbc=True)


def reference(nn, atoms):
    return fs_evaluate(nn, atoms) if _family(nn) == "fs" else oracle_eam_eval(nn, atoms)


def nn_models():
    """(id, model, frames) of every nn pair class: fast for NT = 1..4 with softplus and tanh, 1h, generic by
    its LDS image (H1 = 128, H2 = 64: 83 KB), for eam/alloy and eam/fs."""
    out = []
    for act in ("softplus", "tanh"):
        for nt in (1, 2, 3, 4):
            hs = [32, 16 * nt]
            out.append((f"fast-{act}-nt{nt}", make_eam(["Ni"], 6.0, potential=None, hidden_sizes=hs, activation=act),
                        [fcc(rep=(2, 2, 2), seed=nt)]))
            out.append((f"fs-fast-{act}-nt{nt}", fs_nn(hs, act, seed=nt), alfe(seed=nt)))
        out.append((f"1h-{act}", make_eam(["Mo", "Ni"], 6.0, potential=None, hidden_sizes=[40], activation=act),
                    nimo()))
        out.append((f"fs-1h-{act}", fs_nn([40], act), alfe()))
    out.append(("generic-lds", make_eam(["Ni"], 6.0, potential=None, hidden_sizes=[128, 64]), [fcc(rep=(2, 2, 2))]))
    out.append(("fs-generic-lds", fs_nn([128, 64]), alfe()))
    return out


Row = namedtuple("Row", "id targets model frames tables")

# In-process rows (the library's default switches). `targets`: builds the row is named after.
ROWS = [
    Row("alloy-zjw04", ("eam_atom_kernel<false,16,false>", "eam_force_kernel<false,16,false>", "geom_done=2"),
        lambda: make_eam(["Mo", "Ni"], 6.0), lambda: nimo() + nimo(seed=9), True),
    Row("alloy-sutton90", ("eam_atom_kernel<true,16,false>", "eam_force_kernel<true,16,false>"),
        lambda: make_eam(["Ag"], 8.0, potential="sutton90"), ag, True),
    Row("alloy-be1", ("eam_atom_kernel<true,16,false>", "eam_force_kernel<true,16,false>"),
        lambda: make_eam(["Be"], 5.0, potential="Be/1"), lambda: [hcp(rep=(3, 3, 3), jitter=0.05, seed=4)], True),
    Row("alloy-grimes", ("eam_atom_kernel<true,16,false>", "eam_force_kernel<true,16,false>"),
        lambda: make_eam(["Pu"], 6.0, potential="grimes"), lambda: [fcc("Pu", a=4.6, rep=(2, 2, 2), jitter=0.08)],
        True),
    Row("fs-spline", ("eam_atom_kernel<false,16,true>", "eam_force_kernel<false,16,true>"),
        mendelev, lambda: [bcc_fe()], True),
    Row("adp-zjw04", ("eam_atom_kernel<false,32,false>", "adp_force_kernel<false,32>"),
        lambda: make_eam(["Mo", "Ni"], 6.0, adp=True), nimo, True),
    Row("adp-sutton90", ("eam_atom_kernel<true,32,false>", "adp_force_kernel<true,32>"), adp_other, ag, True),
    Row("alloy-nn-exact", ("eam_pair_kernel<false,false>", "force_gather", "geom_done=1",
                           "eam_nn_pair_fast_kernel<softplus,2,false>", "eam_nn_embed_kernel<false>"),
        lambda: make_eam(["Mo", "Ni"], 6.0, potential=None), nimo, False),
    Row("other-nn-exact", ("eam_pair_kernel<true,false>", "eam_atom_kernel<true,16,false>"), other_nn_pair, ag,
        False),
    Row("fs-nn-exact", ("eam_pair_kernel<false,true>", "eam_nn_embed_kernel<true>",
                        "eam_nn_pair_fast_kernel<softplus,2,true>"), fs_nn, alfe, False),
    Row("adp-nn-exact", ("eam_pair_kernel<false,false>", "eam_atom_kernel<false,32,false>",
                         "eam_nn_pair_fast_kernel<softplus,1,false>"),
        lambda: make_eam(["Mo", "Ni"], 6.0, adp=True, potential=None, hidden_sizes=[32, 16]), nimo, False),
]
for _id, _nn, _frames in nn_models():
    _cls = nn_pair_class(_nn)
    _fs = "true" if _id.startswith("fs-") else "false"
    _t = {"fast": lambda c: f"eam_nn_pair_fast_kernel<{c[1]},{c[2]},{_fs}>",
          "1h": lambda c: f"eam_nn_pair_1h_kernel<{c[1]},{_fs}>",
          "generic": lambda c: f"eam_nn_pair_kernel<{_fs}>"}[_cls[0]](_cls)
    ROWS.append(Row(_id, (_t,), lambda m=_nn: m, lambda f=_frames: f, False))


def nn_switch_cases():
    """Exact-network models for TA_EAM_NN_TABLES=0 (with and without TA_EAM_NN_GENERIC): fast-, 1h- and
    generic-shaped networks, eam/alloy and eam/fs."""
    return [("alloy-fast", make_eam(["Mo", "Ni"], 6.0, potential=None), nimo(seed=21)),
            ("alloy-1h", make_eam(["Ni"], 6.0, potential=None, hidden_sizes=[24], activation="tanh"),
             [fcc(rep=(2, 2, 2), seed=22)]),
            ("fs-fast", fs_nn(), alfe(seed=23)),
            ("fs-1h", fs_nn([40]), alfe(seed=24)),
            ("adp-fast", make_eam(["Mo", "Ni"], 6.0, adp=True, potential=None, hidden_sizes=[32, 16]), nimo(seed=25))]


SWITCHES = [("nn_switch_cases", {"TA_EAM_NN_TABLES": "0"}),
            ("nn_switch_cases", {"TA_EAM_NN_TABLES": "0", "TA_EAM_NN_GENERIC": "1"})]


def _n(frames):
    return sum(len(a) for a in frames)


# -- CPU: the rows and the restatement -------------------------------------------------------------------------

def test_restatement_of_the_nn_classes():
    """CPU: the LDS formula's edges: H2 = 64 after H1 = 128 exceeds 64 KB, after H1 = 96 it does not;
    mixed H2 or depths leave the fast kernel."""
    mk = lambda hs: make_eam(["Ni"], 6.0, potential=None, hidden_sizes=hs)
    assert nn_pair_class(mk([128, 64])) == ("generic",)
    assert nn_pair_class(mk([96, 64])) == ("fast", "softplus", 4)
    assert nn_pair_class(mk([64, 32])) == ("fast", "softplus", 2)
    assert nn_pair_class(mk([64, 33])) == ("fast", "softplus", 3)      # H2 padded to 48
    assert nn_pair_class(mk([64, 65])) == ("generic",)                 # H2 padded to 80
    assert nn_pair_class(mk([40])) == ("1h", "softplus")
    assert nn_pair_class(mk([40]), generic_env=True) == ("generic",)
    assert nn_pair_class(mk([16, 16, 16])) == ("generic",)
    hs = {"Ni": {"rho": [16, 16]}, "NiNi": {"phi": [16, 32]}}
    assert nn_pair_class(mk(hs)) == ("generic",)
    assert nn_pair_class(make_eam(["Ni"], 6.0)) is None


def test_rows_cover_every_build():
    """CPU: every row reaches the builds it is named after, and the rows together (in-process rows, the
    switches, the want subsets and the scale rows) reach every build `eam_compute` can launch."""
    seen = set()
    for row in ROWS:
        frames = row.frames()
        got = eam_builds(row.model(), _n(frames), FULL, row.tables)
        assert set(row.targets) <= got, (row.id, set(row.targets) - got)
        seen |= got
    for func, env in SWITCHES:
        for name, nn, frames in globals()[func]():
            seen |= eam_builds(nn, _n(frames), FULL, True, env)
    for fam, (model, frames) in WANT_MODELS.items():
        for want in WANTS:
            seen |= eam_builds(model(), _n(frames()), want)
    seen |= eam_builds(make_eam(["Ni"], 6.0, adp=True), ADP_NARROW)
    seen |= eam_builds(adp_other(), ADP_NARROW)
    assert seen == reachable_builds(), (sorted(reachable_builds() - seen), sorted(seen - reachable_builds()))


def test_switch_rows_select_their_builds():
    """CPU: what each switch changes, on the nn switch cases."""
    cases = {name: (nn, frames) for name, nn, frames in nn_switch_cases()}
    nn, fr = cases["alloy-1h"]
    assert "eam_nn_pair_1h_kernel<other,false>" in eam_builds(nn, _n(fr), env={"TA_EAM_NN_TABLES": "0"})
    assert "eam_nn_pair_kernel<false>" in eam_builds(nn, _n(fr), env={"TA_EAM_NN_TABLES": "0",
                                                                      "TA_EAM_NN_GENERIC": "1"})
    assert "eam_force_kernel<false,16,false>" in eam_builds(nn, _n(fr))


def test_w_boundary_of_the_adp_rows():
    nn = make_eam(["Ni"], 6.0, adp=True)
    assert "adp_force_kernel<false,32>" in eam_builds(nn, ADP_NARROW - 1)
    assert "adp_force_kernel<true,16>" in eam_builds(adp_other(), ADP_NARROW)
    assert "adp_force_kernel<false,16>" in eam_builds(nn, ADP_NARROW)
    assert "eam_force_kernel<false,16,false>" in eam_builds(make_eam(["Ni"], 6.0), 10)


# -- GPU: the rows --------------------------------------------------------------------------------------------

def _run(nn, frames, tables, want=FULL):
    from tensoralloy_amd import Engine
    with Engine(nn) as eng:
        if not tables:
            eng.set_nn_tables(False)
        res = eng.evaluate(frames, want=want)
        info = (int(eng.info.n_atoms), int(eng.info.n_pairs))
    return res, info


def tables_check(t, x, tag):
    """Hermite tables against the exact networks on the same engine."""
    dev = dict(E=abs(t["energy"] - x["energy"]), F=np.abs(t["forces"] - x["forces"]).max(),
               W=np.abs(t["virial"] - x["virial"]).max())
    print(f"DEV {tag}/tables-vs-exact " + " ".join(f"{k}={v:.2e}" for k, v in dev.items()))
    assert dev["E"] < 1e-9 and dev["F"] < 1e-8 and dev["W"] < 1e-7, (tag, dev)


@gpu
@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_dispatch_row(lib, row):
    nn, frames = row.model(), row.frames()
    assert set(row.targets) <= eam_builds(nn, _n(frames), FULL, row.tables), row.id
    res, _ = _run(nn, frames, row.tables)
    for k, (atoms, r) in enumerate(zip(frames, res)):
        check(r, reference(nn, atoms), f"{row.id}/frame{k}", descriptors=False)
    if not row.tables and nn_pair_class(nn) is not None:   # the same networks through their tables
        tab, _ = _run(nn, frames, True)
        for k, (atoms, t, x) in enumerate(zip(frames, tab, res)):
            o = reference(nn, atoms)
            assert abs(t["energy"] - o["energy"]) < E_TOL and np.abs(t["forces"] - o["forces"]).max() < F_TOL
            assert np.abs(t["virial"] - o["virial"]).max() < W_TOL
            tables_check(t, x, f"{row.id}/frame{k}")


@gpu
@pytest.mark.parametrize("func,env", SWITCHES, ids=["-".join(f"{k}={v}" for k, v in e.items()) for _, e in SWITCHES])
def test_switches_set_before_the_engine(lib, monkeypatch, func, env):
    from tensoralloy_amd import Engine
    for name, nn, frames in globals()[func]():
        for var, value in env.items():
            monkeypatch.setenv(var, value)
        eng = Engine(nn)
        for var in env:
            monkeypatch.delenv(var)
        with eng:
            res = eng.evaluate(frames, descriptors=False)
        builds = eam_builds(nn, _n(frames), FULL, True, env)
        tag = "-".join(f"{k}={v}" for k, v in env.items())
        for k, (atoms, r) in enumerate(zip(frames, res)):
            check(r, reference(nn, atoms), f"{tag}/{name}/frame{k}:" + "+".join(
                sorted(x for x in builds if "<" in x)), descriptors=False)


# -- want subsets ----------------------------------------------------------------------------------------------

WANTS = [E, E | A, E | F, E | V, FULL]
WANT_MODELS = {"alloy": (lambda: make_eam(["Mo", "Ni"], 6.0), lambda: nimo(seed=31)),
               "alloy-other": (lambda: make_eam(["Be"], 5.0, potential="Be/1"), lambda: [hcp(seed=32)]),
               "adp": (lambda: make_eam(["Mo", "Ni"], 6.0, adp=True), lambda: nimo(seed=33)),
               "fs": (mendelev, lambda: [bcc_fe(seed=34)]),
               "alloy-nn-exact": (lambda: make_eam(["Mo", "Ni"], 6.0, potential=None, hidden_sizes=[24, 16]),
                                  lambda: nimo(seed=35))}


@gpu
@pytest.mark.parametrize("fam", list(WANT_MODELS))
def test_want_subsets(lib, fam):
    """E, E|atomic, E|F, E|virial and the full request against the reference, and each subset against the full
    request to 1e-12 relative (energy-only runs the atom kernel without pair records, geom_done = 2)."""
    model, frames = WANT_MODELS[fam]
    nn, frames = model(), frames()
    tables = nn_pair_class(nn) is None
    assert "geom_done=2" in eam_builds(nn, _n(frames), E, tables) or not tables
    full, _ = _run(nn, frames, tables)
    for want in WANTS:
        res, _ = _run(nn, frames, tables, want)
        for k, (atoms, r, f) in enumerate(zip(frames, res, full)):
            o = reference(nn, atoms)
            tag = f"want{want}/{fam}/frame{k}"
            dev = {"E": abs(r["energy"] - o["energy"])}
            assert abs(r["energy"] - f["energy"]) <= 1e-12 * max(1.0, abs(f["energy"])), tag
            if want & A:
                dev["e"] = np.abs(r["atomic"] - o["atomic"]).max()
                assert np.abs(r["atomic"] - f["atomic"]).max() <= 1e-12 * max(1.0, np.abs(f["atomic"]).max()), tag
            else:
                assert "atomic" not in r, tag
            if want & (F | V):
                dev["F"] = np.abs(r["forces"] - o["forces"]).max()
                dev["W"] = np.abs(r["virial"] - o["virial"]).max()
                assert np.abs(r["forces"] - f["forces"]).max() <= 1e-12 * max(1.0, np.abs(f["forces"]).max()), tag
                assert np.abs(r["virial"] - f["virial"]).max() <= 1e-12 * max(1.0, np.abs(f["virial"]).max()), tag
            print(f"DEV {tag} " + " ".join(f"{k}={v:.2e}" for k, v in dev.items()))
            e_scale = max(1.0, abs(o["energy"]))
            assert dev["E"] < E_TOL and dev["E"] < E_REL * e_scale, (tag, dev)
            if "e" in dev:
                assert dev["e"] < E_TOL and dev["e"] < E_REL * e_scale, (tag, dev)
            if "F" in dev:
                assert dev["F"] < F_TOL and dev["F"] < F_REL * max(1.0, np.abs(o["forces"]).max()), (tag, dev)
                assert dev["W"] < W_TOL and dev["W"] < W_REL * max(1.0, np.abs(o["virial"]).max()), (tag, dev)


@gpu
def test_energy_only_through_the_calculator(lib, tmp_path):
    """`TensorAlloyCalculator.get_potential_energy` asks for ENERGY | ATOMIC only (calculator.py)."""
    from tensoralloy_amd import TensorAlloyCalculator
    for k, (model, frames) in enumerate((WANT_MODELS["alloy"], WANT_MODELS["adp"])):
        nn, atoms = model(), frames()[0]
        path = str(tmp_path / f"m{k}.pb")
        nn.export(path)
        calc = TensorAlloyCalculator(path)
        e = calc.get_potential_energy(atoms)
        o = oracle_eam_eval(nn, atoms)
        print(f"DEV calculator-energy/{k} E={abs(e - o['energy']):.2e}")
        assert abs(e - o["energy"]) < min(E_TOL, E_REL * max(1.0, abs(o["energy"])))


# -- the element limit -----------------------------------------------------------------------------------------

@gpu
def test_five_elements_and_the_refusal_of_six(lib):
    from tensoralloy_amd import Engine
    els = ["Al", "Co", "Cu", "Fe", "Ni"]
    nn = make_eam(els, 6.0)
    frames = [_alloy(els, rep=(2, 2, 3), a=3.6, seed=41), _alloy(els, rep=(3, 3, 3), a=3.55, seed=42)]
    res, _ = _run(nn, frames, True)
    for k, (atoms, r) in enumerate(zip(frames, res)):
        check(r, oracle_eam_eval(nn, atoms), f"5el/frame{k}", descriptors=False)
    with pytest.raises(ValueError, match="at most 5 elements"):
        Engine(make_eam(els + ["Mo"], 6.0))


# -- scale rows ------------------------------------------------------------------------------------------------

def ni_4000(seed, jitter=0.05):
    return fcc(rep=(10, 10, 10), seed=seed, jitter=jitter)


@gpu
@pytest.mark.parametrize("hidden,nt", [([32, 16], 1), ([24, 64], 4)], ids=["nt1", "nt4"])
def test_fast_kernel_beyond_one_grid_stride(lib, hidden, nt):
    """Exact networks over more than 2048 x 4 x 16 pair rows (the fast kernel's grid cap): ~360k pairs of the
    4000-atom Ni frame at rc 6.5; then its tables against the exact run."""
    nn = make_eam(["Ni"], 6.5, potential=None, hidden_sizes=hidden)
    frames = [ni_4000(51)]
    assert f"eam_nn_pair_fast_kernel<softplus,{nt},false>" in eam_builds(nn, 4000, FULL, False)
    exact, (_, n_pairs) = _run(nn, frames, False)
    assert n_pairs > FAST_ROWS, n_pairs
    o = oracle_eam_eval(nn, frames[0])
    check(exact[0], o, f"fast-nt{nt}-{n_pairs}pairs", descriptors=False)
    tab, _ = _run(nn, frames, True)
    assert abs(tab[0]["energy"] - o["energy"]) < E_TOL and np.abs(tab[0]["forces"] - o["forces"]).max() < F_TOL
    tables_check(tab[0], exact[0], f"fast-nt{nt}")


@gpu
def test_1h_kernel_beyond_one_grid_stride(lib):
    """Exact 1 -> H -> 1 networks over more than 4096 x 256 pairs: four distinct 4000-atom frames."""
    nn = make_eam(["Ni"], 6.5, potential=None, hidden_sizes=[40])
    frames = [ni_4000(60 + k, 0.03 + 0.01 * k) for k in range(4)]
    assert "eam_nn_pair_1h_kernel<softplus,false>" in eam_builds(nn, _n(frames), FULL, False)
    res, (_, n_pairs) = _run(nn, frames, False)
    assert n_pairs > ONE_H_PAIRS, n_pairs
    for k, (atoms, r) in enumerate(zip(frames, res)):
        check(r, oracle_eam_eval(nn, atoms), f"1h-{n_pairs}pairs/frame{k}", descriptors=False)


@gpu
def test_64_frame_batch(lib):
    """The README's 64-frame Zjw04 batch (4000-atom Ni frames, rc 6.5): 64 distinct frames, each against the
    oracle."""
    nn = make_eam(["Ni"], 6.5)
    frames = [ni_4000(100 + k, 0.02 + 0.001 * k) for k in range(64)]
    assert "eam_force_kernel<false,16,false>" in eam_builds(nn, _n(frames))
    res, _ = _run(nn, frames, True)
    energies = [r["energy"] for r in res]
    assert len(set(energies)) == 64
    for k, (atoms, r) in enumerate(zip(frames, res)):
        check(r, oracle_eam_eval(nn, atoms), f"64frames/frame{k}", descriptors=False)


@gpu
def test_adp_at_the_lane_boundary(lib):
    """ADP batches of 32767 atoms (W = 32) and 32768 atoms (W = 16): two 16384-atom frames, the second one
    atom short in the smaller batch."""
    nn = make_eam(["Ni"], 6.0, adp=True)
    a = fcc(rep=(16, 16, 16), seed=71, jitter=0.06)
    b = fcc(rep=(16, 16, 16), seed=72, jitter=0.04)
    for frames, W in (([a, drop(b, 1)], 32), ([a, b], 16)):
        assert _n(frames) == ADP_NARROW - (W == 32)
        assert f"adp_force_kernel<false,{W}>" in eam_builds(nn, _n(frames))
        res, _ = _run(nn, frames, True)
        for k, (atoms, r) in enumerate(zip(frames, res)):
            check(r, oracle_eam_eval(nn, atoms), f"adp-{_n(frames)}atoms-W{W}/frame{k}", descriptors=False)


@gpu
def test_adp_other_at_the_narrow_width(lib):
    """ADP with a sutton90 element at 32768 atoms (W = 16): two 16384-atom Ag frames."""
    nn = adp_other()
    frames = [fcc("Ag", a=4.09, rep=(16, 16, 16), jitter=0.06, seed=81),
              fcc("Ag", a=4.09, rep=(16, 16, 16), jitter=0.04, seed=82)]
    assert _n(frames) == ADP_NARROW
    assert {"eam_atom_kernel<true,16,false>", "adp_force_kernel<true,16>"} <= eam_builds(nn, _n(frames))
    res, _ = _run(nn, frames, True)
    for k, (atoms, r) in enumerate(zip(frames, res)):
        check(r, oracle_eam_eval(nn, atoms), f"adp-other-{_n(frames)}atoms-W16/frame{k}", descriptors=False)
