"""GPU parity of the EAM / ADP kernels against the CPU oracle (oracle/eam.py)."""
import numpy as np
import pytest

from tests.helpers import fcc, golden_setfl, hcp, make_eam, oracle_eam_eval
from tests.test_gpu_sf import _alloy, E_TOL, F_TOL, W_TOL

pytestmark = pytest.mark.gpu


def _fp64(got, ref):
    """What fp64 kernels owe an fp64 reference (tests/test_gpu_eam_dispatch.py): energies to
    1e-9 x max(1, |E|), forces to 1e-9 x max(1, max|F|), virial to 1e-8 x max(1, max|W|)."""
    e_scale = max(1.0, abs(ref["energy"]))
    dev = dict(E=abs(got["energy"] - ref["energy"]), e=np.abs(got["atomic"] - ref["atomic"]).max(),
               F=np.abs(got["forces"] - ref["forces"]).max(initial=0.0),
               W=np.abs(got["virial"] - ref["virial"]).max())
    assert dev["E"] < 1e-9 * e_scale and dev["e"] < 1e-9 * e_scale, dev
    assert dev["F"] < 1e-9 * max(1.0, np.abs(ref["forces"]).max(initial=0.0)), dev
    assert dev["W"] < 1e-8 * max(1.0, np.abs(ref["virial"]).max()), dev


def _compare(nn, atoms_list):
    """GPU against the oracle at north_star's tolerances. Models with nn pair functions run twice:
    through the Hermite tables the library builds from the networks (the default for inference,
    `ta_set_nn_tables`) and with the networks evaluated exactly for every pair; the two must agree
    far inside the tolerances (the tables are an implementation of the same functions, not a model
    change): 1e-9 eV per structure, 1e-8 eV/A. Analytic functions, spline tables and exact networks
    are also held to the fp64 bounds of `_fp64`."""
    from tensoralloy_amd import Engine
    from tests.test_gpu_eam_dispatch import pair_nets
    tabulated = bool(pair_nets(nn))   # `res` went through the Hermite tables of nn pair functions
    with Engine(nn) as eng:
        res = eng.evaluate(atoms_list)
        eng.set_nn_tables(False)
        exact = eng.evaluate(atoms_list)
    for atoms, r, x in zip(atoms_list, res, exact):
        o = oracle_eam_eval(nn, atoms)
        for got in (r, x):
            assert abs(got["energy"] - o["energy"]) < E_TOL
            assert np.abs(got["atomic"] - o["atomic"]).max() < E_TOL
            assert np.abs(got["forces"] - o["forces"]).max() < F_TOL
            assert np.abs(got["virial"] - o["virial"]).max() < W_TOL
            assert np.abs(got["stress"] - o["stress_voigt"]).max() < 1e-8
        _fp64(x, o)
        if not tabulated:
            _fp64(r, o)
        assert abs(r["energy"] - x["energy"]) < 1e-9
        assert np.abs(r["forces"] - x["forces"]).max() < 1e-8
        assert np.abs(r["virial"] - x["virial"]).max() < 1e-7


def test_eam_ni(lib):
    _compare(make_eam(["Ni"], 6.5), [fcc(rep=(3, 3, 3)), fcc(rep=(2, 2, 2), a=3.3, seed=5)])


def test_eam_ni_rc6(lib):
    _compare(make_eam(["Ni"], 6.0), [fcc(rep=(2, 2, 2), a=3.52, jitter=0.1)])


def test_eam_binary_ni_mo(lib):
    _compare(make_eam(["Ni", "Mo"], 6.5), [_alloy(["Ni", "Ni", "Ni", "Mo"], rep=(2, 2, 3))])


def test_eam_ternary(lib):
    _compare(make_eam(["Al", "Cu", "Ni"], 6.0), [_alloy(["Al", "Cu", "Ni"], rep=(2, 2, 2), a=3.8)])


def test_adp_ni(lib):
    _compare(make_eam(["Ni"], 6.5, adp=True), [fcc(rep=(3, 3, 3), jitter=0.08)])


def test_adp_binary(lib):
    _compare(make_eam(["Mo", "Ni"], 6.0, adp=True), [_alloy(["Ni", "Ni", "Mo"], rep=(2, 2, 2))])


def test_adp_large_batch_uses_the_narrow_groups(lib):
    """Batches of 32768 atoms or more run the ADP kernels with 16 lanes per atom, smaller ones with
    32 (ta_eam.hip: eam_compute): the same binary frame, 160 copies in one batch (34560 atoms) against
    the one-frame evaluation that `_compare` pins to the oracle."""
    from tensoralloy_amd import Engine
    nn = make_eam(["Mo", "Ni"], 6.0, adp=True)
    atoms = _alloy(["Ni", "Ni", "Mo"], rep=(3, 3, 3), a=3.6)
    n_copies = 32768 // len(atoms) + 1
    with Engine(nn) as eng:
        one = eng.evaluate([atoms])[0]
        many = eng.evaluate([atoms] * n_copies)
    o = oracle_eam_eval(nn, atoms)
    assert abs(one["energy"] - o["energy"]) < E_TOL
    for r in (many[0], many[n_copies // 2], many[-1]):
        assert abs(r["energy"] - one["energy"]) < 1e-9
        assert np.abs(r["forces"] - one["forces"]).max() < 1e-10
        assert np.abs(r["virial"] - one["virial"]).max() < 1e-8


@pytest.mark.parametrize("generic", [False, True])
def test_nn_eam_default_potentials(lib, monkeypatch, generic):
    """The reference's default `EamAlloyNN(elements)`: rho, phi and embed are all "nn" functions
    with `Defaults.hidden_sizes` = [64, 32] (alloy.py:110-112, eam.py:174-190). Both device paths:
    the one-wavefront kernel for 1 -> H1 -> H2 -> 1 and the generic 16-row MLP tile."""
    if generic:
        monkeypatch.setenv("TA_EAM_NN_GENERIC", "1")
    nn = make_eam(["Ni"], 6.0, potential=None)
    assert nn.potentials == {"Ni": {"rho": "nn", "embed": "nn"}, "NiNi": {"phi": "nn"}}
    assert nn.hidden_sizes["Ni"]["rho"] == [64, 32]
    _compare(nn, [fcc(rep=(3, 3, 3)), fcc(rep=(2, 2, 2), a=3.3, seed=5), fcc(rep=(1, 1, 1))])


@pytest.mark.parametrize("generic", [False, True])
def test_nn_eam_one_hidden_layer(lib, monkeypatch, generic):
    """1 -> H -> 1 functions: the no-GEMM kernel and the generic tile."""
    if generic:
        monkeypatch.setenv("TA_EAM_NN_GENERIC", "1")
    frames = [_alloy(["Ni", "Ni", "Mo"], rep=(2, 2, 2)), fcc(rep=(1, 1, 1))]
    _compare(make_eam(["Mo", "Ni"], 6.0, potential=None, hidden_sizes=[40]), frames[:1])
    _compare(make_eam(["Ni"], 6.0, adp=True, potential=None, hidden_sizes=[7], activation="tanh"), frames[1:])


def test_nn_eam_binary_and_other_shapes(lib):
    frames = [_alloy(["Ni", "Ni", "Ni", "Mo"], rep=(2, 2, 3)), _alloy(["Mo", "Ni"], rep=(2, 2, 2), a=3.3)]
    _compare(make_eam(["Ni", "Mo"], 6.5, potential=None), frames)
    hs = {"Ni": {"rho": [16], "embed": [24, 24, 24]}, "Mo": {"rho": [40, 8]}, "MoNi": {"phi": [100]}}
    _compare(make_eam(["Ni", "Mo"], 6.0, potential=None, hidden_sizes=hs, activation="tanh"), frames)
    _compare(make_eam(["Al", "Cu", "Ni"], 6.0, potential=None, hidden_sizes=[32, 32], activation="squareplus"),
             [_alloy(["Al", "Cu", "Ni"], rep=(2, 2, 2), a=3.8)])


def test_nn_and_analytic_functions_in_one_model(lib):
    """`custom_potentials` per function, as test_eam_alloy_nn.py:55-63 builds its models."""
    frames = [_alloy(["Ni", "Ni", "Mo"], rep=(2, 2, 2))]
    pots = {"Ni": {"rho": "zjw04", "embed": "nn"}, "Mo": {"rho": "nn", "embed": "zjw04"},
            "NiNi": {"phi": "zjw04"}, "MoNi": {"phi": "nn"}, "MoMo": {"phi": "zjw04"}}
    _compare(make_eam(["Mo", "Ni"], 6.0, potential=pots), frames)
    pots = {"Ni": {"rho": "nn", "embed": "zjw04"}, "NiNi": {"phi": "zjw04"}}
    _compare(make_eam(["Ni"], 6.5, potential=pots), [fcc(rep=(2, 2, 2))])


def test_nn_adp(lib):
    frames = [_alloy(["Ni", "Ni", "Mo"], rep=(2, 2, 2))]
    _compare(make_eam(["Mo", "Ni"], 6.0, adp=True, potential=None, hidden_sizes=[32, 16]), frames)
    pots = {"Ni": {"rho": "zjw04", "embed": "zjw04"}, "NiNi": {"phi": "nn", "dipole": "mishinh", "quadrupole": "nn"}}
    _compare(make_eam(["Ni"], 6.0, adp=True, potential=pots), [fcc(rep=(2, 2, 2), jitter=0.08)])


def test_nn_eam_model_file_and_tables(lib, tmp_path):
    """export -> TensorAlloyCalculator round trip, and the setfl tables of nn functions
    (`export_to_setfl`, alloy.py:198-381, exists to tabulate exactly these)."""
    from oracle.eam import nn_function, read_setfl
    from tensoralloy_amd import Engine, TensorAlloyCalculator
    nn = make_eam(["Mo", "Ni"], 6.0, potential=None, hidden_sizes=[32, 16])
    atoms = _alloy(["Ni", "Ni", "Mo"], rep=(2, 2, 2))
    nn.export(str(tmp_path / "MoNi.pb"))
    calc = TensorAlloyCalculator(str(tmp_path / "MoNi.pb"))
    o = oracle_eam_eval(nn, atoms)
    assert abs(calc.get_potential_energy(atoms) - o["energy"]) < E_TOL
    assert np.abs(calc.get_forces(atoms) - o["forces"]).max() < F_TOL
    r = np.arange(200) * 0.03
    rho = np.arange(100) * 0.5
    with Engine(nn) as eng:
        tab = eng.eam_tabulate(r, rho)
    for k, el in enumerate(nn.elements):
        assert np.abs(tab["rho"][k] - nn_function(r, nn.weights[el]["rho"])[0]).max() < 1e-12
        assert np.abs(tab["embed"][k] - nn_function(rho, nn.weights[el]["embed"])[0]).max() < 1e-10
    for k, key in enumerate(tab["pairs"]):
        assert np.abs(tab["phi"][k] - nn_function(r, nn.weights[key]["phi"])[0]).max() < 1e-12
    path = nn.export_to_setfl(str(tmp_path / "MoNi.eam.alloy"), nr=200, dr=0.03, nrho=100, drho=0.5)
    back = read_setfl(path)
    assert np.abs(back["rho"]["Mo"] - nn_function(r, nn.weights["Mo"]["rho"])[0]).max() < 1e-12
    assert np.abs(back["rphi"]["MoNi"] - r * nn_function(r, nn.weights["MoNi"]["phi"])[0]).max() < 1e-11


def test_setfl_tables_run_as_splines(lib, tmp_path):
    """A LAMMPS setfl file evaluated as natural cubic splines (`spline@` potentials; the
    reference's `CubicInterpolator`, potentials/tests/test_mishin.py:36-160). Two checks: against
    the oracle's SciPy splines of the same tables, and -- since `Zhou_AlCu.alloy.eam` IS the Zjw04
    potential tabulated at dr = 0.003 (the reference asserts table == graph to 1e-12,
    test_eam_alloy_nn.py:139-164) -- against the analytic Zjw04 model, where only the
    interpolation error of the table remains."""
    from tensoralloy_amd import Engine, TensorAlloyCalculator, UniversalTransformer
    from tensoralloy_amd.eam import EamAlloyNN
    path = golden_setfl("Zhou_AlCu.alloy.eam", tmp_path)
    nn = EamAlloyNN.from_setfl(path)
    nn.attach_transformer(UniversalTransformer(["Al", "Cu"], rcut=5.99))
    frames = [_alloy(["Al", "Cu"], rep=(2, 2, 2), a=3.9), _alloy(["Al", "Al", "Cu"], rep=(2, 2, 3), a=4.05)]
    _compare(nn, frames)
    analytic = make_eam(["Al", "Cu"], 5.99)
    with Engine(nn) as e1, Engine(analytic) as e2:
        for a, b in zip(e1.evaluate(frames), e2.evaluate(frames)):
            assert abs(a["energy"] - b["energy"]) < 2e-6 * len(a["forces"])
            assert np.abs(a["forces"] - b["forces"]).max() < 2e-4
    # one tabulated function inside an otherwise analytic model, and the model file round trip
    pots = {"Al": {"rho": "spline@" + path, "embed": "zjw04"}, "Cu": {"rho": "zjw04", "embed": "spline@" + path},
            "AlAl": {"phi": "zjw04"}, "AlCu": {"phi": "spline@" + path}, "CuCu": {"phi": "zjw04"}}
    mixed = make_eam(["Al", "Cu"], 5.99, potential=pots)
    _compare(mixed, frames[:1])
    mixed.export(str(tmp_path / "mixed.pb"))
    calc = TensorAlloyCalculator(str(tmp_path / "mixed.pb"))
    assert abs(calc.get_potential_energy(frames[0]) - oracle_eam_eval(mixed, frames[0])["energy"]) < E_TOL


def test_adp_tables_run_as_splines(lib, tmp_path):
    from tensoralloy_amd import UniversalTransformer
    from tensoralloy_amd.eam import AdpNN
    nn = AdpNN.from_setfl(golden_setfl("AlCu_thinned.adp", tmp_path))
    nn.attach_transformer(UniversalTransformer(["Al", "Cu"], rcut=6.2))
    _compare(nn, [_alloy(["Al", "Al", "Cu"], rep=(2, 2, 2), a=4.0)])


def test_sutton90_and_agrawal_potentials(lib, tmp_path):
    """`sutton90` (AgSutton90) and `Be/1` (AgrawalBe) of the reference's `available_potentials`.
    Besides the oracle: the reference checks `Be/1` against LAMMPS running Agrawal's own
    `Be_Agrawal.eam.alloy` (potentials/tests/test_agrawal.py:52-110); that table, run here as
    splines, must give the energies and forces of the analytic kernels (its density is tabulated in
    other units, which the embedding table absorbs: only whole-structure values are comparable).
    The table is not the formula to more than about 1 meV per atom (F of the table and of the
    published constants differ in the fourth digit): the reference's own bounds are 1e-2 eV on the energy
    of 16 atoms and 1e-2 eV/A on the forces (test_agrawal.py:99-100); here 1.5e-3 eV per atom, 1e-2 eV/A,
    on the same kind of structure (hcp Be, 0.1 A noise)."""
    from tensoralloy_amd import Engine, UniversalTransformer
    from tensoralloy_amd.eam import EamAlloyNN
    _compare(make_eam(["Ag"], 8.0, potential="sutton90"), [fcc("Ag", a=4.09, rep=(2, 2, 2), jitter=0.08)])
    pots = {"Ag": {"rho": "sutton90", "embed": "sutton90"}, "AgAg": {"phi": "sutton90"}}   # test_sutton90.py:104-106
    _compare(make_eam(["Ag"], 6.0, potential=pots), [fcc("Ag", a=4.2, rep=(2, 2, 2))])
    be = make_eam(["Be"], 5.0, potential="Be/1")
    frames = [hcp(), hcp(rep=(3, 3, 3), jitter=0.05, seed=4)]
    _compare(be, frames)
    tab = EamAlloyNN.from_setfl(golden_setfl("Be_Agrawal_thinned.eam.alloy", tmp_path))
    tab.attach_transformer(UniversalTransformer(["Be"], rcut=5.0))
    with Engine(be) as e1, Engine(tab) as e2:
        for a, b in zip(e1.evaluate(frames), e2.evaluate(frames)):
            assert abs(a["energy"] - b["energy"]) < 1.5e-3 * len(a["forces"])
            assert np.abs(a["forces"] - b["forces"]).max() < 1e-2
    _compare(make_eam(["Pu"], 6.0, potential="grimes"), [fcc("Pu", a=4.6, rep=(2, 2, 2), jitter=0.08)])
    mixed = {"Be": {"rho": "Be/1", "embed": "nn"}, "BeBe": {"phi": "Be/1"}}
    _compare(make_eam(["Be"], 5.0, potential=mixed, hidden_sizes=[8]), frames[:1])


def test_nn_and_table_models_edge_cases(lib, tmp_path):
    """Lone atoms (no pairs: rho = 0, F(0) of an nn embedding is not 0), an empty batch, uneven
    batches, a molecule without periodicity, 'medium' precision, and a second evaluation with other
    frames on the same handle (buffers grow)."""
    from tensoralloy_amd import Atoms, Engine, UniversalTransformer
    from tensoralloy_amd.eam import EamAlloyNN
    nn = make_eam(["Mo", "Ni"], 5.5, potential=None, hidden_sizes=[16, 16])
    lone = Atoms(symbols=["Ni"], positions=[[1.0, 2.0, 3.0]], cell=np.eye(3) * 25.0, pbc=True)
    mol = Atoms(symbols=["Ni", "Mo", "Ni", "Mo", "Ni"], positions=np.random.RandomState(3).rand(5, 3) * 4.0,
                cell=np.eye(3) * 20.0, pbc=False)
    big = _alloy(["Ni", "Ni", "Mo"], rep=(2, 2, 3))
    with Engine(nn) as eng:
        assert eng.evaluate([]) == []
        for frames in ([lone], [lone, big, mol], [big], [mol, lone]):
            res = eng.evaluate(frames)
            for a, r in zip(frames, res):
                o = oracle_eam_eval(nn, a)
                assert abs(r["energy"] - o["energy"]) < E_TOL
                assert np.abs(r["forces"] - o["forces"]).max() < F_TOL
                assert np.abs(r["virial"] - o["virial"]).max() < W_TOL
    assert abs(oracle_eam_eval(nn, lone)["energy"]) > 1e-3          # F(0) != 0 for an nn embedding
    med = make_eam(["Ni"], 6.0, potential=None, hidden_sizes=[8])
    med.precision = "medium"
    _compare(med, [fcc(rep=(2, 2, 2))])
    tab = EamAlloyNN.from_setfl(golden_setfl("Zhou_AlCu.alloy.eam", tmp_path))
    tab.attach_transformer(UniversalTransformer(["Al", "Cu"], rcut=5.5))
    lone_al = Atoms(symbols=["Al"], positions=[[0.0, 0.0, 0.0]], cell=np.eye(3) * 25.0, pbc=True)
    _compare(tab, [lone_al, _alloy(["Al", "Cu"], rep=(2, 2, 2), a=3.9)])


def test_device_softplus_accuracy(lib):
    """The device softplus (own exp / log1p / reciprocals, ta_math.h) against NumPy in extended
    precision, through the table of an nn function whose only live unit is softplus(x)."""
    from tensoralloy_amd import Engine
    nn = make_eam(["Ni"], 6.0, potential=None, hidden_sizes=[4])
    w1 = np.zeros((1, 4)); w1[0, 0] = 1.0; w1[0, 1] = -1.0
    for sec, fn in (("Ni", "rho"), ("Ni", "embed"), ("NiNi", "phi")):
        nn.weights[sec][fn] = [(w1, np.zeros(4)), (np.array([[1.0], [0.0], [0.0], [0.0]]), None)]
    nn.weights["Ni"]["embed"][1] = (np.array([[0.0], [1.0], [0.0], [0.0]]), None)   # softplus(-x)
    x = np.concatenate([np.linspace(0.0, 45.0, 4001), np.geomspace(1e-12, 700.0, 3000)])
    with Engine(nn) as eng:
        tab = eng.eam_tabulate(x, x)
    xl = x.astype(np.longdouble)
    ref_pos = (xl + np.log1p(np.exp(-xl))).astype(np.float64)
    ref_neg = np.log1p(np.exp(-xl)).astype(np.float64)
    assert np.abs(tab["rho"][0] / ref_pos - 1.0).max() < 2e-15
    ok = ref_neg > 1e-300
    assert np.abs(tab["embed"][0][ok] / ref_neg[ok] - 1.0).max() < 2e-15


def test_zjw04xc_blended_embedding(lib):
    # densities on both sides of 0.85 rho_e and 1.15 rho_e: compressed, equilibrium, expanded
    frames = [fcc(rep=(2, 2, 2), a=a, seed=3) for a in (3.3, 3.52, 3.8)]
    _compare(make_eam(["Ni"], 6.0, potential="zjw04xc"), frames)
    _compare(make_eam(["Al", "Cu"], 6.5, potential="zjw04uxc"), [_alloy(["Al", "Cu"], rep=(2, 2, 2), a=3.9)])


def test_zjw04xcp_cross_term(lib):
    _compare(make_eam(["Mo", "Ni"], 6.5, potential="zjw04xcp"), [_alloy(["Ni", "Ni", "Ni", "Mo"], rep=(2, 2, 3))])
    with pytest.raises(ValueError, match="no phi constants"):
        make_eam(["Cu", "Ni"], 6.5, potential="zjw04xcp").to_desc()


def test_device_functions_reproduce_the_reference_setfl_tables(lib, tmp_path):
    """`Zhou_AlCu.alloy.eam` / `zjw04_Ni.alloy.eam`: the tables the reference asserts its Zjw04 graph
    against to 1e-12 (nn/eam/tests/test_eam_alloy_nn.py:139-164), plus the literals of
    io/tests/test_lammps.py:25-71. Here the DEVICE functions of the energy kernels are tabulated
    (`ta_eam_tabulate`, what `export_to_setfl` writes) and held to the same tolerance."""
    import json
    import os
    from tensoralloy_amd import Engine
    with open(os.path.join(os.path.dirname(__file__), "golden", "eam_tables.json")) as fp:
        t = json.load(fp)
    for tag in ("AlCu", "Ni"):
        d = t[tag]
        nn = make_eam(d["elements"], d["rcut"])
        r = np.array(d["r_index"]) * d["dr"]
        rho = np.array(d["rho_index"]) * d["drho"]
        with Engine(nn) as eng:
            tab = eng.eam_tabulate(r, rho)
        for k, el in enumerate(nn.elements):
            ref = np.array(d["rho"][el])
            assert np.abs(tab["rho"][k] - ref).max() < 1e-12 * max(1, np.abs(ref).max())
            assert np.abs(tab["embed"][k] - np.array(d["embed"][el])).max() < 1e-12
        for key, ref in d["rphi"].items():
            a, b = sorted([key[:2], key[2:]])
            row = tab["pairs"].index(a + b)
            got = tab["phi"][row][1:] * r[1:]
            ref = np.array(ref)[1:]
            assert np.abs(got - ref).max() < 1e-12 * max(1, np.abs(ref).max())
    lit = t["literal"]
    nn = make_eam(["Al", "Cu"], t["AlCu"]["rcut"])
    with Engine(nn) as eng:
        tab = eng.eam_tabulate([t["AlCu"]["dr"]], [10 * t["AlCu"]["drho"]])
    assert abs(tab["embed"][0][0] - lit["F_Al_10"]) < 1e-14
    assert abs(tab["phi"][tab["pairs"].index("CuCu")][0] * t["AlCu"]["dr"] - lit["rphi_CuCu_1"]) < 1e-12
    # the file writer: same grids as the reference's fixture, read back with the oracle's reader
    from oracle.eam import read_setfl
    path = nn.export_to_setfl(str(tmp_path / "AlCu.alloy.eam"), nr=2000, dr=0.003, nrho=2000, drho=0.05,
                              lattice_constants={"Al": 4.05, "Cu": 3.61})
    back = read_setfl(path)
    assert back["elements"] == ["Al", "Cu"] and back["nr"] == 2000 and back["nrho"] == 2000
    assert abs(back["dr"] - 0.003) < 1e-15 and abs(back["rcut"] - t["AlCu"]["rcut"]) < 1e-12
    d = t["AlCu"]
    for el in ("Al", "Cu"):
        assert np.abs(back["rho"][el][d["r_index"]] - np.array(d["rho"][el])).max() < 1e-12 * 30
        assert np.abs(back["embed"][el][d["rho_index"]] - np.array(d["embed"][el])).max() < 1e-12
    for key, ref in d["rphi"].items():
        got = back["rphi"][key][d["r_index"]][1:]
        assert np.abs(got - np.array(ref)[1:]).max() < 1e-12 * max(1, np.abs(ref).max())


@pytest.mark.parametrize("kind", ["zjw04", "zjw04_binary_skin", "setfl", "nn_tables", "nn_all", "adp", "adp_nn"])
def test_analytic_hessian_vectors(lib, tmp_path, kind):
    """`ta_hessian_vectors` (dual-number tangents through the analytic EAM force kernels; replaces
    tf.hessians, nn/basic.py:411-421, and the cell derivative of the virial behind the elastic
    constants, nn/constraint/elastic.py:24-44) against central differences of the GPU's own analytic
    forces and virials along random directions of positions AND cell, and the symmetry of the Hessian
    from the unit directions. Models: Zjw04 Ni; Mo-Ni with the cross pair term, a sheared cell and a
    Verlet skin; the Al-Cu setfl tables as splines; nn pair functions through their Hermite tables; the
    reference's default all-nn Mo-Ni model (embedding networks included); ADP with the MishinH functions and
    with networks for everything. This guards the consistency of the force kernels with their dual-arithmetic
    copies; against the oracle (a stencil of its forces, or the analytic second derivatives of
    tests/eam_hvp_reference.py for tabulated functions) and on batches of different frames: test_gpu_hvp_oracle.py."""
    from tensoralloy_amd import Atoms, Engine
    from tensoralloy_amd.eam import EamAlloyNN
    if kind == "zjw04":
        nn, atoms = make_eam(["Ni"], 6.0), fcc(rep=(2, 2, 2), seed=3)
    elif kind == "zjw04_binary_skin":
        nn = make_eam(["Mo", "Ni"], 6.0)
        atoms = _alloy(["Ni", "Ni", "Mo"], rep=(2, 2, 3), seed=5)
        cell = np.asarray(atoms.get_cell(complete=True)).copy()
        cell[1, 0] = 0.2 * cell[0, 0]
        atoms = Atoms(symbols=atoms.get_chemical_symbols(), positions=atoms.positions, cell=cell, pbc=True)
    elif kind == "setfl":
        from tensoralloy_amd import UniversalTransformer
        nn = EamAlloyNN.from_setfl(golden_setfl("Zhou_AlCu.alloy.eam", tmp_path))
        nn.attach_transformer(UniversalTransformer(["Al", "Cu"], rcut=5.99))
        atoms = _alloy(["Al", "Cu"], rep=(2, 2, 2), a=3.9, seed=7)
    elif kind == "nn_tables":
        nn = make_eam(["Ni"], 6.0, potential={"Ni": {"rho": "nn", "embed": "zjw04"}, "NiNi": {"phi": "nn"}},
                      hidden_sizes=[16, 16])
        atoms = fcc(rep=(2, 2, 2), seed=9)
    elif kind == "nn_all":   # the reference's default: every function a network (pair functions through their
        # tables, F'' of the embedding networks by a value / first / second derivative sweep)
        nn = make_eam(["Mo", "Ni"], 5.5, potential=None, hidden_sizes=[12, 12])
        atoms = _alloy(["Ni", "Mo"], rep=(2, 2, 2), seed=4)
    elif kind == "adp":      # Zjw04 + MishinH dipole / quadrupole, two elements, sheared cell
        nn = make_eam(["Mo", "Ni"], 6.0, adp=True)
        atoms = _alloy(["Ni", "Ni", "Mo"], rep=(2, 2, 2), seed=6)
        cell = np.asarray(atoms.get_cell(complete=True)).copy()
        cell[2, 0] = 0.15 * cell[0, 0]
        atoms = Atoms(symbols=atoms.get_chemical_symbols(), positions=atoms.positions, cell=cell, pbc=True)
    else:                    # nn-ADP, the reference's default ADP model. (Networks do not vanish at the cutoff:
        # rc = 5.8 A sits between the 5.57 and 6.10 A shells, so that no pair crosses it in the differences)
        nn = make_eam(["Ni"], 5.8, adp=True, potential=None, hidden_sizes=[8, 8])
        atoms = fcc(rep=(2, 2, 2), seed=8)
    n = len(atoms)
    h = np.asarray(atoms.get_cell(complete=True), dtype=float)
    rng = np.random.RandomState(2)
    dR = rng.normal(size=(2, n, 3))
    dh = rng.normal(size=(2, 1, 3, 3)) * 0.3
    dR[1] = 0.0        # second direction: the cell alone (the elastic-constant case)
    want = 1 | 2 | 4
    eps = 1e-4
    with Engine(nn) as eng:
        if kind == "zjw04_binary_skin":
            eng.set_skin(0.4)
        eng.set_frames([atoms])
        dF, dW = eng.hessian_vectors(dR=dR, dh=dh, want_virial=True)
        H = -eng.hessian_vectors()                  # [3 n, n, 3]
        for d in range(2):
            fd_F, fd_W = 0.0, 0.0
            for sgn in (1.0, -1.0):
                a = Atoms(symbols=atoms.get_chemical_symbols(), positions=atoms.positions + sgn * eps * dR[d],
                          cell=h + sgn * eps * dh[d, 0], pbc=True)
                r = eng.evaluate([a], want=want)[0]
                fd_F = fd_F + sgn * r["forces"] / (2 * eps)
                fd_W = fd_W + sgn * r["virial"] / (2 * eps)
            tol_f = 2e-6 * max(1.0, np.abs(fd_F).max())
            assert np.abs(dF[d] - fd_F).max() < tol_f, (d, np.abs(dF[d] - fd_F).max())
            assert np.abs(dW[d, 0] - fd_W).max() < 2e-6 * max(1.0, np.abs(fd_W).max())
    Hm = H.reshape(3 * n, 3 * n)
    assert np.abs(Hm - Hm.T).max() < 1e-9 * max(1.0, np.abs(Hm).max())
    assert np.abs(Hm.sum(axis=1)).max() < 1e-8          # acoustic sum rule: a rigid shift costs nothing


def test_hessian_vectors_refuse_models_without_the_analytic_path(lib):
    from tensoralloy_amd import Engine
    for nn, atoms in ((make_eam(["Ag"], 7.0, potential="sutton90"), fcc("Ag", a=4.09, rep=(1, 1, 1))),):  # sutton90
        with Engine(nn) as eng:
            eng.set_frames([atoms])
            with pytest.raises(ValueError, match="analytic second derivatives"):
                eng.hessian_vectors()
