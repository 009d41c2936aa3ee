"""CPU: the temperature-dependent model class, its files and the NumPy restatement of its head
(tests/td_reference.py). No GPU needed."""
import json

import numpy as np
import pytest

from tensoralloy_amd import _lib
from tensoralloy_amd.model import load_model
from tensoralloy_amd.td import FiniteTemperatureOptions, TemperatureDependentAtomicNN
from tests.helpers import make_grap_nn, make_nn
from tests.td_reference import td_head


def _td(base, layers=(20, 37), hidden=(30,), algo="default", resnet=True, minmax=True, seed=3):
    nn = TemperatureDependentAtomicNN(base.elements, base.descriptor, hidden_sizes=list(hidden),
                                      minmax_scale=minmax, use_resnet_dt=resnet,
                                      finite_temperature={"layers": list(layers), "algo": algo})
    nn.attach_transformer(base.transformer)
    nn.initialize(seed=seed, bias_scale=0.1)
    if minmax:
        rng = np.random.RandomState(seed)
        for el in nn.elements:
            nn.minmax[el] = (rng.rand(nn.ndim()) * 0.1, 1.0 + rng.rand(nn.ndim()))
    return nn


def _grap_base(elements=("Be",), algorithm="pexp"):
    return make_grap_nn(list(elements), 5.0, [16], algorithm=algorithm)


@pytest.mark.parametrize("algo", ["default", "Sommerfeld"])
def test_head_against_central_differences(algo):
    nn = _td(make_nn(["Mo", "Ni"], 5.0, False, [16]), layers=(24, 24, 17), hidden=(19, 19), algo=algo)
    rng = np.random.RandomState(1)
    D = nn.ndim()
    G = rng.rand(6, D)
    syms = ["Mo", "Ni", "Ni", "Mo", "Ni", "Mo"]
    T = rng.rand(6) + 0.2
    r = td_head(nn, syms, G, T)
    assert np.allclose(r["F"], r["U"] - T * r["S"], rtol=0, atol=1e-12)
    h = 1e-6
    for k in range(D):
        Gp, Gm = G.copy(), G.copy()
        Gp[:, k] += h
        Gm[:, k] -= h
        fd = (td_head(nn, syms, Gp, T)["F"] - td_head(nn, syms, Gm, T)["F"]) / (2 * h)
        assert np.abs(fd - r["dFdG"][:, k]).max() < 1e-7 * max(1.0, np.abs(fd).max())
    # T enters z as the last column: dF/dT = dU/dT - S - T dS/dT (checked through F(T))
    dT = 1e-6
    Fp, Fm = td_head(nn, syms, G, T + dT)["F"], td_head(nn, syms, G, T - dT)["F"]
    Sp, Sm = td_head(nn, syms, G, T + dT)["S"], td_head(nn, syms, G, T - dT)["S"]
    Up, Um = td_head(nn, syms, G, T + dT)["U"], td_head(nn, syms, G, T - dT)["U"]
    dF = (Fp - Fm) / (2 * dT)
    assert np.allclose(dF, (Up - Um) / (2 * dT) - r["S"] - T * (Sp - Sm) / (2 * dT), atol=1e-6)


def test_sommerfeld_entropy_vanishes_at_zero_temperature():
    nn = _td(_grap_base(), algo="Sommerfeld")
    G = np.random.RandomState(2).rand(4, nn.ndim())
    r = td_head(nn, ["Be"] * 4, G, np.zeros(4))
    assert np.all(r["S"] == 0.0) and np.array_equal(r["F"], r["U"])


def test_options_and_as_dict_round_trip(tmp_path):
    assert FiniteTemperatureOptions() == FiniteTemperatureOptions("softplus", (128, 128), "default")
    with pytest.raises(ValueError):
        FiniteTemperatureOptions(activation="nope")
    nn = _td(_grap_base(("Be", "Mo")), algo="Sommerfeld")
    d = nn.as_dict()
    assert d["class"] == "TemperatureDependentAtomicNN"
    assert d["finite_temperature"] == {"activation": "softplus", "layers": [20, 37], "algo": "Sommerfeld"}
    d = json.loads(json.dumps(d))
    d.pop("class")
    again = TemperatureDependentAtomicNN(**d)
    assert again.as_dict() == nn.as_dict()
    assert nn.is_finite_temperature and nn.variational_energy == "free_energy"
    # json + npz model file
    path = nn.export(str(tmp_path / "td.json"))
    meta = json.load(open(path))
    assert meta["Metadata/is_finite_temperature"] == 1
    assert meta["Metadata/variational_energy"] == "free_energy"
    assert {"energy", "eentropy", "free_energy"} <= set(meta["Metadata/ops"])
    nn2, _, _ = load_model(path)
    assert isinstance(nn2, TemperatureDependentAtomicNN) and nn2.as_dict() == nn.as_dict()
    for el in nn.elements:
        for net in "HUS":
            for (w1, b1), (w2, b2) in zip(nn.weights[el][net], nn2.weights[el][net]):
                assert np.array_equal(w1, w2) and np.array_equal(b1, b2)
        assert all(np.array_equal(a, b) for a, b in zip(nn.minmax[el], nn2.minmax[el]))


def test_model_description_layout():
    nn = _td(make_nn(["Mo", "Ni"], 5.0, True, [16]), algo="Sommerfeld")
    desc, keep = nn.to_desc()
    assert desc.finite_temperature == (_lib.TA_TD_ON | _lib.TA_TD_SOMMERFELD |
                                       (_lib.TA_ACT["softplus"] << _lib.TA_TD_ACT_SHIFT))
    D, K = nn.ndim(), 37
    n_layers = [desc.n_layers[k] for k in range(6)]
    assert n_layers == [2, 2, 2, 2, 2, 2]    # H[Mo], H[Ni], U[Mo], U[Ni], S[Mo], S[Ni]
    sizes = [desc.layer_sizes[k] for k in range(18)]
    assert sizes == [D, 20, K] * 2 + [K + 1, 30, 1] * 4
    plain, _ = make_nn(["Ni"], 5.0, False, [16]).to_desc()
    assert plain.finite_temperature == 0


# the reference writer's layout (finite_temperature.py:455-650) for one element, pexp descriptor
REF_KEYS = {"rmax", "nelt", "masses", "numbers", "max_moment", "fctype", "tdnp", "precision", "is_T_symmetric",
            "tdnp::Sommerfeld", "descriptor::method", "descriptor::rl", "descriptor::pl"} | \
    {f"{n}::{k}" for n in "HSU" for k in ("nlayers", "actfn", "layer_sizes", "use_resnet_dt", "apply_output_bias")}


@pytest.mark.parametrize("algo", ["default", "Sommerfeld"])
@pytest.mark.parametrize("static", [True, False])
def test_native_writer_layout_and_round_trip(tmp_path, algo, static):
    base = _grap_base()
    nn = TemperatureDependentAtomicNN(["Be"], base.descriptor, hidden_sizes=[30, 30], minmax_scale=False,
                                      use_resnet_dt=True, use_atomic_static_energy=static,
                                      atomic_static_energy={"Be": -3.7},
                                      finite_temperature={"layers": [20, 37], "algo": algo, "activation": "tanh"})
    nn.attach_transformer(base.transformer)
    nn.initialize(seed=9, bias_scale=0.1)
    path = nn.export_to_lammps_native(str(tmp_path / "td.npz"))
    z = np.load(path)
    weights = {f"{n}::weights_0_{j}" for n, L in (("H", 2), ("S", 3), ("U", 3)) for j in range(L)}
    biases = {f"{n}::biases_0_{j}" for n, L in (("H", 2), ("S", 3), ("U", 3 if static else 2)) for j in range(L)}
    assert set(z.files) == REF_KEYS | weights | biases
    assert int(z["tdnp"]) == 1 and int(z["tdnp::Sommerfeld"]) == (algo == "Sommerfeld")
    assert list(z["H::layer_sizes"]) == [20, 37] and list(z["U::layer_sizes"]) == [30, 30, 1]
    assert int(z["H::actfn"]) == 2 and int(z["U::actfn"]) == 1 and int(z["S::actfn"]) == 1
    assert int(z["H::apply_output_bias"]) == 1 and int(z["S::apply_output_bias"]) == 1
    assert int(z["U::apply_output_bias"]) == int(static)
    assert z["H::weights_0_0"].shape == (nn.ndim(), 20) and z["H::weights_0_1"].shape == (20, 37)
    assert z["U::weights_0_0"].shape == (38, 30) and z["U::weights_0_2"].shape == (30,)
    assert z["S::biases_0_2"].shape == (1,)
    nn2, clf, meta = load_model(path)
    assert isinstance(nn2, TemperatureDependentAtomicNN)
    assert meta["Metadata/is_finite_temperature"] == 1
    assert nn2.finite_temperature_options == nn.finite_temperature_options
    assert nn2._use_atomic_static_energy == static and nn2._use_resnet_dt
    for net in "HUS":
        for (w1, b1), (w2, b2) in zip(nn.weights["Be"][net], nn2.weights["Be"][net]):
            assert np.array_equal(w1, w2)
            assert (b1 is None and b2 is None) or np.array_equal(b1, b2)


def test_model_from_be_grap_sf_quad_options():
    """The options of the reference's training input test_files/inputs/Be_grap_sf_quad.toml: GRAP `sf`
    (8 eta x 3 omega), moment tensor 2, rcut 5.0, Be hidden [64, 64], softplus, medium precision;
    finite_temperature and use_resnet_dt from defaults.toml (:118-121)."""
    from tensoralloy_amd import GenericRadialAtomicPotential, UniversalTransformer
    gd = GenericRadialAtomicPotential(["Be"], "sf", {"eta": [0.1, 0.5, 1.0, 2.0, 4.0, 8.0, 20.0, 40.0],
                                                    "omega": [0.0, 1.5, 3.0]},
                                      param_space_method="cross", moment_tensors=[2])
    nn = TemperatureDependentAtomicNN(["Be"], gd, hidden_sizes={"Be": [64, 64]}, activation="softplus",
                                      kernel_initializer="he_normal", use_resnet_dt=True,
                                      minimize_properties=["energy", "eentropy", "free_energy", "forces", "stress"],
                                      export_properties=["energy", "forces", "stress"],
                                      finite_temperature=FiniteTemperatureOptions())
    nn.attach_transformer(UniversalTransformer(["Be"], rcut=5.0, angular=False))
    nn.precision = "medium"
    nn.initialize()
    sizes = nn.layer_sizes("Be")
    assert sizes == {"H": [nn.ndim(), 128, 128], "U": [129, 64, 64, 1], "S": [129, 64, 64, 1]}
    desc, _ = nn.to_desc()
    assert desc.kind == _lib.TA_MODEL_GRAP_MLP and desc.eps == 1e-8
    assert [desc.n_layers[k] for k in range(3)] == [2, 3, 3]
