"""The GRAP `nn` filter network through its device-built Hermite table (`ta_set_filter_tables`,
`Engine.set_filter_tables`, `TensorAlloyCalculator(filter_tables=True)`; csrc/ta_grap.hip) against the exact
evaluation of the same engine and against oracle/grap.py.

Bounds: tables against exact as tests/test_gpu_eam.py holds the EAM tables (1e-9 eV, 1e-8 eV/A, 1e-7 eV
virial); both against the oracle at E_TOL, F_TOL, W_TOL of tests/test_gpu_sf.py."""
import copy

import numpy as np
import pytest

from tensoralloy_amd import _lib
from tensoralloy_amd.grap import FILTER_TABLE_KNOTS
from tests.helpers import fcc, make_grap_nn, oracle_grap_eval
from tests.test_gpu_sf import _alloy, E_TOL, F_TOL, W_TOL

pytestmark = pytest.mark.gpu

TE, TF, TW = 1e-9, 1e-8, 1e-7   # tables against exact
ALL = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES | _lib.TA_WANT_VIRIAL | _lib.TA_WANT_ATOMIC


def _default_nn():
    """defaults.toml `[nn.atomic.grap.nn]`: softplus 32-32-32 with ResNet skips, 16 filters, rc 6, moments 0..3"""
    return make_grap_nn(["Ni"], 6.0, [64, 64], "nn", moment_tensors=[0, 1, 2, 3])


def _close(tab, exact, tag=""):
    dE = abs(tab["energy"] - exact["energy"])
    dF = np.abs(tab["forces"] - exact["forces"]).max() if len(exact["forces"]) else 0.0
    dW = np.abs(tab["virial"] - exact["virial"]).max()
    print(f"tables vs exact {tag}: dE {dE:.2e} dF {dF:.2e} dW {dW:.2e}")
    assert dE < TE and dF < TF and dW < TW, (tag, dE, dF, dW)


def _oracle(nn, atoms, got):
    o = oracle_grap_eval(nn, atoms)
    assert abs(got["energy"] - o["energy"]) < E_TOL
    assert np.abs(got["atomic"] - o["atomic"]).max() < E_TOL
    assert np.abs(got["forces"] - o["forces"]).max() < F_TOL
    assert np.abs(got["virial"] - o["virial"]).max() < W_TOL


def _parity(nn, atoms_list):
    from tensoralloy_amd import Engine
    with Engine(nn) as eng:
        assert eng.filter_table_knots == 0          # off unless asked for
        eng.set_filter_tables(True)
        assert eng.filter_table_knots == FILTER_TABLE_KNOTS
        tab = eng.evaluate(atoms_list)
        eng.set_filter_tables(False)
        assert eng.filter_table_knots == 0
        exact = eng.evaluate(atoms_list)
    for k, (atoms, t, x) in enumerate(zip(atoms_list, tab, exact)):
        _close(t, x, f"frame {k}")
        _oracle(nn, atoms, t)
        _oracle(nn, atoms, x)


def test_default_network_two_frames(lib):
    _parity(_default_nn(), [fcc(rep=(3, 3, 3)), fcc(rep=(1, 1, 1))])


def test_tanh_network_binary_symmetric(lib):
    par = {"hidden_sizes": [24, 40], "num_filters": 10, "activation": "tanh", "use_resnet_dt": False}
    nn = make_grap_nn(["Mo", "Ni"], 5.5, [16], "nn", par, moment_tensors=[0, 1, 2], symmetric=True)
    _parity(nn, [_alloy(["Ni", "Ni", "Mo"], rep=(2, 2, 2))])


@pytest.mark.parametrize("modifier", [1, 2])
def test_input_modifiers(lib, modifier):
    """The table is one function of the network's input x = r / rcov or exp(-r / rcov) for both elements."""
    par = {"hidden_sizes": [32, 32], "num_filters": 8, "h_abck_modifier": modifier}
    nn = make_grap_nn(["Mo", "Ni"], 5.5, [16, 16], "nn", par, moment_tensors=[0, 1, 2, 3])
    _parity(nn, [_alloy(["Ni", "Ni", "Mo"], rep=(2, 2, 2)), fcc(rep=(2, 2, 2))])


def test_moments_up_to_5(lib):
    """The 56-component kernels."""
    nn = make_grap_nn(["Ni"], 5.0, [16], "nn", {"hidden_sizes": [16, 16], "num_filters": 6},
                      moment_tensors=[0, 1, 2, 3, 4, 5])
    _parity(nn, [fcc(rep=(2, 2, 2), seed=3)])


def test_coarse_tables_deviate_and_converge(lib):
    """33, 129, 513 knots against exact: a 33-knot table is visibly coarse (3e-5 eV/A in the numpy study of the
    scheme; a silent fall-back to the exact path would give 1e-14), and each fourfold refinement shrinks the
    force deviation at least 8x (fourth-order Hermite: 64x for the derivative in theory)."""
    from tensoralloy_amd import Engine
    nn, atoms = _default_nn(), fcc(rep=(3, 3, 3))
    dev = []
    with Engine(nn) as eng:
        exact = eng.evaluate([atoms])[0]
        for knots in (33, 129, 513):
            eng.set_filter_tables(True, knots=knots)
            assert eng.filter_table_knots == knots
            r = eng.evaluate([atoms])[0]
            dev.append(np.abs(r["forces"] - exact["forces"]).max())
    print("force deviation at 33 / 129 / 513 knots:", dev)
    assert dev[0] > 1e-6
    assert dev[1] < dev[0] / 8
    assert dev[2] < dev[1] / 8


def _moves(atoms, n_small=4):
    """Displaced copies: small moves that keep a skin list, then one jump that rebuilds it."""
    rng = np.random.RandomState(17)
    out, pos = [], atoms.positions.copy()
    for k in range(n_small + 1):
        pos = pos + rng.normal(0, 0.02 if k < n_small else 0.6, pos.shape)
        a = atoms.copy()
        a.positions = pos.copy()
        out.append(a)
    return out


def test_calculator_with_skin(lib, tmp_path):
    from tensoralloy_amd import Engine, TensorAlloyCalculator
    nn = _default_nn()
    calc = TensorAlloyCalculator(nn.export(str(tmp_path / "fnn")), filter_tables=True, skin=0.5)
    assert calc._engine.filter_table_knots == FILTER_TABLE_KNOTS
    plain = TensorAlloyCalculator(nn.export(str(tmp_path / "fnn2")))
    assert plain._engine.filter_table_knots == 0
    with Engine(nn) as exact:
        for k, a in enumerate(_moves(fcc(rep=(2, 2, 2), jitter=0.05))):
            x = exact.evaluate([a])[0]
            e, f = calc.get_potential_energy(a), calc.get_forces(a)
            s = calc.get_stress(a)
            print(f"move {k}: dE {abs(e - x['energy']):.2e} dF {np.abs(f - x['forces']).max():.2e}")
            assert abs(e - x["energy"]) < TE
            assert np.abs(f - x["forces"]).max() < TF
            assert np.abs(s - x["stress"]).max() * a.get_volume() < TW


def test_step_view_two_uneven_frames_with_skin(lib):
    from tensoralloy_amd import Engine
    nn = _default_nn()
    frames = [fcc(rep=(2, 2, 2), jitter=0.05), fcc(rep=(1, 1, 2), jitter=0.05, seed=9)]
    n0 = len(frames[0])
    paths = [_moves(f) for f in frames]
    with Engine(nn) as eng, Engine(nn) as exact:
        eng.set_skin(0.5)
        eng.set_filter_tables(True)
        eng.set_frames(frames)
        for k in range(len(paths[0])):
            now = [p[k] for p in paths]
            pos = np.concatenate([a.positions for a in now])
            got = {key: np.array(v) for key, v in eng.step(pos, ALL, view=True).items()}
            ref = exact.evaluate(now)
            for f, x in enumerate(ref):
                sl = slice(0, n0) if f == 0 else slice(n0, None)
                _close({"energy": got["energy"][f], "forces": got["forces"][sl], "virial": got["virial"][f]}, x,
                       f"step {k} frame {f}")
        assert eng.filter_table_knots == FILTER_TABLE_KNOTS


def test_update_filter_weights_rebuilds_the_table(lib):
    from tensoralloy_amd import Engine
    from tensoralloy_amd.train import flatten_filter_weights
    nn, atoms = _default_nn(), fcc(rep=(2, 2, 2), jitter=0.05)
    new = copy.deepcopy(nn)
    rng = np.random.RandomState(5)
    new.descriptor.filter_weights = [(W + 0.05 * rng.normal(size=np.shape(W)), b) for W, b in nn.descriptor.filter_weights]
    with Engine(nn) as eng, Engine(new) as fresh:
        eng.set_filter_tables(True)
        old = eng.evaluate([atoms])[0]
        eng.update_filter_weights(flatten_filter_weights(new))
        assert eng.filter_table_knots == FILTER_TABLE_KNOTS
        eng.compute(ALL)
        got = eng._per_frame(eng.fetch(ALL))[0]
        ref = fresh.evaluate([atoms])[0]
    assert abs(got["energy"] - old["energy"]) > 1e-6      # the new network, not the old table
    _close(got, ref, "after update_filter_weights")


def test_training_turns_tables_off_for_good(lib):
    from tensoralloy_amd import Engine
    from tensoralloy_amd.train import Trainer
    frames = [fcc(rep=(1, 1, 2), jitter=0.1, seed=30 + k) for k in range(3)]
    par = {"hidden_sizes": [16, 16], "num_filters": 8}
    nn = make_grap_nn(["Ni"], 5.0, [16], "nn", par, moment_tensors=[0, 1, 2, 3])
    teacher = copy.deepcopy(nn)
    w, b = teacher.descriptor.filter_weights[-1]
    teacher.descriptor.filter_weights[-1] = (w * 1.3, b)
    with Engine(teacher) as eng:
        res = eng.evaluate(frames)
    labels = ([r["energy"] for r in res], [r["forces"] for r in res], np.array([r["stress"] for r in res]))
    grads = []
    for tables in (True, False):
        tr = Trainer(copy.deepcopy(nn), frames, *labels, train_filters=True)
        if tables:
            tr.engine.set_filter_tables(True)
            assert tr.engine.filter_table_knots == FILTER_TABLE_KNOTS
        grads.append(tr.loss_and_gradient())
        assert tr.engine.filter_table_knots == 0
        if tables:
            tr.engine.set_filter_tables(True)          # ignored from here on
            assert tr.engine.filter_table_knots == 0
        tr.close()
    (l1, _, g1), (l0, _, g0) = grads
    assert abs(l1 - l0) <= 1e-12 * abs(l0)
    assert np.abs(g0).max() > 0
    assert np.abs(g1 - g0).max() <= 1e-12 * np.abs(g0).max()
    # ... and the plain weight gradient of an engine that had tables on
    c = np.ones(len(frames))
    with Engine(nn) as a, Engine(nn) as b2:
        a.set_filter_tables(True)
        a.set_frames(frames)
        a.compute(ALL)                                  # descriptors of the table are resident
        b2.set_frames(frames)
        ga, gb = a.energy_gradient(c), b2.energy_gradient(c)
        assert a.filter_table_knots == 0
        a.set_filter_tables(True)
        assert a.filter_table_knots == 0
    assert np.abs(ga - gb).max() <= 1e-12 * np.abs(gb).max()


def test_force_loss_gradient_with_frozen_filters_turns_tables_off(lib):
    """`ta_loss_gradient` (forces and stress, the filters frozen) needs pair Jacobians of the exact network:
    through `Trainer(train_filters=False)` and on a bare engine with the table's descriptors resident."""
    from tensoralloy_amd import Engine
    from tensoralloy_amd.train import Trainer
    frames = [fcc(rep=(1, 1, 2), jitter=0.1, seed=40 + k) for k in range(2)]
    nn = make_grap_nn(["Ni"], 5.0, [16], "nn", {"hidden_sizes": [16, 16], "num_filters": 8}, moment_tensors=[0, 1, 2, 3])
    teacher = copy.deepcopy(nn)
    w, b = teacher.descriptor.filter_weights[-1]
    teacher.descriptor.filter_weights[-1] = (w * 1.3, b)
    with Engine(teacher) as eng:
        res = eng.evaluate(frames)
    labels = ([r["energy"] for r in res], [r["forces"] for r in res], np.array([r["stress"] for r in res]))
    out = []
    for tables in (True, False):
        tr = Trainer(copy.deepcopy(nn), frames, *labels)
        if tables:
            tr.engine.set_filter_tables(True)
        out.append(tr.loss_and_gradient())
        tr.engine.set_filter_tables(True)
        assert tr.engine.filter_table_knots == 0
        tr.close()
    (l1, _, g1), (l0, _, g0) = out
    assert abs(l1 - l0) <= 1e-12 * abs(l0)
    assert np.abs(g0).max() > 0 and np.abs(g1 - g0).max() <= 1e-12 * np.abs(g0).max()
    rng = np.random.RandomState(11)
    n = sum(len(f) for f in frames)
    c, dR, dh = rng.normal(size=len(frames)), rng.normal(size=(n, 3)), rng.normal(size=(len(frames), 3, 3)) * 0.1
    with Engine(nn) as a, Engine(nn) as ref:
        a.set_filter_tables(True)
        a.set_frames(frames)
        a.compute(ALL)
        ref.set_frames(frames)
        ga, gr = a.loss_gradient(c, dR, dh), ref.loss_gradient(c, dR, dh)
        assert a.filter_table_knots == 0
        a.set_filter_tables(True)
        assert a.filter_table_knots == 0
    assert np.abs(gr).max() > 0 and np.abs(ga - gr).max() <= 1e-12 * np.abs(gr).max()


def test_td_loss_gradient_turns_tables_off(lib):
    """`ta_td_loss_gradient` with a force direction on a temperature-dependent GRAP `nn` model."""
    from tensoralloy_amd import Engine
    from tensoralloy_amd.td import TemperatureDependentAtomicNN
    base = make_grap_nn(["Ni"], 5.0, [16], "nn", {"hidden_sizes": [16, 16], "num_filters": 8},
                        moment_tensors=[0, 1, 2, 3])
    td = TemperatureDependentAtomicNN(base.elements, base.descriptor, hidden_sizes=[8], activation="softplus",
                                      export_properties=("energy", "forces", "stress"),
                                      finite_temperature={"activation": "softplus", "layers": [4], "algo": "default"})
    td.attach_transformer(base.transformer)
    td.initialize(seed=3, bias_scale=0.1)
    frames = [fcc(rep=(1, 1, 2), jitter=0.1, seed=50), fcc(rep=(1, 1, 1), jitter=0.1, seed=51)]
    for a, T in zip(frames, (0.3, 0.8)):
        a.info["etemperature"] = T
    rng = np.random.RandomState(12)
    n, F = sum(len(f) for f in frames), len(frames)
    cf, cu, cs = rng.normal(size=F), rng.normal(size=F), rng.normal(size=F)
    dR, dh = rng.normal(size=(n, 3)), rng.normal(size=(F, 3, 3)) * 0.1
    with Engine(td) as a, Engine(td) as ref:
        a.set_filter_tables(True)
        a.set_frames(frames)
        a.compute(ALL)
        assert a.filter_table_knots == FILTER_TABLE_KNOTS
        ref.set_frames(frames)
        ga, gr = a.td_loss_gradient(cf, cu, cs, dR, dh), ref.td_loss_gradient(cf, cu, cs, dR, dh)
        assert a.filter_table_knots == 0
        a.set_filter_tables(True)
        assert a.filter_table_knots == 0
    assert np.abs(gr).max() > 0 and np.abs(ga - gr).max() <= 1e-12 * np.abs(gr).max()


def test_hessian_vectors_are_those_of_the_exact_network(lib):
    from tensoralloy_amd import Engine
    nn = make_grap_nn(["Ni"], 6.0, [16], "nn", moment_tensors=[0, 1, 2])
    atoms = fcc(rep=(2, 2, 2), seed=3, jitter=0.1)
    rng = np.random.RandomState(2)
    dR = rng.normal(size=(2, len(atoms), 3))
    dh = rng.normal(size=(2, 1, 3, 3)) * 0.3
    with Engine(nn) as eng, Engine(nn) as exact:
        exact.set_frames([atoms])
        ref_F, ref_W = exact.hessian_vectors(dR=dR, dh=dh, want_virial=True)
        x = exact.evaluate([atoms])[0]
        eng.set_filter_tables(True)
        eng.set_frames([atoms])
        eng.compute(ALL)
        dF, dW = eng.hessian_vectors(dR=dR, dh=dh, want_virial=True)
        assert eng.filter_table_knots == FILTER_TABLE_KNOTS
        eng.compute(ALL)
        after = eng._per_frame(eng.fetch(ALL))[0]
    assert np.abs(dF - ref_F).max() <= 1e-12 * np.abs(ref_F).max()
    assert np.abs(dW - ref_W).max() <= 1e-12 * np.abs(ref_W).max()
    _close(after, x, "after hessian_vectors")


def test_frame_without_pairs(lib):
    from tensoralloy_amd import Atoms, Engine
    nn = _default_nn()
    atom = Atoms(symbols=["Ni"], positions=[[10.0, 10.0, 10.0]], cell=np.eye(3) * 20.0, pbc=False)
    with Engine(nn) as eng:
        eng.set_filter_tables(True)
        tab = eng.evaluate([atom])[0]
        eng.set_filter_tables(False)
        exact = eng.evaluate([atom])[0]
    _close(tab, exact, "one atom")
    assert np.abs(tab["forces"]).max() == 0.0


def test_no_op_on_analytic_filters_and_bad_knot_counts(lib):
    from tensoralloy_amd import Engine
    atoms = fcc(rep=(2, 2, 2))
    pexp = make_grap_nn(["Ni"], 6.0, [16], moment_tensors=[0, 1, 2, 3])
    with Engine(pexp) as eng:
        before = eng.evaluate([atoms])[0]
        eng.set_filter_tables(True)
        assert eng.filter_table_knots == 0
        after = eng.evaluate([atoms])[0]
    for key in ("energy", "forces", "virial", "atomic"):
        assert np.array_equal(before[key], after[key])
    with Engine(_default_nn()) as eng:
        for bad in (4, -1, (1 << 20) + 2):
            with pytest.raises(ValueError):
                eng.set_filter_tables(True, knots=bad)
        assert eng.filter_table_knots == 0
        eng.set_filter_tables(True, knots=5)
        assert eng.filter_table_knots == 5


def test_temperature_dependent_model(lib):
    """U, S, F and the forces of a TemperatureDependentAtomicNN over GRAP `nn` filters."""
    from tensoralloy_amd import Engine
    from tensoralloy_amd.td import TemperatureDependentAtomicNN
    base = make_grap_nn(["Ni"], 5.5, [16], "nn", {"hidden_sizes": [16, 16], "num_filters": 8},
                        moment_tensors=[0, 1, 2, 3])
    td = TemperatureDependentAtomicNN(base.elements, base.descriptor, hidden_sizes=[8], activation="softplus",
                                      export_properties=("energy", "forces", "stress"),
                                      finite_temperature={"activation": "softplus", "layers": [4], "algo": "default"})
    td.attach_transformer(base.transformer)
    td.initialize(seed=3, bias_scale=0.1)
    frames = [fcc(rep=(2, 2, 2), jitter=0.05), fcc(rep=(1, 1, 2), jitter=0.05, seed=4)]
    for a, T in zip(frames, (0.3, 0.8)):
        a.info["etemperature"] = T
    with Engine(td) as eng:
        eng.set_filter_tables(True)
        assert eng.filter_table_knots == FILTER_TABLE_KNOTS
        tab = eng.evaluate(frames)
        eng.set_filter_tables(False)
        exact = eng.evaluate(frames)
    for t, x in zip(tab, exact):
        _close(t, x, "td")
        assert abs(t["free_energy"] - x["free_energy"]) < TE
        assert abs(t["eentropy"] - x["eentropy"]) < TE
