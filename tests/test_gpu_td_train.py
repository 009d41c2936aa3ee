"""GPU: training of temperature-dependent models: `ta_td_loss_gradient` (csrc/ta_td_train.hip) against the
NumPy restatement (tests/td_train_reference.py) on the engine's own descriptors and tangents, the whole
U + F + S + forces + stress loss against central differences of the oracle's loss, the parameter layout
and weight updates, refusals, and the trainer on a teacher and on the Be fixture."""
from pathlib import Path

import numpy as np
import pytest

from tensoralloy_amd import Engine, _lib
from tensoralloy_amd.td import TemperatureDependentAtomicNN
from tensoralloy_amd.train import (Trainer, energy_loss, flatten_weights, forces_loss, stress_loss,
                                   trainable_mask, unflatten_weights)
from tests.helpers import fcc, hcp, make_grap_nn, make_nn
from tests.td_reference import oracle_td_eval
from tests.td_train_reference import td_loss_gradient_reference

pytestmark = pytest.mark.gpu

ALL = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES | _lib.TA_WANT_VIRIAL | _lib.TA_WANT_ATOMIC
TEMPERATURES = (0.0, 0.45, 1.3)


def td_from(base, layers, hidden, algo="default", resnet=True, minmax=False, act_h="softplus",
            activation="softplus", seed=7, static=None):
    nn = TemperatureDependentAtomicNN(base.elements, base.descriptor, hidden_sizes=list(hidden),
                                      activation=activation, minmax_scale=minmax, use_resnet_dt=resnet,
                                      atomic_static_energy=static or {},
                                      export_properties=("energy", "forces", "stress"),
                                      finite_temperature={"activation": act_h, "layers": list(layers),
                                                          "algo": algo})
    nn.attach_transformer(base.transformer)
    nn.initialize(seed=seed, bias_scale=0.1)
    if minmax:
        rng = np.random.RandomState(seed + 1)
        D = nn.ndim()
        for el in nn.elements:
            nn.minmax[el] = (rng.rand(D) * 0.1, 1.0 + rng.rand(D) * 5.0)
    return nn


def _base(desc, elements):
    if desc == "sf":
        return make_nn(elements, 4.5, True, [16], sf_kwargs={"eta": [0.1, 1.0], "omega": [0.0], "beta": [0.005],
                                                             "gamma": [1.0, -1.0], "zeta": [1.0, 4.0]})
    return make_grap_nn(elements, 4.5, [16], algorithm="pexp", moment_tensors=(0, 1, 2))


def _frames(desc, elements, temperatures=TEMPERATURES, small=False):
    out = []
    for k, T in enumerate(temperatures):
        if desc == "sf":
            a = fcc("Ni", rep=(1, 1, 2) if small else (2, 2, 1 + k % 2), jitter=0.08, seed=20 + k)
        else:
            a = hcp("Be", rep=(2, 2, 1) if small else (2, 2, 2), jitter=0.08, seed=30 + k)
        if len(elements) == 2:
            syms = [elements[0] if i % (2 + k) == 0 else elements[1] for i in range(len(a))]
            a = a.__class__(symbols=syms, positions=a.positions, cell=a.get_cell(complete=True), pbc=a.pbc)
        a.info["etemperature"] = T
        out.append(a)
    return out


# the grid: descriptor x algo x elements x min-max (ResNet on); activations vary along the rows
ROWS = []
for _desc in ("sf", "grap"):
    for _algo in ("default", "Sommerfeld"):
        for _els in (("Ni",), ("Mo", "Ni")) if _desc == "sf" else (("Be",), ("Be", "Mo")):
            for _mm in (False, True):
                ROWS.append((f"{_desc}-{_algo}-{len(_els)}el-{'minmax' if _mm else 'raw'}", _desc, _algo, _els, _mm))
ACTS = [("softplus", "softplus"), ("tanh", "squareplus"), ("elu", "tanh"), ("squareplus", "softplus")]


def _row_model(row, k, layers=(20, 20, 9), hidden=(16, 16), seed=7):
    _, desc, algo, els, mm = row
    act_h, act = ACTS[k % len(ACTS)]
    static = {el: -1.0 - 0.5 * i for i, el in enumerate(els)}
    return td_from(_base(desc, list(els)), layers, hidden, algo=algo, minmax=mm, act_h=act_h, activation=act,
                   seed=seed, static=static)


def _per_atom(frames, per_frame):
    return np.concatenate([np.full(len(a), float(v)) for a, v in zip(frames, per_frame)])


def _symbols(frames):
    return [s for a in frames for s in a.get_chemical_symbols()]


def _assert_td_close(r, o, what=""):
    for key, ref in (("free_energy", o["energy"]), ("energy", o["U"]), ("eentropy", o["S"])):
        assert abs(r[key] - ref) <= 1e-9 * max(1.0, abs(ref)), (what, key, r[key], ref)
    assert np.abs(r["forces"] - o["forces"]).max() <= 1e-9 * max(1.0, np.abs(o["forces"]).max()), what
    assert np.abs(r["virial"] - o["virial"]).max() <= 1e-8 * max(1.0, np.abs(o["virial"]).max()), what


@pytest.mark.parametrize("k", range(len(ROWS)), ids=[r[0] for r in ROWS])
def test_param_count_and_weight_update(k, monkeypatch):
    row = ROWS[k]
    nn = _row_model(row, k)
    frames = _frames(row[1], row[3])
    theta = flatten_weights(nn)
    rng = np.random.RandomState(k)
    new = theta + 0.05 * rng.normal(size=theta.shape) * trainable_mask(nn)
    with Engine(nn, device=0) as eng:
        assert eng.param_count() == len(theta)
        eng.set_frames(frames)
        eng.compute(ALL)
        eng.update_weights(new)
        res = eng.evaluate(frames, want=ALL)
        with pytest.raises(ValueError):
            eng.update_weights(new[:-1])
    nn.weights = unflatten_weights(nn, new)
    for a, r in zip(frames, res):
        _assert_td_close(r, oracle_td_eval(nn, a, monkeypatch), f"{row[0]} T={a.info['etemperature']}")


def _engine_inputs(eng, frames):
    res = eng.evaluate(frames, want=ALL, descriptors=True)
    G = np.concatenate([r["descriptors"] for r in res])
    T = _per_atom(frames, [a.info["etemperature"] for a in frames])
    return res, G, T


@pytest.mark.parametrize("k", range(len(ROWS)), ids=[r[0] for r in ROWS])
def test_energy_terms_against_reference(k):
    row = ROWS[k]
    nn = _row_model(row, k)
    frames = _frames(row[1], row[3])
    F = len(frames)
    rng = np.random.RandomState(100 + k)
    a, b, g = rng.normal(size=F), rng.normal(size=F), rng.normal(size=F)
    zero = np.zeros(F)
    with Engine(nn, device=0) as eng:
        _, G, T = _engine_inputs(eng, frames)
        syms = _symbols(frames)
        dG = np.zeros_like(G)
        for ca, cb, cg in ((a, None, None), (None, b, None), (None, None, g), (a, b, g)):
            got = eng.td_loss_gradient(cb, ca, cg)
            ref = td_loss_gradient_reference(nn, syms, G, dG, T, *(_per_atom(frames, zero if c is None else c)
                                                                  for c in (ca, cb, cg)))
            scale = max(1.0, np.abs(ref).max())
            assert np.abs(got - ref).max() <= 1e-9 * scale, (row[0], np.abs(got - ref).max())


@pytest.mark.parametrize("k", range(len(ROWS)), ids=[r[0] for r in ROWS])
def test_direction_term_against_reference(k):
    row = ROWS[k]
    nn = _row_model(row, k)
    frames = _frames(row[1], row[3])
    F = len(frames)
    N = sum(len(a) for a in frames)
    rng = np.random.RandomState(200 + k)
    a, b, g = rng.normal(size=F), rng.normal(size=F), rng.normal(size=F)
    dR, dh = rng.normal(size=(N, 3)), 0.1 * rng.normal(size=(F, 3, 3))
    with Engine(nn, device=0) as eng:
        _, G, T = _engine_inputs(eng, frames)
        got, dG = eng.td_loss_gradient(b, a, g, dR, dh, return_tangent=True)
        only_dir, dG2 = eng.td_loss_gradient(None, None, None, dR, dh, return_tangent=True)
    assert np.abs(dG).max() > 0.0 and np.array_equal(dG, dG2)
    syms = _symbols(frames)
    ref = td_loss_gradient_reference(nn, syms, G, dG, T, _per_atom(frames, a), _per_atom(frames, b),
                                     _per_atom(frames, g))
    scale = max(1.0, np.abs(ref).max())
    assert np.abs(got - ref).max() <= 1e-9 * scale, (row[0], np.abs(got - ref).max())
    zero = np.zeros(N)
    ref0 = td_loss_gradient_reference(nn, syms, G, dG, T, zero, zero, zero)
    assert np.abs(only_dir - ref0).max() <= 1e-9 * max(1.0, np.abs(ref0).max())


def _labels(teacher, frames):
    with Engine(teacher, device=0) as eng:
        res = eng.evaluate(frames, want=ALL)
    return dict(energies=np.array([r["energy"] for r in res]), free_energies=np.array([r["free_energy"] for r in res]),
                eentropies=np.array([r["eentropy"] for r in res]), forces=[r["forces"].copy() for r in res],
                stresses=np.array([r["stress"] for r in res]))


def _oracle_loss(nn, frames, lab, monkeypatch):
    outs = [oracle_td_eval(nn, a, monkeypatch) for a in frames]
    n = np.array([len(a) for a in frames], dtype=float)
    loss = energy_loss(np.array([o["U"] for o in outs]), lab["energies"], n)[0]
    loss += energy_loss(np.array([o["energy"] for o in outs]), lab["free_energies"], n)[0]
    loss += energy_loss(np.array([o["S"] for o in outs]), lab["eentropies"], n)[0]
    loss += forces_loss([o["forces"] for o in outs], lab["forces"])[0]
    loss += stress_loss(np.array([o["stress_voigt"] for o in outs]), lab["stresses"])[0]
    return loss


def _sampled_parameters(nn):
    """A first-layer weight and a hidden bias of every net, and every output weight and bias."""
    picks, off = [], 0
    for el, net in [(el, net) for net in ("H", "U", "S") for el in nn.elements]:
        layers = nn.weights[el][net]
        sizes = [(np.size(w), np.shape(w)[1]) for w, _ in layers]
        picks.append(off + 1)                       # W_0[0][1]
        picks.append(off + sizes[0][0] + 2)          # b_0[2] (a hidden bias)
        start = off + sum(nw + nb for nw, nb in sizes[:-1])
        picks.extend(range(start, start + sizes[-1][0] + sizes[-1][1]))
        off += sum(nw + nb for nw, nb in sizes)
    return picks


FD_ROWS = [0, 3, 9, 14]   # sf default 1el raw, sf default 2el minmax, grap default 1el minmax, grap Sommerfeld 2el raw


@pytest.mark.parametrize("k", FD_ROWS, ids=[ROWS[k][0] for k in FD_ROWS])
def test_whole_loss_against_oracle_central_differences(k, monkeypatch):
    row = ROWS[k]
    nn = _row_model(row, k, layers=(10, 10, 4), hidden=(8, 8), seed=3)
    teacher = _row_model(row, k, layers=(10, 10, 4), hidden=(8, 8), seed=5)
    frames = _frames(row[1], row[3], temperatures=(0.0, 0.6), small=True)
    lab = _labels(teacher, frames)
    tr = Trainer(nn, frames, device=0, **lab)
    total, terms, grad = tr.loss_and_gradient()
    tr.close()
    assert set(terms) == {"energy", "free_energy", "eentropy", "forces", "stress"}
    assert abs(total - _oracle_loss(nn, frames, lab, monkeypatch)) < 1e-9 * max(1.0, total)
    theta = flatten_weights(nn)
    mask = trainable_mask(nn)
    d = 1e-5
    for p in _sampled_parameters(nn):
        if mask[p] == 0.0:
            assert grad[p] == 0.0
            continue
        th = theta.copy()
        th[p] += d
        nn.weights = unflatten_weights(nn, th)
        lp = _oracle_loss(nn, frames, lab, monkeypatch)
        th[p] -= 2 * d
        nn.weights = unflatten_weights(nn, th)
        lm = _oracle_loss(nn, frames, lab, monkeypatch)
        nn.weights = unflatten_weights(nn, theta)
        fd = (lp - lm) / (2 * d)
        assert abs(fd - grad[p]) < 2e-6 * max(1.0, abs(fd)), (row[0], p, fd, grad[p])


def test_existing_entry_points_are_the_free_energy_case():
    row = ROWS[11]
    nn = _row_model(row, 11)
    frames = _frames(row[1], row[3])
    F, N = len(frames), sum(len(a) for a in frames)
    rng = np.random.RandomState(5)
    c, dR, dh = rng.normal(size=F), rng.normal(size=(N, 3)), 0.1 * rng.normal(size=(F, 3, 3))
    with Engine(nn, device=0) as eng:
        eng.evaluate(frames, want=ALL)
        e1 = eng.energy_gradient(c)
        e2 = eng.td_loss_gradient(c)
        l1 = eng.loss_gradient(c, dR, dh)
        l2 = eng.td_loss_gradient(c, None, None, dR, dh)
        l3 = eng.td_loss_gradient(c, None, None, dR, dh)
        full1 = eng.td_loss_gradient(c, c[::-1], -c, dR, dh)
        full2 = eng.td_loss_gradient(c, c[::-1], -c, dR, dh)
    assert np.array_equal(e1, e2) and np.abs(e1).max() > 0.0
    assert np.array_equal(l1, l2) and np.array_equal(l2, l3)
    assert np.array_equal(full1, full2)
    assert not np.array_equal(l1, e1)


def test_refusals_leave_the_handle_usable():
    row = ROWS[1]
    nn = _row_model(row, 1)
    frames = _frames(row[1], row[3])
    F, N = len(frames), sum(len(a) for a in frames)
    rng = np.random.RandomState(6)
    c, dR = rng.normal(size=F), rng.normal(size=(N, 3))
    with Engine(nn, device=0) as eng:
        eng.evaluate(frames, want=ALL)
        ref = eng.td_loss_gradient(c, c, c, dR)
        # a skin-filtered batch
        eng.set_skin(0.5)
        eng.set_frames(frames)
        eng.compute(ALL)
        with pytest.raises(ValueError, match="skin-filtered"):
            eng.td_loss_gradient(c, c, c, dR)
        with pytest.raises(ValueError, match="skin-filtered"):
            eng.loss_gradient(c, dR)
        eng.set_skin(0.0)
        eng.set_frames(frames)
        eng.compute(ALL)
        # a wrong n_grad
        grad = np.zeros(eng.param_count() - 1)
        null = _lib._dp()
        cc = np.ascontiguousarray(c)
        with pytest.raises(ValueError, match="expected room"):
            eng._check(eng._lib.ta_td_loss_gradient(eng._handle, _lib.as_dp(cc), null, null, null, null,
                                                    _lib.as_dp(grad), len(grad), null))
        # TD Hessians stay out of scope
        with pytest.raises(ValueError):
            eng.hessian_vectors(dR=dR[None])
        again = eng.td_loss_gradient(c, c, c, dR)
    # a rebuilt list may order the pairs differently: equal up to rounding
    assert np.abs(again - ref).max() < 1e-12 * max(1.0, np.abs(ref).max())
    plain = make_nn(["Ni"], 4.5, True, [8])
    with Engine(plain, device=0) as eng:
        eng.evaluate([fcc("Ni", rep=(1, 1, 1))], want=ALL)
        with pytest.raises(ValueError, match="not a temperature-dependent model"):
            eng.td_loss_gradient(np.ones(1))
        assert eng.energy_gradient(np.ones(1)).shape == (eng.param_count(),)


def test_trainer_analytic_against_central_difference():
    row = ROWS[7]   # sf Sommerfeld 2el minmax
    nn = _row_model(row, 7, layers=(12, 12, 6), hidden=(10, 10), seed=3)
    teacher = _row_model(row, 7, layers=(12, 12, 6), hidden=(10, 10), seed=9)
    frames = _frames(row[1], row[3], temperatures=(0.5, 1.2))
    lab = _labels(teacher, frames)
    grads = []
    for analytic in (True, False):
        tr = Trainer(nn, frames, device=0, analytic=analytic, **lab)
        grads.append(tr.loss_and_gradient()[2])
        tr.close()
    ga, gf = grads
    scale = max(1.0, np.abs(gf).max())
    assert np.abs(ga - gf).max() < 1e-5 * scale
    # at T = 0 the answer differs: the displaced copies must have kept each frame's temperature
    cold = [a.copy() for a in frames]
    for a in cold:
        a.info.pop("etemperature", None)
    tr = Trainer(nn, cold, device=0, analytic=True, **lab)
    g0 = tr.loss_and_gradient()[2]
    tr.close()
    assert np.abs(g0 - gf).max() > 1e-3 * scale


def test_teacher_fit():
    row = ROWS[2]   # sf default 2el raw
    teacher = _row_model(row, 2, layers=(16, 16, 8), hidden=(16,), seed=4)
    student = _row_model(row, 2, layers=(16, 16, 8), hidden=(16,), seed=4)
    rng = np.random.RandomState(12)
    theta = flatten_weights(teacher)
    student.weights = unflatten_weights(student, theta + 0.03 * rng.normal(size=theta.shape) * trainable_mask(student))
    frames = _frames(row[1], row[3], temperatures=(0.0, 0.2, 0.5, 0.9, 1.4))
    lab = _labels(teacher, frames)
    tr = Trainer(student, frames, device=0, learning_rate=0.005, decay_rate=0.05, decay_steps=200, **lab)
    hist = tr.fit(250)
    tr.close()
    assert set(hist[0]) == {"energy", "free_energy", "eentropy", "forces", "stress", "total"}
    assert hist[-1]["total"] < 0.1 * hist[0]["total"], (hist[0]["total"], hist[-1]["total"])


def test_be_fixture_fit_and_reload(tmp_path):
    from tensoralloy_amd import TensorAlloyCalculator
    from tensoralloy_amd.io import read_extxyz
    frames = read_extxyz(str(Path(__file__).parent / "golden" / "Be_liquid_4000K_TS.extxyz"))
    base = make_grap_nn(["Be"], 5.0, [32], algorithm="sf",
                        parameters={"eta": [0.1, 0.5, 1.0, 2.0, 4.0, 8.0], "omega": [0.0, 1.5, 3.0]},
                        moment_tensors=(0, 2), param_space_method="cross")
    nn = td_from(base, (32, 16), (32, 32), static={"Be": -3.0}, seed=11)
    voigt = [np.asarray(a.info["stress"]).reshape(3, 3) for a in frames]
    lab = dict(energies=[a.info["energy"] for a in frames], free_energies=[a.info["free_energy"] for a in frames],
               eentropies=[a.info["eentropy"] for a in frames], forces=[a.info["forces"] for a in frames],
               stresses=np.array([[s[0, 0], s[1, 1], s[2, 2], s[1, 2], s[0, 2], s[0, 1]] for s in voigt]))
    tr = Trainer(nn, frames, device=0, learning_rate=0.002, **lab)
    hist = tr.fit(50)
    assert set(hist[0]) == {"energy", "free_energy", "eentropy", "forces", "stress", "total"}
    final = tr.loss_and_gradient()[0]
    assert final < hist[0]["total"]
    res = tr.engine.evaluate(frames, want=ALL)
    tr.close()
    calc = TensorAlloyCalculator(nn.export(str(tmp_path / "be_td_trained.json")))
    for a, r in zip(frames, res):
        a.calc = calc
        for got, want in ((calc.get_potential_energy(a), r["energy"]), (calc.get_free_energy(a), r["free_energy"]),
                          (calc.get_electron_entropy(a), r["eentropy"])):
            assert abs(got - want) <= 1e-10 * max(1.0, abs(want)), (got, want)
