"""GPU: training the GRAP `nn` filter network together with the atomic networks (`ta_grap_loss_gradient`,
`ta_update_filter_weights`, `Trainer(train_filters=True)`). References: central differences in the filter
parameters of the fp64 oracle's energy + forces + stress functional (tests/grap_filter_reference.py), and
the existing MLP-only gradients of the same handle."""
import copy

import numpy as np
import pytest

from tensoralloy_amd import Engine, _lib
from tensoralloy_amd.train import Trainer, filter_trainable_mask, flatten_filter_weights
from tests.grap_filter_reference import filter_directional_fd, random_direction
from tests.helpers import fcc, make_grap_nn, make_nn
from tests.test_gpu_sf import _alloy

pytestmark = pytest.mark.gpu

ALL = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES | _lib.TA_WANT_VIRIAL | _lib.TA_WANT_ATOMIC
RCUT = 4.75   # between the third (4.3 A) and fourth (5.0 A) shells of the jittered fcc cells


def _model(elements=("Ni",), K=8, hidden=(16, 16), activation="softplus", resnet=True, modifier=0,
           moments=(0, 1, 2, 3), minmax=False, seed=611):
    par = {"hidden_sizes": list(hidden), "num_filters": K, "activation": activation, "use_resnet_dt": resnet,
           "h_abck_modifier": modifier}
    return make_grap_nn(list(elements), RCUT, [16], "nn", par, moment_tensors=list(moments), minmax=minmax,
                        seed=seed)


def _frames(elements=("Ni",)):
    """A multi-frame batch of uneven frames."""
    if len(elements) == 1:
        return [fcc(rep=(1, 1, 2), jitter=0.08, seed=21), fcc(rep=(1, 1, 1), jitter=0.08, seed=22)]
    return [_alloy(["Ni", "Ni", "Mo"], rep=(1, 1, 2)), _alloy(["Ni", "Mo"], rep=(1, 1, 1), seed=8)]


def _directions(mask, rng, n_random, coords):
    """Random unit directions over the real parameters (the oracle has no output bias), then coordinates."""
    n = len(mask)
    out = [d / np.linalg.norm(d) for d in (rng.normal(0, 1, n) * mask for _ in range(n_random))]
    for i in coords:
        e = np.zeros(n)
        e[i] = 1.0
        out.append(e)
    return out


def _check_filter_part(nn, frames, g_filter, c, u, Y, rng, n_random, n_coords, tol=1e-6):
    theta = flatten_filter_weights(nn)
    mask = filter_trainable_mask(nn)
    coords = rng.choice(np.flatnonzero(mask), n_coords, replace=False)
    scale = np.linalg.norm(g_filter * mask)
    for d in _directions(mask, rng, n_random, coords):
        fd = filter_directional_fd(nn, frames, theta, d, c, u, Y)
        mine = float(np.dot(g_filter, d))
        assert abs(mine - fd) <= tol * max(abs(fd), 1e-3 * scale), (mine, fd)


def test_energy_term_matches_oracle(lib):
    """ta_grap_loss_gradient(c, NULL, NULL): the filter part against the central difference of the oracle's
    sum_f c_f E_f along 3 random directions and 5 coordinates; the MLP part against ta_energy_gradient."""
    rng = np.random.RandomState(3)
    nn, frames = _model(), _frames()
    c = rng.normal(0, 1, len(frames))
    with Engine(nn) as eng:
        eng.set_frames(frames)
        nw, nf = eng.param_count(), eng.filter_param_count()
        assert nf == len(flatten_filter_weights(nn))
        g = eng.grap_loss_gradient(c)
        assert len(g) == nw + nf
        g_mlp = eng.energy_gradient(c)
    assert np.abs(g[:nw] - g_mlp).max() <= 1e-12 * max(1.0, np.abs(g_mlp).max())
    _check_filter_part(nn, frames, g[nw:], c, None, None, rng, 3, 5)


def test_forces_stress_term_matches_oracle(lib):
    """Random u and Y: the filter part against the central difference of the oracle's sum_f c_f E_f + sum u.F
    + sum Y.W; the MLP part against ta_loss_gradient (pair Jacobian path) of the same direction."""
    rng = np.random.RandomState(4)
    nn, frames = _model(), _frames()
    c = rng.normal(0, 1, len(frames))
    u, Y, dR, dh = random_direction(frames, rng)
    with Engine(nn) as eng:
        eng.set_frames(frames)
        nw = eng.param_count()
        g = eng.grap_loss_gradient(c, dR, dh)
        g_again = eng.grap_loss_gradient(c, dR, dh)
        g_mlp = eng.loss_gradient(c, dR, dh)
    assert np.array_equal(g, g_again)   # deterministic: no float atomics on the result
    assert np.abs(g[:nw] - g_mlp).max() <= 1e-12 * max(1.0, np.abs(g_mlp).max())
    _check_filter_part(nn, frames, g[nw:], c, u, Y, rng, 3, 5)


SHAPES = {
    "MoNi": dict(elements=("Mo", "Ni")),
    "modifier1": dict(modifier=1),
    "modifier2": dict(modifier=2),
    "no_resnet": dict(resnet=False),
    "tanh": dict(activation="tanh"),
    "moments012": dict(moments=(0, 1, 2)),
    "moments0to5": dict(moments=(0, 1, 2, 3, 4, 5), K=8),
    "K16": dict(K=16, hidden=(32, 32, 32)),
    "K32_minmax": dict(K=32, hidden=(24,), minmax=True),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_shapes_match_oracle(lib, shape):
    """Elements, input modifiers, ResNet off, tanh, moments 0..2 / 0..5, K = 8 / 16 / 32, minmax on: the
    whole (energy + forces + stress) gradient's filter part along 2 random directions and 2 coordinates."""
    kw = dict(SHAPES[shape])
    elements = kw.get("elements", ("Ni",))
    rng = np.random.RandomState(sum(map(ord, shape)))
    nn, frames = _model(**kw), _frames(elements)
    c = rng.normal(0, 1, len(frames))
    u, Y, dR, dh = random_direction(frames, rng)
    with Engine(nn) as eng:
        eng.set_frames(frames)
        nw = eng.param_count()
        g = eng.grap_loss_gradient(c, dR, dh)
        g_mlp = eng.loss_gradient(c, dR, dh)
    assert np.abs(g[:nw] - g_mlp).max() <= 1e-12 * max(1.0, np.abs(g_mlp).max())
    _check_filter_part(nn, frames, g[nw:], c, u, Y, rng, 2, 2)


def test_update_filter_weights_matches_fresh_engine(lib):
    """After ta_update_filter_weights a live handle agrees with a fresh one: energies, forces, virials, then
    ta_loss_gradient and ta_hessian_vectors (pair Jacobian and descriptors rebuilt, not stale), and
    energies(reuse_descriptors=True) sees the new filters."""
    rng = np.random.RandomState(5)
    nn, frames = _model(), _frames()
    c = rng.normal(0, 1, len(frames))
    _, _, dR, dh = random_direction(frames, rng)
    new = copy.deepcopy(nn)
    new.descriptor.initialize_filters(seed=99, bias_scale=0.1)
    flat_new = flatten_filter_weights(new)
    with Engine(nn) as live, Engine(new) as fresh:
        live.set_frames(frames)
        fresh.set_frames(frames)
        e_old = live.energies(reuse_descriptors=False)
        live.loss_gradient(c, dR, dh)                  # pair Jacobian and descriptors of the old network
        live.hessian_vectors(dR[None], dh[None])
        live.update_filter_weights(flat_new)           # same resident batch: nothing may be reused
        e_reuse = live.energies(reuse_descriptors=True)
        e_fresh = fresh.energies(reuse_descriptors=False)
        assert np.abs(e_reuse - e_old).max() > 1e-6
        assert np.abs(e_reuse - e_fresh).max() < 1e-12 * max(1.0, np.abs(e_fresh).max())
        g_live = live.loss_gradient(c, dR, dh)
        g_fresh = fresh.loss_gradient(c, dR, dh)
        assert np.abs(g_live - g_fresh).max() <= 1e-12 * max(1.0, np.abs(g_fresh).max())
        h_live = live.hessian_vectors(dR[None], dh[None])
        h_fresh = fresh.hessian_vectors(dR[None], dh[None])
        assert np.abs(h_live - h_fresh).max() < 1e-12 * max(1.0, np.abs(h_fresh).max())
        gg_live = live.grap_loss_gradient(c, dR, dh)
        gg_fresh = fresh.grap_loss_gradient(c, dR, dh)
        assert np.abs(gg_live - gg_fresh).max() <= 1e-12 * max(1.0, np.abs(gg_fresh).max())
        live.compute(ALL)
        got = live._per_frame(live.fetch(ALL))
        fresh.compute(ALL)
        ref = fresh._per_frame(fresh.fetch(ALL))
        for a, b in zip(got, ref):
            assert abs(a["energy"] - b["energy"]) < 1e-12 * max(1.0, abs(b["energy"]))
            assert np.abs(a["forces"] - b["forces"]).max() < 1e-12
            assert np.abs(a["virial"] - b["virial"]).max() < 1e-12
        with pytest.raises(ValueError, match="expected"):
            live.update_filter_weights(flat_new[:-1])


def _teacher_data(teacher, frames):
    with Engine(teacher) as eng:
        res = eng.evaluate(frames)
    return ([r["energy"] for r in res], [r["forces"] for r in res], np.array([r["stress"] for r in res]))


def test_trainer_fits_the_filters(lib, tmp_path):
    """A teacher and a student that share the MLP weights but not the filter network: train_filters=True
    lowers the energy + forces + stress loss at least fourfold in 40 steps and moves the filters;
    train_filters=False keeps them bit-identical; after fit() the native export reproduces the trained
    engine."""
    from tensoralloy_amd.model import load_lammps_native
    frames = [fcc(rep=(1, 1, 2), jitter=0.1, seed=30 + k) for k in range(4)]
    teacher = _model(K=8, hidden=(16, 16))
    labels = _teacher_data(teacher, frames)
    student = copy.deepcopy(teacher)
    w, b = student.descriptor.filter_weights[-1]
    student.descriptor.filter_weights[-1] = (w * 1.3, b)
    before = copy.deepcopy(student.descriptor.filter_weights)
    tr = Trainer(student, frames, *labels, train_filters=True, learning_rate=2e-3)
    hist = tr.fit(40)
    first, last = hist[0]["total"], hist[-1]["total"]
    assert last < first / 4, (first, last)
    assert any(np.abs(w1 - w0).max() > 0 for (w0, _), (w1, _) in zip(before, student.descriptor.filter_weights))
    assert student.descriptor.filter_weights[-1][1] is None          # the output layer keeps no bias
    e_trained = tr.engine.energies(reuse_descriptors=False)
    tr.close()
    nn2, _, _ = load_lammps_native(student.export_to_lammps_native(str(tmp_path / "trained.npz")))
    with Engine(nn2) as eng:
        eng.set_frames(frames)
        e_native = eng.energies(reuse_descriptors=False)
    assert np.abs(e_native - e_trained).max() < 1e-12 * max(1.0, np.abs(e_trained).max())
    # today's behaviour: the filters stay put
    frozen = copy.deepcopy(teacher)
    w, b = frozen.descriptor.filter_weights[-1]
    frozen.descriptor.filter_weights[-1] = (w * 1.3, b)
    flat0 = flatten_filter_weights(frozen)
    tr = Trainer(frozen, frames, *labels, learning_rate=2e-3)
    tr.fit(5)
    e_frozen = tr.engine.energies(reuse_descriptors=False)
    tr.close()
    assert np.array_equal(flatten_filter_weights(frozen), flat0)
    with Engine(frozen) as eng:       # the trained MLP on the untouched filters: what the trainer's engine had
        eng.set_frames(frames)
        assert np.array_equal(eng.energies(reuse_descriptors=False), e_frozen)


def test_refusals(lib):
    """train_filters=True needs a trainable GRAP/nn filter network, analytic gradients and a model that is not
    temperature-dependent; ta_grap_loss_gradient returns TA_ERR_UNSUPPORTED for other models."""
    from tensoralloy_amd.td import TemperatureDependentAtomicNN
    frames = _frames()
    e = [0.0] * len(frames)
    sf = make_nn(["Ni"], RCUT, False, [8])
    pexp = make_grap_nn(["Ni"], RCUT, [8], moment_tensors=[0, 1])
    for other in (sf, pexp):
        with pytest.raises(ValueError, match="filter network"):
            Trainer(other, frames, e, train_filters=True)
        with Engine(other) as eng:
            assert eng.filter_param_count() == 0
            eng.set_frames(frames)
            with pytest.raises(ValueError, match="ta_grap_loss_gradient"):
                eng.grap_loss_gradient(np.ones(len(frames)))
            with pytest.raises(ValueError, match="no filter network"):
                eng.update_filter_weights(np.zeros(3))
    nn = _model()
    with pytest.raises(ValueError, match="analytic"):
        Trainer(nn, frames, e, train_filters=True, analytic=False)
    frozen = _model()
    frozen.descriptor.algorithm.trainable = False
    with pytest.raises(ValueError, match="trainable=False"):
        Trainer(frozen, frames, e, train_filters=True)
    td = TemperatureDependentAtomicNN(nn.elements, nn.descriptor, hidden_sizes=[8], activation="softplus",
                                      export_properties=("energy", "forces", "stress"),
                                      finite_temperature={"activation": "softplus", "layers": [4], "algo": "default"})
    td.attach_transformer(nn.transformer)
    td.initialize(seed=3, bias_scale=0.1)
    with pytest.raises(ValueError, match="temperature-dependent"):
        Trainer(td, frames, e, train_filters=True)
    for a in frames:
        a.info["etemperature"] = 0.5
    with Engine(td) as eng:
        eng.set_frames(frames)
        eng.set_electron_temperatures([0.5] * len(frames))
        with pytest.raises(ValueError, match="temperature-dependent"):
            eng.grap_loss_gradient(np.ones(len(frames)))
