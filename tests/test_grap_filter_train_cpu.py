"""CPU: the GRAP `nn` filter network's flat parameter layout and the refusals of `Trainer(train_filters=True)`
(raised before any engine is created)."""
import numpy as np
import pytest

from tensoralloy_amd.train import (Trainer, filter_trainable_mask, flatten_filter_weights,
                                   unflatten_filter_weights)
from tests.helpers import fcc, make_grap_nn, make_nn


def _nn(**par):
    base = {"hidden_sizes": [8, 8], "num_filters": 4}
    base.update(par)
    return make_grap_nn(["Ni"], 4.75, [8], "nn", base, moment_tensors=[0, 1])


def test_filter_layout_round_trip():
    nn = _nn()
    flat = flatten_filter_weights(nn)
    # the layout of GenericRadialAtomicPotential.flat_parameters' network block: W [in][out], then b [out]
    sizes = [1, 8, 8, 4]
    assert len(flat) == sum(sizes[l] * sizes[l + 1] + sizes[l + 1] for l in range(3))
    head = 6 + 4 + len(sizes)
    assert np.array_equal(nn.descriptor.flat_parameters()[head:], flat)
    back = unflatten_filter_weights(nn, flat * 2.0)
    for (w0, b0), (w1, b1) in zip(nn.descriptor.filter_weights, back):
        assert np.array_equal(w1, 2.0 * np.asarray(w0))
        assert (b0 is None and b1 is None) or np.array_equal(b1, 2.0 * np.asarray(b0))
    assert back[-1][1] is None   # no output bias (grap.py:640)
    mask = filter_trainable_mask(nn)
    assert mask.sum() == len(flat) - 4 and not mask[-4:].any()


def test_train_filters_refusals():
    from tensoralloy_amd.td import TemperatureDependentAtomicNN
    frames = [fcc(rep=(1, 1, 1))]
    e = [0.0]
    for other in (make_nn(["Ni"], 4.75, False, [8]), make_grap_nn(["Ni"], 4.75, [8], moment_tensors=[0, 1])):
        with pytest.raises(ValueError, match="filter network"):
            Trainer(other, frames, e, train_filters=True)
    with pytest.raises(ValueError, match="analytic"):
        Trainer(_nn(), frames, e, train_filters=True, analytic=False)
    frozen = _nn(trainable=False)
    with pytest.raises(ValueError, match="trainable=False"):
        Trainer(frozen, frames, e, train_filters=True)
    nn = _nn()
    td = TemperatureDependentAtomicNN(nn.elements, nn.descriptor, hidden_sizes=[8], activation="softplus",
                                      export_properties=("energy", "forces", "stress"),
                                      finite_temperature={"activation": "softplus", "layers": [4], "algo": "default"})
    td.attach_transformer(nn.transformer)
    td.initialize(seed=3, bias_scale=0.1)
    with pytest.raises(ValueError, match="temperature-dependent"):
        Trainer(td, frames, None, free_energies=e, train_filters=True)
