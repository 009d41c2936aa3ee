"""CPU references for training the GRAP `nn` filter network: the energy + forces + stress functional
sum_f c_f E_f + sum u.F + sum Y.W of the fp64 oracle (oracle/grap.py) with the filter network replaced by a
flat parameter vector, and its central difference along a direction in that vector."""
import copy

import numpy as np

from oracle.train import central_difference_6
from tensoralloy_amd.train import unflatten_filter_weights
from tests.helpers import oracle_grap_eval


def oracle_filter_functional(nn, frames, theta_f, c, u=None, Y=None):
    """sum_f c_f E_f + sum u.F + sum Y.W of the oracle with filter network `theta_f` (flat layout of
    `ta_filter_param_count`); u, Y = None: the energy term only."""
    trial = copy.deepcopy(nn)
    trial.descriptor.filter_weights = unflatten_filter_weights(trial, theta_f)
    total = 0.0
    for f, a in enumerate(frames):
        o = oracle_grap_eval(trial, a)
        total += c[f] * o["energy"]
        if u is not None:
            total += float(np.sum(u[f] * o["forces"])) + float(np.sum(Y[f] * o["virial"]))
    return total


def filter_directional_fd(nn, frames, theta_f, direction, c, u=None, Y=None, h=1e-3):
    """7-point central difference of `oracle_filter_functional` along `direction` (error O(h^6))."""
    return central_difference_6(lambda t: oracle_filter_functional(nn, frames, theta_f + t * direction, c, u, Y),
                                0.0, h)


def random_direction(frames, rng, u_scale=0.3, y_scale=0.05):
    """Random u per atom and symmetric Y per frame, and the (dR, dh) they make: dR = R.Y - u, dh = h.Y."""
    u = [rng.normal(0, u_scale, (len(a), 3)) for a in frames]
    Y = []
    for _ in frames:
        y = rng.normal(0, y_scale, (3, 3))
        Y.append(0.5 * (y + y.T))
    dR = np.concatenate([a.positions @ Y[k] - u[k] for k, a in enumerate(frames)])
    dh = np.array([np.asarray(a.get_cell(complete=True)) @ Y[k] for k, a in enumerate(frames)])
    return u, Y, dR, dh
