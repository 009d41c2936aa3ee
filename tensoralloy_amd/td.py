"""
Temperature-dependent atomistic networks (reference tensoralloy/nn/atomic/finite_temperature.py).

  FiniteTemperatureOptions      <- nn/atomic/dataclasses.py:27-33
  TemperatureDependentAtomicNN  <- finite_temperature.py:24-388 (model), :390-650 (native export)

For atom i of element e in a frame of electron temperature T (eV): H = H_e(minmax(G_i)) (hidden sizes
`finite_temperature.layers[:-1]`, linear output of width K = layers[-1] with bias), z = [H, T],
U_i = U_e(z), s_i = S_e(z) (hidden sizes `hidden_sizes[e]`, model activation; S always has an output
bias, U has one iff `use_atomic_static_energy`), S_i = s_i T for algo "Sommerfeld" else s_i, and
F_i = U_i - T S_i. Forces, stress and pressure derive from F (`variational_energy == "free_energy"`,
basic.py:186-201). All arithmetic happens in the HIP library: inference in csrc/ta_td.hip, the loss
gradient of training (`train.Trainer`, `Engine.td_loss_gradient`) in csrc/ta_td_train.hip.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List

import numpy as np

from . import _lib
from .model import NATIVE_ACTFN, AtomicNN
from .utils import Defaults

NETS = ("H", "U", "S")


@dataclass
class FiniteTemperatureOptions:
    """Options of the finite-temperature head (dataclasses.py:27-33). Any `algo` other than
    "Sommerfeld" is the default algorithm, as in the reference (finite_temperature.py:159)."""
    activation: str = "softplus"
    layers: tuple = (128, 128)
    algo: str = "default"

    def __post_init__(self):
        self.layers = tuple(int(x) for x in np.atleast_1d(self.layers))
        if not self.layers or min(self.layers) < 1:
            raise ValueError("finite_temperature.layers must list at least the width of H's output")
        if self.activation.lower() not in _lib.TA_ACT:
            raise ValueError(f"The activation function '{self.activation}' cannot be recognized!")

    def as_dict(self):
        return {"activation": self.activation, "layers": list(self.layers), "algo": self.algo}


def _he_normal(rng, fan_in, fan_out):
    """He-normal kernel truncated at 2 sigma (nn/init_ops.py:20-30), as AtomicNN.initialize."""
    sigma = np.sqrt(2.0 / fan_in)
    w = rng.normal(0.0, sigma, size=(fan_in, fan_out))
    bad = np.abs(w) > 2 * sigma
    while bad.any():
        w[bad] = rng.normal(0.0, sigma, size=int(bad.sum()))
        bad = np.abs(w) > 2 * sigma
    return w


class TemperatureDependentAtomicNN(AtomicNN):
    """
    Temperature-dependent atomistic network: `AtomicNN`'s constructor plus `finite_temperature`
    (a `FiniteTemperatureOptions` or its dict). Weights are
    `{element: {"H": [(W, b), ...], "U": [...], "S": [...]}}`, the last entry of each list being the
    output layer (`b` None for U's output layer without atomic static energy).
    """

    scope = "TD"

    def __init__(self, elements, descriptor, hidden_sizes=None, activation=None,
                 kernel_initializer="he_normal", minmax_scale=True, use_resnet_dt=False,
                 atomic_static_energy=None, use_atomic_static_energy=True,
                 fixed_atomic_static_energy=False, minimize_properties=("energy", "forces"),
                 export_properties=("energy", "forces"), finite_temperature=None):
        super().__init__(elements, descriptor, hidden_sizes=hidden_sizes, activation=activation,
                         kernel_initializer=kernel_initializer, minmax_scale=minmax_scale,
                         use_resnet_dt=use_resnet_dt, atomic_static_energy=atomic_static_energy,
                         use_atomic_static_energy=use_atomic_static_energy,
                         fixed_atomic_static_energy=fixed_atomic_static_energy,
                         minimize_properties=minimize_properties, export_properties=export_properties)
        if finite_temperature is None:
            finite_temperature = FiniteTemperatureOptions()
        elif isinstance(finite_temperature, dict):
            finite_temperature = FiniteTemperatureOptions(**finite_temperature)
        elif not isinstance(finite_temperature, FiniteTemperatureOptions):
            raise ValueError("finite_temperature must be FiniteTemperatureOptions or a dict")
        self._finite_temperature = finite_temperature
        self.weights: Dict[str, Dict[str, List]] = {}

    @property
    def finite_temperature_options(self) -> FiniteTemperatureOptions:
        return self._finite_temperature

    @property
    def is_finite_temperature(self) -> bool:
        return True

    @property
    def variational_energy(self):
        return "free_energy"

    def as_dict(self):
        d = super().as_dict()
        d["finite_temperature"] = self._finite_temperature.as_dict()
        return d

    def layer_sizes(self, element: str) -> Dict[str, List[int]]:
        """[in, hidden..., out] of the three nets of `element`."""
        ft = self._finite_temperature
        K = ft.layers[-1]
        hidden = list(self._hidden_sizes[element])
        return {"H": [self.ndim()] + list(ft.layers), "U": [K + 1] + hidden + [1], "S": [K + 1] + hidden + [1]}

    def initialize(self, seed=Defaults.seed, bias_scale=0.0):
        """He-normal kernels, zero biases (`bias_scale` > 0: normal biases of that scale, tests), U's
        output bias = the atomic static energy (finite_temperature.py:271-274), xlo = 1000 / xhi = 0."""
        rng = np.random.RandomState(seed)
        D = self.ndim()
        for el in self._elements:
            nets = {}
            for name, sizes in self.layer_sizes(el).items():
                layers = []
                for l in range(len(sizes) - 1):
                    w = _he_normal(rng, sizes[l], sizes[l + 1])
                    last = l == len(sizes) - 2
                    if last and name == "U":
                        b = (np.full(1, float(self._atomic_static_energy.get(el, 0.0)))
                             if self._use_atomic_static_energy else None)
                    else:
                        b = bias_scale * rng.normal(size=sizes[l + 1]) if bias_scale else np.zeros(sizes[l + 1])
                    layers.append((w, b))
                nets[name] = layers
            self.weights[el] = nets
            if self._minmax_scale:
                self.minmax[el] = (np.full(D, 1000.0), np.zeros(D))

    # -- model file ---------------------------------------------------------------------------
    def _energy_ops(self) -> dict:
        # the three energy ops of _get_energy_ops (finite_temperature.py:308-355): scopes U, S, E
        return {"energy": "Output/Energy/U/energy:0", "energy/atom": "Output/Energy/U/atomic:0",
                "eentropy": "Output/Energy/S/eentropy:0", "eentropy/atom": "Output/Energy/S/atomic:0",
                "free_energy": "Output/Energy/E/free_energy:0", "free_energy/atom": "Output/Energy/E/atomic:0"}

    def _weight_arrays(self) -> dict:
        data = {}
        for i, el in enumerate(self._elements):
            for net in NETS:
                for j, (w, b) in enumerate(self.weights[el][net]):
                    data[f"{net}::weights_{i}_{j}"] = np.asarray(w, dtype=np.float64)
                    if b is not None:
                        data[f"{net}::biases_{i}_{j}"] = np.asarray(b, dtype=np.float64)
        return data

    def set_weight_arrays(self, npz):
        """Inverse of `_weight_arrays` (json + npz model files)."""
        for i, el in enumerate(self._elements):
            nets = {}
            for net in NETS:
                layers, j = [], 0
                while f"{net}::weights_{i}_{j}" in npz:
                    w = np.array(npz[f"{net}::weights_{i}_{j}"], dtype=np.float64)
                    if w.ndim == 1:
                        w = w.reshape(-1, 1)
                    key = f"{net}::biases_{i}_{j}"
                    layers.append((w, np.array(npz[key], dtype=np.float64).ravel() if key in npz else None))
                    j += 1
                if not layers:
                    raise ValueError(f"no {net} weights for element {el}")
                nets[net] = layers
            self.weights[el] = nets

    def export_to_lammps_native(self, model_path: str, dtype=np.float64):
        """
        The reference's native `.npz` of a TD model (finite_temperature.py:390-650): `tdnp = 1`,
        `tdnp::Sommerfeld`, the descriptor keys, and per net `H::`, `S::`, `U::` `nlayers`, `actfn`,
        `layer_sizes`, `use_resnet_dt`, `apply_output_bias`, `weights_i_j`, `biases_i_j` (output
        kernels of U and S squeezed to 1-D; U's output bias only with `use_atomic_static_energy`).
        GRAP descriptors, no min-max scaling.
        """
        if getattr(self._descriptor, "name", "") != "GRAP":
            raise ValueError("The descriptor GenericRadialAtomicPotential is required")
        if self._transformer is None:
            raise ValueError("A transformer must be attached before exporting to a pb file.")
        if self._minmax_scale:
            raise ValueError("the native format has no slot for min-max scaling (atomic.py:360-478)")
        sizes = list(self._hidden_sizes[self._elements[0]])
        for el in self._elements[1:]:
            if list(self._hidden_sizes[el]) != sizes:
                raise ValueError("Layer sizes of all elements must be the same")
        ft = self._finite_temperature
        for act in (self._activation, ft.activation):
            if act.lower() not in NATIVE_ACTFN:
                raise ValueError(f"activation '{act}' has no code in the native format")
        data = self._native_descriptor_data(dtype)
        if int(data.get("use_fnn", 0)) == 0:
            data.pop("use_fnn", None)  # written by the reference's TD exporter for `nn` filters only
        data["tdnp"] = np.int32(1)
        data["tdnp::Sommerfeld"] = np.int32(ft.algo == "Sommerfeld")
        heads = {"H": (list(ft.layers), ft.activation, 1),
                 "S": (sizes + [1], self._activation, 1),
                 "U": (sizes + [1], self._activation, int(self._use_atomic_static_energy))}
        for net, (layer_sizes, act, bias_out) in heads.items():
            L = len(layer_sizes)
            data[f"{net}::nlayers"] = np.int32(L)
            data[f"{net}::actfn"] = np.int32(NATIVE_ACTFN[act.lower()])
            data[f"{net}::layer_sizes"] = np.array(layer_sizes, dtype=np.int32)
            data[f"{net}::use_resnet_dt"] = np.int32(self._use_resnet_dt)
            data[f"{net}::apply_output_bias"] = np.int32(bias_out)
            for i, el in enumerate(self._elements):
                layers = self.weights[el][net]
                for j, (w, b) in enumerate(layers):
                    last = j == L - 1
                    data[f"{net}::weights_{i}_{j}"] = (np.asarray(w, dtype=dtype).ravel() if last and net != "H"
                                                        else np.asarray(w, dtype=dtype))
                    if last and not bias_out:
                        continue
                    data[f"{net}::biases_{i}_{j}"] = (np.zeros(np.shape(w)[1], dtype=dtype) if b is None
                                                       else np.asarray(b, dtype=dtype).ravel())
        np.savez(model_path, **data)
        return model_path if str(model_path).endswith(".npz") else str(model_path) + ".npz"

    # -- C ABI --------------------------------------------------------------------------------
    def _desc_nets(self, D):
        K = self._finite_temperature.layers[-1]
        nets = []
        for net in NETS:
            for el in self._elements:
                nets.append((self.weights[el][net], D if net == "H" else K + 1, net == "H"))
        return nets

    def to_desc(self):
        desc, keep = super().to_desc()
        ft = self._finite_temperature
        desc.finite_temperature = (_lib.TA_TD_ON | (_lib.TA_TD_SOMMERFELD if ft.algo == "Sommerfeld" else 0) |
                                   (_lib.TA_ACT[ft.activation.lower()] << _lib.TA_TD_ACT_SHIFT))
        return desc, keep
