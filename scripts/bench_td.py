"""Temperature-dependent head timings on one GPU (`engine.time_compute`: energy + forces + virial,
warmed).

The TD model (`TemperatureDependentAtomicNN`, default head: H layers (128, 128), U / S hidden [64, 64],
ResNet on) against the plain `AtomicNN` with the same descriptor and hidden [64, 64], alternated in one
process, on the symmetry-function benchmark frame (4000-atom Ni fcc, rc 6.5, G2 + G4) and on a
64-frame batch of it. Per-kernel times of the head come from the `mlp` slot of `time_compute`.
Every line printed is one JSON record. Usage: python scripts/bench_td.py [--steps 200] [--repeats 3]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tensoralloy_amd import Engine, _lib  # noqa: E402
from tensoralloy_amd.td import TemperatureDependentAtomicNN  # noqa: E402
from tests.helpers import fcc, make_nn  # noqa: E402

WANT = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES | _lib.TA_WANT_VIRIAL


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    plain = make_nn(["Ni"], 6.5, True, [64, 64])
    td = TemperatureDependentAtomicNN(["Ni"], plain.descriptor, hidden_sizes=[64, 64], minmax_scale=False,
                                      use_resnet_dt=True, finite_temperature={"layers": [128, 128]})
    td.attach_transformer(plain.transformer)
    td.initialize(seed=5, bias_scale=0.1)
    for n_frames in (1, 64):
        frames = []
        for k in range(n_frames):
            a = fcc("Ni", rep=(10, 10, 10), seed=100 + k)
            a.info["etemperature"] = 0.3
            frames.append(a)
        engines = {}
        for name, nn in (("AtomicNN", plain), ("TemperatureDependentAtomicNN", td)):
            eng = Engine(nn, device=0)
            eng.set_frames(frames)
            engines[name] = eng
        times = {name: [] for name in engines}
        heads = {name: [] for name in engines}
        for _ in range(args.repeats):
            for name, eng in engines.items():
                ms, slots = eng.time_compute(WANT, 20, args.steps, per_kernel=True)
                times[name].append(1e3 * ms / args.steps)
                heads[name].append(1e3 * slots["mlp"])
        n_atoms = sum(len(a) for a in frames)
        for name in engines:
            best = min(times[name])
            print(json.dumps({"bench": "td", "model": name, "frames": n_frames, "atoms": n_atoms,
                              "us_per_step": [round(t, 2) for t in times[name]],
                              "head_kernel_us": [round(t, 2) for t in heads[name]],
                              "atom_steps_per_s": round(n_atoms / best * 1e6)}), flush=True)
        for eng in engines.values():
            eng.close()
        print(json.dumps({"bench": "td", "frames": n_frames, "td_over_plain":
                          round(min(times["TemperatureDependentAtomicNN"]) / min(times["AtomicNN"]), 3)}), flush=True)


if __name__ == "__main__":
    main()
