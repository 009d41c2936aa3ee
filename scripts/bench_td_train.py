"""Loss-gradient timings of a temperature-dependent model on one GPU.

One `td_loss_gradient` call with a force and stress direction (U, F and S coefficients set) on the TD
model (`TemperatureDependentAtomicNN`, default head: H layers (128, 128), U / S hidden [64, 64], ResNet
on), against one `loss_gradient` call with the same direction on the plain `AtomicNN` with the same
descriptor and hidden [64, 64], alternated in one process, on resident batches of 1 and 16 frames of
the 4000-atom Ni fcc symmetry-function frame (rc 6.5, G2 + G4). The descriptor Jacobian is built by the
warm-up calls; each timed call is host to host (direction and coefficients in, gradient out).
Every line printed is one JSON record. Usage: python scripts/bench_td_train.py [--steps 20] [--repeats 3]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tensoralloy_amd import Engine  # noqa: E402
from tensoralloy_amd.td import TemperatureDependentAtomicNN  # noqa: E402
from tests.helpers import fcc, make_nn  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 16])
    args = ap.parse_args()
    plain = make_nn(["Ni"], 6.5, True, [64, 64])
    td = TemperatureDependentAtomicNN(["Ni"], plain.descriptor, hidden_sizes=[64, 64], minmax_scale=False,
                                      use_resnet_dt=True, finite_temperature={"layers": [128, 128]})
    td.attach_transformer(plain.transformer)
    td.initialize(seed=5, bias_scale=0.1)
    rng = np.random.RandomState(0)
    for n_frames in args.frames:
        frames = []
        for k in range(n_frames):
            a = fcc("Ni", rep=(10, 10, 10), seed=100 + k)
            a.info["etemperature"] = 0.1 + 0.05 * k
            frames.append(a)
        n_atoms = sum(len(a) for a in frames)
        c = rng.normal(size=n_frames)
        dR = 1e-3 * rng.normal(size=(n_atoms, 3))
        dh = 1e-3 * rng.normal(size=(n_frames, 3, 3))
        calls = {}
        engines = []
        for name, nn in (("AtomicNN", plain), ("TemperatureDependentAtomicNN", td)):
            eng = Engine(nn, device=0)
            eng.set_frames(frames)
            eng.compute(1)
            engines.append(eng)
            if name == "AtomicNN":
                calls[name] = (lambda e=eng: e.loss_gradient(c, dR, dh))
            else:
                calls[name] = (lambda e=eng: e.td_loss_gradient(c, c, c, dR, dh))
            for _ in range(3):   # the descriptor Jacobian, buffers, first launches
                calls[name]()
        times = {name: [] for name in calls}
        for _ in range(args.repeats):
            for name, fn in calls.items():
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    fn()
                times[name].append(1e6 * (time.perf_counter() - t0) / args.steps)
        for name in calls:
            print(json.dumps({"bench": "td_train", "model": name, "frames": n_frames, "atoms": n_atoms,
                              "us_per_call": [round(t, 1) for t in times[name]],
                              "best_us": round(min(times[name]), 1)}), flush=True)
        for eng in engines:
            eng.close()
        print(json.dumps({"bench": "td_train", "frames": n_frames, "td_over_plain":
                          round(min(times["TemperatureDependentAtomicNN"]) / min(times["AtomicNN"]), 3)}),
              flush=True)


if __name__ == "__main__":
    main()
