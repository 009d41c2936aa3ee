"""Milliseconds per `Trainer.step` of a GRAP/nn model with the filter network frozen and with it trained.

Workload: the reference's GRAP/nn defaults (moments 0..3, rcut 6.0, filter network 1 -> 32 -> 32 -> 32 -> 16
softplus with ResNet; atomic MLP [64, 64]) on 32 frames of 108-atom Ni fcc, energy + forces + stress loss,
labels from a teacher with other filters. `frozen`: `Trainer(...)` (ta_loss_gradient, the descriptor Jacobian
reused across steps); `trained`: `Trainer(..., train_filters=True)` (ta_grap_loss_gradient, the descriptors
recomputed every step). `*_gradient_ms` times the gradient call alone on the resident batch; `filter_part_ms`
= trained minus frozen gradient call: what the filter network's part adds to a step; `mlp_only_fresh_jacobian_ms`
= the MLP-only gradient when the filters change every call (pair Jacobian rebuilt each time).
Every line printed is one JSON record. Usage: python scripts/bench_grap_filter_train.py [--steps 20]
"""
import argparse
import copy
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tensoralloy_amd import Engine  # noqa: E402
from tensoralloy_amd.train import Trainer  # noqa: E402
from tests.helpers import fcc, make_grap_nn  # noqa: E402


def _sync_ms(fn, steps):
    fn()   # warm-up (buffers, Jacobian)
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=32)
    args = ap.parse_args()
    par = {"hidden_sizes": [32, 32, 32], "num_filters": 16, "activation": "softplus", "use_resnet_dt": True}
    teacher = make_grap_nn(["Ni"], 6.0, [64, 64], "nn", par, moment_tensors=[0, 1, 2, 3])
    frames = [fcc("Ni", rep=(3, 3, 3), jitter=0.05, seed=100 + k) for k in range(args.frames)]
    with Engine(teacher) as eng:
        res = eng.evaluate(frames)
    labels = ([r["energy"] for r in res], [r["forces"] for r in res], np.array([r["stress"] for r in res]))
    student = copy.deepcopy(teacher)
    student.descriptor.initialize_filters(seed=5, bias_scale=0.1)
    rec = {"workload": f"GRAP/nn Ni fcc {args.frames} x 108 atoms, rc 6.0, moments 0-3, filters 1-32-32-32-16"}
    for mode in ("frozen", "trained"):
        tr = Trainer(copy.deepcopy(student), frames, *labels, train_filters=(mode == "trained"), learning_rate=1e-3)
        rec[f"{mode}_step_ms"] = round(_sync_ms(tr.step, args.steps), 3)
        eng = tr.engine
        rng = np.random.RandomState(0)
        c = rng.normal(0, 1, len(frames))
        dR = rng.normal(0, 0.1, (sum(len(a) for a in frames), 3))
        dh = rng.normal(0, 0.01, (len(frames), 3, 3))
        grad = eng.grap_loss_gradient if mode == "trained" else eng.loss_gradient
        rec[f"{mode}_gradient_ms"] = round(_sync_ms(lambda: grad(c, dR, dh), args.steps), 3)
        if mode == "trained":
            # the MLP-only path on a Jacobian rebuilt every call, as a trained filter network would need it
            def mlp_only():
                eng.update_filter_weights(tr.theta[tr._n_weights:])
                eng.loss_gradient(c, dR, dh)
            rec["mlp_only_fresh_jacobian_ms"] = round(_sync_ms(mlp_only, max(2, args.steps // 4)), 3)
            rec["filter_part_ms"] = round(rec["trained_gradient_ms"] - rec["frozen_gradient_ms"], 3)
        tr.close()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
