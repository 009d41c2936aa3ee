"""eam/fs timings on one GPU (`engine.time_compute`: energy + forces + virial, warmed).

1. FS overhead: Zhou's Al-Cu eam/alloy file against the same file rewritten as eam/fs (each density
   table repeated), on one ~4000-atom Al-Cu fcc frame, rc 6.5, alternated in one process. Same
   functions and pairs: the ratio is the cost of the FS path itself.
2. Mendelev's Al-Fe eam/fs (tests/golden fixture) on an 8192-atom bcc Fe cell (16^3) with 10 % Al: atom-steps
   per second for one frame and for a 64-frame batch.
Every line printed is one JSON record. Usage: python scripts/bench_fs.py [--steps 200] [--repeats 3]
"""
import argparse
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tensoralloy_amd import Atoms, Engine, UniversalTransformer, _lib  # noqa: E402
from tensoralloy_amd.eam import EamAlloyNN, EamFsNN  # noqa: E402
from tests.fs_reference import alloy_as_fs  # noqa: E402
from tests.helpers import golden_setfl  # noqa: E402

WANT = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES | _lib.TA_WANT_VIRIAL


def lattice(basis, a, rep, symbols, seed, jitter=0.05):
    pts = np.array([basis * a + np.array([x, y, z]) * a for x in range(rep) for y in range(rep)
                    for z in range(rep)]).reshape(-1, 3)
    rng = np.random.RandomState(seed)
    pts = pts + rng.normal(0.0, jitter, pts.shape)
    syms = [symbols[0]] * len(pts)
    for k in rng.choice(len(pts), int(round(symbols[2] * len(pts))), replace=False):
        syms[k] = symbols[1]
    return Atoms(symbols=syms, positions=pts, cell=np.eye(3) * a * rep, pbc=True)


def us_per_step(eng, steps, warmup=20):
    ms, _ = eng.time_compute(WANT, warmup, steps, per_kernel=False)
    return 1e3 * ms / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    tmp = tempfile.mkdtemp()
    fcc = np.array([[0, 0, 0], [.5, .5, 0], [.5, 0, .5], [0, .5, .5]])
    bcc = np.array([[0, 0, 0], [.5, .5, .5]])

    # 1. FS overhead
    src = golden_setfl("Zhou_AlCu.alloy.eam", tmp)
    alloy = EamAlloyNN.from_setfl(src)
    fs = EamFsNN.from_setfl(alloy_as_fs(src, os.path.join(tmp, "AlCu.fs.eam")))
    frame = lattice(fcc, 4.05, 10, ("Al", "Cu", 0.3), seed=1)
    times = {"alloy": [], "fs": []}
    engines = {}
    for name, nn in (("alloy", alloy), ("fs", fs)):
        nn.attach_transformer(UniversalTransformer(["Al", "Cu"], rcut=6.5, angular=False))
        engines[name] = Engine(nn)
        engines[name].set_frames([frame])
    for _ in range(args.repeats):
        for name in ("alloy", "fs"):
            times[name].append(us_per_step(engines[name], args.steps))
    for e in engines.values():
        e.close()
    ratio = [f / a for f, a in zip(times["fs"], times["alloy"])]
    print(json.dumps({"case": "fs_overhead_zhou_alcu", "atoms": len(frame), "steps": args.steps,
                      "alloy_us": times["alloy"], "fs_us": times["fs"],
                      "ratio_median": float(np.median(ratio)), "ratio_spread": [min(ratio), max(ratio)]}))

    # 2. Mendelev Al-Fe
    nn = EamFsNN.from_setfl(golden_setfl("Mendelev_Al_Fe_thinned.fs.eam", tmp))
    nn.attach_transformer(UniversalTransformer(["Al", "Fe"], rcut=6.5, angular=False))
    for n_frames in (1, 64):
        frames = [lattice(bcc, 2.855312, 16, ("Fe", "Al", 0.1), seed=10 + k) for k in range(n_frames)]
        with Engine(nn) as eng:
            eng.set_frames(frames)
            steps = args.steps if n_frames == 1 else max(args.steps // 8, 10)
            us = [us_per_step(eng, steps) for _ in range(args.repeats)]
        atoms = sum(len(f) for f in frames)
        print(json.dumps({"case": "mendelev_alfe", "frames": n_frames, "atoms": atoms, "steps": steps, "us": us,
                          "M_atom_steps_per_s": [atoms / u for u in us]}))


if __name__ == "__main__":
    main()
