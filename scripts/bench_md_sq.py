#!/usr/bin/env python3
"""What the structure factors inside the device MD loop (`Engine.md_set_sq`) add to a step, on the workloads of
scripts/bench_md_device.py under the Nose-Hoover chain thermostat:

    sf     one 4000-atom Ni frame, G2 + G4 symmetry functions
    eam    the same frame with the Ni zjw04 EAM
    eam64  64 such frames in one batch, zjw04 EAM

One process, one engine per path (each following its own trajectory), the paths alternating window by window:
`--repeats` windows of `--steps` steps each, every step sampled. Paths: `off` (the feature never set), `L1` and
`L1c` (the static structure factor: one lag, without and with currents), `L256` and `L256c` (`--lags` lags,
without and with currents; warmed up until the ring is full, so that every sample correlates with all the lags).
The wave vectors are all of `md.q_points` up to the |q| that gives about `--n-q` of them for the frame's cell.
Every window ends with a device synchronise.

    python scripts/bench_md_sq.py --out profiles/md_sq          # .json and .md
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_md_sq.py --trace eam

`--trace W`: only the `L256c` loop of workload W, for a kernel trace (run the profiler apart from the timing: its
hooks cost launch latency). `--only-off`: the `off` path alone, which also runs on a build without the feature
(the per-step time of the parent commit, same machine, for the one gated comparison).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import bench_md_device as base  # noqa: E402
from tensoralloy_amd import Engine, md  # noqa: E402


class DeviceLoop:
    def __init__(self, nn, frames, v0, masses, dt, skin, kT, tau, miller=None, lags=1, currents=False):
        self.eng = Engine(nn)
        self.eng.set_skin(skin)
        self.eng.set_frames(frames)
        self.eng.md_init(masses, v0)
        self.eng.md_set_nose_hoover(kT, tau)
        if miller is not None:
            self.eng.md_set_sq(miller, lags, 1, currents)
        self.dt, self.lags = dt, lags
        self.n_rebuilds = 0

    def run(self, steps):
        self.n_rebuilds += self.eng.md_run(steps, self.dt, record_every=max(steps, 1))["n_rebuilds"]
        self.eng.synchronize()


def stats(t):
    t = np.array(t)
    return dict(us=t.tolist(), median=float(np.median(t)), min=float(t.min()), max=float(t.max()))


def wave_vectors(cell, n_q):
    """All triples of `md.q_points` up to the |q| that gives about n_q of them: (miller, q_max). The count below a
    |q| is V q^3 / (12 pi^2) for one of each +-n pair; the shell that crosses n_q is taken whole."""
    q_max = (12.0 * np.pi ** 2 * n_q / abs(np.linalg.det(cell))) ** (1.0 / 3.0)
    miller = md.q_points(cell, q_max)
    return miller, float(q_max)


PATHS = (("L1", 1, False), ("L1c", 1, True), ("L256", None, False), ("L256c", None, True))


def measure(name, steps, repeats, skin, tau_steps, n_q, lags, only_off):
    nn, frames, v0, masses, dt, T = base.setup(name, skin)
    n_atoms = len(masses)
    kT, tau = md.kB * T, tau_steps * dt
    paths = {"off": DeviceLoop(nn, frames, v0, masses, dt, skin, kT, tau)}
    miller, q_max = np.zeros((0, 3), dtype=np.int32), 0.0
    if not only_off:
        miller, q_max = wave_vectors(np.asarray(frames[0].get_cell(complete=True)), n_q)
        for key, L, cur in PATHS:
            paths[key] = DeviceLoop(nn, frames, v0, masses, dt, skin, kT, tau, miller, L or lags, cur)
    for loop in paths.values():   # warm-up: every shape once, and a full ring
        loop.run(max(steps, loop.lags + 8))
    times = {k: [] for k in paths}
    for _ in range(repeats):
        for key, loop in paths.items():
            t0 = time.perf_counter()
            loop.run(steps)
            times[key].append((time.perf_counter() - t0) / steps * 1e6)
    row = dict(workload=name, n_frames=len(frames), n_atoms=n_atoms, steps_per_window=steps, windows=repeats, skin=skin,
               temperature_K=T, dt_fs=dt / md.fs, tau_steps=tau_steps, n_q=int(len(miller)), q_max=q_max, lags=lags,
               n_elements=len(nn.elements))
    for key, loop in paths.items():
        row[key] = dict(stats(times[key]), list_builds=int(loop.n_rebuilds))
    row["spread_off_us"] = row["off"]["max"] - row["off"]["min"]
    if not only_off:
        out = paths["L256c"].eng.md_sq()
        row["chunk"], row["n_samples_L256c"] = out["chunk"], out["n_samples"]
        s_ab, s = md.structure_factor(out["a_rho"], out["n_samples"], out["n_by_element"])
        row["s_max"], row["s_median"] = float(np.nanmax(s)), float(np.nanmedian(s))
        for key, _, _ in PATHS:
            row[key]["added_us_per_sample"] = row[key]["median"] - row["off"]["median"]
            row[key]["share_of_step"] = row[key]["added_us_per_sample"] / row["off"]["median"]
            row[key]["ns_per_atom_q"] = 1e3 * row[key]["added_us_per_sample"] / (n_atoms * len(miller))
    for loop in paths.values():
        loop.eng.close()
    return row


def write_report(prefix, rows, argv):
    with open(prefix + ".json", "w") as fp:
        json.dump(dict(script="scripts/bench_md_sq.py", command="python " + " ".join(argv), rows=rows), fp, indent=1)

    def cell(d):
        return f"{d['median']:.1f} ({d['min']:.1f} .. {d['max']:.1f})"
    lines = ["# Structure factors inside the device MD loop", "",
             "Written by `python " + " ".join(argv) + "`: microseconds per step, median (min .. max) over the windows, under",
             "the Nose-Hoover chain; the paths alternate window by window in one process and sample every step, so what a",
             "path adds to a step is what a sample costs. `L1`: one lag (the static structure factor), `L256`: a full ring",
             "of that many lags; `c`: with currents. ns per (atom, q) is the added time over atoms x wave vectors.", "",
             "| workload | atoms | steps x windows | Q, q_max | feature off | L1 | L1c | L256 | L256c | added per sample: L1 | L1c | "
             "L256 | L256c | ns per (atom, q): L1 | L1c |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        head = (f"| {r['workload']} | {r['n_frames']} x {r['n_atoms'] // r['n_frames']} | {r['steps_per_window']} x "
                f"{r['windows']} | {r['n_q']}, {r['q_max']:.3f} | {cell(r['off'])} | ")
        if "L1" not in r:
            lines.append(head + "| | | | | | | | | |")
            continue
        lines.append(head + " | ".join(cell(r[k]) for k, _, _ in PATHS) + " | " +
                     " | ".join(f"{r[k]['added_us_per_sample']:+.1f}" for k, _, _ in PATHS) + " | " +
                     f"{r['L1']['ns_per_atom_q']:.4f} | {r['L1c']['ns_per_atom_q']:.4f} |")
    lines += ["", "Lags of the `L256` paths, atoms per workgroup of the amplitude launch, and S(q) of the `L256c` path "
              "(largest and median over the wave vectors, first frame included):", ""]
    for r in rows:
        if "L1" in r:
            lines.append(f"- {r['workload']}: {r['lags']} lags, {r['chunk']} atoms per workgroup, {r['n_samples_L256c']} samples, "
                         f"S max {r['s_max']:.2f}, median {r['s_median']:.3f}.")
    lines += ["", "No threshold is set on these numbers."]
    with open(prefix + ".md", "w") as fp:
        fp.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="sf,eam,eam64")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skin", type=float, default=0.5)
    ap.add_argument("--tau-steps", type=float, default=100.0, help="time constant of the thermostat, in steps")
    ap.add_argument("--n-q", type=int, default=1000, help="about this many wave vectors")
    ap.add_argument("--lags", type=int, default=256, help="lags of the L256 paths")
    ap.add_argument("--only-off", action="store_true", help="time the loop without the feature alone")
    ap.add_argument("--out", default=None, help="prefix of the .json / .md report")
    ap.add_argument("--trace", default=None, help="workload: the L256c loop only, for a kernel trace")
    args = ap.parse_args()
    if args.trace:
        nn, frames, v0, masses, dt, T = base.setup(args.trace, args.skin)
        miller, _ = wave_vectors(np.asarray(frames[0].get_cell(complete=True)), args.n_q)
        loop = DeviceLoop(nn, frames, v0, masses, dt, args.skin, md.kB * T, args.tau_steps * dt, miller, args.lags, True)
        loop.run(args.steps)
        print(json.dumps(dict(trace=args.trace, n_q=int(len(miller)), steps=args.steps, list_builds=loop.n_rebuilds)))
        loop.eng.close()
        return
    rows = []
    for name in args.workloads.split(","):
        rows.append(measure(name, args.steps, args.repeats, args.skin, args.tau_steps, args.n_q, args.lags, args.only_off))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        write_report(args.out, rows, ["scripts/bench_md_sq.py"] + sys.argv[1:])


if __name__ == "__main__":
    main()
