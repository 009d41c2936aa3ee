#!/usr/bin/env python3
"""What the heat current and pressure tensor inside the device MD loop (`Engine.md_set_flux`) add to a step, on the
workloads of scripts/bench_md_device.py under the Nose-Hoover chain thermostat:

    sf     one 4000-atom Ni frame, G2 + G4 symmetry functions
    eam    the same frame with the Ni zjw04 EAM
    eam64  64 such frames in one batch, zjw04 EAM

One process, one engine per path (each following its own trajectory), the paths alternating window by window:
`--repeats` windows of `--steps` steps each. Paths: `off` (the feature never set), `idle` (the feature on with a
sample_every no window reaches: the evaluations take the builds that leave the centre-side pair gradients, per apex
instead of triangle-once on `sf`, pair kernel and force gather on the resident list instead of the folded force kernel
on `eam`, and nothing is sampled), `e10` and `e1` (a sample every 10 steps and every step, `--lags` lags, warmed up
until the ring is full). `idle - off` is what the other build costs per step, `e1 - idle` what a sample costs.
Every window ends with a device synchronise.

    python scripts/bench_md_flux.py --out profiles/md_flux          # .json and .md
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_md_flux.py --trace eam

`--trace W`: only the `e1` loop of workload W, for a kernel trace (run the profiler apart from the timing: its hooks
cost launch latency). `--only-off`: the `off` path alone, which also runs on a build without the feature (the
per-step time of the parent commit, same machine, for the one gated comparison).
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

NEVER = 1 << 30   # a sample_every no window reaches (the entry state, step 0, is sampled once)


class DeviceLoop:
    def __init__(self, nn, frames, v0, masses, dt, skin, kT, tau, lags=0, every=1):
        self.eng = Engine(nn)
        self.eng.set_skin(skin)
        self.eng.set_frames(frames)
        self.eng.md_init(masses, v0)
        self.eng.md_set_nose_hoover(kT, tau)
        if lags:
            self.eng.md_set_flux(lags, every)
        self.dt, self.lags, self.every = dt, lags, every
        self.n_rebuilds = 0

    def run(self, steps):
        self.n_rebuilds += self.eng.md_run(steps, self.dt, record_every=max(steps, 1))["n_rebuilds"]
        self.eng.synchronize()


def stats(t):
    t = np.array(t)
    return dict(us=t.tolist(), median=float(np.median(t)), min=float(t.min()), max=float(t.max()))


PATHS = (("idle", NEVER), ("e10", 10), ("e1", 1))


def measure(name, steps, repeats, skin, tau_steps, lags, only_off):
    nn, frames, v0, masses, dt, T = base.setup(name, skin)
    n_atoms = len(masses)
    kT, tau = md.kB * T, tau_steps * dt
    paths = {"off": DeviceLoop(nn, frames, v0, masses, dt, skin, kT, tau)}
    if not only_off:
        for key, every in PATHS:
            paths[key] = DeviceLoop(nn, frames, v0, masses, dt, skin, kT, tau, lags, every)
    for loop in paths.values():   # warm-up: every shape once, and a full ring
        loop.run(max(steps, (loop.lags + 8) * (loop.every if loop.every < NEVER else 0)))
    times = {k: [] for k in paths}
    for _ in range(repeats):
        for key, loop in paths.items():
            t0 = time.perf_counter()
            loop.run(steps)
            times[key].append((time.perf_counter() - t0) / steps * 1e6)
    row = dict(workload=name, n_frames=len(frames), n_atoms=n_atoms, steps_per_window=steps, windows=repeats, skin=skin,
               temperature_K=T, dt_fs=dt / md.fs, tau_steps=tau_steps, lags=lags, n_elements=len(nn.elements))
    for key, loop in paths.items():
        row[key] = dict(stats(times[key]), list_builds=int(loop.n_rebuilds))
    row["spread_off_us"] = row["off"]["max"] - row["off"]["min"]
    if not only_off:
        out = paths["e1"].eng.md_flux()
        row["chunk"], row["blocks_per_frame"], row["n_samples_e1"] = out["chunk"], out["blocks_per_frame"], out["n_samples"]
        row["n_pairs"] = int(paths["e1"].eng.info.n_pairs)
        row["build_us_per_step"] = row["idle"]["median"] - row["off"]["median"]
        row["sample_us_e1"] = row["e1"]["median"] - row["idle"]["median"]
        row["sample_us_e10"] = 10.0 * (row["e10"]["median"] - row["idle"]["median"])
        row["added_us_per_step_e1"] = row["e1"]["median"] - row["off"]["median"]
        row["added_us_per_step_e10"] = row["e10"]["median"] - row["off"]["median"]
        c = md.heat_current_acf(out["a_heat"], out["n_samples"])
        row["jj0_mean"] = float(np.nanmean(c[..., 0]))
    for loop in paths.values():
        loop.eng.close()
    return row


def write_report(prefix, rows, argv):
    with open(prefix + ".json", "w") as fp:
        json.dump(dict(script="scripts/bench_md_flux.py", command="python " + " ".join(argv), rows=rows), fp, indent=1)

    def cell(d):
        return f"{d['median']:.1f} ({d['min']:.1f} .. {d['max']:.1f})"
    lines = ["# Heat current and pressure tensor inside the device MD loop: timing", "",
             "Written by `python " + " ".join(argv) + "`: microseconds per step, median (min .. max) over the windows, under",
             "the Nose-Hoover chain; the paths alternate window by window in one process. `idle`: the feature on, nothing",
             "sampled (the other build of the evaluation alone); `e10`, `e1`: a sample every 10 steps, every step.", "",
             "| workload | atoms | steps x windows | feature off | idle | e10 | e1 | other build, per step | a sample (e1) | "
             "a sample (e10) | added per step: e10 | e1 |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        head = (f"| {r['workload']} | {r['n_frames']} x {r['n_atoms'] // r['n_frames']} | {r['steps_per_window']} x "
                f"{r['windows']} | {cell(r['off'])} | ")
        if "e1" not in r:
            lines.append(head + "| | | | | | | |")
            continue
        lines.append(head + " | ".join(cell(r[k]) for k, _ in PATHS) + f" | {r['build_us_per_step']:+.1f} | "
                     f"{r['sample_us_e1']:+.1f} | {r['sample_us_e10']:+.1f} | {r['added_us_per_step_e10']:+.1f} | "
                     f"{r['added_us_per_step_e1']:+.1f} |")
    lines += ["", "Lags, atoms per workgroup of the pair sweep, most workgroups of a frame, pairs of the resident list:", ""]
    for r in rows:
        if "e1" in r:
            lines.append(f"- {r['workload']}: {r['lags']} lags, {r['chunk']} atoms per workgroup, {r['blocks_per_frame']} workgroups "
                         f"per frame, {r['n_pairs']} pairs, {r['n_samples_e1']} samples on the `e1` path.")
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
    ap.add_argument("--lags", type=int, default=64, help="rows of the ring")
    ap.add_argument("--only-off", action="store_true", help="time the loop without the feature alone")
    ap.add_argument("--out", default=None, help="prefix of the .json / .md report")
    ap.add_argument("--trace", default=None, help="workload: the e1 loop only, for a kernel trace")
    args = ap.parse_args()
    if args.trace:
        nn, frames, v0, masses, dt, T = base.setup(args.trace, args.skin)
        loop = DeviceLoop(nn, frames, v0, masses, dt, args.skin, md.kB * T, args.tau_steps * dt, args.lags, 1)
        loop.run(args.steps)
        print(json.dumps(dict(trace=args.trace, steps=args.steps, list_builds=loop.n_rebuilds)))
        loop.eng.close()
        return
    rows = []
    for name in args.workloads.split(","):
        rows.append(measure(name, args.steps, args.repeats, args.skin, args.tau_steps, args.lags, args.only_off))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        write_report(args.out, rows, ["scripts/bench_md_flux.py"] + sys.argv[1:])


if __name__ == "__main__":
    main()
