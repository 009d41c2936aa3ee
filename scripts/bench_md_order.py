#!/usr/bin/env python3
"""What the bond-orientational order parameters inside the device MD loop (`Engine.md_set_order`) add to a step, on
the workloads of scripts/bench_md_device.py under the Nose-Hoover chain thermostat:

    sf     one 4000-atom Ni frame, G2 + G4 symmetry functions
    eam    the same frame with the Ni zjw04 EAM
    eam64  64 such frames in one batch, zjw04 EAM

One process, one engine per path (each following its own trajectory), the paths alternating window by window:
`--repeats` windows of `--steps` steps each. Paths: `off` (the feature never set), and for each of two bond
cutoffs, a first-shell one (`--first-shell`, 3.0 A for Ni) and the model's cutoff, the degrees `--degrees` in
`--bins` bins with every step sampled (`s1`) and with every fourth step sampled (`s4`). Every window ends with a
device synchronise.

    python scripts/bench_md_order.py --out profiles/md_order          # .json and .md
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_md_order.py --trace eam --trace-rbond 3.0

`--trace W`: only the `s1` loop of workload W (`--trace-rbond`: its cutoff, default the model's), for a kernel
trace (run the profiler apart from the timing: its hooks cost launch latency). `--only-off`: the `off` path alone,
which also runs on a build without the feature (the per-step time of the parent commit, same machine).
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
    def __init__(self, nn, frames, v0, masses, dt, skin, kT, tau, bins=0, r_bond=None, every=1, degrees=(4, 6)):
        self.eng = Engine(nn)
        self.eng.set_skin(skin)
        self.eng.set_frames(frames)
        self.eng.md_init(masses, v0)
        self.eng.md_set_nose_hoover(kT, tau)
        if bins:
            self.eng.md_set_order(degrees, r_bond, bins, every, (degrees[-1], 0.5))
        self.dt = dt
        self.n_rebuilds = 0

    def run(self, steps):
        self.n_rebuilds += self.eng.md_run(steps, self.dt, record_every=max(steps, 1))["n_rebuilds"]
        self.eng.synchronize()


def stats(t):
    t = np.array(t)
    return dict(us=t.tolist(), median=float(np.median(t)), min=float(t.min()), max=float(t.max()))


CUTOFFS = ("shell", "cutoff")   # the first-shell cutoff, the model's cutoff


def measure(name, steps, repeats, skin, tau_steps, bins, first_shell, degrees, only_off):
    nn, frames, v0, masses, dt, T = base.setup(name, skin)
    kT, tau = md.kB * T, tau_steps * dt
    paths = {"off": DeviceLoop(nn, frames, v0, masses, dt, skin, kT, tau)}
    if not only_off:
        for cut, r_bond in zip(CUTOFFS, (first_shell, None)):
            for every in (1, 4):
                paths[f"{cut}_s{every}"] = DeviceLoop(nn, frames, v0, masses, dt, skin, kT, tau, bins, r_bond, every, degrees)
    for loop in paths.values():
        loop.run(steps)
    times = {k: [] for k in paths}
    for _ in range(repeats):
        for key, loop in paths.items():
            t0 = time.perf_counter()
            loop.run(steps)
            times[key].append((time.perf_counter() - t0) / steps * 1e6)
    row = dict(workload=name, n_frames=len(frames), n_atoms=len(masses), steps_per_window=steps, windows=repeats,
               skin=skin, temperature_K=T, dt_fs=dt / md.fs, tau_steps=tau_steps, bins=bins, degrees=list(degrees))
    for key, loop in paths.items():
        row[key] = dict(stats(times[key]), list_builds=int(loop.n_rebuilds))
    row["spread_off_us"] = row["off"]["max"] - row["off"]["min"]
    if not only_off:
        for cut in CUTOFFS:
            eng = paths[f"{cut}_s1"].eng
            out, atoms = eng.md_order(), eng.md_order_atoms()
            row[f"r_bond_{cut}"] = float(out["r_bond"][0, 0])
            row[f"bonds_per_atom_{cut}"] = float(atoms["n_bonds"].mean())
            row[f"solid_share_{cut}"] = float(md.classify_solid(atoms["n_conn"], 8).mean())
            row[f"mean_q_{cut}"] = atoms["q"].mean(axis=0).tolist()
            for every in (1, 4):
                r = row[f"{cut}_s{every}"]
                r["added_us_per_step"] = r["median"] - row["off"]["median"]
                r["added_us_per_sample"] = r["added_us_per_step"] * every
                r["share_of_step"] = r["added_us_per_step"] / row["off"]["median"]
    for loop in paths.values():
        loop.eng.close()
    return row


def write_report(prefix, rows, argv):
    with open(prefix + ".json", "w") as fp:
        json.dump(dict(script="scripts/bench_md_order.py", command="python " + " ".join(argv), rows=rows), fp, indent=1)

    def cell(d):
        return f"{d['median']:.1f} ({d['min']:.1f} .. {d['max']:.1f})"
    lines = ["# Bond-orientational order inside the device MD loop", "",
             "Written by `python " + " ".join(argv) + "`: microseconds per step, median (min .. max) over the windows, under",
             "the Nose-Hoover chain; the paths alternate window by window in one process. `s = 1`: every step sampled,",
             "`s = 4`: every fourth.", "",
             "| workload | atoms | steps x windows | degrees, bins, r_bond | feature off | s = 1 | s = 4 | added per sample, s = 1 | "
             "added per sample, s = 4 | share of the step, s = 1 | share, s = 4 | bonds per atom |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        head = (f"| {r['workload']} | {r['n_frames']} x {r['n_atoms'] // r['n_frames']} | {r['steps_per_window']} x "
                f"{r['windows']} | ")
        if "shell_s1" not in r:
            lines.append(head + f"| {cell(r['off'])} | | | | | | | |")
            continue
        for cut in CUTOFFS:
            s1, s4 = r[f"{cut}_s1"], r[f"{cut}_s4"]
            lines.append(head + f"{tuple(r['degrees'])}, {r['bins']}, {r['r_bond_' + cut]:.2f} | {cell(r['off'])} | {cell(s1)} | "
                         f"{cell(s4)} | {s1['added_us_per_sample']:+.1f} | {s4['added_us_per_sample']:+.1f} | "
                         f"{100 * s1['share_of_step']:.1f} % | {100 * s4['share_of_step']:.1f} % | "
                         f"{r['bonds_per_atom_' + cut]:.1f} |")
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
    ap.add_argument("--bins", type=int, default=200)
    ap.add_argument("--degrees", default="4,6", help="the degrees l, comma-separated; solid bonds from the last one")
    ap.add_argument("--first-shell", type=float, default=3.0, help="the first-shell bond cutoff, in A")
    ap.add_argument("--only-off", action="store_true", help="time the loop without the feature alone")
    ap.add_argument("--out", default=None, help="prefix of the .json / .md report")
    ap.add_argument("--trace", default=None, help="workload: the s = 1 loop only, for a kernel trace")
    ap.add_argument("--trace-rbond", type=float, default=None, help="bond cutoff of --trace (default: the model's)")
    args = ap.parse_args()
    degrees = tuple(int(l) for l in args.degrees.split(","))
    if args.trace:
        nn, frames, v0, masses, dt, T = base.setup(args.trace, args.skin)
        loop = DeviceLoop(nn, frames, v0, masses, dt, args.skin, md.kB * T, args.tau_steps * dt, args.bins,
                          args.trace_rbond, 1, degrees)
        loop.run(args.steps)
        print(json.dumps(dict(trace=args.trace, bins=args.bins, steps=args.steps, list_builds=loop.n_rebuilds)))
        loop.eng.close()
        return
    rows = []
    for name in args.workloads.split(","):
        rows.append(measure(name, args.steps, args.repeats, args.skin, args.tau_steps, args.bins, args.first_shell,
                            degrees, args.only_off))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        write_report(args.out, rows, ["scripts/bench_md_order.py"] + sys.argv[1:])


if __name__ == "__main__":
    main()
