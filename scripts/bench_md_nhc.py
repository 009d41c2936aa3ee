#!/usr/bin/env python3
"""Time per step of the device-resident MD loop under the Nose-Hoover chain thermostat
(`Engine.md_set_nose_hoover`) against the Berendsen NVT loop of the same build and against the host-driven
loop (`Engine.step(view=True)` + velocity Verlet in NumPy), on the workloads of scripts/bench_md_device.py:

    sf     one 4000-atom Ni frame, G2 + G4 symmetry functions
    eam    the same frame with the Ni zjw04 EAM
    eam64  64 such frames in one batch, zjw04 EAM

One process, one engine per path (each following its own trajectory), the paths alternating window by window:
`--repeats` windows of `--steps` steps each after one warm-up window per path. Every window ends with a device
synchronise. Both thermostats aim at the workload's temperature with a time constant of `--tau-steps` steps;
both integrator launches are one workgroup of 1024 threads per frame, so their difference is the chain
arithmetic of one thread (two half-updates, 2 M - 1 exp() each per loop) and what the launch waits for it.

    python scripts/bench_md_nhc.py --out profiles/md_nhc_loop          # .json and .md
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_md_nhc.py --trace eam --thermostat nhc

`--trace W`: only the device loop of workload W under `--thermostat` (nhc or berendsen), once, for a kernel
trace (run the profiler separately from the timing: its hooks cost launch latency).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import bench_md_device as base  # noqa: E402
from tensoralloy_amd import Engine, md  # noqa: E402


class DeviceLoop:
    def __init__(self, nn, frames, v0, masses, dt, skin, thermostat, kT, tau, chain, loops):
        self.eng = Engine(nn)
        self.eng.set_skin(skin)
        self.eng.set_frames(frames)
        self.eng.md_init(masses, v0)
        if thermostat == "nhc":
            self.eng.md_set_nose_hoover(kT, tau, chain=chain, loops=loops)
        else:
            self.eng.md_set_thermostat(kT, tau)
        self.dt = dt
        self.n_rebuilds = 0

    def run(self, steps):
        self.n_rebuilds += self.eng.md_run(steps, self.dt, record_every=max(steps, 1))["n_rebuilds"]
        self.eng.synchronize()

    def rebuilds(self):
        return self.n_rebuilds


def measure(name, steps, repeats, skin, tau_steps, chain, loops):
    nn, frames, v0, masses, dt, T = base.setup(name, skin)
    n_atoms = len(masses)
    kT, tau = md.kB * T, tau_steps * dt
    paths = {"nhc": DeviceLoop(nn, frames, v0, masses, dt, skin, "nhc", kT, tau, chain, loops),
             "berendsen": DeviceLoop(nn, frames, v0, masses, dt, skin, "berendsen", kT, tau, chain, loops),
             "host": base.HostLoop(nn, frames, v0, masses, dt, skin)}
    for loop in paths.values():
        loop.run(steps)
    times = {k: [] for k in paths}
    for _ in range(repeats):
        for key, loop in paths.items():
            t0 = time.perf_counter()
            loop.run(steps)
            times[key].append((time.perf_counter() - t0) / steps * 1e6)
    row = dict(workload=name, n_frames=len(frames), n_atoms=n_atoms, steps_per_window=steps, windows=repeats, skin=skin,
               temperature_K=T, dt_fs=dt / md.fs, tau_steps=tau_steps, chain=chain, loops=loops)
    for key, loop in paths.items():
        t = np.array(times[key])
        row[key] = dict(us_per_step=t.tolist(), median=float(np.median(t)), min=float(t.min()), max=float(t.max()),
                        list_builds=int(loop.rebuilds()))
        loop.eng.close()
    row["nhc_minus_berendsen_us"] = row["nhc"]["median"] - row["berendsen"]["median"]
    row["spread_us"] = max(row[k]["max"] - row[k]["min"] for k in ("nhc", "berendsen"))
    row["host_over_nhc"] = row["host"]["median"] / row["nhc"]["median"]
    return row


def write_report(prefix, rows, argv):
    with open(prefix + ".json", "w") as fp:
        json.dump(dict(script="scripts/bench_md_nhc.py", command="python " + " ".join(argv), rows=rows), fp, indent=1)
    lines = ["# Device MD loop under the Nose-Hoover chain thermostat", "",
             "Written by `python " + " ".join(argv) + "`: microseconds per step, median (min .. max) over the windows;",
             "the three paths alternate window by window in one process. `builds` = neighbour lists built during all",
             "windows of the path (warm-up included). Both device paths launch one workgroup of 1024 threads per frame.", "",
             "| workload | atoms | steps x windows | Nose-Hoover chain | builds | Berendsen | builds | host `step` + NumPy | builds | "
             "chain - Berendsen | largest spread | host / chain |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        def cell(d):
            return f"{d['median']:.1f} ({d['min']:.1f} .. {d['max']:.1f})"
        lines.append(f"| {r['workload']} | {r['n_frames']} x {r['n_atoms'] // r['n_frames']} | "
                     f"{r['steps_per_window']} x {r['windows']} | {cell(r['nhc'])} | {r['nhc']['list_builds']} | "
                     f"{cell(r['berendsen'])} | {r['berendsen']['list_builds']} | {cell(r['host'])} | "
                     f"{r['host']['list_builds']} | {r['nhc_minus_berendsen_us']:+.1f} | {r['spread_us']:.1f} | "
                     f"{r['host_over_nhc']:.2f} |")
    r0 = rows[0]
    lines += ["", f"Chain of {r0['chain']} thermostats, {r0['loops']} loop(s) per half-update, time constant "
              f"{r0['tau_steps']:g} steps, target = the workload's temperature. No threshold is set on these numbers."]
    with open(prefix + ".md", "w") as fp:
        fp.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="sf,eam,eam64")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skin", type=float, default=0.5)
    ap.add_argument("--tau-steps", type=float, default=100.0, help="time constant of both thermostats, in steps")
    ap.add_argument("--chain", type=int, default=3)
    ap.add_argument("--loops", type=int, default=1)
    ap.add_argument("--out", default=None, help="prefix of the .json / .md report")
    ap.add_argument("--trace", default=None, help="workload: one device run only, for a kernel trace")
    ap.add_argument("--thermostat", default="nhc", choices=["nhc", "berendsen"], help="with --trace")
    args = ap.parse_args()
    if args.trace:
        nn, frames, v0, masses, dt, T = base.setup(args.trace, args.skin)
        loop = DeviceLoop(nn, frames, v0, masses, dt, args.skin, args.thermostat, md.kB * T, args.tau_steps * dt,
                          args.chain, args.loops)
        loop.run(args.steps)
        print(json.dumps(dict(trace=args.trace, thermostat=args.thermostat, steps=args.steps, list_builds=loop.rebuilds())))
        loop.eng.close()
        return
    rows = []
    for name in args.workloads.split(","):
        rows.append(measure(name, args.steps, args.repeats, args.skin, args.tau_steps, args.chain, args.loops))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        write_report(args.out, rows, ["scripts/bench_md_nhc.py"] + sys.argv[1:])


if __name__ == "__main__":
    main()
