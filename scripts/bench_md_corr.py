#!/usr/bin/env python3
"""What sampling inside the device MD loop (`Engine.md_set_sampling`) adds to a step, on the workloads of
scripts/bench_md_device.py under the Nose-Hoover chain thermostat:

    sf     one 4000-atom Ni frame, G2 + G4 symmetry functions
    eam    the same frame with the Ni zjw04 EAM
    eam64  64 such frames in one batch, zjw04 EAM

One process, one engine per path (each following its own trajectory), the paths alternating window by window:
`--repeats` windows of `--steps` steps each. Paths: `off` (sampling never set), `s1` (`--lags` lags, every step
sampled), `s4` (every fourth step) and `host`, the route sampling replaces: one `md_run(s)` + `md_state()` per
sample and the same accumulation in NumPy over a host ring of `--lags` rows. Before the windows every sampling
path runs until its ring is full (lags x sample_every steps), so that every sample of a window correlates
against all `--lags` rows; the host path's windows are `--host-samples` samples long, its cost per sample does
not depend on how full the ring is. Every window ends with a device synchronise.

    python scripts/bench_md_corr.py --out profiles/md_sampling          # .json and .md
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_md_corr.py --trace eam

`--trace W`: only the `s1` loop of workload W, ring filled first, for a kernel trace (run the profiler apart
from the timing: its hooks cost launch latency). `--only-off`: the `off` path alone, which also runs on a build
without sampling (the per-step time of the parent commit, same machine, for the one gated comparison).
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
    def __init__(self, nn, frames, v0, masses, dt, skin, kT, tau, lags=0, every=1):
        self.eng = Engine(nn)
        self.eng.set_skin(skin)
        self.eng.set_frames(frames)
        self.eng.md_init(masses, v0)
        self.eng.md_set_nose_hoover(kT, tau)
        if lags:
            self.eng.md_set_sampling(lags, every)
        self.dt, self.lags, self.every = dt, lags, every
        self.n_rebuilds = 0

    def run(self, steps):
        self.n_rebuilds += self.eng.md_run(steps, self.dt, record_every=max(steps, 1))["n_rebuilds"]
        self.eng.synchronize()

    def fill(self):
        self.run(self.lags * self.every)


class HostCorrelator:
    """The route sampling replaces: cut the run at every sample, pull (x, v), accumulate in NumPy."""

    def __init__(self, nn, frames, v0, masses, dt, skin, kT, tau, lags, every):
        self.loop = DeviceLoop(nn, frames, v0, masses, dt, skin, kT, tau)
        self.every, self.lags = every, lags
        n = len(masses)
        self.frame = np.repeat(np.arange(len(frames)), [len(a) for a in frames])
        self.n_frames = len(frames)
        self.ring_x, self.ring_v = np.zeros((lags, n, 3)), np.zeros((lags, n, 3))
        self.acc_v, self.acc_x = np.zeros((len(frames), lags)), np.zeros((len(frames), lags))
        self.n = 0

    def sample(self):
        self.loop.run(self.every)
        x, v = self.loop.eng.md_state()
        L = self.lags
        slot = self.n % L
        self.ring_x[slot], self.ring_v[slot] = x, v
        order = (slot - np.arange(L)) % L   # row of lag k
        pv = np.einsum("lnc,nc->ln", self.ring_v[order], v)
        d = self.ring_x[order] - x
        px = np.einsum("lnc,lnc->ln", d, d)
        for f in range(self.n_frames):   # (one element: per frame only)
            sel = self.frame == f
            self.acc_v[f] += pv[:, sel].sum(axis=1)
            self.acc_x[f] += px[:, sel].sum(axis=1)
        self.n += 1


def stats(t):
    t = np.array(t)
    return dict(us=t.tolist(), median=float(np.median(t)), min=float(t.min()), max=float(t.max()))


def measure(name, steps, repeats, skin, tau_steps, lags, host_samples, only_off):
    nn, frames, v0, masses, dt, T = base.setup(name, skin)
    n_atoms = len(masses)
    kT, tau = md.kB * T, tau_steps * dt
    paths = {"off": DeviceLoop(nn, frames, v0, masses, dt, skin, kT, tau)}
    if not only_off:
        paths["s1"] = DeviceLoop(nn, frames, v0, masses, dt, skin, kT, tau, lags, 1)
        paths["s4"] = DeviceLoop(nn, frames, v0, masses, dt, skin, kT, tau, lags, 4)
    for loop in paths.values():
        loop.run(steps)
        if loop.lags:
            loop.fill()
    times = {k: [] for k in paths}
    for _ in range(repeats):
        for key, loop in paths.items():
            t0 = time.perf_counter()
            loop.run(steps)
            times[key].append((time.perf_counter() - t0) / steps * 1e6)
    row = dict(workload=name, n_frames=len(frames), n_atoms=n_atoms, steps_per_window=steps, windows=repeats, skin=skin,
               temperature_K=T, dt_fs=dt / md.fs, tau_steps=tau_steps, lags=lags)
    for key, loop in paths.items():
        row[key] = dict(stats(times[key]), list_builds=int(loop.n_rebuilds))
    row["spread_off_us"] = row["off"]["max"] - row["off"]["min"]
    if only_off:
        for loop in paths.values():
            loop.eng.close()
        return row
    row["hbm_copy_GBps"] = float(paths["off"].eng.measure_hbm_copy())
    row["ring_bytes"] = 2 * lags * n_atoms * 24
    row["bytes_per_sample"] = lags * n_atoms * 48
    for key, every in (("s1", 1), ("s4", 4)):
        row[key]["added_us_per_step"] = row[key]["median"] - row["off"]["median"]
        row[key]["added_us_per_sample"] = row[key]["added_us_per_step"] * every
        row[key]["share_of_step"] = row[key]["added_us_per_step"] / row["off"]["median"]
    for loop in paths.values():
        loop.eng.close()
    host = HostCorrelator(nn, frames, v0, masses, dt, skin, kT, tau, lags, 4)
    host.sample()
    t_host = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(host_samples):
            host.sample()
        t_host.append((time.perf_counter() - t0) / host_samples * 1e6)
    host.loop.eng.close()
    row["host_s4"] = dict(stats(t_host), samples_per_window=host_samples)   # microseconds per sample (4 steps each)
    row["host_over_s4"] = row["host_s4"]["median"] / (4.0 * row["s4"]["median"])
    return row


def write_report(prefix, rows, argv):
    with open(prefix + ".json", "w") as fp:
        json.dump(dict(script="scripts/bench_md_corr.py", command="python " + " ".join(argv), rows=rows), fp, indent=1)

    def cell(d):
        return f"{d['median']:.1f} ({d['min']:.1f} .. {d['max']:.1f})"
    lines = ["# Sampling inside the device MD loop", "",
             "Written by `python " + " ".join(argv) + "`: microseconds per step, median (min .. max) over the windows, under",
             "the Nose-Hoover chain; the paths alternate window by window in one process, every sampling path with its",
             f"ring of {rows[0]['lags']} rows already full. `host, s = 4` is the route sampling replaces (`md_run(4)` + `md_state()` + the",
             "accumulation in NumPy), in microseconds per sample, i.e. per four steps.", "",
             "| workload | atoms | steps x windows | sampling off | s = 1 | s = 4 | added per sample, s = 1 | added per sample, s = 4 | "
             "share of the step, s = 1 | share, s = 4 | ring | host, s = 4, per sample | host / device, s = 4 |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        if "s1" not in r:
            lines.append(f"| {r['workload']} | {r['n_frames']} x {r['n_atoms'] // r['n_frames']} | {r['steps_per_window']} x "
                         f"{r['windows']} | {cell(r['off'])} | | | | | | | | | |")
            continue
        lines.append(f"| {r['workload']} | {r['n_frames']} x {r['n_atoms'] // r['n_frames']} | {r['steps_per_window']} x "
                     f"{r['windows']} | {cell(r['off'])} | {cell(r['s1'])} | {cell(r['s4'])} | "
                     f"{r['s1']['added_us_per_sample']:+.1f} | {r['s4']['added_us_per_sample']:+.1f} | "
                     f"{100 * r['s1']['share_of_step']:.1f} % | {100 * r['s4']['share_of_step']:.1f} % | "
                     f"{r['ring_bytes'] / 1e6:.0f} MB | {cell(r['host_s4'])} | {r['host_over_s4']:.1f} |")
    lines += ["", "Bytes the correlation launch reads per sample with the ring full (lags x atoms x 48) and the copy rate "
              "`ta_measure_hbm_copy` gave in the same process:", ""]
    for r in rows:
        if "s1" in r:
            lines.append(f"- {r['workload']}: {r['bytes_per_sample'] / 1e6:.1f} MB per sample; device-to-device copy "
                         f"{r['hbm_copy_GBps']:.0f} GB/s (read + written).")
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
    ap.add_argument("--lags", type=int, default=256)
    ap.add_argument("--host-samples", type=int, default=3, help="samples per window of the host route")
    ap.add_argument("--only-off", action="store_true", help="time the loop without sampling alone")
    ap.add_argument("--out", default=None, help="prefix of the .json / .md report")
    ap.add_argument("--trace", default=None, help="workload: the s = 1 loop only, for a kernel trace")
    args = ap.parse_args()
    if args.trace:
        nn, frames, v0, masses, dt, T = base.setup(args.trace, args.skin)
        loop = DeviceLoop(nn, frames, v0, masses, dt, args.skin, md.kB * T, args.tau_steps * dt, args.lags, 1)
        loop.fill()
        loop.run(args.steps)
        print(json.dumps(dict(trace=args.trace, lags=args.lags, steps=args.steps, list_builds=loop.n_rebuilds)))
        loop.eng.close()
        return
    rows = []
    for name in args.workloads.split(","):
        rows.append(measure(name, args.steps, args.repeats, args.skin, args.tau_steps, args.lags, args.host_samples,
                            args.only_off))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        write_report(args.out, rows, ["scripts/bench_md_corr.py"] + sys.argv[1:])


if __name__ == "__main__":
    main()
