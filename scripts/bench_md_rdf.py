#!/usr/bin/env python3
"""What the pair distributions inside the device MD loop (`Engine.md_set_rdf`) add to a step, on the workloads
of scripts/bench_md_device.py under the Nose-Hoover chain thermostat:

    sf     one 4000-atom Ni frame, G2 + G4 symmetry functions
    eam    the same frame with the Ni zjw04 EAM
    eam64  64 such frames in one batch, zjw04 EAM

One process, one engine per path (each following its own trajectory), the paths alternating window by window:
`--repeats` windows of `--steps` steps each. Paths: `off` (the feature never set), `s1` (`--bins` bins up to the
model's cutoff, every step sampled) and `s4` (every fourth step). Every window ends with a device synchronise.
`host` is the route the feature replaces, per sample: one `md_run(4)` + `md_state()` and the brute-force NumPy
count of tests/md_rdf_reference.py. That count takes the better part of a minute per 4000-atom frame, so it is
timed on `--host-samples` samples of the FIRST frame of the batch and, the reference working frame by frame,
multiplied by the number of frames; the `md_run(4)` + `md_state()` part is timed on the whole batch.

    python scripts/bench_md_rdf.py --out profiles/md_rdf          # .json and .md
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_md_rdf.py --trace eam

`--trace W`: only the `s1` loop of workload W, for a kernel trace (run the profiler apart from the timing: its
hooks cost launch latency). `--only-off`: the `off` path alone, which also runs on a build without the feature
(the per-step time of the parent commit, same machine, for the one gated comparison).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # tests/ (the host route)
import numpy as np  # noqa: E402

import bench_md_device as base  # noqa: E402
from tensoralloy_amd import Engine, md  # noqa: E402


class DeviceLoop:
    def __init__(self, nn, frames, v0, masses, dt, skin, kT, tau, bins=0, every=1):
        self.eng = Engine(nn)
        self.eng.set_skin(skin)
        self.eng.set_frames(frames)
        self.eng.md_init(masses, v0)
        self.eng.md_set_nose_hoover(kT, tau)
        if bins:
            self.eng.md_set_rdf(bins, None, every)
        self.dt, self.bins, self.every = dt, bins, every
        self.n_rebuilds = 0

    def run(self, steps):
        self.n_rebuilds += self.eng.md_run(steps, self.dt, record_every=max(steps, 1))["n_rebuilds"]
        self.eng.synchronize()


def stats(t):
    t = np.array(t)
    return dict(us=t.tolist(), median=float(np.median(t)), min=float(t.min()), max=float(t.max()))


def host_route(nn, frames, v0, masses, dt, skin, kT, tau, bins, r_max, samples):
    """Microseconds per sample of `md_run(4)` + `md_state()` on the batch, and of the NumPy count on its first
    frame (one list entry per sample each)."""
    from tests import md_rdf_reference
    loop = DeviceLoop(nn, frames, v0, masses, dt, skin, kT, tau)
    loop.run(4)
    n0 = len(frames[0])
    els = list(nn.elements)
    species = np.array([els.index(s) for s in frames[0].get_chemical_symbols()])
    cell = np.asarray(frames[0].get_cell(complete=True))
    t_pull, t_count, pairs = [], [], 0
    for _ in range(samples):
        t0 = time.perf_counter()
        loop.run(4)
        x, _ = loop.eng.md_state()
        t1 = time.perf_counter()
        counts, _ = md_rdf_reference.pair_counts(x[None, :n0], [cell], [[True] * 3], species, [n0], len(els), bins, r_max)
        t2 = time.perf_counter()
        t_pull.append((t1 - t0) * 1e6)
        t_count.append((t2 - t1) * 1e6)
        pairs = int(counts.sum())
    loop.eng.close()
    return t_pull, t_count, pairs


def measure(name, steps, repeats, skin, tau_steps, bins, host_samples, only_off):
    nn, frames, v0, masses, dt, T = base.setup(name, skin)
    n_atoms = len(masses)
    kT, tau = md.kB * T, tau_steps * dt
    paths = {"off": DeviceLoop(nn, frames, v0, masses, dt, skin, kT, tau)}
    if not only_off:
        paths["s1"] = DeviceLoop(nn, frames, v0, masses, dt, skin, kT, tau, bins, 1)
        paths["s4"] = DeviceLoop(nn, frames, v0, masses, dt, skin, kT, tau, bins, 4)
    for loop in paths.values():
        loop.run(steps)
    times = {k: [] for k in paths}
    for _ in range(repeats):
        for key, loop in paths.items():
            t0 = time.perf_counter()
            loop.run(steps)
            times[key].append((time.perf_counter() - t0) / steps * 1e6)
    row = dict(workload=name, n_frames=len(frames), n_atoms=n_atoms, steps_per_window=steps, windows=repeats, skin=skin,
               temperature_K=T, dt_fs=dt / md.fs, tau_steps=tau_steps, bins=bins)
    for key, loop in paths.items():
        row[key] = dict(stats(times[key]), list_builds=int(loop.n_rebuilds))
    row["spread_off_us"] = row["off"]["max"] - row["off"]["min"]
    if only_off:
        for loop in paths.values():
            loop.eng.close()
        return row
    out = paths["s1"].eng.md_rdf()
    row["r_max"] = out["r_max"]
    row["n_samples_s1"] = out["n_samples"]
    row["pairs_per_sample"] = float(out["counts"].sum()) / max(out["n_samples"], 1)
    for key, every in (("s1", 1), ("s4", 4)):
        row[key]["added_us_per_step"] = row[key]["median"] - row["off"]["median"]
        row[key]["added_us_per_sample"] = row[key]["added_us_per_step"] * every
        row[key]["share_of_step"] = row[key]["added_us_per_step"] / row["off"]["median"]
    for loop in paths.values():
        loop.eng.close()
    if host_samples > 0:
        t_pull, t_count, pairs = host_route(nn, frames, v0, masses, dt, skin, kT, tau, bins, out["r_max"], host_samples)
        F = len(frames)
        per_sample = [p + F * c for p, c in zip(t_pull, t_count)]
        row["host_s4"] = dict(stats(per_sample), samples=host_samples, run_and_state=stats(t_pull),
                              numpy_count_first_frame=stats(t_count), frames_multiplied=F, pairs_first_frame=pairs)
        row["host_over_s4"] = row["host_s4"]["median"] / (4.0 * row["s4"]["median"])
    return row


def write_report(prefix, rows, argv):
    with open(prefix + ".json", "w") as fp:
        json.dump(dict(script="scripts/bench_md_rdf.py", command="python " + " ".join(argv), rows=rows), fp, indent=1)

    def cell(d):
        if len(d["us"]) == 1:   # (one sample has no spread)
            return f"{d['median']:.1f} (n = 1)"
        return f"{d['median']:.1f} ({d['min']:.1f} .. {d['max']:.1f})"
    lines = ["# Pair distributions inside the device MD loop", "",
             "Written by `python " + " ".join(argv) + "`: microseconds per step, median (min .. max) over the windows, under",
             "the Nose-Hoover chain; the paths alternate window by window in one process. `host, s = 4` is the route the",
             "feature replaces, in microseconds per sample, i.e. per four steps: `md_run(4)` + `md_state()` on the batch plus the",
             "brute-force NumPy count of tests/md_rdf_reference.py, timed on the first frame and multiplied by the frames.", "",
             "| workload | atoms | steps x windows | bins, r_max | feature off | s = 1 | s = 4 | added per sample, s = 1 | "
             "added per sample, s = 4 | share of the step, s = 1 | share, s = 4 | pairs per sample | host, s = 4, per sample | "
             "host / device, s = 4 |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        head = (f"| {r['workload']} | {r['n_frames']} x {r['n_atoms'] // r['n_frames']} | {r['steps_per_window']} x "
                f"{r['windows']} | ")
        if "s1" not in r:
            lines.append(head + f"| {cell(r['off'])} | | | | | | | | | |")
            continue
        host = f"{cell(r['host_s4'])} | {r['host_over_s4']:.0f} |" if "host_s4" in r else "| |"
        lines.append(head + f"{r['bins']}, {r['r_max']:.2f} | {cell(r['off'])} | {cell(r['s1'])} | {cell(r['s4'])} | "
                     f"{r['s1']['added_us_per_sample']:+.1f} | {r['s4']['added_us_per_sample']:+.1f} | "
                     f"{100 * r['s1']['share_of_step']:.1f} % | {100 * r['s4']['share_of_step']:.1f} % | "
                     f"{r['pairs_per_sample']:.0f} | " + host)
    lines += ["", "The host route in parts, microseconds per sample, median (min .. max):", ""]
    for r in rows:
        if "host_s4" in r:
            h = r["host_s4"]
            lines.append(f"- {r['workload']}: `md_run(4)` + `md_state()` {cell(h['run_and_state'])}; NumPy count of one frame "
                         f"{cell(h['numpy_count_first_frame'])} x {h['frames_multiplied']} frames; {h['samples']} sample(s).")
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
    ap.add_argument("--bins", type=int, default=256)
    ap.add_argument("--host-samples", type=int, default=1, help="samples of the host route (0: skip it)")
    ap.add_argument("--only-off", action="store_true", help="time the loop without the feature alone")
    ap.add_argument("--out", default=None, help="prefix of the .json / .md report")
    ap.add_argument("--trace", default=None, help="workload: the s = 1 loop only, for a kernel trace")
    args = ap.parse_args()
    if args.trace:
        nn, frames, v0, masses, dt, T = base.setup(args.trace, args.skin)
        loop = DeviceLoop(nn, frames, v0, masses, dt, args.skin, md.kB * T, args.tau_steps * dt, args.bins, 1)
        loop.run(args.steps)
        print(json.dumps(dict(trace=args.trace, bins=args.bins, steps=args.steps, list_builds=loop.n_rebuilds)))
        loop.eng.close()
        return
    rows = []
    for name in args.workloads.split(","):
        rows.append(measure(name, args.steps, args.repeats, args.skin, args.tau_steps, args.bins, args.host_samples,
                            args.only_off))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        write_report(args.out, rows, ["scripts/bench_md_rdf.py"] + sys.argv[1:])


if __name__ == "__main__":
    main()
