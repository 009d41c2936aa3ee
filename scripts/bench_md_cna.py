#!/usr/bin/env python3
"""What the common neighbour analysis inside the device MD loop (`Engine.md_set_cna`) adds to a step, on the workloads
of scripts/bench_md_device.py under the Nose-Hoover chain thermostat:

    sf     one 4000-atom Ni frame, G2 + G4 symmetry functions
    eam    the same frame with the Ni zjw04 EAM
    eam64  64 such frames in one batch, zjw04 EAM

One process, one engine per path (each following its own trajectory), the paths alternating window by window:
`--repeats` windows of `--steps` steps each, every window ending with a device synchronise. Paths:

    off          no observable set
    adf_s1       `md_set_adf` with first-shell bonds, every step: a sweep of the list that only bins
    order_s1     `md_set_order` (degrees 4, 6; first-shell bonds), every step
    adaptive_s1  the adaptive analysis at the model's reach (6.5 A), every step
    adaptive_s4  the same, every fourth step
    fixed_s1     the fixed-cutoff analysis at the first-shell cutoff, every step
    fixed_s4     the same, every fourth step

The cost of a sample is the path's time less that of `off` (times four for the paths of every fourth step). The route
the feature replaces is timed on the `adaptive_s1` engine at the end of every window of a one-frame workload:
`md_run(4)` + `md_state()` + the 14 nearest neighbours from a periodic k-d tree (SciPy) + the signatures in NumPy, all
atoms at once; its types are compared with the device's for the same state.

    python scripts/bench_md_cna.py --out profiles/md_cna          # .json and .md

    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_md_cna.py --trace eam

`--trace W`: only the `adaptive_s1` loop of workload W, for a kernel trace (run the profiler apart from the timing: its
hooks cost launch latency). `--only-off`: the `off` path alone, which also runs on a build without the feature (the
per-step time of the parent commit, same machine).
"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import bench_md_device as base  # noqa: E402
from tensoralloy_amd import Engine, md  # noqa: E402

SCALE = (1.0 + math.sqrt(2.0)) / 2.0


class DeviceLoop:
    def __init__(self, nn, frames, v0, masses, dt, skin, kT, tau, adf=0, order=0, cna=None):
        self.eng = Engine(nn)
        self.eng.set_skin(skin)
        self.eng.set_frames(frames)
        self.eng.md_init(masses, v0)
        self.eng.md_set_nose_hoover(kT, tau)
        if adf:
            self.eng.md_set_adf(180, adf, 1)
        if order:
            self.eng.md_set_order((4, 6), order, 200, 1, (6, 0.5))
        if cna:
            self.eng.md_set_cna(**cna)
        self.dt = dt
        self.n_rebuilds = 0

    def run(self, steps):
        self.n_rebuilds += self.eng.md_run(steps, self.dt, record_every=max(steps, 1))["n_rebuilds"]
        self.eng.synchronize()


def stats(t):
    t = np.array(t)
    return dict(us=t.tolist(), median=float(np.median(t)), min=float(t.min()), max=float(t.max()))


def signature_counts(d, rc):
    """For the neighbour vectors d [N, n, 3] of N atoms under the bond cutoffs rc [N]: how many of every atom's n
    neighbours have the signatures (4,2,1), (4,2,2), (5,5,5), (6,6,6), (4,4,4), [N, 5]. All atoms at once."""
    n = d.shape[1]
    sep2 = ((d[:, :, None, :] - d[:, None, :, :]) ** 2).sum(axis=-1)
    adj = (sep2 < (rc * rc)[:, None, None]) & ~np.eye(n, dtype=bool)[None]
    # bonds among the common neighbours of the centre and neighbour j: B[N, j, a, b]
    bonds = adj[:, None, :, :] & adj[:, :, :, None] & adj[:, :, None, :]
    n_cn, n_b = adj.sum(axis=2), bonds.sum(axis=(2, 3)) // 2
    # the sets of nodes joined by bonds (closure by squaring: paths of 1, 2, 4, 8, 16 bonds), the bonds inside each
    reach = (bonds | np.eye(n, dtype=bool)[None, None]).astype(np.float32)
    for _ in range(4):
        reach = (reach @ reach > 0.0).astype(np.float32)
    inside = np.einsum("njab,njbc,njac->nja", reach, bonds.astype(np.float32), reach) / 2.0
    l_cb = np.rint(inside.max(axis=2)).astype(np.int64)
    code = n_cn * 10000 + n_b * 100 + l_cb
    return np.stack([(code == c).sum(axis=1) for c in (40201, 40202, 50505, 60606, 40404)], axis=1)


def host_route(eng, frames, dt, r_max):
    """The route the feature replaces, one point: seconds, and whether its types are the device's (both look at the
    state behind the four steps)."""
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    eng.md_run(4, dt, record_every=4)
    x = eng.md_state()[0]
    kind = np.zeros(len(x), dtype=np.int32)
    a0 = 0
    for atoms in frames:
        n = len(atoms)
        box = np.diag(np.asarray(atoms.get_cell(complete=True)))   # (the workloads' cells are orthorhombic)
        wrapped = np.mod(x[a0:a0 + n], box)
        wrapped[wrapped >= box] = 0.0   # (a tiny negative coordinate wraps onto the box length itself)
        dist, idx = cKDTree(wrapped, boxsize=box).query(wrapped, k=15, distance_upper_bound=r_max)
        dist, idx = dist[:, 1:], idx[:, 1:]   # (the atom itself comes first)
        have = np.isfinite(dist).sum(axis=1)
        d = wrapped[np.minimum(idx, n - 1)] - wrapped[:, None, :]
        d -= box * np.rint(d / box)
        out = np.zeros(n, dtype=np.int32)
        first = np.nonzero(have >= 12)[0]
        c = signature_counts(d[first, :12], SCALE * dist[first, :12].mean(axis=1))
        out[first] = np.where(c[:, 0] == 12, 1, np.where((c[:, 0] == 6) & (c[:, 1] == 6), 2, np.where(c[:, 2] == 12, 4, 0)))
        second = np.nonzero((have >= 14) & (out == 0))[0]
        if len(second):
            rc = SCALE * (2.0 / math.sqrt(3.0) * dist[second, :8].sum(axis=1) + dist[second, 8:14].sum(axis=1)) / 14.0
            c = signature_counts(d[second, :14], rc)
            out[second] = np.where((c[:, 3] == 8) & (c[:, 4] == 6), 3, 0)
        kind[a0:a0 + n] = out
        a0 += n
    seconds = time.perf_counter() - t0
    return seconds, bool(np.array_equal(kind, eng.md_cna_atoms()["structure"]))


def measure(name, steps, repeats, skin, tau_steps, series, first_shell, only_off, trace=False):
    nn, frames, v0, masses, dt, T = base.setup(name, skin)
    kT, tau = md.kB * T, tau_steps * dt
    common = (nn, frames, v0, masses, dt, skin, kT, tau)
    if trace:
        loop = DeviceLoop(*common, cna=dict(mode="adaptive", n_series=series))
        loop.run(steps)
        print(json.dumps(dict(trace=name, steps=steps, list_builds=loop.n_rebuilds,
                              newest_row=loop.eng.md_cna()["series"][-1].tolist()[:2])))
        loop.eng.close()
        return None
    paths = {"off": DeviceLoop(*common)}
    if not only_off:
        paths["adf_s1"] = DeviceLoop(*common, adf=first_shell)
        paths["order_s1"] = DeviceLoop(*common, order=first_shell)
        paths["adaptive_s1"] = DeviceLoop(*common, cna=dict(mode="adaptive", n_series=series))
        paths["adaptive_s4"] = DeviceLoop(*common, cna=dict(mode="adaptive", n_series=series, sample_every=4))
        paths["fixed_s1"] = DeviceLoop(*common, cna=dict(mode="fixed", r_cut=first_shell, n_series=series))
        paths["fixed_s4"] = DeviceLoop(*common, cna=dict(mode="fixed", r_cut=first_shell, n_series=series, sample_every=4))
    for loop in paths.values():
        loop.run(steps)
    times = {k: [] for k in paths}
    host, host_same = [], True
    for _ in range(repeats):
        for key, loop in paths.items():
            t0 = time.perf_counter()
            loop.run(steps)
            times[key].append((time.perf_counter() - t0) / steps * 1e6)
        if not only_off and len(frames) == 1:
            try:
                seconds, same = host_route(paths["adaptive_s1"].eng, frames, dt, float(paths["adaptive_s1"].eng._md_cutoff))
                host.append(seconds * 1e6)
                host_same = host_same and same
            except ImportError:   # (no SciPy: the host route is not timed)
                pass
    row = dict(workload=name, n_frames=len(frames), n_atoms=len(masses), steps_per_window=steps, windows=repeats,
               skin=skin, temperature_K=T, dt_fs=dt / md.fs, tau_steps=tau_steps, n_series=series, r_cut=first_shell)
    for key, loop in paths.items():
        row[key] = dict(stats(times[key]), list_builds=int(loop.n_rebuilds))
    row["spread_off_us"] = row["off"]["max"] - row["off"]["min"]
    if not only_off:
        off = row["off"]["median"]
        row["r_max"] = float(paths["adaptive_s1"].eng._md_cutoff)
        for key in ("adf_s1", "order_s1", "adaptive_s1", "fixed_s1"):
            row[key.replace("_s1", "") + "_added_us_per_sample_s1"] = row[key]["median"] - off
        for key in ("adaptive_s4", "fixed_s4"):
            row[key.replace("_s4", "") + "_added_us_per_sample_s4"] = 4.0 * (row[key]["median"] - off)
        for key in ("adaptive_s1", "fixed_s1"):
            out = paths[key].eng.md_cna()
            row[key]["newest_row"] = out["series"][-1].tolist()[:2]
            row[key]["n_samples"] = out["n_samples"]
        if host:
            row["host_route_us_per_point"] = stats(host)
            row["host_route_types_equal_device"] = host_same
    for loop in paths.values():
        loop.eng.close()
    return row


def write_report(prefix, rows, argv):
    with open(prefix + ".json", "w") as fp:
        json.dump(dict(script="scripts/bench_md_cna.py", command="python " + " ".join(argv), rows=rows), fp, indent=1)

    def cell(d):
        return f"{d['median']:.1f} ({d['min']:.1f} .. {d['max']:.1f})"
    keys = ("off", "adf_s1", "order_s1", "adaptive_s1", "adaptive_s4", "fixed_s1", "fixed_s4")
    lines = ["# Common neighbour analysis inside the device MD loop", "",
             "Written by `python " + " ".join(argv) + "`: microseconds per step, median (min .. max) over the windows, under",
             "the Nose-Hoover chain; the paths alternate window by window in one process. `adf`: `md_set_adf` with first-shell",
             "bonds; `order`: `md_set_order` at degrees (4, 6), first-shell bonds; `adaptive`: `md_set_cna` at the model's reach;",
             "`fixed`: `md_set_cna` at the first-shell cutoff.", "",
             "| workload | atoms | steps x windows | " + " | ".join(k.replace("_s", ", s = ") for k in keys) +
             " | added per sample: adf | order | adaptive, s = 1 | adaptive, s = 4 | fixed, s = 1 | fixed, s = 4 | "
             "host route per point | newest row, adaptive |",
             "|" + "---|" * (3 + len(keys) + 8)]
    for r in rows:
        head = f"| {r['workload']} | {r['n_frames']} x {r['n_atoms'] // r['n_frames']} | {r['steps_per_window']} x {r['windows']} | "
        if "adaptive_s1" not in r:
            lines.append(head + f"{cell(r['off'])} |" + " |" * (len(keys) - 1 + 8))
            continue
        host = cell(r["host_route_us_per_point"]) if "host_route_us_per_point" in r else "not timed"
        added = [r["adf_added_us_per_sample_s1"], r["order_added_us_per_sample_s1"], r["adaptive_added_us_per_sample_s1"],
                 r["adaptive_added_us_per_sample_s4"], r["fixed_added_us_per_sample_s1"], r["fixed_added_us_per_sample_s4"]]
        lines.append(head + " | ".join(cell(r[k]) for k in keys) + " | " + " | ".join(f"{a:+.1f}" for a in added) +
                     f" | {host} | {r['adaptive_s1']['newest_row'][0]} |")
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
    ap.add_argument("--series", type=int, default=1024, help="rows of the time series kept on the device")
    ap.add_argument("--first-shell", type=float, default=3.0, help="the first-shell cutoff of the fixed mode, in A")
    ap.add_argument("--only-off", action="store_true", help="time the loop without the feature alone")
    ap.add_argument("--out", default=None, help="prefix of the .json / .md report")
    ap.add_argument("--trace", default=None, help="workload: the adaptive_s1 loop only, for a kernel trace")
    args = ap.parse_args()
    if args.trace:
        measure(args.trace, args.steps, 0, args.skin, args.tau_steps, args.series, args.first_shell, False, trace=True)
        return
    rows = []
    for name in args.workloads.split(","):
        rows.append(measure(name, args.steps, args.repeats, args.skin, args.tau_steps, args.series, args.first_shell,
                            args.only_off))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        write_report(args.out, rows, ["scripts/bench_md_cna.py"] + sys.argv[1:])


if __name__ == "__main__":
    main()
