#!/usr/bin/env python3
"""What the cluster analysis inside the device MD loop (`Engine.md_set_clusters`) adds to a step, on the workloads of
scripts/bench_md_device.py under the Nose-Hoover chain thermostat:

    sf     one 4000-atom Ni frame, G2 + G4 symmetry functions
    eam    the same frame with the Ni zjw04 EAM
    eam64  64 such frames in one batch, zjw04 EAM

One process, one engine per path (each following its own trajectory), the paths alternating window by window:
`--repeats` windows of `--steps` steps each, every window ending with a device synchronise. Paths:

    off        no observable set
    order_s1   `md_set_order` alone (degrees 4, 6; first-shell bonds), every step: what `solid` stands on
    solid_s1   the same with the clusters of the atoms with at least `--n-min` solid bonds, first-shell links, every step
    links_s1   the clusters of all atoms of the element (n_min 0, no order feature), first-shell links, every step
    links_s4   the same, every fourth step

The cost of a cluster sample with n_min > 0 is solid_s1 - order_s1, that of species selection links_s1 - off. The
route the feature replaces is timed on the `solid_s1` engine at the end of every window (`--host-points` of them
for a batch of many frames): `md_order_atoms()` + `md_state()` + links from a periodic k-d tree (SciPy) + the reference
union-find of tests/md_cluster_reference.py, per point; its labels are compared with the device's.

    python scripts/bench_md_cluster.py --out profiles/md_cluster          # .json and .md

    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_md_cluster.py --trace eam

`--trace W`: only the `links_s1` loop of workload W, for a kernel trace (run the profiler apart from the timing: its
hooks cost launch latency). `--only-off`: the `off` path alone, which also runs on a build without the feature (the
per-step time of the parent commit, same machine).
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
    def __init__(self, nn, frames, v0, masses, dt, skin, kT, tau, order=0, cluster=None):
        self.eng = Engine(nn)
        self.eng.set_skin(skin)
        self.eng.set_frames(frames)
        self.eng.md_init(masses, v0)
        self.eng.md_set_nose_hoover(kT, tau)
        if order:
            self.eng.md_set_order((4, 6), order, 200, 1, (6, 0.5))
        if cluster:
            self.eng.md_set_clusters(**cluster)
        self.dt = dt
        self.n_rebuilds = 0

    def run(self, steps):
        self.n_rebuilds += self.eng.md_run(steps, self.dt, record_every=max(steps, 1))["n_rebuilds"]
        self.eng.synchronize()


def stats(t):
    t = np.array(t)
    return dict(us=t.tolist(), median=float(np.median(t)), min=float(t.min()), max=float(t.max()))


def host_route(eng, frames, r_link, n_min):
    """The route the feature replaces, for the resident state: seconds, and whether its labels are the device's."""
    from scipy.spatial import cKDTree
    from tests.md_cluster_reference import components
    t0 = time.perf_counter()
    n_conn = eng.md_order_atoms()["n_conn"]
    x = eng.md_state()[0]
    label = np.full(len(x), -1, dtype=np.int64)
    a0 = 0
    for atoms in frames:
        n = len(atoms)
        box = np.diag(np.asarray(atoms.get_cell(complete=True)))   # (the workloads' cells are orthorhombic)
        wrapped = np.mod(x[a0:a0 + n], box)
        wrapped[wrapped >= box] = 0.0   # (a tiny negative coordinate wraps onto the box length itself)
        pairs = cKDTree(wrapped, boxsize=box).query_pairs(r_link, output_type="ndarray")
        lab, _ = components(n, pairs.tolist(), n_conn[a0:a0 + n] >= n_min)
        label[a0:a0 + n] = np.where(lab >= 0, lab + a0, -1)
        a0 += n
    seconds = time.perf_counter() - t0
    return seconds, bool(np.array_equal(label, eng.md_cluster_atoms()["label"]))


def measure(name, steps, repeats, skin, tau_steps, bins, series, first_shell, n_min, only_off, host_points):
    nn, frames, v0, masses, dt, T = base.setup(name, skin)
    kT, tau = md.kB * T, tau_steps * dt
    common = (nn, frames, v0, masses, dt, skin, kT, tau)
    paths = {"off": DeviceLoop(*common)}
    if not only_off:
        setting = dict(r_link=first_shell, n_bins=bins, n_series=series)
        paths["order_s1"] = DeviceLoop(*common, order=first_shell)
        paths["solid_s1"] = DeviceLoop(*common, order=first_shell, cluster=dict(setting, n_min=n_min))
        paths["links_s1"] = DeviceLoop(*common, cluster=dict(setting, n_min=0))
        paths["links_s4"] = DeviceLoop(*common, cluster=dict(setting, n_min=0, sample_every=4))
    for loop in paths.values():
        loop.run(steps)
    times = {k: [] for k in paths}
    host, host_same = [], True
    for w in range(repeats):
        for key, loop in paths.items():
            t0 = time.perf_counter()
            loop.run(steps)
            times[key].append((time.perf_counter() - t0) / steps * 1e6)
        if not only_off and (len(frames) == 1 or w < host_points):
            try:
                seconds, same = host_route(paths["solid_s1"].eng, frames, first_shell, n_min)
                host.append(seconds * 1e6)
                host_same = host_same and same
            except ImportError:   # (no SciPy: the host route is not timed)
                pass
    row = dict(workload=name, n_frames=len(frames), n_atoms=len(masses), steps_per_window=steps, windows=repeats,
               skin=skin, temperature_K=T, dt_fs=dt / md.fs, tau_steps=tau_steps, bins=bins, n_series=series,
               r_link=first_shell, n_min=n_min)
    for key, loop in paths.items():
        row[key] = dict(stats(times[key]), list_builds=int(loop.n_rebuilds))
    row["spread_off_us"] = row["off"]["max"] - row["off"]["min"]
    if not only_off:
        row["solid_added_us_per_sample"] = row["solid_s1"]["median"] - row["order_s1"]["median"]
        row["order_added_us_per_sample"] = row["order_s1"]["median"] - row["off"]["median"]
        row["links_added_us_per_sample_s1"] = row["links_s1"]["median"] - row["off"]["median"]
        row["links_added_us_per_sample_s4"] = 4.0 * (row["links_s4"]["median"] - row["off"]["median"])
        for key in ("solid_s1", "links_s1"):
            out = paths[key].eng.md_clusters()
            row[key]["last_rows"] = out["series"][-1].tolist()[:4]
            row[key]["n_samples"] = out["n_samples"]
        if host:
            row["host_route_us_per_point"] = stats(host)
            row["host_route_labels_equal_device"] = host_same
    for loop in paths.values():
        loop.eng.close()
    return row


def write_report(prefix, rows, argv):
    with open(prefix + ".json", "w") as fp:
        json.dump(dict(script="scripts/bench_md_cluster.py", command="python " + " ".join(argv), rows=rows), fp, indent=1)

    def cell(d):
        return f"{d['median']:.1f} ({d['min']:.1f} .. {d['max']:.1f})"
    lines = ["# Clusters of solid or selected atoms inside the device MD loop", "",
             "Written by `python " + " ".join(argv) + "`: microseconds per step, median (min .. max) over the windows, under",
             "the Nose-Hoover chain; the paths alternate window by window in one process. `order`: `md_set_order` alone;",
             "`solid`: with the clusters of the atoms with n_conn >= n_min on top; `links`: the clusters of all atoms",
             "(n_min 0, no order feature). First-shell links and bonds.", "",
             "| workload | atoms | steps x windows | off | order, s = 1 | solid, s = 1 | links, s = 1 | links, s = 4 | "
             "added per sample: solid - order | links, s = 1 | links, s = 4 | host route per point | newest row, solid |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        head = f"| {r['workload']} | {r['n_frames']} x {r['n_atoms'] // r['n_frames']} | {r['steps_per_window']} x {r['windows']} | "
        if "solid_s1" not in r:
            lines.append(head + f"{cell(r['off'])} | | | | | | | | | |")
            continue
        host = cell(r["host_route_us_per_point"]) if "host_route_us_per_point" in r else "not timed"
        lines.append(head + " | ".join(cell(r[k]) for k in ("off", "order_s1", "solid_s1", "links_s1", "links_s4")) +
                     f" | {r['solid_added_us_per_sample']:+.1f} | {r['links_added_us_per_sample_s1']:+.1f} | "
                     f"{r['links_added_us_per_sample_s4']:+.1f} | {host} | {r['solid_s1']['last_rows'][0]} |")
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
    ap.add_argument("--series", type=int, default=1024, help="rows of the time series kept on the device")
    ap.add_argument("--first-shell", type=float, default=3.0, help="the first-shell link and bond cutoff, in A")
    ap.add_argument("--n-min", type=int, default=8, help="solid bonds that make an atom solid")
    ap.add_argument("--host-points", type=int, default=1, help="points of the host route on a batch of many frames")
    ap.add_argument("--only-off", action="store_true", help="time the loop without the feature alone")
    ap.add_argument("--out", default=None, help="prefix of the .json / .md report")
    ap.add_argument("--trace", default=None, help="workload: the links_s1 loop only, for a kernel trace")
    args = ap.parse_args()
    if args.trace:
        nn, frames, v0, masses, dt, T = base.setup(args.trace, args.skin)
        loop = DeviceLoop(nn, frames, v0, masses, dt, args.skin, md.kB * T, args.tau_steps * dt,
                          cluster=dict(r_link=args.first_shell, n_bins=args.bins, n_series=args.series, n_min=0))
        loop.run(args.steps)
        print(json.dumps(dict(trace=args.trace, steps=args.steps, list_builds=loop.n_rebuilds,
                              newest_row=loop.eng.md_clusters()["series"][-1].tolist()[:2])))
        loop.eng.close()
        return
    rows = []
    for name in args.workloads.split(","):
        rows.append(measure(name, args.steps, args.repeats, args.skin, args.tau_steps, args.bins, args.series,
                            args.first_shell, args.n_min, args.only_off, args.host_points))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        write_report(args.out, rows, ["scripts/bench_md_cluster.py"] + sys.argv[1:])


if __name__ == "__main__":
    main()
