#!/usr/bin/env python3
"""Time per step of the device-resident MD loop under the Martyna-Tobias-Klein barostat (`Engine.md_set_mtk`),
isotropic and per axis, against the Berendsen-NPT + chain loop and the plain chain loop of the same build, on the
workloads of scripts/bench_md_device.py:

    sf     one 4000-atom Ni frame, G2 + G4 symmetry functions
    eam    the same frame with the Ni zjw04 EAM
    eam64  64 such frames in one batch, zjw04 EAM

One process, one engine per path (each following its own trajectory), the paths alternating window by window:
`--repeats` windows of `--steps` steps each after one warm-up window per path. Every window ends with a device
synchronise. All paths run the Nose-Hoover chain at the workload's temperature (`--tau-steps`) and launch one
workgroup of 1024 threads per frame; the barostats aim at P0 = 0 with a time constant of `--pdamp-steps` steps
(Berendsen: `--taup-steps`, beta = 0.9 A^3 / eV). The symmetry-function model has random weights, a pressure of its
own of the order of -1 eV / A^3 and the wrong sign of stiffness (scripts/bench_md_npt.py): its target is the pressure
of its initial state, its pdamp 100 times longer (in steps: its step is 0.005 fs) and its beta 1000 times smaller,
which keeps the cell from running away inside the windows. The work per step does not depend on the size of the
strain while the list holds.

    python scripts/bench_md_mtk.py --out profiles/md_mtk_loop                       # .json and .md
    python scripts/bench_md_mtk.py --paths chain,npt_chain --out parent_md_mtk     # in a checkout of another commit
    python scripts/bench_md_mtk.py --other parent_md_mtk.json --out profiles/md_mtk_loop

`--paths` restricts the paths (a commit without this barostat runs `chain,npt_chain`); `--other FILE.json` puts the
rows of such a run beside this build's in the report, to show what the untouched paths cost before.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import bench_md_device as base  # noqa: E402
from tensoralloy_amd import Engine, _lib, md  # noqa: E402

WANT = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES | _lib.TA_WANT_VIRIAL
BETA = 0.9   # A^3 / eV
PATHS = ("mtk_iso", "mtk_axis", "npt_chain", "chain")
TITLES = {"mtk_iso": "MTK, isotropic", "mtk_axis": "MTK, per axis", "npt_chain": "Berendsen-NPT + chain", "chain": "chain"}


class DeviceLoop:
    def __init__(self, path, nn, frames, v0, masses, dt, skin, kT, tau, p0, pdamp, taup, beta):
        self.eng = Engine(nn)
        self.eng.set_skin(skin)
        self.eng.set_frames(frames)
        self.eng.md_init(masses, v0)
        self.eng.md_set_nose_hoover(kT, tau)
        if path == "mtk_iso":
            self.eng.md_set_mtk(p0, pdamp)
        elif path == "mtk_axis":
            self.eng.md_set_mtk(p0, pdamp, mask=(1, 1, 1))
        elif path == "npt_chain":
            self.eng.md_set_barostat(p0, taup, beta)
        self.dt = dt
        self.n_rebuilds = 0

    def run(self, steps):
        self.n_rebuilds += self.eng.md_run(steps, self.dt, record_every=max(steps, 1))["n_rebuilds"]
        self.eng.synchronize()


def initial_pressure(nn, frames, v0, masses, skin):
    """The mean over frames and axes of (sum m v_c^2 - W_cc) / V of the state at entry."""
    with Engine(nn) as eng:
        eng.set_skin(skin)
        eng.set_frames(frames)
        x = np.ascontiguousarray(np.concatenate([a.positions for a in frames]))
        W = np.diagonal(eng.step(x, WANT)["virial"], axis1=1, axis2=2).copy()   # (the results live in the engine)
    F, n = len(frames), len(frames[0])
    S = (masses.reshape(F, n, 1) * v0.reshape(F, n, 3) ** 2).sum(axis=1)
    V = np.abs(np.linalg.det([np.asarray(a.get_cell(complete=True)) for a in frames]))
    return float(((S - W) / V[:, None]).mean())


def measure(name, paths, steps, repeats, skin, tau_steps, pdamp_steps, taup_steps):
    nn, frames, v0, masses, dt, T = base.setup(name, skin)
    kT, sf = md.kB * T, name == "sf"
    p0 = initial_pressure(nn, frames, v0, masses, skin) if sf else 0.0
    pdamp, beta = (100.0 if sf else 1.0) * pdamp_steps * dt, (1e-3 if sf else 1.0) * BETA
    loops = {p: DeviceLoop(p, nn, frames, v0, masses, dt, skin, kT, tau_steps * dt, p0, pdamp, taup_steps * dt, beta)
             for p in paths}
    for loop in loops.values():
        loop.run(steps)
    times = {k: [] for k in loops}
    for _ in range(repeats):
        for key, loop in loops.items():
            t0 = time.perf_counter()
            loop.run(steps)
            times[key].append((time.perf_counter() - t0) / steps * 1e6)
    row = dict(workload=name, n_frames=len(frames), n_atoms=len(masses), steps_per_window=steps, windows=repeats, skin=skin,
               temperature_K=T, dt_fs=dt / md.fs, tau_steps=tau_steps, pdamp_steps=pdamp / dt, taup_steps=taup_steps,
               target_pressure_eV_A3=p0, compressibility_A3_eV=beta)
    for key, loop in loops.items():
        t = np.array(times[key])
        V = np.abs(np.linalg.det(loop.eng.md_cells()))
        V0 = np.abs(np.linalg.det([np.asarray(a.get_cell(complete=True)) for a in frames]))
        row[key] = dict(us_per_step=t.tolist(), median=float(np.median(t)), min=float(t.min()), max=float(t.max()),
                        list_builds=int(loop.n_rebuilds), largest_volume_change_relative=float(np.abs(V / V0 - 1.0).max()))
        loop.eng.close()
    return row


def write_report(prefix, rows, other, argv):
    with open(prefix + ".json", "w") as fp:
        json.dump(dict(script="scripts/bench_md_mtk.py", command="python " + " ".join(argv), rows=rows, other=other), fp, indent=1)

    def cell(d):
        return f"{d['median']:.1f} ({d['min']:.1f} .. {d['max']:.1f}), {d['list_builds']}"
    paths = [p for p in PATHS if p in rows[0]]
    lines = ["# Device MD loop under the Martyna-Tobias-Klein barostat", "",
             "Written by `python " + " ".join(argv) + "`: microseconds per step, median (min .. max) over the windows, then the",
             "neighbour lists built during all windows of the path (warm-up included; a loop that moves its cell builds one",
             "per window for its final cells). The paths alternate window by window in one process; all of them run the",
             "Nose-Hoover chain and launch one workgroup of 1024 threads per frame.", "",
             "| workload | atoms | steps x windows | " + " | ".join(TITLES[p] for p in paths) + " |",
             "|---|---|---|" + "---|" * len(paths)]
    for r in rows:
        lines.append(f"| {r['workload']} | {r['n_frames']} x {r['n_atoms'] // r['n_frames']} | "
                     f"{r['steps_per_window']} x {r['windows']} | " + " | ".join(cell(r[p]) for p in paths) + " |")
    if "mtk_iso" in paths and "npt_chain" in paths:
        lines += ["", "MTK, isotropic minus Berendsen-NPT + chain, medians: " +
                  ", ".join(f"{r['workload']} {r['mtk_iso']['median'] - r['npt_chain']['median']:+.1f} us" for r in rows) +
                  "; largest |V / V0 - 1| of the isotropic path: " +
                  ", ".join(f"{r['workload']} {r['mtk_iso']['largest_volume_change_relative']:.1e}" for r in rows) + "."]
    if other:
        lines += ["", "## The untouched paths before this barostat", "",
                  "The same script with `--paths chain,npt_chain` in a checkout of the parent commit, in the same session on the",
                  "same device, beside this build's numbers for those paths.", "",
                  "| workload | chain, parent | chain, this build | Berendsen-NPT + chain, parent | Berendsen-NPT + chain, this build |",
                  "|---|---|---|---|---|"]
        by_name = {r["workload"]: r for r in other}
        for r in rows:
            o = by_name.get(r["workload"])
            if o:
                lines.append(f"| {r['workload']} | {cell(o['chain'])} | {cell(r['chain'])} | {cell(o['npt_chain'])} | "
                             f"{cell(r['npt_chain'])} |")
    r0 = rows[0]
    lines += ["", f"Chains of 3 thermostats, 1 loop per half-update; tdamp = {r0['tau_steps']:g} steps, pdamp = "
              f"{rows[-1]['pdamp_steps']:g} steps (sf: {r0['pdamp_steps']:g}), taup = {r0['taup_steps']:g} steps. No threshold is set on "
              "these numbers."]
    with open(prefix + ".md", "w") as fp:
        fp.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="sf,eam,eam64")
    ap.add_argument("--paths", default=",".join(PATHS))
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skin", type=float, default=0.5)
    ap.add_argument("--tau-steps", type=float, default=100.0, help="time constant of the chain, in steps")
    ap.add_argument("--pdamp-steps", type=float, default=1000.0, help="time constant of the MTK barostat, in steps")
    ap.add_argument("--taup-steps", type=float, default=20.0, help="time constant of the Berendsen barostat, in steps")
    ap.add_argument("--other", default=None, help=".json of a run of this script on another commit, for the report")
    ap.add_argument("--out", default=None, help="prefix of the .json / .md report")
    args = ap.parse_args()
    paths = [p for p in args.paths.split(",") if p]
    if not paths or any(p not in PATHS for p in paths):
        ap.error("--paths: a comma-separated choice of " + ", ".join(PATHS))
    rows = []
    for name in args.workloads.split(","):
        rows.append(measure(name, paths, args.steps, args.repeats, args.skin, args.tau_steps, args.pdamp_steps, args.taup_steps))
        print(json.dumps(rows[-1]), flush=True)
    other = None
    if args.other:
        with open(args.other) as fp:
            other = json.load(fp)["rows"]
    if args.out:
        write_report(args.out, rows, other, ["scripts/bench_md_mtk.py"] + [a for a in sys.argv[1:]])


if __name__ == "__main__":
    main()
