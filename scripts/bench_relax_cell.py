#!/usr/bin/env python3
"""Atom-steps per second of the device-resident relaxation with cells (`Engine.relax_set_cell` +
`Engine.relax_run`) against the host-driven one: the same scheme (ASE's `UnitCellFilter` under FIRE) in NumPy
around `Engine.step(x, cells=h)`, on the same model, frames and parameters. A host-driven loop hands the
library a new cell at every step, which `ta_update_positions` answers with a new neighbour list; the device
loop keeps its list while the strain-aware skin test holds. A third path is the device loop with fixed cells
on the same frames: the distance between its time per step and the cell loop's is what the cell rows, the
q = x G^-T / x = q G'^T transforms, the virial and the extra list builds cost.

One process, one engine per path, the paths alternating window by window: `--repeats` windows of `--steps`
FIRE steps each after one warm-up window per path. `fmax` is so small that no frame converges; every window
starts again from the jittered lattice in the start cell (the reset is not timed) and ends with a device
synchronise. Device and host take the same steps from the same start, so they must end at the same energies:
the largest per-frame gap is reported. Workloads as scripts/bench_relax_device.py (sf, eam, eam64).

    python scripts/bench_relax_cell.py --out profiles/relax_cell_loop          # .json and .md

What stands below the line `<!-- kept -->` of an existing .md report is carried over.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

from bench_md_device import workload  # noqa: E402
from bench_relax_device import FIRE, FMAX, KEPT, DeviceFire  # noqa: E402
from tensoralloy_amd import Engine, _lib  # noqa: E402

WANT = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES | _lib.TA_WANT_VIRIAL


def _cells(frames):
    return np.ascontiguousarray([np.asarray(a.get_cell(complete=True)) for a in frames], dtype=np.float64)


class HostCellFire:
    """The cell scheme in NumPy around `Engine.step(x, cells=h)`, all frames at once (they have the same size):
    what a caller does without `relax_set_cell`."""

    def __init__(self, nn, frames, skin, fire):
        self.eng = Engine(nn)
        self.eng.set_skin(skin)
        self.eng.set_frames(frames)
        self.p = fire
        self.F = len(frames)
        assert len({len(a) for a in frames}) == 1
        self.n = len(frames[0])
        self.x0 = np.ascontiguousarray(np.concatenate([a.positions for a in frames]))
        self.h0 = _cells(frames)
        self.rebuilds0 = self.eng.list_stats()[0]
        self.steps = 0
        self.reset()

    def reset(self):
        """Back to the start of the relaxation (not timed)."""
        F = self.F
        self.x, self.h = self.x0.copy(), self.h0.copy()
        self.G = np.tile(np.eye(3), (F, 1, 1))
        self.v = np.zeros((F, self.n + 3, 3))
        self.dt = np.full(F, self.p["dt"])
        self.a = np.full(F, self.p["astart"])
        self.npos = np.zeros(F, dtype=np.int64)
        self.first = True
        self.res = self.eng.step(self.x, WANT, cells=self.h)
        self.eng.synchronize()

    def run(self, steps):
        F, n, p = self.F, self.n, self.p
        dt, a, npos, v = self.dt, self.a, self.npos, self.v
        self.steps = 0
        for _ in range(steps):
            G = self.G
            Gi = np.linalg.inv(G)
            f = np.empty((F, n + 3, 3))
            f[:, :n] = self.res["forces"].reshape(F, n, 3) @ G
            f[:, n:] = -(self.res["virial"] @ Gi.transpose(0, 2, 1)) / n      # p = 0, cell factor n
            f2 = np.einsum("fij,fij->fi", f, f).max(axis=1)
            active = f2 >= FMAX * FMAX
            if not active.any():
                break
            if self.first:
                self.first = False
            else:
                vf = np.einsum("fij,fij->f", f, v)
                ff = np.einsum("fij,fij->f", f, f)
                vv = np.einsum("fij,fij->f", v, v)
                down = vf > 0.0
                v *= np.where(down, 1.0 - a, 0.0)[:, None, None]
                v += f * np.where(down, a * np.sqrt(vv) / np.sqrt(ff), 0.0)[:, None, None]
                grow = down & (npos > p["nmin"])
                dt[grow] = np.minimum(dt[grow] * p["finc"], p["dtmax"])
                a[grow] *= p["fa"]
                npos[down] += 1
                up = ~down
                npos[up] = 0
                dt[up] *= p["fdec"]
                a[up] = p["astart"]
            v += f * dt[:, None, None]
            dr = v * dt[:, None, None]
            norm = np.sqrt(np.einsum("fij,fij->f", dr, dr))
            dr *= (np.where(norm > p["maxstep"], p["maxstep"] / np.maximum(norm, 1e-300), 1.0) * active)[:, None, None]
            q = self.x.reshape(F, n, 3) @ Gi.transpose(0, 2, 1) + dr[:, :n]
            self.G = G + dr[:, n:] / n
            self.h = np.ascontiguousarray(self.h0 @ self.G.transpose(0, 2, 1))
            self.x = np.ascontiguousarray((q @ self.G.transpose(0, 2, 1)).reshape(-1, 3))
            self.res = self.eng.step(self.x, WANT, cells=self.h)
            self.steps += 1
        self.eng.synchronize()

    def energies(self):
        return np.array(self.res["energy"], dtype=np.float64)

    def rebuilds(self):
        return self.eng.list_stats()[0] - self.rebuilds0


class DeviceCellFire(DeviceFire):
    def __init__(self, nn, frames, skin, fire):
        self.h0 = _cells(frames)
        super().__init__(nn, frames, skin, fire)

    def reset(self):
        """Back to the start of the relaxation, start cell included (not timed)."""
        self.eng.update_positions(self.x0, self.h0)
        self.eng.relax_init(**self.fire)
        self.eng.relax_set_cell(True)
        self.eng.synchronize()


def measure(name, steps, repeats, skin):
    nn, frames, _, _ = workload(name)
    n_atoms = sum(len(a) for a in frames)
    # (the symmetry-function model has random weights and holds no lattice: short steps, as in bench_relax_device)
    fire = dict(FIRE, maxstep=0.002) if name == "sf" else dict(FIRE)
    loops = {"device": DeviceCellFire(nn, frames, skin, fire), "host": HostCellFire(nn, frames, skin, fire),
             "fixed": DeviceFire(nn, frames, skin, fire)}
    for loop in loops.values():   # warm-up: every shape of every path once
        loop.run(min(steps, 100))
    rates = {k: [] for k in loops}
    all_steps = True
    for _ in range(repeats):
        for key, loop in loops.items():
            loop.reset()
            t0 = time.perf_counter()
            loop.run(steps)
            rates[key].append(n_atoms * steps / (time.perf_counter() - t0))
            all_steps = all_steps and loop.steps == steps
    gap = float(np.abs(loops["device"].energies() - loops["host"].energies()).max())
    strain = float(np.abs(loops["device"].eng.relax_cell_state()["deform"] - np.eye(3)).max())
    row = dict(workload=name, n_frames=len(frames), n_atoms=n_atoms, steps_per_window=steps, windows=repeats,
               skin=skin, fmax=FMAX, fire=fire, energy_gap_eV=gap, same_energies=bool(gap <= 1e-9),
               largest_strain_component=strain, every_window_took_all_steps=bool(all_steps))
    for key, loop in loops.items():
        r = np.array(rates[key])
        row[key] = dict(atom_steps_per_s=r.tolist(), median=float(np.median(r)), min=float(r.min()),
                        max=float(r.max()), list_builds=int(loop.rebuilds()),
                        us_per_step=float(n_atoms / np.median(r) * 1e6))
        loop.eng.close()
    row["cell_minus_fixed_us_per_step"] = row["device"]["us_per_step"] - row["fixed"]["us_per_step"]
    row["device_over_host"] = row["device"]["median"] / row["host"]["median"]
    return row


def write_report(prefix, rows):
    with open(prefix + ".json", "w") as fp:
        json.dump(dict(script="scripts/bench_relax_cell.py", rows=rows), fp, indent=1)
    kept = []
    if os.path.exists(prefix + ".md"):
        old = open(prefix + ".md").read().split("\n")
        if KEPT in old:
            kept = old[old.index(KEPT):]
    lines = ["# Device-resident relaxation with cells against the host-driven one", "",
             "Written by `scripts/bench_relax_cell.py`: atom-steps/s, median (min .. max) over the windows; the paths",
             "alternate window by window in one process. FIRE with ASE's default parameters (sf: `maxstep` 0.002), cell",
             f"factor = atoms of the frame, p = 0, all six strain components free, `fmax` = {FMAX:g} (every window starts",
             "from the jittered lattice in the start cell and takes all its steps). The host path is the same scheme in",
             "NumPy around `Engine.step(x, cells=h)`; a new cell means a new neighbour list there at every step.",
             "`builds` = neighbour lists built during all windows of the path (warm-up included; the device loop",
             "builds one per window for its final cells). No ratio is a gate.", "",
             "| workload | atoms | steps x windows | device `relax_run`, cells | builds | host `step(cells=)` + NumPy | builds | device / host | energy gap, eV | largest \\|G - I\\| |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        def cell(d):
            return f"{d['median'] / 1e6:.2f} M ({d['min'] / 1e6:.2f} .. {d['max'] / 1e6:.2f})"
        lines.append(f"| {r['workload']} | {r['n_frames']} x {r['n_atoms'] // r['n_frames']} | "
                     f"{r['steps_per_window']} x {r['windows']} | {cell(r['device'])} | {r['device']['list_builds']} | "
                     f"{cell(r['host'])} | {r['host']['list_builds']} | {r['device_over_host']:.2f} | "
                     f"{r['energy_gap_eV']:.1e} | {r['largest_strain_component']:.1e} |")
    short = [r["workload"] for r in rows if not r["every_window_took_all_steps"]]
    if short:
        lines += ["", "INVALID: a frame converged inside a window on " + ", ".join(short) + "."]
    off = [r["workload"] for r in rows if not r["same_energies"]]
    lines += ["", "Both paths end at the same energies to 1e-9 eV per frame: " +
              ("yes, on every workload." if not off else "NO on " + ", ".join(off) + " (gaps in the table).")]
    lines += ["", "## Beside the fixed-cell step", "",
              "`Engine.relax_run` with fixed cells on the same frames, same windows: time per step from the median",
              "rate. The difference is what a cell step adds: the virial in the evaluation, the cell rows and the two",
              "3 x 3 transforms per atom in the step launch, and whatever the two trajectories' list builds differ by",
              "(the end-of-window build for the final cells included).", "",
              "| workload | atoms | fixed cells, us / step | builds | cells, us / step | builds | cell - fixed, us |",
              "|---|---|---|---|---|---|---|"]
    for r in rows:
        d, g = r["fixed"], r["device"]
        lines.append(f"| {r['workload']} | {r['n_frames']} x {r['n_atoms'] // r['n_frames']} | {d['us_per_step']:.1f} | "
                     f"{d['list_builds']} | {g['us_per_step']:.1f} | {g['list_builds']} | "
                     f"{r['cell_minus_fixed_us_per_step']:+.1f} |")
    with open(prefix + ".md", "w") as fp:
        fp.write("\n".join(lines + [""] + kept) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="sf,eam,eam64")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--skin", type=float, default=0.5)
    ap.add_argument("--out", default=None, help="prefix of the .json / .md report")
    args = ap.parse_args()
    rows = []
    for name in args.workloads.split(","):
        rows.append(measure(name, args.steps, args.repeats, args.skin))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        write_report(args.out, rows)


if __name__ == "__main__":
    main()
