#!/usr/bin/env python3
"""Atom-steps per second of the device-resident relaxation (`Engine.relax_run`) against the host-driven one
(the same FIRE in NumPy around `Engine.step(view=True)`) on the same model, frames and parameters.

One process, one engine per path, the paths alternating window by window: `--repeats` windows of `--steps`
FIRE steps each after one warm-up window per path. `fmax` is so small that no frame converges, so every window
starts again from the jittered lattice (the reset is not timed) and takes exactly `--steps` steps of every
frame, which the report checks; every window ends with a device synchronise. Both paths take
the same steps from the same start, so they must end at the same energies: the largest per-frame gap is
reported and checked against 1e-9 eV. A third path is `Engine.md_run` (velocity Verlet, no thermostat) on the
same frames: the distance between its time per step and the relaxation's is what the second launch and the
reductions cost. Workloads as scripts/bench_md_device.py:

    sf     bench.ni_frame / bench.ni_model: one 4000-atom Ni frame, G2 + G4 symmetry functions
    eam    the same frame with the Ni zjw04 EAM
    eam64  64 such frames (different jitter) in one batch, zjw04 EAM

    python scripts/bench_relax_device.py --out profiles/relax_device_loop          # .json and .md

What stands below the line `<!-- kept -->` of an existing .md report is carried over (kernel resources and
test gaps are written there by hand).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

from bench_md_device import DeviceLoop as MdLoop, setup as md_setup, workload  # noqa: E402
from tensoralloy_amd import Engine, _lib  # noqa: E402

WANT = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES
FMAX = 1e-12   # never reached
FIRE = dict(dt=0.1, dtmax=1.0, maxstep=0.2, finc=1.1, fdec=0.5, astart=0.1, fa=0.99, nmin=5)
KEPT = "<!-- kept -->"


class HostFire:
    """FIRE in NumPy around `Engine.step(view=True)`, all frames at once (they have the same size): what a
    caller does without `relax_run`."""

    def __init__(self, nn, frames, skin, fire):
        self.eng = Engine(nn)
        self.eng.set_skin(skin)
        self.eng.set_frames(frames)
        self.p = fire
        self.F = len(frames)
        assert len({len(a) for a in frames}) == 1
        self.x0 = np.ascontiguousarray(np.concatenate([a.positions for a in frames]))
        self.x, self.v, self.tmp = self.x0.copy(), np.zeros_like(self.x0), np.empty_like(self.x0)
        self.rebuilds0 = self.eng.list_stats()[0]
        self.steps = 0
        self.reset()

    def reset(self):
        """Back to the start of the relaxation (not timed)."""
        self.x[:] = self.x0
        self.v[:] = 0.0
        self.dt = np.full(self.F, self.p["dt"])
        self.a = np.full(self.F, self.p["astart"])
        self.npos = np.zeros(self.F, dtype=np.int64)
        self.first = True
        self.res = self.eng.step(self.x, WANT, view=True)
        self.eng.synchronize()

    def run(self, steps):
        F, p, step = self.F, self.p, self.eng.step
        x, v, tmp = self.x.reshape(F, -1), self.v.reshape(F, -1), self.tmp.reshape(F, -1)
        dt, a, npos = self.dt, self.a, self.npos
        f = self.res["forces"]
        self.steps = 0
        for _ in range(steps):
            f2 = np.einsum("ij,ij->i", f, f).reshape(F, -1).max(axis=1)
            active = f2 >= FMAX * FMAX
            if not active.any():
                break
            f = f.reshape(F, -1)
            if self.first:
                self.first = False
            else:
                vf = np.einsum("ij,ij->i", f, v)
                ff = np.einsum("ij,ij->i", f, f)
                vv = np.einsum("ij,ij->i", v, v)
                down = vf > 0.0
                v *= np.where(down, 1.0 - a, 0.0)[:, None]
                np.multiply(f, np.where(down, a * np.sqrt(vv) / np.sqrt(ff), 0.0)[:, None], out=tmp)
                v += tmp
                grow = down & (npos > p["nmin"])
                dt[grow] = np.minimum(dt[grow] * p["finc"], p["dtmax"])
                a[grow] *= p["fa"]
                npos[down] += 1
                up = ~down
                npos[up] = 0
                dt[up] *= p["fdec"]
                a[up] = p["astart"]
            np.multiply(f, dt[:, None], out=tmp)
            v += tmp
            np.multiply(v, dt[:, None], out=tmp)
            norm = np.sqrt(np.einsum("ij,ij->i", tmp, tmp))
            scale = np.where(norm > p["maxstep"], p["maxstep"] / np.maximum(norm, 1e-300), 1.0) * active
            tmp *= scale[:, None]
            x += tmp
            self.res = step(self.x, WANT, view=True)
            f = self.res["forces"]
            self.steps += 1
        self.eng.synchronize()

    def energies(self):
        return np.array(self.res["energy"], dtype=np.float64)

    def rebuilds(self):
        return self.eng.list_stats()[0] - self.rebuilds0


class DeviceFire:
    def __init__(self, nn, frames, skin, fire):
        self.eng = Engine(nn)
        self.eng.set_skin(skin)
        self.eng.set_frames(frames)
        self.fire = fire
        self.x0 = np.ascontiguousarray(np.concatenate([a.positions for a in frames]))
        self.n_rebuilds = 0
        self.out = None
        self.steps = 0
        self.reset()

    def reset(self):
        """Back to the start of the relaxation (not timed)."""
        self.eng.update_positions(self.x0)
        self.eng.relax_init(**self.fire)
        self.eng.synchronize()

    def run(self, steps):
        self.out = self.eng.relax_run(steps, FMAX)
        self.n_rebuilds += self.out["n_rebuilds"]
        self.steps = int(self.out["steps"].min())
        self.eng.synchronize()

    def energies(self):
        return self.out["energy"]

    def rebuilds(self):
        return self.n_rebuilds


def measure(name, steps, repeats, skin):
    nn, frames, _, _ = workload(name)
    n_atoms = sum(len(a) for a in frames)
    _, _, v0, masses, dt_md, _ = md_setup(name, skin)
    # The symmetry-function model has random weights and is no potential that holds a lattice (see
    # bench_md_device.workload): its steps are kept short, so that all windows together move an atom by
    # less than 0.1 A. The work per step does not depend on the step length while the list holds.
    fire = dict(FIRE, maxstep=0.002) if name == "sf" else dict(FIRE)
    loops = {"device": DeviceFire(nn, frames, skin, fire), "host": HostFire(nn, frames, skin, fire),
             "md_run": MdLoop(nn, frames, v0, masses, dt_md, skin)}
    for loop in loops.values():   # warm-up: every shape of every path once
        loop.run(min(steps, 100))
    rates = {k: [] for k in loops}
    all_steps = True
    for _ in range(repeats):
        for key, loop in loops.items():
            if key != "md_run":   # every window relaxes the jittered start again: nothing gets near a minimum
                loop.reset()
            t0 = time.perf_counter()
            loop.run(steps)
            rates[key].append(n_atoms * steps / (time.perf_counter() - t0))
            if key != "md_run":
                all_steps = all_steps and loop.steps == steps
    gap = float(np.abs(loops["device"].energies() - loops["host"].energies()).max())
    row = dict(workload=name, n_frames=len(frames), n_atoms=n_atoms, steps_per_window=steps, windows=repeats,
               skin=skin, fmax=FMAX, fire=fire, energy_gap_eV=gap, same_energies=bool(gap <= 1e-9),
               every_window_took_all_steps=bool(all_steps))
    for key, loop in loops.items():
        r = np.array(rates[key])
        row[key] = dict(atom_steps_per_s=r.tolist(), median=float(np.median(r)), min=float(r.min()),
                        max=float(r.max()), list_builds=int(loop.rebuilds()),
                        us_per_step=float(n_atoms / np.median(r) * 1e6))
        loop.eng.close()
    row["relax_minus_md_us_per_step"] = row["device"]["us_per_step"] - row["md_run"]["us_per_step"]
    row["device_over_host"] = row["device"]["median"] / row["host"]["median"]
    row["device_no_slower"] = bool(row["device"]["median"] >= row["host"]["median"])
    return row


def write_report(prefix, rows):
    with open(prefix + ".json", "w") as fp:
        json.dump(dict(script="scripts/bench_relax_device.py", rows=rows), fp, indent=1)
    kept = []
    if os.path.exists(prefix + ".md"):
        old = open(prefix + ".md").read().split("\n")
        if KEPT in old:
            kept = old[old.index(KEPT):]
    lines = ["# Device-resident relaxation against the host-driven one", "",
             "Written by `scripts/bench_relax_device.py`: atom-steps/s, median (min .. max) over the windows; the",
             "paths alternate window by window in one process. FIRE with ASE's default parameters (sf: `maxstep` 0.002), `fmax` = "
             f"{FMAX:g}", "(every window starts from the jittered lattice and takes all its steps). `builds` = neighbour lists built "
             "during all windows", "of the path (warm-up included).", "",
             "| workload | atoms | steps x windows | device `relax_run` | builds | host `step` + NumPy FIRE | builds | device / host | energy gap, eV |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        def cell(d):
            return f"{d['median'] / 1e6:.2f} M ({d['min'] / 1e6:.2f} .. {d['max'] / 1e6:.2f})"
        lines.append(f"| {r['workload']} | {r['n_frames']} x {r['n_atoms'] // r['n_frames']} | "
                     f"{r['steps_per_window']} x {r['windows']} | {cell(r['device'])} | {r['device']['list_builds']} | "
                     f"{cell(r['host'])} | {r['host']['list_builds']} | {r['device_over_host']:.2f} | "
                     f"{r['energy_gap_eV']:.1e} |")
    missed = [r["workload"] for r in rows if not r["device_no_slower"]]
    lines += ["", "Acceptance (device no slower than host, margin 0): " +
              ("met on every workload." if not missed else "MISSED on " + ", ".join(missed) + ".")]
    short = [r["workload"] for r in rows if not r["every_window_took_all_steps"]]
    if short:
        lines += ["", "INVALID: a frame converged inside a window on " + ", ".join(short) + "."]
    off = [r["workload"] for r in rows if not r["same_energies"]]
    lines += ["", "Both paths end at the same energies to 1e-9 eV per frame: " +
              ("yes, on every workload." if not off else "NO on " + ", ".join(off) + " (gaps in the table).")]
    lines += ["", "## Beside the velocity-Verlet step", "",
              "`Engine.md_run` without a thermostat on the same frames, same windows: time per step from the median",
              "rate. The difference is what the FIRE step adds to the one integrator launch of the MD loop (a second",
              "launch and four reductions) together with whatever the two trajectories' list builds differ by.",
              "Not a gate.", "",
              "| workload | atoms | `md_run`, us / step | builds | `relax_run`, us / step | builds | relax - md, us |",
              "|---|---|---|---|---|---|---|"]
    for r in rows:
        d, g = r["md_run"], r["device"]
        lines.append(f"| {r['workload']} | {r['n_frames']} x {r['n_atoms'] // r['n_frames']} | {d['us_per_step']:.1f} | "
                     f"{d['list_builds']} | {g['us_per_step']:.1f} | {g['list_builds']} | "
                     f"{r['relax_minus_md_us_per_step']:+.1f} |")
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
