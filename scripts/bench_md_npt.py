#!/usr/bin/env python3
"""Atom-steps per second of the device-resident NPT loop (`Engine.md_set_barostat` + `Engine.md_run`: Berendsen
thermostat and Berendsen barostat) against the host-driven one: the same scheme in NumPy around
`Engine.step(x, cells=h)`, on the same model, frames, velocities and step. A host-driven loop hands the library
a new cell at every step, which `ta_update_positions` answers with a new neighbour list; the device loop keeps
its list while the strain-aware skin test holds. A third path is the device loop with the Berendsen thermostat
alone (NVT) on the same frames: the distance between its time per step and the NPT loop's is what the barostat
adds: the virial in the evaluation, three sums in place of one, the cell update, the strain-aware list test and
the list build for the final cells of every window.

One process, one engine per path (each following its own trajectory), the paths alternating window by window:
`--repeats` windows of `--steps` steps each after one warm-up window per path. Every window ends with a device
synchronise. Device and host take the same steps from the same start: the largest relative gap between their
volumes after the last window is reported. Workloads as scripts/bench_md_device.py (sf, eam, eam64); the
symmetry-function model has random weights, a pressure of its own of the order of -1 eV / A^3 and the wrong sign
of stiffness (the pressure falls as the cell shrinks), so its target pressure is the pressure of its initial state
and its compressibility 1000 times smaller, which keeps the cell from running away inside the windows. The work
per step does not depend on the size of the factors while the list holds.

    python scripts/bench_md_npt.py --out profiles/md_npt_loop          # .json and .md
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

from bench_md_device import setup  # noqa: E402
from tensoralloy_amd import Engine, _lib, md  # noqa: E402

WANT = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES | _lib.TA_WANT_VIRIAL
BETA = 0.9          # A^3 / eV
TAU_STEPS = 20.0    # taut = taup = 20 steps


def _cells(frames):
    return np.ascontiguousarray([np.asarray(a.get_cell(complete=True)) for a in frames], dtype=np.float64)


class HostNPT:
    """The scheme of `ta_md_run` under the barostat in NumPy around `Engine.step(x, cells=h)`, all frames at
    once (they have the same size): what a caller does without `md_set_barostat`."""

    def __init__(self, nn, frames, v0, masses, dt, skin, kT0, p0, beta):
        self.eng = Engine(nn)
        self.eng.set_skin(skin)
        self.eng.set_frames(frames)
        self.F, self.n = len(frames), len(frames[0])
        assert len({len(a) for a in frames}) == 1
        self.x = np.ascontiguousarray(np.concatenate([a.positions for a in frames]))
        self.h = _cells(frames)
        self.v = v0.copy()
        self.m = masses.reshape(self.F, self.n, 1)
        self.dt, self.kT0, self.p0, self.beta = dt, kT0, p0, beta
        self.rebuilds0 = self.eng.list_stats()[0]
        self.res = self.eng.step(self.x, WANT, cells=self.h)
        self.eng.synchronize()

    def pressure(self):
        """Per frame and axis, of the current state."""
        S = (self.m * self.v.reshape(self.F, self.n, 3) ** 2).sum(axis=1)
        W = np.diagonal(self.res["virial"], axis1=1, axis2=2)
        return (S - W) / np.abs(np.linalg.det(self.h))[:, None]

    def run(self, steps):
        F, n, dt, m = self.F, self.n, self.dt, self.m
        k_t, k_p = 1.0 / TAU_STEPS, 1.0 / TAU_STEPS * self.beta / 3.0
        for _ in range(steps):
            f = np.array(self.res["forces"]).reshape(F, n, 3)
            W = np.diagonal(self.res["virial"], axis1=1, axis2=2)
            v = self.v.reshape(F, n, 3)
            S = (m * v * v).sum(axis=1)
            kT = S.sum(axis=1) / (3.0 * n)
            lam = np.clip(np.sqrt(1.0 + (self.kT0 / kT - 1.0) * k_t), 0.9, 1.1)
            v *= lam[:, None, None]
            P = ((lam * lam)[:, None] * S - W) / np.abs(np.linalg.det(self.h))[:, None]
            mu = 1.0 - k_p * (self.p0 - P.mean(axis=1))
            v += 0.5 * dt * f / m
            x = self.x.reshape(F, n, 3) * mu[:, None, None] + dt * v
            self.h = np.ascontiguousarray(self.h * mu[:, None, None])
            self.x = np.ascontiguousarray(x.reshape(-1, 3))
            self.res = self.eng.step(self.x, WANT, cells=self.h)
            v += 0.5 * dt * np.array(self.res["forces"]).reshape(F, n, 3) / m
            self.v = v.reshape(-1, 3)
        self.eng.synchronize()

    def volumes(self):
        return np.abs(np.linalg.det(self.h))

    def rebuilds(self):
        return self.eng.list_stats()[0] - self.rebuilds0


class DeviceMD:
    """`Engine.md_run` under the Berendsen thermostat, with the barostat (`p0` not None) or without."""

    def __init__(self, nn, frames, v0, masses, dt, skin, kT0, p0=None, beta=BETA):
        self.eng = Engine(nn)
        self.eng.set_skin(skin)
        self.eng.set_frames(frames)
        self.eng.md_init(masses, v0)
        self.eng.md_set_thermostat(kT0, TAU_STEPS * dt)
        if p0 is not None:
            self.eng.md_set_barostat(p0, TAU_STEPS * dt, beta)
        self.dt = dt
        self.n_rebuilds = 0

    def run(self, steps):
        self.n_rebuilds += self.eng.md_run(steps, self.dt, record_every=max(steps, 1))["n_rebuilds"]
        self.eng.synchronize()

    def volumes(self):
        return np.abs(np.linalg.det(self.eng.md_cells()))

    def rebuilds(self):
        return self.n_rebuilds


def measure(name, steps, repeats, skin):
    nn, frames, v0, masses, dt, T = setup(name, skin)
    n_atoms = len(masses)
    kT0 = md.kB * T
    beta = 1e-3 * BETA if name == "sf" else BETA
    host = HostNPT(nn, frames, v0, masses, dt, skin, kT0, 0.0, beta)
    # (a random network holds no lattice at P = 0: its target is where it starts)
    p0 = float(host.pressure().mean()) if name == "sf" else 0.0
    host.p0 = p0
    V0 = host.volumes()
    loops = {"device": DeviceMD(nn, frames, v0, masses, dt, skin, kT0, p0, beta), "host": host,
             "nvt": DeviceMD(nn, frames, v0, masses, dt, skin, kT0)}
    for loop in loops.values():   # warm-up: every shape of every path once
        loop.run(steps)
    rates = {k: [] for k in loops}
    for _ in range(repeats):
        for key, loop in loops.items():
            t0 = time.perf_counter()
            loop.run(steps)
            rates[key].append(n_atoms * steps / (time.perf_counter() - t0))
    Vd, Vh = loops["device"].volumes(), host.volumes()
    row = dict(workload=name, n_frames=len(frames), n_atoms=n_atoms, steps_per_window=steps, windows=repeats, skin=skin,
               temperature_K=T, dt_fs=dt / md.fs, target_pressure_eV_A3=p0, compressibility_A3_eV=beta,
               tau_steps=TAU_STEPS, volume_gap_relative=float(np.abs(Vd / Vh - 1.0).max()),
               largest_volume_change_relative=float(np.abs(Vd / V0 - 1.0).max()))
    for key, loop in loops.items():
        r = np.array(rates[key])
        row[key] = dict(atom_steps_per_s=r.tolist(), median=float(np.median(r)), min=float(r.min()),
                        max=float(r.max()), list_builds=int(loop.rebuilds()),
                        us_per_step=float(n_atoms / np.median(r) * 1e6))
        loop.eng.close()
    row["npt_minus_nvt_us_per_step"] = row["device"]["us_per_step"] - row["nvt"]["us_per_step"]
    row["device_over_host"] = row["device"]["median"] / row["host"]["median"]
    return row


def write_report(prefix, rows):
    with open(prefix + ".json", "w") as fp:
        json.dump(dict(script="scripts/bench_md_npt.py", rows=rows), fp, indent=1)
    lines = ["# Device-resident NPT loop against the host-driven one", "",
             "Written by `scripts/bench_md_npt.py`: atom-steps/s, median (min .. max) over the windows; the paths",
             "alternate window by window in one process. Berendsen thermostat at the workload's temperature and",
             f"Berendsen barostat, isotropic, taut = taup = {TAU_STEPS:g} steps, beta = {BETA:g} A^3 / eV, P0 = 0 (sf, a random",
             "network with the wrong sign of stiffness: the pressure of its initial state and beta / 1000, see the",
             "script). The host path is the same scheme in NumPy around",
             "`Engine.step(x, cells=h)`; a new cell means a new neighbour list there at every step. `builds` =",
             "neighbour lists built during all windows of the path (warm-up included; the device loop builds one per",
             "window for its final cells). No ratio is a gate.", "",
             "| workload | atoms | steps x windows | device `md_run`, NPT | builds | host `step(cells=)` + NumPy | builds | device / host | volume gap, relative | largest \\|V / V0 - 1\\| |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        def cell(d):
            return f"{d['median'] / 1e6:.2f} M ({d['min'] / 1e6:.2f} .. {d['max'] / 1e6:.2f})"
        lines.append(f"| {r['workload']} | {r['n_frames']} x {r['n_atoms'] // r['n_frames']} | "
                     f"{r['steps_per_window']} x {r['windows']} | {cell(r['device'])} | {r['device']['list_builds']} | "
                     f"{cell(r['host'])} | {r['host']['list_builds']} | {r['device_over_host']:.2f} | "
                     f"{r['volume_gap_relative']:.1e} | {r['largest_volume_change_relative']:.1e} |")
    lines += ["", "## Beside the NVT step", "",
              "`Engine.md_run` with the Berendsen thermostat alone on the same frames, same windows: time per step from",
              "the median rate. The difference is what the barostat adds: the virial in the evaluation, three sums in",
              "place of one and the cell update in the integrator launch, and whatever the two trajectories' list",
              "builds differ by (the end-of-window build for the final cells included).", "",
              "| workload | atoms | NVT, us / step | builds | NPT, us / step | builds | NPT - NVT, us |",
              "|---|---|---|---|---|---|---|"]
    for r in rows:
        d, g = r["nvt"], r["device"]
        lines.append(f"| {r['workload']} | {r['n_frames']} x {r['n_atoms'] // r['n_frames']} | {d['us_per_step']:.1f} | "
                     f"{d['list_builds']} | {g['us_per_step']:.1f} | {g['list_builds']} | "
                     f"{r['npt_minus_nvt_us_per_step']:+.1f} |")
    with open(prefix + ".md", "w") as fp:
        fp.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="sf,eam,eam64")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
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
