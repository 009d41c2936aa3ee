#!/usr/bin/env python3
"""Atom-steps per second of the device-resident MD loop (`Engine.md_run`) against the host-driven loop
(`Engine.step(view=True)` + velocity Verlet in NumPy) on the same model, frames, velocities and step.

One process, one engine per path (each following its own trajectory), the paths alternating window by
window: `--repeats` windows of `--steps` steps each after one warm-up window per path and shape. Every
window ends with a device synchronise. A third path is the device loop with the Langevin thermostat
(bath at the workload's temperature, `--friction` per fs) on the same frames: its distance from the
velocity-Verlet device loop is what the counter-based noise costs per step. Workloads:

    sf     bench.ni_frame / bench.ni_model: one 4000-atom Ni frame, G2 + G4 symmetry functions
    eam    the same frame with the Ni zjw04 EAM
    eam64  64 such frames (different jitter) in one batch, zjw04 EAM

    python scripts/bench_md_device.py --out profiles/md_device_loop          # .json and .md
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_md_device.py --trace sf --steps 200

`--trace W`: only the device loop of workload W, once, for a kernel trace (run the profiler separately
from the timing: its hooks cost launch latency).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from bench import ni_frame, ni_model  # noqa: E402
from tensoralloy_amd import Engine, _lib, md  # noqa: E402
from tensoralloy_amd.atoms import atomic_masses  # noqa: E402

WANT = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES


def workload(name):
    """(model, frames, temperature in K, time step). The symmetry-function model has random weights and is
    no potential that holds a lattice (at 0.2 fs per step the frame collapses within 1000 steps): it is
    integrated cold and with a very short step, so that all windows together cover about 50 fs. The work
    per step does not depend on the step length while the list holds."""
    if name == "sf":
        return ni_model(), [ni_frame(611)], 30.0, 0.005 * md.fs
    from tensoralloy_amd import UniversalTransformer
    from tensoralloy_amd.eam import EamAlloyNN
    nn = EamAlloyNN(["Ni"], custom_potentials="zjw04")
    nn.attach_transformer(UniversalTransformer(["Ni"], rcut=6.5, angular=False))
    frames = [ni_frame(611 + k) for k in range(64 if name == "eam64" else 1)]
    return nn, frames, 300.0, 1.0 * md.fs


class HostLoop:
    """Velocity Verlet in NumPy around `Engine.step(view=True)`: what a caller does without `md_run`."""

    def __init__(self, nn, frames, v0, masses, dt, skin):
        self.eng = Engine(nn)
        self.eng.set_skin(skin)
        self.eng.set_frames(frames)
        self.x = np.ascontiguousarray(np.concatenate([a.positions for a in frames]))
        self.v = v0.copy()
        self.dt = dt
        self.half = (0.5 * dt / masses)[:, None]
        self.tmp = np.empty_like(self.x)
        self.rebuilds0 = self.eng.list_stats()[0]
        self.f = self.eng.step(self.x, WANT, view=True)["forces"]

    def run(self, steps):
        x, v, half, tmp, dt, step = self.x, self.v, self.half, self.tmp, self.dt, self.eng.step
        f = self.f
        for _ in range(steps):
            np.multiply(f, half, out=tmp)
            v += tmp
            np.multiply(v, dt, out=tmp)
            x += tmp
            f = step(x, WANT, view=True)["forces"]
            np.multiply(f, half, out=tmp)
            v += tmp
        self.f = f
        self.eng.synchronize()

    def rebuilds(self):
        return self.eng.list_stats()[0] - self.rebuilds0


class DeviceLoop:
    def __init__(self, nn, frames, v0, masses, dt, skin, langevin=None):
        self.eng = Engine(nn)
        self.eng.set_skin(skin)
        self.eng.set_frames(frames)
        self.eng.md_init(masses, v0)
        if langevin:
            self.eng.md_set_langevin(*langevin)   # (kT, friction, seed)
        self.dt = dt
        self.n_rebuilds = 0

    def run(self, steps):
        self.n_rebuilds += self.eng.md_run(steps, self.dt, record_every=max(steps, 1))["n_rebuilds"]
        self.eng.synchronize()

    def rebuilds(self):
        return self.n_rebuilds


def setup(name, skin):
    nn, frames, T, dt = workload(name)
    masses = np.array([atomic_masses[z] for a in frames for z in a.numbers])
    v0 = md.maxwell_boltzmann(masses, md.kB * T, np.random.RandomState(611))
    return nn, frames, v0, masses, dt, T


def noise_gap(eng, n_atoms, seed):
    """Largest |device - NumPy reference| over the normals of four steps (`Engine.md_noise` against
    tests/md_langevin_reference.py), the step beyond 2^32 among them."""
    from tests import md_langevin_reference
    gap = 0.0
    for step in (0, 1, 7, 2 ** 32 + 5):
        xi, eta = eng.md_noise(step)
        r_xi, r_eta = md_langevin_reference.normals(seed, step, n_atoms)
        gap = max(gap, float(np.abs(xi - r_xi).max()), float(np.abs(eta - r_eta).max()))
    return gap


def measure(name, steps, repeats, skin, friction_per_fs):
    nn, frames, v0, masses, dt, T = setup(name, skin)
    n_atoms = len(masses)
    langevin = (md.kB * T, friction_per_fs / md.fs, 611)
    loops = {"device": DeviceLoop(nn, frames, v0, masses, dt, skin), "host": HostLoop(nn, frames, v0, masses, dt, skin),
             "device_langevin": DeviceLoop(nn, frames, v0, masses, dt, skin, langevin)}
    for loop in loops.values():   # warm-up: every shape of both paths once
        loop.run(min(steps, 200))
    rates = {k: [] for k in loops}
    for _ in range(repeats):
        for key, loop in loops.items():
            t0 = time.perf_counter()
            loop.run(steps)
            rates[key].append(n_atoms * steps / (time.perf_counter() - t0))
    row = dict(workload=name, n_frames=len(frames), n_atoms=n_atoms, steps_per_window=steps, windows=repeats,
               skin=skin, temperature_K=T, dt_fs=dt / md.fs, friction_per_fs=friction_per_fs,
               noise_gap=noise_gap(loops["device_langevin"].eng, n_atoms, langevin[2]))
    for key, loop in loops.items():
        r = np.array(rates[key])
        row[key] = dict(atom_steps_per_s=r.tolist(), median=float(np.median(r)), min=float(r.min()),
                        max=float(r.max()), list_builds=int(loop.rebuilds()),
                        us_per_step=float(n_atoms / np.median(r) * 1e6))
        loop.eng.close()
    row["langevin_minus_nve_us_per_step"] = row["device_langevin"]["us_per_step"] - row["device"]["us_per_step"]
    row["device_over_host"] = row["device"]["median"] / row["host"]["median"]
    row["device_no_slower"] = bool(row["device"]["median"] >= row["host"]["median"])
    return row


def write_report(prefix, rows):
    with open(prefix + ".json", "w") as fp:
        json.dump(dict(script="scripts/bench_md_device.py", rows=rows), fp, indent=1)
    lines = ["# Device-resident MD loop against the host-driven loop", "",
             "Written by `scripts/bench_md_device.py`: atom-steps/s, median (min .. max) over the windows; the",
             "paths alternate window by window in one process. `builds` = neighbour lists built during all windows",
             "of the path (warm-up included).", "",
             "| workload | atoms | steps x windows | device `md_run` | builds | host `step` + NumPy | builds | device / host |",
             "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        def cell(d):
            return f"{d['median'] / 1e6:.2f} M ({d['min'] / 1e6:.2f} .. {d['max'] / 1e6:.2f})"
        lines.append(f"| {r['workload']} | {r['n_frames']} x {r['n_atoms'] // r['n_frames']} | "
                     f"{r['steps_per_window']} x {r['windows']} | {cell(r['device'])} | {r['device']['list_builds']} | "
                     f"{cell(r['host'])} | {r['host']['list_builds']} | {r['device_over_host']:.2f} |")
    missed = [r["workload"] for r in rows if not r["device_no_slower"]]
    lines += ["", "Acceptance (device no slower than host, margin 0): " +
              ("met on every workload." if not missed else "MISSED on " + ", ".join(missed) + ".")]
    lines += ["", "## Langevin thermostat", "",
              "The device loop with `md_set_langevin` (bath at the workload's temperature) beside the velocity-Verlet",
              "device loop of the table above, same frames, same windows: time per step from the median rate. The",
              "difference is the cost of the noise (per atom and launch six Philox4x32-10 blocks, log, sqrt and",
              "sincos in fp64) together with whatever the two trajectories' list builds differ by. Not a gate.", "",
              "| workload | atoms | friction (1/fs) | velocity Verlet, us / step | builds | Langevin, us / step | builds | Langevin - Verlet, us |",
              "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        d, g = r["device"], r["device_langevin"]
        lines.append(f"| {r['workload']} | {r['n_frames']} x {r['n_atoms'] // r['n_frames']} | {r['friction_per_fs']:g} | "
                     f"{d['us_per_step']:.1f} | {d['list_builds']} | {g['us_per_step']:.1f} | {g['list_builds']} | "
                     f"{r['langevin_minus_nve_us_per_step']:+.1f} |")
    lines += ["", "Noise against the NumPy reference (`Engine.md_noise`, all atoms of the workload, steps 0, 1, 7 and "
              "2^32 + 5), largest |difference|: " +
              ", ".join(f"{r['workload']} {r['noise_gap']:.2e}" for r in rows) + " (bound of the tests: 1e-13)."]
    with open(prefix + ".md", "w") as fp:
        fp.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="sf,eam,eam64")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skin", type=float, default=0.5)
    ap.add_argument("--friction", type=float, default=0.01, help="of the Langevin path, per fs")
    ap.add_argument("--langevin", action="store_true", help="with --trace: the Langevin device loop")
    ap.add_argument("--out", default=None, help="prefix of the .json / .md report")
    ap.add_argument("--trace", default=None, help="workload: one device run only, for a kernel trace")
    args = ap.parse_args()
    if args.trace:
        nn, frames, v0, masses, dt, T = setup(args.trace, args.skin)
        langevin = (md.kB * T, args.friction / md.fs, 611) if args.langevin else None
        loop = DeviceLoop(nn, frames, v0, masses, dt, args.skin, langevin)
        loop.run(args.steps)
        print(json.dumps(dict(trace=args.trace, langevin=bool(langevin), steps=args.steps, list_builds=loop.rebuilds())))
        loop.eng.close()
        return
    rows = []
    for name in args.workloads.split(","):
        rows.append(measure(name, args.steps, args.repeats, args.skin, args.friction))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        write_report(args.out, rows)


if __name__ == "__main__":
    main()
