#!/usr/bin/env python3
"""Atom-steps per second of the device-resident nudged elastic band (`Engine.relax_set_band` + `relax_run`)
against the host-driven one (the same band force and the same whole-band FIRE in NumPy around
`Engine.step(view=True)`) on the same model, images and parameters.

One process, one engine per path, the paths alternating window by window: `--repeats` windows of `--steps` band
steps each after one warm-up window per path. `fmax` is so small that the band never converges, so every window
starts again from the interpolated band (the reset is not timed) and takes exactly `--steps` steps, which the
report checks; every window ends with a device synchronise. Both paths take the same steps from the same start,
so they must end at the same energies: the largest per-image gap is reported and checked against 1e-9 eV. A
third path is a plain `Engine.relax_run` of the same batch as independent frames: the distance between its time
per step and the band's is what the two band launches cost. Both endpoint images are evaluated at every step on
every path (2 / n_images of the work).

The band is a vacancy hop in the jittered lattice of bench.ni_frame: atom 0 is taken out, and in the final state
its neighbour at (a/2, a/2, 0) sits in its place; linearly interpolated images, ASE's spring constant and a
climbing image. (A band whose images all relax towards the same lattice would make every energy gap along it
small, and the tangent weights, ratios of such gaps, would amplify the rounding of the energies: the two paths
would then drift apart for reasons that have nothing to do with either.) Workloads:

    sf8     8 images of bench.ni_frame / bench.ni_model with the vacancy: 3999 Ni atoms, G2 + G4 symmetry functions
    eam8    the same images with the Ni zjw04 EAM
    eam16   16 images of the 500-atom cell with the vacancy (499 atoms), zjw04 EAM

    python scripts/bench_neb.py --out profiles/neb_device_loop          # .json and .md
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

from bench import ni_frame, ni_model  # noqa: E402
from tensoralloy_amd import Atoms, Engine, _lib, interpolate  # noqa: E402

WANT = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES
FMAX = 1e-12   # never reached
FIRE = dict(dt=0.1, dtmax=1.0, maxstep=0.2, finc=1.1, fdec=0.5, astart=0.1, fa=0.99, nmin=5)
K_SPRING = 0.1


def hop_band(rep, n_images, a=3.524):
    """The images of a vacancy hop in ni_frame(611, rep) with atom 0 removed."""
    full = ni_frame(611, rep=rep, a=a)
    initial = Atoms(numbers=full.numbers[1:], positions=full.positions[1:],
                    cell=np.asarray(full.get_cell(complete=True)), pbc=True)
    final = initial.copy()
    j = int(np.argmin(((initial.positions - [a / 2, a / 2, 0.0]) ** 2).sum(axis=1)))
    final.positions[j] = full.positions[0]
    return interpolate(initial, final, n_images)


def workload(name):
    """(model, images)."""
    if name == "sf8":
        nn, n_images, rep = ni_model(), 8, 10
    else:
        from tensoralloy_amd import UniversalTransformer
        from tensoralloy_amd.eam import EamAlloyNN
        nn = EamAlloyNN(["Ni"], custom_potentials="zjw04")
        nn.attach_transformer(UniversalTransformer(["Ni"], rcut=6.5, angular=False))
        n_images, rep = (8, 10) if name == "eam8" else (16, 5)
    return nn, hop_band(rep, n_images)


def band_force(X, E, F, k, out, tmp):
    """B of the improved-tangent band with a climbing image into `out` [n_images, 3n] (rows 0 and -1 stay 0)."""
    dp, dm = X[2:] - X[1:-1], X[1:-1] - X[:-2]
    em, e0, ep = E[:-2], E[1:-1], E[2:]
    up, dn = np.abs(ep - e0), np.abs(em - e0)
    hi, lo = np.maximum(up, dn), np.minimum(up, dn)
    rising, falling = (ep > e0) & (e0 > em), (ep < e0) & (e0 < em)
    wp = np.where(rising, 1.0, np.where(falling, 0.0, np.where(ep > em, hi, lo)))
    wm = np.where(rising, 0.0, np.where(falling, 1.0, np.where(ep > em, lo, hi)))
    t = tmp[1:-1]
    np.multiply(dp, wp[:, None], out=t)
    t += dm * wm[:, None]
    tt = np.einsum("ij,ij->i", t, t)
    t *= np.where(tt > 0.0, 1.0 / np.sqrt(np.where(tt > 0.0, tt, 1.0)), 0.0)[:, None]
    ftau = np.einsum("ij,ij->i", F[1:-1], t)
    along = k * (np.sqrt(np.einsum("ij,ij->i", dp, dp)) - np.sqrt(np.einsum("ij,ij->i", dm, dm))) - ftau
    along[int(np.argmax(e0))] = -2.0 * ftau[int(np.argmax(e0))]
    np.multiply(t, along[:, None], out=out[1:-1])
    out[1:-1] += F[1:-1]


class HostBand:
    """The band force and one FIRE over the whole band in NumPy around `Engine.step(view=True)`: what a caller
    does without `relax_set_band`."""

    def __init__(self, nn, images, skin, fire):
        self.eng = Engine(nn)
        self.eng.set_skin(skin)
        self.eng.set_frames(images)
        self.p = fire
        self.F = len(images)
        self.x0 = np.ascontiguousarray(np.concatenate([a.positions for a in images]))
        self.x, self.v = self.x0.copy(), np.zeros_like(self.x0)
        self.B, self.tmp = np.zeros_like(self.x0), np.zeros_like(self.x0)
        self.n_rebuilds = 0   # lists built inside `run`, as the device path counts them (the resets' are left out)
        self.steps = 0
        self.reset()

    def reset(self):
        """Back to the interpolated band (not timed)."""
        self.x[:] = self.x0
        self.v[:] = 0.0
        self.dt, self.a, self.npos, self.first = self.p["dt"], self.p["astart"], 0, True
        self.res = self.eng.step(self.x, WANT, view=True)
        self.eng.synchronize()

    def run(self, steps):
        F, p, step = self.F, self.p, self.eng.step
        x, v, B, tmp = self.x.reshape(F, -1), self.v.reshape(F, -1), self.B.reshape(F, -1), self.tmp.reshape(F, -1)
        self.steps = 0
        built = self.eng.list_stats()[0]
        for _ in range(steps):
            band_force(x, np.asarray(self.res["energy"]), np.asarray(self.res["forces"]).reshape(F, -1), K_SPRING, B, tmp)
            b = B.reshape(-1, 3)
            if np.einsum("ij,ij->i", b, b).max() < FMAX * FMAX:
                break
            if self.first:
                self.first = False
            else:
                vf, ff, vv = np.vdot(B, v), np.vdot(B, B), np.vdot(v, v)
                if vf > 0.0:
                    v *= 1.0 - self.a
                    np.multiply(B, self.a * np.sqrt(vv) / np.sqrt(ff), out=tmp)
                    v += tmp
                    if self.npos > p["nmin"]:
                        self.dt = min(self.dt * p["finc"], p["dtmax"])
                        self.a *= p["fa"]
                    self.npos += 1
                else:
                    v[:] = 0.0
                    self.a, self.npos = p["astart"], 0
                    self.dt *= p["fdec"]
            np.multiply(B, self.dt, out=tmp)
            v += tmp
            np.multiply(v, self.dt, out=tmp)
            norm = np.sqrt(np.vdot(tmp, tmp))
            if norm > p["maxstep"]:
                tmp *= p["maxstep"] / norm
            x += tmp
            self.res = step(self.x, WANT, view=True)
            self.steps += 1
        self.eng.synchronize()
        self.n_rebuilds += self.eng.list_stats()[0] - built

    def energies(self):
        return np.array(self.res["energy"], dtype=np.float64)

    def rebuilds(self):
        return self.n_rebuilds


class DeviceBand:
    """`band=True`: the device band; `band=False`: `relax_run` of the same batch as independent frames."""

    def __init__(self, nn, images, skin, fire, band=True):
        self.eng = Engine(nn)
        self.eng.set_skin(skin)
        self.eng.set_frames(images)
        self.fire, self.band = fire, band
        self.x0 = np.ascontiguousarray(np.concatenate([a.positions for a in images]))
        self.n_rebuilds = 0
        self.out = None
        self.steps = 0
        self.reset()

    def reset(self):
        """Back to the interpolated band (not timed)."""
        self.eng.update_positions(self.x0)
        self.eng.relax_init(**self.fire)
        if self.band:
            self.eng.relax_set_band(True, k=K_SPRING, climb=True)
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
    nn, images = workload(name)
    n_atoms = sum(len(a) for a in images)
    # The symmetry-function model has random weights and is no potential that holds a lattice (see
    # bench_md_device.workload): its steps are kept short. The work per step does not depend on the step length
    # while the list holds.
    fire = dict(FIRE, maxstep=0.002) if name == "sf8" else dict(FIRE)
    loops = {"device": DeviceBand(nn, images, skin, fire), "host": HostBand(nn, images, skin, fire),
             "relax_run": DeviceBand(nn, images, skin, fire, band=False)}
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
    row = dict(workload=name, n_images=len(images), n_atoms=n_atoms, steps_per_window=steps, windows=repeats,
               skin=skin, fmax=FMAX, fire=fire, k=K_SPRING, climb=True, energy_gap_eV=gap,
               same_energies=bool(gap <= 1e-9), every_window_took_all_steps=bool(all_steps))
    for key, loop in loops.items():
        r = np.array(rates[key])
        row[key] = dict(atom_steps_per_s=r.tolist(), median=float(np.median(r)), min=float(r.min()),
                        max=float(r.max()), list_builds=int(loop.rebuilds()),
                        us_per_step=float(n_atoms / np.median(r) * 1e6))
        loop.eng.close()
    row["band_minus_relax_us_per_step"] = row["device"]["us_per_step"] - row["relax_run"]["us_per_step"]
    row["device_over_host"] = row["device"]["median"] / row["host"]["median"]
    row["device_no_slower"] = bool(row["device"]["median"] >= row["host"]["median"])
    return row


def write_report(prefix, rows):
    with open(prefix + ".json", "w") as fp:
        json.dump(dict(script="scripts/bench_neb.py", rows=rows), fp, indent=1)
    lines = ["# Device-resident nudged elastic band against the host-driven one", "",
             "Written by `scripts/bench_neb.py`: atom-steps/s, median (min .. max) over the windows; the paths",
             "alternate window by window in one process. Improved-tangent band with k = 0.1 eV/A^2 and a climbing",
             f"image, FIRE with ASE's default parameters (sf8: `maxstep` 0.002), `fmax` = {FMAX:g} (every window starts",
             "from the interpolated band and takes all its steps). `builds` = neighbour lists built inside the windows",
             "of the path (warm-up window included, the untimed resets between windows not). Both endpoint images are evaluated at every step on both paths.", "",
             "| workload | images x atoms | steps x windows | device band | builds | host `step` + NumPy band | builds | device / host | energy gap, eV |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        def cell(d):
            return f"{d['median'] / 1e6:.2f} M ({d['min'] / 1e6:.2f} .. {d['max'] / 1e6:.2f})"
        lines.append(f"| {r['workload']} | {r['n_images']} x {r['n_atoms'] // r['n_images']} | "
                     f"{r['steps_per_window']} x {r['windows']} | {cell(r['device'])} | {r['device']['list_builds']} | "
                     f"{cell(r['host'])} | {r['host']['list_builds']} | {r['device_over_host']:.2f} | "
                     f"{r['energy_gap_eV']:.1e} |")
    missed = [r["workload"] for r in rows if not r["device_no_slower"]]
    lines += ["", "Condition (device no slower than host, margin 0): " +
              ("met on every workload." if not missed else "MISSED on " + ", ".join(missed) + ".")]
    short = [r["workload"] for r in rows if not r["every_window_took_all_steps"]]
    if short:
        lines += ["", "INVALID: a band converged inside a window on " + ", ".join(short) + "."]
    off = [r["workload"] for r in rows if not r["same_energies"]]
    lines += ["", "Both paths end at the same energies to 1e-9 eV per image: " +
              ("yes, on every workload." if not off else "NO on " + ", ".join(off) + " (gaps in the table).")]
    lines += ["", "## Beside a plain relaxation step", "",
              "`Engine.relax_run` of the same batch as independent frames, same windows: time per step from the median",
              "rate. The difference is what the two band launches add to a FIRE step, together with whatever the two",
              "trajectories' list builds differ by. Not a gate.", "",
              "| workload | images x atoms | `relax_run`, us / step | builds | band, us / step | builds | band - relax, us |",
              "|---|---|---|---|---|---|---|"]
    for r in rows:
        d, g = r["relax_run"], r["device"]
        lines.append(f"| {r['workload']} | {r['n_images']} x {r['n_atoms'] // r['n_images']} | {d['us_per_step']:.1f} | "
                     f"{d['list_builds']} | {g['us_per_step']:.1f} | {g['list_builds']} | "
                     f"{r['band_minus_relax_us_per_step']:+.1f} |")
    with open(prefix + ".md", "w") as fp:
        fp.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="sf8,eam8,eam16")
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
