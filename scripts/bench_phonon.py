#!/usr/bin/env python3
"""Times the harmonic-phonon path (`tensoralloy_amd.phonons`, csrc/ta_phonon.hip) on a uniform mesh and writes
profiles/phonon.md:

    n = 3    Ni zjw04 EAM, one-atom fcc primitive cell, 3 x 3 x 3 supercell
    n = 12   the same model, cubic four-atom cell, 2 x 2 x 2 supercell
    n = 48   the same model, a 2 x 2 x 1 block of cubic cells (16 atoms) as home cell, 1 x 1 x 2 supercell

Per workload, over a `--mesh`^3 shifted mesh (default 48): `frequencies` (dynamical matrices + solver + the copy
of the frequencies to the host), `frequencies` with eigenvectors, `dos` (total and partial; nothing but the
histogram leaves the device), the solver alone on as many caller matrices (`Engine.phonon_eigh`, upload
included), and the same work in NumPy on this host: the restatement's D(q) vectorised over q, then
`numpy.linalg.eigvalsh` on the stacked matrices (on `--numpy-q` q-points, scaled). The kernel split is read from
the differences: solver alone against `frequencies`, `dos` against `frequencies`. Also the measured accuracy
margins of tests/test_gpu_phonons.py, and `--step-loop`: an `Engine.step` loop on bench.py's frame, which this
feature does not touch, as windows of `--steps` steps (run it with the parent commit's checkout too).

    python scripts/bench_phonon.py --out profiles/phonon.md
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402


def workloads():
    from tensoralloy_amd import Atoms
    a = 3.52
    prim = Atoms(symbols=["Ni"], positions=[[0.0, 0.0, 0.0]],
                 cell=np.array([[0, a / 2, a / 2], [a / 2, 0, a / 2], [a / 2, a / 2, 0]]), pbc=True)
    cubic = Atoms(symbols=["Ni"] * 4, positions=np.array([[0, 0, 0], [.5, .5, 0], [.5, 0, .5], [0, .5, .5]]) * a,
                  cell=np.eye(3) * a, pbc=True)
    return [(3, prim, (3, 3, 3)), (12, cubic, (2, 2, 2)), (48, cubic.repeat((2, 2, 1)), (1, 1, 2))]


def timed(fn, repeats):
    fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), float(min(t)), float(max(t))


def numpy_frequencies(ph, q_cart):
    """D(q) of the definition, vectorised over q, and eigvalsh of the stack."""
    nb, N = ph.force_constants.shape[:2]
    n = 3 * nb
    D = np.zeros((len(q_cart), n, n), dtype=complex)
    inv = 1.0 / np.sqrt(ph.masses)
    for b in range(nb):
        for s in range(N):
            v = ph.vectors[ph.start[b * N + s]:ph.start[b * N + s + 1]]
            phase = np.exp(1j * (q_cart @ v.T)).sum(axis=1) / len(v)
            bp = ph.basis_of[s]
            D[:, 3 * b:3 * b + 3, 3 * bp:3 * bp + 3] += phase[:, None, None] * (ph.force_constants[b, s] * inv[b] * inv[bp])
    lam = np.linalg.eigvalsh(0.5 * (D + D.conj().transpose(0, 2, 1)))
    return np.sign(lam) * np.sqrt(np.abs(lam))


def step_loop(windows, steps):
    import bench
    from tensoralloy_amd import Engine, _lib
    nn, atoms = bench.ni_model(), bench.ni_frame(611)
    want = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES | _lib.TA_WANT_VIRIAL
    out = []
    with Engine(nn) as eng:
        eng.set_frames([atoms])
        pos = atoms.positions.copy()
        for _ in range(20):
            eng.step(pos, want)
        for _ in range(windows):
            t0 = time.perf_counter()
            for _ in range(steps):
                eng.step(pos, want)
            out.append((time.perf_counter() - t0) / steps * 1e6)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", type=int, default=48)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--numpy-q", type=int, default=4096)
    ap.add_argument("--bins", type=int, default=200)
    ap.add_argument("--out", default="")
    ap.add_argument("--step-loop", action="store_true", help="only the Engine.step windows, one line")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    if args.step_loop:
        w = step_loop(args.windows, args.steps)
        print("step_loop_us " + " ".join(f"{x:.1f}" for x in w) + f"  median {np.median(w):.1f}")
        return
    from tests import phonon_reference as R
    from tests.helpers import make_eam
    from tensoralloy_amd import Engine
    from tensoralloy_amd.phonons import Phonons, mesh_points
    q_red = mesh_points(args.mesh, args.mesh, args.mesh, shift=True)
    Q = len(q_red)
    rows = []
    with Engine(make_eam(["Ni"], 6.0)) as eng:
        for n, home, reps in workloads():
            ph = Phonons(eng, home, supercell=reps)
            q_cart = ph.q_cartesian(q_red)
            nu = ph.frequencies(q_red)
            hi = float(nu.max()) * 1.05
            t_f = timed(lambda: ph.frequencies(q_red), args.repeats)
            q_v = q_red[:min(Q, max(1, (512 << 20) // (n * n * 16)))]   # (the modes of all q would not fit the host)
            t_v = timed(lambda: ph.frequencies(q_v, eigenvectors=True), args.repeats)
            t_v = tuple(x * Q / len(q_v) for x in t_v)
            t_d = timed(lambda: ph.dos(q_red, args.bins, (0.0, hi)), args.repeats)
            t_p = timed(lambda: ph.dos(q_red, args.bins, (0.0, hi), partial=True), args.repeats)
            rng = np.random.RandomState(n)
            m_q = min(Q, max(1, (256 << 20) // (n * n * 16)))
            X = rng.normal(size=(m_q, n, n)) + 1j * rng.normal(size=(m_q, n, n))
            t_e = timed(lambda: eng.phonon_eigh(X, eigenvectors=False), args.repeats)
            k = min(Q, args.numpy_q)
            t0 = time.perf_counter()
            ref = numpy_frequencies(ph, q_cart[:k])
            t_np = time.perf_counter() - t0
            err = np.abs(nu[:k] / R.THZ - ref).max()
            rows.append(dict(n=n, N=len(ph.super_atoms), f=t_f, v=t_v, d=t_d, p=t_p, e=(t_e[0] / m_q, m_q),
                             np_us=t_np / k * 1e6, err=err, numax=float(nu.max())))
            print(rows[-1], flush=True)
    ref_set = R.mp_reference_set()
    r_np = R.numpy_margin(ref_set)
    r_dev = 0.0
    with Engine(make_eam(["Ni"], 6.0)) as eng:
        for nn_, kind, A, w_mp in ref_set:
            w, _, info = eng.phonon_eigh(A)
            u = R.unit_of(A)
            ok = u > 0
            if ok.any():
                r_dev = max(r_dev, float((np.abs(w - w_mp).max(axis=1)[ok] / u[ok]).max()))
    us = lambda t: t[0] / Q * 1e6  # noqa: E731
    lines = ["# Harmonic phonons on the device: timing and accuracy", "",
             f"`python scripts/bench_phonon.py --mesh {args.mesh}`: a shifted {args.mesh}^3 mesh, Q = {Q} q-points, "
             f"Ni zjw04 EAM (rc = 6 A), median of {args.repeats} calls after one warm-up call, wall time of the Python "
             "call (uploads of q, chunking and the copies out included). NumPy: the same D(q) vectorised over q and "
             f"`eigvalsh` on the stacked matrices, on the first {min(Q, args.numpy_q)} q-points of the mesh, same host.", "",
             "| n | supercell atoms | frequencies us/q | + eigenvectors us/q | dos (total) us/q | dos (partial) us/q | "
             "solver alone us/matrix | NumPy us/q | NumPy / device | max abs(d sqrt(lambda)) vs NumPy |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['n']} | {r['N']} | {us(r['f']):.3f} | {us(r['v']):.3f} | {us(r['d']):.3f} | {us(r['p']):.3f} | "
                     f"{r['e'][0] * 1e6:.3f} ({r['e'][1]} matrices) | {r['np_us']:.2f} | {r['np_us'] / us(r['f']):.0f}x | "
                     f"{r['err']:.1e} |")
    lines += ["", "Kernel split, from the differences: `dos (total)` runs the dynamical-matrix kernel and the solver "
              "without eigenvectors and copies nothing but the histogram out, so `frequencies - dos` is about the "
              "copy of the frequencies; the solver alone includes the upload of its matrices (16 n^2 bytes each), which "
              "`frequencies` does not have; what `frequencies` takes beyond the solver is the phase sums.", "",
              "## Accuracy margins (tests/test_gpu_phonons.py)", "",
              "Unit u = n eps ||A||_F per matrix, on the matrices of order <= 12 with an mpmath reference at 50 digits:", "",
              f"- `numpy.linalg.eigvalsh` against mpmath: {r_np:.3f} u",
              f"- the device solver against mpmath: {r_dev:.3f} u",
              f"- the tests allow the device 4 x max({r_np:.3f}, 1) = {4 * max(r_np, 1.0):.3f} u.", ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(text)


if __name__ == "__main__":
    main()
