#!/usr/bin/env python3
"""Phase timeline of the angular kernels and of the MLP tile kernel from a -DTA_PHASE_STAMPS run
(scripts/build_stamps_lib.sh): per kernel, the mean / median / max over the workgroups of the time between
consecutive stamps, and of each stamp relative to the kernel's first stamp (s_memrealtime ticks of 10 ns).
The MLP tile kernel (rows "2 ...") stamps entry, rows staged, every forward GEMM phase, energies emitted,
every backward GEMM phase and dE/dG stored: as many slots as its body has phases, the rest left zero."""
import sys
import numpy as np

names = {0: ["entry", "staged", "masks", "jobs built", "list written", "sweep done", "assembled"],
         1: ["entry", "staged", "job words", "sweep done", "barrier", "epilogue done"]}
rows = {0: [], 1: []}
for line in open(sys.argv[1]):
    p = line.split()
    k, v = int(p[0]), np.array([int(x) for x in p[2:]], dtype=np.int64)
    if k in rows and v[0] and v[1]:
        rows[k].append(v)
for k in (0, 1):
    if not rows[k]:
        continue
    a = np.array(rows[k])
    n = len(names[k])
    if a.shape[1] >= 10 and (a[:, 8] > 0).all():
        # slots 8 / 9: the wavefront's first instruction (in front of every argument load) and the arrival
        # of the run header; "entry" is the stamp in front of the staging loop
        h = a[(a[:, 9] > 0) & (a[:, 0] > 0)]
        for label, d in (("wave start -> header arrived", (h[:, 9] - h[:, 8]) / 100.0),
                         ("header arrived -> entry", (h[:, 0] - h[:, 9]) / 100.0)):
            print(f"kernel {'forward' if k == 0 else 'backward'}: {label:<28s} mean {d.mean():6.2f}  "
                  f"median {np.median(d):6.2f}  max {d.max():6.2f} us")
        print(f"kernel {'forward' if k == 0 else 'backward'}: first wave start -> last end "
              f"{(a[:, n - 1].max() - a[:, 8].min()) / 100:.1f} us")
    a = a[:, :n]
    ok = (a > 0).all(axis=1)
    a = a[ok]
    t0 = a[:, 0].min()
    print(f"kernel {'forward' if k == 0 else 'backward'}: {len(a)} workgroups; first entry -> last end "
          f"{(a[:, n - 1].max() - t0) / 100:.1f} us; entry spread {(a[:, 0].max() - t0) / 100:.1f} us")
    for q in range(1, n):
        d = (a[:, q] - a[:, q - 1]) / 100.0
        rel = (a[:, q] - t0) / 100.0
        print(f"  {names[k][q - 1]:>14s} -> {names[k][q]:<14s} mean {d.mean():6.2f}  median {np.median(d):6.2f}  "
              f"max {d.max():6.2f} us | reached at mean {rel.mean():6.2f}  max {rel.max():6.2f} us")

mlp = []
for line in open(sys.argv[1]):
    p = line.split()
    if p[0] == "2":
        mlp.append([int(x) for x in p[2:]])
if mlp:
    a = np.array(mlp, dtype=np.int64)
    n = int((a > 0).all(axis=0).sum())          # slots every workgroup stamped
    a = a[:, :n]
    t0 = a[:, 0].min()
    print(f"kernel mlp tile: {len(a)} workgroups, {n} stamps; first entry -> last end "
          f"{(a[:, n - 1].max() - t0) / 100:.1f} us; entry spread {(a[:, 0].max() - t0) / 100:.1f} us; "
          f"entry -> end median {np.median(a[:, n - 1] - a[:, 0]) / 100:.2f} us")
    for q in range(1, n):
        d = (a[:, q] - a[:, q - 1]) / 100.0
        print(f"  stamp {q - 1} -> {q}: mean {d.mean():6.2f}  median {np.median(d):6.2f}  max {d.max():6.2f} us")
