#!/usr/bin/env python3
"""
Generates tests/golden/Mendelev_Al_Fe_thinned.fs.eam.gz from the reference mounted at
/root/reference. Run in the BUILD container only (the reference never travels to the GPU box):
`python tests/golden/make_golden_fs.py`.

The source is the LAMMPS eam/fs data file the reference's own tests read
(test_files/lammps/Mendelev_Al_Fe.fs.eam: Mendelev et al.'s Al-Fe potential, nr = nrho = 10000).
It gzips to 776 KB; the fixture keeps every 5th knot of both the r and the rho tables
(nr = nrho = 2000, dr = 0.00325 A, drho = 0.15), values copied verbatim, in the same layout:
per element a header line, F(rho), then N density tables; then the r * phi(r) tables in
(1,1), (2,1), (2,2) order. Data only: no reference source text is stored.
"""
import gzip
import os

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
K = 5


def main():
    with open(f"{REF}/test_files/lammps/Mendelev_Al_Fe.fs.eam") as fp:
        lines = fp.read().replace("\r", "").split("\n")
    head = lines[3].split()
    n_el = int(head[0])
    v = lines[4].split()
    nrho, drho, nr, dr, rcut = int(v[0]), float(v[1]), int(v[2]), float(v[3]), v[4]
    if nr % K or nrho % K:
        raise RuntimeError("table lengths are not multiples of the thinning step")
    tok = " ".join(lines[5:]).split()
    pos = 0

    def take(n):
        nonlocal pos
        out = tok[pos:pos + n]
        if len(out) != n:
            raise RuntimeError("file ends inside a table")
        pos += n
        return out

    out = [lines[0] + "\n", lines[1] + "\n",
           f"thinned to every {K}th knot of the r and rho tables by tests/golden/make_golden_fs.py\n",
           lines[3] + "\n", f"{nrho // K} {drho * K!r} {nr // K} {dr * K!r} {rcut}\n"]
    for _ in range(n_el):
        out.append(" ".join(take(4)) + "\n")
        out += [x + "\n" for x in take(nrho)[::K]]
        for _ in range(n_el):
            out += [x + "\n" for x in take(nr)[::K]]
    for _ in range(n_el * (n_el + 1) // 2):
        out += [x + "\n" for x in take(nr)[::K]]
    if pos != len(tok):
        raise RuntimeError(f"{len(tok) - pos} tokens left over")
    with gzip.GzipFile(os.path.join(HERE, "Mendelev_Al_Fe_thinned.fs.eam.gz"), "wb", compresslevel=9,
                       mtime=0) as fo:
        fo.write("".join(out).encode())


if __name__ == "__main__":
    main()
