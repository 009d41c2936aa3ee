"""
The per-workgroup block header of the second-generation angular kernels (`BlockHeader`, ta_device.h), path by
path, against the C oracle.

Every producer of the run packing also writes one 64-byte header per run slot (first centre, number of
centres, first pair, number of pairs, every centre's first pair, the `one_pass` decision), and the forward and
backward kernels take all of that from the header and from a table in LDS instead of walking blk_center ->
pair_start -> pair_i -> pair_start / pair_stop. The inputs below are the smallest that reach each path:

  ni108     108-atom jittered fcc Ni, rcut = acut = 4.5: three or four centres per workgroup, two in the last
  batch3    5 + 32 + 108 atoms in three DIFFERENT triclinic cells: a workgroup straddles a frame boundary and
            must take each centre's own cell
  wide      a bcc slab whose inner atoms have more than 128 neighbours (n / 2 > 64: not `one_pass`) plus one
            atom with no neighbour at all, rcut = 6.5, acut = 4.0
  strided   a 54-atom bcc cell, a = 2.0, rcut = 6.5: more than 256 neighbours, M > workgroup size
  md        set_skin(0.5), set_frames, two `step` calls with every atom moved by up to 0.1 A: the device packer
            (filter_group_kernel) writes the headers, unused run slots included
  nimo64    a 64-atom Ni-Mo frame: the two-element builds and an MLP atom map that is not the identity

Each case asks for energy, forces and virial and runs with the triangle-once backward pass on and off. Bounds
are those of test_gpu_sf_dispatch.py: descriptors to 1e-10, energies and forces to 1e-9 x max(1, |.|), virial
to 1e-8 x max(1, |.|).
"""
import functools

import numpy as np
import pytest

from tests.helpers import fcc, make_nn, oracle_model
from tensoralloy_amd import Atoms

gpu = pytest.mark.gpu

G_TOL = 1e-10
E_REL, F_REL, W_REL = 1e-9, 1e-9, 1e-8


def sheared(atoms, shear):
    """`atoms` in a triclinic cell: cell and positions times (1 + shear)."""
    T = np.eye(3) + np.asarray(shear, dtype=float)
    return Atoms(symbols=atoms.get_chemical_symbols(), positions=atoms.positions @ T,
                 cell=np.asarray(atoms.get_cell()) @ T, pbc=True)


def bcc(a, rep, seed, jitter=0.03, vacuum=0.0, extra=None):
    """bcc Ni block, periodic; `vacuum` lengthens the cell along z, `extra` adds atoms at given positions."""
    base = np.array([[0, 0, 0], [.5, .5, .5]]) * a
    pts = np.array([base + np.array([x, y, z]) * a
                    for x in range(rep[0]) for y in range(rep[1]) for z in range(rep[2])]).reshape(-1, 3)
    pts = pts + np.random.RandomState(seed).normal(0.0, jitter, pts.shape)
    if extra is not None:
        pts = np.concatenate([pts, np.asarray(extra, dtype=float).reshape(-1, 3)])
    return Atoms(symbols=["Ni"] * len(pts), positions=pts,
                 cell=np.diag([a * rep[0], a * rep[1], a * rep[2] + vacuum]), pbc=True)


def neighbour_counts(atoms, rc):
    from oracle.neighbors import neighbor_list
    i, _, _ = neighbor_list(atoms.positions, np.asarray(atoms.get_cell(complete=True)), atoms.pbc, rc)
    return np.bincount(i, minlength=len(atoms))


def ni108():
    # a = 3.18: the fourth shell sits at the cutoff, so the counts vary (45 .. 51) and the runs hold 3 or 4 centres
    return fcc(rep=(3, 3, 3), a=3.18, seed=7)


def nimo64():
    atoms = fcc(rep=(4, 2, 2), a=3.6, seed=9)
    syms = ["Ni", "Mo"] * (len(atoms) // 2)
    np.random.RandomState(9).shuffle(syms)
    return Atoms(symbols=syms, positions=atoms.positions, cell=np.asarray(atoms.get_cell()), pbc=True)


@functools.lru_cache(maxsize=None)
def case(name):
    """(model, frames) of a static case; made once, shared by the triangle and the per-apex run."""
    if name == "ni108":
        return make_nn(["Ni"], 4.5, True, [16, 16]), (ni108(),)
    if name == "batch3":
        five = fcc(rep=(2, 1, 1), seed=1)
        five = Atoms(symbols=["Ni"] * 5, positions=five.positions[:5], cell=np.asarray(five.get_cell()), pbc=True)
        frames = (sheared(five, [[0, 0, 0], [0.15, 0, 0], [0.05, -0.1, 0]]),
                  sheared(fcc(rep=(2, 2, 2), seed=2), [[0, 0.08, 0], [0, 0, 0.12], [-0.1, 0, 0]]),
                  sheared(fcc(rep=(3, 3, 3), seed=3), [[0, 0, 0.06], [-0.07, 0, 0], [0, 0.09, 0]]))
        return make_nn(["Ni"], 4.5, True, [16, 16]), frames
    if name == "wide":
        # 3 x 3 x 4 bcc cells (72 atoms) as a slab periodic in x and y, and one atom 15 A above it
        slab = bcc(2.4, (3, 3, 4), seed=4, vacuum=30.4, extra=[[3.0, 3.0, 25.0]])
        return make_nn(["Ni"], 6.5, True, [16, 16], acut=4.0), (slab,)
    if name == "strided":
        return make_nn(["Ni"], 6.5, True, [16, 16]), (bcc(2.0, (3, 3, 3), seed=5),)
    if name == "nimo64":
        return make_nn(["Ni", "Mo"], 4.5, True, [16, 16]), (nimo64(),)
    raise KeyError(name)


def c_oracle(nn, atoms):
    from bench import host_cores
    from oracle import csf
    m = oracle_model(nn)
    return csf.run(m, csf.prepare(m, atoms.get_chemical_symbols(), atoms.positions,
                                  np.asarray(atoms.get_cell(complete=True)), atoms.pbc), True, host_cores())


@functools.lru_cache(maxsize=None)
def reference(name):
    nn, frames = case(name)
    return tuple(c_oracle(nn, a) for a in frames)


def check(r, o, tag, descriptors=True):
    dev = dict(E=abs(r["energy"] - o["energy"]), e=np.abs(r["atomic"] - o["atomic"]).max(initial=0.0),
               F=np.abs(r["forces"] - o["forces"]).max(initial=0.0), W=np.abs(r["virial"] - o["virial"]).max())
    if descriptors:
        dev["G"] = np.abs(r["descriptors"] - o["descriptors"]).max(initial=0.0)
    print(f"DEV {tag} " + " ".join(f"{k}={v:.2e}" for k, v in dev.items()))
    e_scale = max(1.0, abs(o["energy"]))
    assert dev["E"] < E_REL * e_scale, (tag, dev)
    assert dev["e"] < E_REL * e_scale, (tag, dev)
    assert dev["F"] < F_REL * max(1.0, np.abs(o["forces"]).max(initial=0.0)), (tag, dev)
    assert dev["W"] < W_REL * max(1.0, np.abs(o["virial"]).max()), (tag, dev)
    if descriptors:
        assert dev["G"] < G_TOL, (tag, dev)


def runs_of(counts, cap=192, max_centres=16):
    """The run packing of ta_set_frames: whole centres, <= cap pairs and <= 16 centres per run."""
    runs, load, nc = [0], 0, 0
    for i, n in enumerate(counts):
        if load + n > cap or nc >= max_centres:
            runs.append(i)
            load = nc = 0
        load += n
        nc += 1
    return runs + [len(counts)]


def test_inputs_reach_their_paths():
    """CPU: the neighbour counts that send each case down the path it is named after."""
    n = neighbour_counts(case("ni108")[1][0], 4.5)
    runs = runs_of(n)
    sizes = np.diff(runs)
    assert n.max() <= 64 and sizes.max() >= 2 and sizes[-1] < sizes.max(), sizes   # last workgroup partial
    frames = case("batch3")[1]
    assert [len(a) for a in frames] == [5, 32, 108]
    runs = runs_of(np.concatenate([neighbour_counts(a, 4.5) for a in frames]))
    assert any(lo < edge < hi for lo, hi in zip(runs[:-1], runs[1:]) for edge in (5, 37)), runs   # a run straddles frames
    cells = [np.asarray(a.get_cell()) for a in frames]
    assert all(abs(c - np.diag(np.diag(c))).max() > 0.1 for c in cells)                       # triclinic
    n = neighbour_counts(case("wide")[1][0], 6.5)
    assert n.min() == 0 and 128 < n.max() <= 192, (n.min(), n.max())
    n = neighbour_counts(case("strided")[1][0], 6.5)
    assert n.max() > 256, n.max()
    assert set(case("nimo64")[1][0].get_chemical_symbols()) == {"Ni", "Mo"} and len(case("nimo64")[1][0]) == 64


@gpu
@pytest.mark.parametrize("triangles", [True, False], ids=["triangles", "per-apex"])
@pytest.mark.parametrize("name", ["ni108", "batch3", "wide", "strided", "nimo64"])
def test_header_paths(lib, name, triangles):
    from tensoralloy_amd import Engine
    nn, frames = case(name)
    with Engine(nn) as eng:
        eng.set_triangles(triangles)
        res = eng.evaluate(list(frames), descriptors=True)
        variant = eng.backward_variant()
    if name == "ni108":   # the one-element default grid in a cell wider than the cutoff: the build asked for
        assert variant == (2 if triangles else 1), variant
    for k, (r, o) in enumerate(zip(res, reference(name))):
        check(r, o, f"{name}/{'tri' if triangles else 'apex'}/frame{k}")


@gpu
@pytest.mark.parametrize("triangles", [True, False], ids=["triangles", "per-apex"])
def test_header_of_the_device_packer(lib, triangles):
    """The MD packing path: the exact list of every step, its run slots (unused ones included) and their headers
    are made on the device from the skin list; each step against the oracle at the moved positions."""
    from tensoralloy_amd import Engine, _lib
    nn, (atoms,) = case("ni108")
    want = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES | _lib.TA_WANT_VIRIAL | _lib.TA_WANT_ATOMIC
    rng = np.random.RandomState(11)
    pos = atoms.positions.copy()
    with Engine(nn) as eng:
        eng.set_triangles(triangles)
        eng.set_skin(0.5)
        eng.set_frames([atoms])
        for step in range(2):
            pos = pos + rng.uniform(-0.1, 0.1, pos.shape) / np.sqrt(3.0)   # every atom by up to 0.1 A
            got = {k: np.array(v) for k, v in eng.step(pos, want).items()}
            moved = Atoms(symbols=atoms.get_chemical_symbols(), positions=pos, cell=np.asarray(atoms.get_cell()),
                          pbc=True)
            r = dict(energy=got["energy"][0], atomic=got["atomic"], forces=got["forces"], virial=got["virial"][0])
            check(r, c_oracle(nn, moved), f"md/{'tri' if triangles else 'apex'}/step{step}", descriptors=False)
        builds, reuses = eng.list_stats()
        assert builds == 1 and reuses == 2, (builds, reuses)
