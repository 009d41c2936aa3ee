"""
The triangle-once angular backward pass (ta_kernels_v2.hip: `backward_v2_kernel<.., TRI = true>`), against the
C oracle and against the per-apex pass on the same handle.

A triangle {i, j, k} with all three sides below acut adds a G4 term at each of its three apexes. One-element
models with the default zeta grid evaluate the three terms in the backward pass once, at the owner of the
triangle (`owns_triangle`, ta_device.h), when every periodic cell width exceeds max(rcut, acut); the host
dispatcher keeps the per-apex pass otherwise. `Engine.backward_variant()` tells which one ran (bit 0 per apex,
bit 1 triangles).

Bounds as in tests/test_gpu_sf_dispatch.py (descriptors 1e-10; energies, forces, virial 1e-9 / 1e-9 / 1e-8
relative), and the two passes agree to 1e-12 relative in forces (same terms, other summation order).
"""
import numpy as np
import pytest

from bench import ni_frame, ni_model
from tests.helpers import fcc, make_nn
from tests.test_gpu_sf_dispatch import c_oracle, check, drop

gpu = pytest.mark.gpu
PER_APEX, TRIANGLES = 1, 2


def host_triples(atoms, rc):
    """Every contributing triple (centre, neighbour a, neighbour b), all three sides below rc, from the
    oracle's neighbour list (pairs {a, b} of a centre unordered)."""
    from oracle.neighbors import neighbor_list
    R, h = atoms.positions, np.asarray(atoms.get_cell(complete=True))
    i, j, S = neighbor_list(R, h, atoms.pbc, rc)
    D = R[j] - R[i] + S @ h
    r2 = np.sum(D * D, axis=1) + 1e-14
    order = np.argsort(i, kind="stable")
    i, j, D, r2 = i[order], j[order], D[order], r2[order]
    start = np.searchsorted(i, np.arange(len(R) + 1))
    out = []
    for c in range(len(R)):
        sel = np.arange(start[c], start[c + 1])
        sel = sel[r2[sel] < rc * rc]
        ta, tb = np.triu_indices(len(sel), 1)
        E = D[sel][tb] - D[sel][ta]
        ok = np.sum(E * E, axis=1) + 1e-14 < rc * rc
        out.append(np.stack([np.full(ok.sum(), c), j[sel][ta[ok]], j[sel][tb[ok]]], axis=1))
    return np.concatenate(out).astype(np.int32)


def owners(lib, abc):
    abc = np.ascontiguousarray(abc, dtype=np.int32)
    own = np.empty(len(abc), dtype=np.int32)
    from tensoralloy_amd import _lib
    assert lib.ta_triangle_owner(len(abc), _lib.as_ip(abc), _lib.as_ip(own)) == 0
    return own


def test_owner_rule_on_the_host(lib):
    """CPU: the host restatement of the ownership rule on the benchmark frame: every triangle is seen from its
    three vertices and exactly one of them owns it, the owner does not depend on the order of the atoms, and
    every centre owns about a third of its triangles."""
    atoms = ni_frame(0)
    T = host_triples(atoms, 6.5)
    own = owners(lib, T)
    assert (own >= 0).all()
    assert np.array_equal(own, owners(lib, T[:, [2, 0, 1]])) and np.array_equal(own, owners(lib, T[:, [1, 2, 0]]))
    N = len(atoms)
    key = np.sort(T, axis=1).astype(np.int64)
    key = (key[:, 0] * N + key[:, 1]) * N + key[:, 2]
    mine = own == T[:, 0]
    uniq, count = np.unique(key, return_counts=True)
    assert (count == 3).all()                                     # the cell is wider than 2 acut: one triangle per key
    assert np.array_equal(np.unique(key[mine]), uniq) and mine.sum() == len(uniq)   # one owner each
    frac = np.bincount(T[mine, 0], minlength=N) / np.bincount(T[:, 0], minlength=N)
    print(f"owned fraction per centre: mean {frac.mean():.4f} min {frac.min():.4f} max {frac.max():.4f}")
    assert abs(frac.mean() - 1 / 3) < 0.005
    assert np.abs(frac - 1 / 3).max() < 0.06
    assert (owners(lib, np.array([[3, 3, 5], [7, 2, 7]])) == -1).all()


def run(nn, frames, triangles=True, skin=None):
    from tensoralloy_amd import Engine
    with Engine(nn) as eng:
        eng.set_triangles(triangles)
        res = eng.evaluate(frames, descriptors=True)
        variant = eng.backward_variant()
        owned, contributing = eng.count_owned_triangles(), eng.count_contributing_triples()
    return res, variant, owned, contributing


def check_frames(nn, frames, res, tag):
    for k, (atoms, r) in enumerate(zip(frames, res)):
        check(r, c_oracle(nn, atoms), f"{tag}/frame{k}")


def same_forces(a, b, tag):
    for k, (x, y) in enumerate(zip(a, b)):
        scale = max(1.0, np.abs(y["forces"]).max())
        dF = np.abs(x["forces"] - y["forces"]).max()
        dW = np.abs(x["virial"] - y["virial"]).max()
        print(f"TRI-vs-APEX {tag}/frame{k} dF={dF:.2e} dW={dW:.2e}")
        assert dF <= 1e-12 * scale, (tag, k, dF)
        assert dW <= 1e-12 * max(1.0, np.abs(y["virial"]).max()), (tag, k, dW)
        assert abs(x["energy"] - y["energy"]) <= 1e-12 * max(1.0, abs(y["energy"])), (tag, k)


@gpu
def test_benchmark_frame(lib):
    """The 4000-atom Ni frame of bench.py: triangle pass against the oracle and against the per-apex pass on
    the same handle; 3 x owned triangles = contributing triples, and the device owns what the host rule says."""
    from tensoralloy_amd import Engine
    nn, atoms = ni_model(), ni_frame(0)
    with Engine(nn) as eng:
        tri = eng.evaluate([atoms], descriptors=True)
        assert eng.backward_variant() == TRIANGLES
        eng.set_triangles(False)
        apex = eng.evaluate([atoms], descriptors=True)
        assert eng.backward_variant() == PER_APEX
        eng.set_triangles(True)
        again = eng.evaluate([atoms], descriptors=True)
        assert eng.backward_variant() == TRIANGLES
        owned, contributing = eng.count_owned_triangles(), eng.count_contributing_triples()
    T = host_triples(atoms, 6.5)
    assert 3 * owned == contributing == len(T), (owned, contributing, len(T))
    assert owned == int((owners(lib, T) == T[:, 0]).sum())
    check_frames(nn, [atoms], tri, "bench-frame")
    same_forces(tri, apex, "bench-frame")
    same_forces(again, tri, "bench-frame-again")   # LDS atomics: the order of the sums varies between runs


@gpu
def test_batch_straddling_runs(lib):
    """Uneven frames in one batch: angular workgroups (runs of up to 16 centres) straddle frame boundaries.
    The 2 x 2 x 2 cells are 7.05 A wide, between acut and 2 acut: an atom has two images within acut of a
    centre, which the ownership rule admits (they are never in one triangle)."""
    nn = make_nn(["Ni"], 6.5, True, [16, 16])
    frames = [drop(fcc(rep=(2, 2, 2), seed=31), 3), drop(fcc(rep=(2, 2, 3), seed=32), 5), fcc(rep=(3, 2, 2), seed=33)]
    res, variant, owned, contributing = run(nn, frames)
    assert variant == TRIANGLES and 3 * owned == contributing, (variant, owned, contributing)
    check_frames(nn, frames, res, "straddle")
    apex, variant, _, _ = run(nn, frames, triangles=False)
    assert variant == PER_APEX
    same_forces(res, apex, "straddle")


@gpu
def test_thin_cell_falls_back(lib):
    """A cell thinner than max(rcut, acut) along one axis: triangles could hold two images of one atom, so the
    per-apex pass runs."""
    nn = make_nn(["Ni"], 6.5, True, [16, 16])
    frames = [fcc(rep=(1, 3, 3), seed=41)]
    res, variant, owned, contributing = run(nn, frames)
    assert variant == PER_APEX, variant
    check_frames(nn, frames, res, "thin")


@gpu
def test_no_job_list_path(lib):
    """More than 128 neighbours per centre (rc = 8.6, cap 256): the forward kernel makes no job list and the
    triangle build tests ownership per triple; also the <.., 12, true, 0> triangle build."""
    nn = make_nn(["Ni"], 8.6, True, [16], sf_kwargs=dict(eta=[0.05, 4.0, 20.0], beta=[0.005], gamma=[1.0, -1.0],
                                                          zeta=[1.0, 4.0]))
    frames = [fcc(rep=(3, 3, 3), seed=43)]
    res, variant, owned, contributing = run(nn, frames)
    assert variant == TRIANGLES and 3 * owned == contributing, (variant, owned, contributing)
    check_frames(nn, frames, res, "no-list")
    apex, _, _, _ = run(nn, frames, triangles=False)
    same_forces(res, apex, "no-list")


@gpu
def test_md_path(lib):
    """The MD path (exact list filtered on the device from a skin list, ta_step_view): its pair slots are
    not the fresh list's; several steps with list reuse and a rebuild, each against the oracle."""
    from tensoralloy_amd import Atoms, Engine, _lib
    want = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES | _lib.TA_WANT_VIRIAL | _lib.TA_WANT_ATOMIC
    nn = make_nn(["Ni"], 6.5, True, [16, 16])
    frames = [drop(fcc(rep=(3, 2, 2), seed=51), 3), fcc(rep=(2, 3, 3), seed=52)]
    sizes = np.cumsum([0] + [len(a) for a in frames])
    rng = np.random.RandomState(7)
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        eng.set_frames(frames)
        pos = np.concatenate([a.positions for a in frames])
        for step in range(4):
            pos = pos + rng.normal(0, 0.2 if step == 2 else 0.02, pos.shape)
            got = {k: np.array(v) for k, v in eng.step(pos, want, view=True).items()}
            assert eng.backward_variant() == TRIANGLES
            for f, atoms in enumerate(frames):
                moved = Atoms(symbols=atoms.get_chemical_symbols(), positions=pos[sizes[f]:sizes[f + 1]],
                              cell=np.asarray(atoms.get_cell()), pbc=True)
                r = dict(energy=got["energy"][f], atomic=got["atomic"][sizes[f]:sizes[f + 1]],
                         forces=got["forces"][sizes[f]:sizes[f + 1]], virial=got["virial"][f])
                check(r, c_oracle(nn, moved), f"md/step{step}/frame{f}", descriptors=False)
        owned, contributing = eng.count_owned_triangles(), eng.count_contributing_triples()
        assert 3 * owned == contributing, (owned, contributing)
        builds, reuses = eng.list_stats()
        assert builds >= 2 and reuses >= 1, (builds, reuses)
