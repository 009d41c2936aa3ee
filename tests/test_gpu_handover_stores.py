"""
The stores with which the angular kernels hand data to the kernels behind them (ta_kernels_v2.hip): the pair
record of `stage()` goes out behind the item's LDS writes, and the forward kernel leaves out the full job list
when every backward launch of the evaluation takes the triangle build and reads the owned lists.

Every case is held to the CPU oracle with the bounds of the angular dispatch tests (descriptors 1e-10,
energies / forces / virial 1e-9 / 1e-9 / 1e-8 relative, `check` of test_gpu_sf_dispatch). Shapes are the
smallest at which each path is taken: 108-atom cells with one or two centres per workgroup, whose runs hold
numbers of pairs and of jobs that are no multiple of four.

The full list has a second reader: the per-apex kernel that `ta_hessian_vectors` and the direction terms of
`ta_loss_gradient` launch on the lists of an earlier forward pass. The handle knows whether that list is
there; `test_full_list_validity` alternates evaluations that skip it with calls that need it.
"""
import numpy as np
import pytest

from tests.helpers import fcc, make_nn
from tests.test_gpu_sf_dispatch import E_REL, F_REL, W_REL, alloy, c_oracle, check, drop

gpu = pytest.mark.gpu
PER_APEX, TRIANGLES = 1, 2          # ta_backward_variant, or-ed over the backward launches of an evaluation

_oracle_cache = {}


def oracle_of(key, nn, atoms):
    """One oracle evaluation per (model, frame) of this module."""
    if key not in _oracle_cache:
        _oracle_cache[key] = c_oracle(nn, atoms)
    return _oracle_cache[key]


def ni_model():
    return make_nn(["Ni"], 6.5, True, [16, 16])


def ni_frame():
    return fcc(rep=(3, 3, 3), seed=61)


def run_and_check(nn, frames, tag, triangles=None, expect=None):
    from tensoralloy_amd import Engine
    with Engine(nn) as eng:
        if triangles is not None:
            eng.set_triangles(triangles)
        res = eng.evaluate(frames, descriptors=True)
        variant = eng.backward_variant()
    if expect is not None:
        assert variant == expect, (tag, variant)
    for k, (atoms, r) in enumerate(zip(frames, res)):
        check(r, oracle_of((tag, k), nn, atoms), f"{tag}/frame{k}")
    return res


def test_shapes_have_ragged_tails():
    """CPU: the 108-atom frame's neighbour counts are not all multiples of four (16-byte tails of the lists),
    and every cell width exceeds the cutoff (the triangle pass is admitted)."""
    from oracle.neighbors import neighbor_list
    atoms = ni_frame()
    i, _, _ = neighbor_list(atoms.positions, np.asarray(atoms.get_cell()), atoms.pbc, 6.5)
    counts = np.bincount(i, minlength=len(atoms))
    assert len(atoms) == 108 and np.any(counts % 4) and np.any((counts[0::2] + counts[1::2]) % 4)
    assert 64 < counts.max() <= 128    # one or two centres per 192-record workgroup, one scan pass (n / 2 <= 64)
    assert np.diag(np.asarray(atoms.get_cell())).min() > 6.5


@gpu
def test_triangle_build_without_the_full_list(lib):
    """One element, default grid, forces wanted: every backward launch is a triangle build, the forward kernel
    writes the owned list only."""
    run_and_check(ni_model(), [ni_frame()], "tri-108", expect=TRIANGLES)


@gpu
def test_batch_with_straddling_runs(lib):
    """Three uneven frames: runs of centres straddle the frame boundaries."""
    frames = [drop(fcc(rep=(2, 2, 2), seed=31), 3), drop(fcc(rep=(2, 2, 3), seed=32), 5), fcc(rep=(3, 2, 2), seed=33)]
    run_and_check(ni_model(), frames, "tri-straddle", expect=TRIANGLES)


@gpu
def test_several_chunks(lib):
    """Two beta values: two forward launches and two backward launches, the second of which reads g[p] back.
    Both chunks are default-grid ones, so the full list is skipped; with a third, exact-path beta that chunk
    falls back to the per-apex kernel and the full list is kept for it."""
    kw = dict(eta=[0.05, 4.0], gamma=[1.0, -1.0], zeta=[1.0, 4.0])
    frames = [ni_frame()]
    nn = make_nn(["Ni"], 6.5, True, [16], sf_kwargs=dict(beta=[0.005, 0.2], **kw))       # Hd series of 12 and 16
    run_and_check(nn, frames, "chunks-tri", expect=TRIANGLES)
    nn = make_nn(["Ni"], 6.5, True, [16], sf_kwargs=dict(beta=[0.005, 10.0], **kw))      # series and exact
    run_and_check(nn, frames, "chunks-mixed", expect=TRIANGLES | PER_APEX)


@gpu
def test_no_job_list(lib):
    """rc = 8.6: more than 128 neighbours, no job list at all (job_count = -1 in both lists), ownership tested
    in the backward kernel."""
    nn = make_nn(["Ni"], 8.6, True, [16], sf_kwargs=dict(eta=[0.05, 4.0, 20.0], beta=[0.005], gamma=[1.0, -1.0],
                                                          zeta=[1.0, 4.0]))
    res = run_and_check(nn, [fcc(rep=(3, 3, 3), seed=43)], "no-list", expect=TRIANGLES)
    assert np.isfinite(res[0]["forces"]).all()


@gpu
def test_per_apex_paths(lib):
    """Two elements (default-grid forward, per-apex backward, full list read), a cell too thin for triangles, and
    triangles switched off on the handle: the full list is written and read as before."""
    els = ["Mo", "Ni"]
    run_and_check(make_nn(els, 6.0, True, [16, 16]), [alloy(els, rep=(3, 3, 3))], "nimo", expect=PER_APEX)
    run_and_check(ni_model(), [fcc(rep=(1, 3, 3), seed=41)], "thin", expect=PER_APEX)
    run_and_check(ni_model(), [ni_frame()], "tri-108", triangles=False, expect=PER_APEX)


def _same(a, b, rel, tag):
    scale = max(1.0, np.abs(b).max(initial=0.0))
    dev = np.abs(np.asarray(a) - np.asarray(b)).max(initial=0.0)
    print(f"DEV {tag} {dev:.2e} (scale {scale:.2e})")
    assert dev < rel * scale, (tag, dev, scale)


@gpu
@pytest.mark.parametrize("toggle", [False, True], ids=["triangles-on", "triangles-toggled"])
def test_full_list_validity(lib, toggle):
    """One handle, one resident batch: E + F + virial (triangle build, no full list), Hessian-vector products
    (per-apex launches on the full list), E + F + virial again. Each result equals that of a fresh handle which
    ran only that call. `toggle`: ta_set_triangles off and on between the evaluations."""
    from tensoralloy_amd import Engine, _lib
    want = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES | _lib.TA_WANT_VIRIAL | _lib.TA_WANT_ATOMIC
    nn, frames = ni_model(), [ni_frame()]
    atoms = frames[0]
    rng = np.random.RandomState(5)
    dR = rng.normal(0.0, 1.0, (2, len(atoms), 3))
    o = oracle_of(("tri-108", 0), nn, atoms)
    with Engine(nn) as fresh:
        fresh.set_frames(frames)
        ref_dF, ref_dW = fresh.hessian_vectors(dR=dR, want_virial=True)
    with Engine(nn) as fresh:
        fresh.set_frames(frames)
        fresh.compute(want)
        ref = fresh._per_frame(fresh.fetch(want))[0]
    check(ref, o, "validity/fresh", descriptors=False)
    with Engine(nn) as eng:
        eng.set_frames(frames)
        plan = [TRIANGLES, "hvp", TRIANGLES, "hvp", TRIANGLES]
        if toggle:
            plan = [TRIANGLES, "hvp", PER_APEX, TRIANGLES, "hvp", PER_APEX, "hvp", TRIANGLES]
        for k, what in enumerate(plan):
            if what == "hvp":
                dF, dW = eng.hessian_vectors(dR=dR, want_virial=True)
                _same(dF, ref_dF, F_REL, f"validity/{k}/dF")
                _same(dW, ref_dW, W_REL, f"validity/{k}/dW")
                continue
            eng.set_triangles(what == TRIANGLES)
            eng.compute(want)
            assert eng.backward_variant() == what, (k, eng.backward_variant())
            r = eng._per_frame(eng.fetch(want))[0]
            check(r, o, f"validity/{k}", descriptors=False)
            _same([r["energy"]], [ref["energy"]], E_REL, f"validity/{k}/E")
            _same(r["forces"], ref["forces"], F_REL, f"validity/{k}/F")
            _same(r["virial"], ref["virial"], W_REL, f"validity/{k}/W")


@gpu
def test_md_step(lib):
    """One ta_step with a 0.5 A skin on a two-frame batch: the device packer and the exact list."""
    from tensoralloy_amd import Atoms, Engine, _lib
    want = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES | _lib.TA_WANT_VIRIAL | _lib.TA_WANT_ATOMIC
    nn = ni_model()
    frames = [drop(fcc(rep=(3, 2, 2), seed=51), 3), fcc(rep=(2, 3, 3), seed=52)]
    sizes = np.cumsum([0] + [len(a) for a in frames])
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        eng.set_frames(frames)
        pos = np.concatenate([a.positions for a in frames]) + np.random.RandomState(7).normal(0, 0.02, (sizes[-1], 3))
        got = {k: np.array(v) for k, v in eng.step(pos, want, view=True).items()}
        assert eng.backward_variant() == TRIANGLES
    for f, atoms in enumerate(frames):
        moved = Atoms(symbols=atoms.get_chemical_symbols(), positions=pos[sizes[f]:sizes[f + 1]],
                      cell=np.asarray(atoms.get_cell()), pbc=True)
        r = dict(energy=got["energy"][f], atomic=got["atomic"][sizes[f]:sizes[f + 1]],
                 forces=got["forces"][sizes[f]:sizes[f + 1]], virial=got["virial"][f])
        check(r, c_oracle(nn, moved), f"md-step/frame{f}", descriptors=False)
