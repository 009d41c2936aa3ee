"""GPU: structure factors inside the device MD loop (`ta_md_set_sq`, csrc/ta_md_sq.hip) against the long-double
NumPy definition (tests/md_sq_reference.py), which shares nothing with the library.

The reference is fed the device's own whole-step states: `md_state()` between the calls of a run cut at every
sample (x and v of the state each sample was taken of), or the ring of `md_set_sampling`. Positions are thermalised
(a jittered lattice moved by the dynamics), dt = 1 fs, at most 140 atoms and 30 steps (one case of 20000 atoms
samples its entry state only).

The bound is no hand-picked constant. For every rho_a(q) the reference computes, from its own numbers alone,
    B = N_a 2^-53 (16 + 2 pi 4 kappa_inf(h) max_i sum_c |n_c s_ic| + m)
with m = (atoms per workgroup of the amplitude launch) + (workgroups of the frame): in csrc/ta_md_sq.hip a partial
is a chain of at most `chunk` additions in atom order (md_sq_amplitude_kernel) and a ring entry a chain of the
frame's partials in index order (md_sq_sum_kernel); `chunk` is read from the plan (`md_sq()["chunk"]`). A current
component has B |v|_max, an accumulator the propagated bound (tests/md_sq_reference.py). Every case prints the
largest error / bound. Measured on the MI355X (profiles/md_sq.md): at most 0.25 on rho (a frame of one atom; 0.18 on
the 32-atom frames, 0.043 at |n_c| = 64), 0.052 on A_rho, 0.038 on the currents, 0.013 on A_L and 0.0085 on A_J; 2.3e-3
on the frame of 20000 atoms, where the bound grows with N_a and the error with its root. A ratio that small could
not catch a single-precision slip, so every case also asserts an absolute error below 1e-9 N_a on rho.

The run that fails (for the getters behind it) fails on the host: its record buffers, 2^31 records of 128 frames,
are 2.5 TB that no device has, and `ta_md_run` allocates them before it enqueues anything.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import md_sq_reference as ref
from tests.helpers import fcc, make_eam, make_nn
from tests.test_gpu_md import DT, WANT, _ni_setup, _velocities
from tests.test_gpu_md_corr import _assert_a
from tests.test_gpu_sf import _alloy
from tensoralloy_amd import Atoms, md

pytestmark = pytest.mark.gpu

KT0, TAU = md.kB * 600.0, 20 * DT
FRICTION, SEED = 0.01 / md.fs, 0x9E3779B97F4A7C15

SETUPS = {
    "nve": lambda eng: None,
    "berendsen": lambda eng: eng.md_set_thermostat(KT0, TAU),
    "langevin": lambda eng: eng.md_set_langevin(KT0, FRICTION, SEED),
    "nhc": lambda eng: eng.md_set_nose_hoover(KT0, TAU, chain=3),
}


def _triples(top):
    """All triples with |n_c| <= top, one of each +-n pair, and (0, 0, 0)."""
    g = np.arange(-top, top + 1)
    n = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    first = np.where(n[:, 0] != 0, n[:, 0], np.where(n[:, 1] != 0, n[:, 1], n[:, 2]))
    return np.ascontiguousarray(n[first >= 0], dtype=np.int32)


MILLER3 = _triples(3)
assert len(MILLER3) == (7 ** 3 - 1) // 2 + 1 and (MILLER3 == 0).all(axis=1).sum() == 1


def _freeze(out):
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
        elif isinstance(a, dict):
            _freeze(a)
    return out


def _run(nn, frames, v0, skin, runs, miller=None, lags=1, every=1, currents=True, integrator="nve", sampling=None):
    """The runs `runs` (steps per md_run call) on the device: final state, records, the whole-step states (x, v) at
    entry and behind every call (`states`, `vels`, at the absolute steps `steps`), with `miller` the structure
    factors (`sq`, `amps`), with `sampling` = (n_lags, sample_every) the ring and sums of `md_set_sampling` too."""
    from tensoralloy_amd import Engine
    with Engine(nn) as eng:
        eng.set_skin(skin)
        eng.set_frames(frames)
        eng.md_init(None, v0)
        SETUPS[integrator](eng)
        if sampling is not None:
            eng.md_set_sampling(*sampling)
        if miller is not None:
            eng.md_set_sq(miller, lags, every, currents)
        states, vels, steps, outs = [eng.md_state()[0]], [eng.md_state()[1]], [0], []
        for n in runs:
            outs.append(eng.md_run(n, DT))
            x, v = eng.md_state()
            states.append(x)
            vels.append(v)
            steps.append(steps[-1] + n)
        x, v = eng.md_state()
        res = dict(x=x, v=v, n_rebuilds=sum(o["n_rebuilds"] for o in outs), states=np.array(states), vels=np.array(vels),
                   steps=np.array(steps))
        if miller is not None:
            res["sq"], res["amps"] = eng.md_sq(), eng.md_sq_amplitudes()
        if sampling is not None:
            res["corr"], res["samples"] = eng.md_correlations(), eng.md_samples()
    for k in ("epot", "ekin", "echain"):
        if k in outs[0]:
            res[k] = np.concatenate([o[k][1 if j else 0:] for j, o in enumerate(outs)])
    return _freeze(res)


def _species(nn, frames):
    els = list(nn.elements)
    return np.array([els.index(sym) for a in frames for sym in a.get_chemical_symbols()])


def _sampled(dev, every):
    """The states of a run cut at every sample: those at the multiples of `every`."""
    keep = dev["steps"] % every == 0
    keep[1:] &= dev["steps"][1:] != dev["steps"][:-1]   # (a call of 0 steps repeats a state, it is sampled once)
    return dev["states"][keep], dev["vels"][keep], dev["steps"][keep]


def _cuts(steps, every):
    return [every] * (steps // every) + ([steps % every] if steps % every else [])


def _check(dev, nn, frames, xs, vs, steps, miller, lags, every, currents=True):
    """Everything `dev` holds of the structure factors against the reference on the samples xs, vs [S, N, 3] taken
    at `steps`: `info`, the amplitude rows the ring holds, the accumulators. Prints and returns the largest
    error / bound."""
    sq, amps = dev["sq"], dev["amps"]
    E, S, Q, F = len(nn.elements), len(xs), len(miller), len(frames)
    held = min(S, lags)
    assert (sq["n_samples"], sq["n_lags"], sq["sample_every"], sq["last_step"], sq["currents"]) == \
        (S, lags, every, int(steps[-1]), currents)
    assert np.array_equal(sq["miller"], miller) and sq["miller"].dtype == np.int32
    assert np.array_equal(sq["n_origins"], np.maximum(0, S - np.arange(lags)))
    assert sq["a_rho"].shape == (F, E, E, lags, Q) and amps["rho"].shape == (held, F, E, Q)
    assert np.array_equal(amps["steps"], np.asarray(steps)[-held:])
    if not currents:
        assert sq["a_l"] is None and sq["a_j"] is None and amps["cur"] is None
    species = _species(nn, frames)
    chunk = sq["chunk"]
    worst, at = 0.0, 0
    for f, atoms in enumerate(frames):
        n = len(atoms)
        cell = np.asarray(atoms.get_cell(complete=True))
        sp = species[at:at + n]
        chain = min(chunk, max(n, 1)) + max(1, -(-n // chunk))   # the two chains of additions, from the plan
        want = ref.structure_factors(xs[:, at:at + n], vs[:, at:at + n] if currents else None, cell, sp, E, miller, lags, chain)
        assert np.abs(sq["q"][f] - want["q"]).max() < 1e-13 * max(1.0, np.abs(want["q"]).max())
        pairs = [("rho", amps["rho"][:, f], want["rho"][-held:], want["rho_bound"][-held:]),
                 ("a_rho", sq["a_rho"][f], want["a_rho"], want["a_rho_bound"])]
        if currents:
            pairs += [("cur", amps["cur"][:, f], want["cur"][-held:], want["cur_bound"][-held:, :, :, None]),
                      ("a_l", sq["a_l"][f], want["a_l"], want["a_l_bound"]),
                      ("a_j", sq["a_j"][f], want["a_j"], want["a_j_bound"])]
        for key, got, exp, bound in pairs:
            gap = np.abs(got - exp)
            bound = np.broadcast_to(bound, gap.shape)
            has = bound > 0.0
            ratio = float((gap[has] / bound[has]).max()) if has.any() else 0.0
            print(f"frame {f} {key}: largest error / bound {ratio:.3e} (largest error {float(gap.max()):.3e})")
            worst = max(worst, ratio)
            assert np.all(gap <= bound), (f, key, ratio, float(gap.max()))
        n_a = np.bincount(sp, minlength=E)[:E].astype(np.float64)
        assert np.all(np.abs(amps["rho"][:, f] - want["rho"][-held:]) <= 1e-9 * n_a[None, :, None])   # no fp32 slip
        at += n
    print(f"largest error / bound of the case: {worst:.3e}")
    return worst


# -- 1: single frame, EAM and G2 -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ni_model(model):
    nn, atoms = _ni_setup()   # 32 Ni atoms, cell 7.05
    if model == "g2":
        nn = make_nn(["Ni"], 6.0, False, [8])
    return nn, atoms


@functools.lru_cache(maxsize=None)
def _ni_run(model, every, cut, skin=0.3, sampling=None, steps=20):
    nn, atoms = _ni_model(model)
    v0 = _velocities([atoms], 600.0, 3)
    return _run(nn, [atoms], v0, skin, _cuts(steps, every) if cut else [steps], MILLER3, 8, every, True, sampling=sampling)


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("model", ["eam", "g2"])
def test_single_frame_against_the_reference(lib, model, every):
    """NVE, 20 steps, L = 8: the ring wraps. The amplitudes of the last 8 samples, all three accumulators, info."""
    nn, atoms = _ni_model(model)
    dev = _ni_run(model, every, True)
    xs, vs, steps = _sampled(dev, every)
    assert np.array_equal(steps, np.arange(0, 21, every)) and len(MILLER3) == 172
    _check(dev, nn, [atoms], xs, vs, steps, MILLER3, 8, every)
    assert np.abs(dev["sq"]["a_rho"][0, 0, 0, 0, 0] - len(xs) * 32.0 ** 2) == 0.0   # n = 0: rho = N, exactly
    assert np.abs(dev["sq"]["a_j"]).max() > 0.0 and np.abs(dev["sq"]["a_l"]).max() > 0.0


# -- 2: a cut run is the uncut run, bit for bit; rebuilds ---------------------------------------------------------
@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("model", ["eam", "g2"])
def test_uncut_run_gives_the_bits_of_the_cut_run(lib, model, every):
    cut, uncut = _ni_run(model, every, True), _ni_run(model, every, False)
    assert np.array_equal(uncut["x"], cut["x"]) and np.array_equal(uncut["v"], cut["v"])
    for key in ("n_samples", "n_lags", "sample_every", "last_step", "currents", "chunk"):
        assert uncut["sq"][key] == cut["sq"][key], key
    for key in ("a_rho", "a_l", "a_j"):
        assert np.array_equal(uncut["sq"][key], cut["sq"][key]), key
    for key in ("rho", "cur", "steps"):
        assert np.array_equal(uncut["amps"][key], cut["amps"][key]), key
    assert np.abs(cut["sq"]["a_rho"]).sum() > 0.0


def test_rebuilds_in_the_middle_of_a_run(lib):
    """A skin of 0.05: the run rebuilds its list inside the windows of steps the loop enqueues ahead, and the launches
    behind a stale list are enqueued again. The snapshots are this run's own: the ring of `md_set_sampling`."""
    nn, atoms = _ni_model("eam")
    dev = _ni_run("eam", 1, False, skin=0.05, sampling=(32, 1))
    assert dev["n_rebuilds"] > 0
    assert np.array_equal(dev["samples"]["steps"], np.arange(21))
    _check(dev, nn, [atoms], dev["samples"]["x"], dev["samples"]["v"], np.arange(21), MILLER3, 8, 1)


# -- 3: every thermostat: the velocities are the whole-step ones ----------------------------------------------------
@pytest.mark.parametrize("integrator", ["berendsen", "langevin", "nhc"])
def test_every_thermostat_with_currents(lib, integrator):
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 600.0, 3)
    plain = _run(nn, [atoms], v0, 0.3, _cuts(10, 2), integrator=integrator)
    dev = _run(nn, [atoms], v0, 0.3, _cuts(10, 2), MILLER3, 4, 2, True, integrator)
    for k in ("x", "v", "epot", "ekin", "states", "vels") + (("echain",) if integrator == "nhc" else ()):
        assert np.array_equal(dev[k], plain[k]), k   # bit for bit: the launches only read the snapshot
    xs, vs, steps = _sampled(dev, 2)
    assert np.array_equal(steps, [0, 2, 4, 6, 8, 10])
    _check(dev, nn, [atoms], xs, vs, steps, MILLER3, 4, 2)


# -- 4: two elements, three frames of different sizes and triclinic cells --------------------------------------------
def _sheared(atoms, m):
    m = np.eye(3) + np.asarray(m)
    return Atoms(symbols=atoms.get_chemical_symbols(), positions=atoms.positions @ m,
                 cell=np.asarray(atoms.get_cell(complete=True)) @ m, pbc=True)


@functools.lru_cache(maxsize=None)
def _nimo():
    nn = make_eam(["Mo", "Ni"], 6.0, potential="zjw04")
    frames = [_sheared(_alloy(["Ni", "Mo"], rep=(2, 2, 2)), [[0.0, 0.0, 0.0], [0.12, 0.0, 0.0], [-0.07, 0.09, 0.0]]),
              _sheared(fcc(rep=(2, 2, 3), jitter=0.02, seed=3), [[0.0, 0.0, 0.0], [-0.05, 0.0, 0.0], [0.1, 0.04, 0.0]]),
              _sheared(_alloy(["Ni", "Ni", "Mo"], rep=(2, 3, 2), seed=5), [[0.0, 0.0, 0.0], [0.08, 0.0, 0.0], [0.03, -0.11, 0.0]])]
    return nn, frames, _velocities(frames, 600.0, 5)


def test_two_element_batch_one_frame_without_the_second_element(lib):
    nn, frames, v0 = _nimo()
    assert [len(a) for a in frames] == [32, 48, 48]
    mo, ni = list(nn.elements).index("Mo"), list(nn.elements).index("Ni")
    dev = _run(nn, frames, v0, 0.3, _cuts(8, 2), MILLER3, 3, 2, True)
    xs, vs, steps = _sampled(dev, 2)
    _check(dev, nn, frames, xs, vs, steps, MILLER3, 3, 2)
    sq = dev["sq"]
    assert np.array_equal(sq["n_by_element"][:, mo], [16, 0, 16])
    # the partials a != b in both orders: at lag 0 they are each other's transpose, at later lags they are not
    for key in ("a_rho", "a_l", "a_j"):
        a = sq[key]
        assert np.array_equal(a[:, mo, ni, 0], a[:, ni, mo, 0]) and np.abs(a[0, mo, ni, 0]).max() > 0.0, key
        assert not np.array_equal(a[0, mo, ni, 1], a[0, ni, mo, 1]), key
        assert not a[1, mo].any() and not a[1, :, mo].any() and np.abs(a[1, ni, ni]).max() > 0.0, key   # no Mo in frame 1
    assert not dev["amps"]["rho"][:, 1, mo].any() and not dev["amps"]["cur"][:, 1, mo].any()
    f_ab = md.intermediate_scattering(sq["a_rho"], sq["n_samples"], sq["n_by_element"])
    assert np.all(np.isnan(f_ab[1, mo])) and np.all(np.isnan(f_ab[1, :, mo])) and np.all(np.isfinite(f_ab[1, ni, ni]))
    assert np.all(np.isfinite(f_ab[0])) and np.all(np.isfinite(f_ab[2]))
    s_ab, s = md.structure_factor(sq["a_rho"], sq["n_samples"], sq["n_by_element"])
    assert np.all(np.isfinite(s)) and np.array_equal(s[1], s_ab[1, ni, ni])


# -- 5: shape edges ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_q", [1, 65, 257])
def test_vector_counts_around_the_tile(lib, n_q):
    """A workgroup of the amplitude launch owns 64 q-vectors: one vector, one more than a tile, one more than four."""
    nn, atoms = _ni_setup()
    miller = np.ascontiguousarray(_triples(4)[-n_q:])
    assert len(miller) == n_q
    dev = _run(nn, [atoms], _velocities([atoms], 600.0, 3), 0.3, [1, 1], miller, 2, 1, True)
    _check(dev, nn, [atoms], dev["states"], dev["vels"], dev["steps"], miller, 2, 1)


def _with_vacancies(atoms, n_keep, seed):
    keep = np.sort(np.random.RandomState(seed).permutation(len(atoms))[:n_keep])
    return Atoms(symbols=[atoms.get_chemical_symbols()[k] for k in keep], positions=atoms.positions[keep],
                 cell=np.asarray(atoms.get_cell(complete=True)), pbc=True)


def test_a_frame_of_one_chunk_plus_one_atom_and_a_frame_of_one_atom(lib):
    nn = _ni_setup()[0]
    big = _with_vacancies(fcc(rep=(2, 3, 3), jitter=0.02, seed=7), 65, 1)
    one = Atoms(symbols=["Ni"], positions=[[0.4, 1.1, 2.3]], cell=np.diag([5.0, 5.2, 5.4]), pbc=True)
    frames = [big, one]
    dev = _run(nn, frames, _velocities(frames, 600.0, 9), 0.3, [2, 2], MILLER3, 3, 2, True)
    assert len(big) == dev["sq"]["chunk"] + 1   # the second workgroup of frame 0 owns one atom
    _check(dev, nn, frames, dev["states"], dev["vels"], dev["steps"], MILLER3, 3, 2)
    assert np.allclose(np.abs(dev["amps"]["rho"][:, 1, 0]), 1.0, rtol=0.0, atol=1e-15)   # one atom: |rho| = 1


@pytest.mark.parametrize("lags, steps", [(1, 4), (16, 4)])
def test_static_case_and_a_ring_that_does_not_fill(lib, lags, steps):
    nn, atoms = _ni_setup()
    dev = _run(nn, [atoms], _velocities([atoms], 600.0, 3), 0.3, [1] * steps, MILLER3, lags, 1, True)
    _check(dev, nn, [atoms], dev["states"], dev["vels"], dev["steps"], MILLER3, lags, 1)
    if lags > steps + 1:   # lags without a time origin hold nothing
        assert not dev["sq"]["a_rho"][..., steps + 1:, :].any() and dev["sq"]["n_origins"][steps + 1] == 0


def test_largest_indices_and_atoms_far_from_the_cell(lib):
    """|n_c| = 64 with every atom displaced by up to +-3 lattice vectors of its own: n . s reaches several hundred,
    and the exact reduction of the phase is what keeps the error inside the bound."""
    nn, atoms = _ni_setup()
    rng = np.random.RandomState(21)
    cell = np.asarray(atoms.get_cell(complete=True))
    far = Atoms(symbols=atoms.get_chemical_symbols(), positions=atoms.positions + rng.randint(-3, 4, size=(32, 3)) @ cell,
                cell=cell, pbc=True)
    miller = np.array([[64, 64, 64], [64, -64, 64], [-64, 0, 63], [0, 0, 64], [1, 0, 0], [0, 0, 0], [33, -64, 7]], dtype=np.int32)
    v0 = _velocities([atoms], 600.0, 3)
    dev = _run(nn, [far], v0, 0.3, [1, 1], miller, 2, 1, True)
    assert np.abs(dev["states"][0] - far.positions).max() == 0.0 and np.abs(dev["states"]).max() > 3 * 7.0
    _check(dev, nn, [far], dev["states"], dev["vels"], dev["steps"], miller, 2, 1)


def test_without_currents(lib):
    from tensoralloy_amd import Engine, _lib
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 600.0, 3)
    dev = _run(nn, [atoms], v0, 0.3, [2, 2], MILLER3, 3, 2, False)
    _check(dev, nn, [atoms], dev["states"], dev["vels"], dev["steps"], MILLER3, 3, 2, currents=False)
    with_currents = _run(nn, [atoms], v0, 0.3, [2, 2], MILLER3, 3, 2, True)
    assert np.array_equal(dev["sq"]["a_rho"], with_currents["sq"]["a_rho"])   # the density part is the same build's bits
    with Engine(nn) as eng:
        eng.set_frames([atoms])
        eng.md_init(None, v0)
        eng.md_set_sq(MILLER3, 2, 1, False)
        eng.md_run(1, DT)
        buf = np.zeros((1, 1, 1, 2, len(MILLER3)))
        null = C.POINTER(C.c_double)()
        for args in ((null, _lib.as_dp(buf), null), (null, null, _lib.as_dp(buf))):
            rc = eng._lib.ta_md_get_sq(eng._handle, *args, None, C.POINTER(C.c_int32)())
            assert rc == _lib.TA_ERR_INVALID
            assert "ta_md_get_sq: a_l and a_j need the currents" in eng._lib.ta_last_error(eng._handle).decode()
        cur = np.zeros((1, 1, 1, len(MILLER3), 3, 2))
        rc = eng._lib.ta_md_get_sq_amplitudes(eng._handle, 0, 1, null, _lib.as_dp(cur), None)
        assert rc == _lib.TA_ERR_INVALID
        assert "ta_md_get_sq_amplitudes: cur needs the currents" in eng._lib.ta_last_error(eng._handle).decode()
        assert eng._lib.ta_md_get_sq(eng._handle, _lib.as_dp(buf), null, null, None, C.POINTER(C.c_int32)()) == _lib.TA_OK
        assert np.abs(buf).max() > 0.0


def test_both_snapshot_routes_in_one_run(lib):
    """`md_set_sampling` every 2 steps and the structure factors every 3: at steps 0, 6, 12 the integrator writes
    the state to the slot of the correlation ring and the structure factors read it there, at 3 and 9 it writes
    to the two rows of this feature; the VACF / MSD sums still meet their own reference."""
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 600.0, 3)
    dev = _run(nn, [atoms], v0, 0.3, _cuts(12, 3), MILLER3, 4, 3, True, sampling=(8, 2))
    xs, vs, steps = _sampled(dev, 3)
    assert np.array_equal(steps, [0, 3, 6, 9, 12])
    _check(dev, nn, [atoms], xs, vs, steps, MILLER3, 4, 3)
    assert np.array_equal(dev["samples"]["steps"], np.arange(0, 13, 2))
    for n, t in ((0, 0), (3, 6), (6, 12)):   # the states both features sampled are the same doubles
        k = list(steps).index(t)
        assert np.array_equal(dev["samples"]["x"][n], xs[k]) and np.array_equal(dev["samples"]["v"][n], vs[k])
    _assert_a(dev, dev["samples"]["x"], dev["samples"]["v"], [32], _species(nn, [atoms]), 1, 8)
    alone = _run(nn, [atoms], v0, 0.3, _cuts(12, 3), sampling=(8, 2))
    for key in ("vacf_sum", "msd_sum"):
        assert np.array_equal(dev["corr"][key], alone["corr"][key]), key


# -- 6: one large frame: the sum over many chunks -------------------------------------------------------------------
def test_frame_of_20000_atoms(lib):
    """Above 16384 atoms a workgroup owns 1024 atoms: 20 chunks, slabs of 64 atoms inside each, and the sum of the
    chunks in index order. The entry state only (`md_run(0)`)."""
    nn = _ni_setup()[0]
    atoms = fcc(rep=(10, 20, 25), jitter=0.05, seed=1)
    assert len(atoms) == 20000
    miller = md.q_points(np.asarray(atoms.get_cell(complete=True)), 0.545)
    assert 250 <= len(miller) <= 350
    dev = _run(nn, [atoms], _velocities([atoms], 600.0, 7), 0.3, [0], miller, 1, 1, True)
    assert dev["sq"]["chunk"] == 1024
    _check(dev, nn, [atoms], dev["states"][:1], dev["vels"][:1], dev["steps"][:1], miller, 1, 1)
    s_ab, s = md.structure_factor(dev["sq"]["a_rho"], 1, dev["sq"]["n_by_element"])
    assert s.shape == (1, len(miller)) and np.all(s >= 0.0) and np.all(s < 5.0)   # below the first Bragg peak: diffuse only


# -- 7: life cycle and refusals --------------------------------------------------------------------------------------
def test_life_cycle_and_refusals(lib):
    from tensoralloy_amd import Engine
    nn, atoms = _ni_setup()
    v0 = _velocities([atoms], 300.0, 3)
    ok = MILLER3[:10]
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        with pytest.raises(ValueError, match="no resident batch"):
            eng.md_sq()
        eng.md_set_sq(None)   # off is always allowed
        with pytest.raises(ValueError, match="ta_md_set_sq: no resident batch"):
            eng.md_set_sq(ok)
        eng.set_frames([atoms])
        with pytest.raises(ValueError, match="ta_md_get_sq called before ta_md_init"):
            eng.md_sq()
        with pytest.raises(ValueError, match="ta_md_set_sq called before ta_md_init"):
            eng.md_set_sq(ok)
        eng.md_init(None, v0)
        with pytest.raises(ValueError, match=r"ta_md_get_sq: the structure factors are off \(ta_md_set_sq\)"):
            eng.md_sq()
        with pytest.raises(ValueError, match=r"ta_md_get_sq_amplitudes: the structure factors are off \(ta_md_set_sq\)"):
            eng.md_sq_amplitudes()
        eng.md_set_sq(ok, 4, 2, True)
        for what, args in (("n_lags", (ok, 0, 1)), ("n_lags", (ok, 4097, 1)), ("sample_every", (ok, 1, 0)),
                           ("sample_every", (ok, 1, -2))):
            with pytest.raises(ValueError, match="ta_md_set_sq: " + what):
                eng.md_set_sq(*args)
        with pytest.raises(ValueError, match="Miller indices must be within"):
            eng.md_set_sq(np.array([[65, 0, 0]]))
        with pytest.raises(ValueError, match="at most 4096"):
            eng.md_set_sq(np.ones((4097, 3), dtype=int))
        with pytest.raises(ValueError, match="miller must be integers"):
            eng.md_set_sq(np.ones((4, 2), dtype=int))
        # ... and through the C ABI, past the checks of the Python layer
        from tensoralloy_amd import _lib
        bad = np.array([[1, 0, 0], [0, -65, 0]], dtype=np.int32)
        for p, m, text in ((_lib.MdSqParams(2, 1, 1, 0), bad, r"miller[1][1] = -65 must be within +-64"),
                           (_lib.MdSqParams(4097, 1, 1, 0), bad, "n_q must be 0 .. 4096"),
                           (_lib.MdSqParams(-1, 1, 1, 0), bad, "n_q must be 0 .. 4096"),
                           (_lib.MdSqParams(2, 1, 1, 2), bad, "currents must be 0 or 1"),
                           (_lib.MdSqParams(2, 1, 1, 0), None, "miller is NULL")):
            ptr = m.ctypes.data_as(C.POINTER(C.c_int32)) if m is not None else C.POINTER(C.c_int32)()
            assert eng._lib.ta_md_set_sq(eng._handle, C.byref(p), ptr) == _lib.TA_ERR_INVALID
            assert "ta_md_set_sq: " + text in eng._lib.ta_last_error(eng._handle).decode()
        out = eng.md_sq()   # ... and a refused call left the setting as it was
        assert out["a_rho"].shape == (1, 1, 1, 4, 10) and not out["a_rho"].any() and not out["a_j"].any()
        assert (out["n_samples"], out["n_lags"], out["sample_every"], out["last_step"], out["currents"]) == (0, 4, 2, -1, True)
        with pytest.raises(ValueError, match=r"first_lag \+ n = 1 exceeds the 0 rows held"):
            eng.md_sq_amplitudes(1)
        res = eng.md_run(10, DT)
        assert set(res) == {"epot", "ekin", "n_rebuilds"}   # the result dict is unchanged
        assert (eng.md_sq()["n_samples"], eng.md_sq()["last_step"]) == (6, 10)
        assert eng.md_sq_amplitudes()["rho"].shape == (4, 1, 1, 10) and eng.md_sq_amplitudes(2)["steps"].tolist() == [8, 10]
        with pytest.raises(ValueError, match=r"first_lag \+ n = 5 exceeds the 4 rows held"):
            eng.md_sq_amplitudes(5)
        # the barostat and the structure factors together: refused by the run, both named, nothing lost
        x0, v_before = eng.md_state()
        before = eng.md_sq()
        eng.md_set_barostat(0.0, 100 * DT, 1.0)
        with pytest.raises(ValueError, match=r"ta_md_run: the structure factors \(ta_md_set_sq\) and the barostat \(ta_md_set_barostat\)"):
            eng.md_run(5, DT)
        eng.md_set_barostat(0.0, 0.0, 0.0)
        x1, v1 = eng.md_state()
        after = eng.md_sq()
        assert np.array_equal(x0, x1) and np.array_equal(v_before, v1)
        assert np.array_equal(before["a_rho"], after["a_rho"]) and after["n_samples"] == 6
        eng.md_run(2, DT)   # after the refusal the loop still runs: step 12
        assert (eng.md_sq()["n_samples"], eng.md_sq()["last_step"]) == (7, 12)
        # setting it again zeroes; sample 0 is then the first multiple of sample_every not behind the step
        eng.md_run(1, DT)   # step 13
        eng.md_set_sq(ok[:3], 1, 3, False)
        out = eng.md_sq()
        assert out["a_rho"].shape == (1, 1, 1, 1, 3) and out["n_samples"] == 0 and not out["a_rho"].any() and out["a_l"] is None
        eng.md_run(5, DT)   # steps 14 .. 18: samples at 15 and 18
        assert (eng.md_sq()["n_samples"], eng.md_sq()["last_step"]) == (2, 18)
        # set_frames keeps the setting and drops the data with the MD state; md_init starts from zero sums
        eng.set_frames([atoms])
        with pytest.raises(ValueError, match="ta_md_get_sq called before ta_md_init"):
            eng.md_sq()
        eng.md_init(None, v0)
        out = eng.md_sq()
        assert out["a_rho"].shape == (1, 1, 1, 1, 3) and not out["a_rho"].any()
        assert (out["n_samples"], out["sample_every"], out["last_step"]) == (0, 3, -1)
        eng.md_run(3, DT)
        assert (eng.md_sq()["n_samples"], eng.md_sq()["last_step"]) == (2, 3)
        # a frame that is not periodic in all three directions has no wave vectors of its own: a batch with one
        # switches the feature off at md_init (which says so), and the setter refuses it
        slab = Atoms(symbols=atoms.get_chemical_symbols(), positions=atoms.positions,
                     cell=np.asarray(atoms.get_cell(complete=True)), pbc=[True, True, False])
        eng.set_frames([atoms, slab])
        with pytest.raises(ValueError, match=r"ta_md_init: ta_md_set_sq: frame 1 is not periodic along all three axes.*the feature is off"):
            eng.md_init(None, np.concatenate([v0, v0]))
        assert eng.md_sq_vectors == 0
        eng.md_run(1, DT)
        with pytest.raises(ValueError, match="ta_md_set_sq: frame 1 is not periodic along all three axes"):
            eng.md_set_sq(ok)
        with pytest.raises(ValueError, match="structure factors are off"):
            eng.md_sq()
        eng.md_run(2, DT)   # ... and the loop runs
        eng.md_set_barostat(0.0, 100 * DT, 1.0)   # with the feature off the barostat runs
        eng.set_frames([atoms])
        eng.md_init(None, v0)
        eng.md_run(2, DT)


def test_getters_after_a_failed_run(lib):
    """A run that fails leaves the data invalid until `md_set_sq` or `md_init` is called again. The failure:
    n_steps = 2^31 - 1 with a record of 128 frames at every step asks for 2.5 TB of `epot` records, which
    `ta_md_run` allocates first, behind the point where it marks the data invalid; nothing is launched."""
    from tensoralloy_amd import Engine, _lib
    nn, atoms = _ni_setup()
    frames = [atoms] * 128
    v0 = np.tile(_velocities([atoms], 300.0, 3), (128, 1))
    null = C.POINTER(C.c_double)()
    ok = MILLER3[:5]

    def failing_run(eng):
        x0, v_before = eng.md_state()
        rc = eng._lib.ta_md_run(eng._handle, 2 ** 31 - 1, DT, WANT, 1, null, null, None)
        msg = eng._lib.ta_last_error(eng._handle).decode()
        print("failed run:", rc, msg)
        assert rc in (_lib.TA_ERR_HIP, _lib.TA_ERR_NOMEM) and "hipMalloc" in msg
        x1, v1 = eng.md_state()
        assert np.array_equal(x0, x1) and np.array_equal(v_before, v1)

    refusal = r"ta_md_get_sq%s: a ta_md_run failed and left the data invalid; call ta_md_set_sq or ta_md_init again"
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        eng.set_frames(frames)
        eng.md_init(None, v0)
        eng.md_set_sq(ok, 2, 1, True)
        eng.md_run(2, DT)
        assert eng.md_sq()["n_samples"] == 3
        failing_run(eng)
        with pytest.raises(ValueError, match=refusal % ""):
            eng.md_sq()
        with pytest.raises(ValueError, match=refusal % "_amplitudes"):
            eng.md_sq_amplitudes()
        eng.md_run(1, DT)   # the loop goes on (step 3) and samples nothing; the getters still refuse
        with pytest.raises(ValueError, match=refusal % ""):
            eng.md_sq()
        eng.md_set_sq(ok, 2, 1, True)   # set again: zero sums, sample 0 is the state of step 3
        out = eng.md_sq()
        assert (out["n_samples"], out["last_step"]) == (0, -1) and not out["a_rho"].any()
        eng.md_run(2, DT)
        out = eng.md_sq()
        assert (out["n_samples"], out["last_step"]) == (3, 5)
        assert np.abs(out["a_rho"][0]).sum() > 0 and np.array_equal(out["a_rho"][127], out["a_rho"][0])
        failing_run(eng)
        with pytest.raises(ValueError, match=refusal % ""):
            eng.md_sq()
        eng.md_init(None, v0)   # ... or md_init: the setting is kept, the sums start from zero
        out = eng.md_sq()
        assert (out["n_samples"], out["sample_every"], out["last_step"]) == (0, 1, -1) and not out["a_rho"].any()
        eng.md_run(1, DT)
        assert eng.md_sq()["n_samples"] == 2


def test_device_md_end_to_end(lib):
    from tensoralloy_amd import Engine
    nn, atoms = _ni_setup()
    atoms = atoms.copy()
    v0 = _velocities([atoms], 600.0, 3)
    cell = np.asarray(atoms.get_cell(complete=True))
    miller = md.q_points(cell, 3.3)   # (the (200) reflections, at 3.57, stay outside)
    with Engine(nn) as eng:
        dyn = md.DeviceMD(eng, atoms, DT, velocities=v0, temperature_K=600.0, tdamp=20 * DT, sq_miller=miller, sq_lags=4,
                          sq_every=2, sq_currents=True)
        dyn.run(6)
        dyn.run(5)
        out = eng.md_sq()
        assert (out["n_samples"], out["last_step"], out["n_lags"]) == (6, 10, 4)
        q, q_norm, s_ab, s = dyn.get_structure_factor()
        assert q.shape == (len(miller), 3) and s_ab.shape == (1, 1, len(miller)) and s.shape == (len(miller),)
        assert np.allclose(q, 2.0 * np.pi * miller @ np.linalg.inv(cell).T, rtol=0.0, atol=1e-13) and np.all(q_norm <= 3.3)
        # fcc, 2 x 2 x 2 cells: the (111) reflections are the triples (+-2, +-2, +-2); S there is nearly N
        bragg = np.all(np.abs(miller) == 2, axis=1)
        assert bragg.sum() == 4 and np.all(s[bragg] > 0.8 * 32) and np.all(s[~bragg] < 0.5)
        t, f_ab, c_l, c_t = dyn.get_intermediate_scattering()
        assert np.array_equal(t, np.arange(4) * 2 * DT) and f_ab.shape == c_l.shape == c_t.shape == (1, 1, 4, len(miller))
        assert np.array_equal(f_ab[0, 0, 0], s) and np.all(np.isfinite(c_l)) and np.all(c_t[0, 0, 0] >= -1e-12)
        nu, s_qw = md.dynamic_structure_factor(f_ab, 2 * DT)
        assert nu.shape == (4,) and s_qw.shape == f_ab.shape
        plain = md.DeviceMD(eng, atoms, DT, velocities=v0)   # sq_miller None: the feature is set off
        assert eng.md_sq_vectors == 0
        with pytest.raises(ValueError, match=r"structure factors are off \(sq_miller\)"):
            plain.get_structure_factor()
        with pytest.raises(ValueError, match=r"structure factors are off \(ta_md_set_sq\)"):
            eng.md_sq()
