"""GPU: heat current and pressure tensor inside the device MD loop (`ta_md_set_flux`, csrc/ta_md_flux.hip) against the
finite-difference reference (tests/md_flux_reference.py): NumPy and the CPU oracles, nothing of the library.

The reference is fed the device's own whole-step states (`md_state()` between the calls of a run cut at every sample).
The bound of a comparison is no hand-picked constant: it is the reference's own uncertainty (its Richardson values
over the steps (h, 2h) against those over (2h, 4h), propagated to each of the 18 numbers of a row) plus a rounding
term 2^-53 x chain x (sum of the |terms| of the number), where `chain` counts the additions of the longest chain of
csrc/ta_md_flux.hip from the plan the library reports (`md_flux()`: atoms per workgroup, lanes per centre, most
workgroups of a frame) and the most neighbours of an atom: a lane adds ceil(nnl_max / lanes) pair terms and one atom
term per pass and makes chunk / 16 passes, a wavefront's sum takes 6 levels, a workgroup adds its 4 wavefronts and a
frame its workgroups. Every case prints the largest error / bound (measured: profiles/md_flux.md). A ratio can hide a
single-precision slip, so every case also asserts an absolute error below 1e-9 x sum |terms|.

The run that fails (for the getters behind it) fails on the host, as in tests/test_gpu_md_sq.py: its record buffers
are 2.5 TB that no device has, and `ta_md_run` allocates them before it enqueues anything."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import md_flux_reference as ref
from tests.helpers import fcc, golden_setfl, make_eam, make_grap_nn, make_nn
from tests.test_gpu_md import DT, WANT, _masses, _velocities
from tests.test_gpu_sf import _alloy
from tensoralloy_amd import Atoms, md

pytestmark = pytest.mark.gpu

KT0, TAU = md.kB * 600.0, 20 * DT
SETUPS = {
    "nve": lambda eng: None,
    "berendsen": lambda eng: eng.md_set_thermostat(KT0, TAU),
    "langevin": lambda eng: eng.md_set_langevin(KT0, 0.01 / md.fs, 0x9E3779B97F4A7C15),
    "nhc": lambda eng: eng.md_set_nose_hoover(KT0, TAU, chain=3),
}
GROUPS = (("J_conv", slice(0, 3)), ("J_pot", slice(3, 6)), ("K", slice(6, 12)), ("W", slice(12, 18)))


def _chain(flux, nnl_max):
    per_pass = -(-max(nnl_max, 1) // flux["lanes"]) + 1
    return (flux["chunk"] // 16) * per_pass + 6 + 4 + flux["blocks_per_frame"]


def _compare(label, got, want, chain):
    """One row against its reference: prints the largest error / bound per part of the row, asserts both bounds."""
    bound = ref.bound(want, chain)
    gap = np.abs(np.asarray(got) - want["row"])
    worst = 0.0
    for name, part in GROUPS:
        has = bound[part] > 0.0
        ratio = float((gap[part][has] / bound[part][has]).max()) if has.any() else 0.0
        worst = max(worst, ratio)
        print(f"{label} {name}: largest error / bound {ratio:.3e} (largest error {float(gap[part].max()):.3e}, "
              f"sum |terms| {float(want['terms'][part].max()):.3e})")
    assert np.all(gap <= bound), (label, gap / np.where(bound > 0.0, bound, 1.0))
    assert np.all(gap <= 1e-9 * want["terms"]), label   # no fp32 slip
    return worst


def _slices(frames):
    at = np.concatenate([[0], np.cumsum([len(a) for a in frames])])
    return [slice(int(at[f]), int(at[f + 1])) for f in range(len(frames))]


def _static_rows(nn, frames, v):
    """The row of every frame for the state (positions of `frames`, v): md_init + md_set_flux + md_run(0)."""
    from tensoralloy_amd import Engine
    with Engine(nn) as eng:
        eng.set_frames(list(frames))
        eng.md_init(None, v)
        eng.md_set_flux(1, 1)
        eng.md_run(0, DT)
        variant = eng.backward_variant()
        out, flux = eng.md_flux_rows(), eng.md_flux()
        assert (flux["n_samples"], flux["n_lags"], flux["last_step"], flux["first_step"]) == (1, 1, 0, 0)
        assert out["rows"].shape == (1, len(frames), 18) and out["steps"].tolist() == [0]
        assert np.array_equal(flux["sums"], out["rows"][0])
        return out["rows"][0], flux, int(eng.info.nnl_max), variant


def _reference_rows(nn, frames, x, v, how=None, h=ref.H):
    """The reference of every frame of the batch state (x, v): by the full matrix, or where `how[f]` says so by the
    cluster identity; `h` is the step of the finite differences."""
    m = _masses(frames)
    out = []
    for f, (atoms, s) in enumerate(zip(frames, _slices(frames))):
        evaluate = ref.oracle_for(nn, atoms)
        if how is not None and how[f] == "identity":
            out.append(ref.cluster_row(evaluate, x[s], v[s], m[s], h=h))
        else:
            out.append(ref.row_from_matrix(evaluate, x[s], v[s], m[s], np.asarray(atoms.get_cell(complete=True)), atoms.pbc,
                                           h=h))
    return out


# -- 1: static rows, one case per build that writes g -------------------------------------------------------------
def _ni32():
    return fcc(rep=(2, 2, 2), jitter=0.08, seed=3)


# The EAM family is piecewise: spline tables (cubic between knots 0.003 .. 0.02 A apart) and the Zjw04 embedding
# function (three branches in rho). A stencil of +-4 h that spans a knot sees a jump in the third derivative, which
# Richardson's extrapolation does not remove; at h = 1e-3 nearly every pair's stencil does, at 1e-4 few do, and the
# rounding of the differences (2^-53 e_j / h) is still below 1e-11. The reference's own self-checks (the oracle's
# analytic forces and virial) and its (h, 2h) / (2h, 4h) distance are what shows this; no device number enters.
STEP = {"eam_zjw04": 1e-4, "setfl": 1e-4, "adp": 1e-4, "eam_fs": 1e-4}


def _case(name, tmp_path):
    from tensoralloy_amd import UniversalTransformer
    from tensoralloy_amd.eam import AdpNN, EamAlloyNN, EamFsNN
    if name == "ni_g2_g4":
        return make_nn(["Ni"], 3.0, True, [16, 16], acut=3.0), _ni32()
    if name == "ni_g2":
        return make_nn(["Ni"], 3.0, False, [16, 16]), _ni32()
    if name == "nimo_g2_g4":
        return make_nn(["Mo", "Ni"], 3.0, True, [16, 16], acut=3.0), _alloy(["Ni", "Mo"], rep=(2, 2, 2))
    if name == "grap":
        return make_grap_nn(["Ni"], 3.0, [16, 16]), _ni32()
    if name == "eam_zjw04":
        return make_eam(["Ni"], 3.0, potential="zjw04"), _ni32()
    if name == "setfl":
        nn = EamAlloyNN.from_setfl(golden_setfl("Zhou_AlCu.alloy.eam", tmp_path))
        nn.attach_transformer(UniversalTransformer(["Al", "Cu"], rcut=3.0))
        return nn, _alloy(["Al", "Cu"], rep=(2, 2, 2), a=3.9)
    if name == "adp":
        return make_eam(["Mo", "Ni"], 3.0, adp=True), _alloy(["Ni", "Ni", "Mo"], rep=(2, 2, 2))
    if name == "eam_fs":
        nn = EamFsNN.from_setfl(golden_setfl("Mendelev_Al_Fe_thinned.fs.eam", tmp_path))
        nn.attach_transformer(UniversalTransformer(["Al", "Fe"], rcut=3.0, angular=False))
        return nn, _alloy(["Fe", "Fe", "Al"], rep=(2, 2, 2), a=3.7)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["ni_g2_g4", "ni_g2", "nimo_g2_g4", "grap", "eam_zjw04", "setfl", "adp", "eam_fs"])
def test_static_row_against_the_reference(lib, tmp_path, name):
    from tensoralloy_amd import Engine
    nn, atoms = _case(name, tmp_path)
    assert len(atoms) == 32 and np.asarray(atoms.get_cell(complete=True)).diagonal().min() > 6.0
    v = _velocities([atoms], 600.0, 5)
    rows, flux, nnl_max, variant = _static_rows(nn, [atoms], v)
    want = _reference_rows(nn, [atoms], atoms.positions, v, h=STEP.get(name, ref.H))[0]
    print(f"{name}: matrix against the oracle's forces {want['force_gap']:.3e}, W against its virial {want['virial_gap']:.3e}")
    assert want["force_gap"] < 1e-8 and want["virial_gap"] < 1e-7
    assert np.abs(want["row"][3:6]).max() > 1e-6 and np.abs(want["row"][12:18]).max() > 1e-3
    _compare(name, rows[0], want, _chain(flux, nnl_max))
    if name == "ni_g2_g4":   # the default dispatch is the triangle-once build; the sampled run took the per-apex one
        with Engine(nn) as eng:
            eng.evaluate([atoms])
            assert eng.backward_variant() == 2
        assert variant == 1


# -- 2: images ----------------------------------------------------------------------------------------------------
def test_images_of_one_atom_among_the_neighbours(lib):
    """The 4-atom fcc cell (3.524 A against a cutoff of 3.0: every neighbour is there as four images): its row times 8 is
    the row of its 2 x 2 x 2 replica with replicated velocities, which the reference checks."""
    nn = make_nn(["Ni"], 3.0, True, [16, 16], acut=3.0)
    small = fcc(rep=(1, 1, 1), jitter=0.06, seed=9)
    a = 3.524
    shifts = np.array([[i, j, k] for i in range(2) for j in range(2) for k in range(2)], dtype=np.float64) * a
    big = Atoms(symbols=["Ni"] * 32, positions=(small.positions[None] + shifts[:, None]).reshape(-1, 3),
                cell=np.eye(3) * 2 * a, pbc=True)
    v4 = _velocities([small], 600.0, 7)
    v32 = np.tile(v4, (8, 1))
    row4, flux4, nnl4, _ = _static_rows(nn, [small], v4)
    row32, flux32, nnl32, _ = _static_rows(nn, [big], v32)
    assert nnl4 == nnl32 == 12
    want = _reference_rows(nn, [big], big.positions, v32)[0]
    chain = _chain(flux32, nnl32)
    _compare("replica", row32[0], want, chain)
    _compare("8 x the 4-atom cell", 8.0 * row4[0], want, chain)
    assert np.abs(row4[0][3:6]).max() > 0.0


# -- 3: shape edges -----------------------------------------------------------------------------------------------
def _with_vacancies(atoms, n_keep, seed):
    keep = np.sort(np.random.RandomState(seed).permutation(len(atoms))[:n_keep])
    return Atoms(symbols=[atoms.get_chemical_symbols()[k] for k in keep], positions=atoms.positions[keep],
                 cell=np.asarray(atoms.get_cell(complete=True)), pbc=True)


def _sphere(n, r, seed):
    """A centre and n points spread over a sphere of radius r about it (a Fibonacci lattice, jittered)."""
    k = np.arange(n) + 0.5
    phi, z = np.pi * (1.0 + 5.0 ** 0.5) * k, 1.0 - 2.0 * k / n
    pts = r * np.stack([np.cos(phi) * np.sqrt(1.0 - z * z), np.sin(phi) * np.sqrt(1.0 - z * z), z], axis=1)
    pts += np.random.RandomState(seed).normal(0.0, 0.03, pts.shape)
    return np.concatenate([np.zeros((1, 3)), pts]) + 15.0


def test_shape_edges_in_one_batch(lib):
    """Frames of 29 and 23 atoms (no multiples of the 16 atoms of a workgroup), a free cluster with an atom that has
    no neighbour, a frame of one atom, and a compressed free cluster whose centre has 17 neighbours, one above the 16
    lanes of a centre (checked by the cluster identity)."""
    nn = make_nn(["Ni"], 3.0, True, [16, 16], acut=3.0)
    box = np.eye(3) * 30.0
    base = _ni32()
    near = np.argsort(np.linalg.norm(base.positions - base.positions.mean(axis=0), axis=1))[:13]
    lonely = Atoms(symbols=["Ni"] * 14, positions=np.concatenate([base.positions[near], [[20.0, 21.0, 22.0]]]), cell=box, pbc=False)
    one = Atoms(symbols=["Ni"], positions=[[0.4, 1.1, 2.3]], cell=np.diag([7.0, 7.2, 7.4]), pbc=True)
    dense = Atoms(symbols=["Ni"] * 18, positions=_sphere(17, 2.3, 4), cell=box, pbc=False)
    frames = [_with_vacancies(base, 29, 1), lonely, one, _with_vacancies(fcc(rep=(2, 2, 2), jitter=0.08, seed=11), 23, 2), dense]
    v = _velocities(frames, 600.0, 13)
    v[_slices(frames)[2]] = [0.011, -0.007, 0.004]   # (one atom with zero total momentum is at rest)
    x = np.concatenate([a.positions for a in frames])
    rows, flux, nnl_max, _ = _static_rows(nn, frames, v)
    d = np.linalg.norm(dense.positions[1:] - dense.positions[0], axis=1)
    assert np.all(d < 3.0) and nnl_max == 17 == flux["lanes"] + 1
    assert flux["chunk"] == 16 and flux["blocks_per_frame"] == 2
    want = _reference_rows(nn, frames, x, v, how=[None, None, None, None, "identity"])
    chain = _chain(flux, nnl_max)
    for f, w in enumerate(want):
        _compare(f"frame {f}", rows[f], w, chain)
    assert not rows[2][3:6].any() and not rows[2][12:18].any() and np.abs(rows[2][0:3]).max() > 0.0   # one atom: no pair
    assert np.abs(rows[4][3:6]).max() > 1e-6 and np.abs(rows[1][3:6]).max() > 1e-8


# -- 4 and 5: dynamics, cut runs, another skin -------------------------------------------------------------------------
STEPS, EVERY, LAGS = 24, 2, 4


@functools.lru_cache(maxsize=None)
def _model(name):
    """32 Ni atoms 0.02 A off the lattice, run at 300 K: no pair and no side of a triangle comes near the cutoff of 3.0
    (the shells are at 2.49, 3.52 and 4.32 A), where the cutoff function's second derivative jumps and no finite
    difference is good. `g2_g4`: the model of the static case, whose default build is triangle-once. `eam` (plain
    Zjw04: the exact list filtered from the skin list and the folded force kernel, unless the sampler runs) and `g2`:
    their evaluations have a fixed order of addition, so runs can be compared bit for bit. (The G2 + G4 evaluation is
    not reproducible to the last bit from run to run, with or without this sampler.)"""
    atoms = fcc(rep=(2, 2, 2), jitter=0.02, seed=3)
    if name == "g2_g4":
        return make_nn(["Ni"], 3.0, True, [16, 16], acut=3.0), atoms
    if name == "g2":
        return make_nn(["Ni"], 3.0, False, [16, 16]), atoms
    return make_eam(["Ni"], 3.0, potential="zjw04"), atoms


def _freeze(out):
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
        elif isinstance(a, dict):
            _freeze(a)
    return out


@functools.lru_cache(maxsize=None)
def _dynamics(model, integrator, cut, skin=0.3, flux=True, others=False):
    """24 steps on the 32-atom Ni frame, in calls of `EVERY` steps (`cut`) or in one: the final state, the records, the
    states behind every call, the newest row behind every call, and what the getters return at the end."""
    from tensoralloy_amd import Engine
    nn, atoms = _model(model)
    v0 = _velocities([atoms], 300.0, 3)
    with Engine(nn) as eng:
        eng.set_skin(skin)
        eng.set_frames([atoms])
        eng.md_init(None, v0)
        SETUPS[integrator](eng)
        if others:
            from tests.test_gpu_md_samplers_together import NAMES, SETTINGS
            for name in NAMES:
                getattr(eng, "md_set_" + name)(**SETTINGS[name])
        if flux:
            eng.md_set_flux(LAGS, EVERY)
        if flux == "off again":
            eng.md_set_flux(0)
        outs, states, vels, newest = [eng.md_run(0, DT)], [eng.md_state()[0]], [eng.md_state()[1]], []
        for n in ([EVERY] * (STEPS // EVERY) if cut else [STEPS]):
            if flux is True:
                newest.append(eng.md_flux_rows(1)["rows"][0])
            outs.append(eng.md_run(n, DT))
            states.append(eng.md_state()[0])
            vels.append(eng.md_state()[1])
        res = dict(x=states[-1], v=vels[-1], states=np.array(states), vels=np.array(vels),
                   epot=np.concatenate([o["epot"][1 if j else 0:] for j, o in enumerate(outs)]),
                   n_rebuilds=sum(o["n_rebuilds"] for o in outs), variant=eng.backward_variant(), nnl_max=int(eng.info.nnl_max),
                   kernel_list=eng.list_layout("kernel")["info"], resident_list=eng.list_layout("resident")["info"])
        if flux is True:
            newest.append(eng.md_flux_rows(1)["rows"][0])
            res.update(all_rows=np.array(newest), flux=eng.md_flux(), rows=eng.md_flux_rows())
    return _freeze(res)


@pytest.mark.parametrize("integrator", ["nve", "berendsen", "langevin", "nhc"])
def test_dynamics_against_the_reference(lib, integrator):
    nn, atoms = _model("g2_g4")
    dev = _dynamics("g2_g4", integrator, True)
    flux, held = dev["flux"], dev["rows"]
    S = STEPS // EVERY + 1
    assert (flux["n_samples"], flux["n_lags"], flux["sample_every"], flux["last_step"], flux["first_step"]) == (S, LAGS, EVERY, STEPS, 0)
    assert held["steps"].tolist() == [18, 20, 22, 24] and dev["all_rows"].shape == (S, 1, 18)
    assert np.array_equal(held["rows"], dev["all_rows"][-LAGS:])
    assert np.array_equal(flux["n_origins"], S - np.arange(LAGS)) and dev["variant"] == 1
    # rows: the oldest and the newest row held, against the reference on the states the samples were taken of
    chain = _chain(flux, dev["nnl_max"])
    for j in (-LAGS, -1):
        want = _reference_rows(nn, [atoms], dev["states"][j], dev["vels"][j])[0]
        _compare(f"{integrator} step {held['steps'][j]}", held["rows"][j][0], want, chain)
    # accumulators and sums: NumPy on the device's own rows, to the rounding of S additions of rounded products
    sums, a_heat, a_press, t_heat, t_press = ref.accumulate(dev["all_rows"], LAGS)
    eps = 2.0 ** -53
    for key, got, want, bound in (("sums", flux["sums"], sums, eps * S * np.abs(dev["all_rows"]).sum(axis=0)),
                                  ("a_heat", flux["a_heat"], a_heat, eps * (S + 4) * t_heat),
                                  ("a_press", flux["a_press"], a_press, eps * (S + 4) * t_press)):
        gap = np.abs(got - want).astype(np.float64)
        has = bound > 0.0
        print(f"{integrator} {key}: largest error / bound {float((gap[has] / bound[has]).max()):.3e}")
        assert np.all(gap <= bound), key
    assert np.abs(flux["a_heat"]).min() > 0.0 and np.abs(flux["a_press"]).min() > 0.0
    c = md.heat_current_acf(flux["a_heat"], flux["n_samples"])
    assert c.shape == (1, 3, LAGS) and np.all(c[:, :, 0] > 0.0)


def _same_flux(a, b):
    for key in ("sums", "a_heat", "a_press", "n_samples", "last_step", "first_step", "chunk", "blocks_per_frame"):
        assert np.array_equal(a["flux"][key], b["flux"][key]), key
    assert np.array_equal(a["rows"]["rows"], b["rows"]["rows"]) and np.array_equal(a["rows"]["steps"], b["rows"]["steps"])


@pytest.mark.parametrize("model, integrator", [("eam", "nve"), ("g2", "nve")])
def test_uncut_run_gives_the_bits_of_the_cut_run(lib, model, integrator):
    """(Under the Nose-Hoover chain a cut trajectory itself agrees with the uncut one to 1e-12, not bit for bit:
    tests/test_gpu_md_nhc.py.)"""
    cut, uncut = _dynamics(model, integrator, True), _dynamics(model, integrator, False)
    assert np.array_equal(uncut["x"], cut["x"]) and np.array_equal(uncut["v"], cut["v"])
    _same_flux(uncut, cut)
    assert np.abs(cut["flux"]["a_heat"]).sum() > 0.0


def test_another_skin_agrees_to_rounding_and_samples_every_due_step_once(lib):
    """A skin of 0.03: the list is rebuilt inside the windows of steps the loop enqueues ahead, the launches behind a
    stale list are enqueued again, and every due step is sampled exactly once. Plain EAM: the sampled run evaluates on
    the resident list itself, whose order of pairs is another one after every rebuild, so g and the trajectory move
    by rounding: the rows agree to 1e-9 of the largest entry of their part of the row over the run (2^-53, grown by
    the conditioning of 24 steps of a stable integrator, stays many orders below that)."""
    base, tight = _dynamics("eam", "nve", False), _dynamics("eam", "nve", False, skin=0.03)
    assert tight["n_rebuilds"] > base["n_rebuilds"] and tight["n_rebuilds"] > 2
    assert tight["flux"]["n_samples"] == base["flux"]["n_samples"] == STEPS // EVERY + 1
    assert np.array_equal(tight["rows"]["steps"], base["rows"]["steps"])
    cut = _dynamics("eam", "nve", True, skin=0.03)   # (the same skin: bit for bit again, and every row of the run)
    _same_flux(cut, tight)
    ref_rows = _dynamics("eam", "nve", True)["all_rows"]
    for name, part in GROUPS:
        scale = np.abs(ref_rows[..., part]).max()
        gap = np.abs(cut["all_rows"][..., part] - ref_rows[..., part]).max()
        print(f"skin 0.03 against 0.3, {name}: largest difference {gap:.3e} of {scale:.3e}")
        assert gap <= 1e-9 * scale, name
    for key in ("sums", "a_heat", "a_press"):
        assert np.allclose(tight["flux"][key], base["flux"][key], rtol=1e-8, atol=0.0), key


# -- 6: on and off ------------------------------------------------------------------------------------------------
def test_set_and_switched_off_again_is_never_set(lib):
    never, off = _dynamics("eam", "nve", False, flux=False), _dynamics("eam", "nve", False, flux="off again")
    for key in ("x", "v", "epot", "states", "vels"):
        assert np.array_equal(never[key], off[key]), key
    assert never["kernel_list"] == off["kernel_list"]


@pytest.mark.parametrize("model", ["g2_g4", "eam"])
def test_the_sampled_run_agrees_with_the_unsampled_one_to_rounding(lib, model):
    """The per-apex build instead of the triangle-once one, the pair kernel and the force gather on the resident list
    instead of the folded force kernel on the exact one: another order of the same sums."""
    never, on = _dynamics(model, "nve", False, flux=False), _dynamics(model, "nve", False)
    if model == "g2_g4":
        assert on["variant"] == 1 and never["variant"] == 2
    # behind the run the evaluations of other calls take their usual builds and list again
    assert on["kernel_list"] == never["kernel_list"] and on["resident_list"] == never["resident_list"]
    gap = np.abs(on["epot"] - never["epot"]).max()
    print(model, "epot of the sampled run against the unsampled one:", gap, "of", np.abs(never["epot"]).max())
    assert gap <= 1e-11 * np.abs(never["epot"]).max()
    assert np.abs(on["x"] - never["x"]).max() <= 1e-11 and np.abs(on["v"] - never["v"]).max() <= 1e-11


def test_beside_all_seven_other_samplers(lib):
    alone, beside = _dynamics("eam", "nve", True, skin=0.1), _dynamics("eam", "nve", True, skin=0.1, others=True)
    for key in ("x", "v", "epot"):
        assert np.array_equal(alone[key], beside[key]), key
    _same_flux(alone, beside)
    assert np.array_equal(alone["all_rows"], beside["all_rows"])


# -- 7: refusals and life cycle ---------------------------------------------------------------------------------------
def test_life_cycle_and_refusals(lib):
    from tensoralloy_amd import Engine, _lib
    nn, atoms = _model("g2_g4")
    v0 = _velocities([atoms], 300.0, 3)
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        with pytest.raises(ValueError, match="no resident batch"):
            eng.md_flux()
        eng.md_set_flux(0)   # off is always allowed
        with pytest.raises(ValueError, match="ta_md_set_flux: no resident batch"):
            eng.md_set_flux(4)
        eng.set_frames([atoms])
        with pytest.raises(ValueError, match="ta_md_get_flux called before ta_md_init"):
            eng.md_flux()
        with pytest.raises(ValueError, match="ta_md_set_flux called before ta_md_init"):
            eng.md_set_flux(4)
        eng.md_init(None, v0)
        with pytest.raises(ValueError, match=r"ta_md_get_flux: the heat current and pressure tensor are off \(ta_md_set_flux\)"):
            eng.md_flux()
        with pytest.raises(ValueError, match=r"ta_md_get_flux_rows: the heat current and pressure tensor are off \(ta_md_set_flux\)"):
            eng.md_flux_rows()
        eng.md_set_flux(4, 2)
        assert eng.md_flux_lags == 4
        for what, args in (("n_lags", (-1, 1)), ("n_lags", (4097, 1)), ("sample_every", (1, 0)), ("sample_every", (1, -2))):
            with pytest.raises(ValueError, match="ta_md_set_flux: " + what):
                eng.md_set_flux(*args)
        out = eng.md_flux()   # a refused call left the setting as it was
        assert out["a_heat"].shape == (1, 4, 3) and out["a_press"].shape == (1, 4, 6) and not out["sums"].any()
        assert (out["n_samples"], out["n_lags"], out["sample_every"], out["last_step"], out["first_step"]) == (0, 4, 2, -1, -1)
        with pytest.raises(ValueError, match=r"first_lag \+ n = 1 exceeds the 0 rows held"):
            eng.md_flux_rows(1)
        res = eng.md_run(10, DT)
        assert set(res) == {"epot", "ekin", "n_rebuilds"}   # the result dict is unchanged
        assert (eng.md_flux()["n_samples"], eng.md_flux()["last_step"]) == (6, 10)
        assert eng.md_flux_rows()["rows"].shape == (4, 1, 18) and eng.md_flux_rows(2)["steps"].tolist() == [8, 10]
        with pytest.raises(ValueError, match=r"first_lag \+ n = 5 exceeds the 4 rows held"):
            eng.md_flux_rows(5)
        # the barostat and this sampler together: refused by the run, both named, nothing lost
        x0, v_before = eng.md_state()
        before = eng.md_flux()
        eng.md_set_barostat(0.0, 100 * DT, 1.0)
        with pytest.raises(ValueError, match=r"ta_md_run: the heat current and pressure tensor \(ta_md_set_flux\) and the barostat "
                                             r"\(ta_md_set_barostat\) are both on; normalising the correlations needs one volume"):
            eng.md_run(5, DT)
        eng.md_set_barostat(0.0, 0.0, 0.0)
        x1, v1 = eng.md_state()
        after = eng.md_flux()
        assert np.array_equal(x0, x1) and np.array_equal(v_before, v1)
        assert np.array_equal(before["a_heat"], after["a_heat"]) and after["n_samples"] == 6
        eng.md_run(2, DT)   # after the refusal the loop still runs: step 12
        assert (eng.md_flux()["n_samples"], eng.md_flux()["last_step"]) == (7, 12)
        # setting it again zeroes; sample 0 is then the first multiple of sample_every not behind the step
        eng.md_run(1, DT)   # step 13
        eng.md_set_flux(1, 3)
        out = eng.md_flux()
        assert out["a_heat"].shape == (1, 1, 3) and out["n_samples"] == 0 and not out["a_heat"].any()
        eng.md_run(5, DT)   # steps 14 .. 18: samples at 15 and 18
        out = eng.md_flux()
        assert (out["n_samples"], out["last_step"], out["first_step"]) == (2, 18, 15)
        # set_frames keeps the setting and drops the data with the MD state; md_init starts from zero sums
        eng.set_frames([atoms])
        with pytest.raises(ValueError, match="ta_md_get_flux called before ta_md_init"):
            eng.md_flux()
        eng.md_init(None, v0)
        out = eng.md_flux()
        assert out["a_heat"].shape == (1, 1, 3) and not out["a_heat"].any() and not out["sums"].any()
        assert (out["n_samples"], out["sample_every"], out["last_step"]) == (0, 3, -1)
        eng.md_run(3, DT)
        assert (eng.md_flux()["n_samples"], eng.md_flux()["last_step"]) == (2, 3)
        # through the C ABI, past the Python layer
        for p, text in ((_lib.MdFluxParams(4097, 1), "n_lags must be 0 .. 4096"), (_lib.MdFluxParams(2, 0), "sample_every must be >= 1")):
            assert eng._lib.ta_md_set_flux(eng._handle, C.byref(p)) == _lib.TA_ERR_INVALID
            assert "ta_md_set_flux: " + text in eng._lib.ta_last_error(eng._handle).decode()
        eng.md_set_flux(0)
        assert eng.md_flux_lags == 0
        eng.md_set_barostat(0.0, 100 * DT, 1.0)   # with the feature off the barostat runs
        eng.md_run(2, DT)


def test_getters_after_a_failed_run(lib):
    """A run that fails leaves the data invalid until `md_set_flux` or `md_init` is called again. The failure:
    n_steps = 2^31 - 1 with a record of 128 frames at every step asks for 2.5 TB of `epot` records, which `ta_md_run`
    allocates first, behind the point where it marks the data invalid; nothing is launched."""
    from tensoralloy_amd import Engine, _lib
    nn, atoms = _model("eam")
    frames = [atoms] * 128
    v0 = np.tile(_velocities([atoms], 300.0, 3), (128, 1))
    null = C.POINTER(C.c_double)()

    def failing_run(eng):
        x0, v_before = eng.md_state()
        rc = eng._lib.ta_md_run(eng._handle, 2 ** 31 - 1, DT, WANT, 1, null, null, None)
        msg = eng._lib.ta_last_error(eng._handle).decode()
        print("failed run:", rc, msg)
        assert rc in (_lib.TA_ERR_HIP, _lib.TA_ERR_NOMEM) and "hipMalloc" in msg
        x1, v1 = eng.md_state()
        assert np.array_equal(x0, x1) and np.array_equal(v_before, v1)

    refusal = r"ta_md_get_flux%s: a ta_md_run failed and left the data invalid; call ta_md_set_flux or ta_md_init again"
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        eng.set_frames(frames)
        eng.md_init(None, v0)
        eng.md_set_flux(2, 1)
        eng.md_run(2, DT)
        assert eng.md_flux()["n_samples"] == 3
        failing_run(eng)
        with pytest.raises(ValueError, match=refusal % ""):
            eng.md_flux()
        with pytest.raises(ValueError, match=refusal % "_rows"):
            eng.md_flux_rows()
        eng.md_run(1, DT)   # the loop goes on (step 3) and samples nothing; the getters still refuse
        with pytest.raises(ValueError, match=refusal % ""):
            eng.md_flux()
        assert eng.list_layout("kernel")["info"]["filtered"]   # ... and its evaluations run on the exact list again
        eng.md_set_flux(2, 1)   # set again: zero sums, sample 0 is the state of step 3
        out = eng.md_flux()
        assert (out["n_samples"], out["last_step"]) == (0, -1) and not out["a_heat"].any()
        eng.md_run(2, DT)
        out = eng.md_flux()
        assert (out["n_samples"], out["last_step"], out["first_step"]) == (3, 5, 3)
        assert np.abs(out["a_heat"][0]).sum() > 0 and np.array_equal(out["a_heat"][127], out["a_heat"][0])
        failing_run(eng)
        eng.md_init(None, v0)   # ... or md_init: the setting is kept, the sums start from zero
        out = eng.md_flux()
        assert (out["n_samples"], out["sample_every"], out["last_step"]) == (0, 1, -1) and not out["a_heat"].any()
        eng.md_run(1, DT)
        assert eng.md_flux()["n_samples"] == 2


def test_device_md_end_to_end(lib):
    from tensoralloy_amd import Engine
    nn, atoms = _model("g2_g4")
    atoms = atoms.copy()
    v0 = _velocities([atoms], 600.0, 3)
    with Engine(nn) as eng:
        dyn = md.DeviceMD(eng, atoms, DT, velocities=v0, temperature_K=600.0, tdamp=20 * DT, flux_lags=4, flux_every=2)
        dyn.run(6)
        dyn.run(5)
        out = eng.md_flux()
        assert (out["n_samples"], out["last_step"], out["n_lags"]) == (6, 10, 4)
        t, c = dyn.get_heat_current_acf()
        assert np.array_equal(t, np.arange(4) * 2 * DT) and c.shape == (3, 4) and np.all(c[:, 0] > 0.0)
        t, p = dyn.get_pressure_acf()
        assert p.shape == (6, 4) and np.all(p[:, 0] >= 0.0)   # a variance
        kappa = md.green_kubo_thermal_conductivity(c, dyn.get_volume(), 600.0, 2 * DT)
        eta = md.green_kubo_viscosity(p, dyn.get_volume(), 600.0, 2 * DT)
        assert kappa.shape == (3, 4) and eta.shape == (3, 4) and np.all(np.isfinite(kappa)) and np.all(np.isfinite(eta))
        plain = md.DeviceMD(eng, atoms, DT, velocities=v0)   # flux_lags None: the sampler is set off
        assert eng.md_flux_lags == 0
        with pytest.raises(ValueError, match=r"heat current is off \(flux_lags\)"):
            plain.get_heat_current_acf()
        with pytest.raises(ValueError, match=r"are off \(ta_md_set_flux\)"):
            eng.md_flux()
