"""GPU: the temperature-dependent head (csrc/ta_td.hip) through the engine and the calculator, against
tests/td_reference.py (the oracle's descriptor chain with the TD head in place of the MLP)."""
import numpy as np
import pytest

from tensoralloy_amd import Engine, _lib
from tensoralloy_amd.td import TemperatureDependentAtomicNN
from tests.helpers import fcc, hcp, make_grap_nn, make_nn
from tests.td_reference import oracle_td_eval, td_head

pytestmark = pytest.mark.gpu

ALL = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES | _lib.TA_WANT_VIRIAL | _lib.TA_WANT_ATOMIC


def td_from(base, layers, hidden, algo="default", resnet=False, minmax=False, act_h="softplus",
            activation="softplus", seed=7, static=None, export=("energy", "forces", "stress")):
    """A TD model on the descriptor and transformer of the plain model `base`."""
    nn = TemperatureDependentAtomicNN(base.elements, base.descriptor, hidden_sizes=list(hidden),
                                      activation=activation, minmax_scale=minmax, use_resnet_dt=resnet,
                                      atomic_static_energy=static or {},
                                      export_properties=export,
                                      finite_temperature={"activation": act_h, "layers": list(layers),
                                                          "algo": algo})
    nn.attach_transformer(base.transformer)
    nn.initialize(seed=seed, bias_scale=0.1)
    if minmax:
        rng = np.random.RandomState(seed + 1)
        D = nn.ndim()
        for el in nn.elements:
            nn.minmax[el] = (rng.rand(D) * 0.1, 1.0 + rng.rand(D) * 5.0)
    return nn


def binary(atoms, other="Mo", every=3):
    syms = atoms.get_chemical_symbols()
    return atoms.__class__(symbols=[other if k % every == 0 else s for k, s in enumerate(syms)],
                           positions=atoms.positions, cell=atoms.get_cell(complete=True), pbc=atoms.pbc)


def assert_close(r, o, what=""):
    E = o["energy"]
    assert abs(r["free_energy"] - E) <= 1e-9 * max(1.0, abs(E)), (what, r["free_energy"], E)
    assert abs(r["energy"] - o["U"]) <= 1e-9 * max(1.0, abs(o["U"])), (what, r["energy"], o["U"])
    assert abs(r["eentropy"] - o["S"]) <= 1e-9 * max(1.0, abs(o["S"])), (what, r["eentropy"], o["S"])
    fmax = max(1.0, np.abs(o["forces"]).max())
    assert np.abs(r["forces"] - o["forces"]).max() <= 1e-9 * fmax, what
    wmax = max(1.0, np.abs(o["virial"]).max())
    assert np.abs(r["virial"] - o["virial"]).max() <= 1e-8 * wmax, what
    assert np.abs(r["free_energy_atomic"] - o["atomic"]).max() <= 1e-9 * max(1.0, np.abs(o["atomic"]).max())
    assert np.abs(r["atomic"] - o["U_atomic"]).max() <= 1e-9 * max(1.0, np.abs(o["U_atomic"]).max())
    assert np.abs(r["eentropy_atomic"] - o["S_atomic"]).max() <= 1e-9 * max(1.0, np.abs(o["S_atomic"]).max())
    # the totals are the sums of the per-atom values
    assert abs(r["energy"] - r["atomic"].sum()) <= 1e-12 * max(1.0, abs(r["energy"]))
    assert abs(r["eentropy"] - r["eentropy_atomic"].sum()) <= 1e-12 * max(1.0, abs(r["eentropy"]))


def _sf(elements, **kw):
    return make_nn(elements, 5.0, True, [16], sf_kwargs={"eta": [0.1, 1.0], "omega": [0.0],
                                                         "beta": [0.005], "gamma": [1.0, -1.0],
                                                         "zeta": [1.0, 4.0]})


def _grap(elements, algorithm):
    params = {"sf": {"eta": [0.1, 0.5, 1.0], "omega": [0.0, 1.5, 3.0]}}.get(algorithm)
    return make_grap_nn(elements, 5.0, [16], algorithm=algorithm, parameters=params, moment_tensors=(0, 1, 2))


# (id, descriptor, elements, algo, resnet, minmax, H layers, U/S hidden, T)
ROWS = [
    ("sf-1el-odd", "sf", ["Ni"], "default", False, False, (20, 37), (30,), 0.3),
    ("sf-1el-default-T0", "sf", ["Ni"], "Sommerfeld", True, False, (128, 128), (64, 64), 0.0),
    ("sf-2el-somm-resnet-minmax", "sf", ["Mo", "Ni"], "Sommerfeld", True, True, (40, 40, 24), (64, 64), 0.5),
    ("sf-2el-default-minmax", "sf", ["Mo", "Ni"], "default", False, True, (128, 128), (30,), 1.2),
    ("grap-pexp-1el", "pexp", ["Be"], "default", False, True, (20, 37), (30, 30), 0.2),
    ("grap-sf-2el-somm", "sf_grap", ["Be", "Mo"], "Sommerfeld", True, False, (128, 128), (64, 64), 1.0),
    ("grap-nn-1el-resnet", "nn", ["Be"], "default", True, True, (32, 32, 16), (30,), 0.4),
    ("grap-nn-1el-T0", "nn", ["Be"], "Sommerfeld", False, False, (20, 37), (30,), 0.0),
]


def _row_model(desc, elements, algo, resnet, minmax, layers, hidden):
    if desc == "sf":
        base = _sf(elements)
    else:
        base = _grap(elements, "sf" if desc == "sf_grap" else desc)
    return td_from(base, layers, hidden, algo=algo, resnet=resnet, minmax=minmax)


def _row_atoms(desc, elements, T):
    if desc == "sf":
        a = fcc("Ni", rep=(2, 2, 2))
    else:
        a = hcp("Be", rep=(2, 2, 2))
    if len(elements) == 2:
        a = binary(a, other="Mo")
    a.info["etemperature"] = T
    return a


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_td_rows_against_oracle(row, monkeypatch):
    _, desc, elements, algo, resnet, minmax, layers, hidden, T = row
    nn = _row_model(desc, elements, algo, resnet, minmax, layers, hidden)
    atoms = _row_atoms(desc, elements, T)
    with Engine(nn, device=0) as eng:
        r = eng.evaluate([atoms], want=ALL)[0]
    o = oracle_td_eval(nn, atoms, monkeypatch)
    assert_close(r, o, row[0])
    if T > 0.0:   # the temperature reaches the result
        o0 = oracle_td_eval(nn, atoms, monkeypatch, T=0.0)
        assert abs(o0["energy"] - o["energy"]) > 1e-6


def test_td_batch_with_different_temperatures(monkeypatch):
    """Each frame's T reaches its own atoms only; the 1-element tiles straddle frame boundaries."""
    nn = td_from(_sf(["Mo", "Ni"]), (20, 37), (30,), algo="Sommerfeld", minmax=True)
    frames = []
    for k, T in enumerate([0.0, 0.5, 2.0, 0.05]):
        a = binary(fcc("Ni", rep=(2, 2, 2) if k % 2 == 0 else (2, 2, 1), seed=10 + k), other="Mo", every=2 + k)
        a.info["etemperature"] = T
        frames.append(a)
    with Engine(nn, device=0) as eng:
        res = eng.evaluate(frames, want=ALL)
    for a, r in zip(frames, res):
        assert_close(r, oracle_td_eval(nn, a, monkeypatch), f"T={a.info['etemperature']}")


def test_td_md_path_keeps_and_resets_temperature(monkeypatch):
    nn = td_from(_grap(["Be"], "pexp"), (20, 37), (30,), algo="default", resnet=True)
    atoms = _row_atoms("pexp", ["Be"], 0.8)
    rng = np.random.RandomState(3)
    with Engine(nn, device=0) as eng:
        eng.set_skin(0.5)
        eng.set_frames([atoms])
        for step in range(3):   # list reuses (small moves) and a rebuild (large one)
            pos = atoms.positions + rng.normal(scale=0.02 if step < 2 else 0.4, size=atoms.positions.shape)
            moved = atoms.copy()
            moved.positions = pos
            moved.info["etemperature"] = 0.8
            if step == 1:
                r = eng.step(pos, ALL)
                r = {"free_energy": float(r["free_energy"][0]), "energy": float(r["energy"][0]),
                     "eentropy": float(r["eentropy"][0]), "forces": r["forces"], "virial": r["virial"][0],
                     "free_energy_atomic": r["free_energy_atomic"], "atomic": r["atomic"],
                     "eentropy_atomic": r["eentropy_atomic"]}
            else:
                eng.update_positions(pos)
                eng.compute(ALL)
                r = eng._per_frame(eng.fetch(ALL))[0]
            assert_close(r, oracle_td_eval(nn, moved, monkeypatch), f"step {step}")
        reuses = eng.list_stats()[1]
        assert reuses >= 1
        # ta_set_frames resets T to 0 (the engine's own call that sets it from `info` is suppressed)
        monkeypatch.setattr(Engine, "set_electron_temperatures", lambda self, T: None)
        eng.set_frames([atoms])
        eng.compute(ALL)
        r = eng._per_frame(eng.fetch(ALL))[0]
    assert_close(r, oracle_td_eval(nn, atoms, monkeypatch, T=0.0), "after set_frames")


def test_td_temperatures_refused_by_plain_model():
    nn = make_nn(["Ni"], 5.0, False, [16])
    with Engine(nn, device=0) as eng:
        eng.set_frames([fcc("Ni", rep=(1, 1, 1))])
        with pytest.raises(ValueError):
            eng.set_electron_temperatures([0.5])


def test_td_forces_are_minus_gradient_of_free_energy():
    nn = td_from(_sf(["Mo", "Ni"]), (20, 37), (30,), algo="Sommerfeld", resnet=True, minmax=True)
    atoms = binary(fcc("Ni", rep=(1, 1, 1), jitter=0.1), other="Mo", every=2)
    atoms.info["etemperature"] = 0.7
    d = 1e-5
    with Engine(nn, device=0) as eng:
        r = eng.evaluate([atoms], want=ALL)[0]
        frames = []
        for i in range(len(atoms)):
            for a in range(3):
                for sgn in (1.0, -1.0):
                    b = atoms.copy()
                    p = b.positions.copy()
                    p[i, a] += sgn * d
                    b.positions = p
                    frames.append(b)
        res = eng.evaluate(frames, want=_lib.TA_WANT_ENERGY)
    fd = np.array([-(res[2 * k]["free_energy"] - res[2 * k + 1]["free_energy"]) / (2 * d)
                   for k in range(3 * len(atoms))]).reshape(-1, 3)
    assert np.abs(fd - r["forces"]).max() < 1e-6 * max(1.0, np.abs(r["forces"]).max())


def test_td_be_fixture_through_calculator(tmp_path, monkeypatch):
    """Be liquid frames (geometry and T of the reference's labelled file; the labels are DFT values and are
    not compared) through the calculator: U, F, S, forces and stress against the oracle; elastic constants
    through the difference fallback."""
    from pathlib import Path
    from tensoralloy_amd import TensorAlloyCalculator
    from tensoralloy_amd.io import read_extxyz
    frames = read_extxyz(str(Path(__file__).parent / "golden" / "Be_liquid_4000K_TS.extxyz"))
    base = make_grap_nn(["Be"], 5.0, [64, 64], algorithm="sf",
                        parameters={"eta": [0.1, 0.5, 1.0, 2.0, 4.0, 8.0, 20.0, 40.0], "omega": [0.0, 1.5, 3.0]},
                        moment_tensors=(2,), param_space_method="cross")
    nn = td_from(base, (128, 128), (64, 64), resnet=True, minmax=False, static={"Be": -3.0},
                 export=("energy", "forces", "stress", "elastic"))
    path = nn.export_to_lammps_native(str(tmp_path / "be_td.npz"))
    calc = TensorAlloyCalculator(path)
    for atoms in frames[:2]:
        atoms.calc = calc
        o = oracle_td_eval(nn, atoms, monkeypatch)
        U, F, S = calc.get_potential_energy(atoms), calc.get_free_energy(atoms), calc.get_electron_entropy(atoms)
        assert abs(U - o["U"]) <= 1e-9 * max(1.0, abs(o["U"]))
        assert abs(F - o["energy"]) <= 1e-9 * max(1.0, abs(o["energy"]))
        assert abs(S - o["S"]) <= 1e-9 * max(1.0, abs(o["S"]))
        assert abs(F - (U - atoms.info["etemperature"] * S)) <= 1e-9 * max(1.0, abs(F))
        fmax = max(1.0, np.abs(o["forces"]).max())
        assert np.abs(calc.get_forces(atoms) - o["forces"]).max() <= 1e-9 * fmax
        assert np.abs(calc.get_stress(atoms) - o["stress_voigt"]).max() <= 1e-8 * max(1.0, np.abs(o["stress_voigt"]).max())
    # elastic constants need the op, which only the json + npz model file lists
    atoms = frames[0]
    atoms.calc = TensorAlloyCalculator(nn.export(str(tmp_path / "be_td.json")))
    C = atoms.calc.get_elastic_constant_tensor(atoms)
    assert C.shape == (6, 6) and np.all(np.isfinite(C))


def test_td_4000_atoms_against_c_oracle_descriptors():
    """One 4000-atom frame: U, S, F per atom against the head applied to the C oracle's descriptors."""
    from oracle import csf
    from tests.helpers import oracle_model
    base = make_nn(["Ni"], 5.0, True, [16])
    nn = td_from(base, (128, 128), (64, 64), algo="Sommerfeld", resnet=True, minmax=True)
    atoms = fcc("Ni", rep=(10, 10, 10))
    atoms.info["etemperature"] = 0.35
    with Engine(nn, device=0) as eng:
        r = eng.evaluate([atoms], want=ALL)[0]
    G = csf.evaluate(oracle_model(base), atoms.get_chemical_symbols(), atoms.positions,
                     np.asarray(atoms.get_cell(complete=True)), atoms.pbc, want_forces=False)["descriptors"]
    h = td_head(nn, atoms.get_chemical_symbols(), G, np.full(len(atoms), 0.35))
    for key, ref in (("free_energy_atomic", h["F"]), ("atomic", h["U"]), ("eentropy_atomic", h["S"])):
        assert np.abs(r[key] - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max()), key
    assert abs(r["free_energy"] - h["F"].sum()) <= 1e-9 * max(1.0, abs(h["F"].sum()))


# -- the act' slab of td_all_kernel in the global scratch slab; ragged and empty tiles; the LDS refusal ------------

TD_LDS_LIMIT = 150 * 1024       # kTdLdsLimit


def td_plan_mirror(nn, da_global=False):
    """td_plan (ta_td.hip) restated: dynamic LDS bytes, where act' lives, threads, doubles of act' per tile."""
    pad = lambda n: (n + 15) // 16 * 16
    w = wz = dah = dan = widest = 0
    for el in nn.elements:
        sizes = nn.layer_sizes(el)
        H = [pad(s) for s in sizes["H"]]
        w, widest = max([w] + H), max([widest] + H[1:])
        dah = max(dah, sum(16 * (n + 2) for n in H[1:-1]))          # one [16][np + 2] block per hidden layer
        for net in ("U", "S"):
            N = [pad(s) for s in sizes[net]]
            wz, w, widest = max(wz, N[0]), max([w] + N[1:]), max([widest] + N[1:])
            dan = max(dan, sum(16 * (n + 2) for n in N[1:-1]))      # U and S share one region
    base = 2 * 16 * (w + 2 + wz + 2) * 8
    with_da = base + (dah + dan) * 8
    in_lds = with_da <= TD_LDS_LIMIT and not da_global
    lds = with_da if in_lds else base
    return dict(lds_bytes=lds, da="lds" if in_lds else "global", threads=512 if widest >= 128 else 256,
                refused=lds > TD_LDS_LIMIT, da_tile=dah + dan, base=base, with_da=with_da)


# name: (H layers, U / S hidden, algo, resnet, minmax, TA_MLP_DA_GLOBAL, where act' must live, threads)
SLAB_ROWS = {
    "lds": ((20, 37), (30,), "default", False, True, False, "lds", 256),
    "global-forced": ((20, 37), (30,), "default", False, True, True, "global", 256),
    "global-by-itself": ((256, 256), (64, 64), "Sommerfeld", True, True, False, "global", 512),
}
TOO_WIDE = ((320, 320), (64, 64))


def slab_model(name):
    layers, hidden, algo, resnet, minmax = SLAB_ROWS[name][:5]
    return td_from(_sf(["Mo", "Ni"]), layers, hidden, algo=algo, resnet=resnet, minmax=minmax)


def slab_frames():
    """Mo 36 atoms (3 tiles, the last one of 4), Ni 92 (6 tiles, the last one of 12): Mo absent from the second
    frame, a single Mo atom in the third; every frame at its own temperature."""
    frames = [binary(fcc("Ni", rep=(2, 2, 2), seed=21), other="Mo", every=3),
              fcc("Ni", rep=(2, 2, 2), seed=22, jitter=0.07),
              binary(fcc("Ni", rep=(2, 2, 1), seed=23), other="Mo", every=16),
              binary(fcc("Ni", rep=(3, 2, 2), seed=24), other="Mo", every=2)]
    for a, T in zip(frames, (0.4, 1.1, 0.0, 0.25)):
        a.info["etemperature"] = T
    return frames


def slab_counts(frames):
    return [[a.get_chemical_symbols().count(el) for el in ("Mo", "Ni")] for a in frames]


_slab_reference = {}
SLAB_SEEN = {}      # row -> launch the engine reported (collected by test_gpu_mlp_dispatch.py)


def slab_launch(name, monkeypatch, frames, want=ALL):
    """Evaluate `frames` with a slab row's model under its switch: (results, reported launch), which must be the
    td build and act' placement the row names."""
    da_global, where, threads = SLAB_ROWS[name][5:]
    nn = slab_model(name)
    plan = td_plan_mirror(nn, da_global)
    assert (plan["da"], plan["threads"], plan["refused"]) == (where, threads, False), plan
    if da_global:
        monkeypatch.setenv("TA_MLP_DA_GLOBAL", "1")
    with Engine(nn, device=0) as eng:
        res = eng.evaluate(frames, want=want)
        launch = eng.mlp_launch()
    monkeypatch.delenv("TA_MLP_DA_GLOBAL", raising=False)
    tiles = sum(-(-sum(c[e] for c in slab_counts(frames)) // 16) for e in (0, 1))
    assert launch == dict(family="td", threads=threads, lh=0, nt=0, grid=(tiles, 1), lds_bytes=plan["lds_bytes"],
                          da=where), launch
    SLAB_SEEN[name] = launch
    return res, launch


def slab_reference(name, k, monkeypatch):
    """The oracle on frame k of slab_frames(), once per model (the two (20, 37) rows share theirs)."""
    key = (SLAB_ROWS[name][:5], k)
    if key not in _slab_reference:
        _slab_reference[key] = oracle_td_eval(slab_model(name), slab_frames()[k], monkeypatch)
    return _slab_reference[key]


@pytest.mark.parametrize("name", list(SLAB_ROWS))
def test_td_slab_rows_against_oracle(name, monkeypatch):
    """act' of H, then of U and S behind it, in LDS or in the global slab (`scratch + blockIdx.x * da_tile`,
    `da + da_h`), over nine tiles with ragged last tiles; the launch the engine reports is checked first."""
    res, launch = slab_launch(name, monkeypatch, slab_frames())
    assert launch["grid"] == (9, 1), launch
    for k, r in enumerate(res):
        assert_close(r, slab_reference(name, k, monkeypatch), f"{name}/frame{k}")


def test_td_too_wide_is_refused_then_a_valid_model(monkeypatch):
    """H (320, 320): 168,960 B without the act' slab, above the 150 KB a workgroup may ask for. Refused with a
    ValueError that names the limit; the process then evaluates a valid model correctly."""
    nn = td_from(_sf(["Mo", "Ni"]), TOO_WIDE[0], TOO_WIDE[1], algo="Sommerfeld", resnet=True, minmax=True)
    frames = slab_frames()
    assert td_plan_mirror(nn)["refused"]
    with Engine(nn, device=0) as eng:
        with pytest.raises(ValueError, match=r"too wide for the LDS tile: 168960 B .* limit 153600"):
            eng.evaluate(frames[:1], want=ALL)
    with Engine(slab_model("lds"), device=0) as eng:
        r = eng.evaluate(frames[:1], want=ALL)[0]
        assert eng.mlp_launch()["family"] == "td"
    assert_close(r, slab_reference("lds", 0, monkeypatch), "after the refusal")
