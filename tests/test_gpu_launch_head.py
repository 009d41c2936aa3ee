"""
The heads of the step's kernels, path by path, against the oracle.

The angular backward kernel takes a 64-byte `LaunchHead` (ta_device.h) as its first parameter, reads the run
header one argument round behind it and takes the model constants of its prologue from the head; the forward
kernel keeps its parameters. None of that may change a result. The inputs are the smallest that reach each
head path:

  batch2    a 108-atom and a 32-atom Ni cell in one batch (in that order): atoms 96..111 are a 16-atom group that
            both frames share, the last group holds 12 atoms; energy, forces and virial PER FRAME (frame sums,
            group partials)
  md        108 atoms, set_skin(0.5), two `step` calls: the device packer (blk_groups > 0, the division of the
            run slot) and unused run slots (ncent == 0); step 2 against the oracle at the moved positions. (The
            grid of these launches is exact: the library never sets `n_blk_dev`, so no test reaches that word.)
  mlp       a 33-atom cell (two full tiles and one atom): one, two and three hidden layers through the generic
            tile kernel (what runs below the quad threshold), the quad kernel (what runs above it) and the wave
            kernel, each chosen with the handle's kernel switch as tests/test_gpu_mlp_dispatch.py does; min-max
            scaling (xlo / xhi) on and off in each of the three; `use_resnet_dt` through the tile kernel, the only
            one that takes layers with a skip connection (the quad and wave forms refuse them, ta_mlp.hip)
  nimo64    64 atoms, 63 Ni and ONE Mo: the multi-element network kernels with a one-atom element and the
            NSPEC = 2 angular builds
  acut      acut = 4.0 < rcut = 4.5, and the zeta grid {1, 2}: the builds without a compile-time capacity or the
            default zeta grid, which keep the launch's workgroup size

Bounds are those of tests/test_gpu_block_header.py: descriptors to 1e-10, energies and forces to 1e-9 x max(1, |.|),
virial to 1e-8 x max(1, |.|). That the head is at most 64 bytes, trivially copyable and the first parameter is
asserted where it is compiled (ta_device.h, ta_kernels_v2.hip).
"""
import functools

import numpy as np
import pytest

from tests.helpers import ENV_SWITCHES, fcc, make_nn, oracle_eval, oracle_model
from tensoralloy_amd import Atoms

gpu = pytest.mark.gpu

RC = 4.5
G_TOL = 1e-10
E_REL, F_REL, W_REL = 1e-9, 1e-9, 1e-8


def c_oracle(nn, atoms):
    from bench import host_cores
    from oracle import csf
    m = oracle_model(nn)
    return csf.run(m, csf.prepare(m, atoms.get_chemical_symbols(), atoms.positions,
                                  np.asarray(atoms.get_cell(complete=True)), atoms.pbc), True, host_cores())


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


def ni108():
    # a = 3.18: the fourth shell sits at the cutoff, so the neighbour counts vary and the runs hold 3 or 4 centres
    return fcc(rep=(3, 3, 3), a=3.18, seed=7)


def ni32():
    return fcc(rep=(2, 2, 2), seed=2)


def ni33():
    """32 jittered fcc sites and one atom in an octahedral hole: three tiles of the per-atom network, the last with
    one atom."""
    a = ni32()
    pos = np.concatenate([a.positions, [[0.5 * 3.524, 0.0, 0.0]]])
    return Atoms(symbols=["Ni"] * 33, positions=pos, cell=np.asarray(a.get_cell()), pbc=True)


def nimo64():
    atoms = fcc(rep=(4, 2, 2), a=3.6, seed=9)
    syms = ["Ni"] * 64
    syms[37] = "Mo"
    return Atoms(symbols=syms, positions=atoms.positions, cell=np.asarray(atoms.get_cell()), pbc=True)


# -- batch edges ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def batch2():
    nn = make_nn(["Ni"], RC, True, [16, 16])
    frames = (ni108(), ni32())
    return nn, frames, tuple(c_oracle(nn, a) for a in frames)


def test_batch2_shares_a_group():
    """CPU: the second frame starts inside a 16-atom group and the batch ends with a short one."""
    n0, n1 = len(ni108()), len(ni32())
    assert n0 % 16 != 0 and (n0 + n1) % 16 != 0 and len(ni33()) == 33, (n0, n1)


@gpu
def test_batch_edges(lib):
    from tensoralloy_amd import Engine
    nn, frames, ref = batch2()
    with Engine(nn) as eng:
        res = eng.evaluate(list(frames), descriptors=True)
    assert len(res) == 2
    for k, (r, o) in enumerate(zip(res, ref)):
        check(r, o, f"batch2/frame{k}")


# -- MD step path -----------------------------------------------------------------------------------------------

@gpu
def test_md_step_path(lib):
    from tensoralloy_amd import Engine, _lib
    nn, atoms = batch2()[0], ni108()
    want = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES | _lib.TA_WANT_VIRIAL | _lib.TA_WANT_ATOMIC
    rng = np.random.RandomState(23)
    pos = atoms.positions.copy()
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        eng.set_frames([atoms])
        for _ in range(2):
            pos = pos + rng.uniform(-0.1, 0.1, pos.shape) / np.sqrt(3.0)   # every atom by up to 0.1 A
            got = {k: np.array(v) for k, v in eng.step(pos, want).items()}
        builds, reuses = eng.list_stats()
    assert builds == 1 and reuses == 2, (builds, reuses)    # both steps went through the device packer
    moved = Atoms(symbols=atoms.get_chemical_symbols(), positions=pos, cell=np.asarray(atoms.get_cell()), pbc=True)
    r = dict(energy=got["energy"][0], atomic=got["atomic"], forces=got["forces"], virial=got["virial"][0])
    check(r, c_oracle(nn, moved), "md/step2", descriptors=False)


# -- per-atom network: depths, kernel families, scaling, skip connections ---------------------------------------------

DEPTHS = {1: [48], 2: [64, 32], 3: [16, 32, 64]}
FAMILY_SWITCH = {"tile": "TA_MLP_TILE_KERNEL", "quad": "TA_MLP_QUAD_KERNEL", "wave": "TA_MLP_WAVE_KERNEL"}
MLP_CASES = [(f"{fam}-{d}", fam, DEPTHS[d], False, False) for fam in FAMILY_SWITCH for d in DEPTHS]
MLP_CASES += [("tile-minmax", "tile", DEPTHS[2], True, False), ("quad-minmax", "quad", DEPTHS[2], True, False),
              ("wave-minmax", "wave", DEPTHS[2], True, False), ("tile-resnet", "tile", [48, 48], False, True)]


@functools.lru_cache(maxsize=None)
def mlp_case(name):
    _, _, hidden, minmax, resnet = next(c for c in MLP_CASES if c[0] == name)
    nn = make_nn(["Ni"], RC, True, list(hidden), minmax=minmax, resnet=resnet)
    return nn, oracle_eval(nn, ni33())


@gpu
@pytest.mark.parametrize("name", [c[0] for c in MLP_CASES])
def test_mlp_heads(lib, monkeypatch, name):
    from tensoralloy_amd import Engine
    family = next(c[1] for c in MLP_CASES if c[0] == name)
    nn, ref = mlp_case(name)
    for env in ENV_SWITCHES:
        monkeypatch.delenv(env, raising=False)
    monkeypatch.setenv(FAMILY_SWITCH[family], "1")      # read when the handle is created
    with Engine(nn) as eng:
        (res,) = eng.evaluate([ni33()], descriptors=True)
        launch = eng.mlp_launch()
    monkeypatch.delenv(FAMILY_SWITCH[family])
    assert launch["family"] == family, (name, launch)
    check(res, ref, f"mlp/{name}")


# -- two elements -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def nimo_case():
    nn = make_nn(["Ni", "Mo"], RC, True, [16, 16])
    atoms = nimo64()
    return nn, atoms, c_oracle(nn, atoms)


def test_nimo64_has_one_mo():
    syms = nimo64().get_chemical_symbols()
    assert len(syms) == 64 and syms.count("Mo") == 1


@gpu
def test_two_elements(lib):
    from tensoralloy_amd import Engine
    nn, atoms, ref = nimo_case()
    with Engine(nn) as eng:
        (res,) = eng.evaluate([atoms], descriptors=True)
        launch = eng.mlp_launch()
    assert launch["family"].endswith("_all"), launch    # one launch for both elements
    check(res, ref, "nimo64")


# -- builds that keep the launch's workgroup size ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def generic_case(name):
    if name == "acut":
        nn = make_nn(["Ni"], RC, True, [16, 16], acut=4.0)
    else:
        nn = make_nn(["Ni"], RC, True, [16, 16], acut=4.0, sf_kwargs=dict(zeta=[1.0, 2.0]))
    atoms = ni108()
    return nn, atoms, c_oracle(nn, atoms)


@gpu
@pytest.mark.parametrize("triangles", [True, False], ids=["triangles", "per-apex"])
@pytest.mark.parametrize("name", ["acut", "acut-zeta12"])
def test_generic_builds(lib, name, triangles):
    from tensoralloy_amd import Engine
    nn, atoms, ref = generic_case(name)
    with Engine(nn) as eng:
        eng.set_triangles(triangles)
        (res,) = eng.evaluate([atoms], descriptors=True)
    check(res, ref, f"{name}/{'tri' if triangles else 'apex'}")
