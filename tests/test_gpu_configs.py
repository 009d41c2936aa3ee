"""GPU: every single-GPU configuration of BASELINE.json at its FULL size, against the CPU oracle
(tolerances of north_star: 1e-6 eV total energy, 1e-5 eV/A per force component).

  C1  snap_Ni_id11.extxyz, G2-only rc = 6.0, one hidden layer, energy only, through the calculator
  C2  4000-atom Ni, G2 + G4 rc = 6.5, MLP 2 x 64, energy + forces + virial
  C3  Ni4Mo (mp-11507) 7 x 7 x 8 = 3920 atoms, cross-element G2 / G4 (D = 20), MLP 2 x 128
  C4  EAM (zjw04) rc = 6.0 / 6.5 and ADP (zjw04 + mishinh) for the 4000-atom Ni frame
(C5, the 512-frame batch over 8 GPUs, needs 8 GPUs: bench.py `config5`; its 2-rank rehearsal is
tests/test_gpu_parallel.py.)
"""
import os

import numpy as np
import pytest

from tests.helpers import make_eam, make_nn, nimo_supercell, oracle_eam_eval, oracle_eval

pytestmark = pytest.mark.gpu

E_TOL, F_TOL, W_TOL = 1e-6, 1e-5, 1e-5
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _c_oracle(nn, atoms):
    from bench import host_cores
    from oracle import csf
    from tests.helpers import oracle_model
    m = oracle_model(nn)
    return csf.run(m, csf.prepare(m, atoms.get_chemical_symbols(), atoms.positions,
                                  np.asarray(atoms.get_cell(complete=True)), atoms.pbc),
                   True, host_cores())


def _check(res, ref, n):
    assert abs(res["energy"] - ref["energy"]) < E_TOL
    assert np.abs(res["atomic"] - ref["atomic"]).max() < E_TOL
    assert np.abs(res["forces"] - ref["forces"]).max() < F_TOL
    assert np.abs(res["virial"] - ref["virial"]).max() < W_TOL
    assert res["forces"].shape == (n, 3)


def test_c1_snap_ni_radial_energy_only_through_the_calculator(lib, tmp_path):
    from tensoralloy_amd import TensorAlloyCalculator
    from tensoralloy_amd.io import read_extxyz
    atoms = read_extxyz(os.path.join(GOLDEN, "snap_Ni_id11.extxyz"))[0]
    assert len(atoms) == 6 and all(atoms.pbc)
    # Defaults of the reference (utils.py:400-406): eta {0.05, 4, 20, 80}, omega {0}, cosine cutoff
    nn = make_nn(["Ni"], 6.0, False, [64], activation="softplus")
    assert nn.ndim() == 4
    stem = str(tmp_path / "Ni_c1")
    nn.export(stem)
    calc = TensorAlloyCalculator(stem + ".json")
    e = calc.get_potential_energy(atoms)
    ref = oracle_eval(nn, atoms, want_forces=False)
    assert abs(e - ref["energy"]) < E_TOL
    assert set(calc.results) == {"energy"}           # energy only: nothing else was asked for
    per_atom = calc.get_atomic(atoms)
    assert np.abs(per_atom - ref["atomic"]).max() < E_TOL
    # the same through the exact-list engine path (skin 0) and the debug descriptors
    calc.skin = 0.0
    calc.calculate(atoms, ["energy"], debug_mode=True)
    assert abs(calc.results["energy"] - ref["energy"]) < E_TOL
    assert np.abs(calc.results["descriptors"] - ref["descriptors"]).max() < 1e-10


def test_c2_ni_4000_full_size(lib):
    from bench import ni_frame, ni_model
    from tensoralloy_amd import Engine
    nn, atoms = ni_model(), ni_frame(611)
    with Engine(nn) as eng:
        res = eng.evaluate([atoms])[0]
        assert int(eng.info.n_atoms) == 4000 and bool(eng.info.nl_on_device)
    _check(res, _c_oracle(nn, atoms), 4000)


def test_c3_ni4mo_3920_full_size(lib):
    from tensoralloy_amd import Engine
    nn = make_nn(["Ni", "Mo"], 6.5, True, [128, 128])
    assert nn.ndim() == 20
    with Engine(nn) as eng:
        # the perfect lattice pins the structure itself: SURVEY 8(d) computed 86 neighbours per
        # atom at rc = 6.5, P = 337 120, T = 14 327 600 for this cell
        info = eng.set_frames([nimo_supercell(jitter=0.0)])
        assert (int(info.n_atoms), int(info.n_pairs), int(info.n_triples)) == (3920, 337120, 14327600)
        atoms = nimo_supercell()
        res = eng.evaluate([atoms])[0]
    assert sorted(set(atoms.get_chemical_symbols())) == ["Mo", "Ni"]
    _check(res, _c_oracle(nn, atoms), 3920)


@pytest.mark.parametrize("rc,adp", [(6.0, False), (6.5, False), (6.5, True)])
def test_c4_eam_adp_4000_full_size(lib, rc, adp):
    from bench import ni_frame
    from tensoralloy_amd import Engine
    nn, atoms = make_eam(["Ni"], rc, adp=adp), ni_frame(611)
    with Engine(nn) as eng:
        res = eng.evaluate([atoms])[0]
    _check(res, oracle_eam_eval(nn, atoms), 4000)


def test_c5_per_gpu_share_64_frames(lib):
    """C5's per-GPU share at full size: 64 distinct 4000-atom Ni frames (seeds and jitter differ, so a frame
    offset bug shows), default G2 + G4 model (rc 6.5, 2 x 64), every frame against the C oracle."""
    from bench import ni_frame, ni_model
    from tensoralloy_amd import Engine
    from tests.test_gpu_sf_dispatch import check
    nn = ni_model()
    frames = [ni_frame(5000 + k, jitter=0.03 + 0.0005 * k) for k in range(64)]
    with Engine(nn) as eng:
        res = eng.evaluate(frames)
        assert int(eng.info.n_atoms) == 64 * 4000 and int(eng.info.nnl_max) <= 192
    energies = []
    for k, (atoms, r) in enumerate(zip(frames, res)):
        ref = _c_oracle(nn, atoms)
        _check(r, ref, 4000)
        check(r, ref, f"c5/frame{k}", descriptors=False)
        energies.append(r["energy"])
    assert len(set(energies)) == 64


def test_uneven_binary_batch_above_16384_atoms(lib):
    """~20 binary frames of uneven sizes (none a multiple of 16), more than 16384 atoms in all: the
    16-lane force gather, the one-wavefront MLP kernel chosen by itself (1024+ tiles) and groups of 16
    atoms that straddle frame boundaries, at scale."""
    from tensoralloy_amd import Atoms, Engine
    from tests.test_gpu_sf_dispatch import check
    nn = make_nn(["Mo", "Ni"], 6.5, True, [64, 64])
    frames = []
    for k in range(20):
        rep = [(6, 6, 6), (5, 6, 7), (7, 6, 5), (6, 5, 7)][k % 4]
        a = 3.52 + 0.01 * (k % 5)
        base = np.array([[0, 0, 0], [.5, .5, 0], [.5, 0, .5], [0, .5, .5]]) * a
        g = np.stack(np.meshgrid(*[np.arange(n) for n in rep], indexing="ij"), axis=-1).reshape(-1, 1, 3) * a
        pts = (g + base[None]).reshape(-1, 3)[: -(2 * k + 1)]      # an odd number of atoms
        rng = np.random.RandomState(700 + k)
        pts = pts + rng.normal(0.0, 0.04 + 0.002 * k, pts.shape)
        syms = np.where(rng.rand(len(pts)) < 0.2 + 0.02 * k, "Mo", "Ni").tolist()
        frames.append(Atoms(symbols=syms, positions=pts, cell=np.diag(np.array(rep) * a), pbc=True))
    n = sum(len(f) for f in frames)
    assert n > 16384 and all(len(f) % 16 for f in frames)
    with Engine(nn) as eng:
        res = eng.evaluate(frames)
        assert int(eng.info.n_atoms) == n
    for k, (atoms, r) in enumerate(zip(frames, res)):
        ref = _c_oracle(nn, atoms)
        _check(r, ref, len(atoms))
        check(r, ref, f"uneven/frame{k}", descriptors=False)
