"""GPU: the Martyna-Tobias-Klein barostat of the device MD loop (`ta_md_set_mtk_barostat`, csrc/ta_md_mtk.hip) against
the NumPy reference (tests/md_mtk_reference.py) driven by the CPU oracle or by a second engine's
`Engine.step(x, cells=h)`.

Parity bound `TOL` = 1e-9 of tests/test_gpu_md_npt.py, by its argument; the exponentials of the strain rates add a
few ulp per step. For omega, xi, vxi (and eta, veta) the bound is 1e-9 x max(1, max |reference|). Every comparison
first asserts on the reference log that no staleness decision is marginal (`md_npt_reference.assert_not_marginal`).

The anchor of tests/test_gpu_md_npt.py: 32 Ni atoms (fcc 2 x 2 x 2, jitter 0.02, seed 3), Zjw04, rc = 6, velocities
maxwell_boltzmann(kB 300, RandomState(3)), dt = 1 fs; Nose-Hoover chain at 300 K, tdamp = 20 fs, M = 3, L = 1; the
barostat's chain M_p = 3, L_p = 1 unless a test says otherwise. Figures of the reference with the oracle:
  A  cell and atoms scaled 1.02, P0 = 0, pdamp = 1000 fs, skin 0.5, 40 steps, isotropic: no rebuild (smallest lim
     0.1663, largest |u| 0.1394, nearest approach of the two 0.0269), cell edge from 7.189 by 0.1069 A, V from 371.53
     to 355.20 A^3, P from -0.05580 to -0.00605 eV / A^3, omega at the end -0.006049 per time unit
  B  scaled 1.03, pdamp = 300 fs, skin 0.3, 36 steps: rebuilds after the drifts of steps 11 (lim 0.0426, max |u|
     0.0595, plain displacement 0.2207) and 19 (0.0208, 0.0311, 0.2212), both by strain alone: |u| stays far below
     skin / 2 = 0.15. Launch 11 is enqueued behind the stale list of step 11 and returns early.
  C  mask (1, 0, 1), P0 = 5 GPa, scale 1.0, pdamp = 50 fs, 40 steps: no rebuild, cell edges from 7.048 to 6.9971 (x),
     7.048 (y, to the bit) and 7.0001 (z), V from 350.10 to 345.21
  physics (256 Ni, 300 K -> 900 K, P0 = 0, dt = 2 fs, tdamp = 50 fs, pdamp = 500 fs, 2000 steps): mean T of the second
     half 897.0 K, excursion of H' 0.02025 eV against 0.00709 eV of E in the NVE run of the same start: ratio 2.854,
     mean V of the second half 2914.9 A^3 (from 2800.8), mean P -0.0086 GPa
"""
import functools

import numpy as np
import pytest

from tests import md_mtk_reference as mtk
from tests import md_npt_reference as npt
from tests.helpers import fcc, make_eam, make_grap_nn, make_nn
from tests.test_gpu_md_nhc import _freeze
from tests.test_gpu_md_npt import (DT, RC, TOL, WANT, _anchor, _cells, _engine_forces, _masses, _natoms, _ni, _oracle_forces,
                                   _positions, _strained, _velocities)
from tests.test_gpu_sf import _alloy
from tensoralloy_amd import Atoms, md

pytestmark = pytest.mark.gpu

KT0, TDAMP = md.kB * 300.0, 20 * DT
KEYS = ("x", "v", "cells", "epot", "ekin", "echain", "ebaro", "volume", "press")
STATE = ("eta", "veta", "omega", "xi", "vxi")
CASES = {  # scale, P0, pdamp, skin, steps, mask
    "A": (1.02, 0.0, 1000 * DT, 0.5, 40, None),
    "B": (1.03, 0.0, 300 * DT, 0.3, 36, None),
    "C": (1.0, 5.0 * md.GPa, 50 * DT, 0.5, 40, (1, 0, 1)),
}


def _reference(force, frames, v0, steps, p0, pdamp, skin, mask=None, nhc=None, rc=RC, **kw):
    """`nhc`: chain, loops, dof_removed of the particle chain; `kw`: pchain, ploops and the state at entry."""
    ref = mtk.run(force, _positions(frames), v0, _masses(frames), _cells(frames), DT, steps, KT0, TDAMP, p0, pdamp, mask=mask,
                  natoms=_natoms(frames), skin=skin, rc=rc, **dict(nhc or {}, **kw))
    npt.assert_not_marginal(ref, skin)
    return ref


def _setup(eng, frames, v0, skin, barostat, nhc=None):
    """`barostat` = (P0, pdamp, pchain, ploop, mask), or None."""
    eng.set_skin(skin)
    eng.set_frames(frames)
    eng.md_init(None, v0)
    eng.md_set_nose_hoover(KT0, TDAMP, **(nhc or {}))
    if barostat:
        eng.md_set_mtk(*barostat)


def _collect(eng, outs):
    x, v = eng.md_state()
    eta, veta = eng.md_chain()
    omega, xi, vxi = eng.md_mtk_state()
    res = dict(x=x, v=v, cells=eng.md_cells(), eta=eta, veta=veta, omega=omega, xi=xi, vxi=vxi,
               n_rebuilds=sum(o["n_rebuilds"] for o in outs))
    for k in ("epot", "ekin", "echain", "ebaro", "volume", "press"):
        res[k] = np.concatenate([o[k][1 if j else 0:] for j, o in enumerate(outs)])
    return res


def _device(nn, frames, v0, skin, steps, barostat, nhc=None, splits=None):
    from tensoralloy_amd import Engine
    with Engine(nn) as eng:
        _setup(eng, frames, v0, skin, barostat, nhc)
        return _collect(eng, [eng.md_run(n, DT) for n in (splits or [steps])])


def _assert_parity(dev, ref, tol=TOL, what="", keys=KEYS):
    gaps = {k: float(np.abs(dev[k] - ref[k]).max()) for k in keys + STATE}
    print("parity gaps", what, gaps, "rebuilds", dev["n_rebuilds"], ref.get("rebuild_steps"), ref.get("end_rebuild"))
    for k in keys + STATE:
        assert dev[k].shape == ref[k].shape, k
    for k in keys:
        assert gaps[k] < tol, gaps
    for k in STATE:
        assert gaps[k] < tol * max(1.0, float(np.abs(ref[k]).max())), gaps


def _assert_rebuilds(dev, ref):
    """The rebuilds the strain-aware rule asks for, and the one for the final cells where the run moved them."""
    assert dev["n_rebuilds"] == ref["n_rebuilds"] + int(ref["end_rebuild"]), (dev["n_rebuilds"], ref["rebuild_steps"],
                                                                              ref["end_rebuild"])


@functools.lru_cache(maxsize=None)
def _case_inputs(case):
    scale, p0, pdamp, skin, steps, mask = CASES[case]
    atoms = _anchor(scale)
    return atoms, _velocities([atoms]), (p0, pdamp, 3, 1, mask)


@functools.lru_cache(maxsize=None)
def _case_reference(case):
    _, p0, pdamp, skin, steps, mask = CASES[case]
    atoms, v0, _ = _case_inputs(case)
    return _freeze(_reference(_oracle_forces(_ni(), [atoms]), [atoms], v0, steps, p0, pdamp, skin, mask=mask))


@functools.lru_cache(maxsize=None)
def _case_device(case):
    _, _, _, skin, steps, _ = CASES[case]
    atoms, v0, barostat = _case_inputs(case)
    return _freeze(_device(_ni(), [atoms], v0, skin, steps, barostat))


# -- 1 ---------------------------------------------------------------------------------------------------
def test_parity_without_rebuild(lib):
    ref, dev = _case_reference("A"), _case_device("A")
    atoms, _, _ = _case_inputs("A")
    assert ref["rebuild_steps"] == [] and ref["end_rebuild"]
    assert abs(np.abs(ref["cells"] - _cells([atoms])).max() - 0.1069) < 5e-5        # (> 1e-3 A, as asked)
    assert abs(ref["volume"][0, 0] - 371.53) < 5e-3 and abs(ref["volume"][-1, 0] - 355.20) < 5e-3
    assert abs(ref["press"][0, 0].mean() - -0.05580) < 5e-6 and abs(ref["press"][-1, 0].mean() - -0.00605) < 5e-6
    assert np.abs(ref["omega"][0] - -0.006049).max() < 5e-7
    assert dev["epot"].shape == (41, 1) and dev["press"].shape == (41, 1, 3) and dev["ebaro"].shape == (41, 1)
    _assert_parity(dev, ref, what="A")
    assert dev["n_rebuilds"] == 1   # the build for the final cells
    H = mtk.conserved(dev)[:, 0]
    print("excursion of H' on the device", np.abs(H - H[0]).max(), "of the reference", np.ptp(mtk.conserved(ref)[:, 0]))


# -- 2 ---------------------------------------------------------------------------------------------------
def test_rebuilds_caused_by_strain_alone(lib):
    """Parity of omega and of both chains behind the rebuilds also says that the launch enqueued behind the stale
    list of step 11 advanced none of them."""
    ref, dev = _case_reference("B"), _case_device("B")
    assert ref["rebuild_steps"] == [11, 19] and ref["end_rebuild"]
    for step, lim, umax, dmax in ((11, 0.0426, 0.0595, 0.2207), (19, 0.0208, 0.0311, 0.2212)):
        rec = ref["log"][step - 1]
        assert rec["step"] == step
        assert abs(rec["lim"][0] - lim) < 5e-5 and abs(rec["umax"][0] - umax) < 5e-5 and abs(rec["dmax"][0] - dmax) < 5e-5
        assert rec["lim"][0] < rec["umax"][0] < 0.15   # stale by the strain-aware rule, |u| far below skin / 2
    assert all(r["umax"][0] < 0.15 for r in ref["log"])
    assert dev["n_rebuilds"] == ref["n_rebuilds"] + 1
    _assert_parity(dev, ref, what="B")


# -- 3 ---------------------------------------------------------------------------------------------------
def test_mask(lib):
    ref, dev = _case_reference("C"), _case_device("C")
    atoms, _, _ = _case_inputs("C")
    assert ref["rebuild_steps"] == [] and ref["end_rebuild"]
    assert abs(ref["volume"][0, 0] - 350.10) < 5e-3 and abs(ref["volume"][-1, 0] - 345.21) < 5e-3
    assert abs(ref["cells"][0][0, 0] - 6.9971) < 5e-5 and abs(ref["cells"][0][2, 2] - 7.0001) < 5e-5
    h0 = _cells([atoms])[0]
    assert np.array_equal(dev["cells"][0][:, 1], h0[:, 1]) and np.array_equal(ref["cells"][0][:, 1], h0[:, 1])
    assert dev["omega"][0, 1] == 0.0
    assert np.abs(dev["cells"][0][:, [0, 2]] - h0[:, [0, 2]]).max() > 1e-2
    assert abs(dev["cells"][0][0, 0] - dev["cells"][0][2, 2]) > 1e-6   # each free axis has its own strain rate
    _assert_parity(dev, ref, what="C")
    assert dev["n_rebuilds"] == 1


# -- 4 ---------------------------------------------------------------------------------------------------
def test_split_runs_and_restart(lib):
    """10 + 20 steps against 30, and 10 steps, the state carried to a fresh engine, 20 more."""
    from tensoralloy_amd import Engine
    _, _, _, skin, _, _ = CASES["A"]
    atoms, v0, barostat = _case_inputs("A")
    whole = _device(_ni(), [atoms], v0, skin, 30, barostat)
    split = _device(_ni(), [atoms], v0, skin, 30, barostat, splits=[10, 20])
    _assert_parity(split, whole, tol=1e-12, what="10 + 20")
    with Engine(_ni()) as eng:
        _setup(eng, [atoms], v0, skin, barostat)
        omega, xi, vxi = eng.md_mtk_state()
        assert omega.shape == (1, 3) and xi.shape == (1, 3) and not omega.any() and not xi.any() and not vxi.any()
        put = np.array([[1e-3, -2e-3, 3e-3]]), np.array([[0.1, -0.2, 0.3]]), np.array([[-0.01, 0.02, 0.03]])
        eng.md_set_mtk_state(*put)
        assert all(np.array_equal(a, b) for a, b in zip(eng.md_mtk_state(), put))
        eng.md_set_mtk_state(vxi=put[2])   # (None = zeros)
        got = eng.md_mtk_state()
        assert not got[0].any() and not got[1].any() and np.array_equal(got[2], put[2])
        eng.md_set_mtk_state()
        first = eng.md_run(10, DT)
        (x, v), (eta, veta), state, cells = eng.md_state(), eng.md_chain(), eng.md_mtk_state(), eng.md_cells()
        assert np.abs(state[0]).max() > 1e-6
    cut = atoms.copy()
    cut.set_cell(cells[0])
    cut.positions[:] = x
    with Engine(_ni()) as eng:
        eng.md_set_nose_hoover(KT0, TDAMP)
        eng.md_set_mtk(*barostat)
        eng.set_skin(skin)
        eng.set_frames([cut])     # (keeps the settings)
        eng.md_init(None, v)      # (puts the chains and the barostat at rest)
        assert not eng.md_mtk_state()[0].any()
        eng.md_set_chain(eta, veta)
        eng.md_set_mtk_state(*state)
        second = eng.md_run(20, DT)
        res = _collect(eng, [first, second])
    _assert_parity(res, whole, tol=1e-12, what="restart")


# -- 5 ---------------------------------------------------------------------------------------------------
def test_frame_above_1024_atoms(lib):
    """1372 atoms in one workgroup of 1024 threads: each thread meets several atoms."""
    from tensoralloy_amd import Engine
    nn = _ni()
    big = _strained(fcc(rep=(7, 7, 7), jitter=0.02, seed=8), 1.02)
    assert len(big) == 1372
    v0 = _velocities([big], seed=8)
    with Engine(nn) as other:
        other.set_skin(0.0)
        other.set_frames([big])
        ref = _reference(_engine_forces(other), [big], v0, 10, 0.0, 300 * DT, 0.3)
    dev = _device(nn, [big], v0, 0.3, 10, (0.0, 300 * DT, 3, 1, None))
    _assert_rebuilds(dev, ref)
    _assert_parity(dev, ref, what="1372 atoms")
    assert np.abs(dev["cells"] - _cells([big])).max() > 1e-3


# -- 6 ---------------------------------------------------------------------------------------------------
def test_batch_of_unlike_frames(lib):
    """Four frames at once, every one with its own strain rates and chains. The lone atom (g = 3) feels no force
    and no virial: its trajectory and cell are those of a force-free one-atom reference run."""
    nn = make_eam(["Mo", "Ni"], 6.0, potential="zjw04")
    lone = Atoms(symbols=["Ni"], positions=[[10.0, 10.0, 10.0]], cell=np.diag([20.0, 20.0, 20.0]), pbc=True)
    frames = [_anchor(1.02), _alloy(["Ni", "Mo"], rep=(2, 2, 3)), fcc(rep=(3, 3, 3), jitter=0.02, seed=4), lone]
    natoms = _natoms(frames)
    assert natoms == [32, 48, 108, 1]
    v0 = _velocities(frames, seed=11)
    v0[-1] = [0.01, -0.02, 0.03]
    barostat = (0.0, 300 * DT, 3, 1, None)
    ref = _reference(_oracle_forces(nn, frames), frames, v0, 20, 0.0, 300 * DT, 0.3)
    dev = _device(nn, frames, v0, 0.3, 20, barostat)
    assert dev["omega"].shape == (4, 3) and dev["xi"].shape == (4, 3) and dev["ebaro"].shape == (21, 4)
    _assert_rebuilds(dev, ref)
    _assert_parity(dev, ref, what="batch")
    for f in range(4):   # no two barostats alike
        for j in range(f):
            assert abs(dev["omega"][f, 0] - dev["omega"][j, 0]) > 1e-9 and np.abs(dev["vxi"][f] - dev["vxi"][j]).max() > 1e-9, (f, j)
    assert np.all(dev["epot"][:, 3] == dev["epot"][0, 3])
    free = lambda x, cells: (np.zeros(1), np.zeros_like(x), np.zeros((1, 3, 3)))
    alone = mtk.run(free, lone.positions, v0[-1:], _masses([lone]), _cells([lone]), DT, 20, KT0, TDAMP, 0.0, 300 * DT)
    gaps = dict(x=np.abs(alone["x"] - dev["x"][-1:]).max(), v=np.abs(alone["v"] - dev["v"][-1:]).max(),
                cells=np.abs(alone["cells"][0] - dev["cells"][3]).max(),
                ekin=np.abs(alone["ekin"][:, 0] - dev["ekin"][:, 3]).max(),
                echain=np.abs(alone["echain"][:, 0] - dev["echain"][:, 3]).max(),
                ebaro=np.abs(alone["ebaro"][:, 0] - dev["ebaro"][:, 3]).max(),
                omega=np.abs(alone["omega"][0] - dev["omega"][3]).max(), vxi=np.abs(alone["vxi"][0] - dev["vxi"][3]).max())
    print("lone atom", gaps)
    assert max(gaps.values()) < 1e-12 * max(1.0, float(np.abs(alone["ebaro"]).max())), gaps
    assert np.abs(dev["v"][-1] - v0[-1]).max() > 1e-6 and dev["cells"][3][0, 0] > 20.0   # (chain and barostat act on it)


# -- 7 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [dict(pchain=1), dict(pchain=8, ploops=4), dict(dof_removed=3)],
                         ids=["Mp1", "Mp8_Lp4", "dof3"])
def test_chain_shapes(lib, shape):
    _, p0, _, skin, _, _ = CASES["A"]
    atoms, v0, _ = _case_inputs("A")
    pdamp = 100 * DT
    nhc = {k: v for k, v in shape.items() if k == "dof_removed"}
    pchain, ploops = shape.get("pchain", 3), shape.get("ploops", 1)
    ref = _reference(_oracle_forces(_ni(), [atoms]), [atoms], v0, 20, p0, pdamp, skin, nhc=nhc, pchain=pchain, ploops=ploops)
    dev = _device(_ni(), [atoms], v0, skin, 20, (p0, pdamp, pchain, ploops, None), nhc=nhc)
    assert dev["xi"].shape == (1, pchain)
    _assert_rebuilds(dev, ref)
    _assert_parity(dev, ref, what=str(shape))


# -- 8 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["sf", "grap"])
def test_model_families(lib, family):
    """20 steps against a second engine. The randomly initialised networks have a pressure of their own, of the
    order of -1 eV / A^3 for SF (tests/test_gpu_md_npt.py), so the target is the pressure of the initial state
    + 0.01 eV / A^3."""
    from tensoralloy_amd import Engine
    nn = make_nn(["Ni"], 6.0, True, [8]) if family == "sf" else make_grap_nn(["Ni"], 6.0, [16])
    frames = [_anchor(1.02)]
    v0 = _velocities(frames)
    pdamp, skin = 200 * DT, 0.5
    with Engine(nn) as other:
        other.set_skin(0.0)
        other.set_frames(frames)
        _, _, W = _engine_forces(other)(_positions(frames), _cells(frames))
        S, V = npt.frame_sums(_masses(frames), v0, [32]), npt.volumes(_cells(frames))
        p0 = float(((S - np.diagonal(W, axis1=1, axis2=2)) / V[:, None]).mean()) + 0.01
        ref = _reference(_engine_forces(other), frames, v0, 20, p0, pdamp, skin)
    print(family, "P0", p0, "omega", ref["omega"], "V", ref["volume"][0, 0], ref["volume"][-1, 0])
    assert np.abs(ref["omega"]).max() > 1e-6
    dev = _device(nn, frames, v0, skin, 20, (p0, pdamp, 3, 1, None))
    _assert_rebuilds(dev, ref)
    _assert_parity(dev, ref, what=family)


# -- 9 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("berendsen", [False, True], ids=["chain", "berendsen_npt_chain"])
def test_existing_paths_untouched(lib, berendsen):
    """Switched on, used, and switched off again: the plain chain run and the Berendsen-NPT + chain run that follow
    are those of an engine that never heard of it, bit for bit."""
    from tensoralloy_amd import Engine
    _, _, _, skin, _, _ = CASES["A"]
    atoms, v0, barostat = _case_inputs("A")

    def run(eng):
        eng.set_frames([atoms])
        eng.md_init(None, v0)
        if berendsen:
            eng.md_set_barostat(0.0, 20 * DT, 0.9)
        out = eng.md_run(30, DT)
        assert "ebaro" not in out and ("volume" in out) == berendsen
        x, v = eng.md_state()
        eta, veta = eng.md_chain()
        res = dict(x=x, v=v, cells=eng.md_cells(), eta=eta, veta=veta, epot=out["epot"], ekin=out["ekin"], echain=out["echain"])
        if berendsen:
            res.update(volume=out["volume"], press=out["press"])
        return res

    with Engine(_ni()) as eng:
        eng.set_skin(skin)
        eng.md_set_nose_hoover(KT0, TDAMP)
        fresh = run(eng)
    with Engine(_ni()) as eng:
        _setup(eng, [atoms], v0, skin, barostat)
        assert "ebaro" in eng.md_run(3, DT)
        eng.md_set_mtk(0.0, 0.0)
        after = run(eng)
    for k in fresh:
        assert np.array_equal(fresh[k], after[k]), k
    assert np.abs(fresh["x"] - atoms.positions).max() > 1e-3


# -- 10 --------------------------------------------------------------------------------------------------
def test_device_md_driver(lib):
    """`DeviceMD(..., pdamp=)`: runs cut at the observers' intervals continue the barostat and its chain."""
    from tensoralloy_amd import DeviceMD, Engine
    _, p0, pdamp, skin, steps, _ = CASES["A"]
    atoms, v0, _ = _case_inputs("A")
    atoms = atoms.copy()
    dev = _case_device("A")
    H = mtk.conserved(dev)[:, 0]
    seen = []
    with Engine(_ni()) as eng:
        eng.set_skin(skin)
        with pytest.raises(ValueError, match="pdamp .* and taup .* exclude each other"):
            DeviceMD(eng, atoms, DT, temperature_K=300.0, tdamp=TDAMP, velocities=v0, pressure=p0, pdamp=pdamp, taup=20 * DT,
                     compressibility=0.9)
        dyn = DeviceMD(eng, atoms, DT, temperature_K=300.0, tdamp=TDAMP, velocities=v0, pressure=p0, pdamp=pdamp)
        assert abs(dyn.get_volume() - dev["volume"][0, 0]) < 1e-9 and abs(dyn.get_conserved_energy() - H[0]) < 1e-12
        assert dyn.get_conserved_energy() == dyn.ekin[0] + dyn.epot[0] + dyn.echain[0] + dyn.ebaro[0]
        dyn.attach(lambda: seen.append((dyn.nsteps, dyn.get_volume(), dyn.get_pressure(), dyn.get_conserved_energy())),
                   interval=15)
        dyn.run(steps)
        cell = dyn.get_cell()
        omega, _, vxi = eng.md_mtk_state()
        assert [s[0] for s in seen] == [15, 30]
        for step, volume, press, h in seen:
            assert abs(volume - dev["volume"][step, 0]) < 1e-12 * dev["volume"][step, 0]
            assert abs(press - dev["press"][step, 0].mean()) < 1e-12 and abs(h - H[step]) < 1e-12 * max(1.0, abs(H[step]))
        assert np.abs(atoms.positions - dev["x"]).max() < 1e-12 and np.abs(dyn.velocities - dev["v"]).max() < 1e-12
        assert np.array_equal(np.asarray(atoms.get_cell(complete=True)), cell) and np.abs(cell - dev["cells"][0]).max() < 1e-12
        assert np.abs(omega - dev["omega"]).max() < 1e-12 and np.abs(vxi - dev["vxi"]).max() < 1e-12
        assert abs(dyn.get_conserved_energy() - H[-1]) < 1e-12 * max(1.0, abs(H[-1]))
        # a Berendsen-barostat driver on the same engine afterwards: the constructor switched this barostat off
        other = DeviceMD(eng, _anchor(1.02).copy(), DT, temperature_K=300.0, tdamp=TDAMP, velocities=v0, pressure=p0,
                         taup=20 * DT, compressibility=0.9)
        other.run(3)
        assert other.ebaro is None
        with pytest.raises(ValueError, match="Martyna-Tobias-Klein barostat is off"):
            eng.md_mtk_state()


# -- 11 --------------------------------------------------------------------------------------------------
def test_refusals(lib):
    from tensoralloy_amd import Engine
    nn = _ni()
    nan, inf = float("nan"), float("inf")
    _, p0, pdamp, skin, _, _ = CASES["A"]
    atoms, v0, barostat = _case_inputs("A")
    good = _device(nn, [atoms], v0, skin, 3, barostat)
    with Engine(nn) as eng:
        _setup(eng, [atoms], v0, skin, barostat)
        for kw, what in ((dict(pressure=nan), "pressure must be finite"), (dict(pressure=inf), "pressure must be finite"),
                         (dict(pdamp=nan), "tau_p must be finite"), (dict(pdamp=inf), "tau_p must be finite"),
                         (dict(chain=0), "chain must be 1 .. 8"), (dict(chain=9), "chain must be 1 .. 8"),
                         (dict(loops=0), "loops must be 1 .. 16"), (dict(loops=17), "loops must be 1 .. 16"),
                         (dict(mask=(0, 0, 0)), "mask leaves no axis")):
            args = dict(pressure=p0, pdamp=pdamp)
            args.update(kw)
            with pytest.raises(ValueError, match="ta_md_set_mtk_barostat: " + what):
                eng.md_set_mtk(**args)
        with pytest.raises(ValueError, match="three entries"):
            eng.md_set_mtk(p0, pdamp, mask=(1, 1))
        # only one barostat, in both directions
        with pytest.raises(ValueError, match="ta_md_set_barostat: the Martyna-Tobias-Klein barostat is on"):
            eng.md_set_barostat(0.0, 20 * DT, 0.9)
        eng.md_set_barostat(0.0, 0.0, 0.0)       # switching off is always allowed
        with pytest.raises(ValueError, match="had no Martyna-Tobias-Klein barostat"):   # no run yet
            eng._check(eng._lib.ta_md_get_mtk_records(eng._handle, None))
        with pytest.raises(ValueError, match="omega"):
            eng.md_set_mtk_state(np.zeros((1, 2)))
        with pytest.raises(ValueError, match="non-finite vxi"):
            eng.md_set_mtk_state(None, None, np.array([[0.0, nan, 0.0]]))
        same = _collect(eng, [eng.md_run(3, DT)])   # the refused calls left the setting as it was
        for k in KEYS + STATE:
            assert np.array_equal(good[k], same[k]), k
        # what ta_md_run asks for: the Nose-Hoover chain and no other thermostat
        eng.md_set_nose_hoover(0.0)
        with pytest.raises(ValueError, match="ta_md_run: the Martyna-Tobias-Klein barostat .* Nose-Hoover chain thermostat is off"):
            eng.md_run(1, DT)
        eng.md_set_thermostat(KT0, TDAMP)
        with pytest.raises(ValueError, match="ta_md_run: the Martyna-Tobias-Klein barostat .* so is the Berendsen thermostat"):
            eng.md_run(1, DT)
        eng.md_set_thermostat(0.0, 0.0)
        eng.md_set_langevin(KT0, 0.01 / DT, 1)
        with pytest.raises(ValueError, match="ta_md_run: the Martyna-Tobias-Klein barostat .* so is the Langevin thermostat"):
            eng.md_run(1, DT)
        eng.md_set_langevin(0.0, 0.0, 0)
        eng.md_set_nose_hoover(KT0, TDAMP)
        # the samplers that refuse the barostat, for the same reasons; the others run
        for on, off, what in ((lambda: eng.md_set_sampling(4, 1), lambda: eng.md_set_sampling(0), r"sampling \(ta_md_set_sampling\)"),
                              (lambda: eng.md_set_rdf(16), lambda: eng.md_set_rdf(0), r"the pair distributions \(ta_md_set_rdf\)"),
                              (lambda: eng.md_set_sq(np.array([[1, 0, 0]], dtype=np.int32)), lambda: eng.md_set_sq(None),
                               r"the structure factors \(ta_md_set_sq\)"),
                              (lambda: eng.md_set_flux(4), lambda: eng.md_set_flux(0),
                               r"the heat current and pressure tensor \(ta_md_set_flux\)")):
            on()
            with pytest.raises(ValueError, match="ta_md_run: " + what + r" and the barostat \(ta_md_set_mtk_barostat\) are both on"):
                eng.md_run(1, DT)
            off()
        eng.md_set_adf(16, 3.0)
        eng.md_set_order((4, 6), 3.0, 16)
        eng.md_set_clusters(3.0, 0, None, 8)
        eng.md_set_cna("adaptive")
        assert "ebaro" in eng.md_run(2, DT)
        # a barostat that is off: the getters say so, the switch at the other end too
        eng.md_set_mtk(0.0, 0.0)
        with pytest.raises(ValueError, match="ta_md_get_mtk_state: the Martyna-Tobias-Klein barostat is off"):
            eng.md_mtk_state()
        eng.md_set_barostat(0.0, 20 * DT, 0.9)
        with pytest.raises(ValueError, match="ta_md_set_mtk_barostat: the Berendsen barostat is on"):
            eng.md_set_mtk(p0, pdamp)
        out = eng.md_run(1, DT)                    # (the Berendsen barostat stayed on)
        assert "volume" in out and "ebaro" not in out
    slab = atoms.copy()
    slab.pbc = [True, True, False]
    with Engine(nn) as eng:
        _setup(eng, [atoms, slab], np.concatenate([v0, v0]), skin, barostat)
        x0, vv0 = eng.md_state()
        with pytest.raises(ValueError, match="frame 1 is not periodic along all three axes"):
            eng.md_run(3, DT)
        x1, vv1 = eng.md_state()
        assert np.array_equal(x0, x1) and np.array_equal(vv0, vv1) and np.array_equal(eng.md_cells(), _cells([atoms, slab]))
        eng.set_frames([atoms])                  # keeps the setting, drops the MD state
        with pytest.raises(ValueError, match="ta_md_get_mtk_state called before ta_md_init"):
            eng.md_mtk_state()
        with pytest.raises(ValueError, match="ta_md_set_mtk_state called before ta_md_init"):
            eng.md_set_mtk_state()


# -- 12 --------------------------------------------------------------------------------------------------
def test_physics(lib):
    """256 Ni atoms (fcc 4 x 4 x 4, EAM) from 300 K to a 900 K target at P0 = 0, dt = 2 fs, tdamp = 50 fs, pdamp = 500
    fs, 2000 steps, on the device alone. The mean T of the second half is within 5 % of the target (the argument of
    tests/test_gpu_md_nhc.py::test_thermalisation). The excursion of H' is at most 2 x 2.854 = 5.708 times the
    excursion of E in the NVE run of the same start and length: 2.854 is the ratio of the NumPy reference with the
    CPU oracle on this case (0.02025 eV against 0.00709 eV; mean T 897.0 K), and the factor 2 is for the chaotic
    divergence of device and reference trajectories over 4 ps. Mean pressure and compressibility are printed, not
    asserted: 256 atoms fluctuate by GPa (the reference: -0.0086 GPa, 1.90 A^3 / eV while the cell still expands)."""
    from tensoralloy_amd import Engine
    from tests.test_gpu_md import _velocities as _nve_velocities
    nn = make_eam(["Ni"], 6.0, potential="zjw04")
    frames = [fcc(rep=(4, 4, 4))]
    n = len(frames[0])
    assert n == 256
    v0 = _nve_velocities(frames, 300.0, 7)
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        eng.set_frames(frames)
        eng.md_init(None, v0)
        nve = eng.md_run(2000, 2 * DT)
        eng.set_frames(frames)
        eng.md_init(None, v0)
        eng.md_set_nose_hoover(md.kB * 900.0, 50 * DT)
        eng.md_set_mtk(0.0, 500 * DT)
        out = eng.md_run(2000, 2 * DT)
    T = 2.0 * out["ekin"][:, 0] / (3 * n * md.kB)
    H = mtk.conserved(out)[:, 0]
    E = (nve["ekin"] + nve["epot"])[:, 0]
    d_H, d_E = np.abs(H - H[0]).max(), np.abs(E - E[0]).max()
    print("mean T of the second half", T[1000:].mean(), "start", T[0], "excursion of H'", d_H, "of E (NVE)", d_E, "ratio",
          d_H / d_E, "V", out["volume"][0, 0], out["volume"][1000:, 0].mean(), "mean P (GPa)",
          out["press"][1000:, 0].mean() / md.GPa, "compressibility (A^3 / eV)",
          md.isothermal_compressibility(out["volume"][1000:, 0], 900.0), "rebuilds", out["n_rebuilds"])
    assert abs(T[1000:].mean() - 900.0) < 0.05 * 900.0
    assert d_E > 0.0 and d_H <= 2.0 * 2.854 * d_E
