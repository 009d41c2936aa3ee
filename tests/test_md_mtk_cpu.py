"""CPU: the NumPy reference of the Martyna-Tobias-Klein barostat (tests/md_mtk_reference.py) alone, with the CPU
oracle on the 32-atom Ni anchor of tests/test_gpu_md_npt.py (fcc 2 x 2 x 2, jitter 0.02, seed 3, cell and atoms
scaled 1.02, Zjw04, rc = 6, 300 K velocities), kT0 = kB 300 K, tdamp = 20 fs, pdamp = 50 fs, P0 = 0: the scheme the
device is held to is second order, time-reversible, keeps a masked axis exactly and knows its two modes apart.

Figures of the reference here. Excursion of H' over 32 fs at dt = 2, 1, 0.5 fs: isotropic 0.3244, 0.0813, 0.0202 eV
(ratios 3.99, 4.03); per axis, all free 0.3244, 0.0811, 0.0200 (4.00, 4.05); mask (1, 0, 1) 0.2112, 0.0533, 0.0138
(3.96, 3.87). A run of 30 steps of 1 fs reversed returns to its start to 2.1e-14 at the worst (vxi of the isotropic
mode, per time unit; x to 7.1e-15 A, v to 1.9e-15); the bound below is 100 x that."""
import numpy as np
import pytest

from tests import md_mtk_reference as mtk
from tests.test_gpu_md_npt import _anchor, _cells, _masses, _ni, _oracle_forces, _velocities
from tensoralloy_amd import md

DT = md.fs
KT0, TDAMP, PDAMP = md.kB * 300.0, 20 * DT, 50 * DT
MODES = {"isotropic": None, "all_free": (1, 1, 1), "masked": (1, 0, 1)}


def _run(steps, dt=DT, mask=None, start=None, **kw):
    atoms = _anchor(1.02)
    s = start or dict(x=atoms.positions, v=_velocities([atoms]), cells=_cells([atoms]))
    return mtk.run(_oracle_forces(_ni(), [atoms]), s["x"], s["v"], _masses([atoms]), s["cells"], dt, steps, KT0, TDAMP, 0.0,
                   PDAMP, mask=mask, **kw)


@pytest.mark.parametrize("mode", list(MODES))
def test_conserved_quantity_is_second_order(mode):
    exc = []
    for steps, dt in ((16, 2 * DT), (32, DT), (64, 0.5 * DT)):
        H = mtk.conserved(_run(steps, dt, MODES[mode]))[:, 0]
        exc.append(np.abs(H - H[0]).max())
    print(mode, "excursions of H'", exc, "ratios", exc[0] / exc[1], exc[1] / exc[2])
    assert exc[0] / exc[1] >= 3.5 and exc[1] / exc[2] >= 3.5


@pytest.mark.parametrize("mode", ["isotropic", "masked"])
def test_reversed_run_returns_to_its_start(mode):
    atoms = _anchor(1.02)
    a = _run(30, mask=MODES[mode])
    assert np.abs(a["x"] - atoms.positions).max() > 0.1 and np.abs(a["cells"] - _cells([atoms])).max() > 1e-2
    b = _run(30, mask=MODES[mode], start=dict(x=a["x"], v=-a["v"], cells=a["cells"]), eta0=a["eta"], veta0=-a["veta"],
             omega0=-a["omega"], xi0=a["xi"], vxi0=-a["vxi"])
    gaps = dict(x=np.abs(b["x"] - atoms.positions).max(), v=np.abs(b["v"] + _velocities([atoms])).max(),
                cells=np.abs(b["cells"] - _cells([atoms])).max(), omega=np.abs(b["omega"]).max(),
                veta=np.abs(b["veta"]).max(), vxi=np.abs(b["vxi"]).max())
    print(mode, "reversal gaps", gaps)
    assert max(gaps.values()) < 100 * 2.1e-14, gaps


def test_masked_axis_keeps_its_column_bit_for_bit():
    h0 = _cells([_anchor(1.02)])[0]
    r = _run(30, mask=MODES["masked"])
    assert np.array_equal(r["cells"][0][:, 1], h0[:, 1]) and r["omega"][0, 1] == 0.0
    assert np.abs(r["cells"][0][:, 0] - h0[:, 0]).max() > 1e-2 and np.abs(r["cells"][0][:, 2] - h0[:, 2]).max() > 1e-2
    assert abs(r["cells"][0][0, 0] - r["cells"][0][2, 2]) > 1e-6   # each free axis follows its own pressure


def test_the_mode_is_not_a_bystander():
    iso, free = _run(30), _run(30, mask=MODES["all_free"])
    assert np.all(iso["omega"][0] == iso["omega"][0, 0])           # one strain rate
    assert np.abs(free["omega"][0] - free["omega"][0, 0]).max() > 1e-6
    assert np.abs(iso["x"] - free["x"]).max() > 1e-6 and np.abs(iso["cells"] - free["cells"]).max() > 1e-6


def test_lone_atom_is_an_ideal_gas():
    """One atom, no force and no virial: S_c = m v_c^2 alone drives the cell outwards, and the excursion of H' falls
    by 4 per halving of dt here too."""
    free = lambda x, cells: (np.zeros(1), np.zeros_like(x), np.zeros((1, 3, 3)))
    exc = []
    for steps, dt in ((20, DT), (40, 0.5 * DT)):
        r = mtk.run(free, [[10.0, 10.0, 10.0]], [[0.01, -0.02, 0.03]], [58.6934], [np.diag([20.0, 20.0, 20.0])], dt, steps,
                    KT0, TDAMP, 0.0, PDAMP)
        H = mtk.conserved(r)[:, 0]
        exc.append(np.abs(H - H[0]).max())
        assert np.all(r["volume"][1:, 0] > r["volume"][:-1, 0]) and np.all(r["epot"] == 0.0)
    print("lone atom: excursions of H'", exc)
    assert exc[0] / exc[1] >= 3.5


def test_isothermal_compressibility():
    rng = np.random.RandomState(1)
    V = 1000.0 + 3.0 * rng.standard_normal(200000)
    kappa = md.isothermal_compressibility(V, 300.0)
    assert abs(kappa - 9.0 / (md.kB * 300.0 * 1000.0)) < 0.02 * kappa
    with pytest.raises(ValueError, match="volumes"):
        md.isothermal_compressibility([1.0], 300.0)
    with pytest.raises(ValueError, match="temperature_K"):
        md.isothermal_compressibility(V, 0.0)


def test_device_md_refusals_without_a_device():
    from tensoralloy_amd import DeviceMD
    args = (object(), [object()], DT)
    with pytest.raises(ValueError, match="pdamp .* and taup .* exclude each other"):
        DeviceMD(*args, temperature_K=300.0, tdamp=TDAMP, pressure=0.0, pdamp=PDAMP, taup=1.0, compressibility=1.0)
    with pytest.raises(ValueError, match="needs pressure with pdamp, and the Nose-Hoover"):
        DeviceMD(*args, pressure=0.0, pdamp=PDAMP)
    with pytest.raises(ValueError, match="needs pressure with pdamp, and the Nose-Hoover"):
        DeviceMD(*args, temperature_K=300.0, tdamp=TDAMP, pdamp=PDAMP)
    with pytest.raises(ValueError, match="compressibility belongs to the Berendsen barostat"):
        DeviceMD(*args, temperature_K=300.0, tdamp=TDAMP, pressure=0.0, pdamp=PDAMP, compressibility=1.0)
    with pytest.raises(ValueError, match="pdamp must be a finite time > 0"):
        DeviceMD(*args, temperature_K=300.0, tdamp=TDAMP, pressure=0.0, pdamp=0.0)
    with pytest.raises(ValueError, match="pchain must be 1 .. 8"):
        DeviceMD(*args, temperature_K=300.0, tdamp=TDAMP, pressure=0.0, pdamp=PDAMP, pchain=9)
    with pytest.raises(ValueError, match="ploop must be 1 .. 16"):
        DeviceMD(*args, temperature_K=300.0, tdamp=TDAMP, pressure=0.0, pdamp=PDAMP, ploop=0)
    with pytest.raises(ValueError, match="mask must have three flags"):
        DeviceMD(*args, temperature_K=300.0, tdamp=TDAMP, pressure=0.0, pdamp=PDAMP, mask=(0, 0, 0))


def test_header_and_binding_agree():
    import re
    from tensoralloy_amd import _lib
    header = (_lib.INCLUDE_DIR / "tensoralloy_amd.h").read_text()
    for name in ("ta_md_set_mtk_barostat", "ta_md_get_mtk_state", "ta_md_set_mtk_state", "ta_md_get_mtk_records"):
        assert re.search(r"^int %s\(" % name, header, re.M) and name in _lib.EXPORTED_SYMBOLS
    assert "ta_md_mtk.hip" in _lib.SOURCES
    fields = re.search(r"typedef struct \{([^}]*)\} ta_md_mtk_params;", header).group(1)
    names = re.findall(r"(\w+)(?:\[3\])?;", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))   # (comments hold ';' too)
    assert names == [n for n, _ in _lib.MdMtkParams._fields_]
