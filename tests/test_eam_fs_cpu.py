"""eam/fs (Finnis-Sinclair) host side: the file reader and its density convention, and the model
surface of `EamFsNN` (no GPU)."""
import gzip
import os

import numpy as np
import pytest

from tests.fs_reference import synthetic_listed_tables, write_synthetic_fs
from tests.helpers import golden_setfl

FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "Mendelev_Al_Fe_thinned.fs.eam.gz")


def test_reader_on_the_mendelev_fixture():
    from tensoralloy_amd.io import read_eam_fs_setfl
    fl = read_eam_fs_setfl(FIXTURE)    # gzip'ed files are read as they are
    assert fl.elements == ["Al", "Fe"]
    assert (fl.nr, fl.nrho) == (2000, 2000)
    assert fl.dr == pytest.approx(0.00325, abs=1e-15) and fl.drho == pytest.approx(0.15, abs=1e-15)
    assert fl.rcut == 6.5
    assert fl.atomic_masses == pytest.approx([26.9815385, 55.845])
    assert fl.lattice_constants == pytest.approx([4.04527, 2.855312])
    assert fl.lattice_types == ["fcc", "bcc"]
    assert sorted(fl.rho) == ["AlAl", "AlFe", "FeAl", "FeFe"]
    assert sorted(fl.embed) == ["Al", "Fe"] and sorted(fl.phi) == ["AlAl", "AlFe", "FeFe"]
    # every token consumed: the token count is exactly what the header implies
    with gzip.open(FIXTURE, "rt") as fp:
        tok = " ".join(fp.read().split("\n")[5:]).split()
    assert len(tok) == 2 * (4 + 2000 + 2 * 2000) + 3 * 2000
    # this file's cross densities are symmetric
    np.testing.assert_array_equal(fl.rho["AlFe"].y, fl.rho["FeAl"].y)
    # phi is r * phi / r except at r = 0, where the raw value stays (as _read_setfl)
    r = fl.phi["FeFe"].x
    assert r[0] == 0.0 and r[1] == pytest.approx(0.00325)
    raw = np.array(tok[2 * (4 + 6000) + 2 * 2000:2 * (4 + 6000) + 3 * 2000], dtype=float)  # (2,2) = FeFe
    np.testing.assert_array_equal(fl.phi["FeFe"].y[1:], raw[1:] / r[1:])
    assert fl.phi["FeFe"].y[0] == raw[0]


def test_reader_refuses_an_alloy_file(tmp_path):
    from tensoralloy_amd.io import read_eam_fs_setfl
    with pytest.raises(ValueError):
        read_eam_fs_setfl(golden_setfl("Zhou_AlCu.alloy.eam", tmp_path))


def test_density_convention_on_an_asymmetric_file(tmp_path):
    """LAMMPS: the J-th density table under element I is what an I-neighbour puts at a J-centre,
    so it lands at key J + I (centre first)."""
    from tensoralloy_amd.io import read_eam_fs_setfl
    path = write_synthetic_fs(str(tmp_path / "syn.fs.eam"))
    fl = read_eam_fs_setfl(path)
    r = fl.rho["AlAl"].x
    listed = synthetic_listed_tables(r)
    assert not np.allclose(listed[("Al", "Fe")], listed[("Fe", "Al")])
    for (I, J), table in listed.items():
        np.testing.assert_allclose(fl.rho[J + I].y, table, rtol=1e-15, atol=0.0)


def test_export_to_setfl_round_trips_the_keys(tmp_path, monkeypatch):
    """export_to_setfl writes rho[J + I] as the J-th table under element I, so read_eam_fs_setfl
    gives back every key. The device tabulation is replaced by the file's own knot values here
    (the GPU test runs the real one)."""
    import tensoralloy_amd.engine as engine
    from tensoralloy_amd import UniversalTransformer
    from tensoralloy_amd.eam import EamFsNN
    from tensoralloy_amd.io import read_eam_fs_setfl
    src = read_eam_fs_setfl(write_synthetic_fs(str(tmp_path / "syn.fs.eam")))
    els = src.elements

    class KnotTables:
        def __init__(self, nn, device=0):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

        def eam_tabulate(self, r, rho):
            assert len(r) == src.nr and len(rho) == src.nrho
            pairs = [a + b for i, a in enumerate(els) for b in els[i:]]
            return {"rho": np.array([src.rho[a + b].y for a in els for b in els]),
                    "embed": np.array([src.embed[el].y for el in els]),
                    "phi": np.array([src.pair("phi", p[:2], p[2:]).y for p in pairs]), "pairs": pairs}

    monkeypatch.setattr(engine, "Engine", KnotTables)
    nn = EamFsNN(els)
    nn.attach_transformer(UniversalTransformer(els, rcut=src.rcut, angular=False))
    out = nn.export_to_setfl(str(tmp_path / "out.fs.eam"), nr=src.nr, dr=src.dr, nrho=src.nrho, drho=src.drho)
    back = read_eam_fs_setfl(out)
    assert sorted(back.rho) == sorted(src.rho)
    for key in src.rho:
        np.testing.assert_allclose(back.rho[key].y, src.rho[key].y, rtol=1e-15, atol=1e-300)
    for key in src.phi:
        np.testing.assert_allclose(back.phi[key].y[1:], src.phi[key].y[1:], rtol=1e-14)
    for el in els:
        np.testing.assert_allclose(back.embed[el].y, src.embed[el].y, rtol=1e-15)


def test_model_surface_two_elements():
    from tensoralloy_amd.eam import EamFsNN
    from tensoralloy_amd.utils import Defaults
    nn = EamFsNN(["Fe", "Al"])
    d = list(Defaults.hidden_sizes)
    assert nn.elements == ["Al", "Fe"]
    assert nn.all_kbody_terms == ["AlAl", "AlFe", "FeAl", "FeFe"]
    assert nn.potentials == {"Al": {"embed": "nn"}, "Fe": {"embed": "nn"},
                             "AlAl": {"rho": "nn", "phi": "nn"}, "AlFe": {"rho": "nn", "phi": "nn"},
                             "FeAl": {"rho": "nn"}, "FeFe": {"rho": "nn", "phi": "nn"}}
    assert nn.hidden_sizes == {"Al": {"embed": d}, "Fe": {"embed": d}, "AlAl": {"rho": d, "phi": d},
                               "AlFe": {"rho": d, "phi": d}, "FeAl": {"rho": d}, "FeFe": {"rho": d, "phi": d}}
    assert sum(fn == "rho" for fns in nn.hidden_sizes.values() for fn in fns) == 4
    assert sum(fn == "phi" for fns in nn.hidden_sizes.values() for fn in fns) == 3
    # ABI slot order: rho[centre][neighbour] centre-major, embed[element], phi[pair a <= b]
    assert nn.nn_functions() == [("AlAl", "rho"), ("AlFe", "rho"), ("FeAl", "rho"), ("FeFe", "rho"),
                                 ("Al", "embed"), ("Fe", "embed"),
                                 ("AlAl", "phi"), ("AlFe", "phi"), ("FeFe", "phi")]
    hs = EamFsNN(["Al", "Fe"], hidden_sizes={"FeAl": {"rho": [8]}, "Fe": {"embed": [4, 4]}}).hidden_sizes
    assert hs["FeAl"]["rho"] == [8] and hs["Fe"]["embed"] == [4, 4] and hs["AlFe"]["rho"] == d


def test_model_round_trip_and_kind():
    from tensoralloy_amd import _lib
    from tensoralloy_amd.eam import EamFsNN, nn_from_dict
    nn = EamFsNN(["Al", "Fe"], hidden_sizes=[8, 4], activation="tanh",
                 custom_potentials={"FeAl": {"rho": "spline@" + FIXTURE}, "AlFe": {"phi": "spline@" + FIXTURE}})
    nn.initialize(seed=3)
    assert set(nn.weights) == {"Al", "Fe", "AlAl", "AlFe", "FeFe"}
    assert "rho" in nn.weights["AlFe"] and "phi" not in nn.weights["AlFe"]
    cfg = nn.as_dict()
    assert cfg["class"] == "EamFsNN"
    npz = {f"{sec}/{fn}/weights_{j}": w for sec, fns in nn.weights.items() for fn, layers in fns.items()
           for j, (w, b) in enumerate(layers)}
    npz.update({f"{sec}/{fn}/biases_{j}": b for sec, fns in nn.weights.items() for fn, layers in fns.items()
                for j, (w, b) in enumerate(layers) if b is not None})
    back = nn_from_dict("EamFsNN", {k: v for k, v in cfg.items() if k != "class"}, npz)
    assert type(back) is EamFsNN
    assert back.potentials == nn.potentials and back.hidden_sizes == nn.hidden_sizes
    assert back.nn_functions() == nn.nn_functions()
    for sec, fns in nn.weights.items():
        for fn, layers in fns.items():
            for (w0, b0), (w1, b1) in zip(layers, back.weights[sec][fn]):
                np.testing.assert_array_equal(w0, w1)
    # the tabulated density is the file's (2, 1) table keyed centre first
    assert back.spline_table("FeAl", "rho").y.shape == (2000,)
    from tensoralloy_amd import UniversalTransformer
    nn.attach_transformer(UniversalTransformer(["Al", "Fe"], rcut=6.0, angular=False))
    desc, _keep = nn.to_desc()
    assert desc.kind == _lib.TA_MODEL_EAM_FS == 5
    assert desc.n_eam_nets == 4 + 2 + 3
    assert _lib.TA_ABI_VERSION == 5


def test_from_setfl_builds_an_all_spline_model(tmp_path):
    from tensoralloy_amd.eam import EamFsNN
    nn = EamFsNN.from_setfl(FIXTURE)
    assert nn.nn_functions() == [None] * 9
    assert all(nn.is_spline(sec, fn) for sec, fns in nn.potentials.items() for fn in fns)
    np.testing.assert_array_equal(nn.spline_table("AlFe", "rho").y, nn.spline_table("FeAl", "rho").y)


def test_analytic_potentials_are_refused():
    from tensoralloy_amd.eam import EamAlloyNN, EamFsNN
    with pytest.raises(ValueError, match="not implemented for eam/fs"):
        EamFsNN(["Al", "Fe"], custom_potentials="zjw04")
    with pytest.raises(ValueError, match="from_setfl"):
        EamFsNN(["Al", "Fe"], custom_potentials="msah11")
    with pytest.raises(ValueError, match="from_setfl"):
        EamFsNN(["Fe"], custom_potentials={"FeFe": {"rho": "msah11"}})
    with pytest.raises(ValueError):
        EamAlloyNN(["Ni"], custom_potentials="msah11")
    with pytest.raises(ValueError, match="inference only"):
        EamFsNN(["Fe"]).constants()
