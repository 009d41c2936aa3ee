"""GPU: every entry point of the device-resident runs (csrc/ta_api_md.hip, ta_api_relax.hip, ta_resident.hip) on
handles that are then destroyed, three times over in one process. `ta_destroy` releases nothing by hand: every
buffer of the handle frees itself, the barostat's and the temperature-dependent head's included. Every call must
return TA_OK (the engine raises otherwise), and the third repetition must reproduce the first bit for bit:
energies, final positions and g(r) counts. (No assertion on free device memory: the buffers in question are a
few KB, below anything an allocator is known to report.)"""
import numpy as np
import pytest

from tensoralloy_amd import Engine, _lib, interpolate, md
from tensoralloy_amd.atoms import atomic_masses
from tensoralloy_amd.td import TemperatureDependentAtomicNN
from tests.helpers import fcc, make_nn

pytestmark = pytest.mark.gpu

DT = md.fs
WANT = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES
NEVER = 1e-10   # an fmax no run here reaches
SKIN = 0.4


def _model():
    """Radial symmetry functions only: the angular kernels add with floating-point atomics in LDS, so their
    forces differ in the last bit from run to run, on any build; this model's evaluation is reproducible."""
    return make_nn(["Ni"], 4.5, False, [8], sf_kwargs={"eta": [0.1, 0.5, 1.0, 2.0], "omega": [0.0, 1.5]})


def _td_model(base):
    nn = TemperatureDependentAtomicNN(base.elements, base.descriptor, hidden_sizes=[8], activation="softplus",
                                      export_properties=("energy", "forces", "stress"),
                                      finite_temperature={"activation": "softplus", "layers": [8], "algo": "default"})
    nn.attach_transformer(base.transformer)
    nn.initialize(seed=7, bias_scale=0.1)
    return nn


def _sequence(nn, td):
    """One pass over the three handles; what it returns is compared bit for bit between passes."""
    out = {}
    frames = [fcc(rep=(2, 2, 2), jitter=0.05, seed=3), fcc(rep=(2, 2, 2), jitter=0.05, seed=4)]
    masses = np.array([atomic_masses[z] for a in frames for z in a.numbers], dtype=np.float64)
    rng = np.random.RandomState(5)
    v0 = np.concatenate([md.maxwell_boltzmann(masses[:32], md.kB * 300.0, rng),
                         md.maxwell_boltzmann(masses[32:], md.kB * 300.0, rng)])
    with Engine(nn) as eng:   # Nose-Hoover chain with sampling and g(r); then NPT; then a cell relaxation
        eng.set_skin(SKIN)
        eng.set_frames(frames)
        eng.md_init(masses, v0)
        eng.md_set_nose_hoover(md.kB * 300.0, 20 * DT, chain=3)
        eng.md_set_sampling(n_lags=4, sample_every=2)
        eng.md_set_rdf(n_bins=16, sample_every=2)
        run = eng.md_run(8, DT)
        out["nvt_epot"], out["nvt_echain"] = run["epot"], run["echain"]
        out["nvt_x"], out["nvt_v"] = eng.md_state()
        corr, rdf = eng.md_correlations(), eng.md_rdf()
        assert corr["n_samples"] == 5 and rdf["n_samples"] == 5 and rdf["counts"].sum() > 0
        out["vacf_sum"], out["rdf_counts"] = corr["vacf_sum"], rdf["counts"]
        eng.md_set_sampling(0)
        eng.md_set_rdf(0)
        eng.md_set_barostat(0.0, 20 * DT, 0.9)
        run = eng.md_run(8, DT, want=WANT | _lib.TA_WANT_VIRIAL)
        out["npt_epot"], out["npt_volume"] = run["epot"], run["volume"]
        out["npt_x"], _ = eng.md_state()
        out["npt_cells"] = eng.md_cells()
        eng.relax_init()
        eng.relax_set_cell(True)
        run = eng.relax_run(5, NEVER, want=WANT | _lib.TA_WANT_VIRIAL)
        assert list(run["steps"]) == [5, 5]
        out["relax_energy"] = run["energy"]
        out["relax_x"] = eng.relax_state()["positions"]
        out["relax_cells"] = eng.relax_cell_state()["cells"]
    with Engine(nn) as eng:   # a 5-image band
        eng.set_skin(SKIN)
        eng.set_frames(interpolate(frames[0], frames[1], 5))
        eng.relax_init()
        eng.relax_set_band(True, k=0.1, climb=True)
        run = eng.relax_run(5, NEVER)
        assert list(run["steps"]) == [5] * 5
        band = eng.relax_band_state()
        out["band_energy"], out["band_forces"] = band["energies"], band["forces"]
        out["band_x"] = eng.relax_state()["positions"]
    hot = frames[0].copy()
    hot.info["etemperature"] = 0.5
    with Engine(td) as eng:   # the temperature-dependent head: its temperatures, U and S per atom
        r = eng.evaluate([hot], want=WANT)[0]
        out["td_energy"], out["td_forces"] = np.float64(r["energy"]), r["forces"]
    return out


def test_three_rounds_of_create_run_destroy_are_bitwise_equal():
    nn = _model()
    td = _td_model(nn)
    rounds = [_sequence(nn, td) for _ in range(3)]
    first, third = rounds[0], rounds[2]
    assert sorted(first) == sorted(third)
    differ = {}
    for key in first:
        a, b = np.asarray(first[key]), np.asarray(third[key])
        assert np.all(np.isfinite(a.astype(np.float64))), key
        assert a.shape == b.shape, key
        if a.tobytes() != b.tobytes():
            differ[key] = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
    print("keys that differ between round 1 and round 3 (largest |difference|):", differ)
    assert not differ
