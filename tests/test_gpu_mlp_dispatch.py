"""
The per-atom network kernels (csrc/ta_mlp.hip, ta_mlp_tile.h) build by build and edge by edge, against the oracle.

`launch_mlp_all` / `launch_mlp_impl` choose among twenty kernel instantiations:
  * the generic 16-row tile, `mlp_kernel<256/512>` and `mlp_all_kernel<256/512>` (512 threads from a padded
    width of 128 on), with the act' slab in LDS while (2 + layers) x 16 x stride x 8 B fit in 64 KB and
    `TA_MLP_DA_GLOBAL` is unset, else in the global scratch slab;
  * one wavefront per tile, `mlp_wave_kernel<1..3>` and `mlp_wave_all_kernel<1..3>`: from 1024 tiles on (or
    `TA_MLP_WAVE_KERNEL`), 1 to 3 hidden layers up to 64 wide, no skip connection, staged weights of at most
    150 KB; a grid-stride loop over at most 256 workgroups of 8 wavefronts (256 / n_elements per grid row);
  * four or eight wavefronts per tile, `mlp_quad_kernel<1..3, 4/8>` and `mlp_quad_all_kernel<1..3, 4/8>`: widths
    up to 64 from 257 to 1023 tiles (or `TA_MLP_QUAD_KERNEL`), widths 65..128 from the first tile to 4095.
`tests.helpers.mirror_launch` restates these rules on the CPU from the model, the frames and the switch alone. Every row of ROWS
names the launch it must take and the side of each boundary it sits on; `test_rows_sit_where_they_say` proves
both without a GPU, and every GPU row first asserts that `Engine.mlp_launch()` reports exactly that launch: a row
that silently ran another kernel fails instead of comparing the generic kernel with itself.

Bounds (tests/test_gpu_td.py::assert_close, tests/test_gpu_train_scale.py): energy, per-atom energies and forces
to 1e-9 x max(1, |ref|), virial to 1e-8 x max(1, |ref|), against oracle/sf.py or oracle/grap.py frame by frame.
The 33,000-atom rows hold every atom's energy to the network applied to the GPU's own descriptors with every
layer in np.longdouble (oracle.sf.apply_mlp on extended-precision input; the result is rounded to fp64 on return;
descriptors pinned to the oracle on the first frame), forces and virial to the oracle on the first frame, the
frame holding the first tile of the second stride iteration and the last frame, and every atom's force to the
same batch under `TA_MLP_TILE_KERNEL` (one workgroup per tile, no stride loop) at 1e-10 x max(1, |value|).
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import pytest

from tensoralloy_amd import Atoms, _lib
from tests.helpers import (ENV_SWITCHES, LDS_64K, LDS_150K, QUAD_MIN_TILES, TILE_ROWS, WAVE_MIN_TILES, element_tiles, fcc,
                           make_grap_nn, make_nn, mirror_launch, net_of, oracle_eval, oracle_grap_eval, oracle_model,
                           tile_slab_bytes, wave_lds_bytes)
from tests.test_gpu_sf_dispatch import alloy, drop
from tests.test_gpu_train_scale import RC, pin_descriptors

gpu = pytest.mark.gpu

E_REL = F_REL = 1e-9
W_REL = 1e-8
CROSS_REL = 1e-10                   # the same batch through two kernels


# -- models ----------------------------------------------------------------------------------------------------

def etas(n):
    return [0.1 + 0.3 * k for k in range(n)]


def sf(els, hidden, n, **kw):
    """Radial-only symmetry functions: D = n x number of elements."""
    return make_nn(list(els), RC, False, hidden, sf_kwargs=dict(eta=etas(n), omega=[0.0]), **kw)


def pexp(K):
    return {"rl": [1.0 + 0.11 * k for k in range(K)], "pl": [5.0 - 0.12 * k for k in range(K)]}


def grap(els, hidden, K, mom):
    """GRAP with K power-exponential filters: D = K x number of moments x number of elements."""
    return make_grap_nn(list(els), RC, hidden, "pexp", pexp(K), moment_tensors=list(mom))


def flat_channel(nn, k=2):
    """Min-max bounds with xhi == xlo in channel k: the div_no_nan branch (atomic.py:195)."""
    for el in nn.elements:
        lo, hi = nn.minmax[el]
        hi[k] = lo[k]
    return nn


NI, MN, ACN = ("Ni",), ("Mo", "Ni"), ("Al", "Cu", "Ni")
NARROW, WIDE = [24, 40], [80, 96]

MODELS = {
    # quad, NT = 4 (forced on small frames): depth 1..3, D off the 4-step, D = 16 and 17, two and three j0 passes
    "ni-48-D5": lambda: sf(NI, [48], 5),
    "ni-64.32-D16": lambda: sf(NI, [64, 32], 16),
    "ni-16.32.64-D17": lambda: sf(NI, [16, 32, 64], 17),
    "ni-64.32-D69": lambda: grap(NI, [64, 32], 23, (0, 1, 2)),
    "ni-48-D135": lambda: grap(NI, [48], 27, (0, 1, 2, 3, 4)),
    "ni-32.32-D5": lambda: sf(NI, [32, 32], 5),
    "mn-48-D6": lambda: sf(MN, [48], 3),
    "mn-64.32-D16": lambda: sf(MN, [64, 32], 8),
    "mn-16.32.64-D34": lambda: sf(MN, [16, 32, 64], 17),
    "mn-64.32-D102": lambda: grap(MN, [64, 32], 17, (0, 1, 2)),
    # quad, NT = 8 (by itself from the first tile)
    "ni-80-D5": lambda: sf(NI, [80], 5),
    "ni-128.128-D16": lambda: sf(NI, [128, 128], 16),
    "ni-96.128.112-D17": lambda: sf(NI, [96, 128, 112], 17),
    "ni-128.128-D135": lambda: grap(NI, [128, 128], 27, (0, 1, 2, 3, 4)),
    "mn-80-D6": lambda: sf(MN, [80], 3),
    "mn-128.128-D16": lambda: sf(MN, [128, 128], 8),
    "mn-96.128.112-D34": lambda: sf(MN, [96, 128, 112], 17),
    "mn-80.96-D132": lambda: grap(MN, [80, 96], 22, (0, 1, 2)),
    # wave: the 64 KB and 150 KB boundaries of the staged weights
    "ni-32-D5": lambda: sf(NI, [32], 5),
    "ni-32.32-D16": lambda: sf(NI, [32, 32], 16),
    "ni-16.16.16-D13": lambda: sf(NI, [16, 16, 16], 13),
    "ni-32.32-D17": lambda: sf(NI, [32, 32], 17),
    "ni-64.64-D16": lambda: sf(NI, [64, 64], 16),
    "ni-64.64-D37": lambda: sf(NI, [64, 64], 37),
    "ni-64.64-D49": lambda: sf(NI, [64, 64], 49),
    "mn-32-D6": lambda: sf(MN, [32], 3),
    "mn-32.32-D16": lambda: sf(MN, [32, 32], 8),
    "mn-32.32.32-D34": lambda: sf(MN, [32, 32, 32], 17),
    "mn-64.64-D50": lambda: sf(MN, [64, 64], 25),
    "mn-32.32-D10": lambda: sf(MN, [32, 32], 5),
    # generic tile: skips, four hidden layers, widths 129..512
    "ni-48.48r-D5": lambda: sf(NI, [48, 48], 5, resnet=True),
    "ni-32x4-D5": lambda: sf(NI, [32, 32, 32, 32], 5),
    "ni-112.112r-D5": lambda: sf(NI, [112, 112], 5, resnet=True),
    "ni-130.200-D5": lambda: sf(NI, [130, 200], 5),
    "ni-512-D17": lambda: sf(NI, [512], 17),
    "ni-256.256r-D5": lambda: sf(NI, [256, 256], 5, resnet=True),
    "mn-48.48r-D10": lambda: sf(MN, [48, 48], 5, resnet=True),
    "mn-32x4-D10": lambda: sf(MN, [32, 32, 32, 32], 5),
    "mn-112.112r-D10": lambda: sf(MN, [112, 112], 5, resnet=True),
    "mn-130.200-D10": lambda: sf(MN, [130, 200], 5),
    "mn-512-D34": lambda: sf(MN, [512], 17),
    "mn-256.256r-D10": lambda: sf(MN, [256, 256], 5, resnet=True),
    # per-element networks that differ
    "pe-narrow": lambda: sf(MN, {"Mo": [48, 16], "Ni": [32, 64]}, 5),
    "pe-wide": lambda: sf(MN, {"Mo": [80, 96], "Ni": [128, 112]}, 5),
    "pe-nt-differs": lambda: sf(MN, {"Mo": [48], "Ni": [96]}, 5),
    "pe-depths": lambda: sf(MN, {"Mo": [32], "Ni": [16, 24, 40]}, 5),
    # three elements, for the element-layout rows
    "acn-narrow": lambda: sf(ACN, NARROW, 3),
    "acn-wide": lambda: sf(ACN, WIDE, 3),
}
for _act in sorted(_lib.TA_ACT):
    MODELS[f"act-{_act}-narrow"] = lambda a=_act: sf(NI, NARROW, 5, activation=a, seed=21)
    MODELS[f"act-{_act}-wide"] = lambda a=_act: sf(NI, WIDE, 5, activation=a, seed=21)
MODELS["minmax-narrow"] = lambda: flat_channel(sf(NI, NARROW, 5, minmax=True))
MODELS["minmax-wide"] = lambda: flat_channel(sf(NI, WIDE, 5, minmax=True))


@lru_cache(maxsize=None)
def model(key):
    return MODELS[key]()


# -- frames ----------------------------------------------------------------------------------------------------

def labelled(els, counts, seed):
    """fcc Ni positions with exactly counts[e] atoms of els[e], shuffled (surplus lattice sites left empty)."""
    n = sum(counts)
    rep = (2, 2, 2) if n <= 32 else (3, 2, 2)
    atoms = fcc(rep=rep, a=3.52, seed=seed, jitter=0.05)
    syms = [el for el, c in zip(els, counts) for _ in range(c)]
    np.random.RandomState(seed).shuffle(syms)
    return Atoms(symbols=syms, positions=atoms.positions[:n], cell=np.asarray(atoms.get_cell()), pbc=True)


def big_frames(minority=None):
    """33,000 atoms in 66 differently jittered 5 x 5 x 5 fcc frames: 2063 tiles, the last one of 8 atoms; with
    `minority` about a quarter of every frame relabelled to that element."""
    frames = []
    for k in range(66):
        a = fcc(rep=(5, 5, 5), jitter=0.03 + 0.0005 * k, seed=200 + k)
        if minority:
            pick = np.random.RandomState(900 + k).rand(len(a)) < 0.25
            a = Atoms(symbols=[minority if p else "Ni" for p in pick], positions=a.positions,
                      cell=np.asarray(a.get_cell()), pbc=True)
        frames.append(a)
    return frames


FRAMES = {
    # 32 + 45 atoms: five tiles, the last one ragged (13 atoms)
    "ni": lambda: [fcc(rep=(2, 2, 2), jitter=0.05), drop(fcc(rep=(3, 2, 2), a=3.4, seed=2, jitter=0.08), 3)],
    "mn": lambda: [alloy(MN, rep=(2, 2, 2), a=3.52, seed=3), drop(alloy(MN, rep=(2, 2, 3), a=3.52, seed=8), 5)],
    "ni-5000": lambda: [fcc(rep=(5, 5, 5), jitter=0.03 + 0.004 * k, seed=50 + k) for k in range(10)],
    "big-ni": lambda: big_frames(),
    "big-mn": lambda: big_frames("Mo"),
    # element layout (Al, Cu, Ni): an element absent from the batch, elements of 1, 15, 16 and 17 atoms
    "first-absent": lambda: [labelled(ACN, (0, 17, 15), 31), labelled(ACN, (0, 16, 1), 32)],
    "middle-absent": lambda: [labelled(ACN, (15, 0, 17), 33), labelled(ACN, (1, 0, 16), 34)],
    "last-absent": lambda: [labelled(ACN, (17, 15, 0), 35), labelled(ACN, (16, 1, 0), 36)],
    "counts-1-15-16": lambda: [labelled(ACN, (1, 15, 16), 37)],
    "counts-17-16-1": lambda: [labelled(ACN, (17, 16, 1), 38)],
}
LAYOUTS = ["first-absent", "middle-absent", "last-absent", "counts-1-15-16", "counts-17-16-1"]


@lru_cache(maxsize=None)
def frames_of(key):
    return FRAMES[key]()


def _is_grap(nn):
    return type(nn.descriptor).__name__ == "GenericRadialAtomicPotential"


@lru_cache(maxsize=None)
def reference(model_key, frames_key, k):
    """The oracle on frame k, computed once per (model, frames) and shared by the rows that use them."""
    nn = model(model_key)
    return (oracle_grap_eval if _is_grap(nn) else oracle_eval)(nn, frames_of(frames_key)[k])


# -- the table -------------------------------------------------------------------------------------------------

Row = namedtuple("Row", "model frames env launch D where")
TILE, WAVE, QUAD, DA = ENV_SWITCHES


def L(family, threads=0, lh=0, nt=0, da="registers"):
    if family.startswith("quad"):
        threads = 64 * nt
    elif family.startswith("wave"):
        threads = 512
    return dict(family=family, threads=threads, lh=lh, nt=nt, da=da)


ROWS = {
    # -- quad, NT = 4 --
    "quad4-lh1-D5": Row("ni-48-D5", "ni", QUAD, L("quad", lh=1, nt=4), 5, ["j0x1"]),
    "quad4-lh2-D16": Row("ni-64.32-D16", "ni", QUAD, L("quad", lh=2, nt=4), 16, ["j0x1"]),
    "quad4-lh3-D17": Row("ni-16.32.64-D17", "ni", QUAD, L("quad", lh=3, nt=4), 17, ["j0x1"]),
    "quad4-lh2-D69-two-passes": Row("ni-64.32-D69", "ni", QUAD, L("quad", lh=2, nt=4), 69, ["j0x2"]),
    "quad4-lh1-D135-three-passes": Row("ni-48-D135", "ni", QUAD, L("quad", lh=1, nt=4), 135, ["j0x3"]),
    "quad4-by-itself-313-tiles": Row("ni-32.32-D5", "ni-5000", None, L("quad", lh=2, nt=4), 5, ["tiles=313", "j0x1"]),
    "quad4all-lh1-D6": Row("mn-48-D6", "mn", QUAD, L("quad_all", lh=1, nt=4), 6, ["j0x1"]),
    "quad4all-lh2-D16": Row("mn-64.32-D16", "mn", QUAD, L("quad_all", lh=2, nt=4), 16, ["j0x1"]),
    "quad4all-lh3-D34": Row("mn-16.32.64-D34", "mn", QUAD, L("quad_all", lh=3, nt=4), 34, ["j0x1"]),
    "quad4all-lh2-D102-two-passes": Row("mn-64.32-D102", "mn", QUAD, L("quad_all", lh=2, nt=4), 102, ["j0x2"]),
    # -- quad, NT = 8 --
    "quad8-lh1-D5": Row("ni-80-D5", "ni", None, L("quad", lh=1, nt=8), 5, ["j0x1"]),
    "quad8-lh2-D16": Row("ni-128.128-D16", "ni", None, L("quad", lh=2, nt=8), 16, ["j0x1"]),
    "quad8-lh3-D17": Row("ni-96.128.112-D17", "ni", None, L("quad", lh=3, nt=8), 17, ["j0x1"]),
    "quad8-lh2-D135-two-passes": Row("ni-128.128-D135", "ni", None, L("quad", lh=2, nt=8), 135, ["j0x2"]),
    "quad8all-lh1-D6": Row("mn-80-D6", "mn", None, L("quad_all", lh=1, nt=8), 6, ["j0x1"]),
    "quad8all-lh2-D16": Row("mn-128.128-D16", "mn", None, L("quad_all", lh=2, nt=8), 16, ["j0x1"]),
    "quad8all-lh3-D34": Row("mn-96.128.112-D34", "mn", None, L("quad_all", lh=3, nt=8), 34, ["j0x1"]),
    "quad8all-lh2-D132-two-passes": Row("mn-80.96-D132", "mn", None, L("quad_all", lh=2, nt=8), 132, ["j0x2"]),
    # -- wave, forced on small frames --
    "wave-lh1-below-64K": Row("ni-32-D5", "ni", WAVE, L("wave", lh=1), 5, ["wave<=64K"]),
    "wave-lh2-below-64K": Row("ni-32.32-D16", "ni", WAVE, L("wave", lh=2), 16, ["wave<=64K", "wave_lds=56064"]),
    "wave-lh3-below-64K": Row("ni-16.16.16-D13", "ni", WAVE, L("wave", lh=3), 13, ["wave<=64K"]),
    "wave-lh2-just-above-64K": Row("ni-32.32-D17", "ni", WAVE, L("wave", lh=2), 17, ["64K<wave<=150K", "wave_lds=74496"]),
    "wave-lh2-100K": Row("ni-64.64-D16", "ni", WAVE, L("wave", lh=2), 16, ["64K<wave<=150K", "wave_lds=101888"]),
    "wave-lh2-just-below-150K": Row("ni-64.64-D37", "ni", WAVE, L("wave", lh=2), 37,
                                    ["64K<wave<=150K", "wave_lds=138752"]),
    "wave-lh2-above-150K-not-taken": Row("ni-64.64-D49", "ni", WAVE, L("tile", threads=256, da="lds"), 49,
                                         ["wave>150K", "wave_lds=165376", "da-lds"]),
    "waveall-lh1": Row("mn-32-D6", "mn", WAVE, L("wave_all", lh=1), 6, ["wave<=64K"]),
    "waveall-lh2": Row("mn-32.32-D16", "mn", WAVE, L("wave_all", lh=2), 16, ["wave<=64K"]),
    "waveall-lh3-above-64K": Row("mn-32.32.32-D34", "mn", WAVE, L("wave_all", lh=3), 34, ["64K<wave<=150K"]),
    "waveall-above-150K-not-taken": Row("mn-64.64-D50", "mn", WAVE, L("tile_all", threads=256, da="lds"), 50,
                                        ["wave>150K", "da-lds"]),
    # -- wave, by itself, second iteration of the grid-stride loop --
    "wave-by-itself-2063-tiles": Row("ni-32.32-D5", "big-ni", None, L("wave", lh=2), 5,
                                     ["tiles=2063", "grid=256x1", "second-stride-iteration", "ragged-last-tile=8"]),
    "waveall-by-itself-33000-atoms": Row("mn-32.32-D10", "big-mn", None, L("wave_all", lh=2), 10,
                                        ["grid=128x2", "second-stride-iteration"]),
    # -- generic tile --
    "tile256-skip-lds": Row("ni-48.48r-D5", "ni", None, L("tile", threads=256, da="lds"), 5, ["da-lds"]),
    "tile256-four-hidden-lds": Row("ni-32x4-D5", "ni", None, L("tile", threads=256, da="lds"), 5, ["da-lds"]),
    "tile256-skip-global-forced": Row("ni-48.48r-D5", "ni", DA, L("tile", threads=256, da="global"), 5,
                                      ["da-global-forced"]),
    "tile256-skip-global-by-itself": Row("ni-112.112r-D5", "ni", None, L("tile", threads=256, da="global"), 5,
                                         ["da-global-by-itself"]),
    "tile512-130.200": Row("ni-130.200-D5", "ni", None, L("tile", threads=512, da="global"), 5, ["da-global-by-itself"]),
    "tile512-512-wide-131K": Row("ni-512-D17", "ni", None, L("tile", threads=512, da="global"), 17,
                                 ["da-global-by-itself", "lds=131584"]),
    "tile512-256.256-skip": Row("ni-256.256r-D5", "ni", None, L("tile", threads=512, da="global"), 5,
                                ["da-global-by-itself"]),
    "tileall256-skip-lds": Row("mn-48.48r-D10", "mn", None, L("tile_all", threads=256, da="lds"), 10, ["da-lds"]),
    "tileall256-four-hidden-lds": Row("mn-32x4-D10", "mn", None, L("tile_all", threads=256, da="lds"), 10, ["da-lds"]),
    "tileall256-skip-global-forced": Row("mn-48.48r-D10", "mn", DA, L("tile_all", threads=256, da="global"), 10,
                                         ["da-global-forced"]),
    "tileall256-skip-global-by-itself": Row("mn-112.112r-D10", "mn", None, L("tile_all", threads=256, da="global"),
                                            10, ["da-global-by-itself"]),
    "tileall512-130.200": Row("mn-130.200-D10", "mn", None, L("tile_all", threads=512, da="global"), 10,
                              ["da-global-by-itself"]),
    "tileall512-512-wide": Row("mn-512-D34", "mn", None, L("tile_all", threads=512, da="global"), 34,
                               ["da-global-by-itself", "lds=131584"]),
    "tileall512-256.256-skip": Row("mn-256.256r-D10", "mn", None, L("tile_all", threads=512, da="global"), 10,
                                   ["da-global-by-itself"]),
    # -- per-element networks --
    "per-element-quad4all": Row("pe-narrow", "mn", QUAD, L("quad_all", lh=2, nt=4), 10, []),
    "per-element-quad8all": Row("pe-wide", "mn", None, L("quad_all", lh=2, nt=8), 10, []),
    "per-element-waveall": Row("pe-narrow", "mn", WAVE, L("wave_all", lh=2), 10, ["64K<wave<=150K"]),
    "per-element-nt-differs": Row("pe-nt-differs", "mn", None, L("tile_all", threads=256, da="lds"), 10, ["da-lds"]),
    "per-element-nt-differs-forced": Row("pe-nt-differs", "mn", QUAD, L("tile_all", threads=256, da="lds"), 10,
                                         ["da-lds"]),
    "per-element-depths-1-and-3": Row("pe-depths", "mn", QUAD, L("tile_all", threads=256, da="lds"), 10,
                                      ["da-lds", "layers=4"]),
}
for _lay in LAYOUTS:   # element layout, through each `_all` family
    ROWS[f"layout-{_lay}-tileall"] = Row("acn-narrow", _lay, TILE, L("tile_all", threads=256, da="lds"), 9, ["da-lds"])
    ROWS[f"layout-{_lay}-waveall"] = Row("acn-narrow", _lay, WAVE, L("wave_all", lh=2), 9, [])
    ROWS[f"layout-{_lay}-quad4all"] = Row("acn-narrow", _lay, QUAD, L("quad_all", lh=2, nt=4), 9, [])
    ROWS[f"layout-{_lay}-quad8all"] = Row("acn-wide", _lay, None, L("quad_all", lh=2, nt=8), 9, [])
for _m in [f"act-{a}" for a in sorted(_lib.TA_ACT)] + ["minmax"]:   # activations and min-max, one row per family
    ROWS[f"{_m}-tile"] = Row(f"{_m}-narrow", "ni", TILE, L("tile", threads=256, da="lds"), 5, ["da-lds"])
    ROWS[f"{_m}-wave"] = Row(f"{_m}-narrow", "ni", WAVE, L("wave", lh=2), 5, [])
    ROWS[f"{_m}-quad4"] = Row(f"{_m}-narrow", "ni", QUAD, L("quad", lh=2, nt=4), 5, [])
    ROWS[f"{_m}-quad8"] = Row(f"{_m}-wide", "ni", None, L("quad", lh=2, nt=8), 5, [])

BIG = [name for name, row in ROWS.items() if row.frames.startswith("big-")]
SMALL = [name for name in ROWS if name not in BIG]

# every instantiation the dispatcher can choose, and both act' placements of the generic tile
EVERY_BUILD = ({(f, t, 0, 0, da) for f in ("tile", "tile_all") for t, da in ((256, "lds"), (256, "global"), (512, "global"))} |
               {(f, 512, lh, 0, "registers") for f in ("wave", "wave_all") for lh in (1, 2, 3)} |
               {(f, 64 * nt, lh, nt, "registers") for f in ("quad", "quad_all") for lh in (1, 2, 3) for nt in (4, 8)})


# the temperature-dependent head (rows of tests/test_gpu_td.py): both builds, both act' placements
EVERY_TD_BUILD = {("td", 256, 0, 0, "lds"), ("td", 256, 0, 0, "global"), ("td", 512, 0, 0, "global")}


def build_of(launch):
    return (launch["family"], launch["threads"], launch["lh"], launch["nt"], launch["da"])


# -- CPU: the table sits where it says --------------------------------------------------------------------------

def check_where(name, row, nn, frames, got):
    counts, tiles = element_tiles(nn, frames)
    nets = [net_of(nn, el) for el in nn.elements]
    wave_lds = max(wave_lds_bytes(n) for n in nets)
    slab = tile_slab_bytes(nn)
    for claim in row.where:
        key, _, value = claim.partition("=")
        if claim.startswith("j0x"):      # passes of the quad kernel's dE/dG loop, for j0 = 16 nt + 16 NT p < D
            assert got["family"].startswith("quad") and -(-row.D // (16 * got["nt"])) == int(claim[3:]), (name, claim)
        elif key == "tiles":
            assert sum(tiles) == int(value), (name, sum(tiles))
        elif key == "grid":
            assert "%dx%d" % got["grid"] == value, (name, got["grid"])
        elif key == "wave_lds":
            assert wave_lds == int(value), (name, wave_lds)
        elif key == "lds":
            assert got["lds_bytes"] == int(value), (name, got["lds_bytes"])
        elif key == "layers":
            assert max(len(n.kp) for n in nets) == int(value) and len({len(n.kp) for n in nets}) > 1, name
        elif claim == "wave<=64K":
            assert got["family"].startswith("wave") and got["lds_bytes"] == wave_lds <= LDS_64K, (name, wave_lds)
        elif claim == "64K<wave<=150K":
            assert got["family"].startswith("wave") and LDS_64K < got["lds_bytes"] == wave_lds <= LDS_150K, (name, wave_lds)
        elif claim == "wave>150K":       # the shape fits the wave kernel in every respect but the staged bytes
            assert row.env == WAVE and wave_lds > LDS_150K and got["family"].startswith("tile"), (name, wave_lds)
            assert all(1 <= len(n.kp) - 1 <= 3 and max(n.np_[:-1]) <= 64 and not any(n.res) for n in nets), name
        elif claim == "da-lds":
            assert got["da"] == "lds" and slab <= LDS_64K and row.env != DA and got["lds_bytes"] == slab, (name, slab)
        elif claim == "da-global-forced":
            assert got["da"] == "global" and slab <= LDS_64K and row.env == DA, (name, slab)
        elif claim == "da-global-by-itself":
            assert got["da"] == "global" and slab > LDS_64K and row.env is None, (name, slab)
        elif claim == "second-stride-iteration":
            assert got["family"].startswith("wave") and row.env is None
            assert max(tiles) > 8 * got["grid"][0] and sum(tiles) >= 2049, (name, tiles, got["grid"])
        elif key == "ragged-last-tile":
            assert counts[-1] % TILE_ROWS == int(value), (name, counts)
        else:
            raise AssertionError(f"{name}: unknown claim {claim}")


@pytest.mark.parametrize("name", list(ROWS))
def test_rows_sit_where_they_say(name):
    """CPU: each row's model has the D it names, takes the launch it names by the restated dispatch rules, and
    sits on the claimed side of every tile-count and LDS boundary."""
    row = ROWS[name]
    nn, frames = model(row.model), frames_of(row.frames)
    assert nn.ndim() == row.D, (name, nn.ndim())
    got = mirror_launch(nn, frames, row.env)
    assert {k: got[k] for k in row.launch} == row.launch, (name, got)
    check_where(name, row, nn, frames, got)
    counts, tiles = element_tiles(nn, frames)
    if row.frames in ("ni", "mn"):
        assert any(n % TILE_ROWS for n in counts) and len(frames) == 2, (name, counts)   # two frames, a ragged tile
    if row.env is None and got["family"].startswith("quad") and got["nt"] == 4:
        assert QUAD_MIN_TILES <= sum(tiles) < WAVE_MIN_TILES, (name, tiles)


def test_layout_frames_are_what_they_say():
    """CPU: an element absent from the batch as first, middle and last; elements of 1, 15, 16 and 17 atoms."""
    nn = model("acn-narrow")
    got = {key: element_tiles(nn, frames_of(key))[0] for key in LAYOUTS}
    assert got["first-absent"][0] == 0 and got["middle-absent"][1] == 0 and got["last-absent"][2] == 0
    for key in LAYOUTS[:3]:
        assert sorted(got[key]) == [0, 16, 33], (key, got[key])     # one full tile; two full tiles and one atom
    assert got["counts-1-15-16"] == [1, 15, 16] and got["counts-17-16-1"] == [17, 16, 1]


def test_big_frames_reach_the_second_stride_iteration():
    """CPU: 33,000 atoms; Ni alone exceeds the 1024 tiles one pass of its grid row of the alloy covers."""
    for key, nn in (("big-ni", model("ni-32.32-D5")), ("big-mn", model("mn-32.32-D10"))):
        counts, tiles = element_tiles(nn, frames_of(key))
        assert sum(counts) == 33000 and len(frames_of(key)) == 66
        if key == "big-ni":
            assert tiles == [2063] and counts[0] % TILE_ROWS == 8
        else:
            assert 0.2 < counts[0] / 33000 < 0.3 and tiles[1] > 8 * 128 and tiles[0] < 8 * 128, (counts, tiles)


def test_td_slab_rows_sit_where_they_say():
    """CPU: td_plan's byte counts for the rows of tests/test_gpu_td.py: act' in LDS, in the global slab only when
    forced, in the global slab by itself (186,112 B with the slab, 136,192 B without), and the refused model."""
    from tests import test_gpu_td as td
    for name, row in td.SLAB_ROWS.items():
        da_global, where, threads = row[5:]
        plan = td.td_plan_mirror(td.slab_model(name), da_global)
        assert (plan["da"], plan["threads"], plan["refused"]) == (where, threads, False), (name, plan)
        assert (plan["with_da"] <= td.TD_LDS_LIMIT) == (name != "global-by-itself"), (name, plan)
    plan = td.td_plan_mirror(td.slab_model("global-by-itself"))
    assert (plan["with_da"], plan["base"], plan["lds_bytes"]) == (186112, 136192, 136192), plan
    wide = td.td_from(td._sf(["Mo", "Ni"]), *td.TOO_WIDE)
    assert td.td_plan_mirror(wide)["refused"] and td.td_plan_mirror(wide)["base"] == 168960
    counts = td.slab_counts(td.slab_frames())
    assert counts[1][0] == 0 and counts[2][0] == 1                      # Mo absent; a single Mo atom
    assert [sum(c[e] for c in counts) for e in (0, 1)] == [36, 92]      # 3 + 6 tiles, both last tiles ragged


def test_rows_cover_every_build():
    """CPU: the launches the rows name reach each of the twenty instantiations and both act' placements."""
    named = {build_of(row.launch) for row in ROWS.values()}
    assert EVERY_BUILD <= named, sorted(EVERY_BUILD - named)


# -- GPU ----------------------------------------------------------------------------------------------------------

SEEN = {}   # row -> launch the engine reported


def set_switch(monkeypatch, env):
    for name in ENV_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    if env:
        monkeypatch.setenv(env, "1")


def evaluate(name, monkeypatch, descriptors=False, want=None):
    """Evaluate a row's frames under its switch; the reported launch must be the one the row names."""
    from tensoralloy_amd import Engine
    row = ROWS[name]
    nn, frames = model(row.model), frames_of(row.frames)
    set_switch(monkeypatch, row.env)
    with Engine(nn) as eng:
        res = eng.evaluate(frames, want=want, descriptors=descriptors)
        launch = eng.mlp_launch()
    set_switch(monkeypatch, None)
    print(f"LAUNCH {name} {launch}")
    assert launch == mirror_launch(nn, frames, row.env), (name, launch)
    assert {k: launch[k] for k in row.launch} == row.launch, (name, launch)
    SEEN[name] = launch
    return res


def assert_close(r, o, tag):
    """The bounds of tests/test_gpu_td.py::assert_close for a plain model."""
    dev = dict(E=abs(r["energy"] - o["energy"]), e=np.abs(r["atomic"] - o["atomic"]).max(),
               F=np.abs(r["forces"] - o["forces"]).max(), W=np.abs(r["virial"] - o["virial"]).max())
    print(f"DEV {tag} " + " ".join(f"{k}={v:.2e}" for k, v in dev.items()))
    assert dev["E"] <= E_REL * max(1.0, abs(o["energy"])), (tag, dev)
    assert dev["e"] <= E_REL * max(1.0, np.abs(o["atomic"]).max()), (tag, dev)
    assert dev["F"] <= F_REL * max(1.0, np.abs(o["forces"]).max()), (tag, dev)
    assert dev["W"] <= W_REL * max(1.0, np.abs(o["virial"]).max()), (tag, dev)


@gpu
@pytest.mark.parametrize("name", SMALL)
def test_small_rows_against_oracle(lib, monkeypatch, name):
    row = ROWS[name]
    res = evaluate(name, monkeypatch)
    assert len(res) == len(frames_of(row.frames))
    for k, r in enumerate(res):
        assert_close(r, reference(row.model, row.frames, k), f"{name}/frame{k}")


def second_iteration_frame(nn, frames, launch):
    """The frame that holds the first atom of the first tile a wavefront takes in its second iteration: tile
    8 x gridDim.x of the element with the most tiles (tile 2048 of the one-element batch)."""
    counts, tiles = element_tiles(nn, frames)
    el = nn.elements[int(np.argmax(tiles))]
    first = 8 * launch["grid"][0] * TILE_ROWS          # index among the atoms of `el`, in batch order
    assert first < max(counts)
    seen = 0
    for k, a in enumerate(frames):
        n = a.get_chemical_symbols().count(el)
        if seen + n > first:
            return k
        seen += n
    raise AssertionError("not reached")


@gpu
@pytest.mark.parametrize("name", BIG)
def test_second_stride_iteration_of_the_wave_kernels(lib, monkeypatch, name):
    from oracle.sf import apply_mlp
    from tensoralloy_amd import Engine
    row = ROWS[name]
    nn, frames = model(row.model), frames_of(row.frames)
    pin_descriptors(nn, frames[0])
    res = evaluate(name, monkeypatch, descriptors=True)
    launch = SEEN[name]
    assert launch["grid"] == ((256, 1) if len(nn.elements) == 1 else (128, 2)), launch
    # every atom's energy: the network on the GPU's own descriptors, layers in extended precision, result in fp64
    syms = [s for a in frames for s in a.get_chemical_symbols()]
    G = np.concatenate([r["descriptors"] for r in res])
    e_ref, _ = apply_mlp(oracle_model(nn), syms, G.astype(np.longdouble))
    e_got = np.concatenate([r["atomic"] for r in res])
    dev = np.abs(e_got - e_ref)
    print(f"DEV {name} atomic={dev.max():.2e}")
    assert np.all(dev <= E_REL * np.maximum(1.0, np.abs(e_ref))), (name, dev.max())
    # forces and virial: the oracle on the first frame, the first frame of the second iteration, the last frame
    for k in sorted({0, second_iteration_frame(nn, frames, launch), len(frames) - 1}):
        assert_close(res[k], reference(row.model, row.frames, k), f"{name}/frame{k}")
    # every atom's force: one workgroup per tile, no stride loop
    set_switch(monkeypatch, TILE)
    with Engine(nn) as eng:
        tile = eng.evaluate(frames)
        tile_launch = eng.mlp_launch()
    set_switch(monkeypatch, None)
    assert tile_launch == mirror_launch(nn, frames, TILE) and tile_launch["family"].startswith("tile"), tile_launch
    F, Ft = np.concatenate([r["forces"] for r in res]), np.concatenate([r["forces"] for r in tile])
    assert np.all(np.abs(F - Ft) <= CROSS_REL * np.maximum(1.0, np.abs(Ft))), (name, np.abs(F - Ft).max())
    e_tile = np.concatenate([r["atomic"] for r in tile])
    assert np.all(np.abs(e_got - e_tile) <= CROSS_REL * np.maximum(1.0, np.abs(e_tile)))


@gpu
def test_every_build_was_launched(lib, monkeypatch):
    """The launches reported over the table and over the slab rows of tests/test_gpu_td.py (rows that have not run
    in this process are launched here, energies only) reach each of the twenty instantiations, both act'
    placements of the generic tile and both of `td_all_kernel`."""
    from tests import test_gpu_td as td
    for name in ROWS:
        if name not in SEEN:
            evaluate(name, monkeypatch, want=_lib.TA_WANT_ENERGY)
    for name in td.SLAB_ROWS:
        if name not in td.SLAB_SEEN:
            td.slab_launch(name, monkeypatch, td.slab_frames()[:1], want=_lib.TA_WANT_ENERGY)
    seen = {build_of(launch) for launch in list(SEEN.values()) + list(td.SLAB_SEEN.values())}
    assert EVERY_BUILD | EVERY_TD_BUILD <= seen, sorted((EVERY_BUILD | EVERY_TD_BUILD) - seen)
