"""
The two bodies of the 16-row tile kernels (csrc/ta_mlp_tile.h), against the oracle and against each other.

`mlp_kernel<256/512>` and `mlp_all_kernel<256/512>` run `mlp_tile_scalar` for a network of hidden layers without
skip connections and one linear output unit (no padded 1-column GEMMs, no elementwise passes, energies summed
from per-tile partial sums in a fixed order) and the generic `mlp_tile` for every other network or when
`TA_MLP_TILE_GENERIC=1` is set. The launch geometry is the same either way, so `Engine.mlp_launch()` cannot tell
the bodies apart; `Engine.mlp_tile_body()` does.

Every case evaluates the small frames of tests/test_gpu_mlp_dispatch.py (32 + 45 atoms: five tiles, the last one
ragged) by the dispatch its switch gives, asserts the reported launch against `tests.helpers.mirror_launch` and the
reported body against the case, holds energy, per-atom energies, forces and virial to the oracle at the bounds of
tests/test_gpu_td.py::assert_close (1e-9 x max(1, |ref|), virial 1e-8), and evaluates once more under
`TA_MLP_TILE_GENERIC=1`: the two bodies agree to CROSS_REL = 1e-10 x max(1, |value|).
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import pytest

from tensoralloy_amd import _lib
from tests.helpers import mirror_launch, net_of, oracle_eval
from tests.test_gpu_mlp_dispatch import (CROSS_REL, DA, E_REL, MN, NI, TILE, assert_close, flat_channel, frames_of,
                                         set_switch, sf)

gpu = pytest.mark.gpu

GENERIC = "TA_MLP_TILE_GENERIC"
ENERGY_ONLY = _lib.TA_WANT_ENERGY | _lib.TA_WANT_ATOMIC

Case = namedtuple("Case", "model frames env body family threads da mode")


def case(model, frames="ni", env=None, body="scalar", family="tile", threads=256, da="lds", mode="full"):
    return Case(model, frames, env, body, family, threads, da, mode)


CASES = {
    "a-bench-net-8-64-64-1": case(lambda: sf(NI, [64, 64], 8)),
    "b-one-hidden-48-D5": case(lambda: sf(NI, [48], 5)),
    "c-three-hidden-16.32.64": case(lambda: sf(NI, [16, 32, 64], 5)),
    "d-four-hidden-32x4": case(lambda: sf(NI, [32] * 4, 5)),
    "e-padded-widths-20.50": case(lambda: sf(NI, [20, 50], 5)),
    "f-tanh": case(lambda: sf(NI, [24, 40], 5, activation="tanh", seed=21)),
    "f-elu": case(lambda: sf(NI, [24, 40], 5, activation="elu", seed=21)),
    "f-squareplus": case(lambda: sf(NI, [24, 40], 5, activation="squareplus", seed=21)),
    "g-minmax-flat-channel": case(lambda: flat_channel(sf(NI, [24, 40], 5, minmax=True))),
    "h-D37-three-grad-tiles": case(lambda: sf(NI, [64, 64], 37)),
    "i-width-128-512-threads": case(lambda: sf(NI, [128, 128], 16), env=TILE, threads=512, da="global"),
    "j-act-slab-global": case(lambda: sf(NI, [64, 64], 8), env=DA, da="global"),
    "k-resnet": case(lambda: sf(NI, [48, 48], 5, resnet=True), body="generic"),
    "l-two-elements-depths-1-and-3": case(lambda: sf(MN, {"Mo": [32], "Ni": [16, 24, 40]}, 5), frames="mn",
                                          family="tile_all"),
    "m-energy-only": case(lambda: sf(NI, [64, 64], 8), mode="energy"),
    "n-reuse-descriptors": case(lambda: sf(NI, [64, 64], 8), mode="reuse"),
}


@lru_cache(maxsize=None)
def model(name):
    return CASES[name].model()


@lru_cache(maxsize=None)
def reference(name, k):
    """The oracle on frame k of a case, computed once."""
    return oracle_eval(model(name), frames_of(CASES[name].frames)[k])


def scalar_ok(net):
    """mlp_tile_scalar_ok (ta_mlp_tile.h): at least one hidden layer, no skip connection, one linear output unit
    (tests.helpers.net_of builds every network with that output layer)."""
    return len(net.kp) >= 2 and not any(net.res)


@pytest.mark.parametrize("name", list(CASES))
def test_cases_sit_where_they_say(name):
    """CPU: every case takes a tile launch of the named family, threads and act' placement by the restated
    dispatch rules, and its networks have the shape of the body it names."""
    c = CASES[name]
    nn, frames = model(name), frames_of(c.frames)
    got = mirror_launch(nn, frames, c.env)
    assert (got["family"], got["threads"], got["da"]) == (c.family, c.threads, c.da), (name, got)
    nets = [net_of(nn, el) for el in nn.elements]
    assert all(scalar_ok(n) for n in nets) == (c.body == "scalar"), name
    counts = [sum(a.get_chemical_symbols().count(el) for a in frames) for el in nn.elements]
    assert any(n % 16 for n in counts) and got["grid"][0] > 1, (name, counts)      # a ragged tile, several tiles
    if name.startswith("h-"):
        assert nets[0].kp[0] == 48                       # three 16-column dE/dG tiles, several k-steps in layer 0
    if name.startswith("e-"):
        assert nets[0].np_[:2] == [32, 64] and list(nn.hidden_sizes["Ni"]) == [20, 50]
    if name.startswith("l-"):
        assert sorted(len(n.kp) for n in nets) == [2, 4]


def run(name, monkeypatch, generic):
    """Evaluate a case under its switch, with or without TA_MLP_TILE_GENERIC=1; the launch and the body checked."""
    from tensoralloy_amd import Engine
    c = CASES[name]
    nn, frames = model(name), frames_of(c.frames)
    set_switch(monkeypatch, c.env)
    if generic:
        monkeypatch.setenv(GENERIC, "1")
    else:
        monkeypatch.delenv(GENERIC, raising=False)
    with Engine(nn) as eng:
        if c.mode == "energy":
            res = eng.evaluate(frames, want=ENERGY_ONLY)
        else:
            res = eng.evaluate(frames)
        if c.mode == "reuse":       # the head alone, on the descriptors the evaluation above left behind
            full = res
            eng.compute(ENERGY_ONLY | _lib.TA_WANT_REUSE_DESCRIPTORS)
            res = eng._per_frame(eng.fetch(ENERGY_ONLY))
            for r, f in zip(res, full):
                assert abs(r["energy"] - f["energy"]) <= CROSS_REL * max(1.0, abs(f["energy"]))
        launch, body = eng.mlp_launch(), eng.mlp_tile_body()
    set_switch(monkeypatch, None)
    monkeypatch.delenv(GENERIC, raising=False)
    print(f"LAUNCH {name} generic={int(generic)} {launch} body={body}")
    assert launch == mirror_launch(nn, frames, c.env), (name, launch)
    assert body == ("generic" if generic else c.body), (name, body)
    return res


def close_energies(r, o, tag):
    dev = dict(E=abs(r["energy"] - o["energy"]), e=np.abs(r["atomic"] - o["atomic"]).max())
    print(f"DEV {tag} " + " ".join(f"{k}={v:.2e}" for k, v in dev.items()))
    assert dev["E"] <= E_REL * max(1.0, abs(o["energy"])), (tag, dev)
    assert dev["e"] <= E_REL * max(1.0, np.abs(o["atomic"]).max()), (tag, dev)


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_bodies_against_oracle_and_each_other(lib, monkeypatch, name):
    c = CASES[name]
    res = run(name, monkeypatch, generic=False)
    assert len(res) == len(frames_of(c.frames))
    for k, r in enumerate(res):
        if c.mode == "full":
            assert_close(r, reference(name, k), f"{name}/frame{k}")
        else:
            close_energies(r, reference(name, k), f"{name}/frame{k}")
    other = run(name, monkeypatch, generic=True)
    keys = ("energy", "atomic", "forces", "virial") if c.mode == "full" else ("energy", "atomic")
    for k, (r, g) in enumerate(zip(res, other)):
        for key in keys:
            a, b = np.asarray(r[key], dtype=float), np.asarray(g[key], dtype=float)
            dev = np.abs(a - b)
            print(f"CROSS {name}/frame{k} {key}={dev.max():.2e}")
            assert np.all(dev <= CROSS_REL * np.maximum(1.0, np.abs(b))), (name, k, key, dev.max())
