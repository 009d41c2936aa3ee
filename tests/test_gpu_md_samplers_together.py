"""GPU: all seven samplers of the device MD loop on at once (`md_set_sampling`, `_rdf`, `_adf`, `_order`, `_clusters`,
`_cna`, `_sq`), which no single-feature test sees. The samplers share one host-side lifecycle (csrc/ta_api_md.hip): one
allocation skeleton, one loop over them in `ta_md_init` and `ta_md_run`. What that could break shows only when several
are on: a schedule that is not restored, buffers of one released with another's, a snapshot shared wrongly between the
correlation ring and the structure factors.

Expectation: every getter returns, bit for bit (`np.array_equal`, integers and doubles alike), what an engine running
that feature ALONE on the same trajectory returns. The launches only read the state and every sampler's sums are
ordered by its own fixed layout, which is what the single-feature tests' bitwise "the feature does not disturb the
trajectory" checks rely on. Only public `Engine.md_*` calls are used. This held bit for bit, for every output, on the
library as it was before the samplers shared their lifecycle.

Protocol (a few seconds): two fcc Ni frames of different size, a skin small enough that the list is rebuilt inside the
runs, different `sample_every` (1, 2, 3, 2, 4, 3, 2), clusters with n_min > 0 (they read the order launches' n_conn),
S(q) with currents (its snapshot is the correlation ring's on common steps, its own on the others); runs of 7 and 6
steps, then `set_frames` with the frames swapped, `md_init` (every sampler is allocated again from its stored setting)
and a run of 6 steps. Every getter is read after each of the three stages.

The last test is about the place the integrator writes a sampled state to (the correlation ring, the rows of
`md_set_sq`, the rows of `md_set_flux`): one run that takes all three while all three readers are on."""
import functools

import numpy as np
import pytest

from tests.helpers import fcc, make_eam
from tests.test_gpu_md import DT, _velocities

pytestmark = pytest.mark.gpu

SKIN = 0.07     # the fastest atom moves 0.0136 A per step: past skin / 2 at every third step or so
T0 = 1500.0
RUNS = (7, 6)      # before set_frames + md_init
RERUN = 6          # behind them
MILLER = np.array([[1, 0, 0], [0, 1, 0], [1, 1, 0], [1, 1, 1], [2, 0, 1]], dtype=np.int32)

# in the library's canonical order; n_lags = 4 of the correlations is below the samples of every stage (no NaN in the
# normalised sums, which np.array_equal would not take for equal)
SETTINGS = {
    "sampling": dict(n_lags=4, sample_every=1),
    "rdf": dict(n_bins=32, sample_every=2),
    "adf": dict(n_bins=24, r_bond=3.0, sample_every=3),
    "order": dict(degrees=(4, 6), r_bond=3.0, n_bins=16, sample_every=2),
    "clusters": dict(r_link=3.0, n_min=6, n_bins=8, n_series=3, sample_every=4),
    "cna": dict(mode="adaptive", n_series=2, sample_every=3),
    "sq": dict(miller=MILLER, n_lags=3, sample_every=2, currents=True),
}
OFF = {
    "sampling": dict(n_lags=0), "rdf": dict(n_bins=0), "adf": dict(n_bins=0), "order": dict(n_bins=0),
    "clusters": dict(n_bins=0), "cna": dict(n_series=0), "sq": dict(miller=None),
}
GETTERS = {
    "sampling": ("md_correlations", "md_samples"), "rdf": ("md_rdf",), "adf": ("md_adf",),
    "order": ("md_order", "md_order_atoms"), "clusters": ("md_clusters", "md_cluster_atoms"),
    "cna": ("md_cna", "md_cna_atoms"), "sq": ("md_sq", "md_sq_amplitudes"),
}
NAMES = tuple(SETTINGS)
NEEDS = {"clusters": ("order", "clusters")}   # n_min > 0 reads n_conn of the order launches


@functools.lru_cache(maxsize=None)
def _setup():
    nn = make_eam(["Ni"], 6.0, potential="zjw04")
    frames = (fcc(rep=(2, 2, 2)), fcc(rep=(3, 2, 2)))
    v = tuple(_velocities([a], T0, 3 + j) for j, a in enumerate(frames))
    return nn, frames, v


def _collect(eng, names):
    return {g: getattr(eng, g)() for name in names for g in GETTERS[name]}


def _protocol(on, switch_off=False):
    """The protocol with the samplers `on`: per stage the trajectory's end and records and every getter's output. With
    `switch_off` also, behind the last stage, what the getters of the samplers still on return after each sampler in
    turn has been switched off."""
    from tensoralloy_amd import Engine
    nn, frames, v = _setup()
    stages, after_off = [], []
    with Engine(nn) as eng:
        eng.set_skin(SKIN)

        def stage(n):
            out = eng.md_run(n, DT)
            x, vel = eng.md_state()
            stages.append(dict(x=x, v=vel, epot=out["epot"], ekin=out["ekin"], n_rebuilds=out["n_rebuilds"],
                               got=_collect(eng, on)))

        eng.set_frames(list(frames))
        eng.md_init(None, np.concatenate(v))
        for name in NAMES:
            if name in on:
                getattr(eng, "md_set_" + name)(**SETTINGS[name])
        for n in RUNS:
            stage(n)
        eng.set_frames(list(frames[::-1]))
        eng.md_init(None, np.concatenate(v[::-1]))
        stage(RERUN)
        if switch_off:
            left = list(on)
            for name in on:
                getattr(eng, "md_set_" + name)(**OFF[name])
                left.remove(name)
                after_off.append((name, _collect(eng, left)))
    return stages, after_off


@functools.lru_cache(maxsize=None)
def _together():
    return _protocol(NAMES, switch_off=True)


def _same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    return type(a) is type(b) and a == b


def _differing(got, want):
    """The keys `getter.key` on which two collections differ."""
    assert got.keys() == want.keys()
    bad = []
    for g in got:
        assert got[g].keys() == want[g].keys(), g
        bad += [f"{g}.{k}" for k in got[g] if not _same(got[g][k], want[g][k])]
    return bad


def test_the_lists_are_rebuilt_inside_the_runs():
    stages, _ = _together()
    print("n_rebuilds per stage", [s["n_rebuilds"] for s in stages])
    assert 0 < stages[1]["n_rebuilds"] < RUNS[1]   # launches replayed behind a rebuild, and launches on a list that held


@pytest.mark.parametrize("name", NAMES)
def test_together_equals_alone(name):
    together, _ = _together()
    alone, _ = _protocol(NEEDS.get(name, (name,)))
    for j, (t, a) in enumerate(zip(together, alone)):
        # the same trajectory: no sampler disturbs it
        assert all(np.array_equal(t[k], a[k]) for k in ("x", "v", "epot", "ekin")) and t["n_rebuilds"] == a["n_rebuilds"], j
        got = {g: t["got"][g] for g in GETTERS[name]}
        want = {g: a["got"][g] for g in GETTERS[name]}
        bad = _differing(got, want)
        print("stage", j, name, "differing outputs:", bad)
        assert not bad, (j, bad)


def test_steps_against_enumeration():
    together, _ = _together()
    ends = [RUNS[0], RUNS[0] + RUNS[1], RERUN]   # md_init sets the clock back to 0
    for stage, end in zip(together, ends):
        got = stage["got"]
        for name in NAMES:
            steps = list(range(0, end + 1, SETTINGS[name]["sample_every"]))
            head = got[GETTERS[name][0]]
            assert (head["n_samples"], head["sample_every"], head["last_step"]) == \
                (len(steps), SETTINGS[name]["sample_every"], steps[-1]), (name, end)
        for getter, rows in (("md_samples", SETTINGS["sampling"]["n_lags"]), ("md_clusters", SETTINGS["clusters"]["n_series"]),
                             ("md_cna", SETTINGS["cna"]["n_series"]), ("md_sq_amplitudes", SETTINGS["sq"]["n_lags"])):
            name = next(n for n in NAMES if getter in GETTERS[n])
            steps = list(range(0, end + 1, SETTINGS[name]["sample_every"]))
            assert got[getter]["steps"].tolist() == steps[-rows:], (getter, end)
        for name, getter in (("order", "md_order_atoms"), ("clusters", "md_cluster_atoms"), ("cna", "md_cna_atoms")):
            assert got[getter]["step"] == end // SETTINGS[name]["sample_every"] * SETTINGS[name]["sample_every"], (getter, end)


def test_switching_one_off_leaves_the_others():
    stages, after_off = _together()
    before = stages[-1]["got"]
    assert [name for name, _ in after_off] == list(NAMES)
    for name, got in after_off:
        want = {g: before[g] for g in got}
        bad = _differing(got, want)
        print("after", name, "went off, differing outputs:", bad)
        assert not bad, (name, bad)
    assert after_off[-1][1] == {}


# -- the three places the integrator writes a sampled state to, all taken in one run ------------------------------------
# With sample_every = 1 of md_set_sampling (above) every sampled state goes to the correlation ring. Here the ring takes
# the steps t % 4 == 0, the rows of md_set_sq those with t % 4 == 2 and the rows of md_set_flux the odd ones, while all
# three readers of the snapshot are on. md_set_flux is on in every run compared: it switches the builds of the
# evaluation, and with them the trajectory's rounding.
ROUTES = {
    "sampling": dict(n_lags=3, sample_every=4),
    "sq": dict(miller=MILLER, n_lags=3, sample_every=2, currents=True),
    "flux": dict(n_lags=3, sample_every=1),
}
ROUTE_GETTERS = {"sampling": ("md_correlations", "md_samples"), "sq": ("md_sq", "md_sq_amplitudes"),
                 "flux": ("md_flux", "md_flux_rows")}


def _routes_protocol(on):
    """Runs of 7 and 6 steps with the samplers `on` at the settings of ROUTES: per run the trajectory's end and records
    and every getter's output."""
    from tensoralloy_amd import Engine
    nn, frames, v = _setup()
    stages = []
    with Engine(nn) as eng:
        eng.set_skin(SKIN)
        eng.set_frames(list(frames))
        eng.md_init(None, np.concatenate(v))
        for name in on:
            getattr(eng, "md_set_" + name)(**ROUTES[name])
        for n in RUNS:
            out = eng.md_run(n, DT)
            x, vel = eng.md_state()
            stages.append(dict(x=x, v=vel, epot=out["epot"], n_rebuilds=out["n_rebuilds"],
                               got={g: getattr(eng, g)() for name in on for g in ROUTE_GETTERS[name]}))
    return stages


def _same_bits(a, b):
    """np.array_equal; the normalised sums of a lag that has no time origin yet are NaN on both sides, which counts as
    equal."""
    if isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.dtype.kind in "fc":
        return np.array_equal(a, b, equal_nan=True)
    return _same(a, b)


def test_all_three_snapshot_routes_in_one_run():
    """One trajectory of 13 steps in which the correlation ring (t % 4 == 0), the rows of md_set_sq (t % 4 == 2) and the
    rows of md_set_flux (odd t) each take the integrator's snapshot, with all three readers on: every output of the six
    getters equals, bit for bit, that of the same protocol with only that sampler and md_set_flux on, where the
    snapshots take other routes (S(q) alone: its own rows at every sample; flux alone: its own rows always)."""
    together = _routes_protocol(tuple(ROUTES))
    print("n_rebuilds per run", [s["n_rebuilds"] for s in together])
    assert 0 < together[1]["n_rebuilds"] < RUNS[1]
    ends = [RUNS[0], RUNS[0] + RUNS[1]]
    for stage, end in zip(together, ends):
        for name, (head, ring) in ROUTE_GETTERS.items():
            every, steps = ROUTES[name]["sample_every"], list(range(0, end + 1, ROUTES[name]["sample_every"]))
            got = stage["got"][head]
            assert (got["n_samples"], got["sample_every"], got["last_step"]) == (len(steps), every, steps[-1]), (name, end)
            assert stage["got"][ring]["steps"].tolist() == steps[-ROUTES[name]["n_lags"]:], (name, end)
    # all three routes are taken, each by more than one launch
    taken = {route: [t for t in range(ends[-1] + 1) if cond(t)] for route, cond in
             (("ring", lambda t: t % 4 == 0), ("sq rows", lambda t: t % 4 == 2), ("flux rows", lambda t: t % 2 == 1))}
    assert all(len(ts) > 1 for ts in taken.values()), taken
    for name in ROUTES:
        alone = _routes_protocol((name,) if name == "flux" else (name, "flux"))
        for j, (t, a) in enumerate(zip(together, alone)):
            assert all(np.array_equal(t[k], a[k]) for k in ("x", "v", "epot")) and t["n_rebuilds"] == a["n_rebuilds"], (name, j)
            for g in ROUTE_GETTERS[name]:
                assert t["got"][g].keys() == a["got"][g].keys(), g
                bad = [k for k in t["got"][g] if not _same_bits(t["got"][g][k], a["got"][g][k])]
                print("run", j, g, "differing outputs:", bad)
                assert not bad, (j, g, bad)
