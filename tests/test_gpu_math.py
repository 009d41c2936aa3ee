"""GPU: the device math every kernel family shares (csrc/ta_math.h, ta_dual.h, ta_reduce.h), one primitive at a
time through the probe library (tests/native/math_probe.hip, compiled with the library's flags), against a
50-digit reference from the defining formulas (tests/math_reference.py).

The bounds are set from an IEEE emulation of the same arithmetic against long double (exp 0.87 ulp, softplus
2.96 / 2.50 ulp, rcp_1_3 0.5 ulp, cosine cutoff 1.9e-16 / 9.2e-16 / 2.5e-15, polynomial cutoff 1.6e-15 / 8.3e-16 /
3.0e-15) with a factor of about two on top, from <= 2 ulp per libm call, and from the rounding steps of each
formula; none of them from what the device returned. profiles/device_math_accuracy.md holds the measured maxima.
Every test prints its figures before it asserts."""
import json
import os

import numpy as np
import pytest

from tensoralloy_amd import _lib
from tests import math_reference as R
from tests.math_probe import DUAL_OPS, PLAIN, call

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def report(what, value, bound):
    print(f"[device math] {what}: {value:.4g} (bound {bound:.4g})")


def worst(err, x):
    """max of err and the input where it sits (for the failure message)."""
    k = int(np.nanargmax(err))
    return float(err[k]), float(np.ravel(x)[k])


# -- ta_exp ----------------------------------------------------------------------------------------------------

def test_exp_against_reference():
    x = R.exp_grid()
    assert len(x) <= 2 ** 17
    got = call("mp_exp", x)[0]
    ref = R.exp_ref(x)
    assert np.all(np.isfinite(got)) and np.all(got >= 0.0)
    normal = np.abs(ref.hi) >= 2.0 ** -1022
    e_n, at_n = worst(np.where(normal, R.err_ulp(got, ref), 0.0), x)
    e_s, at_s = worst(np.where(normal, 0.0, R.err_abs(got, ref)) / R.TINY, x)
    report("ta_exp, normal results, ulp", e_n, 1.5)
    report("ta_exp, subnormal results, units of 2^-1074", e_s, 2.0)
    assert e_n <= 1.5, (e_n, at_n)
    assert e_s <= 2.0, (e_s, at_s)
    assert got[x == 0.0].tolist() == [1.0] * int(np.sum(x == 0.0))


def test_exp_is_zero_far_below_and_keeps_nan():
    x = R.exp_zero_grid()
    assert x.min() >= -1e6 and x.max() <= -746.0
    got = call("mp_exp", x)[0]
    assert np.all(bits(got) == 0), x[bits(got) != 0][:5]
    assert np.all(np.isnan(call("mp_exp", np.array([np.nan, -np.nan]))[0]))


# -- cutoffs ---------------------------------------------------------------------------------------------------

CUTOFF_BOUNDS = {"cosine": (4e-16, 2e-15, 5e-15), "polynomial": (3.2e-15, 1.7e-15, 6e-15)}


@pytest.mark.parametrize("kind", sorted(_lib.TA_CUTOFF))
def test_cutoff_against_reference(kind):
    u = R.cutoff_grid()
    f1, df1, f2, df2, d2f2, fv = call("mp_cutoff", u, arg=_lib.TA_CUTOFF[kind])
    assert np.array_equal(bits(f1), bits(f2)) and np.array_equal(bits(f1), bits(fv))
    assert np.array_equal(bits(df1), bits(df2))
    for name, got, ref, bound in zip(("f", "df/du", "d2f/du2"), (f1, df1, d2f2), R.cutoff_ref(kind, u),
                                     CUTOFF_BOUNDS[kind]):
        e, at = worst(R.err_abs(got, ref), u)
        report(f"{kind} cutoff, {name}, absolute", e, bound)
        assert e <= bound, (kind, name, e, at)
    assert f1[u == 0.0].tolist() == [1.0]
    last = call("mp_cutoff", np.array([1.0 - 2.0 ** -53]), arg=_lib.TA_CUTOFF[kind])
    assert last[0, 0] >= 0.0 and last[2, 0] >= 0.0 and last[5, 0] >= 0.0


# -- rcp_1_3 ---------------------------------------------------------------------------------------------------

def test_rcp_1_3_against_reference():
    d = R.rcp_grid()
    got = call("mp_rcp_1_3", d)[0]
    e, at = worst(R.err_ulp(got, R.rcp_ref(d)), d)
    report("rcp_1_3, ulp", e, 1.0)
    assert e <= 1.0, (e, at)
    assert got[d == 1.0].tolist() == [1.0] and got[d == 2.0].tolist() == [0.5]


# -- softplus_fn -----------------------------------------------------------------------------------------------

def test_softplus_against_reference():
    x = R.softplus_grid()
    h, dh = call("mp_softplus", x)
    rh, rdh = R.softplus_ref(x)
    inner = np.abs(x) <= 700.0
    e_h, at_h = worst(np.where(inner, R.err_ulp(h, rh), 0.0), x)
    e_d, at_d = worst(np.where(inner, R.err_ulp(dh, rdh), 0.0), x)
    report("softplus_fn, h, |x| <= 700, ulp", e_h, 4.0)
    report("softplus_fn, dh, |x| <= 700, ulp", e_d, 4.0)
    assert e_h <= 4.0, (e_h, at_h)
    assert e_d <= 4.0, (e_d, at_d)
    # |x| > 700: absolute bounds
    bound_h = 4.0 * R.ulp_of(np.maximum(x, 0.0)) + 2.0 ** -1020
    bound_d = np.where(x > 0.0, 4.0 * 2.0 ** -52, 2.0 ** -1020)
    o_h, at_oh = worst(np.where(inner, 0.0, R.err_abs(h, rh) / bound_h), x)
    o_d, at_od = worst(np.where(inner, 0.0, R.err_abs(dh, rdh) / bound_d), x)
    report("softplus_fn, h, |x| > 700, share of its absolute bound", o_h, 1.0)
    report("softplus_fn, dh, |x| > 700, share of its absolute bound", o_d, 1.0)
    assert o_h <= 1.0, (o_h, at_oh)
    assert o_d <= 1.0, (o_d, at_od)
    assert np.all((dh >= 0.0) & (dh <= 1.0))
    assert np.all(h >= np.maximum(x, 0.0))


# -- activation_fn, activation_fn2 -----------------------------------------------------------------------------

def _act_code(name):
    return _lib.TA_ACT.get(name, max(_lib.TA_ACT.values()) + 1)      # anything else: the linear default


def test_activation_names_cover_the_library():
    assert sorted(R.ACTIVATIONS) == sorted(list(_lib.TA_ACT) + ["linear"])
    assert sorted(R.LIBM_ACTIVATIONS + R.RATIONAL_ACTIVATIONS + ("softplus",)) == sorted(R.ACTIVATIONS)


@pytest.mark.parametrize("name", R.ACTIVATIONS)
def test_activation_against_reference(name):
    x = R.activation_grid()
    h1, dh1, h, dh, d2h = call("mp_activation", x, arg=_act_code(name))
    assert np.array_equal(bits(h1), bits(h)) and np.array_equal(bits(dh1), bits(dh))
    rh, rdh, rd2h = R.activation_ref(name, x)
    if name in R.LIBM_ACTIVATIONS:
        t1, t2 = R.activation_terms(name, x)
        checks = [("h, ulp", R.err_ulp(h, rh), 4.0),
                  ("dh, share of 16 x 2^-53 x max|term|", _share(R.err_abs(dh, rdh), 16.0 * EPS * t1), 1.0),
                  ("d2h, share of 16 x 2^-53 x max|term|", _share(R.err_abs(d2h, rd2h), 16.0 * EPS * t2), 1.0)]
    elif name == "softplus":    # h and dh as softplus_fn; d2h = dh (1 - dh): terms dh, dh^2
        checks = [("h, ulp", R.err_ulp(h, rh), 4.0), ("dh, ulp", R.err_ulp(dh, rdh), 4.0),
                  ("d2h, share of 16 x 2^-53 x max|term|", _share(R.err_abs(d2h, rd2h), 16.0 * EPS * rdh.hi), 1.0)]
    else:
        checks = [("h, ulp", R.err_ulp(h, rh), 4.0), ("dh, ulp", R.err_ulp(dh, rdh), 4.0),
                  ("d2h, ulp", R.err_ulp(d2h, rd2h), 4.0)]
    results = [(what, *worst(err, x), bound) for what, err, bound in checks]
    for what, e, at, bound in results:
        report(f"{name}, {what}", e, bound)
    for what, e, at, bound in results:
        assert e <= bound, (name, what, e, at)


def _share(err, bound):
    """err / bound, 0 where both are 0 (an exact constant)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(err == 0.0, 0.0, err / bound)


PIECEWISE_AT_ZERO = {   # name: (h, dh, d2h) at x = +-0 (oracle/sf.py::activation, oracle/train.py::activation2)
    "relu": (0.0, 0.0, 0.0), "leaky_relu": (0.0, 0.2, 0.0), "softsign": (0.0, 1.0, 0.0), "elu": (0.0, 1.0, 1.0),
    "linear": (0.0, 1.0, 0.0), "squareplus": (1.0, 0.5, 0.25),
}


@pytest.mark.parametrize("name", sorted(PIECEWISE_AT_ZERO))
def test_piecewise_activations_around_zero(name):
    from oracle.sf import activation
    from oracle.train import activation2
    t = 2.0 ** -30
    x = np.array([0.0, -0.0, t, -t, 5e-324, -5e-324])
    _, _, h, dh, d2h = call("mp_activation", x, arg=_act_code(name))
    for k in (0, 1):
        assert (h[k], dh[k], d2h[k]) == PIECEWISE_AT_ZERO[name], (name, x[k], h[k], dh[k], d2h[k])
    if name != "linear":
        oh, odh = activation(name, x)
        od2h = activation2(name, x)
        for got, ref in ((h, oh), (dh, odh), (d2h, od2h)):
            assert np.all(np.abs(got - ref) <= 4.0 * R.ulp_of(ref)), (name, got, ref)
    sides = {"relu": ((t, 1.0, 0.0), (0.0, 0.0, 0.0)), "leaky_relu": ((t, 1.0, 0.0), (-0.2 * t, 0.2, 0.0))}
    if name in sides:
        assert (h[2], dh[2], d2h[2]) == sides[name][0] and (h[3], dh[3], d2h[3]) == sides[name][1]
    if name == "softsign":
        assert d2h[2] < -1.99 and d2h[3] > 1.99 and d2h[4] == -2.0 and d2h[5] == 2.0
    if name == "elu":
        assert (h[2], dh[2], d2h[2]) == (t, 1.0, 0.0) and 0.0 < d2h[3] < 1.0 and h[3] < 0.0


# -- pow_int_m1, safe_pow --------------------------------------------------------------------------------------

def test_pow_int_m1_against_reference():
    base, zi = R.pow_int_grid()
    got = call("mp_pow_int_m1", base, zi)[0]
    err = R.err_ulp(got, R.pow_int_ref(base, zi))
    share = _share(err, zi - 1.0)
    e, at = worst(err, base)
    report("pow_int_m1, ulp (bound zi - 1 per point)", e, 63.0)
    assert np.all(err <= zi - 1.0), (float(share.max()), at)
    assert np.all(got[zi == 1.0] == 1.0) and np.all(bits(got[zi == 2.0]) == bits(base[zi == 2.0]))
    assert np.all(got[(base == 0.0) & (zi > 1.0)] == 0.0)


@pytest.mark.parametrize("safe", [0, 1])
def test_safe_pow_against_reference(safe):
    x, y = R.safe_pow_grid()
    value = call("mp_safe_pow", x, y, arg=safe)[0]
    grad = call("mp_safe_pow", x, y - 1.0, arg=safe)[1]
    rv, rg = R.safe_pow_ref(safe, x, y)
    for what, got, ref in (("value", value, rv), ("gradient factor", grad, rg)):
        finite = np.isfinite(ref.hi)
        assert np.array_equal(np.isnan(got), np.isnan(ref.hi)), (what, x[np.isnan(got) != np.isnan(ref.hi)])
        assert np.array_equal(got[np.isinf(ref.hi)], ref.hi[np.isinf(ref.hi)]), what
        e, at = worst(np.where(finite, R.err_ulp(got, ref), 0.0), x)
        report(f"safe_pow {what}, safe = {safe}, ulp", e, 2.0)
        assert e <= 2.0, (what, e, at)
    # the rules of the header comment, literally
    neg_frac = (x < 0.0) & (y != np.floor(y))
    assert np.all(np.isnan(value[neg_frac])) and neg_frac.sum() == 2
    zero_neg = (x == 0.0) & (y < 0.0)
    assert np.all(value[zero_neg] == (0.0 if safe else np.inf))
    assert np.all(grad[(x == 0.0) & (y < 1.0)] == (0.0 if safe else np.inf))
    if safe:
        assert np.all(grad[neg_frac] == 0.0) and np.all(np.isfinite(grad))
    else:
        assert np.all(np.isnan(grad[neg_frac]))
    tiny = (x == 1e-300) & (y == -1.5)
    assert value[tiny][0] == (0.0 if safe else np.inf)


# -- cross-lane sums -------------------------------------------------------------------------------------------

WIDTHS = ((0, 16), (1, 32), (2, 64))     # output row of mp_lane_sums, group width


def test_lane_sums_of_integers_stay_inside_their_group():
    lanes = np.arange(256)
    v = (lanes * 7 + 3) % 251 + 1000.0 * (lanes // 16)       # distinct, every group has a total of its own
    assert len(set(v.tolist())) == 256
    out = call("mp_lane_sums", v)
    for row, w in WIDTHS:
        total = v.reshape(-1, w).sum(axis=1)
        assert len(set(total.tolist())) == 256 // w
        assert np.array_equal(out[row], np.repeat(total, w)), w
    assert np.array_equal(out[3], np.repeat(v.reshape(4, 64).max(axis=1), 64))


def test_lane_sums_follow_the_documented_order():
    rng = np.random.RandomState(71)
    v = np.concatenate([rng.standard_normal(256) * 10.0 ** rng.uniform(-8, 8, 256), rng.standard_normal(256)])
    out = call("mp_lane_sums", v)
    for row, w in WIDTHS:
        want = R.lane_sum_order(v.reshape(-1, 64), w).ravel()
        assert np.array_equal(bits(out[row]), bits(want)), (w, np.flatnonzero(bits(out[row]) != bits(want))[:8])
    exact = np.array([float(np.sum(np.array(c, dtype=np.longdouble))) for c in v.reshape(-1, 64)])
    assert np.all(np.abs(out[2].reshape(-1, 64) - exact[:, None]) <= 64 * EPS * np.abs(v).reshape(-1, 64).sum(1)[:, None])


def test_wave_max_drops_nan_unless_every_lane_is_nan():
    rng = np.random.RandomState(72)
    base = rng.standard_normal(64)
    rows, want = [], []
    # one NaN lane, at the four DPP rotation distances from the largest lane and in the other half-rows
    top = int(np.argmax(base))
    for shift in (8, 4, 2, 1, 16, 32, 0):
        for src in ((top & ~15) | ((top + shift) & 15), (top & ~15) | ((top - shift) & 15), top ^ (shift & 48)):
            r = base.copy()
            r[src] = np.nan
            rows.append(r)
            want.append(np.nanmax(r))
    for keep in (0, 17, 63):                      # all but one lane NaN
        r = np.full(64, np.nan)
        r[keep] = base[keep]
        rows.append(r)
        want.append(base[keep])
    rows.append(np.full(64, np.nan))
    want.append(np.nan)
    for fill, lane_value, expect in ((-np.inf, 3.0, 3.0), (-np.inf, -np.inf, -np.inf), (1.0, np.inf, np.inf),
                                     (-1.0, -0.0, -0.0), (-0.0, 0.0, 0.0), (np.nan, -np.inf, -np.inf)):
        r = np.full(64, fill)
        r[37] = lane_value
        rows.append(r)
        want.append(expect)
    while len(rows) % 4:
        rows.append(base.copy())
        want.append(base.max())
    got = call("mp_lane_sums", np.concatenate(rows))[3].reshape(-1, 64)
    for k, (g, w) in enumerate(zip(got, want)):
        if np.isnan(w):
            assert np.all(np.isnan(g)), k
        else:
            assert np.all(g == w), (k, w, g[:4])
            if w == 0.0 and np.signbit(w):         # max(-1, -0) is -0; fmax leaves max(-0, +0) open
                assert np.all(np.signbit(g)), (k, w)


# -- dual numbers ----------------------------------------------------------------------------------------------

def _dual_operands(op):
    """(a.v, a.d, b.v, b.d) inside the domain of `op`, with both signs where it allows them."""
    rng = np.random.RandomState(81 + DUAL_OPS[op])
    n = 400
    av, bv = rng.uniform(-3.0, 3.0, n), rng.uniform(-3.0, 3.0, n)
    ad, bd = rng.standard_normal(n) * 2.0, rng.standard_normal(n) * 2.0
    if op.startswith("div"):
        bv = np.where(np.abs(bv) < 0.05, -0.5, bv)
        bv[:40] = -np.abs(bv[:40])                      # negative divisors
    if op in ("t_log", "t_sqrt") or op.startswith("t_pow"):
        av = np.exp(rng.uniform(np.log(1e-3), np.log(30.0), n))
    if op in ("t_exp", "t_exp_libm"):
        av = rng.uniform(-40.0, 10.0, n)
    if op == "t_floor_at":
        bv = rng.uniform(-1.0, 1.0, n)
        av = bv + rng.choice([-1.0, -2.0 ** -40, 0.0, 2.0 ** -40, 1.0], n)
        av[:3], bv[:3] = [1e-12, 5e-13, 2e-12], 1e-12   # the floor ta_eam.hip uses
    return av, ad, bv, bd


@pytest.mark.parametrize("op", sorted(DUAL_OPS, key=DUAL_OPS.get))
def test_dual_rule_against_reference(op):
    av, ad, bv, bd = _dual_operands(op)
    code = np.full(len(av), float(DUAL_OPS[op]))
    v, d = call("mp_dual_ops", code, av, ad, bv, bd)
    plain, zero = call("mp_dual_ops", code + PLAIN, av, ad, bv, bd)
    assert np.array_equal(bits(v), bits(plain)) and np.all(zero == 0.0), op
    rd, terms = R.dual_ref(op, av, ad, bv, bd)
    share = _share(R.err_abs(d, rd), 8.0 * EPS * terms)
    e, at = worst(share, av)
    report(f"dual {op}, derivative, share of 8 x 2^-53 x sum|terms|", e, 1.0)
    assert np.all(np.isfinite(d)) and e <= 1.0, (op, e, at)
    if op == "t_floor_at":
        assert np.all(v == np.maximum(av, bv)) and np.all(d[av <= bv] == 0.0) and np.all(d[av > bv] == ad[av > bv])
        assert (av < bv).any() and (av == bv).any() and (av > bv).any()


@pytest.mark.parametrize("op", ["t_pow_dd", "t_pow_ds", "t_pow_sd"])
def test_dual_pow_at_zero_base_skips_the_unseeded_terms(op):
    yv = np.array([0.0, 0.5, 1.0, 2.0, 3.0])
    zeros = np.zeros_like(yv)
    code = np.full(len(yv), float(DUAL_OPS[op]))
    v, d = call("mp_dual_ops", code, zeros, zeros, yv, zeros)       # x = (0, 0), y = (yv, 0)
    assert v.tolist() == [1.0, 0.0, 0.0, 0.0, 0.0] and np.all(bits(d) == 0), (op, v, d)
    # y' = 0 alone at x.v = 0.7, and x' = 0 alone: the other term is untouched
    v, d = call("mp_dual_ops", code, zeros + 0.7, zeros + 1.5, yv, zeros)
    rd, terms = R.dual_ref(op, zeros + 0.7, zeros + 1.5, yv, zeros)
    assert np.all(R.err_abs(d, rd) <= 8.0 * EPS * terms) and (op == "t_pow_sd" or np.all(d[1:] != 0.0))


# -- index maps ------------------------------------------------------------------------------------------------

def test_term_index_maps():
    rows = [(a, b, nel) for nel in range(1, 6) for a in range(nel) for b in range(nel)]
    a, b, nel = (np.array(c, dtype=float) for c in zip(*rows))
    radial, angular = call("mp_term_index", a, b, nel)
    for (ia, ib, n), r, g in zip(rows, radial, angular):
        assert r == R.radial_term_numpy(ia, ib), (ia, ib)
        assert g == R.angular_term_numpy(ia, ib, n), (ia, ib, n)
    for n in range(1, 6):
        pick = nel == n
        assert sorted(set(angular[pick].tolist())) == list(range(n * (n + 1) // 2))
        for c in range(n):
            assert sorted(radial[pick & (a == c)].tolist()) == list(range(n))
    # the reference's own term lists (symmetric, angular), wherever the fixture has the element set
    with open(os.path.join(GOLDEN, "kbody_terms.json")) as f:
        cases = [c for c in json.load(f)["cases"] if c["angular"] and c["symmetric"]]
    assert {len(c["sorted_elements"]) for c in cases} >= {1, 2, 3, 4}
    rows, want = [], []           # (a, b, nel) of every case and centre, in one call
    for case in cases:
        els = case["sorted_elements"]
        n = len(els)
        for ci, center in enumerate(els):
            terms = case["terms_for_element"][center]
            for j in range(n):
                for k in range(n):
                    lo, hi = min(j, k), max(j, k)
                    rows.append((j, k, n))
                    want.append((terms.index(center + els[lo] + els[hi]) - n, (els, center, j, k)))
            for o in range(n):
                rows.append((ci, o, n))
                want.append((terms.index(center + els[o]), (els, center, o)))
    a, b, nel = (np.array(c, dtype=float) for c in zip(*rows))
    radial, angular = call("mp_term_index", a, b, nel)
    for (ia, ib, n), (index, what), r, g in zip(rows, want, radial, angular):
        assert (g if len(what) == 4 else r) == index, what
