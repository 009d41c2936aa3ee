"""CPU: what tests/test_gpu_math.py stands on. The probe compiles for gfx950 with the library's flags and exports
every launcher; the 50-digit reference agrees with extended-precision closed forms in NumPy; every input grid holds
the points it promises; and an IEEE restatement of ta_exp and of the cosine cutoff stays inside the GPU test's
bounds, so correct code can reach them."""
import ctypes
import os

import numpy as np

from tensoralloy_amd import _lib
from tests import math_probe
from tests import math_reference as R

LD = np.longdouble


# -- the probe -------------------------------------------------------------------------------------------------

def test_probe_compiles_with_the_library_flags_and_exports_every_launcher():
    cmd = math_probe.compile_command("out.so")
    assert cmd == [_lib.hipcc_path()] + _lib._compile_flags() + ["-shared", math_probe.SOURCE, "-o", "out.so"]
    assert "--offload-arch=gfx950" in cmd
    obj = math_probe.build()
    assert os.path.getmtime(obj) >= max(os.path.getmtime(p) for p in math_probe.dependencies())
    before = os.path.getmtime(obj)
    assert math_probe.build() == obj and os.path.getmtime(obj) == before     # up to date: not compiled again
    lib = ctypes.CDLL(obj)
    for name in math_probe.LAUNCHERS:
        assert hasattr(lib, name), name
    with open(math_probe.SOURCE) as f:
        text = f.read()
    for header in ("tensoralloy_amd.h", "ta_device.h", "ta_math.h", "ta_dual.h", "ta_reduce.h"):
        assert f'#include "{header}"' in text
    assert "printf" not in text and "assert(" not in text
    assert sorted(math_probe.DUAL_OPS.values()) == list(range(len(math_probe.DUAL_OPS)))


# -- the reference against closed forms in long double ---------------------------------------------------------

def _pinned(got_ld, ref):
    """|double(long-double closed form) - ref| in ulp."""
    return R.err_ulp(np.asarray(got_ld, dtype=LD).astype(np.float64), ref).max()


def test_reference_matches_closed_forms_at_ordinary_points():
    rng = np.random.RandomState(1)
    x = rng.uniform(-20.0, 20.0, 300)
    xl = x.astype(LD)
    pi = LD(np.pi) + LD(1.2246467991473532e-16)
    assert _pinned(np.exp(xl), R.exp_ref(x)) <= 1.0
    d = rng.uniform(1.0, 3.0, 300)
    assert _pinned(1 / d.astype(LD), R.rcp_ref(d)) <= 1.0
    h, dh = R.softplus_ref(x)
    assert _pinned(np.log1p(np.exp(xl)), h) <= 1.0
    assert _pinned(1 / (1 + np.exp(-xl)), dh) <= 1.0
    u = rng.uniform(0.01, 0.9, 300)
    s = np.sqrt(u.astype(LD))
    f, df, d2f = R.cutoff_ref("cosine", u)
    assert _pinned((1 + np.cos(pi * s)) / 2, f) <= 1.0
    assert _pinned(-pi * np.sin(pi * s) / (4 * s), df) <= 1.0
    assert np.all(R.err_abs(np.float64(-pi * (pi * s * np.cos(pi * s) - np.sin(pi * s)) / (8 * s ** 3)), d2f)
                  <= 2.0 ** -52 * 4.0)                    # the closed form cancels: 1 ulp of its terms (<= 4)
    f, df, d2f = R.cutoff_ref("polynomial", u)
    assert _pinned(1 + 5 * s ** 6 - 6 * s ** 5, f) <= 1.0
    assert _pinned(15 * s ** 3 * (s - 1), df) <= 1.0
    assert np.all(R.err_abs(np.float64(30 * u.astype(LD) - LD(22.5) * s), d2f) <= 2.0 ** -52 * 32.0)
    t = np.tanh(xl)
    sg = 1 / (1 + np.exp(-xl))
    sq = np.sqrt(xl * xl + 4)
    closed = {
        "tanh": (t, 1 - t * t, -2 * t * (1 - t * t)),
        "sigmoid": (sg, sg * (1 - sg), sg * (1 - sg) * (1 - 2 * sg)),
        "softplus": (np.log1p(np.exp(xl)), sg, sg * (1 - sg)),
        "softsign": (xl / (1 + abs(xl)), 1 / (1 + abs(xl)) ** 2, -2 * np.sign(xl) / (1 + abs(xl)) ** 3),
        "squareplus": ((xl + sq) / 2, (1 + xl / sq) / 2, 2 / sq ** 3),
        "elu": (np.where(xl > 0, xl, np.expm1(xl)), np.where(xl > 0, 1, np.exp(xl)), np.where(xl > 0, 0, np.exp(xl))),
        "relu": (np.maximum(xl, 0), (xl > 0).astype(LD), 0 * xl),
        "leaky_relu": (np.where(xl > 0, xl, xl / 5), np.where(xl > 0, LD(1), LD(1) / 5), 0 * xl),
        "linear": (xl, 1 + 0 * xl, 0 * xl),
    }
    assert sorted(closed) == sorted(R.ACTIVATIONS)
    small = np.abs(x) <= 3.0          # where no closed form above cancels (1 - t^2, 1 - s, x + sqrt(x^2 + 4))
    for name, forms in closed.items():
        for k, (form, ref) in enumerate(zip(forms, R.activation_ref(name, x[small]))):
            assert _pinned(np.asarray(form)[small], ref) <= 1.0, (name, k)


def test_reference_matches_the_oracle_activations():
    """oracle/sf.py::activation and oracle/train.py::activation2 in double against the reference, where they do
    not cancel."""
    from oracle.sf import activation
    from oracle.train import activation2
    x = np.concatenate([np.random.RandomState(2).uniform(-3.0, 3.0, 200), [0.0, -0.0]])
    for name in _lib.TA_ACT:
        h, dh = activation(name, x)
        d2h = activation2(name, x)
        for k, (got, ref) in enumerate(zip((h, dh, d2h), R.activation_ref(name, x))):
            assert np.all(R.err_abs(got, ref) <= 2.0 ** -50), (name, k)


def test_cosine_series_joins_the_closed_form():
    u = np.array([2.0 ** -20, np.nextafter(2.0 ** -20, 0.0)])
    for ref in R.cutoff_ref("cosine", u):
        assert abs((ref.hi[0] - ref.hi[1]) + (ref.lo[0] - ref.lo[1])) <= 1e-20
    f, df, d2f = R.cutoff_ref("cosine", np.array([0.0]))
    assert f.hi[0] == 1.0 and abs(df.hi[0] + np.pi ** 2 / 4) < 1e-15 and abs(d2f.hi[0] - np.pi ** 4 / 24) < 1e-14


def test_pow_rules_and_ulp_helpers():
    assert R.ulp_of(np.array([1.0, 1.5, 2.0, 0.0, 2.0 ** -1030, -3.0])).tolist() == \
        [2.0 ** -52, 2.0 ** -52, 2.0 ** -51, R.TINY, R.TINY, 2.0 ** -51]
    third = R.Ref([R.mpf(1) / 3, R.mpf(1) - R.mpf(2) ** -80])
    assert third.hi.tolist() == [1 / 3, 1.0] and third.lo[0] != 0.0
    assert R.ulp_of(third).tolist() == [2.0 ** -54, 2.0 ** -53]          # 1 - 2^-80 sits below the power of two
    assert R.err_ulp(np.array([np.nextafter(1 / 3, 1.0), 1.0]), third)[0] > 0.5
    x, y = R.safe_pow_grid()
    for safe in (0, 1):
        v, g = R.safe_pow_ref(safe, x, y)
        with np.errstate(all="ignore"):
            pv, pg = np.power(x, y), np.power(x, y - 1.0)
        if safe:
            pv, pg = np.where(np.isinf(pv), 0.0, pv), np.where(np.isfinite(pg), pg, 0.0)
        for got, ref in ((pv, v), (pg, g)):
            assert np.array_equal(np.isnan(got), np.isnan(ref.hi)) and np.array_equal(np.isinf(got), np.isinf(ref.hi))
            ok = np.isfinite(ref.hi)
            assert np.all(R.err_ulp(got, ref)[ok] <= 1.0)


def test_dual_reference_is_the_derivative_of_its_operation():
    """Each rule of dual_ref against a central difference of the operation along (a', b') in 50 digits."""
    plain = {"neg": lambda a, b: -a, "add": lambda a, b: a + b, "iadd": lambda a, b: a + b,
             "sub": lambda a, b: a - b, "mul": lambda a, b: a * b, "div": lambda a, b: a / b,
             "t_val": lambda a, b: R.mpf(0), "t_exp": lambda a, b: R.MP.exp(a), "t_exp_libm": lambda a, b: R.MP.exp(a),
             "t_log": lambda a, b: R.MP.log(a), "t_sqrt": lambda a, b: R.MP.sqrt(a),
             "t_pow": lambda a, b: R.MP.power(a, b), "t_floor_at": lambda a, b: max(a, b)}
    a, da, b, db = 1.7, 0.6, 0.9, -1.3
    h = R.mpf(10) ** -20
    for op in math_probe.DUAL_OPS:
        kind = "t_pow" if op.startswith("t_pow") else op if op.startswith("t_") else op.split("_")[0]
        ea = 0 if op.endswith("_sd") else da
        eb = 0 if op.endswith("_ds") or op == "t_floor_at" else db
        f = plain[kind]
        fd = (f(R.mpf(a) + h * ea, R.mpf(b) + h * eb) - f(R.mpf(a) - h * ea, R.mpf(b) - h * eb)) / (2 * h)
        d, terms = R.dual_ref(op, [a], [da], [b], [db])
        assert abs(d.hi[0] - float(fd)) <= 1e-14 * max(1.0, terms[0]), op
        assert terms[0] >= abs(d.hi[0]) * (1 - 1e-15)


def test_index_and_lane_order_restatements():
    assert [R.radial_term_numpy(1, o) for o in range(3)] == [1, 0, 2]          # B: BB, BA, BC
    assert [R.angular_term_numpy(j, k, 3) for j, k in ((0, 0), (0, 2), (2, 1), (2, 2))] == [0, 2, 4, 5]
    v = np.arange(64.0)
    assert np.all(R.lane_sum_order(v, 16) == np.repeat(v.reshape(4, 16).sum(1), 16))
    assert np.all(R.lane_sum_order(v, 32) == np.repeat(v.reshape(2, 32).sum(1), 32))
    assert np.all(R.lane_sum_order(v, 64) == v.sum())


# -- the grids -------------------------------------------------------------------------------------------------

def _has(grid, points):
    return all(np.any(bits(grid) == bits(np.array([p]))[0]) for p in points)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_exp_grid_holds_its_boundaries():
    x = R.exp_grid()
    assert len(x) <= 2 ** 17 and x.min() >= -745.2 and x.max() <= 50.0
    assert _has(x, [0.0, -0.0, 2.0 ** -60, -2.0 ** -60, -745.13])
    b = R.exp_boundaries()
    assert len(b) == 2295 and abs(b[0] + 2150 * np.log(2) / 2) < 1e-12 and abs(b[-1] - 72 * np.log(2)) < 1e-13
    for k in (-2, -1, 0, 1, 2):
        assert _has(x, R._steps(b[0], [k]) + R._steps(b[1000], [k]) + R._steps(b[-1], [k]))
    moved = np.array([R._steps(v, [-2, -1, 0, 1, 2]) for v in b]).ravel()
    assert np.all(np.isin(bits(moved), bits(x)))
    # odd k: rint(x log2 e) really switches within +-2 ulp of the boundary
    odd = b[1::2]
    kf = np.array([np.rint(np.array(R._steps(v, [-2, 2])) * 1.4426950408889634074) for v in odd])
    assert np.all(kf[:, 1] - kf[:, 0] == 1.0)
    assert _has(x, R._steps(float(-1022 * R.LN2), range(-4, 5)))
    sub = R.exp_ref(x).hi < 2.0 ** -1022
    assert 0.0 < sub.mean() <= 0.05, sub.mean()
    z = R.exp_zero_grid()
    assert z.min() == -1e6 and z.max() == -746.0 and len(z) <= 2 ** 17


def test_cutoff_rcp_softplus_activation_grids_hold_their_edges():
    u = R.cutoff_grid()
    k = np.arange(1, 54)
    assert len(u) <= 2 ** 17 and u.min() == 0.0 and u.max() == 1.0 - 2.0 ** -53
    assert _has(u, list(2.0 ** -k) + list(1.0 - 2.0 ** -k))
    d = R.rcp_grid()
    assert len(d) <= 2 ** 17 and d.min() == 1.0 and d.max() == 3.0
    assert _has(d, [1.0 + 2.0 ** -52, 2.0, np.nextafter(2.0, 3.0), np.nextafter(2.0, 1.0), np.nextafter(3.0, 1.0)])
    x = R.softplus_grid()
    assert len(x) <= 2 ** 17 and x.min() == -800.0 and x.max() == 800.0
    assert abs(np.exp(R.SOFTPLUS_SWITCH) - 0.41421356237309503) < 1e-16
    for s in (1.0, -1.0):
        assert _has(x, R._steps(s * R.SOFTPLUS_SWITCH, range(-2, 3)) + R._steps(s * 708.0, (-1, 0, 1)) + [s * 750.0])
    assert _has(x, [0.0, -0.0])
    e = np.exp(-np.abs(np.array(R._steps(R.SOFTPLUS_SWITCH, (-2, 2)))))
    assert (e[0] > 0.41421356237309503) != (e[1] > 0.41421356237309503) or e[0] != e[1]
    a = R.activation_grid()
    assert len(a) <= 2 ** 17 and _has(a, [0.0, -0.0, 2.0 ** -30, -2.0 ** -30, 700.0, -700.0])
    assert np.all((np.abs(a) <= 50.0) | (np.abs(a) == 700.0))
    base, zi = R.pow_int_grid()
    assert set(zi.tolist()) == set(range(1, 65)) and _has(base, [0.0, 1.0, -1.5, 0.1, 2.0])
    inner = base[(base != 0.0) & (base != 1.0) & (base != -1.5)]
    assert inner.min() >= 0.1 and inner.max() <= 2.0
    sx, sy = R.safe_pow_grid()
    assert len(sx) == 35 and set(sx.tolist()) == set(R.SAFE_POW_X) and set(sy.tolist()) == set(R.SAFE_POW_Y)


# -- the bounds are reachable: an IEEE restatement in NumPy ---------------------------------------------------

def fma(a, b, c):
    """a b + c with the product and the sum in long double (NumPy has no fma)."""
    return (np.asarray(a, dtype=LD) * np.asarray(b, dtype=LD) + np.asarray(c, dtype=LD)).astype(np.float64)


def exp_restated(x):
    """ta_exp of csrc/ta_math.h, step by step."""
    kf = np.rint(x * 1.4426950408889634074)
    r = fma(-kf, 6.93147180369123816490e-01, x)
    r = fma(-kf, 1.90821492927058770002e-10, r)
    p = np.full_like(x, 1.0 / 6227020800.0)
    for c in (479001600.0, 39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0, 2.0, 1.0, 1.0):
        p = fma(p, r, 1.0 / c)
    return np.ldexp(p, np.maximum(kf, -1100.0).astype(np.int64))


def cosine_restated(u):
    """cutoff_u2 of csrc/ta_math.h (cosine): Horner on c_k, k c_k and k (k - 1) c_k; f = Y^2."""
    q = -2.4674011002723396547
    coef = [1.0]
    for j in range(1, 12):
        coef.append(coef[-1] * (q / float((2 * j - 1) * (2 * j))))
    y = np.full_like(u, coef[11])
    d = np.full_like(u, 11.0 * coef[11])
    dd = np.full_like(u, 110.0 * coef[11])
    for k in range(10, -1, -1):
        y = fma(y, u, coef[k])
    for k in range(10, 0, -1):
        d = fma(d, u, float(k) * coef[k])
    for k in range(10, 1, -1):
        dd = fma(dd, u, float(k * (k - 1)) * coef[k])
    return y * y, 2.0 * y * d, 2.0 * (d * d + y * dd)


def test_ieee_restatement_of_exp_stays_inside_the_bounds():
    x = R.exp_grid()
    got, ref = exp_restated(x), R.exp_ref(x)
    normal = ref.hi >= 2.0 ** -1022
    assert R.err_ulp(got, ref)[normal].max() <= 1.5
    assert R.err_abs(got, ref)[~normal].max() <= 2.0 * R.TINY
    assert np.all(exp_restated(R.exp_zero_grid()) == 0.0)


def test_ieee_restatement_of_the_cosine_cutoff_stays_inside_the_bounds():
    u = R.cutoff_grid()
    for got, ref, bound in zip(cosine_restated(u), R.cutoff_ref("cosine", u), (4e-16, 2e-15, 5e-15)):
        assert R.err_abs(got, ref).max() <= bound
    assert cosine_restated(np.array([1.0 - 2.0 ** -53]))[0][0] >= 0.0
