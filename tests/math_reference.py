"""High-precision reference (mpmath, 50 digits) of the device math in csrc/ta_math.h and ta_dual.h, from the
defining formulas and not from the device's algorithms, and the deterministic input grids of
tests/test_gpu_math.py (tests/test_math_reference_cpu.py checks that the grids hold what they promise).

A reference value travels as a `Ref`: the nearest double `hi` and the remainder `lo` = ref - hi, so that errors
are formed in NumPy: got - hi is exact for any got within a factor two of hi, and lo carries the rest."""
import math

import mpmath
import numpy as np

MP = mpmath.mp.clone()
MP.dps = 50
mpf = MP.mpf

TINY = 2.0 ** -1074
ACTIVATIONS = ("relu", "softplus", "tanh", "squareplus", "leaky_relu", "sigmoid", "softsign", "elu", "linear")
LIBM_ACTIVATIONS = ("tanh", "sigmoid", "elu")
RATIONAL_ACTIVATIONS = ("relu", "leaky_relu", "softsign", "squareplus", "linear")


class Ref:
    """hi + lo of an array of reference values (NaN and infinities live in hi, with lo = 0)."""

    def __init__(self, values):
        hi, lo = np.empty(len(values)), np.zeros(len(values))
        for k, v in enumerate(values):
            if isinstance(v, float):
                hi[k] = v
                continue
            try:
                hi[k] = float(v)
            except OverflowError:
                hi[k] = math.inf if v > 0 else -math.inf
            if math.isfinite(hi[k]):
                lo[k] = float(v - mpf(hi[k]))
        self.hi, self.lo = hi, lo

    def __len__(self):
        return len(self.hi)


def ulp_of(ref):
    """Spacing of the doubles at |ref| (2^-1074 in the subnormal range and at 0)."""
    hi, lo = (ref.hi, ref.lo) if isinstance(ref, Ref) else (np.asarray(ref, dtype=float), 0.0)
    m, e = np.frexp(np.abs(hi))
    e = e - ((m == 0.5) & (lo * np.sign(hi) < 0))      # just below a power of two
    return np.where(hi == 0.0, TINY, np.ldexp(1.0, np.maximum(e - 53, -1074)))


def err_abs(got, ref):
    with np.errstate(invalid="ignore"):
        return np.abs((np.asarray(got) - ref.hi) - ref.lo)


def err_ulp(got, ref):
    return err_abs(got, ref) / ulp_of(ref)


def _m(x):
    return [mpf(float(v)) for v in np.asarray(x, dtype=float).ravel()]


# -- the primitives ------------------------------------------------------------------------------------------

def exp_ref(x):
    return Ref([MP.exp(v) for v in _m(x)])


def rcp_ref(d):
    return Ref([1 / v for v in _m(d)])


_SERIES_BELOW = 2.0 ** -20


def _cosine_series(u):
    """f = 1 + sum_k a_k u^k, a_k = (-1)^k pi^(2k) / (2 (2k)!): value, first and second derivative in u."""
    f, df, d2f = mpf(1), mpf(0), mpf(0)
    for k in range(1, 13):
        a = (-1) ** k * MP.pi ** (2 * k) / (2 * MP.factorial(2 * k))
        f += a * u ** k
        df += k * a * u ** (k - 1)
        if k >= 2:
            d2f += k * (k - 1) * a * u ** (k - 2)
    return f, df, d2f


def cutoff_ref(kind, u):
    """(f, df/du, d2f/du2) of 0.5 (1 + cos(pi sqrt(u))) ("cosine") or 1 + 5 x^6 - 6 x^5, x = sqrt(u) ("polynomial")."""
    out = ([], [], [])
    for v in _m(u):
        s = MP.sqrt(v)
        if kind == "cosine":
            if v < _SERIES_BELOW:
                vals = _cosine_series(v)
            else:
                sn, cs = MP.sin(MP.pi * s), MP.cos(MP.pi * s)
                vals = ((1 + cs) / 2, -MP.pi * sn / (4 * s), -MP.pi * (MP.pi * s * cs - sn) / (8 * s ** 3))
        elif kind == "polynomial":
            vals = (1 + 5 * s ** 6 - 6 * s ** 5, 15 * s ** 3 * (s - 1), 30 * v - mpf(22.5) * s)
        else:
            raise ValueError(kind)
        for o, val in zip(out, vals):
            o.append(val)
    return tuple(Ref(o) for o in out)


def softplus_ref(x):
    """log1p(exp(x)) and the logistic function."""
    xs = _m(x)
    return Ref([MP.log1p(MP.exp(v)) for v in xs]), Ref([1 / (1 + MP.exp(-v)) for v in xs])


def _activation_point(name, x):
    """(h, h', h'') at one point; at a kink the one-sided conventions of oracle/sf.py::activation (x > 0 picks the
    right branch) and oracle/train.py::activation2 (sign(0) = 0)."""
    zero, one = mpf(0), mpf(1)
    if name == "linear":
        return x, one, zero
    if name == "relu":
        return (x, one, zero) if x > 0 else (zero, zero, zero)
    if name == "leaky_relu":
        a = mpf("0.2")
        return (x, one, zero) if x > 0 else (a * x, a, zero)
    if name == "softplus":
        s = 1 / (1 + MP.exp(-x))
        return MP.log1p(MP.exp(x)), s, s * (1 - s)
    if name == "tanh":
        t = MP.tanh(x)
        return t, 1 - t * t, -2 * t * (1 - t * t)
    if name == "sigmoid":
        s = 1 / (1 + MP.exp(-x))
        return s, s * (1 - s), s * (1 - s) * (1 - 2 * s)
    if name == "softsign":
        d = 1 + abs(x)
        return x / d, 1 / d ** 2, -2 * MP.sign(x) / d ** 3
    if name == "elu":
        return (x, one, zero) if x > 0 else (MP.expm1(x), MP.exp(x), MP.exp(x))
    if name == "squareplus":
        s = MP.sqrt(x * x + 4)
        return (x + s) / 2, (1 + x / s) / 2, 2 / s ** 3
    raise ValueError(name)


def activation_ref(name, x):
    rows = [_activation_point(name, v) for v in _m(x)]
    return tuple(Ref([r[k] for r in rows]) for k in range(3))


def activation_terms(name, x):
    """Largest |term| of the kernel's own formulas for h' and h'' of the libm-based activations, on the reference:
    tanh: h' = 1 - t^2 (terms 1, t^2), h'' = -2 t h' (terms 2 t, 2 t^3);
    sigmoid: h' = s - s^2, h'' = h' (1 - 2 s) (terms s, s^2, 2 s^2, 2 s^3);
    elu: h' = h'' = exp(x) on x <= 0 (one term), the constants 1 and 0 on x > 0."""
    x = np.asarray(x, dtype=float)
    h = activation_ref(name, x)[0].hi
    if name == "tanh":
        return np.ones_like(x), 2.0 * np.abs(h)
    if name == "sigmoid":
        return h, np.maximum(h, 2.0 * h * h)
    if name == "elu":
        e = activation_ref(name, x)[1].hi
        return e, np.where(x > 0, 0.0, e)
    raise ValueError(name)


def _is_integer(y):
    return float(y) == math.floor(float(y))


def pow_point(x, y):
    """x^y by the IEEE rules at the edges (mpf, or a float for Inf / NaN)."""
    if x == 0:
        return mpf(1) if y == 0 else (mpf(0) if y > 0 else math.inf)
    if x < 0:
        if not _is_integer(y):
            return math.nan
        return MP.power(-x, y) * (-1 if int(y) % 2 else 1)
    return MP.power(x, y)


def safe_pow_ref(safe, x, y):
    """(x^y, x^(y-1)) as ta_math.h quotes the reference: safe = 1 zeroes an infinite value and an infinite or NaN
    gradient factor; a NaN value stays NaN in both modes."""
    value, grad = [], []
    for xv, yv in zip(_m(x), _m(y)):
        v, g = pow_point(xv, yv), pow_point(xv, yv - 1)
        v_inf = isinstance(v, float) and math.isinf(v) or (not isinstance(v, float) and abs(v) > mpf(2) ** 1024)
        g_bad = isinstance(g, float) or abs(g) > mpf(2) ** 1024
        value.append(0.0 if safe and v_inf else v)
        grad.append(0.0 if safe and g_bad else g)
    return Ref(value), Ref(grad)


def pow_int_ref(base, zi):
    return Ref([b ** (int(z) - 1) for b, z in zip(_m(base), np.asarray(zi).ravel())])


def dual_ref(op, av, ad, bv, bd):
    """The derivative part of Dual operation `op` (a name of tests/math_probe.py::DUAL_OPS) as the exact rule at
    the given operands, with the sum of the |terms| of that rule."""
    d, terms = [], []
    for a, da, b, db in zip(_m(av), _m(ad), _m(bv), _m(bd)):
        kind = "t_pow" if op.startswith("t_pow") else op if op.startswith("t_") else op.split("_")[0]
        left_scalar, right_scalar = op.endswith("_sd"), op.endswith("_ds")
        if left_scalar:
            da = mpf(0)
        if right_scalar:
            db = mpf(0)
        if kind == "neg":
            t = [-da]
        elif kind in ("add", "iadd"):
            t = [da, db]
        elif kind == "sub":
            t = [da, -db]
        elif kind == "mul":
            t = [a * db, da * b]
        elif kind == "div":
            t = [da / b, -a * db / (b * b)]
        elif kind == "t_val":
            t = [mpf(0)]
        elif kind in ("t_exp", "t_exp_libm"):
            t = [MP.exp(a) * da]
        elif kind == "t_log":
            t = [da / a]
        elif kind == "t_sqrt":
            t = [da / (2 * MP.sqrt(a))]
        elif kind == "t_pow":
            # d(x^y) = x^y ln(x) y' + y x^(y-1) x'; a term with a zero seed is absent (x may be 0 there)
            t = [MP.power(a, b) * MP.log(a) * db if db != 0 else mpf(0),
                 b * MP.power(a, b - 1) * da if da != 0 else mpf(0)]
        elif kind == "t_floor_at":
            t = [da if a > b else mpf(0)]
        else:
            raise ValueError(op)
        d.append(sum(t, mpf(0)))
        terms.append(float(sum((abs(v) for v in t), mpf(0))))
    return Ref(d), np.array(terms)


# -- NumPy restatements ----------------------------------------------------------------------------------------

def radial_term_numpy(center, other):
    """[AA, AB (B != A, sorted)]: the centre's own element first, the others in element order."""
    order = [center] + [s for s in range(max(center, other) + 1) if s != center]
    return order.index(other)


def angular_term_numpy(s1, s2, nel):
    """sorted pair (j <= k) in row-major upper-triangular order."""
    pairs = [(a, b) for a in range(nel) for b in range(a, nel)]
    return pairs.index((min(s1, s2), max(s1, s2)))


def lane_sum_order(v, width):
    """The documented order of row16_sum / group_sum<32> / wave_sum on [..., 64] lanes: rotations by 8, 4, 2, 1
    inside each row of 16, then xor 16, then xor 32. After the rotation by 8 the partial sums repeat with period
    8 inside the row, then 4, then 2, and addition commutes, so the bits do not depend on the direction of the
    rotations (written here as lane l taking lane (l - n) mod 16): the comparison pins the distances and their
    order, not the direction."""
    v = np.array(v, dtype=np.float64)
    lanes = np.arange(64)
    for n in (8, 4, 2, 1):
        v = v + v[..., (lanes & ~15) | ((lanes - n) & 15)]
    if width >= 32:
        v = v + v[..., lanes ^ 16]
    if width >= 64:
        v = v + v[..., lanes ^ 32]
    return v


# -- input grids -----------------------------------------------------------------------------------------------

def _steps(x, ks):
    """x moved by k ulp for every k of ks."""
    out = []
    for k in ks:
        v = np.float64(x)
        for _ in range(abs(k)):
            v = np.nextafter(v, np.inf if k > 0 else -np.inf)
        out.append(float(v))
    return out


def _fill(seed, lo, hi, n, log_from=None, signed=True):
    """n uniform points of [lo, hi] and n log-uniform magnitudes of [log_from, max(|lo|, |hi|)] (both signs when
    `signed`), clipped into [lo, hi]."""
    rng = np.random.RandomState(seed)
    parts = [rng.uniform(lo, hi, n)]
    if log_from is not None:
        top = max(abs(lo), abs(hi))
        mag = np.exp(rng.uniform(np.log(log_from), np.log(top), n))
        sign = np.where(rng.rand(n) < 0.5, -1.0, 1.0) if signed else 1.0
        parts.append(np.clip(sign * mag, lo, hi))
    return np.concatenate(parts)


LN2 = MP.log(2)
EXP_BOUNDARY_K = range(-2150, 145)


def exp_boundaries():
    """k ln2 / 2 for k = -2150 ... 144: where rint(x log2 e) of the reduction switches (odd k) and sits exactly (even k)."""
    return np.array([float(k * LN2 / 2) for k in EXP_BOUNDARY_K])


def exp_grid():
    """x in [-745.2, 50]."""
    edges = [0.0, -0.0, 2.0 ** -60, -2.0 ** -60, -745.13, -745.2, 50.0]
    for b in exp_boundaries():
        edges += _steps(b, (-2, -1, 0, 1, 2))
    edges += _steps(float(-1022 * LN2), range(-4, 5))
    x = np.concatenate([_fill(11, -745.2, 50.0, 6000, log_from=2.0 ** -60), np.array(edges)])
    return x[(x >= -745.2) & (x <= 50.0)]


def exp_zero_grid():
    """x in [-1e6, -746]: the result is exactly 0."""
    rng = np.random.RandomState(12)
    return np.concatenate([[-746.0, -1e6, -1100.0 / 1.4426950408889634, -1101.0 * 0.6931471805599453],
                           rng.uniform(-1e6, -746.0, 2000), -np.exp(rng.uniform(np.log(746.0), np.log(1e6), 2000))])


def cutoff_grid():
    """u in [0, 1)."""
    k = np.arange(1, 54)
    edges = np.concatenate([[0.0], 2.0 ** -k, 1.0 - 2.0 ** -k])
    u = np.concatenate([_fill(21, 0.0, 1.0, 6000, log_from=1e-300, signed=False), edges])
    return u[(u >= 0.0) & (u < 1.0)]


def rcp_grid():
    """d in [1, 3]."""
    edges = [1.0, 3.0, 2.0, 1.0 + 2.0 ** -52] + _steps(2.0, (-1, 1)) + _steps(3.0, (-1,))
    return np.concatenate([_fill(31, 1.0, 3.0, 16000), np.array(edges)])


SOFTPLUS_SWITCH = float(MP.log(MP.sqrt(2) - 1))     # e = exp(-|x|) crosses sqrt(2) - 1 at |x| = 0.8813...


def softplus_grid():
    """x in [-800, 800]."""
    edges = [0.0, -0.0, 750.0, -750.0, 700.0, -700.0, 800.0, -800.0]
    for s in (1.0, -1.0):
        edges += _steps(s * SOFTPLUS_SWITCH, (-2, -1, 0, 1, 2))
        edges += _steps(s * 708.0, (-1, 0, 1))
    return np.concatenate([_fill(41, -800.0, 800.0, 6000, log_from=2.0 ** -60), np.array(edges)])


def activation_grid():
    """x in [-50, 50] and +-700."""
    edges = [0.0, -0.0, 2.0 ** -30, -2.0 ** -30, 700.0, -700.0, 50.0, -50.0]
    return np.concatenate([_fill(51, -50.0, 50.0, 2000, log_from=2.0 ** -40), np.array(edges)])


def pow_int_grid():
    """(base, zi): bases of [0.1, 2] and 0, 1, -1.5 with every exponent zi = 1 ... 64."""
    bases = np.concatenate([np.random.RandomState(61).uniform(0.1, 2.0, 60), [0.1, 2.0, 0.0, 1.0, -1.5]])
    b, z = np.meshgrid(bases, np.arange(1, 65), indexing="ij")
    return b.ravel(), z.ravel().astype(float)


SAFE_POW_X = (0.0, 1e-300, 0.5, 2.0, -2.0)
SAFE_POW_Y = (-1.5, -1.0, 0.0, 0.5, 1.0, 2.0, 3.0)


def safe_pow_grid():
    x, y = np.meshgrid(SAFE_POW_X, SAFE_POW_Y, indexing="ij")
    return x.ravel(), y.ravel()
