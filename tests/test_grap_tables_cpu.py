"""The GRAP filter table without a GPU: the C ABI names it adds, the knot count the library and the Python
package agree on, and that knot count itself: a numpy cubic Hermite table of `oracle.grap.nn_filters`, built
in the network's own input x as csrc/ta_grap.hip builds it (value and x-derivative exact at every knot,
    c0 = f_k, c1 = f'_k, c2 = (3 s - 2 f'_k - f'_k+1) / h, c3 = (f'_k + f'_k+1 - 2 s) / h^2, s = (f_k+1 - f_k) / h,
forces from the cubic's own derivative times dx/dr), against the exact network."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests.helpers import make_grap_nn

ROOT = Path(__file__).resolve().parents[1]

# Relative to the largest |v| and |dv/dr| over the sample. Measured at 4097 knots (modifiers 0, 1, 2): value
# 7.6e-16, 1.3e-15, 7.8e-16; derivative 5.2e-12, 8.2e-12, 1.01e-11. The value keeps the bound 1e-12 (700x
# room). The derivative is rounding of (f_k+1 - f_k) / h, not truncation; modifier 2 sits 9.9x inside 1e-10,
# nearer than 10x, so its bound is 10x the measured 1.01e-11.
V_REL, DV_REL = 1e-12, 1.01e-10


def test_abi_names_the_filter_table_entries():
    from tensoralloy_amd import _lib
    header = (ROOT / "include" / "tensoralloy_amd.h").read_text()
    for name in ("ta_set_filter_tables", "ta_filter_table_knots"):
        assert name in _lib.EXPORTED_SYMBOLS
        assert re.search(r"\bint\s+%s\s*\(" % name, header)


def test_default_knot_count_is_one_number():
    from tensoralloy_amd import grap
    assert 4097 <= grap.FILTER_TABLE_KNOTS <= 8193
    src = (ROOT / "tensoralloy_amd" / "csrc" / "ta_grap.hip").read_text()
    m = re.search(r"constexpr\s+int\s+kFilterTableKnots\s*=\s*(\d+)\s*;", src)
    assert m and int(m.group(1)) == grap.FILTER_TABLE_KNOTS
    header = (ROOT / "include" / "tensoralloy_amd.h").read_text()
    assert "library default, %d" % grap.FILTER_TABLE_KNOTS in header


def _x_of_r(mod, r, rcov):
    if mod == 0:
        return r, np.ones_like(r)
    if mod == 1:
        return r / rcov, 1.0 / rcov
    x = np.exp(-r / rcov)
    return x, -x / rcov


def hermite_table(net, n_knots, xmax):
    """[n_knots, K, 4] pieces of the network as a function of its input x (modifier taken out: the network
    sees x itself)."""
    from oracle.grap import nn_filters
    plain = dict(net, h_abck_modifier=0)
    h = xmax / (n_knots - 1)
    xk = np.arange(n_knots) * h
    f, d = nn_filters(xk, plain)
    tab = np.zeros((n_knots, f.shape[1], 4))
    tab[:, :, 0], tab[:, :, 1] = f, d
    s = (f[1:] - f[:-1]) / h
    tab[:-1, :, 2] = (3.0 * s - 2.0 * d[:-1] - d[1:]) / h
    tab[:-1, :, 3] = (d[:-1] + d[1:] - 2.0 * s) / (h * h)
    return tab, h


def table_eval(tab, h, x):
    k = np.clip((x / h).astype(np.int64), 0, len(tab) - 2)
    t = (x - k * h)[:, None]
    c = tab[k]
    v = c[..., 0] + t * (c[..., 1] + t * (c[..., 2] + t * c[..., 3]))
    dv = c[..., 1] + t * (2.0 * c[..., 2] + 3.0 * t * c[..., 3])
    return v, dv


@pytest.mark.parametrize("modifier", [0, 1, 2])
def test_hermite_table_matches_the_network_at_the_default_knots(modifier):
    """10 000 random r in (0.5, rcut), a random centre element per pair: the default network (modifier 0) and
    the 32-32, K = 8 network over Mo-Ni (modifiers 1, 2)."""
    from oracle.grap import nn_filters
    from tensoralloy_amd.grap import FILTER_TABLE_KNOTS
    from tests.helpers import oracle_grap_model
    rcut = 6.0
    if modifier == 0:
        nn = make_grap_nn(["Ni"], rcut, [16], "nn", moment_tensors=[0, 1, 2, 3])
    else:
        par = {"hidden_sizes": [32, 32], "num_filters": 8, "h_abck_modifier": modifier}
        nn = make_grap_nn(["Mo", "Ni"], rcut, [16], "nn", par, moment_tensors=[0, 1, 2, 3])
    model = oracle_grap_model(nn)
    net = model.filter_net
    from oracle.grap import COVALENT_RADII
    rcovs = np.array([COVALENT_RADII[el] for el in nn.elements]) if modifier else np.array([1.0])
    xmax = {0: rcut, 1: rcut / rcovs.min(), 2: 1.0}[modifier]
    tab, h = hermite_table(net, FILTER_TABLE_KNOTS, xmax)
    rng = np.random.RandomState(7)
    r = rng.uniform(0.5, rcut, 10000)
    rcov = rcovs[rng.randint(len(rcovs), size=len(r))]
    v, dv = nn_filters(r, net, rcov)
    x, dxdr = _x_of_r(modifier, r, rcov)
    tv, tdv = table_eval(tab, h, x)
    tdv = tdv * dxdr[:, None]
    ev, edv = np.abs(tv - v).max() / np.abs(v).max(), np.abs(tdv - dv).max() / np.abs(dv).max()
    print(f"modifier {modifier}: value {ev:.2e}, derivative {edv:.2e} (relative)")
    assert ev < V_REL
    assert edv < DV_REL
