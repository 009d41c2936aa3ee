"""
NumPy restatement of the loss gradient of the temperature-dependent head (test infrastructure only),
analytic, as csrc/ta_td_train.hip computes it.

For atom i with electron temperature T, c = T (Sommerfeld) or 1, and per-atom coefficients a, b, g of
U, F and S, the quantity differentiated with respect to the weights is

    phi_i = a U_i + b F_i + g S_i + (dF_i/dG_i) . dG_i,    dF/dG . dG = (dU/dz - T c ds/dz) . z',

z' = [J_H(x) x', 0], x' = minmax'(G) dG. Every net runs forward with its tangent (x, x') and backward
with two adjoints (kappa of x, nu of x'):
    lambda = kappa a'(z) + nu a''(z) z',  mu = nu a'(z),  dW = x^T lambda + x'^T mu,  db = sum lambda,
    kappa_in = lambda W^T (+ kappa),  nu_in = mu W^T (+ nu)   (ResNet skip).
U is seeded with (a + b, 1), S with (c (g - T b), -T c); their input adjoints, summed over the first K
columns, seed H. With nu = 0 the sweeps reduce to `td_reference.net_forward` / `net_backward`
(tests/test_td_train_cpu.py checks that).
"""
import numpy as np

from oracle.sf import activation
from tests.td_reference import minmax, td_head


def activation2(name, x):
    """Second derivative of the reference activations (as ta_math.h::activation_fn2)."""
    name = name.lower()
    a, da = activation(name, x)
    if name == "softplus":
        return da * (1.0 - da)
    if name == "sigmoid":
        return da * (1.0 - 2.0 * a)
    if name == "tanh":
        return -2.0 * a * da
    if name == "softsign":
        d = 1.0 + np.abs(x)
        return np.where(x >= 0.0, -2.0, 2.0) / (d * d * d)
    if name == "elu":
        return np.where(x > 0, 0.0, np.exp(np.minimum(x, 0.0)))
    if name == "squareplus":
        s = np.sqrt(x * x + 4.0)
        return 2.0 / (s * s * s)
    return np.zeros_like(x)   # relu, leaky relu


def net_forward2(layers, act, x, xt, resnet):
    """Forward with tangent. Returns (out, out', cache); cache per layer = (x, x', a', a'' z', skip)."""
    h, ht, cache = x, xt, []
    L = len(layers)
    for l, (W, b) in enumerate(layers):
        z = h @ W + (b if b is not None else 0.0)
        zt = ht @ W
        if l < L - 1:
            a, da = activation(act, z)
            dd = activation2(act, z) * zt
            res = bool(resnet and l > 0 and W.shape[0] == W.shape[1])   # convolutional.py:272-273
            cache.append((h, ht, da, dd, res))
            h, ht = (a + h, da * zt + ht) if res else (a, da * zt)
        else:
            cache.append((h, ht, np.ones_like(z), np.zeros_like(z), False))
            h, ht = z, zt
    return h, ht, cache


def net_reverse2(layers, cache, kappa, nu):
    """Adjoints (kappa, nu) of the output [n, out] -> ([(dW, db) per layer], kappa_in, nu_in). db is formed
    for every layer (layers without a bias give the gradient of a bias that would be there)."""
    grads = [None] * len(layers)
    for l in range(len(layers) - 1, -1, -1):
        W, _ = layers[l]
        x, xt, da, dd, res = cache[l]
        lam = kappa * da + nu * dd
        mu = nu * da
        grads[l] = (x.T @ lam + xt.T @ mu, lam.sum(axis=0))
        k_in, n_in = lam @ W.T, mu @ W.T
        kappa, nu = (k_in + kappa, n_in + nu) if res else (k_in, n_in)
    return grads, kappa, nu


def td_grad_element(nn, el, G, dG, T, a, b, g):
    """G, dG [n, D], T, a, b, g [n] of atoms of element `el` -> {"H" | "U" | "S": [(dW, db), ...]}."""
    ft = nn.finite_temperature_options
    w = nn.weights[el]
    resnet = nn._use_resnet_dt
    x, scale = minmax(nn, el, G)
    xt = dG * scale
    H, Ht, cH = net_forward2(w["H"], ft.activation, x, xt, resnet)
    K = H.shape[1]
    n = len(G)
    z = np.concatenate([H, T[:, None]], axis=1)
    zt = np.concatenate([Ht, np.zeros((n, 1))], axis=1)
    _, _, cU = net_forward2(w["U"], nn._activation, z, zt, resnet)
    _, _, cS = net_forward2(w["S"], nn._activation, z, zt, resnet)
    c = T if ft.algo == "Sommerfeld" else np.ones(n)
    gU, kU, nU = net_reverse2(w["U"], cU, (a + b)[:, None], np.ones((n, 1)))
    gS, kS, nS = net_reverse2(w["S"], cS, (c * (g - T * b))[:, None], (-T * c)[:, None])
    gH, _, _ = net_reverse2(w["H"], cH, (kU + kS)[:, :K], (nU + nS)[:, :K])
    return {"H": gH, "U": gU, "S": gS}


def td_loss_gradient_reference(nn, symbols, G, dG, T_atoms, a_atoms, b_atoms, g_atoms):
    """Flat gradient in the C ABI's layout (H of every element, then U, then S; per layer W then b) of
    sum_i phi_i over all atoms (per-atom T and coefficients)."""
    symbols = list(symbols)
    per = {}
    for el in nn.elements:
        idx = np.array([k for k, s in enumerate(symbols) if s == el], dtype=np.int64)
        if len(idx):
            per[el] = td_grad_element(nn, el, G[idx], dG[idx], *(np.asarray(v, dtype=np.float64)[idx]
                                                                 for v in (T_atoms, a_atoms, b_atoms, g_atoms)))
    out = []
    for net in ("H", "U", "S"):
        for el in nn.elements:
            for l, (W, _) in enumerate(nn.weights[el][net]):
                W = np.asarray(W)
                if el in per:
                    dW, db = per[el][net][l]
                else:
                    dW, db = np.zeros(W.shape), np.zeros(W.shape[1])
                out += [np.ravel(dW), np.ravel(db)]
    return np.concatenate(out)


def td_objective(nn, symbols, G, dG, T_atoms, a_atoms, b_atoms, g_atoms):
    """sum_i phi_i evaluated directly (values and dF/dG of `td_reference.td_head`)."""
    r = td_head(nn, symbols, G, np.asarray(T_atoms, dtype=np.float64))
    return float(np.sum(a_atoms * r["U"] + b_atoms * r["F"] + g_atoms * r["S"]) + np.sum(r["dFdG"] * dG))

