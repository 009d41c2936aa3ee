"""
NumPy restatement of the temperature-dependent head (test infrastructure only).

Reference: tensoralloy/nn/atomic/finite_temperature.py:211-304 (`_get_model_outputs`: H on the
min-max scaled descriptors, z = [H, T] by `_add_electron_temperature` :94-118, U :162-209, S :120-160
with the Sommerfeld factor :153-157, F = U - T S :300-302) and nn/convolutional.py:257-290 (dense
layers, ResNet skip of hidden layer j > 0 with equal widths, linear output layer).

`td_head` gives F, U, S per atom and dF/dG. For whole structures, `oracle_td_eval` runs the oracle's
own descriptor chain (oracle.sf.evaluate / oracle.grap.evaluate) with its module-level `apply_mlp`
replaced by the TD head through pytest's `monkeypatch`, so forces and virial come from the
oracle's exact descriptor Jacobian.
"""
import numpy as np

from oracle.sf import activation


def net_forward(layers, act, x, resnet):
    """Dense layers; returns the output and the cache of the backward pass."""
    h, cache = x, []
    L = len(layers)
    for l, (W, b) in enumerate(layers):
        z = h @ W + (b if b is not None else 0.0)
        if l < L - 1:
            a, da = activation(act, z)
            res = bool(resnet and l > 0 and W.shape[0] == W.shape[1])   # convolutional.py:272-273
            cache.append((da, res))
            h = a + h if res else a
        else:
            cache.append((None, False))
            h = z
    return h, cache


def net_backward(layers, cache, delta):
    """d(seed . output)/d(input), given delta = d/d(output) [n, out]."""
    for l in range(len(layers) - 1, -1, -1):
        W, _ = layers[l]
        da, res = cache[l]
        dz = delta * da if da is not None else delta
        back = dz @ W.T
        delta = back + delta if res else back
    return delta


def minmax(nn, el, G):
    """x and dx/dG of atomic.py:157-195 (div_no_nan)."""
    if not nn._minmax_scale:
        return G, np.ones(G.shape[1])
    xlo, xhi = (np.asarray(a, dtype=np.float64) for a in nn.minmax[el])
    den = xhi - xlo
    ok = den != 0.0
    safe = np.where(ok, den, 1.0)
    return np.where(ok, (xhi - G) / safe, 0.0), np.where(ok, -1.0 / safe, 0.0)


def td_head_element(nn, el, G, T):
    """G [n, D] of atoms of element `el`, T [n]: dict of F, U, S [n] and dFdG [n, D]."""
    ft = nn.finite_temperature_options
    w = nn.weights[el]
    x, scale = minmax(nn, el, G)
    H, cH = net_forward(w["H"], ft.activation, x, nn._use_resnet_dt)
    K = H.shape[1]
    z = np.concatenate([H, T[:, None]], axis=1)
    U, cU = net_forward(w["U"], nn._activation, z, nn._use_resnet_dt)
    s, cS = net_forward(w["S"], nn._activation, z, nn._use_resnet_dt)
    U, s = U[:, 0], s[:, 0]
    ones = np.ones((len(G), 1))
    dUdz = net_backward(w["U"], cU, ones)
    dsdz = net_backward(w["S"], cS, ones)
    somm = ft.algo == "Sommerfeld"
    S = s * T if somm else s
    F = U - T * S
    c = T if somm else 1.0
    dFdz = dUdz - (T * c)[:, None] * dsdz
    dFdx = net_backward(w["H"], cH, dFdz[:, :K])
    return {"F": F, "U": U, "S": S, "dFdG": dFdx * scale}


def td_head(nn, symbols, G, T_atoms):
    """All atoms: dict of F, U, S [N] and dFdG [N, D] (T_atoms [N] in eV)."""
    N, D = G.shape
    out = {k: np.zeros(N) for k in ("F", "U", "S")}
    out["dFdG"] = np.zeros((N, D))
    symbols = list(symbols)
    for el in nn.elements:
        idx = np.array([k for k, s in enumerate(symbols) if s == el], dtype=np.int64)
        if len(idx):
            r = td_head_element(nn, el, G[idx], np.asarray(T_atoms, dtype=np.float64)[idx])
            for k in out:
                out[k][idx] = r[k]
    return out


def oracle_td_eval(nn, atoms, monkeypatch, T=None):
    """The oracle evaluation of one structure with the TD head in place of the MLP. Returns the oracle's
    dict (energy = F, atomic = F per atom, forces, virial, descriptors, ...) plus U, S, and the per-atom
    `U_atomic`, `S_atomic`."""
    import oracle.grap
    import oracle.sf
    from tests.helpers import oracle_eval, oracle_grap_eval
    T = float(atoms.info.get("etemperature", 0.0)) if T is None else float(T)
    side = {}

    def head(model, symbols, G):
        r = td_head(nn, symbols, G, np.full(len(G), T))
        side.update(r)
        return r["F"], r["dFdG"]

    with monkeypatch.context() as m:
        m.setattr(oracle.sf, "apply_mlp", head)
        m.setattr(oracle.grap, "apply_mlp", head)
        grap = getattr(nn.descriptor, "name", "SF") == "GRAP"
        out = oracle_grap_eval(nn, atoms) if grap else oracle_eval(nn, atoms)
    out.update(U=float(side["U"].sum()), S=float(side["S"].sum()), U_atomic=side["U"], S_atomic=side["S"])
    return out
