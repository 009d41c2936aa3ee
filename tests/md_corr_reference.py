"""NumPy reference of the time correlations of the device MD loop (`ta_md_set_sampling`, csrc/ta_md_corr.hip).

Samples are numbered n = 0, 1, ...; at every new sample n, for every lag k = 0 .. min(n, L - 1), frame f and
element e:
    A_v[f, e, k] += sum_{i in f, species e} v_i(n) . v_i(n - k)
    A_x[f, e, k] += sum_{i in f, species e} |x_i(n) - x_i(n - k)|^2
With n_k = max(0, n_samples - k) time origins at lag k and N_fe atoms, vacf = A_v / (n_k N_fe) and
msd = A_x / (n_k N_fe), NaN where n_k N_fe = 0. No centre-of-mass correction.

`correlate` is the definition as direct loops. The trajectory builders return the whole-step (x, v) of every step
by calling the references of the integrators one step at a time, so the dynamics are the ones those pin.
"""
import numpy as np

from tests import md_langevin_reference, md_nhc_reference, md_reference


def correlate(xs, vs, natoms, species, n_elements, n_lags):
    """`xs`, `vs` [n_samples, N, 3]; `natoms` atoms per frame; `species` [N] element index of every atom.
    Returns dict(vacf_sum, msd_sum [F, E, L], vacf, msd (normalised, NaN where undefined), n_origins [L],
    counts [F, E], and for the rounding bound of a sum taken in any order, per entry: n_terms_v, n_terms_x
    (scalar products added, three per atom and origin) and abs_v, abs_x (the sum of their absolute values))."""
    xs, vs = np.asarray(xs, dtype=np.float64), np.asarray(vs, dtype=np.float64)
    species = np.asarray(species)
    S, F, E, L = len(xs), len(natoms), int(n_elements), int(n_lags)
    start = np.concatenate([[0], np.cumsum(natoms)])
    shape = (F, E, L)
    out = {k: np.zeros(shape) for k in ("vacf_sum", "msd_sum", "abs_v", "abs_x")}
    out["n_terms_v"], out["n_terms_x"] = np.zeros(shape, dtype=np.int64), np.zeros(shape, dtype=np.int64)
    counts = np.zeros((F, E), dtype=np.int64)
    members = {}
    for f in range(F):
        for e in range(E):
            idx = np.arange(start[f], start[f + 1])
            members[f, e] = idx[species[idx] == e]
            counts[f, e] = len(members[f, e])
    for n in range(S):
        for k in range(min(n, L - 1) + 1):
            for f in range(F):
                for e in range(E):
                    i = members[f, e]
                    pv = vs[n, i] * vs[n - k, i]
                    dx = xs[n, i] - xs[n - k, i]
                    px = dx * dx
                    out["vacf_sum"][f, e, k] += pv.sum()
                    out["msd_sum"][f, e, k] += px.sum()
                    out["abs_v"][f, e, k] += np.abs(pv).sum()
                    out["abs_x"][f, e, k] += px.sum()
                    out["n_terms_v"][f, e, k] += pv.size
                    out["n_terms_x"][f, e, k] += px.size
    n_origins = np.maximum(0, S - np.arange(L))
    den = (counts[:, :, None] * n_origins[None, None, :]).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["vacf"] = np.where(den > 0, out["vacf_sum"] / den, np.nan)
        out["msd"] = np.where(den > 0, out["msd_sum"] / den, np.nan)
    out["n_origins"], out["counts"] = n_origins, counts
    return out


def _memo(force_fn):
    """The step-by-step drivers evaluate every state twice (last of one call, first of the next): keep one."""
    last = {}

    def force(x):
        key = np.ascontiguousarray(x).tobytes()
        if last.get("key") != key:
            e, f = force_fn(x)
            last.update(key=key, e=np.array(e, dtype=np.float64), f=np.array(f, dtype=np.float64))
        return last["e"].copy(), last["f"].copy()
    return force


def _collect(x0, v0, n_steps, one_step):
    x = np.array(x0, dtype=np.float64).reshape(-1, 3)
    v = np.array(v0, dtype=np.float64).reshape(-1, 3)
    xs, vs, ekin = [x.copy()], [v.copy()], []
    for k in range(n_steps):
        out = one_step(k, x, v)
        if k == 0:
            ekin.append(out["ekin"][0])
        x, v = out["x"], out["v"]
        xs.append(x.copy())
        vs.append(v.copy())
        ekin.append(out["ekin"][1])
    return np.array(xs), np.array(vs), np.array(ekin)


def trajectory_verlet(force_fn, x0, v0, masses, dt, n_steps, natoms=None, kT0=0.0, tau=0.0):
    """(xs, vs [n_steps + 1, N, 3], ekin [n_steps + 1, F]) of velocity Verlet, with kT0 > 0 under Berendsen: the
    velocities after the second half-kick, before the next step's factor."""
    force = _memo(force_fn)
    return _collect(x0, v0, n_steps, lambda k, x, v: md_reference.run(force, x, v, masses, dt, 1, natoms=natoms,
                                                                      kT0=kT0, tau=tau))


def trajectory_langevin(force_fn, x0, v0, masses, dt, n_steps, kT0, friction, seed, natoms=None):
    """... of the Langevin step: the velocities after the second update of each step."""
    force = _memo(force_fn)
    return _collect(x0, v0, n_steps, lambda k, x, v: md_langevin_reference.run(
        force, x, v, masses, dt, 1, kT0, friction, seed, natoms=natoms, first_step=k))


def trajectory_nhc(force_fn, x0, v0, masses, dt, n_steps, kT0, tau, chain=3, loops=1, dof_removed=0, natoms=None):
    """... of the Nose-Hoover chain: the velocities after the closing half-update of each step."""
    force = _memo(force_fn)
    state = {"eta": None, "veta": None}

    def one_step(k, x, v):
        out = md_nhc_reference.run(force, x, v, masses, dt, 1, kT0, tau, chain=chain, loops=loops,
                                   dof_removed=dof_removed, natoms=natoms, eta0=state["eta"], veta0=state["veta"])
        state["eta"], state["veta"] = out["eta"].copy(), out["veta"].copy()
        return out
    return _collect(x0, v0, n_steps, one_step)
