"""NumPy reference of the device nudged elastic band (`ta_relax_set_band` + `ta_relax_run`): the improved
tangent of Henkelman and Jonsson (J. Chem. Phys. 113, 9978) with one spring constant, as ASE's
`NEB(method='improvedtangent', climb=...)`, under ONE FIRE (ASE's, `downhill_check=False`) over the whole band,
with the skin / 2 list rule of `ta_update_positions` applied to count the list rebuilds as
`relax_reference.run` does. Forces come from a callback, so the same loop serves an oracle, a second engine or
an analytic surface. Test infrastructure only.

The band is F >= 3 images of the same n atoms; images 0 and F - 1 are fixed endpoints. With X_i, E_i, F_i the
positions, energy and forces of image i, forces of `fixed` atoms read as 0, and ., |.| over the 3n components
of an image:

    d+ = X_{i+1} - X_i,   d- = X_i - X_{i-1}
    if   E_{i+1} > E_i > E_{i-1}:  t = d+
    elif E_{i+1} < E_i < E_{i-1}:  t = d-
    else: hi = max(|E_{i+1}-E_i|, |E_{i-1}-E_i|), lo = min(the same two)
          t = d+ hi + d- lo   if E_{i+1} > E_{i-1}   else   t = d+ lo + d- hi
    tau = t / |t|                      (t.t == 0: tau = 0)
    B_i = F_i - (F_i.tau) tau + k (|d+| - |d-|) tau          ordinary image
    B_c = F_c - 2 (F_c.tau) tau                               climbing image, if climb
    B = 0 for images 0 and F-1 and for every fixed atom

The climbing image is the interior image of highest energy, chosen anew at every step; on a tie the lowest
index wins. FIRE is the recurrence of `relax_reference` on B with one dt, one a and one npos, every ., |.| and
the maxstep clamp over all moving components of the band, and convergence when max |B_i| < fmax over the band.
"""
import numpy as np

from tests.relax_reference import DEFAULTS

GAP = 1e-6   # eV: the smallest energy gap at which a tangent case or the climbing image counts as decided


def tangent_case(em, e0, ep):
    """'up' (t = d+), 'down' (t = d-) or 'mixed' for an image with neighbours' energies em, ep."""
    if ep > e0 > em:
        return "up"
    if ep < e0 < em:
        return "down"
    return "mixed"


def band_forces(X, E, F, k, climb=False, fixed=None):
    """X, F [n_images, n, 3], E [n_images], `fixed` boolean [n] or None. Returns (B [n_images, n, 3],
    tau [n_images, n, 3], climbing image index or -1)."""
    X, F, E = np.asarray(X, dtype=np.float64), np.asarray(F, dtype=np.float64), np.asarray(E, dtype=np.float64)
    nim, n = X.shape[0], X.shape[1]
    free = np.ones(n, dtype=bool) if fixed is None else ~np.asarray(fixed, dtype=bool).ravel()
    F = np.where(free[None, :, None], F, 0.0)
    B, tau = np.zeros_like(X), np.zeros_like(X)
    c = -1
    if climb:
        c = 1
        for i in range(2, nim - 1):
            if E[i] > E[c]:
                c = i
    for i in range(1, nim - 1):
        dp, dm = X[i + 1] - X[i], X[i] - X[i - 1]
        case = tangent_case(E[i - 1], E[i], E[i + 1])
        if case == "up":
            t = dp.copy()
        elif case == "down":
            t = dm.copy()
        else:
            up, dn = abs(E[i + 1] - E[i]), abs(E[i - 1] - E[i])
            hi, lo = max(up, dn), min(up, dn)
            t = dp * hi + dm * lo if E[i + 1] > E[i - 1] else dp * lo + dm * hi
        tt = float(np.vdot(t, t))
        if tt != 0.0:
            tau[i] = t / np.sqrt(tt)
        ftau = float(np.vdot(F[i], tau[i]))
        if i == c:
            B[i] = F[i] - 2.0 * ftau * tau[i]
        else:
            B[i] = F[i] - ftau * tau[i] + k * (np.sqrt(np.vdot(dp, dp)) - np.sqrt(np.vdot(dm, dm))) * tau[i]
        B[i][~free] = 0.0
    return B, tau, c


def new_state(X0, **params):
    """State of a band optimisation that has not taken a step. X0 [n_images, n, 3]."""
    p = dict(DEFAULTS)
    unknown = set(params) - set(p)
    if unknown:
        raise ValueError(f"unknown FIRE parameter {sorted(unknown)[0]}")
    p.update(params)
    x = np.array(X0, dtype=np.float64)
    assert x.ndim == 3 and x.shape[0] >= 3 and x.shape[2] == 3
    return dict(x=x, v=np.zeros_like(x), dt=float(p["dt"]), a=float(p["astart"]), npos=0, first=True, params=p,
                ref=x.copy())


def run(force_fn, state, max_steps, fmax, k=0.1, climb=False, fixed=None, skin=None):
    """`force_fn(x [n_images * n, 3]) -> (energies [n_images], forces [n_images * n, 3])`. Continues from `state`
    (of `new_state` or of an earlier run; it is not modified). `fixed`: boolean mask [n] applied to every
    image. `skin`: None = no list bookkeeping; otherwise the list is rebuilt whenever, after a drift, some atom
    of some image is not within skin / 2 of where it was at the last build (skin = 0: after every step).

    Returns dict(state, x, v [n_images, n, 3], dt, a, npos, steps, converged, fmax (the band's max |B_i| of the
    final state), energy [n_images], band, tau, climbing (of the final state), n_rebuilds, rebuild_steps, log).
    `log[s]` describes the test before step s and the step, if one followed: dict(fmax, converged, cases (the
    tangent case of every interior image), gaps ([n_images - 2, 2]: |E_{i+1} - E_i|, |E_{i-1} - E_i|), top_gap
    (between the two highest interior energies; None with one interior image), climbing, and for a step: branch
    ('first' | 'mix' | 'reset'), cos (B.v / (|B||v|), None at the first step), dr (|dr| before the clamp),
    dr_applied, clamped, dt_grew, dt, a, npos (after the step))."""
    p = state["params"]
    x, v = state["x"].copy(), state["v"].copy()
    dt, a, npos, first = state["dt"], state["a"], state["npos"], state["first"]
    ref = state["ref"].copy()
    nim, n = x.shape[0], x.shape[1]
    moving = np.zeros((nim, n), dtype=bool)
    moving[1:-1] = True if fixed is None else ~np.asarray(fixed, dtype=bool).ravel()
    log, rebuild_steps = [], []
    steps, converged = 0, False
    while True:
        e, f = force_fn(x.reshape(-1, 3))
        e = np.array(e, dtype=np.float64).reshape(nim)
        f = np.array(f, dtype=np.float64).reshape(nim, n, 3)
        B, tau, c = band_forces(x, e, f, k, climb, fixed)
        m2 = float((B * B).sum(axis=2).max())
        inner = np.sort(e[1:-1])
        entry = dict(fmax=np.sqrt(m2), converged=bool(m2 < fmax * fmax), climbing=c,
                     cases=[tangent_case(e[i - 1], e[i], e[i + 1]) for i in range(1, nim - 1)],
                     gaps=np.array([[abs(e[i + 1] - e[i]), abs(e[i - 1] - e[i])] for i in range(1, nim - 1)]),
                     top_gap=float(inner[-1] - inner[-2]) if len(inner) > 1 else None)
        log.append(entry)
        if entry["converged"]:
            converged = True
            break
        if steps == max_steps:
            break
        grew = False
        if first:
            v = np.zeros_like(v)
            first = False
            entry.update(branch="first", cos=None)
        else:
            vf = float(np.vdot(B, v))
            nv, nf = np.sqrt(np.vdot(v, v)), np.sqrt(np.vdot(B, B))
            entry["cos"] = vf / (nv * nf) if nv * nf > 0.0 else 0.0
            if vf > 0.0:
                v = (1.0 - a) * v + a * B * nv / nf
                if npos > p["nmin"]:
                    grew = min(dt * p["finc"], p["dtmax"]) > dt
                    dt = min(dt * p["finc"], p["dtmax"])
                    a *= p["fa"]
                npos += 1
                entry["branch"] = "mix"
            else:
                v = np.zeros_like(v)
                a = p["astart"]
                dt *= p["fdec"]
                npos = 0
                entry["branch"] = "reset"
        v = v + dt * B
        dr = dt * v
        norm = float(np.sqrt(np.vdot(dr, dr)))
        clamped = norm > p["maxstep"]
        if clamped:
            dr = dr * p["maxstep"] / norm
        x[moving] = x[moving] + dr[moving]     # (endpoints and fixed atoms are not written at all)
        steps += 1
        entry.update(dr=norm, dr_applied=float(np.sqrt(np.vdot(dr, dr))), clamped=clamped, dt_grew=bool(grew),
                     dt=float(dt), a=float(a), npos=int(npos))
        if skin is not None:
            d2 = ((x - ref) ** 2).sum(axis=2)
            if skin == 0.0 or not np.all(d2 <= 0.25 * skin * skin):
                ref = x.copy()
                rebuild_steps.append(steps)
    out_state = dict(x=x, v=v, dt=dt, a=a, npos=npos, first=first, params=p, ref=ref)
    return dict(state=out_state, x=x, v=v, dt=dt, a=a, npos=npos, steps=steps, converged=converged,
                fmax=log[-1]["fmax"], energy=e.copy(), band=B, tau=tau, climbing=c,
                n_rebuilds=len(rebuild_steps), rebuild_steps=rebuild_steps, log=log)


def assert_not_marginal(out, fmax=None, climb=False, maxstep=None, rel=1e-6, gap=GAP):
    """No decision of the run is marginal, at every step: the three conditions of
    `relax_reference.assert_not_marginal` (|cos| >= rel, ||dr| - maxstep| >= rel maxstep and, with `fmax` given,
    |max|B| - fmax| >= rel fmax), every energy gap that picks a tangent case or its weights >= `gap` eV and,
    under `climb`, the gap between the two highest interior energies >= `gap` eV."""
    maxstep = out["state"]["params"]["maxstep"] if maxstep is None else maxstep
    for e in out["log"]:
        assert e["gaps"].min() >= gap, e
        if climb and e["top_gap"] is not None:
            assert e["top_gap"] >= gap, e
        if fmax is not None:
            assert abs(e["fmax"] - fmax) >= rel * fmax, e
        if e["converged"] or "branch" not in e:
            continue
        if e["cos"] is not None:
            assert abs(e["cos"]) >= rel, e
        assert abs(e["dr"] - maxstep) >= rel * maxstep, e
