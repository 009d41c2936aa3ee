"""NumPy reference of the device relaxation (`ta_relax_run`): ASE's `FIRE` with `downhill_check=False`, frame
by frame, with the skin / 2 list rule of `ta_update_positions` applied to count the list rebuilds as
`md_reference.run` does. Forces come from a callback, so the same loop serves an oracle, a second engine or
an analytic potential. Test infrastructure only.

Per frame, with F the forces at the current positions (those of `fixed` atoms read as 0) and |.|, . over
all 3 n components of the frame:

    before every step:  if max_i |F_i|^2 < fmax^2: the frame is converged; it does not move again in this run
    if first: v = 0; first = false
    else:
      vf = F.v
      if vf > 0:  v = (1 - a) v + a F |v| / |F|;  if npos > nmin: dt = min(dt finc, dtmax); a = a fa;  npos += 1
      else:       v = 0; a = astart; dt = dt fdec; npos = 0
    v += dt F;  dr = dt v;  if |dr| > maxstep: dr = dr maxstep / |dr|;  x += dr
"""
import numpy as np

DEFAULTS = dict(dt=0.1, dtmax=1.0, maxstep=0.2, finc=1.1, fdec=0.5, astart=0.1, fa=0.99, nmin=5)


def new_state(x0, natoms=None, **params):
    """State of a relaxation that has not taken a step. `natoms`: atoms per frame (default: one frame)."""
    p = dict(DEFAULTS)
    unknown = set(params) - set(p)
    if unknown:
        raise ValueError(f"unknown FIRE parameter {sorted(unknown)[0]}")
    p.update(params)
    x = np.array(x0, dtype=np.float64).reshape(-1, 3)
    natoms = [len(x)] if natoms is None else list(natoms)
    F = len(natoms)
    return dict(x=x, v=np.zeros_like(x), dt=np.full(F, float(p["dt"])), a=np.full(F, float(p["astart"])),
                npos=np.zeros(F, dtype=np.int64), first=np.ones(F, dtype=bool), natoms=natoms, params=p,
                ref=x.copy())


def run(force_fn, state, max_steps, fmax, fixed=None, skin=None):
    """`force_fn(x) -> (epot [n_frames], forces [N, 3])`. Continues from `state` (of `new_state` or of an earlier
    run; it is not modified) with every frame unfrozen. `fixed`: boolean mask [N]. `skin`: None = no list
    bookkeeping; otherwise the list is rebuilt whenever, after a drift, some atom is not within skin / 2 of
    where it was at the last build (so with skin = 0 after every step that moved a frame).

    Returns dict(state, x, v, dt, a, npos, steps [F], converged [F], fmax [F], energy [F], n_rebuilds,
    rebuild_steps, log). `log[k]` is the list of step k's entries, one per frame that was not frozen before the
    step: dict(frame, fmax (max |F_i| the frame was tested with), converged (it froze at this test, the other
    keys are then missing), branch ('first' | 'mix' | 'reset'), cos (vf / (|v| |F|), None at the first
    step), dr (|dr| before the clamp), dr_applied (after it), clamped, dt_grew, dt, a, npos (after the step))."""
    p = state["params"]
    x, v = state["x"].copy(), state["v"].copy()
    dt, a, npos, first = state["dt"].copy(), state["a"].copy(), state["npos"].copy(), state["first"].copy()
    ref = state["ref"].copy()
    natoms = state["natoms"]
    F = len(natoms)
    start = np.concatenate([[0], np.cumsum(natoms)]).astype(int)
    free = np.ones(len(x), dtype=bool) if fixed is None else ~np.asarray(fixed, dtype=bool).ravel()
    frozen = np.zeros(F, dtype=bool)
    steps = np.zeros(F, dtype=np.int64)
    fmax_out = np.zeros(F)
    log, rebuild_steps = [], []
    k = 0
    while True:
        e, f = force_fn(x)
        f = np.where(free[:, None], np.array(f, dtype=np.float64).reshape(-1, 3), 0.0)
        entries, moved = [], False
        for fr in range(F):
            if frozen[fr]:
                continue
            s = slice(start[fr], start[fr + 1])
            ff, vf_ = f[s], v[s]
            m2 = float((ff * ff).sum(axis=1).max()) if natoms[fr] else 0.0
            fmax_out[fr] = np.sqrt(m2)
            entry = dict(frame=fr, fmax=np.sqrt(m2), converged=bool(m2 < fmax * fmax))
            if entry["converged"]:
                frozen[fr] = True
                entries.append(entry)
                continue
            if k == max_steps:
                entries.append(entry)   # (the test of the last evaluation; no step follows)
                continue
            grew = False
            if first[fr]:
                vf_ = np.zeros_like(vf_)
                first[fr] = False
                entry.update(branch="first", cos=None)
            else:
                vf = float(np.vdot(ff, vf_))
                nv, nf = np.sqrt(np.vdot(vf_, vf_)), np.sqrt(np.vdot(ff, ff))
                entry["cos"] = vf / (nv * nf) if nv * nf > 0.0 else 0.0
                if vf > 0.0:
                    vf_ = (1.0 - a[fr]) * vf_ + a[fr] * ff * nv / nf
                    if npos[fr] > p["nmin"]:
                        grew = min(dt[fr] * p["finc"], p["dtmax"]) > dt[fr]
                        dt[fr] = min(dt[fr] * p["finc"], p["dtmax"])
                        a[fr] *= p["fa"]
                    npos[fr] += 1
                    entry["branch"] = "mix"
                else:
                    vf_ = np.zeros_like(vf_)
                    a[fr] = p["astart"]
                    dt[fr] *= p["fdec"]
                    npos[fr] = 0
                    entry["branch"] = "reset"
            vf_ = vf_ + dt[fr] * ff
            dr = dt[fr] * vf_
            norm = float(np.sqrt(np.vdot(dr, dr)))
            clamped = norm > p["maxstep"]
            if clamped:
                dr = dr * p["maxstep"] / norm
            v[s] = vf_
            xs = x[s]
            fs = free[s]
            xs[fs] = xs[fs] + dr[fs]     # (fixed atoms are not written at all)
            steps[fr] += 1
            moved = True
            entry.update(dr=norm, dr_applied=float(np.sqrt(np.vdot(dr, dr))), clamped=clamped, dt_grew=bool(grew), dt=float(dt[fr]), a=float(a[fr]),
                         npos=int(npos[fr]))
            entries.append(entry)
        if entries:
            log.append(entries)
        if not moved:
            break
        k += 1
        if skin is not None:
            d2 = ((x - ref) ** 2).sum(axis=1)
            if skin == 0.0 or not np.all(d2 <= 0.25 * skin * skin):
                ref = x.copy()
                rebuild_steps.append(k)
    out_state = dict(x=x, v=v, dt=dt, a=a, npos=npos, first=first, natoms=natoms, params=p, ref=ref)
    return dict(state=out_state, x=x, v=v, dt=dt, a=a, npos=npos, steps=steps, converged=frozen.copy(),
                fmax=fmax_out, energy=np.array(e, dtype=np.float64).reshape(-1).copy(), n_rebuilds=len(rebuild_steps),
                rebuild_steps=rebuild_steps, log=log)


def flat_log(out, frame=0):
    """The entries of one frame, in step order."""
    return [e for entries in out["log"] for e in entries if e["frame"] == frame]


def assert_not_marginal(out, fmax=None, maxstep=None, rel=1e-6):
    """No branch decision of the run is marginal: |cos| >= rel, ||dr| - maxstep| >= rel maxstep and, where the
    steps to convergence are counted (`fmax` given), |max|F| - fmax| >= rel fmax, at every step of every frame."""
    maxstep = out["state"]["params"]["maxstep"] if maxstep is None else maxstep
    for entries in out["log"]:
        for e in entries:
            if fmax is not None:
                assert abs(e["fmax"] - fmax) >= rel * fmax, e
            if e["converged"] or "branch" not in e:
                continue
            if e["cos"] is not None:
                assert abs(e["cos"]) >= rel, e
            assert abs(e["dr"] - maxstep) >= rel * maxstep, e
