"""NumPy reference of the device relaxation with cells (`ta_relax_set_cell` + `ta_relax_run`): the construction
of ASE's `UnitCellFilter` under ASE's `FIRE` with `downhill_check=False`, frame by frame, with the strain-aware
list rule of the device loop applied to count the list rebuilds. Energies, forces and virials come from a
callback, so the same loop serves an oracle, a second engine or an analytic energy. Test infrastructure only.

Per frame of n atoms: h0 the cell at the start (rows are lattice vectors), G a deformation gradient (identity at
the start), cf the cell factor (default n), p an external pressure, M a symmetric 0/1 mask:

    h = h0 G^T,  x_i = q_i G^T,  generalised coordinates: the n + 3 rows [q_1 .. q_n ; cf G]
    f_i    = F_i G                                  (a fixed atom: 0)
    f_cell = -((W + p V I) G^-T)                    hydrostatic: f_cell = I trace(f_cell) / 3
    f_cell = f_cell o M / cf

with W the virial (dE / d strain) and V = |det h|. FIRE is the recurrence of `relax_reference` over all
3 (n + 3) components and n + 3 rows (convergence: max_row |f_row|^2 < fmax^2). The step, with the clamped dr:

    q_i = x_i G^-T;  q_i += dr_i;  G += dr_cell / cf;  h = h0 G^T;  x_i = q_i G^T

List rule: with h_ref, x_ref of the last build, rc = max(rcut, acut), A = h_ref^-1 h, u_i = x_i - x_ref,i A the
list is stale when lim = (skin - (rc + skin) |A - I|_F) / 2 <= 0 or some |u_i|^2 >= lim^2.
"""
import numpy as np

from tests.relax_reference import DEFAULTS, assert_not_marginal, flat_log  # noqa: F401  (same conventions)


def voigt_mask(mask):
    """6 Voigt entries (xx, yy, zz, yz, xz, xy; None: all free) as a symmetric 3 x 3 array of 0. / 1."""
    m = np.ones(6) if mask is None else (np.asarray(mask).reshape(6) != 0).astype(np.float64)
    return np.array([[m[0], m[5], m[4]], [m[5], m[1], m[3]], [m[4], m[3], m[2]]])


def new_state(x0, cells, natoms=None, cell_factor=None, pressure=0.0, mask=None, hydrostatic=False, **params):
    """State of a cell relaxation that has not taken a step. `cells` [F, 3, 3]; `natoms`: atoms per frame."""
    p = dict(DEFAULTS)
    unknown = set(params) - set(p)
    if unknown:
        raise ValueError(f"unknown FIRE parameter {sorted(unknown)[0]}")
    p.update(params)
    x = np.array(x0, dtype=np.float64).reshape(-1, 3)
    natoms = [len(x)] if natoms is None else list(natoms)
    F = len(natoms)
    cells = np.array(cells, dtype=np.float64).reshape(F, 3, 3)
    cf = np.array([float(n) if cell_factor is None else float(cell_factor) for n in natoms])
    return dict(x=x, v=np.zeros_like(x), cells=cells, h0=cells.copy(), G=np.tile(np.eye(3), (F, 1, 1)),
                vc=np.zeros((F, 3, 3)), dt=np.full(F, float(p["dt"])), a=np.full(F, float(p["astart"])),
                npos=np.zeros(F, dtype=np.int64), first=np.ones(F, dtype=bool), natoms=natoms, params=p,
                cell=dict(cf=cf, pressure=float(pressure), mask=voigt_mask(mask), hydrostatic=bool(hydrostatic)),
                ref=x.copy(), ref_cells=cells.copy())


def generalized_forces(F_atoms, W, G, h, cf, pressure, mask, hydrostatic, free=None):
    """(f [n, 3], f_cell [3, 3]) of one frame."""
    f = F_atoms @ G
    if free is not None:
        f = np.where(free[:, None], f, 0.0)
    V = abs(np.linalg.det(h))
    fc = -((W + pressure * V * np.eye(3)) @ np.linalg.inv(G).T)
    if hydrostatic:
        fc = np.eye(3) * np.trace(fc) / 3.0
    return f, fc * mask / cf


def list_is_stale(x, ref, h, h_ref, skin, rc):
    """The strain-aware rule for one frame; also returns (lim, max |u|, max |x - x_ref|)."""
    A = np.linalg.inv(h_ref) @ h
    lim = 0.5 * (skin - (rc + skin) * np.sqrt(((A - np.eye(3)) ** 2).sum()))
    u2 = ((x - ref @ A) ** 2).sum(axis=1) if len(x) else np.zeros(0)
    stale = bool(lim <= 0.0 or not np.all(u2 < lim * lim))
    plain = float(np.sqrt(((x - ref) ** 2).sum(axis=1).max())) if len(x) else 0.0
    return stale, (float(lim), float(np.sqrt(u2.max())) if len(x) else 0.0, plain)


def run(force_fn, state, max_steps, fmax, fixed=None, skin=None, rc=None):
    """`force_fn(x, cells) -> (epot [F], forces [N, 3], virial [F, 3, 3])`. Continues from `state` (of `new_state`
    or of an earlier run; it is not modified) with every frame unfrozen. `fixed`: boolean mask [N]. `skin`: None =
    no list bookkeeping; otherwise (`rc` is then needed) the list is rebuilt whenever the strain-aware rule finds
    it stale after a step. As on the device, a run that ends with cells other than those of its list rebuilds once
    more for the final state: `end_rebuild` (not among `rebuild_steps`).

    Returns dict(state, x, v, G, vc, cells, dt, a, npos, steps [F], converged [F], fmax [F], cell_fmax [F],
    energy [F], virial [F, 3, 3], n_rebuilds, rebuild_steps, rebuild_info, end_rebuild, log). The log is that of
    `relax_reference.run` with `cell_fmax` (max row |f_cell|) added; `rebuild_info[k]` = dict(step, lim, u, plain)
    of the frame that made the list stale (plain = max |x - x_ref|, what the fixed-cell rule looks at)."""
    p = state["params"]
    c = state["cell"]
    x, v = state["x"].copy(), state["v"].copy()
    cells, h0, G, vc = state["cells"].copy(), state["h0"], state["G"].copy(), state["vc"].copy()
    dt, a, npos, first = state["dt"].copy(), state["a"].copy(), state["npos"].copy(), state["first"].copy()
    ref, ref_cells = state["ref"].copy(), state["ref_cells"].copy()
    natoms = state["natoms"]
    F = len(natoms)
    start = np.concatenate([[0], np.cumsum(natoms)]).astype(int)
    free = np.ones(len(x), dtype=bool) if fixed is None else ~np.asarray(fixed, dtype=bool).ravel()
    frozen = np.zeros(F, dtype=bool)
    steps = np.zeros(F, dtype=np.int64)
    fmax_out, cell_fmax = np.zeros(F), np.zeros(F)
    log, rebuild_steps, rebuild_info = [], [], []
    k = 0
    while True:
        e, f_all, w_all = force_fn(x, cells)
        f_all = np.array(f_all, dtype=np.float64).reshape(-1, 3)
        w_all = np.array(w_all, dtype=np.float64).reshape(F, 3, 3)
        entries, moved = [], False
        for fr in range(F):
            if frozen[fr]:
                continue
            s = slice(start[fr], start[fr + 1])
            n = natoms[fr]
            fa, fc = generalized_forces(f_all[s], w_all[fr], G[fr], cells[fr], c["cf"][fr], c["pressure"], c["mask"],
                                        c["hydrostatic"], free[s])
            ff = np.vstack([fa, fc])
            vf_ = np.vstack([v[s], vc[fr]])
            m2 = float((ff * ff).sum(axis=1).max())
            fmax_out[fr] = np.sqrt(m2)
            cell_fmax[fr] = np.sqrt((fc * fc).sum(axis=1).max())
            entry = dict(frame=fr, fmax=np.sqrt(m2), cell_fmax=float(cell_fmax[fr]), converged=bool(m2 < fmax * fmax))
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
            v[s], vc[fr] = vf_[:n], vf_[n:]
            q = x[s] @ np.linalg.inv(G[fr]).T + dr[:n]   # (a fixed atom has f = 0 and v = 0: its q stays)
            G[fr] = G[fr] + dr[n:] / c["cf"][fr]
            cells[fr] = h0[fr] @ G[fr].T
            x[s] = q @ G[fr].T
            steps[fr] += 1
            moved = True
            entry.update(dr=norm, dr_applied=float(np.sqrt(np.vdot(dr, dr))), clamped=clamped, dt_grew=bool(grew),
                         dt=float(dt[fr]), a=float(a[fr]), npos=int(npos[fr]))
            entries.append(entry)
        if entries:
            log.append(entries)
        if not moved:
            break
        k += 1
        if skin is not None:
            for fr in range(F):
                s = slice(start[fr], start[fr + 1])
                stale, (lim, u, plain) = list_is_stale(x[s], ref[s], cells[fr], ref_cells[fr], skin, rc)
                if stale:
                    ref, ref_cells = x.copy(), cells.copy()
                    rebuild_steps.append(k)
                    rebuild_info.append(dict(step=k, frame=fr, lim=lim, u=u, plain=plain))
                    break
    end_rebuild = bool(skin is not None and not np.array_equal(cells, ref_cells))
    if end_rebuild:
        ref, ref_cells = x.copy(), cells.copy()
    out_state = dict(x=x, v=v, cells=cells, h0=h0, G=G, vc=vc, dt=dt, a=a, npos=npos, first=first, natoms=natoms,
                     params=p, cell=c, ref=ref, ref_cells=ref_cells)
    return dict(state=out_state, x=x, v=v, G=G, vc=vc, cells=cells, dt=dt, a=a, npos=npos, steps=steps,
                converged=frozen.copy(), fmax=fmax_out, cell_fmax=cell_fmax,
                energy=np.array(e, dtype=np.float64).reshape(-1).copy(), virial=w_all.copy(),
                n_rebuilds=len(rebuild_steps), rebuild_steps=rebuild_steps, rebuild_info=rebuild_info,
                end_rebuild=end_rebuild, log=log)
