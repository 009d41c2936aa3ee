"""NumPy reference of the Berendsen barostat of the device MD loop (`ta_md_set_barostat`, `ta_md_run`): ASE's
`NPTBerendsen` (isotropic) and `Inhomogeneous_NPTBerendsen` (per axis) with one force evaluation per step, under
velocity Verlet, the Berendsen thermostat or the Langevin step of `tests/md_langevin_reference.py`. Forces come
from a callback `force_fn(x, cells) -> (e [F], forces [N, 3], virial [F, 3, 3])`, so the same loop serves an
oracle, a second engine or an analytic potential. Test infrastructure only.

Per frame, with h the cell (rows are lattice vectors), V = |det h| and W the virial (dE / d strain) of the
evaluation at x_k, step k -> k + 1 does:

    1. Berendsen thermostat: v <- lambda v (`md_reference.berendsen_factors`); Langevin: nothing here
    2. P_c = (sum_i m_i v_ic^2 - W_cc) / V from the velocities after 1.
       isotropic (mask None): P = (P_x + P_y + P_z) / 3, mu_c = 1 - (dt / taup) (beta / 3) (P0 - P) for all c
       mask: mu_c = 1 - (dt / taup) (beta / 3) (P0 - P_c) on free axes, mu_c = 1 exactly on the others
       x_ic <- mu_c x_ic,  h[:, c] <- mu_c h[:, c]   (velocities are not scaled, mu is not clamped)
    3. the half-kick and the drift (Langevin: the first update and the drift) with F_k, the forces at the
       UNSCALED x_k; then the evaluation at x_{k+1} and the second half-kick (update)

Records (slot k // record_every for every k that is a multiple of record_every, the entry state first): epot,
ekin = half the total of the three sums, volume and press = (sums - diag W) / V of the state, from the
velocities BEFORE the thermostat's scaling.

List bookkeeping (`skin` not None): s is the product of the mu since the list was built (h = h_ref diag(s)),
u_i = x_i - x_ref,i o s, lim = (skin - (rc + skin) |s - 1|_2) / 2 per frame; the list of the whole batch is
rebuilt after a drift when some frame has lim <= 0 or some |u_i|^2 >= lim^2. `log` holds, per step, the arrays
lim [F], max |u| [F] and max |x - x_ref| [F] before the decision; `end_rebuild` says whether the run ended with
cells other than its list's (the device then builds one more list)."""
import numpy as np

from tests import md_reference


def frame_sums(masses, v, natoms):
    """[F, 3]: sum_i m_i v_ic^2 per frame."""
    t = masses[:, None] * v * v
    out, a = np.zeros((len(natoms), 3)), 0
    for f, n in enumerate(natoms):
        out[f] = t[a:a + n].sum(axis=0)
        a += n
    return out


def volumes(cells):
    return np.abs(np.linalg.det(cells))


def scale_factors(S, W, V, dt, pressure, taup, beta, mask):
    """mu [F, 3] from the kinetic sums S [F, 3], the virials W [F, 3, 3] and the volumes V [F]."""
    P = (S - np.diagonal(W, axis1=1, axis2=2)) / V[:, None]
    if mask is None:
        P = np.repeat(P.mean(axis=1)[:, None], 3, axis=1)
    mu = 1.0 - dt / taup * beta / 3.0 * (pressure - P)
    if mask is not None:
        mu = np.where(np.asarray(mask, dtype=bool)[None, :], mu, 1.0)
    return mu


def run(force_fn, x0, v0, masses, cells0, dt, n_steps, pressure, taup, beta, mask=None, natoms=None, skin=None,
        rc=None, kT0=0.0, tau=0.0, friction=0.0, lv_kT0=0.0, noise=None, first_step=0, record_every=1):
    """`noise(step) -> (xi, eta) [N, 3]`: the normals of absolute step `step` (Langevin, `friction` > 0).
    Returns dict(x, v, cells, epot, ekin, volume [n_rec, F], press [n_rec, F, 3], mu [n_steps, F, 3], n_rebuilds,
    rebuild_steps, end_rebuild, log)."""
    x = np.array(x0, dtype=np.float64).reshape(-1, 3)
    v = np.array(v0, dtype=np.float64).reshape(-1, 3)
    m = np.asarray(masses, dtype=np.float64).ravel()
    h = np.array(cells0, dtype=np.float64).reshape(-1, 3, 3)
    natoms = [len(x)] if natoms is None else list(natoms)
    F = len(natoms)
    assert len(h) == F and not (kT0 > 0.0 and friction > 0.0)
    frame = np.repeat(np.arange(F), natoms)
    fr = float(friction)
    if fr > 0.0:
        sigma = np.sqrt(2.0 * lv_kT0 * fr / m)[:, None]
        c1 = dt / 2.0 - dt * dt * fr / 8.0
        c2 = dt * fr / 2.0 - dt * dt * fr * fr / 8.0
        c3 = np.sqrt(dt) * sigma / 2.0 - dt ** 1.5 * fr * sigma / 8.0
        c5 = dt ** 1.5 * sigma / (2.0 * np.sqrt(3.0))
        c4 = fr / 2.0 * c5
    ref, ref_cells, s = x.copy(), h.copy(), np.ones((F, 3))
    rebuild_steps, log, mus = [], [], []
    epot, ekin, vol, press = [], [], [], []
    e, f, W = force_fn(x, h)
    W = np.asarray(W, dtype=np.float64).reshape(F, 3, 3)
    for k in range(n_steps + 1):
        S = frame_sums(m, v, natoms)
        ke = 0.5 * S.sum(axis=1)
        V = volumes(h)
        if k % record_every == 0:
            epot.append(np.array(e, dtype=np.float64).reshape(-1).copy())
            ekin.append(ke)
            vol.append(V)
            press.append((S - np.diagonal(W, axis1=1, axis2=2)) / V[:, None])
        if k == n_steps:
            break
        if kT0 > 0.0:
            v = v * md_reference.berendsen_factors(ke, natoms, kT0, dt, tau)[frame][:, None]
            S = frame_sums(m, v, natoms)
        mu = scale_factors(S, W, V, dt, pressure, taup, beta, mask)
        mus.append(mu)
        x = x * mu[frame]
        h = h * mu[:, None, :]
        s = s * mu
        if fr > 0.0:
            xi, eta = noise(first_step + k)
            rv, rp = c3 * xi - c4 * eta, c5 * eta
            v = v + (c1 * f / m[:, None] - c2 * v + rv)
            x = x + dt * v + rp
        else:
            v = v + 0.5 * dt * f / m[:, None]
            x = x + dt * v
        if skin is not None:
            lim = 0.5 * (skin - (rc + skin) * np.sqrt(((s - 1.0) ** 2).sum(axis=1)))
            u2 = ((x - ref * s[frame]) ** 2).sum(axis=1)
            d2 = ((x - ref) ** 2).sum(axis=1)
            umax, dmax, a = np.zeros(F), np.zeros(F), 0
            for j, n in enumerate(natoms):
                if n:
                    umax[j], dmax[j] = np.sqrt(u2[a:a + n].max()), np.sqrt(d2[a:a + n].max())
                a += n
            log.append(dict(step=k + 1, lim=lim, umax=umax, dmax=dmax))
            if np.any(lim <= 0.0) or np.any(u2 >= (lim * lim)[frame]):
                ref, ref_cells, s = x.copy(), h.copy(), np.ones((F, 3))
                rebuild_steps.append(k + 1)
        e, f, W = force_fn(x, h)
        W = np.asarray(W, dtype=np.float64).reshape(F, 3, 3)
        if fr > 0.0:
            v = v + (c1 * f / m[:, None] - c2 * v + rv)
        else:
            v = v + 0.5 * dt * f / m[:, None]
    return dict(x=x, v=v, cells=h, epot=np.array(epot), ekin=np.array(ekin), volume=np.array(vol),
                press=np.array(press), mu=np.array(mus).reshape(-1, F, 3), n_rebuilds=len(rebuild_steps),
                rebuild_steps=rebuild_steps, end_rebuild=bool(skin is not None and not np.array_equal(h, ref_cells)),
                log=log)


def assert_not_marginal(out, skin, rel=1e-6):
    """No staleness decision of the run's log is within `rel` (relative) of its threshold: the sign of lim
    against the skin, and the largest |u| against lim where lim > 0."""
    for rec in out["log"]:
        for lim, umax in zip(rec["lim"], rec["umax"]):
            if skin == 0.0:
                continue   # (lim = 0 exactly: every step rebuilds)
            assert abs(lim) > rel * skin, ("marginal lim", rec["step"], lim)
            if lim > 0.0:
                assert abs(umax - lim) > rel * lim, ("marginal |u|", rec["step"], umax, lim)
