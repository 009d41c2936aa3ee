"""NumPy reference of the device MD loop (`ta_md_run`): ASE's `VelocityVerlet` step and
`NVTBerendsen.scale_velocities`, with the skin / 2 list rule of `ta_update_positions` applied to count the
list rebuilds. Forces come from a callback, so the same loop serves an oracle, a second engine or an
analytic potential. Test infrastructure only.

    v' = v + dt/2 F(x)/m;   x <- x + dt v';   v <- v' + dt/2 F(x)/m

Before each step, per frame: kT = 2 KE / (3 n), lambda = sqrt(1 + (kT0 / kT - 1) dt / tau) clamped to
[0.9, 1.1] (1 when KE = 0), v <- lambda v. No centre-of-mass fix."""
import numpy as np


def kinetic_energies(masses, v, natoms):
    """Per-frame kinetic energies of the concatenated atoms."""
    e = 0.5 * masses * (v * v).sum(axis=1)
    out, a = np.zeros(len(natoms)), 0
    for f, n in enumerate(natoms):
        out[f] = e[a:a + n].sum()
        a += n
    return out


def berendsen_factors(ke, natoms, kT0, dt, tau):
    lam = np.ones(len(natoms))
    for f, n in enumerate(natoms):
        if ke[f] > 0.0:
            kT = 2.0 * ke[f] / (3.0 * n)
            lam[f] = min(1.1, max(0.9, np.sqrt(1.0 + (kT0 / kT - 1.0) * dt / tau)))
    return lam


def run(force_fn, x0, v0, masses, dt, n_steps, natoms=None, skin=None, kT0=0.0, tau=0.0, record_every=1):
    """`force_fn(x) -> (epot [n_frames], forces [N, 3])`. `natoms`: atoms per frame (default: one frame).
    `skin`: None = no list bookkeeping; otherwise the list is rebuilt whenever, after a drift, some atom is
    not within skin / 2 of where it was at the last build (so with skin = 0 after every step).
    Returns dict(x, v, epot, ekin [n_steps // record_every + 1, n_frames], n_rebuilds, rebuild_steps)."""
    x = np.array(x0, dtype=np.float64).reshape(-1, 3)
    v = np.array(v0, dtype=np.float64).reshape(-1, 3)
    m = np.asarray(masses, dtype=np.float64).ravel()
    natoms = [len(x)] if natoms is None else list(natoms)
    frame = np.repeat(np.arange(len(natoms)), natoms)
    ref = x.copy()
    rebuild_steps = []
    epot, ekin = [], []
    e, f = force_fn(x)
    for k in range(n_steps + 1):
        ke = kinetic_energies(m, v, natoms)
        if k % record_every == 0:
            epot.append(np.array(e, dtype=np.float64).reshape(-1).copy())
            ekin.append(ke)
        if k == n_steps:
            break
        if kT0 > 0.0:
            v = v * berendsen_factors(ke, natoms, kT0, dt, tau)[frame][:, None]
        v = v + 0.5 * dt * f / m[:, None]
        x = x + dt * v
        if skin is not None:
            d2 = ((x - ref) ** 2).sum(axis=1)
            if skin == 0.0 or not np.all(d2 <= 0.25 * skin * skin):
                ref = x.copy()
                rebuild_steps.append(k + 1)
        e, f = force_fn(x)
        v = v + 0.5 * dt * f / m[:, None]
    return dict(x=x, v=v, epot=np.array(epot), ekin=np.array(ekin), n_rebuilds=len(rebuild_steps),
                rebuild_steps=rebuild_steps)
