"""NumPy reference of the Nose-Hoover chain thermostat of the device MD loop (`ta_md_set_nose_hoover`,
`ta_md_run`): the scheme of include/tensoralloy_amd.h, with the skin / 2 list rule of `ta_update_positions`
applied to count the list rebuilds, and optionally the Berendsen barostat of tests/md_npt_reference.py. Forces
come from a callback, so the same loop serves an oracle, a second engine or an analytic potential. Test
infrastructure only.

Per frame: g = 3 n - dof_removed, a chain of M thermostats (eta_k, veta_k) with Q_1 = g kT0 tau^2 and
Q_k = kT0 tau^2 (k >= 2), G_1 = (2 K - g kT0) / Q_1, G_k = (Q_{k-1} veta_{k-1}^2 - kT0) / Q_k. One half-update
over Delta = dt / 2 is L loops of d = Delta / L, s starting at 1 and G_1 taken with the current K s^2:

    veta_M += (d/2) G_M
    for k = M-1 .. 1:  a = exp(-(d/4) veta_{k+1});  veta_k = (veta_k a + (d/2) G_k) a
    s *= exp(-d veta_1);   eta_k += d veta_k
    for k = 1 .. M-1:  a = exp(-(d/4) veta_{k+1});  veta_k = (veta_k a + (d/2) G_k) a
    veta_M += (d/2) G_M

then v <- s v. A step: half-update; v += dt/2 F/m; x += dt v; evaluate; v += dt/2 F/m; half-update. Records:
slot 0 the state at entry, slot r > 0 the state after the closing half-update of its step, with
echain = sum_k Q_k veta_k^2 / 2 + g kT0 eta_1 + kT0 sum_{k>=2} eta_k, so that ekin + epot + echain is the
conserved quantity at every slot.

With the barostat (`barostat` = dict(pressure, taup, beta, mask, cells, rc); `force_fn(x, cells)` then also
returns the virials): between the opening half-update and the first half-kick, mu from the velocities as they
stand (`md_npt_reference.scale_factors`), x and the cells scaled, the list rule that knows strain."""
import numpy as np

from tests import md_npt_reference as npt
from tests import md_reference


def chain_masses(g, kT0, tau, M):
    Q = np.full(M, kT0 * tau * tau)
    Q[0] *= g
    return Q


def half_update(eta, veta, K, g, kT0, Q, delta, loops):
    """One half-update of one frame's chain, eta and veta [M] in place; returns s (K becomes K s^2)."""
    M = len(eta)
    d = delta / loops
    s = 1.0

    def G(k):
        if k == 0:
            return (2.0 * K * s * s - g * kT0) / Q[0]
        return (Q[k - 1] * veta[k - 1] ** 2 - kT0) / Q[k]

    for _ in range(loops):
        veta[M - 1] += 0.5 * d * G(M - 1)
        for k in range(M - 2, -1, -1):
            a = np.exp(-0.25 * d * veta[k + 1])
            veta[k] = (veta[k] * a + 0.5 * d * G(k)) * a
        s *= np.exp(-d * veta[0])
        eta += d * veta
        for k in range(M - 1):
            a = np.exp(-0.25 * d * veta[k + 1])
            veta[k] = (veta[k] * a + 0.5 * d * G(k)) * a
        veta[M - 1] += 0.5 * d * G(M - 1)
    return s


def chain_energy(eta, veta, g, kT0, Q):
    return float((0.5 * Q * veta ** 2).sum() + g * kT0 * eta[0] + kT0 * eta[1:].sum())


def run(force_fn, x0, v0, masses, dt, n_steps, kT0, tau, chain=3, loops=1, dof_removed=0, natoms=None, skin=None,
        record_every=1, eta0=None, veta0=None, barostat=None):
    """`force_fn(x) -> (epot [F], forces [N, 3])`; with `barostat`: `force_fn(x, cells) -> (epot, forces, virial)`.
    `natoms`: atoms per frame (default: one frame). `skin`: None = no list bookkeeping. `eta0`, `veta0` [F, chain]:
    the chains at entry (default: at rest).
    Returns dict(x, v, eta, veta [F, chain], epot, ekin, echain [n_steps // record_every + 1, F], n_rebuilds,
    rebuild_steps); with the barostat also cells, volume, press, end_rebuild."""
    x = np.array(x0, dtype=np.float64).reshape(-1, 3)
    v = np.array(v0, dtype=np.float64).reshape(-1, 3)
    m = np.asarray(masses, dtype=np.float64).ravel()
    natoms = [len(x)] if natoms is None else list(natoms)
    F, M = len(natoms), int(chain)
    frame = np.repeat(np.arange(F), natoms)
    g = [3 * n - dof_removed for n in natoms]
    assert min(g) >= 1
    Q = [chain_masses(g[f], kT0, tau, M) for f in range(F)]
    eta = np.zeros((F, M)) if eta0 is None else np.array(eta0, dtype=np.float64).reshape(F, M)
    veta = np.zeros((F, M)) if veta0 is None else np.array(veta0, dtype=np.float64).reshape(F, M)
    baro = barostat is not None
    if baro:
        h = np.array(barostat["cells"], dtype=np.float64).reshape(F, 3, 3)
        ref_cells, sc = h.copy(), np.ones((F, 3))
        rc = barostat.get("rc")

    def evaluate():
        if baro:
            e, f, W = force_fn(x, h)
            return np.array(e, dtype=np.float64).reshape(-1), f, np.asarray(W, dtype=np.float64).reshape(F, 3, 3)
        e, f = force_fn(x)
        return np.array(e, dtype=np.float64).reshape(-1), f, None

    def thermostat(ke):
        """A half-update of every frame from its kinetic energy: the factors [F]."""
        return np.array([half_update(eta[f], veta[f], ke[f], g[f], kT0, Q[f], 0.5 * dt, loops) for f in range(F)])

    ref = x.copy()
    rebuild_steps = []
    epot, ekin, echain, vol, press = [], [], [], [], []
    e, f, W = evaluate()
    for k in range(n_steps + 1):
        if k > 0:   # the closing half-update of step k
            s1 = thermostat(md_reference.kinetic_energies(m, v, natoms))
            v = v * s1[frame][:, None]
        S = npt.frame_sums(m, v, natoms)
        ke = md_reference.kinetic_energies(m, v, natoms)
        if k % record_every == 0:
            epot.append(e.copy())
            ekin.append(0.5 * S.sum(axis=1) if baro else ke)
            echain.append(np.array([chain_energy(eta[j], veta[j], g[j], kT0, Q[j]) for j in range(F)]))
            if baro:
                V = npt.volumes(h)
                vol.append(V)
                press.append((S - np.diagonal(W, axis1=1, axis2=2)) / V[:, None])
        if k == n_steps:
            break
        s2 = thermostat(ke)
        v = v * s2[frame][:, None]
        if baro:
            mu = npt.scale_factors(npt.frame_sums(m, v, natoms), W, npt.volumes(h), dt, barostat["pressure"],
                                   barostat["taup"], barostat["beta"], barostat.get("mask"))
            x = x * mu[frame]
            h = h * mu[:, None, :]
            sc = sc * mu
        v = v + 0.5 * dt * f / m[:, None]
        x = x + dt * v
        if skin is not None:
            if baro:
                lim = 0.5 * (skin - (rc + skin) * np.sqrt(((sc - 1.0) ** 2).sum(axis=1)))
                u2 = ((x - ref * sc[frame]) ** 2).sum(axis=1)
                stale = np.any(lim <= 0.0) or np.any(u2 >= (lim * lim)[frame])
            else:
                d2 = ((x - ref) ** 2).sum(axis=1)
                stale = skin == 0.0 or not np.all(d2 <= 0.25 * skin * skin)
            if stale:
                ref = x.copy()
                rebuild_steps.append(k + 1)
                if baro:
                    ref_cells, sc = h.copy(), np.ones((F, 3))
        e, f, W = evaluate()
        v = v + 0.5 * dt * f / m[:, None]
    out = dict(x=x, v=v, eta=eta, veta=veta, epot=np.array(epot), ekin=np.array(ekin), echain=np.array(echain),
               n_rebuilds=len(rebuild_steps), rebuild_steps=rebuild_steps)
    if baro:
        out.update(cells=h, volume=np.array(vol), press=np.array(press),
                   end_rebuild=bool(skin is not None and not np.array_equal(h, ref_cells)))
    return out
