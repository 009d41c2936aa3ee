"""NumPy reference of the Martyna-Tobias-Klein barostat of the device MD loop (`ta_md_set_mtk_barostat`,
`ta_md_run`): the scheme of include/tensoralloy_amd.h, with the strain-aware list rule of
tests/md_npt_reference.py applied to count the list rebuilds. Forces come from a callback
`force_fn(x, cells) -> (epot [F], forces [N, 3], virial [F, 3, 3])`, so the same loop serves an oracle, a second
engine or an analytic potential. Test infrastructure only.

Per frame: n atoms, g = 3 n - dof_removed, the particle chain of tests/md_nhc_reference.py (kT0, tau, M, L), the
cell h (rows are lattice vectors), V = |det h|, W_vir the virial (dE / d strain) of the last evaluation,
S_c = sum m v_c^2, K = (S_x + S_y + S_z) / 2, free_c the free axes (mask None: isotropic, all free),
d_b = 1 (isotropic) or sum free_c. State: the strain rates omega_c and a chain (xi_k, vxi_k), k = 1 .. M_p, with

    W_c = (g + 3) kT0 taup^2 / 3,   Q'_1 = d_b kT0 taup^2,   Q'_k = kT0 taup^2 (k >= 2)
    G_c = free_c [S_c - W_vir,cc - P0 V + 2 K / g] / W_c     (isotropic: the mean of the three for every c)
    alpha_c = omega_c + (omega_x + omega_y + omega_z) / g,   K_b = sum_c W_c omega_c^2 / 2

and half(chain, K, dof, tau) = `md_nhc_reference.half_update` over dt / 2. One step:

    1. s = half(particle chain, K, g, tau); v <- s v
    2. s_b = half(barostat chain, K_b, d_b, taup); omega <- s_b omega
    3. omega_c += (dt/2) G_c
    4. v_c <- v_c exp(-(dt/2) alpha_c); v += (dt/2) F/m
    5. x_c <- exp(omega_c dt) x_c + dt exp(omega_c dt/2) v_c; h[:, c] <- exp(omega_c dt) h[:, c]
    6. evaluate
    7. v += (dt/2) F/m; v_c <- v_c exp(-(dt/2) alpha_c)
    8. omega_c += (dt/2) G_c
    9. s_b = half(barostat chain, ...); omega <- s_b omega; s = half(particle chain, ...); v <- s v

Records (slot 0 the state at entry, slot r > 0 the state after step 9 of its step): epot, ekin = K, echain (the
particle chain's terms), ebaro = P0 V + K_b + sum_k Q'_k vxi_k^2 / 2 + d_b kT0 xi_1 + kT0 sum_{k>=2} xi_k, volume
and press = (S - diag W_vir) / V; ekin + epot + echain + ebaro is the conserved quantity at every slot.

List bookkeeping (`skin` not None) as in `md_npt_reference.run` with s the product of the exp(omega_c dt) since the
list was built; `log` and `end_rebuild` likewise, so `md_npt_reference.assert_not_marginal` reads the log."""
import numpy as np

from tests import md_nhc_reference as nhc
from tests import md_npt_reference as npt


def barostat_masses(g, kT0, taup, M_p, d_b):
    """(W_c, Q' [M_p]) of a frame with g degrees of freedom."""
    Q = np.full(M_p, kT0 * taup * taup)
    Q[0] *= d_b
    return (g + 3.0) * kT0 * taup * taup / 3.0, Q


def driving_force(S, Wvir, V, g, Wc, pressure, free, iso):
    """G [3] of one frame from its kinetic sums S [3], virial [3, 3] and volume."""
    K = 0.5 * (S[0] + S[1] + S[2])
    G = free * (S - np.diagonal(Wvir) - pressure * V + 2.0 * K / g) / Wc
    if iso:
        G = np.full(3, (G[0] + G[1] + G[2]) / 3.0)
    return G


def barostat_energy(omega, xi, vxi, V, pressure, Wc, Q, d_b, kT0):
    return float(pressure * V + 0.5 * Wc * (omega ** 2).sum() + (0.5 * Q * vxi ** 2).sum() + d_b * kT0 * xi[0] +
                 kT0 * xi[1:].sum())


def run(force_fn, x0, v0, masses, cells0, dt, n_steps, kT0, tau, pressure, taup, chain=3, loops=1, pchain=3, ploops=1,
        dof_removed=0, mask=None, natoms=None, skin=None, rc=None, record_every=1, eta0=None, veta0=None, omega0=None,
        xi0=None, vxi0=None):
    """`mask`: None = isotropic, else three flags (x, y, z). `eta0`, `veta0` [F, chain], `omega0` [F, 3], `xi0`,
    `vxi0` [F, pchain]: the extended state at entry (default: at rest).
    Returns dict(x, v, cells, eta, veta, omega, xi, vxi, epot, ekin, echain, ebaro, volume [n_rec, F],
    press [n_rec, F, 3], n_rebuilds, rebuild_steps, end_rebuild, log)."""
    x = np.array(x0, dtype=np.float64).reshape(-1, 3)
    v = np.array(v0, dtype=np.float64).reshape(-1, 3)
    m = np.asarray(masses, dtype=np.float64).ravel()
    h = np.array(cells0, dtype=np.float64).reshape(-1, 3, 3)
    natoms = [len(x)] if natoms is None else list(natoms)
    F, M, Mp = len(natoms), int(chain), int(pchain)
    assert len(h) == F
    frame = np.repeat(np.arange(F), natoms)
    g = [3 * n - dof_removed for n in natoms]
    assert min(g) >= 1
    iso = mask is None
    free = np.ones(3) if iso else np.asarray(mask, dtype=bool).astype(np.float64)
    d_b = 1.0 if iso else float(free.sum())
    assert d_b >= 1.0
    Q = [nhc.chain_masses(g[f], kT0, tau, M) for f in range(F)]
    Wc, Qp = zip(*[barostat_masses(g[f], kT0, taup, Mp, d_b) for f in range(F)])

    def state(a, shape):
        return np.zeros(shape) if a is None else np.array(a, dtype=np.float64).reshape(shape)
    eta, veta = state(eta0, (F, M)), state(veta0, (F, M))
    omega, xi, vxi = state(omega0, (F, 3)), state(xi0, (F, Mp)), state(vxi0, (F, Mp))

    def evaluate():
        e, f, W = force_fn(x, h)
        return np.array(e, dtype=np.float64).reshape(-1), f, np.asarray(W, dtype=np.float64).reshape(F, 3, 3)

    def particle_half(S):
        """Step 1 / the second part of step 9: the factors [F]."""
        return np.array([nhc.half_update(eta[f], veta[f], 0.5 * S[f].sum(), g[f], kT0, Q[f], 0.5 * dt, loops)
                         for f in range(F)])

    def barostat_half():
        """Step 2 / the first part of step 9, omega in place."""
        for f in range(F):
            Kb = 0.5 * Wc[f] * (omega[f] ** 2).sum()
            omega[f] *= nhc.half_update(xi[f], vxi[f], Kb, d_b, kT0, Qp[f], 0.5 * dt, ploops)

    def kick_omega(S, W):
        """Steps 3 and 8."""
        V = npt.volumes(h)
        for f in range(F):
            omega[f] += 0.5 * dt * driving_force(S[f], W[f], V[f], g[f], Wc[f], pressure, free, iso)

    def alpha():
        return omega + omega.sum(axis=1)[:, None] / np.array(g, dtype=np.float64)[:, None]

    ref, ref_cells, sc = x.copy(), h.copy(), np.ones((F, 3))
    rebuild_steps, log = [], []
    epot, ekin, echain, ebaro, vol, press = [], [], [], [], [], []
    e, f, W = evaluate()
    for k in range(n_steps + 1):
        S = npt.frame_sums(m, v, natoms)
        V = npt.volumes(h)
        if k % record_every == 0:
            epot.append(e.copy())
            ekin.append(0.5 * S.sum(axis=1))
            echain.append(np.array([nhc.chain_energy(eta[j], veta[j], g[j], kT0, Q[j]) for j in range(F)]))
            ebaro.append(np.array([barostat_energy(omega[j], xi[j], vxi[j], V[j], pressure, Wc[j], Qp[j], d_b, kT0)
                                   for j in range(F)]))
            vol.append(V)
            press.append((S - np.diagonal(W, axis1=1, axis2=2)) / V[:, None])
        if k == n_steps:
            break
        s = particle_half(S)                                   # 1
        v = v * s[frame][:, None]
        barostat_half()                                        # 2
        kick_omega(npt.frame_sums(m, v, natoms), W)            # 3
        a = alpha()
        v = v * np.exp(-0.5 * dt * a)[frame]                   # 4
        v = v + 0.5 * dt * f / m[:, None]
        e1, e2 = np.exp(omega * dt), np.exp(omega * (0.5 * dt))
        x = e1[frame] * x + dt * e2[frame] * v                 # 5
        h = h * e1[:, None, :]
        sc = sc * e1
        if skin is not None:
            lim = 0.5 * (skin - (rc + skin) * np.sqrt(((sc - 1.0) ** 2).sum(axis=1)))
            u2 = ((x - ref * sc[frame]) ** 2).sum(axis=1)
            d2 = ((x - ref) ** 2).sum(axis=1)
            umax, dmax, a0 = np.zeros(F), np.zeros(F), 0
            for j, n in enumerate(natoms):
                if n:
                    umax[j], dmax[j] = np.sqrt(u2[a0:a0 + n].max()), np.sqrt(d2[a0:a0 + n].max())
                a0 += n
            log.append(dict(step=k + 1, lim=lim, umax=umax, dmax=dmax))
            if not np.all(lim > 0.0) or not np.all(u2 < (lim * lim)[frame]):
                ref, ref_cells, sc = x.copy(), h.copy(), np.ones((F, 3))
                rebuild_steps.append(k + 1)
        e, f, W = evaluate()                                   # 6
        v = v + 0.5 * dt * f / m[:, None]                      # 7
        v = v * np.exp(-0.5 * dt * a)[frame]
        S = npt.frame_sums(m, v, natoms)
        kick_omega(S, W)                                       # 8
        barostat_half()                                        # 9
        s = particle_half(S)
        v = v * s[frame][:, None]
    return dict(x=x, v=v, cells=h, eta=eta, veta=veta, omega=omega, xi=xi, vxi=vxi, epot=np.array(epot),
                ekin=np.array(ekin), echain=np.array(echain), ebaro=np.array(ebaro), volume=np.array(vol),
                press=np.array(press), n_rebuilds=len(rebuild_steps), rebuild_steps=rebuild_steps,
                end_rebuild=bool(skin is not None and not np.array_equal(h, ref_cells)), log=log)


def conserved(out):
    """H' [n_rec, F] of a run's records."""
    return out["ekin"] + out["epot"] + out["echain"] + out["ebaro"]
