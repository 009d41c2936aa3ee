"""NumPy reference of the Langevin step of the device MD loop (`ta_md_set_langevin`, `ta_md_run`): the
counter-based noise (Philox4x32-10, Salmon et al. SC'11, then Box-Muller) and the second-order scheme of
ASE's `Langevin` without its centre-of-mass correction, with the rebuild bookkeeping of
`tests/md_reference.py`. Test infrastructure only.

Noise of (seed, step, atom i, component c): key (seed & 0xffffffff, seed >> 32), counter
(i, c, step & 0xffffffff, step >> 32); from the output words w0 .. w3

    u1 = ((w0 >> 5) 2^26 + (w1 >> 6) + 0.5) 2^-53,  u2 likewise from w2, w3
    xi = sqrt(-2 ln u1) cos(2 pi u2),  eta = sqrt(-2 ln u1) sin(2 pi u2)

Step, with sigma_i = sqrt(2 kT0 fr / m_i):

    c1 = dt/2 - dt^2 fr/8            c2 = dt fr/2 - dt^2 fr^2/8
    c3_i = sqrt(dt) sigma_i/2 - dt^1.5 fr sigma_i/8
    c5_i = dt^1.5 sigma_i/(2 sqrt 3) c4_i = fr/2 c5_i
    rv = c3 xi - c4 eta;  rp = c5 eta
    v += c1 F(x)/m - c2 v + rv;   x += dt v + rp;   v += c1 F(x_new)/m - c2 v + rv
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """`counter` [..., 4] of 32-bit words, `key` = (k0, k1) -> output words [..., 4] (uint32)."""
    c = [np.asarray(counter)[..., j].astype(np.uint64) & MASK for j in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]     # 32 x 32 -> 64 bits, exact in uint64
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def _uniform(hi, lo):
    return ((hi >> 5).astype(np.float64) * 67108864.0 + (lo >> 6).astype(np.float64) + 0.5) * 2.0 ** -53


def normals(seed, step, n_atoms, first_atom=0):
    """(xi, eta) [n_atoms, 3] of absolute step `step` for atoms first_atom .. first_atom + n_atoms - 1."""
    seed, step = int(seed), int(step)
    assert 0 <= seed < 2 ** 64 and 0 <= step < 2 ** 63
    counter = np.empty((n_atoms, 3, 4), dtype=np.uint64)
    counter[..., 0] = np.arange(first_atom, first_atom + n_atoms, dtype=np.uint64)[:, None]
    counter[..., 1] = np.arange(3, dtype=np.uint64)[None, :]
    counter[..., 2] = step & 0xFFFFFFFF
    counter[..., 3] = step >> 32
    w = philox4x32_10(counter, (seed & 0xFFFFFFFF, seed >> 32))
    u1, u2 = _uniform(w[..., 0], w[..., 1]), _uniform(w[..., 2], w[..., 3])
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)


def kinetic_energies(masses, v, natoms):
    e = 0.5 * masses * (v * v).sum(axis=1)
    out, a = np.zeros(len(natoms)), 0
    for f, n in enumerate(natoms):
        out[f] = e[a:a + n].sum()
        a += n
    return out


def run(force_fn, x0, v0, masses, dt, n_steps, kT0, friction, seed, natoms=None, skin=None, record_every=1,
        first_step=0):
    """`force_fn(x) -> (epot [n_frames], forces [N, 3])`; arguments and the returned dict as
    `md_reference.run` (x, v, epot, ekin [n_steps // record_every + 1, n_frames], n_rebuilds, rebuild_steps),
    the records being those of the state after each step. `first_step`: absolute index of the first step."""
    x = np.array(x0, dtype=np.float64).reshape(-1, 3)
    v = np.array(v0, dtype=np.float64).reshape(-1, 3)
    m = np.asarray(masses, dtype=np.float64).ravel()
    natoms = [len(x)] if natoms is None else list(natoms)
    fr = float(friction)
    sigma = np.sqrt(2.0 * kT0 * fr / m)[:, None]
    c1 = dt / 2.0 - dt * dt * fr / 8.0
    c2 = dt * fr / 2.0 - dt * dt * fr * fr / 8.0
    c3 = np.sqrt(dt) * sigma / 2.0 - dt ** 1.5 * fr * sigma / 8.0
    c5 = dt ** 1.5 * sigma / (2.0 * np.sqrt(3.0))
    c4 = fr / 2.0 * c5
    ref = x.copy()
    rebuild_steps = []
    epot, ekin = [], []
    e, f = force_fn(x)
    for k in range(n_steps + 1):
        if k % record_every == 0:
            epot.append(np.array(e, dtype=np.float64).reshape(-1).copy())
            ekin.append(kinetic_energies(m, v, natoms))
        if k == n_steps:
            break
        if fr > 0.0:
            xi, eta = normals(seed, first_step + k, len(x))
            rv, rp = c3 * xi - c4 * eta, c5 * eta
        else:
            rv = rp = 0.0
        v = v + (c1 * f / m[:, None] - c2 * v + rv)
        x = x + dt * v + rp
        if skin is not None:
            d2 = ((x - ref) ** 2).sum(axis=1)
            if skin == 0.0 or not np.all(d2 <= 0.25 * skin * skin):
                ref = x.copy()
                rebuild_steps.append(k + 1)
        e, f = force_fn(x)
        v = v + (c1 * f / m[:, None] - c2 * v + rv)
    return dict(x=x, v=v, epot=np.array(epot), ekin=np.array(ekin), n_rebuilds=len(rebuild_steps),
                rebuild_steps=rebuild_steps)
