"""NumPy restatement of the eam/fs (Finnis-Sinclair) model for the GPU tests (test infrastructure).

A direct sum over the oracle's exact neighbour list (`oracle.neighbors.neighbor_list`) with the
oracle's function evaluators (`oracle.eam.spline_function` for `spline@` functions, `nn_function`
for "nn" ones). For the directed pair p = (i -> j) with D = R_j - R_i + S h, r = |D|,
  rho_i  = sum_j rho_{A B}(r)                 (A = species of i, B = species of j),
  E_i    = F_A(rho_i) + 1/2 sum_j phi_{AB}(r),
  g_p    = dE/dD_p (centre's terms) = (F'_A(rho_i) rho'_{AB}(r) + phi'_{AB}(r) / 2) D / r,
so that F_k = sum_{p: i = k} g_p - sum_{p: j = k} g_p and W = sum_p g_p D^T; the reverse pair
carries F'_B(rho_j) rho'_{BA}(r), hence dE/dr_ij = F'_A rho'_AB + F'_B rho'_BA + phi'_AB.
"""
import numpy as np

from oracle.eam import GPA, nn_function, spline_function
from oracle.neighbors import _complete_cell, neighbor_list


def fs_function(nn, section, fn, x):
    """f(x), f'(x) of one function of an `EamFsNN`."""
    x = np.asarray(x, dtype=np.float64)
    if len(x) == 0:
        return np.zeros(0), np.zeros(0)
    if nn.is_spline(section, fn):
        sp = nn.spline_table(section, fn)
        return spline_function(x, (sp.x, sp.y))
    return nn_function(x, nn.weights[section][fn], nn._activation)


def fs_evaluate(nn, atoms, eps=1e-14):
    els = nn.elements
    R = np.asarray(atoms.positions, dtype=np.float64).reshape(-1, 3)
    N = len(R)
    pbc = np.asarray(atoms.pbc, dtype=bool).reshape(3)
    h = _complete_cell(np.asarray(atoms.get_cell(complete=True)), pbc)
    volume = abs(np.linalg.det(h))
    spec = np.array([els.index(s) for s in atoms.get_chemical_symbols()])
    pi, pj, pS = neighbor_list(R, h, pbc, nn.transformer.rcut)
    D = R[pj] - R[pi] + pS.astype(np.float64) @ h
    r = np.sqrt(np.sum(D * D, axis=1) + eps)
    si, sj = spec[pi], spec[pj]
    rho_p, drho_p = np.zeros(len(pi)), np.zeros(len(pi))
    phi_p, dphi_p = np.zeros(len(pi)), np.zeros(len(pi))
    for a, ea in enumerate(els):
        for b, eb in enumerate(els):
            m = (si == a) & (sj == b)
            rho_p[m], drho_p[m] = fs_function(nn, ea + eb, "rho", r[m])
            phi_p[m], dphi_p[m] = fs_function(nn, "".join(sorted([ea, eb])), "phi", r[m])
    rho = np.zeros(N)
    np.add.at(rho, pi, rho_p)
    phisum = np.zeros(N)
    np.add.at(phisum, pi, phi_p)
    F, dF = np.zeros(N), np.zeros(N)
    for a, ea in enumerate(els):
        m = spec == a
        F[m], dF[m] = fs_function(nn, ea, "embed", rho[m])
    atomic = F + 0.5 * phisum
    g = ((dF[pi] * drho_p + 0.5 * dphi_p) / r)[:, None] * D
    forces = np.zeros((N, 3))
    np.add.at(forces, pi, g)
    np.add.at(forces, pj, -g)
    W = g.T @ D
    stress = W / volume
    return dict(energy=float(atomic.sum()), atomic=atomic, forces=forces, virial=W, rho=rho,
                stress_voigt=np.array([stress[0, 0], stress[1, 1], stress[2, 2], stress[1, 2], stress[0, 2],
                                       stress[0, 1]]),
                total_pressure=float(np.trace(stress) / (-3.0 * GPA)), volume=volume)


# ---- eam/fs files written by the tests ------------------------------------------------------------

def write_fs_setfl(path, elements, nrho, drho, nr, dr, rcut, embed, listed, rphi, comment="tests"):
    """A LAMMPS eam/fs file in its own layout: per element I (file order) a header line, F(rho), then
    N density tables `listed[(I, J)]` for J in file order; then r * phi(r) `rphi[(I, J)]` for the
    (1,1), (2,1), (2,2), ... pairs (I >= J in file order). Values at 17 significant digits."""
    from tensoralloy_amd.atoms import atomic_masses, atomic_numbers

    def block(values):
        return "".join("%.17g\n" % v for v in values)

    out = [f"eam/fs file written by {comment}\n", "\n", "\n", f"{len(elements)} " + " ".join(elements) + "\n",
           f"{nrho} {drho!r} {nr} {dr!r} {rcut!r}\n"]
    for I in elements:
        z = atomic_numbers[I]
        out.append(f"{z} {atomic_masses[z]!r} 0.0 fcc\n")
        out.append(block(embed[I]))
        for J in elements:
            out.append(block(listed[(I, J)]))
    for i, I in enumerate(elements):
        for J in elements[:i + 1]:
            out.append(block(rphi[(I, J)]))
    with open(path, "w") as fp:
        fp.write("".join(out))
    return path


def synthetic_listed_tables(r, rc=5.6):
    """Four distinct density tables of a 2-element Al-Fe file, keyed by their FILE position
    (element block I, position J): smooth polynomials that vanish at rc."""
    c = np.where(r < rc, (rc - r) ** 4, 0.0)
    return {("Al", "Al"): 0.020 * c,
            ("Al", "Fe"): 0.006 * c * (1.0 + 0.5 * r),
            ("Fe", "Al"): 0.030 * c / (1.0 + 0.2 * r * r),
            ("Fe", "Fe"): 0.012 * c * (2.0 - 0.2 * r)}


def write_synthetic_fs(path):
    """A 2-element Al-Fe eam/fs file whose cross densities differ (rho_AlFe != rho_FeAl)."""
    nr, dr, nrho, drho, rcut = 600, 0.01, 500, 0.1, 5.6
    r = np.arange(nr) * dr
    rho = np.arange(nrho) * drho
    embed = {"Al": 0.02 * rho * rho - 0.8 * rho, "Fe": 0.001 * rho ** 3 + 0.01 * rho * rho - 1.1 * rho}
    cut = np.where(r < rcut, (rcut - r) ** 3 / rcut ** 3, 0.0)

    def morse(d, a, r0):
        return d * (np.exp(-2 * a * (r - r0)) - 2 * np.exp(-a * (r - r0))) * cut * r

    rphi = {("Al", "Al"): morse(0.3, 1.4, 2.86), ("Fe", "Al"): morse(0.4, 1.5, 2.6),
            ("Fe", "Fe"): morse(0.5, 1.6, 2.48)}
    return write_fs_setfl(path, ["Al", "Fe"], nrho, drho, nr, dr, rcut, embed, synthetic_listed_tables(r), rphi)


def alloy_as_fs(src, dst):
    """An eam/alloy file rewritten as eam/fs: every element's density table repeated N times (the
    density an I-neighbour contributes is the same at every centre)."""
    from tensoralloy_amd.io import read_eam_alloy_setfl
    fl = read_eam_alloy_setfl(src)
    els = fl.elements
    r = fl.rho[els[0]].x
    listed = {(I, J): fl.rho[I].y for I in els for J in els}
    rphi = {}
    for i, I in enumerate(els):
        for J in els[:i + 1]:
            y = fl.pair("phi", I, J).y
            rphi[(I, J)] = np.concatenate([y[:1], y[1:] * r[1:]])
    return write_fs_setfl(dst, els, fl.nrho, fl.drho, fl.nr, fl.dr, fl.rcut, {el: fl.embed[el].y for el in els},
                          listed, rphi, comment=f"alloy_as_fs({src})")
