"""CPU: the NumPy reference of the cell relaxation (tests/relax_cell_reference.py) against itself: its
generalised forces are minus the gradient of E + p V in the generalised coordinates, and its list rule keeps
every pair that was outside rc + skin at the build outside rc."""
import numpy as np

from tests import relax_cell_reference as rc


def _quadratic(k=1.3, c=0.7, seed=5, n=7):
    """E = 1/2 sum_i k |x_i - s_i h|^2 + 1/2 c |h - h*|^2 with its forces and its virial
    W_ab = sum_i dE/dx_ia x_ib + sum_r dE/dh_ra h_rb (the derivative with respect to a strain of everything)."""
    rng = np.random.RandomState(seed)
    s = rng.rand(n, 3)
    h_star = np.diag([5.0, 6.0, 7.0]) + 0.3 * rng.randn(3, 3)

    def energy(x, h):
        r = x - s @ h
        return 0.5 * k * (r * r).sum() + 0.5 * c * ((h - h_star) ** 2).sum()

    def force_fn(x, cells):
        h = cells[0]
        r = x - s @ h
        dEdh = -k * s.T @ r + c * (h - h_star)
        W = k * r.T @ x + dEdh.T @ h
        return np.array([energy(x, h)]), -k * r, W[None]
    return energy, force_fn, rng


def test_generalized_force_is_minus_the_gradient():
    """Central differences (step 1e-5) of E + p |det h| in (q, cf G) at a sheared, rotated G against
    `generalized_forces`, p = 0.37, cf = 3.5, on a quadratic energy with a virial that is not symmetric. The
    energy is quadratic and p V cubic in the coordinates, so the difference quotient is exact up to
    p V O(step^2) and rounding of order eps E / step ~ 1e-9. Measured gap: 5.7e-9 (largest component; the
    atom rows are of order 8, the cell rows of order 50); the bound is 10 x that."""
    energy, force_fn, rng = _quadratic()
    n, p, cf, d = 7, 0.37, 3.5, 1e-5
    h0 = np.diag([5.2, 5.9, 7.3]) + 0.2 * rng.randn(3, 3)
    G = np.eye(3) + 0.05 * rng.randn(3, 3)
    q = rng.rand(n, 3) @ h0 + 0.1 * rng.randn(n, 3)

    def total(q_, G_):
        h = h0 @ G_.T
        return energy(q_ @ G_.T, h) + p * abs(np.linalg.det(h))

    x, h = q @ G.T, h0 @ G.T
    _, F, W = force_fn(x, h[None])
    f, fc = rc.generalized_forces(F, W[0], G, h, cf, p, rc.voigt_mask(None), False)
    num_f, num_c = np.zeros_like(q), np.zeros((3, 3))
    for i in range(n):
        for a in range(3):
            e = np.zeros_like(q)
            e[i, a] = d
            num_f[i, a] = -(total(q + e, G) - total(q - e, G)) / (2 * d)
    for a in range(3):
        for b in range(3):
            e = np.zeros((3, 3))
            e[a, b] = d / cf        # a step d of the coordinate cf G_ab
            num_c[a, b] = -(total(q, G + e) - total(q, G - e)) / (2 * d)
    gap = max(np.abs(f - num_f).max(), np.abs(fc - num_c).max())
    print("gap", gap, "scale", np.abs(f).max(), np.abs(fc).max())
    assert np.abs(W[0] - W[0].T).max() > 0.1      # the index convention is under test
    assert gap < 5.7e-8
    # the mask and the hydrostatic projection act on the cell rows alone
    m = rc.voigt_mask([1, 1, 0, 0, 0, 1])
    assert np.array_equal(m, m.T) and m[2].sum() == 0 and m[:, 2].sum() == 0 and m[0, 1] == 1
    _, fm = rc.generalized_forces(F, W[0], G, h, cf, p, m, False)
    assert np.array_equal(fm, fc * m)
    _, fh = rc.generalized_forces(F, W[0], G, h, cf, p, rc.voigt_mask(None), True)
    assert np.allclose(fh, np.eye(3) * np.trace(fc) / 3.0, rtol=0, atol=1e-15 * np.abs(fc).max())


def test_reference_descends_to_the_minimum():
    """The loop on the quadratic energy: it converges, E + p V went down, and at the end the cell rows of the
    generalised force are below fmax."""
    energy, force_fn, rng = _quadratic()
    h0 = np.diag([5.2, 5.9, 7.3])
    x0 = rng.rand(7, 3) @ h0
    st = rc.new_state(x0, [h0], pressure=0.01)
    out = rc.run(force_fn, st, 2000, 1e-4, skin=0.5, rc=3.0)
    assert out["converged"].all() and out["cell_fmax"][0] < 1e-4 and out["fmax"][0] < 1e-4
    start = energy(x0, h0) + 0.01 * abs(np.linalg.det(h0))
    end = out["energy"][0] + 0.01 * abs(np.linalg.det(out["cells"][0]))
    assert end < start - 1.0
    assert np.abs(out["cells"][0] - h0 @ out["G"][0].T).max() < 1e-13
    assert out["n_rebuilds"] >= 1 and out["rebuild_steps"] == sorted(set(out["rebuild_steps"]))


def test_list_rule_keeps_outside_pairs_outside():
    """Pairs just outside rc + skin at the build, strained by a random A and displaced by u at the edge of the
    bound 2 max |u_i| + (rc + skin) |A - I|_F < skin: the rule calls the list valid and no pair is inside rc.
    The worst case (compression along the pair, both atoms moving towards each other) ends exactly at rc."""
    rng = np.random.RandomState(11)
    rcut, skin = 6.0, 0.5
    worst = np.inf
    for trial in range(400):
        d = rng.randn(3)
        d /= np.linalg.norm(d)
        D = d * (rcut + skin) * (1.0 + 1e-9 + (1e-3 * rng.rand() if trial % 2 else 0.0))
        t = rng.rand() * skin / (rcut + skin) * 0.999          # |A - I|_F
        if trial % 4 < 2:
            E = -np.outer(d, d)                                # the compression along the pair
        else:
            E = rng.randn(3, 3)
        A = np.eye(3) + t * E / np.sqrt((E * E).sum())
        lim = 0.5 * (skin - (rcut + skin) * t)
        assert lim > 0.0
        xi = rng.randn(3) * 3.0
        ref = np.array([xi, xi + D])
        if trial % 4 < 2:
            u = np.array([d, -d]) * lim * (1.0 - 1e-12)       # towards each other, at the edge
        else:
            u = rng.randn(2, 3)
            u *= lim * (1.0 - 1e-12) / np.linalg.norm(u, axis=1)[:, None]
        x = ref @ A + u
        # (the cells only enter through A = h_ref^-1 h)
        h_ref = np.diag([9.0, 10.0, 11.0]) + 0.1 * rng.randn(3, 3)
        stale, (lim_out, umax, _) = rc.list_is_stale(x, ref, h_ref @ A, h_ref, skin, rcut)
        assert not stale and abs(lim_out - lim) < 1e-12 and umax < lim
        r_new = np.linalg.norm(x[1] - x[0])
        worst = min(worst, r_new - rcut)
        assert r_new >= rcut - 1e-12, (trial, r_new)
        # one more hair of displacement and the rule fires
        stale, _ = rc.list_is_stale(ref @ A + u * (1.0 + 1e-9), ref, h_ref @ A, h_ref, skin, rcut)
        assert stale
    print("smallest r_new - rc", worst)
    assert worst < 1e-6      # the edge was reached
    # A = I: the skin / 2 rule; skin = 0: always stale
    ref = rng.randn(5, 3)
    h = np.eye(3) * 8.0
    assert not rc.list_is_stale(ref + np.array([0.2499, 0, 0]), ref, h, h, 0.5, 6.0)[0]
    assert rc.list_is_stale(ref + np.array([0.25, 0, 0]), ref, h, h, 0.5, 6.0)[0]
    assert rc.list_is_stale(ref, ref, h, h, 0.0, 6.0)[0]
