"""
The whole layout of the GPU neighbour list (tensoralloy_amd/csrc/ta_nlist.hip and the list code of
ta_api.hip) against the oracle, through `Engine.list_layout`: pair_start / pair_stop, seg_start, the
reverse index, key order, the run packing, and the exact list the skin filter compacts in place. The
checker is tests/list_reference.py (integer equality only); tests/test_list_reference_cpu.py shows that
it rejects every single mutation a subtly wrong kernel could produce.

Every case names its builder and asserts it (`info.builder`), so that no case passes on another path
than the one it is about. "Away from the cutoff" cases assert the oracle's margin | |D| - rc | / rc
above 1e-6 as a condition on the input; case J puts the cutoff on a shell on purpose.
Each case prints one line: case, builder, atoms, pairs, nnl_max, margin.
"""
import numpy as np
import pytest

from tests import list_reference as lr
from tests.helpers import RawCellAtoms, fcc, make_eam, make_grap_nn, make_nn
from tensoralloy_amd import Atoms

pytestmark = pytest.mark.gpu

EL8 = ["Al", "Co", "Cr", "Cu", "Fe", "Mo", "Ni", "Ti"]  # sorted: index = element of the model
BUILDER_ENV = {"one_pass": None, "two_pass": "TA_NL_TWO_PASS", "host": "TA_HOST_NL"}
ALL = ("one_pass", "two_pass", "host")


# ---- plumbing -----------------------------------------------------------------------------------------

def _frames(atoms_list, positions=None):
    out, a = [], 0
    for at in atoms_list:
        pos = at.positions if positions is None else positions[a:a + len(at)]
        out.append((np.array(pos), np.asarray(at.get_cell(complete=True)), np.asarray(at.pbc, bool)))
        a += len(at)
    return out


def _species(nn, atoms_list):
    return np.concatenate([nn.transformer.species_indices(a) for a in atoms_list]).astype(np.int64)


_REF = {}


def _reference(key, frames, rc):
    """(rows, margin) of the oracle at rc, once per geometry. The margin needs the pairs on both sides of rc,
    so the oracle runs at 1.02 rc as well; its rows cut back to d < rc must be the oracle's own list at rc."""
    if key not in _REF:
        wide = lr.oracle_pairs(frames, 1.02 * rc)
        d = lr.pair_lengths(frames, wide) if len(wide) else np.zeros(0)
        margin = float(min(np.min(np.abs(d - rc)) / rc, 0.02)) if len(wide) else 0.02
        assert margin > 1e-6, f"{key}: a pair at {margin:.1e} of the cutoff (a condition on the input)"
        rows = wide[d < rc]
        assert np.array_equal(rows, lr.oracle_pairs(frames, rc)), f"{key}: the cut-back rows are not the oracle's list"
        _REF[key] = (rows, margin)
    return _REF[key]


def _select(monkeypatch, builder):
    for var in ("TA_NL_TWO_PASS", "TA_HOST_NL"):
        monkeypatch.delenv(var, raising=False)
    if BUILDER_ENV[builder]:
        monkeypatch.setenv(BUILDER_ENV[builder], "1")


def _same_views(a, b):
    assert a["info"] == b["info"]
    for k in ("pair_start", "pair_stop", "seg_start", "pair_i", "pair_j", "pair_shift", "pair_rev"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["blk_center"] is None) == (b["blk_center"] is None)
    if a["blk_center"] is not None:
        assert np.array_equal(a["blk_center"], b["blk_center"])


def _build_check(eng, nn, atoms_list, rc, builder, name, *, key=None, packing=None, band=None, expected=None,
                 margin=None):
    """set_frames, then the resident layout against the oracle; the kernel view must be the same list."""
    frames = _frames(atoms_list)
    if expected is None:
        expected, margin = _reference(key or name, frames, rc)
    info = eng.set_frames(atoms_list)
    L = eng.list_layout("resident")
    assert L["info"]["builder"] == builder, (name, L["info"]["builder"])
    assert bool(info.nl_on_device) == (builder != "host")
    assert not L["info"]["filtered"] and not L["info"]["rev_indirect"]
    got = lr.check_layout(L, frames, _species(nn, atoms_list), rc, key_order=builder == "one_pass", packing=packing,
                          counts=dict(n_pairs=int(info.n_pairs), nnl_max=int(info.nnl_max),
                                      n_triples=int(info.n_triples)), expected=expected, band=band)
    assert L["seg_close"] == L["pair_start"][-1]
    _same_views(L, eng.list_layout("kernel"))
    print(f"LIST {name}: builder={builder} atoms={L['info']['atoms']} pairs={got['n_pairs']} "
          f"nnl_max={got['nnl_max']} margin={margin:.1e}" + (f" extra={got['extra']} missing={got['missing']}"
                                                             if band is not None else ""))
    return L, got


def _run_builders(monkeypatch, nn, atoms_list, rc, name, builders=ALL, **kw):
    from tensoralloy_amd import Engine
    out = {}
    for b in builders:
        _select(monkeypatch, b)
        with Engine(nn) as eng:
            out[b] = _build_check(eng, nn, atoms_list, rc, b, name, **kw)
    rows = {b: np.concatenate([L["pair_i"][:, None], L["pair_j"][:, None], L["pair_shift"]], axis=1)
            for b, (L, _) in out.items()}
    return out, rows


def _bins(cell, pbc, rc):
    """Bins per axis of nl_make_grid for periodic axes (perpendicular width / rc, at most 64)."""
    vol = abs(np.linalg.det(cell))
    nb = []
    for a in range(3):
        height = vol / np.linalg.norm(np.cross(cell[(a + 1) % 3], cell[(a + 2) % 3]))
        nb.append(max(1, min(int(np.floor(height / rc)), 64)) if pbc[a] else None)
    return nb


# ---- geometries ---------------------------------------------------------------------------------------

CELL_A = np.array([[9.1, 0.0, 0.0], [1.3, 8.7, 0.0], [-0.9, 1.1, 10.2]])


def case_a(elements=EL8, seed=3):
    """37 atoms, triclinic, pbc (T, T, F), atoms up to two cells outside; of 8 elements: 7 present, 3 absent,
    6 with a single atom."""
    rng = np.random.RandomState(seed)
    pos = (rng.rand(37, 3) * 3.0 - 1.0) @ CELL_A
    sp = rng.choice([0, 1, 2, 4, 5, 7], size=37)
    sp[:6] = [0, 1, 2, 4, 5, 7]
    sp[20] = 6
    return Atoms(symbols=[elements[s % len(elements)] for s in sp], positions=pos, cell=CELL_A, pbc=[True, True, False])


CELL_B = np.array([[60.0, 0.0, 0.0], [6.0, 60.0, 0.0], [3.0, -4.0, 60.0]])


def case_b(n=700, clumps=0, seed=11, elements=("Mo", "Ni")):
    rng = np.random.RandomState(seed)
    if clumps:
        centres = rng.rand(clumps, 3) @ CELL_B
        pos = (centres[:, None, :] + rng.normal(0.0, 1.6, (clumps, 20, 3))).reshape(-1, 3)
    else:
        pos = rng.rand(n, 3) @ CELL_B
    return Atoms(symbols=[elements[k % len(elements)] for k in range(len(pos))], positions=pos, cell=CELL_B, pbc=True)


def case_c(seed=15):
    rng = np.random.RandomState(seed)
    centres = rng.rand(30, 3) * 300.0
    pos = (centres[:, None, :] + rng.normal(0.0, 1.6, (30, 20, 3))).reshape(-1, 3)
    return Atoms(symbols=["Mo" if k % 3 == 0 else "Ni" for k in range(len(pos))], positions=pos,
                 cell=np.eye(3) * 300.0, pbc=True)


def case_e(seed=13):
    """Cubic cell of 12.5 A, rc 4: three bins per axis. Per axis, atoms whose fractional coordinate is 0,
    -1e-17 (wraps to exactly 1.0), 1 - 2^-53, 1/3 and 2/3 (the bin boundaries) as floating point gives them,
    the same 3 cells out and -3 cells out, and one atom with all three coordinates on a seam; 70 more at
    random."""
    L = 12.5
    rng = np.random.RandomState(seed)
    seams = [0.0, -1e-17, 1.0 - 2.0 ** -53, 1.0 / 3.0, 2.0 / 3.0]
    frac = []
    for axis in range(3):
        for f in seams:
            for shift in (0.0, 3.0, -3.0):
                p = rng.rand(3)
                p[axis] = f + shift
                frac.append(p)
    frac.append(np.array([0.0, -1e-17, 1.0 / 3.0]))
    frac.append(np.array([2.0 / 3.0, 1.0 - 2.0 ** -53, 2.0 / 3.0]))
    frac = np.concatenate([np.array(frac), rng.rand(70, 3)])
    return Atoms(symbols=["Mo" if k % 2 else "Ni" for k in range(len(frac))], positions=frac * L, cell=np.eye(3) * L,
                 pbc=True)


def case_f(n, seed=14):
    """n points in a ball of diameter 0.999 rc (rc 10.5): every atom has exactly n - 1 neighbours."""
    rng = np.random.RandomState(seed)
    pts = np.zeros((0, 3))
    while len(pts) < n:
        p = rng.rand(4 * n, 3) * 2.0 - 1.0
        pts = np.concatenate([pts, p[np.sum(p * p, axis=1) < 1.0]])
    return Atoms(symbols=["Ni"] * n, positions=30.0 + pts[:n] * (0.4995 * 10.5), cell=np.eye(3) * 60.0, pbc=False)


# ---- builders -----------------------------------------------------------------------------------------

def test_a_eight_elements_triclinic(lib, monkeypatch):
    """Element indices 4 to 7: the top bits of nl_key, lanes 4 to 8 of the segment scan."""
    nn = make_nn(EL8, 6.0, False, [8])
    atoms = [case_a()]
    sp = _species(nn, atoms)
    assert 7 in sp and 3 not in sp and (sp == 6).sum() == 1
    out, rows = _run_builders(monkeypatch, nn, atoms, 6.0, "A")
    assert np.abs(out["one_pass"][0]["pair_shift"]).max() >= 2  # the shifts carry the wrap


@pytest.mark.parametrize("clumps", [0, 40])
def test_b_more_than_2048_bins(lib, monkeypatch, clumps):
    """place_recs_kernel<false> behind a scan launch (one-pass), and the two-pass / host builders on the same."""
    nn = make_nn(["Mo", "Ni"], 4.5, False, [8])
    atoms = [case_b(clumps=clumps)]
    assert np.prod(_bins(CELL_B, [1, 1, 1], 4.5)) == 13 ** 3 > 2048
    out, _ = _run_builders(monkeypatch, nn, atoms, 4.5, f"B{clumps}")
    L = out["one_pass"][0]
    if not clumps:
        assert ((L["pair_stop"] - L["pair_start"][:-1]) == 0).sum() > 50  # centres without a neighbour


def test_c_bins_capped_at_64_per_axis(lib, monkeypatch):
    nn = make_nn(["Mo", "Ni"], 4.5, False, [8])
    atoms = [case_c()]
    assert 300.0 / 4.5 > 64 and _bins(np.eye(3) * 300.0, [1, 1, 1], 4.5) == [64, 64, 64]
    _run_builders(monkeypatch, nn, atoms, 4.5, "C")


@pytest.mark.parametrize("rep", [(1, 1, 1), (1, 2, 2)])
def test_d_small_cells(lib, monkeypatch, rep):
    """Self-images and several images of one neighbour in a segment: the reverse of (i, i, S) is (i, i, -S)."""
    nn = make_nn(["Ni"], 6.5, False, [8])
    atoms = [fcc(rep=rep)]
    out, _ = _run_builders(monkeypatch, nn, atoms, 6.5, f"D{rep[1]}")
    L = out["one_pass"][0]
    own = L["pair_i"] == L["pair_j"]
    assert own.any()
    assert np.array_equal(L["pair_shift"][L["pair_rev"][own]], -L["pair_shift"][own])


def test_e_seam_coordinates(lib, monkeypatch):
    nn = make_nn(["Mo", "Ni"], 4.0, False, [8])
    atoms = [case_e()]
    assert _bins(np.eye(3) * 12.5, [1, 1, 1], 4.0) == [3, 3, 3]
    f = atoms[0].positions * (1.0 / 12.5)  # as the kernel forms it: position times the inverse cell
    assert ((f - np.floor(f)) == 1.0).any(), "no coordinate wraps to exactly 1.0"
    out, _ = _run_builders(monkeypatch, nn, atoms, 4.0, "E")
    L = out["one_pass"][0]
    assert ((L["pair_stop"] - L["pair_start"][:-1]) > 0).all()  # every centre has neighbours


def test_f_384_against_385_neighbours(lib, monkeypatch):
    """The one-pass builder keeps 384 neighbours per centre in LDS: 384 must stay with it, 385 must go to
    the two-pass builder by itself (no environment switch), with the oracle's set both times."""
    from tensoralloy_amd import Engine
    nn = make_nn(["Ni"], 10.5, False, [8])
    _select(monkeypatch, "one_pass")
    for n, builder in ((385, "one_pass"), (386, "two_pass")):
        atoms = [case_f(n)]
        with Engine(nn) as eng:
            L, got = _build_check(eng, nn, atoms, 10.5, builder, f"F{n}")
        assert got["nnl_max"] == n - 1 and got["n_pairs"] == n * (n - 1)


def test_g_late_reverse_index(lib, monkeypatch):
    """The list fits the arrays (grown by the first frame) but exceeds the stretch the reverse index was
    launched over (previous count of the same atoms + 25 % + 4096): nl_reverse_sorted runs afterwards."""
    from tensoralloy_amd import Engine
    nn = make_nn(["Mo", "Ni"], 6.0, False, [8])
    _select(monkeypatch, "one_pass")

    def lattice(a, rep, seed):
        base = fcc(a=a, rep=rep, jitter=0.02, seed=seed)
        return Atoms(symbols=["Mo" if k % 4 == 0 else "Ni" for k in range(len(base))], positions=base.positions,
                     cell=base.get_cell(complete=True), pbc=True)
    with Engine(nn) as eng:
        _, big = _build_check(eng, nn, [lattice(3.524, (5, 5, 5), 1)], 6.0, "one_pass", "G1")
        _, wide = _build_check(eng, nn, [lattice(4.6, (4, 4, 4), 2)], 6.0, "one_pass", "G2")
        # the condition for the late branch, from the oracle's counts
        ref, _ = _reference("G3", _frames([lattice(3.524, (4, 4, 4), 2)]), 6.0)
        assert wide["n_pairs"] + wide["n_pairs"] // 4 + 4096 < len(ref) <= big["n_pairs"]
        _build_check(eng, nn, [lattice(3.524, (4, 4, 4), 2)], 6.0, "one_pass", "G3")


def test_h_reused_zero_block(lib, monkeypatch):
    """The zero block (statistics, look-back words, bin histogram) is cleared by the kernels themselves while
    atoms and bins stay the same, and by a memset when either changes."""
    from tensoralloy_amd import Engine
    nn = make_nn(["Mo", "Ni"], 4.5, False, [8])
    _select(monkeypatch, "one_pass")
    rng = np.random.RandomState(21)

    def frame(L, frac):
        return Atoms(symbols=["Mo" if k % 2 else "Ni" for k in range(len(frac))], positions=frac * L,
                     cell=np.eye(3) * L, pbc=True)
    f1, f2 = rng.rand(150, 3), rng.rand(150, 3)
    assert _bins(np.eye(3) * 20.0, [1, 1, 1], 4.5) != _bins(np.eye(3) * 24.0, [1, 1, 1], 4.5)
    with Engine(nn) as eng:
        for name, atoms in (("H1", frame(20.0, f1)), ("H1", frame(20.0, f1)), ("H1", frame(20.0, f1)),
                            ("H2", frame(24.0, f1)), ("H3", frame(24.0, f2))):
            _build_check(eng, nn, [atoms], 4.5, "one_pass", name)


def _batch_thin_thick_slab():
    thin = fcc(rep=(1, 1, 2), seed=4)
    thick = fcc(rep=(3, 3, 3), seed=5)
    rng = np.random.RandomState(6)
    cell = np.array([[3.1, 0.0, 0.0], [1.2, 9.0, 0.0], [0.4, -0.8, 16.0]])
    slab = Atoms(symbols=["Ni"] * 30, positions=(rng.rand(30, 3) * 3.0 - 1.0) @ cell, cell=cell,
                 pbc=[True, True, False])
    return [thin, thick, slab]


def test_i_uneven_batch_on_the_device(lib, monkeypatch):
    nn = make_nn(["Ni"], 6.5, False, [8])
    _run_builders(monkeypatch, nn, _batch_thin_thick_slab(), 6.5, "I")


def test_i_incomplete_cell_takes_the_host_builder(lib, monkeypatch):
    """A frame whose cell has zero rows (a molecule without a box, pbc off) cannot be binned: the whole batch
    is built on the host, for the reason the host builder exists, and must pass the same checks."""
    from tensoralloy_amd import Engine
    nn = make_nn(["Ni"], 6.5, False, [8])
    rng = np.random.RandomState(8)
    molecule = RawCellAtoms(symbols=["Ni"] * 9, positions=rng.rand(9, 3) * 7.0, cell=np.zeros((3, 3)), pbc=False)
    assert not np.asarray(molecule.get_cell(complete=True)).any()
    atoms = _batch_thin_thick_slab() + [molecule]
    _select(monkeypatch, "one_pass")  # nothing asks for the host builder but the cell
    with Engine(nn) as eng:
        _build_check(eng, nn, atoms, 6.5, "host", "I+molecule")
        assert eng.info.nl_on_device == 0


# ---- J: the cutoff exactly on a shell ---------------------------------------------------------------------

A_J = 3.52
RC_J = A_J * np.sqrt(3.0)
BAND = 1e-12


def _case_j(symbols=("Ni",)):
    base = fcc(a=A_J, rep=(4, 4, 4), jitter=0.0)
    return Atoms(symbols=[symbols[k % len(symbols)] for k in range(len(base))], positions=base.positions,
                 cell=base.get_cell(complete=True), pbc=True)


def _reference_j(frames):
    """The oracle's list at rc, and the condition: the band holds exactly the 2048 pairs of the <111> a shell,
    every other pair is more than 6 % away."""
    if "J" not in _REF:
        wide = lr.oracle_pairs(frames, 1.07 * RC_J)
        off = np.abs(lr.pair_lengths(frames, wide) - RC_J) / RC_J
        assert (off <= BAND).sum() == 2048
        assert off[off > BAND].min() > 0.06
        ref = lr.oracle_pairs(frames, RC_J)
        inband = int((np.abs(lr.pair_lengths(frames, ref) - RC_J) / RC_J <= BAND).sum())
        _REF["J"] = (ref, inband)
    return _REF["J"]


def _in_band(frames, L):
    slots = np.concatenate([np.arange(a, b) for a, b in zip(L["pair_start"][:-1], L["pair_stop"])])
    rows = np.concatenate([L["pair_i"][slots, None], L["pair_j"][slots, None], L["pair_shift"][slots]], axis=1)
    return int((np.abs(lr.pair_lengths(frames, rows) - RC_J) / RC_J <= BAND).sum())


def test_j_cutoff_on_a_shell_builders(lib, monkeypatch):
    """Both device builders must keep exactly the same pairs (the claim next to `valid` in
    build_pairs_kernel), every builder's list must be symmetric, and all agree with the oracle outside the
    band of 1e-12 rc around the cutoff (coordinate rounding is 1e-15: a thousandfold margin)."""
    nn = make_nn(["Ni"], RC_J, False, [8])
    atoms = [_case_j()]
    frames = _frames(atoms)
    ref, oracle_inband = _reference_j(frames)
    out, rows = _run_builders(monkeypatch, nn, atoms, RC_J, "J", expected=ref, margin=0.0, band=BAND)
    kept = {b: _in_band(frames, L) for b, (L, _) in out.items()}
    print(f"LIST J in-band pairs kept: oracle={oracle_inband} " + " ".join(f"{b}={n}" for b, n in kept.items()))
    srt = lambda a: a[np.lexsort(a.T[::-1])]
    assert np.array_equal(srt(rows["one_pass"]), srt(rows["two_pass"])), "the device builders keep different pairs"


@pytest.mark.parametrize("model", ["angular", "eam"])
def test_j_cutoff_on_a_shell_filter(lib, model):
    """The exact list under a skin with the cutoff on a shell: "a pair and its reverse have the same length,
    so both are inside rmax or neither is" (filter_rev_kernel). Checked on the layout before anything
    evaluates on it: a missing reverse pair is an assertion here, not a kernel reading slot -1."""
    from tensoralloy_amd import Engine
    nn = make_nn(["Ni"], RC_J, True, [8]) if model == "angular" else make_eam(["Cu", "Ni"], rcut=RC_J)
    atoms = [_case_j(("Ni",) if model == "angular" else ("Cu", "Ni"))]
    frames, sp = _frames(atoms), _species(nn, atoms)
    ref, oracle_inband = _reference_j(frames)
    ref_list, margin = _reference("J+skin", frames, RC_J + 0.5)
    with Engine(nn) as eng:
        eng.set_skin(0.5)
        info = eng.set_frames(atoms)
        R, K = eng.list_layout("resident"), eng.list_layout("kernel")
        assert R["info"]["builder"] == "one_pass" and K["info"]["filtered"]
        assert K["info"]["rev_indirect"] == (model == "angular")
        lr.check_layout(R, frames, sp, RC_J + 0.5, key_order=True, packing="resident" if model == "angular" else None,
                        counts=dict(n_pairs=int(info.n_pairs), nnl_max=int(info.nnl_max), n_triples=int(info.n_triples)),
                        expected=ref_list)
        got = lr.check_layout(K, frames, sp, RC_J, packing="filtered" if model == "angular" else None, resident=R,
                              expected=ref, band=BAND)
        print(f"LIST J+skin/{model}: builder=one_pass atoms={len(sp)} pairs={got['n_pairs']} nnl_max={got['nnl_max']} "
              f"margin(list)={margin:.1e} in-band kept: oracle={oracle_inband} kernel={_in_band(frames, K)}")


# ---- the skin filter -----------------------------------------------------------------------------------

RC_F, SKIN = 6.0, 0.5


def _near_faces(frac, cell, pbc, k=4):
    """Put the first k atoms 0.05 A inside the lower face of a periodic axis (they cross it in step 3)."""
    axes = [a for a in range(3) if pbc[a]]
    for n in range(min(k, len(frac))):
        a = axes[n % len(axes)]
        frac[n, a] = 0.05 / np.linalg.norm(cell[a])
    return frac


def _filter_frames(name):
    rng = np.random.RandomState({"A": 31, "A5": 31, "n16": 32, "n17": 33, "n1": 34, "B300": 35, "two": 36}[name])

    def make(n, cell, pbc, scale=1.0, lo=0.0):
        cell = np.asarray(cell, float)
        frac = _near_faces(rng.rand(n, 3) * scale - lo, cell, pbc)
        return dict(sp=rng.randint(0, 3, size=n), pos=frac @ cell, cell=cell, pbc=pbc)
    small = np.array([[7.0, 0.0, 0.0], [0.8, 7.5, 0.0], [-0.5, 0.6, 8.0]])
    if name in ("A", "A5"):
        f = make(37, CELL_A, [True, True, False], 3.0, 1.0)
        f["sp"][:3] = [0, 1, 2]
        if name == "A5":  # five elements, one of them with a single atom
            f["sp"] = np.array([0, 1, 2, 4])[(f["sp"] + 2 * (np.arange(37) % 2)) % 4]
            f["sp"][20] = 3
        return [f]
    if name == "n16":
        return [make(16, small, [True] * 3)]
    if name == "n17":
        return [make(17, small, [True] * 3)]
    if name == "n1":
        return [dict(sp=np.array([1]), pos=np.array([[0.02, 1.0, 2.0]]), cell=np.eye(3) * 3.5, pbc=[True] * 3)]
    if name == "B300":
        return [make(300, CELL_B, [True] * 3)]
    return [make(23, small, [True] * 3), make(40, np.diag([9.5, 12.0, 8.2]), [True, False, True])]


def _atoms_of(frames, elements, positions=None):
    out, a = [], 0
    for f in frames:
        n = len(f["sp"])
        pos = f["pos"] if positions is None else positions[a:a + n]
        out.append(Atoms(symbols=[elements[s % len(elements)] for s in f["sp"]], positions=pos, cell=f["cell"], pbc=f["pbc"]))
        a += n
    return out


def _displacements(frames, name):
    """Norms below 0.49 skin; the atoms next to a face move 0.15 A through it."""
    rng = np.random.RandomState(77)
    out = []
    for f in frames:
        n = len(f["sp"])
        d = rng.normal(size=(n, 3))
        d *= (rng.uniform(0.1, 0.48 * SKIN, n) / np.linalg.norm(d, axis=1))[:, None]
        axes = [a for a in range(3) if f["pbc"][a]]
        for k in range(min(4, n)):
            a = axes[k % len(axes)]
            d[k] = -0.15 * f["cell"][a] / np.linalg.norm(f["cell"][a])
        out.append(d)
    d = np.concatenate(out)
    assert np.linalg.norm(d, axis=1).max() < 0.49 * SKIN
    return d


MODELS = {
    "sf1": (lambda: make_nn(["Ni"], RC_F, True, [8]), {}, "sf"),
    "sf3": (lambda: make_nn(["Al", "Mo", "Ni"], RC_F, True, [8]), {}, "sf"),
    "sf3_rev_kernel": (lambda: make_nn(["Al", "Mo", "Ni"], RC_F, True, [8]), {"TA_FILTER_REV_KERNEL": "1"}, "sf"),
    "eam": (lambda: make_eam(["Cu", "Ni"], rcut=RC_F), {}, "eam"),
    # five elements, the most any model the filter applies to can have (EAM: 5; second-generation
    # symmetry-function kernels: 5): lanes 5 to 7 of kFilterMaxEl cannot be reached
    "eam5": (lambda: make_eam(["Al", "Co", "Cu", "Fe", "Ni"], rcut=RC_F), {}, "eam"),
    # (the default 2 x 2 angular grid: the only one the second-generation kernels take with 5 elements)
    "sf5": (lambda: make_nn(["Al", "Co", "Cu", "Fe", "Ni"], RC_F, True, [8]), {}, "sf"),
}
FILTER_CASES = [(m, g) for m in ("sf1", "sf3", "sf3_rev_kernel", "eam") for g in ("A", "n16", "n17", "n1", "B300", "two")] + \
    [("eam5", "A5"), ("sf5", "A5")]


@pytest.mark.parametrize("model,geometry", FILTER_CASES)
def test_filter_exact_list(lib, monkeypatch, model, geometry):
    """set_frames under a skin, both views; move every atom by less than half the skin (some through a cell
    face): the list is kept and the exact list follows the oracle at the new positions; move one atom
    further: rebuilt, both views again; only then evaluate, against a fresh engine without a skin."""
    from tensoralloy_amd import Engine
    make, env, kind = MODELS[model]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    nn = make()
    raw = _filter_frames(geometry)
    atoms = _atoms_of(raw, nn.elements)
    sp = _species(nn, atoms)
    pos0 = np.concatenate([f["pos"] for f in raw])
    pack = dict(res="resident", ex="filtered") if kind == "sf" else dict(res=None, ex=None)

    def check_both(eng, pos, tag, resident_too):
        frames = _frames(atoms, pos)
        R, K = eng.list_layout("resident"), eng.list_layout("kernel")
        assert R["info"]["builder"] == "one_pass" and not R["info"]["filtered"]
        assert K["info"]["filtered"] and K["info"]["rev_indirect"] == (kind == "sf" and not env)
        if resident_too:
            ref_r, m_r = _reference(f"filter/{geometry}/{tag}/list", frames, RC_F + SKIN)
            lr.check_layout(R, frames, sp, RC_F + SKIN, key_order=True, packing=pack["res"], expected=ref_r,
                            counts=dict(n_pairs=int(eng.info.n_pairs), nnl_max=int(eng.info.nnl_max),
                                        n_triples=int(eng.info.n_triples)))
        ref_k, m_k = _reference(f"filter/{geometry}/{tag}/exact", frames, RC_F)
        got = lr.check_layout(K, frames, sp, RC_F, packing=pack["ex"], resident=R, expected=ref_k)
        print(f"LIST filter/{model}/{geometry}/{tag}: builder=one_pass atoms={len(sp)} pairs={got['n_pairs']} "
              f"nnl_max={got['nnl_max']} margin={m_k:.1e}")
        if geometry == "B300":
            assert ((K["pair_stop"] - K["pair_start"][:-1]) == 0).sum() > 20, "no centre without a neighbour"
        return ref_k

    with Engine(nn) as eng:
        eng.set_skin(SKIN)
        eng.set_frames(atoms)                                   # 1, 2
        ref0 = check_both(eng, pos0, "built", True)
        pos1 = pos0 + _displacements(raw, geometry)             # 3
        hinv, k = np.linalg.inv(raw[0]["cell"]), min(4, len(raw[0]["sp"]))
        assert (np.floor(pos0[:k] @ hinv) != np.floor(pos1[:k] @ hinv)).any(axis=1).all(), "no atom crosses a cell face"
        assert eng.update_positions(pos1) is False
        ref1 = check_both(eng, pos1, "moved", False)
        if geometry != "n1":  # (one atom and its own images: no distance changes)
            s0, s1 = set(map(tuple, ref0.tolist())), set(map(tuple, ref1.tolist()))
            assert s1 - s0 and s0 - s1, "no pair entered or left the cutoff"
        pos2 = pos1.copy()                                      # 4
        pos2[-1] = pos0[-1] + np.array([0.6 * SKIN, 0.0, 0.0])  # from where the list was built
        assert eng.update_positions(pos2) is True
        check_both(eng, pos2, "rebuilt", True)
        from tensoralloy_amd import _lib
        want = _lib.TA_WANT_ENERGY | _lib.TA_WANT_FORCES
        eng.compute(want)                                       # 5
        res = eng.fetch(want)
    with Engine(nn) as fresh:
        exact = fresh.evaluate(_atoms_of(raw, nn.elements, pos2))
    energy = np.array([r["energy"] for r in exact])
    forces = np.concatenate([r["forces"] for r in exact])
    assert np.abs(np.asarray(res["energy"]) - energy).max() < 1e-9
    assert np.abs(np.asarray(res["forces"]).reshape(-1, 3) - forces).max() < 1e-10


def test_filter_does_not_apply_to_grap(lib):
    """GRAP kernels run on the skin list itself: the kernel view is the resident list."""
    from tensoralloy_amd import Engine
    nn = make_grap_nn(["Mo", "Ni"], RC_F, [8])
    raw = _filter_frames("A")
    atoms = _atoms_of(raw, nn.elements)
    frames, sp = _frames(atoms), _species(nn, atoms)
    ref, margin = _reference("filter/A/built/list", frames, RC_F + SKIN)
    with Engine(nn) as eng:
        eng.set_skin(SKIN)
        info = eng.set_frames(atoms)
        R = eng.list_layout("resident")
        assert R["info"]["builder"] == "one_pass"
        _same_views(R, eng.list_layout("kernel"))
        got = lr.check_layout(R, frames, sp, RC_F + SKIN, key_order=True, expected=ref,
                              counts=dict(n_pairs=int(info.n_pairs), nnl_max=int(info.nnl_max),
                                          n_triples=int(info.n_triples)))
        print(f"LIST filter/grap/A: builder=one_pass atoms={len(sp)} pairs={got['n_pairs']} nnl_max={got['nnl_max']} "
              f"margin={margin:.1e}")
        assert eng.update_positions(np.concatenate([f["pos"] for f in raw]) + _displacements(raw, "A")) is False
        _same_views(eng.list_layout("resident"), eng.list_layout("kernel"))
