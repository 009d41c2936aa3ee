"""
The layout checker of tests/list_reference.py on layouts made in numpy from the oracle: it accepts a
correct resident list (key order, greedy packing) and a correct exact list (groups compacted in place,
16 run slots per group), and rejects each single mutation a subtly wrong kernel could produce. This is
what makes a pass of tests/test_gpu_nlist_layout.py mean something. No GPU, no library.
"""
import copy

import numpy as np
import pytest

from tests import list_reference as lr

RC_LIST, RC = 5.0, 4.5
CAP = 192


@pytest.fixture(scope="module")
def case():
    """Two elements, 40 atoms (a partial last group of 8), a triclinic periodic cell 4.7 A thick along x: self-images and
    several images of one neighbour in a segment; atoms given up to two cells outside."""
    rng = np.random.RandomState(7)
    cell = np.array([[4.7, 0.0, 0.0], [1.1, 6.8, 0.0], [-0.6, 0.9, 7.3]])
    pos = (rng.rand(40, 3) * 3.0 - 1.0) @ cell
    species = (np.arange(40) % 3 == 0).astype(np.int64)
    frames = [(pos, cell, np.array([True, True, True]))]
    res = lr.reference_layout(frames, species, 2, RC_LIST, CAP)
    keep = lr.pair_lengths(frames, np.concatenate([res["pair_i"][:, None], res["pair_j"][:, None],
                                                   res["pair_shift"]], axis=1)) < RC
    assert np.array_equal(keep, keep[res["pair_rev"]])
    ex = lr.reference_filtered(res, keep, species, CAP)
    return frames, species, res, ex


def _check_res(case, res):
    frames, species, _, _ = case
    return lr.check_layout(res, frames, species, RC_LIST, key_order=True, packing="resident")


def _check_ex(case, ex):
    frames, species, res, _ = case
    return lr.check_layout(ex, frames, species, RC, packing="filtered", resident=res)


def _swap(L, a, b):
    """Exchange the contents of slots a and b and keep the reverse index consistent."""
    for k in ("pair_j", "pair_shift", "pair_rev"):
        L[k][[a, b]] = L[k][[b, a]]
    L["pair_rev"][L["pair_rev"][a]] = a
    L["pair_rev"][L["pair_rev"][b]] = b


def _foreign(L, q):
    return L["pair_j"][q] != L["pair_i"][q]


def test_correct_layouts_pass(case):
    frames, species, res, ex = case
    got = _check_res(case, res)
    assert got["n_pairs"] == res["info"]["n_slots"] > 0 and res["info"]["n_blk"] > 3
    assert (res["pair_i"] == res["pair_j"]).any()  # self-images are in
    got_ex = _check_ex(case, ex)
    assert 0 < got_ex["n_pairs"] < got["n_pairs"]
    # the exact list really leaves slots unused and empty run slots behind
    assert (ex["pair_stop"][15] < ex["pair_start"][16]) and (np.diff(ex["blk_center"]) == 0).any()
    # the counts a library would report are compared as well
    lr.check_layout(res, frames, species, RC_LIST, key_order=True, packing="resident",
                    counts=dict(n_pairs=got["n_pairs"], nnl_max=got["nnl_max"], n_triples=got["n_triples"]))
    with pytest.raises(AssertionError, match="nnl_max"):
        lr.check_layout(res, frames, species, RC_LIST, counts=dict(n_pairs=got["n_pairs"], nnl_max=got["nnl_max"] + 1,
                                                                   n_triples=got["n_triples"]))


def _boundary_slot(L):
    """Last slot of segment 0 of a centre whose segments 0 and 1 both hold foreign neighbours."""
    seg = L["seg_start"]
    for i in range(len(seg)):
        q = seg[i, 1] - 1
        if seg[i, 0] <= q and q + 1 < seg[i, 2] and _foreign(L, q) and _foreign(L, q + 1):
            return int(q)
    raise AssertionError("no such centre")


@pytest.mark.parametrize("which", ["resident", "filtered"])
def test_swap_across_a_segment_boundary(case, which):
    L = copy.deepcopy(case[2] if which == "resident" else case[3])
    q = _boundary_slot(L)
    _swap(L, q, q + 1)
    with pytest.raises(AssertionError, match="segment of another element"):
        (_check_res if which == "resident" else _check_ex)(case, L)


@pytest.mark.parametrize("which", ["resident", "filtered"])
def test_rev_at_another_image_of_the_same_neighbour(case, which):
    L = copy.deepcopy(case[2] if which == "resident" else case[3])
    own = np.concatenate([np.arange(a, b) for a, b in zip(L["pair_start"][:-1], L["pair_stop"])])
    for q in own[:-1]:
        if q + 1 in own and L["pair_i"][q] == L["pair_i"][q + 1] and L["pair_j"][q] == L["pair_j"][q + 1] \
                and _foreign(L, q):
            break
    else:
        raise AssertionError("no neighbour with two images")
    L["pair_rev"][q] = L["pair_rev"][q + 1]
    with pytest.raises(AssertionError, match="another image"):
        (_check_res if which == "resident" else _check_ex)(case, L)


@pytest.mark.parametrize("which", ["resident", "filtered"])
def test_rev_of_minus_one(case, which):
    L = copy.deepcopy(case[2] if which == "resident" else case[3])
    L["pair_rev"][L["pair_start"][17] + 2] = -1
    with pytest.raises(AssertionError, match="-1"):
        (_check_res if which == "resident" else _check_ex)(case, L)


@pytest.mark.parametrize("which", ["resident", "filtered"])
def test_one_pair_dropped(case, which):
    L = copy.deepcopy(case[2] if which == "resident" else case[3])
    L["pair_stop"][-1] -= 1
    L["seg_start"][-1, -1] -= 1
    if which == "resident":
        L["pair_start"][-1] -= 1
    with pytest.raises(AssertionError, match="missing"):
        (_check_res if which == "resident" else _check_ex)(case, L)


@pytest.mark.parametrize("which", ["resident", "filtered"])
def test_one_pair_duplicated(case, which):
    L = copy.deepcopy(case[2] if which == "resident" else case[3])
    q = int(L["seg_start"][5, 0])
    assert q + 1 < L["seg_start"][5, 1]
    L["pair_j"][q + 1], L["pair_shift"][q + 1] = L["pair_j"][q], L["pair_shift"][q]
    with pytest.raises(AssertionError, match="appears twice"):
        (_check_res if which == "resident" else _check_ex)(case, L)


def test_run_crossing_a_group(case):
    L = copy.deepcopy(case[3])
    assert L["blk_center"][16] == 16
    L["blk_center"][16] = 17  # the last run slot of group 0 now ends inside group 1
    with pytest.raises(AssertionError, match="crosses a group"):
        _check_ex(case, L)


@pytest.mark.parametrize("which", ["resident", "filtered"])
def test_run_over_cap(case, which):
    L = copy.deepcopy(case[2] if which == "resident" else case[3])
    if which == "resident":  # two runs merged
        L["blk_center"] = np.delete(L["blk_center"], 1)
        L["info"] = dict(L["info"], n_blk=L["info"]["n_blk"] - 1)
    else:                    # the second run of group 0 emptied into the first
        L["blk_center"][1] = L["blk_center"][2]
    with pytest.raises(AssertionError, match="more than cap"):
        (_check_res if which == "resident" else _check_ex)(case, L)


def test_key_order_inversion(case):
    L = copy.deepcopy(case[2])
    seg = L["seg_start"]
    q = next(int(seg[i, 1]) for i in range(40) if seg[i, 2] - seg[i, 1] >= 2 and _foreign(L, seg[i, 1])
             and _foreign(L, seg[i, 1] + 1))
    _swap(L, q, q + 1)
    with pytest.raises(AssertionError, match="not increasing"):
        _check_res(case, L)
    lr.check_layout(L, case[0], case[1], RC_LIST, packing="resident")  # still a valid list without the key order
