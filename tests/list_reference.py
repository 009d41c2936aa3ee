"""
Layout checker for the neighbour list as the kernels read it (`Engine.list_layout`): numpy and the
oracle's list only, nothing from the library. Every check is integer equality.

A layout is a dict: `info` (atoms, elements, n_slots, n_blk, cap, builder, filtered, rev_indirect) and
the arrays pair_start [N + 1], pair_stop [N], seg_start [N, nel + 1], pair_i, pair_j, pair_shift
[n_slots, 3], pair_rev [n_slots], blk_center [n_blk + 1] or None. Centre i owns the slots
[pair_start[i], pair_stop[i]); no other slot is ever read here.

Frames are (positions [n, 3], cell [3, 3], pbc [3]) tuples; atoms of a batch are numbered through.
"""
import numpy as np

from oracle import neighbors as onl

GROUP = 16  # centres per builder / filter workgroup, and the most centres one run may hold


def _sorted_rows(a):
    a = np.asarray(a, np.int64).reshape(-1, 5)
    return a[np.lexsort(a.T[::-1])] if len(a) else a


def oracle_pairs(frames, rc):
    """Directed pairs (i, j, Sx, Sy, Sz) of a batch from the oracle, sorted; S relative to the positions as given."""
    out, off = [], 0
    for pos, cell, pbc in frames:
        i, j, S = onl.neighbor_list(pos, cell, pbc, rc)
        out.append(np.concatenate([(i + off)[:, None], (j + off)[:, None], np.asarray(S).reshape(-1, 3)], axis=1))
        off += len(pos)
    return _sorted_rows(np.concatenate(out) if out else np.zeros((0, 5)))


def pair_lengths(frames, rows):
    """|R_j - R_i + S.h| of (i, j, S) rows, in the operation order of the oracle."""
    rows = np.asarray(rows, np.int64).reshape(-1, 5)
    R = np.concatenate([np.asarray(p, np.float64).reshape(-1, 3) for p, _, _ in frames])
    foa = np.concatenate([np.full(len(p), f) for f, (p, _, _) in enumerate(frames)])
    H = np.stack([onl._complete_cell(c, b) for _, c, b in frames])
    D = R[rows[:, 1]] - R[rows[:, 0]] + np.einsum("pa,pab->pb", rows[:, 2:].astype(np.float64), H[foa[rows[:, 0]]])
    return np.sqrt(np.sum(D * D, axis=1))


def greedy_runs(counts, cap):
    """The run packing of the resident list: whole centres in order, a new run when the next centre would
    exceed `cap` pairs or be the 17th."""
    blk, load, nc = [0], 0, 0
    for i, c in enumerate(counts):
        if load + c > cap or nc >= GROUP:
            blk.append(i)
            load, nc = 0, 0
        load += int(c)
        nc += 1
    blk.append(len(counts))
    return np.asarray(blk, np.int64)


def _owned(start, stop):
    cnt = stop - start
    assert (cnt >= 0).all(), "a centre's stop lies before its start"
    first = np.cumsum(cnt) - cnt
    slots = np.repeat(start, cnt) + (np.arange(int(cnt.sum())) - np.repeat(first, cnt))
    return slots, np.repeat(np.arange(len(cnt)), cnt), cnt


def check_layout(layout, frames, species, rc, *, key_order=False, packing=None, resident=None, counts=None,
                 expected=None, band=None):
    """Assert that `layout` is a correct list of the batch at cutoff `rc`.

    key_order: inside every segment (j, Sx, Sy, Sz) strictly increases (one-pass builder).
    packing:   None, "resident" (greedy runs) or "filtered" (16 run slots per group of 16 centres).
    resident:  the resident layout this exact list was extracted from (needed when info.filtered).
    counts:    dict(n_pairs, nnl_max, n_triples) the library reported for this list.
    expected:  the oracle's rows when the caller has them already.
    band:      relative half-width around rc inside which a pair may be kept or dropped; pairs that
               differ from the oracle's must lie in it (None: the sets are equal).
    Returns dict(n_pairs, nnl_max, n_triples, extra, missing) of the layout."""
    info = layout["info"]
    species = np.asarray(species, np.int64)
    N, nel, P = len(species), info["elements"], info["n_slots"]
    assert info["atoms"] == N
    start = np.asarray(layout["pair_start"], np.int64)
    stop = np.asarray(layout["pair_stop"], np.int64)
    seg = np.asarray(layout["seg_start"], np.int64).reshape(N, nel + 1)
    pi, pj = np.asarray(layout["pair_i"], np.int64), np.asarray(layout["pair_j"], np.int64)
    ps = np.asarray(layout["pair_shift"], np.int64).reshape(-1, 3)
    rev = np.asarray(layout["pair_rev"], np.int64)
    assert len(start) == N + 1 and len(stop) == N
    assert (start[:N] >= 0).all() and (stop <= P).all(), "a centre's range leaves the pair arrays"
    slots, centre, cnt = _owned(start[:N], stop)
    assert len(np.unique(slots)) == len(slots), "a slot belongs to two centres"

    # -- starts
    if info["filtered"]:
        assert resident is not None
        rstart = np.asarray(resident["pair_start"], np.int64)
        first = np.arange(0, N, GROUP)
        assert np.array_equal(start[first], rstart[first]), "a group does not start at its offset in the resident list"
        inner = np.arange(N - 1)[(np.arange(N - 1) + 1) % GROUP != 0]
        assert np.array_equal(start[inner + 1], stop[inner]), "centres of a group are not contiguous"
        last = np.minimum(first + GROUP, N) - 1
        assert (stop[last] <= rstart[np.minimum(first + GROUP, N)]).all(), "a group runs into the next one"
        assert start[N] == rstart[N]
    else:
        assert start[0] == 0, "pair_start[0] != 0"
        assert np.array_equal(stop, start[1:]), "pair_stop[i] != pair_start[i + 1]"
    if counts is not None and not info["filtered"]:
        assert start[N] == counts["n_pairs"], "pair_start[N] != n_pairs"

    # -- set of pairs
    assert np.array_equal(pi[slots], centre), "pair_i[q] != the centre that owns q"
    j = pj[slots]
    assert ((j >= 0) & (j < N)).all(), "pair_j out of range"
    rows = np.concatenate([centre[:, None], j[:, None], ps[slots]], axis=1)
    srt = _sorted_rows(rows)
    assert len(srt) < 2 or (np.diff(srt, axis=0) != 0).any(axis=1).all(), "a pair appears twice"
    ref = oracle_pairs(frames, rc) if expected is None else _sorted_rows(expected)
    as_set = lambda a: set(map(tuple, a.tolist()))
    dev_set, ref_set = as_set(srt), as_set(ref)
    extra = np.array(sorted(dev_set - ref_set), np.int64).reshape(-1, 5)
    missing = np.array(sorted(ref_set - dev_set), np.int64).reshape(-1, 5)
    if band is None:
        assert not len(missing), f"{len(missing)} pairs of the oracle are missing, first {missing[:1].tolist()}"
        assert not len(extra), f"{len(extra)} pairs are not in the oracle's list, first {extra[:1].tolist()}"
    else:
        for name, diff in (("missing", missing), ("extra", extra)):
            if len(diff):
                off = np.abs(pair_lengths(frames, diff) - rc) / rc
                assert (off <= band).all(), f"{name} pair outside the band: {diff[np.argmax(off)].tolist()} at {off.max():.3e}"

    # -- segments
    assert np.array_equal(seg[:, 0], start[:N]), "seg[i][0] != pair_start[i]"
    assert np.array_equal(seg[:, nel], stop), "seg[i][nel] != pair_stop[i]"
    assert (np.diff(seg, axis=1) >= 0).all(), "seg_start decreases inside a centre"
    sj = species[j]
    assert ((seg[centre, sj] <= slots) & (slots < seg[centre, sj + 1])).all(), \
        "a slot lies in the segment of another element than its neighbour's"

    # -- reverse index
    r = rev[slots]
    assert (r >= 0).all(), "pair_rev of -1"
    assert ((r >= start[j]) & (r < stop[j])).all(), "pair_rev outside the neighbour's range"
    assert np.array_equal(pi[r], j) and np.array_equal(pj[r], centre), "pair_rev is not a pair j -> i"
    assert np.array_equal(ps[r], -ps[slots]), "pair_rev points at another image"
    assert np.array_equal(rev[r], slots), "pair_rev is not an involution"

    # -- key order
    if key_order and len(slots) > 1:
        key = np.concatenate([centre[:, None], sj[:, None], j[:, None], ps[slots]], axis=1)
        d = np.diff(key, axis=0)
        nz = d != 0
        assert nz.any(axis=1).all(), "equal keys"
        lead = d[np.arange(len(d)), np.argmax(nz, axis=1)]
        assert (lead > 0).all(), "keys are not increasing inside a segment"

    # -- run packing
    blk, cap = layout["blk_center"], info["cap"]
    if packing is None:
        pass
    else:
        assert blk is not None and info["n_blk"] > 0, "no run packing"
        blk = np.asarray(blk, np.int64)
        assert len(blk) == info["n_blk"] + 1
        assert blk[0] == 0 and blk[-1] == N and (np.diff(blk) >= 0).all(), "runs do not cover 0 .. N in order"
        csum = np.concatenate([[0], np.cumsum(cnt)])
        ncen, load = np.diff(blk), csum[blk[1:]] - csum[blk[:-1]]
        assert (ncen <= GROUP).all(), "a run holds more than 16 centres"
        assert ((load <= cap) | (ncen == 1)).all(), "a run of several centres holds more than cap pairs"
        if packing == "resident":
            assert (ncen >= 1).all(), "an empty run in the resident packing"
            assert np.array_equal(blk, greedy_runs(cnt, cap)), "the packing is not the greedy one"
        else:
            assert packing == "filtered"
            n_groups = (N + GROUP - 1) // GROUP
            assert info["n_blk"] == GROUP * n_groups, "not 16 run slots per group"
            g = np.arange(GROUP * n_groups) // GROUP
            assert (blk[1:] <= np.minimum(GROUP * (g + 1), N)).all(), "a run crosses a group"
            assert np.array_equal(blk[0:GROUP * n_groups:GROUP], GROUP * np.arange(n_groups)), \
                "a group's first run slot does not start at the group's first centre"

    # -- counts
    tri = int((cnt * (cnt - 1) // 2).sum())
    got = dict(n_pairs=int(cnt.sum()), nnl_max=int(cnt.max()) if N else 0, n_triples=tri,
               extra=len(extra), missing=len(missing))
    if counts is not None:
        if band is None:  # the layout's counts are the oracle's by the equality of the sets; say so directly
            oc = np.bincount(ref[:, 0], minlength=N) if len(ref) else np.zeros(N, np.int64)
            assert counts["nnl_max"] == (int(oc.max()) if N else 0), "nnl_max"
            assert counts["n_triples"] == int((oc * (oc - 1) // 2).sum()), "n_triples"
        else:
            assert counts["nnl_max"] == got["nnl_max"] and counts["n_triples"] == got["n_triples"], "counts"
    return got


# ---- a correct layout made from the oracle (what the CPU test mutates) ---------------------------------

def reference_layout(frames, species, nel, rc, cap):
    """Resident layout in key order with the greedy packing, from the oracle's pairs."""
    species = np.asarray(species, np.int64)
    N = len(species)
    rows = oracle_pairs(frames, rc)
    order = np.lexsort((rows[:, 4], rows[:, 3], rows[:, 2], rows[:, 1], species[rows[:, 1]], rows[:, 0]))
    rows = rows[order]
    P = len(rows)
    cnt = np.bincount(rows[:, 0], minlength=N)
    start = np.concatenate([[0], np.cumsum(cnt)])
    seg = np.zeros((N, nel + 1), np.int64)
    per = np.zeros((N, nel), np.int64)
    np.add.at(per, (rows[:, 0], species[rows[:, 1]]), 1)
    seg[:, 0] = start[:N]
    seg[:, 1:] = start[:N, None] + np.cumsum(per, axis=1)
    where = {tuple(r): q for q, r in enumerate(rows.tolist())}
    rev = np.array([where[(r[1], r[0], -r[2], -r[3], -r[4])] for r in rows.tolist()], np.int64)
    blk = greedy_runs(cnt, cap)
    info = dict(atoms=N, elements=nel, n_slots=P, n_blk=len(blk) - 1, cap=cap, builder="one_pass", filtered=False,
                rev_indirect=False)
    return dict(info=info, pair_start=start, pair_stop=start[1:].copy(), seg_start=seg, pair_i=rows[:, 0].copy(),
                pair_j=rows[:, 1].copy(), pair_shift=rows[:, 2:].copy(), pair_rev=rev, blk_center=blk)


def reference_filtered(res, keep, species, cap):
    """The exact list of `res` restricted to the slots in `keep` (a symmetric mask): every group of 16 centres
    compacted in place at its own offset, 16 run slots per group."""
    species = np.asarray(species, np.int64)
    N, nel, P = res["info"]["atoms"], res["info"]["elements"], res["info"]["n_slots"]
    start, stop = np.zeros(N + 1, np.int64), np.zeros(N, np.int64)
    seg = np.zeros((N, nel + 1), np.int64)
    pi, pj, ps = np.full(P, -7, np.int64), np.full(P, -7, np.int64), np.full((P, 3), 99, np.int64)
    new_of = np.full(P, -1, np.int64)
    n_groups = (N + GROUP - 1) // GROUP
    blk = np.zeros(GROUP * n_groups + 1, np.int64)
    for g in range(n_groups):
        at = int(res["pair_start"][GROUP * g])
        iend = min(GROUP * g + GROUP, N)
        slot, load, nc = GROUP * g, 0, 0
        for i in range(GROUP * g, iend):
            start[i] = at
            n_i = 0
            for s in range(nel):
                seg[i, s] = at
                for q in range(int(res["seg_start"][i, s]), int(res["seg_start"][i, s + 1])):
                    if keep[q]:
                        pi[at], pj[at], ps[at], new_of[q] = i, res["pair_j"][q], res["pair_shift"][q], at
                        at += 1
                        n_i += 1
            seg[i, nel] = stop[i] = at
            if i == GROUP * g or load + n_i > cap or nc >= GROUP:
                blk[slot] = i
                slot += 1
                load, nc = 0, 0
            load += n_i
            nc += 1
        blk[slot:GROUP * g + GROUP] = iend
    blk[-1] = N
    start[N] = res["pair_start"][N]
    rev = np.full(P, -1, np.int64)
    kept = np.nonzero(keep)[0]
    rev[new_of[kept]] = new_of[np.asarray(res["pair_rev"])[kept]]
    info = dict(res["info"], n_blk=GROUP * n_groups, filtered=True, rev_indirect=False)
    return dict(info=info, pair_start=start, pair_stop=stop, seg_start=seg, pair_i=pi, pair_j=pj, pair_shift=ps,
                pair_rev=rev, blk_center=blk)
