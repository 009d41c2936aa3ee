"""CPU: the cluster analysis of the device MD loop: the union-find of the reference (tests/md_cluster_reference.py)
against an independent flood fill on random graphs, the reference on frames whose clusters are known, the `md.*`
helpers on hand-made arrays, the argument checks of `DeviceMD` and the C ABI of `ta_md_set_clusters` /
`ta_md_get_clusters` / `ta_md_get_cluster_atoms`."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import md_cluster_reference as ref
from tensoralloy_amd import md


def _flood_fill(n, links, selected):
    """Components by a breadth-first search over adjacency sets: label (smallest member) and size per atom."""
    adj = [set() for _ in range(n)]
    for i, j in links:
        if i != j and selected[i] and selected[j]:
            adj[i].add(j)
            adj[j].add(i)
    label, size = [-1] * n, [0] * n
    for start in range(n):
        if not selected[start] or label[start] >= 0:
            continue
        seen, front = {start}, [start]
        while front:
            nxt = []
            for a in front:
                for b in adj[a]:
                    if b not in seen:
                        seen.add(b)
                        nxt.append(b)
            front = nxt
        for a in seen:
            label[a], size[a] = min(seen), len(seen)
    return np.array(label), np.array(size)


@pytest.mark.parametrize("n, n_links, share", [(1, 0, 1.0), (2, 1, 1.0), (40, 15, 1.0), (200, 120, 0.7), (300, 900, 0.5),
                                               (500, 260, 1.0), (64, 0, 0.5)])
def test_reference_union_find_against_a_flood_fill(n, n_links, share):
    for seed in range(4):
        rng = np.random.RandomState(1000 * n + seed)
        links = [(int(a), int(b)) for a, b in rng.randint(0, n, size=(n_links, 2))]   # (self-links among them)
        links += [(b, a) for a, b in links[::3]]                                      # ... and some links twice
        selected = rng.rand(n) < share
        label, size = ref.components(n, links, selected)
        want_label, want_size = _flood_fill(n, links, selected)
        assert np.array_equal(label, want_label) and np.array_equal(size, want_size)
        assert np.all((label >= 0) == selected) and np.all((size > 0) == selected)
        assert np.all(label[selected] <= np.nonzero(selected)[0])   # the label is the smallest member


def test_reference_on_a_chain_through_the_boundary():
    """40 atoms on a line, 2.5 A apart, in a cell of 100 A: closed through the boundary they are one cluster of 40
    atoms (not images); with the links 9 -> 10 and 29 -> 30 stretched to 3.5 A they fall into two, since 30 .. 39 and
    0 .. 9 still meet through the boundary."""
    n = 40
    perm = np.random.RandomState(5).permutation(n)
    x = np.zeros((n, 3))
    x[perm, 0] = 2.5 * np.arange(n)
    desc = dict(cells=[np.diag([2.5 * n, 12.0, 12.0])], pbc=[[True] * 3], species=np.zeros(n, dtype=int), natoms=[n],
                n_elements=1, r_link=3.0, species_mask=1)
    out = ref.clusters(x[None], n_bins=50, **desc)
    assert out["gap_r"] == pytest.approx(1.0 / 6.0, abs=1e-12)
    assert np.array_equal(out["label"], [0] * n) and np.array_equal(out["size"], [n] * n)
    assert out["hist"][0, n - 1] == 1 == out["hist"].sum() and out["series"].tolist() == [[[n, 1, n, 0]]]
    cut = x.copy()
    pos = 2.5 * np.arange(n)
    pos[10:] += 1.0
    pos[30:] += 1.0
    cut[perm, 0] = pos
    desc["cells"] = [np.diag([2.5 * n + 2.0, 12.0, 12.0])]
    out = ref.clusters(cut[None], n_bins=4, **desc)
    sizes, members = md.clusters_from_labels(out["label"])
    assert sizes.tolist() == [20, 20]
    assert sorted(map(sorted, (m.tolist() for m in members))) == sorted([sorted(perm[10:30].tolist()),
                                                                        sorted(perm[np.r_[0:10, 30:40]].tolist())])
    assert out["hist"].tolist() == [[0, 0, 0, 2]]   # the overflow bin
    assert out["series"][0, 0].tolist() == [n, 2, 20, 0]   # among equals the smallest label: atom 0 is in one of them
    # a species that is not selected, and nothing selected at all
    desc["species"] = (np.arange(n) % 2)
    desc["n_elements"] = 2
    none = ref.clusters(cut[None], n_bins=4, **dict(desc, species_mask=2, r_link=1.0))
    assert none["series"][0, 0].tolist() == [20, 20, 1, 1] and none["hist"].tolist() == [[20, 0, 0, 0]]
    assert np.array_equal(none["label"], np.where(np.arange(n) % 2, np.arange(n), -1))
    n_conn = np.zeros((1, n), dtype=int)
    empty = ref.clusters(cut[None], n_bins=4, n_min=3, n_conn=n_conn, **desc)
    assert empty["series"][0, 0].tolist() == [0, 0, 0, -1] and not empty["hist"].any()
    assert np.array_equal(empty["label"], [-1] * n) and not empty["size"].any()


def test_helpers_on_hand_made_arrays():
    series = np.array([[[5, 2, 3, 0], [0, 0, 0, -1]], [[6, 1, 6, 0], [2, 2, 1, 9]], [[6, 2, 4, 1], [3, 1, 3, 8]]])
    t, size = md.largest_cluster(series, [0, 4, 8], 0.5)
    assert np.array_equal(t, [0.0, 2.0, 4.0]) and np.array_equal(size, [[3, 0], [6, 1], [4, 3]])
    with pytest.raises(ValueError, match="series must be"):
        md.largest_cluster(series[:, :, :3], [0, 4, 8], 0.5)
    with pytest.raises(ValueError, match="series must be"):
        md.largest_cluster(series, [0, 4], 0.5)
    hist = np.array([[4, 0, 2, 0], [0, 2, 0, 6]])
    sizes, mean = md.cluster_size_distribution(hist, n_samples=2)
    assert np.array_equal(sizes, [1, 2, 3, 4]) and np.array_equal(mean, [1.0, 0.5, 0.5, 1.5])
    assert np.array_equal(md.cluster_size_distribution(hist[0])[1], [4.0, 0.0, 2.0, 0.0])
    with pytest.raises(ValueError, match="hist must be"):
        md.cluster_size_distribution(np.zeros((2, 0)))
    with pytest.raises(ValueError, match="n_samples must be"):
        md.cluster_size_distribution(hist, 0)
    sizes, members = md.clusters_from_labels(np.array([3, -1, 2, 3, 2, 5, 2, -1], dtype=np.int32))
    assert sizes.tolist() == [3, 2, 1] and [m.tolist() for m in members] == [[2, 4, 6], [0, 3], [5]]
    sizes, members = md.clusters_from_labels(np.array([4, 1, 1, -1, 4]))   # equal sizes: the smaller label first
    assert sizes.tolist() == [2, 2] and [m.tolist() for m in members] == [[1, 2], [0, 4]]
    assert md.clusters_from_labels(np.full(3, -1))[0].shape == (0,)
    with pytest.raises(ValueError, match="label must be"):
        md.clusters_from_labels(np.zeros((2, 2)))
    for name in ("largest_cluster", "cluster_size_distribution", "clusters_from_labels"):
        assert name in md.__all__ and callable(getattr(md, name))


def test_device_md_argument_errors():
    from tests.helpers import fcc
    atoms = fcc(rep=(1, 1, 1))

    class Recorder:  # stands in for an engine: anything it is asked to do is a failure of the checks
        def md_run(self, *a, **k):
            raise AssertionError("reached the engine")
        set_frames = md_init = md_set_thermostat = md_set_langevin = md_set_nose_hoover = md_set_sampling = md_run
        md_set_barostat = md_set_rdf = md_set_adf = md_set_order = md_set_clusters = md_clusters = md_cluster_atoms = md_run

    for bad in (0, -1, 4097, 2.5, True):
        with pytest.raises(ValueError, match="cluster_bins must be"):
            md.DeviceMD(Recorder(), atoms, md.fs, cluster_bins=bad)
    for bad in (0, -3, 1.5, False):
        with pytest.raises(ValueError, match="cluster_every must be"):
            md.DeviceMD(Recorder(), atoms, md.fs, cluster_bins=8, cluster_every=bad)
    for bad in (0, -1, 1048577, 2.0, True):
        with pytest.raises(ValueError, match="cluster_series must be"):
            md.DeviceMD(Recorder(), atoms, md.fs, cluster_bins=8, cluster_series=bad)
    for bad in (-1, 32, 1.5, True):
        with pytest.raises(ValueError, match="cluster_nmin must be"):
            md.DeviceMD(Recorder(), atoms, md.fs, cluster_bins=8, cluster_nmin=bad, order_bins=8)
    with pytest.raises(ValueError, match=r"cluster_nmin > 0 reads the solid bonds .* \(order_bins\)"):
        md.DeviceMD(Recorder(), atoms, md.fs, cluster_bins=8, cluster_nmin=8)
    with pytest.raises(ValueError, match="cluster_every must be a multiple of order_every"):
        md.DeviceMD(Recorder(), atoms, md.fs, cluster_bins=8, cluster_nmin=8, cluster_every=3, order_bins=8, order_every=2)
    for bad in ((), (-1,), (0.5,), (True,), -2):
        with pytest.raises(ValueError, match="cluster_species must be"):
            md.DeviceMD(Recorder(), atoms, md.fs, cluster_bins=8, cluster_species=bad)
    for bad in (0.0, -1.0, float("nan"), [3.0, 3.0], [[3.0, 2.0], [2.5, 3.0]]):
        with pytest.raises(ValueError, match="cluster_rlink must be"):
            md.DeviceMD(Recorder(), atoms, md.fs, cluster_bins=8, cluster_rlink=bad)
    for kw in (dict(cluster_every=2), dict(cluster_rlink=3.0), dict(cluster_nmin=8), dict(cluster_species=("Ni",)),
               dict(cluster_series=4)):
        with pytest.raises(ValueError, match="belong to the cluster analysis"):
            md.DeviceMD(Recorder(), atoms, md.fs, **kw)
    with pytest.raises(AssertionError, match="reached the engine"):   # a valid request gets through, under the barostat too
        md.DeviceMD(Recorder(), atoms, md.fs, cluster_bins=8, pressure=0.0, taup=100 * md.fs, compressibility=1.0)


def test_device_md_hands_a_valid_request_to_md_set_clusters():
    from tests.helpers import fcc
    atoms = fcc(rep=(1, 1, 1))
    calls = []

    class Reached(Exception):
        pass

    class Old:   # the engine as it was before the cluster analysis
        def _ok(self, *a, **k):
            return None
        set_frames = md_init = md_set_thermostat = md_set_langevin = md_set_nose_hoover = md_set_barostat = _ok
        md_set_sampling = md_set_rdf = md_set_adf = md_set_order = _ok

        def md_run(self, n, dt, **k):
            raise Reached("md_run")

    class New(Old):
        def md_set_clusters(self, *a, **k):
            calls.append((a, k))
            raise Reached("md_set_clusters")

    with pytest.raises(Reached, match="md_set_clusters"):
        md.DeviceMD(New(), atoms, md.fs, cluster_bins=100, cluster_rlink=3.0, cluster_every=4, cluster_nmin=8, order_bins=8,
                    order_every=2, cluster_species=("Ni",), cluster_series=16)
    assert calls == [((3.0, 8, ("Ni",), 100, 16, 4), {})]
    with pytest.raises(Reached, match="md_set_clusters"):
        md.DeviceMD(New(), atoms, md.fs, cluster_bins=np.int64(16))
    assert calls[1] == ((None, 0, None, 16, 1, 1), {})
    with pytest.raises(Reached, match="md_run"):   # nothing new is called when cluster_bins is None
        md.DeviceMD(Old(), atoms, md.fs)
    assert len(calls) == 2

    class LeftOn(New):   # an engine on which an earlier DeviceMD left the feature on is told to switch it off
        md_cluster_bins = 50

    with pytest.raises(Reached, match="md_set_clusters"):
        md.DeviceMD(LeftOn(), atoms, md.fs)
    assert calls[2] == ((), {"n_bins": 0})


def test_abi_of_the_cluster_calls(lib):
    from tensoralloy_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "tensoralloy_amd.h")) as fp:
        header = re.sub(r"/\*.*?\*/", "", fp.read(), flags=re.S)
    for name in ("ta_md_set_clusters", "ta_md_get_clusters", "ta_md_get_cluster_atoms"):
        assert re.search(r"\bint %s\s*\(ta_handle h," % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert re.search(r"\bint ta_md_set_clusters\s*\(ta_handle h, const ta_md_cluster_params \*p, const double \*r_link_pairs\);",
                     header)
    assert re.search(r"\bint ta_md_get_clusters\s*\(ta_handle h, int64_t \*hist, int64_t \*series, int64_t \*steps, "
                     r"int64_t \*info,\s+double \*r_link_pairs\);", header)
    assert re.search(r"\bint ta_md_get_cluster_atoms\s*\(ta_handle h, int32_t \*label, int32_t \*size\);", header)
    assert re.search(r"^#define TA_MD_CLUSTER_MAX_SERIES 1048576$", header, re.M) and _lib.TA_MD_CLUSTER_MAX_SERIES == 1048576
    assert re.search(r"^#define TA_ABI_VERSION 5$", header, re.M) and lib.ta_abi_version() == 5 == _lib.TA_ABI_VERSION
    struct = re.search(r"typedef struct \{([^}]*)\} ta_md_cluster_params;", header).group(1)
    names = ["r_link", "n_min", "species_mask", "n_bins", "n_series", "sample_every"]
    assert re.findall(r"\b(?:double|int32_t)\s+(\w+);", struct) == names
    assert C.sizeof(_lib.MdClusterParams) == 32
    assert [f[0] for f in _lib.MdClusterParams._fields_] == names
    assert [getattr(_lib.MdClusterParams, n).offset for n in names] == [0, 8, 12, 16, 20, 24]
    assert "ta_md_cluster.hip" in _lib.SOURCES
    assert os.path.exists(os.path.join(root, "tensoralloy_amd", "csrc", "ta_md_cluster.hip"))
    with open(os.path.join(root, "tensoralloy_amd", "csrc", "ta_md.h")) as fp:
        text = fp.read()
    assert "struct MdClusterLaunch" in text and "void launch_md_cluster(const MdClusterLaunch &a, hipStream_t s);" in text
