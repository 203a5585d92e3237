"""The minimum spanning forest without a GPU: the two forms of the NumPy statement tests/mst_statement.py (Kruskal, Boruvka by
rank) against each other, against the friends-of-friends statement and against scipy's minimum_spanning_tree; the nesting of the
forests in rmax; analysis/mst.py's vectorised branches against a plain walk; the normalisation of mst_statistics; and every
validation rule of abacus_mst[_dev] - refused before the device is touched."""
import ctypes as C
import functools

import groups_statement as gst
import mst_statement as st
import numpy as np
import pytest
from test_groups_host import BOX, catalogue

# (name, rmax): the catalogues of test_groups_host.py, sparse and percolating, and two lattices on which every edge ties
CASES = [('clustered', 2.0), ('clustered', 7.6), ('uniform', 2.0), ('uniform', 7.6), ('lattice6', 1.25), ('lattice8', 1.25)]
CASE_IDS = [f'{c}-{r}' for c, r in CASES]
# edges of G(rmax), edges whose r2 is not the first of its value, edges of the forest, rounds of Boruvka by rank
EXPECTED = {('clustered', 2.0): (12204, 2, 2351, 4), ('clustered', 7.6): (83998, 88, 3880, 6), ('uniform', 2.0): (268, 0, 263, 1),
            ('uniform', 7.6): (14762, 9, 3998, 7), ('lattice6', 1.25): (648, 647, 215, None), ('lattice8', 1.25): (1344, 1343, 511, None)}


@functools.lru_cache(maxsize=None)
def points(kind):
    """(columns, boxsize).  'lattice6': 6^3 points a unit apart that fill a periodic box of 6 - every face wraps; 'lattice8': 8^3
    points a unit apart in a corner of a box of 100 - nothing wraps; both in a random order, so that the index order of the
    tie-break has nothing to do with the geometry.  Else the catalogues of test_groups_host.py in their box of 100."""
    if kind.startswith('lattice'):
        m = int(kind[7:])
        g = np.stack(np.meshgrid(*[np.arange(m) + 0.5] * 3, indexing='ij'), axis=-1).reshape(-1, 3)
        g = g[np.random.default_rng(60 + m).permutation(len(g))]
        cols = [g[:, d].copy() for d in range(3)]
        for c in cols:
            c.setflags(write=False)
        return cols, (6.0 if m == 6 else 100.0)
    return catalogue(kind), BOX


@functools.lru_cache(maxsize=None)
def judged(kind, rmax):
    """(graph edges, forest) of the statement: (lo, hi, r2) each, in key order; computed once, shared, read-only"""
    cols, box = points(kind)
    edges = st.graph_edges(*cols, box, rmax)
    forest = st.forest(*cols, box, rmax, edges=edges)
    for a in (*edges, *forest):
        a.setflags(write=False)
    return edges, forest


def tied(r2):
    return len(r2) - len(np.unique(r2))


@pytest.mark.parametrize('kind,rmax', CASES, ids=CASE_IDS)
def test_kruskal_boruvka_groups_and_scipy_agree(kind, rmax):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import minimum_spanning_tree
    cols, box = points(kind)
    n = len(cols[0])
    edges, (lo, hi, r2) = judged(kind, rmax)
    blo, bhi, br2, rounds = st.forest_by_rank(*cols, box, rmax, edges=edges)
    print(f'{kind} rmax = {rmax}: {len(edges[0])} edges, {tied(edges[2])} tied, {len(lo)} in the forest, {rounds} rounds')
    # edge for edge, in the key order
    np.testing.assert_array_equal(lo, blo), np.testing.assert_array_equal(hi, bhi)
    np.testing.assert_array_equal(r2.view(np.uint32), br2.view(np.uint32))
    assert np.all(lo < hi)
    order = np.lexsort((hi, lo, r2))
    np.testing.assert_array_equal(order, np.arange(len(lo)))
    # the trees are the friends-of-friends groups at b = rmax
    groups = gst.groups(*cols, box, rmax)[0]
    labels, ncomp = st.labels_of(n, lo, hi)
    np.testing.assert_array_equal(labels, groups)
    assert len(lo) == n - ncomp == n - len(np.unique(groups))
    want = EXPECTED[kind, rmax]
    assert (len(edges[0]), tied(edges[2]), len(lo)) == want[:3]
    assert want[3] is None or rounds == want[3]
    assert rounds <= int(np.ceil(np.log2(n)))
    # scipy's tree has the same multiset of weights (csgraph reads a zero weight as no edge: none of these cases has one)
    assert np.all(edges[2] > 0)
    graph = coo_matrix((edges[2].astype(np.float64), (edges[0], edges[1])), shape=(n, n))
    theirs = np.sort(minimum_spanning_tree(graph).data)
    np.testing.assert_array_equal(theirs, np.sort(r2.astype(np.float64)))


def test_the_cases_are_no_degenerate_ones():
    """conditions on the input, not tolerances: a sparse case of many trees, a percolating one of a single large tree, ties that
    the order must break in the catalogues and everywhere on the lattices, and nodes of every kind - leaves, chains, junctions"""
    n = 4000
    sizes = lambda kind, rmax: np.bincount(st.labels_of(n, *judged(kind, rmax)[1][:2])[0].astype(np.int64))   # noqa: E731
    assert (sizes('uniform', 2.0) == 1).sum() > n // 2
    assert sizes('uniform', 7.6).max() > n // 2 and sizes('clustered', 7.6).max() > n // 2
    assert (sizes('clustered', 2.0) >= 10).sum() >= 20 and (sizes('clustered', 2.0) == 1).sum() > 100
    assert tied(judged('clustered', 7.6)[0][2]) > 50 and tied(judged('uniform', 7.6)[0][2]) > 0
    for kind in ('lattice6', 'lattice8'):
        assert len(np.unique(judged(kind, 1.25)[0][2])) == 1
    lo, hi, _ = judged('clustered', 7.6)[1]
    degree = np.bincount(lo, minlength=n) + np.bincount(hi, minlength=n)
    assert (degree == 1).sum() > 500 and (degree == 2).sum() > 500 and (degree >= 3).sum() > 500 and degree.max() >= 4


@pytest.mark.parametrize('kind', ['clustered', 'uniform'])
def test_the_forests_nest(kind):
    """the forest of G(r1) is the forest of G(r2) without its edges of r2 >= r1^2"""
    small, large = judged(kind, 2.0)[1], judged(kind, 7.6)[1]
    keep = large[2] < np.float32(2.0) * np.float32(2.0)
    assert 0 < keep.sum() < len(keep)
    for a, b in zip(small, large):
        np.testing.assert_array_equal(a, b[keep])


def test_twins_and_the_strict_edge():
    """coincident points are joined at r2 = 0 and the index breaks the tie; r2 == rmax^2 is no edge"""
    x = np.array([10.0, 50.0, 10.0, 10.0])
    lo, hi, r2 = st.forest(x, x, x, 100.0, 1.0)
    np.testing.assert_array_equal(lo, [0, 0]), np.testing.assert_array_equal(hi, [2, 3])
    assert not r2.any()
    blo, bhi, _, _ = st.forest_by_rank(x, x, x, 100.0, 1.0)
    np.testing.assert_array_equal(lo, blo), np.testing.assert_array_equal(hi, bhi)
    assert len(st.forest([0.0, 1.5], [0.0, 0.0], [0.0, 0.0], 100.0, 1.5)[0]) == 0
    assert len(st.forest([0.0, 1.4999999], [0.0, 0.0], [0.0, 0.0], 100.0, 1.5)[0]) == 1


def _compare_branches(i, j, cols, box):
    """analysis/mst.py against the walk.  The ends and edge counts are integers; b and the end-to-end vector are float64 sums of
    at most k <= 10^3 terms of either sign taken in another order: they differ by at most k 2^-53 of the sum of the terms'
    magnitudes, which is b itself - 1e-12 b, and 1e-12 on s = |vector| / b"""
    from abacusutils_amd.analysis.mst import mst_branches
    got = mst_branches(i, j, *cols, box)
    want = st.branches_by_walking(i, j, *cols, box)
    assert len(got['b']) == len(want)
    if want:
        e0, e1, k, b, s = map(np.array, zip(*want))
        assert k.max() <= 1000
        np.testing.assert_array_equal(got['end0'], e0), np.testing.assert_array_equal(got['end1'], e1)
        np.testing.assert_array_equal(got['nedges'], k)
        np.testing.assert_allclose(got['b'], b, rtol=1e-12, atol=0)
        np.testing.assert_allclose(got['s'], s, rtol=0, atol=1e-12)
        assert np.all(got['s'] <= 1 + 1e-12) and np.all(got['nedges'] >= 2)
    n = len(cols[0])
    np.testing.assert_array_equal(got['degree'], np.bincount(np.asarray(i, np.int64), minlength=n) + np.bincount(np.asarray(j, np.int64), minlength=n))
    return got


@pytest.mark.parametrize('rmax', [2.0, 7.6])
def test_branches_of_the_clustered_forests(rmax):
    lo, hi, _ = judged('clustered', rmax)[1]
    got = _compare_branches(lo, hi, catalogue('clustered'), BOX)
    assert len(got['b']) > 100 and got['nedges'].max() >= 4 and got['s'].min() < 0.9
    print(f'clustered rmax = {rmax}: {len(got["b"])} branches, the longest of {got["nedges"].max()} edges')


def test_branches_of_hand_built_graphs():
    from abacusutils_amd.analysis.mst import mst_branches
    zeros = lambda n: np.zeros(n)   # noqa: E731
    # a star: no node of degree 2, no branch
    x = np.array([50.0, 51.0, 49.0, 50.0, 50.0])
    y = np.array([50.0, 50.0, 50.0, 51.0, 49.0])
    got = _compare_branches([0, 0, 0, 0], [1, 2, 3, 4], [x, y, zeros(5)], 100.0)
    assert len(got['b']) == 0 and list(got['degree']) == [4, 1, 1, 1, 1]
    # a path with a right angle: one branch over all of it, b = 4, end to end sqrt(8)
    x, y = np.array([10.0, 11.0, 12.0, 12.0, 12.0]), np.array([10.0, 10.0, 10.0, 11.0, 12.0])
    got = _compare_branches([0, 1, 2, 3], [1, 2, 3, 4], [x, y, zeros(5)], 100.0)
    assert list(got['end0']) == [0] and list(got['end1']) == [4] and list(got['nedges']) == [4]
    assert got['b'][0] == 4.0 and got['s'][0] == pytest.approx(np.sqrt(8.0) / 4.0, abs=1e-15)
    # a straight path through the periodic face, the edges in no order: s = 1 - the chain is unwrapped, not its ends' minimum image
    x = np.array([97.0, 98.5, 99.5, 1.0, 2.0, 3.5])
    got = _compare_branches([3, 0, 4, 2, 1], [4, 1, 5, 3, 2], [x, zeros(6), zeros(6)], 100.0)
    assert list(got['end0']) == [0] and list(got['end1']) == [5] and got['b'][0] == 6.5 and got['s'][0] == 1.0
    # ... and one longer than half the box: 80 steps of 1 along x
    x = (60.0 + np.arange(81)) % 100.0
    got = _compare_branches(np.arange(80), np.arange(1, 81), [x, zeros(81), zeros(81)], 100.0)
    assert got['b'][0] == 80.0 and got['s'][0] == 1.0 and list(got['nedges']) == [80]
    # a junction of three chains of 1, 2 and 3 interior nodes around node 0
    nodes = [(0, 0)] + [(k, 0) for k in (1, 2)] + [(0, k) for k in (1, 2, 3)] + [(-k, 0) for k in (1, 2, 3, 4)]
    p = 50.0 + np.array(nodes, dtype=np.float64)
    i, j = [0, 1, 0, 3, 4, 0, 6, 7, 8], [1, 2, 3, 4, 5, 6, 7, 8, 9]
    got = _compare_branches(i, j, [p[:, 0].copy(), p[:, 1].copy(), zeros(10)], 100.0)
    assert list(got['end0']) == [0, 0, 0] and list(got['end1']) == [2, 5, 9] and list(got['nedges']) == [2, 3, 4]
    # an isolated edge beside a path of three: the edge is no branch
    x = np.array([10.0, 11.0, 12.0, 40.0, 41.0])
    got = _compare_branches([0, 1, 3], [1, 2, 4], [x, zeros(5), zeros(5)], 100.0)
    assert list(got['end0']) == [0] and list(got['end1']) == [2]
    # nothing at all
    got = mst_branches([], [], [1.0], [1.0], [1.0], 100.0)
    assert len(got['b']) == 0 and list(got['degree']) == [0]
    with pytest.raises(ValueError):
        mst_branches([0], [5], x, x, x, 100.0)
    with pytest.raises(ValueError):
        mst_branches([0], [1, 2], x, x, x, 100.0)


def test_statistics_are_fractions_that_sum_to_one():
    from abacusutils_amd.analysis.mst import mst_branches, mst_statistics
    lo, hi, r2 = judged('clustered', 7.6)[1]
    n = 4000
    degree = (np.bincount(lo, minlength=n) + np.bincount(hi, minlength=n)).astype(np.uint32)
    result = {'i': lo, 'j': hi, 'r2': r2, 'length': np.sqrt(r2.astype(np.float64)), 'degree': degree, 'n': n}
    br = mst_branches(lo, hi, *catalogue('clustered'), BOX)
    got = mst_statistics(result, br, np.linspace(0.0, 7.6, 20), np.linspace(0.0, br['b'].max(), 12), np.linspace(0.0, 1.0, 11), dmax=8)
    assert got['d'].shape == (9,) and got['l'].shape == (19,) and got['b'].shape == (11,) and got['s'].shape == (10,)
    for k in 'dlbs':
        assert got[k].dtype == np.float64 and np.all(got[k] >= 0) and got[k].sum() == pytest.approx(1.0, abs=1e-12)
    np.testing.assert_array_equal(got['d'], np.bincount(degree, minlength=9) / n)
    # dmax: the last entry is open; bins that do not cover everything leave the rest out of the sum, not out of the norm
    low = mst_statistics(result, br, [0.0, 1.0], [0.0, 1.0], [0.0, 0.5], dmax=2)
    assert low['d'][2] == (degree >= 2).sum() / n and low['d'].sum() == pytest.approx(1.0, abs=1e-12)
    assert low['l'][0] == (result['length'] < 1.0).sum() / len(lo) < 1.0
    empty = mst_statistics({'length': np.zeros(0), 'degree': np.zeros(3, np.uint32)}, mst_branches([], [], [1.0] * 3, [1.0] * 3, [1.0] * 3, 10.0),
                           [0.0, 1.0], [0.0, 1.0], [0.0, 1.0])
    assert empty['d'][0] == 1.0 and not empty['l'].any() and not empty['b'].any()
    with pytest.raises(ValueError):
        mst_statistics(dict(result, degree=None), br, [0.0, 1.0], [0.0, 1.0], [0.0, 1.0])
    with pytest.raises(ValueError):
        mst_statistics(result, br, [1.0, 1.0], [0.0, 1.0], [0.0, 1.0])


def test_argument_validation_happens_before_the_device():
    """every rule of include/abacus_hip.h, through the C entries themselves on a machine without a device; every message starts
    with `abacus_mst: `, from the resident form too, and a refused call writes nothing"""
    import re

    from abacusutils_amd import _lib
    from abacusutils_amd.analysis.mst import minimum_spanning_tree
    L = _lib.lib()
    f = np.zeros(4, np.float32)
    ei, ej, deg, lab = (np.full(4, 77, np.uint32) for _ in range(4))
    er2 = np.full(4, 77.0, np.float32)
    ne, nc = C.c_uint64(77), C.c_uint64(77)
    p, n4, big = _lib.ptr, C.c_int64(4), C.c_int64(1 << 31)
    fl = C.c_float

    def refused(rc):
        assert rc != 0 and re.match(r'^abacus_mst: ', L.abacus_last_error().decode())

    def host(x=f, y=f, z=f, n=n4, box=100.0, rmax=1.0, i=ei, j=ej, r2=er2, e=ne, c=nc):
        return L.abacus_mst(p(x), p(y), p(z), n, fl(box), fl(rmax), p(i), p(j), p(r2), p(deg), p(lab), None if e is None else C.byref(e),
                            None if c is None else C.byref(c))

    def dev(dt, n=n4, box=100.0, rmax=1.0):
        # the host arrays stand in for device pointers - a refused call reads none of them
        return L.abacus_mst_dev(p(f), p(f), p(f), n, dt, fl(box), fl(rmax), p(ei), p(ej), p(er2), p(deg), p(lab), C.byref(ne), C.byref(nc))
    for kw in (dict(x=None), dict(y=None), dict(z=None), dict(i=None), dict(j=None), dict(r2=None), dict(e=None), dict(c=None),   # null arguments
               dict(box=0.0), dict(box=-1.0), dict(box=float('nan')),                                                       # boxsize > 0
               dict(rmax=0.0), dict(rmax=-1.0), dict(rmax=float('nan')), dict(rmax=50.5),                                   # 0 < rmax <= L / 2
               dict(n=big), dict(n=C.c_int64(-1))):                                                                         # 0 <= n < 2^31
        refused(host(**kw))
    refused(dev(7))                                                                                                          # pos_dtype
    refused(dev(-1))
    for kw in (dict(rmax=0.0), dict(rmax=60.0), dict(box=0.0), dict(n=big), dict(n=C.c_int64(-1))):
        refused(dev(0, **kw))
        refused(dev(1, **kw))
    for a in (ei, ej, deg, lab):
        assert np.all(a == 77)
    assert np.all(er2 == 77.0) and ne.value == 77 and nc.value == 77
    # and through the Python entry
    x = np.linspace(1.0, 9.0, 4)
    for rmax in (0.0, -2.0, 51.0):
        with pytest.raises(_lib.AbacusHipError, match=r'^abacus_mst: '):
            minimum_spanning_tree(x, x, x, 100.0, rmax)
    with pytest.raises(ValueError):
        minimum_spanning_tree(x, x, x[:3], 100.0, 1.0)
