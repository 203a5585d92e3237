"""The minimum spanning forest on the device (csrc/mst.hip: mst_scan, mst_tie, mst_hook, mst_flatten, the edge sort; C ABI
abacus_mst[_dev]; analysis/mst.py) against the NumPy statement tests/mst_statement.py.  Needs an MI355X: run with `-m gpu`.
Every comparison is exact: the edges' ends, the bits of r2, the degrees, the labels, nedges and ncomp - no tolerance anywhere."""
import mst_statement as st
import numpy as np
import pytest
from test_groups_host import BOX, catalogue
from test_mst_host import CASE_IDS, CASES, judged, points

pytestmark = pytest.mark.gpu


def _device(cols, box, rmax):
    """the device's result with degrees and labels; without them the edges are what they were"""
    from abacusutils_amd.analysis.mst import minimum_spanning_tree
    res = minimum_spanning_tree(*cols, box, rmax, return_degree=True, return_labels=True)
    bare = minimum_spanning_tree(*cols, box, rmax, return_degree=False, return_labels=False)
    assert bare['degree'] is None and bare['labels'] is None and bare['n'] == res['n'] == len(res['labels']) == len(res['degree'])
    assert (bare['nedges'], bare['ncomp']) == (res['nedges'], res['ncomp'])
    for k in ('i', 'j'):
        np.testing.assert_array_equal(bare[k], res[k])
    np.testing.assert_array_equal(bare['r2'].view(np.uint32), res['r2'].view(np.uint32))
    return res


def _check(cols, box, rmax, want=None, host=None):
    """`cols` (host or resident) on the device against the statement's forest of the host columns `host`"""
    lo, hi, r2 = want if want is not None else st.forest(*(host or cols), box, rmax)
    n = len(cols[0])
    res = _device(cols, box, rmax)
    assert res['i'].dtype == res['j'].dtype == res['degree'].dtype == res['labels'].dtype == np.uint32
    assert res['r2'].dtype == np.float32 and res['length'].dtype == np.float64
    assert res['nedges'] == len(lo) == len(res['i']) == len(res['j']) == len(res['r2'])
    np.testing.assert_array_equal(res['i'], lo)
    np.testing.assert_array_equal(res['j'], hi)
    np.testing.assert_array_equal(res['r2'].view(np.uint32), r2.view(np.uint32))
    np.testing.assert_array_equal(res['length'], np.sqrt(r2.astype(np.float64)))
    np.testing.assert_array_equal(res['degree'], np.bincount(lo, minlength=n) + np.bincount(hi, minlength=n))
    labels, ncomp = st.labels_of(n, lo, hi)
    np.testing.assert_array_equal(res['labels'], labels)
    assert res['ncomp'] == ncomp == n - res['nedges']
    return res


def _frame(cols, frame, box, seed):
    """the columns shifted into [frame, frame + box), or - 'unwrapped' - spilling over both box edges"""
    if frame == 'unwrapped':
        return [v + np.where(np.random.default_rng(seed + s).random(len(v)) < 0.1, box, 0.0) - 20.0 for s, v in enumerate(cols)]
    return [v + frame for v in cols]


@pytest.mark.parametrize('frame', [0.0, -50.0, 'unwrapped'])
@pytest.mark.parametrize('kind,rmax', CASES[:4], ids=CASE_IDS[:4])
def test_statement_cases_in_every_frame(kind, rmax, frame):
    """the clustered and the uniform catalogue, sparse (rmax = 2) and percolating (7.6), in [0, L), [-L/2, L/2) and with
    coordinates spilling over both box edges: host columns, then DeviceArray columns of float32 and of float64.  That the cases
    are no degenerate ones is asserted on the statement in test_mst_host.py; a shifted frame rounds the float32 coordinates
    anew, so its statement is computed for it"""
    from abacusutils_amd import _lib
    cols = catalogue(kind)
    if frame == 0.0:
        want = judged(kind, rmax)[1]
    else:
        cols = _frame(cols, frame, BOX, 1)
        want = st.forest(*cols, BOX, rmax)
    assert 0 < len(want[0]) < len(cols[0])
    _check(cols, BOX, rmax, want=want)
    for dt in (np.float32, np.float64):
        dev = [_lib.DeviceArray(np.ascontiguousarray(c, dtype=dt)) for c in cols]
        try:
            _check(dev, BOX, rmax, want=want)
        finally:
            for a in dev:
                a.free()
    with pytest.raises(TypeError):
        d = _lib.DeviceArray(np.ascontiguousarray(cols[0], dtype=np.float32))
        try:
            _device([d, cols[1], cols[2]], BOX, rmax)
        finally:
            d.free()


@pytest.mark.parametrize('kind,rmax', CASES[4:], ids=CASE_IDS[4:])
def test_lattices_where_every_edge_ties(kind, rmax):
    """6^3 points that fill a periodic box of 6 and 8^3 in a corner of a box of 100, in random order: one value of r2 for every
    edge, so the forest is decided by the indices alone - edge for edge.  A missing tie-break shows here (as a cycle, or as
    another tree of the same weight)"""
    from abacusutils_amd.analysis.mst import last_stats
    cols, box = points(kind)
    res = _check(cols, box, rmax, want=judged(kind, rmax)[1])
    assert res['ncomp'] == 1 and len(np.unique(res['r2'])) == 1 and res['r2'][0] == 1.0
    assert 1 <= last_stats()['rounds'] <= int(np.ceil(np.log2(len(cols[0]))))


def test_coincident_points_and_the_strict_edge():
    """300 positions, each present three times: edges of length zero whose order is the indices' alone, under longer ones; and two
    points at exactly r2 == rmax^2, which are not joined"""
    rng = np.random.default_rng(52)
    p = np.tile(rng.random((300, 3)) * 100.0, (3, 1))[rng.permutation(900)]
    cols = [p[:, d].copy() for d in range(3)]
    res = _check(cols, 100.0, 12.0)
    assert (res['r2'] == 0).sum() == 600 and (res['r2'] > 0).sum() > 100
    res = _check([[0.0, 1.5], [0.0, 0.0], [0.0, 0.0]], 100.0, 1.5)
    assert res['nedges'] == 0 and res['ncomp'] == 2 and list(res['labels']) == [0, 1] and list(res['degree']) == [0, 0]
    res = _check([[0.0, 1.4999999], [0.0, 0.0], [0.0, 0.0]], 100.0, 1.5)
    assert res['nedges'] == 1 and res['ncomp'] == 1 and list(res['labels']) == [0, 0] and list(res['degree']) == [1, 1]


def test_small_n():
    from abacusutils_amd.analysis.mst import last_stats
    res = _check([np.zeros(0)] * 3, 100.0, 1.0)
    assert (res['nedges'], res['ncomp'], res['n']) == (0, 0, 0) and res['i'].shape == (0,) and res['labels'].shape == (0,)
    assert last_stats()['rounds'] == 0
    res = _check([[5.0], [6.0], [7.0]], 100.0, 1.0)
    assert (res['nedges'], res['ncomp']) == (0, 1) and list(res['labels']) == [0] and list(res['degree']) == [0]
    assert last_stats()['rounds'] == 0
    res = _check([[5.0, 5.5], [6.0, 6.0], [7.0, 7.0]], 100.0, 1.0)
    assert (list(res['i']), list(res['j']), list(res['r2'])) == ([0], [1], [0.25]) and res['ncomp'] == 1
    assert last_stats()['rounds'] == 1
    res = _check([[5.0, 6.5], [6.0, 6.0], [7.0, 7.0]], 100.0, 1.0)
    assert (res['nedges'], res['ncomp']) == (0, 2)
    res = _check([[99.75, 0.25], [6.0, 6.0], [0.25, 99.75]], 100.0, 1.0)                      # through two faces
    assert res['nedges'] == 1 and list(res['r2']) == [0.5]
    res = _check([[5.0, 5.5, 6.25], [6.0, 6.0, 6.0], [7.0, 7.0, 7.0]], 100.0, 1.0)            # 0 - 1 - 2, and 0 - 2 too long
    assert (list(res['i']), list(res['j'])) == ([0, 1], [1, 2]) and list(res['degree']) == [1, 2, 1]
    res = _check([[5.0, 50.0, 5.5], [6.0, 6.0, 6.0], [7.0, 7.0, 7.0]], 100.0, 1.0)
    assert (list(res['i']), list(res['j'])) == ([0], [2]) and list(res['labels']) == [0, 1, 0] and res['ncomp'] == 2


def winding_line(n, box, b, seed, cut=None):
    """n points 0.9 b apart (a little more: the line climbs) on a line along x that winds through the periodic x face, every
    winding 2 b further in y, so that only neighbours along the line lie within b; handed over in a random permutation.  `cut`:
    that point of the line is left out, which opens a gap of 1.8 b.  Returns (columns, the position of every point along the
    line)."""
    s = np.arange(n) * 0.9 * b
    x, y, z = s % box, 1.0 + s / box * 2.0 * b, np.full(n, 0.25 * box)
    assert y.max() < box - 3.0 * b                   # the first and the last winding do not meet through the y face
    along = np.arange(n)
    if cut is not None:
        keep = along != cut
        x, y, z, along = x[keep], y[keep], z[keep], along[keep]
    perm = np.random.default_rng(seed).permutation(len(x))
    return [x[perm], y[perm], z[perm]], along[perm]


def test_a_line_is_its_own_tree():
    """5000 points on one line through the periodic face, in random order, held to the statement: the forest is the line's
    m - 1 links; with one point cut out, two trees"""
    for cut in (None, 3210):
        cols, along = winding_line(5000, 100.0, 1.0, 71 + (cut is not None), cut=cut)
        res = _check(cols, 100.0, 1.0)
        m = len(along)
        assert res['ncomp'] == (1 if cut is None else 2) and res['nedges'] == m - res['ncomp']
        assert np.all(np.abs(along[res['i']] - along[res['j']]) == 1)


def test_a_long_line_on_both_sort_paths(options):
    """the same line with 250 000 points, above the switch to the radix sort, and the counting sort on the same input
    (pairs_countsort): the statement's n^2 pairs are out of reach, but the answer is known - every edge joins neighbours along the
    line (the 5000-point form above is held to the statement) - and both paths must give it, byte for byte"""
    from abacusutils_amd.analysis.mst import last_stats, minimum_spanning_tree
    n, b = 250000, 0.14
    for cut in (None, 123456):
        cols, along = winding_line(n, 100.0, b, 73, cut=cut)
        m, trees = len(along), 1 if cut is None else 2
        radix = minimum_spanning_tree(*cols, 100.0, b, return_labels=True)
        rounds = last_stats()['rounds']
        options.set('pairs_countsort')
        counting = minimum_spanning_tree(*cols, 100.0, b, return_labels=True)
        assert last_stats()['rounds'] == rounds <= int(np.ceil(np.log2(m))) + 1
        options.reset()
        for k in ('i', 'j', 'r2', 'degree', 'labels'):
            assert radix[k].tobytes() == counting[k].tobytes(), k
        for res in (radix, counting):
            assert (res['nedges'], res['ncomp']) == (m - trees, trees)
            assert np.all(np.abs(along[res['i']].astype(np.int64) - along[res['j']]) == 1)   # (the cut leaves a gap of 1.8 b: no edge)
            np.testing.assert_array_equal(np.bincount(res['degree']), [0, 2 * trees, m - 2 * trees])
            assert np.all(np.diff(res['r2'].view(np.uint32).astype(np.int64)) >= 0) and np.all(res['i'] < res['j'])
            side = np.zeros(m, bool) if cut is None else along > cut
            for sd in (False, True):
                if (side == sd).any():
                    assert np.all(res['labels'][side == sd] == np.flatnonzero(side == sd).min())


@pytest.mark.parametrize('rmax', [2.0, 0.05])
def test_a_crowded_cell(rmax):
    """700 points inside a fifth of one cell of the grid - three slices of primaries and, at rmax = 2, three tiles of candidates in
    one workgroup; at rmax = 2 every pair of them is an edge of the graph, at 0.05 they fall into many trees - with exact twins
    among them, and 400 uniform points elsewhere"""
    rng = np.random.default_rng(43)
    blob = 11.0 + 0.4 * rng.random((700, 3))              # [11, 11.4) in every dimension
    blob[600:] = blob[:100]                               # twins
    rest = rng.random((400, 3)) * 100.0
    p = np.concatenate([blob, rest])[rng.permutation(1100)]
    cols = [p[:, d].copy() for d in range(3)]
    for nc in (49, 128):                                  # the cells per dimension at rmax = 2 and at 0.05 (capped): one cell, a fifth or half of it
        assert np.floor(11.0 * nc / 100.0) == np.floor(11.3999 * nc / 100.0)
    res = _check(cols, 100.0, rmax)
    size = np.bincount(res['labels'])
    assert size.max() >= 700 if rmax == 2.0 else (size.max() > 4 and (size == 1).sum() > 100)
    assert (res['r2'] == 0).sum() == 100


@pytest.mark.parametrize('rmax', [40.0, 50.0])
def test_fewer_than_three_cells_per_dimension(rmax):
    """rmax = 0.4 L and exactly L / 2: every dimension is one cell that is its own neighbour, and the minimum image decides"""
    from abacusutils_amd.analysis.mst import last_stats
    p = np.random.default_rng(21).random((1200, 3)) * 100.0
    res = _check([p[:, d].copy() for d in range(3)], 100.0, rmax)
    assert res['ncomp'] == 1 and last_stats()['cells_xy'] == 1 and last_stats()['cells_z'] == 1


def test_against_the_group_finder_on_the_device():
    """60 000 points, a third of them in clumps: the trees are the groups of fof_groups at b = rmax; the edges alone span exactly
    those components without a cycle; the forest at rmax = 2 is the one at 7.6 filtered; the rounds are logarithmic"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    from abacusutils_amd.analysis.groups import fof_groups
    from abacusutils_amd.analysis.mst import last_stats, minimum_spanning_tree
    rng = np.random.default_rng(64)
    n, box = 60000, 250.0
    centres = rng.random((400, 3)) * box
    p = np.concatenate([(np.repeat(centres, 50, axis=0) + rng.normal(0.0, 1.5, (20000, 3))) % box, rng.random((40000, 3)) * box])
    cols = [p[:, d].copy() for d in range(3)]
    got = {}
    for rmax in (2.0, 7.6):
        res = got[rmax] = minimum_spanning_tree(*cols, box, rmax, return_labels=True)
        stats = last_stats()
        groups = fof_groups(*cols, box, rmax, nmax=8)
        np.testing.assert_array_equal(res['labels'], groups['labels'])
        assert res['ncomp'] == groups['ngroups'] and res['nedges'] == n - res['ncomp'] and 1 < res['ncomp'] < n
        graph = coo_matrix((np.ones(res['nedges'], np.int8), (res['i'], res['j'])), shape=(n, n))
        ncomp, comp = connected_components(graph, directed=False)
        assert ncomp == res['ncomp']                       # n - nedges components from nedges edges: no cycle
        first = np.full(ncomp, n, dtype=np.int64)
        np.minimum.at(first, comp, np.arange(n))
        np.testing.assert_array_equal(first[comp], res['labels'])
        np.testing.assert_array_equal(res['degree'], np.bincount(res['i'], minlength=n) + np.bincount(res['j'], minlength=n))
        assert np.all(res['r2'] < np.float32(rmax) * np.float32(rmax)) and np.all(res['i'] < res['j'])
        order = np.lexsort((res['j'], res['i'], res['r2']))
        np.testing.assert_array_equal(order, np.arange(res['nedges']))
        assert 1 <= stats['rounds'] <= int(np.ceil(np.log2(n))) + 1
        per = stats['per_round']
        assert per.shape == (stats['rounds'] + 1, 3) and per[:, 2].sum() == res['nedges'] and per[-1, 2] == 0 and per[0, 0] == n
        assert np.all(per[:, 1] <= per[:, 0]) and np.all(np.diff(per[:, 0].astype(np.int64)) <= 0)
        assert stats['candidates'] > 0
    small, large = got[2.0], got[7.6]
    keep = large['r2'] < np.float32(2.0) * np.float32(2.0)
    assert 0 < keep.sum() < len(keep)
    for k in ('i', 'j'):
        np.testing.assert_array_equal(small[k], large[k][keep])
    np.testing.assert_array_equal(small['r2'].view(np.uint32), large['r2'][keep].view(np.uint32))


def test_two_calls_give_identical_arrays(options):
    """the atomics emit the edges in whatever order, the counting sort hands out slots by atomics: the output depends on neither,
    nor on the plain load that spares most atomics on a root's slot (mst_always_atomic: the comparator without it)"""
    from abacusutils_amd.analysis.mst import minimum_spanning_tree
    cols = catalogue('clustered')
    first = minimum_spanning_tree(*cols, BOX, 7.6, return_labels=True)
    second = minimum_spanning_tree(*cols, BOX, 7.6, return_labels=True)
    options.set('mst_always_atomic')
    third = minimum_spanning_tree(*cols, BOX, 7.6, return_labels=True)
    options.reset()
    for other in (second, third):
        for k in ('i', 'j', 'r2', 'length', 'degree', 'labels'):
            assert first[k].tobytes() == other[k].tobytes(), k
        assert (first['nedges'], first['ncomp']) == (other['nedges'], other['ncomp'])
    np.testing.assert_array_equal(first['i'], judged('clustered', 7.6)[1][0])


def test_abacus_hod_mst():
    """AbacusHOD.compute_mst: the catalogue still in HBM gives what its host columns give"""
    from abacusutils_amd import synth
    from abacusutils_amd.analysis.groups import linking_lengths
    from abacusutils_amd.analysis.mst import minimum_spanning_tree
    from abacusutils_amd.hod.abacus_hod import AbacusHOD
    hd, pd, params = synth.synth_hod_inputs(100000, 100000, seed=19, lbox=1000.0)
    hod = dict(tracer_flags={'LRG': True, 'ELG': True, 'QSO': False}, want_ranks=False, want_AB=True, want_shear=False, want_rsd=True,
               LRG_params=dict(synth.LRG_PARAMS, logM_cut=12.3, logM1=13.3), ELG_params=dict(synth.ELG_PARAMS), QSO_params=synth.QSO_PARAMS)
    clustering = dict(clustering_type='xirppi', pimax=30, pi_bin_size=5, bin_params=dict(logmin=-0.77, logmax=1.47, nbins=9))
    ball = AbacusHOD.from_arrays(hd, pd, params, hod, clustering)
    mock = ball.run_hod()
    assert all(mock.device_xyz(tr) is not None for tr in mock)
    plain = {tr: dict(mock[tr]) for tr in mock}
    rmax = {tr: linking_lengths(len(plain[tr]['x']), ball.lbox, 1.0)[0] for tr in mock}
    for tr in mock:
        n = len(plain[tr]['x'])
        got = ball.compute_mst(mock, rmax[tr], return_labels=True)[tr]
        want = ball.compute_mst(plain, rmax[tr], return_labels=True)[tr]
        direct = minimum_spanning_tree(*[np.asarray(plain[tr][c]) for c in 'xyz'], ball.lbox, rmax[tr], return_labels=True)
        for other in (want, direct):
            for k in ('i', 'j', 'r2', 'length', 'degree', 'labels'):
                assert got[k].tobytes() == other[k].tobytes(), (tr, k)
            assert (got['nedges'], got['ncomp'], got['n']) == (other['nedges'], other['ncomp'], other['n']) and got['n'] == n
        assert 0 < got['nedges'] == n - got['ncomp'] and (got['degree'] >= 3).sum() > 0
    bare = ball.compute_mst(mock, rmax['LRG'], return_degree=False)
    assert set(bare) == set(mock) and all(v['degree'] is None and v['labels'] is None for v in bare.values())
