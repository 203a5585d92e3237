"""Friends-of-friends groups on the device (csrc/fof.hip: fof_link, fof_flatten, fof_reduce, fof_emit; C ABI
abacus_fof[_dev]; analysis/groups.py) against the NumPy statement tests/groups_statement.py.  Needs an MI355X: run with
`-m gpu`.  Every comparison is between integers and exact: labels, ngroups, mult, and the links of abacus_fof_stats."""
import functools

import groups_statement as st
import numpy as np
import pytest
from test_groups_host import BOX, CASE_IDS, CASES, catalogue, judged, sizes_of

pytestmark = pytest.mark.gpu

NMAX = 64


def _device(cols, box, b_perp, b_par=None, nmax=NMAX):
    """the device's result with labels and its links; without the labels mult and ngroups are what they were"""
    from abacusutils_amd.analysis.groups import fof_groups, last_stats
    res = fof_groups(*cols, box, b_perp, b_par=b_par, nmax=nmax)
    links = last_stats()['links']
    bare = fof_groups(*cols, box, b_perp, b_par=b_par, nmax=nmax, return_labels=False)
    assert bare['labels'] is None and bare['n'] == res['n'] == len(res['labels'])
    assert bare['ngroups'] == res['ngroups'] and last_stats()['links'] == links
    np.testing.assert_array_equal(bare['mult'], res['mult'])
    return res, links


def _check(cols, box, b_perp, b_par=None, nmax=NMAX, want=None, host=None):
    """`cols` (host or resident) on the device against the statement of the host columns `host`"""
    labels_s, _, links_s = want if want is not None else st.groups(*(host or cols), box, b_perp, b_par)
    mult_s, ngroups_s = st.multiplicity(labels_s, nmax)
    res, links = _device(cols, box, b_perp, b_par, nmax)
    assert res['labels'].dtype == np.uint32 and res['mult'].dtype == np.uint64 and res['mult'].shape == (nmax + 1,)
    np.testing.assert_array_equal(res['labels'], labels_s)
    np.testing.assert_array_equal(res['mult'], mult_s)
    assert res['ngroups'] == ngroups_s and links == links_s
    return res


def _uniform(n, box, seed):
    p = np.random.default_rng(seed).random((n, 3)) * box
    return [p[:, d].copy() for d in range(3)]


@pytest.mark.parametrize('frame', [0.0, -50.0, 'unwrapped'])
@pytest.mark.parametrize('kind,b_perp,b_par', CASES, ids=CASE_IDS)
def test_statement_cases_in_every_frame(kind, b_perp, b_par, frame):
    """the clustered catalogue (spheres at b = 1 and 2, cylinders several b_perp long) and the uniform one (sparse at b = 2.5:
    mostly singletons; percolating at b = 7.6: one group of nearly all; cylinders) in [0, L), [-L/2, L/2) and with coordinates
    spilling over both box edges: host columns, then DeviceArray columns of float32 and of float64.  That the cases are no
    degenerate ones is asserted on the statement in test_groups_host.py and, for the frame at hand, below"""
    from test_pairs_weighted_gpu import _frame

    from abacusutils_amd import _lib
    cols = catalogue(kind)
    if frame == 0.0:
        want = judged(kind, b_perp, b_par)
    else:
        cols = _frame(cols, frame, BOX, 1)
        want = st.groups(*cols, BOX, b_perp, b_par)
    size = sizes_of(want[0])
    if kind == 'uniform' and b_par is None:
        assert (size == 1).sum() > len(size) // 2 if b_perp == 2.5 else size.max() > len(size) // 2
    else:
        assert (size == 1).sum() > 0 and (size >= 3).sum() > 0
    _check(cols, BOX, b_perp, b_par, want=want)
    for dt in (np.float32, np.float64):
        dev = [_lib.DeviceArray(np.ascontiguousarray(c, dtype=dt)) for c in cols]
        try:
            _check(dev, BOX, b_perp, b_par, want=want)
        finally:
            for a in dev:
                a.free()
    with pytest.raises(TypeError):
        d = _lib.DeviceArray(np.ascontiguousarray(cols[0], dtype=np.float32))
        try:
            _device([d, cols[1], cols[2]], BOX, b_perp, b_par)
        finally:
            d.free()


def winding_line(n, box, b, seed, cut=None):
    """n points 0.9 b apart (a little more: the line climbs) on a line along x that winds through the periodic x face, every
    winding 2 b further in y, so that only neighbours along the line are friends; handed over in a random permutation.  `cut`:
    that point of the line is left out, which opens a gap of 1.8 b.  Returns (columns, labels expected): the smallest index of
    the permuted order on either side of the cut."""
    s = np.arange(n) * 0.9 * b
    x, y, z = s % box, 1.0 + s / box * 2.0 * b, np.full(n, 0.25 * box)
    assert y.max() < box - 3.0 * b                   # the first and the last winding do not meet through the y face
    along = np.arange(n)
    if cut is not None:
        keep = along != cut
        x, y, z, along = x[keep], y[keep], z[keep], along[keep]
    perm = np.random.default_rng(seed).permutation(len(x))
    x, y, z, along = x[perm], y[perm], z[perm], along[perm]
    side = np.zeros(len(x), bool) if cut is None else along > cut
    labels = np.zeros(len(x), np.uint32)
    for sd in (False, True):
        if (side == sd).any():
            labels[side == sd] = np.flatnonzero(side == sd).min()
    return [x, y, z], labels


def test_the_deepest_tree():
    """5000 points on one line through the periodic face, in random order: one group, labelled 0; with one link cut, exactly two"""
    cols, expect = winding_line(5000, 100.0, 1.0, 71)
    res = _check(cols, 100.0, 1.0, nmax=8000)
    assert not res['labels'].any() and not expect.any() and res['ngroups'] == 1 and res['mult'][5000] == 1
    cols, expect = winding_line(5000, 100.0, 1.0, 72, cut=3210)
    res = _check(cols, 100.0, 1.0, nmax=8000)
    np.testing.assert_array_equal(res['labels'], expect)
    assert res['ngroups'] == 2 and res['mult'][3210] == 1 and res['mult'][1789] == 1


def test_the_deepest_tree_on_both_sort_paths(options):
    """the same line with 250 000 points, above the switch to the radix sort, and the counting sort on the same input
    (pairs_countsort): the statement's n^2 pairs are out of reach here, but the answer is known - the line is built so that only
    neighbours along it are friends (the 5000-point form above is held to the statement) - and both paths must give it"""
    from abacusutils_amd.analysis.groups import fof_groups, last_stats
    n, b = 250000, 0.14
    for cut in (None, 123456):
        cols, expect = winding_line(n, 100.0, b, 73, cut=cut)
        m = len(expect)
        radix = fof_groups(*cols, 100.0, b, nmax=8)
        links = last_stats()['links']
        options.set('pairs_countsort')
        counting = fof_groups(*cols, 100.0, b, nmax=8)
        assert last_stats()['links'] == links == m - (1 if cut is None else 2)
        options.reset()
        for res in (radix, counting):
            np.testing.assert_array_equal(res['labels'], expect)
            assert res['ngroups'] == (1 if cut is None else 2) and res['mult'][8] == res['ngroups'] and res['mult'].sum() == res['ngroups']


@pytest.mark.parametrize('b_perp,b_par', [(2.0, None), (0.05, None), (0.05, 0.3)])
def test_a_crowded_cell(b_perp, b_par):
    """700 points inside one cell of the grid - three slices of one workgroup; at b = 2 every pair of them is a friend pair, a
    quarter of a million unions on one tree, at b = 0.05 they fall into many groups - with exact twins among them, and 400
    uniform points elsewhere"""
    rng = np.random.default_rng(43)
    blob = 11.0 + 0.7 * rng.random((700, 3))              # [11, 11.7) in every dimension
    blob[600:] = blob[:100]                               # twins
    rest = rng.random((400, 3)) * 100.0
    p = np.concatenate([blob, rest])[rng.permutation(1100)]
    cols = [p[:, d].copy() for d in range(3)]
    for nc in (49, 128):                                  # the cells per dimension at b = 2 and at b = 0.05 or 0.3 (capped): one cell
        assert np.floor(11.0 * nc / 100.0) == np.floor(11.6999 * nc / 100.0)
    res = _check(cols, 100.0, b_perp, b_par, nmax=1024)
    size = sizes_of(res['labels'])
    assert size.max() >= 700 if b_perp == 2.0 else (size.max() > 4 and (size == 1).sum() > 100)


@pytest.mark.parametrize('b_perp,b_par', [(40.0, None), (50.0, None), (40.0, 50.0), (3.0, 40.0), (40.0, 3.0)])
def test_one_cell_per_dimension(b_perp, b_par):
    """b = 0.4 L and b exactly L / 2: fewer than three cells fit, every dimension is one cell that is its own neighbour - every
    pair must still be taken once; and grids that are one cell in xy or in z only"""
    cols = _uniform(1500, 100.0, 21)
    _check(cols, 100.0, b_perp, b_par, nmax=2000)


def test_small_n_and_no_labels():
    none = [np.zeros(0) for _ in range(3)]
    res = _check(none, 100.0, 1.0, nmax=4)
    assert res['labels'].shape == (0,) and res['ngroups'] == 0 and not res['mult'].any()
    for b_par in (None, 2.0):
        res = _check([[5.0], [6.0], [7.0]], 100.0, 1.0, b_par, nmax=4)
        np.testing.assert_array_equal(res['mult'], [0, 1, 0, 0, 0])
        assert res['ngroups'] == 1 and list(res['labels']) == [0]
        res = _check([[5.0, 5.5], [6.0, 6.0], [7.0, 7.0]], 100.0, 1.0, b_par, nmax=4)        # friends
        np.testing.assert_array_equal(res['mult'], [0, 0, 1, 0, 0])
        assert list(res['labels']) == [0, 0]
        res = _check([[5.0, 6.5], [6.0, 6.0], [7.0, 7.0]], 100.0, 1.0, b_par, nmax=4)        # not friends
        np.testing.assert_array_equal(res['mult'], [0, 2, 0, 0, 0])
        assert list(res['labels']) == [0, 1]
        res = _check([[99.75, 0.25], [6.0, 6.0], [0.25, 99.75]], 100.0, 1.0, b_par, nmax=4)  # friends through two faces
        assert list(res['labels']) == [0, 0]
    # nmax = 1: everything lands in the open bin
    res = _check(catalogue('clustered'), BOX, 1.0, nmax=1, want=judged('clustered', 1.0, None))
    np.testing.assert_array_equal(res['mult'], [0, res['ngroups']])
    # the largest nmax the LDS histogram takes
    res = _check(catalogue('clustered'), BOX, 2.0, nmax=8191, want=judged('clustered', 2.0, None))
    assert res['mult'][120] == 1 and not res['mult'][121:].any()


def test_the_upper_edge_is_strict():
    for b_par in (None, 3.0):
        assert _check([[0.0, 1.5], [0.0, 0.0], [0.0, 0.0]], 100.0, 1.5, b_par)['ngroups'] == 2
        assert _check([[0.0, 1.4999999], [0.0, 0.0], [0.0, 0.0]], 100.0, 1.5, b_par)['ngroups'] == 1
    assert _check([[0.0, 0.5], [0.0, 0.0], [0.0, 3.0]], 100.0, 1.5, 3.0)['ngroups'] == 2
    assert _check([[0.0, 0.5], [0.0, 0.0], [0.0, 2.9999998]], 100.0, 1.5, 3.0)['ngroups'] == 1


def test_two_calls_give_identical_arrays():
    """the unions race, the counting sort hands out slots by atomics: the labels do not depend on either"""
    from abacusutils_amd.analysis.groups import fof_groups
    cols = catalogue('clustered')
    first = fof_groups(*cols, BOX, 2.0, b_par=6.0)
    second = fof_groups(*cols, BOX, 2.0, b_par=6.0)
    np.testing.assert_array_equal(first['labels'], second['labels'])
    np.testing.assert_array_equal(first['mult'], second['mult'])
    assert first['ngroups'] == second['ngroups']
    np.testing.assert_array_equal(first['labels'], judged('clustered', 2.0, 6.0)[0])


def test_abacus_hod_groups():
    """AbacusHOD.compute_groups: the catalogue still in HBM gives what its host columns give"""
    from test_abacus_hod_gpu import CLUSTERING, HOD_PARAMS

    from abacusutils_amd import synth
    from abacusutils_amd.analysis.groups import fof_groups, linking_lengths
    from abacusutils_amd.hod.abacus_hod import AbacusHOD
    hd, pd, params = synth.synth_hod_inputs(100000, 100000, seed=19, lbox=1000.0)
    hod = dict(HOD_PARAMS, LRG_params=dict(synth.LRG_PARAMS, logM_cut=12.3, logM1=13.3), ELG_params=dict(synth.ELG_PARAMS))
    ball = AbacusHOD.from_arrays(hd, pd, params, hod, CLUSTERING)
    mock = ball.run_hod()
    assert all(mock.device_xyz(tr) is not None for tr in mock)
    plain = {tr: dict(mock[tr]) for tr in mock}
    for cyl in (False, True):
        for tr in mock:
            n = len(plain[tr]['x'])
            bp, bl = linking_lengths(n, ball.lbox, 0.2, 1.0)
            kw = dict(b_par=bl if cyl else None, nmax=32)
            got = ball.compute_groups(mock, bp, return_labels=True, **kw)[tr]
            want = ball.compute_groups(plain, bp, return_labels=True, **kw)[tr]
            direct = fof_groups(*[np.asarray(plain[tr][c]) for c in 'xyz'], ball.lbox, bp, **kw)
            for other in (want, direct):
                np.testing.assert_array_equal(got['labels'], other['labels'])
                np.testing.assert_array_equal(got['mult'], other['mult'])
                assert got['ngroups'] == other['ngroups'] and got['n'] == other['n'] == n
            assert got['mult'][1] > 0 and got['mult'][2:].sum() > 0 and got['mult'].sum() == got['ngroups']
    bare = ball.compute_groups(mock, bp)
    assert set(bare) == set(mock) and all(v['labels'] is None for v in bare.values())
