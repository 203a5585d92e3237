"""Counts in spheres on the device (csrc/spheres.hip: sphere_count, C ABI abacus_spherecount[_dev]; analysis/spheres.py)
against the NumPy statement tests/spheres_statement.py.  Needs an MI355X: run with `-m gpu`.  Every comparison is between
integers and exact."""
import functools

import numpy as np
import pytest
from spheres_statement import count_in_spheres as statement
from test_spheres_host import BOX, CASE_IDS, CASES, KMAX, RADII, catalogue, judged

pytestmark = pytest.mark.gpu


def _device(data, queries, box, radii, pimax=None, kmax=8):
    """the device's hist and counts; without the counts the histogram is what it was"""
    from abacusutils_amd.analysis.spheres import count_in_spheres
    q = (None,) * 3 if queries is None else queries
    res = count_in_spheres(*data, box, radii, *q, pimax=pimax, kmax=kmax, return_counts=True)
    bare = count_in_spheres(*data, box, radii, *q, pimax=pimax, kmax=kmax)
    assert bare['counts'] is None and bare['nquery'] == res['nquery'] == len(res['counts'])
    np.testing.assert_array_equal(bare['hist'], res['hist'])
    return res['hist'], res['counts']


def _check(data, queries, box, radii, pimax=None, kmax=8, want=None):
    hist_s, counts_s = want if want is not None else statement(*data, box, radii, *((None,) * 3 if queries is None else queries),
                                                               pimax=pimax, kmax=kmax)
    hist, counts = _device(data, queries, box, radii, pimax, kmax)
    assert hist.dtype == np.uint64 and counts.dtype == np.uint32
    np.testing.assert_array_equal(counts, counts_s)
    np.testing.assert_array_equal(hist, hist_s)
    return hist, counts


def _uniform(n, box, seed):
    p = np.random.default_rng(seed).random((n, 3)) * box
    return [p[:, d].copy() for d in range(3)]


@functools.lru_cache(maxsize=None)
def _framed(frame):
    from test_pairs_weighted_gpu import _frame
    data, queries = catalogue()
    if frame == 0.0:
        return data, queries
    return _frame(data, frame, BOX, 1), _frame(queries, frame, BOX, 4)


@pytest.mark.parametrize('frame', [0.0, -100.0, 'unwrapped'])
@pytest.mark.parametrize('pimax,own', CASES, ids=CASE_IDS)
def test_statement_cases_in_every_frame(pimax, own, frame):
    """the four host cases in [0, L), [-L/2, L/2) and with coordinates spilling over both box edges: host columns, then
    DeviceArray columns of float32 and of float64"""
    from abacusutils_amd import _lib
    data, queries = _framed(frame)
    q = None if own else queries
    want = judged(pimax, own) if frame == 0.0 else statement(*data, BOX, RADII, *((None,) * 3 if own else queries), pimax=pimax, kmax=KMAX)
    hist, _ = _check(data, q, BOX, RADII, pimax, KMAX, want=want)
    assert hist[:, 0].sum() > 0 and hist[:, KMAX].sum() > 0
    for dt in (np.float32, np.float64):
        dd = [_lib.DeviceArray(np.ascontiguousarray(c, dtype=dt)) for c in data]
        dq = None if own else [_lib.DeviceArray(np.ascontiguousarray(c, dtype=dt)) for c in queries]
        try:
            _check(dd, dq, BOX, RADII, pimax, KMAX, want=want)
            if not own:      # host queries next to resident data: uploaded in the data's dtype
                _check(dd, queries, BOX, RADII, pimax, KMAX, want=want)
        finally:
            for a in dd + (dq or []):
                a.free()
    if not own:
        with pytest.raises(TypeError):
            _device(data, [_lib.DeviceArray(np.ascontiguousarray(c, dtype=np.float32)) for c in queries], BOX, RADII)


@pytest.mark.parametrize('pimax', [None, 40.0])
@pytest.mark.parametrize('own', [False, True])
def test_one_cell_per_dimension(own, pimax):
    """r_max = 0.4 L: fewer than three cells fit, every dimension is one cell that is its own neighbour"""
    data, queries = _uniform(1500, 100.0, 21), _uniform(300, 100.0, 22)
    _check(data, None if own else queries, 100.0, np.linspace(4.0, 40.0, 10), pimax, kmax=40)


@pytest.mark.parametrize('pimax', [None, 50.0])
def test_radius_of_half_the_box(pimax):
    data, queries = _uniform(1200, 100.0, 23), _uniform(200, 100.0, 24)
    _check(data, queries, 100.0, [10.0, 30.0, 50.0], pimax, kmax=100)
    _check(data, None, 100.0, [10.0, 30.0, 50.0], pimax, kmax=100)


@pytest.mark.parametrize('nq', [1, 255, 257])
def test_query_counts_around_a_slice(nq):
    data = catalogue()[0]
    _check(data, _uniform(nq, BOX, 30 + nq), BOX, RADII, kmax=KMAX)


def test_many_queries_in_one_cell():
    """600 queries inside one cell of the grid: three slices of one workgroup, and their rows return in the caller's order"""
    data = catalogue()[0]
    q = [10.0 + 2.0 * c / BOX for c in _uniform(600, BOX, 41)]        # all in [10, 12)^3, a cell is 33 wide
    _, counts = _check(data, q, BOX, RADII, kmax=KMAX)
    assert len(np.unique(counts, axis=0)) > 50                          # rows differ: a permutation would show


def test_a_crowded_and_an_empty_neighbourhood():
    """more than 256 data points around one query (several rounds of candidates, counts above any lane's share) and none around another"""
    rng = np.random.default_rng(43)
    blob = 50.0 + rng.normal(0, 0.5, (700, 3))
    far = 150.0 + 40.0 * (rng.random((300, 3)) - 0.5)
    far = far[np.linalg.norm(far - 150.0, axis=1) > 12.0]
    p = np.concatenate([blob, far])
    data = [p[:, d].copy() for d in range(3)]
    queries = [np.array([50.0, 150.0]) for _ in range(3)]
    hist, counts = _check(data, queries, 200.0, [1.0, 3.0, 10.0], kmax=600)
    assert counts[0, 2] == 700 and counts[0, 0] > 256 and not counts[1].any()
    assert hist[2, 600] == 1 and hist[2, 0] == 1
    _check(data, queries, 200.0, [1.0, 3.0, 10.0], pimax=5.0, kmax=600)


def test_empty_sets():
    q = _uniform(10, 100.0, 51)
    none = [np.zeros(0) for _ in range(3)]
    hist, counts = _check(none, q, 100.0, [1.0, 2.0], kmax=3)
    np.testing.assert_array_equal(hist[:, 0], [10, 10])
    assert not counts.any() and counts.shape == (10, 2)
    hist, counts = _check(q, none, 100.0, [1.0, 2.0], kmax=3)
    assert not hist.any() and counts.shape == (0, 2)
    hist, counts = _check(none, None, 100.0, [1.0, 2.0], kmax=3)
    assert not hist.any() and counts.shape == (0, 2)


@pytest.mark.parametrize('nr,kmax', [(1, 1), (1, 8), (32, 1), (32, 255)])
def test_extreme_radii_and_kmax(nr, kmax):
    """one radius and 32; kmax = 1 and the largest that 32 radii allow (32 * 256 = 8192 histogram entries)"""
    data, queries = catalogue()
    radii = [30.0] if nr == 1 else np.logspace(0.0, np.log10(30.0), 32)
    hist, _ = _check(data, queries, BOX, radii, kmax=kmax)
    assert hist.shape == (nr, kmax + 1)
    _check(data, None, BOX, radii, pimax=10.0, kmax=kmax)


def test_a_duplicated_point_counts_its_twin():
    data = [c.copy() for c in catalogue()[0]]
    for c in data:
        c[17] = c[2500]
    _, counts = _check(data, None, BOX, RADII, kmax=KMAX)
    lone = statement(*[np.delete(c, 17) for c in data], BOX, RADII, kmax=KMAX)[1]
    np.testing.assert_array_equal(counts[2500], lone[2499] + 1)          # the twin, at distance 0, inside every radius
    np.testing.assert_array_equal(counts[17], counts[2500])


def test_strict_upper_edge():
    up = np.nextafter(np.float32(5.0), np.float32(np.inf))
    for pimax in (None, 1.0):
        _, counts = _check([[3.0], [4.0], [0.0]], [[0.0], [0.0], [0.0]], 100.0, [5.0, up], pimax, kmax=2)
        np.testing.assert_array_equal(counts, [[0, 1]])


def test_both_sort_paths(options):
    """250 000 points in each set: the radix sort carries the caller's index of a query, and so does the counting sort
    (pairs_countsort); both give the same rows, whose sums are the oracle's cumulative cross counts"""
    from abacusutils_amd.analysis.spheres import count_in_spheres
    from oracle import oracle
    box, radii = 1000.0, np.linspace(2.5, 20.0, 8).astype(np.float32)
    data, queries = _uniform(250000, box, 61), _uniform(250000, box, 62)
    radix = count_in_spheres(*data, box, radii, *queries, kmax=8, return_counts=True)
    options.set('pairs_countsort')
    counting = count_in_spheres(*data, box, radii, *queries, kmax=8, return_counts=True)
    options.reset()
    np.testing.assert_array_equal(radix['hist'], counting['hist'])
    np.testing.assert_array_equal(radix['counts'], counting['counts'])
    edges = np.concatenate([[0.0], radii]).astype(np.float32)
    pairs = oracle.paircount_cells('r', *queries, box, edges, *data, nthread=oracle.max_threads())
    np.testing.assert_array_equal(radix['counts'].sum(axis=0, dtype=np.uint64), np.cumsum(pairs.ravel()))
    # the rows belong to their queries: a sample of them against the statement
    pick = np.arange(0, 250000, 6250)
    want = statement(*data, box, radii, *[c[pick] for c in queries], kmax=8)[1]
    np.testing.assert_array_equal(radix['counts'][pick], want)
    kmax = 8
    for j in range(len(radii)):
        np.testing.assert_array_equal(radix['hist'][j], np.bincount(np.minimum(radix['counts'][:, j], kmax), minlength=kmax + 1))


def test_abacus_hod_vpf_and_knn():
    """AbacusHOD.compute_vpf / compute_knn: the catalogue still in HBM gives what its host columns give, and '{a}_{a}' is
    knn_cdf with the data as queries"""
    from test_abacus_hod_gpu import CLUSTERING, HOD_PARAMS

    from abacusutils_amd import synth
    from abacusutils_amd.analysis.spheres import knn_cdf, vpf
    from abacusutils_amd.hod.abacus_hod import AbacusHOD
    hd, pd, params = synth.synth_hod_inputs(100000, 100000, seed=19, lbox=1000.0)
    hod = dict(HOD_PARAMS, LRG_params=dict(synth.LRG_PARAMS, logM_cut=12.3, logM1=13.3), ELG_params=dict(synth.ELG_PARAMS))
    ball = AbacusHOD.from_arrays(hd, pd, params, hod, CLUSTERING)
    mock = ball.run_hod()
    assert all(mock.device_xyz(tr) is not None for tr in mock)
    plain = {tr: dict(mock[tr]) for tr in mock}
    radii, ks = np.logspace(0.5, 1.5, 6), [1, 2, 4]
    got_v, want_v = ball.compute_vpf(mock, 40.0, 5, 3000, numpN=4, seed=7), ball.compute_vpf(plain, 40.0, 5, 3000, numpN=4, seed=7)
    assert set(got_v) == set(want_v) == set(mock)
    for tr in mock:
        np.testing.assert_array_equal(got_v[tr], want_v[tr])
        xyz = [np.asarray(plain[tr][c]) for c in 'xyz']
        np.testing.assert_array_equal(got_v[tr], vpf(40.0, 5, 3000, 4, 7, *xyz, boxsize=ball.lbox))
        assert got_v[tr]['pN'].shape == (5, 4) and 0 < got_v[tr]['pN'][0, 0] <= 1 and np.all(np.diff(got_v[tr]['pN'][:, 0]) <= 0)
    for pimax in (None, 20.0):
        got = ball.compute_knn(mock, radii, ks, 3000, seed=7, pimax=pimax, data_queries=True)
        want = ball.compute_knn(plain, radii, ks, 3000, seed=7, pimax=pimax, data_queries=True)
        assert set(got) == set(want) == set(mock) | {a + '_' + b for a in mock for b in mock}
        for k in want:
            assert got[k].shape == (len(ks), len(radii))
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
        for tr in mock:
            xyz = [np.asarray(plain[tr][c]) for c in 'xyz']
            np.testing.assert_array_equal(got[tr + '_' + tr], knn_cdf(*xyz, ball.lbox, radii, ks, pimax=pimax))
            assert np.all(np.diff(got[tr], axis=1) >= 0) and np.all(np.diff(got[tr], axis=0) <= 0)
