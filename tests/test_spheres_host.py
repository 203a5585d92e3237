"""Counts in spheres without a GPU: the NumPy statement tests/spheres_statement.py against the oracle's pair counter (its
column sums are the cumulative pair counts), its edge conventions, the arithmetic of vpf / knn_cdf on a given histogram, and
every validation rule of abacus_spherecount[_dev] - refused before the device is touched."""
import ctypes as C
import functools

import numpy as np
import pytest
from spheres_statement import count_in_spheres as statement

BOX = 200.0
RADII = np.logspace(np.log10(2.0), np.log10(30.0), 12).astype(np.float32)
KMAX = 16
CASES = [(pimax, own) for pimax in (None, 20.0) for own in (False, True)]
CASE_IDS = [f'{"cyl" if p else "sph"}-{"data" if own else "random"}' for p, own in CASES]


@functools.lru_cache(maxsize=None)
def catalogue():
    """3000 clustered data points (seed 11) and 1000 uniform queries (seed 5) in a box of 200"""
    from test_pairs_weighted_gpu import _points
    return _points(3000, BOX, 11), _points(1000, BOX, 5, clustered=False)


@functools.lru_cache(maxsize=None)
def judged(pimax, own):
    """(hist, counts) of the statement for one of the four cases; computed once, shared, read-only"""
    data, queries = catalogue()
    hist, counts = statement(*data, BOX, RADII, *((None,) * 3 if own else queries), pimax=pimax, kmax=KMAX)
    hist.setflags(write=False), counts.setflags(write=False)
    return hist, counts


@pytest.mark.parametrize('pimax,own', CASES, ids=CASE_IDS)
def test_statement_sums_to_the_oracle_pair_counts(pimax, own):
    """counts.sum(axis=0) == cumsum of oracle.paircount_brute over the edges (0, r_1 .. r_nr): N(<r) with a strict upper edge is
    the cumulative [lo, hi) pair count; and the case is no degenerate one"""
    from oracle import oracle
    data, queries = catalogue()
    hist, counts = judged(pimax, own)
    edges = np.concatenate([[0.0], RADII]).astype(np.float32)
    second = (None,) * 3 if own else data          # set 1 of the pair counter: the queries
    first = data if own else queries
    kw = dict(pimax=pimax, npibins=1) if pimax else {}
    pairs = oracle.paircount_brute('rppi' if pimax else 'r', *first, BOX, edges, *second, nthread=oracle.max_threads(), **kw)
    np.testing.assert_array_equal(counts.sum(axis=0, dtype=np.uint64), np.cumsum(pairs.ravel()))
    assert np.all(hist.sum(axis=1) == counts.shape[0]) and counts.shape == ((3000 if own else 1000), len(RADII))
    rich = int(((hist > 0).sum(axis=1) >= 3).sum())
    print(f'{rich} of {len(RADII)} radii with at least 3 non-empty columns')
    assert rich >= 7
    assert hist[:, 0].sum() > 0 and hist[:, KMAX].sum() > 0


def test_the_upper_edge_is_strict():
    """a query at the origin, a data point at (3, 4, 0): r2 = 25 exactly; radius 5 does not contain it, the next float32 does"""
    up = np.nextafter(np.float32(5.0), np.float32(np.inf))
    for pimax in (None, 1.0):
        hist, counts = statement([3.0], [4.0], [0.0], 100.0, [5.0, up], [0.0], [0.0], [0.0], pimax=pimax, kmax=2)
        np.testing.assert_array_equal(counts, [[0, 1]])
        np.testing.assert_array_equal(hist, [[1, 0, 0], [0, 1, 0]])
    # and |dz| < pimax is strict too
    _, counts = statement([3.0], [4.0], [1.0], 100.0, [6.0], [0.0], [0.0], [0.0], pimax=1.0, kmax=2)
    assert counts[0, 0] == 0


def test_a_twin_counts_and_self_does_not():
    x, y, z = [10.0, 10.0, 50.0], [20.0, 20.0, 50.0], [30.0, 30.0, 50.0]
    hist, counts = statement(x, y, z, 100.0, [1.0], kmax=2)
    np.testing.assert_array_equal(counts[:, 0], [1, 1, 0])
    np.testing.assert_array_equal(hist, [[1, 2, 0]])


def test_empty_sets():
    hist, counts = statement([], [], [], 100.0, [1.0, 2.0], [1.0, 2.0], [1.0, 2.0], [1.0, 2.0], kmax=3)
    np.testing.assert_array_equal(hist, [[2, 0, 0, 0], [2, 0, 0, 0]])
    assert counts.shape == (2, 2) and not counts.any()
    hist, counts = statement([1.0], [1.0], [1.0], 100.0, [1.0], [], [], [], kmax=3)
    assert not hist.any() and counts.shape == (0, 1)


def test_vpf_and_knn_arithmetic_on_a_given_histogram():
    """1024 queries (a power of two: every probability is a dyadic rational and every sum below exact).  rows of pN plus the
    saturated share sum to 1, and CDF_k = 1 - sum_{j<k} pN_j"""
    from abacusutils_amd.analysis.spheres import cdf_from_hist, pn_from_hist
    rng = np.random.default_rng(8)
    nq, kmax, nr = 1024, 6, 5
    counts = rng.integers(0, 10, (nq, nr))
    hist = np.array([np.bincount(np.minimum(counts[:, j], kmax), minlength=kmax + 1) for j in range(nr)], dtype=np.uint64)
    pn = pn_from_hist(hist, nq, kmax)
    assert pn.shape == (nr, kmax) and pn.dtype == np.float64
    np.testing.assert_array_equal(pn.sum(axis=1) + hist[:, kmax] / nq, np.ones(nr))
    np.testing.assert_array_equal(pn[:, 0], (counts == 0).mean(axis=0))
    ks = [1, 2, 6]
    cdf = cdf_from_hist(hist, nq, ks)
    assert cdf.shape == (len(ks), nr)
    for i, k in enumerate(ks):
        np.testing.assert_array_equal(cdf[i], 1.0 - pn[:, :k].sum(axis=1))
        np.testing.assert_array_equal(cdf[i], (counts >= k).mean(axis=0))
    with pytest.raises(ValueError):
        cdf_from_hist(hist, nq, [kmax + 1])
    with pytest.raises(ValueError):
        pn_from_hist(hist, nq, kmax + 1)


def test_random_centres_and_the_wrappers_arguments():
    from abacusutils_amd.analysis import spheres as S
    a, b = S.random_centres(100, 50.0, 3), S.random_centres(100, 50.0, 3)
    want = np.random.default_rng(3).random((100, 3)) * 50.0
    for d in range(3):
        assert a[d].dtype == np.float32 and a[d].flags.c_contiguous
        np.testing.assert_array_equal(a[d], b[d])
        np.testing.assert_array_equal(a[d], want[:, d].astype(np.float32))
    x = np.zeros(4)
    with pytest.raises(NotImplementedError):
        S.vpf(10.0, 4, 100, 3, 1, x, x, x, periodic=False, boxsize=100.0)
    with pytest.raises(NotImplementedError):
        S.vpf(10.0, 4, 100, 3, 1, x, x, x)
    with pytest.raises(ValueError, match='not both'):
        S.knn_cdf(x, x, x, 100.0, [1.0], [1], QX=x, QY=x, QZ=x, nquery=10, seed=1)
    with pytest.raises(ValueError, match='nquery and seed'):
        S.knn_cdf(x, x, x, 100.0, [1.0], [1], nquery=10)
    with pytest.raises(ValueError, match='positive'):
        S.knn_cdf(x, x, x, 100.0, [1.0], [0])


def test_argument_validation_happens_before_the_device():
    """every rule of include/abacus_hip.h raises through the Python entry on a machine without a device, and the message
    starts with the entry's name"""
    from abacusutils_amd import _lib
    from abacusutils_amd.analysis.spheres import count_in_spheres
    x = np.linspace(1.0, 9.0, 4)
    ok = dict(boxsize=100.0, radii=[1.0, 2.0])
    bad = [dict(ok, radii=[]), dict(ok, radii=np.arange(1, 34) * 0.5),                       # 1 <= nr <= 32
           dict(ok, kmax=0), dict(ok, radii=np.arange(1, 33) * 0.5, kmax=256),               # kmax >= 1; nr (kmax + 1) <= 8192
           dict(ok, radii=[0.0, 1.0]), dict(ok, radii=[-1.0, 1.0]), dict(ok, radii=[np.nan]),
           dict(ok, radii=[1.0, 1.0]), dict(ok, radii=[2.0, 1.0]),                           # positive and increasing
           dict(ok, radii=[1.0, 50.5]), dict(ok, pimax=50.5), dict(ok, boxsize=0.0)]         # r_nr, pimax <= L / 2
    for kw in bad:
        for q in ((), (x, x, x)):
            with pytest.raises(_lib.AbacusHipError, match=r'^abacus_spherecount: '):
                count_in_spheres(x, x, x, kw['boxsize'], kw['radii'], *q, **{k: v for k, v in kw.items() if k not in ('boxsize', 'radii')})
    with pytest.raises(ValueError):
        count_in_spheres(x, x, x, 100.0, [1.0], pimax=0.0)
    with pytest.raises(ValueError):
        count_in_spheres(x, x, x, 100.0, [1.0], QX=x)
    with pytest.raises(ValueError):
        count_in_spheres(x, x, x[:3], 100.0, [1.0])
    # what the Python entry cannot express, through the C entries themselves: point counts, null arguments, pos_dtype
    L = _lib.lib()
    f = np.zeros(4, np.float32)
    r = np.array([1.0, 2.0], np.float32)
    hist = np.zeros(2 * 9, np.uint64)
    p, n4, big = _lib.ptr, C.c_int64(4), C.c_int64(1 << 31)
    tail = (C.c_float(100.0), p(r), 2, C.c_float(0.0), 8, p(hist), None)

    def refused(rc, name='abacus_spherecount'):
        assert rc != 0 and L.abacus_last_error().decode().startswith(name + ': ')
    refused(L.abacus_spherecount(p(f), p(f), p(f), big, None, None, None, C.c_int64(0), *tail))
    refused(L.abacus_spherecount(p(f), p(f), p(f), C.c_int64(-1), None, None, None, C.c_int64(0), *tail))
    refused(L.abacus_spherecount(p(f), p(f), p(f), n4, p(f), p(f), p(f), big, *tail))
    refused(L.abacus_spherecount(None, p(f), p(f), n4, None, None, None, C.c_int64(0), *tail))
    refused(L.abacus_spherecount(p(f), p(f), None, n4, None, None, None, C.c_int64(0), *tail))
    refused(L.abacus_spherecount(p(f), p(f), p(f), n4, p(f), None, p(f), n4, *tail))
    refused(L.abacus_spherecount(p(f), p(f), p(f), n4, None, None, None, C.c_int64(0), C.c_float(100.0), None, 2, C.c_float(0.0), 8, p(hist), None))
    refused(L.abacus_spherecount(p(f), p(f), p(f), n4, None, None, None, C.c_int64(0), C.c_float(100.0), p(r), 2, C.c_float(0.0), 8, None, None))
    refused(L.abacus_spherecount(p(f), p(f), p(f), n4, None, None, None, C.c_int64(0), C.c_float(100.0), p(r), 2, C.c_float(-1.0), 8, p(hist), None))
    # the resident form: the host arrays stand in for device pointers - a refused call reads none of them
    refused(L.abacus_spherecount_dev(p(f), p(f), p(f), n4, None, None, None, C.c_int64(0), 7, *tail), 'abacus_spherecount_dev')
    refused(L.abacus_spherecount_dev(p(f), p(f), p(f), big, None, None, None, C.c_int64(0), 0, *tail), 'abacus_spherecount_dev')
    assert not hist.any()
