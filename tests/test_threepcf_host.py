"""The 3PCF multipoles without a GPU: the two NumPy statements of tests/threepcf_statement.py against each other (the algorithm in
float64 against the brute-force sum over triplets), the statement's pair counts against the oracle's brute-force counter, known
answers, the normalisation of analysis/threepcf.py, and every validation rule of abacus_threepcf[_dev] - refused before the
device is touched."""
import ctypes as C
import functools

import numpy as np
import pytest
import threepcf_statement as st

BOX = 100.0
EDGES = np.linspace(2.0, 25.0, 6)
LMAX = 10


@functools.lru_cache(maxsize=None)
def uniform(n, box=BOX, seed=1):
    p = np.random.default_rng(seed).random((n, 3)) * box
    cols = tuple(np.ascontiguousarray(p[:, d], dtype=np.float32) for d in range(3))
    for c in cols:
        c.setflags(write=False)
    return cols


@functools.lru_cache(maxsize=None)
def dr_weights(n=400):
    """a third of the points at weight 1 (the data), the rest at -N_D / N_R (the randoms)"""
    nd = n // 3
    w = np.full(n, -nd / (n - nd), dtype=np.float32)
    w[:nd] = 1.0
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def judged(weighted, form='harmonic', dtype='float64'):
    """the statement on the 400-point shape; computed once, shared, read-only"""
    fn = st.brute if form == 'brute' else functools.partial(st.harmonic, dtype=np.dtype(dtype).type)
    out = fn(*uniform(400), BOX, EDGES, LMAX, w=dr_weights() if weighted else None)
    for v in out.values():
        v.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------- 1. harmonic against brute
@pytest.mark.parametrize('weighted', [False, True], ids=['unit', 'd-r'])
def test_harmonic_equals_brute(weighted):
    """max error over max |want| per l below 1e-11 (a prototype gave 4e-15 to 6e-14), self-term subtraction included"""
    want, got = judged(weighted, 'brute'), judged(weighted)
    for l in range(LMAX + 1):
        scale = np.abs(want['zeta'][l]).max()
        assert scale > 0
        err = np.abs(got['zeta'][l] - want['zeta'][l]).max() / scale
        print(f'l = {l}: {err:.3g}')
        assert err < 1e-11, (l, err)
    np.testing.assert_allclose(got['wself'], want['wself'], rtol=1e-13)
    np.testing.assert_array_equal(got['npairs'], want['npairs'])
    for l in range(LMAX + 1):                       # both triangles
        np.testing.assert_array_equal(got['zeta'][l], got['zeta'][l].T)
    if not weighted:                                # unit weights: l = 0 counts triplets, wself pairs
        np.testing.assert_array_equal(got['wself'], got['npairs'].astype(np.float64))
        assert np.all(got['zeta'][0] == np.round(got['zeta'][0]))


# ------------------------------------------------------------------------------------------------- 2. pair counts
def test_npairs_is_the_oracle_pair_count():
    from oracle import oracle
    want = oracle.paircount_brute('r', *uniform(400), BOX, EDGES.astype(np.float32))
    np.testing.assert_array_equal(judged(False)['npairs'], want)
    assert want.min() > 100


# ------------------------------------------------------------------------------------------------- 3. known answers
def legendre(lmax, mu):
    P = [1.0, mu]
    for l in range(1, lmax):
        P.append(((2 * l + 1) * mu * P[l] - l * P[l - 1]) / (l + 1))
    return np.array(P[:lmax + 1])


def three_points():
    """a primary at (50, 50, 50), j at d = (1, 2, 2) (r = 3) and k at d = (-6, 2, -4) (r = 7.48): float32 holds them exactly;
    |jk| = 9.2 is outside the edges, so each of the other two primaries sees the first one alone: (columns, cos theta)"""
    dj, dk = np.array([1.0, 2.0, 2.0]), np.array([-6.0, 2.0, -4.0])
    p = np.array([[50.0, 50.0, 50.0], 50.0 + dj, 50.0 + dk])
    return [p[:, d].copy() for d in range(3)], dj @ dk / np.sqrt((dj @ dj) * (dk @ dk))


def check_three_points(fn, tol):
    cols, mu = three_points()
    assert np.linalg.norm([c[1] - c[2] for c in cols]) > 8.5
    edges3 = np.array([1.0, 4.0, 6.5, 8.0])          # j in bin 0, k in bin 2
    out = fn(*cols, BOX, edges3, 8)
    want = np.zeros((9, 3, 3))
    want[:, 0, 2] = want[:, 2, 0] = legendre(8, mu)
    np.testing.assert_allclose(out['zeta'], want, rtol=0, atol=tol)
    np.testing.assert_array_equal(out['npairs'], [2, 0, 2])
    np.testing.assert_allclose(out['wself'], [2.0, 0.0, 2.0], rtol=0, atol=tol)   # the primary's j, and j's primary (k likewise)
    return out


def check_twin(fn):
    """two points at one place: a pair of bin 0 (the first edge is 0) for the counter, but no direction - nothing in zeta or wself"""
    x = np.array([10.0, 10.0, 60.0])
    out = fn(x, x, x, BOX, np.array([0.0, 1.0, 2.0]), 3)
    np.testing.assert_array_equal(out['npairs'], [2, 0])
    assert not out['zeta'].any() and not out['wself'].any()
    return out


def check_small(fn):
    """lmax = 0 with one bin: zeta[0] = sum_i n_i (n_i - 1) for unit weights"""
    cols = uniform(60, seed=9)
    out = fn(*cols, BOX, np.array([5.0, 40.0]), 0)
    assert out['zeta'].shape == (1, 1, 1) and out['wself'].shape == (1,) and out['npairs'].dtype == np.uint64
    want = st.brute(*cols, BOX, np.array([5.0, 40.0]), 0)
    assert out['zeta'][0, 0, 0] == want['zeta'][0, 0, 0] > 0
    assert out['npairs'][0] == want['npairs'][0] == out['wself'][0]
    return out


@pytest.mark.parametrize('form', ['brute', 'harmonic'])
def test_known_answers(form):
    fn = getattr(st, form)
    check_three_points(fn, 1e-13)
    check_twin(fn)
    check_small(fn)
    out = fn([], [], [], BOX, EDGES, 2)
    assert out['zeta'].shape == (3, 5, 5) and not out['zeta'].any() and not out['npairs'].any()


def test_second_set_is_appended():
    cols, w = uniform(400), dr_weights()
    nd = 400 // 3
    out = st.harmonic(*[c[:nd] for c in cols], BOX, EDGES, 4, None, *[c[nd:] for c in cols], w[nd:])
    np.testing.assert_array_equal(out['zeta'], judged(True)['zeta'][:5])


# ------------------------------------------------------------------------------------------------- 4. normalisation
def test_zeta_from_counts_by_hand():
    from abacusutils_amd.analysis.threepcf import zeta_from_counts
    rng = np.random.default_rng(3)
    raw = rng.normal(size=(4, 3, 3))
    edges, W, L = np.array([1.0, 2.0, 4.0, 8.0]), 1234.5, 300.0
    got = zeta_from_counts(raw, W, L, edges)
    assert got.dtype == np.float64 and got.shape == raw.shape
    for l in range(4):
        for b1 in range(3):
            for b2 in range(3):
                V1 = 4.0 * np.pi / 3.0 * (edges[b1 + 1] ** 3 - edges[b1] ** 3)
                V2 = 4.0 * np.pi / 3.0 * (edges[b2 + 1] ** 3 - edges[b2] ** 3)
                want = (2 * l + 1) * raw[l, b1, b2] / (W * (W / L ** 3) ** 2 * V1 * V2)
                assert abs(got[l, b1, b2] - want) <= 1e-14 * abs(want)
    with pytest.raises(ValueError):
        zeta_from_counts(raw, W, L, edges[:3])


@pytest.mark.parametrize('seed', [1, 2, 3, 4, 5])
def test_natural_monopole_of_a_uniform_catalogue_is_one(seed):
    """3000 uniform points: the natural l = 0 estimate lies within 10 % of 1 in every bin pair (measured: at most 2.7 %; the cap
    only has to catch a wrong factor of 2 or 4 pi).  The raw l = 0 sums come from per-primary bin counts: with unit weights
    zeta[0][b1][b2] = sum_i n_i(b1) n_i(b2) - [b1 == b2] n_i(b1)"""
    from abacusutils_amd.analysis.threepcf import zeta_from_counts
    edges = np.array([8.0, 12.0, 16.0, 20.0])
    p, _ = st.catalogue(*uniform(3000, seed=seed))
    raw = np.zeros((1, 3, 3))
    for i, j, b, d, r2 in st.neighbours(p, BOX, edges):
        n = np.bincount(b, minlength=3).astype(np.float64)
        raw[0] += np.outer(n, n) - np.diag(n)
    z = zeta_from_counts(raw, 3000.0, BOX, edges)
    print(f'seed {seed}: natural monopole within {np.abs(z - 1).max():.3%} of 1')
    assert np.abs(z - 1).max() < 0.10


# ------------------------------------------------------------------------------------------------- 5. validation
def test_argument_validation_happens_before_the_device():
    """every rule of include/abacus_hip.h raises on a machine without a device, and the message starts with the entry's name"""
    from abacusutils_amd import _lib
    from abacusutils_amd.analysis.threepcf import calc_3pcf, triplet_multipoles
    x = np.linspace(1.0, 9.0, 4)
    ok = dict(boxsize=100.0, rbins=[1.0, 2.0, 3.0], lmax=2)
    bad = [dict(ok, rbins=[1.0]), dict(ok, rbins=np.arange(34) * 0.5),                       # 1 <= nbins <= 32
           dict(ok, lmax=-1), dict(ok, lmax=11),                                             # 0 <= lmax <= 10
           dict(ok, rbins=[-1.0, 1.0]), dict(ok, rbins=[np.nan, 1.0]), dict(ok, rbins=[1.0, 1.0]), dict(ok, rbins=[2.0, 1.0]),
           dict(ok, rbins=[1.0, np.nan]), dict(ok, rbins=[1.0, 50.5]),                       # non-negative, increasing, <= L / 2
           dict(ok, boxsize=0.0), dict(ok, boxsize=-100.0)]
    for kw in bad:
        for second in ({}, dict(X2=x, Y2=x, Z2=x)):
            with pytest.raises(_lib.AbacusHipError, match=r'^abacus_threepcf: '):
                triplet_multipoles(x, x, x, kw['boxsize'], kw['rbins'], kw['lmax'], **second)
    with pytest.raises(ValueError):
        triplet_multipoles(x, x, x, 100.0, [1.0, 2.0], 2, X2=x)
    with pytest.raises(ValueError):
        triplet_multipoles(x, x, x[:3], 100.0, [1.0, 2.0], 2)
    with pytest.raises(ValueError):
        triplet_multipoles(x, x, x, 100.0, [1.0, 2.0], 2, w=x[:3])
    with pytest.raises(ValueError):
        triplet_multipoles(x, x, x, 100.0, [1.0, 2.0], 2, w2=x)                              # w2 without a second set
    with pytest.raises(ValueError):
        calc_3pcf(x, x, x, 100.0, [1.0, 2.0], 2, randoms=10)                                 # random centres need a seed
    # what the Python entry cannot express, through the C entries themselves: point counts, null arguments, pos_dtype
    L = _lib.lib()
    f = np.zeros(4, np.float32)
    r = np.array([1.0, 2.0, 3.0], np.float32)
    zeta, wself, npairs = np.full(3 * 2 * 2, 7.0), np.full(2, 7.0), np.full(2, 7, np.uint64)
    p, n4, n0, big, half = _lib.ptr, C.c_int64(4), C.c_int64(0), C.c_int64(1 << 31), C.c_int64(1 << 30)
    tail = (C.c_float(100.0), p(r), 2, 2, p(zeta), p(wself), p(npairs))
    none4 = (None, None, None, None)

    def refused(rc, name='abacus_threepcf'):
        assert rc != 0 and L.abacus_last_error().decode().startswith(name + ': ')
    fn = L.abacus_threepcf
    refused(fn(p(f), p(f), p(f), None, big, *none4, n0, *tail))
    refused(fn(p(f), p(f), p(f), None, C.c_int64(-1), *none4, n0, *tail))
    refused(fn(p(f), p(f), p(f), None, n4, p(f), p(f), p(f), None, C.c_int64(-1), *tail))
    refused(fn(p(f), p(f), p(f), None, half, p(f), p(f), p(f), None, half, *tail))          # n + n2 = 2^31
    refused(fn(None, p(f), p(f), None, n4, *none4, n0, *tail))
    refused(fn(p(f), None, p(f), None, n4, *none4, n0, *tail))
    refused(fn(p(f), p(f), None, None, n4, *none4, n0, *tail))
    refused(fn(p(f), p(f), p(f), None, n4, p(f), None, p(f), None, n4, *tail))              # y2 with x2
    refused(fn(p(f), p(f), p(f), None, n4, p(f), p(f), None, None, n4, *tail))              # z2 with x2
    refused(fn(p(f), p(f), p(f), None, n4, None, p(f), p(f), None, n4, *tail))              # ... and only with it
    refused(fn(p(f), p(f), p(f), None, n4, None, None, None, p(f), n4, *tail))              # w2 only with x2
    refused(fn(p(f), p(f), p(f), None, n4, *none4, n0, C.c_float(100.0), None, 2, 2, p(zeta), p(wself), p(npairs)))
    refused(fn(p(f), p(f), p(f), None, n4, *none4, n0, C.c_float(100.0), p(r), 2, 2, None, p(wself), p(npairs)))
    refused(fn(p(f), p(f), p(f), None, n4, *none4, n0, C.c_float(100.0), p(r), 2, 2, p(zeta), None, p(npairs)))
    refused(fn(p(f), p(f), p(f), None, n4, *none4, n0, C.c_float(100.0), p(r), 2, 2, p(zeta), p(wself), None))
    # the resident form: the host arrays stand in for device pointers - a refused call reads none of them
    dev = L.abacus_threepcf_dev
    refused(dev(p(f), p(f), p(f), None, n4, *none4, n0, 7, *tail), 'abacus_threepcf_dev')
    refused(dev(p(f), p(f), p(f), None, big, *none4, n0, 0, *tail), 'abacus_threepcf_dev')
    refused(dev(p(f), p(f), p(f), None, n4, *none4, n0, 0, C.c_float(100.0), p(r), 33, 2, p(zeta), p(wself), p(npairs)),
            'abacus_threepcf_dev')
    assert np.all(zeta == 7.0) and np.all(wself == 7.0) and np.all(npairs == 7)              # a refused call writes nothing
