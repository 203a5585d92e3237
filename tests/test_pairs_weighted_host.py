"""The weighted estimator arithmetic of analysis/tpcf_corrfunc.py without a GPU: `_natural_estimator` and the three
calc_*_fast wrappers on a stand-in counter built from tests/pairs_statement.py (the way oracle/make_golden.py stands in
for Corrfunc with the brute-force counter for the unweighted goldens)."""
import numpy as np
import pytest
from pairs_statement import paircount as statement


def _counters(calls):
    def res(n, ws):
        out = np.zeros(len(n), dtype=[('npairs', 'u8'), ('weightsum', 'f8')])
        out['npairs'], out['weightsum'] = n, ws
        return out

    def DDrppi(autocorr, nthreads, binfile=None, pimax=None, X1=None, Y1=None, Z1=None, X2=None, Y2=None, Z2=None,
               boxsize=None, weights1=None, weights2=None, weight_type=None, **kw):
        calls.append(('rppi', weights1 is not None, weights2 is not None, weight_type))
        s = (None, None, None) if autocorr else (X2, Y2, Z2)
        n, ws, _, _ = statement('rppi', X1, Y1, Z1, float(boxsize), binfile, *s, w1=weights1, w2=weights2,
                                pimax=float(pimax), npibins=int(pimax))
        return res(n, ws)

    def DDsmu(autocorr, nthreads, binfile=None, mu_max=None, nmu_bins=None, X1=None, Y1=None, Z1=None, X2=None, Y2=None,
              Z2=None, boxsize=None, weights1=None, weights2=None, weight_type=None, **kw):
        calls.append(('smu', weights1 is not None, weights2 is not None, weight_type))
        s = (None, None, None) if autocorr else (X2, Y2, Z2)
        n, ws, _, _ = statement('smu', X1, Y1, Z1, float(boxsize), binfile, *s, w1=weights1, w2=weights2,
                                mu_max=float(mu_max), nmubins=int(nmu_bins))
        return res(n, ws)
    return DDrppi, DDsmu


@pytest.fixture
def T(monkeypatch):
    from abacusutils_amd.analysis import tpcf_corrfunc as mod
    mod.calls = []
    DDrppi, DDsmu = _counters(mod.calls)
    monkeypatch.setattr(mod, 'DDrppi', DDrppi)
    monkeypatch.setattr(mod, 'DDsmu', DDsmu)
    yield mod
    del mod.calls


def _cat(n, box, seed):
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3)) * box
    p[: n // 3] = (p[0] + rng.normal(0, 3.0, (n // 3, 3))) % box          # a clump: xi > 0 at small separations
    w = rng.integers(512, 1536, n).astype(np.float32) / np.float32(1024)   # [0.5, 1.5) on a grid of 2^-10
    return [p[:, i].copy() for i in range(3)], w


def test_natural_estimator_weighted_definition(T):
    """DD = sum w_i w_j (the counter's weightsum), RR = measure / L^3 * W1 * W2 * 2 with W = sum of the weights in float64,
    W2 = W1 for an autocorrelation and W = N for a side without weights; no weights: the unweighted call, untouched"""
    box = np.float32(120.0)
    (x1, y1, z1), w1 = _cat(500, 120.0, 1)
    (x2, y2, z2), w2 = _cat(400, 120.0, 2)
    edges = np.linspace(1.0, 12.0, 5).astype(np.float32)
    shell = (np.pi * (edges[1:] ** 2 - edges[:-1] ** 2))
    kw = dict(nthreads=1, binfile=edges, pimax=np.float32(6))
    W1, W2 = float(np.sum(w1, dtype=np.float64)), float(np.sum(w2, dtype=np.float64))
    for second, ws, want_w in (((None, None, None), (w1, None), W1 * W1), ((x2, y2, z2), (w1, w2), W1 * W2),
                               ((x2, y2, z2), (w1, None), W1 * 400.0), ((x2, y2, z2), (None, w2), 500.0 * W2)):
        dd, rr = T._natural_estimator(T.DDrppi, (x1, y1, z1), second, edges, box, shell, 6, w1=ws[0], w2=ws[1], **kw)
        s = (None, None, None) if second[0] is None else [np.asarray(c, np.float32) for c in second]
        _, want_dd, _, _ = statement('rppi', x1, y1, z1, 120.0, edges, *s, w1=ws[0], w2=ws[1], pimax=6.0, npibins=6)
        np.testing.assert_array_equal(dd.ravel(), want_dd)       # the same statement, the same order: identical
        assert rr.dtype == np.float32
        # float32 RR: three float32 products after the float64 W1 W2 - a few 2^-24
        np.testing.assert_allclose(rr, shell.astype(np.float64) / 120.0 ** 3 * want_w * 2, rtol=4 * 2.0 ** -24)
        assert T.calls[-1][3] == 'pair_product'
    dd, rr = T._natural_estimator(T.DDrppi, (x1, y1, z1), (None, None, None), edges, box, shell, 6, **kw)
    assert T.calls[-1] == ('rppi', False, False, None) and dd.dtype == np.uint64
    np.testing.assert_array_equal(rr, shell / box**3 * 500.0 * 500.0 * 2)


def test_duplicated_catalogue_is_weight_two(T):
    """Every point twice (weights w) is the catalogue with weights 2 w: sum (2 w_i)(2 w_j) over the pairs of the original
    = sum over the four copies of each pair, and W = sum 2 w both ways; the two copies of one point sit at r = 0, below the
    first edge.  Rounding allowed: NONE.  The weights lie on a grid of 2^-10, so every product is a multiple of 2^-20, every
    partial sum of products and of weights (far below 2^53 such units) is exact in float64 whatever its order, DD and W are
    the same numbers on both sides and everything after them is the same sequence of operations."""
    (x, y, z), w = _cat(700, 150.0, 3)
    dup = lambda a: np.concatenate([a, a])       # noqa: E731
    rpbins = np.geomspace(0.5, 15.0, 7)
    two = (2 * w).astype(np.float32)
    (x2, y2, z2), w2 = _cat(300, 150.0, 4)
    for second_o, second_d in (({}, {}), (dict(x2=x2, y2=y2, z2=z2, w2=w2), dict(x2=x2, y2=y2, z2=z2, w2=w2))):
        for f, args in ((T.calc_wp_fast, (rpbins, 10, 150.0, 1)), (T.calc_xirppi_fast, (rpbins, 10, 5, 150.0, 1)),
                        (T.calc_multipole_fast, (rpbins, 150.0, 1))):
            kw = dict(nbins_mu=8, orders=[0, 2]) if f is T.calc_multipole_fast else {}
            a = f(dup(x), dup(y), dup(z), *args, w1=dup(w), **second_d, **kw)
            b = f(x, y, z, *args, w1=two, **second_o, **kw)
            assert np.all(np.isfinite(a)) and np.abs(a).max() > 0.1
            np.testing.assert_array_equal(a, b)
    # unit weights: the duplicated catalogue through the UNWEIGHTED path (integer counts, N as a float) against weights 2
    a = T.calc_wp_fast(dup(x), dup(y), dup(z), rpbins, 10, 150.0, 1)
    b = T.calc_wp_fast(x, y, z, rpbins, 10, 150.0, 1, w1=np.full(700, 2.0, np.float32))
    np.testing.assert_array_equal(a, b)
    assert [c[1] for c in T.calls[-2:]] == [False, True]


def test_weight_keywords_are_checked_before_the_device():
    """the ValueError / NotImplementedError rules of DD / DDrppi / DDsmu need no GPU"""
    from abacusutils_amd.analysis import tpcf_corrfunc as T
    x = np.linspace(0.0, 9.0, 10)
    w = np.ones(10, np.float32)
    bins = np.linspace(0.5, 3.0, 4)
    for call in (lambda **k: T.DD(1, 1, bins, x, x, x, boxsize=20.0, **k),
                 lambda **k: T.DDrppi(1, 1, binfile=bins, pimax=3.0, X1=x, Y1=x, Z1=x, boxsize=20.0, **k),
                 lambda **k: T.DDsmu(1, 1, bins, 1.0, 4, x, x, x, boxsize=20.0, **k)):
        with pytest.raises(ValueError, match='weight_type'):
            call(weights1=w)
        with pytest.raises(NotImplementedError, match='pair_sum'):
            call(weights1=w, weight_type='pair_sum')
        with pytest.raises(ValueError, match='weights1'):
            call(weights1=w[:-1], weight_type='pair_product')
    with pytest.raises(ValueError, match='weights2'):
        T.DD(0, 1, bins, x, x, x, X2=x, Y2=x, Z2=x, boxsize=20.0, weights1=w, weights2=w[:3], weight_type='pair_product')
