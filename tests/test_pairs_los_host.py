"""The light-cone pair counter without a GPU: the NumPy statement (tests/pairs_los_statement.py) against a scalar double
loop and closed-form pairs, its invariants, the Landy-Szalay algebra of analysis/tpcf_corrfunc.py on a stubbed counter, the
sky-coordinate wrappers' argument rules and the C ABI's validation, which comes before the device is touched."""
import ctypes as C

import numpy as np
import pytest
from pairs_los_statement import centre, paircount as statement, scalar, shell_points

GEOM = {'r': {}, 'rppi': dict(pimax=12.0, npibins=12), 'smu': dict(mu_max=1.0, nmubins=5)}


@pytest.mark.parametrize('auto', [True, False])
@pytest.mark.parametrize('mode', ['r', 'rppi', 'smu'])
def test_statement_against_scalar_loop(mode, auto):
    origin = (-990.0, -990.0, -990.0)
    a = shell_points(40, 1, chi=(1500.0, 1520.0), clump=0.7, spread=0.02)
    b = None if auto else shell_points(33, 2, chi=(1500.0, 1520.0), clump=0.7, spread=0.02)
    rng = np.random.default_rng(3)
    w1 = rng.random(40).astype(np.float32) + np.float32(0.5)
    w2 = None if auto else rng.random(33).astype(np.float32) - np.float32(0.5)
    bins = np.array([0.0, 1.0, 3.0, 8.0, 20.0, 60.0])
    second = (None, None, None) if auto else b
    n, ws, rs, wabs = statement(mode, *a, bins, *second, w1=w1, w2=w2, origin=origin, **GEOM[mode])
    pa = np.stack(centre(a, origin), axis=1)
    pb = None if auto else np.stack(centre(b, origin), axis=1)
    n0, ws0, rs0 = scalar(mode, pa, bins, pb, w1, w2, **GEOM[mode])
    assert n.sum() > 20
    np.testing.assert_array_equal(n, n0)
    np.testing.assert_allclose(ws, ws0, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(rs, rs0, rtol=1e-13)
    assert np.all(wabs >= np.abs(ws) - 1e-12)


def test_closed_form_pairs():
    bins = np.array([0.0, 5.0, 15.0, 300.0])
    rp = dict(pimax=20.0, npibins=20)
    # along the line of sight: pi = 10 exactly, rp = 0
    x, y, z = np.zeros(2), np.zeros(2), np.array([100.0, 110.0])
    n, _, rs, _ = statement('rppi', x, y, z, bins, **rp)
    want = np.zeros((3, 20), np.uint64)
    want[0, 10] = 2
    np.testing.assert_array_equal(n.reshape(3, 20), want)
    assert rs.sum() == 0.0
    n, _, rs, _ = statement('smu', x, y, z, bins, mu_max=1.0, nmubins=4)
    assert n.sum() == 0                       # mu = 1 is not below mu_max
    n, _, rs, _ = statement('smu', x, y, z, bins, mu_max=1.5, nmubins=3)
    np.testing.assert_array_equal(n.reshape(3, 3)[1], [0, 0, 2])
    assert rs.reshape(3, 3)[1, 2] == 20.0
    # across it: pi = 0, rp = 10
    x = np.array([5.0, -5.0])
    y, z = np.zeros(2), np.full(2, 100.0)
    n, _, rs, _ = statement('rppi', x, y, z, bins, **rp)
    want[:] = 0
    want[1, 0] = 2
    np.testing.assert_array_equal(n.reshape(3, 20), want)
    assert rs.reshape(3, 20)[1, 0] == 20.0
    # p and -p: l = 0, no line of sight: s only
    x, y, z = np.array([3.0, -3.0]), np.array([4.0, -4.0]), np.array([12.0, -12.0])
    assert statement('rppi', x, y, z, bins, **rp)[0].sum() == 0
    assert statement('smu', x, y, z, bins, mu_max=1.0, nmubins=4)[0].sum() == 0
    n, _, rs, _ = statement('r', x, y, z, bins)
    np.testing.assert_array_equal(n, [0, 0, 2])
    assert rs[2] == 52.0
    # the origin is subtracted in the column's dtype: the first case again, seen from (7, -3, 50)
    n, _, _, _ = statement('rppi', np.full(2, 7.0), np.full(2, -3.0), np.array([150.0, 160.0]), bins, origin=(7.0, -3.0, 50.0), **rp)
    assert n.reshape(3, 20)[0, 10] == 2


@pytest.mark.parametrize('mode', ['r', 'rppi', 'smu'])
def test_statement_invariants(mode):
    """swapping the sets of a cross count leaves every bin bit-equal (t changes sign, t^2 does not; the weight products
    commute); every bin of an autocorrelation holds an even count"""
    origin = (-990.0, -990.0, -990.0)
    a, b = shell_points(300, 5, chi=(1500.0, 1530.0), spread=0.03), shell_points(250, 6, chi=(1500.0, 1530.0), spread=0.03)
    bins = np.geomspace(0.5, 30.0, 7)
    ab = statement(mode, *a, bins, *b, origin=origin, **GEOM[mode])
    ba = statement(mode, *b, bins, *a, origin=origin, **GEOM[mode])
    assert ab[0].sum() > 100
    np.testing.assert_array_equal(ab[0], ba[0])
    np.testing.assert_allclose(ab[2], ba[2], rtol=1e-13)
    aa = statement(mode, *a, bins, origin=origin, **GEOM[mode])
    assert aa[0].sum() > 100 and np.all(aa[0] % np.uint64(2) == 0)


def test_landy_szalay_algebra(monkeypatch):
    """every term a weight sum over its normalisation - Wa Wb for cross counts, W^2 - sum w^2 for the ordered
    autocorrelations (N (N - 1) for unit weights) -, DR counted once for an autocorrelation, RR once per binning"""
    from abacusutils_amd.analysis import tpcf_corrfunc as T

    def fake_init(self, x, y, z, w=None, origin=(0.0, 0.0, 0.0)):
        self.n, self.cols, self.w = len(x), [x, y, z], w
        hw = np.ones(self.n) if w is None else np.asarray(w, np.float64)
        self.W, self.W2 = float(hw.sum()), float((hw * hw).sum())
    monkeypatch.setattr(T._LCSample, '__init__', fake_init)
    calls = []
    table = {}

    def fake_count(mode, X1, Y1, Z1, bins, X2=None, Y2=None, Z2=None, W1=None, W2=None, want_rsum=True, **geom):
        key = (X1[0], None if X2 is None else X2[0])
        calls.append((mode, key, geom))
        nsub = geom.get('npibins') or geom.get('nmubins') or 1
        rng = np.random.default_rng(abs(hash(key)) % 1000)
        table[key] = rng.integers(50, 500, (len(bins) - 1) * nsub).astype(np.float64)
        return None, table[key], None
    monkeypatch.setattr(T, '_paircount_los', fake_count)
    tag = lambda t, n: (np.full(n, t), np.zeros(n), np.zeros(n))      # noqa: E731
    wr = np.linspace(0.5, 1.5, 50)
    R = T.LCRandoms(*tag(9.0, 50), w=wr)
    w1 = np.linspace(1.0, 2.0, 20)
    rpbins = np.array([1.0, 2.0, 4.0])
    # autocorrelation, weighted
    xi = T.calc_xirppi_lc(*tag(1.0, 20), rpbins, 4, 2, R, w1=w1)
    assert [c[1] for c in calls] == [(9.0, None), (1.0, 9.0), (1.0, None)]
    g = lambda a: a.reshape(2, 2, 2).sum(axis=2)                      # noqa: E731
    dd, dr, rr = g(table[(1.0, None)]), g(table[(1.0, 9.0)]), g(table[(9.0, None)])
    W1, Wr = w1.sum(), wr.sum()
    ndd, nrr = W1 ** 2 - (w1 ** 2).sum(), Wr ** 2 - (wr ** 2).sum()
    want = (dd / ndd - 2 * dr / (W1 * Wr) + rr / nrr) / (rr / nrr)
    assert xi.shape == (2, 2)
    np.testing.assert_allclose(xi, want, rtol=1e-14)
    # cross correlation, unit weights on the second set; RR comes from the cache
    del calls[:]
    xi = T.calc_xirppi_lc(*tag(1.0, 20), rpbins, 4, 2, R, x2=tag(2.0, 30)[0], y2=np.zeros(30), z2=np.zeros(30), w1=w1)
    assert [c[1] for c in calls] == [(1.0, 9.0), (1.0, 2.0), (2.0, 9.0)] and R.rr_counted == 1
    d12, d1r, d2r = g(table[(1.0, 2.0)]), g(table[(1.0, 9.0)]), g(table[(2.0, 9.0)])
    want = (d12 / (W1 * 30.0) - d1r / (W1 * Wr) - d2r / (30.0 * Wr) + rr / nrr) / (rr / nrr)
    np.testing.assert_allclose(xi, want, rtol=1e-14)
    # wp: 2 * the sum over unit pi bins; the same (mode, bins, pi binning): still one RR
    wp = T.calc_wp_lc(*tag(1.0, 20), rpbins, 4, R)
    assert R.rr_counted == 1
    u = lambda a: a.reshape(2, 4)                                     # noqa: E731
    dd, dr, rr4 = u(table[(1.0, None)]), u(table[(1.0, 9.0)]), u(table[(9.0, None)])
    want = 2 * np.sum((dd / (20.0 * 19.0) - 2 * dr / (20.0 * Wr) + rr4 / nrr) / (rr4 / nrr), axis=1)
    np.testing.assert_allclose(wp, want, rtol=1e-14)
    # multipoles: another mode, another RR
    xl = T.calc_multipole_lc(*tag(1.0, 20), rpbins, R, nbins_mu=4, orders=[0, 2])
    assert R.rr_counted == 2 and xl.shape == (4,) and calls[-1][0] == 2 and calls[-1][2] == dict(mu_max=1.0, nmubins=4)
    dd, dr, rrm = u(table[(1.0, None)]), u(table[(1.0, 9.0)]), u(table[(9.0, None)])
    xi = (dd / (20.0 * 19.0) - 2 * dr / (20.0 * Wr) + rrm / nrr) / (rrm / nrr)
    mu = np.linspace(0, 1, 5)
    want = np.concatenate([T.tpcf_multipole(xi, mu, order=ell) for ell in (0, 2)])
    np.testing.assert_allclose(xl, want, rtol=1e-14)
    with pytest.raises(ValueError, match='divisor'):
        T.calc_xirppi_lc(*tag(1.0, 20), rpbins, 4, 3, R)
    with pytest.raises(TypeError, match='LCRandoms'):
        T.calc_wp_lc(*tag(1.0, 20), rpbins, 4, tag(9.0, 50))
    # the unit-weight ordered normalisation is N (N - 1)
    assert T._LCSample(*tag(1.0, 20)).auto_norm == 20.0 * 19.0


def test_radec_round_trip():
    from abacusutils_amd.analysis.tpcf_corrfunc import radec_to_xyz
    rng = np.random.default_rng(8)
    ra, dec, d = rng.uniform(0, 360, 200), np.degrees(np.arcsin(rng.uniform(-1, 1, 200))), rng.uniform(100, 3000, 200)
    x, y, z = radec_to_xyz(ra, dec, d)
    assert x.dtype == y.dtype == z.dtype == np.float64
    np.testing.assert_allclose(np.sqrt(x * x + y * y + z * z), d, rtol=1e-14)
    np.testing.assert_allclose(np.degrees(np.arcsin(z / d)), dec, atol=1e-10)
    np.testing.assert_allclose(np.degrees(np.arctan2(y, x)) % 360.0, ra, atol=1e-10)
    np.testing.assert_allclose(radec_to_xyz(90.0, 0.0, 2.0), (0.0, 2.0, 0.0), atol=1e-15)
    np.testing.assert_allclose(radec_to_xyz(0.0, 90.0, 2.0), (0.0, 0.0, 2.0), atol=1e-15)


def test_wrapper_argument_errors():
    """raised before any library call"""
    from abacusutils_amd.analysis import tpcf_corrfunc as T
    ra = dec = np.linspace(1.0, 9.0, 10)
    d = np.linspace(1000.0, 1100.0, 10)
    w = np.ones(10, np.float32)
    bins = np.linspace(0.5, 3.0, 4)
    with pytest.raises(NotImplementedError, match='is_comoving_dist'):
        T.DDrppi_mocks(1, 1, 1, 3.0, bins, ra, dec, d)
    with pytest.raises(NotImplementedError, match='is_comoving_dist'):
        T.DDsmu_mocks(1, 1, 1, 1.0, 4, bins, ra, dec, d)
    with pytest.raises(ValueError, match='RA2'):
        T.DDrppi_mocks(0, 1, 1, 3.0, bins, ra, dec, d, is_comoving_dist=True)
    for call in (lambda **k: T.DD_los(1, 1, bins, d, d, d, **k),
                 lambda **k: T.DDrppi_los(1, 1, bins, 3.0, d, d, d, **k),
                 lambda **k: T.DDsmu_los(1, 1, bins, 1.0, 4, d, d, d, **k),
                 lambda **k: T.DDrppi_mocks(1, None, 1, 3.0, bins, ra, dec, d, is_comoving_dist=True, **k)):
        with pytest.raises(ValueError, match='weight_type'):
            call(weights1=w)
        with pytest.raises(NotImplementedError, match='pair_sum'):
            call(weights1=w, weight_type='pair_sum')
        with pytest.raises(ValueError, match='weights1'):
            call(weights1=w[:-1], weight_type='pair_product')
    with pytest.raises(ValueError, match='origin'):
        T.DD_los(1, 1, bins, d, d, d, origin=(0.0, 0.0))
    with pytest.raises(ValueError, match='pimax'):
        T.DDrppi_los(1, 1, bins, 0.0, d, d, d)
    with pytest.raises(ValueError, match='mu_max'):
        T.DDsmu_los(1, 1, bins, 0.0, 4, d, d, d)
    with pytest.raises(ValueError, match='X2'):
        T.DD_los(0, 1, bins, d, d, d)


def test_abacus_hod_randoms_need_an_origin():
    from abacusutils_amd.hod.abacus_hod import AbacusHOD
    ball = AbacusHOD.__new__(AbacusHOD)
    ball.halo_lc, ball.params = False, {'origin': None}
    for call in (lambda: ball.compute_wp({}, np.array([1.0, 2.0]), 4, 1, randoms=object()),
                 lambda: ball.compute_xirppi({}, np.array([1.0, 2.0]), 4, 1, randoms=object()),
                 lambda: ball.compute_multipole({}, np.array([1.0, 2.0]), 4, np.array([1.0, 2.0]), 4, randoms=object())):
        with pytest.raises(ValueError, match='origin'):
            call()


def test_c_abi_validates_before_the_device():
    """every rule of include/abacus_hip.h's abacus_paircount_los answers with an error of its own, with or without a GPU"""
    from abacusutils_amd import _lib
    from abacusutils_amd._lib import ptr
    L = _lib.lib()
    x = np.linspace(0.0, 9.0, 10).astype(np.float32)
    w = np.ones(10, np.float32)
    origin = np.zeros(3)
    bins = np.array([0.5, 1.0, 2.0], np.float32)
    out, ws, rs = np.zeros(64, np.uint64), np.zeros(64), np.zeros(64)

    def call(mode=1, x1=x, w2=None, x2=None, org=origin, b=bins, nb=2, pimax=4.0, npi=4, mu_max=1.0, nmu=4, npairs=out):
        return L.abacus_paircount_los(mode, ptr(x1), ptr(x), ptr(x), ptr(w), C.c_int64(10), ptr(x2), ptr(x2), ptr(x2), ptr(w2),
                                      C.c_int64(0 if x2 is None else 10), ptr(org), ptr(b), nb, C.c_float(pimax), npi,
                                      C.c_float(mu_max), nmu, ptr(npairs), ptr(ws), ptr(rs))
    for kw, text in ((dict(mode=3), 'unknown mode'), (dict(x1=None), 'null'), (dict(org=None), 'null'), (dict(b=None), 'null'),
                     (dict(npairs=None), 'null'), (dict(nb=0), 'nbins'), (dict(b=np.array([0.5, 2.0, 2.0], np.float32)), 'increase'),
                     (dict(b=np.array([2.0, 1.0, 3.0], np.float32)), 'increase'), (dict(b=np.array([-1.0, 1.0, 3.0], np.float32)), 'negative'),
                     (dict(w2=w), 'autocorrelation'), (dict(pimax=0.0), 'pimax'), (dict(pimax=-1.0), 'pimax'),
                     (dict(mode=2, mu_max=0.0), 'mu_max'), (dict(mode=2, nmu=0), 'mu_max'), (dict(npi=0), 'pimax'),
                     (dict(org=np.array([0.0, np.inf, 0.0])), 'origin')):
        assert call(**kw) != 0, kw
        assert text in L.abacus_last_error().decode(), (kw, L.abacus_last_error().decode())
    assert L.abacus_paircount_los_dev(1, ptr(x), ptr(x), ptr(x), None, C.c_int64(10), None, None, None, None, C.c_int64(0), 7,
                                      ptr(origin), ptr(bins), 2, C.c_float(4.0), 4, C.c_float(1.0), 4, ptr(out), None, None) != 0
    assert 'pos_dtype' in L.abacus_last_error().decode()
