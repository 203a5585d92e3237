"""The NumPy side of the jackknife (abacusutils_amd/analysis/jackknife.py: delete_one, delete_one_norm, jackknife_covariance,
the box estimator on given counts) on per-region counts made by the statements (tests/pairs_jk_statement.py) from a few
hundred points.  Runs without a GPU."""
import functools

import numpy as np
import pytest
import pairs_jk_statement as jks
from pairs_los_statement import shell_points

from abacusutils_amd.analysis import jackknife as jk

BOX = 100.0
BINS = np.linspace(0.0, 20.0, 6)          # from 0: coincident points are pairs
SUBKW = {'r': {}, 'rppi': dict(pimax=20.0, npibins=4), 'smu': dict(mu_max=1.0, nmubins=3)}
NREG = 4


def _box_points(n, seed):
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3)) * BOX
    p[: n // 4] = (p[n // 4] + rng.normal(0, 3.0, (n // 4, 3))) % BOX
    p[5] = p[6]                           # a duplicated point
    return [p[:, i].copy() for i in range(3)]


@functools.lru_cache(maxsize=None)
def _case(family, mode, auto):
    """(statement, a, la, b, lb, w1, w2, counts)"""
    rng = np.random.default_rng(7)
    if family == 'box':
        a, b = _box_points(300, 1), (None if auto else _box_points(260, 2))
        st = jks.box(BOX, BINS, **SUBKW[mode])
    else:
        origin = (-990.0, -990.0, -990.0)
        a = shell_points(300, 3, chi=(1500.0, 1560.0), origin=origin, spread=0.03)
        b = None if auto else shell_points(260, 4, chi=(1500.0, 1560.0), origin=origin, spread=0.03)
        st = jks.los(BINS, origin=origin, **SUBKW[mode])
    la = rng.integers(0, NREG, 300)
    lb = None if auto else rng.integers(0, NREG, 260)
    w1 = (2 * rng.random(300) - 1).astype(np.float32)
    w2 = None if auto else (0.5 + rng.random(260)).astype(np.float32)
    return st, a, la, b, lb, w1, w2, jks.counts(st, mode, a, la, NREG, b, lb, w1, w2)


CASES = [(f, m, au) for f in ('box', 'los') for m in ('r', 'rppi', 'smu') for au in (True, False)]


@pytest.mark.parametrize('family,mode,auto', CASES)
def test_count_identities(family, mode, auto):
    c = _case(family, mode, auto)[-1]
    n = jks.pick(c, 'npairs')
    assert n['total'].sum() > 0
    np.testing.assert_array_equal(n['first'].sum(axis=0), n['total'])
    np.testing.assert_array_equal(n['second'].sum(axis=0), n['total'])
    assert np.all(n['both'] <= n['first']) and np.all(n['both'] <= n['second'])
    if auto:
        np.testing.assert_array_equal(n['second'], n['first'])


@pytest.mark.parametrize('family,mode', [(f, m) for f in ('box', 'los') for m in ('r', 'rppi', 'smu')])
def test_exchange_symmetry(family, mode):
    """membership is symmetric under exchange of the two points: the exchanged cross call has first <-> second and the same both"""
    st, a, la, b, lb, w1, w2, c = _case(family, mode, False)
    x = jks.counts(st, mode, b, lb, NREG, a, la, w2, w1)
    np.testing.assert_array_equal(x['both']['npairs'], c['both']['npairs'])
    np.testing.assert_array_equal(x['first']['npairs'], c['second']['npairs'])
    np.testing.assert_array_equal(x['second']['npairs'], c['first']['npairs'])
    np.testing.assert_array_equal(x['total']['npairs'], c['total']['npairs'])


@pytest.mark.parametrize('family,mode,auto', CASES)
def test_removal_identity(family, mode, auto):
    """delete_one at cross_weight 1 IS the count of the catalogue without region k: exactly in npairs, to rounding in wsum"""
    st, a, la, b, lb, w1, w2, c = _case(family, mode, auto)
    dn = jk.delete_one(jks.pick(c, 'npairs'), 1.0)
    dw = jk.delete_one(jks.pick(c, 'wsum'), 1.0)
    assert dn.dtype == np.int64
    for k in range(NREG):
        n, ws, wabs = jks.removed(st, mode, a, la, k, b, lb, w1, w2)
        np.testing.assert_array_equal(dn[k], n.astype(np.int64))
        # four float64 sums of at most N terms each, combined: a few N 2^-52 of sum |w w| over the whole bin
        tol = 8 * c['total']['npairs'] * 2.0 ** -52 * c['total']['wabs'] + 1e-300
        assert np.all(np.abs(dw[k] - ws) <= tol)


def test_delete_one_takes_counts_objects():
    c = _case('box', 'rppi', False)[-1]
    shape = (len(BINS) - 1, 4)
    term = lambda t: jk.JKTerm(c[t]['npairs'].reshape((-1,) + shape), c[t]['wsum'].reshape((-1,) + shape))   # noqa: E731
    obj = jk.JKCounts(jk.JKTerm(c['total']['npairs'].reshape(shape), c['total']['wsum'].reshape(shape)), term('first'),
                      term('second'), term('both'))
    assert obj.nreg == NREG
    for alpha in (1.0, 0.5):
        d = jk.delete_one(obj, alpha)
        np.testing.assert_array_equal(d.npairs.reshape(NREG, -1), jk.delete_one(jks.pick(c, 'npairs'), alpha))
        np.testing.assert_array_equal(d.wsum.reshape(NREG, -1), jk.delete_one(jks.pick(c, 'wsum'), alpha))
    half = jk.delete_one(jks.pick(c, 'npairs'), 0.5)
    np.testing.assert_array_equal(half, c['total']['npairs'][None] - 0.5 * (c['first']['npairs'] + c['second']['npairs'].astype(np.float64)))


@pytest.mark.parametrize('unit', [True, False])
@pytest.mark.parametrize('auto', [True, False])
def test_delete_one_norm_is_the_reduced_normalisation(auto, unit):
    rng = np.random.default_rng(11)
    la, lb = rng.integers(0, NREG, 300), rng.integers(0, NREG, 260)
    w1 = None if unit else (0.5 + rng.random(300)).astype(np.float32)
    w2 = None if unit else (0.5 + rng.random(260)).astype(np.float32)
    k1, sq1 = jk.region_sums(la, NREG, w1)
    k2, _ = jk.region_sums(lb, NREG, w2)
    v1 = np.ones(300) if unit else w1.astype(np.float64)
    v2 = np.ones(260) if unit else w2.astype(np.float64)
    if auto:
        total, dels = jk.delete_one_norm(k1, None, 1.0, sq1)
        want_total = v1.sum() ** 2 - (v1 * v1).sum()
        want = [v1[la != k].sum() ** 2 - (v1[la != k] ** 2).sum() for k in range(NREG)]
    else:
        total, dels = jk.delete_one_norm(k1, k2, 1.0)
        want_total = v1.sum() * v2.sum()
        want = [v1[la != k].sum() * v2[lb != k].sum() for k in range(NREG)]
    if unit:                  # integer-valued float64: exact
        assert total == want_total
        np.testing.assert_array_equal(dels, want)
    else:
        np.testing.assert_allclose(total, want_total, rtol=1e-13)
        np.testing.assert_allclose(dels, want, rtol=1e-12)
    # cross_weight 1/2: total - (first + second) / 2
    first = k1 * k2.sum() if not auto else k1 * k1.sum() - sq1
    second = k1.sum() * k2 if not auto else first
    np.testing.assert_allclose(jk.delete_one_norm(k1, None if auto else k2, 0.5, sq1 if auto else None)[1],
                               total - 0.5 * (first + second), rtol=1e-13)
    with pytest.raises(ValueError):
        jk.delete_one_norm(k1, None, 1.0)


def test_covariance_against_a_loop():
    rng = np.random.default_rng(3)
    s = rng.normal(size=(9, 5)) * np.arange(1, 6)
    cov = jk.jackknife_covariance(s)
    mean = s.mean(axis=0)
    want = np.zeros((5, 5))
    for k in range(9):
        want += np.outer(s[k] - mean, s[k] - mean)
    want *= 8 / 9
    np.testing.assert_allclose(cov, want, rtol=1e-13, atol=1e-15)
    np.testing.assert_array_equal(cov, cov.T)
    assert np.linalg.eigvalsh(cov).min() >= -1e-12 * np.abs(cov).max()
    assert np.all(jk.jackknife_covariance(s[:1]) == 0)


@pytest.mark.parametrize('auto', [True, False])
def test_box_estimator_on_statement_counts(auto):
    """natural_samples against a few-line restatement: xi_-k = (total - (first_k + second_k) / 2) / (RR (1 - s1_k / 2 - s2_k / 2)) - 1"""
    st, a, la, b, lb, w1, w2, c = _case('box', 'rppi', auto)
    n = jks.pick(c, 'npairs')
    nb, npi = len(BINS) - 1, 4
    rr = np.linspace(50.0, 90.0, nb)
    stat = lambda dd, r: 2 * np.sum(dd.reshape(nb, npi) / r[:, None] - 1, axis=1)   # noqa: E731
    share1 = np.bincount(la, minlength=NREG) / len(la)
    share2 = share1 if auto else np.bincount(lb, minlength=NREG) / len(lb)
    full, samples, cov = jk.natural_samples(n, rr, share1, share2, stat, False)
    np.testing.assert_array_equal(full, stat(n['total'], rr))
    for k in range(NREG):
        d = n['total'].astype(np.float64) - 0.5 * (n['first'][k].astype(np.float64) + n['second'][k])
        xi = d.reshape(nb, npi) / (rr * (1 - 0.5 * share1[k] - 0.5 * share2[k]))[:, None] - 1
        np.testing.assert_allclose(samples[k], 2 * xi.sum(axis=1), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(cov, jk.jackknife_covariance(samples))
    assert samples.shape == (NREG, nb) and cov.shape == (nb, nb)


def test_box_cross_weight_other_than_half_is_refused():
    x = np.zeros(4)
    lab = np.zeros(4, np.int32)
    for fn, args in ((jk.calc_wp_jk, (BINS, 20, BOX, 1)), (jk.calc_xirppi_jk, (BINS, 20, 5, BOX, 1)), (jk.calc_multipole_jk, (BINS, BOX, 1))):
        with pytest.raises(NotImplementedError, match='share of the weight'):
            fn(x, x, x, *args, lab, 1, cross_weight=1.0)


def test_empty_region_is_refused():
    jk.check_populated(3, np.array([0, 1]), np.array([2]))
    with pytest.raises(ValueError, match=r'regions \[1\]'):
        jk.check_populated(3, np.array([0, 0]), np.array([2]))


def test_one_region():
    """nreg = 1: first = both = total, the delete-one count and normalisation are zero"""
    st, a, _, b, _, w1, w2, _ = _case('box', 'smu', False)
    c = jks.counts(st, 'smu', a, np.zeros(300, int), 1, b, np.zeros(260, int), w1, w2)
    n = jks.pick(c, 'npairs')
    np.testing.assert_array_equal(n['first'][0], n['total'])
    np.testing.assert_array_equal(n['both'][0], n['total'])
    assert np.all(jk.delete_one(n, 1.0) == 0)
    assert jk.delete_one_norm([300.0], [260.0], 1.0)[1][0] == 0
    assert jk.delete_one_norm([300.0], None, 1.0, [300.0])[1][0] == 0


def test_host_box_regions():
    L = 100.0
    x = np.array([0.0, 49.999, 50.0, 99.999, 100.0, -0.001, 150.0, np.nextafter(np.float32(100.0), np.float32(0.0))])
    z = np.zeros_like(x)
    lab = jk.box_regions(x, z, z, L, (2, 1, 1))
    assert lab.dtype == np.int32
    np.testing.assert_array_equal(lab, [0, 0, 1, 1, 0, 1, 1, 1])
    lab3 = jk.box_regions(x, x, x, L, 2)
    np.testing.assert_array_equal(lab3, lab * 7)
    with pytest.raises(ValueError):
        jk.box_regions(x, z, z, L, (2, 0, 1))


def _abi():
    import ctypes as C
    from abacusutils_amd import _lib
    return C, _lib.lib(), _lib.ptr


def _refused(L, entry, rc, text, what):
    msg = L.abacus_last_error().decode()
    assert rc != 0, (entry, what)
    assert text in msg and f'{entry}:' in msg, (entry, what, msg)


def test_jackknife_c_abi_validates_before_the_device():
    """every rule of abacus_paircount_jk / abacus_paircount_los_jk and their _dev forms (include/abacus_hip.h) answers with an
    error of its own that names the entry called, with or without a GPU: nothing touches the device for a refused call"""
    C, L, ptr = _abi()
    x = np.linspace(0.0, 9.0, 10).astype(np.float32)
    w, lab = np.ones(10, np.float32), (np.arange(10) % 4).astype(np.int32)
    origin = np.zeros(3)
    bins = np.array([0.5, 1.0, 2.0], np.float32)
    cnt = [np.zeros(64, np.uint64), np.zeros(64, np.uint64)]
    sums = [np.zeros(64), np.zeros(64)]

    def call(entry, mode=1, x1=x, x2=None, y2=None, z2=None, w2=None, lab1=lab, lab2=None, n1=10, n2=0, pos_dtype=0, nreg=4, box=100.0,
             org=origin, b=bins, nb=2, pimax=4.0, npi=4, mu_max=1.0, nmu=4, nfirst=cnt[0], wfirst=sums[0], wboth=sums[1]):
        dt = (pos_dtype,) if entry.endswith('_dev') else ()
        geom = (ptr(org),) if '_los_' in entry else (C.c_float(box),)
        return getattr(L, entry)(mode, ptr(x1), ptr(x), ptr(x), ptr(w), ptr(lab1), C.c_int64(n1), ptr(x2), ptr(y2), ptr(z2), ptr(w2),
                                 ptr(lab2), C.c_int64(n2), *dt, nreg, *geom, ptr(b), nb, C.c_float(pimax), npi, C.c_float(mu_max), nmu,
                                 ptr(nfirst), ptr(cnt[1]), ptr(wfirst), ptr(wboth))
    both = [(dict(mode=3), 'unknown mode'), (dict(x1=None), 'null'), (dict(b=None), 'null'), (dict(nb=0), 'nbins'),
            (dict(x2=x, n2=10, lab2=lab), 'y2 / z2'), (dict(x2=x, y2=x, n2=10, lab2=lab), 'y2 / z2'),
            (dict(w2=w), 'w2 given for an autocorrelation'), (dict(lab2=lab), 'labels2 given for an autocorrelation'),
            (dict(lab1=None), 'labels1 is NULL'), (dict(x2=x, y2=x, z2=x, n2=10), 'labels2 is NULL'), (dict(n1=-1), 'point counts'),
            (dict(x2=x, y2=x, z2=x, n2=-1, lab2=lab), 'point counts'), (dict(n1=1 << 31), 'point counts'),
            (dict(nreg=0), 'nreg'), (dict(nreg=65536), 'nreg'), (dict(nreg=60000, npi=200), '2^24'),
            (dict(nfirst=None), 'npairs_first'), (dict(wboth=None), 'go together'), (dict(wfirst=None), 'go together'),
            (dict(npi=3000), 'exceed the LDS histogram'),
            (dict(b=np.array([0.5, 2.0, 2.0], np.float32)), 'increase'), (dict(b=np.array([2.0, 1.0, 3.0], np.float32)), 'increase'),
            (dict(b=np.array([0.5, np.nan, 3.0], np.float32)), 'increase')]
    box = both + [(dict(box=0.0), 'boxsize'), (dict(npi=0), 'pi / mu bin'), (dict(mode=2, nmu=0), 'pi / mu bin'),
                  (dict(wfirst=None, wboth=None), 'wsum_first / wsum_both is NULL'),
                  (dict(b=np.array([0.5, 1.0, 51.0], np.float32)), 'half the box'), (dict(pimax=50.5), 'half the box')]
    los = both + [(dict(npi=0), 'pimax'), (dict(pimax=0.0), 'pimax'), (dict(mode=2, nmu=0), 'mu_max'), (dict(mode=2, mu_max=0.0), 'mu_max'),
                  (dict(org=None), 'null'), (dict(b=np.array([-1.0, 1.0, 3.0], np.float32)), 'negative'),
                  (dict(org=np.array([0.0, np.inf, 0.0])), 'origin'), (dict(org=np.array([np.nan, 0.0, 0.0])), 'origin')]
    for family, rules in (('abacus_paircount_jk', box), ('abacus_paircount_los_jk', los)):
        for entry in (family, family + '_dev'):
            for kw, text in rules:
                _refused(L, entry, call(entry, **kw), text, kw)
        _refused(L, family + '_dev', call(family + '_dev', pos_dtype=7), 'pos_dtype', 'pos_dtype')


def test_box_c_abi_validates_before_the_device():
    """the same for abacus_paircount and abacus_paircount_weighted: the rules they had, and those of the other counters they
    lacked (point counts below zero, y2 / z2 NULL beside x2)"""
    C, L, ptr = _abi()
    x = np.linspace(0.0, 9.0, 10).astype(np.float32)
    w = np.ones(10, np.float32)
    bins = np.array([0.5, 1.0, 2.0], np.float32)
    out, ws, rs = np.zeros(64, np.uint64), np.zeros(64), np.zeros(64)

    def call(entry, mode=1, x1=x, x2=None, y2=None, z2=None, w2=None, n1=10, n2=0, pos_dtype=0, box=100.0, b=bins, nb=2, pimax=4.0,
             npi=4, mu_max=1.0, nmu=4, npairs=out, wsum=ws):
        weighted = 'weighted' in entry
        dt = (pos_dtype,) if entry.endswith('_dev') else ()
        w12, sums = (((ptr(w),), (ptr(w2),)), (ptr(wsum), ptr(rs))) if weighted else (((), ()), ())
        return getattr(L, entry)(mode, ptr(x1), ptr(x), ptr(x), *w12[0], C.c_int64(n1), ptr(x2), ptr(y2), ptr(z2), *w12[1], C.c_int64(n2),
                                 *dt, C.c_float(box), ptr(b), nb, C.c_float(pimax), npi, C.c_float(mu_max), nmu, ptr(npairs), *sums)
    rules = [(dict(mode=3), 'unknown mode'), (dict(x1=None), 'null'), (dict(b=None), 'null'), (dict(npairs=None), 'null'),
             (dict(nb=0), 'nbins'), (dict(box=0.0), 'boxsize'), (dict(box=-1.0), 'boxsize'), (dict(npi=0), 'pi / mu bin'),
             (dict(mode=2, nmu=0), 'pi / mu bin'), (dict(npi=9000), 'exceed the LDS histogram'), (dict(n1=1 << 31), 'point counts'),
             (dict(b=np.array([0.5, 2.0, 2.0], np.float32)), 'increase'), (dict(b=np.array([2.0, 1.0, 3.0], np.float32)), 'increase'),
             (dict(b=np.array([0.5, 1.0, 51.0], np.float32)), 'half the box'), (dict(pimax=50.5), 'half the box'),
             # inherited from the other three drivers
             (dict(n1=-1), 'point counts'), (dict(x2=x, y2=x, z2=x, n2=-1), 'point counts'),
             (dict(x2=x, n2=10), 'y2 / z2'), (dict(x2=x, y2=x, n2=10), 'y2 / z2')]
    weighted_rules = [(dict(wsum=None), 'wsum is NULL'), (dict(w2=w), 'w2 given for an autocorrelation'),
                      (dict(npi=3000), 'exceed the LDS histogram')]
    for family in ('abacus_paircount', 'abacus_paircount_weighted'):
        for entry in (family, family + '_dev'):
            for kw, text in rules + (weighted_rules if 'weighted' in family else []):
                _refused(L, entry, call(entry, **kw), text, kw)
        _refused(L, family + '_dev', call(family + '_dev', pos_dtype=7), 'pos_dtype', 'pos_dtype')
