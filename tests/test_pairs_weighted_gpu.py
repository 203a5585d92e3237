"""Weighted pair counts and mean separations (csrc/pairs.hip: pair_count_w, C ABI abacus_paircount_weighted[_dev]) against
tests/pairs_statement.py - the oracle's pair loop restated in NumPy with float64 weight products - and the weight keywords
of DD / DDrppi / DDsmu, the calc_*_fast wrappers and AbacusHOD.  Needs an MI355X: run with `-m gpu`.

Tolerances (derived, see pairs_statement.bounds): the weight products are exact in float64, so wsum differs from the
statement only by the order of summation, |d wsum| <= n_b 2^-52 sum_b |w_i w_j|; rsum sums float32 square roots,
|d rsum| <= 2^-23 sum_b r (one float32 ulp per term).  Every test prints its largest error in units of the bound.
Observed on an MI355X over all statement cases: wsum 0.16 of its bound at most (weights of mixed sign; 0.033 with positive
weights), rsum equal to the statement's bit for bit (profiles/weighted_pairs/README.md)."""
import functools

import numpy as np
import pytest
from pairs_statement import MODES, bounds, paircount as statement

pytestmark = pytest.mark.gpu

LOGBINS = np.logspace(-1, np.log10(30.0), 14)
SUBKW = {'r': {}, 'rppi': dict(pimax=30.0, npibins=30), 'smu': dict(mu_max=1.0, nmubins=20)}


def _points(n, box, seed, clustered=True):
    """the clustered recipe of tests/test_pairs_gpu.py::_points"""
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3)) * box
    if clustered:
        k = n // 4
        centers = rng.random((20, 3)) * box
        p[:k] = (centers[rng.integers(0, 20, k)] + rng.normal(0, 2.0, (k, 3))) % box
    return [p[:, i].copy() for i in range(3)]


def _frame(cols, frame, box, seed):
    if frame == 'unwrapped':   # coordinates spilling over both box edges, as test_dense_half_stencil_any_frame builds them
        return [v + np.where(np.random.default_rng(seed + s).random(len(v)) < 0.1, box, 0.0) - 20.0 for s, v in enumerate(cols)]
    return [v + frame for v in cols]


def _weights(n, seed, signed=False):
    u = np.random.default_rng(seed).random(n)
    return ((2 * u - 1) if signed else (0.5 + u)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _catalogue(n1, n2, box, frame, auto, clustered=True):
    a = _frame(_points(n1, box, 11, clustered), frame, box, 1)
    b = None if auto else _frame(_points(n2, box, 12, clustered), frame, box, 4)
    return a, b


def _judge(mode, a, b, box, bins, w1, w2, kw, label):
    """the device's three outputs against the statement, itself first pinned to the oracle's integer counts"""
    from abacusutils_amd.analysis.tpcf_corrfunc import _paircount, _paircount_weighted
    from oracle import oracle
    second = (None, None, None) if b is None else b
    n_s, w_s, r_s, wabs = statement(mode, *a, box, bins, *second, w1=w1, w2=w2, **kw)
    np.testing.assert_array_equal(n_s, oracle.paircount_brute(mode, *a, box, bins, *second, nthread=oracle.max_threads(), **kw).ravel())
    assert n_s.sum() > 0
    n, ws, rs = _paircount_weighted(MODES[mode], *a, box, bins, *second, W1=w1, W2=w2, **kw)
    np.testing.assert_array_equal(n, n_s)
    np.testing.assert_array_equal(n, _paircount(MODES[mode], *a, box, bins, *second, **kw))
    bw, br = bounds(n_s, wabs, r_s)
    some = n_s > 0
    ew = np.divide(np.abs(ws - w_s), bw, out=np.zeros_like(bw), where=bw > 0).max()
    er = np.divide(np.abs(rs - r_s), br, out=np.zeros_like(br), where=br > 0).max()
    print(f'{label}: max |d wsum| = {ew:.3g} of its bound, max |d rsum| = {er:.3g} of its bound')
    assert np.all(np.abs(ws - w_s) <= bw), (ws - w_s, bw)
    assert np.all(np.abs(rs - r_s) <= br), (rs - r_s, br)
    assert np.all(ws[~some] == 0) and np.all(rs[~some] == 0)
    # rsum is optional: without it the other two outputs are what they were
    n0, ws0, rs0 = _paircount_weighted(MODES[mode], *a, box, bins, *second, W1=w1, W2=w2, want_rsum=False, **kw)
    assert rs0 is None
    np.testing.assert_array_equal(n0, n_s)
    assert np.all(np.abs(ws0 - w_s) <= bw)
    return n, ws, rs


def _unit(mode, a, b, box, bins, kw):
    """w = 1 passed explicitly: every partial sum is an integer below 2^53, so wsum == npairs exactly"""
    from abacusutils_amd.analysis.tpcf_corrfunc import _paircount, _paircount_weighted
    second = (None, None, None) if b is None else b
    one = lambda c: None if c is None else np.ones(len(c[0]), np.float32)   # noqa: E731
    n, ws, _ = _paircount_weighted(MODES[mode], *a, box, bins, *second, W1=one(a), W2=one(b), **kw)
    np.testing.assert_array_equal(n, _paircount(MODES[mode], *a, box, bins, *second, **kw))
    assert n.sum() > 0
    np.testing.assert_array_equal(ws, n.astype(np.float64))


@pytest.mark.parametrize('frame', [0.0, -100.0, 'unwrapped'])
@pytest.mark.parametrize('auto', [True, False])
@pytest.mark.parametrize('mode', ['r', 'rppi', 'smu'])
def test_statement_sparse(mode, auto, frame):
    """7 points per cell of the reach: a few points of many cells per staging round"""
    a, b = _catalogue(1500, 1200, 200.0, frame, auto)
    w2 = None if auto else _weights(1200, 22)
    _judge(mode, a, b, 200.0, LOGBINS, _weights(1500, 21), w2, SUBKW[mode], f'sparse {mode} auto={auto} frame={frame}')
    _unit(mode, a, b, 200.0, LOGBINS, SUBKW[mode])


@pytest.mark.parametrize('signed', [False, True])
@pytest.mark.parametrize('frame', [0.0, 37.3])
@pytest.mark.parametrize('auto', [True, False])
@pytest.mark.parametrize('mode', ['r', 'rppi', 'smu'])
def test_statement_dense(mode, auto, frame, signed):
    """20 points per cell of the reach (above the 12 at which the unweighted counter turns to its 125-cell stencil: npairs
    is compared with that kernel's), several staging rounds per cell; weights in [0.5, 1.5), then of mixed sign in
    [-1, 1) - cancellation, and the bound is still the one on sum |w w|"""
    a, b = _catalogue(6000, 5000, 200.0, frame, auto)
    w2 = None if auto else _weights(5000, 32, signed)
    _judge(mode, a, b, 200.0, LOGBINS, _weights(6000, 31, signed), w2, SUBKW[mode],
           f'dense {mode} auto={auto} frame={frame} signed={signed}')
    if not signed:
        _unit(mode, a, b, 200.0, LOGBINS, SUBKW[mode])


@pytest.mark.parametrize('auto', [True, False])
@pytest.mark.parametrize('mode', ['r', 'rppi'])
def test_one_cell_per_dimension(mode, auto):
    """reach 40 in a box of 100: fewer than 3 cells fit, every dimension is one cell that is its own neighbour"""
    a, b = _catalogue(1500, 1200, 100.0, 0.0, auto, clustered=False)
    bins = np.linspace(2.0, 40.0, 11)
    kw = dict(pimax=40.0, npibins=40) if mode == 'rppi' else {}
    _judge(mode, a, b, 100.0, bins, _weights(1500, 41), None if auto else _weights(1200, 42), kw, f'one cell {mode} auto={auto}')
    _unit(mode, a, b, 100.0, bins, kw)


@pytest.mark.parametrize('auto', [True, False])
@pytest.mark.parametrize('mode', ['r', 'smu'])
def test_bins_from_zero(mode, auto):
    """linear bins starting at 0: a pair of DISTINCT points at r = 0 is counted (s = 0: mu = 0), a point with itself is not"""
    a, b = _catalogue(1500, 1200, 200.0, 0.0, auto)
    a = [v.copy() for v in a]
    if auto:
        for v in a:
            v[1] = v[0]
    else:
        b = [v.copy() for v in b]
        for v, u in zip(b, a):
            v[0] = u[0]
    bins = np.linspace(0.0, 20.0, 11)
    n, ws, rs = _judge(mode, a, b, 200.0, bins, _weights(1500, 51), None if auto else _weights(1200, 52), SUBKW[mode],
                       f'from zero {mode} auto={auto}')
    assert n[0] >= (2 if auto else 1)


@pytest.mark.parametrize('mode,auto', [('r', True), ('r', False), ('smu', True), ('smu', False)])
def test_more_bins_than_one_launch_holds(mode, auto):
    """70 separation bins (> 63 per launch), and 30 s bins x 100 mu bins = 3000 entries (> the weighted kernel's LDS cap): runs
    of consecutive separation bins.  A fifth of the points sit on a half-integer lattice and one pair is placed ON an edge
    that two runs share (r^2 == edge^2 in float32): it belongs to the upper bin in all three outputs"""
    box = 200.0
    a, b = _catalogue(1500, 1200, box, 0.0, auto)
    a = [v.copy() for v in a]
    for v in a:
        v[:300] = np.round(v[:300] * 2) / 2 % box
    if mode == 'r':
        bins, kw, edge = (0.5 + 0.25 * np.arange(71)).astype(np.float32), {}, 63        # runs of 63 bins
    else:
        bins, kw, edge = (1.0 + 0.5 * np.arange(31)).astype(np.float32), dict(mu_max=1.0, nmubins=100), 20   # runs of <= 20
    tgt = a if auto else [v.copy() for v in b]
    a[0][400], a[1][400], a[2][400] = 10.0, 20.0, 30.0
    tgt[0][401], tgt[1][401], tgt[2][401] = 10.0 + float(bins[edge]), 20.0, 30.0
    if not auto:
        b = tgt
    d = np.float32(a[0][400]) - np.float32(tgt[0][401])
    assert d * d == bins[edge] * bins[edge]
    w1, w2 = _weights(1500, 61), None if auto else _weights(1200, 62)
    n, ws, rs = _judge(mode, a, b, box, bins, w1, w2, kw, f'runs {mode} auto={auto}')
    nsub = kw.get('nmubins', 1)
    assert n[edge * nsub] >= 1 and rs[edge * nsub] >= float(bins[edge])    # mu = 0: sub-bin 0 of the UPPER bin


@pytest.mark.parametrize('mode', ['r', 'rppi'])
@pytest.mark.parametrize('auto', [True, False])
@pytest.mark.parametrize('n', [200000, 199999])
def test_weight_follows_its_point_through_both_sorts(n, auto, mode):
    """200 000 points is the first size sorted by radix sort + gather, 199 999 the last one counting-sorted.  Weights from
    the classes {0, 0.375, 1, 2.5}: wsum_b = sum_uv a_u a_v N_uv(b) with the integer counts N_uv between the class
    sub-catalogues from oracle.paircount_cells; every term is a multiple of 2^-6 far below 2^53, so the equality is EXACT
    whatever the order of summation - a weight attached to the wrong point shows at any size"""
    from abacusutils_amd.analysis.tpcf_corrfunc import _paircount_weighted
    from oracle import oracle
    box, classes = 200.0, np.array([0.0, 0.375, 1.0, 2.5], np.float32)
    bins = np.linspace(1.0, 10.0, 6)
    kw = dict(pimax=10.0, npibins=10) if mode == 'rppi' else {}
    rng = np.random.default_rng(70)
    p1 = (rng.random((200000, 3)) * box)[:n]
    k1 = rng.integers(0, 4, 200000)[:n]
    p2 = None if auto else rng.random((150000, 3)) * box
    k2 = k1 if auto else rng.integers(0, 4, 150000)
    cols = lambda p: [np.ascontiguousarray(p[:, i]) for i in range(3)]   # noqa: E731
    second = (None, None, None) if auto else cols(p2)
    got_n, got_w, _ = _paircount_weighted(MODES[mode], *cols(p1), box, bins, *second, W1=classes[k1],
                                          W2=None if auto else classes[k2], **kw)
    want_w = np.zeros(len(got_w))
    nth = oracle.max_threads()
    q2 = p1 if auto else p2
    for u in range(1, 4):
        for v in range(1, 4):
            if auto and v < u:
                continue
            A, B = p1[k1 == u], q2[k2 == v]
            if auto and u == v:
                c, mult = oracle.paircount_cells(mode, *cols(A), box, bins, nthread=nth, **kw), 1
            else:
                c, mult = oracle.paircount_cells(mode, *cols(A), box, bins, *cols(B), nthread=nth, **kw), (2 if auto else 1)
            want_w += float(classes[u]) * float(classes[v]) * mult * c.ravel().astype(np.float64)
    assert got_n.sum() > 10**6
    np.testing.assert_array_equal(got_w, want_w)


def test_resident_columns():
    """float64 and float32 DeviceArray coordinates in [-L/2, L/2) with host or resident weights: npairs identical to the
    host call, wsum within twice the bound (both sides carry the summation error; positive weights: sum |w w| = wsum)"""
    from abacusutils_amd import _lib
    from abacusutils_amd.analysis.tpcf_corrfunc import _paircount_weighted
    box = 500.0
    rng = np.random.default_rng(3)
    p1 = (rng.random((40000, 3)) - 0.5) * box
    p2 = (rng.random((30000, 3)) - 0.5) * box
    w1, w2 = _weights(40000, 81), _weights(30000, 82)
    bins = np.linspace(0.5, 20.0, 11)
    worst = 0.0
    for dt in (np.float64, np.float32):
        h1 = [np.ascontiguousarray(p1[:, i], dtype=dt) for i in range(3)]
        h2 = [np.ascontiguousarray(p2[:, i], dtype=dt) for i in range(3)]
        d1, d2 = [_lib.DeviceArray(c) for c in h1], [_lib.DeviceArray(c) for c in h2]
        dw1, dw2 = _lib.DeviceArray(w1), _lib.DeviceArray(w2)
        for mode, kw in ((0, {}), (1, dict(pimax=20.0, npibins=20))):
            for second_h, second_d, wh, wd in (((None,) * 3, (None,) * 3, None, None), (h2, d2, w2, dw2)):
                n, ws, rs = _paircount_weighted(mode, *h1, box, bins, *second_h, W1=w1, W2=wh, **kw)
                bound = n.astype(np.float64) * 2.0 ** -52 * ws
                for a1, a2 in ((w1, wh), (dw1, wd)):
                    gn, gw, gr = _paircount_weighted(mode, *d1, box, bins, *second_d, W1=a1, W2=a2, **kw)
                    np.testing.assert_array_equal(gn, n)
                    assert np.all(np.abs(gw - ws) <= 2 * bound)
                    assert np.all(np.abs(gr - rs) <= 2 * 2.0 ** -23 * rs)
                    worst = max(worst, (np.abs(gw - ws)[n > 0] / bound[n > 0]).max())
        for arr in d1 + d2 + [dw1, dw2]:
            arr.free()
    print(f'resident columns: max |d wsum| = {worst:.3g} of the bound')
    with pytest.raises(TypeError):
        _paircount_weighted(0, *h1, box, bins, W1=_lib.DeviceArray(w1))


def test_corrfunc_keywords():
    """DD / DDrppi / DDsmu: weights1, weights2, weight_type, output_*avg - fields, values, errors; nothing asked: today's dtype"""
    from abacusutils_amd.analysis import tpcf_corrfunc as T
    box = 200.0
    a, b = _catalogue(1500, 1200, box, 0.0, False)
    w1, w2 = _weights(1500, 91), _weights(1200, 92)
    bins = np.concatenate([[0.001, 0.002], np.linspace(1.0, 20.0, 6)])       # the first bin stays empty
    geo = dict(periodic=True, boxsize=box)
    calls = {
        'ravg': lambda **k: T.DD(0, 4, bins, *a, X2=b[0], Y2=b[1], Z2=b[2], **geo, **k),
        'rpavg': lambda **k: T.DDrppi(0, 4, binfile=bins, pimax=20.0, X1=a[0], Y1=a[1], Z1=a[2], X2=b[0], Y2=b[1], Z2=b[2], **geo, **k),
        'savg': lambda **k: T.DDsmu(0, 4, bins, 1.0, 10, *a, X2=b[0], Y2=b[1], Z2=b[2], **geo, **k),
    }
    for avg, call in calls.items():
        plain = call()
        assert 'weightavg' not in plain.dtype.names and avg not in plain.dtype.names
        assert plain.dtype.names[:3] == ('rmin', 'rmax', 'npairs') and len(plain.dtype.names) == (3 if avg == 'ravg' else 4)
        mode = {'ravg': 0, 'rpavg': 1, 'savg': 2}[avg]
        kw = {0: {}, 1: dict(pimax=20.0, npibins=20), 2: dict(mu_max=1.0, nmubins=10)}[mode]
        n, ws, rs = T._paircount_weighted(mode, *a, box, bins, *b, W1=w1, W2=w2, **kw)
        res = call(weights1=w1, weights2=w2, weight_type='pair_product', **{'output_' + avg: True})
        assert set(res.dtype.names) == set(plain.dtype.names) | {avg, 'weightavg', 'weightsum'}
        for f in plain.dtype.names:
            np.testing.assert_array_equal(res[f], plain[f])
        some = n > 0
        assert not some[0] and some.sum() > 3
        assert np.all(res['weightavg'][~some] == 0) and np.all(res[avg][~some] == 0) and np.all(res['weightsum'][~some] == 0)
        # the sums are reproducible to their rounding bound only: compare at 1e-12 relative, far above it
        np.testing.assert_allclose(res['weightavg'][some], ws[some] / n[some], rtol=1e-12)
        np.testing.assert_allclose(res[avg][some], rs[some] / n[some], rtol=1e-12)
        np.testing.assert_allclose(res['weightsum'], ws, rtol=1e-12)
        assert np.all((res[avg][some] >= res['rmin'][some]) & (res[avg][some] < res['rmax'][some]))
        # only weights1 for a cross count: unit weights for set 2
        one = call(weights1=w1, weight_type='pair_product')
        n1, ws1, _ = T._paircount_weighted(mode, *a, box, bins, *b, W1=w1, W2=np.ones(1200, np.float32), want_rsum=False, **kw)
        np.testing.assert_allclose(one['weightsum'], ws1, rtol=1e-12)
        assert np.all(one[avg] == 0)                     # not asked for
        # the average alone
        np.testing.assert_allclose(call(**{'output_' + avg: True})[avg][some], rs[some] / n[some], rtol=1e-12)
        with pytest.raises(ValueError, match='weight_type'):
            call(weights1=w1)
        with pytest.raises(NotImplementedError):
            call(weights1=w1, weight_type='pair_sum')
        with pytest.raises(ValueError, match='weights1'):
            call(weights1=w1[:-1], weight_type='pair_product')
        with pytest.raises(ValueError, match='weights2'):
            call(weights1=w1, weights2=w2[:5], weight_type='pair_product')


def test_unit_weights_through_the_estimator():
    """calc_wp_fast(..., w1 = ones) == calc_wp_fast(...) exactly: integer sums, W = N"""
    from abacusutils_amd.analysis import tpcf_corrfunc as T
    a, b = _catalogue(6000, 5000, 200.0, 0.0, False)
    rpbins = np.logspace(-0.5, 1.3, 8)
    one = np.ones(6000, np.float32)
    np.testing.assert_array_equal(T.calc_wp_fast(*a, rpbins, 20, 200.0, 4, w1=one), T.calc_wp_fast(*a, rpbins, 20, 200.0, 4))
    np.testing.assert_array_equal(T.calc_wp_fast(*a, rpbins, 20, 200.0, 4, x2=b[0], y2=b[1], z2=b[2], w1=one),
                                  T.calc_wp_fast(*a, rpbins, 20, 200.0, 4, x2=b[0], y2=b[1], z2=b[2]))
    np.testing.assert_array_equal(T.calc_xirppi_fast(*a, rpbins, 20, 5, 200.0, 4, w1=one), T.calc_xirppi_fast(*a, rpbins, 20, 5, 200.0, 4))
    np.testing.assert_array_equal(T.calc_multipole_fast(*a, rpbins, 200.0, 4, nbins_mu=10, w1=one),
                                  T.calc_multipole_fast(*a, rpbins, 200.0, 4, nbins_mu=10))


def test_abacus_hod_weights():
    """AbacusHOD.compute_wp(weights='w'): the named column of every tracer that has it, unit weights for the others, with the
    coordinates still in HBM; without the keyword a 'w' column is ignored, as the reference ignores it"""
    from test_abacus_hod_gpu import CLUSTERING, HOD_PARAMS

    from abacusutils_amd import synth
    from abacusutils_amd.analysis.tpcf_corrfunc import calc_wp_fast
    from abacusutils_amd.hod.abacus_hod import AbacusHOD
    hd, pd, params = synth.synth_hod_inputs(100000, 100000, seed=19, lbox=1000.0)
    hod = dict(HOD_PARAMS, LRG_params=dict(synth.LRG_PARAMS, logM_cut=12.3, logM1=13.3), ELG_params=dict(synth.ELG_PARAMS))
    ball = AbacusHOD.from_arrays(hd, pd, params, hod, CLUSTERING)
    mock = ball.run_hod()
    base = ball.compute_wp(mock, ball.rpbins, ball.pimax, ball.pi_bin_size)
    w = _weights(len(mock['LRG']['x']), 101)
    mock['LRG']['w'] = w                                   # ELG has no such column: unit weights
    assert mock.device_xyz('LRG') is not None              # a new column leaves the coordinates resident
    same = ball.compute_wp(mock, ball.rpbins, ball.pimax, ball.pi_bin_size)
    got = ball.compute_wp(mock, ball.rpbins, ball.pimax, ball.pi_bin_size, weights='w')
    xyz = {tr: [np.asarray(mock[tr][c]) for c in 'xyz'] for tr in mock}
    for k in base:
        np.testing.assert_array_equal(same[k], base[k])
    args = (ball.rpbins, ball.pimax, ball.lbox, 8)
    want = {'LRG_LRG': calc_wp_fast(*xyz['LRG'], *args, w1=w),
            'LRG_ELG': calc_wp_fast(*xyz['LRG'], *args, x2=xyz['ELG'][0], y2=xyz['ELG'][1], z2=xyz['ELG'][2], w1=w),
            'ELG_ELG': base['ELG_ELG']}
    assert not np.array_equal(got['LRG_LRG'], base['LRG_LRG'])
    # two runs of the same sums differ by the order of their atomics: each bin's DD within n_b 2^-52 (relative, positive
    # weights) of the exact sum, and wp + 2 pimax = 2 sum_pi DD / RR is a sum of positive terms, so the two values lie within
    # 2 * n_b 2^-52 (wp + 2 pimax) of each other; n_b < 10^6 pairs per (rp, pi) bin for the few 10^4 galaxies of this box
    for k, v in want.items():
        assert np.all(np.abs(got[k] - v) <= 2 * 1e6 * 2.0 ** -52 * (np.abs(v) + 2 * ball.pimax)), k
    np.testing.assert_array_equal(got['ELG_LRG'], got['LRG_ELG'])
