"""Light-cone pair counts (csrc/pairs.hip: pair_count_los, C ABI abacus_paircount_los[_dev]) against the NumPy statement
tests/pairs_los_statement.py, and the Landy-Szalay estimators of analysis/tpcf_corrfunc.py against the same estimator
evaluated on statement counts.  Needs an MI355X: run with `-m gpu`.  No Corrfunc run stands behind either side.

Tolerances (derived, pairs_los_statement.bounds): npairs is bit-equal - every expression that decides membership is IEEE
float32 / float64 arithmetic in a fixed order on both sides; the weight products (24 + 24 bits) are exact and the float64
square roots correctly rounded, so wsum and rsum differ by the order of summation only: |d| <= n_b 2^-52 sum_b |term|.
Every test prints its largest error in units of that bound.
Observed on an MI355X over all statement cases: wsum 0.041 of its bound at most, rsum 0.23; the estimators 0.2 of their
tolerance at most (profiles/los_pairs/README.md)."""
import functools

import numpy as np
import pytest
from pairs_los_statement import MODES, bounds, paircount as statement, shell_points

pytestmark = pytest.mark.gpu

ORIGIN = (-990.0, -990.0, -990.0)
LOGBINS = np.logspace(-1, np.log10(30.0), 14)
SUBKW = {'r': {}, 'rppi': dict(pimax=30.0, npibins=30), 'smu': dict(mu_max=1.0, nmubins=20)}


def _weights(n, seed, signed=False):
    u = np.random.default_rng(seed).random(n)
    return ((2 * u - 1) if signed else (0.5 + u)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _shell(n, seed):
    """an octant shell, chi in [1500, 1800] around ORIGIN, float64 box coordinates; half of the points in clumps"""
    return tuple(shell_points(n, seed))


@functools.lru_cache(maxsize=None)
def _cone(n, seed, spread=0.04, chi=(1500.0, 1600.0), clump=0.3):
    """a patch of that shell ~ 2 spread chi wide: dense enough for randoms"""
    return tuple(shell_points(n, seed, chi=chi, spread=spread, clump=clump))


def _grid():
    import ctypes as C
    from abacusutils_amd import _lib
    nc = (C.c_int * 3)()
    _lib.check(_lib.lib().abacus_paircount_los_grid(nc))
    return tuple(nc)


def _judge(mode, a, b, bins, w1, w2, kw, label, origin=ORIGIN, expect_pairs=True):
    """the device's three outputs against the statement; the integer counts also without sums and without rsum"""
    from abacusutils_amd.analysis.tpcf_corrfunc import _paircount_los
    second = (None, None, None) if b is None else b
    n_s, w_s, r_s, wabs = statement(mode, *a, bins, *second, w1=w1, w2=w2, origin=origin, **kw)
    assert n_s.sum() > 0 or not expect_pairs
    n, ws, rs = _paircount_los(MODES[mode], *a, bins, *second, W1=w1, W2=w2, origin=origin, **kw)
    np.testing.assert_array_equal(n, n_s)
    bw, br = bounds(n_s, wabs, r_s)
    ew = np.divide(np.abs(ws - w_s), bw, out=np.zeros_like(bw), where=bw > 0).max()
    er = np.divide(np.abs(rs - r_s), br, out=np.zeros_like(br), where=br > 0).max()
    print(f'{label}: {int(n_s.sum())} pairs, max |d wsum| = {ew:.3g} of its bound, max |d rsum| = {er:.3g} of its bound')
    assert np.all(np.abs(ws - w_s) <= bw), (ws - w_s, bw)
    assert np.all(np.abs(rs - r_s) <= br), (rs - r_s, br)
    none = n_s == 0
    assert np.all(ws[none] == 0) and np.all(rs[none] == 0)
    n0, ws0, rs0 = _paircount_los(MODES[mode], *a, bins, *second, W1=w1, W2=w2, origin=origin, want_rsum=False, **kw)
    assert rs0 is None
    np.testing.assert_array_equal(n0, n_s)
    assert np.all(np.abs(ws0 - w_s) <= bw)
    n1, ws1, rs1 = _paircount_los(MODES[mode], *a, bins, *second, origin=origin, want_sums=False, **kw)
    assert ws1 is None and rs1 is None
    np.testing.assert_array_equal(n1, n_s)          # weighted and unweighted counts are the same pairs
    return n, ws, rs


@pytest.mark.parametrize('auto', [True, False])
@pytest.mark.parametrize('mode', ['r', 'rppi', 'smu'])
def test_statement_octant_shell(mode, auto):
    """3000 (x 2500) points of the octant shell seen from a non-zero origin: an open grid of ~40 cells per dimension, most of
    them empty; float64 host columns"""
    a, b = _shell(3000, 11), None if auto else _shell(2500, 12)
    w2 = None if auto else _weights(2500, 22, signed=True)
    n, ws, _ = _judge(mode, a, b, LOGBINS, _weights(3000, 21), w2, SUBKW[mode], f'shell {mode} auto={auto}')
    assert max(_grid()) > 30
    if auto:
        assert np.all(n % np.uint64(2) == 0)       # ordered pairs: every bin is even


@pytest.mark.parametrize('mode', ['r', 'rppi', 'smu'])
def test_swap_and_unit_weights(mode):
    """swapping the sets of a cross count leaves every count bit-equal (t changes sign, t^2 does not); unit weights passed
    explicitly: every partial sum is an integer below 2^53, wsum == npairs exactly"""
    from abacusutils_amd.analysis.tpcf_corrfunc import _paircount_los
    a, b = _cone(2000, 31), _cone(1500, 32)
    one = lambda c: np.ones(len(c[0]), np.float32)   # noqa: E731
    n_ab, ws, _ = _paircount_los(MODES[mode], *a, LOGBINS, *b, W1=one(a), W2=one(b), origin=ORIGIN, **SUBKW[mode])
    n_ba, _, _ = _paircount_los(MODES[mode], *b, LOGBINS, *a, origin=ORIGIN, want_sums=False, **SUBKW[mode])
    assert n_ab.sum() > 1000
    np.testing.assert_array_equal(n_ab, n_ba)
    np.testing.assert_array_equal(ws, n_ab.astype(np.float64))
    n_aa, _, _ = _paircount_los(MODES[mode], *a, LOGBINS, origin=ORIGIN, want_sums=False, **SUBKW[mode])
    assert n_aa.sum() > 1000 and np.all(n_aa % np.uint64(2) == 0)


def _cube(n, seed, side, centre=(900.0, 1000.0, 1100.0)):
    rng = np.random.default_rng(seed)
    return [np.asarray(c) + ORIGIN[i] + (rng.random(n) - 0.5) * s for i, (c, s) in
            enumerate(zip(centre, np.broadcast_to(side, 3)))]


def test_thin_slab():
    """a slab 5 Mpc/h thin along z: one cell deep, several cells across"""
    a = _cube(3000, 41, (200.0, 150.0, 5.0))
    _judge('rppi', a, None, np.linspace(0.5, 10.0, 8), _weights(3000, 42), None, dict(pimax=10.0, npibins=10), 'thin slab')
    nc = _grid()
    assert nc[2] == 1 and nc[0] > 3 and nc[1] > 3 and nc[0] != nc[1]


@pytest.mark.parametrize('width, cells', [(1.5, 1), (2.5, 2)])
@pytest.mark.parametrize('auto', [True, False])
def test_small_boxes(width, cells, auto):
    """boxes 1.5 and 2.5 reaches wide: 1 and 2 cells per dimension - every cell is at a face of the grid, the clipped stencil
    has 1 and 8 cells - with points exactly on the bounding box's maximum (they belong to the last cell)"""
    kw = dict(pimax=10.0, npibins=10)
    reach = np.sqrt(200.0)
    a = _cube(1500, 51, width * reach)
    hi = [c.max() for c in a]
    for k in range(1, 5):                       # four points on the maximum corner, one more on each maximal face
        for d in range(3):
            a[d][k] = hi[d]
    for d in range(3):
        a[d][5 + d] = hi[d]
    b = None if auto else _cube(1200, 52, width * reach * 0.98)
    bins = np.array([0.0, 0.5, 2.0, 5.0, 10.0])
    _judge('rppi', a, b, bins, _weights(1500, 53), None if auto else _weights(1200, 54), kw, f'{width} reaches auto={auto}')
    assert _grid() == (cells,) * 3
    _judge('r', a, b, bins, _weights(1500, 53), None if auto else _weights(1200, 54), {}, f'{width} reaches (s) auto={auto}')


@pytest.mark.parametrize('mode', ['r', 'rppi', 'smu'])
def test_clump_in_one_cell(mode):
    """700 points within 4 Mpc/h of each other - a few cells at most - over a background: cell slices longer than the 256
    threads of a workgroup and a neighbour list of several rounds (test_small_boxes has 1500 points in ONE cell for certain)"""
    a = [c.copy() for c in _cone(1500, 61)]
    rng = np.random.default_rng(62)
    for c in a:
        c[:700] = c[800] + rng.random(700) * 4.0
    _judge(mode, a, None, LOGBINS, _weights(1500, 63, signed=True), None, SUBKW[mode], f'clump {mode}')


@pytest.mark.parametrize('mode', ['r', 'rppi', 'smu'])
def test_duplicated_points_from_zero(mode):
    """bins from 0 and every fifth point twice: s = 0 pairs of DISTINCT points are counted (pi = 0, rp = 0, mu = 0), a point
    with itself is not"""
    a = [c.copy() for c in _cone(1500, 71)]
    for c in a:
        c[1::5] = c[0::5]
    bins = np.linspace(0.0, 20.0, 11)
    kw = dict(rppi=dict(pimax=20.0, npibins=20)).get(mode, SUBKW[mode])
    n, _, _ = _judge(mode, a, None, bins, _weights(1500, 72), None, kw, f'duplicates {mode}')
    assert n[0] >= 600


@pytest.mark.parametrize('mode', ['r', 'rppi', 'smu'])
def test_antipodal_pairs_have_no_line_of_sight(mode):
    """origin = 0 and every point with its mirror image: the pairs (p, -p) have l = 0 - counted in s, never in (rp, pi) or
    (s, mu); checked on the statement's counts and on a catalogue of antipodal pairs alone"""
    from abacusutils_amd.analysis.tpcf_corrfunc import _paircount_los
    rng = np.random.default_rng(81)
    p = rng.normal(0, 6.0, (400, 3)).astype(np.float32)
    a = [np.concatenate([p[:, d], -p[:, d]]) for d in range(3)]
    bins = np.linspace(0.0, 40.0, 9)
    kw = dict(rppi=dict(pimax=40.0, npibins=40)).get(mode, SUBKW[mode])
    _judge(mode, a, None, bins, _weights(800, 82), None, kw, f'antipodal {mode}', origin=(0.0, 0.0, 0.0))
    far = [np.array([v, -v], np.float32) for v in (3.0, 4.0, 12.0)]      # |p - (-p)| = 26
    n, _, _ = _paircount_los(MODES[mode], *far, bins, want_sums=False, **kw)
    assert n.sum() == (2 if mode == 'r' else 0)


def test_empty_second_set():
    from abacusutils_amd.analysis.tpcf_corrfunc import _paircount_los
    a = _cone(500, 91)
    e = np.zeros(0)
    n, ws, rs = _paircount_los(1, *a, LOGBINS, e, e, e, origin=ORIGIN, **SUBKW['rppi'])
    assert n.shape == (13 * 30,) and not n.any() and not ws.any() and not rs.any()
    n, ws, rs = _paircount_los(1, e, e, e, LOGBINS, *a, origin=ORIGIN, **SUBKW['rppi'])
    assert not n.any() and not ws.any() and not rs.any()


@pytest.mark.parametrize('auto', [True, False])
def test_many_bins_are_counted_in_runs(auto):
    """70 separation bins x 40 pi bins = 2800 histogram entries: more than one launch holds, counted in runs of separation
    bins with a grid each; a pair on an edge shared by two runs belongs to the upper bin"""
    a, b = _cone(2000, 101), None if auto else _cone(1500, 102)
    bins = np.linspace(0.0, 35.0, 71)
    _judge('rppi', a, b, bins, _weights(2000, 103), None if auto else _weights(1500, 104), dict(pimax=40.0, npibins=40),
           f'70 x 40 bins auto={auto}')
    _judge('r', a, b, bins, _weights(2000, 103), None if auto else _weights(1500, 104), {}, f'70 bins auto={auto}')


@pytest.mark.parametrize('mode', ['r', 'rppi', 'smu'])
def test_device_columns(mode):
    """float64 and float32 columns in HBM against float32 host arrays of the same catalogue: bit-equal counts (the float64
    difference of two float32 values is exact, its rounding is the float32 difference), sums within the bound; device and
    host weights"""
    from abacusutils_amd import _lib
    from abacusutils_amd.analysis.tpcf_corrfunc import _paircount_los
    a32 = [c.astype(np.float32) for c in _cone(2000, 111)]
    b32 = [c.astype(np.float32) for c in _cone(1500, 112)]
    w1, w2 = _weights(2000, 113), _weights(1500, 114)
    n_s, w_s, r_s, wabs = statement(mode, *a32, LOGBINS, *b32, w1=w1, w2=w2, origin=ORIGIN, **SUBKW[mode])
    bw, br = bounds(n_s, wabs, r_s)
    host = _paircount_los(MODES[mode], *a32, LOGBINS, *b32, W1=w1, W2=w2, origin=ORIGIN, **SUBKW[mode])
    np.testing.assert_array_equal(host[0], n_s)
    assert n_s.sum() > 1000
    for dt in (np.float64, np.float32):
        da, db = [_lib.DeviceArray(c.astype(dt)) for c in a32], [_lib.DeviceArray(c.astype(dt)) for c in b32]
        dw1 = _lib.DeviceArray(w1)
        try:
            n, ws, rs = _paircount_los(MODES[mode], *da, LOGBINS, *db, W1=dw1, W2=w2, origin=ORIGIN, **SUBKW[mode])
            np.testing.assert_array_equal(n, n_s)
            assert np.all(np.abs(ws - w_s) <= bw) and np.all(np.abs(rs - r_s) <= br)
            n, _, _ = _paircount_los(MODES[mode], *da, LOGBINS, origin=ORIGIN, want_sums=False, **SUBKW[mode])
            np.testing.assert_array_equal(n, _paircount_los(MODES[mode], *a32, LOGBINS, origin=ORIGIN, want_sums=False, **SUBKW[mode])[0])
        finally:
            for d in da + db + [dw1]:
                d.free()
    with pytest.raises(TypeError, match='one dtype'):
        _paircount_los(MODES[mode], _lib.DeviceArray(a32[0]), a32[1], a32[2], LOGBINS, **SUBKW[mode])


def test_radix_sort_path():
    """200 000 points: the cell sort turns to the radix sort; against the counting sort (option pairs_countsort) every count
    is bit-equal.  Bins to 2 Mpc/h keep the pair loop short; no statement at this size."""
    from abacusutils_amd import _lib
    from abacusutils_amd.analysis.tpcf_corrfunc import _paircount_los
    a = _shell(200000, 121)
    w = _weights(200000, 122)
    bins = np.array([0.0, 0.5, 1.0, 2.0])
    kw = dict(pimax=2.0, npibins=2)
    n_radix, ws_radix, _ = _paircount_los(1, *a, bins, W1=w, origin=ORIGIN, **kw)
    assert max(_grid()) == 128
    _lib.set_option('pairs_countsort', 1)
    try:
        n_count, ws_count, _ = _paircount_los(1, *a, bins, W1=w, origin=ORIGIN, **kw)
    finally:
        _lib.set_option('pairs_countsort', 0)
    assert n_radix.sum() > 0
    np.testing.assert_array_equal(n_radix, n_count)
    np.testing.assert_allclose(ws_radix, ws_count, rtol=1e-12)     # the weights travelled with their points on both paths


def test_results_of_the_public_counters():
    """DD_los / DDrppi_los / DDsmu_los and the sky-coordinate wrappers: Corrfunc's structured results on the statement's numbers"""
    from abacusutils_amd.analysis import tpcf_corrfunc as T
    a = _cone(1500, 131)
    w = _weights(1500, 132)
    bins = np.linspace(1.0, 20.0, 6)
    n_s, w_s, r_s, _ = statement('rppi', *a, bins, w1=w, origin=ORIGIN, pimax=10.0, npibins=10)
    res = T.DDrppi_los(1, 1, bins, 10.0, *a, origin=ORIGIN, weights1=w, weight_type='pair_product', output_rpavg=True)
    np.testing.assert_array_equal(res['npairs'], n_s)
    some = n_s > 0
    np.testing.assert_allclose(res['weightavg'][some], (w_s / np.maximum(n_s, 1))[some], rtol=1e-12)
    np.testing.assert_allclose(res['rpavg'][some], (r_s / np.maximum(n_s, 1))[some], rtol=1e-12)
    np.testing.assert_array_equal(res['pimax'][:10], np.arange(1, 11))
    plain = T.DDrppi_los(1, 1, bins, 10.0, *a, origin=ORIGIN)
    assert 'weightavg' not in plain.dtype.names
    np.testing.assert_array_equal(plain['npairs'], n_s)
    np.testing.assert_array_equal(T.DD_los(1, 1, bins, *a, origin=ORIGIN)['npairs'], statement('r', *a, bins, origin=ORIGIN)[0])
    np.testing.assert_array_equal(T.DDsmu_los(1, 1, bins, 1.0, 10, *a, origin=ORIGIN)['npairs'],
                                  statement('smu', *a, bins, origin=ORIGIN, mu_max=1.0, nmubins=10)[0])
    # sky coordinates: the wrapper counts what the statement counts on radec_to_xyz's columns
    p = [c - o for c, o in zip(a, ORIGIN)]
    d = np.sqrt(p[0] ** 2 + p[1] ** 2 + p[2] ** 2)
    ra, dec = np.degrees(np.arctan2(p[1], p[0])), np.degrees(np.arcsin(p[2] / d))
    xyz = T.radec_to_xyz(ra, dec, d)
    res = T.DDrppi_mocks(1, None, 1, 10.0, bins, ra, dec, d, is_comoving_dist=True)
    np.testing.assert_array_equal(res['npairs'], statement('rppi', *xyz, bins, pimax=10.0, npibins=10)[0])
    res = T.DDsmu_mocks(1, None, 1, 1.0, 10, bins, ra, dec, d, is_comoving_dist=True)
    np.testing.assert_array_equal(res['npairs'], statement('smu', *xyz, bins, mu_max=1.0, nmubins=10)[0])


def _close(got, want, label):
    """relative 1e-12 where |xi| is not tiny (above 1e-3 of the largest), absolute 1e-12 max|xi| below"""
    assert got.shape == want.shape and np.all(np.isfinite(want))
    big = np.abs(want).max()
    tol = np.where(np.abs(want) >= 1e-3 * big, 1e-12 * np.abs(want), 1e-12 * big)
    err = np.abs(got - want)
    print(f'{label}: max error {np.max(err / tol):.3g} of the tolerance, max |xi| = {big:.3g}')
    assert np.all(err <= tol), (got, want)


RPBINS, SBINS = np.geomspace(2.0, 25.0, 6), np.geomspace(4.0, 30.0, 6)
LSKW = {'rppi': (RPBINS, dict(pimax=20.0, npibins=20)), 'smu': (SBINS, dict(mu_max=1.0, nmubins=8))}


@functools.lru_cache(maxsize=None)
def _ls_case():
    """two galaxy samples and randoms on one patch; weights for the first sample ('g1w') and for the randoms"""
    cat = {'g1': _cone(1200, 141, clump=0.5), 'g2': _cone(1000, 142, clump=0.5), 'r': _cone(3000, 143, clump=0.0)}
    cat['g1w'] = cat['g1']
    return cat, {'g1': None, 'g2': None, 'g1w': _weights(1200, 144), 'r': _weights(3000, 145)}


@functools.lru_cache(maxsize=None)
def _ls_ws(mode, ka, kb):
    """the statement's weight sums of samples ka x kb (kb None: ka with itself), computed once for all tests"""
    cat, w = _ls_case()
    bins, kw = LSKW[mode]
    second = (None,) * 3 if kb is None else cat[kb]
    return statement(mode, *cat[ka], bins, *second, w1=w[ka], w2=None if kb is None else w[kb], origin=ORIGIN, **kw)[1]


def _ls_statement(mode, k1, k2):
    """the four weight sums of the statement and the normalisations of the Landy-Szalay estimator: Wa Wb for cross counts,
    W^2 - sum w^2 for the ordered autocorrelations"""
    cat, w = _ls_case()
    tot = lambda k: float(len(cat[k][0])) if w[k] is None else float(np.sum(w[k], dtype=np.float64))          # noqa: E731
    sq = lambda k: float(len(cat[k][0])) if w[k] is None else float(np.sum(w[k].astype(np.float64) ** 2))     # noqa: E731
    rr, d1r = _ls_ws(mode, 'r', None), _ls_ws(mode, k1, 'r')
    if k2 is None:
        dd, n12, d2r, n2r = _ls_ws(mode, k1, None), tot(k1) ** 2 - sq(k1), d1r, tot(k1) * tot('r')
    else:
        dd, n12, d2r, n2r = _ls_ws(mode, k1, k2), tot(k1) * tot(k2), _ls_ws(mode, k2, 'r'), tot(k2) * tot('r')
    return (dd, d1r, d2r, rr), (n12, tot(k1) * tot('r'), n2r, tot('r') ** 2 - sq('r'))


@pytest.mark.parametrize('auto', [True, False])
def test_landy_szalay_estimators(auto):
    """calc_xirppi_lc, calc_wp_lc and calc_multipole_lc against the same estimator on statement counts; the RR of the randoms
    is counted once per (mode, bins, pi / mu binning) - the second call launches one pair kernel less"""
    from abacusutils_amd import _lib
    from abacusutils_amd.analysis import tpcf_corrfunc as T
    cat, w = _ls_case()
    g1, w1 = cat['g1w'], w['g1w']
    x2 = {} if auto else dict(zip(('x2', 'y2', 'z2'), cat['g2']))
    k2 = None if auto else 'g2'
    R = T.LCRandoms(*cat['r'], w=w['r'], origin=ORIGIN)
    terms, norms = _ls_statement('rppi', 'g1w', k2)
    _lib.profile_enable(True)
    try:
        _lib.profile_reset()
        got = T.calc_xirppi_lc(*g1, RPBINS, 20, 5, R, w1=w1, origin=ORIGIN, **x2)
        first = _lib.profile_get()['pair_count_los'][1]
        _lib.profile_reset()
        wp = T.calc_wp_lc(*g1, RPBINS, 20, R, w1=w1, origin=ORIGIN, **x2)
        second = _lib.profile_get()['pair_count_los'][1]
    finally:
        _lib.profile_enable(False)
    assert (first, second) == ((3, 2) if auto else (4, 3)) and R.rr_counted == 1
    group = lambda t: t.reshape(5, 4, 5).sum(axis=2)   # noqa: E731
    _close(got, T.landy_szalay(*map(group, terms), *norms), f'xi(rp, pi) auto={auto}')
    _close(wp, 2 * np.sum(T.landy_szalay(*(t.reshape(5, 20) for t in terms), *norms), axis=1), f'wp auto={auto}')
    terms, norms = _ls_statement('smu', 'g1w', k2)
    got = T.calc_multipole_lc(*g1, SBINS, R, nbins_mu=8, orders=[0, 2], w1=w1, origin=ORIGIN, **x2)
    assert R.rr_counted == 2
    xi = T.landy_szalay(*(t.reshape(5, 8) for t in terms), *norms)
    want = np.concatenate([T.tpcf_multipole(xi, np.linspace(0, 1, 9), order=ell) for ell in (0, 2)])
    _close(got, want, f'multipoles auto={auto}')


def test_abacus_hod_compute_wp_with_randoms():
    """AbacusHOD.compute_wp(randoms=...) on a light-cone object: the galaxy columns with the object's origin through
    calc_wp_lc, for the autocorrelations and the cross pair; float64 columns in HBM give the same numbers"""
    from abacusutils_amd import _lib
    from abacusutils_amd.analysis import tpcf_corrfunc as T
    from abacusutils_amd.hod.abacus_hod import AbacusHOD
    cat, w = _ls_case()
    ball = AbacusHOD.__new__(AbacusHOD)
    ball.halo_lc, ball.params, ball.lbox = True, {'origin': np.array(ORIGIN)}, 2000.0
    mock = {'LRG': dict(zip('xyz', cat['g1'])), 'ELG': dict(zip('xyz', cat['g2']))}
    R = T.LCRandoms(*cat['r'], w=w['r'], origin=ORIGIN)
    got = ball.compute_wp(mock, RPBINS, 20, 1, randoms=R)
    assert set(got) == {'LRG_LRG', 'LRG_ELG', 'ELG_LRG', 'ELG_ELG'} and R.rr_counted == 1
    for key, k1, k2 in (('LRG_LRG', 'g1', None), ('ELG_ELG', 'g2', None), ('LRG_ELG', 'g1', 'g2')):
        terms, norms = _ls_statement('rppi', k1, k2)
        _close(got[key], 2 * np.sum(T.landy_szalay(*(t.reshape(5, 20) for t in terms), *norms), axis=1), f'compute_wp {key}')
    dev = [_lib.DeviceArray(c) for c in cat['g1']]
    try:
        np.testing.assert_allclose(T.calc_wp_lc(*dev, RPBINS, 20, R, origin=ORIGIN), got['LRG_LRG'], rtol=1e-12)
    finally:
        for d in dev:
            d.free()
    ball.halo_lc = False
    with pytest.raises(ValueError, match='origin'):
        ball.compute_wp(mock, RPBINS, 20, 1, randoms=R)
