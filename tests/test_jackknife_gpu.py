"""Jackknife pair counts (csrc/pairs_jk.hip: pair_count_jk, pair_count_los_jk; C ABI abacus_paircount_jk[_dev],
abacus_paircount_los_jk[_dev], abacus_jk_box_labels_dev) against tests/pairs_jk_statement.py, and the estimators of
abacusutils_amd/analysis/jackknife.py on top.  Needs an MI355X: run with `-m gpu`.

Every (region, bin, sub-bin) is compared: npairs of first / second / both exactly, |d wsum| <= n 2^-52 sum |w_i w_j| per
entry (pairs_statement.bounds: the products are exact in float64, the device differs by the order of summation only, whatever
the number of partial flushes).  Every case prints its largest error in units of that bound.
Observed on an MI355X over all cases: npairs bit-equal, wsum 0.26 of its bound at most (profiles/jackknife/README.md)."""
import ctypes as C
import functools

import numpy as np
import pytest
import pairs_jk_statement as jks
from pairs_los_statement import shell_points

pytestmark = pytest.mark.gpu

BOX = 100.0
LOGBINS = np.logspace(-1, np.log10(11.0), 10)
SUBKW = {'r': {}, 'rppi': dict(pimax=11.0, npibins=11), 'smu': dict(mu_max=1.0, nmubins=8)}
N1, N2 = 3500, 3000
ORIGIN = (-990.0, -990.0, -990.0)


def _jk():
    from abacusutils_amd.analysis import jackknife
    return jackknife


def _points(n, box, seed, clustered=True):
    """the clustered recipe of tests/test_pairs_weighted_gpu.py::_points"""
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3)) * box
    if clustered:
        k = n // 4
        centers = rng.random((20, 3)) * box
        p[:k] = (centers[rng.integers(0, 20, k)] + rng.normal(0, 2.0, (k, 3))) % box
    return [p[:, i].copy() for i in range(3)]


def _weights(n, seed):
    return (2 * np.random.default_rng(seed).random(n) - 1).astype(np.float32)     # mixed sign


def _labels(scheme, cols, seed, box=BOX):
    """(labels, nreg) of a labelling scheme"""
    n = len(cols[0])
    rng = np.random.default_rng(seed)
    if scheme == 'random7':      # every cell slice is many runs, runs end inside slices, the last run is short
        return rng.integers(0, 7, n).astype(np.int32), 7
    if scheme == 'sub222':       # one run per cell, the same label over consecutive cells
        return _jk().box_regions(*cols, box, 2), 8
    if scheme == 'sub321':
        return _jk().box_regions(*cols, box, (3, 2, 1)), 6
    if scheme == 'unused':       # labels 3 and 6 of 7 are carried by no point
        return rng.choice(np.array([0, 1, 2, 4, 5], np.int32), n), 7
    if scheme == 'one':
        return np.zeros(n, np.int32), 1
    raise KeyError(scheme)


@functools.lru_cache(maxsize=None)
def _box_case(mode, auto, scheme, frame=0.0):
    a = [v + frame for v in _points(N1, BOX, 11)]
    b = None if auto else [v + frame for v in _points(N2, BOX, 12)]
    la, nreg = _labels(scheme, a, 5)
    lb = None if auto else _labels(scheme, b, 6)[0]
    w1, w2 = _weights(N1, 21), (None if auto else _weights(N2, 22))
    return a, la, b, lb, w1, w2, nreg, jks.counts(jks.box(BOX, LOGBINS, **SUBKW[mode]), mode, a, la, nreg, b, lb, w1, w2)


WORST = {'wsum': 0.0}


def _compare(got, want, label, weighted=True):
    """a JKCounts against the statement's dict: every entry of every term"""
    nreg = want['first']['npairs'].shape[0]
    worst = 0.0
    for t in ('total', 'first', 'second', 'both'):
        g, w = getattr(got, t), want[t]
        shape = w['npairs'].shape
        np.testing.assert_array_equal(g.npairs.reshape(shape), w['npairs'], err_msg=f'{label} {t}')
        if not weighted:
            assert g.wsum is None
            continue
        # total is the sum of nreg rows, each within its own bound: the bounds add up to at most the whole bin's
        bound = w['npairs'].astype(np.float64) * 2.0 ** -52 * w['wabs']
        err = np.abs(g.wsum.reshape(shape) - w['wsum'])
        worst = max(worst, np.divide(err, bound, out=np.zeros_like(err), where=bound > 0).max())
        assert np.all(err <= bound), (label, t, err.max())
        assert np.all(g.wsum.reshape(shape)[w['npairs'] == 0] == 0)
    WORST['wsum'] = max(WORST['wsum'], worst)
    print(f'{label}: nreg {nreg}, {int(want["total"]["npairs"].sum())} pairs, max |d wsum| = {worst:.3g} of its bound '
          f'(so far over all cases {WORST["wsum"]:.3g})')
    assert want['total']['npairs'].sum() > 0


def _stats():
    from abacusutils_amd import _lib
    cand, fl, wg = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
    _lib.check(_lib.lib().abacus_paircount_stats(C.byref(cand), None, None, None))
    _lib.check(_lib.lib().abacus_paircount_jk_stats(C.byref(fl), C.byref(wg)))
    return cand.value, fl.value, wg.value


BOX_CASES = ([(m, au, 'random7') for m in ('r', 'rppi', 'smu') for au in (True, False)]
             + [(m, True, 'sub222') for m in ('r', 'rppi', 'smu')] + [('rppi', False, 'sub222')]
             + [('r', True, 'sub321'), ('smu', False, 'sub321'), ('rppi', True, 'unused'), ('r', False, 'unused'),
                ('smu', True, 'one'), ('rppi', False, 'one')])


@pytest.mark.parametrize('mode,auto,scheme', BOX_CASES)
def test_box_statement(mode, auto, scheme):
    """3500 (x 3000) points, a quarter clustered, in a box of 100: 9^3 cells, one cell per workgroup"""
    a, la, b, lb, w1, w2, nreg, want = _box_case(mode, auto, scheme)
    got = _jk().paircount_jk(mode, *a, BOX, LOGBINS, la, nreg, *(b or jks.NONE3), labels2=lb, W1=w1, W2=w2, **SUBKW[mode])
    _compare(got, want, f'box {mode} auto={auto} {scheme}')
    if scheme == 'unused':
        for t in (got.first, got.both, got.second):
            assert not t.npairs[[3, 6]].any() and not t.wsum[[3, 6]].any()
    if scheme == 'one':
        np.testing.assert_array_equal(got.first.npairs[0], got.total.npairs)
        np.testing.assert_array_equal(got.both.npairs[0], got.total.npairs)


@pytest.mark.parametrize('mode,auto,scheme', [('rppi', True, 'sub222'), ('r', True, 'sub321'), ('smu', False, 'random7'),
                                              ('rppi', False, 'sub222'), ('r', True, 'random7')])
def test_box_many_cells_per_workgroup(mode, auto, scheme, options):
    """five workgroups for 729 cells, as a large catalogue has many cells per workgroup: the histograms live across cells
    and are flushed when the label changes - with sub-box labels far less often than once per cell"""
    options.set('pairs_jk_grid', 5)
    a, la, b, lb, w1, w2, nreg, want = _box_case(mode, auto, scheme)
    jk = _jk()
    got = jk.paircount_jk(mode, *a, BOX, LOGBINS, la, nreg, *(b or jks.NONE3), labels2=lb, W1=w1, W2=w2, **SUBKW[mode])
    _compare(got, want, f'box, 5 workgroups, {mode} auto={auto} {scheme}')
    single = lambda: jk._jk_counter('paircount_jk', mode, LOGBINS.astype(np.float32), (*a, *(b or jks.NONE3)), (w1, w2), (la, lb), nreg,   # noqa: E731
                                    (C.c_float(BOX),), **dict(dict(pimax=0.0, npibins=0, mu_max=1.0, nmubins=0), **SUBKW[mode]))
    np.testing.assert_array_equal(single()[0], want['first']['npairs'])
    _, flushes, wg = _stats()
    options.set('pairs_jk_grid', 0)      # the default grid: hundreds of workgroups, a cell or two each
    np.testing.assert_array_equal(single()[0], want['first']['npairs'])
    _, many, wg_all = _stats()
    print(f'{scheme}: {flushes} flushes by {wg} workgroups, {many} by {wg_all} workgroups; 729 cells')
    assert wg == 5 and wg_all > 5 and 5 <= flushes <= many
    if scheme != 'random7':
        assert flushes < many            # consecutive cells of one sub-box flush once


@pytest.mark.parametrize('variant', ['dev32', 'dev64', 'dev_labels', 'frame'])
def test_box_columns(variant):
    """DeviceArray columns of both dtypes (host labels and weights uploaded, or resident), and coordinates in another frame"""
    from abacusutils_amd import _lib
    jk = _jk()
    mode = 'rppi'
    a, la, b, lb, w1, w2, nreg, want = _box_case(mode, False, 'random7', 1000.0 if variant == 'frame' else 0.0)
    if variant == 'frame':
        got = jk.paircount_jk(mode, *a, BOX, LOGBINS, la, nreg, *b, labels2=lb, W1=w1, W2=w2, **SUBKW[mode])
    else:
        dt = np.float64 if variant == 'dev64' else np.float32
        da, db = [_lib.DeviceArray(np.asarray(c, dt)) for c in a], [_lib.DeviceArray(np.asarray(c, dt)) for c in b]
        if variant == 'dev_labels':
            la, lb, w1, w2 = _lib.DeviceArray(la), _lib.DeviceArray(lb), _lib.DeviceArray(w1), _lib.DeviceArray(w2)
        before = jk.calls['dev']
        got = jk.paircount_jk(mode, *da, BOX, LOGBINS, la, nreg, *db, labels2=lb, W1=w1, W2=w2, **SUBKW[mode])
        assert jk.calls['dev'] == before + 2
        with pytest.raises(TypeError):
            jk.paircount_jk(mode, *a, BOX, LOGBINS, _lib.DeviceArray(np.zeros(N1, np.int32)), nreg, **SUBKW[mode])
    _compare(got, want, f'box columns {variant}')


def _clump_case(several):
    rng = np.random.default_rng(31)
    bg = _points(1200, BOX, 33, clustered=False)
    clump = 52.0 + rng.normal(0, 0.4, (600, 3))
    a = [np.concatenate((bg[i], clump[:, i])) for i in range(3)]
    if several:                  # 600 points of two labels in one cell: ~300 each, a run goes on across slices and ends inside one
        la = np.concatenate((rng.integers(0, 3, 1200), rng.integers(0, 2, 600))).astype(np.int32)
        return a, la, 3
    return a, _jk().box_regions(*a, BOX, 2), 8     # the clump is one label: more than 256 points of it in a cell


@pytest.mark.parametrize('several', [False, True])
@pytest.mark.parametrize('mode', ['r', 'smu'])
def test_box_clump(mode, several):
    a, la, nreg = _clump_case(several)
    w1 = _weights(1800, 41)
    want = jks.counts(jks.box(BOX, LOGBINS, **SUBKW[mode]), mode, a, la, nreg, w1=w1)
    got = _jk().paircount_jk(mode, *a, BOX, LOGBINS, la, nreg, W1=w1, **SUBKW[mode])
    _compare(got, want, f'clump {mode} several labels={several}')


@pytest.mark.parametrize('auto', [True, False])
@pytest.mark.parametrize('mode', ['r', 'rppi'])
def test_box_one_cell_per_dimension(mode, auto):
    """reach 40 in a box of 100: every dimension is one cell that is its own neighbour; self pairs are excluded by index"""
    a, b = _points(1200, BOX, 51, clustered=False), (None if auto else _points(1000, BOX, 52, clustered=False))
    bins = np.linspace(2.0, 40.0, 8)
    kw = dict(pimax=40.0, npibins=8) if mode == 'rppi' else {}
    la, nreg = _labels('random7', a, 53)
    lb = None if auto else _labels('random7', b, 54)[0]
    w1, w2 = _weights(1200, 55), (None if auto else _weights(1000, 56))
    want = jks.counts(jks.box(BOX, bins, **kw), mode, a, la, nreg, b, lb, w1, w2)
    got = _jk().paircount_jk(mode, *a, BOX, bins, la, nreg, *(b or jks.NONE3), labels2=lb, W1=w1, W2=w2, **kw)
    _compare(got, want, f'one cell per dimension {mode} auto={auto}')


@pytest.mark.parametrize('mode', ['r', 'rppi'])
def test_box_many_bins_are_counted_in_runs(mode):
    """mode r: 70 separation bins (runs of 63 + 7); mode rppi: 30 x 80 = 2400 histogram entries (runs of 25 + 5).  A pair ON
    the edge shared by two runs (separation 8.375 = edge 63 of mode r, 3.5 = edge 25 of mode rppi, exactly) is of the upper bin"""
    a = _points(2000, BOX, 61)
    for c, v in zip(a, ((10.0, 18.375, 30.0, 33.5), (10.0, 10.0, 30.0, 30.0), (10.0, 10.0, 30.0, 30.0))):
        c[:4] = v
    la, nreg = _labels('random7', a, 62)
    la[:4] = (1, 2, 3, 3)
    if mode == 'r':
        bins, kw = 0.5 + 0.125 * np.arange(71), {}
    else:
        bins, kw = 0.375 + 0.125 * np.arange(31), dict(pimax=10.0, npibins=80)
    w1 = _weights(2000, 63)
    want = jks.counts(jks.box(BOX, bins, **kw), mode, a, la, nreg, w1=w1)
    got = _jk().paircount_jk(mode, *a, BOX, bins, la, nreg, W1=w1, **kw)
    _compare(got, want, f'runs {mode}')
    nsub = 80 if mode == 'rppi' else 1
    edge = 63 if mode == 'r' else 25
    assert got.first.npairs.reshape(nreg, -1, nsub)[1 if mode == 'r' else 3, edge, 0] >= 1


@pytest.mark.parametrize('mode', ['r', 'smu'])
def test_box_bins_from_zero_with_duplicates(mode):
    a = _points(1500, BOX, 71)
    for c in a:
        c[100:130] = c[200:230]          # 30 duplicated points: pairs at r = 0, in different regions or the same
    la, nreg = _labels('random7', a, 72)
    bins = np.linspace(0.0, 10.0, 6)
    want = jks.counts(jks.box(BOX, bins, **SUBKW[mode]), mode, a, la, nreg)
    got = _jk().paircount_jk(mode, *a, BOX, bins, la, nreg, **SUBKW[mode])
    _compare(got, want, f'from zero {mode}')
    assert want['total']['npairs'][0] >= 60
    np.testing.assert_array_equal(got.first.wsum, got.first.npairs.astype(np.float64))     # unit weights: exact


def _sectors(cols, nsec):
    """labels by azimuth around the observer: they cut across the cells of the open grid"""
    phi = np.arctan2(np.asarray(cols[1]) - ORIGIN[1], np.asarray(cols[0]) - ORIGIN[0])
    return np.clip((phi / (np.pi / 2) * nsec).astype(np.int32), 0, nsec - 1)


@functools.lru_cache(maxsize=None)
def _los_case(mode, auto, weighted):
    a = shell_points(3000, 11, origin=ORIGIN)
    b = None if auto else shell_points(2500, 12, origin=ORIGIN)
    la, lb = _sectors(a, 6), (None if auto else _sectors(b, 6))
    w1 = _weights(3000, 81) if weighted else None
    w2 = _weights(2500, 82) if weighted and not auto else None
    bins = np.logspace(-1, np.log10(30.0), 10)
    kw = {'r': {}, 'rppi': dict(pimax=30.0, npibins=15), 'smu': dict(mu_max=1.0, nmubins=8)}[mode]
    return a, la, b, lb, w1, w2, bins, kw, jks.counts(jks.los(bins, ORIGIN, **kw), mode, a, la, 6, b, lb, w1, w2)


@pytest.mark.parametrize('mode,auto,weighted', [('rppi', True, False), ('smu', False, True), ('r', True, True), ('rppi', False, False)])
def test_los_statement(mode, auto, weighted, options):
    """3000 (x 2500) points of an octant shell seen from outside it, labels by azimuth sector; unweighted: integer counts
    only (no float64 histograms in LDS).  Once with one cell per workgroup, once with five workgroups for the whole grid"""
    a, la, b, lb, w1, w2, bins, kw, want = _los_case(mode, auto, weighted)
    for grid in (0, 5):
        options.set('pairs_jk_grid', grid)
        got = _jk().paircount_los_jk(mode, *a, bins, la, 6, *(b or jks.NONE3), labels2=lb, W1=w1, W2=w2, origin=ORIGIN,
                                     want_sums=weighted, **kw)
        _compare(got, want, f'los {mode} auto={auto} weighted={weighted} grid={grid}', weighted)
    assert len(np.unique(la)) == 6


@functools.lru_cache(maxsize=None)
def _los_runs_case(mode):
    """the cone of tests/test_pairs_los_gpu.py, five azimuth sectors across it, 70 separation bins: more than one launch holds"""
    kw = dict(chi=(1500.0, 1600.0), spread=0.04, clump=0.3)
    a = shell_points(2000, 101, **kw)
    b = None if mode == 'r' else shell_points(1500, 102, **kw)

    def sectors(cols):
        phi = np.arctan2(np.asarray(cols[1]) - ORIGIN[1], np.asarray(cols[0]) - ORIGIN[0])
        return np.clip(((phi - (np.pi / 4 - 0.08)) / 0.16 * 5).astype(np.int32), 0, 4)
    la, lb = sectors(a), (None if b is None else sectors(b))
    w1 = _weights(2000, 103) if mode == 'r' else None
    bins = np.linspace(0.0, 35.0, 71)
    sub = dict(pimax=40.0, npibins=40) if mode == 'rppi' else {}
    return a, la, b, lb, w1, bins, sub, jks.counts(jks.los(bins, ORIGIN, **sub), mode, a, la, 5, b, lb, w1, None)


@pytest.mark.parametrize('mode,first_run', [('r', 63), ('rppi', 51)])
def test_los_many_bins_are_counted_in_runs(mode, first_run, options):
    """70 separation bins on the light cone: mode r (autocorrelation, signed weights) in runs of 63 + 7 bins, mode rppi (cross
    count, 40 pi bins, integer counts only) in runs of 51 + 19 - each run writes its own columns of the [nreg][ntot] block.
    Every region has pairs on both sides of the boundary, in `first` and in `both`"""
    a, la, b, lb, w1, bins, sub, want = _los_runs_case(mode)
    nsub = sub.get('npibins', 1)
    for term in ('first', 'both'):
        per_bin = want[term]['npairs'].reshape(5, 70, nsub).sum(axis=2)
        assert np.all(per_bin[:, first_run:].sum(axis=1) > 0) and np.all(per_bin[:, :first_run].sum(axis=1) > 0)
    total = want['total']['npairs'].reshape(70, nsub).sum(axis=1)
    assert total[first_run - 1] > 0 and total[first_run] > 0
    for grid in (0, 5):
        options.set('pairs_jk_grid', grid)
        got = _jk().paircount_los_jk(mode, *a, bins, la, 5, *(b or jks.NONE3), labels2=lb, W1=w1, origin=ORIGIN,
                                     want_sums=mode == 'r', **sub)
        _compare(got, want, f'los runs {mode} grid={grid}', weighted=mode == 'r')


def test_los_device_columns():
    from abacusutils_amd import _lib
    a, la, b, lb, w1, w2, bins, kw, want = _los_case('smu', False, True)
    da, db = [_lib.DeviceArray(np.asarray(c, np.float64)) for c in a], [_lib.DeviceArray(np.asarray(c, np.float64)) for c in b]
    got = _jk().paircount_los_jk('smu', *da, bins, _lib.DeviceArray(la), 6, *db, labels2=lb, W1=w1, W2=w2, origin=ORIGIN, **kw)
    _compare(got, want, 'los device columns')


@pytest.mark.parametrize('auto', [True, False])
@pytest.mark.parametrize('mode', ['r', 'rppi', 'smu'])
def test_total_and_candidates_are_the_parents(mode, auto):
    """total = the weighted / light-cone counter's result on the same input (npairs bit for bit), and so is the candidate count"""
    from abacusutils_amd.analysis.tpcf_corrfunc import _paircount_los, _paircount_weighted
    jk = _jk()
    a, la, b, lb, w1, w2, nreg, want = _box_case(mode, auto, 'random7')
    second = b or jks.NONE3
    n, ws, _ = _paircount_weighted(jks.pairs_statement.MODES[mode], *a, BOX, LOGBINS, *second, W1=w1, W2=w2, **SUBKW[mode])
    cand = _stats()[0]
    kw = dict(dict(pimax=0.0, npibins=0, mu_max=1.0, nmubins=0), **SUBKW[mode])
    raw = jk._jk_counter('paircount_jk', mode, LOGBINS.astype(np.float32), (*a, *second), (w1, w2), (la, lb), nreg, (C.c_float(BOX),), **kw)
    assert _stats()[0] == cand and cand > 0
    np.testing.assert_array_equal(raw[0].sum(axis=0, dtype=np.uint64), n)
    bound = n.astype(np.float64) * 2.0 ** -51 * want['total']['wabs']
    assert np.all(np.abs(raw[2].sum(axis=0) - ws) <= bound)
    los_cases = {('rppi', True): False, ('smu', False): True, ('r', True): True, ('rppi', False): False}   # those of test_los_statement
    if (mode, auto) not in los_cases:
        return
    a, la, b, lb, w1, w2, bins, lkw, want = _los_case(mode, auto, los_cases[(mode, auto)])
    second = b or jks.NONE3
    n = _paircount_los(jks.pairs_statement.MODES[mode], *a, bins, *second, origin=ORIGIN, want_sums=False, **lkw)[0]
    cand = _stats()[0]
    kw = dict(dict(pimax=0.0, npibins=0, mu_max=1.0, nmubins=0), **lkw)
    centred = [None if c is None else (np.asarray(c) - o).astype(np.float32) for c, o in zip((*a, *second), ORIGIN * 2)]
    zero = np.zeros(3)
    raw = jk._jk_counter('paircount_los_jk', mode, bins.astype(np.float32), centred, (None, None), (la, lb), 6, (jk.ptr(zero),),
                         want_sums=False, **kw)
    assert _stats()[0] == cand and cand > 0
    np.testing.assert_array_equal(raw[0].sum(axis=0, dtype=np.uint64), n)


def test_error_paths_leave_the_device_usable():
    from abacusutils_amd._lib import AbacusHipError
    jk = _jk()
    a, la, b, lb, w1, w2, nreg, want = _box_case('r', False, 'random7')
    good = lambda: _compare(jk.paircount_jk('r', *a, BOX, LOGBINS, la, nreg, *b, labels2=lb, W1=w1, W2=w2), want, 'after an error')   # noqa: E731
    bad = la.copy()
    for value, text in ((-1, r'labels span \[-1, 6\]'), (7, r'labels span \[0, 7\]')):
        bad[1234] = value
        with pytest.raises(AbacusHipError, match=text):
            jk.paircount_jk('r', *a, BOX, LOGBINS, bad, nreg, *b, labels2=lb)
        with pytest.raises(AbacusHipError, match='labels span'):          # in the second set, and on the light cone
            jk.paircount_jk('r', *b, BOX, LOGBINS, lb, nreg, *a, labels2=bad)
        with pytest.raises(AbacusHipError, match='labels span'):
            jk.paircount_los_jk('r', *a, LOGBINS, bad, nreg, origin=ORIGIN)
        good()
    for n_bad in (0, 65536):
        with pytest.raises(AbacusHipError, match='nreg'):
            jk.paircount_jk('r', *a, BOX, LOGBINS, la, n_bad, *b, labels2=lb)
        with pytest.raises(AbacusHipError, match='nreg'):
            jk.paircount_los_jk('r', *a, LOGBINS, la, n_bad)
    with pytest.raises(AbacusHipError, match='2\\^24'):
        jk.paircount_jk('rppi', *a, BOX, LOGBINS, la, 60000, pimax=11.0, npibins=40)      # 60000 x 9 x 40 entries
    with pytest.raises(AbacusHipError, match='2\\^24'):
        jk.paircount_los_jk('rppi', *a, LOGBINS, la, 60000, pimax=11.0, npibins=40)
    with pytest.raises(ValueError, match='labels2 given for an autocorrelation'):
        jk.paircount_jk('r', *a, BOX, LOGBINS, la, nreg, labels2=la)
    raw_args = dict(pimax=0.0, npibins=0, mu_max=1.0, nmubins=0)
    with pytest.raises(ValueError, match='labels1 has shape'):
        jk.paircount_jk('r', *a, BOX, LOGBINS, la[:-1], nreg)
    with pytest.raises(ValueError, match='labels2 has shape'):
        jk.paircount_jk('r', *a, BOX, LOGBINS, la, nreg, *b, labels2=lb[:-1])
    # the C ABI itself refuses labels2 without a second set
    from abacusutils_amd import _lib
    f4 = [np.ascontiguousarray(c, np.float32) for c in a]
    out = [np.zeros(nreg * 9, np.uint64), np.zeros(nreg * 9, np.uint64), np.zeros(nreg * 9), np.zeros(nreg * 9)]
    bins = LOGBINS.astype(np.float32)
    rc = _lib.lib().abacus_paircount_jk(0, *map(_lib.ptr, f4), None, _lib.ptr(la), C.c_int64(N1), None, None, None, None, _lib.ptr(la),
                                        C.c_int64(0), nreg, C.c_float(BOX), _lib.ptr(bins), 9, C.c_float(0), 0, C.c_float(1), 0,
                                        *map(_lib.ptr, out))
    assert rc != 0 and b'labels2 given for an autocorrelation' in _lib.lib().abacus_last_error()
    assert raw_args
    good()


def test_box_regions_on_resident_columns():
    from abacusutils_amd import _lib
    jk = _jk()
    rng = np.random.default_rng(91)
    L = 100.0
    below = np.nextafter(np.float32(L), np.float32(0))
    edge = np.array([0.0, below, L, -1e-6, -30.0, 130.0, 250.0, 99.9999999, 33.333333, 66.666666, 50.0, 1e-30], np.float64)
    x = np.concatenate((edge, rng.random(5000) * 3 * L - L))
    y, z = rng.permutation(x), rng.permutation(x)
    for dt in (np.float32, np.float64):
        cols = [np.asarray(c, dt) for c in (x, y, z)]
        for nsplit in (5, (3, 2, 1), (1, 1, 7)):
            host = jk.box_regions(*cols, L, nsplit)
            dev = jk.box_regions(*[_lib.DeviceArray(c) for c in cols], L, nsplit)
            assert dev.dtype == np.int32
            np.testing.assert_array_equal(dev.get(), host)
            nreg = int(np.prod(jk._split(nsplit)))
            assert host.min() >= 0 and host.max() < nreg
    lab = jk.box_regions(np.asarray(edge, np.float64), np.zeros(12), np.zeros(12), L, (4, 1, 1))
    np.testing.assert_array_equal(lab[:3], [0, 3, 0])           # x = L lands in the first sub-box, not in sub-box 4


# ----------------------------------------------------------------------------------------------------- estimators ----
RP = np.logspace(-1, np.log10(11.0), 10)


@pytest.mark.parametrize('auto', [True, False])
def test_box_estimators_full_is_the_fast_result(auto):
    from abacusutils_amd.analysis import tpcf_corrfunc as tc
    jk = _jk()
    a, la, b, lb, _, _, nreg, _ = _box_case('rppi', auto, 'sub222')
    kw = {} if auto else dict(x2=b[0], y2=b[1], z2=b[2])
    jkw = dict(kw, regions2=lb)
    full, samples, cov = jk.calc_wp_jk(*a, RP, 11, BOX, 1, la, nreg, **jkw)
    np.testing.assert_array_equal(full, tc.calc_wp_fast(*a, RP, 11, BOX, 1, **kw))
    assert samples.shape == (nreg, 9) and cov.shape == (9, 9) and np.all(np.isfinite(cov))
    full, samples, cov = jk.calc_xirppi_jk(*a, RP, 10, 5, BOX, 1, la, nreg, **jkw)
    np.testing.assert_array_equal(full, tc.calc_xirppi_fast(*a, RP, 10, 5, BOX, 1, **kw))
    assert full.shape == (9, 2) and samples.shape == (nreg, 18) and cov.shape == (18, 18)
    sb = np.linspace(0.5, 11.0, 8)
    full, samples, cov = jk.calc_multipole_jk(*a, sb, BOX, 1, la, nreg, nbins_mu=8, **jkw)
    np.testing.assert_array_equal(full, tc.calc_multipole_fast(*a, sb, BOX, 1, nbins_mu=8, **kw))
    assert samples.shape == (nreg, 14) and cov.shape == (14, 14)
    assert np.all(np.linalg.eigvalsh(cov) >= -1e-10 * np.abs(cov).max())


@pytest.mark.parametrize('auto,weighted', [(True, False), (False, False), (False, True)])
def test_box_samples_are_the_host_formula_on_statement_counts(auto, weighted):
    """xi_-k = (total - (first_k + second_k) / 2) / (RR (1 - W1_k / 2 W1 - W2_k / 2 W2)) - 1 on the statement's counts.
    Unweighted the counts are exact integers and only the order of the float64 estimator arithmetic differs: 1e-12."""
    jk = _jk()
    a, la, b, lb, w1, w2, nreg, want = _box_case('rppi', auto, 'random7')
    if weighted:                          # positive weights: the estimator divides by their sums
        w1, w2 = np.abs(w1) + 0.5, np.abs(w2) + 0.5
        want = jks.counts(jks.box(BOX, LOGBINS, **SUBKW['rppi']), 'rppi', a, la, nreg, b, lb, w1, w2)
    kw = {} if auto else dict(x2=b[0], y2=b[1], z2=b[2], regions2=lb)
    if weighted:
        kw.update(w1=w1, w2=w2)
    full, samples, cov = jk.calc_wp_jk(*a, RP, 11, BOX, 1, la, nreg, **kw)
    c = jks.pick(want, 'wsum' if weighted else 'npairs')
    e = RP.astype(np.float32)
    v1 = w1.astype(np.float64) if weighted else np.ones(N1)
    v2 = v1 if auto else (w2.astype(np.float64) if weighted else np.ones(N2))
    l2 = la if auto else lb
    # RR as `_natural_estimator` forms it: float32 bins and box, the sums of the weights as Python floats
    rr = (np.pi * (e[1:] ** 2 - e[:-1] ** 2) / np.float32(BOX) ** 3 * float(v1.sum()) * float(v2.sum()) * 2).astype(np.float64)
    # weighted: wsum differs from the statement by the order of summation, n 2^-52 < 1e5 * 2.3e-16 = 2.3e-11 of a bin of
    # positive terms, and xi = D / RR - 1 summed to wp amplifies that by (1 + xi) / wp < 50: 1e-9
    rtol = 1e-9 if weighted else 1e-12
    for k in range(nreg):
        d = c['total'].astype(np.float64) - 0.5 * (c['first'][k].astype(np.float64) + c['second'][k])
        f = 1 - 0.5 * v1[la == k].sum() / v1.sum() - 0.5 * v2[l2 == k].sum() / v2.sum()
        xi = d.reshape(9, 11) / (rr * f)[:, None] - 1
        np.testing.assert_allclose(samples[k], 2 * xi.sum(axis=1), rtol=rtol, atol=0)
    np.testing.assert_allclose(cov, jk.jackknife_covariance(samples))


def _lc_data():
    data = shell_points(1500, 21, chi=(1500.0, 1600.0), origin=ORIGIN, spread=0.04, clump=0.3)
    rand = shell_points(3000, 22, chi=(1500.0, 1600.0), origin=ORIGIN, spread=0.04, clump=0.0)
    # four sectors of the patch by the sign of two coordinates relative to its centre
    centre = [np.median(c) for c in rand]
    lab = lambda cols: ((np.asarray(cols[0]) > centre[0]).astype(np.int32) * 2 + (np.asarray(cols[1]) > centre[1]))   # noqa: E731
    return data, lab(data), rand, lab(rand)


def test_light_cone_samples_are_the_estimator_without_the_region():
    """unit weights, cross_weight 1: every sum is an exact integer in float64 and the same landy_szalay forms both, so sample
    k is bit-equal to calc_wp_lc / calc_multipole_lc on data and randoms without region k.  The per-region RR is counted once"""
    from abacusutils_amd.analysis import tpcf_corrfunc as tc
    jk = _jk()
    data, ld, rand, lr = _lc_data()
    data2 = shell_points(1200, 23, chi=(1500.0, 1600.0), origin=ORIGIN, spread=0.04, clump=0.3)
    l2 = ((np.asarray(data2[0]) > np.median(rand[0])).astype(np.int32) * 2 + (np.asarray(data2[1]) > np.median(rand[1])))
    rp = np.logspace(0.0, np.log10(20.0), 7)
    randoms = jk.LCRandomsJK(*rand, lr, 4, origin=ORIGIN)
    full, samples, cov = jk.calc_wp_lc_jk(*data, rp, 20, randoms, ld, 4, origin=ORIGIN)
    assert randoms.rr_jk_counted == 1
    plain = tc.LCRandoms(*rand, origin=ORIGIN)
    np.testing.assert_array_equal(full, tc.calc_wp_lc(*data, rp, 20, plain, origin=ORIGIN))
    cut = lambda cols, lab, k: [np.asarray(c)[lab != k] for c in cols]   # noqa: E731
    for k in range(4):
        rk = tc.LCRandoms(*cut(rand, lr, k), origin=ORIGIN)
        np.testing.assert_array_equal(samples[k], tc.calc_wp_lc(*cut(data, ld, k), rp, 20, rk, origin=ORIGIN), err_msg=f'wp, region {k}')
    assert samples.shape == (4, 6) and cov.shape == (6, 6)
    # a cross count on the same randoms and binning: RR comes from the cache
    fullx, samplesx, _ = jk.calc_wp_lc_jk(*data, rp, 20, randoms, ld, 4, x2=data2[0], y2=data2[1], z2=data2[2], regions2=l2, origin=ORIGIN)
    assert randoms.rr_jk_counted == 1
    for k in (0, 3):
        rk = tc.LCRandoms(*cut(rand, lr, k), origin=ORIGIN)
        d2 = cut(data2, l2, k)
        np.testing.assert_array_equal(samplesx[k], tc.calc_wp_lc(*cut(data, ld, k), rp, 20, rk, x2=d2[0], y2=d2[1], z2=d2[2], origin=ORIGIN))
    sb = np.linspace(2.0, 20.0, 6)
    full, samples, cov = jk.calc_multipole_lc_jk(*data, sb, randoms, ld, 4, nbins_mu=6, origin=ORIGIN)
    assert randoms.rr_jk_counted == 2
    for k in (1, 2):
        rk = tc.LCRandoms(*cut(rand, lr, k), origin=ORIGIN)
        np.testing.assert_array_equal(samples[k], tc.calc_multipole_lc(*cut(data, ld, k), sb, rk, nbins_mu=6, origin=ORIGIN))
    full, samples, cov = jk.calc_xirppi_lc_jk(*data, rp, 20, 5, randoms, ld, 4, origin=ORIGIN, w1=np.full(1500, 0.5, np.float32))
    np.testing.assert_allclose(full, tc.calc_xirppi_lc(*data, rp, 20, 5, plain, origin=ORIGIN), rtol=1e-12)   # a constant weight drops out
    assert full.shape == (6, 4) and samples.shape == (4, 24)
    # a region without any point
    with pytest.raises(ValueError, match=r'regions \[4\]'):
        jk.calc_wp_lc_jk(*data, rp, 20, jk.LCRandomsJK(*rand, lr, 5, origin=ORIGIN), ld, 5, origin=ORIGIN)
    with pytest.raises(TypeError):
        jk.calc_wp_lc_jk(*data, rp, 20, plain, ld, 4, origin=ORIGIN)


def test_abacus_hod_compute_jackknife():
    """the catalogue of run_hod, still in HBM: labels from abacus_jk_box_labels_dev, counts from abacus_paircount_jk_dev"""
    from abacusutils_amd import synth
    from abacusutils_amd.hod.abacus_hod import AbacusHOD
    from test_abacus_hod_gpu import CLUSTERING, HOD_PARAMS
    jk = _jk()
    hd, pd, params = synth.synth_hod_inputs(300000, 300000, seed=9, lbox=1000.0)
    hod = dict(HOD_PARAMS, LRG_params=dict(synth.LRG_PARAMS, logM_cut=12.3, logM1=13.3), ELG_params=dict(synth.ELG_PARAMS))
    ball = AbacusHOD.from_arrays(hd, pd, params, hod, CLUSTERING)
    mock = ball.run_hod()
    assert all(mock.device_xyz(tr) is not None for tr in mock)
    before = dict(jk.calls)
    res = ball.compute_jackknife(mock, 'wp', 2, ball.rpbins, ball.pimax, ball.pi_bin_size)
    assert jk.calls['host'] == before['host'] and jk.calls['dev'] == before['dev'] + 4       # LRG, ELG, and LRG x ELG both ways
    wp = ball.compute_wp(mock, ball.rpbins, ball.pimax, ball.pi_bin_size)
    assert set(res) == set(wp)
    for pair in wp:
        full, samples, cov = res[pair]
        np.testing.assert_array_equal(full, wp[pair], err_msg=pair)
        assert samples.shape == (8, 9) and cov.shape == (9, 9)
    x, y, z = (mock['LRG'][c] for c in 'xyz')
    lab = jk.box_regions(x, y, z, ball.lbox, 2)
    np.testing.assert_array_equal(np.unique(lab), np.arange(8))
    want = jk.calc_wp_jk(x, y, z, ball.rpbins, ball.pimax, ball.lbox, 1, lab, 8)
    np.testing.assert_array_equal(res['LRG_LRG'][1], want[1])
    x2, y2, z2 = (mock['ELG'][c] for c in 'xyz')
    want = jk.calc_wp_jk(x, y, z, ball.rpbins, ball.pimax, ball.lbox, 1, lab, 8, x2=x2, y2=y2, z2=z2,
                         regions2=jk.box_regions(x2, y2, z2, ball.lbox, 2))
    np.testing.assert_array_equal(res['LRG_ELG'][1], want[1])
    multi = ball.compute_jackknife(mock, 'multipole', (2, 2, 1), ball.rpbins, ball.pimax, np.linspace(0.5, 30.0, 8), 10)
    np.testing.assert_array_equal(multi['ELG_ELG'][0], ball.compute_multipole(mock, ball.rpbins, ball.pimax, np.linspace(0.5, 30.0, 8), 10)['ELG_ELG'])
    assert multi['ELG_ELG'][1].shape == (4, 9 + 14)
    with pytest.raises(ValueError):
        ball.compute_jackknife(mock, 'power', 2)
