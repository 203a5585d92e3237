"""The two geometries of the cell walk (csrc/pairs.hip: pair_count_w on the periodic grid, pair_count_los on the open one) held
to EACH OTHER, on inputs that make the arithmetic of both exact.  Needs an MI355X: run with `-m gpu`.

Coordinates are multiples of 0.25 within [40, 72), weights multiples of 0.5 within [0.5, 4], the squared edges multiples of
1/16: every difference, every squared separation (below 2^12 / 16) and every squared edge is exact in float32 - so the periodic
counter (box 112, reach 9: no minimum image wraps) and the light-cone counter (float64 from the same float32 differences) see
the same numbers - and every product and sum of weights is exact in float64 in any order (multiples of 0.25 far below 2^53).
npairs and weightsum of `DD` and `DD_los` are therefore IDENTICAL arrays, and identical to those of the two statements.  The
separation sums differ (sqrtf against sqrt): each family's is held to its own statement with that statement's own bound."""
import functools

import numpy as np
import pytest
import pairs_los_statement
import pairs_statement

pytestmark = pytest.mark.gpu

BOX = 112.0
EDGES = np.array([0.0, 0.25, 0.5, 1.0, 1.75, 3.0, 5.5, 9.0])


def _lattice(n, lo, hi, seed):
    """n points, one `integers` draw per column in x, y, z order, then the weights"""
    rng = np.random.default_rng(seed)
    cols = [(rng.integers(lo, hi, n) * 0.25).astype(np.float32) for _ in range(3)]
    return cols, (rng.integers(1, 9, n) * 0.5).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(set 1, weights 1, set 2 or None, weights 2 or None)"""
    if name == 'wide_auto':       # 12 periodic cells per dimension, 3 open ones: the open walk skips out-of-range neighbours
        return _lattice(1500, 160, 288, 1) + (None, None)
    if name == 'wide_cross':
        return _lattice(1500, 160, 288, 1) + _lattice(1100, 160, 288, 2)
    # the open grid is ONE cell of 3000 points (twelve slices, twelve candidate rounds); more than a thousand points in one
    # periodic cell (several slices, wrap arithmetic on, nothing wrapped)
    return _lattice(3000, 160, 196, 3) + (None, None)


@pytest.mark.parametrize('name', ['wide_auto', 'wide_cross', 'clumped_auto'])
def test_periodic_and_open_walk_agree(name):
    from abacusutils_amd.analysis.tpcf_corrfunc import DD, DD_los, _paircount_los, _paircount_weighted
    a, w1, b, w2 = _case(name)
    auto = b is None
    second = (None, None, None) if auto else b
    n_p, ws_p, rs_p, wabs_p = pairs_statement.paircount(0, *a, BOX, EDGES, *second, w1=w1, w2=w2)
    n_o, ws_o, rs_o, wabs_o = pairs_los_statement.paircount(0, *a, EDGES, *second, w1=w1, w2=w2)
    # the two statements agree exactly, and every bin but the first of an autocorrelation (no coincident pair is asked for) counts
    np.testing.assert_array_equal(n_p, n_o)
    np.testing.assert_array_equal(ws_p, ws_o)
    print(f'{name}: npairs {n_p.tolist()}')
    assert np.all(n_p[1:] > 0)

    kw = dict(weights1=w1, weight_type='pair_product', output_ravg=True)
    if not auto:
        kw['weights2'] = w2
    box = DD(auto, 1, EDGES, *a, *second, periodic=True, boxsize=BOX, **kw)
    cone = DD_los(auto, 1, EDGES, *a, *second, **kw)
    np.testing.assert_array_equal(box['npairs'], cone['npairs'])
    np.testing.assert_array_equal(box['weightsum'], cone['weightsum'])
    np.testing.assert_array_equal(box['npairs'], n_p)
    np.testing.assert_array_equal(box['weightsum'], ws_p)

    # the separation sums: each family against its own statement
    n, ws, rs = _paircount_weighted(0, *a, BOX, EDGES, *second, W1=w1, W2=w2)
    np.testing.assert_array_equal(n, n_p)
    np.testing.assert_array_equal(ws, ws_p)
    br = pairs_statement.bounds(n_p, wabs_p, rs_p)[1]
    print(f'{name}: periodic max |d rsum| = {np.divide(np.abs(rs - rs_p), br, out=np.zeros_like(br), where=br > 0).max():.3g} of its bound')
    assert np.all(np.abs(rs - rs_p) <= br), (rs - rs_p, br)
    n, ws, rs = _paircount_los(0, *a, EDGES, *second, W1=w1, W2=w2)
    np.testing.assert_array_equal(n, n_o)
    np.testing.assert_array_equal(ws, ws_o)
    br = pairs_los_statement.bounds(n_o, wabs_o, rs_o)[1]
    print(f'{name}: open max |d rsum| = {np.divide(np.abs(rs - rs_o), br, out=np.zeros_like(br), where=br > 0).max():.3g} of its bound')
    assert np.all(np.abs(rs - rs_o) <= br), (rs - rs_o, br)


NREG = 4
TERMS = ('total', 'first', 'second', 'both')


@functools.lru_cache(maxsize=None)
def _turns():
    """the eight calls of test_families_take_turns_on_the_work_buffers as (name, call, statement's (npairs, wsum | None)),
    npairs and wsum of a jackknife call being its four terms side by side"""
    import pairs_jk_statement as jks
    from abacusutils_amd.analysis import jackknife as jk
    from abacusutils_amd.analysis.tpcf_corrfunc import _paircount, _paircount_los, _paircount_weighted
    a, w1, b, w2 = _case('wide_cross')
    la = np.random.default_rng(5).integers(0, NREG, 1500).astype(np.int32)
    lb = np.random.default_rng(6).integers(0, NREG, 1100).astype(np.int32)
    sub = dict(pimax=9.0, npibins=9)

    def plain(res):
        return res[0], res[1]

    def terms(counts):            # a JKCounts, or the dict of the statement
        get = (lambda t, f: counts[t][f]) if isinstance(counts, dict) else (lambda t, f: getattr(getattr(counts, t), f))
        wsum = None if get('total', 'wsum') is None else np.concatenate([np.ravel(get(t, 'wsum')) for t in TERMS])
        return np.concatenate([np.ravel(get(t, 'npairs')) for t in TERMS]), wsum

    def no_sums(res):
        return res[0], None
    box_jk = jks.counts(jks.box(BOX, EDGES, **sub), 'rppi', a, la, NREG, w1=w1)
    cone_x = jks.counts(jks.los(EDGES), 'r', a, la, NREG, b, lb, w1, w2)
    cone_a = jks.counts(jks.los(EDGES), 'r', a, la, NREG)
    for cone, box in ((cone_x, jks.counts(jks.box(BOX, EDGES), 'r', a, la, NREG, b, lb, w1, w2)),
                      (cone_a, jks.counts(jks.box(BOX, EDGES), 'r', a, la, NREG))):
        for t in TERMS:           # the two statements agree bit for bit in every jackknife term
            np.testing.assert_array_equal(cone[t]['npairs'], box[t]['npairs'])
            np.testing.assert_array_equal(cone[t]['wsum'], box[t]['wsum'])
    return (
        ('weighted box cross', lambda: plain(_paircount_weighted(0, *a, BOX, EDGES, *b, W1=w1, W2=w2)),
         plain(pairs_statement.paircount(0, *a, BOX, EDGES, *b, w1=w1, w2=w2))),
        ('light-cone auto of set 2, no sums', lambda: plain(_paircount_los(0, *b, EDGES, want_sums=False)),
         no_sums(pairs_los_statement.paircount(0, *b, EDGES))),
        ('box jackknife auto of set 1, rppi', lambda: terms(jk.paircount_jk('rppi', *a, BOX, EDGES, la, NREG, W1=w1, **sub)), terms(box_jk)),
        ('unweighted box cross, smaller set first', lambda: (_paircount(0, *b, BOX, EDGES, *a), None),
         no_sums(pairs_statement.paircount(0, *b, BOX, EDGES, *a))),
        ('light-cone jackknife cross', lambda: terms(jk.paircount_los_jk('r', *a, EDGES, la, NREG, *b, labels2=lb, W1=w1, W2=w2)),
         terms(cone_x)),
        ('weighted box auto of set 2, no weights', lambda: plain(_paircount_weighted(0, *b, BOX, EDGES)),
         plain(pairs_statement.paircount(0, *b, BOX, EDGES))),
        ('light-cone jackknife auto, no sums', lambda: terms(jk.paircount_los_jk('r', *a, EDGES, la, NREG, want_sums=False)),
         no_sums(terms(cone_a))),
        ('weighted light-cone cross', lambda: plain(_paircount_los(0, *a, EDGES, *b, W1=w1, W2=w2)),
         plain(pairs_los_statement.paircount(0, *a, EDGES, *b, w1=w1, w2=w2))),
    )


def test_families_take_turns_on_the_work_buffers():
    """The four families - plain and jackknife, periodic and open - share the sorted sets, the flag block and the output block of
    one process.  Eight calls that differ in family, sets, weights and outputs, then the same eight in reverse order: every
    result is its statement's, exactly (the lattice makes every product and sum exact in float64), whoever used the buffers
    before - no sorted weight or label column, flag or output size of the previous caller shows"""
    turns = _turns()
    seen = {}
    for name, call, want in turns + turns[::-1]:
        npairs, wsum = call()
        np.testing.assert_array_equal(np.ravel(npairs), np.ravel(want[0]), err_msg=name)
        assert (wsum is None) == (want[1] is None), name
        if wsum is not None:
            np.testing.assert_array_equal(np.ravel(wsum), np.ravel(want[1]), err_msg=name)
        if name in seen:          # the second pass returns what the first did
            np.testing.assert_array_equal(np.ravel(npairs), seen[name][0], err_msg=name)
            assert wsum is None or np.array_equal(np.ravel(wsum), seen[name][1]), name
        seen[name] = (np.ravel(npairs).copy(), None if wsum is None else np.ravel(wsum).copy())
        if name == 'weighted box auto of set 2, no weights':
            np.testing.assert_array_equal(wsum, npairs.astype(np.float64))
        assert np.ravel(want[0]).sum() > 0, name
