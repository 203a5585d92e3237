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
