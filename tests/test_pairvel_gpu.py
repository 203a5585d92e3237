"""Pairwise velocity sums on the device (csrc/pairs.hip: pair_vel, C ABI abacus_pairvel[_dev], analysis/pairwise_velocity.py,
AbacusHOD.compute_pairwise_velocity) against the NumPy statement tests/pairvel_statement.py.  Needs an MI355X: run with `-m gpu`.

Judging, per (bin, sub-bin), every ratio printed: npairs exact; wsum as tests/test_pairs_weighted_gpu.py judges it,
|d wsum| <= n 2^-52 sum |w w|; each of the five velocity sums |device - statement| <= (n + 8) 2^-52 sum |term|
(pairvel_statement.bound: n float64 additions in any order, and a square root and a division that may each be an ulp from
NumPy's).  Observed on an MI355X: profiles/pairvel/README.md."""
import ctypes as C
import functools

import numpy as np
import pytest
from pairvel_statement import SUMS, bound, pairvel as statement, velocities
from test_pairs_weighted_gpu import _frame, _points, _weights

pytestmark = pytest.mark.gpu

ALL = ('npairs', 'wsum') + SUMS
BOX = 100.0
EDGES = np.geomspace(0.5, 20.0, 9).astype(np.float32)
SUBKW = {'r': {}, 'rppi': dict(pimax=20.0, npibins=4), 'smu': dict(mu_max=1.0, nmubins=5)}
FRAMES = {'box': 0.0, 'centred': -50.0, 'unwrapped': 'unwrapped'}


@functools.lru_cache(maxsize=None)
def _set(n, seed, frame='box'):
    """(six float64 position / float32 velocity columns, signed float32 weights) of the clustered catalogue in a frame; the
    velocities are those of the points, whatever the frame"""
    p = _points(n, BOX, seed)
    return _frame(p, FRAMES[frame], BOX, seed) + velocities(p, BOX, seed + 100), _weights(n, seed + 200, signed=True)


def _candidates():
    from abacusutils_amd import _lib
    c = C.c_uint64(0)
    _lib.check(_lib.lib().abacus_paircount_stats(C.byref(c), None, None, None))
    return c.value


def _device(mode, c1, w1, c2, w2, bins, kw, box=BOX):
    from abacusutils_amd.analysis.pairwise_velocity import pairwise_velocity_sums
    second = {} if c2 is None else dict(zip(('X2', 'Y2', 'Z2', 'VX2', 'VY2', 'VZ2'), c2))
    return pairwise_velocity_sums(mode, *c1, box, bins, **second, W1=w1, W2=w2, **kw)


def _compare(got, want, scale, label):
    np.testing.assert_array_equal(got['npairs'], want['npairs'])
    n = want['npairs'].astype(np.float64)
    worst = {}
    for k in ('wsum',) + SUMS:
        b = n * 2.0 ** -52 * scale[k] if k == 'wsum' else bound(want['npairs'], scale[k])
        err = np.abs(got[k] - want[k])
        worst[k] = np.divide(err, b, out=np.zeros_like(b), where=b > 0).max() if b.size else 0.0
    print(f'{label}: ' + ', '.join(f'{k} {worst[k]:.3g}' for k in worst) + ' of the bound')
    for k in ('wsum',) + SUMS:
        b = n * 2.0 ** -52 * scale[k] if k == 'wsum' else bound(want['npairs'], scale[k])
        assert np.all(np.abs(got[k] - want[k]) <= b), (label, k, got[k] - want[k], b)
        assert np.all(got[k][want['npairs'] == 0] == 0), (label, k)


def _judge(mode, s1, s2, bins, kw, label, flavours=('host',), box=BOX):
    """the device's seven sums against the statement, for every way of handing the columns over"""
    from abacusutils_amd._lib import DeviceArray
    (c1, w1), (c2, w2) = s1, (s2 if s2 is not None else (None, None))
    want, scale = statement(mode, *c1, box, bins, *(c2 or ()), w1=w1, w2=w2, **kw)
    n1, n2 = len(c1[0]), len(c1[0] if c2 is None else c2[0])
    for fl in flavours:
        if fl == 'host':
            got = _device(mode, c1, w1, c2, w2, bins, kw, box)
        else:
            dt = np.float32 if 'f32' in fl else np.float64
            up = lambda cols: None if cols is None else [DeviceArray(np.asarray(c, dtype=dt)) for c in cols]   # noqa: E731
            upw = lambda w: DeviceArray(w) if w is not None and 'resident' in fl else w                        # noqa: E731
            d1, d2 = up(c1), up(c2)
            got = _device(mode, d1, upw(w1), d2, upw(w2), bins, kw, box)
        if n1 * n2 >= 300 * 3000:
            assert 0 < _candidates() < n1 * n2, 'a walk over neighbour cells, not over the box'
        _compare(got, want, scale, f'{label} [{fl}]')
    return want


ALL_FLAVOURS = ('host', 'f32', 'f32 resident', 'f64', 'f64 resident')


@pytest.mark.parametrize('frame', list(FRAMES))
@pytest.mark.parametrize('auto', [True, False])
@pytest.mark.parametrize('mode', ['r', 'rppi', 'smu'])
def test_statement(mode, auto, frame):
    """the 3000-point catalogue with itself and 300 x 3000, every mode, three coordinate frames, five ways of passing columns"""
    big, small = _set(3000, 81, frame), _set(300, 82, frame)
    want = _judge(mode, big if auto else small, None if auto else big, EDGES, SUBKW[mode], f'{mode} auto={auto} {frame}', ALL_FLAVOURS)
    if frame == 'box':
        assert np.count_nonzero(want['npairs'] == 0) == (6 if (mode == 'smu' and not auto) else 0)


@pytest.mark.parametrize('mode', ['r', 'rppi', 'smu'])
def test_unit_weights_and_zero_velocities(mode):
    (c, _), (c2, _) = _set(3000, 81), _set(300, 82)
    zero = lambda cols: cols[:3] + [np.zeros(len(cols[0]), np.float32)] * 3   # noqa: E731
    for second in (None, zero(c)):
        first = zero(c) if second is None else zero(c2)
        n = len(first[0])
        got = _device(mode, first, np.ones(n, np.float32), second, None, EDGES, SUBKW[mode])
        assert got['npairs'].sum() > 0
        np.testing.assert_array_equal(got['wsum'], got['npairs'].astype(np.float64))
        for k in SUMS:
            assert not got[k].any(), k
    # equal velocities: u = 0 whatever the common velocity is
    same = c[:3] + [np.full(3000, 123.456, np.float32), np.full(3000, -7.0, np.float32), np.full(3000, 1e4, np.float32)]
    got = _device(mode, same, None, None, None, EDGES, SUBKW[mode])
    assert got['npairs'].sum() > 0 and not any(got[k].any() for k in SUMS)


@pytest.mark.parametrize('auto', [True, False])
def test_one_bin(auto):
    """nbins = 1: in mode 0 every pair takes the per-lane path of the last bin"""
    bins = np.array([0.5, 20.0], np.float32)
    want = _judge('r', _set(3000, 81) if auto else _set(300, 82), None if auto else _set(3000, 81), bins, {}, f'one bin auto={auto}')
    assert want['npairs'][0] > 10000
    _judge('rppi', _set(300, 82), None, bins, dict(pimax=20.0, npibins=1), 'one bin rppi')


def test_last_bin_comparator():
    """option pairvel_lds_top: the pairs of the last bin through the LDS atomics like the others - the same sums"""
    from abacusutils_amd import _lib
    _lib.set_option('pairvel_lds_top', 1)
    try:
        _judge('r', _set(3000, 81), None, EDGES, {}, 'last bin in LDS', ('host', 'f32 resident'))
        _judge('r', _set(300, 82), _set(3000, 81), EDGES[-2:], {}, 'last bin in LDS, one bin')
    finally:
        _lib.set_option('pairvel_lds_top', 0)


@pytest.mark.parametrize('last', [40.0, 50.0])
@pytest.mark.parametrize('mode', ['r', 'rppi'])
def test_one_cell_grid(mode, last):
    """last edge 0.4 L and exactly L / 2: fewer than three cells of the reach fit, a dimension is one cell that is its own
    neighbour (rppi: one cell in x and y, four along z)"""
    bins = np.geomspace(1.0, last, 6).astype(np.float32)
    assert bins[-1] == np.float32(last)
    _judge(mode, _set(700, 83), None, bins, SUBKW[mode], f'one cell {mode} {last}', ('host', 'f64 resident'))
    _judge(mode, _set(300, 82), _set(700, 83), bins, SUBKW[mode], f'one cell cross {mode} {last}')


@pytest.mark.parametrize('n1', [255, 256, 257, 600])
def test_slice_boundaries(n1):
    """n1 points of set 1 inside ONE cell (a cube of side 8 in a cell of side 25): slices of 256 points, full, one short, one
    over, and three slices; against 300 spread points"""
    rng = np.random.default_rng(n1)
    p = [30.0 + 8.0 * rng.random(n1) for _ in range(3)]
    s1 = (p + velocities(p, BOX, n1 + 1), _weights(n1, n1 + 2, signed=True))
    want = _judge('r', s1, _set(300, 82), EDGES, {}, f'slice {n1}', ('host', 'f32'))
    assert want['npairs'].sum() > 0
    _judge('smu', s1, None, EDGES, SUBKW['smu'], f'slice auto {n1}')


@pytest.mark.parametrize('nbins', [26, 52])
def test_more_entries_than_the_lds_histogram(nbins):
    """rppi with 40 pi bins: 1040 entries, just above the 1024 of one launch (runs of 25 and 1 separation bins), and 2080
    (25 + 25 + 2): the same sums per cell as ONE statement call over all bins"""
    bins = np.linspace(0.5, 20.0, nbins + 1).astype(np.float32)
    want = _judge('rppi', _set(3000, 81), None, bins, dict(pimax=20.0, npibins=40), f'{nbins} x 40 entries', ('host', 'f32 resident'))
    assert want['npairs'].shape == (nbins * 40,) and np.count_nonzero(want["npairs"]) > nbins * 20


def test_tiny_and_disjoint_sets():
    (c, w) = _set(300, 82)
    e = [np.zeros(0, np.float32)] * 6
    one = [np.asarray(col[:1]) for col in c]
    for mode, n in (('r', 8), ('rppi', 32), ('smu', 40)):
        for first, second in ((e, None), (e, c), (c, e), (one, None)):
            got = _device(mode, first, None, second, None, EDGES, SUBKW[mode])
            assert all(got[k].shape == (n,) and not got[k].any() for k in ALL) and got['npairs'].dtype == np.uint64
        assert _candidates() >= 0
    _judge('r', (one, w[:1]), (c, w), EDGES, {}, '1 x 300')
    _judge('r', (c, w), (one, w[:1]), EDGES, {}, '300 x 1')
    # two sets that share no cell and no neighbour cell: nothing is counted
    rng = np.random.default_rng(3)
    a = [5.0 * rng.random(200) for _ in range(3)]
    b = [50.0 + 5.0 * rng.random(200) for _ in range(3)]
    got = _device('r', a + velocities(a, BOX, 4), None, b + velocities(b, BOX, 5), None, EDGES, {})
    assert not any(got[k].any() for k in ALL)


def test_argument_errors():
    from abacusutils_amd._lib import DeviceArray
    c, w = _set(300, 82)
    dev = [DeviceArray(np.asarray(col, dtype=np.float32)) for col in c]
    with pytest.raises(TypeError):
        _device('r', dev[:3] + c[3:], None, None, None, EDGES, {})               # host velocities beside resident positions
    with pytest.raises(TypeError):
        _device('r', dev, None, c, None, EDGES, {})                              # a host second set
    with pytest.raises(TypeError):
        _device('r', c, DeviceArray(w), None, None, EDGES, {})                   # resident weights beside host columns
    with pytest.raises(TypeError):
        _device('r', dev[:5] + [DeviceArray(np.asarray(c[5], dtype=np.float64))], None, None, None, EDGES, {})
    with pytest.raises(ValueError):
        _device('r', c, None, None, None, np.array([1.0, 50.5], np.float32), {})
    with pytest.raises(ValueError):
        _device('rppi', c, None, None, None, EDGES, dict(pimax=51.0, npibins=4))
    with pytest.raises(ValueError):
        _device('r', c[:5] + [None], None, None, None, EDGES, {})


def test_halotools_named_wrappers():
    """the four wrappers are moments of the statement's sums with unit weights"""
    from abacusutils_amd.analysis import pairwise_velocity as V
    c, _ = _set(300, 82)
    big, _ = _set(3000, 81)
    pos, vel = np.stack(c[:3], axis=1), np.stack(c[3:], axis=1)
    pos2, vel2 = np.stack(big[:3], axis=1), np.stack(big[3:], axis=1)
    rb = EDGES[3:]
    for second, kw2 in ((None, {}), (big, dict(sample2=pos2, velocities2=vel2))):
        s, _ = statement('r', *c, BOX, rb, *(second or ()))
        m = V.moments_from_sums(s)
        np.testing.assert_allclose(V.mean_radial_velocity_vs_r(pos, vel, rb, period=BOX, **kw2), m['v12'], rtol=1e-10, atol=1e-9)
        np.testing.assert_allclose(V.radial_pvd_vs_r(pos, vel, rb, period=BOX, **kw2), m['sigma_r'], rtol=1e-10)
        s, _ = statement('rppi', *c, BOX, rb, *(second or ()), pimax=15.0, npibins=1)
        m = V.moments_from_sums(s)
        np.testing.assert_allclose(V.mean_los_velocity_vs_rp(pos, vel, rb, 15.0, period=BOX, **kw2), m['vlos'], rtol=1e-10, atol=1e-9)
        np.testing.assert_allclose(V.los_pvd_vs_rp(pos, vel, rb, 15.0, period=BOX, **kw2), m['sigma_los'], rtol=1e-10)
    with pytest.raises(ValueError):
        V.mean_radial_velocity_vs_r(pos, vel, rb, period=None)


def test_abacus_hod_compute_pairwise_velocity():
    """AbacusHOD.compute_pairwise_velocity: the catalogue still in HBM gives what its host columns give.  Both calls read the same
    float32 values, so npairs agree exactly and the sums differ by the order of the float64 atomics alone: each is within
    (n + 8) 2^-52 S of the exact sum, S = sum |term|, so they are within twice that of each other.  With the unit weights of a
    mock S is the sum itself for wsum, vr2, u2 and vz2, and by Cauchy-Schwarz S <= sqrt(npairs vr2) for vr1, sqrt(npairs vz2) for
    vz1."""
    from test_abacus_hod_gpu import CLUSTERING, HOD_PARAMS

    from abacusutils_amd import synth
    from abacusutils_amd.analysis.pairwise_velocity import moments_from_sums, pairwise_velocity_sums
    from abacusutils_amd.hod.abacus_hod import AbacusHOD
    hd, pd, params = synth.synth_hod_inputs(100000, 100000, seed=19, lbox=1000.0)
    hod = dict(HOD_PARAMS, LRG_params=dict(synth.LRG_PARAMS, logM_cut=12.3, logM1=13.3), ELG_params=dict(synth.ELG_PARAMS))
    ball = AbacusHOD.from_arrays(hd, pd, params, hod, CLUSTERING)
    mock = ball.run_hod()
    assert all(mock.device_xyz(tr) is not None and mock.device_vel(tr) is not None for tr in mock)
    plain = {tr: dict(mock[tr]) for tr in mock}
    rbins = np.geomspace(1.0, 30.0, 7)
    for mode, kw in (('r', {}), ('rppi', dict(pimax=30.0, npibins=3))):
        got, want = ball.compute_pairwise_velocity(mock, rbins, mode=mode, **kw), ball.compute_pairwise_velocity(plain, rbins, mode=mode, **kw)
        tracers = list(mock)
        assert set(got) == set(want) == {a + '_' + b for a in tracers for b in tracers}
        for i, a in enumerate(tracers):
            for b in tracers[i:]:
                g = got[a + '_' + b]
                assert got[b + '_' + a] is g and g['npairs'].sum() > 0
                six = lambda tr: [np.asarray(plain[tr][c]) for c in ('x', 'y', 'z', 'vx', 'vy', 'vz')]   # noqa: E731
                second = {} if a == b else dict(zip(('X2', 'Y2', 'Z2', 'VX2', 'VY2', 'VZ2'), six(b)))
                direct = pairwise_velocity_sums(mode, *six(a), ball.lbox, rbins, **second, pimax=kw.get('pimax', 0.0),
                                                npibins=kw.get('npibins', 0))
                n = g['npairs'].astype(np.float64)
                scale = dict(wsum=n, vr2=g['vr2'], u2=g['u2'], vz2=g['vz2'], vr1=np.sqrt(n * g['vr2']), vz1=np.sqrt(n * g['vz2']))
                for other in (want[a + '_' + b], direct):
                    np.testing.assert_array_equal(g['npairs'], other['npairs'])
                    np.testing.assert_array_equal(g['wsum'], n)
                    for k in SUMS:
                        tol = 2 * bound(g['npairs'], scale[k]) * (1 + 1e-9)
                        assert np.all(np.abs(g[k] - other[k]) <= tol), (mode, a, b, k)
                m = moments_from_sums(g)
                for k in m:
                    np.testing.assert_array_equal(g[k], m[k])
    # a modified host velocity column: the device copy no longer stands for the mock
    tr = tracers[0]
    mock[tr]['vz'][0] += 1.0
    assert mock.device_vel(tr) is None and mock.device_xyz(tr) is not None
    after = ball.compute_pairwise_velocity(mock, rbins)[tr + '_' + tr]
    ref = pairwise_velocity_sums('r', *[np.asarray(mock[tr][c]) for c in ('x', 'y', 'z', 'vx', 'vy', 'vz')], ball.lbox, rbins)
    np.testing.assert_array_equal(after['npairs'], ref['npairs'])
    np.testing.assert_allclose(after['vz2'], ref['vz2'], rtol=1e-12)
