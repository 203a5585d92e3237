"""The pairwise velocity sums without a GPU: the NumPy statement tests/pairvel_statement.py (the judge of tests/test_pairvel_gpu.py)
against pairs_statement.paircount for membership, against a plain double loop, closed forms, symmetries and edge rules;
moments_from_sums; and every validation rule of abacus_pairvel[_dev] through the C entries, which refuse before the device is
touched."""
import math

import numpy as np
import pytest
from pairs_statement import MODES, paircount
from pairvel_statement import SUMS, bound, pairvel, velocities
from test_pairs_weighted_gpu import _points, _weights

ALL = ('npairs', 'wsum') + SUMS
BOX = 100.0
EDGES = np.geomspace(0.5, 20.0, 9).astype(np.float32)
SUBKW = {'r': {}, 'rppi': dict(pimax=20.0, npibins=4), 'smu': dict(mu_max=1.0, nmubins=5)}


def big():
    a = _points(3000, BOX, 81)
    return a, velocities(a, BOX, 181), _weights(3000, 281, signed=True)


def small():
    b = _points(300, BOX, 82)
    return b, velocities(b, BOX, 182), _weights(300, 282, signed=True)


@pytest.mark.parametrize('mode,least', [('r', 132), ('rppi', 90), ('smu', 22)])
def test_membership_is_the_weighted_counters(mode, least):
    """npairs and wsum of the statement are pairs_statement.paircount's, cell by cell; the catalogue of the GPU tests populates
    every (bin, sub-bin) of the auto count, and of the cross count wherever the GPU tests rely on it"""
    (a, va, wa), (b, vb, wb) = big(), small()
    kw = SUBKW[mode]
    s, scale = pairvel(mode, *a, *va, BOX, EDGES, w1=wa, **kw)
    n, w, _, wabs = paircount(mode, *a, BOX, EDGES, w1=wa, **kw)
    np.testing.assert_array_equal(s['npairs'], n)
    np.testing.assert_array_equal(s['wsum'], w)
    np.testing.assert_array_equal(scale['wsum'], wabs)
    assert n.min() == least
    s, _ = pairvel(mode, *b, *vb, BOX, EDGES, *a, *va, w1=wb, w2=wa, **kw)
    n, w, _, _ = paircount(mode, *b, BOX, EDGES, *a, w1=wb, w2=wa, **kw)
    np.testing.assert_array_equal(s['npairs'], n)
    np.testing.assert_array_equal(s['wsum'], w)
    assert np.count_nonzero(n == 0) == (6 if mode == 'smu' else 0)


def loop(mode, p, v, w, box, bins, q=None, vq=None, wq=None, upper=False, pimax=0.0, npibins=0, mu_max=1.0, nmubins=0):
    """the contract as a plain double loop: np.float32 scalars where it says float32, Python floats (float64) elsewhere"""
    f = np.float32
    auto = q is None
    if auto:
        q, vq, wq = p, v, w
    nsub = 1 if mode == 0 else (npibins if mode == 1 else nmubins)
    nb = len(bins) - 1
    e2 = [f(e) * f(e) for e in bins]
    box, half = f(box), f(box) * f(0.5)
    out = {k: [0.0] * (nb * nsub) for k in ALL}

    def image(d):
        return d - box if d > half else (d + box if d < -half else d)
    for i in range(len(p)):
        for j in range(len(q)):
            if auto and (i == j or (upper and j < i)):
                continue
            dx, dy, dz = (image(f(p[i][d]) - f(q[j][d])) for d in range(3))
            sub = 0
            if mode == 1:
                if not abs(dz) < f(pimax):
                    continue
                r2 = dx * dx + dy * dy
                sub = int(abs(dz) / (f(pimax) / f(npibins)))
            else:
                r2 = dx * dx + dy * dy + dz * dz
            if not (e2[0] <= r2 < e2[nb]):
                continue
            b = max(k for k in range(nb) if e2[k] <= r2)
            if mode == 2:
                sep = np.sqrt(r2)
                mu = abs(dz) / sep if sep > 0 else f(0)
                if not mu < f(mu_max):
                    continue
                sub = int(mu * (f(nmubins) / f(mu_max)))
            if sub >= nsub:
                continue
            ux, uy, uz = (float(f(v[i][d]) - f(vq[j][d])) for d in range(3))
            dx, dy, dz = float(dx), float(dy), float(dz)
            s2 = dx * dx + dy * dy + dz * dz
            t = ux * dx + uy * dy + uz * dz
            vr = t / math.sqrt(s2) if s2 > 0 else 0.0
            uu = ux * ux + uy * uy + uz * uz
            vz = uz * float(np.sign(dz))
            ww = float(f(w[i])) * float(f(wq[j]))
            c = b * nsub + sub
            for k, term in zip(ALL, (1, ww, ww * vr, ww * (vr * vr), ww * uu, ww * vz, ww * (uz * uz))):
                out[k][c] += term
    return {k: np.array(x, dtype=np.uint64 if k == 'npairs' else np.float64) for k, x in out.items()}


def cloud(n, seed, lo=0.0, hi=10.0):
    rng = np.random.default_rng(seed)
    p = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    v = rng.normal(0, 300, (n, 3)).astype(np.float32)
    w = rng.uniform(-1, 1, n).astype(np.float32)
    return p, v, w


def by_columns(p, v):
    return [p[:, d] for d in range(3)] + [v[:, d] for d in range(3)]


def assert_within_bounds(got, want, scale, npairs):
    np.testing.assert_array_equal(got['npairs'], want['npairs'])
    for k in ('wsum',) + SUMS:
        b = bound(npairs, scale[k])
        assert np.all(np.abs(got[k] - want[k]) <= b), (k, got[k] - want[k], b)


@pytest.mark.parametrize('mode', ['r', 'rppi', 'smu'])
def test_statement_against_a_plain_double_loop(mode):
    """40 points in a box of 10 (pairs wrap in every dimension), auto and cross, every mode"""
    p, v, w = cloud(40, 5)
    q, vq, wq = cloud(25, 6)
    bins = np.array([0.0, 0.7, 1.5, 2.5, 4.0], np.float32)
    kw = dict(r={}, rppi=dict(pimax=3.0, npibins=3), smu=dict(mu_max=1.0, nmubins=3))[mode]
    s, scale = pairvel(mode, *by_columns(p, v), 10.0, bins, w1=w, **kw)
    ref = loop(MODES[mode], p, v, w, 10.0, bins, **kw)
    assert ref['npairs'].sum() > 300
    assert_within_bounds(s, ref, scale, ref['npairs'])
    s, scale = pairvel(mode, *by_columns(p, v), 10.0, bins, *by_columns(q, vq), w1=w, w2=wq, **kw)
    ref = loop(MODES[mode], p, v, w, 10.0, bins, q, vq, wq, **kw)
    assert ref['npairs'].sum() > 200
    assert_within_bounds(s, ref, scale, ref['npairs'])


def all_pairs(p):
    i, j = np.nonzero(~np.eye(len(p), dtype=bool))
    return (p[i] - p[j]).astype(np.float64)     # float32 differences: no pair wraps in the tests that use this


def test_hubble_flow():
    """v = H x with H a power of two: u = H d exactly, so vr = H r, u2 = vr2 and nothing is transverse"""
    from abacusutils_amd.analysis.pairwise_velocity import moments_from_sums
    H = 4.0
    p = np.random.default_rng(7).uniform(30.0, 50.0, (200, 3)).astype(np.float32)
    v = np.float32(H) * p
    one_bin = np.array([1e-3, 49.0], np.float32)
    s, _ = pairvel('r', *by_columns(p, v), BOX, one_bin)
    d = all_pairs(p)
    r = np.sqrt((d * d).sum(axis=1))
    assert s['npairs'][0] == 200 * 199
    np.testing.assert_allclose(s['vr1'][0], H * r.sum(), rtol=1e-13)
    np.testing.assert_allclose(s['vr2'][0], H * H * (r * r).sum(), rtol=1e-13)
    np.testing.assert_allclose(s['u2'][0], s['vr2'][0], rtol=1e-13)
    m = moments_from_sums(s)
    np.testing.assert_allclose(m['v12'][0], H * r.mean(), rtol=1e-13)
    assert m['sigma_t'][0] <= 1e-6 * H * r.mean()
    # several bins: the mean infall of a bin lies between H times its edges
    bins = np.array([1.0, 5.0, 10.0, 20.0, 40.0], np.float32)
    m = moments_from_sums(pairvel('r', *by_columns(p, v), BOX, bins)[0])
    assert np.all(m['v12'] > H * bins[:-1]) and np.all(m['v12'] < H * bins[1:])


def test_rigid_rotation_about_z():
    """v = Omega z^ x p with Omega a power of two: u = Omega (-dy, dx, 0) exactly, so u . d = 0 in float64 (the products of
    float32 values are exact) and u2 = Omega^2 sum r_perp^2"""
    Om = 8.0
    p = np.random.default_rng(8).uniform(30.0, 50.0, (150, 3)).astype(np.float32)
    v = np.stack([-np.float32(Om) * p[:, 1], np.float32(Om) * p[:, 0], np.zeros(150, np.float32)], axis=1)
    s, scale = pairvel('r', *by_columns(p, v), BOX, np.array([1e-3, 49.0], np.float32))
    d = all_pairs(p)
    assert s['npairs'][0] == 150 * 149 and s['vr1'][0] == 0 and s['vr2'][0] == 0 and scale['vr1'][0] == 0
    np.testing.assert_allclose(s['u2'][0], Om * Om * (d[:, 0] ** 2 + d[:, 1] ** 2).sum(), rtol=1e-13)
    assert s['vz1'][0] == 0 and s['vz2'][0] == 0


def test_two_points_head_on():
    p = np.array([[10, 10, 10], [13, 14, 10]], np.float32)
    v = np.array([[3, 4, 0], [-3, -4, 0]], np.float32) * np.float32(25)
    s, _ = pairvel('r', *by_columns(p, v), BOX, np.array([4.0, 6.0], np.float32))
    absu = 250.0
    assert s['npairs'][0] == 2 and s['vr1'][0] == -2 * absu and s['vr2'][0] == 2 * absu ** 2 and s['u2'][0] == 2 * absu ** 2
    assert s['vz1'][0] == 0 and s['vz2'][0] == 0
    s, _ = pairvel('r', *by_columns(p, -v), BOX, np.array([4.0, 6.0], np.float32))     # receding: positive
    assert s['vr1'][0] == 2 * absu


def test_symmetries():
    p, v, w = cloud(40, 15)
    q, vq, wq = cloud(30, 16)
    bins = np.array([0.0, 1.0, 2.0, 4.0], np.float32)
    kw = dict(pimax=3.0, npibins=2)
    # the ordered pairs of an autocorrelation: twice the pairs i < j
    s, scale = pairvel('rppi', *by_columns(p, v), 10.0, bins, w1=w, **kw)
    up = loop(1, p, v, w, 10.0, bins, upper=True, **kw)
    np.testing.assert_array_equal(s['npairs'], 2 * up['npairs'])
    for k in ('wsum',) + SUMS:
        assert np.all(np.abs(s[k] - 2 * up[k]) <= bound(s['npairs'], scale[k])), k
    # cross (1, 2) and (2, 1): the same seven sums
    s12, scale = pairvel('rppi', *by_columns(p, v), 10.0, bins, *by_columns(q, vq), w1=w, w2=wq, **kw)
    s21, _ = pairvel('rppi', *by_columns(q, vq), 10.0, bins, *by_columns(p, v), w1=wq, w2=w, **kw)
    assert s12['npairs'].sum() > 100
    assert_within_bounds(s21, s12, scale, s12['npairs'])
    # a constant velocity that every float32 sum carries exactly: velocities on a grid of 1/8 below 1024, plus 2048
    v8 = (np.round(v * 8) / 8).astype(np.float32)
    base, _ = pairvel('rppi', *by_columns(p, v8), 10.0, bins, w1=w, **kw)
    moved, _ = pairvel('rppi', *by_columns(p, v8 + np.float32(2048.0)), 10.0, bins, w1=w, **kw)
    assert np.abs(v8).max() < 2048 and np.array_equal((v8 + np.float32(2048.0)) - np.float32(2048.0), v8)
    for k in ALL:
        np.testing.assert_array_equal(moved[k], base[k])


def test_edge_rules():
    bins = np.array([0.0, 1.0], np.float32)
    # a coincident pair with first edge 0: no radial direction, the velocity difference still counts
    p = np.array([[5, 5, 5], [5, 5, 5]], np.float32)
    v = np.array([[1, 2, 3], [-1, 0, 7]], np.float32)
    s, _ = pairvel('r', *by_columns(p, v), BOX, bins)
    assert s['npairs'][0] == 2 and s['vr1'][0] == 0 and s['vr2'][0] == 0
    assert s['u2'][0] == 2 * (4 + 4 + 16) and s['vz2'][0] == 2 * 16 and s['vz1'][0] == 0
    # dz == 0: nothing to vz1, uz^2 to vz2
    p = np.array([[5, 5, 5], [5.5, 5, 5]], np.float32)
    s, _ = pairvel('r', *by_columns(p, v), BOX, bins)
    assert s['npairs'][0] == 2 and s['vz1'][0] == 0 and s['vz2'][0] == 32 and s['vr1'][0] == 2 * (2 * -0.5 / 0.5)
    # dz != 0: the sign of dz decides
    p = np.array([[5, 5, 5], [5, 5, 5.5]], np.float32)
    s, _ = pairvel('r', *by_columns(p, v), BOX, bins)
    assert s['vz1'][0] == 2 * 4 and s['vr1'][0] == 2 * 4     # z_1 < z_2 and v_1z < v_2z: receding
    # empty sets
    e = np.zeros(0, np.float32)
    for mode, n in (('r', 8), ('rppi', 32), ('smu', 40)):
        for first, second in (([e] * 6, []), ([e] * 6, by_columns(p, v)), (by_columns(p, v), [e] * 6)):
            s, scale = pairvel(mode, *first, BOX, EDGES, *second, **SUBKW[mode])
            assert all(s[k].shape == (n,) and not s[k].any() for k in ALL) and s['npairs'].dtype == np.uint64
            assert all(scale[k].shape == (n,) for k in ('wsum',) + SUMS)


def test_moments_from_sums():
    import warnings
    from abacusutils_amd.analysis.pairwise_velocity import moments_from_sums
    sums = dict(npairs=np.array([4, 0, 2], np.uint64), wsum=np.array([4.0, 0.0, 2.0]), vr1=np.array([-8.0, 0.0, 2.0]),
                vr2=np.array([52.0, 0.0, 1.0]), u2=np.array([84.0, 0.0, 5.0]), vz1=np.array([2.0, 0.0, -4.0]),
                vz2=np.array([17.0, 0.0, 8.0]))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        m = moments_from_sums(sums)
    np.testing.assert_array_equal(m['v12'], [-2.0, np.nan, 1.0])
    np.testing.assert_array_equal(m['sigma_r'], [3.0, np.nan, 0.0])          # 13 - 4 | the variance -0.5 is clipped to 0
    np.testing.assert_array_equal(m['sigma_t'], [2.0, np.nan, 1.0])          # (84 - 52) / 8 | (5 - 1) / 4
    np.testing.assert_array_equal(m['vlos'], [0.5, np.nan, -2.0])
    np.testing.assert_array_equal(m['sigma_los'], [2.0, np.nan, 0.0])        # 4.25 - 0.25 | 4 - 4
    assert set(m) == {'v12', 'sigma_r', 'sigma_t', 'vlos', 'sigma_los'}


def test_c_abi_validates_before_the_device():
    """every rule of abacus_pairvel and abacus_pairvel_dev answers with a message that starts with the entry's name, with or
    without a GPU: the rules of the periodic weighted counter and those of the velocity columns and of vsum"""
    import ctypes as C
    from abacusutils_amd import _lib
    L, ptr = _lib.lib(), _lib.ptr
    x = np.linspace(0.0, 9.0, 10).astype(np.float32)
    w = np.ones(10, np.float32)
    bins = np.array([0.5, 1.0, 2.0], np.float32)
    out, ws, vs = np.zeros(64, np.uint64), np.zeros(64), np.zeros(5 * 64)
    second = dict(x2=x, y2=x, z2=x, vx2=x, vy2=x, vz2=x, n2=10)

    def call(entry, mode=1, x1=x, vx1=x, vy1=x, vz1=x, x2=None, y2=None, z2=None, vx2=None, vy2=None, vz2=None, w2=None, n1=10, n2=0,
             pos_dtype=0, box=100.0, b=bins, nb=2, pimax=4.0, npi=4, mu_max=1.0, nmu=4, npairs=out, wsum=ws, vsum=vs):
        dt = (pos_dtype,) if entry.endswith('_dev') else ()
        return getattr(L, entry)(mode, ptr(x1), ptr(x), ptr(x), ptr(vx1), ptr(vy1), ptr(vz1), ptr(w), C.c_int64(n1), ptr(x2), ptr(y2),
                                 ptr(z2), ptr(vx2), ptr(vy2), ptr(vz2), ptr(w2), C.c_int64(n2), *dt, C.c_float(box), ptr(b), nb,
                                 C.c_float(pimax), npi, C.c_float(mu_max), nmu, ptr(npairs), ptr(wsum), ptr(vsum))
    rules = [(dict(mode=3), 'unknown mode'), (dict(x1=None), 'null'), (dict(b=None), 'null'), (dict(npairs=None), 'null'),
             (dict(nb=0), 'nbins'), (dict(box=0.0), 'boxsize'), (dict(box=-1.0), 'boxsize'), (dict(npi=0), 'pi / mu bin'),
             (dict(mode=2, nmu=0), 'pi / mu bin'), (dict(npi=1025), 'exceed the LDS histogram'), (dict(n1=1 << 31), 'point counts'),
             (dict(n1=-1), 'point counts'), ({**second, 'n2': -1}, 'point counts'),
             (dict(b=np.array([0.5, 2.0, 2.0], np.float32)), 'increase'), (dict(b=np.array([2.0, 1.0, 3.0], np.float32)), 'increase'),
             (dict(b=np.array([0.5, 1.0, 51.0], np.float32)), 'half the box'), (dict(pimax=50.5), 'half the box'),
             ({**second, 'y2': None}, 'y2 / z2'), ({**second, 'z2': None}, 'y2 / z2'),
             (dict(wsum=None), 'wsum is NULL'), (dict(w2=w), 'w2 given for an autocorrelation'),
             # the rules of this entry
             (dict(vx1=None), 'null velocity column'), (dict(vy1=None), 'null velocity column'), (dict(vz1=None), 'null velocity column'),
             ({**second, 'vy2': None}, 'null velocity column'), ({**second, 'vx2': None, 'vz2': None}, 'null velocity column'),
             ({**second, 'vx2': None, 'vy2': None, 'vz2': None}, 'but not for set 2'),
             (dict(vsum=None), 'vsum is NULL')]
    for entry in ('abacus_pairvel', 'abacus_pairvel_dev'):
        for kw, text in rules + ([(dict(pos_dtype=7), 'pos_dtype')] if entry.endswith('_dev') else []):
            rc = call(entry, **kw)
            msg = L.abacus_last_error().decode()
            assert rc != 0 and msg.startswith(entry + ': ') and text in msg, (entry, kw, msg)
