"""The spherical void finder on the device (abacusutils_amd.analysis.voids, C ABI abacus_void_*) against the NumPy statement
tests/voids_statement.py.  Needs an MI355X: run with `-m gpu`.

The finder's decisions are integers: `cell`, `level`, the bits of the float32 `delta` and the candidates and voids per level are held
to the sequential statement exactly, the rounds per level to the round statement.  Shapes: n = 16 (power of two, dense pitch 16 and
padded pitch 32) and n = 24 (mixed radix, padded pitch 32 != n); radii of 3, 2.5, 1.5 and 1 cells give brick grids of 2, 3 (n = 16) and
4, 8, 12 (n = 24) bricks per dimension, so both the walk over all bricks of a dimension and the walk over three of them run; the
constant mesh has every cell a candidate and needs 24 rounds.  The padded copies carry -1e30 in every pad float: a read of the padding
would be a candidate below every cell.

Fields: max |got - want| / max |want| <= 4 e_ref (the rule at the head of tests/test_zcv_gpu.py), e_ref the statement's own float32
noise - its float32 / complex64 evaluation against its float64 one, computed here - times log2(n^3) / log2(16^3) beyond 16^3."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import voids_statement as st
from test_voids_host import check_planted

pytestmark = pytest.mark.gpu

PAD = np.float32(-1e30)
THR = -0.7


def _lib():
    from abacusutils_amd import _lib
    return _lib


def _pitch(n):
    return (n + 2 + 31) // 32 * 32


@functools.lru_cache(maxsize=None)
def _case(name, n):
    """(mesh or list of meshes, D in cells, threshold); the references below are computed once per case"""
    radii, thr = st.RADII_CELLS, THR
    if name in ('white', 'quantised', 'constant'):
        mesh = st.case_mesh(name, n)
    elif name == 'none':
        mesh = np.abs(st.case_mesh('white', n)) + np.float32(1.0)
    elif name == 'zeros':                                             # +0.0 and -0.0 under a positive threshold: one value, cell order
        mesh = np.where(np.random.default_rng(7).random((n, n, n)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
        thr = 0.25
    elif name == 'inf':
        mesh = st.case_mesh('white', n).copy()
        mesh[n - 3, 1, n // 2] = -np.inf
    elif name == 'corners':                                           # minima in the cells 0 and n - 1 of every axis
        mesh = np.zeros((n, n, n), dtype=np.float32)
        for q, (i, j, k) in enumerate(np.ndindex(2, 2, 2)):
            mesh[i * (n - 1), j * (n - 1), k * (n - 1)] = -1.0 - 0.125 * q
        mesh[n // 2, 0, n - 1], mesh[0, n // 2, 0], mesh[n - 1, n - 1, n // 2] = -3.0, -2.5, -2.75
    elif name == 'touching':                                          # d2 = 25 = D: two voids; d2 = 22: one
        radii = (2.5, 2.5 * (1 - 2.0**-40))                           # two levels of 2.5 cells: every D is 25
        assert st.d_table(radii, float(n), n).tolist() == [[25, 25], [25, 25]]
        mesh = np.zeros((n, n, n), dtype=np.float32)
        mesh[2, 2, 2], mesh[5, 6, 2] = -2.0, -1.0
        mesh[10, 10, 10], mesh[13, 13, 12] = -2.0, -1.0
    elif name == 'gap':                                               # per-level meshes: the middle level has no candidate at all
        radii = (3.0, 2.0, 1.0)
        mesh = [st.case_mesh('white', n), np.ones((n, n, n), dtype=np.float32), st.case_mesh('quantised', n)]
    else:
        raise KeyError(name)
    for f in mesh if isinstance(mesh, list) else [mesh]:
        f.setflags(write=False)
    return mesh, st.d_table(radii, float(n), n), radii, thr


@functools.lru_cache(maxsize=None)
def _want(name, n):
    mesh, D, _, thr = _case(name, n)
    return st.find_sequential(mesh, D, thr), st.find_rounds(mesh, D, thr)['rounds']


def _assert_equal(got, want, rounds, label):
    np.testing.assert_array_equal(got['cell'], want['cell'], err_msg=label)
    np.testing.assert_array_equal(got['level'], want['level'], err_msg=label)
    assert got['cell'].dtype == np.int32 and got['level'].dtype == np.int32 and got['delta'].dtype == np.float32
    assert got['delta'].tobytes() == want['delta'].tobytes(), label
    np.testing.assert_array_equal(got['counts'][:, :2], want['counts'][:, :2], err_msg=label)
    if rounds is not None:
        np.testing.assert_array_equal(got['counts'][:, 2], rounds, err_msg=label + ' rounds')


def _padded(mesh):
    n = mesh.shape[0]
    full = np.full((n, n, _pitch(n)), PAD, dtype=np.float32)
    full[:, :, :n] = mesh
    return full


def _run_c(meshes, n, pitch, D, thr):
    """the C ABI on device meshes of any pitch: dict like find_voids_mesh's"""
    lib = _lib()
    L, m = lib.lib(), len(D)
    handle, counts = C.c_void_p(), np.zeros((m, 3), dtype=np.int64)
    lib.check(L.abacus_void_create(n, m, lib.ptr(np.ascontiguousarray(D, dtype=np.int64)), C.byref(handle)))
    try:
        for i in range(m):
            c = [C.c_int64(-1) for _ in range(3)]
            lib.check(L.abacus_void_level_dev(handle, meshes[i].ptr, pitch, i, C.c_float(thr), *[C.byref(x) for x in c]))
            counts[i] = [x.value for x in c]
        nv = C.c_int64(-1)
        lib.check(L.abacus_void_count(handle, C.byref(nv)))
        cell, level, delta = np.zeros((nv.value, 3), dtype=np.int32), np.zeros(nv.value, dtype=np.int32), np.zeros(nv.value, dtype=np.float32)
        lib.check(L.abacus_void_fetch(handle, lib.ptr(cell), lib.ptr(level), lib.ptr(delta)))
    finally:
        lib.check(L.abacus_void_free(handle))
    return dict(cell=cell, level=level, delta=delta, counts=counts)


# ------------------------------------------------------------------------------------------------- 1. the finder on given meshes
@pytest.mark.parametrize('n', (16, 24))
@pytest.mark.parametrize('name', ('white', 'quantised', 'constant', 'none', 'zeros', 'inf', 'corners', 'touching', 'gap'))
def test_finder_equals_the_statement(name, n):
    from abacusutils_amd.analysis.voids import find_voids_mesh
    lib = _lib()
    mesh, D, radii, thr = _case(name, n)
    want, rounds = _want(name, n)
    meshes = mesh if isinstance(mesh, list) else [mesh]
    got = find_voids_mesh(mesh, float(n), radii, thr)
    _assert_equal(got, want, rounds, f'{name} n={n} host mesh')
    np.testing.assert_array_equal(got['centres'], want['cell'].astype(np.float64))           # a = 1
    np.testing.assert_array_equal(got['radius'], np.asarray(radii)[want['level']])
    dense, padded = [lib.DeviceArray(f) for f in meshes], [lib.DeviceArray(_padded(f)) for f in meshes]
    try:
        dev = dense[0] if not isinstance(mesh, list) else dense
        _assert_equal(find_voids_mesh(dev, float(n), radii, thr), want, rounds, f'{name} n={n} DeviceArray')
        m = len(D)
        _assert_equal(_run_c(padded * m if len(padded) == 1 else padded, n, _pitch(n), D, thr), want, rounds, f'{name} n={n} padded')
        for d, p, f in zip(dense, padded, meshes):
            assert d.get().tobytes() == f.tobytes(), 'the mesh was modified'
            assert p.get().tobytes() == _padded(f).tobytes(), 'the padded mesh was modified'
    finally:
        for a in dense + padded:
            a.free()
    # what the cases are there for
    nv = want['counts'][:, 1]
    if name == 'none':
        assert want['counts'].sum() == 0 and rounds.sum() == 0 and len(got['level']) == 0 and got['cell'].shape == (0, 3)
    elif name == 'zeros':
        assert want['counts'][0, 0] == n**3 and want['cell'][0].tolist() == [0, 0, 0] and not np.signbit(got['delta']).any()
    elif name == 'inf':
        assert want['cell'][0].tolist() == [n - 3, 1, n // 2] and got['delta'][0] == -np.inf
    elif name == 'corners':
        assert nv[0] >= 3 and (want['cell'] == 0).any() and (want['cell'] == n - 1).any()
    elif name == 'touching':
        assert want['cell'].tolist() == [[2, 2, 2], [10, 10, 10], [5, 6, 2]]
    elif name == 'gap':
        assert nv[0] > 0 and want['counts'][1].tolist() == [0, 0] and rounds[1] == 0 and nv[2] > 0
    elif name == 'constant' and n == 24:
        assert rounds.tolist() == [24, 0, 11, 2]


# ------------------------------------------------------------------------------------------------- 2. from particles
@functools.lru_cache(maxsize=None)
def _dyadic_points():
    """(N, 3) float64 multiples of 1 / 32 in [0, 128): exact in float32 in every frame used below; clumps over a uniform background"""
    p = np.floor(st_points(4000, 128.0, 23) * 32.0) / 32.0
    p.setflags(write=False)
    return p


def st_points(npts, L, seed):
    rng = np.random.default_rng(seed)
    half = npts // 2
    centres = rng.uniform(0, L, (12, 3))
    clump = centres[rng.integers(0, 12, half)] + rng.normal(0, 0.06 * L, (half, 3))
    return np.mod(np.concatenate([clump, rng.uniform(0, L, (npts - half, 3))]), L)


@pytest.mark.parametrize('n', (16, 24))
@pytest.mark.parametrize('paste', ('CIC', 'TSC'))
def test_find_voids_from_particles(paste, n):
    from abacusutils_amd.analysis.voids import find_voids
    L = 128.0
    pos = _dyadic_points()
    radii = np.array([3.0, 2.0, 1.25]) * L / n
    before = pos.copy()
    got = find_voids(pos, L, radii, nmesh=n, paste=paste, return_fields=True)
    assert np.array_equal(pos, before)
    fields = got['fields']
    assert len(fields) == 3 and all(f.shape == (n, n, n) and f.dtype == np.float32 and np.isfinite(f).all() for f in fields)
    D = st.d_table(radii, L, n)
    want = st.find_sequential(fields, D, THR)
    _assert_equal(got, want, st.find_rounds(fields, D, THR)['rounds'], f'{paste} n={n}')
    assert len(got['level']) >= 3 and (want['counts'][:, 1] > 0).sum() >= 2      # voids at two levels at least
    np.testing.assert_array_equal(got['centres'], got['cell'].astype(np.float64) * (L / n))
    np.testing.assert_array_equal(got['radius'], radii[got['level']])
    assert (got['centres'] >= 0).all() and (got['centres'] < L).all() and np.array_equal(got['radii'], radii)
    for v in range(len(got['level'])):                                  # delta is the centre value of its level's field
        i, j, k = got['cell'][v]
        assert fields[got['level'][v]][i, j, k] == got['delta'][v]
    # the frames: [-L/2, L/2), unwrapped, float32 and device columns - the wrapped float32 positions are the same numbers
    shifted = np.where(pos >= L / 2, pos - L, pos)
    unwrapped = pos + L * np.random.default_rng(5).integers(-1, 3, pos.shape)
    lib = _lib()
    cols = [lib.DeviceArray(np.ascontiguousarray(shifted[:, a])) for a in range(3)]
    try:
        others = dict(shifted=find_voids(shifted, L, radii, nmesh=n, paste=paste), unwrapped=find_voids(unwrapped, L, radii, nmesh=n, paste=paste),
                      float32=find_voids(pos.astype(np.float32), L, radii, nmesh=n, paste=paste), columns=find_voids(cols, L, radii, nmesh=n, paste=paste))
    finally:
        for c in cols:
            c.free()
    for label, r in others.items():
        assert 'fields' not in r
        _assert_equal(r, got, got['counts'][:, 2], f'{paste} n={n} {label}')
    w = np.random.default_rng(9).uniform(0.2, 2.0, len(pos)).astype(np.float32)
    weighted = find_voids(pos, L, radii, nmesh=n, paste=paste, w=w, compensated=False, interlaced=False, return_fields=True)
    assert not np.array_equal(weighted['fields'][0], fields[0])
    _assert_equal(weighted, st.find_sequential(weighted['fields'], D, THR), None, f'{paste} n={n} weighted')


# ------------------------------------------------------------------------------------------------- 3. the fields
def _stages(n):
    return max(1.0, math.log2(float(n) ** 3) / math.log2(16.0 ** 3))


@pytest.mark.parametrize('n', (16, 24))
def test_fields_against_the_float64_statement(n):
    from abacusutils_amd.analysis.voids import find_voids, tophat_smooth
    L = 1000.0
    white = np.random.default_rng(400 + n).standard_normal((n, n, n))
    spec = (np.fft.rfftn(white) / float(n) ** 3).astype(np.complex64)
    for label, R in (('R = a', L / n), ('R = L/4', L / 4), ('R = 0', 0.0)):
        f64, f32 = st.tophat_field(spec, n, L, R, np.float64), st.tophat_field(spec, n, L, R, np.float32)
        e_ref = np.abs(f32 - f64).max() / np.abs(f64).max()
        assert 1e-8 < e_ref < 1e-5, f'e_ref {e_ref:.3g} outside (1e-8, 1e-5): the statement is broken'
        got = tophat_smooth(spec, L, R)
        assert got.dtype == np.float32 and got.shape == (n, n, n)
        err = np.abs(got - f64).max() / np.abs(f64).max()
        print(f'top hat n={n} {label}: err {err:.3g} = {err / e_ref:.2f} e_ref (e_ref {e_ref:.3g}), bound {4 * _stages(n):.2f} e_ref')
        assert err <= 4 * e_ref * _stages(n)
    # the multiplier itself where the closed form cancels: a single mode of unit amplitude comes back with the amplitude W
    for s in (1, 2):
        one = np.zeros((n, n, n // 2 + 1), dtype=np.complex64)
        one[0, 0, s] = 0.5                                              # a cosine of amplitude 1 along z
        R = 0.04 * L / (2 * np.pi * s)                                  # x = 0.04: the series branch
        got = tophat_smooth(one, L, R)
        W = float(st.tophat_w(0.04))
        assert abs(W - (1 - 0.04**2 / 10)) < 1e-6
        assert abs(float(got.max()) - W) <= 4 * 2.0**-24 * (3 * np.log2(n) + 2), (got.max(), W)
    # a constant density: one particle at every cell centre - the contrast is 0 and there is no void
    g = np.arange(n) * (L / n)
    lattice = np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3)
    r = find_voids(lattice, L, (L / 8, L / 16), nmesh=n, paste='CIC', return_fields=True)
    assert max(np.abs(f).max() for f in r['fields']) < 1e-5
    assert len(r['level']) == 0 and r['counts'].sum() == 0


# ------------------------------------------------------------------------------------------------- 4. planted voids
def test_planted_voids_on_the_device():
    from abacusutils_amd.analysis.voids import find_voids, void_size_function
    p = st.PLANTED
    got = find_voids(st.planted_points(), p['L'], p['radii'], threshold=p['threshold'], nmesh=p['n'])
    check_planted(got['cell'], got['level'], got['delta'])
    assert got['level'].tolist() == [0, 1, 1, 2] and got['radius'].tolist() == [28.0, 20.0, 20.0, 14.0]
    assert void_size_function(got, p['radii'], p['L'])['counts'].tolist() == [1, 2, 1]


# ------------------------------------------------------------------------------------------------- 5. void-galaxy xi
def test_void_galaxy_xi_against_brute_force():
    from abacusutils_amd.analysis.voids import void_galaxy_xi
    L, n = 128.0, 16
    gal = _dyadic_points()[:1500].astype(np.float32)
    rng = np.random.default_rng(31)
    cell = rng.integers(0, n, (40, 3)).astype(np.int32)
    voids = dict(centres=cell.astype(np.float64) * (L / n), level=rng.integers(0, 3, 40).astype(np.int32))
    bins = np.array([0.0, 4.3, 9.7, 17.1, 30.3])
    for levels in (None, [0, 2], 1):
        pick = np.ones(40, dtype=bool) if levels is None else np.isin(voids['level'], levels)
        want, margin = st.cross_pairs(voids['centres'][pick], gal, L, bins)
        assert margin > 1e-4                                          # no pair within float32 noise of an edge: the counts are exact
        got = void_galaxy_xi(voids, gal[:, 0].copy(), gal[:, 1].copy(), gal[:, 2].copy(), L, bins, levels=levels)
        np.testing.assert_array_equal(got['npairs'].astype(np.int64), want)
        assert got['nvoids'] == pick.sum() and got['ngal'] == 1500 and want.sum() > 1000
        dV = 4.0 * np.pi / 3.0 * (bins[1:] ** 3 - bins[:-1] ** 3)
        xi = want / (pick.sum() * 1500 * dV / L**3) - 1.0
        np.testing.assert_allclose(got['xi'], xi, rtol=1e-12, atol=0)
        np.testing.assert_array_equal(got['r'], 0.5 * (bins[1:] + bins[:-1]))


# ------------------------------------------------------------------------------------------------- 6. AbacusHOD.compute_voids
class _Mock(dict):
    """a mock dictionary whose columns are also resident in HBM, as GRAND_HOD.MockDict.device_xyz hands them out"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.dev = {}

    def device_xyz(self, tracer):
        if tracer not in self.dev:
            self.dev[tracer] = [_lib().DeviceArray(np.ascontiguousarray(self[tracer][c], dtype=np.float64)) for c in 'xyz']
        return self.dev[tracer]


def test_abacus_hod_compute_voids():
    from abacusutils_amd.analysis.voids import find_voids
    from abacusutils_amd.hod.abacus_hod import AbacusHOD
    L, n = 128.0, 24
    radii = (14.0, 9.0, 6.0)
    pos = _dyadic_points()
    w = np.random.default_rng(4).uniform(0.5, 1.5, 1500).astype(np.float32)
    cols = dict(LRG=dict(zip('xyz', pos.T.copy())), ELG=dict(zip('xyz', pos[:1500].T.copy()), w=w))
    before = {tr: {c: v.copy() for c, v in d.items()} for tr, d in cols.items()}
    ball = AbacusHOD.__new__(AbacusHOD)
    ball.lbox = L
    mock = _Mock(cols)
    try:
        dev = ball.compute_voids(mock, radii, num_cells=n)
        assert set(mock.dev) == {'LRG', 'ELG'}                         # the columns came from HBM
        for tr in mock.dev:
            for c, col in zip('xyz', mock.dev[tr]):
                assert np.array_equal(col.get(), before[tr][c])
    finally:
        for d in mock.dev.values():
            for c in d:
                c.free()
    assert set(dev) == {'LRG', 'ELG'}
    for tr in cols:
        fetched = np.stack([cols[tr][c] for c in 'xyz'], axis=1)
        want = find_voids(fetched, L, radii, nmesh=n, w=cols[tr].get('w'))
        _assert_equal(dev[tr], want, want['counts'][:, 2], tr)
        np.testing.assert_array_equal(dev[tr]['centres'], want['centres'])
        assert len(dev[tr]['level']) >= 2
        for c in before[tr]:
            assert np.array_equal(cols[tr][c], before[tr][c])
    assert not np.array_equal(dev['LRG']['cell'], dev['ELG']['cell'])


# ------------------------------------------------------------------------------------------------- 7. errors
def test_errors_come_before_any_launch():
    lib = _lib()
    L = lib.lib()
    n = 8
    some = lib.DeviceArray(np.full((n, n, n), -1.0, dtype=np.float32))
    other = lib.DeviceArray(nbytes=n * n * _pitch(n) * 4, dtype=np.float32, shape=(n, n, _pitch(n)))
    D = np.array([[9, 7], [7, 4]], dtype=np.int64)
    handle = C.c_void_p()
    lib.check(L.abacus_void_create(n, 2, lib.ptr(D), C.byref(handle)))
    c = [C.c_int64(0) for _ in range(3)]
    out = [C.byref(x) for x in c]
    lib.check(L.abacus_void_level_dev(handle, some.ptr, n, 0, C.c_float(THR), *out))        # level 0 is taken: 512 candidates
    assert c[0].value == n**3 and c[1].value > 0 and c[2].value > 0
    lib.sync()
    lib.profile_reset()
    lib.profile_enable(True)
    try:
        def refused(rc, match, entry):
            assert rc != 0
            msg = L.abacus_last_error().decode()
            assert msg.startswith(entry + ':') and match in msg, msg

        def create(n=n, m=2, D=D, handle_out=True):
            h = C.c_void_p()
            rc = L.abacus_void_create(n, m, None if D is None else lib.ptr(np.ascontiguousarray(D, dtype=np.int64)), C.byref(h) if handle_out else None)
            assert rc != 0 and not h.value
            return rc

        for kw, match in ((dict(n=7), 'odd'), (dict(n=2), 'out of range'), (dict(n=1026), 'out of range'), (dict(m=0), 'levels'),
                          (dict(m=33, D=np.ones((33, 33))), 'levels'), (dict(D=[[9, 7], [6, 4]]), 'symmetric'), (dict(D=[[9, 0], [0, 4]]), 'positive'),
                          (dict(D=[[9, -7], [-7, 4]]), 'positive'), (dict(D=[[17, 7], [7, 4]]), 'exceeds'), (dict(D=None), 'null'),
                          (dict(handle_out=False), 'null')):
            refused(create(**kw), match, 'abacus_void_create')

        def level(h=handle, mesh=some.ptr, pitch=n, lv=1, thr=THR, outs=out):
            return L.abacus_void_level_dev(h, mesh, pitch, lv, C.c_float(thr), *outs)

        who = 'abacus_void_level_dev'
        refused(level(pitch=n - 1), 'pitch', who)
        refused(level(lv=2), 'out of range', who)
        refused(level(lv=-1), 'out of range', who)
        refused(level(lv=0), 'increasing order', who)                   # given twice
        refused(level(thr=np.nan), 'finite', who)
        refused(level(thr=np.inf), 'finite', who)
        refused(level(mesh=None), 'null', who)
        refused(level(h=None), 'null', who)
        refused(level(outs=[out[0], None, out[2]]), 'null', who)
        refused(L.abacus_void_count(handle, None), 'null', 'abacus_void_count')
        refused(L.abacus_void_fetch(handle, None, None, None), 'null', 'abacus_void_fetch')
        stale = C.c_void_p(handle.value)
        lib.check(L.abacus_void_free(handle))
        refused(level(h=stale), 'not a live', who)
        nv = C.c_int64(0)
        refused(L.abacus_void_count(stale, C.byref(nv)), 'not a live', 'abacus_void_count')
        refused(L.abacus_void_fetch(stale, None, None, None), 'not a live', 'abacus_void_fetch')
        refused(L.abacus_void_free(stale), 'not a live', 'abacus_void_free')
        assert L.abacus_void_free(None) == 0

        def tophat(spec=other.ptr, n=n, Lbox=100.0, R=5.0, dst=some.ptr):
            return L.abacus_void_tophat_dev(spec, n, C.c_double(Lbox), C.c_double(R), dst)

        who = 'abacus_void_tophat_dev'
        refused(tophat(spec=None), 'null', who)
        refused(tophat(dst=None), 'null', who)
        refused(tophat(n=7), 'odd', who)
        refused(tophat(n=2), 'out of range', who)
        refused(tophat(n=1026), 'out of range', who)
        refused(tophat(dst=other.ptr), 'different', who)
        refused(tophat(Lbox=0.0), 'Lbox', who)
        refused(tophat(R=-1.0), 'R must', who)
        refused(tophat(R=np.nan), 'R must', who)
        who = 'abacus_void_check_memory'
        refused(L.abacus_void_check_memory(7, 0), 'odd', who)
        refused(L.abacus_void_check_memory(2048, 0), 'out of range', who)
        refused(L.abacus_void_check_memory(16, -1), 'negative', who)
        refused(L.abacus_void_check_memory(1024, 10**12), 'largest mesh that fits', who)
        names = lib.profile_get()
        assert not any(k.startswith('void_') or k.startswith('scan_') or k.startswith('hipfft') for k in names), f'a kernel was launched: {names}'
    finally:
        lib.profile_enable(False)
        some.free()
        other.free()
