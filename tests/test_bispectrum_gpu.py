"""The bispectrum on the device (abacusutils_amd.analysis.bispectrum, C ABI abacus_bk_*) against the NumPy statement
tests/bispectrum_statement.py.  Every comparison runs over ALL cells / bins.  Needs an MI355X: run with `-m gpu`.

Bounds: the rule of tests/test_lc_power_gpu.py `_check`: err / max |want| <= factor e_ref with factor = 4 max(1, log2(n^3) / log2(16^3)),
`e_ref` the statement's own float32 noise (its float32 evaluation against its float64 one, relative to the largest value), taken per
quantity, and 1e-8 < e_ref < 1e-4 asserted so that a broken statement cannot loosen a bound.  The float32 statement of the sums adds
in float32 over blocks of 128 consecutive cells, as the C ABI states the device may, so its e_ref carries the noise of such chains (the
order inside a block differs on the device: the bound is statistical in the same way as for the transforms).  Every ratio err / e_ref is
printed; the measured ones are recorded in profiles/bispectrum/README.md.

Shapes: n = 16 (power of two) and n = 24 (mixed radix; a row of 24 cells is one and a half 16-cell steps of the MFMA kernel, pitch 32
leaves 8 pad columns; n = 16 has pitch 32 as well, 16 pad columns); 3000 uniform points; linear edges from 0.5 dk to n / 3 dk.  Shell
counts 1, 5, 16, 17, 32: one tile group below, at and above the 16-column tile and the full two blocks.

interlaced=True: abacus_zcv_spectrum_dev accepts it at both sizes (calc_power runs interlaced at n = 24 in tests/test_power_gpu.py).  The
statement has no interlaced deposit, so that case is judged from the spectrum on: the statement runs on the spectrum fetched from the
device."""
import ctypes as C
import functools
import itertools
import math

import bispectrum_statement as st
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = (16, 24)
L = 1000.0
DK = 2.0 * np.pi / L
NPTS = 3000
SENTINEL = 7.25


def _stages(n):
    return max(1.0, math.log2(float(n) ** 3) / math.log2(16.0 ** 3))


def _edges(n, nb):
    return np.linspace(0.5, n / 3, nb + 1) * DK


def _eref(label, x32, x64):
    e = st.e_ref(x32, x64)
    assert 1e-8 < e < 1e-4, f'{label}: e_ref {e:.3g} outside (1e-8, 1e-4): the statement is broken'
    return e


def _check(label, got, want, e_ref, n, scale=1.0):
    factor = 4.0 * _stages(n) * scale
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max() / np.abs(want).max()
    print(f'{label}: err {err:.3g}, e_ref {e_ref:.3g}, err / e_ref {err / e_ref:.3g} (bound {factor:.3g})')
    assert err <= factor * e_ref, f'{label}: {err:.3g} > {factor:.3g} x {e_ref:.3g}'


@functools.lru_cache(maxsize=None)
def _points():
    return st.uniform_points(NPTS, L, 11)


@functools.lru_cache(maxsize=None)
def _spectrum(n):
    """the statement's spectrum of the points as the device holds one: complex64"""
    return st.density_spectrum(_points(), None, n, L).astype(np.complex64)


@functools.lru_cache(maxsize=None)
def _fields(n, nb, ones=False):
    """(float64 statement, float32 statement) of the shell fields"""
    spec = None if ones else _spectrum(n)
    return tuple(st.shell_fields(spec, n, L, _edges(n, nb), t) for t in (np.float64, np.float32))


@functools.lru_cache(maxsize=None)
def _sums(n, nb):
    """the float32 shell fields of the statement as the meshes under test, and (float64 sums, float32 sums) of exactly these meshes"""
    m = _fields(n, nb)[1]
    return m, st.sums(m), st.sums(m, np.float32)


# ------------------------------------------------------------------------------------------------- the device side
def _lib():
    from abacusutils_amd import _lib
    return _lib


def _table(devs):
    return (C.c_void_p * len(devs))(*[d.ptr.value for d in devs])


def _device_shells(spec, n, nb):
    """the nb padded meshes (nb, n, n, pitch) after abacus_bk_shells_dev; every float holds SENTINEL before the call"""
    lib = _lib()
    pitch = (n + 2 + 31) // 32 * 32
    devs = [lib.DeviceArray(np.full((n, n, pitch), SENTINEL, dtype=np.float32)) for _ in range(nb)]
    sdev = None
    try:
        if spec is not None:
            row = np.zeros((n, n, pitch // 2), dtype=np.complex64)
            row[:, :, :n // 2 + 1] = spec
            sdev = lib.DeviceArray(row)
        ke = np.ascontiguousarray(_edges(n, nb))
        lib.check(lib.lib().abacus_bk_shells_dev(None if sdev is None else sdev.ptr, n, C.c_double(L), lib.ptr(ke), nb, _table(devs)))
        return np.stack([d.get() for d in devs])
    finally:
        for d in devs + ([] if sdev is None else [sdev]):
            d.free()


def _device_triple(meshes, n, pad_value=0.0):
    lib = _lib()
    nb = len(meshes)
    devs = [lib.DeviceArray(st.padded(m, pad_value)) for m in meshes]
    try:
        T, G = np.full((nb, nb, nb), np.nan), np.full(nb, np.nan)
        lib.check(lib.lib().abacus_bk_triple_dev(_table(devs), n, nb, lib.ptr(T), lib.ptr(G)))
        return T, G
    finally:
        for d in devs:
            d.free()


# ------------------------------------------------------------------------------------------------- 1. shell fields
@pytest.mark.parametrize('nb', (5, 17))
@pytest.mark.parametrize('n', NS)
def test_shell_fields(n, nb):
    for ones in (False, True):
        f64, f32 = _fields(n, nb, ones)
        got = _device_shells(None if ones else _spectrum(n), n, nb)
        name = 'I' if ones else 'D'
        _check(f'{name} fields n={n} nb={nb}', got[..., :n], f64, _eref(name, f32, f64), n)
        assert (got[..., n + 2:] == SENTINEL).all(), 'a pad column was written'


# ------------------------------------------------------------------------------------------------- 2. the sums
@pytest.mark.parametrize('nb', (1, 5, 16, 17, 32))
@pytest.mark.parametrize('n', NS)
def test_triple_sums(n, nb):
    m, (T64, G64), (T32, G32) = _sums(n, nb)
    # G against its own noise floor.  T against the larger of its own and G's: the same arithmetic makes both, and with one shell T is a
    # single number whose float32 error is one draw
    eG = st.e_ref(G32, G64)
    assert 1e-9 < eG < 1e-4, f'G: e_ref {eG:.3g} outside (1e-9, 1e-4): the statement is broken'
    eT = max(eG, _eref('T', T32, T64) if nb > 1 else st.e_ref(T32, T64))
    T, G = _device_triple(m, n)
    _check(f'T n={n} nb={nb}', T, T64, eT, n)
    _check(f'G n={n} nb={nb}', G, G64, eG, n)
    # a value planted in every pad column changes no bit, and neither does a second call
    T2, G2 = _device_triple(m, n, pad_value=3.0)
    assert np.array_equal(T, T2) and np.array_equal(G, G2), 'the pad columns entered the sums, or two runs differ'
    # T is symmetric under every permutation of (i, j, l) up to the bound (two entries, each within it)
    sym = max(np.abs(T - T.transpose(p)).max() for p in itertools.permutations(range(3))) / np.abs(T64).max()
    print(f'symmetry n={n} nb={nb}: {sym:.3g} of max |T|, {sym / eT:.3g} e_ref')
    assert sym <= 2 * 4.0 * _stages(n) * eT
    if nb > 1:                                    # the cube is not one number repeated: a wrong (i, j, l) map cannot pass
        assert np.unique(np.round(T64 / np.abs(T64).max(), 6)).size > nb


# ------------------------------------------------------------------------------------------------- 3. end to end
def _check_result(label, got, s64, s32, n):
    assert np.array_equal(got['ijl'], s64['ijl']), label
    for key in ('B', 'P', 'N_tri'):
        _check(f'{label} {key}', got[key], s64[key], _eref(f'{label} {key}', s32[key], s64[key]), n)
    np.testing.assert_allclose(got['k_mean'], s64['k_mean'], rtol=1e-14)
    np.testing.assert_allclose(got['N_mode'], s64['N_mode'], rtol=0, atol=1e-3)
    for a, b in zip('123', range(3)):
        assert np.array_equal(got['k' + a], got['k_mean'][got['ijl'][:, b]])
    assert got['N_tri'].dtype == np.float64


@pytest.mark.parametrize('paste,compensated', (('TSC', True), ('CIC', True), ('TSC', False)))
@pytest.mark.parametrize('n', NS)
def test_calc_bispectrum(n, paste, compensated):
    from abacusutils_amd.analysis.bispectrum import calc_bispectrum
    ke = _edges(n, 5)
    pos = _points()
    before = pos.copy()
    got = calc_bispectrum(pos, L, ke, nmesh=n, paste=paste, compensated=compensated, interlaced=False)
    assert np.array_equal(pos, before)
    s64, s32 = (st.bispectrum(pos, L, ke, n, None, paste, compensated, t) for t in (np.float64, np.float32))
    _check_result(f'n={n} {paste} compensated={compensated}', got, s64, s32, n)
    P_shot, B_shot, Q = st.shot_noise_and_Q(got['B'], got['P'], got['ijl'], NPTS / L**3)
    assert got['P_shot'] == P_shot
    np.testing.assert_allclose(got['B_shot'], B_shot, rtol=1e-14)
    np.testing.assert_allclose(got['Q'], Q, rtol=1e-12)


@pytest.mark.parametrize('n', NS)
def test_calc_bispectrum_interlaced_and_weighted(n):
    """interlaced=True from the spectrum on (module docstring): the statement runs on the spectrum the device made of the same points"""
    from abacusutils_amd.analysis.bispectrum import _padded, calc_bispectrum
    from abacusutils_amd.analysis.power_spectrum import get_W_compensated
    lib = _lib()
    ke = _edges(n, 5)
    pos = _points()
    w = np.random.default_rng(3).uniform(0.5, 1.5, NPTS).astype(np.float32)
    for weights in (None, w):
        got = calc_bispectrum(pos, L, ke, nmesh=n, w=weights, interlaced=True)
        W = np.ascontiguousarray(get_W_compensated(L, n, 'TSC', True), dtype=np.float32)
        work, spec = lib.DeviceArray(pos.astype(np.float32)), _padded(n)
        wdev = None if weights is None else lib.DeviceArray(weights)
        try:
            lib.check(lib.lib().abacus_zcv_spectrum_dev(work.ptr, C.c_int64(NPTS), None if wdev is None else wdev.ptr, C.c_double(L), n, 0,
                                                        lib.ptr(W), 1, spec.ptr))
            host = np.empty((n, n, n // 2 + 1), dtype=np.complex64)
            lib.check(lib.lib().abacus_zcv_spectrum_fetch(spec.ptr, n, lib.ptr(host)))
        finally:
            for d in (work, spec, wdev):
                if d is not None:
                    d.free()
        N_gal = None if weights is not None else NPTS
        s64, s32 = (st.bispectrum_from_spectrum(host, n, L, ke, N_gal, t) for t in (np.float64, np.float32))
        _check_result(f'n={n} interlaced weighted={weights is not None}', got, s64, s32, n)
        if weights is None:                       # (Q divides by a sum of products of P that may nearly cancel: held to its formula)
            np.testing.assert_allclose(got['Q'], st.shot_noise_and_Q(got['B'], got['P'], got['ijl'], NPTS / L**3)[2], rtol=1e-12)
        else:
            assert got['Q'] is None and got['B_shot'] is None and got['P_shot'] is None


# ------------------------------------------------------------------------------------------------- 4. triangle counts and their cache
@pytest.mark.parametrize('n', NS)
def test_triangle_counts_are_the_brute_integers_and_are_cached(n):
    from abacusutils_amd.analysis import bispectrum as bk
    ke = _edges(n, 5)
    _, Nb = st.brute(None, n, L, ke)
    bk._counts.clear()
    built = bk.counts_built()
    c = bk.triangle_counts(n, L, ke)
    assert bk.counts_built() == built + 1
    assert np.array_equal(np.rint(c['N']).astype(np.int64), Nb)
    print(f'n={n}: N up to {Nb.max()}, largest distance from an integer {np.abs(c["N"] - Nb).max():.3g}')
    _, cnt = st.k_mean(n, L, ke)
    assert np.array_equal(np.rint(c['M']), cnt)
    pos = _points()
    a = bk.calc_bispectrum(pos, L, ke, nmesh=n, interlaced=False)
    b = bk.calc_bispectrum(pos[:2000], L, ke, nmesh=n, interlaced=False)
    assert bk.counts_built() == built + 1 and bk.triangle_counts(n, L, ke) is c
    assert np.array_equal(a['N_tri'], b['N_tri']) and np.array_equal(np.rint(a['N_tri']).astype(np.int64), Nb[tuple(a['ijl'].T)])
    bk.calc_bispectrum(pos, L, _edges(n, 4), nmesh=n, interlaced=False)            # other edges: built again
    assert bk.counts_built() == built + 2


# ------------------------------------------------------------------------------------------------- 5. AbacusHOD.compute_bispectrum
class _Mock(dict):
    """a mock dictionary whose columns are also resident in HBM, as GRAND_HOD.MockDict.device_xyz hands them out"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.dev = {}

    def device_xyz(self, tracer):
        if tracer not in self.dev:
            self.dev[tracer] = [_lib().DeviceArray(np.ascontiguousarray(self[tracer][c], dtype=np.float64)) for c in 'xyz']
        return self.dev[tracer]


def test_abacus_hod_compute_bispectrum():
    from abacusutils_amd.analysis.bispectrum import calc_bispectrum
    from abacusutils_amd.hod.abacus_hod import AbacusHOD
    n = 24
    ke = _edges(n, 5)
    pos = _points()
    w = np.random.default_rng(4).uniform(0.5, 1.5, 2000).astype(np.float32)
    cols = dict(LRG=dict(zip('xyz', pos.T.copy())), ELG=dict(zip('xyz', pos[:2000].T.copy()), w=w))
    before = {tr: {c: v.copy() for c, v in d.items()} for tr, d in cols.items()}
    ball = AbacusHOD.__new__(AbacusHOD)
    ball.lbox = L
    mock = _Mock(cols)
    try:
        dev = ball.compute_bispectrum(mock, ke, num_cells=n)
        assert set(mock.dev) == {'LRG', 'ELG'}                 # the columns came from HBM
        for tr in mock.dev:
            for c, col in zip('xyz', mock.dev[tr]):
                assert np.array_equal(col.get(), before[tr][c])
    finally:
        for d in mock.dev.values():
            for c in d:
                c.free()
    host = ball.compute_bispectrum(cols, ke, num_cells=n)
    for tr in cols:
        for c in before[tr]:
            assert np.array_equal(cols[tr][c], before[tr][c])
    want = dict(LRG=calc_bispectrum(pos, L, ke, nmesh=n), ELG=calc_bispectrum(pos[:2000], L, ke, nmesh=n, w=w))
    s64, s32 = (st.bispectrum(pos, L, ke, n, None, 'TSC', True, t) for t in (np.float64, np.float32))
    eB, eP = _eref('B', s32['B'], s64['B']), _eref('P', s32['P'], s64['P'])
    assert set(dev) == set(host) == {'LRG', 'ELG'}
    for tr in cols:                                            # the same float32 positions either way; the deposit's sums are not ordered
        for other in (host, want):
            assert np.array_equal(dev[tr]['ijl'], other[tr]['ijl'])
            _check(f'compute_bispectrum {tr} B', dev[tr]['B'], other[tr]['B'], eB, n)
            _check(f'compute_bispectrum {tr} P', dev[tr]['P'], other[tr]['P'], eP, n)
    assert dev['ELG']['Q'] is None and dev['LRG']['Q'] is not None


# ------------------------------------------------------------------------------------------------- 6. errors
def test_errors_come_before_any_launch():
    from abacusutils_amd.analysis import bispectrum as bk
    lib = _lib()
    n = 16
    ke = np.ascontiguousarray(_edges(n, 5))
    some = lib.DeviceArray(nbytes=64, dtype=np.uint8, shape=(64,))            # never read or written: every call below is refused
    lib.profile_reset()
    lib.profile_enable(True)
    try:
        def refused(rc, match):
            assert rc != 0
            msg = lib.lib().abacus_last_error().decode()
            assert msg.startswith('abacus_bk_') and match in msg, msg

        def shells(n=n, ke=ke, nb=5, spec=None):
            tab = (C.c_void_p * 33)(*[some.ptr.value + 0 for _ in range(33)])
            return lib.lib().abacus_bk_shells_dev(spec, n, C.c_double(L), lib.ptr(np.ascontiguousarray(ke)), nb, tab)

        T, G = np.zeros(33**3), np.zeros(33)
        tab = (C.c_void_p * 33)(*[some.ptr.value for _ in range(33)])
        refused(shells(n=15), 'odd')
        refused(shells(nb=0), 'shells')
        refused(shells(nb=33, ke=np.linspace(0.5, 5.3, 34) * DK), 'shells')
        refused(shells(ke=ke[::-1]), 'increase')
        refused(shells(ke=np.linspace(0.5, 5.5, 6) * DK), 'n / 3')
        refused(shells(), 'same buffer')
        refused(lib.lib().abacus_bk_triple_dev(tab, 15, 5, lib.ptr(T), lib.ptr(G)), 'odd')
        refused(lib.lib().abacus_bk_triple_dev(tab, n, 0, lib.ptr(T), lib.ptr(G)), 'shells')
        refused(lib.lib().abacus_bk_triple_dev(tab, n, 33, lib.ptr(T), lib.ptr(G)), 'shells')
        refused(lib.lib().abacus_bk_triple_dev(None, n, 5, lib.ptr(T), lib.ptr(G)), 'null')
        refused(lib.lib().abacus_bk_check_memory(15, 5, C.c_int64(0)), 'odd')
        # a mesh that cannot fit: refused from the sizes alone, naming the largest that does
        refused(lib.lib().abacus_bk_check_memory(32766, 32, C.c_int64(10**9)), 'largest mesh that fits')
        pos = _points()
        for kw, match in ((dict(nmesh=15), 'nmesh'), (dict(kedges=ke[:1]), 'shells'), (dict(kedges=np.linspace(0.5, 5.3, 35) * DK), 'shells'),
                          (dict(kedges=ke[::-1]), 'increasing'), (dict(kedges=np.linspace(0.5, 5.5, 6) * DK), 'n / 3')):
            with pytest.raises(ValueError, match=match):
                bk.calc_bispectrum(**{**dict(pos=pos, Lbox=L, kedges=ke, nmesh=n), **kw})
        with pytest.raises(lib.AbacusHipError, match='largest mesh that fits'):
            bk.calc_bispectrum(pos, L * 2000, _edges(32766, 32) / 2000, nmesh=32766)
        assert not any(k.startswith('bk_') for k in lib.profile_get()), 'a kernel was launched'
    finally:
        lib.profile_enable(False)
        some.free()
    assert bk.calc_bispectrum(pos, L, ke, nmesh=n, interlaced=False)['B'].shape == (32,)      # and the library still works
