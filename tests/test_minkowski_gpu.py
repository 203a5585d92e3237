"""The Minkowski functionals on the device (abacusutils_amd.analysis.minkowski, C ABI abacus_mf_*) against the NumPy statement
tests/minkowski_statement.py.  Needs an MI355X: run with `-m gpu`.

Counts are integers and are held to the statement exactly, over all thresholds.  Shapes: n = 2 (every neighbour is the mesh wrapping
onto itself), 3 and 5 (smaller than a tile of 16 x 64 cells, odd: a dense mesh takes the scalar loads, the padded copy with its pitch
of 32 the 16-byte loads with the wrap inside a float4), 16 (a dense mesh with 16-byte loads), 33 (one past two rows of tiles and one
past a chunk of 32 planes), 70 (one tile and 6 cells along z, not a multiple of anything).  The padded copies carry +1e30 in every pad
float: a read of the padding would put cells above every threshold.

Moments: |sum - float64 NumPy sum| <= n^3 2^-53 sum |x| (every term is exact in float64, at most n^3 roundings), the same for x^2.
Smoothing: max |got - want| / max |want| <= 4 e_ref (the rule of tests/test_shear_gpu.py), e_ref the statement's own float32 noise:
its float32 / complex64 evaluation against its float64 one, computed here."""
import ctypes as C
import functools

import minkowski_statement as st
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L = 1000.0
PAD = np.float32(1e30)
FIELDS = ('constant', 'spike0', 'spike1', 'plane', 'line', 'checker', 'normal', 'levels')


def _lib():
    from abacusutils_amd import _lib
    return _lib


def _pitch(n):
    return (n + 2 + 31) // 32 * 32


@functools.lru_cache(maxsize=None)
def _field(n, name):
    m = np.zeros((n, n, n), dtype=np.float32)
    if name == 'constant':
        m[:] = 0.5
    elif name == 'spike0':
        m[0, 0, 0] = 1.0
    elif name == 'spike1':
        m[n - 1, n - 1, n - 1] = 1.0
    elif name == 'plane':
        m[:, n - 1, :] = 1.0
    elif name == 'line':
        m[n - 1, 0, :] = 1.0
    elif name == 'checker':
        i = np.arange(n)
        m = ((i[:, None, None] + i[None, :, None] + i[None, None, :]) % 2).astype(np.float32)
    elif name == 'normal':
        m = np.random.default_rng(100 + n).standard_normal((n, n, n)).astype(np.float32)
    elif name == 'levels':
        m = (np.random.default_rng(200 + n).integers(0, 8, (n, n, n)) * 0.125).astype(np.float32)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _thresholds(n, name, nthr):
    """float32 thresholds: 1 - a value some cell holds (a tie); 2 - one below the minimum, one above the maximum; 64 - up to 8 values
    the cells hold (all 8 levels of the quantised field), a grid from below the minimum to above the maximum between them"""
    m = _field(n, name)
    vals, lo, hi = np.unique(m), m.min(), m.max()
    if nthr == 1:
        return np.array([vals[len(vals) // 2]], dtype=np.float32)
    if nthr == 2:
        return np.array([lo - 1, hi + 1], dtype=np.float32)
    picks = np.unique(vals[np.linspace(0, len(vals) - 1, 8).astype(int)])
    t = np.unique(np.concatenate([picks, np.linspace(lo - 1, hi + 1, nthr - len(picks)).astype(np.float32)]))
    while len(t) < nthr:
        t = np.append(t, t[-1] + np.float32(1))
    assert len(t) == nthr == 64 and t[0] < lo and t[-1] > hi and np.isin(picks, t).all() and t.dtype == np.float32
    return t


@functools.lru_cache(maxsize=None)
def _want(n, name, nthr):
    return st.counts(_field(n, name), _thresholds(n, name, nthr))


def _padded_dev(mesh):
    """the mesh in the padded layout, every pad float +1e30: through abacus_recon_pad_dev where it takes the size (even n), else
    uploaded in that layout"""
    lib = _lib()
    n = mesh.shape[0]
    full = np.full((n, n, _pitch(n)), PAD, dtype=np.float32)
    if n % 2:
        full[:, :, :n] = mesh
        return lib.DeviceArray(full)
    out, src = lib.DeviceArray(full), lib.DeviceArray(mesh)
    try:
        lib.check(lib.lib().abacus_recon_pad_dev(src.ptr, n, out.ptr))
    finally:
        src.free()
    return out


def _counts_c(dev, n, pitch, t32):
    lib = _lib()
    out = np.full((4, len(t32)), -1, dtype=np.int64)
    lib.check(lib.lib().abacus_mf_counts_dev(dev.ptr, n, pitch, lib.ptr(np.ascontiguousarray(t32)), len(t32), lib.ptr(out)))
    return out


# ------------------------------------------------------------------------------------------------- 1. counts
@pytest.mark.parametrize('n', (2, 3, 5, 16, 33, 70))
def test_counts_equal_the_statement(n):
    from abacusutils_amd.analysis.minkowski import minkowski_counts
    lib = _lib()
    for name in FIELDS:
        mesh = _field(n, name)
        dense, padded = lib.DeviceArray(mesh), _padded_dev(mesh)
        try:
            for nthr in (1, 2, 64):
                t, want = _thresholds(n, name, nthr), _want(n, name, nthr)
                np.testing.assert_array_equal(minkowski_counts(mesh, t), want, err_msg=f'{name} n={n} nthr={nthr} host mesh')
                got = minkowski_counts(dense, t)
                assert got.dtype == np.int64 and got.shape == (4, nthr)
                np.testing.assert_array_equal(got, want, err_msg=f'{name} n={n} nthr={nthr} DeviceArray')
                np.testing.assert_array_equal(_counts_c(padded, n, _pitch(n), t), want, err_msg=f'{name} n={n} nthr={nthr} padded')
            assert np.array_equal(dense.get(), mesh), 'the mesh was modified'
            back = padded.get()
            assert np.array_equal(back[:, :, :n], mesh) and (back[:, :, n:] == PAD).all(), 'the padded mesh was modified'
        finally:
            dense.free()
            padded.free()
    # the known answers once more, on the device
    N = n**3
    for name in ('spike0', 'spike1'):
        assert tuple(_want(n, name, 1)[:, 0]) == (8, 12, 6, 1)
    assert tuple(_want(n, 'constant', 1)[:, 0]) == (N, 3 * N, 3 * N, N)


# ------------------------------------------------------------------------------------------------- 2. moments
@pytest.mark.parametrize('n', (5, 16, 33, 70))
def test_moments(n):
    from abacusutils_amd.analysis.minkowski import mesh_moments
    lib = _lib()
    mesh = (_field(n, 'normal') * np.float32(3.0) + np.float32(0.75)).astype(np.float32)
    x = mesh.astype(np.float64)
    want = np.array([x.sum(), (x * x).sum()])
    bound = float(n) ** 3 * 2.0**-53 * np.array([np.abs(x).sum(), (x * x).sum()])
    dense, padded = lib.DeviceArray(mesh), _padded_dev(mesh)
    try:
        sums = []
        for dev, pitch in ((dense, n), (padded, _pitch(n)), (dense, n)):
            s = np.full(2, np.nan)
            lib.check(lib.lib().abacus_mf_moments_dev(dev.ptr, n, pitch, lib.ptr(s)))
            print(f'n={n} pitch={pitch}: |sum - want| = {np.abs(s - want)}, bound {bound}')
            assert (np.abs(s - want) <= bound).all()
            sums.append(s)
        assert sums[0].tobytes() == sums[2].tobytes(), 'two calls differ'
        mean, var = mesh_moments(dense)
        assert (mean, var) == mesh_moments(mesh)
        N = float(n) ** 3
        assert mean == sums[0][0] / N
        # var = S2 / N - mean^2 with mean^2 << S2 / N here is not assumed: the roundings of the two terms and of the difference
        assert var == sums[0][1] / N - mean * mean
        assert abs(var - (want[1] / N - (want[0] / N) ** 2)) <= (bound[1] + 2 * abs(want[0] / N) * bound[0]) / N + 2.0**-50 * want[1] / N
    finally:
        dense.free()
        padded.free()


# ------------------------------------------------------------------------------------------------- 3. smoothing
def _device_smooth(spec, n, R):
    """abacus_mf_smooth_spectrum_dev on the complex64 half spectrum (n, n, n/2 + 1): the (n, n, n) real mesh"""
    lib = _lib()
    row = np.zeros((n, n, _pitch(n) // 2), dtype=np.complex64)
    row[:, :, :n // 2 + 1] = spec
    dev = lib.DeviceArray(row)
    try:
        lib.check(lib.lib().abacus_mf_smooth_spectrum_dev(dev.ptr, n, C.c_double(L), C.c_double(R)))
        lib.sync()
        return dev.get().view(np.float32).reshape(n, n, _pitch(n))[:, :, :n].copy()
    finally:
        dev.free()


@pytest.mark.parametrize('n', (32, 48))
def test_smooth_spectrum(n):
    field = np.random.default_rng(300 + n).standard_normal((n, n, n))
    spec = (np.fft.rfftn(field) / float(n) ** 3).astype(np.complex64)
    for R in (2.5 * L / n, 0.0):
        f64, f32 = st.smooth_spectrum(spec, n, L, R, np.float64), st.smooth_spectrum(spec, n, L, R, np.float32)
        e_ref = np.abs(f32 - f64).max() / np.abs(f64).max()
        assert 1e-8 < e_ref < 1e-5, f'e_ref {e_ref:.3g} outside (1e-8, 1e-5): the statement is broken'
        got = _device_smooth(spec, n, R)
        err = np.abs(got - f64).max() / np.abs(f64).max()
        print(f'smoothing n={n} R={R:g}: err {err:.3g} = {err / e_ref:.2f} e_ref (e_ref {e_ref:.3g})')
        assert err <= 4 * e_ref
        if R > 0:                                         # and it did smooth: the variance fell by more than an order of magnitude
            assert got.var() < 0.1 * st.smooth_spectrum(spec, n, L, 0.0).var()
    # a constant field is the mode k = 0 alone, which the filter leaves as it is: every cell within the roundings of a transform that
    # adds zeros to it, one per stage of at most 3 log2(n) + 2 stages
    const = np.zeros((n, n, n // 2 + 1), dtype=np.complex64)
    const[0, 0, 0] = 0.7
    got = _device_smooth(const, n, 2.5 * L / n)
    assert np.abs(got - np.float32(0.7)).max() <= (3 * np.log2(n) + 2) * 2.0**-24 * 0.7


# ------------------------------------------------------------------------------------------------- 4. the chain
def _moment_bounds(field):
    """(|mean| bound, sigma bound) of the device's mean and sigma against the float64 NumPy ones of the same mesh: the bounds of the two
    sums carried through mean = S1 / N, var = S2 / N - mean^2, sigma = sqrt(var) (d sigma = d var / (2 sigma); the factor 2 is kept as
    slack for the roundings of these few operations)"""
    x = field.astype(np.float64)
    N = float(x.size)
    b1, b2 = N * 2.0**-53 * np.abs(x).sum(), N * 2.0**-53 * (x * x).sum()
    mean, sigma = x.mean(), x.std()
    dmean = b1 / N + 2.0**-52 * abs(mean)
    dvar = b2 / N + 2 * abs(mean) * dmean + 2.0**-51 * (x * x).mean()
    return mean, sigma, dmean, dvar / sigma + 2.0**-52 * sigma


@functools.lru_cache(maxsize=None)
def _points():
    p = st.clustered_points(20000, L, 17)
    p.setflags(write=False)
    return p


@pytest.mark.parametrize('n', (32, 48))
def test_calc_minkowski_chain(n):
    from abacusutils_amd.analysis.minkowski import calc_minkowski, minkowski_from_counts
    lib = _lib()
    pos, nu = _points(), np.linspace(-1.5, 4.0, 12)
    before = pos.copy()
    w = np.random.default_rng(5).uniform(0.5, 1.5, len(pos)).astype(np.float32)
    cols = [lib.DeviceArray(np.ascontiguousarray(pos[:, a])) for a in range(3)]
    try:
        runs = dict(host=calc_minkowski(pos, L, nu, 2.0 * L / n, nmesh=n, return_field=True),
                    columns=calc_minkowski(cols, L, nu, 2.0 * L / n, nmesh=n, return_field=True),
                    weighted=calc_minkowski(pos, L, nu, 2.0 * L / n, nmesh=n, w=w, return_field=True),
                    plain=calc_minkowski(pos.astype(np.float32), L, nu * 0.5, 0.0, nmesh=n, paste='CIC', compensated=False, interlaced=False,
                                         sigma_units=False, return_field=True))
        for a, col in enumerate(cols):
            assert np.array_equal(col.get(), before[:, a])
    finally:
        for c in cols:
            c.free()
    assert np.array_equal(pos, before)
    for label, r in runs.items():
        f = r['field']
        assert f.shape == (n, n, n) and f.dtype == np.float32 and np.isfinite(f).all()
        # exact on whatever mesh the device holds
        np.testing.assert_array_equal(r['counts'], st.counts(f, r['thresholds']), err_msg=label)
        np.testing.assert_array_equal(r['V'], minkowski_from_counts(r['counts'], n, L))
        mean, sigma, dmean, dsigma = _moment_bounds(f)
        print(f'{label} n={n}: mean {r["mean"]:.3g} (off {abs(r["mean"] - mean):.3g}, bound {dmean:.3g}), sigma {r["sigma"]:.6g} '
              f'(off {abs(r["sigma"] - sigma):.3g}, bound {dsigma:.3g})')
        assert abs(r['mean'] - mean) <= dmean and abs(r['sigma'] - sigma) <= dsigma
        assert sigma > 0.05 and abs(mean) < 1e-3                                # a density contrast: mean 0 up to float32 noise
        if label == 'plain':
            assert np.array_equal(r['thresholds'], (nu * 0.5).astype(np.float32))
        else:
            assert np.array_equal(r['thresholds'], (nu * r['sigma'] + r['mean']).astype(np.float32))
        assert (np.diff(r['V'][0]) <= 0).all() and 1.0 >= r['V'][0, 0] > r['V'][0, -1] >= 0.0
    assert not np.array_equal(runs['host']['field'], runs['weighted']['field'])
    without = calc_minkowski(pos, L, nu, 2.0 * L / n, nmesh=n)
    assert 'field' not in without and np.array_equal(without['counts'], runs['host']['counts'])


# ------------------------------------------------------------------------------------------------- 5. AbacusHOD.compute_minkowski
class _Mock(dict):
    """a mock dictionary whose columns are also resident in HBM, as GRAND_HOD.MockDict.device_xyz hands them out"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.dev = {}

    def device_xyz(self, tracer):
        if tracer not in self.dev:
            self.dev[tracer] = [_lib().DeviceArray(np.ascontiguousarray(self[tracer][c], dtype=np.float64)) for c in 'xyz']
        return self.dev[tracer]


def test_abacus_hod_compute_minkowski():
    from abacusutils_amd.hod.abacus_hod import AbacusHOD
    n, nu = 32, np.linspace(-1.0, 3.0, 9)
    pos = _points()
    w = np.random.default_rng(4).uniform(0.5, 1.5, 5000).astype(np.float32)
    cols = dict(LRG=dict(zip('xyz', pos.T.copy())), ELG=dict(zip('xyz', pos[:5000].T.copy()), w=w))
    before = {tr: {c: v.copy() for c, v in d.items()} for tr, d in cols.items()}
    ball = AbacusHOD.__new__(AbacusHOD)
    ball.lbox = L
    mock = _Mock(cols)
    try:
        dev = ball.compute_minkowski(mock, nu, 2.0 * L / n, num_cells=n)
        assert set(mock.dev) == {'LRG', 'ELG'}                 # the columns came from HBM
        for tr in mock.dev:
            for c, col in zip('xyz', mock.dev[tr]):
                assert np.array_equal(col.get(), before[tr][c])
    finally:
        for d in mock.dev.values():
            for c in d:
                c.free()
    host = ball.compute_minkowski(cols, nu, 2.0 * L / n, num_cells=n)
    for tr in cols:
        for c in before[tr]:
            assert np.array_equal(cols[tr][c], before[tr][c])
    assert set(dev) == set(host) == {'LRG', 'ELG'}
    for tr in cols:
        np.testing.assert_array_equal(dev[tr]['counts'], host[tr]['counts'])
        assert np.array_equal(dev[tr]['thresholds'], host[tr]['thresholds']) and np.array_equal(dev[tr]['V'], host[tr]['V'])
        assert dev[tr]['counts'][3, 0] > dev[tr]['counts'][3, -1] >= 0
    assert not np.array_equal(dev['LRG']['counts'], dev['ELG']['counts'])


# ------------------------------------------------------------------------------------------------- 6. errors
def test_errors_come_before_any_launch():
    lib = _lib()
    some = lib.DeviceArray(nbytes=4096, dtype=np.uint8, shape=(4096,))          # never read or written: every call below is refused
    lib.profile_reset()
    lib.profile_enable(True)
    try:
        def refused(rc, match):
            assert rc != 0
            msg = lib.lib().abacus_last_error().decode()
            assert msg.startswith('abacus_mf_') and match in msg, msg

        def counts(n=8, pitch=8, t=(0.0, 1.0), nthr=None, mesh=some.ptr):
            t32 = np.ascontiguousarray(t, dtype=np.float32)
            out = np.zeros((4, 65), dtype=np.int64)
            return lib.lib().abacus_mf_counts_dev(mesh, n, pitch, lib.ptr(t32), len(t32) if nthr is None else nthr, lib.ptr(out))

        refused(counts(n=1), 'out of range')
        refused(counts(n=32768), 'out of range')
        refused(counts(pitch=7), 'pitch')
        refused(counts(nthr=0), 'thresholds')
        refused(counts(t=np.arange(65.0)), 'thresholds')
        refused(counts(t=(1.0, 0.0)), 'increase')
        refused(counts(t=(1.0, 1.0 + 1e-9)), 'increase')
        refused(counts(t=(0.0, np.inf)), 'finite')
        refused(counts(t=(np.nan,)), 'finite')
        refused(counts(mesh=None), 'null')
        s = np.zeros(2)
        refused(lib.lib().abacus_mf_moments_dev(some.ptr, 1, 1, lib.ptr(s)), 'out of range')
        refused(lib.lib().abacus_mf_moments_dev(some.ptr, 8, 4, lib.ptr(s)), 'pitch')
        refused(lib.lib().abacus_mf_smooth_spectrum_dev(some.ptr, 7, C.c_double(L), C.c_double(1.0)), 'odd')
        refused(lib.lib().abacus_mf_smooth_spectrum_dev(some.ptr, 8, C.c_double(L), C.c_double(-1.0)), 'R must')
        refused(lib.lib().abacus_mf_smooth_spectrum_dev(some.ptr, 8, C.c_double(L), C.c_double(np.nan)), 'R must')
        refused(lib.lib().abacus_mf_smooth_spectrum_dev(some.ptr, 8, C.c_double(0.0), C.c_double(1.0)), 'Lbox')
        refused(lib.lib().abacus_mf_check_memory(7, C.c_int64(0)), 'odd')
        refused(lib.lib().abacus_mf_check_memory(32766, C.c_int64(10**9)), 'largest mesh that fits')
        names = lib.profile_get()
        assert not any(k.startswith('mf_') or k.startswith('zcv_mult') for k in names), f'a kernel was launched: {names}'
    finally:
        lib.profile_enable(False)
        some.free()
