"""The wavelet scattering transform on the device (abacusutils_amd.analysis.wst, C ABI abacus_wst_*) against the NumPy statement
tests/wst_statement.py.  Needs an MI355X: run with `-m gpu`.

Moments: |sum - float64 NumPy sum| <= (N 2^-53 + 2^-48) sum of the terms: N roundings of the additions at most, and 16 ulp per pow, the
OpenCL full-profile limit for the double pow that OCML keeps.  Shapes: n = 5 (odd, smaller than a workgroup's row), 16 (a dense mesh
with 16-byte loads), 33 (odd, scalar loads on the dense mesh and 16-byte loads with a scalar tail on the padded one), 70 (4900 rows
dealt to 2048 workgroups: a workgroup sums several rows).  The padded copies carry +1e30 in every pad float: a read of the padding
would be seen in every sum.

Fields: max |U_dev - U_64| / max |U_64| <= 4 e_ref (the rule of tests/test_shear_gpu.py), e_ref the statement's own float32 noise: its
float32 / complex64 evaluation against its float64 one, computed here.  Shapes: n = 8 (smaller than any tile: one float4 of modes and
two of cells per row), 16, 30 (2 * 3 * 5: the mixed-radix transform; its pitch 32 leaves no pad mode), 48.

Measured on an MI355X (the maxima over the cases): see profiles/wst/README.md."""
import ctypes as C
import functools

import numpy as np
import pytest
import wst_statement as st

pytestmark = pytest.mark.gpu

LBOX = 1000.0
PAD = np.float32(1e30)
SIGMA0 = 0.8
QS = (0.5, 0.8, 1.0, 2.0, 3.0)


def _lib():
    from abacusutils_amd import _lib
    return _lib


def _wst():
    from abacusutils_amd.analysis import wst
    return wst


def _pitch(n):
    return (n + 2 + 31) // 32 * 32


def _e_ref(f32, f64):
    e = np.abs(f32.astype(np.float64) - f64).max() / np.abs(f64).max()
    assert 1e-8 < e < 1e-5, f'e_ref {e:.3g} outside (1e-8, 1e-5): the statement is broken'
    return e


# ------------------------------------------------------------------------------------------------- 1. moments
@pytest.mark.parametrize('n', (5, 16, 33, 70))
def test_moments(n):
    lib, wst = _lib(), _wst()
    rng = np.random.default_rng(400 + n)
    mesh = (rng.standard_normal((n, n, n)) * 3.0 + 0.75).astype(np.float32)
    mesh[rng.random((n, n, n)) < 0.05] = 0.0
    mesh[0, 0, 0], mesh[-1, -1, -1] = 0.0, -2.5
    assert (mesh < 0).any() and (mesh == 0).any() and (mesh > 0).any()
    q = np.array(QS)
    terms = np.abs(mesh.astype(np.float64))[None] ** q[:, None, None, None]
    want = terms.reshape(len(q), -1).sum(axis=1)
    bound = (float(n) ** 3 * 2.0**-53 + 2.0**-48) * want
    full = np.full((n, n, _pitch(n)), PAD, dtype=np.float32)
    full[:, :, :n] = mesh
    dense, padded = lib.DeviceArray(mesh), lib.DeviceArray(full)
    try:
        sums = []
        for dev, pitch in ((dense, n), (padded, _pitch(n)), (dense, n)):
            s = np.full(len(q), np.nan)
            lib.check(wst._lib_wst().abacus_wst_moments_dev(dev.ptr, n, pitch, lib.ptr(q), len(q), lib.ptr(s)))
            print(f'n={n} pitch={pitch}: |sum - want| / bound = {np.abs(s - want) / bound}')
            assert (np.abs(s - want) <= bound).all()
            sums.append(s)
        assert sums[0].tobytes() == sums[2].tobytes(), 'two calls differ'
        assert np.array_equal(dense.get(), mesh), 'the mesh was modified'
        assert np.array_equal(padded.get(), full), 'the padded mesh was modified'
        means = wst.wst_moments(dense, q)
        assert np.array_equal(means, sums[0] / float(n) ** 3) and np.array_equal(means, wst.wst_moments(mesh, q))
        one = wst.wst_moments(mesh, 2.0)                          # one exponent alone: the same sum as among five
        assert one.shape == (1,) and one[0] == means[3]
    finally:
        dense.free()
        padded.free()


# ------------------------------------------------------------------------------------------------- 2. modulus fields
@functools.lru_cache(maxsize=None)
def _normal(n):
    m = (1.0 + 0.5 * np.random.default_rng(500 + n).standard_normal((n, n, n))).astype(np.float32)
    m.setflags(write=False)
    return m


def _statement_modulus(mesh, sigma, ell, dtype):
    return st.modulus(st.spectrum(mesh, dtype), mesh.shape[0], sigma, ell, dtype)


@pytest.mark.parametrize('n', (8, 16, 30, 48))
def test_modulus_against_the_statement(n):
    wst = _wst()
    mesh = _normal(n)
    before = mesh.copy()
    sigmas = [SIGMA0 * 2.0**j for j in range(8) if SIGMA0 * 2.0**j <= n / 6.0]
    assert sigmas
    worst = 0.0
    for ell in range(5):
        first = None
        for j, sigma in enumerate(sigmas):
            u64, u32 = _statement_modulus(mesh, sigma, ell, np.float64), _statement_modulus(mesh, sigma, ell, np.float32)
            e_ref = _e_ref(u32, u64)
            got = wst.wst_modulus(mesh, sigma, ell)
            assert got.shape == (n, n, n) and got.dtype == np.float32 and (got >= 0).all()
            err = np.abs(got - u64).max() / u64.max()
            print(f'U1 n={n} l={ell} j={j}: err {err:.3g} = {err / e_ref:.2f} e_ref (e_ref {e_ref:.3g})')
            worst = max(worst, err / e_ref)
            assert err <= 4 * e_ref
            if j == 0:
                first = got
        # second order: scale j = 1 on the device's own U1[0, l] - the statement starts from the same mesh, only the new step is judged
        sigma = SIGMA0 * 2.0
        u64, u32 = _statement_modulus(first, sigma, ell, np.float64), _statement_modulus(first, sigma, ell, np.float32)
        e_ref = _e_ref(u32, u64)
        got = wst.wst_modulus(first, sigma, ell)
        err = np.abs(got - u64).max() / u64.max()
        print(f'U2 n={n} l={ell}: err {err:.3g} = {err / e_ref:.2f} e_ref (e_ref {e_ref:.3g})')
        worst = max(worst, err / e_ref)
        assert err <= 4 * e_ref
    print(f'n={n}: worst err / e_ref = {worst:.2f}')
    assert np.array_equal(mesh, before)
    # a spectrum handed over as one gives the field of its mesh; a resident mesh the bits of a host mesh
    lib = _lib()
    dev = lib.DeviceArray(mesh)
    try:
        again = wst.wst_modulus(dev, sigmas[0], 3)
        assert np.array_equal(dev.get(), mesh)
    finally:
        dev.free()
    assert np.array_equal(again, wst.wst_modulus(mesh, sigmas[0], 3))
    spec = st.spectrum(mesh, np.float64).astype(np.complex64)
    u64 = st.modulus(spec, n, sigmas[0], 3)
    e_ref = _e_ref(st.modulus(spec, n, sigmas[0], 3, np.float32), u64)
    assert np.abs(wst.wst_modulus(spec, sigmas[0], 3) - u64).max() / u64.max() <= 4 * e_ref


# ------------------------------------------------------------------------------------------------- 3. known answers
@pytest.mark.parametrize('n', (16, 30))
def test_constant_field_and_checkerboard(n):
    """a constant c is the mode k = 0 alone and (-1)^(x + y + z) the mode (n/2, n/2, n/2) alone: every multiplier of l > 0 is exactly
    zero on both.  l = 0 keeps the constant: every cell within the roundings of a transform that adds zeros to it, one per stage of
    at most 3 log2(n) + 2 stages; the second order passes through two more transforms and the 1 / N product."""
    wst = _wst()
    c = -0.7
    q = np.array(QS)
    const = np.zeros((n, n, n // 2 + 1), dtype=np.complex64)
    const[0, 0, 0] = c
    board = const.copy()
    board[n // 2, n // 2, n // 2] = 0.25
    eps = (3 * np.log2(n) + 2) * 2.0**-24
    a = abs(float(np.float32(c)))
    for ell in range(1, 5):
        for sigma in (SIGMA0, 2 * SIGMA0):
            for spec in (const, board):
                U = wst.wst_modulus(spec, sigma, ell)
                assert not U.any(), (ell, sigma)
    for eps_k, order in ((eps, 1), (3 * eps + 2.0**-24, 2)):
        U = wst.wst_modulus(const, SIGMA0, 0)
        if order == 2:
            U = wst.wst_modulus(U, 2 * SIGMA0, 0)
        assert np.abs(U - a).max() <= eps_k * a, order
        got = wst.wst_moments(U, q)
        want = a**q
        field = np.maximum((1 + eps_k) ** q - 1, 1 - (1 - eps_k) ** q) * want
        moment = (float(n) ** 3 * 2.0**-53 + 2.0**-48) * want
        print(f'constant n={n} order {order}: |S - |c|^q| = {np.abs(got - want)}, bound {field + moment}')
        assert (np.abs(got - want) <= field + moment).all()


def test_plane_wave():
    """<U1^2> = A^2 g^2 / 2 (1 + A^2 g^2 / 2 for l = 0) for four wave vectors of one length"""
    wst = _wst()
    n, sigma, A, phi = 16, 1.6, 0.3, 0.7
    i = np.arange(n)
    X, Y, Z = i[:, None, None], i[None, :, None], i[None, None, :]
    for p in ((3, 0, 0), (0, 0, 3), (2, 2, 1), (1, 2, 2)):
        rho = (1.0 + A * np.cos(2.0 * np.pi * (p[0] * X + p[1] * Y + p[2] * Z) / n + phi)).astype(np.float32)
        for ell in range(5):
            g = float(np.float32(st.profile(n, sigma, ell, 9)))
            want = A * A * g * g / 2.0 + (1.0 if ell == 0 else 0.0)
            u64 = _statement_modulus(rho, sigma, ell, np.float64)
            e_ref = _e_ref(_statement_modulus(rho, sigma, ell, np.float32), u64)
            U = wst.wst_modulus(rho, sigma, ell)
            got = wst.wst_moments(U, 2.0)[0]
            print(f'plane wave p={p} l={ell}: <U^2> off by {abs(got - want):.3g}, bound {4 * e_ref * u64.max() ** 2:.3g}')
            assert abs(got - want) <= 4 * e_ref * u64.max() ** 2
            if ell:
                # the driver on the same mesh: it sets the mode k = 0, which l > 0 never sees - the same cells, the same sums
                r = wst.wst_mesh(rho, J=1, L=4, q=(2.0,), sigma0=sigma, second_order=False)
                assert r['S1'][0, ell, 0] == got


# ------------------------------------------------------------------------------------------------- 4. the chain
@functools.lru_cache(maxsize=None)
def _points():
    p = st.clustered_points(20000, LBOX, 17)
    p.setflags(write=False)
    return p


def _check_against_statement(label, r, n, J, L, q, contrast):
    spec = r['spectrum']
    assert spec.shape == (n, n, n // 2 + 1) and spec.dtype == np.complex64
    s64 = st.coefficients(spec, n, J, L, q, SIGMA0, contrast, details=True)
    s32 = st.coefficients(spec, n, J, L, q, SIGMA0, contrast, dtype=np.float32, details=True)
    worst = 0.0
    for key, f64 in s64['fields'].items():
        e_ref, umax = _e_ref(s32['fields'][key], f64), np.abs(f64).max()
        if key[0] == 0:
            got, want = r['S0'], s64['S0']
        elif key[0] == 1:
            got, want = r['S1'][key[1], key[2]], s64['S1'][key[1], key[2]]
        else:
            got, want = r['S2'][key[1], key[2], key[3]], s64['S2'][key[1], key[2], key[3]]
        for k, e in enumerate(q):
            bound = 4 * e * e_ref * umax**e if e >= 1 else (4 * e_ref * umax) ** e
            worst = max(worst, abs(got[k] - want[k]) / bound)
            assert abs(got[k] - want[k]) <= bound, (label, key, e, got[k], want[k], bound)
    print(f'{label} n={n}: worst |S_dev - S_64| / bound = {worst:.3g} over {len(s64["fields"])} fields')


@pytest.mark.parametrize('n', (32, 48))
def test_calc_wst_chain(n):
    wst, lib = _wst(), _lib()
    J, L, q = 3, 4, (0.8, 2.0)
    pos = _points()
    before = pos.copy()
    w = np.random.default_rng(5).uniform(0.5, 1.5, len(pos)).astype(np.float32)
    cols = [lib.DeviceArray(np.ascontiguousarray(pos[:, a])) for a in range(3)]
    kw = dict(J=J, L=L, q=q, sigma0=SIGMA0, nmesh=n, return_spectrum=True)
    try:
        runs = dict(host=wst.calc_wst(pos, LBOX, **kw), columns=wst.calc_wst(cols, LBOX, **kw), weighted=wst.calc_wst(pos, LBOX, w=w, **kw),
                    plain=wst.calc_wst(pos.astype(np.float32), LBOX, paste='CIC', compensated=False, interlaced=False, contrast=True, **kw))
        for a, col in enumerate(cols):
            assert np.array_equal(col.get(), before[:, a])
    finally:
        for c in cols:
            c.free()
    assert np.array_equal(pos, before)
    j1, j2 = np.meshgrid(np.arange(J), np.arange(J), indexing='ij')
    for label, r in runs.items():
        assert r['S0'].shape == (2,) and r['S1'].shape == (J, L + 1, 2) and r['S2'].shape == (J, J, L + 1, 2) and r['n'] == n
        assert np.array_equal(r['sigmas'], SIGMA0 * 2.0 ** np.arange(J)) and np.array_equal(r['q'], q)
        assert np.isfinite(r['S0']).all() and np.isfinite(r['S1']).all()
        assert np.array_equal(np.isnan(r['S2']), np.broadcast_to((j2 <= j1)[:, :, None, None], r['S2'].shape))
        assert (r['S1'] > 0).all()
        assert wst.wst_flatten(r).shape == (2 * (1 + J * (L + 1) + J * (J - 1) // 2 * (L + 1)),)
    for k in ('S0', 'S1', 'S2', 'spectrum'):
        assert runs['host'][k].tobytes() == runs['columns'][k].tobytes(), k
    assert not np.array_equal(runs['host']['S1'], runs['weighted']['S1'])
    for label in ('host', 'weighted', 'plain'):
        _check_against_statement(label, runs[label], n, J, L, q, contrast=label == 'plain')
    first = wst.calc_wst(pos, LBOX, J=J, L=L, q=q, sigma0=SIGMA0, nmesh=n, second_order=False)
    assert 'spectrum' not in first and np.isnan(first['S2']).all()
    assert first['S0'].tobytes() == runs['host']['S0'].tobytes() and first['S1'].tobytes() == runs['host']['S1'].tobytes()
    assert wst.wst_flatten(first).shape == (2 * (1 + J * (L + 1)),)


# ------------------------------------------------------------------------------------------------- 5. AbacusHOD.compute_wst
class _Mock(dict):
    """a mock dictionary whose columns are also resident in HBM, as GRAND_HOD.MockDict.device_xyz hands them out"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.dev = {}

    def device_xyz(self, tracer):
        if tracer not in self.dev:
            self.dev[tracer] = [_lib().DeviceArray(np.ascontiguousarray(self[tracer][c], dtype=np.float64)) for c in 'xyz']
        return self.dev[tracer]


def test_abacus_hod_compute_wst():
    from abacusutils_amd.hod.abacus_hod import AbacusHOD
    n, kw = 32, dict(J=2, L=2, q=(0.8, 1.0))
    pos = _points()
    w = np.random.default_rng(4).uniform(0.5, 1.5, 5000).astype(np.float32)
    cols = dict(LRG=dict(zip('xyz', pos.T.copy())), ELG=dict(zip('xyz', pos[:5000].T.copy()), w=w))
    before = {tr: {c: v.copy() for c, v in d.items()} for tr, d in cols.items()}
    ball = AbacusHOD.__new__(AbacusHOD)
    ball.lbox = LBOX
    mock = _Mock(cols)
    try:
        dev = ball.compute_wst(mock, num_cells=n, **kw)
        assert set(mock.dev) == {'LRG', 'ELG'}                 # the columns came from HBM
        for tr in mock.dev:
            for c, col in zip('xyz', mock.dev[tr]):
                assert np.array_equal(col.get(), before[tr][c])
    finally:
        for d in mock.dev.values():
            for c in d:
                c.free()
    host = ball.compute_wst(cols, num_cells=n, **kw)
    for tr in cols:
        for c in before[tr]:
            assert np.array_equal(cols[tr][c], before[tr][c])
    assert set(dev) == set(host) == {'LRG', 'ELG'}
    direct = _wst().calc_wst(pos, LBOX, nmesh=n, **kw)
    for k in ('S0', 'S1', 'S2'):
        for tr in cols:
            assert dev[tr][k].tobytes() == host[tr][k].tobytes(), (tr, k)
        assert dev['LRG'][k].tobytes() == direct[k].tobytes(), k
    assert not np.array_equal(dev['LRG']['S1'], dev['ELG']['S1'])


# ------------------------------------------------------------------------------------------------- 6. errors
def test_errors_come_before_any_launch():
    lib, wst = _lib(), _wst()
    L = wst._lib_wst()
    some = lib.DeviceArray(nbytes=1 << 16, dtype=np.uint8, shape=(1 << 16,))         # never read or written: every call below is refused
    a, b, c = (C.c_void_p(some.ptr.value + k * 16384) for k in range(3))             # three meshes of 8 * 8 * 32 floats = 8192 bytes
    lib.profile_reset()
    lib.profile_enable(True)
    try:
        def refused(rc, entry, match):
            assert rc != 0
            msg = L.abacus_last_error().decode()
            assert msg.startswith(entry + ':') and match in msg, msg

        def modulus(spec=a, n=8, sigma=1.0, ell=1, work=b, out=c):
            return L.abacus_wst_modulus_dev(spec, n, sigma, ell, work, out)

        def moments(mesh=a, n=8, pitch=8, q=(0.8,), nq=None):
            e, s = np.ascontiguousarray(q, dtype=np.float64), np.zeros(16)
            return L.abacus_wst_moments_dev(mesh, n, pitch, lib.ptr(e), len(e) if nq is None else nq, lib.ptr(s))

        name = 'abacus_wst_modulus_dev'
        for n in (2, 0, -4, 32768):
            refused(modulus(n=n), name, 'out of range')
        refused(modulus(n=7), name, 'odd')
        refused(modulus(ell=5), name, 'ell')
        refused(modulus(ell=-1), name, 'ell')
        for s in (0.0, -1.0, np.nan, np.inf):
            refused(modulus(sigma=s), name, 'sigma')
        refused(modulus(spec=None), name, 'null')
        refused(modulus(work=None), name, 'null')
        refused(modulus(out=None), name, 'null')
        refused(modulus(work=a), name, 'aliased')
        refused(modulus(out=a), name, 'aliased')
        refused(modulus(out=b), name, 'aliased')
        refused(modulus(out=C.c_void_p(b.value + 4096)), name, 'aliased')        # overlapping, not equal
        refused(modulus(spec=C.c_void_p(a.value + 4)), name, 'aligned')
        name = 'abacus_wst_moments_dev'
        for n in (1, 32768):
            refused(moments(n=n, pitch=40000), name, 'out of range')
        refused(moments(pitch=7), name, 'pitch')
        refused(moments(nq=0), name, 'exponents')
        refused(moments(q=np.linspace(0.1, 0.9, 9)), name, 'exponents')
        for q in (0.0, -0.5, np.nan, 8.5):
            refused(moments(q=(0.8, q)), name, 'exponent 1')
        refused(moments(mesh=None), name, 'null')
        refused(L.abacus_wst_spectrum_dev(a, 6 + 1), 'abacus_wst_spectrum_dev', 'odd')
        refused(L.abacus_wst_spectrum_dev(None, 8), 'abacus_wst_spectrum_dev', 'null')
        e, s = np.array([0.8]), np.zeros(1024)
        coeff = lambda J=2, Lmax=2, sigma0=0.8, nq=1, n=8: L.abacus_wst_coefficients_dev(   # noqa: E731
            a, n, J, Lmax, sigma0, lib.ptr(e), nq, 0, 1, lib.ptr(s), lib.ptr(s), lib.ptr(s))
        name = 'abacus_wst_coefficients_dev'
        refused(coeff(J=0), name, 'J =')
        refused(coeff(J=9), name, 'J =')
        refused(coeff(Lmax=5), name, 'L =')
        refused(coeff(sigma0=0.0), name, 'sigma0')
        refused(coeff(nq=9), name, 'exponents')
        refused(coeff(n=10 + 1), name, 'odd')
        refused(L.abacus_wst_check_memory(7, 0), 'abacus_wst_check_memory', 'odd')
        refused(L.abacus_wst_check_memory(32766, 10**9), 'abacus_wst_check_memory', 'largest mesh that fits')
        names = lib.profile_get()
        assert not any(k.startswith('wst_') for k in names), f'a kernel was launched: {names}'
    finally:
        lib.profile_enable(False)
        some.free()
