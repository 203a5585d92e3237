"""The NumPy statement of the wavelet scattering transform (tests/wst_statement.py) held to facts it cannot fake: the addition theorem
of its harmonics, the closed form for a plane wave, the Nyquist rule against a full complex transform, known answers (constant field,
checkerboard), invariance under whole-cell shifts and axis permutations, a brute-force convolution in real space; and the argument
checks of the package, which run before the library loads.  No GPU needed."""
import itertools

import numpy as np
import pytest
import wst_statement as st

from abacusutils_amd.analysis import wst

Q = (0.5, 0.8, 1.0, 2.0)


def _spec(field):
    return np.fft.rfftn(np.asarray(field, dtype=np.float64)) / float(field.size)


def _table(n, sigma, ell, p):
    """the profile at the mode p as the multiplier holds it: the float64 expression rounded once to float32"""
    return float(np.float32(st.profile(n, sigma, ell, sum(c * c for c in p))))


def test_addition_theorem():
    rng = np.random.default_rng(1)
    a, b = rng.standard_normal((2, 200, 3))
    a /= np.linalg.norm(a, axis=1)[:, None]
    b /= np.linalg.norm(b, axis=1)[:, None]
    mu = (a * b).sum(axis=1)
    for ell in range(5):
        Sa, Sb = st.harmonics(ell, *a.T), st.harmonics(ell, *b.T)
        assert len(Sa) == 2 * ell + 1
        total = sum(x * y for x, y in zip(Sa, Sb))
        assert np.abs(total - st.legendre(ell, mu)).max() < 1e-14, ell
        assert np.abs(sum(x * x for x in Sa) - 1.0).max() < 1e-14, ell


def test_plane_wave():
    """rho = 1 + A cos(2 pi p . x / n + phi): <U1^2> = A^2 g(kappa_p)^2 / 2 for l = 1 .. 4 and 1 + A^2 g^2 / 2 for l = 0, whatever the
    direction of p - the sum over m of S_lm^2 is 1.  g is the table's value (float32 of the float64 profile)."""
    n, sigma, A, phi = 16, 1.6, 0.3, 0.7
    i = np.arange(n)
    X, Y, Z = i[:, None, None], i[None, :, None], i[None, None, :]
    worst = 0.0
    for p in ((3, 0, 0), (0, 0, 3), (2, 2, 1), (1, 2, 2)):
        rho = 1.0 + A * np.cos(2.0 * np.pi * (p[0] * X + p[1] * Y + p[2] * Z) / n + phi)
        spec = _spec(rho)
        for ell in range(5):
            U = st.modulus(spec, n, sigma, ell)
            g = _table(n, sigma, ell, p)
            want = A * A * g * g / 2.0 + (1.0 if ell == 0 else 0.0)
            worst = max(worst, abs(np.mean(U * U) - want))
            assert abs(np.mean(U * U) - want) < 1e-13, (p, ell)
    print(f'plane wave: worst |<U^2> - closed form| = {worst:.3g}')
    # the four wave vectors have |p|^2 = 9: one value of g per l
    assert len({sum(c * c for c in p) for p in ((3, 0, 0), (0, 0, 3), (2, 2, 1), (1, 2, 2))}) == 1


def test_nyquist_rule_makes_the_product_hermitian():
    n, sigma = 8, 1.1
    field = 1.0 + 0.5 * np.random.default_rng(2).standard_normal((n, n, n))
    half, full = _spec(field), np.fft.fftn(field) / float(field.size)
    for ell in (1, 2, 3):
        u2 = np.zeros((n, n, n))
        for mult in st.multipliers(n, sigma, ell, full=True):
            w = np.fft.ifftn(full * mult) * float(field.size)
            assert np.abs(w.imag).max() < 1e-14, ell
            u2 += w.real**2
        U = st.modulus(half, n, sigma, ell)
        assert np.abs(U - np.sqrt(u2)).max() < 1e-13 * U.max(), ell
        assert U.max() > 1e-3


def test_constant_field():
    n, c, J, L = 8, -0.7, 3, 4
    spec = np.zeros((n, n, n // 2 + 1), dtype=np.complex128)
    spec[0, 0, 0] = c
    r = st.coefficients(spec, n, J, L, Q, set_mean=False)
    want = np.abs(c) ** np.array(Q)
    np.testing.assert_allclose(r['S0'], want, rtol=1e-13)
    for j1 in range(J):
        np.testing.assert_allclose(r['S1'][j1, 0], want, rtol=1e-13)
        assert not r['S1'][j1, 1:].any()
        for j2 in range(J):
            if j2 > j1:
                np.testing.assert_allclose(r['S2'][j1, j2, 0], want, rtol=1e-13)
                assert not r['S2'][j1, j2, 1:].any()
            else:
                assert np.isnan(r['S2'][j1, j2]).all()


def test_checkerboard():
    """(-1)^(x + y + z) is the mode (n/2, n/2, n/2) alone, which every multiplier of l > 0 sets to zero"""
    n, J, L = 8, 2, 4
    i = np.arange(n)
    board = 1.0 - 2.0 * ((i[:, None, None] + i[None, :, None] + i[None, None, :]) % 2)
    spec = _spec(board)
    only = np.zeros_like(spec)
    only[n // 2, n // 2, n // 2] = 1.0
    assert np.abs(spec - only).max() < 1e-15
    for s in (spec, only):
        r = st.coefficients(s, n, J, L, Q, set_mean=False)
        assert not r['S1'][:, 1:].any() and not r['S2'][0, 1, 1:].any()
        assert (r['S1'][:, 0] >= 0).all()


def test_invariance_under_shifts_and_axis_permutations():
    n, J, L = 12, 2, 4
    field = 1.0 + 0.5 * np.random.default_rng(3).standard_normal((n, n, n))
    base = st.coefficients(_spec(field), n, J, L, Q)
    keep = ~np.isnan(base['S2'])
    variants = [np.roll(field, (3, -5, 1), axis=(0, 1, 2))] + [np.transpose(field, p) for p in itertools.permutations(range(3)) if p != (0, 1, 2)]
    for v in variants:
        r = st.coefficients(_spec(v), n, J, L, Q)
        assert np.abs(r['S1'] / base['S1'] - 1).max() < 1e-12
        assert np.abs(r['S2'][keep] / base['S2'][keep] - 1).max() < 1e-12
        assert np.array_equal(np.isnan(r['S2']), ~keep)


def test_brute_force_convolution():
    """U of one (sigma, l) from the wavelets in real space: psi_m = the inverse transform of the multiplier, convolved with rho by
    direct sums over the torus"""
    n, sigma, ell = 8, 1.3, 3
    N = n**3
    field = 1.0 + 0.5 * np.random.default_rng(4).standard_normal((n, n, n))
    idx = np.arange(n)
    d = (idx[:, None] - idx[None, :]) % n                          # d[x, y] = (x - y) mod n
    u2 = np.zeros((n, n, n))
    for mult in st.multipliers(n, sigma, ell, full=True):
        psi = np.fft.ifftn(mult)
        assert np.abs(psi.imag).max() < 1e-15
        psi = psi.real
        # conv[x1, x2, x3] = sum_y rho[y] psi[(x - y) mod n]
        kernel = psi[d[:, None, None, :, None, None], d[None, :, None, None, :, None], d[None, None, :, None, None, :]]
        conv = np.einsum('abcxyz,xyz->abc', kernel, field)
        u2 += conv**2
    U = st.modulus(_spec(field), n, sigma, ell)
    assert np.abs(U - np.sqrt(u2)).max() < 1e-12 * U.max()
    assert N == field.size and U.max() > 1e-3


def test_float32_evaluation_is_the_noise_scale():
    n = 16
    field = 1.0 + 0.5 * np.random.default_rng(5).standard_normal((n, n, n))
    spec = _spec(field).astype(np.complex64)
    for ell in range(5):
        u64, u32 = st.modulus(spec, n, 1.6, ell), st.modulus(spec, n, 1.6, ell, np.float32)
        assert u32.dtype == np.float32 and u64.dtype == np.float64
        e_ref = np.abs(u32 - u64).max() / u64.max()
        assert 1e-8 < e_ref < 1e-5, (ell, e_ref)


def test_flatten_order():
    J, L, nq = 3, 2, 2
    S1 = np.arange(J * (L + 1) * nq, dtype=np.float64).reshape(J, L + 1, nq) + 100
    S2 = np.full((J, J, L + 1, nq), np.nan)
    for j1 in range(J):
        for j2 in range(j1 + 1, J):
            S2[j1, j2] = 1000 * (j1 + 1) + 100 * j2 + np.arange((L + 1) * nq).reshape(L + 1, nq)
    r = dict(S0=np.array([1.0, 2.0]), S1=S1, S2=S2)
    v = wst.wst_flatten(r)
    assert v.shape == (nq * (1 + J * (L + 1) + J * (J - 1) // 2 * (L + 1)),) and np.isfinite(v).all()
    assert v[:2].tolist() == [1.0, 2.0] and np.array_equal(v[2:2 + S1.size], S1.ravel())
    assert np.array_equal(v[2 + S1.size:], np.concatenate([S2[0, 1].ravel(), S2[0, 2].ravel(), S2[1, 2].ravel()]))
    first = wst.wst_flatten(dict(r, S2=np.full_like(S2, np.nan)))
    assert first.shape == (nq * (1 + J * (L + 1)),)
    with pytest.raises(ValueError, match='not a WST result'):
        wst.wst_flatten(dict(r, S2=S2[:2]))


def test_argument_checks_need_no_device(monkeypatch):
    from abacusutils_amd import _lib

    def no_library():
        raise AssertionError('the library was touched')

    monkeypatch.setattr(_lib, 'lib', no_library)
    call = lambda **kw: wst.calc_wst(**{**dict(pos=np.zeros((10, 3)), Lbox=1000.0, J=2, L=2, nmesh=16), **kw})   # noqa: E731
    for J in (0, 9, 2.5):
        with pytest.raises(ValueError, match='J ='):
            call(J=J)
    for L in (5, -1):
        with pytest.raises(ValueError, match='L ='):
            call(L=L)
    for q in (0.0, -1.0, np.nan, np.inf, 8.5, (0.8, 0.0), [], np.linspace(0.1, 0.9, 9), [[0.5]]):
        with pytest.raises(ValueError, match='q must|exponent'):
            call(q=q)
    for n in (15, 2, 0, 32768):
        with pytest.raises(ValueError, match='nmesh'):
            call(nmesh=n)
    for s in (0.0, -0.8, np.nan, np.inf):
        with pytest.raises(ValueError, match='sigma0'):
            call(sigma0=s)
    with pytest.raises(ValueError, match='Lbox'):
        call(Lbox=0.0)
    with pytest.raises(ValueError, match='pasting'):
        call(paste='NGP')
    with pytest.raises(ValueError, match='shape'):
        call(pos=np.zeros((10, 2)))
    with pytest.raises(ValueError, match='weights'):
        call(w=np.ones(9))
    mesh = np.ones((8, 8, 8), dtype=np.float32)
    with pytest.raises(ValueError, match='cubic'):
        wst.wst_mesh(np.ones((8, 8, 6), dtype=np.float32))
    with pytest.raises(TypeError, match='float32'):
        wst.wst_mesh(mesh.astype(np.float64))
    with pytest.raises(ValueError, match='nmesh'):
        wst.wst_mesh(np.ones((7, 7, 7), dtype=np.float32))
    with pytest.raises(ValueError, match='not finite'):
        wst.wst_mesh(mesh * np.float32(np.nan))
    with pytest.raises(ValueError, match='ell'):
        wst.wst_modulus(mesh, 1.0, 5)
    with pytest.raises(ValueError, match='sigma'):
        wst.wst_modulus(mesh, 0.0, 1)
    with pytest.raises(ValueError, match='spectrum'):
        wst.wst_modulus(np.zeros((8, 8, 4), dtype=np.complex64), 1.0, 1)
    with pytest.raises(ValueError, match='exponent'):
        wst.wst_moments(mesh, (0.0,))
    assert wst._exponents(8.0).tolist() == [8.0] and len(wst._exponents(np.linspace(0.1, 0.8, 8))) == 8


def test_c_entries_refuse_bad_arguments_before_the_device():
    """the checks of the C ABI come before the device is touched: on a machine without one they are what answers"""
    import ctypes as C

    from abacusutils_amd import _lib
    lib = wst._lib_wst()
    a, b, c = (C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20))        # never dereferenced: every call is refused
    q, s = np.array([0.8]), np.zeros(8)

    def refused(rc, entry, match):
        msg = lib.abacus_last_error().decode()
        assert rc != 0 and msg.startswith(entry + ':') and match in msg, msg

    refused(lib.abacus_wst_modulus_dev(a, 7, 1.0, 1, b, c), 'abacus_wst_modulus_dev', 'odd')
    refused(lib.abacus_wst_modulus_dev(a, 2, 1.0, 1, b, c), 'abacus_wst_modulus_dev', 'out of range')
    refused(lib.abacus_wst_modulus_dev(a, 8, 1.0, 5, b, c), 'abacus_wst_modulus_dev', 'ell')
    refused(lib.abacus_wst_modulus_dev(a, 8, 0.0, 1, b, c), 'abacus_wst_modulus_dev', 'sigma')
    refused(lib.abacus_wst_modulus_dev(a, 8, 1.0, 1, a, c), 'abacus_wst_modulus_dev', 'aliased')
    refused(lib.abacus_wst_modulus_dev(a, 8, 1.0, 1, b, None), 'abacus_wst_modulus_dev', 'null')
    refused(lib.abacus_wst_spectrum_dev(a, 9), 'abacus_wst_spectrum_dev', 'odd')
    refused(lib.abacus_wst_moments_dev(a, 8, 4, _lib.ptr(q), 1, _lib.ptr(s)), 'abacus_wst_moments_dev', 'pitch')
    refused(lib.abacus_wst_moments_dev(a, 8, 8, _lib.ptr(q), 0, _lib.ptr(s)), 'abacus_wst_moments_dev', 'exponents')
    refused(lib.abacus_wst_coefficients_dev(a, 8, 9, 2, 0.8, _lib.ptr(q), 1, 0, 1, _lib.ptr(s), _lib.ptr(s), _lib.ptr(s)),
            'abacus_wst_coefficients_dev', 'J =')
    refused(lib.abacus_wst_check_memory(7, 0), 'abacus_wst_check_memory', 'odd')
