"""The NumPy statement of the bispectrum (tests/bispectrum_statement.py) pinned on the host: its FFT form against the brute-force triangle
sum, the aliasing rule, a known answer, the shot-noise arithmetic and the argument checks of the package.  No GPU."""
import bispectrum_statement as st
import numpy as np
import pytest

from abacusutils_amd.analysis import bispectrum as bk

N, L = 12, 1000.0
DK = 2.0 * np.pi / L
EDGES = np.array([0.5, 1.5, 2.5, 3.5, 4.0]) * DK


def _spectrum(n=N, seed=5):
    return st.density_spectrum(st.uniform_points(3000, L, seed), None, n, L, 'TSC', True)


def test_fft_form_is_the_brute_triangle_sum():
    """every mode below n / 3: the sums over the mesh close exactly the triangles.  Bound: the float64 transforms and the sums of up to
    4008 products of three values each carry a few 1e-16 of the largest term; 1e-14 of max |S| leaves an order of magnitude"""
    spec = _spectrum()
    s = st.bispectrum_from_spectrum(spec, N, L, EDGES)
    S, Nb = st.brute(spec, N, L, EDGES)
    err = np.abs(s['S'] - S).max() / np.abs(S).max()
    print(f'FFT against brute: S err {err:.3g} of max |S|, N err {np.abs(s["N"] - Nb).max():.3g}, closed ordered bins {(Nb > 0).sum()} of {Nb.size}')
    assert err < 1e-14
    assert np.array_equal(np.rint(s['N']).astype(np.int64), Nb) and np.abs(s['N'] - Nb).max() < 1e-9
    assert (Nb > 0).sum() == 61 and Nb.size == 64
    _, cnt = st.k_mean(N, L, EDGES)                               # sum_x I^2 / n^3 counts the modes of the full shell
    np.testing.assert_allclose(s['M'], cnt, rtol=0, atol=1e-9)
    ijl = s['ijl']
    assert (np.diff(ijl[:, 0] * 16 + ijl[:, 1] * 4 + ijl[:, 2]) > 0).all() and (ijl[:, 0] <= ijl[:, 1]).all() and (ijl[:, 1] <= ijl[:, 2]).all()
    np.testing.assert_allclose(s['B'], L**6 * S[tuple(ijl.T)] / Nb[tuple(ijl.T)], rtol=0, atol=1e-13 * np.abs(s['B']).max())


def test_modes_beyond_a_third_of_the_mesh_alias():
    """a top edge of 5.5 dk at n = 12: the mesh closes triangles modulo n that are none, N is off by thousands"""
    edges = np.array([0.5, 1.5, 2.5, 3.5, 5.5]) * DK
    spec = _spectrum()
    s = st.bispectrum_from_spectrum(spec, N, L, edges)
    S, Nb = st.brute(spec, N, L, edges)
    off = np.abs(np.rint(s['N']).astype(np.int64) - Nb).max()
    print(f'top edge 5.5 dk: N off by up to {off}, S by {np.abs(s["S"] - S).max() / np.abs(S).max():.3g} of max |S|')
    assert off > 1000
    assert np.abs(s['S'] - S).max() > 1e-3 * np.abs(S).max()
    with pytest.raises(ValueError, match='n / 3'):
        bk._check_args(N, L, edges)


def test_three_plane_waves_close_one_triangle():
    n = 16
    edges = np.array([0.5, 1.5, 2.5, 3.5, 4.5, 5.3]) * DK
    k = np.array([(2, 0, 0), (1, 3, 0), (-3, -3, 0)])          # |k| = 2, 3.16, 4.24: shells 1, 2, 3
    A, phi = np.array([0.3, 0.5, 0.7]), np.array([0.4, 1.1, -0.6])
    x = np.arange(n) / n
    X = np.stack(np.meshgrid(x, x, x, indexing='ij'), axis=-1)
    delta = sum(a * np.cos(2 * np.pi * (X @ kk) + p) for a, kk, p in zip(A, k, phi))
    spec = np.fft.rfftn(delta) / n**3
    s = st.bispectrum_from_spectrum(spec, n, L, edges)
    _, Nb = st.brute(None, n, L, edges)
    want = L**6 * (A.prod() / 4.0) * np.cos(phi.sum()) / Nb[1, 2, 3]
    hit = (s['ijl'] == (1, 2, 3)).all(axis=1)
    assert hit.sum() == 1
    np.testing.assert_allclose(s['B'][hit], want, rtol=1e-12)
    assert np.abs(s['B'][~hit]).max() < 1e-12 * abs(want)
    Pw = np.zeros(5)
    _, cnt = st.k_mean(n, L, edges)
    Pw[[1, 2, 3]] = L**3 * 2 * (A / 2) ** 2 / cnt[[1, 2, 3]]
    np.testing.assert_allclose(s['P'], Pw, rtol=1e-12, atol=1e-12 * Pw.max())


def test_shot_noise_and_reduced_bispectrum_by_hand():
    nbar = 1e-3                                                   # 1 / nbar = 1000, 1 / nbar^2 = 1e6
    P = np.array([3000.0, 2000.0, 1500.0])                        # shot-subtracted: 2000, 1000, 500
    ijl = np.array([(0, 0, 0), (0, 1, 2), (1, 2, 2)])
    B = np.array([1.9e7, 7.5e6, 4.25e6])
    for f in (bk.shot_noise_and_Q, st.shot_noise_and_Q):
        P_shot, B_shot, Q = f(B, P, ijl, nbar)
        assert P_shot == 1000.0
        np.testing.assert_allclose(B_shot, [6000e3 + 1e6, 3500e3 + 1e6, 2000e3 + 1e6], rtol=1e-15)
        np.testing.assert_allclose(Q, [(1.9e7 - 7e6) / 12e6, (7.5e6 - 4.5e6) / 3.5e6, (4.25e6 - 3e6) / 1.25e6], rtol=1e-15)
    with pytest.raises(ValueError, match='nbar'):
        bk.shot_noise_and_Q(B, P, ijl, 0.0)


def test_k_mean_of_the_package_is_the_statement():
    for n, edges in ((N, EDGES), (16, np.linspace(0.5, 16 / 3, 18) * DK)):
        got, cnt = bk.shell_k_mean(n, L, edges)
        want, wcnt = st.k_mean(n, L, edges)
        np.testing.assert_allclose(got, want, rtol=1e-15)
        assert np.array_equal(cnt, wcnt.astype(np.int64))


def test_argument_checks_need_no_device(monkeypatch):
    from abacusutils_amd import _lib

    def no_library():
        raise AssertionError('the library was touched')

    monkeypatch.setattr(_lib, 'lib', no_library)
    pos = np.zeros((10, 3))
    ok = np.linspace(0.5, 16 / 3, 6) * DK
    call = lambda **kw: bk.calc_bispectrum(**{**dict(pos=pos, Lbox=L, kedges=ok, nmesh=16), **kw})   # noqa: E731
    for n in (15, 0, -2, 32768):
        with pytest.raises(ValueError, match='nmesh'):
            call(nmesh=n)
    with pytest.raises(ValueError, match='shells'):
        call(kedges=ok[:1])
    with pytest.raises(ValueError, match='shells'):
        call(kedges=np.linspace(0.5, 16 / 3, 34) * DK)
    with pytest.raises(ValueError, match='increasing'):
        call(kedges=ok[::-1])
    with pytest.raises(ValueError, match='increasing'):
        call(kedges=np.array([0.0, 1.0, 2.0]) * DK)
    with pytest.raises(ValueError, match='increasing'):
        call(kedges=np.array([1.0, np.nan, 2.0]) * DK)
    with pytest.raises(ValueError, match='n / 3'):
        call(kedges=np.linspace(0.5, 5.5, 6) * DK)
    with pytest.raises(ValueError, match='Lbox'):
        call(Lbox=0.0)
    with pytest.raises(ValueError, match='pasting'):
        call(paste='NGP')
    with pytest.raises(ValueError, match='shape'):
        call(pos=np.zeros((10, 2)))
    with pytest.raises(ValueError, match='weights'):
        call(w=np.ones(9))
    with pytest.raises(ValueError, match='n / 3'):
        bk.bispectrum_from_spectrum(1234, 16, L, np.linspace(0.5, 5.5, 6) * DK)
    with pytest.raises(ValueError, match='n / 3'):
        bk.triangle_counts(16, L, np.linspace(0.5, 5.5, 6) * DK)
