"""Light-cone power spectrum multipoles: what can be checked without a device.  The NumPy statement tests/lc_power_statement.py is
the yardstick of the GPU tests; here its harmonics are held to the addition theorem, its end-point line of sight to the
plane-parallel limit, and `radial_nbar` and the argument checks of abacusutils_amd.analysis.lc_power are exercised."""
import lc_power_statement as st
import numpy as np
import pytest

from abacusutils_amd.analysis import lc_power
from abacusutils_amd.analysis.tpcf_corrfunc import LCRandoms


@pytest.mark.parametrize('ell', [2, 4])
def test_addition_theorem(ell):
    rng = np.random.default_rng(41 + ell)
    a, b = (v / np.linalg.norm(v, axis=1, keepdims=True) for v in (rng.normal(size=(1000, 3)), rng.normal(size=(1000, 3))))
    Sa, Sb = st.harmonics(ell, *a.T), st.harmonics(ell, *b.T)
    assert len(Sa) == 2 * ell + 1
    err = np.abs(sum(p * q for p, q in zip(Sa, Sb)) - st.legendre(ell, (a * b).sum(axis=1))).max()
    print(f'addition theorem l = {ell}: max error {err:.3g}')
    assert err < 1e-13


def _mirrored(cols, z0):
    """the points and their mirror images in the plane z = z0"""
    x, y, z = (np.asarray(c, dtype=np.float64) for c in cols)
    return np.concatenate((x, x)), np.concatenate((y, y)), np.concatenate((z, 2 * z0 - z))


def test_distant_observer_is_plane_parallel():
    """The same mesh seen by an observer 10^6 L down -z against the plane-parallel variant, to 1e-9 of the largest |P_l|.

    For a general mesh the two differ at FIRST order in L / d: with r^ = z^ + (x, y, 0) / d the harmonics with |m| = 1 enter as
    (1 / d) sum over pairs of x_mid F F' G(r - r'), G odd in the separation along z.  Measured on an octant shell without the mirror
    images below: 3.6e-7 of max |P_2| and 1.2e-6 of max |P_4| at d = 10^6 L (second assertion, which pins that order).  The first-order term changes sign under a reflection
    of the mesh in a plane z = const, so it vanishes for a mesh that is mirror-symmetric about the mid-plane of the box; what is left
    is second order, 10^-12.  Hence the mirrored sample: the limit is then reached to rounding, harmonics, k^ and all."""
    n, L, z0 = 16, 1600.0, 400.0
    plain = st.octant_shell(1500, 300.0, 700.0, seed=5, modulation=0.6), st.octant_shell(4000, 300.0, 700.0, seed=6)
    kedges = np.linspace(2 * np.pi / L, np.pi * n / L, 7)
    kw = dict(n=n, kedges=kedges, Lbox=L, paste='TSC')
    rel = {}
    wd0 = np.random.default_rng(7).uniform(0.5, 1.5, len(plain[0][0])).astype(np.float32)
    wr0 = np.random.default_rng(8).uniform(0.5, 1.5, len(plain[1][0])).astype(np.float32)
    for name, (data, rand), (wd, wr) in (('mirrored', [_mirrored(c, z0) for c in plain], (np.tile(wd0, 2), np.tile(wr0, 2))),
                                         ('plain', plain, (wd0, wr0))):          # a point and its image carry one weight
        data, rand = st.f32cols(data), st.f32cols(rand)
        nbar = np.full(len(rand[0]), 1e-4)
        pp = st.power_lc(data, wd, rand, wr, nbar, plane_parallel=True, **kw)['poles']
        far = st.power_lc(data, wd, rand, wr, nbar, los_shift=(0.0, 0.0, 1e6 * L), **kw)['poles']
        for q, ell in enumerate(st.POLES):
            rel[name, ell] = np.abs(far[q] - pp[q]).max() / np.abs(pp[q]).max()
            print(f'{name}, l = {ell}: distant observer against plane-parallel, max difference / max |P_l| = {rel[name, ell]:.3g}')
    for ell in st.POLES:
        assert rel['mirrored', ell] < 1e-9
    assert 1e-9 < rel['plain', 2] < 1e-5 and 1e-9 < rel['plain', 4] < 1e-5       # first order in L / d, not zero and not more


def test_radial_nbar_of_a_uniform_shell():
    """uniform points in an octant shell: every shell's density is N / V within the Poisson error of its count (seed fixed)"""
    x, y, z = st.octant_shell(200000, 200.0, 800.0, seed=3)
    edges = np.linspace(200.0, 800.0, 7)
    nbar = lc_power.radial_nbar(x, y, z, edges, fsky=0.125)
    assert nbar.shape == x.shape and nbar.dtype == np.float64
    want = len(x) / (0.125 * 4 * np.pi / 3 * (800.0**3 - 200.0**3))
    chi = np.sqrt(x * x + y * y + z * z)
    for lo, hi in zip(edges[:-1], edges[1:]):
        inside = (chi >= lo) & (chi < hi)
        values = np.unique(nbar[inside])
        assert len(values) == 1
        assert abs(values[0] / want - 1) < 4 / np.sqrt(inside.sum())
    np.testing.assert_allclose(nbar, st.radial_nbar((x, y, z), edges, 0.125), rtol=1e-14)
    # an observer elsewhere, and points outside the edges
    moved = lc_power.radial_nbar(x + 10.0, y - 5.0, z + 2.0, edges, 0.125, origin=(10.0, -5.0, 2.0))
    np.testing.assert_allclose(moved, nbar, rtol=1e-9)
    assert lc_power.radial_nbar(np.array([1.0]), np.array([0.0]), np.array([0.0]), edges, 0.125)[0] == 0.0


def _fake_randoms(nbar=None):
    r = LCRandoms.__new__(LCRandoms)       # no device: the checks under test come before any use of it
    r.nbar = nbar
    return r


def test_argument_checks_need_no_device():
    x = np.ones(4)
    with pytest.raises(TypeError, match='LCRandoms'):
        lc_power.calc_power_lc(x, x, x, object(), 4, nmesh=16, norm=1.0)
    with pytest.raises(TypeError, match='LCRandoms'):
        lc_power.fkp_field(x, x, x, None, 16)
    with pytest.raises(ValueError, match='nbar'):
        lc_power.calc_power_lc(x, x, x, _fake_randoms(), 4, nmesh=16)
    for bad in (0.0, np.nan, np.inf):
        with pytest.raises(ValueError, match='norm'):
            lc_power.calc_power_lc(x, x, x, _fake_randoms(), 4, nmesh=16, norm=bad)
    for n in (15, 0, -2, 32768):
        with pytest.raises(ValueError, match='nmesh'):
            lc_power.calc_power_lc(x, x, x, _fake_randoms(), 4, nmesh=n, norm=1.0)
        with pytest.raises(ValueError, match='nmesh'):
            lc_power.fkp_field(x, x, x, _fake_randoms(), n)
    for poles in ((1,), (0, 6), (), (2, 2)):
        with pytest.raises(ValueError, match='poles'):
            lc_power.calc_power_lc(x, x, x, _fake_randoms(), 4, nmesh=16, poles=poles, norm=1.0)
    with pytest.raises(ValueError, match='pasting'):
        lc_power.calc_power_lc(x, x, x, _fake_randoms(), 4, nmesh=16, paste='NGP', norm=1.0)
    with pytest.raises(ValueError, match='x2'):
        lc_power.calc_power_lc(x, x, x, _fake_randoms(), 4, nmesh=16, norm=1.0, w2=x)
    with pytest.raises(ValueError, match='edges'):
        lc_power.radial_nbar(x, x, x, [3.0, 2.0], 0.5)
    with pytest.raises(ValueError, match='fsky'):
        lc_power.radial_nbar(x, x, x, [1.0, 2.0], 0.0)
