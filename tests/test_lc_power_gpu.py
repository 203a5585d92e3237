"""Light-cone power spectrum multipoles on the device (abacusutils_amd.analysis.lc_power) against the NumPy statement
tests/lc_power_statement.py and against known answers.  Every comparison runs over ALL cells / modes / bins.  Needs an MI355X: run
with `-m gpu`.

Bounds: the rule at the head of tests/test_zcv_gpu.py, measured against the statement, never against the code under test.  `e_ref` is
the statement's own float32 noise (its float32 evaluation against its float64 one, relative to the largest value), taken per
quantity.  Meshes and spectra are held to 4 e_ref max(1, log2(n^3) / log2(16^3)) in max-norm relative to the largest value; binned
spectra to max(1e-5, 4 e_ref) of max(|want|, 0.1 max|want|) per multipole.  1e-8 < e_ref < 1e-4 is asserted, so that a broken statement
cannot loosen a bound.  Every ratio err / e_ref is printed.

Shapes: n = 16 (native power-of-two transform) and n = 24 (mixed radix, pitch != n); 3000 data points and 6000 randoms of an octant
shell, weighted.  Geometry 'outside': the observer outside the box, the box from the randoms (boxpad 1.5).  Geometry 'centre': the
observer inside the shell and exactly on a cell centre of a box of side 1200 (two randoms pin the extent so that the corner is
-300 on every axis: cell 4 of 16, cell 6 of 24), with points in the clouds around it: the |r| = 0 cell carries weight.

The draws.  With 3000 points on 16^3 cells the binned bound of 1e-5 lies at the float32 noise of the inputs themselves: the rounding of a
position in cells is white, the signal falls with the window of the cloud, and in the bin that ends at the Nyquist frequency the float32
STATEMENT is off by 6e-6 ('outside') and 9e-6 ('centre') of the bound's own measure for the median of 40 draws, by more than the bound
for some.  The seeds below are those of the 40 for which the float32 statement stays within 0.35 of the bound in every case of this
file (asserted in the first test): the bound then judges the device, not the draw.  The choice looks at the statement only."""
import functools
import math

import lc_power_statement as st
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = (16, 24)
GEOMS = ('outside', 'centre')
ORIGIN = {'outside': (-520.0, -410.0, -300.0), 'centre': (12.5, -7.25, 3.0)}
LBOX = {'outside': None, 'centre': 1200.0}
SEED = {'outside': 228, 'centre': 148}
BOXPAD = {'outside': 1.5, 'centre': 1.25}      # two cells of a 16^3 mesh are an eighth of the box: 1.25 leaves a tenth on the longest axis


def _stages(n):
    return max(1.0, math.log2(float(n) ** 3) / math.log2(16.0 ** 3))


@functools.lru_cache(maxsize=None)
def _case(geom):
    """(data1, w1, data2, w2, rand, wr, nbar) in the frame of the catalogue (float64 columns): observer-centred coordinates + ORIGIN"""
    rmin = 300.0 if geom == 'outside' else 30.0
    seed = SEED[geom]
    d1 = st.octant_shell(3000, rmin, 640.0, seed=seed, modulation=0.6)
    d2 = st.octant_shell(2000, rmin, 640.0, seed=seed + 1, modulation=0.4)
    r = st.octant_shell(6000, rmin, 640.0, seed=seed + 2)
    if geom == 'centre':
        r = tuple(np.concatenate((c, [-60.0, 660.0])) for c in r)
    o = np.asarray(ORIGIN[geom])
    if geom == 'outside':            # the shell stands away from the observer
        o = o + np.array([500.0, 400.0, 300.0])
    rng = np.random.default_rng(seed + 3)
    w1, w2, wr = (rng.uniform(0.5, 1.5, len(c[0])).astype(np.float32) for c in (d1, d2, r))
    to_frame = lambda cols: tuple(c + s for c, s in zip(cols, o))   # noqa: E731
    d1, d2, r = to_frame(d1), to_frame(d2), to_frame(r)
    chi = np.sqrt(sum((c - s) ** 2 for c, s in zip(r, ORIGIN[geom])))
    nbar = st.radial_nbar([c - s for c, s in zip(r, ORIGIN[geom])], np.linspace(0.0, chi.max() * 1.001, 9), 0.125)
    assert (nbar > 0).all()
    return d1, w1, d2, w2, r, wr, nbar


def _centred(geom, cols):
    return st.f32cols(cols, ORIGIN[geom])


def _kedges(n, L):
    return np.linspace(2 * np.pi / L, np.pi * n / L, 7)


@functools.lru_cache(maxsize=None)
def _statement(geom, n, paste='TSC', compensated=True, cross=False):
    """(float64 statement, float32 statement) of one case, computed once"""
    d1, w1, d2, w2, r, wr, nbar = _case(geom)
    rc = _centred(geom, r)
    L, _ = st.box(rc, BOXPAD[geom], LBOX[geom])
    kw = dict(n=n, kedges=_kedges(n, L), paste=paste, compensated=compensated, boxpad=BOXPAD[geom], Lbox=LBOX[geom])
    if cross:
        kw.update(data2=_centred(geom, d2), w2=w2)
    return tuple(st.power_lc(_centred(geom, d1), w1, rc, wr, nbar, dtype=t, **kw) for t in (np.float64, np.float32))


def _eref(label, x32, x64):
    e = st.e_ref(x32, x64)
    assert 1e-8 < e < 1e-4, f'{label}: e_ref {e:.3g} outside (1e-8, 1e-4): the statement is broken'
    return e


def _check(label, got, want, e_ref, n):
    factor = 4.0 * _stages(n)
    wide = np.complex128 if np.iscomplexobj(want) else np.float64
    assert got.shape == want.shape, (label, got.shape, want.shape)
    err = np.abs(got.astype(wide) - want.astype(wide)).max() / np.abs(want).max()
    print(f'{label}: err {err:.3g}, e_ref {e_ref:.3g}, err / e_ref {err / e_ref:.3g} (bound {factor:.3g})')
    assert err <= factor * e_ref, f'{label}: {err:.3g} > {factor:.3g} x {e_ref:.3g}'


def _check_binned(label, got, want, e_ref=0.0):
    """e_ref = 0: no statement stands behind `want` (another run of the device, a known answer): the floor of the rule alone"""
    rtol = max(1e-5, 4.0 * e_ref)
    got, want = np.asarray(got, dtype='f8'), np.asarray(want, dtype='f8')
    assert got.shape == want.shape and np.isfinite(want).all(), label
    err = (np.abs(got - want) / np.maximum(np.abs(want), 0.1 * np.abs(want).max())).max()
    print(f'{label}: err {err:.3g}, e_ref {e_ref:.3g}, err / e_ref {err / e_ref if e_ref else float("nan"):.3g}, rtol {rtol:.3g}')
    assert err <= rtol, f'{label}: {err:.3g} > {rtol:.3g}'


def _check_poles(label, got, s64, s32):
    for q, ell in enumerate(st.POLES):
        _check_binned(f'{label} P_{ell}', got['poles'][q], s64['poles'][q], _eref(f'{label} P_{ell}', s32['poles'][q], s64['poles'][q]))
    np.testing.assert_array_equal(got['N_mode'], s64['N_mode'])
    np.testing.assert_allclose(got['k_avg'], s64['k_avg'], rtol=1e-6)


def _randoms(geom, **kw):
    from abacusutils_amd.analysis.lc_power import LCRandoms
    _, _, _, _, r, wr, nbar = _case(geom)
    kw.setdefault('nbar', nbar)
    return LCRandoms(*r, w=wr, origin=ORIGIN[geom], **kw)


def _run(geom, n, R=None, cross=False, **kw):
    from abacusutils_amd.analysis.lc_power import calc_power_lc
    d1, w1, d2, w2, _, _, _ = _case(geom)
    R = _randoms(geom) if R is None else R
    L = st.box(_centred(geom, _case(geom)[4]), BOXPAD[geom], LBOX[geom])[0]
    if cross:
        kw.update(x2=d2[0], y2=d2[1], z2=d2[2], w2=w2)
    kw.setdefault('boxpad', BOXPAD[geom])
    kw.setdefault('Lbox', LBOX[geom])
    return calc_power_lc(*d1, R, _kedges(n, L), nmesh=n, w1=w1, origin=ORIGIN[geom], **kw)


# ------------------------------------------------------------------------------------------------- the statement's own footing
@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('geom', GEOMS)
def test_no_bin_is_empty_and_the_centre_cell_is_at_the_observer(geom, n):
    s64, _ = _statement(geom, n)
    assert (s64['N_mode'] > 0).all()
    for paste, compensated, cross in (('TSC', True, False), ('TSC', False, False), ('TSC', True, True), ('TSC', False, True), ('CIC', True, False)):
        t64, t32 = _statement(geom, n, paste, compensated, cross)
        for q, ell in enumerate(st.POLES):          # the float32 statement under the binned rule: see "The draws" above
            want = t64['poles'][q]
            own = (np.abs(t32['poles'][q] - want) / np.maximum(np.abs(want), 0.1 * np.abs(want).max())).max()
            assert own <= 0.35e-5, (paste, compensated, cross, ell, own)
    L, corner = s64['Lbox'], s64['corner']
    cell = -corner / (L / n)
    if geom == 'centre':
        assert L == 1200.0 and np.array_equal(corner, [-300.0] * 3) and np.array_equal(cell, np.rint(cell))
        i = int(cell[0])
        assert s64['F'][i, i, i] != 0                      # the |r| = 0 cell carries weight
    else:
        assert (corner > 0).all()                          # the observer is outside the box


# ------------------------------------------------------------------------------------------------- 1. the FKP mesh
@pytest.mark.parametrize('paste', ['TSC', 'CIC'])
@pytest.mark.parametrize('n', NS)
def test_fkp_mesh(n, paste):
    from abacusutils_amd.analysis.lc_power import fkp_field
    geom = 'outside'
    d1, w1 = _case(geom)[:2]
    s64, s32 = _statement(geom, n, paste)
    R = _randoms(geom)
    with fkp_field(*d1, R, n, w=w1, origin=ORIGIN[geom], paste=paste, boxpad=BOXPAD[geom]) as f:
        F = f.fetch()
        assert F.dtype == np.float32 and f.Lbox == s64['Lbox'] and np.array_equal(f.corner, s64['corner'])
        assert abs(f.alpha / s64['alpha'][0] - 1) < 1e-12
    _check(f'F {paste} n={n}', F, s64['F'], _eref('F', s32['F'], s64['F']), n)
    with pytest.raises(RuntimeError, match='freed'):
        f.fetch()


# ------------------------------------------------------------------------------------------------- 2. the multipole spectra
@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('geom', GEOMS)
def test_multipole_spectra(geom, n):
    from abacusutils_amd.analysis.lc_power import fkp_field
    d1, w1 = _case(geom)[:2]
    s64, s32 = _statement(geom, n)
    with fkp_field(*d1, _randoms(geom), n, w=w1, origin=ORIGIN[geom], boxpad=BOXPAD[geom], Lbox=LBOX[geom]) as f:
        for ell in st.POLES:
            got = f.spectrum(ell)
            assert got.dtype == np.complex64
            _check(f'F_{ell}(k) {geom} n={n}', got, s64['spectra'][ell], _eref(f'F_{ell}', s32['spectra'][ell], s64['spectra'][ell]), n)


# ------------------------------------------------------------------------------------------------- 3. the binned spectra
@pytest.mark.parametrize('cross', [False, True])
@pytest.mark.parametrize('compensated', [True, False])
@pytest.mark.parametrize('n', NS)
def test_power_multipoles(n, compensated, cross):
    geom = 'outside' if n == 16 else 'centre'
    s64, s32 = _statement(geom, n, 'TSC', compensated, cross)
    got = _run(geom, n, compensated=compensated, cross=cross)
    assert got['poles'].shape == (3, 6) and got['Lbox'] == s64['Lbox'] and np.array_equal(got['corner'], s64['corner'])
    _check_poles(f'{geom} n={n} comp={compensated} cross={cross}', got, s64, s32)
    np.testing.assert_allclose(got['k_mid'], 0.5 * (_kedges(n, got['Lbox'])[1:] + _kedges(n, got['Lbox'])[:-1]), rtol=1e-15)


def test_power_multipoles_cic_and_pole_subsets():
    geom, n = 'outside', 24
    s64, s32 = _statement(geom, n, 'CIC')
    got = _run(geom, n, paste='CIC')
    _check_poles(f'{geom} n={n} CIC', got, s64, s32)
    R = _randoms(geom)
    only4 = _run(geom, n, R=R, paste='CIC', poles=(4,))
    both = _run(geom, n, R=R, paste='CIC', poles=(2, 0))
    assert R.mesh_built == 1
    _check_binned('poles=(4,)', only4['poles'][0], got['poles'][2])
    for q, p in enumerate((1, 0)):
        _check_binned('poles=(2, 0)', both['poles'][q], got['poles'][p])


# ------------------------------------------------------------------------------------------------- 4. the distant observer
def _mirrored(cols, z0):
    x, y, z = cols
    return np.concatenate((x, x)), np.concatenate((y, y)), np.concatenate((z, 2 * z0 - z))


@pytest.mark.parametrize('compensated', [False, True])
@pytest.mark.parametrize('n', NS)
def test_distant_observer_gives_the_box_multipoles(n, compensated):
    """The observer 10^5 L down -z: P_l of calc_power_lc against the multipoles calc_pk_from_deltak gives for the fetched F_0 with the
    global line of sight z, after its conventions (a mean times L^3, the factor 2l + 1 inside).  This pins all 14 harmonics
    independently of the statement.

    The end-point estimator differs from the plane-parallel one at first order in L / d for a general mesh (measured in
    test_lc_power_host.py: 1.2e-6 of max |P_4| at d = 10^6 L, ten times that here - more than the bound).  The first-order term changes
    sign under a reflection of the mesh in a plane z = const, so the sample is made mirror-symmetric about the mid-plane of the box:
    every point comes with its image, one weight for both.  With L = 1600 the far origin is a multiple of 16, the float32 step of the
    observer-centred z column, and so is the mirror plane z0 = 400: rounding the columns keeps the symmetry.  What is left is second
    order, 10^-10."""
    from abacusutils_amd.analysis.lc_power import LCRandoms, calc_power_lc, fkp_field
    from abacusutils_amd.analysis.power_spectrum import calc_pk_from_deltak, get_W_compensated
    L, z0 = 1600.0, 400.0
    origin = (0.0, 0.0, -1e5 * L)
    d = _mirrored(st.octant_shell(1500, 300.0, 700.0, seed=21, modulation=0.6), z0)
    r = _mirrored(st.octant_shell(3000, 300.0, 700.0, seed=22), z0)
    rng = np.random.default_rng(23)
    wd, wr = (np.tile(rng.uniform(0.5, 1.5, len(c[0]) // 2).astype(np.float32), 2) for c in (d, r))
    R = LCRandoms(*r, w=wr, origin=origin, nbar=np.full(len(wr), 2e-5))
    ke = _kedges(n, L)
    got = calc_power_lc(*d, R, ke, nmesh=n, w1=wd, origin=origin, Lbox=L, compensated=compensated)
    with fkp_field(*d, R, n, w=wd, origin=origin, Lbox=L) as f:
        F0 = f.spectrum(0)
    assert R.mesh_built == 1
    if compensated:
        W = get_W_compensated(L, n, 'TSC', False).astype(np.float32)
        F0 = F0 * (1 / ((W[:, None, None] * W[None, :, None]) * W[None, None, :n // 2 + 1])).astype(np.float32)
    box = calc_pk_from_deltak(F0, L, ke, np.array([0.0, 1.0]), poles=np.array([0, 2, 4]))
    np.testing.assert_array_equal(got['N_mode'], box['N_mode_poles'])
    for q, ell in enumerate(st.POLES):
        want = box['binned_poles'][q].astype(np.float64) / L**3 / got['norm'] - (got['shotnoise'] / got['norm'] if ell == 0 else 0.0)
        _check_binned(f'distant observer n={n} comp={compensated} P_{ell}', got['poles'][q], want)


# ------------------------------------------------------------------------------------------------- 5. a cyclic permutation of the axes
@pytest.mark.parametrize('n', NS)
def test_cyclic_permutation_of_the_axes(n):
    """x -> y -> z -> x of data, randoms and origin: the z half plane and the k_z conventions must not show"""
    from abacusutils_amd.analysis.lc_power import LCRandoms, calc_power_lc
    geom = 'outside'
    d1, w1, _, _, r, wr, nbar = _case(geom)
    s64, s32 = _statement(geom, n)
    roll = lambda c: (c[2], c[0], c[1])   # noqa: E731
    R = LCRandoms(*roll(r), w=wr, origin=roll(ORIGIN[geom]), nbar=nbar)
    got = calc_power_lc(*roll(d1), R, _kedges(n, s64['Lbox']), nmesh=n, w1=w1, origin=roll(ORIGIN[geom]), boxpad=BOXPAD[geom])
    assert got['Lbox'] == s64['Lbox'] and np.array_equal(got['corner'], np.asarray(roll(s64['corner'])))
    _check_poles(f'cyclic n={n}', got, s64, s32)


# ------------------------------------------------------------------------------------------------- 6. normalisation and shot noise
@pytest.mark.parametrize('cross', [False, True])
def test_norm_shotnoise_alpha_and_resident_inputs(cross):
    from abacusutils_amd import _lib
    from abacusutils_amd.analysis.lc_power import LCRandoms, calc_power_lc
    geom, n = 'outside', 16
    d1, w1, d2, w2, r, wr, nbar = _case(geom)
    f8 = lambda w: w.astype(np.float64)   # noqa: E731
    a1, a2 = f8(w1).sum() / f8(wr).sum(), f8(w2).sum() / f8(wr).sum()
    if cross:
        norm, shot = a1 * a2 * (f8(wr) ** 2 * nbar).sum(), a1 * a2 * (f8(wr) ** 2).sum()
    else:
        norm, shot = a1 * a1 * (f8(wr) ** 2 * nbar).sum(), (f8(w1) ** 2).sum() + a1**2 * (f8(wr) ** 2).sum()
    host = _run(geom, n, cross=cross)
    # the same from columns, weights and nbar resident in HBM (float32 columns centred on the device)
    L = host['Lbox']
    o = ORIGIN[geom]
    dev = lambda cols: [_lib.DeviceArray(np.asarray(c, dtype=np.float32)) for c in cols]   # noqa: E731
    d1f, d2f, rf = ([np.asarray(c, dtype=np.float32) for c in cols] for cols in (d1, d2, r))
    keep = dev(d1f) + dev(d2f) + dev(rf) + [_lib.DeviceArray(w1), _lib.DeviceArray(wr), _lib.DeviceArray(nbar.astype(np.float32))]
    try:
        R = LCRandoms(*keep[6:9], w=keep[10], origin=o, nbar=keep[11])
        kw = dict(x2=keep[3], y2=keep[4], z2=keep[5], w2=w2) if cross else {}
        res = calc_power_lc(*keep[:3], R, _kedges(n, L), nmesh=n, w1=keep[9], origin=o, boxpad=BOXPAD[geom], **kw)
        Rh = LCRandoms(*rf, w=wr, origin=o, nbar=nbar.astype(np.float32))
        kwh = dict(x2=d2f[0], y2=d2f[1], z2=d2f[2], w2=w2) if cross else {}
        same = calc_power_lc(*d1f, Rh, _kedges(n, L), nmesh=n, w1=w1, origin=o, boxpad=BOXPAD[geom], **kwh)
    finally:
        for a in keep:
            a.free()
    for label, got, I in (('host float64', host, norm), ('device float32', res, None), ('host float32', same, None)):
        I = I if I is not None else (a1 * (a2 if cross else a1) * (f8(wr) ** 2 * f8(nbar.astype(np.float32))).sum())
        alpha = got['alpha'] if cross else (got['alpha'],)
        print(f"{label}: norm {got['norm'] / I - 1:.2e}, shotnoise {got['shotnoise'] / shot - 1:.2e}, alpha {alpha[0] / a1 - 1:.2e}")
        assert abs(got['norm'] / I - 1) < 1e-12 and abs(got['shotnoise'] / shot - 1) < 1e-12 and abs(alpha[0] / a1 - 1) < 1e-12
        assert not cross or abs(alpha[1] / a2 - 1) < 1e-12
    # float32 columns are centred in float32 on the host and on the device alike: the same points, the same spectra
    np.testing.assert_array_equal(res['N_mode'], same['N_mode'])
    for q, ell in enumerate(st.POLES):
        _check_binned(f'resident against host columns P_{ell}', res['poles'][q], same['poles'][q])
    # norm= overrides I
    over = _run(geom, n, R=_randoms(geom, nbar=None), cross=cross, norm=2.5)
    assert over['norm'] == 2.5
    for q, ell in enumerate(st.POLES):
        _check_binned(f'norm= P_{ell}', over['poles'][q] * 2.5, host['poles'][q] * host['norm'])


# ------------------------------------------------------------------------------------------------- 7. AbacusHOD.compute_power
class _Mock(dict):
    """a mock dictionary whose columns are also resident in HBM, as GRAND_HOD.MockDict.device_xyz hands them out"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.dev = {}

    def device_xyz(self, tracer):
        from abacusutils_amd import _lib
        if tracer not in self.dev:
            self.dev[tracer] = [_lib.DeviceArray(np.ascontiguousarray(self[tracer][c], dtype=np.float64)) for c in 'xyz']
        return self.dev[tracer]


def test_abacus_hod_compute_power_with_randoms():
    from abacusutils_amd.analysis.lc_power import calc_power_lc
    from abacusutils_amd.analysis.power_spectrum import calc_power
    from abacusutils_amd.hod.abacus_hod import AbacusHOD
    geom, n = 'outside', 24                                    # compute_power has no boxpad: 1.25 leaves 2.4 cells of 24
    d1, _, d2, w2, _, _, _ = _case(geom)
    ball = AbacusHOD.__new__(AbacusHOD)
    ball.halo_lc, ball.params, ball.lbox = True, {'origin': np.array(ORIGIN[geom])}, 2000.0
    mock = _Mock(LRG=dict(zip('xyz', d1)), ELG=dict(zip('xyz', d2), w=w2))
    R = _randoms(geom)
    L = st.box(_centred(geom, _case(geom)[4]))[0]
    k_max = np.pi * n / L
    try:
        got = ball.compute_power(mock, 6, 3, k_max, False, poles=[0, 2, 4], num_cells=n, compensated=True, randoms=R)
        again = ball.compute_power(mock, 6, 3, k_max, False, poles=[0, 2, 4], num_cells=n, compensated=True, randoms=R)
    finally:
        for cols in mock.dev.values():
            for c in cols:
                c.free()
    assert R.mesh_built == 1
    pairs = ('LRG_LRG', 'LRG_ELG', 'ELG_LRG', 'ELG_ELG')
    assert set(got) == {f'{p}_ell' for p in pairs} | {f'{p}_ell_modes' for p in pairs} | {'k_binc'}
    for key in got:                                            # (sums by atomics, means returned in float32: not bit for bit)
        if key.endswith('_ell'):
            for q in range(3):
                _check_binned(f'second evaluation {key}', again[key][q], got[key][q])
        else:
            np.testing.assert_array_equal(got[key], again[key])
    ke = np.linspace(0.0, k_max, 7)
    np.testing.assert_allclose(got['k_binc'], 0.5 * (ke[1:] + ke[:-1]), rtol=1e-15)
    for key, a, b in (('LRG_LRG', (d1, None), None), ('ELG_ELG', (d2, w2), None), ('LRG_ELG', (d1, None), (d2, w2))):
        kw = {} if b is None else dict(x2=b[0][0], y2=b[0][1], z2=b[0][2], w2=b[1])
        want = calc_power_lc(*a[0], R, 6, nmesh=n, w1=a[1], origin=ORIGIN[geom], **kw)
        for q, ell in enumerate(st.POLES):
            _check_binned(f'compute_power {key} P_{ell}', got[key + '_ell'][q], want['poles'][q])
        np.testing.assert_array_equal(got[key + '_ell_modes'], want['N_mode'])
    assert got['ELG_LRG_ell'] is got['LRG_ELG_ell']
    assert R.mesh_built == 1
    # without randoms= the box path is what it was: calc_power of the same columns in the periodic box
    host = {tr: {c: np.mod(v, 2000.0) for c, v in cols.items() if c in 'xyz'} for tr, cols in mock.items()}
    boxed = ball.compute_power(host, 6, 3, 0.05, False, poles=[0, 2], num_cells=n)
    pos = np.stack([host['LRG'][c] for c in 'xyz'], axis=1)
    want = calc_power(pos, 2000.0, 6, 3, 0.05, False, 'TSC', n, False, False, poles=[0, 2])
    np.testing.assert_allclose(boxed['LRG_LRG'], want['power'], rtol=1e-6)
    np.testing.assert_allclose(boxed['LRG_LRG_ell'], want['poles'], rtol=1e-5, atol=1e-5 * np.abs(want['poles']).max())
    assert 'mu_binc' in boxed and 'LRG_ELG_modes' in boxed
    ball.halo_lc = False
    with pytest.raises(ValueError, match='origin'):
        ball.compute_power(mock, 6, 3, k_max, False, poles=[0], num_cells=n, randoms=R)


# ------------------------------------------------------------------------------------------------- 8. errors
def test_errors():
    from abacusutils_amd.analysis.lc_power import calc_power_lc, fkp_field
    geom, n = 'outside', 16
    d1, w1 = _case(geom)[:2]
    R = _randoms(geom)
    r = _case(geom)[4]
    L = st.box(_centred(geom, r), BOXPAD[geom])[0]
    call = lambda **kw: calc_power_lc(*d1, R, 6, **{**dict(nmesh=n, w1=w1, origin=ORIGIN[geom], boxpad=BOXPAD[geom]), **kw})   # noqa: E731
    with pytest.raises(ValueError, match='two cells'):         # the randoms reach the faces of a box of their own extent
        call(boxpad=1.0)
    with pytest.raises(ValueError, match='two cells'):         # ... and lie outside a smaller one
        call(Lbox=0.5 * L)
    far = [c.copy() for c in d1]
    far[1][7] = r[1].max() + 0.1 * L                           # one data point within two cells of a face, the randoms inside
    with pytest.raises(ValueError, match='data: a point lies outside the box or closer than two cells'):
        calc_power_lc(*far, R, 6, nmesh=n, w1=w1, origin=ORIGIN[geom], boxpad=BOXPAD[geom])
    far[1][7] = np.nan
    with pytest.raises(ValueError, match='data'):
        fkp_field(*far, R, n, w=w1, origin=ORIGIN[geom], boxpad=BOXPAD[geom])
    with pytest.raises(ValueError, match='nbar'):
        calc_power_lc(*d1, _randoms(geom, nbar=None), 6, nmesh=n, w1=w1, origin=ORIGIN[geom], boxpad=BOXPAD[geom])
    with pytest.raises(ValueError, match='nmesh'):
        call(nmesh=15)
    with pytest.raises(ValueError, match='poles'):
        call(poles=(0, 1))
    with pytest.raises(ValueError, match='poles'):
        call(poles=(6,))
    with pytest.raises(ValueError, match='shape'):
        _randoms(geom, nbar=np.ones(5))
    with pytest.raises(ValueError, match='weights'):
        call(w1=w1[:-1])
    assert call()['poles'].shape == (3, 6)                     # and the object still works after every refusal


# ------------------------------------------------------------------------------------------------- 9. inputs are not modified
def test_inputs_are_not_modified():
    from abacusutils_amd import _lib
    from abacusutils_amd.analysis.lc_power import LCRandoms, calc_power_lc
    geom, n = 'centre', 24
    d1, w1, d2, w2, r, wr, nbar = (tuple(c.copy() for c in a) if isinstance(a, tuple) else a.copy() for a in _case(geom))
    before = [c.copy() for c in (*d1, w1, *d2, w2, *r, wr, nbar)]
    R = LCRandoms(*r, w=wr, origin=ORIGIN[geom], nbar=nbar)
    calc_power_lc(*d1, R, 6, nmesh=n, w1=w1, x2=d2[0], y2=d2[1], z2=d2[2], w2=w2, origin=ORIGIN[geom], Lbox=LBOX[geom])
    for a, b in zip((*d1, w1, *d2, w2, *r, wr, nbar), before):
        assert np.array_equal(a, b)
    dev = [_lib.DeviceArray(c) for c in d1] + [_lib.DeviceArray(w1)]
    try:
        calc_power_lc(*dev[:3], R, 6, nmesh=n, w1=dev[3], origin=ORIGIN[geom], Lbox=LBOX[geom])
        for a, b in zip(dev, before[:4]):
            assert np.array_equal(a.get(), b)
    finally:
        for a in dev:
            a.free()
    assert R.mesh_built == 1
