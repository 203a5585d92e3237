"""Zel'dovich control variates on the device (abacusutils_amd.hod.zcv) against the reference's own results (tests/golden/zcv_*.npz,
written by scripts/make_zcv_golden.py) and against known answers.  Every comparison runs over ALL cells / modes / bins.  Needs an
MI355X: run with `-m gpu`.

Bounds.  Each golden case carries `e_ref`, the reference's own float32 noise (its float32 result against a float64 evaluation of
the same formulas, relative to the largest value).  Meshes and spectra are held to 4 e_ref in max-norm relative to the reference's
largest value: two independent float32 evaluations, times two for a transform with another summation order.  Binned spectra are
held to max(1e-5, 4 e_ref) of max(|want|, 0.1 max|want|) element by element, with the pair's own e_ref (weakly correlated pairs
nearly cancel inside a bin, so the reference against itself is not within 1e-5 there).  At sizes beyond the goldens the bound grows
with the number of butterfly stages of the transform: times log2(n^3) / log2(16^3).  The measured ratio err / e_ref is printed."""
import math

import numpy as np
import pytest
from conftest import assert_spectrum_close, load_golden

from abacusutils_amd import synth

pytestmark = pytest.mark.gpu

FILTER = ['white16_half', 'white16_fifth', 'white24_half', 'white24_fifth']
FIELDS = ['filtered_white16_half', 'filtered_white24_half', 'white16_unfiltered', 'lognormal24', 'planewave16']
SPECTRAL = ['filter_field', 'n2_fft', 'sij_fft_00', 'sij_fft_01', 'sij_fft_02', 'sij_fft_11', 'sij_fft_12', 'sij_fft_22', 'add_ij',
            'dk_to_s2', 'dk_to_n2']
LATTICE = ['f0', 'f0.8']
ADVECT = ['TSC_TT', 'TSC_FF', 'CIC_TT', 'CIC_FF']
KEYNAMES = ['1cb', 'delta', 'delta2', 'tidal2', 'nabla2']
PAIRS = [f'{a}_{b}' for i, a in enumerate(KEYNAMES) for j, b in enumerate(KEYNAMES) if i >= j]
FIELD_KEYS = ('d', 'd2', 's2', 'n2')


@pytest.fixture(scope='module')
def gold():
    g = {}
    for name in ('zcv_cases', 'zcv_fields_cases', 'zcv_advect_cases'):
        g.update(load_golden(name))
    return g


HOD_PARAMS = dict(tracer_flags={'LRG': True, 'ELG': True, 'QSO': False}, want_ranks=False, want_AB=True, want_shear=False, want_rsd=True,
                  LRG_params=synth.LRG_PARAMS, ELG_params=synth.ELG_PARAMS, QSO_params=synth.QSO_PARAMS)
CLUSTERING = dict(clustering_type='xirppi', pimax=30, pi_bin_size=5,
                  bin_params=dict(logmin=-0.7728787904780005, logmax=1.4771212597864314, nbins=9))


def _names(g, key):
    return [str(s) for s in g[key]]


def _mode(name):
    return name[:3], name[4] == 'T', name[5] == 'T'


def _stages(n):
    return math.log2(float(n) ** 3) / math.log2(16.0 ** 3)


def _check(label, got, want, e_ref, factor=4.0):
    """max-norm relative to the reference's largest value, over all elements"""
    want = np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (label, got.shape, got.dtype)
    wide = np.complex128 if np.iscomplexobj(want) else np.float64
    err = np.abs(got.astype(wide) - want.astype(wide)).max() / np.abs(want).max()
    print(f'{label}: err {err:.3g}, e_ref {e_ref:.3g}, err / e_ref {err / e_ref:.3g} (bound {factor:.3g})')
    assert err <= factor * e_ref, f'{label}: {err:.3g} > {factor:.3g} x {e_ref:.3g}'
    return err / e_ref


def _check_binned(label, got, want, e_ref):
    rtol = max(1e-5, 4.0 * float(e_ref))
    want = np.asarray(want, dtype='f8')
    ok = ~np.isnan(want)
    if ok.any():
        floor = 0.1 * np.abs(want[ok]).max()
        err = (np.abs(np.asarray(got, dtype='f8')[ok] - want[ok]) / np.maximum(np.abs(want[ok]), floor)).max()
        print(f'{label}: err {err:.3g}, e_ref {float(e_ref):.3g}, err / e_ref {err / float(e_ref):.3g}, rtol {rtol:.3g}')
    assert_spectrum_close(got, want, rtol=rtol, err_msg=label)


def test_case_lists_match_the_golden(gold):
    assert _names(gold, 'filter_names') == FILTER and _names(gold, 'fields_names') == FIELDS
    assert _names(gold, 'spectral_names') == SPECTRAL and _names(gold, 'lattice_names') == LATTICE
    assert _names(gold, 'advect_names') == ADVECT and _names(gold, 'keynames') == KEYNAMES


# ------------------------------------------------------------------------------------------------- 1. - 3. ic_fields
@pytest.mark.parametrize('name', FILTER)
def test_gaussian_filter_matches_the_reference(gold, name):
    from abacusutils_amd.hod.zcv.ic_fields import gaussian_filter
    f = gold[f'filter/{name}/field']
    keep = f.copy()
    got = gaussian_filter(f, len(f), float(gold[f'filter/{name}/Lbox']), float(gold[f'filter/{name}/kcut']))
    assert np.array_equal(f, keep)
    _check(f'filter {name}', got, gold[f'filter/{name}/out'], float(gold[f'filter/{name}/e_ref']))


@pytest.mark.parametrize('name', FIELDS)
def test_get_fields_matches_the_reference(gold, name):
    """white16_unfiltered has full power on the Nyquist planes: it fails when the Hermitian-part rule is wrong or missing on
    either of the planes c = 0, c = n/2"""
    from abacusutils_amd.hod.zcv.ic_fields import get_fields
    delta = gold[f'fields/{name}/delta']
    keep = delta.copy()
    got = get_fields(delta, float(gold[f'fields/{name}/Lbox']), len(delta))
    assert np.array_equal(delta, keep) and len(got) == 4
    for key, g in zip(FIELD_KEYS, got):
        _check(f'fields {name} {key}', g, gold[f'fields/{name}/{key}'], float(gold[f'fields/{name}/e_ref_{key}']))


@pytest.mark.parametrize('name', SPECTRAL)
def test_piecewise_functions_match_the_reference(gold, name):
    from abacusutils_amd.hod.zcv import ic_fields as I
    dk, L, kcut = gold['spectral/delta_k'], float(gold['spectral/Lbox']), float(gold['spectral/kcut'])
    n = dk.shape[0]
    keep = dk.copy()
    if name == 'filter_field':
        work = dk.copy()
        got = I.filter_field(work, n, L, kcut)
        assert got is work                                    # in place, like the reference
    elif name == 'n2_fft':
        got = I.get_n2_fft(dk, n, L)
    elif name.startswith('sij_fft_'):
        got = I.get_sij_fft(int(name[-2]), int(name[-1]), dk, n, L)
    elif name == 'add_ij':
        got = gold['spectral/add_ij/final'].copy()
        add = gold['spectral/add_ij/add']
        assert I.add_ij(got, add, n, float(gold['spectral/add_ij/factor'])) is None
    elif name == 'dk_to_s2':
        got = I.get_dk_to_s2(dk, n, L)
    else:
        got = I.get_dk_to_n2(dk, n, L)
    assert np.array_equal(dk, keep)
    _check(f'spectral {name}', got, gold[f'spectral/{name}/out'], float(gold[f'spectral/{name}/e_ref']))


# ------------------------------------------------------------------------------------------------- 4. lattice
@pytest.mark.parametrize('name', LATTICE)
def test_lattice_positions_are_bit_equal(gold, name):
    from abacusutils_amd.hod.zcv.advect_fields import lattice_positions
    disp = [gold[f'lattice/disp_{a}'] for a in 'xyz']
    keep = [d.copy() for d in disp]
    want = gold[f'lattice/{name}/pos']
    got = lattice_positions(*disp, float(gold['lattice/Lbox']), float(gold['lattice/D']), float(gold[f'lattice/{name}/f_growth']))
    assert got.dtype == np.float32 and all(np.array_equal(a, b) for a, b in zip(disp, keep))
    np.testing.assert_array_equal(got, want)
    print(f'lattice {name}: {len(want)} sites bit-equal')
    dev = lattice_positions(*disp, float(gold['lattice/Lbox']), float(gold['lattice/D']), float(gold[f'lattice/{name}/f_growth']),
                            device_out=True)
    np.testing.assert_array_equal(dev.get(), want)
    dev.free()


# ------------------------------------------------------------------------------------------------- 5. - 6. advect, tracer
def _advect_golden(gold, mode, device=False):
    from abacusutils_amd._lib import DeviceArray
    from abacusutils_amd.hod.zcv.advect_fields import advect
    paste, comp, inter = _mode(mode)
    disp = [gold[f'advect/disp_{a}'] for a in 'xyz']
    fields = {k: gold[f'advect/field_{k}'] for k in KEYNAMES[1:]}
    if device:
        disp = [DeviceArray(a) for a in disp]
        fields = {k: DeviceArray(v) for k, v in fields.items()}
    adv = advect(disp, fields, float(gold['advect/Lbox']), 16, float(gold['advect/D']), float(gold['advect/f_growth']), paste, comp, inter)
    return adv, disp, fields


@pytest.mark.parametrize('mode', ADVECT)
def test_advected_spectra_and_pair_dictionary_match_the_reference(gold, mode):
    from abacusutils_amd.hod.zcv.advect_fields import field_power
    adv, disp, fields = _advect_golden(gold, mode)
    with adv:
        for key in KEYNAMES:
            _check(f'advect {mode} spectrum {key}', adv.spectrum(key), gold[f'advect/{mode}/spec_{key}'],
                   float(gold[f'advect/{mode}/e_ref_spec_{key}']))
        got = field_power(adv, gold['advect/k_bin_edges'], gold['advect/mu_bin_edges'], gold['advect/poles'], float(gold['advect/D']))
    want_keys = {'k_binc', 'mu_binc'} | {f'{q}_{p}' for p in PAIRS for q in ('P_kmu', 'N_kmu', 'P_ell', 'N_ell')}
    assert set(got) == want_keys
    ke, me = gold['advect/k_bin_edges'], gold['advect/mu_bin_edges']
    np.testing.assert_array_equal(got['k_binc'], (ke[1:] + ke[:-1]) * 0.5)
    np.testing.assert_array_equal(got['mu_binc'], (me[1:] + me[:-1]) * 0.5)
    for p in PAIRS:
        np.testing.assert_array_equal(got[f'N_kmu_{p}'], gold[f'advect/{mode}/N_kmu_{p}'])
        np.testing.assert_array_equal(got[f'N_ell_{p}'], gold[f'advect/{mode}/N_ell_{p}'])
        e = gold[f'advect/{mode}/e_ref_{p}']
        _check_binned(f'advect {mode} P_kmu_{p}', got[f'P_kmu_{p}'], gold[f'advect/{mode}/P_kmu_{p}'], e)
        _check_binned(f'advect {mode} P_ell_{p}', got[f'P_ell_{p}'], gold[f'advect/{mode}/P_ell_{p}'], e)


@pytest.mark.parametrize('mode', ADVECT)
def test_tracer_power_matches_the_reference_and_shifts_in_place(gold, mode):
    from abacusutils_amd.hod.zcv.tracer_power import tracer_power
    adv, _, _ = _advect_golden(gold, mode)
    pos = gold['tracer/pos'].copy()
    with adv:
        got = tracer_power(pos, adv, gold['advect/k_bin_edges'], gold['advect/mu_bin_edges'], gold['advect/poles'], float(gold['advect/D']))
    np.testing.assert_array_equal(pos, gold['tracer/pos_shifted'])     # the reference's in-place contract (:157-158)
    pairs = ['tr_tr'] + [f'{k}_tr' for k in KEYNAMES]
    # the reference's pk_tr_dict, written out from hod/zcv/tracer_power.py :88-90 (k_binc, mu_binc), :216-219 and :269-272
    assert set(got) == {'k_binc', 'mu_binc',
                        'P_kmu_tr_tr', 'N_kmu_tr_tr', 'P_ell_tr_tr', 'N_ell_tr_tr',
                        'P_kmu_1cb_tr', 'N_kmu_1cb_tr', 'P_ell_1cb_tr', 'N_ell_1cb_tr',
                        'P_kmu_delta_tr', 'N_kmu_delta_tr', 'P_ell_delta_tr', 'N_ell_delta_tr',
                        'P_kmu_delta2_tr', 'N_kmu_delta2_tr', 'P_ell_delta2_tr', 'N_ell_delta2_tr',
                        'P_kmu_tidal2_tr', 'N_kmu_tidal2_tr', 'P_ell_tidal2_tr', 'N_ell_tidal2_tr',
                        'P_kmu_nabla2_tr', 'N_kmu_nabla2_tr', 'P_ell_nabla2_tr', 'N_ell_nabla2_tr'}
    ke, me = gold['advect/k_bin_edges'], gold['advect/mu_bin_edges']
    np.testing.assert_array_equal(got['k_binc'], (ke[1:] + ke[:-1]) * 0.5)
    np.testing.assert_array_equal(got['mu_binc'], (me[1:] + me[:-1]) * 0.5)
    for p in pairs:
        np.testing.assert_array_equal(got[f'N_kmu_{p}'], gold[f'tracer/{mode}/N_kmu_{p}'])
        np.testing.assert_array_equal(got[f'N_ell_{p}'], gold[f'tracer/{mode}/N_ell_{p}'])
        e = gold[f'tracer/{mode}/e_ref_{p}']
        _check_binned(f'tracer {mode} P_kmu_{p}', got[f'P_kmu_{p}'], gold[f'tracer/{mode}/P_kmu_{p}'], e)
        _check_binned(f'tracer {mode} P_ell_{p}', got[f'P_ell_{p}'], gold[f'tracer/{mode}/P_ell_{p}'], e)


def _consume_like_run_zcv(power_tr_dict, power_ij_dict, want_rsd, keynames, poles):
    """the accesses the reference's tools_cv.read_power_dict (:446-497, the first thing run_zcv does with the two dictionaries) makes:
    every key it reads, every reshape it applies"""
    k = power_tr_dict['k_binc'].flatten()
    key, shape = ('P_ell', (len(poles), len(k))) if want_rsd else ('P_kmu', (len(k), 1))
    pk_tt = power_tr_dict[f'{key}_tr_tr'].reshape(shape)
    nmodes = power_tr_dict['N_ell_tr_tr' if want_rsd else 'N_kmu_tr_tr'].flatten()
    pk_zt = np.stack([power_tr_dict[f'{key}_{a}_tr'].reshape(shape) for a in keynames])
    pk_zz = np.stack([power_ij_dict[f'{key}_{a}_{b}'].reshape(shape) for i, a in enumerate(keynames) for j, b in enumerate(keynames) if i >= j])
    return k, pk_tt, pk_zz, pk_zt, nmodes


@pytest.mark.parametrize('want_rsd', [True, False])
def test_dictionaries_feed_the_references_run_zcv(gold, want_rsd):
    """both dictionaries go through the access pattern of the reference's read_power_dict: redshift space reads the multipoles
    (len(poles), len(k)); real space reads P_kmu of ONE mu bin as (len(k), 1)"""
    from abacusutils_amd.hod.zcv.advect_fields import field_power
    from abacusutils_amd.hod.zcv.tracer_power import tracer_power
    adv, _, _ = _advect_golden(gold, 'TSC_TT')
    ke, poles, D = gold['advect/k_bin_edges'], gold['advect/poles'], float(gold['advect/D'])
    me = gold['advect/mu_bin_edges'] if want_rsd else np.array([0.0, 1.0])
    with adv:
        ij = field_power(adv, ke, me, poles, D)
        tr = tracer_power(gold['tracer/pos'].copy(), adv, ke, me, poles, D)
    k, pk_tt, pk_zz, pk_zt, nmodes = _consume_like_run_zcv(tr, ij, want_rsd, KEYNAMES, poles)
    nk = len(ke) - 1
    shape = (len(poles), nk) if want_rsd else (nk, 1)
    assert k.shape == (nk,) and pk_tt.shape == shape and pk_zz.shape == (15,) + shape and pk_zt.shape == (5,) + shape and nmodes.shape == (nk,)
    np.testing.assert_array_equal(k, ij['k_binc'])
    np.testing.assert_array_equal(nmodes, gold['tracer/TSC_TT/N_ell_tr_tr'])
    if want_rsd:
        np.testing.assert_array_equal(pk_zt[1], tr['P_ell_delta_tr'])
        _check_binned('run_zcv access P_ell_tr_tr', pk_tt, gold['tracer/TSC_TT/P_ell_tr_tr'], gold['tracer/TSC_TT/e_ref_tr_tr'])
    else:
        # one mu bin: P_kmu is the monopole
        _check_binned('run_zcv access P_kmu_tr_tr', pk_tt[:, 0], gold['tracer/TSC_TT/P_ell_tr_tr'][0], gold['tracer/TSC_TT/e_ref_tr_tr'])


def test_lattice_positions_at_a_size_with_several_passes_per_row():
    """n = 264: more than 256 cells per row (a second trip through the kernel's lane loop) and many rows per workgroup; against
    NumPy float32 array arithmetic over the site indices, bit for bit.  rms displacement 2 cells, so many sites wrap."""
    from abacusutils_amd.hod.zcv.advect_fields import lattice_positions
    n, L, D, fg = 264, 750.0, 0.7, 0.35
    f4 = np.float32
    rng = np.random.default_rng(264)
    disp = [(rng.standard_normal((n, n, n), dtype=f4) * f4(2.0 / n / D)) for _ in range(3)]
    got = lattice_positions(*disp, L, D, fg)
    site = np.indices((n, n, n), dtype=np.int64).reshape(3, -1)
    wrapped = 0
    for axis in range(3):
        x = disp[axis].reshape(-1) * f4(D)
        if axis == 2:
            x = x * f4(1 + fg)
        x = (x + site[axis].astype(f4) / f4(n)) * f4(L)
        wrapped += int(((x < 0) | (x >= f4(L))).sum())
        np.testing.assert_array_equal(got[:, axis], np.remainder(x, f4(L)))
    print(f'lattice {n}^3: {3 * n ** 3} coordinates bit-equal, {wrapped} wrapped')
    assert wrapped > 1000


# ------------------------------------------------------------------------------------------------- known answers at size
@pytest.mark.parametrize('n', [256, 576])
def test_plane_wave_known_answers(gold, n):
    """delta = A cos(k.x) with an oblique integer wavevector gives n2 = -k^2 delta, d2 = delta^2 - A^2/2 and
    s2 = (2/3)(delta^2 - A^2/2) in every cell (float64 closed forms of the float32 input).  The wave is the golden's `planewave16`
    at the same wavelength IN CELLS, m = (1, 2, 3) n / 16: the float32 rounding of the input is white noise, which -k^2 amplifies
    by (k_Nyquist / k_wave)^2, so that ratio is kept at the value it has where e_pw was measured.
    Bound: 4 e_pw log2(n^3) / log2(16^3), e_pw the golden's e_ref of the same field (transform rounding grows with the stages)."""
    from abacusutils_amd.hod.zcv.ic_fields import get_fields
    A, m = float(gold['planewave/A']), gold['planewave/m'] * (n // 16)
    L = float(gold['fields/planewave16/Lbox'])
    x = np.arange(n) / n
    delta = (A * np.cos(2 * np.pi * (m[0] * x[:, None, None] + m[1] * x[None, :, None] + m[2] * x[None, None, :]))).astype(np.float32)
    got = dict(zip(FIELD_KEYS, get_fields(delta, L, n)))
    d64 = delta.astype(np.float64)
    k2 = float((m.astype(np.float64) ** 2).sum()) * (2 * np.pi / L) ** 2
    for key, want in (('n2', lambda: -k2 * d64), ('d2', lambda: d64 * d64 - 0.5 * A * A), ('s2', lambda: (2.0 / 3.0) * (d64 * d64 - 0.5 * A * A))):
        w = want()
        err = np.abs(got[key] - w).max() / np.abs(w).max()
        e_pw = float(gold[f'fields/planewave16/e_ref_{key}'])
        bound = 4.0 * e_pw * _stages(n)
        print(f'plane wave {n}^3 {key}: err {err:.3g}, e_pw {e_pw:.3g}, err / e_pw {err / e_pw:.3g}, bound {bound:.3g}')
        assert err <= bound, (key, err, bound)
        del w


def test_zero_displacement_known_answer(gold):
    """disp = 0, TSC, not compensated, not interlaced, n = Lbox = 128: every lattice position is an exact float32 integer, the cloud
    weights are exactly 1/8, 3/4, 1/8, and each field is rfftn(w) prod_axes(3/4 + 1/4 cos(2 pi a / n)) / n^3 - delta_{k,0}; the DC
    mode is mean(w) - 1.  Bound 4 e log2(128^3) / log2(16^3), e the golden e_ref of the (TSC, F, F) spectrum of that field."""
    from abacusutils_amd.hod.zcv.advect_fields import advect
    n = 128
    rng = np.random.default_rng(128)
    fields = {k: rng.standard_normal((n, n, n)).astype(np.float32) for k in KEYNAMES[1:]}
    zero = np.zeros((n, n, n), dtype=np.float32)
    a = np.arange(n)
    c = 0.75 + 0.25 * np.cos(2 * np.pi * a / n)
    window = c[:, None, None] * c[None, :, None] * c[None, None, :n // 2 + 1]
    with advect([zero, zero, zero], fields, float(n), n, 0.6, 0.0, 'TSC', False, False) as adv:
        for key in KEYNAMES:
            w = np.ones((n, n, n)) if key == '1cb' else fields[key].astype(np.float64)
            want = np.fft.rfftn(w) * window / float(n) ** 3
            want[0, 0, 0] -= 1.0
            got = adv.spectrum(key)
            e = float(gold[f'advect/TSC_FF/e_ref_spec_{key}'])
            bound = 4.0 * e * _stages(n)
            scale = max(np.abs(want).max(), 1e-300)
            err = np.abs(got - want).max() / scale
            dc = abs(complex(got[0, 0, 0]) - (w.mean() - 1.0)) / scale
            print(f'zero displacement {key}: err {err:.3g}, DC err {dc:.3g}, e {e:.3g}, err / e {err / e:.3g}, bound {bound:.3g}')
            if key == '1cb':      # a uniform lattice of unit weights: every mode is zero; the bound is taken of the unit density
                assert np.abs(got).max() <= bound
            else:
                assert err <= bound and dc <= bound


@pytest.mark.parametrize('mode', ADVECT)
def test_device_chain_equals_the_composition_of_public_functions(gold, mode):
    """lattice_positions -> host -> get_field_fft(pos, w = ...) x 5 -> calc_pk_from_deltak x 15 at 64^3.  A secondary check (both
    sides are this package; the right-hand side is pinned by the existing tests), the goldens are the primary one."""
    from abacusutils_amd.analysis.power_spectrum import calc_pk_from_deltak, get_field_fft, get_k_mu_edges, get_W_compensated
    from abacusutils_amd.hod.zcv import ic_fields as I
    from abacusutils_amd.hod.zcv.advect_fields import advect, field_power, lattice_positions
    paste, comp, inter = _mode(mode)
    n, L, D, fg = 64, 100.0, 0.7, 0.4
    kny = np.pi * n / L
    rng = np.random.default_rng(64)
    dens = I.gaussian_filter(rng.standard_normal((n, n, n)).astype(np.float32), n, L, 0.5 * kny)
    disp = [I.gaussian_filter((1.5 / n) * rng.standard_normal((n, n, n)).astype(np.float32), n, L, 0.3 * kny) * np.float32(8) for _ in range(3)]
    fields = dict(zip(KEYNAMES[1:], I.get_fields(dens, L, n)))       # (d, d2, s2, n2) = delta, delta2, tidal2, nabla2
    ke, me = get_k_mu_edges(L, kny, 12, 3, False)
    poles = [0, 2, 4]
    with advect(disp, fields, L, n, D, fg, paste, comp, inter) as adv:
        spec = {k: adv.spectrum(k) for k in KEYNAMES}
        got = field_power(adv, ke, me, poles, D)
    pos = lattice_positions(*disp, L, D, fg)
    W = get_W_compensated(L, n, paste, inter) if comp else None
    ref = {k: get_field_fft(pos.copy(), L, n, paste, None if k == '1cb' else fields[k].ravel(), W, comp, inter) for k in KEYNAMES}
    for k in KEYNAMES:
        e = float(gold[f'advect/{mode}/e_ref_spec_{k}'])
        _check(f'chain {mode} spectrum {k}', spec[k], ref[k], e, factor=4.0 * _stages(n))
    fD = {'1cb': 1.0, 'delta': D, 'delta2': D ** 2, 'tidal2': D ** 2, 'nabla2': D}
    for i, a in enumerate(KEYNAMES):
        for j, b in enumerate(KEYNAMES):
            if i < j:
                continue
            P = calc_pk_from_deltak(ref[a], L, ke, me, field2_fft=ref[b], poles=np.asarray(poles))
            np.testing.assert_array_equal(got[f'N_kmu_{a}_{b}'], P['N_mode'])
            np.testing.assert_array_equal(got[f'N_ell_{a}_{b}'], P['N_mode_poles'])
            if i == j:
                assert_spectrum_close(got[f'P_kmu_{a}_{b}'], P['power'] * (fD[a] * fD[b]), rtol=1e-5, err_msg=f'{mode} P_kmu {a}')
                assert_spectrum_close(got[f'P_ell_{a}_{b}'], P['binned_poles'] * (fD[a] * fD[b]), rtol=1e-5, err_msg=f'{mode} P_ell {a}')


# ------------------------------------------------------------------------------------------------- conventions
def test_device_arrays_in_give_device_arrays_out(gold):
    from abacusutils_amd._lib import DeviceArray
    from abacusutils_amd.hod.zcv import ic_fields as I
    from abacusutils_amd.hod.zcv.advect_fields import field_power
    from abacusutils_amd.hod.zcv.tracer_power import tracer_power
    name = 'lognormal24'
    delta = gold[f'fields/{name}/delta']
    L, n = float(gold[f'fields/{name}/Lbox']), len(delta)
    dd = DeviceArray(delta)
    host = I.get_fields(delta, L, n)
    dev = I.get_fields(dd, L, n)
    assert all(isinstance(a, DeviceArray) and a.dtype == np.float32 and a.shape == (n, n, n) for a in dev)
    for h, d in zip(host, dev):
        np.testing.assert_array_equal(d.get(), h)
    np.testing.assert_array_equal(dd.get(), delta)
    kcut = 0.5 * np.pi * n / L
    fd = I.gaussian_filter(dd, n, L, kcut)
    assert isinstance(fd, DeviceArray)
    np.testing.assert_array_equal(fd.get(), I.gaussian_filter(delta, n, L, kcut))
    np.testing.assert_array_equal(dd.get(), delta)
    dk = gold['spectral/delta_k']
    dkd = DeviceArray(dk)
    for f, args in ((I.get_n2_fft, ()), (I.get_dk_to_s2, ()), (I.get_dk_to_n2, ())):
        out = f(dkd, 16, L, *args)
        assert isinstance(out, DeviceArray)
        np.testing.assert_array_equal(out.get(), f(dk, 16, L, *args))
    out = I.get_sij_fft(0, 2, dkd, 16, L)
    np.testing.assert_array_equal(out.get(), I.get_sij_fft(0, 2, dk, 16, L))
    np.testing.assert_array_equal(dkd.get(), dk)
    # advect / tracer_power with everything resident
    mode = 'TSC_TT'
    ke, me, poles, D = gold['advect/k_bin_edges'], gold['advect/mu_bin_edges'], gold['advect/poles'], float(gold['advect/D'])
    adv_h, _, _ = _advect_golden(gold, mode)
    adv_d, disp_d, fields_d = _advect_golden(gold, mode, device=True)
    with adv_h, adv_d:
        for k in KEYNAMES:
            np.testing.assert_array_equal(adv_d.spectrum(k), adv_h.spectrum(k))
        for a, key in zip(disp_d, 'xyz'):
            np.testing.assert_array_equal(a.get(), gold[f'advect/disp_{key}'])
        for k, a in fields_d.items():
            np.testing.assert_array_equal(a.get(), gold[f'advect/field_{k}'])
        ph, pd_ = field_power(adv_h, ke, me, poles, D), field_power(adv_d, ke, me, poles, D)
        assert set(ph) == set(pd_) and all(np.array_equal(ph[k], pd_[k]) for k in ph)
        tpos = DeviceArray(gold['tracer/pos'])
        th = tracer_power(gold['tracer/pos'].copy(), adv_h, ke, me, poles, D)
        td = tracer_power(tpos, adv_d, ke, me, poles, D)
        np.testing.assert_array_equal(tpos.get(), gold['tracer/pos_shifted'])
        assert set(th) == set(td) and all(np.array_equal(th[k], td[k]) for k in th)


def test_get_fields_is_bit_identical_from_run_to_run(gold):
    from abacusutils_amd.hod.zcv.ic_fields import get_fields
    rng = np.random.default_rng(3)
    n = 96
    delta = np.exp(0.5 * rng.standard_normal((n, n, n))).astype(np.float32)
    a = get_fields(delta, 300.0, n)
    b = get_fields(delta, 300.0, n)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def test_compute_power_between_two_tracer_power_calls(gold):
    """calc_power_multi (behind AbacusHOD.compute_power) keeps its own field slots; a live AdvectedFields owns its spectra: all three
    results equal those obtained in isolation"""
    from abacusutils_amd.hod.abacus_hod import AbacusHOD
    from abacusutils_amd.hod.zcv import ic_fields as I
    from abacusutils_amd.hod.zcv.advect_fields import advect
    from abacusutils_amd.hod.zcv.tracer_power import tracer_power
    hd, pd, params = synth.synth_hod_inputs(300000, 300000, seed=9, lbox=1000.0)
    hod = dict(HOD_PARAMS, LRG_params=dict(synth.LRG_PARAMS, logM_cut=12.3, logM1=13.3), ELG_params=dict(synth.ELG_PARAMS))
    ball = AbacusHOD.from_arrays(hd, pd, params, hod, CLUSTERING)
    mock = ball.run_hod()
    kw = dict(nbins_k=8, nbins_mu=2, k_hMpc_max=0.2, logk=False, poles=[0, 2], num_cells=64)
    alone = ball.compute_power(mock, **kw)
    tr = np.stack((mock['LRG']['x'], mock['LRG']['y'], mock['LRG']['z']), axis=1).astype(np.float32)
    n, L, D = 64, 1000.0, 0.6
    rng = np.random.default_rng(5)
    dens = I.gaussian_filter(rng.standard_normal((n, n, n)).astype(np.float32), n, L, 0.5 * np.pi * n / L)
    disp = [(0.5 / n) * rng.standard_normal((n, n, n)).astype(np.float32) for _ in range(3)]
    fields = dict(zip(KEYNAMES[1:], I.get_fields(dens, L, n)))
    ke, me = np.linspace(0, 0.2, 9), np.linspace(0, 1, 3)
    with advect(disp, fields, L, n, D) as adv:
        first = tracer_power(tr.copy(), adv, ke, me, [0, 2], D)
        between = ball.compute_power(mock, **kw)
        second = tracer_power(tr.copy(), adv, ke, me, [0, 2], D)
    assert set(between) == set(alone) and set(first) == set(second)
    for k in alone:
        np.testing.assert_array_equal(between[k], alone[k], err_msg=k)
    for k in first:
        np.testing.assert_array_equal(second[k], first[k], err_msg=k)


def test_bad_arguments_raise_the_documented_exceptions(gold):
    from abacusutils_amd._lib import DeviceArray
    from abacusutils_amd.hod.zcv import ic_fields as I
    from abacusutils_amd.hod.zcv.advect_fields import advect, lattice_positions
    from abacusutils_amd.hod.zcv.tracer_power import tracer_power
    z16 = np.zeros((16, 16, 16), dtype=np.float32)
    fields = {k: z16 for k in KEYNAMES[1:]}
    with pytest.raises(ValueError, match='odd'):
        I.get_fields(np.zeros((15, 15, 15), dtype=np.float32), 100.0, 15)
    with pytest.raises(ValueError, match='odd'):
        I.gaussian_filter(np.zeros((15, 15, 15), dtype=np.float32), 15, 100.0, 0.1)
    with pytest.raises(ValueError, match='cubic'):
        I.get_fields(np.zeros((16, 16, 12), dtype=np.float32), 100.0, 16)
    with pytest.raises(ValueError):
        I.get_n2_fft(np.zeros((16, 16, 16), dtype=np.complex64), 16, 100.0)
    d64 = DeviceArray(np.zeros((16, 16, 16), dtype=np.float64))
    with pytest.raises(TypeError):
        I.get_fields(d64, 100.0, 16)
    with pytest.raises(TypeError):
        lattice_positions(d64, d64, d64, 100.0, 0.5)
    with pytest.raises(TypeError):
        advect([z16, z16, z16], dict(fields, delta=d64), 100.0, 16, 0.5)
    with pytest.raises(KeyError):
        advect([z16, z16, z16], fields, 100.0, 16, 0.5, keynames=('1cb', 'vorticity'))
    with pytest.raises(KeyError):
        advect([z16, z16, z16], {'delta': z16}, 100.0, 16, 0.5)
    with pytest.raises(ValueError, match='nmesh'):
        advect([z16, z16, z16], dict(fields, delta2=np.zeros((18, 18, 18), dtype=np.float32)), 100.0, 16, 0.5)
    with pytest.raises(ValueError, match='nmesh'):
        advect([z16, z16, z16], fields, 100.0, 18, 0.5)
    with advect([z16, z16, z16], {'delta': z16}, 100.0, 16, 0.5, keynames=('1cb', 'delta')) as adv:
        with pytest.raises(KeyError):
            adv.spectrum('nabla2')
        with pytest.raises(ValueError):
            tracer_power(np.zeros((10, 2), dtype=np.float32), adv, [0, 0.1], [0, 1], [0], 0.5)
        with pytest.raises(TypeError):
            tracer_power(DeviceArray(np.zeros((10, 3), dtype=np.float64)), adv, [0, 0.1], [0, 1], [0], 0.5)
    with pytest.raises(RuntimeError):
        adv.spectrum('delta')                                 # freed
