"""Linear control variates on the device (abacusutils_amd.hod.zcv.linear_fields, tracer_power.recon_power) against the reference's own
results (tests/golden/lcv_cases.npz, lcv_recon_cases.npz, written by scripts/make_lcv_golden.py) and against known answers.  Every
comparison runs over ALL modes / cells / bins.  Needs an MI355X: run with `-m gpu`.

Bounds are those of tests/test_zcv_gpu.py (the reasoning is in its head): each golden array carries `e_ref`, the reference's own
float32 noise; spectra and 3-D grids are held to 4 e_ref in max-norm relative to the reference's largest value, binned spectra to
max(1e-5, 4 e_ref) of max(|want|, 0.1 max|want|) element by element, every N_* array and every NaN pattern must be equal.  At sizes
beyond the goldens the bound grows with the stages of the transform: times log2(n^3) / log2(16^3).  err / e_ref is printed.

`combine_field_spectra_k3D_lcv(..., 'reciso')` has no reference output (the reference raises ValueError on that branch): it is held
to the golden script's NumPy float32 statement of it, which uses the reference's own `get_smoothing`."""
import math

import numpy as np
import pytest
from conftest import assert_spectrum_close, load_golden

from abacusutils_amd import synth

pytestmark = pytest.mark.gpu

LINEAR = ['white16', 'white24', 'white16_unfiltered']
MODES = ['TSC_TT', 'TSC_FF', 'CIC_TT', 'CIC_FF']
RECON = MODES + ['TSC_TT_norandoms', 'TSC_TT_mu1']
KEYNAMES = ['delta', 'deltamu2']
LIN_PAIRS = ['delta_delta', 'deltamu2_delta', 'deltamu2_deltamu2']
TR_PAIRS = ['tr_tr', 'delta_tr', 'deltamu2_tr']
BINNED = ('P_kmu', 'N_kmu', 'P_ell', 'N_ell')


@pytest.fixture(scope='module')
def gold():
    g = {}
    for name in ('lcv_cases', 'lcv_recon_cases'):
        g.update(load_golden(name))
    return g


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


def _check_binned(label, got, want, e_ref):
    rtol = max(1e-5, 4.0 * float(e_ref))
    want = np.asarray(want, dtype='f8')
    ok = ~np.isnan(want)
    if ok.any():
        floor = 0.1 * np.abs(want[ok]).max()
        err = (np.abs(np.asarray(got, dtype='f8')[ok] - want[ok]) / np.maximum(np.abs(want[ok]), floor)).max()
        print(f'{label}: err {err:.3g}, e_ref {float(e_ref):.3g}, err / e_ref {err / float(e_ref):.3g}, rtol {rtol:.3g}')
    assert_spectrum_close(got, want, rtol=rtol, err_msg=label)


def _check_dict(label, got, gold, head, pairs, ke, me):
    assert set(got) == {'k_binc', 'mu_binc'} | {f'{q}_{p}' for p in pairs for q in BINNED}
    np.testing.assert_array_equal(got['k_binc'], (ke[1:] + ke[:-1]) * 0.5)
    np.testing.assert_array_equal(got['mu_binc'], (me[1:] + me[:-1]) * 0.5)
    for p in pairs:
        np.testing.assert_array_equal(got[f'N_kmu_{p}'], gold[f'{head}/N_kmu_{p}'])
        np.testing.assert_array_equal(got[f'N_ell_{p}'], gold[f'{head}/N_ell_{p}'])
        e = gold[f'{head}/e_ref_{p}']
        _check_binned(f'{label} P_kmu_{p}', got[f'P_kmu_{p}'], gold[f'{head}/P_kmu_{p}'], e)
        _check_binned(f'{label} P_ell_{p}', got[f'P_ell_{p}'], gold[f'{head}/P_ell_{p}'], e)


def _check_3d(label, got, gold, head, pairs):
    assert set(got) == {f'P_k3D_{p}' for p in pairs}
    for p in pairs:
        _check(f'{label} P_k3D_{p}', got[f'P_k3D_{p}'], gold[f'{head}/P_k3D_{p}'], float(gold[f'{head}/e_ref_k3D_{p}']))


def _linear(gold, case='white16', device=False):
    from abacusutils_amd._lib import DeviceArray
    from abacusutils_amd.hod.zcv.linear_fields import linear_fields
    delta = gold[f'linear/{case}/delta_lin']
    return linear_fields(DeviceArray(delta) if device else delta, float(gold[f'linear/{case}/Lbox']), len(delta))


def _mode(name):
    return name[:3], name[4] == 'T', name[5] == 'T'


def _recon(gold, lin, case, tracer=None, randoms=None, **kw):
    from abacusutils_amd.hod.zcv.tracer_power import recon_power
    paste, comp, inter = _mode(case)
    tracer = gold['recon/tracer_pos'].copy() if tracer is None else tracer
    if randoms is None and not case.endswith('norandoms'):
        randoms = gold['recon/random_pos'].copy()
    return recon_power(tracer, randoms, lin, gold['recon/k_bin_edges'], gold[f'recon/{case}/mu_bin_edges'], gold['recon/poles'], paste, comp,
                       inter, **kw)


def test_case_lists_match_the_golden(gold):
    assert [str(s) for s in gold['linear_names']] == LINEAR and [str(s) for s in gold['recon_names']] == RECON
    assert [str(s) for s in gold['combine_names']] == ['recsym', 'reciso']


# ------------------------------------------------------------------------------------------------- 1. linear fields
@pytest.mark.parametrize('case', LINEAR)
def test_linear_fields_match_the_reference(gold, case):
    """white24: not a power of two, 13 of 16 padded columns hold modes; white16_unfiltered: full power on the Nyquist planes, where
    the mode number is negative on x and y"""
    from abacusutils_amd.hod.zcv.linear_fields import KEYNAMES as K, linear_power, linear_power3d
    delta = gold[f'linear/{case}/delta_lin']
    keep = delta.copy()
    ke, me = gold[f'linear/{case}/k_bin_edges'], gold[f'linear/{case}/mu_bin_edges']
    with _linear(gold, case) as lin:
        assert np.array_equal(delta, keep) and lin.keynames == K == tuple(KEYNAMES)
        assert lin.nmesh == len(delta) and lin.Lbox == float(gold[f'linear/{case}/Lbox'])
        for key in KEYNAMES:
            _check(f'linear {case} spectrum {key}', lin.spectrum(key), gold[f'linear/{case}/spec_{key}'],
                   float(gold[f'linear/{case}/e_ref_spec_{key}']))
        got = linear_power(lin, ke, me, gold[f'linear/{case}/poles'])
        got3 = linear_power3d(lin)
    _check_dict(f'linear {case}', got, gold, f'linear/{case}', LIN_PAIRS, ke, me)
    _check_3d(f'linear {case}', got3, gold, f'linear/{case}', LIN_PAIRS)


def test_linear_fields_from_a_device_array(gold):
    from abacusutils_amd._lib import DeviceArray
    from abacusutils_amd.hod.zcv.linear_fields import linear_fields
    delta = gold['linear/white24/delta_lin']
    dd = DeviceArray(delta)
    with _linear(gold, 'white24') as host, linear_fields(dd, float(gold['linear/white24/Lbox']), 24) as dev:
        for key in KEYNAMES:
            np.testing.assert_array_equal(dev.spectrum(key), host.spectrum(key))
    np.testing.assert_array_equal(dd.get(), delta)
    dd.free()


# ------------------------------------------------------------------------------------------------- 2. recon_power
@pytest.mark.parametrize('case', RECON)
def test_recon_power_matches_the_reference(gold, case):
    """tracers and randoms reach three cells outside [0, Lbox) on both sides; `norandoms`: random_pos=None; `mu1`: one mu bin, P_kmu
    is squeezed to (len(k),)"""
    from abacusutils_amd._lib import DeviceArray
    tracer, randoms = gold['recon/tracer_pos'].copy(), gold['recon/random_pos'].copy()
    with_rn = not case.endswith('norandoms')
    ke, me = gold['recon/k_bin_edges'], gold[f'recon/{case}/mu_bin_edges']
    with _linear(gold) as lin:
        got = _recon(gold, lin, case, tracer, randoms if with_rn else None)
        got3 = _recon(gold, lin, case, tracer, randoms if with_rn else None, save_3D_power=True)
        # NumPy inputs are not modified (the TSC deposit wraps a device copy)
        np.testing.assert_array_equal(tracer, gold['recon/tracer_pos'])
        np.testing.assert_array_equal(randoms, gold['recon/random_pos'])
        # float64 positions are deposited as float32; resident float32 positions give the same bits and may be wrapped in place
        got64 = _recon(gold, lin, case, tracer.astype(np.float64), randoms.astype(np.float64) if with_rn else None)
        dt, dr = DeviceArray(tracer), DeviceArray(randoms)
        gotd = _recon(gold, lin, case, dt, dr if with_rn else None)
        L = lin.Lbox
        for dev, host in ((dt, tracer), (dr, randoms)):
            back = dev.get()
            assert np.array_equal(back, host) or (np.abs(np.abs(back - host)[back != host] - np.float32(L)) < 1e-3 * L).all()
            dev.free()
    _check_dict(f'recon {case}', got, gold, f'recon/{case}', TR_PAIRS, ke, me)
    _check_3d(f'recon {case}', got3, gold, f'recon/{case}', TR_PAIRS)
    assert set(got64) == set(got) == set(gotd)
    for k in got:
        np.testing.assert_array_equal(got64[k], got[k], err_msg=k)
        np.testing.assert_array_equal(gotd[k], got[k], err_msg=k)


# ------------------------------------------------------------------------------------------------- 3. field-level combination
def test_combine_field_spectra_k3d_lcv(gold):
    """recsym against the reference's function; reciso against the golden script's NumPy float32 statement (the reference raises
    ValueError on that branch, so there is no reference output for it)"""
    from abacusutils_amd.hod.zcv.linear_fields import combine_field_spectra_k3D_lcv
    bias, f_growth, D, R = (float(gold[f'combine/{k}']) for k in ('bias', 'f_growth', 'D', 'R'))
    L = float(gold['combine/Lbox'])
    assert str(gold['combine/linear_case']) == 'white16' and str(gold['combine/recon_case']) == 'TSC_TT'
    with _linear(gold) as lin:
        with pytest.raises(RuntimeError, match='recon_power'):
            combine_field_spectra_k3D_lcv(bias, f_growth, D, lin, 16, L, None, 'recsym')
        _recon(gold, lin, 'TSC_TT')
        for algo in ('recsym', 'reciso'):
            got = combine_field_spectra_k3D_lcv(bias, f_growth, D, lin, 16, L, R, algo)
            assert len(got) == 3
            for key, g in zip(('pk_tt', 'pk_ll', 'pk_lt'), got):
                _check(f'combine {algo} {key}', g, gold[f'combine/{algo}/{key}'], float(gold[f'combine/{algo}/e_ref_{key}']))
        # recsym ignores R, like the reference
        again = combine_field_spectra_k3D_lcv(bias, f_growth, D, lin, 16, L, None, 'recsym')
        for key, g in zip(('pk_tt', 'pk_ll', 'pk_lt'), again):
            _check(f'combine recsym R=None {key}', g, gold[f'combine/recsym/{key}'], float(gold[f'combine/recsym/e_ref_{key}']))
        with pytest.raises(ValueError, match='R'):
            combine_field_spectra_k3D_lcv(bias, f_growth, D, lin, 16, L, None, 'reciso')
        with pytest.raises(ValueError, match='rec_algo'):
            combine_field_spectra_k3D_lcv(bias, f_growth, D, lin, 16, L, R, 'recs')
        with pytest.raises(ValueError, match='nmesh'):
            combine_field_spectra_k3D_lcv(bias, f_growth, D, lin, 24, L, R, 'recsym')


# ------------------------------------------------------------------------------------------------- 4. known answer at size
def test_plane_wave_known_answer(gold):
    """delta = A cos(2 pi m.x / n) with the oblique integer m = (5, -9, 7) at n = 256: the spectrum is A / 2 at index
    (5, n - 9, 7) and 0 elsewhere (the partner -m has a negative z number and is not stored), deltamu2 is that times
    m_z^2 / |m|^2 = 49 / 155, and P_k3D_delta_delta is A^2 / 4 there.  Errors over ALL modes relative to the expected peak.
    Bound: 4 e log2(n^3) / log2(16^3), e the golden's e_ref of the matching `white16` array.  No LCV kernel strides its lanes
    along z (they walk the flat index of eight padded rows at a time, five trips through the lane loop at this size), so there is
    no second size for a z lane loop."""
    from abacusutils_amd.hod.zcv.linear_fields import linear_fields, linear_power3d
    n, A, L = 256, 0.7, 500.0
    m = np.array([5, -9, 7])
    x = np.arange(n) / n
    delta = (A * np.cos(2 * np.pi * (m[0] * x[:, None, None] + m[1] * x[None, :, None] + m[2] * x[None, None, :]))).astype(np.float32)
    at = (m[0] % n, m[1] % n, m[2])
    mu2 = m[2] ** 2 / float((m ** 2).sum())
    with linear_fields(delta, L, n) as lin:
        for key, peak, e_key in (('delta', 0.5 * A, 'e_ref_spec_delta'), ('deltamu2', 0.5 * A * mu2, 'e_ref_spec_deltamu2')):
            got = lin.spectrum(key).astype(np.complex128)
            got[at] -= peak
            err = np.abs(got).max() / peak
            e = float(gold[f'linear/white16/{e_key}'])
            bound = 4.0 * e * _stages(n)
            print(f'plane wave {n}^3 {key}: err {err:.3g}, e {e:.3g}, err / e {err / e:.3g}, bound {bound:.3g}')
            assert err <= bound, (key, err, bound)
            del got
        p3 = linear_power3d(lin)['P_k3D_delta_delta'].astype(np.float64)
    peak = 0.25 * A * A
    p3[at] -= peak
    err = np.abs(p3).max() / peak
    e = float(gold['linear/white16/e_ref_k3D_delta_delta'])
    bound = 4.0 * e * _stages(n)
    print(f'plane wave {n}^3 P_k3D_delta_delta: err {err:.3g}, e {e:.3g}, err / e {err / e:.3g}, bound {bound:.3g}')
    assert err <= bound, (err, bound)


# ------------------------------------------------------------------------------------------------- 5. plumbing
@pytest.mark.parametrize('mode', MODES)
def test_device_chain_equals_the_composition_of_public_functions(gold, mode):
    """rfftn / n^3 -> get_delta_mu2; get_field_fft twice -> host subtraction; calc_pk_from_deltak x 6 at 64^3 (several trips through
    the kernels' lane loop, many workgroups).  A SECONDARY check: both sides are this package (the right-hand side is pinned by
    the existing tests); the goldens are the primary one."""
    from abacusutils_amd.analysis.power_spectrum import calc_pk_from_deltak, get_delta_mu2, get_field_fft, get_k_mu_edges, get_W_compensated
    from abacusutils_amd.hod.zcv import ic_fields as I
    from abacusutils_amd.hod.zcv.linear_fields import linear_fields, linear_power
    from abacusutils_amd.hod.zcv.tracer_power import recon_power
    paste, comp, inter = _mode(mode)
    n, L = 64, 400.0
    kny = np.pi * n / L
    rng = np.random.default_rng(640)
    dens = I.gaussian_filter(rng.standard_normal((n, n, n)).astype(np.float32), n, L, 0.5 * kny)
    p_sel = np.exp(1.5 * dens.ravel() / dens.std())
    site = np.stack(np.unravel_index(rng.choice(n ** 3, size=40000, p=p_sel / p_sel.sum()), (n, n, n)), axis=1)
    tracer = ((site + rng.uniform(0, 1, site.shape)) * (L / n)).astype(np.float32)
    tracer[:2000] -= np.float32(2.5 * L / n)                  # some beyond the lower faces
    tracer[2000:4000] += np.float32(2.5 * L / n)              # and some beyond the upper ones
    randoms = rng.uniform(-2.0 * L / n, L + 2.0 * L / n, (120000, 3)).astype(np.float32)
    ke, me = get_k_mu_edges(L, kny, 16, 3, False)
    poles = [0, 2, 4]
    with linear_fields(dens, L, n) as lin:
        spec = {k: lin.spectrum(k) for k in KEYNAMES}
        got_lin = linear_power(lin, ke, me, poles)
        got_tr = recon_power(tracer.copy(), randoms.copy(), lin, ke, me, poles, paste, comp, inter)
    d = (np.fft.rfftn(dens.astype(np.float64)) / float(n) ** 3).astype(np.complex64)
    ref = {'delta': d, 'deltamu2': get_delta_mu2(d, n)}
    for k in KEYNAMES:
        _check(f'chain {mode} spectrum {k}', spec[k], ref[k], float(gold[f'linear/white16/e_ref_spec_{k}']), factor=4.0 * _stages(n))
    W = get_W_compensated(L, n, paste, inter) if comp else None
    tr = get_field_fft(tracer.copy(), L, n, paste, None, W, comp, inter)
    tr = tr - get_field_fft(randoms.copy(), L, n, paste, None, W, comp, inter)
    for pair, a, b, got in [(p, ref[p.split('_')[0]], ref[p.split('_')[1]], got_lin) for p in LIN_PAIRS] + \
                           [('tr_tr', tr, None, got_tr), ('delta_tr', ref['delta'], tr, got_tr), ('deltamu2_tr', ref['deltamu2'], tr, got_tr)]:
        P = calc_pk_from_deltak(a, L, ke, me, field2_fft=None if (b is None or a is b) else b, poles=np.asarray(poles))
        np.testing.assert_array_equal(got[f'N_kmu_{pair}'], P['N_mode'])
        np.testing.assert_array_equal(got[f'N_ell_{pair}'], P['N_mode_poles'])
        assert_spectrum_close(got[f'P_kmu_{pair}'], P['power'], rtol=1e-5, err_msg=f'{mode} P_kmu {pair}')
        assert_spectrum_close(got[f'P_ell_{pair}'], P['binned_poles'], rtol=1e-5, err_msg=f'{mode} P_ell {pair}')


# ------------------------------------------------------------------------------------------------- 6. state
HOD_PARAMS = dict(tracer_flags={'LRG': True, 'ELG': True, 'QSO': False}, want_ranks=False, want_AB=True, want_shear=False, want_rsd=True,
                  LRG_params=synth.LRG_PARAMS, ELG_params=synth.ELG_PARAMS, QSO_params=synth.QSO_PARAMS)
CLUSTERING = dict(clustering_type='xirppi', pimax=30, pi_bin_size=5,
                  bin_params=dict(logmin=-0.7728787904780005, logmax=1.4771212597864314, nbins=9))


def test_two_recon_power_calls_on_one_holder_and_compute_power_in_between(gold):
    """the holder keeps the tracer and randoms buffers from call to call: two calls with different tracers equal the same calls in
    isolation, and calc_power_multi (behind AbacusHOD.compute_power) in between changes neither; after free() everything raises"""
    from abacusutils_amd.hod.abacus_hod import AbacusHOD
    from abacusutils_amd.hod.zcv.linear_fields import combine_field_spectra_k3D_lcv, linear_power, linear_power3d
    hd, pd, params = synth.synth_hod_inputs(300000, 300000, seed=9, lbox=1000.0)
    hod = dict(HOD_PARAMS, LRG_params=dict(synth.LRG_PARAMS, logM_cut=12.3, logM1=13.3), ELG_params=dict(synth.ELG_PARAMS))
    ball = AbacusHOD.from_arrays(hd, pd, params, hod, CLUSTERING)
    mock = ball.run_hod()
    kw = dict(nbins_k=8, nbins_mu=2, k_hMpc_max=0.2, logk=False, poles=[0, 2], num_cells=64)
    alone = ball.compute_power(mock, **kw)
    first_tr = gold['recon/tracer_pos']
    second_tr = np.ascontiguousarray(first_tr[::2][:, ::-1])                     # other tracers: half of them, axes swapped
    with _linear(gold) as a:
        want1 = _recon(gold, a, 'TSC_TT', first_tr.copy())
    with _linear(gold) as b:
        want2 = _recon(gold, b, 'CIC_FF', second_tr.copy())
        want2_3d = _recon(gold, b, 'CIC_FF', second_tr.copy(), save_3D_power=True)
    lin = _linear(gold)
    got1 = _recon(gold, lin, 'TSC_TT', first_tr.copy())
    between = ball.compute_power(mock, **kw)
    got2 = _recon(gold, lin, 'CIC_FF', second_tr.copy())
    got2_3d = _recon(gold, lin, 'CIC_FF', second_tr.copy(), save_3D_power=True)
    assert set(between) == set(alone)
    for k in alone:
        np.testing.assert_array_equal(between[k], alone[k], err_msg=k)
    for got, want in ((got1, want1), (got2, want2), (got2_3d, want2_3d)):
        assert set(got) == set(want)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    ke, me, poles = gold['recon/k_bin_edges'], gold['recon/TSC_TT/mu_bin_edges'], gold['recon/poles']
    lin.free()
    lin.free()                                                   # a second free is harmless
    for call in (lambda: linear_power(lin, ke, me, poles), lambda: linear_power3d(lin), lambda: lin.spectrum('delta'),
                 lambda: _recon(gold, lin, 'TSC_TT'), lambda: combine_field_spectra_k3D_lcv(1.8, 0.75, 0.6, lin, 16, lin.Lbox, None, 'recsym')):
        with pytest.raises(RuntimeError, match='freed'):
            call()


# ------------------------------------------------------------------------------------------------- 7. consumption
def _consume_like_run_lcv(power_lin_dict, power_rsd_tr_dict, D, bias, f_growth, poles, rsd=True):
    """the accesses the reference's tools_cv makes to the two dictionaries with rec_algo = 'recsym': combine_kaiser_spectra
    (:196-208) reads P_ell_deltamu2_delta, P_ell_deltamu2_deltamu2, P_ell_delta_delta; combine_cross_kaiser_spectra (:153-163) reads
    P_ell_delta_tr, P_ell_deltamu2_tr (P_kmu_* in real space); run_lcv (:1089-1096) reshapes both results and P_ell_tr_tr to
    (len(poles), len(k_binc)) and flattens N_ell_tr_tr"""
    k_binc = power_rsd_tr_dict['k_binc']
    key = 'P_ell' if rsd else 'P_kmu'
    pk_ll = D ** 2 * (2.0 * bias * f_growth * power_lin_dict[f'{key}_deltamu2_delta'] + f_growth ** 2 * power_lin_dict[f'{key}_deltamu2_deltamu2']
                      + bias ** 2 * power_lin_dict[f'{key}_delta_delta'])
    pk_tl = D * (bias * power_rsd_tr_dict[f'{key}_delta_tr'] + f_growth * power_rsd_tr_dict[f'{key}_deltamu2_tr'])
    if not rsd:
        return k_binc, pk_ll, pk_tl, power_rsd_tr_dict['P_kmu_tr_tr'], power_rsd_tr_dict['N_kmu_tr_tr'].flatten()
    shape = (len(poles), len(k_binc))
    return k_binc, pk_ll.reshape(shape), pk_tl.reshape(shape), power_rsd_tr_dict['P_ell_tr_tr'].reshape(shape), power_rsd_tr_dict['N_ell_tr_tr'].flatten()


@pytest.mark.parametrize('rsd', [True, False])
def test_dictionaries_feed_the_references_run_lcv(gold, rsd):
    """redshift space reads the multipoles as (len(poles), len(k)); real space (one mu bin) reads P_kmu as (len(k),)"""
    from abacusutils_amd.hod.zcv.linear_fields import linear_power
    case = 'TSC_TT' if rsd else 'TSC_TT_mu1'
    ke, me, poles = gold['recon/k_bin_edges'], gold[f'recon/{case}/mu_bin_edges'], gold['recon/poles']
    D, bias, f_growth = 0.6, 1.8, 0.75
    with _linear(gold) as lin:
        power_lin_dict = linear_power(lin, ke, me, poles)
        power_rsd_tr_dict = _recon(gold, lin, case)
    k, pk_ll, pk_tl, pk_tt, nmodes = _consume_like_run_lcv(power_lin_dict, power_rsd_tr_dict, D, bias, f_growth, poles, rsd)
    nk = len(ke) - 1
    shape = (len(poles), nk) if rsd else (nk,)
    assert k.shape == (nk,) and pk_ll.shape == shape and pk_tl.shape == shape and pk_tt.shape == shape and nmodes.shape == (nk,)
    np.testing.assert_array_equal(k, power_lin_dict['k_binc'])
    np.testing.assert_array_equal(nmodes, gold[f'recon/{case}/N_ell_tr_tr'])
    g = {q: gold[f'linear/white16/{"P_ell" if rsd else "P_kmu"}_{q}'] for q in LIN_PAIRS}
    if rsd:
        want_ll = D ** 2 * (2.0 * bias * f_growth * g['deltamu2_delta'] + f_growth ** 2 * g['deltamu2_deltamu2'] + bias ** 2 * g['delta_delta'])
        e = max(float(gold[f'linear/white16/e_ref_{q}']) for q in LIN_PAIRS)
        _check_binned('run_lcv access pk_ll', pk_ll, want_ll, e)
        _check_binned('run_lcv access P_ell_tr_tr', pk_tt, gold[f'recon/{case}/P_ell_tr_tr'], gold[f'recon/{case}/e_ref_tr_tr'])
    else:
        # one mu bin: P_kmu is the monopole
        _check_binned('run_lcv access P_kmu_tr_tr', pk_tt, gold[f'recon/{case}/P_ell_tr_tr'][0], gold[f'recon/{case}/e_ref_tr_tr'])
