"""tests/power_f64_statement.py (the float64 judge of the dtype=np.float64 path) pinned to what the shimmed reference returned
(tests/golden/power_f64.npz, n = 24, 30 and the odd 21) and to its own long-double form.  CPU only."""
import numpy as np
import pytest
from conftest import assert_spectrum_close, load_golden

import power_f64_statement as st
from abacusutils_amd import synth
from oracle import oracle


@pytest.fixture(scope='module')
def gold():
    g = load_golden('power_f64')
    Lb, N = float(g['meta.L']), int(g['meta.N'])
    pos = synth.synth_positions(N, Lb, seed=300, clustered=True)
    pos2 = synth.synth_positions(N // 2, Lb, seed=301, clustered=True)
    for a in (pos, pos2):
        a.setflags(write=False)
    return g, Lb, pos, pos2


def _close(a, want, tol, what):
    assert a.dtype == want.dtype and a.shape == want.shape, what
    err = np.abs(a - want).max() / np.abs(want).max()
    print(f'{what}: {err:.3g} of the largest value (bound {tol:g})')
    assert err <= tol, (what, err)


@pytest.mark.parametrize('n', [24, 30, 21])
def test_statement_meshes_and_spectra_against_reference_goldens(gold, n):
    """float64 positions: the same float64 operations as the reference up to the order of the sums - 1e-12 of the largest
    value.  float32 positions: the shimmed reference evaluates d**2 of the float32 cloud weights through NumPy's float32 power
    where Numba, the oracle and the device multiply - one float32 ulp of a weight, the 2e-7 of test_power_gpu.py"""
    g, Lb, pos, _ = gold
    w = g['w']
    W = oracle.get_W_compensated(Lb, n, 'TSC', False)
    _close(st.get_field(pos.astype(np.float64), Lb, n, 'CIC'), g[f'n{n}.field_cic_p8'], 1e-12, f'n{n}.field_cic_p8')
    _close(st.get_field_fft(pos.astype(np.float64), Lb, n, 'TSC', None, None, False), g[f'n{n}.fft_tsc_p8'], 1e-12, f'n{n}.fft_tsc_p8')
    _close(st.get_field(pos.copy(), Lb, n, 'TSC', w), g[f'n{n}.field_tsc'], 2e-7, f'n{n}.field_tsc')
    _close(st.get_field_fft(pos.copy(), Lb, n, 'TSC', w, W, True), g[f'n{n}.fft_tsc_comp'], 2e-7, f'n{n}.fft_tsc_comp')


@pytest.mark.parametrize('n', [24, 30, 21])
@pytest.mark.parametrize('name', ['auto', 'cross'])
def test_statement_tables_against_reference_goldens(gold, n, name):
    g, Lb, pos, pos2 = gold
    kw = dict(auto=dict(compensated=True, w=g['w']), cross=dict(compensated=False, pos2=pos2.copy()))[name]
    tab = st.calc_power(pos.copy(), Lb, 10, 3, k_max=np.pi * n / Lb + 1e-6, paste='TSC', nmesh=n, poles=[0, 2, 4], **kw)
    for c in ('N_mode', 'N_mode_poles'):
        np.testing.assert_array_equal(tab[c], g[f'n{n}.{name}.{c}'])
    for c in ('power', 'poles', 'k_avg'):
        assert tab[c].dtype == g[f'n{n}.{name}.{c}'].dtype == np.float32
        assert_spectrum_close(tab[c], g[f'n{n}.{name}.{c}'], rtol=1e-5, err_msg=f'n{n}.{name}.{c}')


def test_cic_statement_agrees_with_the_oracle_float32_mesh():
    """the np.add.at restatement against oracle.cic_serial (float64 clouds summed into a float32 grid): float32 round-off of
    at most ~40 addends per cell, weights and float32 positions included"""
    Lb, n, N = 300.0, 16, 20000
    pos = synth.synth_positions(N, Lb, seed=5, clustered=True)
    w = (0.5 + np.random.default_rng(6).random(N, dtype=np.float32)).astype(np.float32)
    want = np.zeros((n, n, n), dtype=np.float32)
    oracle.cic_serial(pos, want, Lb, weights=w)
    got = st.cic_mesh(pos, Lb, n, w)
    assert abs(got.sum() - w.astype(np.float64).sum()) <= 1e-12 * w.sum()
    assert np.abs(got - want).max() <= 64 * 2.0 ** -24 * want.max()


@pytest.mark.parametrize('n', [40, 104, 210])
def test_float64_transform_round_off_against_long_double(n):
    """e_ref = max |float64 - long double| / max |long double| of the spectrum of white noise: a few 1e-16 (3.0e-16, 3.2e-16,
    4.6e-16 measured at 40, 104, 210).  Outside (1e-17, 1e-14) the statement itself is broken: no long double on the platform
    (0 exactly), or a float32 step somewhere (1e-8)"""
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
    field = np.random.default_rng(n).standard_normal((n, n, n))
    f = st.spectrum(field, longdouble=True)
    assert f.dtype == np.result_type(np.longdouble, np.complex64) and f.dtype.itemsize > 16
    e = st.e_ref(field)
    print(f'n = {n}: e_ref = {e:.2e}')
    assert 1e-17 < e < 1e-14
