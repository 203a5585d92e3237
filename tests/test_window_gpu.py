"""GPU checks of the ZCV mode-coupling window (abacusutils_amd.hod.zcv.zenbu_window, csrc/window.hip): every golden case through
`periodic_window_function`, and the float64 statement (tests/window_statement.py) evaluated here at the shapes where the kernel
takes another path or can go wrong - column counts that fill no workgroup, one bin, mostly empty bins, the switch from the LDS
histogram to device memory, non-uniform and logarithmic edges, edges that leave part of the mesh out, |k| exactly on an edge.

Bounds.  `nmodes` holds integers below 2^53 in float64: EXACT.  `window` and `keff` against the statement: 1e-9 of the block's
largest entry - both sides add the same float64 terms (the per-mode float32 values are bit-equal) and only the order differs, which
costs at most N * 2^-53 * 9 relative for N <= 10^6 modes per bin.  Against the reference's arrays: 4 x e_ref, the project's usual
factor over the reference's own float32 accumulation noise (tests/golden/zcv_window_cases.npz)."""
import os
from functools import lru_cache

import numpy as np
import pytest
from conftest import load_golden
from window_statement import block_error, window_statement

pytestmark = pytest.mark.gpu

NAMES = [f'n{n}_b{b}_{kin}_{w}' for n, b in ((8, 4), (12, 6), (16, 8), (16, 5)) for kin in ('centres', 'fine') for w in ('k2w', 'flat')]
NAMES.append('n16_integer_edges')
LOGK = ['n8_b4_logk', 'n16_b6_logk']
TOL = 1e-9


@pytest.fixture(scope='module')
def golden():
    return load_golden('zcv_window_cases')


def case(g, name):
    pre = f'case/{name}/'
    return {k[len(pre):]: v for k, v in g.items() if k.startswith(pre)}


def kny(nmesh, lbox):
    return np.pi * nmesh / lbox


def all_modes(nmesh):
    """multiplicities of the whole half mesh: n^2 on the plane k = 0 and 2 n^2 on each of the n/2 - 1 others"""
    return nmesh * nmesh * (nmesh - 1)


def centres(kout):
    return 0.5 * (kout[1:] + kout[:-1])


def check_against(window, keff, want_window, want_keff, nkout, nkin, tol, what):
    e_w = block_error(window, want_window, nkout, nkin)
    e_k = np.abs(keff - want_keff).max() / np.abs(want_keff).max()
    print(f'{what}: window {e_w:.3g}, keff {e_k:.3g} (bounds {tol[0]:.3g}, {tol[1]:.3g})')
    assert e_w <= tol[0], what
    assert e_k <= tol[1], what


@pytest.mark.parametrize('name', NAMES + LOGK)
def test_golden_cases(golden, name):
    from abacusutils_amd.hod.zcv.zenbu_window import periodic_window_function, window_moments
    c = case(golden, name)
    nmesh, lbox, k2w = int(c['nmesh']), float(c['lbox']), bool(c['k2weight'])
    nkout, nkin = len(c['kout']) - 1, len(c['kin'])
    m = window_moments(nmesh, lbox, c['kout'])
    np.testing.assert_array_equal(m['nmodes'], c['nmodes'])
    assert m['S'].shape == (nkout, 3, 3) and m['S'].dtype == np.float64
    np.testing.assert_array_equal(m['S'][:, 0, 0], c['nmodes'])
    window, keff = periodic_window_function(nmesh, lbox, c['kout'], c['kin'], k2weight=k2w)
    assert window.dtype == np.float64 and keff.dtype == np.float64
    assert window.shape == (3 * nkout, 3 * nkin) and keff.shape == (nkout,)
    check_against(window, keff, c['window64'], c['keff64'], nkout, nkin, (TOL, TOL), f'{name} vs statement')
    if name in LOGK:
        # the k = 0 mode lies below the first edge and is left out (the reference wraps it to the last row of the l = 4 block)
        assert c['kout'][0] > 0 and m['nmodes'].sum() == c['nmodes'].sum()
        return
    check_against(window, keff, c['window'], c['keff'], nkout, nkin, (4 * c['e_ref_window'], 4 * c['e_ref_keff']), f'{name} vs reference')


def test_integer_edges_put_every_mode_on_the_right_side(golden):
    """L = 2 pi: the wavenumbers are integers and |k| equals an edge exactly for every mode with an integer norm.  digitize's rule
    is kout[o] <= knorm < kout[o + 1]: such a mode belongs to the bin that STARTS at its edge"""
    from abacusutils_amd.hod.zcv.zenbu_window import window_moments
    c = case(golden, 'n16_integer_edges')
    m = window_moments(16, float(c['lbox']), c['kout'])
    np.testing.assert_array_equal(m['nmodes'], c['nmodes'])
    # counted independently, in integers
    f = np.where(np.arange(16) < 8, np.arange(16), np.arange(16) - 16)
    k2 = f[:, None, None] ** 2 + f[None, :, None] ** 2 + np.arange(8)[None, None, :] ** 2
    mult = np.broadcast_to(np.where(np.arange(8) == 0, 1, 2)[None, None, :], k2.shape)
    want = [mult[(k2 >= o * o) & (k2 < (o + 1) * (o + 1))].sum() for o in range(8)]
    np.testing.assert_array_equal(m['nmodes'], want)
    on_edge = np.isin(k2, np.arange(9) ** 2) & (k2 < 64)
    assert on_edge.sum() >= 50


def _edges(kind, nmesh, lbox, nb):
    k = kny(nmesh, lbox)
    if kind == 'cover':            # beyond the corner of the mesh, sqrt(3) k_Nyquist: every mode is counted
        return np.linspace(0.0, 1.8 * k, nb + 1)
    if kind == 'nyquist':
        return np.linspace(0.0, k, nb + 1)
    if kind == 'short':            # the last edge at 0.6 k_Nyquist
        return np.linspace(0.0, 0.6 * k, nb + 1)
    if kind == 'uneven':
        return k * np.array([0.0, 0.05, 0.1, 0.3, 0.35, 0.7, 1.0, 1.0001, 1.5, 1.8])
    if kind == 'logk':
        from abacusutils_amd.analysis.power_spectrum import get_k_mu_edges
        return get_k_mu_edges(lbox, 1.8 * k, nb, 1, True)[0]
    raise KeyError(kind)


# name: nmesh, box, edges, bins.  nmesh 2 .. 18: 4 .. 324 columns, fewer than one workgroup of 512; 64 and 96: 8 and 18 workgroups.
# 744 | 745 bins: the last size with the histogram in LDS and the first that goes to device memory; 2048: the size asked for.
SHAPES = {
    'n2': (2, 10.0, 'cover', 1), 'n4': (4, 10.0, 'cover', 2), 'n6': (6, 33.0, 'cover', 3), 'n10': (10, 100.0, 'cover', 5),
    'n18': (18, 250.0, 'cover', 9), 'n64_b32': (64, 1000.0, 'nyquist', 32), 'n96_b48': (96, 2000.0, 'nyquist', 48),
    'one_bin': (16, 100.0, 'cover', 1), 'n16_b200': (16, 100.0, 'cover', 200), 'uneven': (24, 150.0, 'uneven', 9),
    'logk': (16, 200.0, 'logk', 7), 'short': (32, 500.0, 'short', 6), 'n16_b744': (16, 100.0, 'cover', 744),
    'n16_b745': (16, 100.0, 'cover', 745), 'n16_b2048': (16, 100.0, 'cover', 2048), 'n64_b1000': (64, 1000.0, 'cover', 1000),
}


@lru_cache(maxsize=None)
def stated(name):
    nmesh, lbox, kind, nb = SHAPES[name]
    kout = _edges(kind, nmesh, lbox, nb)
    kin = centres(kout)
    if len(kin) < 2:
        kin = np.array([0.25, 0.75]) * kout[-1]
    out = window_statement(nmesh, lbox, kout, kin, True)
    for a in (kout, kin) + out:
        a.setflags(write=False)
    return (kout, kin) + out


@pytest.mark.parametrize('name', list(SHAPES))
def test_against_the_statement(name):
    from abacusutils_amd.hod.zcv.zenbu_window import periodic_window_function, window_moments
    nmesh, lbox, kind, nb = SHAPES[name]
    kout, kin, want_window, want_keff, S, nmodes, ksum = stated(name)
    nkout, nkin = len(kout) - 1, len(kin)
    assert nkout == nb
    m = window_moments(nmesh, lbox, kout)
    np.testing.assert_array_equal(m['nmodes'], nmodes)
    if kind in ('cover', 'uneven'):
        assert m['nmodes'].sum() == all_modes(nmesh)
    elif kind == 'logk':
        assert m['nmodes'].sum() == all_modes(nmesh) - 1          # all but k = 0
    else:
        assert 0 < m['nmodes'].sum() < all_modes(nmesh)
    if name == 'n16_b200':
        assert (nmodes == 0).sum() > 50                           # many empty bins
    for q, (got, want) in enumerate(((m['ksum'], ksum), ) + tuple((m['S'][:, a, b], S[:, a, b]) for a in range(3) for b in range(3))):
        scale = np.abs(want).max()
        assert np.abs(got - want).max() <= TOL * scale, (name, q)
    window, keff = periodic_window_function(nmesh, lbox, kout, kin, k2weight=True)
    check_against(window, keff, want_window, want_keff, nkout, nkin, (TOL, TOL), name)
    assert (window[np.tile(nmodes == 0, 3)] == 0).all() and (keff[nmodes == 0] == 0).all()


def test_counts_of_a_2048_mesh():
    """4.3 x 10^9 modes, 4.2 x 10^6 columns: the counts are exact in float64 (the total is beyond 2^32), and the nine sums obey
    what holds for any mesh: S[0, 0] is the count, S[2, 0] = 5 S[0, 2] and S[4, 0] = 9 S[0, 4] up to float32 rounding of the
    products"""
    from abacusutils_amd.hod.zcv.zenbu_window import window_moments
    nmesh, lbox = 2048, 2000.0
    k = kny(nmesh, lbox)
    m = window_moments(nmesh, lbox, np.array([0.0, k, 1.8 * k]))
    assert m['nmodes'].sum() == all_modes(nmesh) == 2048 * 2048 * 2047
    np.testing.assert_array_equal(m['S'][:, 0, 0], m['nmodes'])
    assert (m['nmodes'] > 2 ** 31).all()
    for ell, pref in ((1, 5.0), (2, 9.0)):
        assert np.abs(m['S'][:, ell, 0] - pref * m['S'][:, 0, ell]).max() <= 1e-6 * m['nmodes'].max()
    # the mean wavenumber of the inner bin (a sphere of radius k_Nyquist cut from the cube is the ball itself): 3/4 k to a grid error
    assert abs(m['ksum'][0] / m['nmodes'][0] / k - 0.75) < 1e-3


def test_save_window(tmp_path):
    from abacusutils_amd.analysis.power_spectrum import get_k_mu_edges
    from abacusutils_amd.hod.zcv.zenbu_window import save_window
    nmesh, lbox = 16, 200.0
    fn = save_window(tmp_path, 'AbacusSummit_small', nmesh, lbox, kny(nmesh, lbox), 8)
    assert fn == tmp_path / 'AbacusSummit_small' / 'window_nmesh16.npz' and fn.exists()
    data = np.load(fn)
    assert sorted(data.files) == ['keff', 'window']
    window, keff = data['window'], data['keff']
    k_bins, _ = get_k_mu_edges(lbox, kny(nmesh, lbox), 8, 1, False)
    k_binc = centres(k_bins)
    assert window.shape == (24, 24) and window.dtype == np.float64
    # the two asserts run_zcv makes on the file it loads (tools_cv.py:644-647)
    assert len(keff) == len(k_binc)
    assert np.abs(keff[-1] - k_binc[-1]) / k_binc[-1] < 0.1
    want_window, want_keff = window_statement(nmesh, lbox, k_bins, k_binc, True)[:2]
    check_against(window, keff, want_window, want_keff, 8, 8, (TOL, TOL), 'save_window')
    # an existing file is left alone (its modification time is set to a known past value: no waiting for the clock)
    os.utime(fn, ns=(10 ** 18, 10 ** 18))
    assert save_window(tmp_path, 'AbacusSummit_small', nmesh, lbox, kny(nmesh, lbox), 8) == fn
    assert os.stat(fn).st_mtime_ns == 10 ** 18
    assert save_window(tmp_path, 'AbacusSummit_small', nmesh, lbox, kny(nmesh, lbox), 8, overwrite=True) == fn
    assert os.stat(fn).st_mtime_ns != 10 ** 18
    np.testing.assert_array_equal(np.load(fn)['window'], window)
    # fewer bins than nmesh // 2: the name carries the bin width
    fn5 = save_window(tmp_path, 'AbacusSummit_small', nmesh, lbox, 0.2, 5)
    assert fn5.name == 'window_nmesh16_dk0.040.npz' and np.load(fn5)['keff'].shape == (5,)
