"""The float64-mesh path (dtype=np.float64 of get_field / get_field_fft / calc_power: csrc/power.hip field64_dev -> the float64
deposit of csrc/tsc.hip, csrc/gfft.hip instantiated in double, f64_scale_compensate, f64_raw_power) against the plain float64
statement of tests/power_f64_statement.py, at every size class the double-precision transform has code for.

Bounds.  float64 positions: the device and the statement do the same float64 operations in another order - 1e-12 of the
largest |want| (the figure of test_float64_meshes_against_reference_goldens), ~2000 x the round-off of the float64 transform
itself (e_ref, tests/test_power_f64_host.py) and five decades below a float-rounded twiddle or butterfly constant.  float32
positions (or a float32 set beside a float64 one): 2e-7, one float32 ulp of a cloud weight.  Every case prints its error;
the table is kept in profiles/power_f64/README.md."""
import ctypes as C
import warnings

import numpy as np
import pytest
from conftest import assert_spectrum_close

import power_f64_statement as st
from abacusutils_amd import synth

pytestmark = pytest.mark.gpu

L = 1000.0
TOL64, TOL32 = 1e-12, 2e-7


def _positions(npart, seed, dtype=np.float64, outside=True, uniform=False):
    if uniform:
        pos = (np.random.default_rng(seed).random((npart, 3)) * L).astype(dtype)
    else:
        pos = synth.synth_positions(npart, L, seed=seed, clustered=True).astype(dtype)
    if outside:                    # one box length out on either side: the in-place wrap runs
        pos[::7, 0] += L
        pos[3::11, 1] -= L
        pos[5::13, 2] += L
    return pos


def _weights(npart, seed, dtype):
    return (0.5 + np.random.default_rng(seed).random(npart)).astype(dtype)


def _rel_err(got, want):
    """max |got - want| / max |want|, plane by plane (the 770^3 spectra are 3.7 GB each); NaN if anything is NaN"""
    assert got.dtype == want.dtype and got.shape == want.shape
    scale = max(float(np.abs(p).max()) for p in want)
    worst = 0.0
    for a, b in zip(got, want):
        d = float(np.abs(a - b).max())
        if not d <= worst:
            worst = d
            if d != d:
                break
    return worst / scale


def _profiled(fn):
    from abacusutils_amd import _lib
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        out = fn()
    finally:
        _lib.profile_enable(False)
    return out, _lib.profile_get()


def _regime(n):
    """(column tile C, row tile NSEQ, dynamic LDS bytes) of csrc/gfft.hip in double (launch_rows, r2c_inplace): CG = 2 sequences
    per work item, a tile of at most maxv<double>() x G_NT = 12 x 512 complex values, C <= 16, NSEQ <= 32"""
    cap = 12 * 512
    nseq = c = 2
    while 2 * nseq <= 32 and 2 * nseq * (n // 2) <= cap:
        nseq *= 2
    while 2 * c <= 16 and 2 * c * n <= cap:
        c *= 2
    return c, nseq, 16 * max(n + (n // 2) * (nseq + 1), n + n * (c + 1))


# ---- a. the spectrum, size by size ---------------------------------------------------------------------------------------------
SIZES = [8,                 # smallest size the mixed-radix transform takes
         14, 22, 26,        # n/2 a single radix-7 / 11 / 13 stage
         40,                # kzlen = 21 in two column tiles of 16: a ragged last tile inside a row pitch of 24
         56, 88, 104,       # 2^3 x 7, 11, 13
         154, 182, 286,     # two large radices, odd n/2 (286: first column tile above 80 KiB -> one workgroup per CU)
         210,               # 2 x 3 x 5 x 7
         64, 256,           # powers of two: gfft in double (fft.hip is float only)
         384,               # the tile cap exactly at C = 16 / NSEQ = 32: 110,592 B of LDS
         390,               # first size past it: C = 8 / NSEQ = 16
         768,               # the cap exactly in the second regime
         770]               # C = 4 / NSEQ = 8
REGIMES = {8: (16, 32), 40: (16, 32), 384: (16, 32), 390: (8, 16), 768: (8, 16), 770: (4, 8)}


@pytest.mark.parametrize('n', SIZES)
def test_spectrum_by_size(n):
    from abacusutils_amd import _lib
    from abacusutils_amd.analysis.power_spectrum import get_field_fft
    c, nseq, lds = _regime(n)
    if n in REGIMES:
        assert (c, nseq) == REGIMES[n]
    if n in (286, 384, 768):                    # dynamic LDS above 80 KiB: hipFuncSetAttribute, one workgroup per CU
        assert lds > 80 * 1024
    npart = 20_000 if n <= 210 else 200_000
    pos = _positions(npart, seed=n)
    p_dev, p_st = pos.copy(), pos.copy()
    got, prof = _profiled(lambda: get_field_fft(p_dev, L, n, 'TSC', None, None, False, False, dtype=np.float64))
    assert got.dtype == np.complex128 and got.shape == (n, n, n // 2 + 1)
    for k in ('gfft_rows', 'gfft_cols_y', 'gfft_cols_x'):
        assert k in prof, sorted(prof)
    assert 'hipfft_d2z' not in prof, sorted(prof)
    field = st.get_field(p_st, L, n, 'TSC')
    np.testing.assert_array_equal(p_dev, p_st)                     # wrapped in place like oracle.wrap_inplace
    want = st.spectrum(field)
    err = _rel_err(got, want)
    msg = f'f64 spectrum n = {n}: C = {c}, NSEQ = {nseq}, LDS = {lds} B, err = {err:.3g}'
    if n <= 210:
        ld = st.spectrum(field, longdouble=True)
        e_ref = float(np.abs(want - ld).max() / np.abs(ld).max())
        msg += f', e_ref = {e_ref:.3g}, err / e_ref = {err / e_ref:.3g}'
    print(msg)
    assert err <= TOL64, msg
    if n == 40:
        # every element of the output is written: the entry point itself into a NaN-filled buffer
        out = np.full((n, n, n // 2 + 1), np.nan + 1j * np.nan, dtype=np.complex128)
        p2 = pos.copy()
        _lib.check(_lib.lib().abacus_field_fft_f64(_lib.ptr(p2), 1, C.c_int64(len(p2)), None, C.c_double(L), n, 0, None, _lib.ptr(out)))
        assert not np.isnan(out.view(np.float64)).any()
        assert _rel_err(out, want) <= TOL64


# ---- b. sizes left to hipFFT's double-precision transform on the same padded in-place layout -----------------------------------
@pytest.mark.parametrize('n', [6, 34])          # below 8; a prime factor above 13 (row pitch 48 != n + 2)
def test_even_sizes_on_the_hipfft_side(n):
    from abacusutils_amd.analysis.power_spectrum import get_field_fft
    pos = _positions(20_000, seed=n)
    p_dev, p_st = pos.copy(), pos.copy()
    got, prof = _profiled(lambda: get_field_fft(p_dev, L, n, 'TSC', None, None, False, False, dtype=np.float64))
    assert 'hipfft_d2z' in prof and not any(k.startswith('gfft_') for k in prof), sorted(prof)
    field = st.get_field(p_st, L, n, 'TSC')
    want = st.spectrum(field)
    ld = st.spectrum(field, longdouble=True)
    e_ref = float(np.abs(want - ld).max() / np.abs(ld).max())
    err = _rel_err(got, want)
    print(f'f64 spectrum n = {n} (hipFFT D2Z): err = {err:.3g}, e_ref = {e_ref:.3g}, err / e_ref = {err / e_ref:.3g}')
    assert err <= TOL64
    np.testing.assert_array_equal(p_dev, p_st)


# ---- c. the float64 mesh -------------------------------------------------------------------------------------------------------
def _entries_per_cell(pos, shape, reach):
    """how many cloud entries land in each cell: particles per nearest cell, spread over the cloud's reach (3 cells per axis for
    TSC, the 2 of a CIC cloud bounded by 3)"""
    idx = [np.rint(pos[:, a].astype(np.float64) / L * shape[a]).astype(np.int64) % shape[a] for a in range(3)]
    cnt = np.bincount((idx[0] * shape[1] + idx[1]) * shape[2] + idx[2], minlength=int(np.prod(shape))).reshape(shape)
    for a in range(3):
        cnt = sum(np.roll(cnt, s, axis=a) for s in range(-(reach // 2), reach // 2 + 1))
    return int(cnt.max())


def _assert_sums_short_enough(kmax):
    # both sides add at most kmax float64 terms of one sign per cell, each in its own order: each sum is off by at most
    # kmax 2^-53 of its value, their difference by kmax 2^-52, and the cloud products and the normalisation add a few ulp
    assert (kmax + 4) * 2.0 ** -52 <= TOL64, kmax


MESH_CASES = [(50_000, False), (2_100_000, True)]       # (particles, uniform); 2.1e6: the multisplit list build (>= 2e6)


@pytest.mark.parametrize('ptype', [np.float32, np.float64], ids=['pos32', 'pos64'])
@pytest.mark.parametrize('n', [64, 40])
@pytest.mark.parametrize('npart,uniform', MESH_CASES)
@pytest.mark.parametrize('paste', ['TSC', 'CIC'])
def test_get_field(paste, npart, uniform, n, ptype):
    """TSC with weights and a shift of 0.37 cells, positions partly outside the box; CIC (no wrap in the reference: inside)"""
    from abacusutils_amd.analysis.power_spectrum import get_field
    tsc = paste == 'TSC'
    pos = _positions(npart, seed=n + npart % 97, dtype=ptype, outside=tsc, uniform=uniform)
    w = _weights(npart, 9, ptype) if tsc else None
    d = 0.37 * L / n if tsc else 0.0
    p_dev, p_st = pos.copy(), pos.copy()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')           # the CIC advice of the reference
        got = get_field(p_dev, L, n, paste, w, d, dtype=np.float64)
    want = st.get_field(p_st, L, n, paste, w, d)
    kmax = _entries_per_cell(p_st + ptype(d), (n, n, n), 3)
    _assert_sums_short_enough(kmax)
    # (a CIC cloud is float64 arithmetic whatever the dtype of the positions, analysis/cic.py:30-33)
    tol = TOL64 if ptype == np.float64 or not tsc else TOL32
    err = _rel_err(got, want)
    wsum = float(npart) if w is None else float(w.astype(np.float64).sum())
    mass = abs(float((got + 1.0).sum()) * npart / n ** 3 - wsum) / wsum
    print(f'f64 mesh {paste} n = {n}, {npart} x {np.dtype(ptype).name}: err = {err:.3g}, mass = {mass:.3g}, <= {kmax} addends per cell')
    assert err <= tol
    # the float32 TSC cloud weights of the reference sum to 1 only to float32 round-off (the statement's own mass is off by 2e-10)
    assert mass <= (TOL32 if tsc and ptype == np.float32 else TOL64)
    if tsc:
        np.testing.assert_array_equal(p_dev, p_st)
        assert p_dev.min() >= 0 and p_dev.max() <= L
        inside = p_dev.copy()                     # a second call: nothing left to wrap, the array stays as it is
        get_field(p_dev, L, n, paste, w, d, dtype=np.float64)
        np.testing.assert_array_equal(p_dev, inside)
    else:
        np.testing.assert_array_equal(p_dev, pos)


@pytest.mark.parametrize('ptype', [np.float32, np.float64], ids=['pos32', 'pos64'])
@pytest.mark.parametrize('npart,uniform', MESH_CASES)
def test_tsc_parallel_into_a_float64_grid_that_holds_values(npart, uniform, ptype):
    """an anisotropic (50, 77, 40) user grid, accumulated into, offset -0.3 cells"""
    from abacusutils_amd.analysis.tsc import tsc_parallel
    shape, off = (50, 77, 40), -0.3 * L / 77
    pos = _positions(npart, seed=77 + npart % 97, dtype=ptype, uniform=uniform)
    w = _weights(npart, 10, ptype)
    start = np.random.default_rng(11).random(shape) * (npart / np.prod(shape))      # of the size of a cell's mass
    got, want = start.copy(), start.copy()
    p_dev, p_st = pos.copy(), pos.copy()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')           # the float32 advice of the reference
        assert tsc_parallel(p_dev, got, L, weights=w, offset=off) is None
    st.tsc_mesh(p_st, L, shape, w, off, grid=want)
    kmax = _entries_per_cell(p_st + ptype(off), shape, 3) + 1
    _assert_sums_short_enough(kmax)
    err = _rel_err(got, want)
    wsum = float(w.astype(np.float64).sum())
    mass = abs(float((got - start).sum()) - wsum) / wsum
    print(f'f64 grid (50, 77, 40), {npart} x {np.dtype(ptype).name}: err = {err:.3g}, mass = {mass:.3g}, <= {kmax} addends per cell')
    assert err <= (TOL64 if ptype == np.float64 else TOL32)
    # (got - start) cancels the values the grid held: a few ulp of the cell values on top of the deposit's own
    assert mass <= (TOL32 if ptype == np.float32 else TOL64)
    np.testing.assert_array_equal(p_dev, p_st)


def test_multisplit_fine_pass_feeds_the_float64_tile_deposit():
    """256^3: 2048 tiles of 16 x 16 x 32 are more than the 1024 buckets of the coarse pass, so the lists of 2.1e6 particles
    go through ms_fine as well (at 64 and 40 every coarse bucket is a tile already)"""
    from abacusutils_amd.analysis.power_spectrum import get_field
    n, npart = 256, 2_100_000
    pos = _positions(npart, seed=256, uniform=True)
    w = _weights(npart, 12, np.float64)
    p_dev, p_st = pos.copy(), pos.copy()
    got, prof = _profiled(lambda: get_field(p_dev, L, n, 'TSC', w, dtype=np.float64))
    assert 'tsc_ms_fine_scatter' in prof and 'tsc_ms_coarse_scatter' in prof, sorted(prof)
    want = st.get_field(p_st, L, n, 'TSC', w)
    _assert_sums_short_enough(_entries_per_cell(p_st, (n, n, n), 3))
    err = _rel_err(got, want)
    print(f'f64 mesh TSC n = 256, {npart} x float64 (ms_fine): err = {err:.3g}')
    assert err <= TOL64
    np.testing.assert_array_equal(p_dev, p_st)


# ---- d. the whole chain --------------------------------------------------------------------------------------------------------
def _ragged_edges(n):
    return np.pi * n / L * np.array([0.0, 0.04, 0.05, 0.21, 0.22, 0.5, 0.83, 1.0])


CHAIN = {
    'auto': dict(compensated=True, weights=True),
    'cross': dict(compensated=False, cross=np.float64),
    'mixed': dict(compensated=True, cross=np.float64, ptype=np.float32),       # pos float32 beside pos2 float64
    'ragged': dict(compensated=True, ragged=True),
}


@pytest.mark.parametrize('variant', list(CHAIN))
@pytest.mark.parametrize('n', [104, 390])
def test_calc_power_float64_chain(n, variant):
    from abacusutils_amd.analysis.power_spectrum import calc_power
    v = CHAIN[variant]
    npart = 100_000
    ptype = v.get('ptype', np.float64)
    pos = _positions(npart, seed=n + 1, dtype=ptype)
    kw = dict(paste='TSC', nmesh=n, compensated=v['compensated'], poles=[0, 2, 4])
    if v.get('weights'):
        kw['w'] = _weights(npart, 13, ptype)
    if 'cross' in v:
        kw['pos2'] = _positions(npart // 2, seed=n + 2, dtype=v['cross'])
    kbins = _ragged_edges(n) if v.get('ragged') else 40
    kw_dev = dict(kw, pos2=kw['pos2'].copy()) if 'pos2' in kw else kw
    tab = calc_power(pos.copy(), L, kbins=kbins, mubins=5, interlaced=False, dtype=np.float64, **kw_dev)
    kw_st = dict(kw, pos2=kw['pos2'].copy()) if 'pos2' in kw else kw
    want = st.calc_power(pos.copy(), L, kbins, 5, **kw_st)
    for c in ('N_mode', 'N_mode_poles'):
        np.testing.assert_array_equal(np.asarray(tab[c]), want[c], err_msg=c)
    for c in ('power', 'poles', 'k_avg'):
        assert np.asarray(tab[c]).dtype == want[c].dtype == np.float32
        assert_spectrum_close(tab[c], want[c], rtol=1e-5, err_msg=f'n = {n} {variant} {c}')


def test_interlaced_ignores_the_mesh_dtype():
    """the interlaced branch of the reference never sees dtype (analysis/power_spectrum.py:1048-1052): the float32 call, bit for bit"""
    from abacusutils_amd.analysis.power_spectrum import calc_power
    n = 104
    pos = _positions(20_000, seed=3, dtype=np.float32)
    kw = dict(kbins=40, mubins=5, paste='TSC', nmesh=n, compensated=True, interlaced=True, poles=[0, 2, 4])
    a = calc_power(pos.copy(), L, dtype=np.float64, **kw)
    b = calc_power(pos.copy(), L, **kw)
    for c in ('power', 'N_mode', 'poles', 'N_mode_poles', 'k_avg'):
        np.testing.assert_array_equal(np.asarray(a[c]), np.asarray(b[c]), err_msg=c)
