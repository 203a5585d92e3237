"""BAO reconstruction on the device (abacusutils_amd.hod.zcv.reconstruction) against tests/recon_statement.py, the float64 NumPy
statement of the four steps (there is no reference implementation), and against closed forms.  Every comparison runs over ALL
cells / particles.  Needs an MI355X: run with `-m gpu`.

Bounds.  The same statement run in float32 gives the noise floor: e_ref = max over the three components of max|psi32 - psi64| /
max|psi64|.  Meshes are held to the rule at the head of tests/test_zcv_gpu.py: 4 e_ref in max-norm relative to the component's
largest value (two independent float32 evaluations, times two for a transform with another summation order), times
log2(n^3) / log2(16^3) beyond 16^3.  Shifted positions are compared in periodic distance: see each test.  The measured ratios are
printed (profiles/recon/README.md records them).  Shapes: n = 16 (native power-of-two transform) and n = 24 (mixed radix, 13 of 16
padded columns used), 2 - 4 x 10^3 particles: the smallest that exercise pitch != n, the Nyquist planes and periodic stencils."""
import functools
import math

import numpy as np
import pytest
import recon_statement as S
from conftest import assert_spectrum_close

from abacusutils_amd import synth

pytestmark = pytest.mark.gpu

L, BIAS, F, R = 100.0, 2.0, 0.8, 10.0
EPS = float(np.finfo(np.float32).eps)
HOD_PARAMS = dict(tracer_flags={'LRG': True, 'ELG': True, 'QSO': False}, want_ranks=False, want_AB=True, want_shear=False, want_rsd=True,
                  LRG_params=synth.LRG_PARAMS, ELG_params=synth.ELG_PARAMS, QSO_params=synth.QSO_PARAMS)       # tests/test_zcv_gpu.py's
CLUSTERING = dict(clustering_type='xirppi', pimax=30, pi_bin_size=5,
                  bin_params=dict(logmin=-0.7728787904780005, logmax=1.4771212597864314, nbins=9))


def _stages(n):
    return max(1.0, math.log2(float(n) ** 3) / math.log2(16.0 ** 3))


@functools.lru_cache(maxsize=None)
def _tracers(n):
    return S.modulated_particles(3000, L, seed=n)


@functools.lru_cache(maxsize=None)
def _randoms():
    rng = np.random.default_rng(77)
    return (rng.random((4000, 3)) * L).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _field(paste, rsd, n):
    """(psi64, psi32, e_ref) of the statement for the tracers of this mesh size; computed once, never modified"""
    pos = _tracers(n)
    p64 = S.displacement_field(pos, L, n, BIAS, F, R, rsd, paste)
    p32 = S.displacement_field(pos, L, n, BIAS, F, R, rsd, paste, np.float32)
    for a in (p64, p32):
        a.setflags(write=False)
    return p64, p32, S.e_ref(p32, p64)


def _check_mesh(label, got, want, e_ref, n, scale=None):
    """every component: max-norm relative to the statement's largest value of that component (or `scale`)"""
    assert got.shape == want.shape == (3, n, n, n) and got.dtype == np.float32, (label, got.shape, got.dtype)
    bound = 4.0 * _stages(n)
    worst = 0.0
    for q, c in enumerate('xyz'):
        ref = np.abs(want[q]).max() if scale is None else scale
        err = np.abs(got[q].astype(np.float64) - want[q]).max() / ref
        print(f'{label} psi_{c}: err {err:.3g}, e_ref {e_ref:.3g}, err / e_ref {err / e_ref:.3g} (bound {bound:.3g})')
        worst = max(worst, err / e_ref)
    assert worst <= bound, f'{label}: err / e_ref {worst:.3g} > {bound:.3g}'


# ------------------------------------------------------------------------------------------------- 1. displacement from particles
@pytest.mark.parametrize('n', [16, 24])
@pytest.mark.parametrize('rsd', [True, False])
@pytest.mark.parametrize('paste', ['CIC', 'TSC'])
def test_displacement_from_particles_matches_the_statement(paste, rsd, n):
    from abacusutils_amd.hod.zcv.reconstruction import displacement_field
    pos = _tracers(n)
    keep = pos.copy()
    p64, _, e_ref = _field(paste, rsd, n)
    assert 1e-8 < e_ref < 1e-5
    with displacement_field(pos, L, n, BIAS, F, R, rsd=rsd, paste=paste) as disp:
        assert (disp.nmesh, disp.Lbox, disp.paste, disp.f_growth, disp.rsd) == (n, L, paste, F, rsd)
        got = disp.fetch()
    assert np.array_equal(pos, keep)
    _check_mesh(f'particles {paste} rsd={rsd} n={n}', got, p64, e_ref, n)


# ------------------------------------------------------------------------------------------------- 2. displacement from a density mesh
@pytest.mark.parametrize('axis', [0, 2])
def test_plane_wave_closed_form(axis):
    """delta = A cos(k x) and A cos(k z) at n = 16: psi = -A S(k) sin(k .) / (k b (1 + beta mu^2)) along the wave; the other two
    components vanish: they are held to 4 e_ref of the wave's amplitude"""
    from abacusutils_amd._lib import DeviceArray
    from abacusutils_amd.hod.zcv.reconstruction import displacement_from_delta
    n, A, mode = 16, 0.3, 2
    delta = S.plane_wave(n, L, A, mode, axis)[0].astype(np.float32)
    keep = delta.copy()
    want = S.plane_wave_displacement(n, L, A, mode, axis, BIAS, F, R, True)
    p64 = S.displacement_from_delta(delta, L, BIAS, F, R, True)
    p32 = S.displacement_from_delta(delta, L, BIAS, F, R, True, np.float32)
    e_ref = float(np.abs(p32[axis] - p64[axis]).max() / np.abs(p64[axis]).max())
    amp = np.abs(want[axis]).max()
    # the float32 rounding of the input mesh moves the statement by less than an ulp of the amplitude
    assert np.abs(p64 - want).max() / amp < 4 * EPS
    with displacement_from_delta(delta, L, BIAS, F, R, rsd=True, paste='TSC') as disp:
        assert disp.paste == 'TSC' and disp.nmesh == n
        got = disp.fetch()
    assert np.array_equal(delta, keep)
    _check_mesh(f'plane wave axis {axis}', got, want, e_ref, n, scale=amp)
    dd = DeviceArray(delta)
    with displacement_from_delta(dd, L, BIAS, F, R) as disp:
        np.testing.assert_array_equal(disp.fetch(), got)
    np.testing.assert_array_equal(dd.get(), delta)
    dd.free()


def test_white_noise_pins_the_nyquist_rule():
    """white noise at n = 16, R = L / 100: full power on every Nyquist plane, where a solver that keeps the wavenumber in i k_i
    hands the inverse transform a spectrum that is not Hermitian"""
    from abacusutils_amd.hod.zcv.reconstruction import displacement_from_delta
    n, R1 = 16, 1.0
    delta = np.random.default_rng(5).standard_normal((n, n, n)).astype(np.float32)
    for rsd in (True, False):
        p64 = S.displacement_from_delta(delta, L, BIAS, F, R1, rsd)
        p32 = S.displacement_from_delta(delta, L, BIAS, F, R1, rsd, np.float32)
        with displacement_from_delta(delta, L, BIAS, F, R1, rsd=rsd) as disp:
            got = disp.fetch()
        _check_mesh(f'white noise rsd={rsd}', got, p64, S.e_ref(p32, p64), n)


# ------------------------------------------------------------------------------------------------- 3. / 4. the shift
def _edge_positions(n, count, seed):
    """random positions plus the corners of the read-out: exactly 0, nextafter(L, 0), negative values, values beyond L, cell centres
    and the half-cell ties (i + 1/2) L / n"""
    rng = np.random.default_rng(seed)
    pos = (rng.random((count, 3)) * L).astype(np.float32)
    cell = L / n
    special = [0.0, float(np.nextafter(np.float32(L), np.float32(0))), -1e-6, -0.3 * cell, -2.5 * cell, -L - 1.0, L, L + 1e-5, L + 2.25 * cell, 2 * L + 3.0]
    special += [i * cell for i in (1, 5, n - 1)] + [(i + 0.5) * cell for i in (0, 3, n - 2, n - 1)]
    k = 0
    for a in range(3):
        for v in special:
            pos[k, a] = v
            k += 1
    for v in special:                         # and all three coordinates at once
        pos[k] = v
        k += 1
    return pos


@pytest.mark.parametrize('paste', ['CIC', 'TSC'])
def test_shift_in_a_constant_field(paste):
    """psi = (c_x, c_y, c_z): every particle lands at wrap(p - c - f c_z z^).  Tolerance 4 eps32 (L + (1 + f) |c|) in periodic
    distance: each coordinate is a short chain of correctly rounded float32 operations on operands bounded by L and (1 + f) |c|"""
    from abacusutils_amd.hod.zcv.reconstruction import Displacement, shift
    n = 24
    c = np.array([3.7, -11.3, 6.1])
    pos = _edge_positions(n, 2000, 3)
    meshes = [np.full((n, n, n), v, dtype=np.float32) for v in c]
    c32 = np.array([m[0, 0, 0] for m in meshes], dtype=np.float64)
    tol = 4 * EPS * (L + (1 + F) * np.abs(c).max())
    with Displacement.from_meshes(*meshes, L, paste, F, True) as disp:
        np.testing.assert_array_equal(disp.fetch(), np.stack(meshes))
        for los, f_z in ((None, F), (0.0, 0.0), (0.35, 0.35)):
            got = shift(pos, disp, los_factor=los)
            assert got.dtype == np.float32 and got.shape == pos.shape and got.min() >= 0 and got.max() <= L
            want = np.remainder(pos.astype(np.float64), L) - c32
            want[:, 2] -= f_z * c32[2]
            err = S.periodic_distance(got, np.remainder(want, L), L)
            print(f'constant field {paste} los={los}: err {err:.3g}, tolerance {tol:.3g}, ratio {err / tol:.3g}')
            assert err <= tol
    with Displacement.from_meshes(*meshes, L, paste, F, False) as disp:         # rsd off: the default los factor is 0
        np.testing.assert_array_equal(shift(pos, disp), shift(pos, disp, los_factor=0.0))


@pytest.mark.parametrize('n', [16, 24])
@pytest.mark.parametrize('paste', ['CIC', 'TSC'])
def test_shift_in_a_smooth_field_matches_the_statement(paste, n):
    """a smooth random field through from_meshes.  Periodic distance <= 4 e_shift max|psi| + eps32 L, e_shift the float32 statement
    against the float64 statement for this step alone, relative to max|psi|"""
    from abacusutils_amd.hod.zcv.reconstruction import Displacement, shift
    delta = np.random.default_rng(11).standard_normal((n, n, n))
    psi = S.displacement_from_delta(delta, L, BIAS, F, R, True)
    psi = (psi * (4.0 / np.abs(psi).max())).astype(np.float32)                 # up to 4 units: 0.6 - 1 cell
    pos = _edge_positions(n, 3000, 4)
    keep = pos.copy()
    pmax = float(np.abs(psi).max())
    with Displacement.from_meshes(psi[0], psi[1], psi[2], L, paste, F, True) as disp:
        for los in (F, 0.0):
            want = S.shift(pos, psi, L, paste, los)
            e_shift = S.periodic_distance(S.shift(pos, psi, L, paste, los, np.float32), want, L) / pmax
            tol = 4 * e_shift * pmax + EPS * L
            got = shift(pos, disp, los_factor=los)
            err = S.periodic_distance(got, want, L)
            print(f'smooth field {paste} n={n} los={los}: err {err:.3g}, e_shift {e_shift:.3g}, tolerance {tol:.3g}, ratio {err / tol:.3g}')
            assert err <= tol
    assert np.array_equal(pos, keep)


# ------------------------------------------------------------------------------------------------- 5. reconstruct
@pytest.mark.parametrize('rsd', [True, False])
@pytest.mark.parametrize('rec_algo', ['recsym', 'reciso'])
def test_reconstruct_matches_the_statement(rec_algo, rsd):
    """tracers and randoms in periodic distance, bound (1 + f) 4 e_ref max|psi| + eps32 L"""
    from abacusutils_amd.hod.zcv.reconstruction import reconstruct
    n, paste = 16, 'CIC'
    tr, rn = _tracers(n), _randoms()
    p64, _, e_ref = _field(paste, rsd, n)
    want_tr, want_rn, psi = S.reconstruct(tr, rn, L, n, BIAS, F, R, rec_algo, rsd, paste)
    assert np.array_equal(psi, p64)
    tol = (1 + F) * 4 * e_ref * float(np.abs(p64).max()) + EPS * L
    got_tr, got_rn = reconstruct(tr, rn, L, n, BIAS, F, R, rec_algo=rec_algo, rsd=rsd, paste=paste)
    for name, got, want, src in (('tracers', got_tr, want_tr, tr), ('randoms', got_rn, want_rn, rn)):
        assert got.dtype == np.float32 and got.shape == src.shape
        err = S.periodic_distance(got, want, L)
        print(f'reconstruct {rec_algo} rsd={rsd} {name}: err {err:.3g}, tolerance {tol:.3g}, ratio {err / tol:.3g}')
        assert err <= tol
    only_tr, none = reconstruct(tr, None, L, n, BIAS, F, R, rec_algo=rec_algo, rsd=rsd, paste=paste)
    assert none is None
    np.testing.assert_array_equal(only_tr, got_tr)
    if rsd and rec_algo == 'reciso':          # the randoms of the two algorithms differ along the line of sight only, by f psi_z
        sym = reconstruct(tr, rn, L, n, BIAS, F, R, rec_algo='recsym', rsd=True, paste=paste)[1]
        np.testing.assert_array_equal(sym[:, :2], got_rn[:, :2])
        assert S.periodic_distance(sym[:, 2], got_rn[:, 2], L) > 0.1


# ------------------------------------------------------------------------------------------------- 6. input forms
@pytest.mark.parametrize('paste', ['CIC', 'TSC'])
def test_input_forms_give_identical_bits(paste):
    from abacusutils_amd._lib import DeviceArray
    from abacusutils_amd.hod.zcv.reconstruction import reconstruct
    n = 24
    tr, rn = _edge_positions(n, 3000, 8), _edge_positions(n, 2500, 9)
    kw = dict(rec_algo='reciso', rsd=True, paste=paste)
    base_tr, base_rn = reconstruct(tr, rn, L, n, BIAS, F, R, **kw)
    assert isinstance(base_tr, np.ndarray) and isinstance(base_rn, np.ndarray)
    tr64, rn64 = tr.astype(np.float64), rn.astype(np.float64)
    got = reconstruct(tr64, rn64, L, n, BIAS, F, R, **kw)
    np.testing.assert_array_equal(got[0], base_tr)
    np.testing.assert_array_equal(got[1], base_rn)
    assert got[0].dtype == np.float32 and np.array_equal(tr64, tr) and np.array_equal(rn64, rn)
    dtr, drn = DeviceArray(tr), DeviceArray(rn)
    got = reconstruct(dtr, drn, L, n, BIAS, F, R, **kw)
    assert all(isinstance(g, DeviceArray) and g.dtype == np.float32 for g in got) and got[0] is not dtr and got[1] is not drn
    np.testing.assert_array_equal(got[0].get(), base_tr)
    np.testing.assert_array_equal(got[1].get(), base_rn)
    np.testing.assert_array_equal(dtr.get(), tr)               # the deposit worked on a copy
    np.testing.assert_array_equal(drn.get(), rn)
    for g in got:
        g.free()
    cols = [[DeviceArray(np.ascontiguousarray(a[:, q])) for q in range(3)] for a in (tr64, rn64)]
    got = reconstruct(tuple(cols[0]), cols[1], L, n, BIAS, F, R, **kw)          # a tuple and a list (what device_xyz returns)
    assert all(isinstance(g, DeviceArray) for g in got)
    np.testing.assert_array_equal(got[0].get(), base_tr)
    np.testing.assert_array_equal(got[1].get(), base_rn)
    for g in got:
        g.free()
    # a non-zero offset equals adding it beforehand (float32 sum)
    off = np.float32(L / 2)
    mtr, mrn = tr - off, rn - off
    want = reconstruct(mtr + off, mrn + off, L, n, BIAS, F, R, **kw)
    got = reconstruct(mtr, mrn, L, n, BIAS, F, R, offset=float(off), **kw)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    mcols = [[DeviceArray(np.ascontiguousarray(a[:, q].astype(np.float64))) for q in range(3)] for a in (mtr, mrn)]
    dgot = reconstruct(mcols[0], mcols[1], L, n, BIAS, F, R, offset=float(off), **kw)
    np.testing.assert_array_equal(dgot[0].get(), want[0])
    np.testing.assert_array_equal(dgot[1].get(), want[1])
    for a in list(dgot) + [dtr, drn] + cols[0] + cols[1] + mcols[0] + mcols[1]:
        a.free()


# ------------------------------------------------------------------------------------------------- 7. the chain in HBM
def test_chain_stays_in_hbm():
    """run_hod -> device_xyz -> reconstruct -> recon_power with nothing on the host, against the same calls through host arrays of
    the same float32 values: equal mode counts, spectra within 1e-5"""
    from abacusutils_amd._lib import DeviceArray
    from abacusutils_amd.hod.abacus_hod import AbacusHOD
    from abacusutils_amd.hod.zcv.linear_fields import linear_fields
    from abacusutils_amd.hod.zcv.reconstruction import reconstruct
    from abacusutils_amd.hod.zcv.tracer_power import recon_power
    Lb, n = 1000.0, 32
    hd, pd, params = synth.synth_hod_inputs(100000, 100000, seed=9, lbox=Lb)
    hod = dict(HOD_PARAMS, LRG_params=dict(synth.LRG_PARAMS, logM_cut=12.3, logM1=13.3), ELG_params=dict(synth.ELG_PARAMS))
    ball = AbacusHOD.from_arrays(hd, pd, params, hod, CLUSTERING)
    mock = ball.run_hod()
    cols = mock.device_xyz('LRG')
    assert cols is not None and len(cols) == 3 and len(cols[0]) > 1000
    rng = np.random.default_rng(2)
    rn = ((rng.random((4 * len(cols[0]), 3)) - 0.5) * Lb).astype(np.float32)          # mock coordinates: [-L/2, L/2)
    half = np.float32(Lb / 2)
    host_tr = (np.stack([mock['LRG'][c] for c in 'xyz'], axis=1) + float(half)).astype(np.float32)
    host_rn = rn + half
    delta = np.random.default_rng(3).standard_normal((n, n, n)).astype(np.float32)
    ke, me, poles = np.linspace(0, np.pi * n / Lb, 9), np.linspace(0, 1, 3), [0, 2]
    kw = dict(rec_algo='recsym', rsd=True, paste='TSC')
    with linear_fields(delta, Lb, n) as lin:
        drn = DeviceArray(rn)
        dtr_rec, drn_rec = reconstruct(cols, drn, Lb, n, 1.8, F, 15.0, offset=float(half), **kw)
        assert isinstance(dtr_rec, DeviceArray) and isinstance(drn_rec, DeviceArray) and dtr_rec.shape == (len(cols[0]), 3)
        dev = recon_power(dtr_rec, drn_rec, lin, ke, me, poles)
        htr_rec, hrn_rec = reconstruct(host_tr, host_rn, Lb, n, 1.8, F, 15.0, **kw)
        host = recon_power(htr_rec, hrn_rec, lin, ke, me, poles)
        for a in (drn, dtr_rec, drn_rec):
            a.free()
    assert mock.device_xyz('LRG') is not None                 # the catalogue in HBM was read, not touched
    assert set(dev) == set(host)
    for k in host:
        if k.startswith('N_'):
            np.testing.assert_array_equal(dev[k], host[k], err_msg=k)
        elif k.startswith('P_'):
            assert_spectrum_close(dev[k], host[k], rtol=1e-5, err_msg=k)
    assert np.isfinite(host['P_kmu_tr_tr']).any() and np.nanmax(np.abs(host['P_kmu_tr_tr'])) > 0


# ------------------------------------------------------------------------------------------------- 8. lifecycle
def test_lifecycle():
    from abacusutils_amd._lib import AbacusHipError
    from abacusutils_amd.hod.zcv.reconstruction import Displacement, displacement_field, shift
    pos = _tracers(16)
    disp = displacement_field(pos, L, 16, BIAS, F, R)
    first = disp.fetch()
    with disp as d:
        assert d is disp
        np.testing.assert_array_equal(shift(pos[:10], d), shift(pos, d)[:10])
    for _ in range(2):
        disp.free()
    with pytest.raises(RuntimeError, match='freed'):
        disp.fetch()
    with pytest.raises(RuntimeError, match='freed'):
        shift(pos, disp)
    again = displacement_field(pos, L, 16, BIAS, F, R)          # the same bits from run to run
    np.testing.assert_array_equal(again.fetch(), first)
    again.free()
    z = np.zeros((16, 16, 16), dtype=np.float32)
    with Displacement.from_meshes(z, z, z, L, 'TSC', 0.0, True) as disp:
        np.testing.assert_array_equal(shift(pos, disp), np.remainder(pos, np.float32(L)))
    assert issubclass(AbacusHipError, RuntimeError)
