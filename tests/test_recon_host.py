"""No-GPU checks of BAO reconstruction (abacusutils_amd.hod.zcv.reconstruction): the module imports without the device library, the
public names and argument lists, every bad argument raises before the library is touched, the C ABI declares the entry points, and
the yardstick itself (tests/recon_statement.py) reproduces the closed form of a plane wave and writes Hermitian spectra."""
import inspect
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import recon_statement as S

REPO = Path(__file__).resolve().parent.parent
E = inspect.Parameter.empty
L, BIAS, F, R = 100.0, 2.0, 0.8, 10.0


def _sig(f):
    return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]


def test_imports_without_the_library():
    code = ('import sys; sys.path.insert(0, %r)\n'
            'from abacusutils_amd import _lib\n'
            'def boom(*a, **k): raise SystemExit("the device library was loaded on import")\n'
            '_lib.lib = boom\n'
            'from abacusutils_amd.hod.zcv import reconstruction as RC\n'
            'from abacusutils_amd.hod import zcv\n'
            'assert zcv.reconstruct is RC.reconstruct and _lib._lib is None\n'
            'print("ok")\n') % str(REPO)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stderr[-2000:] + r.stdout


def test_signatures_and_exports():
    from abacusutils_amd.hod import zcv
    from abacusutils_amd.hod.zcv import reconstruction as RC
    from abacusutils_amd.hod.zcv.tracer_power import recon_power
    assert set(RC.__all__) == {'REC_ALGOS', 'Displacement', 'displacement_field', 'displacement_from_delta', 'shift', 'reconstruct'}
    assert RC.REC_ALGOS == ('recsym', 'reciso')
    assert _sig(RC.displacement_field) == [('tracer_pos', E), ('Lbox', E), ('nmesh', E), ('bias', E), ('f_growth', E), ('R', E), ('rsd', True),
                                           ('paste', 'CIC'), ('offset', 0.0)]
    assert _sig(RC.displacement_from_delta) == [('delta', E), ('Lbox', E), ('bias', E), ('f_growth', E), ('R', E), ('rsd', True), ('paste', 'CIC')]
    assert _sig(RC.shift) == [('pos', E), ('disp', E), ('los_factor', None), ('offset', 0.0)]
    assert _sig(RC.reconstruct) == [('tracer_pos', E), ('random_pos', E), ('Lbox', E), ('nmesh', E), ('bias', E), ('f_growth', E), ('R', E),
                                    ('rec_algo', 'recsym'), ('rsd', True), ('paste', 'CIC'), ('offset', 0.0)]
    assert _sig(RC.Displacement.from_meshes) == [('psi_x', E), ('psi_y', E), ('psi_z', E), ('Lbox', E), ('paste', E), ('f_growth', E), ('rsd', E)]
    assert all(hasattr(RC.Displacement, m) for m in ('fetch', 'free', 'from_meshes', '__enter__', '__exit__'))
    for name in ('Displacement', 'displacement_field', 'displacement_from_delta', 'shift', 'reconstruct'):
        assert getattr(zcv, name) is getattr(RC, name) and name in zcv.__all__
    assert zcv.reconstruction is RC and 'reconstruction' in zcv.__all__ and 'reconstruction' in zcv.__doc__
    assert {'LinearFields', 'recon_power', 'AdvectedFields', 'periodic_window_function'} <= set(zcv.__all__)      # nothing disturbed
    assert 'reconstruct' in recon_power.__doc__ and 'sort' in RC.reconstruct.__doc__.lower() and 'sort' in RC.shift.__doc__.lower()


@pytest.fixture
def no_library(monkeypatch):
    """any attempt to load (or use) the device library fails the test"""
    from abacusutils_amd import _lib

    def boom(*a, **k):
        raise AssertionError('the device library was touched before the arguments were checked')
    monkeypatch.setattr(_lib, 'lib', boom)


def _device(shape, dtype):
    """stands for a DeviceArray of the given dtype and shape without touching the library"""
    from abacusutils_amd._lib import DeviceArray
    a = DeviceArray.__new__(DeviceArray)
    a.ptr, a.shape, a.dtype, a.nbytes, a._view = None, tuple(shape), np.dtype(dtype), 0, True
    return a


def test_bad_arguments_raise_before_the_library_is_loaded(no_library):
    from abacusutils_amd.hod.zcv import reconstruction as RC
    good = np.zeros((10, 3), dtype=np.float32)
    cols = tuple(_device((10,), np.float64) for _ in range(3))

    def field(pos=good, Lbox=L, nmesh=16, bias=BIAS, f=F, R_=R, **kw):
        return RC.displacement_field(pos, Lbox, nmesh, bias, f, R_, **kw)

    def recon(tr=good, rn=good, Lbox=L, nmesh=16, bias=BIAS, f=F, R_=R, **kw):
        return RC.reconstruct(tr, rn, Lbox, nmesh, bias, f, R_, **kw)

    for call in (field, recon):
        with pytest.raises(ValueError, match=r'shape \(N, 3\)'):
            call(np.zeros((10, 2), dtype=np.float32))
        with pytest.raises(ValueError, match=r'shape \(N, 3\)'):
            call(np.zeros(30, dtype=np.float32))
        with pytest.raises(ValueError, match='no particles'):
            call(np.zeros((0, 3), dtype=np.float32))
        with pytest.raises(TypeError, match='float32 or float64'):
            call(np.zeros((10, 3), dtype=np.int32))
        with pytest.raises(TypeError, match='float32'):
            call(_device((10, 3), np.float64))
        with pytest.raises(TypeError, match='float64'):
            call(tuple(_device((10,), np.float32) for _ in range(3)))
        with pytest.raises(ValueError, match='one shape'):
            call((cols[0], cols[1], _device((9,), np.float64)))
        with pytest.raises(ValueError, match='no particles'):
            call(tuple(_device((0,), np.float64) for _ in range(3)))
        with pytest.raises(TypeError):
            call('positions')
        with pytest.raises(ValueError, match='pasting'):
            call(paste='NGP')
        with pytest.raises(ValueError, match='nmesh'):
            call(nmesh=15)
        with pytest.raises(ValueError, match='nmesh'):
            call(nmesh=0)
        with pytest.raises(ValueError, match='bias'):
            call(bias=0.0)
        with pytest.raises(ValueError, match='bias'):
            call(bias=-1.0)
        with pytest.raises(ValueError, match='Lbox'):
            call(Lbox=0.0)
        with pytest.raises(ValueError, match='Lbox'):
            call(Lbox=-5.0)
        with pytest.raises(ValueError, match='R must not be negative'):
            call(R_=-1.0)
        with pytest.raises(ValueError, match='f_growth'):
            call(f=-0.1)
        with pytest.raises(ValueError, match='bias'):
            call(bias=float('nan'))
        with pytest.raises(ValueError, match='offset'):
            call(offset=float('inf'))
    with pytest.raises(ValueError, match='rec_algo'):
        recon(rec_algo='rectangular')
    with pytest.raises(ValueError, match='random_pos'):
        recon(rn=np.zeros((10, 2), dtype=np.float32))
    with pytest.raises(ValueError, match='random_pos holds no particles'):
        recon(rn=np.zeros((0, 3), dtype=np.float32))
    with pytest.raises(TypeError, match='float32'):
        recon(rn=_device((10, 3), np.float64))
    # a density mesh
    z16 = np.zeros((16, 16, 16), dtype=np.float32)
    with pytest.raises(ValueError, match='cubic'):
        RC.displacement_from_delta(np.zeros((16, 16, 12), dtype=np.float32), L, BIAS, F, R)
    with pytest.raises(ValueError, match='nmesh'):
        RC.displacement_from_delta(np.zeros((15, 15, 15), dtype=np.float32), L, BIAS, F, R)
    with pytest.raises(TypeError, match='float32'):
        RC.displacement_from_delta(z16.astype(np.float64), L, BIAS, F, R)
    with pytest.raises(TypeError, match='float32'):
        RC.displacement_from_delta(_device((16, 16, 16), np.float64), L, BIAS, F, R)
    with pytest.raises(ValueError, match='bias'):
        RC.displacement_from_delta(z16, L, 0.0, F, R)
    with pytest.raises(ValueError, match='R must not be negative'):
        RC.displacement_from_delta(z16, L, BIAS, F, -2.0)
    with pytest.raises(ValueError, match='pasting'):
        RC.displacement_from_delta(z16, L, BIAS, F, R, paste='PCS')
    # caller meshes
    with pytest.raises(ValueError, match='psi_y has 18'):
        RC.Displacement.from_meshes(z16, np.zeros((18, 18, 18), dtype=np.float32), z16, L, 'CIC', F, True)
    with pytest.raises(ValueError, match='nmesh'):
        m15 = np.zeros((15, 15, 15), dtype=np.float32)
        RC.Displacement.from_meshes(m15, m15, m15, L, 'CIC', F, True)
    with pytest.raises(TypeError, match='float32'):
        RC.Displacement.from_meshes(z16, z16, z16.astype(np.float64), L, 'CIC', F, True)
    with pytest.raises(ValueError, match='pasting'):
        RC.Displacement.from_meshes(z16, z16, z16, L, 'NGP', F, True)
    with pytest.raises(ValueError, match='Lbox'):
        RC.Displacement.from_meshes(z16, z16, z16, 0.0, 'CIC', F, True)
    # the shift: a holder without meshes is a freed holder
    disp = RC.Displacement(L, 16, 'cic', F, True)
    assert (disp.nmesh, disp.Lbox, disp.paste, disp.f_growth, disp.rsd) == (16, L, 'CIC', F, True)
    with pytest.raises(TypeError, match='Displacement'):
        RC.shift(good, 'not a holder')
    with pytest.raises(RuntimeError, match='freed'):
        RC.shift(good, disp)
    with pytest.raises(RuntimeError, match='freed'):
        disp.fetch()
    with pytest.raises(ValueError, match=r'shape \(N, 3\)'):
        RC.shift(np.zeros((10, 2), dtype=np.float32), disp)
    with pytest.raises(TypeError, match='float32'):
        RC.shift(_device((10, 3), np.float64), disp)
    disp.free()
    disp.free()


def test_header_declares_the_entry_points():
    text = (REPO / 'include' / 'abacus_hip.h').read_text()
    src = (REPO / 'abacusutils_amd' / 'csrc' / 'recon.hip').read_text()
    names = ('abacus_recon_check_memory', 'abacus_recon_pack_soa64_dev', 'abacus_recon_wrap_dev', 'abacus_recon_pad_dev', 'abacus_recon_delta_dev',
             'abacus_recon_displacement_dev', 'abacus_recon_shift_dev')
    for name in names:
        assert re.search(rf'\bint {name}\(', text), name
        assert re.search(rf'\bint {name}\(', src), name
    assert text.index('BAO reconstruction') > text.index('linear control variates')
    for kernel in ('recon_mult', 'recon_shift', 'recon_pack_soa64'):
        assert re.search(rf'__global__[^;{{]*\bvoid {kernel}\(', src), kernel


# ------------------------------------------------------------------------------------------------- the statement itself
@pytest.mark.parametrize('n', [16, 24])
@pytest.mark.parametrize('axis', [0, 1, 2])
@pytest.mark.parametrize('rsd', [True, False])
def test_statement_reproduces_the_plane_wave_closed_form(n, axis, rsd):
    """psi = -A S(k) sin(k x) / (k b (1 + beta mu^2)) along the wave and nothing across it, to float64 rounding.  Modes 1 to 3: the
    transform leaks 1e-16 A into every other mode, and relative to a wave near the Nyquist frequency, which S / k damps by 1e5 at
    R = L / 10, the multiplier of the lowest modes turns that rounding into 1e-11"""
    for mode in (1, 2, 3):
        delta, _ = S.plane_wave(n, L, 0.3, mode, axis)
        got = S.displacement_from_delta(delta, L, BIAS, F, R, rsd)
        want = S.plane_wave_displacement(n, L, 0.3, mode, axis, BIAS, F, R, rsd)
        scale = np.abs(want).max()
        assert scale > 0
        err = np.abs(got - want).max() / scale
        assert err < 1e-12, (n, axis, rsd, mode, err)
    z = S.plane_wave_displacement(n, L, 0.3, 2, 2, BIAS, F, R, True)
    x = S.plane_wave_displacement(n, L, 0.3, 2, 0, BIAS, F, R, True)
    assert np.abs(x).max() / np.abs(z).max() == pytest.approx(1 + F / BIAS, rel=1e-12)      # the Kaiser factor sits on z alone
    assert np.array_equal(S.plane_wave_displacement(n, L, 0.3, 2, 2, BIAS, F, R, False)[2], np.moveaxis(x[0], 0, 2))


@pytest.mark.parametrize('n', [16, 24])
def test_statement_spectra_are_hermitian(n):
    """white noise with full power on every Nyquist plane: the half spectra the statement writes equal their own Hermitian
    completion - the full inverse transform of the completed spectrum has no imaginary part and equals the irfftn.  R = L / 100: the
    smoothing leaves the Nyquist planes their power"""
    R = 1.0
    rng = np.random.default_rng(n)
    delta = rng.standard_normal((n, n, n))
    spec = S.displacement_spectra(delta, L, BIAS, F, R, True)
    assert spec.shape == (3, n, n, n // 2 + 1) and spec.dtype == np.complex128
    neg = (-np.arange(n)) % n
    full = np.zeros((3, n, n, n), dtype=np.complex128)
    full[..., :n // 2 + 1] = spec
    for c in range(n // 2 + 1, n):
        full[..., c] = np.conj(spec[:, neg][:, :, neg][..., n - c])
    x = np.fft.ifftn(full, axes=(1, 2, 3)) * float(n) ** 3
    psi = S.displacement_from_delta(delta, L, BIAS, F, R, True)
    scale = np.abs(psi).max()
    assert np.abs(x.imag).max() < 1e-12 * scale and np.abs(x.real - psi).max() < 1e-12 * scale
    # and the rule is needed: with the full wavenumber in i k_i on the Nyquist planes the imaginary part does not vanish
    kx, kz = S.wavenumbers(n, L)
    bad = spec.copy()
    k2 = kx[n // 2] ** 2 + kx[:, None] ** 2 + kz[None, :] ** 2
    dk = np.fft.rfftn(delta)[n // 2] / float(n) ** 3
    bad[0, n // 2] = 1j * kx[n // 2] * np.exp(-k2 * R * R / 2) / (k2 * BIAS * (1 + (F / BIAS) * kz[None, :] ** 2 / k2)) * dk
    full[..., :n // 2 + 1] = bad
    assert np.abs((np.fft.ifftn(full, axes=(1, 2, 3)) * float(n) ** 3).imag).max() > 1e-3 * scale


def test_statement_clouds_and_noise_floor():
    """weights sum to one, ties and the box edge land on periodic cells, and the float32 statement sits at float32 noise"""
    p = np.array([0.0, np.nextafter(np.float32(L), np.float32(0)), -3.0, L + 7.0, 5 * L / 16, 5.5 * L / 16], dtype=np.float32)
    for paste, K in (('CIC', 2), ('TSC', 3)):
        for dtype in (np.float64, np.float32):
            idx, w = S.cloud(p, 16, L, paste, dtype)
            assert idx.shape == w.shape == (len(p), K) and idx.min() >= 0 and idx.max() < 16 and w.dtype == dtype
            np.testing.assert_allclose(w.sum(axis=1), 1.0, atol=4 * np.finfo(dtype).eps)
        idx, w = S.cloud(p, 16, L, paste)
        rho = S.deposit(np.stack((p, p, p), axis=1), 16, L, paste)
        assert rho.sum() == pytest.approx(len(p), rel=1e-12)
    pos = S.modulated_particles(2000, L, 1)
    assert pos.dtype == np.float32 and 1500 < len(pos) < 2500 and pos.min() >= 0 and pos.max() < L
    p64 = S.displacement_field(pos, L, 16, BIAS, F, R, True, 'CIC')
    p32 = S.displacement_field(pos, L, 16, BIAS, F, R, True, 'CIC', np.float32)
    assert p32.dtype == np.float32 and 1e-8 < S.e_ref(p32, p64) < 1e-5 and 0.3 < np.abs(p64).max() < 5
    tr, rn, psi = S.reconstruct(pos, pos[:100], L, 16, BIAS, F, R, 'reciso', True, 'CIC')
    sym = S.reconstruct(pos, pos[:100], L, 16, BIAS, F, R, 'recsym', True, 'CIC')[1]
    assert np.array_equal(psi, p64) and np.array_equal(sym, tr[:100]) and not np.array_equal(rn[:, 2], sym[:, 2])
    assert np.array_equal(rn[:, :2], sym[:, :2]) and tr.min() >= 0 and tr.max() <= L
