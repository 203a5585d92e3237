"""Tidal shear on the device (abacusutils_amd.analysis.shear, prepare_sim.calc_shearmark) against the reference's own results
(tests/golden/shear_cases.npz, written by scripts/make_shear_golden.py) and against known answers.  Every comparison runs over
ALL cells of the mesh.  Needs an MI355X: run with `-m gpu`.

Bounds: the smoothing bound is derived (non-negative inputs, positive weights: three passes, each a 2 radius + 1 term sum plus one
store); shear and tidal cases are held to 4 e_ref, e_ref being the reference's own float32 noise stored with each case (two
independent float32 evaluations, times two for a transform with another summation order)."""
import json

import numpy as np
import pytest
from conftest import GOLD, load_golden

pytestmark = pytest.mark.gpu

MINI = GOLD / 'Mini_N64_L32'


@pytest.fixture(scope='module')
def gold():
    return load_golden('shear_cases')


def _names(g, key):
    return [str(s) for s in g[key]]


SMOOTH = ['p16_s0.5', 'p16_s1.0', 'p16_s2.3', 'p12_s3.5']
SHEAR = ['poisson16', 'lognormal24', 'lognormal32', 'lognormal24_R3', 'mini32']
TIDAL = ['poisson16', 'poisson16_R4']


def test_case_lists_match_the_golden(gold):
    assert _names(gold, 'smooth_names') == SMOOTH and _names(gold, 'shear_names') == SHEAR and _names(gold, 'tidal_names') == TIDAL


# ---------------------------------------------------------------------------------------------------- 1. smoothing
@pytest.mark.parametrize('name', SMOOTH)
def test_smoothing_matches_scipy_within_the_derived_bound(gold, name):
    from abacusutils_amd.analysis.shear import smooth_density
    D, want = gold[f'smooth/{name}/D'], gold[f'smooth/{name}/out']
    N, radius = len(D), int(gold[f'smooth/{name}/radius'])
    assert radius == {'p16_s0.5': 2, 'p16_s1.0': 4, 'p16_s2.3': 9, 'p12_s3.5': 14}[name] and (name != 'p12_s3.5' or radius > N)
    keep = D.copy()
    got = smooth_density(D, float(gold[f'smooth/{name}/R']), N, float(gold[f'smooth/{name}/Lbox']))
    assert np.array_equal(D, keep) and got.dtype == np.float32 and got.shape == want.shape
    err = np.abs(got.astype(np.float64) - want)
    bound = 3 * (2 * radius + 2) * 2.0 ** -24 * want.astype(np.float64)
    print(f'smoothing {name}: max err / bound = {(err / bound).max():.3g}, max rel err {(err / want).max():.3g}')
    assert (want > 0).all() and (err <= bound).all()


@pytest.mark.parametrize('sigma', [0.5, 1.0, 2.3, 5.0])
def test_constant_field_stays_constant(sigma):
    """normalisation and the reflect boundary: to 1 ulp, in every cell"""
    from abacusutils_amd.analysis.shear import smooth_density
    N, c = 14, np.float32(3.7)
    got = smooth_density(np.full((N, N, N), c, dtype=np.float32), sigma, N, float(N))
    assert np.abs(got - c).max() <= np.spacing(c)


def test_corner_spike_is_reflected_not_wrapped():
    """a spike in cell (0, 0, 0): with `reflect` the cell's mirror image lies next to it, so along each axis the response is
    w[j] + w[j + 1] at distance j (separable: the product over the axes) - and nothing arrives at the far faces, where a periodic
    filter would put w[1]"""
    from abacusutils_amd.analysis.shear import gaussian_weights, smooth_density
    N, sigma = 16, 1.0
    radius, w = gaussian_weights(sigma)
    D = np.zeros((N, N, N), dtype=np.float32)
    D[0, 0, 0] = 1.0
    got = smooth_density(D, sigma, N, float(N))
    full = np.concatenate([w, np.zeros(N)])
    line = np.array([full[j] + full[j + 1] for j in range(N)])
    want = line[:, None, None] * line[None, :, None] * line[None, None, :]
    assert np.abs(got - want).max() <= 1e-6 * want.max()
    assert got[N - 1, 0, 0] == 0 and got[0, N - 1, 0] == 0 and got[0, 0, N - 1] == 0        # a wrapped filter leaves w[1] w[0]^2 there
    assert abs(got.sum(dtype=np.float64) - 1) < 1e-5
    # a mesh that is already on the device: same values, returned on the device, the input untouched
    from abacusutils_amd import _lib
    dev = _lib.DeviceArray(D)
    out = smooth_density(dev, sigma, N, float(N))
    assert isinstance(out, _lib.DeviceArray) and np.array_equal(out.get(), got) and np.array_equal(dev.get(), D)


# ---------------------------------------------------------------------------------------------------- 2. shear vs the golden
@pytest.mark.parametrize('name', SHEAR)
def test_shear_matches_the_reference(gold, name):
    from abacusutils_amd.analysis.shear import get_shear
    dsmo, ref = gold[f'shear/{name}/dsmo'], gold[f'shear/{name}/out']
    R, e_ref = float(gold[f'shear/{name}/R']), float(gold[f'shear/{name}/e_ref'])
    got = get_shear(dsmo, len(dsmo), float(gold[f'shear/{name}/Lbox']), R=None if R < 0 else R)
    assert got.dtype == np.float32 and got.shape == ref.shape
    err = np.abs(got.astype(np.float64) - ref).max() / ref.max()
    print(f'shear {name}: max |got - ref| / max(ref) = {err:.3g} = {err / e_ref:.2f} e_ref (e_ref {e_ref:.3g})')
    assert err <= 4 * e_ref


def test_get_shear_reads_a_npy_path_and_keeps_device_arrays_on_the_device(gold, tmp_path):
    from abacusutils_amd import _lib
    from abacusutils_amd.analysis.shear import get_shear
    dsmo = gold['shear/poisson16/dsmo']
    a = get_shear(dsmo, 16, 50.0)
    np.save(tmp_path / 'd.npy', dsmo)
    assert np.array_equal(get_shear(str(tmp_path / 'd.npy'), 16, 50.0), a)
    dev = _lib.DeviceArray(dsmo)
    out = get_shear(dev, 16, 50.0)
    assert isinstance(out, _lib.DeviceArray) and np.array_equal(out.get(), a) and np.array_equal(dev.get(), dsmo)


# ---------------------------------------------------------------------------------------------------- 3. known answers
def _wave(N, mode, phase=0.3, A=1.0):
    x = np.arange(N)
    arg = 2 * np.pi * (mode[0] * x[:, None, None] + mode[1] * x[None, :, None] + mode[2] * x[None, None, :]) / N + phase
    return A * np.cos(arg)


@pytest.mark.parametrize('N', [16, 20, 64])
@pytest.mark.parametrize('axis', [0, 1, 2])
def test_plane_wave_along_an_axis_gives_exactly_zero(N, axis):
    """the reference skips every mode with a zero index: a wave along one axis has no tidal field at all.  Exactly zero where the
    forward transform of a constant row is exact - radix-2 butterflies form v - v = 0, so N = 16 and 64 -; a radix-5 butterfly (N = 20)
    sums five rounded products that cancel only to rounding, which leaks a few 2^-24 of the amplitude into kept modes: there the
    field is held to the single-mode tolerance of 1e-5 of the amplitude (observed: 2e-16)"""
    from abacusutils_amd.analysis.shear import get_shear
    mode = [0, 0, 0]
    mode[axis] = 3
    got = get_shear(_wave(N, mode).astype(np.float32), N, 100.0)
    print(f'plane wave N = {N} axis {axis}: max shear {got.max():.3g}')
    assert got.shape == (N, N, N)
    if N & (N - 1) == 0:
        assert not got.any()
    else:
        assert got.max() <= 1e-5


@pytest.mark.parametrize('N,mode', [(16, (1, 2, 3)), (20, (3, 1, 2)), (64, (5, 60, 7)), (34, (2, 3, 4))])
def test_single_mode_gives_the_modulus_of_the_wave(N, mode):
    """k k^T / k^2 - I / 3 has eigenvalues 2/3, -1/3, -1/3: the shear is |delta(x)|.  Sizes: mixed-radix (16, 20), power of two (64)
    and one only hipFFT covers (34 = 2 * 17)"""
    from abacusutils_amd.analysis.shear import get_shear
    A = 2.5
    d = _wave(N, mode, A=A)
    got = get_shear(d.astype(np.float32), N, 75.0)
    err = np.abs(got - np.abs(d)).max() / A
    print(f'single mode N = {N}: max err / A = {err:.3g}')
    assert err <= 1e-5


def _shear64(d, N, Lbox, nyquist_sign=-1.0):
    """float64 statement of the definition with NumPy's transforms: modes with a zero index dropped, wavenumbers fftfreq's (the
    Nyquist entry negative; `nyquist_sign=+1` flips it, to show that a test tells the two apart)"""
    df = np.fft.rfftn(d.astype(np.float64))
    k = np.fft.fftfreq(N, d=Lbox / (2 * np.pi * N))
    k[N // 2] *= -nyquist_sign
    ka, kb, kc = k[:, None, None], k[None, :, None], k[None, None, :N // 2 + 1]
    i = np.arange(N)
    mask = (i[:, None, None] * i[None, :, None] * i[None, None, :N // 2 + 1]) != 0
    dok2 = np.where(mask, df / np.where(mask, ka ** 2 + kb ** 2 + kc ** 2, 1.0), 0.0)
    t = [np.fft.irfftn(c * dok2, s=(N, N, N), axes=(0, 1, 2)) for c in (ka * ka, ka * kb, ka * kc, kb * kb, kb * kc, kc * kc)]
    tr2 = t[0] ** 2 + t[3] ** 2 + t[5] ** 2 + 2 * (t[1] ** 2 + t[2] ** 2 + t[4] ** 2)
    return np.sqrt(np.maximum(0.5 * (3 * tr2 - (t[0] + t[3] + t[5]) ** 2), 0))


@pytest.mark.parametrize('modes', [((1, 2, 8), (2, 1, 3)), ((8, 2, 3), (2, 1, 3)), ((3, 8, 8), (1, 1, 1))])
def test_nyquist_modes_follow_fftfreq(modes):
    """a mode on a Nyquist plane (index N/2 = 8) superposed with an ordinary one: the cross terms between the two depend on the sign
    the Nyquist wavenumber is given.  On the x / y planes flipping the sign changes the field far beyond the tolerance; on the
    z plane the non-Hermitian part drops out of the reference's inverse transform, and must here too."""
    from abacusutils_amd.analysis.shear import get_shear
    N, L, A = 16, 40.0, 1.0
    d = _wave(N, modes[0], phase=0.4, A=A) + _wave(N, modes[1], phase=1.1, A=0.7 * A)
    want = _shear64(d, N, L)
    got = get_shear(d.astype(np.float32), N, L)
    err = np.abs(got - want).max() / A
    other = np.abs(_shear64(d, N, L, nyquist_sign=+1.0) - want).max() / A
    print(f'nyquist {modes}: max err / A = {err:.3g}; the other sign convention is {other:.3g} away')
    assert err <= 1e-5
    if modes[0][2] != N // 2:
        assert other > 1e-2


@pytest.mark.parametrize('N,mode', [(1000, (3, 994, 7)), (1024, (1019, 2, 5))])
def test_single_mode_on_full_size_meshes(N, mode):
    """64-bit indexing, the mixed-radix (1000 = 2^3 5^3) and the power-of-two transform at the production size: the single-mode
    answer, checked in every cell (plane by plane on the host)"""
    from abacusutils_amd import _lib
    from abacusutils_amd.analysis.shear import get_shear
    A = 1.5
    x = np.arange(N, dtype=np.float64)
    ph = 2 * np.pi / N
    d = np.empty((N, N, N), dtype=np.float32)
    yz = ph * (mode[1] * x[:, None] + mode[2] * x[None, :]) + 0.3
    cy, sy = np.cos(yz), np.sin(yz)
    for i in range(N):                                   # cos(px + yz) = cos px cos yz - sin px sin yz, float64 then rounded
        d[i] = A * (np.cos(ph * mode[0] * i) * cy - np.sin(ph * mode[0] * i) * sy)
    dev = _lib.DeviceArray(d)
    out = get_shear(dev, N, 2000.0)
    got = out.get()
    dev.free()
    out.free()
    _lib.check(_lib.lib().abacus_scratch_release())
    worst = 0.0
    for i in range(N):
        worst = max(worst, float(np.abs(got[i] - np.abs(d[i])).max()))
    print(f'single mode N = {N}: max err / A = {worst / A:.3g}')
    assert worst / A <= 1e-5


# ---------------------------------------------------------------------------------------------------- 4. get_tidal
@pytest.mark.parametrize('name', TIDAL)
def test_get_tidal_matches_the_reference(gold, name):
    from abacusutils_amd.analysis.shear import get_tidal
    dfour, karr, ref = gold[f'tidal/{name}/dfour'], gold[f'tidal/{name}/karr'], gold[f'tidal/{name}/out']
    R, e_ref = float(gold[f'tidal/{name}/R']), float(gold[f'tidal/{name}/e_ref'])
    got = get_tidal(dfour, karr, len(karr), None if R < 0 else R)
    assert got.dtype == np.complex64 and got.shape == ref.shape == (16, 16, 9, 6)
    err = np.abs(got.astype(np.complex128) - ref).max() / np.abs(ref).max()
    print(f'tidal {name}: max |got - ref| / max |ref| = {err:.3g} = {err / e_ref:.2f} e_ref')
    assert err <= 4 * e_ref
    assert not got[0].any() and not got[:, 0].any() and not got[:, :, 0].any()          # the skipped planes


# ---------------------------------------------------------------------------------------------------- 5. end to end
def test_calc_shearmark_on_the_mini_simulation(gold, tmp_path):
    """every particle of the field_rv_A / halo_rv_A fixtures (partdown = 1: the random choice is a permutation, only the order of
    the deposit differs), N = 32, against the reference's tsc_parallel + smooth_density + get_shear"""
    from abacusutils_amd.hod.prepare_sim import calc_shearmark
    ref, e_ref = gold['shear/mini32/out'], float(gold['shear/mini32/e_ref'])
    fn = str(tmp_path / 'shear_N32')
    got = calc_shearmark(str(MINI), 'Mini_N64_L32', 0.0, 32, float(gold['mini/R']), fn, partdown=1, rng=np.random.default_rng(7))
    assert got.dtype == np.float32 and got.shape == (32, 32, 32)
    assert np.array_equal(np.load(fn + '.npy'), got)
    err = np.abs(got.astype(np.float64) - ref).max() / ref.max()
    print(f'calc_shearmark mini32: max |got - ref| / max(ref) = {err:.3g} = {err / e_ref:.2f} e_ref')
    assert err <= 4 * e_ref
    # the down-sampling draws from `rng`: same seed, same field; a third of the particles, another field
    a = calc_shearmark(str(MINI), 'Mini_N64_L32', 0.0, 32, 1.5, fn, partdown=3, rng=np.random.default_rng(1))
    b = calc_shearmark(str(MINI), 'Mini_N64_L32', 0.0, 32, 1.5, fn, partdown=3, rng=np.random.default_rng(1))
    assert np.array_equal(a, b) and not np.array_equal(a, got)


@pytest.mark.parametrize('rng', ['numpy', 11])
def test_prepare_slab_arrays_takes_a_device_resident_field(rng):
    """the same shear field as a NumPy array and as a DeviceArray: identical shear_rank / halo_shear, on the host path (rng='numpy')
    and on the device path (integer seed)"""
    from abacusutils_amd import _lib, synth
    from abacusutils_amd.analysis.shear import mesh_gather
    from abacusutils_amd.hod import prepare_sim as ps
    g = load_golden('prepare_sim')
    slabs, header = synth.synth_compaso_slabs(**json.loads(str(g['meta.synth_json'])))
    field = np.random.default_rng(5).random((16, 16, 16)).astype(np.float32)
    res = []
    for f in (field, _lib.DeviceArray(field)):
        ps.reference_seed(600, 0)
        H, P, _ = ps.prepare_slab_arrays(slabs[0]['halos'], slabs[0]['parts'], header['ParticleMassHMsun'], header['H0'] / 100.0, True,
                                         want_ranks=False, want_AB=True, shearmark=f, Lbox=header['BoxSizeHMpc'], rng=rng)
        res.append((np.asarray(H['shear_rank']), np.asarray(P['halo_shear'])))
    assert len(res[0][0]) > 0 and np.ptp(res[0][0]) > 0
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    # and the gather itself, cell for cell
    idx = np.random.default_rng(3).integers(0, 16, size=(1000, 3))
    assert np.array_equal(mesh_gather(_lib.DeviceArray(field), idx), field[idx[:, 0], idx[:, 1], idx[:, 2]])


# ---------------------------------------------------------------------------------------------------- 6. scratch
def _free_bytes():
    """free device memory as the HIP runtime reports it (the runtime libabacus_hip.so is linked against)"""
    import ctypes as C

    from abacusutils_amd import _lib
    _lib.sync()
    hip = C.CDLL('libamdhip64.so')
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_scratch_is_reused_and_released():
    """calls with changing N neither pile up work meshes nor keep them after abacus_scratch_release: free device memory returns
    to what it was before the (warmed-up) series"""
    from abacusutils_amd import _lib
    from abacusutils_amd.analysis.shear import get_shear, shearmark_from_positions
    rng = np.random.default_rng(2)
    sizes = (96, 160, 128, 200, 96)
    fields = {N: rng.random((N, N, N), dtype=np.float32) for N in set(sizes)}
    pos = (rng.random((200000, 3), dtype=np.float32) * 100).astype(np.float32)

    def series():
        for N in sizes:
            get_shear(fields[N], N, 100.0)
            shearmark_from_positions(pos, N, 100.0, 1.5)
        _lib.check(_lib.lib().abacus_scratch_release())
    series()                       # warm-up: code objects, twiddle tables, the deposit's work lists
    free0 = _free_bytes()
    series()
    series()
    free1 = _free_bytes()
    print(f'free device memory before / after: {free0} / {free1}')
    assert free1 == free0
