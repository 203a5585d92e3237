"""The mesh families take turns on the ONE cache of in-place hipFFT plans (csrc/mesh.hip: two sizes per direction, behind
`r2c_inplace` / `c2r_inplace` of csrc/mesh_common.hpp), in one process.  Needs an MI355X: run with `-m gpu`.

The families live in translation units of their own (shear.hip, zcv.hip, lcv.hip, recon.hip, lc_power.hip, bispectrum.hip,
minkowski.hip, voids.hip, wst.hip).  Whatever the family before left behind - a plan of another size, a plan bound to work areas
that were given back, scratch blocks of another size - must not reach the next one: every result of the interleaved series is
the SAME BITS as the same call made alone, right after abacus_scratch_release().

n = 16 and n = 24 both have rows of 32 floats while the transform uses n + 2 = 18 and 26 of them: the pad columns are live.  The
series alternates the two sizes with the families rotating through them, so both entries of a direction are in use; one call at
n = 12 in the middle pushes a third size through, after which one of the two is made again.  All of it runs with the native R2C
and with the option fft_hipfft, where the R2C comes from the cache as well."""
import numpy as np
import pytest
from test_shear_gpu import _free_bytes      # free device memory, as test_scratch_is_reused_and_released reads it

pytestmark = pytest.mark.gpu

SIZES = (16, 24)
THIRD = 12
LBOX = 200.0
NPART = 4000


def _inputs():
    rng = np.random.default_rng(20240521)
    fields = {n: rng.standard_normal((n, n, n)).astype(np.float32) for n in SIZES + (THIRD,)}
    spectra = {n: (np.fft.rfftn(fields[n].astype(np.float64)) / n ** 3).astype(np.complex64) for n in SIZES}
    pos = (rng.random((NPART, 3)) * LBOX).astype(np.float32)
    # a light cone seen from the origin: randoms in a cube well off it, the data every third of them
    cone = (100.0 + rng.random((NPART, 3)) * 100.0).astype(np.float32)
    return fields, spectra, pos, cone


def _families(fields, spectra, pos, cone):
    """name -> f(n): a tuple of arrays, every one of them the output of a chain that transforms through the shared cache"""
    from abacusutils_amd.analysis.bispectrum import calc_bispectrum
    from abacusutils_amd.analysis.lc_power import LCRandoms, fkp_field
    from abacusutils_amd.analysis.minkowski import calc_minkowski
    from abacusutils_amd.analysis.shear import get_shear
    from abacusutils_amd.analysis.voids import tophat_smooth
    from abacusutils_amd.analysis.wst import wst_modulus
    from abacusutils_amd.hod.zcv.ic_fields import get_fields
    from abacusutils_amd.hod.zcv.linear_fields import linear_fields
    from abacusutils_amd.hod.zcv.reconstruction import displacement_field

    def shear(n):
        return (np.asarray(get_shear(fields[n], n, LBOX)),)

    def zcv(n):
        return tuple(np.asarray(a) for a in get_fields(fields[n], LBOX, n))

    def lcv(n):
        with linear_fields(fields[n], LBOX, n) as lin:
            return lin.spectrum('delta'), lin.spectrum('deltamu2')

    def recon(n):
        with displacement_field(pos, LBOX, n, 1.8, 0.8, 10.0) as disp:
            return tuple(np.asarray(a) for a in disp.fetch())

    def lc_power(n):
        randoms = LCRandoms(*cone.T.copy())
        with fkp_field(*cone[::3].T.copy(), randoms, n, boxpad=1.6) as f:      # two cells of margin at n = 16: 1 / (1 - 4 / 16) and some
            return (f.spectrum(2),)

    def bispectrum(n):
        dk = 2 * np.pi / LBOX
        got = calc_bispectrum(pos, LBOX, np.linspace(dk, 0.98 * dk * n / 3.0, 4), nmesh=n)
        return got['B'], got['P']

    def minkowski(n):
        got = calc_minkowski(pos, LBOX, (-1.0, 0.0, 1.0), 12.0, nmesh=n, return_field=True)
        return got['field'], got['counts']

    def voids(n):
        return (tophat_smooth(spectra[n], LBOX, 20.0),)

    def wst(n):
        return (wst_modulus(fields[n], 1.5, 1),)

    return dict(shear=shear, zcv=zcv, lcv=lcv, recon=recon, lc_power=lc_power, bispectrum=bispectrum, minkowski=minkowski, voids=voids,
                wst=wst)


def _same_bits(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_nine_families_take_turns_on_one_plan_cache():
    from abacusutils_amd import _lib
    from abacusutils_amd.analysis.shear import get_shear
    fields, spectra, pos, cone = _inputs()
    fam = _families(fields, spectra, pos, cone)
    names = list(fam)
    assert len(names) % 2 == 1         # an odd count: alternating the sizes gives every family both of them in two rounds

    def release():
        _lib.check(_lib.lib().abacus_scratch_release())

    def third():
        return (np.asarray(get_shear(fields[THIRD], THIRD, LBOX)),)

    before = _lib.get_option('fft_hipfft')
    try:
        # every call alone (this is the warm-up of the memory check as well: code objects, twiddle tables, the triangle counts)
        alone = {}
        for hipfft in (0, 1):
            _lib.set_option('fft_hipfft', hipfft)
            for name in names:
                for n in SIZES:
                    release()
                    alone[hipfft, name, n] = fam[name](n)
                    assert all(np.any(np.nan_to_num(a) != 0) for a in alone[hipfft, name, n]), (hipfft, name, n)
            release()
            alone[hipfft, 'third', THIRD] = third()
        for name in names:             # the two sizes are two different problems
            assert not _same_bits(alone[0, name, 16], alone[0, name, 24]), name
        release()
        free0 = _free_bytes()

        for hipfft in (0, 1):
            _lib.set_option('fft_hipfft', hipfft)
            for step in range(2 * len(names)):         # sizes 16, 24, 16, 24, 16, ... with the families rotating
                name, n = names[step % len(names)], SIZES[step % 2]
                assert _same_bits(fam[name](n), alone[hipfft, name, n]), f'fft_hipfft={hipfft} step {step}: {name} at n={n}'
                if step == len(names):                 # a third size between a 24 and a 16: one of the two has to go
                    assert _same_bits(third(), alone[hipfft, 'third', THIRD]), f'fft_hipfft={hipfft}: shear at n={THIRD}'
        release()
        free1 = _free_bytes()
    finally:
        _lib.set_option('fft_hipfft', before)
    print(f'free device memory before / after: {free0} / {free1}')
    assert free1 == free0
