"""MI355X drop-in for the array side of `abacusnbody.hod.zcv.ic_fields` (reference: abacusnbody/hod/zcv/ic_fields.py).

`gaussian_filter`, `filter_field`, `get_n2_fft`, `get_sij_fft`, `add_ij`, `get_dk_to_s2`, `get_dk_to_n2` and `get_fields` keep the
reference's names, argument order and defaults.  The work runs on the GPU (csrc/zcv.hip); `gaussian_filter` and `get_fields` are one
device call each: one upload, the whole chain (R2C, spectral multipliers, C2R rounds, accumulation, deterministic float64 means) in
HBM.  NumPy arrays in give NumPy arrays out; a `DeviceArray` in gives a `DeviceArray` out and nothing crosses PCIe.  Nothing is
printed.  There is no CPU fallback.  Only `dtype=np.float32` is built.  Spectra are un-normalised `rfftn` output, complex64
`(n, n, n//2+1)`; the `1/n^3` comes with the inverse transform, as with `irfftn`.

The file side of the reference module (`compress_asdf`, `load_dens`, `load_disp`, `main`) is not built.

Wavenumbers are the reference's: `dk = float32(2 pi / L)`, index `i -> i` below `n//2` and `i - n` from there on (x, y; the Nyquist
index is negative), `0 .. n//2` on z.  With that the `s_ij` spectra are not Hermitian on the planes `c = 0` and `c = n//2`; the
reference's `irfftn` uses the Hermitian part of those planes and so does the device chain (written out in its multiplier kernel).
"""
import ctypes as C

import numpy as np

from ... import _lib
from ..._lib import DeviceArray, check

__all__ = ['gaussian_filter', 'filter_field', 'get_n2_fft', 'get_sij_fft', 'add_ij', 'get_dk_to_s2', 'get_dk_to_n2', 'get_fields']

_OP_FILTER, _OP_N2, _OP_SIJ = 0, 1, 2


def _f32_only(dtype, who):
    if np.dtype(dtype) != np.float32:
        raise TypeError(f'{who} is built for dtype=np.float32 (the reference\'s default)')


def _even(n, who):
    n = int(n)
    if n < 2:
        raise ValueError(f'{who}: mesh size {n} out of range')
    if n % 2:
        raise ValueError(f'{who}: nmesh = {n} is odd: the reference fails there (irfftn returns n - 1 cells along z and add_ij '
                         'indexes past it); use an even mesh')
    return n


def _positive(x, name):
    x = float(x)
    if not x > 0:
        raise ValueError(f'{name} must be positive, got {x}')
    return x


def _mesh(a, name, n=None):
    """shape / dtype checks of a real mesh, made before the library is loaded; returns the mesh size"""
    shape = tuple(a.shape)
    if len(shape) != 3 or len(set(shape)) != 1:
        raise ValueError(f'{name} must be a cubic 3-D mesh, got shape {shape}')
    if n is not None and shape[0] != int(n):
        raise ValueError(f'{name} has {shape[0]} cells per side, nmesh = {n}')
    if isinstance(a, DeviceArray):
        if a.dtype != np.float32:
            raise TypeError(f'a DeviceArray mesh must be float32, got {a.dtype}')
    elif np.dtype(a.dtype).kind not in 'fiu':
        raise TypeError(f'{name} must be a real array, got dtype {a.dtype}')
    return shape[0]


def _spectrum(a, name, n):
    n = int(n)
    want = (n, n, n // 2 + 1)
    if tuple(a.shape) != want:
        raise ValueError(f'{name} must have the rfftn shape {want}, got {tuple(a.shape)}')
    if isinstance(a, DeviceArray):
        if a.dtype != np.complex64:
            raise TypeError(f'a DeviceArray spectrum must be complex64, got {a.dtype}')
    elif np.dtype(a.dtype).kind not in 'cfiu':
        raise TypeError(f'{name} must be a numeric array, got dtype {a.dtype}')


def _up_f32(a):
    """(DeviceArray float32, owned)"""
    if isinstance(a, DeviceArray):
        return a, False
    return DeviceArray(np.ascontiguousarray(a, dtype=np.float32)), True


def _up_c64(a):
    if isinstance(a, DeviceArray):
        return a, False
    return DeviceArray(np.ascontiguousarray(a, dtype=np.complex64)), True


def _new_mesh(n):
    return DeviceArray(nbytes=4 * n ** 3, dtype=np.float32, shape=(n, n, n))


def _down(dev, on_device):
    if on_device:
        return dev
    res = dev.get()
    dev.free()
    return res


def gaussian_filter(field, nmesh, lbox, kcut):
    """`field` times exp(-k^2 / (2 kcut^2)) in Fourier space (reference :79-107): float32 (nmesh, nmesh, nmesh).  `field` is not
    modified.  One device call: R2C, multiplier, C2R."""
    n = _even(nmesh, 'gaussian_filter')
    _mesh(field, 'field', n)
    lbox, kcut = _positive(lbox, 'lbox'), _positive(kcut, 'kcut')
    src, owned = _up_f32(field)
    out = src if owned else _new_mesh(n)
    check(_lib.lib().abacus_zcv_filter_dev(src.ptr, out.ptr, n, C.c_double(lbox), C.c_double(kcut)))
    _lib.sync()
    return _down(out, not owned)


def _spectral(op, delta_k, n1d, L, i_comp=0, j_comp=0, kcut=1.0, inplace=False):
    L = _positive(L, 'L')
    n = int(n1d)
    src, owned = _up_c64(delta_k)
    dst = src if (inplace or owned) else DeviceArray(nbytes=src.nbytes, dtype=np.complex64, shape=src.shape)
    check(_lib.lib().abacus_zcv_spectral_dev(src.ptr, dst.ptr, n, C.c_double(L), op, int(i_comp), int(j_comp), C.c_double(float(kcut))))
    _lib.sync()
    return _down(dst, not owned)


def filter_field(delta_k, n1d, L, kcut, dtype=np.float32):
    """exp(-k^2 / (2 kcut^2)) * delta_k (reference :110-148).  Like the reference it works IN PLACE and returns its argument: a
    complex64 C-contiguous NumPy array or a DeviceArray is overwritten; any other array is converted first and the result returned."""
    _f32_only(dtype, 'filter_field')
    _spectrum(delta_k, 'delta_k', n1d)
    kcut = _positive(kcut, 'kcut')
    res = _spectral(_OP_FILTER, delta_k, n1d, L, kcut=kcut, inplace=True)
    if isinstance(delta_k, DeviceArray):
        return delta_k
    if delta_k.dtype == np.complex64 and delta_k.flags.c_contiguous and delta_k.flags.writeable:
        delta_k[...] = res
        return delta_k
    return res


def get_n2_fft(delta_k, n1d, L, dtype=np.float32):
    """-k^2 delta_k (reference :151-189)"""
    _f32_only(dtype, 'get_n2_fft')
    _spectrum(delta_k, 'delta_k', n1d)
    return _spectral(_OP_N2, delta_k, n1d, L)


def get_sij_fft(i_comp, j_comp, delta_k, n1d, L, dtype=np.float32):
    """(k_i k_j / k^2 - delta_ij / 3) delta_k (reference :192-255); the zero vector gives -delta_ij / 3 * delta_k.  Returned as
    the reference returns it, that is not Hermitian on the planes c = 0 and c = n1d // 2 (see the module docstring)."""
    _f32_only(dtype, 'get_sij_fft')
    if int(i_comp) not in (0, 1, 2) or int(j_comp) not in (0, 1, 2):
        raise ValueError(f'tensor component ({i_comp}, {j_comp}) out of range')
    _spectrum(delta_k, 'delta_k', n1d)
    return _spectral(_OP_SIJ, delta_k, n1d, L, i_comp, j_comp)


def add_ij(final_field, field_to_add, n1d, factor=1.0, dtype=np.float32):
    """final_field += factor * field_to_add**2, in place (reference :258-268); returns None like the reference.  `final_field`: a
    float32 DeviceArray or a float32 C-contiguous NumPy array."""
    _f32_only(dtype, 'add_ij')
    n = _mesh(final_field, 'final_field', n1d)
    _mesh(field_to_add, 'field_to_add', n)
    if not isinstance(final_field, DeviceArray) and not (final_field.dtype == np.float32 and final_field.flags.c_contiguous
                                                         and final_field.flags.writeable):
        raise TypeError('final_field is updated in place: it must be a writeable C-contiguous float32 array')
    fin, fin_owned = _up_f32(final_field)
    add, add_owned = _up_f32(field_to_add)
    check(_lib.lib().abacus_zcv_add_ij_dev(fin.ptr, add.ptr, n, C.c_double(float(factor))))
    _lib.sync()
    if add_owned:
        add.free()
    if fin_owned:
        final_field[...] = fin.get()
        fin.free()


def _dk_to(which, delta_k, nmesh, lbox, who):
    n = _even(nmesh, who)
    _spectrum(delta_k, 'delta_k', n)
    lbox = _positive(lbox, 'lbox')
    src, owned = _up_c64(delta_k)
    out = _new_mesh(n)
    check(_lib.lib().abacus_zcv_dk_to_dev(src.ptr, n, C.c_double(lbox), which, out.ptr))
    _lib.sync()
    if owned:
        src.free()
    return _down(out, not owned)


def get_dk_to_s2(delta_k, nmesh, lbox):
    """s^2 = s_ij s_ij with s_ij = (k_i k_j / k^2 - delta_ij / 3) delta_k (reference :271-309): six multiplier + C2R + accumulate
    rounds in one device call; float32 (nmesh, nmesh, nmesh)"""
    return _dk_to(0, delta_k, nmesh, lbox, 'get_dk_to_s2')


def get_dk_to_n2(delta_k, nmesh, lbox):
    """nabla^2 delta = IFFT(-k^2 delta_k) (reference :312-333); float32 (nmesh, nmesh, nmesh)"""
    return _dk_to(1, delta_k, nmesh, lbox, 'get_dk_to_n2')


def get_fields(delta_lin, Lbox, nmesh):
    """(d, d2, s2, n2) = (delta - mean, delta^2 - mean, s_ij s_ij - mean, nabla^2 delta) of the linear density mesh (reference
    :336-366) in ONE device call: one R2C, seven multiplier + C2R rounds, the three mean subtractions.  The means are two-stage
    float64 sums in a fixed order: the same bits on every run.  `delta_lin` is not modified."""
    n = _even(nmesh, 'get_fields')
    _mesh(delta_lin, 'delta_lin', n)
    Lbox = _positive(Lbox, 'Lbox')
    src, owned = _up_f32(delta_lin)
    d = src if owned else _new_mesh(n)
    d2, s2, n2 = _new_mesh(n), _new_mesh(n), _new_mesh(n)
    check(_lib.lib().abacus_zcv_fields_dev(src.ptr, n, C.c_double(Lbox), d.ptr, d2.ptr, s2.ptr, n2.ptr))
    _lib.sync()
    return tuple(_down(a, not owned) for a in (d, d2, s2, n2))
