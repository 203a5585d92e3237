"""MI355X drop-in for `abacusnbody.analysis.shear` (reference: abacusnbody/analysis/shear.py).

`smooth_density`, `get_tidal`, `get_shear_nb` and `get_shear` keep the reference's names, argument order and defaults.  The work
runs on the GPU (csrc/shear.hip): the Gaussian filter as three separable passes with SciPy's `reflect` boundary, the tidal
tensor in Fourier space, six inverse transforms and the shear `sqrt(((l2-l1)^2 + (l3-l1)^2 + (l3-l2)^2) / 2)` from the traceless
tensor as `sqrt(1.5 tr(S^2))` (no eigen-solver, no cancellation).  NumPy arrays in give NumPy arrays out; a `DeviceArray` in gives a
`DeviceArray` out and nothing crosses PCIe.  Nothing is printed.  There is no CPU fallback.

`shearmark_from_positions` is the device part of `prepare_sim.calc_shearmark`: deposit, smoothing and shear in one call.
"""
import ctypes as C

import numpy as np

from .. import _lib
from .._lib import DeviceArray, check, ptr

__all__ = ['smooth_density', 'get_tidal', 'get_shear_nb', 'get_shear', 'shearmark_from_positions', 'gaussian_weights', 'mesh_gather']


def gaussian_weights(sigma, truncate=4.0):
    """(radius, w): scipy.ndimage's Gaussian kernel for `sigma` cells, radius = int(truncate * sigma + 0.5), float64 weights
    exp(-x^2 / (2 sigma^2)) normalised to sum 1 over the 2 radius + 1 taps; w[k] is the weight at distance k from the centre"""
    sigma = float(sigma)
    radius = int(truncate * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return radius, np.ascontiguousarray(phi[radius:], dtype=np.float64)


def _cube(a, name, N_dim=None):
    """shape / dtype checks shared by the entry points, made before the library is loaded"""
    shape = tuple(a.shape)
    if len(shape) != 3 or len(set(shape)) != 1:
        raise ValueError(f'{name} must be a cubic 3-D mesh, got shape {shape}')
    if N_dim is not None and shape[0] != int(N_dim):
        raise ValueError(f'{name} has {shape[0]} cells per side, N_dim = {N_dim}')
    if np.dtype(a.dtype).kind not in 'fiu':
        raise TypeError(f'{name} must be a real array, got dtype {a.dtype}')
    return shape[0]


def _to_device_f32(a):
    """(DeviceArray float32, owned): uploads a NumPy array; a float32 DeviceArray is used as it is"""
    if isinstance(a, DeviceArray):
        if a.dtype != np.float32:
            raise TypeError(f'a DeviceArray mesh must be float32, got {a.dtype}')
        return a, False
    return DeviceArray(np.ascontiguousarray(a, dtype=np.float32)), True


def smooth_density(D, R, N_dim, Lbox):
    """Gaussian smoothing of the mesh `D` with scale `R` (same length units as `Lbox`): scipy.ndimage.gaussian_filter(D, R / cell)
    with SciPy's defaults (truncate 4, boundary 'reflect').  `D` is not modified.  Returns float32 (SciPy keeps the dtype of `D`;
    the meshes of this package are float32)."""
    n = _cube(D, 'D', N_dim)
    if not isinstance(D, DeviceArray) and np.dtype(D.dtype) != np.float32:
        raise TypeError(f'D must be float32 (the dtype of the meshes tsc_parallel returns), got {D.dtype}')
    sigma = float(R) / (float(Lbox) / N_dim)
    src, owned = _to_device_f32(D)
    if owned:
        out = src
    else:
        out = DeviceArray(nbytes=src.nbytes, dtype=np.float32, shape=src.shape)
        check(_lib.lib().abacus_memcpy_d2d(out.ptr, src.ptr, C.c_uint64(src.nbytes)))
    if sigma > 1e-15:                                # (scipy skips an axis with sigma <= 1e-15)
        radius, w = gaussian_weights(sigma)
        tmp = DeviceArray(nbytes=out.nbytes, dtype=np.float32, shape=out.shape)
        check(_lib.lib().abacus_gauss_smooth_dev(out.ptr, tmp.ptr, int(n), ptr(w), int(radius)))
        _lib.sync()
        tmp.free()
    if owned:
        res = out.get()
        out.free()
        return res
    return out


def get_tidal(dfour, karr, N_dim, R, dtype=np.float32):
    """The six components k_i k_j / k^2 * dfour of the tidal tensor in Fourier space, (N, N, N/2+1, 6) complex64 in the order
    xx, xy, xz, yy, yz, zz; modes with a zero index on any axis stay 0 (reference :47).  `R` not None: times the top-hat window."""
    N_dim = int(N_dim)
    kz = N_dim // 2 + 1
    if tuple(dfour.shape) != (N_dim, N_dim, kz):
        raise ValueError(f'dfour must have shape {(N_dim, N_dim, kz)}, got {tuple(dfour.shape)}')
    karr = np.ascontiguousarray(karr, dtype=np.float32)
    if karr.shape != (N_dim,):
        raise ValueError(f'karr must hold {N_dim} wavenumbers')
    on_device = isinstance(dfour, DeviceArray)
    if on_device and dfour.dtype != np.complex64:
        raise TypeError('a DeviceArray spectrum must be complex64')
    d = dfour if on_device else DeviceArray(np.ascontiguousarray(dfour, dtype=np.complex64))
    k = DeviceArray(karr)
    out = DeviceArray(nbytes=N_dim * N_dim * kz * 6 * 8, dtype=np.complex64, shape=(N_dim, N_dim, kz, 6))
    check(_lib.lib().abacus_tidal_dev(d.ptr, k.ptr, N_dim, C.c_double(-1.0 if R is None else float(R)), out.ptr))
    _lib.sync()
    k.free()
    if on_device:
        return out
    d.free()
    res = out.get()
    out.free()
    return res


def _shear_from_components(t):
    """sqrt(1.5 tr(S^2)) of the traceless part of the symmetric tensors t[..., 6] (xx, xy, xz, yy, yz, zz)"""
    t = np.asarray(t, dtype=np.float32)
    third = (t[..., 0] + t[..., 3] + t[..., 5]) / np.float32(3)
    q = (t[..., 0] - third) ** 2 + (t[..., 3] - third) ** 2 + (t[..., 5] - third) ** 2
    q = q + np.float32(2) * (t[..., 1] ** 2 + t[..., 2] ** 2 + t[..., 4] ** 2)
    return np.sqrt(np.float32(1.5) * q).astype(np.float32)


def get_shear_nb(tidr, N_dim):
    """Shear of a real-space tidal tensor `tidr` (N, N, N, 6), reference :69-93.  Kept so that imports keep working: the device
    chain (`get_shear`) never materialises the six meshes this takes; the formula is evaluated with array operations."""
    N_dim = int(N_dim)
    if tuple(np.shape(tidr)) != (N_dim, N_dim, N_dim, 6):
        raise ValueError(f'tidr must have shape {(N_dim, N_dim, N_dim, 6)}')
    return _shear_from_components(tidr)


def get_shear(dsmo, N_dim, Lbox, R=None, dtype=np.float32):
    """The shear field of the (smoothed) density mesh `dsmo` - an array, a DeviceArray or the path of a `.npy` file -, (N, N, N)
    float32.  `R` not None applies the top-hat window of that radius to the tidal tensor.  Only `dtype=np.float32` is built."""
    N_dim = int(N_dim)
    if N_dim % 2:
        raise ValueError(f'N_dim = {N_dim} is odd: the reference fails there (irfftn returns N - 1 cells); use an even mesh')
    if np.dtype(dtype) != np.float32:
        raise TypeError('get_shear is built for dtype=np.float32 (the reference\'s default)')
    if isinstance(dsmo, str):
        dsmo = np.load(dsmo)
    _cube(dsmo, 'dsmo', N_dim)
    src, owned = _to_device_f32(dsmo)
    out = DeviceArray(nbytes=src.nbytes, dtype=np.float32, shape=src.shape)
    check(_lib.lib().abacus_shear_dev(src.ptr, out.ptr, N_dim, C.c_double(float(Lbox)), C.c_double(-1.0 if R is None else float(R))))
    _lib.sync()
    if not owned:
        return out
    src.free()
    res = out.get()
    out.free()
    return res


def shearmark_from_positions(pos, N_dim, Lbox, R, device_out=False):
    """calc_shearmark's compute chain (hod/prepare_sim.py:1113-1123) in one device call: TSC counts of `pos` (n, 3) float32 on an
    N_dim^3 mesh, Gaussian smoothing with scale `R`, shear with R = None.  `pos` (NumPy or DeviceArray) is not modified."""
    N_dim = int(N_dim)
    if N_dim % 2:
        raise ValueError(f'N_dim = {N_dim} is odd: the reference fails there (irfftn returns N - 1 cells); use an even mesh')
    if len(pos.shape) != 2 or pos.shape[1] != 3:
        raise ValueError('pos must have shape (n, 3)')
    if np.dtype(pos.dtype) != np.float32:
        raise TypeError(f'pos must be float32, got {pos.dtype}')
    n = int(pos.shape[0])
    if n < 1:
        raise ValueError('no particles')
    p = pos if isinstance(pos, DeviceArray) else DeviceArray(np.ascontiguousarray(pos))
    out = DeviceArray(nbytes=4 * N_dim ** 3, dtype=np.float32, shape=(N_dim,) * 3)
    sigma = float(R) / (float(Lbox) / N_dim)
    check(_lib.lib().abacus_shearmark_dev(p.ptr, C.c_int64(n), N_dim, C.c_double(float(Lbox)), C.c_double(sigma), out.ptr))
    _lib.sync()
    if p is not pos:
        p.free()
    if device_out:
        return out
    res = out.get()
    out.free()
    return res


def mesh_gather(mesh, g):
    """mesh[g[:, 0], g[:, 1], g[:, 2]] of a float32 DeviceArray mesh (n, n, n) for host cell indices g (nh, 3): float32 NumPy array"""
    n = _cube(mesh, 'mesh')
    if mesh.dtype != np.float32:
        raise TypeError('the mesh must be float32')
    g = np.ascontiguousarray(g, dtype=np.int64)
    if g.ndim != 2 or g.shape[1] != 3:
        raise ValueError('g must have shape (nh, 3)')
    nh = len(g)
    if nh == 0:
        return np.empty(0, dtype=np.float32)
    if g.min() < 0 or g.max() >= n:
        raise IndexError('cell index outside the mesh')
    gd = DeviceArray(g)
    od = DeviceArray(nbytes=4 * nh, dtype=np.float32, shape=(nh,))
    check(_lib.lib().abacus_mesh_gather_dev(mesh.ptr, int(n), gd.ptr, C.c_int64(nh), od.ptr))
    res = od.get()
    gd.free()
    od.free()
    return res
