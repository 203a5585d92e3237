"""Minkowski functionals of the smoothed density field on the MI355X: Crofton's formula on the cubic lattice (Schmalzing & Buchert
1997).  The reference has no morphological statistic; no reference code stands behind this module - its arithmetic is stated in
include/abacus_hip.h and pinned to the NumPy statement tests/minkowski_statement.py.

1. Field.  A periodic float32 mesh of n^3 cells, a = Lbox / n, N = n^3.  From particles (`calc_minkowski`): delta(k) as `get_field_fft`
   leaves it (paste, compensation and interlacing as in `calc_power`), resident in HBM in the padded layout
   (`abacus_zcv_spectrum_dev`); every mode times float32(exp(-k^2 R^2 / 2)) with dk = float32(2 pi / L), mode numbers i -> i below
   n/2, i - n from n/2 on (x, y), 0 .. n/2 on z; the C2R in place (`abacus_mf_smooth_spectrum_dev`).  The mesh is delta_R(x), mean 0.
   From a mesh (`minkowski_functionals`): `hod.zcv.ic_fields.gaussian_filter` with kcut = 1 / R, the same filter.
2. Thresholds.  T <= 64 values, finite and strictly increasing as float32.  With `sigma_units` a threshold nu stands for
   float32(nu sigma + mean), mean = sum x / N and sigma^2 = sum x^2 / N - mean^2 from the float64 sums of `abacus_mf_moments_dev`
   (two stages in a fixed order: the same bits on every run).
3. Counts (`abacus_mf_counts_dev`, one pass over the mesh for all thresholds, exact integers).  The excursion set of a threshold is
   the union of the closed voxels with value >= threshold, compared in float32, a tie inside.  n3, n2, n1, n0: its voxels, faces,
   edges and vertices; an element of the lattice belongs to it iff the maximum of the voxels that touch it (2 for a face, 4 for an
   edge, 8 for a vertex) is >= threshold.  Voxel (i, j, k) owns its cube, its three faces towards +x, +y, +z, the three edges between
   them and the vertex at (i + 1, j + 1, k + 1), all read from its 2 x 2 x 2 block with periodic indices: every element of the torus
   is counted once.
4. Functionals (host, float64):  V0 = n3 / N,  V1 = 2 (n2 - 3 n3) / (9 a N),  V2 = 2 (n1 - 2 n2 + 3 n3) / (9 a^2 N),
   V3 = (n0 - n1 + n2 - n3) / (a^3 N): the volume fraction, and the densities of surface area, integrated mean curvature and Euler
   characteristic in the normalisation in which a Gaussian field follows Tomita's curves (`gaussian_prediction`).

The mesh must be finite: a host mesh is checked, a device mesh is not (a NaN lies below every threshold, +inf above every one).

Not built: Minkowski tensors, the Koenderink-invariant estimator, masked or non-periodic meshes, light-cone fields, cross-field
morphology, multi-GPU slabs, float64 meshes.  There is no CPU fallback.
"""
import ctypes as C
import math

import numpy as np

from .. import _lib
from .._lib import DeviceArray, check, ptr

__all__ = ['minkowski_counts', 'minkowski_from_counts', 'mesh_moments', 'minkowski_functionals', 'calc_minkowski',
           'gaussian_prediction', 'MAX_THRESHOLDS']

MAX_THRESHOLDS = 64


# ------------------------------------------------------------------------------------------------- checks made before the library loads
def _thresholds(thresholds):
    """(float64 values, their float32 roundings) or ValueError; the limits of abacus_mf_counts_dev, judged the same way"""
    t = np.atleast_1d(np.asarray(thresholds, dtype=np.float64))
    if t.ndim != 1 or not 1 <= t.size <= MAX_THRESHOLDS:
        raise ValueError(f'thresholds must hold 1 .. {MAX_THRESHOLDS} values, got shape {t.shape}')
    if not np.isfinite(t).all():
        raise ValueError('the thresholds must be finite')
    with np.errstate(over='ignore'):
        t32 = t.astype(np.float32)
    if not (np.isfinite(t32).all() and (np.diff(t32) > 0).all()):
        raise ValueError('the thresholds must be finite and strictly increasing (in float32)')
    return t, np.ascontiguousarray(t32)


def _mesh(mesh):
    """the number of cells per side of a float32 (n, n, n) NumPy array or dense `DeviceArray`"""
    if not hasattr(mesh, 'shape') or not hasattr(mesh, 'dtype'):
        raise TypeError(f'the mesh must be a float32 (n, n, n) array or DeviceArray, got {type(mesh).__name__}')
    shape = tuple(mesh.shape)
    if len(shape) != 3 or len(set(shape)) != 1:
        raise ValueError(f'the mesh must be cubic, (n, n, n), got shape {shape}')
    if np.dtype(mesh.dtype) != np.float32:
        raise TypeError(f'the mesh must be float32, got {mesh.dtype}')
    if not 2 <= shape[0] <= 32767:
        raise ValueError(f'the mesh must have 2 .. 32767 cells per side, got {shape[0]}')
    if not isinstance(mesh, DeviceArray) and not np.isfinite(mesh).all():
        raise ValueError('the mesh holds values that are not finite')
    return shape[0]


def _box(Lbox):
    L = float(Lbox)
    if not (L > 0 and np.isfinite(L)):
        raise ValueError(f'Lbox must be positive, got {Lbox}')
    return L


def _radius(R, n):
    """R as a float (None: 0.0, no smoothing); smoothing goes through the half spectrum of an even mesh"""
    if R is None:
        return 0.0
    R = float(R)
    if not (R >= 0 and np.isfinite(R)):
        raise ValueError(f'R must be finite and not negative, got {R}')
    if R > 0 and n % 2:
        raise ValueError(f'nmesh = {n}: smoothing needs an even mesh (the half spectrum is laid out for one)')
    return R


# ------------------------------------------------------------------------------------------------- device calls on a resident mesh
def _up(mesh):
    """(dense DeviceArray, owned)"""
    if isinstance(mesh, DeviceArray):
        return mesh, False
    return DeviceArray(np.ascontiguousarray(mesh, dtype=np.float32)), True


def _counts(mesh_ptr, n, pitch, t32):
    out = np.empty((4, len(t32)), dtype=np.int64)
    check(_lib.lib().abacus_mf_counts_dev(mesh_ptr, n, pitch, ptr(t32), len(t32), ptr(out)))
    return out


def _moments(mesh_ptr, n, pitch):
    """(mean, variance) in float64 from the two float64 sums"""
    s = np.empty(2, dtype=np.float64)
    check(_lib.lib().abacus_mf_moments_dev(mesh_ptr, n, pitch, ptr(s)))
    N = float(n) ** 3
    mean = float(s[0]) / N
    return mean, max(float(s[1]) / N - mean * mean, 0.0)


def _in_sigma_units(nu, mean, sigma):
    """float32(nu sigma + mean), which must still increase strictly"""
    t32 = np.ascontiguousarray((nu * sigma + mean).astype(np.float32))
    if not (np.isfinite(t32).all() and (np.diff(t32) > 0).all()):
        raise ValueError(f'the thresholds nu sigma + mean do not increase strictly in float32 (sigma = {sigma:g}, mean = {mean:g})')
    return t32


def _measure(mesh_ptr, n, pitch, L, t, t32, sigma_units):
    mean, var = _moments(mesh_ptr, n, pitch)
    sigma = math.sqrt(var)
    if sigma_units:
        t32 = _in_sigma_units(t, mean, sigma)
    counts = _counts(mesh_ptr, n, pitch, t32)
    return dict(V=minkowski_from_counts(counts, n, L), counts=counts, thresholds=t32, mean=mean, sigma=sigma)


# ------------------------------------------------------------------------------------------------- the public interface
def minkowski_counts(mesh, thresholds):
    """int64 (4, T): the rows n0, n1, n2, n3 (vertices, edges, faces, voxels of the excursion sets, step 3 of the module docstring)
    for the thresholds as given (rounded to float32).  `mesh`: a float32 (n, n, n) NumPy array (checked to be finite) or a dense
    `DeviceArray`; not modified."""
    _, t32 = _thresholds(thresholds)
    n = _mesh(mesh)
    dev, owned = _up(mesh)
    try:
        return _counts(dev.ptr, n, n, t32)
    finally:
        if owned:
            dev.free()


def minkowski_from_counts(counts, n, Lbox):
    """float64 (4, T): V0 .. V3 from the counts (rows n0, n1, n2, n3) of a mesh of n cells per side in a box of side Lbox: step 4 of
    the module docstring.  Host only."""
    c = np.asarray(counts)
    if c.ndim != 2 or c.shape[0] != 4:
        raise ValueError(f'counts must have shape (4, T), got {c.shape}')
    n, L = int(n), _box(Lbox)
    if n < 1:
        raise ValueError(f'n must be positive, got {n}')
    n0, n1, n2, n3 = c.astype(np.float64)
    N, a = float(n) ** 3, L / n
    return np.stack([n3 / N, 2.0 * (n2 - 3.0 * n3) / (9.0 * a * N), 2.0 * (n1 - 2.0 * n2 + 3.0 * n3) / (9.0 * a**2 * N),
                     (n0 - n1 + n2 - n3) / (a**3 * N)])


def mesh_moments(mesh):
    """(mean, variance) of the n^3 cells in float64, from float64 sums of x and x^2 taken in a fixed order on the device"""
    n = _mesh(mesh)
    dev, owned = _up(mesh)
    try:
        return _moments(dev.ptr, n, n)
    finally:
        if owned:
            dev.free()


def minkowski_functionals(mesh, Lbox, thresholds, R=None, sigma_units=False):
    """The four functionals of a periodic mesh at the thresholds.  `R` (units of Lbox; None or 0: none) smooths the mesh first with
    `hod.zcv.ic_fields.gaussian_filter` at kcut = 1 / R; with `sigma_units` the thresholds are nu and stand for nu sigma + mean of
    the (smoothed) mesh.  `mesh` is not modified.

    Returns dict(V (4, T) float64, counts (4, T) int64, thresholds (T,) the float32 values used, mean, sigma)."""
    t, t32 = _thresholds(thresholds)
    n, L = _mesh(mesh), _box(Lbox)
    R = _radius(R, n)
    dev, owned = _up(mesh)
    try:
        if R > 0:
            from ..hod.zcv.ic_fields import gaussian_filter
            smooth = gaussian_filter(dev, n, L, 1.0 / R)         # a new device mesh: the caller's is left alone
            if owned:
                dev.free()
            dev, owned = smooth, True
        return _measure(dev.ptr, n, n, L, t, t32, sigma_units)
    finally:
        if owned:
            dev.free()


def calc_minkowski(pos, Lbox, thresholds, R, nmesh=256, w=None, paste='TSC', compensated=True, interlaced=True, sigma_units=True,
                   return_field=False):
    """The four functionals of the density contrast of the particles `pos` in the periodic box of side `Lbox`, smoothed with a
    Gaussian of radius `R` (units of Lbox; 0: none): steps 1 to 4 of the module docstring.  The mesh stays in HBM.

    `pos`: (N, 3) NumPy float32 / float64, an (N, 3) float32 `DeviceArray`, or three float64 `DeviceArray` columns
    (`MockDict.device_xyz`); not modified - the deposit works on a wrapped float32 copy.  `w`: per-particle weights or None.
    `thresholds`: nu in units of sigma around the mean with `sigma_units`, else values of delta_R.

    Returns dict(V (4, T) float64, counts (4, T) int64, thresholds (T,) the float32 values used, mean, sigma) and, with
    `return_field`, field: the (n, n, n) float32 mesh the counts were taken on."""
    from ..hod.zcv.reconstruction import _positions, _working_copy
    from .power_spectrum import _paste_code, get_W_compensated
    t, t32 = _thresholds(thresholds)
    n, L = int(nmesh), _box(Lbox)
    if n < 2 or n % 2 or n > 32767:
        raise ValueError(f'nmesh = {n}: the functionals of particles need an even mesh of 2 .. 32766 cells per side')
    if R is None:
        raise ValueError('R must be given (0: no smoothing)')
    R = _radius(R, n)
    code = _paste_code(paste, ':')
    npart = _positions(pos, 'pos')
    if w is not None:
        w = np.ascontiguousarray(w, dtype=np.float32)
        if w.shape != (npart,):
            raise ValueError(f'the weights have shape {w.shape}, expected ({npart},)')
    W = np.ascontiguousarray(get_W_compensated(L, n, paste, bool(interlaced)), dtype=np.float32) if compensated else None
    lib = _lib.lib()
    check(lib.abacus_mf_check_memory(n, C.c_int64(npart)))
    spec = work = wdev = None
    try:
        nb = C.c_uint64(0)
        check(lib.abacus_zcv_spectrum_bytes(n, C.byref(nb)))
        pitch = int(lib.abacus_slab_pitch(n))
        spec = DeviceArray(nbytes=nb.value, dtype=np.float32, shape=(n, n, pitch))
        work = _working_copy(pos, npart, 0.0, L)
        wdev = None if w is None else DeviceArray(w)
        check(lib.abacus_zcv_spectrum_dev(work.ptr, C.c_int64(npart), None if wdev is None else wdev.ptr, C.c_double(L), n, code, ptr(W),
                                          int(bool(interlaced)), spec.ptr))
        _lib.sync()
        work.free()
        work = None
        check(lib.abacus_mf_smooth_spectrum_dev(spec.ptr, n, C.c_double(L), C.c_double(R)))
        out = _measure(spec.ptr, n, pitch, L, t, t32, sigma_units)
        if return_field:
            out['field'] = np.ascontiguousarray(spec.get()[:, :, :n])
        return out
    finally:
        for a in (spec, work, wdev):
            if a is not None:
                a.free()


def gaussian_prediction(nu, lam):
    """float64 (4, T): Tomita's curves V0 .. V3 of a Gaussian random field at the thresholds nu (units of sigma), with
    lam = sqrt(sigma1^2 / (6 pi sigma0^2)), sigma0^2 the variance of the field and sigma1^2 that of its gradient (lam is an
    inverse length in the units of Lbox):  V0 = erfc(nu / sqrt 2) / 2,  V1 = (2 / 3) lam g,  V2 = (2 / 3) lam^2 nu g,
    V3 = lam^3 (nu^2 - 1) g with g = exp(-nu^2 / 2) / sqrt(2 pi).  Host only."""
    nu = np.atleast_1d(np.asarray(nu, dtype=np.float64))
    lam = float(lam)
    g = np.exp(-0.5 * nu * nu) / math.sqrt(2.0 * math.pi)
    V0 = np.array([0.5 * math.erfc(x / math.sqrt(2.0)) for x in nu])
    return np.stack([V0, 2.0 / 3.0 * lam * g, 2.0 / 3.0 * lam**2 * nu * g, lam**3 * (nu * nu - 1.0) * g])
