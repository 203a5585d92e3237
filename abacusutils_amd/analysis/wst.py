"""Solid-harmonic wavelet scattering transform (WST) of the density field on the MI355X: the coefficients S0, S1, S2 of Eickenberg et
al. (2018) as used on AbacusSummit mocks by Valogiannis & Dvorkin (2022) and Valogiannis, Yuan & Dvorkin (2023).  The reference has no
such statistic; no reference code stands behind this module - its arithmetic is stated in include/abacus_hip.h and pinned to the
NumPy statement tests/wst_statement.py.

Mesh of n^3 cells, n even, N = n^3; everything stays in HBM as periodic float32 meshes.

1. Field.  rho^(k): the padded half spectrum as `abacus_zcv_spectrum_dev` leaves it (delta(k) / N; paste, compensation and interlacing
   as in `calc_power`), its mode k = 0 set to 1 (rho = 1 + delta) or, with `contrast`, to 0.
2. Mode numbers.  Index i -> i below n/2, i - n from n/2 on (x, y); 0 .. n/2 on z.
3. Scales.  sigma_j = sigma0 2^j cells, j = 0 .. J - 1.  With kappa = (2 pi / n) sqrt(i^2 + j^2 + l^2) the radial profile is
   g_{j,l}(kappa) = (sigma_j kappa)^l exp(-sigma_j^2 kappa^2 / 2), l = 0 .. L: float64, rounded once to float32, tabulated over the
   integer i^2 + j^2 + l^2.
4. Harmonics.  S_lm(k^), m = 1 .. 2 l + 1: the real harmonics scaled so that sum_m S_lm(a) S_lm(b) = P_l(a . b), polynomials of the
   unit vector formed in float32 from the mode numbers.
5. Multiplier of a mode.  g S_lm for even l; i g S_lm for odd l, (re, im) -> (-im, re).  For l > 0 it is exactly 0 at k = 0 and on
   every mode with a mode number n/2 in any axis: the stored mode stands for +-n/2 and S_lm differs on the two, so only with the zeros
   is the product Hermitian and its C2R defined.
6. First order.  U1[j, l](x) = sqrt(sum_m (C2R[multiplier_{j,l,m} rho^](x))^2), the C2R without normalisation.
7. Second order, the same l and j1 < j2 only.  U^ = R2C(U1[j1, l]) / N; U2[j1, j2, l] is step 6 on U^ at scale j2.
8. Coefficients, for Q exponents q.  S0[q] = <|rho|^q>, S1[j, l, q] = <U1^q>, S2[j1, j2, l, q] = <U2^q>: means over the N cells of
   pow((double)u, q) of the float32 cell, summed in float64 in two stages of a fixed order - every run gives the same bits.

Limits: 1 <= J <= 8, 0 <= L <= 4, 1 <= Q <= 8, 0 < q <= 8, sigma0 > 0, all finite; n even, 4 .. 32766.  A scale is useful while
sigma_j stays below about n / 6; larger ones are computed as asked.

Not built: second order across different l, light-cone or masked fields, float64 meshes, multi-GPU slabs, the multiplier fused into
the transform's first pass.  There is no CPU fallback.
"""
import ctypes as C

import numpy as np

from .. import _lib
from .._lib import DeviceArray, check, ptr

__all__ = ['calc_wst', 'wst_mesh', 'wst_modulus', 'wst_moments', 'wst_flatten', 'MAX_J', 'MAX_L', 'MAX_Q', 'MAX_EXPONENT']

MAX_J, MAX_L, MAX_Q, MAX_EXPONENT = 8, 4, 8, 8.0
MIN_N, MAX_N = 4, 32766


# ------------------------------------------------------------------------------------------------- checks made before the library loads
def _exponents(q):
    e = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if e.ndim != 1 or not 1 <= e.size <= MAX_Q:
        raise ValueError(f'q must hold 1 .. {MAX_Q} exponents, got shape {e.shape}')
    if not (np.isfinite(e).all() and (e > 0).all() and (e <= MAX_EXPONENT).all()):
        raise ValueError(f'every exponent q must lie in (0, {MAX_EXPONENT:g}], got {e.tolist()}')
    return np.ascontiguousarray(e)


def _orders(J, L):
    if int(J) != J or not 1 <= int(J) <= MAX_J:
        raise ValueError(f'J = {J}: the number of scales must be 1 .. {MAX_J}')
    if int(L) != L or not 0 <= int(L) <= MAX_L:
        raise ValueError(f'L = {L}: the largest angular order must be 0 .. {MAX_L}')
    return int(J), int(L)


def _sigma(sigma, name='sigma0'):
    s = float(sigma)
    if not (s > 0 and np.isfinite(s)):
        raise ValueError(f'{name} must be positive and finite, got {sigma}')
    return s


def _nmesh(n):
    if int(n) != n or not MIN_N <= int(n) <= MAX_N or int(n) % 2:
        raise ValueError(f'nmesh = {n}: the transform needs an even mesh of {MIN_N} .. {MAX_N} cells per side')
    return int(n)


def _box(Lbox):
    L = float(Lbox)
    if not (L > 0 and np.isfinite(L)):
        raise ValueError(f'Lbox must be positive, got {Lbox}')
    return L


def _mesh(mesh, even=True):
    """the number of cells per side of a float32 (n, n, n) NumPy array or dense `DeviceArray`"""
    if not hasattr(mesh, 'shape') or not hasattr(mesh, 'dtype'):
        raise TypeError(f'the mesh must be a float32 (n, n, n) array or DeviceArray, got {type(mesh).__name__}')
    shape = tuple(mesh.shape)
    if len(shape) != 3 or len(set(shape)) != 1:
        raise ValueError(f'the mesh must be cubic, (n, n, n), got shape {shape}')
    if np.dtype(mesh.dtype) != np.float32:
        raise TypeError(f'the mesh must be float32, got {mesh.dtype}')
    if even:
        _nmesh(shape[0])
    elif not 2 <= shape[0] <= 32767:
        raise ValueError(f'the mesh must have 2 .. 32767 cells per side, got {shape[0]}')
    if not isinstance(mesh, DeviceArray) and not np.isfinite(mesh).all():
        raise ValueError('the mesh holds values that are not finite')
    return shape[0]


# ------------------------------------------------------------------------------------------------- device calls
def _lib_wst():
    lib = _lib.lib()
    if not getattr(lib, '_wst_ready', False):
        lib.abacus_wst_check_memory.argtypes = [C.c_int, C.c_int64]
        lib.abacus_wst_modulus_dev.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
        lib.abacus_wst_spectrum_dev.argtypes = [C.c_void_p, C.c_int]
        lib.abacus_wst_moments_dev.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        lib.abacus_wst_coefficients_dev.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                    C.c_void_p, C.c_void_p, C.c_void_p]
        for name in ('check_memory', 'modulus_dev', 'spectrum_dev', 'moments_dev', 'coefficients_dev'):
            getattr(lib, 'abacus_wst_' + name).restype = C.c_int
        lib._wst_ready = True
    return lib


def _padded(n):
    """(an uninitialised padded mesh in HBM, its pitch in floats)"""
    lib = _lib.lib()
    nb = C.c_uint64(0)
    check(lib.abacus_zcv_spectrum_bytes(n, C.byref(nb)))
    pitch = int(lib.abacus_slab_pitch(n))
    return DeviceArray(nbytes=nb.value, dtype=np.float32, shape=(n, n, pitch)), pitch


def _mesh_spectrum(mesh, n):
    """the padded spectrum rfftn(mesh) / N of a float32 (n, n, n) host mesh or dense DeviceArray; the caller frees it"""
    lib = _lib_wst()
    src, owned = (mesh, False) if isinstance(mesh, DeviceArray) else (DeviceArray(np.ascontiguousarray(mesh, dtype=np.float32)), True)
    spec = None
    try:
        spec, _ = _padded(n)
        check(lib.abacus_recon_pad_dev(src.ptr, n, spec.ptr))
        check(lib.abacus_wst_spectrum_dev(spec.ptr, n))
        return spec
    except Exception:
        if spec is not None:
            spec.free()
        raise
    finally:
        if owned:
            src.free()


def _upload_spectrum(spec, n):
    """a complex64 (n, n, n/2 + 1) host spectrum in the padded layout in HBM"""
    pitch = (n + 2 + 31) // 32 * 32
    row = np.zeros((n, n, pitch // 2), dtype=np.complex64)
    row[:, :, :n // 2 + 1] = spec
    return DeviceArray(row.view(np.float32).reshape(n, n, pitch))


def _coefficients(spec_ptr, n, J, L, sigma0, e, contrast, second_order):
    Q = len(e)
    S0, S1 = np.full(Q, np.nan), np.full((J, L + 1, Q), np.nan)
    S2 = np.full((J, J, L + 1, Q), np.nan)
    check(_lib_wst().abacus_wst_coefficients_dev(spec_ptr, n, J, L, sigma0, ptr(e), Q, int(bool(contrast)), int(bool(second_order)), ptr(S0),
                                                 ptr(S1), ptr(S2)))
    return dict(S0=S0, S1=S1, S2=S2, sigmas=sigma0 * 2.0 ** np.arange(J), q=e.copy(), n=n)


# ------------------------------------------------------------------------------------------------- the public interface
def calc_wst(pos, Lbox, J=4, L=4, q=(0.8,), sigma0=0.8, nmesh=256, w=None, paste='TSC', compensated=True, interlaced=True, contrast=False,
             second_order=True, return_spectrum=False):
    """The scattering coefficients of the density field of the particles `pos` in the periodic box of side `Lbox`: steps 1 to 8 of the
    module docstring.  The meshes stay in HBM: the spectrum and three more padded meshes (two without `second_order`).

    `pos`: (N, 3) NumPy float32 / float64, an (N, 3) float32 `DeviceArray`, or three float64 `DeviceArray` columns
    (`MockDict.device_xyz`); not modified - the deposit works on a wrapped float32 copy.  `w`: per-particle weights or None.
    `sigma0`: the smallest scale in cells; `q`: 1 .. 8 exponents in (0, 8].

    Returns dict(S0 (Q,), S1 (J, L + 1, Q), S2 (J, J, L + 1, Q) with NaN where j2 <= j1 (everywhere without `second_order`), sigmas
    (J,) in cells, q (Q,), n) and, with `return_spectrum`, spectrum: the complex64 (n, n, n/2 + 1) half spectrum as the deposit
    left it (its mode k = 0 not yet replaced)."""
    from ..hod.zcv.reconstruction import _positions, _working_copy
    from .power_spectrum import _paste_code, get_W_compensated
    J, L = _orders(J, L)
    e, sigma0 = _exponents(q), _sigma(sigma0)
    n, box = _nmesh(nmesh), _box(Lbox)
    code = _paste_code(paste, ':')
    npart = _positions(pos, 'pos')
    if w is not None:
        w = np.ascontiguousarray(w, dtype=np.float32)
        if w.shape != (npart,):
            raise ValueError(f'the weights have shape {w.shape}, expected ({npart},)')
    W = np.ascontiguousarray(get_W_compensated(box, n, paste, bool(interlaced)), dtype=np.float32) if compensated else None
    lib = _lib_wst()
    check(lib.abacus_wst_check_memory(n, npart))
    spec = work = wdev = None
    try:
        spec, _ = _padded(n)
        work = _working_copy(pos, npart, 0.0, box)
        wdev = None if w is None else DeviceArray(w)
        check(lib.abacus_zcv_spectrum_dev(work.ptr, C.c_int64(npart), None if wdev is None else wdev.ptr, C.c_double(box), n, code, ptr(W),
                                          int(bool(interlaced)), spec.ptr))
        _lib.sync()
        work.free()
        work = None
        fetched = None
        if return_spectrum:
            fetched = np.empty((n, n, n // 2 + 1), dtype=np.complex64)
            check(lib.abacus_zcv_spectrum_fetch(spec.ptr, n, ptr(fetched)))
        out = _coefficients(spec.ptr, n, J, L, sigma0, e, contrast, second_order)
        if return_spectrum:
            out['spectrum'] = fetched
        return out
    finally:
        for a in (spec, work, wdev):
            if a is not None:
                a.free()


def wst_mesh(mesh, J=4, L=4, q=(0.8,), sigma0=0.8, contrast=False, second_order=True):
    """`calc_wst` from a float32 (n, n, n) mesh rho(x) - a NumPy array (checked to be finite) or a dense `DeviceArray`; not modified.
    Its spectrum is R2C(mesh) / N; the mode k = 0 is then replaced as in step 1 (1, or 0 with `contrast`), so a mesh of mean 1 (or a
    contrast of mean 0) is measured as it is."""
    J, L = _orders(J, L)
    e, sigma0 = _exponents(q), _sigma(sigma0)
    n = _mesh(mesh)
    spec = _mesh_spectrum(mesh, n)
    try:
        return _coefficients(spec.ptr, n, J, L, sigma0, e, contrast, second_order)
    finally:
        spec.free()


def wst_modulus(mesh_or_spectrum, sigma, ell):
    """U[sigma, ell] (steps 3 to 6) as a float32 (n, n, n) array.  `mesh_or_spectrum`: a float32 (n, n, n) mesh (NumPy or dense
    `DeviceArray`; its spectrum is R2C(mesh) / N, the mode k = 0 kept) or a complex64 (n, n, n/2 + 1) NumPy half spectrum in the
    1 / N convention; not modified.  `sigma` in cells."""
    sigma = _sigma(sigma, 'sigma')
    if int(ell) != ell or not 0 <= int(ell) <= MAX_L:
        raise ValueError(f'ell = {ell}: the angular order must be 0 .. {MAX_L}')
    ell = int(ell)
    given = mesh_or_spectrum
    if isinstance(given, np.ndarray) and given.dtype == np.complex64:
        shape = given.shape
        if given.ndim != 3 or shape[0] != shape[1] or shape[2] != shape[0] // 2 + 1:
            raise ValueError(f'a spectrum must have shape (n, n, n/2 + 1), got {shape}')
        n = _nmesh(shape[0])
        if not np.isfinite(given).all():
            raise ValueError('the spectrum holds values that are not finite')
        spec = _upload_spectrum(given, n)
    else:
        n = _mesh(given)
        spec = _mesh_spectrum(given, n)
    work = out = None
    try:
        work, _ = _padded(n)
        out, _ = _padded(n)
        check(_lib_wst().abacus_wst_modulus_dev(spec.ptr, n, sigma, ell, work.ptr, out.ptr))
        _lib.sync()
        return np.ascontiguousarray(out.get()[:, :, :n])
    finally:
        for a in (spec, work, out):
            if a is not None:
                a.free()


def wst_moments(mesh, q):
    """float64 (Q,): the means <|x|^q> over the cells of a float32 (n, n, n) mesh (NumPy or dense `DeviceArray`, any n of 2 .. 32767),
    from the float64 sums of step 8."""
    e = _exponents(q)
    n = _mesh(mesh, even=False)
    dev, owned = (mesh, False) if isinstance(mesh, DeviceArray) else (DeviceArray(np.ascontiguousarray(mesh, dtype=np.float32)), True)
    try:
        s = np.full(len(e), np.nan)
        check(_lib_wst().abacus_wst_moments_dev(dev.ptr, n, n, ptr(e), len(e), ptr(s)))
        return s / float(n) ** 3
    finally:
        if owned:
            dev.free()


def wst_flatten(result):
    """The coefficient vector of a result of `calc_wst` / `wst_mesh`, float64, for an emulator.  Order: S0[q]; then S1[j, l, q] with j
    slowest and q fastest; then, when the second order was computed, S2[j1, j2, l, q] over the pairs j1 < j2 only, j1 slowest, then
    j2, l, q.  Length Q (1 + J (L + 1) + J (J - 1) / 2 (L + 1)), or Q (1 + J (L + 1)) without second order.  Host only."""
    S0, S1, S2 = (np.asarray(result[k], dtype=np.float64) for k in ('S0', 'S1', 'S2'))
    J = S1.shape[0]
    if S1.ndim != 3 or S2.shape != (J, J) + S1.shape[1:] or S0.shape != S1.shape[2:]:
        raise ValueError(f'not a WST result: S0 {S0.shape}, S1 {S1.shape}, S2 {S2.shape}')
    parts = [S0.ravel(), S1.ravel()]
    j1, j2 = np.triu_indices(J, 1)
    if len(j1) and not np.isnan(S2[j1, j2]).all():
        parts.append(S2[j1, j2].ravel())
    return np.concatenate(parts)
