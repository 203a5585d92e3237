"""Spherical voids of the density field on the MI355X: the mesh-based spherical void finder of Banerjee & Dalal (2016), the void size
function and the void-galaxy cross-correlation.  The reference has no void finder; no reference code stands behind this module - its
arithmetic is stated in include/abacus_hip.h and pinned to the NumPy statement tests/voids_statement.py.

1. Mesh.  A periodic box of side L, n^3 cells of side a = L / n, cell i centred at i a.  m <= 32 radii R_1 > R_2 > .. > R_m > 0 with
   2 R_1 <= L / 2 (the minimum image of two centres is then unique), a threshold delta_th (default -0.7).
2. Field of level i (`find_voids`).  delta(k) as `get_field_fft` leaves it (paste, compensation and interlacing as in `calc_power`),
   resident in HBM in the padded layout (`abacus_zcv_spectrum_dev`); every mode times float32(W(x)), W(x) = 3 (sin x - x cos x) / x^3
   evaluated in float64 (1 - x^2/10 + x^4/280 below x = 0.1), x = |k| R_i, |k| = (2 pi / L) sqrt(i^2 + j^2 + l^2) of the integer mode
   numbers (i below n/2, i - n from n/2 on (x, y), 0 .. n/2 on z), written to a second padded mesh, the C2R in place there
   (`abacus_void_tophat_dev`).  delta(k) is kept for the next radius.
3. Candidates of level i.  The cells with value < float32(delta_th), compared in float32: never a NaN, -inf is one.  Key: (value, flat
   index (x n + y) n + z), by value first; -0.0 and +0.0 are one value.
4. Selection.  D[i][j] = ceil((R_i / a + R_j / a)^2), int64 from float64, computed here once.  Two voids of levels i and j overlap
   iff the integer squared minimum-image distance of their centre cells is below D[i][j]; touching spheres do not overlap.  Levels in
   order; within a level the candidates in ascending key order; a candidate becomes a void iff it overlaps no void accepted so far.
   The device reaches the same set in rounds of two kernels (`abacus_void_level_dev`): no thread waits for another.
5. Output in level order, within a level in ascending key order: `cell`, `level`, `delta` (the centre value; -0.0 comes back as
   +0.0), `centres` = cell a, `radius`, and per level the candidates, voids and rounds.

Limits: n even, 4 .. 1024; 1 .. 32 radii, positive, finite, strictly decreasing, 2 R_1 <= L / 2; the threshold finite in float32.  A
host mesh must be free of NaN (checked); a device mesh is not checked.

Not built: partial overlap fractions (a void is kept or dropped whole), profiles stacked in r / R_v, light cones or masks, float64
meshes, multi-GPU slabs, voids across tracers.  Watershed voids: analysis/watershed.py.  There is no CPU fallback.
"""
import ctypes as C
import math

import numpy as np

from .. import _lib
from .._lib import DeviceArray, check, ptr

__all__ = ['find_voids', 'find_voids_mesh', 'tophat_smooth', 'void_size_function', 'void_galaxy_xi', 'overlap_table', 'MAX_LEVELS']

MAX_LEVELS = 32
MIN_MESH, MAX_MESH = 4, 1024


# ------------------------------------------------------------------------------------------------- checks made before the library loads
def _box(Lbox):
    L = float(Lbox)
    if not (L > 0 and np.isfinite(L)):
        raise ValueError(f'Lbox must be positive, got {Lbox}')
    return L


def _nmesh(n):
    n = int(n)
    if n < MIN_MESH or n > MAX_MESH or n % 2:
        raise ValueError(f'nmesh = {n}: the void finder needs an even mesh of {MIN_MESH} .. {MAX_MESH} cells per side')
    return n


def _radii(radii, L):
    r = np.atleast_1d(np.asarray(radii, dtype=np.float64))
    if r.ndim != 1 or not 1 <= r.size <= MAX_LEVELS:
        raise ValueError(f'radii must hold 1 .. {MAX_LEVELS} values, got shape {r.shape}')
    if not (np.isfinite(r).all() and (r > 0).all()):
        raise ValueError('the radii must be finite and positive')
    if not (np.diff(r) < 0).all():
        raise ValueError('the radii must decrease strictly: the largest voids are taken first')
    if 2.0 * r[0] > 0.5 * L:
        raise ValueError(f'the largest radius {r[0]:g} exceeds Lbox / 4 = {0.25 * L:g}: two voids must fit half the box')
    return r


def _threshold(threshold):
    t = float(threshold)
    with np.errstate(over='ignore'):
        t32 = np.float32(t)
    if not (np.isfinite(t) and np.isfinite(t32)):
        raise ValueError(f'the threshold must be finite (in float32), got {threshold}')
    return float(t32)


def overlap_table(radii, Lbox, n):
    """int64 (m, m): D[i][j] = ceil((R_i / a + R_j / a)^2) with a = Lbox / n, from float64 (step 4 of the module docstring)"""
    r = np.asarray(radii, dtype=np.float64) / (float(Lbox) / int(n))
    return np.ceil((r[:, None] + r[None, :]) ** 2).astype(np.int64)


def _table(radii, L, n):
    D = np.ascontiguousarray(overlap_table(radii, L, n))
    if D.max() > (n // 2) ** 2:                                  # 2 R_1 <= L / 2 in exact arithmetic; the float64 roundings may differ
        raise ValueError(f'the largest radius {radii[0]:g} does not fit: ceil((2 R / a)^2) = {D.max()} exceeds (n / 2)^2')
    return D


def _meshes(fields, m):
    """(list of m meshes, n): m given float32 (n, n, n) meshes, or one mesh used at every level"""
    one = hasattr(fields, 'shape') and hasattr(fields, 'dtype') and len(tuple(fields.shape)) == 3
    if one:
        fields = [fields] * m
    else:
        fields = list(fields)
    if len(fields) != m:
        raise ValueError(f'{len(fields)} meshes for {m} radii')
    n = None
    for f in fields:
        if not hasattr(f, 'shape') or not hasattr(f, 'dtype'):
            raise TypeError(f'a mesh must be a float32 (n, n, n) array or DeviceArray, got {type(f).__name__}')
        shape = tuple(f.shape)
        if len(shape) != 3 or len(set(shape)) != 1:
            raise ValueError(f'a mesh must be cubic, (n, n, n), got shape {shape}')
        if np.dtype(f.dtype) != np.float32:
            raise TypeError(f'a mesh must be float32, got {f.dtype}')
        if n is not None and shape[0] != n:
            raise ValueError(f'the meshes differ in size: {n} and {shape[0]}')
        n = _nmesh(shape[0])
        if not isinstance(f, DeviceArray) and np.isnan(f).any():
            raise ValueError('a mesh holds NaN')
    return fields, n


# ------------------------------------------------------------------------------------------------- the finder on resident meshes
class _Finder:
    """the handle of abacus_void_create and the per-level counts"""

    def __init__(self, n, D):
        self.n, self.m = n, len(D)
        self.handle = C.c_void_p()
        self.counts = np.zeros((self.m, 3), dtype=np.int64)
        check(_lib.lib().abacus_void_create(n, self.m, ptr(D), C.byref(self.handle)))

    def level(self, i, mesh_ptr, pitch, t32):
        nc, nv, nr = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(_lib.lib().abacus_void_level_dev(self.handle, mesh_ptr, int(pitch), int(i), C.c_float(t32), C.byref(nc), C.byref(nv),
                                               C.byref(nr)))
        self.counts[i] = nc.value, nv.value, nr.value

    def fetch(self):
        lib = _lib.lib()
        nv = C.c_int64(0)
        check(lib.abacus_void_count(self.handle, C.byref(nv)))
        cell = np.zeros((nv.value, 3), dtype=np.int32)
        level, delta = np.zeros(nv.value, dtype=np.int32), np.zeros(nv.value, dtype=np.float32)
        check(lib.abacus_void_fetch(self.handle, ptr(cell), ptr(level), ptr(delta)))
        return cell, level, delta

    def free(self):
        if self.handle:
            _lib.lib().abacus_void_free(self.handle)
            self.handle = C.c_void_p()


def _result(finder, radii, L, n):
    cell, level, delta = finder.fetch()
    return dict(centres=cell.astype(np.float64) * (L / n), radius=radii[level], level=level, delta=delta, cell=cell,
                counts=finder.counts.copy(), radii=radii.copy())


# ------------------------------------------------------------------------------------------------- the public interface
def find_voids_mesh(fields, Lbox, radii, threshold=-0.7):
    """The finder alone (steps 3 to 5 of the module docstring) on m given float32 (n, n, n) meshes, one per radius, or on one mesh
    used at every level.  The meshes: NumPy arrays (checked to be free of NaN) or dense `DeviceArray`; not modified.

    Returns dict(centres (Nv, 3) float64 in [0, L), radius (Nv,), level (Nv,) int32, delta (Nv,) float32, cell (Nv, 3) int32,
    counts (m, 3) int64: the candidates, voids and rounds per level, radii)."""
    L = _box(Lbox)
    r = _radii(radii, L)
    t32 = _threshold(threshold)
    fields, n = _meshes(fields, len(r))
    D = _table(r, L, n)
    finder = _Finder(n, D)
    try:
        dev, shared = None, None                                 # one upload for a mesh that serves several levels in a row
        for i, f in enumerate(fields):
            if isinstance(f, DeviceArray):
                finder.level(i, f.ptr, n, t32)
                continue
            if f is not shared:
                if dev is not None:
                    dev.free()
                dev, shared = DeviceArray(np.ascontiguousarray(f, dtype=np.float32)), f
            finder.level(i, dev.ptr, n, t32)
        if dev is not None:
            dev.free()
        return _result(finder, r, L, n)
    finally:
        finder.free()


def _spectrum(pos, L, n, w, paste, compensated, interlaced):
    """(spec, pitch): the padded spectrum of the particles in HBM, as `calc_minkowski` takes it"""
    from ..hod.zcv.reconstruction import _positions, _working_copy
    from .power_spectrum import _paste_code, get_W_compensated
    code = _paste_code(paste, ':')
    npart = _positions(pos, 'pos')
    if w is not None:
        w = np.ascontiguousarray(w, dtype=np.float32)
        if w.shape != (npart,):
            raise ValueError(f'the weights have shape {w.shape}, expected ({npart},)')
    W = np.ascontiguousarray(get_W_compensated(L, n, paste, bool(interlaced)), dtype=np.float32) if compensated else None
    lib = _lib.lib()
    check(lib.abacus_void_check_memory(n, C.c_int64(npart)))
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
        return spec, pitch
    except Exception:
        if spec is not None:
            spec.free()
        raise
    finally:
        for a in (work, wdev):
            if a is not None:
                a.free()


def find_voids(pos, Lbox, radii, threshold=-0.7, nmesh=256, w=None, paste='TSC', compensated=True, interlaced=True, return_fields=False):
    """The spherical voids of the density contrast of the particles `pos` in the periodic box of side `Lbox`: steps 1 to 5 of the
    module docstring.  The meshes stay in HBM.

    `pos`: (N, 3) NumPy float32 / float64, an (N, 3) float32 `DeviceArray`, or three float64 `DeviceArray` columns
    (`MockDict.device_xyz`); not modified - the deposit works on a wrapped float32 copy.  `w`: per-particle weights or None.
    `radii`: at most 32 values, strictly decreasing, in the units of `Lbox`.

    Returns dict(centres (Nv, 3) float64 in [0, L), radius (Nv,), level (Nv,) int32, delta (Nv,) float32, cell (Nv, 3) int32,
    counts (m, 3) int64: the candidates, voids and rounds per level, radii) and, with `return_fields`, fields: the m float32
    (n, n, n) meshes the decisions were taken on."""
    L = _box(Lbox)
    r = _radii(radii, L)
    t32 = _threshold(threshold)
    n = _nmesh(nmesh)
    D = _table(r, L, n)
    spec, pitch = _spectrum(pos, L, n, w, paste, compensated, interlaced)
    out = finder = None
    try:
        lib = _lib.lib()
        out = DeviceArray(nbytes=spec.nbytes, dtype=np.float32, shape=(n, n, pitch))
        finder = _Finder(n, D)
        fields = []
        for i, R in enumerate(r):
            check(lib.abacus_void_tophat_dev(spec.ptr, n, C.c_double(L), C.c_double(R), out.ptr))
            finder.level(i, out.ptr, pitch, t32)
            if return_fields:
                fields.append(np.ascontiguousarray(out.get()[:, :, :n]))
        res = _result(finder, r, L, n)
        if return_fields:
            res['fields'] = fields
        return res
    finally:
        if finder is not None:
            finder.free()
        for a in (spec, out):
            if a is not None:
                a.free()


def tophat_smooth(spectrum, Lbox, R):
    """The filter alone: the complex64 half spectrum (n, n, n/2 + 1) of a mesh, normalised by 1 / n^3, times the top hat of radius `R`
    and transformed back (step 2 of the module docstring): the float32 (n, n, n) mesh."""
    s = np.asarray(spectrum)
    if s.ndim != 3 or s.shape[0] != s.shape[1] or s.shape[2] != s.shape[0] // 2 + 1:
        raise ValueError(f'the spectrum must have shape (n, n, n/2 + 1), got {s.shape}')
    n, L, R = _nmesh(s.shape[0]), _box(Lbox), float(R)
    if not (R >= 0 and np.isfinite(R)):
        raise ValueError(f'R must be finite and not negative, got {R}')
    lib = _lib.lib()
    pitch = int(lib.abacus_slab_pitch(n))
    row = np.zeros((n, n, pitch // 2), dtype=np.complex64)
    row[:, :, :n // 2 + 1] = s
    src, dst = DeviceArray(row), DeviceArray(nbytes=row.nbytes, dtype=np.float32, shape=(n, n, pitch))
    try:
        check(lib.abacus_void_tophat_dev(src.ptr, n, C.c_double(L), C.c_double(R), dst.ptr))
        _lib.sync()
        return np.ascontiguousarray(dst.get()[:, :, :n])
    finally:
        src.free()
        dst.free()


def void_size_function(level_or_counts, radii, Lbox):
    """The void size function.  `level_or_counts`: a result of `find_voids`, its (m, 3) `counts` table (the voids per level are its
    second column), or the 1-D integer `level` of every void.  For i = 1 .. m - 1:  dn/dlnR = N_i / (L^3 ln(R_i / R_{i+1})) at
    Rbar_i = (R_i + R_{i+1}) / 2, with the Poisson error sqrt(N_i) over the same denominator.  Host only.

    Returns dict(R (m - 1,), dn_dlnR, error, counts: N_1 .. N_{m-1})."""
    L = _box(Lbox)
    r = np.atleast_1d(np.asarray(radii, dtype=np.float64))
    if r.ndim != 1 or r.size < 2 or not (np.isfinite(r).all() and (r > 0).all() and (np.diff(r) < 0).all()):
        raise ValueError('the size function needs at least two finite, positive, strictly decreasing radii')
    v = level_or_counts['counts'] if isinstance(level_or_counts, dict) else level_or_counts
    v = np.asarray(v)
    if not np.issubdtype(v.dtype, np.integer):
        raise ValueError(f'levels or counts must be integers, got {v.dtype}')
    if v.ndim == 2:
        if v.shape != (r.size, 3):
            raise ValueError(f'the counts table has shape {v.shape}, expected ({r.size}, 3)')
        counts = v[:, 1].astype(np.int64)
    elif v.ndim == 1:
        if v.size and (v.min() < 0 or v.max() >= r.size):
            raise ValueError(f'a level is outside 0 .. {r.size - 1}')
        counts = np.bincount(v, minlength=r.size).astype(np.int64)
    else:
        raise ValueError(f'levels (1-D) or a counts table (m, 3) expected, got shape {v.shape}')
    if (counts < 0).any():
        raise ValueError('negative counts')
    N = counts[:-1].astype(np.float64)
    den = L**3 * np.log(r[:-1] / r[1:])
    return dict(R=0.5 * (r[:-1] + r[1:]), dn_dlnR=N / den, error=np.sqrt(N) / den, counts=counts[:-1].copy())


def void_galaxy_xi(voids, X, Y, Z, Lbox, bins, levels=None):
    """The void-galaxy cross-correlation xi_vg(r) = DD / (N_v N_g dV / L^3) - 1 with dV = 4 pi (r_hi^3 - r_lo^3) / 3, from the
    cross pair counts `DD(autocorr=0, ...)` of the void centres (first set) and the galaxies, in float64 on the host.  `voids`: a
    result of `find_voids`; `levels`: None or the radius classes to stack.  X, Y, Z: the galaxies' columns as `DD` takes them.

    Returns dict(r (the bin centres), xi, npairs uint64, nvoids, ngal)."""
    from .tpcf_corrfunc import DD
    L = _box(Lbox)
    bins = np.asarray(bins, dtype=np.float64)
    if bins.ndim != 1 or bins.size < 2 or not (np.diff(bins) > 0).all() or bins[0] < 0:
        raise ValueError('bins must be at least two increasing, non-negative edges')
    centres, level = np.asarray(voids['centres'], dtype=np.float64), np.asarray(voids['level'])
    if levels is not None:
        centres = centres[np.isin(level, np.atleast_1d(levels))]
    nv, ng = len(centres), len(X)
    if nv == 0:
        raise ValueError('no void to correlate' + ('' if levels is None else f' at the levels {levels}'))
    c32 = [np.ascontiguousarray(centres[:, a], dtype=np.float32) for a in range(3)]
    res = DD(0, 1, bins, c32[0], c32[1], c32[2], X2=X, Y2=Y, Z2=Z, periodic=True, boxsize=L)
    npairs = res['npairs'].astype(np.uint64)
    dV = 4.0 * math.pi / 3.0 * (bins[1:] ** 3 - bins[:-1] ** 3)
    xi = npairs.astype(np.float64) / (float(nv) * float(ng) * dV / L**3) - 1.0
    return dict(r=0.5 * (bins[1:] + bins[:-1]), xi=xi, npairs=npairs, nvoids=nv, ngal=ng)
