"""Bispectrum of a periodic box on the MI355X: the FFT estimator of Scoccimarro 2015 (see also Sefusatti et al. 2016).  The reference
has no three-point statistic; no reference code stands behind this module - its arithmetic is stated in include/abacus_hip.h and pinned
to the NumPy statement tests/bispectrum_statement.py.

1. Spectrum.  delta(k) of the particles as `get_field_fft` leaves it (divided by n^3; paste, compensation and interlacing as in
   `calc_power`), resident in HBM in the padded layout (`abacus_zcv_spectrum_dev`).
2. Shells.  dk = float32(2 pi / L); mode numbers i -> i below n/2, i - n from n/2 on (x, y), 0 .. n/2 on z;
   |k| = dk sqrt(float32(ix^2 + iy^2 + iz^2)) in float32; a mode belongs to shell b iff kedges[b] <= |k| < kedges[b + 1] against the
   float32 edges.  D_b(x) = sum_{k in b} delta(k) e^{ikx}, I_b(x) the same with delta -> 1: one masking pass that writes all nb padded
   spectra, nb C2R in place (`abacus_bk_shells_dev`).
3. Sums over the n^3 cells (`abacus_bk_triple_dev`: float32 products on the matrix cores, float64 sums):
   S[i][j][l] = sum_x D_i D_j D_l / n^3,  N[i][j][l] = sum_x I_i I_j I_l / n^3 (the number of closed triangles),
   G[i] = sum_x D_i^2 / n^3,  M[i] = sum_x I_i^2 / n^3 (the modes of the full shell).
4. B(i, j, l) = L^6 S / N for i <= j <= l with N > 0.5 (and kedges[l] < kedges[i + 1] + kedges[j + 1]: no triangle closes otherwise, and
   the float32 noise of N on a large mesh must not open such a bin), in lexicographic order;  P(i) = L^3 G / M;  k of a side: the
   mode-weighted mean |k| of its shell (host, float64).
5. Shot noise (unit weights, nbar = N_gal / L^3; host, float64): P_shot = 1 / nbar, B_shot = (P_i + P_j + P_l) / nbar + 1 / nbar^2 and
   Q = (B - B_shot) / (P_i P_j + P_j P_l + P_l P_i) with the shot-subtracted P.  With weights B and P are returned raw.

The sums close triangles modulo n: they are the triangles only while every mode used lies below n / 3, so kedges[nb] <= dk n / 3 is
required.  The Nyquist planes are then never inside a shell and every masked spectrum is Hermitian as written.  N and M depend on
(n, L, kedges) only: `triangle_counts` computes them once per key (`counts_built()` counts how often).  The I fields and the D fields
share the nb work meshes.

Not built: cross bispectra, multipoles with respect to a line of sight, light-cone (FKP) bispectra, more than 32 shells, multi-GPU
slabs.  There is no CPU fallback.
"""
import ctypes as C

import numpy as np

from .. import _lib
from .._lib import DeviceArray, check, ptr
from .power_spectrum import _paste_code, get_W_compensated

__all__ = ['calc_bispectrum', 'bispectrum_from_spectrum', 'triangle_counts', 'counts_built', 'shot_noise_and_Q', 'MAX_SHELLS']

MAX_SHELLS = 32
_counts = {}
_built = [0]


# ------------------------------------------------------------------------------------------------- checks made before the library loads
def _check_args(n, Lbox, kedges):
    """(n, L, float64 edges) or ValueError; the limits of abacus_bk_shells_dev, judged the same way"""
    n, L = int(n), float(Lbox)
    if n < 2 or n % 2 or n > 32767:
        raise ValueError(f'nmesh = {n}: the bispectrum needs an even mesh of 2 .. 32766 cells per side')
    if not (L > 0 and np.isfinite(L)):
        raise ValueError(f'Lbox must be positive, got {Lbox}')
    ke = np.ascontiguousarray(kedges, dtype=np.float64)
    if ke.ndim != 1 or not 1 <= len(ke) - 1 <= MAX_SHELLS:
        raise ValueError(f'kedges must hold the edges of 1 .. {MAX_SHELLS} shells, got shape {ke.shape}')
    e32 = ke.astype(np.float32)
    if not (np.isfinite(ke).all() and (ke > 0).all() and (np.diff(e32) > 0).all()):
        raise ValueError('kedges must be finite, positive and increasing (in float32)')
    # the rule with the slack of the two float32 roundings (dk and the edge), so that float64(2 pi / L) n / 3 passes; and what it stands
    # for, exactly: the first mode number at or beyond n / 3 on an axis is in no shell
    dk32, mc = np.float32(2.0 * np.pi / L), (n + 2) // 3
    top = float(dk32) * n / 3.0
    if not (float(e32[-1]) <= top * (1.0 + 2.0**-22) and dk32 * np.sqrt(np.float32(mc * mc)) >= e32[-1]):
        raise ValueError(f'the top edge {ke[-1]:g} lies above dk n / 3 = {top:g}: the sums over the mesh would close triangles modulo n; '
                         'use a larger mesh or a lower edge')
    return n, L, ke


def _padded(n, count=1):
    """`count` padded meshes of n^3 cells in one allocation (one hipMalloc however many shells)"""
    nb = C.c_uint64(0)
    check(_lib.lib().abacus_zcv_spectrum_bytes(n, C.byref(nb)))
    return DeviceArray(nbytes=count * nb.value, dtype=np.uint8, shape=(count * nb.value,))


def _table(block, count):
    """the host array of device pointers to the `count` meshes of a `_padded` block (a padded mesh is a multiple of 128 bytes long)"""
    each = block.nbytes // count
    return (C.c_void_p * count)(*[block.ptr.value + b * each for b in range(count)])


def _sums(spec_ptr, n, L, ke, meshes):
    """(T (nb, nb, nb), G (nb,)) / n^3 of the shell fields of the padded spectrum (None: the I fields) through the work meshes"""
    nb = len(ke) - 1
    lib = _lib.lib()
    check(lib.abacus_bk_shells_dev(spec_ptr, n, C.c_double(L), ptr(ke), nb, _table(meshes, nb)))
    T, G = np.empty((nb, nb, nb), dtype=np.float64), np.empty(nb, dtype=np.float64)
    check(lib.abacus_bk_triple_dev(_table(meshes, nb), n, nb, ptr(T), ptr(G)))
    return T / float(n) ** 3, G / float(n) ** 3


def shell_k_mean(n, Lbox, kedges):
    """(k_mean (nb,), modes (nb,) int64) of the full shells on the host: the float32 rule of the module docstring decides the shell, the
    mean of float64(dk) sqrt(m2) is taken in float64; modes with k_z > 0 count twice (their mirror images)"""
    n, L, ke = _check_args(n, Lbox, kedges)
    nb = len(ke) - 1
    dk, e32 = np.float32(2.0 * np.pi / L), ke.astype(np.float32)
    f = np.where(np.arange(n) < n // 2, np.arange(n), np.arange(n) - n).astype(np.int64)
    kz = np.arange(n // 2 + 1, dtype=np.int64)
    mult = np.where((kz == 0) | (kz == n // 2), 1.0, 2.0)
    ksum, cnt = np.zeros(nb), np.zeros(nb)
    for a in f:                                   # one (y, z) plane at a time: the host never holds the whole mesh
        m2 = a * a + f[:, None] ** 2 + kz[None, :] ** 2
        k = dk * np.sqrt(m2.astype(np.float32))
        b = np.searchsorted(e32, k.ravel(), side='right') - 1
        ok = (b >= 0) & (b < nb)
        w = np.broadcast_to(mult, m2.shape).ravel()[ok]
        cnt += np.bincount(b[ok], weights=w, minlength=nb)
        ksum += np.bincount(b[ok], weights=w * np.sqrt(m2.ravel()[ok].astype(np.float64)), minlength=nb)
    with np.errstate(divide='ignore', invalid='ignore'):
        k_mean = np.where(cnt > 0, float(dk) * ksum / cnt, 0.0)
    return k_mean, np.rint(cnt).astype(np.int64)


def counts_built():
    """how often `triangle_counts` has run the I fields on the device since the module was loaded"""
    return _built[0]


def triangle_counts(n, Lbox, kedges, _meshes=None):
    """N[i][j][l] = sum_x I_i I_j I_l / n^3, M[i] = sum_x I_i^2 / n^3 and the mode-weighted mean k of every shell: they depend on
    (n, Lbox, kedges) only and are kept by that key.  Returns dict(N (nb, nb, nb) float64, M (nb,) float64, k_mean (nb,))."""
    n, L, ke = _check_args(n, Lbox, kedges)
    key = (n, L, tuple(float(e) for e in ke))
    if key not in _counts:
        k_mean, _ = shell_k_mean(n, L, ke)
        meshes = None
        try:
            if _meshes is None:
                check(_lib.lib().abacus_bk_check_memory(n, len(ke) - 1, C.c_int64(0)))
                meshes = _padded(n, len(ke) - 1)
            N, M = _sums(None, n, L, ke, meshes if _meshes is None else _meshes)
        finally:
            if meshes is not None:
                meshes.free()
        _counts[key] = dict(N=N, M=M, k_mean=k_mean)
        _built[0] += 1
    return _counts[key]


# ------------------------------------------------------------------------------------------------- host arithmetic
def shot_noise_and_Q(B, P, ijl, nbar):
    """(P_shot, B_shot (ntri,), Q (ntri,)) in float64 from the raw B (ntri,), the raw P (nb,), the bin indices ijl (ntri, 3) and the
    number density nbar of unit-weight tracers: step 5 of the module docstring"""
    B, P, ijl = np.asarray(B, dtype=np.float64), np.asarray(P, dtype=np.float64), np.asarray(ijl, dtype=np.int64).reshape(-1, 3)
    if not (nbar > 0 and np.isfinite(nbar)):
        raise ValueError(f'nbar must be positive, got {nbar}')
    P_shot = 1.0 / nbar
    Ps = P - P_shot
    p1, p2, p3 = Ps[ijl[:, 0]], Ps[ijl[:, 1]], Ps[ijl[:, 2]]
    B_shot = (p1 + p2 + p3) / nbar + 1.0 / nbar**2
    with np.errstate(divide='ignore', invalid='ignore'):
        Q = (B - B_shot) / (p1 * p2 + p2 * p3 + p3 * p1)
    return P_shot, B_shot, Q


def _result(S, G, counts, L, N_gal, ke):
    N, M, k_mean = counts['N'], counts['M'], counts['k_mean']
    nb = len(M)
    # N > 0.5, and the triangle inequality on the edges: a bin whose longest side cannot be reached by the other two holds no triangle,
    # whatever float32 noise its N carries on a large mesh (it reaches 0.5 from 64^3 on, profiles/bispectrum/README.md)
    ijl = np.array([(i, j, l) for i in range(nb) for j in range(i, nb) for l in range(j, nb)
                    if N[i, j, l] > 0.5 and ke[l] < ke[i + 1] + ke[j + 1]], dtype=np.int64).reshape(-1, 3)
    i, j, l = ijl[:, 0], ijl[:, 1], ijl[:, 2]
    N_tri = N[i, j, l]
    B = L**6 * S[i, j, l] / N_tri
    with np.errstate(divide='ignore', invalid='ignore'):
        P = np.where(M > 0.5, L**3 * G / M, 0.0)
    out = dict(k1=k_mean[i], k2=k_mean[j], k3=k_mean[l], B=B, N_tri=N_tri, ijl=ijl, k_mean=k_mean, P=P, N_mode=M,
               P_shot=None, B_shot=None, Q=None)
    if N_gal is not None:
        out['P_shot'], out['B_shot'], out['Q'] = shot_noise_and_Q(B, P, ijl, N_gal / L**3)
    return out


# ------------------------------------------------------------------------------------------------- the estimator
def bispectrum_from_spectrum(spec_padded, n, Lbox, kedges, N_gal=None):
    """Steps 2 to 5 from a spectrum that is resident already: `spec_padded` a `DeviceArray` (or a device pointer) holding delta(k) in the
    padded layout, normalised as `get_field_fft` normalises; it is not modified.  `N_gal`: the number of unit-weight tracers behind the
    spectrum (None: no shot noise, `P_shot`, `B_shot` and `Q` are None).  Returns the dict of `calc_bispectrum`."""
    n, L, ke = _check_args(n, Lbox, kedges)
    if N_gal is not None and not N_gal > 0:
        raise ValueError(f'N_gal must be positive, got {N_gal}')
    spec_ptr = spec_padded.ptr if isinstance(spec_padded, DeviceArray) else C.c_void_p(int(spec_padded))
    if not spec_ptr:
        raise ValueError('the spectrum is a null pointer')
    nb = len(ke) - 1
    check(_lib.lib().abacus_bk_check_memory(n, nb, C.c_int64(0)))
    meshes = None
    try:
        meshes = _padded(n, nb)
        counts = triangle_counts(n, L, ke, _meshes=meshes)       # the I fields first, in the meshes the D fields then take
        S, G = _sums(spec_ptr, n, L, ke, meshes)
    finally:
        if meshes is not None:
            meshes.free()
    return _result(S, G, counts, L, N_gal, ke)


def calc_bispectrum(pos, Lbox, kedges, nmesh=256, w=None, paste='TSC', compensated=True, interlaced=True):
    """B(k1, k2, k3) of the particles `pos` in the periodic box of side `Lbox` for every triangle bin of the shells `kedges` (h/Mpc,
    increasing, at most 32 shells, the top edge at most 2 pi / Lbox * nmesh / 3): steps 1 to 5 of the module docstring.

    `pos`: (N, 3) NumPy float32 / float64, an (N, 3) float32 `DeviceArray`, or three float64 `DeviceArray` columns
    (`MockDict.device_xyz`); not modified - the deposit works on a wrapped float32 copy.  `w`: per-particle weights or None.

    Returns dict(k1, k2, k3 (ntri,), B (ntri,), N_tri (ntri,) float64 and not rounded, ijl (ntri, 3), k_mean (nb,), P (nb,),
    N_mode (nb,), P_shot, B_shot (ntri,), Q (ntri,)); B and P are raw (shot noise included); `P_shot`, `B_shot` and `Q` are None with
    weights."""
    from ..hod.zcv.reconstruction import _positions, _working_copy
    n, L, ke = _check_args(nmesh, Lbox, kedges)
    code = _paste_code(paste, ':')
    npart = _positions(pos, 'pos')
    if w is not None:
        w = np.ascontiguousarray(w, dtype=np.float32)
        if w.shape != (npart,):
            raise ValueError(f'the weights have shape {w.shape}, expected ({npart},)')
    W = np.ascontiguousarray(get_W_compensated(L, n, paste, bool(interlaced)), dtype=np.float32) if compensated else None
    lib = _lib.lib()
    check(lib.abacus_bk_check_memory(n, len(ke) - 1, C.c_int64(npart)))
    spec = work = wdev = None
    try:
        spec = _padded(n)
        work = _working_copy(pos, npart, 0.0, L)
        wdev = None if w is None else DeviceArray(w)
        check(lib.abacus_zcv_spectrum_dev(work.ptr, C.c_int64(npart), None if wdev is None else wdev.ptr, C.c_double(L), n, code, ptr(W),
                                          int(bool(interlaced)), spec.ptr))
        _lib.sync()
        work.free()
        work = None
        return bispectrum_from_spectrum(spec, n, L, ke, N_gal=None if w is not None else npart)
    finally:
        for a in (spec, work, wdev):
            if a is not None:
                a.free()
