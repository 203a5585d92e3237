"""`periodic_window_function` of the reference (abacusnbody/hod/zcv/zenbu_window.py:48-181) on the MI355X: the mode-coupling matrix
that `tools_cv.run_zcv` folds into the ZeNBu theory (tools_cv.py:640-647, :703-706), and the file it is loaded from.  The ZeNBu and
classy parts of the reference's module (`zenbu_spectra`, `_lpt_pk`, `main`) stay with the reference; this module imports without
classy, ZeNBu, yaml or a GPU.

    window, keff = periodic_window_function(nmesh, lbox, kout, kin, k2weight=True)   # the reference's signature and returns
    save_window(zcv_dir, sim_name, nmesh, Lbox, k_hMpc_max, n_k_bins)                 # the file run_zcv loads

The reference visits every mode (i, j, k) of the nmesh x nmesh x nmesh/2 half mesh and, inside, every input column `beta`.  The
inner work multiplies one per-mode value by a per-column weight, so the window is a histogram of nine Legendre products over the
`kout` bins (`window_moments`: one device pass, no mesh in memory, csrc/window.hip) followed by an outer product with the column
weights (`assemble_window`: NumPy).  What a mode contributes, every step in float32 and in this order:

    kvals  = the reference's two float32 `np.arange` halves (:75-81); the half axis is its first half (the Nyquist plane of the
             last axis is NOT visited)
    knorm  = sqrt((kvals[k]^2 + kvals[j]^2) + kvals[i]^2)          (`meshgrid` returns zz, yy, xx: :36-45, :86-87)
    mu     = kvals[i] / knorm, 0 at the origin                     (the line of sight is axis 0, signed)
    L0, L2, L4 = 1, (3 mu^2 - 1) / 2, (35 mu^4 - 30 mu^2 + 3) / 8  with mu^4 = (mu^2)^2
    o      = digitize(knorm, kout) - 1                             (float32 against the float64 edges: kout[o] <= knorm < kout[o+1])
    m      = 1 on the plane k = 0, 2 elsewhere
    nmodes[o] += m;  ksum[o] += m knorm;  S[o, l, l'] += m fl32(fl32(pref_l L_l) L_l'),  pref = 1, 5, 9

(NumPy evaluates `mu**4` through `powf`, which may differ from the square of the square by one unit in the last place: far inside the
float32 noise of the reference, and not something a second implementation can be held to.)  The reference adds these up one after
the other in float32, which is its noise (1.9e-7 .. 5.7e-5 of a block's largest entry on 8^3 .. 16^3 meshes); the sums here are float64.

Two defects of the reference are not reproduced:

1.  `for i in range(len(kout))` (:109) writes `nmodes_in[nkout]`, one past the end.  Numba does that silently, plain Python raises
    `IndexError`.  The element is never used; the loop here ends at `nkout`.
2.  A mode below `kout[0]` gets the index -1, which Python wraps to the LAST row of the l = 4 block (and `nmodes_out[-1::nkout]` to
    its count).  With `logk` edges this happens to the k = 0 mode; on an 8^3 mesh it changes that block by 0.5 - 0.96 of its largest
    entry.  Here such modes are left out, like the modes at and beyond the last edge.
"""
import ctypes as C
import os
from pathlib import Path

import numpy as np

from ... import _lib
from ..._lib import check, ptr
from ...analysis.power_spectrum import get_k_mu_edges

__all__ = ['mesh_wavenumbers', 'window_moments', 'assemble_window', 'periodic_window_function', 'window_path', 'save_window']

MAX_NMESH = 32766      # csrc/window.hip
MAX_BINS = 4096


def _check_mesh(nmesh, lbox):
    if isinstance(nmesh, bool) or not isinstance(nmesh, (int, np.integer)):
        raise ValueError(f'nmesh must be an integer, got {nmesh!r}')
    if nmesh <= 0 or nmesh % 2 or nmesh > MAX_NMESH:
        raise ValueError(f'nmesh must be even and in 2 .. {MAX_NMESH}, got {nmesh}')
    lbox = float(lbox)
    if not np.isfinite(lbox) or lbox <= 0:
        raise ValueError(f'lbox must be positive and finite, got {lbox}')
    return int(nmesh), lbox


def _check_kout(kout):
    kout = np.ascontiguousarray(kout, dtype=np.float64)
    if kout.ndim != 1 or len(kout) < 2:
        raise ValueError('kout must hold at least 2 bin edges')
    if not np.isfinite(kout).all():
        raise ValueError('kout must be finite')
    if not (np.diff(kout) > 0).all():
        raise ValueError('kout must be strictly increasing')
    if len(kout) - 1 > MAX_BINS:
        raise ValueError(f'{len(kout) - 1} output bins, at most {MAX_BINS} are supported')
    return kout


def _check_kin(kin, k2weight):
    kin = np.asarray(kin, dtype=np.float64)
    if kin.ndim != 1:
        raise ValueError('kin must be one-dimensional')
    if not np.isfinite(kin).all():
        raise ValueError('kin must be finite')
    if k2weight and len(kin) < 2:
        raise ValueError('k2weight needs at least 2 kin (the weight is kin^2 times the spacing of kin)')
    return kin


def mesh_wavenumbers(nmesh, lbox):
    """The float32 wavenumbers of the mesh as reference :75-81 forms them: two `np.arange` in float32, the non-negative half and
    the negative half.  Its first `nmesh // 2` values are the half axis.  (Where rounding makes an `arange` one element longer
    than `nmesh // 2`, the reference raises on the assignment; the first `nmesh // 2` are taken here.)"""
    nmesh, lbox = _check_mesh(nmesh, lbox)
    half = nmesh // 2
    kvals = np.zeros(nmesh, dtype=np.float32)
    kvals[:half] = np.arange(0, 2 * np.pi * nmesh / lbox / 2, 2 * np.pi / lbox, dtype=np.float32)[:half]
    kvals[half:] = np.arange(-2 * np.pi * nmesh / lbox / 2, 0, 2 * np.pi / lbox, dtype=np.float32)[:half]
    return kvals


def window_moments(nmesh, lbox, kout):
    """The mesh pass, on the device: `dict(S, nmodes, ksum)` with `S` (nkout, 3, 3), `nmodes` (nkout,) and `ksum` (nkout,), all
    float64 - per output bin the sums of m fl32(fl32(pref_l L_l) L_l'), of m and of m knorm over the modes of the half mesh (module
    docstring).  `nmodes` is exact.  There is no CPU fallback."""
    kvals = mesh_wavenumbers(nmesh, lbox)
    kout = _check_kout(kout)
    nkout = len(kout) - 1
    S = np.zeros((nkout, 3, 3), dtype=np.float64)
    nmodes = np.zeros(nkout, dtype=np.float64)
    ksum = np.zeros(nkout, dtype=np.float64)
    check(_lib.lib().abacus_window_moments(C.c_int(int(nmesh)), ptr(kvals), ptr(kout), C.c_int(nkout), ptr(S), ptr(nmodes), ptr(ksum)))
    return dict(S=S, nmodes=nmodes, ksum=ksum)


def assemble_window(S, nmodes, ksum, kout, kin, k2weight=True):
    """`(window, keff)` from the moments of the mesh pass: pure NumPy.

        window[l nkout + o, l' nkin + beta] = S[o, l, l'] w[beta] / nmodes[o] / nmodes_in[o]   where digitize(kin[beta], kout) - 1 == o

    and exactly 0 elsewhere; `w = kin^2 dk` with `dk` the forward difference of `kin` (its last value repeated) when `k2weight`, else
    1; `nmodes_in[o]` the sum of `w` over the columns of bin `o`, held in float32 as the reference holds it (:107-117), and its
    reciprocal taken in float32 (0 for a bin without columns); `keff = ksum / nmodes`.  Rows of bins without modes are 0.  Both are
    float64, `(3 nkout, 3 nkin)` and `(nkout,)`."""
    kout = _check_kout(kout)
    kin = _check_kin(kin, k2weight)
    nkout, nkin = len(kout) - 1, len(kin)
    S = np.asarray(S, dtype=np.float64)
    nmodes = np.asarray(nmodes, dtype=np.float64)
    ksum = np.asarray(ksum, dtype=np.float64)
    if S.shape != (nkout, 3, 3) or nmodes.shape != (nkout,) or ksum.shape != (nkout,):
        raise ValueError(f'S, nmodes, ksum must have shapes ({nkout}, 3, 3), ({nkout},), ({nkout},)')
    if k2weight:
        dk = np.zeros_like(kin)
        dk[:-1] = kin[1:] - kin[:-1]
        dk[-1] = dk[-2]
        w = kin ** 2 * dk
    else:
        w = np.ones(nkin, dtype=np.float64)
    idx_i = np.digitize(kin, kout) - 1
    nmodes_in = np.zeros(nkout, dtype=np.float32)
    for o in range(nkout):          # (the reference's loop runs one further, past the end of nmodes_in)
        nmodes_in[o] = np.sum(w[idx_i == o])
    with np.errstate(divide='ignore'):
        norm_in = np.float32(1) / nmodes_in
        norm_out = 1.0 / nmodes
    norm_in[nmodes_in == 0] = 0
    norm_out[nmodes == 0] = 0
    norm_in = norm_in.astype(np.float64)
    window = np.zeros((3 * nkout, 3 * nkin), dtype=np.float64)
    cols = np.nonzero((idx_i >= 0) & (idx_i < nkout))[0]
    o = idx_i[cols]
    for ell in range(3):
        for ellp in range(3):
            window[ell * nkout + o, ellp * nkin + cols] = S[o, ell, ellp] * w[cols] * norm_out[o] * norm_in[o]
    return window, ksum * norm_out


def periodic_window_function(nmesh, lbox, kout, kin, k2weight=True):
    """The matrix that convolves a finely evaluated theory prediction with the mode coupling of a periodic box: `np.dot(window,
    pell_th)` is the convolved theory (reference :48-181, same arguments and returns).

    `nmesh`: size of the mesh of the power-spectrum measurement (even); `lbox`: box size; `kout`: the k bin edges of the
    measurement; `kin`: the k values of the theory; `k2weight`: weight the columns by `kin^2 dk`.  Returns `window` (float64,
    `(3 nkout, 3 nkin)`, blocks in the order l = 0, 2, 4) and `keff` (float64, `(nkout,)`), the effective k of each output bin.
    Differences to the reference (float64 sums; its two indexing defects) are in the module docstring.  Raises `ValueError` for an odd
    or non-positive `nmesh`, edges that are not strictly increasing or fewer than 2, `k2weight` with fewer than 2 `kin`, and
    non-finite inputs - before the device is touched."""
    _check_mesh(nmesh, lbox)
    kout = _check_kout(kout)
    kin = _check_kin(kin, k2weight)
    m = window_moments(nmesh, lbox, kout)
    return assemble_window(m['S'], m['nmodes'], m['ksum'], kout, kin, k2weight=k2weight)


def window_path(zcv_dir, sim_name, nmesh, k_bins, logk):
    """The file `run_zcv` loads the window from (reference :386-397, tools_cv.py:588-600): `<zcv_dir>/<sim_name>/window_nmesh{n}.npz`
    when there are `nmesh // 2` bins, else `..._dk{dk:.3f}.npz` with `dk` the width of the first bin (`logk`: of its logarithm)."""
    k_bins = np.asarray(k_bins, dtype=np.float64)
    save_dir = Path(zcv_dir) / sim_name
    if len(k_bins) - 1 == nmesh // 2:
        return save_dir / f'window_nmesh{nmesh:d}.npz'
    dk = np.log(k_bins[1] / k_bins[0]) if logk else k_bins[1] - k_bins[0]
    return save_dir / f'window_nmesh{nmesh:d}_dk{dk:.3f}.npz'


def save_window(zcv_dir, sim_name, nmesh, Lbox, k_hMpc_max, n_k_bins, logk=False, overwrite=False):
    """Writes the window file of one box and mesh as the reference's `main` does (:381-383, :447-456): edges from `get_k_mu_edges`,
    `kin` the bin centres, `k2weight=True`, `np.savez(window=..., keff=...)`.  An existing file is left alone unless `overwrite`.
    Returns the path."""
    k_bins, _ = get_k_mu_edges(Lbox, k_hMpc_max, int(n_k_bins), 1, logk)
    k_binc = (k_bins[1:] + k_bins[:-1]) * 0.5
    fn = window_path(zcv_dir, sim_name, nmesh, k_bins, logk)
    if os.path.exists(fn) and not overwrite:
        return fn
    window, keff = periodic_window_function(nmesh, Lbox, k_bins, k_binc, k2weight=True)
    os.makedirs(fn.parent, exist_ok=True)
    np.savez(fn, window=window, keff=keff)
    return fn
