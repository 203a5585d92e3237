"""Pairwise velocity statistics on the MI355X: the mean pairwise infall v12(r), the radial and transverse pairwise dispersions
and the line-of-sight pairwise mean and dispersion in (rp, pi), from ONE pair walk over the periodic box (csrc/pairs.hip:
pair_vel, C ABI `abacus_pairvel[_dev]`).

`pairwise_velocity_sums` returns seven sums per (bin, sub-bin) - the pairs of a bin are exactly those of the weighted pair
counter (`tpcf_corrfunc._paircount_weighted`), so `npairs` and `wsum` are that counter's - and `moments_from_sums` (NumPy,
float64) turns them into the moments.  Per counted ordered pair (i, j), with d = p_i - p_j the minimum-image float32 separation
and u = v_i - v_j the float32 velocity difference, in float64:

    vr = u . d / |d|  (0 for a coincident pair; NEGATIVE = the pair approaches),   vz = u_z sign(d_z)  (the line of sight is z)
    wsum = sum w_i w_j     vr1 = sum w w vr     vr2 = sum w w vr^2     u2 = sum w w |u|^2     vz1 = sum w w vz     vz2 = sum w w u_z^2

The contract is written out in include/abacus_hip.h and restated in NumPy in tests/pairvel_statement.py.

The four wrappers at the end carry the names and the calling convention of halotools.mock_observables'
`mean_radial_velocity_vs_r`, `radial_pvd_vs_r`, `mean_los_velocity_vs_rp` and `los_pvd_vs_rp`.  halotools is not a dependency
and NO halotools run stands behind them: their definitions are the ones above (unit weights), pinned against the NumPy
statement only.
"""
import ctypes as C

import numpy as np

from .._lib import DeviceArray, check, ptr
from .tpcf_corrfunc import _call_on_columns, _f4

MODES = {'r': 0, 'rppi': 1, 'smu': 2}
SUMS = ('vr1', 'vr2', 'u2', 'vz1', 'vz2')     # the rows of the C entry's vsum block


def pairwise_velocity_sums(mode, X1, Y1, Z1, VX1, VY1, VZ1, boxsize, bins, X2=None, Y2=None, Z2=None, VX2=None, VY2=None,
                           VZ2=None, W1=None, W2=None, pimax=0.0, npibins=0, mu_max=1.0, nmubins=0):
    """{'npairs', 'wsum', 'vr1', 'vr2', 'u2', 'vz1', 'vz2'}: arrays of nbins * (1 | npibins | nmubins) entries, laid out like the
    pair counters' results.  mode: 0 | 'r', 1 | 'rppi', 2 | 'smu'.  Columns: host arrays (cast to float32) or - all twelve of
    them - `DeviceArray` columns of one dtype, float32 or float64 (rounded once to float32 on the device); mixing the two raises
    TypeError.  W1 / W2: float32 weights (None: unit weights), a host array or, next to resident columns, a DeviceArray.
    X2 is None: the autocorrelation (ordered pairs, no self pairs)."""
    mode = MODES.get(mode, mode)
    if mode not in (0, 1, 2):
        raise ValueError(f"mode must be one of 0, 1, 2, 'r', 'rppi', 'smu' (got {mode!r})")
    bins = _f4(np.asarray(bins))
    if bins.ndim != 1 or len(bins) < 2 or not np.all(np.diff(bins) > 0):
        raise ValueError('bins must be one dimension of at least two increasing edges (as float32)')
    half = np.float32(0.5) * np.float32(boxsize)
    if not np.float32(boxsize) > 0 or bins[-1] > half or (mode == 1 and np.float32(pimax) > half):
        raise ValueError('boxsize must be positive and the maximum separation at most half the box (minimum image not unique beyond)')
    nsub = 1 if mode == 0 else int(npibins if mode == 1 else nmubins)
    if nsub < 1:
        raise ValueError('need at least one pi / mu bin')
    arr = lambda a: a if a is None or isinstance(a, DeviceArray) else np.asarray(a)   # noqa: E731
    first, second = tuple(map(arr, (X1, Y1, Z1, VX1, VY1, VZ1))), tuple(map(arr, (X2, Y2, Z2, VX2, VY2, VZ2)))
    W1, W2 = arr(W1), arr(W2)
    auto = X2 is None
    if any(c is None for c in first) or (not auto and any(c is None for c in second)):
        raise ValueError('a set needs all six columns x, y, z, vx, vy, vz')
    if auto and (any(c is not None for c in second) or W2 is not None):
        raise ValueError('columns or weights of a second set given for an autocorrelation (X2 is None)')
    n1, n2 = len(first[0]), (0 if auto else len(second[0]))
    for name, cols, w, n in (('set 1', first, W1, n1), ('set 2', () if auto else second, W2, n2)):
        if any(len(c.shape) != 1 or c.shape[0] != n for c in cols):
            raise ValueError(f'the columns of {name} must be one dimension of one length')
        if w is not None and (len(w.shape) != 1 or w.shape[0] != n):
            raise ValueError(f'the weights of {name} have shape {tuple(w.shape)}, expected ({n},)')
    nb = len(bins) - 1
    ntot = nb * nsub
    npairs, wsum, vsum = np.zeros(ntot, np.uint64), np.zeros(ntot), np.zeros((5, ntot))
    tail = (C.c_float(boxsize), ptr(bins), nb, C.c_float(pimax), int(npibins), C.c_float(mu_max), int(nmubins), ptr(npairs),
            ptr(wsum), ptr(vsum))

    def call(fn, p, cols, w, lab, geom, *dt):
        check(fn(mode, *map(p, cols[:6]), p(w[0]), C.c_int64(n1), *map(p, cols[6:]), p(w[1]), C.c_int64(n2), *dt, *tail))
    _call_on_columns('pairvel', first + second, (W1, W2), (), (), call)
    return dict(npairs=npairs, wsum=wsum, **{k: vsum[q] for q, k in enumerate(SUMS)})


def moments_from_sums(sums):
    """The moments of the weighted pair distribution of every (bin, sub-bin), float64; NaN (no warning) where wsum == 0:
        v12       vr1 / wsum: the mean radial pairwise velocity, negative = infall
        sigma_r   sqrt(max(vr2 / wsum - v12^2, 0)): the radial pairwise dispersion about that mean
        sigma_t   sqrt(max((u2 - vr2) / (2 wsum), 0)): the transverse dispersion PER transverse direction (|u|^2 = vr^2 + the two
                  transverse components squared; the mean transverse velocity of an isotropic sample is zero)
        vlos      vz1 / wsum: the mean line-of-sight pairwise velocity (z), negative = approaching
        sigma_los sqrt(max(vz2 / wsum - vlos^2, 0))"""
    w = np.asarray(sums['wsum'], dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        mean = lambda k: np.where(w != 0, np.asarray(sums[k], dtype=np.float64) / w, np.nan)   # noqa: E731
        root = lambda a: np.where(w != 0, np.sqrt(np.maximum(a, 0.0)), np.nan)                 # noqa: E731
        v12, vlos = mean('vr1'), mean('vz1')
        return dict(v12=v12, sigma_r=root(mean('vr2') - v12 * v12), sigma_t=root(0.5 * (mean('u2') - mean('vr2'))), vlos=vlos,
                    sigma_los=root(mean('vz2') - vlos * vlos))


def _halotools_sums(mode, sample1, velocities1, bins, sample2, velocities2, period, **kw):
    """the sums for (N, 3) positions and velocities and a scalar period, unit weights"""
    if period is None or np.ndim(period) != 0:
        raise ValueError('period must be a scalar: the periodic box alone is supported')

    def six(s, v):
        if isinstance(s, np.ndarray) and isinstance(v, np.ndarray) and s.ndim == 2 and v.shape == s.shape and s.shape[1] == 3:
            return [np.ascontiguousarray(s[:, d]) for d in range(3)] + [np.ascontiguousarray(v[:, d]) for d in range(3)]
        raise ValueError('a sample and its velocities must be arrays of one shape (N, 3)')
    if (sample2 is None) != (velocities2 is None):
        raise ValueError('sample2 and velocities2 go together')
    second = {} if sample2 is None else dict(zip(('X2', 'Y2', 'Z2', 'VX2', 'VY2', 'VZ2'), six(np.asarray(sample2), np.asarray(velocities2))))
    return pairwise_velocity_sums(mode, *six(np.asarray(sample1), np.asarray(velocities1)), float(period), bins, **second, **kw)


def mean_radial_velocity_vs_r(sample1, velocities1, rbins, sample2=None, velocities2=None, period=None):
    """v12(r) per bin of `rbins`: the mean over the pairs of (v_1 - v_2) . (x_1 - x_2) / |x_1 - x_2|, negative = approaching.
    The name and the arguments of halotools.mock_observables.mean_radial_velocity_vs_r ((N, 3) arrays, a scalar `period`);
    no halotools run stands behind it (see the module docstring).  NaN for a bin without pairs."""
    return moments_from_sums(_halotools_sums(0, sample1, velocities1, rbins, sample2, velocities2, period))['v12']


def radial_pvd_vs_r(sample1, velocities1, rbins, sample2=None, velocities2=None, period=None):
    """sigma_r(r): the dispersion of the radial pairwise velocity about its mean per bin of `rbins` (halotools'
    radial_pvd_vs_r by name and arguments; no halotools run stands behind it).  NaN for a bin without pairs."""
    return moments_from_sums(_halotools_sums(0, sample1, velocities1, rbins, sample2, velocities2, period))['sigma_r']


def mean_los_velocity_vs_rp(sample1, velocities1, rp_bins, pi_max, sample2=None, velocities2=None, period=None):
    """The mean line-of-sight pairwise velocity (v_1z - v_2z) sign(z_1 - z_2) of the pairs with |pi| < pi_max per bin of
    `rp_bins`; the line of sight is z, negative = approaching (halotools' mean_los_velocity_vs_rp by name and arguments; no
    halotools run stands behind it).  NaN for a bin without pairs."""
    return moments_from_sums(_halotools_sums(1, sample1, velocities1, rp_bins, sample2, velocities2, period, pimax=float(pi_max),
                                             npibins=1))['vlos']


def los_pvd_vs_rp(sample1, velocities1, rp_bins, pi_max, sample2=None, velocities2=None, period=None):
    """The dispersion of the line-of-sight pairwise velocity about its mean, pairs with |pi| < pi_max per bin of `rp_bins`
    (halotools' los_pvd_vs_rp by name and arguments; no halotools run stands behind it).  NaN for a bin without pairs."""
    return moments_from_sums(_halotools_sums(1, sample1, velocities1, rp_bins, sample2, velocities2, period, pimax=float(pi_max),
                                             npibins=1))['sigma_los']
