"""Galaxy-galaxy lensing on the MI355X: the excess surface density Delta Sigma(R) of the matter around galaxies in the periodic
box, projected along a box axis over the whole box (csrc/lens.hip: lens_walk, C ABI `abacus_lens_*`).

The matter particles of a fit never change, the galaxies do at every HOD evaluation: `ProjectedParticles` sorts the two
transverse particle columns once into a 2-D cell grid that stays in HBM, `projected_sums` walks it for one set of galaxies and
returns the pair counts and mass sums of the inner disc R < R_0 and of every bin, and `delta_sigma_from_sums` (NumPy, float64)
turns the sums into Sigma(R), the mean Sigma inside R and Delta Sigma.  `delta_sigma` does both, `delta_sigma_box` is the
one-shot form that also builds and frees the handle.

The reference has none of this: the conventions are those of include/abacus_hip.h, pinned against the NumPy statement
tests/lensing_statement.py.  A pair belongs to row 0 iff r2 < R_0^2, to row b + 1 iff R_b^2 <= r2 < R_{b+1}^2, all in float32.
A projection along the whole box does not see displacements along the line of sight, so redshift-space distortions along that
axis change nothing; for another axis pass real-space columns.
"""
import ctypes as C

import numpy as np

from .. import _lib
from .._lib import check, ptr
from .tpcf_corrfunc import _call_on_columns, _f4

MAX_BINS = 32
_AXES = {'x': (1, 2), 'y': (0, 2), 'z': (0, 1)}


def transverse_axes(los):
    """the two column indices transverse to the line of sight `los` ('x': (y, z), 'y': (x, z), 'z': (x, y))"""
    if los not in _AXES:
        raise ValueError(f"los must be 'x', 'y' or 'z' (got {los!r})")
    return _AXES[los]


def _edges(rp_bins, rmax=None):
    """the float32 edges after the rules of abacus_lens_profile"""
    edges = _f4(np.asarray(rp_bins))
    if edges.ndim != 1 or not 2 <= len(edges) <= MAX_BINS + 1:
        raise ValueError(f'rp_bins must be one dimension of 2 .. {MAX_BINS + 1} edges (got shape {edges.shape})')
    if not edges[0] > 0 or not np.all(np.diff(edges) > 0):
        raise ValueError('rp_bins must be positive and increasing (as float32)')
    if rmax is not None and edges[-1] > np.float32(rmax):
        raise ValueError(f'the last edge {edges[-1]} exceeds the rmax {rmax} the particles were sorted for')
    return edges


def _pair_of_columns(X, Y, w, what, wname):
    n = len(X)
    if len(Y) != n:
        raise ValueError(f'the two {what} columns differ in length')
    if w is not None and (len(getattr(w, 'shape', ())) != 1 or w.shape[0] != n):
        raise ValueError(f'{wname} has shape {tuple(getattr(w, "shape", ()))}, expected ({n},)')
    if n >= 2**31:
        raise ValueError(f'{what} counts must lie in [0, 2^31)')
    return n


class ProjectedParticles:
    """The particles' two transverse columns (X, Y) in HBM, sorted into the 2-D periodic cell grid of a reach of `rmax` in a box
    of side `boxsize` (abacus_lens_create): 8 bytes per particle, 12 with `mass` (float32 per particle; None: unit masses).
    Host arrays are cast to float32; or both columns are DeviceArray of one dtype (the rules of `_call_on_columns`, `mass` then
    a float32 DeviceArray or a host array).  Built once, it serves any number of `projected_sums` calls whose last edge is at
    most `rmax`.  `free()` releases the HBM (also at exit of a `with` block and at garbage collection); use after it raises."""

    def __init__(self, X, Y, boxsize, rmax, mass=None):
        self._h = C.c_void_p()
        self.boxsize, self.rmax = float(boxsize), float(rmax)
        if not np.float32(boxsize) > 0:
            raise ValueError('boxsize must be positive')
        if not np.float32(rmax) > 0 or np.float32(rmax) > np.float32(0.5) * np.float32(boxsize):
            raise ValueError('rmax must be positive and at most half the box (minimum image not unique beyond)')
        if mass is not None and not isinstance(mass, _lib.DeviceArray):
            mass = _f4(np.asarray(mass))
        self.n = _pair_of_columns(X, Y, mass, 'particle', 'mass')
        h = C.c_void_p()

        def call(fn, p, cols, w, lab, geom, *dt):
            check(fn(p(cols[0]), p(cols[1]), p(w[0]), C.c_int64(self.n), *dt, *geom, C.byref(h)))
        _call_on_columns('lens_create', [X, Y], (mass, None), (), (C.c_float(boxsize), C.c_float(rmax)), call)
        self._h = h
        total, n = C.c_double(0), C.c_int64(0)
        check(_lib.lib().abacus_lens_mass(self._h, C.byref(total), C.byref(n)))
        self.mass_sum = total.value          # sum(mass) in float64; n without masses

    def _handle(self):
        if not self._h:
            raise ValueError('these ProjectedParticles were freed')
        return self._h

    def free(self):
        if self._h:
            _lib.lib().abacus_lens_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def projected_sums(parts, GX, GY, rp_bins, weights=None):
    """{'npairs': uint64, 'wsum': float64}, each of length nb + 1, of the galaxies (GX, GY) (the same two transverse axes as the
    particles) around the particles of `parts`: row 0 is the inner disc R < rp_bins[0], row b + 1 the bin [rp_bins[b],
    rp_bins[b + 1]); wsum is the sum of galaxy weight x particle mass over the row's pairs (`weights`: float32 per galaxy, may
    be negative; None: unit weights).  Columns: host arrays, or both DeviceArray of one dtype - the columns of an HOD catalogue
    still in HBM."""
    if not isinstance(parts, ProjectedParticles):
        raise TypeError('parts must be ProjectedParticles')
    handle = parts._handle()
    edges = _edges(rp_bins, parts.rmax)
    if weights is not None and not isinstance(weights, _lib.DeviceArray):
        weights = _f4(np.asarray(weights))
    ng = _pair_of_columns(GX, GY, weights, 'galaxy', 'weights')
    nb = len(edges) - 1
    npairs, wsum = np.zeros(nb + 1, dtype=np.uint64), np.zeros(nb + 1, dtype=np.float64)

    def call(fn, p, cols, w, lab, geom, *dt):
        check(fn(handle, p(cols[0]), p(cols[1]), p(w[0]), C.c_int64(ng), *dt, ptr(edges), nb, ptr(npairs), ptr(wsum)))
        return {'npairs': npairs, 'wsum': wsum}
    return _call_on_columns('lens_profile', [GX, GY], (weights, None), (), (), call)


def walk_stats():
    """(candidate (galaxy, particle) pairs evaluated, cells per dimension) of the last `projected_sums` call"""
    cand, nc = C.c_uint64(0), C.c_int(0)
    check(_lib.lib().abacus_lens_stats(C.byref(cand), C.byref(nc)))
    return int(cand.value), int(nc.value)


def delta_sigma_from_sums(wsum, rp_bins, wgal, particle_mass=1.0):
    """Sigma and Delta Sigma from the mass sums of `projected_sums`, in NumPy float64.  With R the float32 edges as float64 and
    W = `wgal` the number of galaxies (or the sum of their weights):
        sigma[b]      = wsum[b + 1] / (W pi (R_{b+1}^2 - R_b^2))                  the mean surface density in bin b
        sigma_mean[j] = cumsum(wsum)[j] / (W pi R_j^2),  j = 0 .. nb              the mean surface density inside R_j
        rp_mid[b]     = sqrt(R_b R_{b+1})
        delta_sigma[b] = sigma_mean(< rp_mid[b]) - sigma[b]
    where sigma_mean(< rp_mid[b]) is interpolated between the two edges of the bin linearly in (log R, log sigma_mean) - the
    common halotools convention - or, where a value at an edge is not positive, linearly in log R of sigma_mean itself.
    `particle_mass` scales everything; the units are mass / length^2 of the inputs.  The uniform background
    (sigma_box of `delta_sigma`) is contained in sigma and in sigma_mean and cancels in delta_sigma."""
    R = _edges(rp_bins).astype(np.float64)
    wsum = np.asarray(wsum, dtype=np.float64)
    if wsum.shape != (len(R),):
        raise ValueError(f'wsum has shape {wsum.shape}, expected ({len(R)},): the inner disc and one row per bin')
    W = float(wgal)
    if not W != 0.0 or not np.isfinite(W):
        raise ValueError('wgal (the number of galaxies or the sum of their weights) must be finite and not zero')
    pm = float(particle_mass)
    sigma = pm * wsum[1:] / (W * np.pi * (R[1:] ** 2 - R[:-1] ** 2))
    sigma_mean = pm * np.cumsum(wsum) / (W * np.pi * R ** 2)
    rp_mid = np.sqrt(R[:-1] * R[1:])
    t = np.log(rp_mid / R[:-1]) / np.log(R[1:] / R[:-1])
    lo, hi = sigma_mean[:-1], sigma_mean[1:]
    inner = (1.0 - t) * lo + t * hi
    ok = (lo > 0) & (hi > 0)
    with np.errstate(divide='ignore', invalid='ignore'):
        loglog = np.exp((1.0 - t) * np.log(lo) + t * np.log(hi))
    inner = np.where(ok, loglog, inner)
    return {'sigma': sigma, 'sigma_mean': sigma_mean, 'delta_sigma': inner - sigma, 'rp_mid': rp_mid}


def _weight_total(weights, ng):
    if weights is None:
        return float(ng)
    w = weights.get() if isinstance(weights, _lib.DeviceArray) else _f4(np.asarray(weights))
    return float(np.sum(w, dtype=np.float64))


def delta_sigma(parts, GX, GY, rp_bins, weights=None, particle_mass=1.0):
    """`projected_sums` and `delta_sigma_from_sums` in one: their two dicts merged, with 'wgal' (the number of galaxies or the
    sum of `weights`) and 'sigma_box' = particle_mass sum(mass) / boxsize^2, the mean surface density of the box that sigma and
    sigma_mean contain and delta_sigma does not."""
    sums = projected_sums(parts, GX, GY, rp_bins, weights)
    wgal = _weight_total(weights, len(GX))
    out = dict(sums, **delta_sigma_from_sums(sums['wsum'], rp_bins, wgal, particle_mass))
    out['wgal'] = wgal
    out['sigma_box'] = float(particle_mass) * parts.mass_sum / parts.boxsize ** 2
    return out


def _columns(xyz, what):
    """three columns from an (n, 3) array or from a sequence of three columns"""
    if isinstance(xyz, np.ndarray):
        if xyz.ndim != 2 or xyz.shape[1] != 3:
            raise ValueError(f'{what} has shape {xyz.shape}, expected (n, 3) or three columns')
        return [xyz[:, d] for d in range(3)]
    cols = list(xyz)
    if len(cols) != 3:
        raise ValueError(f'{what}: expected (n, 3) or three columns')
    return cols


def delta_sigma_box(gal_xyz, part_xyz, boxsize, rp_bins, los='z', weights=None, mass=None, particle_mass=1.0, rmax=None):
    """One shot: Delta Sigma of the galaxies `gal_xyz` in the particles `part_xyz` (each an (n, 3) array or three columns, host
    or DeviceArray) projected along the box axis `los`; builds the particle handle for a reach of `rmax` (None: the last edge),
    profiles and frees it.  The result of `delta_sigma`.  In a fit keep a `ProjectedParticles` and call `delta_sigma`."""
    a, b = transverse_axes(los)
    edges = _edges(rp_bins)
    g, p = _columns(gal_xyz, 'gal_xyz'), _columns(part_xyz, 'part_xyz')
    with ProjectedParticles(p[a], p[b], boxsize, float(edges[-1]) if rmax is None else rmax, mass=mass) as parts:
        return delta_sigma(parts, g[a], g[b], edges, weights=weights, particle_mass=particle_mass)
