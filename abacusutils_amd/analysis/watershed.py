"""Watershed voids of the density field on the MI355X: the zones of steepest descent of ZOBOV (Neyrinck 2008) / VIDE on a mesh, as the
voxel finder of REVOLVER takes them, the saddle tree between them, the ZOBOV hierarchy and the 0-dimensional persistence pairs that
follow from it.  The reference has no void finder; no reference code stands behind this module - its arithmetic is stated in
include/abacus_hip.h and pinned to the NumPy statement tests/watershed_statement.py.  Every decision is an integer comparison.

1. Mesh.  A periodic float32 mesh of n^3 cells, a = L / n, flat index f = (x n + y) n + z; n even, 4 .. 1024, so f < 2^30.  The key of
   a cell is (value, f), by value first, compared in float32; -0.0 and +0.0 are one value: a strict total order.
2. Descent.  `connectivity` 6 (faces) or 26 (faces, edges, corners).  down[c] = the cell of smallest key among c and its periodic
   neighbours; a cell with down[c] == c is a core.
3. Zones.  The zone of c is the core reached by following down; zones are numbered 0 .. Z - 1 in ascending flat index of their core;
   `labels` is the int32 (n, n, n) array of zone numbers.
4. Zone properties.  `ncell` int64; `core` int32 x 3; `delta_min` float32, the keyed value (-0.0 comes back as +0.0); `offset_sum`
   int64 x 3, per axis the sum over the zone's cells of (c - core) mod n, minus n where that is >= n / 2 - exact; `delta_sum` float64,
   the sum of its cells' values in no fixed order, the only inexact output.  On the host, in float64: volume = ncell a^3, radius =
   (3 volume / 4 pi)^(1/3), centres = (core + offset_sum / ncell) a mod L, delta_mean = delta_sum / ncell.
5. Saddle tree.  An edge is a pair of adjacent cells (the same connectivity) in different zones; `hi` is the cell of the larger key,
   `lo` the other; the weight (key(hi), key(lo)), compared lexicographically, is unique per cell pair.  The saddle tree is the minimum
   spanning tree of the zone graph under these weights: Z - 1 edges (the torus is connected), unique.  Per edge `hi_cell`, `lo_cell`
   (int64 flat indices), `zone_hi`, `zone_lo` (int32), `saddle` (float32, the value at hi), in ascending weight - the order in which
   rising water joins basins.
6. Hierarchy (`zone_hierarchy`, host).  The edges in order with a union-find over zones; a component's founder is its zone of smallest
   core key.  When P and Q join with founder(P) deeper than founder(Q), founder(Q) gets `parent` = founder(P), `saddle`,
   `saddle_cell` and `ncell_at_merge`, `nzones_at_merge`: Q's totals at that moment - the ZOBOV void of that zone.  The deepest zone
   of the box gets parent -1, saddle +inf and ncell n^3.  In float64 from the float32 values: `persistence` = saddle - delta_min,
   `ratio` = (1 + saddle) / (1 + delta_min) for a density contrast.  `persistence_pairs`: (birth = delta_min, death = saddle), the
   H0 persistence diagram of the sublevel sets.
7. `merge_zones(result, saddle_max)` (host).  The void of a zone is its component in the tree restricted to the edges with saddle <
   float32(saddle_max) - VIDE's link threshold 0.2 rho_mean at saddle_max = -0.8.  Voids are numbered in ascending number of their
   deepest zone.

Limits: n even, 4 .. 1024; connectivity 6 or 26; a host mesh must be finite (checked), a device mesh is not checked.  The hierarchy,
the merging and the statistics below are host loops over the zones.

Not built: light cones and masks, float64 meshes, multi-GPU slabs, particle-level (Voronoi) ZOBOV, profiles stacked in r / R_v, zones
across tracers, per-galaxy zone membership (a host lookup in `labels`), higher-dimensional persistence (H1, H2).  There is no CPU
fallback.
"""
import ctypes as C
import math

import numpy as np

from .. import _lib
from .._lib import DeviceArray, check, ptr

__all__ = ['watershed_mesh', 'find_watershed_voids', 'zone_hierarchy', 'merge_zones', 'persistence_pairs', 'watershed_size_function',
           'zone_galaxy_xi']

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
        raise ValueError(f'nmesh = {n}: the watershed needs an even mesh of {MIN_MESH} .. {MAX_MESH} cells per side')
    return n


def _connectivity(c):
    if c not in (6, 26):
        raise ValueError(f'connectivity must be 6 (faces) or 26 (faces, edges and corners), got {c}')
    return int(c)


def _smoothing(R):
    R = float(R)
    if not (R >= 0 and np.isfinite(R)):
        raise ValueError(f'R must be finite and not negative, got {R}')
    return R


def _mesh(field):
    """(n, pitch) of a float32 (n, n, n) NumPy array or a dense (n, n, n) or padded (n, n, pitch) DeviceArray"""
    if not hasattr(field, 'shape') or not hasattr(field, 'dtype'):
        raise TypeError(f'the mesh must be a float32 (n, n, n) array or DeviceArray, got {type(field).__name__}')
    shape = tuple(field.shape)
    if np.dtype(field.dtype) != np.float32:
        raise TypeError(f'the mesh must be float32, got {field.dtype}')
    if len(shape) != 3 or shape[0] != shape[1]:
        raise ValueError(f'the mesh must be cubic, (n, n, n), got shape {shape}')
    n = _nmesh(shape[0])
    if isinstance(field, DeviceArray):
        if shape[2] != n and shape[2] != (n + 2 + 31) // 32 * 32:
            raise ValueError(f'a device mesh must be dense, (n, n, n), or padded, (n, n, {(n + 2 + 31) // 32 * 32}), got shape {shape}')
        return n, shape[2]
    if shape[2] != n:
        raise ValueError(f'the mesh must be cubic, (n, n, n), got shape {shape}')
    if not np.isfinite(field).all():
        raise ValueError('the mesh holds NaN or inf')
    return n, n


# ------------------------------------------------------------------------------------------------- the finder on a resident mesh
def _run(mesh_ptr, n, pitch, L, connectivity, return_labels):
    lib = _lib.lib()
    handle = C.c_void_p()
    check(lib.abacus_ws_create(n, connectivity, C.byref(handle)))
    try:
        nz, rounds, jumps = C.c_int64(0), C.c_int(0), C.c_int(0)
        check(lib.abacus_ws_run_dev(handle, mesh_ptr, int(pitch), C.byref(nz), C.byref(rounds), C.byref(jumps)))
        Z = nz.value
        ncell, core, dmin = np.zeros(Z, dtype=np.int64), np.zeros((Z, 3), dtype=np.int32), np.zeros(Z, dtype=np.float32)
        osum, dsum = np.zeros((Z, 3), dtype=np.int64), np.zeros(Z, dtype=np.float64)
        check(lib.abacus_ws_fetch_zones(handle, ptr(ncell), ptr(core), ptr(dmin), ptr(osum), ptr(dsum)))
        hi, lo = np.zeros(Z - 1, dtype=np.int64), np.zeros(Z - 1, dtype=np.int64)
        zh, zl, saddle = np.zeros(Z - 1, dtype=np.int32), np.zeros(Z - 1, dtype=np.int32), np.zeros(Z - 1, dtype=np.float32)
        check(lib.abacus_ws_fetch_tree(handle, ptr(hi), ptr(lo), ptr(zh), ptr(zl), ptr(saddle)))
        out = dict(ncell=ncell, core=core, delta_min=dmin, offset_sum=osum, delta_sum=dsum, hi_cell=hi, lo_cell=lo, zone_hi=zh, zone_lo=zl,
                   saddle=saddle, nzones=Z, rounds=rounds.value)
        if return_labels:
            labels = np.zeros((n, n, n), dtype=np.int32)
            check(lib.abacus_ws_fetch_labels(handle, ptr(labels)))
            out['labels'] = labels
    finally:
        lib.abacus_ws_free(handle)
    if int(ncell.sum()) != n**3:
        raise _lib.AbacusHipError(f'watershed: the zones hold {int(ncell.sum())} of {n**3} cells')
    out.update(_derived(out, L, n))
    return out


def _derived(z, L, n):
    """step 4 of the module docstring, the host part"""
    a = L / n
    nc = z['ncell'].astype(np.float64)
    volume = nc * a**3
    return dict(volume=volume, radius=np.cbrt(3.0 * volume / (4.0 * math.pi)),
                centres=np.mod((z['core'].astype(np.float64) + z['offset_sum'].astype(np.float64) / nc[:, None]) * a, L),
                delta_mean=z['delta_sum'] / nc, Lbox=L, nmesh=n)


# ------------------------------------------------------------------------------------------------- the public interface
def watershed_mesh(field, Lbox, connectivity=26, return_labels=False):
    """Steps 1 to 5 of the module docstring on a float32 (n, n, n) NumPy array (checked to be finite) or a dense (n, n, n) or padded
    (n, n, pitch) `DeviceArray`; not modified.

    Returns dict(ncell, core, delta_min, offset_sum, delta_sum, centres (Z, 3) float64 in [0, L), volume, radius, delta_mean; hi_cell,
    lo_cell, zone_hi, zone_lo, saddle (Z - 1 each, ascending weight); nzones; rounds: the rounds of the tree, for information; Lbox,
    nmesh) and, with `return_labels`, labels (n, n, n) int32."""
    L = _box(Lbox)
    conn = _connectivity(connectivity)
    n, pitch = _mesh(field)
    if isinstance(field, DeviceArray):
        return _run(field.ptr, n, pitch, L, conn, return_labels)
    dev = DeviceArray(np.ascontiguousarray(field, dtype=np.float32))
    try:
        return _run(dev.ptr, n, n, L, conn, return_labels)
    finally:
        dev.free()


def find_watershed_voids(pos, Lbox, R, nmesh=256, w=None, paste='TSC', compensated=True, interlaced=True, connectivity=26, min_radius=0.0,
                         saddle_max=None, return_field=False, return_labels=False):
    """The watershed voids of the density contrast of the particles `pos` in the periodic box of side `Lbox`, smoothed with a Gaussian
    of radius `R` (units of Lbox; 0: none) exactly as `calc_minkowski` smooths it (`abacus_zcv_spectrum_dev`, then
    `abacus_mf_smooth_spectrum_dev`).  The mesh stays in HBM.

    `pos`: (N, 3) NumPy float32 / float64, an (N, 3) float32 `DeviceArray`, or three float64 `DeviceArray` columns
    (`MockDict.device_xyz`); not modified - the deposit works on a wrapped float32 copy.  `w`: per-particle weights or None.

    Returns the dict of `watershed_mesh` plus hierarchy: the dict of `zone_hierarchy`, keep (Z,) bool: radius >= min_radius, with
    `saddle_max` merged: the dict of `merge_zones`, and with `return_field` field: the float32 (n, n, n) mesh the decisions were
    taken on."""
    from ..hod.zcv.reconstruction import _positions, _working_copy
    from .power_spectrum import _paste_code, get_W_compensated
    L, n, conn, R = _box(Lbox), _nmesh(nmesh), _connectivity(connectivity), _smoothing(R)
    min_radius = float(min_radius)
    if not (min_radius >= 0 and np.isfinite(min_radius)):
        raise ValueError(f'min_radius must be finite and not negative, got {min_radius}')
    if saddle_max is not None:
        saddle_max = _saddle_max(saddle_max)
    code = _paste_code(paste, ':')
    npart = _positions(pos, 'pos')
    if w is not None:
        w = np.ascontiguousarray(w, dtype=np.float32)
        if w.shape != (npart,):
            raise ValueError(f'the weights have shape {w.shape}, expected ({npart},)')
    W = np.ascontiguousarray(get_W_compensated(L, n, paste, bool(interlaced)), dtype=np.float32) if compensated else None
    lib = _lib.lib()
    check(lib.abacus_ws_check_memory(n, C.c_int64(npart)))
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
        out = _run(spec.ptr, n, pitch, L, conn, return_labels)
        if return_field:
            out['field'] = np.ascontiguousarray(spec.get()[:, :, :n])
    finally:
        for a in (spec, work, wdev):
            if a is not None:
                a.free()
    out['hierarchy'] = zone_hierarchy(out)
    out['keep'] = out['radius'] >= min_radius
    if saddle_max is not None:
        out['merged'] = merge_zones(out, saddle_max)
    return out


# ------------------------------------------------------------------------------------------------- host helpers
def _saddle_max(s):
    s = float(s)
    with np.errstate(over='ignore'):
        s32 = np.float32(s)
    if np.isnan(s) or np.isnan(s32):
        raise ValueError('saddle_max must not be NaN')
    return s32


def _find(parent, a):
    while parent[a] != a:
        parent[a] = parent[parent[a]]
        a = parent[a]
    return a


def _zones_and_tree(result):
    try:
        z = {k: np.asarray(result[k]) for k in ('ncell', 'core', 'delta_min', 'offset_sum', 'hi_cell', 'zone_hi', 'zone_lo', 'saddle')}
        n = int(result['nmesh'])
    except (KeyError, TypeError, IndexError) as e:
        raise ValueError(f'a result of watershed_mesh or find_watershed_voids is expected: {e!r}') from None
    Z = len(z['ncell'])
    if Z < 1 or len(z['zone_hi']) != Z - 1 or len(z['zone_lo']) != Z - 1 or len(z['saddle']) != Z - 1 or len(z['hi_cell']) != Z - 1:
        raise ValueError(f'{Z} zones need a tree of {Z - 1} edges')
    return z, Z, n


def zone_hierarchy(result):
    """Step 6 of the module docstring from a result of `watershed_mesh`.  Host only: a loop over the Z - 1 edges.

    Returns dict(parent (Z,) int32, saddle (Z,) float32, saddle_cell (Z,) int64 (-1 for the deepest zone), ncell_at_merge,
    nzones_at_merge (Z,) int64, persistence, ratio (Z,) float64)."""
    z, Z, n = _zones_and_tree(result)
    core = z['core'].astype(np.int64)
    flat = (core[:, 0] * n + core[:, 1]) * n + core[:, 2]
    dmin = np.where(z['delta_min'] == 0, np.float32(0), z['delta_min'])
    depth = np.empty(Z, dtype=np.int64)
    depth[np.lexsort((flat, dmin))] = np.arange(Z)                   # a zone's place in the order of the core keys
    parent, saddle = np.full(Z, -1, dtype=np.int32), np.full(Z, np.inf, dtype=np.float32)
    saddle_cell, ncell_at, nzones_at = np.full(Z, -1, dtype=np.int64), np.zeros(Z, dtype=np.int64), np.zeros(Z, dtype=np.int64)
    uf, founder = list(range(Z)), list(range(Z))
    ncell, nzones = [int(c) for c in z['ncell']], [1] * Z
    zh, zl, depth = z['zone_hi'].tolist(), z['zone_lo'].tolist(), depth.tolist()
    for e in range(Z - 1):
        p, q = _find(uf, zh[e]), _find(uf, zl[e])
        if p == q:
            raise ValueError(f'edge {e} joins two zones of one component: not a tree')
        if depth[founder[q]] < depth[founder[p]]:
            p, q = q, p
        fq = founder[q]
        parent[fq], saddle[fq], saddle_cell[fq] = founder[p], z['saddle'][e], z['hi_cell'][e]
        ncell_at[fq], nzones_at[fq] = ncell[q], nzones[q]
        uf[q] = p
        ncell[p] += ncell[q]
        nzones[p] += nzones[q]
    top = _find(uf, 0)
    ncell_at[founder[top]], nzones_at[founder[top]] = ncell[top], nzones[top]
    d64, s64 = z['delta_min'].astype(np.float64), saddle.astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = (1.0 + s64) / (1.0 + d64)
    return dict(parent=parent, saddle=saddle, saddle_cell=saddle_cell, ncell_at_merge=ncell_at, nzones_at_merge=nzones_at,
                persistence=s64 - d64, ratio=ratio)


def persistence_pairs(result):
    """float32 (Z, 2): (birth = delta_min, death = saddle) of every zone, the H0 persistence diagram of the sublevel sets of the mesh;
    the deepest zone never dies (+inf).  `result`: of `watershed_mesh` or `find_watershed_voids`."""
    saddle = (result['hierarchy'] if 'hierarchy' in result else zone_hierarchy(result))['saddle']
    return np.stack([np.asarray(result['delta_min'], dtype=np.float32), np.asarray(saddle, dtype=np.float32)], axis=1)


def merge_zones(result, saddle_max):
    """Step 7 of the module docstring.  Host only.

    Returns dict(void (Z,) int32: the void of every zone; nvoids; ncell (V,) int64, volume, radius (V,) float64; zone (V,) int32: the
    deepest zone of every void; core (V, 3) int32 and delta_min (V,) float32: that zone's; centres (V, 3) float64 in [0, L): the
    barycentre (core_d + sum_z [ncell_z mi(core_z - core_d) + offset_sum_z] / sum_z ncell_z) a mod L over the void's zones z, d its
    deepest zone, mi the integer minimum image ((c) mod n, minus n where that is >= n / 2), in float64)."""
    s32 = _saddle_max(saddle_max)
    z, Z, n = _zones_and_tree(result)
    L = _box(result['Lbox'])
    core = z['core'].astype(np.int64)
    flat = (core[:, 0] * n + core[:, 1]) * n + core[:, 2]
    dmin = np.where(z['delta_min'] == 0, np.float32(0), z['delta_min'])
    depth = np.empty(Z, dtype=np.int64)
    depth[np.lexsort((flat, dmin))] = np.arange(Z)
    uf = list(range(Z))
    zh, zl = z['zone_hi'].tolist(), z['zone_lo'].tolist()
    for e in np.flatnonzero(z['saddle'] < s32).tolist():
        p, q = _find(uf, zh[e]), _find(uf, zl[e])
        if depth[q] < depth[p]:
            p, q = q, p
        uf[q] = p                                                    # the root of a component is its deepest zone
    deepest = np.array([_find(uf, k) for k in range(Z)], dtype=np.int64)
    zone = np.unique(deepest)
    void = np.searchsorted(zone, deepest).astype(np.int32)
    V = len(zone)
    nc = z['ncell'].astype(np.int64)
    ncell = np.zeros(V, dtype=np.int64)
    np.add.at(ncell, void, nc)
    shift = (core - core[deepest]) % n
    shift = np.where(shift >= n // 2, shift - n, shift)
    moment = np.zeros((V, 3), dtype=np.float64)
    np.add.at(moment, void, nc[:, None].astype(np.float64) * shift.astype(np.float64) + z['offset_sum'].astype(np.float64))
    a = L / n
    volume = ncell.astype(np.float64) * a**3
    return dict(void=void, nvoids=V, ncell=ncell, volume=volume, radius=np.cbrt(3.0 * volume / (4.0 * math.pi)), zone=zone.astype(np.int32),
                core=z['core'][zone].astype(np.int32), delta_min=z['delta_min'][zone].astype(np.float32),
                centres=np.mod((core[zone].astype(np.float64) + moment / ncell[:, None].astype(np.float64)) * a, L))


def watershed_size_function(radius, bins, Lbox):
    """The size function of zones or voids: dn/dlnR = N_b / (L^3 ln(bins[b + 1] / bins[b])) for the N_b radii with bins[b] <= radius <
    bins[b + 1], with the Poisson error sqrt(N_b) over the same denominator, at the geometric bin centres.  Host only.

    Returns dict(R, dn_dlnR, error, counts)."""
    L = _box(Lbox)
    bins = np.asarray(bins, dtype=np.float64)
    if bins.ndim != 1 or bins.size < 2 or not (np.isfinite(bins).all() and (bins > 0).all() and (np.diff(bins) > 0).all()):
        raise ValueError('bins must be at least two finite, positive, strictly increasing edges')
    r = np.asarray(radius, dtype=np.float64)
    if r.ndim != 1 or not np.isfinite(r).all() or (r < 0).any():
        raise ValueError('the radii must be a 1-D array of finite, non-negative values')
    counts = np.bincount(np.searchsorted(bins, r, side='right'), minlength=bins.size + 1)[1:bins.size].astype(np.int64)
    den = L**3 * np.log(bins[1:] / bins[:-1])
    N = counts.astype(np.float64)
    return dict(R=np.sqrt(bins[1:] * bins[:-1]), dn_dlnR=N / den, error=np.sqrt(N) / den, counts=counts)


def zone_galaxy_xi(result, X, Y, Z, Lbox, bins, select=None):
    """The zone-galaxy cross-correlation xi(r) = DD / (N_z N_g dV / L^3) - 1 with dV = 4 pi (r_hi^3 - r_lo^3) / 3, from the cross pair
    counts `DD(autocorr=0, ...)` of the centres (first set) and the galaxies, in float64 on the host, as `void_galaxy_xi` forms it.
    `result`: any dict with `centres` (a result of `watershed_mesh`, `find_watershed_voids` or `merge_zones`); `select`: None, a
    boolean mask or the indices of the centres to stack (`keep`, for one).  X, Y, Z: the galaxies' columns as `DD` takes them.

    Returns dict(r (the bin centres), xi, npairs uint64, nzones, ngal)."""
    L = _box(Lbox)
    bins = np.asarray(bins, dtype=np.float64)
    if bins.ndim != 1 or bins.size < 2 or not (np.diff(bins) > 0).all() or bins[0] < 0:
        raise ValueError('bins must be at least two increasing, non-negative edges')
    centres = np.asarray(result['centres'], dtype=np.float64)
    if centres.ndim != 2 or centres.shape[1] != 3:
        raise ValueError(f'centres must have shape (N, 3), got {centres.shape}')
    if select is not None:
        centres = centres[np.asarray(select)]
    nz, ng = len(centres), len(X)
    if nz == 0:
        raise ValueError('no zone to correlate')
    from .tpcf_corrfunc import DD
    c32 = [np.ascontiguousarray(centres[:, a], dtype=np.float32) for a in range(3)]
    res = DD(0, 1, bins, c32[0], c32[1], c32[2], X2=X, Y2=Y, Z2=Z, periodic=True, boxsize=L)
    npairs = res['npairs'].astype(np.uint64)
    dV = 4.0 * math.pi / 3.0 * (bins[1:] ** 3 - bins[:-1] ** 3)
    xi = npairs.astype(np.float64) / (float(nz) * float(ng) * dV / L**3) - 1.0
    return dict(r=0.5 * (bins[1:] + bins[:-1]), xi=xi, npairs=npairs, nzones=nz, ngal=ng)
