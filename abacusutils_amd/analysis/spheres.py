"""Counts in spheres on the MI355X: for every query point the number of data points inside each of a set of radii, on the
periodic box (csrc/spheres.hip: sphere_count, C ABI `abacus_spherecount[_dev]`), and what is built from it - the void
probability function and the count probabilities P_N(r) (`vpf`, Corrfunc.theory.vpf's signature), the k-nearest-neighbour
CDFs (`knn_cdf`: P(N(<r) >= k)) in 3-D and in the (rp, pi) form, and the per-centre counts a counts-in-cells or
density-split analysis starts from (`count_in_spheres(..., return_counts=True)`).

The reference has none of this and Corrfunc is not vendored: the conventions are those of include/abacus_hip.h, pinned
against the NumPy statement tests/spheres_statement.py, whose column sums are the pair counter's cumulative counts.  A data
point is inside radius r iff r2 < float32(r) * float32(r) in float32 - strictly, like the upper edge of a pair bin.
"""
import ctypes as C

import numpy as np

from .. import _lib
from .._lib import check, ptr
from .tpcf_corrfunc import _call_on_columns, _f4


def count_in_spheres(X, Y, Z, boxsize, radii, QX=None, QY=None, QZ=None, pimax=None, kmax=8, return_counts=False):
    """N(<r_j) of the data (X, Y, Z) around every query (QX, QY, QZ) - around every data point, itself excluded, when no
    queries are given - for the increasing float32 `radii`; `pimax`: cylinders along z (rp < r_j, |dz| < pimax) instead of
    spheres.  Returns {'hist': (nr, kmax + 1) uint64 - hist[j, k] queries with exactly k points inside r_j, the last column
    those with kmax or more; 'nquery'; 'counts': (nquery, nr) uint32 in the order of the queries, or None unless
    `return_counts`}.  Columns: host arrays, or all DeviceArray of one dtype (`_call_on_columns`); host queries next to
    resident data are uploaded in the data's dtype and freed after the call."""
    radii = np.atleast_1d(_f4(radii))
    if radii.ndim != 1:
        raise ValueError(f'radii has shape {radii.shape}, expected one dimension')
    if pimax is not None and not pimax > 0:
        raise ValueError('pimax must be positive (None: spheres)')
    given = [q is not None for q in (QX, QY, QZ)]
    if any(given) and not all(given):
        raise ValueError('queries need QX, QY and QZ')
    data, queries = [X, Y, Z], [QX, QY, QZ]
    n = len(X)
    if not (len(Y) == n and len(Z) == n):
        raise ValueError('X, Y and Z differ in length')
    nq = n if QX is None else len(QX)
    if QX is not None and not (len(QY) == nq and len(QZ) == nq):
        raise ValueError('QX, QY and QZ differ in length')
    own = []
    if QX is not None and isinstance(X, _lib.DeviceArray) and not any(isinstance(q, _lib.DeviceArray) for q in queries):
        own = [_lib.DeviceArray(np.ascontiguousarray(q, dtype=X.dtype)) for q in queries]
        queries = own
    nr, kmax = len(radii), int(kmax)
    nh = nr * (kmax + 1)
    hist = np.zeros(nh if 0 < nh <= 8192 else 1, dtype=np.uint64)       # outside: the library refuses the call and writes nothing
    counts = np.zeros((nq, nr), dtype=np.uint32) if return_counts else None

    def call(fn, p, cols, w, lab, geom, *dt):
        check(fn(*map(p, cols[:3]), C.c_int64(n), *map(p, cols[3:]), C.c_int64(nq), *dt, *geom, ptr(radii), nr,
                 C.c_float(0.0 if pimax is None else pimax), kmax, ptr(hist), ptr(counts)))
        return {'hist': hist.reshape(nr, -1), 'nquery': nq, 'counts': counts}
    try:
        return _call_on_columns('spherecount', data + queries, (None, None), (), (C.c_float(boxsize),), call)
    finally:
        for a in own:
            a.free()


def random_centres(n, boxsize, seed):
    """n uniform centres in [0, boxsize)^3 as three float32 host columns, from np.random.default_rng(seed): one (n, 3) draw of
    float64, scaled and rounded.  This is this project's stream - NOT Corrfunc's GSL stream: a VPF agrees with Corrfunc's in
    distribution only (unpinned, like the rest of Corrfunc here)."""
    p = np.random.default_rng(seed).random((int(n), 3)) * float(boxsize)
    return [np.ascontiguousarray(p[:, d], dtype=np.float32) for d in range(3)]


def pn_from_hist(hist, nquery, numpN):
    """P_N(r_j) for N = 0 .. numpN - 1: hist[:, :numpN] / nquery, (nr, numpN) float64 (numpN <= kmax: exact counts only)"""
    hist = np.asarray(hist)
    if not 1 <= numpN <= hist.shape[1] - 1:
        raise ValueError(f'numpN = {numpN} must lie in [1, kmax = {hist.shape[1] - 1}]')
    return hist[:, :numpN].astype(np.float64) / float(nquery)


def cdf_from_hist(hist, nquery, ks):
    """P(N(<r_j) >= k) for every k of `ks`: (nquery - sum_{m<k} hist[:, m]) / nquery, (len(ks), nr) float64"""
    hist = np.asarray(hist)
    ks = [int(k) for k in ks]
    if not ks or min(ks) < 1 or max(ks) > hist.shape[1] - 1:
        raise ValueError(f'ks must lie in [1, kmax = {hist.shape[1] - 1}]')
    below = np.array([hist[:, :k].sum(axis=1, dtype=np.uint64) for k in ks], dtype=np.int64)
    return (int(nquery) - below).astype(np.float64) / float(nquery)


def vpf(rmax, nbins, nspheres, numpN, seed, X, Y, Z, verbose=False, periodic=True, boxsize=None):
    """Corrfunc.theory.vpf: the count probabilities P_0 (the void probability function) .. P_{numpN - 1} of `nspheres` random
    spheres of radii rmax (i + 1) / nbins, i = 0 .. nbins - 1.  A structured array with 'rmax' (f8) and 'pN' (f8, numpN per
    row).  The centres come from `random_centres(nspheres, boxsize, seed)`, one set for all radii."""
    if not periodic or boxsize is None:
        raise NotImplementedError('only periodic boxes with an explicit boxsize are supported')
    nbins, nspheres, numpN = int(nbins), int(nspheres), int(numpN)
    if nbins < 1 or nspheres < 1 or numpN < 1:
        raise ValueError('nbins, nspheres and numpN must be at least 1')
    radii = float(rmax) * (np.arange(nbins) + 1) / nbins
    res = count_in_spheres(X, Y, Z, boxsize, radii, *random_centres(nspheres, boxsize, seed), kmax=numpN)
    out = np.zeros(nbins, dtype=[('rmax', 'f8'), ('pN', 'f8', (numpN,))])
    out['rmax'] = radii
    out['pN'] = pn_from_hist(res['hist'], nspheres, numpN)
    return out


def knn_cdf(X, Y, Z, boxsize, radii, ks, QX=None, QY=None, QZ=None, nquery=None, seed=None, pimax=None):
    """the k-nearest-neighbour CDFs: the fraction of queries whose k-th nearest data point lies inside r, i.e. with
    N(<r) >= k, for every k of `ks` and r of `radii`: (len(ks), nr) float64 from ONE count with kmax = max(ks).  Queries:
    explicit (QX, QY, QZ), or `nquery` random centres of `seed`, or neither - the data themselves, self excluded.  `pimax`:
    the (rp, pi) form, cylinders of half-height pimax along z."""
    explicit, rand = QX is not None or QY is not None or QZ is not None, nquery is not None or seed is not None
    if explicit and rand:
        raise ValueError('give explicit queries, or nquery and seed, or neither (the data as queries) - not both')
    if rand:
        if nquery is None or seed is None:
            raise ValueError('random queries need nquery and seed')
        QX, QY, QZ = random_centres(nquery, boxsize, seed)
    ks = [int(k) for k in np.atleast_1d(ks)]
    if not ks or min(ks) < 1:
        raise ValueError('ks must be positive integers')
    res = count_in_spheres(X, Y, Z, boxsize, radii, QX, QY, QZ, pimax=pimax, kmax=max(ks))
    if res['nquery'] == 0:
        raise ValueError('no queries')
    return cdf_from_hist(res['hist'], res['nquery'], ks)
