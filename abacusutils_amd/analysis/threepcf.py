"""Three-point correlation function multipoles zeta_l(r1, r2) on the MI355X: the multipole algorithm of Slepian & Eisenstein
(2015, MNRAS 454, 4142) on the periodic box (csrc/threepcf.hip: threepcf_walk, C ABI `abacus_threepcf[_dev]`) - the
configuration-space partner of `analysis.bispectrum.calc_bispectrum`.

The reference has none of this and Corrfunc has no 3PCF: the conventions are those of include/abacus_hip.h, pinned against the
NumPy statement tests/threepcf_statement.py (a brute-force sum over triplets and the algorithm itself).

  triplet_multipoles   the raw sums zeta[l][b1][b2] = sum_i w_i sum_{j in b1, k in b2, k != j} w_j w_k P_l(u_ij . u_ik), with
                       `wself` and the pair counts;
  zeta_from_counts     their normalisation by the expectation of an unclustered catalogue;
  calc_3pcf            the connected zeta_l(r1, r2) from D - R (randoms with weight -W / N_R appended as a second set: RRR of the
                       periodic box is analytic, no edge correction is needed), or the natural multipoles of the data alone.
"""
import ctypes as C

import numpy as np

from .. import _lib
from .._lib import check, ptr
from .spheres import random_centres
from .tpcf_corrfunc import _call_on_columns, _f4, _set_sizes

__all__ = ['triplet_multipoles', 'zeta_from_counts', 'calc_3pcf', 'last_stats']


def triplet_multipoles(X, Y, Z, boxsize, rbins, lmax, w=None, X2=None, Y2=None, Z2=None, w2=None):
    """The raw multipole sums of the catalogue (X, Y, Z, w) with the optional second set (X2, Y2, Z2, w2) appended to it by the
    library.  `rbins`: the nbins + 1 <= 33 float32 edges; 0 <= lmax <= 10; weights float32, None = 1, and may be negative.
    Returns {'zeta': (lmax + 1, nbins, nbins) float64, symmetric bit for bit in its last two axes; 'wself': (nbins,) float64, the
    j = k term already taken off the diagonal; 'npairs': (nbins,) uint64, the weighted pair counter's}.  Columns: host arrays, or
    all DeviceArray of one dtype (`_call_on_columns`); a host second set next to resident data is uploaded in the data's dtype
    and freed after the call."""
    rbins = np.atleast_1d(_f4(rbins))
    if rbins.ndim != 1:
        raise ValueError(f'rbins has shape {rbins.shape}, expected one dimension')
    given = [q is not None for q in (X2, Y2, Z2)]
    if any(given) and not all(given):
        raise ValueError('a second set needs X2, Y2 and Z2')
    if not (len(Y) == len(X) and len(Z) == len(X)):
        raise ValueError('X, Y and Z differ in length')
    if X2 is not None and not (len(Y2) == len(X2) and len(Z2) == len(X2)):
        raise ValueError('X2, Y2 and Z2 differ in length')
    second = [X2, Y2, Z2]
    own = []
    if X2 is not None and isinstance(X, _lib.DeviceArray) and not any(isinstance(q, _lib.DeviceArray) for q in second):
        own = [_lib.DeviceArray(np.ascontiguousarray(q, dtype=X.dtype)) for q in second]
        second = own
    nb, lmax = len(rbins) - 1, int(lmax)
    ok = 1 <= nb <= 32 and 0 <= lmax <= 10                # outside: the library refuses the call and writes nothing
    zeta = np.zeros((lmax + 1, nb, nb) if ok else 1, dtype=np.float64)
    wself = np.zeros(nb if ok else 1, dtype=np.float64)
    npairs = np.zeros(nb if ok else 1, dtype=np.uint64)
    cols = [X, Y, Z] + second
    as1d = lambda a: a if a is None or isinstance(a, _lib.DeviceArray) else np.asarray(a).ravel()   # noqa: E731
    weights = (as1d(w), as1d(w2))
    n1, n2 = _set_sizes(cols, weights)

    def call(fn, p, cols, wts, lab, geom, *dt):
        check(fn(*map(p, cols[:3]), p(wts[0]), C.c_int64(n1), *map(p, cols[3:]), p(wts[1]), C.c_int64(n2), *dt, *geom,
                 ptr(rbins), nb, lmax, ptr(zeta), ptr(wself), ptr(npairs)))
        return {'zeta': zeta, 'wself': wself, 'npairs': npairs}
    try:
        return _call_on_columns('threepcf', cols, weights, (), (C.c_float(boxsize),), call)
    finally:
        for a in own:
            a.free()


def last_stats():
    """{'candidates', 'counted', 'ncell'} of the last call: candidate pairs evaluated, counted pairs, cells per dimension"""
    cand, cnt, nc = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
    check(_lib.lib().abacus_threepcf_stats(C.byref(cand), C.byref(cnt), C.byref(nc)))
    return {'candidates': cand.value, 'counted': cnt.value, 'ncell': nc.value}


def zeta_from_counts(zeta_raw, wdata, boxsize, rbins):
    """(2l + 1) Z_l / (W nbar_w^2 V_b1 V_b2) with W = `wdata` = the sum of the data's weights, nbar_w = W / L^3 and V_b = 4 pi / 3
    (r_hi^3 - r_lo^3), everything in float64: the raw sums over the triplet count of an unclustered catalogue of the same
    weighted density, per unit of P_l - so that zeta(r1, r2, mu) = sum_l zeta_l(r1, r2) P_l(mu)."""
    Z = np.asarray(zeta_raw, dtype=np.float64)
    r = np.asarray(_f4(rbins), dtype=np.float64)
    if Z.ndim != 3 or Z.shape[1:] != (len(r) - 1, len(r) - 1):
        raise ValueError(f'zeta_raw has shape {Z.shape}, expected (lmax + 1, {len(r) - 1}, {len(r) - 1})')
    W = float(wdata)
    nbar = W / float(boxsize) ** 3
    V = 4.0 * np.pi / 3.0 * (r[1:] ** 3 - r[:-1] ** 3)
    ell = np.arange(Z.shape[0], dtype=np.float64)
    return (2.0 * ell + 1.0)[:, None, None] * Z / (W * nbar * nbar * V[:, None] * V[None, :])


def calc_3pcf(X, Y, Z, boxsize, rbins, lmax, w=None, randoms=None, seed=None):
    """zeta_l(r1, r2) of the data (X, Y, Z) with weights `w` (None: 1) in the periodic box.

    randoms: an int - that many `spheres.random_centres(randoms, boxsize, seed)` - or three columns.  The randoms are appended as
    a second set with weight -W / N_R each (W = sum of the data's weights): every point then carries the weight of the field
    D - R, whose triple product is the CONNECTED three-point function (Szapudi & Szalay's estimator with RRR analytic: the
    periodic box has no edge, so the denominator is the expectation `zeta_from_counts` divides by).
    randoms=None: the natural multipoles of the data alone, DDD / RRR per multipole.  These are the multipoles of the FULL
    three-point function 1 + xi(r1) + xi(r2) + xi(r12) + zeta, not of the connected part: l = 0 is close to 1 + xi(r1) + xi(r2)
    (1 for an unclustered catalogue), and xi(r12) feeds every l.

    Returns {'zeta': (lmax + 1, nbins, nbins) float64; 'zeta_raw', 'wself', 'npairs': of `triplet_multipoles`; 'ell';
    'r_mid': the bin centres; 'wdata': W; 'nrand'}."""
    n = len(X)
    if w is None:
        W = float(n)
    else:
        wh = w.get() if isinstance(w, _lib.DeviceArray) else np.asarray(w)
        W = float(np.sum(wh, dtype=np.float64))
    R, w2, nrand = (None, None, None), None, 0
    if randoms is not None:
        if isinstance(randoms, (int, np.integer)):
            if seed is None:
                raise ValueError('random centres need a seed')
            R = random_centres(int(randoms), boxsize, seed)
        else:
            R = list(randoms)
            if len(R) != 3:
                raise ValueError('randoms: an int, or three columns')
        nrand = len(R[0])
        if nrand < 1:
            raise ValueError('no randoms')
        w2 = np.full(nrand, -W / nrand, dtype=np.float32)   # (data without weights beside them: the library counts them with 1)
    raw = triplet_multipoles(X, Y, Z, boxsize, rbins, lmax, w=w, X2=R[0], Y2=R[1], Z2=R[2], w2=w2)
    r = np.asarray(_f4(rbins), dtype=np.float64)
    return {'zeta': zeta_from_counts(raw['zeta'], W, boxsize, rbins), 'zeta_raw': raw['zeta'], 'wself': raw['wself'],
            'npairs': raw['npairs'], 'ell': np.arange(int(lmax) + 1), 'r_mid': 0.5 * (r[1:] + r[:-1]), 'wdata': W, 'nrand': nrand}
