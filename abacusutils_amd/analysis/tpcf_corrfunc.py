"""MI355X drop-in for `abacusnbody.analysis.tpcf_corrfunc` (reference: abacusnbody/analysis/tpcf_corrfunc.py).

The reference wraps the third-party Corrfunc pair counters; here `DD`, `DDrppi` and `DDsmu` are provided by the
HIP cell-list kernel (csrc/pairs.hip, C ABI `abacus_paircount`) with Corrfunc's calling conventions as used by the
reference, so the reference's own wrappers bind to them unchanged.  The four wrapper entry points the rest of abacusutils calls

    calc_xirppi_fast     (:97-203)      calc_wp_fast (:301-372)
    calc_multipole_fast  (:206-298)     tpcf_multipole (:17-94)

are kept as signatures over ONE shared estimator, `_natural_estimator` (float32 casts of coordinates and bins before
counting, analytic RR of the periodic box in the reference's dtype and operation order, xi = DD / RR - 1); their results
are pinned bit for bit against the reference's functions run with a brute-force Corrfunc stand-in
(tests/golden/pair_wrappers.npz, oracle/make_golden.py).

Corrfunc is not vendored in the reference and none of its tests cover these functions: parity of the pair counts is
pinned against the brute-force float32 counter of the oracle only ("parity unpinned" with respect to Corrfunc).
"""
import ctypes as C

import numpy as np

from .. import _lib
from .._lib import check, ptr


def _f4(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def _paircount(mode, X1, Y1, Z1, boxsize, bins, X2=None, Y2=None, Z2=None, pimax=0.0, npibins=0, mu_max=1.0,
               nmubins=0):
    """host arrays (cast to float32 like the reference, tpcf_corrfunc.py:134-139) or - all of them - `_lib.DeviceArray`
    columns of float32 / float64 already in HBM (the HOD catalogue: `abacus_paircount_dev`, no PCIe round trip)"""
    bins = _f4(bins)
    nb = len(bins) - 1
    nsub = 1 if mode == 0 else (npibins if mode == 1 else nmubins)
    out = np.zeros(nb * nsub, dtype=np.uint64)
    cols = [c for c in (X1, Y1, Z1, X2, Y2, Z2) if c is not None]
    if any(isinstance(c, _lib.DeviceArray) for c in cols):
        if not all(isinstance(c, _lib.DeviceArray) and c.dtype == cols[0].dtype for c in cols):
            raise TypeError('device-resident coordinates: every column must be a DeviceArray of one dtype')
        dt = {np.dtype(np.float32): 0, np.dtype(np.float64): 1}[cols[0].dtype]
        dp = lambda c: None if c is None else c.ptr     # noqa: E731
        check(_lib.lib().abacus_paircount_dev(
            int(mode), dp(X1), dp(Y1), dp(Z1), C.c_int64(X1.shape[0]), dp(X2), dp(Y2), dp(Z2),
            C.c_int64(0 if X2 is None else X2.shape[0]), dt, C.c_float(boxsize), ptr(bins), int(nb), C.c_float(pimax),
            int(npibins), C.c_float(mu_max), int(nmubins), ptr(out)))
        return out
    X1, Y1, Z1, X2, Y2, Z2 = map(_f4, (X1, Y1, Z1, X2, Y2, Z2))
    check(_lib.lib().abacus_paircount(
        int(mode), ptr(X1), ptr(Y1), ptr(Z1), C.c_int64(len(X1)), ptr(X2), ptr(Y2), ptr(Z2),
        C.c_int64(0 if X2 is None else len(X2)), C.c_float(boxsize), ptr(bins), int(nb), C.c_float(pimax),
        int(npibins), C.c_float(mu_max), int(nmubins), ptr(out)))
    return out


def _paircount_weighted(mode, X1, Y1, Z1, boxsize, bins, X2=None, Y2=None, Z2=None, W1=None, W2=None, pimax=0.0,
                        npibins=0, mu_max=1.0, nmubins=0, want_rsum=True):
    """`_paircount` with per-point float32 weights (None: unit weights): (npairs, wsum, rsum) per (bin, sub-bin) with
    wsum = sum of w_i * w_j and rsum = sum of the pair separation (r | rp | s), both accumulated in float64 on the device
    (`abacus_paircount_weighted[_dev]`); rsum is None when `want_rsum` is false.  A host weight array next to resident
    coordinates is uploaded (float32), resident weights next to host coordinates are not accepted."""
    bins = _f4(bins)
    nb = len(bins) - 1
    nsub = 1 if mode == 0 else (npibins if mode == 1 else nmubins)
    out = np.zeros(nb * nsub, dtype=np.uint64)
    wsum = np.zeros(nb * nsub, dtype=np.float64)
    rsum = np.zeros(nb * nsub, dtype=np.float64) if want_rsum else None
    if X2 is None and W2 is not None:
        raise ValueError('weights2 given for an autocorrelation')
    n1, n2 = len(X1), (0 if X2 is None else len(X2))
    for name, w, n in (('weights1', W1, n1), ('weights2', W2, n2)):
        if w is not None and (len(w.shape) != 1 or w.shape[0] != n):
            raise ValueError(f'{name} has shape {tuple(w.shape)}, expected ({n},)')
    cols = [c for c in (X1, Y1, Z1, X2, Y2, Z2) if c is not None]
    tail = (C.c_float(boxsize), ptr(bins), int(nb), C.c_float(pimax), int(npibins), C.c_float(mu_max), int(nmubins), ptr(out),
            ptr(wsum), ptr(rsum))
    if any(isinstance(c, _lib.DeviceArray) for c in cols):
        if not all(isinstance(c, _lib.DeviceArray) and c.dtype == cols[0].dtype for c in cols):
            raise TypeError('device-resident coordinates: every column must be a DeviceArray of one dtype')
        dt = {np.dtype(np.float32): 0, np.dtype(np.float64): 1}[cols[0].dtype]
        dp = lambda c: None if c is None else c.ptr     # noqa: E731
        own = []

        def dev_w(w):
            if w is None:
                return None
            if isinstance(w, _lib.DeviceArray):
                if w.dtype != np.float32:
                    raise TypeError('device-resident weights must be float32')
                return w
            own.append(_lib.DeviceArray(_f4(w)))
            return own[-1]
        try:
            d1, d2 = dev_w(W1), dev_w(W2)
            check(_lib.lib().abacus_paircount_weighted_dev(
                int(mode), dp(X1), dp(Y1), dp(Z1), dp(d1), C.c_int64(n1), dp(X2), dp(Y2), dp(Z2), dp(d2), C.c_int64(n2), dt,
                *tail))
        finally:
            for a in own:
                a.free()
        return out, wsum, rsum
    if isinstance(W1, _lib.DeviceArray) or isinstance(W2, _lib.DeviceArray):
        raise TypeError('device-resident weights need device-resident coordinates')
    X1, Y1, Z1, X2, Y2, Z2, W1, W2 = map(_f4, (X1, Y1, Z1, X2, Y2, Z2, W1, W2))
    check(_lib.lib().abacus_paircount_weighted(
        int(mode), ptr(X1), ptr(Y1), ptr(Z1), ptr(W1), C.c_int64(n1), ptr(X2), ptr(Y2), ptr(Z2), ptr(W2), C.c_int64(n2),
        *tail))
    return out, wsum, rsum


def _result(npairs, bins, nsub, extra, sums=None, avg_name=None):
    """structured array like Corrfunc's results: one row per (r-bin, sub-bin).  `sums` = (wsum, rsum) of a weighted call adds
    Corrfunc's `weightavg` and `avg_name` (averages over the bin's pairs, 0 for an empty bin) and `weightsum`"""
    nb = len(bins) - 1
    dt = [('rmin', 'f8'), ('rmax', 'f8'), ('npairs', 'u8')] + [(k, 'f8') for k in extra]
    if sums is not None:
        dt += [(avg_name, 'f8'), ('weightavg', 'f8'), ('weightsum', 'f8')]
    res = np.zeros(nb * nsub, dtype=dt)
    res['rmin'] = np.repeat(bins[:-1], nsub)
    res['rmax'] = np.repeat(bins[1:], nsub)
    res['npairs'] = npairs
    for k, v in extra.items():
        res[k] = np.tile(v, nb)
    if sums is not None:
        some = npairs > 0
        res['weightsum'] = sums[0]
        res['weightavg'][some] = sums[0][some] / npairs[some]
        if sums[1] is not None:
            res[avg_name][some] = sums[1][some] / npairs[some]
    return res


def _weight_kw(kw, avg_kw, autocorr):
    """the weight keywords of a Corrfunc call: None when neither weights nor the average separation are asked for (today's
    unweighted call), else (weights1, weights2, want the average)"""
    w1, w2 = kw.get('weights1'), kw.get('weights2')
    want_avg = bool(kw.get(avg_kw, False))
    if autocorr:
        w2 = None                      # Corrfunc ignores the second set of an autocorrelation
    wt = kw.get('weight_type')
    if wt is not None and wt != 'pair_product':
        raise NotImplementedError(f"weight_type={wt!r}: only 'pair_product' is implemented")
    if (w1 is not None or w2 is not None) and wt is None:
        raise ValueError("weights1 / weights2 given without weight_type='pair_product' (Corrfunc would ignore them silently)")
    if w1 is None and w2 is None and not want_avg:
        return None
    return w1, w2, want_avg


def _count(mode, autocorr, bins, nsub, extra, X1, Y1, Z1, X2, Y2, Z2, kw, avg_kw, **geom):
    """the body shared by DD / DDrppi / DDsmu"""
    second = (None, None, None) if autocorr else (X2, Y2, Z2)
    wk = _weight_kw(kw, avg_kw, autocorr)
    if wk is None:
        return _result(_paircount(mode, X1, Y1, Z1, geom.pop('boxsize'), bins, *second, **geom), bins, nsub, extra)
    n, ws, rs = _paircount_weighted(mode, X1, Y1, Z1, geom.pop('boxsize'), bins, *second, W1=_w_arr(wk[0]), W2=_w_arr(wk[1]),
                                    want_rsum=wk[2], **geom)
    return _result(n, bins, nsub, extra, sums=(ws, rs), avg_name=avg_kw[len('output_'):])


def _w_arr(w):
    return w if w is None or isinstance(w, _lib.DeviceArray) else np.asarray(w)


def DD(autocorr, nthreads, binfile, X1, Y1, Z1, X2=None, Y2=None, Z2=None, periodic=True, boxsize=None, **kw):
    """3-D pair counts in r bins (Corrfunc.theory.DD as called at scripts/emulator/generate_cfs/generate_cf.py:65-74)"""
    if not periodic or boxsize is None:
        raise NotImplementedError('only periodic boxes with an explicit boxsize are supported')
    bins = np.asarray(binfile, dtype=np.float64)
    return _count(0, autocorr, bins, 1, {}, X1, Y1, Z1, X2, Y2, Z2, kw, 'output_ravg', boxsize=float(boxsize))


def DDrppi(autocorr, nthreads, binfile=None, pimax=None, X1=None, Y1=None, Z1=None, X2=None, Y2=None, Z2=None,
           periodic=True, boxsize=None, max_cells_per_dim=None, verbose=False, **kw):
    """pair counts in (rp, pi) with 1-unit pi bins up to pimax (Corrfunc.theory.DDrppi, tpcf_corrfunc.py:144-156)"""
    if not periodic or boxsize is None:
        raise NotImplementedError('only periodic boxes with an explicit boxsize are supported')
    bins = np.asarray(binfile, dtype=np.float64)
    npi = int(pimax)
    return _count(1, autocorr, bins, npi, {'pimax': np.arange(1, npi + 1, dtype='f8')}, X1, Y1, Z1, X2, Y2, Z2, kw,
                  'output_rpavg', boxsize=float(boxsize), pimax=float(pimax), npibins=npi)


def DDsmu(autocorr, nthreads, binfile, mu_max, nmu_bins, X1, Y1, Z1, X2=None, Y2=None, Z2=None, periodic=True,
          boxsize=None, max_cells_per_dim=None, verbose=False, **kw):
    """pair counts in (s, mu) (Corrfunc.theory.DDsmu, tpcf_corrfunc.py:240-252)"""
    if not periodic or boxsize is None:
        raise NotImplementedError('only periodic boxes with an explicit boxsize are supported')
    bins = np.asarray(binfile, dtype=np.float64)
    return _count(2, autocorr, bins, int(nmu_bins), {'mumax': (np.arange(1, nmu_bins + 1) * mu_max / nmu_bins)}, X1, Y1, Z1,
                  X2, Y2, Z2, kw, 'output_savg', boxsize=float(boxsize), mu_max=float(mu_max), nmubins=int(nmu_bins))


def _check_int(name, v):
    if not isinstance(v, int):
        raise ValueError(f'{name} needs to be an integer')


def _natural_estimator(counter, sample1, sample2, edges, lbox, shell_measure, nsub, w1=None, w2=None, **counter_kw):
    """xi = DD / RR - 1 on a periodic box, shape (len(edges) - 1, nsub).

    counter         DDrppi | DDsmu (Corrfunc calling convention), called on float32 copies of the coordinates
    sample2         None for an autocorrelation (Corrfunc then returns ordered pairs, hence the factor 2 in RR,
                    which the reference also keeps for cross counts: tpcf_corrfunc.py:190-198,284-292,363-370)
    shell_measure   volume of a bin per unit (box volume)^-1 before the N1 N2 / L^3 normalisation, already shaped
                    (nbins, 1) or (nbins, nsub); RR is formed as measure / L^3 * N1 * N2 * 2 in that order and in the
                    dtype NumPy gives the reference's expression (float32 bins and box -> float32 RR)
    w1, w2          per-point weights (None: unit weights; both None: the unweighted estimator above, untouched).  DD is
                    then the counter's `weightsum` (sum of w_i w_j) and RR = measure / L^3 * W1 * W2 * 2 with W = the
                    float64 sum of a sample's weights (its size for unit weights; W2 = W1 for an autocorrelation)
    """
    # device-resident columns (the HOD catalogue in HBM) are cast to float32 on the device by abacus_paircount_dev
    cast = lambda cols: [c if isinstance(c, _lib.DeviceArray) else np.asarray(c).astype(np.float32) for c in cols]  # noqa: E731
    first = cast(sample1)
    n1 = float(len(first[0]))
    if sample2 is None or sample2[0] is None:
        second, n2, auto = {}, n1, 1
    else:
        second = dict(zip(('X2', 'Y2', 'Z2'), cast(sample2)))
        n2, auto = len(second['X2']), 0
    if w1 is not None or w2 is not None:
        total = lambda w, n: float(n) if w is None else float(np.sum(_host(w), dtype=np.float64))   # noqa: E731
        big1 = total(w1, n1)
        big2 = big1 if auto else total(w2, n2)
        res = counter(auto, counter_kw.pop('nthreads'), X1=first[0], Y1=first[1], Z1=first[2], boxsize=lbox, periodic=True,
                      weights1=w1, weights2=None if auto else w2, weight_type='pair_product', **second, **counter_kw)
        dd = res['weightsum'].reshape(len(edges) - 1, nsub)
        rr = shell_measure / lbox**3 * big1 * big2 * 2
        return dd, rr
    res = counter(auto, counter_kw.pop('nthreads'), X1=first[0], Y1=first[1], Z1=first[2], boxsize=lbox, periodic=True,
                  **second, **counter_kw)
    dd = res['npairs'].reshape(len(edges) - 1, nsub)
    rr = shell_measure / lbox**3 * n1 * n2 * 2
    return dd, rr


def _host(w):
    """a weight column as the float32 values the counter sees"""
    return (w.get() if isinstance(w, _lib.DeviceArray) else np.asarray(w)).astype(np.float32)


def tpcf_multipole(s_mu_tcpf_result, mu_bins, order=0):
    """Legendre multipole of xi(s, mu) over mu in [0, 1] bins, doubled to cover [-1, 1] (tpcf_corrfunc.py:17-94):
    (2l + 1)/2 * sum_mu xi * dmu * (L_l(mu) + L_l(-mu))."""
    from scipy.special import legendre
    xi = np.atleast_1d(s_mu_tcpf_result)
    edges = np.atleast_1d(mu_bins)
    ell = int(order)
    mid = (edges[:-1] + edges[1:]) / 2.0
    poly = legendre(ell)          # poly1d, evaluated like the reference does (same rounding)
    both_signs = poly(mid) + poly(-1.0 * mid)
    return (2.0 * ell + 1.0) / 2.0 * np.sum(xi * np.diff(edges) * both_signs, axis=1)


def calc_xirppi_fast(x1, y1, z1, rpbins, pimax, pi_bin_size, lbox, Nthread, num_cells=20, x2=None, y2=None, z2=None,
                     w1=None, w2=None):
    """xi(rp, pi) in pi bins of `pi_bin_size` built from unit pi bins (tpcf_corrfunc.py:97-203); w1 / w2: per-point weights
    (an extension: `_natural_estimator`)"""
    _check_int('pimax', pimax)
    _check_int('pi_bin_size', pi_bin_size)
    if pimax % pi_bin_size:
        raise ValueError('pi_bin_size needs to be an integer divisor of pimax, current values are ', pi_bin_size, pimax)
    edges = rpbins.astype(np.float32)
    lbox = np.float32(lbox)
    annulus = np.pi * (edges[1:] ** 2 - edges[:-1] ** 2) * pi_bin_size
    dd, rr = _natural_estimator(DDrppi, (x1, y1, z1), (x2, y2, z2), edges, lbox, annulus, pimax, nthreads=Nthread,
                                binfile=edges, pimax=np.float32(pimax), max_cells_per_dim=num_cells, verbose=False, w1=w1, w2=w2)
    grouped = dd.reshape(len(edges) - 1, pimax // pi_bin_size, pi_bin_size).sum(axis=2)
    return grouped / rr[:, None] - 1


def calc_multipole_fast(x1, y1, z1, sbins, lbox, Nthread, nbins_mu=50, num_cells=20, x2=None, y2=None, z2=None,
                        orders=[0, 2], w1=None, w2=None):
    """xi_l(s), the requested orders concatenated, from DD(s, mu) (tpcf_corrfunc.py:206-298); w1 / w2: per-point weights"""
    edges = sbins.astype(np.float32)
    lbox = np.float32(lbox)
    mu_edges = np.linspace(0, 1, nbins_mu + 1)
    wedge = 2 * np.pi / 3 * (edges[1:, None] ** 3 - edges[:-1, None] ** 3) * (mu_edges[None, 1:] - mu_edges[None, :-1])
    dd, rr = _natural_estimator(DDsmu, (x1, y1, z1), (x2, y2, z2), edges, lbox, wedge, nbins_mu, nthreads=Nthread,
                                binfile=edges, mu_max=1, nmu_bins=nbins_mu, max_cells_per_dim=num_cells, w1=w1, w2=w2)
    xi = dd / rr - 1
    return np.concatenate([tpcf_multipole(xi, mu_edges, order=ell) for ell in orders])


def calc_wp_fast(x1, y1, z1, rpbins, pimax, lbox, Nthread, num_cells=30, x2=None, y2=None, z2=None, w1=None, w2=None):
    """wp(rp) = 2 * sum over unit pi bins of xi(rp, pi) (tpcf_corrfunc.py:301-372); w1 / w2: per-point weights"""
    _check_int('pimax', pimax)
    edges = rpbins.astype(np.float32)
    lbox = np.float32(lbox)
    annulus = np.pi * (edges[1:] ** 2 - edges[:-1] ** 2)
    dd, rr = _natural_estimator(DDrppi, (x1, y1, z1), (x2, y2, z2), edges, lbox, annulus, pimax, nthreads=Nthread,
                                binfile=edges, pimax=np.float32(pimax), max_cells_per_dim=num_cells, w1=w1, w2=w2)
    return 2 * np.sum(dd / rr[:, None] - 1, axis=1)
