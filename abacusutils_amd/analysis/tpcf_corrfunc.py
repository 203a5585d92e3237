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


def _i4(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32)


def _set_sizes(cols, weights):
    """(n1, n2) of `cols` = (X1, Y1, Z1, X2, Y2, Z2), after the checks of `weights` = (W1, W2) against them"""
    X1, X2 = cols[0], cols[3]
    if X2 is None and weights[1] is not None:
        raise ValueError('weights2 given for an autocorrelation')
    n1, n2 = len(X1), (0 if X2 is None else len(X2))
    for name, w, n in (('weights1', weights[0], n1), ('weights2', weights[1], n2)):
        if w is not None and (len(w.shape) != 1 or w.shape[0] != n):
            raise ValueError(f'{name} has shape {tuple(w.shape)}, expected ({n},)')
    return n1, n2


def _call_on_columns(entry, cols, weights, labels, geom, call, host_prep=None, calls=None):
    """The column rules of every pair counter, plain (`_counter`) and jackknife (`jackknife._jk_counter`).  Columns are host
    arrays (cast to float32) or - all of them - DeviceArray columns of one dtype.  `weights` = (W1, W2) (float32) and `labels` =
    (L1, L2) (int32) ride along: a host array next to resident coordinates is uploaded and freed after the call, a resident one
    next to host coordinates is not accepted.  `host_prep(cols, geom)` -> (cols, geom), if given, has the last word on host
    columns, after every check.  Returns call(fn, p, cols, weights, labels, geom, *dt): fn is `abacus_<entry>` (host columns)
    or `abacus_<entry>_dev` (resident ones, dt = (pos_dtype,)), p turns an array into its pointer.  `calls`: a dict that counts
    the calls by where the columns were."""
    given = [c for c in cols if c is not None]
    if any(isinstance(c, _lib.DeviceArray) for c in given):
        if not all(isinstance(c, _lib.DeviceArray) and c.dtype == given[0].dtype for c in given):
            raise TypeError('device-resident coordinates: every column must be a DeviceArray of one dtype')
        dt = {np.dtype(np.float32): 0, np.dtype(np.float64): 1}[given[0].dtype]
        own = []

        def dev(a, cast, what):
            if a is None:
                return None
            if isinstance(a, _lib.DeviceArray):
                if a.dtype != what:
                    raise TypeError(f'device-resident weights must be float32, labels int32 (got {a.dtype})')
                return a
            own.append(_lib.DeviceArray(cast(a)))
            return own[-1]
        try:
            if calls is not None:
                calls['dev'] += 1
            return call(getattr(_lib.lib(), f'abacus_{entry}_dev'), lambda c: None if c is None else c.ptr, cols,
                        [dev(w, _f4, np.float32) for w in weights], [dev(lab, _i4, np.int32) for lab in labels], geom, dt)
        finally:
            for a in own:
                a.free()
    if any(isinstance(a, _lib.DeviceArray) for a in (*weights, *labels)):
        raise TypeError('device-resident weights or labels need device-resident coordinates')
    if host_prep is not None:
        cols, geom = host_prep(cols, geom)
    if calls is not None:
        calls['host'] += 1
    return call(getattr(_lib.lib(), f'abacus_{entry}'), ptr, [_f4(c) for c in cols], [_f4(w) for w in weights],
                [_i4(lab) for lab in labels], geom)


def _counter(entry, mode, bins, cols, weights, geom, pimax, npibins, mu_max, nmubins, want_sums=True, want_rsum=True,
             host_prep=None):
    """What the three counters below share.  `entry`: the C function `abacus_<entry>[_dev]`; `bins`: float32 edges; `cols` =
    (X1, Y1, Z1, X2, Y2, Z2); `weights` = (W1, W2), or None for an entry without weight and sum arguments; `geom`: the ctypes
    arguments between the columns and the bins (box size | origin).  Columns, weights and `host_prep` as `_call_on_columns`
    takes them.  Returns (npairs, wsum, rsum); the sums are None when not asked for."""
    nb = len(bins) - 1
    nsub = 1 if mode == 0 else (npibins if mode == 1 else nmubins)
    out = np.zeros(nb * nsub, dtype=np.uint64)
    wsum = np.zeros(nb * nsub, dtype=np.float64) if want_sums else None
    rsum = np.zeros(nb * nsub, dtype=np.float64) if want_sums and want_rsum else None
    n1, n2 = _set_sizes(cols, weights or (None, None))
    tail = (ptr(bins), int(nb), C.c_float(pimax), int(npibins), C.c_float(mu_max), int(nmubins), ptr(out))
    if weights is not None:
        tail += (ptr(wsum), ptr(rsum))

    def call(fn, p, cols, w, lab, geom, *dt):
        ws = ((p(w[0]),), (p(w[1]),)) if weights is not None else ((), ())
        check(fn(int(mode), *map(p, cols[:3]), *ws[0], C.c_int64(n1), *map(p, cols[3:]), *ws[1], C.c_int64(n2), *dt, *geom, *tail))
        return out, wsum, rsum
    return _call_on_columns(entry, cols, weights or (None, None), (), geom, call, host_prep)


def _paircount(mode, X1, Y1, Z1, boxsize, bins, X2=None, Y2=None, Z2=None, pimax=0.0, npibins=0, mu_max=1.0,
               nmubins=0):
    """host arrays (cast to float32 like the reference, tpcf_corrfunc.py:134-139) or - all of them - `_lib.DeviceArray`
    columns of float32 / float64 already in HBM (the HOD catalogue: `abacus_paircount_dev`, no PCIe round trip)"""
    return _counter('paircount', mode, _f4(bins), (X1, Y1, Z1, X2, Y2, Z2), None, (C.c_float(boxsize),), pimax, npibins, mu_max,
                    nmubins, want_sums=False)[0]


def _paircount_weighted(mode, X1, Y1, Z1, boxsize, bins, X2=None, Y2=None, Z2=None, W1=None, W2=None, pimax=0.0,
                        npibins=0, mu_max=1.0, nmubins=0, want_rsum=True):
    """`_paircount` with per-point float32 weights (None: unit weights): (npairs, wsum, rsum) per (bin, sub-bin) with
    wsum = sum of w_i * w_j and rsum = sum of the pair separation (r | rp | s), both accumulated in float64 on the device
    (`abacus_paircount_weighted[_dev]`); rsum is None when `want_rsum` is false."""
    return _counter('paircount_weighted', mode, _f4(bins), (X1, Y1, Z1, X2, Y2, Z2), (W1, W2), (C.c_float(boxsize),), pimax,
                    npibins, mu_max, nmubins, want_rsum=want_rsum)


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


def _count(los, mode, autocorr, bins, nsub, extra, X1, Y1, Z1, X2, Y2, Z2, kw, avg_kw, **geom):
    """the body shared by DD / DDrppi / DDsmu (`los` false: `geom` holds the box size) and their `_los` forms (`los` true:
    `geom` holds the origin).  `count(**weights)` below is the one place where the two families differ."""
    second = (None, None, None) if autocorr else (X2, Y2, Z2)
    if los:
        if not autocorr and any(c is None for c in second):
            raise ValueError('a cross count needs X2, Y2 and Z2')
        count = lambda **w: _paircount_los(mode, X1, Y1, Z1, bins, *second, want_sums=bool(w), **w, **geom)     # noqa: E731
    else:
        box = geom.pop('boxsize')
        count = lambda **w: (_paircount_weighted(mode, X1, Y1, Z1, box, bins, *second, **w, **geom) if w else       # noqa: E731
                             (_paircount(mode, X1, Y1, Z1, box, bins, *second, **geom), None, None))
    wk = _weight_kw(kw, avg_kw, autocorr)
    if wk is None:
        return _result(count()[0], bins, nsub, extra)
    n, ws, rs = count(W1=_w_arr(wk[0]), W2=_w_arr(wk[1]), want_rsum=wk[2])
    return _result(n, bins, nsub, extra, sums=(ws, rs), avg_name=avg_kw[len('output_'):])


def _w_arr(w):
    return w if w is None or isinstance(w, _lib.DeviceArray) else np.asarray(w)


def DD(autocorr, nthreads, binfile, X1, Y1, Z1, X2=None, Y2=None, Z2=None, periodic=True, boxsize=None, **kw):
    """3-D pair counts in r bins (Corrfunc.theory.DD as called at scripts/emulator/generate_cfs/generate_cf.py:65-74)"""
    if not periodic or boxsize is None:
        raise NotImplementedError('only periodic boxes with an explicit boxsize are supported')
    bins = np.asarray(binfile, dtype=np.float64)
    return _count(False, 0, autocorr, bins, 1, {}, X1, Y1, Z1, X2, Y2, Z2, kw, 'output_ravg', boxsize=float(boxsize))


def DDrppi(autocorr, nthreads, binfile=None, pimax=None, X1=None, Y1=None, Z1=None, X2=None, Y2=None, Z2=None,
           periodic=True, boxsize=None, max_cells_per_dim=None, verbose=False, **kw):
    """pair counts in (rp, pi) with 1-unit pi bins up to pimax (Corrfunc.theory.DDrppi, tpcf_corrfunc.py:144-156)"""
    if not periodic or boxsize is None:
        raise NotImplementedError('only periodic boxes with an explicit boxsize are supported')
    bins = np.asarray(binfile, dtype=np.float64)
    npi = int(pimax)
    return _count(False, 1, autocorr, bins, npi, {'pimax': np.arange(1, npi + 1, dtype='f8')}, X1, Y1, Z1, X2, Y2, Z2, kw,
                  'output_rpavg', boxsize=float(boxsize), pimax=float(pimax), npibins=npi)


def DDsmu(autocorr, nthreads, binfile, mu_max, nmu_bins, X1, Y1, Z1, X2=None, Y2=None, Z2=None, periodic=True,
          boxsize=None, max_cells_per_dim=None, verbose=False, **kw):
    """pair counts in (s, mu) (Corrfunc.theory.DDsmu, tpcf_corrfunc.py:240-252)"""
    if not periodic or boxsize is None:
        raise NotImplementedError('only periodic boxes with an explicit boxsize are supported')
    bins = np.asarray(binfile, dtype=np.float64)
    return _count(False, 2, autocorr, bins, int(nmu_bins), {'mumax': (np.arange(1, nmu_bins + 1) * mu_max / nmu_bins)}, X1, Y1, Z1,
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


# ---------------------------------------------------------------------------------------------------------------------
# Light cones: pair counts with a pairwise line of sight on an open grid (csrc/pairs.hip: pair_count_los, C ABI
# abacus_paircount_los[_dev]) and the Landy-Szalay estimators on top.  The reference leaves this to Corrfunc.mocks; no
# Corrfunc run stands behind the code here - the conventions are those of include/abacus_hip.h, pinned against the NumPy
# statement tests/pairs_los_statement.py only.

def _paircount_los(mode, X1, Y1, Z1, bins, X2=None, Y2=None, Z2=None, W1=None, W2=None, origin=(0.0, 0.0, 0.0), pimax=0.0,
                   npibins=0, mu_max=1.0, nmubins=0, want_sums=True, want_rsum=True):
    """(npairs, wsum, rsum) per (bin, sub-bin) of the light-cone counter; wsum and rsum are None when `want_sums` is false
    (integer counts only), rsum when `want_rsum` is false.  Columns: host arrays (float64 columns are centred on `origin` in
    float64 here, float32 ones on the device in float32) or - all of them - DeviceArray columns of one dtype; weights as in
    `_paircount_weighted`"""
    bins = _f4(bins)
    nb = len(bins) - 1
    nsub = 1 if mode == 0 else (npibins if mode == 1 else nmubins)
    if nb < 1 or nsub < 1:
        raise ValueError('need at least one separation bin and one pi / mu bin')
    origin, centre = _los_origin(origin)
    return _counter('paircount_los', mode, bins, (X1, Y1, Z1, X2, Y2, Z2), (W1, W2), (ptr(origin),), pimax, npibins, mu_max,
                    nmubins, want_sums=want_sums, want_rsum=want_rsum, host_prep=centre)


def _los_origin(origin):
    """the origin of a light-cone call as the C ABI takes it, and the `host_prep` of its counter (`_paircount_los`,
    `jackknife.paircount_los_jk`)"""
    origin = np.ascontiguousarray(origin, dtype=np.float64)
    if origin.shape != (3,):
        raise ValueError(f'origin has shape {origin.shape}, expected (3,)')
    zero = np.zeros(3)

    def centre(cols, geom):
        host = [None if c is None else np.asarray(c) for c in cols]
        if not any(c is not None and c.dtype == np.float64 for c in host):
            return cols, geom
        # float64 columns: the subtraction in float64, one rounding to float32 - on the host, the C ABI takes float32 arrays
        return [None if c is None else (c - c.dtype.type(origin[i % 3])).astype(np.float32) if c.dtype == np.float64
                else _f4(c) - np.float32(origin[i % 3]) for i, c in enumerate(host)], (ptr(zero),)
    return origin, centre


def DD_los(autocorr, nthreads, binfile, X1, Y1, Z1, X2=None, Y2=None, Z2=None, origin=(0.0, 0.0, 0.0), **kw):
    """pair counts in s bins of a non-periodic catalogue in Cartesian columns seen from `origin` (no box, no wrapping);
    weights1 / weights2 / weight_type / output_ravg as `DD`"""
    bins = np.asarray(binfile, dtype=np.float64)
    return _count(True, 0, autocorr, bins, 1, {}, X1, Y1, Z1, X2, Y2, Z2, kw, 'output_ravg', origin=origin)


def DDrppi_los(autocorr, nthreads, binfile, pimax, X1, Y1, Z1, X2=None, Y2=None, Z2=None, origin=(0.0, 0.0, 0.0), **kw):
    """pair counts in (rp, pi) with the line of sight of each PAIR, l = p_i + p_j seen from `origin`: pi = |d.l| / |l|,
    rp^2 = s^2 - pi^2, unit pi bins up to pimax; weight keywords as `DDrppi`"""
    if not pimax > 0:
        raise ValueError('pimax must be positive')
    bins = np.asarray(binfile, dtype=np.float64)
    npi = int(pimax)
    if npi < 1:
        raise ValueError('pimax must be at least 1 (unit pi bins)')
    return _count(True, 1, autocorr, bins, npi, {'pimax': np.arange(1, npi + 1, dtype='f8')}, X1, Y1, Z1, X2, Y2, Z2, kw,
                  'output_rpavg', origin=origin, pimax=float(pimax), npibins=npi)


def DDsmu_los(autocorr, nthreads, binfile, mu_max, nmu_bins, X1, Y1, Z1, X2=None, Y2=None, Z2=None, origin=(0.0, 0.0, 0.0),
              **kw):
    """pair counts in (s, mu), mu = pi / s with the pairwise line of sight of `DDrppi_los`; weight keywords as `DDsmu`"""
    if not mu_max > 0 or int(nmu_bins) < 1:
        raise ValueError('mu_max must be positive, with at least one mu bin')
    bins = np.asarray(binfile, dtype=np.float64)
    return _count(True, 2, autocorr, bins, int(nmu_bins), {'mumax': (np.arange(1, nmu_bins + 1) * mu_max / nmu_bins)}, X1, Y1, Z1,
                  X2, Y2, Z2, kw, 'output_savg', origin=origin, mu_max=float(mu_max), nmubins=int(nmu_bins))


def radec_to_xyz(ra_deg, dec_deg, dist):
    """float64 Cartesian columns of (right ascension, declination) in degrees and a comoving distance:
    x = d cos(dec) cos(ra), y = d cos(dec) sin(ra), z = d sin(dec)"""
    ra, dec = np.radians(np.asarray(ra_deg, dtype=np.float64)), np.radians(np.asarray(dec_deg, dtype=np.float64))
    d = np.asarray(dist, dtype=np.float64)
    return d * np.cos(dec) * np.cos(ra), d * np.cos(dec) * np.sin(ra), d * np.sin(dec)


def _mocks_columns(is_comoving_dist, RA1, DEC1, CZ1, RA2, DEC2, CZ2, autocorr):
    if not is_comoving_dist:
        raise NotImplementedError('is_comoving_dist=False needs a cosmology to turn cz into distances; none is carried here: '
                                  'pass comoving distances and is_comoving_dist=True')
    first = radec_to_xyz(RA1, DEC1, CZ1)
    if autocorr:
        return first, (None, None, None)
    if RA2 is None or DEC2 is None or CZ2 is None:
        raise ValueError('a cross count needs RA2, DEC2 and CZ2')
    return first, radec_to_xyz(RA2, DEC2, CZ2)


def DDrppi_mocks(autocorr, cosmology, nthreads, pimax, binfile, RA1, DEC1, CZ1, weights1=None, RA2=None, DEC2=None, CZ2=None,
                 weights2=None, is_comoving_dist=False, **kw):
    """Corrfunc.mocks.DDrppi_mocks over `DDrppi_los`.  The argument order is Corrfunc's published one as far as it can be
    recalled without the package at hand - check it against your Corrfunc before relying on positional calls.  `cosmology`
    is accepted and ignored; the CZ columns must be comoving distances (is_comoving_dist=True), else NotImplementedError."""
    first, second = _mocks_columns(is_comoving_dist, RA1, DEC1, CZ1, RA2, DEC2, CZ2, autocorr)
    return DDrppi_los(autocorr, nthreads, binfile, pimax, *first, *second, weights1=weights1, weights2=weights2, **kw)


def DDsmu_mocks(autocorr, cosmology, nthreads, mu_max, nmu_bins, binfile, RA1, DEC1, CZ1, weights1=None, RA2=None, DEC2=None,
                CZ2=None, weights2=None, is_comoving_dist=False, **kw):
    """Corrfunc.mocks.DDsmu_mocks over `DDsmu_los`; the remarks of `DDrppi_mocks` on argument order, `cosmology` and
    `is_comoving_dist` apply"""
    first, second = _mocks_columns(is_comoving_dist, RA1, DEC1, CZ1, RA2, DEC2, CZ2, autocorr)
    return DDsmu_los(autocorr, nthreads, binfile, mu_max, nmu_bins, *first, *second, weights1=weights1, weights2=weights2, **kw)


class _LCSample:
    """a point set of the Landy-Szalay estimators: observer-centred float32 columns in HBM (centred ONCE, then counted against
    several other sets with origin 0), float32 weights in HBM or None, W = sum w and sum w^2 in float64"""

    def __init__(self, x, y, z, w=None, origin=(0.0, 0.0, 0.0)):
        origin = np.asarray(origin, dtype=np.float64)
        cols = (x, y, z)
        self.n = len(x)
        if all(isinstance(c, _lib.DeviceArray) for c in cols):
            if cols[0].dtype == np.float32 and not origin.any():
                self.cols = list(cols)
            else:
                dt = {np.dtype(np.float32): 0, np.dtype(np.float64): 1}[cols[0].dtype]
                self.cols = [_lib.DeviceArray(nbytes=4 * self.n, dtype=np.float32, shape=(self.n,)) for _ in cols]
                for c, o, dst in zip(cols, origin, self.cols):
                    check(_lib.lib().abacus_paircount_los_centre(c.ptr, dt, C.c_int64(self.n), C.c_double(o), dst.ptr))
        elif any(isinstance(c, _lib.DeviceArray) for c in cols):
            raise TypeError('device-resident coordinates: every column must be a DeviceArray')
        else:
            host = [np.asarray(c) for c in cols]
            host = [c if c.dtype == np.float64 else c.astype(np.float32) for c in host]
            self.cols = [_lib.DeviceArray((c - c.dtype.type(o)).astype(np.float32)) for c, o in zip(host, origin)]
        if w is None:
            self.w, self.W, self.W2 = None, float(self.n), float(self.n)
        else:
            hw = _host(w).astype(np.float64)
            if hw.shape != (self.n,):
                raise ValueError(f'weights have shape {hw.shape}, expected ({self.n},)')
            self.w = w if isinstance(w, _lib.DeviceArray) else _lib.DeviceArray(hw.astype(np.float32))
            self.W, self.W2 = float(hw.sum()), float((hw * hw).sum())

    @property
    def auto_norm(self):
        """normalisation of the ordered autocorrelation: W^2 - sum w^2 (N (N - 1) for unit weights)"""
        return self.W * self.W - self.W2


def _ls_weightsum(mode, a, b, bins, geom):
    """sum of w_i w_j per (bin, sub-bin) of sample `a` with itself (b None, ordered pairs) or with sample `b`"""
    second = (None, None, None) if b is None else b.cols
    _, ws, _ = _paircount_los(mode, *a.cols, bins, *second, W1=a.w, W2=None if b is None else b.w, want_rsum=False, **geom)
    return ws


class LCRandoms(_LCSample):
    """The randoms of a light-cone catalogue for `calc_xirppi_lc` / `calc_wp_lc` / `calc_multipole_lc`: uploaded once,
    and RR - the most expensive term - counted once per (mode, bins, pi / mu binning) and kept.  For `analysis.lc_power` (`fkp_field`,
    `calc_power_lc`) the same object keeps the randoms' mesh, deposited once per (nmesh, box, cloud), and takes `nbar`: the number
    density of the random catalogue at each random (a host array or a `DeviceArray`, e.g. from `lc_power.radial_nbar`), which
    normalises the power spectrum."""

    def __init__(self, x, y, z, w=None, origin=(0.0, 0.0, 0.0), nbar=None):
        super().__init__(x, y, z, w, origin)
        self._rr = {}
        self.rr_counted = 0      # RR runs so far (a cache hit does not count)
        if nbar is not None and tuple(nbar.shape if isinstance(nbar, _lib.DeviceArray) else np.shape(nbar)) != (self.n,):
            raise ValueError(f'nbar must have shape ({self.n},)')
        self.nbar = nbar
        self._mesh = {}          # lc_power: (nmesh, box side, corner, cloud) -> the randoms' padded mesh in HBM
        self.mesh_built = 0      # deposits of the randoms so far (a cache hit does not count)
        self._w2n = None         # lc_power: sum w^2 nbar in float64

    def rr(self, mode, bins, geom):
        key = (int(mode), _f4(bins).tobytes(), tuple(sorted(geom.items())))
        if key not in self._rr:
            self._rr[key] = _ls_weightsum(mode, self, None, bins, geom)
            self.rr_counted += 1
        return self._rr[key]


def landy_szalay(d1d2, d1r, d2r, rr, n12, n1r, n2r, nrr):
    """xi = (D1D2 / N12 - D1R / N1r - D2R / N2r + RR / Nrr) / (RR / Nrr), every term a weight sum, float64; a bin without RR
    pairs comes out as nan or inf"""
    d1d2, d1r, d2r, rr = (np.asarray(a, dtype=np.float64) for a in (d1d2, d1r, d2r, rr))
    with np.errstate(divide='ignore', invalid='ignore'):
        return (d1d2 / n12 - d1r / n1r - d2r / n2r + rr / nrr) / (rr / nrr)


def _ls_terms(mode, s1, s2, randoms, bins, geom):
    """the four weight sums and their normalisations.  Cross normalisations are Wa Wb, those of the ordered autocorrelations
    W^2 - sum w^2; an autocorrelation counts DR once: D2R = D1R"""
    if not isinstance(randoms, LCRandoms):
        raise TypeError('randoms must be an LCRandoms')
    rr = randoms.rr(mode, bins, geom)
    d1r = _ls_weightsum(mode, s1, randoms, bins, geom)
    if s2 is None:
        dd, n12 = _ls_weightsum(mode, s1, None, bins, geom), s1.auto_norm
        d2r, n2r = d1r, s1.W * randoms.W
    else:
        dd, n12 = _ls_weightsum(mode, s1, s2, bins, geom), s1.W * s2.W
        d2r, n2r = _ls_weightsum(mode, s2, randoms, bins, geom), s2.W * randoms.W
    return (dd, d1r, d2r, rr), (n12, s1.W * randoms.W, n2r, randoms.auto_norm)


def _ls_samples(x1, y1, z1, x2, y2, z2, w1, w2, origin):
    s1 = _LCSample(x1, y1, z1, w1, origin)
    if x2 is None:
        if w2 is not None:
            raise ValueError('w2 given for an autocorrelation')
        return s1, None
    return s1, _LCSample(x2, y2, z2, w2, origin)


def calc_xirppi_lc(x1, y1, z1, rpbins, pimax, pi_bin_size, randoms, Nthread=1, x2=None, y2=None, z2=None, w1=None, w2=None,
                   origin=(0.0, 0.0, 0.0)):
    """Landy-Szalay xi(rp, pi) of a light-cone catalogue seen from `origin`, in pi bins of `pi_bin_size` built from unit pi
    bins (every count is grouped before the estimator is formed): the shape of `calc_xirppi_fast`.  randoms: an LCRandoms"""
    _check_int('pimax', pimax)
    _check_int('pi_bin_size', pi_bin_size)
    if pimax % pi_bin_size:
        raise ValueError('pi_bin_size needs to be an integer divisor of pimax, current values are ', pi_bin_size, pimax)
    edges = np.asarray(rpbins).astype(np.float32)
    s1, s2 = _ls_samples(x1, y1, z1, x2, y2, z2, w1, w2, origin)
    terms, norms = _ls_terms(1, s1, s2, randoms, edges, dict(pimax=float(pimax), npibins=int(pimax)))
    group = lambda a: a.reshape(len(edges) - 1, pimax // pi_bin_size, pi_bin_size).sum(axis=2)   # noqa: E731
    return landy_szalay(*map(group, terms), *norms)


def calc_wp_lc(x1, y1, z1, rpbins, pimax, randoms, Nthread=1, x2=None, y2=None, z2=None, w1=None, w2=None,
               origin=(0.0, 0.0, 0.0)):
    """wp(rp) = 2 * sum over unit pi bins of the Landy-Szalay xi(rp, pi): the shape of `calc_wp_fast`"""
    _check_int('pimax', pimax)
    edges = np.asarray(rpbins).astype(np.float32)
    s1, s2 = _ls_samples(x1, y1, z1, x2, y2, z2, w1, w2, origin)
    terms, norms = _ls_terms(1, s1, s2, randoms, edges, dict(pimax=float(pimax), npibins=int(pimax)))
    shape = lambda a: a.reshape(len(edges) - 1, pimax)   # noqa: E731
    return 2 * np.sum(landy_szalay(*map(shape, terms), *norms), axis=1)


def calc_multipole_lc(x1, y1, z1, sbins, randoms, Nthread=1, nbins_mu=50, x2=None, y2=None, z2=None, orders=[0, 2], w1=None,
                      w2=None, origin=(0.0, 0.0, 0.0)):
    """xi_l(s), the requested orders concatenated, from the Landy-Szalay xi(s, mu) in `nbins_mu` bins of mu in [0, 1): the
    shape of `calc_multipole_fast`"""
    edges = np.asarray(sbins).astype(np.float32)
    mu_edges = np.linspace(0, 1, nbins_mu + 1)
    s1, s2 = _ls_samples(x1, y1, z1, x2, y2, z2, w1, w2, origin)
    terms, norms = _ls_terms(2, s1, s2, randoms, edges, dict(mu_max=1.0, nmubins=int(nbins_mu)))
    shape = lambda a: a.reshape(len(edges) - 1, nbins_mu)   # noqa: E731
    xi = landy_szalay(*map(shape, terms), *norms)
    return np.concatenate([tpcf_multipole(xi, mu_edges, order=ell) for ell in orders])
