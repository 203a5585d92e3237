"""Jackknife errors of the pair-count statistics: per-region counts from ONE pair walk, delete-one samples, covariances.

Nothing in the reference does this (it leaves pair counting to Corrfunc, which has no jackknife either); the conventions are
those of include/abacus_hip.h (abacus_paircount_jk, abacus_paircount_los_jk), pinned against NumPy statements
(tests/pairs_jk_statement.py) only.

Counts.  Every point carries a label in [0, nreg).  Per (bin, sub-bin) q and region k, over the pairs (i, j) the parent
counter puts into q (`_paircount_weighted` on the box, `_paircount_los` on the light cone; ordered pairs without self pairs for
an autocorrelation):

    first[k, q]   label1(i) = k                       second[k, q]  label2(j) = k
    both[k, q]    label1(i) = k and label2(j) = k     total[q]      = sum_k first[k, q]: the parent's result

each as an integer count and as sum of w_i w_j.  The device returns first and both.  Membership of a pair is symmetric under
exchange of its points in every mode of both families (d -> -d; l, |dz| and t^2 do not change), so `second` of (1, 2) is
`first` of (2, 1): an autocorrelation has second = first, a cross count is counted again with the sets exchanged.

Delete-one.  With cross_weight alpha, D_-k = total - both_k - alpha (first_k + second_k - 2 both_k): alpha = 1 removes every
pair that touches region k - the counts of the catalogue without the region; alpha = 1/2 removes a pair with ONE point in k
by half: total - (first_k + second_k) / 2.  The same formula on the normalisations (`delete_one_norm`).

Estimators.  Periodic box (`calc_wp_jk`, `calc_xirppi_jk`, `calc_multipole_jk`): the natural estimator, alpha = 1/2 only,
xi_-k = D_-k / (RR (1 - W1_k / 2 W1 - W2_k / 2 W2)) - 1: with alpha = 1/2 the expected random count of the reduced sample
needs each region's share of the weight and nothing of its geometry, so any label map works (with alpha = 1 it would need
the volume of the bin's shell inside and outside region k).  Light cone (`calc_wp_lc_jk`, ...): Landy-Szalay of the
delete-one weight sums of DD, DR and RR and their delete-one normalisations; the randoms carry labels (`LCRandomsJK`),
alpha = 1 by default.  Covariance: (n - 1) / n sum_k (theta_k - mean)(theta_k - mean)^T.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from .. import _lib
from .._lib import check, ptr
from . import tpcf_corrfunc as tc
from .tpcf_corrfunc import _f4, _i4

MODES = {'r': 0, 'rppi': 1, 'smu': 2}
calls = {'dev': 0, 'host': 0}      # counter calls so far, by where the columns were (tests: the resident path was taken)


@dataclass
class JKTerm:
    """one of total / first / second / both: integer counts and sums of w_i w_j (None: not asked for)"""
    npairs: np.ndarray
    wsum: np.ndarray = None


@dataclass
class JKCounts:
    """per-region pair counts: `total` is shaped (nbins, nsub), the others (nreg, nbins, nsub)"""
    total: JKTerm
    first: JKTerm
    second: JKTerm
    both: JKTerm

    @property
    def nreg(self):
        return self.first.npairs.shape[0]


def _check_labels(name, lab, n):
    if lab is None:
        raise ValueError(f'{name} is needed')
    shape = tuple(lab.shape) if isinstance(lab, _lib.DeviceArray) else np.shape(lab)
    if shape != (n,):
        raise ValueError(f'{name} has shape {shape}, expected ({n},)')
    if isinstance(lab, _lib.DeviceArray):
        if lab.dtype != np.int32:
            raise TypeError(f'device-resident {name} must be int32')
    elif not np.issubdtype(np.asarray(lab).dtype, np.integer):
        raise TypeError(f'{name} must be integers')


def _jk_counter(entry, mode, bins, cols, weights, labels, nreg, geom, pimax, npibins, mu_max, nmubins, want_sums=True,
                host_prep=None):
    """one call of `abacus_<entry>[_dev]` under the column rules of `tpcf_corrfunc._call_on_columns`, which `_counter` follows
    too.  Returns (npairs_first, npairs_both, wsum_first, wsum_both), each (nreg, nbins * nsub)"""
    mode = MODES.get(mode, mode)
    nb = len(bins) - 1
    nsub = 1 if mode == 0 else (npibins if mode == 1 else nmubins)
    if nb < 1 or nsub < 1:
        raise ValueError('need at least one separation bin and one pi / mu bin')
    X2 = cols[3]
    L1, L2 = labels
    n1, n2 = tc._set_sizes(cols, weights)
    if X2 is None and L2 is not None:
        raise ValueError('labels2 given for an autocorrelation')
    _check_labels('labels1', L1, n1)
    if X2 is not None:
        _check_labels('labels2', L2, n2)
    cnt = max(int(nreg), 0) * nb * nsub
    if cnt > 1 << 24:           # the library refuses it too; do not allocate for it
        cnt = 0
    nf, nbo = np.zeros(cnt, dtype=np.uint64), np.zeros(cnt, dtype=np.uint64)
    wf = np.zeros(cnt, dtype=np.float64) if want_sums else None
    wb = np.zeros(cnt, dtype=np.float64) if want_sums else None
    tail = (ptr(bins), int(nb), C.c_float(pimax), int(npibins), C.c_float(mu_max), int(nmubins), ptr(nf), ptr(nbo), ptr(wf), ptr(wb))

    def call(fn, p, cols, w, lab, geom, *dt):
        check(fn(int(mode), *map(p, cols[:3]), p(w[0]), p(lab[0]), C.c_int64(n1), *map(p, cols[3:]), p(w[1]), p(lab[1]), C.c_int64(n2),
                 *dt, int(nreg), *geom, *tail))
        shape = (int(nreg), nb * nsub)
        return nf.reshape(shape), nbo.reshape(shape), None if wf is None else wf.reshape(shape), None if wb is None else wb.reshape(shape)
    return tc._call_on_columns(entry, cols, weights, labels, geom, call, host_prep, calls)


def _assemble(raw, exchanged, shape):
    """JKCounts of one call (autocorrelation: second = first) or of the call and its exchange (cross count)"""
    nf, nb, wf, wb = raw
    term = lambda n, w: JKTerm(n.reshape((-1,) + shape), None if w is None else w.reshape((-1,) + shape))   # noqa: E731
    first, both = term(nf, wf), term(nb, wb)
    if exchanged is None:
        second = first
    else:
        second = term(exchanged[0], exchanged[2])
        if not np.array_equal(exchanged[1], nb):
            raise _lib.AbacusHipError('jackknife pair counts: `both` of the exchanged call differs (membership must be symmetric)')
    total = JKTerm(first.npairs.sum(axis=0, dtype=np.uint64), None if wf is None else first.wsum.sum(axis=0))
    return JKCounts(total, first, second, both)


def _count_jk(entry, mode, bins, first, second, W, L, nreg, geom, kw, want_sums, host_prep=None):
    mode = MODES.get(mode, mode)
    bins = _f4(bins)
    nsub = 1 if mode == 0 else (kw['npibins'] if mode == 1 else kw['nmubins'])
    auto = second[0] is None
    raw = _jk_counter(entry, mode, bins, (*first, *second), W, L, nreg, geom, want_sums=want_sums, host_prep=host_prep, **kw)
    ex = None
    if not auto:
        ex = _jk_counter(entry, mode, bins, (*second, *first), W[::-1], L[::-1], nreg, geom, want_sums=want_sums, host_prep=host_prep,
                         **kw)
    return _assemble(raw, ex, (len(bins) - 1, nsub))


def paircount_jk(mode, X1, Y1, Z1, boxsize, bins, labels1, nreg, X2=None, Y2=None, Z2=None, labels2=None, W1=None, W2=None,
                 pimax=0.0, npibins=0, mu_max=1.0, nmubins=0):
    """per-region pair counts on the periodic box (`abacus_paircount_jk[_dev]`): a `JKCounts`; columns as `_paircount_weighted`
    takes them, labels int32 in [0, nreg) (host arrays or, next to resident columns, a DeviceArray).  A cross count walks twice
    (sets exchanged) for `second`"""
    kw = dict(pimax=pimax, npibins=npibins, mu_max=mu_max, nmubins=nmubins)
    return _count_jk('paircount_jk', mode, bins, (X1, Y1, Z1), (X2, Y2, Z2), (W1, W2), (labels1, labels2), nreg,
                     (C.c_float(boxsize),), kw, True)


def paircount_los_jk(mode, X1, Y1, Z1, bins, labels1, nreg, X2=None, Y2=None, Z2=None, labels2=None, W1=None, W2=None,
                     origin=(0.0, 0.0, 0.0), pimax=0.0, npibins=0, mu_max=1.0, nmubins=0, want_sums=True):
    """per-region pair counts on the light cone (`abacus_paircount_los_jk[_dev]`), columns and origin as `_paircount_los`;
    `want_sums` false: integer counts only (wsum None)"""
    origin, centre = tc._los_origin(origin)
    kw = dict(pimax=pimax, npibins=npibins, mu_max=mu_max, nmubins=nmubins)
    return _count_jk('paircount_los_jk', mode, bins, (X1, Y1, Z1), (X2, Y2, Z2), (W1, W2), (labels1, labels2), nreg, (ptr(origin),),
                     kw, want_sums, host_prep=centre)


def _split(nsplit):
    n = (nsplit,) * 3 if np.isscalar(nsplit) else tuple(nsplit)
    if len(n) != 3 or any(int(v) != v or v < 1 for v in n):
        raise ValueError(f'nsplit must be a positive int or three of them, got {nsplit!r}')
    n = tuple(int(v) for v in n)
    if n[0] * n[1] * n[2] > 65535:
        raise ValueError('at most 65535 regions')
    return n


def box_regions(x, y, z, lbox, nsplit):
    """labels of an nx x ny x nz split of the periodic box: (cx ny + cy) nz + cz with c = int(frac(float32(v) / L) n), the
    fraction wrapped into [0, 1) in float32 like the counter's cell grid does (a coordinate that rounds to L lands in sub-box
    0).  Host columns: an int32 array; DeviceArray columns of one dtype: an int32 DeviceArray, computed in HBM"""
    nx, ny, nz = _split(nsplit)
    cols = (x, y, z)
    if all(isinstance(c, _lib.DeviceArray) for c in cols):
        if any(c.dtype != x.dtype for c in cols) or x.dtype not in (np.float32, np.float64):
            raise TypeError('device-resident coordinates: float32 or float64 columns of one dtype')
        n = len(x)
        out = _lib.DeviceArray(nbytes=4 * n, dtype=np.int32, shape=(n,))
        check(_lib.lib().abacus_jk_box_labels_dev(x.ptr, y.ptr, z.ptr, 0 if x.dtype == np.float32 else 1, C.c_int64(n),
                                                  C.c_float(lbox), nx, ny, nz, out.ptr))
        return out
    if any(isinstance(c, _lib.DeviceArray) for c in cols):
        raise TypeError('device-resident coordinates: every column must be a DeviceArray')
    inv = np.float32(1.0) / np.float32(lbox)

    def coord(v, nc):
        f = np.asarray(v).astype(np.float32) * inv
        f = f - np.floor(f)
        with np.errstate(invalid='ignore'):
            c = (f * np.float32(nc)).astype(np.int32)
        return np.clip(c, 0, nc - 1)
    return ((coord(x, nx) * ny + coord(y, ny)) * nz + coord(z, nz)).astype(np.int32)


# ------------------------------------------------------------------------------------------------ NumPy algebra ----
def _delete_one(total, first, second, both, alpha):
    total, first, second, both = (np.asarray(a) for a in (total, first, second, both))
    if alpha == 1 and all(np.issubdtype(a.dtype, np.integer) for a in (total, first, second, both)):
        t, f, s, b = (a.astype(np.int64) for a in (total, first, second, both))
        return t[None] - f - s + b               # exact: the counts of the catalogue without region k
    t, f, s, b = (a.astype(np.float64) for a in (total, first, second, both))
    return t[None] - b - alpha * (f + s - 2.0 * b)


def delete_one(counts, cross_weight=1.0):
    """D_-k = total - both_k - cross_weight (first_k + second_k - 2 both_k) for every region k: of a `JKCounts` a `JKTerm`
    (npairs in int64 for cross_weight 1, else float64; wsum float64), of a dict of arrays total / first / second / both an array"""
    if isinstance(counts, JKCounts):
        n = _delete_one(counts.total.npairs, counts.first.npairs, counts.second.npairs, counts.both.npairs, cross_weight)
        w = None
        if counts.first.wsum is not None:
            w = _delete_one(counts.total.wsum, counts.first.wsum, counts.second.wsum, counts.both.wsum, cross_weight)
        return JKTerm(n, w)
    return _delete_one(counts['total'], counts['first'], counts['second'], counts['both'], cross_weight)


def region_sums(labels, nreg, w=None):
    """(W_k, sum_{i in k} w_i^2) per region in float64; unit weights: the region's population, twice"""
    lab = labels.get() if isinstance(labels, _lib.DeviceArray) else np.asarray(labels)
    if lab.size and (lab.min() < 0 or lab.max() >= nreg):
        raise ValueError(f'labels span [{lab.min()}, {lab.max()}], outside [0, {nreg})')
    if w is None:
        pop = np.bincount(lab, minlength=nreg).astype(np.float64)
        return pop, pop.copy()
    hw = tc._host(w).astype(np.float64)
    return np.bincount(lab, weights=hw, minlength=nreg), np.bincount(lab, weights=hw * hw, minlength=nreg)


def delete_one_norm(w1_regions, w2_regions=None, cross_weight=1.0, sq_regions=None):
    """the delete-one formula on the pair normalisations: first = W1_k W2, second = W1 W2_k, both = W1_k W2_k, total = W1 W2
    with W_k a sample's weight in region k.  Ordered autocorrelation (`w2_regions` None, `sq_regions` = sum_{i in k} w_i^2):
    the self terms leave first, second and both by sq_k and total by sum_k sq_k.  Returns (total, array of the nreg delete-one
    normalisations)"""
    a = np.asarray(w1_regions, dtype=np.float64)
    auto = w2_regions is None
    b = a if auto else np.asarray(w2_regions, dtype=np.float64)
    big1, big2 = a.sum(), b.sum()
    first, second, both, total = a * big2, big1 * b, a * b, big1 * big2
    if auto:
        if sq_regions is None:
            raise ValueError('an autocorrelation needs sq_regions (sum of w^2 per region)')
        sq = np.asarray(sq_regions, dtype=np.float64)
        first, second, both, total = first - sq, second - sq, both - sq, total - sq.sum()
    elif sq_regions is not None:
        raise ValueError('sq_regions belongs to an autocorrelation')
    return total, _delete_one(np.float64(total), first, second, both, cross_weight)


def jackknife_covariance(samples):
    """(n - 1) / n sum_k (theta_k - mean)(theta_k - mean)^T over the n rows of `samples`"""
    s = np.asarray(samples, dtype=np.float64)
    if s.ndim != 2 or s.shape[0] < 1:
        raise ValueError('samples must be (nreg, nstat)')
    n = s.shape[0]
    d = s - s.mean(axis=0)
    return (n - 1) / n * (d.T @ d)


# ------------------------------------------------------------------------------------------------ periodic box ----
def natural_samples(counts, rr, share1, share2, stat, weighted):
    """the box estimator on per-region counts (arrays or a JKCounts): full = stat(DD, RR) with DD = total, sample k =
    stat(D_-k, RR (1 - share1_k / 2 - share2_k / 2)) with D_-k at cross_weight 1/2 and share_k = W_k / W of a sample"""
    if isinstance(counts, JKCounts):
        pick = (lambda t: t.wsum) if weighted else (lambda t: t.npairs)
        counts = dict(total=pick(counts.total), first=pick(counts.first), second=pick(counts.second), both=pick(counts.both))
    full = stat(counts['total'], rr)
    dk = _delete_one(counts['total'], counts['first'], counts['second'], counts['both'], 0.5)
    rr64 = np.asarray(rr, dtype=np.float64)
    factor = 1.0 - 0.5 * np.asarray(share1, dtype=np.float64) - 0.5 * np.asarray(share2, dtype=np.float64)
    samples = np.stack([np.ravel(stat(dk[k], rr64 * factor[k])) for k in range(len(factor))])
    return full, samples, jackknife_covariance(samples)


def _box_jk(mode, sample1, sample2, w1, w2, regions1, regions2, nreg, edges, lbox, shell_measure, nsub, stat, cross_weight, **kw):
    if cross_weight != 0.5:
        raise NotImplementedError(
            f'cross_weight={cross_weight!r}: the natural estimator of a periodic box supports 0.5 only.  With 0.5 the expected '
            'random count of the reduced sample follows from each region\'s share of the weight, RR (1 - W1_k / 2 W1 - W2_k / 2 W2); '
            'any other value needs the volume of every bin\'s shell inside and outside each region, which a label map does not give')
    # `_natural_estimator`'s casts, counts and RR, expression by expression
    cast = lambda cols: [c if isinstance(c, _lib.DeviceArray) else np.asarray(c).astype(np.float32) for c in cols]  # noqa: E731
    first = cast(sample1)
    n1 = float(len(first[0]))
    auto = sample2 is None or sample2[0] is None
    if auto:
        second, n2, regions2, w2 = (None, None, None), n1, None, None
    else:
        second = cast(sample2)
        n2 = len(second[0])
    weighted = w1 is not None or w2 is not None
    counts = paircount_jk(mode, *first, float(lbox), edges, regions1, nreg, *second, labels2=regions2,
                          W1=None if w1 is None else tc._w_arr(w1), W2=None if w2 is None else tc._w_arr(w2), **kw)
    if weighted:
        total = lambda w, n: float(n) if w is None else float(np.sum(tc._host(w), dtype=np.float64))   # noqa: E731
        big1 = total(w1, n1)
        big2 = big1 if auto else total(w2, n2)
        rr = shell_measure / lbox**3 * big1 * big2 * 2
    else:
        rr = shell_measure / lbox**3 * n1 * n2 * 2
    k1 = region_sums(regions1, nreg, w1)[0]
    k2 = k1 if auto else region_sums(regions2, nreg, w2)[0]
    return natural_samples(counts, rr, k1 / k1.sum(), k2 / k2.sum(), stat, weighted)


def calc_wp_jk(x1, y1, z1, rpbins, pimax, lbox, Nthread, regions1, nreg, num_cells=30, x2=None, y2=None, z2=None, w1=None, w2=None,
               regions2=None, cross_weight=0.5):
    """`calc_wp_fast` with its jackknife: (full, samples (nreg, nbins), cov).  Unweighted, `full` is bit-equal to
    `calc_wp_fast`"""
    tc._check_int('pimax', pimax)
    edges = rpbins.astype(np.float32)
    lbox = np.float32(lbox)
    annulus = np.pi * (edges[1:] ** 2 - edges[:-1] ** 2)
    stat = lambda dd, rr: 2 * np.sum(dd.reshape(len(edges) - 1, pimax) / rr[:, None] - 1, axis=1)   # noqa: E731
    return _box_jk(1, (x1, y1, z1), (x2, y2, z2), w1, w2, regions1, regions2, nreg, edges, lbox, annulus, pimax, stat, cross_weight,
                   pimax=np.float32(pimax), npibins=pimax)


def calc_xirppi_jk(x1, y1, z1, rpbins, pimax, pi_bin_size, lbox, Nthread, regions1, nreg, num_cells=20, x2=None, y2=None, z2=None,
                   w1=None, w2=None, regions2=None, cross_weight=0.5):
    """`calc_xirppi_fast` with its jackknife: (full (nbins, pimax / pi_bin_size), samples (nreg, full.size), cov)"""
    tc._check_int('pimax', pimax)
    tc._check_int('pi_bin_size', pi_bin_size)
    if pimax % pi_bin_size:
        raise ValueError('pi_bin_size needs to be an integer divisor of pimax, current values are ', pi_bin_size, pimax)
    edges = rpbins.astype(np.float32)
    lbox = np.float32(lbox)
    annulus = np.pi * (edges[1:] ** 2 - edges[:-1] ** 2) * pi_bin_size
    stat = lambda dd, rr: dd.reshape(len(edges) - 1, pimax // pi_bin_size, pi_bin_size).sum(axis=2) / rr[:, None] - 1   # noqa: E731
    return _box_jk(1, (x1, y1, z1), (x2, y2, z2), w1, w2, regions1, regions2, nreg, edges, lbox, annulus, pimax, stat, cross_weight,
                   pimax=np.float32(pimax), npibins=pimax)


def calc_multipole_jk(x1, y1, z1, sbins, lbox, Nthread, regions1, nreg, nbins_mu=50, num_cells=20, x2=None, y2=None, z2=None,
                      orders=[0, 2], w1=None, w2=None, regions2=None, cross_weight=0.5):
    """`calc_multipole_fast` with its jackknife: (full, samples (nreg, len(full)), cov)"""
    edges = sbins.astype(np.float32)
    lbox = np.float32(lbox)
    mu_edges = np.linspace(0, 1, nbins_mu + 1)
    wedge = 2 * np.pi / 3 * (edges[1:, None] ** 3 - edges[:-1, None] ** 3) * (mu_edges[None, 1:] - mu_edges[None, :-1])

    def stat(dd, rr):
        xi = dd.reshape(len(edges) - 1, nbins_mu) / rr - 1
        return np.concatenate([tc.tpcf_multipole(xi, mu_edges, order=ell) for ell in orders])
    return _box_jk(2, (x1, y1, z1), (x2, y2, z2), w1, w2, regions1, regions2, nreg, edges, lbox, wedge, nbins_mu, stat, cross_weight,
                   mu_max=1, nmubins=nbins_mu)


# -------------------------------------------------------------------------------------------------- light cone ----
class LCRandomsJK(tc.LCRandoms):
    """`LCRandoms` whose points carry jackknife labels: `regions` (int32 in [0, nreg), a host array or a DeviceArray).  The
    per-region RR is counted once per (mode, bins, pi / mu binning, weighted or not) and kept, like `rr()` keeps RR"""

    def __init__(self, x, y, z, regions, nreg, w=None, origin=(0.0, 0.0, 0.0), nbar=None):
        super().__init__(x, y, z, w, origin, nbar)
        _check_labels('regions', regions, self.n)
        self.nreg = int(nreg)
        self.regions = regions if isinstance(regions, _lib.DeviceArray) else _lib.DeviceArray(_i4(regions))
        self._rr_jk = {}
        self.rr_jk_counted = 0      # per-region RR runs so far (a cache hit does not count)

    def rr_jk(self, mode, bins, geom, weighted):
        key = (int(mode), _f4(bins).tobytes(), tuple(sorted(geom.items())), bool(weighted))
        if key not in self._rr_jk:
            self._rr_jk[key] = _ls_counts(mode, self, None, self.regions, None, self.nreg, bins, geom, weighted)
            self.rr_jk_counted += 1
        return self._rr_jk[key]


def _ls_counts(mode, a, b, la, lb, nreg, bins, geom, weighted):
    """JKCounts of centred sample `a` with itself (b None) or with `b`; unweighted: integer counts only"""
    second = (None, None, None) if b is None else b.cols
    return paircount_los_jk(mode, *a.cols, bins, la, nreg, *second, labels2=lb, W1=a.w if weighted else None,
                            W2=None if b is None or not weighted else b.w, want_sums=weighted, **geom)


def _dev_labels(lab, n, name):
    _check_labels(name, lab, n)
    return lab if isinstance(lab, _lib.DeviceArray) else _lib.DeviceArray(_i4(lab))


def check_populated(nreg, *labels):
    """ValueError when a region holds no point of any of the label arrays (the data samples and the randoms)"""
    pop = sum(np.bincount(np.asarray(lab), minlength=nreg)[:nreg] for lab in labels)
    if np.any(pop == 0):
        raise ValueError(f'regions {np.flatnonzero(pop == 0).tolist()} hold no point of the data or the randoms: their delete-one '
                         'samples would repeat the full estimate and shrink the covariance')


def _ls_jk(mode, s1, s2, w1, w2, regions1, regions2, nreg, randoms, bins, geom, cross_weight, stat):
    if not isinstance(randoms, LCRandomsJK):
        raise TypeError('randoms must be an LCRandomsJK (randoms with regions)')
    if randoms.nreg != nreg:
        raise ValueError(f'the randoms carry {randoms.nreg} regions, the data {nreg}')
    auto = s2 is None
    l1 = _dev_labels(regions1, s1.n, 'regions1')
    l2 = None if auto else _dev_labels(regions2, s2.n, 'regions2')
    w1k, sq1k = region_sums(l1, nreg, w1)
    w2k, sq2k = (w1k, sq1k) if auto else region_sums(l2, nreg, w2)
    wrk, sqrk = region_sums(randoms.regions, nreg, None if randoms.w is None else randoms.w)
    check_populated(nreg, *(lab.get() for lab in (l1, randoms.regions) + (() if auto else (l2,))))
    weighted = s1.w is not None or randoms.w is not None or (s2 is not None and s2.w is not None)
    pick = (lambda t: t.wsum) if weighted else (lambda t: t.npairs)
    arrays = lambda c: dict(total=pick(c.total), first=pick(c.first), second=pick(c.second), both=pick(c.both))   # noqa: E731
    rr = arrays(randoms.rr_jk(mode, bins, geom, weighted))
    d1r = arrays(_ls_counts(mode, s1, randoms, l1, randoms.regions, nreg, bins, geom, weighted))
    n1r = delete_one_norm(w1k, wrk, cross_weight)
    if auto:
        dd, n12 = arrays(_ls_counts(mode, s1, None, l1, None, nreg, bins, geom, weighted)), delete_one_norm(w1k, None, cross_weight, sq1k)
        d2r, n2r = d1r, n1r
    else:
        dd, n12 = arrays(_ls_counts(mode, s1, s2, l1, l2, nreg, bins, geom, weighted)), delete_one_norm(w1k, w2k, cross_weight)
        d2r, n2r = arrays(_ls_counts(mode, s2, randoms, l2, randoms.regions, nreg, bins, geom, weighted)), delete_one_norm(w2k, wrk, cross_weight)
    nrr = delete_one_norm(wrk, None, cross_weight, sqrk)
    terms, norms = (dd, d1r, d2r, rr), (n12, n1r, n2r, nrr)
    f8 = lambda a: np.asarray(a, dtype=np.float64)   # noqa: E731
    full = stat(*(f8(t['total']) for t in terms), *(n[0] for n in norms))
    dels = [f8(delete_one(t, cross_weight)) for t in terms]
    samples = np.stack([np.ravel(stat(*(d[k] for d in dels), *(n[1][k] for n in norms))) for k in range(nreg)])
    return full, samples, jackknife_covariance(samples)


def calc_xirppi_lc_jk(x1, y1, z1, rpbins, pimax, pi_bin_size, randoms, regions1, nreg, Nthread=1, x2=None, y2=None, z2=None, w1=None,
                      w2=None, origin=(0.0, 0.0, 0.0), regions2=None, cross_weight=1.0):
    """`calc_xirppi_lc` with its jackknife: (full, samples (nreg, full.size), cov); randoms: an `LCRandomsJK`"""
    tc._check_int('pimax', pimax)
    tc._check_int('pi_bin_size', pi_bin_size)
    if pimax % pi_bin_size:
        raise ValueError('pi_bin_size needs to be an integer divisor of pimax, current values are ', pi_bin_size, pimax)
    edges = np.asarray(rpbins).astype(np.float32)
    s1, s2 = tc._ls_samples(x1, y1, z1, x2, y2, z2, w1, w2, origin)
    group = lambda a: a.reshape(len(edges) - 1, pimax // pi_bin_size, pi_bin_size).sum(axis=2)   # noqa: E731
    stat = lambda dd, d1r, d2r, rr, *norms: tc.landy_szalay(group(dd), group(d1r), group(d2r), group(rr), *norms)   # noqa: E731
    return _ls_jk(1, s1, s2, w1, w2, regions1, regions2, nreg, randoms, edges, dict(pimax=float(pimax), npibins=int(pimax)),
                  cross_weight, stat)


def calc_wp_lc_jk(x1, y1, z1, rpbins, pimax, randoms, regions1, nreg, Nthread=1, x2=None, y2=None, z2=None, w1=None, w2=None,
                  origin=(0.0, 0.0, 0.0), regions2=None, cross_weight=1.0):
    """`calc_wp_lc` with its jackknife: (full, samples (nreg, nbins), cov); randoms: an `LCRandomsJK`.  With cross_weight 1
    sample k is the estimate of data and randoms without region k"""
    tc._check_int('pimax', pimax)
    edges = np.asarray(rpbins).astype(np.float32)
    s1, s2 = tc._ls_samples(x1, y1, z1, x2, y2, z2, w1, w2, origin)
    shape = lambda a: a.reshape(len(edges) - 1, pimax)   # noqa: E731
    stat = lambda dd, d1r, d2r, rr, *norms: 2 * np.sum(tc.landy_szalay(shape(dd), shape(d1r), shape(d2r), shape(rr), *norms), axis=1)   # noqa: E731
    return _ls_jk(1, s1, s2, w1, w2, regions1, regions2, nreg, randoms, edges, dict(pimax=float(pimax), npibins=int(pimax)),
                  cross_weight, stat)


def calc_multipole_lc_jk(x1, y1, z1, sbins, randoms, regions1, nreg, Nthread=1, nbins_mu=50, x2=None, y2=None, z2=None, orders=[0, 2],
                         w1=None, w2=None, origin=(0.0, 0.0, 0.0), regions2=None, cross_weight=1.0):
    """`calc_multipole_lc` with its jackknife: (full, samples (nreg, len(full)), cov); randoms: an `LCRandomsJK`"""
    edges = np.asarray(sbins).astype(np.float32)
    mu_edges = np.linspace(0, 1, nbins_mu + 1)
    s1, s2 = tc._ls_samples(x1, y1, z1, x2, y2, z2, w1, w2, origin)
    shape = lambda a: a.reshape(len(edges) - 1, nbins_mu)   # noqa: E731

    def stat(dd, d1r, d2r, rr, *norms):
        xi = tc.landy_szalay(shape(dd), shape(d1r), shape(d2r), shape(rr), *norms)
        return np.concatenate([tc.tpcf_multipole(xi, mu_edges, order=ell) for ell in orders])
    return _ls_jk(2, s1, s2, w1, w2, regions1, regions2, nreg, randoms, edges, dict(mu_max=1.0, nmubins=int(nbins_mu)), cross_weight,
                  stat)
