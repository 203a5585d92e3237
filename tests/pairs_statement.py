"""A chunked NumPy statement of the oracle's pair loop (oracle/abacus_oracle.c, oracle_paircount_brute) that also carries
weights: the judge of the weighted pair counter (helper of tests/test_pairs_weighted_*.py, not a test module).

Per pair, in float32 like the oracle: dx = x1 - x2 (and dy, dz), minimum image by ONE addition of -+L when |d| > L/2,
r^2 = dx dx + dy dy (+ dz dz) left to right, r-bin = searchsorted(edges^2, r^2, 'right') - 1 on float32 squared edges,
pi-bin = int(|dz| / (pimax / npibins)) with |dz| < pimax, mu = |dz| / sqrt(r^2), mu-bin = int(mu * (nmubins / mu_max)) with
mu < mu_max; ordered pairs for an autocorrelation, self pairs excluded.  The weight products and all sums are float64.

`paircount(...)` returns per (bin, sub-bin): npairs (uint64), wsum = sum w_i w_j, rsum = sum of the float32 square root of
the r^2 that chose the bin, and wabs = sum |w_i w_j| (the scale of the rounding bound of wsum).
"""
import numpy as np

MODES = {'r': 0, 'rppi': 1, 'smu': 2}


def paircount(mode, x1, y1, z1, boxsize, bins, x2=None, y2=None, z2=None, w1=None, w2=None, pimax=0.0, npibins=0,
              mu_max=1.0, nmubins=0, chunk=512):
    mode = MODES.get(mode, mode)
    f4 = lambda a: np.ascontiguousarray(a, dtype=np.float32)   # noqa: E731
    auto = x2 is None
    x1, y1, z1 = f4(x1), f4(y1), f4(z1)
    x2, y2, z2 = (x1, y1, z1) if auto else (f4(x2), f4(y2), f4(z2))
    n1, n2 = len(x1), len(x2)
    w1 = np.ones(n1, np.float32) if w1 is None else f4(w1)
    w2 = w1 if auto else (np.ones(n2, np.float32) if w2 is None else f4(w2))
    w1d, w2d = w1.astype(np.float64), w2.astype(np.float64)
    bins = f4(bins)
    nb = len(bins) - 1
    e2 = bins * bins                                     # float32 products, like the oracle's b2[]
    nsub = 1 if mode == 0 else (npibins if mode == 1 else nmubins)
    box = np.float32(boxsize)
    half = box * np.float32(0.5)
    dpi = np.float32(pimax) / np.float32(npibins) if npibins > 0 else np.float32(1)
    inv_dmu = np.float32(nmubins) / np.float32(mu_max) if nmubins > 0 else np.float32(1)
    ntot = nb * nsub
    npairs = np.zeros(ntot, np.uint64)
    wsum, rsum, wabs = np.zeros(ntot), np.zeros(ntot), np.zeros(ntot)

    def image(d):
        return np.where(d > half, d - box, np.where(d < -half, d + box, d))

    for a in range(0, n1, chunk):
        b = min(a + chunk, n1)
        dx = image(x1[a:b, None] - x2[None, :])
        dy = image(y1[a:b, None] - y2[None, :])
        dz = image(z1[a:b, None] - z2[None, :])
        ok = np.ones(dx.shape, bool)
        if auto:
            ok[np.arange(b - a), np.arange(a, b)] = False
        sub = np.zeros(dx.shape, np.int64)
        if mode == 1:
            adz = np.abs(dz)
            r2 = dx * dx + dy * dy
            ok &= adz < np.float32(pimax)
            sub = (adz / dpi).astype(np.int64)
            ok &= sub < npibins
        else:
            r2 = dx * dx + dy * dy + dz * dz
        assert r2.dtype == np.float32
        ok &= (r2 >= e2[0]) & (r2 < e2[nb])
        rb = np.searchsorted(e2, r2.ravel(), 'right').reshape(r2.shape) - 1
        sep = np.sqrt(r2)                                # float32, correctly rounded
        if mode == 2:
            with np.errstate(divide='ignore', invalid='ignore'):
                mu = np.where(sep > 0, np.abs(dz) / sep, np.float32(0))
            ok &= mu < np.float32(mu_max)
            sub = (mu * inv_dmu).astype(np.int64)
            ok &= sub < nmubins
        ii, jj = np.nonzero(ok)
        q = rb[ii, jj] * nsub + sub[ii, jj]
        ww = w1d[a + ii] * w2d[jj]
        npairs += np.bincount(q, minlength=ntot).astype(np.uint64)
        wsum += np.bincount(q, weights=ww, minlength=ntot)
        wabs += np.bincount(q, weights=np.abs(ww), minlength=ntot)
        rsum += np.bincount(q, weights=sep[ii, jj].astype(np.float64), minlength=ntot)
    return npairs, wsum, rsum, wabs


def bounds(npairs, wabs, rsum):
    """the rounding bounds of the device sums: (n 2^-52 sum|w w|, 2^-23 sum r) per bin"""
    return npairs.astype(np.float64) * 2.0 ** -52 * wabs, 2.0 ** -23 * rsum
