"""A chunked NumPy statement of the counts in spheres (include/abacus_hip.h, abacus_spherecount): the judge of
csrc/spheres.hip's sphere_count (helper of tests/test_spheres_*.py, not a test module).

Per (query, data) pair, in float32 like tests/pairs_statement.py and the oracle's pair loop: d = q - p per component,
minimum image by ONE addition of -+L when |d| > L/2, r2 = dx dx + dy dy + dz dz left to right (cylinders: r2 = dx dx + dy dy
and the pair needs |dz| < pimax).  The data point is inside radius j iff r2 < e2[j] with e2 = radii * radii in float32 -
strictly, so counts.sum(axis=0) is the cumulative sum of the pair counter's [lo, hi) bins over the edges (0, r_1 .. r_nr).
Queries that are the data (qx None) do not count themselves, by index: a coincident twin counts.

`count_in_spheres(...)` returns (hist, counts): counts[i, j] = N(<r_j) of query i (uint32, the caller's order) and
hist[j, k] = queries with exactly k points inside r_j for k < kmax, hist[j, kmax] = those with kmax or more (uint64).
"""
import numpy as np


def count_in_spheres(x, y, z, boxsize, radii, qx=None, qy=None, qz=None, pimax=None, kmax=8, chunk=256):
    f4 = lambda a: np.ascontiguousarray(a, dtype=np.float32)   # noqa: E731
    own = qx is None
    x, y, z = f4(x), f4(y), f4(z)
    qx, qy, qz = (x, y, z) if own else (f4(qx), f4(qy), f4(qz))
    radii = np.atleast_1d(f4(radii))
    e2 = radii * radii                                   # float32 products
    nq, nr = len(qx), len(radii)
    box = np.float32(boxsize)
    half = box * np.float32(0.5)

    def image(d):
        return np.where(d > half, d - box, np.where(d < -half, d + box, d))

    counts = np.zeros((nq, nr), np.uint32)
    for a in range(0, nq, chunk):
        if len(x) == 0:
            break
        b = min(a + chunk, nq)
        dx = image(qx[a:b, None] - x[None, :])
        dy = image(qy[a:b, None] - y[None, :])
        dz = image(qz[a:b, None] - z[None, :])
        ok = np.ones(dx.shape, bool)
        if own:
            ok[np.arange(b - a), np.arange(a, b)] = False
        if pimax is not None:
            r2 = dx * dx + dy * dy
            ok &= np.abs(dz) < np.float32(pimax)
        else:
            r2 = dx * dx + dy * dy + dz * dz
        assert r2.dtype == np.float32
        for j in range(nr):
            counts[a:b, j] = (ok & (r2 < e2[j])).sum(axis=1)
    hist = np.zeros((nr, kmax + 1), np.uint64)
    for j in range(nr):
        hist[j] = np.bincount(np.minimum(counts[:, j], kmax), minlength=kmax + 1).astype(np.uint64)
    return hist, counts
