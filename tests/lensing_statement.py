"""A chunked NumPy statement of the projected mass sums (include/abacus_hip.h, abacus_lens_profile): the judge of
csrc/lens.hip's lens_walk (helper of tests/test_lensing_*.py, not a test module).

Per (galaxy, particle) pair, in float32 like tests/spheres_statement.py's cylinders without the dz test: d = g - p per
component, minimum image by ONE addition of -+L when |d| > L/2, r2 = dx dx + dy dy left to right.  With e2 = edges * edges in
float32 the row of a pair is np.searchsorted(e2, r2, side='right'): 0 for the inner disc r2 < e2[0], b + 1 for the bin
e2[b] <= r2 < e2[b + 1], nb + 1 (dropped) for r2 >= e2[nb].

`projected_sums(...)` returns (npairs, wsum, asum): npairs uint64 and exact; wsum the sum of float64(gw) * float64(pm) over
the row's pairs by math.fsum - every product is exact in float64 and fsum rounds once, so wsum is the correctly rounded sum;
asum the fsum of |product|, the scale of the device's tolerance.
"""
import math

import numpy as np


def projected_sums(px, py, gx, gy, boxsize, edges, pm=None, gw=None, chunk=256):
    f4 = lambda a: np.ascontiguousarray(a, dtype=np.float32)   # noqa: E731
    px, py, gx, gy = f4(px), f4(py), f4(gx), f4(gy)
    edges = f4(edges)
    e2 = edges * edges                                    # float32 products
    rows = len(edges)
    box = np.float32(boxsize)
    half = box * np.float32(0.5)
    pm = np.ones(len(px), np.float64) if pm is None else f4(pm).astype(np.float64)
    gw = np.ones(len(gx), np.float64) if gw is None else f4(gw).astype(np.float64)

    def image(d):
        return np.where(d > half, d - box, np.where(d < -half, d + box, d))

    npairs = np.zeros(rows, np.uint64)
    terms = [[] for _ in range(rows)]
    for a in range(0, len(gx), chunk):
        if len(px) == 0:
            break
        b = min(a + chunk, len(gx))
        dx = image(gx[a:b, None] - px[None, :])
        dy = image(gy[a:b, None] - py[None, :])
        r2 = dx * dx + dy * dy
        assert r2.dtype == np.float32
        row = np.searchsorted(e2, r2.ravel(), side='right').reshape(r2.shape)
        prod = gw[a:b, None] * pm[None, :]                # exact: two float32 values
        for r in range(rows):
            hit = row == r
            npairs[r] += np.uint64(hit.sum())
            terms[r].append(prod[hit])
    wsum = np.array([math.fsum(np.concatenate(t)) if t else 0.0 for t in terms])
    asum = np.array([math.fsum(np.abs(np.concatenate(t))) if t else 0.0 for t in terms])
    return npairs, wsum, asum
