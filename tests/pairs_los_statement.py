"""A chunked NumPy statement of the light-cone pair counter (csrc/pairs.hip: pair_count_los, C ABI abacus_paircount_los): the
judge of tests/test_pairs_los_*.py, not a test module.  No Corrfunc run stands behind these conventions; they are the
contract of include/abacus_hip.h restated:

points: p = float32(column - origin[d]), the subtraction in the column's own dtype.  Per ordered pair (self pairs of an
autocorrelation excluded): d = p_i - p_j and l = p_i + p_j in float32; then float64, left to right: s2 = dx dx + dy dy + dz dz,
l2 = lx lx + ly ly + lz lz, t = dx lx + dy ly + dz lz, pi2 = t t / l2; l2 == 0: not counted in modes 1 and 2.
mode 0 bins s2.  mode 1: pi = sqrt(pi2) < float64(float32(pimax)), rp2 = max(s2 - pi2, 0) is binned, sub = int(pi / (pimax /
npibins)).  mode 2 bins s2, mu = s2 > 0 ? sqrt(pi2 / s2) : 0 < mu_max, sub = int(mu * (nmubins / mu_max)).  sub >= the number
of sub-bins drops the pair.  Edges are float32, compared as float64(edge) * float64(edge): e2[b] <= q < e2[b + 1].

`paircount(...)` returns per (bin, sub-bin): npairs (uint64), wsum = sum w_i w_j (float64 products of float32 weights),
rsum = sum sqrt(q) of the q that chose the bin (float64) and wabs = sum |w_i w_j|.  The products (24 + 24 bits) are exact and
the float64 square roots correctly rounded on both sides, so the device differs by the order of summation only:
`bounds` = n_b 2^-52 sum_b |term| for both sums.
"""
import numpy as np

MODES = {'r': 0, 'rppi': 1, 'smu': 2}


def centre(cols, origin=(0.0, 0.0, 0.0)):
    """observer-centred float32 columns: float64 columns subtract in float64, float32 columns in float32, one rounding"""
    out = []
    for c, o in zip(cols, origin):
        c = np.ascontiguousarray(c)
        if c.dtype != np.float64:
            c = c.astype(np.float32)
        out.append((c - c.dtype.type(o)).astype(np.float32))
    return out


def paircount(mode, x1, y1, z1, bins, x2=None, y2=None, z2=None, w1=None, w2=None, origin=(0.0, 0.0, 0.0), pimax=0.0,
              npibins=0, mu_max=1.0, nmubins=0, chunk=256):
    mode = MODES.get(mode, mode)
    f4 = lambda a: np.ascontiguousarray(a, dtype=np.float32)   # noqa: E731
    auto = x2 is None
    x1, y1, z1 = centre((x1, y1, z1), origin)
    x2, y2, z2 = (x1, y1, z1) if auto else centre((x2, y2, z2), origin)
    n1, n2 = len(x1), len(x2)
    w1 = np.ones(n1, np.float32) if w1 is None else f4(w1)
    w2 = w1 if auto else (np.ones(n2, np.float32) if w2 is None else f4(w2))
    w1d, w2d = w1.astype(np.float64), w2.astype(np.float64)
    e2 = f4(bins).astype(np.float64)
    e2 = e2 * e2
    nb = len(e2) - 1
    nsub = 1 if mode == 0 else (npibins if mode == 1 else nmubins)
    pimax_d, mu_max_d = np.float64(np.float32(pimax)), np.float64(np.float32(mu_max))
    dpi = pimax_d / npibins if npibins > 0 else np.float64(1)
    inv_dmu = nmubins / mu_max_d if nmubins > 0 else np.float64(1)
    ntot = nb * nsub
    npairs = np.zeros(ntot, np.uint64)
    wsum, rsum, wabs = np.zeros(ntot), np.zeros(ntot), np.zeros(ntot)
    if n2 == 0:
        return npairs, wsum, rsum, wabs
    for a in range(0, n1, chunk):
        b = min(a + chunk, n1)
        d = [(u[a:b, None] - v[None, :]) for u, v in ((x1, x2), (y1, y2), (z1, z2))]
        ell = [(u[a:b, None] + v[None, :]) for u, v in ((x1, x2), (y1, y2), (z1, z2))]
        assert d[0].dtype == np.float32 and ell[0].dtype == np.float32
        dx, dy, dz = (c.astype(np.float64) for c in d)
        ok = np.ones(dx.shape, bool)
        if auto:
            ok[np.arange(b - a), np.arange(a, b)] = False
        s2 = dx * dx + dy * dy + dz * dz
        sub = np.zeros(dx.shape, np.int64)
        q = s2
        if mode != 0:
            lx, ly, lz = (c.astype(np.float64) for c in ell)
            l2 = lx * lx + ly * ly + lz * lz
            t = dx * lx + dy * ly + dz * lz
            ok &= l2 != 0
            with np.errstate(divide='ignore', invalid='ignore'):
                pi2 = t * t / l2
                if mode == 1:
                    pi = np.sqrt(pi2)
                    ok &= pi < pimax_d
                    q = np.maximum(s2 - pi2, 0.0)
                    sub = np.where(ok, pi / dpi, 0.0).astype(np.int64)
                else:
                    mu = np.where(s2 > 0, np.sqrt(pi2 / s2), 0.0)
                    ok &= mu < mu_max_d
                    sub = np.where(ok, mu * inv_dmu, 0.0).astype(np.int64)
            ok &= sub < nsub
        ok &= (q >= e2[0]) & (q < e2[nb])
        ii, jj = np.nonzero(ok)
        qq = q[ii, jj]
        h = (np.searchsorted(e2, qq, 'right') - 1) * nsub + sub[ii, jj]
        ww = w1d[a + ii] * w2d[jj]
        npairs += np.bincount(h, minlength=ntot).astype(np.uint64)
        wsum += np.bincount(h, weights=ww, minlength=ntot)
        wabs += np.bincount(h, weights=np.abs(ww), minlength=ntot)
        rsum += np.bincount(h, weights=np.sqrt(qq), minlength=ntot)
    return npairs, wsum, rsum, wabs


def bounds(npairs, wabs, rsum):
    """the rounding bounds of the device sums: n 2^-52 sum|term| per bin, for wsum and for rsum (terms of rsum are positive)"""
    n = npairs.astype(np.float64) * 2.0 ** -52
    return n * wabs, n * rsum


def scalar(mode, p1, bins, p2=None, w1=None, w2=None, pimax=0.0, npibins=0, mu_max=1.0, nmubins=0):
    """the same conventions as a scalar double loop over already centred float32 points (p: (n, 3) float32): the judge of the
    statement itself on a few dozen points"""
    import math
    mode = MODES.get(mode, mode)
    auto = p2 is None
    p1 = np.asarray(p1, np.float32)
    p2 = p1 if auto else np.asarray(p2, np.float32)
    w1 = np.ones(len(p1), np.float32) if w1 is None else np.asarray(w1, np.float32)
    w2 = w1 if auto else (np.ones(len(p2), np.float32) if w2 is None else np.asarray(w2, np.float32))
    e2 = [float(e) * float(e) for e in np.asarray(bins, np.float32)]
    nb = len(e2) - 1
    nsub = 1 if mode == 0 else (npibins if mode == 1 else nmubins)
    pm, mm = float(np.float32(pimax)), float(np.float32(mu_max))
    npairs = np.zeros(nb * nsub, np.uint64)
    wsum, rsum = np.zeros(nb * nsub), np.zeros(nb * nsub)
    for i in range(len(p1)):
        for j in range(len(p2)):
            if auto and i == j:
                continue
            d = [float(np.float32(p1[i, k] - p2[j, k])) for k in range(3)]
            ell = [float(np.float32(p1[i, k] + p2[j, k])) for k in range(3)]
            s2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
            q, sub = s2, 0
            if mode != 0:
                l2 = ell[0] * ell[0] + ell[1] * ell[1] + ell[2] * ell[2]
                if l2 == 0.0:
                    continue
                t = d[0] * ell[0] + d[1] * ell[1] + d[2] * ell[2]
                pi2 = t * t / l2
                if mode == 1:
                    pi = math.sqrt(pi2)
                    if not pi < pm:
                        continue
                    q = max(s2 - pi2, 0.0)
                    sub = int(pi / (pm / npibins))
                else:
                    mu = math.sqrt(pi2 / s2) if s2 > 0 else 0.0
                    if not mu < mm:
                        continue
                    sub = int(mu * (nmubins / mm))
                if sub >= nsub:
                    continue
            if not (e2[0] <= q < e2[nb]):
                continue
            b = max(k for k in range(nb) if e2[k] <= q)
            h = b * nsub + sub
            npairs[h] += np.uint64(1)
            wsum[h] += float(w1[i]) * float(w2[j])
            rsum[h] += math.sqrt(q)
    return npairs, wsum, rsum


def shell_points(n, seed, chi=(1500.0, 1800.0), origin=(-990.0, -990.0, -990.0), clump=0.5, dtype=np.float64, spread=None):
    """points of an octant shell around `origin` (box coordinates) - of a cone of opening ~ `spread` radians around its
    diagonal when given -, a fraction of them in clumps of 5 Mpc/h"""
    rng = np.random.default_rng(seed)
    u = np.abs(rng.normal(size=(n, 3))) if spread is None else 1.0 + spread * rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    r = np.cbrt(rng.uniform(chi[0] ** 3, chi[1] ** 3, n))
    p = u * r[:, None]
    k = int(n * clump)
    if k:
        centers = p[rng.integers(k, n, max(k // 8, 1))]
        p[:k] = centers[rng.integers(0, len(centers), k)] + rng.normal(0, 5.0, (k, 3))
    p += np.asarray(origin)
    return [p[:, i].astype(dtype) for i in range(3)]
