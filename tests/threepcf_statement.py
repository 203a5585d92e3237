"""NumPy statements of the three-point correlation function multipoles (include/abacus_hip.h, abacus_threepcf): the judge of
csrc/threepcf.hip's threepcf_walk.  Two forms:

  brute      per primary the k x k matrix of cosines between its neighbours, Legendre polynomials by recurrence on that matrix, the
             diagonal (j = k) zeroed: O(N k^2), float64, and independent of the algorithm;
  harmonic   the Slepian & Eisenstein (2015) algorithm itself: per primary the real spherical-harmonic sums a[bin][component] of
             its neighbours and their Gram matrix per l, minus the self term on the diagonal: O(N k).  `dtype` sets the precision of
             the directions, the harmonics and the per-primary sums; what is summed over primaries is float64 in both.

Both decide membership with the float32 expressions of the periodic pair counters (d = p_i - p_j per component, one -+L when |d| >
L / 2; r2 = dx dx + dy dy + dz dz left to right; bin b iff e2[b] <= r2 < e2[b + 1] with e2 = edge * edge in float32), and both
normalise a direction in the working precision from the float32 COMPONENTS - not from the float32 r2 that chose the bin, which
would leave 1e-7 on the float64 form.

The components (harmonic): for m = 0 .. lmax with (cm, sm) = (Re, Im) (ux + i uy)^m and R_l^m(uz) from
  R_m^m = D_m,   R_l^m = A_lm uz R_{l-1}^m - B_lm R_{l-2}^m,
  D_0 = 1, D_m = sqrt(2 prod_{k<=m} (2k - 1) / (2k)),   A_lm = (2l - 1) / sqrt(l^2 - m^2),   B_lm = sqrt(((l - 1)^2 - m^2) / (l^2 - m^2)),
component l^2 is R_l^0 and components l^2 + 2m - 1, l^2 + 2m are R_l^m cm, R_l^m sm: sum over the 2l + 1 components of l of
y_c(u1) y_c(u2) = P_l(u1 . u2) (the addition theorem, the m > 0 terms doubled by the sqrt(2) in D_m).
"""
import numpy as np


def ncomp(lmax):
    return (lmax + 1) ** 2


def coefficients(lmax):
    """(D[m], A[l][m], B[l][m]) in float64; A and B are zero where they are not used (l <= m)"""
    D = np.ones(lmax + 1)
    for m in range(1, lmax + 1):
        D[m] = D[m - 1] * np.sqrt((2 * m - 1) / (2 * m))
    D[1:] *= np.sqrt(2.0)
    A, B = np.zeros((lmax + 1, lmax + 1)), np.zeros((lmax + 1, lmax + 1))
    for m in range(lmax + 1):
        for l in range(m + 1, lmax + 1):
            A[l, m] = (2 * l - 1) / np.sqrt(l * l - m * m)
            B[l, m] = np.sqrt(((l - 1) ** 2 - m * m) / (l * l - m * m))
    return D, A, B


def harmonics(u, lmax, dtype=np.float64):
    """the (lmax + 1)^2 real components of every direction of u (k, 3), in `dtype`: (k, ncomp)"""
    D, A, B = (t.astype(dtype) for t in coefficients(lmax))
    u = np.asarray(u, dtype=dtype)
    ux, uy, uz = u[:, 0], u[:, 1], u[:, 2]
    Y = np.zeros((len(u), ncomp(lmax)), dtype=dtype)
    cm, sm = np.ones(len(u), dtype=dtype), np.zeros(len(u), dtype=dtype)
    for m in range(lmax + 1):
        if m:
            cm, sm = cm * ux - sm * uy, sm * ux + cm * uy
        p2 = p1 = np.zeros(len(u), dtype=dtype)        # B[m + 1][m] = 0: R_{m-1}^m never enters
        for l in range(m, lmax + 1):
            r = np.full(len(u), D[m], dtype=dtype) if l == m else A[l, m] * uz * p1 - B[l, m] * p2
            p2, p1 = p1, r
            if m == 0:
                Y[:, l * l] = r
            else:
                Y[:, l * l + 2 * m - 1] = r * cm
                Y[:, l * l + 2 * m] = r * sm
    return Y


def catalogue(x, y, z, w=None, x2=None, y2=None, z2=None, w2=None):
    """set 1 with set 2 appended, as the library appends them: float32 columns and float32 weights (None: 1)"""
    f4 = lambda a: np.ascontiguousarray(a, dtype=np.float32).ravel()   # noqa: E731
    p = np.stack([f4(x), f4(y), f4(z)], axis=1)
    wt = np.ones(len(p), np.float32) if w is None else f4(w)
    if x2 is not None:
        q = np.stack([f4(x2), f4(y2), f4(z2)], axis=1)
        p = np.concatenate([p, q])
        wt = np.concatenate([wt, np.ones(len(q), np.float32) if w2 is None else f4(w2)])
    return p, wt


def neighbours(p, box, edges):
    """per primary i: (i, j, b, d) - the indices of its counted neighbours, their bins and the float32 separation vectors; every
    expression is float32, as the periodic pair counters form it"""
    box = np.float32(box)
    half = box * np.float32(0.5)
    e = np.ascontiguousarray(edges, dtype=np.float32)
    e2 = e * e
    nb = len(e) - 1
    for i in range(len(p)):
        d = p[i] - p
        d = np.where(d > half, d - box, np.where(d < -half, d + box, d)).astype(np.float32)
        r2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        ok = (r2 >= e2[0]) & (r2 < e2[nb])
        ok[i] = False
        j = np.nonzero(ok)[0]
        b = np.searchsorted(e2, r2[j], side='right') - 1
        yield i, j, b, d[j], r2[j]


def _empty(nb, lmax):
    return {'zeta': np.zeros((lmax + 1, nb, nb)), 'wself': np.zeros(nb), 'npairs': np.zeros(nb, dtype=np.uint64)}


def _directions(d, dtype):
    d = d.astype(dtype)
    return d / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])[:, None]


def brute(x, y, z, boxsize, edges, lmax, w=None, x2=None, y2=None, z2=None, w2=None):
    p, wt = catalogue(x, y, z, w, x2, y2, z2, w2)
    nb = len(edges) - 1
    out = _empty(nb, lmax)
    for i, j, b, d, r2 in neighbours(p, boxsize, edges):
        out['npairs'] += np.bincount(b, minlength=nb).astype(np.uint64)
        keep = r2 > 0                                   # a coincident twin has no direction
        j, b, d = j[keep], b[keep], d[keep]
        if not len(j):
            continue
        u = _directions(d, np.float64)
        mu = np.clip(u @ u.T, -1.0, 1.0)
        wj = wt[j].astype(np.float64)
        ww = np.outer(wj, wj)
        np.fill_diagonal(ww, 0.0)
        onehot = np.zeros((len(j), nb))
        onehot[np.arange(len(j)), b] = 1.0
        wi = float(wt[i])
        out['wself'] += wi * (onehot.T @ (wj * wj))
        P0, P1 = np.ones_like(mu), mu
        for l in range(lmax + 1):
            P = P0 if l == 0 else P1
            out['zeta'][l] += wi * (onehot.T @ (ww * P) @ onehot)
            if l >= 1:
                P0, P1 = P1, ((2 * l + 1) * mu * P1 - l * P0) / (l + 1)
    return out


def harmonic(x, y, z, boxsize, edges, lmax, w=None, x2=None, y2=None, z2=None, w2=None, dtype=np.float64):
    p, wt = catalogue(x, y, z, w, x2, y2, z2, w2)
    nb = len(edges) - 1
    out = _empty(nb, lmax)
    for i, j, b, d, r2 in neighbours(p, boxsize, edges):
        out['npairs'] += np.bincount(b, minlength=nb).astype(np.uint64)
        keep = r2 > 0
        j, b, d = j[keep], b[keep], d[keep]
        if not len(j):
            continue
        wj = wt[j].astype(dtype)
        Y = harmonics(_directions(d, dtype), lmax, dtype) * wj[:, None]
        a = np.zeros((nb, ncomp(lmax)), dtype=dtype)
        s2 = np.zeros(nb, dtype=dtype)
        np.add.at(a, b, Y)                               # sequential sums in `dtype`
        np.add.at(s2, b, wj * wj)
        wi = float(wt[i])
        out['wself'] += wi * s2.astype(np.float64)
        for l in range(lmax + 1):
            al = a[:, l * l:(l + 1) * (l + 1)]
            g = al @ al.T
            g[np.arange(nb), np.arange(nb)] -= s2
            out['zeta'][l] += wi * g.astype(np.float64)
    return out


def e_ref(z32, z64):
    """the float32 form against the float64 one: max over l >= 1 of max|difference| / max|float64 form| of that l"""
    return max(np.abs(z32[l] - z64[l]).max() / np.abs(z64[l]).max() for l in range(1, len(z64)))
