"""A chunked NumPy statement of the pairwise velocity sums (include/abacus_hip.h: abacus_pairvel; csrc/pairs.hip: pair_vel): the
loop of pairs_statement.paircount - the same float32 expressions decide which pairs are counted and where - extended by the
velocities.  Helper of tests/test_pairvel_*.py, not a test module.

Per counted ordered pair (i, j): u = v_i - v_j componentwise in float32; then in float64, left to right:
    s2 = dx dx + dy dy + dz dz,  t = ux dx + uy dy + uz dz,  vr = s2 > 0 ? t / sqrt(s2) : 0,  uu = ux ux + uy uy + uz uz,
    vz = uz sign(dz)     (dx, dy, dz: the minimum-image float32 separation; np.sign: sign(0) = 0)
and with ww = (double)w_i (double)w_j the sums npairs, wsum = sum ww, vr1 = sum ww vr, vr2 = sum ww vr^2, u2 = sum ww uu,
vz1 = sum ww vz, vz2 = sum ww uz^2.

`pairvel(...)` returns (sums, scale): two dicts of arrays per (bin, sub-bin).  `sums` holds the seven quantities; `scale` holds for
'wsum' and each of the five velocity sums the sum of the ABSOLUTE terms - the scale of the rounding bounds (`bound`).
"""
import numpy as np

from pairs_statement import MODES

SUMS = ('vr1', 'vr2', 'u2', 'vz1', 'vz2')


def pairvel(mode, x1, y1, z1, vx1, vy1, vz1, boxsize, bins, x2=None, y2=None, z2=None, vx2=None, vy2=None, vz2=None, w1=None,
            w2=None, pimax=0.0, npibins=0, mu_max=1.0, nmubins=0, chunk=512):
    mode = MODES.get(mode, mode)
    f4 = lambda a: np.ascontiguousarray(a, dtype=np.float32)   # noqa: E731
    auto = x2 is None
    x1, y1, z1, vx1, vy1, vz1 = map(f4, (x1, y1, z1, vx1, vy1, vz1))
    x2, y2, z2, vx2, vy2, vz2 = (x1, y1, z1, vx1, vy1, vz1) if auto else map(f4, (x2, y2, z2, vx2, vy2, vz2))
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
    sums = {'npairs': np.zeros(ntot, np.uint64), 'wsum': np.zeros(ntot), **{k: np.zeros(ntot) for k in SUMS}}
    scale = {'wsum': np.zeros(ntot), **{k: np.zeros(ntot) for k in SUMS}}

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
        if mode == 2:
            sep = np.sqrt(r2)                            # float32, correctly rounded
            with np.errstate(divide='ignore', invalid='ignore'):
                mu = np.where(sep > 0, np.abs(dz) / sep, np.float32(0))
            ok &= mu < np.float32(mu_max)
            sub = (mu * inv_dmu).astype(np.int64)
            ok &= sub < nmubins
        ii, jj = np.nonzero(ok)
        q = rb[ii, jj] * nsub + sub[ii, jj]
        ww = w1d[a + ii] * w2d[jj]
        # the velocities of the counted pairs: float32 differences, then float64
        ux, uy, uz = ((v1[a + ii] - v2[jj]).astype(np.float64) for v1, v2 in ((vx1, vx2), (vy1, vy2), (vz1, vz2)))
        assert (vx1[a + ii] - vx2[jj]).dtype == np.float32
        ddx, ddy, ddz = (d[ii, jj].astype(np.float64) for d in (dx, dy, dz))
        s2 = ddx * ddx + ddy * ddy + ddz * ddz
        t = ux * ddx + uy * ddy + uz * ddz
        pos = s2 > 0
        vr = np.zeros_like(t)
        vr[pos] = t[pos] / np.sqrt(s2[pos])
        uu = ux * ux + uy * uy + uz * uz
        vz = uz * np.sign(ddz)
        terms = {'wsum': ww, 'vr1': ww * vr, 'vr2': ww * (vr * vr), 'u2': ww * uu, 'vz1': ww * vz, 'vz2': ww * (uz * uz)}
        sums['npairs'] += np.bincount(q, minlength=ntot).astype(np.uint64)
        for k, v in terms.items():
            sums[k] += np.bincount(q, weights=v, minlength=ntot)
            scale[k] += np.bincount(q, weights=np.abs(v), minlength=ntot)
    return sums, scale


def velocities(cols, box, seed, frame_shift=0.0):
    """test velocities for the positions `cols` (three columns in [frame_shift, frame_shift + box)): float32 normal draws of
    width 300 plus a coherent inflow of 5 per unit length towards the box centre"""
    rng = np.random.default_rng(seed)
    centre = frame_shift + 0.5 * box
    return [(rng.normal(0.0, 300.0, len(c)) - 5.0 * (np.asarray(c, dtype=np.float64) - centre)).astype(np.float32) for c in cols]


def bound(npairs, scale_k):
    """|device - statement| of a velocity sum per cell: n float64 additions in any order cost at most n 2^-52 sum|term|, higher
    orders and the statement's own summation included; 8 more for a square root and a division that may each be an ulp from
    NumPy's, doubled in vr^2"""
    return (npairs.astype(np.float64) + 8.0) * 2.0 ** -52 * scale_k
