"""A plain float64 statement of the reference's dtype=np.float64 chain (analysis/power_spectrum.py:808-857 get_field,
:1001-1070 get_field_fft, :1131-1319 calc_power with interlaced=False): the judge of the float64-mesh path of csrc/power.hip
(float64 deposit of csrc/tsc.hip, csrc/gfft.hip in double, f64_scale_compensate, f64_raw_power).  Helper of
tests/test_power_f64_*.py, not a test module; NumPy, SciPy and the oracle only, nothing of the package.

  mesh      TSC: oracle.wrap_inplace, then oracle.tsc_scatter into a float64 grid - cloud weights in the dtype of the positions
            (analysis/tsc.py:400), float64 sums in input order.  CIC: analysis/cic.py restated with np.add.at - float64 cloud
            arithmetic whatever the positions' dtype, no wrap of the positions, single-step wrap of the cell indices.
            overdensity = field * float64(M / N) - 1 (:856, :894-898).
  spectrum  scipy.fft.rfftn of the float64 mesh (complex128) times float64(1 / M) (:1058-1060); compensated: divided by the
            FLOAT32 products (W[i] W[j]) W[k] (:1063-1069).  longdouble=True: the same transform of the mesh cast to
            np.longdouble (complex256 where the platform's long double is wider than a double) - only there to measure the
            round-off of the float64 transform itself, `e_ref`.
  power     |a|^2 or Re(conj(a) b) (:707-727) rounded to float32, oracle.bin_kmu with float64 sums, times L^3 (:785-792).
"""
import numpy as np
from scipy.fft import rfftn

from oracle import oracle


def tsc_mesh(pos, Lbox, shape, w=None, d=0.0, grid=None):
    """raw float64 TSC sums; `pos` (float32 or float64, C-contiguous) is wrapped IN PLACE like tsc_parallel does
    (analysis/tsc.py:171-173); `grid`: accumulate into this float64 array instead of a fresh one"""
    if grid is None:
        grid = np.zeros((shape,) * 3 if np.isscalar(shape) else tuple(shape), dtype=np.float64)
    assert grid.dtype == np.float64 and pos.dtype in (np.float32, np.float64)
    oracle.wrap_inplace(pos, Lbox)
    oracle.tsc_scatter(pos, grid, Lbox, weights=w, offset=d)
    return grid


def cic_mesh(pos, Lbox, n, w=None):
    """raw float64 CIC sums (analysis/cic.py:13-125).  A cloud has two non-zero weights per axis - the nearest cell's
    1 - |d| and, on the side the particle leans to, |d| - so 8 of the reference's 27 updates add something; the other 19 add
    0.0 and are left out.  Positions must lie in [0, L]: the reference wraps cell indices by one period only."""
    p = np.asarray(pos)
    assert p.min() >= 0 and p.max() <= Lbox
    W = np.ones(len(p), dtype=np.float64) if w is None else np.asarray(w, dtype=p.dtype).astype(np.float64)
    idx, wt = [], []
    for ax in range(3):
        px = (p[:, ax].astype(np.float64) / Lbox) * n          # float64 whatever the dtype of the positions (:30-33)
        ix = np.rint(px).astype(np.int64)
        dd = ix - px
        side = np.where(dd > 0.0, ix - 1, ix + 1)
        wrap = lambda j: np.where(j >= n, j - n, np.where(j < 0, j + n, j))   # noqa: E731
        idx.append((wrap(ix), wrap(side)))
        wt.append((1.0 - np.abs(dd), np.abs(dd)))
    flat = np.zeros(n * n * n, dtype=np.float64)
    for a in range(2):
        for b in range(2):
            for c in range(2):
                np.add.at(flat, (idx[0][a] * n + idx[1][b]) * n + idx[2][c], wt[0][a] * wt[1][b] * wt[2][c] * W)
    return flat.reshape(n, n, n)


def normalize(field, npart):
    """in place, like the reference's normalize_field(inplace=True)"""
    field *= np.float64(field.size / npart)
    field -= np.float64(1.0)
    return field


def get_field(pos, Lbox, nmesh, paste, w=None, d=0.0):
    paste = paste.upper()
    if paste == 'TSC':
        field = tsc_mesh(pos, Lbox, nmesh, w, d)
    elif paste == 'CIC':
        field = cic_mesh(pos + d if d != 0.0 else pos, Lbox, nmesh, w)
    else:
        raise ValueError(paste)
    return normalize(field, len(pos))


def spectrum(field, W=None, longdouble=False, workers=None):
    """delta_k of a float64 overdensity mesh; W: the 1-D float32 window to compensate with, or None"""
    nmesh = field.shape[0]
    workers = workers or oracle.max_threads()
    if longdouble:
        f = rfftn(field.astype(np.longdouble), workers=workers)
        f *= np.longdouble(1) / np.longdouble(field.size)
    else:
        f = rfftn(field, workers=workers)
        assert f.dtype == np.complex128
        f *= np.float64(1 / field.size)
    if W is not None:
        W = np.asarray(W, dtype=np.float32)
        f /= (W[:, None, None] * W[None, :, None]) * W[None, None, :nmesh // 2 + 1]
    return f


def get_field_fft(pos, Lbox, nmesh, paste, w, W, compensated, longdouble=False):
    return spectrum(get_field(pos, Lbox, nmesh, paste, w), W if compensated else None, longdouble)


def e_ref(field):
    """round-off of the float64 transform: max |float64 - long double| / max |long double|"""
    a, b = spectrum(field), spectrum(field, longdouble=True)
    return float(np.abs(a - b).max() / np.abs(b).max())


def raw_power(a, b=None):
    p = np.abs(a) ** 2 if b is None else (np.conj(a) * b).real
    return p.astype(np.float32)


def calc_power(pos, Lbox, kbins, mubins, k_max=None, paste='TSC', nmesh=128, compensated=True, w=None, pos2=None, w2=None,
               poles=None, logk=False):
    """calc_power(..., interlaced=False, dtype=np.float64) as a dict of the Table's measured columns"""
    if k_max is None:
        k_max = np.pi * nmesh / Lbox
    W = oracle.get_W_compensated(Lbox, nmesh, paste, False) if compensated else None
    a = get_field_fft(pos, Lbox, nmesh, paste, w, W, compensated)
    b = None if pos2 is None else get_field_fft(pos2, Lbox, nmesh, paste, w2, W, compensated)
    ke, me = oracle.get_k_mu_edges(Lbox, k_max, kbins, mubins, logk)
    pl = np.asarray(poles or [], dtype=np.int64)
    power, N_mode, bpoles, N_mode_poles, k_avg = oracle.bin_kmu(nmesh, Lbox, ke, me, raw_power(a, b), pl, accum64=True,
                                                                nthread=oracle.max_threads())
    power *= Lbox ** 3
    bpoles *= Lbox ** 3
    if len(me) == 2:
        power, N_mode, k_avg = power[:, 0], N_mode[:, 0], k_avg[:, 0]
    return dict(power=power, N_mode=N_mode, poles=bpoles.T, N_mode_poles=N_mode_poles, k_avg=k_avg)
