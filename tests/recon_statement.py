"""A plain NumPy statement of standard plane-parallel BAO reconstruction in a periodic box (line of sight = z), written from the
definition and independent of abacusutils_amd: TEST INFRASTRUCTURE.  It is the yardstick of abacusutils_amd.hod.zcv.reconstruction
(there is no reference implementation); every function takes `dtype`: np.float64 is the statement, np.float32 the same statement
in single precision, whose distance to the float64 one is the noise floor e_ref the device is held to.

The four steps (Chen et al. 2019 conventions, as tools_cv.combine_kaiser_spectra assumes them):

1. delta(k): the tracers (positions modulo L) are deposited with the CIC cloud of analysis/cic.py (8 cells) or the TSC cloud of
   analysis/tsc.py (27 cells): cell i is centred at i L / n, the nearest cell is found by rounding, indices are periodic.
   delta = rho n^3 / N - 1, delta(k) = rfftn(delta) / n^3.
2. psi_i(k) = i k_i S(k) delta(k) / (k^2 b (1 + beta mu^2)), S = exp(-k^2 R^2 / 2), beta = f / b with rsd else 0, mu^2 = k_z^2 / k^2,
   0 for the zero vector.  Wavenumbers: dk = float32(2 pi / L), index i -> i below n/2 and i - n from n/2 on (x, y), 0 .. n/2 on z.
   Nyquist rule: in the factor i k_i ONLY, the wavenumber of axis i is 0 at index n/2 of that axis (k^2, mu^2 and S keep the full
   wavenumber); all three spectra are Hermitian then.
3. psi_i(x) = sum_k psi_i(k) exp(i k x) = irfftn(psi_i(k)) n^3.
4. psi is read at a particle (position modulo L) with the same cloud as the deposit; tracers and recsym randoms move to
   s - psi - f psi_z z^ (f = 0 without rsd), reciso randoms to s - psi; outputs are wrapped into [0, L) with NumPy's remainder.
"""
import numpy as np
import scipy.fft

PASTES = ('CIC', 'TSC')


def wavenumbers(n, L, dtype=np.float64):
    """(kx, kz): the n wavenumbers of the x and y axes and the n/2+1 of the z axis, from dk = float32(2 pi / L)"""
    dk = dtype(np.float32(2.0 * np.pi / L))
    i = np.arange(n)
    kx = np.where(i < n // 2, i, i - n).astype(dtype) * dk
    kz = np.arange(n // 2 + 1).astype(dtype) * dk
    return kx, kz


def cloud(p, n, L, paste, dtype=np.float64):
    """per axis: the periodic cell indices (N, K) and the weights (N, K) of the cloud of `paste` around the coordinates p (N,)
    (K = 2 for CIC: the nearest cell and its neighbour on the particle's side; K = 3 for TSC: i - 1, i, i + 1)"""
    if paste not in PASTES:
        raise ValueError(paste)
    p = np.remainder(np.asarray(p, dtype=dtype), dtype(L))
    g = p * dtype(n / L)
    i0 = np.rint(g)
    d = i0 - g                                # distance from the particle to the centre of its nearest cell, in cells
    i0 = i0.astype(np.int64)
    if paste == 'CIC':                        # analysis/cic.py: 1 - |d| on the nearest cell, |d| on the neighbour towards the particle
        idx = np.stack((i0, np.where(d > 0, i0 - 1, i0 + 1)), axis=1)
        w = np.stack((dtype(1) - np.abs(d), np.abs(d)), axis=1)
    else:                                     # analysis/tsc.py _tsc_scatter
        h = dtype(0.5)
        idx = np.stack((i0 - 1, i0, i0 + 1), axis=1)
        w = np.stack((h * (h + d) ** 2, dtype(0.75) - d * d, h * (h - d) ** 2), axis=1)
    return np.mod(idx, n), w.astype(dtype)


def deposit(pos, n, L, paste, dtype=np.float64):
    """rho (n, n, n): every particle adds wx wy wz to the 8 / 27 cells of its cloud"""
    pos = np.asarray(pos)
    (ix, wx), (iy, wy), (iz, wz) = (cloud(pos[:, a], n, L, paste, dtype) for a in range(3))
    rho = np.zeros((n, n, n), dtype=dtype)
    K = ix.shape[1]
    for a in range(K):
        for b in range(K):
            for c in range(K):
                np.add.at(rho, (ix[:, a], iy[:, b], iz[:, c]), wx[:, a] * wy[:, b] * wz[:, c])
    return rho


def delta_from_particles(pos, n, L, paste, dtype=np.float64):
    rho = deposit(pos, n, L, paste, dtype)
    return rho * dtype(float(n) ** 3 / len(pos)) - dtype(1)


def displacement_spectra(delta, L, bias, f_growth, R, rsd=True, dtype=np.float64):
    """step 2 from a density mesh: the three spectra psi_i(k), complex (3, n, n, n/2+1)"""
    delta = np.asarray(delta, dtype=dtype)
    n = delta.shape[0]
    dk = scipy.fft.rfftn(delta) / dtype(float(n) ** 3)
    kx, kz = wavenumbers(n, L, dtype)
    KX, KY, KZ = kx[:, None, None], kx[None, :, None], kz[None, None, :]
    k2 = KX * KX + KY * KY + KZ * KZ
    beta = dtype(f_growth / bias) if rsd else dtype(0)
    with np.errstate(divide='ignore', invalid='ignore'):
        mu2 = KZ * KZ / k2
        g = np.exp(-k2 * dtype(R * R / 2.0)) / (k2 * dtype(bias) * (dtype(1) + beta * mu2))
    g[0, 0, 0] = 0
    kx_n, kz_n = kx.copy(), kz.copy()
    kx_n[n // 2] = 0                          # the Nyquist rule, in the factor i k_i only
    kz_n[n // 2] = 0
    fac = (kx_n[:, None, None], kx_n[None, :, None], kz_n[None, None, :])
    out = np.stack([(1j * (f * g)).astype(dk.dtype) * dk for f in fac])
    assert out.dtype == (np.complex64 if dtype == np.float32 else np.complex128)
    return out


def displacement_from_delta(delta, L, bias, f_growth, R, rsd=True, dtype=np.float64):
    """steps 2 and 3: psi (3, n, n, n) from a density mesh"""
    spec = displacement_spectra(delta, L, bias, f_growth, R, rsd, dtype)
    n = spec.shape[1]
    psi = np.stack([scipy.fft.irfftn(s, s=(n, n, n)) * dtype(float(n) ** 3) for s in spec])
    assert psi.dtype == dtype
    return psi


def displacement_field(pos, L, n, bias, f_growth, R, rsd=True, paste='CIC', dtype=np.float64):
    """steps 1 to 3: psi (3, n, n, n) from tracer positions"""
    return displacement_from_delta(delta_from_particles(pos, n, L, paste, dtype), L, bias, f_growth, R, rsd, dtype)


def read_out(psi, pos, L, paste, dtype=np.float64):
    """psi (3, n, n, n) at the particles, (N, 3): sum over the cells of the cloud of w psi"""
    psi = np.asarray(psi, dtype=dtype)
    pos = np.asarray(pos)
    n = psi.shape[1]
    (ix, wx), (iy, wy), (iz, wz) = (cloud(pos[:, a], n, L, paste, dtype) for a in range(3))
    out = np.zeros((len(pos), 3), dtype=dtype)
    K = ix.shape[1]
    for a in range(K):
        for b in range(K):
            for c in range(K):
                w = wx[:, a] * wy[:, b] * wz[:, c]
                for q in range(3):
                    out[:, q] += w * psi[q][ix[:, a], iy[:, b], iz[:, c]]
    return out


def shift(pos, psi, L, paste, los_factor, dtype=np.float64):
    """step 4: wrap(s - psi - los_factor psi_z z^), (N, 3)"""
    s = np.remainder(np.asarray(pos, dtype=dtype), dtype(L))
    d = read_out(psi, pos, L, paste, dtype)
    out = s - d
    out[:, 2] = out[:, 2] - dtype(los_factor) * d[:, 2]
    return np.remainder(out, dtype(L))


def reconstruct(tracer_pos, random_pos, L, n, bias, f_growth, R, rec_algo='recsym', rsd=True, paste='CIC', dtype=np.float64):
    """(tracer_rec, random_rec or None, psi)"""
    if rec_algo not in ('recsym', 'reciso'):
        raise ValueError(rec_algo)
    psi = displacement_field(tracer_pos, L, n, bias, f_growth, R, rsd, paste, dtype)
    los = f_growth if rsd else 0.0
    tr = shift(tracer_pos, psi, L, paste, los, dtype)
    rn = None if random_pos is None else shift(random_pos, psi, L, paste, los if rec_algo == 'recsym' else 0.0, dtype)
    return tr, rn, psi


def plane_wave(n, L, A, mode, axis):
    """delta = A cos(k x_axis) on the mesh, float64: the phase at cell i is 2 pi mode i / n exactly (a mode of the mesh); also
    returns the wavenumber the solver assigns to it, k = mode float32(2 pi / L)"""
    k = mode * float(np.float32(2.0 * np.pi / L))
    phase = 2.0 * np.pi * mode * np.arange(n) / n
    shape = [1, 1, 1]
    shape[axis] = n
    return np.broadcast_to(A * np.cos(phase).reshape(shape), (n, n, n)).copy(), k


def plane_wave_displacement(n, L, A, mode, axis, bias, f_growth, R, rsd=True):
    """the closed form psi_axis = -A S(k) sin(k x) / (k b (1 + beta mu^2)) of delta = A cos(k x), mu^2 = 1 along z and 0 otherwise;
    the other two components vanish.  (3, n, n, n) float64; 0 < mode < n/2"""
    k = mode * float(np.float32(2.0 * np.pi / L))
    phase = 2.0 * np.pi * mode * np.arange(n) / n
    beta = f_growth / bias if rsd else 0.0
    amp = -A * np.exp(-k * k * R * R / 2.0) / (k * bias * (1.0 + (beta if axis == 2 else 0.0)))
    shape = [1, 1, 1]
    shape[axis] = n
    psi = np.zeros((3, n, n, n))
    psi[axis] = np.broadcast_to(amp * np.sin(phase).reshape(shape), (n, n, n))
    return psi


def periodic_distance(a, b, L):
    """max over particles and axes of the distance on the circle of length L, float64"""
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    return float(np.minimum(d, L - d).max())


def e_ref(psi32, psi64):
    """the noise floor: max over the components of max|psi32 - psi64| / max|psi64|"""
    return max(float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max()) for a, b in zip(psi32, psi64))


def modulated_particles(N, L, seed, amplitude=0.6, modes=(1, 2, 1)):
    """~N particles of a modulated-uniform density (1 + amplitude prod_i cos(2 pi m_i x_i / L)) by rejection, float32 (M, 3) in [0, L)"""
    rng = np.random.default_rng(seed)
    p = rng.random((int(N * (1 + amplitude)) + 16, 3)) * L
    dens = 1.0 + amplitude * np.prod([np.cos(2 * np.pi * m * p[:, a] / L) for a, m in enumerate(modes)], axis=0)
    keep = rng.random(len(p)) * (1 + amplitude) < dens
    out = p[keep].astype(np.float32)
    out[out >= np.float32(L)] = 0
    return out
