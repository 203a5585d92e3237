"""Plain NumPy float64 statements of what every pass of the hand-written transform (csrc/fft.hip) leaves in memory, and of the
index rule of the pencil transpose (slab_pack / slab_unpack, csrc/power.hip): the judges of tests/test_fft_passes_*.py.  Helper,
not a test module; NumPy only, nothing of the package.

  plain form   z + y passes of a plane: fft(rfft(plane, axis z), axis y); x pass of a y-row: fft along x.  Natural order.
  fused form   the z pass applies the first radix-2 DIF stage of y and of x on its way out (fft_z_r2c<.., FUSE>), the y and x
               passes are two independent n/2-point transforms over rows [0, n/2) and [n/2, n).  Row r of either axis then holds
               frequency f[r] = 2 (r mod n/2) + (r div n/2); a plane pair (x, x + n/2) is stored as the sum and the twiddled
               difference of its two transformed planes.  All pairs + `x_fused` = rfftn(a)[f][:, f].
  transpose    send[q][s h + p][yl][k] = data[s xsep + p][q nyl + yl][k];  out[yl][s n/2 + q h + p][k] = recv[q][s h + p][yl][k].
"""
import numpy as np


def zy_plain(planes):
    """(..., y, z) real -> (..., ky, kz <= n/2) complex128"""
    return np.fft.fft(np.fft.rfft(np.asarray(planes, dtype=np.float64), axis=-1), axis=-2)


def perm(n):
    """f[r]: the frequency held by row r of the fused form"""
    r = np.arange(n)
    return 2 * (r % (n // 2)) + r // (n // 2)


def fuse_pair(T0, T1, xg, n):
    """first radix-2 DIF stage of x on two transformed planes (`zy_plain` of global x = xg and xg + n/2), rows in the order f"""
    f = perm(n)
    return (T0 + T1)[f], ((T0 - T1) * np.exp(-2j * np.pi * xg / n))[f]


def zy_fused(P0, P1, xg, n):
    """the planes with global x = xg and xg + n/2 after the fused z + y passes: (stored first plane, stored second plane)"""
    return fuse_pair(zy_plain(P0), zy_plain(P1), xg, n)


def x_plain(G):
    """layout (y_local, x, k)"""
    return np.fft.fft(np.asarray(G, dtype=np.complex128), axis=1)


def x_fused(G):
    G = np.asarray(G, dtype=np.complex128)
    H = G.shape[1] // 2
    return np.concatenate([np.fft.fft(G[:, :H], axis=1), np.fft.fft(G[:, H:], axis=1)], axis=1)


def impulses_zy(n, points):
    """closed form of `zy_plain` of a plane that is zero but for the weights w at (y0, z0): sum w exp(-2 pi i (ky y0 + kz z0) / n),
    points = [(y0, z0, w), ...] - no transform involved"""
    ky, kz = np.arange(n)[:, None], np.arange(n // 2 + 1)[None, :]
    out = np.zeros((n, n // 2 + 1), dtype=np.complex128)
    for y0, z0, w in points:
        # the phase from the integer product mod n: exact arguments whatever the size
        out += w * np.exp(-2j * np.pi * ((ky * y0 + kz * z0) % n) / n)
    return out


def pack(data, send, world, h, xsep, p0, pc):
    """slab_pack: data (planes, n, cols) of one rank, send (world, 2 h, nyl, cols); the pairs [p0, p0 + pc)"""
    nyl = data.shape[1] // world
    for q in range(world):
        for s in range(2):
            for p in range(p0, p0 + pc):
                send[q, s * h + p] = data[s * xsep + p, q * nyl:(q + 1) * nyl]
    return send


def unpack(recv, n):
    """slab_unpack: recv (world, 2 h, nyl, cols) -> out (nyl, n, cols)"""
    world, h2, nyl, cols = recv.shape
    h = h2 // 2
    out = np.empty((nyl, n, cols), dtype=recv.dtype)
    for q in range(world):
        for s in range(2):
            for p in range(h):
                out[:, s * (n // 2) + q * h + p] = recv[q, s * h + p]
    return out
