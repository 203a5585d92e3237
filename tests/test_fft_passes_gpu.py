"""Every pass of the hand-written transforms (csrc/fft.hip, csrc/gfft.hip) against a float64 statement, MODE BY MODE.

The binned P(k, mu) the rest of the suite checks the transforms through cannot see a conjugated plane, swapped or mirrored axes or
a shifted origin (the binning is symmetric under all of them), and at production sizes a bin averages so many modes that single
wrong ones vanish below 1e-5.  Here nothing is binned and no mode is left out.

Power-of-two passes run at full row length on a few planes / y-rows through the slab entry points (HipSlabBackend.fft_zy, .fft_x,
.pack, .unpack), judged by tests/fft_statement.py (pinned on the CPU by tests/test_fft_passes_host.py):
  inputs    (a) white noise N(0, 1): every mode has the same expected size, so the max norm is a per-mode test; (b) two impulses
            in one plane, expected spectrum in closed form (no FFT library): permutations, conjugation, off-by-one; (c) the
            checkerboard (-1)^(y+z): only mode (n/2, n/2), the kz = n/2 element of the even/odd split.  The row padding is NaN
            on entry and every compared output must be finite; neighbouring planes hold a sentinel and must come back bit for bit.
  yardstick rho(n): the largest per-mode error of scipy.fft IN FLOAT32 (the reference's transform at the reference's precision)
            on the same white noise against the float64 statement, over the Frobenius norm of the transformed plane (x pass: the
            2-norm of the column; whole meshes: the Frobenius norm of the spectrum).  The device gets 4 rho(n) x that norm of the
            expected output per mode, for every input of that n, and 4 x scipy-float32's relative l2 error over the plane.
            The 4 covers float32 twiddle tables and another radix order; a structural error is ~1e6 rho.
Mixed radix (no entry point takes a caller's mesh): unweighted particles on integer cell centres of a box L = n make the TSC
deposit exact (dyadic weights), so get_field must EQUAL the NumPy mesh and get_field_fft is judged per mode against rfftn of it.
1536 is left out: its spectrum alone is 14.5 GB to bring back.  At 768 and 1024 the float64 reference is restricted to six planes of kx
(see _kx_corners): the whole float64 rfftn takes 4.0 s at 768^3 alone and the NumPy mesh 14 s / 31 s.

Measured on an MI355X: largest device error in units of rho (allowed 4), worst input and plane of each n; the relative l2 error
was between 0.44 and 1.05 x scipy-float32's everywhere (allowed 4).
  z + y plain     64: 1.42   128: 1.16   256: 1.02   512: 1.05   1024: 0.91   2048: 1.12     (impulses <= 0.62, checkerboard exact)
  z + y fused     256: 1.09   1024: 1.01   2048: 1.01 on noise, both geometries; impulses <= 0.59
                  checkerboard: exact but for the twiddled mode (n/2, n/2) of the difference plane, which is 3.6 / 10.4 / 30.4 rho
                  off at 256 / 1024 / 2048 (worst geometry) = 0.18 / 0.17 / 0.26 x 2^-24 of the mode itself - FLOAT32_HALF_ULP below
  y pass packing  256, 1024, 2048: the send buffer EQUALS the pack of the in-place result bit for bit, sentinels intact
  x plain         64: 0.83   128: 0.91   256: 0.94   512: 0.90   1024: 1.02   2048: 0.90     (impulses <= 0.39)
  x fused         256: 0.88   1024: 0.95   2048: 0.92                                          (impulses <= 0.28)
  whole mesh      64: 1.04   128: 1.15   256: 1.06 plain, 1.00 fused
  lattice         72: 1.01   98: 0.97   110: 1.11   130: 1.41   154: 1.08   182: 1.18   384: 0.65   512 (three-pass): 1.06
                  550: 0.43 compile-time plan, 0.45 runtime plan, 0.55 one against the other (l2 1.11)
                  768, six planes of kx: 0.32 compile-time plan, 0.30 runtime plan; one against the other on every mode 0.45 (l2 1.22)
                  1024 (three-pass), six planes of kx: 1.18
Wall time of the large cases on the GPU machine (16 host threads): 512 2.6 s, 550 4.6 s, 768 5.1 s, 1024 6.1 s - host-side
references and the spectra coming back (1.3 to 4.3 GB), not kernels; every other test of the module is below 1.2 s.
The device is as accurate as pocketfft in float32: but for that one checkerboard mode, which no float32 can hold to 4 rho, nothing
needed more than 1.5 of the 4.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.fft

import fft_statement as st

pytestmark = pytest.mark.gpu

POW2 = [64, 128, 256, 512, 1024, 2048]
FUSED = [256, 1024, 2048]
SENT_BYTE = 0x5A
SENT = np.uint32(0x5A5A5A5A)          # finite as a float (1.5e16), never produced by a transform of these inputs
WORKERS = 16
FACTOR = 4.0
# rho ||want|| is the share of one mode in an error that is spread over the plane, as it is for white noise and for the impulses.
# The checkerboard puts the whole plane into ONE mode, |want_k| = ||want|| = n^2; where the fused form multiplies that mode by
# an x twiddle that is not 1, no float32 can hold the product closer than half an ulp, 2^-24 |want_k| = 6e-8 ||want||, which is
# 20 (n = 256) to 115 (n = 2048) times rho ||want||: the bound of the white-noise case cannot be met by any float32 output.
# For the fused pairs that hold the checkerboard, mode k is therefore allowed 4 (rho ||want|| + 2^-24 |want_k|); every mode but
# (n/2, n/2) is zero there and keeps 4 rho ||want||, as does every other comparison of this module.  For the same reason the
# checkerboard has a pair to itself (the other plane is zero): its column kz = n/2 holds rows of +-n, and a second input added to
# them is rounded at ulp(n) in every row - an error that is correct float32 arithmetic, but confined to that one column, where it
# is sqrt(n/2) times the share rho ||want|| assumes (measured 7.9 rho at n = 256 with the impulses in the other plane).
FLOAT32_HALF_ULP = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------- yardstick
def _norm(a, axes):
    return np.sqrt((np.abs(a) ** 2).sum(axis=axes, keepdims=True))


class Ref:
    """expected output `want` (complex128) with the per-mode bound and the l2 bound that go with it"""

    def __init__(self, want, rho, l2, axes):
        self.want, self.rho, self.l2, self.axes = want, rho, l2, axes


def _yardstick(got32, want, axes):
    """(rho, l2) of a float32 CPU transform: max over the blocks (planes / columns) of max|err| / ||want|| and of ||err|| / ||want||"""
    assert got32.dtype == np.complex64 and want.dtype == np.complex128
    err = np.abs(got32 - want)
    nrm = _norm(want, axes)
    rho, l2 = float((err / nrm).max()), float((_norm(err, axes) / nrm).max())
    # a yardstick is only as good as the statement: scipy in float32 has to BE the statement up to float32 round-off, within
    # the worst-case bound of a float32 FFT of N points, log2(N) * 7 u (Higham, Accuracy and Stability of Numerical Algorithms,
    # thm 24.2; measured 1.1e-7 to 2.0e-7) - a statement that says something else than the transform would otherwise buy itself
    # a bound as wide as its own mistake
    points = np.prod([want.shape[a] for a in axes])
    assert l2 <= np.log2(2 * points) * 7 * 2.0 ** -24, f'the float64 statement is not what scipy computes in float32: relative l2 {l2:.3g}'
    return rho, l2


def _judge(label, got, ref, own=0.0):
    """got (complex64 from the device) against ref.want block by block: finite, every mode within 4 rho ||want||, relative l2
    within 4 x scipy-float32's.  own > 0 adds 4 own |want_k| to the bound of mode k: see FLOAT32_HALF_ULP"""
    want = ref.want
    assert got.shape == want.shape, (label, got.shape, want.shape)
    assert np.isfinite(got.view(np.float32)).all(), f'{label}: non-finite output (row padding leaked into a mode?)'
    err = np.abs(got - want)
    nrm = _norm(want, ref.axes)
    ratio = float((err / nrm).max() / ref.rho)
    if own > 0.0:
        print(f'RATIO {label}: max/rho {ratio:.3f} before the allowance for the rounding of the mode itself')
        ratio = float((err / (ref.rho * nrm + own * np.abs(want))).max())
    l2r = float((_norm(err, ref.axes) / nrm).max() / ref.l2)
    print(f'RATIO {label}: max/rho {ratio:.3f} l2/l2ref {l2r:.3f} (rho {ref.rho:.3e}, l2ref {ref.l2:.3e})')
    assert ratio <= FACTOR, f'{label}: worst mode at {ratio:.3g} rho (rho = {ref.rho:.3g} of the norm), allowed {FACTOR}'
    assert l2r <= FACTOR, f'{label}: relative l2 error {l2r:.3g} x scipy-float32 ({ref.l2:.3g}), allowed {FACTOR}'


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ------------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def _zy_inputs(n):
    """planes (4, n, n) float32: two of white noise, the impulses, the checkerboard; T: zy_plain of each (closed forms for the
    last two); yardstick from the noise planes"""
    rng = np.random.default_rng(1000 + n)
    P = np.zeros((4, n, n), dtype=np.float32)
    P[:2] = rng.standard_normal((2, n, n)).astype(np.float32)
    pts = [(1, 1, 1.0), (n - 1, n // 2 + 3, -0.5)]
    for y0, z0, w in pts:
        P[2, y0, z0] = w
    P[3] = (1 - 2 * (np.add.outer(np.arange(n), np.arange(n)) & 1)).astype(np.float32)
    T = np.zeros((4, n, n // 2 + 1), dtype=np.complex128)
    T[:2] = st.zy_plain(P[:2])
    T[2] = st.impulses_zy(n, pts)
    T[3, n // 2, n // 2] = float(n) * n
    T32 = scipy.fft.fft(scipy.fft.rfft(P[:2], axis=-1), axis=-2)
    rho, l2 = _yardstick(T32, T[:2], (1, 2))
    _frozen(P, T)
    return P, T, rho, l2


@functools.lru_cache(maxsize=None)
def _x_inputs(n):
    """(3, n, n/2 + 1) complex64: white noise rows, and one row of impulses at x = 1 (weight 1 + 0.5i) and x = n/2 + 1 (-0.5)"""
    rng = np.random.default_rng(2000 + n)
    kz = n // 2 + 1
    G = (rng.standard_normal((3, n, kz)) + 1j * rng.standard_normal((3, n, kz))).astype(np.complex64)
    I = np.zeros((1, n, kz), dtype=np.complex64)
    I[0, 1] = 1 + 0.5j
    I[0, n // 2 + 1] = -0.5
    k = np.arange(n)[:, None] * np.ones((1, kz))
    plain = (1 + 0.5j) * np.exp(-2j * np.pi * k / n) - 0.5 * np.exp(-2j * np.pi * ((k * (n // 2 + 1)) % n) / n)
    j = k[:n // 2]
    w = np.exp(-2j * np.pi * j / (n // 2))
    fused = np.concatenate([(1 + 0.5j) * w, -0.5 * w])
    _frozen(G, I, plain, fused)
    return G, I, plain[None], fused[None]


@functools.lru_cache(maxsize=None)
def _x_ref(n, form):
    G = _x_inputs(n)[0]
    if form == 'plain':
        want, got32 = st.x_plain(G), scipy.fft.fft(G, axis=1)
    else:
        H = n // 2
        want = st.x_fused(G)
        got32 = np.concatenate([scipy.fft.fft(G[:, :H], axis=1), scipy.fft.fft(G[:, H:], axis=1)], axis=1)
    # a column is the n (plain) or n/2 (fused) points of one transform
    wv, gv = (want, got32) if form == 'plain' else (want.reshape(6, n // 2, -1), got32.reshape(6, n // 2, -1))
    rho, l2 = _yardstick(gv, wv, (1,))
    _frozen(want)
    return want, rho, l2


# ------------------------------------------------------------------------------------------------------------- device side
def _backend():
    from abacusutils_amd.analysis import slab_power as sp
    return sp, sp.HipSlabBackend()


def _fill(buf, off=0, nfloat=None):
    from abacusutils_amd import _lib
    _lib.check(_lib.lib().abacus_memset(buf.ptr(off), SENT_BYTE, C.c_uint64(4 * (buf.n - off if nfloat is None else nfloat))))


def _real_planes(n, pitch, nplanes, fill):
    """host image (nplanes, n, pitch) float32: sentinel everywhere, then fill = {plane index: (n, n) reals} with NaN padding"""
    host = np.empty((nplanes, n, pitch), dtype=np.float32)
    host.view(np.uint32)[...] = SENT
    for i, p in fill.items():
        host[i, :, :n] = p
        host[i, :, n:] = np.nan
    return host


def _spectrum_of(plane_f32, n):
    """(n, pitch) float32 -> the n/2 + 1 valid complex columns"""
    return np.ascontiguousarray(plane_f32).view(np.complex64)[:, :n // 2 + 1]


def _run_zy(n, geometry, fill, nplanes):
    """upload, z + y passes in place, read everything back: (planes (nplanes, n, pitch) float32)"""
    sp, be = _backend()
    pitch = be.pitch(n)
    world, xsep, xg0, p0, pc = geometry
    mesh = sp.HipBuf(nplanes * n * pitch)
    try:
        mesh.set(0, _real_planes(n, pitch, nplanes, fill))
        be.fft_zy(mesh, 0, None, n, world, xsep, xg0, p0, pc)
        be.sync()
        return mesh.get(0, mesh.n).reshape(nplanes, n, pitch)
    finally:
        mesh.free()


def _untouched(out, planes, label):
    for i in planes:
        assert (out[i].view(np.uint32) == SENT).all(), f'{label}: plane {i} beside the transformed ones was written'


def _fused_on(n, options):
    from abacusutils_amd import _lib
    if n == 256:
        options.set('fft_fuse_small', 1)
    assert _lib.lib().abacus_slab_fused(n) == 1


# ----------------------------------------------------------------------------------------------- z + y passes, plain form
@pytest.mark.parametrize('n', POW2)
def test_zy_plain(n, options):
    """fft_z_r2c<n/2, B> + fft_cols<n, C> on planes 1 and 4 of five (world n/4: h = 2, halves 3 apart, pair 1 of 2)"""
    from abacusutils_amd import _lib
    options.set('slab_nofuse', 1)
    assert _lib.lib().abacus_slab_fused(n) == 0
    P, T, rho, l2 = _zy_inputs(n)
    geom = (n // 4, 3, 0, 1, 1)
    for name, a, b in (('noise', 0, 1), ('impulses|checkerboard', 2, 3)):
        out = _run_zy(n, geom, {1: P[a], 4: P[b]}, 5)
        _untouched(out, (0, 2, 3), f'zy plain {n} {name}')
        for plane, src in ((1, a), (4, b)):
            _judge(f'zy plain n={n} {name} plane {plane}', _spectrum_of(out[plane], n)[None], Ref(T[src][None], rho, l2, (1, 2)))


# ----------------------------------------------------------------------------------------------- z + y passes, fused form
@pytest.mark.parametrize('geometry', ['contiguous', 'apart'])
@pytest.mark.parametrize('n', FUSED)
def test_zy_fused(n, geometry, options):
    """fft_z_r2c<n/2, 4, FUSE> + fft_cols<n/2, 16>: the stored pair is the sum and the twiddled difference, rows in the order f.
    contiguous: halves back to back (xsep = pc = 2, p0 = 0: the one-launch branch of fft3d_fused_zy_slab), global planes 0, 1;
    apart: pair 1 of a slab whose halves lie 3 planes apart and whose first plane is global plane 6 - the x twiddle is that of
    plane 7, which only a non-zero xg0 can show"""
    _fused_on(n, options)
    P, T, rho, l2 = _zy_inputs(n)
    if geometry == 'contiguous':
        geom, pairs, idle = (n // 4, 2, 0, 0, 2), [(0, 2, 0), (1, 3, 1)], (4,)       # (first plane, second plane, global x)
    else:
        geom, pairs, idle = (n // 4, 3, 6, 1, 1), [(1, 4, 7)], (0, 2, 3)
    Z = np.zeros((n, n), dtype=np.float32), np.zeros((n, n // 2 + 1), dtype=np.complex128)
    plane = lambda i: (Z[0], Z[1]) if i is None else (P[i], T[i])   # noqa: E731
    for name, srcs in (('noise', [(0, 1), (1, 0)]), ('impulses', [(2, None), (None, 2)]), ('checkerboard', [(3, None), (None, 3)])):
        fill = {}
        for (i0, i1, _), (a, b) in zip(pairs, srcs):
            fill[i0], fill[i1] = plane(a)[0], plane(b)[0]
        out = _run_zy(n, geom, fill, 5)
        _untouched(out, idle, f'zy fused {n} {geometry} {name}')
        for (i0, i1, xg), (a, b) in zip(pairs, srcs):
            w0, w1 = st.fuse_pair(plane(a)[1], plane(b)[1], xg, n)
            if name == 'noise':     # the statement from the planes themselves
                v0, v1 = st.zy_fused(P[a], P[b], xg, n)
                assert np.array_equal(v0, w0) and np.array_equal(v1, w1)
            own = FLOAT32_HALF_ULP if name == 'checkerboard' else 0.0
            _judge(f'zy fused n={n} {geometry} {name} sum plane {i0}', _spectrum_of(out[i0], n)[None], Ref(w0[None], rho, l2, (1, 2)), own)
            _judge(f'zy fused n={n} {geometry} {name} difference plane {i1}', _spectrum_of(out[i1], n)[None], Ref(w1[None], rho, l2, (1, 2)), own)


# ------------------------------------------------------------------------------ y pass that writes the transpose buffer
@pytest.mark.parametrize('n,world', [(256, 4), (1024, 8), (2048, 16)])
def test_zy_fused_packed(n, world, options):
    """fft_cols<n/2, 16, false, PACK>: the y pass writes send[q][s h + p][yl][:] itself.  Pairs 3 and 4 of the rank's h; the
    slices must equal the restated pack of the in-place result of the same input (verified per mode by test_zy_fused; the
    in-place and the packing instantiation run the same transform, so BIT equality is asked), abacus_slab_pack_dev of the in-place
    buffer is a second comparator, and every other element of the send buffer keeps its sentinel: at n = 256 all of it is read
    back, above that the blocks on both sides of every written one and a strided sample of the rest (2.1 GB at 2048).  The mesh planes on both sides
    of the owned pairs hold the sentinel too and must keep it in either run."""
    from abacusutils_amd import _lib
    _fused_on(n, options)
    sp, be = _backend()
    pitch = be.pitch(n)
    h, nyl = n // (2 * world), n // world
    xsep, p0, pc, xg0 = h + 1, 3, 2, 5
    rng = np.random.default_rng(3000 + n)
    P = rng.standard_normal((2 * pc, n, n)).astype(np.float32)
    owned = [s * xsep + p for s in range(2) for p in range(p0, p0 + pc)]
    host = _real_planes(n, pitch, pc, {})          # image of pc consecutive planes
    block = nyl * pitch                            # floats of one (peer, plane) block of the send buffer
    mesh, send = sp.HipBuf((xsep + h) * n * pitch), sp.HipBuf(2 * h * n * pitch)

    beside = [s * xsep + p for s in range(2) for p in (p0 - 1, p0 + pc)]   # the mesh planes on both sides of the owned ones

    def mesh_beside_untouched(what):
        for i in beside:
            assert (mesh.get(i * n * pitch, n * pitch).view(np.uint32) == SENT).all(), f'{what}: mesh plane {i} beside the owned pairs was written'

    def upload():
        for i in beside:
            _fill(mesh, i * n * pitch, n * pitch)
        for s in range(2):
            img = host.copy()
            img[:, :, :n] = P[s * pc:(s + 1) * pc]
            img[:, :, n:] = np.nan
            mesh.set((s * xsep + p0) * n * pitch, img)

    def slices():
        """the written blocks with one block on either side, per (peer, half): (world, 2, pc + 2, nyl, pitch) as uint32"""
        got = np.empty((world, 2, pc + 2, nyl, pitch), dtype=np.uint32)
        for q in range(world):
            for s in range(2):
                got[q, s] = send.get(((q * 2 * h) + s * h + p0 - 1) * block, (pc + 2) * block).view(np.uint32).reshape(pc + 2, nyl, pitch)
        return got

    try:
        upload()
        be.fft_zy(mesh, 0, None, n, world, xsep, xg0, p0, pc)
        be.sync()
        inplace = np.stack([mesh.get(i * n * pitch, n * pitch).reshape(n, pitch) for i in owned])   # (s, p) order
        mesh_beside_untouched('in place')
        assert np.isfinite(inplace.view(np.complex64)[:, :, :n // 2 + 1].view(np.float32)).all()
        # the restated pack of the in-place result, laid out like slices()
        data = np.zeros((xsep + h, n, pitch), dtype=np.float32) if n == 256 else None
        want = np.empty((world, 2, pc, nyl, pitch), dtype=np.uint32)
        for q in range(world):
            for s in range(2):
                for u in range(pc):
                    want[q, s, u] = inplace[s * pc + u, q * nyl:(q + 1) * nyl].view(np.uint32)
        if data is not None:                      # ... and through st.pack on the whole buffer where that is small
            for i, pl in zip(owned, inplace):
                data[i] = pl
            full = np.empty((world, 2 * h, nyl, pitch), dtype=np.float32)
            full.view(np.uint32)[...] = SENT
            st.pack(data, full, world, h, xsep, p0, pc)
            assert np.array_equal(full.view(np.uint32)[:, [s * h + p0 + u for s in range(2) for u in range(pc)]].reshape(world, 2, pc, nyl, pitch), want)

        # second comparator first (it reads the in-place buffer): the device's own pack pass
        _fill(send)
        be.pack(mesh, 0, send, n, world, xsep, p0, pc)
        be.sync()
        got = slices()
        assert np.array_equal(got[:, :, 1:1 + pc], want), 'abacus_slab_pack_dev differs from the restated pack'
        assert (got[:, :, [0, pc + 1]] == SENT).all()

        # the y pass that packs
        _fill(send)
        upload()
        _lib.profile_reset()
        _lib.profile_enable(True)
        be.fft_zy(mesh, 0, send, n, world, xsep, xg0, p0, pc)
        be.sync()
        _lib.profile_enable(False)
        prof = _lib.profile_get()
        assert 'fft_cols_y' in prof and 'slab_pack' not in prof, sorted(prof)
        mesh_beside_untouched('packing y pass')
        got = slices()
        cols = slice(0, 2 * (n // 2 + 1))          # floats of the valid columns
        differ = int((got[:, :, 1:1 + pc, :, cols] != want[..., cols]).sum())
        print(f'RATIO zy packed n={n}: {differ} of {want[..., cols].size} valid floats differ in their bits from the in-place result')
        assert differ == 0
        assert np.array_equal(got[:, :, 1:1 + pc], want), 'padding columns differ from the in-place result'
        assert (got[:, :, [0, pc + 1]] == SENT).all(), 'a block beside the written ones lost its sentinel'
        written = {q * 2 * h + s * h + p0 + u for q in range(world) for s in range(2) for u in range(pc)}
        nblock = world * 2 * h
        if n == 256:
            sample = range(nblock)
        else:
            sample = sorted(set(np.linspace(0, nblock - 1, 61).astype(int)) | {0, nblock - 1})
        for b in sample:
            if b not in written:
                assert (send.get(b * block, block).view(np.uint32) == SENT).all(), f'block {b} of the send buffer lost its sentinel'
    finally:
        mesh.free()
        send.free()


# ---------------------------------------------------------------------------------------------------------------- x pass
def _run_x(n, G):
    """G (nyl, n, n/2 + 1) complex64 on the layout (y_local, x, pitch / 2) with NaN padding columns -> the same after fft_x"""
    sp, be = _backend()
    pitch = be.pitch(n)
    nyl, kz = G.shape[0], n // 2 + 1
    host = np.full((nyl, n, pitch // 2), np.nan + 1j * np.nan, dtype=np.complex64)
    host[:, :, :kz] = G
    buf = sp.HipBuf(nyl * n * pitch)
    try:
        buf.set(0, host.view(np.float32))
        be.fft_x(buf, 0, n, nyl)
        be.sync()
        return np.ascontiguousarray(buf.get(0, buf.n).view(np.complex64).reshape(nyl, n, pitch // 2)[:, :, :kz])
    finally:
        buf.free()


@pytest.mark.parametrize('nyl', [1, 3])
@pytest.mark.parametrize('n', POW2)
def test_x_plain(n, nyl, options):
    """fft_cols<n, C> along x (element stride: a whole row of pitch / 2) over all n/2 + 1 columns of 1 and 3 y-rows"""
    from abacusutils_amd import _lib
    options.set('slab_nofuse', 1)
    assert _lib.lib().abacus_slab_fused(n) == 0
    G, I, iplain, _ = _x_inputs(n)
    want, rho, l2 = _x_ref(n, 'plain')
    _judge(f'x plain n={n} nyl={nyl} noise', _run_x(n, G[:nyl]), Ref(want[:nyl], rho, l2, (1,)))
    Gi = np.concatenate([I] * nyl)
    _judge(f'x plain n={n} nyl={nyl} impulses', _run_x(n, Gi), Ref(np.concatenate([iplain] * nyl), rho, l2, (1,)))


@pytest.mark.parametrize('n', FUSED)
def test_x_fused(n, options):
    """fft_cols<n/2, 16>: two independent n/2-point transforms over rows [0, n/2) and [n/2, n) of each of 2 y-rows"""
    _fused_on(n, options)
    G, I, _, ifused = _x_inputs(n)
    want, rho, l2 = _x_ref(n, 'fused')
    H = n // 2
    halves = lambda a: np.ascontiguousarray(a).reshape(a.shape[0] * 2, H, -1)   # noqa: E731  (a block = one n/2-point transform)
    _judge(f'x fused n={n} noise', halves(_run_x(n, G[:2])), Ref(halves(want[:2]), rho, l2, (1,)))
    Gi = np.concatenate([I, I])
    _judge(f'x fused n={n} impulses', halves(_run_x(n, Gi)), Ref(halves(np.concatenate([ifused, ifused])), rho, l2, (1,)))


# ------------------------------------------------------------------------------------------- whole small meshes, one rank
@functools.lru_cache(maxsize=None)
def _mesh_ref(n):
    a = np.random.default_rng(4000 + n).standard_normal((n, n, n)).astype(np.float32)
    want = scipy.fft.rfftn(a.astype(np.float64), workers=WORKERS)
    rho, l2 = _yardstick(scipy.fft.rfftn(a, workers=WORKERS)[None], want[None], (1, 2, 3))
    _frozen(a, want)
    return a, want, rho, l2


@pytest.mark.parametrize('n,form', [(64, 'plain'), (128, 'plain'), (256, 'plain'), (256, 'fused')])
def test_whole_mesh(n, form, options):
    """fft_zy over all n/2 pairs, device pack + unpack, fft_x over all y: every mode of np.fft.rfftn of a white-noise mesh - in
    the fused form permuted by f on both axes.  Ties the statements of the passes to the transform the binning believes it reads."""
    from abacusutils_amd import _lib
    if form == 'fused':
        _fused_on(n, options)
    else:
        options.set('slab_nofuse', 1)
        assert _lib.lib().abacus_slab_fused(n) == 0
    a, want, rho, l2 = _mesh_ref(n)
    sp, be = _backend()
    pitch, H = be.pitch(n), n // 2
    mesh, send = sp.HipBuf(n * n * pitch), sp.HipBuf(n * n * pitch)
    try:
        mesh.set(0, _real_planes(n, pitch, n, {i: a[i] for i in range(n)}))
        be.fft_zy(mesh, 0, None, n, 1, H, 0, 0, H)
        be.pack(mesh, 0, send, n, 1, H, 0, H)
        be.unpack(send, mesh, 0, n, 1)
        be.fft_x(mesh, 0, n, n)
        be.sync()
        got = mesh.get(0, mesh.n).view(np.complex64).reshape(n, n, pitch // 2)[:, :, :H + 1].transpose(1, 0, 2)   # (y, x, k) -> (x, y, k)
    finally:
        mesh.free()
        send.free()
    if form == 'fused':
        f = st.perm(n)
        want = want[f][:, f]
    _judge(f'whole mesh n={n} {form}', np.ascontiguousarray(got)[None], Ref(want[None], rho, l2, (1, 2, 3)))


# ------------------------------------------------------------------------- exact lattice deposit: get_field / get_field_fft
def _lattice_pos(n):
    """n^3 / 8 uniformly drawn integer cell centres of a box L = n (repeats allowed), as int32 cells"""
    return np.random.default_rng(5000 + n).integers(0, n, size=(n ** 3 // 8, 3), dtype=np.int32)


@functools.lru_cache(maxsize=1)
def _lattice(n):
    """unweighted particles on integer cell centres: every TSC weight is a product of 0.75 and 0.125, every cell sum an exact
    dyadic number whatever the order of the additions, norm = 8 exactly.
    Returns (positions float32, the overdensity mesh rho 8 - 1 as float32, exact)"""
    cells = _lattice_pos(n)
    flat = (cells[:, 0].astype(np.int64) * n + cells[:, 1]) * n + cells[:, 2]
    c = np.bincount(flat, minlength=n ** 3).astype(np.float32).reshape(n, n, n)      # small integers: exact
    del flat
    for ax in range(3):                                                              # separable 3-point cloud, exact in float32:
        s = np.roll(c, 1, axis=ax)                                                   # multiples of 2^-9 below 2^7
        s += np.roll(c, -1, axis=ax)
        s *= np.float32(0.125)
        c *= np.float32(0.75)
        c += s
    del s
    assert c.max() < 128.0
    c *= np.float32(8.0)
    c -= np.float32(1.0)
    pos = cells.astype(np.float32)
    _frozen(pos, c)
    return pos, c


def _lattice_fft(n, pos=None, native='gfft_'):
    from abacusutils_amd import _lib
    from abacusutils_amd.analysis.power_spectrum import get_field_fft
    pos = _lattice(n)[0] if pos is None else pos
    _lib.profile_reset()
    _lib.profile_enable(True)
    got = get_field_fft(pos.copy(), float(n), n, 'TSC', None, None, False, False)
    _lib.profile_enable(False)
    prof = _lib.profile_get()
    assert any(k.startswith(native) for k in prof) and 'hipfft_r2c' not in prof, sorted(prof)
    return got


def _mesh_fft_ref(mesh, n):
    """get_field_fft's convention (rfftn / n^3) of the exact mesh in float64 through scipy, with scipy's float32 rfftn of the
    same mesh as the yardstick"""
    want = scipy.fft.rfftn(mesh.astype(np.float64), workers=WORKERS)
    want *= 1.0 / float(n) ** 3
    w32 = scipy.fft.rfftn(mesh, workers=WORKERS)
    w32 *= np.float32(1.0 / float(n) ** 3)
    rho, l2 = _yardstick(w32[None], want[None], (1, 2, 3))
    return Ref(want[None], rho, l2, (1, 2, 3))


# 768^3 and 1024^3: neither the NumPy mesh (14 s and 31 s measured for bincount + the separable cloud) nor a float64 rfftn (4.0 s at
# 768^3 alone) fits a test, so (1) the mesh is the device's own (get_field), asserted EQUAL to the NumPy lattice mesh on two whole
# planes, and (2) the float64 reference is restricted to six planes of kx - the corners of the x transform: 0, 1, n/2 - 1, n/2,
# n/2 + 1, n - 1 -: zy_plain of every plane, then those outputs of x_plain as a 6 x n matrix product.  The yardstick is scipy's
# float32 rfftn of the same mesh on the same six planes, per plane as for the passes (error over the Frobenius norm of the plane).
def _kx_corners(n):
    return [0, 1, n // 2 - 1, n // 2, n // 2 + 1, n - 1]


def _lattice_planes(cells, n, xs):
    """the exact lattice mesh (see _lattice) on the planes xs only: (len(xs), n, n) float32"""
    out = []
    for x in xs:
        c = np.zeros((n, n), dtype=np.float32)
        for dx, wx in ((-1, 0.125), (0, 0.75), (1, 0.125)):
            sel = cells[cells[:, 0] == (x + dx) % n]
            c += np.float32(wx) * np.bincount(sel[:, 1].astype(np.int64) * n + sel[:, 2], minlength=n * n).astype(np.float32).reshape(n, n)
        for ax in range(2):
            c = np.float32(0.75) * c + np.float32(0.125) * (np.roll(c, 1, axis=ax) + np.roll(c, -1, axis=ax))
        out.append(c * np.float32(8.0) - np.float32(1.0))
    return np.stack(out)


def _device_lattice_mesh(n):
    """(positions float32, the device's mesh of them) - the mesh asserted exact on planes 0 and n/2 + 1"""
    from abacusutils_amd.analysis.power_spectrum import get_field
    cells = _lattice_pos(n)
    pos = cells.astype(np.float32)
    mesh = get_field(pos.copy(), float(n), n, 'TSC')
    xs = [0, n // 2 + 1]
    assert np.array_equal(mesh[xs], _lattice_planes(cells, n, xs)), 'the deposit of lattice particles is not exact'
    return pos, mesh


def _kx_planes_ref(mesh, n):
    """Ref of the planes kx = _kx_corners(n) of rfftn(mesh) / n^3: zy_plain of every plane (scipy in float64, 64 planes at a time;
    the first plane checked against the NumPy statement), then the six outputs of x_plain"""
    KX = _kx_corners(n)
    Wm = np.exp(-2j * np.pi * (np.outer(KX, np.arange(n)) % n) / n)
    want = np.zeros((len(KX), n, n // 2 + 1), dtype=np.complex128)
    for x0 in range(0, n, 64):
        T = scipy.fft.fft(scipy.fft.rfft(mesh[x0:x0 + 64].astype(np.float64), axis=-1, workers=WORKERS), axis=-2, workers=WORKERS)
        if x0 == 0:
            assert np.abs(T[0] - st.zy_plain(mesh[0])).max() <= 1e-12 * np.abs(T[0]).max()
        want += np.tensordot(Wm[:, x0:x0 + 64], T, 1)
    want *= 1.0 / float(n) ** 3
    w32 = np.ascontiguousarray(scipy.fft.rfftn(mesh, workers=WORKERS)[KX])
    w32 *= np.float32(1.0 / float(n) ** 3)
    rho, l2 = _yardstick(w32, want, (1, 2))
    return Ref(want, rho, l2, (1, 2))


@pytest.mark.parametrize('n', [72, 98, 110, 130, 154, 182, 384])
def test_mixed_radix_lattice(n):
    """every radix of gfft.hip (2, 3, 4, 5, 7, 8, 11, 13) in the n-point and in the n/2-point plan: 72 = 2^3 3^2 (36), 98 = 2 7^2
    (49), 110 = 2 5 11 (55), 130 = 2 5 13 (65), 154 = 2 7 11 (77), 182 = 2 7 13 (91), 384 = 2^7 3 (192, a compile-time plan)"""
    from abacusutils_amd.analysis.power_spectrum import get_field
    pos, mesh = _lattice(n)
    assert np.array_equal(get_field(pos.copy(), float(n), n, 'TSC'), mesh), 'the deposit of lattice particles is not exact'
    _judge(f'lattice n={n} mixed radix', _lattice_fft(n)[None], _mesh_fft_ref(mesh, n))


def _judge_pair(label, a, b, rho, l2):
    """two float32 spectra of the same mesh against each other, every mode, plane by plane of kx: within 4 rho of the plane's
    Frobenius norm and 4 x the relative l2 error - the bound each has against the truth, not the sum of the two"""
    n = a.shape[0]
    worst = worst2 = 0.0
    for i in range(0, n, 64):                      # in slabs: a spectrum is up to 1.8 GB
        x = a[i:i + 64].astype(np.complex128)
        d = np.abs(x - b[i:i + 64])
        nrm = np.sqrt((np.abs(x) ** 2).sum(axis=(1, 2)))
        worst = max(worst, float((d.max(axis=(1, 2)) / nrm).max()))
        worst2 = max(worst2, float((np.sqrt((d ** 2).sum(axis=(1, 2))) / nrm).max()))
    differ = int((a.view(np.uint32) != b.view(np.uint32)).sum())
    print(f'RATIO {label}: {differ} of {a.size * 2} floats differ in their bits; max/rho {worst / rho:.3f} l2/l2ref {worst2 / l2:.3f} '
          f'(rho {rho:.3e}, l2ref {l2:.3e})')
    assert worst <= FACTOR * rho, f'{label}: worst mode {worst / rho:.3g} rho apart'
    assert worst2 <= FACTOR * l2, f'{label}: {worst2 / l2:.3g} x the relative l2 error of scipy-float32 apart'


def test_mixed_radix_550_fixed_runtime_scipy(options):
    """compute_power's default mesh: the compile-time plan (GFixed<550>, GFixed<275>) and the runtime plan (gfft_nofixed), each
    per mode against scipy's float64 rfftn (1.3 GB on the host), and against each other within the same 4 rho ||F||"""
    n = 550
    pos, mesh = _lattice(n)
    fixed = _lattice_fft(n)
    options.set('gfft_nofixed', 1)
    runtime = _lattice_fft(n)
    options.set('gfft_nofixed', 0)
    ref = _mesh_fft_ref(mesh, n)
    _judge(f'lattice n={n} fixed plan', fixed[None], ref)
    _judge(f'lattice n={n} runtime plan', runtime[None], ref)
    d = np.abs(fixed - runtime)
    nrm = float(_norm(ref.want, ref.axes).max())
    differ = int((fixed.view(np.uint32) != runtime.view(np.uint32)).sum())
    print(f'RATIO lattice n={n} fixed vs runtime plan: {differ} of {fixed.size * 2} floats differ in their bits; max/rho '
          f'{d.max() / nrm / ref.rho:.3f} l2/l2ref {np.sqrt((d.astype(np.float64) ** 2).sum()) / nrm / ref.l2:.3f}')
    assert d.max() <= FACTOR * ref.rho * nrm
    assert np.sqrt((d.astype(np.float64) ** 2).sum()) <= FACTOR * ref.l2 * nrm


def test_mixed_radix_768_fixed_runtime(options):
    """GFixed<768> / GFixed<384> and the runtime plan: each against the float64 reference on the six corner planes of kx, and
    against each other on EVERY mode, plane by plane, with the yardstick scipy's float32 rfftn shows at 768 itself on those six
    planes.  The two plans run the same stages in the same order, yet their results differ in the last bits: the compiler
    contracts differently once the strides are constants.  1536 is left out: 14.5 GB of spectrum to bring back."""
    n = 768
    pos, mesh = _device_lattice_mesh(n)
    ref = _kx_planes_ref(mesh, n)
    del mesh
    fixed = _lattice_fft(n, pos)
    options.set('gfft_nofixed', 1)
    runtime = _lattice_fft(n, pos)
    options.set('gfft_nofixed', 0)
    KX = _kx_corners(n)
    _judge(f'lattice n={n} fixed plan, six planes of kx', np.ascontiguousarray(fixed[KX]), ref)
    _judge(f'lattice n={n} runtime plan, six planes of kx', np.ascontiguousarray(runtime[KX]), ref)
    _judge_pair(f'lattice n={n} fixed vs runtime plan', fixed, runtime, ref.rho, ref.l2)


def test_pow2_512_lattice():
    """the plain three-pass form (get_field_fft never takes the fused one) end to end at a production row length"""
    n = 512
    pos, mesh = _lattice(n)
    _judge(f'lattice n={n} three-pass', _lattice_fft(n, native='fft_z_r2c')[None], _mesh_fft_ref(mesh, n))


def test_pow2_1024_lattice_six_planes():
    """... and at 1024, where the whole float64 transform does not fit: the planes kx = 0, 1, 511, 512, 513, 1023 of the device's
    spectrum, sliced before anything is converted, against zy_plain of every plane + those six outputs of x_plain"""
    n = 1024
    pos, mesh = _device_lattice_mesh(n)
    ref = _kx_planes_ref(mesh, n)
    del mesh
    got = np.ascontiguousarray(_lattice_fft(n, pos, native='fft_z_r2c')[_kx_corners(n)])
    _judge(f'lattice n={n} three-pass, six planes of kx', got, ref)
