"""The float64 statements of the transform's passes (tests/fft_statement.py) against np.fft.rfftn, and the index rule of the
pencil transpose as a round trip: what tests/test_fft_passes_gpu.py judges the kernels by is itself pinned here, on the CPU."""
import numpy as np
import pytest

import fft_statement as st

TOL = 1e-12   # of the largest mode: float64 transforms of n <= 64 agree to ~1e-15 of it


def _mesh(n, seed=0):
    return np.random.default_rng(seed).standard_normal((n, n, n))


def _close(a, b):
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= TOL * np.abs(b).max()


def test_perm_is_the_first_dif_stage_order():
    for n in (16, 64):
        f = st.perm(n)
        assert sorted(f) == list(range(n))
        assert list(f[:n // 2]) == list(range(0, n, 2)) and list(f[n // 2:]) == list(range(1, n, 2))


@pytest.mark.parametrize('n', [16, 64])
def test_plain_passes_are_rfftn(n):
    a = _mesh(n)
    zy = st.zy_plain(a)                                   # (x, ky, kz)
    full = st.x_plain(zy.transpose(1, 0, 2)).transpose(1, 0, 2)
    _close(full, np.fft.rfftn(a))


@pytest.mark.parametrize('n', [16, 64])
def test_fused_passes_are_rfftn_permuted_on_both_axes(n):
    a = _mesh(n, 1)
    H = n // 2
    S = np.empty((n, n, H + 1), dtype=np.complex128)
    for xg in range(H):
        S[xg], S[xg + H] = st.zy_fused(a[xg], a[xg + H], xg, n)
    full = st.x_fused(S.transpose(1, 0, 2)).transpose(1, 0, 2)
    f = st.perm(n)
    _close(full, np.fft.rfftn(a)[f][:, f])


def test_fused_pair_depends_on_the_global_plane():
    """the x twiddle is exp(-2 pi i xg / n) of the GLOBAL plane: a pair stored elsewhere in a buffer keeps it"""
    n = 16
    a = _mesh(n, 2)
    s0, d0 = st.zy_fused(a[0], a[1], 0, n)
    s7, d7 = st.zy_fused(a[0], a[1], 7, n)
    assert np.array_equal(s0, s7)
    _close(d7, d0 * np.exp(-2j * np.pi * 7 / n))


def test_impulse_closed_form():
    n = 16
    pts = [(1, 1, 1.0), (n - 1, n // 2 + 3, -0.5)]
    p = np.zeros((n, n))
    for y0, z0, w in pts:
        p[y0, z0] = w
    _close(st.impulses_zy(n, pts), st.zy_plain(p))
    yz = np.add.outer(np.arange(n), np.arange(n))
    cb = st.zy_plain((-1.0) ** yz)
    want = np.zeros_like(cb)
    want[n // 2, n // 2] = n * n
    assert np.abs(cb - want).max() <= TOL * n * n


@pytest.mark.parametrize('n,world,ghost', [(16, 1, 0), (16, 2, 0), (16, 4, 3), (64, 8, 1)])
def test_pack_unpack_round_trip(n, world, ghost):
    """every rank packs its folded slab (pairs in two chunks), the all-to-all swaps the peer blocks, unpack leaves (y_local, x, k)
    with x in global order: together the transposition of the mesh"""
    cols = 5
    h, nyl = n // (2 * world), n // world
    xsep = h + ghost
    g = np.random.default_rng(3).standard_normal((n, n, cols))
    sends = []
    for r in range(world):
        data = np.full((xsep + h, n, cols), np.nan)
        data[:h] = g[r * h:(r + 1) * h]
        data[xsep:xsep + h] = g[n // 2 + r * h:n // 2 + (r + 1) * h]
        send = np.full((world, 2 * h, nyl, cols), np.nan)
        cut = max(h // 2, 1)
        st.pack(data, send, world, h, xsep, 0, cut)
        if cut < h:
            st.pack(data, send, world, h, xsep, cut, h - cut)
        sends.append(send)
    for r in range(world):
        recv = np.stack([sends[q][r] for q in range(world)])
        out = st.unpack(recv, n)
        assert np.array_equal(out, g[:, r * nyl:(r + 1) * nyl].transpose(1, 0, 2))
