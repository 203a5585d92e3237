#!/usr/bin/env python
"""Writes tests/golden/shear_cases.npz: the REFERENCE's own smooth_density, get_tidal, get_shear and tsc_parallel
(abacusnbody/analysis/shear.py, tsc.py), run under the identity Numba shim of oracle/shim, on small seeded inputs.

    python scripts/make_shear_golden.py /path/to/abacusutils

Needs the reference checkout, NumPy >= 2 and SciPy; no GPU.  Per shear / tidal case the file also holds `e_ref`, the largest
difference between the reference's float32 result and a float64 restatement of the same formulas, relative to the largest value
of the reference: the float32 noise of the reference itself, from which the GPU tests derive their bound (4 e_ref).
"""
import contextlib
import io
import sys
import types
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / 'oracle' / 'shim'))
sys.path.insert(0, str(REPO))
MINI = REPO / 'tests' / 'golden' / 'Mini_N64_L32' / 'Mini_N64_L32' / 'halos' / 'z0.000'


def import_reference(ref):
    """abacusnbody/__init__.py imports a generated version.py that a checkout does not have: register a bare package"""
    pkg = types.ModuleType('abacusnbody')
    pkg.__path__ = [str(Path(ref) / 'abacusnbody')]
    sys.modules['abacusnbody'] = pkg
    data = types.ModuleType('abacusnbody.data')      # (its __init__ wants astropy.utils; bitpacked.py itself does not)
    data.__path__ = [str(Path(ref) / 'abacusnbody' / 'data')]
    sys.modules['abacusnbody.data'] = data
    import abacusnbody.analysis.shear as S
    import abacusnbody.analysis.tsc as T
    import abacusnbody.data.bitpacked as B
    return S, T, B


def quiet(f, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return f(*a, **k)


def wavenumbers(N, Lbox):
    return np.fft.fftfreq(N, d=Lbox / (2 * np.pi * N)).astype(np.float32)


def tidal64(d, N, Lbox, R):
    """float64 restatement of rfftn + get_tidal: the six full components, (N, N, N/2+1, 6) complex128"""
    import scipy.fft as sf
    df = sf.rfftn(d.astype(np.float64))
    k = wavenumbers(N, Lbox).astype(np.float64)
    ka, kb, kc = k[:, None, None], k[None, :, None], k[None, None, :N // 2 + 1]
    idx = np.arange(N)
    mask = (idx[:, None, None] * idx[None, :, None] * idx[None, None, :N // 2 + 1]) != 0
    ksq = ka ** 2 + kb ** 2 + kc ** 2
    dok2 = np.where(mask, df / np.where(mask, ksq, 1.0), 0.0)
    if R is not None:
        x = np.sqrt(np.where(mask, ksq, 1.0)) * R
        dok2 = dok2 * (3 * (np.sin(x) - x * np.cos(x)) / x ** 3)
    return np.stack([ka * ka * dok2, ka * kb * dok2, ka * kc * dok2, kb * kb * dok2, kb * kc * dok2, kc * kc * dok2], axis=-1)


def shear64(d, N, Lbox, R):
    """float64 restatement of get_shear"""
    import scipy.fft as sf
    t = sf.irfftn(tidal64(d, N, Lbox, R), s=(N, N, N), axes=(0, 1, 2))
    tr2 = t[..., 0] ** 2 + t[..., 3] ** 2 + t[..., 5] ** 2 + 2 * (t[..., 1] ** 2 + t[..., 2] ** 2 + t[..., 4] ** 2)
    tr = t[..., 0] + t[..., 3] + t[..., 5]
    return np.sqrt(np.maximum(0.5 * (3 * tr2 - tr ** 2), 0))


def mini_positions(B):
    """pos of every field_rv_A and halo_rv_A file of the Mini_N64_L32 fixtures, in that order, files sorted by name"""
    from abacusutils_amd.data.asdf import AsdfFile
    out, Lbox = [], None
    for kind in ('field_rv_A', 'halo_rv_A'):
        for fn in sorted((MINI / kind).glob('*.asdf')):
            af = AsdfFile(str(fn))
            header = af.tree['header']
            Lbox = float(header['BoxSizeHMpc'])
            pos, _ = B.unpack_rvint(af.array('rvint'), header['BoxSize'], float_dtype=np.float32, velout=False)
            out.append(np.asarray(pos, dtype=np.float32))
    return np.concatenate(out), Lbox


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    assert int(np.__version__.split('.')[0]) >= 2, 'golden vectors are generated under NumPy >= 2'
    S, T, B = import_reference(sys.argv[1])
    import scipy.fft as sf
    G = {}
    Lbox = 50.0

    # ---- smoothing: non-negative inputs; sigma 0.5, 1.0, 2.3 cells (radii 2, 4, 9) and one radius beyond the mesh
    rng = np.random.default_rng(16)
    poisson16 = rng.poisson(3.0, size=(16, 16, 16)).astype(np.float32)
    rng = np.random.default_rng(12)
    poisson12 = rng.poisson(3.0, size=(12, 12, 12)).astype(np.float32)
    smooth_cases = [('p16_s0.5', poisson16, 0.5), ('p16_s1.0', poisson16, 1.0), ('p16_s2.3', poisson16, 2.3), ('p12_s3.5', poisson12, 3.5)]
    for name, D, sigma in smooth_cases:
        N = len(D)
        R = sigma * (Lbox / N)
        G[f'smooth/{name}/D'] = D
        G[f'smooth/{name}/R'] = np.float64(R)
        G[f'smooth/{name}/Lbox'] = np.float64(Lbox)
        G[f'smooth/{name}/radius'] = np.int64(int(4.0 * (R / (Lbox / N)) + 0.5))
        G[f'smooth/{name}/out'] = S.smooth_density(D.copy(), R, N, Lbox)
    G['smooth_names'] = np.array([c[0] for c in smooth_cases])

    # ---- shear: Poisson counts, a high-contrast lognormal field (exposes cancellation), a TSC deposit of real particles
    shear_cases = []
    shear_cases.append(('poisson16', S.smooth_density(poisson16.copy(), 1.0 * Lbox / 16, 16, Lbox), Lbox, None))
    for N in (24, 32):
        rng = np.random.default_rng(N)
        D = np.exp(2.0 * rng.standard_normal((N, N, N))).astype(np.float32)
        shear_cases.append((f'lognormal{N}', S.smooth_density(D, 2.0, N, Lbox), Lbox, None))
    shear_cases.append(('lognormal24_R3', shear_cases[1][1], Lbox, 3.0))
    pos, Lmini = mini_positions(B)
    G['mini/npart'] = np.int64(len(pos))
    G['mini/Lbox'] = np.float64(Lmini)
    G['mini/R'] = np.float64(1.5)
    dens = T.tsc_parallel(pos.copy(), 32, Lmini, nthread=1)
    dsmo_mini = S.smooth_density(dens, 1.5, 32, Lmini)
    shear_cases.append(('mini32', dsmo_mini, Lmini, None))
    for name, dsmo, L, R in shear_cases:
        N = len(dsmo)
        ref = quiet(S.get_shear, dsmo.copy(), N, L, R)
        assert ref.dtype == np.float32 and ref.shape == (N, N, N)
        G[f'shear/{name}/dsmo'] = dsmo.astype(np.float32)
        G[f'shear/{name}/Lbox'] = np.float64(L)
        G[f'shear/{name}/R'] = np.float64(-1.0 if R is None else R)
        G[f'shear/{name}/out'] = ref
        G[f'shear/{name}/e_ref'] = np.float64(np.abs(ref - shear64(dsmo, N, L, R)).max() / ref.max())
        print(f'shear {name}: N = {N}, max {ref.max():.4g}, e_ref {G[f"shear/{name}/e_ref"]:.3g}')
    G['shear_names'] = np.array([c[0] for c in shear_cases])

    # ---- get_tidal: the six full components
    tidal_cases = [('poisson16', shear_cases[0][1], Lbox, None), ('poisson16_R4', shear_cases[0][1], Lbox, 4.0)]
    for name, dsmo, L, R in tidal_cases:
        N = len(dsmo)
        dfour = sf.rfftn(dsmo.astype(np.float32))
        karr = wavenumbers(N, L)
        ref = S.get_tidal(dfour, karr, N, R)
        assert ref.dtype == np.complex64
        G[f'tidal/{name}/dfour'] = dfour
        G[f'tidal/{name}/karr'] = karr
        G[f'tidal/{name}/R'] = np.float64(-1.0 if R is None else R)
        G[f'tidal/{name}/out'] = ref
        G[f'tidal/{name}/e_ref'] = np.float64(np.abs(ref - tidal64(dsmo, N, L, R)).max() / np.abs(ref).max())
        print(f'tidal {name}: e_ref {G[f"tidal/{name}/e_ref"]:.3g}')
    G['tidal_names'] = np.array([c[0] for c in tidal_cases])

    out = REPO / 'tests' / 'golden' / 'shear_cases.npz'
    np.savez_compressed(out, **G)
    print(out, out.stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
