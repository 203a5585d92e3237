#!/usr/bin/env python
"""Writes tests/golden/zcv_cases.npz, zcv_fields_cases.npz and zcv_advect_cases.npz: the REFERENCE's own hod/zcv/ic_fields.py (gaussian_filter, get_fields, filter_field,
get_n2_fft, get_sij_fft, add_ij) and analysis/power_spectrum.py (get_field_fft, calc_pk_from_deltak) run under the identity Numba
shim of oracle/shim on small seeded inputs, following hod/zcv/advect_fields.py main :213-370 and tracer_power.py :155-273.

    python scripts/make_zcv_golden.py /path/to/abacusutils

Needs the reference checkout, NumPy >= 2 and SciPy; no GPU.  `asdf`, `classy` and `abacusnbody.metadata` are imported by the
reference modules at module level but not used by the functions called here: empty stand-ins are registered for them.

With every case the file holds `e_ref`: the largest difference between the reference's float32 result and a float64 evaluation
of the same formulas, relative to the largest value of the reference's array (binned spectra: relative to
max(|want|, 0.1 max|want|) element by element).  That is the float32 noise of the reference itself, from which the GPU tests
derive their bounds.
"""
import contextlib
import io
import sys
import types
import warnings
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / 'oracle' / 'shim'))

KEYNAMES = ['1cb', 'delta', 'delta2', 'tidal2', 'nabla2']
MODES = [('TSC', True, True), ('TSC', False, False), ('CIC', True, True), ('CIC', False, False)]
POLES = [0, 2, 4]
JVEC = [[0, 0], [0, 1], [0, 2], [1, 1], [1, 2], [2, 2]]


def mode_name(paste, compensated, interlaced):
    return f'{paste}_{"T" if compensated else "F"}{"T" if interlaced else "F"}'


def import_reference(ref):
    """abacusnbody/__init__.py imports a generated version.py that a checkout does not have: register a bare package, and empty
    stand-ins for the modules the zcv files import without using them here"""
    pkg = types.ModuleType('abacusnbody')
    pkg.__path__ = [str(Path(ref) / 'abacusnbody')]
    sys.modules['abacusnbody'] = pkg
    asdf = types.ModuleType('asdf')
    asdf_exc = types.ModuleType('asdf.exceptions')
    asdf_exc.AsdfWarning = type('AsdfWarning', (Warning,), {})
    asdf.exceptions = asdf_exc
    meta = types.ModuleType('abacusnbody.metadata')
    meta.get_meta = None
    classy = types.ModuleType('classy')
    classy.Class = None
    sys.modules.update({'asdf': asdf, 'asdf.exceptions': asdf_exc, 'abacusnbody.metadata': meta, 'classy': classy})
    import abacusnbody.analysis.power_spectrum as P
    import abacusnbody.hod.zcv.ic_fields as I
    import abacusnbody.hod.zcv.advect_fields as A  # noqa: F401  (imports must work: the recipe below follows its main)
    import abacusnbody.hod.zcv.tracer_power as T  # noqa: F401
    return I, P


def quiet(f, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return f(*a, **k)


def relmax(ref, f64):
    ref = np.asarray(ref)
    return np.float64(np.abs(ref.astype(np.complex128 if np.iscomplexobj(ref) else np.float64) - f64).max() / np.abs(ref).max())


def relbin(ref, f64):
    """binned spectra: element by element relative to max(|want|, 0.1 max|want|); NaN (empty bins) must match"""
    ref = np.asarray(ref, dtype=np.float64)
    f64 = np.asarray(f64, dtype=np.float64)
    assert np.array_equal(np.isnan(ref), np.isnan(f64))
    ok = ~np.isnan(ref)
    floor = 0.1 * np.abs(ref[ok]).max()
    return np.float64((np.abs(ref[ok] - f64[ok]) / np.maximum(np.abs(ref[ok]), floor)).max())


# ---- float64 evaluations of the reference's formulas ---------------------------------------------------------------------------
def kvec64(n, L):
    dk = 2.0 * np.pi / L
    idx = np.arange(n)
    kxy = np.where(idx < n // 2, idx, idx - n).astype(np.float64) * dk
    return kxy[:, None, None], kxy[None, :, None], (np.arange(n // 2 + 1) * dk)[None, None, :]


def filter64(field, n, L, kcut):
    import scipy.fft as sf
    kx, ky, kz = kvec64(n, L)
    fk = sf.rfftn(field.astype(np.float64))
    return sf.irfftn(np.exp(-(kx ** 2 + ky ** 2 + kz ** 2) / (2.0 * kcut ** 2)) * fk, s=(n, n, n))


def sij_factor64(i, j, n, L):
    kx, ky, kz = kvec64(n, L)
    k2 = kx ** 2 + ky ** 2 + kz ** 2
    inv = np.zeros_like(k2)
    inv[k2 > 0] = 1.0 / k2[k2 > 0]
    kk = [kx, ky, kz]
    return kk[i] * kk[j] * inv - (1.0 / 3.0 if i == j else 0.0)


def s2_from_dk64(dk64, n, L):
    import scipy.fft as sf
    s2 = np.zeros((n, n, n))
    for i, j in JVEC:
        s2 += (1.0 if i == j else 2.0) * sf.irfftn(sij_factor64(i, j, n, L) * dk64, s=(n, n, n)) ** 2
    return s2


def n2_from_dk64(dk64, n, L):
    import scipy.fft as sf
    kx, ky, kz = kvec64(n, L)
    return sf.irfftn(-(kx ** 2 + ky ** 2 + kz ** 2) * dk64, s=(n, n, n))


def fields64(delta, n, L):
    import scipy.fft as sf
    d = delta.astype(np.float64)
    dk64 = sf.rfftn(d)
    s2 = s2_from_dk64(dk64, n, L)
    return d - d.mean(), d * d - (d * d).mean(), s2 - s2.mean(), n2_from_dk64(dk64, n, L)


def W64(L, n, paste, interlaced):
    """the compensation window of the deposit in float64 (what get_W_compensated returns as float32): with u = pi m / n for the
    signed mode number m, interlaced (sin u / u)^p with p = 3 (TSC) or 2 (CIC); otherwise the first-order aliasing form
    sqrt(1 - s + 2 s^2 / 15) (TSC) or sqrt(1 - 2 s / 3) (CIC) with s = sin^2 u"""
    m = np.arange(n)
    m = np.where(m < (n + 1) // 2, m, m - n)
    u = np.pi * m / n
    if interlaced:
        return np.sinc(u / np.pi) ** (3.0 if paste == 'TSC' else 2.0)
    s = np.sin(u) ** 2
    return np.sqrt(1 - s + 2.0 * s * s / 15.0) if paste == 'TSC' else np.sqrt(1 - 2.0 * s / 3.0)


def field_fft64(P, pos, L, n, paste, w, compensated, interlaced):
    """get_field_fft with float64 positions, weights, meshes and window; the interlaced branch of the reference ignores `dtype`
    (its four lines are restated with float64 meshes)"""
    import scipy.fft as sf
    pos = pos.astype(np.float64)
    w = None if w is None else w.astype(np.float64)
    if interlaced:
        d = L / n
        f = sf.rfftn(quiet(P.get_field, pos, L, n, paste, w, dtype=np.float64))
        fs = sf.rfftn(quiet(P.get_field, pos, L, n, paste, w, d=0.5 * d, dtype=np.float64))
        P.shift_field_fft(f, fs, n, L, d, dtype=np.float64)
    else:
        f = sf.rfftn(quiet(P.get_field, pos, L, n, paste, w, dtype=np.float64)) * (1.0 / n ** 3)
    if compensated:
        W = W64(L, n, paste, interlaced)
        f = f / (W[:, None, None] * W[None, :, None] * W[None, None, :n // 2 + 1])
    return f


def pk64(a, b, L, kedges, muedges, poles):
    """calc_pk_from_deltak in float64 sums.  The (k, mu) bin of a mode is a discrete choice: it is made as the reference makes it,
    with float32 squared edges and float32 mu^2 (bin_kmu :217-256), so that both evaluations average the same modes."""
    n = a.shape[0]
    dk = 2.0 * np.pi / L
    raw = (np.conj(a) * b).real if b is not None else np.abs(a) ** 2
    ke2 = ((kedges / dk) ** 2).astype(np.float32)
    me2 = (muedges ** 2).astype(np.float32)
    idx = np.arange(n)
    f = np.where(idx < n // 2, idx, idx - n)
    kz = np.arange(n // 2 + 1)
    k2i = (f[:, None, None] ** 2 + f[None, :, None] ** 2 + kz[None, None, :] ** 2)
    kmag2 = k2i.astype(np.float32)
    with np.errstate(divide='ignore', invalid='ignore'):
        mu2_32 = np.where(k2i > 0, (kz[None, None, :] ** 2).astype(np.float32) * kmag2 ** np.float32(-1), np.float32(0)).astype(np.float32)
        mu2_64 = np.where(k2i > 0, kz[None, None, :] ** 2 / np.maximum(k2i, 1), 0.0)
    mu2_32 = np.broadcast_to(mu2_32, k2i.shape)
    mu2_64 = np.broadcast_to(mu2_64, k2i.shape)
    keep = (kmag2 >= ke2[0]) & (kmag2 < ke2[-1])
    bk = np.searchsorted(ke2[1:], kmag2, side='left')
    bmu = np.searchsorted(me2[1:], mu2_32, side='left')
    Nk, Nmu = len(kedges) - 1, len(muedges) - 1
    mult = np.broadcast_to(np.where(kz == 0, 1, 2)[None, None, :], k2i.shape)
    flat = (bk * Nmu + bmu)[keep]
    m = mult[keep]
    cnt = np.bincount(flat, weights=m, minlength=Nk * Nmu).reshape(Nk, Nmu).astype(np.int64)
    psum = np.bincount(flat, weights=m * raw[keep], minlength=Nk * Nmu).reshape(Nk, Nmu)
    cnt_k = cnt.sum(axis=1)
    pole_sums = np.zeros((len(poles), Nk))
    mu = np.sqrt(mu2_64[keep])
    for ip, ell in enumerate(poles):
        if ell == 0:
            pole_sums[ip] = psum.sum(axis=1)
        else:
            leg = np.polynomial.legendre.legval(mu, [0] * ell + [1]) * (2 * ell + 1)
            pole_sums[ip] = np.bincount(bk[keep], weights=m * raw[keep] * leg, minlength=Nk)
    with np.errstate(divide='ignore', invalid='ignore'):
        power = np.where(cnt > 0, psum / np.maximum(cnt, 1), psum) * L ** 3
        bpoles = np.where(cnt_k[None, :] > 0, pole_sums / np.maximum(cnt_k, 1)[None, :], pole_sums) * L ** 3
    return dict(power=power, N_mode=cnt, binned_poles=bpoles, N_mode_poles=cnt_k)


def white(seed, n):
    return np.random.default_rng(seed).standard_normal((n, n, n)).astype(np.float32)


def zeldovich(delta, n, L):
    """displacement of the density in box units: psi_k = i k / k^2 delta_k (float64 NumPy), returned as float32 meshes"""
    import scipy.fft as sf
    kx, ky, kz = kvec64(n, L)
    k2 = kx ** 2 + ky ** 2 + kz ** 2
    inv = np.zeros_like(k2)
    inv[k2 > 0] = 1.0 / k2[k2 > 0]
    dk = sf.rfftn(delta.astype(np.float64))
    return [(sf.irfftn(1j * k * inv * dk, s=(n, n, n)) / L).astype(np.float32) for k in (kx + 0 * k2, ky + 0 * k2, kz + 0 * k2)]


def lattice_numpy(disp, n, L, D, f_growth):
    """One particle per lattice site (i, j, k) of an n^3 mesh, moved by the displacement (box units) scaled by the growth factor,
    the line-of-sight component also by 1 + f_growth: what advect_fields.py main :213-239 computes, written as float32 array
    arithmetic over the site indices.  Every step is one correctly rounded float32 operation, in this order: scale, add the site's
    box coordinate index / n, times the box size, NumPy's remainder."""
    f4 = np.float32
    site = np.indices((n, n, n), dtype=np.int64).reshape(3, -1)
    scale = [(f4(D),), (f4(D),), (f4(D), f4(1 + f_growth))]
    out = np.empty((n ** 3, 3), dtype=f4)
    for axis in range(3):
        x = disp[axis].reshape(-1).astype(f4)
        for factor in scale[axis]:
            x = x * factor
        x = x + site[axis].astype(f4) / f4(n)
        x = x * f4(L)
        out[:, axis] = np.remainder(x, f4(L))
    assert out.dtype == f4
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    assert int(np.__version__.split('.')[0]) >= 2, 'golden vectors are generated under NumPy >= 2'
    I, P = import_reference(sys.argv[1])
    import scipy.fft as sf
    G = {}
    L = 200.0

    # ---- 1. gaussian_filter: white noise 16^3 and 24^3, kcut = half the Nyquist frequency and a smaller one
    filter_names = []
    filtered = {}
    for n in (16, 24):
        f = white(100 + n, n)
        kny = np.pi * n / L
        for tag, kcut in (('half', 0.5 * kny), ('fifth', 0.2 * kny)):
            name = f'white{n}_{tag}'
            ref = I.gaussian_filter(f.copy(), n, L, kcut)
            assert ref.dtype == np.float32
            G[f'filter/{name}/field'], G[f'filter/{name}/Lbox'], G[f'filter/{name}/kcut'] = f, np.float64(L), np.float64(kcut)
            G[f'filter/{name}/out'] = ref
            G[f'filter/{name}/e_ref'] = relmax(ref, filter64(f, n, L, kcut))
            print(f'filter {name}: e_ref {G[f"filter/{name}/e_ref"]:.3g}')
            filter_names.append(name)
            filtered[name] = ref
    G['filter_names'] = np.array(filter_names)

    # ---- 2. get_fields: filtered fields, unfiltered white noise (full power on the Nyquist planes), a lognormal field with a mean,
    #         and the plane wave of the known-answer tests at 16^3 (its e_ref scales their bounds)
    n = 16
    x = np.arange(n) / n
    wave = (0.7 * np.cos(2 * np.pi * (1 * x[:, None, None] + 2 * x[None, :, None] + 3 * x[None, None, :]))).astype(np.float32)
    fields_cases = [(f'filtered_{k}', v) for k, v in filtered.items() if k.endswith('half')]
    fields_cases.append(('white16_unfiltered', white(7, 16)))
    fields_cases.append(('lognormal24', np.exp(0.8 * white(24, 24)).astype(np.float32)))
    fields_cases.append(('planewave16', wave))
    for name, delta in fields_cases:
        n = len(delta)
        ref = quiet(I.get_fields, delta.copy(), L, n)
        f64 = fields64(delta, n, L)
        G[f'fields/{name}/delta'], G[f'fields/{name}/Lbox'] = delta, np.float64(L)
        for key, r, f in zip(('d', 'd2', 's2', 'n2'), ref, f64):
            assert r.dtype == np.float32 and r.shape == (n, n, n), (key, r.dtype, r.shape)
            G[f'fields/{name}/{key}'] = r
            G[f'fields/{name}/e_ref_{key}'] = relmax(r, f)
        print(f'fields {name}: e_ref ' + ' '.join(f'{k} {G[f"fields/{name}/e_ref_{k}"]:.3g}' for k in ('d', 'd2', 's2', 'n2')))
    G['fields_names'] = np.array([c[0] for c in fields_cases])
    G['planewave/A'], G['planewave/m'] = np.float64(0.7), np.array([1, 2, 3], dtype=np.int64)

    # ---- 3. the piecewise functions on a 16^3 spectrum
    n = 16
    kcut = 0.5 * np.pi * n / L
    dk = sf.rfftn(white(33, n)).astype(np.complex64)
    dk64 = dk.astype(np.complex128)
    kx, ky, kz = kvec64(n, L)
    k2 = kx ** 2 + ky ** 2 + kz ** 2
    G['spectral/delta_k'], G['spectral/Lbox'], G['spectral/kcut'] = dk, np.float64(L), np.float64(kcut)
    spectral = {'filter_field': (I.filter_field(dk.copy(), n, L, kcut), np.exp(-k2 / (2 * kcut ** 2)) * dk64),
                'n2_fft': (I.get_n2_fft(dk.copy(), n, L), -k2 * dk64)}
    for i, j in JVEC:
        spectral[f'sij_fft_{i}{j}'] = (I.get_sij_fft(i, j, dk.copy(), n, L), sij_factor64(i, j, n, L) * dk64)
    fin, add = white(34, n), white(35, n)
    fin_ref = fin.copy()
    I.add_ij(fin_ref, add, n, 2.0)
    G['spectral/add_ij/final'], G['spectral/add_ij/add'], G['spectral/add_ij/factor'] = fin, add, np.float64(2.0)
    spectral['add_ij'] = (fin_ref, fin.astype(np.float64) + 2.0 * add.astype(np.float64) ** 2)
    spectral['dk_to_s2'] = (I.get_dk_to_s2(dk.copy(), n, L), s2_from_dk64(dk64, n, L))
    spectral['dk_to_n2'] = (I.get_dk_to_n2(dk.copy(), n, L), n2_from_dk64(dk64, n, L))
    for name, (ref, f64) in spectral.items():
        assert ref.dtype in (np.float32, np.complex64), (name, ref.dtype)
        G[f'spectral/{name}/out'] = ref
        G[f'spectral/{name}/e_ref'] = relmax(ref, f64)
        print(f'spectral {name}: e_ref {G[f"spectral/{name}/e_ref"]:.3g}')
    G['spectral_names'] = np.array(list(spectral))

    # ---- 4. lattice positions: displacement rms about 3 cells (many sites wrap), D = 0.6, f_growth 0 and 0.8
    n = 12
    rng = np.random.default_rng(44)
    disp = [(3.0 / n / 0.6 * rng.standard_normal((n, n, n))).astype(np.float32) for _ in range(3)]
    for q, a in enumerate(disp):
        G[f'lattice/disp_{"xyz"[q]}'] = a
    G['lattice/Lbox'], G['lattice/D'] = np.float64(L), np.float64(0.6)
    lattice_names = []
    for tag, fg in (('f0', 0.0), ('f0.8', 0.8)):
        pos = lattice_numpy(disp, n, L, 0.6, fg)
        assert pos.dtype == np.float32
        G[f'lattice/{tag}/f_growth'], G[f'lattice/{tag}/pos'] = np.float64(fg), pos
        lattice_names.append(tag)
        print(f'lattice {tag}: {(pos == np.float32(L)).sum()} coordinates equal Lbox, rms displacement '
              f'{np.sqrt(np.mean((disp[0] * 0.6 * n) ** 2)):.2f} cells')
    G['lattice_names'] = np.array(lattice_names)

    # ---- 5. advect: Gaussian-filtered white-noise density and its own Zel'dovich displacement, four deposit modes
    # (a small box: nabla^2 delta ~ k^2 delta is then of order one like the other weights.  get_field forms mesh * norm - 1 in
    # float32, so a weighted field whose values are far below one loses that many digits in the reference itself)
    n = 16
    L = 25.0
    D, fg = 0.6, 0.5
    kny = np.pi * n / L
    kcut = 0.5 * kny
    dens0 = (1.2 * white(55, n)).astype(np.float32)
    dens = I.gaussian_filter(dens0, n, L, kcut)
    # (the amplitude of the displacement is set to an rms of about one cell after growth, so that the advected '1cb' field - unit
    # weights - carries signal well above the float32 noise of a deposit)
    psi = [I.gaussian_filter(p, n, L, kcut) for p in zeldovich(dens0, n, L)]
    amp = np.float32(1.0 / (n * D * np.sqrt(np.mean(np.square(psi[0], dtype=np.float64)))))
    psi = [(p * amp).astype(np.float32) for p in psi]
    d, d2, s2, n2 = quiet(I.get_fields, dens.copy(), L, n)
    weights = {'delta': d, 'delta2': d2, 'tidal2': s2, 'nabla2': n2}
    pos = lattice_numpy(psi, n, L, D, fg)
    kedges, muedges = P.get_k_mu_edges(L, kny, 8, 4, False)
    G['advect/Lbox'], G['advect/D'], G['advect/f_growth'] = np.float64(L), np.float64(D), np.float64(fg)
    G['advect/k_bin_edges'], G['advect/mu_bin_edges'], G['advect/poles'] = kedges, muedges, np.array(POLES, dtype=np.int64)
    for q, a in enumerate(psi):
        G[f'advect/disp_{"xyz"[q]}'] = a
    for k, v in weights.items():
        G[f'advect/field_{k}'] = v
    print(f'advect: rms displacement {np.sqrt(np.mean((psi[0] * D * n) ** 2)):.2f} cells')
    field_D = [1, D, D ** 2, D ** 2, D]
    # tracers in [-L/2, L/2): a biased sample of the advected lattice plus uniform points
    rng = np.random.default_rng(66)
    p_sel = np.exp(1.5 * d.flatten() / d.std())
    sel = rng.choice(n ** 3, size=1500, replace=False, p=p_sel / p_sel.sum())
    tr = np.concatenate([pos[sel].astype(np.float64) + rng.uniform(-0.3, 0.3, (1500, 3)) * (L / n), rng.uniform(0, L, (500, 3))])
    tracer0 = ((tr % L) - L / 2).astype(np.float32)
    tracer0 = np.clip(tracer0, -L / 2, np.nextafter(np.float32(L / 2), np.float32(0))).astype(np.float32)
    G['tracer/pos'] = tracer0
    shifted = tracer0.copy()
    shifted += L / 2.0
    shifted %= L
    G['tracer/pos_shifted'] = shifted
    advect_names = []
    for paste, comp, inter in MODES:
        mn = mode_name(paste, comp, inter)
        advect_names.append(mn)
        W = P.get_W_compensated(L, n, paste, inter) if comp else None
        spec, spec64 = [], []
        for i, key in enumerate(KEYNAMES):
            w = None if i == 0 else weights[key].flatten()
            ref = quiet(P.get_field_fft, pos.copy(), L, n, paste, w, W, comp, inter)
            assert ref.dtype == np.complex64, ref.dtype
            f64 = field_fft64(P, pos, L, n, paste, w, comp, inter)
            spec.append(ref)
            spec64.append(f64)
            G[f'advect/{mn}/spec_{key}'] = ref
            G[f'advect/{mn}/e_ref_spec_{key}'] = relmax(ref, f64)
        print(f'advect {mn}: spectra e_ref ' + ' '.join(f'{G[f"advect/{mn}/e_ref_spec_{k}"]:.3g}' for k in KEYNAMES))
        worst = 0.0
        for i in range(len(KEYNAMES)):
            for j in range(len(KEYNAMES)):
                if i < j:
                    continue
                Pij = P.calc_pk_from_deltak(spec[i], L, kedges, muedges, field2_fft=spec[j], poles=np.asarray(POLES))
                Pij['power'] *= field_D[i] * field_D[j]
                Pij['binned_poles'] *= field_D[i] * field_D[j]
                P64 = pk64(spec64[i], spec64[j], L, kedges, muedges, POLES)
                assert np.array_equal(Pij['N_mode'], P64['N_mode']) and np.array_equal(Pij['N_mode_poles'], P64['N_mode_poles'])
                pair = f'{KEYNAMES[i]}_{KEYNAMES[j]}'
                G[f'advect/{mn}/P_kmu_{pair}'], G[f'advect/{mn}/N_kmu_{pair}'] = Pij['power'], Pij['N_mode']
                G[f'advect/{mn}/P_ell_{pair}'], G[f'advect/{mn}/N_ell_{pair}'] = Pij['binned_poles'], Pij['N_mode_poles']
                e = max(relbin(Pij['power'], P64['power'] * field_D[i] * field_D[j]),
                        relbin(Pij['binned_poles'], P64['binned_poles'] * field_D[i] * field_D[j]))
                G[f'advect/{mn}/e_ref_{pair}'] = np.float64(e)
                worst = max(worst, e)
                print(f'    advect {mn} {pair}: e_ref {e:.3g}')
        print(f'advect {mn}: 15 pairs, largest e_ref {worst:.3g}')

        # ---- 6. tracer x fields through tracer_power.py :155-273
        tpos = tracer0.copy()
        tpos += L / 2.0
        tpos %= L
        tr_fft = quiet(P.get_field_fft, tpos.copy(), L, n, paste, None, W, comp, inter)
        tr64 = field_fft64(P, tpos, L, n, paste, None, comp, inter)
        worst = 0.0
        for key, a, a64, g in [('tr', tr_fft, tr64, 1.0)] + [(k, spec[i], spec64[i], field_D[i]) for i, k in enumerate(KEYNAMES)]:
            auto = key == 'tr'
            Pt = P.calc_pk_from_deltak(a, L, kedges, muedges, field2_fft=None if auto else tr_fft, poles=np.asarray(POLES))
            Pt['power'] *= g
            Pt['binned_poles'] *= g
            P64 = pk64(a64, None if auto else tr64, L, kedges, muedges, POLES)
            assert np.array_equal(Pt['N_mode'], P64['N_mode'])
            pair = f'{key}_tr'
            G[f'tracer/{mn}/P_kmu_{pair}'], G[f'tracer/{mn}/N_kmu_{pair}'] = Pt['power'], Pt['N_mode']
            G[f'tracer/{mn}/P_ell_{pair}'], G[f'tracer/{mn}/N_ell_{pair}'] = Pt['binned_poles'], Pt['N_mode_poles']
            e = max(relbin(Pt['power'], P64['power'] * g), relbin(Pt['binned_poles'], P64['binned_poles'] * g))
            G[f'tracer/{mn}/e_ref_{pair}'] = np.float64(e)
            worst = max(worst, e)
            print(f'    tracer {mn} {pair}: e_ref {e:.3g}')
        print(f'tracer {mn}: 6 spectra, largest e_ref {worst:.3g}')
    G['advect_names'] = np.array(advect_names)
    G['keynames'] = np.array(KEYNAMES)

    # three files, each well under the 1 MiB a committed file may have (white noise does not compress)
    parts = {'zcv_cases.npz': ('filter', 'spectral', 'lattice'), 'zcv_fields_cases.npz': ('fields', 'planewave'),
             'zcv_advect_cases.npz': ('advect', 'tracer', 'keynames')}
    done = set()
    for fn, heads in parts.items():
        sub = {k: v for k, v in G.items() if k.split('/')[0].split('_names')[0] in heads}
        done |= set(sub)
        out = REPO / 'tests' / 'golden' / fn
        np.savez_compressed(out, **sub)
        print(out, out.stat().st_size, 'bytes')
        assert out.stat().st_size < 1 << 20
    assert done == set(G), set(G) - done


if __name__ == '__main__':
    main()
