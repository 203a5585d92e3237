#!/usr/bin/env python
"""Writes tests/golden/lcv_cases.npz (linear fields, field-level combination) and tests/golden/lcv_recon_cases.npz (tracer minus
randoms): the REFERENCE's own functions - scipy's rfftn, analysis/power_spectrum.py get_delta_mu2, get_field_fft,
calc_pk_from_deltak, get_smoothing and hod/zcv/tools_cv.py combine_field_spectra_k3D_lcv - run under the identity Numba shim of
oracle/shim on small seeded inputs, following hod/zcv/linear_fields.py main :108-170 and tracer_power.py get_recon_power :396-532.

    python scripts/make_lcv_golden.py /path/to/abacusutils

Needs what scripts/make_zcv_golden.py needs (whose helpers and `e_ref` definitions are imported, not copied).  The reference's
combine function reads its six 3-D products through `asdf.open(fn)['data'][key]`: the `asdf` stand-in is given an `open()` that
serves the arrays from memory.

`e_ref` is defined exactly as in the ZCV script: the reference's float32 result against a float64 evaluation of the same formulas,
`relmax` for spectra and 3-D grids, `relbin` for binned spectra.  The tracer - randoms spectrum cancels partly: its e_ref is taken
of the difference, relative to the difference's largest value.

`rec_algo='reciso'` of combine_field_spectra_k3D_lcv cannot run in the reference (it reshapes the (n, n, n//2+1) smoothing kernel
to (n, n, n): ValueError; asserted below).  The `combine/reciso` arrays are therefore NOT reference output: they are this script's
NumPy float32 evaluation of the same combination with f_eff = f_growth (1 - S) on the (n, n, n//2+1) grid, S the reference's own
get_smoothing output and the P_k3D arrays the same ones the recsym call reads.  `combine/reciso/source` records that.
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import make_zcv_golden as Z  # noqa: E402

REPO = Z.REPO
KEYNAMES = ['delta', 'deltamu2']
PAIRS = [('delta', 'delta'), ('deltamu2', 'delta'), ('deltamu2', 'deltamu2')]
POLES = Z.POLES


def mu2_64(n):
    idx = np.arange(n)
    f = np.where(idx < n // 2, idx, idx - n).astype(np.float64)
    kz = np.arange(n // 2 + 1, dtype=np.float64)
    k2 = f[:, None, None] ** 2 + f[None, :, None] ** 2 + kz[None, None, :] ** 2
    return np.where(k2 > 0, kz[None, None, :] ** 2 / np.maximum(k2, 1.0), 0.0), k2


def p3d(a, b):
    """the reference's save_3D_power product (linear_fields.py:138-141, tracer_power.py:464, :501-503)"""
    return np.array((a * np.conj(b)).real, dtype=np.float32)


def store_binned(G, head, pair, Pref, P64):
    assert np.array_equal(Pref['N_mode'], P64['N_mode'].reshape(Pref['N_mode'].shape)) and np.array_equal(Pref['N_mode_poles'], P64['N_mode_poles'])
    G[f'{head}/P_kmu_{pair}'], G[f'{head}/N_kmu_{pair}'] = Pref['power'], Pref['N_mode']
    G[f'{head}/P_ell_{pair}'], G[f'{head}/N_ell_{pair}'] = Pref['binned_poles'], Pref['N_mode_poles']
    e = max(Z.relbin(Pref['power'], P64['power'].reshape(Pref['power'].shape)), Z.relbin(Pref['binned_poles'], P64['binned_poles']))
    G[f'{head}/e_ref_{pair}'] = np.float64(e)
    return e


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    assert int(np.__version__.split('.')[0]) >= 2, 'golden vectors are generated under NumPy >= 2'
    I, P = Z.import_reference(sys.argv[1])
    import abacusnbody.hod.zcv.linear_fields as LF  # noqa: F401  (imports must work: the recipe below follows its main)
    import abacusnbody.hod.zcv.tools_cv as T
    import scipy.fft as sf
    G = {}
    L = 200.0

    # ---- 1. linear fields: Gaussian-filtered white noise at 16^3 and 24^3 (24 is not a power of two; kzlen is 13 of 16 padded
    #         columns) and unfiltered white noise, which has full power on the Nyquist planes
    lin_cases = []
    for n in (16, 24):
        lin_cases.append((f'white{n}', I.gaussian_filter(Z.white(200 + n, n), n, L, 0.5 * np.pi * n / L)))
    lin_cases.append(('white16_unfiltered', Z.white(77, 16)))
    spectra, spectra64, edges = {}, {}, {}
    for name, delta in lin_cases:
        n = len(delta)
        assert delta.dtype == np.float32
        delta_fft = sf.rfftn(delta, workers=-1) / np.float32(n ** 3)                    # linear_fields.py:114
        assert delta_fft.dtype == np.complex64 and np.array_equal(delta_fft, sf.rfftn(delta, workers=-1) / n ** 3)     # tracer_power.py:446
        fields = {'delta': delta_fft, 'deltamu2': P.get_delta_mu2(delta_fft, n)}
        d64 = sf.rfftn(delta.astype(np.float64)) / float(n) ** 3
        fields64 = {'delta': d64, 'deltamu2': d64 * mu2_64(n)[0]}
        ke, me = P.get_k_mu_edges(L, np.pi * n / L, n // 2, 4, False)
        G[f'linear/{name}/delta_lin'], G[f'linear/{name}/Lbox'] = delta, np.float64(L)
        G[f'linear/{name}/k_bin_edges'], G[f'linear/{name}/mu_bin_edges'], G[f'linear/{name}/poles'] = ke, me, np.array(POLES, dtype=np.int64)
        for key in KEYNAMES:
            assert fields[key].dtype == np.complex64
            G[f'linear/{name}/spec_{key}'] = fields[key]
            G[f'linear/{name}/e_ref_spec_{key}'] = Z.relmax(fields[key], fields64[key])
        for a, b in PAIRS:
            pair = f'{a}_{b}'
            Pij = P.calc_pk_from_deltak(fields[a], L, ke, me, field2_fft=fields[b], poles=np.asarray(POLES))
            e = store_binned(G, f'linear/{name}', pair, Pij, Z.pk64(fields64[a], fields64[b], L, ke, me, POLES))
            pk3d = p3d(fields[a], fields[b])
            G[f'linear/{name}/P_k3D_{pair}'] = pk3d
            G[f'linear/{name}/e_ref_k3D_{pair}'] = Z.relmax(pk3d, (fields64[a] * np.conj(fields64[b])).real)
            print(f'linear {name} {pair}: binned e_ref {e:.3g}, 3-D e_ref {G[f"linear/{name}/e_ref_k3D_{pair}"]:.3g}')
        print(f'linear {name}: spectra e_ref ' + ' '.join(f'{G[f"linear/{name}/e_ref_spec_{k}"]:.3g}' for k in KEYNAMES))
        spectra[name], spectra64[name], edges[name] = fields, fields64, (ke, me)
    G['linear_names'] = np.array([c[0] for c in lin_cases])

    # ---- 2. recon: 3000 tracers (a biased sample of the `white16` density plus uniform points) and 12000 uniform randoms, both
    #         reaching three cells outside [0, L) on both sides as reconstruction leaves them
    n = 16
    dens = dict(lin_cases)['white16']
    fields, fields64 = spectra['white16'], spectra64['white16']
    ke, me = edges['white16']
    cell = L / n
    rng = np.random.default_rng(88)
    p_sel = np.exp(1.5 * dens.flatten() / dens.std())
    sel = rng.choice(n ** 3, size=2500, p=p_sel / p_sel.sum())
    site = np.stack(np.unravel_index(sel, (n, n, n)), axis=1).astype(np.float64)
    tr = np.concatenate([(site + rng.uniform(0.0, 1.0, (2500, 3))) * cell, rng.uniform(0, L, (500, 3))])
    rn = rng.uniform(0, L, (12000, 3))

    def spill(pos):
        """every second point within three cells of a face moves to the periodic image beyond that face"""
        pos = pos.copy()
        flip = rng.random(pos.shape) < 0.5
        low, high = (pos < 3 * cell) & flip, (pos > L - 3 * cell) & flip
        pos[low] += L
        pos[high] -= L
        return pos.astype(np.float32)
    tracer, randoms = spill(tr), spill(rn)
    for nm, p in (('tracer', tracer), ('randoms', randoms)):
        assert p.min() < -2 * cell and p.max() > L + 2 * cell and p.min() > -3.01 * cell and p.max() < L + 3.01 * cell, (nm, p.min(), p.max())
    G['recon/tracer_pos'], G['recon/random_pos'], G['recon/linear_case'] = tracer, randoms, np.array('white16')
    G['recon/k_bin_edges'], G['recon/mu_bin_edges'], G['recon/poles'] = ke, me, np.array(POLES, dtype=np.int64)
    recon_names = []
    kept = {}
    cases = [(Z.mode_name(*m), m, True, me) for m in Z.MODES] + [('TSC_TT_norandoms', Z.MODES[0], False, me),
                                                                  ('TSC_TT_mu1', Z.MODES[0], True, np.array([0.0, 1.0]))]
    for name, (paste, comp, inter), with_rn, mue in cases:
        recon_names.append(name)
        key = (paste, comp, inter, with_rn)
        if key not in kept:
            W = P.get_W_compensated(L, n, paste, inter) if comp else None
            tr_fft = Z.quiet(P.get_field_fft, tracer.copy(), L, n, paste, None, W, comp, inter)       # tracer_power.py:407-409
            tr64 = Z.field_fft64(P, tracer, L, n, paste, None, comp, inter)
            if with_rn:
                tr_fft -= Z.quiet(P.get_field_fft, randoms.copy(), L, n, paste, None, W, comp, inter)  # :411-414
                tr64 = tr64 - Z.field_fft64(P, randoms, L, n, paste, None, comp, inter)
            assert tr_fft.dtype == np.complex64
            kept[key] = (tr_fft, tr64)
        tr_fft, tr64 = kept[key]
        head = f'recon/{name}'
        G[f'{head}/mu_bin_edges'] = mue
        G[f'{head}/spec_tr'], G[f'{head}/e_ref_spec_tr'] = tr_fft, Z.relmax(tr_fft, tr64)
        worst = 0.0
        for pair, a, a64 in [('tr_tr', tr_fft, tr64)] + [(f'{k}_tr', fields[k], fields64[k]) for k in KEYNAMES]:
            auto = pair == 'tr_tr'
            Pt = P.calc_pk_from_deltak(a, L, ke, mue, field2_fft=None if auto else tr_fft, poles=np.asarray(POLES))
            worst = max(worst, store_binned(G, head, pair, Pt, Z.pk64(a64, None if auto else tr64, L, ke, mue, POLES)))
            pk3d = p3d(a, tr_fft)
            G[f'{head}/P_k3D_{pair}'] = pk3d
            G[f'{head}/e_ref_k3D_{pair}'] = Z.relmax(pk3d, (a64 * np.conj(tr64)).real)
        print(f'recon {name}: spectrum e_ref {G[f"{head}/e_ref_spec_tr"]:.3g}, largest binned e_ref {worst:.3g}, 3-D e_ref '
              + ' '.join(f'{G[f"{head}/e_ref_k3D_{p}"]:.3g}' for p in ('tr_tr', 'delta_tr', 'deltamu2_tr')))
    G['recon_names'] = np.array(recon_names)

    # ---- 3. combine_field_spectra_k3D_lcv on the TSC_TT products, the reference's function through an in-memory asdf.open
    bias, f_growth, D, R = 1.8, 0.75, 0.6, 10.0
    lin_keys = [f'P_k3D_{a}_{b}' for a, b in PAIRS]
    tr_keys = ['P_k3D_tr_tr', 'P_k3D_delta_tr', 'P_k3D_deltamu2_tr']
    store = {k: {'data': {k: G[f'linear/white16/{k}']}} for k in lin_keys}
    store.update({k: {'data': {k: G[f'recon/TSC_TT/{k}']}} for k in tr_keys})
    T.asdf.open = lambda fn: store[fn]
    tr_fft, tr64 = kept[('TSC', True, True, True)]
    d64, m64 = fields64['delta'], fields64['deltamu2']

    def combine64(f_eff):
        ll = D ** 2 * (2.0 * bias * f_eff * (m64 * np.conj(d64)).real + f_eff ** 2 * np.abs(m64) ** 2 + bias ** 2 * np.abs(d64) ** 2)
        lt = D * (bias * (d64 * np.conj(tr64)).real + f_eff * (m64 * np.conj(tr64)).real)
        return np.abs(tr64) ** 2, ll, lt
    ref = T.combine_field_spectra_k3D_lcv(bias, f_growth, D, lin_keys, tr_keys, n, L, R, 'recsym')
    try:
        T.combine_field_spectra_k3D_lcv(bias, f_growth, D, lin_keys, tr_keys, n, L, R, 'reciso')
        raise AssertionError('the reference ran its reciso branch: pin reciso to it')
    except ValueError as e:
        print('reference reciso:', e)
    # reciso, restated: the Kaiser factor is damped per mode by the reference's own smoothing kernel, on the rfftn grid
    S = P.get_smoothing(n, L, R)
    assert S.dtype == np.float32 and S.shape == (n, n, n // 2 + 1)
    damp = f_growth * (1.0 - S)
    Pdd, Pmd, Pmm = (store[k]['data'][k] for k in lin_keys)
    Ptt, Pdt, Pmt = (store[k]['data'][k] for k in tr_keys)
    iso = (Ptt, D ** 2 * (2.0 * bias * damp * Pmd + damp ** 2 * Pmm + bias ** 2 * Pdd), D * (bias * Pdt + damp * Pmt))
    S64 = np.exp(-mu2_64(n)[1] * (2.0 * np.pi / L) ** 2 * R ** 2 / 2.0)
    for algo, got, want64 in (('recsym', ref, combine64(f_growth)), ('reciso', iso, combine64(f_growth * (1.0 - S64)))):
        for key, g, w in zip(('pk_tt', 'pk_ll', 'pk_lt'), got, want64):
            assert g.dtype == np.float32 and g.shape == (n, n, n // 2 + 1), (algo, key, g.dtype, g.shape)
            G[f'combine/{algo}/{key}'], G[f'combine/{algo}/e_ref_{key}'] = g, Z.relmax(g, w)
        print(f'combine {algo}: e_ref ' + ' '.join(f'{k} {G[f"combine/{algo}/e_ref_{k}"]:.3g}' for k in ('pk_tt', 'pk_ll', 'pk_lt')))
    G['combine/recsym/source'] = np.array("the reference's tools_cv.combine_field_spectra_k3D_lcv")
    G['combine/reciso/source'] = np.array("NumPy float32 evaluation by scripts/make_lcv_golden.py from the reference's get_smoothing and "
                                          'P_k3D arrays (the reference raises ValueError on this branch)')
    for k, v in (('bias', bias), ('f_growth', f_growth), ('D', D), ('R', R), ('Lbox', L)):
        G[f'combine/{k}'] = np.float64(v)
    G['combine/linear_case'], G['combine/recon_case'] = np.array('white16'), np.array('TSC_TT')
    G['combine_names'] = np.array(['recsym', 'reciso'])

    # two files, each well under the 1 MiB a committed file may have (white noise does not compress)
    parts = {'lcv_cases.npz': ('linear', 'combine'), 'lcv_recon_cases.npz': ('recon',)}
    done = set()
    for fn, heads in parts.items():
        sub = {k: v for k, v in G.items() if k.split('/')[0].split('_names')[0] in heads}
        done |= set(sub)
        out = REPO / 'tests' / 'golden' / fn
        np.savez_compressed(out, **sub)
        print(out, out.stat().st_size, 'bytes')
        assert out.stat().st_size < 700 << 10
    assert done == set(G), set(G) - done


if __name__ == '__main__':
    main()
