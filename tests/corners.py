"""Corner cases of the HOD populate shared by the oracle-vs-reference pin (CPU), the envelope / key test (CPU) and the
HIP-vs-oracle matrix (GPU): parameters outside every MCMC prior (where the host-built guards of the filter switch paths)
and catalogues with values the key window, the q code and the envelope ranges were not tuned for.

Every case exists as the three-tracer mix (dense superblocks) and, where the case touches the LRG block or the
catalogue, as its LRG-only restriction (sparse superblocks, key index) in three flag variants:
    <case>            LRG + ELG + QSO, ranks on, box RSD
    <case>_lrg        LRG alone, ranks on, box RSD
    <case>_lrg_plain  LRG alone, ranks off, rsd=False
    <case>_lrg_lc     LRG alone, ranks on, light-cone RSD (`origin`)
Where a case gives three values they are LRG / ELG / QSO."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np

from abacusutils_amd import synth

NH, NP, SEED = 100_003, 150_001, 4242   # 4 + 5 sparse superblocks of 16 x 2048 objects, ragged last tiles
NAN = float('nan')


def _each(**kw):
    return {tr: dict(kw) for tr in ('LRG', 'ELG', 'QSO')}


def _per(key, lrg, elg, qso):
    return {'LRG': {key: lrg}, 'ELG': {key: elg}, 'QSO': {key: qso}}


# parameter cases: overrides of synth.PRODUCTION_TRACERS per tracer
_PARAM_CASES = {
    'production': {},
    'sigma_tiny': _per('sigma', 1e-4, 1e-3, 1e-4),      # guard `sigma > 1e-3` fails
    'sigma_narrow': _per('sigma', 0.004, 0.01, 0.02),   # guard passes, erfc is a step
    'sigma_5': _each(sigma=5.0),
    # (ELG keeps its sigma: the reference's Gaussian divides a Python float by it and raises ZeroDivisionError)
    'sigma_zero': {'LRG': dict(sigma=0.0), 'QSO': dict(sigma=0.0)},
    'sigma_neg': _each(sigma=-0.3),
    'ic_zero': _each(ic=0.0),
    'ic_gt1': _per('ic', 1.7, 2.5, 0.3),
    'pmax_lt_invQ': {'ELG': dict(p_max=0.001, Q=20.0)},
    'cut_below_all': _each(logM_cut=9.0, logM1=16.5),
    'cut_above_all': _each(logM_cut=17.0),
    'alpha_zero': {'LRG': dict(alpha=0.0), 'ELG': dict(alpha=0.0, alpha_EE=0.0, alpha_EL=0.0), 'QSO': dict(alpha=0.0)},
    'alpha_neg': {'LRG': dict(alpha=-0.5)},             # sat_basic must fail
    'kappa_50': _each(kappa=50.0),
    'kappa_neg': _each(kappa=-2.0),
    'AB_3': {'LRG': dict(Acent=3.0, Bcent=-3.0, Asat=-3.0, Bsat=3.0), 'ELG': dict(Acent=-3.0, Bcent=3.0, Asat=3.0, Bsat=-3.0),
             'QSO': dict(Acent=3.0, Bcent=3.0, Asat=-3.0, Bsat=-3.0)},
    's_big': {'LRG': dict(s=-3.0), 'ELG': dict(s_v=2.5), 'QSO': dict(s_r=-2.0)},   # 1 + s * rank changes sign
    'gamma_neg': {'ELG': dict(gamma=-4.0)},
    'gamma_zero': {'ELG': dict(gamma=0.0)},
    'nan_sigma': _each(sigma=NAN),
    'nan_cut': _each(logM_cut=NAN),
}
# catalogue cases: production parameters on a modified catalogue
_CATALOGUE_CASES = ('catalogue', 'mass_nonfinite', 'env_50', 'env_nan', 'ranks_20')
VARIANTS = ('', '_lrg', '_lrg_plain', '_lrg_lc')


def _has_lrg_only(base):
    return base in _CATALOGUE_CASES or base == 'production' or 'LRG' in _PARAM_CASES[base]


_RANK_ONLY = ('s_big', 'ranks_20')   # with the ranks off these are the production case: no `_lrg_plain` variant
CORNERS = [base + v for base in list(_PARAM_CASES) + list(_CATALOGUE_CASES) for v in VARIANTS
           if v == '' or (_has_lrg_only(base) and not (v == '_lrg_plain' and base in _RANK_ONLY))]


@functools.lru_cache(maxsize=1)
def _base_catalogue():
    hd, pd, params = synth.synth_hod_inputs(NH, NP, seed=SEED, with_ranks=True)
    for d in (hd, pd):
        for v in d.values():
            v.setflags(write=False)
    return hd, pd, params


def _catalogue(kind):
    hd, pd, params = _base_catalogue()
    hd, pd = dict(hd), dict(pd)
    if kind is None:
        return hd, pd, params
    rng = np.random.default_rng(SEED + 1)
    host = pd['pinds']

    def own(d, *keys):
        for k in keys:
            d[k] = d[k].copy()

    if kind == 'catalogue':
        own(hd, 'hmultis', 'hmass')
        own(pd, 'pweights')
        hd['hmultis'][::7] = 0.0
        hd['hmultis'][3::11] = -1.0
        pd['pweights'][::5] = 0.0
        pd['pweights'][1::13] = -0.5
        hd['hrandoms'] = rng.random(NH, dtype=np.float32).astype(np.float64)
        pd['prandoms'] = rng.random(NP, dtype=np.float32).astype(np.float64)
        hd['hrandoms'][::14] = 0.0
        pd['prandoms'][::1000] = 0.0
        hd['hmass'][5::97] = 3e10     # below the key window (2^36 = 6.9e10) ...
        hd['hmass'][11::89] = 8e15    # ... and above it (2^51.9 = 4.2e15)
        pd['phmass'] = hd['hmass'][host]
    elif kind == 'mass_nonfinite':
        own(hd, 'hmass')
        big = np.argsort(hd['hmass'])[-40:]      # hosts that own particles
        hd['hmass'][big[3]] = NAN
        hd['hmass'][big[17]] = np.inf
        hd['hmass'][1234] = NAN
        hd['hmass'][4321] = np.inf
        pd['phmass'] = hd['hmass'][host]
    elif kind == 'env_50':
        hd['hdeltac'] = rng.uniform(-50.0, 50.0, NH)
        hd['hfenv'] = rng.uniform(-50.0, 50.0, NH)
        hd['hdeltac'][:2] = (-50.0, 50.0)
        hd['hfenv'][:2] = (50.0, -50.0)
        pd['pdeltac'], pd['pfenv'] = hd['hdeltac'][host], hd['hfenv'][host]
    elif kind == 'env_nan':
        own(hd, 'hdeltac')
        hd['hdeltac'][np.argsort(hd['hmass'])[-30::7]] = NAN
        hd['hdeltac'][17::9973] = NAN
        pd['pdeltac'] = hd['hdeltac'][host]
    elif kind == 'ranks_20':
        for k in ('pranks', 'pranksv', 'pranksp', 'pranksr'):
            pd[k] = rng.uniform(-20.0, 20.0, NP)
            pd[k][:2] = (-20.0, 20.0)
    else:
        raise KeyError(kind)
    return hd, pd, params


def split_name(name):
    """(base case, variant suffix)"""
    for v in ('_lrg_plain', '_lrg_lc', '_lrg'):
        if name.endswith(v):
            return name[:-len(v)], v
    return name, ''


def corner_case(name):
    """(halo_data, particle_data, params, tracers, enable_ranks, rsd) of one entry of CORNERS; the arrays of the unmodified
    catalogue are shared between the cases and read-only"""
    if name not in CORNERS:
        raise KeyError(name)
    base, variant = split_name(name)
    hd, pd, params = _catalogue(base if base in _CATALOGUE_CASES else None)
    over = _PARAM_CASES.get(base, {})
    if base == 'env_50':   # |A| = 0.3 on the wide environment columns
        over = {'LRG': dict(Acent=-0.3, Asat=0.3, Bcent=0.3, Bsat=-0.3), 'ELG': dict(Acent=0.3, Asat=-0.3, Bcent=-0.3, Bsat=0.3),
                'QSO': dict(Acent=0.3, Asat=0.3, Bcent=-0.3, Bsat=0.3)}
    tracers = {tr: dict(v, **over.get(tr, {})) for tr, v in synth.PRODUCTION_TRACERS.items()}
    if variant:
        tracers = {'LRG': tracers['LRG']}
    if variant == '_lrg_lc':
        params = dict(params, origin=np.array([-990.0, -990.0, -990.0]))
    plain = variant == '_lrg_plain'
    return hd, pd, params, tracers, not plain, not plain


def corner_checksum(hd, pd):
    """the input checksum of the golden files (conftest.input_checksum) with the non-finite entries some corners plant
    replaced by finite stand-ins, so that it still compares"""
    s = 0.0
    for d in (hd, pd):
        for k in sorted(d):
            a = np.nan_to_num(np.asarray(d[k], dtype=np.float64).ravel(), nan=-7.0, posinf=1e30, neginf=-1e30)
            s += float(np.dot(a, np.cos(np.arange(a.size) * 0.001)))
    return s


def neighbour(tracers, shift=0.07):
    """the same tracers with every logM_cut shifted"""
    return {tr: dict(v, logM_cut=v['logM_cut'] + shift) for tr, v in tracers.items()}


# ---- the host side of the filter (abacusutils_amd/csrc/hod_envelope.hpp), compiled for the host ---------------------------
_NATIVE = Path(__file__).resolve().parent / 'native'


@functools.lru_cache(maxsize=1)
def envelope_lib():
    """tests/native/envelope_host.cpp built with g++ (rebuilt when the header or the source is newer)"""
    so, src = _NATIVE / 'libenvelope_host.so', _NATIVE / 'envelope_host.cpp'
    csrc = _NATIVE.parents[1] / 'abacusutils_amd' / 'csrc'
    newest = max(f.stat().st_mtime for f in (src, csrc / 'hod_envelope.hpp', csrc / 'hod_classify.hpp'))
    if not so.exists() or so.stat().st_mtime < newest:
        subprocess.check_call(['g++', '-O2', '-ffp-contract=off', '-shared', '-fPIC', '-o', str(so), str(src)])
    return C.CDLL(str(so))


def _range(d, key, absent):
    """what compute_ranges measures on the device: NaNs ignored, an absent (or all-NaN) column keeps `absent`"""
    if key not in d:
        return absent, absent
    a = np.asarray(d[key], dtype=np.float64)
    a = a[~np.isnan(a)]
    return (float(a.min()), float(a.max())) if a.size else (absent, absent)


def host_keys(mass, wgt, rnd):
    """the 16-bit filter key of every object (k16_key)"""
    n = len(mass)
    out = np.empty(n, np.uint16)
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (mass, wgt, rnd)]
    envelope_lib().env_keys(C.c_int64(n), *[a.ctypes.data_as(C.c_void_p) for a in arrs], out.ctypes.data_as(C.c_void_p))
    return out


def envelope(hd, pd, params, tracers, enable_ranks, rsd, one_stage=0):
    """(flags, passes_c, passes_s): the guard flags {cent_ok, sat_ok, sat_basic, c_ok, s_ok} of make_filter / make_cheap and,
    per halo / particle, whether the key filter `code(key) <= table[bin(key)]` lets it through"""
    from abacusutils_amd.hod.GRAND_HOD import marshal_params
    p = marshal_params(tracers, params, enable_ranks, rsd)
    rng = [_range(hd, k, 0.0) for k in ('hdeltac', 'hfenv', 'hshear')] + [_range(pd, k, 0.0) for k in ('pdeltac', 'pfenv', 'pshear')]
    rng += [_range(pd, k, 1.0) for k in ('pranks', 'pranksv', 'pranksp', 'pranksr')]
    ranges = np.array(rng, dtype=np.float64).ravel()
    flags, dec = (C.c_int * 5)(), C.c_float()
    tc, ts = np.empty(128, np.uint16), np.empty(128, np.uint16)
    envelope_lib().env_tables(C.byref(p), ranges.ctypes.data_as(C.c_void_p), C.c_int(one_stage), flags, C.byref(dec),
                              tc.ctypes.data_as(C.c_void_p), ts.ctypes.data_as(C.c_void_p))
    f = dict(zip(('cent_ok', 'sat_ok', 'sat_basic', 'c_ok', 's_ok'), (bool(v) for v in flags)))
    kh = host_keys(hd['hmass'], hd['hmultis'], hd['hrandoms'])
    kp = host_keys(pd['phmass'], pd['pweights'], pd['prandoms'])
    pc = (kh >> 7).astype(np.int32) <= tc[kh & 127].astype(np.int32)
    ps = (kp >> 7).astype(np.int32) <= ts[kp & 127].astype(np.int32)
    return f, pc, ps
