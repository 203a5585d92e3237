"""Inputs of the exact NFW checks, shared by tests/test_oracle_nfw.py (the fragility cap, on the CPU) and
tests/test_nfw_exact_gpu.py (device against oracle): both must see the same catalogues, tracers, tables and seeds."""
import numpy as np

from abacusutils_amd import synth

TRACERS = ('LRG', 'ELG', 'QSO')
LBOX = 1000.0


def nfw_table(n=200000, cmax=12.0, seed=3):
    """draws of r/r_s from an NFW mass profile truncated at cmax (what abacusutils ships as NFW_draw)"""
    rng = np.random.default_rng(seed)
    x = np.linspace(0, cmax, 20001)
    mcum = np.log1p(x) - x / (1 + x)
    return np.interp(rng.random(n) * mcum[-1], mcum, x)


def catalogue(nh, seed, n_part=1000):
    """synthetic halos with concentrations uniform in 3 .. 9 and Rvir ~ M^(1/3)"""
    hd, pd, params = synth.synth_hod_inputs(nh, n_part, seed=seed, lbox=LBOX)
    rng = np.random.default_rng(seed + 1000)
    hd['hc'] = rng.uniform(3.0, 9.0, nh)
    hd['hrvir'] = 0.3 * (hd['hmass'] / 1e13) ** (1 / 3)
    return hd, pd, params


def cut(hd, pd, a, b):
    """halos [a, b) of a catalogue with their particles (`pinds` is non-decreasing), as a catalogue of its own"""
    lo, hi = np.searchsorted(pd['pinds'], [a, b])
    h = {k: np.ascontiguousarray(v[a:b]) for k, v in hd.items()}
    p = {k: np.ascontiguousarray(v[lo:hi]) for k, v in pd.items()}
    p['pinds'] = p['pinds'] - a
    return h, p


# assembly bias, conformity parameters away from their defaults (synth.PRODUCTION_TRACERS), distinct velocity factors
MIX = {'LRG': dict(synth.PRODUCTION_TRACERS['LRG'], f_sigv=0.8),
       'ELG': dict(synth.PRODUCTION_TRACERS['ELG'], f_sigv=1.1),
       'QSO': dict(synth.PRODUCTION_TRACERS['QSO'], f_sigv=0.5)}
assert MIX['ELG']['logM1_EE'] != MIX['ELG']['logM1'] != MIX['ELG']['logM1_EL'] and MIX['ELG']['alpha_EE'] != MIX['ELG']['alpha']

EXTENDED = dict(MIX, ELG=dict(MIX['ELG'], exp_frac=0.3, exp_scale=1.7, nfw_rescale=0.8))

# M1 lowered by 1.5 .. 3.9 dex: thousands of halos above the sampler switch at lam = 10, hundreds above 100
RICH = {'LRG': dict(MIX['LRG'], logM1=12.8),
        'ELG': dict(MIX['ELG'], logM1=11.0, logM1_EE=10.8, logM1_EL=11.2),
        'QSO': dict(MIX['QSO'], logM1=10.0, ic=0.5)}


def _case(name, nh, cat_seed, tracers, seed, draw=None, index0=0, edit=None):
    def make():
        hd, pd, params = catalogue(nh, cat_seed)
        if edit is not None:
            edit(hd)
        return dict(name=name, hd=hd, pd=pd, params=params, tracers=tracers, seed=seed, index0=index0,
                    draw=nfw_table() if draw is None else draw())
    make.__name__ = name
    return make


def _at_origin(hd):
    hd['hpos'] = np.zeros_like(hd['hpos'])
    hd['hvel'] = np.zeros_like(hd['hvel'])


def _no_satellites(hd):
    hd['hmass'] = np.full_like(hd['hmass'], 1e10)      # below kappa * M_cut of every tracer: lam = 0 everywhere


def _table_above_a_third():
    return np.random.default_rng(8).uniform(5.0, 12.0, 5000)   # no entry below 5: fallback for hc < 5, a third of 3 .. 9


def _one_entry():
    return np.array([6.0])


SUBSET_NH = (1, 255, 256, 257)

# every populate of tests/test_nfw_exact_gpu.py is one of these (name -> builder); sizes keep that file under a minute
CASES = {c.__name__: c for c in (
    _case('mix', 400000, 21, MIX, 12345),
    _case('extended', 200000, 22, EXTENDED, 2024),
    _case('rich', 50000, 23, RICH, 99),
    _case('fallback_third', 100000, 24, MIX, 31337, draw=_table_above_a_third),
    _case('fallback_one_entry', 100000, 24, MIX, 31338, draw=_one_entry),
    _case('offsets_only', 400000, 21, MIX, 12345, edit=_at_origin),
    _case('index_123457', 100000, 25, MIX, 777, index0=123457),
    _case('index_2p33', 100000, 25, MIX, 777, index0=2**33 + 5),
    _case('elg_only', 100000, 26, {'ELG': MIX['ELG']}, 5),
    _case('lrg_qso', 100000, 26, {'LRG': MIX['LRG'], 'QSO': MIX['QSO']}, 6),
    _case('no_f_sigv', 100000, 26, {k: {q: v for q, v in MIX[k].items() if q != 'f_sigv'} for k in MIX}, 7),
    _case('no_satellites', 20000, 27, MIX, 8, edit=_no_satellites),
    _case('small', 20000, 28, RICH, 9),          # the nh = 1, 255, 256, 257 catalogues are cuts of this one
)}
SHARD_CUTS = (0, 31337, 31338 + 40001, 100000)   # the index_* catalogue in three uneven pieces


def small_cut(case, nh, lam_elg):
    """`nh` consecutive halos of the `small` case, from the first start at which the first halo and the last halo of each
    of the sizes 255, 256, 257 all have an ELG mean of at least 1: the halos on either side of the 256-thread block
    boundary of the count kernel hold satellites"""
    ok = lam_elg >= 1.0
    n = len(ok) - max(SUBSET_NH)
    a = int(np.nonzero(ok[:n] & ok[254:n + 254] & ok[255:n + 255] & ok[256:n + 256])[0][0])
    hd, pd = cut(case['hd'], case['pd'], a, a + nh)
    return a, dict(case, hd=hd, pd=pd)
