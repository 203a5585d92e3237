"""NFW satellites of the device (`hod_nfw_count`, `hod_nfw_emit` behind abacus_hod_populate_nfw) against the oracle's
restatement, satellite by satellite.  The kernels are a pure function of (seed, global halo index, tracer, satellite rank)
through counter-based Philox streams, so nothing here is statistical (the statistical link reference -> oracle is
tests/test_oracle_nfw.py; the inputs are tests/nfw_cases.py, whose fragility cap is checked there on the CPU):

counts   equal to oracle.nfw_counts at every (halo, tracer) the oracle does not flag as fragile (a comparison of the draw
         decided by less than 2^-36 relative: the device's and glibc's math libraries may round it either way);
exact    `id`, `mass` bit-equal, satellites in halo order, centrals bit-equal to the particle path;
values   err = max |device - oracle_longdouble| / scale over ALL satellites, scale = |hpos component| + r for x, y, z and
         |hvel component| + sig for the velocities (z under RSD: circular difference modulo Lbox), against
         e_ref = the same measure of the oracle's own double evaluation: err <= 4 e_ref, the margin of profiles/zcv - the
         chain composes four or five library calls, each within a few ulp on the device against <= 1 in glibc.
         Printed per case and column with -s; the record of a run is profiles/nfw/README.md."""
import warnings

import numpy as np
import pytest

import nfw_cases
from oracle import oracle

pytestmark = pytest.mark.gpu

TR = oracle.TRACERS
VALUE_COLS = ('x', 'y', 'z', 'vx', 'vy', 'vz')
MARGIN = 4.0


@pytest.fixture(scope='module')
def G():
    from abacusutils_amd.hod import GRAND_HOD
    return GRAND_HOD


_cache = {}


def get_case(name):
    """the cases are built once per module (the catalogue of 400 000 halos takes longer than its populate)"""
    if name not in _cache:
        _cache[name] = nfw_cases.CASES[name]()
    return _cache[name]


def device_run(G, case, rsd, staged=None, through_gen_gal_cat=False):
    """one populate; returns (Ncent[3], Nsat[3], {tracer: columns} for all three tracers, keep_cent)"""
    hd, pd, tracers = case['hd'], case['pd'], case['tracers']
    st = staged if staged is not None else G.StagedCatalog(hd, pd)
    try:
        if through_gen_gal_cat:
            assert case['index0'] == 0
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                mock = G.gen_gal_cat(hd, pd, tracers, case['params'], rsd=rsd, nfw=case['seed'], NFW_draw=case['draw'], staged=st)
            ncent, nsat = st.counts[:3].copy(), st.counts[3:].copy()
            cats = {tr: dict(mock[tr]) for tr in tracers}
        else:
            p = G.marshal_params(tracers, case['params'], False, rsd)
            ncent, nsat = st.populate_nfw(p, tracers, hd, case['draw'], case['seed'], halo_index0=case['index0'])
            cats = {tr: st.fetch(tr) for tr in tracers}
        for tr in TR:
            if tr not in tracers:   # a tracer that was not asked for: nothing emitted, nothing to fetch
                t = TR.index(tr)
                assert ncent[t] == 0 and nsat[t] == 0, (tr, ncent, nsat)
        for tr in tracers:
            t = TR.index(tr)
            assert cats[tr]['Ncent'] == ncent[t] and len(cats[tr]['x']) == ncent[t] + nsat[t]
        kc, _ = st.fetch_keep()
    finally:
        if staged is None:
            st.free()
    return ncent, nsat, cats, kc


def hosts_and_ranks(hd, ids):
    """host halo (local index) and rank within it of every satellite, from the host ids; asserts the halo order"""
    hid = np.asarray(hd['hid'])
    assert np.all(np.diff(hid) > 0)
    h = np.searchsorted(hid, ids)
    assert np.all(h < len(hid)) and np.array_equal(hid[h], ids)
    assert np.all(np.diff(h) >= 0), 'satellites are not emitted in halo order'
    n_per = np.bincount(h, minlength=len(hid))
    rank = np.arange(len(h)) - np.repeat(np.cumsum(n_per) - n_per, n_per)
    return h, rank, n_per


def scaled_error(got, want_l, scale, circular=None):
    d = np.abs(np.asarray(got, dtype=np.longdouble) - want_l)
    if circular is not None:
        d = np.minimum(d, np.abs(np.longdouble(circular) - d))
    zero = scale == 0
    assert not d[zero].any()                       # nothing to scale by: the value is the host's, exactly
    return float((d[~zero] / scale[~zero]).max()) if (~zero).any() else 0.0


def check_against_oracle(case, rsd, ncent, nsat, cats, kc, label):
    """counts, exact columns and value columns of one device run; returns the oracle's (counts, lam, branches)"""
    hd, tracers, params = case['hd'], case['tracers'], case['params']
    counts, lam, fragile = oracle.nfw_counts(hd, tracers, params, kc, case['seed'], case['index0'])
    assert fragile.mean() <= 1e-5
    L = params['Lbox']
    branches = {}
    for tr in tracers:
        t = TR.index(tr)
        c = cats[tr]
        nc = c['Ncent']
        ids = c['id'][nc:]
        h, rank, n_dev = hosts_and_ranks(hd, ids)
        assert n_dev.sum() == nsat[t] == len(c['x']) - nc
        bad = np.nonzero((n_dev != counts[t]) & ~fragile[t])[0]
        assert len(bad) == 0, (f'{label} {tr}: {len(bad)} halos with a wrong number of satellites; first: halo {bad[0]} '
                               f'(global {case["index0"] + bad[0]}), device {n_dev[bad[0]]}, oracle {counts[t][bad[0]]}, '
                               f'lam {lam[t][bad[0]]!r}')
        if not fragile[t].any():
            assert nsat[t] == counts[t].sum()
        ref = oracle.nfw_satellites(hd, tracers, params, case['draw'], case['seed'], t, h, rank, rsd, case['index0'])
        branches[tr] = ref['branch']
        np.testing.assert_array_equal(c['id'][nc:], ref['double']['id'])
        np.testing.assert_array_equal(c['mass'][nc:], ref['double']['mass'])
        if rsd and len(h):
            assert c['z'][nc:].min() >= 0 and c['z'][nc:].max() <= L
        if oracle.ldbl_mant_dig() < 64:
            print(f'{label} {tr}: long double is no wider than double here - the ulp tier is skipped')
            continue
        for q, col in enumerate(VALUE_COLS):
            base = hd['hpos'][h, q] if q < 3 else hd['hvel'][h, q - 3]
            scale = np.abs(base) + (ref['r'] if q < 3 else ref['sig'])
            circ = L if (rsd and col == 'z') else None
            err = scaled_error(c[col][nc:], ref['longdouble'][col], scale, circ)
            e_ref = scaled_error(ref['double'][col], ref['longdouble'][col], scale, circ)
            ratio = err / e_ref if e_ref > 0 else (0.0 if err == 0 else np.inf)
            print(f'NFW {label:28s} {tr} {col:2s} n={len(h):8d} err={err:.3e} e_ref={e_ref:.3e} ratio={ratio:.2f}')
            assert err <= MARGIN * e_ref, (label, tr, col, err, e_ref, ratio)
    return counts, lam, branches


def check_centrals(G, case, rsd, cats):
    plain = G.gen_gal_cat(case['hd'], case['pd'], case['tracers'], case['params'], rsd=rsd)   # particle path: same centrals
    for tr in case['tracers']:
        nc = cats[tr]['Ncent']
        assert nc == plain[tr]['Ncent']
        for k in VALUE_COLS + ('mass', 'id'):
            np.testing.assert_array_equal(cats[tr][k][:nc], plain[tr][k][:nc])


@pytest.mark.parametrize('rsd', [False, True])
def test_mix(G, rsd):
    """LRG + ELG + QSO with assembly bias and conformity parameters off their defaults, through gen_gal_cat"""
    case = get_case('mix')
    ncent, nsat, cats, kc = device_run(G, case, rsd, through_gen_gal_cat=True)
    _, lam, _ = check_against_oracle(case, rsd, ncent, nsat, cats, kc, f'mix rsd={int(rsd)}')
    check_centrals(G, case, rsd, cats)
    assert set(np.unique(kc[lam[1] > 0])) >= {0, 1, 2}       # every conformity branch of the ELG mean
    assert all(nsat[t] >= 50 for t in range(3))              # no tracer's comparison is vacuous


def test_extended_profile(G):
    """exp_frac = 0.3, exp_scale = 1.7, nfw_rescale = 0.8 (taken from the ELG dict for every tracer)"""
    case = get_case('extended')
    ncent, nsat, cats, kc = device_run(G, case, True)
    _, _, branches = check_against_oracle(case, True, ncent, nsat, cats, kc, 'extended')
    br = np.concatenate(list(branches.values()))
    assert (br == 1).mean() >= 0.1 and (br == 0).mean() >= 0.1 and not (br == 2).any()


def test_rich(G):
    """Thousands of halos above the sampler switch at lam = 10, and the capacity-growth path: the first populate of a
    fresh StagedCatalog emits more galaxies than the buffers staging allocates, (n_halo + n_part) / 64 per tracer
    (abacus_hod_stage).  That capacity is not readable through the ABI; the assertion below restates the formula."""
    case = get_case('rich')
    st = G.StagedCatalog(case['hd'], case['pd'])
    try:
        ncent, nsat, cats, kc = device_run(G, case, False, staged=st)
        initial = (st.n_halo + st.n_part) // 64
        assert all(ncent[t] + nsat[t] > initial for t in range(3)), (ncent, nsat, initial)
        _, lam, _ = check_against_oracle(case, False, ncent, nsat, cats, kc, 'rich (grown)')
        assert (lam[1] >= 10).sum() >= 2000 and (lam > 100).any(axis=0).sum() > 0
        assert (np.abs(lam[1] - 10) <= 0.5).sum() >= 100
        check_centrals(G, case, False, cats)                 # the centrals were emitted again into the grown buffers
        again = device_run(G, case, False, staged=st)        # second call: no growth, same catalogue
        for tr in case['tracers']:
            for k in VALUE_COLS + ('mass', 'id'):
                np.testing.assert_array_equal(again[2][tr][k], cats[tr][k])
    finally:
        st.free()


@pytest.mark.parametrize('name', ['fallback_third', 'fallback_one_entry'])
def test_fallback(G, name):
    """tables without an entry below the concentration of many halos: 256 rejected probes, then d = c * uniform"""
    case = get_case(name)
    ncent, nsat, cats, kc = device_run(G, case, False)
    _, _, branches = check_against_oracle(case, False, ncent, nsat, cats, kc, name)
    for tr, br in branches.items():
        c = cats[tr]
        nc = c['Ncent']
        h, _, _ = hosts_and_ranks(case['hd'], c['id'][nc:])
        fb = br == 2
        assert 0.2 < fb.mean() < 0.6, (tr, fb.mean())
        below = case['hd']['hc'][h] < case['draw'].min()     # no admissible entry at all (a halo just above may also run out of probes)
        assert np.all(fb[below]) and below.mean() > 0.2
        r = np.linalg.norm(np.stack([c[k][nc:] for k in 'xyz'], 1) - case['hd']['hpos'][h], axis=1)
        assert np.all(r[fb] > 0) and np.all(r[fb] <= case['hd']['hrvir'][h[fb]] * (1 + 1e-9))


@pytest.mark.parametrize('rsd', [False, True])
def test_offsets_only(G, rsd):
    """the mix with every halo at rest at the origin: the scale is r and sig alone, the comparison sees the trigonometric and
    logarithm chain itself instead of the final rounding against a coordinate of order 1000"""
    case = get_case('offsets_only')
    ncent, nsat, cats, kc = device_run(G, case, rsd)
    check_against_oracle(case, rsd, ncent, nsat, cats, kc, f'offsets only rsd={int(rsd)}')


@pytest.mark.parametrize('name', ['index_123457', 'index_2p33'])
def test_global_index(G, name):
    """halo_index0 != 0 against the oracle, and the sharding invariance the kernel promises: the catalogue cut at two uneven
    points, each piece staged on its own with the matching halo_index0, emits the single run's satellites bit for bit"""
    case = get_case(name)
    ncent, nsat, cats, kc = device_run(G, case, True)
    check_against_oracle(case, True, ncent, nsat, cats, kc, name)
    base = dict(case, index0=0)
    other = device_run(G, base, True)
    assert any(not np.array_equal(other[2][tr]['id'], cats[tr]['id']) for tr in case['tracers'])   # the index is used
    pieces = []
    cuts = nfw_cases.SHARD_CUTS
    for a, b in zip(cuts[:-1], cuts[1:]):
        hd, pd = nfw_cases.cut(case['hd'], case['pd'], a, b)
        sub = dict(case, hd=hd, pd=pd, index0=case['index0'] + a)
        n_c, n_s, cat, kcs = device_run(G, sub, True)
        np.testing.assert_array_equal(kcs, kc[a:b])
        check_against_oracle(sub, True, n_c, n_s, cat, kcs, f'{name} [{a}:{b})')
        pieces.append(cat)
    for tr in case['tracers']:
        nc = cats[tr]['Ncent']
        for k in VALUE_COLS + ('mass', 'id'):
            joined = np.concatenate([pc[tr][k][pc[tr]['Ncent']:] for pc in pieces])
            np.testing.assert_array_equal(joined, cats[tr][k][nc:], err_msg=f'{tr}.{k}')


@pytest.mark.parametrize('name', ['elg_only', 'lrg_qso'])
def test_tracer_subsets(G, name):
    """a tracer that is not asked for gets no galaxy (device_run asserts its counts are zero)"""
    case = get_case(name)
    ncent, nsat, cats, kc = device_run(G, case, False)
    check_against_oracle(case, False, ncent, nsat, cats, kc, name)
    check_centrals(G, case, False, cats)
    assert set(cats) == set(case['tracers']) and all(nsat[TR.index(tr)] > 0 for tr in case['tracers'])


def test_without_f_sigv_the_satellites_move_with_their_halo(G):
    case = get_case('no_f_sigv')
    ncent, nsat, cats, kc = device_run(G, case, False)
    check_against_oracle(case, False, ncent, nsat, cats, kc, 'no f_sigv')
    for tr in case['tracers']:
        c = cats[tr]
        nc = c['Ncent']
        h, _, _ = hosts_and_ranks(case['hd'], c['id'][nc:])
        assert len(h) >= 50
        for q, k in enumerate(('vx', 'vy', 'vz')):
            np.testing.assert_array_equal(c[k][nc:], case['hd']['hvel'][h, q])


@pytest.mark.parametrize('nh', nfw_cases.SUBSET_NH)
def test_degenerate_sizes(G, nh):
    """one halo, and catalogues one below, at and one above the block size of the count kernel"""
    whole = get_case('small')
    kc = device_run(G, whole, False)[3]
    lam = oracle.nfw_counts(whole['hd'], whole['tracers'], whole['params'], kc, whole['seed'])[1]
    a, case = nfw_cases.small_cut(whole, nh, lam[1])
    ncent, nsat, cats, kcs = device_run(G, case, True)
    np.testing.assert_array_equal(kcs, kc[a:a + nh])
    check_against_oracle(case, True, ncent, nsat, cats, kcs, f'nh={nh}')
    assert nsat.sum() > 0


def test_no_satellites_anywhere(G):
    """every mean is zero: the call succeeds and emits centrals only"""
    case = get_case('no_satellites')
    ncent, nsat, cats, kc = device_run(G, case, True)
    assert not nsat.any()
    counts, lam, _ = check_against_oracle(case, True, ncent, nsat, cats, kc, 'no satellites')
    assert not lam.any() and not counts.any()
    check_centrals(G, case, True, cats)
