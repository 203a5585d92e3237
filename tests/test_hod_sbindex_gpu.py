"""Sparse mixes on unchanged keys from the per-superblock key index: hod_exact (hod_exact_sbidx: the candidates of a superblock
read off its own `cum` / `sidx`) followed by hod_emit over the kept lists, two launches and no look-back.  Every populate is
held exactly to the CPU oracle (counts, both keep masks, the whole catalogue) or byte for byte to a comparator on the same
staged catalogue (`hod_sbindex` = 1: the bitmap path; `hod_deal` = 1: the tile queues); the kernels a populate launched are
read off the library's profiler so that each case provably runs the path it is about."""
import numpy as np
import pytest
from conftest import assert_mock_equal

from abacusutils_amd import synth

pytestmark = pytest.mark.gpu

STAGING = ('hod_index_keys', 'hod_index_sort', 'hod_index_last')


@pytest.fixture(scope='module')
def G():
    from abacusutils_amd.hod import GRAND_HOD
    return GRAND_HOD


def _lrg(lc, sigma=0.3, **kw):
    return {'LRG': dict(synth.LRG_PARAMS, logM_cut=lc, logM1=lc + 0.9, sigma=sigma, **kw)}


def _inputs(nh, npart, seed):
    """synthetic inputs (staged halos, staged particles, params, the oracle's halos, the oracle's particles); without halos:
    the particles of a catalogue whose halos are not staged, nor their host index - the oracle keeps both"""
    if nh > 0:
        hd, pd, params = synth.synth_hod_inputs(nh, npart, seed=seed)
        return hd, pd, params, hd, pd
    hd, pd, params = synth.synth_hod_inputs(1000, npart, seed=seed)
    return ({k: v[:0].copy() for k, v in hd.items()}, {k: v for k, v in pd.items() if k != 'pinds'}, params, hd, pd)


def _populate(G, st, tracers, params, enable_ranks=False):
    """one populate; returns (counts, keep_cent, keep_sat, catalogue, {kernel: launches})"""
    from abacusutils_amd import _lib
    p = G.marshal_params(tracers, params, enable_ranks, True)
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        ncent, nsat = st.populate(p)
    finally:
        _lib.profile_enable(False)
    launches = {k: n for k, (ms, n) in _lib.profile_get().items() if n}
    _lib.profile_reset()
    kc, ks = st.fetch_keep()
    return (np.asarray(ncent), np.asarray(nsat)), kc, ks, {tr: st.fetch(tr) for tr in tracers}, launches


def _new_path(launches):
    return (launches.get('hod_exact', 0) >= 1 and launches.get('hod_emit', 0) >= 1 and 'hod_deal' not in launches
            and 'hod_filter' not in launches)


def _check_oracle(hd, pd, tracers, params, got, err_msg, enable_ranks=False, sats_only=False):
    """`sats_only`: the halos were not staged - the satellites (LRG alone: they do not depend on the centrals) are the
    oracle's, the centrals none"""
    from oracle import oracle
    counts, kc, ks, mock, _ = got
    want, wkc, wks = oracle.gen_gal_cat(hd, pd, tracers, params, Nthread=oracle.max_threads(), enable_ranks=enable_ranks,
                                        rsd=True, return_keep=True)
    if sats_only:
        assert kc.size == 0 and list(tracers) == ['LRG']
        nc = int(want['LRG']['Ncent'])
        want = {'LRG': dict({c: np.asarray(v)[nc:] for c, v in want['LRG'].items() if c != 'Ncent'}, Ncent=0)}
    else:
        np.testing.assert_array_equal(kc, wkc, err_msg=err_msg)
    np.testing.assert_array_equal(ks, wks, err_msg=err_msg)
    for tr in tracers:
        assert counts[0][0] == want[tr]['Ncent'], err_msg
    assert_mock_equal(mock, want, exact=True)


def _check_same(a, b, err_msg):
    np.testing.assert_array_equal(a[0][0], b[0][0], err_msg=err_msg)
    np.testing.assert_array_equal(a[0][1], b[0][1], err_msg=err_msg)
    np.testing.assert_array_equal(a[1], b[1], err_msg=err_msg)
    np.testing.assert_array_equal(a[2], b[2], err_msg=err_msg)
    assert_mock_equal(a[3], b[3], exact=True)


@pytest.mark.parametrize('nh,npart', [(32767, 32769), (32768, 32768), (5, 70_000), (300_001, 299_999), (250_000, 0),
                                      (0, 250_000)])
def test_catalogue_shapes(G, options, nh, npart):
    """one superblock against two with a boundary object on either side, sizes that are no multiple of the 2048-object tile,
    a kind without superblocks: repeated populates against the oracle, then once more through the bitmap path"""
    hd, pd, params, ohd, opd = _inputs(nh, npart, 41)
    st = G.StagedCatalog(hd, pd)
    try:
        for step, lc in enumerate((13.0, 13.0, 12.8, 13.2)):
            got = _populate(G, st, _lrg(lc), params)
            _check_oracle(ohd, opd, _lrg(lc), params, got, f'({nh}, {npart}) step {step}: logM_cut {lc}', sats_only=nh == 0)
            if step >= 1:   # the indices are built by the second populate on unchanged keys
                assert _new_path(got[4]), got[4]
            if step == 1:
                assert all(k in got[4] for k in STAGING), got[4]
            if step >= 2:
                assert not any(k in got[4] for k in STAGING), got[4]
        options.set('hod_sbindex', 1)
        cmp_ = _populate(G, st, _lrg(13.2), params)
        _check_same(got, cmp_, f'({nh}, {npart}): against hod_sbindex = 1')
        options.set('hod_sbindex', 0)
        again = _populate(G, st, _lrg(13.2), params)
        assert _new_path(again[4]), again[4]
        _check_same(again, cmp_, f'({nh}, {npart}): back from hod_sbindex = 1')
    finally:
        st.free()


def test_crowded_and_empty_superblocks(G):
    """a superblock with more candidates than threads and superblocks with none in the same populate, then thresholds above
    every mass (hod_emit still launched, next to nothing kept), then the crowded populate again"""
    n = 300_000
    hd, pd, params = synth.synth_hod_inputs(n, n, seed=42)
    sb = 16 * 2048
    for d, col in ((hd, 'hmass'), (pd, 'phmass')):   # superblocks 2 and 5 of both kinds: below every threshold
        d[col][2 * sb:3 * sb] = 10 ** 10.0
        d[col][5 * sb:6 * sb] = 10 ** 10.0
    st = G.StagedCatalog(hd, pd)
    try:
        for step, lc in enumerate((12.3, 12.3, 20.0, 12.3)):
            got = _populate(G, st, _lrg(lc), params)
            _check_oracle(hd, pd, _lrg(lc), params, got, f'step {step}: logM_cut {lc}')
            if step >= 1:
                assert _new_path(got[4]), got[4]
                cand = st.candidates()
            if lc == 20.0:
                assert got[0][0].sum() + got[0][1].sum() <= 2
            elif step >= 1:
                assert cand[0] > 256 * 10 and cand[1] > 256 * 10, cand   # ten superblocks a kind: some hold more than 256
                assert not got[1][2 * sb:3 * sb].any() and not got[2][5 * sb:6 * sb].any()
    finally:
        st.free()


def test_unkeep_of_shrinking_growing_and_moving_kept_sets(G):
    """kept sets that shrink, grow and move between superblocks: the keep masks are exact after every populate"""
    n = 300_000
    hd, pd, params = synth.synth_hod_inputs(n, n, seed=43)
    sb = 16 * 2048
    lo, hi = 3 * sb + 1000, 3 * sb + 5000   # inside superblock 3 of both kinds
    hd['hmass'] = np.minimum(hd['hmass'], 10 ** 14.3)
    hd['hmass'][lo:hi] = 10 ** 15.5
    pd['phmass'] = np.minimum(pd['phmass'], 10 ** 14.3)
    pd['phmass'][lo:hi] = 10 ** 15.5
    st = G.StagedCatalog(hd, pd)
    try:
        seq = [(13.3, 0.3), (13.3, 0.3), (13.6, 0.3), (12.9, 0.3), (15.4, 0.05), (13.1, 0.3), (15.4, 0.05), (15.45, 0.05),
               (13.3, 0.3)]
        for step, (lc, sigma) in enumerate(seq):
            got = _populate(G, st, _lrg(lc, sigma), params)
            _check_oracle(hd, pd, _lrg(lc, sigma), params, got, f'step {step}: logM_cut {lc}')
            if step >= 1:
                assert _new_path(got[4]), got[4]
            if sigma < 0.1:   # only objects of one superblock can be kept
                kept_c, kept_s = np.flatnonzero(got[1]), np.flatnonzero(got[2])
                assert kept_c.size > 100 and kept_s.size > 0, (kept_c.size, kept_s.size)
                assert kept_c.min() >= lo and kept_c.max() < hi and kept_s.min() >= lo and kept_s.max() < hi
    finally:
        st.free()


def test_path_changes_on_one_catalogue(G, options):
    """the per-superblock path, the bitmap path and the tile-queue path alternate from populate to populate on one staged
    catalogue: each hands the next keep masks it must clear, and all give what a second catalogue that stays on one path gives"""
    hd, pd, params = synth.synth_hod_inputs(300_000, 300_000, seed=44)
    st, ref = G.StagedCatalog(hd, pd), G.StagedCatalog(hd, pd)
    try:
        seq = [(13.0, 0, 0), (13.0, 0, 0), (12.8, 1, 0), (13.2, 0, 0), (12.9, 0, 1), (13.1, 0, 0), (12.7, 1, 1), (13.3, 1, 0),
               (12.9, 0, 1), (12.9, 0, 1), (13.05, 0, 0), (13.0, 1, 0), (12.85, 0, 0)]
        for step, (lc, sbindex, deal) in enumerate(seq):
            options.set('hod_sbindex', 0)
            options.set('hod_deal', 0)
            want = _populate(G, ref, _lrg(lc), params)
            options.set('hod_sbindex', sbindex)
            options.set('hod_deal', deal)
            got = _populate(G, st, _lrg(lc), params)
            _check_same(got, want, f'step {step}: logM_cut {lc}, hod_sbindex {sbindex}, hod_deal {deal}')
            if step >= 1:
                assert _new_path(want[4]), want[4]
                if not sbindex and not deal:
                    assert _new_path(got[4]), got[4]
                if deal:
                    assert 'hod_deal' in got[4] or 'hod_filter' in got[4], got[4]
            if step in (4, 8, 12):
                _check_oracle(hd, pd, _lrg(lc), params, got, f'step {step}: oracle')
    finally:
        st.free()
        ref.free()


def test_fallback_to_the_streaming_filter_and_back(G):
    """a dense threshold set (more than an eighth of the objects are candidates) streams the keys; the sparse populates
    around it run from the index, and no keep byte of either survives into the other"""
    hd, pd, params = synth.synth_hod_inputs(250_000, 350_000, seed=45)
    st = G.StagedCatalog(hd, pd)
    try:
        fell = 0
        for step, lc in enumerate((13.0, 13.0, 12.8, 10.5, 13.1, 10.5, 10.6, 12.9)):
            got = _populate(G, st, _lrg(lc), params)
            _check_oracle(hd, pd, _lrg(lc), params, got, f'step {step}: logM_cut {lc}')
            if lc < 11:
                cand = st.candidates()
                assert cand[0] + cand[1] > (250_000 + 350_000) // 8, cand
                assert 'hod_filter' in got[4], got[4]
                fell += 1
            elif step >= 1:
                assert _new_path(got[4]), got[4]
        assert fell == 3
    finally:
        st.free()


def test_index_invalidation(G, options):
    """a reseed, then an update of a random column: the indices are rebuilt by the second populate behind each and the
    results follow the new randoms; a change of the superblock layout between populates rebuilds the index or declines the path"""
    hd, pd, params = synth.synth_hod_inputs(200_000, 300_000, seed=46)
    st = G.StagedCatalog(hd, pd)
    try:
        for lc in (13.0, 13.0, 12.9):
            got = _populate(G, st, _lrg(lc), params)
        assert _new_path(got[4]), got[4]
        st.reseed(7, hsigma3d=hd['hsigma3d'])
        hd = dict(hd, hrandoms=st.fetch_field('hrandoms'), hveldev=st.fetch_field('hveldev').reshape(-1, 3))
        pd = dict(pd, prandoms=st.fetch_field('prandoms'))
        rng = np.random.default_rng(5)
        pd['prandoms'] = rng.random(len(pd['prandoms']))
        st.update('prandoms', pd['prandoms'])
        for step, lc in enumerate((12.9, 13.1, 12.8)):
            got = _populate(G, st, _lrg(lc), params)
            _check_oracle(hd, pd, _lrg(lc), params, got, f'after reseed + update, step {step}')
            if step == 0:
                assert 'hod_filter' in got[4], got[4]
            if step == 1:
                assert all(k in got[4] for k in STAGING) and _new_path(got[4]), got[4]
            if step == 2:
                assert _new_path(got[4]) and not any(k in got[4] for k in STAGING), got[4]
        for step, (opt, val, lc) in enumerate((('hod_sbtiles', 8, 13.0), ('hod_sbtiles', 8, 12.9), ('hod_sbtiles', 0, 13.1),
                                               ('hod_nobalance', 1, 12.8), ('hod_sbtiles', 8, 13.0), ('hod_nobalance', 0, 12.9),
                                               ('hod_sbtiles', 0, 13.2), ('hod_sbtiles', 0, 12.8))):
            options.set(opt, val)
            got = _populate(G, st, _lrg(lc), params)
            _check_oracle(hd, pd, _lrg(lc), params, got, f'layout step {step}: {opt} = {val}')
        assert _new_path(got[4]), got[4]
    finally:
        st.free()


def test_repeated_capacity_growth(G):
    """populates that outgrow the catalogue buffers several times: each re-emission is hod_emit alone on the kept lists"""
    hd, pd, params = synth.synth_hod_inputs(400_000, 400_000, seed=47)
    st = G.StagedCatalog(hd, pd)
    try:
        grew = 0
        for lc in (14.8, 14.8, 14.0, 13.2, 14.8, 12.6, 12.3, 14.8, 12.3):
            got = _populate(G, st, _lrg(lc), params)
            _check_oracle(hd, pd, _lrg(lc), params, got, f'logM_cut {lc}')
            if _new_path(got[4]) and got[4].get('hod_emit', 0) >= 2:
                assert got[4]['hod_exact'] == 1, got[4]
                grew += 1
        assert _new_path(got[4]), got[4]
        assert grew >= 2, grew
    finally:
        st.free()


def test_rank_parameters(G):
    """enable_ranks with staged ranks and non-zero LRG rank parameters: the candidates read their ranks from the record"""
    hd, pd, params = synth.synth_hod_inputs(200_000, 300_000, seed=48, with_ranks=True)
    st = G.StagedCatalog(hd, pd)
    try:
        for step, lc in enumerate((13.0, 13.0, 12.8, 13.1)):
            tracers = _lrg(lc, s=0.3, s_v=-0.2, s_p=0.15, s_r=-0.1)
            got = _populate(G, st, tracers, params, enable_ranks=True)
            _check_oracle(hd, pd, tracers, params, got, f'step {step}: logM_cut {lc}', enable_ranks=True)
            if step >= 1:
                assert _new_path(got[4]), got[4]
        assert got[0][1].sum() > 100
    finally:
        st.free()
