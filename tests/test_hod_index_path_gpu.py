"""The queue-free index path of the sparse mixes (hod_exact_index -> hod_emit_bm): kept bitmaps alternating by populate
parity, lazy keep masks cleared by the emission, totals written straight into mapped host memory.  Every populate is held
to the CPU oracle and to the three-launch comparator (`hod_deal` = 1); the kernels a populate launched are read off the
library's profiler so that each case provably runs the path it is about."""
import numpy as np
import pytest
from conftest import assert_mock_equal

from abacusutils_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def G():
    from abacusutils_amd.hod import GRAND_HOD
    return GRAND_HOD


def _lrg(lc):
    return {'LRG': dict(synth.LRG_PARAMS, logM_cut=lc, logM1=lc + 0.9)}


def _populate(G, st, tracers, params):
    """one populate; returns (counts, keep_cent, keep_sat, catalogue, {kernel: launches})"""
    from abacusutils_amd import _lib
    p = G.marshal_params(tracers, params, False, True)
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


def _queue_free(launches):
    return launches.get('hod_exact', 0) >= 1 and 'hod_deal' not in launches and 'hod_filter' not in launches


def _check_oracle(hd, pd, tracers, params, got, err_msg):
    from oracle import oracle
    counts, kc, ks, mock, _ = got
    want, wkc, wks = oracle.gen_gal_cat(hd, pd, tracers, params, Nthread=oracle.max_threads(), enable_ranks=False, rsd=True,
                                        return_keep=True)
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


def test_c2_moving_kept_set_matches_oracle_and_deal_path(G, options):
    """C2 size, one staged catalogue per path, logM_cut changing every populate so that the kept set moves: after each
    populate the keep masks and the catalogue equal the oracle's and the three-launch path's"""
    n = 10_000_000
    hd, pd, params = synth.synth_hod_inputs(n, n, seed=600)
    new, old = G.StagedCatalog(hd, pd), G.StagedCatalog(hd, pd)
    seq = [13.3, 13.3, 13.5, 13.15, 13.4, 13.3]
    try:
        for step, lc in enumerate(seq):
            tracers = _lrg(lc)
            options.set('hod_deal', 1)
            b = _populate(G, old, tracers, params)
            options.set('hod_deal', 0)
            a = _populate(G, new, tracers, params)
            if step >= 1:   # the key index is built by the second populate on unchanged keys
                assert _queue_free(a[4]), a[4]
                assert 'hod_deal' in b[4] or step == 1, b[4]
            _check_same(a, b, f'step {step}: logM_cut {lc}')
            if step >= 1:
                _check_oracle(hd, pd, tracers, params, a, f'step {step}: logM_cut {lc}')
    finally:
        new.free()
        old.free()


def test_capacity_growth_inside_the_index_path(G):
    """a populate of the queue-free path that emits more rows than the catalogue buffers hold: the buffers grow and the
    re-emission (abacus_hod_counts) finds its bitmaps and counts intact"""
    hd, pd, params = synth.synth_hod_inputs(300_000, 300_000, seed=3)
    st = G.StagedCatalog(hd, pd)
    try:
        for lc in (14.5, 14.5, 12.6, 12.6, 14.5):
            got = _populate(G, st, _lrg(lc), params)
            _check_oracle(hd, pd, _lrg(lc), params, got, f'logM_cut {lc}')
        assert _queue_free(got[4]), got[4]
        st.populate(G.marshal_params(_lrg(12.6), params, False, True))
        got = _populate(G, st, _lrg(12.3), params)   # 40 000 rows against ~21 000 of capacity
        assert _queue_free(got[4]) and got[4].get('hod_emit', 0) >= 2, got[4]
        _check_oracle(hd, pd, _lrg(12.3), params, got, 'growth')
    finally:
        st.free()


def test_index_path_then_key_filter_then_index_path(G, options):
    """leaving the queue-free path for the streaming key filter and coming back leaves no stale keep byte or bit"""
    hd, pd, params = synth.synth_hod_inputs(250_000, 350_000, seed=21)
    st = G.StagedCatalog(hd, pd)
    try:
        steps = [(13.0, 0), (13.0, 0), (12.7, 0), (13.2, 1), (12.9, 1), (13.1, 0), (12.8, 0), (12.8, 0)]
        for lc, noindex in steps:
            options.set('hod_noindex', noindex)
            got = _populate(G, st, _lrg(lc), params)
            if noindex:
                assert 'hod_filter' in got[4], got[4]
            _check_oracle(hd, pd, _lrg(lc), params, got, f'logM_cut {lc}, hod_noindex {noindex}')
        assert _queue_free(got[4]), got[4]
    finally:
        st.free()


def test_candidate_free_step(G):
    """thresholds above every mass: (next to) no candidate; the emission still un-keeps every object the previous populate
    kept and reports the totals, and the next populate is exact again"""
    hd, pd, params = synth.synth_hod_inputs(250_000, 350_000, seed=22)
    st = G.StagedCatalog(hd, pd)
    try:
        for lc in (12.9, 12.9, 20.0, 12.8, 20.0, 20.0, 13.0):
            got = _populate(G, st, _lrg(lc), params)
            if lc == 20.0:
                assert 'hod_deal' not in got[4] and 'hod_filter' not in got[4], got[4]
                assert got[0][0].sum() + got[0][1].sum() <= 2
            _check_oracle(hd, pd, _lrg(lc), params, got, f'logM_cut {lc}')
        assert _queue_free(got[4]), got[4]
    finally:
        st.free()


def test_4e7_matches_deal_path(G, options):
    """4e7 halos + 4e7 particles: the queue-free path and the three-launch path give the same keep masks, counts and
    catalogue over populates whose kept set moves"""
    n = 40_000_000
    hd, pd, params = synth.synth_hod_inputs(n, n, seed=605)
    new, old = G.StagedCatalog(hd, pd), G.StagedCatalog(hd, pd)
    try:
        for step, lc in enumerate((13.3, 13.3, 13.45, 13.2)):
            options.set('hod_deal', 1)
            b = _populate(G, old, _lrg(lc), params)
            options.set('hod_deal', 0)
            a = _populate(G, new, _lrg(lc), params)
            if step >= 1:
                assert _queue_free(a[4]), a[4]
            _check_same(a, b, f'step {step}: logM_cut {lc}')
        assert 'hod_deal' in b[4], b[4]
        assert a[0][0][0] > 100_000
    finally:
        new.free()
        old.free()
