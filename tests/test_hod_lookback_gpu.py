"""Output offsets of the queue-free index path by decoupled look-back (hod_emit_bm): the superblocks publish their popcount
aggregates and inclusive prefixes as tagged status words, and the last superblock writes the totals.  Every populate is held to the CPU oracle or to the three-launch comparator (`hod_deal` = 1), the latter on the
same staged catalogue so that the two paths alternate; the kernels a populate launched are read off the library's
profiler so that each case provably runs the path it is about."""
import numpy as np
import pytest
from conftest import assert_mock_equal

from abacusutils_amd import synth

pytestmark = pytest.mark.gpu

SB_OBJ = 16 * 2048   # objects per superblock of the sparse mixes


@pytest.fixture(scope='module')
def G():
    from abacusutils_amd.hod import GRAND_HOD
    return GRAND_HOD


def _lrg(lc, sigma=0.3):
    return {'LRG': dict(synth.LRG_PARAMS, logM_cut=lc, logM1=lc + 0.9, sigma=sigma)}


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


def test_kept_set_in_one_superblock_then_everywhere(G):
    """only the objects of one superblock can be kept under one parameter set, objects everywhere under the other; the
    two alternate, so the look-back sums runs of empty aggregates on both sides of a single non-empty one and the
    previous populate's bits move between superblocks"""
    n = 300_000
    hd, pd, params = synth.synth_hod_inputs(n, n, seed=31)
    lo, hi = 3 * SB_OBJ + 1000, 3 * SB_OBJ + 5000   # inside superblock 3 of both kinds
    hd['hmass'] = np.minimum(hd['hmass'], 10 ** 14.3)
    hd['hmass'][lo:hi] = 10 ** 15.5
    pd['phmass'] = np.minimum(pd['phmass'], 10 ** 14.3)
    pd['phmass'][lo:hi] = 10 ** 15.5
    st = G.StagedCatalog(hd, pd)
    try:
        seq = [(13.3, 0.3), (13.3, 0.3), (15.4, 0.05), (13.1, 0.3), (15.4, 0.05), (15.45, 0.05), (13.3, 0.3), (15.4, 0.05)]
        for step, (lc, sigma) in enumerate(seq):
            tracers = _lrg(lc, sigma)
            got = _populate(G, st, tracers, params)
            _check_oracle(hd, pd, tracers, params, got, f'step {step}: logM_cut {lc}')
            if sigma < 0.1:
                assert _queue_free(got[4]), got[4]
                kept_c, kept_s = np.flatnonzero(got[1]), np.flatnonzero(got[2])
                assert kept_c.size > 100 and kept_s.size > 0, (kept_c.size, kept_s.size)
                assert kept_c.min() >= lo and kept_c.max() < hi
                assert kept_s.min() >= lo and kept_s.max() < hi
    finally:
        st.free()


def test_repeated_capacity_growth(G):
    """populates that outgrow the catalogue buffers several times: every re-emission (abacus_hod_counts) runs the look-back
    again on the same bitmaps, under a new tag and a new ticket range, and the populates after it stay exact"""
    hd, pd, params = synth.synth_hod_inputs(400_000, 400_000, seed=32)
    st = G.StagedCatalog(hd, pd)
    try:
        grew = 0
        for lc in (14.8, 14.8, 14.0, 13.2, 14.8, 12.6, 12.3, 14.8, 12.3):
            got = _populate(G, st, _lrg(lc), params)
            _check_oracle(hd, pd, _lrg(lc), params, got, f'logM_cut {lc}')
            if _queue_free(got[4]) and got[4].get('hod_emit', 0) >= 2:
                grew += 1
        assert _queue_free(got[4]), got[4]
        assert grew >= 1, grew
    finally:
        st.free()


def test_empty_steps_and_no_particles(G):
    """steps that keep nothing between steps that keep thousands: every superblock publishes an empty aggregate and the
    last ticket reports zero totals; a catalogue without particles (no satellite superblock) populates exactly too"""
    hd, pd, params = synth.synth_hod_inputs(250_000, 350_000, seed=33)
    st = G.StagedCatalog(hd, pd)
    try:
        for step, lc in enumerate((12.9, 12.9, 20.0, 20.0, 12.8, 20.0, 13.0)):
            got = _populate(G, st, _lrg(lc), params)
            _check_oracle(hd, pd, _lrg(lc), params, got, f'logM_cut {lc}')
            if lc == 20.0:   # (next to) no candidate: hod_exact_index may not even be launched
                assert 'hod_deal' not in got[4] and 'hod_filter' not in got[4] and 'hod_emit' in got[4], got[4]
                assert got[0][0].sum() + got[0][1].sum() <= 2
        assert _queue_free(got[4]), got[4]
    finally:
        st.free()
    hd, pd, params = synth.synth_hod_inputs(250_000, 0, seed=34)
    st = G.StagedCatalog(hd, pd)
    try:
        for lc in (12.9, 12.9, 13.1):
            got = _populate(G, st, _lrg(lc), params)
            _check_oracle(hd, pd, _lrg(lc), params, got, f'no particles, logM_cut {lc}')
            assert got[0][1].sum() == 0
    finally:
        st.free()


def test_alternating_with_deal_path_on_one_catalogue(G, options):
    """the queue-free path and the three-launch comparator alternate on one staged catalogue: each hands the other keep
    masks it must clear, and both give the same masks, counts and catalogue"""
    hd, pd, params = synth.synth_hod_inputs(300_000, 300_000, seed=35)
    st = G.StagedCatalog(hd, pd)
    try:
        for step, lc in enumerate((13.0, 13.0, 12.8, 13.2, 12.9, 12.9)):
            options.set('hod_deal', 1)
            b = _populate(G, st, _lrg(lc), params)
            options.set('hod_deal', 0)
            a = _populate(G, st, _lrg(lc), params)
            if step >= 1:   # the comparator finds no kept lists behind this path: it streams the keys instead of hod_deal
                assert _queue_free(a[4]) and not _queue_free(b[4]), (a[4], b[4])
            _check_same(a, b, f'step {step}: logM_cut {lc}')
        _check_oracle(hd, pd, _lrg(12.9), params, a, 'last')
    finally:
        st.free()


def test_grid_beyond_one_round_of_workgroups(G, options):
    """5e7 halos + 5e7 particles: 3052 superblocks, more than the GPU holds workgroups at once (at most 8 per CU), so the
    capped grid takes several in turn; alternating with the comparator on the same catalogue"""
    n = 50_000_000
    hd, pd, params = synth.synth_hod_inputs(n, n, seed=606)
    st = G.StagedCatalog(hd, pd)
    try:
        for step, lc in enumerate((13.3, 13.3, 13.45, 13.2)):
            options.set('hod_deal', 1)
            b = _populate(G, st, _lrg(lc), params)
            options.set('hod_deal', 0)
            a = _populate(G, st, _lrg(lc), params)
            if step >= 1:
                assert _queue_free(a[4]), a[4]
            _check_same(a, b, f'step {step}: logM_cut {lc}')
        assert a[0][0][0] > 100_000
    finally:
        st.free()
