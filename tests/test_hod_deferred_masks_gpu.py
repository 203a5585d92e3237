"""Keep masks on demand and the emission's early loads on the per-superblock index path (hod_exact_sbidx -> hod_emit).

A populate of that path writes no keep byte: its kept lists are the record, and the masks are written (hod_keep_masks) when
somebody asks - abacus_hod_fetch_keep, or a populate of any other path, which reads or rewrites the bytes.  Every result is held
exactly to the CPU oracle (counts, both keep masks, the whole catalogue), or byte for byte to a second staged catalogue that
keeps its masks populate by populate (`hod_keepmasks` = 1); the kernels a populate launched are read off the library's
profiler so that each case provably leaves the deferred state the way it is about."""
import numpy as np
import pytest
from conftest import assert_mock_equal

from abacusutils_amd import synth

pytestmark = pytest.mark.gpu

SB = 16 * 2048   # objects of a superblock of the sparse layout


@pytest.fixture(scope='module')
def G():
    from abacusutils_amd.hod import GRAND_HOD
    return GRAND_HOD


def _lrg(lc, sigma=0.3, **kw):
    return {'LRG': dict(synth.LRG_PARAMS, logM_cut=lc, logM1=lc + 0.9, sigma=sigma, **kw)}


class _Profiled:
    """the launches of the library calls made inside the block: {kernel: launches}"""

    def __enter__(self):
        from abacusutils_amd import _lib
        _lib.profile_reset()
        _lib.profile_enable(True)
        self.launches = {}
        return self

    def __exit__(self, *exc):
        from abacusutils_amd import _lib
        _lib.profile_enable(False)
        self.launches.update({k: n for k, (ms, n) in _lib.profile_get().items() if n})
        _lib.profile_reset()
        return False


def _unobserved(G, st, tracers, params):
    """one populate, nothing read back but its counts"""
    st.populate(G.marshal_params(tracers, params, False, True))


def _observed(G, st, tracers, params):
    """one populate; (counts, keep_cent, keep_sat, catalogue, {kernel: launches of the populate alone})"""
    with _Profiled() as prof:
        ncent, nsat = st.populate(G.marshal_params(tracers, params, False, True))
    kc, ks = st.fetch_keep()
    return (np.asarray(ncent), np.asarray(nsat)), kc, ks, {tr: st.fetch(tr) for tr in tracers}, prof.launches


def _deferred(launches):
    """the populate ran hod_exact + hod_emit and nothing else: no filter, no queues, no mask kernel"""
    return set(launches) == {'hod_exact', 'hod_emit'} and launches['hod_exact'] == 1


def _oracle(hd, pd, tracers, params):
    from oracle import oracle
    return oracle.gen_gal_cat(hd, pd, tracers, params, Nthread=oracle.max_threads(), enable_ranks=False, rsd=True,
                              return_keep=True)


def _check_oracle(hd, pd, tracers, params, got, err_msg, want=None):
    counts, kc, ks, mock, _ = got
    want, wkc, wks = want if want is not None else _oracle(hd, pd, tracers, params)
    np.testing.assert_array_equal(kc, wkc, err_msg=err_msg)
    np.testing.assert_array_equal(ks, wks, err_msg=err_msg)
    for t, tr in enumerate(('LRG', 'ELG', 'QSO')):
        if tr in tracers:
            assert counts[0][t] == want[tr]['Ncent'], err_msg
    assert_mock_equal(mock, want, exact=True)


def _check_same(a, b, err_msg):
    np.testing.assert_array_equal(a[0][0], b[0][0], err_msg=err_msg)
    np.testing.assert_array_equal(a[0][1], b[0][1], err_msg=err_msg)
    np.testing.assert_array_equal(a[1], b[1], err_msg=err_msg)
    np.testing.assert_array_equal(a[2], b[2], err_msg=err_msg)
    assert_mock_equal(a[3], b[3], exact=True)


def _moving_catalogue(n, seed):
    """the mass pattern of test_unkeep_of_shrinking_growing_and_moving_kept_sets: a block of very heavy objects inside
    superblock 3 of both kinds, everything else capped below it"""
    hd, pd, params = synth.synth_hod_inputs(n, n, seed=seed)
    lo, hi = 3 * SB + 1000, 3 * SB + 5000
    hd['hmass'] = np.minimum(hd['hmass'], 10 ** 14.3)
    hd['hmass'][lo:hi] = 10 ** 15.5
    pd['phmass'] = np.minimum(pd['phmass'], 10 ** 14.3)
    pd['phmass'][lo:hi] = 10 ** 15.5
    return hd, pd, params


MOVING = [(13.3, 0.3), (13.3, 0.3), (13.6, 0.3), (12.9, 0.3), (15.4, 0.05), (13.1, 0.3), (15.4, 0.05), (15.45, 0.05), (13.3, 0.3)]


def test_masks_after_unobserved_populates(G):
    """seven populates of the index path with kept sets that shrink, grow and move between superblocks, no mask read in
    between: the masks asked for afterwards are the oracle's for the LAST parameters, a second read gives the same bytes, and
    the profiler saw hod_exact + hod_emit per populate and hod_keep_masks once"""
    hd, pd, params = _moving_catalogue(300_000, 43)
    st = G.StagedCatalog(hd, pd)
    try:
        for lc, sigma in MOVING[:2]:   # the streaming filter, then the populate that builds the indices
            _unobserved(G, st, _lrg(lc, sigma), params)
        with _Profiled() as prof:
            for lc, sigma in MOVING[2:]:
                ncent, nsat = st.populate(G.marshal_params(_lrg(lc, sigma), params, False, True))
            kc, ks = st.fetch_keep()
            mock = {'LRG': st.fetch('LRG')}
            kc2, ks2 = st.fetch_keep()
        lc, sigma = MOVING[-1]
        got = ((np.asarray(ncent), np.asarray(nsat)), kc, ks, mock, prof.launches)
        _check_oracle(hd, pd, _lrg(lc, sigma), params, got, 'after seven unobserved populates')
        np.testing.assert_array_equal(kc2, kc)
        np.testing.assert_array_equal(ks2, ks)
        n = len(MOVING) - 2
        assert set(prof.launches) == {'hod_exact', 'hod_emit', 'hod_keep_masks'}, prof.launches
        assert prof.launches['hod_exact'] == n and prof.launches['hod_emit'] >= n, prof.launches   # more: capacity growth
        assert prof.launches['hod_keep_masks'] == 1, prof.launches
    finally:
        st.free()


def _enter_deferred(G, st, params, seq=((13.0, 0.3), (13.0, 0.3), (12.8, 0.3), (13.2, 0.3), (12.9, 0.3))):
    """two populates that build the indices, then three of the index path; the last three provably deferred"""
    for step, (lc, sigma) in enumerate(seq):
        with _Profiled() as prof:
            _unobserved(G, st, _lrg(lc, sigma), params)
        if step >= 2:
            assert _deferred(prof.launches), prof.launches


@pytest.mark.parametrize('exit_', ['hod_sbindex', 'hod_deal', 'dense', 'hod_sbtiles', 'elg', 'reseed'])
def test_exit_from_deferred_masks_by_another_path(G, options, exit_):
    """three deferred populates, then - with no mask read first - a populate of a path that reads or rewrites the keep bytes:
    the bitmap path, the tile queues, the streaming filter of a dense threshold set, the other superblock size, a mix with
    ELG conformity (keep_cent[pinds]), and a populate behind a reseed"""
    hd, pd, params = synth.synth_hod_inputs(250_000, 350_000, seed=51)
    st = G.StagedCatalog(hd, pd)
    try:
        _enter_deferred(G, st, params)
        tracers = _lrg(13.1)
        if exit_ in ('hod_sbindex', 'hod_deal'):
            options.set(exit_, 1)
        elif exit_ == 'dense':
            tracers = _lrg(10.5)
        elif exit_ == 'hod_sbtiles':
            options.set('hod_sbtiles', 8)
        elif exit_ == 'elg':
            tracers = dict(_lrg(13.1), ELG=synth.ELG_PARAMS)
        elif exit_ == 'reseed':
            st.reseed(7, hsigma3d=hd['hsigma3d'])
            hd = dict(hd, hrandoms=st.fetch_field('hrandoms'), hveldev=st.fetch_field('hveldev').reshape(-1, 3))
            pd = dict(pd, prandoms=st.fetch_field('prandoms'))
        got = _observed(G, st, tracers, params)
        _check_oracle(hd, pd, tracers, params, got, f'exit by {exit_}')
        assert got[4].get('hod_keep_masks') == 1 and not _deferred(got[4]), got[4]
        if exit_ in ('dense', 'reseed', 'hod_sbtiles', 'elg'):
            assert 'hod_filter' in got[4], got[4]
        got = _observed(G, st, tracers, params)   # the path by itself: nothing left deferred
        _check_oracle(hd, pd, tracers, params, got, f'second populate after the exit by {exit_}')
        assert 'hod_keep_masks' not in got[4], got[4]
    finally:
        st.free()


def test_exit_from_deferred_masks_by_capacity_growth(G):
    """a populate that outgrows the catalogue buffers stays deferred: its re-emission is hod_emit alone on the kept lists"""
    hd, pd, params = synth.synth_hod_inputs(400_000, 400_000, seed=47)
    st = G.StagedCatalog(hd, pd)
    try:
        _enter_deferred(G, st, params, seq=((14.8, 0.3), (14.8, 0.3), (14.6, 0.3), (14.8, 0.3), (14.7, 0.3)))
        got = _observed(G, st, _lrg(12.3), params)
        assert got[4] == {'hod_exact': 1, 'hod_emit': 2}, got[4]
        _check_oracle(hd, pd, _lrg(12.3), params, got, 'outgrown buffers')
    finally:
        st.free()


def test_keepmasks_comparator_and_back(G, options):
    """`hod_keepmasks` = 1 behind three deferred populates, then 0 again: byte-identical at every step to a second staged
    catalogue that stays on `hod_keepmasks` = 1, and the oracle's at the end"""
    hd, pd, params = _moving_catalogue(300_000, 52)
    st, ref = G.StagedCatalog(hd, pd), G.StagedCatalog(hd, pd)
    try:
        options.set('hod_keepmasks', 1)
        for lc, sigma in MOVING[:5]:
            _unobserved(G, ref, _lrg(lc, sigma), params)
        options.set('hod_keepmasks', 0)
        _enter_deferred(G, st, params, seq=MOVING[:5])
        for step, (lc, sigma, keepmasks) in enumerate(((13.1, 0.3, 1), (15.4, 0.05, 1), (15.45, 0.05, 0), (13.3, 0.3, 0),
                                                       (12.9, 0.3, 1), (13.6, 0.3, 0))):
            options.set('hod_keepmasks', 1)
            want = _observed(G, ref, _lrg(lc, sigma), params)
            options.set('hod_keepmasks', keepmasks)
            got = _observed(G, st, _lrg(lc, sigma), params)
            _check_same(got, want, f'step {step}: logM_cut {lc}, hod_keepmasks {keepmasks}')
            assert want[4] == {'hod_exact': 1, 'hod_emit': want[4]['hod_emit']}, want[4]
            if keepmasks:   # the masks it un-keeps from are written first, where the populate before left them deferred
                assert set(got[4]) - {'hod_keep_masks'} == {'hod_exact', 'hod_emit'}, got[4]
                assert ('hod_keep_masks' in got[4]) == (step == 0), got[4]   # later steps: the read-back wrote them
            else:
                assert set(got[4]) == {'hod_exact', 'hod_emit'}, got[4]
        _check_oracle(hd, pd, _lrg(lc, sigma), params, got, 'the last step against the oracle')
    finally:
        st.free()
        ref.free()


HEAVY = (0, 1, 255, 256, 257, 511, 512, 513, 700, 0)


def test_emission_corners_kept_counts_around_the_workgroup_size(G):
    """ten superblocks a kind whose kept counts are 0, 1 and the values around one and two rounds of the emission's 256
    threads: the early kept-entry loads of hod_emit (entries tid and tid + 256, read before the counts are known) meet slices
    with fewer entries than that, exactly that many, and more"""
    n = len(HEAVY) * SB
    hd, pd, params = synth.synth_hod_inputs(n, n, seed=53)
    rng = np.random.default_rng(54)
    hd['hmass'][:] = 10 ** 10.0
    pd['phmass'][:] = 10 ** 10.0
    for k, nk in enumerate(HEAVY):   # heavy objects: certain centrals (N_cent = ic), certain satellites (weight 1, N_sat > 1)
        for d, mass, rand, extra in ((hd, 'hmass', 'hrandoms', 'hmultis'), (pd, 'phmass', 'prandoms', 'pweights')):
            at = k * SB + rng.choice(SB, size=nk, replace=False)
            d[mass][at] = 10 ** 15.0
            d[rand][at] = 1e-6
            d[extra][at] = 1.0
    tracers = _lrg(13.0)
    want = _oracle(hd, pd, tracers, params)
    for mask in want[1:]:   # a condition on the inputs: the oracle keeps exactly the heavy objects
        assert tuple(np.count_nonzero(mask.reshape(len(HEAVY), SB), axis=1)) == HEAVY
    st = G.StagedCatalog(hd, pd)
    try:
        for step in range(3):
            got = _observed(G, st, tracers, params)
            _check_oracle(hd, pd, tracers, params, got, f'step {step}', want=want)
            if step >= 2:
                assert _deferred(got[4]), got[4]
    finally:
        st.free()


@pytest.mark.parametrize('nh,npart', [(32773, 32773), (5, 70_000)])
def test_emission_corners_short_last_superblock(G, nh, npart):
    """a last superblock of fewer than 512 objects: the early kept-entry loads reach into the slack behind the kept lists,
    freshly allocated and never written"""
    hd, pd, params = synth.synth_hod_inputs(nh, npart, seed=55)
    st = G.StagedCatalog(hd, pd)
    try:
        for step, lc in enumerate((13.0, 13.0, 12.8, 13.2)):
            got = _observed(G, st, _lrg(lc), params)
            _check_oracle(hd, pd, _lrg(lc), params, got, f'({nh}, {npart}) step {step}: logM_cut {lc}')
            if step >= 2:
                assert _deferred(got[4]), got[4]
    finally:
        st.free()
