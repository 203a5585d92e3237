"""Every HOD populate path held to the oracle at the parameter and catalogue corners of tests/corners.py.

One staged catalogue per case and a sequence of populates on it; after EVERY populate the keep masks, the six counts, all
eight columns of every tracer and their order are bit-equal to oracle.gen_gal_cat(..., return_keep=True).  No tolerances.

  1  the corner parameters (first use of the keys: the streaming filter)
  2  the same again (LRG alone: the key index is built; the queue-free path hod_exact_index -> hod_emit_bm wherever both
     envelope tables are on and the threshold set is not dense)
  3  a neighbour: every logM_cut + 0.07
  4  the corner again (the neighbour's bits and bytes must be gone)
  5  the corner under each comparator option hod_opts() reads (all but `dbg`): hod_deal, hod_noindex, hod_nokeys, hod_nolazy,
     hod_one_stage, hod_f64filter, hod_norec, hod_nocls, hod_pipe 1 / 2, hod_eblock 256 / 384, hod_sbtiles 8 / 16,
     hod_nobalance
  6  the corner with the defaults restored (queue-free again where step 2 was)

Path evidence: the launch table of the library's profiler (hod_filter / hod_deal / hod_exact / hod_emit / hod_build_keys) and
the filter's candidate count (StagedCatalog.candidates), which with the default options must equal what the host restatement
of the filter (corners.envelope: hod_envelope.hpp built with g++) lets through - per kind the number of keys at or below their
bin's threshold where the kind's table is on, every object where the kind's guard is false.  What neither can tell apart:
hod_norec, hod_nocls and hod_pipe select instantiations of kernels profiled under the one name hod_exact, hod_eblock of
hod_emit; hod_nobalance only acts above 256 superblocks (2e6 objects) and is a no-op at this size.  For those the evidence is
that the option was set while the populate ran and the result is exact."""
import time

import numpy as np
import pytest
from conftest import assert_mock_equal
from corners import CORNERS, corner_case, envelope, neighbour

from abacusutils_amd import synth

pytestmark = pytest.mark.gpu

OPTIONS = [('hod_deal', 1), ('hod_noindex', 1), ('hod_nokeys', 1), ('hod_nolazy', 1), ('hod_one_stage', 1), ('hod_f64filter', 1),
           ('hod_norec', 1), ('hod_nocls', 1), ('hod_pipe', 1), ('hod_pipe', 2), ('hod_eblock', 256), ('hod_eblock', 384),
           ('hod_sbtiles', 8), ('hod_sbtiles', 16), ('hod_nobalance', 1)]
STREAMING = ('hod_noindex', 'hod_nokeys', 'hod_nolazy', 'hod_one_stage', 'hod_f64filter')   # options under which a filter kernel must run


@pytest.fixture(scope='module')
def G():
    from abacusutils_amd.hod import GRAND_HOD
    return GRAND_HOD


def _populate(st, p, tracers):
    """one populate; (counts[6], keep_cent, keep_sat, catalogue, {kernel: launches}, (halo, particle) candidates)"""
    from abacusutils_amd import _lib
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        ncent, nsat = st.populate(p)
    finally:
        _lib.profile_enable(False)
    launches = {k: n for k, (ms, n) in _lib.profile_get().items() if n}
    _lib.profile_reset()
    kc, ks = st.fetch_keep()
    return np.concatenate((ncent, nsat)), kc, ks, {tr: st.fetch(tr) for tr in tracers}, launches, st.candidates()


def _queue_free(launches):
    return 'hod_deal' not in launches and 'hod_filter' not in launches and launches.get('hod_emit', 0) >= 1


class _Want:
    """the oracle's answer for one parameter set, evaluated once, and the host restatement of its filter"""

    def __init__(self, hd, pd, params, tracers, ranks, rsd):
        from oracle import oracle
        self.tracers = tracers
        self.mock, self.kc, self.ks = oracle.gen_gal_cat(hd, pd, tracers, params, Nthread=oracle.max_threads(), enable_ranks=ranks,
                                                         rsd=rsd, return_keep=True)
        self.counts = np.zeros(6, np.int64)
        for t, tr in enumerate(('LRG', 'ELG', 'QSO')):
            if tr in tracers:
                self.counts[t], self.counts[3 + t] = self.mock[tr]['Ncent'], len(self.mock[tr]['x']) - self.mock[tr]['Ncent']
        self.flags, pc, ps = envelope(hd, pd, params, tracers, ranks, rsd)
        nh, npart = len(pc), len(ps)
        # candidates of the default options; None: the arithmetic bound of the fallback filter decides (not restated on the host)
        self.cand_c = int(pc.sum()) if self.flags['c_ok'] else (nh if not self.flags['cent_ok'] else None)
        self.cand_s = int(ps.sum()) if self.flags['s_ok'] else (npart if not self.flags['sat_ok'] else None)
        sparse = set(tracers) == {'LRG'}
        dense_set = self.flags['c_ok'] and self.flags['s_ok'] and int(pc.sum()) + int(ps.sum()) > (nh + npart) // 8
        self.index = sparse and self.flags['c_ok'] and self.flags['s_ok'] and not dense_set   # the key index serves this set

    def check(self, got, what, default_filter=True):
        counts, kc, ks, mock, launches, cand = got
        np.testing.assert_array_equal(kc, self.kc, err_msg=f'{what}: keep mask of the halos')
        np.testing.assert_array_equal(ks, self.ks, err_msg=f'{what}: keep mask of the particles')
        np.testing.assert_array_equal(counts, self.counts, err_msg=f'{what}: counts')
        try:
            assert_mock_equal(mock, self.mock, exact=True)
        except AssertionError as e:
            raise AssertionError(f'{what}: {e}') from None
        if default_filter:
            for kind, c, w in (('halo', cand[0], self.cand_c), ('particle', cand[1], self.cand_s)):
                assert w is None or c == w, f'{what}: {c} {kind} candidates, the host restatement of the filter gives {w} ({launches})'


@pytest.mark.parametrize('name', CORNERS)
def test_corner_through_every_path(G, options, name):
    hd, pd, params, tracers, ranks, rsd = corner_case(name)
    t0 = time.perf_counter()
    want = _Want(hd, pd, params, tracers, ranks, rsd)
    near = neighbour(tracers)
    want_near = _Want(hd, pd, params, near, ranks, rsd)
    t_oracle = time.perf_counter() - t0
    p, p_near = G.marshal_params(tracers, params, ranks, rsd), G.marshal_params(near, params, ranks, rsd)
    st = G.StagedCatalog(hd, pd)
    t_stage = time.perf_counter() - t0 - t_oracle
    try:
        got = _populate(st, p, tracers)                                   # 1
        want.check(got, f'{name} step 1')
        assert 'hod_filter' in got[4] and got[4].get('hod_build_keys', 0) == 2, got[4]
        got = _populate(st, p, tracers)                                   # 2
        want.check(got, f'{name} step 2')
        step2 = 'queue-free' if _queue_free(got[4]) else ('hod_deal' if 'hod_deal' in got[4] else 'streaming')
        if set(tracers) == {'LRG'}:
            assert step2 == ('queue-free' if want.index else 'streaming'), (name, got[4], want.flags)
        else:
            assert step2 == 'streaming', (name, got[4])
        print(f'{name}: galaxies {want.counts[:3] + want.counts[3:]}, false flags {[k for k, v in want.flags.items() if not v]}, '
              f'candidates {got[5][0] / len(want.kc):.4f} / {got[5][1] / len(want.ks):.4f}, step 2 {step2}')
        got = _populate(st, p_near, near)                                 # 3
        want_near.check(got, f'{name} step 3 (neighbour)')
        got = _populate(st, p, tracers)                                   # 4
        want.check(got, f'{name} step 4')
        for opt, value in OPTIONS:                                        # 5
            options.set(opt, value)
            # the comparator of the index path needs the previous populate's kept lists: its first populate streams the keys
            for rep in range(2 if opt == 'hod_deal' else 1):
                got = _populate(st, p, tracers)
                want.check(got, f'{name} step 5 ({opt} = {value})', default_filter=opt not in ('hod_nokeys', 'hod_one_stage', 'hod_f64filter'))
            if opt == 'hod_deal' and want.index:   # (without a candidate there is nothing to deal: no launch)
                assert ('hod_deal' in got[4]) == (want.cand_c + want.cand_s > 0) and 'hod_filter' not in got[4], (name, got[4])
            if opt in STREAMING or (opt == 'hod_sbtiles' and value == 8):
                assert 'hod_filter' in got[4], (name, opt, got[4])
            if opt in ('hod_one_stage', 'hod_f64filter') and not want.flags['cent_ok']:
                assert got[5][0] == len(want.kc), (name, opt, got[5])     # no bound covers the parameters: every halo a candidate
            options.set(opt, 0)
        got = _populate(st, p, tracers)                                   # 6
        want.check(got, f'{name} step 6')
        assert _queue_free(got[4]) == (step2 == 'queue-free'), (name, got[4])
    finally:
        st.free()
    print(f'{name}: oracle {t_oracle:.2f} s, staging {t_stage:.2f} s, populates {time.perf_counter() - t0 - t_oracle - t_stage:.2f} s')


def test_update_and_reseed_on_the_index_path(G):
    """StagedCatalog.update() and reseed() invalidate the keys, the shadows, the record fields and the index: the keys are
    rebuilt once per change (two hod_build_keys launches, one per kind, in the first populate after it), that populate
    streams them, and the queue-free path resumes with the second populate.  Every populate is held to the oracle on the
    arrays then resident."""
    hd, pd, params, _, _, _ = corner_case('production_lrg')
    tracers = {'LRG': synth.PRODUCTION_TRACERS['LRG']}
    p = G.marshal_params(tracers, params, True, True)
    rng = np.random.default_rng(99)
    nh, npart = len(hd['hmass']), len(pd['phmass'])
    st = G.StagedCatalog(hd, pd)

    def run(n, hd, pd, what):
        want = _Want(hd, pd, params, tracers, True, True)
        assert want.index
        for k in range(n):
            got = _populate(st, p, tracers)
            want.check(got, f'{what}, populate {k}')
            assert got[4].get('hod_build_keys', 0) == (2 if k == 0 else 0), (what, k, got[4])
            assert ('hod_filter' in got[4]) if k == 0 else _queue_free(got[4]), (what, k, got[4])

    try:
        run(2, hd, pd, 'as staged')
        new_h = rng.random(nh, dtype=np.float32).astype(np.float64)
        new_p = rng.random(npart, dtype=np.float32).astype(np.float64)
        new_v = (rng.standard_normal((nh, 3)) * (hd['hsigma3d'] / np.sqrt(3.0))[:, None]).astype(np.float32).astype(np.float64)
        st.update('hrandoms', new_h)
        st.update('prandoms', new_p)
        st.update('hveldev', new_v)
        hd2, pd2 = dict(hd, hrandoms=new_h, hveldev=new_v), dict(pd, prandoms=new_p)
        run(3, hd2, pd2, 'after update')
        st.reseed(12345, hsigma3d=hd['hsigma3d'])
        hd3 = dict(hd, hrandoms=st.fetch_field('hrandoms'), hveldev=st.fetch_field('hveldev'))
        pd3 = dict(pd, prandoms=st.fetch_field('prandoms'))
        assert not np.array_equal(hd3['hrandoms'], new_h) and not np.array_equal(pd3['prandoms'], new_p)
        run(2, hd3, pd3, 'after reseed')
    finally:
        st.free()
