"""The seeded prepare path (`prepare_slab_arrays(rng=<seed>)`: abacus_prepare_slab / abacus_prepare_slab_fetch and the
column-by-column path over abacus_prepare_particles, csrc/prepare.hip) against the oracle's seeded restatement
(oracle/prepare_oracle.py: the device's Philox streams restated in NumPy, pinned to the C restatement and the published vectors,
around the deterministic code the reference-held goldens pin - tests/test_oracle_prepare.py), value for value, on the corner slabs
of tests/prepare_corners.py and one synthetic slab: the selection itself (pos, vel, halo_id, Np, the new offsets, the mask), the
random columns, the rank columns.

On the corner slabs every column is compared exactly, `ranksp` and `ranksc` included: the restatement breaks equal rank keys by
particle index like the device (so `ranksc`, whose keys tie whenever two kept particles are each other's nearest neighbour, is
exact everywhere), and a CPU test holds that the restatement's `ranksp` order on these slabs does not depend on how the float32
logarithms are rounded.  On the synthetic slab `ranksp` keeps the swap rule of test_prepare_gpu.compare_tables.

What the exact comparison found: the `wave_edges` corner (998 kept particles in one halo) had two neighbouring `ranksp` ranks
exchanged on the device.  One of the two particles moves almost radially (v_tan2 = 11246 out of v2 = 9794494: eleven float32 ulps
of v2), and the kernel took r0 with `__fsqrt_rn`, which compiles to the bare v_sqrt_f32 - one ulp off np.sqrt's correctly rounded
root there, two ulps in vel_rad, 3e-4 in the key, more than the 2.9e-4 between the two keys.  prep_ranks now calls sqrtf, which
the compiler rounds correctly.

Which test fails when the device code is broken (tried by reading, each names a corner that cannot pass):
  prep_keys drawing from stream 5 instead of 3, prep_pick without cstart[j]   test_both_paths_against_the_oracle[mixed],
                                                                              [wave_edges], [synthetic] (another selection)
  prep_rank_work taking kept >= 3                                             [single_2], [many_halos] (pairs never ranked)
  key_before without the `ia < ib` rule                                       [rank_keys] (identical particles share a rank)"""
import ctypes as C

import numpy as np
import prepare_corners as pc
import pytest
from test_prepare_gpu import compare_tables

pytestmark = pytest.mark.gpu

SWAP = ('ranksp', 'ranksc')


def prepare(c, MT, want_ranks, columnwise, options, shear=False, device=False, halos=None, **kw):
    from abacusutils_amd import _lib
    from abacusutils_amd.hod import prepare_sim as ps
    options.set('prep_columnwise', 1 if columnwise else 0)
    halos, parts = c.halos if halos is None else halos, c.parts
    held = []
    if device:
        halos = {k: _lib.DeviceArray(v) for k, v in halos.items()}
        parts = {k: _lib.DeviceArray(v) for k, v in parts.items()}
        held = list(halos.values()) + list(parts.values())
    args = dict(want_ranks=want_ranks, want_AB=pc.want_AB(c), shearmark=pc.shear_field() if shear else None, Lbox=pc.LBOX, rng=c.seed,
                halo_index0=c.halo_index0, part_index0=c.part_index0)
    args.update(kw)
    try:
        return ps.prepare_slab_arrays(halos, parts, c.Mpart, c.h, MT, **args)
    finally:
        for a in held:
            a.free()


def check(got, name, MT, want_ranks, label, shear=False):
    """the tables of a call against the restatement's: compare_tables' rules, and on the corner slabs the two swap columns exactly"""
    H, P, m = got
    Ho, Po, mo = pc.oracle_tables(name, MT, shear)
    if not want_ranks:
        Po = pc.without_ranks(Po)
    label = f'{name} MT={MT} ranks={want_ranks} {label}'
    np.testing.assert_array_equal(m, mo, err_msg=label)
    assert m.dtype == mo.dtype
    compare_tables(H, Ho, label + ' halos')
    assert sorted(P) == sorted(Po), (label, sorted(P), sorted(Po))
    if name == 'synthetic':
        compare_tables(P, Po, label + ' particles')
        if want_ranks:
            np.testing.assert_array_equal(P['ranksc'], Po['ranksc'], err_msg=label + ' ranksc')
        return
    compare_tables({k: v for k, v in P.items() if k not in SWAP}, {k: v for k, v in Po.items() if k not in SWAP}, label + ' particles')
    for k in SWAP:
        if k in Po:
            assert P[k].dtype == Po[k].dtype and P[k].shape == Po[k].shape, (label, k)
            np.testing.assert_array_equal(P[k], Po[k], err_msg=f'{label} {k}')


@pytest.mark.parametrize('name', pc.CORNERS + ['synthetic'])
def test_both_paths_against_the_oracle(name, options):
    """one pass and column by column, MT x want_ranks, host columns: every column of both tables and the mask"""
    c = pc.synthetic() if name == 'synthetic' else pc.corner(name)
    for MT in c.MT:
        for want_ranks in (True, False):
            for columnwise in (False, True):
                check(prepare(c, MT, want_ranks, columnwise, options), name, MT, want_ranks, 'columnwise' if columnwise else 'one pass')


@pytest.mark.parametrize('columnwise', [False, True])
def test_shear_ranks_against_the_oracle(columnwise, options):
    c = pc.corner('mixed')
    assert pc.shear_has_no_ties(c, pc.shear_field())
    got = prepare(c, True, True, columnwise, options, shear=True)
    check(got, 'mixed', True, True, 'shear', shear=True)
    assert np.ptp(got[0]['shear_rank']) > 0.5


@pytest.mark.parametrize('name', ['mixed', 'wave_edges', 'rank_keys', 'index_above', 'seed_negative', 'no_particles', 'none_kept',
                                  'kept_without_particles', 'lds_big', 'strided', 'synthetic'])
def test_device_resident_inputs(name, options):
    """every input column a `_lib.DeviceArray` (what the reader's unpack kernels leave in HBM): used in place, same tables"""
    c = pc.synthetic() if name == 'synthetic' else pc.corner(name)
    for MT in c.MT:
        for want_ranks in (True, False):
            check(prepare(c, MT, want_ranks, False, options, device=True), name, MT, want_ranks, 'device columns')


@pytest.mark.parametrize('name', ['mixed', 'rank_keys', 'lds_big', 'many_halos'])
def test_profiler_on_and_off(name, options):
    """the rank kernel runs on the library stream under the profiler and on a stream of its own without it"""
    from abacusutils_amd import _lib
    c = pc.corner(name)
    MT = c.MT[-1]
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        on = prepare(c, MT, True, False, options)
    finally:
        _lib.profile_enable(False)
    prof = _lib.profile_get()
    assert 'prep_ranks' in prof and 'prep_compact' in prof, sorted(prof)
    check(on, name, MT, True, 'profiler on')
    _lib.profile_reset()
    check(prepare(c, MT, True, False, options), name, MT, True, 'profiler off')
    assert 'prep_ranks' not in _lib.profile_get()


def raw_prepare(c, MT, want_ranks, mbins=None):
    """abacus_prepare_slab alone, without the fetch: returns (return code, kept halos, kept particles)"""
    from abacusutils_amd import _lib
    from abacusutils_amd.hod import prepare_sim as ps
    keep = []
    a = ps._SlabArgs()
    a.nh, a.npart = c.nh, len(c.parts['pos'])
    for fld, (name, dt, _) in zip(('N', 'x', 'v', 'r25', 'r90', 'r98', 'npstartA', 'npoutA', 'id', 'sigmav'), ps._SLAB_HALO_IN):
        setattr(a, fld, ps._slab_col(c.halos[name], dt, keep))
    a.pos, a.vel = ps._slab_col(c.parts['pos'], np.float32, keep), ps._slab_col(c.parts['vel'], np.float32, keep)
    a.fenv_rank = a.shear_rank = None
    if mbins is None:
        a.mbins, a.n_edges = None, 0
    else:
        a.mbins, a.n_edges = ps._slab_col(mbins, np.float64, keep), len(mbins)
    a.MT, a.want_ranks, a.Mpart, a.h = int(MT), int(want_ranks), c.Mpart, c.h
    a.seed, a.halo_index0, a.part_index0 = c.seed & (2**64 - 1), c.halo_index0, c.part_index0
    nk, ns = C.c_int64(-1), C.c_int64(-1)
    rc = _lib.lib().abacus_prepare_slab(C.byref(a), C.byref(nk), C.byref(ns), None)
    return rc, int(nk.value), int(ns.value)


def no_slab_left():
    """the fetch after a failed abacus_prepare_slab finds nothing: no half-filled columns"""
    from abacusutils_amd import _lib
    with pytest.raises(_lib.AbacusHipError, match='no prepared slab'):
        _lib.check(_lib.lib().abacus_prepare_slab_fetch(None, None))


def good_call(options):
    """after a failure both paths still prepare a slab like the oracle"""
    for columnwise in (False, True):
        check(prepare(pc.corner('mixed'), False, True, columnwise, options), 'mixed', False, True, 'after a failure')


def test_calls_back_to_back_hand_the_side_stream_over(options):
    """a prepared slab whose rank columns are still being written on the side stream is dropped by the next call (no fetch in
    between), and fetched without its rank columns: the tables that follow are the oracle's"""
    from abacusutils_amd import _lib
    big, c = pc.corner('lds_big'), pc.corner('mixed')
    Ho, Po, mo = pc.oracle_tables('lds_big', False)
    rc, nk, ns = raw_prepare(big, False, True)
    assert rc == 0 and nk == len(Ho['N']) and ns == len(Po['pos'])
    check(prepare(c, True, False, False, options), 'mixed', True, False, 'after an unfetched slab')
    rc, nk, ns = raw_prepare(big, False, True)
    assert rc == 0 and ns == len(Po['pos'])
    _lib.check(_lib.lib().abacus_prepare_slab_fetch(None, None))            # no column wanted: waits for the rank kernel, releases
    no_slab_left()
    check(prepare(c, True, True, False, options), 'mixed', True, True, 'after a slab fetched without columns')
    check(prepare(c, True, False, False, options), 'mixed', True, False, 'ranks off after on')
    check(prepare(big, False, True, False, options), 'lds_big', False, True, 'and the large halo again')


@pytest.mark.parametrize('name', ['reader_uint64', 'reader_int64'])
def test_reader_dtypes_take_the_one_pass_path(name, options):
    """npstartA uint64 and npoutA uint32, as the CompaSO reader hands them over (host or device columns), go through
    abacus_prepare_slab (prep_compact ran) and give the tables of int64 columns bit for bit, dtypes included"""
    from abacusutils_amd import _lib
    c = pc.corner(name)
    assert c.halos['npstartA'].dtype == np.uint64 and c.halos['npoutA'].dtype == np.uint32
    as_int64 = dict(c.halos, npstartA=c.halos['npstartA'].astype(np.int64), npoutA=c.halos['npoutA'].astype(np.int64))
    for MT in c.MT:
        want = prepare(c, MT, True, False, options, halos=as_int64)
        check(want, name, MT, True, 'int64 columns')
        for device in (False, True):
            _lib.profile_reset()
            _lib.profile_enable(True)
            try:
                got = prepare(c, MT, True, False, options, device=device)
            finally:
                _lib.profile_enable(False)
            assert 'prep_compact' in _lib.profile_get(), (device, sorted(_lib.profile_get()))
            np.testing.assert_array_equal(got[2], want[2])
            for g, w in zip(got[:2], want[:2]):
                assert list(g) == list(w)
                for k in w:
                    assert g[k].dtype == w[k].dtype and g[k].shape == w[k].shape, (k, g[k].dtype, w[k].dtype)
                    np.testing.assert_array_equal(g[k], w[k], err_msg=k)
            assert got[0]['id'].dtype == c.halos['id'].dtype
        check(prepare(c, MT, True, True, options), name, MT, True, 'columnwise')


@pytest.mark.parametrize('name', ['empty', 'empty_with_particles'])
def test_an_empty_slab_gives_empty_tables(name, options):
    """nh == 0: empty tables with the keys (in order), dtypes and row shapes of a slab with halos - host and device columns, both
    paths; and the library's own entry point leaves an empty slab the fetch accepts"""
    from abacusutils_amd import _lib
    c, full = pc.corner(name), pc.corner('mixed')
    for want_ranks in (True, False):
        for columnwise in (False, True):
            H1, P1, m1 = prepare(full, True, want_ranks, columnwise, options)
            for device in (False, True):
                H0, P0, m0 = prepare(c, True, want_ranks, columnwise, options, device=device, want_AB=True)
                assert m0.shape == (0,) and m0.dtype == m1.dtype
                for e, f in ((H0, H1), (P0, P1)):
                    assert list(e) == list(f)
                    for k in f:
                        assert e[k].shape == (0,) + f[k].shape[1:] and e[k].dtype == f[k].dtype, (k, e[k].shape, e[k].dtype, f[k].dtype)
                check((H0, P0, m0), name, True, want_ranks, 'empty')
    rc, nk, ns = raw_prepare(c, True, True)
    assert (rc, nk, ns) == (0, 0, 0)
    _lib.check(_lib.lib().abacus_prepare_slab_fetch(None, None))
    no_slab_left()


def test_a_halo_over_the_rank_kernels_lds_is_refused(options):
    """3151 and more kept particles in one halo: both entry points say so, nothing is left behind, and without the rank columns
    the slab is prepared like any other"""
    from abacusutils_amd import _lib
    c = pc.corner('lds_over')
    with pytest.raises(_lib.AbacusHipError, match=c.raises):
        prepare(c, False, True, False, options)
    no_slab_left()
    with pytest.raises(_lib.AbacusHipError, match=c.raises):
        prepare(c, False, True, True, options)
    no_slab_left()
    good_call(options)
    for columnwise in (False, True):
        check(prepare(c, False, False, columnwise, options), 'lds_over', False, False, 'no ranks')


def test_mass_bins_that_do_not_increase_are_refused(options):
    from abacusutils_amd import _lib
    c = pc.corner('mixed')
    with pytest.raises(_lib.AbacusHipError, match='mass bin edges must increase'):
        prepare(c, False, True, False, options, want_AB=True, mcut=1e16)             # logspace(16, 15.5): falling edges
    no_slab_left()
    rc, nk, ns = raw_prepare(c, False, True, mbins=np.array([1e11, 1e12, 1e12, 1e13]))
    assert rc != 0 and 'must increase' in _lib.lib().abacus_last_error().decode()
    no_slab_left()
    good_call(options)


@pytest.mark.parametrize('name', ['slice_overshoot', 'slice_minus_one'])
def test_a_slice_outside_the_particle_array_is_refused(name, options):
    """a kept halo whose slice ends one particle behind the particle array, or starts at -1: both entry points refuse the slab (the
    kernels that walk slices test them: none reads outside its arrays on the way to the error), nothing is left behind"""
    from abacusutils_amd import _lib
    c = pc.corner(name)
    for columnwise in (False, True):
        for want_ranks in (True, False):
            with pytest.raises(_lib.AbacusHipError, match=c.raises):
                prepare(c, False, want_ranks, columnwise, options)
            no_slab_left()
    good_call(options)
