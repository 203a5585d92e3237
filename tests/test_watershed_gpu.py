"""The watershed void finder on the device (abacusutils_amd.analysis.watershed, C ABI abacus_ws_*) against the NumPy statement
tests/watershed_statement.py.  Needs an MI355X: run with `-m gpu`.

Every output but one is an integer or the bits of a float32 of the mesh: `labels`, `ncell`, `core`, `delta_min`, `offset_sum`, the five
tree columns in order, `nzones` and the hierarchy derived from them are held to the statement exactly.  `delta_sum` is a float64 sum in
no fixed order: per zone |got - fsum| <= ncell 2^-53 sum |x|, the worst case of a float64 sum of ncell terms in any order (derived in
`watershed_statement.delta_sum_bound`, not measured).

Shapes: n = 16 (dense pitch 16 and padded pitch 32) and n = 24 (padded pitch 32 != n), 4096 and 13824 cells - 16 and 54 workgroups;
both connectivities.  `white`: 85 / 208 zones (n = 16, 26 / 6 neighbours) and 289 / 726 (n = 24), several rounds of the tree;
`quantised`: many equal values, decided by the index half of the key; `constant`: one zone, chains of n cells, every cell on one
atomic target and every lane of a wave in one run; `zeros`: +0.0 and -0.0 mixed, one value; `corners`: cores in the cells 0 and n - 1 of
every axis, so every wrap of the stencil and of the offsets runs; the two-well and three-well meshes of the host test at their own
sizes (n = 8 and 12, padded pitch 32).  The padded copies carry -1e30 in every pad float: a pad read would be the deepest core."""
import functools

import numpy as np
import pytest
import watershed_statement as st

pytestmark = pytest.mark.gpu

PAD = np.float32(-1e30)
CASES = [(name, n) for n in (16, 24) for name in ('white', 'quantised', 'constant', 'zeros', 'corners')] + [('two_wells', 8), ('three_wells', 12)]
ZONES = {('white', 16, 26): 85, ('white', 16, 6): 208, ('white', 24, 26): 289, ('white', 24, 6): 726}


def _lib():
    from abacusutils_amd import _lib
    return _lib


def _pitch(n):
    return (n + 2 + 31) // 32 * 32


@functools.lru_cache(maxsize=None)
def _mesh(name, n):
    mesh = st.case(name, n)
    mesh.setflags(write=False)
    return mesh


@functools.lru_cache(maxsize=None)
def _want(name, n, connectivity):
    """the statement, once per case; its hierarchy too"""
    w = st.watershed(_mesh(name, n), connectivity)
    return w, st.hierarchy(w, w, n)


def _padded(mesh):
    n = mesh.shape[0]
    full = np.full((n, n, _pitch(n)), PAD, dtype=np.float32)
    full[:, :, :n] = mesh
    return full


def _assert_equal(got, want, label, labels=True):
    from abacusutils_amd.analysis.watershed import zone_hierarchy
    w, h = want
    assert got['nzones'] == w['nzones'], label
    keys = [k for k in st.INTEGER_KEYS if labels or k != 'labels']
    for k in keys:
        assert got[k].dtype == st.DTYPES[k] and got[k].shape == w[k].shape, (label, k)
        assert got[k].tobytes() == w[k].tobytes(), (label, k)
    assert got['delta_sum'].dtype == np.float64
    err, bound = np.abs(got['delta_sum'] - w['delta_sum']), st.delta_sum_bound(w)
    print(f'{label}: {w["nzones"]} zones, rounds {got["rounds"]}; delta_sum: max |got - fsum| / bound = {np.max(err / np.maximum(bound, 1e-300)):.3g}')
    assert (err <= bound).all(), label
    assert got['rounds'] == w['rounds'], label                       # Boruvka's rounds are determined by the order of the weights
    gh = zone_hierarchy(got)
    for k in h:
        assert gh[k].dtype == h[k].dtype and gh[k].tobytes() == h[k].tobytes(), (label, k)


# ------------------------------------------------------------------------------------------------- 1. the finder on given meshes
@pytest.mark.parametrize('connectivity', (26, 6))
@pytest.mark.parametrize('name,n', CASES)
def test_finder_equals_the_statement(name, n, connectivity):
    from abacusutils_amd.analysis.watershed import watershed_mesh
    lib = _lib()
    mesh, want = _mesh(name, n), _want(name, n, connectivity)
    L = 10.0 * n
    got = watershed_mesh(mesh, L, connectivity, return_labels=True)
    _assert_equal(got, want, f'{name} n={n} c={connectivity} host mesh')
    w = want[0]
    # the host part of step 4
    nc = w['ncell'].astype(np.float64)
    np.testing.assert_array_equal(got['volume'], nc * 10.0**3)
    np.testing.assert_array_equal(got['radius'], np.cbrt(3.0 * got['volume'] / (4.0 * np.pi)))
    np.testing.assert_array_equal(got['centres'], np.mod((w['core'] + w['offset_sum'] / nc[:, None]) * 10.0, L))
    np.testing.assert_array_equal(got['delta_mean'], got['delta_sum'] / nc)
    assert (got['centres'] >= 0).all() and (got['centres'] < L).all()
    dense, padded = lib.DeviceArray(mesh), lib.DeviceArray(_padded(mesh))
    try:
        a = watershed_mesh(dense, L, connectivity, return_labels=True)
        b = watershed_mesh(padded, L, connectivity, return_labels=True)
        c = watershed_mesh(padded, L, connectivity)
        _assert_equal(a, want, f'{name} n={n} c={connectivity} DeviceArray')
        _assert_equal(b, want, f'{name} n={n} c={connectivity} padded')
        _assert_equal(c, want, f'{name} n={n} c={connectivity} padded, no labels', labels=False)
        assert 'labels' not in c
        for k in st.INTEGER_KEYS:                                     # two calls: identical bytes for every integer output
            assert a[k].tobytes() == got[k].tobytes() == b[k].tobytes(), k
        assert dense.get().tobytes() == mesh.tobytes(), 'the mesh was modified'
        assert padded.get().tobytes() == _padded(mesh).tobytes(), 'the padded mesh was modified'
    finally:
        dense.free()
        padded.free()
    # what the cases are there for
    if (name, n, connectivity) in ZONES:
        assert w['nzones'] == ZONES[name, n, connectivity] and got['rounds'] >= 3
    elif name == 'quantised':
        assert len(np.unique(mesh)) < 16 and w['nzones'] > 10
    elif name == 'constant':
        assert w['nzones'] == 1 and got['core'].tolist() == [[0, 0, 0]] and got['ncell'].tolist() == [n**3] and got['rounds'] == 0
        assert got['offset_sum'].tolist() == [[-n**3 // 2] * 3] and got['delta_sum'][0] == -float(n**3) and len(got['saddle']) == 0
    elif name == 'zeros':
        assert np.signbit(mesh).any() and not np.signbit(mesh).all() and w['nzones'] == 1 and not np.signbit(got['delta_min']).any()
    elif name == 'corners':
        cores = {tuple(c) for c in got['core'].tolist()}
        assert set(st.corner_seeds(n)) <= cores and all({0, n - 1} <= {c[ax] for c in cores} for ax in range(3))
    elif name == 'two_wells':
        assert got['ncell'].tolist() == [320, 192] and got['saddle'].tolist() == [1.0] and got['hi_cell'].tolist() == [213]
    elif name == 'three_wells':
        assert got['ncell'].tolist() == [720, 576, 432] and got['saddle'].tolist() == [0.5, 1.5]


def test_reduce_without_combining_gives_the_same_sums(options):
    """ws_reduce_per_cell: the comparator that issues the atomics cell by cell instead of per run of one zone inside a wave"""
    from abacusutils_amd.analysis.watershed import watershed_mesh
    for name in ('white', 'constant'):
        want = _want(name, 24, 26)
        options.set('ws_reduce_per_cell')
        got = watershed_mesh(_mesh(name, 24), 240.0, 26, return_labels=True)
        options.reset()
        _assert_equal(got, want, f'{name} n=24 c=26 ws_reduce_per_cell')


# ------------------------------------------------------------------------------------------------- 2. from particles
def _condition(res, n):
    """the statement on the returned field gives the same result exactly, and the planted condition of the host test holds"""
    p = st.PLANTED
    field = res['field']
    assert field.shape == (n, n, n) and field.dtype == np.float32 and np.isfinite(field).all()
    return st.check_planted(res['labels'], res['core'], p['L'])


@pytest.mark.parametrize('connectivity', (26, 6))
@pytest.mark.parametrize('n', (16, 24))
def test_find_watershed_voids_end_to_end(n, connectivity):
    from abacusutils_amd.analysis.watershed import find_watershed_voids, merge_zones, persistence_pairs
    p = st.PLANTED
    pos = st.planted_points()
    before = pos.copy()
    got = find_watershed_voids(pos, p['L'], p['R'], nmesh=n, connectivity=connectivity, min_radius=30.0, saddle_max=-0.5, return_field=True,
                               return_labels=True)
    assert np.array_equal(pos, before)
    w = st.watershed(got['field'], connectivity)
    h = st.hierarchy(w, w, n)
    _assert_equal(got, (w, h), f'planted n={n} c={connectivity}')
    for k in h:
        assert got['hierarchy'][k].tobytes() == h[k].tobytes(), k
    zones = _condition(got, n)
    assert (got['delta_min'][zones] < -0.8).all()
    assert got['keep'].dtype == np.bool_ and np.array_equal(got['keep'], got['radius'] >= 30.0) and got['keep'][zones].all()
    m = merge_zones(got, -0.5)
    for k in m:
        assert np.array_equal(got['merged'][k], m[k]), k
    assert m['ncell'].sum() == n**3 and 1 <= m['nvoids'] <= got['nzones']
    pairs = persistence_pairs(got)
    assert np.array_equal(pairs[:, 0], got['delta_min']) and np.isinf(pairs[:, 1]).sum() == 1 and (pairs[:, 1] >= pairs[:, 0]).all()
    plain = find_watershed_voids(pos, p['L'], p['R'], nmesh=n, connectivity=connectivity)
    assert 'field' not in plain and 'labels' not in plain and 'merged' not in plain and plain['keep'].all()
    for k in st.INTEGER_KEYS[1:]:
        assert plain[k].tobytes() == got[k].tobytes(), k


# ------------------------------------------------------------------------------------------------- 3. AbacusHOD.compute_watershed_voids
class _Mock(dict):
    """a mock dictionary whose columns are also resident in HBM, as GRAND_HOD.MockDict.device_xyz hands them out"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.dev = {}

    def device_xyz(self, tracer):
        if tracer not in self.dev:
            self.dev[tracer] = [_lib().DeviceArray(np.ascontiguousarray(self[tracer][c], dtype=np.float64)) for c in 'xyz']
        return self.dev[tracer]


def test_abacus_hod_compute_watershed_voids():
    from abacusutils_amd.analysis.watershed import find_watershed_voids
    from abacusutils_amd.hod.abacus_hod import AbacusHOD
    p = st.PLANTED
    L, n, R = p['L'], 24, p['R']
    pos = np.floor(st.planted_points()[:6000] * 32.0) / 32.0           # multiples of 1 / 32: exact in float32
    w = np.random.default_rng(4).uniform(0.5, 1.5, 2500).astype(np.float32)
    cols = dict(LRG=dict(zip('xyz', pos.T.copy())), ELG=dict(zip('xyz', pos[:2500].T.copy()), w=w))
    before = {tr: {c: v.copy() for c, v in d.items()} for tr, d in cols.items()}
    ball = AbacusHOD.__new__(AbacusHOD)
    ball.lbox = L
    mock = _Mock(cols)
    try:
        dev = ball.compute_watershed_voids(mock, R, num_cells=n, saddle_max=-0.3, return_labels=True)
        assert set(mock.dev) == {'LRG', 'ELG'}                         # the columns came from HBM
        for tr in mock.dev:
            for c, col in zip('xyz', mock.dev[tr]):
                assert np.array_equal(col.get(), before[tr][c])
    finally:
        for d in mock.dev.values():
            for c in d:
                c.free()
    assert set(dev) == {'LRG', 'ELG'}
    for tr in cols:
        fetched = np.stack([cols[tr][c] for c in 'xyz'], axis=1)
        want = find_watershed_voids(fetched, L, R, nmesh=n, w=cols[tr].get('w'), saddle_max=-0.3, return_labels=True)
        assert dev[tr]['nzones'] == want['nzones'] >= 2
        for k in st.INTEGER_KEYS:
            assert dev[tr][k].tobytes() == want[k].tobytes(), (tr, k)
        for k in want['hierarchy']:
            assert dev[tr]['hierarchy'][k].tobytes() == want['hierarchy'][k].tobytes(), (tr, k)
        assert np.array_equal(dev[tr]['merged']['void'], want['merged']['void'])
        for c in before[tr]:
            assert np.array_equal(cols[tr][c], before[tr][c])
    assert dev['LRG']['labels'].tobytes() != dev['ELG']['labels'].tobytes()


# ------------------------------------------------------------------------------------------------- 4. errors
def test_errors_come_before_any_launch():
    import ctypes as C
    lib = _lib()
    L = lib.lib()
    n = 8
    some = lib.DeviceArray(np.full((n, n, n), -1.0, dtype=np.float32))
    handle = C.c_void_p()
    lib.check(L.abacus_ws_create(n, 26, C.byref(handle)))
    nz = C.c_int64(0)
    lib.sync()
    lib.profile_reset()
    lib.profile_enable(True)
    try:
        def refused(rc, match, entry):
            assert rc != 0
            msg = L.abacus_last_error().decode()
            assert msg.startswith(entry + ':') and match in msg, msg

        def create(n=n, conn=26, out=True):
            h = C.c_void_p()
            rc = L.abacus_ws_create(n, conn, C.byref(h) if out else None)
            assert rc != 0 and not h.value
            return rc

        for kw, match in ((dict(n=7), 'odd'), (dict(n=2), 'out of range'), (dict(n=1026), 'out of range'), (dict(conn=18), 'connectivity'),
                          (dict(out=False), 'null')):
            refused(create(**kw), match, 'abacus_ws_create')
        who = 'abacus_ws_run_dev'
        refused(L.abacus_ws_run_dev(handle, some.ptr, n - 1, C.byref(nz), None, None), 'pitch', who)
        refused(L.abacus_ws_run_dev(handle, None, n, C.byref(nz), None, None), 'null', who)
        refused(L.abacus_ws_run_dev(None, some.ptr, n, C.byref(nz), None, None), 'null', who)
        refused(L.abacus_ws_run_dev(handle, some.ptr, n, None, None, None), 'null', who)
        buf = np.zeros(8 * n**3, dtype=np.int64)
        refused(L.abacus_ws_fetch_zones(handle, *[lib.ptr(buf)] * 5), 'no finished', 'abacus_ws_fetch_zones')
        refused(L.abacus_ws_fetch_zones(handle, None, None, None, None, None), 'null', 'abacus_ws_fetch_zones')
        refused(L.abacus_ws_fetch_tree(handle, *[lib.ptr(buf)] * 5), 'no finished', 'abacus_ws_fetch_tree')
        refused(L.abacus_ws_fetch_labels(handle, lib.ptr(buf)), 'no finished', 'abacus_ws_fetch_labels')
        refused(L.abacus_ws_fetch_labels(handle, None), 'null', 'abacus_ws_fetch_labels')
        stale = C.c_void_p(handle.value)
        lib.check(L.abacus_ws_free(handle))
        refused(L.abacus_ws_run_dev(stale, some.ptr, n, C.byref(nz), None, None), 'not a live', who)
        refused(L.abacus_ws_fetch_zones(stale, *[lib.ptr(buf)] * 5), 'not a live', 'abacus_ws_fetch_zones')
        refused(L.abacus_ws_fetch_tree(stale, *[lib.ptr(buf)] * 5), 'not a live', 'abacus_ws_fetch_tree')
        refused(L.abacus_ws_fetch_labels(stale, lib.ptr(buf)), 'not a live', 'abacus_ws_fetch_labels')
        refused(L.abacus_ws_free(stale), 'not a live', 'abacus_ws_free')
        assert L.abacus_ws_free(None) == 0
        who = 'abacus_ws_check_memory'
        refused(L.abacus_ws_check_memory(7, 0), 'odd', who)
        refused(L.abacus_ws_check_memory(2048, 0), 'out of range', who)
        refused(L.abacus_ws_check_memory(16, -1), 'negative', who)
        refused(L.abacus_ws_check_memory(1024, 10**12), 'largest mesh that fits', who)
        names = lib.profile_get()
        assert not any(k.startswith('ws_') or k.startswith('scan_') for k in names), f'a kernel was launched: {names}'
    finally:
        lib.profile_enable(False)
        some.free()
