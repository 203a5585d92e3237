"""No-GPU checks of the watershed void finder: the NumPy statement tests/watershed_statement.py against itself (two routes to every
result), against closed forms and against a catalogue with planted voids; the host arithmetic of abacusutils_amd.analysis.watershed
(hierarchy, merging, size function, cross-correlation) and its argument checks, which raise before the library loads."""
import functools

import numpy as np
import pytest
import watershed_statement as st


def result_of(mesh, Lbox, connectivity=26):
    """the statement's result in the form `watershed_mesh` returns it"""
    from abacusutils_amd.analysis import watershed as ws
    w = st.watershed(mesh, connectivity)
    n = mesh.shape[0]
    out = {k: w[k] for k in st.DTYPES}
    out.update(nzones=w['nzones'], rounds=w['rounds'])
    out.update(ws._derived(out, float(Lbox), n))
    return out


# ------------------------------------------------------------------------------------------------- 1. the routes agree
@pytest.mark.parametrize('connectivity', (6, 26))
@pytest.mark.parametrize('name', ('white', 'quantised'))
@pytest.mark.parametrize('n', (6, 8))
def test_statement_routes_agree(n, name, connectivity):
    mesh = st.case_mesh(name, n)
    assert np.array_equal(st.descend_roll(mesh, connectivity), st.descend_loop(mesh, connectivity))
    a, b = st.watershed(mesh, connectivity, 'roll'), st.watershed(mesh, connectivity, 'loop')
    assert st.same(a, b) and np.array_equal(a['delta_sum'], b['delta_sum'])
    Z = a['nzones']
    assert Z >= 2 and len(a['saddle']) == Z - 1 and a['ncell'].sum() == n**3 and a['labels'].max() == Z - 1
    assert (a['zone_hi'] != a['zone_lo']).all()                       # every edge joins different zones
    w = np.lexsort((a['lo_cell'], st.keyed(mesh).ravel()[a['lo_cell']], a['hi_cell'], a['saddle']))
    assert np.array_equal(w, np.arange(Z - 1))                        # ascending weight
    for drop in range(Z - 1):                                         # a tree: without any one edge the zone graph falls apart
        parent = list(range(Z))
        for e in range(Z - 1):
            if e != drop:
                p, q = st._find(parent, int(a['zone_hi'][e])), st._find(parent, int(a['zone_lo'][e]))
                parent[max(p, q)] = min(p, q)
        assert len({st._find(parent, z) for z in range(Z)}) == 2
    # the cores are the zones' minima, and every zone is connected to its core through `down`
    flat = st.keyed(mesh).ravel()
    for z in range(Z):
        cells = np.flatnonzero(a['labels'].ravel() == z)
        c = a['core'][z]
        assert flat[cells].min() == a['delta_min'][z] == flat[(c[0] * n + c[1]) * n + c[2]]


def test_zone_counts_of_the_white_meshes():
    """the counts the device tests rely on"""
    for n, connectivity, Z in ((16, 26, 85), (16, 6, 208), (24, 26, 289), (24, 6, 726)):
        down = st.descend_roll(st.case('white', n), connectivity)
        assert (down == np.arange(n**3)).sum() == Z


# ------------------------------------------------------------------------------------------------- 2. closed forms
@pytest.mark.parametrize('connectivity', (6, 26))
def test_constant_and_ramp_are_one_zone(connectivity):
    from abacusutils_amd.analysis.watershed import zone_hierarchy
    n = 8
    for mesh in (np.full((n, n, n), -1.0, dtype=np.float32), np.broadcast_to(np.arange(n, dtype=np.float32)[:, None, None], (n, n, n)).copy(),
                 np.broadcast_to(np.arange(n, dtype=np.float32)[None, None, :], (n, n, n)).copy()):
        w = st.watershed(mesh, connectivity)
        assert w['nzones'] == 1 and w['core'].tolist() == [[0, 0, 0]] and w['ncell'].tolist() == [n**3] and len(w['saddle']) == 0
        assert (w['labels'] == 0).all() and w['delta_sum'][0] == mesh.astype(np.float64).sum()
        # every offset -4 .. 3 equally often on every axis
        assert w['offset_sum'].tolist() == [[-n**3 // 2] * 3]
        h = zone_hierarchy(result_of(mesh, 100.0, connectivity))
        assert h['parent'].tolist() == [-1] and h['saddle'].tolist() == [np.inf] and h['ncell_at_merge'].tolist() == [n**3]


@pytest.mark.parametrize('connectivity', (6, 26))
def test_two_wells(connectivity):
    from abacusutils_amd.analysis.watershed import merge_zones, persistence_pairs, zone_hierarchy
    mesh, n = st.two_wells(), 8
    res = result_of(mesh, 80.0, connectivity)
    # A: the slab x = 0 .. 2 and both walls; B: the slab x = 4 .. 6
    assert res['nzones'] == 2 and res['core'].tolist() == [[1, 4, 4], [5, 4, 4]] and res['ncell'].tolist() == [5 * n * n, 3 * n * n]
    assert res['delta_min'].tolist() == [-5.0, -4.0]
    # one edge through the gate (3, 2, 5); lo is the lowest neighbour of the gate in B: (4, 2, 5) through the face, and (4, 3, 4), the
    # one nearest to B's bottom, among the 26
    lo = (4, 2, 5) if connectivity == 6 else (4, 3, 4)
    assert res['hi_cell'].tolist() == [(3 * n + 2) * n + 5] and res['lo_cell'].tolist() == [(lo[0] * n + lo[1]) * n + lo[2]]
    assert res['saddle'].tolist() == [1.0] and res['zone_hi'].tolist() == [0] and res['zone_lo'].tolist() == [1]
    h = zone_hierarchy(res)
    assert h['parent'].tolist() == [-1, 0] and h['saddle'].tolist() == [np.inf, 1.0] and h['saddle_cell'].tolist() == [-1, (3 * n + 2) * n + 5]
    assert h['ncell_at_merge'].tolist() == [n**3, 3 * n * n] and h['nzones_at_merge'].tolist() == [2, 1]
    assert h['persistence'].tolist() == [np.inf, 5.0] and h['ratio'][1] == 2.0 / -3.0
    assert st.hierarchy(res, res, n)['parent'].tolist() == [-1, 0]
    assert persistence_pairs(res).tolist() == [[-5.0, np.inf], [-4.0, 1.0]] and persistence_pairs(res).dtype == np.float32
    # x offsets of B around x = 5: -1, 0, 1 equally often; A around x = 1: -1, 0, 1, 2 (x = 3) and -2 (x = 7)
    assert res['offset_sum'][:, 0].tolist() == [0, 0]
    assert merge_zones(res, 1.0)['nvoids'] == 2 and merge_zones(res, 1.0 + 1e-6)['nvoids'] == 1     # saddle < saddle_max, strictly


@pytest.mark.parametrize('connectivity', (6, 26))
def test_three_wells(connectivity):
    from abacusutils_amd.analysis.watershed import merge_zones, zone_hierarchy
    mesh, n, L = st.three_wells(), 12, 120.0
    res = result_of(mesh, L, connectivity)
    assert res['nzones'] == 3 and res['core'].tolist() == [[1, 6, 6], [5, 6, 6], [9, 6, 6]]
    assert res['ncell'].tolist() == [5 * n * n, 4 * n * n, 3 * n * n]       # A: its slab and the walls x = 3, 11; B: its slab and x = 7
    # rising water joins A and B through the gate of height 0.5, then C through the gate of 1.5; the wall between C and A (3.0) never
    assert res['saddle'].tolist() == [0.5, 1.5] and res['hi_cell'].tolist() == [(3 * n + 1) * n + 1, (7 * n + 2) * n + 2]
    assert res['zone_hi'].tolist() == [0, 1] and res['zone_lo'].tolist() == [1, 2]
    h = zone_hierarchy(res)
    want = st.hierarchy(res, res, n)
    for k in want:
        assert h[k].dtype == want[k].dtype and np.array_equal(h[k], want[k]), k
    assert h['parent'].tolist() == [-1, 0, 0] and h['saddle'].tolist() == [np.inf, 0.5, 1.5]
    assert h['ncell_at_merge'].tolist() == [n**3, 4 * n * n, 3 * n * n] and h['nzones_at_merge'].tolist() == [3, 1, 1]
    assert h['persistence'].tolist() == [np.inf, 4.5, 4.5]
    below, between, above = merge_zones(res, 0.25), merge_zones(res, 1.0), merge_zones(res, 2.0)
    assert below['void'].tolist() == [0, 1, 2] and between['void'].tolist() == [0, 0, 1] and above['void'].tolist() == [0, 0, 0]
    assert between['ncell'].tolist() == [9 * n * n, 3 * n * n] and between['zone'].tolist() == [0, 2] and between['delta_min'].tolist() == [-5.0, -3.0]
    assert above['ncell'].tolist() == [n**3] and above['core'].tolist() == [[1, 6, 6]]
    a = L / n
    np.testing.assert_array_equal(below['centres'], res['centres'])
    np.testing.assert_allclose(between['volume'], np.array([9.0, 3.0]) * n * n * a**3, rtol=1e-15)
    np.testing.assert_allclose(between['radius'], np.cbrt(3.0 * between['volume'] / (4.0 * np.pi)), rtol=1e-15)
    # the barycentre of A + B: the cells x = 11, 0, .. 7, every (y, z) once: x = 3 from A's core at 1, y and z offsets -6 .. 5: -0.5
    np.testing.assert_allclose(between['centres'][0], np.array([3.0, 5.5, 5.5]) * a, rtol=1e-14)
    np.testing.assert_allclose(between['centres'][1], np.array([9.0, 5.5, 5.5]) * a, rtol=1e-14)


# ------------------------------------------------------------------------------------------------- 3. planted voids
@functools.lru_cache(maxsize=None)
def planted_statement(n, connectivity):
    p = st.PLANTED
    field = st.gaussian_mesh(st.nearest_cell_contrast(st.planted_points(), p['L'], n), p['L'], p['R'])
    return st.watershed(field, connectivity)


@pytest.mark.parametrize('connectivity', (6, 26))
@pytest.mark.parametrize('n', (16, 24))
def test_planted_voids(n, connectivity):
    w = planted_statement(n, connectivity)
    zones = st.check_planted(w['labels'], w['core'], st.PLANTED['L'])
    assert (w['delta_min'][zones] < -0.8).all()


# ------------------------------------------------------------------------------------------------- 4. the interface
def test_size_function_arithmetic():
    from abacusutils_amd.analysis.watershed import watershed_size_function
    bins, L = np.array([5.0, 10.0, 20.0, 40.0]), 1000.0
    radius = np.array([5.0, 7.0, 9.99, 10.0, 25.0, 39.0, 40.0, 3.0, 50.0])       # an edge belongs to the bin above it
    got = watershed_size_function(radius, bins, L)
    assert got['counts'].tolist() == [3, 1, 2] and got['counts'].dtype == np.int64
    np.testing.assert_allclose(got['dn_dlnR'], np.array([3.0, 1.0, 2.0]) / (1e9 * np.log(2.0)), rtol=1e-15)
    np.testing.assert_allclose(got['error'], np.sqrt([3.0, 1.0, 2.0]) / (1e9 * np.log(2.0)), rtol=1e-15)
    np.testing.assert_allclose(got['R'], np.sqrt(bins[1:] * bins[:-1]), rtol=1e-15)
    assert watershed_size_function(np.zeros(0), bins, L)['counts'].tolist() == [0, 0, 0]
    for bad in ([5.0], [10.0, 5.0], [0.0, 5.0], [5.0, np.nan], [5.0, 5.0]):
        with pytest.raises(ValueError, match='bins'):
            watershed_size_function(radius, bad, L)
    for bad in (np.array([-1.0]), np.array([np.nan]), np.ones((2, 2))):
        with pytest.raises(ValueError, match='radii'):
            watershed_size_function(bad, bins, L)
    with pytest.raises(ValueError, match='Lbox'):
        watershed_size_function(radius, bins, 0.0)


def test_zone_galaxy_xi_normalisation(monkeypatch):
    from abacusutils_amd.analysis import tpcf_corrfunc, watershed
    L, bins = 100.0, np.array([0.0, 5.0, 10.0, 20.0])
    centres = np.array([[1.0, 2.0, 3.0], [50.0, 60.0, 70.0], [99.0, 98.0, 97.0], [10.0, 10.0, 10.0]])
    x = np.linspace(0, 99, 25).astype(np.float32)
    seen = {}

    def DD(autocorr, nthreads, b, X1, Y1, Z1, X2=None, Y2=None, Z2=None, periodic=None, boxsize=None):
        seen.update(autocorr=autocorr, first=np.stack([X1, Y1, Z1], axis=1), second=(X2, Y2, Z2), periodic=periodic, boxsize=boxsize, bins=b)
        return dict(npairs=np.array([2, 7, 40], dtype=np.uint64))

    monkeypatch.setattr(tpcf_corrfunc, 'DD', DD)
    for select, nz in ((None, 4), (np.array([True, False, True, True]), 3), ([1, 3], 2)):
        got = watershed.zone_galaxy_xi(dict(centres=centres), x, x, x, L, bins, select=select)
        want = centres if select is None else centres[np.asarray(select)]
        assert seen['autocorr'] == 0 and seen['periodic'] is True and seen['boxsize'] == L and seen['second'][0] is x
        assert seen['first'].dtype == np.float32 and np.array_equal(seen['first'], want.astype(np.float32))     # the centres are the first set
        dV = 4.0 * np.pi / 3.0 * (bins[1:] ** 3 - bins[:-1] ** 3)
        np.testing.assert_allclose(got['xi'], np.array([2.0, 7.0, 40.0]) / (nz * 25 * dV / L**3) - 1.0, rtol=1e-15)
        assert got['nzones'] == nz and got['ngal'] == 25 and got['npairs'].tolist() == [2, 7, 40]
        np.testing.assert_array_equal(got['r'], [2.5, 7.5, 15.0])


def test_argument_checks_come_before_the_library(monkeypatch):
    from abacusutils_amd import _lib
    from abacusutils_amd.analysis import tpcf_corrfunc, watershed as ws
    from abacusutils_amd.hod.abacus_hod import AbacusHOD

    def loaded(*a, **kw):
        raise AssertionError('the library was loaded')

    monkeypatch.setattr(_lib, 'lib', loaded)
    monkeypatch.setattr(tpcf_corrfunc, 'DD', loaded)
    pos, mesh = np.zeros((10, 3), dtype=np.float32), np.zeros((8, 8, 8), dtype=np.float32)
    for kw in (dict(Lbox=0.0), dict(Lbox=-1.0), dict(Lbox=np.inf), dict(Lbox=np.nan), dict(connectivity=18), dict(connectivity=0)):
        with pytest.raises(ValueError):
            ws.watershed_mesh(mesh, **dict(dict(Lbox=100.0), **kw))
        with pytest.raises(ValueError):
            ws.find_watershed_voids(pos, **dict(dict(Lbox=100.0, R=5.0, nmesh=16), **kw))
    for bad, exc in ((np.zeros((8, 8, 4), dtype=np.float32), ValueError), (np.zeros((8, 8, 8)), TypeError), (np.zeros((7, 7, 7), dtype=np.float32), ValueError),
                     (np.zeros((2, 2, 2), dtype=np.float32), ValueError), (np.zeros((8, 8), dtype=np.float32), ValueError), ([mesh], TypeError), (3.0, TypeError),
                     (np.full((8, 8, 8), np.nan, dtype=np.float32), ValueError), (np.full((8, 8, 8), np.inf, dtype=np.float32), ValueError),
                     (np.full((8, 8, 8), -np.inf, dtype=np.float32), ValueError)):
        with pytest.raises(exc):
            ws.watershed_mesh(bad, 100.0)
    one_nan = mesh.copy()
    one_nan[7, 7, 7] = np.nan
    with pytest.raises(ValueError, match='NaN or inf'):
        ws.watershed_mesh(one_nan, 100.0)
    dev = _lib.DeviceArray.view(4096, np.float32, (8, 8, 16))           # a device mesh of a pitch that is neither dense nor padded
    with pytest.raises(ValueError, match='dense'):
        ws.watershed_mesh(dev, 100.0)
    with pytest.raises(TypeError, match='float32'):
        ws.watershed_mesh(_lib.DeviceArray.view(4096, np.float64, (8, 8, 8)), 100.0)
    ok = dict(Lbox=100.0, R=5.0, nmesh=16)
    for kw in (dict(R=-1.0), dict(R=np.nan), dict(R=np.inf), dict(nmesh=2), dict(nmesh=15), dict(nmesh=1026), dict(min_radius=-1.0),
               dict(min_radius=np.nan), dict(saddle_max=np.nan)):
        with pytest.raises(ValueError):
            ws.find_watershed_voids(pos, **dict(ok, **kw))
    with pytest.raises(ValueError, match='Unknown pasting'):
        ws.find_watershed_voids(pos, paste='NGP', **ok)
    with pytest.raises(ValueError, match='shape'):
        ws.find_watershed_voids(np.zeros((10, 2), dtype=np.float32), **ok)
    with pytest.raises(ValueError, match='weights'):
        ws.find_watershed_voids(pos, w=np.ones(9), **ok)
    ball = AbacusHOD.__new__(AbacusHOD)
    ball.lbox = 100.0
    mock = dict(LRG=dict(zip('xyz', np.zeros((3, 10)))))
    for kw in (dict(R=-1.0), dict(R=5.0, num_cells=15), dict(R=5.0, connectivity=7)):
        with pytest.raises(ValueError):
            ball.compute_watershed_voids(mock, **kw)
    res = result_of(st.two_wells(), 80.0)
    for f in (ws.zone_hierarchy, ws.persistence_pairs, lambda r: ws.merge_zones(r, 0.0)):
        with pytest.raises(ValueError, match='result of watershed_mesh'):
            f(dict(ncell=res['ncell']))
        with pytest.raises(ValueError, match='edges'):
            f(dict(res, saddle=res['saddle'][:0]))
    with pytest.raises(ValueError, match='NaN'):
        ws.merge_zones(res, np.nan)
    x = np.zeros(5, dtype=np.float32)
    for bins in ((1.0,), (2.0, 1.0), (-1.0, 1.0)):
        with pytest.raises(ValueError, match='bins'):
            ws.zone_galaxy_xi(res, x, x, x, 80.0, bins)
    with pytest.raises(ValueError, match='no zone'):
        ws.zone_galaxy_xi(res, x, x, x, 80.0, (1.0, 2.0), select=np.zeros(2, dtype=bool))
    with pytest.raises(ValueError, match='centres'):
        ws.zone_galaxy_xi(dict(centres=np.zeros(3)), x, x, x, 80.0, (1.0, 2.0))


def test_compute_watershed_voids_has_no_cpu_fallback():
    """without a GPU the call raises; with one it runs on it"""
    from abacusutils_amd import _lib
    from abacusutils_amd.hod.abacus_hod import AbacusHOD
    ball = AbacusHOD.__new__(AbacusHOD)
    ball.lbox = 100.0
    pts = np.random.default_rng(3).uniform(0, 100.0, (500, 3))
    mock = dict(LRG=dict(zip('xyz', pts.T.copy())))
    if _lib.device_count() > 0:
        assert set(ball.compute_watershed_voids(mock, 10.0, num_cells=16)['LRG']) >= {'ncell', 'core', 'saddle', 'hierarchy', 'keep', 'nzones'}
        return
    with pytest.raises(_lib.AbacusHipError, match='no HIP device'):
        ball.compute_watershed_voids(mock, 10.0, num_cells=16)
