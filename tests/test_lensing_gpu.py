"""Galaxy-galaxy lensing on the device (csrc/lens.hip: lens_walk, C ABI abacus_lens_*; analysis/lensing.py) against the NumPy
statement tests/lensing_statement.py and against the device's own cylinder counts and weighted pair counts.  Needs an MI355X:
run with `-m gpu`.

npairs is compared exactly.  wsum: with unit weights and masses it must equal npairs exactly; otherwise per row
|device - statement| <= npairs * 2^-52 * sum |term|: n float64 additions in any order err by at most (n - 1) 2^-53 sum |t| to
first order, the factor 2 covers the higher orders and the one rounding of the statement's fsum."""
import functools

import numpy as np
import pytest
from lensing_statement import projected_sums as statement

pytestmark = pytest.mark.gpu

BOX = 100.0
EDGES = np.geomspace(0.5, 20.0, 9).astype(np.float32)      # 8 logarithmic bins
EPS = 2.0 ** -52


def _uniform(n, box, seed, dims=2):
    p = np.random.default_rng(seed).random((n, dims)) * box
    return [p[:, d].copy() for d in range(dims)]


def _mass(n, seed):
    return (0.5 + np.random.default_rng(seed).random(n)).astype(np.float32)


def _signed(n, seed):
    return (2.0 * np.random.default_rng(seed).random(n) - 0.6).astype(np.float32)     # about 30 % negative


@functools.lru_cache(maxsize=None)
def _catalogue(frame):
    """3000 clustered particles and 300 galaxies in a box of 100, in the frame [0, L), [-L/2, L/2) or spilling over both edges"""
    from test_pairs_weighted_gpu import _frame, _points
    p, g = _points(3000, BOX, 81)[:2], _points(300, BOX, 82)[:2]
    if frame != 0.0:
        p, g = _frame(p, frame, BOX, 1), _frame(g, frame, BOX, 4)
    return p, g


def _device(p, g, box, edges, rmax=None, pm=None, gw=None):
    """(npairs, wsum, candidates, cells per dimension) of a fresh handle"""
    from abacusutils_amd.analysis import lensing as S
    with S.ProjectedParticles(p[0], p[1], box, float(np.float32(edges[-1])) if rmax is None else rmax, mass=pm) as parts:
        res = S.projected_sums(parts, g[0], g[1], edges, weights=gw)
        cand, nc = S.walk_stats()
    assert res['npairs'].dtype == np.uint64 and res['wsum'].dtype == np.float64
    assert res['npairs'].shape == res['wsum'].shape == (len(edges),)
    return res['npairs'], res['wsum'], cand, nc


def _judge(got, want, unit):
    npairs, wsum = got[0], got[1]
    n_s, w_s, a_s = want
    np.testing.assert_array_equal(npairs, n_s)
    if unit:
        np.testing.assert_array_equal(wsum, npairs.astype(np.float64))
        return
    err, bound = np.abs(wsum - w_s), n_s.astype(np.float64) * EPS * a_s
    print('wsum error / bound per row:', np.array2string(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0), precision=3))
    assert np.all(err <= bound), (err, bound)


def _check(p, g, box, edges, rmax=None, pm=None, gw=None, want=None):
    f4 = lambda a: a.get() if hasattr(a, 'get') else a       # noqa: E731
    if want is None:
        want = statement(f4(p[0]), f4(p[1]), f4(g[0]), f4(g[1]), box, edges, pm=None if pm is None else f4(pm), gw=None if gw is None else f4(gw))
    got = _device(p, g, box, edges, rmax, pm, gw)
    _judge(got, want, pm is None and gw is None)
    return got


@pytest.mark.parametrize('frame', [0.0, -50.0, 'unwrapped'])
def test_general_case_in_every_frame(frame):
    """masses and signed weights, 4 cells per dimension: host columns, then DeviceArray columns of float32 and of float64 with
    host and with resident masses and weights"""
    from abacusutils_amd import _lib
    p, g = _catalogue(frame)
    pm, gw = _mass(3000, 1), _signed(300, 2)
    want = statement(*p, *g, BOX, EDGES, pm=pm, gw=gw)
    assert np.all(want[0] > 0) and (gw < 0).any()
    npairs, wsum, cand, nc = _check(p, g, BOX, EDGES, pm=pm, gw=gw, want=want)
    assert nc >= 3 and cand >= npairs.sum()
    assert cand < 3000 * 300                                 # a walk over the neighbour cells, not over the box
    for dt in (np.float32, np.float64):
        own = [_lib.DeviceArray(np.ascontiguousarray(c, dtype=dt)) for c in p + g]
        own += [_lib.DeviceArray(pm), _lib.DeviceArray(gw)]
        try:
            _check(own[:2], own[2:4], BOX, EDGES, pm=pm, gw=gw, want=want)
            _check(own[:2], own[2:4], BOX, EDGES, pm=own[4], gw=own[5], want=want)
            _check(own[:2], g, BOX, EDGES, pm=own[4], gw=gw, want=want)     # a resident handle serves host galaxies
        finally:
            for a in own:
                a.free()
    with pytest.raises(TypeError):
        dx = _lib.DeviceArray(np.ascontiguousarray(p[0], dtype=np.float32))
        try:
            _device([dx, p[1]], g, BOX, EDGES)
        finally:
            dx.free()


@pytest.mark.parametrize('last', [40.0, 50.0])
def test_one_cell_that_is_its_own_neighbour(last):
    """last edge 0.4 L: fewer than three cells fit, the grid is one cell; and the last edge exactly L / 2"""
    p, g = _uniform(1500, 100.0, 21), _uniform(300, 100.0, 22)
    edges = np.geomspace(2.0, last, 7)
    npairs, _, cand, nc = _check(p, g, 100.0, edges, pm=_mass(1500, 3))
    assert nc == 1 and cand == 1500 * 300
    if last == 50.0:
        _check(p, g, 100.0, edges, rmax=50.0)


@pytest.mark.parametrize('ng', [1, 255, 257])
def test_galaxy_counts_around_a_slice(ng):
    p = _catalogue(0.0)[0]
    _check(p, _uniform(ng, BOX, 30 + ng), BOX, EDGES, pm=_mass(3000, 4), gw=_signed(ng, 5))


def test_many_galaxies_in_one_cell():
    """600 galaxies inside one cell of the grid (a cell is 25 wide): ten slices of 64 over the four waves of a workgroup"""
    p = _catalogue(0.0)[0]
    g = [10.0 + 2.0 * c / BOX for c in _uniform(600, BOX, 41)]          # all in [10, 12)^2
    _, _, cand, nc = _check(p, g, BOX, EDGES, pm=_mass(3000, 6), gw=_signed(600, 7))
    assert nc == 4


def test_a_crowded_cell_and_an_empty_neighbourhood():
    """one cell with 5000 particles - hundreds of scalar-load tiles and a remainder - around one galaxy, and no particle within
    reach of the other"""
    rng = np.random.default_rng(43)
    blob = 50.0 + rng.normal(0, 0.4, (5003, 2))                       # a cell is 10.5 wide and spans 42.1 .. 52.6
    far = 150.0 + 40.0 * (rng.random((300, 2)) - 0.5)
    far = far[np.linalg.norm(far - 150.0, axis=1) > 12.0]
    pts = np.concatenate([blob, far])
    p = [pts[:, 0].copy(), pts[:, 1].copy()]
    g = [np.array([50.0, 150.0]), np.array([50.0, 150.0])]
    pm = _mass(len(pts), 8)
    npairs, wsum, _, nc = _check(p, g, 200.0, [1.0, 3.0, 10.0], pm=pm)
    assert nc >= 3 and npairs.sum() > 4900
    lone = statement(p[0], p[1], g[0][:1], g[1][:1], 200.0, [1.0, 3.0, 10.0], pm=pm)
    np.testing.assert_array_equal(npairs, lone[0])                        # the second galaxy adds nothing


@pytest.mark.parametrize('nb', [1, 32])
def test_extreme_bin_counts(nb):
    """one bin (two rows) and 32 (33 rows, the largest accumulator)"""
    p, g = _catalogue(0.0)
    edges = [2.0, 20.0] if nb == 1 else np.geomspace(0.5, 20.0, 33)
    npairs, _, _, _ = _check(p, g, BOX, edges, pm=_mass(3000, 9), gw=_signed(300, 10))
    assert npairs.shape == (nb + 1,)
    _check(p, g, BOX, edges)
    edges = [2.0, 20.0] if nb == 1 else np.linspace(0.5, 20.0, 33)        # linear bins: a finer look-up table
    _check(p, g, BOX, edges, pm=_mass(3000, 9))


def test_edges_too_close_for_the_table():
    """two edges an ulp apart next to a far one: no table of 1024 cells separates them, the lanes walk on through the edges"""
    p, g = _catalogue(0.0)
    e = np.float32(5.0)
    edges = np.array([e, np.nextafter(e, np.float32(10)), 12.0, np.nextafter(np.float32(12.0), np.float32(20)), 20.0], np.float32)
    npairs, _, _, _ = _check(p, g, BOX, edges, pm=_mass(3000, 11))
    assert npairs[0] > 0 and npairs[2] > 0 and npairs[4] > 0
    # a particle exactly ON an edge and one an ulp of r2 inside it
    _check([[3.0, 3.0], [4.0, np.nextafter(np.float32(4.0), np.float32(0))]], [[0.0], [0.0]], BOX, edges)


@pytest.mark.parametrize('masses,weights', [(True, True), (True, False), (False, True), (False, False)])
def test_weights_and_masses(masses, weights):
    """every combination of given and unit masses and weights; with both unit the sums are the counts, exactly"""
    p, g = _catalogue(0.0)
    _check(p, g, BOX, EDGES, pm=_mass(3000, 12) if masses else None, gw=_signed(300, 13) if weights else None)


def test_strict_upper_edge():
    up = np.nextafter(np.float32(5.0), np.float32(np.inf))
    npairs, wsum, _, _ = _check([[3.0], [4.0]], [[0.0], [0.0]], 100.0, [1.0, 5.0, up], pm=[2.5], gw=[-2.0])
    np.testing.assert_array_equal(npairs, [0, 0, 1])
    np.testing.assert_array_equal(wsum, [0.0, 0.0, -5.0])


def test_shared_rows_comparator(options):
    """the comparator reduction - one set of rows per workgroup, an LDS atomic per pair - gives the same rows"""
    p, g = _catalogue(0.0)
    pm, gw = _mass(3000, 14), _signed(300, 15)
    want = statement(*p, *g, BOX, EDGES, pm=pm, gw=gw)
    options.set('lens_shared_rows')
    _check(p, g, BOX, EDGES, pm=pm, gw=gw, want=want)
    _check(p, g, BOX, EDGES)
    options.reset()
    _check(p, g, BOX, EDGES, pm=pm, gw=gw, want=want)


def test_one_handle_many_calls_and_empty_sets():
    """one handle, two galaxy sets and two sets of edges - one far below its rmax - each as a fresh handle and the statement
    give it; a call after free() raises; n = 0 and ng = 0 give zeros"""
    from abacusutils_amd.analysis import lensing as S
    p, g = _catalogue(0.0)
    g2 = _uniform(257, BOX, 51)
    pm = _mass(3000, 16)
    short = np.geomspace(0.3, 3.0, 5).astype(np.float32)
    with S.ProjectedParticles(p[0], p[1], BOX, 20.0, mass=pm) as parts:
        total = pm.astype(np.float64).sum()
        assert parts.n == 3000 and abs(parts.mass_sum - total) <= 3000 * EPS * total     # a float64 sum in another order
        for gal, edges in ((g, EDGES), (g2, short), (g, short), (g2, EDGES), (g, EDGES)):
            res = S.projected_sums(parts, gal[0], gal[1], edges)
            assert S.walk_stats()[1] == 4                                # the handle's grid, whatever the edges
            want = statement(*p, *gal, BOX, edges, pm=pm)
            _judge((res['npairs'], res['wsum']), want, False)
            fresh = _device(p, gal, BOX, edges, pm=pm)                  # its own grid: the short edges get 33 cells per dimension
            np.testing.assert_array_equal(res['npairs'], fresh[0])
        with pytest.raises(ValueError):
            S.projected_sums(parts, g[0], g[1], [1.0, 20.5])          # beyond the handle's rmax
        none = S.projected_sums(parts, np.zeros(0), np.zeros(0), EDGES)
        assert not none['npairs'].any() and not none['wsum'].any() and S.walk_stats() == (0, 0)
    with pytest.raises(ValueError, match='freed'):
        S.projected_sums(parts, g[0], g[1], EDGES)
    parts.free()                                                        # twice is harmless
    with S.ProjectedParticles(np.zeros(0), np.zeros(0), BOX, 20.0) as empty:
        assert empty.n == 0 and empty.mass_sum == 0.0
        res = S.projected_sums(empty, g[0], g[1], EDGES, weights=_signed(300, 17))
        assert not res['npairs'].any() and not res['wsum'].any() and res['npairs'].shape == (9,)


def test_against_the_cylinder_counts_and_the_weighted_pair_counts():
    """z in [0, 0.2 L): cumsum(npairs) is the device's own count in cylinders of half-height L / 2 summed over the galaxies, and
    the rows of the bins are the weighted (rp, pi) cross count with pimax = L / 2 and one pi bin - counts exactly, sums within the
    bound (both are sums of the same exact products)"""
    from abacusutils_amd.analysis.spheres import count_in_spheres
    from abacusutils_amd.analysis.tpcf_corrfunc import _paircount_weighted
    p, g = _catalogue(0.0)
    pz, gz = _uniform(3000, 0.2 * BOX, 61, 1)[0], _uniform(300, 0.2 * BOX, 62, 1)[0]
    pm, gw = _mass(3000, 18), _signed(300, 19)
    want = statement(*p, *g, BOX, EDGES, pm=pm, gw=gw)
    npairs, wsum, _, _ = _check(p, g, BOX, EDGES, pm=pm, gw=gw, want=want)
    cyl = count_in_spheres(p[0], p[1], pz, BOX, EDGES, g[0], g[1], gz, pimax=BOX / 2, return_counts=True)['counts']
    np.testing.assert_array_equal(np.cumsum(npairs), cyl.sum(axis=0, dtype=np.uint64))
    dd, ww, _ = _paircount_weighted(1, g[0], g[1], gz, BOX, EDGES, p[0], p[1], pz, W1=gw, W2=pm, pimax=BOX / 2, npibins=1)
    np.testing.assert_array_equal(npairs[1:], dd)
    bound = want[0][1:].astype(np.float64) * EPS * want[2][1:]
    assert np.all(np.abs(ww - want[1][1:]) <= bound) and np.all(np.abs(ww - wsum[1:]) <= 2 * bound)


def test_delta_sigma_box_and_the_line_of_sight():
    """delta_sigma_box(los='x') is the call on the (y, z) columns, (n, 3) arrays and column lists alike; sigma_box is the mean
    surface density of the box"""
    from abacusutils_amd.analysis import lensing as S
    rng = np.random.default_rng(71)
    part, gal = rng.random((3000, 3)) * BOX, rng.random((300, 3)) * BOX
    pm = _mass(3000, 20)
    out = S.delta_sigma_box(gal, part, BOX, EDGES, los='x', mass=pm, particle_mass=2.0)
    with S.ProjectedParticles(part[:, 1], part[:, 2], BOX, 20.0, mass=pm) as parts:
        ref = S.delta_sigma(parts, gal[:, 1], gal[:, 2], EDGES, particle_mass=2.0)
    cols = S.delta_sigma_box([gal[:, d] for d in range(3)], [part[:, d] for d in range(3)], BOX, EDGES, los='x', mass=pm, particle_mass=2.0)
    want = statement(part[:, 1], part[:, 2], gal[:, 1], gal[:, 2], BOX, EDGES, pm=pm)
    for o in (out, ref, cols):
        _judge((o['npairs'], o['wsum']), want, False)
        assert o['wgal'] == 300.0 and abs(o['sigma_box'] / (2.0 * pm.astype(np.float64).sum() / BOX ** 2) - 1) <= 3000 * EPS
        again = S.delta_sigma_from_sums(o['wsum'], EDGES, 300.0, particle_mass=2.0)
        for k in ('sigma', 'sigma_mean', 'delta_sigma', 'rp_mid'):
            np.testing.assert_array_equal(o[k], again[k])
    assert not np.array_equal(out['npairs'], S.delta_sigma_box(gal, part, BOX, EDGES, los='z')['npairs'])
    # a uniform box: Sigma scatters around sigma_box
    assert np.all(np.abs(out['sigma'][-3:] / out['sigma_box'] - 1) < 0.1)


def test_abacus_hod_compute_delta_sigma():
    """AbacusHOD.compute_delta_sigma: the catalogue still in HBM gives what its host columns give.  Counts exactly; the sums of
    both calls are within npairs 2^-52 sum |t| of the exact sum of the same positive terms, so within twice that of each other"""
    from test_abacus_hod_gpu import CLUSTERING, HOD_PARAMS

    from abacusutils_amd import synth
    from abacusutils_amd.analysis import lensing as S
    from abacusutils_amd.hod.abacus_hod import AbacusHOD
    hd, pd, params = synth.synth_hod_inputs(100000, 100000, seed=19, lbox=1000.0)
    hod = dict(HOD_PARAMS, LRG_params=dict(synth.LRG_PARAMS, logM_cut=12.3, logM1=13.3), ELG_params=dict(synth.ELG_PARAMS))
    ball = AbacusHOD.from_arrays(hd, pd, params, hod, CLUSTERING)
    mock = ball.run_hod()
    assert all(mock.device_xyz(tr) is not None for tr in mock)
    plain = {tr: dict(mock[tr]) for tr in mock}
    part = _uniform(20000, 1000.0, 91)
    pm = _mass(20000, 92)
    bins = np.geomspace(1.0, 30.0, 7)
    with S.ProjectedParticles(part[0] - 500.0, part[1] - 500.0, ball.lbox, 30.0, mass=pm) as parts:
        got, want = ball.compute_delta_sigma(mock, parts, bins, particle_mass=3.0), ball.compute_delta_sigma(plain, parts, bins, particle_mass=3.0)
        assert set(got) == set(want) == set(mock)
        first = next(iter(mock))
        assert set(ball.compute_delta_sigma(mock, parts, bins, tracers=[first])) == {first}
        for tr in mock:
            direct = S.delta_sigma(parts, np.asarray(plain[tr]['x']), np.asarray(plain[tr]['y']), bins, particle_mass=3.0)
            for other in (want[tr], direct):
                np.testing.assert_array_equal(got[tr]['npairs'], other['npairs'])
                tol = 2 * got[tr]['npairs'].astype(np.float64) * EPS * np.abs(other['wsum'])
                assert np.all(np.abs(got[tr]['wsum'] - other['wsum']) <= tol)
                assert got[tr]['sigma_box'] == other['sigma_box'] == 3.0 * parts.mass_sum / ball.lbox ** 2
            assert got[tr]['npairs'].sum() > 0 and got[tr]['delta_sigma'].shape == (6,)
