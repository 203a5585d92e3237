"""The 3PCF multipoles on the device (csrc/threepcf.hip: threepcf_walk, C ABI abacus_threepcf[_dev]; analysis/threepcf.py) against
the NumPy statement tests/threepcf_statement.py.  Needs an MI355X: run with `-m gpu`.

The bound is the project's rule (test_bispectrum_gpu.py::_check): per l, max|got - want| / max|want_l| <= 4 e_ref, where want is
the statement's `harmonic` form in float64 (pinned to the brute-force form by test_threepcf_host.py) and e_ref the same form in
float32 against it, as the maximum over l >= 1 - l = 0 with unit weights is exact in float32.  e_ref must lie in (1e-8, 1e-4),
else the statement is broken.  Every ratio is printed; the measured ones are recorded in profiles/threepcf/README.md.
npairs is compared bit for bit with the weighted pair counter, the two triangles of zeta with each other, and a second call
through the C entry with sentinel-filled outputs shows that every element is written.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import threepcf_statement as st
from test_threepcf_host import BOX, EDGES, LMAX, check_small, check_three_points, check_twin, dr_weights, judged, uniform

pytestmark = pytest.mark.gpu


def _eref(label, z32, z64):
    e = st.e_ref(z32, z64)
    assert 1e-8 < e < 1e-4, f'{label}: e_ref {e:.3g} outside (1e-8, 1e-4): the statement is broken'
    return e


def _check(label, got, want, e_ref):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float64, (label, got.shape, want.shape)
    for l in range(len(want)):
        err = np.abs(got[l] - want[l]).max() / np.abs(want[l]).max()
        print(f'{label} l = {l}: err {err:.3g}, e_ref {e_ref:.3g}, err / e_ref {err / e_ref:.3g} (bound 4)')
        assert err <= 4.0 * e_ref, f'{label} l = {l}: {err:.3g} > 4 x {e_ref:.3g}'


def _sentinel_call(cols, box, edges, lmax, w, second, w2):
    """abacus_threepcf on host columns with every output element pre-filled with a sentinel"""
    from abacusutils_amd import _lib
    f4 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)   # noqa: E731
    e = f4(edges)
    nb = len(e) - 1
    zeta, wself = np.full((lmax + 1, nb, nb), np.nan), np.full(nb, np.nan)
    npairs = np.full(nb, np.iinfo(np.uint64).max, dtype=np.uint64)
    a = [f4(c) for c in cols] + [f4(w)]
    b = [f4(c) for c in second] + [f4(w2)] if second is not None else [None] * 4
    p = _lib.ptr
    _lib.check(_lib.lib().abacus_threepcf(*map(p, a), C.c_int64(len(a[0])), *map(p, b), C.c_int64(0 if second is None else len(b[0])),
                                          C.c_float(box), p(e), nb, lmax, p(zeta), p(wself), p(npairs)))
    return {'zeta': zeta, 'wself': wself, 'npairs': npairs}


def _device_case(label, cols, box, edges, lmax, w=None, second=None, w2=None, want=None, want32=None):
    """the device against the statement: host columns through analysis.threepcf, then the C entry with sentinels; returns
    (float64 statement, e_ref) for the resident forms of the same case"""
    from abacusutils_amd.analysis.threepcf import triplet_multipoles
    from abacusutils_amd.analysis.tpcf_corrfunc import _paircount_weighted
    kw = dict(w=w) if second is None else dict(w=w, x2=second[0], y2=second[1], z2=second[2], w2=w2)
    want = want if want is not None else st.harmonic(*cols, box, edges, lmax, **kw)
    want32 = want32 if want32 is not None else st.harmonic(*cols, box, edges, lmax, dtype=np.float32, **kw)
    e_ref = _eref(label, want32['zeta'], want['zeta'])
    p, wt = st.catalogue(*cols, **kw)
    pairs = _paircount_weighted(0, p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy(), box, np.asarray(edges, np.float32), W1=wt)[0]
    sec = {} if second is None else dict(X2=second[0], Y2=second[1], Z2=second[2], w2=w2)
    for name, got in (('python', triplet_multipoles(*cols, box, edges, lmax, w=w, **sec)),
                      ('sentinel', _sentinel_call(cols, box, edges, lmax, w, second, w2))):
        assert np.all(np.isfinite(got['zeta'])) and np.all(np.isfinite(got['wself'])), name
        np.testing.assert_array_equal(got['npairs'], pairs, err_msg=name)
        np.testing.assert_array_equal(got['npairs'], want['npairs'], err_msg=name)
        for l in range(lmax + 1):
            np.testing.assert_array_equal(got['zeta'][l], got['zeta'][l].T, err_msg=f'{name}: the triangles differ')
        _check(f'{label} {name}', got['zeta'], want['zeta'], e_ref)
        _check(f'{label} {name} wself', got['wself'][None], want['wself'][None], e_ref)
    return want, e_ref


@pytest.mark.parametrize('weighted', [False, True], ids=['unit', 'd-r'])
def test_case_a_three_cells_per_dimension(weighted):
    """400 points, box 100, edges to 25, lmax 10: three cells per dimension, every neighbour cell wraps"""
    from abacusutils_amd.analysis.threepcf import last_stats
    w = dr_weights() if weighted else None
    _device_case('a', uniform(400), BOX, EDGES, LMAX, w=w, want=judged(weighted), want32=judged(weighted, dtype='float32'))
    s = last_stats()
    assert s['ncell'] == 3 and s['candidates'] >= s['counted'] == int(judged(weighted)['npairs'].sum())


def test_case_b_one_cell_grid():
    from abacusutils_amd.analysis.threepcf import last_stats
    _device_case('b', uniform(400), BOX, np.linspace(5.0, 45.0, 4), 4)
    assert last_stats()['ncell'] == 1 and last_stats()['candidates'] == 400 * 400


@functools.lru_cache(maxsize=None)
def _crowded():
    rng = np.random.default_rng(7)
    p = np.concatenate([rng.random((400, 3)) * BOX, rng.normal(50.0, 2.0, (600, 3))])
    return tuple(np.ascontiguousarray(p[:, d], dtype=np.float32) for d in range(3))


def test_case_c_a_cell_with_more_points_than_any_tile():
    """400 uniform points and 600 from N(50, 2^2) per axis: one cell holds more points than the queue and several rounds of
    candidates, a primary of the blob more counted pairs than a workgroup has lanes"""
    edges = np.linspace(0.5, 20.0, 9)
    want, _ = _device_case('c', _crowded(), BOX, edges, 6)
    assert want['npairs'].sum() > 600 * 500


def test_case_d_data_minus_randoms_as_two_sets():
    """200 data points without weights, 400 randoms appended as set 2 with weight -1/2: resident too, with the second set on the
    host (uploaded in the data's dtype) and resident"""
    from abacusutils_amd import _lib
    from abacusutils_amd.analysis.threepcf import triplet_multipoles
    data, rand = uniform(200, seed=3), uniform(400, seed=4)
    w2 = np.full(400, -0.5, dtype=np.float32)
    want, e_ref = _device_case('d', data, BOX, EDGES, 6, None, rand, w2)
    assert np.abs(want['zeta'][0]).max() < 0.2 * np.abs(st.harmonic(*data, BOX, EDGES, 0)['zeta'][0]).max()   # D - R cancels
    for dt in (np.float32, np.float64):
        dd = [_lib.DeviceArray(np.ascontiguousarray(c, dtype=dt)) for c in data]
        dr = [_lib.DeviceArray(np.ascontiguousarray(c, dtype=dt)) for c in rand]
        dw = _lib.DeviceArray(w2)
        try:
            for label, sec in (('host set 2', dict(X2=rand[0], Y2=rand[1], Z2=rand[2], w2=w2)),
                               ('resident set 2', dict(X2=dr[0], Y2=dr[1], Z2=dr[2], w2=dw))):
                got = triplet_multipoles(*dd, BOX, EDGES, 6, **sec)
                np.testing.assert_array_equal(got['npairs'], want['npairs'])
                _check(f'd {np.dtype(dt).name} {label}', got['zeta'], want['zeta'], e_ref)
        finally:
            for a in dd + dr + [dw]:
                a.free()


def test_case_e_the_largest_lds_configuration():
    """32 bins and lmax = 10 on 300 points"""
    _device_case('e', uniform(300, seed=5), BOX, np.linspace(1.0, 33.0, 33), 10)


@pytest.mark.parametrize('weighted', [False, True], ids=['unit', 'd-r'])
def test_case_f_resident_columns(weighted):
    """float32 and float64 resident columns (and resident weights) against the statement, the host path's bound"""
    from abacusutils_amd import _lib
    from abacusutils_amd.analysis.threepcf import triplet_multipoles
    want = judged(weighted)
    e_ref = _eref('f', judged(weighted, dtype='float32')['zeta'], want['zeta'])
    for dt in (np.float32, np.float64):
        dd = [_lib.DeviceArray(np.ascontiguousarray(c, dtype=dt)) for c in uniform(400)]
        dw = _lib.DeviceArray(np.array(dr_weights())) if weighted else None
        try:
            for w in ([dw, np.array(dr_weights())] if weighted else [None]):     # resident weights; host weights beside resident columns
                got = triplet_multipoles(*dd, BOX, EDGES, LMAX, w=w)
                np.testing.assert_array_equal(got['npairs'], want['npairs'])
                for l in range(LMAX + 1):
                    np.testing.assert_array_equal(got['zeta'][l], got['zeta'][l].T)
                _check(f'f {np.dtype(dt).name}', got['zeta'], want['zeta'], e_ref)
                _check(f'f {np.dtype(dt).name} wself', got['wself'][None], want['wself'][None], e_ref)
        finally:
            for a in dd + ([dw] if dw is not None else []):
                a.free()
    with pytest.raises(TypeError):
        triplet_multipoles(*uniform(400), BOX, EDGES, LMAX, w=_lib.DeviceArray(np.array(dr_weights())))


def test_known_answers_on_the_device():
    """the known answers of the host file: three points give P_l(cos theta) for every l, to float32 (the direction's rounding times
    the slope of P_l, at most l (l + 1) / 2 = 36 at l = 8: 36 x 3 x 2^-24 < 1e-5); a twin is a pair without a direction; lmax = 0
    with one bin; the empty catalogue"""
    from abacusutils_amd.analysis.threepcf import triplet_multipoles

    def fn(x, y, z, box, edges, lmax):
        return triplet_multipoles(x, y, z, box, edges, lmax)
    check_three_points(fn, 1e-5)
    check_twin(fn)
    check_small(fn)
    out = fn(np.zeros(0), np.zeros(0), np.zeros(0), BOX, EDGES, 2)
    assert out['zeta'].shape == (3, 5, 5) and not out['zeta'].any() and not out['npairs'].any() and not out['wself'].any()
    x = np.zeros(0)
    out = triplet_multipoles(x, x, x, BOX, EDGES, 2, X2=x, Y2=x, Z2=x)
    assert not out['zeta'].any()


def test_calc_3pcf_forms():
    """the natural form is zeta_from_counts of the raw sums; the D - R form appends `random_centres` at weight -W / N_R"""
    from abacusutils_amd.analysis.spheres import random_centres
    from abacusutils_amd.analysis.threepcf import calc_3pcf, zeta_from_counts
    cols = uniform(400)
    nat = calc_3pcf(*cols, BOX, EDGES, 4)
    want = judged(False)
    e_ref = _eref('calc_3pcf', judged(False, dtype='float32')['zeta'], want['zeta'])
    _check('calc_3pcf natural', nat['zeta'], zeta_from_counts(want['zeta'][:5], 400.0, BOX, EDGES), e_ref)
    assert nat['nrand'] == 0 and nat['wdata'] == 400.0 and np.array_equal(nat['ell'], np.arange(5))
    w = np.linspace(0.5, 1.5, 400).astype(np.float32)
    W = float(w.sum(dtype=np.float64))
    R = random_centres(800, BOX, 17)
    w2 = np.full(800, -W / 800, dtype=np.float32)
    s64, s32 = (st.harmonic(*cols, BOX, EDGES, 4, w, *R, w2, dtype=t) for t in (np.float64, np.float32))
    e_ref = _eref('calc_3pcf D - R', s32['zeta'], s64['zeta'])
    for label, got in (('int', calc_3pcf(*cols, BOX, EDGES, 4, w=w, randoms=800, seed=17)),
                       ('columns', calc_3pcf(*cols, BOX, EDGES, 4, w=w, randoms=R))):
        assert got['nrand'] == 800 and got['wdata'] == W
        np.testing.assert_array_equal(got['npairs'], s64['npairs'])
        _check(f'calc_3pcf D - R {label} raw', got['zeta_raw'], s64['zeta'], e_ref)
        _check(f'calc_3pcf D - R {label}', got['zeta'], zeta_from_counts(s64['zeta'], W, BOX, EDGES), e_ref)


def test_abacus_hod_compute_3pcf():
    """AbacusHOD.compute_3pcf: the catalogue still in HBM gives what its host columns give.  Both calls read the same float32
    catalogue in the same order, so they differ only by the order of the float32 atomics: npairs, wself and l = 0 - integers
    below 2^24 per primary with unit weights, exact in float32 - agree bit for bit; for l >= 1 each call is within 4 e_ref of the
    exact sums and e_ref < 1e-4 is what every case above asserts of the statement, so the two agree within 8e-4 of max |zeta_l|"""
    from test_abacus_hod_gpu import CLUSTERING, HOD_PARAMS

    from abacusutils_amd import synth
    from abacusutils_amd.analysis.threepcf import calc_3pcf
    from abacusutils_amd.hod.abacus_hod import AbacusHOD
    hd, pd, params = synth.synth_hod_inputs(100000, 100000, seed=19, lbox=1000.0)
    hod = dict(HOD_PARAMS, LRG_params=dict(synth.LRG_PARAMS, logM_cut=12.3, logM1=13.3), ELG_params=dict(synth.ELG_PARAMS))
    ball = AbacusHOD.from_arrays(hd, pd, params, hod, CLUSTERING)
    mock = ball.run_hod()
    assert all(mock.device_xyz(tr) is not None for tr in mock)
    plain = {tr: dict(mock[tr]) for tr in mock}
    rbins = np.linspace(2.0, 30.0, 5)
    got, want = ball.compute_3pcf(mock, rbins, 4), ball.compute_3pcf(plain, rbins, 4)
    assert set(got) == set(want) == set(mock)
    for tr in mock:
        xyz = [np.asarray(plain[tr][c]) for c in 'xyz']
        direct = calc_3pcf(*xyz, ball.lbox, rbins, 4)
        for other in (want[tr], direct):
            np.testing.assert_array_equal(got[tr]['npairs'], other['npairs'])
            np.testing.assert_array_equal(got[tr]['wself'], other['wself'])
            np.testing.assert_array_equal(got[tr]['zeta_raw'][0], other['zeta_raw'][0])
            for l in range(1, 5):
                scale = np.abs(other['zeta_raw'][l]).max()
                err = np.abs(got[tr]['zeta_raw'][l] - other['zeta_raw'][l]).max() / scale
                print(f'compute_3pcf {tr} l = {l}: {err:.3g} of max |zeta_l|')
                assert err <= 8e-4
        assert got[tr]['zeta'].shape == (5, 4, 4) and got[tr]['npairs'].sum() > 0
    # D - R on the resident catalogue: the randoms are uploaded beside it
    dr = ball.compute_3pcf(mock, rbins, 2, randoms=20000, seed=3)
    dr_host = ball.compute_3pcf(plain, rbins, 2, randoms=20000, seed=3)
    for tr in mock:
        assert dr[tr]['nrand'] == 20000
        np.testing.assert_array_equal(dr[tr]['npairs'], dr_host[tr]['npairs'])
