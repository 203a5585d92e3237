"""The NumPy statement of the Minkowski functionals (tests/minkowski_statement.py) pinned on the host: known answers on the lattice,
threshold ties, the normalisation of the package's `minkowski_from_counts`, Tomita's curves on a Gaussian field, and the argument
checks of the package.  No GPU."""
import minkowski_statement as st
import numpy as np
import pytest

from abacusutils_amd.analysis import minkowski as mk

L = 1000.0


def _mesh(n, cells=(), value=1.0):
    m = np.zeros((n, n, n), dtype=np.float32)
    for c in cells:
        m[c] = value
    return m


@pytest.mark.parametrize('n', (2, 3, 5, 8))
def test_known_answers_on_the_lattice(n):
    N, a = n**3, L / n
    chi = lambda c: c[0] - c[1] + c[2] - c[3]      # noqa: E731
    for corner in ((0, 0, 0), (n - 1, n - 1, n - 1)):                         # one voxel: 8 vertices, 12 edges, 6 faces
        c = st.counts(_mesh(n, [corner]), [0.5])[:, 0]
        assert tuple(c) == (8, 12, 6, 1) and chi(c) == 1
        V = mk.minkowski_from_counts(c[:, None], n, L)[:, 0]
        np.testing.assert_allclose(V, [1 / N, 2 * 3 / (9 * a * N), 2 * 3 / (9 * a**2 * N), 1 / (a**3 * N)], rtol=1e-15)
    plane = _mesh(n)
    plane[n - 1] = 1.0                                                         # a full plane through the box: a 2-torus times an interval
    c = st.counts(plane, [0.5])[:, 0]
    assert tuple(c) == (2 * n * n, 5 * n * n, 4 * n * n, n * n) and chi(c) == 0
    line = _mesh(n)
    line[0, n - 1, :] = 1.0                                                    # a full line through the box
    c = st.counts(line, [0.5])[:, 0]
    assert tuple(c) == (4 * n, 8 * n, 5 * n, n) and chi(c) == 0
    full = st.counts(np.ones((n, n, n), dtype=np.float32), [0.5])[:, 0]
    assert tuple(full) == (N, 3 * N, 3 * N, N)
    V = mk.minkowski_from_counts(full[:, None], n, L)[:, 0]
    assert V[0] == 1.0 and V[1] == 0.0 and V[2] == 0.0 and V[3] == 0.0
    empty = st.counts(np.ones((n, n, n), dtype=np.float32), [1.5])
    assert not empty.any() and not mk.minkowski_from_counts(empty, n, L).any()


def test_threshold_ties_are_inside():
    n = 4
    v = np.float32(0.3)
    up = np.nextafter(v, np.float32(1.0))
    m = _mesh(n, [(1, 2, 3)], v)
    c = st.counts(m, [v, up])
    assert tuple(c[:, 0]) == (8, 12, 6, 1), 'a threshold equal to the cell value counts the cell as inside'
    assert not c[:, 1].any(), 'the next float32 above the cell value leaves it outside'
    below = st.counts(m, [np.nextafter(v, np.float32(0.0))])
    assert tuple(below[:, 0]) == (8, 12, 6, 1)
    assert tuple(st.counts(m, [0.0])[:, 0]) == (64, 192, 192, 64)              # the zeros tie with a threshold of 0


def test_the_package_normalises_as_the_statement():
    rng = np.random.default_rng(2)
    m = rng.standard_normal((6, 6, 6)).astype(np.float32)
    c = st.counts(m, np.linspace(-2, 2, 9))
    np.testing.assert_allclose(mk.minkowski_from_counts(c, 6, L), st.functionals(c, 6, L), rtol=1e-15)
    assert (np.diff(c, axis=1) <= 0).all()
    with pytest.raises(ValueError, match='shape'):
        mk.minkowski_from_counts(c[:3], 6, L)
    np.testing.assert_allclose(mk.gaussian_prediction(np.linspace(-3, 3, 13), 0.01), st.gaussian_curves(np.linspace(-3, 3, 13), 0.01),
                               rtol=1e-15)
    P = mk.gaussian_prediction([0.0, 1.0], 0.02)
    np.testing.assert_allclose(P[:, 0], [0.5, 2 / 3 * 0.02 / np.sqrt(2 * np.pi), 0.0, -0.02**3 / np.sqrt(2 * np.pi)], rtol=1e-15)
    assert P[3, 1] == 0.0                                                      # the Euler characteristic changes sign at nu = 1


def test_gaussian_field_follows_tomita():
    """A seeded Gaussian field (seed 1) at 64^3 smoothed over 3 cells, 13 thresholds nu in [-3, 3] in units of its sigma: the statement's
    counts through `minkowski_from_counts` against `gaussian_prediction` with lam measured on the same mesh.  Deviation as a fraction of
    each curve's peak, measured on the CPU: 0.0098, 0.0244, 0.0792, 0.1044 for V0 .. V3 (the lattice estimator at a smoothing length
    of 3 cells, one realisation).  Allowed: twice that, 0.0196, 0.0488, 0.1584, 0.2088 - one realisation, not a bound."""
    n, nu = 64, np.linspace(-3, 3, 13)
    f, lam = st.gaussian_field(n, L, 3 * L / n, 1)
    f64 = f.astype(np.float64)
    thr = (nu * f64.std() + f64.mean()).astype(np.float32)
    V = mk.minkowski_from_counts(st.counts(f, thr), n, L)
    P = mk.gaussian_prediction(nu, lam)
    dev = np.abs(V - P).max(axis=1) / np.abs(P).max(axis=1)
    print('deviation from Tomita as a fraction of the peak, V0 .. V3:', np.array2string(dev, precision=4), f'lam = {lam:.6g}')
    assert (dev <= np.array([0.0196, 0.0488, 0.1584, 0.2088])).all(), dev
    assert (dev > 1e-4).all()                                                  # and it is a measurement, not the prediction fed back


def test_argument_checks_need_no_device(monkeypatch):
    from abacusutils_amd import _lib

    def no_library():
        raise AssertionError('the library was touched')

    monkeypatch.setattr(_lib, 'lib', no_library)
    mesh = np.zeros((4, 4, 4), dtype=np.float32)
    thr = np.linspace(-1, 1, 5)
    up = np.nextafter(np.float32(1.0), np.float32(2.0))
    bad_thresholds = ([], np.linspace(0, 1, 65), [0.5, 0.25], [1.0, 1.0 + 1e-9], [0.0, np.nan], [0.0, np.inf], [[0.0, 1.0]])
    for t in bad_thresholds:
        for call in (lambda: mk.minkowski_counts(mesh, t), lambda: mk.minkowski_functionals(mesh, L, t),
                     lambda: mk.calc_minkowski(np.zeros((10, 3)), L, t, 10.0, nmesh=16)):
            with pytest.raises(ValueError, match='thresholds'):
                call()
    assert mk._thresholds([1.0, up])[1].tolist() == [1.0, float(up)]            # neighbours in float32 do pass
    assert len(mk._thresholds(np.linspace(0, 1, 64))[1]) == 64
    for call in (lambda m: mk.minkowski_counts(m, thr), lambda m: mk.mesh_moments(m), lambda m: mk.minkowski_functionals(m, L, thr)):
        with pytest.raises(ValueError, match='cubic'):
            call(np.zeros((4, 4, 5), dtype=np.float32))
        with pytest.raises(ValueError, match='cubic'):
            call(np.zeros((4, 4), dtype=np.float32))
        with pytest.raises(TypeError, match='float32'):
            call(np.zeros((4, 4, 4), dtype=np.float64))
        with pytest.raises(TypeError, match='mesh'):
            call([[1.0]])
        with pytest.raises(ValueError, match='cells per side'):
            call(np.zeros((1, 1, 1), dtype=np.float32))
        for bad in (np.nan, np.inf, -np.inf):
            m = mesh.copy()
            m[1, 2, 3] = bad
            with pytest.raises(ValueError, match='not finite'):
                call(m)
    odd = np.zeros((5, 5, 5), dtype=np.float32)
    with pytest.raises(ValueError, match='even'):
        mk.minkowski_functionals(odd, L, thr, R=10.0)
    with pytest.raises(ValueError, match='R must'):
        mk.minkowski_functionals(mesh, L, thr, R=-1.0)
    with pytest.raises(ValueError, match='Lbox'):
        mk.minkowski_functionals(mesh, 0.0, thr)
    call = lambda **kw: mk.calc_minkowski(**{**dict(pos=np.zeros((10, 3)), Lbox=L, thresholds=thr, R=10.0, nmesh=16), **kw})   # noqa: E731
    for n in (15, 0, -2, 32768):
        with pytest.raises(ValueError, match='nmesh'):
            call(nmesh=n)
    for R in (-1.0, np.nan, np.inf, None):
        with pytest.raises(ValueError, match='R must'):
            call(R=R)
    with pytest.raises(ValueError, match='Lbox'):
        call(Lbox=-1.0)
    with pytest.raises(ValueError, match='pasting'):
        call(paste='NGP')
    with pytest.raises(ValueError, match='shape'):
        call(pos=np.zeros((10, 2)))
    with pytest.raises(ValueError, match='weights'):
        call(w=np.ones(9))


def test_compute_entries_raise_without_a_device():
    from abacusutils_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip('a HIP device is present')
    mesh = np.zeros((4, 4, 4), dtype=np.float32)
    thr = [0.5]
    for call in (lambda: mk.minkowski_counts(mesh, thr), lambda: mk.mesh_moments(mesh), lambda: mk.minkowski_functionals(mesh, L, thr),
                 lambda: mk.minkowski_functionals(mesh, L, thr, R=100.0),
                 lambda: mk.calc_minkowski(np.zeros((10, 3)), L, thr, 10.0, nmesh=16)):
        with pytest.raises(_lib.AbacusHipError, match='no HIP device'):
            call()
    # and the C entries themselves, past their argument checks
    t32, out = np.array([0.5], dtype=np.float32), np.zeros((4, 1), dtype=np.int64)
    fake = _lib.C.c_void_p(4096)                                                                # never dereferenced: no device to launch on
    lib = _lib.lib()
    for rc in (lib.abacus_mf_counts_dev(fake, 4, 4, _lib.ptr(t32), 1, _lib.ptr(out)), lib.abacus_mf_moments_dev(fake, 4, 4, _lib.ptr(np.zeros(2))),
               lib.abacus_mf_smooth_spectrum_dev(fake, 4, _lib.C.c_double(L), _lib.C.c_double(1.0)), lib.abacus_mf_check_memory(4, _lib.C.c_int64(0))):
        assert rc != 0 and 'no HIP device' in lib.abacus_last_error().decode()


def test_kernels_do_not_spill(tmp_path):
    """mf_count carries the maxima of a plane in registers across its loop over planes and mf_moments two float64 sums: neither may
    spill or use scratch (it cross-compiles, no GPU needed)"""
    import os
    import re
    import shutil
    import subprocess
    from pathlib import Path
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    src = Path(__file__).resolve().parent.parent / 'abacusutils_amd' / 'csrc' / 'minkowski.hip'
    r = subprocess.run([hipcc, '-O3', '-std=c++17', '--offload-arch=gfx950', '-ffp-contract=off', '-munsafe-fp-atomics', '-c', str(src), '-o',
                        str(tmp_path / 'minkowski.o'), '-save-temps=obj'], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    asm = [f for f in os.listdir(tmp_path) if f.startswith('minkowski') and f.endswith('gfx950.s')]
    assert asm, os.listdir(tmp_path)
    text = open(tmp_path / asm[0]).read()
    found = set()
    for m in re.finditer(r'\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)(.*?)\.sgpr_spill_count:\s+(\d+)(.*?)\.vgpr_spill_count:\s+(\d+)',
                         text, re.S):
        name, scratch, sspill, vspill = m.group(1), int(m.group(2)), int(m.group(4)), int(m.group(6))
        for k in ('mf_count', 'mf_moments'):
            if k in name:
                found.add(name)
                assert (scratch, sspill, vspill) == (0, 0, 0), (name, scratch, sspill, vspill)
    assert len(found) >= 6, found                      # mf_count and mf_moments with both kinds of loads, and the two final kernels
