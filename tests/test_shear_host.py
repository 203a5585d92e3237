"""No-GPU checks of the tidal-shear feature (abacusutils_amd.analysis.shear, prepare_sim.calc_shearmark): the public names and
signatures are the reference's, bad arguments raise before the device library is touched, the C ABI declares the new entry points,
and prepare_sim.main computes the field instead of asking for a file."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
MINI = REPO / 'tests' / 'golden' / 'Mini_N64_L32'


def _sig(f):
    return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]


E = inspect.Parameter.empty


def test_signatures_are_the_references():
    """abacusnbody/analysis/shear.py:15,39,70,96 and hod/prepare_sim.py:1055, written out"""
    from abacusutils_amd.analysis import shear as S
    from abacusutils_amd.hod import prepare_sim as PS
    assert _sig(S.smooth_density) == [('D', E), ('R', E), ('N_dim', E), ('Lbox', E)]
    assert _sig(S.get_tidal) == [('dfour', E), ('karr', E), ('N_dim', E), ('R', E), ('dtype', np.float32)]
    assert _sig(S.get_shear_nb) == [('tidr', E), ('N_dim', E)]
    assert _sig(S.get_shear) == [('dsmo', E), ('N_dim', E), ('Lbox', E), ('R', None), ('dtype', np.float32)]
    # the reference's seven parameters, then the seeding extension
    assert _sig(PS.calc_shearmark) == [('simdir', E), ('simname', E), ('z_mock', E), ('N_dim', E), ('R', E), ('fn', E), ('partdown', 100),
                                       ('rng', None)]


@pytest.fixture
def no_library(monkeypatch):
    """any attempt to load (or use) the device library fails the test"""
    from abacusutils_amd import _lib

    def boom(*a, **k):
        raise AssertionError('the device library was touched before the arguments were checked')
    monkeypatch.setattr(_lib, 'lib', boom)


def test_bad_arguments_raise_before_the_library_is_loaded(no_library, tmp_path):
    from abacusutils_amd.analysis import shear as S
    from abacusutils_amd.hod import prepare_sim as PS
    with pytest.raises(ValueError, match='odd'):                       # the reference itself fails on odd meshes
        S.get_shear(np.zeros((21, 21, 21), dtype=np.float32), 21, 50.0)
    with pytest.raises(ValueError, match='odd'):
        S.shearmark_from_positions(np.zeros((5, 3), dtype=np.float32), 21, 50.0, 2.0)
    with pytest.raises(ValueError, match='odd'):
        PS.calc_shearmark(str(MINI), 'Mini_N64_L32', 0.0, 21, 2.0, str(tmp_path / 'shear'))
    with pytest.raises(ValueError, match='cubic'):                     # a non-cubic mesh
        S.get_shear(np.zeros((16, 16, 12), dtype=np.float32), 16, 50.0)
    with pytest.raises(ValueError, match='cubic'):
        S.smooth_density(np.zeros((16, 12, 16), dtype=np.float32), 2.0, 16, 50.0)
    with pytest.raises(ValueError, match='N_dim'):                     # a mesh that is not N_dim cells wide
        S.get_shear(np.zeros((16, 16, 16), dtype=np.float32), 18, 50.0)
    with pytest.raises(TypeError):                                     # wrong dtypes
        S.get_shear(np.zeros((16, 16, 16), dtype=np.complex64), 16, 50.0)
    with pytest.raises(TypeError):
        S.get_shear(np.zeros((16, 16, 16), dtype=np.float32), 16, 50.0, dtype=np.float64)
    with pytest.raises(TypeError):
        S.smooth_density(np.zeros((16, 16, 16), dtype=np.float64), 2.0, 16, 50.0)
    with pytest.raises(TypeError):
        S.shearmark_from_positions(np.zeros((5, 3), dtype=np.float64), 16, 50.0, 2.0)
    with pytest.raises(ValueError):
        S.get_tidal(np.zeros((16, 16, 16), dtype=np.complex64), np.zeros(16, dtype=np.float32), 16, None)   # not (N, N, N/2+1)


def test_gaussian_weights_are_scipys():
    """radius int(4 sigma + 0.5), exp(-x^2 / (2 sigma^2)) normalised to 1: against scipy.ndimage where it is installed, and
    against the closed form everywhere"""
    from abacusutils_amd.analysis.shear import gaussian_weights
    for sigma, radius in ((0.5, 2), (1.0, 4), (2.3, 9), (3.5, 14)):
        r, w = gaussian_weights(sigma)
        assert r == radius and w.dtype == np.float64 and len(w) == radius + 1
        x = np.arange(-radius, radius + 1)
        full = np.exp(-x.astype(np.float64) ** 2 / (2 * sigma * sigma))
        full /= full.sum()
        assert np.allclose(w, full[radius:], rtol=1e-14, atol=0)
        assert abs(w[0] + 2 * w[1:].sum() - 1) < 1e-15
    ndi = pytest.importorskip('scipy.ndimage')
    spike = np.zeros(41)
    spike[20] = 1.0
    r, w = gaussian_weights(2.3)
    assert np.allclose(ndi.gaussian_filter1d(spike, 2.3)[20:20 + r + 1], w, rtol=1e-14, atol=0)


def test_get_shear_nb_is_the_eigenvalue_formula():
    """the thin host function against numpy.linalg on random symmetric tensors"""
    from abacusutils_amd.analysis.shear import get_shear_nb
    rng = np.random.default_rng(5)
    t = rng.standard_normal((4, 4, 4, 6)).astype(np.float32)
    got = get_shear_nb(t, 4)
    m = np.empty((4, 4, 4, 3, 3))
    for q, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        m[..., i, j] = m[..., j, i] = t[..., q]
    ev = np.linalg.eigvalsh(m)
    want = np.sqrt(0.5 * ((ev[..., 1] - ev[..., 0]) ** 2 + (ev[..., 2] - ev[..., 0]) ** 2 + (ev[..., 2] - ev[..., 1]) ** 2))
    assert got.dtype == np.float32 and got.shape == (4, 4, 4)
    assert np.abs(got - want).max() <= 1e-6 * want.max()


def test_header_declares_the_entry_points():
    text = (REPO / 'include' / 'abacus_hip.h').read_text()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in ('abacus_gauss_smooth_dev', 'abacus_shear_dev', 'abacus_shearmark_dev', 'abacus_mesh_gather_dev', 'abacus_tidal_dev'):
        assert re.search(r'\bint\s+' + name + r'\s*\(', code), name
        # ... each under a comment that names what it replaces
        assert re.search(r'/\*\s*replaces:(?:(?!\*/).)*\*/\s*int\s+' + name + r'\s*\(', text, flags=re.S), name
    assert 'shear.hip' in (REPO / 'abacusutils_amd' / 'csrc' / 'Makefile').read_text()


def test_main_with_want_shear_computes_the_field(monkeypatch, tmp_path):
    """prepare_sim.main no longer stops at a NotImplementedError: without a saved field it calls calc_shearmark with the
    configuration's shear_N / shear_R / partdown and hands the field to every slab; a saved field is loaded instead"""
    import yaml

    from abacusutils_amd.hod import prepare_sim as PS
    config = yaml.safe_load(open(MINI / 'abacus_hod.yaml'))
    config['sim_params']['sim_dir'] = str(MINI) + '/'
    config['sim_params']['subsample_dir'] = str(tmp_path / 'data_subs') + '/'
    config['HOD_params'].update(want_shear=True, shear_N=12, shear_R=1.5, partdown=3)
    field = np.arange(12 ** 3, dtype=np.float32).reshape(12, 12, 12)
    calls, slabs = [], []

    def fake_calc(simdir, simname, z_mock, N_dim, R, fn, partdown=100):
        calls.append((simdir, simname, z_mock, N_dim, R, fn, partdown))
        return field

    def fake_slab(i, **kw):
        slabs.append((i, kw['want_shear'], kw['shearmark']))
        return 0
    monkeypatch.setattr(PS, 'calc_shearmark', fake_calc)
    monkeypatch.setattr(PS, 'prepare_slab', fake_slab)
    PS.main(str(MINI / 'abacus_hod.yaml'), params=config)
    savedir = str(tmp_path / 'data_subs') + '/Mini_N64_L32/z0.000'
    assert calls == [(str(MINI) + '/', 'Mini_N64_L32', 0.0, 12, 1.5, savedir + '/shear_N12_R1.5_down3', 3)]
    assert [s[0] for s in slabs] == [0, 1, 2] and all(s[1] is True and s[2] is field for s in slabs)
    # a field on disk is loaded, not recomputed
    np.save(savedir + '/shear_N12_R1.5_down3.npy', field + 1)
    del calls[:], slabs[:]
    PS.main(str(MINI / 'abacus_hod.yaml'), params=config)
    assert calls == [] and len(slabs) == 3 and np.array_equal(slabs[0][2], field + 1)


def test_field_fixtures_are_in_place():
    """the field particles calc_shearmark reads sit next to the halo particles of the Mini_N64_L32 fixtures, and the golden holds
    every case with the float32 noise of the reference (e_ref) the GPU tests derive their bound from"""
    d = MINI / 'Mini_N64_L32' / 'halos' / 'z0.000'
    for kind in ('field_rv_A', 'halo_rv_A'):
        assert sorted(p.name for p in (d / kind).glob('*.asdf')) == [f'{kind}_00{i}.asdf' for i in range(3)]
    g = np.load(REPO / 'tests' / 'golden' / 'shear_cases.npz')
    assert {'poisson16', 'lognormal24', 'lognormal32', 'lognormal24_R3', 'mini32'} <= set(g['shear_names'].tolist())
    for name in g['shear_names']:
        assert 1e-8 < float(g[f'shear/{name}/e_ref']) < 1e-6
