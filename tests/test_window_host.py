"""No-GPU checks of the ZCV mode-coupling window (abacusutils_amd.hod.zcv.zenbu_window): the host half, `assemble_window`, fed the
golden moments, against the float64 statement (tests/window_statement.py) and the reference's own arrays; the structural zeros;
argument checks before the device; the file name `run_zcv` expects; the module imports without classy, ZeNBu or yaml.

Golden file: tests/golden/zcv_window_cases.npz (scripts/make_window_golden.py).  Its `e_ref_*` is the reference's own float32
accumulation noise against the float64 statement; 4 x e_ref is the project's usual factor over that noise."""
import importlib.util
import inspect
import sys
from pathlib import Path

import numpy as np
import pytest
from conftest import load_golden
from window_statement import block_error

REPO = Path(__file__).resolve().parent.parent
NAMES = [f'n{n}_b{b}_{kin}_{w}' for n, b in ((8, 4), (12, 6), (16, 8), (16, 5)) for kin in ('centres', 'fine') for w in ('k2w', 'flat')]
NAMES.append('n16_integer_edges')
LOGK = ['n8_b4_logk', 'n16_b6_logk']


@pytest.fixture(scope='module')
def golden():
    return load_golden('zcv_window_cases')


def case(g, name):
    pre = f'case/{name}/'
    return {k[len(pre):]: v for k, v in g.items() if k.startswith(pre)}


@pytest.fixture
def no_library(monkeypatch):
    """any attempt to load (or use) the device library fails the test"""
    from abacusutils_amd import _lib

    def boom(*a, **k):
        raise AssertionError('the device library was touched before the arguments were checked')
    monkeypatch.setattr(_lib, 'lib', boom)


def test_golden_file_holds_every_case(golden):
    assert list(golden['names']) == NAMES and list(golden['logk_names']) == LOGK
    for name in NAMES:
        c = case(golden, name)
        assert 0 < c['e_ref_window'] <= 1e-3 and 0 < c['e_ref_keff'] <= 1e-3, name
    for name in LOGK:
        assert 'window' not in case(golden, name) and 'window64' in case(golden, name)


@pytest.mark.parametrize('name', NAMES + LOGK)
def test_assemble_window_equals_the_statement(golden, no_library, name):
    from abacusutils_amd.hod.zcv.zenbu_window import assemble_window
    c = case(golden, name)
    nkout, nkin = len(c['kout']) - 1, len(c['kin'])
    window, keff = assemble_window(c['S'], c['nmodes'], c['ksum'], c['kout'], c['kin'], k2weight=bool(c['k2weight']))
    assert window.dtype == np.float64 and keff.dtype == np.float64
    assert window.shape == c['window64'].shape == (3 * nkout, 3 * nkin) and keff.shape == c['keff64'].shape == (nkout,)
    assert block_error(window, c['window64'], nkout, nkin) <= 1e-12
    assert np.abs(keff - c['keff64']).max() <= 1e-12 * np.abs(c['keff64']).max()


@pytest.mark.parametrize('name', NAMES)
def test_assemble_window_agrees_with_the_reference(golden, no_library, name):
    from abacusutils_amd.hod.zcv.zenbu_window import assemble_window
    c = case(golden, name)
    nkout, nkin = len(c['kout']) - 1, len(c['kin'])
    window, keff = assemble_window(c['S'], c['nmodes'], c['ksum'], c['kout'], c['kin'], k2weight=bool(c['k2weight']))
    assert c['window'].dtype == np.float64 and c['window'].shape == window.shape and c['keff'].shape == keff.shape
    e_w, e_k = block_error(window, c['window'], nkout, nkin), np.abs(keff - c['keff']).max() / np.abs(c['keff']).max()
    print(f'{name}: window {e_w:.3g} (e_ref {c["e_ref_window"]:.3g}), keff {e_k:.3g} (e_ref {c["e_ref_keff"]:.3g})')
    assert e_w <= 4 * c['e_ref_window']
    assert e_k <= 4 * c['e_ref_keff']


@pytest.mark.parametrize('name', NAMES + LOGK)
def test_structural_zeros(golden, no_library, name):
    """an entry whose input column lies in another output bin than its row is exactly 0 (inside a block the zero pattern of the
    reference is NOT comparable: exact cancellation differs between float32 and float64 sums); columns of kin beyond the last edge
    are 0"""
    from abacusutils_amd.hod.zcv.zenbu_window import assemble_window
    c = case(golden, name)
    nkout, nkin = len(c['kout']) - 1, len(c['kin'])
    window, _ = assemble_window(c['S'], c['nmodes'], c['ksum'], c['kout'], c['kin'], k2weight=bool(c['k2weight']))
    idx_i = np.digitize(c['kin'], c['kout']) - 1
    off = idx_i[None, :] != np.arange(nkout)[:, None]
    for ell in range(3):
        for ellp in range(3):
            block = window[ell * nkout:(ell + 1) * nkout, ellp * nkin:(ellp + 1) * nkin]
            assert (block[off] == 0).all()
            assert (block[:, c['kin'] >= c['kout'][-1]] == 0).all()
    if 'fine' in name:
        assert (c['kin'] >= c['kout'][-1]).any()
    # the l = l' = 0 block of a filled bin with columns is positive: the pattern above is not trivially met
    assert (window[:nkout, :nkin][~off] > 0).any()


def test_rows_of_empty_bins_and_unmatched_columns_are_zero(no_library):
    from abacusutils_amd.hod.zcv.zenbu_window import assemble_window
    kout = np.array([0.0, 1.0, 2.0, 3.0, 4.0])
    kin = np.array([0.5, 0.6, 1.5, 2.5, 3.5, 4.5, 9.0])       # the last two lie beyond the last edge
    rng = np.random.default_rng(5)
    S = rng.uniform(1.0, 2.0, (4, 3, 3))
    nmodes = np.array([3.0, 0.0, 8.0, 4.0])                     # bin 1 holds no mode
    S[1], ksum = 0.0, np.array([1.0, 0.0, 20.0, 17.0])
    for k2w in (True, False):
        window, keff = assemble_window(S, nmodes, ksum, kout, kin, k2weight=k2w)
        assert np.isfinite(window).all() and np.isfinite(keff).all()
        for ell in range(3):
            assert (window[ell * 4 + 1] == 0).all()
            for ellp in range(3):
                assert (window[ell * 4:(ell + 1) * 4, ellp * 7 + 5:ellp * 7 + 7] == 0).all()
        np.testing.assert_array_equal(keff, [1.0 / 3.0, 0.0, 2.5, 4.25])
        # two columns share bin 0
        assert window[0, 0] > 0 and window[0, 1] > 0 and window[0, 2] == 0
    # without k2weight each column of a bin gets S / nmodes / (columns of the bin)
    window, _ = assemble_window(S, nmodes, ksum, kout, kin, k2weight=False)
    assert window[0, 0] == S[0, 0, 0] * (1.0 / 3.0) * 0.5 and window[2, 3] == S[2, 0, 0] * (1.0 / 8.0)


def test_bad_arguments_raise_before_the_device(no_library):
    from abacusutils_amd.hod.zcv.zenbu_window import assemble_window, periodic_window_function, save_window, window_moments
    kout = np.linspace(0.0, 0.4, 5)
    kin = 0.5 * (kout[1:] + kout[:-1])
    bad = [dict(nmesh=15), dict(nmesh=0), dict(nmesh=-8), dict(kout=kout[::-1]), dict(kout=np.array([0.0, 0.1, 0.1, 0.2])),
           dict(kout=np.array([0.1])), dict(kin=np.array([0.1])), dict(kin=np.array([0.1, np.nan, 0.3])),
           dict(kin=np.array([0.1, np.inf])), dict(kout=np.array([0.0, np.nan, 0.2])), dict(kout=np.array([0.0, 0.1, np.inf])),
           dict(lbox=np.nan), dict(lbox=np.inf), dict(lbox=0.0), dict(lbox=-100.0)]
    for change in bad:
        args = dict(nmesh=16, lbox=100.0, kout=kout, kin=kin, k2weight=True)
        args.update(change)
        with pytest.raises(ValueError):
            periodic_window_function(**args)
    with pytest.raises(ValueError):
        window_moments(15, 100.0, kout)
    with pytest.raises(ValueError):
        window_moments(16, 100.0, kout[::-1])
    with pytest.raises(ValueError):
        assemble_window(np.zeros((3, 3, 3)), np.zeros(4), np.zeros(4), kout, kin)
    with pytest.raises(ValueError):
        save_window('unused', 'sim', 15, 100.0, 0.4, 4)
    # a single kin is fine without the k^2 dk weight: only then no spacing is needed (the check passes, the device is next)
    with pytest.raises(AssertionError, match='device library'):
        periodic_window_function(16, 100.0, kout, np.array([0.1]), k2weight=False)


def test_public_names_and_signatures():
    from abacusutils_amd.hod import zcv
    from abacusutils_amd.hod.zcv import zenbu_window as W
    E = inspect.Parameter.empty

    def sig(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    assert sig(W.periodic_window_function) == [('nmesh', E), ('lbox', E), ('kout', E), ('kin', E), ('k2weight', True)]
    assert sig(W.window_moments) == [('nmesh', E), ('lbox', E), ('kout', E)]
    assert sig(W.assemble_window) == [('S', E), ('nmodes', E), ('ksum', E), ('kout', E), ('kin', E), ('k2weight', True)]
    assert sig(W.window_path) == [('zcv_dir', E), ('sim_name', E), ('nmesh', E), ('k_bins', E), ('logk', E)]
    assert sig(W.save_window) == [('zcv_dir', E), ('sim_name', E), ('nmesh', E), ('Lbox', E), ('k_hMpc_max', E), ('n_k_bins', E),
                                  ('logk', False), ('overwrite', False)]
    assert zcv.zenbu_window is W and zcv.periodic_window_function is W.periodic_window_function and zcv.save_window is W.save_window
    assert {'zenbu_window', 'periodic_window_function', 'save_window'} <= set(zcv.__all__)
    for word in ('range(len(kout))', 'IndexError', 'last row'):
        assert word in W.__doc__ or word.lower() in W.__doc__.lower()


def test_window_path_has_both_forms():
    from abacusutils_amd.analysis.power_spectrum import get_k_mu_edges
    from abacusutils_amd.hod.zcv.zenbu_window import window_path
    nmesh, L = 16, 200.0
    kny = np.pi * nmesh / L
    full, _ = get_k_mu_edges(L, kny, 8, 1, False)
    assert window_path('/data/zcv', 'AbacusSummit_base_c000_ph000', nmesh, full, False) == \
        Path('/data/zcv') / 'AbacusSummit_base_c000_ph000' / 'window_nmesh16.npz'
    some, _ = get_k_mu_edges(L, 0.2, 5, 1, False)
    assert window_path('/data/zcv', 'sim', nmesh, some, False) == Path('/data/zcv/sim/window_nmesh16_dk0.040.npz')
    logk, _ = get_k_mu_edges(L, 0.2, 5, 1, True)
    dk = np.log(logk[1] / logk[0])
    assert window_path(Path('/data/zcv'), 'sim', nmesh, logk, True) == Path(f'/data/zcv/sim/window_nmesh16_dk{dk:.3f}.npz')
    assert f'{dk:.3f}' != '0.040'
    # nmesh // 2 bins take the short name whatever their spacing
    logk8, _ = get_k_mu_edges(L, kny, 8, 1, True)
    assert window_path('/data/zcv', 'sim', nmesh, logk8, True).name == 'window_nmesh16.npz'


def test_module_imports_without_classy_zenbu_yaml(monkeypatch):
    """the reference's module raises ImportError without classy and ZeNBu; this one needs neither (nor yaml): a fresh copy of the
    module is executed with those imports blocked"""
    for mod in ('classy', 'ZeNBu', 'ZeNBu.zenbu', 'ZeNBu.zenbu_rsd', 'yaml'):
        monkeypatch.setitem(sys.modules, mod, None)      # `import classy` raises ImportError
    with pytest.raises(ImportError):
        import classy  # noqa: F401
    import abacusutils_amd.hod.zcv as zcv
    path = Path(zcv.__file__).parent / 'zenbu_window.py'
    spec = importlib.util.spec_from_file_location('abacusutils_amd.hod.zcv._zenbu_window_fresh', path)
    fresh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fresh)
    assert callable(fresh.periodic_window_function) and callable(fresh.save_window)


def test_c_abi_declares_the_entry_point():
    text = (REPO / 'include' / 'abacus_hip.h').read_text()
    assert 'int abacus_window_moments(int nmesh, const float *kvals_host, const double *kout_host, int nkout, double *S_host' in text
    mk = (REPO / 'abacusutils_amd' / 'csrc' / 'Makefile').read_text()
    assert 'window.hip' in mk
    # the float32 per-mode values are bit-equal to NumPy's: no FMA contraction for this file
    assert all('window' not in ln for ln in mk.splitlines() if '-ffp-contract=fast' in ln)


def test_bad_sizes_are_refused_by_the_library():
    """the C entry point checks its own arguments (it may be called without the Python layer), before it asks for a device"""
    import ctypes as C
    from abacusutils_amd import _lib
    from abacusutils_amd._lib import AbacusHipError, check, ptr
    kv = np.zeros(16, dtype=np.float32)
    out = [np.zeros(9 * 4), np.zeros(4), np.zeros(4)]

    def call(nmesh, kout):
        check(_lib.lib().abacus_window_moments(C.c_int(nmesh), ptr(kv), ptr(kout), C.c_int(len(kout) - 1), *[ptr(a) for a in out]))
    with pytest.raises(AbacusHipError, match='even'):
        call(15, np.arange(5.0))
    with pytest.raises(AbacusHipError, match='strictly increasing'):
        call(16, np.array([0.0, 1.0, 1.0, 2.0, 3.0]))
    with pytest.raises(AbacusHipError, match='strictly increasing'):
        call(16, np.array([0.0, 1.0, np.nan, 2.0, 3.0]))
