"""No-GPU checks of the linear control variates (abacusutils_amd.hod.zcv.linear_fields, tracer_power.recon_power): the public names
and argument lists, bad arguments raise before the device library is touched, the golden files hold every case the GPU tests list
with a usable e_ref, and the C ABI declares the new entry points."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
from conftest import load_golden

REPO = Path(__file__).resolve().parent.parent
E = inspect.Parameter.empty

LINEAR = ['white16', 'white24', 'white16_unfiltered']
RECON = ['TSC_TT', 'TSC_FF', 'CIC_TT', 'CIC_FF', 'TSC_TT_norandoms', 'TSC_TT_mu1']
COMBINE = ['recsym', 'reciso']
LIN_PAIRS = ['delta_delta', 'deltamu2_delta', 'deltamu2_deltamu2']
TR_PAIRS = ['tr_tr', 'delta_tr', 'deltamu2_tr']


def _sig(f):
    return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]


def test_signatures_and_exports():
    from abacusutils_amd.hod import zcv
    from abacusutils_amd.hod.zcv import linear_fields as LF, tracer_power as T
    assert LF.KEYNAMES == ('delta', 'deltamu2')
    assert _sig(LF.linear_fields) == [('delta_lin', E), ('Lbox', E), ('nmesh', E)]
    assert _sig(LF.linear_power) == [('lin', E), ('k_bin_edges', E), ('mu_bin_edges', E), ('poles', E)]
    assert _sig(LF.linear_power3d) == [('lin', E)]
    assert _sig(LF.combine_field_spectra_k3D_lcv) == [('bias', E), ('f_growth', E), ('D', E), ('lin', E), ('nmesh', E), ('Lbox', E), ('R', E),
                                                      ('rec_algo', E)]
    assert _sig(T.recon_power) == [('tracer_pos', E), ('random_pos', E), ('lin', E), ('k_bin_edges', E), ('mu_bin_edges', E), ('poles', E),
                                   ('paste', 'TSC'), ('compensated', True), ('interlaced', True), ('save_3D_power', False)]
    assert all(hasattr(LF.LinearFields, m) for m in ('spectrum', 'free', '__enter__', '__exit__'))
    assert zcv.LinearFields is LF.LinearFields and zcv.recon_power is T.recon_power and zcv.linear_fields is LF
    assert zcv.combine_field_spectra_k3D_lcv is LF.combine_field_spectra_k3D_lcv
    assert zcv.linear_power is LF.linear_power and zcv.linear_power3d is LF.linear_power3d
    assert {'linear_fields', 'LinearFields', 'linear_power', 'linear_power3d', 'combine_field_spectra_k3D_lcv', 'recon_power'} <= set(zcv.__all__)
    assert 'in place' in T.recon_power.__doc__.lower() and 'not shifted' in T.recon_power.__doc__.lower()
    assert 'no reference output' in LF.combine_field_spectra_k3D_lcv.__doc__.lower()
    assert 'not built' not in T.__doc__


@pytest.fixture
def no_library(monkeypatch):
    """any attempt to load (or use) the device library fails the test"""
    from abacusutils_amd import _lib

    def boom(*a, **k):
        raise AssertionError('the device library was touched before the arguments were checked')
    monkeypatch.setattr(_lib, 'lib', boom)


def _device(shape, dtype):
    """stands for a DeviceArray of the given dtype and shape without touching the library"""
    from abacusutils_amd._lib import DeviceArray
    a = DeviceArray.__new__(DeviceArray)
    a.ptr, a.shape, a.dtype, a.nbytes, a._view = None, tuple(shape), np.dtype(dtype), 0, True
    return a


def test_bad_arguments_raise_before_the_library_is_loaded(no_library):
    from abacusutils_amd.hod.zcv import linear_fields as LF
    from abacusutils_amd.hod.zcv.tracer_power import recon_power
    z16 = np.zeros((16, 16, 16), dtype=np.float32)
    with pytest.raises(ValueError, match='even'):
        LF.linear_fields(np.zeros((15, 15, 15), dtype=np.float32), 100.0, 15)
    with pytest.raises(ValueError, match='cubic'):
        LF.linear_fields(np.zeros((16, 16, 12), dtype=np.float32), 100.0, 16)
    with pytest.raises(ValueError, match='nmesh'):
        LF.linear_fields(z16, 100.0, 18)
    with pytest.raises(TypeError, match='float32'):
        LF.linear_fields(z16.astype(np.float64), 100.0, 16)
    with pytest.raises(TypeError, match='float32'):
        LF.linear_fields(_device((16, 16, 16), np.float64), 100.0, 16)
    with pytest.raises(ValueError):
        LF.linear_fields(z16, 0.0, 16)
    lin = LF.LinearFields(100.0, 16)                    # a holder without spectra is a freed holder
    for ke, me in (([0.1], [0, 1]), ([0, 0.1], [1.0])):
        with pytest.raises(ValueError, match='two edges'):
            LF.linear_power(lin, ke, me, [0])
        with pytest.raises(ValueError, match='two edges'):
            recon_power(np.zeros((10, 3), dtype=np.float32), None, lin, ke, me, [0])
    with pytest.raises(RuntimeError, match='freed'):
        LF.linear_power(lin, [0, 0.1], [0, 1], [0])
    with pytest.raises(RuntimeError, match='freed'):
        LF.linear_power3d(lin)
    with pytest.raises(TypeError):
        LF.linear_power('not a holder', [0, 0.1], [0, 1], [0])
    with pytest.raises(ValueError, match='rec_algo'):
        LF.combine_field_spectra_k3D_lcv(1.5, 0.8, 0.6, lin, 16, 100.0, 10.0, 'rectangular')
    with pytest.raises(ValueError, match='R'):
        LF.combine_field_spectra_k3D_lcv(1.5, 0.8, 0.6, lin, 16, 100.0, None, 'reciso')
    with pytest.raises(RuntimeError, match='freed'):
        LF.combine_field_spectra_k3D_lcv(1.5, 0.8, 0.6, lin, 16, 100.0, None, 'recsym')
    good = np.zeros((10, 3), dtype=np.float32)
    with pytest.raises(ValueError):
        recon_power(np.zeros((10, 2), dtype=np.float32), None, lin, [0, 0.1], [0, 1], [0])
    with pytest.raises(ValueError):
        recon_power(good, np.zeros((0, 3), dtype=np.float32), lin, [0, 0.1], [0, 1], [0])
    with pytest.raises(TypeError):
        recon_power(np.zeros((10, 3), dtype=np.int32), None, lin, [0, 0.1], [0, 1], [0])
    with pytest.raises(TypeError):
        recon_power(good, np.zeros((10, 3), dtype=np.float16), lin, [0, 0.1], [0, 1], [0])
    with pytest.raises(TypeError, match='float32'):
        recon_power(_device((10, 3), np.float64), None, lin, [0, 0.1], [0, 1], [0])
    with pytest.raises(TypeError, match='float32'):
        recon_power(good, _device((10, 3), np.float64), lin, [0, 0.1], [0, 1], [0])
    with pytest.raises(ValueError, match='pasting'):
        recon_power(good, None, lin, [0, 0.1], [0, 1], [0], paste='NGP')
    with pytest.raises(RuntimeError, match='freed'):
        recon_power(good, None, lin, [0, 0.1], [0, 1], [0])
    with pytest.raises(RuntimeError, match='freed'):
        lin.spectrum('delta')
    with pytest.raises(KeyError):
        lin.spectrum('nabla2')


@pytest.fixture(scope='module')
def gold():
    g = {}
    for name in ('lcv_cases', 'lcv_recon_cases'):
        g.update(load_golden(name))
    return g


def test_golden_files_hold_every_case_with_a_usable_e_ref(gold):
    def names(key):
        return [str(s) for s in gold[key]]
    assert names('linear_names') == LINEAR and names('recon_names') == RECON and names('combine_names') == COMBINE
    binned = ('P_kmu', 'N_kmu', 'P_ell', 'N_ell', 'e_ref')
    for c in LINEAR:
        n = int(c[5:7])
        assert gold[f'linear/{c}/delta_lin'].dtype == np.float32 and gold[f'linear/{c}/delta_lin'].shape == (n, n, n)
        assert len(gold[f'linear/{c}/k_bin_edges']) == n // 2 + 1 and len(gold[f'linear/{c}/mu_bin_edges']) == 5
        assert list(gold[f'linear/{c}/poles']) == [0, 2, 4]
        for k in ('delta', 'deltamu2'):
            assert gold[f'linear/{c}/spec_{k}'].dtype == np.complex64 and gold[f'linear/{c}/spec_{k}'].shape == (n, n, n // 2 + 1)
            assert f'linear/{c}/e_ref_spec_{k}' in gold
        for p in LIN_PAIRS:
            assert {f'linear/{c}/{q}_{p}' for q in binned + ('P_k3D', 'e_ref_k3D')} <= set(gold), (c, p)
            assert gold[f'linear/{c}/P_k3D_{p}'].dtype == np.float32 and gold[f'linear/{c}/P_k3D_{p}'].shape == (n, n, n // 2 + 1)
    # the unfiltered field has full power on the Nyquist planes; the filtered ones have next to none there
    full, filt = gold['linear/white16_unfiltered/P_k3D_delta_delta'], gold['linear/white16/P_k3D_delta_delta']
    assert full[8].mean() > 0.3 * full.mean() and full[:, :, 8].mean() > 0.3 * full.mean() and filt[8].mean() < 0.1 * filt.mean()
    L = float(gold['linear/white16/Lbox'])
    cell = L / 16
    assert str(gold['recon/linear_case']) == 'white16' and list(gold['recon/poles']) == [0, 2, 4]
    for key, count in (('tracer_pos', 3000), ('random_pos', 12000)):
        p = gold[f'recon/{key}']
        assert p.dtype == np.float32 and p.shape == (count, 3)
        assert p.min() < -2 * cell and p.max() > L + 2 * cell            # a few cells outside [0, Lbox) on both sides
    for c in RECON:
        assert gold[f'recon/{c}/spec_tr'].dtype == np.complex64 and gold[f'recon/{c}/spec_tr'].shape == (16, 16, 9)
        assert len(gold[f'recon/{c}/mu_bin_edges']) == (2 if c.endswith('mu1') else 5)
        for p in TR_PAIRS:
            assert {f'recon/{c}/{q}_{p}' for q in binned + ('P_k3D', 'e_ref_k3D')} <= set(gold), (c, p)
        assert gold[f'recon/{c}/P_kmu_tr_tr'].shape == ((8,) if c.endswith('mu1') else (8, 4))
        assert gold[f'recon/{c}/P_ell_tr_tr'].shape == (3, 8)
    assert not np.array_equal(gold['recon/TSC_TT/spec_tr'], gold['recon/TSC_TT_norandoms/spec_tr'])
    for a in COMBINE:
        for k in ('pk_tt', 'pk_ll', 'pk_lt'):
            assert gold[f'combine/{a}/{k}'].dtype == np.float32 and gold[f'combine/{a}/{k}'].shape == (16, 16, 9)
            assert f'combine/{a}/e_ref_{k}' in gold
    assert 'reference' in str(gold['combine/recsym/source']) and 'ValueError' in str(gold['combine/reciso/source'])
    assert not np.array_equal(gold['combine/recsym/pk_ll'], gold['combine/reciso/pk_ll'])
    e_refs = {k: float(v) for k, v in gold.items() if '/e_ref' in k}
    assert len(e_refs) == len(LINEAR) * (2 + 2 * len(LIN_PAIRS)) + len(RECON) * (1 + 2 * len(TR_PAIRS)) + len(COMBINE) * 3
    for k, v in e_refs.items():
        assert 0 < v < 1e-3 and np.isfinite(v), (k, v)            # float32 noise, not a different formula


def test_header_declares_the_lcv_entry_points_and_the_makefile_builds_them():
    text = (REPO / 'include' / 'abacus_hip.h').read_text()
    names = ('abacus_lcv_linear_dev', 'abacus_lcv_spectrum_sub_dev', 'abacus_lcv_power3d', 'abacus_lcv_combine_k3d')
    for name in names:
        assert re.search(rf'\bint {name}\(', text), name
    assert text.index('linear control variates') > text.index("Zel'dovich control variates")
    src = (REPO / 'abacusutils_amd' / 'csrc' / 'lcv.hip').read_text()       # the transform and memory helpers are those of mesh_common.hpp
    for name in names:
        assert re.search(rf'\bint {name}\(', src), name
    assert 'lcv.hip' in (REPO / 'abacusutils_amd' / 'csrc' / 'Makefile').read_text()
