"""No-GPU checks of the Zel'dovich-control-variates package (abacusutils_amd.hod.zcv): the public names and argument lists of
ic_fields are the reference's, bad arguments raise before the device library is touched, the golden files hold every case the GPU
tests list with a usable e_ref, and the C ABI declares the new entry points."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
from conftest import load_golden

REPO = Path(__file__).resolve().parent.parent
E = inspect.Parameter.empty

FILTER = ['white16_half', 'white16_fifth', 'white24_half', 'white24_fifth']
FIELDS = ['filtered_white16_half', 'filtered_white24_half', 'white16_unfiltered', 'lognormal24', 'planewave16']
SPECTRAL = ['filter_field', 'n2_fft', 'sij_fft_00', 'sij_fft_01', 'sij_fft_02', 'sij_fft_11', 'sij_fft_12', 'sij_fft_22', 'add_ij',
            'dk_to_s2', 'dk_to_n2']
LATTICE = ['f0', 'f0.8']
ADVECT = ['TSC_TT', 'TSC_FF', 'CIC_TT', 'CIC_FF']
KEYNAMES = ['1cb', 'delta', 'delta2', 'tidal2', 'nabla2']
PAIRS = [f'{a}_{b}' for i, a in enumerate(KEYNAMES) for j, b in enumerate(KEYNAMES) if i >= j]


def _sig(f):
    return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]


def test_ic_fields_signatures_are_the_references():
    """abacusnbody/hod/zcv/ic_fields.py:79, 111, 152, 193, 259, 271, 312, 336, written out"""
    from abacusutils_amd.hod.zcv import ic_fields as I
    assert _sig(I.gaussian_filter) == [('field', E), ('nmesh', E), ('lbox', E), ('kcut', E)]
    assert _sig(I.filter_field) == [('delta_k', E), ('n1d', E), ('L', E), ('kcut', E), ('dtype', np.float32)]
    assert _sig(I.get_n2_fft) == [('delta_k', E), ('n1d', E), ('L', E), ('dtype', np.float32)]
    assert _sig(I.get_sij_fft) == [('i_comp', E), ('j_comp', E), ('delta_k', E), ('n1d', E), ('L', E), ('dtype', np.float32)]
    assert _sig(I.add_ij) == [('final_field', E), ('field_to_add', E), ('n1d', E), ('factor', 1.0), ('dtype', np.float32)]
    assert _sig(I.get_dk_to_s2) == [('delta_k', E), ('nmesh', E), ('lbox', E)]
    assert _sig(I.get_dk_to_n2) == [('delta_k', E), ('nmesh', E), ('lbox', E)]
    assert _sig(I.get_fields) == [('delta_lin', E), ('Lbox', E), ('nmesh', E)]
    assert set(I.__all__) == {'gaussian_filter', 'filter_field', 'get_n2_fft', 'get_sij_fft', 'add_ij', 'get_dk_to_s2', 'get_dk_to_n2',
                              'get_fields'}


def test_advect_and_tracer_signatures():
    from abacusutils_amd.hod import zcv
    from abacusutils_amd.hod.zcv import advect_fields as A, tracer_power as T
    keys = ('1cb', 'delta', 'delta2', 'tidal2', 'nabla2')
    assert _sig(A.lattice_positions) == [('disp_x', E), ('disp_y', E), ('disp_z', E), ('Lbox', E), ('D', E), ('f_growth', 0.0),
                                         ('device_out', False)]
    assert _sig(A.advect) == [('disp', E), ('fields', E), ('Lbox', E), ('nmesh', E), ('D', E), ('f_growth', 0.0), ('paste', 'TSC'),
                              ('compensated', True), ('interlaced', True), ('keynames', keys)]
    assert _sig(A.field_power) == [('adv', E), ('k_bin_edges', E), ('mu_bin_edges', E), ('poles', E), ('D', E)]
    assert _sig(T.tracer_power) == [('tracer_pos', E), ('adv', E), ('k_bin_edges', E), ('mu_bin_edges', E), ('poles', E), ('D', E)]
    assert 'in place' in T.tracer_power.__doc__.lower()
    assert zcv.AdvectedFields is A.AdvectedFields and all(hasattr(A.AdvectedFields, m) for m in ('spectrum', 'free', '__enter__', '__exit__'))
    # field_D = [1, D, D^2, D^2, D] by field name
    assert [A.field_growth(k, 0.5) for k in keys] == [1.0, 0.5, 0.25, 0.25, 0.5]


@pytest.fixture
def no_library(monkeypatch):
    """any attempt to load (or use) the device library fails the test"""
    from abacusutils_amd import _lib

    def boom(*a, **k):
        raise AssertionError('the device library was touched before the arguments were checked')
    monkeypatch.setattr(_lib, 'lib', boom)


def test_bad_arguments_raise_before_the_library_is_loaded(no_library):
    from abacusutils_amd.hod.zcv import ic_fields as I
    from abacusutils_amd.hod.zcv.advect_fields import advect, lattice_positions
    from abacusutils_amd.hod.zcv.tracer_power import tracer_power
    z15 = np.zeros((15, 15, 15), dtype=np.float32)
    z16 = np.zeros((16, 16, 16), dtype=np.float32)
    k16 = np.zeros((16, 16, 9), dtype=np.complex64)
    for call in (lambda: I.get_fields(z15, 100.0, 15), lambda: I.gaussian_filter(z15, 15, 100.0, 0.1),
                 lambda: I.get_dk_to_s2(np.zeros((15, 15, 8), dtype=np.complex64), 15, 100.0),
                 lambda: I.get_dk_to_n2(np.zeros((15, 15, 8), dtype=np.complex64), 15, 100.0),
                 lambda: advect([z15, z15, z15], {}, 100.0, 15, 0.5, keynames=('1cb',))):
        with pytest.raises(ValueError, match='odd'):                    # the reference itself fails on odd meshes
            call()
    with pytest.raises(ValueError, match='cubic'):
        I.get_fields(np.zeros((16, 16, 12), dtype=np.float32), 100.0, 16)
    with pytest.raises(ValueError, match='nmesh'):
        I.gaussian_filter(z16, 18, 100.0, 0.1)
    with pytest.raises(ValueError):
        I.gaussian_filter(z16, 16, 100.0, 0.0)                           # kcut must be positive
    with pytest.raises(ValueError):
        I.get_n2_fft(np.zeros((16, 16, 16), dtype=np.complex64), 16, 100.0)      # not (N, N, N/2+1)
    with pytest.raises(ValueError):
        I.get_sij_fft(0, 3, k16, 16, 100.0)
    with pytest.raises(TypeError):
        I.get_fields(np.zeros((16, 16, 16), dtype=np.complex64), 100.0, 16)
    for call in (lambda: I.filter_field(k16, 16, 100.0, 0.1, dtype=np.float64), lambda: I.get_n2_fft(k16, 16, 100.0, dtype=np.float64),
                 lambda: I.get_sij_fft(0, 1, k16, 16, 100.0, dtype=np.float64), lambda: I.add_ij(z16.copy(), z16, 16, dtype=np.float64)):
        with pytest.raises(TypeError, match='float32'):
            call()
    with pytest.raises(TypeError):
        I.add_ij(np.zeros((16, 16, 16), dtype=np.float64), z16, 16)       # updated in place: must be float32
    with pytest.raises(TypeError):
        lattice_positions(z16.astype(np.float64), z16, z16, 100.0, 0.5)
    with pytest.raises(ValueError):
        lattice_positions(z16, z16, np.zeros((18, 18, 18), dtype=np.float32), 100.0, 0.5)
    fields = {k: z16 for k in KEYNAMES[1:]}
    with pytest.raises(KeyError):
        advect([z16, z16, z16], fields, 100.0, 16, 0.5, keynames=('1cb', 'vorticity'))
    with pytest.raises(KeyError):
        advect([z16, z16, z16], {'delta': z16}, 100.0, 16, 0.5)
    with pytest.raises(ValueError, match='nmesh'):
        advect([z16, z16, z16], fields, 100.0, 18, 0.5)
    with pytest.raises(ValueError, match='nmesh'):
        advect([z16, z16, z16], dict(fields, nabla2=np.zeros((18, 18, 18), dtype=np.float32)), 100.0, 16, 0.5)
    with pytest.raises(TypeError):
        advect([z16, z16, z16], dict(fields, nabla2=z16.astype(np.float64)), 100.0, 16, 0.5)
    with pytest.raises(ValueError):
        advect([z16, z16, z16], fields, 100.0, 16, 0.5, paste='NGP')
    with pytest.raises(ValueError):
        tracer_power(np.zeros((10, 2), dtype=np.float32), None, [0, 0.1], [0, 1], [0], 0.5)
    with pytest.raises(TypeError):
        tracer_power(np.zeros((10, 3), dtype=np.int32), None, [0, 0.1], [0, 1], [0], 0.5)


@pytest.fixture(scope='module')
def gold():
    g = {}
    for name in ('zcv_cases', 'zcv_fields_cases', 'zcv_advect_cases'):
        g.update(load_golden(name))
    return g


def test_golden_files_hold_every_case_with_a_usable_e_ref(gold):
    def names(key):
        return [str(s) for s in gold[key]]
    assert names('filter_names') == FILTER and names('fields_names') == FIELDS and names('spectral_names') == SPECTRAL
    assert names('lattice_names') == LATTICE and names('advect_names') == ADVECT and names('keynames') == KEYNAMES
    for n in FILTER:
        assert {f'filter/{n}/{k}' for k in ('field', 'Lbox', 'kcut', 'out', 'e_ref')} <= set(gold)
    for n in FIELDS:
        assert {f'fields/{n}/{k}' for k in ('delta', 'Lbox', 'd', 'd2', 's2', 'n2', 'e_ref_d', 'e_ref_d2', 'e_ref_s2', 'e_ref_n2')} <= set(gold)
    for n in SPECTRAL:
        assert {f'spectral/{n}/out', f'spectral/{n}/e_ref'} <= set(gold)
    for n in LATTICE:
        assert gold[f'lattice/{n}/pos'].dtype == np.float32 and gold[f'lattice/{n}/pos'].shape == (gold['lattice/disp_x'].size, 3)
    for m in ADVECT:
        for k in KEYNAMES:
            assert gold[f'advect/{m}/spec_{k}'].dtype == np.complex64 and gold[f'advect/{m}/spec_{k}'].shape == (16, 16, 9)
        for p in PAIRS + ['tr_tr'] + [f'{k}_tr' for k in KEYNAMES]:
            head = 'tracer' if p.endswith('_tr') else 'advect'
            assert {f'{head}/{m}/{q}_{p}' for q in ('P_kmu', 'N_kmu', 'P_ell', 'N_ell', 'e_ref')} <= set(gold), (m, p)
    e_refs = {k: float(v) for k, v in gold.items() if '/e_ref' in k}
    assert len(e_refs) == len(FILTER) + 4 * len(FIELDS) + len(SPECTRAL) + len(ADVECT) * (len(KEYNAMES) + len(PAIRS) + 1 + len(KEYNAMES))
    for k, v in e_refs.items():
        assert np.isfinite(v) and v > 0, (k, v)
        assert v < 1e-3, (k, v)            # float32 noise, not a different formula
    # the lattice case wraps many sites; the tracer positions lie in [-L/2, L/2) and their shifted copy in [0, L)
    L = float(gold['advect/Lbox'])
    assert (gold['tracer/pos'] >= -L / 2).all() and (gold['tracer/pos'] < L / 2).all() and len(gold['tracer/pos']) == 2000
    assert (gold['tracer/pos_shifted'] >= 0).all() and (gold['tracer/pos_shifted'] < L).all()


def test_every_pair_counts_the_same_modes(gold):
    """N_kmu depends on the mesh and the bin edges alone: one set of counts for all 15 + 6 spectra of all four modes"""
    first = gold[f'advect/{ADVECT[0]}/N_kmu_{PAIRS[0]}']
    assert first.shape == (8, 4) and first.sum() > 0
    for m in ADVECT:
        for p in PAIRS:
            assert np.array_equal(gold[f'advect/{m}/N_kmu_{p}'], first) and gold[f'advect/{m}/N_kmu_{p}'].sum() == first.sum()
            assert np.array_equal(gold[f'advect/{m}/N_ell_{p}'], first.sum(axis=1))
        for p in ['tr_tr'] + [f'{k}_tr' for k in KEYNAMES]:
            assert np.array_equal(gold[f'tracer/{m}/N_kmu_{p}'], first) and gold[f'tracer/{m}/N_kmu_{p}'].sum() == first.sum()


def test_header_declares_the_zcv_entry_points():
    text = (REPO / 'include' / 'abacus_hip.h').read_text()
    for name in ('abacus_zcv_filter_dev', 'abacus_zcv_spectral_dev', 'abacus_zcv_add_ij_dev', 'abacus_zcv_dk_to_dev', 'abacus_zcv_fields_dev',
                 'abacus_zcv_lattice_dev', 'abacus_zcv_shift_wrap_dev', 'abacus_zcv_spectrum_bytes', 'abacus_zcv_check_memory',
                 'abacus_zcv_spectrum_dev', 'abacus_zcv_advect_dev', 'abacus_zcv_power_pair', 'abacus_zcv_spectrum_fetch', 'abacus_zcv_release'):
        assert re.search(rf'\bint {name}\(', text), name
    src = (REPO / 'abacusutils_amd' / 'csrc' / 'zcv.hip').read_text()
    assert 'zcv.hip' in (REPO / 'abacusutils_amd' / 'csrc' / 'Makefile').read_text()
    assert 'atomicAdd' not in src                          # the means are two-stage reductions, not floating-point atomics
    for part in ('lcv.hip', 'recon.hip', 'lc_power.hip', 'bispectrum.hip', 'mesh_common.hpp'):       # what came out of zcv.hip: the same rule
        assert 'atomicAdd' not in (REPO / 'abacusutils_amd' / 'csrc' / part).read_text(), part
