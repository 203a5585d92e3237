"""CPU oracle (oracle/abacus_oracle.c) vs the reference's own fixtures and the golden
vectors captured from the reference (oracle/make_golden.py).  No GPU needed."""
import numpy as np
import pytest
from conftest import (SYNTH_CASES, assert_mock_equal, input_checksum, load_golden, synth_case, unpack_inputs,
                      unpack_mock)

from oracle import oracle


@pytest.mark.parametrize('name', ['hod_mini', 'hod_lc'])
@pytest.mark.parametrize('nthread', [1, 4])
def test_reference_fixture(name, nthread):
    """tests/ref_hod/**/galaxies_rsd/{LRGs,ELGs}.dat of the reference (tests/test_hod.py:109-134,
    tests/test_lc_hod.py): ids exact, floats to tests/common.py's rtol 1e-7 - here bit-exact."""
    g = load_golden(name)
    hd, pd, params = unpack_inputs(g)
    import yaml  # noqa: F401  (HOD of tests/abacus_hod.yaml:31-70)
    from abacusutils_amd import synth
    tracers = {'LRG': synth.LRG_PARAMS, 'ELG': synth.ELG_PARAMS}
    mock = oracle.gen_gal_cat(hd, pd, tracers, params, Nthread=nthread, enable_ranks=False, rsd=True)
    want = unpack_mock(g, 'expect')
    assert_mock_equal(mock, want, exact=False, rtol=1e-14)   # ECSV text round trip
    assert_mock_equal(mock, unpack_mock(g, 'shim'), exact=True)   # what the reference returned, bitwise


@pytest.mark.parametrize('name', SYNTH_CASES)
def test_synthetic_golden(name):
    g = load_golden('hod_synth_' + name)
    hd, pd, params, tracers, ranks, rsd = synth_case(g)
    assert input_checksum(hd, pd) == float(g['meta.checksum']), 'numpy Generator stream changed'
    mock = oracle.gen_gal_cat(hd, pd, tracers, params, Nthread=5, enable_ranks=ranks, rsd=rsd)
    assert_mock_equal(mock, unpack_mock(g, 'expect'), exact=True)


def test_thread_count_invariance():
    g = load_golden('hod_synth_all_rich')
    hd, pd, params, tracers, ranks, rsd = synth_case(g)
    a = oracle.gen_gal_cat(hd, pd, tracers, params, Nthread=1, enable_ranks=ranks, rsd=rsd)
    b = oracle.gen_gal_cat(hd, pd, tracers, params, Nthread=7, enable_ranks=ranks, rsd=rsd)
    assert_mock_equal(a, b)


def test_rsd_must_be_bool():
    g = load_golden('hod_mini')
    hd, pd, params = unpack_inputs(g)
    from abacusutils_amd import synth
    with pytest.raises(ValueError):
        oracle.gen_gal_cat(hd, pd, {'LRG': synth.LRG_PARAMS}, params, rsd=1)


def test_empty_inputs():
    from abacusutils_amd import synth
    hd, pd, params = synth.synth_hod_inputs(50, 50, seed=1)
    hd = {k: v[:0] for k, v in hd.items()}
    pd = {k: v[:0] for k, v in pd.items()}
    mock = oracle.gen_gal_cat(hd, pd, {'LRG': synth.LRG_PARAMS}, params, Nthread=3)
    assert mock['LRG']['Ncent'] == 0 and len(mock['LRG']['x']) == 0


@pytest.mark.parametrize('seed', range(40))
def test_random_parameter_sweep_against_reference_digests(seed):
    """40 seeded random parameter sets (tests/sweep.py) run through the shimmed reference by oracle/make_golden.py sweep:
    the oracle reproduces every catalogue bit for bit (counts + SHA-256 of the eight columns)"""
    import hashlib
    from sweep import sweep_case
    g = np.load(__import__('pathlib').Path(__file__).parent / 'golden' / 'hod_sweep.npz')
    hd, pd, params, tracers, ranks, rsd = sweep_case(seed)
    assert input_checksum(hd, pd) == float(g[f'case{seed}.checksum']), 'numpy Generator stream changed'
    mock = oracle.gen_gal_cat(hd, pd, tracers, params, Nthread=4, enable_ranks=ranks, rsd=rsd)
    assert set(mock) == set(tracers)
    for tr, cols in mock.items():
        assert len(cols['x']) == int(g[f'case{seed}.{tr}.n']) and int(cols['Ncent']) == int(g[f'case{seed}.{tr}.ncent'])
        h = hashlib.sha256()
        for c in ('x', 'y', 'z', 'vx', 'vy', 'vz', 'mass'):
            h.update(np.ascontiguousarray(cols[c], dtype=np.float64).tobytes())
        h.update(np.ascontiguousarray(cols['id'], dtype=np.int64).tobytes())
        assert np.array_equal(np.frombuffer(h.digest(), dtype=np.uint8), g[f'case{seed}.{tr}.sha']), (seed, tr)


def _corners():
    from corners import CORNERS
    return CORNERS


@pytest.mark.parametrize('name', _corners())
def test_corner_cases_against_reference_digests(name):
    """the parameter and catalogue corners of tests/corners.py (guards of the filter failing, NaN parameters, masses outside
    the key window, zero / negative weights) run through the shimmed reference by oracle/make_golden.py corners: the oracle
    reproduces every catalogue bit for bit (counts + SHA-256 of the eight columns).  A NaN parameter populates nothing; it
    does not raise."""
    import hashlib
    from corners import corner_case, corner_checksum
    g = np.load(__import__('pathlib').Path(__file__).parent / 'golden' / 'hod_corners.npz')
    hd, pd, params, tracers, ranks, rsd = corner_case(name)
    assert corner_checksum(hd, pd) == float(g[f'{name}.checksum']), 'numpy Generator stream changed'
    mock = oracle.gen_gal_cat(hd, pd, tracers, params, Nthread=4, enable_ranks=ranks, rsd=rsd)
    assert set(mock) == set(tracers)
    for tr, cols in mock.items():
        assert (len(cols['x']), int(cols['Ncent'])) == (int(g[f'{name}.{tr}.n']), int(g[f'{name}.{tr}.ncent'])), (name, tr)
        h = hashlib.sha256()
        for c in ('x', 'y', 'z', 'vx', 'vy', 'vz', 'mass'):
            h.update(np.ascontiguousarray(cols[c], dtype=np.float64).tobytes())
        h.update(np.ascontiguousarray(cols['id'], dtype=np.int64).tobytes())
        assert np.array_equal(np.frombuffer(h.digest(), dtype=np.uint8), g[f'{name}.{tr}.sha']), (name, tr)
