#!/usr/bin/env python
"""Writes tests/golden/zcv_window_cases.npz: the REFERENCE's own hod/zcv/zenbu_window.py periodic_window_function run under the
identity Numba shim of oracle/shim on small meshes, next to the float64 statement of tests/window_statement.py.

    python scripts/make_window_golden.py /path/to/abacusutils

Needs the reference checkout, NumPy >= 2, SciPy and PyYAML; no GPU.  `classy`, `ZeNBu.zenbu`, `ZeNBu.zenbu_rsd` and
`abacusnbody.metadata` are imported by the reference module at module level but not used by the function called here: empty
stand-ins are registered for them.

The function cannot run as it stands outside Numba: its loop over the input bins writes one element past the end of `nmodes_in`
(`range(len(kout))`), which Numba does silently and NumPy refuses.  Its source is obtained at run time and, IN MEMORY ONLY, the
decorator is dropped and that loop bound becomes `nkout` (the extra element is never used); nothing of it is written anywhere.

With every case the file holds `e_ref_window` and `e_ref_keff`: the largest difference between the reference's result (sums in
float32, one mode after the other) and the float64 statement, relative to the largest entry of each of the nine (l, l') blocks
(the largest of the nine ratios) and of keff.  That is the float32 noise of the reference itself, from which the tests derive their
bounds.  A case whose e_ref exceeds 1e-3 is refused: then the two do not compute the same thing.

`logk` cases hold the statement only: below the first edge the reference's index -1 wraps to the last row of the l = 4 block.
"""
import contextlib
import inspect
import io
import sys
import types
import warnings
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / 'oracle' / 'shim'))
sys.path.insert(0, str(REPO / 'tests'))

E_REF_MAX = 1e-3
# nmesh, bins, box
LINEAR = [(8, 4, 100.0), (12, 6, 50.0), (16, 8, 200.0), (16, 5, 200.0)]
LOGK = [(8, 4, 100.0), (16, 6, 200.0)]


def import_reference(ref):
    """abacusnbody/__init__.py imports a generated version.py that a checkout does not have: register a bare package, and empty
    stand-ins for the modules zenbu_window.py imports without using them here"""
    pkg = types.ModuleType('abacusnbody')
    pkg.__path__ = [str(Path(ref) / 'abacusnbody')]
    sys.modules['abacusnbody'] = pkg
    meta = types.ModuleType('abacusnbody.metadata')
    meta.get_meta = None
    classy = types.ModuleType('classy')
    classy.Class = None
    zenbu_pkg = types.ModuleType('ZeNBu')
    zenbu_pkg.__path__ = []
    zenbu = types.ModuleType('ZeNBu.zenbu')
    zenbu.Zenbu = None
    zenbu_rsd = types.ModuleType('ZeNBu.zenbu_rsd')
    zenbu_rsd.Zenbu_RSD = None
    sys.modules.update({'abacusnbody.metadata': meta, 'classy': classy, 'ZeNBu': zenbu_pkg, 'ZeNBu.zenbu': zenbu,
                        'ZeNBu.zenbu_rsd': zenbu_rsd})
    import abacusnbody.hod.zcv.zenbu_window as Z
    return Z


def runnable_reference(Z):
    """periodic_window_function of the reference with the decorator dropped and the nmodes_in loop ending at nkout; compiled from
    its source in memory, in the namespace of its own module (its meshgrid)"""
    src = inspect.getsource(Z.periodic_window_function)
    lines = src.splitlines()
    assert lines[0].lstrip().startswith('@'), lines[0]
    body = '\n'.join(lines[1:])
    bound = 'for i in range(len(kout)):'
    assert body.count(bound) == 1
    body = body.replace(bound, 'for i in range(nkout):')
    ns = dict(vars(Z))
    exec(compile(body, '<reference periodic_window_function, loop bound nkout>', 'exec'), ns)
    return ns['periodic_window_function']


def quiet(f, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        return f(*a, **k)


def block_error(ref, st, nkout, nkin):
    """largest |ref - statement| of a block relative to the block's largest entry, the largest of the nine"""
    worst = 0.0
    for ell in range(3):
        for ellp in range(3):
            r = np.asarray(ref[ell * nkout:(ell + 1) * nkout, ellp * nkin:(ellp + 1) * nkin], dtype=np.float64)
            s = st[ell * nkout:(ell + 1) * nkout, ellp * nkin:(ellp + 1) * nkin]
            worst = max(worst, np.abs(r - s).max() / np.abs(s).max())
    return np.float64(worst)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    assert int(np.__version__.split('.')[0]) >= 2, 'golden vectors are generated under NumPy >= 2'
    from window_statement import window_statement
    Z = import_reference(sys.argv[1])
    ref_fn = runnable_reference(Z)
    G = {}
    names, logk_names = [], []

    def add(name, nmesh, lbox, kout, kin, k2weight, with_ref=True):
        kout, kin = np.asarray(kout, dtype=np.float64), np.asarray(kin, dtype=np.float64)
        nkout, nkin = len(kout) - 1, len(kin)
        w64, k64, S, nmodes, ksum = window_statement(nmesh, lbox, kout, kin, k2weight)
        pre = f'case/{name}/'
        G[pre + 'nmesh'], G[pre + 'lbox'], G[pre + 'k2weight'] = np.int64(nmesh), np.float64(lbox), np.bool_(k2weight)
        G[pre + 'kout'], G[pre + 'kin'] = kout, kin
        G[pre + 'window64'], G[pre + 'keff64'], G[pre + 'S'], G[pre + 'nmodes'], G[pre + 'ksum'] = w64, k64, S, nmodes, ksum
        if not with_ref:
            logk_names.append(name)
            print(f'{name}: statement only, {int(nmodes.sum())} modes counted')
            return
        window, keff = quiet(ref_fn, nmesh, lbox, kout.copy(), kin.copy(), k2weight)
        assert window.shape == (3 * nkout, 3 * nkin) and keff.shape == (nkout,), (window.shape, keff.shape)
        assert window.dtype == np.float64 and keff.dtype == np.float64, (window.dtype, keff.dtype)
        ew = block_error(window, w64, nkout, nkin)
        ek = np.float64(np.abs(keff - k64).max() / np.abs(k64).max())
        print(f'{name}: e_ref window {ew:.3g} keff {ek:.3g}')
        if not (ew <= E_REF_MAX and ek <= E_REF_MAX):
            sys.exit(f'{name}: the reference and the statement differ by more than {E_REF_MAX:g}: not written')
        G[pre + 'window'], G[pre + 'keff'], G[pre + 'e_ref_window'], G[pre + 'e_ref_keff'] = window, keff, ew, ek
        names.append(name)

    for nmesh, nb, lbox in LINEAR:
        kmax = np.pi * nmesh / lbox
        kout = np.linspace(0.0, kmax, nb + 1)
        kins = {'centres': 0.5 * (kout[1:] + kout[:-1]), 'fine': (np.arange(3 * nb) + 0.5) * (1.1 * kmax / (3 * nb))}
        for tag, kin in kins.items():
            for k2w in (True, False):
                add(f'n{nmesh}_b{nb}_{tag}_{"k2w" if k2w else "flat"}', nmesh, lbox, kout, kin, k2w)
    # every |k| with an integer square lies exactly on an edge: the <= / < rule of digitize
    kout = np.arange(9, dtype=np.float64)
    add('n16_integer_edges', 16, 2 * np.pi, kout, 0.5 * (kout[1:] + kout[:-1]), True)
    for nmesh, nb, lbox in LOGK:
        kmax = np.pi * nmesh / lbox
        kout = np.geomspace((1.0 - 1.0e-4) * 2.0 * np.pi / lbox, kmax, nb + 1)      # get_k_mu_edges with logk
        add(f'n{nmesh}_b{nb}_logk', nmesh, lbox, kout, 0.5 * (kout[1:] + kout[:-1]), True, with_ref=False)
    G['names'], G['logk_names'] = np.array(names), np.array(logk_names)
    out = REPO / 'tests' / 'golden' / 'zcv_window_cases.npz'
    np.savez_compressed(out, **G)
    print(out, out.stat().st_size, 'bytes')
    assert out.stat().st_size < 1 << 20


if __name__ == '__main__':
    main()
