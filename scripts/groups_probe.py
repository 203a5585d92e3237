#!/usr/bin/env python
"""Times the friends-of-friends group finder on one MI355X beside the counts in spheres of the same catalogue.

    python scripts/groups_probe.py [--n 1e7] [--reps 5] [--out FILE.json]

Workloads: `n` points in a 2 Gpc/h box, all columns resident in HBM (float32 DeviceArray), labels not copied back (a second row
per workload with labels on): a uniform catalogue and a clustered one (a quarter of the points in Gaussian clumps of 100 members
and sigma = 1 Mpc/h around uniform centres, the recipe of the tests scaled up), each with the linking lengths of
`groups.linking_lengths` at the Berlind et al. (2006) defaults - spheres of b_perp, and cylinders (b_perp, b_par) - and, on the
clustered set, spheres of 0.2 mean separations: the dense-clump case.  The yardstick is `count_in_spheres` of the set around
itself with the single radius b_perp (pimax = b_par for the cylinders; kmax = 2048): the same sort and the same walk, over all
27 cells, with a cheaper reduction.

Per row: HIP-event time of the whole call on the library stream (one warm-up, then the mean, smallest and largest of `reps`
calls; a call ends with its copies to the host), the library's event time per kernel from `reps` further calls, candidates and
links from abacus_fof_stats, and candidates and links per second of fof_link.  The group finder is checked against the sphere
counts: the sum of the per-point counts is twice the links.  Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from abacusutils_amd import _lib  # noqa: E402
from abacusutils_amd.analysis import groups as G  # noqa: E402
from abacusutils_amd.analysis import spheres as S  # noqa: E402
from spheres_probe import stats, timed  # noqa: E402


def clustered(n, L, seed):
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3), dtype=np.float32) * np.float32(L)
    k = n // 4
    centres = rng.random((max(k // 100, 1), 3), dtype=np.float32) * np.float32(L)
    p[:k] = (centres[rng.integers(0, len(centres), k)] + rng.normal(0.0, 1.0, (k, 3)).astype(np.float32)) % np.float32(L)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', default='1e7')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    n, L, nmax, kmax = int(float(a.n)), 2000.0, 64, 2048      # kmax: above any point's friends, so that the sphere counts are exact
    print('device:', _lib.device_name(), file=sys.stderr)
    bp, bl = G.linking_lengths(n, L)
    b02 = G.linking_lengths(n, L, 0.2)[0]
    rows, last = {}, {}
    for cat, p in (('uniform', np.random.default_rng(500).random((n, 3), dtype=np.float32) * np.float32(L)), ('clustered', clustered(n, L, 501))):
        data = [_lib.DeviceArray(np.ascontiguousarray(p[:, i])) for i in range(3)]
        cases = [('spheres', bp, None), ('cylinders', bp, bl)] + ([('spheres 0.2', b02, None)] if cat == 'clustered' else [])
        for shape, b, par in cases:
            for variant in ('', ', labels'):
                name = f'{cat}, {shape}{variant}'
                rows[name] = timed(lambda: last.__setitem__('g', G.fof_groups(*data, L, b, b_par=par, nmax=nmax,
                                                                             return_labels=variant == ', labels')), a.reps, 'fof_link')
                st = G.last_stats()
                g = last['g']
                rows[name].update(stats=st, b_perp=b, b_par=par, ngroups=g['ngroups'], singletons=int(g['mult'][1]),
                                  groups_ge_10=int(g['mult'][10:].sum()), groups_ge_nmax=int(g['mult'][nmax]))
                assert int(g['mult'].sum()) == g['ngroups']
            name = f'{cat}, {shape}: count_in_spheres'
            rows[name] = timed(lambda: last.__setitem__('s', S.count_in_spheres(*data, L, [b], pimax=par, kmax=kmax)), a.reps, 'sphere_count')
            rows[name]['stats'] = stats('abacus_spherecount_stats')
            hist = last['s']['hist'][0]
            assert hist[kmax] == 0, 'a point with kmax or more friends: the check below needs exact counts'
            assert int((hist * np.arange(kmax + 1, dtype=np.uint64)).sum()) == 2 * st['links'], 'the group finder and the sphere counts disagree'
            assert int(hist[0]) == rows[f'{cat}, {shape}']['singletons']
        for d in data:
            d.free()
    for r in rows.values():
        k = r['kernels_ms_per_call'].get(r['kernel'])
        r['candidates_per_s_kernel'] = None if not k else float(f"{r['stats']['candidates'] / (k * 1e-3):.4g}")
        if 'links' in r['stats']:
            r['links_per_s_kernel'] = None if not k else float(f"{r['stats']['links'] / (k * 1e-3):.4g}")
    line = {'n': n, 'Lbox': L, 'nmax': nmax, 'reps': a.reps, 'rows': rows}
    print(json.dumps(line))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(line, indent=1) + '\n')


if __name__ == '__main__':
    main()
