#!/usr/bin/env python
"""Times the minimum spanning forest on one MI355X beside the counts in spheres of the same catalogue.

    python scripts/mst_probe.py [--n 1e7] [--reps 5] [--out FILE.json]

Workloads: `n` points in a 2 Gpc/h box, all columns resident in HBM (float32 DeviceArray): the uniform and the clustered
catalogue of scripts/groups_probe.py, each with rmax at 1.0 and at 1.6 mean separations (`groups.linking_lengths`) - at 1.6 the
uniform catalogue percolates into one tree, the contended case of the slot atomics.  The yardstick is `count_in_spheres` of the
set around itself with the single radius rmax, in the same process: the same staging, the same sort and the full 27-cell walk.

Per row: HIP-event time of the whole call on the library stream (one warm-up, then the mean, smallest and largest of `reps`
calls; a call ends with its copies to the host), the library's event time per kernel from `reps` further calls, and from `reps`
more with the option `mst_round_names` the time of every kernel of every round; rounds, and per round the points scanned (live),
the points settled so far, the points with an edge out of their tree and the edges emitted (abacus_mst_stats); candidates per
second of mst_scan over all rounds; the edge sort; the first round's scan as a multiple of sphere_count.  Prints one JSON line;
--out also writes it to a file."""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from abacusutils_amd import _lib  # noqa: E402
from abacusutils_amd.analysis import groups as G  # noqa: E402
from abacusutils_amd.analysis import mst as M  # noqa: E402
from abacusutils_amd.analysis import spheres as S  # noqa: E402
from groups_probe import clustered  # noqa: E402
from spheres_probe import stats, timed  # noqa: E402


def profile_all(cap=512):
    """_lib.profile_get with room for a name per kernel per round"""
    names, ms, cnt = (C.c_char_p * cap)(), (C.c_double * cap)(), (C.c_int64 * cap)()
    k = _lib.lib().abacus_profile_get(names, ms, cnt, cap)
    return {names[i].decode(): (ms[i], cnt[i]) for i in range(min(k, cap))}


def per_round_ms(call, reps):
    _lib.set_option('mst_round_names', 1)
    _lib.profile_reset()
    _lib.profile_enable(True)
    for _ in range(reps):
        call()
    _lib.sync()
    _lib.profile_enable(False)
    _lib.set_option('mst_round_names', 0)
    out = {}
    for name, (ms, cnt) in profile_all().items():
        if '@' in name and cnt:
            kernel, rnd = name.split('@')
            out.setdefault(kernel, {})[int(rnd)] = round(ms / cnt, 4)
    return {k: [v[r] for r in sorted(v)] for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', default='1e7')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    n, L, kmax = int(float(a.n)), 2000.0, 2048
    print('device:', _lib.device_name(), file=sys.stderr)
    rows, last = {}, {}
    for cat, p in (('uniform', np.random.default_rng(500).random((n, 3), dtype=np.float32) * np.float32(L)), ('clustered', clustered(n, L, 501))):
        data = [_lib.DeviceArray(np.ascontiguousarray(p[:, i])) for i in range(3)]
        for sep in (1.0, 1.6):
            rmax = G.linking_lengths(n, L, sep)[0]
            name = f'{cat}, rmax {sep}'
            call = lambda: last.__setitem__('t', M.minimum_spanning_tree(*data, L, rmax, return_degree=True, return_labels=False))  # noqa: E731
            row = rows[name] = timed(call, a.reps, 'mst_scan')
            st, t = M.last_stats(), last['t']
            per = st.pop('per_round')
            row.update(stats=st, rmax=rmax, nedges=t['nedges'], ncomp=t['ncomp'], longest_edge_in_mean_separations=float(t['length'][-1] / rmax * sep),
                       live_per_round=per[:, 0].tolist(), settled_before_round=(n - per[:, 0].astype(np.int64)).tolist(),
                       with_candidate_per_round=per[:, 1].tolist(), edges_per_round=per[:, 2].tolist(),
                       degree_fractions=(np.bincount(np.minimum(t['degree'], 8), minlength=9) / n).round(5).tolist())
            assert t['nedges'] + t['ncomp'] == n and int(per[:, 2].sum()) == t['nedges']
            row['round_ms'] = per_round_ms(call, a.reps)
            _lib.set_option('mst_always_atomic', 1)         # the comparator: every point with a candidate sends its atomicMin
            try:
                v = timed(call, a.reps, 'mst_scan')
            finally:
                _lib.set_option('mst_always_atomic', 0)
            row['always_atomic'] = {'event_ms_mean': v['event_ms_mean'], 'mst_scan_ms': v['kernels_ms_per_call'].get('mst_scan')}
            assert last['t']['nedges'] == t['nedges'] and np.array_equal(last['t']['i'], t['i']) and np.array_equal(last['t']['j'], t['j'])
            name = f'{cat}, rmax {sep}: count_in_spheres'
            rows[name] = timed(lambda: last.__setitem__('s', S.count_in_spheres(*data, L, [rmax], kmax=kmax)), a.reps, 'sphere_count')
            rows[name]['stats'] = stats('abacus_spherecount_stats')
            hist = last['s']['hist'][0]
            # a point without a neighbour inside rmax is a tree of one, and the only kind of point the first round settles
            assert int(hist[0]) == n - int(per[0, 1]), 'the first scan and the sphere counts disagree on the points without a neighbour'
            k0, ks = row['round_ms'].get('mst_scan', [None])[0], rows[name]['kernels_ms_per_call'].get('sphere_count')
            row['first_scan_over_sphere_count'] = None if not (k0 and ks) else round(k0 / ks, 3)
        for d in data:
            d.free()
    for r in rows.values():
        k = r['kernels_ms_per_call'].get(r['kernel'])
        r['candidates_per_s_kernel'] = None if not k else float(f"{r['stats']['candidates'] / (k * 1e-3):.4g}")
    line = {'n': n, 'Lbox': L, 'reps': a.reps, 'rows': rows}
    print(json.dumps(line))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(line, indent=1) + '\n')


if __name__ == '__main__':
    main()
