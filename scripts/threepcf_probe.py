#!/usr/bin/env python
"""Times the 3PCF multipoles on one MI355X against the weighted pair count of the same catalogue.

    python scripts/threepcf_probe.py [--n 1e6] [--nrand 2e6] [--lmax 10] [--reps 3] [--out FILE.json]

Workload: `n` uniform points in a 1 Gpc/h box, 10 linear bins from 0 to 40 Mpc/h, lmax = 10, all columns resident in HBM
(float32 DeviceArray); then the D - R form with `nrand` randoms appended as a second set at weight -n / nrand.  The yardstick is
`_paircount_weighted` (mode 0, no separation sums) of the same columns, weights and edges: the same grid and the same candidate
pairs, so the ratio of the two kernels is the price of the harmonic work.

Per row: HIP-event time of the whole call on the library stream (one warm-up, then the mean, smallest and largest of `reps`
calls; a call ends with its copies to the host), the library's event time per kernel from `reps` further calls, the candidate
and counted pairs from abacus_threepcf_stats / abacus_paircount_stats, and both per second of the counting kernel.  The two
counters are checked against each other (npairs bit for bit).  Prints one JSON line; --out also writes it to a file."""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from abacusutils_amd import _lib  # noqa: E402
from abacusutils_amd.analysis import threepcf as P  # noqa: E402
from abacusutils_amd.analysis import tpcf_corrfunc as T  # noqa: E402
from abacusutils_amd.analysis.spheres import random_centres  # noqa: E402


def timed(call, reps, kernel):
    call()                                   # warm-up: code objects, work buffers
    _lib.sync()
    ms = []
    for _ in range(reps):
        t0, t1 = _lib.Event(), _lib.Event()
        t0.record()
        call()
        t1.record()
        ms.append(t1.elapsed_ms_since(t0))
    _lib.profile_reset()
    _lib.profile_enable(True)
    for _ in range(reps):
        call()
    _lib.sync()
    _lib.profile_enable(False)
    kern = {k: round(v / reps, 3) for k, (v, cnt) in sorted(_lib.profile_get().items(), key=lambda kv: -kv[1][0]) if cnt}
    return {'event_ms_mean': round(float(np.mean(ms)), 3), 'event_ms_min': round(min(ms), 3), 'event_ms_max': round(max(ms), 3),
            'kernels_ms_per_call': kern, 'kernel': kernel}


def pair_stats():
    cand, ncxy, ncz = C.c_uint64(0), C.c_int(0), C.c_int(0)
    _lib.check(_lib.lib().abacus_paircount_stats(C.byref(cand), C.byref(ncxy), C.byref(ncz), None))
    return {'candidates': int(cand.value), 'ncell': ncxy.value}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', default='1e6')
    ap.add_argument('--nrand', default='2e6')
    ap.add_argument('--lmax', type=int, default=10)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    n, nrand, L, lmax = int(float(a.n)), int(float(a.nrand)), 1000.0, a.lmax
    print('device:', _lib.device_name(), file=sys.stderr)
    edges = np.linspace(0.0, 40.0, 11).astype(np.float32)
    p = np.random.default_rng(700).random((n, 3), dtype=np.float32) * np.float32(L)
    data = [_lib.DeviceArray(np.ascontiguousarray(p[:, i])) for i in range(3)]
    rows, last, held = {}, {}, list(data)

    def pair(name, cols, w, tp_name):
        rows[name] = timed(lambda: last.__setitem__('w', T._paircount_weighted(0, *cols, L, edges, W1=w, want_rsum=False)), a.reps,
                           'pair_count_w')
        rows[name]['stats'] = dict(pair_stats(), counted=int(last['w'][0].sum()))
        assert np.array_equal(last['w'][0], last['t']['npairs']), 'the two counters disagree'
        assert rows[name]['stats']['candidates'] == rows[tp_name]['stats']['candidates'], 'the two walks differ'

    name = f'data alone, lmax {lmax}'
    rows[name] = timed(lambda: last.__setitem__('t', P.triplet_multipoles(*data, L, edges, lmax)), a.reps, 'threepcf_walk')
    rows[name]['stats'] = P.last_stats()
    pair('data alone: weighted pair count', data, None, name)
    if nrand:
        rand = [_lib.DeviceArray(c) for c in random_centres(nrand, L, 701)]
        w2 = _lib.DeviceArray(np.full(nrand, -n / nrand, dtype=np.float32))
        held += rand + [w2]
        name = f'D - R, lmax {lmax}'
        rows[name] = timed(lambda: last.__setitem__('t', P.triplet_multipoles(*data, L, edges, lmax, X2=rand[0], Y2=rand[1], Z2=rand[2],
                                                                            w2=w2)), a.reps, 'threepcf_walk')
        rows[name]['stats'] = P.last_stats()
        both = [_lib.DeviceArray(np.concatenate([d.get(), r.get()])) for d, r in zip(data, rand)]
        wb = _lib.DeviceArray(np.concatenate([np.ones(n, np.float32), w2.get()]))
        held += both + [wb]
        pair('D - R: weighted pair count', both, wb, name)
    for r in rows.values():
        k = r['kernels_ms_per_call'].get(r['kernel'])
        for what in ('candidates', 'counted'):
            r[what + '_per_s_kernel'] = None if not k else float(f"{r['stats'][what] / (k * 1e-3):.4g}")
    line = {'n': n, 'nrand': nrand, 'Lbox': L, 'bins': 10, 'rmax': 40.0, 'lmax': lmax, 'reps': a.reps, 'rows': rows}
    print(json.dumps(line))
    for d in held:
        d.free()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(line, indent=1) + '\n')


if __name__ == '__main__':
    main()
