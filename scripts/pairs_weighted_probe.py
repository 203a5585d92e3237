#!/usr/bin/env python
"""Times the weighted pair counter against the unweighted one on one MI355X, on the catalogue and bins of
bench_pk.bench_pairs (DD(r) of 10^7 uniform points, 13 logarithmic bins 0.1 - 30 Mpc/h, 2 Gpc/h box).

    python scripts/pairs_weighted_probe.py [--n 1e7] [--reps 5] [--out FILE.json]

Per variant - `_paircount`, `_paircount_weighted` with and without rsum - and per residence of the coordinates (host
arrays / DeviceArray columns; the weights live where the coordinates live): wall time per call (host clock around calls
that end in a device synchronise; the mean, the smallest and the largest of `reps` calls after a warm-up) and the library's
event time per kernel, from `reps` further calls.  Candidates per counted pair come from abacus_paircount_stats.  On a
library without the weighted entry points (an older commit) only the unweighted rows are timed.  Prints one JSON line;
--out also writes it to a file."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from abacusutils_amd import _lib  # noqa: E402
from abacusutils_amd.analysis import tpcf_corrfunc as T  # noqa: E402


def timed(call, reps):
    call()                                   # warm-up: code objects, scratch buffers
    _lib.sync()
    walls = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        _lib.sync()
        walls.append((time.perf_counter() - t) * 1e3)
    _lib.profile_reset()
    _lib.profile_enable(True)
    for _ in range(reps):
        call()
    _lib.sync()
    _lib.profile_enable(False)
    kern = {k: round(ms / reps, 3) for k, (ms, cnt) in sorted(_lib.profile_get().items(), key=lambda kv: -kv[1][0]) if cnt}
    return {'wall_ms_mean': round(float(np.mean(walls)), 3), 'wall_ms_min': round(min(walls), 3),
            'wall_ms_max': round(max(walls), 3), 'kernels_ms_per_call': kern}


def stats():
    cand, ncxy, ncz, R = C.c_uint64(0), C.c_int(0), C.c_int(0), C.c_int(0)
    _lib.check(_lib.lib().abacus_paircount_stats(C.byref(cand), C.byref(ncxy), C.byref(ncz), C.byref(R)))
    return {'candidates': int(cand.value), 'cells_xy': ncxy.value, 'cells_z': ncz.value, 'stencil_R': R.value}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', default='1e7')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    n, L = int(float(a.n)), 2000.0
    print('device:', _lib.device_name(), file=sys.stderr)
    rng = np.random.default_rng(500)
    p = rng.random((n, 3), dtype=np.float32) * np.float32(L)
    host = [np.ascontiguousarray(p[:, i]) for i in range(3)]
    w_host = (0.5 + rng.random(n)).astype(np.float32)
    bins = np.geomspace(0.1, 30.0, 14).astype(np.float32)
    dev = [_lib.DeviceArray(c) for c in host]
    w_dev = _lib.DeviceArray(w_host)
    weighted = hasattr(T, '_paircount_weighted')
    rows, counts = {}, {}
    for where, cols, w in (('host', host, w_host), ('device', dev, w_dev)):
        rows[f'unweighted, {where}'] = timed(lambda: counts.__setitem__('n', T._paircount(0, *cols, L, bins)), a.reps)
        rows[f'unweighted, {where}']['stats'] = stats()
        if not weighted:
            continue
        for rs in (True, False):
            name = f'weighted, rsum {"on" if rs else "off"}, {where}'
            rows[name] = timed(lambda: counts.__setitem__('w', T._paircount_weighted(0, *cols, L, bins, W1=w, want_rsum=rs)), a.reps)
            rows[name]['stats'] = stats()
            assert np.array_equal(counts['w'][0], counts['n'])
    pairs = int(counts['n'].sum())
    line = {'n': n, 'Lbox': L, 'bins': 13, 'reps': a.reps, 'weighted_entry_points': weighted, 'counted_pairs': pairs, 'rows': rows}
    for r in rows.values():
        r['candidates_per_counted_pair'] = round(r['stats']['candidates'] / pairs, 2)
    if weighted:
        for where in ('host', 'device'):
            u = rows[f'unweighted, {where}']['wall_ms_mean']
            line[f'ratio_rsum_on_{where}'] = round(rows[f'weighted, rsum on, {where}']['wall_ms_mean'] / u, 2)
            line[f'ratio_rsum_off_{where}'] = round(rows[f'weighted, rsum off, {where}']['wall_ms_mean'] / u, 2)
    print(json.dumps(line))
    for d in dev + [w_dev]:
        d.free()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(line, indent=1) + '\n')


if __name__ == '__main__':
    main()
