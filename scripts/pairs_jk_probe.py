#!/usr/bin/env python
"""Times the jackknife pair counters (pair_count_jk, pair_count_los_jk) beside their parents (pair_count_w, pair_count_los)
on one MI355X, on the SAME catalogue and bins.

    python scripts/pairs_jk_probe.py [--n 1e7] [--ngal 1e6] [--nran 0] [--reps 5] [--no-events] [--out FILE.json]

Box: --n uniform points in a 2 Gpc/h box, 13 logarithmic bins 0.1 - 30 Mpc/h (scripts/pairs_weighted_probe.py), the three
modes (pi_max 30 in unit bins; 20 mu bins), coordinates, weights and labels in HBM, labels of a 5^3 split of the box
(`box_regions`); the worst-case label map - random labels, every cell slice in up to 125 runs - once, mode r.
Light cone: --ngal points of the octant shell of scripts/pairs_los_probe.py (DD of its Landy-Szalay wp: (rp, pi), weighted),
125 labels of 5 x 5 sky patches by 5 radial shells; --nran > 0 adds the RR of that many randoms.
Per row: wall time per call (host clock around calls that end in a device synchronise; median of `reps` calls after a
warm-up) and the library's event time per kernel (median is not available from the event sums: the mean of `reps` further
calls); candidates from abacus_paircount_stats, flushes and workgroups from abacus_paircount_jk_stats.  --no-events leaves
the library's events off (for a run under an external profiler).  Prints one JSON line; --out also writes it to a file."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from abacusutils_amd import _lib  # noqa: E402
from abacusutils_amd.analysis import jackknife as J  # noqa: E402
from abacusutils_amd.analysis import tpcf_corrfunc as T  # noqa: E402

BINS = np.geomspace(0.1, 30.0, 14).astype(np.float32)
SUB = {0: {}, 1: dict(pimax=30.0, npibins=30), 2: dict(mu_max=1.0, nmubins=20)}
FULL = dict(pimax=0.0, npibins=0, mu_max=1.0, nmubins=0)
SORT_KERNELS = ('pair_cell_count', 'pair_cell_sort', 'pair_cell_fill', 'pair_cell_starts', 'pair_jk_keys', 'pair_jk_sort',
                'pair_jk_fill', 'pair_jk_starts', 'pair_jk_label_range')


def timed(call, kernel, reps, events):
    call()                                   # warm-up: code objects, buffers
    _lib.sync()
    walls = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        _lib.sync()
        walls.append((time.perf_counter() - t) * 1e3)
    row = {'wall_ms_median': round(float(np.median(walls)), 3), 'wall_ms_min': round(min(walls), 3), 'wall_ms_max': round(max(walls), 3)}
    if events:
        _lib.profile_reset()
        _lib.profile_enable(True)
        for _ in range(reps):
            call()
        _lib.sync()
        _lib.profile_enable(False)
        kern = {k: round(ms / reps, 3) for k, (ms, cnt) in sorted(_lib.profile_get().items(), key=lambda kv: -kv[1][0]) if cnt}
        row.update(kernels_ms_per_call=kern, kernel_ms=kern.get(kernel, 0.0),
                   sort_ms=round(sum(v for k, v in kern.items() if k in SORT_KERNELS), 3))
    cand, fl, wg = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
    _lib.check(_lib.lib().abacus_paircount_stats(C.byref(cand), None, None, None))
    row['candidates'] = int(cand.value)
    if kernel.endswith('_jk'):
        _lib.check(_lib.lib().abacus_paircount_jk_stats(C.byref(fl), C.byref(wg)))
        row.update(flushes=int(fl.value), workgroups=wg.value, flushes_per_workgroup=round(fl.value / max(wg.value, 1), 1))
    return row


def octant_labels(cols, chi):
    """5 x 5 sky patches by 5 radial shells of the octant: 125 labels"""
    x, y, z = (np.asarray(c, np.float64) for c in cols)
    r = np.sqrt(x * x + y * y + z * z)
    a = np.clip((np.arctan2(y, x) / (np.pi / 2) * 5).astype(np.int32), 0, 4)
    b = np.clip((z / r * 5).astype(np.int32), 0, 4)
    c = np.clip(((r ** 3 - chi[0] ** 3) / (chi[1] ** 3 - chi[0] ** 3) * 5).astype(np.int32), 0, 4)
    return ((a * 5 + b) * 5 + c).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', default='1e7')
    ap.add_argument('--ngal', default='1e6')
    ap.add_argument('--nran', default='0')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-events', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    n, ng, nr, ev = int(float(a.n)), int(float(a.ngal)), int(float(a.nran)), not a.no_events
    print('device:', _lib.device_name(), file=sys.stderr)
    line = {'n': n, 'ngal': ng, 'nran': nr, 'reps': a.reps, 'nreg': 125, 'rows': {}}
    rows = line['rows']
    if n:
        L = 2000.0
        rng = np.random.default_rng(500)
        dev = [_lib.DeviceArray(rng.random(n, dtype=np.float32) * np.float32(L)) for _ in range(3)]
        w = _lib.DeviceArray((0.5 + rng.random(n)).astype(np.float32))
        t = time.perf_counter()
        lab = J.box_regions(*dev, L, 5)
        _lib.sync()
        line['box_regions_ms'] = round((time.perf_counter() - t) * 1e3, 3)
        rand = _lib.DeviceArray(rng.integers(0, 125, n).astype(np.int32))
        for mode, name in ((0, 'r'), (1, 'rppi'), (2, 'smu')):
            kw = dict(FULL, **SUB[mode])
            out = {}
            rows[f'box {name}: pair_count_w'] = timed(lambda: out.__setitem__('w', T._paircount_weighted(mode, *dev, L, BINS, W1=w, want_rsum=False, **SUB[mode])),
                                                      'pair_count_w', a.reps, ev)
            rows[f'box {name}: pair_count_jk, 5^3 sub-boxes'] = timed(
                lambda: out.__setitem__('j', J._jk_counter('paircount_jk', mode, BINS, (*dev, None, None, None), (w, None), (lab, None), 125, (C.c_float(L),), **kw)),
                'pair_count_jk', a.reps, ev)
            assert np.array_equal(out['j'][0].sum(axis=0, dtype=np.uint64), out['w'][0])
            if mode == 0:
                rows['box r: pair_count_jk, random labels (worst case)'] = timed(
                    lambda: J._jk_counter('paircount_jk', mode, BINS, (*dev, None, None, None), (w, None), (rand, None), 125, (C.c_float(L),), **kw),
                    'pair_count_jk', a.reps, ev)
            print(name, file=sys.stderr, flush=True)
        for d in dev + [w, lab, rand]:
            d.free()
    from pairs_los_probe import CHI, octant_shell
    for label, npts, seed in (('DD', ng, 601), ('RR', nr, 602)):
        if not npts:
            continue
        host = octant_shell(npts, seed)
        cols = [_lib.DeviceArray(c) for c in host]
        lab = _lib.DeviceArray(octant_labels(host, CHI))
        w = _lib.DeviceArray((0.5 + np.random.default_rng(603).random(npts)).astype(np.float32))
        zero = np.zeros(3)
        kw = dict(FULL, **SUB[1])
        out = {}
        reps = a.reps if label == 'DD' else 2
        rows[f'light cone {label} rppi: pair_count_los'] = timed(lambda: out.__setitem__('w', T._paircount_los(1, *cols, BINS, W1=w, want_rsum=False, **SUB[1])),
                                                                 'pair_count_los', reps, ev)
        rows[f'light cone {label} rppi: pair_count_los_jk, 125 patches'] = timed(
            lambda: out.__setitem__('j', J._jk_counter('paircount_los_jk', 1, BINS, (*cols, None, None, None), (w, None), (lab, None), 125, (J.ptr(zero),), **kw)),
            'pair_count_los_jk', reps, ev)
        assert np.array_equal(out['j'][0].sum(axis=0, dtype=np.uint64), out['w'][0])
        rows[f'light cone {label} rppi: pair_count_los_jk, unweighted'] = timed(
            lambda: J._jk_counter('paircount_los_jk', 1, BINS, (*cols, None, None, None), (None, None), (lab, None), 125, (J.ptr(zero),), want_sums=False, **kw),
            'pair_count_los_jk', reps, ev)
        for d in cols + [lab, w]:
            d.free()
        print(label, file=sys.stderr, flush=True)
    print(json.dumps(line))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(line, indent=1) + '\n')


if __name__ == '__main__':
    main()
