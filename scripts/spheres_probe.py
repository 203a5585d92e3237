#!/usr/bin/env python
"""Times the counts in spheres on one MI355X against the weighted cross count of the same two sets.

    python scripts/spheres_probe.py [--n 1e7] [--nq 1e6] [--reps 5] [--out FILE.json]

Workload: `n` uniform data points and `nq` random centres (`spheres.random_centres`) in a 2 Gpc/h box, 16 logarithmic radii
1 - 30 Mpc/h, kmax = 8; spheres and cylinders (pimax = 30); `return_counts` off and on; all columns resident in HBM (float32
DeviceArray).  The yardstick is `_paircount_weighted` (mode 0, and mode 1 with one pi bin of 30 for the cylinders) of the
centres against the data with the edges (0, *radii): it walks the same 27-cell grid and does more per counted pair.  Last, the
dense regime: the data as their own queries (spheres, counts off) beside the weighted autocorrelation.

Per row: HIP-event time of the whole call on the library stream (one warm-up, then the mean, smallest and largest of `reps`
calls; a call ends with its copies to the host, so the time includes them), the library's event time per kernel from `reps`
further calls, the candidate pairs from abacus_spherecount_stats / abacus_paircount_stats, and candidates per second of the
counting kernel.  The two counters are checked against each other: the column sums of `counts` are the cumulative pair
counts.  Prints one JSON line; --out also writes it to a file."""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from abacusutils_amd import _lib  # noqa: E402
from abacusutils_amd.analysis import spheres as S  # noqa: E402
from abacusutils_amd.analysis import tpcf_corrfunc as T  # noqa: E402


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


def stats(entry):
    cand, ncxy, ncz = C.c_uint64(0), C.c_int(0), C.c_int(0)
    extra = () if entry == 'abacus_spherecount_stats' else (None,)
    _lib.check(getattr(_lib.lib(), entry)(C.byref(cand), C.byref(ncxy), C.byref(ncz), *extra))
    return {'candidates': int(cand.value), 'cells_xy': ncxy.value, 'cells_z': ncz.value}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', default='1e7')
    ap.add_argument('--nq', default='1e6')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    n, nq, L, kmax = int(float(a.n)), int(float(a.nq)), 2000.0, 8
    print('device:', _lib.device_name(), file=sys.stderr)
    p = np.random.default_rng(500).random((n, 3), dtype=np.float32) * np.float32(L)
    data = [_lib.DeviceArray(np.ascontiguousarray(p[:, i])) for i in range(3)]
    queries = [_lib.DeviceArray(c) for c in S.random_centres(nq, L, 501)]
    radii = np.geomspace(1.0, 30.0, 16).astype(np.float32)
    edges = np.concatenate([[0.0], radii]).astype(np.float32)
    rows, last = {}, {}
    for shape, pimax in (('spheres', None), ('cylinders', 30.0)):
        for want in (False, True):
            name = f'{shape}, counts {"on" if want else "off"}'
            rows[name] = timed(lambda: last.__setitem__('s', S.count_in_spheres(*data, L, radii, *queries, pimax=pimax, kmax=kmax,
                                                                                 return_counts=want)), a.reps, 'sphere_count')
            rows[name]['stats'] = stats('abacus_spherecount_stats')
        kw = dict(pimax=pimax, npibins=1) if pimax else {}
        name = f'{shape}: weighted cross count'
        rows[name] = timed(lambda: last.__setitem__('w', T._paircount_weighted(1 if pimax else 0, *queries, L, edges, *data,
                                                                                want_rsum=False, **kw)), a.reps, 'pair_count_w')
        rows[name]['stats'] = stats('abacus_paircount_stats')
        cum = np.cumsum(last['w'][0])
        assert np.array_equal(last['s']['counts'].sum(axis=0, dtype=np.uint64), cum), 'the two counters disagree'
        assert np.all(last['s']['hist'].sum(axis=1) == nq)
        rows[name]['counted_pairs'] = int(cum[-1])
    # the dense regime: the data as their own queries (the transposed mapping's ground; counts off: 640 MB of rows otherwise)
    rows['spheres, data as queries'] = timed(lambda: last.__setitem__('s', S.count_in_spheres(*data, L, radii, kmax=kmax)), a.reps, 'sphere_count')
    rows['spheres, data as queries']['stats'] = stats('abacus_spherecount_stats')
    assert np.all(last['s']['hist'].sum(axis=1) == n)
    rows['spheres, data as queries: weighted autocorrelation'] = timed(
        lambda: last.__setitem__('w', T._paircount_weighted(0, *data, L, edges, want_rsum=False)), a.reps, 'pair_count_w')
    rows['spheres, data as queries: weighted autocorrelation']['stats'] = stats('abacus_paircount_stats')
    rows['spheres, data as queries: weighted autocorrelation']['counted_pairs'] = int(last['w'][0].sum())
    for r in rows.values():
        k = r['kernels_ms_per_call'].get(r['kernel'])
        r['candidates_per_s_kernel'] = None if not k else float(f"{r['stats']['candidates'] / (k * 1e-3):.4g}")
    line = {'n': n, 'nq': nq, 'Lbox': L, 'radii': 16, 'kmax': kmax, 'reps': a.reps, 'rows': rows}
    print(json.dumps(line))
    for d in data + queries:
        d.free()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(line, indent=1) + '\n')


if __name__ == '__main__':
    main()
