#!/usr/bin/env python
"""Times the projected mass sums behind Delta Sigma on one MI355X against the parent's nearest route.

    python scripts/lensing_probe.py [--n 1e7] [--ng 1e6] [--reps 5] [--out FILE.json]

Workload: `n` uniform particles and `ng` uniform galaxies in a 2 Gpc/h box, 20 logarithmic bins 0.1 - 30 Mpc/h, projected along
z; all columns resident in HBM (float32 DeviceArray).  Rows:
  handle build               `ProjectedParticles` from the resident particle columns, with and without masses (wall time of the
                             call, synchronised, and the library's event time per kernel);
  projected_sums             the per-evaluation call from resident galaxy columns: unit masses and weights, masses and weights,
                             and the same two with the comparator reduction `lens_shared_rows`;
  weighted DDrppi cross      `_paircount_weighted` mode 1 of the galaxies against the particles with pimax = L / 2 and one pi
                             bin, on the same x, y and a z column in [0, 0.2 L): the route to the bins before this module.  It cannot deliver
                             the inner disc, re-sorts the particles in every call, reads z and tests |dz|.
Per row: HIP-event time of the whole call on the library stream (one warm-up, then the mean, smallest and largest of `reps`
calls; a call ends with its copies to the host), the library's event time per kernel from `reps` further calls, the candidate
pairs from abacus_lens_stats / abacus_paircount_stats and candidates per second of the walking kernel.  The two routes are
checked against each other: the counts of the bins are equal.  Prints one JSON line; --out also writes it to a file."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from abacusutils_amd import _lib  # noqa: E402
from abacusutils_amd.analysis import lensing as S  # noqa: E402
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


def pair_stats():
    cand, ncxy, ncz = C.c_uint64(0), C.c_int(0), C.c_int(0)
    _lib.check(_lib.lib().abacus_paircount_stats(C.byref(cand), C.byref(ncxy), C.byref(ncz), None))
    return {'candidates': int(cand.value), 'cells_xy': ncxy.value, 'cells_z': ncz.value}


def lens_stats():
    cand, nc = S.walk_stats()
    return {'candidates': cand, 'cells_xy': nc, 'cells_z': 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', default='1e7')
    ap.add_argument('--ng', default='1e6')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-baseline', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    n, ng, L = int(float(a.n)), int(float(a.ng)), 2000.0
    print('device:', _lib.device_name(), file=sys.stderr)
    rng = np.random.default_rng(700)
    # z in [0, 0.2 L): the pair counter drops a pair at exactly |dz| = L / 2 = pimax, which float32 columns over the whole box do
    # contain at this size; its grid has one cell in z either way, so its work is the same
    depth = (L, L, 0.2 * L)
    part = [_lib.DeviceArray(rng.random(n, dtype=np.float32) * np.float32(d)) for d in depth]
    gal = [_lib.DeviceArray(rng.random(ng, dtype=np.float32) * np.float32(d)) for d in depth]
    pm = _lib.DeviceArray((0.5 + rng.random(n, dtype=np.float32)).astype(np.float32))
    gw = _lib.DeviceArray((0.5 + rng.random(ng, dtype=np.float32)).astype(np.float32))
    edges = np.geomspace(0.1, 30.0, 21).astype(np.float32)
    rows, last = {}, {}
    handles = {}
    for name, mass in (('handle build, unit masses', None), ('handle build, masses', pm)):
        wall = []
        for _ in range(1 + a.reps):          # the first is the warm-up
            _lib.sync()
            t0 = time.perf_counter()
            h = S.ProjectedParticles(part[0], part[1], L, 30.0, mass=mass)
            wall.append((time.perf_counter() - t0) * 1e3)
            h.free()
        _lib.profile_reset()
        _lib.profile_enable(True)
        handles[name] = S.ProjectedParticles(part[0], part[1], L, 30.0, mass=mass)
        _lib.sync()
        _lib.profile_enable(False)
        rows[name] = {'wall_ms_mean': round(float(np.mean(wall[1:])), 3), 'wall_ms_min': round(min(wall[1:]), 3),
                      'wall_ms_max': round(max(wall[1:]), 3),
                      'kernels_ms': {k: round(v, 3) for k, (v, cnt) in sorted(_lib.profile_get().items(), key=lambda kv: -kv[1][0]) if cnt}}
    unit, massive = handles['handle build, unit masses'], handles['handle build, masses']
    for shared in (0, 1):
        _lib.set_option('lens_shared_rows', shared)
        tag = ', shared rows (comparator)' if shared else ''
        for name, h, w in (('projected_sums, unit masses and weights', unit, None), ('projected_sums, masses and weights', massive, gw)):
            rows[name + tag] = timed(lambda: last.__setitem__(name, S.projected_sums(h, gal[0], gal[1], edges, weights=w)), a.reps, 'lens_walk')
            rows[name + tag]['stats'] = lens_stats()
            rows[name + tag]['counted_pairs'] = int(last[name]['npairs'].sum())
    _lib.set_option('lens_shared_rows', 0)
    if not a.no_baseline:
        kw = dict(pimax=L / 2, npibins=1, want_rsum=False)
        for name, w1, w2 in (('weighted DDrppi cross, unit weights', None, None), ('weighted DDrppi cross, weights', gw, pm)):
            rows[name] = timed(lambda: last.__setitem__('w', T._paircount_weighted(1, *gal, L, edges, *part, W1=w1, W2=w2, **kw)), a.reps, 'pair_count_w')
            rows[name]['stats'] = pair_stats()
            rows[name]['counted_pairs'] = int(last['w'][0].sum())
        agree = True
        for name in ('projected_sums, unit masses and weights', 'projected_sums, masses and weights'):
            agree = agree and np.array_equal(last[name]['npairs'][1:], last['w'][0])
        rows['weighted DDrppi cross, weights']['counts_equal_to_projected_sums'] = bool(agree)
        if not agree:
            rows['weighted DDrppi cross, weights']['npairs'] = [int(v) for v in last['w'][0]]
            rows['projected_sums, masses and weights']['npairs'] = [int(v) for v in last['projected_sums, masses and weights']['npairs']]
        ref, got = last['w'][1], last['projected_sums, masses and weights']['wsum'][1:]
        rows['weighted DDrppi cross, weights']['max_rel_diff_of_the_sums'] = float(np.abs(got / ref - 1).max())
    for r in rows.values():
        if 'kernel' in r:
            k = r['kernels_ms_per_call'].get(r['kernel'])
            r['candidates_per_s_kernel'] = None if not k else float(f"{r['stats']['candidates'] / (k * 1e-3):.4g}")
    line = {'n': n, 'ng': ng, 'Lbox': L, 'bins': 20, 'reps': a.reps, 'rows': rows}
    print(json.dumps(line))
    unit.free(), massive.free()
    for d in part + gal + [pm, gw]:
        d.free()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(line, indent=1) + '\n')
    if not a.no_baseline and not agree:
        sys.exit('the two routes disagree')


if __name__ == '__main__':
    main()
