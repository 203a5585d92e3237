#!/usr/bin/env python
"""Times the light-cone pair counter (pair_count_los) on one MI355X on the workload of a Landy-Szalay wp: galaxies and
randoms uniform in an octant shell, chi in [1500, 1800] Mpc/h around the observer, 13 logarithmic rp bins 0.1 - 30 Mpc/h,
pimax 30 in unit pi bins, weighted (wsum, no rsum) as the estimators call it.

    python scripts/pairs_los_probe.py [--ngal 1e6] [--nran 1e7] [--reps 2] [--out FILE.json] [--readme README.md]
    python scripts/pairs_los_probe.py --yardstick-only [--nran 1e7]       (runs on a commit without the light-cone counter)

DD, DR and RR: wall time per call (host clock around calls that end in a device synchronise; after one warm-up call of DD)
and the library's event time per kernel; candidate pairs per second = abacus_paircount_stats' candidates over the event
time of pair_count_los.  The yardstick is `pair_count_w` - the periodic weighted counter this kernel is modelled on - on a
periodic catalogue of --nran points at the randoms' number density, same bins and pimax.  Prints one JSON line; --out also
writes it to a file, --readme rewrites the block between the probe markers of that file."""
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

CHI = (1500.0, 1800.0)
SHELL_VOLUME = np.pi / 6 * (CHI[1] ** 3 - CHI[0] ** 3)      # an octant of the shell
BINS = np.geomspace(0.1, 30.0, 14).astype(np.float32)
PIMAX = 30


def octant_shell(n, seed):
    rng = np.random.default_rng(seed)
    u = np.abs(rng.normal(size=(n, 3)))
    u /= np.linalg.norm(u, axis=1)[:, None]
    r = np.cbrt(rng.uniform(CHI[0] ** 3, CHI[1] ** 3, n))
    p = (u * r[:, None]).astype(np.float32)
    return [np.ascontiguousarray(p[:, i]) for i in range(3)]


def stats():
    cand, ncxy, ncz, R = C.c_uint64(0), C.c_int(0), C.c_int(0), C.c_int(0)
    _lib.check(_lib.lib().abacus_paircount_stats(C.byref(cand), C.byref(ncxy), C.byref(ncz), C.byref(R)))
    return {'candidates': int(cand.value), 'cells_xy': ncxy.value, 'cells_z': ncz.value}


def timed(call, kernel, reps):
    walls, out = [], None
    _lib.profile_reset()
    _lib.profile_enable(True)
    for _ in range(reps):
        t = time.perf_counter()
        out = call()
        _lib.sync()
        walls.append((time.perf_counter() - t) * 1e3)
    _lib.profile_enable(False)
    kern = {k: round(ms / reps, 3) for k, (ms, cnt) in sorted(_lib.profile_get().items(), key=lambda kv: -kv[1][0]) if cnt}
    row = {'wall_ms_mean': round(float(np.mean(walls)), 2), 'wall_ms_min': round(min(walls), 2), 'kernels_ms_per_call': kern,
           'counted_pairs': int(out[0].sum()), **stats()}
    row['kernel_ms'] = kern.get(kernel, 0.0)
    row['candidates_per_s'] = round(row['candidates'] / (row['kernel_ms'] * 1e-3), 0) if row['kernel_ms'] else None
    return row


def yardstick(n, reps):
    """pair_count_w: weighted periodic DDrppi autocorrelation at the randoms' number density"""
    L = float(np.cbrt(SHELL_VOLUME))                 # n points in L^3: the density of n points in the shell
    rng = np.random.default_rng(501)
    dev = [_lib.DeviceArray(rng.random(n, dtype=np.float32) * np.float32(L)) for _ in range(3)]
    w = _lib.DeviceArray((0.5 + rng.random(n)).astype(np.float32))
    call = lambda: T._paircount_weighted(1, *dev, L, BINS, W1=w, pimax=float(PIMAX), npibins=PIMAX, want_rsum=False)   # noqa: E731
    call()
    row = timed(call, 'pair_count_w', reps)
    row['Lbox'] = round(L, 2)
    for d in dev + [w]:
        d.free()
    return row


def render(line):
    rows = ['| term | points | wall ms | pair_count_los ms | sort + centring ms | candidates | candidates / s | counted pairs |', '|---|---|---|---|---|---|---|---|']
    for k in ('DD', 'DR', 'RR'):
        r = line['rows'][k]
        other = sum(v for name, v in r['kernels_ms_per_call'].items() if name != 'pair_count_los')
        rows.append(f"| {k} | {r['points']} | {r['wall_ms_mean']} | {r['kernel_ms']} | {other:.2f} | {r['candidates']:.4g} | "
                    f"{r['candidates_per_s']:.3g} | {r['counted_pairs']:.4g} |")
    y = line['yardstick']
    rows.append(f"| pair_count_w, periodic L = {y['Lbox']} | {line['nran']} | {y['wall_ms_mean']} | {y['kernel_ms']} (pair_count_w) | | "
                f"{y['candidates']:.4g} | {y['candidates_per_s']:.3g} | {y['counted_pairs']:.4g} |")
    rows.append('')
    rows.append(f"Randoms per galaxy: {line['nran'] / line['ngal']:.3g}.  Candidate rate of `pair_count_los` (RR) over `pair_count_w` "
                f"of this build: **{line['ratio_rr_to_yardstick']}**.")
    return '\n'.join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ngal', default='1e6')
    ap.add_argument('--nran', default='1e7')
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--yardstick-only', action='store_true')
    ap.add_argument('--out', default=None)
    ap.add_argument('--readme', default=None)
    a = ap.parse_args()
    ng, nr = int(float(a.ngal)), int(float(a.nran))
    print('device:', _lib.device_name(), file=sys.stderr)
    line = {'ngal': ng, 'nran': nr, 'chi': CHI, 'bins': 13, 'pimax': PIMAX, 'reps': a.reps, 'yardstick': yardstick(nr, a.reps)}
    if not a.yardstick_only:
        gal = [_lib.DeviceArray(c) for c in octant_shell(ng, 601)]
        ran = [_lib.DeviceArray(c) for c in octant_shell(nr, 602)]
        rng = np.random.default_rng(603)
        wg, wr = (_lib.DeviceArray((0.5 + rng.random(n)).astype(np.float32)) for n in (ng, nr))
        kw = dict(pimax=float(PIMAX), npibins=PIMAX, want_rsum=False)
        terms = {'DD': (lambda: T._paircount_los(1, *gal, BINS, W1=wg, **kw), f'{ng}'),
                 'DR': (lambda: T._paircount_los(1, *gal, BINS, *ran, W1=wg, W2=wr, **kw), f'{ng} x {nr}'),
                 'RR': (lambda: T._paircount_los(1, *ran, BINS, W1=wr, **kw), f'{nr}')}
        terms['DD'][0]()                      # warm-up: code objects, buffers
        line['rows'] = {}
        for k, (call, pts) in terms.items():
            line['rows'][k] = dict(timed(call, 'pair_count_los', a.reps), points=pts)
            print(k, json.dumps(line['rows'][k]), file=sys.stderr, flush=True)
        line['ratio_rr_to_yardstick'] = round(line['rows']['RR']['candidates_per_s'] / line['yardstick']['candidates_per_s'], 3)
        for d in gal + ran + [wg, wr]:
            d.free()
    print(json.dumps(line))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(line, indent=1) + '\n')
    if a.readme and 'rows' in line:
        path = Path(a.readme)
        text = path.read_text()
        begin, end = '<!-- probe:begin -->', '<!-- probe:end -->'
        i, j = text.index(begin) + len(begin), text.index(end)
        path.write_text(text[:i] + '\n' + render(line) + '\n' + text[j:])


if __name__ == '__main__':
    main()
