#!/usr/bin/env python
"""Times the bispectrum (abacusutils_amd.analysis.bispectrum) on one MI355X and measures how far its triangle counts are from integers.

    python scripts/bispectrum_probe.py [--out FILE.json] [--steps copy,n256,n512,counts64]
    python scripts/bispectrum_probe.py --step n512          # one step, in this process

Without --step every step runs in a process of its own under `timeout -k 10 <seconds>`, one after the other, and the first one that
fails ends the run (the steps are chained as with &&): nothing is started on a device after a step has faulted or hung on it.

Steps:
  copy      the device-to-device copy rate of a 1 GiB buffer (bytes read + written per second): the yardstick of the streaming kernels.
  n256/n512 1e6 / 8e6 uniform points in a 2 Gpc/h box, TSC, compensated, interlaced, 16 linear shells from 0.5 dk to n / 3 dk:
            the whole `calc_bispectrum` call, first (the triangle counts are built) and repeated (they are cached), HIP-event times; the
            library's event time per kernel; bk_triple as a fraction of the f32 MFMA peak (157.3 TFLOP/s; 2 * 16^3 FLOP per cell for the
            full (i, j, l) cube) and of the copy rate; bk_shell_mask as a fraction of the copy rate (8 + 8 * 16 bytes per mode); the
            largest distance of N_tri from an integer.
  counts64  n = 64, 16 shells: N of the device against the float64 NumPy count of tests/bispectrum_statement.py.
Prints one JSON line per step; --out writes the merged result of a whole run."""
import argparse
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

LIMITS = {'copy': 120, 'n256': 240, 'n512': 420, 'counts64': 180}
MFMA_PEAK = 157.3e12
LBOX = 2000.0
NB = 16


def edges(n):
    return np.linspace(0.5, n / 3, NB + 1) * 2.0 * np.pi / LBOX


def step_copy():
    from abacusutils_amd import _lib
    nbytes = 1 << 30
    a, b = (_lib.DeviceArray(nbytes=nbytes, dtype=np.uint8, shape=(nbytes,)) for _ in range(2))
    import ctypes as C
    copy = lambda: _lib.check(_lib.lib().abacus_memcpy_d2d(b.ptr, a.ptr, C.c_uint64(nbytes)))   # noqa: E731
    copy()
    _lib.sync()
    ms = []
    for _ in range(10):
        t0, t1 = _lib.Event(), _lib.Event()
        t0.record()
        copy()
        t1.record()
        _lib.sync()
        ms.append(t1.elapsed_ms_since(t0))
    a.free()
    b.free()
    return {'copy_GBps_read_plus_write': round(2 * nbytes / (min(ms) * 1e-3) / 1e9, 1), 'ms_min': round(min(ms), 3)}


def step_mesh(n, npts, copy_GBps):
    from abacusutils_amd import _lib
    from abacusutils_amd.analysis import bispectrum as bk
    pos = np.random.default_rng(1).random((npts, 3), dtype=np.float32) * np.float32(LBOX)
    dev = _lib.DeviceArray(pos)
    ke = edges(n)
    call = lambda: bk.calc_bispectrum(dev, LBOX, ke, nmesh=n)   # noqa: E731

    def timed():
        t0, t1 = _lib.Event(), _lib.Event()
        t0.record()
        out = call()
        t1.record()
        _lib.sync()
        return out, t1.elapsed_ms_since(t0)

    _, first = timed()                        # builds the counts, the plans and the host's k_mean
    reps = 3
    out, ms = None, []
    for _ in range(reps):
        out, t = timed()
        ms.append(t)
    bk._counts.clear()
    _lib.profile_reset()
    _lib.profile_enable(True)
    call()                                    # with the I fields: shells and sums run twice
    _lib.sync()
    _lib.profile_enable(False)
    prof = _lib.profile_get()
    kern = {k: {'ms_per_launch': round(v / cnt, 3), 'launches': int(cnt)} for k, (v, cnt) in sorted(prof.items(), key=lambda kv: -kv[1][0]) if cnt}
    dev.free()
    pitch = (n + 2 + 31) // 32 * 32
    res = {'n': n, 'npts': npts, 'shells': NB, 'first_call_ms': round(first, 2), 'cached_call_ms': [round(t, 2) for t in ms], 'kernels': kern,
           'ntri': int(len(out['B'])), 'N_tri_max': float(out['N_tri'].max()),
           'N_tri_max_distance_from_integer': float(np.abs(out['N_tri'] - np.rint(out['N_tri'])).max()),
           'N_tri_max_relative_distance': float((np.abs(out['N_tri'] - np.rint(out['N_tri'])) / out['N_tri']).max())}
    if 'bk_triple' in kern:
        t = kern['bk_triple']['ms_per_launch'] * 1e-3
        res['bk_triple_TFLOPs'] = round(2.0 * NB**3 * n**3 / t / 1e12, 2)
        res['bk_triple_fraction_of_mfma_peak'] = round(2.0 * NB**3 * n**3 / t / MFMA_PEAK, 3)
        res['bk_triple_read_GBps'] = round(NB * 4.0 * n * n * pitch / t / 1e9, 1)
    if 'bk_shell_mask' in kern:
        t = kern['bk_shell_mask']['ms_per_launch'] * 1e-3
        res['bk_shell_mask_GBps'] = round((8.0 + 8.0 * NB) * n * n * (n // 2 + 1) / t / 1e9, 1)
    if copy_GBps:
        for k in ('bk_triple_read_GBps', 'bk_shell_mask_GBps'):
            if k in res:
                res[k.replace('GBps', 'fraction_of_copy_rate')] = round(res[k] / copy_GBps, 3)
    return res


def step_counts64():
    sys.path.insert(0, str(ROOT / 'tests'))
    import bispectrum_statement as st
    from abacusutils_amd.analysis import bispectrum as bk
    n = 64
    ke = edges(n)
    c = bk.triangle_counts(n, LBOX, ke)
    T, _ = st.sums(st.shell_fields(None, n, LBOX, ke))
    N64 = T / float(n) ** 3
    ok = N64 > 0.5
    return {'n': n, 'shells': NB, 'N_max': float(N64.max()), 'max_abs_distance': float(np.abs(c['N'] - N64).max()),
            'max_relative_distance': float((np.abs(c['N'] - N64)[ok] / N64[ok]).max()),
            'float64_count_distance_from_integer': float(np.abs(N64 - np.rint(N64)).max())}


def run_step(name, copy_GBps):
    if name == 'copy':
        return step_copy()
    if name == 'n256':
        return step_mesh(256, 1000000, copy_GBps)
    if name == 'n512':
        return step_mesh(512, 8000000, copy_GBps)
    if name == 'counts64':
        return step_counts64()
    raise SystemExit(f'unknown step {name}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--step')
    ap.add_argument('--steps', default='copy,n256,n512,counts64')
    ap.add_argument('--copy-GBps', type=float, default=0.0)
    ap.add_argument('--out')
    a = ap.parse_args()
    if a.step:
        print(json.dumps({a.step: run_step(a.step, a.copy_GBps)}))
        return 0
    merged, copy_GBps = {}, a.copy_GBps
    for name in a.steps.split(','):
        cmd = ['timeout', '-k', '10', str(LIMITS[name]), sys.executable, str(Path(__file__).resolve()), '--step', name, '--copy-GBps', str(copy_GBps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:                 # a failure, a fault or a time limit: nothing more is started
            print(json.dumps({'failed_step': name, 'returncode': r.returncode, 'done': merged}))
            return r.returncode
        merged.update(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps({name: merged[name]}), flush=True)
        if name == 'copy':
            copy_GBps = merged['copy']['copy_GBps_read_plus_write']
    if a.out:
        Path(a.out).write_text(json.dumps(merged, indent=1) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
