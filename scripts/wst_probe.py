#!/usr/bin/env python
"""Times the wavelet scattering transform (abacusutils_amd.analysis.wst) on one MI355X against the copy rate of the same run.

    python scripts/wst_probe.py [--out FILE.json] [--steps copy256,chain256q1,chain256q4,first256q1]
    python scripts/wst_probe.py --step chain256q1          # one step, in this process

Without --step every step runs in a process of its own under `timeout -k 10 <seconds>`, one after the other, and the first one that
fails ends the run (the steps are chained as with &&): nothing is started on a device after a step has faulted or hung on it.

Steps:
  copy256     the device-to-device copy of one padded 256^3 mesh (abacus_memcpy_d2d), HIP-event time over 20 copies: the copy rate
              (bytes read + bytes written over time) the streaming kernels are held against.
  chain256qK  the whole `calc_wst` call at 1e7 uniform particles resident in HBM, 256^3, TSC, compensated, interlaced, J = 4, L = 4,
              K exponents: first call (plans) and repeated, then the library's event time per kernel of one more call, the share of
              the transforms, and wst_mult / wst_accum / wst_moments as bytes over time against the copy rate measured in this step.
  first256q1  the same with second_order=False.
Prints one JSON line per step; --out writes the merged result of a whole run."""
import argparse
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

LIMITS = {'copy256': 120, 'chain256q1': 300, 'chain256q4': 300, 'first256q1': 300}
LBOX = 2000.0
NPTS = 10_000_000
J, L = 4, 4
EXPONENTS = {1: (0.8,), 4: (0.5, 0.8, 1.0, 2.0)}


def _timed(fn):
    from abacusutils_amd import _lib
    t0, t1 = _lib.Event(), _lib.Event()
    t0.record()
    out = fn()
    t1.record()
    _lib.sync()
    return out, t1.elapsed_ms_since(t0)


def _kernels():
    from abacusutils_amd import _lib
    prof = _lib.profile_get()
    return {k: {'ms_per_launch': round(v / cnt, 4), 'launches': int(cnt), 'ms': round(v, 3)}
            for k, (v, cnt) in sorted(prof.items(), key=lambda kv: -kv[1][0]) if cnt}


def _copy_rate(n, repeats=20):
    """bytes per second (read + written) of a device-to-device copy of one padded mesh"""
    import ctypes as C

    from abacusutils_amd import _lib
    pitch = (n + 2 + 31) // 32 * 32
    nbytes = n * n * pitch * 4
    a = _lib.DeviceArray(nbytes=nbytes, dtype=np.float32, shape=(n, n, pitch))
    b = _lib.DeviceArray(nbytes=nbytes, dtype=np.float32, shape=(n, n, pitch))
    lib = _lib.lib()
    _lib.check(lib.abacus_memset(a.ptr, 0, C.c_uint64(nbytes)))
    copy = lambda: _lib.check(lib.abacus_memcpy_d2d(b.ptr, a.ptr, C.c_uint64(nbytes)))   # noqa: E731
    for _ in range(3):
        copy()
    _lib.sync()
    _, ms = _timed(lambda: [copy() for _ in range(repeats)])
    a.free()
    b.free()
    return 2.0 * nbytes * repeats / (ms * 1e-3), nbytes


def step_copy(n):
    rate, nbytes = _copy_rate(n)
    return {'n': n, 'padded_mesh_bytes': nbytes, 'copy_TBps': round(rate * 1e-12, 3)}


def step_chain(n, nq, second_order=True):
    from abacusutils_amd import _lib
    from abacusutils_amd.analysis.wst import calc_wst
    rate, nbytes = _copy_rate(n)
    pos = np.random.default_rng(2).random((NPTS, 3), dtype=np.float32) * np.float32(LBOX)
    dev = _lib.DeviceArray(pos)
    call = lambda: calc_wst(dev, LBOX, J=J, L=L, q=EXPONENTS[nq], nmesh=n, second_order=second_order)   # noqa: E731
    _, first = _timed(call)
    ms = [_timed(call)[1] for _ in range(3)]
    _lib.profile_reset()
    _lib.profile_enable(True)
    out = call()
    _lib.sync()
    _lib.profile_enable(False)
    dev.free()
    kern = _kernels()
    total = sum(k['ms'] for k in kern.values())
    fft = sum(k['ms'] for name, k in kern.items() if 'fft' in name or 'c2r' in name or 'r2c' in name)
    cells = float(n) ** 3
    # bytes each launch must move: wst_mult 8 B per cell, wst_accum 8 B (first m) or 12 B, wst_moments 4 B, wst_scale 8 B
    nm = sum(2 * l + 1 for l in range(L + 1))
    fields = J * (L + 1) * (1 + ((J - 1) / 2.0 if second_order else 0.0))
    accum_bytes = (fields * 8.0 + (J * nm * (1 + ((J - 1) / 2.0 if second_order else 0.0)) - fields) * 12.0) * cells
    need = {'wst_mult': 8.0 * cells, 'wst_moments': 4.0 * cells, 'wst_scale': 8.0 * cells}
    against = {}
    for name, per_launch in need.items():
        if name in kern:
            bps = per_launch / (kern[name]['ms_per_launch'] * 1e-3)
            against[name] = {'TBps': round(bps * 1e-12, 3), 'of_copy_rate': round(bps / rate, 3)}
    if 'wst_accum' in kern:
        bps = accum_bytes / (kern['wst_accum']['ms'] * 1e-3)
        against['wst_accum'] = {'TBps': round(bps * 1e-12, 3), 'of_copy_rate': round(bps / rate, 3)}
    return {'n': n, 'npts': NPTS, 'J': J, 'L': L, 'q': list(EXPONENTS[nq]), 'second_order': second_order, 'first_call_ms': round(first, 2),
            'call_ms': [round(t, 2) for t in ms], 'copy_TBps': round(rate * 1e-12, 3), 'kernel_ms_total': round(total, 2),
            'transform_ms': round(fft, 2), 'transform_share': round(fft / total, 3), 'kernels': kern, 'streaming_against_copy': against,
            'S0': [float(v) for v in out['S0']], 'S1_j0': [float(v) for v in out['S1'][0, :, 0]]}


def run_step(name):
    if name.startswith('copy'):
        return step_copy(int(name[4:]))
    if name.startswith('chain'):
        n, nq = name[5:].split('q')
        return step_chain(int(n), int(nq))
    if name.startswith('first'):
        n, nq = name[5:].split('q')
        return step_chain(int(n), int(nq), second_order=False)
    raise SystemExit(f'unknown step {name}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--step')
    ap.add_argument('--steps', default='copy256,chain256q1,chain256q4,first256q1')
    ap.add_argument('--out')
    a = ap.parse_args()
    if a.step:
        print(json.dumps({a.step: run_step(a.step)}))
        return 0
    merged = {}
    for name in a.steps.split(','):
        cmd = ['timeout', '-k', '10', str(LIMITS[name]), sys.executable, str(Path(__file__).resolve()), '--step', name]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:                 # a failure, a fault or a time limit: nothing more is started
            print(json.dumps({'failed_step': name, 'returncode': r.returncode, 'done': merged}))
            return r.returncode
        merged.update(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps({name: merged[name]}), flush=True)
        if a.out:
            Path(a.out).write_text(json.dumps(merged, indent=1) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
