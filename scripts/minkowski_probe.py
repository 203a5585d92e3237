#!/usr/bin/env python
"""Times the Minkowski functionals (abacusutils_amd.analysis.minkowski) on one MI355X against the time to read the mesh once.

    python scripts/minkowski_probe.py [--out FILE.json] [--steps counts512,counts1024,chain512,chain1024,numpy256]
    python scripts/minkowski_probe.py --step counts512          # one step, in this process

Without --step every step runs in a process of its own under `timeout -k 10 <seconds>`, one after the other, and the first one that
fails ends the run (the steps are chained as with &&): nothing is started on a device after a step has faulted or hung on it.

Steps:
  counts512/counts1024  a resident dense mesh of seeded white noise (the 1024^3 one is the 512^3 one tiled twice along every axis),
            thresholds linspace(-3, 3, nthr): `abacus_mf_counts_dev` at nthr = 1, 16 and 64, HIP-event time of the call (kernels, the
            copy of 260 totals and the host's suffix sums) and the library's event time of mf_count alone; `abacus_mf_moments_dev`;
            each against the time to read the mesh once, n^3 * 4 B / 6.29 TB/s (MI355X_MICROARCH.md, "Chip-level parameters", row
            "HBM3E peak BW": "8.0 TB/s spec; 6.29 TB/s measured (float4 copy, 79%)").
  chain512/chain1024    the whole `calc_minkowski` call at 1e7 uniform particles resident in HBM, TSC, compensated, interlaced,
            R = 2 cells, 16 thresholds in units of sigma: first call (plans) and repeated, and the library's event time per kernel.
  numpy256  the NumPy statement tests/minkowski_statement.py at 256^3 and 16 thresholds on the host, for scale.
Prints one JSON line per step; --out writes the merged result of a whole run."""
import argparse
import ctypes as C
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

LIMITS = {'counts512': 240, 'counts1024': 420, 'chain512': 300, 'chain1024': 420, 'numpy256': 300}
HBM_READ_BPS = 6.29e12
LBOX = 2000.0
NPTS = 10_000_000


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
    return {k: {'ms_per_launch': round(v / cnt, 4), 'launches': int(cnt)} for k, (v, cnt) in sorted(prof.items(), key=lambda kv: -kv[1][0]) if cnt}


def step_counts(n):
    from abacusutils_amd import _lib
    base = np.random.default_rng(1).standard_normal((512, 512, 512), dtype=np.float32)
    mesh = base if n == 512 else np.tile(base, (n // 512,) * 3)
    dev = _lib.DeviceArray(mesh)
    del mesh
    read_ms = float(n) ** 3 * 4.0 / HBM_READ_BPS * 1e3
    res = {'n': n, 'mesh_read_once_ms': round(read_ms, 4)}
    lib = _lib.lib()
    for nthr in (1, 16, 64):
        t32 = np.ascontiguousarray(np.linspace(-3, 3, nthr) if nthr > 1 else [0.0], dtype=np.float32)
        out = np.empty((4, nthr), dtype=np.int64)
        call = lambda: _lib.check(lib.abacus_mf_counts_dev(dev.ptr, n, n, _lib.ptr(t32), nthr, _lib.ptr(out)))   # noqa: E731
        call()
        ms = [_timed(call)[1] for _ in range(5)]
        _lib.profile_reset()
        _lib.profile_enable(True)
        call()
        _lib.sync()
        _lib.profile_enable(False)
        kern = _kernels()
        k_ms = kern.get('mf_count', {}).get('ms_per_launch', 0.0)
        res[f'nthr{nthr}'] = {'call_ms_min': round(min(ms), 4), 'call_ms': [round(t, 4) for t in ms], 'mf_count_ms': k_ms,
                              'mf_count_final_ms': kern.get('mf_count_final', {}).get('ms_per_launch', 0.0),
                              'mf_count_over_mesh_read': round(k_ms / read_ms, 2), 'call_over_mesh_read': round(min(ms) / read_ms, 2),
                              'voxels_at_first_threshold': int(out[3, 0])}
    s = np.empty(2)
    mom = lambda: _lib.check(lib.abacus_mf_moments_dev(dev.ptr, n, n, _lib.ptr(s)))   # noqa: E731
    mom()
    ms = [_timed(mom)[1] for _ in range(5)]
    res['moments'] = {'call_ms_min': round(min(ms), 4), 'call_over_mesh_read': round(min(ms) / read_ms, 2)}
    dev.free()
    return res


def step_chain(n):
    from abacusutils_amd import _lib
    from abacusutils_amd.analysis.minkowski import calc_minkowski
    pos = np.random.default_rng(2).random((NPTS, 3), dtype=np.float32) * np.float32(LBOX)
    dev = _lib.DeviceArray(pos)
    nu = np.linspace(-3, 3, 16)
    call = lambda: calc_minkowski(dev, LBOX, nu, 2.0 * LBOX / n, nmesh=n)   # noqa: E731
    _, first = _timed(call)
    ms = [_timed(call)[1] for _ in range(3)]
    _lib.profile_reset()
    _lib.profile_enable(True)
    out = call()
    _lib.sync()
    _lib.profile_enable(False)
    dev.free()
    return {'n': n, 'npts': NPTS, 'first_call_ms': round(first, 2), 'call_ms': [round(t, 2) for t in ms], 'kernels': _kernels(),
            'mesh_read_once_ms': round(float(n) ** 3 * 4.0 / HBM_READ_BPS * 1e3, 4), 'sigma': out['sigma'], 'V0': [round(float(v), 5) for v in out['V'][0]]}


def step_numpy256():
    sys.path.insert(0, str(ROOT / 'tests'))
    import minkowski_statement as st
    mesh = np.random.default_rng(3).standard_normal((256, 256, 256), dtype=np.float32)
    t0 = time.perf_counter()
    c = st.counts(mesh, np.linspace(-3, 3, 16))
    return {'n': 256, 'nthr': 16, 'statement_s': round(time.perf_counter() - t0, 2), 'voxels_at_first_threshold': int(c[3, 0])}


def run_step(name):
    if name.startswith('counts'):
        return step_counts(int(name[6:]))
    if name.startswith('chain'):
        return step_chain(int(name[5:]))
    if name == 'numpy256':
        return step_numpy256()
    raise SystemExit(f'unknown step {name}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--step')
    ap.add_argument('--steps', default='counts512,counts1024,chain512,chain1024,numpy256')
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
