#!/usr/bin/env python
"""Times the shear chain (abacus_shearmark_dev: TSC deposit + Gaussian smoothing + tidal shear) on one MI355X.

    python scripts/shear_probe.py [--sizes 1000,1024] [--particles 1e7,1e8] [--sigma 1.0] [--reps 3] [--out FILE.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/shear_probe.py --sizes 1000 --particles 1e7 --reps 1

Per configuration: wall time per call (host clock around a call that ends in a device synchronise, after a warm-up call), the
library's per-kernel event times, each new kernel's algorithmic bytes and the fraction of the COPY rate it reaches - the copy
rate being a device-to-device copy of one N^3 float32 mesh (read + write = 8 N^3 bytes) timed in the same process.
Prints one JSON line per configuration; --out also writes them to a file."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from abacusutils_amd import _lib  # noqa: E402


def copy_rate(n, reps=10):
    """bytes/s of a device-to-device copy of an n^3 float32 mesh (8 n^3 bytes move per copy)"""
    nbytes = 4 * n ** 3
    a = _lib.DeviceArray(nbytes=nbytes, dtype=np.float32, shape=(n, n, n))
    b = _lib.DeviceArray(nbytes=nbytes, dtype=np.float32, shape=(n, n, n))
    _lib.check(_lib.lib().abacus_memset(a.ptr, 0, C.c_uint64(nbytes)))
    _lib.check(_lib.lib().abacus_memcpy_d2d(b.ptr, a.ptr, C.c_uint64(nbytes)))
    e0, e1 = _lib.Event(), _lib.Event()
    e0.record()
    for _ in range(reps):
        _lib.check(_lib.lib().abacus_memcpy_d2d(b.ptr, a.ptr, C.c_uint64(nbytes)))
    e1.record()
    ms = e1.elapsed_ms_since(e0) / reps
    a.free()
    b.free()
    return 2.0 * nbytes / (ms * 1e-3), ms


def algorithmic_bytes(n):
    """per launch, from the shapes: what each new kernel has to move"""
    cells, modes = float(n) ** 3, float(n) * n * (n // 2 + 1)
    return {'gauss_x_ring': 8 * cells, 'gauss_y_ring': 8 * cells, 'gauss_z_lds': 8 * cells, 'gauss_axis_direct': 8 * cells,
            'tidal_component': 16 * modes,            # 8 bytes in, 8 out per mode
            'shear_accumulate': (8 + 4 * 12 + 12) * cells / 6}   # first of six: 4 in + 4 out, the others 4 + 4 in, 4 out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='1000,1024')
    ap.add_argument('--particles', default='1e7,1e8')
    ap.add_argument('--sigma', type=float, default=1.0, help='smoothing scale in cells (shear_R = 2 Mpc/h on 2 Mpc/h cells)')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    L = 2000.0
    lines = []
    print('device:', _lib.device_name(), file=sys.stderr)
    for n in [int(s) for s in a.sizes.split(',')]:
        rate, copy_ms = copy_rate(n)
        for npart in [int(float(s)) for s in a.particles.split(',')]:
            rng = np.random.default_rng(npart % 1000 + n)
            pos = _lib.DeviceArray((rng.random((npart, 3), dtype=np.float32) * np.float32(L)).astype(np.float32))
            out = _lib.DeviceArray(nbytes=4 * n ** 3, dtype=np.float32, shape=(n, n, n))

            def call():
                _lib.check(_lib.lib().abacus_shearmark_dev(pos.ptr, C.c_int64(npart), n, C.c_double(L), C.c_double(a.sigma), out.ptr))
                _lib.sync()
            call()                                   # warm-up: code objects, plans, tables
            t = time.perf_counter()
            for _ in range(a.reps):
                call()
            wall_ms = (time.perf_counter() - t) / a.reps * 1e3
            _lib.profile_reset()
            _lib.profile_enable(True)
            call()
            _lib.profile_enable(False)
            prof = _lib.profile_get()
            ab = algorithmic_bytes(n)
            kernels = {}
            for name, (ms, launches) in sorted(prof.items(), key=lambda kv: -kv[1][0]):
                k = {'ms': round(ms, 3), 'launches': int(launches)}
                if name in ab and ms > 0:
                    k['bytes_per_launch'] = ab[name]
                    k['TB_per_s'] = round(ab[name] * launches / (ms * 1e-3) / 1e12, 3)
                    k['fraction_of_copy_rate'] = round(ab[name] * launches / (ms * 1e-3) / rate, 3)
                kernels[name] = k
            sample = out.get()[::max(1, n // 8), ::max(1, n // 8), ::max(1, n // 8)]
            line = {'nmesh': n, 'particles': npart, 'sigma_cells': a.sigma, 'wall_ms_per_call': round(wall_ms, 2),
                    'kernel_ms_sum': round(sum(k['ms'] for k in kernels.values()), 2), 'copy_TB_per_s': round(rate / 1e12, 3),
                    'copy_ms': round(copy_ms, 3), 'finite': bool(np.isfinite(sample).all()), 'mean_sample': float(sample.mean()),
                    'kernels': kernels}
            print(json.dumps(line))
            sys.stdout.flush()
            lines.append(line)
            pos.free()
            out.free()
            _lib.scratch_release()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text('\n'.join(json.dumps(x) for x in lines) + '\n')


if __name__ == '__main__':
    main()
