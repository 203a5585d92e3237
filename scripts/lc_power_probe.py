#!/usr/bin/env python
"""Times the light-cone power spectrum multipoles (analysis/lc_power.py) on one MI355X.

    python scripts/lc_power_probe.py [--nmesh 512] [--galaxies 1e6] [--randoms 1e7] [--reps 3] [--out FILE.json]

Galaxies and randoms fill an octant shell seen from its centre, weighted, columns resident in HBM.  `calc_power_lc` (l = 0, 2, 4,
compensated, TSC) is timed with a COLD randoms mesh (the cache of the LCRandoms emptied before every call: the randoms are deposited
again) and with a WARM one.  Wall time: host clock around a call, mean of `reps` after a warm-up call.  Kernel times: the library's
event pairs around each launch.  `lc_ylm_mult` moves 8 bytes per cell, `lc_ylm_accum` 16 bytes per mode for the first m of a multipole
and 24 from the second on; those over their times are set against the COPY rate, a device-to-device copy of one padded mesh (read +
write) timed in the same process, as scripts/recon_probe.py does.  Prints one JSON line; --out also writes it to a file."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from abacusutils_amd import _lib  # noqa: E402
from abacusutils_amd.analysis import lc_power  # noqa: E402
from lcv_probe import copy_rate  # noqa: E402


def shell(rng, count, rmin, rmax):
    r = (rmin**3 + (rmax**3 - rmin**3) * rng.random(count)) ** (1 / 3)
    mu, phi = rng.random(count), rng.random(count) * np.pi / 2
    st = np.sqrt(1 - mu * mu)
    return [(r * st * np.cos(phi)).astype(np.float32), (r * st * np.sin(phi)).astype(np.float32), (r * mu).astype(np.float32)]


def timed(call, reps, before=lambda: None):
    before()
    call()
    _lib.sync()
    wall = 0.0
    for _ in range(reps):
        before()
        _lib.sync()
        t = time.perf_counter()
        call()
        _lib.sync()
        wall += time.perf_counter() - t
    _lib.profile_reset()
    _lib.profile_enable(True)
    for _ in range(reps):
        before()
        call()
    _lib.sync()
    _lib.profile_enable(False)
    return wall / reps * 1e3, {k: (ms, int(cnt)) for k, (ms, cnt) in _lib.profile_get().items() if cnt}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nmesh', type=int, default=512)
    ap.add_argument('--galaxies', default='1e6')
    ap.add_argument('--randoms', default='1e7')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    n, ng, nr = a.nmesh, int(float(a.galaxies)), int(float(a.randoms))
    print('device:', _lib.device_name(), file=sys.stderr)
    nb = C.c_uint64(0)
    _lib.check(_lib.lib().abacus_zcv_spectrum_bytes(n, C.byref(nb)))
    rate, copy_ms = copy_rate(nb.value)
    rng = np.random.default_rng(n)
    gal, ran = shell(rng, ng, 800.0, 2000.0), shell(rng, nr, 800.0, 2000.0)
    wg, wr = (rng.uniform(0.5, 1.5, len(c[0])).astype(np.float32) for c in (gal, ran))
    nbar = lc_power.radial_nbar(*ran, np.linspace(800.0, 2000.0, 25), 0.125)
    dev = [_lib.DeviceArray(c) for c in gal + ran + [wg, wr, nbar]]
    R = lc_power.LCRandoms(*dev[3:6], w=dev[7], nbar=dev[8])

    def cold():
        for m in R._mesh.values():
            m.free()
        R._mesh.clear()

    def call():
        return lc_power.calc_power_lc(*dev[:3], R, 40, nmesh=n, w1=dev[6])
    res = call()
    phases = {}
    for name, before in (('cold randoms mesh', cold), ('warm randoms mesh', lambda: None)):
        wall, prof = timed(call, a.reps, before)
        phases[name] = {'wall_ms_per_call': round(wall, 3), 'kernel_ms_per_call': round(sum(ms for ms, _ in prof.values()) / a.reps, 3),
                        'kernels_ms_per_call': {k: [round(ms / a.reps, 3), cnt // a.reps] for k, (ms, cnt) in sorted(prof.items(), key=lambda kv: -kv[1][0])}}
    kernels = phases['warm randoms mesh']['kernels_ms_per_call']
    cells, modes = float(n) ** 3, float(n) * n * (n // 2 + 1)
    stream = {}
    for name, nbytes in (('lc_ylm_mult', 14 * 8 * cells), ('lc_ylm_accum', (2 * 16 + 12 * 24) * modes)):
        ms, cnt = kernels[name]
        stream[name] = {'launches_per_call': cnt, 'bytes_per_call': nbytes, 'ms_per_call': ms, 'TB_per_s': round(nbytes / (ms * 1e-3) / 1e12, 3),
                        'fraction_of_copy_rate': round(nbytes / (ms * 1e-3) / rate, 3)}
    fft_ms = sum(ms for k, (ms, _) in kernels.items() if 'fft' in k)
    line = {'nmesh': n, 'galaxies': ng, 'randoms': nr, 'reps': a.reps, 'Lbox': res['Lbox'], 'copy_TB_per_s': round(rate / 1e12, 3),
            'copy_ms': round(copy_ms, 4), 'padded_mesh_bytes': nb.value, 'finite': bool(np.isfinite(res['poles']).all()),
            'mesh_built': R.mesh_built, 'phases': phases, 'streaming': stream, 'transforms_ms_per_call': round(fft_ms, 3),
            'transforms_share_of_kernels': round(fft_ms / phases['warm randoms mesh']['kernel_ms_per_call'], 3)}
    print(json.dumps(line))
    for d in dev:
        d.free()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(line, indent=1) + '\n')


if __name__ == '__main__':
    main()
