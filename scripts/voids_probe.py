#!/usr/bin/env python
"""Times the spherical void finder on one MI355X.

    python scripts/voids_probe.py [--n 1e7] [--nmesh 512] [--reps 3] [--worst 256] [--out FILE.json]

Workloads: `n` points in a 2 Gpc/h box, positions resident in HBM as an (N, 3) float32 DeviceArray; a uniform catalogue and the
clustered one of scripts/groups_probe.py; 16 radii from 40 down to 5, threshold -0.7.  Per catalogue: HIP-event time of the whole
`find_voids` (one warm-up, then the mean, smallest and largest of `reps` calls), the library's event time per kernel from `reps`
further calls, the candidates, voids and rounds per level.  Beside them: a device-to-device copy of 8 bytes per mode (read 8,
write 8: the traffic of void_tophat) for the copy rate, and `count_in_spheres` of the same catalogue at the one radius 5 for scale.
Last, the worst case of the rounds: a constant mesh of `worst`^3 cells below the threshold, radii of 3, 2.5, 1.5 and 1 cells.
Prints one JSON line; --out also writes it to a file (after every stage, so that a stage that runs long loses nothing)."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from abacusutils_amd import _lib  # noqa: E402
from abacusutils_amd.analysis import spheres as S  # noqa: E402
from abacusutils_amd.analysis import voids as V  # noqa: E402
from groups_probe import clustered  # noqa: E402
from spheres_probe import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', default='1e7')
    ap.add_argument('--nmesh', type=int, default=512)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--worst', type=int, default=256)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    n, L, nmesh = int(float(a.n)), 2000.0, a.nmesh
    radii = np.geomspace(40.0, 5.0, 16)
    print('device:', _lib.device_name(), file=sys.stderr)
    line = {'n': n, 'Lbox': L, 'nmesh': nmesh, 'radii': [round(float(r), 4) for r in radii], 'reps': a.reps, 'rows': {}}

    def save():
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text(json.dumps(line, indent=1) + '\n')

    # the copy rate at the traffic of void_tophat
    nbytes = nmesh * nmesh * (nmesh // 2 + 1) * 8
    src, dst = _lib.DeviceArray(nbytes=nbytes, dtype=np.uint8, shape=(nbytes,)), _lib.DeviceArray(nbytes=nbytes, dtype=np.uint8, shape=(nbytes,))
    _lib.check(_lib.lib().abacus_memset(src.ptr, 0, C.c_uint64(nbytes)))
    copy = timed(lambda: _lib.check(_lib.lib().abacus_memcpy_d2d(dst.ptr, src.ptr, C.c_uint64(nbytes))), 10, 'memcpy_d2d')
    copy['bytes_moved'] = 2 * nbytes
    copy['GB_per_s'] = round(2 * nbytes / (copy['event_ms_min'] * 1e-3) / 1e9, 1)
    line['copy'] = copy
    src.free()
    dst.free()
    save()

    last = {}
    for cat, p in (('uniform', np.random.default_rng(500).random((n, 3), dtype=np.float32) * np.float32(L)), ('clustered', clustered(n, L, 501))):
        pos = _lib.DeviceArray(np.ascontiguousarray(p, dtype=np.float32))
        row = timed(lambda: last.__setitem__('v', V.find_voids(pos, L, radii, nmesh=nmesh)), a.reps, 'void_accept')
        v = last['v']
        row.update(counts=v['counts'].tolist(), nvoids=int(len(v['level'])), size_function=V.void_size_function(v, radii, L)['dn_dlnR'].tolist())
        k = row['kernels_ms_per_call'].get('void_tophat')
        row['tophat_GB_per_s'] = None if not k else round(16 * 2 * nbytes / (k * 1e-3) / 1e9, 1)      # 16 levels per call
        line['rows'][cat] = row
        pos.free()
        cols = [_lib.DeviceArray(np.ascontiguousarray(p[:, i])) for i in range(3)]
        line['rows'][cat + ': count_in_spheres, r = 5'] = timed(lambda: S.count_in_spheres(*cols, L, [5.0], kmax=64), a.reps, 'sphere_count')
        for c in cols:
            c.free()
        save()

    if a.worst:
        w = a.worst
        mesh = _lib.DeviceArray(np.full((w, w, w), -1.0, dtype=np.float32))
        _lib.profile_reset()
        _lib.profile_enable(True)
        t0 = time.perf_counter()
        v = V.find_voids_mesh(mesh, float(w), (3.0, 2.5, 1.5, 1.0))
        _lib.sync()
        wall = time.perf_counter() - t0
        _lib.profile_enable(False)
        line['worst'] = {'n': w, 'wall_s': round(wall, 3), 'counts': v['counts'].tolist(),
                         'kernels_ms': {k: round(ms, 3) for k, (ms, cnt) in _lib.profile_get().items() if cnt}}
        mesh.free()
        save()
    print(json.dumps(line))


if __name__ == '__main__':
    main()
