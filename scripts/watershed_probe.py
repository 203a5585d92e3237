#!/usr/bin/env python
"""Times the watershed void finder on one MI355X.

    python scripts/watershed_probe.py [--n 1e7] [--nmesh 256,512] [--reps 3] [--R 10] [--out FILE.json]

Fields, per mesh size: the density contrast of the clustered catalogue of scripts/groups_probe.py (`n` points, box 2000, TSC compensated
and interlaced) smoothed with a Gaussian of radius R - what `find_watershed_voids` works on - and an unsmoothed white mesh, which has
the most zones.  Each field is resident in HBM as a dense float32 DeviceArray.  Per field and connectivity: HIP-event time of the
whole `watershed_mesh` (one warm-up, then the mean, smallest and largest of `reps` calls; it includes the read-backs and the host sort
of the edges), the library's event time per kernel from `reps` further calls, the zones and the rounds of the tree; the same with the
option ws_reduce_per_cell (no combining of a wave's runs before the atomics).  Beside them: a device-to-device copy of the mesh (4
bytes read and 4 written per cell: the traffic of ws_descend) for the copy rate, and the wall time of one whole
`find_watershed_voids` with its host hierarchy.  Prints one JSON line; --out also writes it to a file after every stage."""
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
from abacusutils_amd.analysis import watershed as W  # noqa: E402
from groups_probe import clustered  # noqa: E402
from spheres_probe import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', default='1e7')
    ap.add_argument('--nmesh', default='256,512')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--R', type=float, default=10.0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    n, L = int(float(a.n)), 2000.0
    print('device:', _lib.device_name(), file=sys.stderr)
    line = {'n': n, 'Lbox': L, 'R': a.R, 'reps': a.reps, 'rows': {}}

    def save():
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text(json.dumps(line, indent=1) + '\n')

    pos = _lib.DeviceArray(np.ascontiguousarray(clustered(n, L, 501), dtype=np.float32))
    last = {}
    for nmesh in [int(s) for s in a.nmesh.split(',')]:
        nbytes = nmesh**3 * 4
        src, dst = _lib.DeviceArray(nbytes=nbytes, dtype=np.uint8, shape=(nbytes,)), _lib.DeviceArray(nbytes=nbytes, dtype=np.uint8, shape=(nbytes,))
        _lib.check(_lib.lib().abacus_memset(src.ptr, 0, C.c_uint64(nbytes)))
        copy = timed(lambda: _lib.check(_lib.lib().abacus_memcpy_d2d(dst.ptr, src.ptr, C.c_uint64(nbytes))), 10, 'memcpy_d2d')
        copy['GB_per_s'] = round(2 * nbytes / (copy['event_ms_min'] * 1e-3) / 1e9, 1)
        line['rows'][f'{nmesh}: copy of the mesh'] = copy
        src.free()
        dst.free()
        t0 = time.perf_counter()
        full = W.find_watershed_voids(pos, L, a.R, nmesh=nmesh, return_field=True)
        line['rows'][f'{nmesh}: find_watershed_voids, smoothed, 26'] = {'wall_s': round(time.perf_counter() - t0, 3), 'nzones': full['nzones']}
        save()
        white = np.random.default_rng(77).standard_normal((nmesh, nmesh, nmesh), dtype=np.float32)
        for name, field in (('smoothed', full['field']), ('white', white)):
            mesh = _lib.DeviceArray(field)
            for conn in (26, 6):
                for option in (0, 1):
                    if option and conn == 6:
                        continue
                    _lib.set_option('ws_reduce_per_cell', option)
                    row = timed(lambda: last.__setitem__('w', W.watershed_mesh(mesh, L, conn)), a.reps, 'ws_descend')
                    _lib.set_option('ws_reduce_per_cell', 0)
                    w = last['w']
                    row.update(nzones=w['nzones'], rounds=w['rounds'], largest_zone=int(w['ncell'].max()))
                    k = row['kernels_ms_per_call'].get('ws_descend')
                    row['descend_GB_per_s'] = None if not k else round(2 * nbytes / (k * 1e-3) / 1e9, 1)
                    line['rows'][f'{nmesh}: {name}, {conn}' + (', ws_reduce_per_cell' if option else '')] = row
                    save()
            mesh.free()
    pos.free()
    print(json.dumps(line))


if __name__ == '__main__':
    main()
