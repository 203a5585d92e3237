#!/usr/bin/env python
"""Times BAO reconstruction (hod/zcv/reconstruction.py) on one MI355X at the LCV tutorial mesh.

    python scripts/recon_probe.py [--nmesh 576] [--tracers 1e6] [--randoms 5e6] [--reps 5] [--paste CIC] [--out FILE.json]

Wall time per call: host clock around a call that ends in a device synchronise, mean of `reps` after a warm-up call; positions
resident.  Kernel times: the library's event pairs around each launch, summed over `reps` calls and divided by the launches.
`recon_mult` moves 32 bytes per mode (8 read, 24 written); that over its time is set against the COPY rate: a device-to-device copy
of one padded spectrum (read + write) timed in the same process, as scripts/lcv_probe.py does.  `recon_shift` is a gather: it is
timed for the tracers in catalogue order (halos at random places, the galaxies of a halo beside each other), for the randoms in
random order and for the same randoms sorted once by their (x, y) cell row, and set beside the four transforms of the call.
Prints one JSON line; --out also writes it to a file."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from abacusutils_amd import _lib  # noqa: E402
from abacusutils_amd.hod.zcv import reconstruction as rc  # noqa: E402
from lcv_probe import copy_rate  # noqa: E402


def timed(call, reps):
    call()                                   # warm-up: code objects, plans, tables
    _lib.sync()
    t = time.perf_counter()
    for _ in range(reps):
        call()
    _lib.sync()
    wall_ms = (time.perf_counter() - t) / reps * 1e3
    _lib.profile_reset()
    _lib.profile_enable(True)
    for _ in range(reps):
        call()
    _lib.sync()
    _lib.profile_enable(False)
    return wall_ms, {k: (ms, int(cnt)) for k, (ms, cnt) in _lib.profile_get().items()}


def catalogue(rng, count, L):
    """galaxies in catalogue order: halo centres at random places, 1 + Poisson(0.25) galaxies per halo within 1 unit of it"""
    per = 1 + rng.poisson(0.25, size=count)
    per = per[:int(np.searchsorted(np.cumsum(per), count)) + 1]
    centres = rng.random((len(per), 3)) * L
    pos = np.repeat(centres, per, axis=0)[:count] + rng.normal(0.0, 0.5, size=(count, 3))
    return np.remainder(pos, L).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nmesh', type=int, default=576, help="the reference tutorial's LCV mesh")
    ap.add_argument('--tracers', default='1e6')
    ap.add_argument('--randoms', default='5e6')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--paste', default='CIC')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    n, L = a.nmesh, 2000.0
    bias, f_growth, R = 1.8, 0.75, 15.0
    ntr, nrn = int(float(a.tracers)), int(float(a.randoms))
    print('device:', _lib.device_name(), file=sys.stderr)
    modes = float(n) * n * (n // 2 + 1)
    nb = C.c_uint64(0)
    _lib.check(_lib.lib().abacus_zcv_spectrum_bytes(n, C.byref(nb)))
    rate, copy_ms = copy_rate(nb.value)
    rng = np.random.default_rng(n)
    tr_host = catalogue(rng, ntr, L)
    rn_host = (rng.random((nrn, 3), dtype=np.float32) * np.float32(L)).astype(np.float32)
    cell = np.minimum((rn_host[:, :2] * (n / L)).astype(np.int64), n - 1)
    rn_sorted = np.ascontiguousarray(rn_host[np.lexsort((cell[:, 1], cell[:, 0]))])
    tracer, randoms, randoms_sorted = (_lib.DeviceArray(p) for p in (tr_host, rn_host, rn_sorted))
    shift_name = f'recon_shift_{a.paste.lower()}'
    phases = {}

    def phase(name, wall_ms, prof):
        phases[name] = {'wall_ms_per_call': round(wall_ms, 3), 'kernel_ms_per_call': round(sum(ms for ms, _ in prof.values()) / a.reps, 3),
                        'kernels_ms_per_call': {k: round(ms / a.reps, 3) for k, (ms, _) in sorted(prof.items(), key=lambda kv: -kv[1][0])}}
        return prof

    def recon(rn):
        out = rc.reconstruct(tracer, rn, L, n, bias, f_growth, R, rec_algo='recsym', rsd=True, paste=a.paste)
        for o in out:
            if o is not None:
                o.free()
    prof = phase('reconstruct (tracers + randoms in random order)', *timed(lambda: recon(randoms), a.reps))
    phase('reconstruct (tracers + randoms sorted by cell row)', *timed(lambda: recon(randoms_sorted), a.reps))
    phase('reconstruct (no randoms)', *timed(lambda: recon(None), a.reps))
    transforms_ms = sum(ms for k, (ms, _) in prof.items() if 'fft' in k) / a.reps        # one R2C (its passes), three C2R
    ms, cnt = prof['recon_mult']
    mult = {'launches_per_call': cnt // a.reps, 'bytes_per_launch': 32 * modes, 'ms_per_launch': round(ms / cnt, 4),
            'TB_per_s': round(32 * modes * cnt / (ms * 1e-3) / 1e12, 3), 'fraction_of_copy_rate': round(32 * modes * cnt / (ms * 1e-3) / rate, 3)}

    def field():
        rc.displacement_field(tracer, L, n, bias, f_growth, R, paste=a.paste).free()
    phase('displacement_field', *timed(field, a.reps))
    shifts = {}
    with rc.displacement_field(tracer, L, n, bias, f_growth, R, paste=a.paste) as disp:
        for name, pos in (('tracers in catalogue order', tracer), ('randoms in random order', randoms),
                          ('randoms sorted by (x, y) cell row', randoms_sorted)):
            wall, p = timed(lambda: rc.shift(pos, disp).free(), a.reps)
            ms, cnt = p[shift_name]
            shifts[name] = {'particles': len(pos), 'wall_ms_per_call': round(wall, 3), 'kernel_ms': round(ms / cnt, 4),
                            'particles_per_us': round(len(pos) / (ms / cnt * 1e3), 1)}
        sample = rc.shift(randoms_sorted, disp)
        finite = bool(np.isfinite(sample.get()[::97]).all())
        sample.free()
    line = {'nmesh': n, 'Lbox': L, 'tracers': ntr, 'randoms': nrn, 'reps': a.reps, 'paste': a.paste, 'copy_TB_per_s': round(rate / 1e12, 3),
            'copy_ms': round(copy_ms, 4), 'padded_spectrum_bytes': nb.value, 'finite': finite, 'phases': phases, 'recon_mult': mult,
            'four_transforms_ms_per_call': round(transforms_ms, 3), 'recon_shift': shifts}
    print(json.dumps(line))
    for d in (tracer, randoms, randoms_sorted):
        d.free()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(line, indent=1) + '\n')


if __name__ == '__main__':
    main()
