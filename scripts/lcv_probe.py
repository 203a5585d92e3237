#!/usr/bin/env python
"""Times the linear-control-variates chain (hod/zcv/linear_fields.py, tracer_power.recon_power) on one MI355X.

    python scripts/lcv_probe.py [--nmesh 576] [--tracers 1e6] [--randoms 5e6] [--reps 5] [--out FILE.json]

Wall time per call: host clock around a call that ends in a device synchronise or a copy to the host, mean of `reps` after a
warm-up call; positions and the density resident unless said otherwise.  Kernel times: the library's event pairs around each
launch, summed over `reps` calls and divided by the launches.  Each new streaming kernel's algorithmic bytes (from the shapes) over
its time is set against the COPY rate: a device-to-device copy of one padded spectrum (read + write) timed in the same process.
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
from abacusutils_amd.hod.zcv import linear_fields as lf  # noqa: E402
from abacusutils_amd.hod.zcv.tracer_power import recon_power  # noqa: E402


def copy_rate(nbytes, reps=20):
    """bytes/s of a device-to-device copy of `nbytes` (2 * nbytes move per copy)"""
    a = _lib.DeviceArray(nbytes=nbytes, dtype=np.uint8, shape=(nbytes,))
    b = _lib.DeviceArray(nbytes=nbytes, dtype=np.uint8, shape=(nbytes,))
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


def timed(call, reps):
    call()                                   # warm-up: code objects, plans, tables, buffers kept on the holder
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nmesh', type=int, default=576, help="the reference tutorial's LCV mesh")
    ap.add_argument('--tracers', default='1e6')
    ap.add_argument('--randoms', default='5e6')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    n, L = a.nmesh, 2000.0
    ntr, nrn = int(float(a.tracers)), int(float(a.randoms))
    print('device:', _lib.device_name(), file=sys.stderr)
    modes = float(n) * n * (n // 2 + 1)
    nb = C.c_uint64(0)
    _lib.check(_lib.lib().abacus_zcv_spectrum_bytes(n, C.byref(nb)))
    padded = float(nb.value)
    rate, copy_ms = copy_rate(nb.value)
    rng = np.random.default_rng(n)
    dens = rng.standard_normal((n, n, n), dtype=np.float32)
    dd = _lib.DeviceArray(dens)
    tracer = _lib.DeviceArray((rng.random((ntr, 3), dtype=np.float32) * np.float32(L)).astype(np.float32))
    randoms = _lib.DeviceArray((rng.random((nrn, 3), dtype=np.float32) * np.float32(L)).astype(np.float32))
    ke, me = np.linspace(0.0, np.pi * n / L, n // 2 + 1), np.linspace(0.0, 1.0, 5)
    poles = [0, 2, 4]
    phases, kernels = {}, {}

    def record(phase, wall_ms, prof, bytes_per_launch):
        phases[phase] = {'wall_ms_per_call': round(wall_ms, 3), 'kernel_ms_per_call': round(sum(ms for ms, _ in prof.values()) / a.reps, 3),
                         'kernels_ms_per_call': {k: round(ms / a.reps, 3) for k, (ms, _) in sorted(prof.items(), key=lambda kv: -kv[1][0])}}
        for name, per in bytes_per_launch.items():
            ms, cnt = prof[name]
            kernels[f'{name} ({phase})'] = {'launches_per_call': cnt // a.reps, 'bytes_per_launch': per, 'ms_per_launch': round(ms / cnt, 4),
                                            'TB_per_s': round(per * cnt / (ms * 1e-3) / 1e12, 3),
                                            'fraction_of_copy_rate': round(per * cnt / (ms * 1e-3) / rate, 3)}

    holder = []

    def make(src):
        if holder:
            holder.pop().free()
        holder.append(lf.linear_fields(src, L, n))
    record('linear_fields (density resident)', *timed(lambda: make(dd), a.reps), {'lcv_linear': 24 * modes})
    wall, prof = timed(lambda: make(dens), a.reps)
    phases['linear_fields (density from NumPy)'] = {'wall_ms_per_call': round(wall, 3)}
    lin = holder[0]
    record('linear_power', *timed(lambda: lf.linear_power(lin, ke, me, poles), a.reps), {})
    # two autos (12 bytes per mode) and one cross (20) per call
    record('linear_power3d', *timed(lambda: lf.linear_power3d(lin), a.reps), {'lcv_power3d': (12 + 12 + 20) / 3 * modes})
    record('recon_power', *timed(lambda: recon_power(tracer, randoms, lin, ke, me, poles), a.reps), {'lcv_sub': 3 * padded})
    record('recon_power (no randoms)', *timed(lambda: recon_power(tracer, None, lin, ke, me, poles), a.reps), {})
    recon_power(tracer, randoms, lin, ke, me, poles)
    record('combine recsym', *timed(lambda: lf.combine_field_spectra_k3D_lcv(1.8, 0.75, 0.6, lin, n, L, None, 'recsym'), a.reps),
           {'lcv_combine': 36 * modes})
    record('combine reciso', *timed(lambda: lf.combine_field_spectra_k3D_lcv(1.8, 0.75, 0.6, lin, n, L, 10.0, 'reciso'), a.reps),
           {'lcv_combine_reciso': 36 * modes})
    pk = lf.combine_field_spectra_k3D_lcv(1.8, 0.75, 0.6, lin, n, L, 10.0, 'reciso')
    line = {'nmesh': n, 'tracers': ntr, 'randoms': nrn, 'reps': a.reps, 'copy_TB_per_s': round(rate / 1e12, 3), 'copy_ms': round(copy_ms, 4),
            'padded_spectrum_bytes': nb.value, 'finite': bool(all(np.isfinite(g[::7, ::7, ::7]).all() for g in pk)), 'phases': phases,
            'kernels': kernels}
    print(json.dumps(line))
    lin.free()
    for d in (dd, tracer, randoms):
        d.free()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(line, indent=1) + '\n')


if __name__ == '__main__':
    main()
