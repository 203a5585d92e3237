#!/usr/bin/env python
"""Timings of hod.zcv.zenbu_window.periodic_window_function behind profiles/window/README.md (needs an MI355X).

    python scripts/window_probe.py [--statement] [--big] [--quick] [--out FILE.json]

Box 2000, linear edges to the Nyquist wavenumber, kin the bin centres, k2weight.  Default: nmesh 576 with 288 bins and 1152 with 576;
three warm-up calls, then the wall time of 11 calls (host clock around a call that ends in a copy to the host) and, with the
library's event pairs around each launch, the kernel times of 7 more.  --statement: also times tests/window_statement.py at 576 on
this host and compares.  --big: nmesh 2048 with 1024 bins instead (the device-memory path).  --quick: one warm-up and three calls,
for a run under `rocprofv3 --kernel-trace --stats` or `--pmc`."""
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / 'tests'))
from abacusutils_amd import _lib  # noqa: E402
from abacusutils_amd.hod.zcv.zenbu_window import periodic_window_function, window_moments  # noqa: E402

quick = '--quick' in sys.argv
L = 2000.0
out = {'device': _lib.device_name()}
cases = [(576, 288), (1152, 576)]
if '--big' in sys.argv:
    cases = [(2048, 1024)]
for nmesh, nb in cases:
    kout = np.linspace(0.0, np.pi * nmesh / L, nb + 1)
    kin = 0.5 * (kout[1:] + kout[:-1])
    for _ in range(1 if quick else 3):
        periodic_window_function(nmesh, L, kout, kin)
    walls, kern, mom = [], [], []
    for _ in range(3 if quick else 11):
        _lib.sync()
        t = time.perf_counter()
        w, keff = periodic_window_function(nmesh, L, kout, kin)
        walls.append(time.perf_counter() - t)
        t = time.perf_counter()
        m = window_moments(nmesh, L, kout)
        mom.append(time.perf_counter() - t)
    if not quick:
        _lib.profile_enable(True)
        for _ in range(7):
            _lib.profile_reset()
            window_moments(nmesh, L, kout)
            _lib.sync()
            kern.append({k: v[0] for k, v in _lib.profile_get().items()})
        _lib.profile_enable(False)
    modes = nmesh * nmesh * (nmesh // 2)
    rec = dict(nmesh=nmesh, bins=nb, modes=modes, counted=float(m['nmodes'].sum()), wall_ms=[1e3 * x for x in walls],
               wall_median_ms=1e3 * float(np.median(walls)), moments_wall_median_ms=1e3 * float(np.median(mom)), kernel_ms=kern)
    if kern:
        tot = [sum(k.values()) for k in kern]
        rec['kernel_median_ms'] = float(np.median(tot))
        rec['modes_per_s_kernel'] = modes / (1e-3 * float(np.median([k.get('window_moments', k.get('window_moments_global', 0.0)) for k in kern])))
    rec['keff_last'] = float(keff[-1])
    out[f'n{nmesh}_b{nb}'] = rec
    print(json.dumps(rec), flush=True)
if '--statement' in sys.argv:
    from window_statement import window_statement
    nmesh, nb = 576, 288
    kout = np.linspace(0.0, np.pi * nmesh / L, nb + 1)
    kin = 0.5 * (kout[1:] + kout[:-1])
    t = time.perf_counter()
    w64, k64, S, nmodes, ksum = window_statement(nmesh, L, kout, kin, True, chunk=8)
    dt = time.perf_counter() - t
    w, keff = periodic_window_function(nmesh, L, kout, kin)
    m = window_moments(nmesh, L, kout)
    from window_statement import block_error
    out['statement_576'] = dict(seconds=dt, nmodes_equal=bool(np.array_equal(m['nmodes'], nmodes)), window_err=float(block_error(w, w64, nb, nb)),
                                keff_err=float(np.abs(keff - k64).max() / np.abs(k64).max()))
    print(json.dumps(out['statement_576']), flush=True)
if '--out' in sys.argv:
    Path(sys.argv[sys.argv.index('--out') + 1]).write_text(json.dumps(out, indent=1) + '\n')
