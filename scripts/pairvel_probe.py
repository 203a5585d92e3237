"""pair_vel beside pair_count_w (rsum on) on the pair-count workload: 10^7 uniform points, 2 Gpc/h box, 20 logarithmic bins
0.1 .. 30, columns, velocities and weights resident, both entries on the same columns in one process; then pair_vel with the
comparator option pairvel_lds_top.  Usage: python scripts/pairvel_probe.py [n] [steps] [out.json]  (profiles/pairvel/README.md)"""
import ctypes as C, json, sys, time
import numpy as np
from abacusutils_amd import _lib
from abacusutils_amd.analysis.pairwise_velocity import pairwise_velocity_sums
from abacusutils_amd.analysis.tpcf_corrfunc import _paircount_weighted

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
box = 2000.0
rng = np.random.default_rng(1)
cols = [rng.random(n, dtype=np.float32) * np.float32(box) for _ in range(3)]
vel = [rng.normal(0, 300, n).astype(np.float32) for _ in range(3)]
w = (0.5 + rng.random(n)).astype(np.float32)
bins = np.geomspace(0.1, 30.0, 21).astype(np.float32)
d = [_lib.DeviceArray(c) for c in cols + vel]
dw = _lib.DeviceArray(w)

def cand():
    c = C.c_uint64(0)
    _lib.check(_lib.lib().abacus_paircount_stats(C.byref(c), None, None, None))
    return c.value

def weighted():
    return _paircount_weighted(0, *d[:3], box, bins, W1=dw)
def velsums():
    return pairwise_velocity_sums(0, *d, box, bins, W1=dw)
def velsums_lds():
    _lib.set_option('pairvel_lds_top', 1)
    try:
        return pairwise_velocity_sums(0, *d, box, bins, W1=dw)
    finally:
        _lib.set_option('pairvel_lds_top', 0)

out = {'n': n, 'steps': steps}
res = {}
for name, fn in (('weighted_rsum', weighted), ('pairvel', velsums), ('pairvel_lds_top', velsums_lds)):
    for _ in range(2):
        r = fn()
    _lib.sync()
    _lib.profile_reset(); _lib.profile_enable(True)
    walls = []
    for _ in range(steps):
        _lib.sync(); t0 = time.perf_counter(); r = fn(); _lib.sync(); walls.append((time.perf_counter() - t0) * 1e3)
    prof = _lib.profile_get(); _lib.profile_enable(False)
    c = cand()
    kern = {k: v[0] / v[1] for k, v in prof.items()}
    main = kern.get('pair_vel', kern.get('pair_count_w'))
    res[name] = r
    npairs = (r[0] if isinstance(r, tuple) else r['npairs'])
    out[name] = dict(call_ms=walls, call_ms_median=float(np.median(walls)), kernel_ms=kern, candidates=c, counted=int(npairs.sum()),
                     candidates_per_s=c / (main * 1e-3))
    print(name, json.dumps(out[name]), flush=True)
np.testing.assert_array_equal(res['weighted_rsum'][0], res['pairvel']['npairs'])
np.testing.assert_array_equal(res['weighted_rsum'][0], res['pairvel_lds_top']['npairs'])
out['wsum_rel_diff'] = float(np.abs(res['weighted_rsum'][1] / res['pairvel']['wsum'] - 1).max())
if len(sys.argv) > 3:
    json.dump(out, open(sys.argv[3], 'w'), indent=1)
print('ok', out['wsum_rel_diff'])
