"""Array-level form of `abacusnbody.hod.zcv.tracer_power.get_tracer_power` (reference: abacusnbody/hod/zcv/tracer_power.py:155-286)
on the MI355X: the tracer field against the advected fields of a live `AdvectedFields`, the call that runs once per HOD
evaluation.  It costs one deposit, one transform and six binnings; nothing belonging to the advected fields is uploaded,
deposited or transformed again, and nothing is read from disk.  `get_recon_power` (the LCV variant) is not built.
"""
import ctypes as C

import numpy as np

from ... import _lib
from ..._lib import DeviceArray, check, ptr
from ...analysis.power_spectrum import _paste_code
from .advect_fields import _bin_pair, _edges, field_growth

__all__ = ['tracer_power']


def tracer_power(tracer_pos, adv, k_bin_edges, mu_bin_edges, poles, D):
    """The reference's `pk_tr_dict`: `k_binc`, `mu_binc`, `P_kmu_tr_tr`, `N_kmu_tr_tr`, `P_ell_tr_tr`, `N_ell_tr_tr` and per field of `adv`
    `P_kmu_{field}_tr`, `N_kmu_{field}_tr`, `P_ell_{field}_tr`, `N_ell_{field}_tr`, the crosses times `field_D[field]`.

    Like the reference (:157-158) this shifts the caller's `tracer_pos` by `Lbox / 2` and wraps it into the box IN PLACE:
    `tracer_pos` ((N, 3) NumPy float32 / float64, positions in [-Lbox/2, Lbox/2), or a float32 DeviceArray) holds the shifted
    positions afterwards.  Paste, compensation and interlacing of the tracer field are those of `adv`."""
    shape = tuple(tracer_pos.shape)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f'tracer_pos must have shape (N, 3), got {shape}')
    if shape[0] < 1:
        raise ValueError('no tracers')
    on_device = isinstance(tracer_pos, DeviceArray)
    if on_device:
        if tracer_pos.dtype != np.float32:
            raise TypeError(f'a DeviceArray of positions must be float32, got {tracer_pos.dtype}')
    elif tracer_pos.dtype not in (np.float32, np.float64):
        raise TypeError(f'tracer_pos must be float32 or float64, got {tracer_pos.dtype}')
    ke, me, pl = _edges(k_bin_edges, mu_bin_edges, poles)
    code = _paste_code(adv.paste, ':')
    L = _lib.lib()
    n = shape[0]
    if adv._tracer is None:          # the tracer's spectrum: allocated with the first call, kept for the next HOD evaluation
        check(L.abacus_zcv_check_memory(adv.nmesh, 1, int(adv.interlaced), C.c_int64(n)))
        adv._tracer = adv._alloc()
    tr = adv._tracer
    if on_device:
        check(L.abacus_zcv_shift_wrap_dev(tracer_pos.ptr, C.c_int64(n), C.c_double(adv.Lbox)))
        pos = tracer_pos
    else:
        tracer_pos += adv.Lbox / 2.0
        tracer_pos %= adv.Lbox
        pos = DeviceArray(np.ascontiguousarray(tracer_pos, dtype=np.float32))
    try:
        check(L.abacus_zcv_spectrum_dev(pos.ptr, C.c_int64(n), None, C.c_double(adv.Lbox), adv.nmesh, code, ptr(adv.W), int(adv.interlaced),
                                        tr.ptr))
        out = {'k_binc': (ke[1:] + ke[:-1]) * 0.5, 'mu_binc': (me[1:] + me[:-1]) * 0.5}      # (reference :84-90)
        P = _bin_pair(adv, tr.ptr, None, ke, me, pl)
        out['P_kmu_tr_tr'], out['N_kmu_tr_tr'], out['P_ell_tr_tr'], out['N_ell_tr_tr'] = P['power'], P['N_mode'], P['binned_poles'], P['N_mode_poles']
        for name in adv.keynames:
            P = _bin_pair(adv, adv._ptr(name), tr.ptr, ke, me, pl)
            g = field_growth(name, D)
            P['power'] *= g
            P['binned_poles'] *= g
            out[f'P_kmu_{name}_tr'], out[f'N_kmu_{name}_tr'] = P['power'], P['N_mode']
            out[f'P_ell_{name}_tr'], out[f'N_ell_{name}_tr'] = P['binned_poles'], P['N_mode_poles']
    finally:
        if not on_device:
            pos.free()
    return out
