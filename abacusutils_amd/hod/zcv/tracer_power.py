"""Array-level form of `abacusnbody.hod.zcv.tracer_power.get_tracer_power` (reference: abacusnbody/hod/zcv/tracer_power.py:155-286)
on the MI355X: the tracer field against the advected fields of a live `AdvectedFields`, the call that runs once per HOD
evaluation.  It costs one deposit, one transform and six binnings; nothing belonging to the advected fields is uploaded,
deposited or transformed again, and nothing is read from disk.

`recon_power` is the array-level form of the LCV variant `get_recon_power` (:289-544) for reconstructed catalogues: the tracer
field minus the randoms' field against the two linear spectra of a live `LinearFields` (linear_fields.py).
"""
import ctypes as C

import numpy as np

from ... import _lib
from ..._lib import DeviceArray, check, ptr
from ...analysis.power_spectrum import _paste_code, get_W_compensated
from .advect_fields import _bin_pair, _edges, field_growth
from .linear_fields import _check_lin, _power3d

__all__ = ['tracer_power', 'recon_power']


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


def _positions(pos, name):
    """checks made before the library is loaded; returns the number of particles"""
    shape = tuple(pos.shape)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f'{name} must have shape (N, 3), got {shape}')
    if shape[0] < 1:
        raise ValueError(f'{name} holds no particles')
    if isinstance(pos, DeviceArray):
        if pos.dtype != np.float32:
            raise TypeError(f'a DeviceArray of positions must be float32, got {pos.dtype}')
    elif pos.dtype not in (np.float32, np.float64):
        raise TypeError(f'{name} must be float32 or float64, got {pos.dtype}')
    return shape[0]


def recon_power(tracer_pos, random_pos, lin, k_bin_edges, mu_bin_edges, poles, paste='TSC', compensated=True, interlaced=True,
                save_3D_power=False):
    """The reference's `get_recon_power` (:396-532) on arrays: the field of the reconstructed tracers minus that of the shifted
    randoms (`random_pos=None` skips the subtraction) against the spectra of `lin`, a live `LinearFields`.  It costs two deposits,
    two transforms, one subtraction and three binnings, all in HBM; the tracer and randoms spectrum buffers are allocated with the
    first call and kept on `lin` (`lin.free()` releases them), and the finished tracer spectrum stays there for
    `combine_field_spectra_k3D_lcv`.

    Positions are (N, 3) in box coordinates and are NOT shifted by `Lbox / 2` (unlike `tracer_power`); reconstruction may leave
    them a few cells outside [0, Lbox), the deposit wraps them.  `reconstruction.reconstruct` produces both sets in HBM (it wraps them
    into the box); an external reconstruction's output is taken as well.  NumPy inputs (float32 or float64, deposited as float32) are not
    modified.  `DeviceArray` inputs must be float32 and may be wrapped into the box IN PLACE by the TSC deposit, as the
    reference's `tsc_parallel` wraps its argument.

    Returns the reference's `pk_tr_dict`: `k_binc`, `mu_binc` and `P_kmu_*`, `N_kmu_*`, `P_ell_*`, `N_ell_*` for `tr_tr`,
    `delta_tr`, `deltamu2_tr`; with `save_3D_power=True` the products the reference writes to files instead: `P_k3D_tr_tr`,
    `P_k3D_delta_tr`, `P_k3D_deltamu2_tr`, float32 (n, n, n//2+1)."""
    n_tr = _positions(tracer_pos, 'tracer_pos')
    n_rn = None if random_pos is None else _positions(random_pos, 'random_pos')
    ke, me, pl = _edges(k_bin_edges, mu_bin_edges, poles)
    code = _paste_code(paste, ':')
    _check_lin(lin)
    W = get_W_compensated(lin.Lbox, lin.nmesh, paste, bool(interlaced)).astype(np.float32) if compensated else None
    L = _lib.lib()
    if lin._tracer is None:
        check(L.abacus_zcv_check_memory(lin.nmesh, 1 if n_rn is None else 2, int(bool(interlaced)), C.c_int64(max(n_tr, n_rn or 0))))
        lin._tracer = lin._alloc()
    if n_rn is not None and lin._randoms is None:
        lin._randoms = lin._alloc()
    lin._tracer_valid = False

    def spectrum(pos, n, dest):
        on_device = isinstance(pos, DeviceArray)
        dev = pos if on_device else DeviceArray(np.ascontiguousarray(pos, dtype=np.float32))
        try:
            check(L.abacus_zcv_spectrum_dev(dev.ptr, C.c_int64(n), None, C.c_double(lin.Lbox), lin.nmesh, code, ptr(W), int(bool(interlaced)),
                                            dest.ptr))
        finally:
            if not on_device:
                dev.free()

    tr = lin._tracer
    spectrum(tracer_pos, n_tr, tr)
    if n_rn is not None:
        spectrum(random_pos, n_rn, lin._randoms)
        check(L.abacus_lcv_spectrum_sub_dev(tr.ptr, lin._randoms.ptr, lin.nmesh))
    lin._tracer_valid = True
    if save_3D_power:
        out = {'P_k3D_tr_tr': _power3d(lin, tr.ptr, None)}
        for name in lin.keynames:
            out[f'P_k3D_{name}_tr'] = _power3d(lin, lin._ptr(name), tr.ptr)
        return out
    out = {'k_binc': (ke[1:] + ke[:-1]) * 0.5, 'mu_binc': (me[1:] + me[:-1]) * 0.5}
    P = _bin_pair(lin, tr.ptr, None, ke, me, pl)
    out['P_kmu_tr_tr'], out['N_kmu_tr_tr'], out['P_ell_tr_tr'], out['N_ell_tr_tr'] = P['power'], P['N_mode'], P['binned_poles'], P['N_mode_poles']
    for name in lin.keynames:
        P = _bin_pair(lin, lin._ptr(name), tr.ptr, ke, me, pl)
        out[f'P_kmu_{name}_tr'], out[f'N_kmu_{name}_tr'] = P['power'], P['N_mode']
        out[f'P_ell_{name}_tr'], out[f'N_ell_{name}_tr'] = P['binned_poles'], P['N_mode_poles']
    return out
