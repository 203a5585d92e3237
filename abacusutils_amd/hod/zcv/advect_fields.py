"""Array-level form of `abacusnbody.hod.zcv.advect_fields.main` (reference: abacusnbody/hod/zcv/advect_fields.py:166-370) on the
MI355X.  The reference is driven by a YAML file, ASDF files and `classy`; here the arrays and numbers stand in their place (the
growth factor `D` and the growth rate `f_growth` are arguments):

    adv = advect(disp, fields, Lbox, nmesh, D)            # lattice advection + one weighted deposit + transform per field
    pk_ij_dict = field_power(adv, k_bin_edges, mu_bin_edges, poles, D)      # the 15 auto / cross spectra, binned in HBM

One particle per lattice site is moved by the Zel'dovich displacement (positions generated on the device, never on the host) and
deposited once per field with that field's mesh as the weights, used where they lie.  The finished spectra (interlacing combined,
compensated: what `get_field_fft` returns) stay in HBM in an `AdvectedFields`, which owns its buffers: `calc_power_multi` /
`AbacusHOD.compute_power` and a live `AdvectedFields` do not touch each other's memory.  There is no CPU fallback.
"""
import ctypes as C

import numpy as np

from ... import _lib
from ..._lib import DeviceArray, check, ptr
from ...analysis.power_spectrum import _alloc_outputs, _pack, _paste_code, get_W_compensated

__all__ = ['KEYNAMES', 'FIELD_GROWTH_POWER', 'lattice_positions', 'advect', 'field_power', 'AdvectedFields']

KEYNAMES = ('1cb', 'delta', 'delta2', 'tidal2', 'nabla2')
# field_D = [1, D, D^2, D^2, D] of the reference (:177), by field NAME (the reference indexes by position in keynames)
FIELD_GROWTH_POWER = {'1cb': 0, 'delta': 1, 'delta2': 2, 'tidal2': 2, 'nabla2': 1}


def field_growth(name, D):
    return float(D) ** FIELD_GROWTH_POWER[name]


def _disp_meshes(disp_x, disp_y, disp_z):
    """checks made before the library is loaded; returns the mesh size"""
    n = None
    for name, a in (('disp_x', disp_x), ('disp_y', disp_y), ('disp_z', disp_z)):
        shape = tuple(a.shape)
        if len(shape) != 3 or len(set(shape)) != 1:
            raise ValueError(f'{name} must be a cubic 3-D mesh, got shape {shape}')
        if n is not None and shape[0] != n:
            raise ValueError(f'{name} has {shape[0]} cells per side, the others {n}')
        n = shape[0]
        if isinstance(a, DeviceArray):
            if a.dtype != np.float32:
                raise TypeError(f'a DeviceArray mesh must be float32, got {a.dtype}')
        elif np.dtype(a.dtype) != np.float32:
            raise TypeError(f'{name} must be float32 (the dtype of the filtered displacements), got {a.dtype}')
    return n


def _up(a):
    if isinstance(a, DeviceArray):
        return a, False
    return DeviceArray(np.ascontiguousarray(a, dtype=np.float32)), True


def lattice_positions(disp_x, disp_y, disp_z, Lbox, D, f_growth=0.0, device_out=False):
    """The (n^3, 3) float32 positions of one particle per lattice site moved by the displacement (box units) times `D`, the z
    component also times `1 + f_growth` (reference :213-239), operation by operation in float32: bit-equal to the NumPy recipe.
    The wrap is NumPy's `%`: a position can equal `Lbox` (the deposit's own wrap handles that)."""
    n = _disp_meshes(disp_x, disp_y, disp_z)
    Lbox = float(Lbox)
    if not Lbox > 0:
        raise ValueError(f'Lbox must be positive, got {Lbox}')
    dev = [_up(a) for a in (disp_x, disp_y, disp_z)]
    pos = DeviceArray(nbytes=12 * n ** 3, dtype=np.float32, shape=(n ** 3, 3))
    check(_lib.lib().abacus_zcv_lattice_dev(dev[0][0].ptr, dev[1][0].ptr, dev[2][0].ptr, n, C.c_double(Lbox), C.c_double(float(D)),
                                            C.c_double(float(f_growth)), pos.ptr))
    _lib.sync()
    for a, owned in dev:
        if owned:
            a.free()
    if device_out:
        return pos
    res = pos.get()
    pos.free()
    return res


class AdvectedFields:
    """The finished spectra of the advected fields, one per name, resident in HBM.  `.spectrum(name)` returns what the reference's
    `get_field_fft(disp_pos, Lbox, nmesh, paste, w, W, compensated, interlaced)` returns (complex64 (n, n, n//2+1), NumPy);
    `.free()` or leaving a `with` block releases the memory."""

    def __init__(self, Lbox, nmesh, paste, compensated, interlaced, keynames):
        self.Lbox, self.nmesh = float(Lbox), int(nmesh)
        self.paste, self.compensated, self.interlaced = paste.upper(), bool(compensated), bool(interlaced)
        self.keynames = tuple(keynames)
        self.W = get_W_compensated(self.Lbox, self.nmesh, self.paste, self.interlaced).astype(np.float32) if self.compensated else None
        self._spec = {}
        self._tracer = None          # tracer_power's spectrum buffer, reused from call to call

    def _alloc(self):
        nb = C.c_uint64(0)
        check(_lib.lib().abacus_zcv_spectrum_bytes(self.nmesh, C.byref(nb)))
        return DeviceArray(nbytes=nb.value, dtype=np.uint8, shape=(nb.value,))

    def _ptr(self, name):
        if name not in self._spec:
            if name in self.keynames:
                raise RuntimeError('the AdvectedFields has been freed')
            raise KeyError(f'unknown field {name!r}: this AdvectedFields holds {self.keynames}')
        return self._spec[name].ptr

    def spectrum(self, name):
        out = np.empty((self.nmesh, self.nmesh, self.nmesh // 2 + 1), dtype=np.complex64)
        check(_lib.lib().abacus_zcv_spectrum_fetch(self._ptr(name), self.nmesh, ptr(out)))
        return out

    def free(self):
        for a in list(self._spec.values()) + ([self._tracer] if self._tracer is not None else []):
            a.free()
        self._spec, self._tracer = {}, None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False


def advect(disp, fields, Lbox, nmesh, D, f_growth=0.0, paste='TSC', compensated=True, interlaced=True, keynames=KEYNAMES):
    """Advects the fields (reference :208-285).  `disp`: the three displacement meshes in box units (what `ic_fields.load_disp`
    returns, after `gaussian_filter`); `fields`: {name: weight mesh} for every name in `keynames` but '1cb', which is unweighted.
    float32 NumPy arrays or DeviceArrays, none modified.  Returns an `AdvectedFields`."""
    nmesh = int(nmesh)
    if nmesh < 2 or nmesh % 2:
        raise ValueError(f'nmesh = {nmesh}: the fields come from get_fields, which needs an even mesh (the reference fails on odd sizes)')
    if len(disp) != 3:
        raise ValueError('disp must hold the three displacement meshes (x, y, z)')
    n = _disp_meshes(*disp)
    if n != nmesh:
        raise ValueError(f'the displacement meshes have {n} cells per side, nmesh = {nmesh}')
    keynames = tuple(keynames)
    if not keynames or len(set(keynames)) != len(keynames):
        raise ValueError('keynames must be distinct field names')
    for name in keynames:
        if name not in FIELD_GROWTH_POWER:
            raise KeyError(f'unknown field {name!r}: known fields are {KEYNAMES}')
        if name != '1cb':
            if name not in fields:
                raise KeyError(f'no weight mesh for field {name!r}')
            w = fields[name]
            if tuple(w.shape) != (nmesh,) * 3:
                raise ValueError(f'the weight mesh of {name!r} has shape {tuple(w.shape)}, nmesh = {nmesh}')
            if w.dtype != np.float32:
                raise TypeError(f'the weight mesh of {name!r} must be float32, got {w.dtype}')
    Lbox = float(Lbox)
    if not Lbox > 0:
        raise ValueError(f'Lbox must be positive, got {Lbox}')
    code = _paste_code(paste, ':')
    adv = AdvectedFields(Lbox, nmesh, paste, compensated, interlaced, keynames)
    L = _lib.lib()
    dev, wdev = [], {}
    try:
        dev = [_up(a) for a in disp]
        wdev = {name: _up(fields[name]) for name in keynames if name != '1cb'}
        # (after the uploads of NumPy inputs: the check then sees what they took)
        check(L.abacus_zcv_check_memory(nmesh, len(keynames), int(adv.interlaced), C.c_int64(0)))
        for name in keynames:
            adv._spec[name] = adv._alloc()
        nf = len(keynames)
        wptrs = (C.c_void_p * nf)(*[None if name == '1cb' else wdev[name][0].ptr.value for name in keynames])
        optrs = (C.c_void_p * nf)(*[adv._spec[name].ptr.value for name in keynames])
        check(L.abacus_zcv_advect_dev(dev[0][0].ptr, dev[1][0].ptr, dev[2][0].ptr, nmesh, C.c_double(Lbox), C.c_double(float(D)),
                                      C.c_double(float(f_growth)), nf, wptrs, code, ptr(adv.W), int(adv.interlaced), optrs))
        _lib.sync()
    except Exception:
        adv.free()
        raise
    finally:
        for a, owned in list(dev) + list(wdev.values()):
            if owned:
                a.free()
    return adv


def _bin_pair(adv, pa, pb, ke, me, pl):
    outs = _alloc_outputs(len(ke) - 1, len(me) - 1, len(pl))
    check(_lib.lib().abacus_zcv_power_pair(pa, pb, adv.nmesh, C.c_double(adv.Lbox), ptr(ke), len(ke) - 1, ptr(me), len(me) - 1, ptr(pl),
                                           len(pl), *[ptr(o) for o in outs]))
    return _pack(*outs, me, True)


def _edges(k_bin_edges, mu_bin_edges, poles):
    ke = np.ascontiguousarray(k_bin_edges, dtype=np.float64)
    me = np.ascontiguousarray(mu_bin_edges, dtype=np.float64)
    pl = np.ascontiguousarray(poles, dtype=np.int64)
    if ke.ndim != 1 or len(ke) < 2 or me.ndim != 1 or len(me) < 2:
        raise ValueError('k_bin_edges and mu_bin_edges must hold at least two edges each')
    return ke, me, pl


def field_power(adv, k_bin_edges, mu_bin_edges, poles, D):
    """The reference's `pk_ij_dict` (:288-370): `k_binc`, `mu_binc` and for every pair i >= j in `adv.keynames` order
    `P_kmu_{i}_{j}`, `N_kmu_{i}_{j}`, `P_ell_{i}_{j}`, `N_ell_{i}_{j}`, the P's times `field_D[i] * field_D[j]` with
    `field_D = [1, D, D^2, D^2, D]` looked up by field name.  Shapes as `calc_pk_from_deltak` returns them.  All binnings read the
    spectra in HBM."""
    ke, me, pl = _edges(k_bin_edges, mu_bin_edges, poles)
    out = {'k_binc': (ke[1:] + ke[:-1]) * 0.5, 'mu_binc': (me[1:] + me[:-1]) * 0.5}
    names = adv.keynames
    for i, ni in enumerate(names):
        for j, nj in enumerate(names):
            if i < j:
                continue
            P = _bin_pair(adv, adv._ptr(ni), None if i == j else adv._ptr(nj), ke, me, pl)
            g = field_growth(ni, D) * field_growth(nj, D)
            P['power'] *= g
            P['binned_poles'] *= g
            out[f'P_kmu_{ni}_{nj}'] = P['power']
            out[f'N_kmu_{ni}_{nj}'] = P['N_mode']
            out[f'P_ell_{ni}_{nj}'] = P['binned_poles']
            out[f'N_ell_{ni}_{nj}'] = P['N_mode_poles']
    return out
