"""Array-level form of `abacusnbody.hod.zcv.linear_fields.main` (reference: abacusnbody/hod/zcv/linear_fields.py:29-179) and of
`tools_cv.combine_field_spectra_k3D_lcv` (tools_cv.py:313-335) on the MI355X: the linear control variates (LCV) that reconstructed
catalogues use.  The reference is driven by a YAML file and ASDF files; here the arrays stand in their place:

    lin = linear_fields(delta_lin, Lbox, nmesh)                      # rfftn / n^3 and that times mu^2, one upload, one pass
    pk_lin_dict = linear_power(lin, k_bin_edges, mu_bin_edges, poles)          # the three auto / cross spectra, binned in HBM
    pk_tr_dict = recon_power(tracer_pos, random_pos, lin, ...)       # tracer_power.py, once per HOD evaluation
    pk_tt, pk_ll, pk_lt = combine_field_spectra_k3D_lcv(bias, f_growth, D, lin, nmesh, Lbox, R, rec_algo)

The two spectra ('delta', 'deltamu2'; what `rfftn(delta) / np.float32(nmesh**3)` and `get_delta_mu2` of it return) stay in HBM in a
`LinearFields`, which owns its buffers like an `AdvectedFields`; `recon_power` keeps the tracer's and the randoms' spectrum buffers
there too.  `tools_cv.run_lcv` and `run_lcv_field` stay with the reference and take what is produced here.  There is no CPU fallback.

`combine_field_spectra_k3D_lcv` with `rec_algo='reciso'`: the reference reshapes the `(n, n, n//2+1)` smoothing kernel to
`(n, n, n)` and raises `ValueError`, so that branch HAS NO REFERENCE OUTPUT.  What it evidently means is built: `f_eff = f_growth *
(1 - S)` on the `(n, n, n//2+1)` grid with `S` the reference's own `get_smoothing`.  It is pinned to a NumPy float32 evaluation of
tools_cv.py:326-334 from the reference's `get_smoothing` output and the reference's `P_k3D` arrays (scripts/make_lcv_golden.py).
"""
import ctypes as C

import numpy as np

from ... import _lib
from ..._lib import DeviceArray, check, ptr
from .advect_fields import _bin_pair, _edges

__all__ = ['KEYNAMES', 'LinearFields', 'linear_fields', 'linear_power', 'linear_power3d', 'combine_field_spectra_k3D_lcv']

KEYNAMES = ('delta', 'deltamu2')
REC_ALGOS = ('recsym', 'reciso')


class LinearFields:
    """The spectra of the linear density and of the linear density times mu^2, resident in HBM.  `.spectrum(name)` returns what
    the reference holds in `fields_fft[name]` (complex64 (n, n, n//2+1), NumPy); `.free()` or leaving a `with` block releases the
    memory, the buffers `recon_power` keeps here included.  A freed holder raises `RuntimeError`."""

    def __init__(self, Lbox, nmesh):
        self.Lbox, self.nmesh = float(Lbox), int(nmesh)
        self.keynames = KEYNAMES
        self._spec = {}
        self._tracer = None          # recon_power's tracer (minus randoms) spectrum, reused from call to call
        self._randoms = None         # and the buffer the randoms are transformed into
        self._tracer_valid = False   # a finished tracer spectrum lies in _tracer

    def _alloc(self):
        nb = C.c_uint64(0)
        check(_lib.lib().abacus_zcv_spectrum_bytes(self.nmesh, C.byref(nb)))
        return DeviceArray(nbytes=nb.value, dtype=np.uint8, shape=(nb.value,))

    def _live(self):
        if not self._spec:
            raise RuntimeError('the LinearFields has been freed')

    def _ptr(self, name):
        if name not in self.keynames:
            raise KeyError(f'unknown field {name!r}: a LinearFields holds {self.keynames}')
        self._live()
        return self._spec[name].ptr

    def spectrum(self, name):
        p = self._ptr(name)
        out = np.empty((self.nmesh, self.nmesh, self.nmesh // 2 + 1), dtype=np.complex64)
        check(_lib.lib().abacus_zcv_spectrum_fetch(p, self.nmesh, ptr(out)))
        return out

    def free(self):
        for a in list(self._spec.values()) + [b for b in (self._tracer, self._randoms) if b is not None]:
            a.free()
        self._spec, self._tracer, self._randoms, self._tracer_valid = {}, None, None, False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False


def _check_lin(lin):
    if not isinstance(lin, LinearFields):
        raise TypeError(f'lin must be a LinearFields (what linear_fields returns), got {type(lin).__name__}')
    lin._live()


def linear_fields(delta_lin, Lbox, nmesh):
    """The two linear spectra of reference :108-124.  `delta_lin`: the filtered IC density (what `ic_fields.gaussian_filter`
    returns), a float32 (nmesh, nmesh, nmesh) NumPy array or DeviceArray, not modified; `nmesh` must be even.  One device call:
    padded copy, R2C in place, one pass that normalises by n^3 and writes delta mu^2 beside it.  Returns a `LinearFields`."""
    nmesh = int(nmesh)
    if nmesh < 2 or nmesh % 2:
        raise ValueError(f'nmesh = {nmesh}: the linear fields come from an even mesh (odd sizes are not built, as in ic_fields)')
    shape = tuple(delta_lin.shape)
    if len(shape) != 3 or len(set(shape)) != 1:
        raise ValueError(f'delta_lin must be a cubic 3-D mesh, got shape {shape}')
    if shape[0] != nmesh:
        raise ValueError(f'delta_lin has {shape[0]} cells per side, nmesh = {nmesh}')
    if np.dtype(delta_lin.dtype) != np.float32:
        raise TypeError(f'delta_lin must be float32 (the dtype of the filtered density), got {delta_lin.dtype}')
    Lbox = float(Lbox)
    if not Lbox > 0:
        raise ValueError(f'Lbox must be positive, got {Lbox}')
    lin = LinearFields(Lbox, nmesh)
    on_device = isinstance(delta_lin, DeviceArray)
    src = delta_lin if on_device else DeviceArray(np.ascontiguousarray(delta_lin))
    try:
        for name in KEYNAMES:
            lin._spec[name] = lin._alloc()
        check(_lib.lib().abacus_lcv_linear_dev(src.ptr, nmesh, lin._spec['delta'].ptr, lin._spec['deltamu2'].ptr))
        _lib.sync()
    except Exception:
        lin.free()
        raise
    finally:
        if not on_device:
            src.free()
    return lin


def _pairs():
    return [(a, b) for i, a in enumerate(KEYNAMES) for j, b in enumerate(KEYNAMES) if i >= j]


def linear_power(lin, k_bin_edges, mu_bin_edges, poles):
    """The reference's `pk_lin_dict` (:127-170): `k_binc`, `mu_binc` and `P_kmu_{i}_{j}`, `N_kmu_{i}_{j}`, `P_ell_{i}_{j}`,
    `N_ell_{i}_{j}` for `delta_delta`, `deltamu2_delta`, `deltamu2_deltamu2`.  Shapes as `calc_pk_from_deltak` returns them.  The
    three binnings read the spectra in HBM."""
    ke, me, pl = _edges(k_bin_edges, mu_bin_edges, poles)
    _check_lin(lin)
    out = {'k_binc': (ke[1:] + ke[:-1]) * 0.5, 'mu_binc': (me[1:] + me[:-1]) * 0.5}
    for a, b in _pairs():
        P = _bin_pair(lin, lin._ptr(a), None if a == b else lin._ptr(b), ke, me, pl)
        out[f'P_kmu_{a}_{b}'], out[f'N_kmu_{a}_{b}'] = P['power'], P['N_mode']
        out[f'P_ell_{a}_{b}'], out[f'N_ell_{a}_{b}'] = P['binned_poles'], P['N_mode_poles']
    return out


def _power3d(lin, pa, pb):
    n = lin.nmesh
    out = _lib.pinned_empty((n, n, n // 2 + 1), np.float32)       # page-locked while the pool has room: one DMA, no page faults
    check(_lib.lib().abacus_lcv_power3d(pa, pb, n, ptr(out)))
    return out


def linear_power3d(lin):
    """The `save_3D_power` branch of the reference (:136-155) without the files: `P_k3D_delta_delta`, `P_k3D_deltamu2_delta`,
    `P_k3D_deltamu2_deltamu2`, float32 (n, n, n//2+1) = Re(field_i conj(field_j)), formed and unpadded on the device."""
    _check_lin(lin)
    return {f'P_k3D_{a}_{b}': _power3d(lin, lin._ptr(a), None if a == b else lin._ptr(b)) for a, b in _pairs()}


def combine_field_spectra_k3D_lcv(bias, f_growth, D, lin, nmesh, Lbox, R, rec_algo):
    """The reference's function of that name (tools_cv.py:313-335) with `lin` in place of the two lists of file names: works from
    the spectra in `lin` and the tracer spectrum the latest `recon_power(..., lin, ...)` left there (`RuntimeError` if there is
    none), in one pass over the three spectra instead of six materialised 3-D products.  Returns `(pk_tt, pk_ll, pk_lt)`, float32
    (n, n, n//2+1).  `rec_algo` is 'recsym' (`f_eff = f_growth`) or 'reciso' (`f_eff = f_growth (1 - exp(-k^2 R^2 / 2))` per mode,
    needs `R`).  The reference's 'reciso' branch raises `ValueError` (it reshapes the (n, n, n//2+1) kernel to (n, n, n)): it has
    no reference output and is pinned to a NumPy float32 evaluation of :326-334 from the reference's `get_smoothing` instead."""
    if rec_algo not in REC_ALGOS:
        raise ValueError(f'rec_algo must be one of {REC_ALGOS}, got {rec_algo!r}')
    reciso = rec_algo == 'reciso'
    if reciso:
        if R is None:
            raise ValueError("rec_algo='reciso' needs the smoothing scale R")
        if not float(R) >= 0:
            raise ValueError(f'R must not be negative, got {R}')
    _check_lin(lin)
    if int(nmesh) != lin.nmesh or float(Lbox) != lin.Lbox:
        raise ValueError(f'nmesh = {nmesh}, Lbox = {Lbox}: the LinearFields was made with nmesh = {lin.nmesh}, Lbox = {lin.Lbox}')
    if not lin._tracer_valid:
        raise RuntimeError('no tracer spectrum: call recon_power(tracer_pos, random_pos, lin, ...) first')
    n = lin.nmesh
    pk_tt, pk_ll, pk_lt = (_lib.pinned_empty((n, n, n // 2 + 1), np.float32) for _ in range(3))
    check(_lib.lib().abacus_lcv_combine_k3d(lin._ptr('delta'), lin._ptr('deltamu2'), lin._tracer.ptr, n, C.c_double(lin.Lbox),
                                           C.c_double(float(bias)), C.c_double(float(f_growth)), C.c_double(float(D)),
                                           C.c_double(float(R) if reciso else 0.0), int(reciso), ptr(pk_tt), ptr(pk_ll), ptr(pk_lt)))
    return pk_tt, pk_ll, pk_lt
