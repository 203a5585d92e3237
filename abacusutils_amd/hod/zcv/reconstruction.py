"""BAO reconstruction on the MI355X: the step between `run_hod` and `tracer_power.recon_power`.  The reference has none - its
`get_recon_power` takes reconstructed tracers and shifted randoms that an external CPU code produced - so the per-evaluation chain
`run_hod -> reconstruct -> recon_power -> run_lcv` left the device exactly here.  Standard plane-parallel reconstruction of a
periodic box (line of sight = z) is a closed-form Fourier solve, with the conventions `tools_cv.combine_kaiser_spectra` assumes
(Chen et al. 2019: RecSym and RecIso, Gaussian smoothing S = exp(-k^2 R^2 / 2), bias b, growth rate f):

    disp = displacement_field(tracer_pos, Lbox, nmesh, bias, f_growth, R)         # deposit, R2C, one multiplier pass, three C2R
    tracer_rec = shift(tracer_pos, disp)                                          # s - psi - f psi_z z^
    random_rec = shift(random_pos, disp, los_factor=0.0)                          # RecIso randoms: s - psi
    tracer_rec, random_rec = reconstruct(tracer_pos, random_pos, Lbox, nmesh, bias, f_growth, R, rec_algo='recsym')

1. delta(k) of the tracers: the deposit of `analysis.power_spectrum` (`paste` 'CIC' or 'TSC', no compensation, no interlacing),
   rho n^3 / N - 1, R2C, / n^3.
2. psi_i(k) = i k_i S(k) delta(k) / (k^2 b (1 + beta mu^2)), beta = f / b with `rsd` else 0, mu^2 = k_z^2 / k^2, 0 for the zero
   vector; wavenumbers dk = float32(2 pi / L), index i -> i below n/2, i - n from n/2 on (x, y), 0 .. n/2 on z.  In the factor i k_i
   only, the wavenumber of axis i is 0 at index n/2 of that axis: the three spectra are Hermitian as written.
3. Three inverse transforms give psi_x, psi_y, psi_z, float32 meshes that stay in HBM (a `Displacement`).
4. psi is read at a particle (position modulo L) with the same cloud as the deposit - cell i centred at i L / n, the nearest cell by
   rounding, periodic indices - and the particle moves to s - psi - f_z psi_z z^, wrapped into [0, L) with NumPy's float32 remainder.

Positions are (N, 3) NumPy float32 / float64 (not modified; float64 is deposited and shifted as float32; NumPy float32 comes back),
an (N, 3) float32 `DeviceArray` (not modified: the deposit works on a copy; a new `DeviceArray` comes back) or three float64
`DeviceArray` columns as `MockDict.device_xyz(tracer)` returns them (a `DeviceArray` comes back): the chain then never leaves HBM.
`offset` is added before anything else; mock coordinates in [-L/2, L/2) use `offset=Lbox / 2`, `tracer_power`'s convention.  There is
no CPU fallback.  tests/recon_statement.py states the four steps in NumPy float64; the device is held to four times the float32
noise of that statement.
"""
import ctypes as C

import numpy as np

from ... import _lib
from ..._lib import DeviceArray, check
from ...analysis.power_spectrum import _paste_code

__all__ = ['REC_ALGOS', 'Displacement', 'displacement_field', 'displacement_from_delta', 'shift', 'reconstruct']

REC_ALGOS = ('recsym', 'reciso')


# ------------------------------------------------------------------------------------------------- checks made before the library loads
def _columns(pos):
    return isinstance(pos, (tuple, list)) and len(pos) == 3 and all(isinstance(c, DeviceArray) for c in pos)


def _positions(pos, name):
    """checks made before the library is loaded; returns the number of particles"""
    if _columns(pos):
        shapes = [tuple(c.shape) for c in pos]
        if any(len(s) != 1 for s in shapes) or len(set(shapes)) != 1:
            raise ValueError(f'{name}: the three columns must have one shape (N,), got {shapes}')
        if any(c.dtype != np.float64 for c in pos):
            raise TypeError(f'{name}: three DeviceArray columns must be float64, got {[str(c.dtype) for c in pos]}')
        if shapes[0][0] < 1:
            raise ValueError(f'{name} holds no particles')
        return shapes[0][0]
    if not hasattr(pos, 'shape') or not hasattr(pos, 'dtype'):
        raise TypeError(f'{name} must be an (N, 3) array, an (N, 3) float32 DeviceArray or three float64 DeviceArray columns, '
                        f'got {type(pos).__name__}')
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


def _box(Lbox):
    Lbox = float(Lbox)
    if not (Lbox > 0 and np.isfinite(Lbox)):
        raise ValueError(f'Lbox must be positive, got {Lbox}')
    return Lbox


def _nmesh(nmesh):
    nmesh = int(nmesh)
    if nmesh < 2 or nmesh % 2 or nmesh > 32767:
        raise ValueError(f'nmesh = {nmesh}: the displacement comes from an even mesh of 2 .. 32766 cells per side (odd sizes are not built)')
    return nmesh


def _model(bias, f_growth, R):
    bias, f_growth, R = float(bias), float(f_growth), float(R)
    if not (bias > 0 and np.isfinite(bias)):
        raise ValueError(f'bias must be positive, got {bias}')
    if not (f_growth >= 0 and np.isfinite(f_growth)):
        raise ValueError(f'f_growth must not be negative, got {f_growth}')
    if not (R >= 0 and np.isfinite(R)):
        raise ValueError(f'R must not be negative, got {R} (0: no smoothing)')
    return bias, f_growth, R


def _offset(offset):
    offset = float(offset)
    if not np.isfinite(offset):
        raise ValueError(f'offset must be finite, got {offset}')
    return offset


def _cubic(mesh, name, nmesh=None):
    shape = tuple(mesh.shape)
    if len(shape) != 3 or len(set(shape)) != 1:
        raise ValueError(f'{name} must be a cubic 3-D mesh, got shape {shape}')
    if nmesh is not None and shape[0] != nmesh:
        raise ValueError(f'{name} has {shape[0]} cells per side, nmesh = {nmesh}')
    if np.dtype(mesh.dtype) != np.float32:
        raise TypeError(f'{name} must be float32, got {mesh.dtype}')
    return _nmesh(shape[0])


# ------------------------------------------------------------------------------------------------- the field
class Displacement:
    """The three components of the displacement field, float32 meshes resident in HBM in the padded layout the inverse transform
    leaves them in.  Attributes `nmesh`, `Lbox`, `paste` (the cloud `shift` reads it with), `f_growth`, `rsd`.  `.fetch()` returns
    float32 (3, n, n, n); `.free()` or leaving a `with` block releases the memory.  A freed holder raises `RuntimeError`."""

    def __init__(self, Lbox, nmesh, paste, f_growth, rsd):
        self.Lbox, self.nmesh, self.paste = float(Lbox), int(nmesh), str(paste).upper()
        self.f_growth, self.rsd = float(f_growth), bool(rsd)
        self._psi = []

    def _alloc(self):
        nb = C.c_uint64(0)
        check(_lib.lib().abacus_zcv_spectrum_bytes(self.nmesh, C.byref(nb)))
        self._psi = [DeviceArray(nbytes=nb.value, dtype=np.uint8, shape=(nb.value,)) for _ in range(3)]

    def _live(self):
        if not self._psi:
            raise RuntimeError('the Displacement has been freed')

    def _ptrs(self):
        self._live()
        return [a.ptr for a in self._psi]

    @classmethod
    def from_meshes(cls, psi_x, psi_y, psi_z, Lbox, paste, f_growth, rsd):
        """wraps three caller meshes ((n, n, n) float32 NumPy arrays or DeviceArrays, copied, not modified): for tests and for a
        solver of the caller's own"""
        meshes = (psi_x, psi_y, psi_z)
        n = _cubic(psi_x, 'psi_x')
        for m, name in zip(meshes[1:], ('psi_y', 'psi_z')):
            _cubic(m, name, n)
        Lbox = _box(Lbox)
        _paste_code(paste, ':')
        f_growth = _model(1.0, f_growth, 0.0)[1]
        self = cls(Lbox, n, paste, f_growth, rsd)
        try:
            self._alloc()
            for m, dst in zip(meshes, self._psi):
                on_device = isinstance(m, DeviceArray)
                src = m if on_device else DeviceArray(np.ascontiguousarray(m))
                try:
                    check(_lib.lib().abacus_recon_pad_dev(src.ptr, n, dst.ptr))
                    _lib.sync()
                finally:
                    if not on_device:
                        src.free()
        except Exception:
            self.free()
            raise
        return self

    def fetch(self):
        n = self.nmesh
        out = np.empty((3, n, n, n), dtype=np.float32)
        row = np.empty((n, n, n // 2 + 1), dtype=np.complex64)      # a padded row as n + 2 floats, the first n of them the mesh
        for q, p in enumerate(self._ptrs()):
            check(_lib.lib().abacus_zcv_spectrum_fetch(p, n, _lib.ptr(row)))
            out[q] = row.view(np.float32)[:, :, :n]
        return out

    def free(self):
        for a in self._psi:
            a.free()
        self._psi = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False


def _check_disp(disp):
    if not isinstance(disp, Displacement):
        raise TypeError(f'disp must be a Displacement (what displacement_field returns), got {type(disp).__name__}')
    disp._live()


def _working_copy(pos, n, offset, Lbox):
    """a new (n, 3) float32 DeviceArray = (pos + offset) % Lbox, what the deposit may wrap and sort as it likes"""
    L = _lib.lib()
    out = DeviceArray(nbytes=12 * n, dtype=np.float32, shape=(n, 3))
    try:
        if _columns(pos):
            check(L.abacus_recon_pack_soa64_dev(pos[0].ptr, pos[1].ptr, pos[2].ptr, C.c_int64(n), C.c_double(offset), out.ptr))
            check(L.abacus_recon_wrap_dev(out.ptr, C.c_int64(n), C.c_double(0.0), C.c_double(Lbox), out.ptr))
        elif isinstance(pos, DeviceArray):
            check(L.abacus_recon_wrap_dev(pos.ptr, C.c_int64(n), C.c_double(offset), C.c_double(Lbox), out.ptr))
        else:
            out.set(np.ascontiguousarray(pos, dtype=np.float32))
            check(L.abacus_recon_wrap_dev(out.ptr, C.c_int64(n), C.c_double(offset), C.c_double(Lbox), out.ptr))
    except Exception:
        out.free()
        raise
    return out


def _solve(disp, delta_ptr, normalised, bias, f_growth, R):
    px, py, pz = disp._ptrs()
    check(_lib.lib().abacus_recon_displacement_dev(delta_ptr, int(normalised), disp.nmesh, C.c_double(disp.Lbox), C.c_double(bias),
                                                   C.c_double(f_growth), C.c_double(R), int(disp.rsd), px, py, pz))


def displacement_field(tracer_pos, Lbox, nmesh, bias, f_growth, R, rsd=True, paste='CIC', offset=0.0):
    """Steps 1 to 3 of the module docstring from tracer positions: one deposit + R2C (on a wrapped copy of the positions), one pass
    that writes the three displacement spectra, three C2R.  `R` is the Gaussian smoothing scale in the units of `Lbox` (0: none).
    Returns a `Displacement`; it holds three padded meshes, a fourth (the deposit's work mesh) is needed while it is made."""
    n = _positions(tracer_pos, 'tracer_pos')
    Lbox, nmesh = _box(Lbox), _nmesh(nmesh)
    bias, f_growth, R = _model(bias, f_growth, R)
    code = _paste_code(paste, ':')
    offset = _offset(offset)
    L = _lib.lib()
    check(L.abacus_recon_check_memory(nmesh, C.c_int64(n)))
    disp = Displacement(Lbox, nmesh, paste, f_growth, rsd)
    work = None
    try:
        disp._alloc()
        work = _working_copy(tracer_pos, n, offset, Lbox)
        spec = disp._psi[2].ptr                  # delta(k) lies in the third mesh; the multiplier pass reads every mode before it writes it
        check(L.abacus_zcv_spectrum_dev(work.ptr, C.c_int64(n), None, C.c_double(Lbox), nmesh, code, None, 0, spec))
        _solve(disp, spec, True, bias, f_growth, R)
        _lib.sync()
    except Exception:
        disp.free()
        raise
    finally:
        if work is not None:
            work.free()
    return disp


def displacement_from_delta(delta, Lbox, bias, f_growth, R, rsd=True, paste='CIC'):
    """Steps 2 and 3 from a given density contrast: `delta` is an (n, n, n) float32 NumPy array or `DeviceArray`, not modified.
    `paste` is only the cloud `shift` reads the field with.  Returns a `Displacement`."""
    nmesh = _cubic(delta, 'delta')
    Lbox = _box(Lbox)
    bias, f_growth, R = _model(bias, f_growth, R)
    _paste_code(paste, ':')
    L = _lib.lib()
    check(L.abacus_recon_check_memory(nmesh, C.c_int64(0)))
    disp = Displacement(Lbox, nmesh, paste, f_growth, rsd)
    on_device = isinstance(delta, DeviceArray)
    src = None
    try:
        disp._alloc()
        src = delta if on_device else DeviceArray(np.ascontiguousarray(delta))
        spec = disp._psi[2].ptr
        check(L.abacus_recon_delta_dev(src.ptr, nmesh, spec))
        _solve(disp, spec, False, bias, f_growth, R)             # a bare R2C: 1 / n^3 rides in the multiplier
        _lib.sync()
    except Exception:
        disp.free()
        raise
    finally:
        if src is not None and not on_device:
            src.free()
    return disp


def _los(disp, los_factor):
    if los_factor is None:
        return disp.f_growth if disp.rsd else 0.0
    los_factor = float(los_factor)
    if not np.isfinite(los_factor):
        raise ValueError(f'los_factor must be finite, got {los_factor}')
    return los_factor


def shift(pos, disp, los_factor=None, offset=0.0):
    """Step 4: `(s - psi(s) - los_factor psi_z(s) z^) % Lbox` with `s = (pos + offset) % Lbox`, psi read with the cloud `disp.paste`.
    `los_factor=None` means `disp.f_growth` if `disp.rsd` else 0 (tracers, RecSym randoms); RecIso randoms take 0.  One kernel, one
    lane per particle, a gather from the three meshes.  The rate depends on the order of the particles: catalogues in halo order or
    sorted by cell share their mesh rows.  Fixed randoms used for many evaluations are worth sorting once by their (x, y) cell row
    (`np.lexsort` of the cell indices) before the first call: the result does not depend on the order, the time does (at 576^3,
    5 x 10^6 randoms: 1.5 ms in random order, 0.8 ms sorted; profiles/recon/README.md).  Returns NumPy float32 for NumPy input, a new
    float32 `DeviceArray` otherwise; `pos` is not modified."""
    n = _positions(pos, 'pos')
    _check_disp(disp)
    los = _los(disp, los_factor)
    offset = _offset(offset)
    code = _paste_code(disp.paste, ':')
    L = _lib.lib()
    host = not _columns(pos) and not isinstance(pos, DeviceArray)
    src = out = None
    own = True
    try:
        if _columns(pos):
            src = DeviceArray(nbytes=12 * n, dtype=np.float32, shape=(n, 3))
            check(L.abacus_recon_pack_soa64_dev(pos[0].ptr, pos[1].ptr, pos[2].ptr, C.c_int64(n), C.c_double(offset), src.ptr))
            offset = 0.0
        elif host:
            src = DeviceArray(np.ascontiguousarray(pos, dtype=np.float32))
        else:
            src, own = pos, False
        out = DeviceArray(nbytes=12 * n, dtype=np.float32, shape=(n, 3))
        px, py, pz = disp._ptrs()
        check(L.abacus_recon_shift_dev(src.ptr, C.c_int64(n), C.c_double(offset), px, py, pz, disp.nmesh, C.c_double(disp.Lbox), code,
                                       C.c_double(los), out.ptr))
        if not host:
            _lib.sync()
            res, out = out, None
            return res
        return out.get()
    finally:
        if own and src is not None:
            src.free()
        if out is not None:
            out.free()


def reconstruct(tracer_pos, random_pos, Lbox, nmesh, bias, f_growth, R, rec_algo='recsym', rsd=True, paste='CIC', offset=0.0):
    """One displacement field from the tracers and two shifts: returns `(tracer_rec, random_rec)`, what `recon_power` takes.
    Tracers move to `s - psi - f_z psi_z z^` (`f_z = f_growth` with `rsd`, else 0); randoms the same under `rec_algo='recsym'`, to
    `s - psi` under 'reciso'.  `random_pos=None` returns `(tracer_rec, None)`.  Host tracers are uploaded once.  The three inverse
    transforms bound the call (6.5 of 13 ms at 576^3); the read-out of unsorted randoms is a fifth of the transforms - sorting fixed
    randoms once still saves its half, see `shift`."""
    n = _positions(tracer_pos, 'tracer_pos')
    if random_pos is not None:
        _positions(random_pos, 'random_pos')
    if rec_algo not in REC_ALGOS:
        raise ValueError(f'rec_algo must be one of {REC_ALGOS}, got {rec_algo!r}')
    Lbox, nmesh = _box(Lbox), _nmesh(nmesh)
    bias, f_growth, R = _model(bias, f_growth, R)
    _paste_code(paste, ':')
    offset = _offset(offset)
    host = not _columns(tracer_pos) and not isinstance(tracer_pos, DeviceArray)
    tr = DeviceArray(np.ascontiguousarray(tracer_pos, dtype=np.float32)) if host else tracer_pos
    try:
        with displacement_field(tr, Lbox, nmesh, bias, f_growth, R, rsd=rsd, paste=paste, offset=offset) as disp:
            tracer_rec = shift(tr, disp, None, offset)
            if host:
                dev, tracer_rec = tracer_rec, tracer_rec.get()
                dev.free()
            random_rec = None
            if random_pos is not None:
                random_rec = shift(random_pos, disp, None if rec_algo == 'recsym' else 0.0, offset)
    finally:
        if host:
            tr.free()
    return tracer_rec, random_rec
