"""Power spectrum multipoles of light-cone catalogues on the MI355X: the Fourier half of the light-cone interface, beside the
Landy-Szalay functions of `tpcf_corrfunc` (`calc_xirppi_lc`, `calc_wp_lc`, `calc_multipole_lc`).  The reference's `calc_power` assumes a
periodic box and a global line of sight; no reference code stands behind this module - its arithmetic is stated in
include/abacus_hip.h and pinned to the NumPy statement tests/lc_power_statement.py.

Estimator: Feldman, Kaiser & Peacock 1994 with the end-point line of sight of Yamamoto et al. 2006, evaluated with the
spherical-harmonic decomposition of Hand et al. 2017 (1 + 5 + 9 transforms for l = 0, 2, 4):

1. Box.  Samples are observer-centred float32 columns in HBM (`_LCSample`).  The randoms fix the box: with lo_i, hi_i their extent per
   axis, L = boxpad max_i(hi_i - lo_i) (or `Lbox`) and corner c_i = float32((lo_i + hi_i) / 2 - L / 2); positions in the box are the
   float32 differences s = r - c.  A point, data or randoms, closer than two cells to a face raises ValueError (the deposit wraps).
2. F = D_a - alpha_a R: raw weighted deposits (weight per cell, TSC or CIC), alpha_a = W_a / W_r.  R is deposited once per
   (nmesh, L, corner, paste) and kept by the `LCRandoms` (`mesh_built` counts the deposits); per call only the data are deposited.
3. F_0 = rfftn(F);  F_l(k) = sum_m S_lm(k^) rfftn[S_lm(r^_cell) F](k) with real harmonics S_lm scaled so that
   sum_m S_lm(a) S_lm(b) = L_l(a . b); r^_cell is the direction of the cell centre c + (i, j, k) L / n.
4. P_l^{ab}(k) = (2l + 1) / I_ab < 1/2 Re[F_l^a conj F_0^b + F_l^b conj F_0^a] / W(k)^2 >_bin - delta_l0 N_ab / I_ab, with the bins,
   `N_mode` and `k_avg` of `calc_pk_from_deltak` (half-mesh multiplicities) and W(k) the product of the three
   `get_W_compensated(L, n, paste, interlaced=False)` factors when `compensated`.
5. I_ab = alpha_a alpha_b sum_r w_r^2 nbar_r with `nbar` the number density of the random catalogue at each random
   (`LCRandoms(nbar=...)`, e.g. from `radial_nbar`; weights are taken to be FKP-type weights);  N_aa = sum_g w_g^2 + alpha_a^2 sum_r w_r^2;
   N_ab = alpha_a alpha_b sum_r w_r^2 for a != b (the randoms are shared).  All in float64; `norm=` overrides I.

Not built: interlacing, float64 meshes, odd multipoles and l > 4, window-function multipoles of the randoms.  There is no CPU fallback.
"""
import ctypes as C

import numpy as np

from .. import _lib
from .._lib import DeviceArray, check, ptr
from .power_spectrum import _alloc_outputs, _paste_code, get_k_mu_edges, get_W_compensated
from .tpcf_corrfunc import LCRandoms, _LCSample

__all__ = ['LCRandoms', 'FKPField', 'radial_nbar', 'fkp_field', 'calc_power_lc', 'POLES']

POLES = (0, 2, 4)


# ------------------------------------------------------------------------------------------------- checks made before the library loads
def _nmesh(nmesh):
    nmesh = int(nmesh)
    if nmesh < 2 or nmesh % 2 or nmesh > 32766:
        raise ValueError(f'nmesh = {nmesh}: the light-cone spectra need an even mesh of 2 .. 32766 cells per side')
    return nmesh


def _poles(poles):
    poles = [int(p) for p in poles]
    if not poles or any(p not in POLES for p in poles) or len(set(poles)) != len(poles):
        raise ValueError(f'poles = {poles}: a non-empty subset of {POLES} without repeats')
    return poles


def _check_randoms(randoms, norm=None, need_norm=False):
    if not isinstance(randoms, LCRandoms):
        raise TypeError(f'randoms must be an LCRandoms, got {type(randoms).__name__}')
    if need_norm and norm is None and randoms.nbar is None:
        raise ValueError('the normalisation I = alpha_a alpha_b sum w^2 nbar needs LCRandoms(nbar=...) or norm=')
    if norm is not None and not (np.isfinite(norm) and norm != 0):
        raise ValueError(f'norm must be finite and not zero, got {norm}')


def radial_nbar(x, y, z, edges, fsky, origin=(0.0, 0.0, 0.0)):
    """The number density of a catalogue at each of its points from its own radial distribution: the count in the shell
    [edges[i], edges[i + 1]) of distance from `origin` (the last shell closed) divided by the shell's volume
    fsky 4 pi / 3 (chi_2^3 - chi_1^3).  Host NumPy, float64; a point outside the edges gets 0.  What `LCRandoms(nbar=...)` takes."""
    edges = np.asarray(edges, dtype=np.float64)
    if edges.ndim != 1 or len(edges) < 2 or not (np.diff(edges) > 0).all() or edges[0] < 0:
        raise ValueError('edges must be at least two increasing distances, the first not negative')
    if not (fsky > 0 and fsky <= 1):
        raise ValueError(f'fsky must lie in (0, 1], got {fsky}')
    chi = np.sqrt(sum((np.asarray(c, dtype=np.float64) - float(o)) ** 2 for c, o in zip((x, y, z), origin)))
    count, _ = np.histogram(chi, bins=edges)
    dens = count / (fsky * 4.0 * np.pi / 3.0 * (edges[1:] ** 3 - edges[:-1] ** 3))
    shell = np.searchsorted(edges, chi, side='right') - 1
    shell[chi == edges[-1]] = len(edges) - 2
    inside = (shell >= 0) & (shell < len(dens))
    return np.where(inside, dens[np.clip(shell, 0, len(dens) - 1)], 0.0)


# ------------------------------------------------------------------------------------------------- box, randoms mesh, normalisation
def _extent(sample):
    """(lo (3,), hi (3,)) float32 of a sample's observer-centred columns: one small reduction on the device, kept by the sample"""
    if getattr(sample, '_lohi', None) is None:
        out = np.empty(6, dtype=np.float32)
        check(_lib.lib().abacus_lc_extent_dev(*[c.ptr for c in sample.cols], C.c_int64(sample.n), ptr(out)))
        sample._lohi = out
    return sample._lohi[:3], sample._lohi[3:]


def _box(randoms, boxpad, Lbox):
    lo, hi = (a.astype(np.float64) for a in _extent(randoms))
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError('the randoms hold a coordinate that is not finite')
    if Lbox is None:
        if not (boxpad >= 1 and np.isfinite(boxpad)):
            raise ValueError(f'boxpad must be at least 1, got {boxpad}')
        L = float(boxpad * (hi - lo).max())
    else:
        L = float(Lbox)
    if not (L > 0 and np.isfinite(L)):
        raise ValueError(f'the box side must be positive, got {L}')
    return L, ((lo + hi) / 2 - L / 2).astype(np.float32).astype(np.float64)


def _check_inside(sample, what, n, L, corner):
    """every point at least two cells from every face, judged on the float32 positions the deposit sees: s = r - c is monotonic in r,
    so the extent of the columns decides"""
    lo, hi = _extent(sample)
    c = corner.astype(np.float32)
    h = L / n
    with np.errstate(invalid='ignore', over='ignore'):
        slo, shi = (lo - c).astype(np.float64), (hi - c).astype(np.float64)
    if not (np.isfinite(slo).all() and np.isfinite(shi).all() and (slo >= 2 * h).all() and (shi <= L - 2 * h).all()):
        raise ValueError(f'{what}: a point lies outside the box or closer than two cells to a face (box side {L:g}, corner '
                         f'{tuple(float(v) for v in corner)}, extent {tuple(float(v) for v in lo)} .. {tuple(float(v) for v in hi)}, '
                         f'cell {h:g}); the deposit would fold it in: enlarge boxpad or Lbox')


def _padded(n):
    nb = C.c_uint64(0)
    check(_lib.lib().abacus_zcv_spectrum_bytes(n, C.byref(nb)))
    return DeviceArray(nbytes=nb.value, dtype=np.uint8, shape=(nb.value,))


def _deposit(sample, n, L, corner, code, mesh):
    """mesh = the raw weighted deposit of the sample, through a packed (N, 3) float32 copy of its columns"""
    work = DeviceArray(nbytes=12 * sample.n, dtype=np.float32, shape=(sample.n, 3))
    try:
        lib = _lib.lib()
        check(lib.abacus_lc_pack_dev(*[c.ptr for c in sample.cols], C.c_int64(sample.n), ptr(corner), work.ptr))
        check(lib.abacus_lc_deposit_dev(work.ptr, C.c_int64(sample.n), None if sample.w is None else sample.w.ptr, C.c_double(L), n, code,
                                        mesh.ptr))
        _lib.sync()
    finally:
        work.free()


def _mesh_key(n, L, corner, paste):
    return (int(n), float(L), tuple(float(v) for v in corner), str(paste).upper())


def _randoms_mesh(randoms, n, L, corner, paste):
    """R, deposited once per (n, L, corner, paste) and kept by the LCRandoms, as RR is"""
    key = _mesh_key(n, L, corner, paste)
    if key not in randoms._mesh:
        _check_inside(randoms, 'randoms', n, L, corner)
        mesh = _padded(n)
        try:
            _deposit(randoms, n, L, corner, _paste_code(paste, ':'), mesh)
        except Exception:
            mesh.free()
            raise
        randoms._mesh[key] = mesh
        randoms.mesh_built += 1
    return randoms._mesh[key]


def _sum_w2n(randoms):
    """sum_r w_r^2 nbar_r in float64: a two-stage reduction on the device, kept by the LCRandoms"""
    if randoms._w2n is None:
        nbar = randoms.nbar
        own = not isinstance(nbar, DeviceArray)
        dev = DeviceArray(np.ascontiguousarray(nbar, dtype=np.float64)) if own else nbar
        try:
            out = np.zeros(1, dtype=np.float64)
            check(_lib.lib().abacus_lc_sum_w2n_dev(None if randoms.w is None else randoms.w.ptr, dev.ptr, int(dev.dtype == np.float64),
                                                   C.c_int64(randoms.n), ptr(out)))
        finally:
            if own:
                dev.free()
        randoms._w2n = float(out[0])
    return randoms._w2n


# ------------------------------------------------------------------------------------------------- the field
class FKPField:
    """F = D - alpha R of one sample, a float32 mesh resident in HBM in the padded layout, and the multipole spectra made from it so
    far.  Attributes `nmesh`, `Lbox`, `corner` (3,), `alpha`, `paste`, `W` and `W2` (the sample's float64 sum of weights and of their
    squares).  `.fetch()` returns the real float32 (n, n, n) mesh, `.spectrum(ell)` the complex64 (n, n, n/2+1) spectrum F_l (not
    compensated); `.free()` or leaving a `with` block releases the memory.  A freed holder raises RuntimeError."""

    def __init__(self, nmesh, Lbox, corner, alpha, paste, W, W2):
        self.nmesh, self.Lbox, self.corner, self.alpha = int(nmesh), float(Lbox), np.asarray(corner, dtype=np.float64), float(alpha)
        self.paste, self.W, self.W2 = str(paste).upper(), float(W), float(W2)
        self._F = None
        self._spec = {}
        self._compensated = False

    def _live(self):
        if self._F is None:
            raise RuntimeError('the FKPField has been freed')

    def _fetch(self, arr):
        n = self.nmesh
        row = np.empty((n, n, n // 2 + 1), dtype=np.complex64)
        check(_lib.lib().abacus_zcv_spectrum_fetch(arr.ptr, n, ptr(row)))
        return row

    def fetch(self):
        self._live()
        return self._fetch(self._F).view(np.float32)[:, :, :self.nmesh].copy()      # a padded row as n + 2 floats, the first n the mesh

    def _spectrum_dev(self, ell):
        """F_l in HBM, built on first use (1 transform for l = 0, 2 l + 1 otherwise)"""
        self._live()
        if ell not in POLES:
            raise ValueError(f'multipole {ell}: one of {POLES}')
        if self._compensated:
            raise RuntimeError('the spectra of this field have been compensated in place')
        if ell not in self._spec:
            out, work = _padded(self.nmesh), None
            try:
                if ell:
                    work = _padded(self.nmesh)
                check(_lib.lib().abacus_lc_multipole_dev(self._F.ptr, self.nmesh, C.c_double(self.Lbox), ptr(self.corner), int(ell),
                                                         None if work is None else work.ptr, out.ptr))
                _lib.sync()
            except Exception:
                out.free()
                raise
            finally:
                if work is not None:
                    work.free()
            self._spec[ell] = out
        return self._spec[ell]

    def spectrum(self, ell):
        return self._fetch(self._spectrum_dev(int(ell)))

    def _compensate(self):
        """every spectrum made so far divided by the window of the cloud, in place (calc_power_lc, on its own fields)"""
        W = np.ascontiguousarray(get_W_compensated(self.Lbox, self.nmesh, self.paste, False), dtype=np.float32)
        for spec in self._spec.values():
            check(_lib.lib().abacus_lc_compensate_dev(spec.ptr, self.nmesh, ptr(W)))
        self._compensated = True

    def free(self):
        for a in [self._F] + list(self._spec.values()):
            if a is not None:
                a.free()
        self._F, self._spec = None, {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False


def _field(sample, randoms, n, L, corner, paste, nspectra=0):
    code = _paste_code(paste, ':')
    _check_inside(sample, 'data', n, L, corner)
    key = _mesh_key(n, L, corner, paste)
    new = 1 + nspectra + (1 if nspectra > 1 else 0) + (0 if key in randoms._mesh else 1)
    check(_lib.lib().abacus_lc_check_memory(n, new, C.c_int64(sample.n + (0 if key in randoms._mesh else randoms.n))))
    R = _randoms_mesh(randoms, n, L, corner, paste)
    if not randoms.W > 0 or not np.isfinite(sample.W):
        raise ValueError('the weights of the randoms must have a positive sum')
    field = FKPField(n, L, corner, sample.W / randoms.W, paste, sample.W, sample.W2)
    try:
        field._F = _padded(n)
        _deposit(sample, n, L, corner, code, field._F)
        check(_lib.lib().abacus_lc_axpy_dev(field._F.ptr, R.ptr, n, C.c_double(-field.alpha)))
        _lib.sync()
    except Exception:
        field.free()
        raise
    return field


def fkp_field(x, y, z, randoms, nmesh, w=None, origin=(0.0, 0.0, 0.0), paste='TSC', boxpad=1.25, Lbox=None):
    """Steps 1 and 2 of the module docstring for one sample: columns as `_LCSample` takes them (host arrays, or three `DeviceArray`s of
    one dtype; not modified), `randoms` an `LCRandoms`.  Returns an `FKPField` (context-managed, like a `Displacement`)."""
    _check_randoms(randoms)
    nmesh = _nmesh(nmesh)
    _paste_code(paste, ':')
    sample = _LCSample(x, y, z, w, origin)
    L, corner = _box(randoms, boxpad, Lbox)
    return _field(sample, randoms, nmesh, L, corner, paste)


# ------------------------------------------------------------------------------------------------- the spectra
def _bin(n, L, a, b, ke):
    """< Re(a conj b) >_bin, N_mode, k_avg of two padded spectra (b None: |a|^2) over one mu bin: power_bin_padded_dev, whose mean
    carries L^3 - taken out again in float64"""
    me = np.array([0.0, 1.0])
    pl = np.empty(0, dtype=np.int64)
    outs = _alloc_outputs(len(ke) - 1, 1, 0)
    check(_lib.lib().abacus_zcv_power_pair(a.ptr, None if b is None else b.ptr, n, C.c_double(L), ptr(ke), len(ke) - 1, ptr(me), 1, ptr(pl), 0,
                                           *[ptr(o) for o in outs]))
    return outs[0][:, 0].astype(np.float64) / L**3, outs[1][:, 0], outs[4][:, 0]


def _edges(L, n, kbins, k_max, logk):
    if k_max is None:
        k_max = np.pi * n / L
    ke, _ = get_k_mu_edges(L, k_max, kbins, 1, logk)
    ke = np.ascontiguousarray(ke, dtype=np.float64)
    if ke.ndim != 1 or len(ke) < 2:
        raise ValueError('kbins must be a number of bins or at least two edges')
    return ke


def _pair_poles(fa, fb, poles, ke, norm, randoms):
    """(poles (Np, Nk), N_mode, k_avg, norm, shotnoise) of the fields fa and fb (fb None or fa: the auto spectrum)"""
    auto = fb is None or fb is fa
    n, L = fa.nmesh, fa.Lbox
    if norm is None:
        norm = fa.alpha * (fa if auto else fb).alpha * _sum_w2n(randoms)
    shot = fa.W2 + fa.alpha**2 * randoms.W2 if auto else fa.alpha * fb.alpha * randoms.W2
    out = []
    for ell in poles:
        if auto:
            p, N_mode, k_avg = _bin(n, L, fa._spec[ell], None if ell == 0 else fa._spec[0], ke)
        else:
            p, N_mode, k_avg = _bin(n, L, fa._spec[ell], fb._spec[0], ke)
            if ell:
                p = 0.5 * (p + _bin(n, L, fb._spec[ell], fa._spec[0], ke)[0])
        out.append((2 * ell + 1) / norm * p - (shot / norm if ell == 0 else 0.0))
    return np.array(out), N_mode, k_avg, norm, shot


def _spectra(field, poles, compensated):
    for ell in sorted(set(poles) | {0}):
        field._spectrum_dev(ell)
    if compensated:
        field._compensate()


def calc_power_lc(x1, y1, z1, randoms, kbins, nmesh=256, poles=(0, 2, 4), k_max=None, logk=False, paste='TSC', compensated=True,
                  x2=None, y2=None, z2=None, w1=None, w2=None, origin=(0.0, 0.0, 0.0), boxpad=1.25, Lbox=None, norm=None):
    """P_l(k) of a light-cone catalogue seen from `origin` (steps 1 to 5 of the module docstring); with x2, y2, z2 the cross spectrum of
    two samples that share the randoms.  Columns: host arrays or - all three of a sample - `DeviceArray`s of one dtype (the `_LCSample`
    rules; nothing is modified); w1 / w2 per-point weights; `randoms` an `LCRandoms` (with `nbar=` unless `norm=` is given).  `kbins`:
    a number of bins up to `k_max` (default: the Nyquist frequency pi nmesh / L) or the edges; `poles` a subset of (0, 2, 4); nmesh even.
    Returns dict(poles (Np, Nk) float64, N_mode, k_avg, k_mid, norm, shotnoise, alpha, Lbox, corner); `alpha` is a float for an auto
    spectrum and a pair for a cross spectrum, `shotnoise` is N_ab (already subtracted from the monopole as N_ab / norm)."""
    _check_randoms(randoms, norm, need_norm=True)
    nmesh, poles = _nmesh(nmesh), _poles(poles)
    _paste_code(paste, ':')
    cross = x2 is not None
    if not cross and (w2 is not None or y2 is not None or z2 is not None):
        raise ValueError('w2, y2 or z2 given without x2')
    s1 = _LCSample(x1, y1, z1, w1, origin)
    s2 = _LCSample(x2, y2, z2, w2, origin) if cross else None
    L, corner = _box(randoms, boxpad, Lbox)
    ke = _edges(L, nmesh, kbins, k_max, logk)
    fields = []
    try:
        for s in (s1, s2) if cross else (s1,):
            fields.append(_field(s, randoms, nmesh, L, corner, paste, nspectra=len(set(poles) | {0})))
            _spectra(fields[-1], poles, compensated)
        P, N_mode, k_avg, norm, shot = _pair_poles(fields[0], fields[-1] if cross else None, poles, ke, norm, randoms)
        alpha = (fields[0].alpha, fields[1].alpha) if cross else fields[0].alpha
    finally:
        for f in fields:
            f.free()
    return dict(poles=P, N_mode=N_mode, k_avg=k_avg, k_mid=0.5 * (ke[1:] + ke[:-1]), norm=norm, shotnoise=shot, alpha=alpha, Lbox=L,
                corner=corner)


def calc_power_lc_multi(samples, randoms, kbins, nmesh, poles, k_max=None, logk=False, paste='TSC', compensated=True,
                        origin=(0.0, 0.0, 0.0), boxpad=1.25, Lbox=None, norm=None):
    """`calc_power_lc` for every pair of the named samples {name: (x, y, z, w or None)}: each sample's F_0 and F_l are built once.
    Returns ({(a, b): result dict for a before or at b in the order of `samples`}, k_mid)."""
    _check_randoms(randoms, norm, need_norm=True)
    nmesh, poles = _nmesh(nmesh), _poles(poles)
    L, corner = _box(randoms, boxpad, Lbox)
    ke = _edges(L, nmesh, kbins, k_max, logk)
    fields, out = {}, {}
    try:
        for name, (x, y, z, w) in samples.items():
            fields[name] = _field(_LCSample(x, y, z, w, origin), randoms, nmesh, L, corner, paste, nspectra=len(set(poles) | {0}))
            _spectra(fields[name], poles, compensated)
        names = list(samples)
        for i, a in enumerate(names):
            for b in names[i:]:
                P, N_mode, k_avg, I, shot = _pair_poles(fields[a], None if a == b else fields[b], poles, ke, norm, randoms)
                out[(a, b)] = dict(poles=P, N_mode=N_mode, k_avg=k_avg, norm=I, shotnoise=shot, Lbox=L, corner=corner,
                                   alpha=fields[a].alpha if a == b else (fields[a].alpha, fields[b].alpha))
    finally:
        for f in fields.values():
            f.free()
    return out, 0.5 * (ke[1:] + ke[:-1])
