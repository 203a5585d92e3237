"""Friends-of-friends galaxy groups on the MI355X: a group label per point and the group multiplicity function n(N) of one
catalogue on the periodic box (csrc/fof.hip: fof_link and the three kernels behind it, C ABI `abacus_fof[_dev]`), and what is
built on the labels on the host - group sizes, richness-binned n(N) per volume, per-group centres and weight sums.

The reference has no group finder: the conventions are those of include/abacus_hip.h, pinned against the NumPy statement
tests/groups_statement.py.  Two points are friends iff r2 < float32(b) * float32(b) in float32, strictly, under the
expressions of the counts in spheres (cylinders along z when `b_par` is given: rp < b_perp and |dz| < b_par, the form of
Berlind et al. 2006); groups are the connected components, and a point's label is the smallest index among its group's members.

Limits: the periodic box only, one catalogue per call, the line of sight along z, no light cone; the labels come back to the
host (nothing stays in HBM for a later device consumer), and the group properties are NumPy.
"""
import ctypes as C

import numpy as np

from .. import _lib
from .._lib import check, ptr
from .tpcf_corrfunc import _call_on_columns


def fof_groups(X, Y, Z, boxsize, b_perp, b_par=None, nmax=64, return_labels=True):
    """The friends-of-friends groups of (X, Y, Z) with linking length `b_perp` (spheres), or `b_perp` across and `b_par` along z
    (cylinders), both in the units of `boxsize`.  Returns {'labels': (n,) uint32 - the smallest index among the members of the
    point's group, in the order of the input - or None unless `return_labels`; 'ngroups'; 'mult': (nmax + 1,) uint64 - mult[N]
    groups of exactly N members, the last entry those of nmax or more; 'n'}.  Columns: host arrays, or all DeviceArray of one
    dtype (`_call_on_columns`)."""
    if b_par is not None and not b_par > 0:
        raise ValueError('b_par must be positive (None: spheres)')
    n = len(X)
    if not (len(Y) == n and len(Z) == n):
        raise ValueError('X, Y and Z differ in length')
    nmax = int(nmax)
    mult = np.zeros(nmax + 1 if 0 < nmax + 1 <= 8192 else 1, dtype=np.uint64)   # outside: the library refuses the call and writes nothing
    labels = np.zeros(n, dtype=np.uint32) if return_labels else None
    ngroups = C.c_uint64(0)

    def call(fn, p, cols, w, lab, geom, *dt):
        check(fn(*map(p, cols), C.c_int64(n), *dt, *geom, C.c_float(b_perp), C.c_float(0.0 if b_par is None else b_par), nmax,
                 ptr(mult), ptr(labels), C.byref(ngroups)))
        return {'labels': labels, 'ngroups': int(ngroups.value), 'mult': mult, 'n': n}
    return _call_on_columns('fof', [X, Y, Z], (None, None), (), (C.c_float(boxsize),), call)


def last_stats():
    """{'candidates', 'links', 'cells_xy', 'cells_z'} of the last call: candidate pairs evaluated, unordered friend pairs found
    (exact) and the cells per dimension (abacus_fof_stats)"""
    cand, links, ncxy, ncz = C.c_uint64(0), C.c_uint64(0), C.c_int(0), C.c_int(0)
    check(_lib.lib().abacus_fof_stats(C.byref(cand), C.byref(links), C.byref(ncxy), C.byref(ncz)))
    return {'candidates': int(cand.value), 'links': int(links.value), 'cells_xy': ncxy.value, 'cells_z': ncz.value}


def linking_lengths(n, boxsize, b_perp=0.14, b_par=0.75):
    """(b_perp, b_par) in box units: the two lengths, given in units of the mean separation, times (L^3 / n)^(1/3).  The
    defaults are those of Berlind et al. (2006)."""
    n = int(n)
    if n < 1:
        raise ValueError('n must be at least 1')
    sep = (float(boxsize) ** 3 / n) ** (1.0 / 3.0)
    return float(b_perp) * sep, float(b_par) * sep


def group_sizes(labels):
    """the number of members of every point's group: (n,) int64"""
    labels = np.asarray(labels).astype(np.int64)
    if labels.size == 0:
        return np.zeros(0, dtype=np.int64)
    return np.bincount(labels, minlength=len(labels))[labels]


def multiplicity_function(mult, edges, boxsize):
    """n(N) per volume in the richness bins [edges[k], edges[k + 1]): sum of mult over the bin / boxsize^3, float64.  The last
    entry of `mult` is open (groups of nmax or more), so a bin that reaches into it is refused."""
    mult = np.asarray(mult, dtype=np.uint64)
    edges = np.asarray(edges)
    if edges.ndim != 1 or len(edges) < 2 or np.any(edges != np.floor(edges)) or np.any(np.diff(edges) <= 0) or edges[0] < 0:
        raise ValueError('edges must be increasing non-negative integers')
    edges = edges.astype(np.int64)
    nmax = len(mult) - 1
    if edges[-1] > nmax:
        raise ValueError(f'the last bin reaches N = {edges[-1] - 1}, but mult[{nmax}] is open (groups of {nmax} or more): raise nmax')
    cum = np.concatenate([[0], np.cumsum(mult[:nmax], dtype=np.uint64)]).astype(np.float64)
    return (cum[edges[1:]] - cum[edges[:-1]]) / float(boxsize) ** 3


def group_properties(labels, X, Y, Z, boxsize, weights=None):
    """Per group, in NumPy float64 and in the order of increasing label: {'label': (ng,) int64, 'size': (ng,) int64, 'wsum':
    (ng,) - the sum of `weights` (unit weights: the size), 'centre': (ng, 3)}.  The centre is the position of the member that
    carries the label plus the mean minimum-image offset of the members from it, wrapped into [0, boxsize).  It is meaningful
    only for groups narrower than half the box: beyond, the minimum image of a member is not the one the chain of friends leads
    to."""
    labels = np.asarray(labels).astype(np.int64)
    pos = np.stack([np.asarray(c, dtype=np.float64) for c in (X, Y, Z)], axis=1)
    n, L = len(labels), float(boxsize)
    if pos.shape != (n, 3):
        raise ValueError('labels, X, Y and Z differ in length')
    w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    if w.shape != (n,):
        raise ValueError(f'weights has shape {w.shape}, expected ({n},)')
    label, inverse, size = np.unique(labels, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    d = pos - pos[labels]
    d -= L * np.round(d / L)
    mean = np.zeros((len(label), 3))
    for a in range(3):
        mean[:, a] = np.bincount(inverse, weights=d[:, a], minlength=len(label)) / np.maximum(size, 1)
    centre = np.mod(pos[label] + mean, L) if n else np.zeros((0, 3))
    centre[centre >= L] = 0.0          # a negative offset smaller than an ulp of L rounds to L
    return {'label': label, 'size': size.astype(np.int64), 'wsum': np.bincount(inverse, weights=w, minlength=len(label)),
            'centre': centre}
