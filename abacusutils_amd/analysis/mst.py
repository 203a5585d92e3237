"""The minimum spanning tree statistic on the MI355X: the minimum spanning forest of one catalogue on the periodic box
(csrc/mst.hip: Boruvka's rounds - mst_scan, mst_tie, mst_hook, mst_flatten - and the edge sort behind them; C ABI
`abacus_mst[_dev]`), and what is built on its edges on the host - branches, and the four distributions of Naidoo et al. (2020):
node degree d, edge length l, branch length b and branch shape s.

The reference has no spanning tree: the conventions are those of include/abacus_hip.h, pinned against the NumPy statement
tests/mst_statement.py.  The graph is G(rmax): two points are joined iff r2 < float32(rmax) * float32(rmax) in float32,
strictly, under the expressions of the counts in spheres - the friendship graph of `groups.fof_groups` with b_perp = rmax.
Edges are ordered by the key (r2, lo, hi), lo < hi the indices of the two ends, which is strict and total: the forest is unique
although float32 values of r2 tie.  Kruskal on the complete graph takes the edges in that order, so the forest of G(rmax) is the
Euclidean minimum spanning tree with its edges of r2 >= rmax^2 removed.  It IS the Euclidean tree whenever it comes back with
one component; the forest at r1 < r2 is the forest at r2 filtered to r2 < r1^2; and its components are the FoF groups at
b = rmax.  MiSTree (Naidoo 2019) spans a k = 20 nearest-neighbour graph instead, which is neither of these: a point in a
clump of more than k members can lose the edge that would have joined two clumps.  Here the cut is a length, and says so.

Choosing rmax (`groups.linking_lengths` turns fractions of the mean separation into box units): for 10^7 uniform points in a box
of 2000 the longest edge of the Euclidean tree is around 1.6 mean separations, so rmax at 1.6 - 2 mean separations returns one
tree; a clustered catalogue of the same density needs more for its emptiest regions, and every separation more costs candidates
as rmax^3.  A forest of a few trees is as good for the statistics: the edges left out are the longest ones.

Limits: the periodic box only, one catalogue per call, spheres (no cylinders, no redshift-space linking), no light cone, a forest
beyond rmax (no growing of the radius for what is left over); the edges come back to the host, and the branches are NumPy.
"""
import ctypes as C

import numpy as np

from .. import _lib
from .._lib import check, ptr
from .tpcf_corrfunc import _call_on_columns


def minimum_spanning_tree(X, Y, Z, boxsize, rmax, return_degree=True, return_labels=False):
    """The minimum spanning forest of the graph G(rmax) of (X, Y, Z), `rmax` in the units of `boxsize` (at most half of it).
    Returns {'i', 'j': (nedges,) uint32 - the smaller and the larger index of every edge's ends, in the order of the input; 'r2':
    (nedges,) float32; 'length': (nedges,) float64, the square root of r2 - all ascending in (r2, i, j); 'degree': (n,) uint32 or
    None unless `return_degree`; 'labels': (n,) uint32 - the smallest index in the point's tree - or None unless `return_labels`;
    'nedges'; 'ncomp' (nedges + ncomp == n: one tree when ncomp == 1); 'n'}.  Columns: host arrays, or all DeviceArray of one
    dtype (`_call_on_columns`)."""
    n = len(X)
    if not (len(Y) == n and len(Z) == n):
        raise ValueError('X, Y and Z differ in length')
    ei, ej, er2 = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.float32)
    degree = np.zeros(n, dtype=np.uint32) if return_degree else None
    labels = np.zeros(n, dtype=np.uint32) if return_labels else None
    nedges, ncomp = C.c_uint64(0), C.c_uint64(0)

    def call(fn, p, cols, w, lab, geom, *dt):
        check(fn(*map(p, cols), C.c_int64(n), *dt, *geom, C.c_float(rmax), ptr(ei), ptr(ej), ptr(er2), ptr(degree), ptr(labels),
                 C.byref(nedges), C.byref(ncomp)))
        ne = int(nedges.value)
        r2 = er2[:ne].copy()
        return {'i': ei[:ne].copy(), 'j': ej[:ne].copy(), 'r2': r2, 'length': np.sqrt(r2.astype(np.float64)), 'degree': degree,
                'labels': labels, 'nedges': ne, 'ncomp': int(ncomp.value), 'n': n}
    return _call_on_columns('mst', [X, Y, Z], (None, None), (), (C.c_float(boxsize),), call)


def last_stats():
    """{'candidates', 'rounds', 'cells_xy', 'cells_z', 'per_round'} of the last call: candidate pairs evaluated over all rounds,
    Boruvka rounds that emitted edges, the cells per dimension, and per round (the last one, which finds nothing, included) the
    points scanned, the points with an edge out of their tree and the edges emitted: (rounds + 1, 3) uint64 (abacus_mst_stats)"""
    cand, rounds, ncxy, ncz = C.c_uint64(0), C.c_int(0), C.c_int(0), C.c_int(0)
    per = np.zeros((32, 3), dtype=np.uint64)
    check(_lib.lib().abacus_mst_stats(C.byref(cand), C.byref(rounds), C.byref(ncxy), C.byref(ncz), ptr(per)))
    return {'candidates': int(cand.value), 'rounds': rounds.value, 'cells_xy': ncxy.value, 'cells_z': ncz.value,
            'per_round': per[:min(rounds.value + 1, 32)].copy()}


def _edge_vectors(i, j, X, Y, Z, boxsize):
    """p_j - p_i by the minimum image, float64: (nedges, 3)"""
    pos = np.stack([np.asarray(c, dtype=np.float64) for c in (X, Y, Z)], axis=1)
    L = float(boxsize)
    d = pos[j] - pos[i]
    d -= L * np.round(d / L)
    return d


def mst_branches(i, j, X, Y, Z, boxsize):
    """The branches of the forest with the edges (i, j): a branch is a maximal chain of edges whose interior nodes all have degree
    2, with at least one interior node (MiSTree's convention: a single edge between two nodes of degree != 2 is no branch).
    Returns {'end0', 'end1': (nb,) int64 - the two end nodes, end0 < end1; 'nedges': (nb,) int64; 'b': (nb,) float64 - the sum of
    the branch's edge lengths; 's': (nb,) float64 - |sum of d_e| / b with d_e the minimum-image edge vectors oriented along the
    chain, i.e. the end-to-end distance of the unwrapped chain, well defined however long the branch; 'degree': (n,) int64},
    ordered by (end0, end1).  Edge lengths are float64 and recomputed from the positions.

    NumPy, vectorised: every edge is two arcs; the arc behind an arc u -> v is the other way out of v when v has degree 2, and
    pointer doubling along these successors adds up vectors, lengths and edge counts in log2(longest branch) passes.  The input
    must be a forest (a cycle of nodes of degree 2 has no end; it is left out)."""
    i, j = np.asarray(i).astype(np.int64), np.asarray(j).astype(np.int64)
    n, ne = len(X), len(i)
    if not (len(Y) == n and len(Z) == n and len(j) == ne):
        raise ValueError('X, Y, Z or i, j differ in length')
    if ne and (min(i.min(), j.min()) < 0 or max(i.max(), j.max()) >= n):
        raise ValueError('edge index outside the catalogue')
    degree = np.bincount(i, minlength=n) + np.bincount(j, minlength=n)
    empty = {'end0': np.zeros(0, np.int64), 'end1': np.zeros(0, np.int64), 'nedges': np.zeros(0, np.int64), 'b': np.zeros(0),
             's': np.zeros(0), 'degree': degree.astype(np.int64)}
    if ne == 0:
        return empty
    d = _edge_vectors(i, j, X, Y, Z, boxsize)
    # arcs 2 e (i -> j, +d) and 2 e + 1 (j -> i, -d); a ^ 1 is the arc back
    tail = np.stack([i, j], axis=1).ravel()
    head = np.stack([j, i], axis=1).ravel()
    vec = np.stack([d, -d], axis=1).reshape(-1, 3)
    length = np.repeat(np.sqrt((d * d).sum(axis=1)), 2)
    count = np.ones(2 * ne, dtype=np.int64)
    # the arcs out of every node, contiguous: the two of a node of degree 2
    order = np.argsort(tail, kind='stable')
    first = np.concatenate([[0], np.cumsum(degree)])[:-1]
    two = degree[head] == 2
    h = head[two]
    out0, out1 = order[first[h]], order[first[h] + 1]
    back = np.flatnonzero(two) ^ 1
    nxt = np.full(2 * ne, -1, dtype=np.int64)          # -1: the arc ends its chain (its head is no interior node)
    nxt[two] = np.where(out0 == back, out1, out0)
    end = head.copy()
    start = np.flatnonzero((degree[tail] != 2) & two)  # from an end node into a chain
    for _ in range(max(2 * ne, 2).bit_length() + 1):
        go = np.flatnonzero(nxt >= 0)
        if not len(go):
            break
        t = nxt[go]
        vec[go], length[go], count[go] = vec[go] + vec[t], length[go] + length[t], count[go] + count[t]   # right sides read the old state
        end[go], nxt[go] = end[t], nxt[t]
    done = nxt[start] < 0                              # (a cycle of interior nodes is reached from no end: nothing to drop in a forest)
    start = start[done]
    start = start[tail[start] < end[start]]            # every branch is walked from both ends
    if not len(start):
        return empty
    keep = start[np.lexsort((end[start], tail[start]))]
    b = length[keep]
    s = np.divide(np.sqrt((vec[keep] ** 2).sum(axis=1)), b, out=np.zeros_like(b), where=b > 0)   # (a chain of coincident twins: b = 0, s = 0)
    return {'end0': tail[keep], 'end1': end[keep], 'nedges': count[keep], 'b': b, 's': s, 'degree': degree.astype(np.int64)}


def mst_statistics(result, branches, l_edges, b_edges, s_edges, dmax=8):
    """The four distributions of the minimum spanning tree statistic, each a histogram of fractions (float64):
    {'d': (dmax + 1,) - the fraction of the points with degree 0, 1 .. dmax - 1 and, last, dmax or more; 'l': the fraction of
    the edges with a length in [l_edges[k], l_edges[k + 1]); 'b', 's': the same for the branches' lengths and shapes}.  The
    fractions are of ALL points, edges or branches, so each histogram sums to one exactly when its bins cover every value (the
    last bin is closed above, as numpy.histogram's); an empty set gives zeros.  `result`: of `minimum_spanning_tree` with its
    degrees; `branches`: of `mst_branches`."""
    dmax = int(dmax)
    if dmax < 1:
        raise ValueError('dmax must be at least 1')
    if result.get('degree') is None:
        raise ValueError('the result carries no degrees (return_degree=True)')
    degree = np.asarray(result['degree']).astype(np.int64)

    def fractions(values, edges):
        edges = np.asarray(edges, dtype=np.float64)
        if edges.ndim != 1 or len(edges) < 2 or np.any(np.diff(edges) <= 0):
            raise ValueError('bin edges must increase')
        values = np.asarray(values, dtype=np.float64)
        hist = np.histogram(values, bins=edges)[0].astype(np.float64)
        return hist / len(values) if len(values) else hist
    d = np.bincount(np.minimum(degree, dmax), minlength=dmax + 1).astype(np.float64)
    return {'d': d / len(degree) if len(degree) else d, 'l': fractions(result['length'], l_edges),
            'b': fractions(branches['b'], b_edges), 's': fractions(branches['s'], s_edges)}
