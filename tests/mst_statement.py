"""A NumPy statement of the minimum spanning forest (include/abacus_hip.h, abacus_mst): the judge of csrc/mst.hip's rounds and of
analysis/mst.py's branches (helper of tests/test_mst_*.py, not a test module).

The graph is that of tests/groups_statement.py: the ordered friend pairs of `friend_pairs` at b_perp = rmax, spheres.  r2 of an
edge is recomputed here with the float32 expressions of the library: d = p_lo - p_hi per component, ONE addition of -+L when
|d| > L/2, r2 = dx dx + dy dy + dz dz left to right.  Edges compare by the key (r2, lo, hi), lo < hi the indices of the ends.

`forest(...)` is Kruskal: the edges in np.lexsort((hi, lo, r2)) order, each taken iff a small union-find has its ends apart.
`forest_by_rank(...)` is Boruvka in a second, independent form: the rank of an edge in that order is its weight, every round
takes per component (scipy.sparse.csgraph.connected_components of the edges taken so far) the smallest rank among the edges that
leave it, by np.minimum.at.  Both return (lo, hi, r2) ascending in the key - the library's output order.
`branches_by_walking(...)`: the branches of a forest by a plain walk from node to node.
"""
import groups_statement as gst
import numpy as np


def graph_edges(x, y, z, boxsize, rmax):
    """(lo, hi, r2) of every edge of G(rmax), once each, in key order; int64, int64, float32"""
    i, j = gst.friend_pairs(x, y, z, boxsize, rmax)
    keep = i < j
    lo, hi = i[keep], j[keep]
    f4 = lambda a: np.ascontiguousarray(a, dtype=np.float32)   # noqa: E731
    x, y, z = f4(x), f4(y), f4(z)
    box = np.float32(boxsize)
    half = box * np.float32(0.5)

    def image(d):
        return np.where(d > half, d - box, np.where(d < -half, d + box, d))
    dx, dy, dz = image(x[lo] - x[hi]), image(y[lo] - y[hi]), image(z[lo] - z[hi])
    r2 = dx * dx + dy * dy + dz * dz
    assert r2.dtype == np.float32 and np.all(r2 < np.float32(rmax) * np.float32(rmax))
    order = np.lexsort((hi, lo, r2))
    return lo[order], hi[order], r2[order]


def tied_values(r2):
    """the number of edges whose r2 equals that of another edge"""
    _, counts = np.unique(r2, return_counts=True)
    return int(counts[counts > 1].sum())


def forest(x, y, z, boxsize, rmax, edges=None):
    """Kruskal over the edges in key order"""
    lo, hi, r2 = edges if edges is not None else graph_edges(x, y, z, boxsize, rmax)
    parent = list(range(len(x)))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    take = np.zeros(len(lo), bool)
    for e, (a, b) in enumerate(zip(lo.tolist(), hi.tolist())):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
            take[e] = True
    return lo[take], hi[take], r2[take]


def forest_by_rank(x, y, z, boxsize, rmax, edges=None):
    """Boruvka with the edge's rank in key order as its weight; returns (lo, hi, r2, rounds)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    lo, hi, r2 = edges if edges is not None else graph_edges(x, y, z, boxsize, rmax)
    n, ne = len(x), len(lo)
    take = np.zeros(ne, bool)
    rank = np.arange(ne)
    rounds = 0
    while True:
        graph = coo_matrix((np.ones(int(take.sum()), np.int8), (lo[take], hi[take])), shape=(n, n))
        _, comp = connected_components(graph, directed=False)
        out = comp[lo] != comp[hi]
        if not out.any():
            break
        best = np.full(n, ne, dtype=np.int64)
        np.minimum.at(best, comp[lo[out]], rank[out])
        np.minimum.at(best, comp[hi[out]], rank[out])
        take[best[best < ne]] = True
        rounds += 1
    return lo[take], hi[take], r2[take], rounds


def labels_of(n, lo, hi):
    """(the smallest index in every point's tree, uint32; the number of trees) from the forest's edges alone"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    if n == 0:
        return np.zeros(0, np.uint32), 0
    graph = coo_matrix((np.ones(len(lo), np.int8), (lo, hi)), shape=(n, n))
    ncomp, comp = connected_components(graph, directed=False)
    return gst._canonical(comp), ncomp


def branches_by_walking(i, j, x, y, z, boxsize):
    """[(end0, end1, edges, b, s)] sorted by the ends, end0 < end1: from every node of degree != 2 along every neighbour of
    degree 2 until the next node of degree != 2, adding up the minimum-image steps in float64"""
    n, L = len(x), float(boxsize)
    pos = np.stack([np.asarray(c, dtype=np.float64) for c in (x, y, z)], axis=1)
    nbrs = [[] for _ in range(n)]
    for a, b in zip(np.asarray(i).tolist(), np.asarray(j).tolist()):
        nbrs[a].append(b), nbrs[b].append(a)
    found = []
    for a in range(n):
        if len(nbrs[a]) == 2:
            continue
        for b in nbrs[a]:
            if len(nbrs[b]) != 2:
                continue
            before, here, steps, total, vec = a, b, 0, 0.0, np.zeros(3)
            while True:
                d = pos[here] - pos[before]
                d -= L * np.round(d / L)
                vec += d
                total += float(np.sqrt((d * d).sum()))
                steps += 1
                if len(nbrs[here]) != 2:
                    break
                nxt = nbrs[here][0] if nbrs[here][0] != before else nbrs[here][1]
                before, here = here, nxt
            if a < here:
                found.append((a, here, steps, total, float(np.sqrt((vec * vec).sum())) / total if total > 0 else 0.0))
    return sorted(found)
