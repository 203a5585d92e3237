"""A chunked NumPy statement of the friends-of-friends groups (include/abacus_hip.h, abacus_fof): the judge of csrc/fof.hip's
fof_link / fof_flatten / fof_reduce / fof_emit (helper of tests/test_groups_*.py, not a test module).

Friendship per pair i != j, in float32 like tests/spheres_statement.py: d = p_i - p_j per component, minimum image by ONE
addition of -+L when |d| > L/2, r2 = dx dx + dy dy + dz dz left to right, friends iff r2 < b * b (a float32 product), strictly;
cylinders (b_par given): r2 = dx dx + dy dy, friends iff r2 < b_perp * b_perp and |dz| < b_par.  A point is not its own friend,
by index: a coincident twin is one.

`groups(...)` returns (labels, degree, links): the components of the friendship graph from scipy.sparse.csgraph, each point
labelled with the smallest index among its group's members (uint32); the number of friends of every point; the number of
unordered friend pairs.  `groups_by_propagation(...)` takes no graph library: every point starts with its own index and takes
the minimum over its friends until nothing changes.  `multiplicity(labels, nmax)`: (mult, ngroups) as the library defines them.
"""
import numpy as np


def friend_pairs(x, y, z, boxsize, b_perp, b_par=None, chunk=256):
    """(i, j) of every ORDERED friend pair (each unordered pair appears twice), int64"""
    f4 = lambda a: np.ascontiguousarray(a, dtype=np.float32)   # noqa: E731
    x, y, z = f4(x), f4(y), f4(z)
    n = len(x)
    b2 = np.float32(b_perp) * np.float32(b_perp)
    box = np.float32(boxsize)
    half = box * np.float32(0.5)

    def image(d):
        return np.where(d > half, d - box, np.where(d < -half, d + box, d))

    ii, jj = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for a in range(0, n, chunk):
        b = min(a + chunk, n)
        dx = image(x[a:b, None] - x[None, :])
        dy = image(y[a:b, None] - y[None, :])
        dz = image(z[a:b, None] - z[None, :])
        ok = np.ones(dx.shape, bool)
        ok[np.arange(b - a), np.arange(a, b)] = False
        if b_par is not None:
            r2 = dx * dx + dy * dy
            ok &= np.abs(dz) < np.float32(b_par)
        else:
            r2 = dx * dx + dy * dy + dz * dz
        assert r2.dtype == np.float32
        i, j = np.nonzero(ok & (r2 < b2))
        ii.append(i.astype(np.int64) + a), jj.append(j.astype(np.int64))
    return np.concatenate(ii), np.concatenate(jj)


def _canonical(comp):
    """component numbers -> the smallest member index of each component, uint32"""
    n = len(comp)
    smallest = np.full(comp.max() + 1 if n else 0, n, dtype=np.int64)
    np.minimum.at(smallest, comp, np.arange(n))
    return smallest[comp].astype(np.uint32)


def groups(x, y, z, boxsize, b_perp, b_par=None):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    n = len(x)
    i, j = friend_pairs(x, y, z, boxsize, b_perp, b_par)
    degree = np.bincount(i, minlength=n).astype(np.int64)
    assert len(i) % 2 == 0 and np.array_equal(degree, np.bincount(j, minlength=n))   # friendship is symmetric
    if n == 0:
        return np.zeros(0, np.uint32), degree, 0
    graph = coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(n, n))
    _, comp = connected_components(graph, directed=False)
    return _canonical(comp), degree, len(i) // 2


def groups_by_propagation(x, y, z, boxsize, b_perp, b_par=None):
    """labels only: min-label propagation over the friend list to a fixed point"""
    n = len(x)
    i, j = friend_pairs(x, y, z, boxsize, b_perp, b_par)
    label = np.arange(n, dtype=np.int64)
    while True:
        new = label.copy()
        np.minimum.at(new, i, label[j])
        new = new[new]                    # pointer jumping: a label is an index whose own label is no larger
        if np.array_equal(new, label):
            return label.astype(np.uint32)
        label = new


def multiplicity(labels, nmax):
    labels = np.asarray(labels).astype(np.int64)
    size = np.bincount(labels, minlength=len(labels))
    size = size[size > 0]
    return np.bincount(np.minimum(size, nmax), minlength=nmax + 1).astype(np.uint64), len(size)
