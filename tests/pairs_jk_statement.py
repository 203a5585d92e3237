"""Per-region pair counts built from the two pair statements (tests/pairs_statement.py for the periodic box,
tests/pairs_los_statement.py for the light cone): the judge of the jackknife counters (helper of tests/test_jackknife_*.py,
not a test module).  Membership is NOT restated here - every number is a call of one of the two `paircount` statements on
subsets of the points:

    cross count       first[k] = statement(set 1 restricted to k, set 2)       second[k] = statement(set 1, set 2 restricted to k)
                      both[k]  = statement(set 1 in k, set 2 in k)
    autocorrelation   both[k]  = auto statement of the subset k
                      first[k] = both[k] + cross statement(subset k, complement of k)        second = first

Nothing passes a point against itself (the subset and its complement are disjoint, the auto statement excludes self pairs),
so bins that start at 0 and duplicated points are handled.  Every entry comes with `wabs` = sum |w_i w_j| for the bound
n 2^-52 wabs of `pairs_statement.bounds`.
"""
import numpy as np
import pairs_los_statement
import pairs_statement

NONE3 = (None, None, None)


def box(boxsize, bins, **kw):
    """statement(mode, a, b, w1, w2) of the periodic box: (npairs, wsum, wabs)"""
    def run(mode, a, b, w1, w2):
        n, ws, _, wabs = pairs_statement.paircount(mode, *a, boxsize, bins, *(NONE3 if b is None else b), w1=w1, w2=w2, **kw)
        return n, ws, wabs
    return run


def los(bins, origin=(0.0, 0.0, 0.0), **kw):
    """statement(mode, a, b, w1, w2) of the light cone"""
    def run(mode, a, b, w1, w2):
        n, ws, _, wabs = pairs_los_statement.paircount(mode, *a, bins, *(NONE3 if b is None else b), w1=w1, w2=w2, origin=origin, **kw)
        return n, ws, wabs
    return run


def _take(cols, w, mask):
    return [np.asarray(c)[mask] for c in cols], (None if w is None else np.asarray(w)[mask])


def counts(statement, mode, a, la, nreg, b=None, lb=None, w1=None, w2=None):
    """dict of total / first / second / both, each a dict of npairs (uint64), wsum and wabs (float64): total (ntot,), the
    others (nreg, ntot)"""
    auto = b is None
    la = np.asarray(la)
    lb = la if auto else np.asarray(lb)
    total = statement(mode, a, b, w1, None if auto else w2)
    ntot = len(total[0])
    names = ('npairs', 'wsum', 'wabs')
    out = {t: dict(npairs=np.zeros((nreg, ntot), np.uint64), wsum=np.zeros((nreg, ntot)), wabs=np.zeros((nreg, ntot)))
           for t in ('first', 'second', 'both')}
    out['total'] = dict(zip(names, total))
    for k in range(nreg):
        ak, wak = _take(a, w1, la == k)
        if auto:
            rest, wrest = _take(a, w1, la != k)
            both = statement(mode, ak, None, wak, None)
            cross = statement(mode, ak, rest, wak, wrest)
            first = tuple(x + y for x, y in zip(both, cross))
            second = first
        else:
            bk, wbk = _take(b, w2, lb == k)
            first = statement(mode, ak, b, wak, w2)
            second = statement(mode, a, bk, w1, wbk)
            both = statement(mode, ak, bk, wak, wbk)
        for t, v in (('first', first), ('second', second), ('both', both)):
            for name, arr in zip(names, v):
                out[t][name][k] = arr
    return out


def removed(statement, mode, a, la, k, b=None, lb=None, w1=None, w2=None):
    """the statement on the catalogue without region k: (npairs, wsum, wabs)"""
    ar, war = _take(a, w1, np.asarray(la) != k)
    if b is None:
        return statement(mode, ar, None, war, None)
    br, wbr = _take(b, w2, np.asarray(lb) != k)
    return statement(mode, ar, br, war, wbr)


def pick(c, name):
    """the arrays of one kind (npairs | wsum | wabs) as the dict `jackknife.delete_one` takes"""
    return {t: c[t][name] for t in ('total', 'first', 'second', 'both')}
