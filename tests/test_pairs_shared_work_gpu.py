"""All seven pair-counting families take turns on the ONE set of work buffers of csrc/pairs_common.hpp (`g_work`: the sorted
sets with their weight and velocity lanes, the flag block, the output block), in one process.  Needs an MI355X: run with `-m gpu`.

The families live in translation units of their own (cellsort.hip, pairs.hip, pairs_jk.hip, spheres.hip, threepcf.hip, fof.hip),
so `g_work` must be a single object to all of them, and no family may depend on what the one before left in it: `SortedSet::sw`
(set by a weighted count, reused by the spheres and the groups as the caller's index), `::sv` (the velocities), the flags.

The lattice of tests/test_pairs_walk_gpu.py makes every squared separation and every sum of weight products exact, so integer
outputs and `weightsum` are IDENTICAL to the statements', not close.  The outputs that depend on the order of float32 additions
(the velocity sums, zeta) are judged in their own modules."""
import groups_statement
import numpy as np
import pairs_los_statement
import pairs_statement
import pytest
import spheres_statement
from test_pairs_walk_gpu import BOX, EDGES, _lattice

pytestmark = pytest.mark.gpu

NSPLIT = 2
B_LINK = 1.75      # a squared linking length of 49/16: exact, like the squared edges
RADII = EDGES[1:]


def test_seven_families_take_turns_on_one_work_object():
    from abacusutils_amd.analysis.groups import fof_groups
    from abacusutils_amd.analysis.jackknife import box_regions, paircount_jk
    from abacusutils_amd.analysis.pairwise_velocity import pairwise_velocity_sums
    from abacusutils_amd.analysis.spheres import count_in_spheres
    from abacusutils_amd.analysis.threepcf import triplet_multipoles
    from abacusutils_amd.analysis.tpcf_corrfunc import DD_los, _paircount, _paircount_weighted
    a, wa = _lattice(1500, 160, 288, 1)
    b, wb = _lattice(1100, 160, 288, 2)
    vel = [np.random.default_rng(7 + d).integers(-300, 301, 1500).astype(np.float32) for d in range(3)]
    labels = box_regions(*a, BOX, NSPLIT)

    n_w, ws_w = pairs_statement.paircount(0, *a, BOX, EDGES, w1=wa)[:2]
    n_u = pairs_statement.paircount(0, *a, BOX, EDGES)[0]
    n_x, ws_x = pairs_los_statement.paircount(0, *a, EDGES, *b, w1=wa, w2=wb)[:2]
    hist_s, counts_s = spheres_statement.count_in_spheres(*a, BOX, RADII, *b)
    labels_s = groups_statement.groups(*a, BOX, B_LINK)[0]
    np.testing.assert_array_equal(n_w, n_u)      # weights do not choose the pairs
    assert n_u.sum() > 0 and n_x.sum() > 0 and counts_s.sum() > 0 and len(np.unique(labels_s)) < 1500

    def weighted_auto(turn):      # counting sort, the weight lane filled
        n, ws, _ = _paircount_weighted(0, *a, BOX, EDGES, W1=wa)
        np.testing.assert_array_equal(n, n_w, err_msg=turn)
        np.testing.assert_array_equal(ws, ws_w, err_msg=turn)

    def unweighted_auto(turn):    # SortedSet::sw is NULL again
        np.testing.assert_array_equal(_paircount(0, *a, BOX, EDGES), n_u, err_msg=turn)

    weighted_auto('1 weighted')
    # velocities: the radix path at every size, SortedSet::sv filled
    got = pairwise_velocity_sums(0, *a, *vel, BOX, EDGES, W1=wa)
    np.testing.assert_array_equal(got['npairs'], n_w, err_msg='2 velocities')
    # queries B in data A: the weight lane of set 0 carries the caller's index
    got = count_in_spheres(*a, BOX, RADII, *b, return_counts=True)
    np.testing.assert_array_equal(got['counts'], counts_s, err_msg='3 spheres')
    np.testing.assert_array_equal(got['hist'], hist_s, err_msg='3 spheres')
    unweighted_auto('4 unweighted')
    got = DD_los(0, 1, EDGES, *a, *b, weights1=wa, weights2=wb, weight_type='pair_product')
    np.testing.assert_array_equal(got['npairs'], n_x, err_msg='5 light cone')
    np.testing.assert_array_equal(got['weightsum'], ws_x, err_msg='5 light cone')
    got = paircount_jk('r', *a, BOX, EDGES, labels, NSPLIT ** 3, W1=wa)
    np.testing.assert_array_equal(np.ravel(got.first.npairs.sum(axis=0, dtype=np.uint64)), n_w, err_msg='6 jackknife')
    got = fof_groups(*a, BOX, B_LINK)
    np.testing.assert_array_equal(got['labels'], labels_s, err_msg='7 groups')
    got = triplet_multipoles(*a, BOX, EDGES, 2)
    np.testing.assert_array_equal(got['npairs'], n_u, err_msg='8 triplets')
    weighted_auto('9 weighted again')
    unweighted_auto('9 unweighted again')
