"""The oracle's restatement of the NFW satellite draw (oracle.nfw_poisson / nfw_counts / nfw_satellites) held to the
reference's laws (gen_sats_nfw, compute_fast_NFW, getPointsOnSphere: hod/GRAND_HOD.py:417-822) with samples far larger
than a GPU test can afford.  The reference draws from unseeded generators, so this link is statistical; the link
oracle -> device is exact (tests/test_nfw_exact_gpu.py).

Bounds.  Goodness-of-fit tests (chi-square, KS) must give p > 1e-4: the seeds are fixed, so a test either passes for
good or fails for good, and with about thirty such tests in this file the chance that a CORRECT sampler was dealt a
failing seed is 3e-3.  Moments are held to 5 standard errors of their estimator (two-sided 6e-7 each)."""
import numpy as np
import pytest
from scipy import stats

import nfw_cases
from oracle import oracle

P_MIN = 1e-4
TR = oracle.TRACERS


def halos(n, c=6.0, rvir=0.5, sigma3d=400.0, lbox=1000.0, seed=1):
    """n halos of one concentration spread over the box [-L/2, L/2)"""
    rng = np.random.default_rng(seed)
    hd = dict(hpos=(rng.random((n, 3)) - 0.5) * lbox, hvel=rng.standard_normal((n, 3)) * 300.0, hmass=np.full(n, 1e13),
              hid=np.arange(n, dtype=np.int64), hsigma3d=np.full(n, sigma3d), hc=np.full(n, c), hrvir=np.full(n, rvir))
    return hd, dict(Lbox=lbox, velz2kms=2000.0, z=0.5)


def sats(hd, params, draw, tracers, t=0, rsd=False, seed=11, per_halo=4, index0=0):
    n = len(hd['hmass'])
    halo = np.repeat(np.arange(n), per_halo)
    rank = np.tile(np.arange(per_halo), n)
    return halo, oracle.nfw_satellites(hd, tracers, params, draw, seed, t, halo, rank, rsd, halo_index0=index0)


@pytest.mark.parametrize('lam', [0.05, 0.7, 3.0, 9.99, 10.0, 10.01, 30.0, 150.0])
def test_poisson_law(lam):
    n = 2_000_000
    k, fragile = oracle.nfw_poisson(np.full(n, lam), seed=int(lam * 1000) + 7, t=1, index0=5_000_000_000)
    assert fragile.all() if lam == 10.0 else fragile.mean() <= 1e-5         # the mean ON the sampler switch is flagged
    # bins of expectation >= 20: single values in the bulk, the two tails pooled
    ks = np.arange(0, int(lam + 40 * np.sqrt(lam) + 40))
    expect = n * stats.poisson.pmf(ks, lam)
    ok = np.nonzero(expect >= 20)[0]
    lo, hi = ok[0], ok[-1]
    obs = np.bincount(np.clip(k, lo, hi) - lo, minlength=hi - lo + 1).astype(float)
    exp = expect[lo:hi + 1].copy()
    exp[0] = n * stats.poisson.cdf(lo, lam)
    exp[-1] = n * stats.poisson.sf(hi - 1, lam)
    assert abs(exp.sum() - n) < 1e-6 * n and len(exp) >= 2
    chi2 = ((obs - exp) ** 2 / exp).sum()
    p = stats.chi2.sf(chi2, len(exp) - 1)
    assert p > P_MIN, (lam, chi2, len(exp), p)
    assert abs(k.mean() - lam) < 5 * np.sqrt(lam / n)
    # var(s^2) = (mu4 - sigma^4) / n with mu4 = lam + 3 lam^2 for a Poisson law
    assert abs(k.var(ddof=1) - lam) < 5 * np.sqrt((lam + 2 * lam * lam) / n)


def test_poisson_streams_differ_by_tracer_index_and_seed():
    lam = np.full(100000, 4.0)
    a = oracle.nfw_poisson(lam, 3, t=0)[0]
    assert not np.array_equal(a, oracle.nfw_poisson(lam, 3, t=1)[0])
    assert not np.array_equal(a, oracle.nfw_poisson(lam, 4, t=0)[0])
    np.testing.assert_array_equal(a[1000:], oracle.nfw_poisson(lam[1000:], 3, t=0, index0=1000)[0])
    assert not np.array_equal(oracle.nfw_poisson(lam, 3, index0=5)[0], oracle.nfw_poisson(lam, 3, index0=2**32 + 5)[0])
    assert oracle.nfw_poisson(np.array([0.0, -1.0, np.nan]), 3)[0].tolist() == [0, 0, 0]


def test_direction_is_isotropic():
    hd, params = halos(250000)
    hd['hpos'][:] = 0.0
    draw = nfw_cases.nfw_table()
    _, s = sats(hd, params, draw, {'LRG': dict(f_sigv=1.0)})
    u = np.stack([s['double'][k] for k in 'xyz'], 1) / s['r'][:, None]
    n = len(u)
    np.testing.assert_allclose(np.linalg.norm(u, axis=1), 1.0, rtol=0, atol=1e-12)
    assert np.abs(u.mean(0)).max() < 5 * np.sqrt(1 / 3 / n)               # var of a component of a uniform direction: 1/3
    assert stats.kstest(u[:, 2], 'uniform', args=(-1, 2)).pvalue > P_MIN  # cos(polar angle) uniform
    phi = np.arctan2(u[:, 1], u[:, 0])
    assert stats.kstest(phi, 'uniform', args=(-np.pi, 2 * np.pi)).pvalue > P_MIN
    assert abs(np.corrcoef(phi, u[:, 2])[0, 1]) < 5 / np.sqrt(n)
    q = u[:, :, None] * u[:, None, :]                                      # <u_i u_j> = delta_ij / 3
    assert np.abs(q.mean(0) - np.eye(3) / 3).max() < 5 * np.sqrt(0.1 / n)  # var(u_i^2) = 4/45, var(u_i u_j) = 1/15


@pytest.mark.parametrize('c', [3.5, 6.0, 9.0])
def test_radius_follows_the_truncated_table(c):
    hd, params = halos(100000, c=c, rvir=0.7)
    draw = nfw_cases.nfw_table()
    _, s = sats(hd, params, draw, {'QSO': dict(f_sigv=1.0)}, t=2, seed=int(c * 10))
    assert np.all(s['branch'] == 0)
    tval = s['r'] / 0.7 * c
    assert tval.max() <= c * (1 + 1e-15)
    assert np.isin(np.round(tval, 9), np.round(draw[draw <= c], 9)).all()   # every radius is an entry of the table
    assert stats.ks_2samp(tval, draw[draw <= c]).pvalue > P_MIN


def test_radius_mixture_with_an_exponential_component():
    c, frac, scale, resc = 6.0, 0.3, 1.7, 0.8
    hd, params = halos(150000, c=c, rvir=0.7)
    draw = nfw_cases.nfw_table()
    tracers = {'LRG': dict(f_sigv=1.0), 'ELG': dict(exp_frac=frac, exp_scale=scale, nfw_rescale=resc)}
    _, s = sats(hd, params, draw, tracers)                                  # LRG satellites: the ELG dict's values apply
    tval = s['r'] / 0.7 * c                                                 # eta * c
    is_exp = s['branch'] == 1
    assert abs(is_exp.mean() - frac) < 5 * np.sqrt(frac * (1 - frac) / len(tval))
    assert not (s['branch'] == 2).any()
    tab = np.sort(draw[draw <= c])

    def cdf(t):   # frac * exponential(scale) + (1 - frac) * [truncated table, rescaled]
        return frac * -np.expm1(-np.asarray(t) / scale) + (1 - frac) * np.searchsorted(tab, np.asarray(t) / resc, side='right') / len(tab)
    assert stats.kstest(tval, cdf).pvalue > P_MIN
    assert stats.kstest(tval[is_exp], 'expon', args=(0, scale)).pvalue > P_MIN
    assert stats.ks_2samp(tval[~is_exp] / resc, tab).pvalue > P_MIN


def test_velocities_are_normal_and_uncorrelated():
    hd, params = halos(250000, sigma3d=431.0)
    f = 0.9
    halo, s = sats(hd, params, nfw_cases.nfw_table(), {'ELG': dict(f_sigv=f)}, t=1)
    np.testing.assert_array_equal(s['sig'], 431.0 * 0.577 * f)
    zv = np.stack([s['double'][k] for k in ('vx', 'vy', 'vz')], 1) - hd['hvel'][halo]
    zv /= s['sig'][:, None]
    n = len(zv)
    for d in range(3):
        assert stats.kstest(zv[:, d], 'norm').pvalue > P_MIN
        assert abs(zv[:, d].mean()) < 5 / np.sqrt(n) and abs(zv[:, d].var() - 1) < 5 * np.sqrt(2 / n)
    assert np.abs(np.corrcoef(zv.T) - np.eye(3)).max() < 5 / np.sqrt(n)
    u = np.stack([s['double'][k] for k in 'xyz'], 1) - hd['hpos'][halo]     # and independent of the position offset
    assert np.abs(np.corrcoef(np.hstack([zv, u]).T)[:3, 3:]).max() < 5 / np.sqrt(n)


def test_fallback_radii_are_uniform_below_c():
    c = 4.0
    hd, params = halos(100000, c=c, rvir=0.6)
    for draw in (np.array([6.0]), np.random.default_rng(2).uniform(4.5, 12.0, 1000)):
        _, s = sats(hd, params, draw, {'LRG': dict(f_sigv=1.0)}, seed=len(draw))
        assert np.all(s['branch'] == 2)
        eta = s['r'] / 0.6
        assert eta.min() > 0 and eta.max() <= 1.0
        assert stats.kstest(eta, 'uniform').pvalue > P_MIN
    _, s = sats(hd, params, np.array([3.0]), {'LRG': dict(f_sigv=1.0)})      # a one-entry table that is admissible
    assert np.all(s['branch'] == 0)
    np.testing.assert_allclose(s['r'], 3.0 / c * 0.6, rtol=2e-16)


def test_rsd_is_the_python_modulo():
    hd, params = halos(100000)
    L, inv = params['Lbox'], 1 / params['velz2kms']
    draw = nfw_cases.nfw_table()
    tr = {'LRG': dict(f_sigv=1.0)}
    _, a = sats(hd, params, draw, tr, rsd=False)
    _, b = sats(hd, params, draw, tr, rsd=True)
    for k in ('x', 'y', 'vx', 'vy', 'vz'):
        np.testing.assert_array_equal(a['double'][k], b['double'][k])
    zr = a['double']['z'] + a['double']['vz'] * inv
    assert (zr < 0).mean() > 0.3 and (zr > 0).mean() > 0.3                  # both sides of the wrap are exercised
    want = zr % L                                                           # (:787-789), NumPy's % is Python's
    d = np.abs(b['double']['z'] - want)
    assert np.minimum(d, L - d).max() <= 4 * np.spacing(L)
    assert b['double']['z'].min() >= 0 and b['double']['z'].max() <= L
    dl = np.abs(b['longdouble']['z'] - np.asarray(want, dtype=np.longdouble))
    assert np.minimum(dl, L - dl).max() <= 4 * np.spacing(L)


def test_satellite_depends_on_seed_halo_tracer_rank_only():
    hd, params = halos(5000)
    draw = nfw_cases.nfw_table()
    tr = {'LRG': dict(f_sigv=1.0), 'ELG': dict(f_sigv=1.0)}
    halo, a = sats(hd, params, draw, tr)
    perm = np.random.default_rng(0).permutation(len(halo))
    b = oracle.nfw_satellites(hd, tr, params, draw, 11, 0, halo[perm], np.tile(np.arange(4), 5000)[perm], False)
    for k in ('x', 'vz'):
        np.testing.assert_array_equal(a['double'][k][perm], b['double'][k])
        np.testing.assert_array_equal(a['longdouble'][k][perm], b['longdouble'][k])
    assert not np.array_equal(a['double']['x'], sats(hd, params, draw, tr, t=1)[1]['double']['x'])
    assert not np.array_equal(a['double']['x'], sats(hd, params, draw, tr, seed=12)[1]['double']['x'])
    assert not np.array_equal(a['double']['x'], sats(hd, params, draw, tr, index0=2**32)[1]['double']['x'])
    h2 = {k: v[100:] for k, v in hd.items()}
    c = sats(h2, params, draw, tr, index0=100)[1]
    np.testing.assert_array_equal(a['double']['y'][400:], c['double']['y'])
    # the double evaluation stays within a few ulp of the long-double one
    if oracle.ldbl_mant_dig() >= 64:
        for k in 'xyz':
            e = np.abs(a['double'][k] - a['longdouble'][k]) / (np.abs(hd['hpos'][halo, 'xyz'.index(k)]) + a['r'])
            assert 0 < e.max() < 4 * np.finfo(float).eps


def oracle_keep_cent(case, rsd=False):
    p = oracle.marshal_params(case['tracers'], case['params'], False, rsd)
    return oracle.gen_cent(case['hd'], p, 4)[0]


def fragile_fraction(case):
    kc = oracle_keep_cent(case)
    counts, lam, fragile = oracle.nfw_counts(case['hd'], case['tracers'], case['params'], kc, case['seed'], case['index0'])
    assert counts.shape == lam.shape == fragile.shape == (3, len(kc))
    assert np.all(counts[lam == 0] == 0) and np.all(counts >= 0)
    return fragile.mean(), counts, lam


@pytest.mark.parametrize('name', list(nfw_cases.CASES))
def test_fragility_cap(name):
    """a condition on the inputs of the device test, not a measurement: at most 1e-5 of the (halo, tracer) pairs of any
    case may be excluded from the exact count comparison (expected with 32-bit uniforms and a 1.5e-11 window: none)"""
    case = nfw_cases.CASES[name]()
    frac, counts, lam = fragile_fraction(case)
    assert frac <= 1e-5, (name, frac)
    if name == 'small':
        for nh in nfw_cases.SUBSET_NH:
            _, sub = nfw_cases.small_cut(case, nh, lam[1])
            assert fragile_fraction(sub)[0] <= 1e-5, (name, nh)
    if name.startswith('index_'):
        cuts = nfw_cases.SHARD_CUTS
        for a, b in zip(cuts[:-1], cuts[1:]):
            hd, pd = nfw_cases.cut(case['hd'], case['pd'], a, b)
            sub = dict(case, hd=hd, pd=pd, index0=case['index0'] + a)
            f, csub, _ = fragile_fraction(sub)
            assert f <= 1e-5
            np.testing.assert_array_equal(csub, counts[:, a:b])             # sharding-invariant


def test_case_conditions():
    """what the device cases rely on, asserted on the oracle alone"""
    rich = nfw_cases.CASES['rich']()
    _, counts, lam = fragile_fraction(rich)
    assert (lam[1] >= 10).sum() >= 2000 and (lam > 100).any(axis=0).sum() > 0
    assert (np.abs(lam[1] - 10) <= 0.5).sum() >= 100
    nothing = nfw_cases.CASES['no_satellites']()
    _, counts, lam = fragile_fraction(nothing)
    assert not lam.any() and not counts.any()
    mix = nfw_cases.CASES['mix']()
    kc = oracle_keep_cent(mix)
    _, _, lam = fragile_fraction(mix)
    assert set(np.unique(kc[lam[1] > 0])) >= {0, 1, 2}                      # ELG conformity: every branch of the mean


def test_expected_counts_match_the_c_means():
    """oracle.nfw_expected_counts (NumPy; the means tests/test_nfw_gpu.py rests on) against the C `lam`.  Tolerance: each
    side evaluates two or three pow / erfc calls within a few ulp (16 eps for the chain), and `M_h - kappa M_cut`
    amplifies the error of M_cut by M_h / (M_h - kappa M_cut) close to the cut."""
    eps = np.finfo(float).eps
    for name in ('mix', 'rich'):
        case = nfw_cases.CASES[name]()
        kc = oracle_keep_cent(case)
        _, lam, _ = oracle.nfw_counts(case['hd'], case['tracers'], case['params'], kc, 1)
        want = oracle.nfw_expected_counts(case['hd'], case['tracers'], case['params'], kc)
        p = oracle.marshal_params(case['tracers'], case['params'], False, True)
        hd = case['hd']
        m = hd['hmass']
        for t, tr in enumerate(TR):
            pre = tr[0] + '_'
            lc = getattr(p, pre + 'logM_cut') + getattr(p, pre + 'Acent') * hd['hdeltac'] + getattr(p, pre + 'Bcent') * hd['hfenv']
            if tr == 'ELG':
                lc = lc + p.E_Ccent * hd['hshear']
            x = m - getattr(p, pre + 'kappa') * 10 ** lc
            alpha = max(getattr(p, pre + 'alpha'), p.E_alpha_EE, p.E_alpha_EL) if tr == 'ELG' else getattr(p, pre + 'alpha')
            pos = lam[t] > 0
            np.testing.assert_array_equal(want[tr] > 0, pos)
            tol = 16 * eps * (1 + alpha * m[pos] / x[pos])
            rel = np.abs(want[tr][pos] - lam[t][pos]) / lam[t][pos]
            assert np.all(rel <= tol), (name, tr, (rel / tol).max())
            assert pos.sum() > 500
