"""Corner slabs of the seeded prepare path (`prepare_slab_arrays(rng=<seed>)`, csrc/prepare.hip) shared by the CPU tests of the
oracle's seeded mode (tests/test_oracle_prepare.py) and the HIP-vs-oracle matrix (tests/test_prepare_seeded_gpu.py): small
hand-made slabs with the dtypes of `synth.synth_compaso_slabs`, each built for one thing the synthetic slabs never have -
empty slabs and slices, slices at the wave width, a work list longer than the rank kernel's grid, targets at their limits,
degenerate rank keys, a halo that fills the rank kernel's LDS, global indices around 2^32, the reader's dtypes.

`corner(name)` returns a `Corner`: halos, parts, Mpart, h, the seed and index offsets of the call, the MT values it is meant for
and, for the two slabs that must be refused, the error they raise.

Exactness is a property of the inputs: for every slab, every MT it is used with, `checked()` asserts on the CPU that no halo's
mask draw lies within 1e-12 of its kept fraction and that no target expression lies within 1e-9 of an integer (the device's
exp / log10 / pow differ from NumPy's in the last place), that no two halos of a mass bin share a concentration (the reference's
order among equal values is an accident of an unstable sort) - pick another mass or seed if one trips."""
import functools
from dataclasses import dataclass

import numpy as np

from abacusutils_amd import synth
from oracle import prepare_oracle as po

MPART = synth.MPART_BASE
H = 0.6736
LBOX = 300.0
SEED = 20240


@dataclass
class Corner:
    name: str
    halos: dict
    parts: dict
    Mpart: float = MPART
    h: float = H
    seed: int = SEED
    halo_index0: int = 0
    part_index0: int = 0
    MT: tuple = (True, False)
    raises: str = None            # with want_ranks: the message of the error both entry points raise

    @property
    def nh(self):
        return len(self.halos['N'])


def _unit(rng, n):
    u = rng.standard_normal((n, 3))
    return u / np.sqrt((u * u).sum(axis=1))[:, None]


def build(N, npout, seed, Mpart=MPART):
    """a slab of halos of N particles with npout subsample particles each, laid out like synth_compaso_slabs does (same dtypes;
    concentrations distinct, particles never on the centre and never on each other)"""
    rng = np.random.default_rng(seed)
    N = np.asarray(N, dtype=np.uint32)
    npout = np.asarray(npout, dtype=np.int64)
    nh = len(N)
    x = ((rng.random((nh, 3)) - 0.5) * LBOX).astype(np.float32)
    v = (rng.standard_normal((nh, 3)) * 300).astype(np.float32)
    m = N.astype(np.float64) * Mpart
    r98 = np.maximum((0.25 * (m / 1e13) ** (1.0 / 3.0) * (1 + 0.1 * rng.standard_normal(nh))).astype(np.float32), np.float32(0.02))
    conc = (4.0 + 6.0 * rng.random(nh)).astype(np.float32)
    r25 = (r98 / conc).astype(np.float32)
    for _ in range(20):           # distinct float32 concentrations r98 / r25
        c = r98 / r25
        _, first = np.unique(c, return_index=True)
        dup = np.setdiff1d(np.arange(nh), first)
        if len(dup) == 0:
            break
        r25[dup] = (r98[dup] / (4.0 + 6.0 * rng.random(len(dup))).astype(np.float32)).astype(np.float32)
    r90 = (r98 * np.float32(0.8)).astype(np.float32)
    sig = (300.0 * (m / 1e13) ** (1.0 / 3.0)).astype(np.float32)
    npstart = np.concatenate(([0], np.cumsum(npout)[:-1])).astype(np.int64) if nh else np.zeros(0, dtype=np.int64)
    host = np.repeat(np.arange(nh), npout)
    nprt = len(host)
    rr = (r98[host] * (0.02 + 0.98 * rng.random(nprt) ** 1.5))[:, None] * _unit(rng, nprt)
    pos = (x[host] + rr.astype(np.float32)).astype(np.float32).reshape(-1, 3)
    vel = (v[host] + (rng.standard_normal((nprt, 3)) * sig[host][:, None] / np.sqrt(3.0)).astype(np.float32)).astype(np.float32).reshape(-1, 3)
    halos = dict(N=N, x_L2com=x, v_L2com=v, r25_L2com=r25, r90_L2com=r90, r98_L2com=r98, npstartA=npstart, npoutA=npout,
                 id=np.uint64(7 * 10**12) + np.arange(nh, dtype=np.uint64), sigmav3d_L2com=sig)
    return halos, dict(pos=pos, vel=vel)


def n_for_mass(mass, Mpart=MPART):
    return np.rint(np.asarray(mass, dtype=np.float64) / Mpart).astype(np.uint32)


def target_expression(masses, MT):
    """the float the reference truncates to the target count (:152-174), NaN below the mass floor"""
    x = np.log10(masses)
    with np.errstate(over='ignore'):
        if MT:
            return np.where(masses < 1e11, np.nan, 1 + 1.5 * 10 ** (x - 12.5))
        return np.where(10 ** x < 1e12, np.nan, 1 + 1.5 * 10 ** (x - 13))


def n_for_target(t, MT, Mpart=MPART):
    """a particle count whose target expression lies near t + 0.5"""
    return int(n_for_mass(10 ** ((12.5 if MT else 13.0) + np.log10((t + 0.5 - 1) / 1.5)), Mpart))


def checked(c):
    """the conditions on the inputs under which device and restatement agree exactly"""
    masses = c.halos['N'] * c.Mpart
    mbins = np.logspace(np.log10(1e11), 15.5, po.NBINS + 1)
    bins = np.searchsorted(mbins, masses)
    conc = np.asarray(c.halos['r98_L2com']) / np.asarray(c.halos['r25_L2com'])
    assert c.nh == 0 or len(np.unique(np.stack([bins.astype(np.float64), conc.astype(np.float64)]), axis=1).T) == c.nh, (c.name, 'equal concentrations in a bin')
    if c.nh:
        u = po.device_uniform_vec(c.seed, c.halo_index0 + np.arange(c.nh, dtype=np.int64), 6)
        for MT in c.MT:
            p = po.subsample_halos(masses, MT)
            assert np.abs(u - p).min() >= 1e-12, (c.name, MT, 'a mask draw on its threshold')
            t = target_expression(masses, MT)
            t = t[np.isfinite(t) & (t < 1e6)]
            assert len(t) == 0 or np.abs(t - np.rint(t)).min() >= 1e-9, (c.name, MT, 'a target on an integer')
    a, n = np.asarray(c.halos['npstartA']).astype(np.int64), np.asarray(c.halos['npoutA']).astype(np.int64)
    if c.raises is None or 'outside' not in c.raises:
        assert np.all(a >= 0) and np.all(a + n <= len(c.parts['pos']))
    return c


# ---- the slabs ------------------------------------------------------------------------------------------------------------------
def _mixed(seed=11, nh=240):
    """a few hundred halos over every branch of the kept fraction and the targets, a few without subsample particles"""
    rng = np.random.default_rng(seed)
    logm = np.minimum(10.9 + rng.exponential(0.7, nh), 15.2)
    N = np.maximum((10 ** logm / MPART).astype(np.int64), 35)
    npout = rng.binomial(N, 0.03)
    npout[rng.random(nh) < 0.05] = 0
    return build(N, npout, seed)


def _empty(with_particles):
    halos, parts = build([], [], 1)
    if with_particles:
        parts = build([20000], [9], 2)[1]
    return Corner('empty', halos, parts)


def _no_particles():
    halos, parts = build(n_for_mass(10 ** np.linspace(11.0, 14.5, 37)), np.zeros(37, dtype=np.int64), 3)
    assert len(parts['pos']) == 0 and parts['pos'].shape == (0, 3)
    return Corner('no_particles', halos, parts)


def _none_kept():
    # particles of 1e5 Msun: halos of 35 .. 99 particles have a kept fraction of 1e-20 and less
    N = np.arange(35, 100)
    halos, parts = build(N, np.full(len(N), 3), 4, Mpart=1e5)
    c = Corner('none_kept', halos, parts, Mpart=1e5)
    for MT in (True, False):
        assert po.subsample_halos(N * 1e5, MT).max() < 1e-19
    return c


def _kept_without_particles():
    # below the particle mass floor of the LRG sample (1e12) but kept by most draws (fraction 0.9 and more), next to heavy halos
    # that have no subsample particles at all
    rng = np.random.default_rng(5)
    mass = np.concatenate([10 ** rng.uniform(11.8, 11.99, 60), 10 ** rng.uniform(13.1, 14.0, 20)])
    npout = np.concatenate([rng.integers(1, 9, 60), np.zeros(20, dtype=np.int64)])
    order = rng.permutation(80)
    halos, parts = build(n_for_mass(mass[order]), npout[order], 5)
    c = Corner('kept_without_particles', halos, parts, MT=(False,))
    m = halos['N'] * MPART
    assert np.all((m < 1e12) | (halos['npoutA'] == 0))
    return c


def _single(k):
    halos, parts = build([n_for_target(7, False)], [k], 6 + k)
    return Corner(f'single_{k}', halos, parts)


WAVE_SLICES = (1, 2, 63, 64, 65, 127, 128, 129, 1000)


def _wave_edges():
    # slices around one and two waves, each as a halo that keeps a few, one that keeps most and one that keeps all of its slice;
    # between them halos that are not kept and halos without particles
    N, npout = [], []
    for s in WAVE_SLICES:
        for t in (3, max(s - 2, 1), s + 5):
            N.append(n_for_target(min(t, 1400), False))
            npout.append(s)
        N += [60, n_for_target(9, False)]
        npout += [4, 0]
    return Corner('wave_edges', *build(N, npout, 8))


def _halo_count(nh):
    rng = np.random.default_rng(20 + nh)
    N = [n_for_target(t, False) for t in rng.integers(2, 40, nh)]
    return Corner(f'halos_{nh}', *build(N, rng.integers(1, 70, nh), 20 + nh))


def _many_halos():
    # more halos of two particles than four times the per-halo kernels' grid (one workgroup takes four halos, 2048 blocks), a
    # third of them keeping both particles - more than the rank kernel's 2048 blocks - the others one (the restatement's rank
    # loop takes 0.6 ms a halo: 2700 of them, not 8197)
    nh = 8197
    rng = np.random.default_rng(9)
    both = np.arange(nh) % 3 == 0
    N = np.where(both, n_for_target(2, False) + rng.integers(0, 600, nh), n_for_target(1, False) + rng.integers(0, 300, nh))
    c = Corner('many_halos', *build(N, np.full(nh, 2), 9), MT=(False,))
    t = target_expression(c.halos['N'] * MPART, False).astype(int)
    assert np.array_equal(t, np.where(both, 2, 1)) and nh // 4 > 2048 and both.sum() > 2048
    return c


def _targets(MT):
    # ntarget == n_in, n_in - 1 and 1; n_in one below the target
    ts = (2, 3, 17, 64, 65, 90)
    N, npout = [], []
    for t in ts:
        n = n_for_target(t, MT)
        N += [n, n, n]
        npout += [t, t + 1, max(t - 1, 1)]
    N += [n_for_target(1, MT)] * 3
    npout += [1, 2, 40]
    c = Corner('targets_mt' if MT else 'targets_lrg', *build(N, npout, 30 + MT), MT=(MT,))
    want = np.repeat(ts + (1,), 3)
    got = target_expression(c.halos['N'] * MPART, MT).astype(int)
    assert np.array_equal(got, want), (got, want)
    return c


def _mt_cap():
    # 1 + 1.5 10^(x - 12.5) far above 100: the ELG sample keeps 100 at most
    N = [n_for_mass(m) for m in (3.1e14, 5.3e14, 9.7e14)]
    c = Corner('mt_cap', *build(N, [100, 101, 5000], 32))
    assert np.all(target_expression(c.halos['N'] * MPART, True) > 100)
    return c


def _lrg_floor():
    # particles of 2e9 Msun: 500 of them are exactly the LRG sample's floor of 1e12, 499 and 501 lie a particle either side
    c = Corner('lrg_floor', *build([499, 500, 501, 499, 500, 501], [5, 5, 5, 1, 1, 1], 33, Mpart=2e9), Mpart=2e9, MT=(False,))
    m = c.halos['N'] * 2e9
    assert m[1] == 1e12 and np.log10(m[1]) == 12.0 and 10 ** np.log10(m[1]) == 1e12
    assert [po.particle_target(mm, 5, False) for mm in m[:3]] == [0, 1, 1]
    # every halo kept, so that the floor decides: pick the seed
    for seed in range(100):
        c.seed = seed
        if np.all(po.device_uniform_vec(seed, np.arange(6), 6) < po.subsample_halos(m, False)):
            return c
    raise AssertionError('no seed keeps all six halos')


def _rank_keys():
    # heavy halos that keep their whole slice, so that the kept particles are chosen here: one on the halo centre (r0 == 0: NaN
    # radial velocity), two identical ones (ties in all five columns, nearest neighbour at distance 0), one at rest relative to the
    # halo (v_tan2 + v_rad2 == 0: NaN perihelion, x2 := 1); and a halo that keeps 2 of 1000, their nearest neighbours being
    # looked for among the thousand
    big = n_for_mass(2.2e15)
    halos, parts = build([big, big, big, big, n_for_target(2, False)], [6, 7, 5, 9, 1000], 34)
    a = halos['npstartA']
    pos, vel = parts['pos'], parts['vel']
    pos[a[0] + 2] = halos['x_L2com'][0]
    pos[a[1] + 4], vel[a[1] + 4] = pos[a[1] + 1], vel[a[1] + 1]
    vel[a[2] + 3] = halos['v_L2com'][2]
    pos[a[3] + 5], vel[a[3] + 5] = halos['x_L2com'][3], halos['v_L2com'][3]     # both at once
    pos[a[3] + 7], vel[a[3] + 7] = pos[a[3] + 0], vel[a[3] + 0]
    c = Corner('rank_keys', halos, parts)
    assert target_expression(halos['N'][4:] * MPART, False).astype(int)[0] == 2
    return c


def _lds(over):
    # one halo whose kept particles fill the rank kernel's shared memory: 12 k + pad + 40 k bytes for k kept particles, guard at
    # 160 KB (k <= 3150).  k = 2800 .. 3000 takes 146 - 156 KB; k >= 3151 must be refused
    t = 3190 if over else 2900
    halos, parts = build([n_for_target(t, False), n_for_target(5, False)], [4000, 12], 35)
    target = po.particle_target(halos['N'][0] * MPART, 4000, False)
    if over:
        assert target >= 3151
        return Corner('lds_over', halos, parts, MT=(False,), raises="exceed the rank kernel's LDS")
    assert 2800 <= target <= 3000
    lds = (3 * target * 4 + 15) // 16 * 16 + 5 * target * 8
    assert 146 * 1024 <= lds <= 156 * 1024, lds
    return Corner('lds_big', halos, parts, MT=(False,))


def _offsets(name):
    kw = {'index_below': dict(halo_index0=2**32 - 100, part_index0=2**32 - 1000),      # the slab straddles 2^32 in both
          'index_above': dict(halo_index0=2**32 + 3, part_index0=2**33 + 11),
          'seed_high': dict(seed=2**63 + 5),
          'seed_negative': dict(seed=-1)}[name]
    halos, parts = _mixed(seed={'index_below': 41, 'index_above': 42, 'seed_high': 43, 'seed_negative': 44}[name])
    c = Corner(name, halos, parts, **kw)
    if name == 'index_below':
        assert c.nh > 100 and len(parts['pos']) > 1000
    return c


def _reader_dtypes(id_dtype):
    halos, parts = _mixed(seed=45)
    halos['npstartA'] = halos['npstartA'].astype(np.uint64)
    halos['npoutA'] = halos['npoutA'].astype(np.uint32)
    halos['id'] = halos['id'].astype(id_dtype)
    return Corner(f'reader_{np.dtype(id_dtype).name}', halos, parts)


def _strided():
    halos, parts = _mixed(seed=46)
    out = {}
    for k, v in halos.items():
        wide = np.zeros((len(v), 2) + v.shape[1:], dtype=v.dtype)
        wide[:, 0] = v
        out[k] = wide[:, 0]
    pp = {}
    for k, v in parts.items():
        wide = np.zeros((len(v), 5), dtype=v.dtype)
        wide[:, 1:4] = v
        pp[k] = wide[:, 1:4]
    assert not out['N'].flags.c_contiguous and not out['x_L2com'].flags.c_contiguous and not pp['pos'].flags.c_contiguous
    return Corner('strided', out, pp)


def _bad_slice(kind):
    # a kept halo (the heaviest: kept fraction 1) whose slice ends one particle behind the array / starts at -1
    halos, parts = _mixed(seed=47)
    j = int(np.argmax(halos['N']))
    assert halos['N'][j] * MPART > 1e13 and halos['npoutA'][j] > 0
    if kind == 'overshoot':
        last = int(np.argmax(halos['npstartA'] + halos['npoutA']))
        halos['N'][last] = halos['N'][j]                    # (the last slice of the array, made a kept halo's)
        halos['npoutA'][last] = halos['npoutA'][last] + 1
        assert halos['npstartA'][last] + halos['npoutA'][last] == len(parts['pos']) + 1
    else:
        halos['npstartA'][j] = -1
    return Corner(f'slice_{kind}', halos, parts, raises='lies outside the particle array')


_BUILDERS = {
    'empty': lambda: _empty(False), 'empty_with_particles': lambda: _empty(True), 'no_particles': _no_particles,
    'none_kept': _none_kept, 'kept_without_particles': _kept_without_particles, 'single_1': lambda: _single(1),
    'single_2': lambda: _single(2), 'wave_edges': _wave_edges, 'halos_1': lambda: _halo_count(1), 'halos_3': lambda: _halo_count(3),
    'halos_4': lambda: _halo_count(4), 'halos_5': lambda: _halo_count(5), 'many_halos': _many_halos,
    'targets_mt': lambda: _targets(True), 'targets_lrg': lambda: _targets(False), 'mt_cap': _mt_cap, 'lrg_floor': _lrg_floor,
    'rank_keys': _rank_keys, 'lds_big': lambda: _lds(False), 'lds_over': lambda: _lds(True),
    'index_below': lambda: _offsets('index_below'), 'index_above': lambda: _offsets('index_above'),
    'seed_high': lambda: _offsets('seed_high'), 'seed_negative': lambda: _offsets('seed_negative'),
    'reader_uint64': lambda: _reader_dtypes(np.uint64), 'reader_int64': lambda: _reader_dtypes(np.int64), 'strided': _strided,
    'mixed': lambda: Corner('mixed', *_mixed()),
    'slice_overshoot': lambda: _bad_slice('overshoot'), 'slice_minus_one': lambda: _bad_slice('minus_one'),
}
ERRORS = ('lds_over', 'slice_overshoot', 'slice_minus_one')
CORNERS = [k for k in _BUILDERS if k not in ERRORS]      # the slabs both device paths must prepare like the oracle


@functools.lru_cache(maxsize=None)
def corner(name):
    c = _BUILDERS[name]()
    c.name = name
    return checked(c)


def shear_field(ndim=64, seed=5):
    return np.random.default_rng(seed).random((ndim, ndim, ndim))


def shear_has_no_ties(c, shearmark):
    """no two halos of a mass bin in one cell of the shear field (equal values rank in the unstable sort's order in the reference)"""
    ndim = len(shearmark)
    g = (c.halos['x_L2com'] / (LBOX / ndim)).astype(int) % ndim
    bins = np.searchsorted(np.logspace(11, 15.5, po.NBINS + 1), c.halos['N'] * c.Mpart)
    code = ((bins * ndim + g[:, 0]) * ndim + g[:, 1]) * ndim + g[:, 2]
    return len(np.unique(code)) == c.nh


def want_AB(c):
    """the concentration ranks are worth comparing where a mass bin holds two halos or more"""
    bins = np.searchsorted(np.logspace(11, 15.5, po.NBINS + 1), c.halos['N'] * c.Mpart)
    return c.nh > 0 and int(np.bincount(bins).max()) >= 2


@functools.lru_cache(maxsize=None)
def synthetic():
    """the one slab of ordinary size: 6000 halos of the synthetic catalogue"""
    slabs, header = synth.synth_compaso_slabs(numslabs=1, n_halo=6000, seed=61, lbox=LBOX)
    return checked(Corner('synthetic', slabs[0]['halos'], slabs[0]['parts'], Mpart=header['ParticleMassHMsun'], h=header['H0'] / 100.0,
                          seed=4242, halo_index0=2**32 + 3, part_index0=2**33 + 11))


@functools.lru_cache(maxsize=None)
def oracle_tables(name, MT, shear=False, rank_log=None):
    """the seeded restatement's tables of a corner (with the rank columns; the tables without them are these without the five
    columns), computed once per session"""
    c = synthetic() if name == 'synthetic' else corner(name)
    kw = {} if rank_log is None else {'rank_log': rank_log}
    with np.errstate(all='ignore'):
        return po.prepare_slab_core(c.halos, c.parts, c.Mpart, c.h, MT, want_ranks=True, want_AB=want_AB(c),
                                    shearmark=shear_field() if shear else None, Lbox=LBOX, rng=c.seed, halo_index0=c.halo_index0,
                                    part_index0=c.part_index0, **kw)


def without_ranks(P):
    return {k: v for k, v in P.items() if k not in ('ranks', 'ranksv', 'ranksp', 'ranksr', 'ranksc')}


def log_rounded_once(a):
    """the float32 logarithm as the device takes it: the float64 logarithm, rounded once"""
    a = np.asarray(a)
    return np.log(a.astype(np.float64)).astype(a.dtype) if a.dtype == np.float32 else np.log(a)
