"""MI355X drop-in for `abacusnbody.hod.abacus_hod.AbacusHOD` (reference: abacusnbody/hod/abacus_hod.py).

Same constructor, attributes and method signatures for the calls on the hot path:

    run_hod            (:706-859)   -> gen_gal_cat on the device-resident subsample (csrc/hod.hip)
    compute_power      (:1338-1472) -> calc_power (csrc/tsc.hip, power.hip)
    compute_xirppi / compute_wp / compute_multipole / compute_clustering  (:1181-1336, :1826-1885) -> csrc/pairs.hip
    compute_ngal       (:861-1179)  the same sums as one pass over the staged halos on the device (abacus_hod_ngal)

The halo/particle subsample is uploaded to HBM on the first `run_hod` and stays there (the reference keeps it in
host RAM across calls, :193-197); `reseed` rewrites the three random arrays in HBM with the device Philox generator
and mirrors them to the host dicts (:824-835).
`AbacusHOD.from_arrays` builds the object from in-memory arrays (tests, synthetic data); the regular constructor
runs `staging()` (needs h5py for the `halos_xcom_*`/`particles_xcom_*` files).
ZCV: the fields, their advection and the spectra are in `abacusutils_amd.hod.zcv`; `apply_zcv*` (the combination with the
ZeNBu model) is not provided.
"""
import logging
import math
import time
from pathlib import Path

import numpy as np

from ..analysis.power_spectrum import calc_power
from ..analysis.tpcf_corrfunc import (calc_multipole_fast, calc_multipole_lc, calc_wp_fast, calc_wp_lc, calc_xirppi_fast,
                                      calc_xirppi_lc)
from .GRAND_HOD import StagedCatalog, gen_gal_cat

_PRIMARY_Z = [3.0, 2.5, 2.0, 1.7, 1.4, 1.1, 0.8, 0.5, 0.4, 0.3, 0.2, 0.1, 0.0]
_SECONDARY_Z = [0.15, 0.25, 0.35, 0.45, 0.575, 0.65, 0.725, 0.875, 0.95, 1.025, 1.175, 1.25, 1.325, 1.475, 1.55,
                1.625, 1.85, 2.25, 2.75, 3.0, 5.0, 8.0]


def _read_asdf_header(fn):
    """`header` mapping of an Abacus ASDF file without the asdf package: the tree is YAML ahead of the first block"""
    import re

    import yaml
    raw = open(fn, 'rb').read()
    end = raw.find(b'\n...')
    text = raw[: end if end >= 0 else len(raw)].decode('utf-8', errors='replace')
    text = re.sub(r'!\S+', '', text)  # drop YAML tags (core/asdf, core/ndarray, ...)
    text = '\n'.join(line for line in text.splitlines() if not line.startswith('%') and not line.startswith('#'))
    tree = yaml.safe_load(text)
    return tree['header']


def _i8(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _searchsorted(a, b):
    """`_searchsorted_parallel` (:588): np.searchsorted(a, b) on the device (abacus_searchsorted_i64)"""
    import ctypes as C

    from .. import _lib
    a, b = _i8(a), _i8(b)
    out = np.empty(len(b), dtype=np.int64)
    _lib.check(_lib.lib().abacus_searchsorted_i64(_lib.ptr(a), C.c_int64(len(a)), _lib.ptr(b), C.c_int64(len(b)), _lib.ptr(out)))
    return out


def _argsort_ids(ids):
    """the halo sort by id (:566-585) on the device (abacus_argsort_i64: stable radix sort)"""
    import ctypes as C

    from .. import _lib
    ids = _i8(ids)
    out = np.empty(len(ids), dtype=np.int64)
    _lib.check(_lib.lib().abacus_argsort_i64(_lib.ptr(ids), C.c_int64(len(ids)), _lib.ptr(out)))
    return out


def calc_fenv_opt(Menv, mbins, halosM):
    """global environment rank per mass bin (:1961-1970) on the device (abacus_fenv_rank)"""
    import ctypes as C

    from .. import _lib
    f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64)   # noqa: E731
    Menv, mbins, halosM = f8(Menv), f8(mbins), f8(halosM)
    out = np.empty(len(Menv), dtype=np.float64)
    _lib.check(_lib.lib().abacus_fenv_rank(_lib.ptr(Menv), _lib.ptr(halosM), C.c_int64(len(Menv)), _lib.ptr(mbins), len(mbins),
                                         _lib.ptr(out)))
    return out


def _concat_tables(tabs):
    """rows of the slabs' subsample tables: HDF5 compound arrays or dicts of columns"""
    if isinstance(tabs[0], dict):
        return {k: np.concatenate([np.asarray(t[k]) for t in tabs]) for k in tabs[0]}
    return np.concatenate(tabs)


def _table_fields(tab):
    return tab.keys() if isinstance(tab, dict) else tab.dtype.fields.keys()


class AbacusHOD:
    """A multi-tracer HOD code for the AbacusSummit simulations (MI355X path)."""

    # Extensions of the reference class (both off = the reference's behaviour):
    # lazy_columns: run_hod() returns at once with the galaxy columns still in HBM; they are copied to NumPy at the first
    #   read (GRAND_HOD.LazyTracer) and only until the next run_hod() - an MCMC step that feeds the mock straight into
    #   compute_power / compute_xirppi / compute_wp / compute_multipole never pays the PCIe copy.
    # reseed_sync_host: after `run_hod(reseed=...)` copy the redrawn random columns back into halo_data / particle_data
    #   like the reference mutates them (True), or leave them on the device only (False).
    lazy_columns = False
    reseed_sync_host = True

    def __init__(self, sim_params, HOD_params, clustering_params=None, chunk=-1, n_chunks=1, skip_staging=False):
        self.logger = logging.getLogger('AbacusHOD')
        self.sim_name = sim_params['sim_name']
        self.sim_dir = sim_params['sim_dir']
        self.subsample_dir = sim_params['subsample_dir']
        self.z_mock = sim_params['z_mock']
        self.output_dir = sim_params.get('output_dir', './')
        self.halo_lc = sim_params.get('halo_lc', False)
        self.force_mt = sim_params.get('force_mt', False)
        self.local_env = sim_params.get('local_env', {})

        if self.halo_lc:
            ztype = 'lightcone'
        elif self.z_mock in _PRIMARY_Z:
            ztype = 'primary'
        elif self.z_mock in _SECONDARY_Z:
            ztype = 'secondary'
        else:
            raise Exception('illegal redshift')
        self.z_type = ztype
        self._init_hod(HOD_params, clustering_params)
        self.chunk = chunk
        self.n_chunks = n_chunks
        assert self.chunk < self.n_chunks, 'Total number of chunks needs to be larger than current chunk index'
        self._staged = None
        if not skip_staging:
            self.halo_data, self.particle_data, self.params, self.mock_dir = self.staging()
            self._build_mass_function()
        else:
            raise NotImplementedError('skip_staging=True needs abacusnbody.metadata (out of the hot-path scope); '
                                      'use AbacusHOD.from_arrays for in-memory data')

    def _init_hod(self, HOD_params, clustering_params):
        tracer_flags = HOD_params['tracer_flags']
        tracers = {}
        for key in tracer_flags.keys():
            if tracer_flags[key]:
                tracers[key] = HOD_params[key + '_params']
        self.tracers = tracers
        self.want_ranks = HOD_params.get('want_ranks', False)
        self.want_AB = HOD_params.get('want_AB', False)
        self.want_shear = HOD_params.get('want_shear', False)
        self.want_expvel = HOD_params.get('want_expvel', False)
        self.want_rsd = HOD_params['want_rsd']
        if clustering_params is not None:
            self.pimax = clustering_params.get('pimax', None)
            self.pi_bin_size = clustering_params.get('pi_bin_size', None)
            bin_params = clustering_params['bin_params']
            self.rpbins = np.logspace(bin_params['logmin'], bin_params['logmax'], bin_params['nbins'] + 1)
            self.clustering_type = clustering_params.get('clustering_type', None)

    @classmethod
    def from_arrays(cls, halo_data, particle_data, params, HOD_params, clustering_params=None, mock_dir='./',
                    z_type='primary'):
        """Build the object from the dictionaries `staging()` would produce (hod/abacus_hod.py:659-704)."""
        self = cls.__new__(cls)
        self.logger = logging.getLogger('AbacusHOD')
        self.sim_name = self.sim_dir = self.subsample_dir = None
        self.z_mock = params['z']
        self.output_dir = str(mock_dir)
        self.halo_lc = params.get('origin', None) is not None
        self.force_mt = False
        self.local_env = {}
        self.z_type = 'lightcone' if self.halo_lc else z_type
        self._init_hod(HOD_params, clustering_params)
        self.chunk, self.n_chunks = params.get('chunk', -1), 1
        self.halo_data, self.particle_data, self.params = halo_data, particle_data, params
        self.mock_dir = Path(mock_dir)
        self.lbox = params['Lbox']
        self._staged = None
        if self.want_AB:
            assert 'hfenv' in self.halo_data.keys()
            assert 'hdeltac' in self.halo_data.keys()
        if self.want_shear:
            assert 'hshear' in self.halo_data.keys()
        self._build_mass_function()
        return self

    @classmethod
    def from_prepared(cls, halo_tables, particle_tables, header, z_mock, HOD_params, clustering_params=None, env=None,
                      mock_dir='./', halo_lc=False):
        """Build the object straight from the subsample tables of prepare_sim (`prepare_slab_arrays` of
        abacusutils_amd/hod/prepare_sim.py, one pair per slab) - what `staging()` reads back from the HDF5 files, without the
        files.  header: BoxSize, ParticleMassHMsun, H0, VelZSpace_to_kms (+ LightConeOrigins) of the simulation; env: the
        concatenated (id, mass, Menv) of `slab_environment` over ALL slabs of the box (needed with want_AB, :595-657)."""
        self = cls.__new__(cls)
        self.logger = logging.getLogger('AbacusHOD')
        self.sim_name = self.sim_dir = self.subsample_dir = None
        self.z_mock = z_mock
        self.output_dir = str(mock_dir)
        self.halo_lc = bool(halo_lc)
        self.force_mt = False
        self.local_env = {}
        self.z_type = 'lightcone' if self.halo_lc else 'primary'
        self._init_hod(HOD_params, clustering_params)
        self.chunk, self.n_chunks = -1, 1
        params = {'z': z_mock, 'h': header['H0'] / 100.0, 'Lbox': header['BoxSize'], 'Mpart': header['ParticleMassHMsun'],
                  'velz2kms': header['VelZSpace_to_kms'] / header['BoxSize'], 'chunk': -1, 'numslabs': len(halo_tables),
                  'origin': np.array(header['LightConeOrigins']).reshape(-1, 3)[0] if self.halo_lc else None}
        if self.want_AB and not self.halo_lc and env is None:
            raise ValueError('want_AB needs the environment masses of the whole box (prepare_sim.slab_environment per slab)')
        self.halo_data, self.particle_data = self._assemble_staged(list(halo_tables), list(particle_tables), env, params, True)
        self.params = params
        self.mock_dir = Path(mock_dir)
        self.lbox = params['Lbox']
        self._staged = None
        self._build_mass_function()
        return self

    def _build_mass_function(self):
        """weighted halo histograms used by compute_ngal (:199-251)"""
        hd = self.halo_data
        n = len(hd['hmass'])
        self.logMbins = np.linspace(np.log10(np.min(hd['hmass'])), np.log10(np.max(hd['hmass'])), 101)
        self.deltacbins = np.linspace(-0.5, 0.5, 101)
        self.fenvbins = np.linspace(-0.5, 0.5, 101)
        self.shearbins = np.linspace(-0.5, 0.5, 101)
        cols = (np.log10(hd['hmass']), hd.get('hdeltac', np.zeros(n)), hd.get('hfenv', np.zeros(n)))
        self.halo_mass_func, _ = np.histogramdd(np.vstack(cols).T, bins=[self.logMbins, self.deltacbins, self.fenvbins],
                                                weights=hd['hmultis'])
        self._mass_func_wshear = None  # 100^4 histogram, built on first ELG compute_ngal

    @property
    def halo_mass_func_wshear(self):
        if self._mass_func_wshear is None:
            hd = self.halo_data
            n = len(hd['hmass'])
            cols = (np.log10(hd['hmass']), hd.get('hdeltac', np.zeros(n)), hd.get('hfenv', np.zeros(n)),
                    hd.get('hshear', np.zeros(n)))
            self._mass_func_wshear, _ = np.histogramdd(
                np.vstack(cols).T, bins=[self.logMbins, self.deltacbins, self.fenvbins, self.shearbins],
                weights=hd['hmultis'])
        return self._mass_func_wshear

    # ------------------------------------------------------------------------------------------------------
    def staging(self):
        """Load the halo+particle subsamples (hod/abacus_hod.py:253-704) into the float64 dictionaries the
        population kernels consume."""
        try:
            import h5py
        except ImportError as e:
            raise ImportError('AbacusHOD.staging() reads the prepare_sim HDF5 subsamples and needs h5py; '
                              'use AbacusHOD.from_arrays for in-memory data') from e
        output_dir = Path(self.output_dir)
        simname = Path(self.sim_name)
        sim_dir = Path(self.sim_dir)
        mock_dir = output_dir / simname / ('z%4.3f' % self.z_mock)
        subsample_dir = Path(self.subsample_dir) / simname / ('z%4.3f' % self.z_mock)
        if not (sim_dir / simname).exists():
            raise FileNotFoundError(f'Simulation directory {sim_dir / simname} not found.')
        if not subsample_dir.exists():
            raise FileNotFoundError(f'Subsample directory {subsample_dir} not found.')
        if self.halo_lc:
            halo_info_fns = [str(sim_dir / simname / ('z%4.3f' % self.z_mock) / 'lc_halo_info.asdf')]
        else:
            halo_info_fns = list((sim_dir / simname / 'halos' / ('z%4.3f' % self.z_mock) / 'halo_info').glob('*.asdf'))
        header = _read_asdf_header(halo_info_fns[0])

        params = {}
        params['z'] = self.z_mock
        params['h'] = header['H0'] / 100.0
        params['Lbox'] = header['BoxSize']
        params['Mpart'] = header['ParticleMassHMsun']
        params['velz2kms'] = header['VelZSpace_to_kms'] / params['Lbox']
        if self.halo_lc:
            params['origin'] = np.array(header['LightConeOrigins']).reshape(-1, 3)[0]
        else:
            params['origin'] = None
        n_chunks = self.n_chunks
        params['chunk'] = self.chunk
        chunk = 0 if self.chunk == -1 else self.chunk
        n_jump = int(np.ceil(len(halo_info_fns) / n_chunks))
        start = chunk * n_jump
        end = min((chunk + 1) * n_jump, len(halo_info_fns))
        params['numslabs'] = end - start
        self.lbox = header['BoxSize']

        def fnames(eslab):
            if ('ELG' not in self.tracers) and ('QSO' not in self.tracers) and (not self.force_mt):
                h = subsample_dir / ('halos_xcom_%d_seed600_abacushod_oldfenv' % eslab)
                p = subsample_dir / ('particles_xcom_%d_seed600_abacushod_oldfenv' % eslab)
            else:
                h = subsample_dir / ('halos_xcom_%d_seed600_abacushod_oldfenv_MT' % eslab)
                p = subsample_dir / ('particles_xcom_%d_seed600_abacushod_oldfenv_MT' % eslab)
            if self.want_ranks:
                p = str(p) + '_withranks'
            return str(h) + '_new.h5', str(p) + '_new.h5'

        with_parts = self.z_type in ('primary', 'lightcone')
        H, P = [], []
        for eslab in range(start, end):
            self.logger.info(f'Loading simulation slab {eslab}')
            hfn, pfn = fnames(eslab)
            with h5py.File(hfn, 'r') as f:
                H.append(f['halos'][:])
            if with_parts:
                with h5py.File(pfn, 'r') as f:
                    P.append(f['particles'][:])
        env = None
        if self.want_AB and (not self.halo_lc):
            ids, masses, menvs = [], [], []
            for eslab in range(len(halo_info_fns)):
                envfilename = subsample_dir / f'env_xcom_{eslab}_abacushod_localenv_new.h5'
                if not envfilename.exists():
                    raise FileNotFoundError(f'Missing env sidecar: {envfilename}')
                with h5py.File(envfilename, 'r') as fenv:
                    ids.append(fenv['id'][:].astype(np.int64))
                    masses.append(fenv['mass'][:])
                    menvs.append(fenv['Menv'][:])
            env = (np.concatenate(ids), np.concatenate(masses), np.concatenate(menvs))
        halo_data, particle_data = self._assemble_staged(H, P, env, params, with_parts)
        return halo_data, particle_data, params, mock_dir

    def _assemble_staged(self, H, P, env, params, with_parts):
        """the arrays of `halo_data` / `particle_data` from the subsample tables of the loaded slabs (:421-704).  H / P: one
        table per slab (HDF5 compound arrays, or dicts of columns as prepare_sim.prepare_slab_arrays returns them); env: the
        concatenated (id, mass, Menv) of the env sidecars of ALL slabs of the box, or None"""
        Hc = _concat_tables(H)
        f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
        hpos, hvel = f8(Hc['x_L2com']), f8(Hc['v_L2com'])
        hmass = f8(Hc['N'] * params['Mpart'])
        hid = Hc['id'].astype(int)
        hmultis, hrandoms = f8(Hc['multi_halos']), f8(Hc['randoms'])
        vdev = Hc['randoms_exp'] if self.want_expvel else Hc['randoms_gaus_vrms']
        if vdev.ndim == 1:
            self.logger.warning('Warning: galaxy x, y velocity bias randoms not set, using z randoms instead. '
                                'x, y velocities may be unreliable.')
            vdev = np.concatenate((vdev, vdev, vdev)).reshape(-1, 3)
        hveldev = f8(vdev)
        hsigma3d = f8(Hc['sigmav3d_L2com'])
        hc = f8(Hc['r98_L2com'] / Hc['r25_L2com'])
        hrvir = f8(Hc['r98_L2com'])
        hdeltac = f8(Hc['deltac_rank']) if self.want_AB else None
        hfenv = f8(Hc['fenv_rank']) if self.want_AB else None
        hshear = f8(Hc['shear_rank']) if self.want_shear else None

        particle_data = {}
        if with_parts:
            Pc = _concat_tables(P)
            fields = _table_fields(Pc)
            ppos, pvel, phvel = f8(Pc['pos']), f8(Pc['vel']), f8(Pc['halo_vel'])
            phmass = f8(Pc['halo_mass'])
            phid = Pc['halo_id'].astype(int)
            pNp, psub, prandoms = f8(Pc['Np']), f8(Pc['downsample_halo']), f8(Pc['randoms'])
            pdeltac = f8(Pc['halo_deltac']) if self.want_AB else None
            pfenv = f8(Pc['halo_fenv']) if self.want_AB else None
            pshear = f8(Pc['halo_shear']) if self.want_shear else None
            ranks = {}
            if self.want_ranks:
                assert 'ranks' in fields and 'ranksv' in fields
                for src, dst in (('ranks', 'pranks'), ('ranksv', 'pranksv'), ('ranksp', 'pranksp'),
                                 ('ranksr', 'pranksr'), ('ranksc', 'pranksc')):
                    ranks[dst] = f8(Pc[src]) if src in fields else np.zeros(len(Pc))
        # sort halos by id, important for conformity (:566-585)
        if not np.all(hid[:-1] <= hid[1:]):
            self.logger.info('Sorting halos for conformity calculation.')
            s = _argsort_ids(hid)
            hpos, hvel, hmass, hid, hmultis, hrandoms, hveldev, hsigma3d, hc, hrvir = (
                a[s] for a in (hpos, hvel, hmass, hid, hmultis, hrandoms, hveldev, hsigma3d, hc, hrvir))
            if self.want_AB:
                hdeltac, hfenv = hdeltac[s], hfenv[s]
            if self.want_shear:
                hshear = hshear[s]
        assert np.all(hid[:-1] <= hid[1:])
        if with_parts:
            pweights = 1 / pNp / psub
            pinds = _searchsorted(hid, phid)

        # global environment ranking from the env sidecars (:595-657)
        if self.want_AB and (not self.halo_lc):
            mcut_env = self.local_env.get('mcut', 1e11)
            nbins_env = self.local_env.get('nbins', 100)
            env_id, env_mass, env_Menv = env
            mbins_env = np.logspace(np.log10(mcut_env), 15.5, nbins_env + 1)
            hfenv_full = calc_fenv_opt(env_Menv, mbins_env, env_mass)
            env_sort = _argsort_ids(env_id)
            env_id, hfenv_full = env_id[env_sort], hfenv_full[env_sort]
            hmatch = _searchsorted(env_id, hid)
            if not np.all(env_id[hmatch] == hid):
                raise RuntimeError('Failed to map global env sidecars onto staged halos by halo ID.')
            hfenv = hfenv_full[hmatch]
            if with_parts:
                if not np.all(hid[pinds] == phid):
                    raise RuntimeError('Particle-to-halo mapping pinds is inconsistent with phid.')
                pfenv = hfenv[pinds]

        halo_data = {'hpos': hpos, 'hvel': hvel, 'hmass': hmass, 'hid': hid, 'hmultis': hmultis,
                     'hrandoms': hrandoms, 'hveldev': hveldev, 'hsigma3d': hsigma3d, 'hc': hc, 'hrvir': hrvir}
        if with_parts:
            particle_data = {'ppos': ppos, 'pvel': pvel, 'phvel': phvel, 'phmass': phmass, 'phid': phid,
                             'pweights': pweights, 'prandoms': prandoms, 'pinds': pinds}
            npart = len(phmass)
            if self.want_ranks:
                particle_data.update(ranks)
            else:
                for k in ('pranks', 'pranksv', 'pranksp', 'pranksr', 'pranksc'):
                    particle_data[k] = np.ones(npart)
        if self.want_AB:
            halo_data['hdeltac'], halo_data['hfenv'] = hdeltac, hfenv
            if with_parts:
                particle_data['pdeltac'], particle_data['pfenv'] = pdeltac, pfenv
        if self.want_shear:
            halo_data['hshear'] = hshear
            if with_parts:
                particle_data['pshear'] = pshear
        return halo_data, particle_data

    # ------------------------------------------------------------------------------------------------------
    def restage(self):
        """Drop the device copy of the subsample (call after modifying halo_data / particle_data in place)."""
        if self._staged is not None:
            self._staged.free()
            self._staged = None

    def _device_catalog(self):
        if self._staged is None:
            self._staged = StagedCatalog(self.halo_data, self.particle_data)
        return self._staged

    def run_hod(self, tracers=None, want_rsd=True, want_nfw=False, NFW_draw=None, reseed=None, write_to_disk=False,
                Nthread=16, verbose=False, fn_ext=None):
        """Runs a custom HOD; returns `mock_dict` {tracer: {'x','y','z','vx','vy','vz','mass','id','Ncent'}}
        with centrals first (hod/abacus_hod.py:706-859)."""
        if tracers is None:
            tracers = self.tracers
        if self.z_type == 'secondary' and not want_nfw:
            raise RuntimeError('Secondary redshifts do not have particle pos/vel outputs and so only NFW profiles '
                               'are supported')
        if reseed:
            start = time.time()
            # The reference draws float32 streams from parallel_numpy_rng.MTGenerator(PCG64(reseed)) (:778-823), a
            # third-party generator that is not available here (stream parity unpinned; the reference only smoke-tests
            # this path).  Same distributions and dtypes from the device's counter-based Philox generator: the three
            # arrays are rewritten in HBM, then copied back so that `halo_data` / `particle_data` are mutated exactly
            # as the reference mutates them (:824-835).  `reseed_sync_host = False` skips the copy (MCMC loops).
            st = self._device_catalog()
            st.reseed(reseed, hsigma3d=self.halo_data['hsigma3d'], want_expvel=self.want_expvel)
            if getattr(self, 'reseed_sync_host', True):
                self.halo_data['hrandoms'] = st.fetch_field('hrandoms').astype(np.float32)    # float32 draws (:780)
                self.halo_data['hveldev'] = st.fetch_field('hveldev')                         # float32 * float64
                self.particle_data['prandoms'] = st.fetch_field('prandoms').astype(np.float32)
            self.logger.info(f'Randoms generated in elapsed time {time.time() - start:.2f} s.')

        start = time.time()
        mock_dict = gen_gal_cat(self.halo_data, self.particle_data, tracers, self.params, Nthread,
                                enable_ranks=self.want_ranks, rsd=want_rsd, nfw=want_nfw, NFW_draw=NFW_draw,
                                write_to_disk=write_to_disk, savedir=self.mock_dir, verbose=verbose, fn_ext=fn_ext,
                                staged=self._device_catalog(), lazy=getattr(self, 'lazy_columns', False))
        self.logger.info(f'HOD generated in elapsed time {time.time() - start:.2f} s.')
        return mock_dict

    # ------------------------------------------------------------------------------------------------------
    def _ngal_cells(self):
        """np.histogramdd's cell of every halo in the (logM, deltac, fenv, shear) histogram (:199-251): uint8 (N, 4),
        255 = outside the range (histogramdd drops those), plus the [4][100] table of cell centres"""
        hd = self.halo_data
        n = len(hd['hmass'])
        cols = (np.log10(hd['hmass']), hd.get('hdeltac', np.zeros(n)), hd.get('hfenv', np.zeros(n)),
                hd.get('hshear', np.zeros(n)))
        edges = (self.logMbins, self.deltacbins, self.fenvbins, self.shearbins)
        bins = np.empty((n, 4), dtype=np.uint8)
        for d, (x, e) in enumerate(zip(cols, edges)):
            idx = np.searchsorted(e, x, side='right') - 1
            idx[x == e[-1]] = len(e) - 2           # the last bin is closed on the right
            idx[(idx < 0) | (idx > len(e) - 2)] = 255
            bins[:, d] = idx
        centres = np.empty((4, len(self.logMbins) - 1))
        centres[0] = 10 ** (0.5 * (self.logMbins[1:] + self.logMbins[:-1]))   # Mh_temp = 10**logMs[i] (:1009)
        for d, e in enumerate(edges[1:], start=1):
            centres[d] = 0.5 * (e[1:] + e[:-1])
        return bins, centres

    def compute_ngal(self, tracers=None, Nthread=16):
        """Expected number of each tracer and its satellite fraction from the weighted halo histogram
        (hod/abacus_hod.py:861-1179), evaluated on the device as the identical sum over halos (abacus_hod_ngal)."""
        import ctypes as C

        from .. import _lib
        from .GRAND_HOD import TRACERS, marshal_params
        if tracers is None:
            tracers = self.tracers
        st = self._device_catalog()
        if not getattr(st, '_ngal_set', False):
            bins, centres = self._ngal_cells()
            _lib.check(_lib.lib().abacus_hod_set_ngal_bins(st._h, _lib.ptr(np.ascontiguousarray(bins)),
                                                           _lib.ptr(np.ascontiguousarray(centres)), centres.shape[1]))
            st._ngal_set = True
        known = {t: dict(tracers[t]) for t in tracers if t in TRACERS}
        for hod in known.values():               # keys gen_gals requires but compute_ngal never reads (:884-976)
            for k in ('alpha_c', 'alpha_s', 's', 's_v', 's_p', 's_r'):
                hod.setdefault(k, 0.0)
        if 'ELG' in known:
            # compute_ngal's own defaults (:925-948), which differ from gen_gals': `A_s` is optional here, and the
            # conformity parameters default to the RAW logM1 / alpha - the z-evolution (:1050-1051) never touches them
            hod = known['ELG']
            hod.setdefault('A_s', 1.0)
            for k, src in (('logM1_EE', 'logM1'), ('alpha_EE', 'alpha'), ('logM1_EL', 'logM1'), ('alpha_EL', 'alpha')):
                hod.setdefault(k, hod[src])
        p = marshal_params(known, dict(self.params, z=self.z_mock), False, True)
        out = (C.c_double * 6)()
        _lib.check(_lib.lib().abacus_hod_ngal(st._h, C.byref(p), out))
        ngal_dict, fsat_dict = {}, {}
        for etracer in known:
            t = TRACERS.index(etracer)
            ngal_cent, ngal_sat = out[t], out[3 + t]
            ngal_dict[etracer] = ngal_cent + ngal_sat
            fsat_dict[etracer] = ngal_sat / (ngal_cent + ngal_sat)
        return ngal_dict, fsat_dict

    # ------------------------------------------------------------------------------------------------------
    def compute_clustering(self, mock_dict, *args, **kwargs):
        """(:1181-1219)"""
        if self.clustering_type == 'xirppi':
            return self.compute_xirppi(mock_dict, *args, **kwargs)
        elif self.clustering_type == 'wp':
            return self.compute_wp(mock_dict, *args, **kwargs)
        elif self.clustering_type == 'multipole':
            return self.compute_multipole(mock_dict, *args, **kwargs)
        raise ValueError('clustering_type not implemented or not specified, use xirppi, wp, multipole')

    @staticmethod
    def _xyz(mock_dict, tracer):
        """the tracer's coordinate columns: still in HBM behind this object's staged catalogue when `mock_dict` is the
        untouched result of the latest run_hod (GRAND_HOD.MockDict.device_xyz), else the host arrays"""
        dev = mock_dict.device_xyz(tracer) if hasattr(mock_dict, 'device_xyz') else None
        if dev is not None:
            return dev
        return mock_dict[tracer]['x'], mock_dict[tracer]['y'], mock_dict[tracer]['z']

    def _pairs(self, mock_dict, fn, weights=None):
        """`fn` over every tracer pair.  weights: None (the reference: a 'w' column is ignored), or the name of a column of
        per-galaxy weights - tracers without it count with unit weights - handed to `fn` as w1= / w2=; the coordinates
        stay in HBM either way, only the weights are uploaded"""
        clustering = {}
        wcol = lambda tr: None if weights is None else mock_dict[tr].get(weights)   # noqa: E731
        wkw = lambda tr1, tr2: {} if weights is None else dict(w1=wcol(tr1), w2=None if tr2 is None else wcol(tr2))   # noqa: E731
        for i1, tr1 in enumerate(mock_dict.keys()):
            x1, y1, z1 = self._xyz(mock_dict, tr1)
            for i2, tr2 in enumerate(mock_dict.keys()):
                if i1 > i2:
                    continue  # cross-correlations are symmetric
                if i1 == i2:
                    clustering[tr1 + '_' + tr2] = fn(x1, y1, z1, None, None, None, **wkw(tr1, None))
                else:
                    x2, y2, z2 = self._xyz(mock_dict, tr2)
                    if isinstance(x1, np.ndarray) != isinstance(x2, np.ndarray):   # one side only in HBM: both from the host
                        x1, y1, z1 = (mock_dict[tr1][c] for c in 'xyz')
                        x2, y2, z2 = (mock_dict[tr2][c] for c in 'xyz')
                    clustering[tr1 + '_' + tr2] = fn(x1, y1, z1, x2, y2, z2, **wkw(tr1, tr2))
                    clustering[tr2 + '_' + tr1] = clustering[tr1 + '_' + tr2]
        return clustering

    def _lc_origin(self):
        """the observer of this object's light cone, for the randoms-based estimators"""
        origin = self.params.get('origin') if getattr(self, 'halo_lc', False) else None
        if origin is None:
            raise ValueError('randoms= needs a light-cone catalogue: this AbacusHOD carries no origin')
        return np.asarray(origin, dtype=np.float64).reshape(-1)[:3]

    def compute_xirppi(self, mock_dict, rpbins, pimax, pi_bin_size, Nthread=8, weights=None, randoms=None):
        """xi(rp, pi) for every tracer pair (:1221-1279); weights: see `_pairs`.  randoms: None (the periodic box), or an
        `LCRandoms` - the Landy-Szalay estimator with the pairwise line of sight seen from the light cone's origin"""
        if randoms is not None:
            origin = self._lc_origin()
            return self._pairs(mock_dict, lambda x1, y1, z1, x2, y2, z2, **w: calc_xirppi_lc(
                x1, y1, z1, rpbins, pimax, pi_bin_size, randoms, Nthread, x2=x2, y2=y2, z2=z2, origin=origin, **w), weights)
        return self._pairs(mock_dict, lambda x1, y1, z1, x2, y2, z2, **w: calc_xirppi_fast(
            x1, y1, z1, rpbins, pimax, pi_bin_size, self.lbox, Nthread, x2=x2, y2=y2, z2=z2, **w), weights)

    def compute_wp(self, mock_dict, rpbins, pimax, pi_bin_size, Nthread=8, weights=None, randoms=None):
        """wp(rp) for every tracer pair (:1826-1885); weights: see `_pairs`; randoms: see `compute_xirppi`"""
        if randoms is not None:
            origin = self._lc_origin()
            return self._pairs(mock_dict, lambda x1, y1, z1, x2, y2, z2, **w: calc_wp_lc(
                x1, y1, z1, rpbins, pimax, randoms, Nthread, x2=x2, y2=y2, z2=z2, origin=origin, **w), weights)
        return self._pairs(mock_dict, lambda x1, y1, z1, x2, y2, z2, **w: calc_wp_fast(
            x1, y1, z1, rpbins, pimax, self.lbox, Nthread, x2=x2, y2=y2, z2=z2, **w), weights)

    def compute_multipole(self, mock_dict, rpbins, pimax, sbins, nbins_mu, orders=[0, 2], Nthread=8, weights=None,
                          randoms=None):
        """wp concatenated with xi_l(s) (:1281-1336; like the reference, cross pairs use `rpbins` as s bins, :1313);
        weights: see `_pairs`; randoms: see `compute_xirppi`"""
        origin = None if randoms is None else self._lc_origin()

        def fn(x1, y1, z1, x2, y2, z2, **w):
            sb = sbins if x2 is None else rpbins
            if randoms is not None:
                new_multi = calc_multipole_lc(x1, y1, z1, sb, randoms, Nthread, nbins_mu=nbins_mu, orders=orders, x2=x2, y2=y2,
                                              z2=z2, origin=origin, **w)
                new_wp = calc_wp_lc(x1, y1, z1, rpbins, pimax, randoms, Nthread, x2=x2, y2=y2, z2=z2, origin=origin, **w)
                return np.concatenate((new_wp, new_multi))
            new_multi = calc_multipole_fast(x1, y1, z1, sb, self.lbox, Nthread, nbins_mu=nbins_mu, orders=orders,
                                            x2=x2, y2=y2, z2=z2, **w)
            new_wp = calc_wp_fast(x1, y1, z1, rpbins, pimax, self.lbox, Nthread, x2=x2, y2=y2, z2=z2, **w)
            return np.concatenate((new_wp, new_multi))
        return self._pairs(mock_dict, fn, weights)

    def compute_jackknife(self, mock_dict, statistic, nsplit, *args, weights=None):
        """(full, delete-one samples, jackknife covariance) of 'wp' | 'xirppi' | 'multipole' for every tracer pair on the
        periodic box, the regions an `nsplit` (an int or three) split of the box into sub-boxes (analysis/jackknife.py: one
        pair walk per count instead of one per region).  `*args` are those of the matching `compute_*`; weights: see `_pairs`.
        The labels are made in HBM when the catalogue is still resident there"""
        from ..analysis import jackknife as jk
        if statistic not in ('wp', 'xirppi', 'multipole'):
            raise ValueError("statistic must be one of 'wp', 'xirppi', 'multipole'")
        if statistic == 'multipole':
            rpbins, pimax, sbins, nbins_mu, *rest = args
            orders, Nthread = (rest + [[0, 2], 8][len(rest):])[:2]
        else:
            rpbins, pimax, pi_bin_size, *rest = args
            Nthread = rest[0] if rest else 8
        nreg = int(np.prod(jk._split(nsplit)))

        def fn(x1, y1, z1, x2, y2, z2, **w):
            r1 = jk.box_regions(x1, y1, z1, self.lbox, nsplit)
            r2 = None if x2 is None else jk.box_regions(x2, y2, z2, self.lbox, nsplit)
            kw = dict(x2=x2, y2=y2, z2=z2, regions2=r2, **w)
            if statistic == 'wp':
                return jk.calc_wp_jk(x1, y1, z1, rpbins, pimax, self.lbox, Nthread, r1, nreg, **kw)
            if statistic == 'xirppi':
                return jk.calc_xirppi_jk(x1, y1, z1, rpbins, pimax, pi_bin_size, self.lbox, Nthread, r1, nreg, **kw)
            sb = sbins if x2 is None else rpbins
            wp = jk.calc_wp_jk(x1, y1, z1, rpbins, pimax, self.lbox, Nthread, r1, nreg, **kw)
            multi = jk.calc_multipole_jk(x1, y1, z1, sb, self.lbox, Nthread, r1, nreg, nbins_mu=nbins_mu, orders=orders, **kw)
            samples = np.hstack((wp[1], multi[1]))
            return np.concatenate((wp[0], multi[0])), samples, jk.jackknife_covariance(samples)
        return self._pairs(mock_dict, fn, weights)

    def compute_vpf(self, mock_dict, rmax, nbins, nspheres, numpN=6, seed=42):
        """{tracer: the void probability function and count probabilities P_0 .. P_{numpN - 1}} of `nspheres` random spheres
        per tracer (analysis/spheres.py: `vpf`, Corrfunc.theory.vpf's result); the galaxies stay in HBM when `mock_dict` is the
        untouched result of the latest run_hod, only the centres are uploaded"""
        from ..analysis.spheres import vpf
        return {tr: vpf(rmax, nbins, nspheres, numpN, seed, *self._xyz(mock_dict, tr), periodic=True, boxsize=self.lbox)
                for tr in mock_dict.keys()}

    def compute_groups(self, mock_dict, b_perp, b_par=None, nmax=64, return_labels=False):
        """{tracer: the friends-of-friends groups of the tracer} (analysis/groups.py: `fof_groups` - 'labels', 'ngroups', 'mult',
        'n'); b_perp and b_par in box units (`groups.linking_lengths` turns fractions of the mean separation into them), b_par:
        cylinders along z.  The galaxies stay in HBM when `mock_dict` is the untouched result of the latest run_hod; one
        catalogue per call - no groups across tracers"""
        from ..analysis.groups import fof_groups
        return {tr: fof_groups(*self._xyz(mock_dict, tr), self.lbox, b_perp, b_par=b_par, nmax=nmax, return_labels=return_labels)
                for tr in mock_dict.keys()}

    def compute_mst(self, mock_dict, rmax, return_degree=True, return_labels=False):
        """{tracer: the minimum spanning forest of the tracer} (analysis/mst.py: `minimum_spanning_tree` - 'i', 'j', 'r2',
        'length', 'degree', 'labels', 'nedges', 'ncomp', 'n'); rmax in box units (`groups.linking_lengths` turns a fraction of the
        mean separation into them).  The galaxies stay in HBM when `mock_dict` is the untouched result of the latest run_hod; one
        catalogue per call - no tree across tracers; `mst.mst_branches` and `mst.mst_statistics` take it from there on the host"""
        from ..analysis.mst import minimum_spanning_tree
        return {tr: minimum_spanning_tree(*self._xyz(mock_dict, tr), self.lbox, rmax, return_degree=return_degree, return_labels=return_labels)
                for tr in mock_dict.keys()}

    def compute_knn(self, mock_dict, radii, ks, nquery, seed=42, pimax=None, data_queries=False):
        """{tracer: the kNN-CDFs (len(ks), len(radii)) of `nquery` random centres} (analysis/spheres.py: `knn_cdf`); pimax: the
        (rp, pi) form.  data_queries: also '{a}_{b}' for every ORDERED tracer pair - the galaxies of a as queries around the
        galaxies of b, a galaxy not counting itself when a is b"""
        from ..analysis.spheres import knn_cdf
        out = {tr: knn_cdf(*self._xyz(mock_dict, tr), self.lbox, radii, ks, nquery=nquery, seed=seed, pimax=pimax)
               for tr in mock_dict.keys()}
        if data_queries:
            for a in mock_dict.keys():
                for b in mock_dict.keys():
                    data = self._xyz(mock_dict, b)
                    if a == b:
                        out[a + '_' + b] = knn_cdf(*data, self.lbox, radii, ks, pimax=pimax)
                        continue
                    queries = self._xyz(mock_dict, a)
                    if isinstance(data[0], np.ndarray) != isinstance(queries[0], np.ndarray):   # one side only in HBM
                        data, queries = [mock_dict[b][c] for c in 'xyz'], [mock_dict[a][c] for c in 'xyz']
                    out[a + '_' + b] = knn_cdf(*data, self.lbox, radii, ks, *queries, pimax=pimax)
        return out

    def compute_power(self, mock_dict, nbins_k, nbins_mu, k_hMpc_max, logk, poles=[], paste='TSC', num_cells=550,
                      compensated=False, interlaced=False, randoms=None):
        r"""P(k, mu) and/or P_l(k) for every tracer pair (:1338-1472).  Returned keys: '{a}_{b}', '..._modes',
        '..._ell', '..._ell_modes', 'k_binc', 'mu_binc'.

        randoms: None (the periodic box, above), or an `LCRandoms` with `nbar=` on a light-cone object - the FKP / Yamamoto
        multipoles of `analysis.lc_power.calc_power_lc` seen from the light cone's origin, every tracer's F_0 and F_l built once
        from its columns in HBM.  Returned keys then: '{a}_{b}_ell' (len(poles), nbins_k), '{a}_{b}_ell_modes' and 'k_binc' only:
        there is no P(k, mu) with a line of sight that varies across the catalogue, `nbins_mu` is ignored, `interlaced` must be
        false, `poles` is a non-empty subset of (0, 2, 4) and `num_cells` even.  A 'w' column weights its tracer."""
        if randoms is not None:
            from ..analysis.lc_power import calc_power_lc_multi
            if interlaced:
                raise NotImplementedError('randoms=: the light-cone spectra are not interlaced')
            origin = self._lc_origin()
            samples = {tr: (*self._xyz(mock_dict, tr), mock_dict[tr].get('w', None)) for tr in mock_dict.keys()}
            tabs, k_mid = calc_power_lc_multi(samples, randoms, nbins_k, num_cells, poles, k_max=k_hMpc_max, logk=logk, paste=paste,
                                              compensated=compensated, origin=origin)
            clustering = {'k_binc': k_mid}
            for (tr1, tr2), power in tabs.items():
                for a, b in ((tr1, tr2), (tr2, tr1)):
                    clustering[f'{a}_{b}_ell'] = power['poles']
                    clustering[f'{a}_{b}_ell_modes'] = power['N_mode']
            return clustering
        Lbox = self.lbox
        clustering = {}
        # the untouched result of the latest run_hod, unweighted: every tracer's field from its columns in HBM, deposited
        # and transformed once, all pairs binned on the device (analysis.power_spectrum.calc_power_multi)
        dev = {tr: (mock_dict.device_xyz(tr) if hasattr(mock_dict, 'device_xyz') and 'w' not in mock_dict[tr] else None)
               for tr in mock_dict.keys()}
        if dev and all(v is not None for v in dev.values()) and len(dev) <= 8:
            from ..analysis.power_spectrum import calc_power_multi
            tabs = calc_power_multi(dev, Lbox, nbins_k, nbins_mu, k_hMpc_max, logk, paste, num_cells, compensated,
                                    interlaced, poles=poles)
            for (tr1, tr2), power in tabs.items():
                key = tr1 + '_' + tr2
                clustering[key] = power['power']
                clustering[key + '_modes'] = power['N_mode']
                clustering[key + '_ell'] = power['poles']
                clustering[key + '_ell_modes'] = power['N_mode_poles']
                if tr1 != tr2:
                    for suffix in ('', '_modes', '_ell', '_ell_modes'):
                        clustering[tr2 + '_' + tr1 + suffix] = clustering[key + suffix]
            clustering['k_binc'] = power['k_mid']
            clustering['mu_binc'] = power['mu_mid'][0]
            return clustering
        for i1, tr1 in enumerate(mock_dict.keys()):
            pos1 = np.stack((mock_dict[tr1]['x'], mock_dict[tr1]['y'], mock_dict[tr1]['z']), axis=1)
            w1 = mock_dict[tr1].get('w', None)
            for i2, tr2 in enumerate(mock_dict.keys()):
                if i1 > i2:
                    continue
                if i1 == i2:
                    power = calc_power(pos1, Lbox, nbins_k, nbins_mu, k_hMpc_max, logk, paste, num_cells, compensated,
                                       interlaced, w=w1, poles=poles)
                else:
                    pos2 = np.stack((mock_dict[tr2]['x'], mock_dict[tr2]['y'], mock_dict[tr2]['z']), axis=1)
                    w2 = mock_dict[tr2].get('w', None)
                    power = calc_power(pos1, Lbox, nbins_k, nbins_mu, k_hMpc_max, logk, paste, num_cells, compensated,
                                       interlaced, w=w1, pos2=pos2, w2=w2, poles=poles)
                key = tr1 + '_' + tr2
                clustering[key] = power['power']
                clustering[key + '_modes'] = power['N_mode']
                clustering[key + '_ell'] = power['poles']  # KeyError with poles=[] exactly like the reference (:1431)
                clustering[key + '_ell_modes'] = power['N_mode_poles']
                if i1 != i2:
                    rkey = tr2 + '_' + tr1
                    for suffix in ('', '_modes', '_ell', '_ell_modes'):
                        clustering[rkey + suffix] = clustering[key + suffix]
        clustering['k_binc'] = power['k_mid']
        clustering['mu_binc'] = power['mu_mid'][0]
        return clustering

    def compute_bispectrum(self, mock_dict, kedges, num_cells=256, paste='TSC', compensated=True, interlaced=True):
        """The auto bispectrum B(k1, k2, k3) of every tracer in the periodic box (no reference counterpart;
        `analysis.bispectrum.calc_bispectrum`): {tracer: its result dict}.  `kedges`: the edges of at most 32 k-shells, the top one at
        most 2 pi / Lbox * num_cells / 3.  The columns are taken from HBM when `mock_dict` is the untouched result of the latest
        run_hod; a 'w' column weights its tracer (B and P are then raw, `Q` and `B_shot` None).  No cross bispectra."""
        from ..analysis.bispectrum import _check_args, calc_bispectrum
        _check_args(num_cells, self.lbox, kedges)
        out = {}
        for tr in mock_dict.keys():
            cols = self._xyz(mock_dict, tr)
            pos = list(cols) if not isinstance(cols[0], np.ndarray) else np.stack([np.asarray(c) for c in cols], axis=1)
            out[tr] = calc_bispectrum(pos, self.lbox, kedges, nmesh=num_cells, w=mock_dict[tr].get('w', None), paste=paste,
                                      compensated=compensated, interlaced=interlaced)
        return out

    def compute_minkowski(self, mock_dict, thresholds, R, num_cells=256, paste='TSC', compensated=True, interlaced=True, sigma_units=True):
        """The four Minkowski functionals V0 .. V3 of every tracer's density contrast in the periodic box, smoothed with a Gaussian of
        radius `R` (no reference counterpart; `analysis.minkowski.calc_minkowski`): {tracer: its result dict}.  `thresholds`: at
        most 64 increasing values, nu in units of sigma around the mean with `sigma_units`, else values of the smoothed contrast.  The
        columns are taken from HBM when `mock_dict` is the untouched result of the latest run_hod; a 'w' column weights its tracer.
        No cross-field morphology."""
        from ..analysis.minkowski import calc_minkowski
        out = {}
        for tr in mock_dict.keys():
            cols = self._xyz(mock_dict, tr)
            pos = list(cols) if not isinstance(cols[0], np.ndarray) else np.stack([np.asarray(c) for c in cols], axis=1)
            out[tr] = calc_minkowski(pos, self.lbox, thresholds, R, nmesh=num_cells, w=mock_dict[tr].get('w', None), paste=paste,
                                     compensated=compensated, interlaced=interlaced, sigma_units=sigma_units)
        return out

    def compute_wst(self, mock_dict, J=4, L=4, q=(0.8,), num_cells=256, sigma0=0.8, paste='TSC', compensated=True, interlaced=True,
                    contrast=False, second_order=True):
        """The solid-harmonic wavelet scattering coefficients S0, S1, S2 of every tracer's density field in the periodic box (no
        reference counterpart; `analysis.wst.calc_wst`): {tracer: its result dict}.  `J` scales sigma0 2^j cells, angular orders
        0 .. `L` <= 4, at most 8 exponents `q`.  The columns are taken from HBM when `mock_dict` is the untouched result of the latest
        run_hod; a 'w' column weights its tracer.  No cross-tracer coefficients."""
        from ..analysis.wst import calc_wst
        out = {}
        for tr in mock_dict.keys():
            cols = self._xyz(mock_dict, tr)
            pos = list(cols) if not isinstance(cols[0], np.ndarray) else np.stack([np.asarray(c) for c in cols], axis=1)
            out[tr] = calc_wst(pos, self.lbox, J=J, L=L, q=q, sigma0=sigma0, nmesh=num_cells, w=mock_dict[tr].get('w', None), paste=paste,
                               compensated=compensated, interlaced=interlaced, contrast=contrast, second_order=second_order)
        return out

    def compute_voids(self, mock_dict, radii, threshold=-0.7, num_cells=256, paste='TSC', compensated=True, interlaced=True,
                      return_fields=False):
        """The spherical voids of every tracer's density contrast in the periodic box (no reference counterpart;
        `analysis.voids.find_voids`): {tracer: its result dict}.  `radii`: at most 32 strictly decreasing radii, the largest at most
        Lbox / 4; a cell is a candidate of a radius where the contrast smoothed with that top hat is below `threshold`.  The columns
        are taken from HBM when `mock_dict` is the untouched result of the latest run_hod; a 'w' column weights its tracer.  No
        voids across tracers."""
        from ..analysis.voids import find_voids
        out = {}
        for tr in mock_dict.keys():
            cols = self._xyz(mock_dict, tr)
            pos = list(cols) if not isinstance(cols[0], np.ndarray) else np.stack([np.asarray(c) for c in cols], axis=1)
            out[tr] = find_voids(pos, self.lbox, radii, threshold=threshold, nmesh=num_cells, w=mock_dict[tr].get('w', None), paste=paste,
                                 compensated=compensated, interlaced=interlaced, return_fields=return_fields)
        return out

    def compute_watershed_voids(self, mock_dict, R, num_cells=256, paste='TSC', compensated=True, interlaced=True, connectivity=26,
                                min_radius=0.0, saddle_max=None, return_field=False, return_labels=False):
        """The watershed voids of every tracer's density contrast in the periodic box, smoothed with a Gaussian of radius `R` (no
        reference counterpart; `analysis.watershed.find_watershed_voids`): {tracer: its result dict} - the zones, their saddle
        tree and the ZOBOV hierarchy; with `saddle_max` the zones merged below that saddle.  The columns are taken from HBM when
        `mock_dict` is the untouched result of the latest run_hod; a 'w' column weights its tracer.  No zones across tracers."""
        from ..analysis.watershed import find_watershed_voids
        out = {}
        for tr in mock_dict.keys():
            cols = self._xyz(mock_dict, tr)
            pos = list(cols) if not isinstance(cols[0], np.ndarray) else np.stack([np.asarray(c) for c in cols], axis=1)
            out[tr] = find_watershed_voids(pos, self.lbox, R, nmesh=num_cells, w=mock_dict[tr].get('w', None), paste=paste,
                                           compensated=compensated, interlaced=interlaced, connectivity=connectivity, min_radius=min_radius,
                                           saddle_max=saddle_max, return_field=return_field, return_labels=return_labels)
        return out

    def compute_3pcf(self, mock_dict, rbins, lmax, randoms=None, seed=42):
        """The three-point correlation function multipoles zeta_l(r1, r2) of every tracer in the periodic box (no reference
        counterpart; `analysis.threepcf.calc_3pcf`): {tracer: its result dict}.  `rbins`: the edges of at most 32 radial bins, the
        last at most Lbox / 2; lmax <= 10.  randoms: None - the natural multipoles of the data alone, which contain the 1 + xi
        terms - or an int (that many random centres of `seed`) or three columns: the connected zeta from D - R.  The columns are
        taken from HBM when `mock_dict` is the untouched result of the latest run_hod; a 'w' column weights its tracer.  Auto
        only: no cross three-point functions between tracers."""
        from ..analysis.threepcf import calc_3pcf
        return {tr: calc_3pcf(*self._xyz(mock_dict, tr), self.lbox, rbins, lmax, w=mock_dict[tr].get('w', None), randoms=randoms,
                              seed=seed) for tr in mock_dict.keys()}

    def compute_delta_sigma(self, mock_dict, parts, rp_bins, tracers=None, particle_mass=1.0):
        """The excess surface density Delta Sigma(R) of the matter around every tracer (no reference counterpart;
        `analysis.lensing.delta_sigma`): {tracer: its result dict}.  `parts`: the `analysis.lensing.ProjectedParticles` of the
        matter particles' x and y columns, built once for the fit; `rp_bins`: at most 32 bins whose last edge is at most its
        rmax.  tracers: None (all) or the names to compute.  The galaxies' x and y are taken from HBM when `mock_dict` is the
        untouched result of the latest run_hod; a 'w' column weights its tracer.  The line of sight is z: redshift-space
        distortions move galaxies along z only, which a projection over the whole box does not see.  For another axis pass
        real-space columns to `analysis.lensing.delta_sigma` yourself - the x or y of a mock with RSD along z are real-space
        columns, its z is not."""
        from ..analysis.lensing import delta_sigma
        out = {}
        for tr in (mock_dict.keys() if tracers is None else tracers):
            x, y, _ = self._xyz(mock_dict, tr)
            out[tr] = delta_sigma(parts, x, y, rp_bins, weights=mock_dict[tr].get('w', None), particle_mass=particle_mass)
        return out

    def compute_pairwise_velocity(self, mock_dict, rbins, mode='r', pimax=None, npibins=1, nmubins=1, weights=None):
        """The pairwise velocity sums and moments of every tracer pair in the periodic box (no reference counterpart;
        `analysis.pairwise_velocity`): {'{a}_{b}': the seven sums of `pairwise_velocity_sums` and the moments of `moments_from_sums`
        (v12, sigma_r, sigma_t, vlos, sigma_los)}, the symmetric key filled like the pair counts'.  mode 'r': bins of r; 'rppi':
        bins of rp and `npibins` bins of |pi| < pimax; 'smu': bins of s and `nmubins` bins of mu in [0, 1).  weights: see `_pairs`.
        The six columns of a tracer are taken from HBM when `mock_dict` is the untouched result of the latest run_hod, else from
        the host columns.  The line of sight is z, and with want_rsd the z column is the REDSHIFT-SPACE one: separations,
        the radial direction and sign(dz) are then those of redshift space, while the velocities are the galaxies' own."""
        from ..analysis.pairwise_velocity import moments_from_sums, pairwise_velocity_sums
        if mode == 'rppi' and pimax is None:
            raise ValueError("mode 'rppi' needs pimax")
        kw = dict(pimax=0.0 if pimax is None else float(pimax), npibins=int(npibins), mu_max=1.0, nmubins=int(nmubins))

        def six(tr, host=False):
            xyz = None if host or not hasattr(mock_dict, 'device_vel') else mock_dict.device_xyz(tr)
            vel = None if xyz is None else mock_dict.device_vel(tr)
            if vel is not None:
                return list(xyz) + list(vel)
            return [mock_dict[tr][c] for c in ('x', 'y', 'z', 'vx', 'vy', 'vz')]
        wcol = lambda tr: None if weights is None else mock_dict[tr].get(weights)   # noqa: E731
        out = {}
        tracers = list(mock_dict.keys())
        for i1, tr1 in enumerate(tracers):
            for tr2 in tracers[i1:]:
                c1, c2 = six(tr1), (None,) * 6 if tr2 == tr1 else six(tr2)
                if tr2 != tr1 and isinstance(c1[0], np.ndarray) != isinstance(c2[0], np.ndarray):   # one side only in HBM: both from the host
                    c1, c2 = six(tr1, host=True), six(tr2, host=True)
                sums = pairwise_velocity_sums(mode, *c1, self.lbox, rbins, *c2, W1=wcol(tr1), W2=None if tr2 == tr1 else wcol(tr2), **kw)
                out[tr1 + '_' + tr2] = out[tr2 + '_' + tr1] = {**sums, **moments_from_sums(sums)}
        return out

    def apply_zcv(self, mock_dict, config, load_presaved=False):
        """signature of hod/abacus_hod.py:1474; not built (needs ZeNBu and classy).  `abacusutils_amd.hod.zcv` produces the spectra that
        the reference's `tools_cv.run_zcv` combines"""
        raise NotImplementedError('tools_cv.run_zcv needs ZeNBu and classy and is not built; the device half of ZCV (fields, advection, spectra) is abacusutils_amd.hod.zcv')

    def apply_zcv_xi(self, mock_dict, config, load_presaved=False):
        """signature of hod/abacus_hod.py:1663; see apply_zcv"""
        raise NotImplementedError('tools_cv.run_zcv needs ZeNBu and classy and is not built; the device half of ZCV (fields, advection, spectra) is abacusutils_amd.hod.zcv')

    def gal_reader(self, output_dir=None, simname=None, sim_dir=None, z_mock=None, want_rsd=None, tracers=None):
        """Load `{tracer}s.dat` ECSV catalogs written by run_hod(write_to_disk=True) (:1887-1950)."""
        if want_rsd is None:
            want_rsd = self.want_rsd
        if tracers is None:
            tracers = self.tracers.keys()
        outdir = Path(self.mock_dir) / ('galaxies' + ('_rsd' if want_rsd else ''))
        mockdict = {}
        for tracer in tracers:
            header, rows, meta = None, [], {}
            for line in open(outdir / (tracer + 's.dat')):
                if line.startswith('#'):
                    if 'Ncent:' in line:
                        meta['Ncent'] = int(line.split('Ncent:')[1].strip(' }\n'))
                    continue
                if header is None:
                    header = line.split()
                    continue
                rows.append(line.split())
            cols = {}
            for j, name in enumerate(header):
                conv = int if name == 'id' else float
                cols[name] = np.array([conv(r[j]) for r in rows], dtype=np.int64 if name == 'id' else np.float64)
            cols.update(meta)
            mockdict[tracer] = cols
        return mockdict
