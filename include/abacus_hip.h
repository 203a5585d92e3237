/*
 * abacus_hip.h - C ABI of libabacus_hip.so (MI355X / gfx950).
 *
 * The reference (abacusorg/abacusutils) has no FFI seam: its hot path is Python + Numba and the drop-in
 * boundary is the Python call signature.  This header is the C boundary underneath our
 * Python mirror of those signatures; each entry point names the reference function(s) it replaces
 * (paths relative to abacusnbody/).  INTEGRATION.md shows the ctypes binding a maintainer of the reference
 * would add.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; abacus_last_error() returns a thread-local message;
 *   - the caller owns all host buffers; the library reads/writes them only during the call;
 *   - device state lives behind explicit handles (`*_stage` / `*_free`), mirroring the residency of
 *     AbacusHOD.staging() (hod/abacus_hod.py:193-197): stage once, populate many times;
 *   - `*_dev` variants take DEVICE pointers and never synchronise with the host: they enqueue on the library
 *     stream (abacus_get_stream), for callers that keep data in HBM (bench, multi-GPU slab path);
 *   - calls are blocking unless stated; re-entrant per handle; HIP is initialised lazily on first use
 *     (fork-safe in the sense of NUMBA_THREADING_LAYER=forksafe, docs/hod.rst:226-240);
 *   - thread counts of the reference API (`Nthread`, `nthread`) have no meaning here and are not part of the ABI.
 */
#ifndef ABACUS_HIP_H
#define ABACUS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- runtime ------------------------------ */
const char *abacus_last_error(void);
int abacus_device_count(int *n);
int abacus_set_device(int device);          /* before any other call; default device 0 */
int abacus_device_name(char *buf, int len);
int abacus_device_sync(void);               /* wait for the library stream */
void *abacus_get_stream(void);              /* hipStream_t the library launches on */
int abacus_set_stream(void *hip_stream);    /* adopt a caller stream (e.g. torch's current stream) */

/* raw device memory for callers that keep inputs resident (bench.py, slab-parallel path) */
int abacus_malloc(void **dptr, uint64_t nbytes);
int abacus_free(void *dptr);
int abacus_memcpy_h2d(void *dst, const void *src, uint64_t nbytes);
int abacus_memcpy_d2h(void *dst, const void *src, uint64_t nbytes);
int abacus_memcpy_d2d(void *dst, const void *src, uint64_t nbytes);   /* enqueued on the library stream */
int abacus_memset(void *dptr, int value, uint64_t nbytes);
/* page-locked host memory (hipHostMalloc): device-to-host copies into it are single DMAs at link speed.  The Python side
 * hands catalogue columns out as NumPy views of such blocks and recycles them (abacusutils_amd/_lib.py pinned_empty) */
int abacus_host_alloc(void **hptr, uint64_t nbytes);
int abacus_host_free(void *hptr);
/* sum_i word[i] * (2 i + 1) mod 2^64 over n 8-byte words in HBM: position-dependent checksum of a device column (is a host
 * copy of the column still what the device holds?) */
int abacus_poshash_u64(const void *dptr, int64_t n, uint64_t *out);

/* HIP-event timers on the library stream (bench.py: roofline.achieved) */
int abacus_event_create(void **ev);
int abacus_event_record(void *ev);
int abacus_event_elapsed_ms(void *start, void *stop, float *ms); /* synchronises on `stop` */
int abacus_event_destroy(void *ev);
/* per-kernel timing: when enabled every kernel launch is bracketed by events on the library stream */
int abacus_profile_enable(int on);
int abacus_profile_reset(void);
/* bracket only the kernel called `name` (NULL or "": all kernels) - keeps the event overhead out of short steps */
int abacus_profile_select(const char *name);
/* writes up to `cap` entries; returns the number of distinct kernels (names are static strings) */
int abacus_profile_get(const char **names, double *total_ms, int64_t *launches, int cap);

/* Diagnostic options: comparator code paths that the parity tests and the A/B scripts switch on (the library reads no
 * environment variables).  Names: fft_nofuse (plain three-pass FFT), fft_hipfft, fft_fuse_small, pk_noxbin (separate last
 * pass + spectrum_bin), tsc_atomic, tsc_noshare, pairs_gen (1 / 2: older pair kernels), hod_nocls, hod_one_stage,
 * hod_f64filter, hod_norec, hod_nokeys, hod_pipe (1 / 2: pipelined hod_exact off / on), hod_eblock (256 / 512 threads per
 * hod_emit workgroup), hod_sbtiles (8 / 16 tiles per superblock), hod_nolazy / hod_noindex (no lazy
 * keep masks / no mass-sorted key index), hod_deal (the index path through hod_deal and the tile queues),
 * hod_sbindex (1: the index path through the global index, hod_exact_index and hod_emit_bm, instead of the per-superblock index),
 * hod_keepmasks (1: the per-superblock index path keeps the keep masks exact populate by populate instead of writing them on
 * demand), pairs_jk_grid (at most that many workgroups for the jackknife pair kernels: a small catalogue then walks many cells
 * per workgroup, as a large one does), lens_shared_rows (lens_walk adds into one set of LDS rows per workgroup instead of a
 * column per lane), dbg / dbg_fft / dbg_tsc (ablation bit masks).  Default 0 = the production path. */
int abacus_set_option(const char *name, int value);
int abacus_get_option(const char *name);

/* ---------------------------------------------------------------- HOD ---------------------------------- */
/*
 * Flat form of the three numba typed dicts gen_gals builds (hod/GRAND_HOD.py:1342-1468) plus the scalars it
 * passes to gen_cent / gen_sats (:1472-1475).  z-evolution and defaults are applied by the caller (Python
 * mirror of gen_gals) before filling this struct.
 */
typedef struct abacus_hod_params {
    int32_t want_LRG, want_ELG, want_QSO;
    int32_t rsd, has_origin, enable_ranks;
    int32_t pad0, pad1;
    double inv_velz2kms, lbox, origin[3];
    /* LRG_hod_dict */
    double L_logM_cut, L_logM1, L_sigma, L_alpha, L_kappa, L_alpha_c, L_alpha_s;
    double L_s, L_s_v, L_s_p, L_s_r, L_Acent, L_Asat, L_Bcent, L_Bsat, L_ic;
    /* ELG_hod_dict */
    double E_p_max, E_Q, E_logM_cut, E_kappa, E_sigma, E_logM1, E_alpha, E_gamma, E_A_s;
    double E_alpha_c, E_alpha_s, E_s, E_s_v, E_s_p, E_s_r;
    double E_Acent, E_Asat, E_Bcent, E_Bsat, E_Ccent, E_Csat, E_ic;
    double E_logM1_EE, E_alpha_EE, E_logM1_EL, E_alpha_EL;
    /* QSO_hod_dict */
    double Q_logM_cut, Q_kappa, Q_sigma, Q_logM1, Q_alpha, Q_alpha_c, Q_alpha_s;
    double Q_s, Q_s_v, Q_s_p, Q_s_r, Q_Acent, Q_Asat, Q_Bcent, Q_Bsat, Q_ic;
} abacus_hod_params;

/*
 * The staged halo / particle subsample: the arrays of AbacusHOD.halo_data / particle_data
 * (hod/abacus_hod.py:659-702) in their reference layout - float64, (N,3) C-order, int64 ids.
 * Optional arrays (NULL = absent, treated as zeros like gen_gals does, hod/GRAND_HOD.py:1485-1487,1541-1543):
 * hdeltac, hfenv, hshear, pdeltac, pfenv, pshear.  pranks* may be NULL when ranks are never enabled.
 * pinds[i] = index of particle i's host halo (hod/abacus_hod.py:588); the keep_cent[pinds] gather the
 * reference does on the host (hod/GRAND_HOD.py:1562) happens on the device.
 */
typedef struct abacus_hod_arrays {
    int64_t n_halo;
    const double *hpos, *hvel, *hmass;
    const int64_t *hid;
    const double *hmultis, *hrandoms, *hveldev, *hdeltac, *hfenv, *hshear;
    int64_t n_part;
    const double *ppos, *pvel, *phvel, *phmass;
    const int64_t *phid;
    const double *pweights, *prandoms, *pdeltac, *pfenv, *pshear;
    const double *pranks, *pranksv, *pranksp, *pranksr;
    const int64_t *pinds;
} abacus_hod_arrays;

typedef struct abacus_hod_state abacus_hod_state;

/* replaces: the host residency set up by AbacusHOD.staging() (hod/abacus_hod.py:253-704); uploads once.
 * `arrays_on_device` != 0: the pointers are device pointers that the handle adopts WITHOUT copying (the caller
 * keeps them alive until abacus_hod_free). */
int abacus_hod_stage(const abacus_hod_arrays *arrays, int arrays_on_device, abacus_hod_state **out);
/* re-upload one staged array after `reseed` rewrote it (hod/abacus_hod.py:824-835).
 * field: "hrandoms" | "hveldev" | "prandoms" (float64 host data, staged length) */
int abacus_hod_update(abacus_hod_state *st, const char *field, const double *host);
/* Device-side `reseed` (hod/abacus_hod.py:775-839): rewrites hrandoms, hveldev and prandoms in HBM from a counter-based
 * Philox4x32-10 generator keyed by `seed` - float32 U[0,1) uniforms, float32 N(0,1) (want_expvel: the two-sided
 * exponential of :799-801) times hsigma3d / sqrt(3) - with no host traffic.  A value depends only on (seed, global
 * object index): `halo_index0` / `part_index0` are the global indices of this catalogue's first halo / particle, so
 * the shards of a multi-GPU run draw what the unsharded catalogue would.  The reference's own stream comes from the
 * third-party parallel_numpy_rng (not in its tree): stream parity is unpinned, distributions and dtypes are the same.
 * abacus_hod_set_sigma3d stages the per-halo hsigma3d once; abacus_hod_fetch_field copies a rewritten array back
 * ("hrandoms" | "hveldev" | "prandoms") for callers that need the reference's host-side mutation (:824-835). */
int abacus_hod_set_sigma3d(abacus_hod_state *st, const double *hsigma3d, int on_device);
int abacus_hod_reseed(abacus_hod_state *st, uint64_t seed, int want_expvel, int64_t halo_index0, int64_t part_index0);
int abacus_hod_fetch_field(abacus_hod_state *st, const char *field, double *host);

/* `AbacusHOD.compute_ngal` (hod/abacus_hod.py:861-1179): expected numbers of centrals and satellites per tracer from the
 * weighted halo histogram.  The reference's sum over the 100^3 / 100^4 histogram cells is evaluated as the identical
 * sum over halos, sum_i multis[i] * n(centre of the cell of halo i).  bins4[i] = {logM, deltac, fenv, shear} cell of
 * halo i under np.histogramdd's edge rule (255 = outside: dropped, as histogramdd drops it); centres = [4][nbin]:
 * 10**logM centres, then the deltac, fenv and shear centres.  out = Ncent[3], Nsat[3] (LRG, ELG, QSO); `p` is the
 * marshalled parameter struct (z-evolution applied). */
int abacus_hod_set_ngal_bins(abacus_hod_state *st, const uint8_t *bins4, const double *centres, int nbin);
int abacus_hod_ngal(abacus_hod_state *st, const abacus_hod_params *p, double out[6]);

/* NFW satellites: `gen_gal_cat(..., nfw=True, NFW_draw=...)` (gen_sats_nfw, compute_fast_NFW, getPointsOnSphere,
 * hod/GRAND_HOD.py:417-822).  Centrals are decided exactly as on the particle path; satellites are Poisson(n_sat(M) ic)
 * per halo and tracer, placed isotropically at r = NFW_draw[k] / c * Rvir (k random with NFW_draw[k] <= c) around
 * their halo with N(v_halo, (0.577 f_sigv vrms)^2) velocities; box RSD only.  The reference draws from NumPy's
 * unseeded per-thread generators (never reproducible): parity is statistical; here the draws are
 * Philox streams of (seed, global halo index, tracer, satellite rank).  Needs abacus_hod_set_sigma3d (vrms) and
 * abacus_hod_set_profile (hc = r98/r25 concentration, hrvir) once per staged catalogue. */
typedef struct abacus_nfw_params {
    uint64_t seed;
    double f_sigv[3];                         /* LRG, ELG, QSO (:566,605,623) */
    double exp_frac, exp_scale, nfw_rescale;  /* ELG_hod_dict values, applied to every tracer as the reference does (:606-608) */
    int64_t halo_index0;                      /* global index of this catalogue's first halo (sharding) */
} abacus_nfw_params;
int abacus_hod_set_profile(abacus_hod_state *st, const double *hc, const double *hrvir);
int abacus_hod_populate_nfw(abacus_hod_state *st, const abacus_hod_params *p, const abacus_nfw_params *nfw,
                            const double *NFW_draw, int64_t n_draw, int64_t counts[6]);
/*
 * replaces: gen_cent + gen_sats + fast_concatenate (hod/GRAND_HOD.py:139-414, 825-1262, 1265-1299) as called from
 * gen_gals (:1477-1589).  Decides and emits on the device; galaxies of tracer t are left in device buffers in the
 * reference's order: centrals (halo order) then satellites (particle order).
 * counts[0..2] = Ncent (LRG, ELG, QSO), counts[3..5] = Nsat.
 */
int abacus_hod_populate(abacus_hod_state *st, const abacus_hod_params *p, int64_t counts[6]);
/* as above but enqueue only (no host sync, counts stay on the device until abacus_hod_counts) */
int abacus_hod_populate_async(abacus_hod_state *st, const abacus_hod_params *p);
int abacus_hod_counts(abacus_hod_state *st, int64_t counts[6]); /* syncs; re-runs emission if buffers grew */
/* diagnostic: how many halos (out[0]) and particles (out[1]) the last populate's filter passed on to the exact
 * float64 decision (no reference counterpart: the reference evaluates every object, hod/GRAND_HOD.py:210,954) */
int abacus_hod_candidates(abacus_hod_state *st, int64_t out[2]);
/* copy tracer t's catalog (x,y,z,vx,vy,vz,mass: float64; id: int64), each of length Ncent+Nsat, to the host */
int abacus_hod_fetch(abacus_hod_state *st, int tracer, double *x, double *y, double *z, double *vx, double *vy,
                     double *vz, double *mass, int64_t *id);
/* the same catalogue as ONE device-to-host transfer: out8 = [8][n] (x, y, z, vx, vy, vz, mass as float64, id as int64),
 * n = Ncent + Nsat of the tracer (checked against n_expected) */
int abacus_hod_fetch_block(abacus_hod_state *st, int tracer, void *out8, int64_t n_expected);
/* device pointers of tracer t's catalog columns (7 float64 + 1 int64), valid until the next populate */
int abacus_hod_device_columns(abacus_hod_state *st, int tracer, void *cols[8]);
/* the int8 masks gen_cent / gen_sats compute (hod/GRAND_HOD.py:210,954); either pointer may be NULL */
int abacus_hod_fetch_keep(abacus_hod_state *st, int8_t *keep_cent, int8_t *keep_sat);
int abacus_hod_free(abacus_hod_state *st);

/* ---------------------------------------------------------------- TSC / CIC ---------------------------- */
/* dtype codes */
#define ABACUS_F32 0
#define ABACUS_F64 1

/*
 * replaces: tsc_parallel = _wrap_inplace + partition_parallel + _tsc_parallel/_tsc_scatter
 * (analysis/tsc.py:10-206, 219-226, 259-384, 229-256, 394-507).
 * pos: (n,3) host array of `pos_dtype`; weights: (n,) same dtype or NULL; grid: (gx,gy,gz) host array of
 * `grid_dtype`, ACCUMULATED into (not zeroed), as the reference does (tsc.py:45-50).
 * wrap != 0: positions are wrapped to [0,box) and the wrapped values are written back to `pos` (the reference
 * mutates the caller's array, tsc.py:171-173).
 */
int abacus_tsc_deposit(void *pos, int64_t n, const void *weights, int pos_dtype, void *grid, int gx, int gy,
                       int gz, int grid_dtype, double box, double offset, int wrap);
/* device-resident variant: pos/weights/grid are device pointers; float32 positions and grid only.
 * zero_grid != 0 overwrites the grid instead of accumulating (saves the separate zeroing pass of get_field,
 * analysis/power_spectrum.py:842).  Enqueues on the library stream. */
int abacus_tsc_deposit_dev(float *pos, int64_t n, const float *weights, float *grid, int gx, int gy, int gz,
                           double box, double offset, int wrap, int zero_grid, int cic);
/* diagnostic (option tsc_lines_clk = 1): shader-clock ticks per phase of the list build's split rounds, summed over workgroups since
 * the last call; out32[0..9] coarse pass (count, barrier, owner, barrier, owner + carries, barrier, place, barrier, write-out,
 * geometry + loads), out32[16..24] fine pass.  Reads and clears. */
int abacus_tsc_lines_clocks(unsigned long long *out32);
/* replaces: cic_serial (analysis/cic.py:13-125): float64 math, float32 grid, no wrap */
int abacus_cic_deposit(const void *pos, int64_t n, const void *weights, int pos_dtype, float *grid, int gx, int gy,
                       int gz, double box);
/* replaces: partition_parallel (analysis/tsc.py:259-384), sort=False: stable counting sort into `npartition`
 * stripes along `coord`.  psort (n,3), starts (npartition+1) int64, wsort (n,) or NULL. */
int abacus_partition(const void *pos, int64_t n, const void *weights, int dtype, int npartition, double box,
                     int coord, void *psort, int64_t *starts, void *wsort);

/* ---------------------------------------------------------------- power spectrum ----------------------- */
/*
 * replaces: get_field_fft (analysis/power_spectrum.py:1001-1070) = get_field (:808-857: zero mesh, deposit,
 * normalize_field :860-901) + scipy.fft.rfftn (:980,986,1059) + _normalize (:1073-1078) or the interlacing
 * combine shift_field_fft (:904-948) + compensation divide (:1063-1069).
 * pos (n,3) float32 host; w (n,) float32 or NULL; W (nmesh,) float32 window or NULL (= not compensated);
 * out: (nmesh, nmesh, nmesh/2+1) complex64 host.  paste: 0 TSC, 1 CIC.
 */
/* get_field (analysis/power_spectrum.py:808-857): overdensity mesh delta = rho * f32(M / len(pos)) - 1 of the particles,
 * deposit and normalisation fused on the device; field: (nmesh, nmesh, nmesh) float32 host array.  TSC wraps pos in place. */
int abacus_field(float *pos, int64_t n, const float *w, double Lbox, int nmesh, int paste, double offset, float *field);
int abacus_field_fft(float *pos, int64_t n, const float *w, double Lbox, int nmesh, int paste, const float *W,
                     int interlaced, void *out_c64);
/*
 * float64 MESHES: get_field / get_field_fft / calc_power with dtype=np.float64 (analysis/power_spectrum.py:808-857, 1001-1070,
 * 1131-1319), non-interlaced (the reference's interlaced branch ignores dtype, :1048-1052).  pos_f64: the positions (and weights)
 * are float64 - the cloud weights are evaluated in the dtype of the positions (analysis/tsc.py:400).  The mesh is deposited,
 * normalised and transformed in float64 (csrc/gfft.hip: even sizes up to 2560 with factors 2, 3, 5, 7, 11, 13 - what fits the 160-KiB LDS tile in double; hipFFT's D2Z otherwise); field:
 * (nmesh,)*3 float64, out_c128: (nmesh, nmesh, nmesh/2+1) complex128; abacus_power_f64 returns what bin_kmu returns, times L^3.
 * abacus_power_f64 takes pos_f64 as a mask, one bit per particle set (bit 0: pos and w, bit 1: pos2 and w2): each set is
 * deposited in its own dtype, like the reference's two get_field_fft calls.
 */
int abacus_field_f64(void *pos, int pos_f64, int64_t n, const void *w, double Lbox, int nmesh, int paste, double offset, double *field);
int abacus_field_fft_f64(void *pos, int pos_f64, int64_t n, const void *w, double Lbox, int nmesh, int paste, const float *W,
                         void *out_c128);
int abacus_power_f64(void *pos, int pos_f64, int64_t n, const void *w, void *pos2, int64_t n2, const void *w2, double Lbox, int nmesh,
                     int paste, const float *W, const double *kedges, int Nk, const double *muedges, int Nmu, const int64_t *poles,
                     int Np, float *power, int64_t *N_mode, float *binned_poles, int64_t *N_mode_poles, float *k_avg);
/*
 * replaces: calc_pk_from_deltak = get_raw_power + bin_kmu (analysis/power_spectrum.py:730-805, 707-727, 150-300)
 * on host spectra.  field2 may be NULL (auto power).  Outputs as bin_kmu returns them, already multiplied by L^3:
 * power (Nk,Nmu) f32, N_mode (Nk,Nmu) i64, binned_poles (Np,Nk) f32, N_mode_poles (Nk) i64, k_avg (Nk,Nmu) f32.
 */
int abacus_pk_from_deltak(const void *field_c64, const void *field2_c64, int nmesh, double Lbox,
                          const double *kedges, int Nk, const double *muedges, int Nmu, const int64_t *poles, int Np,
                          float *power, int64_t *N_mode, float *binned_poles, int64_t *N_mode_poles, float *k_avg);
/*
 * replaces: the whole calc_power chain (analysis/power_spectrum.py:1131-1319) without the spectrum ever leaving
 * HBM: deposit(s) -> FFT(s) -> [interlace combine] -> fused scale/compensate/|delta_k|^2/bin pass.
 * pos2 == NULL -> auto power.  Host inputs; `pos`/`pos2` are wrapped in place like the reference.
 */
int abacus_power_from_particles(float *pos, int64_t n, const float *w, float *pos2, int64_t n2, const float *w2,
                                double Lbox, int nmesh, int paste, const float *W, int interlaced,
                                const double *kedges, int Nk, const double *muedges, int Nmu, const int64_t *poles,
                                int Np, float *power, int64_t *N_mode, float *binned_poles, int64_t *N_mode_poles,
                                float *k_avg);
/* the same for float64 positions (and weights): the cloud weights are evaluated in float64, as the reference computes them
 * in the dtype of the positions (analysis/tsc.py:400 `ftype = positions.dtype.type`); the mesh and the transform stay float32 */
int abacus_power_from_particles_f64(double *pos, int64_t n, const double *w, double *pos2, int64_t n2, const double *w2,
                                    double Lbox, int nmesh, int paste, const float *W_host, int interlaced,
                                    const double *kedges, int Nk, const double *muedges, int Nmu, const int64_t *poles,
                                    int Np, float *power, int64_t *N_mode, float *binned_poles, int64_t *N_mode_poles,
                                    float *k_avg);
/* same with DEVICE particle arrays (bench / HOD-to-P(k) without leaving HBM); outputs are host arrays */
int abacus_power_from_particles_dev(float *pos, int64_t n, const float *w, float *pos2, int64_t n2,
                                    const float *w2, double Lbox, int nmesh, int paste, const float *W_host,
                                    int interlaced, const double *kedges, int Nk, const double *muedges, int Nmu,
                                    const int64_t *poles, int Np, float *power, int64_t *N_mode,
                                    float *binned_poles, int64_t *N_mode_poles, float *k_avg);

/* Multi-tracer spectra (hod/abacus_hod.py:1338-1472 `compute_power`: every auto and cross pair of the tracers) without
 * repeated work and without leaving HBM: `abacus_power_field_soa64` deposits + transforms ONE tracer's galaxies - given as
 * the float64 x | y | z columns of abacus_hod_device_columns, cast to float32 and wrapped like calc_power does - into field
 * slot `slot` (< 8), which stays resident; `abacus_power_from_fields` bins the auto (slot_a == slot_b) or cross spectrum of
 * two resident fields.  LRG x ELG: 2 deposits + FFTs instead of the 4 of three calc_power calls. */
int abacus_power_field_soa64(int slot, const double *x, const double *y, const double *z, int64_t n, double Lbox, int nmesh,
                             int paste, int interlaced);
int abacus_power_from_fields(int slot_a, int slot_b, const float *W_host, const double *kedges, int Nk, const double *muedges,
                             int Nmu, const int64_t *poles, int Np, float *power, int64_t *N_mode, float *binned_poles,
                             int64_t *N_mode_poles, float *k_avg);
int abacus_power_fields_release(void);
/* releases cached FFT plans / work meshes / the cached binning geometry of fft_x_bin */
int abacus_power_release(void);
/* frees the idle scratch blocks the host-array entry points (abacus_prepare_*, abacus_argsort_i64, abacus_searchsorted_i64,
 * abacus_fenv_rank) keep between calls instead of paying hipMalloc + hipFree per temporary */
int abacus_scratch_release(void);
/* milliseconds of the one-off geometry pass behind the most recent fused last pass (abacus_power_from_particles[_dev],
 * auto power, non-interlaced, nmesh 1024 / 2048): N_mode, k_avg and the (k, mu) bin of every mode depend on (nmesh, edges)
 * alone (power_spectrum.py:233-256), so they are computed once per (nmesh, edges) and cached; 0 if none was built */
double abacus_power_geometry_ms(void);
/* diagnostic: batches in which the most recent abacus_power_from_particles uploaded its (first) host position array - more than one
 * when the upload runs on a copy stream behind the deposits of the batches before (csrc/power.hip, HostSrc; option pk_nobatch = 1
 * forces one) */
double abacus_power_last_batches(void);
/* which fused last pass served the most recent spectrum: 2 = cached-geometry kernel, 1 = first generation (bin walk in the
 * kernel: more than 8 mu bins, edges the cell table cannot resolve, option pk_xbin_gen = 1), 0 = none yet */
int abacus_power_xbin_generation(void);


/* ---------------------------------------------------------------- multi-GPU slab building blocks ------- */
/*
 * The reference has no distributed mesh (docs/tutorials/analysis/tsc.ipynb:19); this is new functionality behind
 * calc_power: x-slab mesh decomposition, ghost-plane exchange-add, local z/y FFT passes, all-to-all pencil transpose,
 * x FFT pass and binning on y-slabs, all-reduce of the (k, mu) histogram.  The collectives are the
 * abacus_comm_* entry points below (RCCL); these entry points are the device-side pieces.
 * All pointers are DEVICE pointers; nmesh must be a power of two in [64, 2048] and divisible by twice the number of ranks.
 * Mesh rows have abacus_slab_pitch(nmesh) floats (128-B aligned rows; complex rows of pitch/2).
 */
int abacus_slab_pitch(int nmesh);
/* deposit into planes [xoff, xoff + nx_local) (mod nmesh) of the global mesh as rho*norm - sub (ghost planes included);
 * xoff2 >= 0: TWO windows of nx_local planes each, starting at xoff and xoff2 and stored back to back (the two slabs of a
 * rank's folded pair with their ghosts) - a plane both windows hold receives its deposits in the first.  Particles whose
 * clouds lie outside are skipped.
 * sub = 1: every cell already carries the "-1" of the overdensity (normalize_field, power_spectrum.py:860-901) - a ghost
 * block is then added to its owner as `ghost + 1` (abacus_slab_axpy_dev with add = 1) and no pass over the mesh is spent
 * on the subtraction; xoff2 < 0 and nx_local == nmesh with xoff == 0 is the whole periodic mesh (one rank: no ghosts) */
int abacus_slab_deposit_dev(float *pos, int64_t n, const float *w, float *mesh, int nmesh, int xoff, int xoff2, int nx_local,
                            double Lbox, double offset, double norm, int paste, double sub);
/* the same with a `mesh` buffer the caller padded to nx_alloc planes, nx_alloc the window planes (nx_local, or 2 nx_local with two
 * windows) rounded up to a multiple of 16: unweighted float32 TSC of >= 2e6 particles then takes the third-generation list build
 * of the single-GPU path on the windows' local planes (csrc/tsc_lines3.hpp, L3Win); the padding planes are overwritten.
 * nx_alloc = 0: no padding, the first-generation lists (what abacus_slab_deposit_dev runs). */
int abacus_slab_deposit_padded_dev(float *pos, int64_t n, const float *w, float *mesh, int nmesh, int xoff, int xoff2, int nx_local,
                                   double Lbox, double offset, double norm, int paste, double sub, int nx_alloc);
/* dst[i] += src[i] + add  (ghost-plane accumulation; a constant alone with src == NULL) */
int abacus_slab_axpy_dev(float *dst, const float *src, int64_t nfloat, float add);
/* FOLDED SLABS.  With W ranks the mesh is cut into 2 W slabs of h = nmesh / (2 W) planes and rank r owns slabs r and
 * r + W: the planes x and x + nmesh/2 of a pair sit on ONE rank, so the fused form of the transform (first radix-2 stage of
 * y and x inside the z pass, fft.hip) runs on a slab exactly as on the whole mesh.  A rank's buffer holds its two halves
 * `xsep` planes apart (ghost planes in between).
 *
 * z and y passes of the plane pairs [p0, p0 + pc) of the rank's h pairs: `mesh` = first plane of the first half (global
 * plane xg0; the second half is global plane xg0 + nmesh/2).  send == NULL: in place.  send != NULL: the result goes to the
 * send buffer of the pencil transpose, send[peer][s h + p][y_local][k] (s = 0 / 1: first / second half) - written by the y
 * pass itself where the fused form runs with more than one rank, by a pack pass otherwise */
int abacus_slab_fft_zy_dev(float *mesh, void *send, int nmesh, int world, int64_t xsep, int xg0, int p0, int pc);
/* COMPACT pencil transpose (new functionality like the rest of the slab path; csrc/fft.hip `slab_layout`).  When the spectrum goes
 * to a binning that ends at k_last and nowhere else, the columns of a y row beyond sqrt(k_last^2 - ky^2) never cross the links:
 * a row keeps its first row_len columns (a multiple of 16, decided per aligned group of 16 rows), the rows of a peer's plane block
 * are packed back to back - 21 % fewer bytes when the bins end at the Nyquist frequency.
 * abacus_slab_transpose_layout: P_out[p] = complex elements per plane of the block that goes to peer p (so a rank sends
 * 2 h P_out[p] elements to p and receives 2 h P_out[rank] from everybody); returns 1 when this mesh / rank count has no compact
 * form (then use the regular layout).  abacus_slab_fft_zy_compact_dev writes that send buffer; the receive buffer is read by
 * abacus_slab_xbin_dev(from_transpose = 2) */
int abacus_slab_transpose_layout(int nmesh, int world, double Lbox, double k_last, int64_t *P_out);
int abacus_slab_fft_zy_compact_dev(float *mesh, void *send, int nmesh, int world, int64_t xsep, int xg0, int p0, int pc, double Lbox,
                                   double k_last);
/* the pack pass alone (pairs [p0, p0 + pc)), and recv[q][s h + p][y_local][k] -> out[y_local][s nmesh/2 + q h + p][k]: row
 * s nmesh/2 + i of x is plane i of half s - the plane itself in the plain form; in the fused form the sum (s = 0) or the
 * twiddled difference (s = 1) of planes i and i + nmesh/2, i.e. the inputs of the two nmesh/2-point transforms */
int abacus_slab_pack_dev(const void *data, void *send, int nmesh, int world, int64_t xsep, int p0, int pc);
int abacus_slab_unpack_dev(const void *recv, void *out, int nmesh, int world);
/* x pass on a y-slab in the (y_local, x, k) layout, in place */
int abacus_slab_fft_x_dev(float *data, int nmesh, int ny_local);
/* raw (un-normalised) bin sums of a y-slab: counts u64[Nk*Nmu], sum P f64[Nk*Nmu], sum k f64[Nk*Nmu],
 * pole sums f64[Np'*Nk]; `raw_out` is a HOST buffer of abacus_bin_raw_bytes() bytes (to be all-reduced) */
int abacus_slab_bin_dev(const void *a, const void *as, const void *b, const void *bs, int nmesh, int y0, int ny_local,
                        double Lbox, const float *W_host, int interlaced, const double *kedges, int Nk,
                        const double *muedges, int Nmu, const int64_t *poles, int Np, void *raw_out);
int64_t abacus_bin_raw_bytes(int Nk, int Nmu, const int64_t *poles, int Np);
/* 1 if the slab entry points above run the FUSED form of the transform for this mesh (nmesh 1024 / 2048, like the single-GPU
 * path: n/2-point column passes with 128-B row segments; rows of x and y then come out in the order
 * f = 2 (r mod n/2) + (r div n/2), which abacus_slab_bin_dev and abacus_slab_xbin_dev undo) */
int abacus_slab_fused(int nmesh);
/* last x pass FUSED with the binning on a y-slab (auto power of one non-interlaced field): replaces abacus_slab_fft_x_dev +
 * abacus_slab_bin_dev.  from_transpose = 0: `mesh` is the unpacked (y_local, x, k) block; from_transpose = 1: `mesh` is the
 * RECEIVE buffer of the pencil transpose of a `world`-rank run as it arrived, (peer, 2 h, y_local, k) - no unpack at all,
 * the kernel gathers the rows of a column from the peers' blocks while staging (one rank: the slab itself after its z / y
 * passes).  Returns 0 (raw sums in the host buffer raw_out), 1 when this mesh / histogram is not served (use the two-step
 * form), < 0 on error.  put_geom = 1 on exactly one rank: N_mode and sum |k| are mesh-wide quantities taken from the
 * cached geometry of (nmesh, edges), not from the y-slab */
int abacus_slab_xbin_dev(const void *mesh, int nmesh, int world, int y0, int ny_local, double Lbox, const float *W_host,
                         const double *kedges, int Nk, const double *muedges, int Nmu, const int64_t *poles, int Np,
                         int put_geom, int from_transpose, void *raw_out);
/* the same over two fields in the same layout.  pair_mode 2: their cross power Re(conj(a) b) (calc_power(pos, pos2=...,
 * interlaced=False), analysis/power_spectrum.py:707-727 with field2_fft); pair_mode 1: mesh2 is the half-cell-shifted deposit of
 * the same particles - the auto power of the interlaced combination (:951-998); pair_mode 0 is abacus_slab_xbin_dev (mesh2
 * ignored).  The query form (mesh == NULL) answers for the pair_mode given */
int abacus_slab_xbin_pair_dev(const void *mesh, const void *mesh2, int pair_mode, int nmesh, int world, int y0, int ny_local, double Lbox,
                              const float *W_host, const double *kedges, int Nk, const double *muedges, int Nmu, const int64_t *poles,
                              int Np, int put_geom, int from_transpose, void *raw_out);
/* ... and over four: pair_mode 3 = the cross power of two INTERLACED fields (calc_power(pos, pos2=..., interlaced=True) over slabs,
 * analysis/power_spectrum.py:1200-1260): mesh / mesh2 the first catalogue's unshifted / shifted deposit, mesh3 / mesh4 the second
 * catalogue's, all in the layout of `mesh`; pair_mode 0 - 2 as abacus_slab_xbin_pair_dev (mesh3 / mesh4 ignored) */
int abacus_slab_xbin_quad_dev(const void *mesh, const void *mesh2, const void *mesh3, const void *mesh4, int pair_mode, int nmesh, int world,
                              int y0, int ny_local, double Lbox, const float *W_host, const double *kedges, int Nk, const double *muedges,
                              int Nmu, const int64_t *poles, int Np, int put_geom, int from_transpose, void *raw_out);
/* particle routing on the device: stable bucket sort of (pos (n,3) float32, w or NULL) by the rank that owns the wrapped x
 * (fold = 0: x-slabs of width Lbox / world; fold = 1: the folded slabs above, rank = slab mod world of 2 world slabs);
 * counts[world] on the host.  The blocks then travel with abacus_comm_all_to_all_v. */
int abacus_slab_route_dev(const float *pos, int64_t n, const float *w, double Lbox, int world, int fold, float *pos_out,
                          float *w_out, int64_t *counts);
/* bin_kmu's normalisation (analysis/power_spectrum.py:276-293, 789-792) of reduced raw sums; host only */
int abacus_bin_finalize(const void *raw, double Lbox, int Nk, int Nmu, const int64_t *poles, int Np, float *power,
                        int64_t *N_mode, float *binned_poles, int64_t *N_mode_poles, float *k_avg);

/* ---------------------------------------------------------------- multi-GPU communicator (RCCL) -------- */
/*
 * One process per GPU; the collectives of the slab-decomposed P(k), the sharded HOD and the slab pair counts
 * (SURVEY.md 8e).  New functionality: the reference is single-node shared-memory (its unit of decomposition is the slab
 * chunk, hod/abacus_hod.py:301-312).  librccl is opened on first use.  Rank 0 creates the 128-byte id and distributes it
 * out of band (abacusutils_amd/comm.py: file rendezvous); abacus_comm_init = ncclCommInitRank on the device selected with
 * abacus_set_device.  Device-buffer collectives are enqueued on the library stream and never synchronise with the host;
 * `async` != 0 runs them on the communicator's own stream behind the kernels enqueued so far - abacus_comm_join puts the
 * library stream behind them again (pencil-transpose chunks overlap the FFT passes of the next chunk).
 * dtype codes: 0 int64, 1 float64, 2 float32, 3 uint64; op: 0 sum, 1 max.
 */
#define ABACUS_COMM_ID_BYTES 128
typedef struct abacus_comm abacus_comm;
int abacus_comm_unique_id(void *id, int len);
int abacus_comm_init(int rank, int world, const void *id, int len, abacus_comm **out);
int abacus_comm_info(const abacus_comm *c, int *rank, int *world, int *rccl_version, uint64_t *bytes_sent);
int abacus_comm_free(abacus_comm *c);
int abacus_comm_abort(abacus_comm *c);   /* ncclCommAbort: after a failed or abandoned collective */
int abacus_comm_join(abacus_comm *c);
/* block p of `send` (bytes_per_peer each) goes to rank p, block p of `recv` comes from rank p: ONE group of
 * ncclSend / ncclRecv, every xGMI link busy at once */
int abacus_comm_all_to_all(abacus_comm *c, const void *send, void *recv, uint64_t bytes_per_peer, int async);
/* the same for the piece [offset, offset + bytes) of every peer block (blocks `peer_stride` bytes apart): chunks of the
 * pencil transpose */
int abacus_comm_all_to_all_strided(abacus_comm *c, const void *send, void *recv, uint64_t peer_stride, uint64_t offset,
                                   uint64_t bytes, int async);
/* variable blocks (device-side particle routing): byte counts and offsets per peer, host arrays of `world` entries */
int abacus_comm_all_to_all_v(abacus_comm *c, const void *send, const uint64_t *send_bytes, const uint64_t *send_off, void *recv,
                             const uint64_t *recv_bytes, const uint64_t *recv_off);
/* the same on the communicator's own stream behind an event fork when async != 0 (chunks of the compact pencil transpose) */
int abacus_comm_all_to_all_v_async(abacus_comm *c, const void *send, const uint64_t *send_bytes, const uint64_t *send_off, void *recv,
                                   const uint64_t *recv_bytes, const uint64_t *recv_off, int async);
/* ghost blocks: to_left -> rank-1, to_right -> rank+1; from_right <- what rank+1 sent left, from_left <- what rank-1 sent
 * right (one rank: its own blocks come back, the periodic box) */
int abacus_comm_ring_exchange(abacus_comm *c, const void *to_left, const void *to_right, void *from_right, void *from_left,
                              uint64_t bytes);
int abacus_comm_allreduce_dev(abacus_comm *c, void *buf, int64_t count, int dtype, int op);   /* in place, device buffer */
/* host-buffer conveniences for the few-KB messages (histograms, counts, timings): staged through device scratch, blocking */
int abacus_comm_allreduce_host(abacus_comm *c, void *buf, int64_t count, int dtype, int op);
int abacus_comm_allgather_host(abacus_comm *c, const void *send, void *recv, uint64_t bytes);
int abacus_comm_barrier(abacus_comm *c);

/* ---------------------------------------------------------------- ZCV-facing spectrum helpers ----------- */
/*
 * replaces the remaining Numba kernels of analysis/power_spectrum.py that the control-variates code calls
 * (zcv/tools_cv.py:320,805-923, zcv/tracer_power.py:456).  Grids are host arrays in the rfftn layout (n, n, n/2+1)
 * unless a z-extent `zdim` is given ((n, n, n) real-space grids: zdim = n, only k <= n/2 is read, like the reference).
 */
/* bin_kmu (:150-300) of a caller-supplied real grid: project_3d_to_poles (:415-448) with one mu bin and scale = L^3.
 * fourier = 0 bins a configuration-space grid (dk = L/n, :212).  scale multiplies the means (<= 0: 1). */
int abacus_bin_weights(const float *weights, int n1d, int zdim, double Lbox, int fourier, const double *kedges, int Nk,
                       const double *muedges, int Nmu, const int64_t *poles, int Np, double scale, float *power,
                       int64_t *N_mode, float *binned_poles, int64_t *N_mode_poles, float *k_avg);
/* pk_to_xi (:620-660): Xi = irfftn(Pk) on the device (hipFFT C2R), multipoles of Xi in r bins, times nmesh^3 */
int abacus_pk_to_xi(const float *Pk, int n, double Lbox, const double *redges, int Nr, const int64_t *poles, int Np,
                    float *binned_poles, int64_t *N_poles);
/* bin_kppi (:303-412): mean and mode count per (k_perp, pi) bin, pi edges linspace(0, pimax, Npi+1).  The reference's j
 * loop breaks at the first k_perp beyond the last edge (the rest of that i row is never visited): kept. */
int abacus_bin_kppi(const float *weights, int n1d, int zdim, double Lbox, const double *kedges, int Nk, double pimax, int Npi,
                    int fourier, float *mean, int64_t *counts);
/* get_raw_power (:707-727): |field|^2, or Re(conj(field) field2), of `total` complex64 values -> float32 */
int abacus_raw_power(const void *field_c64, const void *field2_c64, int64_t total, float *out);
/* shift_field_fft (:904-948), in place on `field`: (field + shift * exp(i (d / 2)(kx + ky + kz))) * 0.5 / n1d^3, float32
 * wavenumbers as the reference forms them */
int abacus_shift_field_fft(void *field_c64, const void *shift_c64, int n1d, double Lbox, double d);
/* get_smoothing (:527-577), get_delta_mu2 (:580-617), expand_poles_to_3d (:451-505) */
int abacus_get_smoothing(int n1d, double Lbox, double R, float *out);
int abacus_get_delta_mu2(const void *delta_c64, int n1d, void *out_c64);
int abacus_expand_poles_to_3d(const double *k_ell, const double *P_ell, int nk, int n1d, double Lbox, const int64_t *poles,
                              int Np, float *out);

/* ---------------------------------------------------------------- pair counting ------------------------ */
/*
 * replaces: Corrfunc.theory.DD / DDrppi / DDsmu as called at analysis/tpcf_corrfunc.py:144-156,164-179,
 * 240-273,328-362 and scripts/emulator/generate_cfs/generate_cf.py:65-74 (third-party C, periodic box,
 * float32 coordinates).  mode 0: DD(r), 1: DD(rp,pi) with pi bins of width pimax/npibins, 2: DD(s,mu) with
 * nmubins in [0,mu_max).  x2 == NULL -> autocorrelation (ordered pairs, no self pairs).
 * npairs: nbins * (1 | npibins | nmubins) uint64.
 *
 * Every pair-count entry of this section (abacus_paircount* - plain, weighted, _los, _jk, their _dev forms) validates all of
 * its arguments before the device is touched: a refused call returns non-zero without initialising or launching anything,
 * and its message (abacus_last_error) starts with the name of the entry that was called.  Common rules: mode 0 .. 2; the
 * columns of set 1, bins (and origin / npairs where taken) not NULL; nbins >= 1; y2 and z2 given with x2; w2 (labels2) NULL
 * for an autocorrelation; 0 <= n1, n2 < 2^31; strictly increasing bin edges; pos_dtype ABACUS_F32 or ABACUS_F64.  Periodic
 * entries: boxsize > 0, at least one pi / mu bin in modes 1 / 2, and neither the last edge nor (mode 1) pimax above half the
 * box.  An empty set returns zeros.
 * The bookkeeping entries (abacus_paircount_stats, abacus_paircount_los_grid, abacus_paircount_jk_stats) describe the last
 * pair-count call that passed validation, whichever entry it was: all of them are zero after a call with an empty set or one
 * that failed on the device, and those a call does not produce (the open grid after a periodic call, the jackknife figures
 * after a plain one) are zero too.
 */
int abacus_paircount(int mode, const float *x1, const float *y1, const float *z1, int64_t n1, const float *x2,
                     const float *y2, const float *z2, int64_t n2, float boxsize, const float *bins, int nbins,
                     float pimax, int npibins, float mu_max, int nmubins, uint64_t *npairs);
/* the same with the coordinate columns already in HBM (pos_dtype ABACUS_F32, or ABACUS_F64: cast to float32 on the
 * device as analysis/tpcf_corrfunc.py:134-139 casts on the host) - e.g. the catalogue columns of
 * abacus_hod_device_columns: the HOD -> clustering step of hod/abacus_hod.py:1181-1336 without a PCIe round trip.
 * Coordinates may lie in any interval of one box length ([0, L), [-L/2, L/2), ...), as Corrfunc accepts them. */
int abacus_paircount_dev(int mode, const void *x1, const void *y1, const void *z1, int64_t n1, const void *x2,
                         const void *y2, const void *z2, int64_t n2, int pos_dtype, float boxsize, const float *bins,
                         int nbins, float pimax, int npibins, float mu_max, int nmubins, uint64_t *npairs);

/*
 * Weighted counts (Corrfunc's weights1 / weights2 with weight_type='pair_product', and its output_ravg / _rpavg / _savg).
 * Beside npairs - bit-equal to what abacus_paircount returns for the same arguments - and laid out like it:
 *   wsum  sum over the bin's pairs of w_i * w_j: float32 weights, the product formed in float64 (exact) and
 *         accumulated in float64;
 *   rsum  sum of the pair's separation - r (mode 0), rp = sqrt(dx^2 + dy^2) (mode 1), s (mode 2): the correctly rounded
 *         float32 square root of the r^2 that chose the bin, accumulated in float64.  NULL: not computed.
 * w1 / w2 NULL: unit weights.  x2 == NULL is the autocorrelation (ordered pairs) and w2 must then be NULL.
 * The sums are accumulated by float64 atomics: their last bits depend on the run, |error| <= n * 2^-52 * sum|term| of a bin
 * with n pairs.  abacus_paircount_stats reports the candidate pairs of a weighted call too (stencil_R = 0).
 * _dev: coordinates as in abacus_paircount_dev, w1 / w2 float32 DEVICE pointers.
 */
int abacus_paircount_weighted(int mode, const float *x1, const float *y1, const float *z1, const float *w1, int64_t n1,
                              const float *x2, const float *y2, const float *z2, const float *w2, int64_t n2, float boxsize,
                              const float *bins, int nbins, float pimax, int npibins, float mu_max, int nmubins,
                              uint64_t *npairs, double *wsum, double *rsum);
int abacus_paircount_weighted_dev(int mode, const void *x1, const void *y1, const void *z1, const float *w1, int64_t n1,
                                  const void *x2, const void *y2, const void *z2, const float *w2, int64_t n2, int pos_dtype,
                                  float boxsize, const float *bins, int nbins, float pimax, int npibins, float mu_max,
                                  int nmubins, uint64_t *npairs, double *wsum, double *rsum);

/*
 * Pairwise velocity sums on the periodic box: what the mean pairwise infall v12(r), the radial and transverse pairwise
 * dispersions and the line-of-sight pairwise mean and dispersion in (rp, pi) are moments of (halotools' mean_radial_velocity_vs_r,
 * radial_pvd_vs_r, mean_los_velocity_vs_rp, los_pvd_vs_rp; no halotools run stands behind this - the contract below is pinned
 * against the NumPy statement tests/pairvel_statement.py).
 *   sets     float32 columns x, y, z, vx, vy, vz and optional float32 weights w (NULL: unit weights).  The _dev form takes the
 *            six columns of a set in HBM, all of pos_dtype; ABACUS_F64 columns are rounded once to float32 on the device,
 *            velocities like positions.  x2 == NULL: autocorrelation (w2 must be NULL, the velocities of set 2 are not read).
 *   pairs    ordered; self pairs of an autocorrelation are excluded.  A pair is in a (bin, sub-bin) exactly when
 *            abacus_paircount_weighted puts it there for the same mode, bins, pimax, npibins, mu_max, nmubins: float32
 *            d = p_i - p_j with one minimum-image addition, float32 r2 against float32 squared edges, modes 0 (r), 1 (rp, pi),
 *            2 (s, mu) with that entry's sub-bin rules.  npairs and wsum are that entry's.
 *   a pair   u = v_i - v_j componentwise in float32; then in float64, left to right, no FMA:
 *              s2 = dx dx + dy dy + dz dz          t = ux dx + uy dy + uz dz
 *              vr = s2 > 0 ? t / sqrt(s2) : 0      (negative: the pair approaches)
 *              uu = ux ux + uy uy + uz uz
 *              vz = uz * sign(dz)                  (the sign of the minimum-image float32 dz, sign(0) = 0: the line of sight is z)
 *   sums     per (bin, sub-bin), with ww = (double)w_i * (double)w_j, all float64:
 *              npairs, wsum = sum ww, and in vsum - one block [5][nbins * nsub] -
 *              vr1 = sum ww vr | vr2 = sum ww vr^2 | u2 = sum ww uu | vz1 = sum ww vz | vz2 = sum ww uz^2.
 *            Accumulated by float64 atomics: |error| <= (n + 8) * 2^-52 * sum|term| of a cell with n pairs, the 8 for a
 *            square root and a division that may each differ from the host's by an ulp.
 * The moments: v12 = vr1 / wsum, sigma_r^2 = vr2 / wsum - v12^2, sigma_t^2 = (u2 - vr2) / (2 wsum) per transverse direction,
 * vlos = vz1 / wsum, sigma_los^2 = vz2 / wsum - vlos^2.
 * Validation as for every entry of this section (before the device is touched, the message starts with the entry's name),
 * with the rules of the periodic entries and: no velocity column of set 1 NULL; in a cross count the velocities of set 2 given
 * (all NULL: "velocities ... but not for set 2", some NULL: a null velocity column); wsum and vsum not NULL.  At most 1024
 * sub-bins; binnings of more than 1024 entries are counted in runs of separation bins.  abacus_paircount_stats reports the
 * candidate pairs of this call too (stencil_R = 0).  Periodic box only: no light cone, no jackknife regions.
 */
int abacus_pairvel(int mode, const float *x1, const float *y1, const float *z1, const float *vx1, const float *vy1,
                   const float *vz1, const float *w1, int64_t n1, const float *x2, const float *y2, const float *z2,
                   const float *vx2, const float *vy2, const float *vz2, const float *w2, int64_t n2, float boxsize,
                   const float *bins, int nbins, float pimax, int npibins, float mu_max, int nmubins, uint64_t *npairs,
                   double *wsum, double *vsum);
int abacus_pairvel_dev(int mode, const void *x1, const void *y1, const void *z1, const void *vx1, const void *vy1,
                       const void *vz1, const float *w1, int64_t n1, const void *x2, const void *y2, const void *z2,
                       const void *vx2, const void *vy2, const void *vz2, const float *w2, int64_t n2, int pos_dtype,
                       float boxsize, const float *bins, int nbins, float pimax, int npibins, float mu_max, int nmubins,
                       uint64_t *npairs, double *wsum, double *vsum);

/* bookkeeping of the last pair-count call (bench.py's roofline): candidate pair separations the kernel evaluated (0 when an
 * older-generation kernel ran), cells per dimension in xy / z, stencil half-width in cells (1 or 2; 0: older kernel) */
int abacus_paircount_stats(uint64_t *candidates, int *ncell_xy, int *ncell_z, int *stencil_R);

/*
 * Light-cone pair counts: a line of sight that belongs to the PAIR, on an open (non-periodic) grid - what
 * Corrfunc.mocks.DDrppi_mocks / DDsmu_mocks compute from Cartesian columns.  No Corrfunc run stands behind this: the
 * conventions below are the contract, pinned against the NumPy statement tests/pairs_los_statement.py.
 *   points   p = float32(column - origin[d]), the subtraction in the column's own dtype (float64 columns of the _dev form
 *            subtract in float64, float32 columns in float32); origin = (0, 0, 0) leaves float32 columns untouched;
 *   pair     d = p_i - p_j and l = p_i + p_j in float32, then float64, left to right, no FMA: s2 = d.d, l2 = l.l, t = d.l,
 *            pi2 = t t / l2; a pair with l2 == 0 is not counted in modes 1 and 2; self pairs of an autocorrelation are excluded;
 *   mode 0   bin s2.   mode 1: pi = sqrt(pi2) < (double)pimax, bin rp2 = max(s2 - pi2, 0), sub = int(pi / ((double)pimax / npibins)).
 *   mode 2   bin s2, mu = s2 > 0 ? sqrt(pi2 / s2) : 0 < (double)mu_max, sub = int(mu * (nmubins / (double)mu_max));
 *   bins     float32 edges >= 0, compared as (double)edge * (double)edge: bin b holds e2[b] <= q < e2[b + 1];
 *   sums     per (bin, sub-bin) npairs (ordered pairs for an autocorrelation), wsum = sum w_i w_j (float32 weights, product and
 *            sum in float64), rsum = sum sqrt(q) of the q that chose the bin (s | rp | s), float64.  The float64 atomics leave
 *            |error| <= n * 2^-52 * sum|term| per bin.
 * w1 / w2 NULL: unit weights; x2 == NULL: autocorrelation (w2 must be NULL).  wsum == NULL: integer counts only (rsum is then
 * ignored); rsum == NULL: not computed.  Arguments are validated before the device is touched.
 * _dev: coordinate columns in HBM (pos_dtype ABACUS_F32 / ABACUS_F64), w1 / w2 float32 DEVICE pointers.
 * abacus_paircount_stats reports the candidate pairs (summed over the runs of a call with more than 63 separation bins) and
 * the x / z cell counts of such a call (stencil_R = 0); abacus_paircount_los_grid the cell counts of all three dimensions.
 */
int abacus_paircount_los(int mode, const float *x1, const float *y1, const float *z1, const float *w1, int64_t n1,
                         const float *x2, const float *y2, const float *z2, const float *w2, int64_t n2, const double *origin,
                         const float *bins, int nbins, float pimax, int npibins, float mu_max, int nmubins, uint64_t *npairs,
                         double *wsum, double *rsum);
int abacus_paircount_los_dev(int mode, const void *x1, const void *y1, const void *z1, const float *w1, int64_t n1,
                             const void *x2, const void *y2, const void *z2, const float *w2, int64_t n2, int pos_dtype,
                             const double *origin, const float *bins, int nbins, float pimax, int npibins, float mu_max,
                             int nmubins, uint64_t *npairs, double *wsum, double *rsum);
int abacus_paircount_los_grid(int *ncell /* [3] */);
/* one device column, observer-centred: dst[i] = float32(src[i] - origin), subtracted in the column's dtype (pos_dtype) */
int abacus_paircount_los_centre(const void *src, int pos_dtype, int64_t n, double origin, float *dst);

/*
 * Jackknife pair counts: the per-region counts of a delete-one jackknife from ONE pair walk (no reference code and no
 * Corrfunc run stands behind this; pinned against the NumPy statement tests/pairs_jk_statement.py).  Every point carries an
 * int32 label in [0, nreg).  Pairs and bins are exactly those of abacus_paircount_weighted (abacus_paircount_jk) and of
 * abacus_paircount_los (abacus_paircount_los_jk) for the same columns, weights and binning; per (bin, sub-bin) q, region k:
 *   first[k][q]  over the pairs (i, j) of q with labels1[i] == k
 *   both[k][q]   over those with labels1[i] == k and labels2[j] == k   (autocorrelation: labels2 = labels1)
 * each as an integer count (npairs_*) and as sum of w_i w_j (wsum_*: float64 products and sums, |error| <= n 2^-52 sum|term|),
 * laid out [nreg][nbins * (1 | npibins | nmubins)].  sum_k first[k][q] is the parent's result (npairs bit for bit); there
 * are no separation sums.  The count over labels2[j] == k ("second") is no output: membership of a pair is symmetric
 * under exchange of its points in every mode (d -> -d; l, |dz| and t^2 are unchanged), so it is `first` of the call with the
 * two sets exchanged - and `first` itself for an autocorrelation; `both` of the two calls agrees exactly in npairs.
 * Limits, checked on the host before anything is launched (an error code and a message, never a device fault):
 * 1 <= nreg <= 65535; nreg * nbins * sub-bins <= 2^24; every label in [0, nreg) (a device reduction over the labels runs
 * before the sort); labels2 must be NULL for an autocorrelation (x2 == NULL), like w2.  Regions without points are fine:
 * their rows are zero.  wsum_first / wsum_both: required on the box; on the light cone both NULL = integer counts only.
 * abacus_paircount_stats reports the candidate pairs - the parent's for the same input and grid.
 * _dev: coordinate columns in HBM (pos_dtype), w1 / w2 float32 and labels1 / labels2 int32 DEVICE pointers.
 */
int abacus_paircount_jk(int mode, const float *x1, const float *y1, const float *z1, const float *w1, const int32_t *labels1,
                        int64_t n1, const float *x2, const float *y2, const float *z2, const float *w2, const int32_t *labels2,
                        int64_t n2, int nreg, float boxsize, const float *bins, int nbins, float pimax, int npibins,
                        float mu_max, int nmubins, uint64_t *npairs_first, uint64_t *npairs_both, double *wsum_first,
                        double *wsum_both);
int abacus_paircount_jk_dev(int mode, const void *x1, const void *y1, const void *z1, const float *w1, const int32_t *labels1,
                            int64_t n1, const void *x2, const void *y2, const void *z2, const float *w2, const int32_t *labels2,
                            int64_t n2, int pos_dtype, int nreg, float boxsize, const float *bins, int nbins, float pimax,
                            int npibins, float mu_max, int nmubins, uint64_t *npairs_first, uint64_t *npairs_both,
                            double *wsum_first, double *wsum_both);
int abacus_paircount_los_jk(int mode, const float *x1, const float *y1, const float *z1, const float *w1, const int32_t *labels1,
                            int64_t n1, const float *x2, const float *y2, const float *z2, const float *w2,
                            const int32_t *labels2, int64_t n2, int nreg, const double *origin, const float *bins, int nbins,
                            float pimax, int npibins, float mu_max, int nmubins, uint64_t *npairs_first, uint64_t *npairs_both,
                            double *wsum_first, double *wsum_both);
int abacus_paircount_los_jk_dev(int mode, const void *x1, const void *y1, const void *z1, const float *w1, const int32_t *labels1,
                                int64_t n1, const void *x2, const void *y2, const void *z2, const float *w2,
                                const int32_t *labels2, int64_t n2, int pos_dtype, int nreg, const double *origin,
                                const float *bins, int nbins, float pimax, int npibins, float mu_max, int nmubins,
                                uint64_t *npairs_first, uint64_t *npairs_both, double *wsum_first, double *wsum_both);
/* histogram flushes (summed over the workgroups and runs) and workgroups (of the last run) of the last jackknife call */
int abacus_paircount_jk_stats(uint64_t *flushes, int *workgroups);
/* labels of an nx x ny x nz split of the periodic box from resident columns (pos_dtype), into the int32 DEVICE array `labels`:
 * (cx * ny + cy) * nz + cz with c = int(frac(float32(v) * (1 / boxsize)) * n) in float32, the fraction wrapped into [0, 1) as
 * the counter's cell grid wraps it (a coordinate that rounds to boxsize lands in sub-box 0, not n), c clamped to [0, n - 1] */
int abacus_jk_box_labels_dev(const void *x, const void *y, const void *z, int pos_dtype, int64_t n, float boxsize, int nx, int ny,
                             int nz, int32_t *labels);

/*
 * Counts in spheres: for every query point the number of data points inside each of nr radii, on the periodic box - the
 * primitive under the void probability function and the count probabilities P_N(r) (Corrfunc.theory.vpf), the k-nearest-
 * neighbour CDFs (P(N(<r) >= k)) and counts-in-cells.  No reference code and no Corrfunc run stands behind this: the
 * conventions below are the contract, pinned against the NumPy statement tests/spheres_statement.py, whose column sums are
 * tied to the pair counter's cumulative counts.
 *   inputs   data (x, y, z), n points; queries (qx, qy, qz), nq points, or qx == NULL: the data are the queries (qy, qz and nq
 *            are then ignored); float32 radii r_1 < ... < r_nr; pimax = 0: spheres, pimax > 0: cylinders along z;
 *   pair     float32, the expressions of abacus_paircount: d = q - p per component, one -+boxsize when |d| > boxsize / 2;
 *            r2 = dx dx + dy dy + dz dz left to right, no FMA; cylinders: r2 = dx dx + dy dy and the pair needs |dz| < pimax;
 *   inside   a data point is inside radius j iff r2 < e2[j], e2[j] = r_j * r_j as a float32 product.  Strict: N(<r_j) is the
 *            cumulative sum of the pair counter's [lo, hi) bins over the edges (0, r_1 .. r_nr);
 *   self     when the data are the queries a point does not count itself - by identity, not by distance: a coincident twin counts;
 *   hist     [nr][kmax + 1] uint64: hist[j][k] = queries with exactly k points inside r_j for k < kmax, hist[j][kmax] = those
 *            with kmax or more; every row sums to the number of queries;
 *   counts   NULL, or [nq][nr] uint32 (n rows when the data are the queries): N(<r_j) per query, in the CALLER's query order.
 * Checked before the device is touched (the message starts with the entry's name): 1 <= nr <= 32; kmax >= 1;
 * nr * (kmax + 1) <= 8192; radii positive and increasing; r_nr and pimax at most boxsize / 2; pimax >= 0; boxsize > 0;
 * 0 <= n, nq < 2^31; x, y, z, radii, hist (and qy, qz beside qx) not NULL; pos_dtype ABACUS_F32 or ABACUS_F64.
 * Empty cases: n = 0 gives hist[:][0] = nq and zero counts; nq = 0 gives zeros.
 * _dev: the columns of both sets in HBM, of ONE dtype (pos_dtype; float64 is cast to float32 on the device); radii, hist and
 * counts are host pointers in both forms.  Coordinates may lie in any interval, as for abacus_paircount_dev.
 * abacus_spherecount_stats: candidate (query, data) pairs evaluated and the cells per dimension in xy / z of the last call
 * (the figures abacus_paircount_stats reports for it, like for every counter of this section).
 */
int abacus_spherecount(const float *x, const float *y, const float *z, int64_t n, const float *qx, const float *qy,
                       const float *qz, int64_t nq, float boxsize, const float *radii, int nr, float pimax, int kmax,
                       uint64_t *hist, uint32_t *counts);
int abacus_spherecount_dev(const void *x, const void *y, const void *z, int64_t n, const void *qx, const void *qy, const void *qz,
                           int64_t nq, int pos_dtype, float boxsize, const float *radii, int nr, float pimax, int kmax,
                           uint64_t *hist, uint32_t *counts);
int abacus_spherecount_stats(uint64_t *candidates, int *ncell_xy, int *ncell_z);

/*
 * Friends-of-friends groups of one catalogue on the periodic box: a group label per point and the multiplicity function n(N)
 * (analysis/groups.py).  No reference code stands behind this: the conventions below are the contract, pinned against the NumPy
 * statement tests/groups_statement.py, whose per-point degrees are the counts in spheres of the set around itself.
 *   friends  two points i != j are friends under the float32 expressions of abacus_spherecount, bit for bit: d = p_i - p_j per
 *            component, one -+boxsize when |d| > boxsize / 2;
 *            spheres (b_par = 0): r2 = dx dx + dy dy + dz dz left to right, no FMA; friends iff r2 < b_perp * b_perp (a float32
 *            product), strictly;
 *            cylinders (b_par > 0, the line of sight along z): r2 = dx dx + dy dy; friends iff r2 < b_perp * b_perp and
 *            |dz| < b_par, both strictly;
 *            a coincident twin is a friend; a point is not its own friend - by identity, not by distance;
 *   groups   the connected components of the friendship graph;
 *   labels   NULL, or [n] uint32 in the CALLER's order: labels[i] = the smallest caller index among the members of i's group - a
 *            pure function of the input, whatever order the unions ran in; with NULL nothing of size n is copied back;
 *   ngroups  the number of i with labels[i] == i, i.e. the number of groups;
 *   mult     [nmax + 1] uint64: mult[N] = groups with exactly N members for N < nmax, mult[0] = 0, mult[nmax] = those with nmax or
 *            more; the entries sum to ngroups.
 * Checked before the device is touched (every message starts with "abacus_fof: ", from both entries): x, y, z, mult, ngroups not
 * NULL; pos_dtype ABACUS_F32 or ABACUS_F64; boxsize > 0; b_perp > 0; b_par >= 0; b_perp and b_par at most boxsize / 2 (the
 * minimum image is not unique beyond); 0 <= n < 2^31; nmax >= 1 and nmax + 1 <= 8192 (the LDS histogram).
 * Empty cases: n = 0 gives zeros in every output; n = 1 one group of one.
 * _dev: the columns in HBM, of ONE dtype (pos_dtype; float64 is cast to float32 on the device); mult, labels and ngroups are host
 * pointers in both forms.  Coordinates may lie in any interval, as for abacus_paircount_dev.
 * abacus_fof_stats: of the last call, the candidate pairs evaluated, the unordered friend pairs found (exact: every pair is taken
 * once) and the cells per dimension in xy / z.
 */
int abacus_fof(const float *x, const float *y, const float *z, int64_t n, float boxsize, float b_perp, float b_par, int nmax,
               uint64_t *mult, uint32_t *labels, uint64_t *ngroups);
int abacus_fof_dev(const void *x, const void *y, const void *z, int64_t n, int pos_dtype, float boxsize, float b_perp, float b_par,
                   int nmax, uint64_t *mult, uint32_t *labels, uint64_t *ngroups);
int abacus_fof_stats(uint64_t *candidates, uint64_t *links, int *ncell_xy, int *ncell_z);

/*
 * Minimum spanning forest of one catalogue on the periodic box: the edges, the degree of every point and the label of its tree,
 * from which the minimum-spanning-tree statistics (degree, edge length, branch length, branch shape) follow (analysis/mst.py).
 * No reference code stands behind this: the conventions below are the contract, pinned against the NumPy statement
 * tests/mst_statement.py (Kruskal over the sorted edges, and Boruvka by rank).
 *   graph    G(rmax): i != j are joined under the float32 expressions of abacus_spherecount and abacus_fof, bit for bit: d = p_i -
 *            p_j per component, one -+boxsize when |d| > boxsize / 2, r2 = dx dx + dy dy + dz dz left to right, no FMA; an edge iff
 *            r2 < rmax * rmax (a float32 product), strictly; a coincident twin is a neighbour at r2 = 0.  The edge set is that of
 *            abacus_fof with b_perp = rmax and b_par = 0; spheres only.
 *   order    edges compare by the key (r2, lo, hi), lo < hi the caller's indices of the two ends: strict and total, so the
 *            minimum spanning forest is unique although float32 values of r2 tie.  It is the Euclidean minimum spanning tree
 *            with its edges of r2 >= rmax * rmax removed: the Euclidean tree itself whenever ncomp == 1.
 *   edges    edge_i, edge_j (uint32: lo and hi) and edge_r2 (float32), [n] each, the first nedges entries valid and ascending in
 *            the key - the same bytes from every run and from both sort paths; the entries behind are zero;
 *   degree   NULL, or [n] uint32 in the CALLER's order: the number of forest edges at the point;
 *   labels   NULL, or [n] uint32 in the CALLER's order: the smallest caller index in the point's tree - the labels of abacus_fof;
 *   nedges, ncomp   the number of edges and of trees: nedges + ncomp == n.
 * Checked before the device is touched (every message starts with "abacus_mst: ", from both entries): x, y, z, edge_i, edge_j,
 * edge_r2, nedges, ncomp not NULL; pos_dtype ABACUS_F32 or ABACUS_F64; boxsize > 0; 0 < rmax <= boxsize / 2 (the minimum image is
 * not unique beyond); 0 <= n < 2^31.  A refused call writes nothing.
 * Empty cases: n = 0 gives nedges = ncomp = 0; n = 1 no edge and one tree.
 * The device runs Boruvka's rounds, at most 32 of them (the trees with an outgoing edge at least halve per round); a call that
 * would need more returns an error.
 * _dev: the columns in HBM, of ONE dtype (pos_dtype; float64 is cast to float32 on the device); every output is a host pointer in
 * both forms.  Coordinates may lie in any interval, as for abacus_paircount_dev.
 * abacus_mst_stats: of the last call, the candidate pairs evaluated over all rounds, the rounds that emitted edges, the cells per
 * dimension in xy / z and - per_round not NULL - [32][3] uint64: per round the points scanned, those that found an edge out of
 * their tree, and the edges emitted (the round after the last that emitted is listed too: it finds nothing).
 */
int abacus_mst(const float *x, const float *y, const float *z, int64_t n, float boxsize, float rmax, uint32_t *edge_i, uint32_t *edge_j,
               float *edge_r2, uint32_t *degree, uint32_t *labels, uint64_t *nedges, uint64_t *ncomp);
int abacus_mst_dev(const void *x, const void *y, const void *z, int64_t n, int pos_dtype, float boxsize, float rmax, uint32_t *edge_i,
                   uint32_t *edge_j, float *edge_r2, uint32_t *degree, uint32_t *labels, uint64_t *nedges, uint64_t *ncomp);
int abacus_mst_stats(uint64_t *candidates, int *rounds, int *ncell_xy, int *ncell_z, uint64_t *per_round);

/*
 * Galaxy-galaxy lensing on the periodic box: the projected mass sums around galaxies, from which the excess surface density
 * Delta Sigma(R) follows (analysis/lensing.py).  The line of sight is a box axis and the projection runs along the whole box,
 * so both sets are pairs of TRANSVERSE columns.  The particles are sorted once into a 2-D periodic cell grid and stay in HBM
 * behind a handle; every profile call sorts only its galaxies.  No reference code stands behind this: the conventions below are
 * the contract, pinned against the NumPy statement tests/lensing_statement.py, whose cumulative counts are the cylinder counts of
 * abacus_spherecount with pimax = boxsize / 2.
 *   inputs   particles (px, py), n points, float32 masses pm or NULL (unit mass); galaxies (gx, gy), ng points, float32 weights gw
 *            or NULL (unit weight; a weight may be negative); nb + 1 float32 edges 0 < R_0 < ... < R_nb;
 *   pair     per (galaxy, particle), float32, the expressions of abacus_spherecount's cylinders and no dz test: d = g - p per
 *            component, one -+boxsize when |d| > boxsize / 2; r2 = dx dx + dy dy left to right, no FMA; e2[j] = R_j * R_j as a
 *            float32 product;
 *   rows     nb + 1 of them: row 0 is the inner disc r2 < e2[0], row b + 1 is bin b, e2[b] <= r2 < e2[b + 1]; a pair with
 *            r2 >= e2[nb] is dropped;
 *   npairs   [nb + 1] uint64, exact;
 *   wsum     [nb + 1] float64: the sum of (double)gw * (double)pm over the row's pairs (the product of two float32 values is
 *            exact in float64; the order of the additions is not fixed).  With unit weights and masses wsum[r] == npairs[r].
 * abacus_lens_create[_dev] sorts the particles into a grid sized for a reach of rmax (cells of side >= rmax, at least three per
 * dimension or one), keeps the packed (x, y) and the masses in cell order in HBM - 8 bytes per particle, 12 with masses - and
 * remembers sum(pm) in float64 (n without masses): abacus_lens_mass.  One handle serves any number of profile calls, with any
 * edges whose last edge is at most its rmax.  abacus_lens_free releases it (NULL: nothing to do); a freed handle is refused.
 * Checked before the device is touched (the message starts with the entry's name): 1 <= nb <= 32; edges positive and
 * increasing; R_nb <= rmax <= boxsize / 2; boxsize > 0; 0 <= n, ng < 2^31; the handle, the columns of a non-empty set, edges,
 * npairs and wsum not NULL; pos_dtype ABACUS_F32 or ABACUS_F64.
 * Empty sets: n = 0 gives zeros, ng = 0 gives zeros.
 * _dev: the two columns in HBM, of ONE dtype (pos_dtype; float64 is cast to float32 on the device), pm / gw float32 DEVICE
 * pointers; edges, npairs and wsum are host pointers in both forms.  Coordinates may lie in any interval, as for
 * abacus_paircount_dev.
 * abacus_lens_stats: candidate (galaxy, particle) pairs evaluated and the cells per dimension of the last profile call (zeros
 * after a call with an empty set).
 */
typedef struct abacus_lens abacus_lens;
int abacus_lens_create(const float *px, const float *py, const float *pm, int64_t n, float boxsize, float rmax, abacus_lens **handle);
int abacus_lens_create_dev(const void *px, const void *py, const float *pm, int64_t n, int pos_dtype, float boxsize, float rmax,
                           abacus_lens **handle);
int abacus_lens_profile(abacus_lens *handle, const float *gx, const float *gy, const float *gw, int64_t ng, const float *edges, int nb,
                        uint64_t *npairs, double *wsum);
int abacus_lens_profile_dev(abacus_lens *handle, const void *gx, const void *gy, const float *gw, int64_t ng, int pos_dtype,
                            const float *edges, int nb, uint64_t *npairs, double *wsum);
int abacus_lens_mass(abacus_lens *handle, double *mass, int64_t *n);
int abacus_lens_free(abacus_lens *handle);
int abacus_lens_stats(uint64_t *candidates, int *ncell);

/*
 * Three-point correlation function multipoles zeta_l(r1, r2) of one catalogue on the periodic box, by the multipole algorithm of
 * Slepian & Eisenstein (2015): per primary the spherical-harmonic sums of its neighbours per radial bin, then their Gram matrix
 * per l - O(N k) for k neighbours instead of the O(N k^2) triplet count.  No reference code and no Corrfunc run stands behind
 * this: the conventions below are the contract, pinned against the NumPy statement tests/threepcf_statement.py (a brute-force
 * form over triplets, and the algorithm itself in float64 and float32).
 *   catalogue  set 1 (x, y, z, w, n) with set 2 (x2 .. w2, n2) APPENDED by the library (x2 == NULL: set 1 alone), so resident data
 *              and a set of randoms need no concatenation by the caller; weights float32, NULL = 1, and may be negative (D - R);
 *   pair       ordered (i, j), i != j by identity; float32, the expressions of the periodic counters and no others: d = p_i - p_j
 *              per component, one -+boxsize when |d| > boxsize / 2; r2 = dx dx + dy dy + dz dz left to right, no FMA; the pair
 *              is in bin b exactly when abacus_paircount_weighted mode 0 puts it there for the same nbins + 1 float32 edges
 *              (e2[b] <= r2 < e2[b + 1], e2 = edge * edge in float32);
 *   direction  u = d / sqrt(r2) in float32.  A pair with r2 == 0 (a coincident twin) has no direction: it enters neither zeta nor
 *              wself - it IS a pair of its bin in npairs, as in the weighted counter;
 *   zeta       [lmax + 1][nbins][nbins] float64: zeta[l][b1][b2] = sum_i w_i sum_{j in b1(i)} sum_{k in b2(i), k != j} w_j w_k
 *              P_l(u_ij . u_ik).  One triangle is computed and mirrored: zeta[l][b1][b2] and zeta[l][b2][b1] are bit-equal;
 *   wself      [nbins] float64: wself[b] = sum_i w_i sum_{j in b(i)} w_j^2, the j = k term the algorithm removes from the
 *              diagonal (P_l(1) = 1 for every l), returned as a diagnostic;
 *   npairs     [nbins] uint64, bit for bit the npairs of abacus_paircount_weighted mode 0 for the appended catalogue.
 * Precision: directions, harmonics and a primary's harmonic sums a[bin][component] are float32; the Gram products, the factor
 * w_i and everything summed over primaries are float64.  The float32 sums are LDS atomics and the float64 sums over workgroups
 * global atomics: the order of both depends on the run, so zeta and wself are reproducible to the rounding of those sums
 * (tests: within 4 x the float32 statement's own error), not bit for bit; npairs is exact.
 * Checked before the device is touched (the message starts with the entry's name): 1 <= nbins <= 32; 0 <= lmax <= 10; edges
 * non-negative and increasing, the last at most boxsize / 2; boxsize > 0; 0 <= n, n2 and n + n2 < 2^31; y2 and z2 given with x2
 * and only with it, w2 only with x2; x, y, z, bins, zeta, wself, npairs not NULL; pos_dtype ABACUS_F32 or ABACUS_F64.
 * Every output element is written by every successful call; an empty catalogue returns zeros.
 * _dev: the columns of both sets in HBM, of ONE dtype (pos_dtype; float64 is cast to float32 on the device), w / w2 float32
 * DEVICE pointers; bins and the outputs are host pointers in both forms.  Coordinates may lie in any interval.
 * abacus_threepcf_stats: candidate pairs evaluated, counted pairs (the sum of npairs) and cells per dimension of the last call
 * (1: fewer than three cells of the last edge fit, the box is one cell).
 */
int abacus_threepcf(const float *x, const float *y, const float *z, const float *w, int64_t n, const float *x2, const float *y2,
                    const float *z2, const float *w2, int64_t n2, float boxsize, const float *bins, int nbins, int lmax,
                    double *zeta, double *wself, uint64_t *npairs);
int abacus_threepcf_dev(const void *x, const void *y, const void *z, const float *w, int64_t n, const void *x2, const void *y2,
                        const void *z2, const float *w2, int64_t n2, int pos_dtype, float boxsize, const float *bins, int nbins,
                        int lmax, double *zeta, double *wself, uint64_t *npairs);
int abacus_threepcf_stats(uint64_t *candidates, uint64_t *counted, int *ncell);

/* ---------------------------------------------------------------- staging (the step in front of the HOD) ---- */
/*
 * Data-parallel pieces of AbacusHOD.staging() (hod/abacus_hod.py:253-704); host arrays in and out, staging runs once.
 * abacus_argsort_i64: stable ascending argsort (replaces `np.argsort(hid)` of the halo sort, :566-585).
 * abacus_searchsorted_i64: np.searchsorted(sorted, query, side='left') (replaces `_searchsorted_parallel`, :588).
 * abacus_fenv_rank: `calc_fenv_opt` (:1961-1970): out[i] = rank of Menv[i] among the halos with
 *   mbins[b] < halosM < mbins[b+1] of i's bin, / (N_bin - 1) - 0.5; 0 for halos in no bin or alone in theirs.
 */
int abacus_argsort_i64(const int64_t *keys, int64_t n, int64_t *order);
int abacus_searchsorted_i64(const int64_t *sorted, int64_t n, const int64_t *query, int64_t m, int64_t *out);
int abacus_fenv_rank(const double *Menv, const double *halosM, int64_t n, const double *mbins, int n_edges, double *out);

/* ---------------------------------------------------------------- prepare_sim (subsample preparation) ---- */
/*
 * replaces the data-parallel core of abacusnbody/hod/prepare_sim.py `prepare_slab` (:296-1052); host arrays in and out
 * (runs once per slab).  Host side and file layout: abacusutils_amd/hod/prepare_sim.py.
 *
 * abacus_prepare_halo_factors: p_halos[i] = subsample_halos(N[i] * Mpart, MT) (:83-108); mask[i] = u[i] < p_halos[i] (:449)
 *   when `mask` / `u` are given; ntarget[i] = the number of subsample particles submask_particles keeps for a halo of that
 *   mass with pnum[i] particles (:152-174) when `ntarget` / `pnum` are given.
 * abacus_prepare_particles: for every kept halo (hmask) with pnum > 0, keep a subset of its particle slice
 *   [pstart, pstart + pnum) - either the caller's `submask_in` (npart bytes, drawn on the host in the reference's order) or,
 *   with submask_in == NULL, a uniformly random subset of ntarget[j] particles from counter-based Philox keys (seed, particle
 *   index part_index0 + q).  Outputs: pstart_new / pnum_new per halo as the reference stores them (float64; -1 for dropped
 *   halos and halos without particles, :895-897, :979-981); *n_sel kept particles; if cap_sel >= *n_sel also their input index
 *   (ascending), host halo index, Np (:881) and, with want_ranks, the five rank columns ranks / ranksv / ranksp / ranksr /
 *   ranksc (:899-977).  The number of kept particles is known beforehand - the set bytes of `submask_in`, or the sum of
 *   ntarget over the kept halos - so one call with cap_sel of that size does it all; a call with cap_sel = 0 only sizes the
 *   outputs (pass its `submask_out` as `submask_in` of the second call, so that both see one draw).  Halo slices must be
 *   ordered like the halos (CompaSO's layout).
 */
int abacus_prepare_halo_factors(const uint32_t *N, int64_t n, double Mpart, int MT, const double *u, const int64_t *pnum,
                                double *p_halos, uint8_t *mask, int32_t *ntarget);
/* the reference's two-argument form, subsample_halos(m, MT) on float64 MASSES (hod/prepare_sim.py:83-108) */
int abacus_prepare_halo_factors_mass(const double *mass, int64_t n, int MT, double *p_halos);
int abacus_prepare_particles(int64_t nh, const uint8_t *hmask, const int64_t *pstart, const int64_t *pnum, const uint32_t *N,
                             const float *hpos, const float *hvel, const float *r25, const float *r98, int64_t npart,
                             const float *pos, const float *vel, const uint8_t *submask_in, const int32_t *ntarget, uint64_t seed,
                             int64_t part_index0, double Mpart, double h, int want_ranks, double *pstart_new, double *pnum_new,
                             int64_t *n_sel, int64_t cap_sel, int64_t *sel_idx, int64_t *sel_host, double *sel_np, double *ranks,
                             double *ranksv, double *ranksp, double *ranksr, double *ranksc, uint8_t *submask_out);

/*
 * The same slab prepared WITHOUT a column crossing PCIe twice (what hod/prepare_sim.py:296-1052 does between its loader and its
 * writer, `rng = <seed>` form): abacus_prepare_slab takes the CompaSO columns prepare_slab loads (:404-425; host pointers are
 * uploaded once, device pointers - what the reader's unpack kernels produce - are used in place), draws the halo mask, selects the
 * particles, ranks them and gathers the kept rows of every column of both tables in HBM; abacus_prepare_slab_fetch copies the
 * columns out, one copy each.  mbins / n_edges: the mass bins of the concentration rank (n_edges = 0: deltac_rank = 0, the
 * reference's want_AB = False); fenv_rank / shear_rank: per-halo columns the caller computed (light cones, shear) or NULL = 0.
 * mask_out (nh bytes, host, may be NULL): the halo mask.  Streams and values are those of abacus_prepare_halo_factors /
 * _particles / _randoms with the same seed: both paths give identical tables.
 */
typedef struct abacus_prepare_slab_args {
    int64_t nh, npart;
    const uint32_t *N;                           /* (nh) */
    const float *x, *v;                          /* (nh, 3) x_L2com, v_L2com */
    const float *r25, *r90, *r98, *sigmav;       /* (nh) */
    const int64_t *npstartA, *npoutA;            /* (nh) */
    const void *id;                              /* (nh) 8-byte ids */
    const float *pos, *vel;                      /* (npart, 3) subsample-A particles in halo order */
    const double *fenv_rank, *shear_rank;        /* (nh) or NULL */
    const double *mbins;                         /* (n_edges) host */
    int32_t n_edges, MT, want_ranks, pad_;
    double Mpart, h;
    uint64_t seed;
    int64_t halo_index0, part_index0;
} abacus_prepare_slab_args;
enum {  /* columns of the halo table, in the order of halo_cols[] */
    ABACUS_PREP_H_N = 0, ABACUS_PREP_H_X, ABACUS_PREP_H_V, ABACUS_PREP_H_R25, ABACUS_PREP_H_R90, ABACUS_PREP_H_R98, ABACUS_PREP_H_NPSTART,
    ABACUS_PREP_H_NPOUT, ABACUS_PREP_H_ID, ABACUS_PREP_H_SIGMAV, ABACUS_PREP_H_MASK, ABACUS_PREP_H_MULTI, ABACUS_PREP_H_FENV, ABACUS_PREP_H_DELTAC,
    ABACUS_PREP_H_SHEAR, ABACUS_PREP_H_RANDOMS, ABACUS_PREP_H_REXP, ABACUS_PREP_H_RGAUS, ABACUS_PREP_HALO_COLS
};
enum {  /* columns of the particle table, in the order of part_cols[]; RANKS .. RANKS + 4 = ranks, ranksv, ranksp, ranksr, ranksc */
    ABACUS_PREP_P_POS = 0, ABACUS_PREP_P_VEL, ABACUS_PREP_P_RANKS, ABACUS_PREP_P_DOWNSAMPLE = ABACUS_PREP_P_RANKS + 5, ABACUS_PREP_P_HALO_VEL,
    ABACUS_PREP_P_HALO_MASS, ABACUS_PREP_P_NP, ABACUS_PREP_P_HALO_ID, ABACUS_PREP_P_RANDOMS, ABACUS_PREP_P_DELTAC, ABACUS_PREP_P_FENV,
    ABACUS_PREP_P_SHEAR, ABACUS_PREP_PART_COLS
};
int abacus_prepare_slab(const abacus_prepare_slab_args *args, int64_t *n_halo_kept, int64_t *n_part_kept, uint8_t *mask_out);
int abacus_prepare_slab_fetch(void *const *halo_cols, void *const *part_cols);

/* the random columns of the prepare_sim tables drawn on the device (Philox4x32-10, counter = global object index: shard
 * invariant; NOT the reference's NumPy stream - prepare_sim.py:984-996,1029 - but its distributions and dtypes).  Row r stands
 * for the object index0 + (index ? index[r] : r).  stream_id 4, with scale / randoms_exp / randoms_gaus: the halo columns
 * `randoms` (n) U[0,1), `randoms_exp` (n,3) = +-Exp(1) * scale[r], `randoms_gaus_vrms` (n,3) = N(0,1) * scale[r]; stream_id
 * 5 .. 255 without them: one U[0,1) per object (5: the particles' `randoms`, 6: the draws of the halo mask).  Host pointers. */
int abacus_prepare_randoms(int64_t n, const int64_t *index, int64_t index0, uint64_t seed, int stream_id, const double *scale,
                            double *randoms, double *randoms_exp, double *randoms_gaus);

/* ---------------------------------------------------------------- catalogue side (upstream of the HOD) ---- */
/*
 * replaces: abacusnbody/data/bitpacked.py:32-116 `unpack_rvint` / `_unpack_rvint`.  intdata: (n,3) int32, 20-bit
 * position | 12-bit velocity per word.  pos = (x >> 12) * (boxsize / 1e6), vel = ((x & 0xFFF) - 2048) * 6000 / 2048,
 * formed in float64 and rounded once into float32 (out_f64 = 0) or kept float64 (out_f64 = 1).  posout / velout:
 * (n,3) or NULL (skip, the reference's `False`).  Every pointer of this block may be host or device memory.
 */
int abacus_unpack_rvint(const int32_t *intdata, int64_t n, double boxsize, int out_f64, void *posout, void *velout);
/*
 * replaces: abacusnbody/data/bitpacked.py:118-330 `unpack_pids` / `_unpack_pids`.  packed: (n) uint64 aux words.
 * Outputs (each may be NULL): pid (n) int64 = packed & 0x7FFF7FFF7FFF; lagr_idx (n,3) int16; lagr_pos (n,3) =
 * idx * float_dtype(box / ppd) - float_dtype(box / 2); tagged (n) uint8 = bit 48; density (n) = (bits 49..58)^2.
 */
int abacus_unpack_pids(const uint64_t *packed, int64_t n, double box, int64_t ppd, int out_f64, int64_t *pid,
                       void *lagr_pos, int16_t *lagr_idx, uint8_t *tagged, void *density);
/*
 * replaces: abacusnbody/data/pack9.py:16-123 `unpack_pack9` / `_unpack_pack9`.  data: (nrec, 9) bytes; a record whose
 * first byte is 0xFF is a cell header for the particles after it.  posout / velout: (nrec, 3) or NULL; the first
 * *npart rows are written (records before the first header decode to NaN, like the reference's initial state).
 */
int abacus_unpack_pack9(const uint8_t *data, int64_t nrec, double boxsize, double velzspace_to_kms, int out_f64,
                        void *posout, void *velout, int64_t *npart);
/*
 * replaces: abacusnbody/hod/menv.py:19-87 `do_Menv_from_tree` (scipy KDTree ball queries + gather sums; callers
 * hod/prepare_sim.py:603-612,728-737).  Menv[i] = sum of mass within r_outer of halo i minus the sum within r_inner,
 * over ALL halos (itself included in both), for halos with mass > mcut; 0 for the others.  pos: (n,3) in [-Lbox/2,
 * Lbox/2) or wherever the caller has them: when periodic the kernels apply menv.py:39 `(pos + Lbox/2) % Lbox` in the
 * dtype of pos (NumPy remainder), so the distances are formed from the values the reference's tree sees.
 * r_inner / r_outer: n_inner / n_outer = 1 (scalar) or n values of precision r_f64; r_outer_max = their maximum (sets the
 * cell size).  periodic = 0: open geometry (`halo_lc`), lo / hi = bounding box of pos.  Menv: (n) float64.
 */
int abacus_menv(const void *pos, int pos_f64, const void *mass, int mass_f64, int64_t n, const void *r_inner,
                int64_t n_inner, const void *r_outer, int64_t n_outer, int r_f64, double r_outer_max, double Lbox,
                int periodic, const double *lo, const double *hi, double mcut, double *Menv);

/* ---------------------------------------------------------------- tidal shear field --------------------- */
/*
 * The chain particles -> density -> Gaussian smoothing -> tidal tensor -> shear on DEVICE pointers (csrc/shear.hip); every call
 * enqueues on the library stream.  Meshes are C-contiguous (n, n, n) float32.
 */
/* replaces: smooth_density (analysis/shear.py:15-21) = scipy.ndimage.gaussian_filter with its defaults: three separable passes
 * along axes 0, 1, 2, float64 sums rounded to float32 after each pass, boundary mode 'reflect' (not periodic).  weights: HOST array of
 * radius + 1 float64 values, weights[k] = the normalised kernel at distance k from the centre.  In place on `mesh`; tmp: n^3 floats. */
int abacus_gauss_smooth_dev(float *mesh, float *tmp, int n, const double *weights, int radius);
/* replaces: get_shear (analysis/shear.py:96-131) = rfftn + get_tidal (:38-66) + six irfftn + get_shear_nb (:69-93).  dens is
 * not modified; out (n^3 floats) overlaps nothing.  R_or_negative >= 0: the top-hat window Wth (:24-29) of that radius; < 0: R = None.
 * n even (the reference fails on odd sizes).  The modes with a zero index on any axis are dropped and the Nyquist plane of the last
 * axis carries fftfreq's negative wavenumber, as in the reference.  Two padded work meshes come from the scratch pool; the call
 * fails up front, naming the largest mesh that fits, when they do not fit the free device memory. */
int abacus_shear_dev(float *dens, float *out, int n, double Lbox, double R_or_negative);
/* replaces: the compute part of calc_shearmark (hod/prepare_sim.py:1113-1123): tsc_parallel(pos, n, Lbox) raw counts (positions
 * wrapped into the box on a copy), smooth_density with sigma_cells = R / (Lbox / n) (<= 0: none), get_shear with R = None.
 * pos: (np, 3) float32; out: n^3 floats, also used as a work mesh. */
int abacus_shearmark_dev(const float *pos, int64_t np, int n, double Lbox, double sigma_cells, float *out);
/* replaces: get_tidal (analysis/shear.py:38-66) as it returns: dfour (n, n, n/2+1) complex64, karr (n) float32 wavenumbers,
 * out (n, n, n/2+1, 6) complex64 = the six FULL components k_i k_j / k^2 dfour in the order xx xy xz yy yz zz */
int abacus_tidal_dev(const void *dfour_c64, const float *karr, int n, double R_or_negative, void *out_c64);
/* replaces: the fancy-indexed look-up shearmark[g[:, 0], g[:, 1], g[:, 2]] (hod/prepare_sim.py:786-791) in a field that stays on
 * the device: g (nh, 3) int64 cell indices, out (nh) float32; an index outside [0, n) gives NaN */
int abacus_mesh_gather_dev(const float *mesh, int n, const int64_t *g, int64_t nh, float *out);

/* ---------------------------------------------------------------- Zel'dovich control variates ----------- */
/*
 * The heavy half of abacusnbody/hod/zcv on DEVICE pointers (csrc/zcv.hip); every call enqueues on the library stream.  Meshes are
 * C-contiguous (n, n, n) float32, caller spectra C-contiguous (n, n, n/2+1) complex64 (un-normalised rfftn output); "padded"
 * spectra are n * n rows of abacus_slab_pitch(n) / 2 complex (abacus_zcv_spectrum_bytes bytes).  n is even where an inverse
 * transform is involved (the reference fails on odd sizes).  Wavenumbers as the reference forms them: dk = float32(2 pi / Lbox),
 * index i -> i below n/2, i - n from n/2 on (x, y), 0 .. n/2 on z.
 */
/* replaces: gaussian_filter (hod/zcv/ic_fields.py:79-107) = rfftn, filter_field, irfftn.  field is not modified; out may be field. */
int abacus_zcv_filter_dev(const float *field, float *out, int n, double Lbox, double kcut);
/* replaces: filter_field (:110-148; op 0, exp(-k^2 / (2 kcut^2)), dst may be src), get_n2_fft (:151-189; op 1, -k^2) and
 * get_sij_fft (:192-255; op 2, k_i k_j / k^2 - delta_ij / 3 for component (ci, cj), the zero vector -> -delta_ij / 3) */
int abacus_zcv_spectral_dev(const void *src_c64, void *dst_c64, int n, double Lbox, int op, int ci, int cj, double kcut);
/* replaces: add_ij (:258-268): final_field += float32(factor) * field_to_add^2 */
int abacus_zcv_add_ij_dev(float *final_field, const float *field_to_add, int n, double factor);
/* replaces: get_dk_to_s2 (:271-309; which = 0) and get_dk_to_n2 (:312-333; which = 1) on a caller spectrum.  The s_ij spectra
 * are not Hermitian on the planes c = 0 and c = n/2 (negative Nyquist wavenumber on x and y, positive on z); the reference's irfftn
 * uses the Hermitian part of those planes, which is written out here before the C2R. */
int abacus_zcv_dk_to_dev(const void *delta_k_c64, int n, double Lbox, int which, float *out);
/* replaces: get_fields (:336-366) in one call: d = delta - mean, d2 = delta^2 - mean, s2 = s_ij s_ij - mean, n2 = nabla^2 delta;
 * one R2C, seven multiplier + C2R rounds; the means are deterministic two-stage float64 sums.  Two padded work meshes come from the
 * scratch pool; the call fails up front, naming the largest mesh that fits, when they do not fit the free device memory.
 * delta is not modified; d may be delta. */
int abacus_zcv_fields_dev(const float *delta, int n, double Lbox, float *d, float *d2, float *s2, float *n2);
/* replaces: hod/zcv/advect_fields.py main :213-239: pos (n^3, 3) = ((disp * f32(D) [z: * f32(1 + f_growth)]) + f32(index) / f32(n))
 * * f32(Lbox) % f32(Lbox), every operation a correctly rounded float32 operation, the remainder NumPy's */
int abacus_zcv_lattice_dev(const float *disp_x, const float *disp_y, const float *disp_z, int n, double Lbox, double D, double f_growth,
                           float *pos);
/* replaces: tracer_power.py:157-158 on (np, 3) float32 device positions: pos += f32(Lbox / 2); pos %= f32(Lbox), in place */
int abacus_zcv_shift_wrap_dev(float *pos, int64_t np, double Lbox);
/* bytes of one padded spectrum of an n^3 mesh */
int abacus_zcv_spectrum_bytes(int n, uint64_t *bytes);
/* fails, naming the largest mesh that fits, when `nfield` padded spectra + the work meshes of one deposit + transform + the
 * particles (np, or the n^3 lattice when np = 0) do not fit the free device memory */
int abacus_zcv_check_memory(int n, int nfield, int interlaced, int64_t np);
/* replaces: get_field_fft (analysis/power_spectrum.py:1001-1070) for DEVICE particles: the finished spectrum (interlacing
 * combined, compensated when W_host != NULL) into the caller's padded spectrum.  TSC wraps pos in place.  w: np floats or NULL. */
int abacus_zcv_spectrum_dev(float *pos, int64_t np, const float *w, double Lbox, int n, int paste, const float *W_host, int interlaced,
                            void *out_padded);
/* replaces: advect_fields.py main :213-285: the lattice positions (never on the host) deposited once per field with the mesh
 * weights[f] (device, n^3 floats used where they lie; NULL: unweighted), transformed and finished into out_padded[f].
 * weights / out_padded: HOST arrays of nfield device pointers. */
int abacus_zcv_advect_dev(const float *disp_x, const float *disp_y, const float *disp_z, int n, double Lbox, double D, double f_growth,
                          int nfield, const float *const *weights, int paste, const float *W_host, int interlaced, void *const *out_padded);
/* replaces: calc_pk_from_deltak (analysis/power_spectrum.py:730-805) on two padded spectra in HBM (b_padded NULL: auto power);
 * outputs as abacus_pk_from_deltak returns them */
int abacus_zcv_power_pair(const void *a_padded, const void *b_padded, int n, double Lbox, const double *kedges, int Nk, const double *muedges,
                          int Nmu, const int64_t *poles, int Np, float *power, int64_t *N_mode, float *binned_poles, int64_t *N_mode_poles,
                          float *k_avg);
/* a padded device spectrum as the (n, n, n/2+1) complex64 host array get_field_fft returns */
int abacus_zcv_spectrum_fetch(const void *padded, int n, void *out_c64_host);
/* releases the cached hipFFT plans of this section (abacus_scratch_release does so too) */
int abacus_zcv_release(void);

/* ---------------------------------------------------------------- linear control variates --------------- */
/*
 * The linear half (LCV) of abacusnbody/hod/zcv, the one reconstructed catalogues use, on DEVICE pointers (csrc/lcv.hip, beside
 * the section above whose transform, deposit and binning it shares); every call enqueues on the library stream.  Spectra are
 * padded (n * n rows of abacus_slab_pitch(n) / 2 complex, abacus_zcv_spectrum_bytes bytes) and normalised as get_field_fft
 * normalises (divided by n^3), so abacus_zcv_power_pair bins any pair of them and abacus_zcv_spectrum_fetch copies one out.
 * Mode numbers and mu^2 as get_delta_mu2 forms them: float32, index i -> i below n/2, i - n from n/2 on (x, y), 0 .. n/2 on z;
 * the zero vector has mu^2 = 0.  Calls that need device memory beyond their arguments fail up front, naming the largest mesh
 * that fits.
 */
/* replaces: linear_fields.py:108-124 (and tracer_power.py:440-456): delta (n, n, n) float32, not modified -> padded copy, R2C in
 * place, ONE pass that writes rfftn(delta) / f32(n^3) and that times mu^2 (get_delta_mu2 fused with the normalisation).  n even. */
int abacus_lcv_linear_dev(const float *delta, int n, void *out_delta_padded, void *out_deltamu2_padded);
/* replaces: tr_field_fft -= rn_field_fft (tracer_power.py:410-414): a -= b over two padded spectra */
int abacus_lcv_spectrum_sub_dev(void *a_padded, const void *b_padded, int n);
/* replaces: the P_k3D_* products of save_3D_power (linear_fields.py:138-141, tracer_power.py:464, :501-503): Re(a conj b), or
 * |a|^2 when b_padded is NULL, unpadded on the device and copied out once as the float32 (n, n, n/2+1) HOST array */
int abacus_lcv_power3d(const void *a_padded, const void *b_padded, int n, float *out_host);
/* replaces: combine_field_spectra_k3D_lcv (tools_cv.py:313-335) and the six materialised 3-D products it reads: one pass over
 * the three padded spectra writes pk_ll = D^2 (2 b f_eff P_md + f_eff^2 P_mm + b^2 P_dd), pk_lt = D (b P_dt + f_eff P_mt) and
 * pk_tt = |tr|^2 in NumPy's float32 order of evaluation; float32 (n, n, n/2+1) HOST arrays.  reciso = 0: f_eff = f_growth;
 * reciso = 1: f_eff = f_growth (1 - exp(-k^2 R^2 / 2)) per mode with get_smoothing's float32 wavenumbers, on the (n, n, n/2+1)
 * grid (the reference reshapes that kernel to (n, n, n) and raises: this branch has no reference output). */
int abacus_lcv_combine_k3d(const void *delta_padded, const void *deltamu2_padded, const void *tr_padded, int n, double Lbox, double bias,
                           double f_growth, double D, double R, int reciso, float *pk_tt, float *pk_ll, float *pk_lt);

/* ---------------------------------------------------------------- BAO reconstruction --------------------- */
/*
 * Standard plane-parallel reconstruction of a periodic box (line of sight = z) on DEVICE pointers (csrc/recon.hip, beside the LCV
 * section whose inputs it produces); every call enqueues on the library stream.  replaces: nothing in the reference - its
 * get_recon_power takes reconstructed tracers and shifted randoms that an external CPU code made between run_hod and get_recon_power;
 * this is that step.  Conventions of Chen et al. 2019 (RecSym, RecIso), the ones tools_cv.combine_kaiser_spectra assumes:
 *   psi_i(k) = i k_i S(k) delta(k) / (k^2 b (1 + beta mu^2)),  S = exp(-k^2 R^2 / 2),  beta = f / b (rsd) or 0,  mu^2 = k_z^2 / k^2,
 * 0 for the zero vector; float32 arithmetic, wavenumbers as above (dk = float32(2 pi / Lbox), i -> i below n/2, i - n from n/2 on for
 * x and y, 0 .. n/2 on z).  In the factor i k_i ONLY the wavenumber of axis i is 0 at index n/2 of that axis (k^2, mu^2 and S keep
 * it), which makes the three spectra Hermitian as written.  "Padded meshes" are the real side of the padded spectra above: n * n
 * rows of abacus_slab_pitch(n) floats, the first n of a row used.  n even, 2 .. 32767.
 */
/* fails, naming the largest mesh that fits, when the three displacement meshes + the work mesh of one deposit + transform + the
 * copies of np particles do not fit the free device memory */
int abacus_recon_check_memory(int n, int64_t np);
/* three float64 device columns (what MockDict.device_xyz returns) -> out (np, 3) float32 = f32(column + f64(f32(offset))): for
 * float32-valued columns the same bits as the float32 sum */
int abacus_recon_pack_soa64_dev(const double *x, const double *y, const double *z, int64_t np, double offset, float *out);
/* out (np, 3) float32 = (pos + f32(offset)) % f32(Lbox), NumPy's float32 remainder: the copy a deposit may work on.  out may be pos. */
int abacus_recon_wrap_dev(const float *pos, int64_t np, double offset, double Lbox, float *out);
/* mesh (n, n, n) float32 -> padded mesh (the layout abacus_recon_shift_dev reads) */
int abacus_recon_pad_dev(const float *mesh, int n, float *out_padded);
/* a given density mesh delta (n, n, n) float32, not modified -> padded copy, R2C in place: the BARE spectrum (not divided by n^3;
 * pass normalised = 0 below, which folds 1 / n^3 into the multiplier).  The transform may take one padded work mesh from the scratch pool. */
int abacus_recon_delta_dev(const float *delta, int n, void *out_padded);
/* delta_padded (a padded spectrum; normalised = 1: divided by n^3 as abacus_zcv_spectrum_dev leaves it, 0: a bare R2C) -> ONE pass
 * that writes the three displacement spectra (8 B read, 24 B written per mode) -> three in-place C2R: psi_x, psi_y, psi_z are
 * padded meshes of abacus_zcv_spectrum_bytes(n) bytes each, in the units of Lbox.  delta_padded may be psi_z (and nothing else):
 * three meshes then hold everything.  bias > 0, f_growth >= 0, R >= 0 (0: no smoothing), all finite.  hipFFT may take a work area. */
int abacus_recon_displacement_dev(const void *delta_padded, int normalised, int n, double Lbox, double bias, double f_growth, double R, int rsd,
                                  float *psi_x, float *psi_y, float *psi_z);
/* one lane per particle: s = (pos + f32(offset)) % f32(Lbox); psi read at s from the three padded meshes with the cloud of `paste`
 * (0: the 27 cells of analysis/tsc.py _tsc_scatter, 1: the 8 cells of analysis/cic.py; cell i centred at i Lbox / n, nearest cell by
 * rounding, periodic indices); out (np, 3) float32 = (s - psi - f32(los_factor) psi_z z^) % f32(Lbox), the z component as
 * ((s_z - psi_z) - los psi_z).  los_factor: f_growth for tracers and RecSym randoms under rsd, 0 for RecIso randoms.  pos is not
 * modified; out must not be pos.  No scratch memory. */
int abacus_recon_shift_dev(const float *pos, int64_t np, double offset, const float *psi_x, const float *psi_y, const float *psi_z, int n,
                           double Lbox, int paste, double los_factor, float *out);

/* ---------------------------------------------------------------- light-cone power spectrum --------------- */
/*
 * FKP field and Yamamoto multipoles of a light-cone catalogue on DEVICE pointers (csrc/lc_power.hip, behind the recon section; Python:
 * analysis/lc_power.py); every call enqueues on the library stream.  replaces: nothing in the reference, whose power spectra assume a
 * periodic box and a global line of sight.  Estimator: Feldman, Kaiser & Peacock 1994 with the end-point line of sight of Yamamoto
 * et al. 2006, through the spherical-harmonic decomposition of Hand et al. 2017 (1 + 5 + 9 transforms for l = 0, 2, 4).
 *   F = D - alpha R: the raw weighted deposits (weight per cell, no normalisation) of data and randoms, columns centred on the
 *   observer, in a box of side Lbox with its corner at `corner`; cell i is centred at corner + i Lbox / n.
 *   F_0(k) = R2C(F) (a bare sum over cells);  F_l(k) = sum_m S_lm(k^) R2C[S_lm(r^_cell) F](k),  l = 2, 4,
 * with S_lm the real harmonics scaled so that sum_m S_lm(a) S_lm(b) = L_l(a . b): polynomials in the unit vector, float32, listed in
 * tests/lc_power_statement.py.  S_lm = 0 for l > 0 in the cell with |r| = 0 and at k = 0.  k^ is formed from the mode numbers (index i
 * -> i below n/2, i - n from n/2 on for x and y, 0 .. n/2 on z).  No inverse transform follows: the Nyquist planes are left as
 * computed.  "Padded meshes" as in the recon section: n * n rows of abacus_slab_pitch(n) floats, abacus_zcv_spectrum_bytes(n) bytes;
 * a padded spectrum is the same memory after the in-place R2C.  n even, 2 .. 32767.  The spectra are binned by abacus_zcv_power_pair.
 */
/* fails, naming the largest mesh that fits, when `nmeshes` more padded meshes (F, F_0, the requested F_l, one work mesh, the randoms'
 * mesh where it is not cached yet) + the packed copies, weights and deposit lists of np points do not fit the free device memory */
int abacus_lc_check_memory(int n, int nmeshes, int64_t np);
/* lohi_host[0..2] = the minima of the three float32 device columns, [3..5] the maxima: a two-stage reduction without atomics.  An
 * axis with a coordinate that is not finite reports (-inf, +inf). */
int abacus_lc_extent_dev(const float *x, const float *y, const float *z, int64_t np, float *lohi_host);
/* three float32 device columns -> out (np, 3) float32 = column - f32(corner[axis]), one float32 subtraction: the copy a deposit works on */
int abacus_lc_pack_dev(const float *x, const float *y, const float *z, int64_t np, const double *corner, float *out);
/* mesh_padded = the raw deposit of the np points pos (np, 3) float32 in [0, Lbox) with the weights w (float32, NULL: unit weights) and
 * the cloud of `paste` (0: TSC, 1: CIC), every cell written (no separate zeroing), tile sums in float64.  The deposit is periodic:
 * the caller keeps the points two cells away from the faces.  pos may be sorted in place. */
int abacus_lc_deposit_dev(float *pos, int64_t np, const float *w, double Lbox, int n, int paste, float *mesh_padded);
/* dst_padded += f32(a) src_padded over whole padded meshes (F = D + (-alpha) R: one deposit and this): 8 B read, 4 B written per cell */
int abacus_lc_axpy_dev(float *dst_padded, const float *src_padded, int n, double a);
/* F_padded (not modified) -> out_padded = F_l(k), l = ell in {0, 2, 4}.  ell = 0: a copy and one R2C.  ell > 0, for each of the 2 ell + 1
 * m: lc_ylm_mult (work = S_lm(r^_cell) F, one (i, j) row per wave, 4 B read + 4 B written per cell), R2C of the work mesh in place,
 * lc_ylm_accum (out (+)= S_lm(k^) work, the first m writes: 8 B read + 8 B written per mode, 8 B more read from the second m on).
 * corner[3]: the box corner relative to the observer, used as float32.  work_padded: a padded mesh (unused for ell = 0).  The three
 * buffers must differ.  The transform may take one padded work mesh from the scratch pool or a hipFFT work area. */
int abacus_lc_multipole_dev(const float *F_padded, int n, double Lbox, const double *corner, int ell, float *work_padded, void *out_padded);
/* spec_padded *= 1 / ((W[a] W[b]) W[c]) in float32, W_host the n float32 values of get_W_compensated: the compensation of the cloud */
int abacus_lc_compensate_dev(void *spec_padded, int n, const float *W_host);
/* out_host[0] = sum_i w_i^2 nbar_i in float64 (w float32 device weights, NULL: unit weights; nbar a device column, float64 if nbar_f64
 * else float32): per-workgroup partial sums, then one workgroup over them, both in a fixed order - the same bits on every run */
int abacus_lc_sum_w2n_dev(const float *w, const void *nbar, int nbar_f64, int64_t np, double *out_host);

/* ---------------------------------------------------------------- bispectrum ------------------------------ */
/*
 * Bispectrum of a periodic box on DEVICE pointers (csrc/bispectrum.hip, behind the light-cone section; Python: analysis/bispectrum.py); every
 * call enqueues on the library stream.  replaces: nothing in the reference, which has no three-point statistic.  Estimator: the FFT
 * form of Scoccimarro 2015.  From a padded spectrum delta(k), normalised as get_field_fft normalises (abacus_zcv_spectrum_dev), and
 * nb shells with the edges kedges[0 .. nb]:
 *   dk = float32(2 pi / Lbox); mode numbers: index i -> i below n/2, i - n from n/2 on (x, y), 0 .. n/2 on z;
 *   |k| = dk * sqrt(float32(ix^2 + iy^2 + iz^2)), the square root and the product correctly rounded float32 operations;
 *   a mode belongs to shell b iff float32(kedges[b]) <= |k| < float32(kedges[b + 1]), compared in float32;
 *   D_b(x) = sum_{k in shell b} delta(k) e^{ikx} (no normalisation of the inverse), I_b(x) the same with delta -> 1;
 *   T[i][j][l] = sum_x D_i D_j D_l and G[i] = sum_x D_i^2 over the n^3 cells (the caller divides by n^3).
 * The sums close triangles modulo n, so float32(kedges[nb]) <= dk n / 3 is required (with a slack of 2^-22 for the float32 roundings of
 * dk and the edge, and with what the rule stands for checked exactly: the mode (ceil(n / 3), 0, 0) is in no shell): every component of
 * every mode used is then below n / 3, the Nyquist planes are in no shell and every masked spectrum is Hermitian as written.  "Padded meshes" as in the recon
 * section: n * n rows of abacus_slab_pitch(n) floats, abacus_zcv_spectrum_bytes(n) bytes, aligned to 16 bytes.  Limits, checked
 * before the device is touched, every message starting with the entry's name: n even, 2 .. 32767; 1 <= nb <= 32; edges finite,
 * positive and increasing in float32; no null argument.
 */
/* fails, naming the largest mesh that fits, when the nb shell meshes + the spectrum + the work area of one deposit and transform (two
 * padded meshes) + the copies and deposit lists of np particles do not fit the free device memory */
int abacus_bk_check_memory(int n, int nb, int64_t np);
/* spec_padded (not modified; NULL: the I fields) -> bk_shell_mask: ONE pass in which every mode is read once and written to all nb
 * meshes, the mode inside its shell's mesh and 0 in the others (8 + 8 nb bytes per mode; the floats of a row beyond its n/2 + 1 modes
 * are not written) -> nb in-place C2R.  meshes: a HOST array of nb device pointers to padded meshes, all different and none the
 * spectrum; each holds D_b (or I_b) in its first n floats per row afterwards.  hipFFT may take a work area. */
int abacus_bk_shells_dev(const void *spec_padded, int n, double Lbox, const double *kedges, int nb, float *const *meshes);
/* T_host[nb][nb][nb] and G_host[nb] in float64 from nb padded real meshes (a HOST array of device pointers; not modified; the pad
 * columns of a row never enter).  bk_triple: the sums as a GEMM S[(i, j)][l] = sum_x (D_i D_j)(x) D_l(x) on v_mfma_f32_16x16x4_f32 -
 * the products D_i D_j and the accumulation in float32 for 128 cells (K of the MFMA chain), then added to float64 sums; one
 * float64 partial per workgroup, added by a second kernel in a fixed order: no atomics, the same bits on every run.  nb <= 16: the full
 * (i, j, l) cube in 16 tiles of 16 x 16.  nb > 16: the four block triples in ascending order, the other entries are their mirror
 * images under a permutation of (i, j, l). */
int abacus_bk_triple_dev(const float *const *meshes, int n, int nb, double *T_host, double *G_host);

/* ---------------------------------------------------------------- Minkowski functionals ------------------- */
/*
 * Minkowski functionals of a periodic mesh on DEVICE pointers (csrc/minkowski.hip; Python: analysis/minkowski.py); every call enqueues
 * on the library stream.  replaces: nothing in the reference, which has no morphological statistic.  Estimator: Crofton's formula on
 * the cubic lattice (Schmalzing & Buchert 1997).  For a mesh of n^3 float32 cells with periodic indices and a threshold t:
 *   the excursion set is the union of the closed voxels with value >= t, compared in float32 (a tie is inside);
 *   an element of the lattice belongs to it iff the maximum of the voxels that touch it is >= t: 2 voxels for a face, 4 for an edge,
 *   8 for a vertex; voxel (i, j, k) owns its cube, the faces towards +x, +y, +z, the three edges between those faces and the vertex
 *   at (i + 1, j + 1, k + 1), all read from the block (i .. i + 1, j .. j + 1, k .. k + 1) modulo n: every element is counted once;
 *   n0, n1, n2, n3 = the vertices, edges, faces and voxels inside, exact integers.
 * The caller forms V0 = n3 / N, V1 = 2 (n2 - 3 n3) / (9 a N), V2 = 2 (n1 - 2 n2 + 3 n3) / (9 a^2 N), V3 = (n0 - n1 + n2 - n3) /
 * (a^3 N) with N = n^3 and a = Lbox / n.  "mesh": n * n rows of `pitch` floats, aligned to 4 bytes; pitch == n is a dense mesh,
 * pitch == abacus_slab_pitch(n) the real side of a padded spectrum; the floats of a row beyond its n cells are never read.  A mesh
 * aligned to 16 bytes with a pitch that is a multiple of 4 is read with 16-byte loads.  The mesh must be finite; that is not checked
 * on the device (a NaN lies below every threshold, +inf above every one).  Limits, checked on the host before anything is launched,
 * every message starting with the entry's name: 2 <= n <= 32767 (even for the two entries that handle a spectrum), pitch >= n,
 * 1 <= nthr <= 64, thresholds finite and strictly increasing as float32; no null argument.
 */
/* fails, naming the largest mesh that fits, when the spectrum + the work area of one deposit and transform (two padded meshes) + the
 * copies and deposit lists of np particles do not fit the free device memory */
int abacus_mf_check_memory(int n, int64_t np);
/* counts_host[4][nthr] int64, rows n0, n1, n2, n3, for the nthr thresholds (HOST array) in ONE pass over the mesh (not modified).
 * mf_count: b(v) = the number of thresholds <= v is monotonic, so every cell is located among the thresholds once (8 comparisons
 * against every eighth threshold, 7 against one group of a table in LDS) and the maxima are taken of the bins; tiles of 16 x 64 cells marched along x with a one-cell halo; uint32 bins
 * per workgroup in LDS (integer adds), flushed once per workgroup and added to 64-bit totals by a second kernel: no float atomics,
 * nothing depends on the order of arrival.  The host takes the suffix sums over the bins and checks that every class adds up to its
 * N, 3 N, 3 N, N elements.  Device memory: 1040 bytes per workgroup of 16 x 64 x 32 cells. */
int abacus_mf_counts_dev(const float *mesh, int n, int pitch, const float *thresholds_host, int nthr, int64_t *counts_host);
/* out2_host[0] = sum x, out2_host[1] = sum x^2 over the n^3 cells in float64 (every x and x * x is exact in float64): per-workgroup
 * partial sums over a fixed deal of the rows to 2048 workgroups, then one workgroup per sum over the partials, both in a fixed order -
 * the same bits on every run */
int abacus_mf_moments_dev(const float *mesh, int n, int pitch, double *out2_host);
/* spec_padded: a padded spectrum delta(k), normalised as get_field_fft normalises (abacus_zcv_spectrum_dev), n even, aligned to 16
 * bytes.  In place: every mode times exp(-k^2 R^2 / 2) in float32 - the multiplier of abacus_zcv_filter_dev with kcut = 1 / R:
 * dk = float32(2 pi / Lbox), index i -> i below n/2, i - n from n/2 on (x, y), 0 .. n/2 on z, expf(-(kx^2 + ky^2 + kz^2) /
 * float32(2 / R^2)) - then the C2R in place (no normalisation): the padded real mesh delta_R(x) in the first n floats of every row.
 * R >= 0 and finite; R = 0: no filter.  hipFFT may take a work area. */
int abacus_mf_smooth_spectrum_dev(void *spec_padded, int n, double Lbox, double R);

/* ---------------------------------------------------------------- Spherical voids -------------------------- */
/*
 * Spherical voids of a periodic mesh on DEVICE pointers (csrc/voids.hip; Python: analysis/voids.py); every call enqueues on the
 * library stream.  replaces: nothing in the reference, which has no void finder.  Algorithm: the mesh-based spherical void finder of
 * Banerjee & Dalal 2016, stated so that its decisions are integers (tests/voids_statement.py is the NumPy statement).  A box of side
 * L, a mesh of n^3 cells of side a = L / n, cell i centred at i a; m <= 32 radii R_0 > R_1 > .. > 0 with 2 R_0 <= L / 2 ("levels").
 *   Field of level i: delta(k) as abacus_zcv_spectrum_dev leaves it, every mode times float32(W(x)), W(x) = 3 (sin x - x cos x) / x^3
 *   evaluated in float64 (1 - x^2/10 + x^4/280 below x = 0.1, W(0) = 1), x = |k| R_i, |k| = (2 pi / L) sqrt(i^2 + j^2 + l^2) of the
 *   integer mode numbers (index i -> i below n/2, i - n from n/2 on (x, y), 0 .. n/2 on z; the Nyquist planes keep the multiplier of
 *   their |k|), then the C2R without normalisation.
 *   Candidates of level i: the cells with value < threshold, compared in float32 (never a NaN; -inf is one).  Key: (value, flat index
 *   (x n + y) n + z), ordered by value first; -0.0 and +0.0 are one value.
 *   Overlap: two voids of levels i and j overlap iff d2 < D[i][j], d2 = dx^2 + dy^2 + dz^2 of the minimum-image integer differences of
 *   their centre cells, D[i][j] = ceil((R_i / a + R_j / a)^2) an int64 table computed once by the caller in float64.  d2 = D[i][j],
 *   touching spheres, is no overlap.
 *   Selection: levels in increasing order; within a level the candidates in ascending key order; a candidate becomes a void of its
 *   level iff it overlaps no void accepted so far.  The device reaches the same set in rounds: (1) the candidates that overlap a void
 *   of an earlier level die; (2) every live candidate whose key is below that of every live candidate it overlaps is accepted; (3) the
 *   live candidates that overlap a newly accepted one die; (2) and (3) repeat while one is live.  A round is two kernels (void_accept,
 *   void_settle); the kernel boundary is the only synchronisation - no thread waits for another, no cooperative launch.  Every round
 *   accepts at least the smallest live key, so the rounds of a level are at most its candidates; beyond that the call fails.
 * "Padded meshes" as in the recon section: n * n rows of abacus_slab_pitch(n) floats, abacus_zcv_spectrum_bytes(n) bytes, aligned to
 * 16 bytes.  Limits, checked before the device is touched, every message starting with the entry's name: n even, 4 .. 1024 (a cell
 * is kept as three 10-bit coordinates); pitch >= n; 1 .. 32 levels, taken in increasing order and each at most once; D symmetric,
 * positive and at most (n / 2)^2; the threshold finite; no null argument; a freed handle is refused, not followed.
 */
typedef struct abacus_void abacus_void;
/* fails, naming the largest mesh that fits, when the spectrum, the smoothed mesh, the work area of one deposit and transform, the
 * copies and deposit lists of np particles and the selection's worst case (every cell a candidate: 30 bytes per cell) do not fit */
int abacus_void_check_memory(int n, int64_t np);
/* spec_padded (not modified) -> out_padded: void_wtable fills float32(W) for s = i^2 + j^2 + l^2 = 0 .. 3 (n/2)^2 in float64 (no
 * float32 sin / cos anywhere), void_tophat multiplies every mode by its entry (16 bytes per mode; the floats of a row beyond its
 * n/2 + 1 modes are not written), then the C2R in place in out_padded: the field of a level in the first n floats of every row.
 * R >= 0 and finite; the two meshes must differ.  hipFFT may take a work area. */
int abacus_void_tophat_dev(const void *spec_padded, int n, double Lbox, double R, void *out_padded);
/* a finder for a mesh of n^3 cells and nlevels levels; d2min_host: the table D[nlevels][nlevels] (HOST).  Touches no device memory. */
int abacus_void_create(int n, int nlevels, const int64_t *d2min_host, abacus_void **handle);
/* one level on the mesh (n * n rows of `pitch` floats, aligned to 4 bytes, not modified; the floats of a row beyond its n cells are
 * never read): its candidates binned by integer bricks of at least sqrt(D[level][level]) cells (two passes over the mesh around a
 * prefix scan), the voids of the earlier levels in a brick grid of their own, then the rounds.  *ncand, *nvoid, *rounds (HOST): the
 * candidates, the voids accepted and the rounds of this level; no candidate (or none that survives the earlier levels): 0 voids,
 * 0 rounds.  The live count is read back after every round; the accepted keys are sorted on the host and kept in the handle. */
int abacus_void_level_dev(abacus_void *handle, const float *mesh, int pitch, int level, float threshold, int64_t *ncand, int64_t *nvoid,
                          int64_t *rounds);
/* the number of voids accepted so far, then their cells[nvoid][3] (x, y, z), levels[nvoid] and deltas[nvoid] (the centre value as
 * keyed: -0.0 comes back as +0.0) into HOST arrays, in level order and within a level in ascending key order */
int abacus_void_count(abacus_void *handle, int64_t *nvoid);
int abacus_void_fetch(abacus_void *handle, int32_t *cells, int32_t *levels, float *deltas);
/* releases the handle and its device buffers (NULL: nothing to do); a freed handle is refused */
int abacus_void_free(abacus_void *handle);

/* ---------------------------------------------------------------- Watershed voids -------------------------- */
/*
 * Watershed zones and the saddle tree of a periodic mesh on a DEVICE pointer (csrc/watershed.hip; Python: analysis/watershed.py);
 * every call enqueues on the library stream.  replaces: nothing in the reference, which has no void finder.  Algorithm: the zones of
 * ZOBOV (Neyrinck 2008) / VIDE on a mesh, as the voxel finder of REVOLVER takes them, stated so that every decision is an integer
 * comparison (tests/watershed_statement.py is the NumPy statement).
 *   Mesh: n^3 float32 cells, n even, 4 .. 1024, flat index f = (x n + y) n + z < 2^30.  The key of a cell is (value, f), by value
 *   first, compared in float32 with -0.0 and +0.0 one value: a strict total order.  On the device one 64-bit word: the
 *   order-preserving bit pattern of the value in the high half, f in the low half.
 *   Descent: connectivity 6 (faces) or 26 (faces, edges, corners); down[c] = the cell of smallest key among c and its periodic
 *   neighbours; a cell with down[c] == c is a core.
 *   Zones: the zone of c is the core reached by following down; zones are numbered 0 .. Z - 1 in ascending flat index of their core.
 *   Per zone: ncell; core (x, y, z); delta_min, the keyed value of the core (-0.0 comes back as +0.0); offset_sum, per axis the sum
 *   over its cells of (c - core) mod n, minus n where that is >= n / 2 - exact integers; delta_sum, the float64 sum of its cells'
 *   values in no fixed order, the only inexact output (|error| <= ncell 2^-53 sum |x|).
 *   Saddle tree: an edge is a pair of adjacent cells (the same connectivity) in different zones; hi is the cell of the larger key,
 *   lo the other; its weight is (key(hi), key(lo)), compared lexicographically - unique per cell pair, a strict total order.  The
 *   tree is the minimum spanning tree of the zone graph under these weights: Z - 1 edges (the torus is connected), unique, output in
 *   ascending weight - the order in which rising water joins basins.
 * The mesh: n * n rows of `pitch` floats, aligned to 4 bytes, not modified; pitch == n is a dense mesh, pitch ==
 * abacus_slab_pitch(n) the real side of a padded spectrum; the floats of a row beyond its n cells are never read.  The mesh must be
 * finite; that is not checked on the device.  Limits, checked before the device is touched, every message starting with the
 * entry's name: n even, 4 .. 1024; connectivity 6 or 26; pitch >= n; no null argument; a freed handle is refused, not followed.
 */
typedef struct abacus_ws abacus_ws;
/* fails, naming the largest mesh that fits, when the spectrum and the work area of one deposit and transform (three padded meshes),
 * the copies and deposit lists of np particles and the finder's worst case (16 bytes per cell and 96 bytes per zone, a zone every
 * second cell: 64 bytes per cell) do not fit the free device memory */
int abacus_ws_check_memory(int n, int64_t np);
/* a finder for a mesh of n^3 cells.  Touches no device memory. */
int abacus_ws_create(int n, int connectivity, abacus_ws **handle);
/* the whole finder on one mesh; the results stay in the handle until the next run or abacus_ws_free.  ws_descend (one pass: 4 bytes
 * read and 4 written per cell, the stencil from the caches), ws_jump (pointer jumping in place, a launch per pass until one changes
 * nothing, at most 40), ws_mark + the prefix scan of scan.hip + ws_number (zone numbers), ws_reduce (the sums: runs of one zone
 * inside a wave are combined before the atomics), then Boruvka's rounds over the zones: ws_edges twice (a 64-bit atomicMin of
 * key(hi) per component, then of key(lo) among the pairs that matched; every cell looks at the forward half of its neighbours, so
 * every pair is seen once), ws_hook, ws_flatten; the edge count is read back per round; at most 32 rounds, beyond that the call
 * fails.  No thread waits for another.  The Z - 1 edges are sorted on the host.  HOST out: *nzones = Z; *rounds (may be NULL): the
 * rounds of the tree; *jumps (may be NULL): the passes of ws_jump - neither is part of the result. */
int abacus_ws_run_dev(abacus_ws *handle, const float *mesh, int pitch, int64_t *nzones, int *rounds, int *jumps);
/* HOST arrays of the last run: ncell[Z], core[Z][3], delta_min[Z], offset_sum[Z][3], delta_sum[Z] */
int abacus_ws_fetch_zones(abacus_ws *handle, int64_t *ncell, int32_t *core, float *delta_min, int64_t *offset_sum, double *delta_sum);
/* HOST arrays of Z - 1 entries in ascending weight: the flat indices of hi and lo, their zones, saddle = the value at hi (as keyed) */
int abacus_ws_fetch_tree(abacus_ws *handle, int64_t *hi_cell, int64_t *lo_cell, int32_t *zone_hi, int32_t *zone_lo, float *saddle);
/* labels[n][n][n] (HOST, dense): the zone number of every cell */
int abacus_ws_fetch_labels(abacus_ws *handle, int32_t *labels);
/* releases the handle and its device buffers (NULL: nothing to do); a freed handle is refused */
int abacus_ws_free(abacus_ws *handle);

/* ---------------------------------------------------------------- Wavelet scattering transform ------------- */
/*
 * Solid-harmonic wavelet scattering coefficients S0, S1, S2 of a periodic mesh on DEVICE pointers (csrc/wst.hip; Python:
 * analysis/wst.py); every call enqueues on the library stream.  replaces: nothing in the reference, which has no such statistic.
 * Estimator: Eickenberg et al. (2018) as used by Valogiannis & Dvorkin (2022); tests/wst_statement.py is the NumPy statement.
 * A mesh of n^3 float32 cells, n even, N = n^3.
 *   Field: rho^(k), a padded half spectrum in the delta(k) / N convention of abacus_zcv_spectrum_dev; the driver sets the mode k = 0
 *   to 1 (rho = 1 + delta) or to 0 (the contrast).
 *   Mode numbers: index i -> i below n/2, i - n from n/2 on (x, y), 0 .. n/2 on z.
 *   Scales: sigma_j = sigma0 2^j cells, j = 0 .. J - 1.  Profile: g(kappa) = (sigma kappa)^l exp(-sigma^2 kappa^2 / 2), kappa =
 *   (2 pi / n) sqrt(i^2 + j^2 + l^2), evaluated in float64 per value of the integer i^2 + j^2 + l^2 and rounded once to float32.
 *   Harmonics: S_lm(k^), m = 1 .. 2 l + 1, the real harmonics scaled so that sum_m S_lm(a) S_lm(b) = P_l(a . b): polynomials of the
 *   unit vector formed in float32 from the mode numbers (l = 0, 2, 4 as in the light-cone section; l = 1: z, x, y; l = 3:
 *   z (5 z^2 - 3) / 2, sqrt(6)/4 {x, y} (5 z^2 - 1), sqrt(15)/2 z (x^2 - y^2), sqrt(15) x y z, sqrt(10)/4 x (x^2 - 3 y^2),
 *   sqrt(10)/4 y (3 x^2 - y^2)).
 *   Multiplier of a mode: g S_lm for even l, i g S_lm for odd l ((re, im) -> (-im, re)); for l > 0 exactly 0 at k = 0 and on every
 *   mode with a mode number n/2 in any axis (the stored mode stands for +-n/2, S_lm differs on the two: only with the zeros is the
 *   product Hermitian and the C2R defined).
 *   First order: U1[j, l](x) = sqrt(sum_m (C2R[multiplier_{j, l, m} rho^](x))^2); l = 0: |C2R[..]|.
 *   Second order, the same l and j1 < j2 only: U^ = R2C(U1[j1, l]) / N, U2[j1, j2, l] = the same expression on U^ at scale j2.
 *   Coefficients, for Q exponents q: S0[q] = <|rho|^q>, S1[j, l, q] = <U1^q>, S2[j1, j2, l, q] = <U2^q>, means over the N cells of
 *   pow((double)u, q) of the float32 cell, summed in float64 in two stages of a fixed order: the same bits on every run.
 * Passes and their traffic per cell of the mesh: wst_mult 8 B (8 B read + 8 B written per mode, half as many modes as cells);
 * wst_accum 8 B for the first m (4 read, 4 written), 12 B after it; wst_scale 8 B; wst_moments 4 B; between them the C2R (one per
 * (j, l, m)) and the R2C (one per (j1, l)) in place.  "Padded meshes" as in the recon section: n * n rows of abacus_slab_pitch(n)
 * floats, abacus_zcv_spectrum_bytes(n) bytes, aligned to 16 bytes; the floats of a row beyond its n cells (n/2 + 1 modes) are
 * never read as data.  Limits, checked on the host before anything is launched, every message starting with the entry's name:
 * n even, 4 .. 32766 (abacus_wst_moments_dev: 2 .. 32767, any parity, pitch >= n); 1 <= J <= 8; 0 <= L, ell <= 4; 1 <= nq <= 8 and
 * 0 < q <= 8; sigma > 0 and finite; no null argument; the three meshes of abacus_wst_modulus_dev must not overlap.
 */
/* fails, naming the largest mesh that fits, when the four padded meshes of the chain (the spectrum, the work mesh, u2 / U, the
 * spectrum of U), the profile table and the copies and deposit lists of np particles do not fit the free device memory */
int abacus_wst_check_memory(int n, int64_t np);
/* U[sigma, ell] of spec_padded (any padded spectrum in the 1 / N convention; not modified) into the first n floats of every row of
 * out_padded, through work_padded (overwritten): wst_table, then for every m wst_mult, the C2R in place in work_padded and
 * wst_accum.  sigma_cells in cells.  hipFFT may take a work area. */
int abacus_wst_modulus_dev(const void *spec_padded, int n, double sigma_cells, int ell, void *work_padded, void *out_padded);
/* the forward step of the second order: the R2C in place of a padded real mesh, every stored mode times float32(1 / N) (wst_scale) */
int abacus_wst_spectrum_dev(void *mesh_padded, int n);
/* sums_host[nq] (HOST, float64) = sum over the n^3 cells of pow((double)|x|, q_host[k]); mesh: n * n rows of `pitch` floats, aligned
 * to 4 bytes, not modified (16-byte loads when aligned to 16 bytes with a pitch that is a multiple of 4).  Per-workgroup partial sums
 * over a fixed deal of the rows to at most 2048 workgroups per exponent, then one workgroup per exponent over the partials: no float
 * atomics, and the sum of an exponent does not depend on the others asked for.  q = 1, 2 and 0.5 are taken as |x|, x x (exact in
 * float64) and the correctly rounded sqrt, which is what pow returns up to its own error (16 ulp) */
int abacus_wst_moments_dev(const float *mesh, int n, int pitch, const double *q_host, int nq, double *sums_host);
/* the whole (J, L, Q) loop on a resident spectrum.  spec_padded: its mode k = 0 is overwritten (1, or 0 with `contrast`), the rest
 * is kept.  HOST arrays out, float64, the means: S0_host[nq], S1_host[J][L + 1][nq], S2_host[J][J][L + 1][nq] with NaN where
 * j2 <= j1 (all NaN, or S2_host NULL, without `second_order`).  Takes three more padded meshes (two without second order) from the
 * library's scratch.  (L + 1)^2 J C2R in first order, (L + 1)^2 J (J - 1) / 2 C2R and (L + 1) (J - 1) R2C in second; one copy of
 * the sums and one synchronisation at the end. */
int abacus_wst_coefficients_dev(void *spec_padded, int n, int J, int L, double sigma0_cells, const double *q_host, int nq, int contrast,
                                int second_order, double *S0_host, double *S1_host, double *S2_host);

/* ---- ZCV mode-coupling window (window.hip) ---------------------------------------------------------------------------------
 * replaces: the mesh loop of periodic_window_function (abacusnbody/hod/zcv/zenbu_window.py:75-89, :103, :126-174): for every mode
 * (i, j, k) of the n x n x n/2 half mesh (the Nyquist plane of the last axis is not visited) knorm = sqrt((kvals[k]^2 + kvals[j]^2)
 * + kvals[i]^2) and mu = kvals[i] / knorm (0 at the origin) in float32, L2 = (3 mu^2 - 1) / 2, L4 = (35 mu^4 - 30 mu^2 + 3) / 8 with
 * mu^4 = (mu^2)^2, the bin o with kout[o] <= knorm < kout[o + 1] (float32 against the float64 edges), multiplicity m = 1 on the
 * plane k = 0 and 2 elsewhere.  Per bin, in float64: nmodes += m, ksum += m knorm, S[o][l][l'] += m fl32(fl32(pref_l L_l) L_l')
 * with pref = 1, 5, 9.  Modes below kout[0] or at and beyond kout[nkout] are left out.  kvals_host: the n float32 wavenumbers of
 * the mesh as the caller's NumPy forms them (its first n/2 are the half axis); kout_host: nkout + 1 finite, strictly increasing
 * edges, nkout <= 4096; n even, 2 .. 32766.  One pass, no mesh in memory, O(nkout) device memory.  Host arrays out:
 * S_host [nkout][3][3], nmodes_host [nkout], ksum_host [nkout]. */
int abacus_window_moments(int nmesh, const float *kvals_host, const double *kout_host, int nkout, double *S_host /*[nkout][3][3]*/,
                          double *nmodes_host, double *ksum_host);

#ifdef __cplusplus
}
#endif
#endif /* ABACUS_HIP_H */
