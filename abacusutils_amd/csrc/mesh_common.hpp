// What the mesh families share: the padded layout of a float32 mesh, its in-place transforms, the memory check, the scratch holder and
// the few device helpers and kernels that more than one of them uses.  Everything here is declared once, in namespace abacus; the
// sources keep what is theirs alone in an anonymous namespace.
//   mesh_common.hpp  this file
//   mesh.hip         host code only: the one cache of in-place hipFFT plans (two sizes per direction), r2c_inplace, c2r_inplace,
//                    release_plans
//   power.hip        deposit + transform + binning of P(k) with its own plan maps and mesh slots; power_field_spectrum_dev and
//                    power_bin_padded_dev, which the control variates and the mesh statistics call
//   shear.hip        the Gaussian filter passes, tidal_component, tidal_full, shear_accumulate, mesh_gather (abacus_shear_*)
//   zcv.hip          Zel'dovich control variates: zcv_mult, zcv_delta, zcv_accum, zcv_mean, zcv_unpad, zcv_sub_means, zcv_add_ij,
//                    zcv_lattice, zcv_shift_wrap (abacus_zcv_*), and smooth_c2r_inplace beside the zcv_mult<OP_FILTER> it launches
//   lcv.hip          linear control variates: lcv_linear, lcv_sub, lcv_power3d, lcv_combine (abacus_lcv_*)
//   recon.hip        BAO reconstruction: recon_mult, recon_wrap, recon_pack_soa64, recon_shift (abacus_recon_*)
//   lc_power.hip     light-cone power multipoles: lc_ylm_mult, lc_ylm_accum, lc_extent, lc_pack, lc_axpy, lc_compensate, lc_sum_*
//                    (abacus_lc_*)
//   bispectrum.hip   bk_shell_mask, bk_triple, bk_triple_final (abacus_bk_*)
//   minkowski.hip    mf_* kernels (abacus_mf_*); voids.hip: void_* kernels (abacus_void_*); wst.hip: wst_* kernels (abacus_wst_*);
//                    window.hip: the mode-coupling window (abacus_window_*)
// zcv_pad stands here because lcv.hip and recon.hip both launch it: a kernel in this header is compiled into every file that uses
// it, as the same code (scripts/kernel_isa_diff.py holds the copies to that).
// What fft.hip, gfft.hip, xbin.hip, tsc.hip and scan.hip offer is declared in common.hpp; release_plans (mesh.hip) too, for runtime.hip.
#pragma once

#include <hipfft/hipfft.h>

#include <algorithm>
#include <vector>

#include "../../include/abacus_hip.h"
#include "common.hpp"

namespace abacus {

constexpr int BLK = 256;         // threads per workgroup of the mesh kernels
constexpr int LCV_ROWS = 8;      // (a, b) rows a workgroup takes at a time in lcv_for_each_mode

// ---- the padded layout: rows of pitch_r floats start on 128-B boundaries and hold the n + 2 floats of the in-place R2C
inline int pitch_r(int n) { return (n + 2 + 31) / 32 * 32; }
inline size_t padded_bytes(int n) { return (size_t)n * n * pitch_r(n) * sizeof(float); }
inline int pitch_r64(int n) { return (n + 2 + 15) / 16 * 16; }          // the float64 meshes: doubles per z row, rows start on 128-B lines
inline unsigned int grid_for(int64_t blocks, int per_cu) {
    return (unsigned int)std::max<int64_t>(1, std::min<int64_t>(blocks, (int64_t)fft_num_cus() * per_cu));
}

struct Scratch {   // scratch_acquire'd blocks released when the entry point returns
    std::vector<void *> blocks;
    ~Scratch() {
        for (void *p : blocks) scratch_release(p);
    }
    template <class T>
    int get(T **out, size_t bytes) {
        void *p = nullptr;
        ABACUS_TRY(scratch_acquire(&p, bytes));
        blocks.push_back(p);
        *out = static_cast<T *>(p);
        return 0;
    }
};

// `bytes_of(n)` bytes must fit beside what is allocated already; the message names the largest even mesh from min_n up that does
template <class F>
int check_memory(const char *who, int n, int min_n, F bytes_of) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const size_t slack = (size_t)256 << 20;
    if (bytes_of(n) + slack <= free_b) return 0;
    ABACUS_TRY(scratch_trim_idle());
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (bytes_of(n) + slack <= free_b) return 0;
    int m = n;
    while (m > min_n && bytes_of(m) + slack > free_b) m -= 2;
    return fail("%s: the meshes of %d^3 need %.1f GB of HBM, %.1f GB are free; the largest mesh that fits is %d^3", who, n,
                1e-9 * (double)bytes_of(n), 1e-9 * (double)free_b, m);
}

// ---- hipFFT
inline int fft_check(hipfftResult r, const char *what) {
    if (r != HIPFFT_SUCCESS) return fail("%s failed (hipfftResult %d)", what, (int)r);
    return 0;
}

// hipFFT allocates its work area when a plan is made: with idle scratch blocks of this library around, give them back and try
// once more before reporting the failure
template <typename F>
hipfftResult plan_with_retry(F make) {
    hipfftResult r = make();
    if (r != HIPFFT_SUCCESS) {
        (void)hipGetLastError();
        if (scratch_trim_idle() == 0) r = make();
    }
    return r;
}

// mesh.hip: the transforms of a padded float32 mesh, in place and without normalisation.  R2C by the native transforms where they
// cover the size (and the option fft_hipfft is not set), else by a cached hipFFT plan; C2R always by a cached hipFFT plan.
int r2c_inplace(float *D, int n);
int c2r_inplace(float *W, int n);
// zcv.hip: D, a padded spectrum normalised as get_field_fft normalises, times exp(-k^2 R^2 / 2) as the filter of gaussian_filter forms
// it with kcut = 1 / R (R = 0: no filter), then the C2R in place: the padded real mesh
int smooth_c2r_inplace(float *D, int n, double Lbox, double R);
// power.hip: deposit + transform of a particle set into a padded spectrum, and the binning of one or two padded spectra
int power_field_spectrum_dev(float *pos, int64_t n, const float *w, double Lbox, int nmesh, int paste, const float *W_host, int interlaced,
                             void *dest);
int power_bin_padded_dev(const void *a, const void *b, int nmesh, double Lbox, const double *kedges, int Nk, const double *muedges, int Nmu,
                         const int64_t *poles, int Np, float *power, int64_t *N_mode, float *binned_poles, int64_t *N_mode_poles,
                         float *k_avg);

// ---- device helpers
// fixed-order sum of one double per thread over the workgroup; the result is valid in thread 0
__device__ __forceinline__ double block_sum(double v, double *lds) {
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int s = BLK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
        __syncthreads();
    }
    const double r = lds[0];
    __syncthreads();
    return r;
}

// the reference's wavenumber of index i on the x and y axes: float32(i) * dk, float32(i - n) * dk from n / 2 on
__device__ __forceinline__ float kxy(int i, int n, float dk) { return (float)(i < n / 2 ? i : i - n) * dk; }

__device__ __forceinline__ int fold(int i, int n) { return i < n / 2 ? i : i - n; }

// f(row, c) for every mode of an n x n x (n/2+1) spectrum whose rows are pc complex apart.  No lane strides along z: a workgroup takes
// LCV_ROWS consecutive (a, b) rows at a time and walks the flat index of their LCV_ROWS * pitch padded elements (32-bit index
// arithmetic; several trips through the lane loop from n = 64 on), skipping the pad columns.
template <class F>
__device__ __forceinline__ void lcv_for_each_mode(int n, int pc, F f) {
    const int kzlen = n / 2 + 1, rows = n * n;
    const int groups = (rows + LCV_ROWS - 1) / LCV_ROWS;
    const unsigned int per = (unsigned int)LCV_ROWS * (unsigned int)pc;
    for (int g = blockIdx.x; g < groups; g += gridDim.x)
        for (unsigned int e = threadIdx.x; e < per; e += BLK) {
            const unsigned int r = e / (unsigned int)pc, c = e - r * (unsigned int)pc;
            const int row = g * LCV_ROWS + (int)r;
            if ((int)c < kzlen && row < rows) f(row, (int)c);
        }
}

// NumPy's float32 `%` (npy_remainderf): fmod, then + b when the remainder is negative (b > 0 here); the sum may round to b itself
__device__ __forceinline__ float np_remainder(float a, float b) {
    float mod = fmodf(a, b);
    if (mod != 0.0f) {
        if (mod < 0.0f) mod = __fadd_rn(mod, b);
    } else {
        mod = 0.0f;
    }
    return mod;
}

// contiguous rows -> padded rows
static __global__ __launch_bounds__(BLK) void zcv_pad(const float *__restrict__ in, float *__restrict__ padded, int n, int64_t pitch) {
    const int64_t rows = (int64_t)n * n;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x)
        for (int c = threadIdx.x; c < n; c += BLK) padded[row * pitch + c] = in[row * n + c];
}

}  // namespace abacus
