// Zel'dovich control variates on MI355X (gfx950): the heavy half of abacusnbody/hod/zcv - ic_fields.py (gaussian_filter :79-107,
// filter_field :110-148, get_n2_fft :151-189, get_sij_fft :192-255, add_ij :258-268, get_dk_to_s2 :271-309, get_dk_to_n2 :312-333,
// get_fields :336-366), the lattice advection of advect_fields.py main :213-239 and the deposits + spectra behind it and behind
// tracer_power.py get_tracer_power :155-273.
//
// get_fields, all in HBM:  delta -> [zcv_delta: padded copy, delta^2, partial sums of both means] -> R2C in place (fft.hip /
// gfft.hip, hipFFT for sizes they do not cover) -> six times [zcv_mult<SIJ>: s_ij(k) / n^3 into the work mesh, hipFFT C2R in place,
// zcv_accum: s2 (+)= w t^2, the last one with the partial sums of mean(s2)] -> [zcv_mult<N2>, C2R, zcv_unpad -> nabla^2 delta] ->
// [zcv_sub_means: d = delta - mean, d2 -= mean, s2 -= mean].  The means are two-stage float64 sums in a fixed order (per thread,
// LDS tree per workgroup, one workgroup over the partials): no floating-point atomics, the same bits on every run.
//
// Wavenumbers as the reference forms them: dk = float32(2 pi / L), index i -> i (i < n/2) or i - n (the Nyquist index is
// NEGATIVE on x and y, positive on z: 0 .. n/2).  With that, k_i k_j is odd under k -> -k on the x and y Nyquist lines, and because
// k_z keeps its sign on the self-conjugate planes c = 0 and c = n/2 the xz / yz components are odd there as well: the s_ij spectra
// are not Hermitian on those two planes.  The reference's irfftn (complex along x and y, real along z last) drops the imaginary part
// of the two transformed planes, which equals replacing each plane by its Hermitian part (t(a, b) + conj t(-a, -b)) / 2.  zcv_mult
// writes that rule out (HERM), so the C2R library always sees a Hermitian spectrum.
//
// The linear control variates (linear_fields.py, tracer_power.py get_recon_power, tools_cv.py combine_field_spectra_k3D_lcv) share this
// file's transform, padding and memory helpers: their four streaming kernels and entry points (abacus_lcv_*) are in the LCV sections below.
// BAO reconstruction (the displacement field and the RecSym / RecIso shifts that produce the catalogues the LCV start from) follows
// them: abacus_recon_*.  The light-cone power spectrum multipoles (analysis/lc_power.py: FKP field, Yamamoto estimator) close the file:
// abacus_lc_*.
//
// This file is compiled with -ffp-contract=off (csrc/Makefile): the lattice positions are bit-equal to NumPy's float32 operations and
// the LCV products follow NumPy's float32 order of evaluation.
#include <hipfft/hipfft.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/abacus_hip.h"
#include "common.hpp"

using namespace abacus;

namespace abacus {
bool fft_native_supported(int n);
int fft_native_r2c_inplace(float *mesh, int n, int pitch_r, float xcut);
int fft_num_cus();
int power_field_spectrum_dev(float *pos, int64_t n, const float *w, double Lbox, int nmesh, int paste, const float *W_host, int interlaced,
                             void *dest);
int power_bin_padded_dev(const void *a, const void *b, int nmesh, double Lbox, const double *kedges, int Nk, const double *muedges, int Nmu,
                         const int64_t *poles, int Np, float *power, int64_t *N_mode, float *binned_poles, int64_t *N_mode_poles,
                         float *k_avg);
}  // namespace abacus

namespace {

constexpr int BLK = 256;
constexpr int OP_FILTER = 0, OP_N2 = 1, OP_SIJ = 2;

int pitch_r(int n) { return (n + 2 + 31) / 32 * 32; }
size_t padded_bytes(int n) { return (size_t)n * n * pitch_r(n) * sizeof(float); }
unsigned int grid_for(int64_t blocks, int per_cu) { return (unsigned int)std::max<int64_t>(1, std::min<int64_t>(blocks, (int64_t)fft_num_cus() * per_cu)); }

// the reference's wavenumber of index i on the x and y axes: float32(i) * dk, float32(i - n) * dk from n / 2 on
__device__ __forceinline__ float kxy(int i, int n, float dk) { return (float)(i < n / 2 ? i : i - n) * dk; }

struct MultArgs {
    int n, pitch_src, pitch_dst;   // pitches in complex elements per (a, b) row
    int ci, cj;                    // s_ij component, 0..2
    float dk, norm, scale;         // float32(2 pi / L), float32(2 kcut^2), factor folded in (1 / n^3 in front of a C2R, else 1)
};

// factor of one mode for OP; (a, b, c) are mesh indices, kc is on the positive z axis
template <int OP>
__device__ __forceinline__ float mode_factor(const MultArgs &m, int a, int b, int c) {
    const float kx = kxy(a, m.n, m.dk), ky = kxy(b, m.n, m.dk), kz = (float)c * m.dk;
    const float kmag2 = kx * kx + ky * ky + kz * kz;
    if (OP == OP_FILTER) return expf(-kmag2 / m.norm);
    if (OP == OP_N2) return -kmag2;
    const float inv = (a + b + c > 0) ? 1.0f / kmag2 : 0.0f;     // only the zero vector is special (ic_fields.py:244-247)
    const float ki = m.ci == 0 ? kx : (m.ci == 1 ? ky : kz), kj = m.cj == 0 ? kx : (m.cj == 1 ? ky : kz);
    return ki * kj * inv - (m.ci == m.cj ? 1.0f / 3.0f : 0.0f);
}

// dst(a, b, c) = factor(a, b, c) * src(a, b, c) * scale: one (a, b) row per workgroup step, lanes along c.  HERM (s_ij in front of a
// C2R): on the planes c = 0 and c = n/2 the Hermitian part (t(a, b) + conj t(-a, -b)) / 2; src and dst are different meshes then
// (the filter runs in place: no restrict).
template <int OP, bool HERM>
__global__ __launch_bounds__(BLK) void zcv_mult(const float2 *src, float2 *dst, MultArgs m) {
    const int n = m.n, kzlen = n / 2 + 1;
    const int64_t rows = (int64_t)n * n;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const int a = (int)(row / n), b = (int)(row % n);
        for (int c = threadIdx.x; c < kzlen; c += BLK) {
            const float f = mode_factor<OP>(m, a, b, c) * m.scale;
            const float2 d = src[row * m.pitch_src + c];
            float2 t = make_float2(d.x * f, d.y * f);
            if (HERM && (c == 0 || c == n / 2)) {
                const int a2 = a ? n - a : 0, b2 = b ? n - b : 0;
                const float f2 = mode_factor<OP>(m, a2, b2, c) * m.scale;
                const float2 d2 = src[((int64_t)a2 * n + b2) * m.pitch_src + c];
                t = make_float2(0.5f * (t.x + d2.x * f2), 0.5f * (t.y - d2.y * f2));
            }
            dst[row * m.pitch_dst + c] = t;
        }
    }
}

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

// delta (n^3 contiguous) -> padded copy for the transform, d2 = delta * delta, partial sums of delta and delta^2 per workgroup
__global__ __launch_bounds__(BLK) void zcv_delta(const float *__restrict__ in, float *__restrict__ padded, float *__restrict__ d2, int n,
                                                 int pitch, double *__restrict__ partial) {
    __shared__ double lds[BLK];
    const int64_t rows = (int64_t)n * n;
    double s1 = 0.0, s2 = 0.0;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const float *src = in + row * n;
        for (int c = threadIdx.x; c < n; c += BLK) {
            const float v = src[c], q = v * v;
            padded[row * pitch + c] = v;
            d2[row * n + c] = q;
            s1 += (double)v;
            s2 += (double)q;
        }
    }
    const double t1 = block_sum(s1, lds), t2 = block_sum(s2, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = t1, partial[gridDim.x + blockIdx.x] = t2;
}

// q (+)= w t^2 over the n^3 cells of the padded work mesh (add_ij, ic_fields.py:258-268); SUM: partial sums of the finished q
template <bool FIRST, bool SUM>
__global__ __launch_bounds__(BLK) void zcv_accum(const float *__restrict__ work, float *__restrict__ q, int n, int64_t pitch, float w,
                                                 double *__restrict__ partial) {
    __shared__ double lds[BLK];
    const int64_t rows = (int64_t)n * n;
    double s = 0.0;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const float *src = work + row * pitch;
        float *dst = q + row * n;
        for (int c = threadIdx.x; c < n; c += BLK) {
            const float t = src[c];
            float acc = w * (t * t);
            if (!FIRST) acc += dst[c];
            dst[c] = acc;
            if (SUM) s += (double)acc;
        }
    }
    if (SUM) {
        const double t = block_sum(s, lds);
        if (threadIdx.x == 0) partial[blockIdx.x] = t;
    }
}

// second stage of the means: one workgroup, mean[j] = float32(sum of partial[j * npart ..] / count)
__global__ __launch_bounds__(BLK) void zcv_mean(const double *__restrict__ partial, int npart, int nsum, double count, float *__restrict__ mean) {
    __shared__ double lds[BLK];
    for (int j = 0; j < nsum; j++) {
        double s = 0.0;
        for (int i = threadIdx.x; i < npart; i += BLK) s += partial[(int64_t)j * npart + i];
        const double t = block_sum(s, lds);
        if (threadIdx.x == 0) mean[j] = (float)(t / count);
    }
}

// padded rows -> contiguous rows
__global__ __launch_bounds__(BLK) void zcv_unpad(const float *__restrict__ work, float *__restrict__ out, int n, int64_t pitch) {
    const int64_t rows = (int64_t)n * n;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x)
        for (int c = threadIdx.x; c < n; c += BLK) out[row * n + c] = work[row * pitch + c];
}

// contiguous rows -> padded rows
__global__ __launch_bounds__(BLK) void zcv_pad(const float *__restrict__ in, float *__restrict__ padded, int n, int64_t pitch) {
    const int64_t rows = (int64_t)n * n;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x)
        for (int c = threadIdx.x; c < n; c += BLK) padded[row * pitch + c] = in[row * n + c];
}

// d = delta - mean[0], d2 -= mean[1], s2 -= mean[2] (get_fields, ic_fields.py:343-359)
__global__ __launch_bounds__(BLK) void zcv_sub_means(const float *delta, float *d, float *__restrict__ d2,
                                                     float *__restrict__ s2, int64_t total, const float *__restrict__ mean) {
    const float m0 = mean[0], m1 = mean[1], m2 = mean[2];
    for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < total; i += (int64_t)gridDim.x * BLK) {
        d[i] = delta[i] - m0;
        d2[i] = d2[i] - m1;
        s2[i] = s2[i] - m2;
    }
}

// final += factor * field^2 on two contiguous meshes (the piecewise add_ij)
__global__ __launch_bounds__(BLK) void zcv_add_ij(float *__restrict__ fin, const float *__restrict__ field, int64_t total, float factor) {
    for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < total; i += (int64_t)gridDim.x * BLK) {
        const float t = field[i];
        fin[i] = fin[i] + factor * (t * t);
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

// advect_fields.py main :213-239, operation by operation in float32 (no contraction): one particle per lattice site (i, j, k),
// ((disp * D [* (1 + f)]) + float32(index) / float32(n)) * L  %  L -> packed (n^3, 3)
__global__ __launch_bounds__(BLK) void zcv_lattice(const float *__restrict__ dx, const float *__restrict__ dy, const float *__restrict__ dz,
                                                   float *__restrict__ pos, int n, float D, float onepf, int rsd, float L) {
    const int64_t rows = (int64_t)n * n;
    const float fn = (float)n;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const int i = (int)(row / n), j = (int)(row % n);
        const float gx = __fdiv_rn((float)i, fn), gy = __fdiv_rn((float)j, fn);
        for (int k = threadIdx.x; k < n; k += BLK) {
            const int64_t p = row * n + k;
            const float gz = __fdiv_rn((float)k, fn);
            float x = __fmul_rn(dx[p], D), y = __fmul_rn(dy[p], D), z = __fmul_rn(dz[p], D);
            if (rsd) z = __fmul_rn(z, onepf);
            x = np_remainder(__fmul_rn(__fadd_rn(x, gx), L), L);
            y = np_remainder(__fmul_rn(__fadd_rn(y, gy), L), L);
            z = np_remainder(__fmul_rn(__fadd_rn(z, gz), L), L);
            pos[3 * p] = x;
            pos[3 * p + 1] = y;
            pos[3 * p + 2] = z;
        }
    }
}

// tracer_power.py:157-158 on float32 device positions: pos += float32(L / 2); pos %= float32(L)
__global__ __launch_bounds__(BLK) void zcv_shift_wrap(float *__restrict__ pos, int64_t total, float half, float L) {
    for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < total; i += (int64_t)gridDim.x * BLK)
        pos[i] = np_remainder(__fadd_rn(pos[i], half), L);
}

// ---- linear control variates (LCV): linear_fields.py :108-124, tracer_power.py get_recon_power :410-414, :464, :501-503 and
// tools_cv.py combine_field_spectra_k3D_lcv :313-335.  Four streaming passes over padded spectra.  None of them strides its lanes
// along z: a workgroup takes LCV_ROWS consecutive (a, b) rows at a time and walks the flat index of their LCV_ROWS * pitch padded
// elements (32-bit index arithmetic; several trips through the lane loop from n = 64 on), skipping the pad columns.
constexpr int LCV_ROWS = 8;

__device__ __forceinline__ int fold(int i, int n) { return i < n / 2 ? i : i - n; }

// f(row, c) for every mode of an n x n x (n/2+1) spectrum whose rows are pc complex apart
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

// get_delta_mu2 (analysis/power_spectrum.py:604-616): kmag2 = f32(i^2 + j^2 + k^2) in mode numbers, mu^2 = f32(k^2) * kmag2**-1,
// 0 for the zero vector
__device__ __forceinline__ float lcv_kmag2(int row, int c, int n) {
    const int a = fold(row / n, n), b = fold(row % n, n);
    return (float)(a * a + b * b + c * c);
}
__device__ __forceinline__ float lcv_mu2(float kmag2, int c) { return kmag2 > 0.f ? __fmul_rn((float)(c * c), __fdiv_rn(1.0f, kmag2)) : 0.f; }

// d = rfftn(delta) in the padded layout -> d * scl (NumPy divides complex64 by a real scalar as a product with its float32
// reciprocal) and, in the same pass, mu = that * mu^2: get_delta_mu2 fused with the normalisation
__global__ __launch_bounds__(BLK) void lcv_linear(float2 *d, float2 *__restrict__ mu, int n, int pc, float scl) {
    lcv_for_each_mode(n, pc, [&](int row, int c) {
        const int64_t q = (int64_t)row * pc + c;
        const float2 v = d[q];
        const float2 t = make_float2(v.x * scl, v.y * scl);
        const float m = lcv_mu2(lcv_kmag2(row, c, n), c);
        d[q] = t;
        mu[q] = make_float2(t.x * m, t.y * m);
    });
}

// a -= b over whole padded spectra (the pad columns ride along: 16-byte accesses, no index arithmetic)
__global__ __launch_bounds__(BLK) void lcv_sub(float4 *__restrict__ a, const float4 *__restrict__ b, int64_t total4) {
    for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < total4; i += (int64_t)gridDim.x * BLK) {
        float4 x = a[i];
        const float4 y = b[i];
        x.x -= y.x, x.y -= y.y, x.z -= y.z, x.w -= y.w;
        a[i] = x;
    }
}

// Re(u conj v) as NumPy forms the real part of a complex64 product: u.re v.re - u.im (-v.im)
__device__ __forceinline__ float lcv_cross(float2 u, float2 v) { return u.x * v.x + u.y * v.y; }

// out (n, n, n/2+1) contiguous = Re(a conj b), b == nullptr: |a|^2 = Re(a conj a)
__global__ __launch_bounds__(BLK) void lcv_power3d(const float2 *__restrict__ a, const float2 *__restrict__ b, float *__restrict__ out, int n,
                                                   int pc) {
    const int kzlen = n / 2 + 1;
    lcv_for_each_mode(n, pc, [&](int row, int c) {
        const int64_t q = (int64_t)row * pc + c;
        const float2 u = a[q];
        out[(int64_t)row * kzlen + c] = lcv_cross(u, b ? b[q] : u);
    });
}

struct CombineArgs {
    int n, pc;
    float c_md, c_mm, c_dd, D2;    // recsym: f32(2 b f), f32(f^2), f32(b^2), f32(D^2); reciso: c_md = f32(2 b), c_mm unused
    float b, f, D;                 // f32(bias), f32(f_growth), f32(D)
    float dk2, R2;                 // get_smoothing: f32(dk)^2 with dk = f32(2 pi / L), f32(R^2)
};

// combine_field_spectra_k3D_lcv (tools_cv.py:319-335) from the three spectra, in NumPy's float32 order of evaluation:
//   pk_ll = D^2 * ((2 b f_eff * P_md + f_eff^2 * P_mm) + b^2 * P_dd),  pk_lt = D * (b * P_dt + f_eff * P_mt),  pk_tt = |tr|^2
// RECISO: f_eff = f * (1 - exp(-kmag2 * dk2 * R2 / 2)) per mode (get_smoothing :572-573), else the scalar f
template <bool RECISO>
__global__ __launch_bounds__(BLK) void lcv_combine(const float2 *__restrict__ delta, const float2 *__restrict__ mu, const float2 *__restrict__ tr,
                                                   float *__restrict__ pk_tt, float *__restrict__ pk_ll, float *__restrict__ pk_lt,
                                                   CombineArgs m) {
    const int kzlen = m.n / 2 + 1;
    lcv_for_each_mode(m.n, m.pc, [&](int row, int c) {
        const int64_t q = (int64_t)row * m.pc + c, o = (int64_t)row * kzlen + c;
        const float2 d = delta[q], u = mu[q], t = tr[q];
        const float P_md = lcv_cross(u, d), P_mm = lcv_cross(u, u), P_dd = lcv_cross(d, d);
        const float P_dt = lcv_cross(d, t), P_mt = lcv_cross(u, t);
        float t_md, t_mm, fe;
        if (RECISO) {
            const float S = expf(-lcv_kmag2(row, c, m.n) * m.dk2 * m.R2 / 2.0f);
            fe = m.f * (1.0f - S);
            t_md = (m.c_md * fe) * P_md;
            t_mm = (fe * fe) * P_mm;
        } else {
            fe = m.f;
            t_md = m.c_md * P_md;
            t_mm = m.c_mm * P_mm;
        }
        pk_tt[o] = lcv_cross(t, t);
        pk_ll[o] = m.D2 * ((t_md + t_mm) + m.c_dd * P_dd);
        pk_lt[o] = m.D * (m.b * P_dt + fe * P_mt);
    });
}

// ---- BAO reconstruction: the producer of the positions the LCV section starts from.  Standard plane-parallel reconstruction of a
// periodic box (line of sight = z) is a closed-form Fourier solve: delta(k) -> [recon_mult: the three displacement spectra in one
// pass] -> three C2R -> [recon_shift: psi read at every particle with the cloud of the deposit, shift, wrap].  No reference code: the
// arithmetic is stated in include/abacus_hip.h and pinned to tests/recon_statement.py.
struct ReconArgs {
    int n, pc;
    float dk;          // float32(2 pi / L)
    float R2h;         // f32(R^2 / 2)
    float b, beta;     // f32(bias), f32(f / bias) or 0
    float scale;       // 1 for a spectrum normalised by n^3 (the deposit's), 1 / n^3 for a bare R2C
};

// psi_i(k) = i k_i S delta / (k^2 b (1 + beta mu^2)) for i = x, y, z from one read of delta(k): 8 B in, 24 B out per mode.  In the factor
// i k_i the wavenumber of axis i is 0 at that axis' Nyquist index (k^2, mu^2 and S keep it): the three spectra are Hermitian as written
// (delta may lie in pz: every mode is read before it is written, by the same lane; no restrict on those two)
__global__ __launch_bounds__(BLK) void recon_mult(const float2 *delta, float2 *__restrict__ px, float2 *__restrict__ py, float2 *pz, ReconArgs m) {
    const int n = m.n, h = n / 2;
    lcv_for_each_mode(n, m.pc, [&](int row, int c) {
        const int a = row / n, b = row % n;
        const int64_t q = (int64_t)row * m.pc + c;
        const float kx = kxy(a, n, m.dk), ky = kxy(b, n, m.dk), kz = (float)c * m.dk;
        const float k2 = kx * kx + ky * ky + kz * kz;
        float g = 0.0f;
        if (a + b + c > 0) {
            const float mu2 = (kz * kz) / k2;
            g = expf(-k2 * m.R2h) / (k2 * m.b * (1.0f + m.beta * mu2)) * m.scale;
        }
        const float2 d = delta[q];
        const float fx = (a == h ? 0.0f : kx) * g, fy = (b == h ? 0.0f : ky) * g, fz = (c == h ? 0.0f : kz) * g;
        px[q] = make_float2(-fx * d.y, fx * d.x);
        py[q] = make_float2(-fy * d.y, fy * d.x);
        pz[q] = make_float2(-fz * d.y, fz * d.x);
    });
}

// out = (pos + off) % L on (np, 3) float32 values: the copy the deposit works on (out may be pos)
__global__ __launch_bounds__(BLK) void recon_wrap(const float *pos, float *out, int64_t total, float off, float L) {
    for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < total; i += (int64_t)gridDim.x * BLK)
        out[i] = np_remainder(__fadd_rn(pos[i], off), L);
}

// three float64 columns -> (np, 3) float32, the offset added in float64 and the sum rounded once
__global__ __launch_bounds__(BLK) void recon_pack_soa64(const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                                                        float *__restrict__ out, int64_t np, double off) {
    for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < np; i += (int64_t)gridDim.x * BLK) {
        out[3 * i] = (float)(x[i] + off);
        out[3 * i + 1] = (float)(y[i] + off);
        out[3 * i + 2] = (float)(z[i] + off);
    }
}

// periodic cell index: any int (the conversion of a non-finite coordinate included) lands in [0, n)
__device__ __forceinline__ int recon_cell(int i, int n) { return ((i % n) + n) % n; }

// the cloud of one coordinate p in [0, L]: K = 2 (CIC: nearest cell, then its neighbour on the particle's side) or 3 (TSC: i - 1, i,
// i + 1) periodic cell indices and weights, as analysis/cic.py and analysis/tsc.py deposit them
template <int K>
__device__ __forceinline__ void recon_cloud(float p, float inv_h, int n, int *idx, float *w) {
    const float g = p * inv_h, r = rintf(g), d = r - g;
    const int i0 = (int)r;
    if (K == 2) {
        idx[0] = recon_cell(i0, n), idx[1] = recon_cell(d > 0.0f ? i0 - 1 : i0 + 1, n);
        w[0] = 1.0f - fabsf(d), w[1] = fabsf(d);
    } else {
        idx[0] = recon_cell(i0 - 1, n), idx[1] = recon_cell(i0, n), idx[K - 1] = recon_cell(i0 + 1, n);
        w[0] = 0.5f * ((0.5f + d) * (0.5f + d)), w[1] = 0.75f - d * d, w[K - 1] = 0.5f * ((0.5f - d) * (0.5f - d));
    }
}

// One lane per particle: s = (pos + off) % L, psi read at s from the three padded meshes where the C2R left them (K^3 cells of each,
// the K cells along z of a row are neighbours in memory), out = (s - psi - los psi_z z^) % L.  A gather: the meshes are read through
// L2 / Infinity Cache, particles that are neighbours in memory and in space share their rows.
template <int K>
__global__ __launch_bounds__(BLK) void recon_shift(const float *__restrict__ pos, int64_t np, float off, const float *__restrict__ mx,
                                                   const float *__restrict__ my, const float *__restrict__ mz, int n, int64_t pitch, float L,
                                                   float inv_h, float los, float *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < np; i += (int64_t)gridDim.x * BLK) {
        float s[3];
        int idx[3][K];
        float w[3][K];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            s[a] = np_remainder(__fadd_rn(pos[3 * i + a], off), L);
            recon_cloud<K>(s[a], inv_h, n, idx[a], w[a]);
        }
        float ax = 0.0f, ay = 0.0f, az = 0.0f;
#pragma unroll
        for (int u = 0; u < K; u++) {
            float bx = 0.0f, by = 0.0f, bz = 0.0f;
#pragma unroll
            for (int v = 0; v < K; v++) {
                const int64_t row = ((int64_t)idx[0][u] * n + idx[1][v]) * pitch;
                float cx = 0.0f, cy = 0.0f, cz = 0.0f;
#pragma unroll
                for (int t = 0; t < K; t++) {
                    const int64_t q = row + idx[2][t];
                    cx += w[2][t] * mx[q], cy += w[2][t] * my[q], cz += w[2][t] * mz[q];
                }
                bx += w[1][v] * cx, by += w[1][v] * cy, bz += w[1][v] * cz;
            }
            ax += w[0][u] * bx, ay += w[0][u] * by, az += w[0][u] * bz;
        }
        out[3 * i] = np_remainder(s[0] - ax, L);
        out[3 * i + 1] = np_remainder(s[1] - ay, L);
        out[3 * i + 2] = np_remainder((s[2] - az) - los * az, L);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
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

// in-place hipFFT plans in the padded layout: [0] R2C (sizes the native transforms do not cover), [1] C2R.  One size is kept.
hipfftHandle g_plan[2] = {0, 0};
int g_plan_n[2] = {0, 0};

int fft_check(hipfftResult r, const char *what) {
    if (r != HIPFFT_SUCCESS) return fail("%s failed (hipfftResult %d)", what, (int)r);
    return 0;
}

int get_plan(int n, int inverse, hipfftHandle *out) {
    if (g_plan_n[inverse] != n) {
        if (g_plan_n[inverse]) (void)hipfftDestroy(g_plan[inverse]);
        g_plan_n[inverse] = 0;
        int dims[3] = {n, n, n};
        int rembed[3] = {n, n, pitch_r(n)}, cembed[3] = {n, n, pitch_r(n) / 2};
        auto make = [&] {
            return inverse ? hipfftPlanMany(&g_plan[1], 3, dims, cembed, 1, 1, rembed, 1, 1, HIPFFT_C2R, 1)
                           : hipfftPlanMany(&g_plan[0], 3, dims, rembed, 1, 1, cembed, 1, 1, HIPFFT_R2C, 1);
        };
        hipfftResult r = make();
        if (r != HIPFFT_SUCCESS) {      // hipFFT allocates its work area with the plan: give idle scratch back and try once more
            (void)hipGetLastError();
            if (scratch_trim_idle() == 0) r = make();
        }
        ABACUS_TRY(fft_check(r, "hipfftPlanMany"));
        g_plan_n[inverse] = n;
    }
    ABACUS_TRY(fft_check(hipfftSetStream(g_plan[inverse], stream()), "hipfftSetStream"));
    *out = g_plan[inverse];
    return 0;
}

int check_size(const char *who, int n) {
    if (n < 2 || n > 32767) return fail("%s: mesh size %d out of range", who, n);
    if (n & 1) return fail("%s: odd mesh size %d (the reference's irfftn drops a cell there and add_ij indexes past it)", who, n);
    return 0;
}

// `bytes_of(n)` bytes must fit beside what is allocated already; the message names the largest even mesh that does
template <class F>
int check_memory(const char *who, int n, F bytes_of) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const size_t slack = (size_t)256 << 20;
    if (bytes_of(n) + slack <= free_b) return 0;
    ABACUS_TRY(scratch_trim_idle());
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (bytes_of(n) + slack <= free_b) return 0;
    int m = n;
    while (m > 2 && bytes_of(m) + slack > free_b) m -= 2;
    return fail("%s: the meshes of %d^3 need %.1f GB of HBM, %.1f GB are free; the largest mesh that fits is %d^3", who, n,
                1e-9 * (double)bytes_of(n), 1e-9 * (double)free_b, m);
}

MultArgs mult_args(int n, double Lbox, int pitch_src, int pitch_dst, double scale) {
    MultArgs m;
    m.n = n, m.pitch_src = pitch_src, m.pitch_dst = pitch_dst, m.ci = m.cj = 0;
    m.dk = (float)(2.0 * M_PI / Lbox);
    m.norm = 1.f;
    m.scale = (float)scale;
    return m;
}

int launch_mult(int op, bool herm, const float2 *src, float2 *dst, const MultArgs &m) {
    const dim3 grid(grid_for((int64_t)m.n * m.n, 16)), block(BLK);
    if (op == OP_FILTER)
        ABACUS_LAUNCH("zcv_mult_filter", (zcv_mult<OP_FILTER, false>), grid, block, 0, src, dst, m);
    else if (op == OP_N2)
        ABACUS_LAUNCH("zcv_mult_n2", (zcv_mult<OP_N2, false>), grid, block, 0, src, dst, m);
    else if (herm)
        ABACUS_LAUNCH("zcv_mult_sij", (zcv_mult<OP_SIJ, true>), grid, block, 0, src, dst, m);
    else
        ABACUS_LAUNCH("zcv_mult_sij", (zcv_mult<OP_SIJ, false>), grid, block, 0, src, dst, m);
    return 0;
}

int forward(float *D, int n) {
    if (fft_native_supported(n) && !option("fft_hipfft")) return fft_native_r2c_inplace(D, n, pitch_r(n), 0.f);
    hipfftHandle fwd;
    ABACUS_TRY(get_plan(n, 0, &fwd));
    prof_begin("hipfft_r2c");
    const hipfftResult r = hipfftExecR2C(fwd, (hipfftReal *)D, (hipfftComplex *)D);
    prof_end("hipfft_r2c");
    return fft_check(r, "hipfftExecR2C");
}

int inverse(float *W, int n) {
    hipfftHandle inv;
    ABACUS_TRY(get_plan(n, 1, &inv));
    prof_begin("hipfft_c2r");
    const hipfftResult r = hipfftExecC2R(inv, (hipfftComplex *)W, (hipfftReal *)W);
    prof_end("hipfft_c2r");
    return fft_check(r, "hipfftExecC2R");
}

// s2 = sum_ij w_ij s_ij(x)^2 from the padded spectrum D through the padded work mesh W; `partial` != nullptr: the last
// accumulate leaves its per-workgroup sums there (grid_rows entries)
int s2_rounds(const float *D, float *W, float *s2, int n, double Lbox, double *partial, unsigned int grid_rows) {
    const int pr = pitch_r(n), pc = pr / 2;
    MultArgs m = mult_args(n, Lbox, pc, pc, 1.0 / ((double)n * n * n));
    static const int comp[6][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}};
    for (int q = 0; q < 6; q++) {
        m.ci = comp[q][0], m.cj = comp[q][1];
        ABACUS_TRY(launch_mult(OP_SIJ, true, (const float2 *)D, (float2 *)W, m));
        ABACUS_TRY(inverse(W, n));
        const float w = m.ci == m.cj ? 1.f : 2.f;
        if (q == 0)
            ABACUS_LAUNCH("zcv_accum", (zcv_accum<true, false>), dim3(grid_rows), dim3(BLK), 0, W, s2, n, (int64_t)pr, w, partial);
        else if (q == 5 && partial)
            ABACUS_LAUNCH("zcv_accum_sum", (zcv_accum<false, true>), dim3(grid_rows), dim3(BLK), 0, W, s2, n, (int64_t)pr, w, partial);
        else
            ABACUS_LAUNCH("zcv_accum", (zcv_accum<false, false>), dim3(grid_rows), dim3(BLK), 0, W, s2, n, (int64_t)pr, w, partial);
    }
    return 0;
}

int n2_round(const float *D, float *W, float *n2, int n, double Lbox, unsigned int grid_rows) {
    const int pr = pitch_r(n), pc = pr / 2;
    const MultArgs m = mult_args(n, Lbox, pc, pc, 1.0 / ((double)n * n * n));
    ABACUS_TRY(launch_mult(OP_N2, false, (const float2 *)D, (float2 *)W, m));
    ABACUS_TRY(inverse(W, n));
    ABACUS_LAUNCH("zcv_unpad", zcv_unpad, dim3(grid_rows), dim3(BLK), 0, W, n2, n, (int64_t)pr);
    return 0;
}

}  // namespace

namespace abacus {
int zcv_release_plans() {
    for (int i = 0; i < 2; i++) {
        if (g_plan_n[i]) (void)hipfftDestroy(g_plan[i]);
        g_plan_n[i] = 0;
    }
    return 0;
}

size_t zcv_padded_bytes(int n) { return padded_bytes(n); }

// minkowski.hip: D, a padded spectrum normalised as get_field_fft normalises, times exp(-k^2 R^2 / 2) as the filter of gaussian_filter
// forms it with kcut = 1 / R (R = 0: no filter), then the C2R in place: the padded real mesh
int zcv_smooth_c2r_inplace(float *D, int n, double Lbox, double R) {
    if (R > 0) {
        const int pc = pitch_r(n) / 2;
        MultArgs m = mult_args(n, Lbox, pc, pc, 1.0);
        m.norm = (float)(2.0 / (R * R));
        if (!(m.norm > 0)) return fail("abacus_mf_smooth_spectrum_dev: R = %g is too large for the float32 filter", R);
        ABACUS_TRY(launch_mult(OP_FILTER, false, (const float2 *)D, (float2 *)D, m));
    }
    return inverse(D, n);
}

// wst.hip: the R2C in place of a padded real mesh (no normalisation), by the transform `forward` picks for the size
int zcv_r2c_inplace(float *D, int n) { return forward(D, n); }
}  // namespace abacus

extern "C" {

int abacus_zcv_filter_dev(const float *field, float *out, int n, double Lbox, double kcut) {
    ABACUS_ENTER();
    if (!field || !out) return fail("abacus_zcv_filter_dev: null argument");
    ABACUS_TRY(check_size("abacus_zcv_filter_dev", n));
    if (!(Lbox > 0) || !(kcut > 0)) return fail("abacus_zcv_filter_dev: Lbox and kcut must be positive");
    ABACUS_TRY(check_memory("zcv gaussian_filter", n, [](int m) { return padded_bytes(m); }));
    Scratch sc;
    float *D = nullptr;
    ABACUS_TRY(sc.get(&D, padded_bytes(n)));
    const int pr = pitch_r(n), pc = pr / 2;
    const unsigned int grid_rows = grid_for((int64_t)n * n, 16);
    ABACUS_LAUNCH("zcv_pad", zcv_pad, dim3(grid_rows), dim3(BLK), 0, field, D, n, (int64_t)pr);
    ABACUS_TRY(forward(D, n));
    MultArgs m = mult_args(n, Lbox, pc, pc, 1.0 / ((double)n * n * n));
    m.norm = (float)(2.0 * kcut * kcut);
    ABACUS_TRY(launch_mult(OP_FILTER, false, (const float2 *)D, (float2 *)D, m));
    ABACUS_TRY(inverse(D, n));
    ABACUS_LAUNCH("zcv_unpad", zcv_unpad, dim3(grid_rows), dim3(BLK), 0, D, out, n, (int64_t)pr);
    return 0;
}

int abacus_zcv_spectral_dev(const void *src_c64, void *dst_c64, int n, double Lbox, int op, int ci, int cj, double kcut) {
    ABACUS_ENTER();
    if (!src_c64 || !dst_c64) return fail("abacus_zcv_spectral_dev: null argument");
    if (n < 2 || n > 32767) return fail("abacus_zcv_spectral_dev: mesh size %d out of range", n);
    if (op < OP_FILTER || op > OP_SIJ) return fail("abacus_zcv_spectral_dev: unknown operator %d", op);
    if (op == OP_SIJ && (ci < 0 || ci > 2 || cj < 0 || cj > 2)) return fail("abacus_zcv_spectral_dev: component (%d, %d) out of range", ci, cj);
    if (!(Lbox > 0) || (op == OP_FILTER && !(kcut > 0))) return fail("abacus_zcv_spectral_dev: Lbox and kcut must be positive");
    const int kz = n / 2 + 1;
    MultArgs m = mult_args(n, Lbox, kz, kz, 1.0);
    if (op == OP_FILTER) m.norm = (float)(2.0 * kcut * kcut);
    m.ci = ci, m.cj = cj;
    return launch_mult(op, false, (const float2 *)src_c64, (float2 *)dst_c64, m);
}

int abacus_zcv_add_ij_dev(float *final_field, const float *field_to_add, int n, double factor) {
    ABACUS_ENTER();
    if (!final_field || !field_to_add) return fail("abacus_zcv_add_ij_dev: null argument");
    if (n < 1 || n > 32767) return fail("abacus_zcv_add_ij_dev: mesh size %d out of range", n);
    const int64_t total = (int64_t)n * n * n;
    ABACUS_LAUNCH("zcv_add_ij", zcv_add_ij, dim3(grid_for(ceil_div(total, BLK), 16)), dim3(BLK), 0, final_field, field_to_add, total,
                  (float)factor);
    return 0;
}

int abacus_zcv_dk_to_dev(const void *delta_k_c64, int n, double Lbox, int which, float *out) {
    ABACUS_ENTER();
    if (!delta_k_c64 || !out) return fail("abacus_zcv_dk_to_dev: null argument");
    ABACUS_TRY(check_size("abacus_zcv_dk_to_dev", n));
    if (which != 0 && which != 1) return fail("abacus_zcv_dk_to_dev: which = %d (0: s2, 1: nabla2)", which);
    if (!(Lbox > 0)) return fail("abacus_zcv_dk_to_dev: Lbox must be positive");
    ABACUS_TRY(check_memory("zcv get_dk_to", n, [](int m) { return 2 * padded_bytes(m); }));
    Scratch sc;
    float *D = nullptr, *W = nullptr;
    ABACUS_TRY(sc.get(&D, padded_bytes(n)));
    ABACUS_TRY(sc.get(&W, padded_bytes(n)));
    const size_t kzb = (size_t)(n / 2 + 1) * 8;
    HIP_TRY(hipMemcpy2DAsync(D, (size_t)pitch_r(n) * sizeof(float), delta_k_c64, kzb, kzb, (size_t)n * n, hipMemcpyDeviceToDevice, stream()));
    const unsigned int grid_rows = grid_for((int64_t)n * n, 16);
    if (which == 0) return s2_rounds(D, W, out, n, Lbox, nullptr, grid_rows);
    return n2_round(D, W, out, n, Lbox, grid_rows);
}

int abacus_zcv_fields_dev(const float *delta, int n, double Lbox, float *d, float *d2, float *s2, float *n2) {
    ABACUS_ENTER();
    if (!delta || !d || !d2 || !s2 || !n2) return fail("abacus_zcv_fields_dev: null argument");
    ABACUS_TRY(check_size("abacus_zcv_fields_dev", n));
    if (!(Lbox > 0)) return fail("abacus_zcv_fields_dev: Lbox must be positive");
    ABACUS_TRY(check_memory("zcv get_fields", n, [](int m) { return 2 * padded_bytes(m); }));
    Scratch sc;
    float *D = nullptr, *W = nullptr, *mean = nullptr;
    double *partial = nullptr;
    ABACUS_TRY(sc.get(&D, padded_bytes(n)));
    ABACUS_TRY(sc.get(&W, padded_bytes(n)));
    const unsigned int grid_rows = grid_for((int64_t)n * n, 16);
    ABACUS_TRY(sc.get(&partial, (size_t)3 * grid_rows * sizeof(double)));
    ABACUS_TRY(sc.get(&mean, 4 * sizeof(float)));
    const double count = (double)n * n * n;
    const int pr = pitch_r(n);
    ABACUS_LAUNCH("zcv_delta", zcv_delta, dim3(grid_rows), dim3(BLK), 0, delta, D, d2, n, pr, partial);
    ABACUS_LAUNCH("zcv_mean", zcv_mean, dim3(1), dim3(BLK), 0, partial, (int)grid_rows, 2, count, mean);
    ABACUS_TRY(forward(D, n));
    ABACUS_TRY(s2_rounds(D, W, s2, n, Lbox, partial + (size_t)2 * grid_rows, grid_rows));
    ABACUS_LAUNCH("zcv_mean", zcv_mean, dim3(1), dim3(BLK), 0, partial + (size_t)2 * grid_rows, (int)grid_rows, 1, count, mean + 2);
    ABACUS_TRY(n2_round(D, W, n2, n, Lbox, grid_rows));
    const int64_t total = (int64_t)n * n * n;
    ABACUS_LAUNCH("zcv_sub_means", zcv_sub_means, dim3(grid_for(ceil_div(total, BLK), 16)), dim3(BLK), 0, delta, d, d2, s2, total, mean);
    return 0;
}

int abacus_zcv_lattice_dev(const float *disp_x, const float *disp_y, const float *disp_z, int n, double Lbox, double D, double f_growth,
                           float *pos) {
    ABACUS_ENTER();
    if (!disp_x || !disp_y || !disp_z || !pos) return fail("abacus_zcv_lattice_dev: null argument");
    if (n < 1 || n > 32767) return fail("abacus_zcv_lattice_dev: mesh size %d out of range", n);
    if (!(Lbox > 0)) return fail("abacus_zcv_lattice_dev: Lbox must be positive");
    // `disp_z * D * (1 + f_growth)`: two float32 multiplications (the reference always does both; * float32(1) changes nothing)
    ABACUS_LAUNCH("zcv_lattice", zcv_lattice, dim3(grid_for((int64_t)n * n, 16)), dim3(BLK), 0, disp_x, disp_y, disp_z, pos, n, (float)D,
                  (float)(1.0 + f_growth), 1, (float)Lbox);
    return 0;
}

int abacus_zcv_shift_wrap_dev(float *pos, int64_t np, double Lbox) {
    ABACUS_ENTER();
    if (!pos || np < 1) return fail("abacus_zcv_shift_wrap_dev: null argument or no particles");
    if (!(Lbox > 0)) return fail("abacus_zcv_shift_wrap_dev: Lbox must be positive");
    ABACUS_LAUNCH("zcv_shift_wrap", zcv_shift_wrap, dim3(grid_for(ceil_div(3 * np, BLK), 16)), dim3(BLK), 0, pos, 3 * np, (float)(Lbox / 2.0),
                  (float)Lbox);
    return 0;
}

int abacus_zcv_spectrum_bytes(int n, uint64_t *bytes) {
    if (!bytes || n < 2 || n > 32767) return fail("abacus_zcv_spectrum_bytes: bad argument");
    *bytes = (uint64_t)padded_bytes(n);
    return 0;
}

int abacus_zcv_check_memory(int n, int nfield, int interlaced, int64_t np) {
    ABACUS_ENTER();
    ABACUS_TRY(check_size("abacus_zcv_check_memory", n));
    if (nfield < 0 || np < 0) return fail("abacus_zcv_check_memory: bad argument");
    // the spectra that stay, the work meshes of a deposit + transform (two when interlaced), positions, and the sorted line lists
    // of the deposit (about one position's worth again)
    const bool lattice = np == 0;
    return check_memory("zcv advect", n, [=](int m) {
        const size_t parts = lattice ? (size_t)m * m * m : (size_t)np;
        return (size_t)(nfield + (interlaced ? 2 : 1)) * padded_bytes(m) + parts * 24;
    });
}

int abacus_zcv_spectrum_dev(float *pos, int64_t np, const float *w, double Lbox, int n, int paste, const float *W_host, int interlaced,
                            void *out_padded) {
    ABACUS_ENTER();
    if (!pos || !out_padded || np < 1) return fail("abacus_zcv_spectrum_dev: null argument or no particles");
    return power_field_spectrum_dev(pos, np, w, Lbox, n, paste, W_host, interlaced, out_padded);
}

int abacus_zcv_advect_dev(const float *disp_x, const float *disp_y, const float *disp_z, int n, double Lbox, double D, double f_growth,
                          int nfield, const float *const *weights, int paste, const float *W_host, int interlaced, void *const *out_padded) {
    ABACUS_ENTER();
    if (!disp_x || !disp_y || !disp_z || !weights || !out_padded || nfield < 1) return fail("abacus_zcv_advect_dev: null argument");
    ABACUS_TRY(check_size("abacus_zcv_advect_dev", n));
    for (int f = 0; f < nfield; f++)
        if (!out_padded[f]) return fail("abacus_zcv_advect_dev: null output spectrum %d", f);
    Scratch sc;
    float *pos = nullptr;
    const int64_t np = (int64_t)n * n * n;
    ABACUS_TRY(sc.get(&pos, (size_t)np * 3 * sizeof(float)));
    ABACUS_TRY(abacus_zcv_lattice_dev(disp_x, disp_y, disp_z, n, Lbox, D, f_growth, pos));
    // the weight of lattice site (i, j, k) is the mesh value at (i, j, k): the mesh itself is the weight array of the n^3 particles
    for (int f = 0; f < nfield; f++)
        ABACUS_TRY(power_field_spectrum_dev(pos, np, weights[f], Lbox, n, paste, W_host, interlaced, out_padded[f]));
    return 0;
}

int abacus_zcv_power_pair(const void *a_padded, const void *b_padded, int n, double Lbox, const double *kedges, int Nk, const double *muedges,
                          int Nmu, const int64_t *poles, int Np, float *power, int64_t *N_mode, float *binned_poles, int64_t *N_mode_poles,
                          float *k_avg) {
    ABACUS_ENTER();
    if (!a_padded) return fail("abacus_zcv_power_pair: null spectrum");
    return power_bin_padded_dev(a_padded, b_padded, n, Lbox, kedges, Nk, muedges, Nmu, poles, Np, power, N_mode, binned_poles, N_mode_poles,
                                k_avg);
}

int abacus_zcv_spectrum_fetch(const void *padded, int n, void *out_c64_host) {
    ABACUS_ENTER();
    if (!padded || !out_c64_host || n < 2 || n > 32767) return fail("abacus_zcv_spectrum_fetch: bad argument");
    const size_t kzb = (size_t)(n / 2 + 1) * 8;
    HIP_TRY(hipMemcpy2DAsync(out_c64_host, kzb, padded, (size_t)pitch_r(n) * sizeof(float), kzb, (size_t)n * n, hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipStreamSynchronize(stream()));
    return 0;
}

int abacus_zcv_release(void) {
    ABACUS_ENTER();
    return zcv_release_plans();
}

// ---- linear control variates --------------------------------------------------------------------------------------------------
int abacus_lcv_linear_dev(const float *delta, int n, void *out_delta_padded, void *out_deltamu2_padded) {
    ABACUS_ENTER();
    if (!delta || !out_delta_padded || !out_deltamu2_padded) return fail("abacus_lcv_linear_dev: null argument");
    if (out_delta_padded == out_deltamu2_padded) return fail("abacus_lcv_linear_dev: the two spectra must be different buffers");
    ABACUS_TRY(check_size("abacus_lcv_linear_dev", n));
    // (the two spectra are the caller's; the transform may take a work mesh of the same size)
    ABACUS_TRY(check_memory("lcv linear_fields", n, [](int m) { return padded_bytes(m); }));
    const int pr = pitch_r(n), pc = pr / 2;
    float *Dm = static_cast<float *>(out_delta_padded);
    ABACUS_LAUNCH("zcv_pad", zcv_pad, dim3(grid_for((int64_t)n * n, 16)), dim3(BLK), 0, delta, Dm, n, (int64_t)pr);
    ABACUS_TRY(forward(Dm, n));
    const float scl = 1.0f / (float)((double)n * n * n);
    ABACUS_LAUNCH("lcv_linear", lcv_linear, dim3(grid_for(ceil_div((int64_t)n * n, LCV_ROWS), 16)), dim3(BLK), 0, (float2 *)Dm,
                  (float2 *)out_deltamu2_padded, n, pc, scl);
    return 0;
}

int abacus_lcv_spectrum_sub_dev(void *a_padded, const void *b_padded, int n) {
    ABACUS_ENTER();
    if (!a_padded || !b_padded || a_padded == b_padded) return fail("abacus_lcv_spectrum_sub_dev: null or aliased argument");
    if (n < 2 || n > 32767) return fail("abacus_lcv_spectrum_sub_dev: mesh size %d out of range", n);
    const int64_t total4 = (int64_t)(padded_bytes(n) / sizeof(float4));       // the pitch is a multiple of 32 floats
    ABACUS_LAUNCH("lcv_sub", lcv_sub, dim3(grid_for(ceil_div(total4, BLK), 16)), dim3(BLK), 0, (float4 *)a_padded, (const float4 *)b_padded,
                  total4);
    return 0;
}

int abacus_lcv_power3d(const void *a_padded, const void *b_padded, int n, float *out_host) {
    ABACUS_ENTER();
    if (!a_padded || !out_host) return fail("abacus_lcv_power3d: null argument");
    if (n < 2 || n > 32767) return fail("abacus_lcv_power3d: mesh size %d out of range", n);
    const size_t grid_bytes = (size_t)n * n * (n / 2 + 1) * sizeof(float);
    ABACUS_TRY(check_memory("lcv power3d", n, [](int m) { return (size_t)m * m * (m / 2 + 1) * sizeof(float); }));
    Scratch sc;
    float *out = nullptr;
    ABACUS_TRY(sc.get(&out, grid_bytes));
    ABACUS_LAUNCH("lcv_power3d", lcv_power3d, dim3(grid_for(ceil_div((int64_t)n * n, LCV_ROWS), 16)), dim3(BLK), 0, (const float2 *)a_padded,
                  (const float2 *)b_padded, out, n, pitch_r(n) / 2);
    HIP_TRY(hipMemcpyAsync(out_host, out, grid_bytes, hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipStreamSynchronize(stream()));
    return 0;
}

int abacus_lcv_combine_k3d(const void *delta_padded, const void *deltamu2_padded, const void *tr_padded, int n, double Lbox, double bias,
                           double f_growth, double D, double R, int reciso, float *pk_tt, float *pk_ll, float *pk_lt) {
    ABACUS_ENTER();
    if (!delta_padded || !deltamu2_padded || !tr_padded || !pk_tt || !pk_ll || !pk_lt) return fail("abacus_lcv_combine_k3d: null argument");
    if (n < 2 || n > 32767) return fail("abacus_lcv_combine_k3d: mesh size %d out of range", n);
    if (!(Lbox > 0)) return fail("abacus_lcv_combine_k3d: Lbox must be positive");
    if (reciso && !(R >= 0)) return fail("abacus_lcv_combine_k3d: reciso needs a smoothing scale R >= 0");
    const size_t grid_bytes = (size_t)n * n * (n / 2 + 1) * sizeof(float);
    ABACUS_TRY(check_memory("lcv combine_k3d", n, [](int m) { return (size_t)3 * m * m * (m / 2 + 1) * sizeof(float); }));
    Scratch sc;
    float *out[3] = {nullptr, nullptr, nullptr};
    for (auto &o : out) ABACUS_TRY(sc.get(&o, grid_bytes));
    CombineArgs m;
    m.n = n, m.pc = pitch_r(n) / 2;
    m.c_md = (float)(reciso ? 2.0 * bias : 2.0 * bias * f_growth);
    m.c_mm = (float)(f_growth * f_growth);
    m.c_dd = (float)(bias * bias);
    m.D2 = (float)(D * D);
    m.b = (float)bias, m.f = (float)f_growth, m.D = (float)D;
    const float dk = (float)(2.0 * M_PI / Lbox);
    m.dk2 = dk * dk;
    m.R2 = (float)(R * R);
    const dim3 grid(grid_for(ceil_div((int64_t)n * n, LCV_ROWS), 16)), block(BLK);
    if (reciso)
        ABACUS_LAUNCH("lcv_combine_reciso", (lcv_combine<true>), grid, block, 0, (const float2 *)delta_padded, (const float2 *)deltamu2_padded,
                      (const float2 *)tr_padded, out[0], out[1], out[2], m);
    else
        ABACUS_LAUNCH("lcv_combine", (lcv_combine<false>), grid, block, 0, (const float2 *)delta_padded, (const float2 *)deltamu2_padded,
                      (const float2 *)tr_padded, out[0], out[1], out[2], m);
    float *host[3] = {pk_tt, pk_ll, pk_lt};
    for (int i = 0; i < 3; i++) HIP_TRY(hipMemcpyAsync(host[i], out[i], grid_bytes, hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipStreamSynchronize(stream()));
    return 0;
}

// ---- BAO reconstruction --------------------------------------------------------------------------------------------------------
namespace {
int recon_check_n(const char *who, int n) {
    if (n < 2 || n > 32767) return fail("%s: mesh size %d out of range", who, n);
    if (n & 1) return fail("%s: odd mesh size %d (the displacement comes back through a real inverse transform)", who, n);
    return 0;
}
}  // namespace

int abacus_recon_check_memory(int n, int64_t np) {
    ABACUS_ENTER();
    ABACUS_TRY(recon_check_n("abacus_recon_check_memory", n));
    if (np < 0) return fail("abacus_recon_check_memory: bad argument");
    // the three displacement meshes (the density spectrum lies in the third), the work mesh of the deposit + transform, the copy of
    // the positions, the sorted line lists of the deposit (about one position's worth again) and the shifted positions
    return check_memory("recon displacement", n, [=](int m) { return (size_t)4 * padded_bytes(m) + (size_t)np * 36; });
}

int abacus_recon_pack_soa64_dev(const double *x, const double *y, const double *z, int64_t np, double offset, float *out) {
    ABACUS_ENTER();
    if (!x || !y || !z || !out || np < 1) return fail("abacus_recon_pack_soa64_dev: null argument or no particles");
    if (!std::isfinite(offset)) return fail("abacus_recon_pack_soa64_dev: offset must be finite");
    ABACUS_LAUNCH("recon_pack_soa64", recon_pack_soa64, dim3(grid_for(ceil_div(np, BLK), 16)), dim3(BLK), 0, x, y, z, out, np,
                  (double)(float)offset);
    return 0;
}

int abacus_recon_wrap_dev(const float *pos, int64_t np, double offset, double Lbox, float *out) {
    ABACUS_ENTER();
    if (!pos || !out || np < 1) return fail("abacus_recon_wrap_dev: null argument or no particles");
    if (!(Lbox > 0) || !std::isfinite(Lbox) || !std::isfinite(offset)) return fail("abacus_recon_wrap_dev: Lbox must be positive, offset finite");
    ABACUS_LAUNCH("recon_wrap", recon_wrap, dim3(grid_for(ceil_div(3 * np, BLK), 16)), dim3(BLK), 0, pos, out, 3 * np, (float)offset,
                  (float)Lbox);
    return 0;
}

int abacus_recon_pad_dev(const float *mesh, int n, float *out_padded) {
    ABACUS_ENTER();
    if (!mesh || !out_padded) return fail("abacus_recon_pad_dev: null argument");
    ABACUS_TRY(recon_check_n("abacus_recon_pad_dev", n));
    ABACUS_LAUNCH("zcv_pad", zcv_pad, dim3(grid_for((int64_t)n * n, 16)), dim3(BLK), 0, mesh, out_padded, n, (int64_t)pitch_r(n));
    return 0;
}

int abacus_recon_delta_dev(const float *delta, int n, void *out_padded) {
    ABACUS_ENTER();
    if (!delta || !out_padded) return fail("abacus_recon_delta_dev: null argument");
    ABACUS_TRY(recon_check_n("abacus_recon_delta_dev", n));
    // (the spectrum is the caller's; the transform may take a work mesh of the same size)
    ABACUS_TRY(check_memory("recon delta", n, [](int m) { return padded_bytes(m); }));
    float *Dm = static_cast<float *>(out_padded);
    ABACUS_LAUNCH("zcv_pad", zcv_pad, dim3(grid_for((int64_t)n * n, 16)), dim3(BLK), 0, delta, Dm, n, (int64_t)pitch_r(n));
    return forward(Dm, n);
}

int abacus_recon_displacement_dev(const void *delta_padded, int normalised, int n, double Lbox, double bias, double f_growth, double R, int rsd,
                                  float *psi_x, float *psi_y, float *psi_z) {
    ABACUS_ENTER();
    if (!delta_padded || !psi_x || !psi_y || !psi_z) return fail("abacus_recon_displacement_dev: null argument");
    if (psi_x == psi_y || psi_x == psi_z || psi_y == psi_z || delta_padded == psi_x || delta_padded == psi_y)
        return fail("abacus_recon_displacement_dev: the three meshes must be different buffers (the spectrum may lie in psi_z only)");
    ABACUS_TRY(recon_check_n("abacus_recon_displacement_dev", n));
    if (!(Lbox > 0) || !std::isfinite(Lbox)) return fail("abacus_recon_displacement_dev: Lbox must be positive");
    if (!(bias > 0) || !std::isfinite(bias)) return fail("abacus_recon_displacement_dev: bias must be positive");
    if (!(f_growth >= 0) || !std::isfinite(f_growth)) return fail("abacus_recon_displacement_dev: f_growth must not be negative");
    if (!(R >= 0) || !std::isfinite(R)) return fail("abacus_recon_displacement_dev: the smoothing scale R must not be negative");
    // (the meshes are the caller's; the inverse transform may take a work mesh of the same size)
    ABACUS_TRY(check_memory("recon displacement", n, [](int m) { return padded_bytes(m); }));
    ReconArgs m;
    m.n = n, m.pc = pitch_r(n) / 2;
    m.dk = (float)(2.0 * M_PI / Lbox);
    m.R2h = (float)(R * R / 2.0);
    m.b = (float)bias;
    m.beta = rsd ? (float)(f_growth / bias) : 0.0f;
    m.scale = normalised ? 1.0f : (float)(1.0 / ((double)n * n * n));
    ABACUS_LAUNCH("recon_mult", recon_mult, dim3(grid_for(ceil_div((int64_t)n * n, LCV_ROWS), 16)), dim3(BLK), 0, (const float2 *)delta_padded,
                  (float2 *)psi_x, (float2 *)psi_y, (float2 *)psi_z, m);
    ABACUS_TRY(inverse(psi_x, n));
    ABACUS_TRY(inverse(psi_y, n));
    return inverse(psi_z, n);
}

int abacus_recon_shift_dev(const float *pos, int64_t np, double offset, const float *psi_x, const float *psi_y, const float *psi_z, int n,
                           double Lbox, int paste, double los_factor, float *out) {
    ABACUS_ENTER();
    if (!pos || !psi_x || !psi_y || !psi_z || !out || np < 1) return fail("abacus_recon_shift_dev: null argument or no particles");
    if (pos == out) return fail("abacus_recon_shift_dev: out must not be pos");
    ABACUS_TRY(recon_check_n("abacus_recon_shift_dev", n));
    if (paste != 0 && paste != 1) return fail("abacus_recon_shift_dev: paste = %d (0: TSC, 1: CIC)", paste);
    if (!(Lbox > 0) || !std::isfinite(Lbox)) return fail("abacus_recon_shift_dev: Lbox must be positive");
    if (!std::isfinite(offset) || !std::isfinite(los_factor)) return fail("abacus_recon_shift_dev: offset and los_factor must be finite");
    const dim3 grid(grid_for(ceil_div(np, BLK), 32)), block(BLK);
    const float L = (float)Lbox, inv_h = (float)((double)n / Lbox);
    if (paste == 1)
        ABACUS_LAUNCH("recon_shift_cic", (recon_shift<2>), grid, block, 0, pos, np, (float)offset, psi_x, psi_y, psi_z, n, (int64_t)pitch_r(n), L,
                      inv_h, (float)los_factor, out);
    else
        ABACUS_LAUNCH("recon_shift_tsc", (recon_shift<3>), grid, block, 0, pos, np, (float)offset, psi_x, psi_y, psi_z, n, (int64_t)pitch_r(n), L,
                      inv_h, (float)los_factor, out);
    return 0;
}

}  // extern "C"

// ---- light-cone power spectrum multipoles: FKP field and Yamamoto estimator (analysis/lc_power.py).  No reference code: the
// arithmetic is stated in include/abacus_hip.h and pinned to tests/lc_power_statement.py.  F = D - alpha R, the raw weighted deposits of
// data and randoms in a box the randoms fix, lies in a padded real mesh.  F_0(k) = R2C(F); for l = 2, 4 and every m:
// [lc_ylm_mult: work = S_lm(r^ of the cell) F, 4 B in + 4 B out per cell] -> R2C in place -> [lc_ylm_accum: F_l(k) (+)= S_lm(k^) work(k),
// the first m writes].  Both streaming kernels give one (i, j) row to a wave, so two of the three coordinates are uniform over the
// wave, and 16 B to a lane and step.  The spectra are binned by power_bin_padded_dev.
namespace {

struct LcGeom {
    int n, pitch;          // cells per side, floats per padded row
    float cx, cy, cz, h;   // corner of the box seen from the observer, cell size; cell i is centred at c + i h
};

constexpr float LC_SQRT3 = 1.7320508075688772f, LC_SQRT5 = 2.23606797749979f, LC_SQRT10 = 3.1622776601683795f,
                LC_SQRT35 = 5.916079783099616f, LC_SQRT70 = 8.366600265340756f;

// the real harmonics of the direction of (x, y, z), scaled so that sum_m S_lm(a) S_lm(b) = L_l(a . b); lm = 0 .. 4: l = 2, lm = 5 .. 13:
// l = 4 (lm is uniform over the launch: a scalar branch).  Every S_lm of even l is a homogeneous polynomial of even degree in the unit
// vector: products of two components times inv2 = 1 / |r|^2, no square root
__device__ __forceinline__ float lc_ylm(int lm, float x, float y, float z, float inv2) {
    const float u = (x * x) * inv2, v = (y * y) * inv2, w = (z * z) * inv2;
    switch (lm) {
    case 0: return 0.5f * (3.0f * w - 1.0f);
    case 1: return LC_SQRT3 * ((x * z) * inv2);
    case 2: return LC_SQRT3 * ((y * z) * inv2);
    case 3: return (0.5f * LC_SQRT3) * (u - v);
    case 4: return LC_SQRT3 * ((x * y) * inv2);
    case 5: return 0.125f * ((35.0f * w - 30.0f) * w + 3.0f);
    case 6: return (0.25f * LC_SQRT10) * (((x * z) * inv2) * (7.0f * w - 3.0f));
    case 7: return (0.25f * LC_SQRT10) * (((y * z) * inv2) * (7.0f * w - 3.0f));
    case 8: return (0.25f * LC_SQRT5) * ((u - v) * (7.0f * w - 1.0f));
    case 9: return (0.5f * LC_SQRT5) * (((x * y) * inv2) * (7.0f * w - 1.0f));
    case 10: return (0.25f * LC_SQRT70) * (((x * z) * inv2) * (u - 3.0f * v));
    case 11: return (0.25f * LC_SQRT70) * (((y * z) * inv2) * (3.0f * u - v));
    case 12: return (0.125f * LC_SQRT35) * ((u * u - 6.0f * (u * v)) + v * v);
    default: return (0.5f * LC_SQRT35) * (((x * y) * inv2) * (u - v));
    }
}

// S_lm of the direction of (x, y, z); 0 for the zero vector.  The hardware reciprocal (1 ulp) stands for the division.
__device__ __forceinline__ float lc_ylm_dir(int lm, float x, float y, float z) {
    const float r2 = x * x + y * y + z * z;
    if (!(r2 > 0.0f)) return 0.0f;
    return lc_ylm(lm, x, y, z, __builtin_amdgcn_rcpf(r2));
}

constexpr int LC_WAVES = BLK / 64;

// work = S_lm(r^_cell) F on padded real meshes: one (i, j) row per wave, four consecutive z cells per lane and step.  The pad cells of
// a row that a 16-byte access touches are written as 0.
__global__ __launch_bounds__(BLK) void lc_ylm_mult(const float *__restrict__ F, float *__restrict__ work, LcGeom g, int lm) {
    const int n = g.n, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t rows = (int64_t)n * n;
    for (int64_t row = (int64_t)blockIdx.x * LC_WAVES + wave; row < rows; row += (int64_t)gridDim.x * LC_WAVES) {
        const int i = (int)(row / n), j = (int)(row % n);
        const float x = g.cx + (float)i * g.h, y = g.cy + (float)j * g.h;
        const float4 *src = reinterpret_cast<const float4 *>(F + row * g.pitch);
        float4 *dst = reinterpret_cast<float4 *>(work + row * g.pitch);
        for (int c4 = lane; 4 * c4 < n; c4 += 64) {       // 4 c4 + 3 <= n + 1 < pitch: inside the row
            const float4 v = src[c4];
            const float in[4] = {v.x, v.y, v.z, v.w};
            float o[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int k = 4 * c4 + q;
                const float z = g.cz + (float)k * g.h;
                o[q] = k < n ? lc_ylm_dir(lm, x, y, z) * in[q] : 0.0f;
            }
            dst[c4] = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
}

// out (+)= S_lm(k^) work over padded spectra: one (a, b) row per wave, two consecutive modes per lane and step.  k^ from the mode
// numbers (a and b folded, c = 0 .. n/2): the direction does not depend on dk.  FIRST writes, pad modes as 0.
template <bool FIRST>
__global__ __launch_bounds__(BLK) void lc_ylm_accum(const float4 *__restrict__ work, float4 *__restrict__ out, int n, int pitch4, int lm) {
    const int kzlen = n / 2 + 1, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t rows = (int64_t)n * n;
    for (int64_t row = (int64_t)blockIdx.x * LC_WAVES + wave; row < rows; row += (int64_t)gridDim.x * LC_WAVES) {
        const float kx = (float)fold((int)(row / n), n), ky = (float)fold((int)(row % n), n);
        for (int c4 = lane; 2 * c4 < kzlen; c4 += 64) {   // 2 c4 + 1 <= n/2 + 1 < pitch / 2: inside the row
            const int c = 2 * c4;
            const bool two = c + 1 < kzlen;
            const int64_t q = row * pitch4 + c4;
            const float4 w = work[q];
            const float s0 = lc_ylm_dir(lm, kx, ky, (float)c);
            const float s1 = two ? lc_ylm_dir(lm, kx, ky, (float)(c + 1)) : 0.0f;
            float4 t = make_float4(s0 * w.x, s0 * w.y, two ? s1 * w.z : 0.0f, two ? s1 * w.w : 0.0f);
            if (!FIRST) {
                const float4 p = out[q];
                t.x += p.x, t.y += p.y, t.z += p.z, t.w += p.w;
            }
            out[q] = t;
        }
    }
}

// extent of three float32 columns, first stage: partial[q * gridDim.x + block], q = 0 .. 2 the minima of x, y, z, 3 .. 5 the maxima.  A
// coordinate that is not finite makes its axis' extent (-inf, +inf).  Minima and maxima do not depend on the order: no atomics needed.
__global__ __launch_bounds__(BLK) void lc_extent(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z, int64_t np,
                                                 float *__restrict__ partial) {
    __shared__ float lds[6][BLK];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t p = (int64_t)blockIdx.x * BLK + threadIdx.x; p < np; p += (int64_t)gridDim.x * BLK) {
        const float v[3] = {x[p], y[p], z[p]};
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const bool ok = fabsf(v[a]) < INFINITY;          // false for inf and nan
            lo[a] = ok ? fminf(lo[a], v[a]) : -INFINITY;
            hi[a] = ok ? fmaxf(hi[a], v[a]) : INFINITY;
        }
    }
    for (int a = 0; a < 3; a++) lds[a][threadIdx.x] = lo[a], lds[3 + a][threadIdx.x] = hi[a];
    __syncthreads();
    for (int s = BLK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int a = 0; a < 3; a++) {
                lds[a][threadIdx.x] = fminf(lds[a][threadIdx.x], lds[a][threadIdx.x + s]);
                lds[3 + a][threadIdx.x] = fmaxf(lds[3 + a][threadIdx.x], lds[3 + a][threadIdx.x + s]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 6) partial[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = lds[threadIdx.x][0];
}

// second stage: one workgroup over the partials
__global__ __launch_bounds__(BLK) void lc_extent_final(const float *__restrict__ partial, int npart, float *__restrict__ out) {
    __shared__ float lds[BLK];
    for (int q = 0; q < 6; q++) {
        float v = q < 3 ? INFINITY : -INFINITY;
        for (int i = threadIdx.x; i < npart; i += BLK) v = q < 3 ? fminf(v, partial[(int64_t)q * npart + i]) : fmaxf(v, partial[(int64_t)q * npart + i]);
        lds[threadIdx.x] = v;
        __syncthreads();
        for (int s = BLK / 2; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) lds[threadIdx.x] = q < 3 ? fminf(lds[threadIdx.x], lds[threadIdx.x + s]) : fmaxf(lds[threadIdx.x], lds[threadIdx.x + s]);
            __syncthreads();
        }
        if (threadIdx.x == 0) out[q] = lds[0];
        __syncthreads();
    }
}

// three float32 columns -> (np, 3) float32, the corner subtracted in float32: the copy a deposit may sort and wrap
__global__ __launch_bounds__(BLK) void lc_pack(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z, int64_t np,
                                               float cx, float cy, float cz, float *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < np; i += (int64_t)gridDim.x * BLK) {
        out[3 * i] = x[i] - cx;
        out[3 * i + 1] = y[i] - cy;
        out[3 * i + 2] = z[i] - cz;
    }
}

// dst += a * src over whole padded meshes (the pad columns ride along)
__global__ __launch_bounds__(BLK) void lc_axpy(float4 *__restrict__ dst, const float4 *__restrict__ src, int64_t total4, float a) {
    for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < total4; i += (int64_t)gridDim.x * BLK) {
        float4 d = dst[i];
        const float4 s = src[i];
        d.x += a * s.x, d.y += a * s.y, d.z += a * s.z, d.w += a * s.w;
        dst[i] = d;
    }
}

// spectrum *= 1 / ((W[a] W[b]) W[c]), the product and the reciprocal in float32 as get_field_fft forms them
__global__ __launch_bounds__(BLK) void lc_compensate(float2 *__restrict__ spec, int n, int pc, const float *__restrict__ W) {
    lcv_for_each_mode(n, pc, [&](int row, int c) {
        const int64_t q = (int64_t)row * pc + c;
        const float scl = 1.0f / ((W[row / n] * W[row % n]) * W[c]);
        const float2 v = spec[q];
        spec[q] = make_float2(v.x * scl, v.y * scl);
    });
}

// first stage of sum_i w_i^2 nbar_i in float64 (w == nullptr: unit weights): one partial per workgroup, summed in a fixed order
template <class T>
__global__ __launch_bounds__(BLK) void lc_sum_w2n(const float *__restrict__ w, const T *__restrict__ nbar, int64_t np, double *__restrict__ partial) {
    __shared__ double lds[BLK];
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < np; i += (int64_t)gridDim.x * BLK) {
        const double wi = w ? (double)w[i] : 1.0;
        s += (wi * wi) * (double)nbar[i];
    }
    const double t = block_sum(s, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// second stage: one workgroup, out[0] = sum of the partials
__global__ __launch_bounds__(BLK) void lc_sum_final(const double *__restrict__ partial, int npart, double *__restrict__ out) {
    __shared__ double lds[BLK];
    double s = 0.0;
    for (int i = threadIdx.x; i < npart; i += BLK) s += partial[i];
    const double t = block_sum(s, lds);
    if (threadIdx.x == 0) out[0] = t;
}

int lc_check_n(const char *who, int n) {
    if (n < 2 || n > 32767) return fail("%s: mesh size %d out of range", who, n);
    if (n & 1) return fail("%s: odd mesh size %d (the half spectrum and its Nyquist plane are laid out for an even mesh)", who, n);
    return 0;
}

}  // namespace

namespace abacus {
int tsc_deposit_f32(float *pos, int64_t n, const float *w, float *grid, int nmesh, int64_t zstride, double box, double offset, int wrap,
                    double norm, int cic, int list_mode, double sub, int zero_grid);
}

extern "C" {

int abacus_lc_check_memory(int n, int nmeshes, int64_t np) {
    ABACUS_ENTER();
    ABACUS_TRY(lc_check_n("abacus_lc_check_memory", n));
    if (nmeshes < 0 || np < 0) return fail("abacus_lc_check_memory: bad argument");
    // the padded meshes still to be allocated, the packed copies of the particles and their weights, and the lists of the deposit
    // (about one position's worth again)
    return check_memory("light-cone power", n, [=](int m) { return (size_t)nmeshes * padded_bytes(m) + (size_t)np * 28; });
}

int abacus_lc_extent_dev(const float *x, const float *y, const float *z, int64_t np, float *lohi_host) {
    ABACUS_ENTER();
    if (!x || !y || !z || !lohi_host || np < 1) return fail("abacus_lc_extent_dev: null argument or no points");
    Scratch sc;
    float *partial = nullptr, *out = nullptr;
    const unsigned int grid = grid_for(ceil_div(np, (int64_t)BLK * 8), 4);
    ABACUS_TRY(sc.get(&partial, (size_t)6 * grid * sizeof(float)));
    ABACUS_TRY(sc.get(&out, 6 * sizeof(float)));
    ABACUS_LAUNCH("lc_extent", lc_extent, dim3(grid), dim3(BLK), 0, x, y, z, np, partial);
    ABACUS_LAUNCH("lc_extent_final", lc_extent_final, dim3(1), dim3(BLK), 0, (const float *)partial, (int)grid, out);
    HIP_TRY(hipMemcpyAsync(lohi_host, out, 6 * sizeof(float), hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipStreamSynchronize(stream()));
    return 0;
}

int abacus_lc_pack_dev(const float *x, const float *y, const float *z, int64_t np, const double *corner, float *out) {
    ABACUS_ENTER();
    if (!x || !y || !z || !corner || !out || np < 1) return fail("abacus_lc_pack_dev: null argument or no points");
    for (int a = 0; a < 3; a++)
        if (!std::isfinite(corner[a])) return fail("abacus_lc_pack_dev: the corner must be finite");
    ABACUS_LAUNCH("lc_pack", lc_pack, dim3(grid_for(ceil_div(np, BLK), 16)), dim3(BLK), 0, x, y, z, np, (float)corner[0], (float)corner[1],
                  (float)corner[2], out);
    return 0;
}

int abacus_lc_deposit_dev(float *pos, int64_t np, const float *w, double Lbox, int n, int paste, float *mesh_padded) {
    ABACUS_ENTER();
    if (!pos || !mesh_padded || np < 1) return fail("abacus_lc_deposit_dev: null argument or no points");
    ABACUS_TRY(lc_check_n("abacus_lc_deposit_dev", n));
    if (paste != 0 && paste != 1) return fail("abacus_lc_deposit_dev: paste = %d (0: TSC, 1: CIC)", paste);
    if (!(Lbox > 0) || !std::isfinite(Lbox)) return fail("abacus_lc_deposit_dev: Lbox must be positive");
    // norm = 0: the weight per cell as deposited, no normalisation; every cell of the mesh is written
    return tsc_deposit_f32(pos, np, w, mesh_padded, n, pitch_r(n), Lbox, 0.0, paste == 0, 0.0, paste, 0, 0.0, 1);
}

int abacus_lc_axpy_dev(float *dst_padded, const float *src_padded, int n, double a) {
    ABACUS_ENTER();
    if (!dst_padded || !src_padded || dst_padded == src_padded) return fail("abacus_lc_axpy_dev: null or aliased argument");
    ABACUS_TRY(lc_check_n("abacus_lc_axpy_dev", n));
    if (!std::isfinite(a)) return fail("abacus_lc_axpy_dev: the factor must be finite");
    const int64_t total4 = (int64_t)(padded_bytes(n) / sizeof(float4));       // the pitch is a multiple of 32 floats
    ABACUS_LAUNCH("lc_axpy", lc_axpy, dim3(grid_for(ceil_div(total4, BLK), 16)), dim3(BLK), 0, (float4 *)dst_padded, (const float4 *)src_padded,
                  total4, (float)a);
    return 0;
}

int abacus_lc_multipole_dev(const float *F_padded, int n, double Lbox, const double *corner, int ell, float *work_padded, void *out_padded) {
    ABACUS_ENTER();
    if (!F_padded || !corner || !out_padded) return fail("abacus_lc_multipole_dev: null argument");
    ABACUS_TRY(lc_check_n("abacus_lc_multipole_dev", n));
    if (ell != 0 && ell != 2 && ell != 4) return fail("abacus_lc_multipole_dev: multipole %d (0, 2 or 4)", ell);
    if (!(Lbox > 0) || !std::isfinite(Lbox)) return fail("abacus_lc_multipole_dev: Lbox must be positive");
    for (int a = 0; a < 3; a++)
        if (!std::isfinite(corner[a])) return fail("abacus_lc_multipole_dev: the corner must be finite");
    if (F_padded == out_padded || (ell && (!work_padded || work_padded == F_padded || (void *)work_padded == out_padded)))
        return fail("abacus_lc_multipole_dev: F, the work mesh and the output must be different buffers");
    // (the meshes are the caller's; the transform may take a work mesh of the same size)
    ABACUS_TRY(check_memory("light-cone power", n, [](int m) { return padded_bytes(m); }));
    if (ell == 0) {
        HIP_TRY(hipMemcpyAsync(out_padded, F_padded, padded_bytes(n), hipMemcpyDeviceToDevice, stream()));
        return forward(static_cast<float *>(out_padded), n);
    }
    LcGeom g;
    g.n = n, g.pitch = pitch_r(n);
    g.cx = (float)corner[0], g.cy = (float)corner[1], g.cz = (float)corner[2];
    g.h = (float)(Lbox / n);
    const int lm0 = ell == 2 ? 0 : 5;
    const dim3 grid(grid_for(ceil_div((int64_t)n * n, LC_WAVES), 16)), block(BLK);
    for (int m = 0; m < 2 * ell + 1; m++) {
        ABACUS_LAUNCH("lc_ylm_mult", lc_ylm_mult, grid, block, 0, F_padded, work_padded, g, lm0 + m);
        ABACUS_TRY(forward(work_padded, n));
        if (m == 0)
            ABACUS_LAUNCH("lc_ylm_accum", (lc_ylm_accum<true>), grid, block, 0, (const float4 *)work_padded, (float4 *)out_padded, n, g.pitch / 4, lm0 + m);
        else
            ABACUS_LAUNCH("lc_ylm_accum", (lc_ylm_accum<false>), grid, block, 0, (const float4 *)work_padded, (float4 *)out_padded, n, g.pitch / 4, lm0 + m);
    }
    return 0;
}

int abacus_lc_compensate_dev(void *spec_padded, int n, const float *W_host) {
    ABACUS_ENTER();
    if (!spec_padded || !W_host) return fail("abacus_lc_compensate_dev: null argument");
    ABACUS_TRY(lc_check_n("abacus_lc_compensate_dev", n));
    Scratch sc;
    float *W = nullptr;
    ABACUS_TRY(sc.get(&W, (size_t)n * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(W, W_host, (size_t)n * sizeof(float), hipMemcpyHostToDevice, stream()));
    ABACUS_LAUNCH("lc_compensate", lc_compensate, dim3(grid_for(ceil_div((int64_t)n * n, LCV_ROWS), 16)), dim3(BLK), 0, (float2 *)spec_padded, n,
                  pitch_r(n) / 2, (const float *)W);
    HIP_TRY(hipStreamSynchronize(stream()));        // W_host is the caller's
    return 0;
}

int abacus_lc_sum_w2n_dev(const float *w, const void *nbar, int nbar_f64, int64_t np, double *out_host) {
    ABACUS_ENTER();
    if (!nbar || !out_host || np < 1) return fail("abacus_lc_sum_w2n_dev: null argument or no points");
    Scratch sc;
    double *partial = nullptr;
    const unsigned int grid = grid_for(ceil_div(np, (int64_t)BLK * 8), 4);
    ABACUS_TRY(sc.get(&partial, (size_t)(grid + 1) * sizeof(double)));
    if (nbar_f64)
        ABACUS_LAUNCH("lc_sum_w2n", (lc_sum_w2n<double>), dim3(grid), dim3(BLK), 0, w, (const double *)nbar, np, partial);
    else
        ABACUS_LAUNCH("lc_sum_w2n", (lc_sum_w2n<float>), dim3(grid), dim3(BLK), 0, w, (const float *)nbar, np, partial);
    ABACUS_LAUNCH("lc_sum_final", lc_sum_final, dim3(1), dim3(BLK), 0, (const double *)partial, (int)grid, partial + grid);
    HIP_TRY(hipMemcpyAsync(out_host, partial + grid, sizeof(double), hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipStreamSynchronize(stream()));
    return 0;
}

}  // extern "C"

// ---- bispectrum of a periodic box: the FFT estimator of Scoccimarro 2015 (analysis/bispectrum.py).  No reference code: the arithmetic
// is stated in include/abacus_hip.h and pinned to tests/bispectrum_statement.py.  A finished padded spectrum ->
// [bk_shell_mask: every mode read once, written to the mesh of its shell and as 0 to the others, 8 + 8 nb bytes per mode] -> nb C2R in
// place -> [bk_triple: T[i][j][l] = sum_x D_i D_j D_l and G[i] = sum_x D_i^2 over the padded real meshes on the f32 matrix cores,
// float64 partial sums per workgroup] -> [bk_triple_final: the partials added in a fixed order].  No floating-point atomics.
namespace {

constexpr int BK_MAX_SHELLS = 32;
constexpr int BK_TILE = 16;              // rows and columns of one v_mfma_f32_16x16x4_f32 tile
constexpr int BK_CHUNK = 16;             // cells of a row one wave step covers: a 16 B load per lane, four MFMA k-slices of four cells
// products an accumulator sums in float32 (the K of its MFMA chain) before it is added to its float64 sum.  At most 1024, where the error
// of an f32 chain is still 1e-7 of sum |a b|; 128 because the triangle sums cancel: in bins of few triangles sum |a b| is thousands of
// times the sum, and the noise of a chain grows with its length (tests/bispectrum_statement.py FLUSH_CELLS: B of such a bin is off by
// 3.5e-4 of the largest B at 1024 and by 2e-5 at 128, n = 24).  A flush is 64 conversions and additions against 512 MFMAs.
constexpr int BK_FLUSH_CELLS = 128;
constexpr int BK_FLUSH_CHUNKS = BK_FLUSH_CELLS / BK_CHUNK;
constexpr int BK_WAVES = BLK / 64;
constexpr int BK_GROUP_OUT = BK_TILE * 4 * 64;   // accumulator values of one tile group: 16 tiles x 4 registers x 64 lanes
constexpr int BK_MAX_GROUPS = 4;
// tile groups (block of i, of j, of l) for nb > 16: the block triples in ascending order; the host fills the rest by symmetry
__constant__ int bk_groups[BK_MAX_GROUPS][3] = {{0, 0, 0}, {0, 0, 1}, {0, 1, 1}, {1, 1, 1}};
const int bk_groups_host[BK_MAX_GROUPS][3] = {{0, 0, 0}, {0, 0, 1}, {0, 1, 1}, {1, 1, 1}};

struct BkEdges {
    float e[BK_MAX_SHELLS + 1];
};

typedef float bk_acc __attribute__((ext_vector_type(4)));

// the shell of the mode with squared mode number m2: e[b] <= dk sqrt(float32(m2)) < e[b + 1] in float32, -1 outside the edges
__device__ __forceinline__ int bk_shell(const BkEdges &ed, int nb, float dk, int m2) {
    const float k = dk * __fsqrt_rn((float)m2);
    if (!(k >= ed.e[0]) || !(k < ed.e[nb])) return -1;
    int b = 0;
    while (k >= ed.e[b + 1]) b++;
    return b;
}

// nb padded spectra from one: mesh b holds the mode (ONES: 1) inside shell b and 0 elsewhere.  One (a, b) row per wave, two
// consecutive modes (16 B) per lane and step; the floats of a row beyond its n/2 + 1 modes are not written.
template <bool ONES>
__global__ __launch_bounds__(BLK) void bk_shell_mask(const float4 *__restrict__ spec, float *const *__restrict__ out, BkEdges ed, int nb, int n,
                                                     int pitch4, float dk) {
    const int kzlen = n / 2 + 1, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t rows = (int64_t)n * n;
    for (int64_t row = (int64_t)blockIdx.x * BK_WAVES + wave; row < rows; row += (int64_t)gridDim.x * BK_WAVES) {
        const int a = fold((int)(row / n), n), b = fold((int)(row % n), n);
        const int ab2 = a * a + b * b;
        for (int c4 = lane; 2 * c4 < kzlen; c4 += 64) {   // 2 c4 + 1 <= n/2 + 1 < pitch / 2: inside the row
            const int c = 2 * c4;
            const bool two = c + 1 < kzlen;
            const int64_t q = row * pitch4 + c4;
            const float4 v = ONES ? make_float4(1.0f, 0.0f, 1.0f, 0.0f) : spec[q];
            const int s0 = bk_shell(ed, nb, dk, ab2 + c * c);
            const int s1 = two ? bk_shell(ed, nb, dk, ab2 + (c + 1) * (c + 1)) : -1;
            for (int m = 0; m < nb; m++) {
                float4 *dst = reinterpret_cast<float4 *>(out[m]) + q;
                const float4 t = make_float4(m == s0 ? v.x : 0.0f, m == s0 ? v.y : 0.0f, m == s1 ? v.z : 0.0f, m == s1 ? v.w : 0.0f);
                if (two)
                    *dst = t;
                else
                    *reinterpret_cast<float2 *>(dst) = make_float2(t.x, t.y);
            }
        }
    }
}

// T[i][j][l] = sum_x D_i(x) D_j(x) D_l(x) as a GEMM on v_mfma_f32_16x16x4_f32: S[(i, j)][l] = sum_x (D_i D_j)(x) D_l(x).  Lane
// (r = lane % 16, k = lane / 16) of a wave loads four consecutive cells 16 s + 4 k .. + 3 of mesh r (16 B); for each of the four,
// its value is the B operand B[k][l = r] as it stands, and the A operand of tile i, A[j = r][k] = D_i(x_k) D_j(x_k), is that value
// times the one lane (i, k) holds (ds_bpermute).  Tile i accumulates C_i[j][l] in four registers: 16 tiles for up to 16 meshes, no LDS
// staging.  Beyond 16 meshes (ONE = false) blockIdx.y picks a tile group (bk_groups): the blocks of 16 meshes i, j and l come from.
// A wave owns a contiguous range of the 16-cell chunks of the rows; the cells of a chunk at and beyond n (the pad columns) enter as 0.
// After BK_FLUSH_CHUNKS chunks (K = BK_FLUSH_CELLS products per accumulator) the accumulators are added to float64 sums in registers
// and cleared.  The waves of a workgroup add their sums in LDS in wave order; partial[(group, workgroup)][tile][register][lane], and
// for the diagonal groups partial_g[(group, workgroup)][r] = sum_x D_r^2 the same way.
template <bool ONE>
__global__ __launch_bounds__(BLK) void bk_triple(const float *const *__restrict__ meshes, int nb, int n, int pitch, double *__restrict__ partial,
                                                 double *__restrict__ partial_g) {
    __shared__ double lds[BK_GROUP_OUT];
    __shared__ double lds_g[BK_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, kq = lane >> 4;
    const int group = blockIdx.y;
    const int ib = bk_groups[group][0], jb = bk_groups[group][1], lb = bk_groups[group][2];
    const int ni = min(BK_TILE, nb - BK_TILE * ib);
    const float *mi = BK_TILE * ib + r < nb ? meshes[BK_TILE * ib + r] : nullptr;
    const float *mj = BK_TILE * jb + r < nb ? meshes[BK_TILE * jb + r] : nullptr;
    const float *ml = BK_TILE * lb + r < nb ? meshes[BK_TILE * lb + r] : nullptr;
    const bool diag = ib == lb;      // (then jb is the same block too)

    const int per_row = (n + BK_CHUNK - 1) / BK_CHUNK;
    const int64_t nchunk = (int64_t)n * n * per_row, nwave = (int64_t)gridDim.x * BK_WAVES;
    const int64_t per = (nchunk + nwave - 1) / nwave, c0 = min(nchunk, ((int64_t)blockIdx.x * BK_WAVES + wave) * per), c1 = min(nchunk, c0 + per);
    int64_t row = c0 / per_row;
    int s = (int)(c0 % per_row);

    bk_acc acc[BK_TILE];
    double sum[BK_TILE][4];
#pragma unroll
    for (int t = 0; t < BK_TILE; t++) {
        acc[t] = bk_acc{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int e = 0; e < 4; e++) sum[t][e] = 0.0;
    }
    float g = 0.0f;
    double gsum = 0.0;
    int pending = 0;
    const int src = (lane & 48) << 2;      // byte address of lane (0, k) for ds_bpermute

    auto load = [&](const float *m, int64_t off, int cell) {
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (m) {                           // 16 s + 4 k + 3 < 16 per_row <= pitch: inside the row
            v = *reinterpret_cast<const float4 *>(m + off);
            v.x = cell < n ? v.x : 0.0f, v.y = cell + 1 < n ? v.y : 0.0f, v.z = cell + 2 < n ? v.z : 0.0f, v.w = cell + 3 < n ? v.w : 0.0f;
        }
        return v;
    };
    auto flush = [&] {
#pragma unroll
        for (int t = 0; t < BK_TILE; t++) {
#pragma unroll
            for (int e = 0; e < 4; e++) sum[t][e] += (double)acc[t][e];
            acc[t] = bk_acc{0.0f, 0.0f, 0.0f, 0.0f};
        }
        gsum += (double)g;
        g = 0.0f;
        pending = 0;
    };

    for (int64_t c = c0; c < c1; c++) {
        const int cell = BK_CHUNK * s + 4 * kq;
        const int64_t off = row * pitch + cell;
        const float4 vj = load(mj, off, cell);
        const float4 vl = ONE ? vj : load(ml, off, cell);
        const float4 vi = ONE ? vj : load(mi, off, cell);
        const float bj[4] = {vj.x, vj.y, vj.z, vj.w}, bl[4] = {vl.x, vl.y, vl.z, vl.w}, bi[4] = {vi.x, vi.y, vi.z, vi.w};
        if (ni == BK_TILE) {
            // all 16 tiles, software-pipelined by hand: the 16 permutes of k-slice q + 1 are in flight while the 16 MFMAs of slice q
            // issue (independent accumulators, back to back); the scheduling barriers keep the compiler from pairing each MFMA with
            // the wait for its own permute again, which ran at a quarter of the MFMA rate
            float a[BK_TILE], d[BK_TILE];
#pragma unroll
            for (int t = 0; t < BK_TILE; t++) a[t] = bj[0] * __int_as_float(__builtin_amdgcn_ds_bpermute(src + 4 * t, __float_as_int(bi[0])));
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if (q < 3) {
#pragma unroll
                    for (int t = 0; t < BK_TILE; t++) d[t] = __int_as_float(__builtin_amdgcn_ds_bpermute(src + 4 * t, __float_as_int(bi[q + 1])));
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int t = 0; t < BK_TILE; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], bl[q], acc[t], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (q < 3) {
#pragma unroll
                    for (int t = 0; t < BK_TILE; t++) a[t] = bj[q + 1] * d[t];
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int t = 0; t < BK_TILE; t++)
                    if (t < ni) {
                        const float di = __int_as_float(__builtin_amdgcn_ds_bpermute(src + 4 * t, __float_as_int(bi[q])));
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(bj[q] * di, bl[q], acc[t], 0, 0, 0);
                    }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) g += bj[q] * bj[q];
        if (++pending == BK_FLUSH_CHUNKS) flush();
        if (++s == per_row) s = 0, row++;
    }
    flush();

    for (int w = 0; w < BK_WAVES; w++) {
        if (wave == w) {
#pragma unroll
            for (int t = 0; t < BK_TILE; t++)
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int q = (t * 4 + e) * 64 + lane;
                    lds[q] = w ? lds[q] + sum[t][e] : sum[t][e];
                }
        }
        __syncthreads();
    }
    lds_g[wave][lane] = gsum;
    __syncthreads();
    const int64_t slot = (int64_t)group * gridDim.x + blockIdx.x;
    for (int q = threadIdx.x; q < BK_GROUP_OUT; q += BLK) partial[slot * BK_GROUP_OUT + q] = lds[q];
    if (diag && threadIdx.x < BK_TILE) {
        double t = 0.0;
        for (int w = 0; w < BK_WAVES; w++)
            for (int k = 0; k < 4; k++) t += lds_g[w][16 * k + threadIdx.x];
        partial_g[slot * BK_TILE + threadIdx.x] = t;
    }
}

// second stage: out[group][q] = the sum over the workgroups of partial[(group, workgroup)][q], in workgroup order; `width` values per slot
__global__ __launch_bounds__(BLK) void bk_triple_final(const double *__restrict__ partial, int nblocks, int ngroups, int width,
                                                       double *__restrict__ out) {
    const int64_t total = (int64_t)ngroups * width;
    for (int64_t q = (int64_t)blockIdx.x * BLK + threadIdx.x; q < total; q += (int64_t)gridDim.x * BLK) {
        const int64_t group = q / width, e = q % width;
        double t = 0.0;
        for (int b = 0; b < nblocks; b++) t += partial[(group * nblocks + b) * width + e];
        out[q] = t;
    }
}

int bk_check_n(const char *who, int n) {
    if (n < 2 || n > 32767) return fail("%s: mesh size %d out of range (2 .. 32767)", who, n);
    if (n & 1) return fail("%s: odd mesh size %d (the half spectrum is laid out for an even mesh)", who, n);
    return 0;
}

int bk_check_nb(const char *who, int nb) {
    if (nb < 1 || nb > BK_MAX_SHELLS) return fail("%s: %d shells (1 .. %d)", who, nb, BK_MAX_SHELLS);
    return 0;
}

int bk_check_meshes(const char *who, const void *const *meshes, int nb) {
    for (int b = 0; b < nb; b++) {
        if (!meshes[b]) return fail("%s: null mesh %d", who, b);
        if ((uintptr_t)meshes[b] % 16) return fail("%s: mesh %d is not aligned to 16 bytes", who, b);
        for (int a = 0; a < b; a++)
            if (meshes[a] == meshes[b]) return fail("%s: meshes %d and %d are the same buffer", who, a, b);
    }
    return 0;
}

}  // namespace

extern "C" {

int abacus_bk_check_memory(int n, int nb, int64_t np) {
    ABACUS_TRY(bk_check_n("abacus_bk_check_memory", n));
    ABACUS_TRY(bk_check_nb("abacus_bk_check_memory", nb));
    if (np < 0) return fail("abacus_bk_check_memory: negative particle count");
    ABACUS_ENTER();
    // the nb shell meshes, the spectrum, the two work meshes of an interlaced deposit + transform (or the work area of a C2R), the
    // packed copy of the particles and the lists of the deposit (about one position's worth again)
    return check_memory("abacus_bk_check_memory", n, [=](int m) { return (size_t)(nb + 3) * padded_bytes(m) + (size_t)np * 24; });
}

int abacus_bk_shells_dev(const void *spec_padded, int n, double Lbox, const double *kedges, int nb, float *const *meshes) {
    static const char *who = "abacus_bk_shells_dev";
    if (!kedges || !meshes) return fail("%s: null argument", who);
    ABACUS_TRY(bk_check_n(who, n));
    ABACUS_TRY(bk_check_nb(who, nb));
    if (!(Lbox > 0) || !std::isfinite(Lbox)) return fail("%s: Lbox must be positive", who);
    const float dk = (float)(2.0 * M_PI / Lbox);
    BkEdges ed;
    for (int b = 0; b <= nb; b++) {
        if (!std::isfinite(kedges[b]) || !(kedges[b] > 0)) return fail("%s: edge %d must be finite and positive", who, b);
        ed.e[b] = (float)kedges[b];
        if (b && !(ed.e[b] > ed.e[b - 1])) return fail("%s: the edges must increase (in float32)", who);
    }
    for (int b = nb + 1; b <= BK_MAX_SHELLS; b++) ed.e[b] = INFINITY;
    // the rule with the slack of the two float32 roundings (dk and the edge), so that float64(2 pi / L) n / 3 passes; and what it stands
    // for, exactly: the first mode number at or beyond n / 3 on an axis is in no shell (|k| is monotonic in the squared mode number)
    const int mc = (n + 2) / 3;
    if (!((double)ed.e[nb] <= (double)dk * n / 3.0 * (1.0 + 0x1p-22)) || !(dk * sqrtf((float)((int64_t)mc * mc)) >= ed.e[nb]))
        return fail("%s: the top edge %g lies above dk n / 3 = %g: the sums over the mesh would close triangles modulo n", who, kedges[nb],
                    (double)dk * n / 3.0);
    ABACUS_TRY(bk_check_meshes(who, (const void *const *)meshes, nb));
    for (int b = 0; b < nb; b++)
        if (meshes[b] == spec_padded) return fail("%s: mesh %d is the spectrum", who, b);
    if (spec_padded && (uintptr_t)spec_padded % 16) return fail("%s: the spectrum is not aligned to 16 bytes", who);
    ABACUS_ENTER();
    Scratch sc;
    float **table = nullptr;
    ABACUS_TRY(sc.get(&table, (size_t)nb * sizeof(float *)));
    HIP_TRY(hipMemcpyAsync(table, meshes, (size_t)nb * sizeof(float *), hipMemcpyHostToDevice, stream()));
    const dim3 grid(grid_for(ceil_div((int64_t)n * n, BK_WAVES), 16)), block(BLK);
    if (spec_padded)
        ABACUS_LAUNCH("bk_shell_mask", (bk_shell_mask<false>), grid, block, 0, (const float4 *)spec_padded, (float *const *)table, ed, nb, n,
                      pitch_r(n) / 4, dk);
    else
        ABACUS_LAUNCH("bk_shell_mask", (bk_shell_mask<true>), grid, block, 0, (const float4 *)nullptr, (float *const *)table, ed, nb, n,
                      pitch_r(n) / 4, dk);
    for (int b = 0; b < nb; b++) ABACUS_TRY(inverse(meshes[b], n));
    HIP_TRY(hipStreamSynchronize(stream()));        // `meshes` is the caller's host array
    return 0;
}

int abacus_bk_triple_dev(const float *const *meshes, int n, int nb, double *T_host, double *G_host) {
    static const char *who = "abacus_bk_triple_dev";
    if (!meshes || !T_host || !G_host) return fail("%s: null argument", who);
    ABACUS_TRY(bk_check_n(who, n));
    ABACUS_TRY(bk_check_nb(who, nb));
    ABACUS_TRY(bk_check_meshes(who, (const void *const *)meshes, nb));
    ABACUS_ENTER();
    const bool one = nb <= BK_TILE;
    const int ngroups = one ? 1 : BK_MAX_GROUPS;
    const int64_t nchunk = (int64_t)n * n * ceil_div(n, BK_CHUNK);
    // persistent workgroups: one per CU over all groups, a wave per SIMD (the accumulators and their float64 sums leave room for one)
    const unsigned int gx = std::max(1u, grid_for(ceil_div(nchunk, BK_WAVES) * ngroups, 1) / ngroups);
    Scratch sc;
    const float **table = nullptr;
    double *partial = nullptr, *partial_g = nullptr, *out = nullptr;
    const size_t nslot = (size_t)ngroups * gx;
    ABACUS_TRY(sc.get(&table, (size_t)nb * sizeof(float *)));
    ABACUS_TRY(sc.get(&partial, nslot * BK_GROUP_OUT * sizeof(double)));
    ABACUS_TRY(sc.get(&partial_g, nslot * BK_TILE * sizeof(double)));
    ABACUS_TRY(sc.get(&out, (size_t)ngroups * (BK_GROUP_OUT + BK_TILE) * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(table, meshes, (size_t)nb * sizeof(float *), hipMemcpyHostToDevice, stream()));
    HIP_TRY(hipMemsetAsync(partial_g, 0, nslot * BK_TILE * sizeof(double), stream()));     // the off-diagonal groups write none
    const dim3 grid(gx, ngroups), block(BLK);
    if (one)
        ABACUS_LAUNCH("bk_triple", (bk_triple<true>), grid, block, 0, (const float *const *)table, nb, n, pitch_r(n), partial, partial_g);
    else
        ABACUS_LAUNCH("bk_triple", (bk_triple<false>), grid, block, 0, (const float *const *)table, nb, n, pitch_r(n), partial, partial_g);
    double *out_g = out + (size_t)ngroups * BK_GROUP_OUT;
    ABACUS_LAUNCH("bk_triple_final", bk_triple_final, dim3((unsigned int)ceil_div((int64_t)ngroups * BK_GROUP_OUT, BLK)), block, 0,
                  (const double *)partial, (int)gx, ngroups, BK_GROUP_OUT, out);
    ABACUS_LAUNCH("bk_triple_final", bk_triple_final, dim3(1), block, 0, (const double *)partial_g, (int)gx, ngroups, BK_TILE, out_g);
    std::vector<double> host((size_t)ngroups * (BK_GROUP_OUT + BK_TILE));
    HIP_TRY(hipMemcpyAsync(host.data(), out, host.size() * sizeof(double), hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipStreamSynchronize(stream()));
    // C_i[j][l] of a tile lies in lane l % 16 + 16 (j / 4), register j % 4.  A triple whose blocks are not in ascending order is the
    // computed one with its indices sorted by block (the sums are symmetric); within a block every order is computed.
    auto value = [&](int i, int j, int l) {
        if (i / BK_TILE > j / BK_TILE) std::swap(i, j);
        if (j / BK_TILE > l / BK_TILE) std::swap(j, l);
        if (i / BK_TILE > j / BK_TILE) std::swap(i, j);
        int group = 0;
        for (int g = 0; g < ngroups; g++)
            if (bk_groups_host[g][0] == i / BK_TILE && bk_groups_host[g][1] == j / BK_TILE && bk_groups_host[g][2] == l / BK_TILE) group = g;
        const int jj = j % BK_TILE, ll = l % BK_TILE;
        return host[(size_t)group * BK_GROUP_OUT + ((i % BK_TILE) * 4 + jj % 4) * 64 + ll + 16 * (jj / 4)];
    };
    for (int i = 0; i < nb; i++)
        for (int j = 0; j < nb; j++)
            for (int l = 0; l < nb; l++) T_host[((size_t)i * nb + j) * nb + l] = value(i, j, l);
    const double *hg = host.data() + (size_t)ngroups * BK_GROUP_OUT;
    for (int i = 0; i < nb; i++) G_host[i] = hg[(i / BK_TILE ? ngroups - 1 : 0) * BK_TILE + i % BK_TILE];
    return 0;
}

}  // extern "C"
