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
// The linear control variates (lcv.hip), BAO reconstruction (recon.hip), the light-cone power multipoles (lc_power.hip) and the
// bispectrum (bispectrum.hip) began in this file; what they share with it - the padded layout, the in-place transforms, the memory
// check - is in mesh_common.hpp and mesh.hip.
//
// This file is compiled with -ffp-contract=off (csrc/Makefile): the lattice positions are bit-equal to NumPy's float32 operations.
#include <algorithm>
#include <cmath>
#include <vector>

#include "mesh_common.hpp"

using namespace abacus;

namespace {

constexpr int OP_FILTER = 0, OP_N2 = 1, OP_SIJ = 2;

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

// ---- host side ------------------------------------------------------------------------------------------------------------
int check_size(const char *who, int n) {
    if (n < 2 || n > 32767) return fail("%s: mesh size %d out of range", who, n);
    if (n & 1) return fail("%s: odd mesh size %d (the reference's irfftn drops a cell there and add_ij indexes past it)", who, n);
    return 0;
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

// s2 = sum_ij w_ij s_ij(x)^2 from the padded spectrum D through the padded work mesh W; `partial` != nullptr: the last
// accumulate leaves its per-workgroup sums there (grid_rows entries)
int s2_rounds(const float *D, float *W, float *s2, int n, double Lbox, double *partial, unsigned int grid_rows) {
    const int pr = pitch_r(n), pc = pr / 2;
    MultArgs m = mult_args(n, Lbox, pc, pc, 1.0 / ((double)n * n * n));
    static const int comp[6][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}};
    for (int q = 0; q < 6; q++) {
        m.ci = comp[q][0], m.cj = comp[q][1];
        ABACUS_TRY(launch_mult(OP_SIJ, true, (const float2 *)D, (float2 *)W, m));
        ABACUS_TRY(c2r_inplace(W, n));
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
    ABACUS_TRY(c2r_inplace(W, n));
    ABACUS_LAUNCH("zcv_unpad", zcv_unpad, dim3(grid_rows), dim3(BLK), 0, W, n2, n, (int64_t)pr);
    return 0;
}

}  // namespace

namespace abacus {
// minkowski.hip, voids.hip, wst.hip (mesh_common.hpp)
int smooth_c2r_inplace(float *D, int n, double Lbox, double R) {
    if (R > 0) {
        const int pc = pitch_r(n) / 2;
        MultArgs m = mult_args(n, Lbox, pc, pc, 1.0);
        m.norm = (float)(2.0 / (R * R));
        if (!(m.norm > 0)) return fail("abacus_mf_smooth_spectrum_dev: R = %g is too large for the float32 filter", R);
        ABACUS_TRY(launch_mult(OP_FILTER, false, (const float2 *)D, (float2 *)D, m));
    }
    return c2r_inplace(D, n);
}
}  // namespace abacus

extern "C" {

int abacus_zcv_filter_dev(const float *field, float *out, int n, double Lbox, double kcut) {
    ABACUS_ENTER();
    if (!field || !out) return fail("abacus_zcv_filter_dev: null argument");
    ABACUS_TRY(check_size("abacus_zcv_filter_dev", n));
    if (!(Lbox > 0) || !(kcut > 0)) return fail("abacus_zcv_filter_dev: Lbox and kcut must be positive");
    ABACUS_TRY(check_memory("zcv gaussian_filter", n, 2, [](int m) { return padded_bytes(m); }));
    Scratch sc;
    float *D = nullptr;
    ABACUS_TRY(sc.get(&D, padded_bytes(n)));
    const int pr = pitch_r(n), pc = pr / 2;
    const unsigned int grid_rows = grid_for((int64_t)n * n, 16);
    ABACUS_LAUNCH("zcv_pad", zcv_pad, dim3(grid_rows), dim3(BLK), 0, field, D, n, (int64_t)pr);
    ABACUS_TRY(r2c_inplace(D, n));
    MultArgs m = mult_args(n, Lbox, pc, pc, 1.0 / ((double)n * n * n));
    m.norm = (float)(2.0 * kcut * kcut);
    ABACUS_TRY(launch_mult(OP_FILTER, false, (const float2 *)D, (float2 *)D, m));
    ABACUS_TRY(c2r_inplace(D, n));
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
    ABACUS_TRY(check_memory("zcv get_dk_to", n, 2, [](int m) { return 2 * padded_bytes(m); }));
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
    ABACUS_TRY(check_memory("zcv get_fields", n, 2, [](int m) { return 2 * padded_bytes(m); }));
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
    ABACUS_TRY(r2c_inplace(D, n));
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
    return check_memory("zcv advect", n, 2, [=](int m) {
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
    return release_plans();
}

}  // extern "C"
