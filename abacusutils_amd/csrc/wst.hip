// Solid-harmonic wavelet scattering transform of a periodic mesh on MI355X (gfx950): the coefficients S0, S1, S2 of Eickenberg et al.
// (2018) as used on AbacusSummit mocks by Valogiannis & Dvorkin (2022).  Python: analysis/wst.py; the arithmetic is stated in
// include/abacus_hip.h and pinned to the NumPy statement tests/wst_statement.py.  replaces: nothing in the reference, which has no
// such statistic.
//
// One modulus field U[sigma, l] of a resident padded spectrum is, for m = 1 .. 2 l + 1:
//   [wst_mult: work(k) = multiplier_{sigma, l, m}(k) src(k), 8 B in + 8 B out per mode = 8 B per cell] -> the C2R in place ->
//   [wst_accum: u2 (+)= work^2, 4 B + (4 B) in, 4 B out per cell; the first m writes, the last m writes sqrt(u2)],
// then [wst_moments: the float64 sums of U^q, 4 B per cell].  The second order feeds U back: a copy, the R2C in place, wst_scale by
// 1 / N (8 B per cell), and the same chain at a larger scale.  Everything but the transforms streams; the transforms dominate.
//
// wst_table.  The radial profile g(kappa) = (sigma kappa)^l exp(-sigma^2 kappa^2 / 2) depends on s = i^2 + j^2 + l^2 of the integer
//   mode numbers alone: the table holds float32(g) of the float64 expression for s = 0 .. 3 (n/2)^2 (the void_wtable pattern); no
//   float32 exp or pow per mode.  At 256^3 it is 196 KB and is served from the L2.
// wst_mult / wst_accum / wst_scale.  One (i, j) row per wave, so two of the three mode numbers are uniform over the wave; 16 B per
//   lane and step (two modes or four cells).  S_lm of the direction of the mode from the float32 mode numbers: one hardware
//   reciprocal (and one reciprocal square root for odd l) per mode and a polynomial - about 30 VALU operations per 16 B moved, an
//   order of magnitude below what the copy rate leaves a CU.  One m per pass: a pass per m keeps the chain at four meshes; producing
//   all 2 l + 1 products of one read would need 2 l + 1 work meshes (2.3 GB more at 512^3, l = 4) to save 8 of 36 bytes per cell.
// wst_moments.  pow((double)|x|, q) per cell and exponent, summed in float64: per-thread sums over a fixed deal of the rows to at
//   most 2048 workgroups per exponent, a tree over the workgroup, then one workgroup per exponent over the partials.  No float
//   atomics: the same bits on every run, whichever other exponents are asked for.  The double pow, not the memory, sets its time.
//   The pad floats of a row are never read.
//
// Compiled with -ffp-contract=off (the default of csrc/Makefile): wst_table is the statement's float64 expression term by term, and
// u2 + w * w in wst_accum is a product rounded to float32 and then a sum, as the statement's float32 evaluation has it.
#include <algorithm>
#include <cmath>
#include <vector>

#include "mesh_common.hpp"

using namespace abacus;

namespace {

constexpr int WAVES = BLK / 64;
constexpr int WST_MIN_N = 4, WST_MAX_N = 32766, WST_MAX_J = 8, WST_MAX_L = 4, WST_MAX_Q = 8;
constexpr double WST_MAX_EXP = 8.0;
constexpr int MOM_GRID = 2048;   // the fixed partition of the moments: rows are dealt to this many workgroups

struct QArgs {   // the exponents of one moment pass
    double q[WST_MAX_Q];
    int nq;
};

int table_count(int n) { return 3 * (n / 2) * (n / 2) + 1; }     // n <= 32766: below 2^30
unsigned int grid_rows(int64_t rows) {
    return (unsigned int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(rows, WAVES), (int64_t)fft_num_cus() * 16));
}

// table[s] = float32(x^ell exp(-x^2 / 2)), x = sigma (dk sqrt(s)) in float64, dk = 2 pi / n; x^ell as ell products, x^0 = 1
__global__ __launch_bounds__(BLK) void wst_table(float *__restrict__ table, int count, double sigma, double dk, int ell) {
    const int s = blockIdx.x * BLK + threadIdx.x;
    if (s >= count) return;
    const double x = sigma * (dk * sqrt((double)s));
    double p = 1.0;
    for (int e = 0; e < ell; e++) p = p * x;
    table[s] = (float)(p * exp(-0.5 * (x * x)));
}

constexpr float W_SQRT3 = 1.7320508075688772f, W_SQRT5 = 2.23606797749979f, W_SQRT6 = 2.449489742783178f, W_SQRT10 = 3.1622776601683795f,
                W_SQRT15 = 3.872983346207417f, W_SQRT35 = 5.916079783099616f, W_SQRT70 = 8.366600265340756f;

// S_lm, m = 0 .. 2 ELL, of the direction of (x, y, z) != 0, scaled so that sum_m S_lm(a) S_lm(b) = P_l(a . b); the order and the
// polynomials are those of `harmonics` in tests/wst_statement.py (l = 2, 4: those of lc_ylm in lc_power.hip).  m is uniform over the
// launch: a scalar branch.  Even l: products of two components times inv2 = 1 / |r|^2; odd l: one component times inv1 = 1 / |r|
// and an even polynomial.  The hardware reciprocal and reciprocal square root (1 ulp) stand for the divisions.
template <int ELL>
__device__ __forceinline__ float wst_ylm(int m, float x, float y, float z) {
    if (ELL == 0) return 1.0f;
    const float r2 = x * x + y * y + z * z;
    const float inv2 = __builtin_amdgcn_rcpf(r2);
    const float u = (x * x) * inv2, v = (y * y) * inv2, w = (z * z) * inv2;
    if (ELL == 1 || ELL == 3) {
        const float inv1 = __builtin_amdgcn_rsqf(r2);
        const float cx = x * inv1, cy = y * inv1, cz = z * inv1;
        if (ELL == 1) return m == 0 ? cz : (m == 1 ? cx : cy);
        switch (m) {
        case 0: return 0.5f * (cz * (5.0f * w - 3.0f));
        case 1: return (0.25f * W_SQRT6) * (cx * (5.0f * w - 1.0f));
        case 2: return (0.25f * W_SQRT6) * (cy * (5.0f * w - 1.0f));
        case 3: return (0.5f * W_SQRT15) * (cz * (u - v));
        case 4: return W_SQRT15 * (cz * ((x * y) * inv2));
        case 5: return (0.25f * W_SQRT10) * (cx * (u - 3.0f * v));
        default: return (0.25f * W_SQRT10) * (cy * (3.0f * u - v));
        }
    }
    if (ELL == 2) {
        switch (m) {
        case 0: return 0.5f * (3.0f * w - 1.0f);
        case 1: return W_SQRT3 * ((x * z) * inv2);
        case 2: return W_SQRT3 * ((y * z) * inv2);
        case 3: return (0.5f * W_SQRT3) * (u - v);
        default: return W_SQRT3 * ((x * y) * inv2);
        }
    }
    switch (m) {
    case 0: return 0.125f * ((35.0f * w - 30.0f) * w + 3.0f);
    case 1: return (0.25f * W_SQRT10) * (((x * z) * inv2) * (7.0f * w - 3.0f));
    case 2: return (0.25f * W_SQRT10) * (((y * z) * inv2) * (7.0f * w - 3.0f));
    case 3: return (0.25f * W_SQRT5) * ((u - v) * (7.0f * w - 1.0f));
    case 4: return (0.5f * W_SQRT5) * (((x * y) * inv2) * (7.0f * w - 1.0f));
    case 5: return (0.25f * W_SQRT70) * (((x * z) * inv2) * (u - 3.0f * v));
    case 6: return (0.25f * W_SQRT70) * (((y * z) * inv2) * (3.0f * u - v));
    case 7: return (0.125f * W_SQRT35) * ((u * u - 6.0f * (u * v)) + v * v);
    default: return (0.5f * W_SQRT35) * (((x * y) * inv2) * (u - v));
    }
}

// dst = multiplier_{l, m} src over padded spectra (rows of pitch4 float4 = 2 pitch4 modes): one (i, j) row per wave, two consecutive
// modes per lane and step; 2 c4 + 1 <= n/2 + 1 <= 2 pitch4 - 1: inside the row.  Even l: g S_lm; odd l: i g S_lm, (re, im) ->
// (-im, re).  l > 0: zeros at k = 0 and on every mode with a mode number n/2 (the stored mode stands for +-n/2 and S_lm differs on
// the two: no Hermitian product exists there).  The mode of a float4 beyond n/2 is written as 0.  src and dst differ.
template <int ELL>
__global__ __launch_bounds__(BLK) void wst_mult(const float4 *__restrict__ src, float4 *__restrict__ dst, int n, int pitch4,
                                                const float *__restrict__ table, int m) {
    const int half = n / 2, kzlen = half + 1, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t rows = (int64_t)n * n;
    for (int64_t row = (int64_t)blockIdx.x * WAVES + wave; row < rows; row += (int64_t)gridDim.x * WAVES) {
        const int i = (int)(row / n), j = (int)(row % n);
        const int fi = i < half ? i : i - n, fj = j < half ? j : j - n;
        const int sij = fi * fi + fj * fj;
        const bool rowzero = ELL > 0 && (i == half || j == half);
        const float x = (float)fi, y = (float)fj;
        auto apply = [&](const float4 &v, int c4) {
            const float in[4] = {v.x, v.y, v.z, v.w};
            float o[4];
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const int l = 2 * c4 + e, s = sij + l * l;
                const bool zero = l >= kzlen || (ELL > 0 && (rowzero || l == half || s == 0));
                float f = 0.0f;
                if (!zero) f = table[s] * wst_ylm<ELL>(m, x, y, (float)l);
                const float re = in[2 * e], im = in[2 * e + 1];
                o[2 * e] = zero ? 0.0f : ((ELL & 1) ? -(f * im) : f * re);
                o[2 * e + 1] = zero ? 0.0f : ((ELL & 1) ? f * re : f * im);
            }
            return make_float4(o[0], o[1], o[2], o[3]);
        };
        // two loads in flight per lane: a row of n/2 + 1 modes is one float4 more than a multiple of 64 at every n = 256 k, and a
        // second trip for that one float4 would double the round trips to memory
        for (int c0 = lane; 2 * c0 < kzlen; c0 += 128) {
            const int c1 = c0 + 64;
            const bool second = 2 * c1 < kzlen;
            const int64_t q = row * pitch4 + c0;
            const float4 v0 = src[q];
            float4 v1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (second) v1 = src[q + 64];
            dst[q] = apply(v0, c0);
            if (second) dst[q + 64] = apply(v1, c1);
        }
    }
}

// out (+)= work^2 over padded real meshes (rows of `pitch` floats, a multiple of 4): one row per wave, four cells per lane and step;
// 4 c4 + 3 <= n + 1 < pitch: inside the row.  FIRST writes; LAST leaves sqrt(u2); FIRST and LAST (l = 0, one m): |work|, which is
// sqrt(work^2) without its two roundings.  The cells of a float4 beyond n are written as 0.
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(BLK) void wst_accum(const float *__restrict__ work, float *__restrict__ out, int n, int pitch) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t rows = (int64_t)n * n;
    for (int64_t row = (int64_t)blockIdx.x * WAVES + wave; row < rows; row += (int64_t)gridDim.x * WAVES) {
        const float4 *src = reinterpret_cast<const float4 *>(work + row * pitch);
        float4 *dst = reinterpret_cast<float4 *>(out + row * pitch);
        for (int c4 = lane; 4 * c4 < n; c4 += 64) {
            const float4 w = src[c4];
            const float in[4] = {w.x, w.y, w.z, w.w};
            float p[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (!FIRST) {
                const float4 t = dst[c4];
                p[0] = t.x, p[1] = t.y, p[2] = t.z, p[3] = t.w;
            }
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                float t;
                if (FIRST && LAST) {
                    t = fabsf(in[e]);
                } else {
                    t = FIRST ? in[e] * in[e] : p[e] + in[e] * in[e];
                    if (LAST) t = sqrtf(t);
                }
                o[e] = 4 * c4 + e < n ? t : 0.0f;
            }
            dst[c4] = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
}

// every stored mode of a padded spectrum times `scale` (1 / N behind the R2C), in place: one row per wave, two modes per lane and step
__global__ __launch_bounds__(BLK) void wst_scale(float4 *__restrict__ spec, int n, int pitch4, float scale) {
    const int kzlen = n / 2 + 1, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t rows = (int64_t)n * n;
    for (int64_t row = (int64_t)blockIdx.x * WAVES + wave; row < rows; row += (int64_t)gridDim.x * WAVES)
        for (int c4 = lane; 2 * c4 < kzlen; c4 += 64) {
            const int64_t q = row * pitch4 + c4;
            const float4 v = spec[q];
            const bool two = 2 * c4 + 1 < kzlen;
            spec[q] = make_float4(v.x * scale, v.y * scale, two ? v.z * scale : 0.0f, two ? v.w * scale : 0.0f);
        }
}

// partial[k gridDim.x + b] = the float64 sum of pow((double)|x|, q_k) over the rows b, b + gridDim.x, ..., k = blockIdx.y: one
// exponent per workgroup (the double pow sets the time, not the 4 bytes per cell, which the exponents after the first read from the
// caches), so the sum of an exponent does not depend on which others are asked for.  q = 1, 2 and 0.5 take |x|, x x (exact in
// float64) and the correctly rounded sqrt: what pow returns up to its own error, at a fraction of its cost.  VEC: float4 loads (rows
// aligned to 16 bytes), the cells beyond the last full float4 one by one.  Only the n cells of a row are read.
template <bool VEC>
__global__ __launch_bounds__(BLK) void wst_moments(const float *__restrict__ mesh, int n, int64_t pitch, QArgs qa, double *__restrict__ partial) {
    __shared__ double lds[BLK];
    const int64_t rows = (int64_t)n * n;
    const double q = qa.q[blockIdx.y];
    const int kind = q == 1.0 ? 1 : (q == 2.0 ? 2 : (q == 0.5 ? 3 : 0));      // uniform over the workgroup
    double s = 0.0;
    auto add = [&](float v) {
        const double a = fabs((double)v);
        double t;
        if (kind == 1) t = a;
        else if (kind == 2) t = a * a;
        else if (kind == 3) t = sqrt(a);
        else t = pow(a, q);
        s += t;
    };
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const float *src = mesh + row * pitch;
        int c0 = 0;
        if (VEC) {
            c0 = n & ~3;
            for (int c = 4 * threadIdx.x; c < c0; c += 4 * BLK) {
                const float4 v = *reinterpret_cast<const float4 *>(src + c);
                add(v.x), add(v.y), add(v.z), add(v.w);
            }
        }
        for (int c = c0 + threadIdx.x; c < n; c += BLK) add(src[c]);
    }
    const double t = block_sum(s, lds);
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
}

// out[k] = the sum of partial[k count ..] in a fixed order: strided per thread, then the tree; one workgroup per exponent
__global__ __launch_bounds__(BLK) void wst_moments_final(const double *__restrict__ partial, int count, double *__restrict__ out) {
    __shared__ double lds[BLK];
    double s = 0.0;
    for (int i = threadIdx.x; i < count; i += BLK) s += partial[(int64_t)blockIdx.x * count + i];
    const double t = block_sum(s, lds);
    if (threadIdx.x == 0) out[blockIdx.x] = t;
}

// ------------------------------------------------------------------------------------------------------------------ host side
int check_n(const char *who, int n) {
    if (n < WST_MIN_N || n > WST_MAX_N) return fail("%s: mesh size %d out of range (%d .. %d)", who, n, WST_MIN_N, WST_MAX_N);
    if (n & 1) return fail("%s: odd mesh size %d (the half spectrum is laid out for an even mesh)", who, n);
    return 0;
}

int check_q(const char *who, const double *q, int nq) {
    if (nq < 1 || nq > WST_MAX_Q) return fail("%s: %d exponents (1 .. %d)", who, nq, WST_MAX_Q);
    for (int k = 0; k < nq; k++)
        if (!(q[k] > 0.0) || !(q[k] <= WST_MAX_EXP)) return fail("%s: exponent %d is %g; every q must lie in (0, %g]", who, k, q[k], WST_MAX_EXP);
    return 0;
}

bool overlap(const void *a, const void *b, size_t bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bytes && y < x + bytes;
}

QArgs qargs(const double *q, int nq) {
    QArgs qa;
    for (int k = 0; k < WST_MAX_Q; k++) qa.q[k] = k < nq ? q[k] : 1.0;
    qa.nq = nq;
    return qa;
}

int moment_grid(int n) { return (int)std::min<int64_t>((int64_t)n * n, MOM_GRID); }

// out_dev[0 .. nq) = the sums of |x|^q over the mesh; partial: nq * moment_grid(n) doubles
int launch_moments(const float *mesh, int n, int pitch, const QArgs &qa, double *partial, double *out_dev) {
    const int grid = moment_grid(n);
    if (pitch % 4 == 0 && (uintptr_t)mesh % 16 == 0)
        ABACUS_LAUNCH("wst_moments", (wst_moments<true>), dim3(grid, qa.nq), dim3(BLK), 0, mesh, n, (int64_t)pitch, qa, partial);
    else
        ABACUS_LAUNCH("wst_moments", (wst_moments<false>), dim3(grid, qa.nq), dim3(BLK), 0, mesh, n, (int64_t)pitch, qa, partial);
    ABACUS_LAUNCH("wst_moments_final", wst_moments_final, dim3(qa.nq), dim3(BLK), 0, (const double *)partial, grid, out_dev);
    return 0;
}

int launch_mult(int ell, const float *spec, float *work, int n, const float *table, int m) {
    const dim3 grid(grid_rows((int64_t)n * n)), block(BLK);
    const int pitch4 = pitch_r(n) / 4;
#define WST_MULT(E) ABACUS_LAUNCH("wst_mult", (wst_mult<E>), grid, block, 0, (const float4 *)spec, (float4 *)work, n, pitch4, table, m)
    switch (ell) {
    case 0: WST_MULT(0); break;
    case 1: WST_MULT(1); break;
    case 2: WST_MULT(2); break;
    case 3: WST_MULT(3); break;
    default: WST_MULT(4); break;
    }
#undef WST_MULT
    return 0;
}

// U[sigma, ell] of the padded spectrum `spec` into `out` through `work`; table: table_count(n) floats.  Arguments already checked.
int modulus(const float *spec, int n, double sigma, int ell, float *work, float *out, float *table) {
    const int count = table_count(n), pitch = pitch_r(n), nm = 2 * ell + 1;
    const dim3 grid(grid_rows((int64_t)n * n)), block(BLK);
    ABACUS_LAUNCH("wst_table", wst_table, dim3((unsigned int)ceil_div(count, BLK)), block, 0, table, count, sigma, 2.0 * M_PI / n, ell);
    for (int m = 0; m < nm; m++) {
        ABACUS_TRY(launch_mult(ell, spec, work, n, table, m));
        ABACUS_TRY(smooth_c2r_inplace(work, n, 1.0, 0.0));      // no filter: the C2R in place
        if (nm == 1)
            ABACUS_LAUNCH("wst_accum", (wst_accum<true, true>), grid, block, 0, (const float *)work, out, n, pitch);
        else if (m == 0)
            ABACUS_LAUNCH("wst_accum", (wst_accum<true, false>), grid, block, 0, (const float *)work, out, n, pitch);
        else if (m == nm - 1)
            ABACUS_LAUNCH("wst_accum", (wst_accum<false, true>), grid, block, 0, (const float *)work, out, n, pitch);
        else
            ABACUS_LAUNCH("wst_accum", (wst_accum<false, false>), grid, block, 0, (const float *)work, out, n, pitch);
    }
    return 0;
}

int spectrum_inplace(float *mesh, int n) {
    ABACUS_TRY(r2c_inplace(mesh, n));
    ABACUS_LAUNCH("wst_scale", wst_scale, dim3(grid_rows((int64_t)n * n)), dim3(BLK), 0, (float4 *)mesh, n, pitch_r(n) / 4,
                  (float)(1.0 / ((double)n * n * n)));
    return 0;
}

}  // namespace

extern "C" {

int abacus_wst_check_memory(int n, int64_t np) {
    static const char *who = "abacus_wst_check_memory";
    ABACUS_TRY(check_n(who, n));
    if (np < 0) return fail("%s: negative particle count", who);
    ABACUS_ENTER();
    // the four padded meshes of the chain (the spectrum, the work mesh, u2 / U and the spectrum of U; the deposit's own work meshes
    // take the place of the last three before the chain starts), the table, the partial sums, and the packed copy and deposit lists
    // of the particles
    auto bytes_of = [=](int m) { return 4 * padded_bytes(m) + (size_t)table_count(m) * 4 + (size_t)np * 24 + ((size_t)1 << 20); };
    return check_memory(who, n, WST_MIN_N, bytes_of);
}

int abacus_wst_modulus_dev(const void *spec_padded, int n, double sigma_cells, int ell, void *work_padded, void *out_padded) {
    static const char *who = "abacus_wst_modulus_dev";
    if (!spec_padded || !work_padded || !out_padded) return fail("%s: null argument", who);
    ABACUS_TRY(check_n(who, n));
    if (ell < 0 || ell > WST_MAX_L) return fail("%s: ell = %d (0 .. %d)", who, ell, WST_MAX_L);
    if (!(sigma_cells > 0) || !std::isfinite(sigma_cells)) return fail("%s: sigma must be positive and finite, got %g", who, sigma_cells);
    if ((uintptr_t)spec_padded % 16 || (uintptr_t)work_padded % 16 || (uintptr_t)out_padded % 16)
        return fail("%s: the meshes are not aligned to 16 bytes", who);
    const size_t bytes = (size_t)n * n * pitch_r(n) * sizeof(float);
    if (overlap(spec_padded, work_padded, bytes) || overlap(spec_padded, out_padded, bytes) || overlap(work_padded, out_padded, bytes))
        return fail("%s: the spectrum, the work mesh and the output are aliased; they must be three different meshes", who);
    ABACUS_ENTER();
    Scratch sc;
    float *table = nullptr;
    ABACUS_TRY(sc.get(&table, (size_t)table_count(n) * sizeof(float)));
    return modulus((const float *)spec_padded, n, sigma_cells, ell, (float *)work_padded, (float *)out_padded, table);
}

int abacus_wst_spectrum_dev(void *mesh_padded, int n) {
    static const char *who = "abacus_wst_spectrum_dev";
    if (!mesh_padded) return fail("%s: null mesh", who);
    ABACUS_TRY(check_n(who, n));
    if ((uintptr_t)mesh_padded % 16) return fail("%s: the mesh is not aligned to 16 bytes", who);
    ABACUS_ENTER();
    return spectrum_inplace((float *)mesh_padded, n);
}

int abacus_wst_moments_dev(const float *mesh, int n, int pitch, const double *q_host, int nq, double *sums_host) {
    static const char *who = "abacus_wst_moments_dev";
    if (!mesh || !q_host || !sums_host) return fail("%s: null argument", who);
    if (n < 2 || n > 32767) return fail("%s: mesh size %d out of range (2 .. 32767)", who, n);
    if (pitch < n) return fail("%s: pitch %d is smaller than the mesh size %d", who, pitch, n);
    if ((uintptr_t)mesh % 4) return fail("%s: the mesh is not aligned to 4 bytes", who);
    ABACUS_TRY(check_q(who, q_host, nq));
    ABACUS_ENTER();
    Scratch sc;
    double *partial = nullptr, *out = nullptr;
    ABACUS_TRY(sc.get(&partial, (size_t)nq * moment_grid(n) * sizeof(double)));
    ABACUS_TRY(sc.get(&out, WST_MAX_Q * sizeof(double)));
    ABACUS_TRY(launch_moments(mesh, n, pitch, qargs(q_host, nq), partial, out));
    HIP_TRY(hipMemcpyAsync(sums_host, out, (size_t)nq * sizeof(double), hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipStreamSynchronize(stream()));
    return 0;
}

int abacus_wst_coefficients_dev(void *spec_padded, int n, int J, int L, double sigma0_cells, const double *q_host, int nq, int contrast,
                                int second_order, double *S0_host, double *S1_host, double *S2_host) {
    static const char *who = "abacus_wst_coefficients_dev";
    if (!spec_padded || !q_host || !S0_host || !S1_host || (second_order && !S2_host)) return fail("%s: null argument", who);
    ABACUS_TRY(check_n(who, n));
    if (J < 1 || J > WST_MAX_J) return fail("%s: J = %d scales (1 .. %d)", who, J, WST_MAX_J);
    if (L < 0 || L > WST_MAX_L) return fail("%s: L = %d (0 .. %d)", who, L, WST_MAX_L);
    if (!(sigma0_cells > 0) || !std::isfinite(sigma0_cells)) return fail("%s: sigma0 must be positive and finite, got %g", who, sigma0_cells);
    ABACUS_TRY(check_q(who, q_host, nq));
    if ((uintptr_t)spec_padded % 16) return fail("%s: the spectrum is not aligned to 16 bytes", who);
    ABACUS_ENTER();
    const size_t bytes = padded_bytes(n);
    const int pitch = pitch_r(n), nl = L + 1;
    const QArgs qa = qargs(q_host, nq);
    const int n1 = J * nl, n2 = J * J * nl, nfield = 1 + n1 + n2;
    Scratch sc;
    float *work = nullptr, *U = nullptr, *Uhat = nullptr, *table = nullptr;
    double *partial = nullptr, *sums = nullptr;
    ABACUS_TRY(sc.get(&work, bytes));
    ABACUS_TRY(sc.get(&U, bytes));
    if (second_order && J > 1) ABACUS_TRY(sc.get(&Uhat, bytes));
    ABACUS_TRY(sc.get(&table, (size_t)table_count(n) * sizeof(float)));
    ABACUS_TRY(sc.get(&partial, (size_t)nq * moment_grid(n) * sizeof(double)));
    ABACUS_TRY(sc.get(&sums, (size_t)nfield * nq * sizeof(double)));
    float *spec = (float *)spec_padded;
    // the mode k = 0: 1 (rho = 1 + delta) or 0 (the contrast), imaginary part 0
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)spec, contrast ? 0 : 0x3f800000, 1, stream()));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(spec + 1), 0, 1, stream()));
    // S0: the field itself
    HIP_TRY(hipMemcpyAsync(work, spec, bytes, hipMemcpyDeviceToDevice, stream()));
    ABACUS_TRY(smooth_c2r_inplace(work, n, 1.0, 0.0));
    ABACUS_TRY(launch_moments(work, n, pitch, qa, partial, sums));
    for (int l = 0; l < nl; l++)
        for (int j1 = 0; j1 < J; j1++) {
            ABACUS_TRY(modulus(spec, n, std::ldexp(sigma0_cells, j1), l, work, U, table));
            ABACUS_TRY(launch_moments(U, n, pitch, qa, partial, sums + (size_t)(1 + j1 * nl + l) * nq));
            if (!Uhat || j1 == J - 1) continue;
            HIP_TRY(hipMemcpyAsync(Uhat, U, bytes, hipMemcpyDeviceToDevice, stream()));
            ABACUS_TRY(spectrum_inplace(Uhat, n));
            for (int j2 = j1 + 1; j2 < J; j2++) {
                ABACUS_TRY(modulus(Uhat, n, std::ldexp(sigma0_cells, j2), l, work, U, table));
                ABACUS_TRY(launch_moments(U, n, pitch, qa, partial, sums + (size_t)(1 + n1 + (j1 * J + j2) * nl + l) * nq));
            }
        }
    std::vector<double> host((size_t)nfield * nq, 0.0);
    HIP_TRY(hipMemcpyAsync(host.data(), sums, host.size() * sizeof(double), hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipStreamSynchronize(stream()));
    const double N = (double)n * n * n, nan = std::nan("");
    for (int k = 0; k < nq; k++) S0_host[k] = host[k] / N;
    for (int f = 0; f < n1; f++)
        for (int k = 0; k < nq; k++) S1_host[(size_t)f * nq + k] = host[(size_t)(1 + f) * nq + k] / N;
    if (S2_host)
        for (int j1 = 0; j1 < J; j1++)
            for (int j2 = 0; j2 < J; j2++)
                for (int l = 0; l < nl; l++)
                    for (int k = 0; k < nq; k++) {
                        const size_t f = (size_t)(j1 * J + j2) * nl + l;
                        S2_host[f * nq + k] = (second_order && j2 > j1) ? host[(1 + n1 + f) * nq + k] / N : nan;
                    }
    return 0;
}

}  // extern "C"
