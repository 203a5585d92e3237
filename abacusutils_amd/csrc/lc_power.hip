// Light-cone power spectrum multipoles on MI355X (gfx950): FKP field and Yamamoto estimator (analysis/lc_power.py).  No reference code: the
// arithmetic is stated in include/abacus_hip.h and pinned to tests/lc_power_statement.py.  F = D - alpha R, the raw weighted deposits of
// data and randoms in a box the randoms fix, lies in a padded real mesh.  F_0(k) = R2C(F); for l = 2, 4 and every m:
// [lc_ylm_mult: work = S_lm(r^ of the cell) F, 4 B in + 4 B out per cell] -> R2C in place -> [lc_ylm_accum: F_l(k) (+)= S_lm(k^) work(k),
// the first m writes].  Both streaming kernels give one (i, j) row to a wave, so two of the three coordinates are uniform over the
// wave, and 16 B to a lane and step.  The spectra are binned by power_bin_padded_dev.
//
// This file is compiled with -ffp-contract=off (csrc/Makefile).
#include <algorithm>
#include <cmath>
#include <vector>

#include "mesh_common.hpp"

using namespace abacus;

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

extern "C" {

int abacus_lc_check_memory(int n, int nmeshes, int64_t np) {
    ABACUS_ENTER();
    ABACUS_TRY(lc_check_n("abacus_lc_check_memory", n));
    if (nmeshes < 0 || np < 0) return fail("abacus_lc_check_memory: bad argument");
    // the padded meshes still to be allocated, the packed copies of the particles and their weights, and the lists of the deposit
    // (about one position's worth again)
    return check_memory("light-cone power", n, 2, [=](int m) { return (size_t)nmeshes * padded_bytes(m) + (size_t)np * 28; });
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
    ABACUS_TRY(check_memory("light-cone power", n, 2, [](int m) { return padded_bytes(m); }));
    if (ell == 0) {
        HIP_TRY(hipMemcpyAsync(out_padded, F_padded, padded_bytes(n), hipMemcpyDeviceToDevice, stream()));
        return r2c_inplace(static_cast<float *>(out_padded), n);
    }
    LcGeom g;
    g.n = n, g.pitch = pitch_r(n);
    g.cx = (float)corner[0], g.cy = (float)corner[1], g.cz = (float)corner[2];
    g.h = (float)(Lbox / n);
    const int lm0 = ell == 2 ? 0 : 5;
    const dim3 grid(grid_for(ceil_div((int64_t)n * n, LC_WAVES), 16)), block(BLK);
    for (int m = 0; m < 2 * ell + 1; m++) {
        ABACUS_LAUNCH("lc_ylm_mult", lc_ylm_mult, grid, block, 0, F_padded, work_padded, g, lm0 + m);
        ABACUS_TRY(r2c_inplace(work_padded, n));
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
