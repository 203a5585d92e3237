// BAO reconstruction on MI355X (gfx950): the producer of the positions the linear control variates (lcv.hip) start from.  Standard
// plane-parallel reconstruction of a periodic box (line of sight = z) is a closed-form Fourier solve: delta(k) -> [recon_mult: the
// three displacement spectra in one pass] -> three C2R -> [recon_shift: psi read at every particle with the cloud of the deposit,
// shift, wrap].  No reference code: the arithmetic is stated in include/abacus_hip.h and pinned to tests/recon_statement.py.
//
// This file is compiled with -ffp-contract=off (csrc/Makefile).
#include <algorithm>
#include <cmath>
#include <vector>

#include "mesh_common.hpp"

using namespace abacus;

namespace {

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

int recon_check_n(const char *who, int n) {
    if (n < 2 || n > 32767) return fail("%s: mesh size %d out of range", who, n);
    if (n & 1) return fail("%s: odd mesh size %d (the displacement comes back through a real inverse transform)", who, n);
    return 0;
}
}  // namespace

extern "C" {

int abacus_recon_check_memory(int n, int64_t np) {
    ABACUS_ENTER();
    ABACUS_TRY(recon_check_n("abacus_recon_check_memory", n));
    if (np < 0) return fail("abacus_recon_check_memory: bad argument");
    // the three displacement meshes (the density spectrum lies in the third), the work mesh of the deposit + transform, the copy of
    // the positions, the sorted line lists of the deposit (about one position's worth again) and the shifted positions
    return check_memory("recon displacement", n, 2, [=](int m) { return (size_t)4 * padded_bytes(m) + (size_t)np * 36; });
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
    ABACUS_TRY(check_memory("recon delta", n, 2, [](int m) { return padded_bytes(m); }));
    float *Dm = static_cast<float *>(out_padded);
    ABACUS_LAUNCH("zcv_pad", zcv_pad, dim3(grid_for((int64_t)n * n, 16)), dim3(BLK), 0, delta, Dm, n, (int64_t)pitch_r(n));
    return r2c_inplace(Dm, n);
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
    ABACUS_TRY(check_memory("recon displacement", n, 2, [](int m) { return padded_bytes(m); }));
    ReconArgs m;
    m.n = n, m.pc = pitch_r(n) / 2;
    m.dk = (float)(2.0 * M_PI / Lbox);
    m.R2h = (float)(R * R / 2.0);
    m.b = (float)bias;
    m.beta = rsd ? (float)(f_growth / bias) : 0.0f;
    m.scale = normalised ? 1.0f : (float)(1.0 / ((double)n * n * n));
    ABACUS_LAUNCH("recon_mult", recon_mult, dim3(grid_for(ceil_div((int64_t)n * n, LCV_ROWS), 16)), dim3(BLK), 0, (const float2 *)delta_padded,
                  (float2 *)psi_x, (float2 *)psi_y, (float2 *)psi_z, m);
    ABACUS_TRY(c2r_inplace(psi_x, n));
    ABACUS_TRY(c2r_inplace(psi_y, n));
    return c2r_inplace(psi_z, n);
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
