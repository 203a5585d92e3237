// Linear control variates on MI355X (gfx950): linear_fields.py :108-124, tracer_power.py get_recon_power :410-414, :464, :501-503 and
// tools_cv.py combine_field_spectra_k3D_lcv :313-335.  Four streaming passes over padded spectra, none of which strides its lanes
// along z (lcv_for_each_mode, mesh_common.hpp).  The transform, the padding and the memory check are those of every mesh family
// (mesh_common.hpp, mesh.hip); the deposits and spectra of the tracers come through abacus_zcv_spectrum_dev (zcv.hip).
//
// This file is compiled with -ffp-contract=off (csrc/Makefile): the LCV products follow NumPy's float32 order of evaluation.
#include <algorithm>
#include <cmath>
#include <vector>

#include "mesh_common.hpp"

using namespace abacus;

namespace {

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

int lcv_check_n(const char *who, int n) {
    if (n < 2 || n > 32767) return fail("%s: mesh size %d out of range", who, n);
    if (n & 1) return fail("%s: odd mesh size %d (the reference's irfftn drops a cell there and add_ij indexes past it)", who, n);
    return 0;
}

}  // namespace

extern "C" {

int abacus_lcv_linear_dev(const float *delta, int n, void *out_delta_padded, void *out_deltamu2_padded) {
    ABACUS_ENTER();
    if (!delta || !out_delta_padded || !out_deltamu2_padded) return fail("abacus_lcv_linear_dev: null argument");
    if (out_delta_padded == out_deltamu2_padded) return fail("abacus_lcv_linear_dev: the two spectra must be different buffers");
    ABACUS_TRY(lcv_check_n("abacus_lcv_linear_dev", n));
    // (the two spectra are the caller's; the transform may take a work mesh of the same size)
    ABACUS_TRY(check_memory("lcv linear_fields", n, 2, [](int m) { return padded_bytes(m); }));
    const int pr = pitch_r(n), pc = pr / 2;
    float *Dm = static_cast<float *>(out_delta_padded);
    ABACUS_LAUNCH("zcv_pad", zcv_pad, dim3(grid_for((int64_t)n * n, 16)), dim3(BLK), 0, delta, Dm, n, (int64_t)pr);
    ABACUS_TRY(r2c_inplace(Dm, n));
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
    ABACUS_TRY(check_memory("lcv power3d", n, 2, [](int m) { return (size_t)m * m * (m / 2 + 1) * sizeof(float); }));
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
    ABACUS_TRY(check_memory("lcv combine_k3d", n, 2, [](int m) { return (size_t)3 * m * m * (m / 2 + 1) * sizeof(float); }));
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

}  // extern "C"
