// Tidal shear field on MI355X (gfx950): replaces abacusnbody/analysis/shear.py (smooth_density :15-21, get_tidal :38-66,
// get_shear_nb :69-93, get_shear :96-131) and the device part of hod/prepare_sim.py:1055-1127 `calc_shearmark`.
//
// Chain, all in HBM:  particles -> TSC counts -> Gaussian filter (three separable passes, reflect boundary, what
// scipy.ndimage.gaussian_filter does) -> R2C in place (fft.hip / gfft.hip, hipFFT for sizes they do not cover) -> for each of the
// six components of the TRACELESS tidal tensor S_ij(k) = (k_i k_j - delta_ij k^2 / 3) / k^2 * delta(k): one streaming kernel
// writes it into the work mesh, hipFFT C2R in place, one streaming kernel accumulates Q += w_ij S_ij(x)^2 -> sqrt(1.5 Q).
//
// Why traceless: the reference takes the eigenvalues of the full tensor and forms sqrt(((l2-l1)^2 + (l3-l1)^2 + (l3-l2)^2) / 2).
// That sum equals 3 tr(T^2) - tr(T)^2, which cancels in float32; with the trace removed in Fourier space it is 3 tr(S^2): one
// accumulator of non-negative terms and no eigen-solver.
//
// Meshes: `dfour` and the work mesh are padded like power.hip's (rows of pitch_r = roundup(n + 2, 32) floats); Q is the caller's
// output (n^3 float32).  All flat indices are 64-bit; grids are sized from the CU count.
#include <algorithm>
#include <cmath>
#include <map>
#include <vector>

#include "mesh_common.hpp"

using namespace abacus;

namespace {

constexpr int RING_MAX = 8;     // radii with a register-ring instantiation (sigma <= 2.1 cells)
constexpr int ZLDS_MAX = 64;    // largest radius of the LDS row kernel
constexpr int ZTILE = 2048;     // outputs per LDS tile of the z pass

// scipy's 'reflect' (d c b a | a b c d | d c b a): period 2n, any j
__device__ __forceinline__ int reflect_any(int j, int n) {
    const int p = 2 * n;
    j %= p;
    if (j < 0) j += p;
    return j < n ? j : p - 1 - j;
}
// the same for -n <= j < 2n
__device__ __forceinline__ int reflect_near(int j, int n) { return j < 0 ? -1 - j : (j >= n ? 2 * n - 1 - j : j); }

struct GaussW {
    double w[RING_MAX + 1];   // w[0] centre, w[k] at distance k
};

// Filter along an axis whose elements are `inner` floats apart (x: inner = n^2, y: inner = n).  The lanes of a wavefront sit
// along the contiguous axis (every load a coalesced line); a thread marches `chunk` cells along the filtered axis with the last
// 2R + 1 inputs in registers, so a cell is read (chunk + 2R) / chunk times.  Sums in float64, farthest pair first, like
// scipy's correlate1d, then one rounding to float32.
template <int R>
__global__ __launch_bounds__(BLK) void gauss_axis_ring(const float *__restrict__ in, float *__restrict__ out, int n, int64_t inner,
                                                       int64_t outer, int chunk, int nchunk, GaussW gw) {
    const int64_t total = outer * nchunk * inner;
    for (int64_t t = (int64_t)blockIdx.x * BLK + threadIdx.x; t < total; t += (int64_t)gridDim.x * BLK) {
        const int64_t i = t % inner, r = t / inner;
        const int ch = (int)(r % nchunk);
        const int64_t o = r / nchunk;
        const float *src = in + o * n * inner + i;
        float *dst = out + o * n * inner + i;
        const int j0 = ch * chunk, j1 = min(n, j0 + chunk);
        float v[2 * R + 1];
#pragma unroll
        for (int k = 0; k < 2 * R; k++) v[k + 1] = src[(int64_t)reflect_near(j0 - R + k, n) * inner];
#pragma unroll 4
        for (int j = j0; j < j1; j++) {
#pragma unroll
            for (int k = 0; k < 2 * R; k++) v[k] = v[k + 1];
            v[2 * R] = src[(int64_t)reflect_near(j + R, n) * inner];
            double acc = (double)v[R] * gw.w[0];
#pragma unroll
            for (int k = R; k >= 1; k--) acc += ((double)v[R - k] + (double)v[R + k]) * gw.w[k];
            dst[(int64_t)j * inner] = (float)acc;
        }
    }
}

// Any axis, any radius (also radius > n): one output per thread, 2 radius + 1 loads served by the caches.  inner == 1 (z axis): the
// output rows are `out_pitch` floats apart.
__global__ __launch_bounds__(BLK) void gauss_axis_direct(const float *__restrict__ in, float *__restrict__ out, int n, int64_t inner,
                                                         int64_t total, int64_t out_pitch, int radius, const double *__restrict__ w) {
    for (int64_t t = (int64_t)blockIdx.x * BLK + threadIdx.x; t < total; t += (int64_t)gridDim.x * BLK) {
        const int64_t q = t / inner;
        const int j = (int)(q % n);
        const float *src = in + (t - (int64_t)j * inner);
        double acc = (double)in[t] * w[0];
        for (int d = radius; d >= 1; d--)
            acc += ((double)src[(int64_t)reflect_any(j - d, n) * inner] + (double)src[(int64_t)reflect_any(j + d, n) * inner]) * w[d];
        const int64_t o = inner == 1 ? (t / n) * out_pitch + j : t;
        out[o] = (float)acc;
    }
}

// z axis (contiguous): a tile of a row and `radius` cells of halo on either side - reflected at the ends of the row, so they come
// from the same row - staged in LDS; rows of the output are `out_pitch` floats apart (the padded mesh of the transform)
__global__ __launch_bounds__(BLK) void gauss_z_lds(const float *__restrict__ in, float *__restrict__ out, int n, int64_t nrows,
                                                   int64_t out_pitch, int radius, const double *__restrict__ w, int tile, int ntile) {
    extern __shared__ double lds_w[];
    float *s = reinterpret_cast<float *>(lds_w + (radius + 1));
    for (int k = threadIdx.x; k <= radius; k += BLK) lds_w[k] = w[k];
    for (int64_t item = blockIdx.x; item < nrows * ntile; item += gridDim.x) {
        const int64_t row = item / ntile;
        const int t0 = (int)(item % ntile) * tile, len = min(tile, n - t0);
        __syncthreads();
        for (int k = threadIdx.x; k < len + 2 * radius; k += BLK) s[k] = in[row * n + reflect_any(t0 - radius + k, n)];
        __syncthreads();
        for (int k = threadIdx.x; k < len; k += BLK) {
            const float *c = s + k + radius;
            double acc = (double)c[0] * lds_w[0];
            for (int d = radius; d >= 1; d--) acc += ((double)c[-d] + (double)c[d]) * lds_w[d];
            out[row * out_pitch + t0 + k] = (float)acc;
        }
    }
}

// top-hat window of the reference (shear.py:24-29), evaluated in float64 (its k * r is float64: r is a Python float)
__device__ __forceinline__ double window_th(float ksq, double R) {
    const double x = (double)sqrtf(ksq) * R;
    return 3.0 * (sin(x) - x * cos(x)) / (x * x * x);
}

// factor of component (ci, cj) of the traceless tensor for wavevector (k0, k1, k2): (k_i k_j - delta_ij k^2 / 3) / k^2 [* window]
template <bool WINDOW>
__device__ __forceinline__ float tidal_factor(float k0, float k1, float k2, int ci, int cj, double R) {
    const float ksq = k0 * k0 + k1 * k1 + k2 * k2;
    const float ki = ci == 0 ? k0 : (ci == 1 ? k1 : k2), kj = cj == 0 ? k0 : (cj == 1 ? k1 : k2);
    float f = (ki * kj - (ci == cj ? ksq * (1.0f / 3.0f) : 0.f)) / ksq;
    if (WINDOW) f = (float)((double)f * window_th(ksq, R));
    return f;
}

// One component of the traceless tidal tensor, times `scale` (the 1 / n^3 of the inverse transform), into the work mesh: padded
// rows of pitch_c complex, one row (a, b) per workgroup step, lanes along c.  Modes with a * b * c == 0 are written as zeros (the
// reference skips them, shear.py:47, and the work mesh is reused).  ci, cj in 0..2.
// The plane c = n/2 is its own mirror image, and with k_z = -n/2 on both mirror partners the reference's xz / yz (and, on the
// x or y Nyquist lines, other) components are not Hermitian there.  Its inverse transform (complex along x and y, then real along
// z) reads only the real part of the transformed plane, which amounts to the plane's Hermitian part (t(a, b) + conj t(-a, -b)) / 2:
// written out here, so that the result does not depend on what a C2R library makes of a non-Hermitian plane.
template <bool WINDOW>
__global__ __launch_bounds__(BLK) void tidal_component(const float2 *__restrict__ dfour, float2 *__restrict__ work,
                                                       const float *__restrict__ karr, int n, int pitch_c, int ci, int cj, float scale,
                                                       double R) {
    const int kzlen = n / 2 + 1;
    const int64_t rows = (int64_t)n * n;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const int a = (int)(row / n), b = (int)(row % n);
        const float ka = karr[a], kb = karr[b];
        for (int c = threadIdx.x; c < kzlen; c += BLK) {
            float2 t = make_float2(0.f, 0.f);
            if (a != 0 && b != 0 && c != 0) {
                const float kc = karr[c];
                const float f = tidal_factor<WINDOW>(ka, kb, kc, ci, cj, R) * scale;
                const float2 d = dfour[row * pitch_c + c];
                t = make_float2(d.x * f, d.y * f);
                if (c == n / 2) {
                    const float f2 = tidal_factor<WINDOW>(karr[n - a], karr[n - b], kc, ci, cj, R) * scale;
                    const float2 d2 = dfour[((int64_t)(n - a) * n + (n - b)) * pitch_c + c];
                    t = make_float2(0.5f * (t.x + d2.x * f2), 0.5f * (t.y - d2.y * f2));
                }
            }
            work[row * pitch_c + c] = t;
        }
    }
}

// get_tidal (shear.py:38-66) as the reference returns it: the six FULL components k_i k_j / k^2 * dfour, (n, n, n/2+1, 6)
// complex64, from a contiguous (n, n, n/2+1) spectrum and the caller's float32 wavenumbers
__global__ __launch_bounds__(BLK) void tidal_full(const float2 *__restrict__ dfour, float2 *__restrict__ out, const float *__restrict__ karr,
                                                  int n, int window, double R) {
    const int kzlen = n / 2 + 1;
    const int64_t rows = (int64_t)n * n;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const int a = (int)(row / n), b = (int)(row % n);
        const float ka = karr[a], kb = karr[b];
        for (int c = threadIdx.x; c < kzlen; c += BLK) {
            float2 *o = out + (row * kzlen + c) * 6;
            float f[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            float2 d = make_float2(0.f, 0.f);
            if (a != 0 && b != 0 && c != 0) {
                const float kc = karr[c];
                const float ksq = ka * ka + kb * kb + kc * kc;
                d = dfour[row * kzlen + c];
                d.x /= ksq;
                d.y /= ksq;
                f[0] = ka * ka, f[1] = ka * kb, f[2] = ka * kc, f[3] = kb * kb, f[4] = kb * kc, f[5] = kc * kc;
                if (window) {
                    const double wth = window_th(ksq, R);
                    d.x = (float)((double)d.x * wth);   // (the reference scales the finished complex64 components)
                    d.y = (float)((double)d.y * wth);
                }
            }
#pragma unroll
            for (int q = 0; q < 6; q++) o[q] = make_float2(f[q] * d.x, f[q] * d.y);
        }
    }
}

// Q (+)= w t^2 over the n^3 cells of the padded work mesh; the last component folds in the final sqrt(1.5 Q)
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(BLK) void shear_accumulate(const float *__restrict__ work, float *__restrict__ q, int n, int pitch, float w) {
    const int64_t rows = (int64_t)n * n;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const float *src = work + row * pitch;
        float *dst = q + row * n;
        for (int c = threadIdx.x; c < n; c += BLK) {
            const float t = src[c];
            float acc = w * t * t;
            if (!FIRST) acc += dst[c];
            dst[c] = LAST ? sqrtf(1.5f * acc) : acc;
        }
    }
}

// out[i] = mesh[g[i,0], g[i,1], g[i,2]]; an index outside the mesh gives NaN (never a read out of bounds)
__global__ __launch_bounds__(BLK) void mesh_gather(const float *__restrict__ mesh, int n, const int64_t *__restrict__ g, int64_t nh,
                                                   float *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < nh; i += (int64_t)gridDim.x * BLK) {
        const int64_t a = g[3 * i], b = g[3 * i + 1], c = g[3 * i + 2];
        const bool ok = a >= 0 && a < n && b >= 0 && b < n && c >= 0 && c < n;
        out[i] = ok ? mesh[(a * n + b) * n + c] : __builtin_nanf("");
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// scipy.ndimage's _gaussian_kernel1d with truncate = 4: w[0] centre .. w[radius], normalised over the 2 radius + 1 taps
void gauss_weights(double sigma, std::vector<double> &w) {
    const int radius = (int)(4.0 * sigma + 0.5);
    w.assign((size_t)radius + 1, 0.0);
    double sum = 0;
    for (int k = 0; k <= radius; k++) {
        w[(size_t)k] = std::exp(-0.5 / (sigma * sigma) * (double)k * (double)k);
        sum += (k ? 2.0 : 1.0) * w[(size_t)k];
    }
    for (double &x : w) x /= sum;
}

int upload(void *dst, const void *src, size_t bytes) {
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream()));
    HIP_TRY(hipStreamSynchronize(stream()));   // `src` is a temporary of the caller
    return 0;
}

template <int R>
int launch_ring(const char *name, const float *in, float *out, int n, int64_t inner, int64_t outer, const double *w) {
    GaussW gw;
    for (int k = 0; k <= R; k++) gw.w[k] = w[k];
    const int chunk = 64, nchunk = (n + chunk - 1) / chunk;
    const int64_t total = outer * nchunk * inner;
    ABACUS_LAUNCH(name, gauss_axis_ring<R>, dim3(grid_for(ceil_div(total, BLK), 16)), dim3(BLK), 0, in, out, n, inner, outer,
                  chunk, nchunk, gw);
    return 0;
}

// one pass along `axis` (0, 1, 2) of a contiguous n^3 mesh; `out_pitch` (floats per z row of the output) only for axis 2
int smooth_axis(const float *in, float *out, int n, int axis, int64_t out_pitch, const std::vector<double> &w, const double *w_dev) {
    const int radius = (int)w.size() - 1;
    const int64_t total = (int64_t)n * n * n;
    if (axis == 2) {
        if (radius <= ZLDS_MAX) {
            const int tile = std::min(n, ZTILE), ntile = (n + tile - 1) / tile;
            const size_t lds = (size_t)(radius + 1) * sizeof(double) + (size_t)(tile + 2 * radius) * sizeof(float);
            ABACUS_LAUNCH("gauss_z_lds", gauss_z_lds, dim3(grid_for((int64_t)n * n * ntile, 8)), dim3(BLK), lds, in, out, n, (int64_t)n * n,
                          out_pitch, radius, w_dev, tile, ntile);
            return 0;
        }
        ABACUS_LAUNCH("gauss_axis_direct", gauss_axis_direct, dim3(grid_for(ceil_div(total, BLK), 16)), dim3(BLK), 0, in, out, n, (int64_t)1,
                      total, out_pitch, radius, w_dev);
        return 0;
    }
    const int64_t inner = axis == 0 ? (int64_t)n * n : n, outer = axis == 0 ? 1 : n;
    const char *name = axis == 0 ? "gauss_x_ring" : "gauss_y_ring";
    if (radius >= 1 && radius <= RING_MAX && radius <= n) {
        switch (radius) {
            case 1: return launch_ring<1>(name, in, out, n, inner, outer, w.data());
            case 2: return launch_ring<2>(name, in, out, n, inner, outer, w.data());
            case 3: return launch_ring<3>(name, in, out, n, inner, outer, w.data());
            case 4: return launch_ring<4>(name, in, out, n, inner, outer, w.data());
            case 5: return launch_ring<5>(name, in, out, n, inner, outer, w.data());
            case 6: return launch_ring<6>(name, in, out, n, inner, outer, w.data());
            case 7: return launch_ring<7>(name, in, out, n, inner, outer, w.data());
            case 8: return launch_ring<8>(name, in, out, n, inner, outer, w.data());
        }
    }
    ABACUS_LAUNCH("gauss_axis_direct", gauss_axis_direct, dim3(grid_for(ceil_div(total, BLK), 16)), dim3(BLK), 0, in, out, n, inner, total,
                  (int64_t)n, radius, w_dev);
    return 0;
}

// x: a -> b, y: b -> a, z: a -> zout (rows zpitch floats apart); a, b: n^3 floats
int smooth3(float *a, float *b, float *zout, int64_t zpitch, int n, const std::vector<double> &w, Scratch &sc) {
    double *w_dev = nullptr;
    ABACUS_TRY(sc.get(&w_dev, w.size() * sizeof(double)));
    ABACUS_TRY(upload(w_dev, w.data(), w.size() * sizeof(double)));
    ABACUS_TRY(smooth_axis(a, b, n, 0, n, w, w_dev));
    ABACUS_TRY(smooth_axis(b, a, n, 1, n, w, w_dev));
    return smooth_axis(a, zout, n, 2, zpitch, w, w_dev);
}

// np.fft.fftfreq(n, d = Lbox / (2 pi n)).astype(float32) as NumPy forms it: signed index times 1 / (n d)
void wavenumbers(int n, double Lbox, std::vector<float> &k) {
    const double d = Lbox / (2.0 * M_PI * n), val = 1.0 / (n * d);
    k.resize((size_t)n);
    for (int i = 0; i < n; i++) k[(size_t)i] = (float)((double)(i < (n + 1) / 2 ? i : i - n) * val);
}

int check_size(const char *who, int n) {
    if (n < 2 || n > 32767) return fail("%s: mesh size %d out of range", who, n);
    if (n & 1) return fail("%s: odd mesh size %d (the reference's irfftn drops a cell there and fails)", who, n);
    return 0;
}

// D: padded mesh holding the (smoothed) density, W: padded work mesh, out: n^3 floats
int shear_run(float *D, float *W, float *out, int n, double Lbox, double R, Scratch &sc) {
    const int pr = pitch_r(n), pc = pr / 2;
    ABACUS_TRY(r2c_inplace(D, n));       // native: the plain three-pass form, rows in natural order
    std::vector<float> kh;
    wavenumbers(n, Lbox, kh);
    float *karr = nullptr;
    ABACUS_TRY(sc.get(&karr, kh.size() * sizeof(float)));
    ABACUS_TRY(upload(karr, kh.data(), kh.size() * sizeof(float)));
    const float scale = (float)(1.0 / ((double)n * n * n));
    const unsigned int grid = grid_for((int64_t)n * n, 16);
    static const int comp[6][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}};
    for (int q = 0; q < 6; q++) {
        const int ci = comp[q][0], cj = comp[q][1];
        if (R >= 0)
            ABACUS_LAUNCH("tidal_component", tidal_component<true>, dim3(grid), dim3(BLK), 0, (const float2 *)D, (float2 *)W, karr, n, pc, ci,
                          cj, scale, R);
        else
            ABACUS_LAUNCH("tidal_component", tidal_component<false>, dim3(grid), dim3(BLK), 0, (const float2 *)D, (float2 *)W, karr, n, pc, ci,
                          cj, scale, 0.0);
        ABACUS_TRY(c2r_inplace(W, n));
        const float w = ci == cj ? 1.f : 2.f;
        if (q == 0)
            ABACUS_LAUNCH("shear_accumulate", (shear_accumulate<true, false>), dim3(grid), dim3(BLK), 0, W, out, n, pr, w);
        else if (q == 5)
            ABACUS_LAUNCH("shear_accumulate", (shear_accumulate<false, true>), dim3(grid), dim3(BLK), 0, W, out, n, pr, w);
        else
            ABACUS_LAUNCH("shear_accumulate", (shear_accumulate<false, false>), dim3(grid), dim3(BLK), 0, W, out, n, pr, w);
    }
    return 0;
}

}  // namespace

extern "C" {

int abacus_gauss_smooth_dev(float *mesh, float *tmp, int n, const double *weights, int radius) {
    ABACUS_ENTER();
    if (!mesh || !tmp || !weights) return fail("abacus_gauss_smooth_dev: null argument");
    if (n < 1 || n > 32767 || radius < 0) return fail("abacus_gauss_smooth_dev: bad size (n %d, radius %d)", n, radius);
    Scratch sc;
    const std::vector<double> w(weights, weights + radius + 1);
    ABACUS_TRY(smooth3(mesh, tmp, tmp, n, n, w, sc));
    HIP_TRY(hipMemcpyAsync(mesh, tmp, (size_t)n * n * n * sizeof(float), hipMemcpyDeviceToDevice, stream()));
    return 0;
}

int abacus_shear_dev(float *dens, float *out, int n, double Lbox, double R_or_negative) {
    ABACUS_ENTER();
    if (!dens || !out) return fail("abacus_shear_dev: null argument");
    ABACUS_TRY(check_size("abacus_shear_dev", n));
    ABACUS_TRY(check_memory("shear", n, 2, [](int m) { return 2 * padded_bytes(m); }));       // the spectrum and the work mesh
    Scratch sc;
    float *D = nullptr, *W = nullptr;
    ABACUS_TRY(sc.get(&D, padded_bytes(n)));
    ABACUS_TRY(sc.get(&W, padded_bytes(n)));
    HIP_TRY(hipMemcpy2DAsync(D, (size_t)pitch_r(n) * sizeof(float), dens, (size_t)n * sizeof(float), (size_t)n * sizeof(float), (size_t)n * n,
                             hipMemcpyDeviceToDevice, stream()));
    return shear_run(D, W, out, n, Lbox, R_or_negative, sc);
}

int abacus_shearmark_dev(const float *pos, int64_t np, int n, double Lbox, double sigma_cells, float *out) {
    ABACUS_ENTER();
    if (!pos || !out || np < 1) return fail("abacus_shearmark_dev: null argument or no particles");
    ABACUS_TRY(check_size("abacus_shearmark_dev", n));
    ABACUS_TRY(check_memory("shear", n, 2, [](int m) { return 2 * padded_bytes(m); }));       // the spectrum and the work mesh
    Scratch sc;
    float *D = nullptr, *W = nullptr, *p = nullptr;
    ABACUS_TRY(sc.get(&D, padded_bytes(n)));
    ABACUS_TRY(sc.get(&W, padded_bytes(n)));
    ABACUS_TRY(sc.get(&p, (size_t)np * 3 * sizeof(float)));   // the deposit wraps positions in place: on a copy
    HIP_TRY(hipMemcpyAsync(p, pos, (size_t)np * 3 * sizeof(float), hipMemcpyDeviceToDevice, stream()));
    if (sigma_cells > 1e-15) {
        // counts into `out`, filtered x: out -> W, y: W -> out, z: out -> D (padded rows)
        ABACUS_TRY(tsc_deposit_f32(p, np, nullptr, out, n, n, Lbox, 0.0, 1, 0.0, 0, 0, 0.0, 1));
        std::vector<double> w;
        gauss_weights(sigma_cells, w);
        ABACUS_TRY(smooth3(out, W, D, pitch_r(n), n, w, sc));
    } else {
        ABACUS_TRY(tsc_deposit_f32(p, np, nullptr, D, n, pitch_r(n), Lbox, 0.0, 1, 0.0, 0, 0, 0.0, 1));
    }
    return shear_run(D, W, out, n, Lbox, -1.0, sc);
}

int abacus_tidal_dev(const void *dfour_c64, const float *karr, int n, double R_or_negative, void *out_c64) {
    ABACUS_ENTER();
    if (!dfour_c64 || !karr || !out_c64) return fail("abacus_tidal_dev: null argument");
    if (n < 1 || n > 32767) return fail("abacus_tidal_dev: mesh size %d out of range", n);
    ABACUS_LAUNCH("tidal_full", tidal_full, dim3(grid_for((int64_t)n * n, 16)), dim3(BLK), 0, (const float2 *)dfour_c64, (float2 *)out_c64, karr,
                  n, R_or_negative >= 0 ? 1 : 0, R_or_negative);
    return 0;
}

int abacus_mesh_gather_dev(const float *mesh, int n, const int64_t *g, int64_t nh, float *out) {
    ABACUS_ENTER();
    if (nh == 0) return 0;
    if (!mesh || !g || !out || n < 1 || nh < 0) return fail("abacus_mesh_gather_dev: bad argument");
    ABACUS_LAUNCH("mesh_gather", mesh_gather, dim3(grid_for(ceil_div(nh, BLK), 16)), dim3(BLK), 0, mesh, n, g, nh, out);
    return 0;
}

}  // extern "C"
