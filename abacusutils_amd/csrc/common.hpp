// Shared runtime plumbing of libabacus_hip.so: error reporting, the library stream, device buffers and the
// per-kernel event profiler behind abacus_profile_* (include/abacus_hip.h).  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <string>

namespace abacus {

int fail(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
int ensure_init();
hipStream_t stream();
// Scratch blocks for the per-call temporaries of the host-array entry points (prepare.hip, staging.hip): hipMalloc + hipFree per
// temporary cost those calls more than their kernels (abacus_prepare_randoms: 5 pairs, 7 ms of a 0.1-ms kernel).  A released
// block is kept for the next call; abacus_scratch_release() frees what is not in use.
int scratch_acquire(void **out, size_t bytes);
void scratch_release(void *p);
int scratch_trim_idle();
// the mesh buffers the P(k) entry points keep between calls (power.hip: up to four fields, 35 GB each at 2048^3; fft.hip: the second
// mesh of the out-of-place passes) hold nothing between calls: given back when an allocation of the caller's fails (abacus_malloc)
int power_trim_caches();
int fft_trim_scratch();
// the in-place hipFFT plans mesh.hip keeps for the mesh families (their work areas are device memory)
int release_plans();

#define HIP_TRY(expr)                                                                                       \
    do {                                                                                                    \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess)                                                                               \
            return ::abacus::fail("%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);      \
    } while (0)

// Every extern "C" entry point starts with ABACUS_ENTER(): the library keeps one stream and reusable scratch
// allocations, so concurrent callers (ctypes releases the GIL) are serialised here; nested entry points re-enter.
std::recursive_mutex &api_mutex();
#define ABACUS_ENTER()                                                              \
    std::lock_guard<std::recursive_mutex> abacus_api_guard_(::abacus::api_mutex()); \
    ABACUS_TRY(::abacus::ensure_init())

#define ABACUS_TRY(expr)        \
    do {                        \
        int r_ = (expr);        \
        if (r_ != 0) return r_; \
    } while (0)

// Diagnostic options (abacus_set_option, include/abacus_hip.h): comparator paths the parity tests and the A/B scripts
// switch on explicitly - nothing in the library reads the environment.  0 when never set.
int option(const char *name);
// bumped by every abacus_set_option: a hot path may keep the options it reads in a snapshot taken at this version
unsigned int option_version();

// profiler hooks: no-ops unless abacus_profile_enable(1)
void prof_begin(const char *name);
void prof_end(const char *name);
bool prof_enabled();

// Launch a kernel on the library stream, bracketed by profiler events when profiling is on.
#define ABACUS_LAUNCH(name, kernel, grid, block, shmem, ...)                                     \
    do {                                                                                         \
        ::abacus::prof_begin(name);                                                              \
        kernel<<<grid, block, shmem, ::abacus::stream()>>>(__VA_ARGS__);                         \
        ::abacus::prof_end(name);                                                                \
        HIP_TRY(hipGetLastError());                                                              \
    } while (0)

// growable device allocation (never shrinks); contents are NOT preserved across grow()
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    int reserve(size_t nbytes) {
        if (nbytes <= cap) return 0;
        if (p) HIP_TRY(hipFree(p));
        p = nullptr;
        cap = 0;
        if (hipMalloc(&p, nbytes) != hipSuccess) {   // idle scratch blocks may be what stands in the way
            (void)hipGetLastError();
            p = nullptr;
            ABACUS_TRY(scratch_trim_idle());
            HIP_TRY(hipMalloc(&p, nbytes));
        }
        cap = nbytes;
        return 0;
    }
    int release() {
        if (p) HIP_TRY(hipFree(p));
        p = nullptr;
        cap = 0;
        return 0;
    }
    template <class T>
    T *as() const {
        return static_cast<T *>(p);
    }
};

static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- what scan.hip, fft.hip, gfft.hip, xbin.hip and tsc.hip offer the other sources: each declared here and nowhere else.  The five
// files include this header, so a default argument stands beside a definition the compiler has checked it against.
struct BinArgs;   // bin_device.hpp
// scan.hip
int exclusive_scan_u32(unsigned int *counters, int64_t n, int64_t *out, DevBuf &scratch, int zero_counters);
// fft.hip: the native transforms of a padded float32 mesh (power-of-two sizes here, the mixed-radix ones through gfft.hip)
bool fft_native_supported(int n);
bool fft_native_pow2(int n);
int fft_native_r2c_inplace(float *mesh, int n, int pitch_r, float xcut = 0.f);
int fft_native_zy(float *mesh, int n, int pitch_r, int64_t nx_local);
int fft_native_x(float *mesh, int n, int pitch_r, int64_t ny_local, int64_t x_stride, int64_t y_stride);
int fft_native_fused_supported(int n);
int fft_native_r2c_fused(float *mesh, int n, int pitch_r, float xcut = 0.f);   // rows come out in the permuted order of fft.hip's fused form
int fft_native_r2c_fused_zy(float *mesh, int n, int pitch_r, float xcut = 0.f);
int fft_native_fused_zy_slab(float *mesh, int n, int pitch_r, int h, int64_t xsep, int xg0, int p0, int pc, float *pack_out, int world,
                             float cut = 0.f);
int fft_native_fused_x_slab(float *mesh, int n, int pitch_r, int64_t ny_local);
int slab_layout_query(int n, int W, float cut, int pitch_c, int64_t *P_out, const unsigned int **row_off_dev);
int fft_native_release();
int fft_num_cus();
const float2 *fft_twiddles(int n);   // exp(-2 pi i m / n), m < n, device table
// gfft.hip
bool gfft_supported(int n, int is_double);
int gfft_r2c_inplace_f32(float *mesh, int n, int pitch_r, float xcut);
int gfft_r2c_inplace_f64(double *mesh, int n, int pitch_r);
int gfft_r2c_zy_f32(float *mesh, int n, int pitch_r);
bool gfft_xbin_supported(int n, const BinArgs &b, bool comp, bool inter = false);
int gfft_x_bin_run(const float *mesh, int n, int pitch_r, float inv_size, const float *W_dev, const BinArgs &b, const float *mesh2 = nullptr,
                   const void *phase = nullptr);
int gfft_release();
// xbin.hip: the last transform pass fused with the binning
bool xbin_supported(int n, int Nk, int Nmu, const BinArgs &b, bool comp);
bool xbin2_supported(int n, const BinArgs &b, bool comp);
int fft_x_bin_run(const float *mesh, int n, int pitch_r, float inv_size, const float *W_dev, const BinArgs &b, int dbg, int y0 = 0,
                  int ny_local = 0, int put_geom = 1, int layout = 0, int world = 1, const float *mesh_shifted = nullptr,
                  const float2 *phase = nullptr, const unsigned int *row_off = nullptr, int64_t plane_elems = 0, const float *mesh_b = nullptr,
                  const float *mesh_b_shifted = nullptr);
int xdesc_lookup(int n, const BinArgs &b, bool comp, size_t lds_other, const unsigned int **lut, const int **U, int *ncell, int *sh, int *off,
                 int *vtop, const unsigned long long **cnt, const double **ksum, int *ok);
double xbin_last_build_ms();
int xbin_last_gen();
int xbin_release();
// tsc.hip: deposits into device meshes and their bookkeeping
int tsc_deposit_f32(float *pos, int64_t n, const float *w, float *grid, int nmesh, int64_t zstride, double box, double offset, int wrap,
                    double norm, int cic, int list_mode = 0, double sub = 1.0, int zero_grid = 1);
int tsc_deposit_f64pos(double *pos, int64_t n, const double *w, float *grid, int nmesh, int64_t zstride, double box, double offset, int wrap,
                       double norm, int cic, double sub = 1.0);
int tsc_deposit_f64mesh(void *pos, int pos_f64, int64_t n, const void *w, double *grid, int nmesh, int64_t zstride, double box, double offset,
                        int wrap, double norm, int cic, double sub);
int tsc_deposit_slab_f32(float *pos, int64_t n, const float *w, float *grid, int nmesh, int xoff, int nx_local, int64_t zstride, double box,
                         double offset, int wrap, double norm, int cic, double sub, int xoff2, int nx_alloc = 0);
void tsc_wrapped_reset();
int tsc_wrapped_seen();
void tsc_lines_defer(int on);
int tsc_lines_deferred_check();
int tsc_release_work();

// Orders the LDS traffic of ONE wave: its lanes' earlier LDS writes are visible to its lanes' later LDS reads (the LDS
// executes a wave's instructions in order; the fences keep the compiler from moving accesses across).  Lets a wave that
// owns a private LDS region work without workgroup barriers.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace abacus
