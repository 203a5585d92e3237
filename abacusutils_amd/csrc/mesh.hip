// The transforms of a padded float32 mesh for every mesh family (mesh_common.hpp), and the one cache of hipFFT plans behind them.
// Host code only.
//
// The plans are in place, in the padded layout.  Per direction ([0] R2C, for the sizes the native transforms do not cover or with the
// option fft_hipfft; [1] C2R) the cache keeps the two sizes used last, the most recent first.  Two, because the shear field at one
// mesh size is interleaved with a control-variate or statistic chain at another; with one size they share one plan and its work area.
// A third size drops the older of the two: shear.hip and the other families each kept a size of their own before, so the one sequence
// that found its plan then and makes it again now is three different sizes in turn with the shear field coming back to its own.
#include "mesh_common.hpp"

using namespace abacus;

namespace {

struct Plan {
    hipfftHandle h = 0;
    int n = 0;   // 0: empty
};
Plan g_plans[2][2];

int get_plan(int n, int inverse, hipfftHandle *out) {
    Plan *p = g_plans[inverse];
    if (p[0].n != n) {
        std::swap(p[0], p[1]);      // the size before comes to the front, or is the one to go
        if (p[0].n != n) {
            if (p[0].n) (void)hipfftDestroy(p[0].h);
            p[0].n = 0;
            int dims[3] = {n, n, n};
            int rembed[3] = {n, n, pitch_r(n)}, cembed[3] = {n, n, pitch_r(n) / 2};
            const hipfftResult r = plan_with_retry([&] {
                return inverse ? hipfftPlanMany(&p[0].h, 3, dims, cembed, 1, 1, rembed, 1, 1, HIPFFT_C2R, 1)
                               : hipfftPlanMany(&p[0].h, 3, dims, rembed, 1, 1, cembed, 1, 1, HIPFFT_R2C, 1);
            });
            ABACUS_TRY(fft_check(r, "hipfftPlanMany"));
            p[0].n = n;
        }
    }
    ABACUS_TRY(fft_check(hipfftSetStream(p[0].h, stream()), "hipfftSetStream"));
    *out = p[0].h;
    return 0;
}

}  // namespace

namespace abacus {

int r2c_inplace(float *D, int n) {
    if (fft_native_supported(n) && !option("fft_hipfft")) return fft_native_r2c_inplace(D, n, pitch_r(n), 0.f);
    hipfftHandle fwd;
    ABACUS_TRY(get_plan(n, 0, &fwd));
    prof_begin("hipfft_r2c");
    const hipfftResult r = hipfftExecR2C(fwd, (hipfftReal *)D, (hipfftComplex *)D);
    prof_end("hipfft_r2c");
    return fft_check(r, "hipfftExecR2C");
}

int c2r_inplace(float *W, int n) {
    hipfftHandle inv;
    ABACUS_TRY(get_plan(n, 1, &inv));
    prof_begin("hipfft_c2r");
    const hipfftResult r = hipfftExecC2R(inv, (hipfftComplex *)W, (hipfftReal *)W);
    prof_end("hipfft_c2r");
    return fft_check(r, "hipfftExecC2R");
}

int release_plans() {
    for (auto &dir : g_plans)
        for (Plan &p : dir) {
            if (p.n) (void)hipfftDestroy(p.h);
            p.n = 0;
        }
    return 0;
}

}  // namespace abacus
