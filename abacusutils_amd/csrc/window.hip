// The mode-coupling window of the Zel'dovich control variates on MI355X (gfx950): the mesh pass of periodic_window_function
// (abacusnbody/hod/zcv/zenbu_window.py:48-181).  The reference walks the n x n x n/2 half mesh and, for every mode, adds
// pref_l L_l(mu) L_l'(mu) w[beta] to one row of the window for every input column beta of the mode's output bin.  The column weight
// does not depend on the mode, so the mesh pass is a histogram of nine Legendre products, the multiplicity and the wavenumber over
// the output bins; the outer product with the column weights is a small host step (hod/zcv/zenbu_window.py: assemble_window).
//
// One pass, no mesh in memory: a thread takes one (i, j) column and walks it along k.  The wavenumber never decreases along k
// (every float32 step is monotone), so neither does the bin: the thread keeps its running float64 sums in registers, moves its bin
// forward against the real edges (in LDS) and writes the sums out only when the bin changes and at the end of the column.  The sums
// go to a histogram of the workgroup in LDS while that fits beside the edges (up to WIN_LDS_BINS bins), else straight to device
// memory; either way they end in 64 interleaved copies of the O(nkout) result (an LDS histogram goes to copy `workgroup % 64`, a
// lane writing to device memory to copy `lane`: the lanes of a wave never meet on one address), which a second kernel adds up
// in a fixed order.  The order in which float64 terms reach one sum is not fixed (atomics); the counts are integers and exact.
//
// The per-mode float32 values are bit-equal to NumPy's: this file keeps -ffp-contract=off, sqrt and the quotient are the correctly
// rounded forms, and the wavenumbers of the mesh are the HOST's (NumPy's arange), uploaded, never re-derived here.
#include <algorithm>
#include <cmath>
#include <vector>

#include "mesh_common.hpp"

using namespace abacus;

namespace {

constexpr int WIN_BLK = 512;
constexpr int WIN_NS = 10;          // sums per bin: multiplicity, multiplicity * k, and the eight products that are not L0 L0 = 1
constexpr int WIN_COPIES = 64;      // interleaved copies of the result in device memory (one per lane of a wave)
constexpr int WIN_MAX_BINS = 4096;  // the edges live in LDS: (nkout + 1) * 8 bytes
constexpr size_t WIN_LDS_LIMIT = 64 << 10;
// the LDS histogram fits beside the edges up to here
constexpr int WIN_LDS_BINS = (int)((WIN_LDS_LIMIT - sizeof(double)) / ((WIN_NS + 1) * sizeof(double)));

size_t win_lds_bytes(int nkout, bool lds_hist) { return ((size_t)nkout + 1 + (lds_hist ? (size_t)nkout * WIN_NS : 0)) * sizeof(double); }

// the ten values of one mode; order of the products: (l, l') = (0,2) (0,4) (2,0) (2,2) (2,4) (4,0) (4,2) (4,4), each
// fl32(fl32(pref_l L_l) L_l') as `pref[ell] * legs[ell] * legs[ellp]` evaluates (zenbu_window.py:126-131, :158-162)
struct WinSums {
    double v[WIN_NS];
};

__device__ __forceinline__ void win_flush(WinSums &s, int bin, int nkout, double *hist, int copy, bool lds) {
    // hist: LDS [nkout][WIN_NS], or device memory [nkout][WIN_NS][WIN_COPIES]
    if (s.v[0] != 0.0 && bin >= 0 && bin < nkout) {
#pragma unroll
        for (int q = 0; q < WIN_NS; q++) {
            if (lds)
                atomicAdd(&hist[bin * WIN_NS + q], s.v[q]);
            else
                atomicAdd(&hist[((int64_t)bin * WIN_NS + q) * WIN_COPIES + copy], s.v[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < WIN_NS; q++) s.v[q] = 0.0;
}

template <bool LDS>
__global__ __launch_bounds__(WIN_BLK) void window_moments(const float *__restrict__ kvals, const double *__restrict__ kout, int nmesh, int nkout,
                                                          double *__restrict__ acc) {
    extern __shared__ double win_lds[];
    double *edges = win_lds;                 // nkout + 1
    double *hist = win_lds + nkout + 1;      // LDS: nkout * WIN_NS
    for (int e = threadIdx.x; e <= nkout; e += WIN_BLK) edges[e] = kout[e];
    if (LDS)
        for (int e = threadIdx.x; e < nkout * WIN_NS; e += WIN_BLK) hist[e] = 0.0;
    __syncthreads();

    const int half = nmesh / 2;
    const int64_t cols = (int64_t)nmesh * nmesh;
    double *target = LDS ? hist : acc;
    const int copy = threadIdx.x & (WIN_COPIES - 1);
    for (int64_t col = (int64_t)blockIdx.x * WIN_BLK + threadIdx.x; col < cols; col += (int64_t)gridDim.x * WIN_BLK) {
        const int i = (int)(col / nmesh), j = (int)(col % nmesh);
        const float kl = kvals[i], ky = kvals[j];       // line of sight: axis 0, signed
        const float kl2 = kl * kl, ky2 = ky * ky;
        WinSums s;
#pragma unroll
        for (int q = 0; q < WIN_NS; q++) s.v[q] = 0.0;
        int bin = -1;                                    // edges[bin] <= knorm < edges[bin + 1]; -1: below the first edge
        for (int k = 0; k < half; k++) {
            const float kr = kvals[k];
            // sqrtf, not __fsqrt_rn: the intrinsic compiles to the bare v_sqrt_f32 (1 ulp), np.sqrt rounds correctly
            const float knorm = sqrtf((kr * kr + ky2) + kl2);
            const double x = (double)knorm;
            // digitize(knorm, kout) - 1 = (number of edges <= knorm) - 1, equality with an edge included: a bisection for the
            // first mode of the column, from there on forward from the bin of the mode before
            int b = bin;
            if (k == 0) {
                int lo = 0, hi = nkout + 1;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (edges[mid] <= x)
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                b = lo - 1;
            } else {
                while (b < nkout && edges[b + 1] <= x) b++;
            }
            if (b != bin) {
                win_flush(s, bin, nkout, target, copy, LDS);
                bin = b;
            }
            if (bin >= nkout) break;                     // beyond the last edge, and so is the rest of the column
            if (bin < 0) continue;
            const float mu = (col == 0 && k == 0) ? 0.0f : __fdiv_rn(kl, knorm);
            const float mu2 = mu * mu;
            const float mu4 = mu2 * mu2;
            const float L2 = (3.0f * mu2 - 1.0f) / 2.0f;
            const float L4 = ((35.0f * mu4 - 30.0f * mu2) + 3.0f) / 8.0f;
            const float p2 = 5.0f * L2, p4 = 9.0f * L4;
            const float m = k == 0 ? 1.0f : 2.0f;        // the plane k = 0 counts once (the multiplication by 2 is exact)
            s.v[0] += (double)m;
            s.v[1] += (double)(m * knorm);
            s.v[2] += (double)(m * L2);
            s.v[3] += (double)(m * L4);
            s.v[4] += (double)(m * p2);
            s.v[5] += (double)(m * (p2 * L2));
            s.v[6] += (double)(m * (p2 * L4));
            s.v[7] += (double)(m * p4);
            s.v[8] += (double)(m * (p4 * L2));
            s.v[9] += (double)(m * (p4 * L4));
        }
        win_flush(s, bin, nkout, target, copy, LDS);
    }
    if (LDS) {
        __syncthreads();
        const int to = blockIdx.x & (WIN_COPIES - 1);
        for (int e = threadIdx.x; e < nkout * WIN_NS; e += WIN_BLK) {
            const double v = hist[e];
            if (v != 0.0) atomicAdd(&acc[(int64_t)e * WIN_COPIES + to], v);
        }
    }
}

// out[e] = sum of the copies of entry e, in the order of the copies
__global__ __launch_bounds__(256) void window_reduce(const double *__restrict__ acc, double *__restrict__ out, int total) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    double s = 0.0;
    for (int c = 0; c < WIN_COPIES; c++) s += acc[(int64_t)e * WIN_COPIES + c];
    out[e] = s;
}

}  // namespace

extern "C" {

int abacus_window_moments(int nmesh, const float *kvals_host, const double *kout_host, int nkout, double *S_host, double *nmodes_host,
                          double *ksum_host) {
    if (!kvals_host || !kout_host || !S_host || !nmodes_host || !ksum_host) return fail("abacus_window_moments: null argument");
    if (nmesh < 2 || nmesh > 32766 || (nmesh & 1)) return fail("abacus_window_moments: mesh size %d must be even and in 2 .. 32766", nmesh);
    if (nkout < 1 || nkout > WIN_MAX_BINS) return fail("abacus_window_moments: %d output bins, 1 .. %d are supported", nkout, WIN_MAX_BINS);
    for (int e = 0; e <= nkout; e++)
        if (!std::isfinite(kout_host[e]) || (e > 0 && !(kout_host[e] > kout_host[e - 1])))
            return fail("abacus_window_moments: the %d bin edges must be finite and strictly increasing (edge %d)", nkout + 1, e);
    for (int i = 0; i < nmesh; i++)
        if (!std::isfinite(kvals_host[i])) return fail("abacus_window_moments: wavenumber %d of the mesh is not finite", i);
    ABACUS_ENTER();
    const int total = nkout * WIN_NS;
    const size_t acc_bytes = (size_t)total * WIN_COPIES * sizeof(double);
    Scratch sc;
    float *kvals = nullptr;
    double *kout = nullptr, *acc = nullptr, *out = nullptr;
    ABACUS_TRY(sc.get(&kvals, (size_t)nmesh * sizeof(float)));
    ABACUS_TRY(sc.get(&kout, ((size_t)nkout + 1) * sizeof(double)));
    ABACUS_TRY(sc.get(&acc, acc_bytes));
    ABACUS_TRY(sc.get(&out, (size_t)total * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(kvals, kvals_host, (size_t)nmesh * sizeof(float), hipMemcpyHostToDevice, stream()));
    HIP_TRY(hipMemcpyAsync(kout, kout_host, ((size_t)nkout + 1) * sizeof(double), hipMemcpyHostToDevice, stream()));
    HIP_TRY(hipMemsetAsync(acc, 0, acc_bytes, stream()));
    const bool lds_hist = nkout <= WIN_LDS_BINS;
    const int64_t cols = (int64_t)nmesh * nmesh;
    const dim3 grid((unsigned int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(cols, WIN_BLK), (int64_t)fft_num_cus() * 8))), block(WIN_BLK);
    const size_t lds = win_lds_bytes(nkout, lds_hist);
    if (lds_hist)
        ABACUS_LAUNCH("window_moments", (window_moments<true>), grid, block, lds, kvals, kout, nmesh, nkout, acc);
    else
        ABACUS_LAUNCH("window_moments_global", (window_moments<false>), grid, block, lds, kvals, kout, nmesh, nkout, acc);
    ABACUS_LAUNCH("window_reduce", window_reduce, dim3((unsigned int)ceil_div(total, 256)), dim3(256), 0, acc, out, total);
    std::vector<double> host((size_t)total);
    HIP_TRY(hipMemcpyAsync(host.data(), out, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipStreamSynchronize(stream()));
    // S[o][l][l'] in the order of the header; (0, 0) is the multiplicity itself
    static const int slot[9] = {0, 2, 3, 4, 5, 6, 7, 8, 9};
    for (int o = 0; o < nkout; o++) {
        const double *h = host.data() + (size_t)o * WIN_NS;
        nmodes_host[o] = h[0];
        ksum_host[o] = h[1];
        for (int q = 0; q < 9; q++) S_host[(size_t)o * 9 + q] = h[slot[q]];
    }
    return 0;
}

}  // extern "C"
