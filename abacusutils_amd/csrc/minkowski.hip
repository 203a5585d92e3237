// Minkowski functionals of a periodic mesh on MI355X (gfx950): the lattice counts of Crofton's formula (Schmalzing & Buchert 1997) for
// up to 64 thresholds in one pass over the mesh, the float64 moments that thresholds in units of sigma need, and the periodic Gaussian
// smoothing of a resident spectrum.  Python: analysis/minkowski.py; the arithmetic is stated in include/abacus_hip.h and pinned to the
// NumPy statement tests/minkowski_statement.py.  replaces: nothing in the reference, which has no morphological statistic.
//
// mf_count.  The excursion set of a threshold is the union of the closed voxels with value >= threshold; a face, edge or vertex of the
// lattice belongs to it iff the maximum of the 2, 4 or 8 voxels that touch it does.  b(v) = the number of thresholds <= v is monotonic,
// so b(max(u, v)) = max(b(u), b(v)): every mesh value is located among the sorted thresholds ONCE (mf_bin: 8 comparisons against
// values every lane shares, then 7 against one group of the table in LDS; no chain of dependent reads), kept as one byte, and the 8
// maxima of a voxel are integer maxima of bytes.
//
//   tile      16 (y) x 64 (z) cells per workgroup of 256 threads, marched along x over a chunk of 32 planes.  Per plane a workgroup
//             loads 17 rows of 17 float4 (the last one for its first cell only: the +z halo), locates them and writes the bytes to
//             one of two plane buffers in LDS (17 x 17 words); the loads of plane x + 2 are in flight while plane x is counted.
//   halo      (17 * 68) / (16 * 64) = 1.129 in (y, z), 33 / 32 in x: at most 1.16 values requested per cell, the surplus mostly
//             from the L2 (the neighbouring tiles run at the same time).
//   carry     a thread owns 4 voxels of a row.  Of each plane it keeps the 2-D maxima over (y, z), (y + 1, z), (y, z + 1),
//             (y + 1, z + 1) in registers; the 8 elements a voxel owns are those of its own plane and their maxima with the next
//             plane's: 4 LDS reads per thread per plane, one barrier per plane.
//   bins      4 classes (vertices, edges, faces, voxels) x 65 bins x 32 copies of uint32 in LDS (33,280 B): a lane adds into copy
//             lane % 32, so no two lanes of a half wave share a bank or an address (ds_add_u32, no return value).  One flush per
//             workgroup: 260 uint32 to its row of `partial`; mf_count_final adds the rows into 64-bit totals (integer adds: exact
//             in any order).  The host takes the suffix sums over the thresholds.
//   budget    streaming at the HBM rate gives a CU ~26 cycles per 64 voxels: ~50 VALU issue slots and 26 LDS cycles.  Per voxel: the
//             search 2 VALU per comparison (8 up to 8 thresholds, 15 and two 16-byte LDS reads beyond), ~10 VALU for the byte
//             maxima, 8 address computations and 8 LDS adds.  The LDS adds were budgeted at the 4 cycles of a ds_write_b32 and take
//             about 10: they, not the loads, set the time ("Minkowski functionals"; profiles/minkowski/README.md).
//
// Compiled with -ffp-contract=off (the default of csrc/Makefile); the only float operations here are comparisons and float64 sums.
#include <algorithm>
#include <cmath>
#include <vector>

#include "mesh_common.hpp"

using namespace abacus;

namespace {

constexpr int MF_MAX_THR = 64, MF_BINS = MF_MAX_THR + 1, MF_OUT = 4 * MF_BINS;
constexpr int MF_TY = 16, MF_TZ = 64, MF_XC = 32;        // tile rows, tile cells along z, planes per chunk
constexpr int MF_ROWS = MF_TY + 1, MF_WORDS = MF_TZ / 4 + 1, MF_TASKS = MF_ROWS * MF_WORDS;
constexpr int MF_TABLE = 128;                            // the thresholds, NaN beyond them: 9 groups of 8 are read at most
constexpr int MOM_GRID = 2048;                           // the fixed partition of the moments: rows are dealt to this many workgroups

// one load task of a plane: a row of the tile (already wrapped) and four cells of it
struct MfTask {
    int64_t roff;   // row offset in floats inside a plane
    int gz0;        // first cell along z
    int ne;         // cells wanted (4, or 1 for the +z halo word)
    int mode;       // 0: nothing to load, 1: one aligned float4 inside the row, 2: cell by cell, cell n wrapping to 0
};

// cells outside the mesh come back as NaN: no threshold is <= NaN, they fall into bin 0 and their voxels are never counted
template <bool VEC>
__device__ __forceinline__ float4 mf_load(const float *__restrict__ plane, const MfTask &t, int n) {
    const float nan = __builtin_nanf("");
    if (VEC && t.mode == 1) return *reinterpret_cast<const float4 *>(plane + t.roff + t.gz0);
    float r[4] = {nan, nan, nan, nan};
    if (t.mode != 0) {
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int g = t.gz0 + e;
            if (e < t.ne && g <= n) r[e] = plane[t.roff + (g == n ? 0 : g)];
        }
    }
    return make_float4(r[0], r[1], r[2], r[3]);
}

// the number of thresholds <= v, with no chain of dependent table reads.  c: 8 values every lane shares (registers).  Up to 8
// thresholds (FINE false): c holds them, NaN beyond the last (never <= v), and the count is the bin.  More (FINE true): c[j] =
// thr[8 j + 7], the top of group j, so k = the number of whole groups at or below v; the 7 thresholds left of group k come from LDS in
// two 16-byte reads at one address per lane, and the bin is 8 k + the count among them.  thr: the table of 128 entries, NaN beyond the
// thresholds, so group 8 (v at or above all 64) reads NaN and adds nothing.
template <bool FINE>
__device__ __forceinline__ unsigned int mf_bin(float v, const float (&c)[8], const float *thr) {
    unsigned int k = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) k += v >= c[j] ? 1u : 0u;
    if (!FINE) return k;
    const float4 lo = *reinterpret_cast<const float4 *>(thr + 8 * k), hi = *reinterpret_cast<const float4 *>(thr + 8 * k + 4);
    unsigned int b = 8 * k;
    b += v >= lo.x ? 1u : 0u;
    b += v >= lo.y ? 1u : 0u;
    b += v >= lo.z ? 1u : 0u;
    b += v >= lo.w ? 1u : 0u;
    b += v >= hi.x ? 1u : 0u;
    b += v >= hi.y ? 1u : 0u;
    b += v >= hi.z ? 1u : 0u;
    return b;
}

template <bool FINE>
__device__ __forceinline__ unsigned int mf_bin4(const float4 &f, const float (&c)[8], const float *thr) {
    return mf_bin<FINE>(f.x, c, thr) | mf_bin<FINE>(f.y, c, thr) << 8 | mf_bin<FINE>(f.z, c, thr) << 16 | mf_bin<FINE>(f.w, c, thr) << 24;
}

// the 2-D maxima of a thread's four voxels in one plane: a (the voxel), by (with y + 1), bz (with z + 1), byz (all four)
struct MfPlane {
    unsigned int a[4], by[4], bz[4], byz[4];
};

__device__ __forceinline__ void mf_read_plane(const unsigned int *B, int ty, int tq, MfPlane &p) {
    const unsigned int w00 = B[ty * MF_WORDS + tq], w01 = B[ty * MF_WORDS + tq + 1];
    const unsigned int w10 = B[(ty + 1) * MF_WORDS + tq], w11 = B[(ty + 1) * MF_WORDS + tq + 1];
    unsigned int r0[5], my[5];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        r0[j] = (w00 >> (8 * j)) & 0xffu;
        my[j] = max(r0[j], (w10 >> (8 * j)) & 0xffu);
    }
    r0[4] = w01 & 0xffu;
    my[4] = max(r0[4], w11 & 0xffu);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        p.a[j] = r0[j];
        p.by[j] = my[j];
        p.bz[j] = max(r0[j], r0[j + 1]);
        p.byz[j] = max(my[j], my[j + 1]);
    }
}

// mesh: n * n rows of `pitch` floats.  grid (z tiles, y tiles, x chunks); partial: one row of MF_OUT uint32 per workgroup, class-major
// (vertices, edges, faces, voxels), bin b = the elements whose maximum has exactly b thresholds at or below it.
template <bool VEC, bool FINE>
__global__ __launch_bounds__(BLK) void mf_count(const float *__restrict__ mesh, int n, int64_t pitch, const float *__restrict__ table,
                                                unsigned int *__restrict__ partial) {
    __shared__ unsigned int hist[MF_OUT * 32];
    __shared__ unsigned int bins[2][MF_TASKS];
    __shared__ __attribute__((aligned(16))) float thr[MF_TABLE];
    const int tid = threadIdx.x;
    for (int i = tid; i < MF_OUT * 32; i += BLK) hist[i] = 0;
    if (tid < MF_TABLE) thr[tid] = table[tid];
    float c[8];
#pragma unroll
    for (int j = 0; j < 8; j++) c[j] = table[FINE ? 8 * j + 7 : j];
    const int z0 = blockIdx.x * MF_TZ, y0 = blockIdx.y * MF_TY, x0 = blockIdx.z * MF_XC, x1 = min(x0 + MF_XC, n);

    MfTask task[2];
    bool has[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int id = tid + k * BLK;
        has[k] = id < MF_TASKS;
        const int r = id / MF_WORDS, q = id % MF_WORDS;
        const int gy = y0 + r;
        task[k].roff = (int64_t)(gy == n ? 0 : gy) * pitch;
        task[k].gz0 = z0 + 4 * q;
        task[k].ne = q == MF_WORDS - 1 ? 1 : 4;
        task[k].mode = (!has[k] || gy > n || task[k].gz0 > n) ? 0 : ((VEC && task[k].ne == 4 && task[k].gz0 + 4 <= n) ? 1 : 2);
    }
    const int64_t plane_floats = (int64_t)n * pitch;
    auto load = [&](int gx, float4 &f0, float4 &f1) {
        const float *plane = mesh + (int64_t)(gx == n ? 0 : gx) * plane_floats;
        f0 = mf_load<VEC>(plane, task[0], n);
        if (has[1]) f1 = mf_load<VEC>(plane, task[1], n);
    };
    auto store = [&](unsigned int *B, const float4 &f0, const float4 &f1) {
        B[tid] = mf_bin4<FINE>(f0, c, thr);
        if (has[1]) B[tid + BLK] = mf_bin4<FINE>(f1, c, thr);
    };

    float4 f0, f1 = make_float4(0.f, 0.f, 0.f, 0.f);
    load(x0, f0, f1);
    __syncthreads();                         // the table and the zeroed bins
    store(bins[0], f0, f1);
    load(x0 + 1, f0, f1);                    // x0 < n: plane x0 + 1 exists (plane n is plane 0)
    __syncthreads();

    const int ty = tid / (MF_TZ / 4), tq = tid % (MF_TZ / 4), lane32 = tid & 31;
    const bool rowok = y0 + ty < n;
    MfPlane C, N;
    mf_read_plane(bins[0], ty, tq, C);
    unsigned int *const h0 = hist + lane32, *const h1 = h0 + MF_BINS * 32, *const h2 = h1 + MF_BINS * 32, *const h3 = h2 + MF_BINS * 32;

    for (int x = x0; x < x1; x++) {
        unsigned int *B = bins[(x - x0 + 1) & 1];
        store(B, f0, f1);                    // plane x + 1
        if (x + 1 < x1) load(x + 2, f0, f1); // x + 2 <= x1 <= n
        __syncthreads();                     // one barrier per plane: the buffer written next was last read before this barrier
        mf_read_plane(B, ty, tq, N);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (rowok && z0 + 4 * tq + j < n) {
                atomicAdd(h3 + C.a[j] * 32, 1u);
                atomicAdd(h2 + max(C.a[j], N.a[j]) * 32, 1u);
                atomicAdd(h2 + C.by[j] * 32, 1u);
                atomicAdd(h2 + C.bz[j] * 32, 1u);
                atomicAdd(h1 + C.byz[j] * 32, 1u);
                atomicAdd(h1 + max(C.bz[j], N.bz[j]) * 32, 1u);
                atomicAdd(h1 + max(C.by[j], N.by[j]) * 32, 1u);
                atomicAdd(h0 + max(C.byz[j], N.byz[j]) * 32, 1u);
            }
        }
        C = N;
    }
    __syncthreads();
    const int64_t wg = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    for (int t = tid; t < MF_OUT; t += BLK) {
        unsigned int s = 0;
        for (int c = 0; c < 32; c++) s += hist[t * 32 + ((c + t) & 31)];     // rotated: the lanes start on different banks
        partial[wg * MF_OUT + t] = s;
    }
}

// out[t] += the sum over the workgroups' rows of partial[.][t]: 64-bit integer adds, exact in any order.  Blocks of 320 threads.
__global__ __launch_bounds__(320) void mf_count_final(const unsigned int *__restrict__ partial, int64_t nwg, unsigned long long *__restrict__ out) {
    const int t = threadIdx.x;
    if (t >= MF_OUT) return;
    unsigned long long s = 0;
    for (int64_t w = blockIdx.x; w < nwg; w += gridDim.x) s += partial[w * MF_OUT + t];
    if (s) atomicAdd(out + t, s);
}

// partial[b] = sum x, partial[gridDim.x + b] = sum x^2 over the rows b, b + gridDim.x, ... in float64; every product x * x of two
// float32 is exact in float64.  VEC: float4 loads (rows aligned to 16 bytes), the cells beyond the last full float4 one by one.
template <bool VEC>
__global__ __launch_bounds__(BLK) void mf_moments(const float *__restrict__ mesh, int n, int64_t pitch, double *__restrict__ partial) {
    __shared__ double lds[BLK];
    const int64_t rows = (int64_t)n * n;
    double s1 = 0.0, s2 = 0.0;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const float *src = mesh + row * pitch;
        int c0 = 0;
        if (VEC) {
            c0 = n & ~3;
            for (int c = 4 * threadIdx.x; c < c0; c += 4 * BLK) {
                const float4 v = *reinterpret_cast<const float4 *>(src + c);
                const double a = v.x, b = v.y, d = v.z, e = v.w;
                s1 += a, s2 += a * a;
                s1 += b, s2 += b * b;
                s1 += d, s2 += d * d;
                s1 += e, s2 += e * e;
            }
        }
        for (int c = c0 + threadIdx.x; c < n; c += BLK) {
            const double a = src[c];
            s1 += a, s2 += a * a;
        }
    }
    const double t1 = block_sum(s1, lds), t2 = block_sum(s2, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = t1, partial[gridDim.x + blockIdx.x] = t2;
}

// out[q] = the sum of partial[q * count .. ] in a fixed order: strided per thread, then the tree; one workgroup, q = blockIdx.x
__global__ __launch_bounds__(BLK) void mf_moments_final(const double *__restrict__ partial, int count, double *__restrict__ out) {
    __shared__ double lds[BLK];
    double s = 0.0;
    for (int i = threadIdx.x; i < count; i += BLK) s += partial[(int64_t)blockIdx.x * count + i];
    const double t = block_sum(s, lds);
    if (threadIdx.x == 0) out[blockIdx.x] = t;
}

int mf_check_mesh(const char *who, const float *mesh, int n, int pitch) {
    if (!mesh) return fail("%s: null mesh", who);
    if (n < 2 || n > 32767) return fail("%s: mesh size %d out of range (2 .. 32767)", who, n);
    if (pitch < n) return fail("%s: pitch %d is smaller than the mesh size %d", who, pitch, n);
    if ((uintptr_t)mesh % 4) return fail("%s: the mesh is not aligned to 4 bytes", who);
    return 0;
}

}  // namespace

extern "C" {

int abacus_mf_check_memory(int n, int64_t np) {
    static const char *who = "abacus_mf_check_memory";
    if (n < 2 || n > 32767) return fail("%s: mesh size %d out of range (2 .. 32767)", who, n);
    if (n & 1) return fail("%s: odd mesh size %d (the half spectrum is laid out for an even mesh)", who, n);
    if (np < 0) return fail("%s: negative particle count", who);
    ABACUS_ENTER();
    // the spectrum (smoothed in place), the two work meshes of an interlaced deposit + transform (or the work area of the C2R), the
    // packed copy of the particles and the lists of the deposit (about one position's worth again)
    auto bytes_of = [=](int m) { return 3 * padded_bytes(m) + (size_t)np * 24; };
    return check_memory(who, n, 2, bytes_of);
}

int abacus_mf_counts_dev(const float *mesh, int n, int pitch, const float *thresholds_host, int nthr, int64_t *counts_host) {
    static const char *who = "abacus_mf_counts_dev";
    if (!thresholds_host || !counts_host) return fail("%s: null argument", who);
    ABACUS_TRY(mf_check_mesh(who, mesh, n, pitch));
    if (nthr < 1 || nthr > MF_MAX_THR) return fail("%s: %d thresholds (1 .. %d)", who, nthr, MF_MAX_THR);
    for (int t = 0; t < nthr; t++) {
        if (!std::isfinite(thresholds_host[t])) return fail("%s: threshold %d is not finite", who, t);
        if (t && !(thresholds_host[t] > thresholds_host[t - 1])) return fail("%s: the thresholds must increase strictly (in float32)", who);
    }
    ABACUS_ENTER();
    std::vector<float> table(MF_TABLE, std::nanf(""));
    for (int t = 0; t < nthr; t++) table[t] = thresholds_host[t];
    const dim3 grid((unsigned int)ceil_div(n, MF_TZ), (unsigned int)ceil_div(n, MF_TY), (unsigned int)ceil_div(n, MF_XC)), block(BLK);
    const int64_t nwg = (int64_t)grid.x * grid.y * grid.z;
    Scratch sc;
    float *dtable = nullptr;
    unsigned int *partial = nullptr;
    unsigned long long *out = nullptr;
    ABACUS_TRY(sc.get(&dtable, MF_TABLE * sizeof(float)));
    ABACUS_TRY(sc.get(&partial, (size_t)nwg * MF_OUT * sizeof(unsigned int)));
    ABACUS_TRY(sc.get(&out, MF_OUT * sizeof(unsigned long long)));
    HIP_TRY(hipMemcpyAsync(dtable, table.data(), MF_TABLE * sizeof(float), hipMemcpyHostToDevice, stream()));
    HIP_TRY(hipMemsetAsync(out, 0, MF_OUT * sizeof(unsigned long long), stream()));
    const bool vec = pitch % 4 == 0 && (uintptr_t)mesh % 16 == 0, fine = nthr > 8;
#define MF_COUNT(V, F) ABACUS_LAUNCH("mf_count", (mf_count<V, F>), grid, block, 0, mesh, n, (int64_t)pitch, (const float *)dtable, partial)
    if (vec && fine) MF_COUNT(true, true);
    else if (vec) MF_COUNT(true, false);
    else if (fine) MF_COUNT(false, true);
    else MF_COUNT(false, false);
#undef MF_COUNT
    ABACUS_LAUNCH("mf_count_final", mf_count_final, dim3((unsigned int)std::min<int64_t>(nwg, 256)), dim3(320), 0,
                  (const unsigned int *)partial, nwg, out);
    unsigned long long host[MF_OUT];
    HIP_TRY(hipMemcpyAsync(host, out, sizeof(host), hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipStreamSynchronize(stream()));
    // every voxel owns 1 vertex, 3 edges, 3 faces and itself: the bins of a class must add up to that many elements
    const int64_t N = (int64_t)n * n * n, owned[4] = {N, 3 * N, 3 * N, N};
    for (int c = 0; c < 4; c++) {
        int64_t all = 0, above = 0;
        for (int b = 0; b < MF_BINS; b++) all += (int64_t)host[c * MF_BINS + b];
        if (all != owned[c]) return fail("%s: class %d holds %lld elements, expected %lld", who, c, (long long)all, (long long)owned[c]);
        for (int t = nthr - 1; t >= 0; t--) {       // suffix sums: an element is inside threshold t iff its bin is t + 1 or higher
            above += (int64_t)host[c * MF_BINS + t + 1];
            counts_host[(size_t)c * nthr + t] = above;
        }
    }
    return 0;
}

int abacus_mf_moments_dev(const float *mesh, int n, int pitch, double *out2_host) {
    static const char *who = "abacus_mf_moments_dev";
    if (!out2_host) return fail("%s: null argument", who);
    ABACUS_TRY(mf_check_mesh(who, mesh, n, pitch));
    ABACUS_ENTER();
    const int grid = (int)std::min<int64_t>((int64_t)n * n, MOM_GRID);
    Scratch sc;
    double *partial = nullptr, *out = nullptr;
    ABACUS_TRY(sc.get(&partial, (size_t)2 * grid * sizeof(double)));
    ABACUS_TRY(sc.get(&out, 2 * sizeof(double)));
    if (pitch % 4 == 0 && (uintptr_t)mesh % 16 == 0)
        ABACUS_LAUNCH("mf_moments", (mf_moments<true>), dim3(grid), dim3(BLK), 0, mesh, n, (int64_t)pitch, partial);
    else
        ABACUS_LAUNCH("mf_moments", (mf_moments<false>), dim3(grid), dim3(BLK), 0, mesh, n, (int64_t)pitch, partial);
    ABACUS_LAUNCH("mf_moments_final", mf_moments_final, dim3(2), dim3(BLK), 0, (const double *)partial, grid, out);
    HIP_TRY(hipMemcpyAsync(out2_host, out, 2 * sizeof(double), hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipStreamSynchronize(stream()));
    return 0;
}

int abacus_mf_smooth_spectrum_dev(void *spec_padded, int n, double Lbox, double R) {
    static const char *who = "abacus_mf_smooth_spectrum_dev";
    if (!spec_padded) return fail("%s: null spectrum", who);
    if (n < 2 || n > 32767) return fail("%s: mesh size %d out of range (2 .. 32767)", who, n);
    if (n & 1) return fail("%s: odd mesh size %d (the half spectrum is laid out for an even mesh)", who, n);
    if ((uintptr_t)spec_padded % 16) return fail("%s: the spectrum is not aligned to 16 bytes", who);
    if (!(Lbox > 0) || !std::isfinite(Lbox)) return fail("%s: Lbox must be positive", who);
    if (!(R >= 0) || !std::isfinite(R)) return fail("%s: R must be finite and not negative, got %g", who, R);
    ABACUS_ENTER();
    return smooth_c2r_inplace((float *)spec_padded, n, Lbox, R);
}

}  // extern "C"
