// Galaxy-galaxy lensing on the periodic box (abacus_lens_*, include/abacus_hip.h): the projected mass sums around galaxies that
// the excess surface density Delta Sigma(R) is built from.  gfx950 only.
//
// The line of sight is one box axis and the projection runs along the whole box, so the problem is two-dimensional: particles
// and galaxies are pairs of transverse float32 coordinates.  The 10^7 .. 10^8 matter particles of a fit never change, only the
// ~10^6 galaxies do: the particles are sorted ONCE into a 2-D periodic cell grid sized for a reach of rmax and stay in HBM
// behind a handle (8 bytes per particle, 12 with masses); a profile call sorts its galaxies into the same grid and walks.
//   per (galaxy, particle) pair, float32, the expressions of sphere_count's cylinders without the dz test: d = g - p per
//   component, one -+L when |d| > L/2; r2 = dx dx + dy dy left to right (no FMA: -ffp-contract=off); e2[j] = R_j R_j as a float32
//   product; row 0 is the inner disc r2 < e2[0], row b + 1 the bin e2[b] <= r2 < e2[b + 1]; r2 >= e2[nb] is dropped.
//   out: npairs[row] exact, wsum[row] = sum of (double)gw (double)pm in float64 (the product of two float32 values is exact).
// No reference code stands behind it: tests/lensing_statement.py is the judge.
//
//   the handle       LensHandle: pxy | pm | pstart in HBM, sum(pm) in float64
//   the 2-D sort     lens_keys (key = cy ncx + cx), rocPRIM radix sort of (key, index), lens_gather, lens_starts
//   the walk         lens_walk: a lane per galaxy, the particles of a neighbour cell by scalar loads, rows in LDS
//   host             tables of a set of edges, create / profile / free / stats / mass, the C ABI
#include <cmath>
#include <cstring>
#include <set>
#include <type_traits>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "../../include/abacus_hip.h"
#include "common.hpp"

using namespace abacus;

namespace {

constexpr int LB = 256;               // threads per workgroup of the walk: four waves, each with galaxies of its own
constexpr int LENS_MAX_BINS = 32;     // 33 rows
constexpr int LENS_MAX_CELLS = 1024;  // per dimension: the key cy ncx + cx stays below 2^20
constexpr int LENS_MAX_LUT = 1024;    // cells of the row look-up
constexpr int LENS_TILE = 8;          // particles per scalar load of the walk

// fractional position in the box, periodic, the expression of the pair counters' grid: any coordinate interval works
__device__ __forceinline__ int lens_cell_coord(float v, int nc, float inv_box) {
    float f = v * inv_box;
    f -= floorf(f);
    const int c = (int)(f * (float)nc);
    return c >= nc ? nc - 1 : (c < 0 ? 0 : c);
}

// ---------------------------------------------------------------------------------------------------- the 2-D sort ----
template <typename T>
__global__ void lens_cast(const T *__restrict__ src, float *__restrict__ dst, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = (float)src[i];
}

__global__ void lens_keys(const float *__restrict__ x, const float *__restrict__ y, int64_t n, int nc, float inv_box,
                          unsigned int *__restrict__ keys, unsigned int *__restrict__ idx) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        keys[i] = (unsigned int)(lens_cell_coord(y[i], nc, inv_box) * nc + lens_cell_coord(x[i], nc, inv_box));
        idx[i] = (unsigned int)i;
    }
}

// the set in cell order (ties in input order: the radix sort is stable, so the packed arrays do not depend on the run)
template <bool W>
__global__ void lens_gather(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ w, int64_t n,
                            const unsigned int *__restrict__ idx, float2 *__restrict__ sxy, float *__restrict__ sw) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        const unsigned int i = idx[s];
        sxy[s] = make_float2(x[i], y[i]);
        if (W) sw[s] = w[i];
    }
}

// start[c] = number of sorted keys below c, c = 0 .. ncell
__global__ void lens_starts(const unsigned int *__restrict__ keys, int64_t n, int ncell, int *__restrict__ start) {
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c <= ncell; c += gridDim.x * blockDim.x) {
        int64_t lo = 0, hi = n;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)keys[mid] < (int64_t)c) lo = mid + 1;
            else hi = mid;
        }
        start[c] = (int)lo;
    }
}

// sum of the masses in float64: a wave's share by shuffles, one atomic per wave
__global__ void lens_mass_sum(const float *__restrict__ m, int64_t n, double *__restrict__ out) {
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) s += (double)m[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0 && s != 0.0) atomicAdd(out, s);
}

// ---------------------------------------------------------------------------------------------------------- the walk ----
// Mapping.  Neither side is sparse here: a 2-D cell of side >= rmax holds thousands of particles and tens to hundreds of
// galaxies, nobody reads a per-galaxy result, and there are up to 33 rows of an exact count and a float64 sum.  So a LANE owns
// a galaxy (x, y and its weight as a double stay in registers) and a WAVE owns 64 galaxies of one cell; the particles of one
// neighbour cell are the same for every lane, their index is wave-uniform, and they come by SCALAR loads (s_load of (x, y) and of
// the mass) - no staging in LDS, no barrier in the loop, and the waves of a workgroup run independently.  A job is (galaxy cell,
// neighbour cell); persistent workgroups stride over the jobs, the waves of a workgroup over the cell's slices of 64 galaxies.
// Row of a pair: the float32 bit pattern of r2, shifted, indexes a small table whose cells hold the number of edges below the
// cell and the one edge inside it ({row, edge}, one 8-byte LDS read; the host picks the shift so that no cell holds two edges,
// `multi` is the rare set of edges for which no shift does: the lane then walks on through e2).  r2 >= 0, so the bit pattern is
// monotone in r2; the compare against the cell's edge is the contract's own float32 compare, the table only says which.
// Reduction (both built, the first is used, the second is the comparator `lens_shared_rows`; profiles/lensing/README.md):
//   private   every lane adds into a column of its own, acc[wave][row][lane]: the bank is the lane's whatever the row, so the
//             LDS atomics (ds_add_u32, ds_add_f64) never conflict and never contend; rows x 768 bytes per wave, rows x 256
//             with unit weights and masses, when no sums are kept;
//   shared    one set of rows per workgroup, an LDS atomic per pair as in pair_count_w: lanes in the same bin serialise.
// A private 32-bit count is flushed to the 64-bit global rows before any column can have seen 2^31 candidates.
#define LENS_CONSTANT __attribute__((address_space(4)))

struct LutCell {
    int row;      // edges in the cells below
    float edge;   // e2[row] (+inf behind the last edge): the one edge that may lie inside this cell
};

struct LensArgs {
    int nc, nnb, rows, multi;          // cells per dimension, neighbour cells per cell (9 | 1), nb + 1
    float box, half, e2max;
    int sh, off, nlut;                 // table cell of r2: clamp((bits(r2) >> sh) - off, 0, nlut - 1)
    const LutCell *lut;                // nlut cells
    const float *e2;                   // rows + 1: the squared edges and +inf
    const float2 *gxy, *pxy;           // both sets in cell order
    const float *gw, *pm;              // NULL: unit weight, unit mass
    const int *gstart, *pstart;
    unsigned long long *npairs;        // [rows]
    double *wsum;                      // [rows]
    unsigned long long *evaluated;
};

template <bool SUMS, bool MASS, bool SHARED>
__global__ __launch_bounds__(LB) void lens_walk(LensArgs a) {
    extern __shared__ double lens_lds[];   // doubles first: the base is 16-byte aligned, every part below at least 8
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rows = a.rows;
    // shared: sum[rows] | cnt64[rows] | lut | e2      private: sum[4][rows][64] (with sums only) | lut | e2 | cnt[4][rows][64]
    const int nacc = SHARED ? rows : (LB / 64) * rows * 64;
    const int nsum = (SHARED || SUMS) ? nacc : 0;   // counts alone: a third of the LDS, three times the resident waves
    double *sum = lens_lds;
    unsigned long long *cnt64 = reinterpret_cast<unsigned long long *>(lens_lds + nsum);   // shared only
    LutCell *lut = reinterpret_cast<LutCell *>(lens_lds + nsum + (SHARED ? rows : 0));
    float *e2 = reinterpret_cast<float *>(lut + a.nlut);
    unsigned int *cnt = reinterpret_cast<unsigned int *>(e2 + ((rows + 2) & ~1));            // private only
    for (int q = tid; q < nacc; q += LB) {
        if (SHARED || SUMS) sum[q] = 0.0;
        if (SHARED) cnt64[q] = 0ull;
        else cnt[q] = 0u;
    }
    for (int q = tid; q < a.nlut; q += LB) lut[q] = a.lut[q];
    for (int q = tid; q <= rows; q += LB) e2[q] = a.e2[q];
    __syncthreads();
    // this wave's columns (private) or the workgroup's rows (shared)
    double *msum = SHARED ? sum : sum + (wave * rows) * 64 + lane;
    unsigned int *mcnt = cnt + (wave * rows) * 64 + lane;
    // the particle arrays are only read here and were written by earlier launches: read through the constant address space, the
    // loads of a wave-uniform index go through the scalar unit
    const LENS_CONSTANT float *pxy = (const LENS_CONSTANT float *)reinterpret_cast<const float *>(a.pxy);   // x, y interleaved
    const LENS_CONSTANT float *pm = (const LENS_CONSTANT float *)a.pm;
    const int njob = a.nc * a.nc * a.nnb;
    const int w3 = a.nnb == 9 ? 3 : 1;
    unsigned long long n_eval = 0;
    unsigned int pending = 0;            // candidates a private column may have seen since the last flush (a bound, the same in every wave)

    // the rows of the workgroup to the global ones: a wave per row, its lanes over the columns, one pair of atomics per row
    auto flush = [&]() {
        __syncthreads();
        for (int r = wave; r < rows; r += LB / 64) {
            unsigned long long c = 0;
            double s = 0.0;
            if (SHARED) {
                if (lane == 0) {
                    c = cnt64[r], s = sum[r];
                    cnt64[r] = 0ull, sum[r] = 0.0;
                }
            } else {
                for (int w = 0; w < LB / 64; w++) {
                    const int q = (w * rows + r) * 64 + lane;
                    c += cnt[q], cnt[q] = 0u;
                    if (SUMS) s += sum[q], sum[q] = 0.0;
                }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64), s += __shfl_xor(s, off, 64);
            }
            if (lane == 0 && c) {
                atomicAdd(&a.npairs[r], c);
                if (SUMS) atomicAdd(&a.wsum[r], s);
            }
        }
        __syncthreads();
    };

    for (int job = blockIdx.x; job < njob; job += gridDim.x) {
        const int c1 = job / a.nnb, k = job - c1 * a.nnb;
        const int g0 = a.gstart[c1], g1 = a.gstart[c1 + 1];
        if (g0 == g1) continue;
        const int cy = c1 / a.nc, cx = c1 - cy * a.nc;
        int nx = cx + k % w3 - (w3 >> 1), ny = cy + k / w3 - (w3 >> 1);
        nx = nx < 0 ? nx + a.nc : (nx >= a.nc ? nx - a.nc : nx);
        ny = ny < 0 ? ny + a.nc : (ny >= a.nc ? ny - a.nc : ny);
        const int c2 = ny * a.nc + nx;
        const int j0 = a.pstart[c2], j1 = a.pstart[c2 + 1];
        if (j0 == j1) continue;
        const int nslice = (g1 - g0 + 63) >> 6;
        for (int s0 = 0; s0 < nslice; s0 += LB / 64) {   // (workgroup-uniform: the flush inside has barriers)
            if (!SHARED) {
                if (pending + (unsigned int)(j1 - j0) >= 0x80000000u) flush(), pending = 0;
                pending += (unsigned int)(j1 - j0);       // j1 - j0 <= n < 2^31
            }
            const int s = s0 + wave;
            if (s >= nslice) continue;
            const int gi = g0 + s * 64 + lane;
            const bool live = gi < g1;
            const float2 g = live ? a.gxy[gi] : make_float2(0.f, 0.f);
            double gwd = 1.0;
            if (SUMS && a.gw && live) gwd = (double)a.gw[gi];
            if (lane == 0) n_eval += (unsigned long long)min(64, g1 - g0 - s * 64) * (unsigned long long)(j1 - j0);
            // The row of one pair, -1 when the pair is dropped.  The look-up runs for every lane (its cell index is clamped into
            // the table) and has no branch, so the LDS reads of a tile's pairs are issued together; only the adds are predicated
            auto row_of = [&](auto MULTI, float px, float py) -> int {
                // min_image, branch-free: its single addition of -+L, or of 0 (which leaves d, and -0 as +0: the same square)
                float dx = g.x - px, dy = g.y - py;
                dx += (dx > a.half ? -a.box : 0.f) + (dx < -a.half ? a.box : 0.f);   // (one of the two is 0: the sum is -L, +L or 0)
                dy += (dy > a.half ? -a.box : 0.f) + (dy < -a.half ? a.box : 0.f);
                const float r2 = dx * dx + dy * dy;
                const bool in = live && r2 < a.e2max;
                int c = (int)(__float_as_uint(r2) >> a.sh) - a.off;
                c = max(0, min(c, a.nlut - 1));
                const LutCell t = lut[c];
                int row = t.row + (r2 >= t.edge ? 1 : 0);
                if (decltype(MULTI)::value && in)
                    while (row < rows && r2 >= e2[row]) row++;
                // (a pair that is in has row <= nb already: the adds stay inside the rows; the OR keeps the read out of a branch)
                return min(row, rows - 1) | (in ? 0 : -1);
            };
            auto add = [&](int row, float m) {
                if (row < 0) return;
                if (SHARED) {
                    atomicAdd(&cnt64[row], 1ull);
                    if (SUMS) atomicAdd(&msum[row], MASS ? gwd * (double)m : gwd);
                } else {
                    atomicAdd(&mcnt[row * 64], 1u);
                    if (SUMS) atomicAdd(&msum[row * 64], MASS ? gwd * (double)m : gwd);
                }
            };
            // tiles of LENS_TILE particles: their coordinates (and masses) arrive in scalar registers by one wide load each, the
            // latency of which is paid once per tile; the index is wave-uniform
            auto walk = [&](auto MULTI) {
                int j = j0;
                for (; j + LENS_TILE <= j1; j += LENS_TILE) {
                    float tx[LENS_TILE], ty[LENS_TILE], tm[LENS_TILE];
                    int row[LENS_TILE];
                    const LENS_CONSTANT float *txy = pxy + 2 * (int64_t)j, *tmm = pm + j;   // constant offsets from here: one wide load each
#pragma unroll
                    for (int q = 0; q < LENS_TILE; q++) {
                        tx[q] = txy[2 * q], ty[q] = txy[2 * q + 1];
                        tm[q] = MASS ? tmm[q] : 1.f;
                    }
#pragma unroll
                    for (int q = 0; q < LENS_TILE; q++) row[q] = row_of(MULTI, tx[q], ty[q]);
#pragma unroll
                    for (int q = 0; q < LENS_TILE; q++) add(row[q], tm[q]);
                }
                for (; j < j1; j++) add(row_of(MULTI, pxy[2 * (int64_t)j], pxy[2 * (int64_t)j + 1]), MASS ? pm[j] : 1.f);
            };
            if (a.multi) walk(std::true_type());
            else walk(std::false_type());
        }
    }
    flush();
    if (lane == 0 && n_eval) atomicAdd(a.evaluated, n_eval);
}

// --------------------------------------------------------------------------------------------------------------- host ----
struct LensHandle {
    int64_t n = 0;
    float box = 0.f, rmax = 0.f;
    int nc = 1;
    bool has_mass = false;
    double mass = 0.0;          // sum(pm) in float64; n without masses
    DevBuf pxy, pm, pstart;     // float2[n] | float[n] | int[nc nc + 1], in cell order
};
std::set<LensHandle *> g_handles;   // the live ones: a freed or foreign pointer is refused, not followed

struct LensWork {   // per-call temporaries of the galaxy side, kept between calls
    DevBuf cols, wts, keys, keys2, idx, idx2, tmp, gxy, gw, gstart, tables, out;
} g_lens;

struct LensStats {
    unsigned long long evaluated = 0;
    int nc = 0;
} g_lens_stats;

int lens_where(int pos_dtype) { return pos_dtype == ABACUS_F32 ? 1 : (pos_dtype == ABACUS_F64 ? 2 : -1); }

int lens_blocks(int64_t n) { return (int)std::min<int64_t>(std::max<int64_t>(ceil_div(n, 256), 1), 2048); }

// the grid of a reach: cells of side >= rmax / 0.9999, at least three per dimension or one (a cell that is its own neighbour)
int lens_ncells(float boxsize, float rmax) {
    int nc = (int)floorf(boxsize / rmax * 0.9999f);
    nc = std::min(nc, LENS_MAX_CELLS);
    return nc < 3 ? 1 : nc;
}

// caller columns -> float32 device columns (where = 0: host float32; 1: device float32, read in place; 2: device float64, cast)
// and the float32 weights (host: uploaded; device: read in place).  n > 0
int lens_stage(const void *const src[2], const float *w, int where, int64_t n, DevBuf &cols, DevBuf &wts, const float *x[2], const float *&wd) {
    if (where == 1) {
        x[0] = (const float *)src[0], x[1] = (const float *)src[1];
    } else {
        ABACUS_TRY(cols.reserve(2 * (size_t)n * 4));
        for (int d = 0; d < 2; d++) {
            float *dst = cols.as<float>() + (size_t)d * n;
            x[d] = dst;
            if (where == 2) ABACUS_LAUNCH("lens_cast", lens_cast<double>, dim3(lens_blocks(n)), dim3(256), 0, (const double *)src[d], dst, n);
            else HIP_TRY(hipMemcpyAsync(dst, src[d], (size_t)n * 4, hipMemcpyHostToDevice, stream()));
        }
    }
    wd = w;
    if (w && where == 0) {
        ABACUS_TRY(wts.reserve((size_t)n * 4));
        HIP_TRY(hipMemcpyAsync(wts.p, w, (size_t)n * 4, hipMemcpyHostToDevice, stream()));
        wd = wts.as<float>();
    }
    return 0;
}

// (x, y[, w]) into cell order on the nc x nc grid: sxy, sw (w != NULL) and start[nc nc + 1].  n > 0
int lens_sort(const char *who, const float *const x[2], const float *w, int64_t n, int nc, float boxsize, DevBuf &keys, DevBuf &keys2, DevBuf &idx,
              DevBuf &idx2, DevBuf &tmp, float2 *sxy, float *sw, int *start) {
    const int ncell = nc * nc, nblk = lens_blocks(n);
    ABACUS_TRY(keys.reserve((size_t)n * 4));
    ABACUS_TRY(keys2.reserve((size_t)n * 4));
    ABACUS_TRY(idx.reserve((size_t)n * 4));
    ABACUS_TRY(idx2.reserve((size_t)n * 4));
    ABACUS_LAUNCH("lens_keys", lens_keys, dim3(nblk), dim3(256), 0, x[0], x[1], n, nc, 1.0f / boxsize, keys.as<unsigned int>(), idx.as<unsigned int>());
    int end_bit = 1;
    while ((1 << end_bit) < ncell) end_bit++;
    size_t tmp_bytes = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, keys.as<unsigned int>(), keys2.as<unsigned int>(), idx.as<unsigned int>(),
                                             idx2.as<unsigned int>(), (int)n, 0, end_bit, stream());
    ABACUS_TRY(tmp.reserve(std::max<size_t>(tmp_bytes, 16)));
    prof_begin("lens_sort");
    const hipError_t sorted = hipcub::DeviceRadixSort::SortPairs(tmp.p, tmp_bytes, keys.as<unsigned int>(), keys2.as<unsigned int>(), idx.as<unsigned int>(),
                                                                 idx2.as<unsigned int>(), (int)n, 0, end_bit, stream());
    prof_end("lens_sort");
    if (sorted != hipSuccess) return fail("%s: radix sort failed (%s)", who, hipGetErrorString(sorted));
    if (w) ABACUS_LAUNCH("lens_gather", lens_gather<true>, dim3(nblk), dim3(256), 0, x[0], x[1], w, n, idx2.as<unsigned int>(), sxy, sw);
    else ABACUS_LAUNCH("lens_gather", lens_gather<false>, dim3(nblk), dim3(256), 0, x[0], x[1], w, n, idx2.as<unsigned int>(), sxy, sw);
    ABACUS_LAUNCH("lens_starts", lens_starts, dim3((unsigned int)std::min<int64_t>(ceil_div(ncell + 1, 256), 4096)), dim3(256), 0, keys2.as<unsigned int>(), n,
                  ncell, start);
    return 0;
}

int lens_check_sets(const char *who, const void *x, const void *y, int64_t n, int where, const char *what) {
    if (where < 0) return fail("%s: pos_dtype must be ABACUS_F32 or ABACUS_F64", who);
    if (n < 0 || n >= ((int64_t)1 << 31)) return fail("%s: %s must lie in [0, 2^31)", who, what);
    if (n > 0 && (!x || !y)) return fail("%s: null argument", who);
    return 0;
}

int lens_create(const char *who, const void *px, const void *py, const float *pm, int64_t n, int where, float boxsize, float rmax,
                abacus_lens **handle) {
    if (!handle) return fail("%s: null argument (handle)", who);
    *handle = nullptr;
    ABACUS_TRY(lens_check_sets(who, px, py, n, where, "n"));
    if (!(boxsize > 0)) return fail("%s: boxsize must be positive", who);
    if (!(rmax > 0)) return fail("%s: rmax must be positive", who);
    if (rmax > 0.5f * boxsize) return fail("%s: rmax exceeds half the box (minimum image not unique)", who);
    ABACUS_ENTER();
    LensHandle *h = new LensHandle;
    h->n = n, h->box = boxsize, h->rmax = rmax, h->nc = lens_ncells(boxsize, rmax), h->has_mass = pm != nullptr && n > 0;
    h->mass = (double)n;
    auto build = [&]() -> int {
        if (n == 0) return 0;
        // the particle side's temporaries go back when the handle stands (10^8 particles: 3 GB of keys, indices and columns)
        DevBuf cols, wts, keys, keys2, idx, idx2, tmp, msum;
        auto body = [&]() -> int {
            const void *src[2] = {px, py};
            const float *x[2], *w;
            ABACUS_TRY(lens_stage(src, pm, where, n, cols, wts, x, w));
            ABACUS_TRY(h->pxy.reserve((size_t)n * 8));
            if (w) ABACUS_TRY(h->pm.reserve((size_t)n * 4));
            ABACUS_TRY(h->pstart.reserve(((size_t)h->nc * h->nc + 1) * 4));
            ABACUS_TRY(lens_sort(who, x, w, n, h->nc, boxsize, keys, keys2, idx, idx2, tmp, h->pxy.as<float2>(), h->pm.as<float>(), h->pstart.as<int>()));
            if (w) {
                ABACUS_TRY(msum.reserve(8));
                HIP_TRY(hipMemsetAsync(msum.p, 0, 8, stream()));
                ABACUS_LAUNCH("lens_mass_sum", lens_mass_sum, dim3(lens_blocks(n)), dim3(256), 0, w, n, msum.as<double>());
                HIP_TRY(hipMemcpyAsync(&h->mass, msum.p, 8, hipMemcpyDeviceToHost, stream()));
            }
            HIP_TRY(hipStreamSynchronize(stream()));
            return 0;
        };
        const int rc = body();
        if (rc != 0) (void)hipStreamSynchronize(stream());   // nothing of the stream's may still read what is freed below
        for (DevBuf *b : {&cols, &wts, &keys, &keys2, &idx, &idx2, &tmp, &msum}) (void)b->release();
        return rc;
    };
    const int rc = build();
    if (rc != 0) {
        (void)h->pxy.release(), (void)h->pm.release(), (void)h->pstart.release();
        delete h;
        return rc;
    }
    g_handles.insert(h);
    *handle = reinterpret_cast<abacus_lens *>(h);
    return 0;
}

// The row look-up of a set of squared edges (e2[0 .. nb], increasing): the largest shift - the smallest table - at which no two
// edges share a cell; else (`multi`) the finest table that fits, and the kernel walks on through the edges of a cell
struct LensTables {
    int sh = 0, off = 0, nlut = 1, multi = 0;
    std::vector<LutCell> lut;
    std::vector<float> e2;   // nb + 2: the squared edges and +inf
};
void lens_tables(const float *edges, int nb, LensTables &t) {
    t.e2.resize(nb + 2);
    for (int j = 0; j <= nb; j++) t.e2[j] = edges[j] * edges[j];
    t.e2[nb + 1] = INFINITY;
    auto bits = [&](int j) {
        uint32_t u;
        memcpy(&u, &t.e2[j], 4);
        return u;
    };
    int fit = 31;   // (bits >> 31 is 0 for every edge: one cell, always fits)
    bool found = false;
    for (int sh = 30; sh >= 0; sh--) {
        if ((int64_t)(bits(nb) >> sh) - (int64_t)(bits(0) >> sh) + 1 > LENS_MAX_LUT) break;
        fit = sh;
        bool distinct = true;
        for (int j = 1; j <= nb && distinct; j++) distinct = (bits(j) >> sh) != (bits(j - 1) >> sh);
        if (distinct) {
            found = true;
            break;
        }
    }
    t.sh = fit, t.multi = found ? 0 : 1;
    t.off = (int)(bits(0) >> fit);
    t.nlut = (int)(bits(nb) >> fit) - t.off + 1;
    t.lut.resize(t.nlut);
    int below = 0;
    for (int c = 0; c < t.nlut; c++) {
        while (below <= nb && (int)(bits(below) >> fit) - t.off < c) below++;
        t.lut[c].row = below;
        t.lut[c].edge = t.e2[below];   // below <= nb + 1
    }
}

template <bool SUMS, bool MASS, bool SHARED>
int lens_launch(const LensArgs &a) {
    const auto kernel = lens_walk<SUMS, MASS, SHARED>;
    const size_t nacc = SHARED ? (size_t)a.rows : (size_t)(LB / 64) * a.rows * 64, nsum = (SHARED || SUMS) ? nacc : 0;
    const size_t lds = nsum * 8 + (SHARED ? (size_t)a.rows * 8 : 0) + (size_t)a.nlut * 8 + (size_t)((a.rows + 2) & ~1) * 4 + (SHARED ? 0 : nacc * 4);
    if (lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int dev = 0, ncu = 256, per_cu = 1;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)kernel, LB, lds));
    const int64_t njob = (int64_t)a.nc * a.nc * a.nnb;
    const dim3 grid((unsigned int)std::min<int64_t>(njob, (int64_t)ncu * std::max(per_cu, 1)));
    ABACUS_LAUNCH("lens_walk", kernel, grid, dim3(LB), lds, a);
    return 0;
}

int lens_profile(const char *who, abacus_lens *handle, const void *gx, const void *gy, const float *gw, int64_t ng, int where, const float *edges,
                 int nb, uint64_t *npairs, double *wsum) {
    if (!handle || !edges || !npairs || !wsum) return fail("%s: null argument", who);
    ABACUS_TRY(lens_check_sets(who, gx, gy, ng, where, "ng"));
    if (nb < 1 || nb > LENS_MAX_BINS) return fail("%s: nb = %d must lie in [1, %d]", who, nb, LENS_MAX_BINS);
    if (!(edges[0] > 0.f)) return fail("%s: edges must be positive", who);
    for (int j = 1; j <= nb; j++)
        if (!(edges[j] > edges[j - 1])) return fail("%s: edges must increase", who);
    std::lock_guard<std::recursive_mutex> guard(api_mutex());   // the registry of handles is the library's state too
    LensHandle *h = reinterpret_cast<LensHandle *>(handle);
    if (!g_handles.count(h)) return fail("%s: the handle is not a live one of abacus_lens_create (freed already?)", who);
    if (edges[nb] > h->rmax) return fail("%s: the last edge %g exceeds the handle's rmax %g", who, (double)edges[nb], (double)h->rmax);
    ABACUS_ENTER();
    const int rows = nb + 1;
    memset(npairs, 0, (size_t)rows * sizeof(uint64_t));
    memset(wsum, 0, (size_t)rows * sizeof(double));
    g_lens_stats = LensStats{};
    if (h->n == 0 || ng == 0) return 0;
    LensWork &W = g_lens;
    const int nc = h->nc, ncell = nc * nc;
    const void *src[2] = {gx, gy};
    const float *x[2], *w;
    ABACUS_TRY(lens_stage(src, gw, where, ng, W.cols, W.wts, x, w));
    ABACUS_TRY(W.gxy.reserve((size_t)ng * 8));
    if (w) ABACUS_TRY(W.gw.reserve((size_t)ng * 4));
    ABACUS_TRY(W.gstart.reserve(((size_t)ncell + 1) * 4));
    ABACUS_TRY(lens_sort(who, x, w, ng, nc, h->box, W.keys, W.keys2, W.idx, W.idx2, W.tmp, W.gxy.as<float2>(), W.gw.as<float>(), W.gstart.as<int>()));
    LensTables t;
    lens_tables(edges, nb, t);
    const size_t lut_bytes = (size_t)t.nlut * sizeof(LutCell), e2_bytes = (size_t)(rows + 1) * 4;
    ABACUS_TRY(W.tables.reserve(lut_bytes + e2_bytes));
    HIP_TRY(hipMemcpyAsync(W.tables.p, t.lut.data(), lut_bytes, hipMemcpyHostToDevice, stream()));
    HIP_TRY(hipMemcpyAsync(W.tables.as<char>() + lut_bytes, t.e2.data(), e2_bytes, hipMemcpyHostToDevice, stream()));
    const size_t out_bytes = (size_t)rows * 16 + 8;   // npairs | wsum | evaluated
    ABACUS_TRY(W.out.reserve(out_bytes));
    HIP_TRY(hipMemsetAsync(W.out.p, 0, out_bytes, stream()));
    LensArgs a;
    a.nc = nc, a.nnb = nc >= 3 ? 9 : 1, a.rows = rows, a.multi = t.multi;
    a.box = h->box, a.half = h->box * 0.5f, a.e2max = t.e2[nb];
    a.sh = t.sh, a.off = t.off, a.nlut = t.nlut;
    a.lut = W.tables.as<LutCell>();
    a.e2 = reinterpret_cast<const float *>(W.tables.as<char>() + lut_bytes);
    a.gxy = W.gxy.as<float2>(), a.pxy = h->pxy.as<float2>();
    a.gw = w ? W.gw.as<float>() : nullptr, a.pm = h->has_mass ? h->pm.as<float>() : nullptr;
    a.gstart = W.gstart.as<int>(), a.pstart = h->pstart.as<int>();
    a.npairs = W.out.as<unsigned long long>();
    a.wsum = reinterpret_cast<double *>(a.npairs + rows);
    a.evaluated = a.npairs + 2 * rows;
    const bool sums = a.gw || a.pm, shared = option("lens_shared_rows") != 0;
    if (!sums) ABACUS_TRY(shared ? (lens_launch<false, false, true>(a)) : (lens_launch<false, false, false>(a)));
    else if (!a.pm) ABACUS_TRY(shared ? (lens_launch<true, false, true>(a)) : (lens_launch<true, false, false>(a)));
    else ABACUS_TRY(shared ? (lens_launch<true, true, true>(a)) : (lens_launch<true, true, false>(a)));
    std::vector<unsigned long long> out(2 * (size_t)rows + 1);
    HIP_TRY(hipMemcpyAsync(out.data(), W.out.p, out_bytes, hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipStreamSynchronize(stream()));   // (the tables above live until here)
    for (int r = 0; r < rows; r++) npairs[r] = out[r];
    if (sums) memcpy(wsum, out.data() + rows, (size_t)rows * 8);
    else
        for (int r = 0; r < rows; r++) wsum[r] = (double)npairs[r];   // unit weights and masses: the sum IS the count
    g_lens_stats.evaluated = out[2 * (size_t)rows];
    g_lens_stats.nc = nc;
    return 0;
}

}  // namespace

extern "C" int abacus_lens_create(const float *px, const float *py, const float *pm, int64_t n, float boxsize, float rmax, abacus_lens **handle) {
    return lens_create("abacus_lens_create", px, py, pm, n, 0, boxsize, rmax, handle);
}

extern "C" int abacus_lens_create_dev(const void *px, const void *py, const float *pm, int64_t n, int pos_dtype, float boxsize, float rmax,
                                      abacus_lens **handle) {
    return lens_create("abacus_lens_create_dev", px, py, pm, n, lens_where(pos_dtype), boxsize, rmax, handle);
}

extern "C" int abacus_lens_profile(abacus_lens *handle, const float *gx, const float *gy, const float *gw, int64_t ng, const float *edges, int nb,
                                   uint64_t *npairs, double *wsum) {
    return lens_profile("abacus_lens_profile", handle, gx, gy, gw, ng, 0, edges, nb, npairs, wsum);
}

extern "C" int abacus_lens_profile_dev(abacus_lens *handle, const void *gx, const void *gy, const float *gw, int64_t ng, int pos_dtype,
                                       const float *edges, int nb, uint64_t *npairs, double *wsum) {
    return lens_profile("abacus_lens_profile_dev", handle, gx, gy, gw, ng, lens_where(pos_dtype), edges, nb, npairs, wsum);
}

extern "C" int abacus_lens_mass(abacus_lens *handle, double *mass, int64_t *n) {
    std::lock_guard<std::recursive_mutex> guard(api_mutex());
    LensHandle *h = reinterpret_cast<LensHandle *>(handle);
    if (!h || !g_handles.count(h)) return fail("abacus_lens_mass: the handle is not a live one of abacus_lens_create (freed already?)");
    if (mass) *mass = h->mass;
    if (n) *n = h->n;
    return 0;
}

extern "C" int abacus_lens_free(abacus_lens *handle) {
    if (!handle) return 0;
    std::lock_guard<std::recursive_mutex> guard(api_mutex());
    LensHandle *h = reinterpret_cast<LensHandle *>(handle);
    if (!g_handles.erase(h)) return fail("abacus_lens_free: the handle is not a live one of abacus_lens_create (freed already?)");
    (void)hipStreamSynchronize(stream());
    (void)h->pxy.release(), (void)h->pm.release(), (void)h->pstart.release();
    delete h;
    return 0;
}

extern "C" int abacus_lens_stats(uint64_t *candidates, int *ncell) {
    if (candidates) *candidates = g_lens_stats.evaluated;
    if (ncell) *ncell = g_lens_stats.nc;
    return 0;
}
