// Periodic-box pair counting on MI355X (gfx950): the kernel behind compute_xirppi / compute_wp / compute_multipole.
// In the reference this arithmetic lives in the third-party Corrfunc library (Corrfunc.theory.DDrppi / DDsmu / DD,
// called at abacusnbody/analysis/tpcf_corrfunc.py:144-156,164-179,240-273,328-362 and
// scripts/emulator/generate_cfs/generate_cf.py:65-74); it is not vendored and no reference test covers it, so the
// conventions below restate Corrfunc's published behaviour and parity is pinned only against the brute-force
// counter in oracle/abacus_oracle.c (same float32 expressions, hence identical integer counts).
//
//   float32 coordinates; periodic minimum image per pair; squared separations compared with squared float32 edges;
//   r-bin b holds edges[b] <= r < edges[b+1]; DDrppi: pi-bin = int(|dz| / (pimax/npibins)), |dz| < pimax;
//   DDsmu: mu = |dz|/s, mu-bin = int(mu * nmubins/mu_max), mu < mu_max; autocorrelation counts ordered pairs (i != j).
//
// Weighted counts (abacus_paircount_weighted, Corrfunc's weight_type='pair_product' and output_ravg / _rpavg / _savg): the pairs
// of a bin are those above - npairs is bit-equal to the unweighted count - and per bin
//   wsum = sum of w_i w_j: float32 weights, the product formed in float64 (24 + 24 bits: exact), accumulated in float64;
//   rsum = sum of the separation (r | rp = sqrt(dx^2 + dy^2) | s): sqrtf - correctly rounded - of the very r^2 that chose the
//          bin, accumulated in float64;
// a missing weight array is unit weights; the weight is sorted into cells WITH its point (both sort paths); float64 atomics
// make the sums reproducible to n 2^-52 sum|term| per bin, not bit for bit.
//
// What this file holds, in order:
//   grids and the cell sort   CellGrid (periodic box), OpenGrid (bounding box of a light cone); cell_count<COUNT, W, Grid>,
//                             cell_fill / cell_gather / cell_starts (counting sort below 200 000 points, radix sort above)
//   unweighted, periodic      pair_count (first generation: the comparator of the tests), pair_count2, pair_count3 (default)
//   weighted and light cone   one walk in two bodies: pair_count_w (periodic, float32), pair_count_los (open grid, float64)
//   pairwise velocities       pair_vel: the walk of pair_count_w with the velocities of both sets, five float64 velocity sums per bin
//   host helpers              one set of work buffers, stage_columns, sort_into_cells, launch helpers, the run loop
//   jackknife                 pair_count_jk / pair_count_los_jk (the two walks with per-region histograms), the label-aware
//                             sort, the per-region outputs
//   counts in spheres         sphere_count: per query the data points inside each of nr radii (the walk of pair_count_w, a
//                             wave-wide ballot per radius instead of a histogram atomic per pair), then a histogram over queries
//   3PCF multipoles           threepcf_walk: per primary the spherical-harmonic sums of its neighbours per bin (the same walk, counted
//                             pairs compacted into an LDS queue), then a Gram matrix per l; its driver count_threepcf stands with it
//   the drivers               count_box (periodic) and count_los (open grid), each the plain and - with labels - the jackknife
//                             counter, and count_spheres; validation, grids, kernel arguments and statistics in one place each;
//                             the C ABI
//   friends-of-friends        fof_link (the walk of sphere_count, a lock-free union per friend pair), fof_flatten, fof_reduce,
//                             fof_emit, their driver find_groups and its C entries: at the file's end, behind every other kernel
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "../../include/abacus_hip.h"
#include "common.hpp"

using namespace abacus;

namespace abacus {
int exclusive_scan_u32(unsigned int *counters, int64_t n, int64_t *out, DevBuf &scratch, int zero_counters);
}

namespace {

constexpr int PB = 256;          // threads per workgroup
constexpr int MAX_HIST = 8192;   // LDS histogram entries (bins * sub-bins)

__device__ __forceinline__ int cell_coord(float v, int nc, float inv_box) {
    // fractional position in the box, periodic: works for [0,L), [-L/2,L/2) or anything else
    float f = v * inv_box;
    f -= floorf(f);
    int c = (int)(f * (float)nc);
    return c >= nc ? nc - 1 : c;
}

struct CellGrid {
    int ncx, ncy, ncz;
    float box, inv_box;
    __device__ __forceinline__ int cell(const float v[3]) const {
        return (cell_coord(v[0], ncx, inv_box) * ncy + cell_coord(v[1], ncy, inv_box)) * ncz + cell_coord(v[2], ncz, inv_box);
    }
};

// Open grid of a light cone: the bounding box of both sets, per-dimension cell counts 1 .. 128 with a cell side >= 1.0001
// reach; cell = min(int((v - lo) inv_cell), nc - 1) in float32; neighbour cells outside the grid are skipped, nothing wraps.
// The three float32 roundings of the cell index move a point by less than 3 2^-24 nc cells, so two points whose indices
// differ by 2 or more are further apart than (1 - 5e-5) of a cell side > reach: the 27 cells suffice.
struct OpenGrid {
    int nc[3];
    float lo[3], inv[3];
    __device__ __forceinline__ int cell(const float v[3]) const {
        int c[3];
#pragma unroll
        for (int d = 0; d < 3; d++) {
            c[d] = (int)((v[d] - lo[d]) * inv[d]);
            c[d] = c[d] >= nc[d] ? nc[d] - 1 : (c[d] < 0 ? 0 : c[d]);   // c < 0: only a NaN coordinate, kept inside the arrays
        }
        return (c[0] * nc[1] + c[1]) * nc[2] + c[2];
    }
};

// Coordinate frame of a catalogue: the smallest and the largest coordinate per dimension as order-preserving integer keys
// (so that atomicMin / atomicMax work on floats).  Corrfunc accepts any coordinate range; galaxies from the HOD live in
// [-L/2, L/2).  When every coordinate of both sets lies in ONE interval [a, a + L) the periodic image of a pair of cells
// is known per cell pair (pair_count3); `outside` only says that the frame is not [0, L).
struct Frame {
    unsigned int mn[3], mx[3];
};
__device__ __forceinline__ unsigned int fkey(float v) {
    const unsigned int u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float funkey(unsigned int k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// A thread's smallest and largest keys per dimension into *frame: wave reduction, then ONE pair of global atomics per workgroup
// and dimension (one per wave was 10^5 atomics on six addresses: 1 ms of cell_count's 1.1).  Every thread of the workgroup calls.
struct MinMax {
    unsigned int mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
    __device__ __forceinline__ void take(const float v[3]) {
#pragma unroll
        for (int d = 0; d < 3; d++) {
            const unsigned int k = fkey(v[d]);
            mn[d] = min(mn[d], k), mx[d] = max(mx[d], k);
        }
    }
};
__device__ __forceinline__ void frame_reduce(const MinMax &m, Frame *__restrict__ frame) {
    __shared__ unsigned int s_mn[3], s_mx[3];
    if (threadIdx.x < 3) s_mn[threadIdx.x] = 0xffffffffu, s_mx[threadIdx.x] = 0u;
    __syncthreads();
#pragma unroll
    for (int d = 0; d < 3; d++) {
        unsigned int a = m.mn[d], b = m.mx[d];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) a = min(a, (unsigned int)__shfl_xor((int)a, off, 64)), b = max(b, (unsigned int)__shfl_xor((int)b, off, 64));
        if ((threadIdx.x & 63) == 0 && a <= b) atomicMin(&s_mn[d], a), atomicMax(&s_mx[d], b);
    }
    __syncthreads();
    if (threadIdx.x < 3 && s_mn[threadIdx.x] <= s_mx[threadIdx.x])
        atomicMin(&frame->mn[threadIdx.x], s_mn[threadIdx.x]), atomicMax(&frame->mx[threadIdx.x], s_mx[threadIdx.x]);
}

// The cell of every point on either grid.  COUNT: per-cell counters by global atomics (counting sort, small inputs); else the
// cell ids become the keys of a radix sort and idx the values.  W (weighted counts): the point's weight rides in the free lane
// of the packed record.  The periodic grid alone keeps the frame and `outside` (some coordinate is not in [0, L)): FramedGrid.
struct FramedGrid : CellGrid {
    int *outside;
    Frame *frame;
};
template <bool COUNT, bool W, typename Grid>
__global__ void cell_count(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z,
                           const float *__restrict__ w, int64_t n, Grid g, unsigned int *__restrict__ counts, unsigned int *__restrict__ cellid,
                           unsigned int *__restrict__ idx, float4 *__restrict__ packed) {
    constexpr bool PERIODIC = std::is_same<Grid, FramedGrid>::value;
    bool out = false;
    MinMax m;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v[3] = {x[i], y[i], z[i]};
        const int c = g.cell(v);
        cellid[i] = (unsigned int)c;
        if (COUNT) atomicAdd(&counts[c], 1u);
        else idx[i] = (unsigned int)i, packed[i] = make_float4(v[0], v[1], v[2], W ? w[i] : 0.f);   // one 16-B piece per point for the gather
        if constexpr (PERIODIC) {
            out = out || !(v[0] >= 0.f && v[0] < g.box && v[1] >= 0.f && v[1] < g.box && v[2] >= 0.f && v[2] < g.box);
            m.take(v);
        }
    }
    if constexpr (PERIODIC) {
        if (out) *g.outside = 1;
        frame_reduce(m, g.frame);
    }
}

// bounding box of a set as order-preserving keys (fkey)
__global__ void bbox_minmax(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z, int64_t n,
                            Frame *__restrict__ frame) {
    MinMax m;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v[3] = {x[i], y[i], z[i]};
        m.take(v);
    }
    frame_reduce(m, frame);
}

// observer-centred float32 columns: the subtraction in the column's own dtype, then one rounding (dst may be src).  With
// origin 0 this is the plain cast of float64 columns (the HOD catalogue), as the reference casts before it calls Corrfunc
// (analysis/tpcf_corrfunc.py:134-139: `.astype(np.float32)`, round to nearest): x - 0.0 is x for every double.
template <typename T>
__global__ void los_centre(const T *src, T origin, float *dst, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = (float)(src[i] - origin);
}

// W: the weight takes the slot its point drew (the order inside a cell differs from run to run, point and weight stay together)
template <bool W>
__global__ void cell_fill(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z,
                          const float *__restrict__ w, int64_t n, const unsigned int *__restrict__ cellid,
                          const int64_t *__restrict__ start, unsigned int *__restrict__ cursor, float *__restrict__ sx,
                          float *__restrict__ sy, float *__restrict__ sz, float *__restrict__ sw) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned int c = cellid[i];
        const int64_t s = start[c] + atomicAdd(&cursor[c], 1u);
        sx[s] = x[i];
        sy[s] = y[i];
        sz[s] = z[i];
        if (W) sw[s] = w[i];
    }
}

// behind the radix sort of (cell id, point index): the points in cell order (ties in input order: the sort is stable, so
// the sorted arrays do not depend on the run) ...
template <bool W>
__global__ void cell_gather(const float4 *__restrict__ packed, int64_t n, const unsigned int *__restrict__ idx,
                            float *__restrict__ sx, float *__restrict__ sy, float *__restrict__ sz, float *__restrict__ sw) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        const float4 p = packed[idx[s]];   // one memory sector per point instead of three (x, y, z live in separate arrays)
        sx[s] = p.x, sy[s] = p.y, sz[s] = p.z;
        if (W) sw[s] = p.w;
    }
}
// ... their velocities behind them, by the same sorted index (abacus_pairvel) ...
__global__ void vel_gather(const float *__restrict__ vx, const float *__restrict__ vy, const float *__restrict__ vz, int64_t n,
                           const unsigned int *__restrict__ idx, float *__restrict__ svx, float *__restrict__ svy, float *__restrict__ svz) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        const unsigned int i = idx[s];
        svx[s] = vx[i], svy[s] = vy[i], svz[s] = vz[i];
    }
}
// ... and the first point of every cell: start[c] = number of keys below c (c = 0 .. ncell)
__global__ void cell_starts(const unsigned int *__restrict__ keys, int64_t n, int64_t ncell, int64_t *__restrict__ start) {
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c <= ncell; c += (int64_t)gridDim.x * blockDim.x) {
        int64_t lo = 0, hi = n;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)keys[mid] < c) lo = mid + 1;
            else hi = mid;
        }
        start[c] = lo;
    }
}

struct PairArgs {
    int mode, autocorr, in_box;   // in_box: every coordinate of both sets lies in [0, L)
    CellGrid g;
    int nbins, nsub;
    float half, pimax, dpi, mu_max, inv_dmu;
    const float *edges2;   // (nbins+1) squared edges
    // bin look-up of pair_count3: the float32 bit pattern of r^2, shifted by lut_sh, minus lut_off indexes lut_ncell cells, none
    // of which holds more than one inner edge (0 cells: the kernel walks the edges instead)
    int lut_sh, lut_off, lut_ncell;
    int no_blocks;         // pair_count3: every cell a job of its own (comparator of the two-cell blocks)
    const float *x1, *y1, *z1, *x2, *y2, *z2;
    const int64_t *start1, *start2;
    unsigned long long *npairs;
};

__device__ __forceinline__ float min_image(float d, float half, float box) {
    if (d > half) return d - box;
    if (d < -half) return d + box;
    return d;
}

// One workgroup per (cell of set 1, slice of its points).
__global__ __launch_bounds__(PB) void pair_count(PairArgs a, const int *__restrict__ work_cell,
                                                 const int *__restrict__ work_off) {
    __shared__ float jx[PB], jy[PB], jz[PB];
    __shared__ unsigned int hist[MAX_HIST];
    __shared__ float e2[64];
    const int tid = threadIdx.x;
    const int nh = a.nbins * a.nsub;
    for (int q = tid; q < nh; q += PB) hist[q] = 0u;
    if (tid <= a.nbins) e2[tid] = a.edges2[tid];
    __syncthreads();
    const float lo2 = e2[0], hi2 = e2[a.nbins];
    const int c1 = work_cell[blockIdx.x];
    const int64_t i0 = a.start1[c1] + work_off[blockIdx.x];
    const int64_t iend = a.start1[c1 + 1];
    const int64_t i = i0 + tid;
    const bool active = i < iend;
    float xi = 0, yi = 0, zi = 0;
    if (active) xi = a.x1[i], yi = a.y1[i], zi = a.z1[i];
    const int cz = c1 % a.g.ncz, cy = (c1 / a.g.ncz) % a.g.ncy, cx = c1 / (a.g.ncz * a.g.ncy);
    // neighbour ranges: all cells when a dimension has fewer than 3 cells (then the 27-stencil would repeat cells)
    const int rx = a.g.ncx >= 3 ? 1 : 0, ry = a.g.ncy >= 3 ? 1 : 0, rz = a.g.ncz >= 3 ? 1 : 0;
    for (int ox = -rx; ox <= rx; ox++)
        for (int oy = -ry; oy <= ry; oy++)
            for (int oz = -rz; oz <= rz; oz++) {
                int nx = cx + ox, ny = cy + oy, nz = cz + oz;
                nx = nx < 0 ? nx + a.g.ncx : (nx >= a.g.ncx ? nx - a.g.ncx : nx);
                ny = ny < 0 ? ny + a.g.ncy : (ny >= a.g.ncy ? ny - a.g.ncy : ny);
                nz = nz < 0 ? nz + a.g.ncz : (nz >= a.g.ncz ? nz - a.g.ncz : nz);
                const int c2 = (nx * a.g.ncy + ny) * a.g.ncz + nz;
                const int64_t j0 = a.start2[c2], j1 = a.start2[c2 + 1];
                for (int64_t jb = j0; jb < j1; jb += PB) {
                    const int m = (int)min((int64_t)PB, j1 - jb);
                    __syncthreads();
                    if (tid < m) {
                        jx[tid] = a.x2[jb + tid];
                        jy[tid] = a.y2[jb + tid];
                        jz[tid] = a.z2[jb + tid];
                    }
                    __syncthreads();
                    if (!active) continue;
                    for (int q = 0; q < m; q++) {
                        if (a.autocorr && jb + q == i) continue;   // same point (the two sorted sets are one array)
                        const float dx = min_image(xi - jx[q], a.half, a.g.box);
                        const float dy = min_image(yi - jy[q], a.half, a.g.box);
                        const float dz = min_image(zi - jz[q], a.half, a.g.box);
                        float r2;
                        int sub = 0;
                        if (a.mode == 1) {
                            const float adz = fabsf(dz);
                            if (adz >= a.pimax) continue;
                            r2 = dx * dx + dy * dy;
                            sub = (int)(adz / a.dpi);
                            if (sub >= a.nsub) continue;
                        } else {
                            r2 = dx * dx + dy * dy + dz * dz;
                        }
                        if (r2 < lo2 || r2 >= hi2) continue;
                        int b = 0;
                        while (r2 >= e2[b + 1]) b++;
                        if (a.mode == 2) {
                            const float s = sqrtf(r2);
                            const float mu = s > 0.f ? fabsf(dz) / s : 0.f;
                            if (mu >= a.mu_max) continue;
                            sub = (int)(mu * a.inv_dmu);
                            if (sub >= a.nsub) continue;
                        }
                        atomicAdd(&hist[b * a.nsub + sub], 1u);
                    }
                }
            }
    __syncthreads();
    for (int q = tid; q < nh; q += PB)
        if (hist[q]) atomicAdd(&a.npairs[q], (unsigned long long)hist[q]);
}

// Second-generation kernel: the (i, j) pairs of (a slice of <= 256 points of cell c1) x (a chunk of <= 256 points of a
// neighbour cell c2) are FLATTENED over the workgroup: thread t takes pairs p = t, t + 256, ... with i = p / m,
// j = p % m.  Every lane has work whatever the cell populations are (35 points per cell at 10^7 points in the
// 2 Gpc/h box left 86 % of the one-thread-per-i-point kernel's lanes idle), and both point sets are read from LDS
// (consecutive lanes: consecutive j, the same i for runs of m lanes: broadcast).  When a dimension has at least 5 cells
// the periodic image of a neighbour cell is known per cell: d = (xi - xj) + shift with shift in {0, +-L} is the very
// expression the per-pair minimum image evaluates, without its compares.  Accepted pairs (15 % of the candidates)
// search their bin from the top - most of the volume is in the outer bins - and bump the LDS histogram.
// AGG = false (dense catalogues): one staging round per neighbour cell chunk, the periodic shift and the self-pair
// test are uniform per round.  AGG = true (a few points per cell): the points of all 27 neighbour cells are appended
// to one 256-slot staging buffer with their shifts and indices, one round per slice instead of 27.
template <int MODE, bool AGG>
__global__ __launch_bounds__(PB) void pair_count2(PairArgs a, const int *__restrict__ outside, int ncell) {
    __shared__ float ix[PB], iy[PB], iz[PB];
    __shared__ float jx[PB], jy[PB], jz[PB];
    __shared__ float jsx[AGG ? PB : 1], jsy[AGG ? PB : 1], jsz[AGG ? PB : 1];   // per-point periodic shifts
    __shared__ int jg[AGG ? PB : 1];                                               // index in the sorted array
    extern __shared__ unsigned int hist[];   // nbins * nsub counters: small histograms leave room for 8 workgroups per CU
    __shared__ float e2[64];
    __shared__ int64_t nb_j0[27], nb_j1[27];   // ranges and shifts of the neighbour cells, fetched in ONE round trip
    __shared__ float nb_sh[27][3];
    const int tid = threadIdx.x;
    const int nh = a.nbins * a.nsub;
    // persistent workgroups over the cells of set 1 (no host-built work list, no host synchronisation before the
    // launch): the LDS histogram lives across cells and is flushed once - per-cell flushes of a sparse catalogue are
    // millions of global atomics on a dozen addresses.  A cell with more than 256 points is walked in slices.
    for (int q = tid; q < nh; q += PB) hist[q] = 0u;
    if (tid <= a.nbins) e2[tid] = a.edges2[tid];
    const bool in_box = *outside == 0;
    for (int c1 = blockIdx.x; c1 < ncell; c1 += gridDim.x) {
    const int64_t cbeg = a.start1[c1], cend = a.start1[c1 + 1];
    if (cbeg == cend) continue;
    __syncthreads();   // the previous cell's reads of the neighbour tables are done
    const int cz = c1 % a.g.ncz, cy = (c1 / a.g.ncz) % a.g.ncy, cx = c1 / (a.g.ncz * a.g.ncy);
    const int rx = a.g.ncx >= 3 ? 1 : 0, ry = a.g.ncy >= 3 ? 1 : 0, rz = a.g.ncz >= 3 ? 1 : 0;
    const int wx = 2 * rx + 1, wy = 2 * ry + 1, wz = 2 * rz + 1, nnb = wx * wy * wz;
    if (tid < nnb) {
        int nx = cx + tid / (wy * wz) - rx, ny = cy + (tid / wz) % wy - ry, nz = cz + tid % wz - rz;
        float shx = 0.f, shy = 0.f, shz = 0.f;   // xi - xj is about -L when c2 wrapped below 0: add L
        if (nx < 0) nx += a.g.ncx, shx = a.g.box;
        else if (nx >= a.g.ncx) nx -= a.g.ncx, shx = -a.g.box;
        if (ny < 0) ny += a.g.ncy, shy = a.g.box;
        else if (ny >= a.g.ncy) ny -= a.g.ncy, shy = -a.g.box;
        if (nz < 0) nz += a.g.ncz, shz = a.g.box;
        else if (nz >= a.g.ncz) nz -= a.g.ncz, shz = -a.g.box;
        const int c2 = (nx * a.g.ncy + ny) * a.g.ncz + nz;
        nb_j0[tid] = a.start2[c2], nb_j1[tid] = a.start2[c2 + 1];
        nb_sh[tid][0] = shx, nb_sh[tid][1] = shy, nb_sh[tid][2] = shz;
    }
    __syncthreads();
    const float lo2 = e2[0], hi2 = e2[a.nbins];
    // per-cell periodic shifts need |d| of an unwrapped neighbour pair (< 2 cells) to stay below half the box
    const bool fast = in_box && a.g.ncx >= 5 && a.g.ncy >= 5 && a.g.ncz >= 5;

    // all pairs (slice of c1) x (the `fill` staged neighbour points); !AGG: uniform shift (ux, uy, uz), the staged chunk
    // starts at sorted index jbase (self pairs only when `self_chunk`)
    auto process = [&](int64_t i0, int ni, int fill, float ux, float uy, float uz, int64_t jbase, bool self_chunk) {
        const int total = ni * fill;
        const float inv_m = 1.0f / (float)fill;
        for (int p = tid; p < total; p += PB) {
            const int i = (int)(((float)p + 0.5f) * inv_m);   // exact: p < 2^16, fill <= 2^8
            const int j = p - i * fill;
            if (AGG) {
                if (a.autocorr && (int64_t)jg[j] == i0 + i) continue;   // the same point
            } else {
                if (self_chunk && jbase + j == i0 + i) continue;
            }
            float dx = ix[i] - jx[j], dy = iy[i] - jy[j], dz = iz[i] - jz[j];
            if (fast) {
                if (AGG) dx += jsx[j], dy += jsy[j], dz += jsz[j];
                else dx += ux, dy += uy, dz += uz;
            } else {
                dx = min_image(dx, a.half, a.g.box);
                dy = min_image(dy, a.half, a.g.box);
                dz = min_image(dz, a.half, a.g.box);
            }
            float r2;
            int sub = 0;
            if (MODE == 1) {
                const float adz = fabsf(dz);
                if (adz >= a.pimax) continue;
                r2 = dx * dx + dy * dy;
                if (r2 < lo2 || r2 >= hi2) continue;
                sub = (int)(adz / a.dpi);
                if (sub >= a.nsub) continue;
            } else {
                r2 = dx * dx + dy * dy + dz * dz;
                if (r2 < lo2 || r2 >= hi2) continue;
            }
            int b = a.nbins - 1;
            while (r2 < e2[b]) b--;
            if (MODE == 2) {
                const float sr = sqrtf(r2);
                const float mu = sr > 0.f ? fabsf(dz) / sr : 0.f;
                if (mu >= a.mu_max) continue;
                sub = (int)(mu * a.inv_dmu);
                if (sub >= a.nsub) continue;
            }
            atomicAdd(&hist[b * a.nsub + sub], 1u);
        }
    };

    for (int64_t i0 = cbeg; i0 < cend; i0 += PB) {
        const int ni = (int)min((int64_t)PB, cend - i0);
        __syncthreads();   // the previous slice's reads of ix/iy/iz (and of the staging buffer) are done
        if (tid < ni) ix[tid] = a.x1[i0 + tid], iy[tid] = a.y1[i0 + tid], iz[tid] = a.z1[i0 + tid];
        int fill = 0;
        for (int nb = 0; nb < nnb; nb++) {
            int64_t jb = nb_j0[nb];
            const int64_t j1 = nb_j1[nb];
            const float shx = nb_sh[nb][0], shy = nb_sh[nb][1], shz = nb_sh[nb][2];
            while (jb < j1) {
                const int take = (int)min((int64_t)(PB - fill), j1 - jb);
                if (!AGG) __syncthreads();   // the previous round's reads of the staging buffer are done
                if (tid < take) {
                    const int q = fill + tid;
                    jx[q] = a.x2[jb + tid], jy[q] = a.y2[jb + tid], jz[q] = a.z2[jb + tid];
                    if (AGG) {
                        jsx[q] = shx, jsy[q] = shy, jsz[q] = shz;
                        jg[q] = (int)(jb + tid);
                    }
                }
                if (AGG) {
                    fill += take;
                    if (fill == PB) {
                        __syncthreads();
                        process(i0, ni, fill, 0.f, 0.f, 0.f, 0, false);
                        __syncthreads();
                        fill = 0;
                    }
                } else {
                    __syncthreads();
                    process(i0, ni, take, shx, shy, shz, jb, a.autocorr && jb < i0 + ni && jb + take > i0);
                }
                jb += take;
            }
        }
        if (AGG && fill) {
            __syncthreads();
            process(i0, ni, fill, 0.f, 0.f, 0.f, 0, false);
        }
    }
    }   // cells
    __syncthreads();
    for (int q = tid; q < nh; q += PB)
        if (hist[q]) atomicAdd(&a.npairs[q], (unsigned long long)hist[q]);
}

// Third-generation kernel: ONE WAVE per cell of set 1, cells of size reach / R (R = 1 or 2), and for an autocorrelation the
// HALF stencil - every unordered pair is evaluated once and the histogram is doubled at the end (exact: dx -> -dx,
// the minimum image and the per-cell shifts negate exactly, so r^2, |dz| and mu of (i, j) and (j, i) are bit-equal).
// Against the workgroup-per-cell kernel with cells of the full reach: R = 2 evaluates 5^3 / 8 instead of 27 cell volumes
// per point (x 1/1.7), the half stencil halves that again, and a wave needs no workgroup barrier - the staging buffers, the
// segment table and the i-slice are wave-private LDS, the waves of a workgroup only share the histogram.
//   * Neighbour cells along z are consecutive in the sorted arrays: the stencil is walked as (2R+1)^2 ROWS, each one
//     contiguous range of points (two when the row wraps around the box in z).
//   * Half stencil: rows (ox, oy) lexicographically after (0, 0) with all 2R+1 cells; of row (0, 0) the cells behind the
//     own one, and the own cell with the test j > i (sorted indices).
//   * Periodic images per segment: coordinates of both sets lie in one interval [a, a + L) (Frame), so a point's
//     coordinate is L frac + const, raised by L when its fraction lies below frac(a); the true separation of a pair from
//     cells (c1, c1 + o) is (xi - xj) - L (w + s(c1) - s(c2)) with w the index wrap and s(c) = [c below the cut cell] - the
//     same single float addition of 0 or -+L the per-pair minimum image performs.  Segments touching the cut cell or its
//     two neighbours (mixed cells, float rounding at the cut) take the per-pair minimum image instead.
constexpr int P3_WAVES = 4, P3_JCAP = 320, P3_ICAP = 64, P3_SLOTS = 64;

//   * Bin of a pair (LUT): r^2 is a positive float, so its bit pattern is monotone in it; the pattern's top bits index a
//     table of cells (2^m per octave, m chosen by the host so that no cell holds two edges) whose entry is the bin of the
//     cell's lower end and the next edge: bin = entry.bin + (r^2 >= entry.edge) - the walk's answer (largest b with
//     edges2[b] <= r^2) from ONE LDS read instead of a data-dependent loop of them.  The inner loop is straight-line,
//     predicated code (counting the pairs of the last bin - three quarters of those in range for logarithmic bins - by a
//     wave-wide ballot + population count instead of LDS atomics measured slower: 6.6 against 5.8 ms).
template <int MODE, bool LUT>
__global__ __launch_bounds__(P3_WAVES * 64) void pair_count3(PairArgs a, const Frame *__restrict__ frame, int ncell, int R,
                                                              unsigned long long *__restrict__ evaluated) {
    __shared__ int64_t seg_j0[P3_WAVES][P3_SLOTS];
    __shared__ int seg_pre[P3_WAVES][P3_SLOTS + 1], seg_code[P3_WAVES][P3_SLOTS];   // exclusive prefix of the segment lengths
    __shared__ float e2[64];
    __shared__ int s_cut[3], s_general[3], s_ok;
    extern __shared__ __align__(8) unsigned int hist[];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);   // w: a scalar, like everything per cell
    const int nh = a.nbins * a.nsub;
    uint2 *lut = reinterpret_cast<uint2 *>(hist + ((nh + 1) & ~1));
    for (int q = tid; q < nh; q += P3_WAVES * 64) hist[q] = 0u;
    if (tid <= a.nbins) e2[tid] = a.edges2[tid];
    if (tid == 0) s_ok = 1;
    __syncthreads();
    if (LUT)
        for (int c = tid; c < a.lut_ncell; c += P3_WAVES * 64) {
            const float low = __uint_as_float((unsigned int)(c + a.lut_off) << a.lut_sh);
            int cnt = 0;
            for (int b = 0; b < a.nbins; b++) cnt += e2[b] <= low ? 1 : 0;
            const int b0 = max(cnt - 1, 0);
            lut[c] = make_uint2((unsigned int)b0, __float_as_uint(b0 + 1 < a.nbins ? e2[b0 + 1] : __builtin_huge_valf()));
        }
    if (tid < 3) {
        const float lo = funkey(frame->mn[tid]), hi = funkey(frame->mx[tid]);
        const int nc = tid == 0 ? a.g.ncx : (tid == 1 ? a.g.ncy : a.g.ncz);
        // one period holds everything?  (margin: the cut cells absorb rounding at the ends)
        if (!((double)hi - (double)lo < (double)a.g.box)) s_ok = 0;
        const bool std_frame = lo >= 0.f && hi < a.g.box;       // [0, L): no raised coordinates, the cut is the index wrap
        s_general[tid] = std_frame ? 0 : 1;
        s_cut[tid] = std_frame ? 0 : cell_coord(lo, nc, a.g.inv_box);
    }
    __syncthreads();
    const float lo2 = e2[0], hi2 = e2[a.nbins];
    const bool frame_ok = s_ok != 0;
    const int ncx = a.g.ncx, ncy = a.g.ncy, ncz = a.g.ncz, W = 2 * R + 1;
    const int nrow = a.autocorr ? (W * W - 1) / 2 + 1 : W * W;     // half stencil: rows after (0, 0), then row (0, 0)
    const int nslot = 2 * nrow + (a.autocorr ? 1 : 0);
    // s(c) - [c below the cut] - and the mixed set {cut-1, cut, cut+1} of a dimension
    auto below = [&](int d, int c) { return s_general[d] && c < s_cut[d] ? 1 : 0; };
    auto mixed1 = [&](int d, int c, int nc) {
        if (!s_general[d]) return false;
        int t = c - s_cut[d];
        if (t < 0) t += nc;
        return t == 0 || t == 1 || t == nc - 1;
    };
    unsigned long long n_eval = 0;   // candidate pairs this wave evaluated (uniform per wave; lane 0 reports)
    const int lsh = a.lut_sh, loff = a.lut_off;
    // the global loads of a cell's table (its own range, the ranges of its segments): issued ONE CELL AHEAD, so that
    // their round trip runs under the pair loop of the cell before
    struct Table {
        int64_t cbeg, cend, j0;
        int len, code;
    };
    // Lane constants of the table: the stencil row / part of slot `lane`.  For a cell at least R cells away from every face of
    // the grid in a standard frame no row wraps and nothing is "mixed": the slot's cell range is the own cell index plus a
    // constant and its code is a constant - two adds and two loads instead of the ~80 instructions of the general case
    // (which the cells of the outer shell and every cell of a shifted frame still take).  PMC had the kernel at 93 % VALU
    // utilisation with two thirds of its vector instructions outside the pair loop.
    int s_ox = 0, s_oy = 0, s_zlo = -R, s_zhi = R, s_filt = 0;
    if (a.autocorr && lane == 2 * nrow) {
        s_zlo = s_zhi = 0, s_filt = 1;
    } else {
        const int row = lane >> 1;
        if (a.autocorr) {
            if (row == nrow - 1) s_zlo = 1;
            else {
                const int t2 = row + (R * W + R) + 1;
                s_ox = t2 / W - R, s_oy = t2 % W - R;
            }
        } else {
            s_ox = row / W - R, s_oy = row % W - R;
        }
    }
    const bool s_valid_in = lane < nslot && !(lane & 1) && s_zlo <= s_zhi;      // interior cells: part 0 only
    const int s_da = (s_ox * ncy + s_oy) * ncz + s_zlo, s_db = (s_ox * ncy + s_oy) * ncz + s_zhi + 1;
    const int s_code_in = 2 | (2 << 3) | (2 << 6) | (s_filt ? 1024 : 0);
    const bool std_frame_all = frame_ok && !s_general[0] && !s_general[1] && !s_general[2];
    // BLOCKS: two z-adjacent interior cells (cz even) are one job.  Their points are consecutive in the sorted arrays, their
    // stencils differ by one cell in z: one table, one staging of the union (rows one cell taller; row (0, 0): the cells behind
    // the block; the own range = both cells with the test j > i, which also counts every (A, B) pair once) for 8.5 slice
    // points instead of 4.3 - the per-cell overheads halve; what a slice point sees of the extra cell is out of reach and falls
    // to the range test (+ 20 % candidates).
    const bool s_own = a.autocorr && lane == 2 * nrow, s_row00 = a.autocorr && !s_own && (lane >> 1) == nrow - 1;
    const int s_zlo2 = s_own ? 0 : (s_row00 ? 2 : -R), s_zhi2 = s_own ? 1 : R + 1;
    const int s_da2 = (s_ox * ncy + s_oy) * ncz + s_zlo2, s_db2 = (s_ox * ncy + s_oy) * ncz + s_zhi2 + 1;
    const bool s_valid_in2 = lane < nslot && !(lane & 1) && s_zlo2 <= s_zhi2;
    auto fetch = [&](int c1, int cx, int cy, int cz, int nb) {
        Table t;
        t.cbeg = a.start1[c1], t.cend = a.start1[c1 + nb], t.j0 = 0, t.len = 0, t.code = 0;
        if (nb == 2) {        // a block: interior by construction
            if (s_valid_in2) {
                t.j0 = a.start2[c1 + s_da2];
                t.len = (int)(a.start2[c1 + s_db2] - t.j0);
                t.code = s_code_in;
            }
            return t;
        }
        const bool inner = std_frame_all && cx >= R && cx < ncx - R && cy >= R && cy < ncy - R && cz >= R && cz < ncz - R;
        if (inner) {
            if (s_valid_in) {
                t.j0 = a.start2[c1 + s_da];
                t.len = (int)(a.start2[c1 + s_db] - t.j0);
                t.code = s_code_in;
            }
            return t;
        }
        if (lane < nslot) {
            int ox = 0, oy = 0, zlo = -R, zhi = R, filt = 0;
            bool valid = true;
            const int part = lane & 1;
            if (a.autocorr && lane == 2 * nrow) {          // the own cell: pairs j > i
                zlo = zhi = 0, filt = 1;
            } else {
                const int row = lane >> 1;
                if (a.autocorr) {
                    if (row == nrow - 1) zlo = 1;          // row (0, 0): the cells behind the own one
                    else {
                        const int t2 = row + (R * W + R) + 1;
                        ox = t2 / W - R, oy = t2 % W - R;
                    }
                } else {
                    ox = row / W - R, oy = row % W - R;
                }
            }
            int nx = cx + ox, ny = cy + oy, wx = 0, wy = 0;
            if (nx < 0) nx += ncx, wx = -1;
            else if (nx >= ncx) nx -= ncx, wx = 1;
            if (ny < 0) ny += ncy, wy = -1;
            else if (ny >= ncy) ny -= ncy, wy = 1;
            // z cells [cz + zlo, cz + zhi]: part 0 = the piece inside [0, ncz), part 1 = the piece that wraps
            int za = cz + zlo, zb = cz + zhi, wz = 0;
            if (filt) {
                if (part) valid = false;     // (lane 2 nrow is even: never taken, kept for clarity)
            } else if (zlo > zhi) {
                valid = false;
            } else if (!part) {
                za = max(za, 0), zb = min(zb, ncz - 1);
            } else if (za < 0) {
                zb = min(zb, -1) + ncz, za = za + ncz, wz = -1;
            } else if (zb >= ncz) {
                za = max(za, ncz) - ncz, zb = zb - ncz, wz = 1;
            } else {
                valid = false;
            }
            if (valid && za <= zb) {
                const int cA = (nx * ncy + ny) * ncz + za, cB = (nx * ncy + ny) * ncz + zb;
                t.j0 = a.start2[cA];
                t.len = (int)(a.start2[cB + 1] - t.j0);
                const int kx = wx + below(0, cx) - below(0, nx), ky = wy + below(1, cy) - below(1, ny),
                          kz = wz + below(2, cz) - below(2, za);
                bool mixed = !frame_ok || mixed1(0, cx, ncx) || mixed1(0, nx, ncx) || mixed1(1, cy, ncy) || mixed1(1, ny, ncy) ||
                             mixed1(2, cz, ncz);
                for (int zc = za; zc <= zb; zc++) mixed = mixed || mixed1(2, zc, ncz);
                t.code = (kx + 2) | ((ky + 2) << 3) | ((kz + 2) << 6) | (mixed ? 512 : 0) | (filt ? 1024 : 0);
            }
        }
        return t;
    };
    // Jobs of this wave: units (cx, cy, pair of z cells) in steps of the grid's wave count; a unit is ONE job when it is a block
    // (both cells interior, standard frame), else its one or two cells are jobs of their own.  Unit coordinates advance by
    // the decomposed stride (scalar adds and carries, no integer division per job).
    const int nbz = (ncz + 1) >> 1, nunit = ncx * ncy * nbz;
    const int ustride = gridDim.x * P3_WAVES;
    int un = blockIdx.x * P3_WAVES + w;
    const int dub = ustride % nbz, duy = (ustride / nbz) % ncy, dux = ustride / (nbz * ncy);
    int ub = un % nbz, uy = (un / nbz) % ncy, ux = un / (nbz * ncy);
    const bool blocks_on = std_frame_all && !a.no_blocks;
    struct Job {
        int c1, cx, cy, cz, nb;
    };
    Job second;                 // the second cell of a unit that is no block, handed out next
    bool have_second = false;
    auto next_job = [&](Job &j) -> bool {
        if (have_second) {
            have_second = false;
            j = second;
            return true;
        }
        if (un >= nunit) return false;
        const int cz = 2 * ub, nb = min(2, ncz - cz), c1 = (ux * ncy + uy) * ncz + cz;
        const bool blk = nb == 2 && blocks_on && ux >= R && ux < ncx - R && uy >= R && uy < ncy - R && cz >= R && cz + 1 < ncz - R;
        j = Job{c1, ux, uy, cz, blk ? 2 : 1};
        if (nb == 2 && !blk) second = Job{c1 + 1, ux, uy, cz + 1, 1}, have_second = true;
        un += ustride;
        ub += dub;
        int carry = ub >= nbz ? 1 : 0;
        ub -= carry * nbz;
        uy += duy + carry;
        carry = uy >= ncy ? 1 : 0;
        uy -= carry * ncy;
        ux += dux + carry;
        return true;
    };
    Job job;
    bool more = next_job(job);
    Table nxt;
    if (more) nxt = fetch(job.c1, job.cx, job.cy, job.cz, job.nb);
    while (more) {
        const Table cur = nxt;
        more = next_job(job);
        if (more) nxt = fetch(job.c1, job.cx, job.cy, job.cz, job.nb);
        const int64_t cbeg = cur.cbeg, cend = cur.cend;
        if (cbeg == cend) continue;
        wave_sync();   // the previous cell's reads of the segment table are done
        const int64_t j0 = cur.j0;
        const int len = cur.len, code = cur.code;
        // exclusive prefix of the segment lengths over the wave: the neighbour points of the cell form ONE virtual list, which
        // is staged P3_JCAP (320) at a time by all lanes at once (a segment at a time was one memory round trip per segment: 27 to 51
        // dependent round trips per cell, 40 us - the kernel was latency-bound at 18 % of its instruction rate)
        int incl = len;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_up(incl, d, 64);
            if (lane >= d) incl += v;
        }
        const int M = __shfl(incl, 63, 64);
        // the table holds the non-empty segments only, in order (half of the slots - the pieces that wrap in z - are empty for
        // all but the outer cells): 14 of them for the half stencil, so the slot search of a staged point takes 4 steps, not 5
        const bool nz = len > 0;
        const unsigned long long nzmask = __ballot(nz);
        const int nseg = __popcll(nzmask);
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(nzmask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)nzmask, 0u));
        const int slot = nz ? rank : nseg + (lane - rank);     // empty ones behind, as sentinels holding the total
        seg_pre[w][slot] = nz ? incl - len : M;
        if (nz) seg_j0[w][slot] = j0, seg_code[w][slot] = code;
        if (lane == 63) seg_pre[w][64] = M;
        const int shi = nseg <= 16 ? 15 : (nseg <= 32 ? 31 : 63);
        wave_sync();
        for (int64_t i0 = cbeg; i0 < cend; i0 += P3_ICAP) {
            const int ni = (int)min((int64_t)P3_ICAP, cend - i0);
            // lane l holds point l of the cell's slice; the pair loop broadcasts point i to the wave with v_readlane (a scalar
            // register: no LDS read, nothing to wait for - PMC had the waves of the LDS-staged form parked in s_waitcnt for
            // 54 % of their cycles at 4 waves per SIMD).  A lane OWNS neighbour points - in the registers it fetched them
            // into - and walks the few points of the slice: no index arithmetic per pair.
            float vix = 0.f, viy = 0.f, viz = 0.f;
            if (lane < ni) vix = a.x1[i0 + lane], viy = a.y1[i0 + lane], viz = a.z1[i0 + lane];
            const int i0i = (int)i0;
            const int niu = __builtin_amdgcn_readfirstlane(ni);
            for (int base = 0; base < M; base += P3_JCAP) {
                const int cnt = min(P3_JCAP, M - base);
                // every lane fetches its points of this round first (all loads in flight together)
                float tx[P3_JCAP / 64], ty[P3_JCAP / 64], tz[P3_JCAP / 64];
                int tg[P3_JCAP / 64], tc[P3_JCAP / 64];
#pragma unroll
                for (int u = 0; u < P3_JCAP / 64; u++) {
                    const int q = u * 64 + lane;
                    tg[u] = -1;
                    tc[u] = 0;
                    tx[u] = ty[u] = tz[u] = 0.f;
                    if (q < cnt) {
                        const int v = base + q;
                        int lo = 0, hi = shi;            // largest slot with seg_pre <= v
                        while (lo < hi) {
                            const int mid = (lo + hi + 1) >> 1;
                            if (seg_pre[w][mid] <= v) lo = mid;
                            else hi = mid - 1;
                        }
                        const int64_t jj = seg_j0[w][lo] + (v - seg_pre[w][lo]);
                        tx[u] = a.x2[jj], ty[u] = a.y2[jj], tz[u] = a.z2[jj];
                        tg[u] = (int)jj, tc[u] = seg_code[w][lo];
                    }
                }
                n_eval += (unsigned long long)ni * (unsigned long long)cnt;
#pragma unroll
                for (int u = 0; u < P3_JCAP / 64; u++) {
                    if (u * 64 >= cnt) break;   // uniform
                    const bool have = tg[u] >= 0;
                    const float xj = tx[u], yj = ty[u], zj = tz[u];
                    const int flags = tc[u];
                    const float sx = (float)(2 - (flags & 7)) * a.g.box;          // -k L, k in {-2 .. 2}
                    const float sy = (float)(2 - ((flags >> 3) & 7)) * a.g.box;
                    const float sz = (float)(2 - ((flags >> 6) & 7)) * a.g.box;
                    // own cell: pairs with i < j - i0 only (every unordered pair once, i ascending); no point: no pairs
                    const int ilim = !have ? 0 : ((flags & 1024) ? min(tg[u] - i0i, ni) : ni);
                    const bool mixed = (flags & 512) != 0;
                    if constexpr (LUT) {
                        // waves none of whose neighbour points needs the per-pair minimum image (all but those near the
                        // frame's cut) run the loop without that code
                        // ... and waves all of whose points come from segments without a periodic shift (every cell away from
                        // the faces of the grid) run it without the shift additions
                        auto run = [&](auto any_mixed, auto no_shift) {
                            constexpr bool MIX = decltype(any_mixed)::value, PLAIN = decltype(no_shift)::value;
                            auto eval = [&](const int i, float &r2o, int &subo, bool &oko) {
                                const int ii = i & 63;
                                const float xi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(vix), ii));
                                const float yi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(viy), ii));
                                const float zi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(viz), ii));
                                float dx = xi - xj, dy = yi - yj, dz = zi - zj;
                                if (MIX) {   // branch-free: the minimum image's single addition of 0 or -+L, per lane
                                    const float mx = dx > a.half ? -a.g.box : (dx < -a.half ? a.g.box : 0.f);
                                    const float my = dy > a.half ? -a.g.box : (dy < -a.half ? a.g.box : 0.f);
                                    const float mz = dz > a.half ? -a.g.box : (dz < -a.half ? a.g.box : 0.f);
                                    dx += mixed ? mx : sx, dy += mixed ? my : sy, dz += mixed ? mz : sz;
                                } else if (!PLAIN) {
                                    dx += sx, dy += sy, dz += sz;
                                }
                                const float adz = fabsf(dz);
                                const float r2 = MODE == 1 ? dx * dx + dy * dy : dx * dx + dy * dy + dz * dz;
                                bool ok = i < ilim && r2 >= lo2 && r2 < hi2;
                                int sub = 0;
                                if (MODE == 1) {
                                    sub = (int)(adz / a.dpi);
                                    ok = ok && adz < a.pimax && sub < a.nsub;
                                }
                                if (MODE == 2) {
                                    const float sr = sqrtf(r2);
                                    const float mu = sr > 0.f ? adz / sr : 0.f;
                                    sub = (int)(mu * a.inv_dmu);
                                    ok = ok && mu < a.mu_max && sub < a.nsub;
                                }
                                r2o = r2, subo = sub, oko = ok;
                            };
                            auto look = [&](const float r2, const bool ok) { return lut[ok ? (int)(__float_as_uint(r2) >> lsh) - loff : 0]; };
                            auto count = [&](const float r2, const int sub, const bool ok, const uint2 cell) {
                                const int b = (int)cell.x + (r2 >= __uint_as_float(cell.y) ? 1 : 0);
                                if (ok) atomicAdd(&hist[MODE == 0 ? b : b * a.nsub + sub], 1u);
                            };
                            // one point of the slice per trip (two or four per trip - their table reads in flight together - pad
                            // the slice of 4.4 points on average: 5.8 / 6.6 ms against 5.5; a software-pipelined read: 5.5)
                            for (int i = 0; i < niu; i++) {
                                float r2;
                                int sub;
                                bool ok;
                                eval(i, r2, sub, ok);
                                count(r2, sub, ok, look(r2, ok));
                            }
                        };
                        if (__any(mixed)) run(std::true_type(), std::false_type());
                        else if (__any(have && (flags & 0x1FF) != (2 | (2 << 3) | (2 << 6)))) run(std::false_type(), std::false_type());
                        else run(std::false_type(), std::true_type());
                        continue;
                    }
                    for (int i = 0; i < ni; i++) {   // uniform trip count: readlane needs a wave-uniform index
                        const float xi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(vix), i));
                        const float yi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(viy), i));
                        const float zi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(viz), i));
                        if (i >= ilim) continue;
                        float dx = xi - xj, dy = yi - yj, dz = zi - zj;
                        if (mixed) {
                            dx = min_image(dx, a.half, a.g.box);
                            dy = min_image(dy, a.half, a.g.box);
                            dz = min_image(dz, a.half, a.g.box);
                        } else {   // 0 or -+L (or -+2L): the minimum image's own single addition
                            dx += sx, dy += sy, dz += sz;
                        }
                        float r2;
                        int sub = 0;
                        if (MODE == 1) {
                            const float adz = fabsf(dz);
                            if (adz >= a.pimax) continue;
                            r2 = dx * dx + dy * dy;
                            if (r2 < lo2 || r2 >= hi2) continue;
                            sub = (int)(adz / a.dpi);
                            if (sub >= a.nsub) continue;
                        } else {
                            r2 = dx * dx + dy * dy + dz * dz;
                            if (r2 < lo2 || r2 >= hi2) continue;
                        }
                        int b = a.nbins - 1;
                        while (r2 < e2[b]) b--;
                        if (MODE == 2) {
                            const float sr = sqrtf(r2);
                            const float mu = sr > 0.f ? fabsf(dz) / sr : 0.f;
                            if (mu >= a.mu_max) continue;
                            sub = (int)(mu * a.inv_dmu);
                            if (sub >= a.nsub) continue;
                        }
                        atomicAdd(&hist[b * a.nsub + sub], 1u);
                    }
                }
            }
        }
    }
    if (lane == 0 && n_eval) atomicAdd(evaluated, n_eval);
    __syncthreads();
    const unsigned long long mult = a.autocorr ? 2ull : 1ull;   // the half stencil evaluated every unordered pair once
    for (int q = tid; q < nh; q += P3_WAVES * 64)
        if (hist[q]) atomicAdd(&a.npairs[q], mult * (unsigned long long)hist[q]);
}

// Weighted counter: per (bin, sub-bin) the integer count, sum of w_i w_j and sum of the pair separation (r | rp | s).
// One kernel for every geometry: cells of the full reach (or one cell per dimension when fewer than 3 fit), a persistent
// workgroup per cell of set 1, the 27 (or fewer) neighbour cells as ONE virtual list of which every thread fetches one point
// per round into registers and walks the slice of its own cell (LDS broadcast reads), and the per-pair minimum image of the
// oracle in every case - the expressions that decide membership are those of the unweighted kernels, so npairs is bit-equal.
//   * w_i w_j is formed in float64 (24 + 24 significant bits: exact) and accumulated in float64 from there on - registers,
//     LDS (ds_add_f64) and global memory; the separation is sqrtf (correctly rounded) of the r^2 that chose the bin, summed in float64.
//     The sums depend on the order of the atomics in their last bits: |error| <= n 2^-52 sum|term| whatever the order.
//   * MODE 0: the last bin takes most pairs of logarithmic bins; every lane keeps that bin's three sums in registers and adds
//     them to the histogram once, at the end (64 lanes on one LDS address serialise; a ballot cannot carry a float64 sum).
//   * An entry is 20 bytes: W_MAX_HIST entries per launch, more are counted in runs of separation bins (for_runs).
//   * The autocorrelation walks the full stencil (ordered pairs, nothing is doubled).
// pair_count_los below is this walk on the open grid: a fix to one belongs in both (profiles/pairs_shared_walk/README.md).
constexpr int W_MAX_HIST = 2048;

struct WeightArgs {
    const float *w1, *w2;   // weights in cell order; NULL: unit weights
    double *wsum, *rsum;    // rsum is read only when RSUM
};

template <int MODE, bool RSUM>
__global__ __launch_bounds__(PB) void pair_count_w(PairArgs a, WeightArgs wa, int ncell, unsigned long long *__restrict__ evaluated) {
    __shared__ float ix[PB], iy[PB], iz[PB], iw[PB];
    __shared__ float e2[64];
    __shared__ int64_t nb_j0[27];
    __shared__ int nb_pre[28];               // exclusive prefix of the neighbour cells' populations
    extern __shared__ __align__(8) double hw[];   // nh sums of w w | nh sums of the separation | nh counts
    const int tid = threadIdx.x;
    const int nh = a.nbins * a.nsub;
    double *hr = hw + nh;
    unsigned int *hc = reinterpret_cast<unsigned int *>(hr + nh);
    for (int q = tid; q < nh; q += PB) hw[q] = 0.0, hr[q] = 0.0, hc[q] = 0u;
    if (tid <= a.nbins) e2[tid] = a.edges2[tid];
    __syncthreads();
    const float lo2 = e2[0], hi2 = e2[a.nbins], top2 = e2[a.nbins - 1];
    const int rx = a.g.ncx >= 3 ? 1 : 0, ry = a.g.ncy >= 3 ? 1 : 0, rz = a.g.ncz >= 3 ? 1 : 0;
    const int wy = 2 * ry + 1, wz = 2 * rz + 1, nnb = (2 * rx + 1) * wy * wz;
    double top_w = 0.0, top_r = 0.0;         // MODE 0: the last bin, per lane
    unsigned long long top_n = 0, n_eval = 0;
    for (int c1 = blockIdx.x; c1 < ncell; c1 += gridDim.x) {
        const int64_t cbeg = a.start1[c1], cend = a.start1[c1 + 1];
        if (cbeg == cend) continue;
        __syncthreads();   // the previous cell's reads of the neighbour table and of the slice are done
        if (tid < 64) {
            int len = 0;
            int64_t j0 = 0;
            if (tid < nnb) {
                const int cz = c1 % a.g.ncz, cy = (c1 / a.g.ncz) % a.g.ncy, cx = c1 / (a.g.ncz * a.g.ncy);
                int nx = cx + tid / (wy * wz) - rx, ny = cy + (tid / wz) % wy - ry, nz = cz + tid % wz - rz;
                nx = nx < 0 ? nx + a.g.ncx : (nx >= a.g.ncx ? nx - a.g.ncx : nx);
                ny = ny < 0 ? ny + a.g.ncy : (ny >= a.g.ncy ? ny - a.g.ncy : ny);
                nz = nz < 0 ? nz + a.g.ncz : (nz >= a.g.ncz ? nz - a.g.ncz : nz);
                const int c2 = (nx * a.g.ncy + ny) * a.g.ncz + nz;
                j0 = a.start2[c2];
                len = (int)(a.start2[c2 + 1] - j0);
            }
            int incl = len;
#pragma unroll
            for (int d = 1; d < 32; d <<= 1) {
                const int v = __shfl_up(incl, d, 64);
                if (tid >= d) incl += v;
            }
            if (tid < nnb) nb_j0[tid] = j0, nb_pre[tid] = incl - len;
            if (tid == nnb - 1) nb_pre[nnb] = incl;
        }
        __syncthreads();
        const int M = nb_pre[nnb];
        for (int64_t i0 = cbeg; i0 < cend; i0 += PB) {
            const int ni = (int)min((int64_t)PB, cend - i0);
            if (i0 > cbeg) __syncthreads();   // the previous slice's reads are done
            if (tid < ni) {
                ix[tid] = a.x1[i0 + tid], iy[tid] = a.y1[i0 + tid], iz[tid] = a.z1[i0 + tid];
                iw[tid] = wa.w1 ? wa.w1[i0 + tid] : 1.0f;
            }
            __syncthreads();
            for (int base = 0; base < M; base += PB) {
                n_eval += (unsigned long long)ni * (unsigned long long)min(PB, M - base);
                const int v = base + tid;
                if (v >= M) continue;
                int sg = 0;
                while (nb_pre[sg + 1] <= v) sg++;        // v < nb_pre[nnb]: ends at a non-empty cell
                const int64_t jj = nb_j0[sg] + (v - nb_pre[sg]);
                const float xj = a.x2[jj], yj = a.y2[jj], zj = a.z2[jj];
                const double wj = wa.w2 ? (double)wa.w2[jj] : 1.0;
                for (int i = 0; i < ni; i++) {
                    if (a.autocorr && jj == i0 + i) continue;   // the same point (the two sorted sets are one array)
                    const float dx = min_image(ix[i] - xj, a.half, a.g.box);
                    const float dy = min_image(iy[i] - yj, a.half, a.g.box);
                    const float dz = min_image(iz[i] - zj, a.half, a.g.box);
                    float r2;
                    int sub = 0;
                    if (MODE == 1) {
                        const float adz = fabsf(dz);
                        if (adz >= a.pimax) continue;
                        r2 = dx * dx + dy * dy;
                        if (r2 < lo2 || r2 >= hi2) continue;
                        sub = (int)(adz / a.dpi);
                        if (sub >= a.nsub) continue;
                    } else {
                        r2 = dx * dx + dy * dy + dz * dz;
                        if (r2 < lo2 || r2 >= hi2) continue;
                    }
                    float sep = 0.f;
                    if (MODE == 2) {
                        sep = sqrtf(r2);
                        const float mu = sep > 0.f ? fabsf(dz) / sep : 0.f;
                        if (mu >= a.mu_max) continue;
                        sub = (int)(mu * a.inv_dmu);
                        if (sub >= a.nsub) continue;
                    } else if (RSUM) {
                        sep = sqrtf(r2);
                    }
                    const double ww = (double)iw[i] * wj;
                    if (MODE == 0 && r2 >= top2) {
                        top_n++, top_w += ww;
                        if (RSUM) top_r += (double)sep;
                        continue;
                    }
                    int b = a.nbins - 1;
                    while (r2 < e2[b]) b--;
                    const int q = b * a.nsub + sub;
                    atomicAdd(&hc[q], 1u);
                    atomicAdd(&hw[q], ww);
                    if (RSUM) atomicAdd(&hr[q], (double)sep);
                }
            }
        }
    }
    if (tid == 0 && n_eval) atomicAdd(evaluated, n_eval);
    if (MODE == 0 && top_n) {
        // a lane's share of a workgroup's last-bin pairs stays far below 2^32
        const int q = a.nbins - 1;
        atomicAdd(&hc[q], (unsigned int)top_n);
        atomicAdd(&hw[q], top_w);
        if (RSUM) atomicAdd(&hr[q], top_r);
    }
    __syncthreads();
    for (int q = tid; q < nh; q += PB)
        if (hc[q]) {
            atomicAdd(&a.npairs[q], (unsigned long long)hc[q]);
            atomicAdd(&wa.wsum[q], hw[q]);
            if (RSUM) atomicAdd(&wa.rsum[q], hr[q]);
        }
}

// Pairwise velocity sums (abacus_pairvel; halotools' mean_radial_velocity_vs_r / radial_pvd_vs_r / mean_los_velocity_vs_rp /
// los_pvd_vs_rp are moments of them).  The walk, the membership tests and the bin of pair_count_w, untouched - npairs and wsum are
// that counter's - with the velocities of both sets riding along; a fix to one walk belongs in all of them
// (profiles/pairs_shared_walk/README.md).  Per counted pair: u = v_i - v_j in float32, then float64, left to right, no FMA
// (this file is built with contraction off):
//   s2 = dx dx + dy dy + dz dz, t = ux dx + uy dy + uz dz, vr = s2 > 0 ? t / sqrt(s2) : 0 (negative: approaching),
//   uu = ux ux + uy uy + uz uz, vz = uz sign(dz) (the minimum-image float32 dz; sign(0) = 0)
// and with ww = (double)w_i (double)w_j five sums beside npairs and wsum: ww vr, ww vr^2, ww uu, ww vz, ww uz^2.
//   * The float64 arithmetic stands behind the membership test: a candidate costs what it costs in pair_count_w.
//   * LDS: 7760 bytes static (the slice of set 1 with its weights and velocities, the edge and neighbour tables) and 52 bytes
//     per histogram entry (a count and six doubles).  V_MAX_HIST = 1024 entries are 53 248 bytes: 61 008 per workgroup, two
//     workgroups (122 016 bytes) in the CU's 163 840; a third would need <= 901 entries.  A launch allocates what its binning
//     needs, so the usual r binning of a few dozen entries is bound by registers, not LDS.  Larger binnings are counted in
//     runs (for_runs).
//   * MODE 0: the last bin's seven sums per lane in registers, added once at the end, as pair_count_w keeps its three.  TOP =
//     false (option pairvel_lds_top, the comparator of profiles/pairvel/README.md) sends them through the LDS atomics too.
constexpr int V_MAX_HIST = 1024;

struct VelArgs {
    const float *v1[3], *v2[3];   // velocities in cell order
    double *vsum;                 // [5][nbins * nsub]: vr1 | vr2 | u2 | vz1 | vz2
};

template <int MODE, bool TOP>
__global__ __launch_bounds__(PB) void pair_vel(PairArgs a, WeightArgs wa, VelArgs va, int ncell, unsigned long long *__restrict__ evaluated) {
    __shared__ float ix[PB], iy[PB], iz[PB], iw[PB], ivx[PB], ivy[PB], ivz[PB];
    __shared__ float e2[64];
    __shared__ int64_t nb_j0[27];
    __shared__ int nb_pre[28];               // exclusive prefix of the neighbour cells' populations
    extern __shared__ __align__(8) double hs[];   // 6 x nh sums: w w | the five velocity sums; then nh counts
    const int tid = threadIdx.x;
    const int nh = a.nbins * a.nsub;
    unsigned int *hc = reinterpret_cast<unsigned int *>(hs + 6 * nh);
    for (int q = tid; q < 6 * nh; q += PB) hs[q] = 0.0;
    for (int q = tid; q < nh; q += PB) hc[q] = 0u;
    if (tid <= a.nbins) e2[tid] = a.edges2[tid];
    __syncthreads();
    const float lo2 = e2[0], hi2 = e2[a.nbins], top2 = e2[a.nbins - 1];
    const int rx = a.g.ncx >= 3 ? 1 : 0, ry = a.g.ncy >= 3 ? 1 : 0, rz = a.g.ncz >= 3 ? 1 : 0;
    const int wy = 2 * ry + 1, wz = 2 * rz + 1, nnb = (2 * rx + 1) * wy * wz;
    double top[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // MODE 0: the last bin, per lane
    unsigned long long top_n = 0, n_eval = 0;
    for (int c1 = blockIdx.x; c1 < ncell; c1 += gridDim.x) {
        const int64_t cbeg = a.start1[c1], cend = a.start1[c1 + 1];
        if (cbeg == cend) continue;
        __syncthreads();   // the previous cell's reads of the neighbour table and of the slice are done
        if (tid < 64) {
            int len = 0;
            int64_t j0 = 0;
            if (tid < nnb) {
                const int cz = c1 % a.g.ncz, cy = (c1 / a.g.ncz) % a.g.ncy, cx = c1 / (a.g.ncz * a.g.ncy);
                int nx = cx + tid / (wy * wz) - rx, ny = cy + (tid / wz) % wy - ry, nz = cz + tid % wz - rz;
                nx = nx < 0 ? nx + a.g.ncx : (nx >= a.g.ncx ? nx - a.g.ncx : nx);
                ny = ny < 0 ? ny + a.g.ncy : (ny >= a.g.ncy ? ny - a.g.ncy : ny);
                nz = nz < 0 ? nz + a.g.ncz : (nz >= a.g.ncz ? nz - a.g.ncz : nz);
                const int c2 = (nx * a.g.ncy + ny) * a.g.ncz + nz;
                j0 = a.start2[c2];
                len = (int)(a.start2[c2 + 1] - j0);
            }
            int incl = len;
#pragma unroll
            for (int d = 1; d < 32; d <<= 1) {
                const int v = __shfl_up(incl, d, 64);
                if (tid >= d) incl += v;
            }
            if (tid < nnb) nb_j0[tid] = j0, nb_pre[tid] = incl - len;
            if (tid == nnb - 1) nb_pre[nnb] = incl;
        }
        __syncthreads();
        const int M = nb_pre[nnb];
        for (int64_t i0 = cbeg; i0 < cend; i0 += PB) {
            const int ni = (int)min((int64_t)PB, cend - i0);
            if (i0 > cbeg) __syncthreads();   // the previous slice's reads are done
            if (tid < ni) {
                ix[tid] = a.x1[i0 + tid], iy[tid] = a.y1[i0 + tid], iz[tid] = a.z1[i0 + tid];
                iw[tid] = wa.w1 ? wa.w1[i0 + tid] : 1.0f;
                ivx[tid] = va.v1[0][i0 + tid], ivy[tid] = va.v1[1][i0 + tid], ivz[tid] = va.v1[2][i0 + tid];
            }
            __syncthreads();
            for (int base = 0; base < M; base += PB) {
                n_eval += (unsigned long long)ni * (unsigned long long)min(PB, M - base);
                const int v = base + tid;
                if (v >= M) continue;
                int sg = 0;
                while (nb_pre[sg + 1] <= v) sg++;        // v < nb_pre[nnb]: ends at a non-empty cell
                const int64_t jj = nb_j0[sg] + (v - nb_pre[sg]);
                const float xj = a.x2[jj], yj = a.y2[jj], zj = a.z2[jj];
                const float vxj = va.v2[0][jj], vyj = va.v2[1][jj], vzj = va.v2[2][jj];
                const double wj = wa.w2 ? (double)wa.w2[jj] : 1.0;
                for (int i = 0; i < ni; i++) {
                    if (a.autocorr && jj == i0 + i) continue;   // the same point (the two sorted sets are one array)
                    const float dx = min_image(ix[i] - xj, a.half, a.g.box);
                    const float dy = min_image(iy[i] - yj, a.half, a.g.box);
                    const float dz = min_image(iz[i] - zj, a.half, a.g.box);
                    float r2;
                    int sub = 0;
                    if (MODE == 1) {
                        const float adz = fabsf(dz);
                        if (adz >= a.pimax) continue;
                        r2 = dx * dx + dy * dy;
                        if (r2 < lo2 || r2 >= hi2) continue;
                        sub = (int)(adz / a.dpi);
                        if (sub >= a.nsub) continue;
                    } else {
                        r2 = dx * dx + dy * dy + dz * dz;
                        if (r2 < lo2 || r2 >= hi2) continue;
                    }
                    if (MODE == 2) {
                        const float sep = sqrtf(r2);
                        const float mu = sep > 0.f ? fabsf(dz) / sep : 0.f;
                        if (mu >= a.mu_max) continue;
                        sub = (int)(mu * a.inv_dmu);
                        if (sub >= a.nsub) continue;
                    }
                    // a counted pair: the float64 part
                    const float fux = ivx[i] - vxj, fuy = ivy[i] - vyj, fuz = ivz[i] - vzj;
                    const double ddx = (double)dx, ddy = (double)dy, ddz = (double)dz;
                    const double ux = (double)fux, uy = (double)fuy, uz = (double)fuz;
                    const double s2 = ddx * ddx + ddy * ddy + ddz * ddz;
                    const double t = ux * ddx + uy * ddy + uz * ddz;
                    const double vr = s2 > 0.0 ? t / sqrt(s2) : 0.0;
                    const double uu = ux * ux + uy * uy + uz * uz;
                    const double vz = dz > 0.f ? uz : (dz < 0.f ? -uz : 0.0);
                    const double ww = (double)iw[i] * wj;
                    const double term[6] = {ww, ww * vr, ww * (vr * vr), ww * uu, ww * vz, ww * (uz * uz)};
                    if (MODE == 0 && TOP && r2 >= top2) {
                        top_n++;
#pragma unroll
                        for (int k = 0; k < 6; k++) top[k] += term[k];
                        continue;
                    }
                    int b = a.nbins - 1;
                    while (r2 < e2[b]) b--;
                    const int q = b * a.nsub + sub;
                    atomicAdd(&hc[q], 1u);
#pragma unroll
                    for (int k = 0; k < 6; k++) atomicAdd(&hs[k * nh + q], term[k]);
                }
            }
        }
    }
    if (tid == 0 && n_eval) atomicAdd(evaluated, n_eval);
    if (MODE == 0 && TOP && top_n) {
        // a lane's share of a workgroup's last-bin pairs stays far below 2^32
        const int q = a.nbins - 1;
        atomicAdd(&hc[q], (unsigned int)top_n);
#pragma unroll
        for (int k = 0; k < 6; k++) atomicAdd(&hs[k * nh + q], top[k]);
    }
    __syncthreads();
    for (int q = tid; q < nh; q += PB)
        if (hc[q]) {
            atomicAdd(&a.npairs[q], (unsigned long long)hc[q]);
            atomicAdd(&wa.wsum[q], hs[q]);
#pragma unroll
            for (int k = 0; k < 5; k++) atomicAdd(&va.vsum[k * nh + q], hs[(k + 1) * nh + q]);
        }
}

// Light cones: pair counts with a PAIRWISE line of sight on an OPEN grid (abacus_paircount_los, Corrfunc.mocks' DDrppi_mocks /
// DDsmu_mocks on Cartesian columns).  No reference code and no Corrfunc run stands behind this; the conventions are restated
// here and pinned against the NumPy statement tests/pairs_los_statement.py.
//   points: observer-centred float32, p = float32(column - origin) with the subtraction in the column's own dtype;
//   per ordered pair (self pairs of an autocorrelation excluded): d = p_i - p_j and l = p_i + p_j componentwise in float32,
//   then float64, left to right, no FMA: s2 = dx dx + dy dy + dz dz, l2 = lx lx + ly ly + lz lz, t = dx lx + dy ly + dz lz,
//   pi2 = t t / l2; a pair with l2 == 0 has no line of sight and is not counted in modes 1 and 2;
//   mode 0: bin s2.   mode 1: pi = sqrt(pi2) < (double)pimax, rp2 = max(s2 - pi2, 0) is binned, sub = int(pi / ((double)pimax
//   / npibins)).   mode 2: bin s2, mu = s2 > 0 ? sqrt(pi2 / s2) : 0 < (double)mu_max, sub = int(mu * (nmubins / (double)mu_max));
//   a sub >= the number of sub-bins drops the pair; float32 edges compared as e2[b] = (double)edge (double)edge,
//   bin b: e2[b] <= q < e2[b + 1]; per (bin, sub-bin) npairs, wsum = sum w_i w_j (float64 product of float32 weights) and
//   rsum = sum sqrt(q) of the q that chose the bin, float64.
// float64 because rp^2 = s^2 - pi^2 cancels at light-cone distances: with |p| ~ 4000 and pi ~ 30 float32 leaves ~1e-4 on rp^2,
// percent-level at rp = 0.1.
//
// Pre-test (cannot change membership).  s2f = dx dx + dy dy + dz dz in float32 from the SAME float32 d: three products and two
// sums of non-negative terms, each rounded once, so s2f = s2 (1 + e) with |e| < 3.1 2^-24 < 2^-22 against the exact - and the
// float64 (error 2^-52) - s2, as long as no product underflows.
//   upper: a counted pair has s2 < R2 (1 + 2^-50), R2 = e2[nbins] (modes 0, 2) or e2[nbins] + pimax^2 (mode 1: rp2 < e2[nbins]
//   and pi < pimax give s2 <= rp2 + pi2 up to two float64 roundings).  pre_hi = float32(R2 (1 + 2^-20)) rounded UP: s2f > pre_hi
//   implies s2 > R2 (1 + 2^-20) (1 - 2^-22) > R2 (1 + 2^-50): never counted.
//   lower (modes 0, 2 only; rp2 of mode 1 may be small whatever s2 is): a counted pair has s2 >= e2[0].  pre_lo =
//   float32(e2[0] (1 - 2^-20)) rounded DOWN, and 0 (test off) when that is below 1e-30: above it an underflowing product
//   (< 1.2e-38 lost) moves s2f by less than 2^-22 relative too.  s2f < pre_lo implies s2 < e2[0] (1 - 2^-20) (1 + 2^-22) < e2[0].
// NaN fails both comparisons and falls to the float64 path, which counts nothing for it.
struct LosArgs {
    int autocorr, nc[3], nbins, nsub;
    // float32 pre-test: a candidate with s2f > pre_hi or s2f < pre_lo skips the float64 arithmetic (see above)
    float pre_lo, pre_hi;
    double pimax, dpi, mu_max, inv_dmu;
    const double *edges2;   // (nbins + 1) squared edges
    const float *x1, *y1, *z1, *w1, *x2, *y2, *z2, *w2;   // cell order; w NULL: unit weights
    const int64_t *start1, *start2;
    unsigned long long *npairs;
    double *wsum, *rsum;
};

// The walk of pair_count_w on the open grid: a persistent workgroup per non-empty cell of set 1, the in-range neighbour cells
// as ONE virtual list; LDS histogram ([WEIGHTED: sums of w w] [RSUM: sums of sqrt(q)] counts), flushed once per workgroup; full
// stencil for the autocorrelation; MODE 0 keeps the last bin in registers.
template <int MODE, bool WEIGHTED, bool RSUM>
__global__ __launch_bounds__(PB) void pair_count_los(LosArgs a, int ncell, unsigned long long *__restrict__ evaluated) {
    __shared__ float ix[PB], iy[PB], iz[PB], iw[PB];
    __shared__ double e2[64];
    __shared__ int64_t nb_j0[27];
    __shared__ int nb_pre[28];               // exclusive prefix of the neighbour cells' populations
    extern __shared__ __align__(8) double hw[];   // [nh sums of w w] [nh sums of sqrt(q)] nh counts
    const int tid = threadIdx.x;
    const int nh = a.nbins * a.nsub;
    double *hr = hw + (WEIGHTED ? nh : 0);
    unsigned int *hc = reinterpret_cast<unsigned int *>(hr + (RSUM ? nh : 0));
    for (int q = tid; q < nh; q += PB) {
        hc[q] = 0u;
        if (WEIGHTED) hw[q] = 0.0;
        if (RSUM) hr[q] = 0.0;
    }
    if (tid <= a.nbins) e2[tid] = a.edges2[tid];
    __syncthreads();
    const double lo2 = e2[0], hi2 = e2[a.nbins], top2 = e2[a.nbins - 1];
    const int ncx = a.nc[0], ncy = a.nc[1], ncz = a.nc[2];
    double top_w = 0.0, top_r = 0.0;         // MODE 0: the last bin, per lane
    unsigned long long top_n = 0, n_eval = 0;
    for (int c1 = blockIdx.x; c1 < ncell; c1 += gridDim.x) {
        const int64_t cbeg = a.start1[c1], cend = a.start1[c1 + 1];
        if (cbeg == cend) continue;
        __syncthreads();   // the previous cell's reads of the neighbour table and of the slice are done
        if (tid < 64) {
            int len = 0;
            int64_t j0 = 0;
            if (tid < 27) {
                const int cz = c1 % ncz, cy = (c1 / ncz) % ncy, cx = c1 / (ncz * ncy);
                const int nx = cx + tid / 9 - 1, ny = cy + (tid / 3) % 3 - 1, nz = cz + tid % 3 - 1;
                if (nx >= 0 && nx < ncx && ny >= 0 && ny < ncy && nz >= 0 && nz < ncz) {   // open grid: nothing wraps
                    const int c2 = (nx * ncy + ny) * ncz + nz;
                    j0 = a.start2[c2];
                    len = (int)(a.start2[c2 + 1] - j0);
                }
            }
            int incl = len;
#pragma unroll
            for (int d = 1; d < 32; d <<= 1) {
                const int v = __shfl_up(incl, d, 64);
                if (tid >= d) incl += v;
            }
            if (tid < 27) nb_j0[tid] = j0, nb_pre[tid] = incl - len;
            if (tid == 26) nb_pre[27] = incl;
        }
        __syncthreads();
        const int M = nb_pre[27];
        for (int64_t i0 = cbeg; i0 < cend; i0 += PB) {
            const int ni = (int)min((int64_t)PB, cend - i0);
            if (i0 > cbeg) __syncthreads();   // the previous slice's reads are done
            if (tid < ni) {
                ix[tid] = a.x1[i0 + tid], iy[tid] = a.y1[i0 + tid], iz[tid] = a.z1[i0 + tid];
                iw[tid] = WEIGHTED && a.w1 ? a.w1[i0 + tid] : 1.0f;
            }
            __syncthreads();
            for (int base = 0; base < M; base += PB) {
                n_eval += (unsigned long long)ni * (unsigned long long)min(PB, M - base);
                const int v = base + tid;
                if (v >= M) continue;
                int sg = 0;
                while (nb_pre[sg + 1] <= v) sg++;        // v < nb_pre[27]: ends at a non-empty cell
                const int64_t jj = nb_j0[sg] + (v - nb_pre[sg]);
                const float xj = a.x2[jj], yj = a.y2[jj], zj = a.z2[jj];
                const double wj = WEIGHTED && a.w2 ? (double)a.w2[jj] : 1.0;
                for (int i = 0; i < ni; i++) {
                    const float dxf = ix[i] - xj, dyf = iy[i] - yj, dzf = iz[i] - zj;
                    const float s2f = dxf * dxf + dyf * dyf + dzf * dzf;
                    if (s2f > a.pre_hi || s2f < a.pre_lo) continue;
                    if (a.autocorr && jj == i0 + i) continue;   // the same point (the two sorted sets are one array)
                    const double dx = (double)dxf, dy = (double)dyf, dz = (double)dzf;
                    const double s2 = dx * dx + dy * dy + dz * dz;
                    double q = s2, pi2 = 0.0;
                    int sub = 0;
                    if (MODE == 0) {
                        if (!(q >= lo2 && q < hi2)) continue;
                    } else {
                        if (MODE == 2 && !(q >= lo2 && q < hi2)) continue;
                        const double lx = (double)(ix[i] + xj), ly = (double)(iy[i] + yj), lz = (double)(iz[i] + zj);
                        const double l2 = lx * lx + ly * ly + lz * lz;
                        if (l2 == 0.0) continue;                // no line of sight
                        const double t = dx * lx + dy * ly + dz * lz;
                        pi2 = t * t / l2;
                        if (MODE == 1) {
                            const double pi = sqrt(pi2);
                            if (!(pi < a.pimax)) continue;
                            const double rp2 = s2 - pi2;
                            q = rp2 > 0.0 ? rp2 : 0.0;
                            if (!(q >= lo2 && q < hi2)) continue;
                            sub = (int)(pi / a.dpi);
                        } else {
                            const double mu = s2 > 0.0 ? sqrt(pi2 / s2) : 0.0;
                            if (!(mu < a.mu_max)) continue;
                            sub = (int)(mu * a.inv_dmu);
                        }
                        if (sub >= a.nsub) continue;
                    }
                    const double ww = WEIGHTED ? (double)iw[i] * wj : 0.0;
                    if (MODE == 0 && q >= top2) {
                        top_n++;
                        if (WEIGHTED) top_w += ww;
                        if (RSUM) top_r += sqrt(q);
                        continue;
                    }
                    int b = a.nbins - 1;
                    while (q < e2[b]) b--;
                    const int h = b * a.nsub + sub;
                    atomicAdd(&hc[h], 1u);
                    if (WEIGHTED) atomicAdd(&hw[h], ww);
                    if (RSUM) atomicAdd(&hr[h], sqrt(q));
                }
            }
        }
    }
    if (tid == 0 && n_eval) atomicAdd(evaluated, n_eval);
    if (MODE == 0 && top_n) {
        // a lane's share of a workgroup's last-bin pairs stays far below 2^32
        const int h = a.nbins - 1;
        atomicAdd(&hc[h], (unsigned int)top_n);
        if (WEIGHTED) atomicAdd(&hw[h], top_w);
        if (RSUM) atomicAdd(&hr[h], top_r);
    }
    __syncthreads();
    for (int q = tid; q < nh; q += PB)
        if (hc[q]) {
            atomicAdd(&a.npairs[q], (unsigned long long)hc[q]);
            if (WEIGHTED) atomicAdd(&a.wsum[q], hw[q]);
            if (RSUM) atomicAdd(&a.rsum[q], hr[q]);
        }
}

// ------------------------------------------------------------------------------------------------------------- host side ----
struct SortedSet {
    DevBuf sorted, counts, cellid, start, keys2, idx, idx2, tmp, packed, wsorted, vsorted;
    float *sx, *sy, *sz, *sw;   // sw: the weights in cell order (weighted counts with weights for this set), else NULL
    float *sv[3];               // the velocities in cell order (sort_into_cells with velocities), else stale
    int64_t n;
};

// Empty frame, block of flags and counters in HBM: [0] outside, [16] Frame, [48] candidate pairs evaluated
const Frame EMPTY_FRAME = {{0xffffffffu, 0xffffffffu, 0xffffffffu}, {0u, 0u, 0u}};
struct Flags {
    int *outside;
    Frame *frame;
    unsigned long long *evaluated;
};

// The work buffers of every counter of this file: the library serialises its entry points (ABACUS_ENTER), so the periodic and
// the light-cone driver take turns on one set
struct Work {
    SortedSet S[2];
    DevBuf cols[2], wts[2];   // staged float32 columns and weights of the two sets
    DevBuf vcols[2];          // and their staged velocities (abacus_pairvel)
    DevBuf scratch, edges, out, list, flag;
    int flags(Flags &f) {
        ABACUS_TRY(flag.reserve(64));
        f.outside = flag.as<int>(), f.frame = reinterpret_cast<Frame *>(flag.as<char>() + 16);
        f.evaluated = reinterpret_cast<unsigned long long *>(flag.as<char>() + 48);
        HIP_TRY(hipMemsetAsync(flag.p, 0, 64, stream()));
        HIP_TRY(hipMemcpyAsync(f.frame, &EMPTY_FRAME, sizeof EMPTY_FRAME, hipMemcpyHostToDevice, stream()));
        return 0;
    }
} g_work;

struct Columns {   // float32 device columns of a set, with its weights (NULL: none)
    const float *x[3], *w;
};

// Caller columns -> float32 device columns.  where = 0: host float32 arrays (and host weights); 1: device float32; 2: device
// float64 (device weights).  origin (NULL: none) is subtracted in the column's own dtype before the one rounding; device float32
// columns that need no shift are read in place.  n > 0.  `label` names the conversion kernel to the profiler.
int stage_columns(const char *label, const void *const src[3], const float *w, int where, int64_t n, const double *origin,
                  DevBuf &cols, DevBuf &wts, Columns &c) {
    const bool shifted = origin && (origin[0] != 0.0 || origin[1] != 0.0 || origin[2] != 0.0);
    const int nblk = (int)std::min<int64_t>(ceil_div(n, 256), 2048);
    if (where == 1 && !shifted) {
        for (int d = 0; d < 3; d++) c.x[d] = (const float *)src[d];
    } else {
        ABACUS_TRY(cols.reserve(3 * (size_t)n * 4));
        for (int d = 0; d < 3; d++) {
            float *dst = cols.as<float>() + (size_t)d * n;
            const double o = origin ? origin[d] : 0.0;
            c.x[d] = dst;
            if (where == 2) {
                ABACUS_LAUNCH(label, los_centre<double>, dim3(nblk), dim3(256), 0, (const double *)src[d], o, dst, n);
                continue;
            }
            const float *from = (const float *)src[d];
            if (where == 0) {
                HIP_TRY(hipMemcpyAsync(dst, from, (size_t)n * 4, hipMemcpyHostToDevice, stream()));
                from = dst;
            }
            if (shifted) ABACUS_LAUNCH(label, los_centre<float>, dim3(nblk), dim3(256), 0, from, (float)o, dst, n);
        }
    }
    c.w = w;
    if (w && where == 0) {
        ABACUS_TRY(wts.reserve((size_t)n * 4));
        HIP_TRY(hipMemcpyAsync(wts.p, w, (size_t)n * 4, hipMemcpyHostToDevice, stream()));
        c.w = wts.as<float>();
    }
    return 0;
}

template <bool COUNT, bool W, typename Grid>
int count_cells(const Columns &c, int64_t n, const Grid &g, SortedSet &s, int nblk) {
    ABACUS_LAUNCH("pair_cell_count", (cell_count<COUNT, W, Grid>), dim3(nblk), dim3(256), 0, c.x[0], c.x[1], c.x[2], COUNT ? nullptr : c.w, n, g,
                  COUNT ? s.counts.as<unsigned int>() : nullptr, s.cellid.as<unsigned int>(), COUNT ? nullptr : s.idx.as<unsigned int>(),
                  COUNT ? nullptr : s.packed.as<float4>());
    return 0;
}

// The set in cell order on either grid (ncell cells): s.sx | sy | sz, s.start and - with weights - s.sw.  vel (NULL: none): three
// float32 device columns that follow their points into s.sv; such a set takes the radix sort at every size, whose sorted index
// says where a point went (the counting sort hands out slots by atomics and keeps no index).  n > 0 with vel.
template <typename Grid>
int sort_into_cells(const Columns &c, int64_t n, const Grid &g, int64_t ncell, SortedSet &s, DevBuf &scratch, const float *const *vel = nullptr) {
    const size_t n1 = (size_t)std::max<int64_t>(n, 1);
    s.n = n;
    ABACUS_TRY(s.sorted.reserve(3 * n1 * 4));
    ABACUS_TRY(s.counts.reserve((size_t)(ncell + 1) * 4));
    ABACUS_TRY(s.cellid.reserve(n1 * 4));
    ABACUS_TRY(s.start.reserve((size_t)(ncell + 1) * 8));
    const float *rx = c.x[0], *ry = c.x[1], *rz = c.x[2], *rw = c.w;
    s.sx = s.sorted.as<float>();
    s.sy = s.sx + n1;
    s.sz = s.sy + n1;
    const int nblk = (int)std::min<int64_t>(std::max<int64_t>(ceil_div(n, 256), 1), 2048);
    s.sw = nullptr;
    if (rw) {
        ABACUS_TRY(s.wsorted.reserve(n1 * 4));
        s.sw = s.wsorted.as<float>();
    }
    // large inputs: stable radix sort of (cell id, index) + gather + a search per cell (10^7 points: 0.6 ms against 2.2 ms of
    // the counting sort below, whose two passes are a global atomic per point each)
    if (vel || (n >= 200000 && n < ((int64_t)1 << 31) && !option("pairs_countsort"))) {
        ABACUS_TRY(s.keys2.reserve(n1 * 4));
        ABACUS_TRY(s.idx.reserve(n1 * 4));
        ABACUS_TRY(s.idx2.reserve(n1 * 4));
        ABACUS_TRY(s.packed.reserve(n1 * 16));
        if (rw) ABACUS_TRY((count_cells<false, true>(c, n, g, s, nblk)));
        else ABACUS_TRY((count_cells<false, false>(c, n, g, s, nblk)));
        int end_bit = 1;
        while (((int64_t)1 << end_bit) < ncell) end_bit++;
        size_t tmp_bytes = 0;
        (void)hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, s.cellid.as<unsigned int>(), s.keys2.as<unsigned int>(),
                                                 s.idx.as<unsigned int>(), s.idx2.as<unsigned int>(), (int)n, 0, end_bit, stream());
        ABACUS_TRY(s.tmp.reserve(tmp_bytes));
        prof_begin("pair_cell_sort");         // library kernels (rocPRIM radix sort of the cell ids): listed with the hand-written ones
        const hipError_t sorted = hipcub::DeviceRadixSort::SortPairs(s.tmp.p, tmp_bytes, s.cellid.as<unsigned int>(), s.keys2.as<unsigned int>(),
                                                                     s.idx.as<unsigned int>(), s.idx2.as<unsigned int>(), (int)n, 0, end_bit, stream());
        prof_end("pair_cell_sort");
        if (sorted != hipSuccess) return fail("abacus_paircount: radix sort failed");
        if (rw)
            ABACUS_LAUNCH("pair_cell_fill", cell_gather<true>, dim3(nblk), dim3(256), 0, s.packed.as<float4>(), n, s.idx2.as<unsigned int>(),
                          s.sx, s.sy, s.sz, s.sw);
        else
            ABACUS_LAUNCH("pair_cell_fill", cell_gather<false>, dim3(nblk), dim3(256), 0, s.packed.as<float4>(), n, s.idx2.as<unsigned int>(),
                          s.sx, s.sy, s.sz, s.sw);
        if (vel) {
            ABACUS_TRY(s.vsorted.reserve(3 * n1 * 4));
            for (int d = 0; d < 3; d++) s.sv[d] = s.vsorted.as<float>() + (size_t)d * n1;
            ABACUS_LAUNCH("pair_vel_gather", vel_gather, dim3(nblk), dim3(256), 0, vel[0], vel[1], vel[2], n, s.idx2.as<unsigned int>(), s.sv[0],
                          s.sv[1], s.sv[2]);
        }
        const int cblk = (int)std::min<int64_t>(ceil_div(ncell + 1, 256), 8192);
        ABACUS_LAUNCH("pair_cell_starts", cell_starts, dim3(cblk), dim3(256), 0, s.keys2.as<unsigned int>(), n, ncell, s.start.as<int64_t>());
        return 0;
    }
    HIP_TRY(hipMemsetAsync(s.counts.p, 0, (size_t)(ncell + 1) * 4, stream()));
    if (n > 0) ABACUS_TRY((count_cells<true, false>(c, n, g, s, nblk)));
    ABACUS_TRY(exclusive_scan_u32(s.counts.as<unsigned int>(), ncell, s.start.as<int64_t>(), scratch, 1));
    if (n > 0 && rw)
        ABACUS_LAUNCH("pair_cell_fill", cell_fill<true>, dim3(nblk), dim3(256), 0, rx, ry, rz, rw, n,
                      s.cellid.as<unsigned int>(), s.start.as<int64_t>(), s.counts.as<unsigned int>(), s.sx, s.sy, s.sz, s.sw);
    else if (n > 0)
        ABACUS_LAUNCH("pair_cell_fill", cell_fill<false>, dim3(nblk), dim3(256), 0, rx, ry, rz, rw, n,
                      s.cellid.as<unsigned int>(), s.start.as<int64_t>(), s.counts.as<unsigned int>(), s.sx, s.sy, s.sz, s.sw);
    return 0;
}

// f(std::integral_constant<int, mode>()): the mode as a template argument of what f launches
template <typename F>
int with_mode(int mode, F &&f) {
    if (mode == 0) return f(std::integral_constant<int, 0>());
    if (mode == 1) return f(std::integral_constant<int, 1>());
    return f(std::integral_constant<int, 2>());
}
template <typename F>
int with_flag(bool on, F &&f) { return on ? f(std::true_type()) : f(std::false_type()); }

int cu_count(int &ncu) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    return 0;
}

// grid of persistent workgroups: min(jobs, CUs x resident workgroups of this kernel at this block size and dynamic LDS)
template <typename K>
int resident_grid(K kernel, int block, size_t lds, int64_t jobs, dim3 &grid) {
    int ncu = 256, per_cu = 1;
    ABACUS_TRY(cu_count(ncu));
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)kernel, block, lds));
    grid = dim3((unsigned int)std::min<int64_t>(jobs, (int64_t)ncu * std::max(per_cu, 1)));
    return 0;
}

// One launch bins into at most 63 separation bins (the kernels' edge tables) and max_hist LDS histogram entries.  More bins -
// Corrfunc takes any number - are counted in runs of consecutive separation bins, each on a grid of its own, smaller reach; a
// pair ON an edge shared by two runs belongs to the upper bin in both ([lo, hi) bins).  f(first bin, bins, offset in the outputs)
template <typename F>
int for_runs(int nbins, int nsub, int max_hist, F &&f) {
    const int run = std::min(63, max_hist / nsub);
    for (int b0 = 0; b0 < nbins; b0 += run) ABACUS_TRY(f(b0, std::min(run, nbins - b0), (size_t)b0 * nsub));
    return 0;
}

// the squared edges of a run in the kernel's edge type, on the host and in g_work.edges
template <typename Q>
int upload_edges(const float *edges, int nb, std::vector<Q> &e2) {
    e2.resize(nb + 1);
    for (int b = 0; b <= nb; b++) e2[b] = (Q)edges[b] * (Q)edges[b];
    ABACUS_TRY(g_work.edges.reserve((size_t)(nb + 1) * sizeof(Q)));
    HIP_TRY(hipMemcpyAsync(g_work.edges.p, e2.data(), (size_t)(nb + 1) * sizeof(Q), hipMemcpyHostToDevice, stream()));
    return 0;
}

// outputs of a run: ntot counts [| ntot sums of w w | ntot sums of the separation] in g_work.out
struct Outputs {
    uint64_t *npairs;
    double *wsum, *rsum;   // NULL: not asked for
    double *vsum = nullptr;   // abacus_pairvel: five velocity sums, [5][vstride] with this block's entries at the front of each row
    size_t vstride = 0;
    Outputs at(size_t o) const { return Outputs{npairs + o, wsum ? wsum + o : nullptr, rsum ? rsum + o : nullptr, vsum ? vsum + o : nullptr, vstride}; }
    void zero(size_t ntot) const {
        memset(npairs, 0, ntot * sizeof(uint64_t));
        if (wsum) memset(wsum, 0, ntot * sizeof(double));
        if (rsum) memset(rsum, 0, ntot * sizeof(double));
        if (vsum) memset(vsum, 0, 5 * vstride * sizeof(double));
    }
};
int device_outputs(size_t ntot, bool sums, bool vel, Outputs &d) {
    const size_t bytes = ((sums ? 3 : 1) + (vel ? 5 : 0)) * ntot * 8;
    ABACUS_TRY(g_work.out.reserve(bytes));
    HIP_TRY(hipMemsetAsync(g_work.out.p, 0, bytes, stream()));
    d.npairs = g_work.out.as<uint64_t>();
    d.wsum = sums ? g_work.out.as<double>() + ntot : nullptr, d.rsum = sums ? d.wsum + ntot : nullptr;
    d.vsum = vel ? g_work.out.as<double>() + (sums ? 3 : 1) * ntot : nullptr, d.vstride = ntot;
    return 0;
}
int fetch_outputs(const Outputs &h, const Outputs &d, size_t ntot) {
    HIP_TRY(hipMemcpyAsync(h.npairs, d.npairs, ntot * 8, hipMemcpyDeviceToHost, stream()));
    if (h.wsum) HIP_TRY(hipMemcpyAsync(h.wsum, d.wsum, ntot * 8, hipMemcpyDeviceToHost, stream()));
    if (h.rsum) HIP_TRY(hipMemcpyAsync(h.rsum, d.rsum, ntot * 8, hipMemcpyDeviceToHost, stream()));
    for (int k = 0; k < 5 && h.vsum; k++)
        HIP_TRY(hipMemcpyAsync(h.vsum + k * h.vstride, d.vsum + k * d.vstride, ntot * 8, hipMemcpyDeviceToHost, stream()));
    return 0;
}

// the sorted sets and the outputs of a run, as a kernel reads them: Args = PairArgs | LosArgs, Sums = WeightArgs | LosArgs
template <typename Args, typename Sums>
void fill_sets(Args &a, Sums &s, int autocorr, int nbins, int nsub, const Outputs &d) {
    const SortedSet &S1 = g_work.S[0], &T = g_work.S[autocorr ? 0 : 1];
    a.autocorr = autocorr, a.nbins = nbins, a.nsub = nsub;
    a.x1 = S1.sx, a.y1 = S1.sy, a.z1 = S1.sz, a.x2 = T.sx, a.y2 = T.sy, a.z2 = T.sz;
    a.start1 = S1.start.as<int64_t>(), a.start2 = T.start.as<int64_t>();
    a.npairs = reinterpret_cast<unsigned long long *>(d.npairs);
    s.w1 = S1.sw, s.w2 = T.sw, s.wsum = d.wsum, s.rsum = d.rsum;
}

// The launches of a run, one function per walk; the two drivers (below the jackknife kernels) choose among them.  Each stands
// behind the instantiation of its family's sort: the code object lists kernels in the order of their instantiation, and the
// launches keep that order whichever driver calls them.
template int sort_into_cells<FramedGrid>(const Columns &, int64_t, const FramedGrid &, int64_t, SortedSet &, DevBuf &, const float *const *);

int launch_weighted(const PairArgs &a, const WeightArgs &wa, bool rsum, const Flags &fl, int64_t ncell) {
    const size_t hist_bytes = (size_t)a.nbins * a.nsub * 20;   // <= W_MAX_HIST * 20 = 40 KiB beside 5 KiB of static LDS
    return with_mode(a.mode, [&](auto M) {
        return with_flag(rsum, [&](auto RS) -> int {
            const auto kernel = pair_count_w<decltype(M)::value, decltype(RS)::value>;
            dim3 grid;
            ABACUS_TRY(resident_grid(kernel, PB, hist_bytes, ncell, grid));
            ABACUS_LAUNCH("pair_count_w", kernel, grid, dim3(PB), hist_bytes, a, wa, (int)ncell, fl.evaluated);
            return 0;
        });
    });
}

// The unweighted periodic count of a run by the generation asked for (pairs_gen; 1, 2: the comparators of the tests); R_used:
// the stencil of pair_count3, 0 when an older kernel ran
int launch_unweighted(PairArgs &a, int gen, int R, const std::vector<float> &e2, const Flags &fl, int64_t ncell, int &R_used) {
    Work &W = g_work;
    const CellGrid &g = a.g;
    const int nb = a.nbins;
    const size_t ntot = (size_t)nb * a.nsub;
    R_used = 0;
    if (gen == 1) {   // first-generation kernel: host-built work list, one workgroup per 256 points of a non-empty cell
        std::vector<int64_t> start1((size_t)ncell + 1);
        HIP_TRY(hipMemcpyAsync(start1.data(), W.S[0].start.p, (size_t)(ncell + 1) * 8, hipMemcpyDeviceToHost, stream()));
        HIP_TRY(hipStreamSynchronize(stream()));
        std::vector<int> wc, wo;
        for (int64_t c = 0; c < ncell; c++)
            for (int64_t off = 0; off < start1[c + 1] - start1[c]; off += PB) wc.push_back((int)c), wo.push_back((int)off);
        const int nwork = (int)wc.size();
        ABACUS_TRY(W.list.reserve((size_t)std::max(nwork, 1) * 8));
        int *d_wc = W.list.as<int>(), *d_wo = d_wc + std::max(nwork, 1);
        HIP_TRY(hipMemcpyAsync(d_wc, wc.data(), (size_t)nwork * 4, hipMemcpyHostToDevice, stream()));
        HIP_TRY(hipMemcpyAsync(d_wo, wo.data(), (size_t)nwork * 4, hipMemcpyHostToDevice, stream()));
        HIP_TRY(hipStreamSynchronize(stream()));
        if (nwork > 0) ABACUS_LAUNCH("pair_count", pair_count, dim3(nwork), dim3(PB), 0, a, d_wc, d_wo);
        return 0;
    }
    if (gen >= 3 && g.ncx >= 2 * R + 1 && g.ncy >= 2 * R + 1 && g.ncz >= 2 * R + 1) {
        R_used = R;
        // cells of the bin table: the coarsest 2^m per octave (m = 2 .. 8) that keep the inner edges apart, at most 8192 cells
        a.no_blocks = option("pairs_noblocks");
        if (!option("pairs_nolut") && e2[0] >= 0.f) {
            auto fbits = [](float v) {
                unsigned int u;
                memcpy(&u, &v, 4);
                return u;
            };
            for (int m = 2; m <= 8 && !a.lut_ncell; m++) {
                const int sh = 23 - m;
                const unsigned int c0 = fbits(e2[0]) >> sh, c1 = fbits(e2[nb]) >> sh;
                if (c1 - c0 + 1 > 8192u) break;
                bool ok = true;
                for (int b = 1; b + 1 < nb && ok; b++) ok = (fbits(e2[b]) >> sh) != (fbits(e2[b + 1]) >> sh);
                for (int b = 0; b < nb && ok; b++) ok = e2[b] < e2[b + 1];
                if (ok) a.lut_sh = sh, a.lut_off = (int)c0, a.lut_ncell = (int)(c1 - c0 + 1);
            }
        }
        const bool lut = a.lut_ncell > 0;
        const size_t hist_bytes = ((ntot + 1) & ~(size_t)1) * sizeof(unsigned int) + (size_t)a.lut_ncell * sizeof(uint2);
        return with_mode(a.mode, [&](auto M) {
            return with_flag(lut, [&](auto LUT) -> int {
                const auto kernel = pair_count3<decltype(M)::value, decltype(LUT)::value>;
                if (hist_bytes > 48 * 1024)
                    HIP_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)hist_bytes));
                dim3 grid;   // persistent waves: as many workgroups as are resident at once
                ABACUS_TRY(resident_grid(kernel, P3_WAVES * 64, hist_bytes, ceil_div(ncell, P3_WAVES), grid));
                ABACUS_LAUNCH("pair_count", kernel, grid, dim3(P3_WAVES * 64), hist_bytes, a, fl.frame, (int)ncell, R, fl.evaluated);
                return 0;
            });
        });
    }
    int ncu = 256;
    ABACUS_TRY(cu_count(ncu));
    const dim3 grid((unsigned int)std::min<int64_t>(ncell, (int64_t)ncu * 8));
    const size_t hist_bytes = ntot * sizeof(unsigned int);
    // a few points per cell: stage all neighbour cells together (one round per slice instead of 27)
    const bool agg = (double)W.S[a.autocorr ? 0 : 1].n / (double)ncell < 12.0;
    return with_mode(a.mode, [&](auto M) {
        return with_flag(agg, [&](auto AGG) -> int {
            ABACUS_LAUNCH("pair_count", (pair_count2<decltype(M)::value, decltype(AGG)::value>), grid, dim3(PB), hist_bytes, a,
                          (const int *)fl.outside, (int)ncell);
            return 0;
        });
    });
}

template int sort_into_cells<OpenGrid>(const Columns &, int64_t, const OpenGrid &, int64_t, SortedSet &, DevBuf &, const float *const *);

// weighted: with sums of w w; rs: and of the separation
int launch_los(int mode, const LosArgs &a, bool weighted, bool rs, const Flags &fl, int64_t ncell) {
    const size_t hist_bytes = (size_t)a.nbins * a.nsub * (4 + (weighted ? 8 : 0) + (rs ? 8 : 0));
    auto launch = [&](auto M, auto WT, auto RS) -> int {
        const auto kernel = pair_count_los<decltype(M)::value, decltype(WT)::value, decltype(RS)::value>;
        dim3 grid;
        ABACUS_TRY(resident_grid(kernel, PB, hist_bytes, ncell, grid));
        ABACUS_LAUNCH("pair_count_los", kernel, grid, dim3(PB), hist_bytes, a, (int)ncell, fl.evaluated);
        return 0;
    };
    return with_mode(mode, [&](auto M) {
        if (rs) return launch(M, std::true_type(), std::true_type());
        if (weighted) return launch(M, std::true_type(), std::false_type());
        return launch(M, std::false_type(), std::false_type());
    });
}

}  // namespace

// a device column, observer-centred: dst = float32(src - origin), the subtraction in the column's dtype (the estimators of
// analysis/tpcf_corrfunc.py centre a sample once and count it against several others)
extern "C" int abacus_paircount_los_centre(const void *src, int pos_dtype, int64_t n, double origin, float *dst) {
    if (pos_dtype != ABACUS_F32 && pos_dtype != ABACUS_F64) return fail("abacus_paircount_los_centre: pos_dtype must be ABACUS_F32 or ABACUS_F64");
    if (n < 0 || (n > 0 && (!src || !dst)) || !std::isfinite(origin)) return fail("abacus_paircount_los_centre: bad argument");
    ABACUS_ENTER();
    if (n == 0) return 0;
    const dim3 grid((unsigned int)std::min<int64_t>(ceil_div(n, 256), 2048));
    if (pos_dtype == ABACUS_F64) ABACUS_LAUNCH("pair_los_centre", los_centre<double>, grid, dim3(256), 0, (const double *)src, origin, dst, n);
    else ABACUS_LAUNCH("pair_los_centre", los_centre<float>, grid, dim3(256), 0, (const float *)src, (float)origin, dst, n);
    HIP_TRY(hipStreamSynchronize(stream()));
    return 0;
}

// ------------------------------------------------------------------------------------------ jackknife pair counts ----
// Per-region pair counts in ONE walk (abacus_paircount_jk, abacus_paircount_los_jk): every point carries an int32 label in
// [0, nreg) and per (bin, sub-bin) q and region k
//   first[k][q] = pairs of q whose point of set 1 has label k,     both[k][q] = those whose point of set 2 has label k too,
// as integer counts and as sums of w_i w_j (float64 products and sums, like wsum above).  total[q] = sum_k first[k][q] is the
// parent counter's result; there are no separation sums here.  second[k][q] (the point of set 2 has label k) is no output:
// membership is symmetric under exchange of the two points in every mode of both families - d -> -d negates exactly (the
// minimum image adds -+L to -+d), so r^2, |dz|, mu, and on the light cone l = p_i + p_j, |t| and pi^2 are bit-equal - hence
// second of (1, 2) is first of (2, 1): the autocorrelation has second = first, a cross count calls again with the sets
// exchanged.  The expressions that decide membership and bin are those of pair_count_w / pair_count_los, untouched.
//   * The labels ride through the cell sort (one radix sort of the key cell << bits | label - the stable label pass in front
//     of the cell pass, fused), so a cell's slice is a few runs of constant label; with sub-box regions normally one.
//   * A primary slice ends with its label run: ni = min(PB, end of run - i0), found in the slice's labels in LDS.
//   * Two LDS histograms of nh entries (first | both, each a float64 sum and a u32 count: 24 bytes per entry, JK_MAX_HIST
//     entries per launch; the unweighted light-cone count drops the sums) accumulate ONE label.  They are flushed - non-zero
//     entries, global atomics to out[label][q] - when the next run's label differs, across cells too, and at the end; a
//     workgroup walks a CONTIGUOUS range of cells (an equal share of the points), so that consecutive cells of one sub-box
//     flush once.
//   * MODE 0 keeps the last bin of both histograms in registers, per run.
// The candidate count is the parent's: splitting slices into runs leaves sum ni M unchanged.
namespace {

constexpr int JK_MAX_HIST = 2048;
constexpr int JK_MAX_REG = 65535;
constexpr int64_t JK_MAX_OUT = (int64_t)1 << 24;

struct JkOut {   // four arrays [nreg][stride]; a run's kernel writes columns 0 .. nh of every row (the pointers are offset)
    unsigned long long *nfirst, *nboth;
    double *wfirst, *wboth;   // not read by an unweighted kernel
    size_t stride;
    unsigned long long *flushes;
};

template <bool WEIGHTED>
struct JkHist {
    double *wf, *wb;
    unsigned int *cf, *cb;
    int nh;
    __device__ __forceinline__ JkHist(double *base, int n) : nh(n) {
        wf = base, wb = base + (WEIGHTED ? n : 0);
        cf = reinterpret_cast<unsigned int *>(wb + (WEIGHTED ? n : 0)), cb = cf + n;
    }
    __device__ __forceinline__ void clear() const {
        for (int q = threadIdx.x; q < nh; q += PB) {
            cf[q] = 0u, cb[q] = 0u;
            if (WEIGHTED) wf[q] = 0.0, wb[q] = 0.0;
        }
    }
    __device__ __forceinline__ void add(int q, bool same, double ww) const {
        atomicAdd(&cf[q], 1u);
        if (WEIGHTED) atomicAdd(&wf[q], ww);
        if (same) {
            atomicAdd(&cb[q], 1u);
            if (WEIGHTED) atomicAdd(&wb[q], ww);
        }
    }
    // every thread of the workgroup: the accumulated entries to region k's rows, and the histograms zero again
    __device__ __forceinline__ void flush(const JkOut &o, int k) const {
        __syncthreads();
        const size_t row = (size_t)k * o.stride;
        for (int q = threadIdx.x; q < nh; q += PB)
            if (cf[q]) {
                atomicAdd(&o.nfirst[row + q], (unsigned long long)cf[q]);
                if (WEIGHTED) atomicAdd(&o.wfirst[row + q], wf[q]), wf[q] = 0.0;
                cf[q] = 0u;
                if (cb[q]) {
                    atomicAdd(&o.nboth[row + q], (unsigned long long)cb[q]);
                    if (WEIGHTED) atomicAdd(&o.wboth[row + q], wb[q]), wb[q] = 0.0;
                    cb[q] = 0u;
                }
            }
        __syncthreads();
    }
};

// MODE 0: a lane's pairs of the last bin for the run's label (a lane's share stays far below 2^32 between two flushes)
template <bool WEIGHTED>
struct JkTop {
    unsigned long long nf = 0, nb = 0;
    double wf = 0.0, wb = 0.0;
    __device__ __forceinline__ void add(bool same, double ww) {
        nf++, wf += ww;
        if (same) nb++, wb += ww;
    }
    __device__ __forceinline__ void fold(const JkHist<WEIGHTED> &h, int q) {
        if (!nf) return;
        atomicAdd(&h.cf[q], (unsigned int)nf);
        if (WEIGHTED) atomicAdd(&h.wf[q], wf);
        if (nb) {
            atomicAdd(&h.cb[q], (unsigned int)nb);
            if (WEIGHTED) atomicAdd(&h.wb[q], wb);
        }
        nf = nb = 0, wf = wb = 0.0;
    }
};

// il[0 .. cap): the labels of the points a slice could take, ascending (the sort's order inside a cell): the length of the
// run of il[0].  Every thread searches the same way (broadcast reads)
__device__ __forceinline__ int jk_run_length(const int *il, int cap) {
    const int L = il[0];
    int lo = 1, hi = cap;   // the first index in [1, cap] whose label is not L
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (il[mid] != L) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// The cells of this workgroup: a CONTIGUOUS range holding its share of the points of set 1 - workgroup b takes the cells whose
// first point lies in [n b / G, n (b + 1) / G) (an equal share of the cells leaves most workgroups of a light cone, whose
// bounding box is mostly empty, without work).  Every thread searches the same way
__device__ __forceinline__ void jk_cell_range(const int64_t *__restrict__ start, int ncell, int &c_lo, int &c_hi) {
    const int64_t n = start[ncell];
    auto first_cell_from = [&](int64_t target) {   // the first cell whose first point is not before `target`
        int lo = 0, hi = ncell;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (start[mid] < target) lo = mid + 1;
            else hi = mid;
        }
        return lo;
    };
    c_lo = first_cell_from(n * (int64_t)blockIdx.x / (int64_t)gridDim.x);
    c_hi = blockIdx.x + 1 == gridDim.x ? ncell : first_cell_from(n * (int64_t)(blockIdx.x + 1) / (int64_t)gridDim.x);
}

// the walk of pair_count_w (no separation sums) with the two histograms of the current label
template <int MODE>
__global__ __launch_bounds__(PB) void pair_count_jk(PairArgs a, WeightArgs wa, const int *__restrict__ lab1, const int *__restrict__ lab2,
                                                    JkOut out, int ncell, unsigned long long *__restrict__ evaluated) {
    __shared__ float ix[PB], iy[PB], iz[PB], iw[PB];
    __shared__ int il[PB];
    __shared__ float e2[64];
    __shared__ int64_t nb_j0[27];
    __shared__ int nb_pre[28];               // exclusive prefix of the neighbour cells' populations
    extern __shared__ __align__(8) double jk_lds[];   // nh sums first | nh sums both | nh counts first | nh counts both
    const int tid = threadIdx.x;
    const int nh = a.nbins * a.nsub;
    const JkHist<true> h(jk_lds, nh);
    h.clear();
    if (tid <= a.nbins) e2[tid] = a.edges2[tid];
    __syncthreads();
    const float lo2 = e2[0], hi2 = e2[a.nbins], top2 = e2[a.nbins - 1];
    const int rx = a.g.ncx >= 3 ? 1 : 0, ry = a.g.ncy >= 3 ? 1 : 0, rz = a.g.ncz >= 3 ? 1 : 0;
    const int wy = 2 * ry + 1, wz = 2 * rz + 1, nnb = (2 * rx + 1) * wy * wz;
    JkTop<true> top;
    unsigned long long n_eval = 0;
    unsigned int nflush = 0;
    int cur = -1;                            // the label the histograms hold (none yet)
    int c_lo, c_hi;
    jk_cell_range(a.start1, ncell, c_lo, c_hi);
    for (int c1 = c_lo; c1 < c_hi; c1++) {
        const int64_t cbeg = a.start1[c1], cend = a.start1[c1 + 1];
        if (cbeg == cend) continue;
        __syncthreads();   // the previous cell's reads of the neighbour table and of the slice are done
        if (tid < 64) {
            int len = 0;
            int64_t j0 = 0;
            if (tid < nnb) {
                const int cz = c1 % a.g.ncz, cy = (c1 / a.g.ncz) % a.g.ncy, cx = c1 / (a.g.ncz * a.g.ncy);
                int nx = cx + tid / (wy * wz) - rx, ny = cy + (tid / wz) % wy - ry, nz = cz + tid % wz - rz;
                nx = nx < 0 ? nx + a.g.ncx : (nx >= a.g.ncx ? nx - a.g.ncx : nx);
                ny = ny < 0 ? ny + a.g.ncy : (ny >= a.g.ncy ? ny - a.g.ncy : ny);
                nz = nz < 0 ? nz + a.g.ncz : (nz >= a.g.ncz ? nz - a.g.ncz : nz);
                const int c2 = (nx * a.g.ncy + ny) * a.g.ncz + nz;
                j0 = a.start2[c2];
                len = (int)(a.start2[c2 + 1] - j0);
            }
            int incl = len;
#pragma unroll
            for (int d = 1; d < 32; d <<= 1) {
                const int v = __shfl_up(incl, d, 64);
                if (tid >= d) incl += v;
            }
            if (tid < nnb) nb_j0[tid] = j0, nb_pre[tid] = incl - len;
            if (tid == nnb - 1) nb_pre[nnb] = incl;
        }
        __syncthreads();
        const int M = nb_pre[nnb];
        for (int64_t i0 = cbeg; i0 < cend;) {
            const int cap = (int)min((int64_t)PB, cend - i0);
            if (i0 > cbeg) __syncthreads();   // the previous slice's reads are done
            if (tid < cap) {                  // the points behind the run's end are loaded again by the next slice
                ix[tid] = a.x1[i0 + tid], iy[tid] = a.y1[i0 + tid], iz[tid] = a.z1[i0 + tid];
                iw[tid] = wa.w1 ? wa.w1[i0 + tid] : 1.0f;
                il[tid] = lab1[i0 + tid];
            }
            __syncthreads();
            const int L = il[0], ni = jk_run_length(il, cap);
            if (L != cur) {                   // uniform: another region from here on
                if (cur >= 0) {
                    if (MODE == 0) top.fold(h, a.nbins - 1);
                    h.flush(out, cur);
                    nflush++;
                }
                cur = L;
            }
            for (int base = 0; base < M; base += PB) {
                n_eval += (unsigned long long)ni * (unsigned long long)min(PB, M - base);
                const int v = base + tid;
                if (v >= M) continue;
                int sg = 0;
                while (nb_pre[sg + 1] <= v) sg++;        // v < nb_pre[nnb]: ends at a non-empty cell
                const int64_t jj = nb_j0[sg] + (v - nb_pre[sg]);
                const float xj = a.x2[jj], yj = a.y2[jj], zj = a.z2[jj];
                const double wj = wa.w2 ? (double)wa.w2[jj] : 1.0;
                const bool same = lab2[jj] == L;
                for (int i = 0; i < ni; i++) {
                    if (a.autocorr && jj == i0 + i) continue;   // the same point (the two sorted sets are one array)
                    const float dx = min_image(ix[i] - xj, a.half, a.g.box);
                    const float dy = min_image(iy[i] - yj, a.half, a.g.box);
                    const float dz = min_image(iz[i] - zj, a.half, a.g.box);
                    float r2;
                    int sub = 0;
                    if (MODE == 1) {
                        const float adz = fabsf(dz);
                        if (adz >= a.pimax) continue;
                        r2 = dx * dx + dy * dy;
                        if (r2 < lo2 || r2 >= hi2) continue;
                        sub = (int)(adz / a.dpi);
                        if (sub >= a.nsub) continue;
                    } else {
                        r2 = dx * dx + dy * dy + dz * dz;
                        if (r2 < lo2 || r2 >= hi2) continue;
                    }
                    if (MODE == 2) {
                        const float sep = sqrtf(r2);
                        const float mu = sep > 0.f ? fabsf(dz) / sep : 0.f;
                        if (mu >= a.mu_max) continue;
                        sub = (int)(mu * a.inv_dmu);
                        if (sub >= a.nsub) continue;
                    }
                    const double ww = (double)iw[i] * wj;
                    if (MODE == 0 && r2 >= top2) {
                        top.add(same, ww);
                        continue;
                    }
                    int b = a.nbins - 1;
                    while (r2 < e2[b]) b--;
                    h.add(b * a.nsub + sub, same, ww);
                }
            }
            i0 += ni;
        }
    }
    if (cur >= 0) {
        if (MODE == 0) top.fold(h, a.nbins - 1);
        h.flush(out, cur);
        nflush++;
    }
    if (tid == 0 && n_eval) atomicAdd(evaluated, n_eval);
    if (tid == 0 && nflush) atomicAdd(out.flushes, (unsigned long long)nflush);
}

// the walk of pair_count_los (no separation sums) with the two histograms of the current label
template <int MODE, bool WEIGHTED>
__global__ __launch_bounds__(PB) void pair_count_los_jk(LosArgs a, const int *__restrict__ lab1, const int *__restrict__ lab2, JkOut out,
                                                        int ncell, unsigned long long *__restrict__ evaluated) {
    __shared__ float ix[PB], iy[PB], iz[PB], iw[PB];
    __shared__ int il[PB];
    __shared__ double e2[64];
    __shared__ int64_t nb_j0[27];
    __shared__ int nb_pre[28];               // exclusive prefix of the neighbour cells' populations
    extern __shared__ __align__(8) double jk_lds[];   // [nh sums first | nh sums both] nh counts first | nh counts both
    const int tid = threadIdx.x;
    const int nh = a.nbins * a.nsub;
    const JkHist<WEIGHTED> h(jk_lds, nh);
    h.clear();
    if (tid <= a.nbins) e2[tid] = a.edges2[tid];
    __syncthreads();
    const double lo2 = e2[0], hi2 = e2[a.nbins], top2 = e2[a.nbins - 1];
    const int ncx = a.nc[0], ncy = a.nc[1], ncz = a.nc[2];
    JkTop<WEIGHTED> top;
    unsigned long long n_eval = 0;
    unsigned int nflush = 0;
    int cur = -1;                            // the label the histograms hold (none yet)
    int c_lo, c_hi;
    jk_cell_range(a.start1, ncell, c_lo, c_hi);
    for (int c1 = c_lo; c1 < c_hi; c1++) {
        const int64_t cbeg = a.start1[c1], cend = a.start1[c1 + 1];
        if (cbeg == cend) continue;
        __syncthreads();   // the previous cell's reads of the neighbour table and of the slice are done
        if (tid < 64) {
            int len = 0;
            int64_t j0 = 0;
            if (tid < 27) {
                const int cz = c1 % ncz, cy = (c1 / ncz) % ncy, cx = c1 / (ncz * ncy);
                const int nx = cx + tid / 9 - 1, ny = cy + (tid / 3) % 3 - 1, nz = cz + tid % 3 - 1;
                if (nx >= 0 && nx < ncx && ny >= 0 && ny < ncy && nz >= 0 && nz < ncz) {   // open grid: nothing wraps
                    const int c2 = (nx * ncy + ny) * ncz + nz;
                    j0 = a.start2[c2];
                    len = (int)(a.start2[c2 + 1] - j0);
                }
            }
            int incl = len;
#pragma unroll
            for (int d = 1; d < 32; d <<= 1) {
                const int v = __shfl_up(incl, d, 64);
                if (tid >= d) incl += v;
            }
            if (tid < 27) nb_j0[tid] = j0, nb_pre[tid] = incl - len;
            if (tid == 26) nb_pre[27] = incl;
        }
        __syncthreads();
        const int M = nb_pre[27];
        for (int64_t i0 = cbeg; i0 < cend;) {
            const int cap = (int)min((int64_t)PB, cend - i0);
            if (i0 > cbeg) __syncthreads();   // the previous slice's reads are done
            if (tid < cap) {                  // the points behind the run's end are loaded again by the next slice
                ix[tid] = a.x1[i0 + tid], iy[tid] = a.y1[i0 + tid], iz[tid] = a.z1[i0 + tid];
                iw[tid] = WEIGHTED && a.w1 ? a.w1[i0 + tid] : 1.0f;
                il[tid] = lab1[i0 + tid];
            }
            __syncthreads();
            const int L = il[0], ni = jk_run_length(il, cap);
            if (L != cur) {                   // uniform: another region from here on
                if (cur >= 0) {
                    if (MODE == 0) top.fold(h, a.nbins - 1);
                    h.flush(out, cur);
                    nflush++;
                }
                cur = L;
            }
            for (int base = 0; base < M; base += PB) {
                n_eval += (unsigned long long)ni * (unsigned long long)min(PB, M - base);
                const int v = base + tid;
                if (v >= M) continue;
                int sg = 0;
                while (nb_pre[sg + 1] <= v) sg++;        // v < nb_pre[27]: ends at a non-empty cell
                const int64_t jj = nb_j0[sg] + (v - nb_pre[sg]);
                const float xj = a.x2[jj], yj = a.y2[jj], zj = a.z2[jj];
                const double wj = WEIGHTED && a.w2 ? (double)a.w2[jj] : 1.0;
                const bool same = lab2[jj] == L;
                for (int i = 0; i < ni; i++) {
                    const float dxf = ix[i] - xj, dyf = iy[i] - yj, dzf = iz[i] - zj;
                    const float s2f = dxf * dxf + dyf * dyf + dzf * dzf;
                    if (s2f > a.pre_hi || s2f < a.pre_lo) continue;
                    if (a.autocorr && jj == i0 + i) continue;   // the same point (the two sorted sets are one array)
                    const double dx = (double)dxf, dy = (double)dyf, dz = (double)dzf;
                    const double s2 = dx * dx + dy * dy + dz * dz;
                    double q = s2, pi2 = 0.0;
                    int sub = 0;
                    if (MODE == 0) {
                        if (!(q >= lo2 && q < hi2)) continue;
                    } else {
                        if (MODE == 2 && !(q >= lo2 && q < hi2)) continue;
                        const double lx = (double)(ix[i] + xj), ly = (double)(iy[i] + yj), lz = (double)(iz[i] + zj);
                        const double l2 = lx * lx + ly * ly + lz * lz;
                        if (l2 == 0.0) continue;                // no line of sight
                        const double t = dx * lx + dy * ly + dz * lz;
                        pi2 = t * t / l2;
                        if (MODE == 1) {
                            const double pi = sqrt(pi2);
                            if (!(pi < a.pimax)) continue;
                            const double rp2 = s2 - pi2;
                            q = rp2 > 0.0 ? rp2 : 0.0;
                            if (!(q >= lo2 && q < hi2)) continue;
                            sub = (int)(pi / a.dpi);
                        } else {
                            const double mu = s2 > 0.0 ? sqrt(pi2 / s2) : 0.0;
                            if (!(mu < a.mu_max)) continue;
                            sub = (int)(mu * a.inv_dmu);
                        }
                        if (sub >= a.nsub) continue;
                    }
                    const double ww = WEIGHTED ? (double)iw[i] * wj : 0.0;
                    if (MODE == 0 && q >= top2) {
                        top.add(same, ww);
                        continue;
                    }
                    int b = a.nbins - 1;
                    while (q < e2[b]) b--;
                    h.add(b * a.nsub + sub, same, ww);
                }
            }
            i0 += ni;
        }
    }
    if (cur >= 0) {
        if (MODE == 0) top.fold(h, a.nbins - 1);
        h.flush(out, cur);
        nflush++;
    }
    if (tid == 0 && n_eval) atomicAdd(evaluated, n_eval);
    if (tid == 0 && nflush) atomicAdd(out.flushes, (unsigned long long)nflush);
}

// smallest and largest label of a set: range[0] = min, range[1] = max (the host refuses a call whose labels leave [0, nreg)
// before anything is sorted or counted)
__global__ void jk_label_range(const int *__restrict__ labels, int64_t n, int *__restrict__ range) {
    int mn = 0x7fffffff, mx = (int)0x80000000;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int l = labels[i];
        mn = min(mn, l), mx = max(mx, l);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mn = min(mn, __shfl_xor(mn, off, 64)), mx = max(mx, __shfl_xor(mx, off, 64));
    if ((threadIdx.x & 63) == 0 && mn <= mx) atomicMin(&range[0], mn), atomicMax(&range[1], mx);
}

// the sort key of a point: its cell above its label (the label masked to its bits: it was range-checked before)
template <typename K, typename Grid>
__global__ void jk_cell_keys(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z,
                             const int *__restrict__ labels, int64_t n, Grid g, int lab_bits, K *__restrict__ keys,
                             unsigned int *__restrict__ idx) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v[3] = {x[i], y[i], z[i]};
        keys[i] = ((K)g.cell(v) << lab_bits) | (K)((unsigned int)labels[i] & ((1u << lab_bits) - 1u));
        idx[i] = (unsigned int)i;
    }
}
// behind the sort: points, weights and labels in (cell, label, input) order
__global__ void jk_gather(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z,
                          const float *__restrict__ w, const int *__restrict__ labels, int64_t n, const unsigned int *__restrict__ idx,
                          float *__restrict__ sx, float *__restrict__ sy, float *__restrict__ sz, float *__restrict__ sw,
                          int *__restrict__ sl) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        const unsigned int i = idx[s];
        sx[s] = x[i], sy[s] = y[i], sz[s] = z[i], sl[s] = labels[i];
        if (w) sw[s] = w[i];
    }
}
template <typename K>
__global__ void jk_cell_starts(const K *__restrict__ keys, int64_t n, int64_t ncell, int lab_bits, int64_t *__restrict__ start) {
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c <= ncell; c += (int64_t)gridDim.x * blockDim.x) {
        int64_t lo = 0, hi = n;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)(keys[mid] >> lab_bits) < c) lo = mid + 1;
            else hi = mid;
        }
        start[c] = lo;
    }
}

// labels of an nx x ny x nz split of the periodic box, from the float32 coordinate the counter sees, wrapped like the cell grid
template <typename T>
__global__ void jk_box_labels(const T *__restrict__ x, const T *__restrict__ y, const T *__restrict__ z, int64_t n, float inv_box,
                              int nx, int ny, int nz, int *__restrict__ labels) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int cx = max(cell_coord((float)x[i], nx, inv_box), 0), cy = max(cell_coord((float)y[i], ny, inv_box), 0),
                  cz = max(cell_coord((float)z[i], nz, inv_box), 0);
        labels[i] = (cx * ny + cy) * nz + cz;
    }
}

struct JkWork {
    DevBuf labs[2], keys[2], sorted_labels[2], range;
    int *sl[2];
} g_jk;

int bits_for(int64_t n) {   // bits that hold 0 .. n - 1
    int b = 1;
    while (((int64_t)1 << b) < n) b++;
    return b;
}

template <typename K, typename Grid>
int jk_sort_keys(const Columns &c, const int *labels, int64_t n, const Grid &g, int64_t ncell, int lab_bits, int end_bit, SortedSet &s,
                 DevBuf &keybuf, int nblk) {
    ABACUS_TRY(keybuf.reserve(2 * (size_t)n * sizeof(K)));
    K *keys = keybuf.as<K>(), *keys2 = keys + n;
    ABACUS_LAUNCH("pair_jk_keys", (jk_cell_keys<K, Grid>), dim3(nblk), dim3(256), 0, c.x[0], c.x[1], c.x[2], labels, n, g, lab_bits, keys,
                  s.idx.as<unsigned int>());
    size_t tmp_bytes = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, keys, keys2, s.idx.as<unsigned int>(), s.idx2.as<unsigned int>(), (int)n, 0,
                                             end_bit, stream());
    ABACUS_TRY(s.tmp.reserve(tmp_bytes));
    prof_begin("pair_jk_sort");
    const hipError_t sorted = hipcub::DeviceRadixSort::SortPairs(s.tmp.p, tmp_bytes, keys, keys2, s.idx.as<unsigned int>(),
                                                                 s.idx2.as<unsigned int>(), (int)n, 0, end_bit, stream());
    prof_end("pair_jk_sort");
    if (sorted != hipSuccess) return fail("abacus_paircount_jk: radix sort failed");
    const int cblk = (int)std::min<int64_t>(ceil_div(ncell + 1, 256), 8192);
    ABACUS_LAUNCH("pair_jk_starts", jk_cell_starts<K>, dim3(cblk), dim3(256), 0, keys2, n, ncell, lab_bits, s.start.as<int64_t>());
    return 0;
}

// The set in (cell, label) order on either grid: s.sx | sy | sz, s.start, s.sw with weights, and g_jk.sl[k].  One stable radix
// sort for every size (the counting sort of sort_into_cells leaves the order inside a cell to the run); n > 0
template <typename Grid>
int sort_into_cells_jk(const Columns &c, const int *labels, int64_t n, const Grid &g, int64_t ncell, int nreg, int k) {
    SortedSet &s = g_work.S[k];
    const size_t n1 = (size_t)n;
    s.n = n;
    ABACUS_TRY(s.sorted.reserve(3 * n1 * 4));
    ABACUS_TRY(s.start.reserve((size_t)(ncell + 1) * 8));
    ABACUS_TRY(s.idx.reserve(n1 * 4));
    ABACUS_TRY(s.idx2.reserve(n1 * 4));
    ABACUS_TRY(g_jk.sorted_labels[k].reserve(n1 * 4));
    s.sx = s.sorted.as<float>(), s.sy = s.sx + n1, s.sz = s.sy + n1, s.sw = nullptr;
    if (c.w) {
        ABACUS_TRY(s.wsorted.reserve(n1 * 4));
        s.sw = s.wsorted.as<float>();
    }
    g_jk.sl[k] = g_jk.sorted_labels[k].as<int>();
    const int nblk = (int)std::min<int64_t>(ceil_div(n, 256), 2048);
    const int lab_bits = bits_for(nreg), end_bit = lab_bits + bits_for(ncell);
    if (end_bit <= 32) ABACUS_TRY((jk_sort_keys<unsigned int, Grid>(c, labels, n, g, ncell, lab_bits, end_bit, s, g_jk.keys[k], nblk)));
    else ABACUS_TRY((jk_sort_keys<unsigned long long, Grid>(c, labels, n, g, ncell, lab_bits, end_bit, s, g_jk.keys[k], nblk)));
    ABACUS_LAUNCH("pair_jk_fill", jk_gather, dim3(nblk), dim3(256), 0, c.x[0], c.x[1], c.x[2], c.w, labels, n, s.idx2.as<unsigned int>(), s.sx,
                  s.sy, s.sz, s.sw, g_jk.sl[k]);
    return 0;
}

struct JkHostOut {
    uint64_t *nfirst, *nboth;
    double *wfirst, *wboth;
};

// what both drivers check before the device is touched
int jk_check(const char *who, int nreg, int nbins, int nsub, int autocorr, const void *labels1, const void *labels2, int64_t n1, int64_t n2,
             const JkHostOut &o, bool need_sums) {
    if (nreg < 1 || nreg > JK_MAX_REG) return fail("%s: nreg = %d must lie in [1, %d]", who, nreg, JK_MAX_REG);
    if (nsub > JK_MAX_HIST) return fail("%s: %d pi / mu bins exceed the LDS histogram", who, nsub);
    if ((int64_t)nreg * nbins * nsub > JK_MAX_OUT) return fail("%s: nreg * nbins * sub-bins = %lld exceeds 2^24 output entries", who, (long long)nreg * nbins * nsub);
    if (!o.nfirst || !o.nboth) return fail("%s: npairs_first / npairs_both is NULL", who);
    if ((o.wfirst == nullptr) != (o.wboth == nullptr)) return fail("%s: wsum_first and wsum_both go together", who);
    if (need_sums && !o.wfirst) return fail("%s: wsum_first / wsum_both is NULL", who);
    if (autocorr && labels2) return fail("%s: labels2 given for an autocorrelation (x2 is NULL)", who);
    if (n1 > 0 && !labels1) return fail("%s: labels1 is NULL", who);
    if (!autocorr && n2 > 0 && !labels2) return fail("%s: labels2 is NULL", who);
    return 0;
}

// labels in HBM (host labels are uploaded) and range-checked by a device reduction: nothing is sorted or counted with a label
// outside [0, nreg)
int jk_stage_labels(const char *who, const int32_t *const src[2], const int64_t ns[2], int nsets, int where, int nreg, const int *dl[2]) {
    ABACUS_TRY(g_jk.range.reserve(8));
    const int init[2] = {0x7fffffff, (int)0x80000000};
    HIP_TRY(hipMemcpyAsync(g_jk.range.p, init, 8, hipMemcpyHostToDevice, stream()));
    for (int k = 0; k < nsets; k++) {
        dl[k] = src[k];
        if (where == 0) {
            ABACUS_TRY(g_jk.labs[k].reserve((size_t)ns[k] * 4));
            HIP_TRY(hipMemcpyAsync(g_jk.labs[k].p, src[k], (size_t)ns[k] * 4, hipMemcpyHostToDevice, stream()));
            dl[k] = g_jk.labs[k].as<int>();
        }
        ABACUS_LAUNCH("pair_jk_label_range", jk_label_range, dim3((unsigned int)std::min<int64_t>(ceil_div(ns[k], 256), 1024)), dim3(256), 0,
                      dl[k], ns[k], g_jk.range.as<int>());
    }
    int range[2];
    HIP_TRY(hipMemcpyAsync(range, g_jk.range.p, 8, hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipStreamSynchronize(stream()));
    if (range[0] < 0 || range[1] >= nreg) return fail("%s: labels span [%d, %d], outside [0, %d)", who, range[0], range[1], nreg);
    return 0;
}

// the four output arrays in g_work.out, zeroed: [nreg][ntot] each
int jk_device_outputs(int nreg, size_t ntot, bool sums, JkOut &d, unsigned long long *flushes) {
    const size_t cnt = (size_t)nreg * ntot, bytes = (sums ? 4 : 2) * cnt * 8;
    ABACUS_TRY(g_work.out.reserve(bytes));
    HIP_TRY(hipMemsetAsync(g_work.out.p, 0, bytes, stream()));
    d.nfirst = g_work.out.as<unsigned long long>(), d.nboth = d.nfirst + cnt;
    d.wfirst = sums ? reinterpret_cast<double *>(d.nboth + cnt) : nullptr, d.wboth = sums ? d.wfirst + cnt : nullptr;
    d.stride = ntot, d.flushes = flushes;
    return 0;
}
JkOut jk_at(const JkOut &d, size_t o) {
    JkOut r = d;
    r.nfirst += o, r.nboth += o;
    if (r.wfirst) r.wfirst += o, r.wboth += o;
    return r;
}
int jk_fetch(const JkHostOut &h, const JkOut &d, size_t cnt) {
    HIP_TRY(hipMemcpyAsync(h.nfirst, d.nfirst, cnt * 8, hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipMemcpyAsync(h.nboth, d.nboth, cnt * 8, hipMemcpyDeviceToHost, stream()));
    if (h.wfirst) {
        HIP_TRY(hipMemcpyAsync(h.wfirst, d.wfirst, cnt * 8, hipMemcpyDeviceToHost, stream()));
        HIP_TRY(hipMemcpyAsync(h.wboth, d.wboth, cnt * 8, hipMemcpyDeviceToHost, stream()));
    }
    return 0;
}
void jk_zero(const JkHostOut &h, size_t cnt) {
    memset(h.nfirst, 0, cnt * 8), memset(h.nboth, 0, cnt * 8);
    if (h.wfirst) memset(h.wfirst, 0, cnt * 8), memset(h.wboth, 0, cnt * 8);
}

// The jackknife launches of a run, like those of the plain walks above; out: the run's columns of the [nreg][ntot] block.
// They take fewer workgroups on request (pairs_jk_grid, tests: many cells per workgroup) and report how many they took.
void cap_jk_grid(dim3 &grid) {
    if (option("pairs_jk_grid") > 0) grid.x = std::min<unsigned int>(grid.x, (unsigned int)option("pairs_jk_grid"));
}

template int sort_into_cells_jk<CellGrid>(const Columns &, const int *, int64_t, const CellGrid &, int64_t, int, int);

int launch_jk(const PairArgs &a, const WeightArgs &wa, const int *lab1, const int *lab2, const JkOut &out, const Flags &fl, int64_t ncell,
              int &workgroups) {
    const size_t hist_bytes = (size_t)a.nbins * a.nsub * 24;   // <= JK_MAX_HIST * 24 = 48 KiB beside 6 KiB of static LDS
    return with_mode(a.mode, [&](auto M) -> int {
        const auto kernel = pair_count_jk<decltype(M)::value>;
        dim3 grid;
        ABACUS_TRY(resident_grid(kernel, PB, hist_bytes, ncell, grid));
        cap_jk_grid(grid);
        ABACUS_LAUNCH("pair_count_jk", kernel, grid, dim3(PB), hist_bytes, a, wa, lab1, lab2, out, (int)ncell, fl.evaluated);
        workgroups = (int)grid.x;
        return 0;
    });
}

template int sort_into_cells_jk<OpenGrid>(const Columns &, const int *, int64_t, const OpenGrid &, int64_t, int, int);

int launch_los_jk(int mode, const LosArgs &a, bool weighted, const int *lab1, const int *lab2, const JkOut &out, const Flags &fl,
                  int64_t ncell, int &workgroups) {
    const size_t hist_bytes = (size_t)a.nbins * a.nsub * (weighted ? 24 : 8);
    return with_mode(mode, [&](auto M) {
        return with_flag(weighted, [&](auto WT) -> int {
            const auto kernel = pair_count_los_jk<decltype(M)::value, decltype(WT)::value>;
            dim3 grid;
            ABACUS_TRY(resident_grid(kernel, PB, hist_bytes, ncell, grid));
            cap_jk_grid(grid);
            ABACUS_LAUNCH("pair_count_los_jk", kernel, grid, dim3(PB), hist_bytes, a, lab1, lab2, out, (int)ncell, fl.evaluated);
            workgroups = (int)grid.x;
            return 0;
        });
    });
}

// ------------------------------------------------------------------------------------------------ counts in spheres ----
// Neighbour counts around query points (abacus_spherecount[_dev]): for every query the number of data points inside each of nr
// radii - the primitive under the void probability function, the kNN-CDFs and counts-in-cells.  No reference code and no
// Corrfunc run stands behind it; the NumPy statement tests/spheres_statement.py is the judge, and its column sums are the
// cumulative counts of the pair counter.
//   per (query, data) pair, float32, the expressions of pair_count_w: d = q - p per component through min_image, r2 = dx dx +
//   dy dy + dz dz left to right (cylinders: r2 = dx dx + dy dy, and the pair needs |dz| < pimax); the point is inside radius j
//   iff r2 < e2[j], e2[j] = r_j r_j as a float32 product - strict, so N(<r_j) is the cumulative sum of the [lo, hi) bins over
//   (0, r_1 .. r_nr).  Queries that ARE the data (qx == NULL) do not count themselves, by identity: a coincident twin counts.
//   out: hist[j][k] = queries with exactly k points inside r_j (k < kmax), hist[j][kmax] = those with kmax or more; and, when
//   asked for, counts[query][j] in the caller's query order.
// Mapping: the walk of pair_count_w with another reduction.  A persistent workgroup takes a query cell; the 27 (or fewer)
// neighbour cells are ONE virtual list of which every lane holds one data point in registers; the queries of the cell are an
// LDS slice read by broadcast (one 16-byte read: x, y, z and the caller's index).  Membership is reduced over the WAVE, not per
// pair: the ballot of r2 < e2[j] is the wave's contribution to N(<r_j), already cumulative, so the radii are walked from the
// largest down and the walk ends at the first empty ballot (logarithmic radii: the sphere's volume halves per step, a round of
// 64 candidates is empty after some five).  Lane j keeps the population count of radius j, and lanes 0 .. nr - 1
// add the round's row to cnt[query][0 .. nr) in LDS with one conflict-free instruction.  No atomics per pair, and a workgroup is
// busy when a cell holds a handful of queries and hundreds of candidates - 10^6 random centres in 10^7 galaxies, the usual
// regime.  (The transposed mapping - a lane per query, data tiles broadcast from LDS, private counters - needs no ballots and
// wins when the queries are as dense as the data; it is not built: with a few queries per cell it leaves most lanes idle.)
// After the walk of a slice hist[j][min(cnt, kmax)] is bumped in an LDS histogram (flushed once per workgroup, 64-bit global
// atomics) and the row goes to counts[caller's index].  That index rides through both sort paths in the weight lane of the
// existing sort kernels, as the bit pattern of a float32 that only moves touch.
struct SphereArgs {
    CellGrid g;
    int nr, kmax, autocorr;
    float half, pimax;
    const float *e2;               // nr squared radii
    const float *qx, *qy, *qz;     // the queries in cell order ...
    const unsigned int *qid;       // ... and their indices in the caller's order (NULL: counts not asked for)
    const float *px, *py, *pz;     // the data in cell order (the queries' arrays when the queries are the data)
    const int64_t *qstart, *pstart;
    unsigned long long *hist;      // [nr][kmax + 1]
    unsigned int *counts;          // [nq][nr], or NULL
    unsigned int nq;               // rows of counts
};

// (a template, like sphere_count: the code object lists such kernels where they are first asked for - behind the kernels that were
// here before, which come out of the compiler as they did; only the two jk_box_labels kernels of the file's last entry follow,
// with their local labels renumbered: profiles/spheres/README.md)
template <typename T>
__global__ void sphere_iota(T *__restrict__ idx, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) idx[i] = (T)i;
}

template <bool CYL>
__global__ __launch_bounds__(PB) void sphere_count(SphereArgs a, int ncell, unsigned long long *__restrict__ evaluated) {
    __shared__ float4 qp[PB];                // the slice: x, y, z, the caller's index as a bit pattern
    __shared__ int64_t nb_j0[27];
    __shared__ int nb_pre[28];               // exclusive prefix of the neighbour cells' populations
    extern __shared__ unsigned int sph_lds[];   // nr (kmax + 1) histogram entries | PB rows of nr counts
    const int tid = threadIdx.x, lane = tid & 63;
    const int nr = a.nr, kw = a.kmax + 1, nh = nr * kw;
    unsigned int *hist = sph_lds, *cnt = sph_lds + nh;
    for (int q = tid; q < nh + PB * nr; q += PB) sph_lds[q] = 0u;
    const float e2l = lane < nr ? a.e2[lane] : 0.f;   // lane j holds e2[j]: read back as a scalar (v_readlane), no memory in the loop
    const int rx = a.g.ncx >= 3 ? 1 : 0, ry = a.g.ncy >= 3 ? 1 : 0, rz = a.g.ncz >= 3 ? 1 : 0;
    const int wy = 2 * ry + 1, wz = 2 * rz + 1, nnb = (2 * rx + 1) * wy * wz;
    unsigned long long n_eval = 0;
    for (int c1 = blockIdx.x; c1 < ncell; c1 += gridDim.x) {
        const int64_t cbeg = a.qstart[c1], cend = a.qstart[c1 + 1];
        if (cbeg == cend) continue;
        __syncthreads();   // the previous cell's reads of the neighbour table and of the slice are done, its count rows are zero again
        if (tid < 64) {
            int len = 0;
            int64_t j0 = 0;
            if (tid < nnb) {
                const int cz = c1 % a.g.ncz, cy = (c1 / a.g.ncz) % a.g.ncy, cx = c1 / (a.g.ncz * a.g.ncy);
                int nx = cx + tid / (wy * wz) - rx, ny = cy + (tid / wz) % wy - ry, nz = cz + tid % wz - rz;
                nx = nx < 0 ? nx + a.g.ncx : (nx >= a.g.ncx ? nx - a.g.ncx : nx);
                ny = ny < 0 ? ny + a.g.ncy : (ny >= a.g.ncy ? ny - a.g.ncy : ny);
                nz = nz < 0 ? nz + a.g.ncz : (nz >= a.g.ncz ? nz - a.g.ncz : nz);
                const int c2 = (nx * a.g.ncy + ny) * a.g.ncz + nz;
                j0 = a.pstart[c2];
                len = (int)(a.pstart[c2 + 1] - j0);
            }
            int incl = len;
#pragma unroll
            for (int d = 1; d < 32; d <<= 1) {
                const int v = __shfl_up(incl, d, 64);
                if (tid >= d) incl += v;
            }
            if (tid < nnb) nb_j0[tid] = j0, nb_pre[tid] = incl - len;
            if (tid == nnb - 1) nb_pre[nnb] = incl;
        }
        __syncthreads();
        const int M = nb_pre[nnb];
        for (int64_t i0 = cbeg; i0 < cend; i0 += PB) {
            const int ni = (int)min((int64_t)PB, cend - i0);
            if (i0 > cbeg) __syncthreads();   // the previous slice's rows are read and zero again
            if (tid < ni) qp[tid] = make_float4(a.qx[i0 + tid], a.qy[i0 + tid], a.qz[i0 + tid], a.qid ? __uint_as_float(a.qid[i0 + tid]) : 0.f);
            __syncthreads();
            for (int base = 0; base < M; base += PB) {
                n_eval += (unsigned long long)ni * (unsigned long long)min(PB, M - base);
                if (base + (tid & ~63) >= M) continue;   // per wave: no candidate left for it in this round
                // every lane of the wave stays in the loop below (the ballots are over the whole wave); one without a point never matches
                const int v = base + tid;
                const bool have = v < M;
                float xj = 0.f, yj = 0.f, zj = 0.f;
                int self = -1;                           // the slice index of this very point (the two sorted sets are one array)
                if (have) {
                    int sg = 0;
                    while (nb_pre[sg + 1] <= v) sg++;    // v < nb_pre[nnb]: ends at a non-empty cell
                    const int64_t jj = nb_j0[sg] + (v - nb_pre[sg]);
                    xj = a.px[jj], yj = a.py[jj], zj = a.pz[jj];
                    if (a.autocorr && jj >= i0 && jj < i0 + ni) self = (int)(jj - i0);
                }
                for (int i = 0; i < ni; i++) {
                    const float4 q = qp[i];
                    // min_image, branch-free: its single addition of -+L, or of 0 (which leaves d, and -0 as +0: the same square)
                    float dx = q.x - xj, dy = q.y - yj, dz = q.z - zj;
                    dx += dx > a.half ? -a.g.box : (dx < -a.half ? a.g.box : 0.f);
                    dy += dy > a.half ? -a.g.box : (dy < -a.half ? a.g.box : 0.f);
                    dz += dz > a.half ? -a.g.box : (dz < -a.half ? a.g.box : 0.f);
                    bool in = have && i != self;
                    float r2;
                    if (CYL) {
                        r2 = dx * dx + dy * dy;
                        in = in && fabsf(dz) < a.pimax;
                    } else {
                        r2 = dx * dx + dy * dy + dz * dz;
                    }
                    if (!in) r2 = __builtin_huge_valf();    // below no radius
                    int mine = 0;                        // lane j: the wave's points inside radius j of query i
                    for (int j = nr - 1; j >= 0; j--) {
                        const float ej = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e2l), j));
                        const unsigned long long m = __builtin_amdgcn_ballot_w64(r2 < ej);
                        if (!m) break;                   // none inside r_j: none inside a smaller radius
                        mine = lane == j ? __popcll(m) : mine;
                    }
                    if (mine) atomicAdd(&cnt[i * nr + lane], (unsigned int)mine);
                }
            }
            __syncthreads();
            // the slice's rows: into the histogram, to the caller's row, and zero again
            for (int p = tid; p < ni * nr; p += PB) {
                const int i = p / nr, j = p - i * nr;
                const unsigned int c = cnt[p];
                cnt[p] = 0u;
                atomicAdd(&hist[j * kw + (int)min(c, (unsigned int)a.kmax)], 1u);
                const unsigned int row = __float_as_uint(qp[i].w);
                if (a.counts && row < a.nq) a.counts[(size_t)row * nr + j] = c;   // (row < nq always: the guard keeps a store inside the array whatever a sort did)
            }
        }
    }
    if (tid == 0 && n_eval) atomicAdd(evaluated, n_eval);
    __syncthreads();
    for (int q = tid; q < nh; q += PB)
        if (hist[q]) atomicAdd(&a.hist[q], (unsigned long long)hist[q]);
}

int launch_spheres(const SphereArgs &a, bool cyl, const Flags &fl, int64_t ncell) {
    const size_t lds = ((size_t)a.nr * (a.kmax + 1) + (size_t)PB * a.nr) * sizeof(unsigned int);   // <= 32 + 32 KiB beside 4.4 KiB static
    return with_flag(cyl, [&](auto CYL) -> int {
        const auto kernel = sphere_count<decltype(CYL)::value>;
        if (lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        dim3 grid;
        ABACUS_TRY(resident_grid(kernel, PB, lds, ncell, grid));
        ABACUS_LAUNCH("sphere_count", kernel, grid, dim3(PB), lds, a, (int)ncell, fl.evaluated);
        return 0;
    });
}

// ------------------------------------------------------------------------------------------------ the drivers ----
// A call as an entry point hands it on.  count_box (periodic) and count_los (open grid) serve the twelve entries; with a
// JkSpec they are the jackknife counters, without one the plain ones.  Inside a run they part only for the sort (labels ride
// along or not), the launch, and the device outputs (a block per run, or one [nreg][ntot] block of which a run takes columns).
struct PointSet {
    const void *x[3];
    const float *w;   // NULL: unit weights
    int64_t n;
    const void *v[3];   // velocity columns of a velocity call (PairCall::vel), in the dtype of x
};
struct Binning {
    int mode;
    const float *bins;
    int nbins;
    float pimax;
    int npibins;
    float mu_max;
    int nmubins;
    int nsub() const { return mode == 0 ? 1 : (mode == 1 ? npibins : nmubins); }
};
struct JkSpec {
    const int32_t *labels[2];
    int nreg;
    JkHostOut out;
};
struct PairCall {
    const char *who;     // the entry point that was called, for its messages
    PointSet set[2];     // set[1].x[0] == NULL: autocorrelation
    int where;           // 0: host float32 arrays (and host weights, labels); 1: device float32; 2: device float64; < 0: neither
    Binning bin;
    Outputs out;         // of a plain call
    const JkSpec *jk;    // NULL: a plain call
    bool vel = false;    // abacus_pairvel: the sets carry velocities, out.vsum takes their sums (a plain, weighted call otherwise)
    int autocorr() const { return set[1].x[0] == nullptr; }
    bool empty() const { return set[0].n == 0 || (!autocorr() && set[1].n == 0); }
};
int where_of(int pos_dtype) { return pos_dtype == ABACUS_F32 ? 1 : (pos_dtype == ABACUS_F64 ? 2 : -1); }

// Validation, before the device is touched.  check_box and check_los hold the rules of their family; both start with
// check_sets_and_bins and end the output rules with check_outputs.
int check_sets_and_bins(const PairCall &c, bool other_null) {
    const char *who = c.who;
    const Binning &b = c.bin;
    const PointSet &s1 = c.set[0], &s2 = c.set[1];
    if (c.where < 0) return fail("%s: pos_dtype must be ABACUS_F32 or ABACUS_F64", who);
    if (b.mode < 0 || b.mode > 2) return fail("%s: unknown mode %d", who, b.mode);
    if (!s1.x[0] || !s1.x[1] || !s1.x[2] || !b.bins || other_null || (!c.jk && !c.out.npairs)) return fail("%s: null argument", who);
    if (b.nbins < 1) return fail("%s: nbins must be at least 1", who);
    if (!c.autocorr() && (!s2.x[1] || !s2.x[2])) return fail("%s: null argument (y2 / z2)", who);
    if (c.autocorr() && s2.w) return fail("%s: w2 given for an autocorrelation (x2 is NULL)", who);
    if (s1.n < 0 || s2.n < 0 || s1.n >= ((int64_t)1 << 31) || s2.n >= ((int64_t)1 << 31)) return fail("%s: point counts must lie in [0, 2^31)", who);
    for (int k = 0; k < b.nbins; k++)
        if (!(b.bins[k + 1] > b.bins[k])) return fail("%s: bin edges must increase", who);
    return 0;
}
int check_outputs(const PairCall &c, int plain_hist, bool need_sums) {
    const int nsub = c.bin.nsub();
    if (!c.jk) return nsub > plain_hist ? fail("%s: %d pi / mu bins exceed the LDS histogram", c.who, nsub) : 0;
    return jk_check(c.who, c.jk->nreg, c.bin.nbins, nsub, c.autocorr(), c.jk->labels[0], c.jk->labels[1], c.set[0].n, c.set[1].n, c.jk->out,
                    need_sums);
}
int check_box(const PairCall &c, float boxsize, bool weighted) {
    const Binning &b = c.bin;
    ABACUS_TRY(check_sets_and_bins(c, false));
    if (!(boxsize > 0)) return fail("%s: boxsize must be positive", c.who);
    if (b.nsub() < 1) return fail("%s: need at least one pi / mu bin", c.who);
    ABACUS_TRY(check_outputs(c, c.vel ? V_MAX_HIST : (weighted ? W_MAX_HIST : MAX_HIST), true));
    if (!c.jk && weighted && !c.out.wsum) return fail("%s: wsum is NULL", c.who);
    if (c.vel) {
        const PointSet &s1 = c.set[0], &s2 = c.set[1];
        if (!s1.v[0] || !s1.v[1] || !s1.v[2]) return fail("%s: null velocity column (set 1)", c.who);
        if (!c.autocorr() && !s2.v[0] && !s2.v[1] && !s2.v[2]) return fail("%s: velocities given for set 1 of a cross count but not for set 2", c.who);
        if (!c.autocorr() && (!s2.v[0] || !s2.v[1] || !s2.v[2])) return fail("%s: null velocity column (set 2)", c.who);
        if (!c.out.vsum) return fail("%s: vsum is NULL", c.who);
    }
    // the edges increase: the last one is the reach of every run
    if (b.bins[b.nbins] > 0.5f * boxsize || (b.mode == 1 && b.pimax > 0.5f * boxsize))
        return fail("%s: maximum separation exceeds half the box (minimum image not unique)", c.who);
    return 0;
}
int check_los(const PairCall &c, const double *origin) {
    const Binning &b = c.bin;
    ABACUS_TRY(check_sets_and_bins(c, origin == nullptr));
    if (!(b.bins[0] >= 0.f)) return fail("%s: bin edges must not be negative", c.who);
    if (b.mode == 1 && (!(b.pimax > 0.f) || b.npibins < 1)) return fail("%s: pimax must be positive, with at least one pi bin", c.who);
    if (b.mode == 2 && (!(b.mu_max > 0.f) || b.nmubins < 1)) return fail("%s: mu_max must be positive, with at least one mu bin", c.who);
    ABACUS_TRY(check_outputs(c, W_MAX_HIST, false));
    for (int d = 0; d < 3; d++)
        if (!std::isfinite(origin[d])) return fail("%s: origin must be finite", c.who);
    return 0;
}

// Bookkeeping of the last call (abacus_paircount_stats, abacus_paircount_los_grid, abacus_paircount_jk_stats): zero when a call
// starts, so what an empty or a refused-on-the-device call leaves is zero in all of them
struct Stats {
    unsigned long long evaluated = 0, flushes = 0;   // candidate pairs (not of the first two generations); jackknife flushes
    int cells[3] = {0, 0, 0};                        // cells in xy, in z, stencil half-width R (0: not pair_count3)
    int los_cells[3] = {0, 0, 0};
    int workgroups = 0;
} g_stats;

// A run's candidate count and, behind it in the block of flags, the flush count of the jackknife kernels (over the call so
// far; 0 from any other kernel) come to the host with the run's synchronise; `sum`: the candidates add up over the runs (light
// cone), else the last run's stand.  workgroups: of a jackknife launch
int record_run(const Flags &fl, bool sum, int ncxy, int ncz, int R, const int *los_nc, int workgroups) {
    unsigned long long ctr[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(ctr, fl.evaluated, 16, hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipStreamSynchronize(stream()));
    g_stats.evaluated = (sum ? g_stats.evaluated : 0) + ctr[0];
    g_stats.flushes = ctr[1];
    g_stats.cells[0] = ncxy, g_stats.cells[1] = ncz, g_stats.cells[2] = R;
    for (int d = 0; d < 3 && los_nc; d++) g_stats.los_cells[d] = los_nc[d];
    g_stats.workgroups = workgroups;
    return 0;
}

// What the periodic kernels read beside the sets; the bin table and the job blocks are pair_count3's and stay off here
void fill_box_args(PairArgs &a, const Binning &b, const CellGrid &g) {
    a.mode = b.mode;
    a.in_box = 1;   // (no kernel reads it: pair_count2 takes the device flag)
    a.g = g;
    a.half = g.box * 0.5f;
    a.pimax = b.pimax;
    a.dpi = b.npibins > 0 ? b.pimax / (float)b.npibins : 1.0f;
    a.mu_max = b.mu_max;
    a.inv_dmu = b.nmubins > 0 ? (float)b.nmubins / b.mu_max : 1.0f;
    a.edges2 = g_work.edges.as<float>();
    a.lut_sh = a.lut_off = a.lut_ncell = 0;
    a.no_blocks = 0;
}

// The periodic grid of a run and its stencil half-width R.  Jackknife and weighted counts walk the 27 cells of the full reach.
// The unweighted kernels take cells of size >= reach / R: R = 2 (125-cell stencil of cells an eighth the volume: 1.7x fewer
// candidate pairs) when the catalogue is dense enough to keep a wave busy with a small cell, else R = 1
int periodic_grid(float boxsize, float reach_xy, float reach_z, bool full_reach, int gen, double nmax, CellGrid &g) {
    auto ncells = [&](float reach, int R, int cap) {
        int nc = (int)floorf(boxsize / reach * (float)R * 0.9999f);   // cell size strictly >= reach / R
        nc = std::min(nc, cap);
        return nc < 3 ? 1 : nc;
    };
    int R = 1;
    if (!full_reach && gen >= 3) {
        const double per_cell = nmax * ((double)reach_xy / boxsize) * ((double)reach_xy / boxsize) * ((double)reach_z / boxsize);
        if (per_cell > 12.0 && ncells(reach_xy, 2, 192) >= 5 && ncells(reach_z, 2, 192) >= 5) R = 2;
    }
    g.box = boxsize;
    g.inv_box = 1.0f / boxsize;
    g.ncx = g.ncy = ncells(reach_xy, R, R == 2 ? 192 : 128);
    g.ncz = ncells(reach_z, R, R == 2 ? 192 : 128);
    // the cap may leave cells larger than reach / R: still correct (a cell >= reach / R is all the stencil needs)
    return R;
}

// pair_vel stands behind every instantiation above, so the kernels before it keep their order in the code object
int launch_vel(const PairArgs &a, const WeightArgs &wa, const VelArgs &va, const Flags &fl, int64_t ncell) {
    const size_t hist_bytes = (size_t)a.nbins * a.nsub * 52;   // <= V_MAX_HIST * 52 = 52 KiB beside 7.6 KiB of static LDS
    return with_mode(a.mode, [&](auto M) {
        return with_flag(a.mode != 0 || !option("pairvel_lds_top"), [&](auto TOP) -> int {   // modes 1, 2 have no such path: one instance
            const auto kernel = pair_vel<decltype(M)::value, decltype(TOP)::value>;
            if (hist_bytes > 48 * 1024)
                HIP_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)hist_bytes));
            dim3 grid;
            ABACUS_TRY(resident_grid(kernel, PB, hist_bytes, ncell, grid));
            ABACUS_LAUNCH("pair_vel", kernel, grid, dim3(PB), hist_bytes, a, wa, va, (int)ncell, fl.evaluated);
            return 0;
        });
    });
}

// The periodic driver.  weighted: the entry takes weights and returns wsum (and rsum unless NULL), by pair_count_w - or, for a
// call with velocities (c.vel), the five velocity sums beside wsum, by pair_vel
int count_box(const PairCall &c, float boxsize, bool weighted) {
    ABACUS_TRY(check_box(c, boxsize, weighted));
    ABACUS_ENTER();
    const Binning &b = c.bin;
    const JkSpec *jk = c.jk;
    const int mode = b.mode, autocorr = c.autocorr(), nsets = autocorr ? 1 : 2, nsub = b.nsub();
    const size_t ntot_all = (size_t)b.nbins * nsub;
    if (jk) jk_zero(jk->out, (size_t)jk->nreg * ntot_all);
    else c.out.zero(ntot_all);
    g_stats = Stats{};
    if (c.empty()) return 0;

    Work &W = g_work;
    const int64_t ns[2] = {c.set[0].n, c.set[1].n};
    const int *dl[2] = {nullptr, nullptr};
    if (jk) ABACUS_TRY(jk_stage_labels(c.who, jk->labels, ns, nsets, c.where, jk->nreg, dl));
    Flags fl;
    ABACUS_TRY(W.flags(fl));
    JkOut jdev = {};
    if (jk) ABACUS_TRY(jk_device_outputs(jk->nreg, ntot_all, true, jdev, fl.evaluated + 1));   // the flush count: behind the candidates
    Columns cols[2];
    for (int k = 0; k < nsets; k++)
        ABACUS_TRY(stage_columns("pair_cast", c.set[k].x, c.set[k].w, c.where, ns[k], nullptr, W.cols[k], W.wts[k], cols[k]));
    Columns vels[2];   // the velocities of a velocity call: staged like the positions (one rounding of float64 columns)
    for (int k = 0; k < nsets && c.vel; k++)
        ABACUS_TRY(stage_columns("pair_cast", c.set[k].v, nullptr, c.where, ns[k], nullptr, W.vcols[k], W.wts[k], vels[k]));
    const int gen = option("pairs_gen") ? option("pairs_gen") : 3;
    // the columns serve every run; a run sorts them into a grid of its own reach and counts
    ABACUS_TRY(for_runs(b.nbins, nsub, jk ? JK_MAX_HIST : (c.vel ? V_MAX_HIST : (weighted ? W_MAX_HIST : MAX_HIST)), [&](int b0, int nb, size_t o) -> int {
        const float *edges = b.bins + b0;
        const float reach_xy = edges[nb], reach_z = mode == 1 ? b.pimax : edges[nb];
        const size_t ntot = (size_t)nb * nsub;
        CellGrid g;
        const int R = periodic_grid(boxsize, reach_xy, reach_z, jk || weighted, gen, (double)std::max(ns[0], autocorr ? ns[0] : ns[1]), g);
        const int64_t ncell = (int64_t)g.ncx * g.ncy * g.ncz;
        // the frame and the outside flag belong to a run's grid; the jackknife kernels keep their flush count over the call
        if (jk) HIP_TRY(hipMemsetAsync(fl.evaluated, 0, 8, stream()));
        else if (b0 > 0) ABACUS_TRY(W.flags(fl));
        for (int k = 0; k < nsets; k++) {
            if (jk) ABACUS_TRY(sort_into_cells_jk(cols[k], dl[k], ns[k], g, ncell, jk->nreg, k));
            else ABACUS_TRY(sort_into_cells(cols[k], ns[k], FramedGrid{g, fl.outside, fl.frame}, ncell, W.S[k], W.scratch, c.vel ? vels[k].x : nullptr));
        }
        std::vector<float> e2;
        ABACUS_TRY(upload_edges(edges, nb, e2));
        Outputs dev = {};
        if (!jk) ABACUS_TRY(device_outputs(ntot, weighted, c.vel, dev));
        PairArgs a;
        WeightArgs wa;
        fill_sets(a, wa, autocorr, nb, nsub, dev);
        fill_box_args(a, b, g);
        int R_used = 0, workgroups = 0;
        if (jk) ABACUS_TRY(launch_jk(a, wa, g_jk.sl[0], g_jk.sl[nsets - 1], jk_at(jdev, o), fl, ncell, workgroups));
        else if (c.vel) {
            const SortedSet &S1 = W.S[0], &T = W.S[nsets - 1];
            ABACUS_TRY(launch_vel(a, wa, VelArgs{{S1.sv[0], S1.sv[1], S1.sv[2]}, {T.sv[0], T.sv[1], T.sv[2]}, dev.vsum}, fl, ncell));
        } else if (weighted) ABACUS_TRY(launch_weighted(a, wa, c.out.rsum != nullptr, fl, ncell));
        else ABACUS_TRY(launch_unweighted(a, gen, R, e2, fl, ncell, R_used));
        if (!jk) ABACUS_TRY(fetch_outputs(c.out.at(o), dev, ntot));
        return record_run(fl, false, g.ncx, g.ncz, R_used, nullptr, workgroups);
    }));
    if (jk) {
        ABACUS_TRY(jk_fetch(jk->out, jdev, (size_t)jk->nreg * ntot_all));
        HIP_TRY(hipStreamSynchronize(stream()));
    }
    return 0;
}

float funkey_host(unsigned int k) {
    const unsigned int u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float v;
    memcpy(&v, &u, 4);
    return v;
}

// The observer-centred frame of a light-cone call: float32 columns of both sets in HBM and their bounding box (one reduction,
// 24 bytes to the host).  They serve every run.
struct LosFrame {
    Columns cols[2];
    double lo[3], extent[3];
};
int los_frame(const PairCall &c, bool weighted, const double *origin, const Flags &fl, LosFrame &f) {
    Work &W = g_work;
    for (int k = 0; k < (c.autocorr() ? 1 : 2); k++) {
        const PointSet &s = c.set[k];
        ABACUS_TRY(stage_columns("pair_los_centre", s.x, weighted ? s.w : nullptr, c.where, s.n, origin, W.cols[k], W.wts[k], f.cols[k]));
        ABACUS_LAUNCH("pair_los_bbox", bbox_minmax, dim3((unsigned int)std::min<int64_t>(ceil_div(s.n, 256), 1024)), dim3(256), 0,
                      f.cols[k].x[0], f.cols[k].x[1], f.cols[k].x[2], s.n, fl.frame);
    }
    Frame fr;
    HIP_TRY(hipMemcpyAsync(&fr, fl.frame, sizeof fr, hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipStreamSynchronize(stream()));
    for (int d = 0; d < 3; d++) {
        f.lo[d] = (double)funkey_host(fr.mn[d]);
        f.extent[d] = (double)funkey_host(fr.mx[d]) - f.lo[d];
        if (!(f.extent[d] >= 0.0) || !std::isfinite(f.extent[d]) || !std::isfinite(f.lo[d])) return fail("%s: coordinates are not finite", c.who);
    }
    return 0;
}

// the open grid of a run: cells of the frame's box that hold the run's reach (reach2: its square)
OpenGrid open_grid(const LosFrame &f, double reach2) {
    const double reach = std::nextafter(std::sqrt(reach2), HUGE_VAL);   // rounded up
    OpenGrid og;
    for (int d = 0; d < 3; d++) {
        const double fit = std::floor(f.extent[d] / (reach * 1.0001));    // cell side >= 1.0001 reach (see OpenGrid)
        og.nc[d] = (int)std::min(128.0, std::max(1.0, fit));
        og.lo[d] = (float)f.lo[d];                                         // exact: a float32 coordinate
        og.inv[d] = f.extent[d] > 0.0 ? (float)((double)og.nc[d] / f.extent[d]) : 0.f;
    }
    return og;
}

// what the light-cone kernels read beside the sets: grid, binning and the pre-test's thresholds (derivation at LosArgs), rounded
// away from the accepted range [e2_lo, reach2)
void fill_los_args(LosArgs &a, const Binning &b, const OpenGrid &og, double reach2, double e2_lo) {
    for (int d = 0; d < 3; d++) a.nc[d] = og.nc[d];
    const double hi_d = reach2 * (1.0 + 0x1p-20), lo_d = e2_lo * (1.0 - 0x1p-20);
    float hi_f = (float)hi_d, lo_f = (float)lo_d;
    if ((double)hi_f < hi_d) hi_f = std::nextafterf(hi_f, HUGE_VALF);
    if ((double)lo_f > lo_d) lo_f = std::nextafterf(lo_f, 0.f);
    a.pre_hi = hi_f;
    a.pre_lo = b.mode != 1 && lo_d >= 1e-30 ? lo_f : 0.f;
    a.pimax = (double)b.pimax;
    a.dpi = b.npibins > 0 ? (double)b.pimax / b.npibins : 1.0;
    a.mu_max = (double)b.mu_max;
    a.inv_dmu = b.nmubins > 0 ? b.nmubins / (double)b.mu_max : 1.0;
    a.edges2 = g_work.edges.as<double>();
}

// The open driver.  plain: wsum == NULL: integer counts only (rsum is then ignored); jackknife: the same with both sums NULL
int count_los(const PairCall &c, const double *origin) {
    ABACUS_TRY(check_los(c, origin));
    ABACUS_ENTER();
    const Binning &b = c.bin;
    const JkSpec *jk = c.jk;
    const int mode = b.mode, autocorr = c.autocorr(), nsets = autocorr ? 1 : 2, nsub = b.nsub();
    const bool weighted = jk ? jk->out.wfirst != nullptr : c.out.wsum != nullptr, rs = !jk && weighted && c.out.rsum != nullptr;
    const Outputs result{c.out.npairs, c.out.wsum, rs ? c.out.rsum : nullptr};
    const size_t ntot_all = (size_t)b.nbins * nsub;
    if (jk) jk_zero(jk->out, (size_t)jk->nreg * ntot_all);
    else result.zero(ntot_all);
    g_stats = Stats{};
    if (c.empty()) return 0;

    Work &W = g_work;
    const int64_t ns[2] = {c.set[0].n, c.set[1].n};
    const int *dl[2] = {nullptr, nullptr};
    if (jk) ABACUS_TRY(jk_stage_labels(c.who, jk->labels, ns, nsets, c.where, jk->nreg, dl));
    Flags fl;
    ABACUS_TRY(W.flags(fl));
    LosFrame fr;
    ABACUS_TRY(los_frame(c, weighted, origin, fl, fr));
    JkOut jdev = {};
    if (jk) ABACUS_TRY(jk_device_outputs(jk->nreg, ntot_all, weighted, jdev, fl.evaluated + 1));
    // a run sorts the frame's columns into a grid of its own reach and counts
    ABACUS_TRY(for_runs(b.nbins, nsub, jk ? JK_MAX_HIST : W_MAX_HIST, [&](int b0, int nb, size_t o) -> int {
        const size_t ntot = (size_t)nb * nsub;
        std::vector<double> e2;
        ABACUS_TRY(upload_edges(b.bins + b0, nb, e2));
        const double reach2 = mode == 1 ? e2[nb] + (double)b.pimax * (double)b.pimax : e2[nb];
        const OpenGrid og = open_grid(fr, reach2);
        const int64_t ncell = (int64_t)og.nc[0] * og.nc[1] * og.nc[2];
        for (int k = 0; k < nsets; k++) {
            if (jk) ABACUS_TRY(sort_into_cells_jk(fr.cols[k], dl[k], ns[k], og, ncell, jk->nreg, k));
            else ABACUS_TRY(sort_into_cells(fr.cols[k], ns[k], og, ncell, W.S[k], W.scratch));
        }
        Outputs dev = {};
        if (!jk) ABACUS_TRY(device_outputs(ntot, true, false, dev));
        HIP_TRY(hipMemsetAsync(fl.evaluated, 0, 8, stream()));
        LosArgs a;
        fill_sets(a, a, autocorr, nb, nsub, dev);
        fill_los_args(a, b, og, reach2, e2[0]);
        int workgroups = 0;
        if (jk) ABACUS_TRY(launch_los_jk(mode, a, weighted, g_jk.sl[0], g_jk.sl[nsets - 1], jk_at(jdev, o), fl, ncell, workgroups));
        else ABACUS_TRY(launch_los(mode, a, weighted, rs, fl, ncell));
        if (!jk) ABACUS_TRY(fetch_outputs(result.at(o), dev, ntot));
        return record_run(fl, true, og.nc[0], og.nc[2], 0, og.nc, workgroups);
    }));
    if (jk) {
        ABACUS_TRY(jk_fetch(jk->out, jdev, (size_t)jk->nreg * ntot_all));
        HIP_TRY(hipStreamSynchronize(stream()));
    }
    return 0;
}

// The sphere driver (abacus_spherecount[_dev]).  Set 0 of the work buffers holds the queries - the data themselves when
// q[0] == NULL - and set 1 the data, both in one periodic grid of the full reach.
constexpr int SPH_MAX_RADII = 32;
struct SphereCall {
    const char *who;
    const void *p[3];    // the data
    int64_t n;
    const void *q[3];    // the queries; q[0] == NULL: the data are the queries (a point does not count itself)
    int64_t nq;
    int where;           // as PairCall::where
    float boxsize;
    const float *radii;
    int nr;
    float pimax;         // 0: spheres; > 0: cylinders along z, |dz| < pimax
    int kmax;
    uint64_t *hist;      // [nr][kmax + 1]
    uint32_t *counts;    // [nq][nr] in the caller's order, or NULL
    bool self() const { return q[0] == nullptr; }
};
struct SphereWork {
    DevBuf counts;
} g_sph;

int check_spheres(const SphereCall &c) {
    const char *who = c.who;
    if (c.where < 0) return fail("%s: pos_dtype must be ABACUS_F32 or ABACUS_F64", who);
    if (!c.p[0] || !c.p[1] || !c.p[2] || !c.radii || !c.hist) return fail("%s: null argument", who);
    if (!c.self() && (!c.q[1] || !c.q[2])) return fail("%s: null argument (qy / qz)", who);
    if (c.nr < 1 || c.nr > SPH_MAX_RADII) return fail("%s: nr = %d must lie in [1, %d]", who, c.nr, SPH_MAX_RADII);
    if (c.kmax < 1) return fail("%s: kmax must be at least 1", who);
    const long long nh = (long long)c.nr * ((long long)c.kmax + 1);
    if (nh > MAX_HIST) return fail("%s: nr * (kmax + 1) = %lld exceeds the LDS histogram of %d entries", who, nh, MAX_HIST);
    if (!(c.boxsize > 0)) return fail("%s: boxsize must be positive", who);
    if (!(c.radii[0] > 0.f)) return fail("%s: radii must be positive", who);
    for (int j = 1; j < c.nr; j++)
        if (!(c.radii[j] > c.radii[j - 1])) return fail("%s: radii must increase", who);
    if (!(c.pimax >= 0.f)) return fail("%s: pimax must be positive (0: spheres)", who);
    if (c.radii[c.nr - 1] > 0.5f * c.boxsize || c.pimax > 0.5f * c.boxsize)
        return fail("%s: the largest radius or pimax exceeds half the box (minimum image not unique)", who);
    if (c.n < 0 || c.n >= ((int64_t)1 << 31) || (!c.self() && (c.nq < 0 || c.nq >= ((int64_t)1 << 31))))
        return fail("%s: point counts must lie in [0, 2^31)", who);
    return 0;
}

int count_spheres(const SphereCall &c) {
    ABACUS_TRY(check_spheres(c));
    ABACUS_ENTER();
    const int self = c.self() ? 1 : 0, nsets = self ? 1 : 2, nr = c.nr, kw = c.kmax + 1;
    const int64_t nq = self ? c.n : c.nq;
    const size_t nh = (size_t)nr * kw;
    memset(c.hist, 0, nh * sizeof(uint64_t));
    if (c.counts) memset(c.counts, 0, (size_t)nq * nr * sizeof(uint32_t));
    g_stats = Stats{};
    if (nq == 0) return 0;
    if (c.n == 0) {   // nothing to count: every query has no neighbour
        for (int j = 0; j < nr; j++) c.hist[(size_t)j * kw] = (uint64_t)nq;
        return 0;
    }
    Work &W = g_work;
    const bool cyl = c.pimax > 0.f;
    const int64_t ns[2] = {nq, c.n};
    Flags fl;
    ABACUS_TRY(W.flags(fl));
    Columns cols[2];
    ABACUS_TRY(stage_columns("pair_cast", self ? c.p : c.q, nullptr, c.where, ns[0], nullptr, W.cols[0], W.wts[0], cols[0]));
    if (!self) ABACUS_TRY(stage_columns("pair_cast", c.p, nullptr, c.where, ns[1], nullptr, W.cols[1], W.wts[1], cols[1]));
    if (c.counts) {   // the caller's index of a query: the "weight" of set 0, a bit pattern the sort only moves
        ABACUS_TRY(W.wts[0].reserve((size_t)nq * 4));
        ABACUS_LAUNCH("sphere_iota", sphere_iota<unsigned int>, dim3((unsigned int)std::min<int64_t>(ceil_div(nq, 256), 2048)), dim3(256), 0,
                      W.wts[0].as<unsigned int>(), nq);
        cols[0].w = W.wts[0].as<float>();
    }
    const float reach = c.radii[nr - 1];
    CellGrid g;
    periodic_grid(c.boxsize, reach, cyl ? c.pimax : reach, true, 3, (double)std::max(ns[0], ns[1]), g);
    const int64_t ncell = (int64_t)g.ncx * g.ncy * g.ncz;
    for (int k = 0; k < nsets; k++) ABACUS_TRY(sort_into_cells(cols[k], ns[k], FramedGrid{g, fl.outside, fl.frame}, ncell, W.S[k], W.scratch));
    std::vector<float> e2;
    ABACUS_TRY(upload_edges(c.radii, nr - 1, e2));   // nr squared radii, float32 products
    ABACUS_TRY(W.out.reserve(nh * 8));
    HIP_TRY(hipMemsetAsync(W.out.p, 0, nh * 8, stream()));
    if (c.counts) ABACUS_TRY(g_sph.counts.reserve((size_t)nq * nr * 4));   // every row is written: each query belongs to one slice
    const SortedSet &Q = W.S[0], &P = W.S[self ? 0 : 1];
    SphereArgs a;
    a.g = g, a.nr = nr, a.kmax = c.kmax, a.autocorr = self;
    a.half = g.box * 0.5f, a.pimax = c.pimax;
    a.e2 = W.edges.as<float>();
    a.qx = Q.sx, a.qy = Q.sy, a.qz = Q.sz, a.qid = c.counts ? reinterpret_cast<const unsigned int *>(Q.sw) : nullptr;
    a.px = P.sx, a.py = P.sy, a.pz = P.sz;
    a.qstart = Q.start.as<int64_t>(), a.pstart = P.start.as<int64_t>();
    a.hist = W.out.as<unsigned long long>();
    a.counts = c.counts ? g_sph.counts.as<unsigned int>() : nullptr;
    a.nq = (unsigned int)nq;
    ABACUS_TRY(launch_spheres(a, cyl, fl, ncell));
    HIP_TRY(hipMemcpyAsync(c.hist, W.out.p, nh * 8, hipMemcpyDeviceToHost, stream()));
    if (c.counts) HIP_TRY(hipMemcpyAsync(c.counts, g_sph.counts.p, (size_t)nq * nr * 4, hipMemcpyDeviceToHost, stream()));
    return record_run(fl, false, g.ncx, g.ncz, 0, nullptr, 0);
}

// ------------------------------------------------------------------------------- three-point function multipoles ----
// zeta_l(r1, r2) of one catalogue on the periodic box by the multipole algorithm of Slepian & Eisenstein (2015)
// (abacus_threepcf[_dev]): per primary i the real spherical-harmonic sums a[bin][component] = sum_j w_j y_c(u_ij) over its
// neighbours, then the Gram matrix per l, which by the addition theorem is sum_{j,k} w_j w_k P_l(u_ij . u_ik); the j = k term
// (P_l(1) = 1: sum_j w_j^2) leaves the diagonal.  O(N k) instead of the O(N k^2) triplet count.  No reference code stands behind
// it; the NumPy statement tests/threepcf_statement.py is the judge (its `harmonic` form restates the components below).
//   pairs: the float32 expressions, the bins and the grid of pair_count_w mode 0 - npairs is bit-equal to that counter's.
//   components: (cm, sm) = w_j (Re, Im) (ux + i uy)^m and R_l^m(uz) by R_m^m = D_m, R_l^m = A_lm uz R_{l-1}^m - B_lm R_{l-2}^m
//   (the host's table `coef`: D | A | B); component l^2 is R_l^0 cm, l^2 + 2m - 1 and l^2 + 2m are R_l^m cm and R_l^m sm.
// Mapping: the walk of sphere_count - a persistent workgroup per primary cell, the neighbour cells as one virtual list, a lane
// per candidate - but ONE primary at a time, shared by the workgroup: its table a[nbins][ncomp] (15.5 KiB at 32 bins and
// lmax = 10) lives once in LDS.  Only ~15 % of the candidates of a 27-cell walk are counted, so a counted pair is not expanded
// where it is found: its direction, weight and bin go into an LDS queue (a ballot per wave, one LDS atomic on the fill count by
// its leader), and whenever the queue holds a workgroup's worth - and after the primary's last round - a pass takes 256 entries:
// a counting sort by bin in place (which also yields the pass's npairs), then an entry per lane: the recurrence in registers
// (two values per m, the loop bounds are uniform), and every component summed per bin inside each row of 16 lanes by four DPP
// steps before the first lane of a bin in its row adds it to the table - an LDS float atomic that at most four lanes of a wave
// share.  (Measured, 10^6 points, 10 bins, lmax 10: an LDS atomic per pair and component - 64 lanes on ten addresses - 228 ms;
// a whole-wave sum per bin of the wave 214 ms; the row-wise segmented sum 53 ms: profiles/threepcf/README.md.)  The order of the
// float32 atomics, and with it the last bits of zeta and wself, depends on the run.
// Gram step, once per primary with a counted pair: lane t owns the triples (l, b1 <= b2) t, t + PB, ...; the 2l + 1 products in
// float64 (exact products of float32), times w_i, into the lane's own float64 accumulators in LDS, which stay there across the
// primaries of all the workgroup's cells and leave once, by float64 global atomics.
struct TpcfArgs {
    CellGrid g;
    int nbins, lmax, npair, ntrip;   // npair = nbins (nbins + 1) / 2, ntrip = (lmax + 1) npair
    const float *e2;                 // nbins + 1 squared edges
    const float *coef;               // D[lmax + 1] | A[(lmax + 1)^2] | B[(lmax + 1)^2], A and B indexed l (lmax + 1) + m
    const float *x, *w;              // the catalogue in cell order: x | y | z, each `stride` floats apart; w NULL: unit weights
    int stride;
    const int64_t *start;
    double *out;                     // zeta [lmax + 1][npair] (the upper triangle, b1 <= b2, row by row) | wself [nbins] | npairs [nbins] |
                                     // candidate pairs evaluated [1] (the last two uint64)
};

constexpr int TPCF_QCAP = 2 * PB;    // a round adds at most PB entries to fewer than PB left over

// lane i's copy of lane i + D's value inside its row of 16 lanes (DPP row_shl); `edge` where the row ends before that
template <int D>
__device__ __forceinline__ int tpcf_row_next(int v, int edge) {
    return __builtin_amdgcn_update_dpp(edge, v, 0x100 + D, 0xF, 0xF, false);
}
template <int D>
__device__ __forceinline__ float tpcf_row_next(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x100 + D, 0xF, 0xF, true));
}

// a value for every element of a column (the weights of a set without weights beside one with)
template <typename T>
__global__ void threepcf_fill(T *__restrict__ dst, T v, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = v;
}

template <bool WEIGHTED>
__global__ __launch_bounds__(PB) void threepcf_walk(TpcfArgs a, int ncell) {
    __shared__ float4 qd[TPCF_QCAP];         // the queue: direction and w_j ...
    __shared__ int qb[TPCF_QCAP];            // ... and bin
    __shared__ int qn;                       // entries in the queue
    __shared__ int ncand;                    // candidates of the cell: the neighbour cells' populations together
    __shared__ int bcnt[32];                 // a pass: its entries per bin (zero between passes)
    __shared__ float e2[33];
    __shared__ int64_t nb_j0[27];
    __shared__ int nb_pre[28];
    extern __shared__ __align__(8) double tp_lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int nb = a.nbins, L1 = a.lmax + 1, nc = L1 * L1, ncoef = L1 + 2 * nc;
    // dynamic LDS: acc[ntrip] | wacc[nb] | hc[nb] (64-bit) | tab[nb][nc] | s2[nb] | coef[ncoef] (32-bit) | pr[npair] (16-bit)
    double *acc = tp_lds, *wacc = acc + a.ntrip;
    unsigned long long *hc = reinterpret_cast<unsigned long long *>(wacc + nb);
    float *tab = reinterpret_cast<float *>(hc + nb), *s2 = tab + nb * nc, *coef = s2 + nb;
    unsigned short *pr = reinterpret_cast<unsigned short *>(coef + ncoef);
    for (int q = tid; q < a.ntrip; q += PB) acc[q] = 0.0;
    for (int q = tid; q < nb; q += PB) wacc[q] = 0.0, hc[q] = 0ull;
    for (int q = tid; q < nb * nc + nb; q += PB) tab[q] = 0.f;   // the table and s2
    for (int q = tid; q < ncoef; q += PB) coef[q] = a.coef[q];
    for (int q = tid; q < a.npair; q += PB) {   // the q-th pair b1 <= b2, row by row
        int b1 = 0, left = q;
        while (left >= nb - b1) left -= nb - b1, b1++;
        pr[q] = (unsigned short)(b1 | ((b1 + left) << 8));
    }
    if (tid <= nb) e2[tid] = a.e2[tid];
    if (tid == 0) qn = 0;
    if (tid < 32) bcnt[tid] = 0;
    __syncthreads();
    const float *cD = coef, *cA = coef + L1, *cB = cA + nc;
    const float lo2 = e2[0], hi2 = e2[nb], half = a.g.box * 0.5f;
    unsigned long long n_eval = 0;

    // The first `cnt` entries of the queue, in bin order, one per lane: their components into the table.  The entries of a bin are
    // consecutive lanes, so a component is summed per bin inside every row of 16 lanes by a segmented suffix sum - four DPP steps
    // on the vector units, lane i taking lane i + d's partial sum where that lane holds the same bin - and the first lane of a
    // bin in its row adds the sum to the table: at most four lanes of a wave meet on one address, whatever the bins' populations.
    auto expand = [&](int cnt) {
        if ((tid & ~63) >= cnt) return;                  // per wave: no entry for it
        const bool live = tid < cnt;
        const float4 u = live ? qd[tid] : make_float4(0.f, 0.f, 0.f, 0.f);
        const int b = live ? qb[tid] : -1;               // (lanes without an entry: a bin of their own, sums of zeros, never added)
        // 1 where lane i + d holds the same bin, else 0: factors in vector registers (as lane masks they would cost eight scalars)
        const float t1 = tpcf_row_next<1>(b, -2) == b ? 1.f : 0.f, t2 = tpcf_row_next<2>(b, -2) == b ? 1.f : 0.f,
                    t4 = tpcf_row_next<4>(b, -2) == b ? 1.f : 0.f, t8 = tpcf_row_next<8>(b, -2) == b ? 1.f : 0.f;
        const bool head = live && __builtin_amdgcn_update_dpp(-2, b, 0x111, 0xF, 0xF, false) != b;   // row_shr:1: the lane before
        float *row = tab + (live ? b : 0) * nc;
        auto add = [&](float *dst, float v) {
            // (every lane runs the DPP move, then takes the value or not: inside the conditional only the taking lanes would be
            // active, and a DPP read of an inactive lane returns nothing)
            const float n1 = tpcf_row_next<1>(v);
            v += t1 * n1;
            const float n2 = tpcf_row_next<2>(v);
            v += t2 * n2;
            const float n4 = tpcf_row_next<4>(v);
            v += t4 * n4;
            const float n8 = tpcf_row_next<8>(v);
            v += t8 * n8;
            if (head) atomicAdd(dst, v);
        };
        add(&s2[live ? b : 0], u.w * u.w);
        float cm = u.w, sm = 0.f;
        for (int m = 0; m < L1; m++) {
            if (m) {
                const float c = cm * u.x - sm * u.y;
                sm = sm * u.x + cm * u.y;
                cm = c;
            }
            float p2 = 0.f, p1 = 0.f;
            for (int l = m; l < L1; l++) {
                const float r = l == m ? cD[m] : cA[l * L1 + m] * u.z * p1 - cB[l * L1 + m] * p2;
                p2 = p1, p1 = r;
                if (m == 0) {
                    add(row + l * l, r * cm);
                } else {
                    add(row + l * l + 2 * m - 1, r * cm);
                    add(row + l * l + 2 * m, r * sm);
                }
            }
        }
    };
    // A pass over the first cnt <= PB entries: a counting sort by bin in place (an entry waits in its lane's registers), the
    // pass's pairs per bin into npairs on the way, then the expansion.  Every lane of the workgroup calls.
    auto pass = [&](int cnt) {
        const bool live = tid < cnt;
        float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
        int b = 0, pos = 0;
        if (live) u = qd[tid], b = qb[tid], pos = atomicAdd(&bcnt[b], 1);
        __syncthreads();
        if (live)
            for (int k = 0; k < b; k++) pos += bcnt[k];
        if (tid < nb) hc[tid] += (unsigned long long)bcnt[tid];
        __syncthreads();
        if (live) qd[pos] = u, qb[pos] = b;
        if (tid < nb) bcnt[tid] = 0;
        __syncthreads();
        expand(cnt);
    };

    for (int c1 = blockIdx.x; c1 < ncell; c1 += gridDim.x) {
        const int64_t cbeg = a.start[c1], cend = a.start[c1 + 1];
        if (cbeg == cend) continue;
        __syncthreads();   // the previous cell's reads of the neighbour table are done
        if (tid < 64) {
            const int rx = a.g.ncx >= 3 ? 1 : 0, ry = a.g.ncy >= 3 ? 1 : 0, rz = a.g.ncz >= 3 ? 1 : 0;
            const int wy = 2 * ry + 1, wz = 2 * rz + 1, nnb = (2 * rx + 1) * wy * wz;
            int len = 0;
            int64_t j0 = 0;
            if (tid < nnb) {
                // (divisions by a vector-register copy of the grid that the compiler cannot see through: as scalars their
                // reciprocals would be formed once and held in six scalar registers across the whole kernel)
                int gz = a.g.ncz, gy = a.g.ncy;
                asm volatile("" : "+v"(gz), "+v"(gy));
                const int cz = c1 % gz, cy = (c1 / gz) % gy, cx = c1 / (gz * gy);
                int nx = cx + tid / (wy * wz) - rx, ny = cy + (tid / wz) % wy - ry, nz = cz + tid % wz - rz;
                nx = nx < 0 ? nx + a.g.ncx : (nx >= a.g.ncx ? nx - a.g.ncx : nx);
                ny = ny < 0 ? ny + a.g.ncy : (ny >= a.g.ncy ? ny - a.g.ncy : ny);
                nz = nz < 0 ? nz + a.g.ncz : (nz >= a.g.ncz ? nz - a.g.ncz : nz);
                const int c2 = (nx * a.g.ncy + ny) * a.g.ncz + nz;
                j0 = a.start[c2];
                len = (int)(a.start[c2 + 1] - j0);
            }
            int incl = len;
#pragma unroll
            for (int d = 1; d < 32; d <<= 1) {
                const int v = __shfl_up(incl, d, 64);
                if (tid >= d) incl += v;
            }
            if (tid < nnb) nb_j0[tid] = j0, nb_pre[tid] = incl - len;
            if (tid == nnb - 1) nb_pre[nnb] = incl, ncand = incl;
        }
        __syncthreads();
        const int M = ncand;
        for (int64_t i = cbeg; i < cend; i++) {
            // (the queue is empty, the table and s2 are zero, and a barrier stands behind all of that)
            const float xi = a.x[i], yi = a.x[i + a.stride], zi = a.x[i + 2 * (int64_t)a.stride];
            bool any = false;                            // the primary has a counted pair with a direction (uniform)
            for (int base = 0; base < M; base += PB) {
                n_eval += (unsigned long long)min(PB, M - base);
                const int v = base + tid;
                float4 e = make_float4(0.f, 0.f, 0.f, 0.f);
                int eb = -1;                               // the bin of a counted pair with a direction
                if (v < M) {
                    int sg = 0;
                    while (nb_pre[sg + 1] <= v) sg++;    // v < nb_pre[nnb]: ends at a non-empty cell
                    const int64_t jj = nb_j0[sg] + (v - nb_pre[sg]);
                    if (jj != i) {                        // not the primary itself, by identity
                        const float dx = min_image(xi - a.x[jj], half, a.g.box);
                        const float dy = min_image(yi - a.x[jj + a.stride], half, a.g.box);
                        const float dz = min_image(zi - a.x[jj + 2 * (int64_t)a.stride], half, a.g.box);
                        const float r2 = dx * dx + dy * dy + dz * dz;
                        if (!(r2 < lo2 || r2 >= hi2)) {
                            int b = nb - 1;
                            while (r2 < e2[b]) b--;
                            if (r2 > 0.f) {
                                const float r = sqrtf(r2);
                                e = make_float4(dx / r, dy / r, dz / r, WEIGHTED ? a.w[jj] : 1.f), eb = b;
                            } else {
                                atomicAdd(&hc[b], 1ull);  // a coincident twin (or a NaN): a pair of its bin without a direction
                            }
                        }
                    }
                }
                // into the queue: one atomic per wave (the ballot's leader), the lanes take consecutive slots behind it
                {
                    const unsigned long long mask = __builtin_amdgcn_ballot_w64(eb >= 0);
                    if (mask) {
                        const int leader = __ffsll((long long)mask) - 1;
                        int slot = 0;
                        if (lane == leader) slot = atomicAdd(&qn, __popcll(mask));
                        slot = __builtin_amdgcn_readlane(slot, leader) + (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)mask, 0u));
                        if (eb >= 0) qd[slot] = e, qb[slot] = eb;   // slot < TPCF_QCAP: fewer than PB were left, a round adds at most PB
                    }
                }
                __syncthreads();
                const int n = qn;
                __syncthreads();                           // every lane has read the count before the next round adds to it
                const bool last = base + PB >= M;
                if (n >= PB || (last && n > 0)) {
                    any = true;
                    pass(min(n, PB));
                    __syncthreads();                       // the first PB entries are read: the rest moves to the front
                    float4 td = make_float4(0.f, 0.f, 0.f, 0.f);
                    int tb = 0;
                    const int rest = n > PB ? n - PB : 0;
                    if (tid < rest) td = qd[PB + tid], tb = qb[PB + tid];
                    if (tid < rest) qd[tid] = td, qb[tid] = tb;   // PB + tid and tid: different entries, no lane reads what another writes
                    if (tid == 0) qn = rest;
                    __syncthreads();
                    if (last && rest > 0) {                // (n < 2 PB: one more pass empties the queue)
                        pass(rest);
                        __syncthreads();
                        if (tid == 0) qn = 0;
                    }
                }
            }
            if (!any) continue;
            __syncthreads();   // every component of this primary is in the table, and the queue is empty again
            const double wi = WEIGHTED ? (double)a.w[i] : 1.0;
            for (int t = tid; t < a.ntrip; t += PB) {
                const int l = t / a.npair, p = t - l * a.npair;
                const int b1 = pr[p] & 0xff, b2 = pr[p] >> 8;
                const float *r1 = tab + b1 * nc, *r2 = tab + b2 * nc;
                double g = 0.0;
                for (int c = l * l; c < (l + 1) * (l + 1); c++) g += (double)r1[c] * (double)r2[c];
                if (b1 == b2) g -= (double)s2[b1];
                acc[t] += wi * g;
            }
            if (tid < nb) wacc[tid] += wi * (double)s2[tid];
            __syncthreads();
            for (int q = tid; q < nb * nc + nb; q += PB) tab[q] = 0.f;
            __syncthreads();
        }
    }
    __syncthreads();
    if (tid == 0 && n_eval) atomicAdd(reinterpret_cast<unsigned long long *>(a.out + a.ntrip + 2 * nb), n_eval);
    for (int t = tid; t < a.ntrip; t += PB)
        if (acc[t] != 0.0) atomicAdd(&a.out[t], acc[t]);
    if (tid < nb) {
        if (wacc[tid] != 0.0) atomicAdd(&a.out[a.ntrip + tid], wacc[tid]);
        if (hc[tid]) atomicAdd(reinterpret_cast<unsigned long long *>(a.out + a.ntrip + nb) + tid, hc[tid]);
    }
}

// The 3PCF driver (abacus_threepcf[_dev]): set 2, when given, is appended to set 1 in HBM and the catalogue sorted into set 0 of
// the work buffers, its weight in the weight lane.
constexpr int TPCF_MAX_BINS = 32, TPCF_MAX_L = 10;
struct TpcfCall {
    const char *who;
    PointSet set[2];     // set[1].x[0] == NULL: no second set
    int where;           // as PairCall::where
    float boxsize;
    const float *bins;
    int nbins, lmax;
    double *zeta;        // [lmax + 1][nbins][nbins]
    double *wself;       // [nbins]
    uint64_t *npairs;    // [nbins]
};
struct TpcfWork {
    DevBuf cat, coef;    // the appended catalogue x | y | z | w; the recurrence's coefficients
    unsigned long long candidates = 0, counted = 0;
    int cells = 0;
} g_tpcf;

int check_threepcf(const TpcfCall &c) {
    const char *who = c.who;
    const PointSet &s1 = c.set[0], &s2 = c.set[1];
    if (c.where < 0) return fail("%s: pos_dtype must be ABACUS_F32 or ABACUS_F64", who);
    if (!s1.x[0] || !s1.x[1] || !s1.x[2] || !c.bins || !c.zeta || !c.wself || !c.npairs) return fail("%s: null argument", who);
    if (s2.x[0] && (!s2.x[1] || !s2.x[2])) return fail("%s: null argument (y2 / z2)", who);
    if (!s2.x[0] && (s2.x[1] || s2.x[2])) return fail("%s: y2 / z2 given without x2", who);
    if (!s2.x[0] && s2.w) return fail("%s: w2 given without a second set (x2 is NULL)", who);
    if (c.nbins < 1 || c.nbins > TPCF_MAX_BINS) return fail("%s: nbins = %d must lie in [1, %d]", who, c.nbins, TPCF_MAX_BINS);
    if (c.lmax < 0 || c.lmax > TPCF_MAX_L) return fail("%s: lmax = %d must lie in [0, %d]", who, c.lmax, TPCF_MAX_L);
    if (!(c.boxsize > 0)) return fail("%s: boxsize must be positive", who);
    if (!(c.bins[0] >= 0.f)) return fail("%s: bin edges must not be negative", who);
    for (int k = 0; k < c.nbins; k++)
        if (!(c.bins[k + 1] > c.bins[k])) return fail("%s: bin edges must increase", who);
    if (c.bins[c.nbins] > 0.5f * c.boxsize) return fail("%s: maximum separation exceeds half the box (minimum image not unique)", who);
    const int64_t n2 = s2.x[0] ? s2.n : 0;
    if (s1.n < 0 || n2 < 0 || s1.n >= ((int64_t)1 << 31) || n2 >= ((int64_t)1 << 31) || s1.n + n2 >= ((int64_t)1 << 31))
        return fail("%s: point counts must not be negative, with n + n2 < 2^31", who);
    return 0;
}

int count_threepcf(const TpcfCall &c) {
    ABACUS_TRY(check_threepcf(c));
    ABACUS_ENTER();
    const int nb = c.nbins, L1 = c.lmax + 1, nc = L1 * L1, npair = nb * (nb + 1) / 2, ntrip = L1 * npair;
    memset(c.zeta, 0, (size_t)L1 * nb * nb * sizeof(double));
    memset(c.wself, 0, (size_t)nb * sizeof(double));
    memset(c.npairs, 0, (size_t)nb * sizeof(uint64_t));
    g_stats = Stats{};
    g_tpcf.candidates = g_tpcf.counted = 0, g_tpcf.cells = 0;
    const int64_t n1 = c.set[0].n, n2 = c.set[1].x[0] ? c.set[1].n : 0, n = n1 + n2;
    if (n == 0) return 0;
    Work &W = g_work;
    Flags fl;
    ABACUS_TRY(W.flags(fl));
    Columns cols[2] = {}, cat;
    if (n1 > 0) ABACUS_TRY(stage_columns("pair_cast", c.set[0].x, c.set[0].w, c.where, n1, nullptr, W.cols[0], W.wts[0], cols[0]));
    if (n2 > 0) ABACUS_TRY(stage_columns("pair_cast", c.set[1].x, c.set[1].w, c.where, n2, nullptr, W.cols[1], W.wts[1], cols[1]));
    if (n2 == 0) {
        cat = cols[0];
    } else {   // set 2 behind set 1, column by column; a set without weights beside one with them counts with 1
        const bool weighted = (n1 > 0 && cols[0].w) || cols[1].w;
        ABACUS_TRY(g_tpcf.cat.reserve((size_t)n * 16));
        float *dst = g_tpcf.cat.as<float>();
        const int64_t ns[2] = {n1, n2}, at[2] = {0, n1};
        for (int k = 0; k < 2; k++) {
            if (ns[k] == 0) continue;
            for (int d = 0; d < 3; d++)
                HIP_TRY(hipMemcpyAsync(dst + (size_t)d * n + at[k], cols[k].x[d], (size_t)ns[k] * 4, hipMemcpyDeviceToDevice, stream()));
            if (weighted && cols[k].w)
                HIP_TRY(hipMemcpyAsync(dst + (size_t)3 * n + at[k], cols[k].w, (size_t)ns[k] * 4, hipMemcpyDeviceToDevice, stream()));
            else if (weighted)
                ABACUS_LAUNCH("threepcf_fill", threepcf_fill<float>, dim3((unsigned int)std::min<int64_t>(ceil_div(ns[k], 256), 2048)), dim3(256), 0,
                              dst + (size_t)3 * n + at[k], 1.0f, ns[k]);
        }
        for (int d = 0; d < 3; d++) cat.x[d] = dst + (size_t)d * n;
        cat.w = weighted ? dst + (size_t)3 * n : nullptr;
    }
    const float reach = c.bins[nb];
    CellGrid g;
    periodic_grid(c.boxsize, reach, reach, true, 3, (double)n, g);
    const int64_t ncell = (int64_t)g.ncx * g.ncy * g.ncz;
    ABACUS_TRY(sort_into_cells(cat, n, FramedGrid{g, fl.outside, fl.frame}, ncell, W.S[0], W.scratch));
    std::vector<float> e2;
    ABACUS_TRY(upload_edges(c.bins, nb, e2));
    // D | A | B of the recurrence, formed in float64 and rounded once
    std::vector<float> coef((size_t)L1 + 2 * nc, 0.f);
    double D = 1.0;
    for (int m = 0; m < L1; m++) {
        if (m) D *= std::sqrt((2.0 * m - 1.0) / (2.0 * m));
        coef[m] = (float)(m ? std::sqrt(2.0) * D : 1.0);
        for (int l = m + 1; l < L1; l++) {
            const double den = (double)l * l - (double)m * m;
            coef[L1 + l * L1 + m] = (float)((2.0 * l - 1.0) / std::sqrt(den));
            coef[L1 + nc + l * L1 + m] = (float)std::sqrt(((l - 1.0) * (l - 1.0) - (double)m * m) / den);
        }
    }
    ABACUS_TRY(g_tpcf.coef.reserve(coef.size() * 4));
    HIP_TRY(hipMemcpyAsync(g_tpcf.coef.p, coef.data(), coef.size() * 4, hipMemcpyHostToDevice, stream()));
    const size_t nout = (size_t)ntrip + 2 * nb + 1;   // zeta's upper triangles | wself | npairs | candidates
    ABACUS_TRY(W.out.reserve(nout * 8));
    HIP_TRY(hipMemsetAsync(W.out.p, 0, nout * 8, stream()));
    const SortedSet &S = W.S[0];
    TpcfArgs a;
    a.g = g, a.nbins = nb, a.lmax = c.lmax, a.npair = npair, a.ntrip = ntrip;
    a.e2 = W.edges.as<float>(), a.coef = g_tpcf.coef.as<float>();
    a.x = S.sx, a.w = S.sw, a.stride = (int)(S.sy - S.sx);   // sort_into_cells: y and z stand behind x, max(n, 1) floats apart
    a.start = S.start.as<int64_t>();
    a.out = W.out.as<double>();
    // acc | wacc | hc (8 B) | table | s2 | coef (4 B) | pairs (2 B): at most 46.4 + 0.5 + 15.5 + 0.1 + 1 + 1 KiB beside 11 KiB static
    const size_t lds = ((size_t)ntrip + 2 * nb) * 8 + ((size_t)nb * nc + nb + coef.size()) * 4 + (((size_t)npair + 3) & ~(size_t)3) * 2;
    ABACUS_TRY(with_flag(S.sw != nullptr, [&](auto WT) -> int {
        const auto kernel = threepcf_walk<decltype(WT)::value>;
        if (lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        dim3 grid;
        ABACUS_TRY(resident_grid(kernel, PB, lds, ncell, grid));
        ABACUS_LAUNCH("threepcf_walk", kernel, grid, dim3(PB), lds, a, (int)ncell);
        return 0;
    }));
    std::vector<double> up((size_t)ntrip);
    HIP_TRY(hipMemcpyAsync(up.data(), a.out, (size_t)ntrip * 8, hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipMemcpyAsync(c.wself, a.out + ntrip, (size_t)nb * 8, hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipMemcpyAsync(c.npairs, a.out + ntrip + nb, (size_t)nb * 8, hipMemcpyDeviceToHost, stream()));
    unsigned long long candidates = 0;
    HIP_TRY(hipMemcpyAsync(&candidates, a.out + ntrip + 2 * nb, 8, hipMemcpyDeviceToHost, stream()));
    ABACUS_TRY(record_run(fl, false, g.ncx, g.ncz, 0, nullptr, 0));   // synchronises
    g_stats.evaluated = candidates;
    // one triangle was computed: the other is its mirror, bit for bit
    for (int l = 0; l < L1; l++) {
        const double *src = up.data() + (size_t)l * npair;
        double *z = c.zeta + (size_t)l * nb * nb;
        for (int b1 = 0, p = 0; b1 < nb; b1++)
            for (int b2 = b1; b2 < nb; b2++, p++) z[b1 * nb + b2] = z[b2 * nb + b1] = src[p];
    }
    g_tpcf.candidates = g_stats.evaluated, g_tpcf.cells = g.ncx;
    for (int b = 0; b < nb; b++) g_tpcf.counted += c.npairs[b];
    return 0;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------- the C ABI ----
#define SETS(w1, w2) {{{x1, y1, z1}, w1, n1}, {{x2, y2, z2}, w2, n2}}
#define BINNING {mode, bins, nbins, pimax, npibins, mu_max, nmubins}
#define JK_SPEC const JkSpec jk = {{labels1, labels2}, nreg, {npairs_first, npairs_both, wsum_first, wsum_both}}

extern "C" int abacus_paircount(int mode, const float *x1, const float *y1, const float *z1, int64_t n1,
                                const float *x2, const float *y2, const float *z2, int64_t n2, float boxsize,
                                const float *bins, int nbins, float pimax, int npibins, float mu_max, int nmubins,
                                uint64_t *npairs) {
    return count_box({"abacus_paircount", SETS(nullptr, nullptr), 0, BINNING, {npairs, nullptr, nullptr}, nullptr}, boxsize, false);
}

extern "C" int abacus_paircount_dev(int mode, const void *x1, const void *y1, const void *z1, int64_t n1, const void *x2,
                                    const void *y2, const void *z2, int64_t n2, int pos_dtype, float boxsize, const float *bins,
                                    int nbins, float pimax, int npibins, float mu_max, int nmubins, uint64_t *npairs) {
    return count_box({"abacus_paircount_dev", SETS(nullptr, nullptr), where_of(pos_dtype), BINNING, {npairs, nullptr, nullptr}, nullptr},
                     boxsize, false);
}

extern "C" int abacus_paircount_weighted(int mode, const float *x1, const float *y1, const float *z1, const float *w1, int64_t n1,
                                         const float *x2, const float *y2, const float *z2, const float *w2, int64_t n2,
                                         float boxsize, const float *bins, int nbins, float pimax, int npibins, float mu_max,
                                         int nmubins, uint64_t *npairs, double *wsum, double *rsum) {
    return count_box({"abacus_paircount_weighted", SETS(w1, w2), 0, BINNING, {npairs, wsum, rsum}, nullptr}, boxsize, true);
}

extern "C" int abacus_paircount_weighted_dev(int mode, const void *x1, const void *y1, const void *z1, const float *w1, int64_t n1,
                                             const void *x2, const void *y2, const void *z2, const float *w2, int64_t n2,
                                             int pos_dtype, float boxsize, const float *bins, int nbins, float pimax, int npibins,
                                             float mu_max, int nmubins, uint64_t *npairs, double *wsum, double *rsum) {
    return count_box({"abacus_paircount_weighted_dev", SETS(w1, w2), where_of(pos_dtype), BINNING, {npairs, wsum, rsum}, nullptr}, boxsize,
                     true);
}

#define VSETS {{{x1, y1, z1}, w1, n1, {vx1, vy1, vz1}}, {{x2, y2, z2}, w2, n2, {vx2, vy2, vz2}}}
extern "C" int abacus_pairvel(int mode, const float *x1, const float *y1, const float *z1, const float *vx1, const float *vy1,
                              const float *vz1, const float *w1, int64_t n1, const float *x2, const float *y2, const float *z2,
                              const float *vx2, const float *vy2, const float *vz2, const float *w2, int64_t n2, float boxsize,
                              const float *bins, int nbins, float pimax, int npibins, float mu_max, int nmubins, uint64_t *npairs,
                              double *wsum, double *vsum) {
    const size_t ntot = (size_t)std::max(nbins, 0) * (size_t)std::max(mode == 0 ? 1 : (mode == 1 ? npibins : nmubins), 0);
    return count_box({"abacus_pairvel", VSETS, 0, BINNING, {npairs, wsum, nullptr, vsum, ntot}, nullptr, true}, boxsize, true);
}

extern "C" int abacus_pairvel_dev(int mode, const void *x1, const void *y1, const void *z1, const void *vx1, const void *vy1,
                                  const void *vz1, const float *w1, int64_t n1, const void *x2, const void *y2, const void *z2,
                                  const void *vx2, const void *vy2, const void *vz2, const float *w2, int64_t n2, int pos_dtype,
                                  float boxsize, const float *bins, int nbins, float pimax, int npibins, float mu_max, int nmubins,
                                  uint64_t *npairs, double *wsum, double *vsum) {
    const size_t ntot = (size_t)std::max(nbins, 0) * (size_t)std::max(mode == 0 ? 1 : (mode == 1 ? npibins : nmubins), 0);
    return count_box({"abacus_pairvel_dev", VSETS, where_of(pos_dtype), BINNING, {npairs, wsum, nullptr, vsum, ntot}, nullptr, true},
                     boxsize, true);
}
#undef VSETS

extern "C" int abacus_paircount_los(int mode, const float *x1, const float *y1, const float *z1, const float *w1, int64_t n1,
                                    const float *x2, const float *y2, const float *z2, const float *w2, int64_t n2,
                                    const double *origin, const float *bins, int nbins, float pimax, int npibins, float mu_max,
                                    int nmubins, uint64_t *npairs, double *wsum, double *rsum) {
    return count_los({"abacus_paircount_los", SETS(w1, w2), 0, BINNING, {npairs, wsum, rsum}, nullptr}, origin);
}

extern "C" int abacus_paircount_los_dev(int mode, const void *x1, const void *y1, const void *z1, const float *w1, int64_t n1,
                                        const void *x2, const void *y2, const void *z2, const float *w2, int64_t n2, int pos_dtype,
                                        const double *origin, const float *bins, int nbins, float pimax, int npibins,
                                        float mu_max, int nmubins, uint64_t *npairs, double *wsum, double *rsum) {
    return count_los({"abacus_paircount_los_dev", SETS(w1, w2), where_of(pos_dtype), BINNING, {npairs, wsum, rsum}, nullptr}, origin);
}

extern "C" int abacus_paircount_jk(int mode, const float *x1, const float *y1, const float *z1, const float *w1, const int32_t *labels1,
                                   int64_t n1, const float *x2, const float *y2, const float *z2, const float *w2, const int32_t *labels2,
                                   int64_t n2, int nreg, float boxsize, const float *bins, int nbins, float pimax, int npibins,
                                   float mu_max, int nmubins, uint64_t *npairs_first, uint64_t *npairs_both, double *wsum_first,
                                   double *wsum_both) {
    JK_SPEC;
    return count_box({"abacus_paircount_jk", SETS(w1, w2), 0, BINNING, {}, &jk}, boxsize, true);
}

extern "C" int abacus_paircount_jk_dev(int mode, const void *x1, const void *y1, const void *z1, const float *w1, const int32_t *labels1,
                                       int64_t n1, const void *x2, const void *y2, const void *z2, const float *w2, const int32_t *labels2,
                                       int64_t n2, int pos_dtype, int nreg, float boxsize, const float *bins, int nbins, float pimax,
                                       int npibins, float mu_max, int nmubins, uint64_t *npairs_first, uint64_t *npairs_both,
                                       double *wsum_first, double *wsum_both) {
    JK_SPEC;
    return count_box({"abacus_paircount_jk_dev", SETS(w1, w2), where_of(pos_dtype), BINNING, {}, &jk}, boxsize, true);
}

extern "C" int abacus_paircount_los_jk(int mode, const float *x1, const float *y1, const float *z1, const float *w1, const int32_t *labels1,
                                       int64_t n1, const float *x2, const float *y2, const float *z2, const float *w2,
                                       const int32_t *labels2, int64_t n2, int nreg, const double *origin, const float *bins, int nbins,
                                       float pimax, int npibins, float mu_max, int nmubins, uint64_t *npairs_first, uint64_t *npairs_both,
                                       double *wsum_first, double *wsum_both) {
    JK_SPEC;
    return count_los({"abacus_paircount_los_jk", SETS(w1, w2), 0, BINNING, {}, &jk}, origin);
}

extern "C" int abacus_paircount_los_jk_dev(int mode, const void *x1, const void *y1, const void *z1, const float *w1, const int32_t *labels1,
                                           int64_t n1, const void *x2, const void *y2, const void *z2, const float *w2,
                                           const int32_t *labels2, int64_t n2, int pos_dtype, int nreg, const double *origin,
                                           const float *bins, int nbins, float pimax, int npibins, float mu_max, int nmubins,
                                           uint64_t *npairs_first, uint64_t *npairs_both, double *wsum_first, double *wsum_both) {
    JK_SPEC;
    return count_los({"abacus_paircount_los_jk_dev", SETS(w1, w2), where_of(pos_dtype), BINNING, {}, &jk}, origin);
}
#undef SETS
#undef BINNING
#undef JK_SPEC

extern "C" int abacus_paircount_stats(uint64_t *candidates, int *ncell_xy, int *ncell_z, int *stencil_R) {
    ABACUS_ENTER();
    if (candidates) *candidates = g_stats.evaluated;
    if (ncell_xy) *ncell_xy = g_stats.cells[0];
    if (ncell_z) *ncell_z = g_stats.cells[1];
    if (stencil_R) *stencil_R = g_stats.cells[2];
    return 0;
}

extern "C" int abacus_paircount_los_grid(int *ncell) {
    ABACUS_ENTER();
    if (!ncell) return fail("abacus_paircount_los_grid: null argument");
    for (int d = 0; d < 3; d++) ncell[d] = g_stats.los_cells[d];
    return 0;
}

extern "C" int abacus_paircount_jk_stats(uint64_t *flushes, int *workgroups) {
    ABACUS_ENTER();
    if (flushes) *flushes = g_stats.flushes;
    if (workgroups) *workgroups = g_stats.workgroups;
    return 0;
}

extern "C" int abacus_spherecount(const float *x, const float *y, const float *z, int64_t n, const float *qx, const float *qy,
                                  const float *qz, int64_t nq, float boxsize, const float *radii, int nr, float pimax, int kmax,
                                  uint64_t *hist, uint32_t *counts) {
    return count_spheres({"abacus_spherecount", {x, y, z}, n, {qx, qy, qz}, nq, 0, boxsize, radii, nr, pimax, kmax, hist, counts});
}

extern "C" int abacus_spherecount_dev(const void *x, const void *y, const void *z, int64_t n, const void *qx, const void *qy,
                                      const void *qz, int64_t nq, int pos_dtype, float boxsize, const float *radii, int nr, float pimax,
                                      int kmax, uint64_t *hist, uint32_t *counts) {
    return count_spheres({"abacus_spherecount_dev", {x, y, z}, n, {qx, qy, qz}, nq, where_of(pos_dtype), boxsize, radii, nr, pimax, kmax,
                          hist, counts});
}

extern "C" int abacus_spherecount_stats(uint64_t *candidates, int *ncell_xy, int *ncell_z) {
    return abacus_paircount_stats(candidates, ncell_xy, ncell_z, nullptr);
}

extern "C" int abacus_threepcf(const float *x, const float *y, const float *z, const float *w, int64_t n, const float *x2,
                               const float *y2, const float *z2, const float *w2, int64_t n2, float boxsize, const float *bins, int nbins,
                               int lmax, double *zeta, double *wself, uint64_t *npairs) {
    return count_threepcf({"abacus_threepcf", {{{x, y, z}, w, n}, {{x2, y2, z2}, w2, n2}}, 0, boxsize, bins, nbins, lmax, zeta, wself, npairs});
}

extern "C" int abacus_threepcf_dev(const void *x, const void *y, const void *z, const float *w, int64_t n, const void *x2, const void *y2,
                                   const void *z2, const float *w2, int64_t n2, int pos_dtype, float boxsize, const float *bins, int nbins,
                                   int lmax, double *zeta, double *wself, uint64_t *npairs) {
    return count_threepcf({"abacus_threepcf_dev", {{{x, y, z}, w, n}, {{x2, y2, z2}, w2, n2}}, where_of(pos_dtype), boxsize, bins, nbins, lmax,
                           zeta, wself, npairs});
}

extern "C" int abacus_threepcf_stats(uint64_t *candidates, uint64_t *counted, int *ncell) {
    ABACUS_ENTER();
    if (candidates) *candidates = g_tpcf.candidates;
    if (counted) *counted = g_tpcf.counted;
    if (ncell) *ncell = g_tpcf.cells;
    return 0;
}

extern "C" int abacus_jk_box_labels_dev(const void *x, const void *y, const void *z, int pos_dtype, int64_t n, float boxsize, int nx, int ny,
                                        int nz, int32_t *labels) {
    if (pos_dtype != ABACUS_F32 && pos_dtype != ABACUS_F64) return fail("abacus_jk_box_labels_dev: pos_dtype must be ABACUS_F32 or ABACUS_F64");
    if (n < 0 || (n > 0 && (!x || !y || !z || !labels))) return fail("abacus_jk_box_labels_dev: bad argument");
    if (!(boxsize > 0)) return fail("abacus_jk_box_labels_dev: boxsize must be positive");
    if (nx < 1 || ny < 1 || nz < 1 || (int64_t)nx * ny * nz > JK_MAX_REG)
        return fail("abacus_jk_box_labels_dev: the split %d x %d x %d must have 1 .. %d regions", nx, ny, nz, JK_MAX_REG);
    ABACUS_ENTER();
    if (n == 0) return 0;
    const dim3 grid((unsigned int)std::min<int64_t>(ceil_div(n, 256), 2048));
    const float inv_box = 1.0f / boxsize;
    if (pos_dtype == ABACUS_F64)
        ABACUS_LAUNCH("pair_jk_box_labels", jk_box_labels<double>, grid, dim3(256), 0, (const double *)x, (const double *)y, (const double *)z, n,
                      inv_box, nx, ny, nz, labels);
    else
        ABACUS_LAUNCH("pair_jk_box_labels", jk_box_labels<float>, grid, dim3(256), 0, (const float *)x, (const float *)y, (const float *)z, n,
                      inv_box, nx, ny, nz, labels);
    HIP_TRY(hipStreamSynchronize(stream()));
    return 0;
}

// ------------------------------------------------------------------------------------- friends-of-friends groups ----
// Groups of one catalogue on the periodic box (abacus_fof[_dev]): the connected components of the friendship graph, as a label
// per point and the multiplicity function.  No reference code stands behind it; the NumPy statement tests/groups_statement.py
// is the judge, and its edge set is that of the counts in spheres with the single radius b_perp.
//   friends: i != j (by identity: a coincident twin is a friend) under the float32 expressions of sphere_count, bit for bit: d
//   = p_i - p_j per component through min_image, r2 = dx dx + dy dy + dz dz left to right and r2 < b b (b b a float32 product),
//   strictly; cylinders (b_par > 0, the line of sight along z): r2 = dx dx + dy dy, r2 < b_perp b_perp and |dz| < b_par.
//   out: labels[i] = the smallest caller's index among the members of i's group - a pure function of the input, whatever order
//   the unions ran in and whichever sort path put the points into cells; mult[N] = groups of exactly N members (N < nmax),
//   mult[nmax] = those of nmax or more; ngroups = sum of mult.
// This section stands at the file's end - behind the last entry point - so that its kernels are listed behind every kernel that
// was in the code object before, and those come out of the compiler as they did (the comment above sphere_iota).
//
// All union-find state lives in SORTED-index space: parent[s], uint32, s at first.  Four launches:
//   fof_link     the walk of sphere_count with the set as its own queries: a persistent workgroup per cell, the neighbour cells as
//                one virtual list, a lane per candidate, the cell's points an LDS slice read by broadcast.  A pair is taken only
//                when jj < ii in sorted index - cells are contiguous and ascending, so the cells behind the primary leave the
//                list and every unordered pair is taken once over the whole grid, on the one-cell-per-dimension grids too.  It
//                is counted by ballot and population count (a scalar add per wave) and united: find both roots, hook the larger
//                root under the smaller by atomicCAS that expects the larger to be a root still; a failed CAS returns what the
//                root was hooked under meanwhile, and the unite carries on from there.
//   fof_flatten  a launch later, so that every hook is visible: root[s] by a find with plain loads.
//   fof_reduce   per point atomicMin(minid[root], caller's index) and size[root] += 1, runs of equal roots combined inside the
//                wave first (a segmented scan: cell order makes such runs the rule, and a percolating group would otherwise put
//                every point's atomic on one word).
//   fof_emit     labels[caller's index] = minid[root]; every root bumps mult[min(size, nmax)] in an LDS histogram, flushed once
//                per workgroup by 64-bit atomics.
// Why fof_link cannot hang, and why stale reads are harmless:
//   * every write to parent[] in fof_link is an atomic whose new value is SMALLER than the old one: a hook is atomicCAS(parent[hi],
//     hi, lo) with lo < hi, on a root (path compression, if it ever returns, must be atomicMin for the same reason).  So
//     parent[s] <= s always, and no cycle forms;
//   * every find strictly descends (and returns at any value that would not: fof_find), every retry of a hook carries on from
//     indices strictly below the one whose CAS failed;
//   * no thread waits for another's progress: no locks, no flags, no spinning;
//   * a plain load of parent[] may return an old value from this CU's L1 or another XCD's L2.  An old value names a point that was
//     an ancestor and is one for ever after (trees only grow at their roots): it costs an extra step or a failed CAS, never a
//     wrong or a lost union - a union is made by a CAS that succeeded on a true root, or was found made already by values that were
//     true once;
//   * the final labels are exact because of the kernel boundary before fof_flatten, not because of fences in fof_link (it has none).
// Bound: n < 2^31 points; nmax + 1 <= MAX_HIST entries of LDS histogram; 16 bytes of union-find state per point beside the sort's.
namespace {

struct FofArgs {
    CellGrid g;
    float half, b2, bpar;          // box / 2; b_perp b_perp (a float32 product); b_par (cylinders)
    const float *px, *py, *pz;     // the catalogue in cell order
    const int64_t *start;
    unsigned int *parent;          // [n]
};

// the root above s as this thread sees it.  p < s at every step: a value that does not descend ends the walk, so the loop is bounded
// by s whatever the memory holds
__device__ __forceinline__ unsigned int fof_find(const unsigned int *parent, unsigned int s) {
    for (;;) {
        const unsigned int p = parent[s];
        if (p >= s) return s;
        s = p;
    }
}

// (no path compression here: an atomicMin(parent[s], root) on both points after their union was measured and made fof_link 0.5 to
// 9 % slower on every workload of profiles/groups/README.md - the trees stay shallow without it, fof_flatten takes 0.02 ms at 10^7)
__device__ __forceinline__ void fof_unite(unsigned int *parent, unsigned int a, unsigned int b) {
    a = fof_find(parent, a), b = fof_find(parent, b);
    while (a != b) {   // roots found equal by plain loads: united already, nothing to do
        const unsigned int hi = max(a, b), lo = min(a, b);
        const unsigned int old = atomicCAS(&parent[hi], hi, lo);
        if (old >= hi) return;       // == hi: hooked (> hi cannot be)
        a = fof_find(parent, old);   // hi was hooked under old < hi meanwhile: both indices are below hi now
        b = lo;
    }
}

template <bool CYL>
__global__ __launch_bounds__(PB) void fof_link(FofArgs a, int ncell, unsigned long long *__restrict__ ctr) {
    __shared__ float4 qp[PB];                // the slice: x, y, z
    __shared__ int64_t nb_j0[27];
    __shared__ int nb_pre[28];               // exclusive prefix of the neighbour cells' populations in front of the primary cell's end
    const int tid = threadIdx.x, lane = tid & 63;
    const int rx = a.g.ncx >= 3 ? 1 : 0, ry = a.g.ncy >= 3 ? 1 : 0, rz = a.g.ncz >= 3 ? 1 : 0;
    const int wy = 2 * ry + 1, wz = 2 * rz + 1, nnb = (2 * rx + 1) * wy * wz;
    unsigned long long n_eval = 0, n_link = 0;   // n_link: per wave
    for (int c1 = blockIdx.x; c1 < ncell; c1 += gridDim.x) {
        const int64_t cbeg = a.start[c1], cend = a.start[c1 + 1];
        if (cbeg == cend) continue;
        __syncthreads();   // the previous cell's reads of the neighbour table and of the slice are done
        if (tid < 64) {
            int len = 0;
            int64_t j0 = 0;
            if (tid < nnb) {
                const int cz = c1 % a.g.ncz, cy = (c1 / a.g.ncz) % a.g.ncy, cx = c1 / (a.g.ncz * a.g.ncy);
                int nx = cx + tid / (wy * wz) - rx, ny = cy + (tid / wz) % wy - ry, nz = cz + tid % wz - rz;
                nx = nx < 0 ? nx + a.g.ncx : (nx >= a.g.ncx ? nx - a.g.ncx : nx);
                ny = ny < 0 ? ny + a.g.ncy : (ny >= a.g.ncy ? ny - a.g.ncy : ny);
                nz = nz < 0 ? nz + a.g.ncz : (nz >= a.g.ncz ? nz - a.g.ncz : nz);
                const int c2 = (nx * a.g.ncy + ny) * a.g.ncz + nz;
                j0 = a.start[c2];
                // only jj < ii is taken: a cell behind the primary holds no such point, the primary itself all of them
                len = (int)max(min(a.start[c2 + 1], cend) - j0, (int64_t)0);
            }
            int incl = len;
#pragma unroll
            for (int d = 1; d < 32; d <<= 1) {
                const int v = __shfl_up(incl, d, 64);
                if (tid >= d) incl += v;
            }
            if (tid < nnb) nb_j0[tid] = j0, nb_pre[tid] = incl - len;
            if (tid == nnb - 1) nb_pre[nnb] = incl;
        }
        __syncthreads();
        const int M = nb_pre[nnb];
        for (int64_t i0 = cbeg; i0 < cend; i0 += PB) {
            const int ni = (int)min((int64_t)PB, cend - i0);
            if (i0 > cbeg) __syncthreads();   // the previous slice is read
            if (tid < ni) qp[tid] = make_float4(a.px[i0 + tid], a.py[i0 + tid], a.pz[i0 + tid], 0.f);
            __syncthreads();
            for (int base = 0; base < M; base += PB) {
                n_eval += (unsigned long long)ni * (unsigned long long)min(PB, M - base);
                if (base + (tid & ~63) >= M) continue;   // per wave: no candidate left for it in this round
                // every lane of the wave stays in the loop below (the ballots are over the whole wave); one without a point never matches
                const int v = base + tid;
                const bool have = v < M;
                float xj = 0.f, yj = 0.f, zj = 0.f;
                int64_t jj = cend;                       // behind every ii
                if (have) {
                    int sg = 0;
                    while (nb_pre[sg + 1] <= v) sg++;    // v < nb_pre[nnb]: ends at a non-empty cell
                    jj = nb_j0[sg] + (v - nb_pre[sg]);
                    xj = a.px[jj], yj = a.py[jj], zj = a.pz[jj];
                }
                for (int i = 0; i < ni; i++) {
                    const float4 q = qp[i];
                    // min_image, branch-free: its single addition of -+L, or of 0 (which leaves d, and -0 as +0: the same square)
                    float dx = q.x - xj, dy = q.y - yj, dz = q.z - zj;
                    dx += dx > a.half ? -a.g.box : (dx < -a.half ? a.g.box : 0.f);
                    dy += dy > a.half ? -a.g.box : (dy < -a.half ? a.g.box : 0.f);
                    dz += dz > a.half ? -a.g.box : (dz < -a.half ? a.g.box : 0.f);
                    bool fr = jj < i0 + i;               // once per unordered pair, and never the point itself
                    float r2;
                    if (CYL) {
                        r2 = dx * dx + dy * dy;
                        fr = fr && fabsf(dz) < a.bpar;
                    } else {
                        r2 = dx * dx + dy * dy + dz * dz;
                    }
                    fr = fr && r2 < a.b2;
                    const unsigned long long m = __builtin_amdgcn_ballot_w64(fr);
                    if (!m) continue;
                    n_link += (unsigned long long)__popcll(m);
                    if (fr) fof_unite(a.parent, (unsigned int)(i0 + i), (unsigned int)jj);
                }
            }
        }
    }
    if (tid == 0 && n_eval) atomicAdd(&ctr[0], n_eval);
    if (lane == 0 && n_link) atomicAdd(&ctr[1], n_link);
}

template <typename T>
__global__ void fof_flatten(const T *__restrict__ parent, T *__restrict__ root, int64_t n) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) root[s] = fof_find(parent, (T)s);
}

// LABELS: the smallest caller's index per root is wanted (id: the caller's index of sorted point s); sizes always.  A block takes
// whole waves' worth of consecutive points: every lane of a wave runs every round (the shuffles are over the whole wave)
template <bool LABELS>
__global__ __launch_bounds__(PB) void fof_reduce(const unsigned int *__restrict__ root, const unsigned int *__restrict__ id, int64_t n,
                                                 unsigned int *__restrict__ minid, unsigned int *__restrict__ size) {
    const int lane = threadIdx.x & 63;
    for (int64_t s0 = (int64_t)blockIdx.x * PB; s0 < n; s0 += (int64_t)gridDim.x * PB) {
        const int64_t s = s0 + threadIdx.x;
        const bool have = s < n;
        const unsigned int r = have ? root[s] : 0xffffffffu;
        unsigned int mn = LABELS && have ? id[s] : 0xffffffffu;
        const unsigned int before = __shfl_up(r, 1, 64);
        const unsigned long long heads = __builtin_amdgcn_ballot_w64(lane == 0 || before != r);
        const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
        const int first = 63 - __clzll((long long)(heads & upto));   // the head of this lane's run (bit 0 is set: lane 0 is a head)
        if (LABELS) {
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned int o = __shfl_up(mn, d, 64);
                if (lane - d >= first) mn = min(mn, o);
            }
        }
        const bool last = lane == 63 || ((heads >> (lane + 1)) & 1ull);
        if (have && last) {   // the run's last lane holds its minimum and knows its length
            if (LABELS) atomicMin(&minid[r], mn);
            atomicAdd(&size[r], (unsigned int)(lane - first + 1));
        }
    }
}

template <bool LABELS>
__global__ __launch_bounds__(PB) void fof_emit(const unsigned int *__restrict__ root, const unsigned int *__restrict__ id, int64_t n,
                                               const unsigned int *__restrict__ minid, const unsigned int *__restrict__ size, int nmax,
                                               unsigned int *__restrict__ labels, unsigned long long *__restrict__ mult) {
    extern __shared__ unsigned int fof_hist[];   // nmax + 1 entries
    for (int q = threadIdx.x; q <= nmax; q += PB) fof_hist[q] = 0u;
    __syncthreads();
    for (int64_t s = (int64_t)blockIdx.x * PB + threadIdx.x; s < n; s += (int64_t)gridDim.x * PB) {
        const unsigned int r = root[s];
        if (LABELS) {
            const unsigned int row = id[s];
            if ((int64_t)row < n) labels[row] = minid[r];   // (row < n always: the guard keeps a store inside the array whatever a sort did)
        }
        if ((int64_t)r == s) atomicAdd(&fof_hist[min(size[s], (unsigned int)nmax)], 1u);
    }
    __syncthreads();
    for (int q = threadIdx.x; q <= nmax; q += PB)
        if (fof_hist[q]) atomicAdd(&mult[q], (unsigned long long)fof_hist[q]);
}

struct FofCall {
    const char *who;
    const void *p[3];
    int64_t n;
    int where;           // as PairCall::where
    float boxsize, b_perp, b_par;   // b_par 0: spheres; > 0: cylinders along z
    int nmax;
    uint64_t *mult;      // [nmax + 1]
    uint32_t *labels;    // [n] in the caller's order, or NULL
    uint64_t *ngroups;
};
struct FofWork {
    DevBuf parent, root, minid, size;
    unsigned long long links = 0;
} g_fof;

int check_fof(const FofCall &c) {
    const char *who = c.who;
    if (c.where < 0) return fail("%s: pos_dtype must be ABACUS_F32 or ABACUS_F64", who);
    if (!c.p[0] || !c.p[1] || !c.p[2] || !c.mult || !c.ngroups) return fail("%s: null argument", who);
    if (!(c.boxsize > 0)) return fail("%s: boxsize must be positive", who);
    if (!(c.b_perp > 0.f)) return fail("%s: b_perp must be positive", who);
    if (!(c.b_par >= 0.f)) return fail("%s: b_par must not be negative (0: spheres)", who);
    if (c.b_perp > 0.5f * c.boxsize || c.b_par > 0.5f * c.boxsize)
        return fail("%s: b_perp or b_par exceeds half the box (minimum image not unique)", who);
    if (c.n < 0 || c.n >= ((int64_t)1 << 31)) return fail("%s: the point count must lie in [0, 2^31)", who);
    if (c.nmax < 1) return fail("%s: nmax must be at least 1", who);
    if ((long long)c.nmax + 1 > MAX_HIST) return fail("%s: nmax + 1 = %lld exceeds the LDS histogram of %d entries", who, (long long)c.nmax + 1, MAX_HIST);
    return 0;
}

int find_groups(const FofCall &c) {
    ABACUS_TRY(check_fof(c));
    ABACUS_ENTER();
    const int64_t n = c.n;
    const size_t nh = (size_t)c.nmax + 1;
    memset(c.mult, 0, nh * sizeof(uint64_t));
    if (c.labels) memset(c.labels, 0, (size_t)n * sizeof(uint32_t));
    *c.ngroups = 0;
    g_stats = Stats{};
    g_fof.links = 0;
    if (n == 0) return 0;
    Work &W = g_work;
    const bool cyl = c.b_par > 0.f, want = c.labels != nullptr;
    Flags fl;
    ABACUS_TRY(W.flags(fl));
    Columns cols;
    ABACUS_TRY(stage_columns("pair_cast", c.p, nullptr, c.where, n, nullptr, W.cols[0], W.wts[0], cols));
    const dim3 pts((unsigned int)std::min<int64_t>(ceil_div(n, 256), 2048));
    if (want) {   // the caller's index of a point: the "weight" of the set, a bit pattern the sort only moves
        ABACUS_TRY(W.wts[0].reserve((size_t)n * 4));
        ABACUS_LAUNCH("sphere_iota", sphere_iota<unsigned int>, pts, dim3(256), 0, W.wts[0].as<unsigned int>(), n);
        cols.w = W.wts[0].as<float>();
    }
    CellGrid g;
    periodic_grid(c.boxsize, c.b_perp, cyl ? c.b_par : c.b_perp, true, 3, (double)n, g);
    const int64_t ncell = (int64_t)g.ncx * g.ncy * g.ncz;
    ABACUS_TRY(sort_into_cells(cols, n, FramedGrid{g, fl.outside, fl.frame}, ncell, W.S[0], W.scratch));
    const SortedSet &S = W.S[0];
    ABACUS_TRY(g_fof.parent.reserve((size_t)n * 4));
    ABACUS_TRY(g_fof.root.reserve((size_t)n * 4));
    ABACUS_TRY(g_fof.size.reserve((size_t)n * 4));
    if (want) ABACUS_TRY(g_fof.minid.reserve((size_t)n * 4));
    ABACUS_TRY(W.out.reserve((nh + 2) * 8));   // mult | candidates, links
    HIP_TRY(hipMemsetAsync(W.out.p, 0, (nh + 2) * 8, stream()));
    HIP_TRY(hipMemsetAsync(g_fof.size.p, 0, (size_t)n * 4, stream()));
    if (want) HIP_TRY(hipMemsetAsync(g_fof.minid.p, 0xff, (size_t)n * 4, stream()));
    unsigned int *parent = g_fof.parent.as<unsigned int>(), *root = g_fof.root.as<unsigned int>();
    unsigned int *labels = parent;   // parent[] is read for the last time by fof_flatten
    unsigned long long *mult = W.out.as<unsigned long long>(), *ctr = mult + nh;
    ABACUS_LAUNCH("sphere_iota", sphere_iota<unsigned int>, pts, dim3(256), 0, parent, n);
    FofArgs a;
    a.g = g, a.half = g.box * 0.5f, a.b2 = c.b_perp * c.b_perp, a.bpar = c.b_par;
    a.px = S.sx, a.py = S.sy, a.pz = S.sz;
    a.start = S.start.as<int64_t>();
    a.parent = parent;
    ABACUS_TRY(with_flag(cyl, [&](auto CYL) -> int {
        const auto kernel = fof_link<decltype(CYL)::value>;
        dim3 grid;
        ABACUS_TRY(resident_grid(kernel, PB, 0, ncell, grid));
        ABACUS_LAUNCH("fof_link", kernel, grid, dim3(PB), 0, a, (int)ncell, ctr);
        return 0;
    }));
    ABACUS_LAUNCH("fof_flatten", fof_flatten<unsigned int>, pts, dim3(256), 0, parent, root, n);
    const unsigned int *id = reinterpret_cast<const unsigned int *>(S.sw);
    ABACUS_TRY(with_flag(want, [&](auto LB) -> int {
        constexpr bool L = decltype(LB)::value;
        ABACUS_LAUNCH("fof_reduce", fof_reduce<L>, pts, dim3(PB), 0, root, id, n, g_fof.minid.as<unsigned int>(), g_fof.size.as<unsigned int>());
        ABACUS_LAUNCH("fof_emit", fof_emit<L>, pts, dim3(PB), nh * sizeof(unsigned int), root, id, n, g_fof.minid.as<unsigned int>(),
                      g_fof.size.as<unsigned int>(), c.nmax, labels, mult);
        return 0;
    }));
    unsigned long long seen[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(c.mult, mult, nh * 8, hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipMemcpyAsync(seen, ctr, 16, hipMemcpyDeviceToHost, stream()));
    if (want) HIP_TRY(hipMemcpyAsync(c.labels, labels, (size_t)n * 4, hipMemcpyDeviceToHost, stream()));
    ABACUS_TRY(record_run(fl, false, g.ncx, g.ncz, 0, nullptr, 0));   // synchronises
    g_stats.evaluated = seen[0];
    g_fof.links = seen[1];
    for (size_t q = 0; q < nh; q++) *c.ngroups += c.mult[q];
    return 0;
}

}  // namespace

extern "C" int abacus_fof(const float *x, const float *y, const float *z, int64_t n, float boxsize, float b_perp, float b_par, int nmax,
                          uint64_t *mult, uint32_t *labels, uint64_t *ngroups) {
    return find_groups({"abacus_fof", {x, y, z}, n, 0, boxsize, b_perp, b_par, nmax, mult, labels, ngroups});
}

extern "C" int abacus_fof_dev(const void *x, const void *y, const void *z, int64_t n, int pos_dtype, float boxsize, float b_perp,
                              float b_par, int nmax, uint64_t *mult, uint32_t *labels, uint64_t *ngroups) {
    return find_groups({"abacus_fof", {x, y, z}, n, where_of(pos_dtype), boxsize, b_perp, b_par, nmax, mult, labels, ngroups});
}

extern "C" int abacus_fof_stats(uint64_t *candidates, uint64_t *links, int *ncell_xy, int *ncell_z) {
    ABACUS_ENTER();
    if (links) *links = g_fof.links;
    return abacus_paircount_stats(candidates, ncell_xy, ncell_z, nullptr);
}
