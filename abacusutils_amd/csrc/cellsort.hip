// The cell sort of every pair-counting family (pairs_common.hpp lists the files): points into the cells of a periodic or an open
// grid, by a counting sort below 200 000 points and a stable radix sort above; the jackknife's sort by (cell, label); staging of
// the caller's columns; the grids; and the one set of work buffers and statistics the families take turns on.
// Every hipCUB call of the library's pair counters stands in THIS file: rocPRIM's kernels come out of the compiler differently
// when a translation unit holds only some of the sorts.
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "pairs_common.hpp"

using namespace abacus;
using namespace abacus::pairs;

namespace abacus {
namespace pairs {

// the one set of work buffers, the bookkeeping of the last call and the jackknife's labels (pairs_common.hpp)
Work g_work;
Stats g_stats;
JkWork g_jk;

namespace {

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

template <bool COUNT, bool W, typename Grid>
int count_cells(const Columns &c, int64_t n, const Grid &g, SortedSet &s, int nblk) {
    ABACUS_LAUNCH("pair_cell_count", (cell_count<COUNT, W, Grid>), dim3(nblk), dim3(256), 0, c.x[0], c.x[1], c.x[2], COUNT ? nullptr : c.w, n, g,
                  COUNT ? s.counts.as<unsigned int>() : nullptr, s.cellid.as<unsigned int>(), COUNT ? nullptr : s.idx.as<unsigned int>(),
                  COUNT ? nullptr : s.packed.as<float4>());
    return 0;
}

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

}  // namespace

// What follows is declared, with its contract, in pairs_common.hpp
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

template <typename Grid>
int sort_into_cells(const Columns &c, int64_t n, const Grid &g, int64_t ncell, SortedSet &s, DevBuf &scratch, const float *const *vel) {
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

template int sort_into_cells<FramedGrid>(const Columns &, int64_t, const FramedGrid &, int64_t, SortedSet &, DevBuf &, const float *const *);
template int sort_into_cells<OpenGrid>(const Columns &, int64_t, const OpenGrid &, int64_t, SortedSet &, DevBuf &, const float *const *);

// (for the light-cone driver of pairs.hip: bbox_minmax is this file's kernel)
int bounding_box(const Columns &c, int64_t n, Frame *frame) {
    ABACUS_LAUNCH("pair_los_bbox", bbox_minmax, dim3((unsigned int)std::min<int64_t>(ceil_div(n, 256), 1024)), dim3(256), 0, c.x[0], c.x[1],
                  c.x[2], n, frame);
    return 0;
}

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

template int sort_into_cells_jk<CellGrid>(const Columns &, const int *, int64_t, const CellGrid &, int64_t, int, int);
template int sort_into_cells_jk<OpenGrid>(const Columns &, const int *, int64_t, const OpenGrid &, int64_t, int, int);

// (the jackknife's label staging and its "labels span" refusal stand here, not in pairs_jk.hip: jk_label_range is this file's kernel)
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

int cu_count(int &ncu) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    return 0;
}

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

}  // namespace pairs
}  // namespace abacus

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
