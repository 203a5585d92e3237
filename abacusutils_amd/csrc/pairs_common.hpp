// What the pair-counting families share: grids, kernel argument structs, the one set of work buffers and the host helpers
// around the cell sort.  Everything here is declared once, in abacus::pairs; the sources keep what is theirs alone in an anonymous
// namespace.
//   pairs_common.hpp  this file
//   cellsort.hip      the cell sort of every family (counting sort, radix sort, the label-aware sort of the jackknife - with
//                     mst.hip the only file that includes hipCUB), staging of the caller's columns, the grids, g_work / g_stats / g_jk
//   pairs.hip         pair_count, pair_count2, pair_count3, pair_count_w, pair_vel, pair_count_los with their launches; the
//                     drivers count_box (periodic) and count_los (open grid); the C ABI of the plain and jackknife counters
//   pairs_jk.hip      pair_count_jk, pair_count_los_jk (the two walks with per-region histograms), their outputs and launches
//   spheres.hip       sphere_count and its driver (abacus_spherecount)
//   threepcf.hip      threepcf_walk and its driver (abacus_threepcf)
//   fof.hip           fof_link, fof_flatten, fof_reduce, fof_emit and their driver (abacus_fof)
//   mst.hip           mst_scan, mst_tie, mst_hook, mst_flatten (Boruvka's rounds), the edge sort (hipCUB, the second file that
//                     includes it), mst_unpack, mst_reduce, mst_label and their driver (abacus_mst)
// The cell walk stands in pair_count_w, pair_vel, pair_count_los (pairs.hip), pair_count_jk, pair_count_los_jk (pairs_jk.hip),
// sphere_count (spheres.hip), threepcf_walk (threepcf.hip), fof_link (fof.hip) and mst_scan (mst.hip): a fix to one walk belongs
// in all of them (profiles/pairs_shared_walk/README.md).
#pragma once

#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/abacus_hip.h"
#include "common.hpp"

namespace abacus {
namespace pairs {

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

// The periodic grid as the cell sort takes it: it alone keeps the frame and `outside` (some coordinate is not in [0, L))
struct FramedGrid : CellGrid {
    int *outside;
    Frame *frame;
};

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

// the weighted walks (pair_count_w, pair_vel, pair_count_jk)
struct WeightArgs {
    const float *w1, *w2;   // weights in cell order; NULL: unit weights
    double *wsum, *rsum;    // rsum is read only when RSUM
};

// the light-cone walks (pair_count_los, pair_count_los_jk): derivation of the pre-test at pair_count_los in pairs.hip
struct LosArgs {
    int autocorr, nc[3], nbins, nsub;
    // float32 pre-test: a candidate with s2f > pre_hi or s2f < pre_lo skips the float64 arithmetic
    float pre_lo, pre_hi;
    double pimax, dpi, mu_max, inv_dmu;
    const double *edges2;   // (nbins + 1) squared edges
    const float *x1, *y1, *z1, *w1, *x2, *y2, *z2, *w2;   // cell order; w NULL: unit weights
    const int64_t *start1, *start2;
    unsigned long long *npairs;
    double *wsum, *rsum;
};

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

// The work buffers of every family: the library serialises its entry points (ABACUS_ENTER), so the families take turns on ONE
// set (defined in cellsort.hip).  None may rely on what the one before left in it: a sort sets sw afresh, sv only with velocities
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
};
extern Work g_work;

struct Columns {   // float32 device columns of a set, with its weights (NULL: none)
    const float *x[3], *w;
};

// Caller columns -> float32 device columns.  where = 0: host float32 arrays (and host weights); 1: device float32; 2: device
// float64 (device weights).  origin (NULL: none) is subtracted in the column's own dtype before the one rounding; device float32
// columns that need no shift are read in place.  n > 0.  `label` names the conversion kernel to the profiler.
int stage_columns(const char *label, const void *const src[3], const float *w, int where, int64_t n, const double *origin,
                  DevBuf &cols, DevBuf &wts, Columns &c);

// The set in cell order on either grid (ncell cells): s.sx | sy | sz, s.start and - with weights - s.sw.  vel (NULL: none): three
// float32 device columns that follow their points into s.sv; such a set takes the radix sort at every size, whose sorted index
// says where a point went (the counting sort hands out slots by atomics and keeps no index).  n > 0 with vel.
template <typename Grid>
int sort_into_cells(const Columns &c, int64_t n, const Grid &g, int64_t ncell, SortedSet &s, DevBuf &scratch, const float *const *vel = nullptr);

// the bounding box of a set into *frame (device), as order-preserving keys (fkey)
int bounding_box(const Columns &c, int64_t n, Frame *frame);

// f(std::integral_constant<int, mode>()): the mode as a template argument of what f launches
template <typename F>
int with_mode(int mode, F &&f) {
    if (mode == 0) return f(std::integral_constant<int, 0>());
    if (mode == 1) return f(std::integral_constant<int, 1>());
    return f(std::integral_constant<int, 2>());
}
template <typename F>
int with_flag(bool on, F &&f) { return on ? f(std::true_type()) : f(std::false_type()); }

int cu_count(int &ncu);

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

// a set as an entry point hands it on
struct PointSet {
    const void *x[3];
    const float *w;   // NULL: unit weights
    int64_t n;
    const void *v[3];   // velocity columns of a velocity call (PairCall::vel), in the dtype of x
};
inline int where_of(int pos_dtype) { return pos_dtype == ABACUS_F32 ? 1 : (pos_dtype == ABACUS_F64 ? 2 : -1); }

// Bookkeeping of the last call (abacus_paircount_stats, abacus_paircount_los_grid, abacus_paircount_jk_stats): zero when a call
// starts, so what an empty or a refused-on-the-device call leaves is zero in all of them
struct Stats {
    unsigned long long evaluated = 0, flushes = 0;   // candidate pairs (not of the first two generations); jackknife flushes
    int cells[3] = {0, 0, 0};                        // cells in xy, in z, stencil half-width R (0: not pair_count3)
    int los_cells[3] = {0, 0, 0};
    int workgroups = 0;
};
extern Stats g_stats;

// A run's candidate count and, behind it in the block of flags, the flush count of the jackknife kernels (over the call so
// far; 0 from any other kernel) come to the host with the run's synchronise; `sum`: the candidates add up over the runs (light
// cone), else the last run's stand.  workgroups: of a jackknife launch
int record_run(const Flags &fl, bool sum, int ncxy, int ncz, int R, const int *los_nc, int workgroups);

// The periodic grid of a run and its stencil half-width R.  Jackknife and weighted counts walk the 27 cells of the full reach.
// The unweighted kernels take cells of size >= reach / R: R = 2 (125-cell stencil of cells an eighth the volume: 1.7x fewer
// candidate pairs) when the catalogue is dense enough to keep a wave busy with a small cell, else R = 1
int periodic_grid(float boxsize, float reach_xy, float reach_z, bool full_reach, int gen, double nmax, CellGrid &g);

// ------------------------------------------------------------------------------------------ jackknife pair counts ----
// What the two drivers see of the jackknife (pairs_jk.hip).  The label-aware sort, and with it the staging and range check of
// the labels (jk_stage_labels launches jk_label_range), stand with their kernels in cellsort.hip
constexpr int JK_MAX_HIST = 2048;
constexpr int JK_MAX_REG = 65535;
constexpr int64_t JK_MAX_OUT = (int64_t)1 << 24;

struct JkOut {   // four arrays [nreg][stride]; a run's kernel writes columns 0 .. nh of every row (the pointers are offset)
    unsigned long long *nfirst, *nboth;
    double *wfirst, *wboth;   // not read by an unweighted kernel
    size_t stride;
    unsigned long long *flushes;
};

struct JkHostOut {
    uint64_t *nfirst, *nboth;
    double *wfirst, *wboth;
};

// labels as uploaded, the sort's keys, and the labels in (cell, label) order: sl[k] of set k, set by sort_into_cells_jk
struct JkWork {
    DevBuf labs[2], keys[2], sorted_labels[2], range;
    int *sl[2];
};
extern JkWork g_jk;

// The set in (cell, label) order on either grid: s.sx | sy | sz, s.start, s.sw with weights, and g_jk.sl[k].  One stable radix
// sort for every size (the counting sort of sort_into_cells leaves the order inside a cell to the run); n > 0
template <typename Grid>
int sort_into_cells_jk(const Columns &c, const int *labels, int64_t n, const Grid &g, int64_t ncell, int nreg, int k);

// what both drivers check before the device is touched
int jk_check(const char *who, int nreg, int nbins, int nsub, int autocorr, const void *labels1, const void *labels2, int64_t n1, int64_t n2,
             const JkHostOut &o, bool need_sums);
// labels in HBM (host labels are uploaded) and range-checked by a device reduction: nothing is sorted or counted with a label
// outside [0, nreg)
int jk_stage_labels(const char *who, const int32_t *const src[2], const int64_t ns[2], int nsets, int where, int nreg, const int *dl[2]);
// the four output arrays in g_work.out, zeroed: [nreg][ntot] each
int jk_device_outputs(int nreg, size_t ntot, bool sums, JkOut &d, unsigned long long *flushes);
JkOut jk_at(const JkOut &d, size_t o);
int jk_fetch(const JkHostOut &h, const JkOut &d, size_t cnt);
void jk_zero(const JkHostOut &h, size_t cnt);
// The jackknife launches of a run; out: the run's columns of the [nreg][ntot] block.  They take fewer workgroups on request
// (pairs_jk_grid, tests: many cells per workgroup) and report how many they took.
int launch_jk(const PairArgs &a, const WeightArgs &wa, const int *lab1, const int *lab2, const JkOut &out, const Flags &fl, int64_t ncell,
              int &workgroups);
int launch_los_jk(int mode, const LosArgs &a, bool weighted, const int *lab1, const int *lab2, const JkOut &out, const Flags &fl,
                  int64_t ncell, int &workgroups);

}  // namespace pairs
}  // namespace abacus
