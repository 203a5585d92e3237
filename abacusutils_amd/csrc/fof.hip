// Friends-of-friends groups on MI355X (gfx950); pairs_common.hpp lists the files of the pair-counting families.  fof_link repeats
// the cell walk of sphere_count (spheres.hip), as do pairs.hip, pairs_jk.hip and threepcf.hip: a fix to one walk belongs in all of them.
// Groups of one catalogue on the periodic box (abacus_fof[_dev]): the connected components of the friendship graph, as a label
// per point and the multiplicity function.  No reference code stands behind it; the NumPy statement tests/groups_statement.py
// is the judge, and its edge set is that of the counts in spheres with the single radius b_perp.
//   friends: i != j (by identity: a coincident twin is a friend) under the float32 expressions of sphere_count, bit for bit: d
//   = p_i - p_j per component through min_image, r2 = dx dx + dy dy + dz dz left to right and r2 < b b (b b a float32 product),
//   strictly; cylinders (b_par > 0, the line of sight along z): r2 = dx dx + dy dy, r2 < b_perp b_perp and |dz| < b_par.
//   out: labels[i] = the smallest caller's index among the members of i's group - a pure function of the input, whatever order
//   the unions ran in and whichever sort path put the points into cells; mult[N] = groups of exactly N members (N < nmax),
//   mult[nmax] = those of nmax or more; ngroups = sum of mult.
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
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "pairs_common.hpp"

using namespace abacus;
using namespace abacus::pairs;

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

// 0, 1, 2 ... into a column: the caller's index of a point, which rides through the cell sort in the weight lane (as in spheres.hip)
template <typename T>
__global__ void sphere_iota(T *__restrict__ idx, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) idx[i] = (T)i;
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
