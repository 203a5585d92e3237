// Counts in spheres on MI355X (gfx950); pairs_common.hpp lists the files of the pair-counting families.  sphere_count repeats the
// cell walk of pair_count_w (pairs.hip), as do pairs_jk.hip, threepcf.hip and fof.hip: a fix to one walk belongs in all of them.
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
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "pairs_common.hpp"

using namespace abacus;
using namespace abacus::pairs;

namespace {

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

// 0, 1, 2 ... into a column: the caller's index of a point, which rides through the cell sort in the weight lane
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

}  // namespace

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
