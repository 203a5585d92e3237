// 3PCF multipoles on MI355X (gfx950); pairs_common.hpp lists the files of the pair-counting families.  threepcf_walk repeats the
// cell walk of sphere_count (spheres.hip), as do pairs.hip, pairs_jk.hip and fof.hip: a fix to one walk belongs in all of them.
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
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "pairs_common.hpp"

using namespace abacus;
using namespace abacus::pairs;

namespace {

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
