// Jackknife pair counts on MI355X (gfx950); pairs_common.hpp lists the files of the pair-counting families.
// Per-region pair counts in ONE walk (abacus_paircount_jk, abacus_paircount_los_jk): every point carries an int32 label in
// [0, nreg) and per (bin, sub-bin) q and region k
//   first[k][q] = pairs of q whose point of set 1 has label k,     both[k][q] = those whose point of set 2 has label k too,
// as integer counts and as sums of w_i w_j (float64 products and sums, like wsum of pairs.hip).  total[q] = sum_k first[k][q] is the
// parent counter's result; there are no separation sums here.  second[k][q] (the point of set 2 has label k) is no output:
// membership is symmetric under exchange of the two points in every mode of both families - d -> -d negates exactly (the
// minimum image adds -+L to -+d), so r^2, |dz|, mu, and on the light cone l = p_i + p_j, |t| and pi^2 are bit-equal - hence
// second of (1, 2) is first of (2, 1): the autocorrelation has second = first, a cross count calls again with the sets
// exchanged.  The expressions that decide membership and bin are those of pair_count_w / pair_count_los (pairs.hip), untouched,
// and so are their walks: a fix to one walk belongs in all of them (pairs.hip, spheres.hip, threepcf.hip, fof.hip hold the others).
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
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "pairs_common.hpp"

using namespace abacus;
using namespace abacus::pairs;

namespace abacus {
namespace pairs {
namespace {

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

void cap_jk_grid(dim3 &grid) {
    if (option("pairs_jk_grid") > 0) grid.x = std::min<unsigned int>(grid.x, (unsigned int)option("pairs_jk_grid"));
}

}  // namespace

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

}  // namespace pairs
}  // namespace abacus

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
