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
// The cell sort, the work buffers and the other families (jackknife, spheres, 3PCF, friends-of-friends): pairs_common.hpp lists
// the files.  Here: the unweighted periodic kernels pair_count (first generation: the comparator of the tests), pair_count2,
// pair_count3 (default); one walk in two bodies, pair_count_w (periodic, float32) and pair_count_los (open grid, float64);
// pair_vel, the walk of pair_count_w with the velocities of both sets; each kernel's launch below it; the two drivers, each the
// plain and - with labels - the jackknife counter (pairs_jk.hip), and the C ABI.
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "pairs_common.hpp"

using namespace abacus;
using namespace abacus::pairs;

namespace {

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
// pair_count_los below is this walk on the open grid, pair_vel its copy with velocities; pair_count_jk and pair_count_los_jk
// (pairs_jk.hip), sphere_count (spheres.hip), threepcf_walk (threepcf.hip) and fof_link (fof.hip) repeat it too: a fix to one
// walk belongs in all of them (profiles/pairs_shared_walk/README.md).
constexpr int W_MAX_HIST = 2048;

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

// Pairwise velocity sums (abacus_pairvel; halotools' mean_radial_velocity_vs_r / radial_pvd_vs_r / mean_los_velocity_vs_rp /
// los_pvd_vs_rp are moments of them).  The walk, the membership tests and the bin of pair_count_w, untouched - npairs and wsum are
// that counter's - with the velocities of both sets riding along; a fix to one walk belongs in all of them
// (the other copies: pair_count_w's comment names their files; profiles/pairs_shared_walk/README.md).  Per counted pair: u = v_i - v_j in float32, then float64, left to right, no FMA
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

// ---------------------------------------------------------------- host side: the outputs of a run (Outputs) in g_work.out ----
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

// ------------------------------------------------------------------------------------------------ the drivers ----
// A call as an entry point hands it on.  count_box (periodic) and count_los (open grid) serve the twelve entries; with a
// JkSpec they are the jackknife counters, without one the plain ones.  Inside a run they part only for the sort (labels ride
// along or not), the launch, and the device outputs (a block per run, or one [nreg][ntot] block of which a run takes columns).
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
        ABACUS_TRY(bounding_box(f.cols[k], s.n, fl.frame));
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
