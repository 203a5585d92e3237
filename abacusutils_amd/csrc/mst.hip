// Minimum spanning forest on MI355X (gfx950); pairs_common.hpp lists the files of the pair-counting families.  mst_scan walks the
// 27 cells of sphere_count (spheres.hip) and fof_link (fof.hip): a fix to one walk belongs in all of them.
// The minimum spanning forest of the graph G(rmax) of one catalogue on the periodic box (abacus_mst[_dev]): its edges in a
// canonical order, the degree of every point in it and the label of every point's tree.  No reference code stands behind it; the
// NumPy statement tests/mst_statement.py (Kruskal, and Boruvka by rank) is the judge.
//   edges of G: i != j (by identity: a coincident twin is a neighbour at r2 = 0) under the float32 expressions of sphere_count and
//   fof_link, bit for bit: d = p_i - p_j per component through min_image, r2 = dx dx + dy dy + dz dz left to right, r2 < rmax rmax
//   (a float32 product), strictly - the edge set of abacus_fof with b_perp = rmax.  (d_ij = -d_ji exactly, so r2 is one number
//   per unordered pair.)
//   order: edges compare by the key (r2, lo, hi), lo < hi the caller's indices: strict and total, so the forest is unique - float32
//   r2 values tie (a lattice: all of them), and Boruvka without one consistent order builds cycles.
//   out: the forest's edges (lo, hi, r2) ascending in that key; degree[i]; labels[i] = the smallest caller's index in i's tree
//   (the labels of abacus_fof); nedges; ncomp = n - nedges.
//
// Boruvka's rounds.  All state lives in SORTED-index space (parent[s], root[s], the candidates, the two slots per root); the
// caller's index rides through the cell sort in the weight lane.  A round is four launches:
//   mst_scan     a persistent workgroup per cell whose points are not all settled.  The neighbour cells are one virtual list, staged
//                in LDS tiles of 256 candidates (x, y, z, root | caller's index | sorted index); the cell's live points are an LDS
//                slice, wave w takes the primaries w, w + 4, ... of the slice, a lane per candidate.  Per primary the lanes with
//                root[t] != root[s], r2 < rmax^2 and r2 <= the primary's best so far are taken by ballot - an empty ballot is the
//                rule once a near neighbour is seen - and compared under the full key one by one through readlane; lane k keeps
//                the best of the wave's k-th primary in registers.  No reduction over the wave, no LDS atomics.  After the walk
//                the point's candidate (r2, partner) is written and (r2 bits << 32 | lo) goes to slot1[root] by a 64-bit atomicMin
//                (the bits of a non-negative float order as an unsigned integer), skipped when a plain load shows a smaller value
//                there already: within the launch the slot only falls, so an old value costs an atomic, never a result - a
//                percolating tree would otherwise put every boundary point's atomic on one word.  A point without a candidate is
//                settled for good (trees only merge), a cell without a candidate is no primary again.  root[] is read-only here.
//   mst_tie      every point whose (r2, lo) equals its root's slot1 sends (hi << 32 | s) to slot2[root] by atomicMin: two 64-bit
//                minima stand in for the 96-bit key.  After it every root with an outgoing edge holds its minimum edge and the
//                point that owns it.
//   mst_hook     every such root r looks up the root r' of the owner's partner, emits the edge unless r' chose the same edge and
//                r > r', and unites r and r' (fof.hip's hook: atomicCAS on a root, larger under smaller).  Under a total order the
//                chosen edges minus the mutual duplicates form a forest over the roots, so the unions give the same trees, and the
//                same roots (the smallest sorted index), in whatever order they run.
//   mst_flatten  a launch later, so that every hook is visible: root[s] by a find from the old root with plain loads; the slots
//                back to "none".
// The host reads the round's counters and repeats until a round emits nothing.  Every tree with an outgoing edge is united with
// another one in its round, so their number at least halves: 31 rounds merge any n < 2^31, the loop is bounded at 32 and returns
// an error beyond - it is not a while (true).
// After the rounds: a stable radix sort (rocPRIM, as the cell sort) by (lo, hi), packed into one word, then by the bits of r2,
// which leaves the edges ascending in (r2, lo, hi) whatever order the atomics emitted them in; mst_unpack writes lo, hi, r2 and bumps
// the degrees; mst_reduce / mst_label are fof_reduce / fof_emit without the sizes.
// Why nothing here can hang, and why stale reads are harmless - the rules of fof.hip:
//   * every write to parent[] is an atomicCAS(parent[hi], hi, lo) with lo < hi on a root: parent[s] <= s always, no cycle forms;
//   * every find strictly descends (mst_find returns at any value that would not), every retry of a hook carries on from indices
//     strictly below the one whose CAS failed;
//   * no thread waits for another's progress: no locks, no flags, no spinning; the barriers of mst_scan are reached by every
//     thread of the workgroup (every loop around them runs on values the whole workgroup shares);
//   * slot1 / slot2 are written by atomicMin only and read for their value only a launch later; the plain loads that spare an
//     atomic are hints;
//   * a plain load of parent[] in mst_hook may return an old value: it names an ancestor that stays one (trees grow at their roots
//     only) and costs an extra step or a failed CAS;
//   * the results are exact because of the kernel boundaries between scan, tie, hook and flatten, not because of fences (there are
//     none).
// Bound: n < 2^31 points; 32 B of state per point beside the sort's during the rounds, 24 B per point of edge buffers and the
// sort's scratch; 12.6 KiB of static LDS and 65 VGPRs in mst_scan, no scratch in any kernel.
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "pairs_common.hpp"

using namespace abacus;
using namespace abacus::pairs;

namespace {

constexpr unsigned int NONE32 = 0xffffffffu;
constexpr unsigned long long NONE64 = ~0ull;
constexpr int MST_MAX_ROUNDS = 32;

struct MstArgs {
    CellGrid g;
    float half, b2;                // box / 2; rmax rmax (a float32 product)
    unsigned int n;
    int always_atomic;             // option mst_always_atomic (comparator): no plain load in front of the atomicMin on slot1
    const float *px, *py, *pz;     // the catalogue in cell order
    const unsigned int *id;        // the caller's index of a sorted point
    const int64_t *start;
    const unsigned int *root;      // [n], flattened a launch ago
    unsigned int *cand_r2, *cand_t;   // [n]: a point's best outgoing edge - the bits of r2 (NONE32: settled) and the partner's sorted index
    unsigned long long *slot1;     // [n], per root
    unsigned int *cell_live;       // [ncell]: some point of the cell found a candidate in the round before
};

// the root above s as this thread sees it.  p < s at every step: a value that does not descend ends the walk, so the loop is bounded
// by s whatever the memory holds (fof_find)
__device__ __forceinline__ unsigned int mst_find(const unsigned int *parent, unsigned int s) {
    for (;;) {
        const unsigned int p = parent[s];
        if (p >= s) return s;
        s = p;
    }
}

// fof_unite
__device__ __forceinline__ void mst_unite(unsigned int *parent, unsigned int a, unsigned int b) {
    a = mst_find(parent, a), b = mst_find(parent, b);
    while (a != b) {
        const unsigned int hi = max(a, b), lo = min(a, b);
        const unsigned int old = atomicCAS(&parent[hi], hi, lo);
        if (old >= hi) return;       // == hi: hooked (> hi cannot be)
        a = mst_find(parent, old);   // hi was hooked under old < hi meanwhile: both indices are below hi now
        b = lo;
    }
}

// 0, 1, 2 ... into a column: the caller's index of a point, which rides through the cell sort in the weight lane (as in spheres.hip)
template <typename T>
__global__ void sphere_iota(T *__restrict__ idx, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) idx[i] = (T)i;
}

__global__ void mst_init(unsigned int *__restrict__ parent, unsigned int *__restrict__ root, unsigned int *__restrict__ cand_r2,
                         unsigned long long *__restrict__ slot1, unsigned long long *__restrict__ slot2, int64_t n) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        parent[s] = root[s] = (unsigned int)s;
        cand_r2[s] = 0u;   // anything but NONE32: live
        slot1[s] = slot2[s] = NONE64;
    }
}

__device__ __forceinline__ unsigned int lane_value(unsigned int v, int l) {
    return (unsigned int)__builtin_amdgcn_readlane((int)v, l);
}

// ctr: [1] points scanned, [2] points that found a candidate
__global__ __launch_bounds__(PB) void mst_scan(MstArgs a, int ncell, unsigned long long *__restrict__ evaluated, unsigned long long *__restrict__ ctr) {
    __shared__ float4 qp[PB];                // the slice: x, y, z, the root as a bit pattern
    __shared__ unsigned int qid[PB], qlive[PB];
    __shared__ float4 cp[PB];                // the tile of candidates: the same
    __shared__ unsigned int cid[PB], cjj[PB];
    __shared__ int64_t nb_j0[27];
    __shared__ int nb_pre[28];               // exclusive prefix of the neighbour cells' populations
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rx = a.g.ncx >= 3 ? 1 : 0, ry = a.g.ncy >= 3 ? 1 : 0, rz = a.g.ncz >= 3 ? 1 : 0;
    const int wy = 2 * ry + 1, wz = 2 * rz + 1, nnb = (2 * rx + 1) * wy * wz;
    unsigned long long n_eval = 0;           // lane 0 of every wave
    unsigned int n_scan = 0, n_found = 0;    // per thread
    for (int c1 = blockIdx.x; c1 < ncell; c1 += gridDim.x) {
        const int64_t cbeg = a.start[c1], cend = a.start[c1 + 1];
        if (cbeg == cend || !a.cell_live[c1]) continue;   // (cell_live[c1] is written by the workgroup that takes c1, a launch ago)
        __syncthreads();   // the previous cell's reads of the neighbour table are done
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
                len = (int)(a.start[c2 + 1] - j0);
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
        int found_here = 0;
        for (int64_t i0 = cbeg; i0 < cend; i0 += PB) {
            const int ni = (int)min((int64_t)PB, cend - i0);
            __syncthreads();   // the previous slice and its last tile are read
            bool live = false;
            if (tid < ni) {
                const int64_t s = i0 + tid;
                live = a.cand_r2[s] != NONE32;
                qp[tid] = make_float4(a.px[s], a.py[s], a.pz[s], __uint_as_float(a.root[s]));
                qid[tid] = a.id[s], qlive[tid] = live ? 1u : 0u;
            }
            if (!__syncthreads_count(live)) continue;   // every point of the slice is settled
            n_scan += live ? 1u : 0u;
            const int nk = ni > wave ? (ni - wave + 3) >> 2 : 0;   // this wave's primaries: wave, wave + 4, ... ; lane k keeps the k-th one's best
            unsigned int br2 = NONE32, blo = NONE32, bhi = NONE32, bt = NONE32;
            for (int tb = 0; tb < M; tb += PB) {
                if (tb) __syncthreads();   // the previous tile is read
                const int v = tb + tid;
                if (v < M) {
                    int sg = 0;
                    while (nb_pre[sg + 1] <= v) sg++;    // v < nb_pre[nnb]: ends at a non-empty cell
                    const int64_t jj = nb_j0[sg] + (v - nb_pre[sg]);
                    cp[tid] = make_float4(a.px[jj], a.py[jj], a.pz[jj], __uint_as_float(a.root[jj]));
                    cid[tid] = a.id[jj], cjj[tid] = (unsigned int)jj;
                }
                __syncthreads();
                const int tn = min(PB, M - tb);
                for (int base = 0; base < tn; base += 64) {
                    // every lane of the wave stays in the loop below (the ballots are over the whole wave); one without a point never matches
                    const bool have = base + lane < tn;
                    const float4 c = have ? cp[base + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
                    const unsigned int rj = __float_as_uint(c.w), idj = have ? cid[base + lane] : 0u, jj = have ? cjj[base + lane] : 0u;
                    const unsigned long long width = (unsigned long long)min(64, tn - base);
                    for (int k = 0; k < nk; k++) {
                        const int i = wave + 4 * k;
                        if (!qlive[i]) continue;
                        if (lane == 0) n_eval += width;
                        const float4 q = qp[i];
                        const unsigned int idi = qid[i];
                        // min_image, branch-free: its single addition of -+L, or of 0 (which leaves d, and -0 as +0: the same square)
                        float dx = q.x - c.x, dy = q.y - c.y, dz = q.z - c.z;
                        dx += dx > a.half ? -a.g.box : (dx < -a.half ? a.g.box : 0.f);
                        dy += dy > a.half ? -a.g.box : (dy < -a.half ? a.g.box : 0.f);
                        dz += dz > a.half ? -a.g.box : (dz < -a.half ? a.g.box : 0.f);
                        const float r2 = dx * dx + dy * dy + dz * dz;
                        const unsigned int r2b = __float_as_uint(r2);
                        unsigned int s_r2 = lane_value(br2, k);
                        // another tree's point (which the point itself is not), inside rmax, and no longer than the best so far
                        const bool ok = have && rj != __float_as_uint(q.w) && r2 < a.b2 && r2b <= s_r2;
                        unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
                        if (!m) continue;
                        const unsigned int lo = min(idi, idj), hi = max(idi, idj);
                        unsigned int s_lo = lane_value(blo, k), s_hi = lane_value(bhi, k), s_t = lane_value(bt, k);
                        while (m) {   // the same for every lane: the values are the wave's
                            const int l = __builtin_ctzll(m);
                            m &= m - 1;
                            const unsigned int c_r2 = lane_value(r2b, l), c_lo = lane_value(lo, l), c_hi = lane_value(hi, l);
                            if (c_r2 < s_r2 || (c_r2 == s_r2 && (c_lo < s_lo || (c_lo == s_lo && c_hi < s_hi))))
                                s_r2 = c_r2, s_lo = c_lo, s_hi = c_hi, s_t = lane_value(jj, l);
                        }
                        if (lane == k) br2 = s_r2, blo = s_lo, bhi = s_hi, bt = s_t;
                    }
                }
            }
            if (lane < nk) {
                const int i = wave + 4 * lane;
                if (qlive[i]) {
                    const int64_t s = i0 + i;
                    a.cand_r2[s] = br2, a.cand_t[s] = bt;   // br2 NONE32: no outgoing edge, settled
                    if (br2 != NONE32) {
                        const unsigned int r = __float_as_uint(qp[i].w);
                        const unsigned long long key = ((unsigned long long)br2 << 32) | blo;
                        // (r < n always: the guard keeps the atomic inside the array)
                        if (r < a.n && (a.always_atomic || a.slot1[r] > key)) atomicMin(&a.slot1[r], key);
                        found_here = 1, n_found++;
                    }
                }
            }
        }
        const int any = __syncthreads_or(found_here);
        if (tid == 0) a.cell_live[c1] = any ? 1u : 0u;
    }
    if (lane == 0 && n_eval) atomicAdd(evaluated, n_eval);
    // per wave: the two point counts
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n_scan += __shfl_down(n_scan, d, 64), n_found += __shfl_down(n_found, d, 64);
    if (lane == 0 && n_scan) atomicAdd(&ctr[1], (unsigned long long)n_scan);
    if (lane == 0 && n_found) atomicAdd(&ctr[2], (unsigned long long)n_found);
}

__global__ void mst_tie(int64_t n, const unsigned int *__restrict__ root, const unsigned int *__restrict__ id,
                        const unsigned int *__restrict__ cand_r2, const unsigned int *__restrict__ cand_t,
                        const unsigned long long *__restrict__ slot1, unsigned long long *slot2) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        const unsigned int r2b = cand_r2[s];
        if (r2b == NONE32) continue;
        const unsigned int t = cand_t[s], r = root[s];
        if ((int64_t)t >= n || (int64_t)r >= n) continue;   // (never: the guards keep every access inside the arrays)
        const unsigned int ia = id[s], ib = id[t];
        const unsigned int lo = min(ia, ib), hi = max(ia, ib);
        if (slot1[r] != (((unsigned long long)r2b << 32) | lo)) continue;
        const unsigned long long key = ((unsigned long long)hi << 32) | (unsigned long long)s;
        if (slot2[r] > key) atomicMin(&slot2[r], key);
    }
}

// Every block takes whole waves' worth of consecutive roots: the emitted edges of a wave take their places by one atomic.
// ctr[0]: edges so far; e_key = lo << idbits | hi
__global__ __launch_bounds__(PB) void mst_hook(int64_t n, int idbits, const unsigned int *__restrict__ root, const unsigned int *__restrict__ cand_t,
                                               const unsigned long long *__restrict__ slot1, const unsigned long long *__restrict__ slot2,
                                               unsigned int *parent, unsigned int *__restrict__ e_r2, unsigned long long *__restrict__ e_key,
                                               unsigned long long *__restrict__ ctr) {
    const int lane = threadIdx.x & 63;
    for (int64_t s0 = (int64_t)blockIdx.x * PB; s0 < n; s0 += (int64_t)gridDim.x * PB) {
        const int64_t s = s0 + threadIdx.x;
        bool chose = false, emit = false;
        unsigned long long k1 = NONE64, k2 = NONE64;
        unsigned int rp = 0;
        if (s < n && root[s] == (unsigned int)s) {
            k1 = slot1[s], k2 = slot2[s];
            const unsigned int owner = (unsigned int)k2;
            if (k1 != NONE64 && k2 != NONE64 && (int64_t)owner < n) {
                const unsigned int t = cand_t[owner];
                if ((int64_t)t < n) {
                    rp = root[t];
                    if ((int64_t)rp < n && rp != (unsigned int)s) {
                        chose = true;
                        const bool mutual = slot1[rp] == k1 && (slot2[rp] >> 32) == (k2 >> 32);   // r' chose this very edge
                        emit = !(mutual && (unsigned int)s > rp);
                    }
                }
            }
        }
        const unsigned long long m = __builtin_amdgcn_ballot_w64(emit);
        if (m) {
            unsigned long long at = 0;
            if (lane == 0) at = atomicAdd(&ctr[0], (unsigned long long)__popcll(m));
            at = __shfl(at, 0, 64) + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
            if (emit && at < (unsigned long long)n) {   // (a forest has fewer than n edges: the guard keeps the store inside the arrays)
                e_r2[at] = (unsigned int)(k1 >> 32);
                e_key[at] = ((k1 & 0xffffffffull) << idbits) | (k2 >> 32);
            }
        }
        if (chose) mst_unite(parent, (unsigned int)s, rp);
    }
}

// root[s]: the old root's root now; the slots back to none
__global__ void mst_flatten(const unsigned int *__restrict__ parent, unsigned int *__restrict__ root, unsigned long long *__restrict__ slot1,
                            unsigned long long *__restrict__ slot2, int64_t n) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        const unsigned int r = root[s];
        root[s] = (int64_t)r < n ? mst_find(parent, r) : (unsigned int)s;
        slot1[s] = slot2[s] = NONE64;
    }
}

// the sorted edges into the output columns; the degrees in the caller's order
__global__ void mst_unpack(int64_t ne, int64_t n, int idbits, const unsigned int *__restrict__ e_r2, const unsigned long long *__restrict__ e_key,
                           unsigned int *__restrict__ out_i, unsigned int *__restrict__ out_j, unsigned int *degree) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long k = e_key[e];
        const unsigned int lo = (unsigned int)(k >> idbits), hi = (unsigned int)(k & ((1ull << idbits) - 1ull));
        out_i[e] = lo, out_j[e] = hi;
        if (degree && (int64_t)lo < n && (int64_t)hi < n) atomicAdd(&degree[lo], 1u), atomicAdd(&degree[hi], 1u);
    }
}

// fof_reduce without the sizes: atomicMin(minid[root], caller's index), runs of equal roots combined inside the wave first; and the
// number of roots, a population count per wave
template <bool LABELS>
__global__ __launch_bounds__(PB) void mst_reduce(const unsigned int *__restrict__ root, const unsigned int *__restrict__ id, int64_t n,
                                                 unsigned int *__restrict__ minid, unsigned long long *__restrict__ nroots) {
    const int lane = threadIdx.x & 63;
    unsigned long long mine = 0;
    for (int64_t s0 = (int64_t)blockIdx.x * PB; s0 < n; s0 += (int64_t)gridDim.x * PB) {
        const int64_t s = s0 + threadIdx.x;
        const bool have = s < n;
        const unsigned int r = have ? root[s] : NONE32;
        mine += (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(have && (int64_t)r == s));
        if (LABELS) {
            unsigned int mn = have ? id[s] : NONE32;
            const unsigned int before = __shfl_up(r, 1, 64);
            const unsigned long long heads = __builtin_amdgcn_ballot_w64(lane == 0 || before != r);
            const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
            const int first = 63 - __clzll((long long)(heads & upto));   // the head of this lane's run (bit 0 is set: lane 0 is a head)
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned int o = __shfl_up(mn, d, 64);
                if (lane - d >= first) mn = min(mn, o);
            }
            const bool last = lane == 63 || ((heads >> (lane + 1)) & 1ull);
            if (have && last && (int64_t)r < n) atomicMin(&minid[r], mn);   // the run's last lane holds its minimum
        }
    }
    if (lane == 0 && mine) atomicAdd(nroots, mine);
}

__global__ void mst_label(const unsigned int *__restrict__ root, const unsigned int *__restrict__ id, int64_t n,
                          const unsigned int *__restrict__ minid, unsigned int *__restrict__ labels) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        const unsigned int row = id[s], r = root[s];
        if ((int64_t)row < n && (int64_t)r < n) labels[row] = minid[r];   // (always: the guard keeps a store inside the array whatever a sort did)
    }
}

struct MstCall {
    const char *who;
    const void *p[3];
    int64_t n;
    int where;           // as PairCall::where
    float boxsize, rmax;
    uint32_t *edge_i, *edge_j;   // [n], the first nedges valid
    float *edge_r2;
    uint32_t *degree, *labels;   // [n] in the caller's order, or NULL
    uint64_t *nedges, *ncomp;
};
struct MstWork {
    DevBuf parent, root, cand_r2, cand_t, slot1, slot2, cell_live, r2a, r2b, keya, keyb, tmp, ctr;
    int rounds = 0;
    unsigned long long per_round[MST_MAX_ROUNDS][3] = {};   // points scanned, points with a candidate, edges emitted
} g_mst;

int check_mst(const MstCall &c) {
    const char *who = c.who;
    if (c.where < 0) return fail("%s: pos_dtype must be ABACUS_F32 or ABACUS_F64", who);
    if (!c.p[0] || !c.p[1] || !c.p[2] || !c.edge_i || !c.edge_j || !c.edge_r2 || !c.nedges || !c.ncomp) return fail("%s: null argument", who);
    if (!(c.boxsize > 0)) return fail("%s: boxsize must be positive", who);
    if (!(c.rmax > 0.f)) return fail("%s: rmax must be positive", who);
    if (c.rmax > 0.5f * c.boxsize) return fail("%s: rmax exceeds half the box (minimum image not unique)", who);
    if (c.n < 0 || c.n >= ((int64_t)1 << 31)) return fail("%s: the point count must lie in [0, 2^31)", who);
    return 0;
}

// ascending in (r2, lo, hi): a stable sort by the packed (lo, hi), then a stable sort by the bits of r2.  r2a / keya -> r2b / keyb -> r2a / keya
int sort_edges(int64_t ne, int idbits) {
    MstWork &M = g_mst;
    unsigned int *r2a = M.r2a.as<unsigned int>(), *r2b = M.r2b.as<unsigned int>();
    unsigned long long *keya = M.keya.as<unsigned long long>(), *keyb = M.keyb.as<unsigned long long>();
    size_t b1 = 0, b2 = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b1, keya, keyb, r2a, r2b, (int)ne, 0, 2 * idbits, stream());
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b2, r2b, r2a, keyb, keya, (int)ne, 0, 32, stream());
    ABACUS_TRY(M.tmp.reserve(std::max(b1, b2)));
    prof_begin("mst_edge_sort");   // library kernels (rocPRIM radix sort): listed with the hand-written ones
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(M.tmp.p, b1, keya, keyb, r2a, r2b, (int)ne, 0, 2 * idbits, stream());
    if (e == hipSuccess) e = hipcub::DeviceRadixSort::SortPairs(M.tmp.p, b2, r2b, r2a, keyb, keya, (int)ne, 0, 32, stream());
    prof_end("mst_edge_sort");
    if (e != hipSuccess) return fail("abacus_mst: radix sort of the edges failed");
    return 0;   // two passes: back in the first pair of buffers
}

int spanning_forest(const MstCall &c) {
    ABACUS_TRY(check_mst(c));
    ABACUS_ENTER();
    const int64_t n = c.n;
    *c.nedges = 0, *c.ncomp = 0;
    if (n > 0) {
        memset(c.edge_i, 0, (size_t)n * 4), memset(c.edge_j, 0, (size_t)n * 4), memset(c.edge_r2, 0, (size_t)n * 4);
        if (c.degree) memset(c.degree, 0, (size_t)n * 4);
        if (c.labels) memset(c.labels, 0, (size_t)n * 4);
    }
    g_stats = Stats{};
    MstWork &M = g_mst;
    M.rounds = 0;
    memset(M.per_round, 0, sizeof M.per_round);
    if (n == 0) return 0;
    Work &W = g_work;
    Flags fl;
    ABACUS_TRY(W.flags(fl));
    Columns cols;
    ABACUS_TRY(stage_columns("pair_cast", c.p, nullptr, c.where, n, nullptr, W.cols[0], W.wts[0], cols));
    const dim3 pts((unsigned int)std::min<int64_t>(ceil_div(n, 256), 2048));
    // the caller's index of a point: the "weight" of the set, a bit pattern the sort only moves
    ABACUS_TRY(W.wts[0].reserve((size_t)n * 4));
    ABACUS_LAUNCH("sphere_iota", sphere_iota<unsigned int>, pts, dim3(256), 0, W.wts[0].as<unsigned int>(), n);
    cols.w = W.wts[0].as<float>();
    CellGrid g;
    periodic_grid(c.boxsize, c.rmax, c.rmax, true, 3, (double)n, g);
    const int64_t ncell = (int64_t)g.ncx * g.ncy * g.ncz;
    ABACUS_TRY(sort_into_cells(cols, n, FramedGrid{g, fl.outside, fl.frame}, ncell, W.S[0], W.scratch));
    const SortedSet &S = W.S[0];
    const size_t n4 = (size_t)n * 4, n8 = (size_t)n * 8;
    ABACUS_TRY(M.parent.reserve(n4));
    ABACUS_TRY(M.root.reserve(n4));
    ABACUS_TRY(M.cand_r2.reserve(n4));
    ABACUS_TRY(M.cand_t.reserve(n4));
    ABACUS_TRY(M.slot1.reserve(n8));
    ABACUS_TRY(M.slot2.reserve(n8));
    ABACUS_TRY(M.cell_live.reserve((size_t)ncell * 4));
    ABACUS_TRY(M.r2a.reserve(n4));
    ABACUS_TRY(M.r2b.reserve(n4));
    ABACUS_TRY(M.keya.reserve(n8));
    ABACUS_TRY(M.keyb.reserve(n8));
    ABACUS_TRY(M.ctr.reserve(32));   // edges so far, points scanned, points with a candidate | roots
    HIP_TRY(hipMemsetAsync(M.ctr.p, 0, 32, stream()));
    HIP_TRY(hipMemsetAsync(M.cell_live.p, 0xff, (size_t)ncell * 4, stream()));
    unsigned int *parent = M.parent.as<unsigned int>(), *root = M.root.as<unsigned int>();
    unsigned long long *slot1 = M.slot1.as<unsigned long long>(), *slot2 = M.slot2.as<unsigned long long>();
    unsigned long long *ctr = M.ctr.as<unsigned long long>();
    const unsigned int *id = reinterpret_cast<const unsigned int *>(S.sw);
    ABACUS_LAUNCH("mst_init", mst_init, pts, dim3(256), 0, parent, root, M.cand_r2.as<unsigned int>(), slot1, slot2, n);
    MstArgs a;
    a.g = g, a.half = g.box * 0.5f, a.b2 = c.rmax * c.rmax, a.n = (unsigned int)n, a.always_atomic = option("mst_always_atomic");
    a.px = S.sx, a.py = S.sy, a.pz = S.sz, a.id = id;
    a.start = S.start.as<int64_t>();
    a.root = root;
    a.cand_r2 = M.cand_r2.as<unsigned int>(), a.cand_t = M.cand_t.as<unsigned int>();
    a.slot1 = slot1;
    a.cell_live = M.cell_live.as<unsigned int>();
    int idbits = 1;
    while (((int64_t)1 << idbits) < n) idbits++;   // bits that hold a caller's index: at most 31
    dim3 grid;
    ABACUS_TRY(resident_grid(mst_scan, PB, 0, ncell, grid));
    unsigned long long edges = 0, before[3] = {0, 0, 0};   // the counters are sums over the rounds
    bool done = false;
    // mst_round_names (scripts/mst_probe.py): the profiler lists the kernels of every round under a name of their own, "mst_scan@03"
    const bool by_round = prof_enabled() && option("mst_round_names");
    for (int round = 0; round < MST_MAX_ROUNDS && !done; round++) {
        char name[4][24];
        const char *kernels[4] = {"mst_scan", "mst_tie", "mst_hook", "mst_flatten"};
        for (int q = 0; q < 4; q++) snprintf(name[q], sizeof name[q], by_round ? "%s@%02d" : "%s", kernels[q], round);
        ABACUS_LAUNCH(name[0], mst_scan, grid, dim3(PB), 0, a, (int)ncell, fl.evaluated, ctr);
        ABACUS_LAUNCH(name[1], mst_tie, pts, dim3(256), 0, n, root, id, a.cand_r2, a.cand_t, slot1, slot2);
        ABACUS_LAUNCH(name[2], mst_hook, pts, dim3(PB), 0, n, idbits, root, a.cand_t, slot1, slot2, parent, M.r2a.as<unsigned int>(),
                      M.keya.as<unsigned long long>(), ctr);
        ABACUS_LAUNCH(name[3], mst_flatten, pts, dim3(256), 0, parent, root, slot1, slot2, n);
        unsigned long long seen[3] = {0, 0, 0};
        HIP_TRY(hipMemcpyAsync(seen, ctr, 24, hipMemcpyDeviceToHost, stream()));
        HIP_TRY(hipStreamSynchronize(stream()));
        if (seen[0] >= (unsigned long long)n) return fail("%s: %llu edges among %lld points: not a forest", c.who, seen[0], (long long)n);
        M.per_round[round][0] = seen[1] - before[1];
        M.per_round[round][1] = seen[2] - before[2];
        M.per_round[round][2] = seen[0] - before[0];
        done = seen[0] == edges;
        edges = seen[0];
        memcpy(before, seen, sizeof before);
        if (!done) M.rounds = round + 1;
    }
    if (!done) return fail("%s: the trees still merge after %d rounds", c.who, MST_MAX_ROUNDS);
    const int64_t ne = (int64_t)edges;
    // after the rounds: the slots, the candidates and parent[] are dead - the output columns, the degrees, minid and the labels
    // take their memory
    unsigned int *out_i = M.slot1.as<unsigned int>(), *out_j = out_i + n;
    unsigned int *degree = c.degree ? M.cand_r2.as<unsigned int>() : nullptr, *minid = M.cand_t.as<unsigned int>(), *labels = parent;
    if (ne > 0) {
        ABACUS_TRY(sort_edges(ne, idbits));
        if (degree) HIP_TRY(hipMemsetAsync(degree, 0, n4, stream()));
        ABACUS_LAUNCH("mst_unpack", mst_unpack, dim3((unsigned int)std::min<int64_t>(ceil_div(ne, 256), 2048)), dim3(256), 0, ne, n, idbits,
                      M.r2a.as<unsigned int>(), M.keya.as<unsigned long long>(), out_i, out_j, degree);
        HIP_TRY(hipMemcpyAsync(c.edge_i, out_i, (size_t)ne * 4, hipMemcpyDeviceToHost, stream()));
        HIP_TRY(hipMemcpyAsync(c.edge_j, out_j, (size_t)ne * 4, hipMemcpyDeviceToHost, stream()));
        HIP_TRY(hipMemcpyAsync(c.edge_r2, M.r2a.p, (size_t)ne * 4, hipMemcpyDeviceToHost, stream()));
        if (degree) HIP_TRY(hipMemcpyAsync(c.degree, degree, n4, hipMemcpyDeviceToHost, stream()));
    }
    if (c.labels) {
        HIP_TRY(hipMemsetAsync(minid, 0xff, n4, stream()));
        ABACUS_LAUNCH("mst_reduce", mst_reduce<true>, pts, dim3(PB), 0, root, id, n, minid, ctr + 3);
        ABACUS_LAUNCH("mst_label", mst_label, pts, dim3(256), 0, root, id, n, minid, labels);
        HIP_TRY(hipMemcpyAsync(c.labels, labels, n4, hipMemcpyDeviceToHost, stream()));
    } else {
        ABACUS_LAUNCH("mst_reduce", mst_reduce<false>, pts, dim3(PB), 0, root, id, n, minid, ctr + 3);
    }
    unsigned long long nroots = 0;
    HIP_TRY(hipMemcpyAsync(&nroots, ctr + 3, 8, hipMemcpyDeviceToHost, stream()));
    ABACUS_TRY(record_run(fl, false, g.ncx, g.ncz, 0, nullptr, 0));   // synchronises
    if (nroots + edges != (unsigned long long)n)
        return fail("%s: %llu edges and %llu trees among %lld points: not a spanning forest", c.who, edges, nroots, (long long)n);
    *c.nedges = edges, *c.ncomp = nroots;
    return 0;
}

}  // namespace

extern "C" int abacus_mst(const float *x, const float *y, const float *z, int64_t n, float boxsize, float rmax, uint32_t *edge_i,
                          uint32_t *edge_j, float *edge_r2, uint32_t *degree, uint32_t *labels, uint64_t *nedges, uint64_t *ncomp) {
    return spanning_forest({"abacus_mst", {x, y, z}, n, 0, boxsize, rmax, edge_i, edge_j, edge_r2, degree, labels, nedges, ncomp});
}

extern "C" int abacus_mst_dev(const void *x, const void *y, const void *z, int64_t n, int pos_dtype, float boxsize, float rmax,
                              uint32_t *edge_i, uint32_t *edge_j, float *edge_r2, uint32_t *degree, uint32_t *labels, uint64_t *nedges,
                              uint64_t *ncomp) {
    return spanning_forest({"abacus_mst", {x, y, z}, n, where_of(pos_dtype), boxsize, rmax, edge_i, edge_j, edge_r2, degree, labels, nedges, ncomp});
}

extern "C" int abacus_mst_stats(uint64_t *candidates, int *rounds, int *ncell_xy, int *ncell_z, uint64_t *per_round) {
    ABACUS_ENTER();
    if (rounds) *rounds = g_mst.rounds;
    for (int q = 0; per_round && q < MST_MAX_ROUNDS * 3; q++) per_round[q] = g_mst.per_round[q / 3][q % 3];
    return abacus_paircount_stats(candidates, ncell_xy, ncell_z, nullptr);
}
