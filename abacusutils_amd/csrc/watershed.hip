// Watershed voids of a periodic mesh on MI355X (gfx950): the zones of steepest descent (the basins of ZOBOV / VIDE and of the voxel
// finder of REVOLVER), their sums, and the saddle tree - the minimum spanning tree of the zone graph under the saddle order, which is
// the ZOBOV hierarchy and the 0-dimensional persistence of the field.  Python: analysis/watershed.py; the arithmetic is stated in
// include/abacus_hip.h and pinned to the NumPy statement tests/watershed_statement.py.
// replaces: nothing in the reference, which has no void finder.
//
// Every decision compares integers.  The key of a cell is one uint64: the order-preserving image of its float32 value (-0.0 taken as
// +0.0 first) in the high half, its flat index f = (x n + y) n + z < 2^30 in the low half - unique, so "the smallest key among a cell
// and its neighbours" and "the smallest edge out of a component" are well defined.  The keys are not stored: a kernel that needs one
// reads the mesh (4 bytes) and forms it.
//
//   ws_descend  down[f] = the low half of the smallest key among f and its 6 or 26 periodic neighbours.  One thread per cell, lanes
//               along z; the stencil's rows come from the L1 / L2 (no LDS tile - see profiles/watershed/README.md).  Honours the row
//               pitch: a cell (x, y, z) is read at (x n + y) pitch + z with z < n, never a pad float.
//   ws_jump     lab[f] = lab[lab[f]] in place, a launch per pass, until a pass changes nothing.  A concurrent read sees an older or a
//               newer pointer; both lie on f's path to its core, so the fixed point - every cell points at its core - is the same on
//               every run, whatever the number of passes.  A path of p steps needs at most log2(p) + 1 passes: 31 for p < 2^30; the
//               host loop is bounded at 40 and fails beyond.
//   ws_mark / exclusive_scan_u32 / ws_number   cores flagged, counted in ascending flat index (scan.hip), the labels rewritten in
//               place to zone numbers (a thread reads and writes its own entry only); a core writes its zone's cell and keyed value.
//   ws_reduce   per cell: its zone's ncell and the three minimum-image offsets from the core (64-bit integer atomics) and delta_sum
//               (a float64 atomic: the one inexact output, its order is free).  Neighbouring lanes mostly share a zone - the constant
//               mesh is one zone - so the runs of equal zones inside a wave are summed by a segmented shuffle scan and the last lane
//               of a run issues the five atomics (option ws_reduce_per_cell: the comparator without that).
//   the saddle tree, Boruvka's rounds over the zones, the pattern of mst.hip.  A round is four launches:
//     ws_edges<min>  every cell looks at the forward half of its neighbours (3 of 6, 13 of 26: every adjacent cell pair once).  For a
//                    pair in different components, khi = the larger of the two keys goes to slot1 of both components by a 64-bit
//                    atomicMin, skipped when a plain load shows a value no larger (within the launch a slot only falls).
//     ws_edges<tie>  the same walk; a pair whose khi equals a component's slot1 sends klo, the smaller key, to its slot2.  (khi, klo)
//                    names one cell pair, so after this launch a component's two slots are its smallest outgoing edge.
//     ws_hook        every root r with an edge finds the root r' at the other end, emits the edge unless r' chose the same one and
//                    r > r', and unites the two (atomicCAS on a root, larger index under smaller).
//     ws_flatten     a launch later: root[z] by a find from the old root; the slots back to "none".
//   The host reads the edge count per round and stops at Z - 1 edges (the torus is connected).  Every component merges in every round,
//   so their number at least halves: 30 rounds cover Z < 2^30; the loop is bounded at 32 and fails beyond - it is not a while (true).
//   The Z - 1 edges go to the host and are sorted there by (khi, klo): the order in which rising water joins basins.
// Why nothing here can hang: no thread waits for another - no locks, flags or spinning; ws_find strictly descends and returns at any
// value that would not; every write to parent[] is an atomicCAS(parent[hi], hi, lo) with lo < hi; slot1 / slot2 are written by
// atomicMin only and read for their value a launch later.  The kernel boundaries are the synchronisation; there are no fences.
// Every index read from memory is checked against its array before it is used as one.
//
// Compiled with -ffp-contract=off (the default of csrc/Makefile); the only float arithmetic is the float64 sum of ws_reduce.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <set>
#include <vector>

#include "mesh_common.hpp"

using namespace abacus;

namespace {

constexpr int WS_MIN_N = 4, WS_MAX_N = 1024, WS_MAX_ROUNDS = 32, WS_MAX_JUMPS = 40;
constexpr unsigned int WS_NONE32 = 0xffffffffu;
constexpr unsigned long long WS_NONE64 = ~0ull;

struct WsMesh {   // n * n rows of `pitch` floats
    const float *v;
    int64_t pitch;
    int n;
};

__device__ __forceinline__ unsigned int ws_fkey(float v) {   // fkey of pairs_common.hpp: an order-preserving integer image
    const unsigned int u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
static inline float host_funkey(unsigned int k) {
    const unsigned int u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

__device__ __forceinline__ float ws_value(const WsMesh &m, int x, int y, int z) {   // -0.0 is +0.0
    const float v = m.v[((int64_t)x * m.n + y) * m.pitch + z];
    return v == 0.f ? 0.f : v;
}
__device__ __forceinline__ unsigned long long ws_key(const WsMesh &m, int x, int y, int z) {
    return (unsigned long long)ws_fkey(ws_value(m, x, y, z)) << 32 | (unsigned int)((x * m.n + y) * m.n + z);
}
__device__ __forceinline__ int ws_wrap(int c, int n) { return c < 0 ? c + n : (c >= n ? c - n : c); }
__device__ __forceinline__ void ws_xyz(int f, int n, int &x, int &y, int &z) {
    const int t = f / n;
    z = f - t * n, x = t / n, y = t - x * n;
}

// f(x', y', z') for the periodic neighbours of (x, y, z): the faces (CONN 6) or the faces, edges and corners (26); FORWARD: the half
// whose offset follows (0, 0, 0) in the order of (dx, dy, dz), so that a walk over all cells meets every adjacent pair once
template <int CONN, bool FORWARD, class F>
__device__ __forceinline__ void ws_neighbours(int x, int y, int z, int n, F &&f) {
#pragma unroll
    for (int k = 0; k < 27; k++) {
        const int dx = k / 9 - 1, dy = k / 3 % 3 - 1, dz = k % 3 - 1;
        if (k == 13 || (FORWARD && k < 13)) continue;
        if (CONN == 6 && dx * dx + dy * dy + dz * dz != 1) continue;
        f(ws_wrap(x + dx, n), ws_wrap(y + dy, n), ws_wrap(z + dz, n));
    }
}

// ----------------------------------------------------------------------------------------------------------------- zones
template <int CONN>
__global__ __launch_bounds__(BLK) void ws_descend(WsMesh m, int total, unsigned int *__restrict__ down) {
    const int n = m.n;
    for (int f = blockIdx.x * BLK + threadIdx.x; f < total; f += gridDim.x * BLK) {
        int x, y, z;
        ws_xyz(f, n, x, y, z);
        unsigned long long best = ws_key(m, x, y, z);
        ws_neighbours<CONN, false>(x, y, z, n, [&](int a, int b, int c) { best = min(best, ws_key(m, a, b, c)); });
        down[f] = (unsigned int)best;
    }
}

// one pass of pointer jumping; *changed = 1 when a pointer moved
__global__ __launch_bounds__(BLK) void ws_jump(unsigned int *lab, int total, unsigned int *__restrict__ changed) {
    bool any = false;
    for (int f = blockIdx.x * BLK + threadIdx.x; f < total; f += gridDim.x * BLK) {
        const unsigned int p = lab[f];
        if (p >= (unsigned int)total) continue;   // (never: the guard keeps the next load inside the array)
        const unsigned int q = lab[p];
        if (q != p && q < (unsigned int)total) lab[f] = q, any = true;
    }
    if (any) *changed = 1u;
}

__global__ __launch_bounds__(BLK) void ws_mark(const unsigned int *__restrict__ lab, int total, unsigned int *__restrict__ flag) {
    for (int f = blockIdx.x * BLK + threadIdx.x; f < total; f += gridDim.x * BLK) flag[f] = lab[f] == (unsigned int)f ? 1u : 0u;
}

// lab[f]: the core's flat index -> the zone's number; a core writes its zone's cell and keyed value
__global__ __launch_bounds__(BLK) void ws_number(WsMesh m, unsigned int *lab, const int64_t *__restrict__ start, int total, int nz,
                                                 unsigned int *__restrict__ corecell, float *__restrict__ dmin) {
    for (int f = blockIdx.x * BLK + threadIdx.x; f < total; f += gridDim.x * BLK) {
        const unsigned int c = lab[f];
        if (c >= (unsigned int)total) continue;   // (never)
        const int64_t zone = start[c];
        if (zone < 0 || zone >= nz) continue;     // (never)
        lab[f] = (unsigned int)zone;
        if (c == (unsigned int)f) {
            int x, y, z;
            ws_xyz(f, m.n, x, y, z);
            corecell[zone] = (unsigned int)f;
            dmin[zone] = ws_value(m, x, y, z);
        }
    }
}

// acc[zone][4]: ncell and the sums of the minimum-image offsets from the core per axis (two's complement); dsum[zone]
template <bool COMBINE>
__global__ __launch_bounds__(BLK) void ws_reduce(WsMesh m, const int *__restrict__ labels, const unsigned int *__restrict__ corecell, int total,
                                                 int nz, unsigned long long *__restrict__ acc, double *__restrict__ dsum) {
    const int n = m.n, lane = threadIdx.x & 63;
    for (int f0 = blockIdx.x * BLK; f0 < total; f0 += gridDim.x * BLK) {   // the same trips for every lane: the ballots are over the wave
        const int f = f0 + threadIdx.x;
        int zone = -1, cnt = 0, ox = 0, oy = 0, oz = 0;
        double v = 0.0;
        if (f < total) {
            zone = labels[f];
            if ((unsigned int)zone >= (unsigned int)nz) zone = -1;   // (never)
        }
        if (zone >= 0) {
            const unsigned int core = corecell[zone];
            if (core < (unsigned int)total) {
                int x, y, z, cx, cy, cz;
                ws_xyz(f, n, x, y, z);
                ws_xyz((int)core, n, cx, cy, cz);
                ox = x - cx, oy = y - cy, oz = z - cz;
                ox += ox < 0 ? n : 0, oy += oy < 0 ? n : 0, oz += oz < 0 ? n : 0;
                ox -= ox >= n / 2 ? n : 0, oy -= oy >= n / 2 ? n : 0, oz -= oz >= n / 2 ? n : 0;
                v = (double)m.v[((int64_t)x * n + y) * m.pitch + z];
                cnt = 1;
            } else {
                zone = -1;   // (never)
            }
        }
        bool last = zone >= 0;
        if (COMBINE) {
            const int before = __shfl_up(zone, 1, 64);
            const unsigned long long heads = __builtin_amdgcn_ballot_w64(lane == 0 || before != zone);
            const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
            const int first = 63 - __clzll((long long)(heads & upto));   // the head of this lane's run (bit 0 is set: lane 0 is a head)
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int c1 = __shfl_up(cnt, d, 64), x1 = __shfl_up(ox, d, 64), y1 = __shfl_up(oy, d, 64), z1 = __shfl_up(oz, d, 64);
                const double v1 = __shfl_up(v, d, 64);
                if (lane - d >= first) cnt += c1, ox += x1, oy += y1, oz += z1, v += v1;
            }
            last = zone >= 0 && (lane == 63 || ((heads >> (lane + 1)) & 1ull));   // the run's last lane holds its sums
        }
        if (last) {
            unsigned long long *a = acc + 4 * (size_t)zone;
            atomicAdd(a, (unsigned long long)cnt);
            if (ox) atomicAdd(a + 1, (unsigned long long)(long long)ox);
            if (oy) atomicAdd(a + 2, (unsigned long long)(long long)oy);
            if (oz) atomicAdd(a + 3, (unsigned long long)(long long)oz);
            atomicAdd(dsum + zone, v);
        }
    }
}

// ----------------------------------------------------------------------------------------------------------------- the saddle tree
// the root above s as this thread sees it.  p < s at every step: a value that does not descend ends the walk (mst_find)
__device__ __forceinline__ unsigned int ws_find(const unsigned int *parent, unsigned int s) {
    for (;;) {
        const unsigned int p = parent[s];
        if (p >= s) return s;
        s = p;
    }
}

// mst_unite
__device__ __forceinline__ void ws_unite(unsigned int *parent, unsigned int a, unsigned int b) {
    a = ws_find(parent, a), b = ws_find(parent, b);
    while (a != b) {
        const unsigned int hi = max(a, b), lo = min(a, b);
        const unsigned int old = atomicCAS(&parent[hi], hi, lo);
        if (old >= hi) return;       // == hi: hooked (> hi cannot be)
        a = ws_find(parent, old);    // hi was hooked under old < hi meanwhile: both indices are below hi now
        b = lo;
    }
}

__global__ __launch_bounds__(BLK) void ws_init(unsigned int *__restrict__ parent, unsigned int *__restrict__ root, unsigned long long *__restrict__ slot1,
                                               unsigned long long *__restrict__ slot2, int nz) {
    for (int s = blockIdx.x * BLK + threadIdx.x; s < nz; s += gridDim.x * BLK) {
        parent[s] = root[s] = (unsigned int)s;
        slot1[s] = slot2[s] = WS_NONE64;
    }
}

// TIE false: khi of every pair across two components to slot1 of both.  TIE true: klo of the pairs that match slot1 to slot2.
template <int CONN, bool TIE>
__global__ __launch_bounds__(BLK) void ws_edges(WsMesh m, const int *__restrict__ labels, const unsigned int *__restrict__ root, int total, int nz,
                                                unsigned long long *slot1, unsigned long long *slot2) {
    const int n = m.n;
    for (int f = blockIdx.x * BLK + threadIdx.x; f < total; f += gridDim.x * BLK) {
        const int zc = labels[f];
        if ((unsigned int)zc >= (unsigned int)nz) continue;   // (never)
        int x, y, z;
        ws_xyz(f, n, x, y, z);
        unsigned int rc = WS_NONE32;
        unsigned long long kc = 0;
        ws_neighbours<CONN, true>(x, y, z, n, [&](int a, int b, int c) {
            const int zd = labels[(a * n + b) * n + c];
            if (zd == zc || (unsigned int)zd >= (unsigned int)nz) return;
            if (rc == WS_NONE32) rc = root[zc], kc = ws_key(m, x, y, z);
            const unsigned int rd = root[zd];
            if (rd == rc || rd >= (unsigned int)nz || rc >= (unsigned int)nz) return;   // (r < nz always: the guards keep the atomics inside the arrays)
            const unsigned long long kd = ws_key(m, a, b, c);
            const unsigned long long khi = max(kc, kd), klo = min(kc, kd);
            if (!TIE) {
                if (slot1[rc] > khi) atomicMin(&slot1[rc], khi);
                if (slot1[rd] > khi) atomicMin(&slot1[rd], khi);
            } else {
                if (slot1[rc] == khi && slot2[rc] > klo) atomicMin(&slot2[rc], klo);
                if (slot1[rd] == khi && slot2[rd] > klo) atomicMin(&slot2[rd], klo);
            }
        });
    }
}

// Every block takes whole waves' worth of consecutive zones: the emitted edges of a wave take their places by one atomic.
// *nedges: edges so far
__global__ __launch_bounds__(BLK) void ws_hook(const int *__restrict__ labels, int total, const unsigned int *__restrict__ root, int nz,
                                               const unsigned long long *__restrict__ slot1, const unsigned long long *__restrict__ slot2,
                                               unsigned int *parent, unsigned long long *__restrict__ e_hi, unsigned long long *__restrict__ e_lo,
                                               int *__restrict__ e_zh, int *__restrict__ e_zl, unsigned long long *__restrict__ nedges) {
    const int lane = threadIdx.x & 63;
    for (int r0 = blockIdx.x * BLK; r0 < nz; r0 += gridDim.x * BLK) {
        const int r = r0 + threadIdx.x;
        bool chose = false, emit = false;
        unsigned long long k1 = WS_NONE64, k2 = WS_NONE64;
        unsigned int rp = 0;
        int zh = 0, zl = 0;
        if (r < nz && root[r] == (unsigned int)r) {
            k1 = slot1[r], k2 = slot2[r];
            const unsigned int hi = (unsigned int)k1, lo = (unsigned int)k2;
            if (k1 != WS_NONE64 && k2 != WS_NONE64 && hi < (unsigned int)total && lo < (unsigned int)total) {
                zh = labels[hi], zl = labels[lo];
                if ((unsigned int)zh < (unsigned int)nz && (unsigned int)zl < (unsigned int)nz) {
                    const unsigned int rh = root[zh], rl = root[zl];
                    rp = rh == (unsigned int)r ? rl : rh;
                    if ((rh == (unsigned int)r || rl == (unsigned int)r) && rp < (unsigned int)nz && rp != (unsigned int)r) {
                        chose = true;
                        const bool mutual = slot1[rp] == k1 && slot2[rp] == k2;   // r' chose this very edge
                        emit = !(mutual && (unsigned int)r > rp);
                    }
                }
            }
        }
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(emit);
        if (mask) {
            unsigned long long at = 0;
            if (lane == 0) at = atomicAdd(nedges, (unsigned long long)__popcll(mask));
            at = __shfl(at, 0, 64) + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
            if (emit && at < (unsigned long long)nz) {   // (a tree has fewer than nz edges: the guard keeps the stores inside the arrays)
                e_hi[at] = k1, e_lo[at] = k2;
                e_zh[at] = zh, e_zl[at] = zl;
            }
        }
        if (chose) ws_unite(parent, (unsigned int)r, rp);
    }
}

// root[s]: the old root's root now; the slots back to none
__global__ __launch_bounds__(BLK) void ws_flatten(const unsigned int *__restrict__ parent, unsigned int *__restrict__ root,
                                                  unsigned long long *__restrict__ slot1, unsigned long long *__restrict__ slot2, int nz) {
    for (int s = blockIdx.x * BLK + threadIdx.x; s < nz; s += gridDim.x * BLK) {
        const unsigned int r = root[s];
        root[s] = r < (unsigned int)nz ? ws_find(parent, r) : (unsigned int)s;
        slot1[s] = slot2[s] = WS_NONE64;
    }
}

struct WsEdge {
    unsigned long long khi, klo;
    int zh, zl;
};

struct WsHandle {
    int n = 0, conn = 0;
    bool ran = false;
    int64_t nzones = 0;
    int rounds = 0, jumps = 0;
    std::vector<WsEdge> edges;               // ascending in (khi, klo)
    DevBuf lab, flag, start, scan, words, corecell, dmin, acc, dsum, parent, root, slot1, slot2, e_hi, e_lo, e_zh, e_zl;
    void release() {
        for (DevBuf *b : {&lab, &flag, &start, &scan, &words, &corecell, &dmin, &acc, &dsum, &parent, &root, &slot1, &slot2, &e_hi, &e_lo, &e_zh, &e_zl})
            (void)b->release();
    }
};
std::set<WsHandle *> g_handles;              // the live ones: a freed or foreign pointer is refused, not followed

unsigned int ws_grid(int64_t items) { return (unsigned int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(items, BLK), 1 << 16)); }

int check_n(const char *who, int n) {
    if (n < WS_MIN_N || n > WS_MAX_N) return fail("%s: mesh size %d out of range (%d .. %d)", who, n, WS_MIN_N, WS_MAX_N);
    if (n & 1) return fail("%s: odd mesh size %d", who, n);
    return 0;
}

WsHandle *live_handle(const char *who, abacus_ws *handle) {
    WsHandle *h = reinterpret_cast<WsHandle *>(handle);
    if (!g_handles.count(h)) {
        (void)fail("%s: the handle is not a live one of abacus_ws_create (freed already?)", who);
        return nullptr;
    }
    return h;
}

int run_body(WsHandle *h, const float *mesh, int pitch) {
    static const char *who = "abacus_ws_run_dev";
    const int n = h->n, total = n * n * n;
    const bool c26 = h->conn == 26;
    const WsMesh m{mesh, (int64_t)pitch, n};
    const dim3 cells(ws_grid(total)), blk(BLK);
    h->ran = false, h->nzones = 0, h->rounds = 0, h->jumps = 0;
    h->edges.clear();
    ABACUS_TRY(h->lab.reserve((size_t)total * 4));
    ABACUS_TRY(h->flag.reserve((size_t)total * 4));
    ABACUS_TRY(h->start.reserve((size_t)(total + 1) * sizeof(int64_t)));
    ABACUS_TRY(h->words.reserve(16));
    unsigned int *lab = h->lab.as<unsigned int>(), *flag = h->flag.as<unsigned int>(), *changed = h->words.as<unsigned int>();
    unsigned long long *nedges = h->words.as<unsigned long long>() + 1;
    int64_t *start = h->start.as<int64_t>();

    // the zones
    if (c26) ABACUS_LAUNCH("ws_descend", (ws_descend<26>), cells, blk, 0, m, total, lab);
    else ABACUS_LAUNCH("ws_descend", (ws_descend<6>), cells, blk, 0, m, total, lab);
    for (;;) {
        if (h->jumps >= WS_MAX_JUMPS) return fail("%s: the labels still move after %d passes of pointer jumping", who, WS_MAX_JUMPS);
        HIP_TRY(hipMemsetAsync(changed, 0, sizeof(unsigned int), stream()));
        ABACUS_LAUNCH("ws_jump", ws_jump, cells, blk, 0, lab, total, changed);
        unsigned int moved = 0;
        HIP_TRY(hipMemcpyAsync(&moved, changed, sizeof moved, hipMemcpyDeviceToHost, stream()));
        HIP_TRY(hipStreamSynchronize(stream()));
        h->jumps++;
        if (!moved) break;
    }
    ABACUS_LAUNCH("ws_mark", ws_mark, cells, blk, 0, (const unsigned int *)lab, total, flag);
    ABACUS_TRY(exclusive_scan_u32(flag, total, start, h->scan, 0));
    int64_t nz64 = 0;
    HIP_TRY(hipMemcpyAsync(&nz64, start + total, sizeof nz64, hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipStreamSynchronize(stream()));
    if (nz64 < 1 || nz64 > total) return fail("%s: %lld zones among %d cells", who, (long long)nz64, total);
    const int nz = (int)nz64;
    const size_t z4 = (size_t)nz * 4, z8 = (size_t)nz * 8;
    ABACUS_TRY(h->corecell.reserve(z4));
    ABACUS_TRY(h->dmin.reserve(z4));
    ABACUS_TRY(h->acc.reserve(4 * z8));
    ABACUS_TRY(h->dsum.reserve(z8));
    unsigned int *corecell = h->corecell.as<unsigned int>();
    HIP_TRY(hipMemsetAsync(corecell, 0xff, z4, stream()));
    HIP_TRY(hipMemsetAsync(h->acc.p, 0, 4 * z8, stream()));
    HIP_TRY(hipMemsetAsync(h->dsum.p, 0, z8, stream()));
    ABACUS_LAUNCH("ws_number", ws_number, cells, blk, 0, m, lab, (const int64_t *)start, total, nz, corecell, h->dmin.as<float>());
    const int *labels = h->lab.as<int>();
    if (option("ws_reduce_per_cell"))
        ABACUS_LAUNCH("ws_reduce", (ws_reduce<false>), cells, blk, 0, m, labels, (const unsigned int *)corecell, total, nz,
                      h->acc.as<unsigned long long>(), h->dsum.as<double>());
    else
        ABACUS_LAUNCH("ws_reduce", (ws_reduce<true>), cells, blk, 0, m, labels, (const unsigned int *)corecell, total, nz,
                      h->acc.as<unsigned long long>(), h->dsum.as<double>());
    h->nzones = nz;

    // the saddle tree
    if (nz > 1) {
        ABACUS_TRY(h->parent.reserve(z4));
        ABACUS_TRY(h->root.reserve(z4));
        ABACUS_TRY(h->slot1.reserve(z8));
        ABACUS_TRY(h->slot2.reserve(z8));
        ABACUS_TRY(h->e_hi.reserve(z8));
        ABACUS_TRY(h->e_lo.reserve(z8));
        ABACUS_TRY(h->e_zh.reserve(z4));
        ABACUS_TRY(h->e_zl.reserve(z4));
        unsigned int *parent = h->parent.as<unsigned int>(), *root = h->root.as<unsigned int>();
        unsigned long long *slot1 = h->slot1.as<unsigned long long>(), *slot2 = h->slot2.as<unsigned long long>();
        const dim3 zones(ws_grid(nz));
        HIP_TRY(hipMemsetAsync(nedges, 0, sizeof(unsigned long long), stream()));
        ABACUS_LAUNCH("ws_init", ws_init, zones, blk, 0, parent, root, slot1, slot2, nz);
        unsigned long long edges = 0;
        for (int round = 0; edges + 1 < (unsigned long long)nz; round++) {
            if (round >= WS_MAX_ROUNDS) return fail("%s: the zones still merge after %d rounds", who, WS_MAX_ROUNDS);
            if (c26) {
                ABACUS_LAUNCH("ws_edge_min", (ws_edges<26, false>), cells, blk, 0, m, labels, (const unsigned int *)root, total, nz, slot1, slot2);
                ABACUS_LAUNCH("ws_edge_tie", (ws_edges<26, true>), cells, blk, 0, m, labels, (const unsigned int *)root, total, nz, slot1, slot2);
            } else {
                ABACUS_LAUNCH("ws_edge_min", (ws_edges<6, false>), cells, blk, 0, m, labels, (const unsigned int *)root, total, nz, slot1, slot2);
                ABACUS_LAUNCH("ws_edge_tie", (ws_edges<6, true>), cells, blk, 0, m, labels, (const unsigned int *)root, total, nz, slot1, slot2);
            }
            ABACUS_LAUNCH("ws_hook", ws_hook, zones, blk, 0, labels, total, (const unsigned int *)root, nz, (const unsigned long long *)slot1,
                          (const unsigned long long *)slot2, parent, h->e_hi.as<unsigned long long>(), h->e_lo.as<unsigned long long>(),
                          h->e_zh.as<int>(), h->e_zl.as<int>(), nedges);
            ABACUS_LAUNCH("ws_flatten", ws_flatten, zones, blk, 0, (const unsigned int *)parent, root, slot1, slot2, nz);
            unsigned long long seen = 0;
            HIP_TRY(hipMemcpyAsync(&seen, nedges, sizeof seen, hipMemcpyDeviceToHost, stream()));
            HIP_TRY(hipStreamSynchronize(stream()));
            if (seen >= (unsigned long long)nz) return fail("%s: %llu edges among %d zones: not a tree", who, seen, nz);
            if (seen == edges) return fail("%s: round %d joined nothing with %llu of %d edges found: the zone graph is not connected", who, round, edges, nz - 1);
            edges = seen;
            h->rounds = round + 1;
        }
        const size_t ne = (size_t)edges;
        std::vector<unsigned long long> khi(ne), klo(ne);
        std::vector<int> zh(ne), zl(ne);
        HIP_TRY(hipMemcpyAsync(khi.data(), h->e_hi.p, ne * 8, hipMemcpyDeviceToHost, stream()));
        HIP_TRY(hipMemcpyAsync(klo.data(), h->e_lo.p, ne * 8, hipMemcpyDeviceToHost, stream()));
        HIP_TRY(hipMemcpyAsync(zh.data(), h->e_zh.p, ne * 4, hipMemcpyDeviceToHost, stream()));
        HIP_TRY(hipMemcpyAsync(zl.data(), h->e_zl.p, ne * 4, hipMemcpyDeviceToHost, stream()));
        HIP_TRY(hipStreamSynchronize(stream()));
        h->edges.resize(ne);
        for (size_t e = 0; e < ne; e++) h->edges[e] = WsEdge{khi[e], klo[e], zh[e], zl[e]};
        std::sort(h->edges.begin(), h->edges.end(),
                  [](const WsEdge &a, const WsEdge &b) { return a.khi != b.khi ? a.khi < b.khi : a.klo < b.klo; });
    }
    HIP_TRY(hipStreamSynchronize(stream()));
    h->ran = true;
    return 0;
}

}  // namespace

extern "C" {

int abacus_ws_check_memory(int n, int64_t np) {
    static const char *who = "abacus_ws_check_memory";
    ABACUS_TRY(check_n(who, n));
    if (np < 0) return fail("%s: negative particle count", who);
    ABACUS_ENTER();
    // the spectrum and the work area of one deposit and transform (three padded meshes), the packed copy and the deposit lists of the
    // particles, the labels, flags and offsets of the zone numbering (16 bytes per cell) and the worst case of the per-zone arrays:
    // 96 bytes per zone, a zone every second cell (a checkerboard under 6 neighbours)
    auto bytes_of = [=](int m) { return 3 * padded_bytes(m) + (size_t)np * 24 + (size_t)m * m * m * 64; };
    return check_memory(who, n, WS_MIN_N, bytes_of);
}

int abacus_ws_create(int n, int connectivity, abacus_ws **handle) {
    static const char *who = "abacus_ws_create";
    if (!handle) return fail("%s: null argument", who);
    *handle = nullptr;
    ABACUS_TRY(check_n(who, n));
    if (connectivity != 6 && connectivity != 26) return fail("%s: connectivity %d (6: faces, or 26: faces, edges and corners)", who, connectivity);
    std::lock_guard<std::recursive_mutex> guard(api_mutex());
    WsHandle *h = new WsHandle;
    h->n = n, h->conn = connectivity;
    g_handles.insert(h);
    *handle = reinterpret_cast<abacus_ws *>(h);
    return 0;
}

int abacus_ws_run_dev(abacus_ws *handle, const float *mesh, int pitch, int64_t *nzones, int *rounds, int *jumps) {
    static const char *who = "abacus_ws_run_dev";
    if (!handle || !mesh || !nzones) return fail("%s: null argument", who);
    if ((uintptr_t)mesh % 4) return fail("%s: the mesh is not aligned to 4 bytes", who);
    std::lock_guard<std::recursive_mutex> guard(api_mutex());   // the registry of handles is the library's state too
    WsHandle *h = live_handle(who, handle);
    if (!h) return -1;
    if (pitch < h->n) return fail("%s: pitch %d is smaller than the mesh size %d", who, pitch, h->n);
    ABACUS_ENTER();
    const int rc = run_body(h, mesh, pitch);
    if (rc != 0) {
        (void)hipStreamSynchronize(stream());
        return rc;
    }
    *nzones = h->nzones;
    if (rounds) *rounds = h->rounds;
    if (jumps) *jumps = h->jumps;
    return 0;
}

int abacus_ws_fetch_zones(abacus_ws *handle, int64_t *ncell, int32_t *core, float *delta_min, int64_t *offset_sum, double *delta_sum) {
    static const char *who = "abacus_ws_fetch_zones";
    if (!handle || !ncell || !core || !delta_min || !offset_sum || !delta_sum) return fail("%s: null argument", who);
    std::lock_guard<std::recursive_mutex> guard(api_mutex());
    WsHandle *h = live_handle(who, handle);
    if (!h) return -1;
    if (!h->ran) return fail("%s: no finished abacus_ws_run_dev on this handle", who);
    ABACUS_ENTER();
    const size_t nz = (size_t)h->nzones;
    const int n = h->n;
    std::vector<unsigned long long> acc(4 * nz);
    std::vector<unsigned int> cells(nz);
    HIP_TRY(hipMemcpyAsync(acc.data(), h->acc.p, 4 * nz * 8, hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipMemcpyAsync(cells.data(), h->corecell.p, nz * 4, hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipMemcpyAsync(delta_min, h->dmin.p, nz * 4, hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipMemcpyAsync(delta_sum, h->dsum.p, nz * 8, hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipStreamSynchronize(stream()));
    for (size_t z = 0; z < nz; z++) {
        ncell[z] = (int64_t)acc[4 * z];
        for (int a = 0; a < 3; a++) offset_sum[3 * z + a] = (int64_t)acc[4 * z + 1 + a];
        const unsigned int f = cells[z];
        core[3 * z] = (int32_t)(f / ((unsigned int)n * n)), core[3 * z + 1] = (int32_t)(f / n % n), core[3 * z + 2] = (int32_t)(f % n);
    }
    return 0;
}

int abacus_ws_fetch_tree(abacus_ws *handle, int64_t *hi_cell, int64_t *lo_cell, int32_t *zone_hi, int32_t *zone_lo, float *saddle) {
    static const char *who = "abacus_ws_fetch_tree";
    if (!handle) return fail("%s: null argument", who);
    std::lock_guard<std::recursive_mutex> guard(api_mutex());
    WsHandle *h = live_handle(who, handle);
    if (!h) return -1;
    if (!h->ran) return fail("%s: no finished abacus_ws_run_dev on this handle", who);
    if (!h->edges.empty() && (!hi_cell || !lo_cell || !zone_hi || !zone_lo || !saddle)) return fail("%s: null argument", who);
    for (size_t e = 0; e < h->edges.size(); e++) {
        const WsEdge &w = h->edges[e];
        hi_cell[e] = (int64_t)(unsigned int)w.khi, lo_cell[e] = (int64_t)(unsigned int)w.klo;
        zone_hi[e] = w.zh, zone_lo[e] = w.zl;
        saddle[e] = host_funkey((unsigned int)(w.khi >> 32));
    }
    return 0;
}

int abacus_ws_fetch_labels(abacus_ws *handle, int32_t *labels) {
    static const char *who = "abacus_ws_fetch_labels";
    if (!handle || !labels) return fail("%s: null argument", who);
    std::lock_guard<std::recursive_mutex> guard(api_mutex());
    WsHandle *h = live_handle(who, handle);
    if (!h) return -1;
    if (!h->ran) return fail("%s: no finished abacus_ws_run_dev on this handle", who);
    ABACUS_ENTER();
    HIP_TRY(hipMemcpyAsync(labels, h->lab.p, (size_t)h->n * h->n * h->n * 4, hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipStreamSynchronize(stream()));
    return 0;
}

int abacus_ws_free(abacus_ws *handle) {
    if (!handle) return 0;
    std::lock_guard<std::recursive_mutex> guard(api_mutex());
    WsHandle *h = reinterpret_cast<WsHandle *>(handle);
    if (!g_handles.erase(h)) return fail("abacus_ws_free: the handle is not a live one of abacus_ws_create (freed already?)");
    (void)hipStreamSynchronize(stream());
    h->release();
    delete h;
    return 0;
}

}  // extern "C"
