// Spherical voids of a periodic mesh on MI355X (gfx950): the top-hat filter of a resident spectrum and the greedy selection of
// non-overlapping under-dense spheres (Banerjee & Dalal 2016), one level (radius) at a time from the largest radius down.  Python:
// analysis/voids.py; the arithmetic is stated in include/abacus_hip.h and pinned to the NumPy statement tests/voids_statement.py.
// replaces: nothing in the reference, which has no void finder.
//
// void_wtable / void_tophat.  The multiplier W(|k| R) depends on s = i^2 + j^2 + l^2 of the integer mode numbers alone: void_wtable
//   evaluates it in float64 for s = 0 .. 3 (n/2)^2 (the series below x = 0.1, where the closed form cancels) and rounds once to
//   float32; void_tophat reads a mode (8 bytes), one table entry (mostly from the L2: 3 MB at n = 1024) and writes the mode to the
//   second mesh.  No float32 sin / cos anywhere.
//
// The selection compares integers only.  A candidate is a cell with value < threshold (float32); its key is (fkey(value), cell) in one
//   uint64, the cell as x << 20 | y << 10 | z, which orders as the flat index does - unique, so "the smallest key among the live
//   candidates that overlap" is well defined.  Overlap of levels (i, j): the squared minimum-image distance of the two cells, an
//   integer, is below D[i][j] from the host.
//
//   bricks    the candidates of a level are binned by integer bricks: nb = n / ceil(sqrt(D[i][i])) per dimension, brick of a
//             coordinate c = c * nb / n, so every brick is at least sqrt(D) cells wide and the bricks -1, 0, +1 per dimension hold
//             every cell that can overlap (nb < 3: all bricks of that dimension, each once).  Two passes over the mesh (count, fill)
//             around the prefix scan of scan.hip; the order inside a brick is the order of arrival and decides nothing.
//   prior     the voids of earlier levels lie in a second brick grid, sized for the largest D[j][i], j < i; void_kill_prior clears the
//             candidates that overlap one.
//   rounds    void_accept: a live candidate with no live overlapping candidate of a smaller key sets its accept flag (it reads
//             `live` and the keys, writes its own flag only).  void_settle: an accepted candidate leaves `live` and appends its key
//             to the level's list; a live candidate that overlaps a flagged one leaves `live`; the rest are counted (it reads the
//             flags, writes its own `live` only).  The kernel boundary is the only synchronisation: no thread waits for another.
//             Every round accepts at least the live candidate with the globally smallest key, so at most ncand rounds run; the
//             host loop carries that guard.  The live count is read back after every round (4 bytes).
//   order     the accepted keys of a level are few: they go to the host, are sorted there and kept in the handle, which is the
//             sequential order of the statement (level, then key).
//
// Compiled with -ffp-contract=off (the default of csrc/Makefile): the only float32 operations are one product per mode component and
// comparisons; void_wtable is float64 and must stay the statement's expression.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <set>
#include <vector>

#include "mesh_common.hpp"

using namespace abacus;

namespace {

constexpr int VOID_MAX_LEVELS = 32, VOID_MIN_N = 4, VOID_MAX_N = 1024;

__device__ __forceinline__ unsigned int void_fkey(float v) {   // fkey of pairs_common.hpp: an order-preserving integer image
    const unsigned int u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
static inline float host_funkey(unsigned int k) {
    const unsigned int u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// ----------------------------------------------------------------------------------------------------------------- the filter
// table[s] = float32(W(x)), x = dkR sqrt(s) in float64: 3 (sin x - x cos x) / x^3, and 1 - x^2/10 + x^4/280 below x = 0.1
__global__ __launch_bounds__(BLK) void void_wtable(float *__restrict__ table, int count, double dkR) {
    const int s = blockIdx.x * BLK + threadIdx.x;
    if (s >= count) return;
    const double x = dkR * sqrt((double)s);
    double w;
    if (x < 0.1) {
        const double x2 = x * x;
        w = 1.0 - x2 / 10.0 + x2 * x2 / 280.0;
    } else {
        w = 3.0 * (sin(x) - x * cos(x)) / (x * x * x);
    }
    table[s] = (float)w;
}

// dst = src * table[i^2 + j^2 + l^2] over the n * n rows of n/2 + 1 modes; rows of pc float2 in both meshes.  One row per
// workgroup pass; the floats of a row beyond its modes are not written.
__global__ __launch_bounds__(BLK) void void_tophat(const float2 *__restrict__ src, float2 *__restrict__ dst, int n, int pc,
                                                   const float *__restrict__ table) {
    const int half = n / 2, nz = half + 1;
    for (int64_t row = blockIdx.x; row < (int64_t)n * n; row += gridDim.x) {
        const int i = (int)(row / n), j = (int)(row % n);
        const int fi = i < half ? i : i - n, fj = j < half ? j : j - n;
        const int sij = fi * fi + fj * fj;
        for (int l = threadIdx.x; l < nz; l += BLK) {
            const float w = table[sij + l * l];
            const float2 v = src[row * pc + l];
            dst[row * pc + l] = make_float2(v.x * w, v.y * w);
        }
    }
}

// ----------------------------------------------------------------------------------------------------------------- the selection
struct Geo {      // a mesh of n^3 cells binned into nb^3 bricks
    int n, nb;
};

// a cell as one word: x << 20 | y << 10 | z (n <= 1024).  It orders as the flat index (x n + y) n + z does, so it stands for it in the keys.
__device__ __forceinline__ unsigned int pack_xyz(int x, int y, int z) { return (unsigned int)x << 20 | (unsigned int)y << 10 | (unsigned int)z; }
__device__ __forceinline__ void cell_xyz(unsigned int cell, int &x, int &y, int &z) {
    x = (int)(cell >> 20), y = (int)(cell >> 10 & 1023u), z = (int)(cell & 1023u);
}
__device__ __forceinline__ int brick_of(int x, int y, int z, const Geo &g) {
    return ((x * g.nb / g.n) * g.nb + (y * g.nb / g.n)) * g.nb + (z * g.nb / g.n);     // c * nb < 2^20: no overflow
}
__device__ __forceinline__ int dist2(int x0, int y0, int z0, int x1, int y1, int z1, int n) {
    int dx = abs(x0 - x1), dy = abs(y0 - y1), dz = abs(z0 - z1);
    dx = min(dx, n - dx), dy = min(dy, n - dy), dz = min(dz, n - dz);
    return dx * dx + dy * dy + dz * dz;                                               // <= 3 (n/2)^2 < 2^20
}

// f(slot) over the slots of the bricks around (x, y, z): -1, 0, +1 per dimension, every brick once; f returns true to stop
template <class F>
__device__ __forceinline__ void walk(int x, int y, int z, const Geo &g, const int64_t *__restrict__ start, F &&f) {
    const int bx = x * g.nb / g.n, by = y * g.nb / g.n, bz = z * g.nb / g.n, span = min(3, g.nb);
    for (int ox = 0; ox < span; ox++) {
        const int cx = (bx + g.nb - 1 + ox) % g.nb;
        for (int oy = 0; oy < span; oy++) {
            const int cy = (by + g.nb - 1 + oy) % g.nb;
            for (int oz = 0; oz < span; oz++) {
                const int cz = (bz + g.nb - 1 + oz) % g.nb;
                const int b = (cx * g.nb + cy) * g.nb + cz;
                const int64_t s1 = start[b + 1];
                for (int64_t s = start[b]; s < s1; s++)
                    if (f(s)) return;
            }
        }
    }
}

// A cell is a candidate iff value < thr in float32: never a NaN, -inf is one.  The key: -0.0 is +0.0 first (fkey would order them).
// FILL false: counters[brick] += 1 per candidate.  FILL true: the candidate's key to slot start[brick] + counters[brick]++.
// A workgroup takes rows (x, y) of the mesh, its threads the cells along z.
template <bool FILL>
__global__ __launch_bounds__(BLK) void void_candidates(const float *__restrict__ mesh, int64_t pitch, Geo g, float thr,
                                                       unsigned int *__restrict__ counters, const int64_t *__restrict__ start,
                                                       uint64_t *__restrict__ keys) {
    const int n = g.n;
    for (int row = blockIdx.x; row < n * n; row += gridDim.x) {
        const int x = row / n, y = row % n;
        for (int z = threadIdx.x; z < n; z += BLK) {
            float v = mesh[(int64_t)row * pitch + z];
            if (!(v < thr)) continue;
            v = v == 0.f ? 0.f : v;
            const int b = brick_of(x, y, z, g);
            const unsigned int at = atomicAdd(counters + b, 1u);
            if (FILL) keys[start[b] + at] = (uint64_t)void_fkey(v) << 32 | pack_xyz(x, y, z);
        }
    }
}

// the voids of earlier levels into their brick grid: (cell, level) to slot start[brick] + counters[brick]++
template <bool FILL>
__global__ __launch_bounds__(BLK) void void_prior_bin(const unsigned int *__restrict__ vcell, const int *__restrict__ vlevel, int nv, Geo g,
                                                      unsigned int *__restrict__ counters, const int64_t *__restrict__ start,
                                                      unsigned int *__restrict__ scell, int *__restrict__ slevel) {
    const int v = blockIdx.x * BLK + threadIdx.x;
    if (v >= nv) return;
    int x, y, z;
    cell_xyz(vcell[v], x, y, z);
    const int b = brick_of(x, y, z, g);
    const unsigned int at = atomicAdd(counters + b, 1u);
    if (FILL) {
        scell[start[b] + at] = vcell[v];
        slevel[start[b] + at] = vlevel[v];
    }
}

struct Drow {     // D[level][j] of the level at work, j = 0 .. 31
    int d[VOID_MAX_LEVELS];
};

// live[r] = 0 for the candidates that overlap a void of an earlier level
__global__ __launch_bounds__(BLK) void void_kill_prior(const uint64_t *__restrict__ keys, int64_t ncand, int n, Geo gv,
                                                       const int64_t *__restrict__ vstart, const unsigned int *__restrict__ scell,
                                                       const int *__restrict__ slevel, Drow D, unsigned char *__restrict__ live) {
    const int64_t r = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (r >= ncand) return;
    int x, y, z;
    cell_xyz((unsigned int)keys[r], x, y, z);
    bool hit = false;
    walk(x, y, z, gv, vstart, [&](int64_t s) {
        int vx, vy, vz;
        cell_xyz(scell[s], vx, vy, vz);
        hit = dist2(x, y, z, vx, vy, vz, n) < D.d[slevel[s]];
        return hit;
    });
    if (hit) live[r] = 0;
}

// accept[r] = 1 for the live candidates whose key is below that of every live candidate they overlap (d2 < Dii)
__global__ __launch_bounds__(BLK) void void_accept(const uint64_t *__restrict__ keys, int64_t ncand, Geo g, const int64_t *__restrict__ start,
                                                   int Dii, const unsigned char *__restrict__ live, unsigned char *__restrict__ accept) {
    const int64_t r = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (r >= ncand || !live[r]) return;
    const uint64_t mine = keys[r];
    int x, y, z;
    cell_xyz((unsigned int)mine, x, y, z);
    bool beaten = false;
    walk(x, y, z, g, start, [&](int64_t s) {
        if (!live[s]) return false;
        const uint64_t other = keys[s];
        if (other >= mine) return false;                      // itself included
        int ox, oy, oz;
        cell_xyz((unsigned int)other, ox, oy, oz);
        beaten = dist2(x, y, z, ox, oy, oz, g.n) < Dii;
        return beaten;
    });
    if (!beaten) accept[r] = 1;
}

// an accepted candidate leaves `live` and appends its key to `taken`; a live one that overlaps an accepted one leaves `live`; the
// others are counted in *nlive.  `accept` is never cleared within a level: what an earlier round accepted has no live neighbour left.
__global__ __launch_bounds__(BLK) void void_settle(const uint64_t *__restrict__ keys, int64_t ncand, Geo g, const int64_t *__restrict__ start,
                                                   int Dii, unsigned char *__restrict__ live, const unsigned char *__restrict__ accept,
                                                   uint64_t *__restrict__ taken, unsigned int *__restrict__ ntaken,
                                                   unsigned int *__restrict__ nlive) {
    const int64_t r = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (r >= ncand || !live[r]) return;
    const uint64_t mine = keys[r];
    if (accept[r]) {
        live[r] = 0;
        taken[atomicAdd(ntaken, 1u)] = mine;                  // at most ncand entries: every candidate is accepted at most once
        return;
    }
    int x, y, z;
    cell_xyz((unsigned int)mine, x, y, z);
    bool hit = false;
    walk(x, y, z, g, start, [&](int64_t s) {
        if (!accept[s]) return false;
        int ox, oy, oz;
        cell_xyz((unsigned int)keys[s], ox, oy, oz);
        hit = dist2(x, y, z, ox, oy, oz, g.n) < Dii;
        return hit;
    });
    if (hit) live[r] = 0;
    else atomicAdd(nlive, 1u);
}

struct VoidHandle {
    int n = 0, nlevels = 0, last = -1;       // last: the highest level taken so far
    std::vector<int> D;                      // nlevels x nlevels
    std::vector<uint64_t> keys;              // the voids in output order
    std::vector<int> levels;
    DevBuf counters, start, ckeys, live, accept, taken, vcell, vlevel, vcounters, vstart, scell, slevel, words, scan;
    void release() {
        for (DevBuf *b : {&counters, &start, &ckeys, &live, &accept, &taken, &vcell, &vlevel, &vcounters, &vstart, &scell, &slevel, &words, &scan})
            (void)b->release();
    }
};
std::set<VoidHandle *> g_handles;            // the live ones: a freed or foreign pointer is refused, not followed

unsigned int grid_for(int64_t items) { return (unsigned int)std::max<int64_t>(1, ceil_div(items, BLK)); }

// bricks per dimension for a reach of sqrt(d2) cells: the widest count whose bricks are all at least ceil(sqrt(d2)) cells wide
int bricks_for(int n, int d2) {
    int side = (int)std::ceil(std::sqrt((double)d2));
    while ((int64_t)side * side < d2) side++;
    return std::max(1, n / std::max(1, side));
}

int level_body(VoidHandle *h, const float *mesh, int pitch, int level, float thr, int64_t *ncand_out, int64_t *nvoid_out, int64_t *rounds_out) {
    const int n = h->n, m = h->nlevels;
    const int Dii = h->D[(size_t)level * m + level];
    const Geo g{n, bricks_for(n, Dii)};
    const int64_t nbrick = (int64_t)g.nb * g.nb * g.nb, total = (int64_t)n * n * n;
    const unsigned int mesh_grid = (unsigned int)std::min<int64_t>((int64_t)n * n, 1 << 16);
    ABACUS_TRY(h->counters.reserve((size_t)nbrick * sizeof(unsigned int)));
    ABACUS_TRY(h->start.reserve((size_t)(nbrick + 1) * sizeof(int64_t)));
    ABACUS_TRY(h->words.reserve(2 * sizeof(unsigned int)));
    unsigned int *counters = h->counters.as<unsigned int>(), *words = h->words.as<unsigned int>();
    int64_t *start = h->start.as<int64_t>();
    HIP_TRY(hipMemsetAsync(counters, 0, (size_t)nbrick * sizeof(unsigned int), stream()));
    ABACUS_LAUNCH("void_cand_count", (void_candidates<false>), dim3(mesh_grid), dim3(BLK), 0, mesh, (int64_t)pitch, g, thr, counters,
                  (const int64_t *)nullptr, (uint64_t *)nullptr);
    ABACUS_TRY(exclusive_scan_u32(counters, nbrick, start, h->scan, 1));
    int64_t ncand = 0;
    HIP_TRY(hipMemcpyAsync(&ncand, start + nbrick, sizeof(int64_t), hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipStreamSynchronize(stream()));
    *ncand_out = ncand, *nvoid_out = 0, *rounds_out = 0;
    if (ncand == 0) return 0;
    if (ncand > total) return fail("abacus_void_level_dev: %lld candidates among %lld cells", (long long)ncand, (long long)total);

    ABACUS_TRY(h->ckeys.reserve((size_t)ncand * sizeof(uint64_t)));
    ABACUS_TRY(h->taken.reserve((size_t)ncand * sizeof(uint64_t)));
    ABACUS_TRY(h->live.reserve((size_t)ncand));
    ABACUS_TRY(h->accept.reserve((size_t)ncand));
    uint64_t *keys = h->ckeys.as<uint64_t>(), *taken = h->taken.as<uint64_t>();
    unsigned char *live = h->live.as<unsigned char>(), *accept = h->accept.as<unsigned char>();
    ABACUS_LAUNCH("void_cand_fill", (void_candidates<true>), dim3(mesh_grid), dim3(BLK), 0, mesh, (int64_t)pitch, g, thr, counters,
                  (const int64_t *)start, keys);
    HIP_TRY(hipMemsetAsync(live, 1, (size_t)ncand, stream()));
    HIP_TRY(hipMemsetAsync(accept, 0, (size_t)ncand, stream()));
    HIP_TRY(hipMemsetAsync(words, 0, 2 * sizeof(unsigned int), stream()));
    const unsigned int cand_grid = grid_for(ncand);

    // the voids of earlier levels: their own brick grid, sized for the largest reach against this level
    const int nv = (int)h->keys.size();
    if (nv > 0) {
        Drow row;
        int reach = 1;
        for (int j = 0; j < VOID_MAX_LEVELS; j++) row.d[j] = j < m ? h->D[(size_t)level * m + j] : 0;
        for (int l : h->levels) reach = std::max(reach, row.d[l]);
        const Geo gv{n, bricks_for(n, reach)};
        const int64_t nvb = (int64_t)gv.nb * gv.nb * gv.nb;
        std::vector<unsigned int> cells(nv);
        for (int v = 0; v < nv; v++) cells[v] = (unsigned int)h->keys[v];
        ABACUS_TRY(h->vcell.reserve((size_t)nv * 4));
        ABACUS_TRY(h->vlevel.reserve((size_t)nv * 4));
        ABACUS_TRY(h->scell.reserve((size_t)nv * 4));
        ABACUS_TRY(h->slevel.reserve((size_t)nv * 4));
        ABACUS_TRY(h->vcounters.reserve((size_t)nvb * sizeof(unsigned int)));
        ABACUS_TRY(h->vstart.reserve((size_t)(nvb + 1) * sizeof(int64_t)));
        unsigned int *vcounters = h->vcounters.as<unsigned int>(), *vcell = h->vcell.as<unsigned int>(), *scell = h->scell.as<unsigned int>();
        int *vlevel = h->vlevel.as<int>(), *slevel = h->slevel.as<int>();
        int64_t *vstart = h->vstart.as<int64_t>();
        HIP_TRY(hipMemcpyAsync(vcell, cells.data(), (size_t)nv * 4, hipMemcpyHostToDevice, stream()));
        HIP_TRY(hipMemcpyAsync(vlevel, h->levels.data(), (size_t)nv * 4, hipMemcpyHostToDevice, stream()));
        HIP_TRY(hipMemsetAsync(vcounters, 0, (size_t)nvb * sizeof(unsigned int), stream()));
        ABACUS_LAUNCH("void_prior_count", (void_prior_bin<false>), dim3(grid_for(nv)), dim3(BLK), 0, (const unsigned int *)vcell,
                      (const int *)vlevel, nv, gv, vcounters, (const int64_t *)nullptr, (unsigned int *)nullptr, (int *)nullptr);
        ABACUS_TRY(exclusive_scan_u32(vcounters, nvb, vstart, h->scan, 1));
        ABACUS_LAUNCH("void_prior_fill", (void_prior_bin<true>), dim3(grid_for(nv)), dim3(BLK), 0, (const unsigned int *)vcell,
                      (const int *)vlevel, nv, gv, vcounters, (const int64_t *)vstart, scell, slevel);
        ABACUS_LAUNCH("void_kill_prior", void_kill_prior, dim3(cand_grid), dim3(BLK), 0, (const uint64_t *)keys, ncand, n, gv,
                      (const int64_t *)vstart, (const unsigned int *)scell, (const int *)slevel, row, live);
        HIP_TRY(hipStreamSynchronize(stream()));   // `cells` is pageable host memory of this scope
    }

    int64_t rounds = 0;
    for (;;) {
        if (rounds > ncand) return fail("abacus_void_level_dev: %lld rounds for %lld candidates - the selection does not end", (long long)rounds, (long long)ncand);
        HIP_TRY(hipMemsetAsync(words + 1, 0, sizeof(unsigned int), stream()));
        ABACUS_LAUNCH("void_accept", void_accept, dim3(cand_grid), dim3(BLK), 0, (const uint64_t *)keys, ncand, g, (const int64_t *)start, Dii,
                      (const unsigned char *)live, accept);
        ABACUS_LAUNCH("void_settle", void_settle, dim3(cand_grid), dim3(BLK), 0, (const uint64_t *)keys, ncand, g, (const int64_t *)start, Dii,
                      live, (const unsigned char *)accept, taken, words, words + 1);
        unsigned int host[2] = {0, 0};   // taken so far, still live
        HIP_TRY(hipMemcpyAsync(host, words, sizeof(host), hipMemcpyDeviceToHost, stream()));
        HIP_TRY(hipStreamSynchronize(stream()));
        // a round in which every candidate was dead already (all killed by earlier levels) accepts nothing and is not a round
        if (rounds == 0 && host[0] == 0 && host[1] == 0) break;
        rounds++;
        if (host[1] == 0) {
            std::vector<uint64_t> got(host[0]);
            if (host[0]) {
                HIP_TRY(hipMemcpyAsync(got.data(), taken, (size_t)host[0] * sizeof(uint64_t), hipMemcpyDeviceToHost, stream()));
                HIP_TRY(hipStreamSynchronize(stream()));
            }
            std::sort(got.begin(), got.end());
            h->keys.insert(h->keys.end(), got.begin(), got.end());
            h->levels.insert(h->levels.end(), got.size(), level);
            *nvoid_out = (int64_t)got.size();
            break;
        }
    }
    *rounds_out = rounds;
    return 0;
}

}  // namespace

extern "C" {

int abacus_void_check_memory(int n, int64_t np) {
    static const char *who = "abacus_void_check_memory";
    if (n < VOID_MIN_N || n > VOID_MAX_N) return fail("%s: mesh size %d out of range (%d .. %d)", who, n, VOID_MIN_N, VOID_MAX_N);
    if (n & 1) return fail("%s: odd mesh size %d (the half spectrum is laid out for an even mesh)", who, n);
    if (np < 0) return fail("%s: negative particle count", who);
    ABACUS_ENTER();
    // the spectrum, the smoothed mesh, the work mesh of an interlaced deposit (or the work area of the C2R), the packed copy and the
    // deposit lists of the particles, and the worst case of the selection: every cell a candidate (two keys and two flags each) in
    // bricks of one cell (a counter and an offset each)
    auto bytes_of = [=](int m) { return 3 * padded_bytes(m) + (size_t)np * 24 + (size_t)m * m * m * 30; };
    return check_memory(who, n, 2, bytes_of);
}

int abacus_void_tophat_dev(const void *spec_padded, int n, double Lbox, double R, void *out_padded) {
    static const char *who = "abacus_void_tophat_dev";
    if (!spec_padded || !out_padded) return fail("%s: null argument", who);
    if (n < VOID_MIN_N || n > VOID_MAX_N) return fail("%s: mesh size %d out of range (%d .. %d)", who, n, VOID_MIN_N, VOID_MAX_N);
    if (n & 1) return fail("%s: odd mesh size %d (the half spectrum is laid out for an even mesh)", who, n);
    if (spec_padded == out_padded) return fail("%s: the spectrum and the output must be different meshes (the spectrum is kept)", who);
    if ((uintptr_t)spec_padded % 16 || (uintptr_t)out_padded % 16) return fail("%s: the meshes are not aligned to 16 bytes", who);
    if (!(Lbox > 0) || !std::isfinite(Lbox)) return fail("%s: Lbox must be positive", who);
    if (!(R >= 0) || !std::isfinite(R)) return fail("%s: R must be finite and not negative, got %g", who, R);
    ABACUS_ENTER();
    const int pc = abacus_slab_pitch(n) / 2, count = 3 * (n / 2) * (n / 2) + 1;
    void *table = nullptr;
    ABACUS_TRY(scratch_acquire(&table, (size_t)count * sizeof(float)));
    auto body = [&]() -> int {
        ABACUS_LAUNCH("void_wtable", void_wtable, dim3(grid_for(count)), dim3(BLK), 0, (float *)table, count, 2.0 * M_PI / Lbox * R);
        ABACUS_LAUNCH("void_tophat", void_tophat, dim3((unsigned int)std::min<int64_t>((int64_t)n * n, 1 << 16)), dim3(BLK), 0,
                      (const float2 *)spec_padded, (float2 *)out_padded, n, pc, (const float *)table);
        return smooth_c2r_inplace((float *)out_padded, n, Lbox, 0.0);
    };
    const int rc = body();
    scratch_release(table);    // the stream orders the next user of the block behind void_tophat
    return rc;
}

int abacus_void_create(int n, int nlevels, const int64_t *d2min_host, abacus_void **handle) {
    static const char *who = "abacus_void_create";
    if (!d2min_host || !handle) return fail("%s: null argument", who);
    if (n < VOID_MIN_N || n > VOID_MAX_N) return fail("%s: mesh size %d out of range (%d .. %d)", who, n, VOID_MIN_N, VOID_MAX_N);
    if (n & 1) return fail("%s: odd mesh size %d", who, n);
    if (nlevels < 1 || nlevels > VOID_MAX_LEVELS) return fail("%s: %d levels (1 .. %d)", who, nlevels, VOID_MAX_LEVELS);
    const int64_t dmax = (int64_t)(n / 2) * (n / 2);
    for (int i = 0; i < nlevels; i++)
        for (int j = 0; j < nlevels; j++) {
            const int64_t d = d2min_host[(size_t)i * nlevels + j];
            if (d != d2min_host[(size_t)j * nlevels + i]) return fail("%s: the table D is not symmetric at (%d, %d)", who, i, j);
            if (d < 1) return fail("%s: D[%d][%d] = %lld is not positive", who, i, j, (long long)d);
            if (d > dmax) return fail("%s: D[%d][%d] = %lld exceeds (n / 2)^2 = %lld: two radii must fit half the box", who, i, j, (long long)d, (long long)dmax);
        }
    std::lock_guard<std::recursive_mutex> guard(api_mutex());
    VoidHandle *h = new VoidHandle;
    h->n = n, h->nlevels = nlevels;
    h->D.resize((size_t)nlevels * nlevels);
    for (size_t q = 0; q < h->D.size(); q++) h->D[q] = (int)d2min_host[q];
    g_handles.insert(h);
    *handle = reinterpret_cast<abacus_void *>(h);
    return 0;
}

int abacus_void_level_dev(abacus_void *handle, const float *mesh, int pitch, int level, float threshold, int64_t *ncand, int64_t *nvoid,
                          int64_t *rounds) {
    static const char *who = "abacus_void_level_dev";
    if (!handle || !mesh || !ncand || !nvoid || !rounds) return fail("%s: null argument", who);
    if (!std::isfinite(threshold)) return fail("%s: the threshold is not finite", who);
    if ((uintptr_t)mesh % 4) return fail("%s: the mesh is not aligned to 4 bytes", who);
    std::lock_guard<std::recursive_mutex> guard(api_mutex());   // the registry of handles is the library's state too
    VoidHandle *h = reinterpret_cast<VoidHandle *>(handle);
    if (!g_handles.count(h)) return fail("%s: the handle is not a live one of abacus_void_create (freed already?)", who);
    if (pitch < h->n) return fail("%s: pitch %d is smaller than the mesh size %d", who, pitch, h->n);
    if (level < 0 || level >= h->nlevels) return fail("%s: level %d out of range (0 .. %d)", who, level, h->nlevels - 1);
    if (level <= h->last) return fail("%s: level %d after level %d - the levels are taken in increasing order, each at most once", who, level, h->last);
    ABACUS_ENTER();
    const int rc = level_body(h, mesh, pitch, level, threshold, ncand, nvoid, rounds);
    if (rc != 0) {
        (void)hipStreamSynchronize(stream());
        return rc;
    }
    h->last = level;
    return 0;
}

int abacus_void_count(abacus_void *handle, int64_t *nvoid) {
    static const char *who = "abacus_void_count";
    if (!handle || !nvoid) return fail("%s: null argument", who);
    std::lock_guard<std::recursive_mutex> guard(api_mutex());
    VoidHandle *h = reinterpret_cast<VoidHandle *>(handle);
    if (!g_handles.count(h)) return fail("%s: the handle is not a live one of abacus_void_create (freed already?)", who);
    *nvoid = (int64_t)h->keys.size();
    return 0;
}

int abacus_void_fetch(abacus_void *handle, int32_t *cells, int32_t *levels, float *deltas) {
    static const char *who = "abacus_void_fetch";
    if (!handle) return fail("%s: null argument", who);
    std::lock_guard<std::recursive_mutex> guard(api_mutex());
    VoidHandle *h = reinterpret_cast<VoidHandle *>(handle);
    if (!g_handles.count(h)) return fail("%s: the handle is not a live one of abacus_void_create (freed already?)", who);
    if (!h->keys.empty() && (!cells || !levels || !deltas)) return fail("%s: null argument", who);
    for (size_t v = 0; v < h->keys.size(); v++) {
        const unsigned int cell = (unsigned int)h->keys[v];
        cells[3 * v] = (int32_t)(cell >> 20), cells[3 * v + 1] = (int32_t)(cell >> 10 & 1023u), cells[3 * v + 2] = (int32_t)(cell & 1023u);
        levels[v] = h->levels[v];
        deltas[v] = host_funkey((unsigned int)(h->keys[v] >> 32));
    }
    return 0;
}

int abacus_void_free(abacus_void *handle) {
    if (!handle) return 0;
    std::lock_guard<std::recursive_mutex> guard(api_mutex());
    VoidHandle *h = reinterpret_cast<VoidHandle *>(handle);
    if (!g_handles.erase(h)) return fail("abacus_void_free: the handle is not a live one of abacus_void_create (freed already?)");
    (void)hipStreamSynchronize(stream());
    h->release();
    delete h;
    return 0;
}

}  // extern "C"
