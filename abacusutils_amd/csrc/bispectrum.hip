// Bispectrum of a periodic box on MI355X (gfx950): the FFT estimator of Scoccimarro 2015 (analysis/bispectrum.py).  No reference code: the arithmetic
// is stated in include/abacus_hip.h and pinned to tests/bispectrum_statement.py.  A finished padded spectrum ->
// [bk_shell_mask: every mode read once, written to the mesh of its shell and as 0 to the others, 8 + 8 nb bytes per mode] -> nb C2R in
// place -> [bk_triple: T[i][j][l] = sum_x D_i D_j D_l and G[i] = sum_x D_i^2 over the padded real meshes on the f32 matrix cores,
// float64 partial sums per workgroup] -> [bk_triple_final: the partials added in a fixed order].  No floating-point atomics.
//
// This file is compiled with -ffp-contract=off (csrc/Makefile).
#include <algorithm>
#include <cmath>
#include <vector>

#include "mesh_common.hpp"

using namespace abacus;

namespace {

constexpr int BK_MAX_SHELLS = 32;
constexpr int BK_TILE = 16;              // rows and columns of one v_mfma_f32_16x16x4_f32 tile
constexpr int BK_CHUNK = 16;             // cells of a row one wave step covers: a 16 B load per lane, four MFMA k-slices of four cells
// products an accumulator sums in float32 (the K of its MFMA chain) before it is added to its float64 sum.  At most 1024, where the error
// of an f32 chain is still 1e-7 of sum |a b|; 128 because the triangle sums cancel: in bins of few triangles sum |a b| is thousands of
// times the sum, and the noise of a chain grows with its length (tests/bispectrum_statement.py FLUSH_CELLS: B of such a bin is off by
// 3.5e-4 of the largest B at 1024 and by 2e-5 at 128, n = 24).  A flush is 64 conversions and additions against 512 MFMAs.
constexpr int BK_FLUSH_CELLS = 128;
constexpr int BK_FLUSH_CHUNKS = BK_FLUSH_CELLS / BK_CHUNK;
constexpr int BK_WAVES = BLK / 64;
constexpr int BK_GROUP_OUT = BK_TILE * 4 * 64;   // accumulator values of one tile group: 16 tiles x 4 registers x 64 lanes
constexpr int BK_MAX_GROUPS = 4;
// tile groups (block of i, of j, of l) for nb > 16: the block triples in ascending order; the host fills the rest by symmetry
__constant__ int bk_groups[BK_MAX_GROUPS][3] = {{0, 0, 0}, {0, 0, 1}, {0, 1, 1}, {1, 1, 1}};
const int bk_groups_host[BK_MAX_GROUPS][3] = {{0, 0, 0}, {0, 0, 1}, {0, 1, 1}, {1, 1, 1}};

struct BkEdges {
    float e[BK_MAX_SHELLS + 1];
};

typedef float bk_acc __attribute__((ext_vector_type(4)));

// the shell of the mode with squared mode number m2: e[b] <= dk sqrt(float32(m2)) < e[b + 1] in float32, -1 outside the edges
__device__ __forceinline__ int bk_shell(const BkEdges &ed, int nb, float dk, int m2) {
    const float k = dk * __fsqrt_rn((float)m2);
    if (!(k >= ed.e[0]) || !(k < ed.e[nb])) return -1;
    int b = 0;
    while (k >= ed.e[b + 1]) b++;
    return b;
}

// nb padded spectra from one: mesh b holds the mode (ONES: 1) inside shell b and 0 elsewhere.  One (a, b) row per wave, two
// consecutive modes (16 B) per lane and step; the floats of a row beyond its n/2 + 1 modes are not written.
template <bool ONES>
__global__ __launch_bounds__(BLK) void bk_shell_mask(const float4 *__restrict__ spec, float *const *__restrict__ out, BkEdges ed, int nb, int n,
                                                     int pitch4, float dk) {
    const int kzlen = n / 2 + 1, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t rows = (int64_t)n * n;
    for (int64_t row = (int64_t)blockIdx.x * BK_WAVES + wave; row < rows; row += (int64_t)gridDim.x * BK_WAVES) {
        const int a = fold((int)(row / n), n), b = fold((int)(row % n), n);
        const int ab2 = a * a + b * b;
        for (int c4 = lane; 2 * c4 < kzlen; c4 += 64) {   // 2 c4 + 1 <= n/2 + 1 < pitch / 2: inside the row
            const int c = 2 * c4;
            const bool two = c + 1 < kzlen;
            const int64_t q = row * pitch4 + c4;
            const float4 v = ONES ? make_float4(1.0f, 0.0f, 1.0f, 0.0f) : spec[q];
            const int s0 = bk_shell(ed, nb, dk, ab2 + c * c);
            const int s1 = two ? bk_shell(ed, nb, dk, ab2 + (c + 1) * (c + 1)) : -1;
            for (int m = 0; m < nb; m++) {
                float4 *dst = reinterpret_cast<float4 *>(out[m]) + q;
                const float4 t = make_float4(m == s0 ? v.x : 0.0f, m == s0 ? v.y : 0.0f, m == s1 ? v.z : 0.0f, m == s1 ? v.w : 0.0f);
                if (two)
                    *dst = t;
                else
                    *reinterpret_cast<float2 *>(dst) = make_float2(t.x, t.y);
            }
        }
    }
}

// T[i][j][l] = sum_x D_i(x) D_j(x) D_l(x) as a GEMM on v_mfma_f32_16x16x4_f32: S[(i, j)][l] = sum_x (D_i D_j)(x) D_l(x).  Lane
// (r = lane % 16, k = lane / 16) of a wave loads four consecutive cells 16 s + 4 k .. + 3 of mesh r (16 B); for each of the four,
// its value is the B operand B[k][l = r] as it stands, and the A operand of tile i, A[j = r][k] = D_i(x_k) D_j(x_k), is that value
// times the one lane (i, k) holds (ds_bpermute).  Tile i accumulates C_i[j][l] in four registers: 16 tiles for up to 16 meshes, no LDS
// staging.  Beyond 16 meshes (ONE = false) blockIdx.y picks a tile group (bk_groups): the blocks of 16 meshes i, j and l come from.
// A wave owns a contiguous range of the 16-cell chunks of the rows; the cells of a chunk at and beyond n (the pad columns) enter as 0.
// After BK_FLUSH_CHUNKS chunks (K = BK_FLUSH_CELLS products per accumulator) the accumulators are added to float64 sums in registers
// and cleared.  The waves of a workgroup add their sums in LDS in wave order; partial[(group, workgroup)][tile][register][lane], and
// for the diagonal groups partial_g[(group, workgroup)][r] = sum_x D_r^2 the same way.
template <bool ONE>
__global__ __launch_bounds__(BLK) void bk_triple(const float *const *__restrict__ meshes, int nb, int n, int pitch, double *__restrict__ partial,
                                                 double *__restrict__ partial_g) {
    __shared__ double lds[BK_GROUP_OUT];
    __shared__ double lds_g[BK_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, kq = lane >> 4;
    const int group = blockIdx.y;
    const int ib = bk_groups[group][0], jb = bk_groups[group][1], lb = bk_groups[group][2];
    const int ni = min(BK_TILE, nb - BK_TILE * ib);
    const float *mi = BK_TILE * ib + r < nb ? meshes[BK_TILE * ib + r] : nullptr;
    const float *mj = BK_TILE * jb + r < nb ? meshes[BK_TILE * jb + r] : nullptr;
    const float *ml = BK_TILE * lb + r < nb ? meshes[BK_TILE * lb + r] : nullptr;
    const bool diag = ib == lb;      // (then jb is the same block too)

    const int per_row = (n + BK_CHUNK - 1) / BK_CHUNK;
    const int64_t nchunk = (int64_t)n * n * per_row, nwave = (int64_t)gridDim.x * BK_WAVES;
    const int64_t per = (nchunk + nwave - 1) / nwave, c0 = min(nchunk, ((int64_t)blockIdx.x * BK_WAVES + wave) * per), c1 = min(nchunk, c0 + per);
    int64_t row = c0 / per_row;
    int s = (int)(c0 % per_row);

    bk_acc acc[BK_TILE];
    double sum[BK_TILE][4];
#pragma unroll
    for (int t = 0; t < BK_TILE; t++) {
        acc[t] = bk_acc{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int e = 0; e < 4; e++) sum[t][e] = 0.0;
    }
    float g = 0.0f;
    double gsum = 0.0;
    int pending = 0;
    const int src = (lane & 48) << 2;      // byte address of lane (0, k) for ds_bpermute

    auto load = [&](const float *m, int64_t off, int cell) {
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (m) {                           // 16 s + 4 k + 3 < 16 per_row <= pitch: inside the row
            v = *reinterpret_cast<const float4 *>(m + off);
            v.x = cell < n ? v.x : 0.0f, v.y = cell + 1 < n ? v.y : 0.0f, v.z = cell + 2 < n ? v.z : 0.0f, v.w = cell + 3 < n ? v.w : 0.0f;
        }
        return v;
    };
    auto flush = [&] {
#pragma unroll
        for (int t = 0; t < BK_TILE; t++) {
#pragma unroll
            for (int e = 0; e < 4; e++) sum[t][e] += (double)acc[t][e];
            acc[t] = bk_acc{0.0f, 0.0f, 0.0f, 0.0f};
        }
        gsum += (double)g;
        g = 0.0f;
        pending = 0;
    };

    for (int64_t c = c0; c < c1; c++) {
        const int cell = BK_CHUNK * s + 4 * kq;
        const int64_t off = row * pitch + cell;
        const float4 vj = load(mj, off, cell);
        const float4 vl = ONE ? vj : load(ml, off, cell);
        const float4 vi = ONE ? vj : load(mi, off, cell);
        const float bj[4] = {vj.x, vj.y, vj.z, vj.w}, bl[4] = {vl.x, vl.y, vl.z, vl.w}, bi[4] = {vi.x, vi.y, vi.z, vi.w};
        if (ni == BK_TILE) {
            // all 16 tiles, software-pipelined by hand: the 16 permutes of k-slice q + 1 are in flight while the 16 MFMAs of slice q
            // issue (independent accumulators, back to back); the scheduling barriers keep the compiler from pairing each MFMA with
            // the wait for its own permute again, which ran at a quarter of the MFMA rate
            float a[BK_TILE], d[BK_TILE];
#pragma unroll
            for (int t = 0; t < BK_TILE; t++) a[t] = bj[0] * __int_as_float(__builtin_amdgcn_ds_bpermute(src + 4 * t, __float_as_int(bi[0])));
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if (q < 3) {
#pragma unroll
                    for (int t = 0; t < BK_TILE; t++) d[t] = __int_as_float(__builtin_amdgcn_ds_bpermute(src + 4 * t, __float_as_int(bi[q + 1])));
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int t = 0; t < BK_TILE; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], bl[q], acc[t], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (q < 3) {
#pragma unroll
                    for (int t = 0; t < BK_TILE; t++) a[t] = bj[q + 1] * d[t];
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int t = 0; t < BK_TILE; t++)
                    if (t < ni) {
                        const float di = __int_as_float(__builtin_amdgcn_ds_bpermute(src + 4 * t, __float_as_int(bi[q])));
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(bj[q] * di, bl[q], acc[t], 0, 0, 0);
                    }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) g += bj[q] * bj[q];
        if (++pending == BK_FLUSH_CHUNKS) flush();
        if (++s == per_row) s = 0, row++;
    }
    flush();

    for (int w = 0; w < BK_WAVES; w++) {
        if (wave == w) {
#pragma unroll
            for (int t = 0; t < BK_TILE; t++)
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int q = (t * 4 + e) * 64 + lane;
                    lds[q] = w ? lds[q] + sum[t][e] : sum[t][e];
                }
        }
        __syncthreads();
    }
    lds_g[wave][lane] = gsum;
    __syncthreads();
    const int64_t slot = (int64_t)group * gridDim.x + blockIdx.x;
    for (int q = threadIdx.x; q < BK_GROUP_OUT; q += BLK) partial[slot * BK_GROUP_OUT + q] = lds[q];
    if (diag && threadIdx.x < BK_TILE) {
        double t = 0.0;
        for (int w = 0; w < BK_WAVES; w++)
            for (int k = 0; k < 4; k++) t += lds_g[w][16 * k + threadIdx.x];
        partial_g[slot * BK_TILE + threadIdx.x] = t;
    }
}

// second stage: out[group][q] = the sum over the workgroups of partial[(group, workgroup)][q], in workgroup order; `width` values per slot
__global__ __launch_bounds__(BLK) void bk_triple_final(const double *__restrict__ partial, int nblocks, int ngroups, int width,
                                                       double *__restrict__ out) {
    const int64_t total = (int64_t)ngroups * width;
    for (int64_t q = (int64_t)blockIdx.x * BLK + threadIdx.x; q < total; q += (int64_t)gridDim.x * BLK) {
        const int64_t group = q / width, e = q % width;
        double t = 0.0;
        for (int b = 0; b < nblocks; b++) t += partial[(group * nblocks + b) * width + e];
        out[q] = t;
    }
}

int bk_check_n(const char *who, int n) {
    if (n < 2 || n > 32767) return fail("%s: mesh size %d out of range (2 .. 32767)", who, n);
    if (n & 1) return fail("%s: odd mesh size %d (the half spectrum is laid out for an even mesh)", who, n);
    return 0;
}

int bk_check_nb(const char *who, int nb) {
    if (nb < 1 || nb > BK_MAX_SHELLS) return fail("%s: %d shells (1 .. %d)", who, nb, BK_MAX_SHELLS);
    return 0;
}

int bk_check_meshes(const char *who, const void *const *meshes, int nb) {
    for (int b = 0; b < nb; b++) {
        if (!meshes[b]) return fail("%s: null mesh %d", who, b);
        if ((uintptr_t)meshes[b] % 16) return fail("%s: mesh %d is not aligned to 16 bytes", who, b);
        for (int a = 0; a < b; a++)
            if (meshes[a] == meshes[b]) return fail("%s: meshes %d and %d are the same buffer", who, a, b);
    }
    return 0;
}

}  // namespace

extern "C" {

int abacus_bk_check_memory(int n, int nb, int64_t np) {
    ABACUS_TRY(bk_check_n("abacus_bk_check_memory", n));
    ABACUS_TRY(bk_check_nb("abacus_bk_check_memory", nb));
    if (np < 0) return fail("abacus_bk_check_memory: negative particle count");
    ABACUS_ENTER();
    // the nb shell meshes, the spectrum, the two work meshes of an interlaced deposit + transform (or the work area of a C2R), the
    // packed copy of the particles and the lists of the deposit (about one position's worth again)
    return check_memory("abacus_bk_check_memory", n, 2, [=](int m) { return (size_t)(nb + 3) * padded_bytes(m) + (size_t)np * 24; });
}

int abacus_bk_shells_dev(const void *spec_padded, int n, double Lbox, const double *kedges, int nb, float *const *meshes) {
    static const char *who = "abacus_bk_shells_dev";
    if (!kedges || !meshes) return fail("%s: null argument", who);
    ABACUS_TRY(bk_check_n(who, n));
    ABACUS_TRY(bk_check_nb(who, nb));
    if (!(Lbox > 0) || !std::isfinite(Lbox)) return fail("%s: Lbox must be positive", who);
    const float dk = (float)(2.0 * M_PI / Lbox);
    BkEdges ed;
    for (int b = 0; b <= nb; b++) {
        if (!std::isfinite(kedges[b]) || !(kedges[b] > 0)) return fail("%s: edge %d must be finite and positive", who, b);
        ed.e[b] = (float)kedges[b];
        if (b && !(ed.e[b] > ed.e[b - 1])) return fail("%s: the edges must increase (in float32)", who);
    }
    for (int b = nb + 1; b <= BK_MAX_SHELLS; b++) ed.e[b] = INFINITY;
    // the rule with the slack of the two float32 roundings (dk and the edge), so that float64(2 pi / L) n / 3 passes; and what it stands
    // for, exactly: the first mode number at or beyond n / 3 on an axis is in no shell (|k| is monotonic in the squared mode number)
    const int mc = (n + 2) / 3;
    if (!((double)ed.e[nb] <= (double)dk * n / 3.0 * (1.0 + 0x1p-22)) || !(dk * sqrtf((float)((int64_t)mc * mc)) >= ed.e[nb]))
        return fail("%s: the top edge %g lies above dk n / 3 = %g: the sums over the mesh would close triangles modulo n", who, kedges[nb],
                    (double)dk * n / 3.0);
    ABACUS_TRY(bk_check_meshes(who, (const void *const *)meshes, nb));
    for (int b = 0; b < nb; b++)
        if (meshes[b] == spec_padded) return fail("%s: mesh %d is the spectrum", who, b);
    if (spec_padded && (uintptr_t)spec_padded % 16) return fail("%s: the spectrum is not aligned to 16 bytes", who);
    ABACUS_ENTER();
    Scratch sc;
    float **table = nullptr;
    ABACUS_TRY(sc.get(&table, (size_t)nb * sizeof(float *)));
    HIP_TRY(hipMemcpyAsync(table, meshes, (size_t)nb * sizeof(float *), hipMemcpyHostToDevice, stream()));
    const dim3 grid(grid_for(ceil_div((int64_t)n * n, BK_WAVES), 16)), block(BLK);
    if (spec_padded)
        ABACUS_LAUNCH("bk_shell_mask", (bk_shell_mask<false>), grid, block, 0, (const float4 *)spec_padded, (float *const *)table, ed, nb, n,
                      pitch_r(n) / 4, dk);
    else
        ABACUS_LAUNCH("bk_shell_mask", (bk_shell_mask<true>), grid, block, 0, (const float4 *)nullptr, (float *const *)table, ed, nb, n,
                      pitch_r(n) / 4, dk);
    for (int b = 0; b < nb; b++) ABACUS_TRY(c2r_inplace(meshes[b], n));
    HIP_TRY(hipStreamSynchronize(stream()));        // `meshes` is the caller's host array
    return 0;
}

int abacus_bk_triple_dev(const float *const *meshes, int n, int nb, double *T_host, double *G_host) {
    static const char *who = "abacus_bk_triple_dev";
    if (!meshes || !T_host || !G_host) return fail("%s: null argument", who);
    ABACUS_TRY(bk_check_n(who, n));
    ABACUS_TRY(bk_check_nb(who, nb));
    ABACUS_TRY(bk_check_meshes(who, (const void *const *)meshes, nb));
    ABACUS_ENTER();
    const bool one = nb <= BK_TILE;
    const int ngroups = one ? 1 : BK_MAX_GROUPS;
    const int64_t nchunk = (int64_t)n * n * ceil_div(n, BK_CHUNK);
    // persistent workgroups: one per CU over all groups, a wave per SIMD (the accumulators and their float64 sums leave room for one)
    const unsigned int gx = std::max(1u, grid_for(ceil_div(nchunk, BK_WAVES) * ngroups, 1) / ngroups);
    Scratch sc;
    const float **table = nullptr;
    double *partial = nullptr, *partial_g = nullptr, *out = nullptr;
    const size_t nslot = (size_t)ngroups * gx;
    ABACUS_TRY(sc.get(&table, (size_t)nb * sizeof(float *)));
    ABACUS_TRY(sc.get(&partial, nslot * BK_GROUP_OUT * sizeof(double)));
    ABACUS_TRY(sc.get(&partial_g, nslot * BK_TILE * sizeof(double)));
    ABACUS_TRY(sc.get(&out, (size_t)ngroups * (BK_GROUP_OUT + BK_TILE) * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(table, meshes, (size_t)nb * sizeof(float *), hipMemcpyHostToDevice, stream()));
    HIP_TRY(hipMemsetAsync(partial_g, 0, nslot * BK_TILE * sizeof(double), stream()));     // the off-diagonal groups write none
    const dim3 grid(gx, ngroups), block(BLK);
    if (one)
        ABACUS_LAUNCH("bk_triple", (bk_triple<true>), grid, block, 0, (const float *const *)table, nb, n, pitch_r(n), partial, partial_g);
    else
        ABACUS_LAUNCH("bk_triple", (bk_triple<false>), grid, block, 0, (const float *const *)table, nb, n, pitch_r(n), partial, partial_g);
    double *out_g = out + (size_t)ngroups * BK_GROUP_OUT;
    ABACUS_LAUNCH("bk_triple_final", bk_triple_final, dim3((unsigned int)ceil_div((int64_t)ngroups * BK_GROUP_OUT, BLK)), block, 0,
                  (const double *)partial, (int)gx, ngroups, BK_GROUP_OUT, out);
    ABACUS_LAUNCH("bk_triple_final", bk_triple_final, dim3(1), block, 0, (const double *)partial_g, (int)gx, ngroups, BK_TILE, out_g);
    std::vector<double> host((size_t)ngroups * (BK_GROUP_OUT + BK_TILE));
    HIP_TRY(hipMemcpyAsync(host.data(), out, host.size() * sizeof(double), hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipStreamSynchronize(stream()));
    // C_i[j][l] of a tile lies in lane l % 16 + 16 (j / 4), register j % 4.  A triple whose blocks are not in ascending order is the
    // computed one with its indices sorted by block (the sums are symmetric); within a block every order is computed.
    auto value = [&](int i, int j, int l) {
        if (i / BK_TILE > j / BK_TILE) std::swap(i, j);
        if (j / BK_TILE > l / BK_TILE) std::swap(j, l);
        if (i / BK_TILE > j / BK_TILE) std::swap(i, j);
        int group = 0;
        for (int g = 0; g < ngroups; g++)
            if (bk_groups_host[g][0] == i / BK_TILE && bk_groups_host[g][1] == j / BK_TILE && bk_groups_host[g][2] == l / BK_TILE) group = g;
        const int jj = j % BK_TILE, ll = l % BK_TILE;
        return host[(size_t)group * BK_GROUP_OUT + ((i % BK_TILE) * 4 + jj % 4) * 64 + ll + 16 * (jj / 4)];
    };
    for (int i = 0; i < nb; i++)
        for (int j = 0; j < nb; j++)
            for (int l = 0; l < nb; l++) T_host[((size_t)i * nb + j) * nb + l] = value(i, j, l);
    const double *hg = host.data() + (size_t)ngroups * BK_GROUP_OUT;
    for (int i = 0; i < nb; i++) G_host[i] = hg[(i / BK_TILE ? ngroups - 1 : 0) * BK_TILE + i % BK_TILE];
    return 0;
}

}  // extern "C"
