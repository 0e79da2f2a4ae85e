// kmc_cov_kernels.hpp -- device kernels of the posterior covariance matrix (kmc_cov.hip): the column sums that give the mean
// (cov_mean_partials / cov_mean_fold) and the centred cross products X^T X over the selected rows, a SYRK on the double-precision matrix
// instruction v_mfma_f64_16x16x4_f64 (cov_tri_partials for up to 32 columns, cov_strip_partials beyond; cov_fold).  include/kissmcmc_hip.h
// has the definition, DESIGN.md section 4j the lane maps and the plan.  Internal.
//
// Rows.  The stored chain is [sample][walker][ld]; the rows a call walks are R = 0 .. rows - 1, row R being storage row first * nl + R,
// walker R % nl: every stored (sample >= first, walker) pair, selected or not.  A row whose walker is masked out, a row past the end and a
// column past the last are fed as zeros by a select -- never loaded, never multiplied away.  The log-densities [sample][walker] are column
// ndim of the same row.
//
// One instruction consumes 4 rows of two tiles of 16 columns: lane l supplies A = x[r0 + (l >> 4)][16 ta + (l & 15)] - mean and
// B = x[r0 + (l >> 4)][16 tb + (l & 15)] - mean, one double each, straight from the chain with one load per lane (the 16 lanes of a row
// group read 16 consecutive elements); no LDS, no transpose.  D[i][j] = sum_k A[i][k] B[k][j] accumulates the cross products of column
// 16 ta + i with column 16 tb + j, and lane l holds D[(l >> 4) + 4 reg][l & 15] in register reg = 0 .. 3 -- not the map of the f32 forms.
//
// Waves.  The rows are cut into blocks of kCovChunkRows; wave w of nwaves takes the blocks w, w + nwaves, ... and walks each 4 rows at a
// time, kCov*InFlight of those loaded before their products are issued.  nwaves comes from the row count and the column count alone
// (kmc_cov.hip), so what a wave adds, and in which order, does not depend on ld, on float or double storage, on where the chain came from
// or on the device.  A wave writes its accumulators to slots of its own; cov_fold adds the waves of an entry in a fixed order.  No
// floating-point atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kmc_chain_kernels.hpp"

namespace kmc_cov {

using namespace kmc_chain;

constexpr int kCovThreads = 256;
constexpr int kCovLanes = 64;
constexpr int kCovWaves = kCovThreads / kCovLanes;
constexpr int kCovTile = 16;                               // columns of a tile: the M and N of the instruction
constexpr int kCovBlockRows = 4;                           // rows one instruction consumes: its K
constexpr int kCovStripTiles = 8;                          // B tiles one wave keeps accumulators for, against one A tile
constexpr int kCovChunkRows = 64;                          // rows of one block of a wave
constexpr int kCovChunkBlocks = kCovChunkRows / kCovBlockRows;
constexpr int kCovTriInFlight = 8;                         // 4-row blocks loaded ahead of their products: cov_tri_partials, cov_mean_partials
constexpr int kCovStripInFlight = 2;                       // ... cov_strip_partials (up to 9 tiles a block)
constexpr int kCovTileEntries = kCovTile * kCovTile;       // 256 sums of a tile pair: 4 registers of 64 lanes
constexpr int kCovFoldWays = 16;                           // partial sums of an entry folded side by side, then added in order
constexpr int kCovMaxCols = 1024;
static_assert(kCovChunkBlocks % kCovTriInFlight == 0 && kCovChunkBlocks % kCovStripInFlight == 0, "a block of rows is walked in whole batches");
static_assert(kCovThreads == kCovFoldWays * kCovTile, "the fold kernels: 16 ways by 16 entries");

typedef double cov_d4 __attribute__((ext_vector_type(4)));

struct CovArgs {
    const void* chain;                 // [sample][nl][ld], float or double
    const double* logp;                // [sample][nl] or nullptr
    const uint8_t* mask;               // [nl] or nullptr: every walker
    double* mean;                      // [ntiles * 16], zeros past ncols
    double* part;                      // mean: [ntiles][nwaves][64]; cov: [nslots][nwaves][256]
    double* out;                       // cov_fold: [nslots][256]
    double n;                          // selected rows
    int64_t row0, rows, nl, ld;
    int32_t ndim, ncols, is_float, nwaves, ntiles;
};

__device__ inline bool cov_row_ok(const CovArgs& a, int64_t R)
{
    return R < a.rows && (a.mask == nullptr || a.mask[R % a.nl] != 0);
}

// element (row R, column c) of the selection, widened; 0.0 where there is none
__device__ inline double cov_load(const CovArgs& a, int64_t R, bool ok, int32_t c)
{
    double x = 0.0;
    if (ok) {
        if (c < a.ndim) x = chain_load(a.chain, a.is_float, (a.row0 + R) * a.ld + c);
        else if (c < a.ncols) x = a.logp[a.row0 + R];
    }
    return x;
}

// ... centred on the device's own mean; 0.0 where there is none
__device__ inline double cov_centred(const CovArgs& a, int64_t R, bool ok, int32_t c, double mu)
{
    const double d = cov_load(a, R, ok, c) - mu;
    return (ok && c < a.ncols) ? d : 0.0;
}

// ---- column sums ----
// Workgroup (blockIdx.x, blockIdx.y = tile t): wave w = 4 blockIdx.x + wave adds, per lane, the elements of its rows in row order --
// lane l: rows r0 + (l >> 4), column 16 t + (l & 15) -- part[t][w][l].  cov_mean_fold (one workgroup a tile) adds for column j the four
// row groups of a wave in order, the waves w = q, q + 16, ... in order for q = 0 .. 15 side by side, then the 16 in order, and divides by n.
__global__ __launch_bounds__(kCovThreads) void cov_mean_partials(CovArgs a)
{
    const int lane = (int)threadIdx.x & (kCovLanes - 1), wave = (int)threadIdx.x >> 6;
    const int64_t wv = (int64_t)blockIdx.x * kCovWaves + wave;
    if (wv >= a.nwaves) return;
    const int t = (int)blockIdx.y, g = lane >> 4;
    const int32_t c = kCovTile * t + (lane & 15);
    const int64_t nchunks = (a.rows + kCovChunkRows - 1) / kCovChunkRows;
    double s = 0.0;
    for (int64_t ck = wv; ck < nchunks; ck += a.nwaves) {
        const int64_t R0 = ck * kCovChunkRows + g;
#pragma unroll 1
        for (int b0 = 0; b0 < kCovChunkBlocks; b0 += kCovTriInFlight) {
            double v[kCovTriInFlight];
#pragma unroll
            for (int u = 0; u < kCovTriInFlight; ++u) {
                const int64_t R = R0 + (int64_t)kCovBlockRows * (b0 + u);
                v[u] = cov_load(a, R, cov_row_ok(a, R), c);
            }
#pragma unroll
            for (int u = 0; u < kCovTriInFlight; ++u) s += v[u];
        }
    }
    a.part[((int64_t)t * a.nwaves + wv) * kCovLanes + lane] = s;
}

__global__ __launch_bounds__(kCovThreads) void cov_mean_fold(CovArgs a)
{
    __shared__ double ways[kCovFoldWays][kCovTile];
    const int t = (int)blockIdx.x, q = (int)threadIdx.x >> 4, j = (int)threadIdx.x & 15;
    double s = 0.0;
    for (int64_t w = q; w < a.nwaves; w += kCovFoldWays) {
        const double* p = a.part + ((int64_t)t * a.nwaves + w) * kCovLanes + j;
#pragma unroll
        for (int g = 0; g < kCovLanes / kCovTile; ++g) s += p[g * kCovTile];
    }
    ways[q][j] = s;
    __syncthreads();
    if (q == 0) {
        double tot = ways[0][j];
        for (int k = 1; k < kCovFoldWays; ++k) tot += ways[k][j];
        a.mean[kCovTile * t + j] = tot / a.n;
    }
}

// ---- centred cross products ----
__device__ inline cov_d4 cov_mfma(double x, double y, cov_d4 acc)
{
    return __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, acc, 0, 0, 0);
}

__device__ inline void cov_store(const CovArgs& a, int64_t slot, int64_t wv, int lane, cov_d4 acc)
{
    double* p = a.part + (slot * a.nwaves + wv) * kCovTileEntries + lane;
#pragma unroll
    for (int r = 0; r < 4; ++r) p[r * kCovLanes] = acc[r];
}

// Up to 32 columns, NT = 1 or 2 tiles: one read of the chain for the tile pairs (0, 0), (0, 1) and (1, 1), slots 0, 1, 2.  A diagonal
// pair takes one register as both operands.
template <int NT>
__global__ __launch_bounds__(kCovThreads) void cov_tri_partials(CovArgs a)
{
    const int lane = (int)threadIdx.x & (kCovLanes - 1), wave = (int)threadIdx.x >> 6;
    const int64_t wv = (int64_t)blockIdx.x * kCovWaves + wave;
    if (wv >= a.nwaves) return;
    const int g = lane >> 4;
    const int32_t c0 = lane & 15, c1 = kCovTile + (lane & 15);
    const double m0 = a.mean[c0], m1 = NT == 2 ? a.mean[c1] : 0.0;
    const int64_t nchunks = (a.rows + kCovChunkRows - 1) / kCovChunkRows;
    cov_d4 acc00 = {0.0, 0.0, 0.0, 0.0}, acc01 = acc00, acc11 = acc00;
    for (int64_t ck = wv; ck < nchunks; ck += a.nwaves) {
        const int64_t R0 = ck * kCovChunkRows + g;
#pragma unroll 1
        for (int b0 = 0; b0 < kCovChunkBlocks; b0 += kCovTriInFlight) {
            double v0[kCovTriInFlight], v1[kCovTriInFlight];
#pragma unroll
            for (int u = 0; u < kCovTriInFlight; ++u) {
                const int64_t R = R0 + (int64_t)kCovBlockRows * (b0 + u);
                const bool ok = cov_row_ok(a, R);
                v0[u] = cov_centred(a, R, ok, c0, m0);
                if (NT == 2) v1[u] = cov_centred(a, R, ok, c1, m1);
            }
#pragma unroll
            for (int u = 0; u < kCovTriInFlight; ++u) {
                acc00 = cov_mfma(v0[u], v0[u], acc00);
                if (NT == 2) {
                    acc01 = cov_mfma(v0[u], v1[u], acc01);
                    acc11 = cov_mfma(v1[u], v1[u], acc11);
                }
            }
        }
    }
    cov_store(a, 0, wv, lane, acc00);
    if (NT == 2) {
        cov_store(a, 1, wv, lane, acc01);
        cov_store(a, 2, wv, lane, acc11);
    }
}

// More than 32 columns, ntiles tiles.  The tile pairs (ta, tb >= ta) are numbered row by row of the upper triangle, slot(ta, tb) =
// ta ntiles - ta (ta - 1) / 2 + tb - ta, and a row ta is cut into strips of up to kCovStripTiles pairs; blockIdx.y counts the strips in
// that order.  A wave keeps the accumulators of one strip and reads, per 4 rows, the A tile and the strip's B tiles (the diagonal pair,
// first of a row's first strip, takes the A register for both): the chain is read once per strip.
__global__ __launch_bounds__(kCovThreads) void cov_strip_partials(CovArgs a)
{
    constexpr int S = kCovStripTiles, U = kCovStripInFlight;
    const int lane = (int)threadIdx.x & (kCovLanes - 1), wave = (int)threadIdx.x >> 6;
    const int64_t wv = (int64_t)blockIdx.x * kCovWaves + wave;
    if (wv >= a.nwaves) return;
    int s = (int)blockIdx.y, ta = 0;
    for (;; ++ta) {
        const int cnt = (a.ntiles - ta + S - 1) / S;
        if (s < cnt) break;
        s -= cnt;
    }
    const int tb0 = ta + s * S, nb = a.ntiles - tb0 < S ? a.ntiles - tb0 : S;
    const bool diag = s == 0;
    const int64_t slot0 = (int64_t)ta * a.ntiles - (int64_t)ta * (ta - 1) / 2 + (tb0 - ta);
    const int g = lane >> 4;
    const int32_t ca = kCovTile * ta + (lane & 15);
    const double ma = a.mean[ca];
    int32_t cb[S];
    double mb[S];
#pragma unroll
    for (int j = 0; j < S; ++j) {
        const int tb = tb0 + j < a.ntiles ? tb0 + j : a.ntiles - 1;       // (j >= nb: not used, kept inside the mean)
        cb[j] = kCovTile * tb + (lane & 15);
        mb[j] = a.mean[cb[j]];
    }
    const int64_t nchunks = (a.rows + kCovChunkRows - 1) / kCovChunkRows;
    cov_d4 acc[S];
#pragma unroll
    for (int j = 0; j < S; ++j) acc[j] = cov_d4{0.0, 0.0, 0.0, 0.0};
    for (int64_t ck = wv; ck < nchunks; ck += a.nwaves) {
        const int64_t R0 = ck * kCovChunkRows + g;
#pragma unroll 1
        for (int b0 = 0; b0 < kCovChunkBlocks; b0 += U) {
            double va[U], vb[U][S];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t R = R0 + (int64_t)kCovBlockRows * (b0 + u);
                const bool ok = cov_row_ok(a, R);
                va[u] = cov_centred(a, R, ok, ca, ma);
#pragma unroll
                for (int j = 0; j < S; ++j) {
                    if (j == 0 && diag) vb[u][j] = va[u];
                    else if (j < nb) vb[u][j] = cov_centred(a, R, ok, cb[j], mb[j]);
                    else vb[u][j] = 0.0;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int j = 0; j < S; ++j)
                    if (j < nb) acc[j] = cov_mfma(va[u], vb[u][j], acc[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < S; ++j)
        if (j < nb) cov_store(a, slot0 + j, wv, lane, acc[j]);
}

// The sums of 16 entries of one tile pair: workgroup blockIdx.x = 16 slot + e0 / 16.  Thread (q, j) adds the waves w = q, q + 16, ... of
// entry e0 + j in order; the 16 ways are then added in order: a fixed order for a given nwaves.  out[slot][entry].
__global__ __launch_bounds__(kCovThreads) void cov_fold(CovArgs a)
{
    __shared__ double ways[kCovFoldWays][kCovTile];
    const int64_t slot = (int64_t)blockIdx.x / (kCovTileEntries / kCovTile);
    const int e0 = ((int)blockIdx.x % (kCovTileEntries / kCovTile)) * kCovTile;
    const int q = (int)threadIdx.x >> 4, j = (int)threadIdx.x & 15;
    double s = 0.0;
#pragma unroll 4
    for (int64_t w = q; w < a.nwaves; w += kCovFoldWays) s += a.part[(slot * a.nwaves + w) * kCovTileEntries + e0 + j];
    ways[q][j] = s;
    __syncthreads();
    if (q == 0) {
        double tot = ways[0][j];
        for (int k = 1; k < kCovFoldWays; ++k) tot += ways[k][j];
        a.out[slot * kCovTileEntries + e0 + j] = tot;
    }
}

}  // namespace kmc_cov
