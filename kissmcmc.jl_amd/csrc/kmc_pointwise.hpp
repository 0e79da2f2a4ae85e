// kmc_pointwise.hpp -- the pointwise log-likelihood of a data density over a stored chain: l[r][j] = term(x_r, d_j) for the selected rows
// r of the chain and the observations j, reduced per observation without the [rows][observations] matrix ever existing (WAIC, the log
// pointwise predictive density), or written out for a range of observations (pw_matrix).  Compiled at run time next to kmc_data.hpp,
// as a module of its own ("pointwise:<ndim>", kmc_pointwise.hip), with the same functor F and ND / NCOLS as constants.
//
// Value contract (include/kissmcmc_hip.h), per observation j over the n selected rows in order:
//     pass 1:  M_j = max_r l[r][j] (NaN when a term is NaN),   S1_j = sum_r l[r][j]
//     pass 2:  E_j = sum_r exp(l[r][j] - M_j) (every row 0.0 when M_j == -inf),   V_j = sum_r (l[r][j] - S1_j / n)^2
// The rows are cut into nruns runs of run_len consecutive selected rows (the plan: from n and the number of observations alone).  A run
// is added up in row order from 0.0; the runs' partials are added in run order from 0.0 (pw_fold).  No atomics.
//
// Kernels:
//   pw_partials<PASS, PACKED = false> -- the transpose of data_partial_lane: one observation per lane, its d_j in registers; a wave walks
//                        one run, each row wave-uniform (scalar loads).  Grid (ceil(J / 64), ceil(nruns / kPwWaves)).
//   pw_partials<PASS, PACKED = true>  -- J < 64: with Jp the next power of two >= J a wave carries 64 / Jp runs side by side; lane l takes
//                        observation l % Jp of the run slot l / Jp, and loads its rows itself.  Grid (1, ceil(nruns / (slots kPwWaves))).
//   pw_fold_body      -- one observation per thread: the runs' partials in run order; pass 1 also writes S1 / n for pass 2.
//   pw_matrix         -- l[r][j] for the selected rows and the observations [obs_first, obs_first + obs_count): [n][obs_count], dense.
#pragma once
#include "kmc_device.hpp"

namespace kmc_pw {

constexpr int kPwWaves = 4;                      // waves per workgroup
constexpr int kPwThreads = kPwWaves * 64;

struct PwArgs {
    const double*  chain;      // [nsamples][nl][ld]
    const double*  data;       // [J][NCOLS] observations
    const int32_t* sel;        // [nsel] the selected walkers, ascending; nullptr: all nl of them
    double*        part;       // [2][nruns][J] partials of one pass
    double*        stats;      // [4][J]: M, S1, E, V
    double*        centre;     // [J]: S1 / n
    double*        out;        // pw_matrix: [n][obs_count]
    int64_t        n;          // selected rows: ordinal k is sample first + (k / nsel) * thin, walker sel[k % nsel]
    int64_t        J;
    int64_t        nl, ld, nsel;
    int64_t        first, thin;
    int64_t        run_len, nruns;
    int64_t        obs_first, obs_count;
    double         nd;         // (double)n
    int32_t        jp_log2;    // PACKED: log2 of Jp
    int32_t        pad_;
    double         p[6];       // params
};

// where ordinal k lies: the position in the list of selected walkers and the first element of its sample
struct RowCursor {
    int64_t wi;
    const double* sample;
    __device__ __forceinline__ RowCursor(const PwArgs& a, int64_t k)
    {
        const int64_t s = k / a.nsel;
        wi = k - s * a.nsel;
        sample = a.chain + (a.first + s * a.thin) * a.nl * a.ld;
    }
    __device__ __forceinline__ const double* row(const PwArgs& a) const { return sample + (a.sel ? (int64_t)a.sel[wi] : wi) * a.ld; }
    __device__ __forceinline__ void next(const PwArgs& a)
    {
        if (++wi == a.nsel) { wi = 0; sample += a.thin * a.nl * a.ld; }
    }
};

template <class F, int ND, int NCOLS, int PASS, bool PACKED>
__device__ __forceinline__ void pw_partials(const PwArgs& a)
{
    const int lane = (int)(threadIdx.x & 63);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));       // provably wave-uniform (scalar addressing below)
    const int64_t wid = (int64_t)blockIdx.y * kPwWaves + wave;
    int64_t j, run;
    if constexpr (PACKED) {
        j = lane & ((1 << a.jp_log2) - 1);
        run = (wid << (6 - a.jp_log2)) + (lane >> a.jp_log2);
    } else {
        j = (int64_t)blockIdx.x * 64 + lane;
        run = wid;
    }
    const bool live = j < a.J && run < a.nruns;
    const int64_t jl = j < a.J ? j : a.J - 1;                                          // (idle lanes hold a real observation, write nothing)
    double d[NCOLS];
#pragma unroll
    for (int c = 0; c < NCOLS; ++c) d[c] = a.data[jl * NCOLS + c];
    int64_t k0 = run * a.run_len, k1 = k0 + a.run_len < a.n ? k0 + a.run_len : a.n;
    if (run >= a.nruns) k0 = k1 = 0;
    double m = 0.0, c = 0.0;
    if constexpr (PASS == 2) { m = a.stats[jl]; c = a.centre[jl]; }
    double acc0 = PASS == 1 ? -INFINITY : 0.0, acc1 = 0.0;
    RowCursor cur(a, k0);
    for (int64_t k = k0; k < k1; ++k) {
        const double* __restrict__ row = cur.row(a);
        double x[ND];
#pragma unroll
        for (int i = 0; i < ND; ++i) x[i] = row[i];
        const double t = F::term(x, ND, d, a.p);
        if constexpr (PASS == 1) {
            acc0 = (t > acc0 || t != t) ? t : acc0;                                  // (a NaN stays: nothing is greater, and no later t replaces it)
            acc1 += t;
        } else {
            acc0 += m == -INFINITY ? 0.0 : exp(t - m);
            const double dv = t - c;
            acc1 += dv * dv;
        }
        cur.next(a);
    }
    if (live) {
        a.part[run * a.J + j] = acc0;
        a.part[(a.nruns + run) * a.J + j] = acc1;
    }
}

// one observation per thread; grid ceil(J / 256)
__device__ __forceinline__ void pw_fold_body(const PwArgs& a, int pass)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.J) return;
    double acc0 = pass == 1 ? -INFINITY : 0.0, acc1 = 0.0;
    for (int64_t r = 0; r < a.nruns; ++r) {
        const double p0 = a.part[r * a.J + j], p1 = a.part[(a.nruns + r) * a.J + j];
        if (pass == 1) acc0 = (p0 > acc0 || p0 != p0) ? p0 : acc0;
        else acc0 += p0;
        acc1 += p1;
    }
    if (pass == 1) {
        a.stats[j] = acc0;
        a.stats[a.J + j] = acc1;
        a.centre[j] = acc1 / a.nd;
    } else {
        a.stats[2 * a.J + j] = acc0;
        a.stats[3 * a.J + j] = acc1;
    }
}

// one observation of the range per lane, run_len rows per wave; grid (ceil(obs_count / 64), ceil(ceil(n / run_len) / kPwWaves))
template <class F, int ND, int NCOLS>
__device__ __forceinline__ void pw_matrix(const PwArgs& a)
{
    const int lane = (int)(threadIdx.x & 63);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t wid = (int64_t)blockIdx.y * kPwWaves + wave;
    const int64_t col = (int64_t)blockIdx.x * 64 + lane;
    const bool live = col < a.obs_count;
    const int64_t j = a.obs_first + (live ? col : a.obs_count - 1);
    const int64_t k0 = wid * a.run_len, k1 = k0 + a.run_len < a.n ? k0 + a.run_len : a.n;
    if (k0 >= a.n) return;
    double d[NCOLS];
#pragma unroll
    for (int c = 0; c < NCOLS; ++c) d[c] = a.data[j * NCOLS + c];
    RowCursor cur(a, k0);
    for (int64_t k = k0; k < k1; ++k) {
        const double* row = cur.row(a);
        double x[ND];
#pragma unroll
        for (int i = 0; i < ND; ++i) x[i] = row[i];
        const double t = F::term(x, ND, d, a.p);
        if (live) a.out[k * a.obs_count + col] = t;
        cur.next(a);
    }
}

}  // namespace kmc_pw
