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
//   pw_weights        -- v[r][j] = exp(l[r][j] - M_j) in groups of 64 observations, [n][64] each: the series whose effective sample
//                        size is PSIS-LOO's relative efficiency.  A module of its own, "pointwise_weights:<ndim>".
//   psis_walk, psis_fold_body, psis_fit_body -- PSIS-LOO over the same walk: below, with their own contract.
#pragma once
#include "kmc_device.hpp"
#include "kmc_psis_fit.hpp"

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

// The weight series behind PSIS-LOO's relative efficiency: v[k][j] = exp(l[k][j] - M_j) for the selected rows k in row order, with M_j
// the exact maximum pass 1 left in a.stats.  IEEE rules: a column whose M_j is NaN or -inf is all NaN, l = -inf under a finite M_j gives
// 0.0, the arg-max rows exactly 1.0.  Output in groups of 64 observations aligned to the absolute index: group g holds the observations
// [64 g, 64 g + 64) as [n][64], a chain of ld = 64 the convergence kernels read where it lies; the lanes outside
// [obs_first, obs_first + obs_count) are written as 0.0.  a.out: [gridDim.x][n][64], the groups group0 .. group0 + gridDim.x - 1.
// pw_matrix's walk: one observation per lane, run_len rows per wave; grid (groups, ceil(ceil(n / run_len) / kPwWaves)).
struct WeightArgs {
    PwArgs  a;
    int64_t group0;
};

template <class F, int ND, int NCOLS>
__device__ __forceinline__ void pw_weights(const WeightArgs& q)
{
    const PwArgs& a = q.a;
    const int lane = (int)(threadIdx.x & 63);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t wid = (int64_t)blockIdx.y * kPwWaves + wave;
    const int64_t jg = (q.group0 + (int64_t)blockIdx.x) * 64 + lane;
    const bool live = jg >= a.obs_first && jg < a.obs_first + a.obs_count;
    const int64_t j = live ? jg : a.obs_first;                                         // (idle lanes hold a real observation, write 0.0)
    const int64_t k0 = wid * a.run_len, k1 = k0 + a.run_len < a.n ? k0 + a.run_len : a.n;
    if (k0 >= a.n) return;
    double d[NCOLS];
#pragma unroll
    for (int c = 0; c < NCOLS; ++c) d[c] = a.data[j * NCOLS + c];
    const double m = a.stats[j];
    double* __restrict__ out = a.out + (int64_t)blockIdx.x * a.n * 64 + lane;
    RowCursor cur(a, k0);
    for (int64_t k = k0; k < k1; ++k) {
        const double* row = cur.row(a);
        double x[ND];
#pragma unroll
        for (int i = 0; i < ND; ++i) x[i] = row[i];
        const double t = F::term(x, ND, d, a.p);
        out[k * 64] = live ? exp(t - m) : 0.0;
        cur.next(a);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// PSIS-LOO (include/kissmcmc_hip.h).  The terms are recomputed in every pass, by the walk of pw_partials over
// the runs of the same plan; a block of observations [obs_first, obs_first + obs_count) is in work at a time, and every buffer below
// is indexed by the column col = j - obs_first.  With y = l - m_j >= 0 (the negated shifted log ratio x = m_j - l) the bits of y order
// as unsigned integers, so the cut-off -- the (M + 1)-th largest x -- is the y of ascending rank M, found digit by digit.
//   psis_walk<MODE = 0>  the run's minimum of l (a NaN stays)
//   psis_walk<MODE = 1>  the run's count of each value of the current digit among the keys that agree with the digits found so far;
//                        a lane counts its own observation in its own column of LDS
//   psis_walk<MODE = 2>  x > xc_j goes to the tail through the observation's integer cursor; the others' exp(x) are summed in row order
//   psis_fold_body       one column per thread: the runs' minima / counts in run order; the last digit also gives xc_j
//   psis_fit_kernel      one workgroup per column: bitonic sort of the tail in LDS, then kmc_psis_fit.hpp
// With Mj the rank looked for is the column's own M_j; the strict tail rule keeps n_tail_j <= M_j <= M, so the stride of the tail, the
// gather's bound and the sort's length stay those of M = max_j M_j.
struct PsisArgs {
    PwArgs    a;            // obs_first / obs_count: the block in work
    double*   runval;       // [nruns][obs_count]: the runs' minima (MODE 0), then their sums outside the tail (MODE 2)
    uint32_t* counts;       // [nruns][obs_count][kSelectBins]
    double*   m;            // [obs_count]: the shift; NaN for an observation whose outputs are NaN
    uint64_t* prefix;       // [obs_count]: the digits of the cut-off's key found so far
    int64_t*  rank;         // [obs_count]: the rank still looked for among the keys that agree with prefix
    double*   xc;           // [obs_count]
    int32_t*  cursor;       // [obs_count]: entries x > xc_j met so far
    double*   tail;         // [obs_count][M]: unordered after MODE 2, ascending and padded with NaN after the fit
    double*   res;          // [4][obs_count]: elpd_loo_j, pareto_k, n_tail_j, sigma
    int32_t   M;            // the tail length; with Mj the largest of them: the stride of tail, what the fit kernel sorts
    int32_t   shift;        // of the current digit
    const int32_t* Mj;      // [obs_count]: the tail length of each observation (a per-observation r_eff); nullptr: M for all
};

// the lane's observation, run and column
template <bool PACKED>
struct PsisLane {
    int64_t j, run, col;
    bool live;
    __device__ __forceinline__ PsisLane(const PwArgs& a)
    {
        const int lane = (int)(threadIdx.x & 63);
        const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        const int64_t wid = (int64_t)blockIdx.y * kPwWaves + wave;
        if constexpr (PACKED) {
            j = lane & ((1 << a.jp_log2) - 1);
            run = (wid << (6 - a.jp_log2)) + (lane >> a.jp_log2);
        } else {
            j = a.obs_first + (int64_t)blockIdx.x * 64 + lane;
            run = wid;
        }
        col = j - a.obs_first;
        live = col >= 0 && col < a.obs_count && run < a.nruns;
        if (!live) { j = a.obs_first; col = 0; }                                       // (idle lanes hold a real observation, write nothing)
    }
};

template <class F, int ND, int NCOLS, int MODE, bool PACKED>
__device__ __forceinline__ void psis_walk(const PsisArgs& q)
{
    const PwArgs& a = q.a;
    const PsisLane<PACKED> ln(a);
    const int64_t j = ln.j, run = ln.run, col = ln.col;
    double d[NCOLS];
#pragma unroll
    for (int c = 0; c < NCOLS; ++c) d[c] = a.data[j * NCOLS + c];
    int64_t k0 = run * a.run_len, k1 = k0 + a.run_len < a.n ? k0 + a.run_len : a.n;
    if (run >= a.nruns) k0 = k1 = 0;
    __shared__ uint32_t cnt[MODE == 1 ? kmc_psis::kSelectBins : 1][kPwThreads];
    double m = 0.0, xc = 0.0, acc = MODE == 0 ? INFINITY : 0.0;
    uint64_t hi = 0;
    const int shift = q.shift;
    if constexpr (MODE >= 1) m = q.m[col];
    if constexpr (MODE == 1) {
        hi = shift + kmc_psis::kSelectBits < 64 ? q.prefix[col] >> (shift + kmc_psis::kSelectBits) : 0;
#pragma unroll
        for (int b = 0; b < kmc_psis::kSelectBins; ++b) cnt[b][threadIdx.x] = 0;
    }
    if constexpr (MODE == 2) xc = q.xc[col];
    RowCursor cur(a, k0);
    for (int64_t k = k0; k < k1; ++k) {
        const double* __restrict__ row = cur.row(a);
        double x[ND];
#pragma unroll
        for (int i = 0; i < ND; ++i) x[i] = row[i];
        const double t = F::term(x, ND, d, a.p);
        if constexpr (MODE == 0) {
            acc = (t < acc || t != t) ? t : acc;
        } else if constexpr (MODE == 1) {
            const uint64_t key = (uint64_t)__double_as_longlong(t - m);
            const uint64_t top = shift + kmc_psis::kSelectBits < 64 ? key >> (shift + kmc_psis::kSelectBits) : 0;
            if (top == hi) cnt[(key >> shift) & (kmc_psis::kSelectBins - 1)][threadIdx.x] += 1;
        } else {
            const double xr = m - t;
            if (xr > xc) {
                if (ln.live) {
                    const int32_t at = atomicAdd(&q.cursor[col], 1);
                    if (at < q.M) q.tail[col * q.M + at] = xr;
                }
            } else {
                acc += exp(xr);
            }
        }
        cur.next(a);
    }
    if (!ln.live) return;
    if constexpr (MODE == 1) {
#pragma unroll
        for (int b = 0; b < kmc_psis::kSelectBins; ++b) q.counts[(run * a.obs_count + col) * kmc_psis::kSelectBins + b] = cnt[b][threadIdx.x];
    } else {
        q.runval[run * a.obs_count + col] = acc;
    }
}

// one column per thread; grid ceil(obs_count / 256).  stage 0: after MODE 0; stage 1: after a MODE 1 pass
__device__ __forceinline__ void psis_fold_body(const PsisArgs& q, int stage)
{
    const PwArgs& a = q.a;
    const int64_t col = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= a.obs_count) return;
    if (stage == 0) {
        double acc = INFINITY;
        for (int64_t r = 0; r < a.nruns; ++r) {
            const double p = q.runval[r * a.obs_count + col];
            acc = (p < acc || p != p) ? p : acc;
        }
        q.m[col] = acc - acc == 0.0 ? acc : __builtin_nan("");                     // (NaN among the terms, or no finite minimum)
        q.prefix[col] = 0;
        q.rank[col] = q.Mj ? q.Mj[col] : q.M;
        q.cursor[col] = 0;
        return;
    }
    int64_t left = q.rank[col], below = 0;
    int digit = kmc_psis::kSelectBins - 1;
    bool found = false;
    for (int b = 0; b < kmc_psis::kSelectBins; ++b) {
        int64_t c = 0;
        for (int64_t r = 0; r < a.nruns; ++r) c += q.counts[(r * a.obs_count + col) * kmc_psis::kSelectBins + b];
        if (!found && left < below + c) { digit = b; found = true; left -= below; }
        if (!found) below += c;
    }
    const uint64_t prefix = q.prefix[col] | ((uint64_t)digit << q.shift);
    q.prefix[col] = prefix;
    q.rank[col] = found ? left : 0;
    if (q.shift == 0) {
        const double y = __longlong_as_double((long long)prefix);
        const double xr = y == 0.0 ? 0.0 : -y;
        const double m = q.m[col];
        q.xc[col] = m != m ? m : (xr > kmc_psis::kLogDblMin ? xr : kmc_psis::kLogDblMin);
    }
}

// the device's context of kmc_psis_fit.hpp
struct PsisDeviceCtx {
    double* red;            // [kFitLanes] in LDS
    template <class Fn> __device__ __forceinline__ void par(int count, Fn f)
    {
        for (int t = (int)threadIdx.x; t < count; t += kmc_psis::kFitLanes) f(t);
        __syncthreads();
    }
    template <class Fn> __device__ __forceinline__ double sum(int count, Fn f)
    {
        double acc = 0.0;
        for (int t = (int)threadIdx.x; t < count; t += kmc_psis::kFitLanes) acc += f(t);
        red[threadIdx.x] = acc;
        __syncthreads();
        for (int h = kmc_psis::kFitLanes / 2; h > 0; h >>= 1) {
            if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
            __syncthreads();
        }
        const double r = red[0];
        __syncthreads();
        return r;
    }
    __device__ __forceinline__ void set(double* arr, int i, double v) { if (threadIdx.x == 0) arr[i] = v; }
    __device__ __forceinline__ void sync() { __syncthreads(); }
};

// one workgroup of kFitLanes threads per column; grid obs_count.  sort_len: the power of two >= M (at most kMaxTail)
__device__ __forceinline__ void psis_fit_body(const PsisArgs& q, int sort_len)
{
    using namespace kmc_psis;
    const PwArgs& a = q.a;
    const int64_t col = blockIdx.x;
    const int tid = (int)threadIdx.x;
    __shared__ double xs[kMaxTail];
    __shared__ double red[kFitLanes];
    __shared__ double grid[3][kMaxGrid];
    double* tail = q.tail + col * q.M;
    const double m = q.m[col];
    if (m != m) {
        for (int t = tid; t < q.M; t += kFitLanes) tail[t] = m;
        if (tid < 4) q.res[tid * a.obs_count + col] = m;
        return;
    }
    int nt = q.cursor[col];
    const int cap = q.Mj ? q.Mj[col] : q.M;
    nt = nt < cap ? nt : cap;
    for (int t = tid; t < sort_len; t += kFitLanes) xs[t] = t < nt ? tail[t] : INFINITY;
    __syncthreads();
    for (int size = 2; size <= sort_len; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < sort_len; t += kFitLanes) {
                const int u = t ^ stride;
                if (u > t) {
                    const double p = xs[t], r = xs[u];
                    const bool up = (t & size) == 0;
                    if ((p > r) == up) { xs[t] = r; xs[u] = p; }
                }
            }
            __syncthreads();
        }
    for (int t = tid; t < q.M; t += kFitLanes) tail[t] = t < nt ? xs[t] : __builtin_nan("");   // (thread t % kFitLanes reads tail[t] back below)
    __syncthreads();
    double nontail = 0.0;
    for (int64_t r = 0; r < a.nruns; ++r) nontail += q.runval[r * a.obs_count + col];
    PsisDeviceCtx ctx{red};
    const FitScratch sc{grid[0], grid[1], grid[2]};
    const FitResult fr = psis_fit(ctx, tail, xs, nt, q.xc[col], sc);
    if (tid == 0) {
        q.res[col] = psis_elpd(m, nontail, a.n, nt, fr);
        q.res[a.obs_count + col] = fr.k;
        q.res[2 * a.obs_count + col] = (double)nt;
        q.res[3 * a.obs_count + col] = fr.sigma;
    }
}

}  // namespace kmc_pw
