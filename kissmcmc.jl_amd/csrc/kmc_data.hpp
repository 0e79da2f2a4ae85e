// kmc_data.hpp -- data densities (KMC_DATA_DENSITY): a log-prior plus a sum of per-observation log-likelihood terms over a data
// array held on the device, the model the reference's `pdf` closure (src/samplers.jl:257) almost always is.  Compiled at run time
// (kmc_rtc.hip) with the user's two function bodies as the functor F and ND (= ndim) / NCOLS (doubles per observation) as constants.
//
// Value contract (include/kissmcmc_hip.h):
//     lp(x) = -inf                      when prior(x) == -inf (the terms are evaluated anyway and ignored)
//     lp(x) = prior(x) + S(x)           otherwise
//     S(x)  = the pairwise tree over t_j = term(x, d_j), j = 0 .. ndata-1, in index order: each level adds neighbours
//             (t0+t1), (t2+t3), ...; an odd last element passes up unchanged.
// Every aligned block of 2^k observations is a node of that tree, and the part of the tree over a block cut short by the end of
// the data is the same pairwise tree over what is there; so the kernels may cut the observations into aligned power-of-two blocks
// however they like and still compute the same value.  A short tail inside a static tree is padded with +0.0 (same value except
// for the sign of a zero sum).
//
// Kernels (one half-step's proposals, or any set of rows):
//   data_partial_lane -- one proposal per lane, its row in registers; the observation row is wave-uniform (scalar loads).  A lane
//                        folds a static tree of kChunk terms, then a binary-counter stack over `rounds` chunks; a workgroup folds its
//                        kWaves waves' nodes through LDS.  Node of kWaves * kChunk * rounds observations per (block, proposal).
//   data_partial_obs  -- one proposal per workgroup, one observation per lane: 64 terms reduced by the fixed DPP / v_permlane
//                        butterfly (group_sum<64>), then the same stack and LDS fold.  Node of kWaves * 64 * rounds observations.
//   data_fold         -- one proposal per thread: the tree over the blocks' nodes, the prior, the log-pdf.
//   data_fold_split   -- the same tree and prior, written separately: S to out[prop], the prior to out[nprop + prop] (likelihood
//                        tempering, DESIGN.md section 4d: a rung samples prior + beta S).
#pragma once
#include "kmc_device.hpp"

namespace kmc_data {

constexpr int kWaves = 4;        // waves per workgroup of the partial kernels
constexpr int kChunk = 16;       // data_partial_lane: terms per static tree (then the stack)
constexpr int kLevels = 13;      // binary-counter stack depth: at most 2^13 - 1 nodes pushed (rounds per wave, blocks per proposal)

struct DataArgs {
    const double* prop;   // [nprop][ld] proposal rows
    const double* data;   // [ndata][NCOLS] observations
    double*       part;   // [nblocks][nprop] tree nodes, one per (workgroup block of observations, proposal)
    double*       out;    // [nprop] log-pdfs (data_fold)
    int64_t       nprop;
    int64_t       ndata;
    int32_t       ld;
    int32_t       rounds; // chunks per wave (power of two, <= 2^(kLevels-1))
    int32_t       nblocks;
    int32_t       pad_;
    double        p[6];   // params
};

// The binary counter of a lane: node i (0-based, in order) of equal-size nodes goes in at level 0 and merges upwards (left + right)
// while the bits of i below the level are set.  i is wave-uniform, so the branches are scalar; the levels are template recursion
// (static indices from the start, so the stack is promoted to registers -- a loop over them left it in scratch memory).
struct Stack {
    double s[kLevels];
    template <int L>
    __device__ __forceinline__ void push_at(double v, uint32_t i)
    {
        if constexpr (L < kLevels) {
            if ((i >> L) & 1u) push_at<L + 1>(s[L] + v, i);
            else s[L] = v;
        }
    }
    __device__ __forceinline__ void push(double v, uint32_t i) { push_at<0>(v, i); }
    // the tree over the n >= 1 nodes pushed: the partial nodes at the set bits of n, right-folded from the lowest level up
    template <int L>
    __device__ __forceinline__ void finish_at(uint32_t n, double& acc, bool& have) const
    {
        if ((n >> L) & 1u) { acc = have ? s[L] + acc : s[L]; have = true; }
        if constexpr (L + 1 < kLevels) finish_at<L + 1>(n, acc, have);      // (one call site per level: inlining stays linear)
    }
    __device__ __forceinline__ double finish(uint32_t n) const { double acc = 0.0; bool have = false; finish_at<0>(n, acc, have); return acc; }
};

template <int NCOLS>
__device__ __forceinline__ const double* obs_row(const double* data, int64_t j) { return data + j * (int64_t)NCOLS; }

// static tree of N terms starting at observation j (wave-uniform); CHECK: rows at or past ndata count as +0.0
template <class F, int ND, int NCOLS, int N, bool CHECK>
__device__ __forceinline__ double chunk_tree(const double* x, const double* data, int64_t j, int64_t ndata, const double* p)
{
    if constexpr (N == 1) {
        if (CHECK && j >= ndata) return 0.0;
        return F::term(x, ND, obs_row<NCOLS>(data, j), p);
    } else {
        const double a = chunk_tree<F, ND, NCOLS, N / 2, CHECK>(x, data, j, ndata, p);
        const double b = chunk_tree<F, ND, NCOLS, N / 2, CHECK>(x, data, j + N / 2, ndata, p);
        return a + b;
    }
}

// the workgroup's kWaves wave nodes (each over `per_wave` observations starting at wave_j0) -> one node, folded through LDS in tree
// order; a wave whose block starts at or past ndata holds nothing and its sibling passes up.  Result valid in wave 0.
__device__ __forceinline__ double fold_waves(double v, int wave, int lane_slot, int nslots, int64_t wg_j0, int64_t per_wave, int64_t ndata, double* lds)
{
    lds[wave * nslots + lane_slot] = v;
    __syncthreads();
    double r = v;
    if (wave == 0) {
        const double w0 = lds[lane_slot], w1 = lds[nslots + lane_slot], w2 = lds[2 * nslots + lane_slot], w3 = lds[3 * nslots + lane_slot];
        const bool h1 = wg_j0 + per_wave < ndata, h2 = wg_j0 + 2 * per_wave < ndata, h3 = wg_j0 + 3 * per_wave < ndata;
        const double a = h1 ? w0 + w1 : w0;
        const double b = h3 ? w2 + w3 : w2;
        r = h2 ? a + b : a;
    }
    return r;
}
static_assert(kWaves == 4, "fold_waves folds four waves");

// one proposal per lane; grid (ceil(nprop / 64), nblocks), kWaves * 64 threads
template <class F, int ND, int NCOLS>
__device__ __forceinline__ void data_partial_lane_body(const DataArgs& a)
{
    __shared__ double lds[kWaves * 64];
    const int lane = (int)(threadIdx.x & 63);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));       // provably wave-uniform (scalar addressing below)
    const int64_t prop = (int64_t)blockIdx.x * 64 + lane;
    const int64_t rows = a.nprop;
    const int64_t per_wave = (int64_t)kChunk * a.rounds;
    const int64_t wg_j0 = (int64_t)blockIdx.y * kWaves * per_wave;
    const int64_t j0 = wg_j0 + (int64_t)wave * per_wave;
    const double* __restrict__ data = a.data;
    double x[ND];
    const int64_t pr = prop < rows ? prop : rows - 1;                                 // (tail lanes evaluate a real row, write nothing)
#pragma unroll
    for (int k = 0; k < ND; ++k) x[k] = a.prop[pr * a.ld + k];
    double v = 0.0;
    if (j0 < a.ndata) {
        const int64_t left = a.ndata - j0;
        const int64_t full = left >= per_wave ? a.rounds : left / kChunk;            // whole chunks
        const int64_t nchunks = left >= per_wave ? a.rounds : (left + kChunk - 1) / kChunk;
        Stack st;
        for (int64_t c = 0; c < full; ++c)
            st.push(chunk_tree<F, ND, NCOLS, kChunk, false>(x, data, j0 + c * kChunk, a.ndata, a.p), (uint32_t)c);
        if (nchunks > full)
            st.push(chunk_tree<F, ND, NCOLS, kChunk, true>(x, data, j0 + full * kChunk, a.ndata, a.p), (uint32_t)full);
        v = st.finish((uint32_t)nchunks);
    }
    const double r = fold_waves(v, wave, lane, 64, wg_j0, per_wave, a.ndata, lds);
    if (wave == 0 && prop < rows) a.part[(int64_t)blockIdx.y * rows + prop] = r;
}

// one proposal per workgroup, one observation per lane; grid (nprop, nblocks), kWaves * 64 threads
template <class F, int ND, int NCOLS>
__device__ __forceinline__ void data_partial_obs_body(const DataArgs& a)
{
    __shared__ double lds[kWaves];
    const int lane = (int)(threadIdx.x & 63);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t prop = blockIdx.x;
    const int64_t per_wave = (int64_t)64 * a.rounds;
    const int64_t wg_j0 = (int64_t)blockIdx.y * kWaves * per_wave;
    const int64_t j0 = wg_j0 + (int64_t)wave * per_wave;
    const double* __restrict__ row = a.prop + prop * a.ld;                             // wave-uniform: scalar loads
    double x[ND];
#pragma unroll
    for (int k = 0; k < ND; ++k) x[k] = row[k];
    double v = 0.0;
    if (j0 < a.ndata) {
        const int64_t left = a.ndata - j0;
        const int64_t n = left >= per_wave ? a.rounds : (left + 63) / 64;
        Stack st;
        for (int64_t c = 0; c < n; ++c) {
            const int64_t j = j0 + c * 64 + lane;
            const double t = j < a.ndata ? F::term(x, ND, obs_row<NCOLS>(a.data, j), a.p) : 0.0;
            st.push(kmc::group_sum<64>(t), (uint32_t)c);                                // the fixed butterfly: the tree of 64 in lane order
        }
        v = st.finish((uint32_t)n);
    }
    const double r = fold_waves(v, wave, 0, 1, wg_j0, per_wave, a.ndata, lds);
    if (wave == 0 && lane == 0) a.part[(int64_t)blockIdx.y * a.nprop + prop] = r;
}

// one proposal per thread: the tree over the nblocks nodes, then the prior
template <class F, int ND>
__device__ __forceinline__ void data_fold_body(const DataArgs& a)
{
    const int64_t prop = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (prop >= a.nprop) return;
    double x[ND];
#pragma unroll
    for (int k = 0; k < ND; ++k) x[k] = a.prop[prop * a.ld + k];
    Stack st;
    for (int b = 0; b < a.nblocks; ++b) st.push(a.part[(int64_t)b * a.nprop + prop], (uint32_t)b);
    const double s = st.finish((uint32_t)a.nblocks);
    const double pri = F::prior(x, ND, a.p);
    a.out[prop] = pri == -INFINITY ? -INFINITY : pri + s;
}

// ... S and the prior as they are ([2][nprop]); what data_fold adds up, bit for bit
template <class F, int ND>
__device__ __forceinline__ void data_fold_split_body(const DataArgs& a)
{
    const int64_t prop = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (prop >= a.nprop) return;
    double x[ND];
#pragma unroll
    for (int k = 0; k < ND; ++k) x[k] = a.prop[prop * a.ld + k];
    Stack st;
    for (int b = 0; b < a.nblocks; ++b) st.push(a.part[(int64_t)b * a.nprop + prop], (uint32_t)b);
    a.out[prop] = st.finish((uint32_t)a.nblocks);
    a.out[a.nprop + prop] = F::prior(x, ND, a.p);
}

}  // namespace kmc_data
