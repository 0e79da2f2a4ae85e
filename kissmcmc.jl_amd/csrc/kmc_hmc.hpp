// kmc_hmc.hpp -- a Hamiltonian Monte Carlo step for the many-chain Metropolis sampler, one chain per lane (gfx950).
//
// The chain-per-lane form of kmc_metropolis.hpp with a gradient-informed proposal: a fixed number of leapfrog steps from the current
// state, the momentum being the normals an iteration of the random walk already draws.  Position, momentum and gradient of a chain of
// up to 32 dimensions live in the lane's registers; every lane runs the same number of leapfrog steps, so nothing diverges; the ~1400
// cycles of Philox, Box-Muller and a logarithm of an iteration are paid once per trajectory instead of once per density evaluation.
//
// The rule (include/kissmcmc_hip.h holds the same text).  Iteration `it` of chain `c` has, from Philox block 0 and blocks b >= 1
// exactly as in kmc_metropolis.hpp, the normals z_0 .. z_{ndim-1} and the accept uniform u, and, new, j = w3 & 0xFFF of block 0 (the
// uniform uses w3 >> 12: these 12 bits are read by nothing else).  Nothing more is drawn.
//   f    = 1.0 + jitter * (((double)j + 0.5) * 0x1p-11 - 1.0)         jitter in [0, 1); jitter == 0 gives f == 1.0 exactly
//   e_i  = step_i * f;   h_i = 0.5 * e_i                               step_i > 0: the step size per dimension (a diagonal metric)
//   m    = z;            K0 = 0.5 * ((m_0 m_0 + m_1 m_1) + ...)        i ascending
//   y    = x;            g  = grad(y)
//   nleap times:   m_i = m_i + h_i * g_i;  y_i = y_i + e_i * m_i  (every i);  g = grad(y);  m_i = m_i + h_i * g_i
//   p1   = logpdf(y);    K1 as K0 from the final m
//   accept  iff  (p1 - K1) - (p0 - K0) > log u                         strict, as src/samplers.jl:101
// Every product and every sum is rounded on its own (-ffp-contract=off, and no fma() is written here).  logpdf is the density's Seq
// evaluation, grad is Grad<Dens> below (a runtime-compiled body density: the caller's grad body, g zero on entry).  A
// non-finite gradient or log-density is not an error: NaN or inf propagates and the strict comparison rejects -- a divergent trajectory
// is a rejected proposal; p0 = -inf at the start is carried, and the first finite proposal is then accepted.  Counters, burn-in,
// thinning, storage and moments are those of metropolis_chains_body, and a chain's result is a pure function of (seed, chain index,
// inputs): independent of the launch geometry and of how the iteration range is cut into launches.
//
// This kernel computes g = grad(x) anew at the start of every iteration (nleap + 1 gradient evaluations per iteration): carrying it
// across a rejected proposal would take a fifth register array.  The step sizes are read through the constant address space at
// compile-time indices (scalar loads, no registers); the moment sums stay in memory and are touched only when a sample is stored, so
// that x, y, m and g (256 VGPRs at 32 dimensions) are all the arrays a lane holds.
#pragma once
#include "kmc_metropolis.hpp"

namespace kmc {

struct HmcArgs {
    MetropolisArgs a;          // step: [max(ndim, 32)] step sizes, zeros beyond ndim; xt / yt / st1 / st2 / blob unused
    int32_t        nleap;      // leapfrog steps per iteration, >= 1
    int32_t        pad_;
    double         jitter;     // in [0, 1)
};

struct GradArgs {              // grad_rows: the gradient of dense rows
    const double* pos;         // [nrows][ndim]
    double*       grad;        // [nrows][ndim]
    int64_t       nrows;
    int32_t       ndim;
    int32_t       pad_;
    DensityParams dp;
};

// ------------------------------------------------------------------------------------------------
// The gradients of the log-densities, Grad<D>::eval<NB>(x, ndim, P, g): THE definition of their operation order (every operation
// rounded on its own; p = the digested parameters of kmc_device.hpp's densities).  They stand here, not next to each Seq, because
// kmc_device.hpp is one of the headers the tracked profile records of the emcee kernels are keyed by (bench.py: kernel_sources_sha16).
// NB > 0: a compile-time bound on ndim, so that the loop unrolls and x and g stay in the caller's registers.
// ------------------------------------------------------------------------------------------------
template <class D> struct Grad;

template <> struct Grad<GaussianIso> {               // t = (x_i - p0) * p1;  g_i = -(t * p1)
    template <int NB = 0>
    __device__ static void eval(const double* x, int ndim, const DensityParams& P, double* g)
    {
#pragma unroll
        for (int i = 0; i < (NB > 0 ? NB : ndim); ++i) {
            if (i < ndim) {
                const double t = (x[i] - P.p[0]) * P.p[1];
                g[i] = -(t * P.p[1]);
            }
        }
    }
};

template <> struct Grad<Exponential> {               // g_i = -p0, outside the support as well (the log-density there is -inf: rejected)
    template <int NB = 0>
    __device__ static void eval(const double*, int ndim, const DensityParams& P, double* g)
    {
#pragma unroll
        for (int i = 0; i < (NB > 0 ? NB : ndim); ++i)
            if (i < ndim) g[i] = -P.p[0];
    }
};

// with a, b, s = p0, p1, p2 and n = ndim, for k = 0 .. n - 1:
//   acc = 0.0
//   k >= 1:      d = x_k - x_{k-1} * x_{k-1};      acc = (2.0 * b) * d
//   k <= n - 2:  d = x_{k+1} - x_k * x_k;          acc = acc - ((4.0 * b) * x_k) * d;     acc = acc - 2.0 * (a - x_k)
//   g_k = -(acc * s)
template <> struct Grad<Rosenbrock> {
    template <int NB = 0>
    __device__ static void eval(const double* x, int ndim, const DensityParams& P, double* g)
    {
        const double a = P.p[0], b2 = 2.0 * P.p[1], b4 = 4.0 * P.p[1];
#pragma unroll
        for (int k = 0; k < (NB > 0 ? NB : ndim); ++k) {
            if (k < ndim) {
                double acc = 0.0;
                if (k >= 1) {
                    const double d = x[k] - x[k - 1] * x[k - 1];
                    acc = b2 * d;
                }
                if ((NB == 0 || k + 1 < NB) && k + 1 < ndim) {
                    const double d = x[k + 1] - x[k] * x[k];
                    acc = acc - (b4 * x[k]) * d;
                    acc = acc - 2.0 * (a - x[k]);
                }
                g[k] = -(acc * P.p[2]);
            }
        }
    }
};

template <> struct Grad<LogNormal> {                 // x_i > 0:  lx = log(x_i);  t = (lx - p0) / p1;  g_i = -((1.0 + t / p1) / x_i);   otherwise 0.0
    template <int NB = 0>
    __device__ static void eval(const double* x, int ndim, const DensityParams& P, double* g)
    {
#pragma unroll
        for (int i = 0; i < (NB > 0 ? NB : ndim); ++i) {
            if (i < ndim) {
                double gi = 0.0;
                if (x[i] > 0.0) {
                    const double lx = log(x[i]);
                    const double t = (lx - P.p[0]) / P.p[1];
                    gi = -((1.0 + t / P.p[1]) / x[i]);
                }
                g[i] = gi;
            }
        }
    }
};

template <> struct Grad<MvNormal2> {                 // d0 = x_0 - p0;  d1 = x_1 - p1;  g_0 = -(p2 * d0 + p3 * d1);  g_1 = -(p3 * d0 + p4 * d1)
    template <int NB = 0>
    __device__ static void eval(const double* x, int, const DensityParams& P, double* g)
    {
        if constexpr (NB == 0 || NB >= 2) {
            const double d0 = x[0] - P.p[0], d1 = x[1] - P.p[1];
            g[0] = -(P.p[2] * d0 + P.p[3] * d1);
            g[1] = -(P.p[3] * d0 + P.p[4] * d1);
        }
    }
};

// A runtime-compiled body density with the caller's gradient (kmc_user_density_set_grad): F has eval(x, n, p) and grad(x, n, p, g).
template <class F, int MAXD>
struct BodyGradDensity : BodyDensity<F, MAXD> { };
template <class F, int MAXD> struct Grad<BodyGradDensity<F, MAXD>> {
    template <int NB = 0>
    __device__ static void eval(const double* x, int ndim, const DensityParams& P, double* g)
    {
#pragma unroll
        for (int i = 0; i < MAXD; ++i) g[i] = 0.0;
        F::grad(x, ndim, P.p, g);
    }
};

// K = 0.5 * ((m_0 m_0 + m_1 m_1) + ...), i ascending
template <int ND>
__device__ __forceinline__ double hmc_kinetic(const double (&m)[ND], int ndim)
{
    double s = m[0] * m[0];
#pragma unroll
    for (int d = 1; d < ND; ++d)
        if (d < ndim) s = s + m[d] * m[d];
    return 0.5 * s;
}

// ND: the register geometry, ndim <= ND.  EXACT: ndim == ND is a compile-time constant (the runtime-compiled modules: a body's
// `for (i < n)` then unrolls and its arrays stay in registers).
template <class Dens, int ND, bool EXACT = false>
__device__ __forceinline__ void metropolis_hmc_body(const HmcArgs& h)
{
    const MetropolisArgs& a = h.a;
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= a.nchains) return;
    const int ndim = EXACT ? ND : a.ndim;
    double x[ND], y[ND], m[ND], g[ND];
    const ConstDoubles sp = const_doubles(a.step);
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        x[d] = d < ndim ? a.pos[c * ndim + d] : 0.0;
        g[d] = 0.0;
    }
    double   p0  = a.logp[c];
    uint32_t na  = a.naccept[c];
    int64_t  cnt = a.cnt0, slot = a.slot0;
    int64_t  n   = a.it0 + 1 - a.nburnin;                                    // :96
    const uint32_t k0 = a.seed_lo ^ 0x4d455452u, k1 = a.seed_hi;
    const int nleap = h.nleap;
    for (int64_t it = a.it0; it < a.it1; ++it, ++n) {
        const U4 w = philox4x32_10((uint32_t)it, (uint32_t)((uint64_t)it >> 32), (uint32_t)c, 0u, k0, k1);
        double nr[ND + 4];
#pragma unroll
        for (int d = 0; d < ND + 4; ++d) nr[d] = 0.0;
        if constexpr (ND == 1) nr[0] = normal_first(w.x, w.y);
        else normal_pair(w.x, w.y, nr[0], nr[1]);
        if constexpr (ND > 2) {
#pragma unroll
            for (int b = 1; 4 * b - 2 < ND; ++b) {
                if (4 * b - 2 < ndim) {
                    const U4 v = philox4x32_10((uint32_t)it, (uint32_t)((uint64_t)it >> 32), (uint32_t)c, (uint32_t)b, k0, k1);
                    normal_pair(v.x, v.y, nr[4 * b - 2], nr[4 * b - 1]);
                    normal_pair(v.z, v.w, nr[4 * b], nr[4 * b + 1]);
                }
            }
        }
        const double f = 1.0 + h.jitter * (((double)(w.w & 0xFFFu) + 0.5) * 0x1.0p-11 - 1.0);
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            m[d] = d < ndim ? nr[d] : 0.0;
            y[d] = x[d];
        }
        const double K0 = hmc_kinetic<ND>(m, ndim);
        Grad<Dens>::template eval<ND>(y, ndim, a.dp, g);
        for (int l = 0; l < nleap; ++l) {
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                if (d < ndim) {
                    const double e = sp[d] * f;
                    const double hh = 0.5 * e;
                    m[d] = m[d] + hh * g[d];
                    y[d] = y[d] + e * m[d];
                }
            }
            Grad<Dens>::template eval<ND>(y, ndim, a.dp, g);
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                if (d < ndim) {
                    const double hh = 0.5 * (sp[d] * f);
                    m[d] = m[d] + hh * g[d];
                }
            }
        }
        typename Dens::Seq q;
        Dens::seq_init(q);
#pragma unroll
        for (int d = 0; d < ND; ++d)
            if (d < ndim) Dens::seq_add(q, y[d], d, a.dp);
        const double p1 = Dens::seq_finish(q, ndim, a.dp);
        const double K1 = hmc_kinetic<ND>(m, ndim);
        const uint64_t kk = ((uint64_t)w.z << 20) | (uint64_t)(w.w >> 12);
        const double lu = log_pos_normal(((double)kk + 0.5) * 0x1.0p-52);
        if ((p1 - K1) - (p0 - K0) > lu) {                                    // :101, note the strict >
#pragma unroll
            for (int d = 0; d < ND; ++d) x[d] = y[d];                        // :102
            p0 = p1;                                                         // :104
            na += n > 0 ? 1u : 0u;                                           // :105
        }
        if (n > 0) {                                                         // :108, :112
            if (++cnt == a.nthin) {
                cnt = 0;
                if (slot < a.nsamples) {
                    if (a.chain != nullptr) {
#pragma unroll
                        for (int d = 0; d < ND; ++d)
                            if (d < ndim) a.chain[(slot * a.nchains + c) * ndim + d] = x[d];     // :113
                    }
                    if (a.chain_logp != nullptr) a.chain_logp[slot * a.nchains + c] = p0;        // :115
                    if (a.csum != nullptr) {                                 // (the sums live in memory: see the top of this file)
#pragma unroll
                        for (int d = 0; d < ND; ++d) {
                            if (d < ndim) {
                                a.csum[c * ndim + d] += x[d];
                                a.csumsq[c * ndim + d] += x[d] * x[d];
                            }
                        }
                    }
                }
                ++slot;
            }
        }
    }
#pragma unroll
    for (int d = 0; d < ND; ++d)
        if (d < ndim) a.pos[c * ndim + d] = x[d];
    a.logp[c] = p0;
    a.naccept[c] = na;
}

// grad[r] = the gradient of the log-density at pos[r], one row per lane (kmc_grad_eval_host)
template <class Dens, int ND, bool EXACT = false>
__device__ __forceinline__ void grad_rows_body(const GradArgs& a)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.nrows) return;
    const int ndim = EXACT ? ND : a.ndim;
    double x[ND], g[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        x[d] = d < ndim ? a.pos[r * ndim + d] : 0.0;
        g[d] = 0.0;
    }
    Grad<Dens>::template eval<ND>(x, ndim, a.dp, g);
#pragma unroll
    for (int d = 0; d < ND; ++d)
        if (d < ndim) a.grad[r * ndim + d] = g[d];
}

template <class Dens, int ND>
__global__ __launch_bounds__(256) void metropolis_hmc(const HmcArgs h)
{
    metropolis_hmc_body<Dens, ND>(h);
}

template <class Dens, int ND>
__global__ __launch_bounds__(256) void grad_rows(const GradArgs a)
{
    grad_rows_body<Dens, ND>(a);
}

#ifndef __HIPCC_RTC__
// the menu densities' instances (kmc_inst_hmc.hip): the kernels of a density id for ndim <= 32, nullptr where there is none
using HmcFn = void (*)(const HmcArgs);
using GradFn = void (*)(const GradArgs);
HmcFn hmc_lookup(int density, int ndim);
GradFn grad_lookup(int density, int ndim);
#endif

}  // namespace kmc
