// kmc_state.hip -- a sampler's state in and out: the initial ensemble and its log-pdfs (reference src/samplers.jl:198,
// :209-210), the device-side initial ball (:311-349), checkpoint / resume, the read-outs (positions, log-pdfs, accept
// statistics :291, streaming moments), the deal of dealt sub-ensembles, and the one-shot `emcee` call (:188-293).
// Every way in ends in reset_run_state (accumulators, run fields, the finiteness scan); the two that start a run from nothing go
// through start_at_generation_0 first.  kmc_sampler_get_moments dispatches to one function per accumulator layout.  The getters
// and setters that only need the stream drained begin with settle() after their argument checks (kmc_sampler_get_moments flushes
// first and keeps its own preamble; the deal kernels and get_accept_ratio drain nothing themselves); temporaries on the device are
// ScopedDeviceBlock (kmc_host.hpp).
#include <signal.h>

#include <cmath>
#include <cstdlib>

#define KMC_DEFINE_STATE_KERNELS
#include "kmc_sampler.hpp"

using namespace kmc;
using namespace kmc_host;

namespace kmc_host {
// Initial log-pdfs of the rows in d_pos (src/samplers.jl:209-210) into d_logp, on the sampler's stream.  KMC_F32: the
// log-pdf kernels read double rows, so the float rows are widened (exactly) into a scratch buffer first.
__global__ __launch_bounds__(256) void widen_rows(const float* src, double* dst, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = (double)src[i];
}
__global__ __launch_bounds__(256) void narrow_rows(const double* src, float* dst, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = (float)src[i];
}

// the per-walker block {logp, naccept, klast} of rung t of a tempered sampler (16 nrows bytes per rung; rung 0: d_logp itself)
static double* rung_logp(const kmc_sampler* s, int t) { return s->d_logp + 2 * (size_t)t * (size_t)s->nrows; }
static uint32_t* rung_naccept(const kmc_sampler* s, int t) { return reinterpret_cast<uint32_t*>(rung_logp(s, t) + s->nrows); }
static double* rung_pos(const kmc_sampler* s, int t) { return s->d_pos + (size_t)t * (size_t)s->nrows * (size_t)s->ld; }

// What every getter and setter starts with, after its argument checks: the sampler's device current and its stream drained;
// p2p_err: and no peer wait timed out (a read-out of a sharded run).
static kmc_status settle(kmc_sampler* s, bool p2p_err = false)
{
    HIP_TRY(hipSetDevice(s->cfg.device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return p2p_err ? check_p2p_err(s) : KMC_OK;
}

// int64 host arrays over uint32 device arrays (accept counters, walker ids); src_host null: zeros
static hipError_t upload_u32(const kmc_sampler* s, uint32_t* dst_dev, const int64_t* src_host, size_t n)
{
    std::vector<uint32_t> tmp(n, 0u);
    if (src_host) for (size_t i = 0; i < n; ++i) tmp[i] = (uint32_t)src_host[i];
    return copy_sync(dst_dev, tmp.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream);
}
static hipError_t download_u32(const kmc_sampler* s, int64_t* dst_host, const uint32_t* src_dev, size_t n)
{
    std::vector<uint32_t> tmp(n);
    const hipError_t e = copy_sync(tmp.data(), src_dev, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream);
    for (size_t i = 0; e == hipSuccess && i < n; ++i) dst_host[i] = (int64_t)tmp[i];
    return e;
}

kmc_status eval_initial_logp(kmc_sampler* s, double* logp_out = nullptr, int rung = 0)      // (logp_out: somewhere else than d_logp -- a caller that only wants the blobs)
{
    const size_t nw = (size_t)s->nrows, nd = (size_t)s->cfg.ndim;
    double* rows = rung_pos(s, rung);
    if (rung > 0 && !logp_out) logp_out = rung_logp(s, rung);
    ScopedDeviceBlock scratch;
    if (s->f32) {
        const int64_t n = (int64_t)(nw * (size_t)s->ld);
        HIP_TRY(scratch.alloc((size_t)n * sizeof(double)));
        hipLaunchKernelGGL(widen_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, reinterpret_cast<const float*>(s->d_pos), scratch.as<double>(), n);
        rows = scratch.as<double>();
    }
    const LogpdfArgs la{rows, logp_out ? logp_out : s->d_logp, (int64_t)nw, (int32_t)nd, (int32_t)s->ld, s->dp, s->d_blob};   // (blobs of the initial evaluations, :209-210)
    if (s->user) {
        HIP_TRY(launch_module(s->uk.logpdf, (unsigned)((nw + 255) / 256), 256u, s->stream, la));
    } else {
        hipLaunchKernelGGL(s->logpdf_fn, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, s->stream, la);
        HIP_TRY(hipGetLastError());
    }
    if (scratch.p) HIP_TRY(hipStreamSynchronize(s->stream));    // (the kernel reads the scratch until then)
    return KMC_OK;
}

// What "start at generation 0" means (kmc_sampler_set_positions, kmc_sampler_init_ball): accept counters, the device's generation
// counter, the P2P progress flags and error word, the moments' base, a dealt sub-ensemble's walker ids.  A field added to a sampler
// that a new start must clear goes here; one that a restored state must clear too goes into reset_run_state.
kmc_status start_at_generation_0(kmc_sampler* s)
{
    HIP_TRY(hipMemsetAsync(s->d_naccept, 0, (size_t)s->nrows * sizeof(uint32_t), s->stream));
    HIP_TRY(hipMemsetAsync(s->d_gen, 0, 64, s->stream));
    if (s->p2p) {                                                // (callers barrier across ranks before running)
        HIP_TRY(fill_sync(s->d_flags, 0, 4096, s->stream));
        HIP_TRY(fill_sync(s->d_err, 0, 64, s->stream));
    }
    s->dev_gen = 0;
    s->moment_base = 0;
    if (s->d_ids) {                                              // dealt sub-ensembles: slot i holds global walker r S + i
        hipLaunchKernelGGL(deal_init_ids, dim3((unsigned)((s->nrows + 255) / 256)), dim3(256), 0, s->stream, s->d_ids, s->nrows,
                           (uint32_t)((uint64_t)s->cfg.deal_rank * (uint64_t)s->nrows));
        HIP_TRY(hipGetLastError());
    }
    return KMC_OK;
}

// Everything an entry point does after the rows are in place -- the only place that zeroes the accumulators, clears the host-side
// run fields and scans for a non-finite log-pdf: initial log-pdfs (src/samplers.jl:209-210) unless they are supplied, accumulators
// (klast: the samples taken so far), the run fields, finiteness check.
kmc_status reset_run_state(kmc_sampler* s, bool eval_logp, int64_t generation, uint32_t klast_value)
{
    const size_t nw = (size_t)s->nrows;
    if (eval_logp) KMC_TRY(eval_initial_logp(s));
    std::vector<double> lp(nw);
    HIP_TRY(copy_sync(lp.data(), s->d_logp, nw * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    if (s->d_msum) {
        HIP_TRY(hipMemsetAsync(s->d_msum, 0, (size_t)s->macc_elems * sizeof(double), s->stream));
        HIP_TRY(hipMemsetAsync(s->d_msumsq, 0, (size_t)s->macc_elems * sizeof(double), s->stream));
        if (s->d_klast) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)s->d_klast, (int)klast_value, nw, s->stream));
        if (s->d_mcnt) HIP_TRY(hipMemsetAsync(s->d_mcnt, 0, 2 * (size_t)s->mring_waves * sizeof(uint32_t), s->stream));
        if (s->d_isum) {
            const size_t ne = (size_t)s->nislands * 4 * (size_t)s->island_K;
            HIP_TRY(hipMemsetAsync(s->d_isum, 0, ne * sizeof(double), s->stream));
            HIP_TRY(hipMemsetAsync(s->d_isumsq, 0, ne * sizeof(double), s->stream));
        }
        s->carry_sum.clear(); s->carry_sumsq.clear();
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->pos2_current = false;
    s->fused_cur = 0;                  // (the caller's state is in d_pos / d_logp: whatever a failed run left in copy 1 is void)
    s->generation = generation;
    s->launches = 0;
    s->have_run_events = false;
    if (s->stream_chain) { HIP_TRY(hipStreamSynchronize(s->copy_stream)); s->blocks_copied = 0; s->blocks_waited = 0; s->flushed_done = -1; }
    for (size_t w = 0; w < nw; ++w)
        if (!std::isfinite(lp[w])) {
            s->positions_set = false;
            return fail(KMC_ERR_NONFINITE_LOGP, "walker " + std::to_string(w) + " has a non-finite initial log-pdf");
        }
    s->positions_set = true;
    return KMC_OK;
}

// Parallel tempering: the ladder's own counters back to zero (or to a checkpoint's values)
kmc_status reset_temper_counters(kmc_sampler* s, const uint64_t* nswap, const double* logp_sum)
{
    if (!s->temper) return KMC_OK;
    const size_t nt = (size_t)s->ntemps;
    std::vector<unsigned long long> ns(nt, 0ull);
    std::vector<double> ls(nt + 2 * (size_t)s->ld, 0.0);                   // logp_sum, then the moments credited at exchanges
    if (nswap) for (size_t t = 0; t + 1 < nt; ++t) ns[t] = nswap[t];
    if (logp_sum) for (size_t t = 0; t < nt; ++t) ls[t] = logp_sum[t];
    HIP_TRY(copy_sync(s->d_nswap, ns.data(), nt * sizeof(unsigned long long), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(copy_sync(s->d_rung_sum, ls.data(), ls.size() * sizeof(double), hipMemcpyHostToDevice, s->stream));
    if (s->temper_like) HIP_TRY(fill_sync(s->d_like_sum, 0, nt * sizeof(double), s->stream));      // (a checkpoint's: kmc_sampler_set_rung_loglike_sum)
    if (s->adapt) {                                                        // the ladder starts again from the caller's (a checkpoint's: kmc_sampler_set_ladder)
        std::vector<double> z(2 * nt + 2, 0.0);                            // S, then round_acc, the ticket and the rounds skipped: zero
        for (size_t j = 0; j < s->S0.size(); ++j) z[j] = s->S0[j];
        HIP_TRY(copy_sync(s->d_betas, s->betas.data(), nt * sizeof(double), hipMemcpyHostToDevice, s->stream));
        HIP_TRY(copy_sync(s->d_S, z.data(), z.size() * sizeof(double), hipMemcpyHostToDevice, s->stream));
    }
    return KMC_OK;
}
// Likelihood tempering: S and the prior of every walker of every rung from the rows in place -- one pass of the data kernels over
// ntemps x nwalkers rows, the value contract's bits whatever the cut.  fill_logp: the rungs above 0 get their log-pdfs from them
// (pri + S as data_fold adds them; rung 0's came from data_fold itself), and a non-finite one is refused like rung 0's.
kmc_status eval_like_all(kmc_sampler* s, bool fill_logp)
{
    const size_t nw = (size_t)s->nrows, nt = (size_t)s->ntemps;
    HIP_TRY(launch_data_eval(s->dk, s->data_ud, s->plan_all, s->d_pos, (int64_t)(nt * nw), (int32_t)s->ld, s->dp.p, s->d_part, s->part_doubles, s->d_like, s->stream, true));
    if (!fill_logp) { HIP_TRY(hipStreamSynchronize(s->stream)); return KMC_OK; }
    std::vector<double> sp(2 * nt * nw), lp(nw);
    HIP_TRY(copy_sync(sp.data(), s->d_like, sp.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    for (size_t t = 1; t < nt; ++t) {
        for (size_t w = 0; w < nw; ++w) {
            const double like = sp[t * nw + w], pri = sp[(nt + t) * nw + w];
            lp[w] = pri == -INFINITY ? -INFINITY : pri + like;
        }
        HIP_TRY(copy_sync(rung_logp(s, (int)t), lp.data(), nw * sizeof(double), hipMemcpyHostToDevice, s->stream));
    }
    return KMC_OK;
}
// rung 0's rows, log-pdfs and zeroed counters into every other rung (kmc_sampler_set_positions of a tempered sampler)
kmc_status replicate_rung0(kmc_sampler* s)
{
    const size_t nw = (size_t)s->nrows;
    for (int t = 1; t < s->ntemps; ++t) {
        HIP_TRY(hipMemcpyAsync(rung_pos(s, t), s->d_pos, nw * (size_t)s->ld * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
        HIP_TRY(hipMemcpyAsync(rung_logp(s, t), s->d_logp, nw * (sizeof(double) + 2 * sizeof(uint32_t)), hipMemcpyDeviceToDevice, s->stream));
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (s->temper_like) KMC_TRY(eval_like_all(s, false));
    return reset_temper_counters(s, nullptr, nullptr);
}

// The ball of kmc_sampler_init_ball into d_pos / d_logp, on the sampler's stream; *nfail: walkers that found no point with pdf > 0.
// (Its temporaries go with this scope, after the stream has drained.)
kmc_status draw_ball(kmc_sampler* s, const double* theta0, const double* ball_radius, uint64_t seed, int halving_steps, int ntries, unsigned long long* nfail)
{
    const size_t nd = (size_t)s->cfg.ndim, nelem = (size_t)s->nrows * (size_t)s->ld;
    ScopedDeviceBlock par, fails, ball;
    HIP_TRY(par.alloc(2 * nd * sizeof(double)));
    HIP_TRY(fails.alloc(sizeof(unsigned long long)));
    double* d_par = par.as<double>();
    HIP_TRY(copy_sync(d_par, theta0, nd * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(copy_sync(d_par + nd, ball_radius, nd * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(fill_sync(fails.p, 0, sizeof(unsigned long long), s->stream));
    double* d_ball = s->d_pos;                  // KMC_F32: the ball is drawn in double, then rounded into the float rows
    if (s->f32) { HIP_TRY(ball.alloc(nelem * sizeof(double))); d_ball = ball.as<double>(); }
    HIP_TRY(fill_sync(d_ball, 0, nelem * sizeof(double), s->stream));
    InitBallFn fn = s->user ? nullptr : with_density(s->cfg.density, InitBallFn(nullptr), [](auto d) { return init_ball_lookup<decltype(d)>(); });
    const int pieces = s->p2p ? 2 : 1;
    for (int piece = 0; piece < pieces; ++piece) {
        InitBallArgs a{};
        const int64_t rows = s->p2p ? s->h_loc : s->nrows;
        a.pos = d_ball + (size_t)piece * (size_t)s->h_loc * (size_t)s->ld;
        a.logp = s->d_logp + (size_t)piece * (size_t)s->h_loc;
        a.theta0 = d_par; a.radius = d_par + nd;
        a.nrows = rows;
        a.row_walker0 = s->p2p ? (int64_t)piece * s->h + s->active_begin
                               : (s->cfg.deal_count > 0 ? (int64_t)s->cfg.deal_rank * s->nrows : 0);   // rows of ONE global ball
        a.ndim = (int32_t)nd; a.ld = (int32_t)s->ld;
        a.halving_steps = halving_steps; a.ntries = ntries;
        a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
        a.dp = s->dp;
        a.fail = fails.as<unsigned long long>();
        a.blob = s->d_blob;
        const unsigned grid = (unsigned)((rows + 255) / 256);
        if (s->user) HIP_TRY(launch_module(s->uk.init_ball, grid, 256u, s->stream, a));
        else { hipLaunchKernelGGL(fn, dim3(grid), dim3(256), 0, s->stream, a); HIP_TRY(hipGetLastError()); }
    }
    if (s->f32) {
        hipLaunchKernelGGL(narrow_rows, dim3((unsigned)((nelem + 255) / 256)), dim3(256), 0, s->stream, d_ball, reinterpret_cast<float*>(s->d_pos), (int64_t)nelem);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(copy_sync(nfail, fails.p, sizeof(*nfail), hipMemcpyDeviceToHost, s->stream));
    return KMC_OK;
}

}  // namespace kmc_host
// Device-side make_theta0s: src/samplers.jl:311-349 (see init_ball in kmc_kernels.hpp).
KMC_EXPORT kmc_status kmc_sampler_init_ball(kmc_sampler* s, const double* theta0, const double* ball_radius,
                                            uint64_t seed, int halving_steps, int ntries)
{
    if (!s || !theta0 || !ball_radius || halving_steps < 1 || ntries < 1) return fail(KMC_ERR_BAD_ARG, "bad argument");
    if (s->data_eval) return fail(KMC_ERR_UNSUPPORTED, "kmc_sampler_init_ball: not with KMC_DATA_DENSITY (build the initial ensemble on the host, e.g. make_theta0s)");
    if (s->host_eval) return fail(KMC_ERR_UNSUPPORTED, "kmc_sampler_init_ball evaluates the density on the device; with KMC_HOST_DENSITY build the ball on the host");
    if (s->temper) return fail(KMC_ERR_UNSUPPORTED, "kmc_sampler_init_ball: not with parallel tempering (build the initial ensemble on the host, e.g. make_theta0s; kmc_sampler_set_positions copies it to every rung)");
    if (s->push) return fail(KMC_ERR_UNSUPPORTED, "kmc_sampler_init_ball fills this rank's rows only; with KMC_P2P_PUSH use kmc_sampler_set_positions (the peers' copies must be filled too)");
    KMC_TRY(settle(s));
    unsigned long long nfail = 0;
    KMC_TRY(draw_ball(s, theta0, ball_radius, seed, halving_steps, ntries, &nfail));
    if (nfail != 0) {
        s->positions_set = false;
        return fail(KMC_ERR_NONFINITE_LOGP, "Could not find suitable initial theta.  PDF is zero in too many places inside ball. (" +
                                            std::to_string(nfail) + " walkers)");
    }
    KMC_TRY(start_at_generation_0(s));
    return reset_run_state(s, /*eval_logp=*/s->f32, 0, 0u);      // KMC_F32: the log-pdfs of the rows as rounded
}

// Checkpoint / resume: restore (positions, log-pdfs, acceptance counters, generation).  The random
// stream is a pure function of (seed, generation, walker), so the continued run is bit-identical to an
// uninterrupted one.  Moments and the chain restart at the restored generation.
static kmc_status set_state_rung0(kmc_sampler* s, const double* pos_host, const double* logp_host, const int64_t* naccept_host, int64_t generation)
{
    if (!s || !pos_host || !logp_host || generation < 0) return fail(KMC_ERR_BAD_ARG, "bad argument");
    // (stored blobs are chain storage too: after a resume past burn-in kmc_sampler_get_blobs would return rows never written)
    if (s->d_chain || s->d_chain_logp || s->d_chain_blob)
        return fail(KMC_ERR_UNSUPPORTED, "kmc_sampler_set_state: not with chain / blob storage (download the chain before checkpointing)");
    if (s->p2p && s->cfg.shard_count > 1)
        return fail(KMC_ERR_UNSUPPORTED, "kmc_sampler_set_state: P2P progress flags restart at 0; restore is single-GPU for now");
    KMC_TRY(settle(s));
    const size_t nw = (size_t)s->nrows;
    HIP_TRY(upload_rows(s, s->d_pos, pos_host, nw));
    HIP_TRY(copy_sync(s->d_logp, logp_host, nw * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(upload_u32(s, s->d_naccept, naccept_host, nw));
    if (s->p2p) {
        HIP_TRY(fill_sync(s->d_flags, 0, 4096, s->stream));
        HIP_TRY(fill_sync(s->d_err, 0, 64, s->stream));
    }
    if (s->d_blob) {
        // the blobs of the restored positions: evaluated again (same kernel and order as the initial evaluation: same bits);
        // the restored log-pdfs stay as given
        ScopedDeviceBlock scratch;
        HIP_TRY(scratch.alloc(nw * sizeof(double)));
        KMC_TRY(eval_initial_logp(s, scratch.as<double>()));
        HIP_TRY(hipStreamSynchronize(s->stream));
    }
    s->generation = generation;            // the device counter follows at the next graph replay
    const int64_t done = samples_done(s);
    s->moment_base = done;
    return reset_run_state(s, /*eval_logp=*/false, generation, (uint32_t)done);
}
KMC_EXPORT kmc_status kmc_sampler_set_state(kmc_sampler* s, const double* pos_host, const double* logp_host,
                                            const int64_t* naccept_host, int64_t generation)
{
    if (s && s->temper) return fail(KMC_ERR_UNSUPPORTED, "kmc_sampler_set_state restores one ensemble: a sampler with parallel tempering takes every rung through kmc_sampler_set_rung_state");
    return set_state_rung0(s, pos_host, logp_host, naccept_host, generation);
}

// theta_host is the GLOBAL ensemble: the whole of it, or (P2P) this shard's slice of each half -- local rows
// [0,h_loc) = global [begin, begin+h_loc), local [h_loc,2h_loc) = global [h+begin, ...) -- and, with KMC_P2P_PUSH, the local copies of the other shards' rows
static kmc_status upload_ensemble(kmc_sampler* s, const double* theta_host)
{
    const size_t nw = (size_t)s->nrows, nd = (size_t)s->cfg.ndim;
    if (!s->p2p) {
        HIP_TRY(upload_rows(s, s->d_pos, theta_host, nw));       // :198 (caller's array untouched)
        return KMC_OK;
    }
    const size_t hl = (size_t)s->h_loc;
    HIP_TRY(upload_rows(s, s->d_pos, theta_host + (size_t)s->active_begin * nd, hl));
    HIP_TRY(upload_rows(s, s->d_pos + hl * (size_t)s->ld, theta_host + ((size_t)s->h + (size_t)s->active_begin) * nd, hl));
    for (int q = 0; s->push && q < s->cfg.shard_count; ++q) {      // (block 1 + q = rank q's rows)
        if (q == s->cfg.shard_rank) continue;
        double* blk = s->d_pos + (size_t)(1 + q) * nw * (size_t)s->ld;
        HIP_TRY(upload_rows(s, blk, theta_host + (size_t)q * hl * nd, hl));
        HIP_TRY(upload_rows(s, blk + hl * (size_t)s->ld, theta_host + ((size_t)s->h + (size_t)q * hl) * nd, hl));
    }
    return KMC_OK;
}

// replicate: a tempered sampler copies the ensemble to every rung (kmc_sampler_set_positions); kmc_sampler_set_rung_state fills the
// other rungs itself
static kmc_status set_positions_rung0(kmc_sampler* s, const double* theta_host, bool replicate)
{
    if (!s || !theta_host) return fail(KMC_ERR_BAD_ARG, "null argument");
    reinstall_abort_backtrace();                                 // (diagnostics: somebody may have replaced the handler)
    KMC_TRY(settle(s));
    const size_t nw = (size_t)s->nrows, nd = (size_t)s->cfg.ndim;
    KMC_TRY(upload_ensemble(s, theta_host));
    // (ahead of the evaluation: if that fails, the counters are already zero and the ids dealt -- the sampler has no positions then, and
    //  every entry point that gives it some starts or restores them again)
    KMC_TRY(start_at_generation_0(s));
    if (s->data_eval) {                                          // :209-210, the same kernels as every half-step's proposals
        HIP_TRY(launch_data_eval(s->dk, s->data_ud, s->plan_all, s->d_pos, (int64_t)nw, (int32_t)s->ld, s->dp.p, s->d_part, s->part_doubles, s->d_logp, s->stream));
    } else if (s->host_eval) {                                   // :209-210, on the caller's thread
        std::vector<double> lp0(nw);
        if (s->cfg.host_logpdf(theta_host, (int64_t)nw, (int64_t)nd, lp0.data(), s->cfg.host_user) != 0) {
            s->positions_set = false;
            return fail(KMC_ERR_BAD_ARG, "the host log-pdf callback failed on the initial ensemble");
        }
        HIP_TRY(copy_sync(s->d_logp, lp0.data(), nw * sizeof(double), hipMemcpyHostToDevice, s->stream));
    } else {
        KMC_TRY(eval_initial_logp(s));                           // :209-210
    }
    KMC_TRY(reset_run_state(s, /*eval_logp=*/false, 0, 0u));
    if (s->temper && replicate) KMC_TRY(replicate_rung0(s));     // the same ensemble on every rung
    return KMC_OK;
}
KMC_EXPORT kmc_status kmc_sampler_set_positions(kmc_sampler* s, const double* theta_host)
{
    return set_positions_rung0(s, theta_host, true);
}

// ---- parallel tempering: every rung in and out (include/kissmcmc_hip.h) ---------------------------------------------------
KMC_EXPORT kmc_status kmc_sampler_set_rung_state(kmc_sampler* s, const double* pos_host, const double* logp_host, const int64_t* naccept_host,
                                                 const uint64_t* nswap_host, const double* logp_sum_host, int64_t generation)
{
    if (!s || !pos_host || generation < 0) return fail(KMC_ERR_BAD_ARG, "bad argument");
    if (!s->temper) return fail(KMC_ERR_BAD_ARG, "kmc_sampler_set_rung_state: the sampler was created without parallel tempering (ntemps < 2)");
    if (generation > 0 && !logp_host) return fail(KMC_ERR_BAD_ARG, "kmc_sampler_set_rung_state: a checkpoint (generation > 0) carries its log-pdfs");
    const size_t nw = (size_t)s->nrows, nd = (size_t)s->cfg.ndim;
    // rung 0 through the untempered entry points (initial log-pdfs, counters, moments, the finiteness check) ...
    if (generation == 0 && !logp_host) {
        KMC_TRY(set_positions_rung0(s, pos_host, false));
        if (naccept_host) HIP_TRY(upload_u32(s, s->d_naccept, naccept_host, nw));
    } else {
        KMC_TRY(set_state_rung0(s, pos_host, logp_host, naccept_host, generation));
    }
    // ... then the others the same way: rows, log-pdfs (given or evaluated), counters; klast as rung 0's (unused: moments are rung 0's)
    // (every rung's rows go up before any rung's log-pdfs are looked at: a non-finite one is reported with all rows in place, positions_set false)
    for (int t = 1; t < s->ntemps; ++t) HIP_TRY(upload_rows(s, rung_pos(s, t), pos_host + (size_t)t * nw * nd, nw));
    // likelihood tempering: every rung's S and prior again from the rows (and the log-pdfs, unless given): the same bits
    if (s->temper_like) KMC_TRY(eval_like_all(s, logp_host == nullptr));
    std::vector<double> lp(nw);
    for (int t = 1; t < s->ntemps; ++t) {
        if (logp_host) HIP_TRY(copy_sync(rung_logp(s, t), logp_host + (size_t)t * nw, nw * sizeof(double), hipMemcpyHostToDevice, s->stream));
        else if (!s->temper_like) KMC_TRY(eval_initial_logp(s, nullptr, t));
        HIP_TRY(upload_u32(s, rung_naccept(s, t), naccept_host ? naccept_host + (size_t)t * nw : nullptr, nw));
        HIP_TRY(hipMemsetAsync(rung_naccept(s, t) + nw, 0, nw * sizeof(uint32_t), s->stream));
        HIP_TRY(copy_sync(lp.data(), rung_logp(s, t), nw * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        for (size_t w = 0; w < nw; ++w)
            if (!std::isfinite(lp[w])) {
                s->positions_set = false;
                return fail(KMC_ERR_NONFINITE_LOGP, "walker " + std::to_string(w) + " of rung " + std::to_string(t) + " has a non-finite initial log-pdf");
            }
    }
    return reset_temper_counters(s, nswap_host, logp_sum_host);
}

KMC_EXPORT kmc_status kmc_sampler_get_rung_state(kmc_sampler* s, double* pos_host, double* logp_host, int64_t* naccept_host, double* logp_sum_host)
{
    if (!s) return fail(KMC_ERR_BAD_ARG, "null sampler");
    if (!s->temper) return fail(KMC_ERR_BAD_ARG, "kmc_sampler_get_rung_state: the sampler was created without parallel tempering (ntemps < 2)");
    KMC_TRY(settle(s));
    const size_t nw = (size_t)s->nrows, nd = (size_t)s->cfg.ndim;
    for (int t = 0; t < s->ntemps; ++t) {
        if (pos_host) HIP_TRY(download_rows(s, pos_host + (size_t)t * nw * nd, rung_pos(s, t), nw));
        if (logp_host) HIP_TRY(copy_sync(logp_host + (size_t)t * nw, rung_logp(s, t), nw * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        if (naccept_host) HIP_TRY(download_u32(s, naccept_host + (size_t)t * nw, rung_naccept(s, t), nw));
    }
    if (logp_sum_host) HIP_TRY(copy_sync(logp_sum_host, s->d_rung_sum, (size_t)s->ntemps * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    return KMC_OK;
}

KMC_EXPORT kmc_status kmc_sampler_get_rung_loglike(kmc_sampler* s, double* loglike_host, double* logprior_host, double* loglike_sum_host)
{
    if (!s) return fail(KMC_ERR_BAD_ARG, "null sampler");
    if (!s->temper_like) return fail(KMC_ERR_BAD_ARG, "kmc_sampler_get_rung_loglike: the sampler was created without likelihood tempering (temper_mode = KMC_TEMPER_LIKELIHOOD)");
    KMC_TRY(settle(s));
    const size_t n = (size_t)s->ntemps * (size_t)s->nrows;
    if (loglike_host) HIP_TRY(copy_sync(loglike_host, s->d_like, n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    if (logprior_host) HIP_TRY(copy_sync(logprior_host, s->d_prior, n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    if (loglike_sum_host) HIP_TRY(copy_sync(loglike_sum_host, s->d_like_sum, (size_t)s->ntemps * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    return KMC_OK;
}

KMC_EXPORT kmc_status kmc_sampler_set_rung_loglike_sum(kmc_sampler* s, const double* loglike_sum_host)
{
    if (!s) return fail(KMC_ERR_BAD_ARG, "null sampler");
    if (!s->temper_like) return fail(KMC_ERR_BAD_ARG, "kmc_sampler_set_rung_loglike_sum: the sampler was created without likelihood tempering (temper_mode = KMC_TEMPER_LIKELIHOOD)");
    KMC_TRY(settle(s));
    if (loglike_sum_host) HIP_TRY(copy_sync(s->d_like_sum, loglike_sum_host, (size_t)s->ntemps * sizeof(double), hipMemcpyHostToDevice, s->stream));
    else HIP_TRY(fill_sync(s->d_like_sum, 0, (size_t)s->ntemps * sizeof(double), s->stream));
    return KMC_OK;
}

KMC_EXPORT kmc_status kmc_sampler_get_swaps(kmc_sampler* s, uint64_t* nswap_host)
{
    if (!s || !nswap_host) return fail(KMC_ERR_BAD_ARG, "null argument");
    if (!s->temper) return fail(KMC_ERR_BAD_ARG, "kmc_sampler_get_swaps: the sampler was created without parallel tempering (ntemps < 2)");
    KMC_TRY(settle(s));
    std::vector<unsigned long long> ns((size_t)s->ntemps);
    HIP_TRY(copy_sync(ns.data(), s->d_nswap, ns.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->stream));
    for (int t = 0; t + 1 < s->ntemps; ++t) nswap_host[t] = (uint64_t)ns[(size_t)t];
    return KMC_OK;
}

KMC_EXPORT kmc_status kmc_sampler_get_ladder(kmc_sampler* s, double* betas_host, double* S_host, uint64_t* round_acc_host, uint64_t* skipped_host)
{
    if (!s) return fail(KMC_ERR_BAD_ARG, "null sampler");
    if (!s->temper) return fail(KMC_ERR_BAD_ARG, "kmc_sampler_get_ladder: the sampler was created without parallel tempering (ntemps < 2)");
    KMC_TRY(settle(s));
    const size_t nt = (size_t)s->ntemps;
    if (betas_host) HIP_TRY(copy_sync(betas_host, s->d_betas, nt * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    if (S_host && nt > 2) HIP_TRY(copy_sync(S_host, s->d_S, (nt - 2) * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    if (round_acc_host) {
        std::vector<unsigned long long> ra(nt);
        HIP_TRY(copy_sync(ra.data(), s->d_round_acc, nt * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->stream));
        for (size_t t = 0; t + 1 < nt; ++t) round_acc_host[t] = (uint64_t)ra[t];
    }
    if (skipped_host) {
        unsigned long long sk = 0ull;
        HIP_TRY(copy_sync(&sk, s->d_skipped, sizeof(sk), hipMemcpyDeviceToHost, s->stream));
        *skipped_host = (uint64_t)sk;
    }
    return KMC_OK;
}

KMC_EXPORT kmc_status kmc_sampler_set_ladder(kmc_sampler* s, const double* betas_host, const double* S_host, const uint64_t* round_acc_host, const uint64_t* skipped_host)
{
    if (!s || !betas_host || !S_host || !round_acc_host || !skipped_host) return fail(KMC_ERR_BAD_ARG, "null argument");
    if (!s->adapt) return fail(KMC_ERR_BAD_ARG, "kmc_sampler_set_ladder: the sampler was created without an adaptive ladder (kmc_config.adapt); a fixed ladder is set at creation");
    const size_t nt = (size_t)s->ntemps;
    if (betas_host[0] != 1.0 || betas_host[nt - 1] != s->betas[nt - 1])
        return fail(KMC_ERR_BAD_ARG, "adaptive ladder: kmc_sampler_set_ladder: the first and the last beta never move -- they must be the sampler's own");
    for (size_t t = 1; t < nt; ++t)
        if (!std::isfinite(betas_host[t]) || !(betas_host[t] < betas_host[t - 1]))
            return fail(KMC_ERR_BAD_ARG, "adaptive ladder: kmc_sampler_set_ladder: betas must be finite and strictly decreasing");
    for (size_t j = 0; j + 2 < nt; ++j)
        if (std::isnan(S_host[j])) return fail(KMC_ERR_BAD_ARG, "adaptive ladder: kmc_sampler_set_ladder: S must not be NaN");
    for (size_t t = 0; t + 1 < nt; ++t)
        if (round_acc_host[t] > (uint64_t)s->nrows) return fail(KMC_ERR_BAD_ARG, "adaptive ladder: kmc_sampler_set_ladder: round_acc counts at most nwalkers exchanges per pair");
    KMC_TRY(settle(s));
    std::vector<unsigned long long> tail(nt + 2, 0ull);                    // round_acc, then the ticket (0: between sweeps) and the rounds skipped
    for (size_t t = 0; t + 1 < nt; ++t) tail[t] = (unsigned long long)round_acc_host[t];
    tail[nt + 1] = (unsigned long long)*skipped_host;
    HIP_TRY(copy_sync(s->d_betas, betas_host, nt * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(copy_sync(s->d_S, S_host, (nt - 2) * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(copy_sync(s->d_round_acc, tail.data(), tail.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, s->stream));
    return KMC_OK;
}

KMC_EXPORT kmc_status kmc_sampler_get_positions(kmc_sampler* s, double* host)
{
    if (!s || !host) return fail(KMC_ERR_BAD_ARG, "null argument");
    KMC_TRY(settle(s, /*p2p_err=*/true));
    HIP_TRY(download_rows(s, host, s->d_pos, (size_t)s->nrows));
    return KMC_OK;
}

KMC_EXPORT kmc_status kmc_sampler_get_logp(kmc_sampler* s, double* host)
{
    if (!s || !host) return fail(KMC_ERR_BAD_ARG, "null argument");
    KMC_TRY(settle(s, /*p2p_err=*/true));
    HIP_TRY(copy_sync(host, s->d_logp, (size_t)s->nrows * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    return KMC_OK;
}

KMC_EXPORT kmc_status kmc_sampler_get_naccept(kmc_sampler* s, int64_t* host)
{
    if (!s || !host) return fail(KMC_ERR_BAD_ARG, "null argument");
    KMC_TRY(settle(s, /*p2p_err=*/true));
    HIP_TRY(download_u32(s, host, s->d_naccept, (size_t)s->nrows));
    return KMC_OK;
}

KMC_EXPORT kmc_status kmc_sampler_get_accept_ratio(kmc_sampler* s, double* host)
{
    if (!s || !host) return fail(KMC_ERR_BAD_ARG, "null argument");
    std::vector<int64_t> na((size_t)s->nrows);
    KMC_TRY(kmc_sampler_get_naccept(s, na.data()));
    const double denom = (double)(s->generation - s->cfg.nburnin);   // :291 (0 -> inf/nan like the reference)
    for (size_t i = 0; i < na.size(); ++i) host[i] = (double)na[i] / denom;
    return KMC_OK;
}

// ---- streaming moments (KMC_MOMENTS): one function per accumulator layout adds what the device holds into S / Q [ndim]; every one keeps
// its summation order (the sums are compared bit for bit: tests/test_gpu_state_routes.py) --------------------------------------------------
namespace {
hipError_t fetch(const kmc_sampler* s, const double* dev, size_t n, std::vector<double>* h)
{
    h->resize(n);
    return copy_sync(h->data(), dev, n * sizeof(double), hipMemcpyDeviceToHost, s->stream);
}

// rows [count][ld] of per-dimension sums, added up in row order: per walker (one launch per generation: laid out like the rows), per island
// (island and resident mode), per wave (half_step_staged with staged_tile_moments)
void add_rows(const double* hs, const double* hq, int64_t count, int64_t ld, int64_t nd, double* S, double* Q)
{
    for (int64_t r = 0; r < count; ++r)
        for (int64_t d = 0; d < nd; ++d) { S[(size_t)d] += hs[(size_t)(r * ld + d)]; Q[(size_t)d] += hq[(size_t)(r * ld + d)]; }
}

// transposed fold (kmc_kernels.hpp, FoldT; K == 2, L = 8 / 16 / 32): every lane of a wave owns NVL of the wave's 8 L / 64 * 64 sums -- sums and
// sums of squares in ONE array [nwaves][NVL][64], added up wave, then register, then lane
void add_transposed(const double* h, int L, int64_t nwaves, int64_t nd, double* S, double* Q)
{
    const int NVL = 8 * L / 64;
    for (int64_t w = 0; w < nwaves; ++w)
        for (int r = 0; r < NVL; ++r)
            for (int lane = 0; lane < 64; ++lane) {
                const int b3 = (lane >> 3) & 1, b4 = (lane >> 4) & 1, b5 = (lane >> 5) & 1;
                const int v = L == 8 ? 4 * b3 + 2 * b4 + b5 : L == 16 ? 4 * b4 + 2 * b5 + r : 4 * b5 + r;
                const int64_t d = 2 * ((int64_t)((v >> 1) & 1) * L + (lane & (L - 1))) + (v & 1);
                if (d >= nd) continue;
                const double x = h[(size_t)((w * NVL + r) * 64 + lane)];
                if (v >> 2) Q[(size_t)d] += x; else S[(size_t)d] += x;
            }
}
bool transposed(int L, int K) { return K == 2 && (L == 8 || L == 16 || L == 32); }

// the vector kernel's plain layout: per chunk k and thread t a pair of dimensions, [K][stride][2]
void add_striped(const double* hs, const double* hq, int L, int K, int64_t stride, int64_t nd, double* S, double* Q)
{
    for (int k = 0; k < K; ++k)
        for (int64_t t = 0; t < stride; ++t) {
            const int64_t d0 = 2 * ((int64_t)k * L + (t % L));
            const int64_t idx = 2 * ((int64_t)k * stride + t);
            if (d0 < nd) { S[(size_t)d0] += hs[(size_t)idx]; Q[(size_t)d0] += hq[(size_t)idx]; }
            if (d0 + 1 < nd) { S[(size_t)d0 + 1] += hs[(size_t)idx + 1]; Q[(size_t)d0 + 1] += hq[(size_t)idx + 1]; }
        }
}

// one walker per lane (half_step_generic; half_step_staged otherwise): columns [ndim][stride]
void add_columns(const double* hs, const double* hq, int64_t stride, int64_t nd, double* S, double* Q)
{
    for (int64_t d = 0; d < nd; ++d)
        for (int64_t t = 0; t < stride; ++t) { S[(size_t)d] += hs[(size_t)(d * stride + t)]; Q[(size_t)d] += hq[(size_t)(d * stride + t)]; }
}

// One launch per generation.  The lane-striped form credits a value when it is replaced (sojourn weights, like the two-launch kernels): every walker's
// CURRENT value still stands for the samples taken since its last move -- credited here, on the host, leaving the device state as it is.
kmc_status add_generation_sums(kmc_sampler* s, double* S, double* Q)
{
    const int64_t nd = s->cfg.ndim, nw = s->cfg.nwalkers, ld = s->ld;
    if (s->fused_fold) {
        const int64_t nwaves = s->nislands;
        std::vector<double> hs;
        HIP_TRY(fetch(s, s->d_isum, (size_t)(nwaves * (8 * s->fused_L / 64) * 64), &hs));
        add_transposed(hs.data(), s->fused_L, nwaves, nd, S, Q);
    } else {
        std::vector<double> hs, hq;                   // (freed before the rows below are fetched, as they always were: 2 x 2 MiB at 16 384 x 16)
        HIP_TRY(fetch(s, s->d_isum, (size_t)(ld * nw), &hs));
        HIP_TRY(fetch(s, s->d_isumsq, (size_t)(ld * nw), &hq));
        add_rows(hs.data(), hq.data(), nw, ld, nd, S, Q);
    }
    if (s->fused_L == 0) return KMC_OK;
    std::vector<double> hp;
    std::vector<uint32_t> kl((size_t)nw);
    HIP_TRY(fetch(s, s->d_pos, (size_t)(ld * nw), &hp));
    HIP_TRY(copy_sync(kl.data(), s->d_klast, kl.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    const uint32_t done = (uint32_t)samples_done(s);
    for (int64_t w = 0; w < nw; ++w) {
        const double wgt = (double)(done - kl[(size_t)w]);
        if (wgt == 0.0) continue;
        for (int64_t d = 0; d < nd; ++d) {
            const double x = hp[(size_t)(w * ld + d)];
            S[(size_t)d] += x * wgt;
            Q[(size_t)d] += (x * x) * wgt;
        }
    }
    return KMC_OK;
}

kmc_status add_island_sums(kmc_sampler* s, double* S, double* Q)
{
    const int64_t per = 4 * (int64_t)s->island_K, nd = s->cfg.ndim;
    std::vector<double> hs, hq;
    HIP_TRY(fetch(s, s->d_isum, (size_t)(s->nislands * per), &hs));
    HIP_TRY(fetch(s, s->d_isumsq, (size_t)(s->nislands * per), &hq));
    add_rows(hs.data(), hq.data(), s->nislands, per, nd < per ? nd : per, S, Q);
    return KMC_OK;
}

// two launches per generation, after flush_moments_now
kmc_status add_two_launch_sums(kmc_sampler* s, double* S, double* Q)
{
    const int64_t nd = s->cfg.ndim;
    std::vector<double> hs, hq;
    HIP_TRY(fetch(s, s->d_msum, (size_t)s->macc_elems, &hs));
    HIP_TRY(fetch(s, s->d_msumsq, (size_t)s->macc_elems, &hq));
    if (s->plan.vec && transposed(s->plan.L, s->plan.K)) add_transposed(hs.data(), s->plan.L, s->macc_stride / 64, nd, S, Q);
    else if (s->plan.vec) add_striped(hs.data(), hq.data(), s->plan.L, s->plan.K, s->macc_stride, nd, S, Q);
    else if (s->user && s->uk.staged != nullptr && staged_tile_moments((int)nd)) add_rows(hs.data(), hq.data(), s->macc_stride / 64, s->ld, nd, S, Q);
    else add_columns(hs.data(), hq.data(), s->macc_stride, nd, S, Q);
    return KMC_OK;
}

// The tail of every read-out, what was credited elsewhere: by temper_sweep when walkers left rung 0 ([2][ld] behind logp_sum; a ladder runs two
// launches per generation), and by a sampler until it stopped running one launch per generation (unfuse: carried on the host)
kmc_status add_credits_from_elsewhere(kmc_sampler* s, double* S, double* Q)
{
    const int64_t nd = s->cfg.ndim;
    if (s->temper && s->plan.vec) {
        std::vector<double> ts;
        HIP_TRY(fetch(s, s->d_tsum, 2 * (size_t)s->ld, &ts));
        for (int64_t d = 0; d < nd; ++d) { S[(size_t)d] += ts[(size_t)d]; Q[(size_t)d] += ts[(size_t)(s->ld + d)]; }
    }
    for (int64_t d = 0; !s->carry_sum.empty() && d < nd; ++d) { S[(size_t)d] += s->carry_sum[(size_t)d]; Q[(size_t)d] += s->carry_sumsq[(size_t)d]; }
    return KMC_OK;
}
}  // namespace

KMC_EXPORT kmc_status kmc_sampler_get_moments(kmc_sampler* s, double* sum, double* sumsq, int64_t* n)
{
    if (!s) return fail(KMC_ERR_BAD_ARG, "null sampler");
    if (!s->d_msum) return fail(KMC_ERR_BAD_ARG, "sampler was created without KMC_MOMENTS");
    HIP_TRY(hipSetDevice(s->cfg.device));
    const bool two_launch = !s->fused && !s->islands && !s->resident;
    if (two_launch) KMC_TRY(flush_moments_now(s));              // (launches on the stream: ahead of the drain)
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (two_launch) KMC_TRY(check_p2p_err(s));
    const size_t nd = (size_t)s->cfg.ndim;
    std::vector<double> S(nd, 0.0), Q(nd, 0.0);
    KMC_TRY(s->fused ? add_generation_sums(s, S.data(), Q.data()) : two_launch ? add_two_launch_sums(s, S.data(), Q.data()) : add_island_sums(s, S.data(), Q.data()));
    KMC_TRY(add_credits_from_elsewhere(s, S.data(), Q.data()));
    for (size_t d = 0; d < nd; ++d) {
        if (sum) sum[d] = S[d];
        if (sumsq) sumsq[d] = Q[d];
    }
    if (n) *n = (samples_done(s) - s->moment_base) * s->nlocal;
    return KMC_OK;
}

// Blobs of a body density with blobs (include/kissmcmc_hip.h): the current ones, and the stored series (KMC_STORE_BLOBS).
KMC_EXPORT kmc_status kmc_sampler_get_blobs(kmc_sampler* s, double* current, double* stored, int by_walker)
{
    if (!s) return fail(KMC_ERR_BAD_ARG, "null sampler");
    if (s->nblob == 0) return fail(KMC_ERR_BAD_ARG, "this sampler's density returns no blobs (kmc_user_density_create_body_blob)");
    KMC_TRY(settle(s));
    const size_t nb = (size_t)s->nblob;
    if (current) HIP_TRY(copy_sync(current, s->d_blob, (size_t)s->nrows * nb * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    if (stored) {
        if (!s->d_chain_blob && s->nsamples > 0) return fail(KMC_ERR_BAD_ARG, "sampler was created without KMC_STORE_BLOBS");
        const int64_t K = samples_done(s);
        if (K > 0) {
            if (by_walker) KMC_TRY(download_by_walker(s->d_chain_blob, false, s->nlocal, (int64_t)nb, (int64_t)nb, K, stored, s->stream));
            else HIP_TRY(copy_sync(stored, s->d_chain_blob, (size_t)K * (size_t)s->nlocal * nb * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        }
    }
    return KMC_OK;
}

KMC_EXPORT uint64_t kmc_deal_seed(uint64_t seed, int32_t deal_rank) { return deal_seed(seed, deal_rank); }

KMC_EXPORT kmc_status kmc_deal_perm(uint64_t seed, int64_t epoch, int32_t deal_rank, int64_t S, int64_t* A, int64_t* C)
{
    if (!A || !C || S < 2 || epoch < 0 || deal_rank < 0) return fail(KMC_ERR_BAD_ARG, "bad argument");
    deal_perm(seed, epoch, deal_rank, S, A, C);
    return KMC_OK;
}

DealArgs deal_args(kmc_sampler* s, void* buf)
{
    DealArgs a{};
    a.pos = s->d_pos; a.logp = s->d_logp; a.naccept = s->d_naccept; a.ids = s->d_ids;
    a.buf = static_cast<double*>(buf);
    a.S = s->nrows; a.A = 1; a.C = 0;
    a.ndim = (int32_t)s->cfg.ndim; a.ld = (int32_t)s->ld;
    return a;
}

KMC_EXPORT kmc_status kmc_sampler_deal_pack(kmc_sampler* s, int64_t epoch, void* send_dev)
{
    if (!s || !send_dev || epoch < 0) return fail(KMC_ERR_BAD_ARG, "bad argument");
    if (!s->d_ids) return fail(KMC_ERR_BAD_ARG, "sampler was created without kmc_config.deal_count");
    if (!s->positions_set) return fail(KMC_ERR_BAD_ARG, "kmc_sampler_set_positions has not succeeded yet");
    HIP_TRY(hipSetDevice(s->cfg.device));
    KMC_TRY(flush_moments_now(s));          // the accumulators are per slot: settle them before walkers change slots
    DealArgs a = deal_args(s, send_dev);
    deal_perm(s->user_seed, epoch, s->cfg.deal_rank, s->nrows, &a.A, &a.C);
    const int64_t n = a.S * ((int64_t)a.ndim + 2);
    hipLaunchKernelGGL(deal_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, a);
    HIP_TRY(hipGetLastError());
    return KMC_OK;
}

KMC_EXPORT kmc_status kmc_sampler_deal_unpack(kmc_sampler* s, const void* recv_dev)
{
    if (!s || !recv_dev) return fail(KMC_ERR_BAD_ARG, "bad argument");
    if (!s->d_ids) return fail(KMC_ERR_BAD_ARG, "sampler was created without kmc_config.deal_count");
    HIP_TRY(hipSetDevice(s->cfg.device));
    const DealArgs a = deal_args(s, const_cast<void*>(recv_dev));
    const int64_t n = a.S * ((int64_t)a.ndim + 2);
    hipLaunchKernelGGL(deal_unpack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, a);
    HIP_TRY(hipGetLastError());
    return KMC_OK;
}

KMC_EXPORT kmc_status kmc_sampler_get_walker_ids(kmc_sampler* s, int64_t* host)
{
    if (!s || !host) return fail(KMC_ERR_BAD_ARG, "null argument");
    KMC_TRY(settle(s));
    if (!s->d_ids) { for (int64_t i = 0; i < s->nrows; ++i) host[i] = i; return KMC_OK; }
    HIP_TRY(download_u32(s, host, s->d_ids, (size_t)s->nrows));
    return KMC_OK;
}

// dealt sub-ensembles, after kmc_sampler_set_state: which global walker each slot holds (a function of the restored generation's
// epoch alone: replay kmc_deal_perm on the host, distributed.deal_slot_ids)
KMC_EXPORT kmc_status kmc_sampler_set_walker_ids(kmc_sampler* s, const int64_t* host)
{
    if (!s || !host) return fail(KMC_ERR_BAD_ARG, "null argument");
    if (!s->d_ids) return fail(KMC_ERR_BAD_ARG, "sampler was created without kmc_config.deal_count");
    KMC_TRY(settle(s));
    for (int64_t i = 0; i < s->nrows; ++i)
        if (host[i] < 0 || host[i] >= (int64_t)1 << 32) return fail(KMC_ERR_BAD_ARG, "walker index out of range");
    HIP_TRY(upload_u32(s, s->d_ids, host, (size_t)s->nrows));
    return KMC_OK;
}

KMC_EXPORT kmc_status kmc_emcee_run(const kmc_config* cfg, const double* theta0, kmc_outputs* out)
{
    if (!cfg || !theta0 || !out) return fail(KMC_ERR_BAD_ARG, "null argument");
    kmc_config c = *cfg;
    if (out->chain) c.flags |= KMC_STORE_CHAIN;
    if (out->chain_logp) c.flags |= KMC_STORE_LOGP;
    if (out->blobs) c.flags |= KMC_STORE_BLOBS;
    if (out->sum || out->sumsq) c.flags |= KMC_MOMENTS;
    c.shard_rank = 0;
    c.shard_count = 1;
    const bool has_blobs = c.density == KMC_USER_DENSITY && c.user_density && static_cast<const kmc_user_density*>(c.user_density)->nblob > 0;
    if ((out->chain || out->chain_logp) && !has_blobs && c.dtype == KMC_F64 && !(c.flags & (KMC_ISLANDS | KMC_P2P)) && c.nthin > 0 && c.ngenerations > c.nburnin) {
        // a chain that does not fit the device is streamed to the caller's buffers while sampling (KMC_STREAM_CHAIN)
        size_t free_b = 0, total_b = 0;
        const size_t ns = (size_t)((c.ngenerations - c.nburnin) / c.nthin), nw_ = (size_t)c.nwalkers;
        const size_t need = ns * nw_ * ((out->chain ? (size_t)(c.ndim + (c.ndim & 1)) * sizeof(double) : 0) + (out->chain_logp ? sizeof(double) : 0));
        if (hipSetDevice(c.device) == hipSuccess && hipMemGetInfo(&free_b, &total_b) == hipSuccess && need > free_b / 10 * 8) c.flags |= KMC_STREAM_CHAIN;
        else (void)hipGetLastError();
    }
    kmc_sampler* s = nullptr;
    KMC_TRY(kmc_sampler_create(&c, &s));
    kmc_status st = KMC_OK;
    if (s->stream_chain) st = kmc_sampler_set_chain_host(s, out->chain, out->chain_logp);
    if (st == KMC_OK) st = kmc_sampler_set_positions(s, theta0);
    if (st == KMC_OK) st = kmc_sampler_run(s, c.ngenerations);
    if (st == KMC_OK) st = kmc_sampler_sync(s);
    if (st == KMC_OK) st = kmc_sampler_last_run_ms(s, &out->device_ms);
    if (st == KMC_OK && (out->chain || out->chain_logp))
        st = (c.flags & KMC_CHAIN_BY_WALKER) ? kmc_sampler_get_chain_by_walker(s, out->chain, out->chain_logp) : kmc_sampler_get_chain(s, out->chain, out->chain_logp);
    if (st == KMC_OK && out->blobs) st = kmc_sampler_get_blobs(s, nullptr, out->blobs, (c.flags & KMC_CHAIN_BY_WALKER) ? 1 : 0);
    if (st == KMC_OK && out->accept_ratio) st = kmc_sampler_get_accept_ratio(s, out->accept_ratio);
    if (st == KMC_OK && out->naccept) st = kmc_sampler_get_naccept(s, out->naccept);
    if (st == KMC_OK && out->final_pos) st = kmc_sampler_get_positions(s, out->final_pos);
    if (st == KMC_OK && out->final_logp) st = kmc_sampler_get_logp(s, out->final_logp);
    out->nmoment = 0;
    if (st == KMC_OK && (out->sum || out->sumsq)) st = kmc_sampler_get_moments(s, out->sum, out->sumsq, &out->nmoment);
    out->nsamples = s->nsamples;
    kmc_sampler_destroy(s);
    return st;
}

// ------------------------------------------------------------------------------------------
// stateless op
// ------------------------------------------------------------------------------------------
KMC_EXPORT kmc_status kmc_logpdf_eval(const kmc_config* cfg, const double* pos_dev, double* logp_dev,
                                      int64_t nrows, void* hip_stream)
{
    if (!cfg || !pos_dev || !logp_dev || nrows < 0) return fail(KMC_ERR_BAD_ARG, "bad argument");
    DensityParams dp;
    KMC_TRY(digest_params(*cfg, &dp));
    if (nrows == 0) return KMC_OK;
    const LogpdfArgs la{pos_dev, logp_dev, nrows, (int32_t)cfg->ndim, (int32_t)cfg->ndim, dp, nullptr};
    const unsigned grid = (unsigned)((nrows + 255) / 256);
    if (cfg->density == KMC_USER_DENSITY) {
        UserKernels uk;
        KMC_TRY(load_user(static_cast<kmc_user_density*>(cfg->user_density), UserModuleSpec::logpdf_only(cfg->ndim), &uk));
        const hipError_t e = launch_module(uk.logpdf, grid, 256u, (hipStream_t)hip_stream, la);
        if (e == hipSuccess) (void)hipStreamSynchronize((hipStream_t)hip_stream);   // (uk's hold on the module ends with this scope)
        HIP_TRY(e);
        return KMC_OK;
    }
    if (cfg->density == KMC_HOST_DENSITY) return fail(KMC_ERR_UNSUPPORTED, "KMC_HOST_DENSITY is evaluated by the caller, not on the device");
    if (cfg->density == KMC_DATA_DENSITY) {
        kmc_user_density* ud = static_cast<kmc_user_density*>(cfg->user_density);
        if (!ud->is_data) return fail(KMC_ERR_BAD_ARG, "KMC_DATA_DENSITY needs kmc_config.user_density made by kmc_data_density_create");
        if (cfg->ndim < 1 || cfg->ndim > kDataMaxDim) return fail(KMC_ERR_UNSUPPORTED, "KMC_DATA_DENSITY: ndim must be in 1 .. " + std::to_string(kDataMaxDim));
        DataKernels dk;
        KMC_TRY(load_data(ud, cfg->ndim, &dk));
        ScopedDeviceBlock part;
        const DataPlan plan = data_plan(ud, nrows);                  // (one plan for the allocation and the launch)
        const size_t part_doubles = (size_t)plan.nblocks * (size_t)nrows;
        HIP_TRY(part.alloc(part_doubles * sizeof(double)));
        HIP_TRY(launch_data_eval(dk, ud, plan, pos_dev, nrows, (int32_t)cfg->ndim, dp.p, part.as<double>(), part_doubles, logp_dev, (hipStream_t)hip_stream));
        HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));      // (the scratch and dk's hold on the module end with this scope)
        return KMC_OK;
    }
    const LogpdfFn lp = logpdf_fn(cfg->density);
    if (!lp) return fail(KMC_ERR_BAD_ARG, "unknown density id");
    hipLaunchKernelGGL(lp, dim3(grid), dim3(256), 0, (hipStream_t)hip_stream, la);
    HIP_TRY(hipGetLastError());
    return KMC_OK;
}

// Host-buffer convenience: logp[i] = log pdf(pos[i]) for dense host rows (used by the host shims for
// make_theta0s' `pdf(theta) > -Inf` test with runtime-compiled densities).
KMC_EXPORT kmc_status kmc_logpdf_eval_host(const kmc_config* cfg, const double* pos_host, double* logp_host, int64_t nrows)
{
    if (!cfg || !pos_host || !logp_host || nrows < 0) return fail(KMC_ERR_BAD_ARG, "bad argument");
    if (nrows == 0) return KMC_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return fail(KMC_ERR_NO_DEVICE, "no HIP device visible");
    }
    HIP_TRY(hipSetDevice(cfg->device));
    ScopedStream ss;
    HIP_TRY(ss.create());
    ScopedDeviceBlock dlp, dpos;                                     // (freed before the stream goes: dpos, then dlp)
    const size_t nb = (size_t)nrows * (size_t)cfg->ndim * sizeof(double);
    HIP_TRY(dpos.alloc(nb));
    HIP_TRY(dlp.alloc((size_t)nrows * sizeof(double)));
    HIP_TRY(copy_sync(dpos.p, pos_host, nb, hipMemcpyHostToDevice, ss.st));
    KMC_TRY(kmc_logpdf_eval(cfg, dpos.as<double>(), dlp.as<double>(), nrows, ss.st));
    HIP_TRY(hipStreamSynchronize(ss.st));
    HIP_TRY(copy_sync(logp_host, dlp.p, (size_t)nrows * sizeof(double), hipMemcpyDeviceToHost, ss.st));
    return KMC_OK;
}

// ... and the blobs with them (a body density with blobs; the reference's `pdf.(theta0s)` under hasblob=true, src/samplers.jl:209-210,
// and make_theta0s' `pdf(theta)[1]`, :336): blob_host [nrows][nblob].
KMC_EXPORT kmc_status kmc_logpdf_blob_eval_host(const kmc_config* cfg, const double* pos_host, double* logp_host, double* blob_host, int64_t nrows)
{
    if (!cfg || !pos_host || !logp_host || !blob_host || nrows < 0) return fail(KMC_ERR_BAD_ARG, "bad argument");
    const kmc_user_density* ud = cfg->density == KMC_USER_DENSITY ? static_cast<const kmc_user_density*>(cfg->user_density) : nullptr;
    if (!ud || ud->nblob == 0) return fail(KMC_ERR_BAD_ARG, "kmc_logpdf_blob_eval_host needs a body density with blobs (kmc_user_density_create_body_blob)");
    if (nrows == 0) return KMC_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return fail(KMC_ERR_NO_DEVICE, "no HIP device visible"); }
    HIP_TRY(hipSetDevice(cfg->device));
    DensityParams dp;
    KMC_TRY(digest_params(*cfg, &dp));
    ScopedStream ss;
    HIP_TRY(ss.create());
    const size_t nb = (size_t)nrows * (size_t)cfg->ndim * sizeof(double), bb = (size_t)nrows * (size_t)ud->nblob * sizeof(double);
    UserKernels uk;                                                  // (its hold on the module ends after the block is freed)
    ScopedDeviceBlock buf;
    HIP_TRY(buf.alloc(nb + (size_t)nrows * sizeof(double) + bb));
    double* dpos = buf.as<double>();
    double* dlp = dpos + (size_t)nrows * (size_t)cfg->ndim;
    double* dbl = dlp + nrows;
    KMC_TRY(load_user(const_cast<kmc_user_density*>(ud), UserModuleSpec::logpdf_only(cfg->ndim), &uk));
    HIP_TRY(copy_sync(dpos, pos_host, nb, hipMemcpyHostToDevice, ss.st));
    const LogpdfArgs la{dpos, dlp, nrows, (int32_t)cfg->ndim, (int32_t)cfg->ndim, dp, dbl};
    HIP_TRY(launch_module(uk.logpdf, (unsigned)((nrows + 255) / 256), 256u, ss.st, la));
    HIP_TRY(hipStreamSynchronize(ss.st));
    HIP_TRY(copy_sync(logp_host, dlp, (size_t)nrows * sizeof(double), hipMemcpyDeviceToHost, ss.st));
    HIP_TRY(copy_sync(blob_host, dbl, bb, hipMemcpyDeviceToHost, ss.st));
    return KMC_OK;
}

// The same on the chain a sampler holds on the device (KMC_STORE_CHAIN; the samples stored so far): no host round trip.
KMC_EXPORT kmc_status kmc_sampler_int_acorr(kmc_sampler* s, double c, double* tau, double* converged)
{
    if (!s) return fail(KMC_ERR_BAD_ARG, "null sampler");
    if (!s->d_chain) return fail(KMC_ERR_BAD_ARG, "sampler was created without KMC_STORE_CHAIN");
    if (s->stream_chain) return fail(KMC_ERR_UNSUPPORTED, "KMC_STREAM_CHAIN: the chain is on the host; use kmc_int_acorr on it");
    if (s->ld != s->cfg.ndim) return fail(KMC_ERR_UNSUPPORTED, "odd ndim: rows are padded on the device; use kmc_int_acorr on the downloaded chain");
    if (s->f32) return fail(KMC_ERR_UNSUPPORTED, "KMC_F32: the device chain is float; use kmc_int_acorr on the downloaded chain");
    KMC_TRY(settle(s));
    const int64_t ns = samples_done(s);
    KMC_TRY(int_acorr_check(ns, s->nlocal, s->cfg.ndim, c, tau, converged));
    return int_acorr_device(s->d_chain, ns, s->nlocal, s->cfg.ndim, c, tau, converged);
}

