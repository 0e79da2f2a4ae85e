// kmc_psis.hip -- PSIS-LOO of a data density over a stored chain (include/kissmcmc_hip.h), on the session of
// kmc_pointwise.hip: kmc_*_psis_loo and the read-out of its tails kmc_*_psis_tail with one r_eff; kmc_*_psis_loo_reff and
// kmc_*_psis_tail_reff with a relative efficiency per observation, supplied or computed from the chain (reff_stage).  psis() is the
// stages in order: the tail lengths, the host lppd_j, the work space of a block, then per block the launches and the read-out.  The plan
// (kmc_psis_plan) and the host stages (kmc_loo_stats, kmc_psis_smooth_host): kmc_pointwise_stages.hip.  Kernels: kmc_pointwise.hpp (the
// walks, in the runtime-compiled module) and kmc_psis_fit.hpp (the fit, compiled here with the fold).
#include <type_traits>

#include "kmc_pointwise_host.hpp"

using namespace kmc_pw_host;

namespace {

__global__ __launch_bounds__(256) void psis_fold(const PsisArgs q, int stage) { psis_fold_body(q, stage); }
__global__ __launch_bounds__(kmc_psis::kFitLanes) void psis_fit_kernel(const PsisArgs q, int sort_len) { psis_fit_body(q, sort_len); }

// what one call hands back, each [obs.count] or nullptr
struct PsisOut {
    double* res = nullptr;        // [4][obs.count]: elpd_loo_j, pareto_k, n_tail_j, sigma_j
    double* lppd_j = nullptr;     // the statistics' passes run only when this is asked for
    double* tail = nullptr;       // [obs.count][M]
    double *m = nullptr, *xc = nullptr;
    int32_t* n_tail = nullptr;
    int64_t* tail_len = nullptr;
    double* r_eff = nullptr;      // a per-observation r_eff: as computed (NaN where it has none) or as supplied
    int64_t *tail_len_j = nullptr, *n_reff_nan = nullptr;
};

// nanoseconds of the stages ahead of the blocks, for info: the statistics' passes; the weight passes, the ESS stage, groups
struct PsisLead {
    int64_t ns_stats = 0, reff[3] = {};
};

// The tail lengths: the statistics' passes where lppd_j or the chain's r_eff needs them, the relative efficiency from the chain, then M
// (the longest tail) with the read-outs of r_eff, tail_len_j and n_reff_nan, and the check of the caller's tail array.
kmc_status resolve_tails(PwSession& S, const PwRequest& q, const PsisOut& out, bool timed, PsisLead* lead, int64_t* M_out)
{
    const int64_t n = S.n, count = q.obs.count;
    if (out.lppd_j || q.computed_reff()) {
        int64_t sinfo[6] = {};
        KMC_TRY(pw_stats(S, &S.b.work, timed && out.lppd_j ? sinfo : nullptr, out.lppd_j ? 2 : 1));
        lead->ns_stats = sinfo[4] + sinfo[5];
    }
    if (q.computed_reff()) {
        std::vector<double> r((size_t)count);
        ReffOut ro;
        ro.r_eff = r.data();
        KMC_TRY(reff_stage(S, q, ro, timed ? lead->reff : nullptr));
        if (out.r_eff) std::copy(r.begin(), r.end(), out.r_eff);
        KMC_TRY(tail_lengths(n, q.obs.first, r.data(), count, &S));
    } else if (q.supplied_reff() && out.r_eff) {
        std::copy(S.r_used.begin(), S.r_used.end(), out.r_eff);
    }
    int64_t M = 0;
    if (S.Mj.empty()) KMC_TRY(psis_check(n, q.r_eff, &M));
    else M = *std::max_element(S.Mj.begin(), S.Mj.end());
    if (out.tail_len_j) for (int64_t c = 0; c < count; ++c) out.tail_len_j[c] = S.Mj.empty() ? M : S.Mj[(size_t)c];
    if (out.n_reff_nan) *out.n_reff_nan = S.n_reff_nan;
    if (out.tail) {
        if (!out.tail_len) return fail(KMC_ERR_BAD_ARG, "null argument");
        if (*out.tail_len < M)
            return fail(KMC_ERR_BAD_ARG, "the tail array has " + std::to_string(*out.tail_len) + " columns, the tail length is " + std::to_string(M));
        *out.tail_len = M;
    }
    *M_out = M;
    return KMC_OK;
}

// lppd_j of the range, from the statistics on the device by the host stage of WAIC
kmc_status host_lppd(PwSession& S, const PwRequest& q, double* lppd_j)
{
    const int64_t J = S.J;
    std::vector<double> stats(4 * (size_t)J), lp((size_t)J), totals(7);
    HIP_TRY(copy_sync(stats.data(), S.a.stats, stats.size() * sizeof(double), hipMemcpyDeviceToHost, S.ss.get()));
    KMC_TRY(kmc_waic_stats(J, S.n, stats.data(), lp.data(), nullptr, nullptr, totals.data()));
    std::copy(lp.begin() + q.obs.first, lp.begin() + q.obs.first + q.obs.count, lppd_j);
    return KMC_OK;
}

// The work space of one block of B observations with R runs and tails of M draws: ONE list of (member of PsisArgs, bytes), in order of
// alignment, from which both the size and the carving follow.
struct PsisWorkspace {
    size_t B, R, M;
    template <class F>
    void each(PsisArgs& qa, F f) const
    {
        f(qa.tail, B * M * 8); f(qa.runval, R * B * 8); f(qa.m, B * 8); f(qa.xc, B * 8); f(qa.prefix, B * 8); f(qa.rank, B * 8);
        f(qa.res, B * 32); f(qa.counts, R * B * kmc_psis::kSelectBins * 4); f(qa.cursor, B * 4);
    }
    size_t bytes() const
    {
        PsisArgs qa{};
        size_t sum = 0;
        each(qa, [&](auto*&, size_t b) { sum += b; });
        return sum;
    }
    void carve(void* base, PsisArgs& qa) const
    {
        char* p = static_cast<char*>(base);
        each(qa, [&](auto*& member, size_t b) { member = reinterpret_cast<std::remove_reference_t<decltype(member)>>(p); p += b; });
    }
};

// the launches of one block of bc observations (qa.a.obs_first, qa.a.obs_count, qa.Mj set): the minimum, the select passes, the gather,
// the fit; ev (or nullptr) gets the five events around them
kmc_status psis_block(const PwSession& S, PsisArgs& qa, int64_t bc, int sort_len, TimedEvents<5>* ev)
{
    const PwPlan& pl = S.pl;
    hipStream_t st = S.ss.get();
    const unsigned gy = (unsigned)((pl.nwaves + kPwWaves - 1) / kPwWaves);
    const unsigned gx = pl.packed ? 1u : (unsigned)((bc + 63) / 64), gf = (unsigned)((bc + 255) / 256);
    const int pk = pl.packed ? 1 : 0;
    if (ev) HIP_TRY(hipEventRecord(ev->e[0], st));
    HIP_TRY(launch_module_y(S.pk.psis[0][pk], gx, gy, kPwThreads, st, qa));
    hipLaunchKernelGGL(psis_fold, dim3(gf), dim3(256), 0, st, qa, 0);
    HIP_TRY(hipGetLastError());
    if (ev) HIP_TRY(hipEventRecord(ev->e[1], st));
    for (int pass = 0; pass < kmc_psis::kSelectPasses; ++pass) {
        qa.shift = 64 - kmc_psis::kSelectBits * (pass + 1);
        HIP_TRY(launch_module_y(S.pk.psis[1][pk], gx, gy, kPwThreads, st, qa));
        hipLaunchKernelGGL(psis_fold, dim3(gf), dim3(256), 0, st, qa, 1);
        HIP_TRY(hipGetLastError());
    }
    if (ev) HIP_TRY(hipEventRecord(ev->e[2], st));
    HIP_TRY(launch_module_y(S.pk.psis[2][pk], gx, gy, kPwThreads, st, qa));
    if (ev) HIP_TRY(hipEventRecord(ev->e[3], st));
    hipLaunchKernelGGL(psis_fit_kernel, dim3((unsigned)bc), dim3(kmc_psis::kFitLanes), 0, st, qa, sort_len);
    HIP_TRY(hipGetLastError());
    if (ev) HIP_TRY(hipEventRecord(ev->e[4], st));
    return KMC_OK;
}

// one block's results [4][bc] into the caller's arrays at b0; adds the block's log1p evaluations to *log1ps
void psis_unpack(const double* res_host, int64_t b0, int64_t bc, int64_t count, const PsisOut& out, int64_t* log1ps)
{
    for (int64_t c = 0; c < bc; ++c) {
        const double nt = res_host[2 * (size_t)bc + (size_t)c];
        if (out.res) for (int k = 0; k < 4; ++k) out.res[k * count + b0 + c] = res_host[(size_t)k * (size_t)bc + (size_t)c];
        if (out.n_tail) out.n_tail[b0 + c] = nt == nt ? (int32_t)nt : -1;
        if (nt >= kmc_psis::kMinFit) *log1ps += (int64_t)nt * (31 + (int64_t)std::floor(std::sqrt(nt)));
    }
}

// what one call did, for info; ns: nanoseconds of the minimum, the select passes, the gather and the fit over all blocks
void psis_info(const PwSession& S, const PwRequest& q, int64_t M, int64_t nblocks, int64_t block, const int64_t ns[4], int64_t log1ps, const PsisLead& lead,
               int64_t* info)
{
    info[0] = S.n; info[1] = M; info[2] = nblocks; info[3] = block;
    for (int k = 0; k < 4; ++k) info[4 + k] = ns[k];
    info[8] = S.n * q.obs.count; info[9] = log1ps; info[10] = lead.ns_stats; info[11] = S.pl.nruns;
    if (q.per_observation_reff()) { info[12] = lead.reff[0]; info[13] = lead.reff[1]; info[14] = lead.reff[2]; info[15] = S.n_reff_nan; }
}

kmc_status psis(const ChainSource& src, const PwRequest& q, const PsisOut& out, int64_t* n_out, int64_t* info)
{
    PwSession S;
    KMC_TRY(pw_open(src, q, out.res ? (const void*)out.res : (const void*)out.tail, &S));
    const int64_t count = q.obs.count;
    if (n_out) *n_out = S.n;
    hipStream_t st = S.ss.get();
    PsisLead lead;
    int64_t M = 0;
    KMC_TRY(resolve_tails(S, q, out, info != nullptr, &lead, &M));
    const PsisPlan pp = psis_plan(M, S.pl, q.workspace);
    const int64_t block = std::min(pp.block, S.pl.packed ? (int64_t)64 : count);
    if (out.lppd_j) KMC_TRY(host_lppd(S, q, out.lppd_j));

    const PsisWorkspace ws{(size_t)block, (size_t)S.pl.nruns, (size_t)M};
    KMC_TRY(check_device_room(ws.bytes(), "the PSIS-LOO work space"));
    HIP_TRY(hipMalloc(&S.b.work2, ws.bytes()));
    if (!S.Mj.empty()) {
        HIP_TRY(hipMalloc((void**)&S.b.Mj, (size_t)count * sizeof(int32_t)));
        HIP_TRY(copy_sync(S.b.Mj, S.Mj.data(), (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    PsisArgs qa{};
    qa.a = S.a;
    qa.M = (int32_t)M;
    ws.carve(S.b.work2, qa);
    TimedEvents<5> ev;
    if (info) HIP_TRY(ev.create());
    int64_t ns[4] = {}, nblocks = 0, log1ps = 0;
    std::vector<double> res_host(4 * (size_t)block);
    for (int64_t b0 = 0; b0 < count; b0 += block, ++nblocks) {
        const int64_t bc = std::min(block, count - b0);
        qa.a.obs_first = q.obs.first + b0;
        qa.a.obs_count = bc;
        qa.Mj = S.b.Mj ? S.b.Mj + b0 : nullptr;
        KMC_TRY(psis_block(S, qa, bc, pp.sort_len, info ? &ev : nullptr));
        HIP_TRY(copy_sync(res_host.data(), qa.res, 4 * (size_t)bc * sizeof(double), hipMemcpyDeviceToHost, st));
        psis_unpack(res_host.data(), b0, bc, count, out, &log1ps);
        if (out.tail) HIP_TRY(copy_sync(out.tail + b0 * M, qa.tail, (size_t)bc * (size_t)M * sizeof(double), hipMemcpyDeviceToHost, st));
        if (out.m) HIP_TRY(copy_sync(out.m + b0, qa.m, (size_t)bc * sizeof(double), hipMemcpyDeviceToHost, st));
        if (out.xc) HIP_TRY(copy_sync(out.xc + b0, qa.xc, (size_t)bc * sizeof(double), hipMemcpyDeviceToHost, st));
        if (info)
            for (int k = 0; k < 4; ++k) {
                int64_t t = 0;
                HIP_TRY(ev.elapsed_ns(k, k + 1, &t));
                ns[k] += t;
            }
    }
    if (info) psis_info(S, q, M, nblocks, block, ns, log1ps, lead, info);
    return KMC_OK;
}

// the relative efficiency of a PSIS-LOO call: one value, or per observation -- supplied, or computed from the chain where r_eff_j is null
struct PsisReff {
    ReffFrom from;
    double r_eff;
    const double* r_eff_j;
    bool split;
    int64_t max_lag;
};
PsisReff one_reff(double r_eff) { return {ReffFrom::One, r_eff, nullptr, true, 0}; }
PsisReff reff_per_obs(const double* r_j, int32_t split, int64_t max_lag) { return {r_j ? ReffFrom::Supplied : ReffFrom::Chain, 1.0, r_j, split != 0, max_lag}; }
// ... and what the *_reff forms hand back about it
struct ReffUsed {
    double* r_eff = nullptr;
    int64_t *tail_len_j = nullptr, *n_reff_nan = nullptr;
};

kmc_status psis_request(PwRequest* q, const PwDensity& d, const Selection& sel, const PsisReff& r, const ObsRange& obs, int64_t workspace)
{
    KMC_TRY(q->begin(PwMode::Psis, d, sel));
    q->reff = r.from; q->r_eff = r.r_eff; q->r_eff_j = r.r_eff_j; q->split = r.split; q->max_lag = r.max_lag;
    q->obs = obs; q->workspace = workspace;
    return KMC_OK;
}

// kmc_*_psis_loo and kmc_*_psis_loo_reff
kmc_status psis_loo(const ChainSource& src, const PwDensity& d, const Selection& sel, const PsisReff& r, const ObsRange& obs, int64_t workspace, double* stats,
                    double* lppd_j, const ReffUsed& used, int64_t* n_out, int64_t* info)
{
    PwRequest q;
    KMC_TRY(psis_request(&q, d, sel, r, obs, workspace));
    if (!lppd_j) return fail(KMC_ERR_BAD_ARG, "null argument");
    PsisOut out;
    out.res = stats; out.lppd_j = lppd_j; out.r_eff = used.r_eff; out.tail_len_j = used.tail_len_j; out.n_reff_nan = used.n_reff_nan;
    return psis(src, q, out, n_out, info);
}

// kmc_*_psis_tail and kmc_*_psis_tail_reff
kmc_status psis_tail(const ChainSource& src, const PwDensity& d, const Selection& sel, const PsisReff& r, const ObsRange& obs, int64_t workspace, double* tail,
                     double* m_j, double* xc_j, int32_t* n_tail_j, int64_t* tail_len, const ReffUsed& used, int64_t* n_out)
{
    PwRequest q;
    KMC_TRY(psis_request(&q, d, sel, r, obs, workspace));
    PsisOut out;
    out.tail = tail; out.m = m_j; out.xc = xc_j; out.n_tail = n_tail_j; out.tail_len = tail_len;
    out.r_eff = used.r_eff; out.tail_len_j = used.tail_len_j; out.n_reff_nan = used.n_reff_nan;
    return psis(src, q, out, n_out, nullptr);
}

}  // namespace

KMC_EXPORT kmc_status kmc_sampler_psis_loo(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int64_t thin, double r_eff, int64_t obs_first,
                                           int64_t obs_count, int64_t workspace_bytes, double* stats, double* lppd_j, int64_t* n_out, int64_t* info)
{
    return psis_loo(ChainSource(s, false, "kmc_chain_psis_loo"), sampler_density(s), {first_sample, walker_mask, thin}, one_reff(r_eff), {obs_first, obs_count},
                    workspace_bytes, stats, lppd_j, {}, n_out, info);
}

KMC_EXPORT kmc_status kmc_chain_psis_loo(kmc_user_density* density, const double* params, const double* chain_host, int64_t nsamples, int64_t nwalkers,
                                         int64_t ndim, int64_t first_sample, const uint8_t* walker_mask, int64_t thin, double r_eff, int64_t obs_first,
                                         int64_t obs_count, int64_t workspace_bytes, int device, double* stats, double* lppd_j, int64_t* n_out, int64_t* info)
{
    return psis_loo(ChainSource(chain_host, nullptr, nsamples, nwalkers, ndim, device), {density, params}, {first_sample, walker_mask, thin}, one_reff(r_eff),
                    {obs_first, obs_count}, workspace_bytes, stats, lppd_j, {}, n_out, info);
}

KMC_EXPORT kmc_status kmc_sampler_psis_tail(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int64_t thin, double r_eff, int64_t obs_first,
                                            int64_t obs_count, int64_t workspace_bytes, double* tail, double* m_j, double* xc_j, int32_t* n_tail_j,
                                            int64_t* tail_len, int64_t* n_out)
{
    return psis_tail(ChainSource(s, false, "kmc_chain_psis_tail"), sampler_density(s), {first_sample, walker_mask, thin}, one_reff(r_eff), {obs_first, obs_count},
                     workspace_bytes, tail, m_j, xc_j, n_tail_j, tail_len, {}, n_out);
}

KMC_EXPORT kmc_status kmc_chain_psis_tail(kmc_user_density* density, const double* params, const double* chain_host, int64_t nsamples, int64_t nwalkers,
                                          int64_t ndim, int64_t first_sample, const uint8_t* walker_mask, int64_t thin, double r_eff, int64_t obs_first,
                                          int64_t obs_count, int64_t workspace_bytes, int device, double* tail, double* m_j, double* xc_j,
                                          int32_t* n_tail_j, int64_t* tail_len, int64_t* n_out)
{
    return psis_tail(ChainSource(chain_host, nullptr, nsamples, nwalkers, ndim, device), {density, params}, {first_sample, walker_mask, thin}, one_reff(r_eff),
                     {obs_first, obs_count}, workspace_bytes, tail, m_j, xc_j, n_tail_j, tail_len, {}, n_out);
}

KMC_EXPORT kmc_status kmc_sampler_psis_loo_reff(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int64_t thin, const double* r_eff_j,
                                                int32_t split, int64_t max_lag, int64_t obs_first, int64_t obs_count, int64_t workspace_bytes,
                                                double* stats, double* lppd_j, double* r_eff_used, int64_t* tail_len_j, int64_t* n_reff_nan,
                                                int64_t* n_out, int64_t* info)
{
    return psis_loo(ChainSource(s, false, "kmc_chain_psis_loo_reff"), sampler_density(s), {first_sample, walker_mask, thin}, reff_per_obs(r_eff_j, split, max_lag),
                    {obs_first, obs_count}, workspace_bytes, stats, lppd_j, {r_eff_used, tail_len_j, n_reff_nan}, n_out, info);
}

KMC_EXPORT kmc_status kmc_chain_psis_loo_reff(kmc_user_density* density, const double* params, const double* chain_host, int64_t nsamples,
                                              int64_t nwalkers, int64_t ndim, int64_t first_sample, const uint8_t* walker_mask, int64_t thin,
                                              const double* r_eff_j, int32_t split, int64_t max_lag, int64_t obs_first, int64_t obs_count,
                                              int64_t workspace_bytes, int device, double* stats, double* lppd_j, double* r_eff_used,
                                              int64_t* tail_len_j, int64_t* n_reff_nan, int64_t* n_out, int64_t* info)
{
    return psis_loo(ChainSource(chain_host, nullptr, nsamples, nwalkers, ndim, device), {density, params}, {first_sample, walker_mask, thin},
                    reff_per_obs(r_eff_j, split, max_lag), {obs_first, obs_count}, workspace_bytes, stats, lppd_j, {r_eff_used, tail_len_j, n_reff_nan}, n_out, info);
}

KMC_EXPORT kmc_status kmc_sampler_psis_tail_reff(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int64_t thin, const double* r_eff_j,
                                                 int32_t split, int64_t max_lag, int64_t obs_first, int64_t obs_count, int64_t workspace_bytes,
                                                 double* tail, double* m_j, double* xc_j, int32_t* n_tail_j, int64_t* tail_len, double* r_eff_used,
                                                 int64_t* tail_len_j, int64_t* n_reff_nan, int64_t* n_out)
{
    return psis_tail(ChainSource(s, false, "kmc_chain_psis_tail_reff"), sampler_density(s), {first_sample, walker_mask, thin}, reff_per_obs(r_eff_j, split, max_lag),
                     {obs_first, obs_count}, workspace_bytes, tail, m_j, xc_j, n_tail_j, tail_len, {r_eff_used, tail_len_j, n_reff_nan}, n_out);
}

KMC_EXPORT kmc_status kmc_chain_psis_tail_reff(kmc_user_density* density, const double* params, const double* chain_host, int64_t nsamples,
                                               int64_t nwalkers, int64_t ndim, int64_t first_sample, const uint8_t* walker_mask, int64_t thin,
                                               const double* r_eff_j, int32_t split, int64_t max_lag, int64_t obs_first, int64_t obs_count,
                                               int64_t workspace_bytes, int device, double* tail, double* m_j, double* xc_j, int32_t* n_tail_j,
                                               int64_t* tail_len, double* r_eff_used, int64_t* tail_len_j, int64_t* n_reff_nan, int64_t* n_out)
{
    return psis_tail(ChainSource(chain_host, nullptr, nsamples, nwalkers, ndim, device), {density, params}, {first_sample, walker_mask, thin},
                     reff_per_obs(r_eff_j, split, max_lag), {obs_first, obs_count}, workspace_bytes, tail, m_j, xc_j, n_tail_j, tail_len,
                     {r_eff_used, tail_len_j, n_reff_nan}, n_out);
}
