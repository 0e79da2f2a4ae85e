// kmc_pointwise_stages.hip -- the parts of the pointwise log-likelihood and of PSIS-LOO that touch no device: the cut of a call
// (kmc_pointwise_plan, kmc_psis_plan; DESIGN.md sections 4k and 4l), the refusals and tail lengths that follow from the sizes alone, and
// the host stages in the operation order of include/kissmcmc_hip.h (kmc_waic_stats, kmc_loo_stats, kmc_psis_smooth_host).  The device
// side: kmc_pointwise.hip, kmc_psis.hip.
#include "kmc_pointwise_host.hpp"

namespace kmc_pw_host {

PwPlan pw_plan(int64_t n, int64_t J)
{
    PwPlan p;
    p.packed = J < 64;
    if (p.packed) {
        p.jp_log2 = 0;
        while (((int64_t)1 << p.jp_log2) < J) ++p.jp_log2;
        p.lanes = 1 << p.jp_log2;
        p.slots = 64 / p.lanes;
    }
    const int64_t groups = (J + 63) / 64;
    const int64_t max_runs = std::max<int64_t>(1, kPwTargetWaves / groups);
    p.run_len = std::max(kPwMinRun, (n + max_runs - 1) / max_runs);
    p.nruns = (n + p.run_len - 1) / p.run_len;
    p.nwaves = (p.nruns + p.slots - 1) / p.slots;
    return p;
}

// the refusals PSIS-LOO adds, from the sizes alone; M: the tail length
kmc_status psis_check(int64_t n, double r_eff, int64_t* M, bool sizes_only)
{
    if (sizes_only) r_eff = 1.0;
    if (!(r_eff > 0.0) || !std::isfinite(r_eff)) return fail(KMC_ERR_BAD_ARG, "r_eff must be finite and > 0 (r_eff = " + std::to_string(r_eff) + ")");
    if (n < kmc_psis::kMinFit) return fail(KMC_ERR_BAD_ARG, "PSIS-LOO needs at least 5 selected rows (n = " + std::to_string(n) + ")");
    if (n >= ((int64_t)1 << 31)) return fail(KMC_ERR_UNSUPPORTED, "too many rows for one PSIS-LOO call: n = " + std::to_string(n) + ", the limit is 2^31");
    const int64_t m = kmc_psis::tail_length(n, r_eff);
    if (m > kmc_psis::kMaxTail && !sizes_only)                                         // (a per-observation r_eff: tail_lengths decides)
        return fail(KMC_ERR_UNSUPPORTED, "a tail of M = " + std::to_string(m) + " draws (n / r_eff = " + std::to_string((double)n / r_eff) + ") is longer than " +
                                             std::to_string(kmc_psis::kMaxTail) + ", what one workgroup sorts: thin the chain");
    if (M) *M = m;
    return KMC_OK;
}

PsisPlan psis_plan(int64_t M, const PwPlan& pl, int64_t workspace)
{
    PsisPlan p;
    p.M = M;
    p.m_est = 30 + (int64_t)std::floor(std::sqrt((double)M));
    while (p.sort_len < M) p.sort_len <<= 1;
    p.per_obs = (size_t)M * 8 + (size_t)pl.nruns * (8 + 4 * kmc_psis::kSelectBins) + 8 * 8 + 8;
    p.block = std::max<int64_t>(64, workspace_budget(workspace) / (int64_t)p.per_obs / 64 * 64);
    return p;
}

// the tail lengths of a per-observation r_eff, and the refusal of one longer than a workgroup sorts
kmc_status tail_lengths(int64_t n, int64_t obs_first, const double* r, int64_t count, PwSession* S)
{
    S->r_used.assign(r, r + count);
    S->Mj.assign((size_t)count, 0);
    S->n_reff_nan = 0;
    for (int64_t c = 0; c < count; ++c) {
        double& rc = S->r_used[(size_t)c];
        if (!(rc > 0.0) || !std::isfinite(rc)) { rc = 1.0; ++S->n_reff_nan; }
        const int64_t m = kmc_psis::tail_length(n, rc);
        if (m > kmc_psis::kMaxTail)
            return fail(KMC_ERR_UNSUPPORTED, "observation " + std::to_string(obs_first + c) + ": a tail of M = " + std::to_string(m) + " draws (n = " + std::to_string(n) +
                                                 ", r_eff_j = " + std::to_string(rc) + ") is longer than " + std::to_string(kmc_psis::kMaxTail) +
                                                 ", what one workgroup sorts: thin the chain");
        S->Mj[(size_t)c] = (int32_t)m;
    }
    return KMC_OK;
}

// the data-density contract's pairwise tree over v[0 .. m), in index order: each level adds neighbours, an odd last element passes up
double pairwise_tree(std::vector<double>& v)
{
    size_t m = v.size();
    while (m > 1) {
        const size_t half = m / 2;
        for (size_t i = 0; i < half; ++i) v[i] = v[2 * i] + v[2 * i + 1];
        if (m & 1) v[half] = v[m - 1];
        m = half + (m & 1);
    }
    return v[0];
}

}  // namespace kmc_pw_host

using namespace kmc_pw_host;

// The cut of the two passes; for tests and benchmarks.  Touches no device.
KMC_EXPORT kmc_status kmc_pointwise_plan(int64_t n, int64_t ndata, int64_t* run_len, int64_t* nruns, int32_t* lanes_per_run, int32_t* slots,
                                         int64_t* nwaves)
{
    if (n < 2) return fail(KMC_ERR_BAD_ARG, "need n >= 2 (n = " + std::to_string(n) + ")");
    if (n >= ((int64_t)1 << 40)) return fail(KMC_ERR_UNSUPPORTED, "too many rows for one pointwise call: n = " + std::to_string(n) + ", the limit is 2^40");
    if (ndata < 1 || ndata > kDataMaxRows) return fail(KMC_ERR_BAD_ARG, "ndata must be in 1 .. 2^30 (ndata = " + std::to_string(ndata) + ")");
    const PwPlan p = pw_plan(n, ndata);
    if (run_len) *run_len = p.run_len;
    if (nruns) *nruns = p.nruns;
    if (lanes_per_run) *lanes_per_run = p.lanes;
    if (slots) *slots = p.slots;
    if (nwaves) *nwaves = p.nwaves;
    return KMC_OK;
}

// The host stage, in the operation order of include/kissmcmc_hip.h.  No device; no fused multiply-add (the library is built with
// -ffp-contract=off).  totals: lppd, p_waic, elpd_waic, se, waic, n_high, n_nan.
KMC_EXPORT kmc_status kmc_waic_stats(int64_t J, int64_t n, const double* stats, double* lppd_j, double* p_waic_j, double* elpd_j, double* totals)
{
    if (J < 1) return fail(KMC_ERR_BAD_ARG, "need J >= 1 (J = " + std::to_string(J) + ")");
    if (n < 2) return fail(KMC_ERR_BAD_ARG, "need n >= 2 (n = " + std::to_string(n) + ")");
    if (!stats || !totals) return fail(KMC_ERR_BAD_ARG, "null argument");
    const double *M = stats, *S1 = stats + J, *E = stats + 2 * J, *V = stats + 3 * J;
    const double logn = std::log((double)n), nm1 = (double)(n - 1), dJ = (double)J;
    std::vector<double> lp((size_t)J), pw((size_t)J), el((size_t)J), t((size_t)J);
    int64_t n_high = 0, n_nan = 0;
    for (int64_t j = 0; j < J; ++j) {
        lp[(size_t)j] = M[j] + (std::log(E[j]) - logn);
        pw[(size_t)j] = V[j] / nm1;
        el[(size_t)j] = lp[(size_t)j] - pw[(size_t)j];
        n_high += pw[(size_t)j] > 0.4;
        n_nan += std::isnan(S1[j]);
    }
    if (lppd_j) std::copy(lp.begin(), lp.end(), lppd_j);
    if (p_waic_j) std::copy(pw.begin(), pw.end(), p_waic_j);
    if (elpd_j) std::copy(el.begin(), el.end(), elpd_j);
    t = lp; totals[0] = pairwise_tree(t);
    t = pw; totals[1] = pairwise_tree(t);
    t = el; totals[2] = pairwise_tree(t);
    const double centre = totals[2] / dJ;
    for (int64_t j = 0; j < J; ++j) { const double dv = el[(size_t)j] - centre; t[(size_t)j] = dv * dv; }
    totals[3] = std::sqrt(dJ * pairwise_tree(t) / (double)(J - 1));
    totals[4] = -2.0 * totals[2];
    totals[5] = (double)n_high;
    totals[6] = (double)n_nan;
    return KMC_OK;
}

// The cut of a PSIS-LOO call; touches no device.
KMC_EXPORT kmc_status kmc_psis_plan(int64_t n, int64_t ndata, double r_eff, int64_t workspace_bytes, int64_t* tail_len, int64_t* m_est,
                                    int64_t* obs_per_block, int64_t* passes)
{
    if (ndata < 1 || ndata > kDataMaxRows) return fail(KMC_ERR_BAD_ARG, "ndata must be in 1 .. 2^30 (ndata = " + std::to_string(ndata) + ")");
    if (workspace_bytes < 0) return fail(KMC_ERR_BAD_ARG, "workspace_bytes must be >= 0 (workspace_bytes = " + std::to_string(workspace_bytes) + ")");
    int64_t M = 0;
    KMC_TRY(psis_check(n, r_eff, &M));
    const PsisPlan p = psis_plan(M, pw_plan(n, ndata), workspace_bytes);
    if (tail_len) *tail_len = p.M;
    if (m_est) *m_est = p.m_est;
    if (obs_per_block) *obs_per_block = p.block;
    if (passes) *passes = p.passes;
    return KMC_OK;
}

// The host stage, in the operation order of include/kissmcmc_hip.h.  stats [4][J]: elpd_loo_j, pareto_k, n_tail_j, sigma_j.
// totals: elpd_loo, se, p_loo, looic, lppd, n_nan, k_counts[4].
KMC_EXPORT kmc_status kmc_loo_stats(int64_t J, int64_t n, const double* stats, const double* lppd_j, double* p_loo_j, double* totals)
{
    if (J < 1) return fail(KMC_ERR_BAD_ARG, "need J >= 1 (J = " + std::to_string(J) + ")");
    if (n < kmc_psis::kMinFit) return fail(KMC_ERR_BAD_ARG, "need n >= 5 (n = " + std::to_string(n) + ")");
    if (!stats || !lppd_j || !totals) return fail(KMC_ERR_BAD_ARG, "null argument");
    const double *el = stats, *kh = stats + J;
    const double dJ = (double)J;
    std::vector<double> pl((size_t)J), t((size_t)J);
    int64_t n_nan = 0, kc[4] = {};
    for (int64_t j = 0; j < J; ++j) {
        pl[(size_t)j] = lppd_j[j] - el[j];
        n_nan += std::isnan(el[j]);
        if (kh[j] <= 0.5) ++kc[0];
        else if (kh[j] <= 0.7) ++kc[1];
        else if (kh[j] <= 1.0) ++kc[2];
        else if (kh[j] > 1.0) ++kc[3];
    }
    if (p_loo_j) std::copy(pl.begin(), pl.end(), p_loo_j);
    t.assign(el, el + J); totals[0] = pairwise_tree(t);
    const double centre = totals[0] / dJ;
    for (int64_t j = 0; j < J; ++j) { const double dv = el[j] - centre; t[(size_t)j] = dv * dv; }
    totals[1] = std::sqrt(dJ * pairwise_tree(t) / (double)(J - 1));
    t = pl; totals[2] = pairwise_tree(t);
    totals[3] = -2.0 * totals[0];
    t.assign(lppd_j, lppd_j + J); totals[4] = pairwise_tree(t);
    totals[5] = (double)n_nan;
    for (int k = 0; k < 4; ++k) totals[6 + k] = (double)kc[k];
    return KMC_OK;
}

// Steps 3 and 4 for one observation on the host, with the arithmetic and the summation order of the device's fit kernel
// (kmc_psis_fit.hpp).  x: the tail ascending, [nt]; s: [nt] out.  sums: sum exp(s_i), sum exp(s_i - x_(i)).
KMC_EXPORT kmc_status kmc_psis_smooth_host(int64_t nt, const double* x, double xc, double* k_hat, double* sigma, double* s, double* sums)
{
    if (nt < 0 || nt > kmc_psis::kMaxTail) return fail(KMC_ERR_BAD_ARG, "the tail must hold 0 .. 4096 draws (nt = " + std::to_string(nt) + ")");
    if (nt > 0 && (!x || !s)) return fail(KMC_ERR_BAD_ARG, "null argument");
    for (int64_t i = 0; i < nt; ++i)
        if (!(x[i] > xc) || x[i] > 0.0 || (i > 0 && x[i] < x[i - 1]))
            return fail(KMC_ERR_BAD_ARG, "the tail must be ascending, above the cut-off and <= 0 (x[" + std::to_string(i) + "] = " + std::to_string(x[i]) + ")");
    double grid[3][kmc_psis::kMaxGrid];
    kmc_psis::HostCtx ctx;
    const kmc_psis::FitScratch sc{grid[0], grid[1], grid[2]};
    const kmc_psis::FitResult r = kmc_psis::psis_fit(ctx, x, s, (int)nt, xc, sc);
    if (k_hat) *k_hat = r.k;
    if (sigma) *sigma = r.sigma;
    if (sums) { sums[0] = r.w_tail; sums[1] = r.n_tail; }
    return KMC_OK;
}
