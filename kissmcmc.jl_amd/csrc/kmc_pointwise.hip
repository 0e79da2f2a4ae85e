// kmc_pointwise.hip -- the pointwise log-likelihood of a data density over a stored chain, on the device where the chain, the data and
// the compiled term are: the per-observation statistics behind WAIC (kmc_sampler_pointwise_stats, kmc_chain_pointwise_stats), the
// matrix itself for a range of observations (kmc_sampler_pointwise_loglike, kmc_chain_pointwise_loglike), the plan (kmc_pointwise_plan)
// and the pure host stage (kmc_waic_stats); and PSIS-LOO over the same rows (kmc_sampler_psis_loo, kmc_chain_psis_loo, the read-out of its
// tails kmc_*_psis_tail, kmc_psis_plan, kmc_loo_stats, kmc_psis_smooth_host; with a relative efficiency per observation, supplied or
// computed from the chain: kmc_*_relative_eff, kmc_*_pointwise_weights, kmc_*_psis_loo_reff, kmc_*_psis_tail_reff, whose ESS stage is
// kmc_convergence.hip's on groups of 64 observations).  include/kissmcmc_hip.h has the definitions, DESIGN.md
// sections 4k and 4l the plans.  Kernels: kmc_pointwise.hpp, compiled at run time with the density's term as the module "pointwise:<ndim>";
// the folds and the PSIS fit, which do not touch the term, are compiled here.
#include <algorithm>
#include <cmath>
#include <sstream>
#include <vector>

#include "kmc_chain_view.hpp"
#include "kmc_convergence_host.hpp"
#include "kmc_pointwise.hpp"

using namespace kmc_host;
using namespace kmc_chain_view;
using namespace kmc_pw;

namespace {

constexpr int64_t kPwTargetWaves = 4096;          // of one pass: 4 per SIMD of 256 compute units
constexpr int64_t kPwMinRun = 16;                 // rows of a run at least: a run loads d_j once and writes two partials
constexpr int64_t kPwMatrixWaves = 65536;         // pw_matrix: waves along the rows at most

// the cut of n rows and J observations: from n and J alone
struct PwPlan {
    int64_t run_len = 0, nruns = 0, nwaves = 0;   // nwaves: along the rows, each over ceil(J / 64) groups of observations
    int32_t lanes = 64, slots = 1, jp_log2 = 6;   // packed (J < 64): lanes = Jp observations per run slot, slots = 64 / Jp
    bool packed = false;
};

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

struct PwKernels {
    std::shared_ptr<void> keep, keep_data, keep_weights;
    hipFunction_t pass[2][2] = {};                // [pass - 1][packed]
    hipFunction_t matrix = nullptr, weights = nullptr;
    hipFunction_t psis[3][2] = {};                // [mode][packed]
};

kmc_status compile_pointwise(kmc_user_density* ud, int64_t ndim, const std::vector<char>** out)
{
    static const RtcModule m{"data density", "kmc_pointwise.hip", {"kmc_device.hpp", "kmc_pointwise.hpp", "kmc_psis_fit.hpp"}, rtc_options()};
    return compile_keyed(ud, "pointwise:" + std::to_string(ndim), m, [&](std::string* text) {
        const std::string t = "<UserData, " + std::to_string(ndim) + ", " + std::to_string(ud->ncols);
        const std::string head = "extern \"C\" __global__ __launch_bounds__(" + std::to_string(kPwThreads) + ") void ";
        std::ostringstream src;
        src << "#include \"kmc_pointwise.hpp\"\n" << data_functor_source(ud)
            << head << "kmc_pw_pass1(const kmc_pw::PwArgs a) { kmc_pw::pw_partials" << t << ", 1, false>(a); }\n"
            << head << "kmc_pw_pass2(const kmc_pw::PwArgs a) { kmc_pw::pw_partials" << t << ", 2, false>(a); }\n"
            << head << "kmc_pw_pass1_packed(const kmc_pw::PwArgs a) { kmc_pw::pw_partials" << t << ", 1, true>(a); }\n"
            << head << "kmc_pw_pass2_packed(const kmc_pw::PwArgs a) { kmc_pw::pw_partials" << t << ", 2, true>(a); }\n"
            << head << "kmc_pw_matrix(const kmc_pw::PwArgs a) { kmc_pw::pw_matrix" << t << ">(a); }\n";
        for (int mode = 0; mode < 3; ++mode)
            for (int packed = 0; packed < 2; ++packed)
                src << head << "kmc_psis_walk" << mode << (packed ? "_packed" : "") << "(const kmc_pw::PsisArgs q) { kmc_pw::psis_walk" << t << ", " << mode << ", "
                    << (packed ? "true" : "false") << ">(q); }\n";
        *text = src.str();
        return KMC_OK;
    }, out);
}

// The weight series' kernel (pw_weights) is a module of its own, "pointwise_weights:<ndim>", compiled when a relative efficiency or the
// series is first asked for: the module above keeps the text it has for WAIC and for PSIS-LOO with one r_eff.
kmc_status compile_weights(kmc_user_density* ud, int64_t ndim, const std::vector<char>** out)
{
    static const RtcModule m{"data density", "kmc_pointwise_weights.hip", {"kmc_device.hpp", "kmc_pointwise.hpp", "kmc_psis_fit.hpp"}, rtc_options()};
    return compile_keyed(ud, "pointwise_weights:" + std::to_string(ndim), m, [&](std::string* text) {
        std::ostringstream src;
        src << "#include \"kmc_pointwise.hpp\"\n" << data_functor_source(ud) << "extern \"C\" __global__ __launch_bounds__(" << kPwThreads
            << ") void kmc_pw_weights(const kmc_pw::WeightArgs q) { kmc_pw::pw_weights<UserData, " << ndim << ", " << ud->ncols << ">(q); }\n";
        *text = src.str();
        return KMC_OK;
    }, out);
}

kmc_status load_weights(kmc_user_density* ud, int64_t ndim, PwKernels* pk)
{
    const std::vector<char>* code = nullptr;
    KMC_TRY(compile_weights(ud, ndim, &code));
    KMC_TRY(shared_module(ud, code, &pk->keep_weights));
    HIP_TRY(hipModuleGetFunction(&pk->weights, static_cast<hipModule_t>(pk->keep_weights.get()), "kmc_pw_weights"));
    return KMC_OK;
}

// compile (cached) + module on the current device + the device copy of the density's own observations
kmc_status load_pointwise(kmc_user_density* ud, int64_t ndim, bool own_data, PwKernels* pk)
{
    const std::vector<char>* code = nullptr;
    KMC_TRY(compile_pointwise(ud, ndim, &code));
    KMC_TRY(shared_module(ud, code, &pk->keep));
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (own_data) KMC_TRY(data_on_device(ud, dev, &pk->keep_data));
    hipModule_t mod = static_cast<hipModule_t>(pk->keep.get());
    HIP_TRY(hipModuleGetFunction(&pk->pass[0][0], mod, "kmc_pw_pass1"));
    HIP_TRY(hipModuleGetFunction(&pk->pass[1][0], mod, "kmc_pw_pass2"));
    HIP_TRY(hipModuleGetFunction(&pk->pass[0][1], mod, "kmc_pw_pass1_packed"));
    HIP_TRY(hipModuleGetFunction(&pk->pass[1][1], mod, "kmc_pw_pass2_packed"));
    HIP_TRY(hipModuleGetFunction(&pk->matrix, mod, "kmc_pw_matrix"));
    for (int mode = 0; mode < 3; ++mode)
        for (int packed = 0; packed < 2; ++packed)
            HIP_TRY(hipModuleGetFunction(&pk->psis[mode][packed], mod, ("kmc_psis_walk" + std::to_string(mode) + (packed ? "_packed" : "")).c_str()));
    return KMC_OK;
}

__global__ __launch_bounds__(256) void pw_fold(const PwArgs a, int pass) { pw_fold_body(a, pass); }
__global__ __launch_bounds__(256) void psis_fold(const PsisArgs q, int stage) { psis_fold_body(q, stage); }
__global__ __launch_bounds__(kmc_psis::kFitLanes) void psis_fit_kernel(const PsisArgs q, int sort_len) { psis_fit_body(q, sort_len); }

// the device copies one call owns, beyond the chain's: the list of selected walkers, held-out observations, the work space
struct PwBuffers : ChainUpload {
    int32_t *sel = nullptr, *Mj = nullptr;
    double *data = nullptr, *work = nullptr;
    void* work2 = nullptr;
    ~PwBuffers() { (void)hipFree(sel); (void)hipFree(Mj); (void)hipFree(data); (void)hipFree(work); (void)hipFree(work2); }
};

// the events around the two passes, for info: each pass is its partial kernel and its fold
struct PassEvents {
    hipEvent_t e[3] = {};
    hipError_t create()
    {
        for (auto& x : e) { const hipError_t r = hipEventCreate(&x); if (r != hipSuccess) return r; }
        return hipSuccess;
    }
    ~PassEvents() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
};

// what the two calls ask for beyond the chain
struct PwRequest {
    kmc_user_density* ud = nullptr;
    const double* params = nullptr;               // 6
    int64_t first_sample = 0, thin = 1;
    const uint8_t* walker_mask = nullptr;
    const double* data = nullptr;                 // held-out observations [ndata2][ncols2] or nullptr
    int64_t ndata2 = 0;
    int32_t ncols2 = 0;
    bool matrix = false;
    int64_t obs_first = 0, obs_count = 0;
    bool psis = false;                            // PSIS-LOO: over the observations [obs_first, obs_first + obs_count)
    double r_eff = 1.0;
    int64_t workspace = 0;                        // bytes of work space a block of observations may take; 0: kPsisWorkspace
    // the relative efficiency per observation: supplied [obs_count], or -- reff_chain -- computed from the chain (reff_stage)
    const double* r_eff_j = nullptr;
    bool reff_chain = false, split = true, weights = false;      // weights: the series itself is asked for (no PSIS, no ESS)
    int64_t max_lag = 0;
    double* weights_M = nullptr;                  // weights: M_j [obs_count] out
};

constexpr int64_t kPsisWorkspace = (int64_t)1 << 30;

// the refusals PSIS-LOO adds, from the sizes alone; M: the tail length
kmc_status psis_check(int64_t n, double r_eff, int64_t* M, bool sizes_only = false)
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

// how PSIS-LOO cuts J' observations of n rows into blocks: from n, the density's J, r_eff and the work-space budget alone
struct PsisPlan {
    int64_t M = 0, m_est = 0, block = 0, passes = 2 + kmc_psis::kSelectPasses;
    size_t per_obs = 0;                           // bytes of work space of one observation
    int sort_len = 1;
};

PsisPlan psis_plan(int64_t M, const PwPlan& pl, int64_t workspace)
{
    PsisPlan p;
    p.M = M;
    p.m_est = 30 + (int64_t)std::floor(std::sqrt((double)M));
    while (p.sort_len < M) p.sort_len <<= 1;
    p.per_obs = (size_t)M * 8 + (size_t)pl.nruns * (8 + 4 * kmc_psis::kSelectBins) + 8 * 8 + 8;
    const int64_t budget = workspace > 0 ? workspace : kPsisWorkspace;
    p.block = std::max<int64_t>(64, budget / (int64_t)p.per_obs / 64 * 64);
    return p;
}

// one call's view of the chain, its stream, kernels and arguments.  (Members die in reverse order: the stream is drained before the
// buffers go.)
struct PwSession {
    ChainView v;
    PwBuffers b;
    ScopedStream ss;
    PwKernels pk;
    PwArgs a{};
    PwPlan pl;
    int64_t n = 0, J = 0;
    kmc_conv_host::ConvShape sh;                  // reff_chain: the chains of the weight series
    int64_t max_lag = 0;
    std::vector<double> r_used;                   // a per-observation r_eff: as used (1.0 where it is not finite and > 0) ...
    std::vector<int32_t> Mj;                      // ... and the tail lengths
    int64_t n_reff_nan = 0;
};

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

// the refusals, then the chain, the stream, the module and the arguments every kernel shares
kmc_status pw_open(const ChainSource& src, const PwRequest& q, const void* result, PwSession* S)
{
    ChainView& v = S->v;
    PwBuffers& b = S->b;
    ScopedStream& ss = S->ss;
    PwKernels& pk = S->pk;
    PwArgs& a = S->a;
    if (!q.ud || !q.ud->is_data) return fail(KMC_ERR_BAD_ARG, "the pointwise log-likelihood needs a data density (kmc_data_density_create): other densities have no per-observation term");
    KMC_TRY(src.describe(&v));
    if (v.ndim > kDataMaxDim) return fail(KMC_ERR_BAD_ARG, "a data density takes at most " + std::to_string(kDataMaxDim) + " dimensions (ndim = " + std::to_string(v.ndim) + ")");
    if (q.thin < 1) return fail(KMC_ERR_BAD_ARG, "thin must be >= 1 (thin = " + std::to_string(q.thin) + ")");
    int64_t n_all = 0;
    KMC_TRY(selection_size(v, q.first_sample, q.walker_mask, &n_all));
    const int64_t kept = (v.nsamples - q.first_sample + q.thin - 1) / q.thin;
    const int64_t nsel = n_all / (v.nsamples - q.first_sample);
    const int64_t n = kept * nsel;
    if (n < 2) return fail(KMC_ERR_BAD_ARG, "the pointwise statistics need at least 2 selected rows (n = " + std::to_string(n) + ")");
    if (n >= ((int64_t)1 << 40)) return fail(KMC_ERR_UNSUPPORTED, "too many rows for one pointwise call: n = " + std::to_string(n) + ", the limit is 2^40");
    if (q.psis) KMC_TRY(psis_check(n, q.r_eff, nullptr, q.r_eff_j || q.reff_chain));
    if (q.reff_chain) {                           // the chains of the weight series: nsel of `kept` samples each
        ChainView gv;
        gv.ld = 64; gv.ndim = 1; gv.nsamples = kept; gv.nl = nsel;
        KMC_TRY(kmc_conv_host::conv_shape(gv, 0, nullptr, q.split, &S->sh));
        S->max_lag = q.max_lag;
        KMC_TRY(kmc_conv_host::resolve_max_lag(S->sh, &S->max_lag));
    }
    int64_t J = q.ud->ndata;
    if (q.data) {
        if (q.ncols2 != q.ud->ncols)
            return fail(KMC_ERR_BAD_ARG, "held-out data of " + std::to_string(q.ncols2) + " columns: the density's observations have " + std::to_string(q.ud->ncols));
        if (q.ndata2 < 1 || q.ndata2 > kDataMaxRows) return fail(KMC_ERR_BAD_ARG, "held-out data: ndata must be in 1 .. 2^30 (ndata = " + std::to_string(q.ndata2) + ")");
        J = q.ndata2;
    }
    if (q.matrix || q.psis || q.reff_chain || q.weights) {
        if (q.obs_count < 1) return fail(KMC_ERR_BAD_ARG, "the matrix needs obs_count >= 1 (obs_count = " + std::to_string(q.obs_count) + ")");
        if (q.obs_first < 0 || q.obs_first > J - q.obs_count)
            return fail(KMC_ERR_BAD_ARG, "observations [" + std::to_string(q.obs_first) + ", " + std::to_string(q.obs_first) + " + " + std::to_string(q.obs_count) +
                                             ") lie outside [0, " + std::to_string(J) + ")");
    }
    if (q.r_eff_j) {
        for (int64_t c = 0; c < q.obs_count; ++c)
            if (!(q.r_eff_j[c] > 0.0) || !std::isfinite(q.r_eff_j[c]))
                return fail(KMC_ERR_BAD_ARG, "r_eff_j must be finite and > 0 (r_eff_j[" + std::to_string(c) + "] = " + std::to_string(q.r_eff_j[c]) + ")");
        KMC_TRY(tail_lengths(n, q.obs_first, q.r_eff_j, q.obs_count, S));
    }
    if (v.is_float) return fail(KMC_ERR_UNSUPPORTED, "a chain of floats: data densities sample in double");
    if (!result || !q.params) return fail(KMC_ERR_BAD_ARG, "null argument");
    S->n = n; S->J = J;
    S->pl = pw_plan(n, J);
    const PwPlan& pl = S->pl;

    KMC_TRY(src.open(b, &v));
    // Never the legacy stream (kmc_host.hpp: copy_sync).  A sampler's own stream, which describe() has drained, serves: creating and
    // destroying a stream for the call costs 3.4 to 4.4 ms, several times the two passes at the README's small shape.
    if (src.host || !src.s->stream) HIP_TRY(ss.create());
    else ss.borrowed = src.s->stream;
    KMC_TRY(load_pointwise(q.ud, v.ndim, !q.data, &pk));

    a.chain = static_cast<const double*>(v.chain);
    a.n = n; a.J = J; a.nl = v.nl; a.ld = v.ld; a.nsel = nsel; a.first = q.first_sample; a.thin = q.thin;
    a.nd = (double)n; a.jp_log2 = pl.jp_log2;
    for (int i = 0; i < 6; ++i) a.p[i] = q.params[i];
    if (q.walker_mask) {
        std::vector<int32_t> sel;
        for (int64_t w = 0; w < v.nl; ++w) if (q.walker_mask[w]) sel.push_back((int32_t)w);
        HIP_TRY(hipMalloc((void**)&b.sel, sel.size() * sizeof(int32_t)));
        HIP_TRY(copy_sync(b.sel, sel.data(), sel.size() * sizeof(int32_t), hipMemcpyHostToDevice, ss.get()));
        a.sel = b.sel;
    }
    if (q.data) {
        const size_t bytes = (size_t)J * (size_t)q.ncols2 * sizeof(double);
        KMC_TRY(check_device_room(bytes, "the held-out observations"));
        HIP_TRY(hipMalloc((void**)&b.data, bytes));
        HIP_TRY(copy_sync(b.data, q.data, bytes, hipMemcpyHostToDevice, ss.get()));
        a.data = b.data;
    } else {
        a.data = static_cast<const double*>(pk.keep_data.get());
    }
    a.run_len = pl.run_len; a.nruns = pl.nruns;
    return KMC_OK;
}

// the two passes of the statistics, left on the device: work gets the work space, a.stats [4][J]
kmc_status pw_stats(PwSession& S, double** work, int64_t* info, int npass = 2)
{
    PwArgs& a = S.a;
    const PwPlan& pl = S.pl;
    const int64_t n = S.n, J = S.J;
    const size_t part = 2 * (size_t)pl.nruns * (size_t)J, doubles = part + 5 * (size_t)J;
    KMC_TRY(check_device_room(doubles * sizeof(double), "the pointwise work space"));
    HIP_TRY(hipMalloc((void**)work, doubles * sizeof(double)));
    a.part = *work; a.stats = *work + part; a.centre = a.stats + 4 * (size_t)J;
    a.run_len = pl.run_len; a.nruns = pl.nruns;
    const unsigned gx = (unsigned)((J + 63) / 64), gy = (unsigned)((pl.nwaves + kPwWaves - 1) / kPwWaves), gf = (unsigned)((J + 255) / 256);
    PassEvents ev;
    if (info) HIP_TRY(ev.create());
    for (int pass = 1; pass <= npass; ++pass) {                                        // (npass = 1: M and S1 alone; info needs both)
        if (info) HIP_TRY(hipEventRecord(ev.e[pass - 1], S.ss.get()));
        HIP_TRY(launch_module_y(S.pk.pass[pass - 1][pl.packed ? 1 : 0], gx, gy, kPwThreads, S.ss.get(), a));
        hipLaunchKernelGGL(pw_fold, dim3(gf), dim3(256), 0, S.ss.get(), a, pass);
        HIP_TRY(hipGetLastError());
    }
    if (info) {
        HIP_TRY(hipEventRecord(ev.e[2], S.ss.get()));
        HIP_TRY(hipStreamSynchronize(S.ss.get()));
        float ms1 = 0.f, ms2 = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms1, ev.e[0], ev.e[1]));
        HIP_TRY(hipEventElapsedTime(&ms2, ev.e[1], ev.e[2]));
        info[0] = n; info[1] = pl.nruns; info[2] = 2 * n * J; info[3] = pl.run_len;
        info[4] = (int64_t)((double)ms1 * 1e6); info[5] = (int64_t)((double)ms2 * 1e6);
    }
    return KMC_OK;
}

// what the relative-efficiency stage hands back, each [obs_count] or nullptr
struct ReffOut {
    double *r_eff = nullptr, *ess = nullptr;
    int64_t* T = nullptr;
    int32_t* flags = nullptr;
    double* v = nullptr;                          // the series itself, dense [n][obs_count]; with it the ESS is not taken
};

// The weight series v = exp(l - M_j) of the observations [obs_first, obs_first + obs_count), in groups of 64 observations aligned to
// the absolute index, and the effective sample size of every column by the convergence diagnostics' own stages (kmc_convergence.hip)
// on each group as a chain [kept][nsel][64].  ld = 64 whatever the group holds: lags_device then has period = 1 and a lane owns one
// column, so the grid and the order of a column's additions follow from the selection's shape alone -- not from the group, the other
// columns, the range or the work space.  Needs a.stats of pass 1.  info3: nanoseconds of the weight passes, of the ESS stage, groups.
kmc_status reff_stage(PwSession& S, const PwRequest& q, const ReffOut& o, int64_t* info3)
{
    const int64_t n = S.n, count = q.obs_count;
    hipStream_t st = S.ss.get();
    KMC_TRY(load_weights(q.ud, S.v.ndim, &S.pk));
    const int64_t g_first = q.obs_first / 64, g_last = (q.obs_first + count - 1) / 64, ngroups = g_last - g_first + 1;
    const double group_bytes = (double)n * 64.0 * 8.0;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (group_bytes > (double)free_b)
        return fail(KMC_ERR_UNSUPPORTED, "the weight series of one group of 64 observations (" + std::to_string((int64_t)group_bytes) + " bytes, n = " +
                                             std::to_string(n) + ") does not fit the device (" + std::to_string(free_b) + " bytes free): thin the chain");
    const int64_t budget = std::min<int64_t>(q.workspace > 0 ? q.workspace : kPsisWorkspace, (int64_t)(free_b / 2));
    const int64_t per_batch = std::max<int64_t>(1, std::min<int64_t>(ngroups, budget / (int64_t)group_bytes));
    double* buf = nullptr;
    HIP_TRY(hipMalloc((void**)&buf, (size_t)per_batch * (size_t)n * 64 * sizeof(double)));
    std::shared_ptr<void> keep(buf, [](void* p) { (void)hipFree(p); });

    WeightArgs wa{};
    wa.a = S.a;
    wa.a.out = buf; wa.a.obs_first = q.obs_first; wa.a.obs_count = count;
    wa.a.run_len = std::max(kPwMinRun, (n + kPwMatrixWaves - 1) / kPwMatrixWaves);
    const int64_t waves = (n + wa.a.run_len - 1) / wa.a.run_len;

    kmc_conv_host::ConvBuffers cb;
    if (!o.v) KMC_TRY(kmc_conv_host::upload_rank(cb, nullptr, S.a.nsel, st));
    ChainView gv;
    gv.ld = 64; gv.nsamples = n / S.a.nsel; gv.nl = S.a.nsel;
    double mean[64], W[64], B[64], vp[64], rhat[64], ess[64], mcse[64];
    int64_t T[64];
    int32_t flags[64];
    const kmc_conv_host::StatsOut so{mean, W, B, vp, rhat, ess, mcse, T, flags};
    const double mh = (double)S.sh.m * (double)S.sh.h;
    std::vector<double> host_group;
    if (o.v) host_group.resize((size_t)n * 64);

    PassEvents ev;
    if (info3) HIP_TRY(ev.create());
    double ms_w = 0.0, ms_e = 0.0;
    for (int64_t g0 = g_first; g0 <= g_last; g0 += per_batch) {
        const int64_t ng = std::min(per_batch, g_last - g0 + 1);
        wa.group0 = g0;
        if (info3) HIP_TRY(hipEventRecord(ev.e[0], st));
        HIP_TRY(launch_module_y(S.pk.weights, (unsigned)ng, (unsigned)((waves + kPwWaves - 1) / kPwWaves), kPwThreads, st, wa));
        if (info3) HIP_TRY(hipEventRecord(ev.e[1], st));
        for (int64_t i = 0; i < ng; ++i) {
            const int64_t j0 = (g0 + i) * 64;
            const int64_t lo = std::max<int64_t>(0, q.obs_first - j0), hi = std::min<int64_t>(63, q.obs_first + count - 1 - j0);    // the live lanes
            const double* group = buf + (size_t)i * (size_t)n * 64;
            if (o.v) {
                HIP_TRY(copy_sync(host_group.data(), group, host_group.size() * sizeof(double), hipMemcpyDeviceToHost, st));
                for (int64_t k = 0; k < n; ++k)
                    for (int64_t l = lo; l <= hi; ++l) o.v[k * count + (j0 + l - q.obs_first)] = host_group[(size_t)(k * 64 + l)];
                continue;
            }
            gv.chain = group;
            gv.ndim = hi + 1;                                                          // (the lanes below lo are constant 0.0: no ESS, no lags)
            KMC_TRY(kmc_conv_host::convergence_on_stream(cb, gv, S.sh, false, S.max_lag, so, nullptr, st));
            for (int64_t l = lo; l <= hi; ++l) {
                const int64_t c = j0 + l - q.obs_first;
                if (o.r_eff) o.r_eff[c] = ess[l] / mh;
                if (o.ess) o.ess[c] = ess[l];
                if (o.T) o.T[c] = T[l];
                if (o.flags) o.flags[c] = flags[l];
            }
        }
        if (info3) {
            HIP_TRY(hipEventRecord(ev.e[2], st));
            HIP_TRY(hipStreamSynchronize(st));
            float t0 = 0.f, t1 = 0.f;
            HIP_TRY(hipEventElapsedTime(&t0, ev.e[0], ev.e[1]));
            HIP_TRY(hipEventElapsedTime(&t1, ev.e[1], ev.e[2]));
            ms_w += (double)t0; ms_e += (double)t1;
        }
    }
    HIP_TRY(hipStreamSynchronize(st));                                                 // (buf goes with this scope)
    if (info3) { info3[0] = (int64_t)(ms_w * 1e6); info3[1] = (int64_t)(ms_e * 1e6); info3[2] = ngroups; }
    return KMC_OK;
}

// stats [4][J] (statistics), or out [n][obs_count] (matrix)
kmc_status pointwise(const ChainSource& src, const PwRequest& q, double* result, int64_t* n_out, int64_t* info)
{
    PwSession S;
    KMC_TRY(pw_open(src, q, result, &S));
    PwBuffers& b = S.b;
    ScopedStream& ss = S.ss;
    PwKernels& pk = S.pk;
    PwArgs& a = S.a;
    const int64_t n = S.n, J = S.J;
    if (n_out) *n_out = n;

    if (q.matrix) {
        const double need = (double)n * (double)q.obs_count * 8.0;
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        if (need > (double)free_b)
            return fail(KMC_ERR_UNSUPPORTED, "a matrix of " + std::to_string(n) + " x " + std::to_string(q.obs_count) + " log-likelihoods (" +
                                                 std::to_string((int64_t)(need / 1048576.0)) + " MiB) does not fit the device (" + std::to_string(free_b >> 20) +
                                                 " MiB free): ask for fewer observations at a time, or thin");
        const size_t bytes = (size_t)n * (size_t)q.obs_count * sizeof(double);
        HIP_TRY(hipMalloc((void**)&b.work, bytes));
        a.out = b.work; a.obs_first = q.obs_first; a.obs_count = q.obs_count;
        a.run_len = std::max(kPwMinRun, (n + kPwMatrixWaves - 1) / kPwMatrixWaves);
        const int64_t waves = (n + a.run_len - 1) / a.run_len;
        HIP_TRY(launch_module_y(pk.matrix, (unsigned)((q.obs_count + 63) / 64), (unsigned)((waves + kPwWaves - 1) / kPwWaves), kPwThreads, ss.get(), a));
        HIP_TRY(copy_sync(result, b.work, bytes, hipMemcpyDeviceToHost, ss.get()));
        if (info) { info[0] = n; info[1] = waves; info[2] = n * q.obs_count; info[3] = a.run_len; }
        return KMC_OK;
    }

    if (q.weights) {
        KMC_TRY(pw_stats(S, &b.work, nullptr, 1));
        ReffOut o;
        o.v = result;
        KMC_TRY(reff_stage(S, q, o, nullptr));
        if (q.weights_M) HIP_TRY(copy_sync(q.weights_M, a.stats + q.obs_first, (size_t)q.obs_count * sizeof(double), hipMemcpyDeviceToHost, ss.get()));
        return KMC_OK;
    }

    KMC_TRY(pw_stats(S, &b.work, info));
    HIP_TRY(copy_sync(result, a.stats, 4 * (size_t)J * sizeof(double), hipMemcpyDeviceToHost, ss.get()));
    return KMC_OK;
}

// r_eff_j = ess_j / (m h) of the weight series, alone.  info [6]: n, groups, nanoseconds of pass 1, of the weight passes, of the ESS
// stage (moments, lags and their copies per group), h.
kmc_status relative_eff(const ChainSource& src, const PwRequest& q, const ReffOut& o, int64_t* m_out, int64_t* h_out, int64_t* n_out, int64_t* info)
{
    PwSession S;
    KMC_TRY(pw_open(src, q, o.r_eff, &S));
    if (m_out) *m_out = S.sh.m;
    if (h_out) *h_out = S.sh.h;
    if (n_out) *n_out = S.n;
    PassEvents ev;
    if (info) { HIP_TRY(ev.create()); HIP_TRY(hipEventRecord(ev.e[0], S.ss.get())); }
    KMC_TRY(pw_stats(S, &S.b.work, nullptr, 1));
    if (info) HIP_TRY(hipEventRecord(ev.e[1], S.ss.get()));
    int64_t i3[3] = {};
    KMC_TRY(reff_stage(S, q, o, info ? i3 : nullptr));
    if (info) {
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, ev.e[0], ev.e[1]));
        info[0] = S.n; info[1] = i3[2]; info[2] = (int64_t)((double)t * 1e6); info[3] = i3[0]; info[4] = i3[1]; info[5] = S.sh.h;
    }
    return KMC_OK;
}

kmc_status sampler_density(kmc_sampler* s, PwRequest* q)
{
    if (!s) return fail(KMC_ERR_BAD_ARG, "null sampler");
    q->ud = s->data_ud;
    q->params = s->dp.p;
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

}  // namespace

KMC_EXPORT kmc_status kmc_sampler_pointwise_stats(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int64_t thin, const double* data,
                                                  int64_t ndata2, int32_t ncols2, double* stats, int64_t* n_out, int64_t* info)
{
    PwRequest q;
    KMC_TRY(sampler_density(s, &q));
    q.first_sample = first_sample; q.thin = thin; q.walker_mask = walker_mask; q.data = data; q.ndata2 = ndata2; q.ncols2 = ncols2;
    return pointwise(ChainSource(s, false, "kmc_chain_pointwise_stats"), q, stats, n_out, info);
}

KMC_EXPORT kmc_status kmc_chain_pointwise_stats(kmc_user_density* density, const double* params, const double* chain_host, int64_t nsamples,
                                                int64_t nwalkers, int64_t ndim, int64_t first_sample, const uint8_t* walker_mask, int64_t thin,
                                                const double* data, int64_t ndata2, int32_t ncols2, int device, double* stats, int64_t* n_out,
                                                int64_t* info)
{
    PwRequest q;
    q.ud = density; q.params = params;
    q.first_sample = first_sample; q.thin = thin; q.walker_mask = walker_mask; q.data = data; q.ndata2 = ndata2; q.ncols2 = ncols2;
    return pointwise(ChainSource(chain_host, nullptr, nsamples, nwalkers, ndim, device), q, stats, n_out, info);
}

KMC_EXPORT kmc_status kmc_sampler_pointwise_loglike(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int64_t thin, const double* data,
                                                    int64_t ndata2, int32_t ncols2, int64_t obs_first, int64_t obs_count, double* out, int64_t* n_out)
{
    PwRequest q;
    KMC_TRY(sampler_density(s, &q));
    q.first_sample = first_sample; q.thin = thin; q.walker_mask = walker_mask; q.data = data; q.ndata2 = ndata2; q.ncols2 = ncols2;
    q.matrix = true; q.obs_first = obs_first; q.obs_count = obs_count;
    return pointwise(ChainSource(s, false, "kmc_chain_pointwise_loglike"), q, out, n_out, nullptr);
}

KMC_EXPORT kmc_status kmc_chain_pointwise_loglike(kmc_user_density* density, const double* params, const double* chain_host, int64_t nsamples,
                                                  int64_t nwalkers, int64_t ndim, int64_t first_sample, const uint8_t* walker_mask, int64_t thin,
                                                  const double* data, int64_t ndata2, int32_t ncols2, int64_t obs_first, int64_t obs_count,
                                                  int device, double* out, int64_t* n_out)
{
    PwRequest q;
    q.ud = density; q.params = params;
    q.first_sample = first_sample; q.thin = thin; q.walker_mask = walker_mask; q.data = data; q.ndata2 = ndata2; q.ncols2 = ncols2;
    q.matrix = true; q.obs_first = obs_first; q.obs_count = obs_count;
    return pointwise(ChainSource(chain_host, nullptr, nsamples, nwalkers, ndim, device), q, out, n_out, nullptr);
}

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

// ---------------------------------------------------------------------------------------------------------------------------------
// PSIS-LOO (include/kissmcmc_hip.h)
// ---------------------------------------------------------------------------------------------------------------------------------
namespace {

struct PsisEvents {
    hipEvent_t e[5] = {};
    hipError_t create()
    {
        for (auto& x : e) { const hipError_t r = hipEventCreate(&x); if (r != hipSuccess) return r; }
        return hipSuccess;
    }
    ~PsisEvents() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
};

// what one call hands back, each [obs_count] or nullptr
struct PsisOut {
    double* res = nullptr;        // [4][obs_count]: elpd_loo_j, pareto_k, n_tail_j, sigma_j
    double* lppd_j = nullptr;     // the statistics' passes run only when this is asked for
    double* tail = nullptr;       // [obs_count][M]
    double *m = nullptr, *xc = nullptr;
    int32_t* n_tail = nullptr;
    int64_t* tail_len = nullptr;
    double* r_eff = nullptr;      // a per-observation r_eff: as computed (NaN where it has none) or as supplied
    int64_t *tail_len_j = nullptr, *n_reff_nan = nullptr;
};

kmc_status psis(const ChainSource& src, const PwRequest& q, const PsisOut& out, int64_t* n_out, int64_t* info)
{
    PwSession S;
    KMC_TRY(pw_open(src, q, out.res ? (const void*)out.res : (const void*)out.tail, &S));
    const int64_t n = S.n, J = S.J, count = q.obs_count;
    if (n_out) *n_out = n;
    hipStream_t st = S.ss.get();
    int64_t ns_stats = 0, reff_info[3] = {};
    if (out.lppd_j || q.reff_chain) {
        int64_t sinfo[6] = {};
        KMC_TRY(pw_stats(S, &S.b.work, info && out.lppd_j ? sinfo : nullptr, out.lppd_j ? 2 : 1));
        ns_stats = sinfo[4] + sinfo[5];
    }
    if (q.reff_chain) {
        std::vector<double> r((size_t)count);
        ReffOut ro;
        ro.r_eff = r.data();
        KMC_TRY(reff_stage(S, q, ro, info ? reff_info : nullptr));
        if (out.r_eff) std::copy(r.begin(), r.end(), out.r_eff);
        KMC_TRY(tail_lengths(n, q.obs_first, r.data(), count, &S));
    } else if (q.r_eff_j && out.r_eff) {
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
    const PwPlan& pl = S.pl;
    const PsisPlan pp = psis_plan(M, pl, q.workspace);
    const int64_t block = std::min(pp.block, pl.packed ? (int64_t)64 : count);

    if (out.lppd_j) {
        std::vector<double> stats(4 * (size_t)J), lp((size_t)J), totals(7);
        HIP_TRY(copy_sync(stats.data(), S.a.stats, stats.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        KMC_TRY(kmc_waic_stats(J, n, stats.data(), lp.data(), nullptr, nullptr, totals.data()));
        std::copy(lp.begin() + q.obs_first, lp.begin() + q.obs_first + count, out.lppd_j);
    }

    // the work space of one block, carved in order of alignment
    const size_t B = (size_t)block, R = (size_t)pl.nruns;
    const size_t bytes = B * (size_t)M * 8 + R * B * 8 + B * 8 * 4 + B * 32 + R * B * kmc_psis::kSelectBins * 4 + B * 4;
    KMC_TRY(check_device_room(bytes, "the PSIS-LOO work space"));
    HIP_TRY(hipMalloc(&S.b.work2, bytes));
    if (!S.Mj.empty()) {
        HIP_TRY(hipMalloc((void**)&S.b.Mj, (size_t)count * sizeof(int32_t)));
        HIP_TRY(copy_sync(S.b.Mj, S.Mj.data(), (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    PsisArgs qa{};
    qa.a = S.a;
    qa.M = (int32_t)M;
    {
        char* p = static_cast<char*>(S.b.work2);
        qa.tail = reinterpret_cast<double*>(p); p += B * (size_t)M * 8;
        qa.runval = reinterpret_cast<double*>(p); p += R * B * 8;
        qa.m = reinterpret_cast<double*>(p); p += B * 8;
        qa.xc = reinterpret_cast<double*>(p); p += B * 8;
        qa.prefix = reinterpret_cast<uint64_t*>(p); p += B * 8;
        qa.rank = reinterpret_cast<int64_t*>(p); p += B * 8;
        qa.res = reinterpret_cast<double*>(p); p += B * 32;
        qa.counts = reinterpret_cast<uint32_t*>(p); p += R * B * kmc_psis::kSelectBins * 4;
        qa.cursor = reinterpret_cast<int32_t*>(p);
    }
    PsisEvents ev;
    if (info) HIP_TRY(ev.create());
    double ms[4] = {};
    std::vector<double> res_host(4 * B);
    const unsigned gy = (unsigned)((pl.nwaves + kPwWaves - 1) / kPwWaves);
    const int pk = pl.packed ? 1 : 0;
    int64_t nblocks = 0, log1ps = 0;
    for (int64_t b0 = 0; b0 < count; b0 += block, ++nblocks) {
        const int64_t bc = std::min(block, count - b0);
        qa.a.obs_first = q.obs_first + b0;
        qa.a.obs_count = bc;
        qa.Mj = S.b.Mj ? S.b.Mj + b0 : nullptr;
        const unsigned gx = pl.packed ? 1u : (unsigned)((bc + 63) / 64), gf = (unsigned)((bc + 255) / 256);
        if (info) HIP_TRY(hipEventRecord(ev.e[0], st));
        HIP_TRY(launch_module_y(S.pk.psis[0][pk], gx, gy, kPwThreads, st, qa));
        hipLaunchKernelGGL(psis_fold, dim3(gf), dim3(256), 0, st, qa, 0);
        HIP_TRY(hipGetLastError());
        if (info) HIP_TRY(hipEventRecord(ev.e[1], st));
        for (int pass = 0; pass < kmc_psis::kSelectPasses; ++pass) {
            qa.shift = 64 - kmc_psis::kSelectBits * (pass + 1);
            HIP_TRY(launch_module_y(S.pk.psis[1][pk], gx, gy, kPwThreads, st, qa));
            hipLaunchKernelGGL(psis_fold, dim3(gf), dim3(256), 0, st, qa, 1);
            HIP_TRY(hipGetLastError());
        }
        if (info) HIP_TRY(hipEventRecord(ev.e[2], st));
        HIP_TRY(launch_module_y(S.pk.psis[2][pk], gx, gy, kPwThreads, st, qa));
        if (info) HIP_TRY(hipEventRecord(ev.e[3], st));
        hipLaunchKernelGGL(psis_fit_kernel, dim3((unsigned)bc), dim3(kmc_psis::kFitLanes), 0, st, qa, pp.sort_len);
        HIP_TRY(hipGetLastError());
        if (info) HIP_TRY(hipEventRecord(ev.e[4], st));
        HIP_TRY(copy_sync(res_host.data(), qa.res, 4 * (size_t)bc * sizeof(double), hipMemcpyDeviceToHost, st));
        for (int64_t c = 0; c < bc; ++c) {
            const double nt = res_host[2 * (size_t)bc + (size_t)c];
            if (out.res) for (int k = 0; k < 4; ++k) out.res[k * count + b0 + c] = res_host[(size_t)k * (size_t)bc + (size_t)c];
            if (out.n_tail) out.n_tail[b0 + c] = nt == nt ? (int32_t)nt : -1;
            if (nt >= kmc_psis::kMinFit) log1ps += (int64_t)nt * (31 + (int64_t)std::floor(std::sqrt(nt)));
        }
        if (out.tail) HIP_TRY(copy_sync(out.tail + b0 * M, qa.tail, (size_t)bc * (size_t)M * sizeof(double), hipMemcpyDeviceToHost, st));
        if (out.m) HIP_TRY(copy_sync(out.m + b0, qa.m, (size_t)bc * sizeof(double), hipMemcpyDeviceToHost, st));
        if (out.xc) HIP_TRY(copy_sync(out.xc + b0, qa.xc, (size_t)bc * sizeof(double), hipMemcpyDeviceToHost, st));
        if (info)
            for (int k = 0; k < 4; ++k) {
                float t = 0.f;
                HIP_TRY(hipEventElapsedTime(&t, ev.e[k], ev.e[k + 1]));
                ms[k] += (double)t;
            }
    }
    if (info) {
        info[0] = n; info[1] = M; info[2] = nblocks; info[3] = block;
        for (int k = 0; k < 4; ++k) info[4 + k] = (int64_t)(ms[k] * 1e6);
        info[8] = n * count; info[9] = log1ps; info[10] = ns_stats; info[11] = pl.nruns;
        if (q.reff_chain || q.r_eff_j) { info[12] = reff_info[0]; info[13] = reff_info[1]; info[14] = reff_info[2]; info[15] = S.n_reff_nan; }
    }
    return KMC_OK;
}

PwRequest psis_request(int64_t first_sample, const uint8_t* walker_mask, int64_t thin, double r_eff, int64_t obs_first, int64_t obs_count, int64_t workspace)
{
    PwRequest q;
    q.first_sample = first_sample; q.thin = thin; q.walker_mask = walker_mask;
    q.psis = true; q.r_eff = r_eff; q.obs_first = obs_first; q.obs_count = obs_count; q.workspace = workspace;
    return q;
}

}  // namespace

KMC_EXPORT kmc_status kmc_sampler_psis_loo(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int64_t thin, double r_eff, int64_t obs_first,
                                           int64_t obs_count, int64_t workspace_bytes, double* stats, double* lppd_j, int64_t* n_out, int64_t* info)
{
    PwRequest q = psis_request(first_sample, walker_mask, thin, r_eff, obs_first, obs_count, workspace_bytes);
    KMC_TRY(sampler_density(s, &q));
    if (!lppd_j) return fail(KMC_ERR_BAD_ARG, "null argument");
    PsisOut out;
    out.res = stats; out.lppd_j = lppd_j;
    return psis(ChainSource(s, false, "kmc_chain_psis_loo"), q, out, n_out, info);
}

KMC_EXPORT kmc_status kmc_chain_psis_loo(kmc_user_density* density, const double* params, const double* chain_host, int64_t nsamples, int64_t nwalkers,
                                         int64_t ndim, int64_t first_sample, const uint8_t* walker_mask, int64_t thin, double r_eff, int64_t obs_first,
                                         int64_t obs_count, int64_t workspace_bytes, int device, double* stats, double* lppd_j, int64_t* n_out, int64_t* info)
{
    PwRequest q = psis_request(first_sample, walker_mask, thin, r_eff, obs_first, obs_count, workspace_bytes);
    q.ud = density; q.params = params;
    if (!lppd_j) return fail(KMC_ERR_BAD_ARG, "null argument");
    PsisOut out;
    out.res = stats; out.lppd_j = lppd_j;
    return psis(ChainSource(chain_host, nullptr, nsamples, nwalkers, ndim, device), q, out, n_out, info);
}

KMC_EXPORT kmc_status kmc_sampler_psis_tail(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int64_t thin, double r_eff, int64_t obs_first,
                                            int64_t obs_count, int64_t workspace_bytes, double* tail, double* m_j, double* xc_j, int32_t* n_tail_j,
                                            int64_t* tail_len, int64_t* n_out)
{
    PwRequest q = psis_request(first_sample, walker_mask, thin, r_eff, obs_first, obs_count, workspace_bytes);
    KMC_TRY(sampler_density(s, &q));
    PsisOut out;
    out.tail = tail; out.m = m_j; out.xc = xc_j; out.n_tail = n_tail_j; out.tail_len = tail_len;
    return psis(ChainSource(s, false, "kmc_chain_psis_tail"), q, out, n_out, nullptr);
}

KMC_EXPORT kmc_status kmc_chain_psis_tail(kmc_user_density* density, const double* params, const double* chain_host, int64_t nsamples, int64_t nwalkers,
                                          int64_t ndim, int64_t first_sample, const uint8_t* walker_mask, int64_t thin, double r_eff, int64_t obs_first,
                                          int64_t obs_count, int64_t workspace_bytes, int device, double* tail, double* m_j, double* xc_j,
                                          int32_t* n_tail_j, int64_t* tail_len, int64_t* n_out)
{
    PwRequest q = psis_request(first_sample, walker_mask, thin, r_eff, obs_first, obs_count, workspace_bytes);
    q.ud = density; q.params = params;
    PsisOut out;
    out.tail = tail; out.m = m_j; out.xc = xc_j; out.n_tail = n_tail_j; out.tail_len = tail_len;
    return psis(ChainSource(chain_host, nullptr, nsamples, nwalkers, ndim, device), q, out, n_out, nullptr);
}

// ---- a per-observation relative efficiency (include/kissmcmc_hip.h) ----
namespace {

PwRequest reff_request(int64_t first_sample, const uint8_t* walker_mask, int64_t thin, int64_t obs_first, int64_t obs_count, int32_t split, int64_t max_lag,
                       int64_t workspace)
{
    PwRequest q;
    q.first_sample = first_sample; q.thin = thin; q.walker_mask = walker_mask;
    q.obs_first = obs_first; q.obs_count = obs_count; q.workspace = workspace;
    q.reff_chain = true; q.split = split != 0; q.max_lag = max_lag;
    return q;
}

// the request of the *_reff forms of PSIS-LOO: r_eff_j supplied, or computed from the chain
PwRequest psis_reff_request(int64_t first_sample, const uint8_t* walker_mask, int64_t thin, const double* r_eff_j, int32_t split, int64_t max_lag,
                            int64_t obs_first, int64_t obs_count, int64_t workspace)
{
    PwRequest q = psis_request(first_sample, walker_mask, thin, 1.0, obs_first, obs_count, workspace);
    q.r_eff_j = r_eff_j;
    q.reff_chain = r_eff_j == nullptr; q.split = split != 0; q.max_lag = max_lag;
    return q;
}

}  // namespace

KMC_EXPORT kmc_status kmc_sampler_relative_eff(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int64_t thin, int64_t obs_first,
                                               int64_t obs_count, int32_t split, int64_t max_lag, int64_t workspace_bytes, double* r_eff_j, double* ess_j,
                                               int64_t* T_j, int32_t* flags_j, int64_t* m_out, int64_t* h_out, int64_t* n_out, int64_t* info)
{
    PwRequest q = reff_request(first_sample, walker_mask, thin, obs_first, obs_count, split, max_lag, workspace_bytes);
    KMC_TRY(sampler_density(s, &q));
    ReffOut o;
    o.r_eff = r_eff_j; o.ess = ess_j; o.T = T_j; o.flags = flags_j;
    return relative_eff(ChainSource(s, false, "kmc_chain_relative_eff"), q, o, m_out, h_out, n_out, info);
}

KMC_EXPORT kmc_status kmc_chain_relative_eff(kmc_user_density* density, const double* params, const double* chain_host, int64_t nsamples, int64_t nwalkers,
                                             int64_t ndim, int64_t first_sample, const uint8_t* walker_mask, int64_t thin, int64_t obs_first,
                                             int64_t obs_count, int32_t split, int64_t max_lag, int64_t workspace_bytes, int device, double* r_eff_j,
                                             double* ess_j, int64_t* T_j, int32_t* flags_j, int64_t* m_out, int64_t* h_out, int64_t* n_out, int64_t* info)
{
    PwRequest q = reff_request(first_sample, walker_mask, thin, obs_first, obs_count, split, max_lag, workspace_bytes);
    q.ud = density; q.params = params;
    ReffOut o;
    o.r_eff = r_eff_j; o.ess = ess_j; o.T = T_j; o.flags = flags_j;
    return relative_eff(ChainSource(chain_host, nullptr, nsamples, nwalkers, ndim, device), q, o, m_out, h_out, n_out, info);
}

KMC_EXPORT kmc_status kmc_sampler_pointwise_weights(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int64_t thin, const double* data,
                                                    int64_t ndata2, int32_t ncols2, int64_t obs_first, int64_t obs_count, double* v, double* M_j,
                                                    int64_t* n_out)
{
    PwRequest q;
    KMC_TRY(sampler_density(s, &q));
    q.first_sample = first_sample; q.thin = thin; q.walker_mask = walker_mask; q.data = data; q.ndata2 = ndata2; q.ncols2 = ncols2;
    q.weights = true; q.obs_first = obs_first; q.obs_count = obs_count; q.weights_M = M_j;
    return pointwise(ChainSource(s, false, "kmc_chain_pointwise_weights"), q, v, n_out, nullptr);
}

KMC_EXPORT kmc_status kmc_chain_pointwise_weights(kmc_user_density* density, const double* params, const double* chain_host, int64_t nsamples,
                                                  int64_t nwalkers, int64_t ndim, int64_t first_sample, const uint8_t* walker_mask, int64_t thin,
                                                  const double* data, int64_t ndata2, int32_t ncols2, int64_t obs_first, int64_t obs_count, int device,
                                                  double* v, double* M_j, int64_t* n_out)
{
    PwRequest q;
    q.ud = density; q.params = params;
    q.first_sample = first_sample; q.thin = thin; q.walker_mask = walker_mask; q.data = data; q.ndata2 = ndata2; q.ncols2 = ncols2;
    q.weights = true; q.obs_first = obs_first; q.obs_count = obs_count; q.weights_M = M_j;
    return pointwise(ChainSource(chain_host, nullptr, nsamples, nwalkers, ndim, device), q, v, n_out, nullptr);
}

KMC_EXPORT kmc_status kmc_sampler_psis_loo_reff(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int64_t thin, const double* r_eff_j,
                                                int32_t split, int64_t max_lag, int64_t obs_first, int64_t obs_count, int64_t workspace_bytes,
                                                double* stats, double* lppd_j, double* r_eff_used, int64_t* tail_len_j, int64_t* n_reff_nan,
                                                int64_t* n_out, int64_t* info)
{
    PwRequest q = psis_reff_request(first_sample, walker_mask, thin, r_eff_j, split, max_lag, obs_first, obs_count, workspace_bytes);
    KMC_TRY(sampler_density(s, &q));
    if (!lppd_j) return fail(KMC_ERR_BAD_ARG, "null argument");
    PsisOut out;
    out.res = stats; out.lppd_j = lppd_j; out.r_eff = r_eff_used; out.tail_len_j = tail_len_j; out.n_reff_nan = n_reff_nan;
    return psis(ChainSource(s, false, "kmc_chain_psis_loo_reff"), q, out, n_out, info);
}

KMC_EXPORT kmc_status kmc_chain_psis_loo_reff(kmc_user_density* density, const double* params, const double* chain_host, int64_t nsamples,
                                              int64_t nwalkers, int64_t ndim, int64_t first_sample, const uint8_t* walker_mask, int64_t thin,
                                              const double* r_eff_j, int32_t split, int64_t max_lag, int64_t obs_first, int64_t obs_count,
                                              int64_t workspace_bytes, int device, double* stats, double* lppd_j, double* r_eff_used,
                                              int64_t* tail_len_j, int64_t* n_reff_nan, int64_t* n_out, int64_t* info)
{
    PwRequest q = psis_reff_request(first_sample, walker_mask, thin, r_eff_j, split, max_lag, obs_first, obs_count, workspace_bytes);
    q.ud = density; q.params = params;
    if (!lppd_j) return fail(KMC_ERR_BAD_ARG, "null argument");
    PsisOut out;
    out.res = stats; out.lppd_j = lppd_j; out.r_eff = r_eff_used; out.tail_len_j = tail_len_j; out.n_reff_nan = n_reff_nan;
    return psis(ChainSource(chain_host, nullptr, nsamples, nwalkers, ndim, device), q, out, n_out, info);
}

KMC_EXPORT kmc_status kmc_sampler_psis_tail_reff(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int64_t thin, const double* r_eff_j,
                                                 int32_t split, int64_t max_lag, int64_t obs_first, int64_t obs_count, int64_t workspace_bytes,
                                                 double* tail, double* m_j, double* xc_j, int32_t* n_tail_j, int64_t* tail_len, double* r_eff_used,
                                                 int64_t* tail_len_j, int64_t* n_reff_nan, int64_t* n_out)
{
    PwRequest q = psis_reff_request(first_sample, walker_mask, thin, r_eff_j, split, max_lag, obs_first, obs_count, workspace_bytes);
    KMC_TRY(sampler_density(s, &q));
    PsisOut out;
    out.tail = tail; out.m = m_j; out.xc = xc_j; out.n_tail = n_tail_j; out.tail_len = tail_len;
    out.r_eff = r_eff_used; out.tail_len_j = tail_len_j; out.n_reff_nan = n_reff_nan;
    return psis(ChainSource(s, false, "kmc_chain_psis_tail_reff"), q, out, n_out, nullptr);
}

KMC_EXPORT kmc_status kmc_chain_psis_tail_reff(kmc_user_density* density, const double* params, const double* chain_host, int64_t nsamples,
                                               int64_t nwalkers, int64_t ndim, int64_t first_sample, const uint8_t* walker_mask, int64_t thin,
                                               const double* r_eff_j, int32_t split, int64_t max_lag, int64_t obs_first, int64_t obs_count,
                                               int64_t workspace_bytes, int device, double* tail, double* m_j, double* xc_j, int32_t* n_tail_j,
                                               int64_t* tail_len, double* r_eff_used, int64_t* tail_len_j, int64_t* n_reff_nan, int64_t* n_out)
{
    PwRequest q = psis_reff_request(first_sample, walker_mask, thin, r_eff_j, split, max_lag, obs_first, obs_count, workspace_bytes);
    q.ud = density; q.params = params;
    PsisOut out;
    out.tail = tail; out.m = m_j; out.xc = xc_j; out.n_tail = n_tail_j; out.tail_len = tail_len;
    out.r_eff = r_eff_used; out.tail_len_j = tail_len_j; out.n_reff_nan = n_reff_nan;
    return psis(ChainSource(chain_host, nullptr, nsamples, nwalkers, ndim, device), q, out, n_out, nullptr);
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
