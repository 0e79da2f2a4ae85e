// kmc_pointwise.hip -- the pointwise log-likelihood of a data density over a stored chain, on the device where the chain, the data and
// the compiled term are: the session every call of the family opens (pw_open: the refusals, then the chain, the stream, the module, the
// arguments), the per-observation statistics behind WAIC (kmc_*_pointwise_stats), the matrix itself for a range of observations
// (kmc_*_pointwise_loglike), the weight series exp(l - M_j) (kmc_*_pointwise_weights) and its relative efficiency per observation
// (kmc_*_relative_eff, whose ESS stage is kmc_convergence.hip's on groups of 64 observations).  PSIS-LOO over the same session:
// kmc_psis.hip; the plans and the host stages: kmc_pointwise_stages.hip; what they share: kmc_pointwise_host.hpp.
// include/kissmcmc_hip.h has the definitions, DESIGN.md sections 4k and 4l the plans.  Kernels: kmc_pointwise.hpp, compiled at run time
// with the density's term as the module "pointwise:<ndim>"; the folds and the PSIS fit, which do not touch the term, are compiled with
// the library.
#include <sstream>

#include "kmc_pointwise_host.hpp"

using namespace kmc_pw_host;

namespace {

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

// pw_open, first part: every refusal and every size that follows from the arguments alone.  Touches no device (a sampler's
// describe() apart): a kmc_chain_* caller with bad arguments runs this and nothing more.
kmc_status pw_check(const ChainSource& src, const PwRequest& q, const void* result, PwSession* S)
{
    ChainView& v = S->v;
    if (!q.ud || !q.ud->is_data) return fail(KMC_ERR_BAD_ARG, "the pointwise log-likelihood needs a data density (kmc_data_density_create): other densities have no per-observation term");
    KMC_TRY(src.describe(&v));
    if (v.ndim > kDataMaxDim) return fail(KMC_ERR_BAD_ARG, "a data density takes at most " + std::to_string(kDataMaxDim) + " dimensions (ndim = " + std::to_string(v.ndim) + ")");
    if (q.sel.thin < 1) return fail(KMC_ERR_BAD_ARG, "thin must be >= 1 (thin = " + std::to_string(q.sel.thin) + ")");
    int64_t n_all = 0;
    KMC_TRY(selection_size(v, q.sel.first_sample, q.sel.walker_mask, &n_all));
    S->kept = (v.nsamples - q.sel.first_sample + q.sel.thin - 1) / q.sel.thin;
    S->nsel = n_all / (v.nsamples - q.sel.first_sample);
    const int64_t n = S->kept * S->nsel;
    if (n < 2) return fail(KMC_ERR_BAD_ARG, "the pointwise statistics need at least 2 selected rows (n = " + std::to_string(n) + ")");
    if (n >= ((int64_t)1 << 40)) return fail(KMC_ERR_UNSUPPORTED, "too many rows for one pointwise call: n = " + std::to_string(n) + ", the limit is 2^40");
    if (q.psis()) KMC_TRY(psis_check(n, q.r_eff, nullptr, q.per_observation_reff()));
    if (q.needs_conv_shape()) {                   // the chains of the weight series: nsel of `kept` samples each
        ChainView gv;
        gv.ld = 64; gv.ndim = 1; gv.nsamples = S->kept; gv.nl = S->nsel;
        KMC_TRY(kmc_conv_host::conv_shape(gv, 0, nullptr, q.split, &S->sh));
        S->max_lag = q.max_lag;
        KMC_TRY(kmc_conv_host::resolve_max_lag(S->sh, &S->max_lag));
    }
    int64_t J = q.ud->ndata;
    if (q.held.data) {
        if (q.held.ncols != q.ud->ncols)
            return fail(KMC_ERR_BAD_ARG, "held-out data of " + std::to_string(q.held.ncols) + " columns: the density's observations have " + std::to_string(q.ud->ncols));
        if (q.held.ndata < 1 || q.held.ndata > kDataMaxRows) return fail(KMC_ERR_BAD_ARG, "held-out data: ndata must be in 1 .. 2^30 (ndata = " + std::to_string(q.held.ndata) + ")");
        J = q.held.ndata;
    }
    if (q.needs_obs_range()) {
        if (q.obs.count < 1) return fail(KMC_ERR_BAD_ARG, "the matrix needs obs_count >= 1 (obs_count = " + std::to_string(q.obs.count) + ")");
        if (q.obs.first < 0 || q.obs.first > J - q.obs.count)
            return fail(KMC_ERR_BAD_ARG, "observations [" + std::to_string(q.obs.first) + ", " + std::to_string(q.obs.first) + " + " + std::to_string(q.obs.count) +
                                             ") lie outside [0, " + std::to_string(J) + ")");
    }
    if (q.supplied_reff()) {
        for (int64_t c = 0; c < q.obs.count; ++c)
            if (!(q.r_eff_j[c] > 0.0) || !std::isfinite(q.r_eff_j[c]))
                return fail(KMC_ERR_BAD_ARG, "r_eff_j must be finite and > 0 (r_eff_j[" + std::to_string(c) + "] = " + std::to_string(q.r_eff_j[c]) + ")");
        KMC_TRY(tail_lengths(n, q.obs.first, q.r_eff_j, q.obs.count, S));
    }
    if (v.is_float) return fail(KMC_ERR_UNSUPPORTED, "a chain of floats: data densities sample in double");
    if (!result || !q.params) return fail(KMC_ERR_BAD_ARG, "null argument");
    S->n = n; S->J = J;
    S->pl = pw_plan(n, J);
    return KMC_OK;
}

// second part: the chain where the kernels read it, the call's stream (ChainSource::stream) and the module
kmc_status pw_device(const ChainSource& src, const PwRequest& q, PwSession* S)
{
    KMC_TRY(src.open(S->b, &S->v));
    HIP_TRY(src.stream(&S->ss));
    return load_pointwise(q.ud, S->v.ndim, !q.held.data, &S->pk);
}

// third part: the arguments every kernel shares, with the list of selected walkers and the held-out observations uploaded
kmc_status pw_args(const PwRequest& q, PwSession* S)
{
    const ChainView& v = S->v;
    PwBuffers& b = S->b;
    PwArgs& a = S->a;
    const hipStream_t st = S->ss.get();
    a.chain = static_cast<const double*>(v.chain);
    a.n = S->n; a.J = S->J; a.nl = v.nl; a.ld = v.ld; a.nsel = S->nsel; a.first = q.sel.first_sample; a.thin = q.sel.thin;
    a.nd = (double)S->n; a.jp_log2 = S->pl.jp_log2;
    for (int i = 0; i < 6; ++i) a.p[i] = q.params[i];
    if (q.sel.walker_mask) {
        std::vector<int32_t> sel;
        for (int64_t w = 0; w < v.nl; ++w) if (q.sel.walker_mask[w]) sel.push_back((int32_t)w);
        HIP_TRY(hipMalloc((void**)&b.sel, sel.size() * sizeof(int32_t)));
        HIP_TRY(copy_sync(b.sel, sel.data(), sel.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        a.sel = b.sel;
    }
    if (q.held.data) {
        const size_t bytes = (size_t)S->J * (size_t)q.held.ncols * sizeof(double);
        KMC_TRY(check_device_room(bytes, "the held-out observations"));
        HIP_TRY(hipMalloc((void**)&b.data, bytes));
        HIP_TRY(copy_sync(b.data, q.held.data, bytes, hipMemcpyHostToDevice, st));
        a.data = b.data;
    } else {
        a.data = static_cast<const double*>(S->pk.keep_data.get());
    }
    a.run_len = S->pl.run_len; a.nruns = S->pl.nruns;
    return KMC_OK;
}

// How reff_stage cuts the range into groups of 64 observations aligned to the absolute index, and the groups into batches that fit the
// work space; the refusal of a group that does not fit the device.
struct ReffPlan {
    int64_t g_first = 0, g_last = 0, ngroups = 0, per_batch = 0;
};

kmc_status reff_plan(int64_t n, const PwRequest& q, ReffPlan* p)
{
    p->g_first = q.obs.first / 64; p->g_last = (q.obs.first + q.obs.count - 1) / 64; p->ngroups = p->g_last - p->g_first + 1;
    const double group_bytes = (double)n * 64.0 * 8.0;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (group_bytes > (double)free_b)
        return fail(KMC_ERR_UNSUPPORTED, "the weight series of one group of 64 observations (" + std::to_string((int64_t)group_bytes) + " bytes, n = " +
                                             std::to_string(n) + ") does not fit the device (" + std::to_string(free_b) + " bytes free): thin the chain");
    const int64_t budget = std::min<int64_t>(workspace_budget(q.workspace), (int64_t)(free_b / 2));
    p->per_batch = std::max<int64_t>(1, std::min<int64_t>(p->ngroups, budget / (int64_t)group_bytes));
    return KMC_OK;
}

// the weight passes of `ng` groups from group g0 on, into wa.a.out
hipError_t weights_batch(const PwSession& S, WeightArgs& wa, int64_t g0, int64_t ng)
{
    wa.group0 = g0;
    return launch_module_y(S.pk.weights, (unsigned)ng, (unsigned)((matrix_waves(S.n) + kPwWaves - 1) / kPwWaves), kPwThreads, S.ss.get(), wa);
}

// one group [n][64] on the device and its live lanes [lo, hi], which are the observations c0 + (lo .. hi) of the range
struct ReffGroup {
    const double* series;
    int64_t lo, hi, c0;
};

// Weights: the live lanes of a group copied into the dense series o.v [n][count]
kmc_status scatter_series(const PwSession& S, const ReffGroup& g, int64_t count, std::vector<double>& host_group, double* v)
{
    HIP_TRY(copy_sync(host_group.data(), g.series, host_group.size() * sizeof(double), hipMemcpyDeviceToHost, S.ss.get()));
    for (int64_t k = 0; k < S.n; ++k)
        for (int64_t l = g.lo; l <= g.hi; ++l) v[k * count + (g.c0 + l)] = host_group[(size_t)(k * 64 + l)];
    return KMC_OK;
}

// ... or the effective sample size of its columns, by the convergence diagnostics' stages on the group as a chain [kept][nsel][64]
kmc_status scatter_ess(const PwSession& S, const ReffGroup& g, kmc_conv_host::ConvBuffers& cb, const ReffOut& o)
{
    ChainView gv;
    gv.ld = 64; gv.nsamples = S.n / S.a.nsel; gv.nl = S.a.nsel;
    gv.chain = g.series;
    gv.ndim = g.hi + 1;                                                                // (the lanes below lo are constant 0.0: no ESS, no lags)
    double mean[64], W[64], B[64], vp[64], rhat[64], ess[64], mcse[64];
    int64_t T[64];
    int32_t flags[64];
    const kmc_conv_host::StatsOut so{mean, W, B, vp, rhat, ess, mcse, T, flags};
    KMC_TRY(kmc_conv_host::convergence_on_stream(cb, gv, S.sh, false, S.max_lag, so, nullptr, S.ss.get()));
    const double mh = (double)S.sh.m * (double)S.sh.h;
    for (int64_t l = g.lo; l <= g.hi; ++l) {
        const int64_t c = g.c0 + l;
        if (o.r_eff) o.r_eff[c] = ess[l] / mh;
        if (o.ess) o.ess[c] = ess[l];
        if (o.T) o.T[c] = T[l];
        if (o.flags) o.flags[c] = flags[l];
    }
    return KMC_OK;
}

}  // namespace

namespace kmc_pw_host {

// the refusals, then the chain, the stream, the module and the arguments every kernel shares
kmc_status pw_open(const ChainSource& src, const PwRequest& q, const void* result, PwSession* S)
{
    KMC_TRY(pw_check(src, q, result, S));
    KMC_TRY(pw_device(src, q, S));
    return pw_args(q, S);
}

// the two passes of the statistics, left on the device: work gets the work space, a.stats [4][J]
kmc_status pw_stats(PwSession& S, double** work, int64_t* info, int npass)
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
    TimedEvents<3> ev;                            // around the two passes, for info: each pass is its partial kernel and its fold
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
        info[0] = n; info[1] = pl.nruns; info[2] = 2 * n * J; info[3] = pl.run_len;
        HIP_TRY(ev.elapsed_ns(0, 1, &info[4]));
        HIP_TRY(ev.elapsed_ns(1, 2, &info[5]));
    }
    return KMC_OK;
}

// The weight series v = exp(l - M_j) of the observations [obs.first, obs.first + obs.count), in groups of 64 observations aligned to
// the absolute index, and the effective sample size of every column by the convergence diagnostics' own stages (kmc_convergence.hip)
// on each group as a chain [kept][nsel][64].  ld = 64 whatever the group holds: lags_device then has period = 1 and a lane owns one
// column, so the grid and the order of a column's additions follow from the selection's shape alone -- not from the group, the other
// columns, the range or the work space.  Needs a.stats of pass 1.  info3: nanoseconds of the weight passes, of the ESS stage, groups.
kmc_status reff_stage(PwSession& S, const PwRequest& q, const ReffOut& o, int64_t* info3)
{
    const int64_t n = S.n, count = q.obs.count;
    hipStream_t st = S.ss.get();
    KMC_TRY(load_weights(q.ud, S.v.ndim, &S.pk));
    ReffPlan p;
    KMC_TRY(reff_plan(n, q, &p));
    double* buf = nullptr;
    HIP_TRY(hipMalloc((void**)&buf, (size_t)p.per_batch * (size_t)n * 64 * sizeof(double)));
    std::shared_ptr<void> keep(buf, [](void* ptr) { (void)hipFree(ptr); });

    WeightArgs wa{};
    wa.a = S.a;
    wa.a.out = buf; wa.a.obs_first = q.obs.first; wa.a.obs_count = count;
    wa.a.run_len = matrix_run_len(n);
    kmc_conv_host::ConvBuffers cb;
    if (!o.v) KMC_TRY(kmc_conv_host::upload_rank(cb, nullptr, S.a.nsel, st));
    std::vector<double> host_group;
    if (o.v) host_group.resize((size_t)n * 64);

    TimedEvents<3> ev;
    if (info3) HIP_TRY(ev.create());
    int64_t ns_w = 0, ns_e = 0;
    for (int64_t g0 = p.g_first; g0 <= p.g_last; g0 += p.per_batch) {
        const int64_t ng = std::min(p.per_batch, p.g_last - g0 + 1);
        if (info3) HIP_TRY(hipEventRecord(ev.e[0], st));
        HIP_TRY(weights_batch(S, wa, g0, ng));
        if (info3) HIP_TRY(hipEventRecord(ev.e[1], st));
        for (int64_t i = 0; i < ng; ++i) {
            const int64_t j0 = (g0 + i) * 64;
            const ReffGroup g{buf + (size_t)i * (size_t)n * 64, std::max<int64_t>(0, q.obs.first - j0), std::min<int64_t>(63, q.obs.first + count - 1 - j0),
                              j0 - q.obs.first};
            if (o.v) KMC_TRY(scatter_series(S, g, count, host_group, o.v));
            else KMC_TRY(scatter_ess(S, g, cb, o));
        }
        if (info3) {
            HIP_TRY(hipEventRecord(ev.e[2], st));
            HIP_TRY(hipStreamSynchronize(st));
            int64_t t0 = 0, t1 = 0;
            HIP_TRY(ev.elapsed_ns(0, 1, &t0));
            HIP_TRY(ev.elapsed_ns(1, 2, &t1));
            ns_w += t0; ns_e += t1;
        }
    }
    HIP_TRY(hipStreamSynchronize(st));                                                 // (buf goes with this scope)
    if (info3) { info3[0] = ns_w; info3[1] = ns_e; info3[2] = p.ngroups; }
    return KMC_OK;
}

}  // namespace kmc_pw_host

namespace {

// Matrix: out [n][obs.count]
kmc_status pw_matrix_out(PwSession& S, const PwRequest& q, double* result, int64_t* info)
{
    PwArgs& a = S.a;
    const int64_t n = S.n, count = q.obs.count;
    const double need = (double)n * (double)count * 8.0;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (need > (double)free_b)
        return fail(KMC_ERR_UNSUPPORTED, "a matrix of " + std::to_string(n) + " x " + std::to_string(count) + " log-likelihoods (" +
                                             std::to_string((int64_t)(need / 1048576.0)) + " MiB) does not fit the device (" + std::to_string(free_b >> 20) +
                                             " MiB free): ask for fewer observations at a time, or thin");
    const size_t bytes = (size_t)n * (size_t)count * sizeof(double);
    HIP_TRY(hipMalloc((void**)&S.b.work, bytes));
    a.out = S.b.work; a.obs_first = q.obs.first; a.obs_count = count;
    a.run_len = matrix_run_len(n);
    const int64_t waves = matrix_waves(n);
    HIP_TRY(launch_module_y(S.pk.matrix, (unsigned)((count + 63) / 64), (unsigned)((waves + kPwWaves - 1) / kPwWaves), kPwThreads, S.ss.get(), a));
    HIP_TRY(copy_sync(result, S.b.work, bytes, hipMemcpyDeviceToHost, S.ss.get()));
    if (info) { info[0] = n; info[1] = waves; info[2] = n * count; info[3] = a.run_len; }
    return KMC_OK;
}

// stats [4][J] (Stats), out [n][obs.count] (Matrix) or the series [n][obs.count] (Weights): the request filled once for both routes
kmc_status pointwise(const ChainSource& src, PwMode mode, const PwDensity& d, const Selection& sel, const HeldOut& held, const ObsRange& obs, double* result,
                     double* weights_M, int64_t* n_out, int64_t* info)
{
    PwRequest q;
    KMC_TRY(q.begin(mode, d, sel));
    q.held = held; q.obs = obs; q.weights_M = weights_M;
    PwSession S;
    KMC_TRY(pw_open(src, q, result, &S));
    if (n_out) *n_out = S.n;
    if (mode == PwMode::Matrix) return pw_matrix_out(S, q, result, info);
    if (mode == PwMode::Weights) {
        KMC_TRY(pw_stats(S, &S.b.work, nullptr, 1));
        ReffOut o;
        o.v = result;
        KMC_TRY(reff_stage(S, q, o, nullptr));
        if (weights_M) HIP_TRY(copy_sync(weights_M, S.a.stats + obs.first, (size_t)obs.count * sizeof(double), hipMemcpyDeviceToHost, S.ss.get()));
        return KMC_OK;
    }
    KMC_TRY(pw_stats(S, &S.b.work, info));
    HIP_TRY(copy_sync(result, S.a.stats, 4 * (size_t)S.J * sizeof(double), hipMemcpyDeviceToHost, S.ss.get()));
    return KMC_OK;
}

// r_eff_j = ess_j / (m h) of the weight series, alone.  info [6]: n, groups, nanoseconds of pass 1, of the weight passes, of the ESS
// stage (moments, lags and their copies per group), h.
kmc_status relative_eff(const ChainSource& src, const PwDensity& d, const Selection& sel, const ObsRange& obs, int32_t split, int64_t max_lag,
                        int64_t workspace, const ReffOut& o, int64_t* m_out, int64_t* h_out, int64_t* n_out, int64_t* info)
{
    PwRequest q;
    KMC_TRY(q.begin(PwMode::RelativeEff, d, sel));
    q.obs = obs; q.workspace = workspace; q.split = split != 0; q.max_lag = max_lag;
    PwSession S;
    KMC_TRY(pw_open(src, q, o.r_eff, &S));
    if (m_out) *m_out = S.sh.m;
    if (h_out) *h_out = S.sh.h;
    if (n_out) *n_out = S.n;
    TimedEvents<2> ev;
    if (info) { HIP_TRY(ev.create()); HIP_TRY(hipEventRecord(ev.e[0], S.ss.get())); }
    KMC_TRY(pw_stats(S, &S.b.work, nullptr, 1));
    if (info) HIP_TRY(hipEventRecord(ev.e[1], S.ss.get()));
    int64_t i3[3] = {};
    KMC_TRY(reff_stage(S, q, o, info ? i3 : nullptr));
    if (info) {
        info[0] = S.n; info[1] = i3[2]; info[3] = i3[0]; info[4] = i3[1]; info[5] = S.sh.h;
        HIP_TRY(ev.elapsed_ns(0, 1, &info[2]));
    }
    return KMC_OK;
}

}  // namespace

KMC_EXPORT kmc_status kmc_sampler_pointwise_stats(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int64_t thin, const double* data,
                                                  int64_t ndata2, int32_t ncols2, double* stats, int64_t* n_out, int64_t* info)
{
    return pointwise(ChainSource(s, false, "kmc_chain_pointwise_stats"), PwMode::Stats, sampler_density(s), {first_sample, walker_mask, thin},
                     {data, ndata2, ncols2}, {}, stats, nullptr, n_out, info);
}

KMC_EXPORT kmc_status kmc_chain_pointwise_stats(kmc_user_density* density, const double* params, const double* chain_host, int64_t nsamples,
                                                int64_t nwalkers, int64_t ndim, int64_t first_sample, const uint8_t* walker_mask, int64_t thin,
                                                const double* data, int64_t ndata2, int32_t ncols2, int device, double* stats, int64_t* n_out,
                                                int64_t* info)
{
    return pointwise(ChainSource(chain_host, nullptr, nsamples, nwalkers, ndim, device), PwMode::Stats, {density, params}, {first_sample, walker_mask, thin},
                     {data, ndata2, ncols2}, {}, stats, nullptr, n_out, info);
}

KMC_EXPORT kmc_status kmc_sampler_pointwise_loglike(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int64_t thin, const double* data,
                                                    int64_t ndata2, int32_t ncols2, int64_t obs_first, int64_t obs_count, double* out, int64_t* n_out)
{
    return pointwise(ChainSource(s, false, "kmc_chain_pointwise_loglike"), PwMode::Matrix, sampler_density(s), {first_sample, walker_mask, thin},
                     {data, ndata2, ncols2}, {obs_first, obs_count}, out, nullptr, n_out, nullptr);
}

KMC_EXPORT kmc_status kmc_chain_pointwise_loglike(kmc_user_density* density, const double* params, const double* chain_host, int64_t nsamples,
                                                  int64_t nwalkers, int64_t ndim, int64_t first_sample, const uint8_t* walker_mask, int64_t thin,
                                                  const double* data, int64_t ndata2, int32_t ncols2, int64_t obs_first, int64_t obs_count,
                                                  int device, double* out, int64_t* n_out)
{
    return pointwise(ChainSource(chain_host, nullptr, nsamples, nwalkers, ndim, device), PwMode::Matrix, {density, params}, {first_sample, walker_mask, thin},
                     {data, ndata2, ncols2}, {obs_first, obs_count}, out, nullptr, n_out, nullptr);
}

KMC_EXPORT kmc_status kmc_sampler_pointwise_weights(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int64_t thin, const double* data,
                                                    int64_t ndata2, int32_t ncols2, int64_t obs_first, int64_t obs_count, double* v, double* M_j,
                                                    int64_t* n_out)
{
    return pointwise(ChainSource(s, false, "kmc_chain_pointwise_weights"), PwMode::Weights, sampler_density(s), {first_sample, walker_mask, thin},
                     {data, ndata2, ncols2}, {obs_first, obs_count}, v, M_j, n_out, nullptr);
}

KMC_EXPORT kmc_status kmc_chain_pointwise_weights(kmc_user_density* density, const double* params, const double* chain_host, int64_t nsamples,
                                                  int64_t nwalkers, int64_t ndim, int64_t first_sample, const uint8_t* walker_mask, int64_t thin,
                                                  const double* data, int64_t ndata2, int32_t ncols2, int64_t obs_first, int64_t obs_count, int device,
                                                  double* v, double* M_j, int64_t* n_out)
{
    return pointwise(ChainSource(chain_host, nullptr, nsamples, nwalkers, ndim, device), PwMode::Weights, {density, params}, {first_sample, walker_mask, thin},
                     {data, ndata2, ncols2}, {obs_first, obs_count}, v, M_j, n_out, nullptr);
}

KMC_EXPORT kmc_status kmc_sampler_relative_eff(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int64_t thin, int64_t obs_first,
                                               int64_t obs_count, int32_t split, int64_t max_lag, int64_t workspace_bytes, double* r_eff_j, double* ess_j,
                                               int64_t* T_j, int32_t* flags_j, int64_t* m_out, int64_t* h_out, int64_t* n_out, int64_t* info)
{
    return relative_eff(ChainSource(s, false, "kmc_chain_relative_eff"), sampler_density(s), {first_sample, walker_mask, thin}, {obs_first, obs_count}, split,
                        max_lag, workspace_bytes, {r_eff_j, ess_j, T_j, flags_j}, m_out, h_out, n_out, info);
}

KMC_EXPORT kmc_status kmc_chain_relative_eff(kmc_user_density* density, const double* params, const double* chain_host, int64_t nsamples, int64_t nwalkers,
                                             int64_t ndim, int64_t first_sample, const uint8_t* walker_mask, int64_t thin, int64_t obs_first,
                                             int64_t obs_count, int32_t split, int64_t max_lag, int64_t workspace_bytes, int device, double* r_eff_j,
                                             double* ess_j, int64_t* T_j, int32_t* flags_j, int64_t* m_out, int64_t* h_out, int64_t* n_out, int64_t* info)
{
    return relative_eff(ChainSource(chain_host, nullptr, nsamples, nwalkers, ndim, device), {density, params}, {first_sample, walker_mask, thin},
                        {obs_first, obs_count}, split, max_lag, workspace_bytes, {r_eff_j, ess_j, T_j, flags_j}, m_out, h_out, n_out, info);
}
