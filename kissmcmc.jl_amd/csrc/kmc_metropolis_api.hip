// kmc_metropolis_api.hip -- host side of the many-chain Metropolis entry points of include/kissmcmc_hip.h
// (kmc_metropolis_validate / kmc_metropolis_run; kernels: kmc_metropolis.hpp).  kmc_metropolis_run is six steps: the argument checks
// and validate, the device, metropolis_density_params, metropolis_setup (one MetroRun: the facts of the config, the stream, one
// MetroBuffers), one route -- metropolis_host_route (caller's closures, an iteration per pass), metropolis_device_route
// (metropolis_device_setup, metropolis_select_kernels, then metropolis_launch_stretch per launch) or metropolis_hmc_route (the HMC step,
// kmc_hmc.hpp) -- and metropolis_read_out.  Also here: kmc_user_density_set_grad and kmc_grad_eval_host.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>

#define KMC_DEFINE_METROPOLIS_KERNELS
#include "kmc_host.hpp"
#include "kmc_chain_view.hpp"
#include "kmc_hmc.hpp"

using namespace kmc;
using namespace kmc_host;

// ------------------------------------------------------------------------------------------
// Many-chain Metropolis: metropolis / _metropolis, reference src/samplers.jl:59-128.
// ------------------------------------------------------------------------------------------
namespace {

int metropolis_nd(int64_t ndim) { return ndim <= 1 ? 1 : ndim <= 2 ? 2 : ndim <= 4 ? 4 : ndim <= 8 ? 8 : ndim <= 16 ? 16 : ndim <= 32 ? 32 : 0; }

// runtime-compiled density: the Metropolis kernel (and the initial log-pdf kernel) for one register geometry
// (TND > 0: also the few-chains kernel that reads its draws from a table, chains in registers -- body densities included)
// (mv: the same program with the covariance-shaped proposal theta + L z in kmc_user_metropolis -- a program of its own, with its own
// name and key; the isotropic programs keep their text and their cache entries)
kmc_status compile_user_metropolis(kmc_user_density* ud, int ND, const std::vector<char>** out, int64_t ndim = 0, int TND = 0, bool mv = false)
{
    if (ud->is_body) ND = 0;                     // a body density: the chain-in-memory kernel (the proposal is collected per lane)
    char key[64];
    std::snprintf(key, sizeof(key), mv ? "MV:%d:%lld:%d" : "M:%d:%lld:%d", ND, ud->is_body ? (long long)ndim : 0ll, TND);
    static const RtcModule m{"user density", "kmc_user_metropolis.hip", {"kmc_kernels.hpp", "kmc_device.hpp", "kmc_metropolis.hpp"}, rtc_options()};
    static const RtcModule mmv{"user density", "kmc_user_metropolis_mv.hip", {"kmc_kernels.hpp", "kmc_device.hpp", "kmc_metropolis.hpp"}, rtc_options()};
    return compile_keyed(ud, key, mv ? mmv : m, [&](std::string* text) {
        std::ostringstream src;
        src << "#include \"kmc_kernels.hpp\"\n#include \"kmc_metropolis.hpp\"\n" << user_functor_source(ud) << user_density_alias(ud, ndim)
            << "extern \"C\" __global__ __launch_bounds__(256) void kmc_user_logpdf(const kmc::LogpdfArgs a) { kmc::logpdf_rows_body<UD>(a); }\n"
            << "extern \"C\" __global__ __launch_bounds__(256) void kmc_user_metropolis(const kmc::MetropolisArgs a) { ";
        if (mv && ND > 0) src << "kmc::metropolis_chains_body<UD, " << ND << ", true>(a); }\n";
        else if (mv) src << "kmc::metropolis_chains_any_body<UD, true>(a); }\n";
        else if (ND > 0) src << "kmc::metropolis_chains_body<UD, " << ND << ">(a); }\n";
        else src << "kmc::metropolis_chains_any_body<UD>(a); }\n";
        if (TND > 0)
            src << "extern \"C\" __global__ __launch_bounds__(128) void kmc_user_metropolis_tabled(const kmc::MetropolisTabledArgs t) { "
                << "kmc::metropolis_chains_tabled_body<UD, " << TND << ">(t.a, t.draws, t.nsteps); }\n";
        *text = src.str();
        return KMC_OK;
    }, out);
}

// A body density with a gradient (kmc_user_density_set_grad): the functor of its two bodies, and the module of the HMC step for one
// ndim -- a template constant there (as for a data density), so that a body's `for (i < n)` unrolls and its arrays stay in registers.
constexpr int64_t kHmcMaxDim = 32;                // the chain lives in registers (kmc_hmc.hpp)
constexpr int32_t kHmcMaxLeap = 1024;

std::string hmc_functor_source(const kmc_user_density* ud, const std::string& grad_body)
{
    std::ostringstream src;
    src << "namespace {\nstruct UserB {\n"
        << "  __device__ static double eval(const double* x, int n, const double* p) { (void)x; (void)n; (void)p;\n" << ud->body << "\n  }\n"
        << "  __device__ static void grad(const double* x, int n, const double* p, double* g) { (void)x; (void)n; (void)p; (void)g;\n" << grad_body << "\n  }\n};\n}\n";
    return src.str();
}

const RtcModule& hmc_rtc_module()
{
    static const RtcModule m{"user density", "kmc_user_hmc.hip", {"kmc_kernels.hpp", "kmc_device.hpp", "kmc_metropolis.hpp", "kmc_hmc.hpp"}, rtc_options()};
    return m;
}

// The identity of a gradient body in the keys of a density's code objects: FNV-1a over its text, and its length.
std::string hmc_grad_id(const std::string& grad_body)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (const unsigned char ch : grad_body) h = (h ^ ch) * 0x100000001b3ull;
    char buf[48];
    std::snprintf(buf, sizeof(buf), "%016llx.%zu", (unsigned long long)h, grad_body.size());
    return buf;
}

// The code object of the density's CURRENT gradient for one ndim, under the key "hmc:<gradient id>:<ndim>".  Code objects are never
// erased from ud->code -- shared_module keys the loaded modules by their addresses -- so a replaced gradient's entries stay, unused,
// and the body read here is the one the key names whatever another thread sets meanwhile.
kmc_status compile_user_hmc(kmc_user_density* ud, int64_t ndim, const std::vector<char>** out)
{
    std::string grad_body;
    { std::lock_guard<std::mutex> lock(ud->mu); grad_body = ud->grad_body; }
    return compile_keyed(ud, "hmc:" + hmc_grad_id(grad_body) + ":" + std::to_string(ndim), hmc_rtc_module(), [&](std::string* text) {
        std::ostringstream src;
        src << "#include \"kmc_kernels.hpp\"\n#include \"kmc_hmc.hpp\"\n" << hmc_functor_source(ud, grad_body)
            << "using UD = kmc::BodyGradDensity<UserB, " << ndim << ">;\n"
            << "extern \"C\" __global__ __launch_bounds__(256) void kmc_user_logpdf(const kmc::LogpdfArgs a) { kmc::logpdf_rows_body<UD>(a); }\n"
            << "extern \"C\" __global__ __launch_bounds__(256) void kmc_user_hmc(const kmc::HmcArgs h) { kmc::metropolis_hmc_body<UD, " << ndim << ", true>(h); }\n"
            << "extern \"C\" __global__ __launch_bounds__(256) void kmc_user_grad(const kmc::GradArgs a) { kmc::grad_rows_body<UD, " << ndim << ", true>(a); }\n";
        *text = src.str();
        return KMC_OK;
    }, out);
}

template <class T>
hipError_t metro_alloc(T** p, size_t bytes) { return cache_alloc(reinterpret_cast<void**>(p), bytes); }

constexpr int64_t kMetroCholMaxDim = 128;         // L is ndim^2 / 2 doubles read per step and lane; nothing larger is tested

// the Cholesky factorisation of include/kissmcmc_hip.h (kmc_cholesky_lower): fixed order, every operation rounded on its own
// (the library is built with -ffp-contract=off).  Returns the failing pivot, or -1.
int cholesky_lower(const double* a, int64_t n, double* L)
{
    for (int64_t i = 0; i < n; ++i) {
        for (int64_t j = 0; j <= i; ++j) {
            double s = a[i * n + j];
            for (int64_t k = 0; k < j; ++k) {
                const double t = L[i * n + k] * L[j * n + k];
                s = s - t;
            }
            if (j < i) L[i * n + j] = s / L[j * n + j];
            else {
                if (!(std::isfinite(s) && s > 0.0)) return (int)i;
                L[i * n + i] = std::sqrt(s);
            }
        }
        for (int64_t j = i + 1; j < n; ++j) L[i * n + j] = 0.0;
    }
    return -1;
}

// The proposal of one run with `chol` or tuning: theta + L z (kmc_metropolis.hpp), L packed by rows on the device, replaced at the
// tuning boundaries by the Cholesky factor of the scaled covariance of the chains' current states.
struct MetroShape {
    bool on = false;                  // false: the isotropic route, theta + step .* z
    int64_t nd = 0;
    std::vector<double> L;            // host [nd][nd], upper triangle 0.0
    std::vector<int64_t> bounds;      // the tuning boundaries b_r, ascending and distinct
    double scale = 0.0;
    int64_t skipped = 0;
    double tune_ms = 0.0;
    double* dev = nullptr;            // device: the packed lower triangle (owned by the run's buffers)

    void init(const kmc_metropolis_config* c)
    {
        on = c->chol != nullptr || c->tune_rounds > 0;
        nd = c->ndim;
        if (!on) return;
        L.assign((size_t)(nd * nd), 0.0);
        for (int64_t i = 0; i < nd; ++i) {
            if (c->chol) for (int64_t j = 0; j <= i; ++j) L[(size_t)(i * nd + j)] = c->chol[i * nd + j];
            else L[(size_t)(i * nd + i)] = c->step[i];
        }
        scale = c->tune_scale > 0.0 ? c->tune_scale : 2.38 / std::sqrt((double)nd);
        for (int64_t r = 1; r <= c->tune_rounds; ++r) {
            const int64_t b = (int64_t)(((__int128)r * c->nburnin) / (c->tune_rounds + 1));
            if (bounds.empty() || bounds.back() != b) bounds.push_back(b);
        }
    }
    // (room for a 32 x 32 triangle at least: the register kernels index it with compile-time offsets)
    size_t dev_doubles() const { const int64_t m = std::max<int64_t>(nd, 32); return (size_t)(m * (m + 1) / 2); }
    hipError_t alloc(double** p, hipStream_t st)
    {
        hipError_t e = metro_alloc(p, dev_doubles() * sizeof(double));
        if (e != hipSuccess) return e;
        dev = *p;
        e = fill_sync(dev, 0, dev_doubles() * sizeof(double), st);
        return e != hipSuccess ? e : upload(st);
    }
    hipError_t upload(hipStream_t st)
    {
        std::vector<double> packed((size_t)(nd * (nd + 1) / 2));
        for (int64_t i = 0; i < nd; ++i)
            for (int64_t j = 0; j <= i; ++j) packed[(size_t)(i * (i + 1) / 2 + j)] = L[(size_t)(i * nd + j)];
        return copy_sync(dev, packed.data(), packed.size() * sizeof(double), hipMemcpyHostToDevice, st);
    }
    bool boundary(int64_t it) const { return std::binary_search(bounds.begin(), bounds.end(), it); }
    int64_t next_boundary(int64_t it, int64_t end) const      // the first boundary after `it`, or `end`
    {
        const auto b = std::upper_bound(bounds.begin(), bounds.end(), it);
        return b == bounds.end() ? end : std::min(*b, end);
    }
    // one tuning boundary: pos_dev [nc][nd] are the chains' current states, everything queued on `st` before is waited for
    kmc_status tune(const double* pos_dev, int64_t nc, hipStream_t st)
    {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<double> mean((size_t)nd), cov((size_t)(nd * nd)), Ln((size_t)(nd * nd));
        KMC_TRY(kmc_chain_view::covariance_of_rows(pos_dev, nc, nd, st, mean.data(), cov.data()));
        const double s2 = scale * scale;
        for (double& v : cov) v = s2 * v;
        if (cholesky_lower(cov.data(), nd, Ln.data()) >= 0) ++skipped;       // the previous L stays
        else {
            L.swap(Ln);
            HIP_TRY(upload(st));
        }
        tune_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return KMC_OK;
    }
    void report(kmc_metropolis_outputs* out) const
    {
        out->tune_skipped = skipped;
        out->tune_ms = tune_ms;
    }
};

// kmc_metropolis_outputs.chol_out: the L in force at the end
void write_chol_out(const kmc_metropolis_config* c, const MetroShape& sh, kmc_metropolis_outputs* out)
{
    if (!out->chol_out) return;
    const int64_t nd = c->ndim;
    if (sh.on) std::copy(sh.L.begin(), sh.L.end(), out->chol_out);
    else
        for (int64_t i = 0; i < nd; ++i)
            for (int64_t j = 0; j < nd; ++j) out->chol_out[i * nd + j] = (i == j && c->step) ? c->step[i] : 0.0;
}

// the digested parameters of the config's density (a menu density's are checked on the way: kmc_metropolis_validate's last refusals)
kmc_status metropolis_density_params(const kmc_metropolis_config* c, DensityParams* dp)
{
    kmc_config e{};
    e.density = c->density;
    for (int i = 0; i < 8; ++i) e.params[i] = c->params[i];
    e.ndim = c->ndim;
    e.user_density = c->user_density;
    return digest_params(e, dp);
}

// device and page-locked host buffers of one kmc_metropolis_run call, whichever route it takes
struct MetroBuffers {
    double *pos = nullptr, *logp = nullptr, *chain = nullptr, *chain_logp = nullptr, *csum = nullptr, *csumsq = nullptr;
    uint32_t* naccept = nullptr;
    double *step = nullptr, *chol = nullptr;      // the proposal: a scale per dimension, the packed L of a covariance-shaped one
    double *xt = nullptr, *yt = nullptr, *st1 = nullptr, *st2 = nullptr;     // device route, chains in memory: dimension-major state and moment sums
    double *blob = nullptr, *chain_blob = nullptr;
    double* draws = nullptr;          // few chains: the draw table of a launch (metro_draw_fill)
    double *prop = nullptr, *p1 = nullptr;                                   // host route: the proposals and their log-pdfs ...
    unsigned char *acc = nullptr, *h_acc = nullptr;                          // ... the accept decisions (host_accepted) ...
    double *h_rows = nullptr, *h_prop = nullptr, *h_p1 = nullptr;            // ... and, page-locked as h_acc, what crosses to the callbacks
    std::shared_ptr<void> keep;       // the module of a runtime-compiled density
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipStream_t stream = nullptr;     // the stream the buffers were used on: waited for before they go back to the allocation cache
    ~MetroBuffers()
    {
        if (stream) (void)hipStreamSynchronize(stream);
        for (void* p : {(void*)pos, (void*)logp, (void*)chain, (void*)chain_logp, (void*)csum, (void*)csumsq, (void*)naccept, (void*)step, (void*)chol,
                        (void*)xt, (void*)yt, (void*)st1, (void*)st2, (void*)blob, (void*)chain_blob, (void*)draws, (void*)prop, (void*)p1, (void*)acc})
            cache_free(p);
        for (void* p : {(void*)h_rows, (void*)h_prop, (void*)h_p1, (void*)h_acc})
            if (p) (void)hipHostFree(p);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};

// One kmc_metropolis_run call: what both routes derive from the config, the stream and the buffers.  (Members die in reverse
// order: the buffers wait for the stream and go back to the allocation cache first, then the stream itself is destroyed.)
struct MetroRun {
    const kmc_metropolis_config* c = nullptr;
    int64_t nc = 0, nd = 0, nsamples = 0;
    size_t rows = 0, vec = 0;         // bytes of one [nchains][ndim] block and of one value per chain
    unsigned grid = 0;                // workgroups of 256 over the chains
    bool want_chain = false, want_logp = false, want_mom = false, want_blobs = false;
    int nblob = 0;
    DensityParams dp{};
    MetroShape sh;
    ScopedStream ss;                  // never the legacy stream (kmc_host.hpp: copy_sync)
    MetroBuffers b;
};

// The set-up both routes share: the stream, the chains' state from theta0, the counters, the chain and the moment sums.
kmc_status metropolis_setup(const kmc_metropolis_config* c, const double* theta0, const kmc_metropolis_outputs* out, MetroRun* R)
{
    MetroBuffers& b = R->b;
    R->c = c;
    R->nc = c->nchains; R->nd = c->ndim; R->nsamples = out->nsamples;
    R->rows = (size_t)R->nc * (size_t)R->nd * sizeof(double);
    R->vec = (size_t)R->nc * sizeof(double);
    R->grid = (unsigned)((R->nc + 255) / 256);
    R->want_chain = (c->flags & KMC_STORE_CHAIN) != 0; R->want_logp = (c->flags & KMC_STORE_LOGP) != 0; R->want_mom = (c->flags & KMC_MOMENTS) != 0;
    R->nblob = c->density == KMC_USER_DENSITY ? static_cast<const kmc_user_density*>(c->user_density)->nblob : 0;
    R->want_blobs = R->nblob > 0 && ((c->flags & KMC_STORE_BLOBS) != 0 || out->blobs != nullptr);
    R->sh.init(c);
    HIP_TRY(R->ss.create());
    const hipStream_t st = b.stream = R->ss.st;
    const size_t rows = R->rows, vec = R->vec, ns = (size_t)R->nsamples;
    HIP_TRY(metro_alloc(&b.pos, rows));
    HIP_TRY(metro_alloc(&b.logp, vec));
    HIP_TRY(metro_alloc(&b.naccept, (size_t)R->nc * sizeof(uint32_t)));
    HIP_TRY(fill_sync(b.naccept, 0, (size_t)R->nc * sizeof(uint32_t), st));
    HIP_TRY(copy_sync(b.pos, theta0, rows, hipMemcpyHostToDevice, st));                              // :68 deepcopy
    if ((R->want_chain || R->want_logp) && ns > 0)
        KMC_TRY(check_device_room(ns * ((R->want_chain ? rows : 0) + (R->want_logp ? vec : 0)), "the Metropolis chain"));
    if (R->want_chain && ns > 0) HIP_TRY(metro_alloc(&b.chain, ns * rows));
    if (R->want_logp && ns > 0) HIP_TRY(metro_alloc(&b.chain_logp, ns * vec));
    if (R->sh.on) HIP_TRY(R->sh.alloc(&b.chol, st));
    if (R->want_mom) {
        HIP_TRY(metro_alloc(&b.csum, rows));
        HIP_TRY(metro_alloc(&b.csumsq, rows));
        HIP_TRY(fill_sync(b.csum, 0, rows, st));
        HIP_TRY(fill_sync(b.csumsq, 0, rows, st));
    }
    HIP_TRY(hipEventCreate(&b.ev0));
    HIP_TRY(hipEventCreate(&b.ev1));
    return KMC_OK;
}

// log-pdf of device rows -> device vector (and those rows' blobs, or nullptr): a module's function, or the menu density's
hipError_t launch_logpdf(const MetroRun& R, hipFunction_t ulp, const double* rows_dev, double* out_dev, double* blob_dev)
{
    const LogpdfArgs la{rows_dev, out_dev, R.nc, (int32_t)R.nd, (int32_t)R.nd, R.dp, blob_dev};
    if (ulp) return launch_module(ulp, R.grid, 256u, R.ss.st, la);
    hipLaunchKernelGGL(logpdf_fn(R.c->density), dim3(R.grid), dim3(256), 0, R.ss.st, la);
    return hipGetLastError();
}

// The read-out both routes share: device_ms between the two events the route recorded, the tuning report, every output asked for.
// (The host route has no blobs: those branches see null pointers.)
kmc_status metropolis_read_out(MetroRun& R, kmc_metropolis_outputs* out)
{
    const kmc_metropolis_config* c = R.c;
    const MetroBuffers& b = R.b;
    const hipStream_t st = R.ss.st;
    const int64_t nc = R.nc, nd = R.nd, nsamples = R.nsamples, nblob = R.nblob;
    const size_t rows = R.rows, vec = R.vec, bb = (size_t)nc * (size_t)nblob * sizeof(double);
    HIP_TRY(hipStreamSynchronize(st));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, b.ev0, b.ev1));
    out->device_ms = (double)ms;
    R.sh.report(out);
    if (!c->host_propose) write_chol_out(c, R.sh, out);        // (proposals from the host: there is no L)
    if (c->flags & KMC_CHAIN_BY_WALKER) {       // thetas[chain][sample], as the reference returns them (:113, :128)
        if (out->chain && b.chain) KMC_TRY(download_by_walker(b.chain, false, nc, nd, nd, nsamples, out->chain, st));
        if (out->chain_logp && b.chain_logp) KMC_TRY(download_by_walker(b.chain_logp, false, nc, 1, 1, nsamples, out->chain_logp, st));
        if (out->blobs && b.chain_blob) KMC_TRY(download_by_walker(b.chain_blob, false, nc, nblob, nblob, nsamples, out->blobs, st));      // (:117)
    } else {
        if (out->chain && b.chain) HIP_TRY(copy_sync(out->chain, b.chain, (size_t)nsamples * rows, hipMemcpyDeviceToHost, st));
        if (out->chain_logp && b.chain_logp) HIP_TRY(copy_sync(out->chain_logp, b.chain_logp, (size_t)nsamples * vec, hipMemcpyDeviceToHost, st));
        if (out->blobs && b.chain_blob) HIP_TRY(copy_sync(out->blobs, b.chain_blob, (size_t)nsamples * bb, hipMemcpyDeviceToHost, st));
    }
    if (out->final_blob && b.blob) HIP_TRY(copy_sync(out->final_blob, b.blob, bb, hipMemcpyDeviceToHost, st));
    if (out->final_pos) HIP_TRY(copy_sync(out->final_pos, b.pos, rows, hipMemcpyDeviceToHost, st));
    if (out->final_logp) HIP_TRY(copy_sync(out->final_logp, b.logp, vec, hipMemcpyDeviceToHost, st));
    if (out->chain_sum && b.csum) HIP_TRY(copy_sync(out->chain_sum, b.csum, rows, hipMemcpyDeviceToHost, st));
    if (out->chain_sumsq && b.csumsq) HIP_TRY(copy_sync(out->chain_sumsq, b.csumsq, rows, hipMemcpyDeviceToHost, st));
    if (out->naccept || out->accept_ratio) {
        std::vector<uint32_t> na((size_t)nc);
        HIP_TRY(copy_sync(na.data(), b.naccept, (size_t)nc * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        const double denom = (double)(c->niter - c->nburnin);                                   // :127 (0/0 as in the reference)
        for (int64_t i = 0; i < nc; ++i) {
            if (out->naccept) out->naccept[i] = (int64_t)na[(size_t)i];
            if (out->accept_ratio) out->accept_ratio[i] = (double)na[(size_t)i] / denom;
        }
    }
    return KMC_OK;
}

// the host route's buffers on top of the shared ones, and the log-pdf function of a device density
kmc_status metropolis_host_setup(MetroRun& R, hipFunction_t* ulp)
{
    const kmc_metropolis_config* c = R.c;
    MetroBuffers& b = R.b;
    HIP_TRY(metro_alloc(&b.prop, R.rows));
    HIP_TRY(metro_alloc(&b.p1, R.vec));
    if (c->step && !R.sh.on) {
        HIP_TRY(metro_alloc(&b.step, (size_t)R.nd * sizeof(double)));
        HIP_TRY(copy_sync(b.step, c->step, (size_t)R.nd * sizeof(double), hipMemcpyHostToDevice, R.ss.st));
    }
    HIP_TRY(hipHostMalloc((void**)&b.h_rows, R.rows, hipHostMallocDefault));
    HIP_TRY(hipHostMalloc((void**)&b.h_prop, R.rows, hipHostMallocDefault));
    HIP_TRY(hipHostMalloc((void**)&b.h_p1, R.vec, hipHostMallocDefault));
    if (c->host_accepted) {
        HIP_TRY(hipMalloc((void**)&b.acc, (size_t)R.nc));
        HIP_TRY(hipHostMalloc((void**)&b.h_acc, (size_t)R.nc, hipHostMallocDefault));
    }
    if (c->density == KMC_USER_DENSITY) {
        const std::vector<char>* code = nullptr;
        KMC_TRY(compile_user_metropolis(static_cast<kmc_user_density*>(c->user_density), metropolis_nd(R.nd), &code, R.nd));
        KMC_TRY(shared_module(static_cast<kmc_user_density*>(c->user_density), code, &b.keep));
        HIP_TRY(hipModuleGetFunction(ulp, static_cast<hipModule_t>(b.keep.get()), "kmc_user_logpdf"));
    } else if (c->density != KMC_HOST_DENSITY && !logpdf_fn(c->density)) return fail(KMC_ERR_BAD_ARG, "unknown density id");
    return KMC_OK;
}

// The host route: `pdf` and / or `sample_ppdf` are caller's closures (src/samplers.jl:59-61).  One iteration of all chains per pass:
// proposals (the device's step, or host_propose on the current states), their log-pdfs
// (host_logpdf on the proposals, or the device density), then the accept test, counters and storage on the device.
kmc_status metropolis_host_route(MetroRun& R, const double* theta0)
{
    const kmc_metropolis_config* c = R.c;
    MetroBuffers& b = R.b;
    MetroShape& sh = R.sh;
    const hipStream_t st = R.ss.st;
    const int64_t nc = R.nc, nd = R.nd;
    const size_t rows = R.rows;
    const bool host_pdf = c->density == KMC_HOST_DENSITY;
    hipFunction_t ulp = nullptr;
    KMC_TRY(metropolis_host_setup(R, &ulp));
    // p0 = pdf(theta0) (:70); whatever comes out is carried, -Inf included, as in the reference
    if (host_pdf) {
        if (c->host_logpdf(theta0, nc, nd, b.h_p1, c->host_user) != 0) return fail(KMC_ERR_BAD_ARG, "the host log-pdf callback failed on the initial states");
        HIP_TRY(copy_sync(b.logp, b.h_p1, R.vec, hipMemcpyHostToDevice, st));
    } else {
        HIP_TRY(launch_logpdf(R, ulp, b.pos, b.logp, nullptr));
    }
    HIP_TRY(hipEventRecord(b.ev0, st));
    int64_t cnt = 0, slot = 0;
    for (int64_t it = 0; it < c->niter; ++it) {
        const int64_t n = it + 1 - c->nburnin;                                                   // :96
        if (sh.on && sh.boundary(it)) KMC_TRY(sh.tune(b.pos, nc, st));
        MetroHostArgs a{};
        a.pos = b.pos; a.logp = b.logp; a.naccept = b.naccept; a.prop = b.prop; a.p1 = b.p1;
        a.chain = b.chain; a.chain_logp = b.chain_logp; a.csum = b.csum; a.csumsq = b.csumsq; a.acc_out = b.acc;
        a.step = sh.on ? b.chol : b.step;                                                        // (the packed L in place of the scales)
        a.nchains = nc; a.it = it; a.n = n; a.ndim = (int32_t)nd;
        a.seed_lo = (uint32_t)c->seed; a.seed_hi = (uint32_t)(c->seed >> 32);
        if (n > 0 && ++cnt == c->nthin) {                                                        // :108, :112
            cnt = 0;
            if (slot < R.nsamples) { a.store = 1; a.slot = slot; }
            ++slot;
        }
        if (c->host_propose) {                                                                   // :98 theta1 = sample_ppdf(theta0)
            HIP_TRY(copy_sync(b.h_rows, b.pos, rows, hipMemcpyDeviceToHost, st));
            if (c->host_propose(b.h_rows, nc, nd, b.h_prop, c->host_user) != 0)
                return fail(KMC_ERR_BAD_ARG, "the host proposal callback failed in iteration " + std::to_string(it));
            HIP_TRY(copy_sync(b.prop, b.h_prop, rows, hipMemcpyHostToDevice, st));
        } else {
            if (sh.on) hipLaunchKernelGGL(metro_host_propose_mv, dim3(R.grid), dim3(256), 0, st, a);
            else hipLaunchKernelGGL(metro_host_propose, dim3(R.grid), dim3(256), 0, st, a);
            HIP_TRY(hipGetLastError());
        }
        if (host_pdf) {                                                                          // :99 p1 = pdf(theta1)
            if (!c->host_propose) HIP_TRY(copy_sync(b.h_prop, b.prop, rows, hipMemcpyDeviceToHost, st));
            if (c->host_logpdf(b.h_prop, nc, nd, b.h_p1, c->host_user) != 0)
                return fail(KMC_ERR_BAD_ARG, "the host log-pdf callback failed in iteration " + std::to_string(it));
            HIP_TRY(copy_sync(b.p1, b.h_p1, R.vec, hipMemcpyHostToDevice, st));
        } else {
            HIP_TRY(launch_logpdf(R, ulp, b.prop, b.p1, nullptr));
        }
        hipLaunchKernelGGL(metro_host_accept, dim3(R.grid), dim3(256), 0, st, a);
        HIP_TRY(hipGetLastError());
        if (c->host_accepted) {
            HIP_TRY(copy_sync(b.h_acc, b.acc, (size_t)nc, hipMemcpyDeviceToHost, st));
            if (c->host_accepted(b.h_acc, nc, 0, it, a.store, c->host_user) != 0)
                return fail(KMC_ERR_BAD_ARG, "the host accept callback failed in iteration " + std::to_string(it));
        }
    }
    HIP_TRY(hipEventRecord(b.ev1, st));
    return KMC_OK;
}

// The kernels of one run.  ND: the register geometry of the chains, 0 for chains kept dimension-major in memory; tabled: the
// few-chains route, whose chains stay in registers whatever the density and read the draws of table_steps iterations per launch.
struct MetroKernels {
    int ND = 0;
    bool tabled = false;
    MetropolisFn fn = nullptr;                    // a menu density's kernels ...
    MetropolisTabledFn tfn = nullptr;
    hipFunction_t ufn = nullptr, ulp = nullptr, utfn = nullptr;       // ... or a module's
    int64_t table_steps = 0;
};

kmc_status metropolis_select_kernels(MetroRun& R, MetroKernels* k)
{
    const kmc_metropolis_config* c = R.c;
    const int64_t nc = R.nc, nd = R.nd;
    kmc_user_density* ud = c->density == KMC_USER_DENSITY ? static_cast<kmc_user_density*>(c->user_density) : nullptr;
    k->ND = ud && ud->is_body ? 0 : metropolis_nd(nd);
    // Few chains (the reference's call is one): the draws of a stretch of iterations come from a wide kernel first, the chains
    // only read them (kmc_metropolis.hpp: metropolis_chains_tabled).  Up to a wave per CU (measured: x6.8 at one chain, x4 at
    // 4096, x2 at 16 384, x0.5 at 65 536 -- there the chains fill the chip themselves).  KMC_DEBUG=metro-table=0|1 forces it off / on.
    std::string opt;
    const bool have = debug_opt("metro-table", &opt);
    const bool off = have && opt == "0", on = have && opt == "1";
    // (up to 8 dimensions for up to 16 384 chains -- measured --; longer rows for the few chains that leave most of the chip idle)
    const int64_t nd_max = ud ? 32 : 8;           // (menu densities: instantiated up to 8 -- build time)
    const bool tabled = k->tabled = !off && R.nblob == 0 && ((nd <= 8 && nc <= 16384) || (nd <= nd_max && nc <= 1024) || (on && nd <= nd_max));
    if (ud) {
        const std::vector<char>* code = nullptr;
        // (the few-chains kernel is the same with L: the isotropic program serves it)
        KMC_TRY(compile_user_metropolis(ud, k->ND, &code, nd, tabled ? metropolis_nd(nd) : 0, R.sh.on && !tabled));
        KMC_TRY(shared_module(ud, code, &R.b.keep));
        const hipModule_t mod = static_cast<hipModule_t>(R.b.keep.get());
        HIP_TRY(hipModuleGetFunction(&k->ufn, mod, "kmc_user_metropolis"));
        HIP_TRY(hipModuleGetFunction(&k->ulp, mod, "kmc_user_logpdf"));
        if (tabled) HIP_TRY(hipModuleGetFunction(&k->utfn, mod, "kmc_user_metropolis_tabled"));
    } else {
        const int n = (int)std::min<int64_t>(nd, 1 << 20);        // the geometry follows ndim (registers <= 32)
        k->fn = with_density(c->density, MetropolisFn(nullptr),
                             [&](auto d) { return R.sh.on ? metropolis_mv_lookup<decltype(d)>(n) : metropolis_lookup<decltype(d)>(n); });
        if (!k->fn) return fail(KMC_ERR_BAD_ARG, "unknown density id");
    }
    if (!tabled) return KMC_OK;
    if (!ud) {
        k->tfn = with_density(c->density, MetropolisTabledFn(nullptr), [&](auto d) { return metropolis_tabled_lookup<decltype(d)>((int)nd); });
        if (!k->tfn) return fail(KMC_ERR_BAD_ARG, "unknown density id");
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k->tfn), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * kMetroTileBytes));
    }
    const int64_t per_step = nc * (nd + 1) * (int64_t)sizeof(double);
    k->table_steps = std::max<int64_t>(64, std::min<int64_t>(1 << 16, ((int64_t)128 << 20) / per_step));
    { const long ts = debug_opt_long("metro-table-steps", 0); if (ts > 0) k->table_steps = ts; }   // (tests: seams)
    k->table_steps = std::min<int64_t>(k->table_steps, std::max<int64_t>(c->niter, 1));
    HIP_TRY(metro_alloc(&R.b.draws, (size_t)(k->table_steps * per_step)));
    return KMC_OK;
}

// the device route's buffers on top of the shared ones: the scales and the blobs (the kernels chosen add the draw table and the
// dimension-major state)
kmc_status metropolis_device_setup(MetroRun& R)
{
    const kmc_metropolis_config* c = R.c;
    MetroBuffers& b = R.b;
    const hipStream_t st = R.ss.st;
    const std::vector<double> ones((size_t)R.nd, 1.0);       // (with L: a step of 1.0 for the few-chains kernel, whose table then holds L z)
    HIP_TRY(metro_alloc(&b.step, (size_t)R.nd * sizeof(double)));
    HIP_TRY(copy_sync(b.step, R.sh.on ? ones.data() : c->step, (size_t)R.nd * sizeof(double), hipMemcpyHostToDevice, st));
    if (R.nblob > 0) {
        const size_t bb = (size_t)R.nc * (size_t)R.nblob * sizeof(double);
        HIP_TRY(metro_alloc(&b.blob, bb));
        HIP_TRY(fill_sync(b.blob, 0, bb, st));
        if (R.want_blobs && R.nsamples > 0) {
            KMC_TRY(check_device_room((size_t)R.nsamples * bb, "the stored blobs"));
            HIP_TRY(metro_alloc(&b.chain_blob, (size_t)R.nsamples * bb));
        }
    }
    return KMC_OK;
}

// the iterations [it0, it1) of every chain in the device route: the draw table first (and L applied to it) on the few-chains route, then one kernel
// the kernel arguments of the iterations [it0, it1) of every chain, `step` aside
MetropolisArgs metropolis_stretch_args(const MetroRun& R, int64_t it0, int64_t it1)
{
    const kmc_metropolis_config* c = R.c;
    const MetroBuffers& b = R.b;
    MetropolisArgs a{};
    a.pos = b.pos; a.logp = b.logp; a.naccept = b.naccept;
    a.chain = b.chain; a.chain_logp = b.chain_logp; a.csum = b.csum; a.csumsq = b.csumsq;
    a.xt = b.xt; a.yt = b.yt; a.st1 = b.st1; a.st2 = b.st2;
    a.nchains = R.nc;
    a.it0 = it0; a.it1 = it1;
    a.nburnin = c->nburnin; a.nthin = c->nthin; a.nsamples = R.nsamples;
    const int64_t npos = it0 - c->nburnin;          // steps with n > 0 taken before it0
    a.cnt0 = npos > 0 ? npos % c->nthin : 0;
    a.slot0 = npos > 0 ? npos / c->nthin : 0;
    a.ndim = (int32_t)R.nd;
    a.seed_lo = (uint32_t)c->seed; a.seed_hi = (uint32_t)(c->seed >> 32);
    a.dp = R.dp;
    a.blob = b.blob; a.chain_blob = b.chain_blob;
    return a;
}

kmc_status metropolis_launch_stretch(const MetroRun& R, const MetroKernels& k, int64_t it0, int64_t it1)
{
    const MetroBuffers& b = R.b;
    const hipStream_t st = R.ss.st;
    const int64_t nc = R.nc;
    MetropolisArgs a = metropolis_stretch_args(R, it0, it1);
    a.step = (R.sh.on && !k.tabled) ? b.chol : b.step;
    if (!k.tabled) {
        if (k.ufn) HIP_TRY(launch_module(k.ufn, R.grid, 256u, st, a));
        else {
            hipLaunchKernelGGL(k.fn, dim3(R.grid), dim3(256), 0, st, a);
            HIP_TRY(hipGetLastError());
        }
        return KMC_OK;
    }
    const int64_t nit = it1 - it0;
    const unsigned fill_grid = (unsigned)((nit * nc + 255) / 256), chain_grid = (unsigned)((nc + 63) / 64);
    MetroDrawArgs da{};
    da.out = b.draws; da.nchains = nc; da.it0 = it0; da.nsteps = (int32_t)nit; da.ndim = (int32_t)R.nd;
    da.seed_lo = a.seed_lo; da.seed_hi = a.seed_hi;
    hipLaunchKernelGGL(metro_draw_fill, dim3(fill_grid), dim3(256), 0, st, da);
    if (R.sh.on) {                                   // the normals of the table become L z
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(metro_draw_shape, dim3(fill_grid), dim3(256), 0, st, MetroDrawMvArgs{da, b.chol});
    }
    HIP_TRY(hipGetLastError());
    if (k.utfn) {
        MetropolisTabledArgs ta{};
        ta.a = a; ta.draws = b.draws; ta.nsteps = (int32_t)nit;
        HIP_TRY(launch_module(k.utfn, chain_grid, 128u, st, ta, 2u * kMetroTileBytes));
    } else {
        hipLaunchKernelGGL(k.tfn, dim3(chain_grid), dim3(128), 2 * kMetroTileBytes, st, a, (const double*)b.draws, (int)nit);
        HIP_TRY(hipGetLastError());
    }
    return KMC_OK;
}

// The device route: the whole run inside kernels, one chain per lane; the loop walks the launches and the tuning boundaries.
kmc_status metropolis_device_route(MetroRun& R)
{
    const kmc_metropolis_config* c = R.c;
    MetroBuffers& b = R.b;
    MetroShape& sh = R.sh;
    const hipStream_t st = R.ss.st;
    MetroKernels k;
    KMC_TRY(metropolis_device_setup(R));            // (before the compile: the refusal for the stored blobs' room comes first)
    KMC_TRY(metropolis_select_kernels(R, &k));
    if (k.ND == 0) {                                // chains in memory: their state and moment sums dimension-major
        HIP_TRY(metro_alloc(&b.xt, R.rows));
        HIP_TRY(metro_alloc(&b.yt, R.rows));
        if (R.want_mom) {
            HIP_TRY(metro_alloc(&b.st1, R.rows));
            HIP_TRY(metro_alloc(&b.st2, R.rows));
            HIP_TRY(fill_sync(b.st1, 0, R.rows, st));
            HIP_TRY(fill_sync(b.st2, 0, R.rows, st));
        }
    }
    // p0 = pdf(theta0)  (:70); unlike emcee the reference carries whatever comes out, -Inf included  (and blob0, :70-72)
    HIP_TRY(launch_logpdf(R, k.ulp, b.pos, b.logp, b.blob));
    const bool in_memory = k.ND == 0 && !k.tabled;  // (the few-chains kernel keeps its chains in registers whatever the density)
    auto transpose = [&](const double* src, double* dst, bool to_dim_major) {
        const TransposeArgs ta{src, dst, R.nc, (int32_t)R.nd, to_dim_major ? 1 : 0};
        hipLaunchKernelGGL(metropolis_transpose, dim3(R.grid), dim3(256), 0, st, ta);
        return hipGetLastError();
    };
    if (in_memory) HIP_TRY(transpose(b.pos, b.xt, true));
    HIP_TRY(hipEventRecord(b.ev0, st));
    const int64_t kItersPerLaunch = k.tabled ? k.table_steps : (int64_t)1 << 16;   // chains are independent: launches only bound a kernel's run time (and the table)
    for (int64_t it0 = 0, it1 = 0; it0 < c->niter; it0 = it1) {
        it1 = std::min<int64_t>(c->niter, it0 + kItersPerLaunch);
        if (sh.on) {                                    // a tuning boundary always ends a launch; L is replaced before iteration b_r runs
            if (sh.boundary(it0)) {
                if (in_memory) HIP_TRY(transpose(b.xt, b.pos, false));     // (the covariance reads the states chain-major)
                KMC_TRY(sh.tune(b.pos, R.nc, st));
            }
            it1 = sh.next_boundary(it0, it1);
        }
        KMC_TRY(metropolis_launch_stretch(R, k, it0, it1));
    }
    HIP_TRY(hipEventRecord(b.ev1, st));
    if (in_memory) {
        HIP_TRY(transpose(b.xt, b.pos, false));
        if (R.want_mom) { HIP_TRY(transpose(b.st1, b.csum, false)); HIP_TRY(transpose(b.st2, b.csumsq, false)); }
    }
    return KMC_OK;
}

// The HMC route (hmc_nleap > 0; kmc_hmc.hpp): one chain per lane in registers, whatever the number of chains -- the draws of an iteration
// are amortised over the trajectory, so there is no few-chains table -- in launches of max(1, 65536 / nleap) iterations.
kmc_status metropolis_hmc_route(MetroRun& R)
{
    const kmc_metropolis_config* c = R.c;
    MetroBuffers& b = R.b;
    const hipStream_t st = R.ss.st;
    // (room for 32 step sizes, zeros beyond ndim: the kernels index them with compile-time offsets)
    std::vector<double> steps((size_t)kHmcMaxDim, 0.0);
    std::copy(c->step, c->step + R.nd, steps.begin());
    HIP_TRY(metro_alloc(&b.step, steps.size() * sizeof(double)));
    HIP_TRY(copy_sync(b.step, steps.data(), steps.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HmcFn fn = nullptr;
    hipFunction_t ufn = nullptr, ulp = nullptr;
    if (c->density == KMC_USER_DENSITY) {
        kmc_user_density* ud = static_cast<kmc_user_density*>(c->user_density);
        const std::vector<char>* code = nullptr;
        KMC_TRY(compile_user_hmc(ud, R.nd, &code));
        KMC_TRY(shared_module(ud, code, &b.keep));
        const hipModule_t mod = static_cast<hipModule_t>(b.keep.get());
        HIP_TRY(hipModuleGetFunction(&ufn, mod, "kmc_user_hmc"));
        HIP_TRY(hipModuleGetFunction(&ulp, mod, "kmc_user_logpdf"));
    } else {
        fn = hmc_lookup(c->density, (int)R.nd);
        if (!fn) return fail(KMC_ERR_BAD_ARG, "unknown density id");
    }
    HIP_TRY(launch_logpdf(R, ulp, b.pos, b.logp, nullptr));     // p0 = pdf(theta0)  (:70), carried whatever it is
    HIP_TRY(hipEventRecord(b.ev0, st));
    int64_t iters = std::max<int64_t>(1, 65536 / c->hmc_nleap);
    { const long n = debug_opt_long("metro-hmc-iters", 0); if (n > 0) iters = n; }     // (tests: the seams between launches)
    for (int64_t it0 = 0, it1 = 0; it0 < c->niter; it0 = it1) {
        it1 = std::min<int64_t>(c->niter, it0 + iters);
        HmcArgs h{};
        h.a = metropolis_stretch_args(R, it0, it1);
        h.a.step = b.step;
        h.nleap = c->hmc_nleap;
        h.jitter = c->hmc_jitter;
        if (ufn) HIP_TRY(launch_module(ufn, R.grid, 256u, st, h));
        else {
            hipLaunchKernelGGL(fn, dim3(R.grid), dim3(256), 0, st, h);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipEventRecord(b.ev1, st));
    return KMC_OK;
}

// kmc_metropolis_validate's refusals of the HMC step, each naming the value
kmc_status metropolis_validate_hmc(const kmc_metropolis_config* c)
{
    if (c->hmc_nleap < 0 || c->hmc_nleap > kHmcMaxLeap)
        return fail(KMC_ERR_BAD_ARG, "hmc_nleap = " + std::to_string(c->hmc_nleap) + ": must be in 0 .. " + std::to_string(kHmcMaxLeap) + " (0: no HMC step)");
    if (!std::isfinite(c->hmc_jitter) || c->hmc_jitter < 0.0 || c->hmc_jitter >= 1.0)
        return fail(KMC_ERR_BAD_ARG, "hmc_jitter = " + num(c->hmc_jitter, "%g") + ": must be finite and in [0, 1)");
    if (c->hmc_nleap == 0) {
        if (c->hmc_jitter != 0.0) return fail(KMC_ERR_BAD_ARG, "hmc_jitter = " + num(c->hmc_jitter, "%g") + " with hmc_nleap = 0: there is no HMC step to jitter");
        return KMC_OK;
    }
    const std::string with = "hmc_nleap = " + std::to_string(c->hmc_nleap) + " with ";
    if (c->chol) return fail(KMC_ERR_UNSUPPORTED, with + "chol: the HMC step has a diagonal metric, the step sizes in `step` (no dense mass matrix)");
    if (c->tune_rounds > 0) return fail(KMC_ERR_UNSUPPORTED, with + "tune_rounds = " + std::to_string(c->tune_rounds) + ": the step sizes of the HMC step are not tuned");
    if (c->host_propose) return fail(KMC_ERR_UNSUPPORTED, with + "host_propose: the HMC step is the proposal");
    if (c->density == KMC_HOST_DENSITY) return fail(KMC_ERR_UNSUPPORTED, with + "KMC_HOST_DENSITY: the HMC step needs the gradient on the device");
    if (c->ndim > kHmcMaxDim)
        return fail(KMC_ERR_UNSUPPORTED, with + "ndim = " + std::to_string(c->ndim) + ": the limit is " + std::to_string(kHmcMaxDim) + " (the chain lives in registers)");
    for (int64_t d = 0; c->step && d < c->ndim; ++d)
        if (!(std::isfinite(c->step[d]) && c->step[d] > 0.0))
            return fail(KMC_ERR_BAD_ARG, "step[" + std::to_string(d) + "] = " + num(c->step[d], "%g") + " with hmc_nleap > 0: every step size must be finite and > 0");
    if (c->density == KMC_USER_DENSITY && c->user_density) {
        kmc_user_density* ud = static_cast<kmc_user_density*>(c->user_density);
        if (!ud->is_body) return fail(KMC_ERR_UNSUPPORTED, with + "a term / pair density (kmc_user_density_create): the HMC step takes a body density with kmc_user_density_set_grad");
        if (ud->nblob > 0) return fail(KMC_ERR_UNSUPPORTED, with + "a density with blobs (nblob = " + std::to_string(ud->nblob) + "): the HMC step carries none");
        std::lock_guard<std::mutex> lock(ud->mu);
        if (ud->grad_body.empty()) return fail(KMC_ERR_BAD_ARG, with + "a runtime-compiled density without a gradient: give it one with kmc_user_density_set_grad");
    }
    return KMC_OK;
}

}  // namespace

KMC_EXPORT kmc_status kmc_metropolis_validate(const kmc_metropolis_config* c)
{
    if (!c) return fail(KMC_ERR_BAD_ARG, "null config");
    if (c->density == KMC_DATA_DENSITY) return fail(KMC_ERR_UNSUPPORTED, "kmc_metropolis_run: not with KMC_DATA_DENSITY (the emcee samplers only)");
    if (c->dtype != KMC_F64) return fail(KMC_ERR_UNSUPPORTED, "only KMC_F64 is implemented");
    if (c->nchains <= 0 || c->ndim <= 0 || c->nthin <= 0 || c->niter < 0 || c->nburnin < 0)
        return fail(KMC_ERR_BAD_ARG, "nchains, ndim, nthin must be positive; niter, nburnin non-negative");
    if (c->nchains > 0xffffffffll) return fail(KMC_ERR_BAD_ARG, "at most 2^32 - 1 chains (the chain index is one Philox counter word)");
    if (c->step && c->chol) return fail(KMC_ERR_BAD_ARG, "both step and chol are given: exactly one of them is the proposal");
    if (c->chol && c->host_propose) return fail(KMC_ERR_BAD_ARG, "chol with host_propose: the proposals come from the host, there is no L to apply");
    if (!c->step && !c->chol && !c->host_propose)
        return fail(KMC_ERR_BAD_ARG, "step (proposal scale per dimension) is NULL and there is no host_propose (neither step nor chol: exactly one of them is the proposal)");
    for (int64_t d = 0; c->step && d < c->ndim; ++d)
        if (!std::isfinite(c->step[d])) return fail(KMC_ERR_BAD_ARG, "step must be finite");
    if (c->tune_rounds < 0) return fail(KMC_ERR_BAD_ARG, "tune_rounds = " + std::to_string(c->tune_rounds) + ": must be >= 0");
    if (!std::isfinite(c->tune_scale) || c->tune_scale < 0.0)
        return fail(KMC_ERR_BAD_ARG, "tune_scale = " + std::to_string(c->tune_scale) + ": must be finite and >= 0 (0: 2.38 / sqrt(ndim))");
    if ((c->chol || c->tune_rounds > 0) && c->ndim > kMetroCholMaxDim)
        return fail(KMC_ERR_UNSUPPORTED, "ndim = " + std::to_string(c->ndim) + " with chol or tuning: the limit is " + std::to_string(kMetroCholMaxDim) +
                                             " (L is ndim^2 / 2 doubles read per step and lane, and nothing larger is tested)");
    for (int64_t i = 0; c->chol && i < c->ndim; ++i) {
        for (int64_t j = 0; j <= i; ++j)
            if (!std::isfinite(c->chol[i * c->ndim + j]))
                return fail(KMC_ERR_BAD_ARG, "chol[" + std::to_string(i) + "][" + std::to_string(j) + "] is not finite");
        if (!(c->chol[i * c->ndim + i] > 0.0))
            return fail(KMC_ERR_BAD_ARG, "chol[" + std::to_string(i) + "][" + std::to_string(i) + "] = " + std::to_string(c->chol[i * c->ndim + i]) +
                                             ": the diagonal of L must be > 0");
    }
    if (c->tune_rounds > 0) {
        if (c->host_propose) return fail(KMC_ERR_BAD_ARG, "tune_rounds = " + std::to_string(c->tune_rounds) + " with host_propose: there is no device proposal to tune");
        if (c->nchains <= c->ndim)
            return fail(KMC_ERR_BAD_ARG, "tune_rounds > 0 with nchains = " + std::to_string(c->nchains) + " <= ndim = " + std::to_string(c->ndim) +
                                             ": the covariance across chains would be singular");
        if (c->nburnin < (int64_t)c->tune_rounds + 1)
            return fail(KMC_ERR_BAD_ARG, "tune_rounds = " + std::to_string(c->tune_rounds) + " needs nburnin >= " + std::to_string(c->tune_rounds + 1) +
                                             " (nburnin = " + std::to_string(c->nburnin) + ")");
        for (int64_t d = 0; c->step && d < c->ndim; ++d)
            if (!(c->step[d] > 0.0))
                return fail(KMC_ERR_BAD_ARG, "step[" + std::to_string(d) + "] = " + std::to_string(c->step[d]) + " with tune_rounds > 0: diag(step) is the initial L, its diagonal must be > 0");
    }
    if (c->flags & ~(uint32_t)(KMC_STORE_CHAIN | KMC_STORE_LOGP | KMC_MOMENTS | KMC_CHAIN_BY_WALKER | KMC_STORE_BLOBS))
        return fail(KMC_ERR_BAD_ARG, "metropolis flags: KMC_STORE_CHAIN | KMC_STORE_LOGP | KMC_MOMENTS | KMC_CHAIN_BY_WALKER | KMC_STORE_BLOBS");
    {
        const int nb = c->density == KMC_USER_DENSITY && c->user_density ? static_cast<const kmc_user_density*>(c->user_density)->nblob : 0;
        if ((c->flags & KMC_STORE_BLOBS) && nb == 0)
            return fail(KMC_ERR_BAD_ARG, "KMC_STORE_BLOBS needs a body density with blobs (kmc_user_density_create_body_blob)");
        if (nb > 0 && c->host_propose)
            return fail(KMC_ERR_UNSUPPORTED, "a density with blobs runs in the in-kernel chains: not with host_propose (use a host log-pdf returning blobs)");
    }
    KMC_TRY(metropolis_validate_hmc(c));
    if (c->density == KMC_HOST_DENSITY) {
        if (!c->host_logpdf) return fail(KMC_ERR_BAD_ARG, "KMC_HOST_DENSITY needs kmc_metropolis_config.host_logpdf");
        return KMC_OK;
    }
    if (c->host_logpdf) return fail(KMC_ERR_BAD_ARG, "host_logpdf needs density == KMC_HOST_DENSITY");
    if (c->density == KMC_USER_DENSITY) {
        if (!c->user_density) return fail(KMC_ERR_BAD_ARG, "KMC_USER_DENSITY needs kmc_metropolis_config.user_density");
        return KMC_OK;
    }
    KMC_TRY(check_ndim(c->density, c->ndim));
    DensityParams dp;
    return metropolis_density_params(c, &dp);
}

KMC_EXPORT kmc_status kmc_metropolis_run(const kmc_metropolis_config* c, const double* theta0, kmc_metropolis_outputs* out)
{
    if (!theta0 || !out) return fail(KMC_ERR_BAD_ARG, "null argument");
    KMC_TRY(kmc_metropolis_validate(c));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return fail(KMC_ERR_NO_DEVICE, "no HIP device visible: the Metropolis path has no CPU fallback");
    }
    if (c->device < 0 || c->device >= ndev) return fail(KMC_ERR_BAD_ARG, "device ordinal out of range");
    HIP_TRY(hipSetDevice(c->device));
    out->nsamples = c->niter > c->nburnin ? (c->niter - c->nburnin) / c->nthin : 0;                 // :88
    out->device_ms = 0.0;
    MetroRun R;
    KMC_TRY(metropolis_density_params(c, &R.dp));
    KMC_TRY(metropolis_setup(c, theta0, out, &R));
    if (c->density == KMC_HOST_DENSITY || c->host_propose) KMC_TRY(metropolis_host_route(R, theta0));
    else if (c->hmc_nleap > 0) KMC_TRY(metropolis_hmc_route(R));
    else KMC_TRY(metropolis_device_route(R));
    return metropolis_read_out(R, out);
}

KMC_EXPORT kmc_status kmc_user_density_set_grad(kmc_user_density* ud, const char* grad_body)
{
    if (!ud || !grad_body) return fail(KMC_ERR_BAD_ARG, "null argument");
    if (!ud->is_body || ud->is_data || ud->nblob > 0)
        return fail(KMC_ERR_BAD_ARG, "kmc_user_density_set_grad: the density must be one made by kmc_user_density_create_body (a function body, no blobs)");
    if (grad_body[0] == '\0') return fail(KMC_ERR_BAD_ARG, "kmc_user_density_set_grad: the gradient body is empty");
    // Compiled once here (any ndim): the compiler's verdict comes now, not at the first run.  Only the verdict is kept: the check's
    // code object is never loaded (no module is keyed by its address), so it is dropped again.
    const std::string body = grad_body;
    static std::atomic<uint64_t> serial{0};
    const std::string key = "hmc-syntax:" + std::to_string(serial.fetch_add(1));      // (a key of this call's own: nobody else holds or erases it)
    const std::vector<char>* code = nullptr;
    const kmc_status st = compile_keyed(ud, key, hmc_rtc_module(), [&](std::string* text) {
        *text = "#include \"kmc_kernels.hpp\"\n#include \"kmc_hmc.hpp\"\n" + hmc_functor_source(ud, body) +
                "extern \"C\" __global__ void kmc_user_grad_check(const double* x, int n, const double* p, double* g) { UserB::grad(x, n, p, g); }\n";
        return KMC_OK;
    }, &code);
    std::lock_guard<std::mutex> lock(ud->mu);
    ud->code.erase(key);
    if (st != KMC_OK) return st;
    ud->grad_body = body;                                     // (the modules of a gradient are keyed by its text: compile_user_hmc)
    return KMC_OK;
}

KMC_EXPORT kmc_status kmc_grad_eval_host(const kmc_config* cfg, const double* pos_host, double* grad_host, int64_t nrows)
{
    if (!cfg || !pos_host || !grad_host || nrows < 0) return fail(KMC_ERR_BAD_ARG, "bad argument");
    if (cfg->ndim < 1 || cfg->ndim > kHmcMaxDim)
        return fail(KMC_ERR_UNSUPPORTED, "kmc_grad_eval_host: ndim = " + std::to_string(cfg->ndim) + ", must be in 1 .. " + std::to_string(kHmcMaxDim));
    kmc_user_density* ud = nullptr;
    if (cfg->density == KMC_USER_DENSITY) {
        ud = static_cast<kmc_user_density*>(cfg->user_density);
        if (!ud) return fail(KMC_ERR_BAD_ARG, "KMC_USER_DENSITY needs kmc_config.user_density");
        std::lock_guard<std::mutex> lock(ud->mu);
        if (ud->grad_body.empty()) return fail(KMC_ERR_BAD_ARG, "kmc_grad_eval_host: the density has no gradient (kmc_user_density_set_grad)");
    } else if (cfg->density == KMC_HOST_DENSITY || cfg->density == KMC_DATA_DENSITY) {
        return fail(KMC_ERR_UNSUPPORTED, "kmc_grad_eval_host: a menu density or a body density with kmc_user_density_set_grad");
    } else {
        KMC_TRY(check_ndim(cfg->density, cfg->ndim));
    }
    DensityParams dp;
    KMC_TRY(digest_params(*cfg, &dp));
    if (nrows == 0) return KMC_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return fail(KMC_ERR_NO_DEVICE, "no HIP device visible");
    }
    HIP_TRY(hipSetDevice(cfg->device));
    ScopedStream ss;
    HIP_TRY(ss.create());
    std::shared_ptr<void> keep;                                      // (the module's hold ends after the blocks are freed and the stream is gone)
    ScopedDeviceBlock dgrad, dpos;
    const size_t nb = (size_t)nrows * (size_t)cfg->ndim * sizeof(double);
    HIP_TRY(dpos.alloc(nb));
    HIP_TRY(dgrad.alloc(nb));
    HIP_TRY(copy_sync(dpos.p, pos_host, nb, hipMemcpyHostToDevice, ss.st));
    const GradArgs ga{dpos.as<double>(), dgrad.as<double>(), nrows, (int32_t)cfg->ndim, 0, dp};
    const unsigned grid = (unsigned)((nrows + 255) / 256);
    if (ud) {
        const std::vector<char>* code = nullptr;
        KMC_TRY(compile_user_hmc(ud, cfg->ndim, &code));
        KMC_TRY(shared_module(ud, code, &keep));
        hipFunction_t f = nullptr;
        HIP_TRY(hipModuleGetFunction(&f, static_cast<hipModule_t>(keep.get()), "kmc_user_grad"));
        HIP_TRY(launch_module(f, grid, 256u, ss.st, ga));
    } else {
        const GradFn f = grad_lookup(cfg->density, (int)cfg->ndim);
        if (!f) return fail(KMC_ERR_BAD_ARG, "unknown density id");
        hipLaunchKernelGGL(f, dim3(grid), dim3(256), 0, ss.st, ga);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(ss.st));
    HIP_TRY(copy_sync(grad_host, dgrad.p, nb, hipMemcpyDeviceToHost, ss.st));
    return KMC_OK;
}

KMC_EXPORT kmc_status kmc_cholesky_lower(const double* a, int n, double* L, int* bad)
{
    if (bad) *bad = -1;
    if (!a || !L) return fail(KMC_ERR_BAD_ARG, "null argument");
    if (n < 1) return fail(KMC_ERR_BAD_ARG, "kmc_cholesky_lower: n = " + std::to_string(n) + ", need n >= 1");
    const int b = cholesky_lower(a, n, L);
    if (b < 0) return KMC_OK;
    if (bad) *bad = b;
    return fail(KMC_ERR_BAD_ARG, "kmc_cholesky_lower: pivot " + std::to_string(b) + " is not finite and positive: the matrix is not positive definite");
}
