// kmc_data.hip -- data densities (KMC_DATA_DENSITY): the handle (two function bodies + the observations, copied at creation), their
// runtime-compiled kernels (kmc_data.hpp, ND / NCOLS as template constants), the planner that cuts one evaluation into workgroups,
// and the launches.  The generation loop that calls them between the host route's two passes is kmc_launch.hip.
#include <algorithm>
#include <sstream>

#include "kmc_sampler.hpp"
#include "kmc_data.hpp"

using namespace kmc;
using namespace kmc_host;

namespace kmc_host {

std::string data_functor_source(const kmc_user_density* ud)
{
    std::ostringstream src;
    src << "namespace {\nstruct UserData {\n"
        << "  __device__ static double term(const double* x, int n, const double* d, const double* p) { (void)x; (void)n; (void)d; (void)p;\n"
        << ud->data_term << "\n  }\n"
        << "  __device__ static double prior(const double* x, int n, const double* p) { (void)x; (void)n; (void)p;\n"
        << (ud->data_prior.empty() ? std::string("return 0.0;") : ud->data_prior) << "\n  }\n};\n}\n";
    return src.str();
}

}  // namespace kmc_host

namespace {
constexpr int kDataTPB = kmc_data::kWaves * 64;
// A cap on the partial kernel's grid: above it, more rounds per wave.  Not the residency: a 4-wave workgroup of ~86 VGPRs fits 5 per CU (5 waves
// per SIMD), 1 280 at once on 256 CUs, so a grid near the cap runs one full round and a partial tail round (S2: 1 568 = 1 280 + 288).
constexpr int64_t kTargetGroups = 2048;

kmc_status compile_data(kmc_user_density* ud, int64_t ndim, const std::vector<char>** out)
{
    static const RtcModule m{"data density", "kmc_data_density.hip", {"kmc_device.hpp", "kmc_data.hpp"}, rtc_options()};
    return compile_keyed(ud, "data:" + std::to_string(ndim), m, [&](std::string* text) {
        const std::string nd = std::to_string(ndim), nc = std::to_string(ud->ncols);
        std::ostringstream src;
        src << "#include \"kmc_data.hpp\"\n" << data_functor_source(ud)
            << "extern \"C\" __global__ __launch_bounds__(" << kDataTPB << ") void kmc_data_lane(const kmc_data::DataArgs a) { kmc_data::data_partial_lane_body<UserData, " << nd << ", " << nc << ">(a); }\n"
            << "extern \"C\" __global__ __launch_bounds__(" << kDataTPB << ") void kmc_data_obs(const kmc_data::DataArgs a) { kmc_data::data_partial_obs_body<UserData, " << nd << ", " << nc << ">(a); }\n"
            << "extern \"C\" __global__ __launch_bounds__(256) void kmc_data_fold(const kmc_data::DataArgs a) { kmc_data::data_fold_body<UserData, " << nd << ">(a); }\n"
            << "extern \"C\" __global__ __launch_bounds__(256) void kmc_data_fold_split(const kmc_data::DataArgs a) { kmc_data::data_fold_split_body<UserData, " << nd << ">(a); }\n";
        *text = src.str();
        return KMC_OK;
    }, out);
}
}  // namespace

namespace kmc_host {

// the observations on device `dev` (the current one): uploaded on first use, shared by everything over this density
kmc_status data_on_device(kmc_user_density* ud, int dev, std::shared_ptr<void>* keep)
{
    std::lock_guard<std::mutex> lock(ud->mu);
    auto& dslot = ud->data_dev[dev];
    if (!dslot) {
        const size_t bytes = ud->data.size() * sizeof(double);
        void* p = nullptr;
        KMC_TRY(check_device_room(bytes, "the data of a data density"));
        HIP_TRY(hipMalloc(&p, bytes));
        ScopedStream ss;
        hipError_t e = ss.create();
        if (e == hipSuccess) e = copy_sync(p, ud->data.data(), bytes, hipMemcpyHostToDevice, ss.st);
        if (e != hipSuccess) { (void)hipFree(p); HIP_TRY(e); }
        dslot = std::shared_ptr<void>(p, [dev](void* q) { int cur = 0; (void)hipGetDevice(&cur); (void)hipSetDevice(dev); (void)hipFree(q); (void)hipSetDevice(cur); });
    }
    *keep = dslot;
    return KMC_OK;
}

kmc_status load_data(kmc_user_density* ud, int64_t ndim, DataKernels* dk)
{
    const std::vector<char>* code = nullptr;
    KMC_TRY(compile_data(ud, ndim, &code));
    KMC_TRY(shared_module(ud, code, &dk->keep));
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    KMC_TRY(data_on_device(ud, dev, &dk->keep_data));
    dk->data = static_cast<const double*>(dk->keep_data.get());
    hipModule_t mod = static_cast<hipModule_t>(dk->keep.get());
    HIP_TRY(hipModuleGetFunction(&dk->lane, mod, "kmc_data_lane"));
    HIP_TRY(hipModuleGetFunction(&dk->obs, mod, "kmc_data_obs"));
    HIP_TRY(hipModuleGetFunction(&dk->fold, mod, "kmc_data_fold"));
    HIP_TRY(hipModuleGetFunction(&dk->fold_split, mod, "kmc_data_fold_split"));
    return KMC_OK;
}

// Which mapping, and how many observations a workgroup covers.  A proposal per lane wants at least a few waves of proposals; with
// fewer (the reference's 100 walkers: 50 per half-step) a wave per proposal and a lane per observation keeps the chip busy instead.
// Then the fewest rounds per wave that keep the workgroups at or under kTargetGroups (and the blocks at or under 4096: the scratch
// bound, nblocks x nprop doubles).  KMC_DEBUG=data-map=lane|obs forces the mapping.
DataPlan data_plan(const kmc_user_density* ud, int64_t nprop)
{
    DataPlan p;
    p.obs = nprop < 512;
    std::string forced;
    if (debug_opt("data-map", &forced)) { if (forced == "lane") p.obs = false; else if (forced == "obs") p.obs = true; }
    const int64_t chunk = p.obs ? 64 : kmc_data::kChunk;
    const int64_t groups = p.obs ? nprop : (nprop + 63) / 64;
    auto blocks = [&](int64_t r) { const int64_t b = (int64_t)kmc_data::kWaves * chunk * r; return (ud->ndata + b - 1) / b; };
    int64_t r = 1;
    const int64_t rmax = (int64_t)1 << (kmc_data::kLevels - 1);
    while (r < rmax && (blocks(r) > 4096 || (groups * blocks(r) > kTargetGroups && blocks(r) > 1))) r *= 2;
    p.rounds = (int32_t)r;
    p.nblocks = (int32_t)blocks(r);
    return p;
}

hipError_t launch_data_eval(const DataKernels& dk, const kmc_user_density* ud, const DataPlan& p, const double* prop, int64_t nprop, int32_t ld,
                            const double* params, double* part, size_t part_doubles, double* out, hipStream_t st, bool split)
{
    if (nprop <= 0) return hipSuccess;
    if ((size_t)p.nblocks * (size_t)nprop > part_doubles) return hipErrorInvalidValue;     // (never launched past the scratch buffer)
    kmc_data::DataArgs a{};
    a.prop = prop; a.data = dk.data; a.part = part; a.out = out;
    a.nprop = nprop; a.ndata = ud->ndata; a.ld = ld;
    a.rounds = p.rounds; a.nblocks = p.nblocks;
    for (int i = 0; i < 6; ++i) a.p[i] = params[i];
    const unsigned gx = p.obs ? (unsigned)nprop : (unsigned)((nprop + 63) / 64);
    {                                                                          // (a 2-D grid: x = proposals, y = blocks of observations)
        kmc_data::DataArgs copy = a;
        size_t size = sizeof(copy);
        void* extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &copy, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
        const hipError_t e = hipModuleLaunchKernel(p.obs ? dk.obs : dk.lane, gx, (unsigned)p.nblocks, 1, kDataTPB, 1, 1, 0, st, nullptr, extra);
        if (e != hipSuccess) return e;
    }
    return launch_module(split ? dk.fold_split : dk.fold, (unsigned)((nprop + 255) / 256), 256u, st, a);
}

}  // namespace kmc_host

KMC_EXPORT kmc_status kmc_data_density_create(const char* term_body, const char* prior_body, const double* data, int64_t ndata, int32_t ncols,
                                              kmc_user_density** out)
{
    if (!term_body || !out) return fail(KMC_ERR_BAD_ARG, "null argument");
    *out = nullptr;
    if (!data) return fail(KMC_ERR_BAD_ARG, "data density: data is NULL");
    if (ndata < 1 || ndata > kDataMaxRows) return fail(KMC_ERR_BAD_ARG, "data density: ndata must be in 1 .. 2^30");
    if (ncols < 1 || ncols > kDataMaxCols) return fail(KMC_ERR_BAD_ARG, "data density: ncols must be in 1 .. " + std::to_string(kDataMaxCols));
    kmc_user_density* ud = new kmc_user_density();
    ud->is_data = true;
    ud->data_term = term_body;
    if (prior_body && prior_body[0]) ud->data_prior = prior_body;
    ud->ndata = ndata;
    ud->ncols = ncols;
    ud->data.assign(data, data + (size_t)ndata * (size_t)ncols);               // a copy: the caller's array may change afterwards
    const std::vector<char>* code = nullptr;
    const kmc_status st = compile_data(ud, 4, &code);                          // syntax check now (placeholder ndim)
    if (st != KMC_OK) { delete ud; return st; }
    *out = ud;
    return KMC_OK;
}
