// kmc_sampler.hip -- the sampler's lifecycle behind the C ABI (include/kissmcmc_hip.h): creation / destruction of the device state of
// the `emcee` front-end (src/samplers.jl:188-216) and the small getters.  Which configurations it takes is kmc_validate.hip; the
// description of how a sampler executes is kmc_describe.hip.  Kernel tables and the launch plan per ndim are kmc_plan.hip.
// kmc_sampler_create runs named steps: init_shape; the route (setup_islands, setup_user_density / setup_menu_resident, setup_generation,
// setup_launch_geometry); the device state (alloc_*).  Every execution route of the library is decided there and nowhere else.
// The generation loop (src/samplers.jl:232-293) is kmc_launch.hip; state in and out is kmc_state.hip; copies and the chain
// ring are kmc_copy.hip; runtime-compiled densities kmc_rtc.hip; multi-GPU wiring kmc_p2p.hip; diagnostics kmc_diag.hip.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <random>

#include "kmc_sampler.hpp"

using namespace kmc;
using namespace kmc_host;

thread_local std::string kmc_host::g_err;

KMC_EXPORT int kmc_version(void) { return KMC_VERSION; }

KMC_EXPORT int kmc_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

KMC_EXPORT const char* kmc_last_error(void) { return g_err.c_str(); }

KMC_EXPORT double kmc_g_pdf(double z, double a)   // src/samplers.jl:224
{
    return (1.0 / a <= z && z <= a) ? 1.0 / std::sqrt(z) * 1.0 / (2.0 * (std::sqrt(a) - std::sqrt(1.0 / a))) : 0.0;
}

KMC_EXPORT double kmc_cdf_g_inv(double u, double a)   // src/samplers.jl:227
{
    const double t = std::fma(u, std::sqrt(a) - std::sqrt(1.0 / a), std::sqrt(1.0 / a));
    return t * t;
}

// hipMalloc does not clear memory.  KMC_DEBUG=poison (diagnostics): every allocation of a sampler starts as 0xFF bytes (NaN doubles,
// 4 294 967 295 counters), so that anything the code forgot to initialise shows up in the tests instead of depending on what the
// allocator happened to return.
// ... and is followed by a 4 KiB guard of 0xA5 that kmc_sampler_destroy checks: a kernel that writes past the end of one of
// its buffers aborts the process there, with the size of the allocation (the tests then fail loudly).
// Every buffer handed out is recorded in kmc_sampler::allocs: kmc_sampler_destroy frees that list, so a new buffer needs no line there.
template <class T>
hipError_t dev_alloc(kmc_sampler* s, T** p, size_t bytes)
{
    static const bool poison = debug_opt("poison");
    const bool guarded = poison && bytes != 0;
    // (IPC-exported buffers stay plain allocations: a peer maps them by their base address)
    hipError_t e = guarded                       ? hipMalloc(reinterpret_cast<void**>(p), bytes + kGuardBytes)
                   : (s->cfg.flags & KMC_P2P)    ? hipMalloc(reinterpret_cast<void**>(p), bytes)
                                                 : cache_alloc(reinterpret_cast<void**>(p), bytes);
    if (e != hipSuccess || !*p) return e;
    s->allocs.push_back({*p, bytes, guarded});
    if (guarded) {
        e = hipMemsetAsync(*p, 0xFF, bytes, s->stream);
        if (e == hipSuccess) e = hipMemsetAsync(reinterpret_cast<char*>(*p) + bytes, 0xA5, kGuardBytes, s->stream);
    }
    return e;
}
// a buffer of the sampler's goes on its own (kmc_sampler_bind_positions): out of the record, back to the allocator
static void dev_free(kmc_sampler* s, void* p)
{
    auto it = std::find_if(s->allocs.begin(), s->allocs.end(), [p](const DevAlloc& a) { return a.p == p; });
    if (it != s->allocs.end()) s->allocs.erase(it);
    cache_free(p);
}

namespace {
// A body that kmc_user_density_create_body recognised as a sum over elements (kmc_rtc.hip: recognise_separable -- a TEXT matcher) is
// run in its generated per-element form only after that form has been evaluated next to the body itself: 256 test rows of the
// sampler's ndim (normal / half-normal / uniform entries on several scales, so that densities on the line, the half-line and the
// unit box all see admissible points), both through the sequential log-pdf kernels of the module just loaded.  They must agree on
// every row (both non-finite alike, or within 1e-9 relative) and at least 8 rows must carry a finite value; otherwise the density's
// density loses its routing.  Once per (ndim, parameter values) of a density -- what agrees at one row length and one parameter set says nothing
// about another: a case where the forms DISAGREE refutes the recogniser (`sep` cleared for every later sampler, describe() says why);
// a case where too few rows are finite shows nothing: THIS sampler runs the body as written (kmc_sampler::sep_off), the density keeps its routing.
// KMC_DEBUG=sum-form-check=fail / =blind force the two negative outcomes (tests).
uint64_t sum_form_case_digest(const kmc_sampler* s)
{
    uint64_t h = 0xcbf29ce484222325ull;
    const unsigned char* b = reinterpret_cast<const unsigned char*>(s->dp.p);
    for (size_t i = 0; i < sizeof(s->dp.p); ++i) { h ^= b[i]; h *= 0x100000001b3ull; }
    return h;
}
// 0: not checked yet for this sampler's (ndim, parameters); 1: agreed; 3: blind
int sum_form_case(kmc_sampler* s)
{
    kmc_user_density* ud = s->user;
    std::lock_guard<std::mutex> lock(ud->mu);
    auto it = ud->sep_case.find({s->cfg.ndim, sum_form_case_digest(s)});
    return it == ud->sep_case.end() ? 0 : it->second;
}
kmc_status check_sum_form(kmc_sampler* s)
{
    kmc_user_density* ud = s->user;
    constexpr int kRows = 256, kFamilies = 8;
    const int64_t nd = s->cfg.ndim, ld = s->ld;
    std::vector<double> rows((size_t)kRows * (size_t)ld, 0.0);
    std::mt19937_64 gen(0x6b6d632d73756d21ull);
    std::normal_distribution<double> normal(0.0, 1.0);
    std::uniform_real_distribution<double> unit(0.0, 1.0);
    for (int r = 0; r < kRows; ++r) {
        const int fam = r % kFamilies;
        for (int64_t d = 0; d < nd; ++d) {
            const double z = normal(gen), u = unit(gen);
            double v = z;
            switch (fam) {
                case 1: v = 0.01 * z; break;
                case 2: v = 10.0 * z; break;
                case 3: v = std::fabs(z); break;
                case 4: v = 0.01 * std::fabs(z); break;
                case 5: v = 10.0 * std::fabs(z); break;
                case 6: v = u; break;
                case 7: v = -std::fabs(z); break;
                default: break;
            }
            rows[(size_t)r * (size_t)ld + (size_t)d] = v;
        }
    }
    // (a stream of its own and copy_sync: nothing here may touch the legacy stream -- another thread may be capturing a graph, kmc_host.hpp)
    double *d_rows = nullptr, *d_out = nullptr;
    std::vector<double> out(2 * kRows);
    ScopedStream ss;
    hipError_t e = ss.create();
    if (e == hipSuccess) e = hipMalloc((void**)&d_rows, rows.size() * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&d_out, out.size() * sizeof(double));
    if (e == hipSuccess) e = copy_sync(d_rows, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice, ss.st);
    if (e == hipSuccess) {
        const LogpdfArgs la{d_rows, d_out, (int64_t)kRows, (int32_t)nd, (int32_t)ld, s->dp, nullptr};
        e = launch_module(s->uk.logpdf, 1u, 256u, ss.st, la);
    }
    if (e == hipSuccess) {
        const LogpdfArgs lb{d_rows, d_out + kRows, (int64_t)kRows, (int32_t)nd, (int32_t)ld, s->dp, nullptr};
        e = launch_module(s->uk.logpdf_sep, 1u, 256u, ss.st, lb);
    }
    if (e == hipSuccess) e = copy_sync(out.data(), d_out, out.size() * sizeof(double), hipMemcpyDeviceToHost, ss.st);
    if (ss.st) (void)hipStreamSynchronize(ss.st);
    if (d_rows) (void)hipFree(d_rows);
    if (d_out) (void)hipFree(d_out);
    HIP_TRY(e);
    int informative = 0, differ = 0, first = -1;
    for (int r = 0; r < kRows; ++r) {
        const double a = out[r], b = out[kRows + r];
        const bool fa = std::isfinite(a), fb = std::isfinite(b);
        bool same;
        if (!fa || !fb) same = (fa == fb) && (std::isnan(a) == std::isnan(b)) && (std::isnan(a) || (a < 0) == (b < 0));
        else { same = std::fabs(a - b) <= 1e-9 * std::fmax(1.0, std::fmax(std::fabs(a), std::fabs(b))); ++informative; }
        if (!same) { if (first < 0) first = r; ++differ; }
    }
    std::string forced;
    if (debug_opt("sum-form-check", &forced)) {
        if (forced == "fail") { differ = 1; first = 0; }
        if (forced == "blind") { differ = 0; informative = 0; }
    }
    std::lock_guard<std::mutex> lock(ud->mu);
    const std::pair<int64_t, uint64_t> key{s->cfg.ndim, sum_form_case_digest(s)};
    if (differ == 0 && informative >= 8) { ud->sep_case[key] = 1; return KMC_OK; }
    char why[256];
    if (differ) {
        std::snprintf(why, sizeof(why), "its per-element form disagrees with the body on %d of %d test rows (row %d: body %.17g, per-element form %.17g)",
                      differ, kRows, first, out[first], out[kRows + first]);
        ud->sep_note = why;
        ud->sep = false;                         // refuted: no later sampler routes this body
    } else {
        std::snprintf(why, sizeof(why), "only %d of %d test rows had a finite log-density at ndim %lld with these parameters: its per-element form could not be checked",
                      informative, kRows, (long long)s->cfg.ndim);
        ud->sep_case[key] = 3;                   // nothing shown HERE: this sampler runs the body as written; other cases are checked on their own
        s->sep_off = true;
        s->sep_off_note = why;
    }
    if (differ)
        std::fprintf(stderr, "kissmcmc_hip: a function body was recognised as a sum over elements, but %s -- it is evaluated per walker, as written "
                             "(please report the body; KMC_DEBUG=no-body-routing skips the attempt)\n", why);
    return KMC_OK;
}
}  // namespace

namespace {
// One launch per generation (kmc_generation.hpp) -- the dependent-launch boundary, which is most of a half-step for small states, is paid
// once per generation instead of twice.  0: no; 1: one walker per lane (ndim <= 8); 2: rows lane-striped like the vector kernels (longer
// rows; lane-striped densities).  Measured against the two-launch kernels (profiles/r04_generation_map.txt): short rows 1.3-1.9 x ahead up
// to 32 768 walkers, 1.25-1.4 x at 65 536 walkers of one or two doubles, behind beyond that; longer rows 1.15-1.55 x ahead while the state
// stays within ~2.3 MiB, 1.25-1.4 x at 4 MiB (8 192 x 64, 32 768 x 16, 16 384 x 32), 1.06-1.3 x between 4 and 8 MiB (C3 1.17 x, 16 384 x 48 1.33, 24 576 x 32 1.18,
// 32 768 x 32 1.06, 49 152 x 16 1.10) except with 65 536 walkers (x 16: 0.94), mixed at 10 MiB (0.91-1.07) and behind from 12 MiB on -- the kernel moves 1.5 x the
// walkers and reads 2.5 x the rows (profiles/r05_generation_mid.txt, profiles/r05_generation_limit.txt: measured again after the row masks went and the stores became
// write-through; C3 was 0.95 x before both).
// KMC_DEBUG=fused=0 / =1: never / wherever a kernel exists.  (Resident and island mode are decided by the caller.)
int generation_wanted(const kmc_sampler* s)
{
    const kmc_config& c = s->cfg;
    if (c.density == KMC_HOST_DENSITY || c.density == KMC_DATA_DENSITY || s->f32 || s->nblob != 0 || c.shard_count != 1 || c.deal_count != 0 ||
        two_launch_only(c) ||                                                                         // (DE, snooker, mixtures, tempered ladders: the two-launch kernels only)
        (c.flags & (KMC_P2P | KMC_NO_GRAPH | KMC_ISLANDS)) || std::getenv("KMC_PLAN") != nullptr)      // (KMC_PLAN: a geometry of the two-launch kernels was asked for)
        return 0;
    // lane-striped forms need a lane-striped density (menu, term / pair, a body recognised as a sum) and the vector kernels' plan
    const bool striped = s->plan.vec && !(s->user && s->user->is_body && !(s->user->sep && !s->sep_off));
    // ndim <= 8: one walker per lane -- or, from 5 dimensions on, the row over a quad (generation_group<4, 1>: the quad shares the draws' four
    // logarithms; measured 1.65 against 1.95 us per half-step at 4 096 x 8, 1.65 against 1.76 at 4 096 x 6, behind at 16 384 x 6)
    int kind = c.ndim <= 8 ? 1 : 2;
    if (kind == 2 && !striped) return 0;
    std::string forced;
    const bool have = debug_opt("fused", &forced);
    if (have && forced == "0") return 0;
    if (kind == 1 && c.ndim >= 5 && striped && forced != "lane" && (have || c.nwalkers <= (s->ld == 8 ? 49152 : 8192))) kind = 3;     // (49 152 x 8: 1.12 x the two launches; 65 536 x 8: 1.01)
    if (have) return kind;                                   // (=1 / =lane: wherever a kernel exists; =lane keeps short rows one walker per lane)
    if (kind == 3) return 3;
    if (kind == 1) return ((c.nwalkers <= 49152 && c.nwalkers * s->ld <= 196608) || (c.nwalkers <= 65536 && s->ld <= 2)) ? 1 : 0;       // (49 152 x 4: 1.09 x; 65 536 x 3 / x 4: 1.03 / 0.99)
    return c.nwalkers * s->ld <= (c.nwalkers <= 49152 ? 1048576 : 524288) ? 2 : 0;     // (8 MiB of state up to 49 152 walkers, 4 MiB beyond)
}
}  // namespace

// ---- kmc_sampler_create: the steps, in the order they run ----------------------------------------------------------------------------
namespace {
// (a step that fails just returns: the sampler under construction is held by this and goes through kmc_sampler_destroy)
struct SamplerDeleter { void operator()(kmc_sampler* s) const { kmc_sampler_destroy(s); } };

// the copied configuration and what follows from it alone: ladder, shard and half sizes, row stride, sample count, parameter digest, plan
kmc_status init_shape(kmc_sampler* s, const kmc_config& cfg)
{
    s->cfg = cfg;
    s->user_seed = cfg.seed;
    s->temper = tempered(cfg);
    s->ntemps = s->temper ? cfg.ntemps : 1;
    if (s->temper) s->betas.assign(cfg.betas, cfg.betas + cfg.ntemps);          // (the caller's array is copied here)
    s->cfg.betas = s->temper ? s->betas.data() : nullptr;
    s->temper_like = s->temper && cfg.temper_mode == KMC_TEMPER_LIKELIHOOD;
    s->adapt = s->temper && cfg.adapt != 0;
    if (s->adapt && s->cfg.adapt_until == 0) s->cfg.adapt_until = cfg.nburnin;
    for (int j = 1; s->temper && j + 1 < s->ntemps; ++j)                          // (state from here on: never derived from the betas again)
        s->S0.push_back(std::log(1.0 / s->betas[(size_t)j] - 1.0 / s->betas[(size_t)j - 1]));
    if (cfg.deal_count > 0) s->cfg.seed = deal_seed(cfg.seed, cfg.deal_rank);    // this sub-ensemble's Philox key
    if (s->cfg.shard_count <= 0) s->cfg.shard_count = 1;
    s->h = cfg.nwalkers / 2;
    s->h_loc = s->h / s->cfg.shard_count;
    s->active_begin = s->h_loc * s->cfg.shard_rank;
    s->nlocal = 2 * s->h_loc;
    s->nsamples = cfg.ngenerations > cfg.nburnin ? (cfg.ngenerations - cfg.nburnin) / cfg.nthin : 0;   // :234
    s->ld = cfg.ndim + (cfg.ndim & 1);      // whole two-element chunks: 16-byte aligned double rows, 8-byte aligned float rows
    s->f32 = cfg.dtype == KMC_F32;
    s->p2p = (cfg.flags & KMC_P2P) != 0;
    s->nrows = s->p2p ? s->nlocal : cfg.nwalkers;
    KMC_TRY(digest_params(cfg, &s->dp));
    s->plan = make_plan(s->cfg, s->h_loc);
    return KMC_OK;
}

// ---- resident mode: the whole ensemble in one workgroup's LDS.  One decision for the menu and the runtime-compiled densities ----
// 16-byte chunks each of a walker's two lanes holds in the pair kernels (resident and island): the smallest power of two K with 2 K >= ld / 2
int row_chunks_K(int64_t ld)
{
    int K = 1;
    while (2 * K < ld / 2) K *= 2;
    return K;
}
// LDS of n walkers, a pair of lanes per walker: two lanes x 2 (K + 1) doubles of row, and the log-pdf
size_t pair_lds_bytes(int64_t n, int K) { return ((size_t)n * (size_t)(4 * (K + 1)) + (size_t)n) * sizeof(double); }
// ... one or two walkers per thread: rows of nd | 1 doubles, and the log-pdf
size_t lane_lds_bytes(int64_t n, int64_t nd) { return ((size_t)n * (size_t)((nd | 1) + 1)) * sizeof(double); }

struct ResidentChoice {
    enum Kind { None, Pair, Lane, Lane2 };   // not resident; a pair of lanes per walker; one walker per thread; two walkers per thread
    Kind kind = None;
    int K = 0;             // row_chunks_K(ld), whatever the kind: the moment sums are sized by it
    int tpb = 256;         // threads of the one workgroup
    size_t lds = 0;        // bytes its rows take (the callers round up: the moment reduction reuses the buffer)
};
// what differs between the callers
struct ResidentFacts {
    bool body;             // a function body: one walker per thread at any row length (kmc_islands.hpp: resident_lane_body), its registers hold the proposal
    bool blobs;
    bool f32;              // float rows: the one-walker-per-thread kernels only -- their LDS rows are double either way
    bool has_pair;         // the density has a pair kernel for these rows
    int64_t pair_max;      // ... for ensembles up to this size
};

// whatever the density: what keeps an ensemble out of resident mode
bool resident_possible(const kmc_config& c)
{
    return c.ndim <= 32 && c.shard_count == 1 && !(c.flags & (KMC_P2P | KMC_NO_GRAPH | KMC_ISLANDS)) && !two_launch_only(c) && !debug_opt("no-resident");
}

ResidentChoice choose_resident(const kmc_config& c, int64_t ld, const ResidentFacts& f)
{
    ResidentChoice r;
    const int64_t n = c.nwalkers;
    if (n > 1024) {                  // 1026 .. 2048 walkers: two walkers per thread (kmc_islands.hpp: resident_lane2_body; short double rows, no blobs), as LDS allows
        if (n > 2048 || f.f32 || c.ndim > 8 || f.blobs || !resident_lane_wanted(c.ndim)) return r;
        r.kind = ResidentChoice::Lane2;
        r.tpb = (int)((n / 2 + 63) / 64 * 64);
        r.lds = lane_lds_bytes(n, lane_nd(c.ndim));
    } else if (f.body || resident_lane_wanted(c.ndim)) {      // short rows: one walker per thread (measured faster up to ndim 8)
        r.kind = ResidentChoice::Lane;
        r.tpb = (int)((n + 63) / 64 * 64);
        r.lds = lane_lds_bytes(n, lane_nd(c.ndim));
    } else if (f.has_pair && n <= f.pair_max) {
        r.kind = ResidentChoice::Pair;
        r.tpb = n <= 256 ? 256 : (n <= 512 ? 512 : 1024);
        r.lds = pair_lds_bytes(n, row_chunks_K(ld));
    }
    if (r.lds > kResidentLdsMax) return ResidentChoice{};
    if (r.kind != ResidentChoice::None) r.K = row_chunks_K(ld);
    return r;
}

void set_resident(kmc_sampler* s, const ResidentChoice& r, size_t lds)
{
    s->resident = true;
    s->island_K = r.K;
    s->nislands = 1;
    s->island_lds = lds;
    s->resident_lane = r.kind != ResidentChoice::Pair;
    s->resident_lane2 = r.kind == ResidentChoice::Lane2;
    s->resident_tpb = r.tpb;
}

// a menu density: the kernel comes from the tables; one that is missing, or that the runtime will not give the LDS, leaves the
// ensemble to the launches per generation
void setup_menu_resident(kmc_sampler* s)
{
    const kmc_config& c = s->cfg;
    if (!resident_possible(c)) return;
    const ResidentChoice r = choose_resident(c, s->ld, ResidentFacts{false, false, s->f32, !s->f32, 1024});
    if (r.kind == ResidentChoice::None) return;
    const ResidentFn rf = with_density(c.density, ResidentFn(nullptr), [&](auto d) {
        using D = decltype(d);
        return r.kind == ResidentChoice::Lane2 ? resident_lane2_lookup<D>((int)c.ndim)
               : r.kind == ResidentChoice::Lane ? resident_lane_lookup<D>((int)c.ndim, s->f32)
                                                : resident_lookup<D>(r.tpb, r.K, 4 * r.K != c.ndim);
    });
    if (!rf) return;
    const size_t lds = std::max<size_t>(r.lds, 8192);           // the moment reduction reuses the buffer
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(rf), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    set_resident(s, r, lds);
    s->resident_kernel = rf;
}

// ---- island mode (KMC_ISLANDS): every island field; a menu density's kernel (a runtime-compiled one's comes with its module) ----
kmc_status setup_islands(kmc_sampler* s)
{
    const kmc_config& c = s->cfg;
    s->islands = true;
    s->island_gens = c.island_gens > 0 ? c.island_gens : 32;
    s->island_size = c.island_size > 0 ? c.island_size : kIslandSizeDefault;
    s->nislands = c.nwalkers / s->island_size;
    s->island_K = row_chunks_K(s->ld);                   // 16-byte chunks per row, 2 lanes per walker
    s->island_ragged = 4 * s->island_K != c.ndim;
    s->island_lds = std::max<size_t>(pair_lds_bytes(s->island_size, s->island_K), 4096);          // the moment reduction reuses the buffer
    if (c.density == KMC_USER_DENSITY) return KMC_OK;
    s->island_kernel = with_density(c.density, IslandFn(nullptr),
                                    [&](auto d) { return island_lookup<decltype(d)>((int)s->island_size, s->island_K, s->island_ragged); });
    if (!s->island_kernel) return fail(KMC_ERR_UNSUPPORTED, "no island kernel for this density / ndim");
    const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(s->island_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)s->island_lds);
    if (ea != hipSuccess) { (void)hipGetLastError(); return fail(KMC_ERR_HIP, std::string("hipFuncSetAttribute: ") + hipGetErrorString(ea)); }
    return KMC_OK;
}

// ---- a runtime-compiled density: what load_user (kmc_rtc.hip) is asked to compile, as a UserModuleSpec ----
// The vector geometry is the plan's; the resident kernel is the ResidentChoice's kind with what that kind is built from -- Pair: the
// row chunks K and whether 4 K != ndim; Lane: a term / pair density's short-row length lane_nd(ndim), a body density's workgroup size
// bound (a body of 32 dimensions needs its registers); Lane2: ndim alone --; in island mode the island size and the same row chunks
// instead; the kernel of one launch per generation by generation_wanted's kind, for what is neither resident nor in islands.
// the kernels of the sampler's plan as it stands (again after a re-plan); `r`: the resident choice, none in island mode
kmc_status load_user_kernels(kmc_sampler* s, const ResidentChoice& r)
{
    using Spec = UserModuleSpec;
    const kmc_config& c = s->cfg;
    Spec m;
    m.vec = s->plan.vec; m.L = s->plan.L; m.K = s->plan.K; m.iter = s->plan.ITER; m.ragged = s->plan.ragged;
    m.f32 = s->f32; m.ndim = c.ndim; m.p2p = (c.flags & KMC_P2P) != 0; m.move = c.move; m.temper = s->temper;
    if (s->islands) m.island_S = (int)s->island_size;
    else m.resident = r.kind == ResidentChoice::Pair ? Spec::Resident::Pair : r.kind == ResidentChoice::Lane ? Spec::Resident::Lane
                      : r.kind == ResidentChoice::Lane2 ? Spec::Resident::Lane2 : Spec::Resident::None;
    if (s->islands || m.resident == Spec::Resident::Pair) {
        m.pair_K = s->islands ? s->island_K : r.K;
        m.pair_ragged = 4 * m.pair_K != c.ndim;
    }
    if (m.resident == Spec::Resident::Lane && s->user->is_body) m.lane_bound = c.nwalkers <= 256 ? 256 : c.nwalkers <= 512 ? 512 : 1024;
    else if (m.resident == Spec::Resident::Lane) m.lane_nd = lane_nd(c.ndim);
    const bool lds_mode = s->islands || m.resident != Spec::Resident::None;
    const int gen = lds_mode ? 0 : generation_wanted(s);
    m.generation = gen == 1 ? Spec::Generation::Lane : gen == 2 ? Spec::Generation::Striped : gen == 3 ? Spec::Generation::Quad : Spec::Generation::None;
    // a big ensemble's kernels are worth the better compiler (hipcc as a child process: ~1.2 s once per density and geometry, then
    // cached on disk): inside a PyTorch process hiprtc means the older comgr the wheel bundles (kmc_rtc.hip: offline_compiler_wanted)
    set_offline_compiler_hint(s->h_loc >= 8192 && !lds_mode);
    const kmc_status st = load_user(s->user, m, &s->uk);
    set_offline_compiler_hint(false);
    return st;
}

kmc_status setup_user_density(kmc_sampler* s)
{
    const kmc_config& c = s->cfg;
    kmc_user_density* ud = s->user = static_cast<kmc_user_density*>(c.user_density);
    s->nblob = ud->nblob;
    if (ud->is_body && s->islands) return fail(KMC_ERR_UNSUPPORTED, "KMC_ISLANDS needs a menu or term / pair density (a body density runs one walker per lane)");
    if (ud->is_body && c.ndim > 1024) return fail(KMC_ERR_UNSUPPORTED, "a body density holds the proposal per lane: ndim <= 1024");
    // small ensembles: resident mode too.  A term / pair density's pair kernel takes 256 walkers
    ResidentChoice r;
    if (resident_possible(c) && !(ud->is_body && c.deal_count > 0))
        r = choose_resident(c, s->ld, ResidentFacts{ud->is_body, ud->nblob > 0, s->f32, !s->f32 && !ud->is_body, 256});
    // the first sampler over a body taken for a sum over elements finds out whether it is one (check_sum_form); samplers created
    // meanwhile on other threads wait for the answer instead of planning on a guess
    std::unique_lock<std::mutex> first_use;
    if (ud->is_body && ud->sep && sum_form_case(s) == 0) {
        first_use = std::unique_lock<std::mutex>(ud->check_mu);
        s->plan = make_plan(s->cfg, s->h_loc);
    }
    if (ud->is_body && ud->sep && sum_form_case(s) == 3) {       // (an earlier sampler of this very case found nothing to check the form against)
        s->sep_off = true;
        s->sep_off_note = "no test row had a finite log-density at this ndim with these parameters: its per-element form could not be checked";
    }
    SepOff sep_off_scope(s->sep_off);        // (for make_plan / compile_user / load_user below, which see the density, not the sampler; the rest of the set-up reads s->sep_off)
    if (s->sep_off) s->plan = make_plan(s->cfg, s->h_loc);
    KMC_TRY(load_user_kernels(s, r));
    // a body taken for a sum over elements: its generated form against the body itself, once, before anything runs it
    if (s->uk.logpdf_sep && sum_form_case(s) != 1) {
        KMC_TRY(check_sum_form(s));
        if (!ud->sep || s->sep_off) {                                 // not shown equal: plan and kernels for the body as written
            g_sep_off = g_sep_off || s->sep_off;                      // (restored by sep_off_scope at the end of this function)
            s->uk = UserKernels{};
            s->plan = make_plan(s->cfg, s->h_loc);
            KMC_TRY(load_user_kernels(s, r));
        }
    }
    if (r.kind != ResidentChoice::None) set_resident(s, r, std::max<size_t>(r.lds, 4096));
    return KMC_OK;
}

// ---- one launch per generation (see generation_wanted), for what is neither resident nor in islands ----
void setup_generation(kmc_sampler* s)
{
    const kmc_config& c = s->cfg;
    const int kind = (!s->islands && !s->resident) ? generation_wanted(s) : 0;
    if (kind == 0) return;
    if (s->user) s->fused = s->uk.generation != nullptr;
    else {
        s->generation_kernel = with_density(c.density, GenerationFn(nullptr), [&](auto d) {
            using D = decltype(d);
            return kind == 1 ? generation_lane_lookup<D>((int)c.ndim) : kind == 3 ? generation_group_lookup<D>(4, 1)
                                                                     : generation_group_lookup<D>(s->plan.L, s->plan.K);
        });
        s->fused = s->generation_kernel != nullptr;
    }
    if (!s->fused) return;
    s->fused_L = kind == 1 ? 0 : kind == 3 ? 4 : s->plan.L;
    // one wave per workgroup (measured best at every size for one walker per lane, `profiles/r04_generation_variants_ab.txt`); lane-striped:
    // two once the half's waves exceed the chip's SIMDs about once
    s->fused_tpb = (kind == 2 && s->h * s->plan.L > 64 * 512) ? 128 : 64;
    s->nislands = c.nwalkers;                     // per-walker moment sums [nwalkers][ld], within [nislands][4 island_K] (kmc_sampler_get_moments)
    s->island_K = (int)((s->ld + 3) / 4);
    s->fused_fold = s->fused_L > 0 && s->plan.K == 2 && (s->fused_L == 8 || s->fused_L == 16 || s->fused_L == 32) && kind == 2;
    if (s->fused_fold) {                          // ... or per-wave accumulators [waves][NVL][64] (generation_group, FoldT): the same sizing fields
        const int64_t per_wg = s->fused_tpb / s->fused_L;
        s->nislands = 2 * ((s->h + per_wg - 1) / per_wg) * (s->fused_tpb / 64);      // waves of a launch
        s->island_K = (8 * s->fused_L / 64) * 16;                                     // 4 island_K = NVL * 64 doubles per wave
    }
}

// ---- grid and accumulator layout of the two-launch kernels ----
void setup_launch_geometry(kmc_sampler* s)
{
    // vec: a wave owns W = (64/L)*ITER walkers; generic: one walker per lane
    const int64_t per_wave = s->plan.vec ? (int64_t)(64 / s->plan.L) * s->plan.ITER : 64;
    const int64_t waves = (s->h_loc + per_wave - 1) / per_wave;
    // vec kernels: vec_tpb(L) threads per workgroup; the generic kernel keeps 256
    const bool staged = s->user && s->uk.staged != nullptr;         // a body density's staged kernel: two waves per workgroup
    s->vec_lds = (s->user && s->user->is_body && !(s->user->sep && !s->sep_off) && s->plan.vec) ? (unsigned)body_vec_lds_bytes(s->plan.L, s->plan.K, s->plan.ITER) : 0u;
    s->tpb = s->plan.vec ? vec_tpb(s->plan.L) : (staged ? kStagedTPB : 256);
    s->grid = (int)((waves * 64 + s->tpb - 1) / s->tpb);
    s->macc_stride = (int64_t)s->grid * s->tpb;
    s->macc_elems = s->plan.vec ? s->macc_stride * 2 * s->plan.K : s->macc_stride * s->cfg.ndim;
}

// ---- device state.  Every fill below is asynchronous on the sampler's stream: kmc_sampler_create waits for all of them once ----
kmc_status create_stream(kmc_sampler* s)
{
    HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    s->own_stream = true;
    HIP_TRY(hipEventCreate(&s->ev0));
    HIP_TRY(hipEventCreate(&s->ev1));
    return KMC_OK;
}

// the mixture's table and the P2P flags
kmc_status alloc_exchange(kmc_sampler* s)
{
    const kmc_config& c = s->cfg;
    if (c.move == KMC_MOVE_MIX) {
        const MixTable mt = mix_table_of(c);
        HIP_TRY(dev_alloc(s, (void**)&s->d_mix, sizeof(MixTable)));
        HIP_TRY(copy_sync(s->d_mix, &mt, sizeof(MixTable), hipMemcpyHostToDevice, s->stream));
    }
    if (s->p2p) {
        HIP_TRY(hipExtMallocWithFlags((void**)&s->d_flags, 4096, hipDeviceMallocFinegrained));
        HIP_TRY(hipMemsetAsync(s->d_flags, 0, 4096, s->stream));
        HIP_TRY(dev_alloc(s, (void**)&s->d_err, 64));
        HIP_TRY(hipMemsetAsync(s->d_err, 0, 64, s->stream));
        // KMC_P2P_PUSH: local copies of the other shards, which their owners write; the menu densities' vector kernels carry it (anything
        // else keeps the pull -- kmc_sampler_describe says which runs)
        s->push = (c.flags & KMC_P2P_PUSH) != 0 && s->plan.vec && s->user == nullptr && !(c.flags & KMC_P2P_FINEGRAINED) && c.shard_count > 1;
    }
    return KMC_OK;
}

// the ladder's block: betas, logp_sum, the moments credited at exchanges, the adaptive ladder's state (kmc_sampler.hpp), and the swap counters
kmc_status alloc_tempering(kmc_sampler* s)
{
    if (!s->temper) return KMC_OK;
    const size_t nt = (size_t)s->ntemps;
    const size_t nb = (2 * nt + 2 * (size_t)s->ld + 2 * nt + 2 + 2 * nt) * sizeof(double);
    HIP_TRY(dev_alloc(s, &s->d_betas, nb));
    HIP_TRY(hipMemsetAsync(s->d_betas, 0, nb, s->stream));
    HIP_TRY(copy_sync(s->d_betas, s->betas.data(), nt * sizeof(double), hipMemcpyHostToDevice, s->stream));
    s->d_rung_sum = s->d_betas + nt;
    s->d_tsum = s->d_rung_sum + nt;
    s->d_S = s->d_tsum + 2 * (size_t)s->ld;
    s->d_round_acc = reinterpret_cast<unsigned long long*>(s->d_S + nt);
    s->d_ticket = reinterpret_cast<unsigned int*>(s->d_round_acc + nt);
    s->d_skipped = s->d_round_acc + nt + 1;
    s->d_stage = reinterpret_cast<double*>(s->d_skipped + 1);
    if (!s->S0.empty()) HIP_TRY(copy_sync(s->d_S, s->S0.data(), s->S0.size() * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(dev_alloc(s, (void**)&s->d_nswap, nt * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(s->d_nswap, 0, nt * sizeof(unsigned long long), s->stream));
    return KMC_OK;
}

// rows, the per-walker block, the generation counter, the schedule, a dealt sub-ensemble's ids; every per-walker array holds ntemps ensembles
kmc_status alloc_state(kmc_sampler* s)
{
    const kmc_config& c = s->cfg;
    const size_t nw = (size_t)s->nrows, nt = (size_t)s->ntemps, ldz = (size_t)s->ld;
    const size_t esz = s->f32 ? sizeof(float) : sizeof(double);      // element size of rows and chain
    const size_t pos_bytes = (s->push ? 1 + (size_t)c.shard_count : nt) * nw * ldz * esz;
    if (s->p2p && (c.flags & KMC_P2P_FINEGRAINED))   // peers map the rows uncached: nothing of them can go stale in a reader's L2
        HIP_TRY(hipExtMallocWithFlags((void**)&s->d_pos, nw * ldz * sizeof(double), hipDeviceMallocFinegrained));
    else
        HIP_TRY(dev_alloc(s, &s->d_pos, pos_bytes));
    HIP_TRY(hipMemsetAsync(s->d_pos, 0, pos_bytes, s->stream));   // the pad column of odd ndim stays 0
    // per-walker block {logp[nrows], naccept[nrows], klast[nrows]}: one allocation, so the half-step kernels reach all
    // three from one preloaded pointer (HalfStepFront::logp)
    const size_t block_bytes = nt * nw * (sizeof(double) + 2 * sizeof(uint32_t));
    HIP_TRY(dev_alloc(s, &s->d_logp, block_bytes));
    if (s->temper) HIP_TRY(hipMemsetAsync(s->d_logp, 0, block_bytes, s->stream));   // (every rung's counters)
    s->d_naccept = reinterpret_cast<uint32_t*>(s->d_logp + nw);
    s->d_klast = s->d_naccept + nw;
    if (s->ragged_vec() && (reinterpret_cast<uint64_t>(s->d_logp) >> 48) != 0)   // (kmc_launch.hip: front_of -- ndim rides in the 16 bits above this address)
        return fail(KMC_ERR_UNSUPPORTED, "device addresses beyond 2^48: the ragged vector kernels carry ndim in the upper 16 bits of a pointer");
    HIP_TRY(hipMemsetAsync(s->d_klast, 0, nw * sizeof(uint32_t), s->stream));
    static_assert(kGraphChunk <= 64, "advance_schedule runs one 64-thread block");
    HIP_TRY(dev_alloc(s, &s->d_gen, 64));
    HIP_TRY(hipMemsetAsync(s->d_gen, 0, 64, s->stream));
    HIP_TRY(dev_alloc(s, &s->d_sched, (size_t)kGraphChunk * sizeof(SchedEntry)));
    HIP_TRY(hipMemsetAsync(s->d_naccept, 0, nw * sizeof(uint32_t), s->stream));
    if (c.deal_count > 0) HIP_TRY(dev_alloc(s, (void**)&s->d_ids, nw * sizeof(uint32_t)));
    return KMC_OK;
}

// the vector kernels' draw ring and resident mode's draw table
kmc_status alloc_draws(kmc_sampler* s)
{
    // Draw ring (kmc_kernels.hpp: kRing; possible for L = 16 / 32 with L / ITER >= 2): a wave computes its walkers' next steps' draws with its idle lanes and parks
    // them, 4 slots x rows x 32 B; tags start at 0xffffffff (no step carries it), so nothing is "parked" yet.  Where it pays was re-measured in round 5
    // (scripts/probes/ring_ab.py, profiles/r05_ring_ab.txt) -- since the launches carry their step among the preloaded parameters Philox starts at wave entry and the
    // ring's entry is one more dependent load in front of the partner row: rows LOSE 2-7 % with it at ITER = 2 and at L = 32, exact-size and ragged alike (the ragged
    // kernels gained 6-10 % from it only while their loads sat behind exec-mask regions and scalar waits; without those they behave like the exact-size ones), and
    // 6-14 % in the large-ensemble geometries (ITER >= 4: bandwidth-bound, the ring is bytes); L = 16, ITER = 1 (C3's geometry) is +-1 % exact-size, -1..2 % ragged, and keeps it.
    // KMC_DEBUG=ring=0|1 forces it off / on wherever the kernel has one.
    const Plan& p = s->plan;
    bool want_ring = p.vec && !two_launch_only(s->cfg) && !s->islands && !s->resident && p.L >= 16 && p.L <= 32 && p.L / p.ITER >= 2;
    std::string forced;
    if (want_ring && debug_opt("ring", &forced)) want_ring = forced != "0";
    else if (want_ring) want_ring = p.L == 16 && p.ITER == 1;
    if (want_ring) {
        const size_t nb = 4 * (size_t)s->nrows * 2 * sizeof(double2);
        HIP_TRY(dev_alloc(s, (void**)&s->d_ring, nb));
        HIP_TRY(hipMemsetAsync(s->d_ring, 0xff, nb, s->stream));
    }
    if (s->resident)                                 // the launch's draws come from a wide kernel (draw_table_fill, kmc_islands.hpp)
        HIP_TRY(dev_alloc(s, (void**)&s->d_draws, (size_t)kDrawTableGens * (size_t)s->nrows * 2 * sizeof(double2)));
    return KMC_OK;
}

// KMC_MOMENTS: the two-launch kernels' accumulators, long rows' moment ring, and the per-island / per-walker / per-wave sums of the other routes
kmc_status alloc_moments(kmc_sampler* s)
{
    if (!(s->cfg.flags & KMC_MOMENTS)) return KMC_OK;
    const size_t macc_bytes = (size_t)s->macc_elems * sizeof(double);
    HIP_TRY(dev_alloc(s, &s->d_msum, macc_bytes));
    HIP_TRY(dev_alloc(s, &s->d_msumsq, macc_bytes));
    HIP_TRY(hipMemsetAsync(s->d_msum, 0, macc_bytes, s->stream));
    HIP_TRY(hipMemsetAsync(s->d_msumsq, 0, macc_bytes, s->stream));
    if (s->plan.vec && s->plan.L == 64 && !s->islands && !s->resident && !debug_opt("no-moment-ring")) {
        // moment ring for long rows (kmc_kernels.hpp, HalfStepArgs::mring): up to 128 posted rows per wave,
        // within 512 MiB in all; swept every kSweepEvery generations
        const int64_t nwaves = s->macc_stride / 64;
        const size_t slot = (size_t)s->plan.K * 64 * sizeof(double2);       // one row
        int64_t depth = (int64_t)(((size_t)1 << 29) / ((size_t)nwaves * slot));
        if (depth > 128) depth = 128;
        const long forced_depth = debug_opt_long("moment-ring-depth", 0);                         // tests: force overflows
        if (forced_depth >= 1 && forced_depth < depth) depth = forced_depth;
        if (depth >= 4 || (depth >= 2 && forced_depth > 0)) {
            HIP_TRY(dev_alloc(s, (void**)&s->d_mring, (size_t)nwaves * (size_t)depth * slot));
            HIP_TRY(dev_alloc(s, (void**)&s->d_mring_w, (size_t)nwaves * (size_t)depth * sizeof(double)));
            HIP_TRY(dev_alloc(s, (void**)&s->d_mcnt, 2 * (size_t)nwaves * sizeof(uint32_t)));
            HIP_TRY(hipMemsetAsync(s->d_mcnt, 0, 2 * (size_t)nwaves * sizeof(uint32_t), s->stream));
            s->mring_depth = (int)depth;
            s->mring_waves = nwaves;
        }
    }
    if (s->islands || s->resident || s->fused) {
        const size_t ne = (size_t)s->nislands * 4 * (size_t)s->island_K;
        HIP_TRY(dev_alloc(s, &s->d_isum, ne * sizeof(double)));
        HIP_TRY(dev_alloc(s, &s->d_isumsq, ne * sizeof(double)));
        HIP_TRY(hipMemsetAsync(s->d_isum, 0, ne * sizeof(double), s->stream));
        HIP_TRY(hipMemsetAsync(s->d_isumsq, 0, ne * sizeof(double), s->stream));
    }
    return KMC_OK;
}

// one launch per generation: the second copy of the state (pad column of an odd ndim: 0 in both)
kmc_status alloc_second_state(kmc_sampler* s)
{
    if (!s->fused) return KMC_OK;
    const size_t nw = (size_t)s->nrows;
    HIP_TRY(dev_alloc(s, &s->d_pos2, nw * (size_t)s->ld * sizeof(double)));
    HIP_TRY(hipMemsetAsync(s->d_pos2, 0, nw * (size_t)s->ld * sizeof(double), s->stream));
    HIP_TRY(dev_alloc(s, &s->d_logp2, nw * sizeof(double)));
    if (s->fused_L > 0) {
        HIP_TRY(dev_alloc(s, (void**)&s->d_glast, nw * sizeof(uint32_t)));
        HIP_TRY(hipMemsetAsync(s->d_glast, 0, nw * sizeof(uint32_t), s->stream));
    }
    return KMC_OK;
}

// KMC_DATA_DENSITY: proposals, their sums and the tree's scratch
kmc_status alloc_data_route(kmc_sampler* s)
{
    // (a likelihood-tempered ladder: every rung's proposals in one pass -- nt h rows, S and the prior apart -- and every rung's rows at set_positions)
    const size_t nt = (size_t)s->ntemps, np_half = nt * (size_t)s->h, np_all = nt * (size_t)s->nrows;
    HIP_TRY(dev_alloc(s, &s->d_prop, np_half * (size_t)s->ld * sizeof(double)));
    HIP_TRY(dev_alloc(s, &s->d_p1, (s->temper_like ? 2 : 1) * np_half * sizeof(double)));
    // the plans are decided here, once (KMC_DEBUG=data-map may change later in the process: the kernels keep the geometry d_part was sized for)
    s->plan_half = data_plan(s->data_ud, (int64_t)np_half);
    s->plan_all = data_plan(s->data_ud, (int64_t)np_all);
    s->part_doubles = std::max((size_t)s->plan_half.nblocks * np_half, (size_t)s->plan_all.nblocks * np_all);
    HIP_TRY(dev_alloc(s, &s->d_part, s->part_doubles * sizeof(double)));
    if (s->temper_like) {
        const size_t nb = (2 * np_all + nt) * sizeof(double);
        HIP_TRY(dev_alloc(s, &s->d_like, nb));
        HIP_TRY(hipMemsetAsync(s->d_like, 0, nb, s->stream));
        s->d_prior = s->d_like + np_all;
        s->d_like_sum = s->d_prior + np_all;
    }
    return KMC_OK;
}

// KMC_HOST_DENSITY: proposals and log-pdfs on the device and page-locked on the host, accept outcomes for host_accepted
kmc_status alloc_host_route(kmc_sampler* s)
{
    const size_t h = (size_t)s->h;
    HIP_TRY(dev_alloc(s, &s->d_prop, h * (size_t)s->ld * sizeof(double)));
    HIP_TRY(dev_alloc(s, &s->d_p1, h * sizeof(double)));
    HIP_TRY(hipHostMalloc((void**)&s->h_prop, h * (size_t)s->cfg.ndim * sizeof(double), hipHostMallocDefault));
    HIP_TRY(hipHostMalloc((void**)&s->h_p1, h * sizeof(double), hipHostMallocDefault));
    if (hipHostGetDevicePointer((void**)&s->h_prop_dev, s->h_prop, 0) != hipSuccess ||
        hipHostGetDevicePointer((void**)&s->h_p1_dev, s->h_p1, 0) != hipSuccess) {
        (void)hipGetLastError();
        s->h_prop_dev = s->h_p1_dev = nullptr;          // (then every batch goes through the copies)
    }
    if (s->cfg.host_accepted) {
        HIP_TRY(dev_alloc(s, &s->d_acc, h));
        HIP_TRY(hipHostMalloc((void**)&s->h_acc, h, hipHostMallocDefault));
    }
    return KMC_OK;
}

// KMC_STREAM_CHAIN: the ring's block size, the transposed / compacted block, the copy stream and its events.  Returns through
// s->ring_slots how many sample slots the chain on the device then has.
kmc_status setup_stream_ring(kmc_sampler* s)
{
    const kmc_config& c = s->cfg;
    // a ring of three blocks; a block holds at least the samples of one launch unit (a graph replay), so a unit never
    // touches more than two blocks, and about 512 MiB otherwise (measured at C2: 128 MiB blocks stream 22-26 GB/s at nthin = 10, 512 MiB blocks 43-45 GB/s of the
    // 56 GB/s this link copies alone; many small blocks cost more at the block boundaries than their earlier start
    // returns -- nthin = 100: +19 % on the loop with 64 MiB blocks, +6 % with 512 MiB; KMC_DEBUG=chain-block=n: samples per block, for tests)
    const int64_t unit = s->resident ? 1 : std::max<int64_t>(kGraphChunk, s->uchunk);     // (a resident launch is cut to the block: kmc_sampler_run)
    const int64_t per_unit = (unit + c.nthin - 1) / c.nthin + 1;
    const size_t sample_bytes = (size_t)s->nlocal * (size_t)s->ld * sizeof(double);
    int64_t blk = (int64_t)(((size_t)512 << 20) / sample_bytes);
    if (blk < 1) blk = 1;
    if (blk > 4096) blk = 4096;
    { const long v = debug_opt_long("chain-block", 0); if (v >= 1) blk = v; }
    if (blk < per_unit) blk = per_unit;
    s->stream_chain = true;
    s->stream_by_walker = (c.flags & KMC_CHAIN_BY_WALKER) != 0;
    const size_t block_doubles = (size_t)blk * (size_t)s->nlocal;
    if (s->stream_by_walker) {
        if (c.flags & KMC_STORE_CHAIN) HIP_TRY(dev_alloc(s, &s->bw_scratch, block_doubles * (size_t)c.ndim * sizeof(double)));
        if (c.flags & KMC_STORE_LOGP) HIP_TRY(dev_alloc(s, &s->bw_scratch_logp, block_doubles * sizeof(double)));
    } else if ((c.flags & KMC_STORE_CHAIN) && s->ld != c.ndim) {
        HIP_TRY(dev_alloc(s, &s->bw_scratch, block_doubles * (size_t)c.ndim * sizeof(double)));   // (rows_compact)
    }
    s->ring_blk = blk;
    s->ring_slots = 3 * blk;
    HIP_TRY(hipStreamCreateWithFlags(&s->copy_stream, hipStreamNonBlocking));
    for (int i = 0; i < 3; ++i) {
        HIP_TRY(hipEventCreateWithFlags(&s->ev_filled[i], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&s->ev_copied[i], hipEventDisableTiming));
    }
    return KMC_OK;
}

// the stored chain, its log-pdfs and blobs -- whole, or as the stream ring
kmc_status alloc_chain(kmc_sampler* s)
{
    const kmc_config& c = s->cfg;
    const size_t ldz = (size_t)s->ld, esz = s->f32 ? sizeof(float) : sizeof(double);
    const bool stored = s->nsamples > 0;
    if ((c.flags & KMC_STREAM_CHAIN) && stored) KMC_TRY(setup_stream_ring(s));
    const size_t slot_rows = (size_t)(s->stream_chain ? s->ring_slots : s->nsamples) * (size_t)s->nlocal;
    if ((c.flags & (KMC_STORE_CHAIN | KMC_STORE_LOGP)) && stored) {
        // A chain that cannot fit is refused HERE, not by a failing hipMalloc: after a failed allocation of hundreds of GB the
        // runtime aborted the process a few calls later (observed: 4 of 5 runs, in the first HIP call of the next sampler).
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        const size_t need = slot_rows * (((c.flags & KMC_STORE_CHAIN) ? ldz * esz : 0) + ((c.flags & KMC_STORE_LOGP) ? sizeof(double) : 0));
        if (need > free_b)
            return fail(KMC_ERR_OOM, "the chain needs " + std::to_string(need >> 20) + " MiB of device memory, " + std::to_string(free_b >> 20) +
                                     (s->nblob > 0 ? " MiB are free: thin it (nthin)" : " MiB are free: thin it (nthin), or stream it to host memory (KMC_STREAM_CHAIN)"));
    }
    if ((c.flags & KMC_STORE_CHAIN) && stored) HIP_TRY(dev_alloc(s, &s->d_chain, slot_rows * ldz * esz));
    if ((c.flags & KMC_STORE_LOGP) && stored) HIP_TRY(dev_alloc(s, &s->d_chain_logp, slot_rows * sizeof(double)));
    if (s->nblob > 0) {
        const size_t blob_bytes = (size_t)s->nrows * (size_t)s->nblob * sizeof(double);
        HIP_TRY(dev_alloc(s, &s->d_blob, blob_bytes));
        HIP_TRY(hipMemsetAsync(s->d_blob, 0, blob_bytes, s->stream));
        if ((c.flags & KMC_STORE_BLOBS) && stored) {
            const size_t need_b = (size_t)s->nsamples * (size_t)s->nlocal * (size_t)s->nblob * sizeof(double);
            size_t free_b = 0, total_b = 0;
            HIP_TRY(hipMemGetInfo(&free_b, &total_b));
            if (need_b > free_b)
                return fail(KMC_ERR_OOM, "the stored blobs need " + std::to_string(need_b >> 20) + " MiB of device memory, " + std::to_string(free_b >> 20) + " MiB are free: thin the chain (nthin)");
            HIP_TRY(dev_alloc(s, &s->d_chain_blob, need_b));
        }
    }
    return KMC_OK;
}
}  // namespace

KMC_EXPORT kmc_status kmc_sampler_create(const kmc_config* cfg, kmc_sampler** out)
{
    if (!out) return fail(KMC_ERR_BAD_ARG, "null out");
    *out = nullptr;
    KMC_TRY(kmc_validate(cfg));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return fail(KMC_ERR_NO_DEVICE, "no HIP device visible: the emcee hot path has no CPU fallback");
    }
    if (cfg->device < 0 || cfg->device >= ndev) return fail(KMC_ERR_BAD_ARG, "device ordinal out of range");
    HIP_TRY(hipSetDevice(cfg->device));

    std::unique_ptr<kmc_sampler, SamplerDeleter> owner(new kmc_sampler());
    kmc_sampler* s = owner.get();
    // which route: islands, resident, one launch per generation, or the two launches of the plan
    KMC_TRY(init_shape(s, *cfg));
    if (cfg->flags & KMC_ISLANDS) KMC_TRY(setup_islands(s));
    if (cfg->density == KMC_USER_DENSITY) {
        KMC_TRY(setup_user_density(s));
    } else if (cfg->density == KMC_HOST_DENSITY) {
        s->host_eval = true;
    } else if (cfg->density == KMC_DATA_DENSITY) {
        // the host route's PROPOSE and ACCEPT passes, with the data kernels in place of the callback (kmc_launch.hip)
        s->host_eval = true;
        s->data_eval = true;
        s->data_ud = static_cast<kmc_user_density*>(cfg->user_density);
        KMC_TRY(load_data(s->data_ud, cfg->ndim, &s->dk));
    } else {
        s->logpdf_fn = logpdf_fn(cfg->density);
        setup_menu_resident(s);
    }
    setup_generation(s);
    setup_launch_geometry(s);
    // its device state
    KMC_TRY(create_stream(s));
    KMC_TRY(alloc_exchange(s));
    KMC_TRY(alloc_tempering(s));
    KMC_TRY(alloc_state(s));
    KMC_TRY(alloc_draws(s));
    KMC_TRY(alloc_moments(s));
    KMC_TRY(alloc_second_state(s));
    if (s->data_eval) KMC_TRY(alloc_data_route(s));
    else if (s->host_eval) KMC_TRY(alloc_host_route(s));
    KMC_TRY(alloc_chain(s));
    HIP_TRY(hipStreamSynchronize(s->stream));         // the fills above (asynchronous, one wait for all of them)
    if (s->p2p) {
        s->peer_pos[s->cfg.shard_rank] = s->d_pos;
        s->peer_flags[s->cfg.shard_rank] = s->d_flags;
        s->connected = s->cfg.shard_count == 1;
    }
    *out = owner.release();
    return KMC_OK;
}

KMC_EXPORT void kmc_sampler_destroy(kmc_sampler* s)
{
    if (!s) return;
    (void)hipSetDevice(s->cfg.device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    if (s->copy_stream) (void)hipStreamSynchronize(s->copy_stream);
    // The buffers go back to the allocation cache below, without the device-wide wait hipFree used to imply.  Work that OTHER
    // streams may still have in flight on them -- a caller's stream bound earlier (kmc_sampler_set_stream), a framework's
    // collectives on a replica shard's rows -- is waited for here; a plain single-GPU sampler (its own stream only) pays nothing.
    if (s->foreign_stream_seen || s->cfg.shard_count > 1 || s->comm) (void)hipDeviceSynchronize();
    if (s->stream) check_guards(s);
    drop_updated_graph(s);
    if (s->graph_exec) (void)hipGraphExecDestroy(s->graph_exec);
    s->uk.keep.reset();                 // (the module goes when its last holder does: the density's cache, other samplers)
    if (s->graph) (void)hipGraphDestroy(s->graph);
    if (s->ev0) (void)hipEventDestroy(s->ev0);
    if (s->ev1) (void)hipEventDestroy(s->ev1);
    if (s->p2p) {
        for (int r = 0; r < 8; ++r) {
            if (r == s->cfg.shard_rank) continue;
            if (s->peer_pos[r]) (void)hipIpcCloseMemHandle(s->peer_pos[r]);
            if (s->peer_flags[r]) (void)hipIpcCloseMemHandle(s->peer_flags[r]);
        }
    }
    if (s->comm) { rccl_comm_destroy(s->comm); s->comm = nullptr; }
    if (s->copy_stream) { (void)hipStreamSynchronize(s->copy_stream); (void)hipStreamDestroy(s->copy_stream); }
    for (int i = 0; i < 3; ++i) {
        if (s->ev_filled[i]) (void)hipEventDestroy(s->ev_filled[i]);
        if (s->ev_copied[i]) (void)hipEventDestroy(s->ev_copied[i]);
    }
    chain_unregister(s);
    for (const DevAlloc& a : s->allocs) cache_free(a.p);              // everything dev_alloc handed out (a bound d_pos is not the sampler's: not in the list)
    // ... and what did not come from it: the fine-grained P2P buffers and the page-locked host arrays
    if (s->p2p) {
        cache_free(s->d_flags);
        if ((s->cfg.flags & KMC_P2P_FINEGRAINED) && s->own_pos) cache_free(s->d_pos);
    }
    if (s->h_prop) (void)hipHostFree(s->h_prop);
    if (s->h_p1) (void)hipHostFree(s->h_p1);
    if (s->h_acc) (void)hipHostFree(s->h_acc);
    for (int i = 0; i < kHostPieces; ++i) if (s->host_ev[i]) (void)hipEventDestroy(s->host_ev[i]);
    if (s->own_stream && s->stream) (void)hipStreamDestroy(s->stream);
    (void)hipGetLastError();
    delete s;
}

KMC_EXPORT kmc_status kmc_sampler_set_stream(kmc_sampler* s, void* hip_stream)
{
    if (!s) return fail(KMC_ERR_BAD_ARG, "null sampler");
    HIP_TRY(hipSetDevice(s->cfg.device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (s->own_stream && s->stream) (void)hipStreamDestroy(s->stream);
    s->stream = (hipStream_t)hip_stream;
    s->own_stream = false;
    s->foreign_stream_seen = true;
    return KMC_OK;
}

KMC_EXPORT kmc_status kmc_sampler_bind_positions(kmc_sampler* s, void* pos_dev)
{
    if (!s || !pos_dev) return fail(KMC_ERR_BAD_ARG, "null argument");
    if (s->p2p) return fail(KMC_ERR_UNSUPPORTED, "KMC_P2P samplers export their own position buffer");
    if (s->temper) return fail(KMC_ERR_UNSUPPORTED, "parallel tempering: the sampler keeps every rung's rows in its own buffer (no kmc_sampler_bind_positions)");
    if (s->f32) return fail(KMC_ERR_UNSUPPORTED, "kmc_sampler_bind_positions takes double rows; a KMC_F32 sampler keeps its own float rows");
    if (s->ld != s->cfg.ndim) return fail(KMC_ERR_UNSUPPORTED, "kmc_sampler_bind_positions needs an even ndim (16-byte rows)");
    HIP_TRY(hipSetDevice(s->cfg.device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (s->graph_exec) { (void)hipGraphExecDestroy(s->graph_exec); s->graph_exec = nullptr; }
    if (s->graph) { (void)hipGraphDestroy(s->graph); s->graph = nullptr; }
    drop_updated_graph(s);                                              // (ensure_updated_graph builds it anew)
    if (s->own_pos) dev_free(s, s->d_pos);                              // (out of the allocation record: its guard, under KMC_DEBUG=poison, goes with it)
    s->d_pos = static_cast<double*>(pos_dev);
    s->own_pos = false;
    s->pos2_current = false;
    s->positions_set = false;
    return KMC_OK;
}

KMC_EXPORT int64_t kmc_sampler_generation(const kmc_sampler* s) { return s ? s->generation : -1; }
KMC_EXPORT int64_t kmc_sampler_nsamples(const kmc_sampler* s) { return s ? s->nsamples : -1; }
KMC_EXPORT int64_t kmc_sampler_launch_count(const kmc_sampler* s) { return s ? s->launches : -1; }

KMC_EXPORT void* kmc_sampler_device_ptr(kmc_sampler* s, int which)
{
    if (!s) return nullptr;
    if (which == 0 || which == 1) s->pos_exposed = true;         // (the caller may write there: a one-launch-per-generation sampler then re-synchronises its second copy before every run)
    switch (which) {
    case 0: return s->d_pos;
    case 1: return s->d_logp;
    case 2: return s->d_naccept;
    default: return nullptr;
    }
}

// (tests; touches no device) The kernel variant -- kVarGeneric, kVarCredit or kVarShareBurnin -- behind a replay of n generations from g0 on, for a menu-density
// sampler of this shape on the two-launch route in the updated-graph mode: the plan, the launch geometry and spec_of_chunk as a real sampler has them.
KMC_EXPORT int kmc_debug_replay_variant(int density, int64_t nwalkers, int64_t ndim, int64_t nburnin, int64_t g0, int64_t n, int moments, int chain)
{
    static double some = 0.0;
    kmc_sampler s;
    s.cfg.density = density; s.cfg.nwalkers = nwalkers; s.cfg.ndim = ndim; s.cfg.nburnin = nburnin; s.cfg.shard_count = 1;
    s.h = s.h_loc = nwalkers / 2;
    s.plan = make_plan(s.cfg, s.h_loc);
    setup_launch_geometry(&s);
    s.d_msum = moments ? &some : nullptr;
    s.d_chain = chain ? &some : nullptr;
    return spec_of_chunk(&s, g0, n);
}

KMC_EXPORT int kmc_sizeof_config(void) { return (int)sizeof(kmc_config); }
KMC_EXPORT int kmc_sizeof_metropolis_config(void) { return (int)sizeof(kmc_metropolis_config); }
KMC_EXPORT int kmc_sizeof_outputs(void) { return (int)sizeof(kmc_outputs); }
KMC_EXPORT int kmc_sizeof_metropolis_outputs(void) { return (int)sizeof(kmc_metropolis_outputs); }

