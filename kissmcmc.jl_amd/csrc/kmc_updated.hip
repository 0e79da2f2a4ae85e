// kmc_updated.hip -- the "updated graph" launch mode of kmc_sampler_run (kmc_launch.hip: launch modes): the eager form of the kernels as the
// nodes of a hipGraph whose parameters are rewritten before every replay, the executables that take turns, and the process-wide budget of
// such parameter updates.  Host code only: the kernels behind the nodes are kmc_launch.hip's.
#include <atomic>
#include <chrono>
#include <cstdio>

#include "kmc_sampler.hpp"

using namespace kmc;
using namespace kmc_host;

namespace kmc_host {

namespace {
// storage the kernelParams pointers of one node refer to: a half-step kernel's leading scalars and its struct, or a generation kernel's
// (one launch per generation) -- a sampler's nodes are all of one kind
struct ParamPack {
    HalfStepFront hf;
    HalfStepArgs ha;
    GenerationFront gf;
    GenerationArgs ga;
    void* ptrs[11];
    explicit ParamPack(bool fused)
    {
        if (fused) {
            ptrs[0] = &gf.sched; ptrs[1] = &gf.pin; ptrs[2] = &gf.lin; ptrs[3] = &gf.pout; ptrs[4] = &gf.seed_lo; ptrs[5] = &gf.seed_hi;
            ptrs[6] = &gf.h; ptrs[7] = &gf.nb; ptrs[8] = &gf.ld; ptrs[9] = &gf.gen; ptrs[10] = &ga;
        } else {
            ptrs[0] = &hf.pos; ptrs[1] = &hf.sched; ptrs[2] = &hf.ring_now; ptrs[3] = &hf.logp; ptrs[4] = &hf.gw0; ptrs[5] = &hf.nact_half;
            ptrs[6] = &hf.seed_lo; ptrs[7] = &hf.seed_hi; ptrs[8] = &hf.nhalf; ptrs[9] = &hf.step; ptrs[10] = &ha;
        }
    }
};

// the kernel behind the nodes of a variant's graph (half-step kernels of a menu density; everything else has the generic variant only)
HalfStepFn variant_fn(const kmc_sampler* s, int variant)
{
    return variant == kVarCredit ? s->plan.fn_credit : variant == kVarShareBurnin ? s->plan.fn_share_burnin : s->plan.fn;
}
}  // namespace

// The shared-draws variant launches SHARE waves per workgroup over the same waves (the global wave index keeps its meaning): its own grid and block.
int variant_share(const kmc_sampler* s, int variant)
{
    return variant == kVarShareBurnin ? s->plan.share_burnin : 0;
}

namespace {
// walkers per workgroup of a variant's launch
int64_t variant_walkers_per_wg(const kmc_sampler* s, int variant)
{
    const int share = variant_share(s, variant);
    return (int64_t)(share > 0 ? share : s->tpb / 64) * (64 / s->plan.L) * s->plan.ITER;
}

hipKernelNodeParams node_params(const kmc_sampler* s, int variant, ParamPack* pk)
{
    hipKernelNodeParams np{};
    if (s->fused) {
        np.func = s->user ? reinterpret_cast<void*>(s->uk.generation) : reinterpret_cast<void*>(s->generation_kernel);
        np.gridDim = dim3(2u * pk->ga.nb);
        np.blockDim = dim3((unsigned)s->fused_tpb);
        np.sharedMemBytes = 0u;
    } else {
        // (a runtime-compiled density's lane-striped kernel is a module function: the runtime accepts its hipFunction_t as the node's
        //  function -- ensure_updated_graph tries it once and the sampler stays with the table graph if it does not)
        np.func = s->user ? reinterpret_cast<void*>(s->uk.vec) : reinterpret_cast<void*>(variant_fn(s, variant));
        np.gridDim = dim3((unsigned)s->grid);
        np.blockDim = dim3((unsigned)s->tpb);
        if (const int share = variant_share(s, variant); share > 0) {       // (spec_variant_possible: h_loc is a whole number of its workgroups)
            np.gridDim = dim3((unsigned)(s->h_loc / variant_walkers_per_wg(s, variant)));
            np.blockDim = dim3(64u * (unsigned)share);
        }
        np.sharedMemBytes = s->user ? s->vec_lds : 0u;
    }
    np.kernelParams = pk->ptrs;
    np.extra = nullptr;
    return np;
}

// The nodes of a replay of s->uchunk generations that starts at generation g0, in their order: visit(k, parameters of node k).  A sampler that
// runs one launch per generation has one node per generation, reading copy g & 1 of the state and writing the other (uchunk is even: a replay
// ends in the copy it started from); otherwise a generation is its two half-steps.
template <class Visit>
kmc_status for_each_node(const kmc_sampler* s, int variant, int64_t g0, Visit&& visit)
{
    ParamPack pk(s->fused);
    const int64_t per_gen = launches_per_generation(s);
    for (int64_t k = 0; k < per_gen * s->uchunk; ++k) {
        const int64_t g = k / per_gen;
        if (s->fused) {
            pk.ga = make_generation_args(s, (int)(g & 1), false, g0 + g);
            pk.gf = generation_front_of(pk.ga, s->fused_tpb);
        } else {
            pk.ha = make_args(s, (int)(k & 1), false, g0 + g);
            pk.hf = front_of(pk.ha, s->ragged_vec());
        }
        KMC_TRY(visit(k, node_params(s, variant, &pk)));
    }
    return KMC_OK;
}
}  // namespace

void drop_updated_graph(kmc_sampler* s)
{
    for (int i = 0; i < kUExec; ++i) {
        for (int v = 0; v < kUVariants; ++v)
            if (s->uexec[v][i]) { (void)hipGraphExecDestroy(s->uexec[v][i]); s->uexec[v][i] = nullptr; }
        if (s->udone[i]) { (void)hipEventDestroy(s->udone[i]); s->udone[i] = nullptr; }      // (ensure_updated_graph creates them anew)
        s->uinflight[i] = false;
    }
    s->unext = 0;
    for (int v = 0; v < kUVariants; ++v)
        if (s->ugraph[v]) { (void)hipGraphDestroy(s->ugraph[v]); s->ugraph[v] = nullptr; }
}

// The phase-specialised instance (kmc_kernels.hpp: Spec::Credit) serves the two-launch vector route of a menu density whose grid is exactly full, with
// streaming moments and nothing stored per sample.  KMC_DEBUG=spec=0: the generic kernel everywhere (A/B runs, tests).
// The workgroup-shared-draws instance (kmc_shared_draws.hpp) serves burn-in replays of the same route where the grid is exactly full in ITS workgroups,
// whatever the sampler stores or credits later (a burn-in generation stores and credits nothing).  KMC_DEBUG=share=0: the generic kernel in burn-in, as
// before it.
bool spec_variant_possible(const kmc_sampler* s, int variant, const char** why_not)
{
    const char* why = nullptr;
    std::string v;
    const bool credits = variant == kVarCredit;
    if (variant == kVarGeneric) return true;
    if (debug_opt("spec", &v) && v == "0") why = "KMC_DEBUG=spec=0";
    else if (variant == kVarShareBurnin && debug_opt("share", &v) && v == "0") why = "KMC_DEBUG=share=0";
    else if (s->user || s->fused || s->host_eval || !s->plan.vec) why = "not the two-launch vector route of a menu density";
    else if (variant_fn(s, variant) == nullptr) why = "no instance for this move, row type or geometry";
    else if (s->h_loc != (int64_t)s->grid * variant_walkers_per_wg(s, kVarGeneric) || s->h_loc % variant_walkers_per_wg(s, variant) != 0) why = "grid not full";
    else if (credits && !s->d_msum) why = "moments off";
    else if (credits && (s->d_chain || s->d_chain_logp || s->d_chain_blob)) why = "chain on";
    if (why_not) *why_not = why;
    return why == nullptr;
}

// A replay runs a specialised variant only when every generation of it qualifies: all of them counted, or all of them burn-in.  (The replay that
// straddles nburnin runs the generic kernel, and so do burn-in replays without the shared-draws instance.)
int spec_of_chunk(const kmc_sampler* s, int64_t g0, int64_t n)
{
    if (g0 >= s->cfg.nburnin) return spec_variant_possible(s, kVarCredit) ? kVarCredit : kVarGeneric;
    if (g0 + n <= s->cfg.nburnin && spec_variant_possible(s, kVarShareBurnin)) return kVarShareBurnin;
    return kVarGeneric;
}

bool updated_graph_possible(const kmc_sampler* s)
{
    if (s->p2p || s->host_eval || s->islands || s->resident || s->comm || s->updated_refused) return false;
    if (s->temper) return false;            // (a tempered sampler replays the table graph: the sweep node's work changes per generation -- DESIGN.md 4d)
    if (s->fused) return s->user ? s->uk.generation != nullptr : s->generation_kernel != nullptr;      // (one node per generation: the generation among the preloaded parameters)
    return s->user ? (s->plan.vec && s->uk.vec != nullptr) : s->plan.fn != nullptr;
}

kmc_status ensure_updated_graph(kmc_sampler* s)
{
    if (s->uexec[kVarGeneric][0]) return KMC_OK;
    // every variant this sampler can need, now: instantiating one at its first use would fall into a run's steady state
    for (int v = 0; v < kUVariants; ++v) {
        if (!spec_variant_possible(s, v)) continue;
        HIP_TRY(hipGraphCreate(&s->ugraph[v], 0));
        s->unodes[v].assign((size_t)(launches_per_generation(s) * s->uchunk), nullptr);
        hipGraphNode_t prev = nullptr;
        KMC_TRY(for_each_node(s, v, 0, [&](int64_t k, const hipKernelNodeParams& np) -> kmc_status {
            hipGraphNode_t node = nullptr;
            HIP_TRY(hipGraphAddKernelNode(&node, s->ugraph[v], prev ? &prev : nullptr, prev ? 1 : 0, &np));
            s->unodes[v][(size_t)k] = node;
            prev = node;
            return KMC_OK;
        }));
        for (int i = 0; i < kUExec; ++i) HIP_TRY(hipGraphInstantiate(&s->uexec[v][i], s->ugraph[v], nullptr, nullptr, 0));
    }
    for (int i = 0; i < kUExec; ++i) HIP_TRY(hipEventCreateWithFlags(&s->udone[i], hipEventDisableTiming));
    return KMC_OK;
}

// hipGraphExecKernelNodeSetParams keeps host memory inside the runtime, per call and for good (kmc_sampler_run: launch modes): ~80 bytes in the HIP 7.0 runtime (the one
// PyTorch's wheel bundles and a Python process therefore runs on), ~1.4 bytes in 7.2 (/opt/rocm of this image; scripts/probes/updated_graph_rss.py, profiles/r05_updated_graph_rss.txt).
// A process-wide budget of such calls -- 64 MiB worth by default, priced by the runtime this process actually loaded.
namespace {
double update_bytes_each()
{
    static const double b = [] {
        int v = 0;
        return (hipRuntimeGetVersion(&v) == hipSuccess && v >= 70200000) ? 2.0 : 80.0;
    }();
    return b;
}
std::atomic<int64_t> g_update_calls{0};
std::atomic<int64_t>& update_budget()
{
    static std::atomic<int64_t> budget{[] {
        double mb = 64.0;
        std::string v;
        if (debug_opt("updated-budget-mb", &v) && !v.empty()) mb = std::atof(v.c_str());
        return (int64_t)(mb * 1048576.0 / update_bytes_each());
    }()};
    return budget;
}
}  // namespace

// room for one more replay of this sampler (a parameter update per node)?  A replay that would overshoot the budget is not started.
bool update_budget_left(const kmc_sampler* s)
{
    return g_update_calls.load(std::memory_order_relaxed) + launches_per_generation(s) * s->uchunk <= update_budget().load(std::memory_order_relaxed);
}

void note_budget_spent(kmc_sampler* s)
{
    s->budget_fallback = true;
    static std::atomic<bool> said{false};
    if (!said.exchange(true))
        std::fprintf(stderr, "[kissmcmc_hip] the updated-graph launch mode has used up this process's budget (%lld parameter updates, "
                             "kmc_set_updated_budget_mb / KMC_DEBUG=updated-budget-mb=n; this HIP runtime keeps ~%.0f B per update): samplers now "
                             "choose between the table graph and eager launches (up to ~9 %% slower per half-step; results are identical)\n",
                     (long long)g_update_calls.load(std::memory_order_relaxed), update_bytes_each());
}

// one replay of s->uchunk generations starting at s->generation.  *launched tells a failure BEFORE the replay was
// enqueued (nothing ran: the caller may issue these generations another way) from one after it (they are running).
kmc_status launch_updated_graph(kmc_sampler* s, bool* launched)
{
    *launched = false;
    KMC_TRY(ensure_updated_graph(s));
    g_update_calls.fetch_add(launches_per_generation(s) * s->uchunk, std::memory_order_relaxed);
    const int i = s->unext;
    // (slot i's event covers whichever variant took that turn; a variant's executable i last ran in an earlier turn of slot i: done as well)
    int v = spec_of_chunk(s, s->generation, s->uchunk);
    if (!s->uexec[v][i]) v = kVarGeneric;                   // (KMC_DEBUG=spec changed after the graphs were built)
    const auto t_wait0 = std::chrono::steady_clock::now();
    if (s->uinflight[i]) { HIP_TRY(hipEventSynchronize(s->udone[i])); s->uinflight[i] = false; }
    const auto t_upd0 = std::chrono::steady_clock::now();
    KMC_TRY(for_each_node(s, v, s->generation, [&](int64_t k, const hipKernelNodeParams& np) -> kmc_status {
        HIP_TRY(hipGraphExecKernelNodeSetParams(s->uexec[v][i], s->unodes[v][(size_t)k], &np));
        return KMC_OK;
    }));
    const auto t_upd1 = std::chrono::steady_clock::now();
    HIP_TRY(hipGraphLaunch(s->uexec[v][i], s->stream));
    const auto t_launch1 = std::chrono::steady_clock::now();
    // where the feeding thread's time goes (kmc_sampler_describe with KMC_DEBUG=feed-stats): waiting for a free executable = the GPU is
    // the bottleneck; updating + launching = the host's own cost per replay, which must stay below the replay's GPU time
    s->feed_wait_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(t_upd0 - t_wait0).count();
    s->feed_update_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(t_upd1 - t_upd0).count();
    s->feed_launch_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(t_launch1 - t_upd1).count();
    s->feed_replays += 1;
    *launched = true;
    HIP_TRY(hipEventRecord(s->udone[i], s->stream));
    s->uinflight[i] = true;
    s->unext = (i + 1) % kUExec;
    return KMC_OK;
}

}  // namespace kmc_host

KMC_EXPORT void kmc_updated_budget(int64_t* calls_used, int64_t* calls_budget)
{
    if (calls_used) *calls_used = g_update_calls.load(std::memory_order_relaxed);
    if (calls_budget) *calls_budget = update_budget().load(std::memory_order_relaxed);
}

KMC_EXPORT void kmc_set_updated_budget_mb(double mb)
{
    update_budget().store(mb <= 0.0 ? 0 : (int64_t)(mb * 1048576.0 / update_bytes_each()), std::memory_order_relaxed);
}
