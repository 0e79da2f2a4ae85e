// kmc_host.hpp -- what the host-side translation units of the library share (kmc_sampler.hip and its siblings, kmc_validate.hip among them: samplers;
// kmc_metropolis_api.hip: many-chain Metropolis; kmc_acorr.hip: autocorrelation diagnostics).  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/kissmcmc_hip.h"
#include "kmc_tables.hpp"

#define KMC_EXPORT extern "C" __attribute__((visibility("default")))

namespace kmc_host {

// message of the last failure on the calling thread (kmc_last_error; both in kmc_sampler.hip)
extern thread_local std::string g_err;
inline kmc_status fail(kmc_status st, const std::string& msg)
{
    g_err = msg;
    return st;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            (void)hipGetLastError();                                                           \
            return ::kmc_host::fail(e_ == hipErrorOutOfMemory ? KMC_ERR_OOM : KMC_ERR_HIP,     \
                                    std::string(#expr) + ": " + hipGetErrorString(e_));        \
        }                                                                                      \
    } while (0)

#define KMC_TRY(expr)                                                                          \
    do {                                                                                       \
        kmc_status s_ = (expr);                                                                \
        if (s_ != KMC_OK) return s_;                                                           \
    } while (0)

// KMC_DEBUG="opt[=value],opt,...": the test-only, A/B and diagnostic switches of the library behind ONE environment variable (the
// documented ones are in README.md; none is needed in normal use).  Read anew at every call (tests set it between samplers).
// Returns whether `name` is listed; *value gets what follows its '=' ("" when nothing does).
inline bool debug_opt(const char* name, std::string* value = nullptr)
{
    const char* e = std::getenv("KMC_DEBUG");
    if (!e) return false;
    const size_t n = std::strlen(name);
    for (const char* p = e; *p;) {
        const char* q = std::strchr(p, ',');
        const size_t len = q ? (size_t)(q - p) : std::strlen(p);
        if (len >= n && std::strncmp(p, name, n) == 0 && (len == n || p[n] == '=')) {
            if (value) *value = len > n ? std::string(p + n + 1, len - n - 1) : std::string();
            return true;
        }
        if (!q) break;
        p = q + 1;
    }
    return false;
}
inline long debug_opt_long(const char* name, long absent)
{
    std::string v;
    return debug_opt(name, &v) && !v.empty() ? std::atol(v.c_str()) : absent;
}

// The menu densities: f(D{}) with the density type D of a menu density id (its kernels: kmc_tables.hpp), `none` for any other id.
template <class R, class F>
R with_density(int density, R none, F&& f)
{
    switch (density) {
    case KMC_GAUSSIAN_ISO: return f(kmc::GaussianIso{});
    case KMC_EXPONENTIAL: return f(kmc::Exponential{});
    case KMC_ROSENBROCK: return f(kmc::Rosenbrock{});
    case KMC_LOGNORMAL: return f(kmc::LogNormal{});
    case KMC_MVNORMAL2: return f(kmc::MvNormal2{});
    default: return none;
    }
}
// kernel tables of the menu densities (kmc_plan.hip; false / nullptr for any other id), their row-length rules and the digest of
// kmc_config.params the kernels take
bool lookup(int density, int L, int K, int iter, bool p2p, bool ragged, bool f32, kmc::HalfStepFn* vec, kmc::HalfStepFn* gen);
// KMC_MOVE_DE: gamma0 as the kernels use it (kmc_config.de_gamma0, or 2.38 / sqrt(2 ndim) when that is 0)
inline double de_gamma0_of(const kmc_config& c) { return c.de_gamma0 > 0.0 ? c.de_gamma0 : 2.38 / std::sqrt(2.0 * (double)c.ndim); }
inline double de_gamma0_of(double gamma0, int64_t ndim) { return gamma0 > 0.0 ? gamma0 : 2.38 / std::sqrt(2.0 * (double)ndim); }
// KMC_MOVE_SNOOKER: gamma as the kernels use it (0 -> 1.7)
inline double snooker_gamma_of(double gamma) { return gamma > 0.0 ? gamma : 1.7; }
// a move with its own stream and the two-launch kernels only (DE, snooker, their mixtures)
inline bool own_stream_move(const kmc_config& c) { return c.move != KMC_MOVE_STRETCH; }
// parallel tempering (kmc_config.ntemps >= 2): a ladder of ensembles in one launch, the two-launch kernels only
inline bool tempered(const kmc_config& c) { return c.ntemps >= 2; }
inline bool two_launch_only(const kmc_config& c) { return own_stream_move(c) || tempered(c); }
inline const char* move_name(int move) { return move == KMC_MOVE_DE ? "KMC_MOVE_DE" : move == KMC_MOVE_SNOOKER ? "KMC_MOVE_SNOOKER" : move == KMC_MOVE_MIX ? "KMC_MOVE_MIX" : "KMC_MOVE_STRETCH"; }
// KMC_MOVE_MIX: the table the mixture kernels read -- weights normalised in double, in member order (weights_out[i], optional), cumulated
// in the same order; the last member's cumulative weight and every one beyond is 2.0 (it catches rounding)
static_assert(kmc::kMoveIdDE == KMC_MOVE_DE && kmc::kMoveIdSnooker == KMC_MOVE_SNOOKER, "the mixture table carries kmc_config's move ids");
inline kmc::MixTable mix_table_of(const kmc_config& c, double* weights_out = nullptr)
{
    kmc::MixTable t{};
    t.count = c.mix_count;
    double sum = 0.0, cum = 0.0;
    for (int i = 0; i < c.mix_count; ++i) sum += c.mix_weight[i];
    for (int i = 0; i < KMC_MIX_MAX; ++i) {
        t.cum[i] = 2.0;
        if (i >= c.mix_count) continue;
        const double w = c.mix_weight[i] / sum;
        cum += w;
        if (weights_out) weights_out[i] = w;
        if (i < c.mix_count - 1) t.cum[i] = cum;
        t.move[i] = c.mix_move[i];
        t.c0[i] = c.mix_move[i] == KMC_MOVE_DE ? de_gamma0_of(c.mix_gamma[i], c.ndim) : snooker_gamma_of(c.mix_gamma[i]);
        t.c1[i] = c.mix_move[i] == KMC_MOVE_DE ? c.mix_sigma[i] : 0.0;
    }
    return t;
}
// the kernels of KMC_MOVE_DE (PART 3), KMC_MOVE_SNOOKER (4) and KMC_MOVE_MIX (5)
bool lookup_move(int move, int density, int L, int K, int iter, bool ragged, kmc::HalfStepFn* vec, kmc::HalfStepFn* gen);
// ... and their tempered forms (kmc_tables.hpp: temper_part), for any of the four moves
bool lookup_temper(int move, int density, int L, int K, int iter, bool ragged, kmc::HalfStepFn* vec, kmc::HalfStepFn* gen);
kmc::LogpdfFn logpdf_fn(int density);
kmc_status check_ndim(int density, int64_t ndim);
kmc_status digest_params(const kmc_config& c, kmc::DensityParams* dp);

// runtime-compiled user densities (hiprtc)
// Blocking copies / fills WITHOUT the legacy (null) stream: hipMemcpy, hipMemset and hipDeviceSynchronize go through it, and
// a legacy-stream operation issued while ANOTHER host thread captures a hipGraph fails ("would make the legacy stream depend
// on a capturing stream") and invalidates that capture.  Everything here runs on a stream the caller names and waits for it.
//
// And WITHOUT handing pageable host memory to an asynchronous copy: for those the runtime page-locks the caller's pages itself
// and keeps the mapping in a cache -- read-only when the memory was a copy's source.  A later device-to-host copy into a
// heap block that malloc placed on the same pages then died with "Memory access fault by GPU ... Write access to a read-only
// page" (intermittent, layout-dependent; found by running the tests in another order).  copy_sync stages pageable memory
// through page-locked bounce buffers of its own (two, so that the host memcpy of one chunk overlaps the DMA of the next); host
// memory that IS page-locked (hipHostMalloc, hipHostRegister) goes straight through.
hipError_t copy_sync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t st);
// (no 2-D variant on purpose: padded rows are repacked on the host or compacted on the device, then copied contiguously)
inline hipError_t fill_sync(void* dst, int value, size_t bytes, hipStream_t st)
{
    const hipError_t e = hipMemsetAsync(dst, value, bytes, st);
    return e != hipSuccess ? e : hipStreamSynchronize(st);
}
// A large allocation that cannot fit is refused BEFORE hipMalloc is asked: after a failed allocation of hundreds of GB the
// runtime aborted the process a few calls later (observed with a 336 GB chain: 4 of 5 runs).
inline kmc_status check_device_room(size_t need, const char* what)
{
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (need > free_b)
        return fail(KMC_ERR_OOM, std::string(what) + " needs " + std::to_string(need >> 20) + " MiB of device memory, " + std::to_string(free_b >> 20) + " MiB are free");
    return KMC_OK;
}
// The free bytes of the current device and whether `need` fits them, for the calls that refuse in their own words, with their own status
// and margin.  A double: the need is a sum of products of sizes, formed before any of them is known to fit an integer.
inline kmc_status device_fits(double need, bool* fits, size_t* free_b)
{
    size_t total_b = 0;
    HIP_TRY(hipMemGetInfo(free_b, &total_b));
    *fits = !(need > (double)*free_b);
    return KMC_OK;
}
// a number in a message, by the printf format of the message's family ("%g", "%.17g")
inline std::string num(double v, const char* fmt)
{
    char buf[40];
    std::snprintf(buf, sizeof buf, fmt, v);
    return buf;
}
// a private non-blocking stream for the duration of one call
struct ScopedStream {
    hipStream_t st = nullptr;
    hipStream_t borrowed = nullptr;      // ... or a stream the caller owns and has drained: synchronised at the end, not destroyed
    hipError_t create() { return hipStreamCreateWithFlags(&st, hipStreamNonBlocking); }
    hipStream_t get() const { return st ? st : borrowed; }
    ~ScopedStream()
    {
        if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
        else if (borrowed) (void)hipStreamSynchronize(borrowed);
    }
};
// N events around the stages of one call, for its info: created only when info is asked for, read after the stream has passed them
template <int N>
struct TimedEvents {
    hipEvent_t e[N] = {};
    hipError_t create()
    {
        for (auto& x : e) { const hipError_t r = hipEventCreate(&x); if (r != hipSuccess) return r; }
        return hipSuccess;
    }
    hipError_t elapsed_ns(int i, int j, int64_t* ns) const
    {
        float ms = 0.f;
        const hipError_t r = hipEventElapsedTime(&ms, e[i], e[j]);
        *ns = (int64_t)((double)ms * 1e6);
        return r;
    }
    ~TimedEvents() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
};
// a hipMalloc block for the duration of one call: freed with the scope, so the stream that uses it is synchronised before the scope ends
struct ScopedDeviceBlock {
    void* p = nullptr;
    ScopedDeviceBlock() = default;
    ScopedDeviceBlock(const ScopedDeviceBlock&) = delete;
    ScopedDeviceBlock& operator=(const ScopedDeviceBlock&) = delete;
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
    template <class T> T* as() const { return static_cast<T*>(p); }
    ~ScopedDeviceBlock() { if (p) (void)hipFree(p); }
};

// hiprtc compilation of `text` (+ named headers) for gfx950, with a DISK CACHE of the code objects: a script that defines its
// density in source pays the compiler (0.2-0.5 s per density and kernel geometry) once, not in every process.  Key: two
// 64-bit hashes over the program, every header, the options and the hiprtc version; directory $KMC_CACHE_DIR, else
// $XDG_CACHE_HOME/kissmcmc_hip, else $HOME/.cache/kissmcmc_hip; KMC_CACHE_DIR=off switches it off; a cache that cannot be
// read or written is simply not used.  On a compile error *log holds the compiler's messages.
kmc_status rtc_compile_cached(const std::string& text, const char* program_name, int nheaders, const char* const* header_text,
                              const char* const* header_names, int nopts, const char* const* opts, std::vector<char>* code, std::string* log);

// One runtime-compiled module of a density: what rtc_compile_cached hashes into the cache file's name besides the text -- the program
// name, the headers in this order, the options in this order -- so none of it changes without recompiling everyone's cache.
struct RtcModule {
    const char* what;                        // "user density" / "data density", for the messages
    const char* program_name;
    std::vector<const char*> headers;        // file names in the header directory (user_header_dir)
    std::vector<const char*> options;
};
inline std::vector<const char*> rtc_options(bool kernarg_preload = false)     // (the preload: the sampler modules' half-step kernels only, kmc_kernels.hpp)
{
    std::vector<const char*> o = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off"};
    if (kernarg_preload) o.insert(o.end(), {"-mllvm", "-amdgpu-kernarg-preload-count=14"});
    return o;
}
// The code object under `key` in ud->code; on a miss: the headers read, `text` asked for the program (a failure of its own is passed on),
// rtc_compile_cached, the compiler's messages worded for `m.what`.  The one compile path of every runtime-compiled module (kmc_rtc.hip).
kmc_status compile_keyed(kmc_user_density* ud, const std::string& key, const RtcModule& m, const std::function<kmc_status(std::string*)>& text,
                         const std::vector<char>** out);
// ... and the one load path: the module of a code object on the current device, shared per (density, code object, device) by everything
// that runs it; unloaded when the last holder -- the density or one of those -- lets go of `keep`
kmc_status shared_module(kmc_user_density* ud, const std::vector<char>* code, std::shared_ptr<void>* keep);

kmc_status download_by_walker(const void* src_dev, bool is_float, int64_t nl, int64_t ld, int64_t width, int64_t K, double* dst_host, hipStream_t st);
std::string user_functor_source(const kmc_user_density* ud);      // the functor(s) ...
std::string user_density_alias(const kmc_user_density* ud, int64_t ndim);   // ... and "using UD = ...;" over them
std::string user_header_dir();                      // where the kernel headers live (KMC_CSRC_DIR or <library dir>/csrc)
std::string read_file(const std::string& path);

template <class Args>
hipError_t launch_module(hipFunction_t f, unsigned grid, unsigned tpb, hipStream_t st, const Args& args, unsigned lds_bytes = 0)
{
    Args copy = args;
    size_t size = sizeof(Args);
    void* extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &copy, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
    return hipModuleLaunchKernel(f, grid, 1, 1, tpb, 1, 1, lds_bytes, st, nullptr, extra);
}
// ... with a second grid dimension (the rungs of a tempered sampler)
template <class Args>
hipError_t launch_module_y(hipFunction_t f, unsigned grid, unsigned grid_y, unsigned tpb, hipStream_t st, const Args& args, unsigned lds_bytes = 0)
{
    Args copy = args;
    size_t size = sizeof(Args);
    void* extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &copy, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
    return hipModuleLaunchKernel(f, grid, grid_y, 1, tpb, 1, 1, lds_bytes, st, nullptr, extra);
}

// Small device allocations, cached per device (kmc_diag.hip).  A sampler of the reference's own size lives for a millisecond or
// two, and hipMalloc / hipFree of its dozen buffers were more than half of that (create 0.35 ms, destroy 0.85 ms of a 1.7 ms
// README call): blocks of up to 8 MiB go back to a free list instead (at most 128 MiB held per device, exact rounded sizes, so
// samplers of one shape reuse each other's blocks).  A block is handed back only after its owner has synchronised the streams that
// touched it (kmc_sampler_destroy: its own streams; the whole device when a caller's stream was ever bound or the sampler is a shard).  Off with KMC_DEBUG=poison (guard bands); kmc_device_cache_release() returns everything.
hipError_t cache_alloc(void** p, size_t bytes);        // on the current device
void cache_free(void* p);                              // nullptr is fine; pointers the cache did not hand out go to hipFree
size_t cache_held_bytes(int device);

// integrated autocorrelation time of a device-resident chain [nsamples][nwalkers][ndim] (kmc_acorr.hip)
kmc_status int_acorr_check(int64_t nsamples, int64_t nwalkers, int64_t ndim, double c, const double* tau, const double* converged);
kmc_status int_acorr_device(const double* chain_dev, int64_t nsamples, int64_t nwalkers, int64_t ndim, double c, double* tau, double* converged);

// RCCL, loaded on demand (kmc_rccl.hip)
kmc_status rccl_version(int* version, const char** path);
kmc_status rccl_unique_id(void* id_out);
kmc_status rccl_comm_create(const void* id_bytes, int rank, int nranks, void** comm_out);
void rccl_comm_destroy(void* comm);
kmc_status rccl_all_gather_f64(void* comm, const double* send, double* recv, size_t count, hipStream_t stream);

}  // namespace kmc_host

// The opaque handle of kmc_user_density_create: the two expressions and the code objects compiled from them so far.
struct kmc_user_density {
    std::string term, pair;
    bool has_pair = false;
    std::string body;                                // kmc_user_density_create_body: the whole function body instead of term / pair
    bool is_body = false;
    int nblob = 0;                                   // kmc_user_density_create_body_blob: doubles the body writes to blob[] per evaluation
    std::string grad_body;                           // kmc_user_density_set_grad: the body of its gradient (the HMC step; under `mu`)
    // A body of the form  `double s = 0; for (int i = 0; i < n; ++i) s += f(x[i]);  return g(s);`  (optionally with the neighbour
    // x[i + 1] and the bound i + 1 < n) is a sum over elements: kmc_user_density_create_body recognises it (kmc_rtc.hip:
    // recognise_separable) and the samplers then run it in the lane-striped vector kernels like a term / pair density, with g as
    // the finish.  Everything else about the density (initial log-pdfs, resident kernels, Metropolis) keeps evaluating the body.
    bool sep = false;
    bool sep_pair = false;                           // the loop reads x[i + 1] / runs to n - 1: its body is the PAIR function
    int sep_nacc = 1;                                // sums the loop feeds (1: SepDensity; 2..4: SepDensityN)
    std::string sep_functor;                         // "struct UserS { term, pair, finish };" generated from the body
    // The recogniser reads TEXT; before a sampler runs the generated form it is evaluated next to the body itself on test points
    // (kmc_sampler.hip: check_sum_form) -- once per (ndim, parameter values): what agrees at one row length and one parameter set says
    // nothing about another.  sep_case: 1 they agree there; 3 no test point had a finite value there (nothing was shown: THAT sampler runs the
    // body as written, the density keeps its routing for other cases).  A case where the two DISAGREE refutes the recogniser: `sep` is
    // cleared for good (sep_note says why) and every later sampler evaluates the body per walker, as written.
    std::map<std::pair<int64_t, uint64_t>, int> sep_case;    // (ndim, digest of the parameter values) -> verdict; under `mu`
    std::mutex check_mu;                             // held by the sampler that finds out (plan, load, check): others over the same density wait
    std::string sep_note;                            // why not (describe())
    std::mutex mu;
    std::map<std::string, std::vector<char>> code;   // geometry key -> gfx950 code object
    // ... and the modules loaded from them, per device: shared by every sampler over this density (hipModuleLoadData is ~0.5 ms,
    // half of what a sampler of the reference's sizes lives); unloaded when the last holder -- this object or a sampler -- lets go
    std::map<std::pair<const void*, int>, std::shared_ptr<void>> modules;
    // kmc_data_density_create (KMC_DATA_DENSITY): two function bodies and the observations, copied at creation (kmc_data.hip)
    bool is_data = false;
    std::string data_term, data_prior;
    int64_t ndata = 0;
    int32_t ncols = 0;
    std::vector<double> data;                        // [ndata][ncols], the caller's array as it was at creation
    std::map<int, std::shared_ptr<void>> data_dev;   // ... and its copy on each device it was used on (under `mu`)
};
// Is the body run in its per-element form BY THE SAMPLER BEING BUILT on this thread?  The density's own flag, unless that sampler's check was blind
// (kmc_sampler_create holds a SepOff for the rest of its set-up; afterwards the sampler's own `sep_off` says it).
inline thread_local bool g_sep_off = false;
struct SepOff { bool prev; explicit SepOff(bool off) : prev(g_sep_off) { if (off) g_sep_off = true; } ~SepOff() { g_sep_off = prev; } };
inline bool sep_routed(const kmc_user_density* ud) { return ud && ud->sep && !g_sep_off; }
