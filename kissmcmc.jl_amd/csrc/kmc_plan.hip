// kmc_plan.hip -- which kernel, in which geometry, for a configuration: the dispatch of a menu density id to its kernel tables
// (kmc_tables.hpp), the launch plan per ndim (lanes per row, chunks per lane, walkers per wave), the parameter digest the
// kernels read, and the island / dealt permutations.  The sampler's lifecycle that uses them is kmc_sampler.hip.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "kmc_sampler.hpp"

using namespace kmc;
using namespace kmc_host;

namespace kmc_host {
// Which part of a density's kernels serves a configuration (kmc_tables.hpp); there are no P2P kernels for KMC_F32 rows.
bool lookup(int density, int L, int K, int iter, bool p2p, bool ragged, bool f32, HalfStepFn* vec, HalfStepFn* gen)
{
    return with_density(density, false, [&](auto d) {
        using D = decltype(d);
        if (p2p && f32) { *vec = nullptr; *gen = nullptr; }
        else if (p2p) density_part<D, 2>(L, K, iter, ragged, false, vec, gen);
        else if (ragged || f32) density_part<D, 1>(L, K, iter, ragged, f32, vec, gen);
        else density_part<D, 0>(L, K, iter, false, false, vec, gen);
        return true;
    });
}

// KMC_MOVE_DE: the differential-evolution kernels (PART 3); KMC_MOVE_SNOOKER: PART 4; KMC_MOVE_MIX: PART 5
bool lookup_move(int move, int density, int L, int K, int iter, bool ragged, HalfStepFn* vec, HalfStepFn* gen)
{
    return with_density(density, false, [&](auto d) {
        if (move == KMC_MOVE_SNOOKER) density_part<decltype(d), 4>(L, K, iter, ragged, false, vec, gen);
        else if (move == KMC_MOVE_MIX) density_part<decltype(d), 5>(L, K, iter, ragged, false, vec, gen);
        else density_part<decltype(d), 3>(L, K, iter, ragged, false, vec, gen);
        return true;
    });
}

// parallel tempering: the tempered form of the move's kernels
bool lookup_temper(int move, int density, int L, int K, int iter, bool ragged, HalfStepFn* vec, HalfStepFn* gen)
{
    return with_density(density, false, [&](auto d) {
        using D = decltype(d);
        if (move == KMC_MOVE_SNOOKER) temper_part<D, Move::Snooker>(L, K, iter, ragged, vec, gen);
        else if (move == KMC_MOVE_MIX) temper_part<D, Move::Mix>(L, K, iter, ragged, vec, gen);
        else if (move == KMC_MOVE_DE) temper_part<D, Move::DE>(L, K, iter, ragged, vec, gen);
        else temper_part<D, Move::Stretch>(L, K, iter, ragged, vec, gen);
        return true;
    });
}

// the phase-specialised instance of PART 0's vector kernel for this geometry (kmc_tables.hpp: spec_part)
HalfStepFn lookup_spec(int density, int L, int K, int iter)
{
    return with_density(density, HalfStepFn(nullptr), [&](auto d) { return spec_part<decltype(d)>(L, K, iter); });
}

// ... and its workgroup-shared-draws instance for burn-in (kmc_tables.hpp: share_part)
HalfStepFn lookup_share(int density, int L, int K, int iter, int* share)
{
    *share = 0;
    return with_density(density, HalfStepFn(nullptr), [&](auto d) -> HalfStepFn {
        if constexpr (std::is_same<decltype(d), MvNormal2>::value) return nullptr;      // (two-dimensional rows: one lane per walker, nothing to share -- no unit)
        else return share_part<decltype(d)>(L, K, iter, share);
    });
}

LogpdfFn logpdf_fn(int density)
{
    return with_density(density, LogpdfFn(nullptr), [](auto d) { return logpdf_lookup<decltype(d)>(); });
}

// resident mode with one walker per thread (short rows) or two lanes per walker: KMC_DEBUG=resident=pair decides for tests
bool resident_lane_wanted(int64_t ndim)
{
    std::string e;
    if (debug_opt("resident", &e) && e == "pair") return false;
    return ndim <= 8;
}
int lane_nd(int64_t ndim) { return (int)ndim; }          // (the lane kernels are instantiated for the exact row length)

// Philox4x32-10 on the host (only for the island deal; Salmon et al., SC'11).
void philox_host(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4])
{
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// The affine permutation s -> (A*s + C) mod n of one Philox draw (ctr, key = seed): C uniform, A made coprime to n by
// stepping upwards (wrapping to 1) from a draw in [1, n).
static void affine_perm(const uint32_t ctr[4], uint64_t seed, int64_t n, int64_t* A, int64_t* C)
{
    const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    uint32_t w[4];
    philox_host(ctr, key, w);
    auto gcd = [](int64_t a, int64_t b) { while (b) { const int64_t t = a % b; a = b; b = t; } return a; };
    int64_t a = (int64_t)((((uint64_t)w[0] << 32) | w[1]) % (uint64_t)n);
    if (a < 1) a = 1;
    while (gcd(a, n) != 1) a = (a + 1 >= n) ? 1 : a + 1;
    *A = a;
    *C = (int64_t)((((uint64_t)w[2] << 32) | w[3]) % (uint64_t)n);
}

// The deal of epoch e: slot s holds walker (A*s + C) mod N.  Epoch 0 is the identity; later epochs
// take (A, C) from Philox(ctr = {e, "ISLA", 0}, key = seed).
void island_perm(uint64_t seed, int64_t epoch, int64_t N, int64_t* A, int64_t* C)
{
    if (epoch == 0 || N <= 2) { *A = 1; *C = 0; return; }
    const uint32_t ctr[4] = {(uint32_t)epoch, (uint32_t)((uint64_t)epoch >> 32), 0x49534c41u, 0u};
    affine_perm(ctr, seed, N, A, C);
}

// Dealt sub-ensembles (kmc_config.deal_count): the Philox key of sub-ensemble r, and the affine shuffle (A, C) its S
// slots go through before the deal of `epoch` (A coprime to S) -- from Philox(ctr = {epoch, "DEAL", r}, key = seed).
constexpr uint64_t kDealSeedStride = 0x9E3779B97F4A7C15ull;
uint64_t deal_seed(uint64_t seed, int32_t rank) { return seed + (uint64_t)(rank + 1) * kDealSeedStride; }
void deal_perm(uint64_t seed, int64_t epoch, int32_t rank, int64_t S, int64_t* A, int64_t* C)
{
    const uint32_t ctr[4] = {(uint32_t)epoch, (uint32_t)((uint64_t)epoch >> 32), 0x4445414cu, (uint32_t)rank};
    affine_perm(ctr, seed, S, A, C);
}

// Default geometry per ndim; KMC_PLAN="L,K,ITER" (or "generic") overrides for tuning.
Plan make_plan(const kmc_config& c, int64_t n_active)
{
    Plan p;
    HalfStepFn vec = nullptr, gen = nullptr;
    int L = 0, K = 0, iter = 1;
    const char* env = std::getenv("KMC_PLAN");
    bool force_generic = false;
    if (env && std::strcmp(env, "generic") == 0) force_generic = true;
    else if (env && std::sscanf(env, "%d,%d,%d", &L, &K, &iter) == 3) { /* forced */ }
    else {
        L = 0;
        // a row = ceil(ndim/2) 16-byte chunks, striped over L lanes x K chunks (2*L*K >= ndim; the
        // ragged tail is masked).  Measured on MI355X (scripts/quick_bench.py): 4 lanes x 2 chunks
        // per 64 B of row is the sweet spot.
        const int64_t chunks = (c.ndim + 1) / 2;
        auto pow2ceil = [](int64_t v) { int p = 1; while (p < v) p <<= 1; return p; };
        if (chunks <= 4) { L = pow2ceil(chunks); K = 1; }
        else if (chunks <= 128) { L = pow2ceil((chunks + 1) / 2); K = 2; }
        else if (chunks <= 256) { L = 64; K = 4; }
        else if (chunks <= 512) { L = 64; K = 8; }
        if (c.density == KMC_USER_DENSITY && chunks > 64 && chunks <= 128) {
            // a function body evaluated once per walker (RowEvalTrait) on rows of 129 ... 256 doubles: one lane walks the whole row, so the walkers per wave
            // count -- 16 lanes x 8 chunks (4 walkers per wave) instead of 64 x 2 (one): 16 384 x 256 30.1 -> 22.7 us per half-step, 4 096 x 256 22.1 -> 16.0, 2 048 x 256
            // 16.9 -> 13.7, 8 192 x 200 26.2 -> 24.7 (profiles/NOTES.md round 5; shorter and longer rows measured no better that way)
            const kmc_user_density* ud = static_cast<const kmc_user_density*>(c.user_density);
            if (ud && ud->is_body && !sep_routed(ud) && body_vec_possible(ud, c.ndim)) { L = 16; K = 8; }
        }
        // walkers per group (ITER): two amortise the per-walker scalar work (Philox, two logs) over
        // the wave -- once that still leaves 1.5 waves per SIMD (measured: 2048 single-walker waves run 3-6 % faster
        // as they are, C3 and 32 768 x 32; 3072 and more are faster paired); more only while the grid keeps >= 4096
        // waves (large ensembles)
        iter = 1;
        if (L > 0) {
            const int64_t waves1 = n_active * L / 64;
            if (2 <= L && 2 * K <= 16 && waves1 >= 3072) iter = 2;
            while (iter >= 2 && iter * 2 <= L && iter * 2 * K <= 16 && waves1 / (iter * 2) >= 4096 && iter < 16) iter *= 2;
        }
    }
    const bool de = own_stream_move(c);
    // (a DE kernel holds three row tiles -- own, two partners -- where the stretch kernel holds two: at most 8 chunks per lane each;
    //  a snooker or mixture kernel holds four -- at most 4 chunks each, 64 of its VGPRs, so that the two sums' butterflies and the
    //  density still fit 128 VGPRs: four waves per SIMD, as DE has them at 8)
    const int tile_cap = c.move == KMC_MOVE_DE ? 8 : 4;
    if (de && (!env || c.move != KMC_MOVE_DE)) while (iter > 1 && iter * K > tile_cap) iter /= 2;
    const bool ragged = L > 0 && 2 * L * K != c.ndim;
    const bool f32 = c.dtype == KMC_F32;
    if ((ragged || f32) && iter > 4) iter = 4;
    if (tempered(c) && iter > 8) iter = 8;                  // (the tempered tables: kmc_tables.hpp, temper_iter)
    if ((c.flags & KMC_P2P) && iter > 8) iter = 8;
    p.ragged = ragged;
    if (c.density == KMC_HOST_DENSITY || c.density == KMC_DATA_DENSITY) {
        // bound by the host callback (or, for a data density, by the data kernels between the two passes): the one-walker-per-lane kernel, any ndim
        p.fn = c.move == KMC_MOVE_MIX ? half_step_host_mix() : c.move == KMC_MOVE_SNOOKER ? half_step_host_snooker() : de ? half_step_host_de() : half_step_host(); p.vec = false; p.ragged = false; p.L = 1; p.K = 1; p.ITER = 1;
        if (tempered(c)) {                                  // (a likelihood-tempered data density: kmc_inst_host_temper*.hip)
            if (c.move == KMC_MOVE_SNOOKER) temper_part<HostEval, Move::Snooker>(1, 1, 1, false, &vec, &p.fn);
            else if (c.move == KMC_MOVE_MIX) temper_part<HostEval, Move::Mix>(1, 1, 1, false, &vec, &p.fn);
            else if (c.move == KMC_MOVE_DE) temper_part<HostEval, Move::DE>(1, 1, 1, false, &vec, &p.fn);
            else temper_part<HostEval, Move::Stretch>(1, 1, 1, false, &vec, &p.fn);
        }
        return p;
    }
    if (c.density == KMC_USER_DENSITY) {
        // kernels are compiled for exactly this geometry when the sampler is created
        const kmc_user_density* ud = static_cast<const kmc_user_density*>(c.user_density);
        // a function body in the vector kernel: lane-striped like term / pair when it was recognised as a sum over elements, else
        // with its rows lane-striped and only the evaluation per walker (RowEvalTrait); KMC_DEBUG=no-body-routing / no-body-vec
        // keep it one walker per lane (ensembles small enough for the resident kernels: decided by the caller)
        const bool body = ud && ud->is_body && !(sep_routed(ud) || body_vec_possible(ud, c.ndim));
        if (!body && !force_generic && L > 0 && 2 * L * K >= c.ndim && iter <= L && iter * K <= 16) {
            // (a body evaluated per walker keeps a tile of the wave's proposals in LDS: at most 64 KiB per workgroup)
            if (ud && ud->is_body && !sep_routed(ud)) while (iter > 1 && body_vec_lds_bytes(L, K, iter) > 65536) iter /= 2;
            p.vec = true; p.L = L; p.K = K; p.ITER = iter;
        } else {
            p.vec = false; p.L = 1; p.K = 1; p.ITER = 1;
        }
        return p;
    }
    if (tempered(c)) lookup_temper(c.move, c.density, L, K, iter, ragged, &vec, &gen);
    else if (de) lookup_move(c.move, c.density, L, K, iter, ragged, &vec, &gen);
    else lookup(c.density, L, K, iter, (c.flags & KMC_P2P) != 0, ragged, f32, &vec, &gen);
    if (!force_generic && L > 0 && 2 * L * K >= c.ndim && vec != nullptr) {
        p.fn = vec; p.vec = true; p.L = L; p.K = K; p.ITER = iter;
        // the stretch move on one GPU, double rows of exact size, one or two walkers per group: PART 0's kernel has a phase-specialised instance
        if (!tempered(c) && !de && !(c.flags & KMC_P2P) && !ragged && !f32 && iter <= 2) {
            p.fn_credit = lookup_spec(c.density, L, K, iter);
            p.fn_share_burnin = lookup_share(c.density, L, K, iter, &p.share_burnin);
        }
    } else {
        p.fn = gen; p.vec = false; p.L = 1; p.K = 1; p.ITER = 1;
    }
    return p;
}

// the menu densities' row lengths (kmc_validate, kmc_metropolis_validate)
kmc_status check_ndim(int density, int64_t ndim)
{
    if (density == KMC_ROSENBROCK && ndim < 2) return fail(KMC_ERR_BAD_ARG, "rosenbrock needs ndim >= 2");
    if (density == KMC_MVNORMAL2 && ndim != 2) return fail(KMC_ERR_BAD_ARG, "mvnormal2 needs ndim == 2");
    return KMC_OK;
}

}  // namespace kmc_host
kmc_status kmc_host::digest_params(const kmc_config& c, DensityParams* dp)
{
    for (double& v : dp->p) v = 0.0;
    dp->ndim = (int32_t)c.ndim;
    dp->pad_ = 0;
    const double* p = c.params;
    switch (c.density) {
    case KMC_USER_DENSITY:
        if (!c.user_density) return fail(KMC_ERR_BAD_ARG, "KMC_USER_DENSITY needs kmc_config.user_density");
        for (int i = 0; i < 6; ++i) dp->p[i] = p[i];
        return KMC_OK;
    case KMC_HOST_DENSITY:
        return KMC_OK;
    case KMC_DATA_DENSITY:
        if (!c.user_density) return fail(KMC_ERR_BAD_ARG, "KMC_DATA_DENSITY needs kmc_config.user_density");
        for (int i = 0; i < 6; ++i) dp->p[i] = p[i];
        return KMC_OK;
    case KMC_GAUSSIAN_ISO:
        if (!(p[1] > 0.0)) return fail(KMC_ERR_BAD_ARG, "gaussian: sigma must be > 0");
        dp->p[0] = p[0]; dp->p[1] = 1.0 / p[1];
        return KMC_OK;
    case KMC_EXPONENTIAL:
        if (!(p[0] > 0.0)) return fail(KMC_ERR_BAD_ARG, "exponential: rate must be > 0");
        dp->p[0] = p[0];
        return KMC_OK;
    case KMC_ROSENBROCK:
        if (!(p[2] > 0.0)) return fail(KMC_ERR_BAD_ARG, "rosenbrock: scale must be > 0");
        dp->p[0] = p[0]; dp->p[1] = p[1]; dp->p[2] = 1.0 / p[2];
        return KMC_OK;
    case KMC_LOGNORMAL:
        if (!(p[1] > 0.0)) return fail(KMC_ERR_BAD_ARG, "lognormal: sigma must be > 0");
        dp->p[0] = p[0]; dp->p[1] = p[1];
        return KMC_OK;
    case KMC_MVNORMAL2:
        for (int i = 0; i < 5; ++i) dp->p[i] = p[i];
        return KMC_OK;
    default:
        return fail(KMC_ERR_BAD_ARG, "unknown density id");
    }
}

KMC_EXPORT int kmc_debug_phase_spec(int density, int L, int K, int iter)
{
    return kmc_host::lookup_spec(density, L, K, iter) != nullptr ? 1 : 0;
}

// waves per workgroup of the shared-draws instance (burn-in replays) for this geometry, 0: none
KMC_EXPORT int kmc_debug_shared_draws(int density, int L, int K, int iter)
{
    int share = 0;
    return kmc_host::lookup_share(density, L, K, iter, &share) != nullptr ? share : 0;
}
