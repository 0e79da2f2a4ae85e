// kmc_validate.hip -- which configurations the `emcee` sampler takes (the reference's asserts, src/samplers.jl:200-205, and what this
// library's features add to them): kmc_validate and kmc_status_string.  Host code only; no device is touched.
// kmc_validate derives a few Facts from the kmc_config once and runs one check per feature over them, in a fixed order: the first refusal
// wins, so the order is part of the interface (tests/test_validate_matrix_cpu.py pins status and message of some 4600 configurations).
// What a feature cannot run with is one named mask of traits next to its message: the compatibility matrix of DESIGN.md, section 1a.
#include <cmath>

#include "kmc_sampler.hpp"

using namespace kmc;
using namespace kmc_host;

KMC_EXPORT const char* kmc_status_string(kmc_status st)
{
    switch (st) {
    case KMC_OK: return "ok";
    case KMC_ERR_A_SCALE: return "a_scale must be > 1";
    case KMC_ERR_ODD_WALKERS: return "Use an even number of walkers.";
    case KMC_ERR_TOO_FEW_WALKERS: return "Use more walkers: at least DOF+2, but better many more.";
    case KMC_ERR_BAD_ARG: return "bad argument";
    case KMC_ERR_NONFINITE_LOGP: return "initial walker with non-finite log-pdf";
    case KMC_ERR_HIP: return "HIP runtime error";
    case KMC_ERR_OOM: return "out of device memory";
    case KMC_ERR_NO_DEVICE: return "no HIP device";
    case KMC_ERR_UNSUPPORTED: return "unsupported configuration";
    }
    return "unknown status";
}

namespace {
// The traits of a configuration that some feature cannot run with, and the words a refusal names them with.  The order of the bits is
// the order in which first_trait names them.
enum Trait : unsigned {
    kIslands = 1u << 0, kP2P = 1u << 1, kSharded = 1u << 2, kDealt = 1u << 3, kFloatRows = 1u << 4,
    kStoreBlobs = 1u << 5, kBlobDensity = 1u << 6, kStreamChain = 1u << 7, kHostDensity = 1u << 8,
};
constexpr const char* kTraitName[] = {"KMC_ISLANDS", "KMC_P2P", "shard_count > 1", "dealt sub-ensembles (deal_count > 0)", "KMC_F32",
                                      "KMC_STORE_BLOBS", "a density with blobs", "KMC_STREAM_CHAIN", "KMC_HOST_DENSITY"};

struct Facts {
    unsigned traits = 0;
    int P = 1;             // the shard count (kmc_config.shard_count, 0 and below: 1)
    int nblob = 0;         // doubles per blob of a runtime-compiled density, 0: none (or no handle)
    bool like = false;     // temper_mode == KMC_TEMPER_LIKELIHOOD
};
Facts facts_of(const kmc_config& c)
{
    Facts f;
    f.P = c.shard_count <= 0 ? 1 : c.shard_count;
    f.nblob = c.density == KMC_USER_DENSITY && c.user_density ? static_cast<const kmc_user_density*>(c.user_density)->nblob : 0;
    f.like = c.temper_mode == KMC_TEMPER_LIKELIHOOD;
    f.traits = (c.flags & KMC_ISLANDS ? kIslands : 0) | (c.flags & KMC_P2P ? kP2P : 0) | (f.P > 1 ? kSharded : 0) | (c.deal_count > 0 ? kDealt : 0) |
               (c.dtype != KMC_F64 ? kFloatRows : 0) |      // (any dtype but KMC_F64: check_row_type lets KMC_F32 alone through)
               (c.flags & KMC_STORE_BLOBS ? kStoreBlobs : 0) | (f.nblob > 0 ? kBlobDensity : 0) | (c.flags & KMC_STREAM_CHAIN ? kStreamChain : 0) |
               (c.density == KMC_HOST_DENSITY ? kHostDensity : 0);
    return f;
}
// the name of the first trait of `excluded` that the configuration has, nullptr: none
const char* first_trait(const Facts& f, unsigned excluded)
{
    const unsigned hit = f.traits & excluded;
    return hit ? kTraitName[__builtin_ctz(hit)] : nullptr;
}

// What each feature cannot run with.  (KMC_ISLANDS also refuses chain storage, which is no trait: check_islands.)
constexpr unsigned kOffOneGpu = kP2P | kIslands | kSharded;      // one GPU, one ensemble in global memory
constexpr unsigned kNotWithHostDensity = kOffOneGpu;
constexpr unsigned kNotWithFloatRows = kOffOneGpu;               // ... and kHostDensity, in a sentence of its own
constexpr unsigned kNotWithIslands = kSharded | kP2P;
constexpr unsigned kNotWithStreamChain = kFloatRows | kOffOneGpu;
constexpr unsigned kNotWithBlobDensity = kFloatRows | kOffOneGpu | kDealt | kStreamChain;
constexpr unsigned kNotWithDealt = kOffOneGpu | kStreamChain | kFloatRows | kHostDensity;
// The own-stream moves and the tempered ladder run the two-launch kernels on one GPU with double rows (the ladder: and a device density)
constexpr unsigned kNotOnOneGpuWithDoubleRows = kOffOneGpu | kDealt | kFloatRows | kStoreBlobs | kBlobDensity;
// KMC_DATA_DENSITY says each in its own words, in this order
constexpr struct { unsigned trait; const char* message; } kNotWithDataDensity[] = {
    {kFloatRows, "KMC_DATA_DENSITY: double rows only (no KMC_F32)"},
    {kIslands, "KMC_DATA_DENSITY: no island mode (KMC_ISLANDS)"},
    {kP2P, "KMC_DATA_DENSITY: one GPU, no KMC_P2P"},
    {kSharded, "KMC_DATA_DENSITY: one GPU, no sharding (shard_count must be 1)"},
    {kDealt, "KMC_DATA_DENSITY: no dealt sub-ensembles (deal_count must be 0)"},
    {kStoreBlobs, "KMC_DATA_DENSITY: no blobs (KMC_STORE_BLOBS)"},
};

// src/samplers.jl:200-205
kmc_status check_sizes(const kmc_config& c, const Facts&)
{
    if (c.nwalkers <= 0 || c.ndim <= 0 || c.nthin <= 0 || c.ngenerations < 0 || c.nburnin < 0)
        return fail(KMC_ERR_BAD_ARG, "nwalkers, ndim, nthin must be > 0 and ngenerations, nburnin >= 0");
    if (!(c.a_scale > 1.0)) return fail(KMC_ERR_A_SCALE, kmc_status_string(KMC_ERR_A_SCALE));
    if (c.nwalkers % 2 != 0) return fail(KMC_ERR_ODD_WALKERS, kmc_status_string(KMC_ERR_ODD_WALKERS));
    if (c.nwalkers < c.ndim + 2) return fail(KMC_ERR_TOO_FEW_WALKERS, kmc_status_string(KMC_ERR_TOO_FEW_WALKERS));
    if (c.nwalkers >= (int64_t)1 << 31 || c.ndim >= (int64_t)1 << 24)
        return fail(KMC_ERR_UNSUPPORTED, "ensemble too large");
    if (c.ngenerations >= (int64_t)1 << 31) return fail(KMC_ERR_UNSUPPORTED, "at most 2^31 - 1 generations (the step index is 32 bits)");
    return KMC_OK;
}

// the handle (or callback) behind a density that has one, and what a data / host density cannot run with
kmc_status check_density_handle(const kmc_config& c, const Facts& f)
{
    const kmc_user_density* ud = static_cast<const kmc_user_density*>(c.user_density);
    if (c.density == KMC_USER_DENSITY && !ud) return fail(KMC_ERR_BAD_ARG, "KMC_USER_DENSITY needs kmc_config.user_density");
    if (c.density == KMC_USER_DENSITY && ud->is_data)
        return fail(KMC_ERR_BAD_ARG, "this handle was made by kmc_data_density_create: use density = KMC_DATA_DENSITY");
    if (c.density == KMC_DATA_DENSITY) {
        if (!ud || !ud->is_data) return fail(KMC_ERR_BAD_ARG, "KMC_DATA_DENSITY needs kmc_config.user_density made by kmc_data_density_create");
        for (const auto& row : kNotWithDataDensity)
            if (f.traits & row.trait) return fail(KMC_ERR_UNSUPPORTED, row.message);
        if (c.ndim > kDataMaxDim) return fail(KMC_ERR_UNSUPPORTED, "KMC_DATA_DENSITY: ndim must be <= " + std::to_string(kDataMaxDim));
    }
    if (c.density == KMC_HOST_DENSITY) {
        if (!c.host_logpdf) return fail(KMC_ERR_BAD_ARG, "KMC_HOST_DENSITY needs kmc_config.host_logpdf");
        if (first_trait(f, kNotWithHostDensity)) return fail(KMC_ERR_UNSUPPORTED, "KMC_HOST_DENSITY runs on one GPU, without KMC_P2P / KMC_ISLANDS / sharding");
    }
    return KMC_OK;
}

kmc_status check_row_type(const kmc_config& c, const Facts& f)
{
    if (c.dtype != KMC_F64 && c.dtype != KMC_F32) return fail(KMC_ERR_UNSUPPORTED, "dtype must be KMC_F64 or KMC_F32");
    if (c.dtype == KMC_F32) {
        if (first_trait(f, kNotWithFloatRows)) return fail(KMC_ERR_UNSUPPORTED, "KMC_F32 rows: one GPU, without KMC_P2P / KMC_ISLANDS / sharding");
        if (first_trait(f, kHostDensity))
            return fail(KMC_ERR_UNSUPPORTED, "KMC_F32 rows: densities evaluated on the device only (built-in or runtime-compiled)");
    }
    return KMC_OK;
}

// what only one kind of density takes: the accept callback, a menu density's row length
kmc_status check_density_arguments(const kmc_config& c, const Facts&)
{
    if (c.host_accepted && c.density != KMC_HOST_DENSITY) return fail(KMC_ERR_BAD_ARG, "kmc_config.host_accepted needs KMC_HOST_DENSITY");
    return check_ndim(c.density, c.ndim);
}

kmc_status check_shards(const kmc_config& c, const Facts& f)
{
    if (c.shard_rank < 0 || c.shard_rank >= f.P) return fail(KMC_ERR_BAD_ARG, "shard_rank out of range");
    if ((c.nwalkers / 2) % f.P != 0) return fail(KMC_ERR_BAD_ARG, "nwalkers/2 must be divisible by shard_count");
    if ((c.flags & KMC_P2P) && f.P > 8) return fail(KMC_ERR_UNSUPPORTED, "KMC_P2P supports at most 8 shards (one node)");
    if (c.flags & ((1u << 8) | (1u << 10)))                 // (KMC_P2P_FOLD_SIGNAL, KMC_P2P_LAZY of rounds 1-4)
        return fail(KMC_ERR_UNSUPPORTED, "the lazy-pull and folded-signal exchange variants were removed in round 5 (they read peer-written memory through the local L2 and could "
                                         "not move the fabric bound): the exchanges are the pull of drawn rows and the push of accepted rows (KMC_P2P_PUSH), both read with "
                                         "system-scope loads");
    if ((c.flags & KMC_P2P_PUSH) && !(c.flags & KMC_P2P)) return fail(KMC_ERR_BAD_ARG, "KMC_P2P_PUSH needs KMC_P2P");
    return KMC_OK;
}

kmc_status check_islands(const kmc_config& c, const Facts& f)
{
    if (!(c.flags & KMC_ISLANDS)) return KMC_OK;
    const int64_t S = c.island_size > 0 ? c.island_size : kIslandSizeDefault;
    if ((S != 64 && S != 128 && S != 256) || c.nwalkers % S != 0 || c.ndim > 32 || c.ndim + 2 > S || first_trait(f, kNotWithIslands) ||
        (c.flags & (KMC_STORE_CHAIN | KMC_STORE_LOGP)) || c.island_gens < 0)
        return fail(KMC_ERR_UNSUPPORTED, "KMC_ISLANDS needs island_size in {64,128,256} >= ndim+2 dividing nwalkers, ndim <= 32, one shard and no chain storage");
    if (c.density == KMC_USER_DENSITY && (size_t)S * (size_t)(2 * c.ndim + 9) * sizeof(double) > kResidentLdsMax)
        return fail(KMC_ERR_UNSUPPORTED, "KMC_ISLANDS with a user density: island_size * (2 ndim + 9) * 8 must stay below 156 KiB");
    return KMC_OK;
}

kmc_status check_stream_chain(const kmc_config& c, const Facts& f)
{
    if (!(c.flags & KMC_STREAM_CHAIN)) return KMC_OK;
    if (!(c.flags & (KMC_STORE_CHAIN | KMC_STORE_LOGP))) return fail(KMC_ERR_BAD_ARG, "KMC_STREAM_CHAIN needs KMC_STORE_CHAIN and / or KMC_STORE_LOGP");
    if (first_trait(f, kNotWithStreamChain)) return fail(KMC_ERR_UNSUPPORTED, "KMC_STREAM_CHAIN: KMC_F64, one GPU, without KMC_P2P / KMC_ISLANDS / sharding");
    return KMC_OK;
}

// KMC_MOVE_DE and KMC_MOVE_SNOOKER, alone (`name`: the move) or as a member of a mixture (`name`: KMC_MOVE_MIX)
kmc_status check_de(const std::string& name, double gamma0, double sigma)
{
    if (!std::isfinite(gamma0) || gamma0 < 0.0) return fail(KMC_ERR_BAD_ARG, name + ": de_gamma0 must be finite and >= 0 (0: 2.38 / sqrt(2 ndim))");
    if (!std::isfinite(sigma) || sigma < 0.0 || sigma >= 1.0) return fail(KMC_ERR_BAD_ARG, name + ": de_sigma must be in [0, 1)");
    return KMC_OK;
}
kmc_status check_snooker(const std::string& name, const kmc_config& c, double gamma)
{
    if (!std::isfinite(gamma) || gamma < 0.0) return fail(KMC_ERR_BAD_ARG, name + ": snooker_gamma must be finite and >= 0 (0: 1.7)");
    if (c.ndim < 2) return fail(KMC_ERR_BAD_ARG, name + ": the snooker move needs ndim >= 2 (it is degenerate in one dimension)");
    if (c.nwalkers < 6) return fail(KMC_ERR_BAD_ARG, name + ": the snooker move needs nwalkers >= 6 (three distinct partners in a half)");
    return KMC_OK;
}
kmc_status check_mixture(const std::string& name, const kmc_config& c)
{
    if (c.mix_count < 2 || c.mix_count > KMC_MIX_MAX) return fail(KMC_ERR_BAD_ARG, "KMC_MOVE_MIX: mix_count must be 2 .. 4");
    for (int i = 0; i < c.mix_count; ++i) {
        if (c.mix_move[i] == KMC_MOVE_STRETCH)
            return fail(KMC_ERR_UNSUPPORTED, "KMC_MOVE_MIX: a stretch member is not supported yet (members are KMC_MOVE_DE and KMC_MOVE_SNOOKER; DESIGN.md section 8)");
        if (c.mix_move[i] != KMC_MOVE_DE && c.mix_move[i] != KMC_MOVE_SNOOKER) return fail(KMC_ERR_BAD_ARG, "KMC_MOVE_MIX: a member must be KMC_MOVE_DE or KMC_MOVE_SNOOKER");
        if (!std::isfinite(c.mix_weight[i]) || !(c.mix_weight[i] > 0.0)) return fail(KMC_ERR_BAD_ARG, "KMC_MOVE_MIX: weights must be finite and > 0");
        if (c.mix_move[i] == KMC_MOVE_DE) KMC_TRY(check_de(name, c.mix_gamma[i], c.mix_sigma[i]));
        else KMC_TRY(check_snooker(name, c, c.mix_gamma[i]));
    }
    double sum = 0.0;
    for (int i = 0; i < c.mix_count; ++i) sum += c.mix_weight[i];
    if (!std::isfinite(sum)) return fail(KMC_ERR_BAD_ARG, "KMC_MOVE_MIX: the weights' sum must be finite");
    return KMC_OK;
}
kmc_status check_move(const kmc_config& c, const Facts& f)
{
    if (c.move != KMC_MOVE_STRETCH && c.move != KMC_MOVE_DE && c.move != KMC_MOVE_SNOOKER && c.move != KMC_MOVE_MIX)
        return fail(KMC_ERR_BAD_ARG, "kmc_config.move must be KMC_MOVE_STRETCH, KMC_MOVE_DE, KMC_MOVE_SNOOKER or KMC_MOVE_MIX");
    if (c.move == KMC_MOVE_STRETCH) return KMC_OK;
    const std::string name = move_name(c.move);
    if (c.move == KMC_MOVE_DE) KMC_TRY(check_de(name, c.de_gamma0, c.de_sigma));
    if (c.move == KMC_MOVE_SNOOKER) KMC_TRY(check_snooker(name, c, c.snooker_gamma));
    if (c.move == KMC_MOVE_MIX) KMC_TRY(check_mixture(name, c));
    if (const char* what = first_trait(f, kNotOnOneGpuWithDoubleRows)) return fail(KMC_ERR_UNSUPPORTED, name + ": two launches per generation on one GPU with double rows -- not with " + what);
    return KMC_OK;
}

kmc_status check_blobs(const kmc_config& c, const Facts& f)
{
    if ((c.flags & KMC_STORE_BLOBS) && f.nblob == 0)
        return fail(KMC_ERR_BAD_ARG, "KMC_STORE_BLOBS needs a body density with blobs (kmc_user_density_create_body_blob)");
    if (f.nblob > 0 && first_trait(f, kNotWithBlobDensity))
        return fail(KMC_ERR_UNSUPPORTED, "a density with blobs: KMC_F64, one GPU, without KMC_P2P / KMC_ISLANDS / KMC_STREAM_CHAIN / sharding / dealt sub-ensembles");
    return KMC_OK;
}

kmc_status check_tempering(const kmc_config& c, const Facts& f)
{
    if (c.ntemps < 0) return fail(KMC_ERR_BAD_ARG, "parallel tempering: ntemps must be >= 0 (0 or 1: off)");
    if (c.swap_every < 0) return fail(KMC_ERR_BAD_ARG, "parallel tempering: swap_every must be >= 0 (0: never)");
    if (c.temper_mode != KMC_TEMPER_WHOLE && c.temper_mode != KMC_TEMPER_LIKELIHOOD)
        return fail(KMC_ERR_BAD_ARG, "parallel tempering: temper_mode must be KMC_TEMPER_WHOLE or KMC_TEMPER_LIKELIHOOD");
    if (f.like && c.ntemps < 2) return fail(KMC_ERR_BAD_ARG, "parallel tempering: KMC_TEMPER_LIKELIHOOD needs a ladder (ntemps >= 2)");
    if (c.ntemps < 2) return KMC_OK;
    if (c.ntemps > KMC_TEMPS_MAX) return fail(KMC_ERR_BAD_ARG, "parallel tempering: ntemps must be 2 .. " + std::to_string(KMC_TEMPS_MAX));
    if (!c.betas) return fail(KMC_ERR_BAD_ARG, "parallel tempering: betas must point to ntemps inverse temperatures");
    if (c.betas[0] != 1.0) return fail(KMC_ERR_BAD_ARG, "parallel tempering: betas[0] must be 1");
    for (int t = 0; t < c.ntemps; ++t) {
        const bool prior_rung = f.like && t == c.ntemps - 1 && c.betas[t] == 0.0;      // (the rung that samples the prior closes the thermodynamic integral)
        if (!std::isfinite(c.betas[t]) || !(c.betas[t] > 0.0 || prior_rung))
            return fail(KMC_ERR_BAD_ARG, f.like ? "parallel tempering: betas must be finite and > 0 (KMC_TEMPER_LIKELIHOOD: the last one may be 0)" : "parallel tempering: betas must be finite and > 0");
        if (t > 0 && !(c.betas[t] < c.betas[t - 1])) return fail(KMC_ERR_BAD_ARG, "parallel tempering: betas must be strictly decreasing");
    }
    if ((int64_t)c.ntemps * c.nwalkers >= (int64_t)1 << 31) return fail(KMC_ERR_BAD_ARG, "parallel tempering: ntemps * nwalkers must stay below 2^31");
    if (f.like && c.density != KMC_DATA_DENSITY)
        return fail(KMC_ERR_UNSUPPORTED, "parallel tempering: KMC_TEMPER_LIKELIHOOD needs KMC_DATA_DENSITY (prior + beta * S): nothing says where another density's prior ends");
    const char* what = first_trait(f, kHostDensity);
    if (!what && c.density == KMC_DATA_DENSITY && !f.like)
        what = "KMC_DATA_DENSITY in the default temper_mode (temper_mode = KMC_TEMPER_LIKELIHOOD, temper=\"likelihood\", tempers its likelihood)";
    if (!what) what = first_trait(f, kNotOnOneGpuWithDoubleRows);
    if (what) return fail(KMC_ERR_UNSUPPORTED, std::string("parallel tempering (ntemps >= 2): a ladder of ensembles on one GPU with double rows and a device density -- not with ") + what);
    return KMC_OK;
}

kmc_status check_adaptive_ladder(const kmc_config& c, const Facts&)
{
    if (c.adapt == 0) return KMC_OK;
    if (c.adapt != 1) return fail(KMC_ERR_BAD_ARG, "adaptive ladder: adapt must be 0 or 1");
    if (c.ntemps < 2) return fail(KMC_ERR_BAD_ARG, "adaptive ladder: adapt needs a ladder (parallel tempering: betas, ntemps)");
    if (c.ntemps < 3) return fail(KMC_ERR_BAD_ARG, "adaptive ladder: ntemps must be >= 3 (the first and the last rung never move)");
    if (c.swap_every == 0) return fail(KMC_ERR_BAD_ARG, "adaptive ladder: swap_every must be >= 1 (the ladder adapts to the swap sweeps' acceptance)");
    if (c.adapt_until < 0 || c.adapt_until > c.nburnin)
        return fail(KMC_ERR_BAD_ARG, "adaptive ladder: adapt_until must be 0 .. nburnin (0: nburnin) -- every stored sample comes from the frozen ladder");
    if (!std::isfinite(c.adapt_lag) || !(c.adapt_lag > 0.0)) return fail(KMC_ERR_BAD_ARG, "adaptive ladder: adapt_lag must be finite and > 0");
    if (!std::isfinite(c.adapt_time) || !(c.adapt_time > 0.0)) return fail(KMC_ERR_BAD_ARG, "adaptive ladder: adapt_time must be finite and > 0");
    return KMC_OK;
}

kmc_status check_dealt(const kmc_config& c, const Facts& f)
{
    if (c.deal_count < 0 || (c.deal_count > 0 && (c.deal_rank < 0 || c.deal_rank >= c.deal_count)))
        return fail(KMC_ERR_BAD_ARG, "deal_rank / deal_count out of range");
    if (c.deal_count == 0) return KMC_OK;
    // (a stored chain is by SLOT: which walker a slot held when a sample was taken follows from kmc_deal_perm, distributed.py)
    if (first_trait(f, kNotWithDealt))
        return fail(KMC_ERR_UNSUPPORTED, "dealt sub-ensembles: KMC_F64, a device density, one shard, no KMC_P2P / KMC_ISLANDS / KMC_STREAM_CHAIN");
    if (c.nwalkers % c.deal_count != 0)
        return fail(KMC_ERR_BAD_ARG, "dealt sub-ensembles: nwalkers (this sub-ensemble's size) must be divisible by deal_count");
    if (c.nwalkers * (int64_t)c.deal_count >= (int64_t)1 << 32) return fail(KMC_ERR_UNSUPPORTED, "dealt sub-ensembles: at most 2^32 - 1 walkers in all");
    return KMC_OK;
}
}  // namespace

KMC_EXPORT kmc_status kmc_validate(const kmc_config* cfg)
{
    if (!cfg) return fail(KMC_ERR_BAD_ARG, "null config");
    const kmc_config& c = *cfg;
    const Facts f = facts_of(c);
    KMC_TRY(check_sizes(c, f));
    KMC_TRY(check_density_handle(c, f));
    KMC_TRY(check_row_type(c, f));
    KMC_TRY(check_density_arguments(c, f));
    KMC_TRY(check_shards(c, f));
    KMC_TRY(check_islands(c, f));
    KMC_TRY(check_stream_chain(c, f));
    KMC_TRY(check_move(c, f));
    KMC_TRY(check_blobs(c, f));
    KMC_TRY(check_tempering(c, f));
    KMC_TRY(check_adaptive_ladder(c, f));
    KMC_TRY(check_dealt(c, f));
    DensityParams dp;
    return digest_params(c, &dp);
}
