// kmc_tables.hpp -- kernel instantiation tables.  The lookup templates below map a launch geometry to a kernel of density D.
// Every translation unit sees their declarations.  Only the kmc_inst_<density>*.hip files define KMC_TABLES_IMPL: they see the
// definitions and instantiate them explicitly for their density (KMC_INSTANTIATE_*).  So the host driver names them without
// instantiating a kernel, and the build compiles a density's kernels in parallel, six translation units per density:
//   kmc_inst_<density>.hip       density_part PART 0: double rows of exact size, one GPU (incl. the tuning geometries); the
//                                log-pdf and initial-ball kernels
//   kmc_inst_<density>_var.hip   density_part PART 1: ragged sizes and KMC_F32 rows, one GPU
//   kmc_inst_<density>_p2p.hip   density_part PART 2: the peer-to-peer kernels (KMC_P2P)
//   kmc_inst_<density>_de.hip    density_part PART 3: the differential-evolution move (KMC_MOVE_DE: exact and ragged double rows, one GPU)
//   kmc_inst_<density>_snooker.hip  density_part PART 4 and 5: the snooker move (KMC_MOVE_SNOOKER) and the DE / snooker mixtures (KMC_MOVE_MIX), as PART 3
//   kmc_inst_<density>_temper.hip          temper_part: the tempered kernels (parallel tempering, the rung as blockIdx.y) of the stretch and DE moves
//   kmc_inst_<density>_temper_snooker.hip  temper_part of the snooker move and the mixtures (exact and ragged double rows, one GPU, like PART 3 .. 5)
//   kmc_inst_host_temper*.hip    temper_part of the host-evaluated density: likelihood tempering of a data density (generic kernels only)
//   kmc_inst_<density>_spec.hip  spec_part: the phase-specialised instance (Spec::Credit) of PART 0's vector kernels, planner geometries with ITER <= 2
//   kmc_inst_<density>_share.hip share_part: the workgroup-shared-draws instance for burn-in (kmc_shared_draws.hpp) of the geometry it serves
//   kmc_inst_<density>_lds.hip   the LDS-resident (islands, resident mode), one-launch-per-generation and many-chain Metropolis kernels
// Which part serves a configuration is decided on the host (kmc_plan.hip: lookup, lookup_move).
#pragma once
#include <type_traits>
#include "kmc_islands.hpp"
#include "kmc_generation.hpp"
#include "kmc_metropolis.hpp"

namespace kmc {

using HalfStepFn = void (*)(KMC_FRONT_TYPES, const HalfStepArgs);
using LogpdfFn = void (*)(const LogpdfArgs);
using FlushFn = void (*)(const FlushArgs);
using IslandFn = void (*)(const IslandArgs);
using ResidentFn = void (*)(const ResidentArgs);
using GenerationFn = void (*)(KMC_GEN_FRONT_TYPES, const GenerationArgs);
using InitBallFn = void (*)(const InitBallArgs);
using MetropolisFn = void (*)(const MetropolisArgs);
using MetropolisTabledFn = void (*)(const MetropolisArgs, const double*, int);

// (the part's vector kernel for this geometry or nullptr, its generic kernel)
template <class D, int PART> void density_part(int L, int K, int iter, bool ragged, bool f32, HalfStepFn* vec, HalfStepFn* gen);
template <class D, Move M> void temper_part(int L, int K, int iter, bool ragged, HalfStepFn* vec, HalfStepFn* gen);
// (the credit instance of half_step_vec<D, L, K, iter, false, false, double>, nullptr where there is none)
template <class D> HalfStepFn spec_part(int L, int K, int iter);
// (the workgroup-shared-draws instance of that kernel for burn-in replays and its waves per workgroup, nullptr and 0 where there is none; defined in
//  kmc_shared_draws.hpp)
template <class D> HalfStepFn share_part(int L, int K, int iter, int* share);
template <class D> LogpdfFn logpdf_lookup();
template <class D> InitBallFn init_ball_lookup();
template <class D> IslandFn island_lookup(int S, int K, bool ragged);
template <class D> ResidentFn resident_lookup(int tpb, int K, bool ragged);
template <class D> ResidentFn resident_lane_lookup(int ndim, bool f32);
template <class D> ResidentFn resident_lane2_lookup(int ndim);
template <class D> GenerationFn generation_lane_lookup(int ndim);
template <class D> GenerationFn generation_group_lookup(int L, int K);
template <class D> MetropolisFn metropolis_lookup(int ndim);
template <class D> MetropolisTabledFn metropolis_tabled_lookup(int ndim);
template <class D> MetropolisFn metropolis_mv_lookup(int ndim);    // the proposal theta + L z (MVNormalStep)
HalfStepFn half_step_host();         // kmc_inst_host.hip
HalfStepFn half_step_host_de();      // KMC_MOVE_DE
HalfStepFn half_step_host_snooker(); // KMC_MOVE_SNOOKER
HalfStepFn half_step_host_mix();     // KMC_MOVE_MIX

#ifdef KMC_TABLES_IMPL
template <class D, int L, int K, int ITER, bool P2P, bool RAGGED, class T, Move M>
HalfStepFn vec_one()
{
    // a group's ITER scalar lanes must fit in its L lanes; keep the register tile (ITER*K chunks) bounded
    // (snooker and the mixtures hold four row tiles: the planner keeps ITER * K <= 4 for them, kmc_plan.hip)
    if constexpr (ITER > L || ITER * K > 16 || ((M == Move::Snooker || M == Move::Mix) && ITER > 1 && ITER * K > 4)) return nullptr;
    else if constexpr (M == Move::Snooker) return half_step_snooker_vec<D, L, K, ITER, RAGGED>;
    else if constexpr (M == Move::Mix) return half_step_mix_vec<D, L, K, ITER, RAGGED>;
    else if constexpr (M == Move::DE) return half_step_de_vec<D, L, K, ITER, RAGGED>;
    else return half_step_vec<D, L, K, ITER, P2P, RAGGED, T>;
}

template <class D, int L, int K, bool P2P, bool RAGGED, class T, Move M = Move::Stretch>
HalfStepFn vec_iter(int iter)
{
    // full ITER range only for the single-GPU exact double kernels (tuning, and the DE move); the others: what make_plan picks
    constexpr bool kWide = !P2P && !RAGGED && sizeof(T) == 8;
    switch (iter) {
    case 1: return vec_one<D, L, K, 1, P2P, RAGGED, T, M>();
    case 2: return vec_one<D, L, K, 2, P2P, RAGGED, T, M>();
    case 4: return vec_one<D, L, K, 4, P2P, RAGGED, T, M>();
    case 8: if constexpr (kWide || (P2P && !RAGGED)) return vec_one<D, L, K, 8, P2P, RAGGED, T, M>(); else return nullptr;
    case 16: if constexpr (kWide) return vec_one<D, L, K, 16, P2P, RAGGED, T, M>(); else return nullptr;
    default: return nullptr;
    }
}

// PART 0 .. 5 of density_part (see the top of this file); each part only names -- and therefore only compiles -- its own instantiations
template <class D, int L, int K, int PART>
HalfStepFn vec_pick(int iter, bool ragged, bool f32)
{
    if constexpr (PART == 0) return vec_iter<D, L, K, false, false, double>(iter);
    else if constexpr (PART == 1) {
        if (f32) return ragged ? vec_iter<D, L, K, false, true, float>(iter) : vec_iter<D, L, K, false, false, float>(iter);   // KMC_F32: single rows, one GPU
        return vec_iter<D, L, K, false, true, double>(iter);
    } else if constexpr (PART == 2) return ragged ? vec_iter<D, L, K, true, true, double>(iter) : vec_iter<D, L, K, true, false, double>(iter);
    else if constexpr (PART == 3) return ragged ? vec_iter<D, L, K, false, true, double, Move::DE>(iter) : vec_iter<D, L, K, false, false, double, Move::DE>(iter);
    else if constexpr (PART == 4) return ragged ? vec_iter<D, L, K, false, true, double, Move::Snooker>(iter) : vec_iter<D, L, K, false, false, double, Move::Snooker>(iter);
    else return ragged ? vec_iter<D, L, K, false, true, double, Move::Mix>(iter) : vec_iter<D, L, K, false, false, double, Move::Mix>(iter);
}

// geometries make_plan can pick: exact + ragged, single-GPU + P2P; the extra exact single-GPU ones
// exist for tuning (KMC_PLAN)
template <class D, int PART>
HalfStepFn vec_lookup(int L, int K, int iter, bool ragged, bool f32)
{
    if constexpr (!D::kHasFrag) {
        return nullptr;
    } else {
#define KMC_LK(l, k) if (L == l && K == k) return vec_pick<D, l, k, PART>(iter, ragged, f32);
        KMC_LK(1, 1) KMC_LK(2, 1) KMC_LK(4, 1) KMC_LK(4, 2) KMC_LK(8, 2) KMC_LK(16, 2) KMC_LK(32, 2) KMC_LK(64, 2)
        KMC_LK(64, 4) KMC_LK(64, 8)
#undef KMC_LK
        if constexpr (PART == 0 && std::is_same<D, GaussianIso>::value) {       // (tuning geometries, KMC_PLAN: the bench density only -- build time)
#define KMC_LK(l, k) if (L == l && K == k) return vec_iter<D, l, k, false, false, double>(iter);
            KMC_LK(8, 1) KMC_LK(16, 1) KMC_LK(32, 1) KMC_LK(64, 1) KMC_LK(4, 4) KMC_LK(8, 4)
#undef KMC_LK
        }
        return nullptr;
    }
}

template <class D, int PART>
void density_part(int L, int K, int iter, bool ragged, bool f32, HalfStepFn* vec, HalfStepFn* gen)
{
    *vec = vec_lookup<D, PART>(L, K, iter, ragged, f32);
    if constexpr (PART == 0) *gen = half_step_generic<D, false, double>;
    else if constexpr (PART == 1) *gen = f32 ? half_step_generic<D, false, float> : half_step_generic<D, false, double>;
    else if constexpr (PART == 2) *gen = half_step_generic<D, true, double>;
    else if constexpr (PART == 3) *gen = half_step_de_generic<D>;
    else if constexpr (PART == 4) *gen = half_step_snooker_generic<D>;
    else *gen = half_step_mix_generic<D>;
}

// parallel tempering: the same geometries with the rung as the grid's second dimension
template <class D, int L, int K, int ITER, bool RAGGED, Move M>
HalfStepFn temper_one()
{
    if constexpr (ITER > L || ITER * K > 16 || ((M == Move::Snooker || M == Move::Mix) && ITER > 1 && ITER * K > 4)) return nullptr;
    else return half_step_temper_vec<D, L, K, ITER, RAGGED, M>;
}
template <class D, int L, int K, bool RAGGED, Move M>
HalfStepFn temper_iter(int iter)
{
    switch (iter) {
    case 1: return temper_one<D, L, K, 1, RAGGED, M>();
    case 2: return temper_one<D, L, K, 2, RAGGED, M>();
    case 4: return temper_one<D, L, K, 4, RAGGED, M>();
    case 8: if constexpr (!RAGGED) return temper_one<D, L, K, 8, RAGGED, M>(); else return nullptr;
    default: return nullptr;
    }
}
template <class D, Move M>
void temper_part(int L, int K, int iter, bool ragged, HalfStepFn* vec, HalfStepFn* gen)
{
    *vec = nullptr;
    *gen = half_step_temper_generic<D, M>;
    if constexpr (D::kHasFrag) {
#define KMC_LK(l, k) if (L == l && K == k) *vec = ragged ? temper_iter<D, l, k, true, M>(iter) : temper_iter<D, l, k, false, M>(iter);
        KMC_LK(1, 1) KMC_LK(2, 1) KMC_LK(4, 1) KMC_LK(4, 2) KMC_LK(8, 2) KMC_LK(16, 2) KMC_LK(32, 2) KMC_LK(64, 2)
        KMC_LK(64, 4) KMC_LK(64, 8)
#undef KMC_LK
    }
}

// the phase-specialised instance: the geometries make_plan picks by itself, one or two walkers per group
template <class D, int L, int K, int ITER>
HalfStepFn spec_one()
{
    if constexpr (ITER <= L && ITER * K <= 16) return half_step_vec_spec<D, L, K, ITER, Spec::Credit>;
    else return nullptr;
}
template <class D>
HalfStepFn spec_part(int L, int K, int iter)
{
    if constexpr (D::kHasFrag && BlobTrait<D>::n == 0 && RowEvalTrait<D>::n == 0) {
#define KMC_LK(l, k) if (L == l && K == k) return iter == 1 ? spec_one<D, l, k, 1>() : iter == 2 ? spec_one<D, l, k, 2>() : nullptr;
        KMC_LK(1, 1) KMC_LK(2, 1) KMC_LK(4, 1) KMC_LK(4, 2) KMC_LK(8, 2) KMC_LK(16, 2) KMC_LK(32, 2) KMC_LK(64, 2)
        KMC_LK(64, 4) KMC_LK(64, 8)
#undef KMC_LK
    }
    return nullptr;
}

template <class D>
LogpdfFn logpdf_lookup() { return logpdf_rows<D>; }
template <class D>
InitBallFn init_ball_lookup() { return init_ball<D>; }

// island mode: one workgroup per S-walker island, rows of up to 4*K doubles
template <class D, int S>
IslandFn island_lookup_s(int K, bool ragged)
{
    switch (K) {
    case 1: return ragged ? island_epoch<D, S, 1, true> : island_epoch<D, S, 1, false>;
    case 2: return ragged ? island_epoch<D, S, 2, true> : island_epoch<D, S, 2, false>;
    case 4: return ragged ? island_epoch<D, S, 4, true> : island_epoch<D, S, 4, false>;
    case 8: return ragged ? island_epoch<D, S, 8, true> : island_epoch<D, S, 8, false>;
    default: return nullptr;
    }
}

template <class D>
IslandFn island_lookup(int S, int K, bool ragged)
{
    if constexpr (!D::kHasFrag) {
        return nullptr;
    } else {
        switch (S) {
        case 64: return island_lookup_s<D, 64>(K, ragged);
        case 128: return island_lookup_s<D, 128>(K, ragged);
        case 256: return island_lookup_s<D, 256>(K, ragged);
        default: return nullptr;
        }
    }
}
// resident mode: the exact sampler for ensembles that fit one workgroup's LDS
template <class D, int TPB>
ResidentFn resident_lookup_t(int K, bool ragged)
{
    switch (K) {
    case 1: return ragged ? resident_epoch<D, 1, true, TPB> : resident_epoch<D, 1, false, TPB>;
    case 2: return ragged ? resident_epoch<D, 2, true, TPB> : resident_epoch<D, 2, false, TPB>;
    case 4: return ragged ? resident_epoch<D, 4, true, TPB> : resident_epoch<D, 4, false, TPB>;
    case 8: return ragged ? resident_epoch<D, 8, true, TPB> : resident_epoch<D, 8, false, TPB>;
    default: return nullptr;
    }
}

template <class D>
ResidentFn resident_lookup(int tpb, int K, bool ragged)
{
    if constexpr (!D::kHasFrag) {
        return nullptr;
    } else {
        switch (tpb) {
        case 256: return resident_lookup_t<D, 256>(K, ragged);
        case 512: return resident_lookup_t<D, 512>(K, ragged);
        case 1024: return resident_lookup_t<D, 1024>(K, ragged);
        default: return nullptr;
        }
    }
}
// resident mode, one walker per thread (short rows: ndim <= ND <= 8); double or float rows
template <class D, class T>
ResidentFn resident_lane_lookup_t(int ndim)
{
    switch (ndim) {           // exact row lengths: no per-element guards in the kernel
    case 1: return resident_lane<D, 1, T>;
    case 2: return resident_lane<D, 2, T>;
    case 3: return resident_lane<D, 3, T>;
    case 4: return resident_lane<D, 4, T>;
    case 5: return resident_lane<D, 5, T>;
    case 6: return resident_lane<D, 6, T>;
    case 7: return resident_lane<D, 7, T>;
    case 8: return resident_lane<D, 8, T>;
    default: return nullptr;
    }
}
template <class D>
ResidentFn resident_lane_lookup(int ndim, bool f32)
{
    return f32 ? resident_lane_lookup_t<D, float>(ndim) : resident_lane_lookup_t<D, double>(ndim);
}
// ... two walkers per thread (1026 .. 2048 walkers, double rows)
template <class D>
ResidentFn resident_lane2_lookup(int ndim)
{
    switch (ndim) {
    case 1: return resident_lane2<D, 1>;
    case 2: return resident_lane2<D, 2>;
    case 3: return resident_lane2<D, 3>;
    case 4: return resident_lane2<D, 4>;
    case 5: return resident_lane2<D, 5>;
    case 6: return resident_lane2<D, 6>;
    case 7: return resident_lane2<D, 7>;
    case 8: return resident_lane2<D, 8>;
    default: return nullptr;
    }
}
// one launch per generation, one walker per lane (mid-size ensembles, short double rows: kmc_generation.hpp)
template <class D>
GenerationFn generation_lane_lookup(int ndim)
{
    switch (ndim) {
    case 1: return generation_lane<D, 1>;
    case 2: return generation_lane<D, 2>;
    case 3: return generation_lane<D, 3>;
    case 4: return generation_lane<D, 4>;
    case 5: return generation_lane<D, 5>;
    case 6: return generation_lane<D, 6>;
    case 7: return generation_lane<D, 7>;
    case 8: return generation_lane<D, 8>;
    default: return nullptr;
    }
}
// ... and lane-striped (longer rows of small ensembles): the geometries make_plan picks for the vector kernels
template <class D>
GenerationFn generation_group_lookup(int L, int K)
{
    if constexpr (!D::kHasFrag) {
        return nullptr;
    } else {
#define KMC_LK(l, k) if (L == l && K == k) return generation_group<D, l, k>;
        KMC_LK(1, 1) KMC_LK(2, 1) KMC_LK(4, 1) KMC_LK(4, 2) KMC_LK(8, 2) KMC_LK(16, 2) KMC_LK(32, 2) KMC_LK(64, 2)
        KMC_LK(64, 4) KMC_LK(64, 8)
#undef KMC_LK
        return nullptr;
    }
}
// many-chain Metropolis: the chain in registers up to 32 dimensions, in memory beyond
template <class D>
MetropolisFn metropolis_lookup(int ndim)
{
    if (ndim <= 1) return metropolis_chains<D, 1>;
    if (ndim <= 2) return metropolis_chains<D, 2>;
    if (ndim <= 4) return metropolis_chains<D, 4>;
    if (ndim <= 8) return metropolis_chains<D, 8>;
    if (ndim <= 16) return metropolis_chains<D, 16>;
    if (ndim <= 32) return metropolis_chains<D, 32>;
    return metropolis_chains<D, 0>;
}
// the same geometries with the covariance-shaped proposal (the few-chains route needs none: its table holds L z)
template <class D>
MetropolisFn metropolis_mv_lookup(int ndim)
{
    if (ndim <= 1) return metropolis_chains_mv<D, 1>;
    if (ndim <= 2) return metropolis_chains_mv<D, 2>;
    if (ndim <= 4) return metropolis_chains_mv<D, 4>;
    if (ndim <= 8) return metropolis_chains_mv<D, 8>;
    if (ndim <= 16) return metropolis_chains_mv<D, 16>;
    if (ndim <= 32) return metropolis_chains_mv<D, 32>;
    return metropolis_chains_mv<D, 0>;
}
// few chains: the draws from a table (kmc_metropolis.hpp: metropolis_chains_tabled), chains in registers up to 8 dimensions (menu densities -- build time; runtime-compiled ones up to 32)
template <class D>
MetropolisTabledFn metropolis_tabled_lookup(int ndim)
{
    if (ndim <= 1) return metropolis_chains_tabled<D, 1>;
    if (ndim <= 2) return metropolis_chains_tabled<D, 2>;
    if (ndim <= 4) return metropolis_chains_tabled<D, 4>;
    if (ndim <= 8) return metropolis_chains_tabled<D, 8>;
    return nullptr;
}
// the explicit instantiations of one translation unit of density D (see the top of this file)
#define KMC_INSTANTIATE_PART(D, PART) template void density_part<D, PART>(int, int, int, bool, bool, HalfStepFn*, HalfStepFn*)
#define KMC_INSTANTIATE_TEMPER(D, M) template void temper_part<D, M>(int, int, int, bool, HalfStepFn*, HalfStepFn*)
#define KMC_INSTANTIATE_SPEC(D) template HalfStepFn spec_part<D>(int, int, int)
#define KMC_INSTANTIATE_ROWS(D) \
    template LogpdfFn logpdf_lookup<D>(); \
    template InitBallFn init_ball_lookup<D>()
#define KMC_INSTANTIATE_LDS(D) \
    template IslandFn island_lookup<D>(int, int, bool); \
    template ResidentFn resident_lookup<D>(int, int, bool); \
    template ResidentFn resident_lane_lookup<D>(int, bool); \
    template ResidentFn resident_lane2_lookup<D>(int); \
    template GenerationFn generation_lane_lookup<D>(int); \
    template GenerationFn generation_group_lookup<D>(int, int); \
    template MetropolisFn metropolis_lookup<D>(int); \
    template MetropolisTabledFn metropolis_tabled_lookup<D>(int); \
    template MetropolisFn metropolis_mv_lookup<D>(int)
#endif  // KMC_TABLES_IMPL

}  // namespace kmc
