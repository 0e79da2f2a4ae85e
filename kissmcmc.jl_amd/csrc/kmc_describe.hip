// kmc_describe.hip -- kmc_sampler_describe: how a sampler executes (kernel family, geometry, exchange), in words.  One writer per part of
// the text, appended in a fixed order; tests/test_gpu_create_routes.py pins the whole string for every route under KMC_DEBUG=geometry.
// Host code only: it reads what kmc_sampler_create (kmc_sampler.hip) decided and touches no device.
#include <cstdio>
#include <sstream>

#include "kmc_sampler.hpp"

using namespace kmc;
using namespace kmc_host;

namespace {
// how kmc_sampler_run issues the launches of the multi-launch kernels (two per generation, or one): kmc_launch.hip
std::string launch_mode_text(const kmc_sampler* s, const char* what)
{
    std::string t = ((s->cfg.flags & KMC_NO_GRAPH) || s->launch_mode == 2) ? std::string(", eager launches (") + what + " among the preloaded kernel parameters)"
                    : s->launch_mode == 3 ? ", hipGraph replay of " + std::to_string(s->uchunk) + " generations with per-replay parameter updates (" + what + " preloaded)"
                                          : std::string(", hipGraph replay of 64 generations");
    if (s->calib_graph_ms > 0.f) {
        char b[128];
        std::snprintf(b, sizeof(b), " (measured per 64 generations: table graph %.3f ms, %s %.3f ms)", s->calib_graph_ms, s->launch_mode == 2 ? "eager launches" : "updated graph", s->calib_eager_ms);
        t += b;
    }
    return t;
}

// ---- the route sentence: one writer per route that takes more than a line
void write_islands(std::ostringstream& o, const kmc_sampler* s)
{
    o << "island mode: " << s->nislands << " islands of " << s->island_size << " walkers in LDS, " << s->island_gens
      << " generations per launch, rows 2 lanes x " << s->island_K << " chunks";
}
void write_resident(std::ostringstream& o, const kmc_sampler* s)
{
    o << "resident mode (exact): whole ensemble in one workgroup's LDS (" << s->resident_tpb
      << " threads), up to " << kDrawTableGens << " generations per launch, "
      << (s->resident_lane2 ? std::string("two walkers per thread") : s->resident_lane ? std::string("one walker per thread") : "rows 2 lanes x " + std::to_string(s->island_K) + " chunks")
      << ", the launch's draws from a wide kernel before it";
}
void write_generation(std::ostringstream& o, const kmc_sampler* s)
{
    if (s->fused_L == 0)
        o << "one launch per generation (exact): generation_lane ND=" << s->cfg.ndim << ", one walker per lane, second-half walkers recompute their partner's first-half move, grid "
          << 2 * ((s->h + s->fused_tpb - 1) / s->fused_tpb) << " x " << s->fused_tpb;
    else
        o << "one launch per generation (exact): generation_group L=" << s->fused_L << " K=" << s->plan.K << ", rows lane-striped, second-half walkers recompute their partner's first-half move, grid "
          << 2 * ((s->h + s->fused_tpb / s->fused_L - 1) / (s->fused_tpb / s->fused_L)) << " x " << s->fused_tpb;
    o << launch_mode_text(s, "generation");
}
void write_data_density(std::ostringstream& o, const kmc_sampler* s)
{
    const DataPlan& ph = s->plan_half;
    const int64_t np = (int64_t)s->ntemps * s->h;                      // (a likelihood-tempered ladder: every rung's proposals in one pass)
    o << "data density (exact): per half-step propose kernel -> " << (ph.obs ? "data_partial_obs (one observation per lane, grid " + std::to_string(np)
                                                                             : "data_partial_lane (one proposal per lane, grid " + std::to_string((np + 63) / 64))
      << " x " << ph.nblocks << " workgroups of 256, " << ph.rounds << " rounds per wave) -> " << (s->temper_like ? "data_fold_split" : "data_fold") << " -> accept kernel, eager launches; "
      << s->data_ud->ndata << " observations of " << s->data_ud->ncols << " doubles; scratch " << ph.nblocks << " x " << np
      << " tree nodes (at most 4096 x " << (s->temper_like ? "ntemps x " : "") << "nwalkers doubles)";
}
void write_host_density(std::ostringstream& o, const kmc_sampler* s)
{
    o << "host-evaluated density (exact): per half-step propose kernel -> D2H -> callback -> H2D -> accept kernel, grid "
      << s->grid << " x 256";
}
void write_two_launch_vec(std::ostringstream& o, const kmc_sampler* s)
{
    o << "multi-launch (exact): half_step_vec L=" << s->plan.L << " K=" << s->plan.K << " ITER=" << s->plan.ITER
      << (s->plan.ragged ? " ragged" : " exact-size") << ", grid " << s->grid << " x " << s->tpb
      << launch_mode_text(s, "step");
    if (s->launch_mode == 3 && !(s->cfg.flags & KMC_NO_GRAPH)) {      // which kernel variant a replay's nodes run (kmc_updated.hip: spec_of_chunk)
        const char* why = nullptr;
        if (spec_variant_possible(s, kVarCredit, &why)) o << "; phase-specialised kernel instance in counted replays";
        else o << "; generic kernel in every phase (" << why << ")";
        // ... and whether one draw pass serves a whole workgroup in burn-in replays (kmc_shared_draws.hpp)
        if (spec_variant_possible(s, kVarShareBurnin, &why)) o << "; workgroup-shared draws in burn-in replays (" << variant_share(s, kVarShareBurnin) << " waves per workgroup)";
        else o << "; no workgroup-shared draws (" << why << ")";
    }
}
void write_two_launch_generic(std::ostringstream& o, const kmc_sampler* s)
{
    o << "multi-launch (exact): " << (s->user && s->uk.staged ? "half_step_staged (one walker per lane, rows staged through LDS)" : "half_step_generic (one walker per lane)")
      << ", grid " << s->grid << " x " << s->tpb;
}
void write_route(std::ostringstream& o, const kmc_sampler* s)
{
    if (s->islands) write_islands(o, s);
    else if (s->resident) write_resident(o, s);
    else if (s->fused) write_generation(o, s);
    else if (s->data_eval) write_data_density(o, s);
    else if (s->host_eval) write_host_density(o, s);
    else if (s->plan.vec) write_two_launch_vec(o, s);
    else write_two_launch_generic(o, s);
}

// KMC_DEBUG=feed-stats: what the feeding thread of the updated-graph mode spent per replay
void write_feed_stats(std::ostringstream& o, const kmc_sampler* s)
{
    if (s->feed_replays <= 0 || !debug_opt("feed-stats")) return;
    char b[200];
    std::snprintf(b, sizeof(b), "; feeding thread per replay of %lld generations: wait for a free executable %.1f us, parameter updates %.1f us, hipGraphLaunch %.1f us (%lld replays)",
                  (long long)s->uchunk, s->feed_wait_ns / 1e3 / s->feed_replays, s->feed_update_ns / 1e3 / s->feed_replays, s->feed_launch_ns / 1e3 / s->feed_replays, (long long)s->feed_replays);
    o << b;
}

// the kernel an own-stream move runs: half_step_<stem>_vec or _generic, the generic one in two passes around a host density's callback
std::string move_kernel(const kmc_sampler* s, const char* stem)
{
    const std::string k = std::string("half_step_") + stem;
    return s->host_eval ? k + "_generic (propose / accept passes)" : s->plan.vec ? k + "_vec" : k + "_generic";
}
void write_move(std::ostringstream& o, const kmc_sampler* s)
{
    char b[160];
    if (s->cfg.move == KMC_MOVE_DE) {
        std::snprintf(b, sizeof(b), "; differential-evolution move (KMC_MOVE_DE): gamma0 %.6g, sigma %.3g, kernel ", de_gamma0_of(s->cfg), s->cfg.de_sigma);
        o << b << move_kernel(s, "de");
    }
    if (s->cfg.move == KMC_MOVE_SNOOKER) {
        std::snprintf(b, sizeof(b), "; snooker move (KMC_MOVE_SNOOKER): gamma %.6g, kernel ", snooker_gamma_of(s->cfg.snooker_gamma));
        o << b << move_kernel(s, "snooker");
    }
    if (s->cfg.move == KMC_MOVE_MIX) {
        double w[KMC_MIX_MAX] = {0.0, 0.0, 0.0, 0.0};
        const MixTable mt = mix_table_of(s->cfg, w);
        o << "; move mixture (KMC_MOVE_MIX), one member per half-step:";
        for (int i = 0; i < mt.count; ++i) {
            if (mt.move[i] == KMC_MOVE_DE) std::snprintf(b, sizeof(b), " %.6g x DE (gamma0 %.6g, sigma %.3g)", w[i], mt.c0[i], mt.c1[i]);
            else std::snprintf(b, sizeof(b), " %.6g x snooker (gamma %.6g)", w[i], mt.c0[i]);
            o << (i ? "," : "") << b;
        }
        o << ", kernel " << move_kernel(s, "mix");
    }
}

void write_tempering(std::ostringstream& o, const kmc_sampler* s)
{
    if (!s->temper) return;
    o << "; parallel tempering: ntemps " << s->ntemps << " rungs in one launch per half-step (grid y = rung), kernel "
      << (s->plan.vec ? "half_step_temper_vec" : "half_step_temper_generic") << ", betas 1 .. ";
    char b[96];
    std::snprintf(b, sizeof(b), "%.6g", s->betas.back());
    o << b << ", swap sweep " << (s->cfg.swap_every > 0 ? "every " + std::to_string(s->cfg.swap_every) + " generations (" + (s->adapt ? (s->temper_like ? "temper_sweep_adapt<like>" : "temper_sweep_adapt<whole>") : s->temper_like ? "temper_sweep_like" : "temper_sweep") + ")" : std::string("off"));
    if (s->adapt) {
        std::snprintf(b, sizeof(b), ", lag %.6g, time %.6g", s->cfg.adapt_lag, s->cfg.adapt_time);
        o << "; adaptive ladder: until generation " << s->cfg.adapt_until << b << " (betas above: the initial ladder)";
    }
    if (s->temper_like) o << "; likelihood tempering: rung t samples prior + beta_t S, four launches per half-step for the whole ladder";
    if (s->temper_updated_fallback) o << "; KMC_LAUNCH=updated asked for: the updated-graph mode is not built for tempered samplers, fell back to the table graph";
}

// where rows, samples and moments are kept or sent (first: a launch mode the process's budget took away)
void write_storage(std::ostringstream& o, const kmc_sampler* s)
{
    if (s->budget_fallback) o << "; updated-graph budget of the process spent (kmc_set_updated_budget_mb): fell back to " << (s->launch_mode == 2 ? "eager launches" : "the table graph");
    if (s->push) o << "; accepted rows pushed into the peers' local copies (KMC_P2P_PUSH)";
    if (s->f32) o << "; rows kept in float (KMC_F32), arithmetic in double";
    if (s->stream_chain) o << "; chain streamed to host memory in blocks of " << s->ring_blk << " samples (device ring of 3 blocks" << (s->dst_chain_reg || s->dst_logp_reg ? ", destination page-locked" : "") << ")";
    if (s->d_ids) o << "; dealt sub-ensemble " << s->cfg.deal_rank << "/" << s->cfg.deal_count << " (walkers re-dealt between epochs)";
    if (s->d_mring) o << "; moments through a ring of " << s->mring_depth << " posted rows per wave";
}

// a runtime-compiled density: how its body is evaluated, the verdict on its sum form, its blobs
void write_density(std::ostringstream& o, const kmc_sampler* s)
{
    if (s->user) o << "; runtime-compiled density";
    if (s->user && s->user->is_body && s->fused)
        o << (s->fused_L == 0 ? " (function body, evaluated as written: one walker per lane)"
                              : " (function body recognised as a sum over elements and checked against the body on test rows: lane-striped)");
    else if (s->user && s->user->is_body && s->plan.vec && !s->resident && !s->islands)
    {
        const std::string& why_not = s->sep_off ? s->sep_off_note : s->user->sep_note;
        o << ((s->user->sep && !s->sep_off) ? " (function body recognised as a sum over elements and checked against the body on test rows: lane-striped)"
                                            : " (function body: rows lane-striped, the body evaluated per walker on the whole proposal" + (why_not.empty() ? std::string() : "; taken for a sum over elements, but " + why_not) + ")");
    }
    if (s->nblob > 0) o << " with a blob of " << s->nblob << " doubles per walker" << (s->d_chain_blob ? " (stored with every sample)" : "");
}

void write_shard(std::ostringstream& o, const kmc_sampler* s)
{
    if (s->p2p) o << "; P2P shard " << s->cfg.shard_rank << "/" << s->cfg.shard_count << (s->connected ? "" : " (not connected)");
    else if (s->cfg.shard_count > 1 || s->comm)
        o << "; replica shard " << s->cfg.shard_rank << "/" << s->cfg.shard_count
          << (s->comm ? ((s->comm_graph_ok && !(s->cfg.flags & KMC_NO_GRAPH) && s->launch_mode != 2) ? ", RCCL all-gather of the updated half after every half-step (captured in the graph)"
                                                                                                     : ", RCCL all-gather of the updated half after every half-step (enqueued launch by launch)") : "");
}

// KMC_DEBUG=geometry: what creation derived from the configuration and the text above does not show (tests/test_gpu_create_routes.py pins
// it); nothing that depends on the machine: no addresses, no word on whether pinned host memory got a device alias
void write_geometry(std::ostringstream& o, const kmc_sampler* s)
{
    if (!debug_opt("geometry")) return;
    const Plan& p = s->plan;
    auto data_plan_text = [](const DataPlan& d) { return std::to_string((int)d.obs) + "/" + std::to_string(d.rounds) + "/" + std::to_string(d.nblocks); };
    o << "; geometry: plan=" << (p.vec ? "vec" : "generic") << "/" << p.L << "/" << p.K << "/" << p.ITER << "/" << (p.ragged ? "ragged" : "exact")
      << " tpb=" << s->tpb << " grid=" << s->grid << " macc_stride=" << s->macc_stride << " macc_elems=" << s->macc_elems << " vec_lds=" << s->vec_lds
      << " nrows=" << s->nrows << " resident=" << s->resident << " resident_tpb=" << s->resident_tpb << " resident_lane=" << s->resident_lane
      << " resident_lane2=" << s->resident_lane2 << " islands=" << s->islands << " island_K=" << s->island_K << " island_ragged=" << s->island_ragged
      << " nislands=" << s->nislands << " island_lds=" << s->island_lds << " fused=" << s->fused << " fused_L=" << s->fused_L
      << " fused_tpb=" << s->fused_tpb << " fused_fold=" << s->fused_fold << " mring_depth=" << s->mring_depth << " mring_waves=" << s->mring_waves
      << " ring_blk=" << s->ring_blk << " ring_slots=" << s->ring_slots << " stream_by_walker=" << s->stream_by_walker << " push=" << s->push
      << " part_doubles=" << s->part_doubles << " plan_half=" << data_plan_text(s->plan_half) << " plan_all=" << data_plan_text(s->plan_all);
    const std::pair<const char*, const void*> bufs[] = {
        {"d_ring", s->d_ring}, {"d_draws", s->d_draws}, {"d_pos2", s->d_pos2}, {"d_glast", s->d_glast}, {"d_isum", s->d_isum}, {"d_msum", s->d_msum},
        {"d_mring", s->d_mring}, {"bw_scratch", s->bw_scratch}, {"bw_scratch_logp", s->bw_scratch_logp}, {"d_ids", s->d_ids}, {"d_mix", s->d_mix},
        {"d_like", s->d_like}, {"d_acc", s->d_acc}, {"d_prop", s->d_prop}, {"d_part", s->d_part}, {"d_betas", s->d_betas}, {"d_chain", s->d_chain},
        {"d_chain_logp", s->d_chain_logp}, {"d_blob", s->d_blob}, {"d_chain_blob", s->d_chain_blob}, {"d_err", s->d_err}};
    for (const auto& b : bufs) o << " " << b.first << "=" << (b.second != nullptr);
}
}  // namespace

// Human-readable description of how this sampler executes (kernel family, geometry, exchange).
KMC_EXPORT kmc_status kmc_sampler_describe(const kmc_sampler* s, char* buf, int64_t buflen)
{
    if (!s || !buf || buflen <= 0) return fail(KMC_ERR_BAD_ARG, "bad argument");
    std::ostringstream o;
    write_route(o, s);
    write_feed_stats(o, s);
    write_move(o, s);
    write_tempering(o, s);
    write_storage(o, s);
    write_density(o, s);
    write_shard(o, s);
    write_geometry(o, s);
    const std::string t = o.str();
    std::snprintf(buf, (size_t)buflen, "%s", t.c_str());
    return KMC_OK;
}
