// kmc_pointwise_host.hpp -- what the host code of the pointwise log-likelihood shares: kmc_pointwise.hip (the session, the statistics,
// the matrix, the weight series, the relative efficiency), kmc_psis.hip (PSIS-LOO over the same session) and kmc_pointwise_stages.hip (the
// plans and the stages that touch no device).  The request of one call, its plan, its session and the stages on them.  Internal.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "kmc_chain_view.hpp"
#include "kmc_convergence_host.hpp"
#include "kmc_pointwise.hpp"

namespace kmc_pw_host {

using namespace kmc_host;
using namespace kmc_chain_view;
using namespace kmc_pw;

constexpr int64_t kPwTargetWaves = 4096;          // of one pass: 4 per SIMD of 256 compute units
constexpr int64_t kPwMinRun = 16;                 // rows of a run at least: a run loads d_j once and writes two partials
constexpr int64_t kPwMatrixWaves = 65536;         // pw_matrix: waves along the rows at most
constexpr int64_t kPsisWorkspace = (int64_t)1 << 30;

// the cut of n rows and J observations: from n and J alone
struct PwPlan {
    int64_t run_len = 0, nruns = 0, nwaves = 0;   // nwaves: along the rows, each over ceil(J / 64) groups of observations
    int32_t lanes = 64, slots = 1, jp_log2 = 6;   // packed (J < 64): lanes = Jp observations per run slot, slots = 64 / Jp
    bool packed = false;
};
PwPlan pw_plan(int64_t n, int64_t J);

// the rows of a run of the matrix and weight kernels, which walk the rows in at most kPwMatrixWaves waves; and the waves
inline int64_t matrix_run_len(int64_t n) { return std::max(kPwMinRun, (n + kPwMatrixWaves - 1) / kPwMatrixWaves); }
inline int64_t matrix_waves(int64_t n) { return (n + matrix_run_len(n) - 1) / matrix_run_len(n); }
// bytes of work space a block of observations may take: the caller's, or kPsisWorkspace for 0
inline int64_t workspace_budget(int64_t workspace) { return workspace > 0 ? workspace : kPsisWorkspace; }

// how PSIS-LOO cuts J' observations of n rows into blocks: from n, the density's J, r_eff and the work-space budget alone
struct PsisPlan {
    int64_t M = 0, m_est = 0, block = 0, passes = 2 + kmc_psis::kSelectPasses;
    size_t per_obs = 0;                           // bytes of work space of one observation
    int sort_len = 1;
};
PsisPlan psis_plan(int64_t M, const PwPlan& pl, int64_t workspace);

struct PwKernels {
    std::shared_ptr<void> keep, keep_data, keep_weights;
    hipFunction_t pass[2][2] = {};                // [pass - 1][packed]
    hipFunction_t matrix = nullptr, weights = nullptr;
    hipFunction_t psis[3][2] = {};                // [mode][packed]
};

// the device copies one call owns, beyond the chain's: the list of selected walkers, held-out observations, the work space
struct PwBuffers : ChainUpload {
    int32_t *sel = nullptr, *Mj = nullptr;
    double *data = nullptr, *work = nullptr;
    void* work2 = nullptr;
    ~PwBuffers() { (void)hipFree(sel); (void)hipFree(Mj); (void)hipFree(data); (void)hipFree(work); (void)hipFree(work2); }
};

// the parts of a request that every entry point passes on as it got them
struct Selection { int64_t first_sample = 0; const uint8_t* walker_mask = nullptr; int64_t thin = 1; };
struct HeldOut { const double* data = nullptr; int64_t ndata = 0; int32_t ncols = 0; };      // [ndata][ncols] or nullptr
struct ObsRange { int64_t first = 0, count = 0; };
// where the density and its parameters come from: the sampler's (sampler_density), or the kmc_chain_* caller's own arguments
struct PwDensity { kmc_user_density* ud = nullptr; const double* params = nullptr; bool null_sampler = false; };
inline PwDensity sampler_density(kmc_sampler* s) { return s ? PwDensity{s->data_ud, s->dp.p, false} : PwDensity{nullptr, nullptr, true}; }

// What a call computes.  Stats: the statistics [4][J] of every observation.  Matrix: l itself over a range.  Weights: the series
// exp(l - M_j) over a range (no PSIS, no ESS).  RelativeEff: r_eff_j of that series, alone.  Psis: PSIS-LOO over a range.
enum class PwMode { Stats, Matrix, Weights, RelativeEff, Psis };
// Psis: where the relative efficiency comes from -- one value (r_eff), supplied per observation (r_eff_j [obs.count]), or computed from
// the chain (reff_stage)
enum class ReffFrom { One, Supplied, Chain };

// what a call asks for beyond the chain
struct PwRequest {
    PwMode mode = PwMode::Stats;
    kmc_user_density* ud = nullptr;
    const double* params = nullptr;               // 6
    Selection sel;
    HeldOut held;
    ObsRange obs;                                 // every mode but Stats
    ReffFrom reff = ReffFrom::One;
    double r_eff = 1.0;
    const double* r_eff_j = nullptr;
    int64_t workspace = 0;                        // see workspace_budget
    bool split = true;                            // the chains of the weight series (needs_conv_shape)
    int64_t max_lag = 0;
    double* weights_M = nullptr;                  // Weights: M_j [obs.count] out

    // the mode, the density and the selection; the sampler route's null-sampler refusal
    kmc_status begin(PwMode m, const PwDensity& d, const Selection& s)
    {
        if (d.null_sampler) return fail(KMC_ERR_BAD_ARG, "null sampler");
        mode = m; ud = d.ud; params = d.params; sel = s;
        return KMC_OK;
    }
    bool psis() const { return mode == PwMode::Psis; }
    bool needs_obs_range() const { return mode != PwMode::Stats; }
    bool per_observation_reff() const { return psis() && reff != ReffFrom::One; }               // tail lengths per observation
    bool supplied_reff() const { return psis() && reff == ReffFrom::Supplied; }
    bool computed_reff() const { return psis() && reff == ReffFrom::Chain; }
    bool needs_conv_shape() const { return mode == PwMode::RelativeEff || computed_reff(); }    // the ESS stage runs: its chains are checked
};

// one call's view of the chain, its stream, kernels and arguments.  (Members die in reverse order: the stream is drained before the
// buffers go.)
struct PwSession {
    ChainView v;
    PwBuffers b;
    ScopedStream ss;
    PwKernels pk;
    PwArgs a{};
    PwPlan pl;
    int64_t n = 0, J = 0, nsel = 0, kept = 0;     // rows = kept samples of nsel walkers
    kmc_conv_host::ConvShape sh;                  // needs_conv_shape: the chains of the weight series
    int64_t max_lag = 0;
    std::vector<double> r_used;                   // a per-observation r_eff: as used (1.0 where it is not finite and > 0) ...
    std::vector<int32_t> Mj;                      // ... and the tail lengths
    int64_t n_reff_nan = 0;
};

// what the relative-efficiency stage hands back, each [obs.count] or nullptr
struct ReffOut {
    double *r_eff = nullptr, *ess = nullptr;
    int64_t* T = nullptr;
    int32_t* flags = nullptr;
    double* v = nullptr;                          // the series itself, dense [n][obs.count]; with it the ESS is not taken
};

// kmc_pointwise_stages.hip: no device
kmc_status psis_check(int64_t n, double r_eff, int64_t* M, bool sizes_only = false);
kmc_status tail_lengths(int64_t n, int64_t obs_first, const double* r, int64_t count, PwSession* S);
double pairwise_tree(std::vector<double>& v);
// kmc_pointwise.hip
kmc_status pw_open(const ChainSource& src, const PwRequest& q, const void* result, PwSession* S);
kmc_status pw_stats(PwSession& S, double** work, int64_t* info, int npass = 2);
kmc_status reff_stage(PwSession& S, const PwRequest& q, const ReffOut& o, int64_t* info3);

}  // namespace kmc_pw_host
