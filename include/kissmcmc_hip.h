/*
 * kissmcmc_hip.h -- C ABI of the MI355X-native emcee (affine-invariant ensemble sampler) hot path.
 *
 * Drop-in boundary.  The reference (mauro3/KissMCMC.jl, pure Julia) has no FFI; the path sits
 * behind three Julia methods, and this header is what a `ccall` binding for that path binds:
 *
 *   emcee(pdf, theta0s; niter, nburnin, nthin, a_scale, ...)     reference src/samplers.jl:188-216
 *   _emcee(...)  (generation loop, stretch move, accept/reject)  reference src/samplers.jl:232-293
 *   g_pdf / cdf_g_inv / sample_g                                 reference src/samplers.jl:224-230
 *
 * `make_theta0s` (src/samplers.jl:311-349) and `squash_walkers` (src/samplers.jl:372-428) are
 * host-side pre/post-processing and stay in the host language.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, caller owns every host buffer.
 *   - Every function returns a kmc_status; kmc_last_error() gives the message of the last
 *     failure on the calling thread.  Nothing aborts the process.
 *   - Threads: any number of handles may be used at once, each by one host thread at a time (the reference's own
 *     call is a blocking function, src/samplers.jl:188).  The library never uses the legacy (null) stream, so one
 *     thread's blocking copies do not disturb the hipGraph capture of another.
 *   - Ensembles are dense row-major [nwalkers][ndim] arrays of double, walker order = the
 *     reference's (walkers 0..nwalkers/2-1 are the first half of src/samplers.jl:247).
 *   - "generation" = one pass of src/samplers.jl:245 (two half-steps, every walker proposes
 *     once).  The reference's `niter`/`nburnin` count log-pdf evaluations; the host shim
 *     converts with the reference's own integer divisions (src/samplers.jl:203-204).
 *   - The user closure `pdf` of src/samplers.jl:257 is replaced by a fixed menu of analytic
 *     log-densities (kmc_density) evaluated on the device.
 *   - Random stream: Philox4x32-10, counter {step_lo, step_hi, walker_lo, walker_hi},
 *     key {seed_lo, seed_hi}, step = 2*generation + half, walker = global walker index: the
 *     block rocRAND's rocrand4() yields after rocrand_init(seed, walker, 4*step).  Results
 *     are a pure function of (seed, inputs), independent of sharding and launch geometry.
 */
#ifndef KISSMCMC_HIP_H
#define KISSMCMC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KMC_VERSION 100 /* 0.1.0 */

typedef enum kmc_status {
    KMC_OK = 0,
    KMC_ERR_A_SCALE = 1,         /* a_scale <= 1                    src/samplers.jl:200 */
    KMC_ERR_ODD_WALKERS = 2,     /* "Use an even number of walkers." src/samplers.jl:202 */
    KMC_ERR_TOO_FEW_WALKERS = 3, /* "Use more walkers: at least DOF+2, but better many more." src/samplers.jl:205 */
    KMC_ERR_BAD_ARG = 4,
    KMC_ERR_NONFINITE_LOGP = 5,  /* an initial walker has log-pdf -inf/nan (reference: make_theta0s guarantees > -Inf, src/samplers.jl:338) */
    KMC_ERR_HIP = 6,
    KMC_ERR_OOM = 7,
    KMC_ERR_NO_DEVICE = 8,
    KMC_ERR_UNSUPPORTED = 9
} kmc_status;

/* Log-density menu (all drop normalisation constants).  p[] = kmc_config.params */
typedef enum kmc_density {
    KMC_GAUSSIAN_ISO = 0, /* -1/2 sum_i ((x_i - p0)/p1)^2                       p = {mu, sigma}      */
    KMC_EXPONENTIAL  = 1, /* any x_i < 0 ? -inf : -p0 * sum_i x_i                p = {rate}           (reference README.md:15) */
    KMC_ROSENBROCK   = 2, /* -sum_{i<N-1} [p1 (x_{i+1}-x_i^2)^2 + (p0-x_i)^2]/p2 p = {a, b, scale}    (reference test/runtests.jl:68 at N=2, {1,100,20}) */
    KMC_LOGNORMAL    = 3, /* any x_i <= 0 ? -inf : sum_i [-log x_i - (log x_i - p0)^2/(2 p1^2)]  p = {mu, sigma} */
    KMC_MVNORMAL2    = 4, /* ndim == 2: -1/2 (d' P d), d = x - {p0,p1}, P = [[p2,p3],[p3,p4]] (precision matrix) */
    KMC_USER_DENSITY = 100, /* runtime-compiled: sum_d term(x_d) + sum_{d<n-1} pair(x_d, x_{d+1}); kmc_config.user_density
                              holds the handle made by kmc_user_density_create; params[0..5] are passed to it as p[] */
    KMC_HOST_DENSITY = 101, /* ANY log-density, evaluated by the caller: per half-step the device writes the batch of
                              proposals, kmc_config.host_logpdf evaluates it on the host, the device accepts/rejects.
                              Keeps the reference's arbitrary `pdf` closure (src/samplers.jl:257); bound by the callback
                              and one PCIe round trip per half-step.  Single GPU, no island mode. */
    KMC_DATA_DENSITY = 102  /* a log-prior plus a sum of per-observation terms over a data array held on the device:
                              kmc_config.user_density holds the handle made by kmc_data_density_create; params[0..5] are
                              passed to it as p[].  See kmc_data_density_create for the value contract. */
} kmc_density;

/* KMC_HOST_DENSITY callback: rows = dense [nrows][ndim]; write the log-pdf of every row to logp_out[nrows].
   Return 0, or non-zero to abort the run (kmc_sampler_run then returns KMC_ERR_BAD_ARG).  Called on the
   thread that called kmc_sampler_set_positions / kmc_sampler_run / kmc_emcee_run.  A large half-step's proposals may arrive
   in several calls (consecutive pieces of the batch, evaluated while the next piece is still crossing PCIe); with
   kmc_config.host_accepted set it is exactly one call per half-step, so that batch state (blobs) lines up with the outcomes. */
typedef int (*kmc_host_logpdf_fn)(const double* rows, int64_t nrows, int64_t ndim, double* logp_out, void* user);
/* KMC_HOST_DENSITY, optional: called after the accept test of every half-step with its outcome, so the caller can
   carry per-walker side data of its density (the reference's blobs: `blob0s[nc] = blob1` on accept :264,
   `reduce_blob!(blobs[nc], blob0s[nc])` when the state is stored :270).  accepted[i] = 1 when row i of the batch
   host_logpdf has just evaluated replaced walker row0 + i; stored = 1 when this generation's states are stored
   (after burn-in, every nthin-th).  Return 0, or non-zero to abort the run. */
typedef int (*kmc_host_accepted_fn)(const uint8_t* accepted, int64_t nrows, int64_t row0, int64_t generation,
                                    int32_t stored, void* user);

/* Many-chain Metropolis, optional: proposals from the host.  rows = current states, dense [nrows][ndim]; write
   sample_ppdf(row) for every row to proposals_out [nrows][ndim] (a SYMMETRIC proposal, as the reference requires,
   src/samplers.jl:41).  Return 0, or non-zero to abort the run. */
typedef int (*kmc_host_propose_fn)(const double* rows, int64_t nrows, int64_t ndim, double* proposals_out, void* user);

enum {
    KMC_F64 = 0, /* state and arithmetic in IEEE double, as the reference (Float64) */
    KMC_F32 = 1  /* throughput option: walker rows and the stored chain are kept in IEEE single ON THE DEVICE (half the
                    row bytes); a proposal is rounded to single before its log-density is evaluated, so a stored row and
                    its log-pdf belong together; draws, log-densities, the accept test, counters and moments stay double,
                    and so does every HOST buffer of this interface.  Densities evaluated on the device (built-in or
                    runtime-compiled), one GPU (no KMC_P2P / KMC_ISLANDS / sharding / kmc_sampler_bind_positions). */
};

/* kmc_config.flags */
enum {
    KMC_STORE_CHAIN = 1u << 0, /* keep thetas      (src/samplers.jl:269) on the device: [nsamples][nwalkers][ndim] */
    KMC_STORE_LOGP  = 1u << 1, /* keep logdensities (src/samplers.jl:271): [nsamples][nwalkers] */
    KMC_MOMENTS     = 1u << 2, /* streaming sum x, sum x^2 per dimension over the samples that would be stored */
    KMC_NO_GRAPH    = 1u << 3, /* launch every half-step eagerly instead of replaying a hipGraph */
    KMC_ISLANDS     = 1u << 6, /* ISLAND MODE (opt-in, not the reference's partner rule): islands of `island_size` walkers live in LDS
                                  for `island_gens` generations per launch and draw partners from their own complementary
                                  half; walkers are re-dealt to islands between launches.  Same target distribution, far
                                  fewer kernel boundaries and no HBM traffic inside an epoch.  Needs nwalkers % island_size == 0,
                                  island_size >= ndim + 2, ndim <= 32, shard_count == 1; no chain storage.  Works with user densities
                                  (their island's rows fit the 160 KiB of LDS for every permitted island_size and ndim). */
    KMC_STREAM_CHAIN = 1u << 11, /* with KMC_STORE_CHAIN / KMC_STORE_LOGP: the chain does NOT live in HBM.  The device keeps a ring of three
                                    blocks of sample slots; every completed block is copied to the caller's host buffers
                                    (kmc_sampler_set_chain_host) by a second stream while sampling goes on, so the number of stored
                                    samples is bounded by host memory, not by the 288 GB of HBM (the reference grows per-walker
                                    vectors without bound, src/samplers.jl:268-272; C2 with nthin = 1 is 84 GB, C5 336 GB).  The
                                    host buffers are page-locked in place (hipHostRegister), so the copies are direct DMA into
                                    their final position; if that fails the copies are blocking and staged through the library's own page-locked
                                    buffers (the sampling then waits for them).  KMC_F64, one GPU
                                    (no KMC_P2P / sharding / KMC_ISLANDS); small ensembles stay in resident mode (their launches are cut to less than a block).
                                    kmc_emcee_run switches it on by itself when the chain would not fit the device. */
    KMC_CHAIN_BY_WALKER = 1u << 12, /* kmc_emcee_run and kmc_metropolis_run: kmc_outputs.chain is [nwalkers][nsamples][ndim] and chain_logp
                                    [nwalkers][nsamples] -- the reference's own order, thetas[w][k] (src/samplers.jl:219-221,
                                    :268-272) -- instead of sample-major.  Transposed on the device before the copy
                                    (kmc_sampler_get_chain_by_walker).  Together with KMC_STREAM_CHAIN (also in kmc_sampler_create):
                                    the host buffers of kmc_sampler_set_chain_host are [nwalkers][nsamples][ndim] and
                                    [nwalkers][nsamples], and a completed block is transposed into a device scratch block and
                                    copied into them as a 2-D window by the copy stream. */
    KMC_STORE_BLOBS = 1u << 13, /* a body density with blobs (kmc_user_density_create_body_blob; the reference's hasblob=true,
                                   src/samplers.jl:194-196): keep the blob of every stored sample, [nsamples][nwalkers][nblob]
                                   (reduce_blob! with the default push!, :196, :270); read with kmc_sampler_get_blobs.  The
                                   blob of every walker's CURRENT position (blob0s, :210, :264) is kept regardless. */
    KMC_P2P_FINEGRAINED = 1u << 7, /* with KMC_P2P: keep the rows in fine-grained (coherent, uncached-for-peers) device memory */
    /* The default exchange under KMC_P2P is the pull of the drawn rows with system-scope loads, ordered by a separate signal kernel. */
    KMC_P2P_PUSH    = 1u << 9, /* with KMC_P2P: every rank keeps local copies of all the other shards and reads its partner rows
                                  from them -- with system-scope loads, like the pull (never from the reader's L2: peers write
                                  that memory); a rank that accepts a move writes the new row into its copy on every peer as
                                  well (write-through stores over xGMI).  Only accepted rows cross the fabric (C2: 23 %), once
                                  per peer, instead of every drawn row once: less per link while the acceptance is below
                                  1 / shard_count (2 ranks: half the bytes; 8 ranks: 1.9 x).  Menu densities in the vector
                                  kernels (anything else keeps the pull: kmc_sampler_describe).  Not with KMC_P2P_FINEGRAINED /
                                  kmc_sampler_init_ball.  In the default library since round 5. */
    /* (bits 8 and 10 were KMC_P2P_FOLD_SIGNAL and KMC_P2P_LAZY of rounds 1-4: removed in round 5, refused with KMC_ERR_UNSUPPORTED) */
    KMC_P2P         = 1u << 4  /* walker sharding with peer-to-peer partner reads over xGMI: the sampler holds only
                                  its shard ([2][nwalkers/2/shard_count][ndim], halves back to back), reads partner
                                  rows straight from the owning rank's HBM and synchronises half-steps with
                                  per-rank progress flags; needs kmc_sampler_p2p_export/_connect (<= 8 shards) */
};

/* kmc_config.move: the proposal of a walker-step.
 *   KMC_MOVE_STRETCH  the reference's stretch move (src/samplers.jl:250-260); the zeroed default.
 *   KMC_MOVE_DE       differential evolution (opt-in, not in the reference; ter Braak 2006, emcee's DEMove): two distinct
 *                     partners j != k, uniform over the complementary half, and y = x + g (x_j - x_k) with
 *                     g = gamma0 (1 + sigma v), v uniform in (-1, 1); accepted when p1 - p0 >= log u (a symmetric move: no
 *                     (N-1) log z term).  Its own Philox stream, key {seed_lo ^ 0x44454D56 ("DEMV"), seed_hi}, counter
 *                     {step_lo, step_hi, walker, block} -- DESIGN.md section 2.  Two launches per generation, one GPU, double
 *                     rows: KMC_ERR_UNSUPPORTED with KMC_ISLANDS, KMC_P2P, shard_count > 1, deal_count > 0, KMC_F32,
 *                     KMC_STORE_BLOBS, a body density with blobs, and in kmc_sampler_rccl_init.
 *   KMC_MOVE_SNOOKER  the DE snooker update (opt-in; ter Braak & Vrugt 2008, emcee's DESnookerMove): three distinct partners z, z1,
 *                     z2, uniform over the complementary half (needs nwalkers >= 6), d = x - z, s = gamma T(d . (z1 - z2)) / T(d . d)
 *                     and y = x + d s; accepted when (ndim - 1) log|1 + s| + p1 - p0 >= log u.  T is the fixed pairwise summation
 *                     order of DESIGN.md section 2; the stream is the DE key family, blocks 2 and 3.  ndim >= 2 (KMC_ERR_BAD_ARG
 *                     otherwise); refused like KMC_MOVE_DE.
 *   KMC_MOVE_MIX      a weighted mixture of 2 to 4 DE / snooker members (mix_*): every HALF-STEP uses one member for all its
 *                     walkers, the first whose cumulative normalised weight exceeds u_mix = (w0 + 1/2) 2^-32 of Philox key
 *                     {seed_lo ^ 0x4D495856 ("MIXV"), seed_hi}, counter {step_lo, step_hi, 0, 0}: a pure function of (seed, step).
 *                     Weights are normalised in double, in member order; the last member catches rounding.  A stretch member is
 *                     KMC_ERR_UNSUPPORTED; the members' restrictions apply. */
enum {
    KMC_MOVE_STRETCH = 0,
    KMC_MOVE_DE      = 1,
    KMC_MOVE_SNOOKER = 3,   /* (2 is not a move: KMC_ERR_BAD_ARG) */
    KMC_MOVE_MIX     = 4
};
#define KMC_MIX_MAX 4
#define KMC_TEMPS_MAX 64
/* kmc_config.temper_mode: what a ladder tempers.
 *   KMC_TEMPER_WHOLE       rung t samples exp(betas[t] * logpdf): the whole log-density (the default)
 *   KMC_TEMPER_LIKELIHOOD  KMC_DATA_DENSITY only: rung t samples prior(x) + betas[t] * S(x), the two values of the data-density value
 *                          contract; the last beta may be 0 (the prior itself).  See kmc_sampler_get_rung_loglike. */
enum {
    KMC_TEMPER_WHOLE      = 0,
    KMC_TEMPER_LIKELIHOOD = 1
};

#define KMC_P2P_HANDLE_BYTES 128
#define KMC_RCCL_ID_BYTES 128

typedef struct kmc_config {
    int32_t  dtype;         /* KMC_F64 or KMC_F32 (device storage of the rows) */
    int32_t  density;       /* kmc_density */
    double   params[8];
    int64_t  nwalkers;      /* GLOBAL ensemble size (all shards) */
    int64_t  ndim;
    int64_t  ngenerations;  /* niter_walker   = niter  / nwalkers   src/samplers.jl:203 */
    int64_t  nburnin;       /* nburnin_walker = nburnin / nwalkers  src/samplers.jl:204 */
    int64_t  nthin;         /*                                      src/samplers.jl:190 */
    double   a_scale;       /*                                      src/samplers.jl:192 */
    uint64_t seed;
    uint32_t flags;
    int32_t  device;        /* HIP device ordinal */
    int32_t  shard_rank;    /* walker sharding: this sampler updates slice shard_rank ...          */
    int32_t  shard_count;   /* ... of shard_count of EACH half; 1 = the whole ensemble (default 0 -> 1) */
    void*    user_density;  /* kmc_user_density* when density == KMC_USER_DENSITY, else NULL */
    int32_t  island_gens;   /* KMC_ISLANDS: generations per epoch (launch); 0 -> 32 */
    int32_t  island_size;   /* KMC_ISLANDS: walkers per island: 64, 128 or 256; 0 -> 256 */
    kmc_host_logpdf_fn host_logpdf; /* KMC_HOST_DENSITY: the callback, else NULL */
    void*    host_user;     /* passed through to host_logpdf / host_accepted */
    kmc_host_accepted_fn host_accepted; /* KMC_HOST_DENSITY: per-half-step accept outcomes, or NULL */
    int32_t  deal_rank;     /* DEALT SUB-ENSEMBLES (opt-in, not the reference's partner rule; see kmc_sampler_deal_pack): this sampler is */
    int32_t  deal_count;    /* sub-ensemble deal_rank of deal_count; 0 = off.  nwalkers is then THIS sub-ensemble's size */
    int32_t  temper_mode;   /* what a ladder tempers: KMC_TEMPER_WHOLE (0, the default) or KMC_TEMPER_LIKELIHOOD (needs ntemps >= 2, KMC_DATA_DENSITY) */
    int32_t  temper_pad_;
    /* ADAPTIVE LADDER (opt-in; see the comment above kmc_sampler_get_ladder).  Zeroed: off.  (Here, in front of `move`: the struct's tail from `betas` on stays as it is.) */
    int64_t  adapt_until;   /* the sweeps of generations g < adapt_until adapt the ladder; 0 -> nburnin; 0 .. nburnin */
    double   adapt_lag;     /* ptemcee's adaptation_lag, in rounds: finite, > 0 (the bindings' default: 10000) */
    double   adapt_time;    /* ptemcee's adaptation_time: finite, > 0 (the bindings' default: 100) */
    int32_t  adapt;         /* 1: adapt the interior rungs during burn-in (needs ntemps >= 3, swap_every >= 1); 0: the ladder stays as given */
    int32_t  adapt_pad_;
    /* (the snooker and mixture fields stand in front of `move`: the four fields from `move` on stay the struct's tail) */
    double   snooker_gamma; /* KMC_MOVE_SNOOKER: gamma of the proposal; 0 -> 1.7 */
    int32_t  mix_count;     /* KMC_MOVE_MIX: members, 2 .. KMC_MIX_MAX */
    int32_t  mix_move[KMC_MIX_MAX];   /* ... each KMC_MOVE_DE or KMC_MOVE_SNOOKER */
    int32_t  mix_pad_[3];
    double   mix_weight[KMC_MIX_MAX]; /* ... its weight: finite, > 0; normalised by the library */
    double   mix_gamma[KMC_MIX_MAX];  /* ... its gamma0 (DE; 0 -> 2.38 / sqrt(2 ndim)) or gamma (snooker; 0 -> 1.7) */
    double   mix_sigma[KMC_MIX_MAX];  /* ... its sigma (DE members; 0 for snooker members) */
    /* PARALLEL TEMPERING (opt-in; see the comment above kmc_sampler_get_rung_state).  Zeroed: off. */
    const double* betas;    /* [ntemps] inverse temperatures, copied at creation: betas[0] == 1, strictly decreasing, finite, > 0
                             * (KMC_TEMPER_LIKELIHOOD: the last one may be 0) */
    int32_t  ntemps;        /* rungs of the ladder: 0 or 1 = off, else 2 .. KMC_TEMPS_MAX */
    int32_t  swap_every;    /* generations between swap sweeps; 0 = never */
    int32_t  move;          /* KMC_MOVE_STRETCH (0, the reference's move), KMC_MOVE_DE, KMC_MOVE_SNOOKER or KMC_MOVE_MIX */
    int32_t  move_pad_;
    double   de_gamma0;     /* KMC_MOVE_DE: gamma0 of the proposal; 0 -> 2.38 / sqrt(2 ndim) */
    double   de_sigma;      /* KMC_MOVE_DE: relative jitter of gamma, in [0, 1); 0 = none */
} kmc_config;

/* Host output buffers of the one-shot call; any pointer may be NULL. */
typedef struct kmc_outputs {
    double*  chain;         /* [nsamples][nwalkers][ndim]  (needs KMC_STORE_CHAIN) */
    double*  chain_logp;    /* [nsamples][nwalkers]        (needs KMC_STORE_LOGP)  */
    double*  accept_ratio;  /* [nwalkers]                  src/samplers.jl:291 */
    int64_t* naccept;       /* [nwalkers] */
    double*  final_pos;     /* [nwalkers][ndim] */
    double*  final_logp;    /* [nwalkers] */
    double*  sum;           /* [ndim]  (needs KMC_MOMENTS) */
    double*  sumsq;         /* [ndim] */
    int64_t  nmoment;       /* out: number of (sample, walker) pairs accumulated */
    int64_t  nsamples;      /* out: (ngenerations - nburnin) / nthin  src/samplers.jl:234 */
    double   device_ms;     /* out: generation loop only, HIP events on the sampler's stream */
    double*  blobs;         /* [nsamples][nwalkers][nblob] ([nwalkers][nsamples][nblob] with KMC_CHAIN_BY_WALKER): the blobs of a
                               body density created with kmc_user_density_create_body_blob (src/samplers.jl:270) */
} kmc_outputs;

typedef struct kmc_sampler kmc_sampler; /* opaque */
typedef struct kmc_user_density kmc_user_density; /* opaque */

/* ---- library ---- */
int         kmc_version(void);
/* sizeof(kmc_config) / sizeof(kmc_metropolis_config) / sizeof(kmc_outputs) / sizeof(kmc_metropolis_outputs) as this library was
   built: a binding checks them against its own mirror of the structs when it loads the library, so layout drift fails loudly
   before the first real call (a SHORTER stale kmc_outputs would have the library read -- and write through -- `blobs` past its end). */
int         kmc_sizeof_config(void);
int         kmc_sizeof_metropolis_config(void);
int         kmc_sizeof_outputs(void);
int         kmc_sizeof_metropolis_outputs(void);
int         kmc_device_count(void);
/* hipMemGetInfo of a device (a caller deciding between a device-resident chain and KMC_STREAM_CHAIN; reference
 * src/samplers.jl:268-272 grows the chain without bound). */
kmc_status  kmc_device_free_bytes(int device, uint64_t* free_bytes, uint64_t* total_bytes);
/* Small device buffers of samplers are recycled through a per-device cache (blocks of up to 8 MiB, at most 128 MiB held;
 * KMC_DEBUG=poison turns it off): a sampler of the reference's own sizes otherwise spends more time in hipMalloc / hipFree
 * than sampling (the README call: 1.7 ms -> 1.0 ms).  This returns every block the cache holds to the device; kmc_device_free_bytes
 * counts held blocks as free. */
void        kmc_device_cache_release(void);
/* Touch every page of a host buffer (one read-modify-write of a byte per 4 KiB, up to `nthreads` threads; contents unchanged): the
 * reference returns per-walker vectors that grew during the run (src/samplers.jl:269-271); a drop-in host allocates the dense output
 * arrays BEFORE the run and has them faulted in by a helper thread while the device samples, so that the chain read-out afterwards
 * copies into resident pages (4 096 walkers x 4 doubles x 1 000 samples: read-out 15.6 -> ~5 ms).  No device involved. */
void        kmc_host_prefault(void* buffer, uint64_t nbytes, int nthreads);
const char* kmc_last_error(void);
const char* kmc_status_string(kmc_status st);

/* Validation only: src/samplers.jl:200-205 plus argument sanity. No device needed. */
kmc_status  kmc_validate(const kmc_config* cfg);

/* Stretch-factor helpers (host): src/samplers.jl:224, :227. */
double      kmc_g_pdf(double z, double a);
double      kmc_cdf_g_inv(double u, double a);

/* ---- user-supplied log-densities: the device-side stand-in for the arbitrary `pdf` closure of
 *      src/samplers.jl:257.  Two C expressions are compiled at run time (hiprtc, gfx950) into the
 *      same kernels:  log p(x) = sum_d TERM + sum_{d<n-1} PAIR, where
 *        term_expr may use  x (= x_d), d, n (= ndim), p (const double*, = params[0..5]);
 *        pair_expr may use  x (= x_d), y (= x_{d+1}), d, n, p;   NULL/"" = no pair term.
 *      Compiled code objects are cached on disk ($KMC_CACHE_DIR, else ~/.cache/kissmcmc_hip; keyed by the program, the kernel
 *      headers, the options and the hiprtc version; KMC_CACHE_DIR=off disables), so later processes skip the compiler.
 *      A term may evaluate to -INFINITY to reject a proposal.  Works in the multi-launch, resident and
 *      island modes and under KMC_P2P (the plain pull; the push is for menu densities only). */
kmc_status  kmc_user_density_create(const char* term_expr, const char* pair_expr, kmc_user_density** out);
/* The general form: the BODY of a C++ function
 *     double logpdf(const double* x, int n, const double* p) { BODY }
 * over the whole proposal x[0..n-1] (n = ndim, p = params[0..5]); any coupling between the dimensions, loops, locals;
 * return -INFINITY to reject.  The emcee samplers keep the rows lane-striped like a menu density's and evaluate the body once
 * per walker on the whole proposal (collected through LDS); with KMC_DEBUG=no-body-vec, and beyond 1024 dimensions, it runs in the
 * one-walker-per-lane kernels (the proposal is collected per lane, ndim <= 1024; for double rows of ndim <= 256 the rows are staged
 * through LDS so that memory is still read in whole rows):
 * emcee (multi-launch), initial log-pdfs, kmc_sampler_init_ball, many-chain Metropolis -- slower than a menu or term / pair
 * density of the same form (those stripe a row over lanes), far faster than a host callback.  Not with KMC_ISLANDS; under KMC_P2P the unstaged kernel.
 * A body that IS a sum over elements --
 *     double s = 0; for (int i = 0; i < n; ++i) s += f(x[i]);  return g(s);       (or: i + 1 < n, reading x[i] and x[i + 1])
 * with the loop body any statements that read the proposal only as x[i] (x[i + 1]) and change s only by `s +=` (up to four such
 * accumulators, `return g(s, t, ...)`) -- is recognised as
 * such (kmc_user_density_is_separable) and the emcee samplers run it in the lane-striped kernels of the menu densities, the loop
 * body as the per-element function and g as the finish: same operations per element, the sum in lane order instead of index
 * order (log-pdfs equal to rounding, like a menu density's).  Early returns, other indices, state carried between elements are
 * not recognised and are evaluated per walker as above.  The recognition reads text, so the first sampler over the density
 * evaluates the generated form next to the body itself on 256 test rows and keeps the route only if they agree (else: per walker,
 * as written; kmc_user_density_is_separable then returns 0 and kmc_sampler_describe says why).  Reference: the arbitrary closure pdf(theta), src/samplers.jl:257. */
kmc_status  kmc_user_density_create_body(const char* body, kmc_user_density** out);
int         kmc_user_density_is_separable(const kmc_user_density* ud);
/* The gradient of a density made by kmc_user_density_create_body (not one with blobs), for the HMC step of kmc_metropolis_run
 * (hmc_nleap > 0) and kmc_grad_eval_host: `grad_body` is the body of
 *     void grad(const double* x, int n, const double* p, double* g)
 * which writes d log p / d x_i to g[i]; g[0 .. n) is zero on entry.  Compiled once here, so a body that does not compile is
 * KMC_ERR_BAD_ARG with the compiler's message (the previous gradient then stays); a later call replaces the gradient for every call
 * that starts after it returns.  Nothing checks that it IS the gradient of the
 * body: a wrong one costs acceptance, never correctness (compare kmc_grad_eval_host with differences of kmc_logpdf_eval_host). */
kmc_status  kmc_user_density_set_grad(kmc_user_density* ud, const char* grad_body);
/* ... returning a BLOB with the log-density -- the reference's `pdf(theta) -> (p, blob)` under hasblob=true
 * (src/samplers.jl:150-151, :194-196, :257) for device densities -- the body of
 *     double logpdf(const double* x, int n, const double* p, double* blob) { BODY }
 * which fills blob[0 .. nblob) (1 <= nblob <= 1024 doubles per evaluation; zero on entry).  A sampler over such a density
 * carries, next to every walker's log-pdf, the blob of its current position (blob0s[nc] = blob1 on accept, :264; initial
 * blobs from the initial evaluations, :209-210) and, with KMC_STORE_BLOBS, the blob of every stored sample (:270).
 * One GPU, double rows, no KMC_ISLANDS / KMC_P2P / KMC_STREAM_CHAIN / dealt sub-ensembles (KMC_ERR_UNSUPPORTED). */
kmc_status  kmc_user_density_create_body_blob(const char* body, int nblob, kmc_user_density** out);
int         kmc_user_density_nblob(const kmc_user_density* ud);   /* 0 for densities without blobs */
/* log-pdfs AND blobs of dense host rows pos_host [nrows][ndim] (evaluated on the device): the reference's `pdf.(theta0s)` under
 * hasblob=true (src/samplers.jl:209-210) -- e.g. the blob0 a caller's init_blobs(blob0, nsamples) receives (:238). */
kmc_status  kmc_logpdf_blob_eval_host(const kmc_config* cfg, const double* pos_host, double* logp_host, double* blob_host /* [nrows][nblob] */, int64_t nrows);
void        kmc_user_density_destroy(kmc_user_density* ud);

/* ---- data densities: the closure `pdf` of src/samplers.jl:257 as it usually is -- a log-prior plus a log-likelihood summed over
 *      a dataset -- evaluated on the device, the data array copied there once.  Two C++ function bodies, compiled at run time:
 *        term:  double term(const double* x, int n, const double* d, const double* p)   x = the proposal (n = ndim), d = ONE
 *               observation row (ncols doubles), p = params[0..5]
 *        prior: double prior(const double* x, int n, const double* p)                    (NULL or "": return 0.0;)
 *      data: float64 [ndata][ncols], COPIED at creation (later changes to the caller's array have no effect).
 *      Value contract (part of the interface: it keeps results a pure function of (seed, inputs), independent of launch geometry):
 *        lp(x) = -inf                 if prior(x) == -inf   (the terms need not be evaluated)
 *        lp(x) = prior(x) + S(x)      otherwise
 *        S(x)  = the pairwise tree over t_j = term(x, d_j), j = 0 .. ndata-1, in index order: each level adds neighbours
 *                (t0+t1), (t2+t3), ...; an odd last element passes up unchanged.  (The kernels may pad a short tail with +0.0: the
 *                same value except for the sign of a zero sum.)
 *      Creation compiles both bodies once (placeholder ndim): a body that does not compile is KMC_ERR_BAD_ARG with the compiler's
 *      message, no device needed.  Limits: 1 <= ncols <= 16, 1 <= ndata <= 2^30, and a sampler's ndim <= 32.
 *      Samplers run it as the host route's generation loop with the callback replaced by device kernels (per half-step: propose,
 *      partial sums, fold, accept; eager launches, no host synchronisation): KMC_STORE_CHAIN / _LOGP, KMC_MOMENTS, KMC_STREAM_CHAIN,
 *      KMC_CHAIN_BY_WALKER, kmc_sampler_set_state, kmc_emcee_run, kmc_logpdf_eval(_host).  KMC_ERR_UNSUPPORTED: KMC_F32, KMC_ISLANDS,
 *      KMC_P2P, sharding, dealt sub-ensembles, kmc_sampler_init_ball, kmc_sampler_half_step, blobs, kmc_metropolis_run.
 *      Freed with kmc_user_density_destroy. */
kmc_status  kmc_data_density_create(const char* term_body, const char* prior_body /* NULL: 0 */, const double* data /* [ndata][ncols] */,
                                    int64_t ndata, int32_t ncols, kmc_user_density** out);

/* ---- one-shot: emcee + _emcee, src/samplers.jl:188-293 ---- */
kmc_status  kmc_emcee_run(const kmc_config* cfg, const double* theta0 /* host [nwalkers][ndim] */,
                          kmc_outputs* out);

/* ---- stateful sampler (device-resident state; what bench.py and the distributed driver use) ---- */
kmc_status  kmc_sampler_create(const kmc_config* cfg, kmc_sampler** out);
/* Waits for the sampler's own streams; small device buffers then go back to a per-device cache WITHOUT the device-wide wait a
 * hipFree implies.  When a caller's stream was ever bound (kmc_sampler_set_stream) or the sampler is a shard (shard_count > 1, an RCCL
 * communicator attached) the whole device is waited for first, so work other streams still have in flight on the sampler's buffers
 * (a framework's collectives on the rows, ...) cannot race the next owner of a recycled block.  Work on a buffer handed out by
 * kmc_sampler_device_ptr that the library cannot know of must have completed before this call. */
void        kmc_sampler_destroy(kmc_sampler* s);
/* Run on a caller-owned HIP stream (hipStream_t) instead of the sampler's own. */
kmc_status  kmc_sampler_set_stream(kmc_sampler* s, void* hip_stream);
/* Use a caller-owned device buffer (double [nwalkers][ndim], e.g. a torch tensor's data_ptr) for
 * the ensemble instead of the sampler's own allocation, so a collective library can gather
 * into it in place.  The caller keeps it alive; call before kmc_sampler_set_positions. */
kmc_status  kmc_sampler_bind_positions(kmc_sampler* s, void* pos_dev);
/* KMC_P2P: export this sampler's IPC handles (KMC_P2P_HANDLE_BYTES), to be all-gathered by the
 * caller (one process per GPU), then connect with the blobs of all shard_count ranks in rank order.
 * With KMC_P2P, kmc_sampler_set_positions still takes the GLOBAL ensemble (each rank keeps its
 * slices; barrier across ranks before the first run), while get_positions/get_logp/get_naccept/
 * get_accept_ratio return this shard's nwalkers/shard_count rows (first-half slice, then
 * second-half slice). */
kmc_status  kmc_sampler_p2p_export(kmc_sampler* s, void* handle_out);
kmc_status  kmc_sampler_p2p_connect(kmc_sampler* s, const void* handles /* [shard_count][KMC_P2P_HANDLE_BYTES] */);
/* The all-gather exchange of the exact partner rule, native: a sampler created with shard_rank / shard_count (no KMC_P2P)
 * holds a full replica of the ensemble and updates its slice of each half; with an RCCL communicator attached,
 * kmc_sampler_run enqueues, per half-step, the kernel and an in-place ncclAllGather of the updated half on the sampler's
 * stream (reference src/samplers.jl:273: the join, across GPUs) -- captured into the same hipGraph chunks as the
 * single-GPU run where RCCL allows capture, enqueued launch by launch otherwise; no host involvement inside a run.
 * kmc_rccl_unique_id: rank 0 creates the id (KMC_RCCL_ID_BYTES), the caller distributes it (any transport), every
 * rank calls kmc_sampler_rccl_init (collective: ncclCommInitRank).  librccl.so is loaded on first use. */
kmc_status  kmc_rccl_unique_id(void* id_out);
kmc_status  kmc_sampler_rccl_init(kmc_sampler* s, const void* id /* KMC_RCCL_ID_BYTES */);
/* Whether the chunk (kernels + all-gathers) is replayed from a captured hipGraph or enqueued launch by launch must be the SAME on
 * every rank: kmc_sampler_rccl_capture captures now and reports this rank's outcome (1 / 0; 0 also with KMC_NO_GRAPH); the
 * driver reduces the answers over the ranks (MIN) and passes the result to kmc_sampler_rccl_set_capture on every rank
 * (0: drop the captured chunk, launch by launch from now on).  Results are identical either way. */
kmc_status  kmc_sampler_rccl_capture(kmc_sampler* s, int* captured);
kmc_status  kmc_sampler_rccl_set_capture(kmc_sampler* s, int use_captured);
/* librccl.so as this process resolves it (dlopen): ncclGetVersion's code (major*10000 + minor*100 + patch) and its path;
 * KMC_ERR_UNSUPPORTED when the library or one of the entry points used here cannot be resolved.  Needs no device. */
kmc_status  kmc_rccl_version(int* version, char* path_buf /* may be NULL */, int64_t path_buflen);
/* The same wiring for shards that live in ONE process on one device (no IPC): shards[r] = the sampler of shard r.
   They run concurrently on their own streams like ranks on separate GPUs (single-process tests, timing, profiling). */
kmc_status  kmc_sampler_p2p_connect_local(kmc_sampler* s, kmc_sampler* const* shards /* [shard_count] */);
/* One fabric link measured with the pull's own access pattern (a connected KMC_P2P sampler with double rows; the peers must be idle): `nrows` whole rows of shard
 * `peer` read at random row indices -- uniform with replacement, what src/samplers.jl:250 makes a link serve -- with the kernels' system-scope loads, `reps`
 * launches -> *gather_gbs; the same shard copied whole by the runtime's device-to-device copy -> *copy_gbs.  Read-only.  peer == own rank: local memory. */
kmc_status  kmc_sampler_p2p_link_probe(kmc_sampler* s, int peer, int64_t nrows, int reps, double* gather_gbs, double* copy_gbs);
/* Upload the ensemble (host, [nwalkers][ndim], global order), evaluate the initial log-pdfs on
 * the device (src/samplers.jl:209-210), reset generation/counters.  Fails with
 * KMC_ERR_NONFINITE_LOGP if any is not finite. */
kmc_status  kmc_sampler_set_positions(kmc_sampler* s, const double* theta_host);
/* Device-side make_theta0s (src/samplers.jl:311-349, intended behaviour): every walker gets
 * theta0 + N(0, diag(ball_radius^2)), redrawn while its log-pdf is -inf (:336-341), up to `ntries` draws per ball
 * size (:327), the ball shrinking WITHIN A WALKER by the reference's compounding factors 1, 1/2, 1/8, 1/64, ...
 * (:326) over `halving_steps` sizes (any value >= 1; the factor underflows to 0, i.e. theta0 itself, near 47).
 * Two deliberate differences from the reference's loop: the shrink factor restarts at 1 for every walker (the
 * reference never resets ball_radius, so one unlucky walker would shrink the ball of all later ones; walkers here
 * are independent and drawn in parallel -- the host-side make_theta0s of the shims keeps the reference's sequential
 * behaviour), and a walker that finds no admissible point is an error (KMC_ERR_NONFINITE_LOGP with the
 * reference's message; its own error() at :345 is unreachable).
 * Random stream: Philox4x32-10, key {seed_lo ^ 0x42414c4c, seed_hi}, counter {attempt, d / 2, walker_lo, walker_hi}
 * (attempt = 0-based try index of that walker over all ball sizes, walker = GLOBAL walker index); words (w0,w1,w2)
 * -> u1 = (((w0 << 20) | (w1 >> 12)) + 1/2) 2^-52, u2 = (w2 + 1/2) 2^-32, Box-Muller pair sqrt(-2 log u1) {cos, sin}(2 pi u2)
 * for dimensions d, d + 1.  A pure function of (seed, walker): sharded samplers draw their own rows of the same ball.
 * Afterwards the sampler is ready to run, as after kmc_sampler_set_positions. */
kmc_status  kmc_sampler_init_ball(kmc_sampler* s, const double* theta0 /* [ndim] */, const double* ball_radius /* [ndim] */,
                                  uint64_t seed, int halving_steps /* 7 */, int ntries /* 100 */);
/* Checkpoint / resume: restore positions [rows][ndim], log-pdfs, acceptance counters (may be NULL = 0)
 * and the generation counter of a previous sampler with the same config.  The random stream is a pure
 * function of (seed, generation, walker), so the continued run is bit-identical to an uninterrupted
 * one; moments restart at the restored generation.  Not with chain storage, single GPU. */
kmc_status  kmc_sampler_set_state(kmc_sampler* s, const double* pos_host, const double* logp_host,
                                  const int64_t* naccept_host, int64_t generation);
/* KMC_STREAM_CHAIN: where the chain goes -- host buffers chain_host [nsamples][nwalkers][ndim] (KMC_STORE_CHAIN) and
 * chain_logp_host [nsamples][nwalkers] (KMC_STORE_LOGP), caller-owned, alive until the sampler is destroyed (or this is
 * called again).  Call before kmc_sampler_run; sample k of a run is complete in these buffers after the kmc_sampler_sync
 * that follows the generation which stored it.  kmc_sampler_get_chain then copies from them (or is a no-op for the same
 * pointers).  A sampler created with KMC_CHAIN_BY_WALKER as well takes [nwalkers][nsamples][ndim] and [nwalkers][nsamples]
 * (the stride between walkers is the whole run's nsamples) and answers kmc_sampler_get_chain_by_walker instead.
 * The buffers are page-locked in place (hipHostRegister) so that blocks arrive by DMA behind the sampling; where that is
 * refused (a container's RLIMIT_MEMLOCK) the blocks come through bounce buffers on the caller's thread -- slower, same result. */
kmc_status  kmc_sampler_set_chain_host(kmc_sampler* s, double* chain_host, double* chain_logp_host);
/* Enqueue `ngenerations` generations (asynchronous).  shard_count must be 1. */
kmc_status  kmc_sampler_run(kmc_sampler* s, int64_t ngenerations);
/* Enqueue ONE half-step (src/samplers.jl:248-273) of the current generation over this shard's
 * slice; half = 1 also advances the generation counter.  For walker-sharded drivers that
 * exchange the updated slice between half-steps.  A sampler that runs one launch per generation (small states:
 * kmc_sampler_describe) goes back to its two-launch kernels at the first such call, in place and for good (same chain, moments
 * credited so far kept); a resident-mode sampler (whole ensemble in one workgroup's LDS) answers KMC_ERR_UNSUPPORTED unless it
 * was created with KMC_NO_GRAPH, which keeps the half-step kernels. */
kmc_status  kmc_sampler_half_step(kmc_sampler* s, int half);
kmc_status  kmc_sampler_sync(kmc_sampler* s);
/* Milliseconds between the start of the first and the end of the last generation enqueued by
 * the most recent kmc_sampler_run (HIP events); synchronises. */
kmc_status  kmc_sampler_last_run_ms(kmc_sampler* s, double* ms);
int64_t     kmc_sampler_generation(const kmc_sampler* s);
int64_t     kmc_sampler_nsamples(const kmc_sampler* s);
/* Number of half-step kernel launches enqueued so far and the algorithmic bytes each moves
 * (read (2 ndim + 1) * 8, write (ndim + 1) * 8 per walker-step).  Resident mode (<= 1024 walkers, <= 2048 for menu densities with ndim <= 8): a launch
 * carries up to 1024 whole generations and is preceded by the kernel that computes its draws; both are counted. */
int64_t     kmc_sampler_launch_count(const kmc_sampler* s);
/* How kmc_sampler_run issues this sampler's launches (same kernels, same results in every mode; reference
 * src/samplers.jl:245-247 -- the generation x half-step loop -- is what the modes enqueue).
 * A sampler measures the table graph against the updated graph (or eager launches) once, at its first kmc_sampler_run of >= 896 generations -- if the
 * job was planned long (kmc_config::ngenerations >= 4096) or the sampler has come that far; until then, and for short jobs, whole chunks replay the table graph
 * (up to ~9 % slower per half-step at C2's size): a caller that drives a long job in pieces -- a progress or checkpoint loop -- should make them >= 896 generations
 * (the Python front end's progress loop does), or decide with KMC_LAUNCH=updated,budget in the environment.
 * *budget_fallback (may be NULL)
 * becomes 1 when the sampler is not in the updated-graph mode because the PROCESS-WIDE budget of graph parameter updates was
 * spent (the HIP runtime keeps host memory per update, ~80 B in HIP 7.0 -- the runtime a PyTorch wheel brings -- and ~1.4 B in 7.2; 64 MiB worth by default, priced by hipRuntimeGetVersion, KMC_DEBUG=updated-budget-mb=n in the
 * environment or kmc_set_updated_budget_mb): said once on stderr, in kmc_sampler_describe, and here. */
#define KMC_LAUNCH_UNDECIDED     0   /* only short runs so far: whole chunks from the table graph, the rest eagerly */
#define KMC_LAUNCH_TABLE_GRAPH   1   /* hipGraph replay of 64 generations, schedule read from a device table */
#define KMC_LAUNCH_EAGER         2   /* one launch per half-step from the host */
#define KMC_LAUNCH_UPDATED_GRAPH 3   /* hipGraph replay (128 generations) with per-replay kernel-node parameter updates (two launches per generation or one: both kinds of kernel) */
#define KMC_LAUNCH_SINGLE        4   /* resident / island kernels (many generations per launch), host-evaluated density */
int         kmc_sampler_launch_mode(const kmc_sampler* s, int* budget_fallback);
void        kmc_updated_budget(int64_t* calls_used, int64_t* calls_budget);   /* parameter updates so far / allowed, this process */
void        kmc_set_updated_budget_mb(double mb);                              /* priced at 80 B (HIP < 7.2) or 2 B per update; <= 0: no updated-graph mode from now on */

/* One line describing how this sampler executes (kernel family and geometry, exchange scheme). */
kmc_status  kmc_sampler_describe(const kmc_sampler* s, char* buf, int64_t buflen);

/* Device pointers for zero-copy exchange (torch / RCCL): which = 0 positions [nwalkers][ndim],
 * 1 logp [nwalkers], 2 naccept (uint32 [nwalkers]). */
void*       kmc_sampler_device_ptr(kmc_sampler* s, int which);

/* Downloads (synchronise the sampler's stream first). */
kmc_status  kmc_sampler_get_positions(kmc_sampler* s, double* host /* [nwalkers][ndim] */);
kmc_status  kmc_sampler_get_logp(kmc_sampler* s, double* host /* [nwalkers] */);
kmc_status  kmc_sampler_get_naccept(kmc_sampler* s, int64_t* host /* [nwalkers] */);

/* Parallel tempering (kmc_config.ntemps >= 2).  The sampler holds ntemps ensembles of nwalkers walkers; rung t
 * samples exp(betas[t] * logpdf) with the configured move, partners from the complementary half of the SAME rung, its draws keyed by
 * the walker word t * nwalkers + w (rung 0 draws what the untempered sampler draws).  Stored log-densities are UNTEMPERED on every
 * rung.  After generation g, when swap_every > 0 and (g + 1) % swap_every == 0, sweep n = (g + 1) / swap_every - 1 exchanges walker w
 * of rung t with walker w of rung t + 1 for every t == n (mod 2), when (beta_t - beta_{t+1}) (logp_{t+1,w} - logp_{t,w}) >= log u,
 * u from Philox key {seed_lo ^ 0x54454D50 ("TEMP"), seed_hi}, counter {n_lo, n_hi, w, t}.  Every existing read-out (positions,
 * log-pdfs, counters, chain, moments) is rung 0's; a stored sample of generation g is the state BEFORE that generation's sweep.
 * One GPU, double rows, two launches per generation (+ the sweep): KMC_ERR_UNSUPPORTED with KMC_HOST_DENSITY, KMC_DATA_DENSITY (unless
 * temper_mode is KMC_TEMPER_LIKELIHOOD, below),
 * blobs, KMC_F32, KMC_ISLANDS, KMC_P2P, sharding, dealt sub-ensembles, kmc_sampler_init_ball, kmc_sampler_bind_positions and
 * kmc_sampler_rccl_init.  kmc_sampler_set_positions copies the ensemble to every rung.
 *   kmc_sampler_get_rung_state  any pointer may be NULL: positions [ntemps][nwalkers][ndim], log-pdfs and acceptance counters
 *                               [ntemps][nwalkers], logp_sum [ntemps] = the sum over stored generations and walkers of the untempered
 *                               log-density of the stored state
 *   kmc_sampler_set_rung_state  all rungs at once: logp NULL = evaluate; naccept, nswap, logp_sum NULL = zero; generation > 0 is a
 *                               checkpoint restore (as kmc_sampler_set_state, which a tempered sampler refuses)
 *   kmc_sampler_get_swaps       accepted exchanges per neighbouring pair [ntemps - 1], counted from the end of burn-in */
kmc_status  kmc_sampler_get_rung_state(kmc_sampler* s, double* pos_host, double* logp_host, int64_t* naccept_host, double* logp_sum_host);
kmc_status  kmc_sampler_set_rung_state(kmc_sampler* s, const double* pos_host, const double* logp_host, const int64_t* naccept_host,
                                       const uint64_t* nswap_host, const double* logp_sum_host, int64_t generation);
kmc_status  kmc_sampler_get_swaps(kmc_sampler* s, uint64_t* nswap_host);
/* Likelihood tempering (kmc_config.temper_mode = KMC_TEMPER_LIKELIHOOD; KMC_DATA_DENSITY with ntemps >= 2).
 * Rung t samples prior(x) + betas[t] * S(x).  The tempered value is q = pri + (beta * S): the product is rounded, then the sum, no
 * fused multiply-add.  Accept tests: stretch and snooker (t1 + q1) - q0 >= log u, DE q1 - q0 >= log u; a proposal whose prior is
 * -inf is never accepted; draws, partners, walker words and the mixture choice as above.  With beta = 1.0 q has the bits of
 * pri + S: rung 0 of a ladder that never swaps is the plain KMC_DATA_DENSITY sampler bit for bit.  The sweep keeps its schedule,
 * pairing and stream; its test is (beta_t - beta_{t+1}) (S_{t+1,w} - S_{t,w}) >= log u (the priors cancel).  The stored log-pdf of
 * every rung stays the untempered posterior pri + S, so every read-out above keeps its meaning; S and the prior are kept next to
 * it per walker and rung and travel with their row in an exchange.  betas[ntemps - 1] may be 0: the prior rung, which closes the
 * thermodynamic integral  log Z = int_0^1 <S>_beta dbeta  (Z is the evidence when the prior body is normalised).  A half-step of the
 * whole ladder is four launches: every rung's proposals go through one pass of the data kernels.
 * KMC_ERR_UNSUPPORTED with any density but KMC_DATA_DENSITY, and with everything KMC_DATA_DENSITY or parallel tempering refuses.
 *   kmc_sampler_get_rung_loglike      any pointer may be NULL: S and the log-prior of every walker [ntemps][nwalkers], loglike_sum
 *                                     [ntemps] = the sum over stored generations and walkers of S of the stored state (taken before
 *                                     that generation's sweep, like logp_sum)
 *   kmc_sampler_set_rung_loglike_sum  a checkpoint's sums back in (NULL: zero).  The per-walker S and priors are NOT part of a
 *                                     checkpoint: kmc_sampler_set_positions and kmc_sampler_set_rung_state evaluate them again from
 *                                     the positions on the device, and the value contract makes that the same bits;
 *                                     kmc_sampler_set_rung_state zeroes the sums, so call this after it */
kmc_status  kmc_sampler_get_rung_loglike(kmc_sampler* s, double* loglike_host, double* logprior_host, double* loglike_sum_host);
kmc_status  kmc_sampler_set_rung_loglike_sum(kmc_sampler* s, const double* loglike_sum_host);

/* Adaptive ladder (kmc_config.adapt = 1; ntemps >= 3, swap_every >= 1; both temper modes, every move; DESIGN.md sections 2 and 4d).
 * The sweep kernels move the interior rungs towards equal swap acceptance between all neighbouring pairs (Vousden, Farr & Mandel
 * 2016, ptemcee's ladder dynamics) while the generation g of a sweep is < adapt_until; from adapt_until <= nburnin on the ladder is
 * frozen, so every stored sample, moment and rung sum comes from one fixed ladder.  Sweeps alternate pair parity, so a ROUND is sweep n
 * even followed by sweep n + 1, and tries every pair once.  A sweep with g < adapt_until adds its accepted exchanges per pair into
 * round_acc; after the odd sweep n of round k = (n - 1) / 2 with g < adapt_until, with A_i = (double)round_acc[i] / (double)nwalkers,
 * each operation rounded on its own:
 *     kappa = (lag / ((double)k + lag)) / time
 *     S'_j  = S_j + kappa * (A_{j-1} - A_j)                         j = 1 .. ntemps - 2
 *     tau_0 = 1,  tau_j = tau_{j-1} + exp(S'_j),  beta'_j = 1 / tau_j
 * S and the interior betas are replaced when every beta'_j is finite and 1 > beta'_1 > ... > beta'_{T-2} > beta_{T-1}; otherwise
 * nothing is and `skipped` counts the round.  round_acc is zeroed either way.  beta_0 and beta_{T-1} never move.  S_j =
 * log(1 / beta_j - 1 / beta_{j-1}) is state: computed once at creation from the caller's ladder, never derived from the betas again.
 * The round number follows from the sweep number alone: the same run in every launch mode and across a checkpoint.
 * kmc_sampler_set_positions starts the ladder again from the caller's.
 *   kmc_sampler_get_ladder  any tempered sampler; any pointer may be NULL: the current betas [ntemps], S [ntemps - 2] (rung j's at
 *                           j - 1), round_acc [ntemps - 1] and the rounds skipped
 *   kmc_sampler_set_ladder  an adaptive sampler: a checkpoint's four values back in (all four are required; betas[0] and
 *                           betas[ntemps - 1] must be the sampler's own).  kmc_sampler_set_rung_state starts the ladder again: call
 *                           this after it */
kmc_status  kmc_sampler_get_ladder(kmc_sampler* s, double* betas_host, double* S_host, uint64_t* round_acc_host, uint64_t* skipped_host);
kmc_status  kmc_sampler_set_ladder(kmc_sampler* s, const double* betas_host, const double* S_host, const uint64_t* round_acc_host, const uint64_t* skipped_host);
kmc_status  kmc_sampler_get_accept_ratio(kmc_sampler* s, double* host /* [nwalkers] */);
kmc_status  kmc_sampler_get_moments(kmc_sampler* s, double* sum, double* sumsq /* [ndim] */, int64_t* n);
/* Chain of this shard: [nsamples][nlocal][ndim] and [nsamples][nlocal]; nlocal = nwalkers /
 * shard_count, local order = (first-half slice, second-half slice).  With shard_count == 1
 * this is the global walker order. */
kmc_status  kmc_sampler_get_chain(kmc_sampler* s, double* chain, double* chain_logp);
/* The same samples in the reference's order (thetas[w][k], logdensities[w][k], src/samplers.jl:219-221, :268-272):
 * chain [nlocal][k][ndim], chain_logp [nlocal][k], k = samples stored so far (= nsamples after a complete run), dense.
 * Transposed on the device in pieces of walkers and copied out contiguously, so the host never reorders gigabytes
 * (what squash_walkers' default, walker-major, concatenation wants; src/samplers.jl:395-413).  With KMC_STREAM_CHAIN only
 * for a sampler created with KMC_CHAIN_BY_WALKER (then a copy of / no-op on the streamed buffers, stride nsamples). */
kmc_status  kmc_sampler_get_chain_by_walker(kmc_sampler* s, double* chain, double* chain_logp);
/* Blobs of a body density with blobs (any pointer may be NULL): current [nwalkers][nblob] = the blob of every walker's present
 * position (blob0s, src/samplers.jl:210, :264); stored (needs KMC_STORE_BLOBS) = the blobs of the samples stored so far,
 * [k][nwalkers][nblob] sample-major, or with by_walker != 0 [nwalkers][k][nblob]: blobs[w][k] in the reference's order (:238, :270). */
kmc_status  kmc_sampler_get_blobs(kmc_sampler* s, double* current, double* stored, int by_walker);

/* ---- dealt sub-ensembles: the multi-GPU mode WITHOUT a per-half-step exchange (opt-in extension) ----
 *
 * The reference draws partners from the whole complementary half (src/samplers.jl:250), which across GPUs costs one
 * exchange of walker rows per half-step (KMC_P2P, or an all-gather): fabric-bound on point-to-point xGMI.  Here each
 * GPU instead runs the reference's algorithm UNCHANGED on its own sub-ensemble of S = kmc_config.nwalkers walkers
 * (partners from that sub-ensemble's complementary half; an ordinary sampler: hipGraph replay, moments, ...) for an
 * epoch of E generations, and between epochs the walkers are RE-DEALT across the deal_count sub-ensembles by a
 * state-independent permutation: one all-to-all of S (ndim + 2) doubles per GPU per epoch (RCCL all_to_all_single in
 * the Python driver) instead of 2 E exchanges.  Every sub-ensemble update is a valid emcee move for its walkers and
 * the deal ignores the state, so the target distribution is unchanged; the partner pool is what differs from the
 * reference, which is why this is opt-in and never what bench.py reports as `value`.
 *
 * Contract (restated by the oracle, kmco_emcee_dealt):
 *   - sub-ensemble r of P initially holds global walkers [r S, (r+1) S) (kmc_sampler_set_positions takes ITS rows);
 *     its Philox key is kmc_deal_seed(seed, r) = seed + (r + 1) * 0x9E3779B97F4A7C15 (mod 2^64), walker index =
 *     local slot, so the draws of a slot do not depend on which walker sits in it;
 *   - after generation g with (g + 1) % E == 0 the deal of epoch e = (g + 1) / E - 1 happens: slot j of
 *     sub-ensemble r goes to send position t = (A j + C) mod S, (A, C) = kmc_deal_perm(seed, e, r, S); chunk
 *     q = t / (S / P) of the send buffer goes to sub-ensemble q and lands at its slots [r S / P, (r + 1) S / P)
 *     in order -- exactly what all_to_all_single(recv, send) with equal splits does;
 *   - a walker carries its position, log-pdf, acceptance counter and global index (kmc_sampler_get_walker_ids).
 * kmc_sampler_deal_pack first credits every walker's current value to the streaming moments (they are per slot).
 * A stored chain (KMC_STORE_CHAIN / KMC_STORE_LOGP) is BY SLOT, as the kernels write it; the sample of a generation is taken
 * before the deal that follows it, and which walker a slot held during an epoch follows from replaying kmc_deal_perm on
 * the host (distributed.deal_slot_ids; DealtEmcee.chain / gather_chain re-file the samples by walker) -- pooling all
 * samples, what squash_walkers does, needs no identities.
 * Needs S % (2 P) == 0, KMC_F64, a device density, no KMC_STREAM_CHAIN / KMC_P2P / KMC_ISLANDS / sharding. */
uint64_t    kmc_deal_seed(uint64_t seed, int32_t deal_rank);
kmc_status  kmc_deal_perm(uint64_t seed, int64_t epoch, int32_t deal_rank, int64_t S, int64_t* A, int64_t* C);
/* Enqueue (on the sampler's stream) the packing of this sub-ensemble's S rows of ndim + 2 doubles into send_dev
 * (device, S * (ndim + 2) doubles), shuffled for the deal of `epoch`; and the taking-over of a received buffer. */
kmc_status  kmc_sampler_deal_pack(kmc_sampler* s, int64_t epoch, void* send_dev);
kmc_status  kmc_sampler_deal_unpack(kmc_sampler* s, const void* recv_dev);
/* Global walker index held by each local slot (host, [nwalkers]); row order of get_positions / get_naccept. */
kmc_status  kmc_sampler_get_walker_ids(kmc_sampler* s, int64_t* host);
/* Checkpoint / resume of a sub-ensemble: kmc_sampler_set_state restores the slots' contents and the generation, this the
 * slot -> walker map that goes with that generation's epoch (host, [nwalkers]; replayed from kmc_deal_perm). */
kmc_status  kmc_sampler_set_walker_ids(kmc_sampler* s, const int64_t* host);

/* ---- stateless device ops on caller-owned device memory ---- */
/* logp[i] = log pdf(pos[i]) for nrows rows, src/samplers.jl:209. */
kmc_status  kmc_logpdf_eval(const kmc_config* cfg, const double* pos_dev, double* logp_dev,
                            int64_t nrows, void* hip_stream);

/* Same on dense host rows [nrows][ndim] (allocates, copies, evaluates, copies back). */
kmc_status  kmc_logpdf_eval_host(const kmc_config* cfg, const double* pos_host, double* logp_host, int64_t nrows);

/* grad[i] = the gradient of log pdf at pos[i] for dense host rows [nrows][ndim], evaluated on the device with the arithmetic of the
 * HMC step (kmc_metropolis_config): a menu density, or a body density with kmc_user_density_set_grad; ndim <= 32. */
kmc_status  kmc_grad_eval_host(const kmc_config* cfg, const double* pos_host, double* grad_host /* [nrows][ndim] */, int64_t nrows);

/* ---- many-chain Metropolis: metropolis / _metropolis, reference src/samplers.jl:59-128 ----
 *
 * The reference's `metropolis(pdf, sample_ppdf, theta0; niter, nburnin, nthin)` is one serial Markov
 * chain; the device form runs `nchains` independent chains at once, one per lane, each the reference's
 * loop (src/samplers.jl:96-126): propose theta1 = sample_ppdf(theta0), accept iff
 * p1 - p0 > log(rand()) (strict, :101), store the current state every nthin-th step after burn-in
 * (:108-116), count accepted steps after burn-in (:105, :122-125), accept_ratio = naccept /
 * (niter - nburnin) (:127).  `niter`, `nburnin` count steps PER CHAIN, as in the reference.
 * `sample_ppdf` is the symmetric Gaussian step of the reference's tests, theta + step .* randn(ndim)
 * (test/runtests.jl:54,59,64,75), `pdf` a menu or runtime-compiled density.
 * Random stream: Philox4x32-10, key {seed_lo ^ 0x4d455452, seed_hi}, counter {it_lo, it_hi, chain, block};
 * block 0 = words (w0,w1) -> Box-Muller pair for dimensions 0,1 and (w2<<20 | w3>>12) -> the accept uniform;
 * block b >= 1 = (w0,w1) -> dimensions 4b-2,4b-1 and (w2,w3) -> dimensions 4b,4b+1.  A chain's result is
 * a pure function of (seed, chain index, inputs).
 *
 * Covariance-shaped proposal (`chol` instead of `step`): theta + L z with a lower-triangular L [ndim][ndim] and the SAME draws --
 * iteration `it` of chain `c` has the normals z_0 .. z_{ndim-1} and the accept uniform above, nothing more is drawn.
 *   delta_i = ((L_i0 z_0 + L_i1 z_1) + ...) + L_ii z_i     j ascending, every j <= i evaluated (zeros included),
 *   y_i     = x_i + delta_i
 * every product and every sum rounded to double on its own: NO fused multiply-add.  The proposal is symmetric, the accept test
 * (p1 - p0 > log u, strict) is the same.  Every entry of the lower triangle must be finite, the diagonal > 0.  A diagonal L is
 * therefore NOT `step` bit for bit: `step` is fma(step_i, z_i, x_i), one rounding less.  (The few-chains route keeps delta in
 * its draw table and runs the table kernel with a step of 1.0: fma(1.0, delta, x) is x + delta exactly.)  ndim <= 128.
 *
 * Tuning across chains (tune_rounds = R >= 1): burn-in is cut at b_r = floor(r nburnin / (R + 1)), r = 1..R (equal boundaries
 * collapse into one).  Before iteration b_r runs, Sigma = the covariance of the nchains CURRENT states (kmc_chain_covariance's
 * definition on them as a chain of one sample and nchains walkers: two passes, divisor nchains - 1, on the device),
 * C = (scale scale) Sigma entry by entry, scale = tune_scale or 2.38 / sqrt(ndim), and L <- kmc_cholesky_lower(C); if that fails
 * the previous L stays and the round is counted in tune_skipped.  The last L is in force from b_R < nburnin on: every stored
 * sample is drawn with one fixed proposal.  A boundary always ends a launch; apart from that results do not depend on how the
 * iteration range is cut, and a run stays a pure function of (seed, inputs).  With tune_rounds > 0 `step` / `chol` is the
 * INITIAL proposal, and a `step` is treated as diag(step) under the rule above from iteration 0 on (one arithmetic throughout).
 * Needs nchains > ndim, nburnin >= tune_rounds + 1, no host_propose.
 *
 * Hamiltonian Monte Carlo step (hmc_nleap = nleap >= 1; `step` holds the step sizes, a diagonal metric): a gradient-informed
 * proposal from the SAME draws.  Iteration `it` of chain `c` has the normals z_0 .. z_{ndim-1} and the accept uniform u above, and
 * j = w3 & 0xFFF of block 0 (the uniform uses w3 >> 12: nothing else reads these 12 bits).  Nothing more is drawn.
 *   f    = 1.0 + jitter * (((double)j + 0.5) * 0x1p-11 - 1.0)       jitter = hmc_jitter in [0, 1); jitter == 0 gives f == 1.0 exactly
 *   e_i  = step_i * f ;   h_i = 0.5 * e_i
 *   m    = z ;            K0 = 0.5 * ((m_0 m_0 + m_1 m_1) + ...)     i ascending
 *   y    = x ;            g  = grad(y)
 *   nleap times:   m_i = m_i + h_i * g_i ;  y_i = y_i + e_i * m_i  (every i) ;  g = grad(y) ;  m_i = m_i + h_i * g_i
 *   p1   = logpdf(y) ;    K1 as K0 from the final m
 *   accept  iff  (p1 - K1) - (p0 - K0) > log u                       strict, as src/samplers.jl:101
 * Every product and every sum is rounded to double on its own: NO fused multiply-add.  logpdf is the density's evaluation as
 * everywhere else, so a stored chain_logp entry has the bits kmc_logpdf_eval gives for that stored position.  grad is a pure function
 * of the position: for a menu density the gradient below, for a runtime-compiled body density the body given to
 * kmc_user_density_set_grad.  A non-finite gradient or log-density is not an error: NaN or inf propagates and the strict comparison
 * rejects (a divergent trajectory is a rejected proposal); p0 = -inf at the start is carried as the reference carries it, and the
 * first finite proposal is then accepted.  Counters, burn-in, thinning, storage and moments are those of the random walk; a chain's
 * result stays a pure function of (seed, chain index, inputs).  The iteration range is cut into launches of max(1, 65536 / nleap)
 * iterations, and never takes the few-chains table route.
 * Gradients of the menu densities (p = the digested parameters the kernels take; the operation order is fixed in kmc_hmc.hpp):
 *   KMC_GAUSSIAN_ISO  (p0 = mu, p1 = 1 / sigma)        t = (x_i - p0) * p1;  g_i = -(t * p1)
 *   KMC_EXPONENTIAL   (p0 = rate)                      g_i = -p0, outside the support as well
 *   KMC_ROSENBROCK    (a, b, s = p0, p1, p2 = 1/scale) acc = 0.0;  k >= 1: d = x_k - x_{k-1} * x_{k-1}, acc = (2.0 * b) * d;
 *                                                      k <= n - 2: d = x_{k+1} - x_k * x_k, acc = acc - ((4.0 * b) * x_k) * d,
 *                                                      acc = acc - 2.0 * (a - x_k);   g_k = -(acc * s)
 *   KMC_LOGNORMAL     (p0 = mu, p1 = sigma)            x_i > 0: lx = log(x_i), t = (lx - p0) / p1, g_i = -((1.0 + t / p1) / x_i);
 *                                                      otherwise g_i = 0.0
 *   KMC_MVNORMAL2     (d0 = x_0 - p0, d1 = x_1 - p1)   g_0 = -(p2 * d0 + p3 * d1);  g_1 = -(p3 * d0 + p4 * d1)
 * Not with chol, tune_rounds > 0, host_propose, KMC_HOST_DENSITY, a runtime-compiled density without a gradient or of the term / pair
 * form, a density with blobs, or ndim > 32 (the chain lives in registers). */
typedef struct kmc_metropolis_config {
    int32_t  dtype;         /* KMC_F64 */
    int32_t  density;       /* kmc_density (menu or KMC_USER_DENSITY) */
    double   params[8];
    int64_t  nchains;       /* independent chains (the reference: 1) */
    int64_t  ndim;
    int64_t  niter;         /* steps per chain                      src/samplers.jl:62 */
    int64_t  nburnin;       /* discarded initial steps per chain    src/samplers.jl:63 */
    int64_t  nthin;         /*                                      src/samplers.jl:64 */
    const double* step;     /* host [ndim]: proposal scale per dimension (theta + step .* randn) */
    uint64_t seed;
    uint32_t flags;         /* KMC_STORE_CHAIN | KMC_STORE_LOGP | KMC_MOMENTS | KMC_STORE_BLOBS | KMC_CHAIN_BY_WALKER (chain [nchains][nsamples][ndim],
                               chain_logp [nchains][nsamples]: thetas[chain][sample], reordered on the device) */
    int32_t  device;
    void*    user_density;  /* kmc_user_density* when density == KMC_USER_DENSITY */
    /* Host route: ANY closure for `pdf` and / or `sample_ppdf` (the reference takes both as arbitrary functions,
       src/samplers.jl:59-61).  One iteration of all chains per round trip: proposals on the device (the Gaussian step) or
       from host_propose, their log-pdfs on the device (menu / runtime-compiled density) or from host_logpdf
       (density == KMC_HOST_DENSITY), the accept test (:101), counters and storage always on the device.  Launch- and
       PCIe-bound (tens of microseconds per iteration): the general route, not the fast one. */
    kmc_host_logpdf_fn   host_logpdf;   /* density == KMC_HOST_DENSITY: log-pdfs of a batch of rows, else NULL */
    void*                host_user;     /* passed to the three callbacks */
    kmc_host_accepted_fn host_accepted; /* optional: accept outcomes per iteration (blobs: :100-103, :116-118); row0 = 0, generation = iteration */
    kmc_host_propose_fn  host_propose;  /* optional: theta1 = sample_ppdf(theta0) for a batch of rows; `step` may then be NULL */
    const double* chol;     /* host [ndim][ndim] row-major, lower triangle read: the proposal theta + L z.  Exactly one of step / chol
                               is non-NULL (neither with host_propose) */
    int32_t  tune_rounds;   /* R >= 0: tuning boundaries during burn-in (0: none) */
    double   tune_scale;    /* 0: the default 2.38 / sqrt(ndim) */
    int32_t  hmc_nleap;     /* 0: off (the random walk above); 1 .. 1024: the HMC step, leapfrog steps per iteration; `step` then
                               holds the step sizes, every one finite and > 0 */
    double   hmc_jitter;    /* in [0, 1): the relative half-width of the per-iteration step-size jitter (0 without hmc_nleap) */
} kmc_metropolis_config;

typedef struct kmc_metropolis_outputs {
    double*  chain;         /* [nsamples][nchains][ndim]   thetas      (needs KMC_STORE_CHAIN)  :113 */
    double*  chain_logp;    /* [nsamples][nchains]         logdensities (needs KMC_STORE_LOGP)  :115 */
    double*  accept_ratio;  /* [nchains]                                                        :127 */
    int64_t* naccept;       /* [nchains] */
    double*  final_pos;     /* [nchains][ndim] */
    double*  final_logp;    /* [nchains] */
    double*  chain_sum;     /* [nchains][ndim] per-chain sum over the stored samples (needs KMC_MOMENTS) */
    double*  chain_sumsq;   /* [nchains][ndim] */
    int64_t  nsamples;      /* out: (niter - nburnin) / nthin   src/samplers.jl:88 */
    double   device_ms;     /* out: the sampling kernels only (HIP events) */
    double*  blobs;         /* [nsamples][nchains][nblob] ([nchains][nsamples][nblob] with KMC_CHAIN_BY_WALKER): the blob of every stored
                               sample (hasblob=true, src/samplers.jl:70-72, :103, :117) of a body density created with
                               kmc_user_density_create_body_blob; in-kernel chains only (no host_propose) */
    double*  final_blob;    /* [nchains][nblob]: blob0 of every chain at the end */
    double*  chol_out;      /* [ndim][ndim] or NULL: the L in force at the end (upper triangle 0.0); with `step` and no tuning, diag(step) */
    int64_t  tune_skipped;  /* out: tuning rounds whose covariance could not be factored (the previous L stayed) */
    double   tune_ms;       /* out: host time spent at the tuning boundaries (covariance kernels, copy, Cholesky, upload), all of them */
} kmc_metropolis_outputs;

/* Cholesky factor of a symmetric positive-definite matrix, host only, fixed operation order: row by row i = 0..n-1, within a row
 * j = 0..i; s = a[i][j], then s = s - L_ik L_jk for k = 0..j-1 ascending, each operation rounded on its own (no fused
 * multiply-add); j < i: L_ij = s / L_jj; j = i: s must be finite and > 0, else KMC_ERR_BAD_ARG with *bad = i, otherwise
 * L_ii = sqrt(s).  Only the lower triangle of `a` [n][n] is read; the upper triangle of L [n][n] is written as 0.0.  `bad` may be NULL;
 * it is -1 on success. */
kmc_status  kmc_cholesky_lower(const double* a, int n, double* L, int* bad);

/* Argument sanity only (the reference asserts nothing for metropolis).  No device needed. */
kmc_status  kmc_metropolis_validate(const kmc_metropolis_config* cfg);
kmc_status  kmc_metropolis_run(const kmc_metropolis_config* cfg, const double* theta0 /* host [nchains][ndim] */,
                               kmc_metropolis_outputs* out);

/* ---- convergence diagnostics: int_acorr / acor1d / auto_window, reference src/analysis.jl:140-167, :252-273, :280-285 ----
 * (that file is entirely commented out in the reference: the code is followed as written, there is no live behaviour to
 * match).  Integrated autocorrelation time per dimension of a chain as the samplers produce it, chain_host
 * [nsamples][nwalkers][ndim]: circular FFT autocorrelation of every walker's series normalised by its lag-0 value, first
 * nsamples/2 lags, averaged over walkers; tau = 2 cumsum(rho) - 1 at the first window M >= c tau(M); converged =
 * nsamples / tau (the reference suggests > 50).  All -1 if any value is NaN (:161-165).  Needs libhipfft.so at run time. */
kmc_status  kmc_int_acorr(const double* chain_host, int64_t nsamples, int64_t nwalkers, int64_t ndim, double c /* 5 */,
                          int device, double* tau /* [ndim] */, double* converged /* [ndim] */);
/* The same on the chain a sampler holds on the device (KMC_STORE_CHAIN, the samples stored so far; even ndim). */
kmc_status  kmc_sampler_int_acorr(kmc_sampler* s, double c, double* tau, double* converged);

/* ---- posterior summaries: exact order statistics and the MAP sample of a stored chain, on the device ----
 * What the summarize_run of reference src/analysis.jl:9-42 (commented out there) needs -- medians, and with them any quantile or
 * credible interval -- without moving the chain to the host.
 *
 * Order statistics.  The selection is the stored samples k >= first_sample of the walkers w with walker_mask[w] != 0 (all walkers when
 * walker_mask is NULL): N = (samples stored - first_sample) * popcount(mask) values per dimension, *n_out (may be NULL).  For each of
 * the nranks <= 16 ranks r (0-based, in [0, N), repeats allowed), theta_out[i][d] is the element of rank r_i of dimension d in
 * ascending order -- every dimension on its own, as np.sort(chain, axis=0)[r] -- and logp_out[i] (may be NULL; needs KMC_STORE_LOGP)
 * the same of the stored log-densities.  The results are elements of the chain, bit for bit (a KMC_F32 chain: its floats widened).
 * Order: a double maps to a 64-bit key, all bits flipped when its sign bit is set, else the sign bit flipped, and keys compare as unsigned
 * integers: -inf < ... < -0.0 < +0.0 < ... < +inf.  NaNs are ordered by bit pattern (a NaN with the sign bit clear above +inf, with
 * it set below -inf); a stored chain holds none.  Algorithm: most-significant-digit radix select, 8 passes of 8 bits over the selection,
 * every pass one read of it for all dimensions and ranks, integer atomics only.
 * KMC_ERR_BAD_ARG: no KMC_STORE_CHAIN; logp_out without KMC_STORE_LOGP; nranks outside 1..16; a rank outside [0, N); N = 0;
 * first_sample outside [0, samples stored].  KMC_ERR_UNSUPPORTED: KMC_STREAM_CHAIN (the chain is on the host: kmc_chain_order_stats);
 * shard_count > 1 or KMC_P2P (a shard holds only its own walkers; a select across GPUs is not built). */
kmc_status  kmc_sampler_order_stats(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask /* [nlocal] or NULL */,
                                    const int64_t* ranks, int32_t nranks,
                                    double* theta_out /* [nranks][ndim] */, double* logp_out /* [nranks] or NULL */, int64_t* n_out);
/* The MAP sample: (sample, walker) of the largest stored log-density of the same selection (needs KMC_STORE_LOGP), ties to the
 * smallest sample, then the smallest walker; NaN entries are ignored (all NaN: KMC_ERR_BAD_ARG).  theta gets that sample's row,
 * logp its log-density.  Refusals as above. */
kmc_status  kmc_sampler_chain_argmax(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask,
                                     int64_t* sample, int64_t* walker, double* theta /* [ndim] */, double* logp);
/* The same two on a chain in host memory, uploaded to `device` first (a streamed chain, Metropolis output).  logp_host may be NULL
 * when logp_out is.  KMC_ERR_UNSUPPORTED when the chain does not fit the device's free memory. */
kmc_status  kmc_chain_order_stats(const double* chain_host /* [nsamples][nwalkers][ndim] */, const double* logp_host /* or NULL */,
                                  int64_t nsamples, int64_t nwalkers, int64_t ndim, int64_t first_sample, const uint8_t* walker_mask,
                                  const int64_t* ranks, int32_t nranks, int device, double* theta_out, double* logp_out, int64_t* n_out);
kmc_status  kmc_chain_argmax(const double* chain_host, const double* logp_host, int64_t nsamples, int64_t nwalkers, int64_t ndim,
                             int64_t first_sample, const uint8_t* walker_mask, int device,
                             int64_t* sample, int64_t* walker, double* theta, double* logp);

/* ---- marginal histograms of a stored chain, on the device: every selected column's 1-D histogram and all pairs' 2-D histograms ----
 * The numbers of a corner plot without moving the chain to the host.  The selection (first_sample, walker_mask, N in *n_out) is that of
 * the order statistics above.  dims lists ndims distinct chain columns in the caller's order (NULL / 0: every dimension, in order); the
 * output columns are those, and with with_logp = 1 (needs KMC_STORE_LOGP) the stored log-densities as one more, last, column: ncols.
 * The rule.  edges[c] is column c's B + 1 = nbins + 1 finite, strictly increasing bin edges e[0..B].  An element x falls in bin i iff
 * e[i] <= x < e[i+1]; the last bin is closed, x == e[B] goes to bin B - 1.  x < e[0] counts in outside[c][0] (below), x > e[B] in
 * outside[c][1] (above), a NaN in outside[c][2]; -inf and +inf are ordinary values under these comparisons.  The bin is decided by
 * comparisons against the edges alone (a binary search), never by float arithmetic, so counts1[c] is np.histogram(x, bins=e)[0] for any
 * edges, and counts1[c] and outside[c] sum to N.  A KMC_F32 chain is widened first, which is exact.
 * counts2 (may be NULL) gets, for every pair (a, b), a < b, of positions in the dims list, in the order (0,1), (0,2), ..., (1,2), ...,
 * the 2-D histogram [bin of dims[a]][bin of dims[b]] of the rows whose two coordinates both lie inside their ranges:
 * np.histogram2d(x_a, x_b, bins=[e_a, e_b])[0].  Chain columns only (never the log-densities); it needs 2..16 selected dimensions and
 * nbins <= 64.  Counts are exact integers (integer atomics only) and do not depend on the launch geometry.
 * KMC_ERR_BAD_ARG: no KMC_STORE_CHAIN; with_logp without KMC_STORE_LOGP; nbins outside 1..256, or outside 1..64 with counts2; with
 * counts2 fewer than 2 or more than 16 selected dimensions; a dimension outside [0, ndim) or listed twice; edges that are not finite
 * and strictly increasing; N = 0; first_sample outside [0, samples stored].  KMC_ERR_UNSUPPORTED: as for the order statistics. */
kmc_status  kmc_sampler_histograms(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask /* [nlocal] or NULL */,
                                   const int32_t* dims, int32_t ndims, const double* edges /* [ncols][nbins + 1] */, int32_t nbins,
                                   int32_t with_logp, int64_t* counts1 /* [ncols][nbins] */, int64_t* outside /* [ncols][3] */,
                                   int64_t* counts2 /* NULL or [npairs][nbins][nbins] */, int64_t* n_out);
/* The same on a chain in host memory, uploaded to `device` first; every argument is checked before the device is touched.  The
 * log-densities are the last 1-D column exactly when logp_host is not NULL. */
kmc_status  kmc_chain_histograms(const double* chain_host /* [nsamples][nwalkers][ndim] */, const double* logp_host /* or NULL */,
                                 int64_t nsamples, int64_t nwalkers, int64_t ndim, int64_t first_sample, const uint8_t* walker_mask,
                                 const int32_t* dims, int32_t ndims, const double* edges, int32_t nbins, int device,
                                 int64_t* counts1, int64_t* outside, int64_t* counts2, int64_t* n_out);
/* How the 2-D kernel cuts the ndims (ndims - 1) / 2 pairs into groups whose counters (nbins^2 x 4 bytes a pair) share one workgroup's
 * LDS next to the edges and a tile of bin indices: the selection is read once per group.  *lds_budget: the bytes a workgroup may use.
 * Needs no device.  KMC_ERR_BAD_ARG unless 2 <= ndims <= 16 and 1 <= nbins <= 64. */
kmc_status  kmc_hist_pair_plan(int32_t ndims, int32_t nbins, int32_t* pairs_per_group, int32_t* ngroups, int32_t* lds_budget);

/* ---- convergence across chains of a stored chain, on the device: split-R^, effective sample size, Monte-Carlo standard error ----
 * The two columns of a summary table that ask whether the chains agree and how much the mean is worth (the evaluate_convergence and
 * error_of_estimated_mean that reference src/analysis.jl:79-95, :242-248 sketches, commented out, over MCMCDiagnostics.jl).  The
 * formulas below are the definition (BDA3: Gelman et al. 2014, pp. 284-287); no other implementation is followed.
 *
 * Chains.  The selection is that of the order statistics: the stored samples k >= first_sample of the walkers in the mask, nw walkers
 * and n samples.  Every selected walker is a chain; with split != 0 it is cut into halves of h = n / 2 samples, [first, first + h) and
 * [first + n - h, first + n) (an odd n leaves the middle sample out), chain j = half * nw + k for the k-th selected walker in ascending
 * order, m = 2 nw chains.  Without split h = n, m = nw.  h >= 4 and m >= 2, else KMC_ERR_BAD_ARG.
 * Columns: every dimension and, when asked (needs KMC_STORE_LOGP), the log-densities as the last: ncols.  Per column, with x[i][j]
 * sample i of chain j:
 *   mu_j, s2_j   chain means and variances; two passes, squares of x - mu_j, h - 1 in the denominator
 *   W = mean_j s2_j;  B / h = var_j(mu_j), m - 1 in the denominator;  var+ = ((h - 1) / h) W + B / h;  R^ = sqrt(var+ / W)
 *   D_t = sum_j sum_{i = t}^{h - 1} (x[i][j] - x[i - t][j])^2     (a pair never straddles the halves of a walker or reaches before
 *                                                                   first_sample)
 *   V_t = D_t / (m (h - t));  rho_t = 1 - V_t / (2 var+)
 *   T: walking T = 1, 3, 5, ...: stop with KMC_CONV_TRUNCATED if T + 2 > max_lag; else stop if rho_(T+1) + rho_(T+2) < 0; else T += 2
 *   ess = m h / (1 + 2 sum_{t = 1}^{T} rho_t), NaN unless the denominator is > 0;  mcse = sqrt(var+ / ess)
 *   mean = mean_j mu_j;  the standard deviation of the table is sqrt(var+)
 * NaN and +-inf in the chain propagate.  W == 0 (a constant chain) gives rhat = ess = mcse = NaN, T = 0, and no error.
 *
 * The device stage.  chain_mean and chain_var [ncols][m] (both or neither may be NULL) and lagsum[c][k] = D_(lag0 + k), k = 0 ..
 * nlags - 1, with 1 <= lag0 and lag0 + nlags - 1 <= h - 1 (nlags may be 0).  The chain is read where it lies: for each block of 32 lags
 * an element is loaded into a window in LDS once per tile as the leading sample of its pairs and at most twice as the trailing one,
 * not once per lag.  No floating-point atomics: workgroups write partial sums and a second kernel adds them in a
 * fixed order, so two identical calls return the same bits; each number is the sum of its terms, formed in double as written above, in
 * an order the library chooses.  Refusals as for the order statistics. */
#define KMC_CONV_NEED_LAGS 1   /* flags bit 0: the rule has not fired within the lags given (call again with more) */
#define KMC_CONV_TRUNCATED 2   /* flags bit 1: the rule has not fired up to max_lag */
kmc_status  kmc_sampler_lag_sums(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask /* [nlocal] or NULL */, int32_t split,
                                 int32_t with_logp, int64_t lag0, int64_t nlags, double* chain_mean, double* chain_var, double* lagsum,
                                 int64_t* m_out, int64_t* h_out);
/* The same on a chain in host memory, uploaded to `device` first; every argument is checked before the device is touched.  The
 * log-densities are the last column exactly when logp_host is not NULL. */
kmc_status  kmc_chain_lag_sums(const double* chain_host /* [nsamples][nwalkers][ndim] */, const double* logp_host /* or NULL */,
                               int64_t nsamples, int64_t nwalkers, int64_t ndim, int64_t first_sample, const uint8_t* walker_mask,
                               int32_t split, int64_t lag0, int64_t nlags, int device, double* chain_mean, double* chain_var,
                               double* lagsum, int64_t* m_out, int64_t* h_out);
/* The host stage; needs no device.  chain_mean, chain_var [ncols][m]; lagsum [ncols][nlags] holds D_1 .. D_nlags (0 <= nlags <= h - 1);
 * max_lag in [3, h - 1].  Fills, per column, mean, W, B, var_plus, rhat, ess, mcse, T and flags.  When the walk needs rho beyond
 * nlags, flags gets KMC_CONV_NEED_LAGS and ess, mcse are taken with the T reached so far: call again with more lags.  Every sum is
 * sequential in index order (j, then t) and (double)(h - 1) / (double)h is formed before the product with W, so a
 * restatement in another language gives the same bits.  KMC_ERR_BAD_ARG: a null pointer, ncols < 1, h < 4, m < 2, max_lag or nlags
 * outside their ranges. */
kmc_status  kmc_convergence_stats(int64_t m, int64_t h, int64_t ncols, const double* chain_mean, const double* chain_var,
                                  const double* lagsum, int64_t nlags, int64_t max_lag, double* mean, double* W, double* B,
                                  double* var_plus, double* rhat, double* ess, double* mcse, int64_t* T, int32_t* flags);
/* The whole thing in one call: the chain moments once, then 32, 64, 128, ... lags in all until every column's rule has fired or max_lag
 * (0: min(h - 1, 1024); else in [3, h - 1]) is reached.  Outputs [ncols] as above; info (may be NULL) gets 4 numbers for benchmarks: the
 * lags computed, the blocks of 32 lags run, the bytes of the chain the lag kernel loaded and those the moment kernels loaded. */
kmc_status  kmc_sampler_convergence(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int32_t split, int32_t with_logp,
                                    int64_t max_lag, double* mean, double* W, double* B, double* var_plus, double* rhat, double* ess,
                                    double* mcse, int64_t* T, int32_t* flags, int64_t* m_out, int64_t* h_out, int64_t* info);
/* The tile of the lag kernel: lags per block (32), leading samples per tile (32), lanes along the (walker, column) axis (64) and the
 * bytes of LDS one workgroup uses.  D_t has the same bits however its lags are cut into calls.  Needs no device; pointers may be NULL. */
kmc_status  kmc_convergence_plan(int32_t* lag_block, int32_t* tile_samples, int32_t* lanes, int32_t* lds_bytes);
kmc_status  kmc_chain_convergence(const double* chain_host, const double* logp_host /* or NULL */, int64_t nsamples, int64_t nwalkers,
                                  int64_t ndim, int64_t first_sample, const uint8_t* walker_mask, int32_t split, int64_t max_lag,
                                  int device, double* mean, double* W, double* B, double* var_plus, double* rhat, double* ess,
                                  double* mcse, int64_t* T, int32_t* flags, int64_t* m_out, int64_t* h_out, int64_t* info);
/* The tile of the lag kernel: lags per block (32), leading samples per tile (32), lanes along the (walker, column) axis (64) and the
 * bytes of LDS one workgroup uses.  D_t has the same bits however its lags are cut into calls.  Needs no device; pointers may be NULL. */
kmc_status  kmc_convergence_plan(int32_t* lag_block, int32_t* tile_samples, int32_t* lanes, int32_t* lds_bytes);

/* ---- rank-normalised R^ with bulk and tail effective sample sizes, ranked on the device ----
 * The R^ above is blind to chains that share a mean but differ in scale, is undefined for heavy tails, and its ess describes the mean
 * only.  Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021, Bayesian Analysis 16, 667-718) replace every draw by the normal score
 * of its rank among all draws and apply the same statistics to the scores, to the scores of the draws folded about the median, and to
 * the indicators of the 5 % and 95 % quantiles.  The formulas below are the definition.
 *
 * Selection and chains: as above (first_sample, walker_mask, split, chain j = half * nw + k, m chains of h samples; columns: every
 * dimension and, when asked, the log-densities as the last).  Everything is per column over the POOLED DRAWS, the S = m h elements that
 * belong to a chain; the middle sample that a split with an odd n leaves out is not among them.  S < 2^31.
 *
 * Rank.  By value, not by bits: x + 0.0 first, so that -0.0 ties with +0.0, then the key of the order statistics above; +-inf are
 * ordinary values.  rank2(x) = #{y < x} + #{y <= x} + 1, an int64 in [2, 2 S]; the average 1-based rank is r = rank2 / 2, and ties
 * share it.  A column whose selection holds a NaN gets NaN in every output below (and rank2 = 0) and the flag KMC_CONV_HAS_NAN; other
 * columns are unaffected.
 * Normal score.  p = (r - 0.375) / (S + 0.25): one correctly rounded division, everything before it exact.  z = Phi^-1(p) is Wichura's
 * AS 241 routine PPND16 in exactly the operation order of CPython's statistics._normal_dist_inv_cdf: q = p - 0.5;
 * |q| <= 0.425: r = 0.180625 - q q, two Horner sums in r, z = (num q) / den; else r = sqrt(-log(min(p, 1 - p))), r - 1.6 for r <= 5 and
 * r - 5 beyond, two Horner sums, z = -+ num / den.  No fused multiply-add on host or device: the central branch (about 85 % of the
 * draws) has the same bits everywhere, the tails differ only as far as the two logarithms do.
 * Transforms of a column:  bulk z(x);  folded z(|x - med|);  I05 = (x <= q05) and I95 = (x <= q95) as 0.0 / 1.0, where med, q05, q95
 * are the quantiles 0.5, 0.05 and 0.95 of the pooled draws by the rule of the order statistics with N = S: h = q (S - 1),
 * lo = floor(h), hi = min(lo + 1, S - 1), frac = h - lo, x_lo + frac (x_hi - x_lo) (x_lo itself where frac == 0), from two order
 * statistics each, read out of the sorted column.  inf - inf in the fold is a NaN of the folded column only: rhat_folded and rhat are
 * NaN and KMC_CONV_HAS_NAN is set.
 * Statistics: those of kmc_convergence_stats applied to the transformed columns.  rhat_bulk = rhat(z), rhat_folded = rhat(z folded),
 * rhat = max of the two (NaN if either is); ess_bulk = ess(z); ess_q05 = ess(I05), ess_q95 = ess(I95), ess_tail = min of the two (NaN
 * if either is).  The ess stays the variogram estimator above with its truncation rule; Stan's FFT / Geyer estimator is not followed.
 *
 * Algorithm.  The selection's keys are gathered column-contiguous, every column is sorted on its own by a
 * least-significant-digit radix sort (8 passes of 8 bits; digit counts per tile, an exclusive scan, a stable scatter; integer atomics in
 * LDS only, none in the scatter), and two binary searches per draw give rank2.  The sorted column is unique, so results do not depend on
 * the launch geometry: two identical calls return the same bits.  The transformed columns are a scratch chain on the device, read by
 * the kernels of the section above.  Work space: 16 B of keys per pooled draw and column, plus 8 B per transformed column (four of them
 * for the whole thing); KMC_ERR_UNSUPPORTED, naming the sizes, when that does not fit the device's free memory -- never a partial answer. */
#define KMC_CONV_HAS_NAN 4     /* flags bit 2: a NaN among the pooled draws of the column (or inf - inf in its fold) */
/* The shape of the sort: keys per workgroup tile, bits per digit, passes, and the bytes of LDS the scatter uses.  Needs no device. */
kmc_status  kmc_rank_plan(int32_t* tile_keys, int32_t* digit_bits, int32_t* passes, int32_t* lds_bytes);
/* The host form of the score: z[i] of rank2[i] among S draws, i < n.  Needs no device.  KMC_ERR_BAD_ARG: S < 1 or a rank2 outside [2, 2 S]. */
kmc_status  kmc_rank_normal_scores(const int64_t* rank2, int64_t n, int64_t S, double* z);
/* The device stage: rank2 and z [ncols][m][h] of the columns (folded = 0) or of the columns folded about their medians (folded = 1; then
 * centre [ncols] gets the medians, else it is left alone), and nan_count [ncols], the NaNs among the (folded) draws -- a column without a
 * median has none but NaNs.  Every output may be NULL.  Refusals as for kmc_sampler_lag_sums, before the device is touched. */
kmc_status  kmc_sampler_rank_scores(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask /* [nlocal] or NULL */, int32_t split,
                                    int32_t with_logp, int32_t folded, int64_t* rank2, double* z, double* centre, int64_t* nan_count,
                                    int64_t* m_out, int64_t* h_out);
kmc_status  kmc_chain_rank_scores(const double* chain_host /* [nsamples][nwalkers][ndim] */, const double* logp_host /* or NULL */,
                                  int64_t nsamples, int64_t nwalkers, int64_t ndim, int64_t first_sample, const uint8_t* walker_mask,
                                  int32_t split, int32_t folded, int device, int64_t* rank2, double* z, double* centre,
                                  int64_t* nan_count, int64_t* m_out, int64_t* h_out);
/* The whole thing.  Per column [ncols]: rhat, rhat_bulk, rhat_folded, ess_bulk, ess_tail, ess_q05, ess_q95, median, q05, q95; T [4][ncols],
 * the truncation lags of the four transforms (bulk, folded, I05, I95); flags [ncols], the OR of the four runs' flags and
 * KMC_CONV_HAS_NAN.  max_lag as for kmc_sampler_convergence.  info (may be NULL) gets 4 numbers for benchmarks: the lags computed, the
 * bytes the two sorts moved, and the bytes the lag kernel and the moment kernels loaded. */
kmc_status  kmc_sampler_rank_convergence(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int32_t split, int32_t with_logp,
                                         int64_t max_lag, double* rhat, double* rhat_bulk, double* rhat_folded, double* ess_bulk,
                                         double* ess_tail, double* ess_q05, double* ess_q95, double* median, double* q05, double* q95,
                                         int64_t* T, int32_t* flags, int64_t* m_out, int64_t* h_out, int64_t* info);
kmc_status  kmc_chain_rank_convergence(const double* chain_host, const double* logp_host /* or NULL */, int64_t nsamples, int64_t nwalkers,
                                       int64_t ndim, int64_t first_sample, const uint8_t* walker_mask, int32_t split, int64_t max_lag,
                                       int device, double* rhat, double* rhat_bulk, double* rhat_folded, double* ess_bulk,
                                       double* ess_tail, double* ess_q05, double* ess_q95, double* median, double* q05, double* q95,
                                       int64_t* T, int32_t* flags, int64_t* m_out, int64_t* h_out, int64_t* info);

/* ---- the effective sample size and Monte-Carlo standard error of quantiles, from bit-packed indicator chains ----
 * How many digits of a reported quantile mean anything.  Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021): the ess of the
 * indicator x <= q_p, then the width of a Beta-distributed rank interval read off the sorted draws.  The formulas below are the
 * definition (the construction of the paper, as posterior::mcse_quantile is understood to use it).
 *
 * Selection, chains and columns: as for kmc_sampler_lag_sums / kmc_sampler_rank_convergence (first_sample, walker_mask, split, chain
 * j = half * nw + k, m chains of h samples; columns: every dimension and, when asked, the log-densities as the last).  Everything is
 * per column over the pooled draws, S = m h of them, S < 2^31, h >= 4, m >= 2.
 * Probabilities: nprobs values p, 1 <= nprobs <= 16, each finite and strictly inside (0, 1); repeats are allowed.  Anything else is
 * KMC_ERR_BAD_ARG, naming the index and the value, before the device is touched.
 *
 * For column c and probability p:
 * 1. quantile.  q_p by the rule of the order statistics with N = S: h = p (S - 1), lo = floor(h), hi = min(lo + 1, S - 1),
 *    frac = h - lo, q_p = x_lo + frac (x_hi - x_lo), and x_lo itself where frac == 0; read out of the sorted column, by value as in the
 *    ranking (x + 0.0 first, +-inf ordinary values).  For p in {0.5, 0.05, 0.95}: kmc_sampler_rank_convergence's median, q05, q95, bit
 *    for bit.
 * 2. Indicator.  I[i][j] = (x[i][j] <= q_p), one bit per draw.
 * 3. Chain moments, from counts.  k_j = sum_i I[i][j]; mu_j = k_j / h; ss_j = k_j ((1 - mu_j)(1 - mu_j)) + (h - k_j)(mu_j mu_j);
 *    s2_j = ss_j / (h - 1).  Every operation rounded to double on its own, in this order, no fused multiply-add (kmc_indicator_moments).
 * 4. Lag counts.  D_t = #{(i, j) : t <= i < h, I[i][j] != I[i - t][j]}: for an indicator (x_i - x_(i-t))^2 is the XOR of two bits.  An
 *    integer, handed on as the double of that integer.  A pair never straddles the halves of a walker or reaches before first_sample.
 * 5. ess, T, flags: kmc_convergence_stats, unchanged, on (m, h, mu, s2, D), with the lag-doubling loop of kmc_sampler_convergence (32,
 *    64, 128, ... lags until every series' rule has fired, or max_lag).  A series with W == 0 -- the indicator that is 1 everywhere: a
 *    constant or two-valued column -- gives ess = NaN, T = 0 and no error.
 * 6. lower, upper, mcse.  A = ess p + 1, B = ess (1 - p) + 1; a = Bq(Phi(-1); A, B), b = Bq(Phi(1); A, B) with Bq the quantile
 *    function of the Beta distribution (kmc_beta_quantile), Phi(-1) = 0.15865525393145707, Phi(1) = 0.8413447460685429;
 *    i1 = max(floor(a S), 1) - 1, i2 = min(ceil(b S), S) - 1, the products rounded once (kmc_quantile_mcse_ranks); lower = sorted[i1],
 *    upper = sorted[i2], both elements of the chain bit for bit (up to the sign of zero); mcse = (upper - lower) / 2.  ess NaN or <= 0:
 *    lower = upper = mcse = NaN.  inf - inf gives NaN and is not an error.
 * 7. NaN.  A column whose selection holds a NaN gets NaN in every output, T = 0 and KMC_CONV_HAS_NAN; other columns are unaffected.
 *
 * Algorithm.  One gather and one sort of the rank statistics; the quantiles are picked and become the thresholds;
 * qind_pack reads the chain where it lies and writes, for every (p, c, chain), words of 64 consecutive samples (bit i & 63 of word
 * i >> 6 is I[i][j], the bits at and beyond h zero) and k_j; qind_lag_counts forms the XOR of each word with the series shifted by t (a
 * funnel of the words t >> 6 and (t >> 6) + 1 back), masks it to the valid pairs and adds its popcount into 64-bit counters by integer
 * adds only.  D_t is an exact integer: equal bits from equal calls, however the lags are cut into calls.  The Beta quantile and the
 * index rule are host stages; the second pick reads the sorted keys, which stay allocated until then.  Work space: the keys of one
 * sort (16 B per pooled draw and column), nprobs ncols m ceil(h / 64) words and the counters; KMC_ERR_UNSUPPORTED, naming the sizes,
 * when that does not fit -- never a partial answer.
 * Not built: the MCSE of the standard deviation and of the ends of a highest-density interval, the ess of the indicator of an interval
 * (ess_local), several GPUs, a streamed chain. */
/* The quantile function of Beta(A, B) at prob: the x with I_x(A, B) = prob.  Host only.  The algorithm is fixed: the regularised
 * incomplete beta function as x^A (1 - x)^B / (A B(A, B)) times the continued fraction of Numerical Recipes' betacf (modified Lentz,
 * ended when a factor is within 4.5e-16 of 1), taken for 1 - x with A and B exchanged when x >= (A + 1) / (A + B + 2); the logarithm
 * of the leading term by the C library's lgamma while A and B are below 10, by Stirling's series (five terms) for an argument from 10
 * on, and with both there in the form of TOMS 708's BRCOMP (lambda = A - (A + B) x and e - log(1 + e)), which forms nothing of the
 * size of A log x; inverted by Newton's iteration from mean -+ sd inside a bracket that every evaluation narrows, a bisection step
 * whenever Newton's leaves the bracket, until the step no longer changes x or the bracket's ends are neighbouring doubles, at most
 * 200 evaluations.  Equal inputs give equal bits on every run.  Works for A, B from 1 up to 2^31 + 1 and beyond.  The library's value
 * is the definition of a and b above; against scipy.special.betaincinv it differs by at most 1.5e-12 relatively over the grid of
 * tests/test_quantile_mcse_cpu.py.  KMC_ERR_BAD_ARG: prob outside (0, 1), A or B not finite or < 1. */
kmc_status  kmc_beta_quantile(double prob, double A, double B, double* x);
/* Step 6's ranks for S pooled draws: a, b, i1, i2 (0-based; each pointer may be NULL).  ess NaN or <= 0: a = b = NaN, i1 = i2 = -1, and
 * KMC_OK.  Host only.  KMC_ERR_BAD_ARG: S < 1 or >= 2^52, p outside (0, 1). */
kmc_status  kmc_quantile_mcse_ranks(int64_t S, double p, double ess, double* a, double* b, int64_t* i1, int64_t* i2);
/* Step 3: mu and s2 of an indicator with k ones among h samples.  Host only.  KMC_ERR_BAD_ARG: h < 2, k outside [0, h]. */
kmc_status  kmc_indicator_moments(int64_t h, int64_t k, double* mu, double* s2);
/* The tile shape of the indicator kernels: samples per word (64), threads per workgroup (256), the words of one (p, c) a workgroup of
 * qind_lag_counts stages in LDS (2048) and the bytes of LDS it uses.  Needs no device; pointers may be NULL. */
kmc_status  kmc_indicator_plan(int32_t* word_bits, int32_t* threads, int32_t* chunk_words, int32_t* lds_bytes);
/* The device stage alone: the indicators x <= thresholds[p][c] (thresholds [nprobs][ncols], any doubles; nothing is <= NaN), their counts
 * ones [nprobs][ncols][m] and the lag counts lagcount [nprobs][ncols][nlags], lagcount[.][.][k] = D_(lag0 + k); the lags must lie in
 * [1, h - 1], nlags may be 0.  No sort.  Refusals as for kmc_sampler_lag_sums (no KMC_STORE_CHAIN, with_logp without KMC_STORE_LOGP, a
 * streamed chain, a sharded or P2P sampler, an empty selection), and nprobs outside 1..16, before the device is touched. */
kmc_status  kmc_sampler_indicator_lags(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask /* [nlocal] or NULL */, int32_t split,
                                       int32_t with_logp, int32_t nprobs, const double* thresholds, int64_t lag0, int64_t nlags,
                                       int64_t* ones, uint64_t* lagcount, int64_t* m_out, int64_t* h_out);
kmc_status  kmc_chain_indicator_lags(const double* chain_host /* [nsamples][nwalkers][ndim] */, const double* logp_host /* or NULL */,
                                     int64_t nsamples, int64_t nwalkers, int64_t ndim, int64_t first_sample, const uint8_t* walker_mask,
                                     int32_t split, int32_t nprobs, const double* thresholds, int64_t lag0, int64_t nlags, int device,
                                     int64_t* ones, uint64_t* lagcount, int64_t* m_out, int64_t* h_out);
/* The whole thing.  [nprobs][ncols]: quantile, ess, mcse, lower, upper, T, flags (those of kmc_convergence_stats and KMC_CONV_HAS_NAN).
 * max_lag as for kmc_sampler_convergence.  info (may be NULL) gets 4 numbers for benchmarks: the lags computed, the bytes the sort
 * moved, the bytes qind_pack read and the words qind_lag_counts read. */
kmc_status  kmc_sampler_quantile_mcse(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int32_t split, int32_t with_logp,
                                      int64_t max_lag, int32_t nprobs, const double* probs, double* quantile, double* ess, double* mcse,
                                      double* lower, double* upper, int64_t* T, int32_t* flags, int64_t* m_out, int64_t* h_out,
                                      int64_t* info);
kmc_status  kmc_chain_quantile_mcse(const double* chain_host, const double* logp_host /* or NULL */, int64_t nsamples, int64_t nwalkers,
                                    int64_t ndim, int64_t first_sample, const uint8_t* walker_mask, int32_t split, int64_t max_lag,
                                    int32_t nprobs, const double* probs, int device, double* quantile, double* ess, double* mcse,
                                    double* lower, double* upper, int64_t* T, int32_t* flags, int64_t* m_out, int64_t* h_out,
                                    int64_t* info);

/* ---- highest-density intervals of a stored chain, scanned on the device ----
 * The narrowest interval that holds a given share of the draws of a column: what ArviZ's summary reports as hdi_3% / hdi_97% and the
 * interval people quote for a skewed posterior, where it differs from the equal-tailed one of two quantiles.  The definition is ArviZ's
 * unimodal rule (arviz.stats.stats._hdi) with the ties and the special values pinned; what follows is the definition.
 *
 * Draws.  Per column the N selected draws: the stored samples >= first_sample of the walkers in the mask, every one of them -- the N
 * of kmc_sampler_order_stats; no split into halves, no middle sample left out.  Columns: every dimension and, when asked, the
 * log-densities as the last.  The draws are sorted ascending by value as the rank sort above does it: zeros canonicalised (x + 0.0,
 * so -0.0 sorts and is reported as +0.0), +-inf ordinary values, a chain of floats (KMC_F32) widened exactly.  x_(0) <= ... <= x_(N-1).
 * Windows.  For a probability p, k = floor(p * N) evaluated in double as written; the windows are i = 0 .. N - k - 1 with the widths
 * w_i = x_(i+k) - x_(i) in double.
 * The rule.  The interval is [x_(i*), x_(i*+k)] with i* the window of the smallest width and, among equal widths, the smallest i.  A
 * NaN width (inf - inf) loses to every number; if every width is NaN, i* = 0.  A column with a NaN among its draws gets NaN for both
 * ends and i* = -1, and nan_count says how many; the other columns are unaffected.
 * Exactness.  Both ends are elements of the chain, bit for bit, up to the sign of zero.  w_i is never negative, so the order
 * "(is NaN, width, i)" is an unsigned compare of the bits of w (NaN mapped to all-ones) followed by i: a total order with a unique
 * minimum.  Nothing depends on the launch geometry; two identical calls return the same bits, and kmc_sampler_hdi equals kmc_chain_hdi
 * on the downloaded chain.
 *
 * Algorithm.  Gather and sort are those of the rank statistics on the unsplit selection, once for all
 * probabilities.  Then a workgroup of 256 lanes scans 4096 consecutive window starts of one sorted column, keeping per probability its
 * best (bits(w), i) in two 64-bit integers -- integer compares only, no atomics, no floating-point minimum -- and one wave per (column,
 * probability) takes the minimum of the tiles' partials.  Work space: the sort's 16 B of keys per draw and column, its counts, and 16 B
 * per (column, probability, tile); KMC_ERR_UNSUPPORTED, naming the sizes, when that does not fit -- never a partial answer.
 *
 * probs [nprob], 1 <= nprob <= 16, each with its own k.  lo, hi [nprob][ncols]; start [nprob][ncols] gets i*; *n_out (may be NULL)
 * gets N; nan_count [ncols] (may be NULL); info (may be NULL) gets 6 numbers for benchmarks: N, the tiles of the scan per column, the
 * bytes the scan loads (8 B per window start and 8 B per window and probability, times the columns), and the nanoseconds of the gather,
 * the sort, and the scan with its fold.  The sampler's route runs on the sampler's own stream.
 * KMC_ERR_BAD_ARG, naming the value: a prob that is not finite, <= 0 or >= 1; k < 1 (p N < 1) or k = N; nprob outside 1..16; N < 2; an
 * empty selection; a null probs, lo, hi or start.  KMC_ERR_UNSUPPORTED: N >= 2^31 or more than 65535 columns (the sort's limits).  The
 * other refusals are those of kmc_sampler_order_stats (no KMC_STORE_CHAIN, with_logp without KMC_STORE_LOGP, a streamed chain, a
 * sharded or P2P sampler, a host chain that does not fit).  All from the sizes, before the device is touched, but the work space.
 * A tempered sampler's chain is rung 0's.  Not built: ArviZ's multimodal intervals, circular variables, the MCSE of the ends, a column
 * subset, sorting in column groups when the work space does not fit, several GPUs. */
kmc_status  kmc_sampler_hdi(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask /* [nlocal] or NULL */, int32_t with_logp,
                            const double* probs, int32_t nprob, double* lo, double* hi, int64_t* start, int64_t* n_out, int64_t* nan_count,
                            int64_t* info);
/* The same on a chain in host memory, uploaded to `device` first.  The log-densities are the last column exactly when logp_host is
 * not NULL. */
kmc_status  kmc_chain_hdi(const double* chain_host /* [nsamples][nwalkers][ndim] */, const double* logp_host /* or NULL */,
                          int64_t nsamples, int64_t nwalkers, int64_t ndim, int64_t first_sample, const uint8_t* walker_mask,
                          const double* probs, int32_t nprob, int device, double* lo, double* hi, int64_t* start, int64_t* n_out,
                          int64_t* nan_count, int64_t* info);
/* k = floor(p * n) and the number of windows n - k for n draws, with the argument checks of the two calls above on n and p.  Needs
 * no device; pointers may be NULL. */
kmc_status  kmc_hdi_span(int64_t n, double p, int64_t* k, int64_t* nwindows);

/* ---- the posterior covariance and correlation matrix of a stored chain, summed on the device ----
 * What a corner plot only shows: the covariance of every pair of columns over the selection -- the Gaussian approximation of the
 * posterior, the shape a proposal, a re-parametrisation or a new starting ball is built from.
 *
 * Selection and columns are those of kmc_sampler_lag_sums without the split: the rows are the pairs (stored sample >= first_sample,
 * walker in the mask), n of them; the columns are the ndim coordinates and, when asked (needs KMC_STORE_LOGP), the log-densities as the
 * last: C = ncols.  With x[r][c] column c of row r:
 *   mean[c]   = (sum_r x[r][c]) / n
 *   cov[a][b] = (sum_r (x[r][a] - mean[a]) (x[r][b] - mean[b])) / (n - 1)      two passes: centred on the device's own mean
 *   corr[a][b] = cov[a][b] / (sqrt(cov[a][a]) * sqrt(cov[b][b]))                in exactly that operation order; the diagonal is 1.0
 *                                                                               exactly where the variance is finite and positive
 * cov is computed for a <= b and mirrored: cov[a][b] and cov[b][a] have the same bits.  A chain of floats (KMC_F32) is widened to double
 * exactly, element by element, and everything after that is double.  NaN and +-inf in a selected row propagate, by the IEEE rules, into
 * the entries of the columns they are in and into no others; a constant column has variance 0 and NaN correlations, and no error.  A
 * row that is not selected -- before first_sample, or of a walker outside the mask -- contributes nothing: its elements are replaced by a
 * select, never multiplied by zero, so a NaN there does no harm.
 *
 * The device stage.  Two passes over the chain where it lies, each writing per-wave partial sums that a second
 * kernel adds in a fixed order; no floating-point atomics.  The cross products are a SYRK on the double-precision matrix instruction
 * (v_mfma_f64_16x16x4_f64): columns in tiles of 16, 4 rows an instruction, operands loaded straight from the chain's
 * [sample][walker][ld] storage.  Up to 32 columns the chain is read once for the products; wider matrices read, per strip of up to
 * strip_tiles tile pairs, the columns of that strip's tiles.  Which wave takes which rows and the order of the fold follow from the
 * selection's shape (samples kept, walkers, mask) and C alone -- not from ld, float or double storage, the route or the device -- so two
 * identical calls return the same bits, and kmc_sampler_covariance equals kmc_chain_covariance on the downloaded chain bit for bit.
 * Each number is the sum of its terms, formed in double as written above, in an order the library and the instruction choose.
 *
 * mean [C], cov [C][C]; *n_out (may be NULL) gets n; info (may be NULL) gets 4 numbers for benchmarks: the rows walked (selected or
 * not), the partial sums per entry the fold added, the strips, and the bytes of the chain the kernels loaded, counted from the shapes.
 * KMC_ERR_UNSUPPORTED, naming the limit, for C > 1024; KMC_ERR_BAD_ARG for n < 2 or a null output; the other refusals are those of
 * kmc_sampler_lag_sums (no KMC_STORE_CHAIN, with_logp without KMC_STORE_LOGP, a streamed chain, a sharded or P2P sampler, an empty
 * selection, a host chain that does not fit), all before the device is touched. */
kmc_status  kmc_sampler_covariance(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask /* [nlocal] or NULL */,
                                   int32_t with_logp, double* mean, double* cov, int64_t* n_out, int64_t* info);
/* The same on a chain in host memory, uploaded to `device` first.  The log-densities are the last column exactly when logp_host is
 * not NULL. */
kmc_status  kmc_chain_covariance(const double* chain_host /* [nsamples][nwalkers][ndim] */, const double* logp_host /* or NULL */,
                                 int64_t nsamples, int64_t nwalkers, int64_t ndim, int64_t first_sample, const uint8_t* walker_mask,
                                 int device, double* mean, double* cov, int64_t* n_out, int64_t* info);
/* The cut of the product kernel for ncols columns: columns of a tile (16), tile pairs a wave keeps accumulators for (strip_tiles: one A
 * tile against up to that many B tiles), the strips -- 1 up to 32 columns (two tiles, three pairs, one read), else the sum over the A
 * tiles ta of ceil((ntiles - ta) / strip_tiles) -- and the rows of one block of a wave (the rows are dealt to the waves in blocks of
 * that many).  Needs no device; pointers may be NULL.  KMC_ERR_BAD_ARG for ncols < 1, KMC_ERR_UNSUPPORTED for ncols > 1024. */
kmc_status  kmc_cov_plan(int64_t ncols, int32_t* tile_cols, int32_t* strip_tiles, int32_t* nstrips, int32_t* rows_per_wave_block);
/* The host stage; needs no device.  cov [ncols][ncols] -> corr [ncols][ncols] and sd [ncols] (may be NULL) = sqrt(cov[a][a]), in the
 * operation order above, so that a restatement in another language gives the same bits.  corr must not overlap cov. */
kmc_status  kmc_cov_correlation(int64_t ncols, const double* cov, double* corr, double* sd);

/* ---- pointwise log-likelihoods of a data density over a stored chain; WAIC ----
 * What a model comparison needs from a fit with KMC_DATA_DENSITY, computed where the chain, the observations and the compiled term are.
 *
 * Rows: the stored samples first_sample, first_sample + thin, ... (thin >= 1) of the walkers in the mask, sample by sample, walkers
 * ascending: n rows, n >= 2.  Observations: the density's own J = ndata rows d_j, or, when `data` is not NULL, a held-out array
 * [ndata2][ncols2] uploaded for the call (ncols2 must be the density's ncols; J = ndata2).
 * Terms: l[r][j] = term(x_r, ndim, d_j, p), the user's term body as the sampler's kernels compile it (same source, -ffp-contract=off,
 * -O3): for a body of + - * only it equals a host evaluation bit for bit.  The prior takes no part.
 *
 * Per observation, two passes over the rows, the second centred on what the first found:
 *   pass 1:  M_j  = max_r l[r][j]   (exact; NaN when a term is NaN),     S1_j = sum_r l[r][j]
 *   pass 2:  E_j  = sum_r exp(l[r][j] - M_j)   (every row contributes 0.0 when M_j == -inf),
 *            V_j  = sum_r (l[r][j] - S1_j / n)^2
 * stats is [4][J]: M, S1, E, V.  The host stage (kmc_waic_stats; no device, every operation in this order, log and sqrt the C
 * library's, so that a restatement in another language gives the same bits):
 *   lppd_j   = M_j + (log(E_j) - log(n))
 *   p_waic_j = V_j / (n - 1)                  the sample variance: n - 1 as in BDA3 and the R package loo (ArviZ divides by n)
 *   elpd_j   = lppd_j - p_waic_j
 *   lppd, p_waic, elpd_waic: the sums over j by the data-density contract's pairwise tree in observation order
 *   se       = sqrt(J * tree_j((elpd_j - elpd_waic / J)^2) / (J - 1))          (NaN for J = 1)
 *   waic     = -2 * elpd_waic
 *   n_high   = #{j : p_waic_j > 0.4}  (loo's warning count);   n_nan = #{j : S1_j is NaN}
 * IEEE rules, no special case beyond the one of E_j: a NaN, or a +inf next to a -inf, among the terms of an observation makes S1_j
 * NaN, then every output of that observation is NaN and it counts in n_nan; a -inf among finite terms leaves lppd_j finite and makes
 * p_waic_j NaN; an observation whose terms are all -inf has lppd_j = -inf.  A row outside the selection is never visited.
 *
 * The device stage.  One observation per lane, its d_j in registers; the rows are cut into nruns runs of
 * run_len consecutive rows, from n and J alone (kmc_pointwise_plan).  A run is added up in row order from 0.0, the runs' partial
 * results in run order from 0.0, by a second kernel: no floating-point atomics.  So two identical calls return the same bits, the
 * selection (first_sample, thin, mask) gives the bits of the same call on the rows copied out, and kmc_sampler_pointwise_stats equals
 * kmc_chain_pointwise_stats on the downloaded chain bit for bit.  Each sum is within (n + 4) 2^-53 sum |term| of the exact sum of its
 * terms as computed.
 *
 * n_out (may be NULL) gets n; info (may be NULL) gets 6 numbers: the rows n, the runs, the terms evaluated (both passes), run_len, and
 * the nanoseconds of pass 1 and of pass 2 on the device (events around each pass's partial kernel and fold; for benchmarks).
 * KMC_ERR_BAD_ARG, naming the value: a sampler or density that is not a data density; ndim > 32; thin < 1; n < 2; first_sample
 * outside [0, samples stored]; held-out data with ncols2 != ncols or ndata2 outside 1 .. 2^30; a null output.  KMC_ERR_UNSUPPORTED:
 * n >= 2^40, and what the other chain read-outs refuse (no stored chain: KMC_ERR_BAD_ARG; a streamed chain; a sharded or P2P sampler;
 * a host chain that does not fit the device).  For a host chain all of these are decided before the device is touched.  A
 * likelihood-tempered sampler is fine: its chain is rung 0's, beta = 1. */
kmc_status  kmc_sampler_pointwise_stats(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask /* [nlocal] or NULL */,
                                        int64_t thin, const double* data /* [ndata2][ncols2] or NULL */, int64_t ndata2, int32_t ncols2,
                                        double* stats, int64_t* n_out, int64_t* info);
/* The same on a chain in host memory, uploaded to `device` first, for the data density `density` with its parameters params[6]. */
kmc_status  kmc_chain_pointwise_stats(kmc_user_density* density, const double* params, const double* chain_host /* [nsamples][nwalkers][ndim] */,
                                      int64_t nsamples, int64_t nwalkers, int64_t ndim, int64_t first_sample, const uint8_t* walker_mask,
                                      int64_t thin, const double* data, int64_t ndata2, int32_t ncols2, int device, double* stats,
                                      int64_t* n_out, int64_t* info);
/* The matrix itself for the observations [obs_first, obs_first + obs_count): out [n][obs_count], dense (the way to PSIS-LOO outside the
 * library).  Besides the refusals above, KMC_ERR_BAD_ARG for obs_count < 1 or a range outside [0, J), and KMC_ERR_UNSUPPORTED, naming
 * the size, for a matrix that does not fit the device's free memory. */
kmc_status  kmc_sampler_pointwise_loglike(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int64_t thin, const double* data,
                                          int64_t ndata2, int32_t ncols2, int64_t obs_first, int64_t obs_count, double* out, int64_t* n_out);
kmc_status  kmc_chain_pointwise_loglike(kmc_user_density* density, const double* params, const double* chain_host, int64_t nsamples,
                                        int64_t nwalkers, int64_t ndim, int64_t first_sample, const uint8_t* walker_mask, int64_t thin,
                                        const double* data, int64_t ndata2, int32_t ncols2, int64_t obs_first, int64_t obs_count, int device,
                                        double* out, int64_t* n_out);
/* The cut of the two passes for n rows and ndata observations: run r covers the rows [r run_len, min(n, (r + 1) run_len)), and there
 * are nruns of them; a wave carries `slots` runs side by side, each over lanes_per_run observations (64 and 1 from 64 observations up;
 * below, the next power of two >= ndata and 64 over it), so nwaves = ceil(nruns / slots) waves walk the rows, wave w with the runs
 * w slots .. w slots + slots - 1.  Needs no device; pointers may be NULL.  KMC_ERR_BAD_ARG for n < 2 or ndata outside 1 .. 2^30,
 * KMC_ERR_UNSUPPORTED for n >= 2^40. */
kmc_status  kmc_pointwise_plan(int64_t n, int64_t ndata, int64_t* run_len, int64_t* nruns, int32_t* lanes_per_run, int32_t* slots,
                               int64_t* nwaves);
/* The host stage; needs no device.  stats [4][J] -> lppd_j, p_waic_j, elpd_j [J] (each may be NULL) and totals [7]: lppd, p_waic,
 * elpd_waic, se, waic, n_high, n_nan.  KMC_ERR_BAD_ARG for J < 1, n < 2 or a null stats / totals. */
kmc_status  kmc_waic_stats(int64_t J, int64_t n, const double* stats, double* lppd_j, double* p_waic_j, double* elpd_j, double* totals);

/* ---- PSIS-LOO: Pareto-smoothed importance-sampling leave-one-out cross-validation of a data density ----
 * (Vehtari, Gelman & Gabry 2017; Vehtari, Simpson, Gelman, Yao & Gabry 2024.)  Rows, observations and terms l[r][j] are those of the
 * block above; the observations are always the density's own (a held-out observation has no leave-one-out), restricted to
 * [obs_first, obs_first + obs_count).  n >= 5.  The [n][J] matrix never exists: every pass recomputes the terms.
 *
 * Per observation j, over the n rows, with l_r = l[r][j]:
 *  1. Shift.  m_j = min_r l_r and x_r = m_j - l_r (<= 0, in double: the shifted log importance ratio).  When a term is NaN or m_j is
 *     not finite, every output of the observation is NaN (n_tail_j: -1) and it counts in n_nan.  l_r = +inf is an ordinary value
 *     (x_r = -inf, weight 0).
 *  2. Tail.  M = ceil(min(0.2 n, 3 sqrt(n / r_eff))), the products and the root in double as written (ArviZ's rule; kmc_psis_plan
 *     returns it).  Cut-off xc_j = max(log(DBL_MIN), x_[n-M-1]) with x_[i] the ascending order statistics, i.e. the (M+1)-th largest,
 *     found exactly.  The tail is {r : x_r > xc_j} (ArviZ's strict rule, not loo's positional one): ties with the cut-off stay out,
 *     n_tail_j <= M.
 *  3. Fit.  nt = n_tail_j.  nt <= 4: k = +inf, the tail keeps its raw weights.  Otherwise, with the tail ascending x_(1..nt) and
 *     e_i = exp(x_(i)) - exp(xc_j), Zhang & Stephens' estimator as ArviZ's _gpdfit writes it:  m_est = 30 + floor(sqrt(nt));
 *     b_i = (1 - sqrt(m_est / (i - 0.5))) / (3 e_[floor(nt/4 + 0.5) - 1]) + 1 / e_[nt-1], i = 1..m_est (0-based indices into e);
 *     kappa_i = mean_t log1p(-b_i e_t);  L_i = nt (log(-b_i / kappa_i) - kappa_i - 1);  w_i = 1 / sum_q exp(L_q - L_i); entries with
 *     w_i < 10 DBL_EPSILON are dropped and the rest divided by their sum;  b = sum w_i b_i;  kappa = mean_t log1p(-b e_t);
 *     sigma = -kappa / b;  k = (nt kappa + 5) / (nt + 10).
 *  4. Smoothing.  k finite: s_i = min(0, log(sigma expm1(-k log1p(-p_i)) / k + exp(xc_j))), p_i = (i - 0.5) / nt, given to the tail in
 *     sorted order; NaN where sigma is not finite and positive, which makes the observation NaN.  k not finite: s_i = x_(i).
 *  5. Result.  W_j = sum_{r outside the tail} exp(x_r) + sum_i exp(s_i),  N_j = (n - nt) + sum_i exp(s_i - x_(i)),
 *     elpd_loo_j = m_j + log(N_j / W_j):  ArviZ's logsumexp(log weights + l), with the raw product w_r p_r = exp(m_j) of a row outside
 *     the tail taken exactly instead of through two roundings.  p_loo_j = lppd_j - elpd_loo_j, lppd_j from the two passes of the block
 *     above over the same rows, run inside the same call.
 *  6. Host stage (kmc_loo_stats; no device, fixed order):  elpd_loo, p_loo, lppd: the data-density contract's pairwise tree over the
 *     observations in order;  se = sqrt(J tree_j((elpd_loo_j - elpd_loo / J)^2) / (J - 1));  looic = -2 elpd_loo;  n_nan = #{j :
 *     elpd_loo_j is NaN};  k_counts = #{k <= 0.5}, #{0.5 < k <= 0.7}, #{0.7 < k <= 1}, #{k > 1} (+inf in the last, NaN in none).
 *
 * Order of summation.  The sum outside the tail runs over the runs of kmc_pointwise_plan(n, J), J the density's own count whatever
 * the range: a run in row order from 0.0, the runs' partials in run order from 0.0.  The sums of steps 3 to 5 over a tail run in an
 * order that depends on its length alone: lane l of 256 adds the entries l, l + 256, ... from 0.0, and the 256 partials are folded by
 * halving (p[l] += p[l + h], h = 128 .. 1); b and the sum of the kept w_i are added in index order.  kmc_psis_smooth_host is the same
 * code compiled for the host (csrc/kmc_psis_fit.hpp), so it differs from the device in exp / log / log1p / expm1 alone.  No
 * floating-point atomics; the tail is collected through an integer cursor per observation and then sorted, the select counts in
 * integers.  So two identical calls return the same bits, a selection gives the bits of the same call on the rows copied out,
 * kmc_sampler_psis_loo equals kmc_chain_psis_loo on the downloaded chain, and the outputs of an observation depend neither on the
 * range asked for nor on workspace_bytes.
 *
 * The device stage.  Observations are worked in blocks whose tail buffer and counters fit workspace_bytes
 * (0: 1 GiB; at least 64 observations).  Per block 2 + 16 passes recompute the terms: the minimum, 16 digits of 4 bits of a radix
 * select on the bits of l - m_j, and the gather; then one workgroup per observation sorts the tail and fits.
 *
 * stats [4][obs_count]: elpd_loo_j, pareto_k, n_tail_j (as double; NaN where the observation is NaN), sigma_j.  lppd_j [obs_count].
 * info (may be NULL) gets 12 numbers: n, M, the blocks, the observations of a block, the nanoseconds of the minimum pass, of the 16
 * select passes, of the gather and of the fit (events; summed over the blocks), the terms of one recompute pass (n obs_count), the
 * log1p evaluations of the fit, the nanoseconds of the two statistics passes, and the runs.
 * Refusals: those of kmc_sampler_pointwise_stats, and KMC_ERR_BAD_ARG, naming the value, for r_eff not finite or <= 0, n < 5, obs_count
 * < 1 or a range outside [0, J); KMC_ERR_UNSUPPORTED for n >= 2^31 and for M > 4096, naming n / r_eff (the tail of one observation is
 * sorted in one workgroup's LDS): never a partial answer.  A per-observation r_eff, supplied or computed from the chain: the *_reff forms below.  Not built: ArviZ's
 * one r_eff from the parameters' ESS, mcse_elpd_loo, moment matching. */
kmc_status  kmc_sampler_psis_loo(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask /* [nlocal] or NULL */, int64_t thin,
                                 double r_eff, int64_t obs_first, int64_t obs_count, int64_t workspace_bytes, double* stats, double* lppd_j,
                                 int64_t* n_out, int64_t* info);
kmc_status  kmc_chain_psis_loo(kmc_user_density* density, const double* params, const double* chain_host /* [nsamples][nwalkers][ndim] */,
                               int64_t nsamples, int64_t nwalkers, int64_t ndim, int64_t first_sample, const uint8_t* walker_mask, int64_t thin,
                               double r_eff, int64_t obs_first, int64_t obs_count, int64_t workspace_bytes, int device, double* stats,
                               double* lppd_j, int64_t* n_out, int64_t* info);
/* Steps 1 and 2 alone, read out: tail [obs_count][tail_len], each row the tail's x ascending, padded with NaN; m_j, xc_j [obs_count];
 * n_tail_j [obs_count] (-1 where the observation is NaN, and then its row, m_j and xc_j are NaN).  Outputs other than tail may be
 * NULL.  tail_len holds the columns of `tail` on entry (size it by kmc_psis_plan; KMC_ERR_BAD_ARG when it is less than M) and M on
 * return. */
kmc_status  kmc_sampler_psis_tail(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int64_t thin, double r_eff, int64_t obs_first,
                                  int64_t obs_count, int64_t workspace_bytes, double* tail, double* m_j, double* xc_j, int32_t* n_tail_j,
                                  int64_t* tail_len, int64_t* n_out);
kmc_status  kmc_chain_psis_tail(kmc_user_density* density, const double* params, const double* chain_host, int64_t nsamples, int64_t nwalkers,
                                int64_t ndim, int64_t first_sample, const uint8_t* walker_mask, int64_t thin, double r_eff, int64_t obs_first,
                                int64_t obs_count, int64_t workspace_bytes, int device, double* tail, double* m_j, double* xc_j,
                                int32_t* n_tail_j, int64_t* tail_len, int64_t* n_out);
/* The cut of a call; needs no device; pointers may be NULL.  tail_len = M, m_est = 30 + floor(sqrt(M)) (the largest grid of a fit),
 * obs_per_block (a multiple of 64: workspace_bytes over the bytes of one observation, 8 M + 72 nruns + 72), passes = 18 recompute
 * passes per block.  Refuses what the calls refuse from n and r_eff, ndata outside 1 .. 2^30 and workspace_bytes < 0. */
kmc_status  kmc_psis_plan(int64_t n, int64_t ndata, double r_eff, int64_t workspace_bytes, int64_t* tail_len, int64_t* m_est,
                          int64_t* obs_per_block, int64_t* passes);
/* Step 6; needs no device.  stats [4][J] and lppd_j [J] -> p_loo_j [J] (may be NULL) and totals [10]: elpd_loo, se, p_loo, looic,
 * lppd, n_nan, k_counts[4].  KMC_ERR_BAD_ARG for J < 1, n < 5 or a null argument. */
kmc_status  kmc_loo_stats(int64_t J, int64_t n, const double* stats, const double* lppd_j, double* p_loo_j, double* totals);
/* Steps 3 and 4 for one observation on the host: x [nt] the tail ascending, every x_i in (xc, 0]; k_hat, sigma, s [nt] and sums [2] =
 * sum_i exp(s_i), sum_i exp(s_i - x_(i)) (k_hat, sigma, sums may be NULL).  KMC_ERR_BAD_ARG, naming the value, for nt outside
 * 0 .. 4096 or a tail that is not ascending within (xc, 0]. */
kmc_status  kmc_psis_smooth_host(int64_t nt, const double* x, double xc, double* k_hat, double* sigma, double* s, double* sums);

/* ---- PSIS-LOO's relative efficiency, per observation, from the chain ----
 * The tail length of step 2 wants r_eff = ESS / n of the importance weights.  For observation j that series is the likelihood
 * exp(l[r][j]) over the selected rows; the library takes
 *     v[k][j] = exp(l[k][j] - M_j),   M_j = max_r l[r][j] exactly (pass 1 of the block above),
 * in the library's row order (sample by sample, selected walkers ascending), and defines
 *     r_eff_j = ess_j / (m h)
 * with ess, m and h exactly those of the convergence contract (kmc_sampler_convergence) on the series v[.][.][j] read as `nsel` chains
 * of n / nsel samples: split (default on) halves each chain (an odd count leaves the middle sample out), max_lag 0 means
 * min(h - 1, 1024).  The effective sample size is invariant under a scale, so this is loo's relative_eff(exp(log_lik)) under the
 * library's BDA3 estimator; the shift by M_j only keeps exp in range.  r_eff_j is NaN where ess is NaN (a constant column, or a NaN
 * in the column) and may exceed 1.  For ensemble chains it is usually well below 1.
 *
 * IEEE rules of v: a column whose M_j is NaN or -inf is all NaN; l = -inf under a finite M_j gives 0.0; the arg-max rows give exactly
 * 1.0.  Elsewhere v is the device's exp of the rounded difference.
 *
 * The device stage.  v is written in groups of 64 observations aligned to the absolute index (group g: observations [64 g, 64 g + 64),
 * laid out [n][64]), as many groups at a time as workspace_bytes holds (0: 1 GiB; at least one), and each group goes through the
 * convergence kernels as a chain of ld = 64 where it lies.  With ld = 64 every lane of the lag kernel owns one column, and the grid
 * depends on the shape of the selection alone: the bits of an observation's outputs depend neither on the range asked for, nor on
 * the other observations, nor on workspace_bytes, and equal kmc_chain_convergence on the group's v padded to 64 columns.
 *
 * r_eff_j, ess_j, T_j (the lag the rule stopped at), flags_j (KMC_CONV_TRUNCATED): each [obs_count] or NULL, but r_eff_j.  info (may
 * be NULL) gets 6 numbers: n, the groups, the nanoseconds of pass 1, of the weight passes and of the ESS stage (chain moments, lag
 * blocks and their copies, per group), and h.  Refusals: those of kmc_sampler_pointwise_loglike and of kmc_sampler_convergence (h < 4,
 * m < 2, max_lag outside [3, h - 1]) in their words, from the sizes, before the device is touched where the sizes suffice; and
 * KMC_ERR_UNSUPPORTED, with the byte count, when one group of 64 n doubles does not fit the device's free memory. */
kmc_status  kmc_sampler_relative_eff(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask /* [nlocal] or NULL */, int64_t thin,
                                     int64_t obs_first, int64_t obs_count, int32_t split, int64_t max_lag, int64_t workspace_bytes,
                                     double* r_eff_j, double* ess_j, int64_t* T_j, int32_t* flags_j, int64_t* m_out, int64_t* h_out, int64_t* n_out,
                                     int64_t* info);
kmc_status  kmc_chain_relative_eff(kmc_user_density* density, const double* params, const double* chain_host /* [nsamples][nwalkers][ndim] */,
                                   int64_t nsamples, int64_t nwalkers, int64_t ndim, int64_t first_sample, const uint8_t* walker_mask, int64_t thin,
                                   int64_t obs_first, int64_t obs_count, int32_t split, int64_t max_lag, int64_t workspace_bytes, int device,
                                   double* r_eff_j, double* ess_j, int64_t* T_j, int32_t* flags_j, int64_t* m_out, int64_t* h_out, int64_t* n_out,
                                   int64_t* info);
/* The series itself, read out: v [n][obs_count] dense and M_j [obs_count] (may be NULL), for the observations (the density's own, or
 * the held-out `data`) [obs_first, obs_first + obs_count).  The refusals of kmc_sampler_pointwise_loglike. */
kmc_status  kmc_sampler_pointwise_weights(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int64_t thin, const double* data,
                                          int64_t ndata2, int32_t ncols2, int64_t obs_first, int64_t obs_count, double* v, double* M_j,
                                          int64_t* n_out);
kmc_status  kmc_chain_pointwise_weights(kmc_user_density* density, const double* params, const double* chain_host, int64_t nsamples,
                                        int64_t nwalkers, int64_t ndim, int64_t first_sample, const uint8_t* walker_mask, int64_t thin,
                                        const double* data, int64_t ndata2, int32_t ncols2, int64_t obs_first, int64_t obs_count, int device,
                                        double* v, double* M_j, int64_t* n_out);
/* PSIS-LOO with a tail length per observation: kmc_*_psis_loo and kmc_*_psis_tail with r_eff_j [obs_count] in place of the one r_eff,
 * or NULL to compute it from the chain as above with `split` and `max_lag`.  M_j = ceil(min(0.2 n, 3 sqrt(n / r))) with r = r_eff_j
 * where that is finite and > 0 and 1.0 elsewhere (a computed NaN; counted in n_reff_nan).  Step 2 uses M_j for observation j; nothing
 * else changes, so r_eff_j all equal to r returns the bits of the scalar call with r, and NULL returns the bits of the call with the
 * computed r_eff_j (NaN replaced by 1) supplied.  r_eff_used [obs_count]: as computed (NaN kept) or as supplied; tail_len_j
 * [obs_count]: M_j; n_reff_nan; each may be NULL.  info as kmc_sampler_psis_loo with info[1] = max_j M_j and four more numbers, 16 in
 * all: the nanoseconds of the weight passes and of the ESS stage, the groups, n_reff_nan.  For the tails, tail_len holds the columns of
 * `tail` on entry and max_j M_j on return, the length of its rows then (KMC_ERR_BAD_ARG when it is less; min(4096, ceil(0.2 n))
 * always suffices).
 * Refusals besides those of the scalar calls and of kmc_sampler_relative_eff: KMC_ERR_BAD_ARG, naming the index, for a supplied entry
 * that is not finite and > 0, before the device is touched; KMC_ERR_UNSUPPORTED for max_j M_j > 4096, naming the observation and its
 * r_eff_j (thin the chain): with r_eff = 0.1, n = 200 000 already asks for 4 243. */
kmc_status  kmc_sampler_psis_loo_reff(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int64_t thin,
                                      const double* r_eff_j /* [obs_count] or NULL */, int32_t split, int64_t max_lag, int64_t obs_first,
                                      int64_t obs_count, int64_t workspace_bytes, double* stats, double* lppd_j, double* r_eff_used,
                                      int64_t* tail_len_j, int64_t* n_reff_nan, int64_t* n_out, int64_t* info);
kmc_status  kmc_chain_psis_loo_reff(kmc_user_density* density, const double* params, const double* chain_host, int64_t nsamples, int64_t nwalkers,
                                    int64_t ndim, int64_t first_sample, const uint8_t* walker_mask, int64_t thin, const double* r_eff_j,
                                    int32_t split, int64_t max_lag, int64_t obs_first, int64_t obs_count, int64_t workspace_bytes, int device,
                                    double* stats, double* lppd_j, double* r_eff_used, int64_t* tail_len_j, int64_t* n_reff_nan, int64_t* n_out,
                                    int64_t* info);
kmc_status  kmc_sampler_psis_tail_reff(kmc_sampler* s, int64_t first_sample, const uint8_t* walker_mask, int64_t thin, const double* r_eff_j,
                                       int32_t split, int64_t max_lag, int64_t obs_first, int64_t obs_count, int64_t workspace_bytes, double* tail,
                                       double* m_j, double* xc_j, int32_t* n_tail_j, int64_t* tail_len, double* r_eff_used, int64_t* tail_len_j,
                                       int64_t* n_reff_nan, int64_t* n_out);
kmc_status  kmc_chain_psis_tail_reff(kmc_user_density* density, const double* params, const double* chain_host, int64_t nsamples, int64_t nwalkers,
                                     int64_t ndim, int64_t first_sample, const uint8_t* walker_mask, int64_t thin, const double* r_eff_j,
                                     int32_t split, int64_t max_lag, int64_t obs_first, int64_t obs_count, int64_t workspace_bytes, int device,
                                     double* tail, double* m_j, double* xc_j, int32_t* n_tail_j, int64_t* tail_len, double* r_eff_used,
                                     int64_t* tail_len_j, int64_t* n_reff_nan, int64_t* n_out);

/* ---- diagnostics ----
 * The random side of the accept test of reference src/samplers.jl:260, "(N-1)*log(z) + p1 - p0 >= log(rand())", exactly as
 * the half-step kernels compute it, for walkers walker0 .. walker0 + n - 1 of one step (= 2 * generation + half): the partner
 * index (:250; may be NULL), z (:252), t1 = (ndim - 1) * log z and lu = log u, into host arrays.  The kernels take the two
 * logarithms from their own < 1 ulp routine, a CPU implementation from its libm: this export lets a test measure that gap
 * and the probability that it flips an accept decision (tests/test_gpu_accept_margin.py). */
kmc_status  kmc_debug_accept_terms(uint64_t seed, uint64_t step, uint64_t walker0, int64_t n, int64_t nhalf, double a_scale,
                                   int64_t ndim, int device, int64_t* partner_host, double* z_host, double* t1_host, double* lu_host);
/* The chain read-out kernels on the caller's data, through the launch code the library itself uses, so that a test can compare
 * them element by element with a host transposition at row lengths no sampler of a testable size reaches
 * (tests/test_gpu_readout_kernels.py).  src_host is a chain [K][nl][ld] of float (is_float = 1) or double, nd <= ld of every row
 * meaningful; dst_host [dst_len] is uploaded as the initial content of the destination, then walkers [w0, w0 + nw) are written as
 * dst[w * dst_stride + k * nd + c] = src[k][w0 + w][c], and all dst_len doubles come back: what the kernel must not touch keeps
 * the caller's values.  KMC_ERR_BAD_ARG, before the device is touched, unless K, nl, nw, nd >= 1, ld >= nd, 0 <= w0,
 * w0 + nw <= nl, dst_stride >= K * nd, dst_len >= (nw - 1) * dst_stride + K * nd, and nl, ld < 2^31. */
kmc_status  kmc_debug_chain_by_walker(const void* src_host, int is_float, int64_t K, int64_t nl, int64_t ld, int64_t nd, int64_t w0,
                                      int64_t nw, int64_t dst_stride, double* dst_host, int64_t dst_len, int device);
/* The same for the compaction of padded rows (a streamed chain of odd ndim): src_host [rows][ld] -> dst[r * nd + c] = src[r][c],
 * c < nd; needs dst_len >= rows * nd. */
kmc_status  kmc_debug_rows_compact(const double* src_host, int64_t rows, int64_t ld, int64_t nd, double* dst_host, int64_t dst_len,
                                   int device);
/* 1 when the library holds the phase-specialised (credit) instance of the lane-striped stretch kernel (double rows of exact size, one GPU)
 * for a menu density in the geometry L lanes x K chunks, iter walkers per group; else 0.  Needs no GPU. */
int         kmc_debug_phase_spec(int density, int L, int K, int iter);
/* Waves per workgroup of the workgroup-shared-draws instance of that kernel (burn-in replays of the updated-graph launch mode: one wave draws for
 * the whole workgroup) for a menu density in that geometry; 0 where the library holds none.  Needs no GPU. */
int         kmc_debug_shared_draws(int density, int L, int K, int iter);
/* The kernel variant behind a replay of n generations from generation g0 on, for a menu-density sampler of nwalkers x ndim (double rows, one GPU,
 * stretch move) on the two-launch route in the updated-graph launch mode: 0 the generic kernel, 1 the phase-specialised (credit) instance, 2 the
 * workgroup-shared-draws instance of burn-in.  moments / chain != 0: the sampler credits streaming moments / stores a chain.  Follows KMC_PLAN and
 * KMC_DEBUG (spec=0, share=0) as a sampler does.  Needs no GPU. */
int         kmc_debug_replay_variant(int density, int64_t nwalkers, int64_t ndim, int64_t nburnin, int64_t g0, int64_t n, int moments, int chain);

#ifdef __cplusplus
}
#endif
#endif /* KISSMCMC_HIP_H */
