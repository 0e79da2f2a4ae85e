# KissMCMCHIP.jl -- thin `ccall` shim over libkissmcmc_hip.so (C ABI: include/kissmcmc_hip.h).
#
# EXTENDS KissMCMC.jl, it does not replace it: `emcee` and `metropolis` get one more method each -- for a `pdf` that is
# one of the device log-densities below (menu, `ExprDensity`) or a `HostLogPdf(f)` around any Julia callable (that one
# stays on the host, KMC_HOST_DENSITY: called on each half-step's batch of proposals while moves, draws, accept test
# and storage run on the GPU) -- with KissMCMC's own keywords and return values (reference src/samplers.jl:188-216,
# :59-77).  `make_theta0s` (src/samplers.jl:311-349) and `squash_walkers` (:372-428) are host-side pre/post-processing
# on exactly the containers these methods take and return, so they are KissMCMC's OWN functions, re-exported here, not
# re-implemented: a device log-density is callable on the host with the kernels' formula, which is all `make_theta0s`
# needs.  A plain closure as `pdf` still dispatches to KissMCMC's CPU methods; wrap it, `HostLogPdf(f)`, to move the
# sampler to the GPU.  There is no CPU fallback inside this module.
#
# A package (julia/Project.toml, julia/test/runtests.jl: `] dev path/to/kissmcmc.jl_amd/julia`, `] test KissMCMCHIP` on a machine with Julia and an MI355X).
# NOT EXECUTED in the build environment (no julia binary there).  Every call it makes is mirrored 1:1 by the Python
# ctypes host (kissmcmc.jl_amd/_lib.py, api.py), which is what the tests drive; struct layouts are checked against the
# library when the module loads (`__init__`).
module KissMCMCHIP

import KissMCMC
import KissMCMC: emcee, metropolis, make_theta0s, squash_walkers     # extended (emcee, metropolis) / re-exported as they are

export emcee, make_theta0s, squash_walkers, metropolis, metropolis_chains, GaussianStep, HostProposal, int_acorr, quantiles, map_sample, histograms, corner, convergence, rank_convergence, rank_scores, quantile_mcse, hdi, covariance, waic, pointwise_loglike, loo, compare_loo, relative_eff, GaussianIso, Exponential, Rosenbrock, LogNormal, MvNormal2, ExprDensity, CDensity, DataDensity, HostLogPdf

using LinearAlgebra: inv

const LIB = get(ENV, "KMC_LIB_PATH", joinpath(@__DIR__, "..", "..", "libkissmcmc_hip.so"))     # julia/src/ -> the package directory that holds the built library

# ---- C structs: field for field include/kissmcmc_hip.h (kmc_config, kmc_outputs).  Built by keyword, so a new field
#      of the header needs one line here and no call site changes; `__init__` compares sizeof with the library's.
#      (They come first: a ccall's argument types are resolved when the enclosing method is defined.) ---
Base.@kwdef struct KmcConfig
    dtype::Int32 = 0                                  # KMC_F64 = 0, KMC_F32 = 1
    density::Int32 = 0
    params::NTuple{8,Float64} = ntuple(_ -> 0.0, 8)
    nwalkers::Int64 = 0
    ndim::Int64 = 0
    ngenerations::Int64 = 0
    nburnin::Int64 = 0
    nthin::Int64 = 1
    a_scale::Float64 = 2.0
    seed::UInt64 = 0
    flags::UInt32 = 0
    device::Int32 = 0
    shard_rank::Int32 = 0
    shard_count::Int32 = 1
    user_density::Ptr{Cvoid} = C_NULL
    island_gens::Int32 = 0                            # KMC_ISLANDS (opt-in island mode); 0 = defaults
    island_size::Int32 = 0
    host_logpdf::Ptr{Cvoid} = C_NULL                  # KMC_HOST_DENSITY callback ...
    host_user::Ptr{Cvoid} = C_NULL                    # ... and its context
    host_accepted::Ptr{Cvoid} = C_NULL                # KMC_HOST_DENSITY: accept outcomes per half-step (blobs), or NULL
    deal_rank::Int32 = 0                              # dealt sub-ensembles (multi-GPU, opt-in); deal_count = 0: off
    deal_count::Int32 = 0
    temper_mode::Int32 = 0                            # what a ladder tempers: KMC_TEMPER_WHOLE = 0, KMC_TEMPER_LIKELIHOOD = 1 (data densities)
    temper_pad_::Int32 = 0
    adapt_until::Int64 = 0                            # adaptive ladder: the sweeps of generations < adapt_until adapt it; 0 -> nburnin
    adapt_lag::Float64 = 0.0                          # ptemcee's adaptation_lag (rounds): finite, > 0
    adapt_time::Float64 = 0.0                         # ptemcee's adaptation_time: finite, > 0
    adapt::Int32 = 0                                  # 1: adapt the interior rungs during burn-in (ntemps >= 3, swap_every >= 1)
    adapt_pad_::Int32 = 0
    snooker_gamma::Float64 = 0.0                      # KMC_MOVE_SNOOKER: 0 -> 1.7
    mix_count::Int32 = 0                              # KMC_MOVE_MIX: 2 .. 4 members (the header's mix_move[4] ... mix_sigma[4], member by member)
    mix_move0::Int32 = 0
    mix_move1::Int32 = 0
    mix_move2::Int32 = 0
    mix_move3::Int32 = 0
    mix_pad0_::Int32 = 0
    mix_pad1_::Int32 = 0
    mix_pad2_::Int32 = 0
    mix_weight0::Float64 = 0.0
    mix_weight1::Float64 = 0.0
    mix_weight2::Float64 = 0.0
    mix_weight3::Float64 = 0.0
    mix_gamma0::Float64 = 0.0                         # a member's gamma0 (DE; 0 -> 2.38 / sqrt(2 ndim)) or gamma (snooker; 0 -> 1.7)
    mix_gamma1::Float64 = 0.0
    mix_gamma2::Float64 = 0.0
    mix_gamma3::Float64 = 0.0
    mix_sigma0::Float64 = 0.0                         # a DE member's sigma
    mix_sigma1::Float64 = 0.0
    mix_sigma2::Float64 = 0.0
    mix_sigma3::Float64 = 0.0
    betas::Ptr{Float64} = C_NULL                      # parallel tempering: [ntemps] inverse temperatures (copied at creation), betas[1] == 1, decreasing
    ntemps::Int32 = 0                                 # rungs of the ladder; 0 or 1 = off
    swap_every::Int32 = 0                             # generations between swap sweeps; 0 = never
    move::Int32 = 0                                   # KMC_MOVE_STRETCH = 0 (the reference's move), KMC_MOVE_DE = 1 (opt-in)
    move_pad_::Int32 = 0
    de_gamma0::Float64 = 0.0                          # KMC_MOVE_DE: 0 -> 2.38 / sqrt(2 ndim)
    de_sigma::Float64 = 0.0                           # KMC_MOVE_DE: relative jitter of gamma
end

Base.@kwdef mutable struct KmcOutputs
    chain::Ptr{Float64} = C_NULL
    chain_logp::Ptr{Float64} = C_NULL
    accept_ratio::Ptr{Float64} = C_NULL
    naccept::Ptr{Int64} = C_NULL
    final_pos::Ptr{Float64} = C_NULL
    final_logp::Ptr{Float64} = C_NULL
    sum::Ptr{Float64} = C_NULL
    sumsq::Ptr{Float64} = C_NULL
    nmoment::Int64 = 0
    nsamples::Int64 = 0
    device_ms::Float64 = 0.0
    blobs::Ptr{Float64} = C_NULL
end

const KMC_STORE_CHAIN = UInt32(1) << 0
const KMC_STORE_LOGP = UInt32(1) << 1
const KMC_CHAIN_BY_WALKER = UInt32(1) << 12     # chain delivered as [walker][sample][dim]: thetas[w][k] are contiguous
const KMC_MOVE_STRETCH = Int32(0)              # kmc_config.move: the reference's stretch move (default)
const KMC_MOVE_DE = Int32(1)                   # ... the opt-in differential-evolution move (one GPU, double rows)
const KMC_TEMPER_WHOLE, KMC_TEMPER_LIKELIHOOD = Int32(0), Int32(1)   # kmc_config.temper_mode: what a ladder tempers (the likelihood only: data densities)
const KMC_MOVE_SNOOKER, KMC_MOVE_MIX = Int32(3), Int32(4)   # ... the opt-in DE snooker update (ndim >= 2), and a weighted mixture of DE / snooker members
const KMC_STORE_BLOBS = UInt32(1) << 13         # a CDensity(body; nblob=m): the blob of every stored sample (src/samplers.jl:270, :117)

last_error() = unsafe_string(ccall((:kmc_last_error, LIB), Cstring, ()))

# ---- menu densities: callable on the host with the same formula the kernels use ----------------
abstract type DeviceLogPdf end
struct GaussianIso <: DeviceLogPdf; mu::Float64; sigma::Float64; end
GaussianIso() = GaussianIso(0.0, 1.0)
struct Exponential <: DeviceLogPdf; rate::Float64; end
Exponential() = Exponential(1.0)
struct Rosenbrock <: DeviceLogPdf; a::Float64; b::Float64; scale::Float64; end
Rosenbrock() = Rosenbrock(1.0, 100.0, 20.0)
struct LogNormal <: DeviceLogPdf; mu::Float64; sigma::Float64; end
struct MvNormal2 <: DeviceLogPdf; mean::Vector{Float64}; prec::Matrix{Float64}; end
MvNormal2(mean, cov::AbstractMatrix) = MvNormal2(collect(Float64, mean), inv(Matrix{Float64}(cov)))

(d::GaussianIso)(x) = -0.5 * sum(((x .- d.mu) ./ d.sigma) .^ 2)
(d::Exponential)(x) = any(x .< 0) ? -Inf : -d.rate * sum(x)          # README.md:15
(d::Rosenbrock)(x) = -sum(d.b .* (x[2:end] .- x[1:end-1] .^ 2) .^ 2 .+ (d.a .- x[1:end-1]) .^ 2) / d.scale  # test/runtests.jl:68
(d::LogNormal)(x) = any(x .<= 0) ? -Inf : sum(-log.(x) .- 0.5 .* ((log.(x) .- d.mu) ./ d.sigma) .^ 2)
(d::MvNormal2)(x) = -0.5 * ((x .- d.mean)' * d.prec * (x .- d.mean))

density_id(::GaussianIso) = Cint(0); params(d::GaussianIso) = [d.mu, d.sigma]
density_id(::Exponential) = Cint(1); params(d::Exponential) = [d.rate]
density_id(::Rosenbrock) = Cint(2);  params(d::Rosenbrock) = [d.a, d.b, d.scale]
density_id(::LogNormal) = Cint(3);   params(d::LogNormal) = [d.mu, d.sigma]
density_id(::MvNormal2) = Cint(4);   params(d::MvNormal2) = [d.mean[1], d.mean[2], d.prec[1,1], 0.5 * (d.prec[1,2] + d.prec[2,1]), d.prec[2,2]]

# Runtime-compiled user density (hiprtc): log p = sum_d term(x_d) + sum_{d<n-1} pair(x_d, x_{d+1}); see
# kmc_user_density_create in include/kissmcmc_hip.h.  The host call evaluates it on the device.
mutable struct ExprDensity <: DeviceLogPdf
    handle::Ptr{Cvoid}; p::Vector{Float64}; nblob::Int
    ExprDensity(handle::Ptr{Cvoid}, p::Vector{Float64}, nblob::Int=0) = new(handle, p, nblob)   # (an existing handle: CDensity below)
    function ExprDensity(term::String, pair::Union{String,Nothing}=nothing; params=Float64[])
        h = Ref{Ptr{Cvoid}}(C_NULL)
        st = ccall((:kmc_user_density_create, LIB), Cint, (Cstring, Cstring, Ref{Ptr{Cvoid}}), term, pair === nothing ? "" : pair, h)
        st == 0 || error("kmc_user_density_create failed: $(last_error())")
        d = new(h[], collect(Float64, params), 0)
        finalizer(x -> ccall((:kmc_user_density_destroy, LIB), Cvoid, (Ptr{Cvoid},), x.handle), d)
        return d
    end
end
# The general device form: the BODY of `double logpdf(const double* x, int n, const double* p) { BODY }` (C++), any coupling
# between the dimensions; runs one walker per lane (kmc_user_density_create_body).  `nblob=m`: the reference's
# `pdf(theta) -> (p, blob)` of hasblob=true (src/samplers.jl:150-151) on the device -- the body is then that of
# `double logpdf(const double* x, int n, const double* p, double* blob)` and fills blob[0..m) (kmc_user_density_create_body_blob).
# `grad=GRAD_BODY`: the body of `void grad(const double* x, int n, const double* p, double* g)` (g zero on entry), the gradient the HMC
# step of `metropolis_chains(...; hmc_nleap)` follows (kmc_user_density_set_grad; compiled here, not with blobs).
function CDensity(body::String; params=Float64[], nblob::Int=0, grad::Union{Nothing,String}=nothing)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    st = nblob > 0 ? ccall((:kmc_user_density_create_body_blob, LIB), Cint, (Cstring, Cint, Ref{Ptr{Cvoid}}), body, nblob, h) :
                     ccall((:kmc_user_density_create_body, LIB), Cint, (Cstring, Ref{Ptr{Cvoid}}), body, h)
    st == 0 || error("kmc_user_density_create_body failed: $(last_error())")
    if grad !== nothing && ccall((:kmc_user_density_set_grad, LIB), Cint, (Ptr{Cvoid}, Cstring), h[], grad) != 0
        msg = last_error()
        ccall((:kmc_user_density_destroy, LIB), Cvoid, (Ptr{Cvoid},), h[])
        error("kmc_user_density_set_grad failed: $msg")
    end
    d = ExprDensity(h[], collect(Float64, params), nblob)
    finalizer(x -> ccall((:kmc_user_density_destroy, LIB), Cvoid, (Ptr{Cvoid},), x.handle), d)
    return d
end
density_id(::ExprDensity) = Cint(100); params(d::ExprDensity) = d.p
user_handle(d::ExprDensity) = d.handle
user_handle(::DeviceLogPdf) = C_NULL
function (d::ExprDensity)(x)
    xs = collect(Float64, x isa Number ? [x] : x); out = Ref(0.0)
    p8 = ntuple(i -> i <= length(d.p) ? d.p[i] : 0.0, 8)
    cfg = Ref(KmcConfig(density=Cint(100), params=p8, nwalkers=2, ndim=length(xs), user_density=d.handle))
    st = ccall((:kmc_logpdf_eval_host, LIB), Cint, (Ref{KmcConfig}, Ptr{Float64}, Ref{Float64}, Int64), cfg, xs, out, 1)
    st == 0 || error(last_error()); out[]
end

# A log-prior plus a sum of per-observation terms over a dataset, on the device (kmc_data_density_create): `term` is the body of
# `double term(const double* x, int n, const double* d, const double* p)` (d = one observation row), `prior` that of
# `double prior(const double* x, int n, const double* p)` (nothing: 0).  `data` is ndata x ncols (a vector: one column), copied at
# creation; lp = -Inf where the prior is -Inf, else prior + the pairwise sum of the terms in observation order.
mutable struct DataDensity <: DeviceLogPdf
    handle::Ptr{Cvoid}; p::Vector{Float64}; ndata::Int
    function DataDensity(term::String, data::AbstractVecOrMat; prior::Union{String,Nothing}=nothing, params=Float64[])
        D = data isa AbstractVector ? reshape(collect(Float64, data), :, 1) : collect(Float64, data)
        rows = permutedims(D)                          # row-major [ndata][ncols] for the C ABI
        h = Ref{Ptr{Cvoid}}(C_NULL)
        st = ccall((:kmc_data_density_create, LIB), Cint, (Cstring, Cstring, Ptr{Float64}, Int64, Int32, Ref{Ptr{Cvoid}}),
                   term, prior === nothing ? "" : prior, rows, size(D, 1), Int32(size(D, 2)), h)
        st == 0 || error("kmc_data_density_create failed: $(last_error())")
        d = new(h[], collect(Float64, params), size(D, 1))
        finalizer(x -> ccall((:kmc_user_density_destroy, LIB), Cvoid, (Ptr{Cvoid},), x.handle), d)
        return d
    end
end
density_id(::DataDensity) = Cint(102); params(d::DataDensity) = d.p
user_handle(d::DataDensity) = d.handle
function (d::DataDensity)(x)
    xs = collect(Float64, x isa Number ? [x] : x); out = Ref(0.0)
    p8 = ntuple(i -> i <= length(d.p) ? d.p[i] : 0.0, 8)
    cfg = Ref(KmcConfig(density=Cint(102), params=p8, nwalkers=2, ndim=length(xs), user_density=d.handle))
    st = ccall((:kmc_logpdf_eval_host, LIB), Cint, (Ref{KmcConfig}, Ptr{Float64}, Ref{Float64}, Int64), cfg, xs, out, 1)
    st == 0 || error(last_error()); out[]
end

# Any Julia callable as the log-density (the reference's closure, src/samplers.jl:257), evaluated on
# the host: kmc_config.host_logpdf points at `host_trampoline`, host_user at the wrapper object.
# With hasblob the closure returns (p, blob) (src/samplers.jl:150-151): the blobs stay on the host --
# `batch` holds those of the rows evaluated last, `blob0s` the walkers' current ones (:264), `blobs` the
# per-walker storage (:238, :270) -- and follow the device's accept decisions, reported per half-step
# through kmc_config.host_accepted (`accepted_trampoline`).
mutable struct HostLogPdf{F} <: DeviceLogPdf
    f::F; scalar::Bool; hasblob::Bool
    batch::Vector{Any}; blob0s::Vector{Any}; blobs::Vector{Any}
    init_blobs::Any; reduce_blob!::Any; nsamples::Int
end
HostLogPdf(f; hasblob=false) = HostLogPdf(f, false, hasblob, Any[], Any[], Any[], nothing, nothing, 0)
(d::HostLogPdf)(x) = d.f(x)
density_id(::HostLogPdf) = Cint(101); params(::HostLogPdf) = Float64[]
function host_trampoline(rows::Ptr{Float64}, nrows::Int64, ndim::Int64, out::Ptr{Float64}, user::Ptr{Cvoid})::Cint
    try
        d = unsafe_pointer_to_objref(user)
        X = unsafe_wrap(Array, rows, (ndim, nrows))       # column w = proposal of walker w
        d.hasblob && resize!(d.batch, nrows)
        for w in 1:nrows
            r = d.scalar ? d.f(X[1, w]) : d.f(X[:, w])
            if d.hasblob
                unsafe_store!(out, Float64(r[1]), w); d.batch[w] = r[2]                 # p1, blob1 = pdf(theta1)  :257
            else
                unsafe_store!(out, Float64(r), w)
            end
        end
        return Cint(0)
    catch
        return Cint(1)                                     # kmc_emcee_run then fails with KMC_ERR_BAD_ARG
    end
end
function accepted_trampoline(accepted::Ptr{UInt8}, nrows::Int64, row0::Int64, generation::Int64, stored::Int32, user::Ptr{Cvoid})::Cint
    try
        d = unsafe_pointer_to_objref(user)
        if isempty(d.blob0s)        # first half-step: the last full evaluation was the initial one (:209-210)
            error("initial blobs missing")
        end
        for i in 1:nrows
            unsafe_load(accepted, i) != 0 && (d.blob0s[row0 + i] = d.batch[i])          # :264
        end
        if stored != 0
            for w in (row0 + 1):(row0 + nrows)
                d.reduce_blob!(d.blobs[w], d.blob0s[w])                                  # :270
            end
        end
        return Cint(0)
    catch
        return Cint(1)
    end
end

"""
    emcee(pdf::DeviceLogPdf, theta0s; niter=10^5, nburnin=niter÷2, nthin=1, a_scale=2.0,
          use_progress_meter=true, hasblob=false, init_blobs, reduce_blob!, seed=rand(UInt64), device=0, dtype=:f64,
          move=:stretch, de_gamma0=0.0, de_sigma=1e-5, snooker_gamma=1.7, betas=Float64[], swap_every=1, temper=:whole,
          adapt=false, adapt_lag=10000.0, adapt_time=100.0, adapt_until=0)

Same meaning as KissMCMC.emcee (src/samplers.jl:188-197); returns
`(thetas, accept_ratio, logdensities, blobs)` with `thetas[w][k]` (src/samplers.jl:292).
`hasblob=true` needs a `pdf` that returns a blob: a host closure (`HostLogPdf(f; hasblob=true)`, blobs of any type, kept on
the host) or a `CDensity(body; nblob=m)` (m doubles computed and carried on the device; `blobs[w][k]::Vector{Float64}`).
`move=:de` selects the opt-in differential-evolution move (KMC_MOVE_DE; `de_gamma0=0` is 2.38/sqrt(2 ndim), `de_sigma` the
relative jitter of gamma); `:stretch` is the reference's move with `a_scale`.  `move=:snooker` is the DE snooker update
(KMC_MOVE_SNOOKER, `snooker_gamma`); `move=[(:de, 0.8), (:snooker, 0.2)]` a mixture of 2 to 4 weighted members (KMC_MOVE_MIX:
one member per half-step, each with `de_gamma0` / `de_sigma` or `snooker_gamma`).
`betas=[1.0, ...]` (strictly decreasing inverse temperatures) switches parallel tempering on: a ladder of ensembles, rung t sampling
`exp(betas[t] * logpdf)`, neighbouring rungs exchanging walkers every `swap_every` generations; `theta0s` starts every rung and
the returned tuple is rung 1's (`betas[1] == 1`, the target itself).  `temper=:likelihood` (KMC_TEMPER_LIKELIHOOD) tempers only the
likelihood of a data density -- rung t samples `prior + betas[t] * S`, and the last beta may be 0 --; the library refuses it for
every other density.  `adapt=true` (KMC's adaptive ladder; `length(betas) >= 3`, `swap_every >= 1`) lets the swap sweeps of burn-in move
the interior rungs towards equal swap acceptance between all neighbouring pairs (ptemcee's dynamics with `adapt_lag`, `adapt_time`)
until generation `adapt_until` (0: `nburnin ÷ nwalkers`, the end of burn-in); every stored sample comes from the frozen ladder.
"""
function emcee(pdf::DeviceLogPdf, theta0s; niter=10^5, nburnin=niter ÷ 2, nthin=1, a_scale=2.0,
               use_progress_meter=true, hasblob=false,
               init_blobs=(blob0, nsamples) -> sizehint!(typeof(blob0)[], nsamples),      # init_output_vector :80-85
               reduce_blob! =(blobs, blob) -> push!(blobs, blob),                         # :196
               seed=rand(UInt64), device=0, dtype=:f64,     # dtype=:f32: float rows on the device (KMC_F32), built-in densities
               move=:stretch, de_gamma0=0.0, de_sigma=1e-5, snooker_gamma=1.7, betas=Float64[], swap_every=1, temper=:whole,
               adapt=false, adapt_lag=10000.0, adapt_time=100.0, adapt_until=0)
    ladder = collect(Float64, betas)                      # (kept alive across the call: GC.@preserve below)
    temper in (:whole, :likelihood) || error("temper must be :whole or :likelihood")
    temper == :whole || !isempty(ladder) || error("temper=:likelihood needs a ladder (betas)")
    !adapt || length(ladder) >= 3 || error("adapt=true needs a ladder of at least 3 rungs (betas)")
    isempty(ladder) || (length(ladder) >= 2 && ladder[1] == 1.0 && all(diff(ladder) .< 0) && all(isfinite, ladder) &&
                        (ladder[end] > 0 || (temper == :likelihood && ladder[end] == 0))) ||
        error("betas must start at 1 and decrease strictly, finite and > 0 (temper=:likelihood: the last one may be 0)")
    mix = move isa AbstractVector ? collect(move) : Tuple{Symbol,Float64}[]
    if move isa AbstractVector
        2 <= length(mix) <= 4 || error("a move mixture has 2 to 4 (move, weight) pairs")
        all(m -> m[1] in (:de, :snooker), mix) || error("mixture members are :de and :snooker (a :stretch member is not supported yet)")
        all(m -> isfinite(m[2]) && m[2] > 0, mix) || error("mixture weights must be finite and > 0")
    else
        move in (:stretch, :de, :snooker) || error("move must be :stretch, :de, :snooker or a vector of (move, weight) pairs")
    end
    mix_id(i) = i <= length(mix) ? (mix[i][1] == :de ? KMC_MOVE_DE : KMC_MOVE_SNOOKER) : Int32(0)
    mix_w(i) = i <= length(mix) ? Float64(mix[i][2]) : 0.0
    mix_g(i) = i <= length(mix) ? (mix[i][1] == :de ? Float64(de_gamma0) : Float64(snooker_gamma)) : 0.0
    mix_s(i) = i <= length(mix) && mix[i][1] == :de ? Float64(de_sigma) : 0.0
    device_blobs = hasblob && pdf isa ExprDensity && pdf.nblob > 0
    hasblob && !device_blobs && !(pdf isa HostLogPdf && pdf.hasblob) &&
        error("hasblob=true needs a pdf that returns a blob: HostLogPdf(f; hasblob=true) or CDensity(body; nblob=m)")
    nwalkers = length(theta0s)
    scalar = theta0s[1] isa Number
    ndim = length(theta0s[1])
    @assert a_scale > 1                                                                  # :200
    @assert iseven(nwalkers) "Use an even number of walkers."                           # :202
    niter_walker = niter ÷ nwalkers                                                      # :203
    nburnin_walker = nburnin ÷ nwalkers                                                  # :204
    @assert nwalkers >= ndim + 2 "Use more walkers: at least DOF+2, but better many more."  # :205
    nsamples = max(0, (niter_walker - nburnin_walker) ÷ nthin)                           # :234

    theta = Matrix{Float64}(undef, ndim, nwalkers)        # column-major [dim, walker] == C row-major [walker][dim]
    for w in 1:nwalkers, d in 1:ndim
        theta[d, w] = scalar ? theta0s[w] : theta0s[w][d]                                # :198 deep copy
    end
    p = params(pdf); p8 = ntuple(i -> i <= length(p) ? p[i] : 0.0, 8)
    host_fn, host_ctx, acc_fn = C_NULL, C_NULL, C_NULL
    if pdf isa HostLogPdf
        pdf.scalar = scalar
        host_fn = @cfunction(host_trampoline, Cint, (Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Cvoid}))
        host_ctx = pointer_from_objref(pdf)
        if pdf.hasblob
            # the initial evaluations (:209-210) here, so that blob storage exists before the run; the library
            # evaluates the same rows once more for its own log-pdfs
            tmp = [pdf.f(scalar ? theta0s[w] : collect(Float64, theta0s[w])) for w in 1:nwalkers]
            pdf.blob0s = Any[t[2] for t in tmp]
            pdf.blobs = Any[init_blobs(pdf.blob0s[w], nsamples) for w in 1:nwalkers]      # :238
            pdf.init_blobs, pdf.reduce_blob!, pdf.nsamples = init_blobs, reduce_blob!, nsamples
            acc_fn = @cfunction(accepted_trampoline, Cint, (Ptr{UInt8}, Int64, Int64, Int64, Int32, Ptr{Cvoid}))
        end
    end
    chain = Array{Float64}(undef, ndim * nsamples * nwalkers)
    clogp = Array{Float64}(undef, nsamples * nwalkers)
    acc = Vector{Float64}(undef, nwalkers)
    nblob = device_blobs ? pdf.nblob : 0
    bl = Array{Float64}(undef, nblob * nsamples * nwalkers)          # device blobs: [walker][sample][nblob] (src/samplers.jl:270)
    out = KmcOutputs(chain=pointer(chain), chain_logp=pointer(clogp), accept_ratio=pointer(acc), blobs=(device_blobs ? pointer(bl) : C_NULL))
    # The chain in the reference's own order (thetas[w][k], :219-221), reordered on the device.  A chain too large for
    # the device is streamed into these arrays while sampling (kmc_emcee_run decides, KMC_STREAM_CHAIN) and then arrives
    # sample-major: that combination is refused (status 9) and the call is repeated without the flag.
    st = 9; by_walker = true
    for flag in (KMC_CHAIN_BY_WALKER, UInt32(0))
        by_walker = flag != 0
        cfg = Ref(KmcConfig(dtype=(dtype == :f32 ? 1 : 0), density=density_id(pdf), params=p8, nwalkers=nwalkers, ndim=ndim,
                            ngenerations=niter_walker, nburnin=nburnin_walker, nthin=nthin, a_scale=a_scale, seed=UInt64(seed),
                            flags=KMC_STORE_CHAIN | KMC_STORE_LOGP | flag, device=Int32(device), user_density=user_handle(pdf),
                            host_logpdf=host_fn, host_user=host_ctx, host_accepted=acc_fn,
                            move=(move isa AbstractVector ? KMC_MOVE_MIX : move == :de ? KMC_MOVE_DE : move == :snooker ? KMC_MOVE_SNOOKER : KMC_MOVE_STRETCH),
                            de_gamma0=Float64(de_gamma0), de_sigma=Float64(de_sigma), snooker_gamma=Float64(snooker_gamma), mix_count=Int32(length(mix)),
                            mix_move0=mix_id(1), mix_move1=mix_id(2), mix_move2=mix_id(3), mix_move3=mix_id(4),
                            mix_weight0=mix_w(1), mix_weight1=mix_w(2), mix_weight2=mix_w(3), mix_weight3=mix_w(4),
                            mix_gamma0=mix_g(1), mix_gamma1=mix_g(2), mix_gamma2=mix_g(3), mix_gamma3=mix_g(4),
                            mix_sigma0=mix_s(1), mix_sigma1=mix_s(2), mix_sigma2=mix_s(3), mix_sigma3=mix_s(4),
                            betas=(isempty(ladder) ? Ptr{Float64}(C_NULL) : pointer(ladder)), ntemps=Int32(length(ladder)),
                            swap_every=Int32(isempty(ladder) ? 0 : swap_every), temper_mode=(temper == :likelihood ? KMC_TEMPER_LIKELIHOOD : KMC_TEMPER_WHOLE),
                            adapt=Int32(adapt ? 1 : 0), adapt_until=Int64(adapt ? adapt_until : 0), adapt_lag=Float64(adapt ? adapt_lag : 0.0),
                            adapt_time=Float64(adapt ? adapt_time : 0.0)))
        st = GC.@preserve pdf theta chain clogp acc bl ladder ccall((:kmc_emcee_run, LIB), Cint,
                                                       (Ref{KmcConfig}, Ptr{Float64}, Ref{KmcOutputs}), cfg, theta, out)
        (st == 9 && by_walker && occursin("KMC_CHAIN_BY_WALKER", last_error())) || break
    end
    st == 0 || error("kmc_emcee_run failed ($st): $(last_error())")
    # column-major views of the C arrays: [dim, sample, walker] (by walker) or [dim, walker, sample]
    ch = by_walker ? reshape(chain, ndim, nsamples, nwalkers) : permutedims(reshape(chain, ndim, nwalkers, nsamples), (1, 3, 2))
    lp = by_walker ? reshape(clogp, nsamples, nwalkers) : permutedims(reshape(clogp, nwalkers, nsamples), (2, 1))
    thetas = scalar ? [ch[1, :, w] for w in 1:nwalkers] :
                      [[ch[:, k, w] for k in 1:nsamples] for w in 1:nwalkers]
    logdensities = [lp[:, w] for w in 1:nwalkers]
    if device_blobs
        # blob0s = the blobs of the initial evaluations (:209-210); then the caller's init_blobs / reduce_blob! over each
        # walker's stored series, in order (:238, :270)
        lp0 = Vector{Float64}(undef, nwalkers); b0 = Matrix{Float64}(undef, nblob, nwalkers)
        cfg0 = Ref(KmcConfig(density=density_id(pdf), params=p8, nwalkers=nwalkers, ndim=ndim, user_density=user_handle(pdf), device=Int32(device)))
        st0 = ccall((:kmc_logpdf_blob_eval_host, LIB), Cint, (Ref{KmcConfig}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64), cfg0, theta, lp0, b0, nwalkers)
        st0 == 0 || error("kmc_logpdf_blob_eval_host failed ($st0): $(last_error())")
        B = by_walker ? reshape(bl, nblob, nsamples, nwalkers) : permutedims(reshape(bl, nblob, nwalkers, nsamples), (1, 3, 2))
        blobs = [init_blobs(b0[:, w], nsamples) for w in 1:nwalkers]
        for w in 1:nwalkers, k in 1:nsamples
            reduce_blob!(blobs[w], B[:, k, w])
        end
        return thetas, acc, logdensities, blobs
    end
    return thetas, acc, logdensities, (pdf isa HostLogPdf && pdf.hasblob) ? pdf.blobs : nothing   # :292
end
# (a bare closure as `pdf` is KissMCMC.emcee's own CPU method; `emcee(HostLogPdf(f; hasblob), theta0s; ...)` runs the
#  sampler on the GPU with `f` evaluated on the host)

# ---- many-chain Metropolis: metropolis / _metropolis, src/samplers.jl:59-128 ---------------------
"Symmetric proposal `theta -> scale .* randn(n) .+ theta` (the one all reference tests use, test/runtests.jl:54,59,64,75)."
struct GaussianStep; scale::Vector{Float64}; end
GaussianStep(c::Real) = GaussianStep([Float64(c)])

Base.@kwdef struct KmcMetropolisConfig
    dtype::Int32 = 0
    density::Int32 = 0
    params::NTuple{8,Float64} = ntuple(_ -> 0.0, 8)
    nchains::Int64 = 0
    ndim::Int64 = 0
    niter::Int64 = 0
    nburnin::Int64 = 0
    nthin::Int64 = 1
    step::Ptr{Float64} = C_NULL
    seed::UInt64 = 0
    flags::UInt32 = 0
    device::Int32 = 0
    user_density::Ptr{Cvoid} = C_NULL
    host_logpdf::Ptr{Cvoid} = C_NULL                  # host route: `pdf` is a closure (density == KMC_HOST_DENSITY) ...
    host_user::Ptr{Cvoid} = C_NULL
    host_accepted::Ptr{Cvoid} = C_NULL                # ... accept outcomes per iteration (blobs)
    host_propose::Ptr{Cvoid} = C_NULL                 # ... `sample_ppdf` is a closure (then `step` may be NULL)
    chol::Ptr{Float64} = C_NULL                       # the proposal theta + L z: [ndim][ndim] row-major, lower triangle read (instead of `step`)
    tune_rounds::Int32 = 0                            # tuning boundaries during burn-in: L from the covariance across chains
    tune_scale::Float64 = 0.0                         # 0: 2.38 / sqrt(ndim)
    hmc_nleap::Int32 = 0                              # 0: off; 1 .. 1024: the HMC step, leapfrog steps per iteration (`step`: the step sizes)
    hmc_jitter::Float64 = 0.0                         # in [0, 1): relative half-width of the per-iteration step-size jitter
end

Base.@kwdef mutable struct KmcMetropolisOutputs
    chain::Ptr{Float64} = C_NULL
    chain_logp::Ptr{Float64} = C_NULL
    accept_ratio::Ptr{Float64} = C_NULL
    naccept::Ptr{Int64} = C_NULL
    final_pos::Ptr{Float64} = C_NULL
    final_logp::Ptr{Float64} = C_NULL
    chain_sum::Ptr{Float64} = C_NULL
    chain_sumsq::Ptr{Float64} = C_NULL
    nsamples::Int64 = 0
    device_ms::Float64 = 0.0
    blobs::Ptr{Float64} = C_NULL
    final_blob::Ptr{Float64} = C_NULL
    chol_out::Ptr{Float64} = C_NULL
    tune_skipped::Int64 = 0
    tune_ms::Float64 = 0.0
end

# Layout drift between these mirrors and the library fails here, when the module loads -- not inside the first real ccall.
function __init__()
    for (n, T) in ((ccall((:kmc_sizeof_config, LIB), Cint, ()), KmcConfig), (ccall((:kmc_sizeof_metropolis_config, LIB), Cint, ()), KmcMetropolisConfig),
                   (ccall((:kmc_sizeof_outputs, LIB), Cint, ()), KmcOutputs), (ccall((:kmc_sizeof_metropolis_outputs, LIB), Cint, ()), KmcMetropolisOutputs))
        n == sizeof(T) || error("$LIB: $(T) is $(sizeof(T)) bytes here but $n in the library (include/kissmcmc_hip.h changed: update the struct in KissMCMCHIP.jl)")
    end
end

# `sample_ppdf` as ANY Julia callable (src/samplers.jl:41, :98), kept on the host: called once per iteration on every
# chain's current state.  The host callbacks of one run share one context object, `MetroCtx`.
mutable struct HostProposal{F}; f::F; scalar::Bool; end
HostProposal(f) = HostProposal(f, false)
mutable struct MetroCtx; pdf::Any; prop::Any; end
function metro_pdf_trampoline(rows::Ptr{Float64}, nrows::Int64, ndim::Int64, out::Ptr{Float64}, user::Ptr{Cvoid})::Cint
    ctx = unsafe_pointer_to_objref(user)::MetroCtx
    return host_trampoline(rows, nrows, ndim, out, pointer_from_objref(ctx.pdf))
end
function metro_propose_trampoline(rows::Ptr{Float64}, nrows::Int64, ndim::Int64, out::Ptr{Float64}, user::Ptr{Cvoid})::Cint
    try
        d = (unsafe_pointer_to_objref(user)::MetroCtx).prop
        X = unsafe_wrap(Array, rows, (ndim, nrows)); Y = unsafe_wrap(Array, out, (ndim, nrows))
        for c in 1:nrows
            Y[:, c] .= d.scalar ? d.f(X[1, c]) : d.f(X[:, c])                            # theta1 = sample_ppdf(theta0)  :98
        end
        return Cint(0)
    catch
        return Cint(1)
    end
end

"""
    metropolis_chains(pdf::DeviceLogPdf, sample_ppdf::Union{GaussianStep,HostProposal}, theta0s; niter=10^5, nburnin=niter÷2, nthin=1, seed, device)

One independent Metropolis chain (src/samplers.jl:96-126) per element of `theta0s`; `niter`/`nburnin` count steps per
chain.  With a menu / `ExprDensity` `pdf` and a `GaussianStep` the chains run inside one kernel, one chain per GPU lane;
a `HostLogPdf(f)` and / or a `HostProposal(g)` keep those closures on the host (one batch call per iteration) while the
accept test, counters and storage stay on the device.  Returns `(thetas, accept_ratio, logdensities, nothing)` shaped
like `emcee`'s output (`thetas[chain][sample]`), so `squash_walkers` applies.

`chol=L` (an `ndim x ndim` matrix, lower triangle read) replaces the `GaussianStep`'s scales by the covariance-shaped proposal
`theta + L z` (include/kissmcmc_hip.h: same draws, `L z` summed in index order without fused multiply-add); `tune_rounds=R > 0`
replaces `L` at `R` boundaries of burn-in by the Cholesky factor of `tune_scale^2` (default `2.38 / sqrt(ndim)`) times the covariance of
the chains' current states across chains, the `GaussianStep` or `chol` being the initial proposal.

`hmc_nleap=n > 0` makes the step a Hamiltonian Monte Carlo proposal (include/kissmcmc_hip.h holds the rule): the `GaussianStep`'s scales are
the step sizes `step_i` (all > 0), the momentum `m` is the normals `z` the random walk would have drawn, `f = 1 + hmc_jitter * (((j + 1/2) 2^-11) - 1)`
with `j` the low 12 bits of word 3 of Philox block 0, `e_i = step_i f`, `h_i = e_i / 2`; from `y = x`, `g = grad(y)`, `n` times
`m += h .* g; y += e .* m; g = grad(y); m += h .* g`; accepted iff `(p1 - K1) - (p0 - K0) > log u` (strict) with `K = 1/2 sum m_i^2`, every product
and sum rounded on its own.  `pdf` is a menu density, or a `CDensity` given a gradient body with `kmc_user_density_set_grad`; `ndim <= 32`; not
with `chol`, `tune_rounds`, a `HostProposal`, a `HostLogPdf` or blobs.
"""
function metropolis_chains(pdf::DeviceLogPdf, sample_ppdf::Union{GaussianStep,HostProposal}, theta0s; niter=10^5, nburnin=niter ÷ 2, nthin=1,
                           chol::Union{Nothing,AbstractMatrix}=nothing, tune_rounds::Integer=0, tune_scale::Real=0.0,
                           hmc_nleap::Integer=0, hmc_jitter::Real=0.0,
                           hasblob=false, init_blobs=(blob0, nsamples) -> sizehint!(typeof(blob0)[], nsamples),
                           reduce_blob! =(blobs, blob) -> push!(blobs, blob), seed=rand(UInt64), device=0)
    device_blobs = hasblob && pdf isa ExprDensity && pdf.nblob > 0 && sample_ppdf isa GaussianStep
    hasblob && !device_blobs &&
        error("hasblob=true for metropolis: a CDensity(body; nblob=m) with a GaussianStep (blobs carried on the device); host closures with blobs are not wired in this shim (the C ABI carries them: kmc_metropolis_config.host_accepted)")
    nchains = length(theta0s); scalar = theta0s[1] isa Number; ndim = length(theta0s[1])
    nsamples = niter > nburnin ? (niter - nburnin) ÷ nthin : 0                            # :88
    theta = Matrix{Float64}(undef, ndim, nchains)          # column-major [dim, chain] == C row-major [chain][dim]
    for c in 1:nchains, d in 1:ndim
        theta[d, c] = scalar ? theta0s[c] : theta0s[c][d]                                # :68 deep copy
    end
    step = Float64[]
    prop_fn = C_NULL
    if sample_ppdf isa GaussianStep
        step = length(sample_ppdf.scale) == 1 ? fill(sample_ppdf.scale[1], ndim) : copy(sample_ppdf.scale)
        @assert length(step) == ndim
        chol === nothing || (step = Float64[])                                            # exactly one of step / chol
    else
        sample_ppdf.scalar = scalar
        prop_fn = @cfunction(metro_propose_trampoline, Cint, (Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Cvoid}))
    end
    pdf_fn = C_NULL
    if pdf isa HostLogPdf
        pdf.scalar = scalar
        pdf_fn = @cfunction(metro_pdf_trampoline, Cint, (Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Cvoid}))
    end
    cholrm = chol === nothing ? Float64[] : vec(permutedims(Matrix{Float64}(chol)))      # row-major [ndim][ndim], as the C ABI reads it
    chol === nothing || size(chol) == (ndim, ndim) || error("chol must be $ndim x $ndim")
    ctx = MetroCtx(pdf, sample_ppdf)
    p = params(pdf); p8 = ntuple(i -> i <= length(p) ? p[i] : 0.0, 8)
    chain = Array{Float64}(undef, ndim, nsamples, nchains)      # column-major == C [chain][sample][dim] (KMC_CHAIN_BY_WALKER)
    clogp = Array{Float64}(undef, nsamples, nchains)
    acc = Vector{Float64}(undef, nchains)
    nblob = device_blobs ? pdf.nblob : 0
    bl = Array{Float64}(undef, nblob, nsamples, nchains)         # blobs[chain][sample] (:117), nblob doubles each
    out = KmcMetropolisOutputs(chain=pointer(chain), chain_logp=pointer(clogp), accept_ratio=pointer(acc), blobs=(device_blobs ? pointer(bl) : C_NULL))
    st = GC.@preserve pdf sample_ppdf ctx theta step cholrm chain clogp acc bl begin
        cfg = Ref(KmcMetropolisConfig(density=density_id(pdf), params=p8, nchains=nchains, ndim=ndim, niter=niter, nburnin=nburnin,
                                      nthin=nthin, step=(isempty(step) ? Ptr{Float64}(C_NULL) : pointer(step)), seed=UInt64(seed),
                                      flags=KMC_STORE_CHAIN | KMC_STORE_LOGP | KMC_CHAIN_BY_WALKER | (device_blobs ? KMC_STORE_BLOBS : UInt32(0)), device=Int32(device), user_density=user_handle(pdf),
                                      host_logpdf=pdf_fn, host_user=pointer_from_objref(ctx), host_propose=prop_fn,
                                      chol=(isempty(cholrm) ? Ptr{Float64}(C_NULL) : pointer(cholrm)), tune_rounds=Int32(tune_rounds), tune_scale=Float64(tune_scale),
                                      hmc_nleap=Int32(hmc_nleap), hmc_jitter=Float64(hmc_jitter)))
        ccall((:kmc_metropolis_run, LIB), Cint, (Ref{KmcMetropolisConfig}, Ptr{Float64}, Ref{KmcMetropolisOutputs}), cfg, theta, out)
    end
    st == 0 || error("kmc_metropolis_run failed ($st): $(last_error())")
    thetas = scalar ? [chain[1, :, c] for c in 1:nchains] :
                      [[chain[:, k, c] for k in 1:nsamples] for c in 1:nchains]
    blobs = nothing
    if device_blobs       # p0, blob0 = pdf(theta0) (:70) for init_blobs (:90), then reduce_blob! over each chain's stored series (:117)
        lp0 = Vector{Float64}(undef, nchains); b0 = Matrix{Float64}(undef, nblob, nchains)
        cfg0 = Ref(KmcConfig(density=density_id(pdf), params=p8, nwalkers=nchains + isodd(nchains), ndim=ndim, user_density=user_handle(pdf), device=Int32(device)))
        st0 = ccall((:kmc_logpdf_blob_eval_host, LIB), Cint, (Ref{KmcConfig}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64), cfg0, theta, lp0, b0, nchains)
        st0 == 0 || error("kmc_logpdf_blob_eval_host failed ($st0): $(last_error())")
        blobs = [init_blobs(b0[:, c], nsamples) for c in 1:nchains]
        for c in 1:nchains, k in 1:nsamples
            reduce_blob!(blobs[c], bl[:, k, c])
        end
    end
    return thetas, acc, [clogp[:, c] for c in 1:nchains], blobs
end

"""
    metropolis(pdf::DeviceLogPdf, sample_ppdf::Union{GaussianStep,HostProposal}, theta0; niter=10^5, nburnin=niter÷2, nthin=1, ...)

One more method of KissMCMC.metropolis, with its signature and return value (src/samplers.jl:59-77, :128), for one chain
on the GPU (a single lane: a drop-in, not a fast path -- use `metropolis_chains` for throughput).  Two plain closures,
`metropolis(pdf, sample_ppdf, theta0)`, remain KissMCMC's own CPU method.
"""
function metropolis(pdf::DeviceLogPdf, sample_ppdf::Union{GaussianStep,HostProposal}, theta0; use_progress_meter=true, kw...)
    thetas, acc, logd, blobs = metropolis_chains(pdf, sample_ppdf, [theta0]; kw...)
    return thetas[1], acc[1], logd[1], blobs === nothing ? nothing : blobs[1]             # :128
end

"""
    int_acorr(thetas; c=5, device=0)

Integrated autocorrelation time per dimension (src/analysis.jl:140-167, commented out in the reference; followed as
written) of `thetas[walker][sample]` as `emcee` / `metropolis_chains` return it.  Returns `(tau, converged)`.
"""
function int_acorr(thetas; c=5, device=0)
    @assert c > 1
    nw = length(thetas); ns = length(thetas[1]); nd = length(thetas[1][1])
    chain = Array{Float64}(undef, nd, nw, ns)              # column-major == C [sample][walker][dim]
    for w in 1:nw, k in 1:ns, d in 1:nd
        chain[d, w, k] = nd == 1 ? thetas[w][k][1] : thetas[w][k][d]
    end
    tau = Vector{Float64}(undef, nd); conv = Vector{Float64}(undef, nd)
    st = ccall((:kmc_int_acorr, LIB), Cint, (Ptr{Float64}, Int64, Int64, Int64, Float64, Cint, Ptr{Float64}, Ptr{Float64}),
               chain, ns, nw, nd, Float64(c), Cint(device), tau, conv)
    st == 0 || error("kmc_int_acorr failed ($st): $(last_error())")
    return tau, conv
end

# thetas[walker][sample](dim) -> column-major (dim, walker, sample) == C [sample][walker][dim]; logdensities[walker][sample] likewise
function _summary_chain(thetas, logdensities)
    nw = length(thetas); ns = length(thetas[1]); nd = length(thetas[1][1])
    chain = Array{Float64}(undef, nd, nw, ns)
    for w in 1:nw, k in 1:ns, d in 1:nd
        chain[d, w, k] = nd == 1 ? thetas[w][k][1] : thetas[w][k][d]
    end
    logp = logdensities === nothing ? nothing : Float64[logdensities[w][k] for w in 1:nw, k in 1:ns]
    return chain, logp, ns, nw, nd
end
_summary_mask(walkers, nw) = walkers === nothing ? nothing : (m = zeros(UInt8, nw); m[walkers] .= 1; m)

"""
    quantiles(thetas, q; logdensities=nothing, first_sample=0, walkers=nothing, device=0)

Quantiles `q` (in [0, 1]) per dimension of `thetas[walker][sample]` as `emcee` / `metropolis_chains` return it, over the samples
after the first `first_sample` of the walkers `walkers` (indices or a Bool mask; all by default): a `length(q) x ndim` matrix, and
with `logdensities` also the vector of their quantiles.  The two order statistics of every quantile are selected exactly on the GPU
(`kmc_chain_order_stats`); the value is `x_lo + frac (x_hi - x_lo)` with `h = q (n - 1)`, `lo = floor(h)`, `frac = h - lo`.
"""
function quantiles(thetas, q; logdensities=nothing, first_sample=0, walkers=nothing, device=0)
    chain, logp, ns, nw, nd = _summary_chain(thetas, logdensities)
    mask = _summary_mask(walkers, nw)
    n = (ns - first_sample) * (mask === nothing ? nw : count(!iszero, mask))
    n >= 1 || error("the selection is empty")
    out = Matrix{Float64}(undef, length(q), nd); outlp = Vector{Float64}(undef, length(q))
    for (i, qi) in enumerate(q)
        @assert 0 <= qi <= 1
        h = qi * (n - 1); lo = floor(Int64, h); hi = min(lo + 1, n - 1); frac = h - lo
        ranks = Int64[lo, hi]
        th = Matrix{Float64}(undef, nd, 2); lp = Vector{Float64}(undef, 2); nout = Ref{Int64}(0)
        st = ccall((:kmc_chain_order_stats, LIB), Cint,
                   (Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Int64, Ptr{UInt8}, Ptr{Int64}, Int32, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
                   chain, logp === nothing ? C_NULL : logp, ns, nw, nd, first_sample, mask === nothing ? C_NULL : mask, ranks, Int32(2), Cint(device),
                   th, logp === nothing ? C_NULL : lp, nout)
        st == 0 || error("kmc_chain_order_stats failed ($st): $(last_error())")
        for d in 1:nd
            out[i, d] = frac == 0 ? th[d, 1] : th[d, 1] + frac * (th[d, 2] - th[d, 1])
        end
        logp === nothing || (outlp[i] = frac == 0 ? lp[1] : lp[1] + frac * (lp[2] - lp[1]))
    end
    return logdensities === nothing ? out : (out, outlp)
end

"""
    map_sample(thetas, logdensities; first_sample=0, walkers=nothing, device=0)

The stored sample of the largest log-density (`kmc_chain_argmax`): `(theta, logdensity, sample, walker)`, 1-based; ties go to the
smallest sample, then the smallest walker.
"""
function map_sample(thetas, logdensities; first_sample=0, walkers=nothing, device=0)
    chain, logp, ns, nw, nd = _summary_chain(thetas, logdensities)
    mask = _summary_mask(walkers, nw)
    k = Ref{Int64}(0); w = Ref{Int64}(0); lp = Ref{Float64}(0.0); theta = Vector{Float64}(undef, nd)
    st = ccall((:kmc_chain_argmax, LIB), Cint,
               (Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Int64, Ptr{UInt8}, Cint, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}),
               chain, logp, ns, nw, nd, first_sample, mask === nothing ? C_NULL : mask, Cint(device), k, w, theta, lp)
    st == 0 || error("kmc_chain_argmax failed ($st): $(last_error())")
    return theta, lp[], k[] + 1, w[] + 1
end

"""
    histograms(thetas, edges; dims=nothing, logdensities=nothing, pairs=false, first_sample=0, walkers=nothing, device=0)

Marginal histograms of `thetas[walker][sample]` as `emcee` / `metropolis_chains` return it, counted on the GPU
(`kmc_chain_histograms`).  `dims`: the dimensions (1-based; all by default), in the order wanted; `edges`: a `(nbins + 1) x ncols` matrix
of strictly increasing bin edges, one column per selected dimension and, with `logdensities`, one more for them.  An element `x` is
in bin `i` iff `e[i] <= x < e[i+1]`, the last bin closed.  Returns `(counts1, outside, counts2, n)`: `counts1` is `nbins x ncols`,
`outside` is `3 x ncols` (below the first edge, above the last, NaN), `counts2` -- with `pairs=true`, else `nothing` -- is
`nbins x nbins x npairs` over the pairs `(a, b)`, `a < b`, of positions in `dims`, `counts2[ib, ia, p]` counting bin `ia` of the pair's
first dimension and `ib` of its second (2 to 16 dimensions, `nbins <= 64`), and `n` the number of selected samples.
"""
function histograms(thetas, edges; dims=nothing, logdensities=nothing, pairs=false, first_sample=0, walkers=nothing, device=0)
    chain, logp, ns, nw, nd = _summary_chain(thetas, logdensities)
    mask = _summary_mask(walkers, nw)
    sel = dims === nothing ? collect(Int32, 0:nd-1) : Int32[d - 1 for d in dims]
    ncols = length(sel) + (logp === nothing ? 0 : 1)
    e = Matrix{Float64}(edges)                               # column-major (nbins + 1, ncols) == C [ncols][nbins + 1]
    size(e, 2) == ncols || error("edges must have one column per selected dimension (and one for the log-densities)")
    nbins = size(e, 1) - 1
    npairs = length(sel) * (length(sel) - 1) ÷ 2
    counts1 = zeros(Int64, nbins, ncols); outside = zeros(Int64, 3, ncols)
    counts2 = pairs ? zeros(Int64, nbins, nbins, npairs) : nothing
    nout = Ref{Int64}(0)
    st = ccall((:kmc_chain_histograms, LIB), Cint,
               (Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Int64, Ptr{UInt8}, Ptr{Int32}, Int32, Ptr{Float64}, Int32, Cint,
                Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
               chain, logp === nothing ? C_NULL : logp, ns, nw, nd, first_sample, mask === nothing ? C_NULL : mask, sel, Int32(length(sel)),
               e, Int32(nbins), Cint(device), counts1, outside, counts2 === nothing ? C_NULL : counts2, nout)
    st == 0 || error("kmc_chain_histograms failed ($st): $(last_error())")
    return counts1, outside, counts2, nout[]
end

"""
    corner(thetas; bins=32, range=nothing, dims=nothing, first_sample=0, walkers=nothing, device=0)

The numbers of a corner plot: `(dims, pairs, edges, hist1d, outside, hist2d, n)` as a named tuple, over `bins` equal bins between
`range = (lo, hi)` (one for all dimensions, or a vector of them), by default each dimension's minimum and maximum over the selection,
taken on the GPU (`kmc_chain_order_stats`; equal limits widened by 0.5 either way).  See `histograms` for the layouts.
"""
function corner(thetas; bins=32, range=nothing, dims=nothing, first_sample=0, walkers=nothing, device=0)
    chain, _, ns, nw, nd = _summary_chain(thetas, nothing)
    sel = dims === nothing ? collect(1:nd) : collect(dims)
    ext = Matrix{Float64}(undef, nd, 2)                      # every dimension's minimum and maximum over the selection: exact, on the device
    if range === nothing
        mask = _summary_mask(walkers, nw)
        n = (ns - first_sample) * (mask === nothing ? nw : count(!iszero, mask))
        n >= 1 || error("the selection is empty")
        nout = Ref{Int64}(0)
        st = ccall((:kmc_chain_order_stats, LIB), Cint,
                   (Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Int64, Ptr{UInt8}, Ptr{Int64}, Int32, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
                   chain, C_NULL, ns, nw, nd, first_sample, mask === nothing ? C_NULL : mask, Int64[0, n - 1], Int32(2), Cint(device), ext, C_NULL, nout)
        st == 0 || error("kmc_chain_order_stats failed ($st): $(last_error())")
    end
    edges = Matrix{Float64}(undef, bins + 1, length(sel))
    for (j, d) in enumerate(sel)
        lo, hi = range === nothing ? (ext[d, 1], ext[d, 2]) : (range isa Tuple ? range : range[j])
        lo == hi && ((lo, hi) = (lo - 0.5, hi + 0.5))
        edges[:, j] = collect(Base.range(lo, hi; length=bins + 1))
    end
    counts1, outside, counts2, n = histograms(thetas, edges; dims=sel, pairs=true, first_sample=first_sample, walkers=walkers, device=device)
    pairs = [(sel[a], sel[b]) for a in 1:length(sel) for b in a+1:length(sel)]
    return (dims=sel, pairs=pairs, edges=edges, hist1d=counts1, outside=outside, hist2d=counts2, n=n)
end

"""
    convergence(thetas; logdensities=nothing, first_sample=0, walkers=nothing, split=true, max_lag=nothing, device=0, rank=false)

Split-R-hat, effective sample size and Monte-Carlo standard error per dimension of `thetas[walker][sample]` as `emcee` /
`metropolis_chains` return it (and of `logdensities`, as a last column, when given), computed on the GPU (`kmc_chain_convergence`; the
definitions are in include/kissmcmc_hip.h: BDA3, Gelman et al. 2014, pp. 284-287).  Every selected walker is a chain, cut into halves
with `split`.  Returns a named tuple `(mean, std, rhat, ess, mcse, lag, truncated, m, h)`.  The walkers of ONE emcee ensemble are not
independent, so R-hat over them is optimistic (src/analysis.jl:69-71): pass the concatenated walkers of separate runs, or Metropolis chains.
`rank=true` adds `rhat_rank`, `ess_bulk` and `ess_tail` of `rank_convergence`.
"""
function convergence(thetas; logdensities=nothing, first_sample=0, walkers=nothing, split=true, max_lag=nothing, device=0, rank=false)
    chain, logp, ns, nw, nd = _summary_chain(thetas, logdensities)
    mask = _summary_mask(walkers, nw)
    ncols = nd + (logp === nothing ? 0 : 1)
    mean = Vector{Float64}(undef, ncols); W = similar(mean); B = similar(mean); var_plus = similar(mean)
    rhat = similar(mean); ess = similar(mean); mcse = similar(mean)
    T = Vector{Int64}(undef, ncols); flags = Vector{Int32}(undef, ncols)
    m = Ref{Int64}(0); h = Ref{Int64}(0)
    st = ccall((:kmc_chain_convergence, LIB), Cint,
               (Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Int64, Ptr{UInt8}, Int32, Int64, Cint,
                Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int32},
                Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
               chain, logp === nothing ? C_NULL : logp, ns, nw, nd, first_sample, mask === nothing ? C_NULL : mask, Int32(split ? 1 : 0),
               max_lag === nothing ? 0 : (max_lag == 0 ? -1 : max_lag), Cint(device),
               mean, W, B, var_plus, rhat, ess, mcse, T, flags, m, h, C_NULL)
    st == 0 || error("kmc_chain_convergence failed ($st): $(last_error())")
    out = (mean=mean, std=sqrt.(var_plus), rhat=rhat, ess=ess, mcse=mcse, lag=T, truncated=(flags .& Int32(2)) .!= 0, m=m[], h=h[])
    rank || return out
    r = rank_convergence(thetas; logdensities=logdensities, first_sample=first_sample, walkers=walkers, split=split, max_lag=max_lag, device=device)
    return merge(out, (rhat_rank=r.rhat, ess_bulk=r.ess_bulk, ess_tail=r.ess_tail))
end

"""
    rank_convergence(thetas; logdensities=nothing, first_sample=0, walkers=nothing, split=true, max_lag=nothing, device=0)

Rank-normalised R-hat with bulk and tail effective sample sizes (Vehtari et al. 2021), ranked on the GPU (`kmc_chain_rank_convergence`; the
definitions are in include/kissmcmc_hip.h).  Returns a named tuple `(rhat, rhat_bulk, rhat_folded, ess_bulk, ess_tail, ess_q05, ess_q95,
median, q05, q95, lag, truncated, has_nan, m, h)`; `lag` is `[column, transform]` for the bulk scores, the folded scores, `I05` and `I95`.
"""
function rank_convergence(thetas; logdensities=nothing, first_sample=0, walkers=nothing, split=true, max_lag=nothing, device=0)
    chain, logp, ns, nw, nd = _summary_chain(thetas, logdensities)
    mask = _summary_mask(walkers, nw)
    ncols = nd + (logp === nothing ? 0 : 1)
    cols = [Vector{Float64}(undef, ncols) for _ in 1:10]
    T = Matrix{Int64}(undef, ncols, 4); flags = Vector{Int32}(undef, ncols)
    m = Ref{Int64}(0); h = Ref{Int64}(0)
    st = ccall((:kmc_chain_rank_convergence, LIB), Cint,
               (Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Int64, Ptr{UInt8}, Int32, Int64, Cint,
                Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                Ptr{Float64}, Ptr{Int64}, Ptr{Int32}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
               chain, logp === nothing ? C_NULL : logp, ns, nw, nd, first_sample, mask === nothing ? C_NULL : mask, Int32(split ? 1 : 0),
               max_lag === nothing ? 0 : (max_lag == 0 ? -1 : max_lag), Cint(device),
               cols[1], cols[2], cols[3], cols[4], cols[5], cols[6], cols[7], cols[8], cols[9], cols[10], T, flags, m, h, C_NULL)
    st == 0 || error("kmc_chain_rank_convergence failed ($st): $(last_error())")
    return (rhat=cols[1], rhat_bulk=cols[2], rhat_folded=cols[3], ess_bulk=cols[4], ess_tail=cols[5], ess_q05=cols[6], ess_q95=cols[7],
            median=cols[8], q05=cols[9], q95=cols[10], lag=T, truncated=(flags .& Int32(2)) .!= 0, has_nan=(flags .& Int32(4)) .!= 0,
            m=m[], h=h[])
end

"""
    quantile_mcse(thetas, probs; logdensities=nothing, first_sample=0, walkers=nothing, split=true, max_lag=nothing, device=0)

Quantiles of the pooled draws with their effective sample sizes and Monte-Carlo standard errors (Vehtari et al. 2021), from bit-packed
indicator chains on the GPU (`kmc_chain_quantile_mcse`; the definitions are in include/kissmcmc_hip.h).  `probs`: 1 to 16 probabilities
strictly inside (0, 1).  Returns a named tuple `(quantile, ess, mcse, lower, upper, lag, flags, m, h)` of `[column, probability]` arrays.
"""
function quantile_mcse(thetas, probs; logdensities=nothing, first_sample=0, walkers=nothing, split=true, max_lag=nothing, device=0)
    chain, logp, ns, nw, nd = _summary_chain(thetas, logdensities)
    mask = _summary_mask(walkers, nw)
    ncols = nd + (logp === nothing ? 0 : 1)
    pr = collect(Float64, probs)
    cols = [Matrix{Float64}(undef, ncols, length(pr)) for _ in 1:5]          # column-major [column, probability] is the library's [nprobs][ncols]
    T = Matrix{Int64}(undef, ncols, length(pr)); flags = Matrix{Int32}(undef, ncols, length(pr))
    m = Ref{Int64}(0); h = Ref{Int64}(0)
    st = ccall((:kmc_chain_quantile_mcse, LIB), Cint,
               (Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Int64, Ptr{UInt8}, Int32, Int64, Int32, Ptr{Float64}, Cint,
                Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int32}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
               chain, logp === nothing ? C_NULL : logp, ns, nw, nd, first_sample, mask === nothing ? C_NULL : mask, Int32(split ? 1 : 0),
               max_lag === nothing ? 0 : (max_lag == 0 ? -1 : max_lag), Int32(length(pr)), pr, Cint(device),
               cols[1], cols[2], cols[3], cols[4], cols[5], T, flags, m, h, C_NULL)
    st == 0 || error("kmc_chain_quantile_mcse failed ($st): $(last_error())")
    return (quantile=cols[1], ess=cols[2], mcse=cols[3], lower=cols[4], upper=cols[5], lag=T, flags=flags, m=m[], h=h[])
end

"""
    covariance(thetas; logdensities=nothing, first_sample=0, walkers=nothing, device=0)

The covariance matrix of the posterior sample `thetas[walker][sample]` as `emcee` / `metropolis_chains` return it (and of `logdensities`,
as a last column, when given), summed on the GPU (`kmc_chain_covariance`; the definitions are in include/kissmcmc_hip.h), and the
correlation matrix taken from it on the host (`kmc_cov_correlation`).  Returns a named tuple `(mean, cov, corr, std, n)`; `cov` has
n - 1 in the denominator and is symmetric bit for bit.
"""
function covariance(thetas; logdensities=nothing, first_sample=0, walkers=nothing, device=0)
    chain, logp, ns, nw, nd = _summary_chain(thetas, logdensities)
    mask = _summary_mask(walkers, nw)
    ncols = nd + (logp === nothing ? 0 : 1)
    mean = Vector{Float64}(undef, ncols); sd = similar(mean)
    cov = Matrix{Float64}(undef, ncols, ncols); corr = similar(cov)      # symmetric: row- and column-major agree
    n = Ref{Int64}(0)
    st = ccall((:kmc_chain_covariance, LIB), Cint,
               (Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Int64, Ptr{UInt8}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}),
               chain, logp === nothing ? C_NULL : logp, ns, nw, nd, first_sample, mask === nothing ? C_NULL : mask, Cint(device),
               mean, cov, n, C_NULL)
    st == 0 || error("kmc_chain_covariance failed ($st): $(last_error())")
    st = ccall((:kmc_cov_correlation, LIB), Cint, (Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), ncols, cov, corr, sd)
    st == 0 || error("kmc_cov_correlation failed ($st): $(last_error())")
    return (mean=mean, cov=cov, corr=corr, std=sd, n=n[])
end

# the six parameters and the held-out observations (row-major [ndata][ncols] for the C ABI) of a pointwise call
_pointwise_params(pdf::DataDensity) = Float64[i <= length(pdf.p) ? pdf.p[i] : 0.0 for i in 1:6]
function _pointwise_data(data)
    data === nothing && return nothing, 0, 0
    D = data isa AbstractVector ? reshape(collect(Float64, data), :, 1) : collect(Float64, data)
    return permutedims(D), size(D, 1), size(D, 2)
end

"""
    waic(pdf::DataDensity, thetas; first_sample=0, thin=1, walkers=nothing, data=nothing, device=0)

WAIC of the data density `pdf` over the posterior sample `thetas[walker][sample]` as `emcee` returns it: the rows are the samples
`first_sample, first_sample + thin, ...` of the walkers `walkers`.  The term of every row and observation is evaluated on the GPU and
reduced per observation (`kmc_chain_pointwise_stats`), the host stage is `kmc_waic_stats`; the definitions are in
include/kissmcmc_hip.h.  Returns a named tuple `(elpd_waic, se, p_waic, lppd, waic, n_high, n_nan, n, lppd_j, p_waic_j, elpd_j)`;
`p_waic_j` has n - 1 in the denominator (BDA3, loo; ArviZ divides by n).  With `data` the observations are that held-out array
`[ndata, ncols]` instead of the density's own.
"""
function waic(pdf::DataDensity, thetas; first_sample=0, thin=1, walkers=nothing, data=nothing, device=0)
    chain, _, ns, nw, nd = _summary_chain(thetas, nothing)
    mask = _summary_mask(walkers, nw)
    D, nd2, nc2 = _pointwise_data(data)
    J = D === nothing ? pdf.ndata : nd2
    stats = Matrix{Float64}(undef, J, 4)                  # column-major [J, 4] is the C ABI's [4][J]
    n = Ref{Int64}(0)
    st = ccall((:kmc_chain_pointwise_stats, LIB), Cint,
               (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Int64, Ptr{UInt8}, Int64, Ptr{Float64}, Int64, Int32, Cint,
                Ptr{Float64}, Ptr{Int64}, Ptr{Int64}),
               pdf.handle, _pointwise_params(pdf), chain, ns, nw, nd, first_sample, mask === nothing ? C_NULL : mask, thin,
               D === nothing ? C_NULL : D, nd2, Int32(nc2), Cint(device), stats, n, C_NULL)
    st == 0 || error("kmc_chain_pointwise_stats failed ($st): $(last_error())")
    lppd_j = Vector{Float64}(undef, J); p_waic_j = similar(lppd_j); elpd_j = similar(lppd_j); tot = Vector{Float64}(undef, 7)
    st = ccall((:kmc_waic_stats, LIB), Cint, (Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
               J, n[], stats, lppd_j, p_waic_j, elpd_j, tot)
    st == 0 || error("kmc_waic_stats failed ($st): $(last_error())")
    return (elpd_waic=tot[3], se=tot[4], p_waic=tot[2], lppd=tot[1], waic=tot[5], n_high=Int(tot[6]), n_nan=Int(tot[7]), n=n[],
            lppd_j=lppd_j, p_waic_j=p_waic_j, elpd_j=elpd_j)
end

"""
    pointwise_loglike(pdf::DataDensity, thetas; first_sample=0, thin=1, walkers=nothing, obs=nothing, data=nothing, device=0)

The matrix `l[j, r] = term(x_r, d_j)` of the selected rows `r` (as for `waic`) and the observations `obs = (first, stop)`, 0-based and
half-open (all by default), evaluated on the GPU (`kmc_chain_pointwise_loglike`): an `(stop - first) x n` matrix, one column per row of
the chain -- what PSIS-LOO outside this package starts from.
"""
function pointwise_loglike(pdf::DataDensity, thetas; first_sample=0, thin=1, walkers=nothing, obs=nothing, data=nothing, device=0)
    chain, _, ns, nw, nd = _summary_chain(thetas, nothing)
    mask = _summary_mask(walkers, nw)
    D, nd2, nc2 = _pointwise_data(data)
    J = D === nothing ? pdf.ndata : nd2
    first, stop = obs === nothing ? (0, J) : obs
    nsel = mask === nothing ? nw : count(!iszero, mask)
    rows = cld(max(ns - first_sample, 0), max(thin, 1)) * nsel
    out = Matrix{Float64}(undef, max(stop - first, 1), max(rows, 1))     # column-major [count, n] is the C ABI's [n][count]
    n = Ref{Int64}(0)
    st = ccall((:kmc_chain_pointwise_loglike, LIB), Cint,
               (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Int64, Ptr{UInt8}, Int64, Ptr{Float64}, Int64, Int32, Int64, Int64,
                Cint, Ptr{Float64}, Ptr{Int64}),
               pdf.handle, _pointwise_params(pdf), chain, ns, nw, nd, first_sample, mask === nothing ? C_NULL : mask, thin,
               D === nothing ? C_NULL : D, nd2, Int32(nc2), first, stop - first, Cint(device), out, n)
    st == 0 || error("kmc_chain_pointwise_loglike failed ($st): $(last_error())")
    return out
end

"""
    loo(pdf::DataDensity, thetas; first_sample=0, thin=1, walkers=nothing, r_eff=1.0, obs=nothing, workspace=0, device=0, split=true, max_lag=0)

PSIS-LOO of the data density `pdf` over the posterior sample `thetas[walker][sample]`: the rows are those of `waic` (at least 5), the
observations `obs = (first, count)`, 0-based (all by default).  Selected, fitted and smoothed on the GPU (`kmc_chain_psis_loo`), the host
stage is `kmc_loo_stats`; the definition is in include/kissmcmc_hip.h.  Returns a named tuple `(elpd_loo, se, p_loo, looic, lppd, n_nan,
k_counts, n, elpd_loo_j, p_loo_j, pareto_k, n_tail_j, lppd_j)`; `k_counts` counts `pareto_k <= 0.5`, `(0.5, 0.7]`, `(0.7, 1]` and `> 1`;
`n_tail_j` is -1 for an observation whose outputs are NaN.  `r_eff` is one number, a vector with one entry per observation asked for, or
`:chain` to compute it per observation from the chain (`kmc_chain_psis_loo_reff`; `split`, `max_lag` as `relative_eff`); the tuple then
also holds `r_eff_j`, `tail_len_j` and `n_reff_nan`.
"""
function loo(pdf::DataDensity, thetas; first_sample=0, thin=1, walkers=nothing, r_eff=1.0, obs=nothing, workspace=0, device=0, split=true, max_lag=0)
    chain, _, ns, nw, nd = _summary_chain(thetas, nothing)
    mask = _summary_mask(walkers, nw)
    first, count = obs === nothing ? (0, pdf.ndata) : obs
    stats = Matrix{Float64}(undef, max(count, 1), 4)      # column-major [count, 4] is the C ABI's [4][count]
    lppd_j = Vector{Float64}(undef, max(count, 1))
    n = Ref{Int64}(0)
    r_eff_j = fill(NaN, max(count, 1)); tail_len_j = zeros(Int64, max(count, 1)); n_reff_nan = Ref{Int64}(0)
    if r_eff isa Real
        st = ccall((:kmc_chain_psis_loo, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Int64, Ptr{UInt8}, Int64, Float64, Int64, Int64, Int64, Cint,
                    Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}),
                   pdf.handle, _pointwise_params(pdf), chain, ns, nw, nd, first_sample, mask === nothing ? C_NULL : mask, thin, Float64(r_eff),
                   first, count, workspace, Cint(device), stats, lppd_j, n, C_NULL)
        st == 0 || error("kmc_chain_psis_loo failed ($st): $(last_error())")
    else
        r_eff === :chain || length(r_eff) == count || error("r_eff must have one entry per observation asked for ($count)")
        given = r_eff === :chain ? C_NULL : Vector{Float64}(r_eff)
        st = ccall((:kmc_chain_psis_loo_reff, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Int64, Ptr{UInt8}, Int64, Ptr{Float64}, Int32, Int64, Int64, Int64,
                    Int64, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
                   pdf.handle, _pointwise_params(pdf), chain, ns, nw, nd, first_sample, mask === nothing ? C_NULL : mask, thin, given,
                   Int32(split), max_lag, first, count, workspace, Cint(device), stats, lppd_j, r_eff_j, tail_len_j, n_reff_nan, n, C_NULL)
        st == 0 || error("kmc_chain_psis_loo_reff failed ($st): $(last_error())")
    end
    p_loo_j = similar(lppd_j); tot = Vector{Float64}(undef, 10)
    st = ccall((:kmc_loo_stats, LIB), Cint, (Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
               count, n[], stats, lppd_j, p_loo_j, tot)
    st == 0 || error("kmc_loo_stats failed ($st): $(last_error())")
    return (elpd_loo=tot[1], se=tot[2], p_loo=tot[3], looic=tot[4], lppd=tot[5], n_nan=Int(tot[6]), k_counts=Tuple(Int.(tot[7:10])), n=n[],
            elpd_loo_j=stats[:, 1], p_loo_j=p_loo_j, pareto_k=stats[:, 2], n_tail_j=[isnan(v) ? -1 : Int(v) for v in stats[:, 3]], lppd_j=lppd_j,
            r_eff_j=r_eff isa Real ? fill(Float64(r_eff), max(count, 1)) : r_eff_j, tail_len_j=tail_len_j, n_reff_nan=n_reff_nan[])
end

"""
    relative_eff(pdf::DataDensity, thetas; first_sample=0, thin=1, walkers=nothing, obs=nothing, split=true, max_lag=0, workspace=0, device=0)

The relative efficiency of PSIS-LOO's importance weights per observation (`kmc_chain_relative_eff`): `r_eff_j = ess_j / (m h)` with
`ess`, `m`, `h` those of `convergence` on the series `exp(l[k][j] - max_r l[r][j])` of the selected rows.  Returns a named tuple
`(r_eff_j, ess_j, lag, truncated, m, h, n)`; `obs = (first, count)`, 0-based.  `r_eff_j` is NaN for a constant column and may exceed 1.
"""
function relative_eff(pdf::DataDensity, thetas; first_sample=0, thin=1, walkers=nothing, obs=nothing, split=true, max_lag=0, workspace=0, device=0)
    chain, _, ns, nw, nd = _summary_chain(thetas, nothing)
    mask = _summary_mask(walkers, nw)
    first, count = obs === nothing ? (0, pdf.ndata) : obs
    k = max(count, 1)
    r = fill(NaN, k); ess = fill(NaN, k); T = zeros(Int64, k); flags = zeros(Int32, k)
    m = Ref{Int64}(0); h = Ref{Int64}(0); n = Ref{Int64}(0)
    st = ccall((:kmc_chain_relative_eff, LIB), Cint,
               (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Int64, Ptr{UInt8}, Int64, Int64, Int64, Int32, Int64, Int64, Cint,
                Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int32}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
               pdf.handle, _pointwise_params(pdf), chain, ns, nw, nd, first_sample, mask === nothing ? C_NULL : mask, thin, first, count,
               Int32(split), max_lag, workspace, Cint(device), r, ess, T, flags, m, h, n, C_NULL)
    st == 0 || error("kmc_chain_relative_eff failed ($st): $(last_error())")
    return (r_eff_j=r, ess_j=ess, lag=T, truncated=(flags .& Int32(2)) .!= 0, m=m[], h=h[], n=n[])
end

"""
    compare_loo(a, b)

The difference of two models' `elpd_loo` over the same observations, from two `loo` results: `(elpd_diff, se, J)` with
`se = sqrt(J var(elpd_loo_j(a) - elpd_loo_j(b)))` (sample variance); positive `elpd_diff`: `a` predicts better.  No device.
"""
function compare_loo(a, b)
    length(a.elpd_loo_j) == length(b.elpd_loo_j) || error("the two results are not over the same observations")
    d = a.elpd_loo_j .- b.elpd_loo_j
    J = length(d)
    m = sum(d) / J
    return (elpd_diff=sum(d), se=J > 1 ? sqrt(J * sum((d .- m) .^ 2) / (J - 1)) : NaN, J=J)
end

"""
    rank_scores(thetas; logdensities=nothing, first_sample=0, walkers=nothing, split=true, folded=false, device=0)

The exact ranks of the pooled draws and their normal scores, ranked on the GPU (`kmc_chain_rank_scores`): a named tuple `(rank2, z, centre,
nan_count, S, m, h)` with `rank2[sample, chain, column] = #{y < x} + #{y <= x} + 1` (twice the average 1-based rank) and `z` its normal score;
with `folded` the draws are folded about their column's median (`centre`) first.
"""
function rank_scores(thetas; logdensities=nothing, first_sample=0, walkers=nothing, split=true, folded=false, device=0)
    chain, logp, ns, nw, nd = _summary_chain(thetas, logdensities)
    mask = _summary_mask(walkers, nw)
    ncols = nd + (logp === nothing ? 0 : 1)
    nsel = mask === nothing ? nw : count(!iszero, mask)
    n = max(ns - first_sample, 0)
    hh = split ? n ÷ 2 : n
    mm = (split ? 2 : 1) * nsel
    rank2 = zeros(Int64, hh, mm, ncols); z = fill(NaN, hh, mm, ncols)
    centre = fill(NaN, ncols); nan_count = zeros(Int64, ncols)
    m = Ref{Int64}(0); h = Ref{Int64}(0)
    st = ccall((:kmc_chain_rank_scores, LIB), Cint,
               (Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Int64, Ptr{UInt8}, Int32, Int32, Cint,
                Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
               chain, logp === nothing ? C_NULL : logp, ns, nw, nd, first_sample, mask === nothing ? C_NULL : mask, Int32(split ? 1 : 0),
               Int32(folded ? 1 : 0), Cint(device), rank2, z, centre, nan_count, m, h)
    st == 0 || error("kmc_chain_rank_scores failed ($st): $(last_error())")
    return (rank2=rank2, z=z, centre=folded ? centre : nothing, nan_count=nan_count, S=m[] * h[], m=m[], h=h[])
end

"""
    hdi(thetas; prob=0.94, logdensities=nothing, first_sample=0, walkers=nothing, device=0)

Highest-density intervals per dimension of `thetas[walker][sample]` as `emcee` / `metropolis_chains` return it (and of `logdensities`, as
a last column, when given): the narrowest interval `[x_(i), x_(i + k)]` of the sorted draws with `k = floor(prob * N)`, the smallest `i`
among equal widths, sorted and scanned on the GPU (`kmc_chain_hdi`; the definition is in include/kissmcmc_hip.h).  Returns a named tuple
`(lo, hi, width, start, k, n, has_nan)`: vectors over the columns for a scalar `prob`, `nprob x ncols` matrices for a vector of up to 16;
`start` is 0-based, -1 with NaN ends for a column that holds a NaN.
"""
function hdi(thetas; prob=0.94, logdensities=nothing, first_sample=0, walkers=nothing, device=0)
    chain, logp, ns, nw, nd = _summary_chain(thetas, logdensities)
    mask = _summary_mask(walkers, nw)
    ncols = nd + (logp === nothing ? 0 : 1)
    probs = prob isa Number ? Float64[prob] : collect(Float64, prob)
    np = length(probs)
    lo = fill(NaN, ncols, np); hi = fill(NaN, ncols, np); start = fill(Int64(-1), ncols, np)       # column-major: C's [nprob][ncols]
    nan_count = zeros(Int64, ncols); n = Ref{Int64}(0)
    st = ccall((:kmc_chain_hdi, LIB), Cint,
               (Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Int64, Ptr{UInt8}, Ptr{Float64}, Int32, Cint,
                Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
               chain, logp === nothing ? C_NULL : logp, ns, nw, nd, first_sample, mask === nothing ? C_NULL : mask, probs, Int32(np), Cint(device),
               lo, hi, start, n, nan_count, C_NULL)
    st == 0 || error("kmc_chain_hdi failed ($st): $(last_error())")
    k = Vector{Int64}(undef, np)
    for (i, p) in enumerate(probs)
        ki = Ref{Int64}(0)
        st = ccall((:kmc_hdi_span, LIB), Cint, (Int64, Float64, Ptr{Int64}, Ptr{Int64}), n[], p, ki, C_NULL)
        st == 0 || error("kmc_hdi_span failed ($st): $(last_error())")
        k[i] = ki[]
    end
    has_nan = nan_count .> 0
    prob isa Number && return (lo=lo[:, 1], hi=hi[:, 1], width=hi[:, 1] .- lo[:, 1], start=start[:, 1], k=k[1], n=n[], has_nan=has_nan)
    return (lo=permutedims(lo), hi=permutedims(hi), width=permutedims(hi .- lo), start=permutedims(start), k=k, n=n[], has_nan=has_nan)
end

# make_theta0s (src/samplers.jl:311-349) and squash_walkers (src/samplers.jl:372-428): KissMCMC's own, imported above.

end # module
