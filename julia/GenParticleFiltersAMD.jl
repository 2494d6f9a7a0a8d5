# GenParticleFiltersAMD.jl -- Julia binding of libgpf_hip.so (include/gpf.h).
#
# UNTESTED in this repository's CI: the build image has no Julia (SURVEY.md F6). It is the thin `ccall`
# layer a maintainer of GenParticleFilters.jl would add so that the device state type participates in the
# package's generic functions.  Every method mirrors the signature of the reference method it stands in
# for (file:line of GenParticleFilters.jl v0.2.3 in the comments).
module GenParticleFiltersAMD

import GenParticleFilters: pf_resize!, pf_multinomial_resize!, pf_residual_resize!, pf_optimal_resize!, pf_replicate!, pf_dereplicate!
import GenParticleFilters: pf_coalesce!, pf_introduce!
import GenParticleFilters: pf_initialize, pf_update!, pf_resample!, pf_multinomial_resample!,
    pf_residual_resample!, pf_stratified_resample!, pf_rejuvenate!, pf_move_accept!, pf_move_reweight!,
    get_log_norm_weights, get_norm_weights, get_ess, get_lml_est
import Gen: effective_sample_size, log_ml_estimate, get_log_weights, sample_unweighted_traces
using Gen: get_choices
import Statistics: mean, var

const libgpf = get(ENV, "LIBGPF_HIP", "libgpf_hip.so")
const GPF_ABI_VERSION = Cint(1)

"Native model descriptor: replaces `model::GenerativeFunction` (src/initialize.jl:31-35)."
struct NativeModel
    id::Cint                 # gpf_model
    params::Vector{Float64}  # layout of csrc/gpf_models.hpp
    dim::Int
end

struct GpfConfig
    abi_version::Cint; model::Cint; n_params::Cint; keep_prev::Cint
    params::Ptr{Cdouble}
    n_particles::Int64; n_global::Int64; gid0::Int64
    seed::UInt64
    device::Cint; reserved::Cint
    stream::Ptr{Cvoid}
end

"Device-resident counterpart of Gen.ParticleFilterState (traces/new_traces/log_weights/log_ml_est/parents)."
mutable struct DeviceParticleFilterState
    handle::Ptr{Cvoid}
    model::NativeModel
    n_particles::Int
    # history = T: the trajectory store for T time steps (gpf.h gpf_history_enable); history_blocks: the block-wise store, which the block-wise
    # calls feed too (gpf_history_enable_blocks); history_weights: that store with every step's log-weights and per-block observations, which
    # block_backward_trajectories needs (gpf_history_enable_blocks_weights); forward: forward-only smoothing per block (gpf_forward_enable_blocks), with
    # the block-wise store or without a store
    function DeviceParticleFilterState(model::NativeModel, n::Int; seed::Integer=1, keep_prev::Bool=false, device::Integer=0, history::Integer=0,
                                       history_blocks::Bool=false, history_weights::Bool=false, forward::Bool=false)
        history_weights && !(history > 0 && history_blocks) && error("history_weights needs the block-wise trajectory store (history = T)")
        h = Ref{Ptr{Cvoid}}(C_NULL)
        GC.@preserve model begin
            cfg = Ref(GpfConfig(GPF_ABI_VERSION, model.id, length(model.params), keep_prev, pointer(model.params),
                                n, n, 0, UInt64(seed), device, 0, C_NULL))
            st = ccall((:gpf_create, libgpf), Cint, (Ref{GpfConfig}, Ref{Ptr{Cvoid}}), cfg, h)
        end
        st == 0 || error(unsafe_string(ccall((:gpf_last_error, libgpf), Cstring, (Ptr{Cvoid},), C_NULL)))
        state = new(h[], model, n)
        finalizer(s -> ccall((:gpf_destroy, libgpf), Cint, (Ptr{Cvoid},), getfield(s, :handle)), state)
        if history > 0
            st = history_weights ? ccall((:gpf_history_enable_blocks_weights, libgpf), Cint, (Ptr{Cvoid}, Cint), h[], history) :
                 history_blocks ? ccall((:gpf_history_enable_blocks, libgpf), Cint, (Ptr{Cvoid}, Cint), h[], history) :
                                  ccall((:gpf_history_enable, libgpf), Cint, (Ptr{Cvoid}, Cint), h[], history)
            st == 0 || error(unsafe_string(ccall((:gpf_last_error, libgpf), Cstring, (Ptr{Cvoid},), h[])))
        end
        if forward
            st = ccall((:gpf_forward_enable_blocks, libgpf), Cint, (Ptr{Cvoid},), h[])
            st == 0 || error(unsafe_string(ccall((:gpf_last_error, libgpf), Cstring, (Ptr{Cvoid},), h[])))
        end
        return state
    end
    # wrap an existing handle (a sub-state view created by gpf_view_create)
    function DeviceParticleFilterState(handle::Ptr{Cvoid}, model::NativeModel, n::Int)
        state = new(handle, model, n)
        finalizer(s -> ccall((:gpf_destroy, libgpf), Cint, (Ptr{Cvoid},), getfield(s, :handle)), state)
        return state
    end
end

# state[a:b] / view(state, a:b): ParticleFilterSubState over a contiguous range (src/view.jl:35-48); every method of this
# file accepts the returned object (it is a DeviceParticleFilterState whose handle aliases the source's particles)
function Base.getindex(s::DeviceParticleFilterState, r::UnitRange{Int})
    h = Ref{Ptr{Cvoid}}(C_NULL)
    _status(s, ccall((:gpf_view_create, libgpf), Cint, (Ptr{Cvoid}, Int64, Int64, Ref{Ptr{Cvoid}}), getfield(s, :handle), first(r) - 1, length(r), h))
    return DeviceParticleFilterState(h[], getfield(s, :model), length(r))
end
Base.view(s::DeviceParticleFilterState, r::UnitRange{Int}) = s[r]
# state[k:5:100] (test/initialize.jl:60, test/update.jl:33): a strided sub-state; particle i of the view is particle first(r) + (i-1) step(r)
function Base.getindex(s::DeviceParticleFilterState, r::StepRange{Int,Int})
    step(r) >= 1 || error("sub-state ranges need a positive step")
    h = Ref{Ptr{Cvoid}}(C_NULL)
    _status(s, ccall((:gpf_view_create_strided, libgpf), Cint, (Ptr{Cvoid}, Int64, Int64, Int64, Ref{Ptr{Cvoid}}), getfield(s, :handle), first(r) - 1, step(r), length(r), h))
    return DeviceParticleFilterState(h[], getfield(s, :model), length(r))
end
Base.view(s::DeviceParticleFilterState, r::StepRange{Int,Int}) = s[r]
# state[idxs] for ANY vector of distinct indices (src/view.jl:35-48 takes idxs::AbstractVector): the same compact-copy view over an index array
function Base.getindex(s::DeviceParticleFilterState, idxs::AbstractVector{<:Integer})
    ix = Int64.(idxs) .- 1
    h = Ref{Ptr{Cvoid}}(C_NULL)
    _status(s, ccall((:gpf_view_create_indexed, libgpf), Cint, (Ptr{Cvoid}, Ptr{Int64}, Int64, Ref{Ptr{Cvoid}}), getfield(s, :handle), ix, length(ix), h))
    return DeviceParticleFilterState(h[], getfield(s, :model), length(ix))
end
Base.getindex(s::DeviceParticleFilterState, mask::AbstractVector{Bool}) = s[findall(mask)]
Base.view(s::DeviceParticleFilterState, idxs::AbstractVector{<:Integer}) = s[idxs]

# status helper; NOT called `check`: the resamplers take a keyword of that name (src/resample.jl:43-46) which would shadow it
_status(state, st) = st == 0 ? nothing :
    error(unsafe_string(ccall((:gpf_last_error, libgpf), Cstring, (Ptr{Cvoid},), state.handle)))   # ErrorException

# src/initialize.jl:31-44
function pf_initialize(model::NativeModel, model_args::Tuple, observations::Vector{Float64}, n_particles::Int; kw...)
    state = DeviceParticleFilterState(model, n_particles; kw...)
    _status(state, ccall((:gpf_initialize, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint),
                       state.handle, observations, length(observations)))
    return state
end

# src/update.jl:12-25
function pf_update!(state::DeviceParticleFilterState, new_args::Tuple, argdiffs::Tuple, observations::Vector{Float64})
    _status(state, ccall((:gpf_update, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint),
                       state.handle, observations, length(observations)))
    return state
end

"Native proposal for pf_initialize / pf_update! (src/initialize.jl:46-62, src/update.jl:79-96): exact conditional of the LG-SSM"
struct LocallyOptimal end
function pf_initialize(model::NativeModel, model_args::Tuple, observations::Vector{Float64}, proposal::LocallyOptimal, proposal_args::Tuple, n_particles::Int; kw...)
    state = DeviceParticleFilterState(model, n_particles; kw...)
    _status(state, ccall((:gpf_initialize_proposal, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cint), state.handle, observations, length(observations), 1))
    return state
end
function pf_update!(state::DeviceParticleFilterState, new_args::Tuple, argdiffs::Tuple, observations::Vector{Float64}, proposal::LocallyOptimal, proposal_args::Tuple)
    _status(state, ccall((:gpf_update_proposal, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cint), state.handle, observations, length(observations), 1))
    return state
end

"priority_fn = w -> alpha*w evaluated on the GPU (test/resample.jl:15 uses alpha = 1/2)"
struct Tempering; alpha::Float64; end
(t::Tempering)(w) = t.alpha * w

function _resample!(state, method::Int, priority_fn, check_kw, sort_particles::Bool)
    chk = check_kw === true ? 2 : (check_kw === :warn ? 1 : 0)
    invalid = Ref{Cint}(0)
    inv_ptr = chk == 0 ? Ptr{Cint}(C_NULL) : Base.unsafe_convert(Ptr{Cint}, invalid)
    GC.@preserve invalid begin
        if priority_fn === nothing || priority_fn isa Tempering
            alpha = priority_fn === nothing ? NaN : priority_fn.alpha
            st = ccall((:gpf_resample, libgpf), Cint, (Ptr{Cvoid}, Cint, Cdouble, Cint, Cint, Ptr{Cint}),
                       state.handle, method, alpha, sort_particles, chk, inv_ptr)
        else    # arbitrary closure: priority_fn.(log_weights) on the host (src/resample.jl:51-52)
            lp = priority_fn.(get_log_weights(state))
            st = ccall((:gpf_resample_with_priorities, libgpf), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Cint, Cint, Ptr{Cint}),
                       state.handle, method, lp, sort_particles, chk, inv_ptr)
        end
    end
    _status(state, st)                                            # error("Invalid weights."), src/resample.jl:55
    check_kw === :warn && invalid[] != 0 && @warn("Invalid weights: resampled with uniform weights.")   # utils.jl:120-135
    return state
end

"""
    pf_step_ess!(state, new_args, argdiffs, observations; ess_threshold=0.5, method=:multinomial, rejuvenate=nothing, n_iters=1, check=:warn, sort_particles=true)

One iteration of the README loop (README.md:66-77) in one ccall (gpf.h gpf_step_ess): `if effective_sample_size(state) < ess_threshold * N;
pf_resample!(state, method); pf_rejuvenate!(state, ...; method=rejuvenate); end; pf_update!(state, new_args, argdiffs, observations)` -- the
same results, without the host's round trip on the steps that do not resample.  Returns whether it resampled.
"""
function pf_step_ess!(s::DeviceParticleFilterState, new_args::Tuple, argdiffs::Tuple, observations::Vector{Float64}; ess_threshold::Real=0.5,
                      method::Symbol=:multinomial, rejuvenate::Union{Nothing,Symbol}=nothing, n_iters::Int=1, check=:warn, sort_particles::Bool=true)
    mid = method == :multinomial ? 0 : method == :residual ? 1 : method == :stratified ? 2 : method == :multinomial_sorted ? 4 : error("Resampling method $method not recognized.")
    rid = rejuvenate === nothing ? -1 : rejuvenate == :move ? 0 : rejuvenate == :reweight ? 1 : error("Method $rejuvenate not recognized.")
    chk = check === true ? 2 : (check === :warn ? 1 : 0)
    resampled = Ref{Cint}(0); invalid = Ref{Cint}(0)
    GC.@preserve resampled invalid begin
        st = ccall((:gpf_step_ess, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cdouble, Cint, Cint, Cint, Cint, Cint, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}),
                   s.handle, observations, length(observations), Float64(ess_threshold), mid, sort_particles, chk, rid, n_iters,
                   Base.unsafe_convert(Ptr{Cint}, resampled), chk == 0 ? Ptr{Cint}(C_NULL) : Base.unsafe_convert(Ptr{Cint}, invalid), Ptr{Cdouble}(C_NULL))
    end
    _status(s, st)
    check === :warn && invalid[] != 0 && @warn("Invalid weights: resampled with uniform weights.")
    return resampled[] != 0
end

"opt-in: pf_resample!(state, :multinomial) leaves its ancestor search to the pf_update! that follows (one fused kernel; gpf.h gpf_set_lazy_search)"
set_lazy_search!(s::DeviceParticleFilterState, enable::Bool=true) =
    (_status(s, ccall((:gpf_set_lazy_search, libgpf), Cint, (Ptr{Cvoid}, Cint), s.handle, enable ? 1 : 0)); s)
"checkpoint / resume (gpf.h gpf_checkpoint_*): the whole state as one byte vector; `restore!` on a state created with the same arguments continues bit for bit"
function checkpoint(s::DeviceParticleFilterState)
    nb = Ref{Int64}(0)
    _status(s, ccall((:gpf_checkpoint_size, libgpf), Cint, (Ptr{Cvoid}, Ptr{Int64}), s.handle, nb))
    blob = Vector{UInt8}(undef, nb[])
    _status(s, ccall((:gpf_checkpoint_save, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64), s.handle, blob, nb[]))
    return blob
end
restore!(s::DeviceParticleFilterState, blob::Vector{UInt8}) =
    (_status(s, ccall((:gpf_checkpoint_load, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64), s.handle, blob, length(blob))); s)
"opt-in extension (gpf.h GPF_RESAMPLE_MULTINOMIAL_SORTED): multinomial resampling with the uniforms drawn already sorted -- state.parents non-decreasing"
pf_multinomial_sorted_resample!(s::DeviceParticleFilterState; priority_fn=nothing, check=:warn) = _resample!(s, 4, priority_fn, check, true)

# src/resample.jl:48-65, 85-120, 143-175, 19-30
pf_multinomial_resample!(s::DeviceParticleFilterState; priority_fn=nothing, check=:warn) = _resample!(s, 0, priority_fn, check, true)
pf_residual_resample!(s::DeviceParticleFilterState; priority_fn=nothing, check=:warn) = _resample!(s, 1, priority_fn, check, true)
pf_stratified_resample!(s::DeviceParticleFilterState; priority_fn=nothing, check=:warn, sort_particles::Bool=true) =
    _resample!(s, 2, priority_fn, check, sort_particles)
function pf_resample!(s::DeviceParticleFilterState, method::Symbol=:multinomial; kwargs...)
    method == :multinomial && return pf_multinomial_resample!(s; kwargs...)
    method == :residual && return pf_residual_resample!(s; kwargs...)
    method == :stratified && return pf_stratified_resample!(s; kwargs...)
    method == :multinomial_sorted && return pf_multinomial_sorted_resample!(s; kwargs...)      # (extension)
    error("Resampling method $method not recognized.")
end

# Many small filters in one state: the batched form of
#     for b in blocks; (ess_frac === nothing || get_ess(state[b]) < ess_frac * length(b)) && pf_resample!(state[b], method; ...); end
# over consecutive blocks of block_size particles (<= 2048) in ONE launch (gpf.h gpf_resample_blocks; sub-state semantics of
# src/resample.jl:185-187,205-218, README.md:60-79 per block).  Returns the number of blocks that resampled.
function pf_resample_blocks!(s::DeviceParticleFilterState, block_size::Int, method::Symbol=:multinomial;
                             priority_fn::Union{Nothing,Tempering}=nothing, ess_frac=nothing, sort_particles::Bool=true, check=:warn)
    m = method == :multinomial ? 0 : method == :residual ? 1 : method == :stratified ? 2 : error("Resampling method $method not recognized.")
    chk = check === true ? 2 : (check === :warn ? 1 : 0)
    invalid = Ref{Cint}(0); count = Ref{Int64}(0)
    st = ccall((:gpf_resample_blocks, libgpf), Cint, (Ptr{Cvoid}, Cint, Int64, Cdouble, Cint, Cdouble, Cint, Ptr{Cint}, Ptr{Int64}),
               s.handle, m, block_size, priority_fn === nothing ? NaN : priority_fn.alpha, sort_particles ? 1 : 0,
               ess_frac === nothing ? NaN : Float64(ess_frac), chk, invalid, count)
    _status(s, st)
    check === :warn && invalid[] != 0 && @warn("Invalid weights in some block: resampled with uniform weights.")
    return Int(count[])
end
# Conditional SMC, the resampling half (gpf.h gpf_resample_blocks_conditional; Andrieu, Doucet & Holenstein 2010): multinomial block-wise resampling in
# which slot 0 of every block that resamples keeps itself (parent 0); the other slots draw as in pf_resample_blocks!.  Blocks of <= 2048 particles.
function pf_resample_blocks_conditional!(s::DeviceParticleFilterState, block_size::Int; ess_frac=nothing, check=:warn)
    chk = check === true ? 2 : (check === :warn ? 1 : 0)
    invalid = Ref{Cint}(0); count = Ref{Int64}(0)
    st = ccall((:gpf_resample_blocks_conditional, libgpf), Cint, (Ptr{Cvoid}, Cint, Int64, Cdouble, Cint, Ptr{Cint}, Ptr{Int64}),
               s.handle, 0, block_size, ess_frac === nothing ? NaN : Float64(ess_frac), chk, invalid, count)
    _status(s, st)
    check === :warn && invalid[] != 0 && @warn("Invalid weights in some block: resampled with uniform weights.")
    return Int(count[])
end
# Particle Gibbs with ancestor sampling, the resampling half (gpf.h gpf_resample_blocks_ancestor; Lindsten, Jordan & Schoen 2014): the conditional call in
# which slot 0 of every block that resamples draws its ancestor with probability proportional to w_i f(reference[:, b] | x_i).  observations (n_obs, n_blocks)
# and reference (dim, n_blocks), column b for block b: the arguments of the pf_update_blocks_ref! that follows -- the step being entered.
function pf_resample_blocks_ancestor!(s::DeviceParticleFilterState, block_size::Int, observations::Matrix{Float64}, reference::Matrix{Float64};
                                      ess_frac=nothing, check=:warn)
    chk = check === true ? 2 : (check === :warn ? 1 : 0)
    invalid = Ref{Cint}(0); count = Ref{Int64}(0)
    st = ccall((:gpf_resample_blocks_ancestor, libgpf), Cint, (Ptr{Cvoid}, Cint, Int64, Cdouble, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Ptr{Cint}, Ptr{Int64}),
               s.handle, 0, block_size, ess_frac === nothing ? NaN : Float64(ess_frac), chk, observations, size(observations, 1),
               reference, size(reference, 1), invalid, count)
    _status(s, st)
    check === :warn && invalid[] != 0 && @warn("Invalid weights in some block: resampled with uniform weights.")
    return Int(count[])
end
"the ancestor log-weights lw_i + log f(reference[:, b] | x_i) of every particle, b its block (gpf.h gpf_block_ancestor_log_weights): one launch, nothing changes"
function block_ancestor_log_weights(s::DeviceParticleFilterState, block_size::Int, observations::Matrix{Float64}, reference::Matrix{Float64})
    out = Vector{Float64}(undef, s.n_particles)
    _status(s, ccall((:gpf_block_ancestor_log_weights, libgpf), Cint, (Ptr{Cvoid}, Int64, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}),
                     s.handle, block_size, observations, size(observations, 1), reference, size(reference, 1), out))
    return out
end
"(effective_sample_size(state[b]), log_ml_estimate(state[b])) of every block of block_size particles (src/utils.jl:163-178), one launch"
function block_stats(s::DeviceParticleFilterState, block_size::Int)
    nb = cld(s.n_particles, block_size)
    ess = Vector{Float64}(undef, nb); lml = Vector{Float64}(undef, nb)
    _status(s, ccall((:gpf_block_stats, libgpf), Cint, (Ptr{Cvoid}, Int64, Ptr{Cdouble}, Ptr{Cdouble}), s.handle, block_size, ess, lml))
    return ess, lml
end
# The state estimates of every block: for b in blocks; mean(state[b], addr); var(state[b], addr); proportionmap(state[b], addr); end
# (src/statistics.jl:13-14, 48-50, 91-101 on sub-states) in one launch, bit-identical to the loop over views (gpf.h gpf_block_moments,
# gpf_block_proportion).  Matrices are (row_width, n_blocks) / (n_values, n_blocks): column b for block b.  addr = 0-based column.
function _row_width(s::DeviceParticleFilterState)
    dim = Ref{Cint}(0); w = Ref{Cint}(0)
    _status(s, ccall((:gpf_state_dim, libgpf), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Cint}), s.handle, dim, w))
    return Int(w[])
end
function block_moments(s::DeviceParticleFilterState, block_size::Int)
    nb = cld(s.n_particles, block_size); W = _row_width(s)
    mu = Matrix{Float64}(undef, W, nb); s2 = Matrix{Float64}(undef, W, nb)
    _status(s, ccall((:gpf_block_moments, libgpf), Cint, (Ptr{Cvoid}, Int64, Ptr{Cdouble}, Ptr{Cdouble}), s.handle, block_size, mu, s2))
    return mu, s2
end
function block_mean(s::DeviceParticleFilterState, block_size::Int, addr::Union{Nothing,Integer}=nothing)
    nb = cld(s.n_particles, block_size); W = _row_width(s)
    mu = Matrix{Float64}(undef, W, nb)
    _status(s, ccall((:gpf_block_moments, libgpf), Cint, (Ptr{Cvoid}, Int64, Ptr{Cdouble}, Ptr{Cdouble}), s.handle, block_size, mu, C_NULL))
    return addr === nothing ? mu : mu[addr + 1, :]
end
function block_var(s::DeviceParticleFilterState, block_size::Int, addr::Union{Nothing,Integer}=nothing)
    nb = cld(s.n_particles, block_size); W = _row_width(s)
    s2 = Matrix{Float64}(undef, W, nb)
    _status(s, ccall((:gpf_block_moments, libgpf), Cint, (Ptr{Cvoid}, Int64, Ptr{Cdouble}, Ptr{Cdouble}), s.handle, block_size, C_NULL, s2))
    return addr === nothing ? s2 : s2[addr + 1, :]
end
# A PAST choice per block: for b in blocks; mean(state[b], t => addr); ...; end (a sub-state is a slice of persistent traces, src/view.jl:35-48) from the
# block-wise trajectory store (pf_initialize_blocks(...; history=T); gpf.h gpf_block_history_moments, gpf_block_history_proportion).  Matrices are
# (dim, n_blocks): the store keeps the latent columns.  Without the store the library refuses (ErrorException naming the trajectory store).
function _latent_dim(s::DeviceParticleFilterState)
    dim = Ref{Cint}(0); w = Ref{Cint}(0)
    _status(s, ccall((:gpf_state_dim, libgpf), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Cint}), s.handle, dim, w))
    return Int(dim[])
end
function block_moments(s::DeviceParticleFilterState, block_size::Int, step::Integer)
    nb = cld(s.n_particles, block_size); d = _latent_dim(s)
    mu = Matrix{Float64}(undef, d, nb); s2 = Matrix{Float64}(undef, d, nb)
    _status(s, ccall((:gpf_block_history_moments, libgpf), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Cdouble}, Ptr{Cdouble}), s.handle, step, block_size, mu, s2))
    return mu, s2
end
function block_mean(s::DeviceParticleFilterState, block_size::Int, addr::Pair{<:Integer,<:Integer})
    nb = cld(s.n_particles, block_size); d = _latent_dim(s)
    mu = Matrix{Float64}(undef, d, nb)
    _status(s, ccall((:gpf_block_history_moments, libgpf), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Cdouble}, Ptr{Cdouble}), s.handle, addr.first, block_size, mu, C_NULL))
    return mu[addr.second + 1, :]
end
function block_var(s::DeviceParticleFilterState, block_size::Int, addr::Pair{<:Integer,<:Integer})
    nb = cld(s.n_particles, block_size); d = _latent_dim(s)
    s2 = Matrix{Float64}(undef, d, nb)
    _status(s, ccall((:gpf_block_history_moments, libgpf), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Cdouble}, Ptr{Cdouble}), s.handle, addr.first, block_size, C_NULL, s2))
    return s2[addr.second + 1, :]
end
function block_proportionmap(s::DeviceParticleFilterState, block_size::Int, addr::Pair{<:Integer,<:Integer}; max_values::Int=256)
    col = Vector{Float64}(undef, s.n_particles)
    _status(s, ccall((:gpf_history_column, libgpf), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Int64), s.handle, addr.first, addr.second, col, length(col)))
    vals = sort(unique(col))
    length(vals) > max_values && error("proportionmap: $(length(vals)) distinct values; the column does not look discrete")
    nb = cld(s.n_particles, block_size)
    out = Matrix{Float64}(undef, length(vals), nb)
    for k0 in 1:16:length(vals)
        chunk = vals[k0:min(k0 + 15, length(vals))]
        part = Matrix{Float64}(undef, length(chunk), nb)
        _status(s, ccall((:gpf_block_history_proportion, libgpf), Cint, (Ptr{Cvoid}, Cint, Int64, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}),
                         s.handle, addr.first, block_size, addr.second, chunk, length(chunk), part))
        out[k0:k0 + length(chunk) - 1, :] = part
    end
    return vals, out
end
# returns (values, proportions): the distinct values of the column over all blocks, and a (n_values, n_blocks) Matrix; 16 values per launch
function block_proportionmap(s::DeviceParticleFilterState, block_size::Int, addr::Integer; max_values::Int=256)
    col = Vector{Float64}(undef, s.n_particles)
    _status(s, ccall((:gpf_get_column, libgpf), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Int64), s.handle, addr, col, length(col)))
    vals = sort(unique(col))
    length(vals) > max_values && error("proportionmap: $(length(vals)) distinct values; the column does not look discrete")
    nb = cld(s.n_particles, block_size)
    out = Matrix{Float64}(undef, length(vals), nb)
    for k0 in 1:16:length(vals)
        chunk = vals[k0:min(k0 + 15, length(vals))]
        part = Matrix{Float64}(undef, length(chunk), nb)
        _status(s, ccall((:gpf_block_proportion, libgpf), Cint, (Ptr{Cvoid}, Int64, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}), s.handle, block_size, addr, chunk, length(chunk), part))
        out[k0:k0 + length(chunk) - 1, :] = part
    end
    return vals, out
end
# Every block a filter on ITS OWN data: per-block initialisation / update / rejuvenation, one launch each (gpf.h gpf_initialize_blocks,
# gpf_update_blocks, gpf_rejuvenate_blocks).  observations: a (n_obs, n_blocks) Matrix -- column b for block b.
function pf_initialize_blocks(model::NativeModel, model_args::Tuple, observations::Matrix{Float64}, n_particles::Int, block_size::Int; history::Integer=0, kw...)
    state = DeviceParticleFilterState(model, n_particles; history=history, history_blocks=history > 0, kw...)    # (history = T: the block-wise store)
    size(observations, 2) == cld(n_particles, block_size) || error("one observation column per block expected")
    _status(state, ccall((:gpf_initialize_blocks, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Int64), state.handle, observations, size(observations, 1), block_size))
    return state
end
function pf_update_blocks!(s::DeviceParticleFilterState, new_args::Tuple, argdiffs::Tuple, observations::Matrix{Float64}, block_size::Int)
    size(observations, 2) == cld(s.n_particles, block_size) || error("one observation column per block expected")
    _status(s, ccall((:gpf_update_blocks, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Int64), s.handle, observations, size(observations, 1), block_size)); s
end
# Conditional SMC, the propagation half (gpf.h gpf_initialize_blocks_ref / gpf_update_blocks_ref): slot 0 of block b is pinned to reference[:, b] (a
# (dim, n_blocks) Matrix -- column b for block b) and weighted by log p(y_b | reference[:, b]); every other particle as without a reference.
function pf_initialize_blocks_ref(model::NativeModel, model_args::Tuple, observations::Matrix{Float64}, reference::Matrix{Float64}, n_particles::Int, block_size::Int; history::Integer=0, kw...)
    state = DeviceParticleFilterState(model, n_particles; history=history, history_blocks=history > 0, kw...)
    size(observations, 2) == size(reference, 2) == cld(n_particles, block_size) || error("one observation column and one reference column per block expected")
    _status(state, ccall((:gpf_initialize_blocks_ref, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Int64, Ptr{Cdouble}, Cint),
                         state.handle, observations, size(observations, 1), block_size, reference, size(reference, 1)))
    return state
end
function pf_update_blocks_ref!(s::DeviceParticleFilterState, new_args::Tuple, argdiffs::Tuple, observations::Matrix{Float64}, reference::Matrix{Float64}, block_size::Int)
    size(observations, 2) == size(reference, 2) == cld(s.n_particles, block_size) || error("one observation column and one reference column per block expected")
    _status(s, ccall((:gpf_update_blocks_ref, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Int64, Ptr{Cdouble}, Cint),
                     s.handle, observations, size(observations, 1), block_size, reference, size(reference, 1))); s
end
# every block stratified by itself (src/initialize.jl:92-109 / src/update.jl:193-210 on each sub-state), one launch; strata: the values of the model's discrete latent
function pf_initialize_blocks(model::NativeModel, model_args::Tuple, observations::Matrix{Float64}, strata::Vector{Float64}, n_particles::Int, block_size::Int; layout::Symbol=:contiguous, kw...)
    state = DeviceParticleFilterState(model, n_particles; kw...)
    size(observations, 2) == cld(n_particles, block_size) || error("one observation column per block expected")
    _status(state, ccall((:gpf_initialize_blocks_strata, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Int64, Ptr{Cdouble}, Cint, Cint),
                         state.handle, observations, size(observations, 1), block_size, strata, length(strata), layout == :interleaved ? 1 : 0))
    return state
end
function pf_update_blocks!(s::DeviceParticleFilterState, new_args::Tuple, argdiffs::Tuple, observations::Matrix{Float64}, strata::Vector{Float64}, block_size::Int; layout::Symbol=:interleaved)
    size(observations, 2) == cld(s.n_particles, block_size) || error("one observation column per block expected")
    _status(s, ccall((:gpf_update_blocks_strata, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Int64, Ptr{Cdouble}, Cint, Cint),
                     s.handle, observations, size(observations, 1), block_size, strata, length(strata), layout == :interleaved ? 1 : 0)); s
end
# "Update with different proposals per view" (test/update.jl:179-189) in one launch: use_proposal[b] = true extends block b with the model's native
# proposal (LocallyOptimal for the LG-SSM: id 1; line_model's fixed proposals: id 2), false with the default one
function pf_update_blocks!(s::DeviceParticleFilterState, new_args::Tuple, argdiffs::Tuple, observations::Matrix{Float64}, block_size::Int, use_proposal::Vector{Bool}, proposal_id::Int=1)
    size(observations, 2) == cld(s.n_particles, block_size) == length(use_proposal) || error("one observation column and one flag per block expected")
    flags = Int32.(use_proposal)
    _status(s, ccall((:gpf_update_blocks_proposal, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Int64, Ptr{Int32}, Cint), s.handle, observations, size(observations, 1), block_size, flags, proposal_id)); s
end
function pf_rejuvenate_blocks!(s::DeviceParticleFilterState, kern=nothing, kern_args::Tuple=(), n_iters::Int=1; method::Symbol=:move, only_resampled::Bool=false)
    m = method == :move ? 0 : method == :reweight ? 1 : error("Method $method not recognized.")
    _status(s, ccall((:gpf_rejuvenate_blocks, libgpf), Cint, (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{UInt64}), s.handle, m, n_iters, only_resampled ? 1 : 0, C_NULL)); s
end
# A whole series per block in ONE launch (gpf.h gpf_run_blocks): bit for bit the loop
#     for t in 1:T; pf_resample_blocks!(s, block_size, method; ess_frac, sort_particles, check=false); pf_update_blocks!(s, (t,), (nothing,), observations[:, t, :], block_size); end
# observations: (n_obs, T, n_blocks) -- block b's series in observations[:, :, b] -- or a (n_obs, T) Matrix, ONE series shared by all blocks (the
# SMC^2 / particle-marginal MH case: the blocks differ by set_block_params!).  ess_frac = nothing: every block resamples at every step.  Returns
# (lml, ess, resampled), each (n_blocks, T): block_stats after step t's update and whether block b resampled at step t.
function pf_run_blocks!(s::DeviceParticleFilterState, observations::Union{Array{Float64,3},Matrix{Float64}}, block_size::Int, method::Symbol=:multinomial;
                        ess_frac=0.5, sort_particles::Bool=true)
    m = method == :multinomial ? 0 : method == :residual ? 1 : method == :stratified ? 2 : error("Resampling method $method not recognized.")
    nb = cld(s.n_particles, min(block_size, s.n_particles)); T = size(observations, 2)
    shared = ndims(observations) == 2
    shared || size(observations, 3) == nb || error("one series per block expected: observations of size (n_obs, T, $nb)")
    ess = Matrix{Float64}(undef, nb, T); lml = Matrix{Float64}(undef, nb, T); words = Matrix{Int32}(undef, nb, T)
    invalid = Ref{Cint}(0)
    _status(s, ccall((:gpf_run_blocks, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cint, Cint, Int64, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}),
                     s.handle, observations, size(observations, 1), T, shared ? 1 : 0, block_size, m, sort_particles ? 1 : 0,
                     ess_frac === nothing ? NaN : Float64(ess_frac), ess, lml, words, invalid))
    return lml, ess, (words .& Int32(1)) .!= 0
end
# for b in blocks: the model arguments of state[b] (src/update.jl:12-25 on a sub-state with new_args_b) -- gpf.h gpf_set_block_params.  params: a
# (n_params, n_blocks) Matrix, column b = block b's parameter vector in the layout of csrc/gpf_models.hpp (derived constants included), or a
# Vector of NativeModel descriptors of the state's model; `nothing` clears them.  While set, the block-wise calls use column b for block b (this
# block_size only) and every call that would use the state's own parameters fails.
function set_block_params!(s::DeviceParticleFilterState, params::Matrix{Float64}, block_size::Int)
    size(params, 2) == cld(s.n_particles, min(block_size, s.n_particles)) || error("one parameter column per block expected")
    _status(s, ccall((:gpf_set_block_params, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Int64), s.handle, params, size(params, 1), block_size)); s
end
function set_block_params!(s::DeviceParticleFilterState, models::Vector{NativeModel}, block_size::Int)
    all(m -> m.id == s.model.id, models) || error("per-block parameters: descriptors of another model")
    allequal(length.(getfield.(models, :params))) || error("per-block parameters: the descriptors' parameter vectors differ in length")
    set_block_params!(s, reduce(hcat, getfield.(models, :params)), block_size)
end
function set_block_params!(s::DeviceParticleFilterState, ::Nothing, block_size::Int=0)
    _status(s, ccall((:gpf_set_block_params, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Int64), s.handle, C_NULL, 0, block_size)); s
end
"the per-block parameters as they stand, a (n_params, n_blocks) Matrix (gpf.h gpf_get_block_params): after pf_resample_across_blocks! permuted by its ancestors"
function get_block_params(s::DeviceParticleFilterState, block_size::Int)
    out = Matrix{Float64}(undef, length(s.model.params), cld(s.n_particles, min(block_size, s.n_particles)))
    _status(s, ccall((:gpf_get_block_params, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Int64), s.handle, out, size(out, 1), size(out, 2)))
    return out
end
# Resampling ACROSS blocks -- the outer level of SMC^2, a nested or an island filter (gpf.h gpf_resample_across_blocks): every block is one
# super-particle with the log-weight log_ml_estimate(state[b]); the blocks are resampled by the reference's resampler (src/resample.jl:19-175) on
# those weights and whole filters are copied -- rows, parents, per-block parameters and observations, log-weights + (M - L[a]).  Returns the
# 1-based block ancestors A (theta = theta[A]), or nothing when the ESS gate did not fire.
function pf_resample_across_blocks!(s::DeviceParticleFilterState, block_size::Int, method::Symbol=:multinomial;
                                    ess_frac=nothing, sort_particles::Bool=true, check=:warn)
    m = method == :multinomial ? 0 : method == :residual ? 1 : method == :stratified ? 2 : error("Resampling method $method not recognized.")
    chk = check === true ? 2 : (check === :warn ? 1 : 0)
    invalid = Ref{Cint}(0); resampled = Ref{Cint}(0); ess = Ref{Cdouble}(0.0)
    st = ccall((:gpf_resample_across_blocks, libgpf), Cint, (Ptr{Cvoid}, Cint, Int64, Cint, Cdouble, Cint, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}),
               s.handle, m, block_size, sort_particles ? 1 : 0, ess_frac === nothing ? NaN : Float64(ess_frac), chk, invalid, resampled, ess)
    _status(s, st)
    check === :warn && invalid[] != 0 && @warn("Invalid block weights (all -Inf): blocks resampled with uniform weights.")
    return resampled[] != 0 ? block_ancestors(s, block_size) : nothing
end
"the 1-based block ancestors of the last pf_resample_across_blocks! that fired"
function block_ancestors(s::DeviceParticleFilterState, block_size::Int)
    out = Vector{Int64}(undef, cld(s.n_particles, block_size))
    _status(s, ccall((:gpf_block_ancestors, libgpf), Cint, (Ptr{Cvoid}, Ptr{Int64}), s.handle, out))
    return out
end
"which blocks the last pf_resample_blocks! resampled"
function block_resampled(s::DeviceParticleFilterState, block_size::Int)
    out = Vector{Cint}(undef, cld(s.n_particles, block_size))
    _status(s, ccall((:gpf_block_resampled, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cint}), s.handle, out))
    return out .!= 0
end

# src/rejuvenate.jl:18-90 with the native kernels (Gen.mh / move_reweight on the current step's latent)
function pf_rejuvenate!(s::DeviceParticleFilterState, kern=nothing, kern_args::Tuple=(), n_iters::Int=1; method::Symbol=:move)
    m = method == :move ? 0 : method == :reweight ? 1 : error("Method $method not recognized.")
    _status(s, ccall((:gpf_rejuvenate, libgpf), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{UInt64}), s.handle, m, n_iters, C_NULL))
    return s
end
# move_reweight(trace, proposal, proposal_args) (src/rejuvenate.jl:134-148) with a native proposal:
#   MoveProposal(1, Float64[])                      the LG-SSM's locally optimal proposal of x_t
#   MoveProposal(2, [q, log(q), log1p(-q)])         line_model: outlier ~ bernoulli(q), the outlier_propose of test/rejuvenate.jl:19-27
struct MoveProposal; id::Int; params::Vector{Float64}; end
function pf_move_reweight!(s::DeviceParticleFilterState, kern, kern_args::Tuple{MoveProposal,Vararg}, n_iters::Int=1)
    mp = kern_args[1]
    _status(s, ccall((:gpf_rejuvenate_proposal, libgpf), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Cint, Cint), s.handle, mp.id, mp.params, length(mp.params), n_iters))
    return s
end
# pf_move_accept!(state, mh, (proposal, proposal_args...), n_iters) (src/rejuvenate.jl:40-53 with Gen.mh(trace, proposal, proposal_args)): the same
# native proposals, accepted iff log(rand()) < weight - fwd_score + bwd_score
function pf_move_accept!(s::DeviceParticleFilterState, kern, kern_args::Tuple{MoveProposal,Vararg}, n_iters::Int=1)
    mp = kern_args[1]
    _status(s, ccall((:gpf_rejuvenate_with_proposal, libgpf), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cint, Cint, Ptr{UInt64}),
                     s.handle, 0, mp.id, mp.params, length(mp.params), n_iters, Ptr{UInt64}(C_NULL)))
    return s
end
pf_move_accept!(s::DeviceParticleFilterState, kern=nothing, kern_args::Tuple=(), n_iters::Int=1) = pf_rejuvenate!(s, kern, kern_args, n_iters; method=:move)
pf_move_reweight!(s::DeviceParticleFilterState, kern=nothing, kern_args::Tuple=(), n_iters::Int=1) = pf_rejuvenate!(s, kern, kern_args, n_iters; method=:reweight)

# src/resize.jl:16-124, 236-297 -- the handle stays valid, its buffers are reallocated
function _refresh!(s)
    n = Ref{Int64}(0); _status(s, ccall((:gpf_n_particles, libgpf), Cint, (Ptr{Cvoid}, Ref{Int64}), s.handle, n)); s.n_particles = n[]; s
end
function _resize!(s, n::Int, method::Int, priority_fn, check_kw)
    chk = check_kw === true ? 2 : (check_kw === :warn ? 1 : 0)
    alpha = priority_fn === nothing ? NaN : (priority_fn::Tempering).alpha
    invalid = Ref{Cint}(0)
    _status(s, ccall((:gpf_resize, libgpf), Cint, (Ptr{Cvoid}, Int64, Cint, Cdouble, Cint, Ref{Cint}), s.handle, n, method, alpha, chk, invalid))
    check_kw === :warn && invalid[] != 0 && @warn("Invalid weights: resampled with uniform weights.")
    _refresh!(s)
end
pf_multinomial_resize!(s::DeviceParticleFilterState, n::Int; priority_fn=nothing, check=:warn) = _resize!(s, n, 0, priority_fn, check)
pf_residual_resize!(s::DeviceParticleFilterState, n::Int; priority_fn=nothing, check=:warn) = _resize!(s, n, 1, priority_fn, check)
pf_optimal_resize!(s::DeviceParticleFilterState, n::Int; check=:warn) = _resize!(s, n, 3, nothing, check)        # src/resize.jl:149-200
function pf_resize!(s::DeviceParticleFilterState, n::Int, method::Symbol=:multinomial; kwargs...)
    method == :multinomial && return pf_multinomial_resize!(s, n; kwargs...)
    method == :residual && return pf_residual_resize!(s, n; kwargs...)
    method == :optimal && return pf_optimal_resize!(s, n; kwargs...)
    error("Resampling method $method not recognized.")
end
function pf_replicate!(s::DeviceParticleFilterState, k::Int; layout::Symbol=:contiguous)
    _status(s, ccall((:gpf_replicate, libgpf), Cint, (Ptr{Cvoid}, Cint, Cint), s.handle, k, layout != :contiguous)); _refresh!(s)
end
function pf_dereplicate!(s::DeviceParticleFilterState, k::Int; layout::Symbol=:contiguous, method::Symbol=:keepfirst)
    _status(s, ccall((:gpf_dereplicate, libgpf), Cint, (Ptr{Cvoid}, Cint, Cint, Cint), s.handle, k, layout != :contiguous, method == :sample)); _refresh!(s)
end
# src/resize.jl:309-334 (gpf.h gpf_coalesce): by = get_choices / identity -> every state column; a column or a tuple of columns of the current step
# (0-based, as gpf_get_column).  Groups come out in ascending order of first occurrence.
function pf_coalesce!(s::DeviceParticleFilterState; by=get_choices)
    mask = UInt64(0)
    if !(by === get_choices || by === identity)
        cols = by isa Integer ? (by,) : by
        (cols isa Tuple && !isempty(cols) && all(c -> c isa Integer && 0 <= c < s.model.dim, cols)) ||
            error("native coalescing accepts by = get_choices / identity, a current-step column or a tuple of current-step columns")
        for c in cols; mask |= UInt64(1) << c; end
    end
    n_new = Ref{Int64}(0)
    _status(s, ccall((:gpf_coalesce, libgpf), Cint, (Ptr{Cvoid}, UInt64, Ref{Int64}), s.handle, mask, n_new))
    _refresh!(s)
end
# src/resize.jl:351-421 (gpf.h gpf_introduce): observations = one column per step 1..t (obs_dim x t); the proposal (native id, 0 = none)
# applies at the last step.  model / model_args are the state's own.
function _introduce!(s::DeviceParticleFilterState, model, observations::AbstractMatrix{<:Real}, proposal_id::Integer, n::Int)
    model === nothing || (model.id == s.model.id && model.params == s.model.params) ||
        error("pf_introduce!: a device filter introduces particles of its own model")
    obs = Matrix{Float64}(observations)                          # column-major: step e's data vector is column e, i.e. [t][obs_dim] row-major
    _status(s, ccall((:gpf_introduce, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cint, Int64, Cint),
                     s.handle, obs, size(obs, 1), size(obs, 2), n, proposal_id))
    _refresh!(s)
end
_steps(observations::AbstractVector{<:Real}) = reshape(Vector{Float64}(observations), :, 1)
_steps(observations::AbstractMatrix{<:Real}) = observations
_proposal_id(::LocallyOptimal) = 1
_proposal_id(id::Integer) = id                                  # 2: line_model's fixed proposals (GPF_PROPOSAL_LINE_FIXED)
pf_introduce!(s::DeviceParticleFilterState, observations::AbstractVecOrMat, n::Int) = _introduce!(s, nothing, _steps(observations), 0, n)
pf_introduce!(s::DeviceParticleFilterState, model::NativeModel, model_args::Tuple, observations::AbstractVecOrMat, n::Int) =
    _introduce!(s, model, _steps(observations), 0, n)
pf_introduce!(s::DeviceParticleFilterState, observations::AbstractVecOrMat, proposal, proposal_args::Tuple, n::Int) =
    _introduce!(s, nothing, _steps(observations), _proposal_id(proposal), n)
pf_introduce!(s::DeviceParticleFilterState, model::NativeModel, model_args::Tuple, observations::AbstractVecOrMat, proposal, proposal_args::Tuple, n::Int) =
    _introduce!(s, model, _steps(observations), _proposal_id(proposal), n)

# src/utils.jl:148-186
function _scalar(s, sym)
    out = Ref{Cdouble}(0)
    _status(s, ccall((sym, libgpf), Cint, (Ptr{Cvoid}, Ref{Cdouble}), s.handle, out))
    return out[]
end
function _vector(s, sym)
    out = Vector{Float64}(undef, s.n_particles)
    _status(s, ccall((sym, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Int64), s.handle, out, length(out)))
    return out
end
effective_sample_size(s::DeviceParticleFilterState) = _scalar(s, :gpf_effective_sample_size)
get_ess(s::DeviceParticleFilterState) = effective_sample_size(s)
log_ml_estimate(s::DeviceParticleFilterState) = _scalar(s, :gpf_log_ml_estimate)
get_lml_est(s::DeviceParticleFilterState) = log_ml_estimate(s)
get_log_weights(s::DeviceParticleFilterState) = _vector(s, :gpf_get_log_weights)
get_log_norm_weights(s::DeviceParticleFilterState) = _vector(s, :gpf_get_log_norm_weights)
get_norm_weights(s::DeviceParticleFilterState) = _vector(s, :gpf_get_norm_weights)

# state.parents (test/resample.jl:11)
function Base.getproperty(s::DeviceParticleFilterState, name::Symbol)
    if name === :parents
        out = Vector{Int64}(undef, getfield(s, :n_particles))
        _status(s, ccall((:gpf_get_parents, libgpf), Cint, (Ptr{Cvoid}, Ptr{Int64}, Int64), getfield(s, :handle), out, length(out)))
        return out
    elseif name === :log_weights
        return get_log_weights(s)
    end
    return getfield(s, name)
end

# src/statistics.jl:13-14, 48-50 -- addr = column of the current-step latent (0-based)
function mean(s::DeviceParticleFilterState, addr::Integer)
    out = Ref{Cdouble}(0); _status(s, ccall((:gpf_mean, libgpf), Cint, (Ptr{Cvoid}, Cint, Ref{Cdouble}), s.handle, addr, out)); out[]
end
function var(s::DeviceParticleFilterState, addr::Integer)
    out = Ref{Cdouble}(0); _status(s, ccall((:gpf_var, libgpf), Cint, (Ptr{Cvoid}, Cint, Ref{Cdouble}), s.handle, addr, out)); out[]
end

# past choices along the surviving ancestry, README.md:97-104: mean(state, 5 => 0) == mean(state, 5 => :moving)
# (needs the trajectory store: gpf_history_enable before pf_initialize)
function mean(s::DeviceParticleFilterState, addr::Pair{<:Integer,<:Integer})
    out = Ref{Cdouble}(0); _status(s, ccall((:gpf_history_mean, libgpf), Cint, (Ptr{Cvoid}, Cint, Cint, Ref{Cdouble}), s.handle, addr.first, addr.second, out)); out[]
end
function var(s::DeviceParticleFilterState, addr::Pair{<:Integer,<:Integer})
    out = Ref{Cdouble}(0); _status(s, ccall((:gpf_history_var, libgpf), Cint, (Ptr{Cvoid}, Cint, Cint, Ref{Cdouble}), s.handle, addr.first, addr.second, out)); out[]
end

# stratified initialisation / update (src/initialize.jl:92-109, src/update.jl:193-210): strata = values of the model's discrete latent
function pf_initialize(model::NativeModel, args::Tuple, obs::Vector{Float64}, strata::Vector{Float64}, n::Int; layout::Symbol=:contiguous, kwargs...)
    s = DeviceParticleFilterState(model, n; kwargs...)
    _status(s, ccall((:gpf_initialize_strata, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Cint),
                   s.handle, obs, length(obs), strata, length(strata), layout != :contiguous)); s
end
# ... with a native proposal for the model's other choice (src/initialize.jl:111-129; line_model + LineFixed: test/initialize.jl:66-90)
function pf_initialize(model::NativeModel, args::Tuple, obs::Vector{Float64}, strata::Vector{Float64}, proposal_id::Int, proposal_args::Tuple, n::Int;
                       layout::Symbol=:contiguous, kwargs...)
    s = DeviceParticleFilterState(model, n; kwargs...)
    _status(s, ccall((:gpf_initialize_strata_proposal, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Cint, Cint),
                   s.handle, obs, length(obs), strata, length(strata), layout != :contiguous, proposal_id)); s
end
function pf_update!(s::DeviceParticleFilterState, new_args::Tuple, argdiffs::Tuple, obs::Vector{Float64}, strata::Vector{Float64}; layout::Symbol=:interleaved)
    _status(s, ccall((:gpf_update_strata, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Cint),
                   s.handle, obs, length(obs), strata, length(strata), layout != :contiguous)); s
end

# Gen.sample_unweighted_traces(state, n) (src/utils.jl:189-194): rows of the drawn particles (n x row_width) and their indices
function sample_unweighted_traces(s::DeviceParticleFilterState, n::Int)
    dim = Ref{Cint}(0); w = Ref{Cint}(0)
    _status(s, ccall((:gpf_state_dim, libgpf), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Cint}), s.handle, dim, w))
    rows = Matrix{Float64}(undef, w[], n); idx = Vector{Int64}(undef, n)
    _status(s, ccall((:gpf_sample_unweighted, libgpf), Cint, (Ptr{Cvoid}, Int64, Ptr{Cdouble}, Ptr{Int64}), s.handle, n, rows, idx))
    permutedims(rows)[:, 1:dim[]], idx
end

# Whole trajectories per block: for b in blocks; sample_unweighted_traces(state[b], n); end (src/utils.jl:7,189-194 on sub-states, src/view.jl:35-48) in one
# launch from the block-wise trajectory store (gpf.h gpf_block_sample_trajectories).  steps = lo:hi, 1-based (default: every recorded step).  Returns the
# paths as a (dim, n_steps, n, n_blocks) array -- [c, s - lo + 1, j, b] = trace[s => c] of draw j of block b -- and the (n, n_blocks) indices of the
# drawn particles inside their blocks (0 for a block with NaN weights, whose paths are NaN).  Advances the RNG epoch once.
function block_sample_trajectories(s::DeviceParticleFilterState, block_size::Int, n::Int=1; steps::Union{Nothing,UnitRange{Int}}=nothing)
    if steps === nothing
        k = Ref{Cint}(0)
        _status(s, ccall((:gpf_history_steps, libgpf), Cint, (Ptr{Cvoid}, Ref{Cint}), s.handle, k))
        steps = 1:Int(k[])
    end
    nb = cld(s.n_particles, min(block_size, s.n_particles)); d = _latent_dim(s)
    traj = Array{Float64}(undef, d, length(steps), n, nb); idx = Matrix{Int64}(undef, n, nb)
    _status(s, ccall((:gpf_block_sample_trajectories, libgpf), Cint, (Ptr{Cvoid}, Int64, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Int64}),
                     s.handle, block_size, n, first(steps), last(steps), traj, idx))
    return traj, idx
end

# Backward simulation per block (gpf.h gpf_block_backward_sample): the step-T draw of block_sample_trajectories, then every earlier step re-drawn from the
# step's recorded weights times the transition density -- one launch.  Needs pf_initialize_blocks(...; history=T, history_weights=true).  Returns the paths
# as a (dim, n_steps, n, n_blocks) array and the (n_steps, n, n_blocks) 1-based GLOBAL indices of the held particles in the final order of their steps
# (0 for a block with NaN weights, whose paths are NaN).  Advances the RNG epoch by T - first(steps) + 1.
function block_backward_trajectories(s::DeviceParticleFilterState, block_size::Int, n::Int=1; steps::Union{Nothing,UnitRange{Int}}=nothing)
    if steps === nothing
        k = Ref{Cint}(0)
        _status(s, ccall((:gpf_history_steps, libgpf), Cint, (Ptr{Cvoid}, Ref{Cint}), s.handle, k))
        steps = 1:Int(k[])
    end
    nb = cld(s.n_particles, min(block_size, s.n_particles)); d = _latent_dim(s)
    traj = Array{Float64}(undef, d, length(steps), n, nb); idx = Array{Int64}(undef, length(steps), n, nb)
    _status(s, ccall((:gpf_block_backward_sample, libgpf), Cint, (Ptr{Cvoid}, Int64, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Int64}),
                     s.handle, block_size, n, first(steps), last(steps), traj, idx))
    return traj, idx
end

# Marginal smoothing per block (gpf.h gpf_block_smooth; FFBSm): deterministic smoothing weights of every particle of every step, and the smoothed mean and
# variance of every latent column under them -- one launch, nothing drawn, the epoch stays.  Needs pf_initialize_blocks(...; history=T,
# history_weights=true).  Returns (mean, var) as (dim, n_steps, n_blocks) arrays, then on request the weights (block_size, n_steps, n_blocks) and the
# (n_steps, n_blocks) 1-based blocks the lineages occupied (0 and NaN where a lineage is undefined or the block's weights are NaN).
function block_smoothed_moments(s::DeviceParticleFilterState, block_size::Int; steps::Union{Nothing,UnitRange{Int}}=nothing,
                                return_weights::Bool=false, return_blocks::Bool=false)
    if steps === nothing
        k = Ref{Cint}(0)
        _status(s, ccall((:gpf_history_steps, libgpf), Cint, (Ptr{Cvoid}, Ref{Cint}), s.handle, k))
        steps = 1:Int(k[])
    end
    bs = min(block_size, s.n_particles); nb = cld(s.n_particles, bs); d = _latent_dim(s)
    mu = Array{Float64}(undef, d, length(steps), nb); s2 = Array{Float64}(undef, d, length(steps), nb)
    w = return_weights ? Array{Float64}(undef, bs, length(steps), nb) : nothing
    blocks = return_blocks ? Array{Int64}(undef, length(steps), nb) : nothing
    _status(s, ccall((:gpf_block_smooth, libgpf), Cint, (Ptr{Cvoid}, Int64, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int64}),
                     s.handle, block_size, first(steps), last(steps), mu, s2, return_weights ? w : C_NULL, return_blocks ? blocks : C_NULL))
    return (mu, s2, (return_weights ? (w,) : ())..., (return_blocks ? (blocks,) : ())...)
end
function block_smoothed_weights(s::DeviceParticleFilterState, block_size::Int; steps::Union{Nothing,UnitRange{Int}}=nothing)
    if steps === nothing
        k = Ref{Cint}(0)
        _status(s, ccall((:gpf_history_steps, libgpf), Cint, (Ptr{Cvoid}, Ref{Cint}), s.handle, k))
        steps = 1:Int(k[])
    end
    bs = min(block_size, s.n_particles); nb = cld(s.n_particles, bs)
    w = Array{Float64}(undef, bs, length(steps), nb)
    _status(s, ccall((:gpf_block_smooth, libgpf), Cint, (Ptr{Cvoid}, Int64, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int64}),
                     s.handle, block_size, first(steps), last(steps), C_NULL, C_NULL, w, C_NULL))
    return w
end

# Pairwise smoothing per block (gpf.h gpf_block_smooth_pairs): the E-step of particle EM -- block_smoothed_moments' mean (dim, n_steps, n_blocks), the
# second moments sum_i W_s^i x_s^i x_s^i' and the lag-one cross moments E[x_s x_{s+1}' | y_1:T] under the pairwise smoothing weights, in one launch.
# The library writes row-major [n_blocks][n_steps][a][c]: second is (dim, dim, n_steps, n_blocks) with second[c, a, s, b] (symmetric), and
# cross[c, a, o, b] = E[x_s[a] x_{s+1}[c]] for s = first(steps) + o - 1, (dim, dim, n_steps - 1, n_blocks) -- empty for a single step.
function block_smoothed_pair_moments(s::DeviceParticleFilterState, block_size::Int; steps::Union{Nothing,UnitRange{Int}}=nothing,
                                     return_blocks::Bool=false)
    if steps === nothing
        k = Ref{Cint}(0)
        _status(s, ccall((:gpf_history_steps, libgpf), Cint, (Ptr{Cvoid}, Ref{Cint}), s.handle, k))
        steps = 1:Int(k[])
    end
    bs = min(block_size, s.n_particles); nb = cld(s.n_particles, bs); d = _latent_dim(s)
    mu = Array{Float64}(undef, d, length(steps), nb); second = Array{Float64}(undef, d, d, length(steps), nb)
    cross = Array{Float64}(undef, d, d, length(steps) - 1, nb)
    blocks = return_blocks ? Array{Int64}(undef, length(steps), nb) : nothing
    _status(s, ccall((:gpf_block_smooth_pairs, libgpf), Cint, (Ptr{Cvoid}, Int64, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int64}),
                     s.handle, block_size, first(steps), last(steps), mu, second, length(steps) > 1 ? cross : C_NULL, return_blocks ? blocks : C_NULL))
    return (mu, second, cross, (return_blocks ? (blocks,) : ())...)
end

# The most probable path per block (gpf.h gpf_block_map_path; particle Viterbi, Godsill, Doucet & West 2001): max-plus dynamic programming over the
# particles of the block's lineage at every recorded step -- one launch, nothing drawn, the epoch stays.  Needs pf_initialize_blocks(...; history=T,
# history_weights=true).  Returns the paths (dim, n_steps, n_blocks), then on request the (n_steps, n_blocks) 1-based GLOBAL indices of their particles and
# the (n_blocks) maxima (comparable within a block, not a normalised density).  NaN and 0 where a lineage is undefined or no path has positive density.
function block_map_trajectories(s::DeviceParticleFilterState, block_size::Int; steps::Union{Nothing,UnitRange{Int}}=nothing,
                                return_indices::Bool=false, return_log_density::Bool=false)
    if steps === nothing
        k = Ref{Cint}(0)
        _status(s, ccall((:gpf_history_steps, libgpf), Cint, (Ptr{Cvoid}, Ref{Cint}), s.handle, k))
        steps = 1:Int(k[])
    end
    bs = min(block_size, s.n_particles); nb = cld(s.n_particles, bs); d = _latent_dim(s)
    path = Array{Float64}(undef, d, length(steps), nb)
    idx = return_indices ? Array{Int64}(undef, length(steps), nb) : nothing
    logp = return_log_density ? Array{Float64}(undef, nb) : nothing
    _status(s, ccall((:gpf_block_map_path, libgpf), Cint, (Ptr{Cvoid}, Int64, Cint, Cint, Ptr{Cdouble}, Ptr{Int64}, Ptr{Cdouble}),
                     s.handle, block_size, first(steps), last(steps), path, return_indices ? idx : C_NULL, return_log_density ? logp : C_NULL))
    return (return_indices || return_log_density) ? (path, (return_indices ? (idx,) : ())..., (return_log_density ? (logp,) : ())...) : path
end

# Forward-only smoothing per block (gpf.h gpf_block_forward_moments; needs pf_initialize_blocks(...; forward=true)): after the current step t, the sums
# over steps of block_smoothed_pair_moments without a store -- sum = sum_s E[x_s | y_1:t] and first = E[x_1 | y_1:t] as (dim, n_blocks); second =
# sum_s E[x_s x_s' | y_1:t], first2, last2 = E[x_t x_t' | y_1:t] (symmetric) and cross as (dim, dim, n_blocks) with cross[c, a, b] = sum_s E[x_s[a]
# x_{s+1}[c] | y_1:t] (the library writes row-major [n_blocks][a][c]) -- and t.  The M-step reads second - last2, second - first2 and cross.
function block_forward_moments(s::DeviceParticleFilterState, block_size::Int)
    bs = min(block_size, s.n_particles); nb = cld(s.n_particles, bs); d = _latent_dim(s)
    sum_ = Array{Float64}(undef, d, nb); first_ = Array{Float64}(undef, d, nb)
    second = Array{Float64}(undef, d, d, nb); cross = Array{Float64}(undef, d, d, nb)
    first2 = Array{Float64}(undef, d, d, nb); last2 = Array{Float64}(undef, d, d, nb)
    t = Ref{Cint}(0)
    _status(s, ccall((:gpf_block_forward_moments, libgpf), Cint, (Ptr{Cvoid}, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Cint}),
                     s.handle, block_size, sum_, second, cross, first_, first2, last2, t))
    return (sum=sum_, second=second, cross=cross, first=first_, first2=first2, last2=last2, n_steps=Int(t[]))
end

# ---------------------------------------------------------------- multi-GPU: one process per GPU, the exchange inside libgpf
# A shard of a filter of `n_global` particles: rank r of `world` holds the contiguous global range that starts at gid0 (the
# first n_global % world ranks hold one particle more).  The communicator is libgpf's own (RCCL); the host only carries the
# 128-byte id from rank 0 to the others, e.g.  id = MPI.bcast(rank == 0 ? comm_unique_id() : nothing, 0, comm).
mutable struct ShardedDeviceParticleFilterState
    handle::Ptr{Cvoid}
    model::NativeModel
    n_particles::Int          # this shard
    n_global::Int
    rank::Int
    world::Int
end
function comm_unique_id()
    id = Vector{UInt8}(undef, 128)
    ccall((:gpf_comm_unique_id, libgpf), Cint, (Ptr{UInt8},), id) == 0 || error("gpf_comm_unique_id failed")
    return id
end
function pf_initialize(model::NativeModel, model_args::Tuple, observations::Vector{Float64}, n_global::Int, id::Vector{UInt8},
                       rank::Int, world::Int; seed::Integer=1, keep_prev::Bool=false, device::Integer=0)
    base, extra = divrem(n_global, world)
    n = base + (rank < extra ? 1 : 0); gid0 = rank * base + min(rank, extra)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve model begin
        cfg = Ref(GpfConfig(GPF_ABI_VERSION, model.id, length(model.params), keep_prev, pointer(model.params),
                            n, n_global, gid0, UInt64(seed), device, 0, C_NULL))
        ccall((:gpf_create, libgpf), Cint, (Ref{GpfConfig}, Ref{Ptr{Cvoid}}), cfg, h) == 0 ||
            error(unsafe_string(ccall((:gpf_last_error, libgpf), Cstring, (Ptr{Cvoid},), C_NULL)))
    end
    s = ShardedDeviceParticleFilterState(h[], model, n, n_global, rank, world)
    finalizer(x -> ccall((:gpf_destroy, libgpf), Cint, (Ptr{Cvoid},), x.handle), s)
    _status(s, ccall((:gpf_comm_create, libgpf), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Cint, Cint), s.handle, id, rank, world))
    _status(s, ccall((:gpf_initialize, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint), s.handle, observations, length(observations)))
    return s
end
function pf_update!(s::ShardedDeviceParticleFilterState, new_args::Tuple, argdiffs::Tuple, observations::Vector{Float64})
    _status(s, ccall((:gpf_update, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint), s.handle, observations, length(observations))); s
end
function pf_rejuvenate!(s::ShardedDeviceParticleFilterState, kern=nothing, kern_args::Tuple=(), n_iters::Int=1; method::Symbol=:move)
    m = method == :move ? 0 : method == :reweight ? 1 : error("Method $method not recognized.")
    _status(s, ccall((:gpf_rejuvenate, libgpf), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{UInt64}), s.handle, m, n_iters, C_NULL)); s
end
# src/resample.jl:19-30 over all shards: ONE call, every collective issued by the library.
# local_only = true: the communication-free "island" resample, pf_resample!(state[shard range], method) on every shard
# (sub-state semantics, src/resample.jl:185-187,205-218), also one call (gpf_resample_local).
function pf_resample!(s::ShardedDeviceParticleFilterState, method::Symbol=:multinomial; check=:warn, sort_particles::Bool=false,
                      local_only::Bool=false, priority_alpha::Union{Nothing,Float64}=nothing)   # priority_fn = w -> priority_alpha * w
    m = method == :multinomial ? 0 : method == :residual ? 1 : method == :stratified ? 2 :
        method == :multinomial_sorted ? 4 : error("Resampling method $method not recognized.")    # (:multinomial_sorted: the opt-in extension, boundary slabs instead of (G-1)/G of all rows)
    chk = check === true ? 2 : (check === :warn ? 1 : 0)
    invalid = Ref{Cint}(0)
    # check = false: NULL for `invalid` keeps the call fully asynchronous (a non-NULL pointer makes the library poll the weight flags)
    inv_ptr = check === false ? Ptr{Cint}(C_NULL) : Base.unsafe_convert(Ptr{Cint}, invalid)
    st = GC.@preserve invalid (local_only ?
        ccall((:gpf_resample_local, libgpf), Cint, (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cint}), s.handle, m, sort_particles ? 1 : 0, chk, inv_ptr) :
        (method == :stratified && sort_particles ?   # the reference's default order of the strata (src/resample.jl:145,156-157): the replicated plan
            (priority_alpha === nothing ? ccall((:gpf_shard_resample_sorted, libgpf), Cint, (Ptr{Cvoid}, Cint, Ptr{Cint}), s.handle, chk, inv_ptr) :
                error("sort_particles = true with a priority_fn is not available across shards")) :
         priority_alpha === nothing ?
            ccall((:gpf_shard_resample, libgpf), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Cint}), s.handle, m, chk, inv_ptr) :
            ccall((:gpf_shard_resample_tempered, libgpf), Cint, (Ptr{Cvoid}, Cint, Cdouble, Cint, Ptr{Cint}), s.handle, m, priority_alpha, chk, inv_ptr)))
    _status(s, st)
    check === :warn && invalid[] != 0 && @warn("Invalid weights: resampled with uniform weights.")
    return s
end
"one iteration of the README loop on the sharded filter, every rank calls it (gpf.h gpf_shard_step_ess; the unsharded pf_step_ess! with the GLOBAL effective sample size)"
function pf_step_ess!(s::ShardedDeviceParticleFilterState, new_args::Tuple, argdiffs::Tuple, observations::Vector{Float64}; ess_threshold::Real=0.5,
                      method::Symbol=:multinomial, rejuvenate::Union{Nothing,Symbol}=nothing, n_iters::Int=1, check=:warn)
    mid = method == :multinomial ? 0 : method == :residual ? 1 : method == :stratified ? 2 : method == :multinomial_sorted ? 4 : error("Resampling method $method not recognized.")
    rid = rejuvenate === nothing ? -1 : rejuvenate == :move ? 0 : rejuvenate == :reweight ? 1 : error("Method $rejuvenate not recognized.")
    chk = check === true ? 2 : (check === :warn ? 1 : 0)
    resampled = Ref{Cint}(0); invalid = Ref{Cint}(0)
    GC.@preserve resampled invalid begin
        st = ccall((:gpf_shard_step_ess, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cdouble, Cint, Cint, Cint, Cint, Ptr{Cint}, Ptr{Cint}),
                   s.handle, observations, length(observations), Float64(ess_threshold), mid, chk, rid, n_iters,
                   Base.unsafe_convert(Ptr{Cint}, resampled), chk == 0 ? Ptr{Cint}(C_NULL) : Base.unsafe_convert(Ptr{Cint}, invalid))
    end
    _status(s, st)
    check === :warn && invalid[] != 0 && @warn("Invalid weights: resampled with uniform weights.")
    return resampled[] != 0
end
"""exchange plan of the i.i.d. resamplers across shards: :push (default) or :pull (gpf.h gpf_comm_set_plan); the same on every rank"""
function shard_plan!(s::ShardedDeviceParticleFilterState, plan::Symbol)
    plan in (:push, :pull) || error("exchange plan :$plan: :push or :pull")
    _status(s, ccall((:gpf_comm_set_plan, libgpf), Cint, (Ptr{Cvoid}, Cint), s.handle, plan == :pull ? 1 : 0)); s
end
"(calls, entries sent to other ranks, entries received from other ranks, bytes per entry) of this rank's sharded resamples so far (gpf.h gpf_comm_traffic)"
function shard_traffic(s::ShardedDeviceParticleFilterState; reset::Bool=false)
    out = zeros(Int64, 4)
    _status(s, ccall((:gpf_comm_traffic, libgpf), Cint, (Ptr{Cvoid}, Ptr{Int64}, Cint), s.handle, out, reset ? 1 : 0))
    (out[1], out[2], out[3], out[4])
end
function shard_plan(s::ShardedDeviceParticleFilterState)
    p = Ref{Cint}(0)
    _status(s, ccall((:gpf_comm_plan, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cint}), s.handle, p))
    p[] == 1 ? :pull : :push
end
"""how the rows of the resamplers with ascending targets (:stratified with sort_particles = false, the opt-in sorted multinomial) cross shards: :p2p = peer
stores into the destination ranks' slot-addressed receive windows (no host wait, no ncclGroup; the default where the mailboxes are up), :rccl = packed
entries through grouped ncclSend / ncclRecv (gpf.h gpf_comm_set_exchange); the same on every rank"""
function shard_exchange!(s::ShardedDeviceParticleFilterState, mode::Symbol)
    mode in (:p2p, :rccl, :p2p_all) || error("exchange mode :$mode: :p2p, :p2p_all or :rccl")
    _status(s, ccall((:gpf_comm_set_exchange, libgpf), Cint, (Ptr{Cvoid}, Cint), s.handle, mode == :rccl ? 0 : (mode == :p2p ? 1 : 2))); s
end
function shard_exchange(s::ShardedDeviceParticleFilterState)
    m = Ref{Cint}(0)
    _status(s, ccall((:gpf_comm_exchange, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cint}), s.handle, m))
    m[] == 0 ? :rccl : (m[] == 1 ? :p2p : :p2p_all)
end
"(us per grouped exchange of `entries` packed entries with every peer, GB/s per link, us per mailbox round, us of an empty launch) on this machine (gpf.h gpf_comm_calibrate; collective)"
function shard_calibrate(s::ShardedDeviceParticleFilterState, entries::Integer; reps::Integer=20)
    out = zeros(Float64, 4)
    _status(s, ccall((:gpf_comm_calibrate, libgpf), Cint, (Ptr{Cvoid}, Int64, Cint, Ptr{Cdouble}), s.handle, entries, reps, out))
    (out[1], out[2], out[3], out[4])
end
"per-phase microseconds of the sharded resamples since `shard_phase_timing!(s, true)` (gpf.h gpf_phase_times): summaries, plan, pack, host wait, exchange, commit + propagate"
shard_phase_timing!(s::ShardedDeviceParticleFilterState, on::Bool) = (_status(s, ccall((:gpf_phase_timing, libgpf), Cint, (Ptr{Cvoid}, Cint), s.handle, on ? 1 : 0)); s)
function shard_phase_times(s::ShardedDeviceParticleFilterState)
    us = zeros(Float64, 6); n = Ref{Int64}(0)
    _status(s, ccall((:gpf_phase_times, libgpf), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ref{Int64}), s.handle, us, n))
    (us, n[])
end
effective_sample_size(s::ShardedDeviceParticleFilterState) = _scalar(s, :gpf_shard_effective_sample_size)
get_ess(s::ShardedDeviceParticleFilterState) = effective_sample_size(s)
log_ml_estimate(s::ShardedDeviceParticleFilterState) = _scalar(s, :gpf_shard_log_ml_estimate)
get_lml_est(s::ShardedDeviceParticleFilterState) = log_ml_estimate(s)

end # module
